// nw_conn_time.hip — over-time connectivity (nw_execute_conn_time): the complex rows of a chunk of
// epochs x channels reduced along the SAMPLE axis into one value per epoch, channel pair and scale.
//
//   src [((e * C + c) * F + f) * n_out + t]   complex T: the chunk's rows, epoch-major
//   sum [(e * P + p) * F + f]                 complex fp64: S_e,p (PLV: Phi_e,p), p = (ia[p], ib[p])
//   SUM_LAG: sum [((e * P + p) * F + f) * 4 ..] fp64 {L0, L1, L2, L3}
//   power [(e * C + c) * F + f]               fp64: P_e,cc (nw_conn_time_power_kernel)
// each the sum over the window's samples s_j = t0 + j * step, j = 0 .. T - 1, of the terms
// nw_conn_accumulate_kernel (nw_conn.hip) adds per epoch: fp64 values, every product and every term
// rounded on its own (no fma into a sum), for PLV each value divided by its hypot first.
//
// Summation order (the contract, ninwave.h; nw_shape.h conn_time_lane): lane l starts every
// accumulator at +0.0 and adds the terms of j = l, l + 64, l + 128, ... in that order; lanes and tail
// samples without a j < T add nothing.  The 64 lane values are then folded, v_l <- v_l + v_{l xor d}
// for d = 32, 16, 8, 4, 2, 1, every component on its own, and lane 0 writes the result.  A result
// depends only on its two rows and on (t0, T, step): not on the pair list, the tiling or the chunks.
//
// nw_conn_time_kernel is nw_conn_accumulate_kernel with "epoch" replaced by "sample tile": a block
// owns one epoch of the chunk, one scale and one pair tile (<= 64 pairs over <= 16 channels), wave w of
// its 4 keeps the pairs w, w + 4, ... in registers, lane = sample of the tile; per sample tile the
// tile's channels are staged once in LDS as fp64 (PLV: as unit phasors), double buffered: the next
// tile's global loads are issued before the current one is consumed and written to the other buffer
// after it, one barrier per sample tile.  The accumulators are never read from memory: every
// (e, pair, f) belongs to exactly one block of exactly one launch (no memset, no read-modify-write).
#include <algorithm>

#include "nw_dcheck.h"
#include "nw_internal.h"

namespace nw {
namespace {

// a rounded fp64 product that the compiler may not fuse into a following add (as nw_conn.hip)
__device__ __forceinline__ double mul_nc(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double add_nc(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}

// the fold of the 64 lane values: every lane ends with the same sum, in the contract's order
__device__ __forceinline__ double fold64(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = add_nc(v, __shfl_xor(v, d, 64));
    return v;
}

constexpr int kConnThreads = kConnWaves * 64;
constexpr int kConnStage = kConnCh / kConnWaves;   // channels a wave stages per sample tile

struct ConnAcc2 { double re, im; };
struct ConnAcc4 { double l0, l1, l2, l3; };

template <typename T, int MODE>
__global__ __launch_bounds__(kConnThreads) void nw_conn_time_kernel(
    const cplx<T>* __restrict__ src, double2* __restrict__ sum, const ConnTile* __restrict__ tiles, int ntiles,
    int64_t ec, int nchan, int nfreq, int64_t n_out, int64_t npairs, int64_t t0, int64_t count, int64_t step, int xcd) {
    static_assert(kConnTileN == 64, "lane = sample of the tile");
    constexpr bool PLV = MODE == SUM_PLV, LAG = MODE == SUM_LAG;
    constexpr int NV = LAG ? 2 : 1;   // double2 values per epoch, pair and scale in `sum`
    __shared__ double stage[2][kConnCh][2][kConnTileN];   // [buffer][slot][re, im][sample]: 32 KiB

    const ConnTimeSlot sl = conn_time_slot((int64_t)blockIdx.x, nfreq, ntiles, xcd != 0);
    if (sl.e >= ec) return;   // padding of the XCD order (the whole block)
    NW_DCHECK(sl.tile >= 0 && sl.tile < ntiles && sl.e >= 0 && sl.f >= 0 && sl.f < nfreq);
    const int64_t e = sl.e;
    const int f = sl.f;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const ConnTile& tile = tiles[sl.tile];
    const int nch = tile.nch, np = tile.npairs;
    NW_DCHECK(nch >= 0 && nch <= kConnCh && np >= 0 && np <= kConnPairs);
    const int64_t fn = (int64_t)nfreq * n_out;
    const int64_t ntl = conn_time_tiles(count);

    // (an array of structs, as nw_conn.hip: plain double[16] arrays end in scratch)
    std::conditional_t<LAG, ConnAcc4, ConnAcc2> acc[kConnPerWave];
#pragma unroll
    for (int k = 0; k < kConnPerWave; ++k) {
        if constexpr (LAG) acc[k].l0 = acc[k].l1 = acc[k].l2 = acc[k].l3 = 0.0;
        else acc[k].re = acc[k].im = 0.0;
    }

    cplx<T> in[kConnStage];
    // the samples j = it * 64 + lane of sample tile `it`; a lane with j >= count loads nothing
    auto load = [&](int64_t it) {
        const int64_t j = it * kConnTileN + lane;
        NW_DCHECK(conn_time_lane(j) == lane);
        const bool live = j < count;
        const int64_t t = t0 + j * step;
#pragma unroll
        for (int q = 0; q < kConnStage; ++q) {
            const int s = w + q * kConnWaves;
            in[q] = cplx<T>{T(0), T(0)};
            if (s < nch && live) {
                const int64_t c = tile.ch[s];
                NW_DCHECK(c >= 0 && c < nchan && t >= 0 && t < n_out);
                NW_DCHECK((e * nchan + c) * fn + (int64_t)f * n_out + t < ec * nchan * fn);
                in[q] = src[(e * nchan + c) * fn + (int64_t)f * n_out + t];
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int q = 0; q < kConnStage; ++q) {
            const int s = w + q * kConnWaves;
            if (s < nch) {
                NW_DCHECK(buf >= 0 && buf < 2 && s < kConnCh && lane < kConnTileN);
                double re = (double)in[q].re, im = (double)in[q].im;
                if constexpr (PLV) {
                    const double m = hypot(re, im);
                    re /= m, im /= m;
                }
                stage[buf][s][0][lane] = re;
                stage[buf][s][1][lane] = im;
            }
        }
    };

    if (ntl > 0) {
        load(0);
        store(0);
    }
    __syncthreads();
    for (int64_t it = 0; it < ntl; ++it) {
        const int cur = (int)(it & 1);
        const bool more = it + 1 < ntl;
        if (more) load(it + 1);
        if (it * kConnTileN + lane < count) {   // a tail sample past the window adds nothing
#pragma unroll
            for (int k = 0; k < kConnPerWave; ++k) {
                const int j = w + k * kConnWaves;
                if (j < np) {
                    const int a = tile.sa[j], b = tile.sb[j];
                    NW_DCHECK(a >= 0 && a < nch && b >= 0 && b < nch);
                    const double ar = stage[cur][a][0][lane], ai = stage[cur][a][1][lane];
                    const double br = stage[cur][b][0][lane], bi = stage[cur][b][1][lane];
                    if constexpr (LAG) {
                        const double m = add_nc(mul_nc(ai, br), -mul_nc(ar, bi));
                        acc[k].l0 = add_nc(acc[k].l0, m);
                        acc[k].l1 = add_nc(acc[k].l1, fabs(m));
                        acc[k].l2 = add_nc(acc[k].l2, mul_nc(m, m));
                        acc[k].l3 = add_nc(acc[k].l3, lag_sgn(m));
                    } else {
                        acc[k].re = add_nc(acc[k].re, add_nc(mul_nc(ar, br), mul_nc(ai, bi)));
                        acc[k].im = add_nc(acc[k].im, add_nc(mul_nc(ai, br), -mul_nc(ar, bi)));
                    }
                }
            }
        }
        // the other buffer was last read before the previous barrier
        if (more) store(cur ^ 1);
        __syncthreads();
    }

    // the fold (every lane of the wave takes part: w and np are wave-uniform), lane 0 writes
#pragma unroll
    for (int k = 0; k < kConnPerWave; ++k) {
        const int j = w + k * kConnWaves;
        if (j < np) {
            const int64_t o = tile.out[j];
            const int64_t at = (e * npairs + o) * nfreq + f;
            NW_DCHECK(o >= 0 && o < npairs && at >= 0 && at < ec * npairs * nfreq);
            if constexpr (LAG) {
                const double l0 = fold64(acc[k].l0), l1 = fold64(acc[k].l1);
                const double l2 = fold64(acc[k].l2), l3 = fold64(acc[k].l3);
                if (lane == 0) {
                    NW_DCHECK(NV * at + 1 < NV * ec * npairs * nfreq);
                    sum[NV * at] = double2{l0, l1};
                    sum[NV * at + 1] = double2{l2, l3};
                }
            } else {
                const double re = fold64(acc[k].re), im = fold64(acc[k].im);
                if (lane == 0) sum[at] = double2{re, im};
            }
        }
    }
}

// power[(e * C + c) * F + f] = sum_j |y_{e,c}[f, s_j]|^2: one wave per row, the order of the contract
template <typename T>
__global__ __launch_bounds__(kConnThreads) void nw_conn_time_power_kernel(const cplx<T>* __restrict__ src,
                                                                         double* __restrict__ power, int64_t nrows,
                                                                         int64_t n_out, int64_t t0, int64_t count,
                                                                         int64_t step) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kConnWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= nrows) return;   // the whole wave
    double p = 0.0;
#pragma unroll 4
    for (int64_t j = lane; j < count; j += kConnTileN) {
        const int64_t t = t0 + j * step;
        NW_DCHECK(conn_time_lane(j) == lane && t >= 0 && t < n_out && row * n_out + t < nrows * n_out);
        const cplx<T> v = src[row * n_out + t];
        const double re = (double)v.re, im = (double)v.im;
        p = add_nc(p, add_nc(mul_nc(re, re), mul_nc(im, im)));
    }
    p = fold64(p);
    if (lane == 0) {
        NW_DCHECK(row >= 0 && row < nrows);
        power[row] = p;
    }
}

}  // namespace

hipError_t launch_conn_time(int dtype, int mode, const void* src, void* sum, double* power, const ConnTile* tiles,
                            int ntiles, int64_t ec, int nchan, int nfreq, int64_t n_out, int64_t npairs, int64_t t0,
                            int64_t count, int64_t step, bool xcd, hipStream_t s) {
    const int64_t blocks = ntiles > 0 ? conn_time_blocks(ec, nfreq, ntiles, xcd) : 0;
    const int64_t nrows = ec * nchan * nfreq;
    const int64_t pb = (nrows + kConnWaves - 1) / kConnWaves;
    if (blocks > 0x7fffffff || pb > 0x7fffffff) return hipErrorInvalidValue;
    for_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (blocks > 0)
            for_sum_mode(mode, [&](auto v) {
                nw_launch(nw_conn_time_kernel<T, decltype(v)::value>, dim3((unsigned)blocks), dim3(kConnThreads), 0, s,
                          (const cplx<T>*)src, (double2*)sum, tiles, ntiles, ec, nchan, nfreq, n_out, npairs, t0, count,
                          step, xcd ? 1 : 0);
            });
        if (power && mode == SUM_CROSS && pb > 0)
            nw_launch(nw_conn_time_power_kernel<T>, dim3((unsigned)pb), dim3(kConnThreads), 0, s, (const cplx<T>*)src,
                      power, nrows, n_out, t0, count, step);
    });
    return hipGetLastError();
}

}  // namespace nw
