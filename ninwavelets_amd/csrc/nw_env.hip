// nw_env.hip — envelope correlation (nw_execute_env_time): the complex rows of a chunk of epochs x
// channels reduced along the SAMPLE axis into the Pearson sums of two amplitude envelopes per epoch,
// channel pair and scale, plain or pairwise orthogonalised (Hipp et al. 2012).
//
//   src  [((e * C + c) * F + f) * n_out + t]     complex T: the chunk's rows, epoch-major
//   NW_ENV_PLAIN: pair [(e * P + p) * F + f]           fp64: sum_j A_a A_b,       p = (ia[p], ib[p])
//   NW_ENV_ORTH:  pair [((e * P + p) * F + f) * 6 ..]  fp64 {sum u, sum u u, sum u A_b, sum v, sum v v, sum v A_a}
//   chan [((e * C + c) * F + f) * 2 ..]          fp64 {sum_j A, sum_j (re re + im im)}  (nw_env_chan_kernel)
// over the window's samples s_j = t0 + j * step, j = 0 .. T - 1, with, in fp64 per channel and sample,
//   h = hypot(re, im),  A = h,  (ur, ui) = (re / h, im / h)
// (SUM_PLV's and nw_pac.hip's unit phasor, NaN where |y| = 0) and per pair and sample
//   s = ua_i ub_r + (-(ua_r ub_i)),  q = |s|,  u = A_a q,  v = A_b q:
// u = |Im(y_a conj(y_b) / |y_b|)|, a orthogonalised against b, and v the reverse.  Every product and
// every term is rounded on its own (no fma into a sum).  A self pair has s = +0.0 exactly.
//
// Summation order: that of nw_execute_conn_time (nw_shape.h conn_time_lane): lane l starts at +0.0 and
// adds the terms of j = l, l + 64, ... in that order, the 64 lane values are folded with xor 32 .. 1,
// every component on its own, and lane 0 writes.  A result depends only on its two rows and on
// (t0, T, step): not on the pair list, the tiling or the chunks.
//
// nw_env_time_kernel is nw_conn_time_kernel with other arithmetic: a block owns one epoch of the
// chunk, one scale and one pair tile (<= 64 pairs over <= 16 channels), wave w of its 4 keeps the
// pairs w, w + 4, ... in registers, lane = sample of the tile.  Per sample tile the tile's channels
// are staged once in LDS as {A, ur, ui}, so the hypot and the two divisions are paid once per channel
// and sample and not once per pair; double buffered, one barrier per sample tile.  The image is
// [buffer][slot][value][sample] in fp64: a wave reads 64 consecutive doubles (ds_read_b64, lane l on
// banks 2 l, 2 l + 1 of its 32-lane half: no conflict).  NW_ENV_ORTH keeps 6 fp64 accumulators for each
// of its 16 pairs in registers (192 of the block's 512 per lane; no scratch: profiles/r17_env_rate.txt).
// Every (e, pair, f) belongs to exactly one block of one launch: no memset, no read-modify-write.
#include <algorithm>

#include "nw_dcheck.h"
#include "nw_internal.h"

namespace nw {
namespace {

// a rounded fp64 product that the compiler may not fuse into a following add (as nw_conn_time.hip)
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

constexpr int kEnvThreads = kConnWaves * 64;
constexpr int kEnvStage = kConnCh / kConnWaves;   // channels a wave stages per sample tile
static_assert(2 * kConnCh * 3 * kConnTileN * sizeof(double) <= 64 * 1024, "double-buffered staging fits the LDS of a block");

struct EnvAcc1 { double ab; };
struct EnvAcc6 { double u, uu, ub, v, vv, va; };

template <typename T, int MODE>
__global__ __launch_bounds__(kEnvThreads) void nw_env_time_kernel(
    const cplx<T>* __restrict__ src, double* __restrict__ pair, const ConnTile* __restrict__ tiles, int ntiles,
    int64_t ec, int nchan, int nfreq, int64_t n_out, int64_t npairs, int64_t t0, int64_t count, int64_t step, int xcd) {
    static_assert(kConnTileN == 64, "lane = sample of the tile");
    static_assert(MODE == NW_ENV_PLAIN || MODE == NW_ENV_ORTH, "envelope mode");
    constexpr bool ORTH = MODE == NW_ENV_ORTH;
    constexpr int NV = env_pair_values(MODE);   // fp64 values per epoch, pair and scale in `pair`
    constexpr int NS = ORTH ? 3 : 1;            // staged fp64 values per channel and sample
    __shared__ double stage[2][kConnCh][NS][kConnTileN];   // [buffer][slot][A, ur, ui][sample]: 48 KiB (plain: 16)

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

    // (an array of structs, as nw_conn_time.hip: plain double arrays end in scratch)
    std::conditional_t<ORTH, EnvAcc6, EnvAcc1> acc[kConnPerWave];
#pragma unroll
    for (int k = 0; k < kConnPerWave; ++k) {
        if constexpr (ORTH) acc[k].u = acc[k].uu = acc[k].ub = acc[k].v = acc[k].vv = acc[k].va = 0.0;
        else acc[k].ab = 0.0;
    }

    cplx<T> in[kEnvStage];
    // the samples j = it * 64 + lane of sample tile `it`; a lane with j >= count loads nothing
    auto load = [&](int64_t it) {
        const int64_t j = it * kConnTileN + lane;
        NW_DCHECK(conn_time_lane(j) == lane);
        const bool live = j < count;
        const int64_t t = t0 + j * step;
#pragma unroll
        for (int q = 0; q < kEnvStage; ++q) {
            const int s = w + q * kConnWaves;
            in[q] = cplx<T>{T(0), T(0)};
            if (s < nch && live) {
                const int64_t c = tile.ch[s];
                NW_DCHECK(c >= 0 && c < nchan && t >= 0 && t < n_out);
                NW_DCHECK((e * nchan + c) * fn + (int64_t)f * n_out + t < ec * nchan * fn);
#ifdef NW_ABL_ENV_NOLOAD   // diagnostic A/B (wrong sums): no global loads, the staging and the pair arithmetic kept
                in[q] = cplx<T>{T(1 + (t & 7)), T(1 + c)};
#else
                in[q] = src[(e * nchan + c) * fn + (int64_t)f * n_out + t];
#endif
            }
        }
    };
    // a lane without a sample holds {0, 0 / 0, 0 / 0}, which the accumulation below skips
    auto store = [&](int buf) {
#pragma unroll
        for (int q = 0; q < kEnvStage; ++q) {
            const int s = w + q * kConnWaves;
            if (s < nch) {
                NW_DCHECK(buf >= 0 && buf < 2 && s < kConnCh && lane < kConnTileN);
                const double re = (double)in[q].re, im = (double)in[q].im;
#ifdef NW_ABL_ENV_NODIV   // diagnostic A/B (wrong sums): the staging without its hypot and its two divisions
                stage[buf][s][0][lane] = fabs(re);
                if constexpr (ORTH) {
                    stage[buf][s][1][lane] = re;
                    stage[buf][s][2][lane] = im;
                }
#else
                const double h = hypot(re, im);
                stage[buf][s][0][lane] = h;
                if constexpr (ORTH) {
                    stage[buf][s][1][lane] = re / h;
                    stage[buf][s][2][lane] = im / h;
                }
#endif
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
                    const double Aa = stage[cur][a][0][lane], Ab = stage[cur][b][0][lane];
                    if constexpr (ORTH) {
                        const double ar = stage[cur][a][1][lane], ai = stage[cur][a][2][lane];
                        const double br = stage[cur][b][1][lane], bi = stage[cur][b][2][lane];
                        const double q = fabs(add_nc(mul_nc(ai, br), -mul_nc(ar, bi)));
                        const double u = mul_nc(Aa, q), v = mul_nc(Ab, q);
                        acc[k].u = add_nc(acc[k].u, u);
                        acc[k].uu = add_nc(acc[k].uu, mul_nc(u, u));
                        acc[k].ub = add_nc(acc[k].ub, mul_nc(u, Ab));
                        acc[k].v = add_nc(acc[k].v, v);
                        acc[k].vv = add_nc(acc[k].vv, mul_nc(v, v));
                        acc[k].va = add_nc(acc[k].va, mul_nc(v, Aa));
                    } else {
                        acc[k].ab = add_nc(acc[k].ab, mul_nc(Aa, Ab));
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
            if constexpr (ORTH) {
                const double u = fold64(acc[k].u), uu = fold64(acc[k].uu), ub = fold64(acc[k].ub);
                const double v = fold64(acc[k].v), vv = fold64(acc[k].vv), va = fold64(acc[k].va);
                if (lane == 0) {
                    NW_DCHECK(NV * at + 5 < NV * ec * npairs * nfreq);
                    double2* const o2 = (double2*)(pair + NV * at);   // 48-byte records: 16-aligned
                    o2[0] = double2{u, uu};
                    o2[1] = double2{ub, v};
                    o2[2] = double2{vv, va};
                }
            } else {
                const double ab = fold64(acc[k].ab);
                if (lane == 0) pair[at] = ab;
            }
        }
    }
}

// chan[(e * C + c) * F + f] = {sum_j A, sum_j |y|^2} of the row: one wave per row, the order of the
// contract; the first sum as nw_pac_rows_kernel forms its amplitude sum, the second as
// nw_conn_time_power_kernel forms its power
template <typename T>
__global__ __launch_bounds__(kEnvThreads) void nw_env_chan_kernel(const cplx<T>* __restrict__ src,
                                                                  double* __restrict__ chan, int64_t nrows,
                                                                  int64_t n_out, int64_t t0, int64_t count,
                                                                  int64_t step) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kConnWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= nrows) return;   // the whole wave
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
    for (int64_t j = lane; j < count; j += kConnTileN) {
        const int64_t t = t0 + j * step;
        NW_DCHECK(conn_time_lane(j) == lane && t >= 0 && t < n_out && row * n_out + t < nrows * n_out);
        const cplx<T> v = src[row * n_out + t];
        const double re = (double)v.re, im = (double)v.im;
        s0 = add_nc(s0, hypot(re, im));
        s1 = add_nc(s1, add_nc(mul_nc(re, re), mul_nc(im, im)));
    }
    s0 = fold64(s0);
    s1 = fold64(s1);
    if (lane == 0) {
        NW_DCHECK(row >= 0 && row < nrows);
        chan[2 * row] = s0;   // (8-aligned only: the sums follow the NW_ENV_PLAIN pair sums)
        chan[2 * row + 1] = s1;
    }
}

}  // namespace

hipError_t launch_env_time(int dtype, int env, const void* src, void* pair, double* chan, const ConnTile* tiles,
                           int ntiles, int64_t ec, int nchan, int nfreq, int64_t n_out, int64_t npairs, int64_t t0,
                           int64_t count, int64_t step, bool xcd, hipStream_t s) {
    const int64_t blocks = ntiles > 0 ? conn_time_blocks(ec, nfreq, ntiles, xcd) : 0;
    const int64_t nrows = ec * nchan * nfreq;
    const int64_t cb = (nrows + kConnWaves - 1) / kConnWaves;
    if (blocks > 0x7fffffff || cb > 0x7fffffff) return hipErrorInvalidValue;
    if (env != NW_ENV_PLAIN && env != NW_ENV_ORTH) return hipErrorInvalidValue;
    for_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        auto go = [&](auto v) {
            nw_launch(nw_env_time_kernel<T, decltype(v)::value>, dim3((unsigned)blocks), dim3(kEnvThreads), 0, s,
                      (const cplx<T>*)src, (double*)pair, tiles, ntiles, ec, nchan, nfreq, n_out, npairs, t0, count, step,
                      xcd ? 1 : 0);
        };
        if (blocks > 0) {
            if (env == NW_ENV_ORTH) go(std::integral_constant<int, NW_ENV_ORTH>{});
            else go(std::integral_constant<int, NW_ENV_PLAIN>{});
        }
        if (chan && cb > 0)
            nw_launch(nw_env_chan_kernel<T>, dim3((unsigned)cb), dim3(kEnvThreads), 0, s, (const cplx<T>*)src,
                      chan, nrows, n_out, t0, count, step);
    });
    return hipGetLastError();
}

}  // namespace nw
