// nw_reduce_dev.h — the device pieces the epoch-chunk reductions share (nw_conn.hip, nw_conn_time.hip,
// nw_env.hip, nw_pac.hip, nw_erpac.hip): the rounded fp64 arithmetic, the fold of a wave, the pair arithmetic as
// policy types, and the two kernel skeletons of the over-time sums.  The summation order is the
// contract (ninwave.h): a change here changes every kernel that uses the piece, identically.
//
// A pair policy P states one measure's arithmetic:
//   kStaged            fp64 values staged in LDS per channel and sample
//   stage(v, img, l)   the staging transform: sample v of a channel into img[value][l]
//   Acc, zero(a)       a pair's accumulators (a struct: plain double arrays end in scratch, tools/regs.py)
//   term(a, ya, yb, l) one sample's (epoch's) terms of the pair (ya, yb) added to a, each rounded on its own
//   Out, kOut          a result is kOut consecutive Out values
//   load, store        a's components from / to a result; fold(a): fold64 of every component
#pragma once
#include "nw_dcheck.h"
#include "nw_internal.h"

namespace nw {

// a rounded fp64 product that the compiler may not fuse into a following add (as nw_kernels.hip)
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
constexpr int kConnStage = kConnCh / kConnWaves;   // channels a wave stages per epoch or sample tile

// one staged channel of one buffer: [value][sample]
template <int NS>
using Staged = double[NS][kConnTileN];

// SUM_CROSS: S = sum y_a conj(y_b) (k_accumulate_pair's terms)
struct CrossSum {
    static constexpr int kStaged = 2, kOut = 1;
    using Out = double2;
    struct Acc { double re, im; };
    static __device__ __forceinline__ void zero(Acc& a) { a.re = a.im = 0.0; }
    template <typename T>
    static __device__ __forceinline__ void stage(cplx<T> v, Staged<2>& img, int lane) {
        img[0][lane] = (double)v.re;
        img[1][lane] = (double)v.im;
    }
    static __device__ __forceinline__ void term(Acc& a, const Staged<2>& ya, const Staged<2>& yb, int lane) {
        const double ar = ya[0][lane], ai = ya[1][lane], br = yb[0][lane], bi = yb[1][lane];
        a.re = add_nc(a.re, add_nc(mul_nc(ar, br), mul_nc(ai, bi)));
        a.im = add_nc(a.im, add_nc(mul_nc(ai, br), -mul_nc(ar, bi)));
    }
    static __device__ __forceinline__ void load(Acc& a, const Out* at) { a.re = at->x, a.im = at->y; }
    static __device__ __forceinline__ void store(const Acc& a, Out* at) { *at = double2{a.re, a.im}; }
    static __device__ __forceinline__ void fold(Acc& a) { a.re = fold64(a.re), a.im = fold64(a.im); }
};

// SUM_PLV: Phi = the cross sum of the unit phasors, a value normalised once and not once per pair
struct PlvSum : CrossSum {
    template <typename T>
    static __device__ __forceinline__ void stage(cplx<T> v, Staged<2>& img, int lane) {
        double re = (double)v.re, im = (double)v.im;
        const double m = hypot(re, im);
        re /= m, im /= m;
        img[0][lane] = re;
        img[1][lane] = im;
    }
};

// SUM_LAG: {L0, L1, L2, L3} = the sums of m, |m|, m^2, sgn m with m = Im y_a conj(y_b); staged as SUM_CROSS.
// A lane reads and writes its 32 B as two 16-byte accesses.
struct LagSum : CrossSum {
    static constexpr int kOut = 2;
    struct Acc { double l0, l1, l2, l3; };
    static __device__ __forceinline__ void zero(Acc& a) { a.l0 = a.l1 = a.l2 = a.l3 = 0.0; }
    static __device__ __forceinline__ void term(Acc& a, const Staged<2>& ya, const Staged<2>& yb, int lane) {
        const double ar = ya[0][lane], ai = ya[1][lane], br = yb[0][lane], bi = yb[1][lane];
        const double m = add_nc(mul_nc(ai, br), -mul_nc(ar, bi));
        a.l0 = add_nc(a.l0, m);
        a.l1 = add_nc(a.l1, fabs(m));
        a.l2 = add_nc(a.l2, mul_nc(m, m));
        a.l3 = add_nc(a.l3, lag_sgn(m));
    }
    static __device__ __forceinline__ void load(Acc& a, const Out* at) {
        const double2 u = at[0], v = at[1];
        a.l0 = u.x, a.l1 = u.y, a.l2 = v.x, a.l3 = v.y;
    }
    static __device__ __forceinline__ void store(const Acc& a, Out* at) {
        at[0] = double2{a.l0, a.l1};
        at[1] = double2{a.l2, a.l3};
    }
    static __device__ __forceinline__ void fold(Acc& a) {
        a.l0 = fold64(a.l0), a.l1 = fold64(a.l1), a.l2 = fold64(a.l2), a.l3 = fold64(a.l3);
    }
};

template <int MODE>
using SumPolicy = std::conditional_t<MODE == SUM_PLV, PlvSum, std::conditional_t<MODE == SUM_LAG, LagSum, CrossSum>>;

// NW_ENV_PLAIN: sum A_a A_b of the amplitude envelopes A = hypot(re, im)
struct EnvPlain {
    static constexpr int kStaged = 1, kOut = 1;
    using Out = double;
    struct Acc { double ab; };
    static __device__ __forceinline__ void zero(Acc& a) { a.ab = 0.0; }
    template <typename T>
    static __device__ __forceinline__ void stage(cplx<T> v, Staged<1>& img, int lane) {
#ifdef NW_ABL_ENV_NODIV   // diagnostic A/B (wrong sums): the staging without its hypot
        img[0][lane] = fabs((double)v.re);
#else
        img[0][lane] = hypot((double)v.re, (double)v.im);
#endif
    }
    static __device__ __forceinline__ void term(Acc& a, const Staged<1>& ya, const Staged<1>& yb, int lane) {
        a.ab = add_nc(a.ab, mul_nc(ya[0][lane], yb[0][lane]));
    }
    static __device__ __forceinline__ void store(const Acc& a, Out* at) { *at = a.ab; }
    static __device__ __forceinline__ void fold(Acc& a) { a.ab = fold64(a.ab); }
};

// NW_ENV_ORTH: {sum u, sum u u, sum u A_b, sum v, sum v v, sum v A_a} with q = |Im u_a conj(u_b)| of the unit
// phasors, u = A_a q, v = A_b q (nw_env.hip).  Staged as {A, ur, ui}: the hypot and the two divisions
// are paid once per channel and sample.  A lane without a sample stages {0, 0 / 0, 0 / 0}.
struct EnvOrth {
    static constexpr int kStaged = 3, kOut = 6;
    using Out = double;
    struct Acc { double u, uu, ub, v, vv, va; };
    static __device__ __forceinline__ void zero(Acc& a) { a.u = a.uu = a.ub = a.v = a.vv = a.va = 0.0; }
    template <typename T>
    static __device__ __forceinline__ void stage(cplx<T> v, Staged<3>& img, int lane) {
        const double re = (double)v.re, im = (double)v.im;
#ifdef NW_ABL_ENV_NODIV   // diagnostic A/B (wrong sums): the staging without its hypot and its two divisions
        img[0][lane] = fabs(re);
        img[1][lane] = re;
        img[2][lane] = im;
#else
        const double h = hypot(re, im);
        img[0][lane] = h;
        img[1][lane] = re / h;
        img[2][lane] = im / h;
#endif
    }
    static __device__ __forceinline__ void term(Acc& a, const Staged<3>& ya, const Staged<3>& yb, int lane) {
        const double Aa = ya[0][lane], Ab = yb[0][lane];
        const double ar = ya[1][lane], ai = ya[2][lane], br = yb[1][lane], bi = yb[2][lane];
        const double q = fabs(add_nc(mul_nc(ai, br), -mul_nc(ar, bi)));
        const double u = mul_nc(Aa, q), v = mul_nc(Ab, q);
        a.u = add_nc(a.u, u);
        a.uu = add_nc(a.uu, mul_nc(u, u));
        a.ub = add_nc(a.ub, mul_nc(u, Ab));
        a.v = add_nc(a.v, v);
        a.vv = add_nc(a.vv, mul_nc(v, v));
        a.va = add_nc(a.va, mul_nc(v, Aa));
    }
    static __device__ __forceinline__ void store(const Acc& a, Out* at) {
        double2* const o2 = (double2*)at;   // 48-byte records: 16-aligned
        o2[0] = double2{a.u, a.uu};
        o2[1] = double2{a.ub, a.v};
        o2[2] = double2{a.vv, a.va};
    }
    static __device__ __forceinline__ void fold(Acc& a) {
        a.u = fold64(a.u), a.uu = fold64(a.uu), a.ub = fold64(a.ub);
        a.v = fold64(a.v), a.vv = fold64(a.vv), a.va = fold64(a.va);
    }
};

// The over-time pair sums (nw_conn_time_kernel, nw_env_time_kernel): a block owns one epoch of the chunk,
// one scale and one pair tile (<= 64 pairs over <= 16 channels), wave w of its 4 keeps the pairs w, w + 4,
// ... in registers, lane = sample of the 64-sample tile.  Per sample tile the tile's channels are staged
// once in LDS by P::stage, double buffered: the next tile's global loads are issued before the current
// one is consumed and written to the other buffer after it, one barrier per sample tile.  Lane l adds
// the terms of j = l, l + 64, ... in that order (conn_time_lane), the 64 lane values are folded and lane
// 0 writes out[((e * npairs + p) * nfreq + f) * P::kOut ..].  The accumulators are never read from memory:
// every (e, pair, f) belongs to exactly one block of exactly one launch (no memset, no read-modify-write).
template <typename P, typename T>
__device__ __forceinline__ void pair_time_sums(const cplx<T>* __restrict__ src, typename P::Out* __restrict__ out,
                                               const ConnTile* __restrict__ tiles, int ntiles, int64_t ec, int nchan,
                                               int nfreq, int64_t n_out, int64_t npairs, int64_t t0, int64_t count,
                                               int64_t step, int xcd) {
    static_assert(kConnTileN == 64, "lane = sample of the tile");
    static_assert(2 * kConnCh * P::kStaged * kConnTileN * sizeof(double) <= 64 * 1024,
                  "double-buffered staging fits the LDS of a block");
    // [buffer][slot][value][sample] in fp64: a wave reads 64 consecutive doubles (ds_read_b64, lane l on
    // banks 2 l, 2 l + 1 of its 32-lane half: no conflict); 16 KiB per staged value
    __shared__ double stage[2][kConnCh][P::kStaged][kConnTileN];

    const ConnTimeSlot sl = conn_time_slot((int64_t)blockIdx.x, nfreq, ntiles, xcd != 0);
    if (sl.e >= ec) return;   // padding of the XCD order (the whole block)
    NW_DCHECK_R(sl.tile >= 0 && sl.tile < ntiles && sl.e >= 0 && sl.f >= 0 && sl.f < nfreq);
    const int64_t e = sl.e;
    const int f = sl.f;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const ConnTile& tile = tiles[sl.tile];
    const int nch = tile.nch, np = tile.npairs;
    NW_DCHECK_R(nch >= 0 && nch <= kConnCh && np >= 0 && np <= kConnPairs);
    const int64_t fn = (int64_t)nfreq * n_out;
    const int64_t ntl = conn_time_tiles(count);

    typename P::Acc acc[kConnPerWave];
#pragma unroll
    for (int k = 0; k < kConnPerWave; ++k) P::zero(acc[k]);

    cplx<T> in[kConnStage];
    // the samples j = it * 64 + lane of sample tile `it`; a lane with j >= count loads nothing
    auto load = [&](int64_t it) {
        const int64_t j = it * kConnTileN + lane;
        NW_DCHECK_R(conn_time_lane(j) == lane);
        const bool live = j < count;
        const int64_t t = t0 + j * step;
#pragma unroll
        for (int q = 0; q < kConnStage; ++q) {
            const int s = w + q * kConnWaves;
            in[q] = cplx<T>{T(0), T(0)};
            if (s < nch && live) {
                const int64_t c = tile.ch[s];
                NW_DCHECK_R(c >= 0 && c < nchan && t >= 0 && t < n_out);
                NW_DCHECK_R((e * nchan + c) * fn + (int64_t)f * n_out + t < ec * nchan * fn);
#ifdef NW_ABL_ENV_NOLOAD   // diagnostic A/B of tools/env_rate.py (wrong sums): no global loads, the rest kept
                in[q] = cplx<T>{T(1 + (t & 7)), T(1 + c)};
#else
                in[q] = src[(e * nchan + c) * fn + (int64_t)f * n_out + t];
#endif
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int q = 0; q < kConnStage; ++q) {
            const int s = w + q * kConnWaves;
            if (s < nch) {
                NW_DCHECK_R(buf >= 0 && buf < 2 && s < kConnCh && lane < kConnTileN);
                P::stage(in[q], stage[buf][s], lane);
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
                    NW_DCHECK_R(a >= 0 && a < nch && b >= 0 && b < nch);
                    P::term(acc[k], stage[cur][a], stage[cur][b], lane);
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
            NW_DCHECK_R(o >= 0 && o < npairs && at >= 0 && at < ec * npairs * nfreq);
            P::fold(acc[k]);
            if (lane == 0) {
                NW_DCHECK_R(P::kOut * at + P::kOut - 1 < P::kOut * ec * npairs * nfreq);
                P::store(acc[k], out + P::kOut * at);
            }
        }
    }
}

// The per-row sums (nw_conn_time_power_kernel, nw_env_chan_kernel, nw_pac_rows_kernel): one wave per
// row, lane l starts at +0.0 and adds the terms of j = l, l + 64, ... in that order, the lane values are
// folded and lane 0 writes.  Row r's samples are src[off(r) + t]; term(r, s0, s1, re, im) adds one sample's
// terms to the two sums and write(r, s0, s1) is lane 0's.  `total` is the length of src (the checks).
template <int WAVES, typename T, typename Off, typename Term, typename Write>
__device__ __forceinline__ void row_time_sums(const cplx<T>* __restrict__ src, int64_t nrows, int64_t total, int64_t n_out,
                                              int64_t t0, int64_t count, int64_t step, Off off, Term term, Write write) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= nrows) return;   // the whole wave
    const int64_t at = off(row);
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
    for (int64_t j = lane; j < count; j += kConnTileN) {
        const int64_t t = t0 + j * step;
        NW_DCHECK_R(conn_time_lane(j) == lane && t >= 0 && t < n_out && at + t < total);
        const cplx<T> v = src[at + t];
        term(row, s0, s1, (double)v.re, (double)v.im);
    }
    s0 = fold64(s0);
    s1 = fold64(s1);
    if (lane == 0) {
        NW_DCHECK_R(row >= 0 && row < nrows);
        write(row, s0, s1);
    }
}

// |y|^2 as k_accumulate_pair adds it to P_aa
__device__ __forceinline__ double power_term(double re, double im) { return add_nc(mul_nc(re, re), mul_nc(im, im)); }

}  // namespace nw
