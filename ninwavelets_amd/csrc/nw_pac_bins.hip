// nw_pac_bins.hip — phase-binned phase-amplitude coupling (nw_execute_pac_bins): the complex rows of a
// chunk of epochs x channels reduced along the SAMPLE axis into one amplitude histogram over nbins phase
// bins per epoch, channel pair, listed phase scale and listed amplitude scale.
//
//   src   [((e * C + c) * F + f) * n_out + t]                  complex T: the chunk's rows, epoch-major
//   sum   [(((e * P + p) * nph + i) * nam + k) * nbins + b]     fp64: sum_{j : bin_j = b} A_j
//   cnt   [((e * C + c) * nph + i) * nbins + b]                 fp64: #{j : bin_j = b}
// over the window's samples s_j = t0 + j * step, j = 0 .. T - 1, with, in fp64,
//   A     = hypot(re, im) of the amplitude channel ia[p]'s row fam[k] at s_j (nw_execute_pac's A),
//   bin_j = pac_bin of the phase channel ip[p]'s row fph[i] at s_j (cnt: of channel c's).
//
// The bin (ninwave.h: THE BIN) uses no atan2: with h = nbins / 2 and edge[b] = {cos theta_b, sin theta_b}
// the doubles of nw_pac_bin_edges, uploaded with the call, the half plane picks base = 0 or h and the
// bin is base + the number of edges k = 1 .. h - 1 with edge[base + k].x * im - edge[base + k].y * re >= 0,
// each product rounded on its own; y = 0 is bin h.
//
// Summation order: that of nw_execute_conn_time (nw_shape.h conn_time_lane) per bin: lane l adds the A_j of
// j = l, l + 64, ... in that order to its partial sum of bin bin_j (each starts at +0.0), each bin's 64 lane
// values are folded with xor 32 .. 1.  A result depends only on its two rows, nbins and (t0, T, step).  (No
// MFMA: it would fix another order.)
//
// nw_pac_bins_kernel<T, CAP, KA>: a block owns one epoch of the chunk, one pair, one listed phase scale and
// a tile of 4 * KA listed amplitude scales; wave w of its 4 keeps the amplitude scales w * KA .. of the tile,
// lane = sample of the 64-sample tile.  A lane's partial sums are addressed by a run-time bin, which in
// registers would mean scratch, so they live in LDS: acc[w][bin * KA + k][lane], 8 B apart along the lane and
// 512 B along the row, so a wave's ds_read_b64 / ds_write_b64 differ in the lane term only and never
// conflict.  A wave's amplitude scales are its own, so it forms their magnitudes in registers (one hypot
// per value); what the waves share is the bin index, staged in LDS: in a round of 4 sample tiles wave w
// forms the bins of tile 4 r + w, so the edge tests are paid once per block and spread over its waves.
// Double buffered as nw_pac_kernel: the next round's global loads are issued before the current one is
// accumulated, its bins go to the other buffer after it, one barrier per round.  Every (e, pair, i, k, b)
// belongs to exactly one block of one launch: no atomics, no memset, no read-modify-write of global memory.
#include <algorithm>

#include "nw_reduce_dev.h"

namespace nw {
namespace {

constexpr int kPacBinsThreads = kPacBinsWaves * 64;

// the edge table of the call in LDS (the first nbins threads copy it; the caller's barrier follows)
__device__ __forceinline__ void stage_edges(double2* edge, const double2* __restrict__ cs, int nbins) {
    if ((int)threadIdx.x < nbins) {
        NW_DCHECK(threadIdx.x < (unsigned)kPacBinsMax);
        edge[threadIdx.x] = cs[threadIdx.x];
    }
}

// THE BIN of ninwave.h; edge: the table in LDS (a lane reads edge[base + k]: two addresses per wave)
__device__ __forceinline__ int pac_bin(double re, double im, const double2* edge, int h) {
    const bool upper = im > 0.0 || (im == 0.0 && re > 0.0);
    const int base = upper ? h : 0;
    int bin = base;
#ifdef NW_ABL_PACBINS_NOBIN   // diagnostic A/B of tools/pac_bins_rate.py (wrong bins): no edge tests
    return bin;
#endif
    for (int k = 1; k < h; ++k) {
        NW_DCHECK(base + k >= 0 && base + k < 2 * h && 2 * h <= kPacBinsMax);
        const double2 cs = edge[base + k];
        bin += add_nc(mul_nc(cs.x, im), -mul_nc(cs.y, re)) >= 0.0 ? 1 : 0;
    }
    return re == 0.0 && im == 0.0 ? h : bin;
}

template <typename T, int CAP, int KA>
__global__ __launch_bounds__(kPacBinsThreads) void nw_pac_bins_kernel(
    const cplx<T>* __restrict__ src, double* __restrict__ sum, const int32_t* __restrict__ ip,
    const int32_t* __restrict__ ia, const int32_t* __restrict__ fph, const int32_t* __restrict__ fam,
    const double2* __restrict__ cs, int64_t ec, int nchan, int nfreq, int64_t n_out, int npairs, int nph, int nam,
    int nbins, int64_t t0, int64_t count, int64_t step, int xcd) {
    static_assert(kConnTileN == 64, "lane = sample of the tile");
    constexpr int W = kPacBinsWaves, AM = W * KA;                  // sample tiles of a round, scales of a tile
    __shared__ double acc[W][CAP * KA][kConnTileN];                // [wave][bin * KA + k][lane]
    __shared__ int bins[2][W][kConnTileN];                         // [buffer][sample tile of the round][sample]
    __shared__ double2 edge[CAP];
    static_assert(sizeof acc + sizeof bins + sizeof edge == (size_t)pac_bins_lds(CAP) && pac_bins_geom(CAP).ka == KA &&
                      pac_bins_geom(CAP).cap == CAP,
                  "the geometry of nw_shape.h");

    const int nta = (int)((nam + AM - 1) / AM);
    const PacSlot sl = pac_slot((int64_t)blockIdx.x, npairs, nph * nta, nta, xcd != 0);
    if (sl.e >= ec) return;   // padding of the XCD order (the whole block)
    NW_DCHECK(nbins >= 2 && nbins <= CAP && nbins % 2 == 0);
    NW_DCHECK(sl.e >= 0 && sl.pair >= 0 && sl.pair < npairs && sl.tp >= 0 && sl.tp < nph && sl.ta >= 0 && sl.ta < nta);
    const int64_t e = sl.e;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int h = nbins / 2;
    const int a0 = sl.ta * AM;
    const int naml = min(AM, nam - a0);                            // this tile's amplitude scales
    const int mine = min(KA, naml - w * KA);                       // ... of them this wave's (<= 0: none)
    NW_DCHECK(naml >= 1);
    const int cp = ip[sl.pair], ca = ia[sl.pair];
    NW_DCHECK(cp >= 0 && cp < nchan && ca >= 0 && ca < nchan);
    const int64_t fn = (int64_t)nfreq * n_out;
    const int64_t ntl = conn_time_tiles(count);
    const int64_t nrounds = (ntl + W - 1) / W;

    const int fp = fph[sl.tp];
    NW_DCHECK(fp >= 0 && fp < nfreq);
    const int64_t offp = (e * nchan + cp) * fn + (int64_t)fp * n_out;
    int64_t offa[KA];
#pragma unroll
    for (int k = 0; k < KA; ++k) {
        offa[k] = 0;
        if (k < mine) {
            const int f = fam[a0 + w * KA + k];
            NW_DCHECK(f >= 0 && f < nfreq);
            offa[k] = (e * nchan + ca) * fn + (int64_t)f * n_out;
        }
    }

    stage_edges(edge, cs, nbins);
    for (int row = 0; row < nbins * KA; ++row) {                   // this wave's partial sums start at +0.0
        NW_DCHECK(row < CAP * KA);
        acc[w][row][lane] = 0.0;
    }
    __syncthreads();                                               // the edge table

    // (arrays of structs, as nw_reduce_dev.h's: plain double arrays end in scratch)
    struct Mag { double a; };
    cplx<T> inp, ina[W][KA];
    Mag mag[W][KA];
    // round r: the sample tiles W r .. W r + W - 1; this wave's amplitude rows of all of them and the phase
    // row of tile W r + w; a lane with j >= count loads nothing
    auto load = [&](int64_t r) {
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const int64_t j = (r * W + q) * kConnTileN + lane;
            NW_DCHECK(conn_time_lane(j) == lane);
            const bool live = j < count;
            const int64_t t = t0 + j * step;
#pragma unroll
            for (int k = 0; k < KA; ++k) {
                ina[q][k] = cplx<T>{T(0), T(0)};
                if (k < mine && live) {
                    NW_DCHECK(t >= 0 && t < n_out && offa[k] + t >= 0 && offa[k] + t < ec * nchan * fn);
                    ina[q][k] = src[offa[k] + t];
                }
            }
        }
        const int64_t j = (r * W + w) * kConnTileN + lane;
        inp = cplx<T>{T(0), T(0)};
        if (j < count) {
            const int64_t t = t0 + j * step;
            NW_DCHECK(t >= 0 && t < n_out && offp + t >= 0 && offp + t < ec * nchan * fn);
            inp = src[offp + t];
        }
    };
    // the bins of this wave's sample tile of the round (a lane without a sample: bin h, never read) and
    // the magnitudes of its amplitude rows
    auto store = [&](int buf) {
        NW_DCHECK(buf >= 0 && buf < 2 && w < W && lane < kConnTileN);
        const int b = pac_bin((double)inp.re, (double)inp.im, edge, h);
        NW_DCHECK(b >= 0 && b < nbins);
        bins[buf][w][lane] = b;
#pragma unroll
        for (int q = 0; q < W; ++q)
#pragma unroll
            for (int k = 0; k < KA; ++k)
#ifdef NW_ABL_PACBINS_NOHYPOT   // diagnostic A/B (wrong sums): the magnitudes without their hypot
                mag[q][k].a = fabs((double)ina[q][k].re);
#else
                mag[q][k].a = k < mine ? hypot((double)ina[q][k].re, (double)ina[q][k].im) : 0.0;
#endif
    };

#ifdef NW_ABL_PACBINS_NOLDS
    Mag reg[KA];
#pragma unroll
    for (int k = 0; k < KA; ++k) reg[k].a = 0.0;
#endif
    if (nrounds > 0) {
        load(0);
        store(0);
    }
    __syncthreads();
    for (int64_t r = 0; r < nrounds; ++r) {
        const int cur = (int)(r & 1);
        const bool more = r + 1 < nrounds;
        if (more) load(r + 1);
        if (mine > 0) {
#pragma unroll
            for (int q = 0; q < W; ++q) {
                if ((r * W + q) * kConnTileN + lane < count) {     // a tail sample past the window adds nothing
                    const int b = bins[cur][q][lane];
                    NW_DCHECK(b >= 0 && b < nbins);
#pragma unroll
                    for (int k = 0; k < KA; ++k) {
                        if (k < mine) {
                            NW_DCHECK(b * KA + k < CAP * KA);
#ifdef NW_ABL_PACBINS_NOLDS   // diagnostic A/B (wrong sums): one register accumulator per scale, no LDS update
                            reg[k].a = add_nc(reg[k].a, mag[q][k].a + (double)b);
#else
                            double* const at = &acc[w][b * KA + k][lane];
                            *at = add_nc(*at, mag[q][k].a);
#endif
                        }
                    }
                }
            }
        }
        // the other buffer was last read before the previous barrier
        if (more) store(cur ^ 1);
        __syncthreads();
    }

#ifdef NW_ABL_PACBINS_NOLDS
#pragma unroll
    for (int k = 0; k < KA; ++k) acc[w][k][lane] = reg[k].a;
#endif
    // the fold of every bin (every lane of the wave takes part: the conditions are wave-uniform); lane b
    // keeps bin b's sum and the first nbins lanes write the histogram
#pragma unroll
    for (int k = 0; k < KA; ++k) {
        if (k < mine) {
            double keep = 0.0;
            for (int b = 0; b < nbins; ++b) {
                NW_DCHECK(b * KA + k < CAP * KA);
                const double v = fold64(acc[w][b * KA + k][lane]);
                if (lane == b) keep = v;
            }
            const int64_t cell = ((e * npairs + sl.pair) * nph + sl.tp) * nam + (a0 + w * KA + k);
            NW_DCHECK(cell >= 0 && cell < ec * npairs * nph * nam);
            if (lane < nbins) sum[cell * nbins + lane] = keep;
        }
    }
}

// cnt[((e * C + c) * nph + i) * nbins + b] = the window samples of row fph[i] in bin b: one wave per (epoch,
// channel, listed phase scale), lane = sample of the 64-sample tile.  Per tile and bin the wave counts its
// lanes in that bin (a ballot) and lane b keeps bin b's count: integers, exact in any order.
template <typename T>
__global__ __launch_bounds__(kPacBinsThreads) void nw_pac_bins_rows_kernel(
    const cplx<T>* __restrict__ src, double* __restrict__ cnt, const int32_t* __restrict__ fph,
    const double2* __restrict__ cs, int64_t nsig, int nfreq, int64_t n_out, int nph, int nbins, int64_t t0,
    int64_t count, int64_t step) {
    __shared__ double2 edge[kPacBinsMax];
    NW_DCHECK(nbins >= 2 && nbins <= kPacBinsMax && nbins % 2 == 0);
    stage_edges(edge, cs, nbins);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kPacBinsWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= nsig * nph) return;   // the whole wave
    const int64_t sig = row / nph;
    const int f = fph[row % nph];
    NW_DCHECK(sig >= 0 && sig < nsig && f >= 0 && f < nfreq);
    const int64_t at = (sig * nfreq + f) * n_out;
    const int h = nbins / 2;
    long long mine = 0;
    for (int64_t j0 = 0; j0 < count; j0 += kConnTileN) {
        const int64_t j = j0 + lane;
        int bin = -1;                // a lane without a sample is in no bin
        if (j < count) {
            const int64_t t = t0 + j * step;
            NW_DCHECK(t >= 0 && t < n_out && at + t >= 0 && at + t < nsig * nfreq * n_out);
            const cplx<T> v = src[at + t];
            bin = pac_bin((double)v.re, (double)v.im, edge, h);
            NW_DCHECK(bin >= 0 && bin < nbins);
        }
        for (int b = 0; b < nbins; ++b) {
            const int c = __popcll(__ballot(bin == b));
            if (lane == b) mine += c;
        }
    }
    NW_DCHECK(row * nbins + nbins <= nsig * nph * nbins);
    if (lane < nbins) cnt[row * nbins + lane] = (double)mine;
}

}  // namespace

hipError_t launch_pac_bins(int dtype, const void* src, void* sum, void* cnt, const int32_t* ip, const int32_t* ia,
                           const int32_t* fph, const int32_t* fam, const void* edges, int64_t ec, int nchan, int nfreq,
                           int64_t n_out, int64_t npairs, int nph, int nam, int nbins, int64_t t0, int64_t count,
                           int64_t step, bool xcd, hipStream_t s) {
    if (!pac_bins_valid(nbins)) return hipErrorInvalidValue;
    const int64_t ntiles = pac_bins_tiles(nph, nam, nbins);
    const int64_t blocks = npairs > 0 && ntiles > 0 ? pac_blocks(ec, npairs, ntiles, xcd) : 0;
    const int64_t nrows = cnt ? ec * nchan * nph : 0;
    const int64_t rb = (nrows + kPacBinsWaves - 1) / kPacBinsWaves;
    if (blocks < 0 || blocks > 0x7fffffff || rb > 0x7fffffff || npairs > 0x7fffffff) return hipErrorInvalidValue;
    for_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        auto pairs = [&](auto kernel) {
            nw_launch(kernel, dim3((unsigned)blocks), dim3(kPacBinsThreads), 0, s, (const cplx<T>*)src, (double*)sum, ip, ia,
                      fph, fam, (const double2*)edges, ec, nchan, nfreq, n_out, (int)npairs, nph, nam, nbins, t0, count,
                      step, xcd ? 1 : 0);
        };
        if (blocks > 0) {
            // the three geometry classes of pac_bins_geom
            if (nbins <= 8) pairs(nw_pac_bins_kernel<T, 8, 4>);
            else if (nbins <= 18) pairs(nw_pac_bins_kernel<T, 18, 2>);
            else pairs(nw_pac_bins_kernel<T, kPacBinsMax, 1>);
        }
        if (rb > 0)
            nw_launch(nw_pac_bins_rows_kernel<T>, dim3((unsigned)rb), dim3(kPacBinsThreads), 0, s, (const cplx<T>*)src,
                      (double*)cnt, fph, (const double2*)edges, ec * nchan, nfreq, n_out, nph, nbins, t0, count, step);
    });
    return hipGetLastError();
}

}  // namespace nw
