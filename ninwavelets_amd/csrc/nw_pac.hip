// nw_pac.hip — phase-amplitude coupling (nw_execute_pac): the complex rows of a chunk of epochs x
// channels reduced along the SAMPLE axis into one comodulogram per epoch and channel pair.
//
//   src   [((e * C + c) * F + f) * n_out + t]          complex T: the chunk's rows, epoch-major
//   m     [((e * P + p) * nph + i) * nam + k]          complex fp64: M = sum_j A u
//   amp   [((e * C + c) * nam + k) * 2 ..]             fp64 {sum_j A, sum_j (re^2 + im^2)}
//   phase [(e * C + c) * nph + i]                      complex fp64: sum_j u
// over the window's samples s_j = t0 + j * step, j = 0 .. T - 1, with, in fp64,
//   A = hypot(re, im) of the amplitude channel ia[p]'s row fam[k] at s_j (amp: of channel c),
//   u = (re / h, im / h), h = hypot(re, im), of the phase channel ip[p]'s row fph[i] (phase: of c):
// SUM_PLV's unit phasor (nw_conn_time.hip), NaN where |y| = 0.  Every product (A * u.re, A * u.im,
// re * re, im * im) and every term is rounded on its own (no fma into a sum).
//
// Summation order: that of nw_execute_conn_time (nw_shape.h conn_time_lane): lane l starts at +0.0 and
// adds the terms of j = l, l + 64, ... in that order, the 64 lane values are folded with xor 32 .. 1
// and lane 0 writes.  A result depends only on its rows and on (t0, T, step): not on the pair list,
// the scale lists, the tiling or the chunks.  (No MFMA: it would fix another order.)
//
// nw_pac_kernel: a block owns one epoch of the chunk, one pair and one scale tile (<= kPacPh listed
// phase scales x <= kPacAm listed amplitude scales); wave w of its 4 keeps the tile's amplitude
// scales 4 w .. 4 w + 3 against all 8 phase scales in registers, lane = sample of the 64-sample tile.
// Per sample tile the phase rows are staged in LDS as unit phasors and the amplitude rows as
// magnitudes, so the hypot and the divisions are paid once per staged value and not once per scale
// combination; double buffered as nw_conn_time_kernel, one barrier per sample tile.  Every
// (e, pair, i, k) belongs to exactly one block of one launch: no memset, no read-modify-write.
#include <algorithm>

#include "nw_reduce_dev.h"

namespace nw {
namespace {

constexpr int kPacThreads = kPacWaves * 64;

struct PacAcc { double re, im; };

template <typename T>
__global__ __launch_bounds__(kPacThreads) void nw_pac_kernel(
    const cplx<T>* __restrict__ src, double2* __restrict__ m, const int32_t* __restrict__ ip,
    const int32_t* __restrict__ ia, const int32_t* __restrict__ fph, const int32_t* __restrict__ fam, int64_t ec,
    int nchan, int nfreq, int64_t n_out, int npairs, int nph, int nam, int64_t t0, int64_t count, int64_t step, int xcd) {
    static_assert(kConnTileN == 64, "lane = sample of the tile");
    __shared__ double uph[2][kPacPh][2][kConnTileN];   // [buffer][phase slot][re, im][sample]: 16 KiB
    __shared__ double mag[2][kPacAm][kConnTileN];      // [buffer][amplitude slot][sample]: 16 KiB

    const int nta = (int)pac_tiles_am(nam);
    const PacSlot sl = pac_slot((int64_t)blockIdx.x, npairs, (int)pac_tiles(nph, nam), nta, xcd != 0);
    if (sl.e >= ec) return;   // padding of the XCD order (the whole block)
    NW_DCHECK(sl.e >= 0 && sl.pair >= 0 && sl.pair < npairs && sl.tp >= 0 && sl.tp < pac_tiles_ph(nph) && sl.ta >= 0 &&
              sl.ta < nta);
    const int64_t e = sl.e;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p0 = sl.tp * kPacPh, a0 = sl.ta * kPacAm;
    const int nphl = min(kPacPh, nph - p0), naml = min(kPacAm, nam - a0);   // this tile's scales
    NW_DCHECK(nphl >= 1 && naml >= 1);
    const int cp = ip[sl.pair], ca = ia[sl.pair];
    NW_DCHECK(cp >= 0 && cp < nchan && ca >= 0 && ca < nchan);
    const int64_t fn = (int64_t)nfreq * n_out;
    const int64_t ntl = conn_time_tiles(count);

    // the rows this wave stages: phase slots w, w + 4 and amplitude slots w, w + 4, w + 8, w + 12
    int64_t offp[kPacStagePh], offa[kPacStageAm];
#pragma unroll
    for (int q = 0; q < kPacStagePh; ++q) {
        const int s = w + q * kPacWaves;
        offp[q] = 0;
        if (s < nphl) {
            const int f = fph[p0 + s];
            NW_DCHECK(f >= 0 && f < nfreq);
            offp[q] = (e * nchan + cp) * fn + (int64_t)f * n_out;
        }
    }
#pragma unroll
    for (int q = 0; q < kPacStageAm; ++q) {
        const int s = w + q * kPacWaves;
        offa[q] = 0;
        if (s < naml) {
            const int f = fam[a0 + s];
            NW_DCHECK(f >= 0 && f < nfreq);
            offa[q] = (e * nchan + ca) * fn + (int64_t)f * n_out;
        }
    }

    // (arrays of structs, as nw_reduce_dev.h's: plain double arrays end in scratch)
    PacAcc acc[kPacAmWave][kPacPh];
#pragma unroll
    for (int k = 0; k < kPacAmWave; ++k)
#pragma unroll
        for (int q = 0; q < kPacPh; ++q) acc[k][q].re = acc[k][q].im = 0.0;

    cplx<T> inp[kPacStagePh], ina[kPacStageAm];
    // the samples j = it * 64 + lane of sample tile `it`; a lane with j >= count loads nothing
    auto load = [&](int64_t it) {
        const int64_t j = it * kConnTileN + lane;
        NW_DCHECK(conn_time_lane(j) == lane);
        const bool live = j < count;
        const int64_t t = t0 + j * step;
#pragma unroll
        for (int q = 0; q < kPacStagePh; ++q) {
            inp[q] = cplx<T>{T(0), T(0)};
            if (w + q * kPacWaves < nphl && live) {
                NW_DCHECK(t >= 0 && t < n_out && offp[q] + t >= 0 && offp[q] + t < ec * nchan * fn);
                inp[q] = src[offp[q] + t];
            }
        }
#pragma unroll
        for (int q = 0; q < kPacStageAm; ++q) {
            ina[q] = cplx<T>{T(0), T(0)};
            if (w + q * kPacWaves < naml && live) {
                NW_DCHECK(t >= 0 && t < n_out && offa[q] + t >= 0 && offa[q] + t < ec * nchan * fn);
                ina[q] = src[offa[q] + t];
            }
        }
    };
    // a slot past the tile's scales holds zeros (its sums are never written); a lane without a sample
    // holds 0 / 0, which the accumulation below skips
    auto store = [&](int buf) {
        NW_DCHECK(buf >= 0 && buf < 2 && lane < kConnTileN);
#pragma unroll
        for (int q = 0; q < kPacStagePh; ++q) {
            const int s = w + q * kPacWaves;
            NW_DCHECK(s >= 0 && s < kPacPh);
            double re = 0.0, im = 0.0;
            if (s < nphl) {
                re = (double)inp[q].re, im = (double)inp[q].im;
                const double h = hypot(re, im);
                re /= h, im /= h;
            }
            uph[buf][s][0][lane] = re;
            uph[buf][s][1][lane] = im;
        }
#pragma unroll
        for (int q = 0; q < kPacStageAm; ++q) {
            const int s = w + q * kPacWaves;
            NW_DCHECK(s >= 0 && s < kPacAm);
            mag[buf][s][lane] = s < naml ? hypot((double)ina[q].re, (double)ina[q].im) : 0.0;
        }
    };

    if (ntl > 0) {
        load(0);
        store(0);
    }
    __syncthreads();
    const bool mine = w * kPacAmWave < naml;   // this wave has an amplitude scale of the tile
    for (int64_t it = 0; it < ntl; ++it) {
        const int cur = (int)(it & 1);
        const bool more = it + 1 < ntl;
        if (more) load(it + 1);
        if (mine && it * kConnTileN + lane < count) {   // a tail sample past the window adds nothing
            PacAcc u[kPacPh];
#pragma unroll
            for (int q = 0; q < kPacPh; ++q) u[q] = PacAcc{uph[cur][q][0][lane], uph[cur][q][1][lane]};
#pragma unroll
            for (int k = 0; k < kPacAmWave; ++k) {
                const double a = mag[cur][w * kPacAmWave + k][lane];
#pragma unroll
                for (int q = 0; q < kPacPh; ++q) {
                    acc[k][q].re = add_nc(acc[k][q].re, mul_nc(a, u[q].re));
                    acc[k][q].im = add_nc(acc[k][q].im, mul_nc(a, u[q].im));
                }
            }
        }
        // the other buffer was last read before the previous barrier
        if (more) store(cur ^ 1);
        __syncthreads();
    }

    // the fold (every lane of the wave takes part: the conditions are wave-uniform), lane 0 writes
#pragma unroll
    for (int k = 0; k < kPacAmWave; ++k) {
        const int a = w * kPacAmWave + k;
        if (a < naml) {
#pragma unroll
            for (int q = 0; q < kPacPh; ++q) {
                if (q < nphl) {
                    const double re = fold64(acc[k][q].re), im = fold64(acc[k][q].im);
                    const int64_t at = ((e * npairs + sl.pair) * nph + (p0 + q)) * nam + (a0 + a);
                    NW_DCHECK(at >= 0 && at < ec * npairs * nph * nam);
                    if (lane == 0) m[at] = double2{re, im};
                }
            }
        }
    }
}

// amp[((e * C + c) * nam + k)] = {sum_j A, sum_j |y|^2} of row fam[k], phase[(e * C + c) * nph + i] =
// sum_j u of row fph[i]: one wave per (epoch, channel, listed scale), the order of the contract; the
// second amplitude sum is formed as nw_conn_time_power_kernel forms its power (row_time_sums, nw_reduce_dev.h)
template <typename T>
__global__ __launch_bounds__(kPacThreads) void nw_pac_rows_kernel(
    const cplx<T>* __restrict__ src, double2* __restrict__ amp, double2* __restrict__ phase,
    const int32_t* __restrict__ fph, const int32_t* __restrict__ fam, int64_t nsig, int nfreq, int64_t n_out, int nph,
    int nam, int64_t t0, int64_t count, int64_t step) {
    const int64_t namp = amp ? nsig * nam : 0, nphs = phase ? nsig * nph : 0;
    row_time_sums<kPacWaves>(
        src, namp + nphs, nsig * nfreq * n_out, n_out, t0, count, step,
        [&](int64_t row) {
            const bool is_amp = row < namp;
            const int64_t r = is_amp ? row : row - namp;
            const int nl = is_amp ? nam : nph;
            const int64_t sig = r / nl;
            const int f = (is_amp ? fam : fph)[r % nl];
            NW_DCHECK(sig >= 0 && sig < nsig && f >= 0 && f < nfreq);
            return (sig * nfreq + f) * n_out;
        },
        [&](int64_t row, double& s0, double& s1, double re, double im) {
            const double h = hypot(re, im);
            if (row < namp) {
                s0 = add_nc(s0, h);
                s1 = add_nc(s1, power_term(re, im));
            } else {
                s0 = add_nc(s0, re / h);
                s1 = add_nc(s1, im / h);
            }
        },
        [&](int64_t row, double s0, double s1) {
            *(row < namp ? amp + row : phase + (row - namp)) = double2{s0, s1};
        });
}

}  // namespace

hipError_t launch_pac(int dtype, const void* src, void* m, void* amp, void* phase, const int32_t* ip, const int32_t* ia,
                      const int32_t* fph, const int32_t* fam, int64_t ec, int nchan, int nfreq, int64_t n_out,
                      int64_t npairs, int nph, int nam, int64_t t0, int64_t count, int64_t step, bool xcd,
                      hipStream_t s) {
    const int64_t ntiles = pac_tiles(nph, nam);
    const int64_t blocks = npairs > 0 && ntiles > 0 ? pac_blocks(ec, npairs, ntiles, xcd) : 0;
    const int64_t nsig = ec * nchan;
    const int64_t nrows = (amp ? nsig * nam : 0) + (phase ? nsig * nph : 0);
    const int64_t rb = (nrows + kPacWaves - 1) / kPacWaves;
    if (blocks < 0 || blocks > 0x7fffffff || rb > 0x7fffffff || npairs > 0x7fffffff) return hipErrorInvalidValue;
    for_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (blocks > 0)
            nw_launch(nw_pac_kernel<T>, dim3((unsigned)blocks), dim3(kPacThreads), 0, s, (const cplx<T>*)src, (double2*)m,
                      ip, ia, fph, fam, ec, nchan, nfreq, n_out, (int)npairs, nph, nam, t0, count, step, xcd ? 1 : 0);
        if (rb > 0)
            nw_launch(nw_pac_rows_kernel<T>, dim3((unsigned)rb), dim3(kPacThreads), 0, s, (const cplx<T>*)src,
                      (double2*)amp, (double2*)phase, fph, fam, nsig, nfreq, n_out, nph, nam, t0, count, step);
    });
    return hipGetLastError();
}

}  // namespace nw
