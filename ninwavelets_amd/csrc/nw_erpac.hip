// nw_erpac.hip — event-related phase-amplitude coupling (nw_execute_erpac): the complex rows of a chunk
// of epochs x channels reduced along the EPOCH axis, one value per channel pair, listed (phase scale,
// amplitude scale) and window sample.
//
//   src   [((e * C + c) * F + f) * n_out + t]           complex T: the chunk's rows, epoch-major
//   m     [((p * nph + i) * nam + k) * T + j]           complex fp64: M += sum_e A u
//   amp   [(((c * nam + k) * T + j) * 2 ..]             fp64 {+= sum_e A, += sum_e (re^2 + im^2)}
//   phase [((c * nph + i) * 5 + plane) * T + j]         fp64, the planes += sum_e c, s, c c, s s, c s
// at the window's samples s_j = t0 + j * step, j = 0 .. T - 1, with, in fp64, nw_pac.hip's quantities:
//   A = hypot(re, im) of the amplitude channel ia[p]'s row fam[k] at s_j (amp: of channel c),
//   (c, s) = (re / h, im / h), h = hypot(re, im), of the phase channel ip[p]'s row fph[i] (phase: of c),
//   u = c + i s, NaN where |y| = 0.
// Every product and every term is rounded on its own (no fma into a sum).
//
// Summation order: every output value has one fp64 accumulator; it starts at +0.0 (the host zeroes the
// sums before the first chunk) and adds the epochs' terms in epoch order, a chunk's launch carrying on
// where the previous one stopped.  A value depends only on its rows and on its sample: not on the pair
// list, the scale lists, the tiling, the window or the chunks.  (No MFMA: it would fix another order.)
//
// nw_erpac_kernel: a block owns one pair, one scale tile (<= kPacPh listed phase scales x <= kPacAm listed
// amplitude scales) and kConnTileN = 64 consecutive window samples (lane = sample: with step = 1 every
// global access is lane-contiguous); wave w of its 4 keeps the tile's amplitude scales 4 w .. 4 w + 3
// against all 8 phase scales in registers (64 fp64 a lane), loaded from `m` once per launch and stored
// once, so the read-modify-write of `m` costs one read and one write per chunk, not per epoch.  Per epoch
// the tile's phase rows are staged in LDS as unit phasors and its amplitude rows as magnitudes, so the
// hypot and the divisions are paid once per staged value and not once per scale combination; the staging
// is double buffered: the next epoch's global loads are issued before the current epoch is consumed and
// written to the other buffer after it, one barrier per epoch.  (nw_conn_accumulate_kernel's loop with
// nw_pac_kernel's staging and inner product.)  nw_erpac_rows_kernel adds the per-channel sums: one thread
// per (channel, listed scale, window sample).
#include <algorithm>

#include "nw_reduce_dev.h"

namespace nw {
namespace {

constexpr int kErpacThreads = kPacWaves * 64;
constexpr int kErpacRowThreads = 256;

struct ErpacAcc { double re, im; };

template <typename T>
__global__ __launch_bounds__(kErpacThreads) void nw_erpac_kernel(
    const cplx<T>* __restrict__ src, double2* __restrict__ m, const int32_t* __restrict__ ip,
    const int32_t* __restrict__ ia, const int32_t* __restrict__ fph, const int32_t* __restrict__ fam, int64_t ec,
    int nchan, int nfreq, int64_t n_out, int npairs, int nph, int nam, int64_t t0, int64_t count, int64_t step, int xcd) {
    static_assert(kConnTileN == 64, "lane = sample of the tile");
    __shared__ double uph[2][kPacPh][2][kConnTileN];   // [buffer][phase slot][re, im][sample]: 16 KiB
    __shared__ double mag[2][kPacAm][kConnTileN];      // [buffer][amplitude slot][sample]: 16 KiB

    const int nta = (int)pac_tiles_am(nam);
    const int64_t nst = erpac_sample_tiles(count);
    const ErpacSlot sl = erpac_slot((int64_t)blockIdx.x, nst, (int)pac_tiles(nph, nam), nta, xcd != 0);
    if (sl.pair >= npairs) return;   // padding of the XCD order (the whole block)
    NW_DCHECK(sl.pair >= 0 && sl.st >= 0 && sl.st < nst && sl.tp >= 0 && sl.tp < pac_tiles_ph(nph) && sl.ta >= 0 &&
              sl.ta < nta);
    const int pair = (int)sl.pair;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p0 = sl.tp * kPacPh, a0 = sl.ta * kPacAm;
    const int nphl = min(kPacPh, nph - p0), naml = min(kPacAm, nam - a0);   // this tile's scales
    NW_DCHECK(nphl >= 1 && naml >= 1);
    const int cp = ip[pair], ca = ia[pair];
    NW_DCHECK(cp >= 0 && cp < nchan && ca >= 0 && ca < nchan);
    const int64_t fn = (int64_t)nfreq * n_out;
    const int64_t efn = (int64_t)nchan * fn;         // one epoch of the chunk
    const int64_t j = sl.st * kConnTileN + lane;     // this lane's window sample
    const bool live = j < count;                     // a lane past the window neither loads nor stores
    const int64_t t = t0 + j * step;
    NW_DCHECK(!live || (t >= 0 && t < n_out));

    // the rows this wave stages, at epoch 0: phase slots w, w + 4 and amplitude slots w, w + 4, w + 8, w + 12
    int64_t offp[kPacStagePh], offa[kPacStageAm];
#pragma unroll
    for (int q = 0; q < kPacStagePh; ++q) {
        const int s = w + q * kPacWaves;
        offp[q] = 0;
        if (s < nphl) {
            const int f = fph[p0 + s];
            NW_DCHECK(f >= 0 && f < nfreq);
            offp[q] = (int64_t)cp * fn + (int64_t)f * n_out + t;
        }
    }
#pragma unroll
    for (int q = 0; q < kPacStageAm; ++q) {
        const int s = w + q * kPacWaves;
        offa[q] = 0;
        if (s < naml) {
            const int f = fam[a0 + s];
            NW_DCHECK(f >= 0 && f < nfreq);
            offa[q] = (int64_t)ca * fn + (int64_t)f * n_out + t;
        }
    }

    // the accumulators, from the call's sums (arrays of structs, as nw_reduce_dev.h's: plain double arrays
    // end in scratch)
    const bool mine = w * kPacAmWave < naml;   // this wave has an amplitude scale of the tile
    ErpacAcc acc[kPacAmWave][kPacPh];
#pragma unroll
    for (int k = 0; k < kPacAmWave; ++k) {
        const int a = w * kPacAmWave + k;
#pragma unroll
        for (int q = 0; q < kPacPh; ++q) {
            acc[k][q].re = acc[k][q].im = 0.0;
            if (a < naml && q < nphl && live) {
                const int64_t at = (((int64_t)pair * nph + (p0 + q)) * nam + (a0 + a)) * count + j;
                NW_DCHECK(at >= 0 && at < (int64_t)npairs * nph * nam * count);
                const double2 v = m[at];
                acc[k][q].re = v.x, acc[k][q].im = v.y;
            }
        }
    }

    cplx<T> inp[kPacStagePh], ina[kPacStageAm];
    auto load = [&](int64_t e) {
        NW_DCHECK(e >= 0 && e < ec);
#pragma unroll
        for (int q = 0; q < kPacStagePh; ++q) {
            inp[q] = cplx<T>{T(0), T(0)};
            if (w + q * kPacWaves < nphl && live) {
                NW_DCHECK(e * efn + offp[q] >= 0 && e * efn + offp[q] < ec * efn);
                inp[q] = src[e * efn + offp[q]];
            }
        }
#pragma unroll
        for (int q = 0; q < kPacStageAm; ++q) {
            ina[q] = cplx<T>{T(0), T(0)};
            if (w + q * kPacWaves < naml && live) {
                NW_DCHECK(e * efn + offa[q] >= 0 && e * efn + offa[q] < ec * efn);
                ina[q] = src[e * efn + offa[q]];
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

    if (ec > 0) {
        load(0);
        store(0);
    }
    __syncthreads();
    for (int64_t e = 0; e < ec; ++e) {
        const int cur = (int)(e & 1);
        const bool more = e + 1 < ec;
        if (more) load(e + 1);
        if (mine && live) {
            ErpacAcc u[kPacPh];
#pragma unroll
            for (int q = 0; q < kPacPh; ++q) u[q] = ErpacAcc{uph[cur][q][0][lane], uph[cur][q][1][lane]};
#pragma unroll
            for (int k = 0; k < kPacAmWave; ++k) {
                NW_DCHECK(w * kPacAmWave + k < kPacAm);
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

#pragma unroll
    for (int k = 0; k < kPacAmWave; ++k) {
        const int a = w * kPacAmWave + k;
#pragma unroll
        for (int q = 0; q < kPacPh; ++q) {
            if (a < naml && q < nphl && live) {
                const int64_t at = (((int64_t)pair * nph + (p0 + q)) * nam + (a0 + a)) * count + j;
                NW_DCHECK(at >= 0 && at < (int64_t)npairs * nph * nam * count);
                m[at] = double2{acc[k][q].re, acc[k][q].im};
            }
        }
    }
}

// amp[(c * nam + k) * T + j] += {sum_e A, sum_e |y|^2} of row fam[k], phase[((c * nph + i) * 5 + plane) * T + j]
// += sum_e {c, s, c c, s s, c s} of row fph[i]: one thread per (channel, listed scale, window sample), the
// chunk's epochs added in order, as nw_conn_power_kernel adds its power (the same term: power_term)
template <typename T>
__global__ __launch_bounds__(kErpacRowThreads) void nw_erpac_rows_kernel(
    const cplx<T>* __restrict__ src, double2* __restrict__ amp, double* __restrict__ phase,
    const int32_t* __restrict__ fph, const int32_t* __restrict__ fam, int64_t ec, int nchan, int nfreq, int64_t n_out,
    int nph, int nam, int64_t t0, int64_t count, int64_t step) {
    const int64_t namp = amp ? (int64_t)nchan * nam : 0, nphs = phase ? (int64_t)nchan * nph : 0;
    const int64_t i = (int64_t)blockIdx.x * kErpacRowThreads + threadIdx.x;
    if (i >= (namp + nphs) * count) return;
    const int64_t row = i / count, j = i % count;
    const bool is_amp = row < namp;
    const int64_t r = is_amp ? row : row - namp;
    const int nl = is_amp ? nam : nph;
    const int64_t c = r / nl;
    const int f = (is_amp ? fam : fph)[r % nl];
    const int64_t t = t0 + j * step;
    NW_DCHECK(c >= 0 && c < nchan && f >= 0 && f < nfreq && t >= 0 && t < n_out);
    const int64_t fn = (int64_t)nfreq * n_out, efn = (int64_t)nchan * fn;
    const int64_t at = c * fn + (int64_t)f * n_out + t;
    if (is_amp) {
        NW_DCHECK(r * count + j >= 0 && r * count + j < namp * count);
        double2 s = amp[r * count + j];
        for (int64_t e = 0; e < ec; ++e) {
            NW_DCHECK(e * efn + at >= 0 && e * efn + at < ec * efn);
            const cplx<T> v = src[e * efn + at];
            const double re = (double)v.re, im = (double)v.im;
            s.x = add_nc(s.x, hypot(re, im));
            s.y = add_nc(s.y, power_term(re, im));
        }
        amp[r * count + j] = s;
    } else {
        double* const o = phase + r * 5 * count + j;    // the five planes are `count` apart
        NW_DCHECK(r * 5 * count + 4 * count + j < nphs * 5 * count);
        double sc = o[0], ss = o[count], scc = o[2 * count], sss = o[3 * count], scs = o[4 * count];
        for (int64_t e = 0; e < ec; ++e) {
            NW_DCHECK(e * efn + at >= 0 && e * efn + at < ec * efn);
            const cplx<T> v = src[e * efn + at];
            const double re = (double)v.re, im = (double)v.im;
            const double h = hypot(re, im);
            const double uc = re / h, us = im / h;
            sc = add_nc(sc, uc);
            ss = add_nc(ss, us);
            scc = add_nc(scc, mul_nc(uc, uc));
            sss = add_nc(sss, mul_nc(us, us));
            scs = add_nc(scs, mul_nc(uc, us));
        }
        o[0] = sc, o[count] = ss, o[2 * count] = scc, o[3 * count] = sss, o[4 * count] = scs;
    }
}

}  // namespace

hipError_t launch_erpac(int dtype, const void* src, void* m, void* amp, void* phase, const int32_t* ip,
                        const int32_t* ia, const int32_t* fph, const int32_t* fam, int64_t ec, int nchan, int nfreq,
                        int64_t n_out, int64_t npairs, int nph, int nam, int64_t t0, int64_t count, int64_t step,
                        bool xcd, hipStream_t s) {
    const int64_t ntiles = pac_tiles(nph, nam), nst = erpac_sample_tiles(count);
    const int64_t blocks = npairs > 0 && ntiles > 0 && nst > 0 ? erpac_blocks(npairs, nst, ntiles, xcd) : 0;
    const int64_t nrows = (amp ? (int64_t)nchan * nam : 0) + (phase ? (int64_t)nchan * nph : 0);
    const int64_t rb = (nrows * count + kErpacRowThreads - 1) / kErpacRowThreads;
    if (blocks < 0 || blocks > 0x7fffffff || rb > 0x7fffffff || npairs > 0x7fffffff) return hipErrorInvalidValue;
    for_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (blocks > 0)
            nw_launch(nw_erpac_kernel<T>, dim3((unsigned)blocks), dim3(kErpacThreads), 0, s, (const cplx<T>*)src,
                      (double2*)m, ip, ia, fph, fam, ec, nchan, nfreq, n_out, (int)npairs, nph, nam, t0, count, step,
                      xcd ? 1 : 0);
        if (rb > 0)
            nw_launch(nw_erpac_rows_kernel<T>, dim3((unsigned)rb), dim3(kErpacRowThreads), 0, s, (const cplx<T>*)src,
                      (double2*)amp, (double*)phase, fph, fam, ec, nchan, nfreq, n_out, nph, nam, t0, count, step);
    });
    return hipGetLastError();
}

}  // namespace nw
