// nw_pac_surr.hip — time-lag surrogates of the phase-amplitude coupling (nw_execute_pac_surr): nw_execute_pac's
// sum with the amplitude shifted circularly inside the window, once per listed lag, and the statistics of
// the surrogate values per cell.
//
//   src    [((e * C + c) * F + f) * n_out + t]                complex T: the chunk's rows, epoch-major
//   stage  pac_surr_phase_at / pac_surr_amp_at (nw_shape.h)    fp64: unit phasors and magnitudes in window order
//   m      [((e * P + p) * nph + i) * nam + k]                 complex fp64: M_0 = nw_execute_pac's M
//   stat   [(((e * P + p) * nph + i) * nam + k) * 4 ..]        fp64 {sum_s h_s, sum_s q_s, #{s : q_s >= q_0}, max_s q_s}
//   all    [(((e * P + p) * nph + i) * nam + k) * nlags + s]   complex fp64: M_{lags[s]}
// with M_l = sum_j A[(j + l) mod T] u[j] over the window indices j = 0 .. T - 1, A and u nw_execute_pac's, every
// product rounded on its own and the sum in nw_execute_conn_time's order on j (nw_shape.h conn_time_lane), so that
// M_0 is nw_pac_kernel's M bit for bit; Mc_l = M_l, or M_l - D with D = ((P.re S_A) / T, (P.im S_A) / T) of the
// pair's sum u and sum A (NW_PAC_SURR_DEBIASED), q_l = Mc.re Mc.re + Mc.im Mc.im, h_l = sqrt(q_l).
//
// nw_pac_stage_kernel pays the hypot and the divisions of nw_pac_kernel's staging once per chunk: every
// signal's listed rows as unit phasors / magnitudes, formed as nw_pac_kernel::store forms them, compacted to
// window order.  nw_pac_surr_kernel is nw_pac_kernel's block (one epoch, one pair, one 8 x 16 scale tile, wave w
// the amplitude slots 4 w .. 4 w + 3, lane = sample of the 64-sample tile, double-buffered LDS staging, one
// barrier per sample tile) looping over the lags l = 0, lags[0], lags[1], ...: the amplitude tile of lag l is
// read at pac_surr_wrap(j, l, T).  After each lag's fold every lane holds the totals; lane
// pac_surr_cell_lane(k, q) keeps cell (k, q)'s q_0 and statistics in registers and writes them once.  Every
// value belongs to exactly one lane of one block of one launch: no memset, no read-modify-write.
#include <algorithm>

#include "nw_reduce_dev.h"

namespace nw {
namespace {

constexpr int kPacThreads = kPacWaves * 64;

struct PacAcc { double re, im; };

// st: the staged planes of the chunk's nsig signals; a thread owns sample j of one listed row
template <typename T>
__global__ __launch_bounds__(kPacSurrStageThreads) void nw_pac_stage_kernel(
    const cplx<T>* __restrict__ src, double* __restrict__ st, const int32_t* __restrict__ fph,
    const int32_t* __restrict__ fam, int64_t nsig, int nfreq, int64_t n_out, int nph, int nam, int64_t t0, int64_t count,
    int64_t step) {
    const int64_t tiles = pac_surr_stage_tiles(count);
    const int64_t row = (int64_t)blockIdx.x / tiles;
    const int64_t j = ((int64_t)blockIdx.x % tiles) * kPacSurrStageThreads + threadIdx.x;
    NW_DCHECK(row >= 0 && row < nsig * (nph + nam));
    if (j >= count) return;
    const int64_t nphs = nsig * nph;
    const bool is_phase = row < nphs;
    const int64_t r = is_phase ? row : row - nphs;
    const int nl = is_phase ? nph : nam;
    const int64_t sig = r / nl;
    const int pos = (int)(r % nl);
    const int f = (is_phase ? fph : fam)[pos];
    const int64_t t = t0 + j * step;
    NW_DCHECK(sig >= 0 && sig < nsig && f >= 0 && f < nfreq && t >= 0 && t < n_out);
    const cplx<T> v = src[(sig * nfreq + f) * n_out + t];
    double re = (double)v.re, im = (double)v.im;
    const double h = hypot(re, im);
    if (is_phase) {
        re /= h, im /= h;
        const int64_t at = pac_surr_phase_at(sig, pos, 0, nph, count) + j;
        NW_DCHECK(at >= 0 && at + count < pac_surr_stage_doubles(nsig, nph, nam, count));
        st[at] = re;
        st[at + count] = im;
    } else {
        const int64_t at = pac_surr_amp_at(nsig, sig, pos, nph, nam, count) + j;
        NW_DCHECK(at >= 0 && at < pac_surr_stage_doubles(nsig, nph, nam, count));
        st[at] = h;
    }
}

// psum, asum: the chunk's (ec, C, nph) sum u and (ec, C, nam) {sum A, sum A^2} (nw_pac_rows_kernel's), read for D
__global__ __launch_bounds__(kPacThreads) void nw_pac_surr_kernel(
    const double* __restrict__ st, const double2* __restrict__ psum, const double2* __restrict__ asum,
    const int64_t* __restrict__ lags, int nlags, int centre, double2* __restrict__ m, double2* __restrict__ stat,
    double2* __restrict__ all, const int32_t* __restrict__ ip, const int32_t* __restrict__ ia, int64_t ec, int nchan,
    int npairs, int nph, int nam, int64_t count, int xcd) {
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
    const int64_t nsig = ec * nchan;
    [[maybe_unused]] const int64_t total = pac_surr_stage_doubles(nsig, nph, nam, count);   // (the checks)
    const int64_t ntl = conn_time_tiles(count);

    // the staged rows this wave copies to LDS: phase slots w, w + 4 and amplitude slots w, w + 4, w + 8, w + 12
    int64_t offp[kPacStagePh], offa[kPacStageAm];
#pragma unroll
    for (int q = 0; q < kPacStagePh; ++q) {
        const int s = w + q * kPacWaves;
        offp[q] = s < nphl ? pac_surr_phase_at(e * nchan + cp, p0 + s, 0, nph, count) : 0;
    }
#pragma unroll
    for (int q = 0; q < kPacStageAm; ++q) {
        const int s = w + q * kPacWaves;
        offa[q] = s < naml ? pac_surr_amp_at(nsig, e * nchan + ca, a0 + s, nph, nam, count) : 0;
    }

    // the cell this lane keeps: amplitude slot w * 4 + (lane >> 3) x phase slot (lane & 7) of the tile
    const int ck = lane / kPacPh, cq = lane % kPacPh;
    const bool own = ck < kPacAmWave && w * kPacAmWave + ck < naml && cq < nphl;
    NW_DCHECK(!own || pac_surr_cell_lane(ck, cq) == lane);
    const int64_t cell = ((e * npairs + sl.pair) * nph + (p0 + cq)) * nam + (a0 + w * kPacAmWave + ck);
    NW_DCHECK(!own || (cell >= 0 && cell < ec * npairs * nph * nam));
    double dre = 0.0, dim = 0.0;   // D of the debiased centring
    if (own && centre != NW_PAC_SURR_PLAIN) {
        const double2 P = psum[(e * nchan + cp) * nph + (p0 + cq)];
        const double SA = asum[(e * nchan + ca) * nam + (a0 + w * kPacAmWave + ck)].x;
        const double Td = (double)count;
        dre = mul_nc(P.x, SA) / Td;
        dim = mul_nc(P.y, SA) / Td;
    }
    double q0 = 0.0, sh = 0.0, sq = 0.0, cnt = 0.0, mx = 0.0;

    // (arrays of structs, as nw_reduce_dev.h's: plain double arrays end in scratch)
    PacAcc acc[kPacAmWave][kPacPh];
#pragma unroll
    for (int k = 0; k < kPacAmWave; ++k)
#pragma unroll
        for (int q = 0; q < kPacPh; ++q) acc[k][q].re = acc[k][q].im = 0.0;

    PacAcc inp[kPacStagePh];
    double ina[kPacStageAm];
    // the terms j = it * 64 + lane of sample tile `it` at the lag l: u[j] and A[(j + l) mod T]; a lane with
    // j >= count loads nothing
    auto load = [&](int64_t it, int64_t l) {
        const int64_t j = it * kConnTileN + lane;
        NW_DCHECK(conn_time_lane(j) == lane && l >= 0 && (l < count || count == 0));
        const bool live = j < count;
        const int64_t jj = pac_surr_wrap(j, l, count);
#pragma unroll
        for (int q = 0; q < kPacStagePh; ++q) {
            inp[q] = PacAcc{0.0, 0.0};
            if (w + q * kPacWaves < nphl && live) {
                NW_DCHECK(offp[q] + j >= 0 && offp[q] + count + j < total);
                inp[q] = PacAcc{st[offp[q] + j], st[offp[q] + count + j]};
            }
        }
#pragma unroll
        for (int q = 0; q < kPacStageAm; ++q) {
            ina[q] = 0.0;
            if (w + q * kPacWaves < naml && live) {
                NW_DCHECK(jj >= 0 && jj < count && offa[q] + jj >= 0 && offa[q] + jj < total);
                ina[q] = st[offa[q] + jj];
            }
        }
    };
    // a slot past the tile's scales and a lane without a sample hold zeros (the accumulation skips the lane)
    auto store = [&](int buf) {
        NW_DCHECK(buf >= 0 && buf < 2 && lane < kConnTileN);
#pragma unroll
        for (int q = 0; q < kPacStagePh; ++q) {
            const int s = w + q * kPacWaves;
            NW_DCHECK(s >= 0 && s < kPacPh);
            uph[buf][s][0][lane] = inp[q].re;
            uph[buf][s][1][lane] = inp[q].im;
        }
#pragma unroll
        for (int q = 0; q < kPacStageAm; ++q) {
            const int s = w + q * kPacWaves;
            NW_DCHECK(s >= 0 && s < kPacAm);
            mag[buf][s][lane] = ina[q];
        }
    };

    if (ntl > 0) {
        load(0, 0);
        store(0);
    }
    __syncthreads();
    const bool mine = w * kPacAmWave < naml;   // this wave has an amplitude scale of the tile
    int cur = 0;
    int64_t l = 0;
    // s = -1: the lag 0 of M itself (q_0); s >= 0: the listed lags in list order
    for (int s = -1; s < nlags; ++s) {
        const bool more_lags = s + 1 < nlags;
        const int64_t lnext = more_lags ? lags[s + 1] : 0;
        for (int64_t it = 0; it < ntl; ++it) {
            const bool last = it + 1 == ntl;
            const bool more = !last || more_lags;
            if (more) load(last ? 0 : it + 1, last ? lnext : l);
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
            cur ^= 1;
        }
        l = lnext;
        if (!mine) continue;   // (wave-uniform)

        // the fold (every lane of the wave takes part: the conditions are wave-uniform); each cell's lane
        // keeps its totals, and the accumulators start the next lag at +0.0
        double mre = 0.0, mim = 0.0;
#pragma unroll
        for (int k = 0; k < kPacAmWave; ++k) {
#pragma unroll
            for (int q = 0; q < kPacPh; ++q) {
                if (w * kPacAmWave + k < naml && q < nphl) {
                    const double re = fold64(acc[k][q].re), im = fold64(acc[k][q].im);
                    if (lane == pac_surr_cell_lane(k, q)) mre = re, mim = im;
                }
                acc[k][q].re = acc[k][q].im = 0.0;
            }
        }
        if (own) {
            const double cre = add_nc(mre, -dre), cim = add_nc(mim, -dim);   // (D = +0.0: M itself)
            const double q = add_nc(mul_nc(cre, cre), mul_nc(cim, cim));
            if (s < 0) {
                q0 = q;
                m[cell] = double2{mre, mim};
            } else {
                sh = add_nc(sh, __dsqrt_rn(q));
                sq = add_nc(sq, q);
                if (q >= q0) cnt = add_nc(cnt, 1.0);
                if (q > mx) mx = q;
                if (all) {
                    NW_DCHECK(cell * nlags + s < ec * npairs * nph * nam * nlags);
                    all[cell * nlags + s] = double2{mre, mim};
                }
            }
        }
    }
    if (own && stat) {
        stat[2 * cell] = double2{sh, sq};
        stat[2 * cell + 1] = double2{cnt, mx};
    }
}

}  // namespace

hipError_t launch_pac_surr(int dtype, const void* src, void* stage, void* m, void* amp, void* phase, void* stat, void* all,
                           const int32_t* ip, const int32_t* ia, const int32_t* fph, const int32_t* fam,
                           const int64_t* lags, int nlags, int centre, int64_t ec, int nchan, int nfreq, int64_t n_out,
                           int64_t npairs, int nph, int nam, int64_t t0, int64_t count, int64_t step, bool xcd,
                           hipStream_t s) {
    const int64_t ntiles = pac_tiles(nph, nam);
    const int64_t blocks = npairs > 0 && ntiles > 0 ? pac_blocks(ec, npairs, ntiles, xcd) : 0;
    const int64_t nsig = ec * nchan;
    const int64_t sb = blocks > 0 ? pac_surr_stage_blocks(nsig * (nph + nam), count) : 0;
    if (blocks < 0 || blocks > 0x7fffffff || sb > 0x7fffffff || npairs > 0x7fffffff || !amp || !phase)
        return hipErrorInvalidValue;
    // the per-channel sums (nw_pac_rows_kernel): the caller's, and what D is formed from
    hipError_t err = launch_pac(dtype, src, nullptr, amp, phase, ip, ia, fph, fam, ec, nchan, nfreq, n_out, 0, nph, nam,
                                t0, count, step, xcd, s);
    if (err != hipSuccess) return err;
    for_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (sb > 0)
            nw_launch(nw_pac_stage_kernel<T>, dim3((unsigned)sb), dim3(kPacSurrStageThreads), 0, s, (const cplx<T>*)src,
                      (double*)stage, fph, fam, nsig, nfreq, n_out, nph, nam, t0, count, step);
    });
    if (blocks > 0)
        nw_launch(nw_pac_surr_kernel, dim3((unsigned)blocks), dim3(kPacThreads), 0, s, (const double*)stage,
                  (const double2*)phase, (const double2*)amp, lags, nlags, centre, (double2*)m, (double2*)stat,
                  (double2*)all, ip, ia, ec, nchan, (int)npairs, nph, nam, count, xcd ? 1 : 0);
    return hipGetLastError();
}

}  // namespace nw
