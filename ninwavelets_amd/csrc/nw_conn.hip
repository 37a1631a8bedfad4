// nw_conn.hip — multi-channel connectivity (nw_execute_conn): the complex rows of a chunk of
// epochs x channels reduced into the cross sums of MANY channel pairs at once.
//
//   src   [((e * C + c) * F + f) * n_out + t]   complex T: the chunk's rows, epoch-major
//   cross [(p * F + f) * n_out + t]             complex fp64: S_p (PLV: Phi_p), p = (ia[p], ib[p])
//   power [(c * F + f) * n_out + t]             fp64: P_cc (not for PLV)
//   SUM_LAG: cross [((p * F + f) * n_out + t) * 4 ..] fp64 {L0, L1, L2, L3} = the sums over the epochs
//   of m, |m|, m^2, sgn m with m = Im y_a conj(y_b) (the imaginary term of S_p); no power
//
// Per pair and epoch the terms are k_accumulate_pair's (nw_kernels.hip), added in epoch order:
// fp64 values, every product and every term rounded on its own (no fma into the sum), for PLV
// each value divided by its hypot first.  A pair's sums are therefore the bits nw_execute_pair
// gives for the same two channels on its per-signal-rows path, however the epochs are chunked.
//
// nw_conn_accumulate_kernel: a block owns one scale f, kConnTileN = 64 consecutive samples
// (lane = sample: every global and LDS access is lane-contiguous) and one pair tile (<= 64 pairs
// over <= 16 distinct channels, host::conn_tiles).  Wave w of its 4 keeps the accumulators of the
// pairs w, w + 4, ... in registers (<= 16 pairs x 2 doubles), loaded from `cross` once per launch
// and stored once, so the read-modify-write of `cross` costs one read and one write per chunk,
// not per epoch.  Per epoch the tile's channels are staged once in LDS as fp64 (PLV: as unit
// phasors, so a value is normalised once, not once per pair it enters); the staging is double
// buffered: the next epoch's global loads are issued before the current epoch is consumed and
// written to the other buffer after it, one barrier per epoch.  SUM_LAG stages as the cross mode
// does and keeps 16 pairs x 4 doubles a wave (128 accumulator registers, at a lower occupancy: no
// second sweep of the epochs); a lane reads and writes its 32 B per pair as two 16-byte accesses.
// nw_conn_power_kernel adds P_cc: one thread per (c, f, t).
#include <algorithm>

#include "nw_reduce_dev.h"

namespace nw {
namespace {

// (the SUM_* staging, accumulators and per-pair terms are the policies of nw_reduce_dev.h, shared with
// nw_conn_time_kernel; the epoch loop tiles otherwise than the over-time skeleton and stays here.  The
// accumulators are an array of structs: two plain double[16] are rewritten into <16 x double> vectors
// before the loops unroll and then live in 32-register tuples, 1412 B of scratch; tools/regs.py)
template <typename T, int MODE>
__global__ __launch_bounds__(kConnThreads) void nw_conn_accumulate_kernel(
    const cplx<T>* __restrict__ src, double2* __restrict__ cross, const ConnTile* __restrict__ tiles, int ntiles,
    int64_t ec, int nchan, int nfreq, int64_t n_out, int64_t npairs, int64_t nunits, int xcd) {
    static_assert(kConnTileN == 64, "lane = sample of the tile");
    using P = SumPolicy<MODE>;
    constexpr int NV = P::kOut;   // double2 values per pair and point in `cross`
    __shared__ double stage[2][kConnCh][2][kConnTileN];   // [buffer][slot][re, im][sample]: 32 KiB

    const ConnSlot sl = conn_slot((int64_t)blockIdx.x, ntiles, xcd != 0);
    if (sl.unit >= nunits) return;   // padding of the XCD order (the whole block)
    NW_DCHECK(sl.tile >= 0 && sl.tile < ntiles);
    const int64_t ntn = (n_out + kConnTileN - 1) / kConnTileN;
    const int f = (int)(sl.unit / ntn);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t t = (sl.unit % ntn) * kConnTileN + lane;
    const bool live = t < n_out;     // samples past the row's end are neither read nor written
    NW_DCHECK(f >= 0 && f < nfreq);
    const ConnTile& tile = tiles[sl.tile];
    const int nch = tile.nch, np = tile.npairs;
    NW_DCHECK(nch >= 0 && nch <= kConnCh && np >= 0 && np <= kConnPairs);
    const int64_t fn = (int64_t)nfreq * n_out;
    const int64_t ft = (int64_t)f * n_out + t;

    // SUM_LAG: four doubles per pair, 128 accumulator registers a lane
    typename P::Acc acc[kConnPerWave];
#pragma unroll
    for (int k = 0; k < kConnPerWave; ++k) {
        const int j = w + k * kConnWaves;
        P::zero(acc[k]);
        if (j < np && live) {
            const int64_t o = tile.out[j];
            NW_DCHECK(o >= 0 && o < npairs && o * fn + ft < npairs * fn);
            NW_DCHECK(NV * (o * fn + ft) + NV - 1 < NV * npairs * fn);
            P::load(acc[k], cross + NV * (o * fn + ft));
        }
    }

    cplx<T> in[kConnStage];
    auto load = [&](int64_t e) {
#pragma unroll
        for (int q = 0; q < kConnStage; ++q) {
            const int s = w + q * kConnWaves;
            in[q] = cplx<T>{T(0), T(0)};
            if (s < nch && live) {
                const int64_t c = tile.ch[s];
                NW_DCHECK(c >= 0 && c < nchan && e >= 0 && e < ec && (e * nchan + c) * fn + ft < ec * nchan * fn);
                in[q] = src[(e * nchan + c) * fn + ft];
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int q = 0; q < kConnStage; ++q) {
            const int s = w + q * kConnWaves;
            if (s < nch) P::stage(in[q], stage[buf][s], lane);
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
#pragma unroll
        for (int k = 0; k < kConnPerWave; ++k) {
            const int j = w + k * kConnWaves;
            if (j < np) {
                const int a = tile.sa[j], b = tile.sb[j];
                NW_DCHECK(a >= 0 && a < nch && b >= 0 && b < nch);
                P::term(acc[k], stage[cur][a], stage[cur][b], lane);
            }
        }
        // the other buffer was last read before the previous barrier
        if (more) store(cur ^ 1);
        __syncthreads();
    }

#pragma unroll
    for (int k = 0; k < kConnPerWave; ++k) {
        const int j = w + k * kConnWaves;
        if (j < np && live) {
            const int64_t o = tile.out[j];
            NW_DCHECK(o >= 0 && o < npairs && o * fn + ft < npairs * fn);
            NW_DCHECK(NV * (o * fn + ft) + NV - 1 < NV * npairs * fn);
            P::store(acc[k], cross + NV * (o * fn + ft));
        }
    }
}

// power[c, f, t] += sum_e |y_{e,c}[f, t]|^2, the term k_accumulate_pair adds to P_aa
template <typename T>
__global__ __launch_bounds__(256) void nw_conn_power_kernel(const cplx<T>* __restrict__ src, double* __restrict__ power,
                                                            int64_t ec, int nchan, int64_t fn) {
    const int64_t count = (int64_t)nchan * fn;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        NW_DCHECK(i >= 0 && i < count);
        double p = power[i];
        for (int64_t e = 0; e < ec; ++e) {
            NW_DCHECK(e * count + i < ec * count);
            const cplx<T> v = src[e * count + i];
            const double re = (double)v.re, im = (double)v.im;
            p += power_term(re, im);
        }
        power[i] = p;
    }
}

}  // namespace

hipError_t launch_conn_accumulate(int dtype, int mode, const void* src, void* cross, double* power,
                                  const ConnTile* tiles, int ntiles, int64_t ec, int nchan, int nfreq, int64_t n_out,
                                  int64_t npairs, bool xcd, hipStream_t s) {
    const int64_t nunits = conn_units(nfreq, n_out);
    const int64_t blocks = ntiles > 0 ? conn_blocks(nunits, ntiles, xcd) : 0;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    for_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (blocks > 0)
            for_sum_mode(mode, [&](auto v) {
                nw_launch(nw_conn_accumulate_kernel<T, decltype(v)::value>, dim3((unsigned)blocks), dim3(kConnThreads), 0, s,
                          (const cplx<T>*)src, (double2*)cross, tiles, ntiles, ec, nchan, nfreq, n_out, npairs, nunits,
                          xcd ? 1 : 0);
            });
        if (power && mode != SUM_LAG) {   // the phase-lag sums carry no power
            const int64_t fn = (int64_t)nfreq * n_out;
            const int64_t pb = std::max<int64_t>(1, std::min<int64_t>(((int64_t)nchan * fn + 255) / 256, 256 * 32));
            nw_launch(nw_conn_power_kernel<T>, dim3((unsigned)pb), dim3(256), 0, s, (const cplx<T>*)src, power, ec, nchan, fn);
        }
    });
    return hipGetLastError();
}

}  // namespace nw
