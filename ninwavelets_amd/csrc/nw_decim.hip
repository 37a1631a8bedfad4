// nw_decim.hip — the one-pass fused CWT with time decimation folded in (gfx950).
//
// decim = d keeps every d-th output sample (the reference's MorseMNE.cwt passes MNE's decim
// through, wavelets.py:170-191).  With Z = W * X and ND = N / d the kept samples are
//   y[d m] = (1/N) sum_{k' < ND} ( sum_{j < d} Z[k' + j ND] ) e^{2 pi i k' m / ND},   m < ND:
// the ND-point inverse transform of the spectrum folded d times -- exact, no store mask.  Only
// pass 0 (the reads of X and W, one multiply-add per bin) keeps the full length; the on-chip
// FFT, its LDS exchanges and the stores are those of a length-ND row.
//
// Block mapping, signal groups and XCD tiles are nw_fused_kernel's (nw_fused.hip) for the
// transform length ND; W is the plan's full-length table (row stride N, 1/N and the
// interpolate mask folded in) and X the R2C half spectrum (row stride N/2 + 1).
// Open: the X LDS-DMA, a signal-pair variant and partial-sum instantiations.
#include "nw_fft_dev.h"

namespace nw {

namespace {

template <typename T, bool REALW> struct WFold;
template <typename T> struct WFold<T, true> {     // analytic wavelets: real rows
    using type = T;
    __device__ static __forceinline__ void add(C2<T>& v, T w, C2<T> x) {
        v.re += w * x.re;
        v.im += w * x.im;
    }
};
template <typename T> struct WFold<T, false> {    // table wavelets: complex rows
    using type = C2<T>;
    __device__ static __forceinline__ void add(C2<T>& v, C2<T> w, C2<T> x) {
        v.re += w.re * x.re - w.im * x.im;
        v.im += w.re * x.im + w.im * x.re;
    }
};

// E = 32: the loads of a fold are issued kFoldBatch elements at a time, so at most that many X and
// W values are in flight beside the 32 accumulators.  (Batches of 8, 4 or none gave these
// instantiations the same scratch; what they still spill, 28-48 B, is in DESIGN.md §4 Round 8.
// Measured with 4.)
constexpr int kFoldBatch = 4;
// waves per SIMD as nw_fused_kernel's output kernels: 4 (128 VGPRs) fp32, 2 (256) fp64
template <typename T> constexpr int kWpsDecim = sizeof(T) == 8 ? 2 : 4;

// n: the full length (decim * ND); wtt: bins per pass-0 element of the W-support table wnz
// (N / E_N, E_N the elements per thread of the undecimated kernel the table was built for);
// tf x tg: the XCD tile
template <typename T, int ND, int E, int OUT, bool REALW>
__global__ __launch_bounds__(ND / E, (kWpsDecim<T>)) void nw_fused_decim_kernel(
    WDesc d, const cplx<T>* __restrict__ X, const void* __restrict__ wtab, void* __restrict__ out,
    const C2<T>* __restrict__ tw, int64_t nsig, int group, int nsg_pad, const int* __restrict__ wnz, int tf, int tg,
    int decim, int wtt) {
    using G = Geometry<ND, E>;
    using WT = typename WFold<T, REALW>::type;
    extern __shared__ __align__(16) unsigned char smem[];
    T* lds = reinterpret_cast<T*>(smem);
    const int t = threadIdx.x;
    const int n = __builtin_amdgcn_readfirstlane((int)d.n);

    // XCD-aware block -> (scale, signal group): block_slot (nw_shape.h)
    const BlockSlot slot = block_slot(blockIdx.x, d.nfreq, tf, tg);
    const int fi = slot.row, sg = slot.group;
    if (fi >= d.nfreq || sg >= nsg_pad || (int64_t)sg * group >= nsig) return;
    const int64_t s_begin = (int64_t)sg * group;
    // the block's signal count pinned in an SGPR (as nw_fused_pair_kernel: an int64 bound in
    // VGPRs costs registers the E = 32 kernels do not have)
    const int cnt = __builtin_amdgcn_readfirstlane((int)(min(nsig, s_begin + group) - s_begin));

    // folds that reach the row's support: fold j covers bins [j ND, (j + 1) ND), and the bins
    // from wnz[f] * wtt up multiply a W the product kernels treat as zero
    const int reach = (wnz[fi] * wtt + ND - 1) / ND;
    const int nfold = __builtin_amdgcn_readfirstlane(max(1, min(decim, reach)));
    NW_DCHECK(fi < d.nfreq && s_begin + cnt <= nsig && (int64_t)decim * ND == d.n && d.nh == n / 2 + 1);
    NW_DCHECK(nfold >= 1 && nfold <= decim && wnz[fi] >= 1 && (int64_t)wnz[fi] * wtt <= d.n);

    const WT* wrow = reinterpret_cast<const WT*>(wtab) + (int64_t)fi * n;
    const uint32_t wo = (uint32_t)t * (uint32_t)sizeof(WT);
    const uint32_t xo = (uint32_t)t * (uint32_t)sizeof(C2<T>);

    Tab1<T, ND, E>::fill(lds, tw, t);      // read after the first exchange's barriers
    TwSplit<T, ND, E>::fill(lds, tw, t);
    if constexpr (TwSplit<T, ND, E>::ON) lds_barrier();   // read before the first exchange
    const int64_t out_esz = (int64_t)(OUT == NW_OUT_CWT ? sizeof(C2<T>) : sizeof(T));
    for (int i = 0; i < cnt; ++i) {
        const int64_t s = s_begin + i;
        const C2<T>* xs = reinterpret_cast<const C2<T>*>(X + s * d.nh);
        // pass 0: the folded product at k' = t + r*T, then the radix-E IDFT in registers
        C2<T> v[E];
#pragma unroll
        for (int r = 0; r < E; ++r) v[r] = C2<T>{T(0), T(0)};
        for (int j = 0; j < nfold; ++j) {
            const int kb = j * ND;           // the fold's first bin; ND divides N/2, so a fold
            const WT* wj = wrow + kb;        // lies wholly on one side of the Nyquist bin
            NW_DCHECK(kb + (E - 1) * G::T + t < n);
            if (kb + ND <= n / 2) {          // X[k], k < N/2
                const C2<T>* xj = xs + kb;
                NW_DCHECK(kb + (E - 1) * G::T + t < d.nh);
#pragma unroll
                for (int r = 0; r < E; ++r) {
                    const C2<T> x = *at(xj, xo, (uint32_t)(r * G::T * sizeof(C2<T>)));
                    const WT w = *at(wj, wo, (uint32_t)(r * G::T * sizeof(WT)));
                    WFold<T, REALW>::add(v[r], w, x);
                    if (E > 16 && r % kFoldBatch == kFoldBatch - 1) __builtin_amdgcn_sched_barrier(0);
                }
            } else {                         // conj(X[N - k]), k >= N/2 (k = N/2: the stored Nyquist bin)
                const uint32_t mo = (uint32_t)((n - kb) * (int)sizeof(C2<T>)) - xo;
                NW_DCHECK(kb >= n / 2 && n - kb - (E - 1) * G::T - t >= 1 && n - kb - t < d.nh);
#pragma unroll
                for (int r = 0; r < E; ++r) {
                    C2<T> x = *at(xs, mo - (uint32_t)(r * G::T * sizeof(C2<T>)));
                    x.im = -x.im;
                    const WT w = *at(wj, wo, (uint32_t)(r * G::T * sizeof(WT)));
                    WFold<T, REALW>::add(v[r], w, x);
                    if (E > 16 && r % kFoldBatch == kFoldBatch - 1) __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        idft_br<T, E, E>(v);
        NW_DCHECK(s * d.nfreq + fi < nsig * d.nfreq);
        void* ocur = (char*)out + (s * d.nfreq + fi) * (int64_t)ND * out_esz;   // row of signal s: ND points
        // the lane index made opaque per signal: the exchange and store offsets derived from it
        // are then recomputed here (a few VALU ops) instead of staying live, as loop invariants,
        // across pass 0, whose accumulators and loads leave them no registers at E = 32
        int tl = t;
        asm volatile("" : "+v"(tl));
        passes_from<T, ND, E, OUT, 1, false, (sizeof(T) == 8 ? kStoreGlobalNt : kStoreGlobal)>(
            v, lds, tl, tw, nullptr, nullptr, ocur, nullptr);
    }
}

template <typename T, int ND, int E>
hipError_t launch_nd(const WDesc& d, int dtype, int out_kind, int decim, const void* X, const void* wtab, void* out,
                     int64_t nsig, hipStream_t s) {
    if (out_kind != NW_OUT_CWT && out_kind != NW_OUT_POWER && out_kind != NW_OUT_ABS) return hipErrorInvalidValue;
    // the block shape of an undecimated launch of length ND
    FusedShape sh{};
    if (!fused_shape(ND, dtype, nsig, d.nfreq, &sh)) return hipErrorNotSupported;
    void* tw = nullptr;
    hipError_t e = fused_twiddles(ND, dtype, &tw);
    if (e != hipSuccess) return e;
    const int wtt = (int)(d.n / fused_e(d.n, dtype));   // the support table was built for the full length's E
    const bool realw = d.kind != NW_TABLE;
    const int* wnz = wtab_wnz(wtab, d.n, d.nfreq, sizeof(T), realw);
    return for_out_kind(out_kind, [&](auto o) {
        auto go = [&](auto kernel) {
            return nw_launch_lds(kernel, (unsigned)sh.blocks, ND / E, kLdsBytes<T, ND, E>, s, d,
                                 reinterpret_cast<const cplx<T>*>(X), wtab, out, reinterpret_cast<const C2<T>*>(tw),
                                 nsig, sh.group, (int)sh.nsg_pad, wnz, sh.tile_f, sh.tile_g, decim, wtt);
        };
        constexpr int OUT = decltype(o)::value;
        return realw ? go(nw_fused_decim_kernel<T, ND, E, OUT, true>) : go(nw_fused_decim_kernel<T, ND, E, OUT, false>);
    });
}

}  // namespace

// the transform length ND = n / decim is a row of the one-pass size table up to kDecimMaxND
// (decim_supported, nw_shape.h), run at that row's E
hipError_t launch_fused_decim(const WDesc& d, int dtype, int out_kind, int decim, const void* X, const void* wtab,
                              void* out, int64_t nsig, hipStream_t s) {
    if (!decim_supported(d.n, dtype, decim)) return hipErrorNotSupported;
    return for_fused_size(d.n / decim, dtype, hipErrorNotSupported, [&]<typename T, int ND, int E>(FusedSize<T, ND, E>) {
        if constexpr (ND <= kDecimMaxND) return launch_nd<T, ND, E>(d, dtype, out_kind, decim, X, wtab, out, nsig, s);
        else return hipErrorNotSupported;
    });
}

}  // namespace nw
