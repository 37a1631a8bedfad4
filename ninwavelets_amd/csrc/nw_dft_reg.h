// nw_dft_reg.h — the register DFT of the on-chip FFT engines: R complex values per thread,
// natural-order input, bit-reversed output.  Plain C++ templates (no inline asm, no amdgcn
// builtins), callable on the host as well, so tests/host/dft_reg_check.cpp checks every
// instantiation against a long-double DFT without a GPU.
//
// Two forms of the same DFT:
//   DIT-FMA (the product form): radix-2 decimation in time on the bit-reversed view of the
//     registers; a non-trivial butterfly is s = u + c*b (4 fma), d = 2u - s (2 fma): 6
//     instructions instead of the DIF form's 8 (add, subtract, constant complex multiply),
//     a pruned first stage is a register copy, and the inter-pass twiddles fold into the
//     first stage (idft_br_tw);
//   DIF (-DNW_DFT_DIF, the form up to round 6): kept as the other arm of tools/ab.sh and as
//     the error yardstick of the host check.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NW_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define NW_HD __attribute__((always_inline)) inline
#endif
#if defined(__clang__)
#define NW_HAVE_F2 1
#else
#define NW_HAVE_F2 0
#endif

namespace nw {
namespace {

template <typename T> struct ScalarOf;
template <typename T> using Sc = typename ScalarOf<T>::type;

#ifdef NW_DFT_DIF   // diagnostic A/B: the radix-2 DIF networks and separate twiddle multiplies
constexpr bool kDftDif = true;
#else
constexpr bool kDftDif = false;
#endif
// The form of one instantiation: the plain entry by (T, R, NZ), the twiddled entry by (T, the
// twiddles' type P, R).  An instantiation that spills or measures slower with the FMA form is
// switched back here, with its numbers.
// NW_DFT_DIF_F64 (defined by nw_large.hip for its own kernels): fp64 keeps the DIF form there.
// The two-pass row kernels sit at 256 VGPRs, and the FMA form moved three of them into
// (more) scratch: rows_kernel<double, 8192, 32, power> 20 -> 24 B, <double, 16384, 32, power>
// 0 -> 12 B, <double, 16384, 16, 4> 232 -> 244 B; with the DIF form they are as before.
#ifdef NW_DFT_DIF_F64
template <typename T> constexpr bool kDifType = kDftDif || sizeof(Sc<T>) == 8;
#else
template <typename T> constexpr bool kDifType = kDftDif;
#endif
template <typename T, int R, int NZ> constexpr bool kUseDif = kDifType<T>;
template <typename T, typename P, int R> constexpr bool kUseDifTw = kDifType<T>;

template <typename T> struct C2 {
    T re, im;
};

// scalar type of a lane value: C2<f2> carries two signals' values of one float element
template <typename T> struct ScalarOf { using type = T; };
#if NW_HAVE_F2
// two fp32 lanes of one VGPR pair: C2<f2> is a PAIR of complex numbers (a.re, b.re),
// (a.im, b.im) on which every butterfly / twiddle template runs as packed math
// (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32: two fp32 operations per instruction)
typedef float f2 __attribute__((ext_vector_type(2)));
template <> struct ScalarOf<f2> { using type = float; };
#endif

template <typename T> NW_HD C2<T> cmul(C2<T> a, C2<T> b) {
    return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
#if NW_HAVE_F2
// a pair of complex numbers (two signals) times one complex number (a shared twiddle):
// the scalar operand is splat across both halves of every packed op
NW_HD C2<f2> cmul(C2<f2> a, C2<float> b) {
    return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
#endif

// explicit fused multiply-add (host and device round alike); scalars splat over a pair
NW_HD float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
NW_HD double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
#if NW_HAVE_F2
NW_HD f2 fma_t(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
NW_HD f2 fma_t(float a, f2 b, f2 c) { return __builtin_elementwise_fma((f2)a, b, c); }
#endif

// cos(2*pi*i/32), i = 0..31
constexpr double kCos32[32] = {
    1.0, 0.98078528040323043, 0.92387953251128674, 0.83146961230254524, 0.70710678118654757,
    0.55557023301960218, 0.38268343236508978, 0.19509032201612825, 0.0, -0.19509032201612825,
    -0.38268343236508978, -0.55557023301960218, -0.70710678118654757, -0.83146961230254524,
    -0.92387953251128674, -0.98078528040323043, -1.0, -0.98078528040323043, -0.92387953251128674,
    -0.83146961230254524, -0.70710678118654757, -0.55557023301960218, -0.38268343236508978,
    -0.19509032201612825, 0.0, 0.19509032201612825, 0.38268343236508978, 0.55557023301960218,
    0.70710678118654757, 0.83146961230254524, 0.92387953251128674, 0.98078528040323043};

template <int R> constexpr int bitrev(int i) {
    int r = 0;
    for (int b = 1; b < R; b <<= 1) {
        r = (r << 1) | (i & 1);
        i >>= 1;
    }
    return r;
}
template <int R> constexpr int ilog2() { return R <= 1 ? 0 : 1 + ilog2<R / 2>(); }

// ---------------------------------------------------------------- DIF (diagnostic arm)
// a * exp(+2 pi i K / LEN) for compile-time K, LEN (LEN | 32); trivial angles special-cased
template <typename T, int K, int LEN>
NW_HD C2<T> twc(C2<T> a) {
    using S = Sc<T>;
    constexpr int idx = K * (32 / LEN);
    if constexpr (idx == 0) {
        return a;
    } else if constexpr (idx == 8) {                  // +i
        return {-a.im, a.re};
    } else if constexpr (idx == 4) {                  // (1+i)/sqrt2
        constexpr S h = (S)0.70710678118654757;
        return {h * (a.re - a.im), h * (a.re + a.im)};
    } else if constexpr (idx == 12) {                 // (-1+i)/sqrt2
        constexpr S h = (S)0.70710678118654757;
        return {-h * (a.re + a.im), h * (a.re - a.im)};
    } else {
        constexpr S c = (S)kCos32[idx];
        constexpr S s = (S)kCos32[(idx + 24) % 32];   // sin(x) = cos(x - pi/2)
        return {a.re * c - a.im * s, a.re * s + a.im * c};
    }
}

// radix-2 DIF butterflies of one stage (half size H), unrolled by template recursion.
// NZ: only the first NZ elements of every group of 2H are nonzero (pruned inputs): a
// butterfly whose partner is zero is a copy plus a twiddle, one with both zero is skipped
// (exact: u + 0 = u), and every group keeps a nonzero prefix of min(NZ, H) after the stage.
template <typename T, int R, int H, int G, int K, int NZ>
NW_HD void dif_bfly(C2<T>* a) {
    if constexpr (G < R) {
        if constexpr (K < H) {
            if constexpr (K + H < NZ) {
                const C2<T> u = a[G + K], w = a[G + K + H];
                a[G + K] = {u.re + w.re, u.im + w.im};
                a[G + K + H] = twc<T, K, 2 * H>(C2<T>{u.re - w.re, u.im - w.im});
            } else if constexpr (K < NZ) {
                a[G + K + H] = twc<T, K, 2 * H>(a[G + K]);
            }
            dif_bfly<T, R, H, G, K + 1, NZ>(a);
        } else {
            dif_bfly<T, R, H, G + 2 * H, 0, NZ>(a);
        }
    }
}

template <typename T, int R, int H, int NZ>
NW_HD void dif_stages(C2<T>* a) {
    if constexpr (H >= 1) {
        dif_bfly<T, R, H, 0, 0, NZ>(a);
        dif_stages<T, R, H / 2, (NZ < H ? NZ : H)>(a);
    }
}

template <typename T, int R, int NZ = R>
NW_HD void idft_br_dif(C2<T>* v) {
    if constexpr (R > 1) dif_stages<T, R, R / 2, NZ>(v);
}

// ---------------------------------------------------------------- DIT with FMA butterflies
// View element i is register v[bitrev<R>(i)]: the view holds the input in bit-reversed order,
// which is what radix-2 DIT consumes, and leaves X in natural order, i.e. v[p] = X[bitrev(p)].
// Stage H (1, 2, .. R/2): group g, k < H: u = view[2Hg + k], b = view[2Hg + k + H],
// c = exp(2 pi i k / 2H): u <- u + c b, b <- u - c b.
// Pruning: before stage H, view element i is the size-H DFT of the inputs bitrev(i - i % H) +
// multiples of R/H, so it is nonzero iff bitrev<R>(i - i % H) < NZ.  Both zero: skipped;
// partner zero: both outputs are u (a register copy); exact, like "u + 0 = u".
template <typename T, int R, int H, int I, int NZ>
NW_HD void dit_bfly(C2<T>* v) {
    if constexpr (I < R) {
        constexpr int K = I % (2 * H);
        if constexpr (K >= H) {
            dit_bfly<T, R, H, I + H, NZ>(v);           // next group
        } else {
            constexpr int iu = bitrev<R>(I), ib = bitrev<R>(I + H);
            constexpr bool nzu = bitrev<R>(I - K) < NZ, nzb = bitrev<R>(I + H - K) < NZ;
            if constexpr (nzu && nzb) {
                const C2<T> u = v[iu], b = v[ib];
                if constexpr (K == 0) {
                    v[iu] = {u.re + b.re, u.im + b.im};
                    v[ib] = {u.re - b.re, u.im - b.im};
                } else if constexpr (2 * K == H) {      // c = +i
                    v[iu] = {u.re - b.im, u.im + b.re};
                    v[ib] = {u.re + b.im, u.im - b.re};
                } else {
                    using S = Sc<T>;
                    constexpr int idx = K * (16 / H);
                    constexpr S cr = (S)kCos32[idx];
                    constexpr S ci = (S)kCos32[(idx + 24) % 32];   // sin(x) = cos(x - pi/2)
                    const C2<T> s{fma_t(-ci, b.im, fma_t(cr, b.re, u.re)), fma_t(ci, b.re, fma_t(cr, b.im, u.im))};
                    v[iu] = s;
                    v[ib] = {fma_t((S)2, u.re, -s.re), fma_t((S)2, u.im, -s.im)};
                }
            } else if constexpr (nzu) {
                v[ib] = v[iu];
            }
            dit_bfly<T, R, H, I + 1, NZ>(v);
        }
    }
}

template <typename T, int R, int H, int NZ>
NW_HD void dit_stages(C2<T>* v) {
    if constexpr (H < R) {
        dit_bfly<T, R, H, 0, NZ>(v);
        dit_stages<T, R, 2 * H, NZ>(v);
    }
}

// inverse DFT of R registers, natural-order input, bit-reversed output:
// v[p] <- X[bitrev<R>(p)], X[n] = sum_r x[r] exp(+2 pi i r n / R); inputs r >= NZ are zero
// (their registers must hold zeros)
template <typename T, int R, int NZ = R>
NW_HD void idft_br_dit(C2<T>* v) {
    dit_stages<T, R, 1, NZ>(v);
}
template <typename T, int R, int NZ = R>
NW_HD void idft_br(C2<T>* v) {
    if constexpr (kUseDif<T, R, NZ>) idft_br_dif<T, R, NZ>(v);
    else idft_br_dit<T, R, NZ>(v);
}

// Twiddle powers w^r (r < R) of one butterfly from the bases p[k] = w^(2^k), handed out pair
// by pair: (w^r, w^(r + R/2)), r < R/2.  w^r is the product of the bases of r's bits (lowest
// first: a chain whose common prefixes the compiler shares), w^(r + R/2) = w^r * p[LR - 1]:
// R - 1 - log2(R) multiplies, and the R powers are never live as a whole.
template <typename P, int R> struct TwPowers {
    using scalar = P;
    static constexpr int LR = ilog2<R>();
    const C2<P>* p;
    NW_HD explicit TwPowers(const C2<P>* bases) : p(bases) {}
    NW_HD C2<P> lo(int r) const {                                  // 1 <= r < R/2
        C2<P> w = p[__builtin_ctz(r)];
#pragma unroll
        for (int k = __builtin_ctz(r) + 1; k < LR - 1; ++k)
            if (r & (1 << k)) w = cmul(w, p[k]);
        return w;
    }
    NW_HD C2<P> hi(int r) const { return r == 0 ? p[LR - 1] : cmul(lo(r), p[LR - 1]); }
};

// idft_br of the twiddled registers v[r] * w(r): W gives w(r) = W.lo(r) (1 <= r < R/2) and
// w(r + R/2) = W.hi(r) (0 <= r < R/2); w(0) = 1.  Stage H = 1 pairs the natural indices
// (r, r + R/2): u = v[r] w(r) (one complex multiply, none for r = 0), s = u + w(r + R/2) v[r + R/2]
// (4 fma with the run-time twiddle), d = 2u - s: one complex multiply per pair less than
// twiddling every element first.
template <typename T, int R, typename W>
NW_HD void idft_br_tw_dit(C2<T>* v, const W& w) {
    static_assert(R >= 2, "a twiddled pass has radix >= 2");
    using S = Sc<T>;
#pragma unroll
    for (int r = 0; r < R / 2; ++r) {
        const C2<T> u = r > 0 ? cmul(v[r], w.lo(r)) : v[r];
        const C2<T> b = v[r + R / 2];
        const auto c = w.hi(r);
        const C2<T> s{fma_t(-c.im, b.im, fma_t(c.re, b.re, u.re)), fma_t(c.im, b.re, fma_t(c.re, b.im, u.im))};
        v[r] = s;
        v[r + R / 2] = {fma_t((S)2, u.re, -s.re), fma_t((S)2, u.im, -s.im)};
    }
    dit_stages<T, R, 2, R>(v);
}
// the DIF arm: every element times its twiddle, then the DIF network
template <typename T, int R, typename W>
NW_HD void idft_br_tw_dif(C2<T>* v, const W& w) {
    static_assert(R >= 2, "a twiddled pass has radix >= 2");
#pragma unroll
    for (int r = 1; r < R / 2; ++r) v[r] = cmul(v[r], w.lo(r));
#pragma unroll
    for (int r = 0; r < R / 2; ++r) v[r + R / 2] = cmul(v[r + R / 2], w.hi(r));
    idft_br_dif<T, R>(v);
}
template <typename T, int R, typename W>
NW_HD void idft_br_tw(C2<T>* v, const W& w) {
    if constexpr (kUseDifTw<T, typename W::scalar, R>) idft_br_tw_dif<T, R>(v, w);
    else idft_br_tw_dit<T, R>(v, w);
}

}  // namespace
}  // namespace nw
