// Host check of the register DFT (ninwavelets_amd/csrc/nw_dft_reg.h): every (T, R, NZ) the
// kernels instantiate, the plain and the twiddled entry, against a direct O(R^2) DFT in long
// double.  Driven by tests/test_dft_reg_host.py; prints one line per case and exits non-zero
// on a failed check.
//   error:  rms relative error of the product form (idft_br / idft_br_tw) over the trials must
//           not exceed 1.5 x the DIF form's on the same inputs;
//   zeros:  with r >= NZ zeroed, idft_br<T, R, NZ> must equal idft_br<T, R, R> on the same
//           padded input to <= 2 ulp of the output norm.
//   usage: dft_reg_check [trials]
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nw_dft_reg.h"

using namespace nw;

namespace {

constexpr double kBound = 1.5;
int g_trials = 400;
int g_fail = 0;

// fixed seeded inputs: splitmix64 -> uniform in [-1, 1)
struct Rng {
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uni() { return (double)(next() >> 11) * (1.0 / 4503599627370496.0) - 1.0; }
};

struct LC { long double re, im; };
LC lmul(LC a, LC b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
LC lexp(long double rev) {   // exp(2 pi i rev)
    const long double a = 2.0L * 3.14159265358979323846264338327950288L * rev;
    return {cosl(a), sinl(a)};
}

// lanes of a value type: 1 for float / double, 2 for f2
template <typename T> struct Lanes {
    static constexpr int n = 1;
    static constexpr const char* name = sizeof(T) == 4 ? "float" : "double";
    static T get(T v, int) { return v; }
    static void set(T& v, int, T x) { v = x; }
};
#if NW_HAVE_F2
template <> struct Lanes<f2> {
    static constexpr int n = 2;
    static constexpr const char* name = "f2";
    static float get(f2 v, int h) { return h ? v.y : v.x; }
    static void set(f2& v, int h, float x) { if (h) v.y = x; else v.x = x; }
};
#endif
template <typename S> constexpr long double eps_of() { return sizeof(S) == 4 ? (long double)FLT_EPSILON : (long double)DBL_EPSILON; }

// sum over lanes and outputs of |got - ref|^2 and |ref|^2; ref[h][n] = X[n] of lane h
template <typename T, int R>
void accumulate(const C2<T>* got, const std::vector<LC>* ref, long double& e2, long double& n2) {
    for (int h = 0; h < Lanes<T>::n; ++h)
        for (int p = 0; p < R; ++p) {
            const LC want = ref[h][bitrev<R>(p)];
            const long double dr = (long double)Lanes<T>::get(got[p].re, h) - want.re;
            const long double di = (long double)Lanes<T>::get(got[p].im, h) - want.im;
            e2 += dr * dr + di * di;
            n2 += want.re * want.re + want.im * want.im;
        }
}

// X[n] = sum_r x[r] exp(+2 pi i r n / R)
template <int R> std::vector<LC> direct_dft(const LC* x) {
    static const std::vector<LC> root = [] {
        std::vector<LC> w(R);
        for (int k = 0; k < R; ++k) w[k] = lexp((long double)k / R);
        return w;
    }();
    std::vector<LC> X(R);
    for (int n = 0; n < R; ++n) {
        LC acc{0, 0};
        for (int r = 0; r < R; ++r) {
            const LC t = lmul(x[r], root[(r * n) % R]);
            acc.re += t.re;
            acc.im += t.im;
        }
        X[n] = acc;
    }
    return X;
}

void report(const char* kind, const char* tname, int R, int NZ, long double en, long double ed) {
    const double ratio = ed > 0 ? (double)(en / ed) : (en == 0 ? 1.0 : INFINITY);
    const bool ok = en <= kBound * ed;
    std::printf("%-7s %-6s R=%-2d NZ=%-2d  new %.3Le  dif %.3Le  ratio %.3f%s\n", kind, tname, R, NZ, en, ed, ratio,
                ok ? "" : "  FAIL");
    if (!ok) ++g_fail;
}

// ---- the plain entry with pruned inputs
template <typename T, int R, int NZ> void check_plain() {
    using S = Sc<T>;
    using L = Lanes<T>;
    Rng rng{0x1234u + 131u * R + NZ + 7u * sizeof(S) + L::n};
    long double e_new = 0, e_dif = 0, n2 = 0, n2b = 0;
    long double worst_zero = 0;
    for (int trial = 0; trial < g_trials; ++trial) {
        C2<T> a[R], b[R], full[R];
        LC x[2][R];
        for (int r = 0; r < R; ++r) {
            a[r] = C2<T>{};
            for (int h = 0; h < L::n; ++h) {
                const S re = r < NZ ? (S)rng.uni() : (S)0, im = r < NZ ? (S)rng.uni() : (S)0;
                L::set(a[r].re, h, re);
                L::set(a[r].im, h, im);
                x[h][r] = LC{(long double)re, (long double)im};
            }
            b[r] = a[r];
            full[r] = a[r];
        }
        std::vector<LC> ref[2];
        for (int h = 0; h < L::n; ++h) ref[h] = direct_dft<R>(x[h]);
        idft_br<T, R, NZ>(a);
        idft_br_dif<T, R, NZ>(b);
        idft_br<T, R, R>(full);
        accumulate<T, R>(a, ref, e_new, n2);
        accumulate<T, R>(b, ref, e_dif, n2b);
        // zero stays zero: the pruned network against the full one on the same padded input
        for (int h = 0; h < L::n; ++h) {
            long double norm2 = 0, dmax = 0;
            for (int p = 0; p < R; ++p) {
                const long double fr = L::get(full[p].re, h), fi = L::get(full[p].im, h);
                norm2 += fr * fr + fi * fi;
                dmax = fmaxl(dmax, fabsl((long double)L::get(a[p].re, h) - fr));
                dmax = fmaxl(dmax, fabsl((long double)L::get(a[p].im, h) - fi));
            }
            const long double ulps = norm2 > 0 ? dmax / (eps_of<S>() * sqrtl(norm2)) : (dmax > 0 ? INFINITY : 0);
            worst_zero = fmaxl(worst_zero, ulps);
        }
    }
    report("plain", L::name, R, NZ, sqrtl(e_new / n2), sqrtl(e_dif / n2b));
    const bool zok = worst_zero <= 2.0L;
    std::printf("zeros   %-6s R=%-2d NZ=%-2d  max |pruned - full| = %.3Lf ulp of the output norm%s\n", L::name, R, NZ,
                worst_zero, zok ? "" : "  FAIL");
    if (!zok) ++g_fail;
}

// ---- the twiddled entry: twiddles w^(r m), w = exp(2 pi i / (NS R)), as the passes use them
// a table of the rounded exact twiddles (the pass-1 table of the kernels)
template <typename P, int R> struct TableTw {
    using scalar = P;
    C2<P> w[R];
    C2<P> lo(int r) const { return w[r]; }
    C2<P> hi(int r) const { return w[r + R / 2]; }
};

// P: the twiddle's type (T: per-lane twiddles; Sc<T>: one twiddle shared by both lanes)
template <typename T, typename P, int R, bool POWERS> void check_tw(const char* kind) {
    using S = Sc<T>;
    using L = Lanes<T>;
    using LP = Lanes<P>;
    constexpr int LR = ilog2<R>();
    constexpr int NS = 512;                      // twiddle denominators NS * R, as a late pass
    Rng rng{0xabcdu + 17u * R + 3u * sizeof(S) + L::n + 5u * LP::n + (POWERS ? 1000u : 0u)};
    long double e_new = 0, e_dif = 0, n2 = 0, n2b = 0;
    for (int trial = 0; trial < g_trials; ++trial) {
        int m[2];
        for (int h = 0; h < LP::n; ++h) m[h] = (int)(rng.next() % NS);
        if (LP::n == 1) m[1] = m[0];
        C2<P> bases[LR > 0 ? LR : 1];
        TableTw<P, R> tab;
        for (int h = 0; h < LP::n; ++h) {
            for (int k = 0; k < LR; ++k) {
                const LC e = lexp((long double)(((long)m[h] << k) % (NS * R)) / (NS * R));
                LP::set(bases[k].re, h, (Sc<P>)e.re);
                LP::set(bases[k].im, h, (Sc<P>)e.im);
            }
            for (int r = 0; r < R; ++r) {
                const LC e = lexp((long double)(((long)m[h] * r) % (NS * R)) / (NS * R));
                LP::set(tab.w[r].re, h, (Sc<P>)e.re);
                LP::set(tab.w[r].im, h, (Sc<P>)e.im);
            }
        }
        C2<T> a[R], b[R];
        LC x[2][R];
        for (int r = 0; r < R; ++r) {
            for (int h = 0; h < L::n; ++h) {
                const S re = (S)rng.uni(), im = (S)rng.uni();
                L::set(a[r].re, h, re);
                L::set(a[r].im, h, im);
                const LC e = lexp((long double)(((long)m[h] * r) % (NS * R)) / (NS * R));
                x[h][r] = lmul(LC{(long double)re, (long double)im}, e);
            }
            b[r] = a[r];
        }
        std::vector<LC> ref[2];
        for (int h = 0; h < L::n; ++h) ref[h] = direct_dft<R>(x[h]);
        if constexpr (POWERS) {
            idft_br_tw<T, R>(a, TwPowers<P, R>(bases));
            idft_br_tw_dif<T, R>(b, TwPowers<P, R>(bases));
        } else {
            idft_br_tw<T, R>(a, tab);
            idft_br_tw_dif<T, R>(b, tab);
        }
        accumulate<T, R>(a, ref, e_new, n2);
        accumulate<T, R>(b, ref, e_dif, n2b);
    }
    report(kind, L::name, R, 0, sqrtl(e_new / n2), sqrtl(e_dif / n2b));
}

template <typename T, int R, int NZ> void plain_if() {
    if constexpr (NZ <= R) check_plain<T, R, NZ>();
}
template <typename T, int R> void all_of_radix() {
    // the pass-0 variants of the fused kernels (4 .. 24, R) and of the chirp-z kernel (1, 2, 4, R/2)
    plain_if<T, R, 1>();
    plain_if<T, R, 2>();
    if constexpr (R > 4) plain_if<T, R, 4>();
    if constexpr (R > 8) plain_if<T, R, 8>();
    plain_if<T, R, 12>();
    if constexpr (R > 16) plain_if<T, R, 16>();
    plain_if<T, R, 20>();
    plain_if<T, R, 24>();
    check_plain<T, R, R>();
    check_tw<T, T, R, true>("tw-pow");
    check_tw<T, T, R, false>("tw-tab");
    if constexpr (Lanes<T>::n == 2) {            // signal pairs: one scalar twiddle for both lanes
        check_tw<T, Sc<T>, R, true>("tw-pow1");
        check_tw<T, Sc<T>, R, false>("tw-tab1");
    }
}
template <typename T> void all_of_type() {
    all_of_radix<T, 2>();
    all_of_radix<T, 4>();
    all_of_radix<T, 8>();
    all_of_radix<T, 16>();
    all_of_radix<T, 32>();
}

}  // namespace

int main(int argc, char** argv) {
    static_assert(!kDftDif, "the check compares the product form with the DIF form: build without NW_DFT_DIF");
    if (argc > 1) g_trials = std::atoi(argv[1]);
    if (g_trials < 1) return 2;
    all_of_type<float>();
    all_of_type<double>();
#if NW_HAVE_F2
    all_of_type<f2>();
#else
    std::printf("f2: this compiler has no ext_vector_type, packed pairs not checked\n");
#endif
    std::printf(g_fail ? "FAILED: %d checks\n" : "ok (%d failures)\n", g_fail);
    return g_fail ? 1 : 0;
}
