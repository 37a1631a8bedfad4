// CPU driver for the sanitizer build of the engine's host-only logic (nw_host.cpp):
// built with -fsanitize=address,undefined by tests/test_host_asan.py.
//   host_asan self      : invariant checks of group_rows / block_of / parallel_copy / advise_output /
//                         normal_rows / row_view_layout / stock_params, and of the kernels' launch
//                         geometry (nw_shape.h): grid <-> block mapping, size table, limits, the
//                         two-pass splits and grids, the chirp-z lengths and M classes
//   host_asan large     : the two-pass rules (split, row E, pass-0 ladder, rows per block, need,
//                         LDS-DMA rule) per dtype, n and row kind, one line each
//   host_asan chirp     : the chirp-z rules (lengths, a row's M class around every class boundary,
//                         E per dtype, M and output, partial sums per class), one line each
//   host_asan grid      : stdin "real_length sfreq interpolate" -> "len_valid len_full delta"
//   host_asan shapes    : the size table's rules (E, pass-0 ladders, support rounding, partial
//                         sums, decimated lengths), one line each
#include <algorithm>
#include <cmath>
#include <iterator>
#include <cstdio>
#include <functional>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/ninwave.h"
#include "../../ninwavelets_amd/csrc/nw_host.h"
#include "../../ninwavelets_amd/csrc/nw_shape.h"

using namespace nw::host;

static int g_fail = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                       \
        }                                                                   \
    } while (0)

// brute-force equality of rows f and g under group_rows' rules
static bool rows_equal(const std::vector<double>& tab, int64_t L, const std::vector<int64_t>* rl, int f, int g) {
    const int64_t lf = rl ? (*rl)[f] : L, lg = rl ? (*rl)[g] : L;
    return lf == lg && std::memcmp(&tab[(size_t)f * L * 2], &tab[(size_t)g * L * 2], (size_t)lf * 16) == 0;
}

static void check_groups(const RowGroups& g, int F, const std::function<bool(int, int)>& eq) {
    CHECK((int)g.rep.size() == F);
    const int U = (int)g.uniq.size();
    CHECK((int)g.packed.size() == U + 1 + F);
    for (int f = 0; f < F; ++f) {
        int first = f;
        for (int h = 0; h < f; ++h)
            if (eq(h, f)) { first = h; break; }
        CHECK(g.rep[f] == first);
    }
    std::vector<int> seen(F, 0);
    CHECK(g.packed[0] == 0 && g.packed[U] == F);
    for (int u = 0; u < U; ++u)
        for (int i = g.packed[u]; i < g.packed[u + 1]; ++i) {
            const int f = g.packed[U + 1 + i];
            CHECK(f >= 0 && f < F);
            if (f < 0 || f >= F) continue;
            seen[f]++;
            CHECK(g.rep[f] == g.uniq[u]);
        }
    for (int f = 0; f < F; ++f) CHECK(seen[f] == 1);
}

static void self_checks() {
    std::mt19937_64 rng(7);
    // group_rows: user tables with repeats and ragged rows
    for (int trial = 0; trial < 200; ++trial) {
        const int F = (int)(rng() % 40);
        const int64_t L = 1 + (int64_t)(rng() % 33);
        std::vector<double> tab((size_t)F * L * 2 + 1);
        std::vector<int64_t> rl(F);
        const int distinct = 1 + (int)(rng() % 5);
        for (int f = 0; f < F; ++f) {
            const int pick = (int)(rng() % distinct);
            rl[f] = 1 + (pick * 7) % L;
            for (int64_t i = 0; i < L * 2; ++i) tab[(size_t)f * L * 2 + i] = (i < rl[f] * 2) ? pick * 1.5 + i : 0.0;
        }
        const bool ragged = trial & 1;
        RowGroups g = group_rows(false, F, nullptr, tab.data(), L, ragged ? rl.data() : nullptr);
        check_groups(g, F, [&](int a, int b) { return rows_equal(tab, L, ragged ? &rl : nullptr, a, b); });
        // freq-keyed rows (analytic kinds) with repeated values, and Shannon
        std::vector<double> fr(F);
        for (int f = 0; f < F; ++f) fr[f] = 0.5 * (double)(rng() % 6);
        RowGroups h = group_rows(false, F, fr.data(), nullptr, L, nullptr);
        check_groups(h, F, [&](int a, int b) { return std::memcmp(&fr[a], &fr[b], 8) == 0; });
        if (F > 0) {
            RowGroups s = group_rows(true, F, fr.data(), nullptr, L, nullptr);
            check_groups(s, F, [](int, int) { return true; });
            CHECK(s.uniq.size() == 1);
        }
    }
    // -0.0 and 0.0 are different bits: different rows (the engine keys on bits)
    {
        const double fr[2] = {0.0, -0.0};
        CHECK(group_rows(false, 2, fr, nullptr, 4, nullptr).uniq.size() == 2);
    }
    // block_of: a partition into balanced contiguous blocks
    for (int64_t nsig = 0; nsig < 200; ++nsig)
        for (int n = 1; n < 12; ++n) {
            int64_t next = 0;
            for (int i = 0; i < n; ++i) {
                int64_t s0, cnt;
                block_of(nsig, i, n, &s0, &cnt);
                CHECK(s0 == next && cnt >= nsig / n && cnt <= nsig / n + 1);
                next = s0 + cnt;
            }
            CHECK(next == nsig);
        }
    // parallel_copy at odd sizes and thread counts
    const size_t sizes[] = {0, 1, 7, (size_t(4) << 20) - 1, (size_t(4) << 20) + 3, (size_t(33) << 20) + 5};
    for (size_t bytes : sizes)
        for (unsigned th : {0u, 1u, 3u, 8u, 64u}) {
            std::vector<char> src(bytes + 1), dst(bytes + 1, 0);
            for (size_t i = 0; i < bytes; ++i) src[i] = (char)(i * 131 + th);
            parallel_copy(dst.data(), src.data(), bytes, th);
            CHECK(std::memcmp(dst.data(), src.data(), bytes) == 0);
        }
    // advise_output: contents kept, whole range writable afterwards, odd bounds and sizes
    for (size_t bytes : {size_t(0), size_t(100), (size_t(2) << 20) - 1, (size_t(37) << 20) + 11,
                         (size_t(130) << 20) + 4097}) {
        std::vector<char> buf(bytes + 64);
        char* dst = buf.data() + 5;                      // not page aligned
        for (size_t i = 0; i < bytes; i += 4093) dst[i] = (char)(i * 7);
        const size_t adv = advise_output(dst, bytes);
        CHECK(adv <= bytes && adv % (size_t(2) << 20) == 0);
        CHECK(bytes >= (size_t(4) << 20) || adv <= (size_t(2) << 20));
        for (size_t i = 0; i < bytes; i += 4093) CHECK(dst[i] == (char)(i * 7));
        std::memset(dst, 1, bytes);
    }
    // normal_rows: offsets tile the batched buffer, rows of equal length consecutive
    for (int mh = 0; mh < 2; ++mh) {
        const double params[3] = {7.0, 1000.0, 1.0};
        std::vector<double> fr = {1., 2., 3., 5., 2., 40., 80., 160.};
        std::vector<nw::NormalRow> rows;
        int64_t lmax = 0, total = 0;
        double sigma = -1;
        const bool ok = normal_rows(mh == 1, params + (mh ? 0 : 1), mh ? 3 : 2, fr.data(), (int)fr.size(), rows,
                                    &lmax, &total, &sigma);
        CHECK(ok);
        int64_t sum = 0;
        for (auto& r : rows) {
            CHECK(r.len == r.m + 2 * r.half && r.half >= 0 && r.len <= lmax);
            CHECK(r.off >= 0 && r.off + r.len <= total);
            sum += r.len;
        }
        CHECK(sum == total);
        // a wavelet longer than sfreq * real_wave_length: negative padding is refused
        const double tiny[3] = {7.0, 10.0, 0.01};
        CHECK(!normal_rows(mh == 1, tiny + (mh ? 0 : 1), mh ? 3 : 2, fr.data(), (int)fr.size(), rows, &lmax, &total,
                           &sigma));
    }
    // row_view_layout: the sections ascend without overlap, aligned (16 B, table rows 256 B),
    // and end at the returned total
    for (int U = 0; U <= 40; ++U)
        for (size_t map_len : {size_t(0), size_t(1), size_t(U), size_t(2 * U + 3), size_t(1000)})
            for (size_t trow : {size_t(0), size_t(16), size_t(40), size_t(4096)}) {
                const RowViewLayout l = row_view_layout(U, map_len, trow);
                const size_t u = (size_t)U;
                const size_t start[] = {l.idx, l.offs, l.order, l.freq, l.peak, l.xstep, l.row_len, l.table};
                const size_t size[] = {u * 4, (u + 1) * 4, map_len * 4, u * 8, u * 8, u * 4, u * 8, u * trow};
                CHECK(l.idx == 0);
                for (int s = 0; s < 8; ++s) {
                    CHECK(start[s] % (s == 7 ? 256 : 16) == 0);
                    const size_t next = s < 7 ? start[s + 1] : l.bytes;
                    CHECK(start[s] + size[s] <= next);
                }
                CHECK(l.table + u * trow == l.bytes);
            }
    // stock_params against the formulas written out (wavelets.py:65-74, 118-136)
    {
        const StockParams m0 = stock_params(NW_MORSE, nullptr, 0);
        CHECK(m0.b == 17.5 && m0.r == 3.0 && m0.b_over_r == 17.5 / 3.0);
        CHECK(m0.sigma == 0.0 && m0.cpi == 0.0 && m0.kappa == 0.0);
        const double mp[2] = {4.0, 0.7};
        const StockParams m1 = stock_params(NW_MORSE, mp, 2);
        CHECK(m1.b == 4.0 && m1.r == 0.7 && m1.b_over_r == 4.0 / 0.7);
        const double quarter = std::pow(M_PI, -0.25);
        auto c_of = [](double s) { return std::pow(1.0 + std::exp(-s * s) - 2.0 * std::exp(-3.0 / 4.0 * (s * s)), -0.5); };
        const StockParams l0 = stock_params(NW_MORLET, nullptr, 0);
        CHECK(l0.sigma == 7.0 && l0.cpi == c_of(7.0) * quarter && l0.kappa == std::exp(-std::pow(7.0, 2.0) / 2.0));
        CHECK(l0.b == 0.0 && l0.r == 0.0 && l0.b_over_r == 0.0);
        for (int gabor = 0; gabor < 2; ++gabor) {
            const double lp[4] = {5.5, (double)gabor, 1.25, 0.125};
            const StockParams l2 = stock_params(NW_MORLET, lp, 2);   // c and k from sigma
            CHECK(l2.sigma == 5.5 && l2.cpi == c_of(5.5) * quarter);
            CHECK(l2.kappa == (gabor ? 0.0 : std::exp(-std::pow(5.5, 2.0) / 2.0)));
            const StockParams l4 = stock_params(NW_MORLET, lp, 4);   // every parameter given
            CHECK(l4.sigma == 5.5 && l4.cpi == 1.25 * quarter && l4.kappa == 0.125);
        }
        const double hp[1] = {3.0};
        CHECK(stock_params(NW_MEXICAN_HAT, nullptr, 0).sigma == 7.0 && stock_params(NW_MEXICAN_HAT, hp, 1).sigma == 3.0);
        CHECK(stock_params(NW_SHANNON, nullptr, 0).sigma == 0.0 && stock_params(NW_HAAR, hp, 1).sigma == 0.0);
        CHECK(morlet_peak(7.0, 2.0) == 7.0 / (1.0 - std::exp(-7.0 * 2.0)));
    }
}

// ---- the launch geometry (nw_shape.h): what the kernels and their launchers compile

// block_slot restricted to the valid slots of grid g is a bijection onto nrows x groups_pad (so
// onto nrows x groups): every (row, group) is computed by exactly one block
static void check_grid(const nw::BlockGrid& g, int64_t groups, int nrows, int tile_f) {
    CHECK(g.ok && g.tile_g >= 1 && g.groups_pad >= groups && g.groups_pad < groups + 8 * g.tile_g);
    CHECK(g.blocks % (8 * tile_f * g.tile_g) == 0);
    std::vector<int> hit((size_t)nrows * (size_t)g.groups_pad, 0);
    for (int64_t b = 0; b < g.blocks; ++b) {
        const nw::BlockSlot sl = nw::block_slot((int)b, nrows, tile_f, g.tile_g);
        CHECK(sl.row >= 0 && sl.group >= 0 && sl.group < g.groups_pad);
        if (sl.row >= 0 && sl.row < nrows && sl.group >= 0 && sl.group < g.groups_pad)
            hit[(size_t)sl.row * (size_t)g.groups_pad + (size_t)sl.group]++;
    }
    for (int h : hit) CHECK(h == 1);
}

static void shape_checks() {
    using namespace nw;
    for (int nrows : {1, 2, 7, 8, 9, 64, 129})
        for (int64_t groups : {1, 2, 7, 8, 9, 31, 32, 33, 65}) {
            for (int tg_max : {1, 2, 4}) {
                const BlockGrid g = block_grid(groups, nrows, kTileF, tg_max);
                CHECK(g.tile_g == std::min<int64_t>(tg_max, (groups + 7) / 8) && g.tile_g == tile_g_of(groups, tg_max));
                check_grid(g, groups, nrows, kTileF);
            }
            check_grid(block_grid_tile(groups, nrows, kTileFC, kTileGC), groups, nrows, kTileFC);       // chirp-z
            check_grid(block_grid_tile(groups, nrows, kRowTileF, kRowTileG), groups, nrows, kRowTileF);  // two-pass rows
        }
    // the 2^31 refusal at the first size that needs it: 8 rows x 2^28 padded groups = 2^31 blocks
    CHECK(block_grid(0, 1, 8, 4).ok && block_grid(0, 1, 8, 4).blocks == 0);
    for (int tg_max : {1, 2, 4}) {
        const int64_t last = (int64_t(1) << 28) - 8 * tg_max;   // the last whole tile below 2^28 groups
        const BlockGrid fits = block_grid(last, 8, 8, tg_max), over = block_grid(last + 1, 8, 8, tg_max);
        CHECK(fits.ok && fits.blocks == (int64_t(1) << 31) - 64 * tg_max);
        CHECK(!over.ok && over.blocks == int64_t(1) << 31);
        CHECK(block_grid(last, 9, 8, tg_max).ok == false);     // one more row tile
        CHECK(!block_grid_tile(int64_t(1) << 31, 1, 1, 1).ok && block_grid_tile((int64_t(1) << 31) - 8, 1, 1, 1).ok);
    }
    // the size table: powers of two 2^10 .. 2^14, both compute dtypes, and nothing else
    for (int dtype : {NW_F32, NW_F64, 7})
        for (int64_t n = 1; n <= 40000; ++n) {
            const bool in = dtype != 7 && n >= 1024 && n <= 16384 && (n & (n - 1)) == 0;
            CHECK(fused_supported(n, dtype) == in && fused_e(n, dtype) == (in ? (n <= 4096 ? 16 : 32) : 0));
            const int seen = for_fused_size(n, dtype, -1, []<typename T, int N, int E>(FusedSize<T, N, E>) {
                return (int)sizeof(T) * 100000 + N / E;
            });
            CHECK(seen == (in ? (dtype == NW_F32 ? 4 : 8) * 100000 + (int)n / fused_e(n, dtype) : -1));
        }
    // group_filling halves down to 2 and never below; the W-support array follows 16-byte padded rows
    for (int base : {8, 16})
        for (int64_t nsig : {1, 7, 64, 256, 4096}) {
            const int g = group_filling(base, nsig, 128);
            CHECK(g >= 2 && g <= base && base % g == 0);
            CHECK(g == base || (nsig + g - 1) / g * 128 >= kMinRounds * kResidentBlocks || g == 2);
        }
    alignas(16) static char buf[64];
    CHECK(reinterpret_cast<const char*>(wtab_wnz(buf, 3, 1, 4, true)) == buf + 16);
    CHECK(reinterpret_cast<const char*>(wtab_wnz(buf, 3, 1, 4, false)) == buf + 32);
}

// ---- the two-pass and chirp-z rules (nw_shape.h)

// The column grid of one form (nf x N2 / C blocks, THREADS threads of E elements) covers every
// (scale, n2, n1) exactly once.  The mapping is a product of three independent ones -- block ->
// (scale, column group), thread slot -> column within the group, (thread, element) -> n1 -- so
// each factor is checked exhaustively; and the largest lane byte offsets fit 32 bits.
template <typename T, bool PAIR, int N1, int N2>
static void check_cols() {
    using CL = nw::ColShape<T, PAIR, N1>;
    CHECK(N2 % CL::C == 0 && CL::THREADS == CL::SLOTS * CL::U && CL::U * CL::E == N1 && CL::THREADS <= 1024);
    CHECK(CL::LDS == N1 * CL::SLOTS * CL::CPS * (int)sizeof(T) && CL::LDS <= 160 * 1024);
    const int ngroups = N2 / CL::C;
    for (int nf : {1, 7, 8, 9}) {
        std::vector<int> hit((size_t)nf * ngroups, 0);
        for (int b = 0; b < nf * ngroups; ++b) hit[(size_t)(b / ngroups) * ngroups + b % ngroups]++;
        for (int h : hit) CHECK(h == 1);
    }
    std::vector<int> col(CL::C, 0), n1(N1, 0);
    for (int t = 0; t < CL::THREADS; ++t) {
        const int c = t % CL::SLOTS, u = t / CL::SLOTS;
        if (u == 0)
            for (int j = 0; j < CL::CPS; ++j) col[CL::CPS * c + j]++;
        if (c == 0)
            for (int r = 0; r < CL::E; ++r) n1[u + CL::U * r]++;
    }
    for (int h : col) CHECK(h == 1);
    for (int h : n1) CHECK(h == 1);
    // B: ((k1 * N2 + col) complex values; out: (col + n1 * N2) values of at most a complex
    const uint64_t last = (uint64_t)(N1 - 1) * N2 + (N2 - 1);
    CHECK(last * 2 * sizeof(T) + 2 * sizeof(T) * CL::CPS <= (uint64_t(1) << 32));
}

static void large_checks() {
    using namespace nw;
    for (int dtype : {NW_F32, NW_F64}) {
        for (int lg = 15; lg <= 24; ++lg) {
            const int64_t n = int64_t(1) << lg;
            const Split sp = large_split(n);
            CHECK(large_supported(n, dtype));
            CHECK((int64_t)sp.n1 * sp.n2 == n && sp.n1 >= 32 && sp.n1 <= 1024 && sp.n2 <= 16384);
            const int64_t seen = for_large_split(n, dtype, int64_t(-1), []<typename T, int N1, int N2>(LargeSplit<T, N1, N2>) {
                check_cols<T, false, N1, N2>();
                if constexpr (sizeof(T) == 4) check_cols<T, true, N1, N2>();
                // the row grid: block_slot onto scales x row groups, each group rgs whole rows
                for (int nf : {1, 7, 8, 9}) {
                    const int rgs = row_group_of(nf);
                    CHECK(rgs == (nf < 8 ? 1 : 4) && N1 % rgs == 0);
                    check_grid(block_grid_tile(N1 / rgs, nf, kRowTileF, kRowTileG), N1 / rgs, nf, kRowTileF);
                }
                return ((int64_t)sizeof(T) << 40) | ((int64_t)N1 << 20) | N2;
            });
            CHECK(seen == (((int64_t)(dtype == NW_F32 ? 4 : 8) << 40) | ((int64_t)sp.n1 << 20) | sp.n2));
        }
        for (int64_t n : {int64_t(1) << 14, int64_t(1) << 25, int64_t(3) << 15, (int64_t(1) << 20) + 1}) {
            CHECK(!large_supported(n, dtype));
            CHECK(for_large_split(n, dtype, -1, []<typename T, int N1, int N2>(LargeSplit<T, N1, N2>) { return 0; }) == -1);
        }
    }
    CHECK(!large_supported(1 << 20, 7) && for_large_split(1 << 20, 7, -1, [](auto) { return 0; }) == -1);
    // the support buffer's sections ascend, 256-B aligned
    for (int nfreq : {1, 63, 64, 65, 512}) {
        CHECK(wmax_offset(nfreq) >= (size_t)nfreq * 4 && wmax_offset(nfreq) % 256 == 0);
        CHECK(tsplit_offset(nfreq) >= wmax_offset(nfreq) + (size_t)nfreq * 8 && tsplit_offset(nfreq) % 256 == 0);
        CHECK(large_support_bytes(nfreq) == tsplit_offset(nfreq) + (size_t)kSplitEntries * 16);
    }
    CHECK(fchunk_of(1 << 24, 512, NW_F32) == 64 && fchunk_of(1 << 24, 512, NW_F64) == 32 && fchunk_of(1 << 15, 3, NW_F32) == 3);
    CHECK(fchunk_clamp(0, 5) == 1 && fchunk_clamp(-3, 5) == 1 && fchunk_clamp(9, 5) == 5 && fchunk_clamp(2, 5) == 2);
}

static void chirp_checks() {
    using namespace nw;
    for (int dtype : {NW_F32, NW_F64}) {
        const int64_t mmax = chirp_mmax(dtype);
        for (int64_t n = 1; n <= 16383; ++n) {
            std::vector<int64_t> ks = {0, 1, n};
            for (int64_t m = 1024; m <= 16384; m *= 2)
                for (int64_t d = -1; d <= 1; ++d) {
                    ks.push_back(m / 2 + d);         // M >= 2K
                    ks.push_back(m - n + 1 + d);     // M >= n + K - 1
                }
            const int64_t top = std::min(chirp_m(n), mmax);
            for (int64_t k : ks) {
                if (k < 0 || k > n) continue;
                const int64_t need = std::max(n + std::max<int64_t>(k, 1) - 1, 2 * k);
                int want = -1;
                for (int c = kChirpClasses - 1; c >= 0; --c)
                    if ((int64_t(1024) << c) >= need && (int64_t(1024) << c) <= top) want = c;
                CHECK(chirp_class(n, k, dtype) == want);
            }
        }
        for (int64_t m = 512; m <= 32768; m *= 2) {
            const int e = chirp_e(m, dtype);
            CHECK(e == (m >= 1024 && m <= mmax ? (m == 16384 ? 32 : 16) : 0));
            const int seen = for_chirp_size(m, dtype, -1, []<typename T, int M, int E>(ChirpSize<T, M, E>) {
                return (int)sizeof(T) * 100000 + M / E;
            });
            CHECK(seen == (e ? (dtype == NW_F32 ? 4 : 8) * 100000 + (int)m / e : -1));
        }
        CHECK(for_chirp_size(3000, dtype, -1, [](auto) { return 0; }) == -1);
    }
    CHECK((kChirpAbsE<float, 8192, 16>) == 32 && (kChirpAbsE<float, 4096, 16>) == 16 && (kChirpAbsE<double, 8192, 16>) == 16);
    // the lengths tests/test_gpu_chirp.py runs, against the definitions
    const int64_t f32n[] = {1, 2, 3, 5, 21, 300, 301, 512, 1000, 1021, 1201, 2049, 3001, 4097, 8191, 10001, 14001, 701};
    const int64_t f64n[] = {1, 3, 21, 300, 301, 1000, 1201, 2049, 4095, 5001, 4097, 701};
    for (int dtype : {NW_F32, NW_F64}) {
        std::vector<int64_t> ns = dtype == NW_F32 ? std::vector<int64_t>(std::begin(f32n), std::end(f32n))
                                                  : std::vector<int64_t>(std::begin(f64n), std::end(f64n));
        for (int64_t n : {1024, 4096, 16384, 8192, 16383, 8193, 0, -5}) ns.push_back(n);
        for (int64_t n : ns) {
            const bool pow2 = n >= 1024 && n <= 16384 && (n & (n - 1)) == 0;
            CHECK(chirp_supported(n, dtype) == (n >= 1 && !pow2 && 2 * n - 1 <= chirp_mmax(dtype)));
            CHECK(chirp_possible(n, dtype) == (n >= 1 && !pow2 && n < chirp_mmax(dtype)));
        }
    }
    CHECK(!chirp_supported(1201, 7) && !chirp_possible(1201, 7));
    const int64_t one_big[kChirpClasses] = {0, 0, 0, 0, 1}, small[kChirpClasses] = {3, 1, 0, 0, 0}, mid[kChirpClasses] = {0, 0, 1, 1, 0};
    CHECK(!chirp_psum_ok(NW_F32, false, one_big) && chirp_psum_ok(NW_F32, true, mid) && chirp_psum_ok(NW_F64, false, mid));
    CHECK(!chirp_psum_ok(NW_F64, true, mid) && chirp_psum_ok(NW_F64, true, small));
    // chirp_psum_chunk: the chunks tile the call, none longer than max_batch, and each is whole
    // signal groups from a group's start (only the call's last group ragged) or lies inside one group
    for (int64_t nsig = 0; nsig <= 70; ++nsig)
        for (int64_t mb = 1; mb <= 40; ++mb) {
            int64_t s0 = 0;
            while (s0 < nsig) {
                const int64_t c = chirp_psum_chunk(s0, nsig, mb);
                CHECK(c >= 1 && c <= mb && s0 + c <= nsig);
                if (c < 1) break;
                const bool whole = s0 % kPsumGroup == 0 && (c % kPsumGroup == 0 || s0 + c == nsig);
                const bool inside = s0 / kPsumGroup == (s0 + c - 1) / kPsumGroup;
                CHECK(whole || inside);
                CHECK(mb < kPsumGroup || whole);
                s0 += c;
            }
            CHECK(s0 == nsig);
        }
}

static const char* out_name(int out) { return out == NW_OUT_CWT ? "cwt" : out == NW_OUT_POWER ? "power" : "abs"; }

template <typename T, int N, int E, int OUT>
static void print_ladder() {
    const char* dt = sizeof(T) == 4 ? "float32" : "float64";
    std::printf("variants %s %d %s single", dt, N, out_name(OUT));
    for (int nz = 1, prev = 0; nz <= E; ++nz) {
        const int v = nw::pass0_variant<E, nw::kNzFineOut<T, N, E, OUT>, nw::kNz24Of<T, N, E>>(nz);
        if (v != prev) std::printf(" %d", v);
        prev = v;
    }
    std::printf("\n");
    if constexpr (nw::kPairMode<T, E, true>) {
        std::printf("variants %s %d %s pair", dt, N, out_name(OUT));
        for (int nz = 1, prev = 0; nz <= E; ++nz) {
            const int v = nw::pair_pass0_variant(nz, E);
            if (v != prev) std::printf(" %d", v);
            prev = v;
        }
        std::printf("\n");
    }
}

// every rule of the table, one line each, for tests/test_host_asan.py to compare with the
// tests' Python restatement (tests/fused_variants.py)
static void print_shapes() {
    using namespace nw;
    for (int dtype : {NW_F32, NW_F64})
        for (int64_t n = 512; n <= 32768; n *= 2)
            for_fused_size(n, dtype, 0, []<typename T, int N, int E>(FusedSize<T, N, E>) {
                const char* dt = sizeof(T) == 4 ? "float32" : "float64";
                std::printf("size %s %d E %d pair %d\n", dt, N, E, (int)kPairMode<T, E, true>);
                print_ladder<T, N, E, NW_OUT_CWT>();
                print_ladder<T, N, E, NW_OUT_ABS>();
                print_ladder<T, N, E, NW_OUT_POWER>();
                std::printf("wnz %s %d", dt, N);
                for (int need = 1; need <= E; ++need) std::printf(" %d", wnz_round(need, E));
                std::printf("\n");
                constexpr int PE = kPsE<T, E, false>, HE = kPsE<T, E, true>;
                std::printf("psum %s %d power E %d shift %d ok %d\n", dt, N, PE, kPsShift<E, PE>, (int)kPSumOK<T, N, E>);
                std::printf("psum %s %d phase E %d shift %d ok %d\n", dt, N, HE, kPsShift<E, HE>, (int)kPhSumOK<T, N, E>);
                return 1;
            });
    const int64_t extra[] = {1000, 3000, 4097, 6144, 12288, 16383, 16385};
    for (int dtype : {NW_F32, NW_F64}) {
        std::vector<int64_t> sizes;
        for (int64_t n = 512; n <= 32768; n *= 2) sizes.push_back(n);
        sizes.insert(sizes.end(), std::begin(extra), std::end(extra));
        for (int64_t n : sizes)
            for (int decim = -2; decim <= 32; ++decim)
                if (decim_supported(n, dtype, decim))
                    std::printf("decim %s %lld %d\n", dtype == NW_F32 ? "float32" : "float64", (long long)n, decim);
    }
}

// the two-pass rules of one (dtype, n, analytic or table rows), one line each, for
// tests/test_host_asan.py to compare with tests/large_variants.py
static const int kNeedCases[][2] = {{-1, 0}, {0, 0}, {0, 5}, {31, 31}, {32, 0}, {1000, 3}, {65535, 1}, {65536, 0},
                                    {1 << 20, 31}, {(1 << 24) - 1, 0}, {(1 << 24) - 1, 1023}};   // (km, k1)
template <typename T, int N1, int N2, bool TABLE>
static void print_large_rows() {
    constexpr int E = TABLE ? nw::kRowETab<T, N2> : nw::kRowE<T, N2>;
    const char* dt = sizeof(T) == 4 ? "float32" : "float64";
    const char* kd = TABLE ? "table" : "analytic";
    const long long n = (long long)N1 * N2;
    std::printf("split %s %lld %s %d %d\n", dt, n, kd, N1, N2);
    std::printf("rowe %s %lld %s %d\n", dt, n, kd, E);
    std::vector<int> lad;
    for (int nz = 1; nz <= E; ++nz) {
        const int v = nw::pass0_variant<E, nw::kRowFine<T, E, TABLE>, (E > 16)>(nz);
        if (lad.empty() || lad.back() != v) lad.push_back(v);
    }
    std::printf("ladder %s %lld %s", dt, n, kd);
    for (int v : lad) std::printf(" %d", v);
    std::printf("\nrowgroup %s %lld %s", dt, n, kd);
    for (int nf = 1; nf <= 16; ++nf) std::printf(" %d", nw::row_group_of(nf));
    std::printf("\nneed %s %lld %s", dt, n, kd);
    for (const auto& c : kNeedCases)
        if (c[0] < n && c[1] < N1) std::printf(" %d", nw::row_need(c[0], c[1], N1, N2 / E));
    std::printf("\nxd %s %lld %s", dt, n, kd);
    for (int v : lad) std::printf(" %d", (int)(nw::kRowXD<T, E, TABLE> && v <= nw::kRowLdsNz<E>));
    std::printf("\n");
}
static void print_large() {
    for (int dtype : {NW_F32, NW_F64})
        for (int lg = nw::kLargeLog2Min; lg <= nw::kLargeLog2Max; ++lg)
            nw::for_large_split(int64_t(1) << lg, dtype, 0, []<typename T, int N1, int N2>(nw::LargeSplit<T, N1, N2>) {
                print_large_rows<T, N1, N2, false>();
                print_large_rows<T, N1, N2, true>();
                return 1;
            });
}

// the chirp-z rules, one line each, for tests/test_host_asan.py to compare with
// tests/chirp_variants.py
static const int64_t kChirpLengths[] = {1, 300, 511, 513, 712, 1201, 2047, 2049, 4095, 4096, 4097, 8191, 8193, 14001, 16383};
static void print_chirp() {
    using namespace nw;
    for (int dtype : {NW_F32, NW_F64}) {
        const char* dt = dtype == NW_F32 ? "float32" : "float64";
        for (int64_t n : kChirpLengths) {
            std::printf("len %s %lld supported %d possible %d m %lld\n", dt, (long long)n, (int)chirp_supported(n, dtype),
                        (int)chirp_possible(n, dtype), (long long)chirp_m(n));
            // K = 0, 1, 2, 3, n / 2, n - 1, n and the K either side of every class boundary
            // (2K <= M and n + K - 1 <= M), ascending
            std::vector<int64_t> ks = {0, 1, 2, 3, n / 2, n - 1, n};
            for (int c = 0; c < kChirpClasses; ++c) {
                const int64_t m = int64_t(1024) << c;
                for (int64_t k : {m / 2, m / 2 + 1, m - n + 1, m - n + 2}) ks.push_back(k);
            }
            std::sort(ks.begin(), ks.end());
            ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
            std::printf("class %s %lld", dt, (long long)n);
            for (int64_t k : ks) {
                if (k < 0 || k > n) continue;
                const int c = chirp_class(n, k, dtype);
                std::printf(" %lld:%lld", (long long)k, c < 0 ? -1LL : (long long)(int64_t(1024) << c));
            }
            std::printf("\n");
        }
        for (int c = 0; c < kChirpClasses; ++c) {
            const int64_t m = int64_t(1024) << c;
            const int abs_e = for_chirp_size(m, dtype, 0, []<typename T, int M, int E>(ChirpSize<T, M, E>) {
                return (int)kChirpAbsE<T, M, E>;
            });
            std::printf("e %s %lld %d abs %d\n", dt, (long long)m, chirp_e(m, dtype), abs_e);
        }
        for (int phase = 0; phase < 2; ++phase)
            for (int c = 0; c < kChirpClasses; ++c) {
                int64_t counts[kChirpClasses] = {0, 0, 0, 0, 0};
                counts[c] = 1;
                std::printf("psum %s %s %lld %d\n", dt, phase ? "phase" : "power", (long long)(int64_t(1024) << c),
                            (int)chirp_psum_ok(dtype, phase != 0, counts));
            }
    }
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "self";
    if (mode == "large") {
        print_large();
        return 0;
    }
    if (mode == "chirp") {
        print_chirp();
        return 0;
    }
    if (mode == "shapes") {
        print_shapes();
        return 0;
    }
    if (mode == "grid") {
        double rl, sf;
        int interp;
        while (std::scanf("%lf %lf %d", &rl, &sf, &interp) == 3) {
            double d;
            int64_t lv, lf;
            trans_grid(rl, sf, interp != 0, &d, &lv, &lf);
            std::printf("%lld %lld %.17g\n", (long long)lv, (long long)lf, d);
        }
        return 0;
    }
    self_checks();
    shape_checks();
    large_checks();
    chirp_checks();
    std::printf("%s\n", g_fail ? "FAIL" : "ok");
    return g_fail ? 1 : 0;
}
