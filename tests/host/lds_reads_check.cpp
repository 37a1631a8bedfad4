// lds_reads_check.cpp — the (base, offset) pairs of the 8-byte LDS reads that the fp32 n = 16384
// kernels issue from inline asm (NW_LDS_ASM_READS; ninwavelets_amd/csrc/nw_shape.h, namespace
// lane_image: rd12_*, tab1_*), checked exhaustively on a CPU against the C++ indexing they replace
// (nw_fft_dev.h lds_read / TwTable), restated here: every thread, component and batch.  Built with
// -fsanitize=address,undefined and run by tests/test_lds_reads_cpu.py.  Prints the figures it
// checked, then "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ninwavelets_amd/csrc/nw_shape.h"

namespace L = nw::lane_image;

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (g_fail++ < 20) {                          \
                std::printf("FAIL %s: ", #cond);          \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

constexpr int N = 16384, E = 32, T = N / E;

static int g_max_off = 0, g_reads = 0;
// one ds_read_b64 field check: the offset is an unsigned 16-bit field, addresses are 8-byte aligned
static void field(int base, int off, const char* what) {
    CHECK(off >= 0 && off < 65536 && off % 8 == 0, "%s offset %d", what, off);
    CHECK(base >= 0 && base % 8 == 0, "%s base %d", what, base);
    if (off > g_max_off) g_max_off = off;
    ++g_reads;
}
// lanes [32 g, 32 g + 32) of one ds_read_b64 cover the 64 banks once (addr: lane -> byte address)
template <typename F> static bool banks_once(F addr, int g) {
    unsigned long long banks = 0;
    int hits = 0;
    for (int l = 0; l < 32; ++l)
        for (int q = 0; q < 2; ++q) {
            const int b = (addr(32 * g + l) / 4 + q) % 64;
            hits += (int)((banks >> b) & 1);
            banks |= 1ull << b;
        }
    return hits == 0 && banks == ~0ull;
}

int main() {
    static_assert(L::kN == N && L::kE == E && L::kT == T, "geometry");
    int max_end_img = 0, max_end_tab = 0;

    // ---- site 1: the 1 -> 2 image's pairs.  lds_read (P = 2): src = lds + rbase_12(2 t), element r
    // of the pair is the 8 bytes at src + roff_12(r) (floats): butterflies 2 t and 2 t + 1
    for (int comp = 0; comp < 2; ++comp)           // re and im travel through the same image
        for (int t = 0; t < T; ++t)
            for (int r = 0; r < 16; ++r) {
                const int byte = L::rd12_base(t) + L::rd12_off(r);
                field(L::rd12_base(t), L::rd12_off(r), "image");
                CHECK(byte == 4 * (L::rbase_12(2 * t) + L::roff_12(r)), "image t %d r %d: %d", t, r, byte);
                for (int q = 0; q < 2; ++q)        // ... which hold slots j2 + 1024 r of j2 = 2 t + q
                    CHECK(byte + 4 * q == 4 * L::addr12(2 * t + q + 1024 * r), "image slot t %d q %d r %d", t, q, r);
                CHECK(byte + 8 <= L::kBytes, "image end t %d r %d: %d", t, r, byte + 8);
                if (byte + 8 > max_end_img) max_end_img = byte + 8;
            }
    for (int r = 0; r < 16; ++r) {
        CHECK(L::rd12_off(r) == L::rd12_off(0) + r * L::rd12_off(1), "image offsets evenly spaced, r %d", r);
        for (int g = 0; g < T / 32; ++g)
            CHECK(banks_once([&](int t) { return L::rd12_base(t) + L::rd12_off(r); }, g), "image r %d group %d conflicts", r, g);
    }

    // ---- site 2: the pass-1 table behind the image.  TwTable: power r of butterfly t is
    // tab[(r - 1) * NS + t % NS], NS = 32, 8-byte entries, tab at byte kBytes; read in batches b of
    // the pairs (r, r + 16), r = 4 b .. 4 b + 3, without r = 0
    {
        int max_batch = 0;
        for (int t = 0; t < T; ++t) {
            std::vector<int> seen(E, 0);
            for (int b = 0; b < (E / 2) / L::kTabBatch; ++b) {
                int n = 0;
                for (int i = 0; i < L::kTabBatch; ++i)
                    for (int h = 0; h < 2; ++h) {
                        const int r = L::kTabBatch * b + i + h * (E / 2);
                        if (r == 0) continue;       // w^0 = 1 is not stored
                        const int byte = L::tab1_base(t) + L::tab1_off(r);
                        field(L::tab1_base(t), L::tab1_off(r), "table");
                        CHECK(byte == L::kBytes + 8 * ((r - 1) * E + t % E), "table t %d r %d: %d", t, r, byte);
                        CHECK(byte >= L::kBytes && byte + 8 <= L::kBytes + L::kTab1Bytes, "table end t %d r %d", t, r);
                        if (byte + 8 > max_end_tab) max_end_tab = byte + 8;
                        ++seen[r];
                        ++n;
                    }
                CHECK(n <= 8, "batch %d holds %d entries", b, n);
                if (n > max_batch) max_batch = n;
            }
            for (int r = 1; r < E; ++r) CHECK(seen[r] == 1, "table t %d power %d read %d times", t, r, seen[r]);
        }
        for (int r = 1; r < E; ++r)
            for (int g = 0; g < T / 32; ++g)
                CHECK(banks_once([&](int t) { return L::tab1_base(t) + L::tab1_off(r); }, g), "table r %d group %d conflicts", r, g);
        CHECK(max_batch == 8, "batches of %d", max_batch);
    }

    std::printf("reads %d max_offset %d image_end %d table_end %d image_bytes %d table_bytes %d\n", g_reads, g_max_off, max_end_img,
                max_end_tab, L::kBytes, L::kTab1Bytes);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
