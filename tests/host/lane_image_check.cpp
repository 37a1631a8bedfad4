// lane_image_check.cpp — the lane-addressed exchange images of the fp32 n = 16384 kernels
// (ninwavelets_amd/csrc/nw_shape.h, namespace lane_image) checked exhaustively on a CPU: every
// thread, slot and component of both images, against the slot formulas of the padded images
// (nw_fft_dev.h lds_write / lds_read), restated here.  Built with -fsanitize=address,undefined
// and run by tests/test_lane_image_cpu.py.  Prints the figures it checked, then "ok".
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

constexpr int N = 16384, E = 32, T = N / E, WAVES = T / 64;

// the padded images' slot semantics (which value a slot holds)
static int slot01_written(int t, int p) { return 32 * t + p; }             // thread t's pass-0 output p
static int slot01_read(int u, int r) { return u + 512 * r; }               // pass-1 butterfly u, element r
static int slot12_written(int j, int ip) { return (j / 32) * 1024 + j % 32 + 32 * ip; }   // butterfly j's output i'
static int slot12_read(int j2, int r) { return j2 + 1024 * r; }            // pass-2 butterfly j2, element r

int main() {
    static_assert(nw::kLaneImageShape<float, N, E> == (NW_LANE_IMAGE != 0), "the trait's one shape");
    static_assert(!nw::kLaneImageShape<double, N, E> && !nw::kLaneImageShape<float, 8192, 32> &&
                  !nw::kLaneImageShape<float, N, 16>, "fp64 and the other sizes keep the padded images");
    static_assert(L::kN == N && L::kE == E && L::kT == T, "geometry");
    int max_off = 0, max_m0 = 0, max_end = 0;
    for (int comp = 0; comp < 2; ++comp) {   // re and im travel through the same image, one after the other
        // ---- exchange 0 -> 1
        {
            std::vector<int> slot_at(L::kElems, -1);        // dword -> slot, from the writer
            for (int t = 0; t < T; ++t)
                for (int p = 0; p < E; ++p) {
                    const int i = slot01_written(t, p), wave = t / 64, lane = t % 64;
                    const int m0 = L::m0_01(wave), off = L::off_01(p);
                    const int byte = m0 + off + 4 * lane;   // 2: base + 4 * lane, base wave-uniform
                    CHECK(byte == 4 * L::addr01(i), "0->1 writer t %d p %d: %d vs %d", t, p, byte, 4 * L::addr01(i));
                    CHECK(off >= 0 && off < 65536 && m0 >= 0 && m0 < 65536, "0->1 fields t %d p %d", t, p);
                    CHECK(byte + 4 <= L::kBytes, "0->1 writer inside the image t %d p %d", t, p);
                    if (off > max_off) max_off = off;
                    if (m0 > max_m0) max_m0 = m0;
                    if (m0 + off + 252 > max_end) max_end = m0 + off + 252;
                    const int a = byte / 4;
                    CHECK(a >= 0 && a < L::kElems && slot_at[a] == -1, "0->1 writer collides t %d p %d", t, p);
                    if (a >= 0 && a < L::kElems) slot_at[a] = i;
                }
            std::vector<char> read(N, 0);
            for (int u = 0; u < T; ++u)
                for (int r = 0; r < E; ++r) {
                    const int i = slot01_read(u, r), a = L::rbase_01(u) + L::roff_01(r);
                    CHECK(a >= 0 && a < L::kElems && slot_at[a] == i, "0->1 reader u %d r %d reads slot %d, wants %d", u, r,
                          a >= 0 && a < L::kElems ? slot_at[a] : -2, i);
                    CHECK(!read[i], "0->1 slot %d read twice", i);
                    read[i] = 1;
                }
            // 3: ds_read_b32, 32 banks, 32-lane groups
            for (int r = 0; r < E; ++r)
                for (int g = 0; g < T / 32; ++g) {
                    unsigned long long banks = 0;
                    for (int l = 0; l < 32; ++l) banks |= 1ull << ((L::rbase_01(32 * g + l) + L::roff_01(r)) % 32);
                    CHECK(banks == 0xffffffffull, "0->1 read r %d group %d conflicts", r, g);
                }
        }
        // ---- exchange 1 -> 2
        {
            std::vector<int> slot_at(L::kElems, -1);
            for (int j = 0; j < T; ++j)
                for (int ip = 0; ip < E; ++ip) {
                    const int i = slot12_written(j, ip), wave = j / 64, lane = j % 64;
                    const int m0 = L::m0_12(wave, ip), off = L::off_12(ip);
                    const int byte = m0 + off + 4 * lane;
                    CHECK(byte == 4 * L::addr12(i), "1->2 writer j %d i' %d: %d vs %d", j, ip, byte, 4 * L::addr12(i));
                    CHECK(off >= 0 && off < 65536 && m0 >= 0 && m0 < 65536, "1->2 fields j %d i' %d", j, ip);
                    CHECK(m0 == L::m0_12(wave, ip < L::kRebias ? 0 : L::kRebias), "1->2 one M0 per half, j %d i' %d", j, ip);
                    CHECK(byte + 4 <= L::kBytes, "1->2 writer inside the image j %d i' %d", j, ip);
                    if (off > max_off) max_off = off;
                    if (m0 > max_m0) max_m0 = m0;
                    if (m0 + off + 252 > max_end) max_end = m0 + off + 252;
                    const int a = byte / 4;
                    CHECK(a >= 0 && a < L::kElems && slot_at[a] == -1, "1->2 writer collides j %d i' %d", j, ip);
                    if (a >= 0 && a < L::kElems) slot_at[a] = i;
                }
            std::vector<char> read(N, 0);
            constexpr int R2 = 16;
            for (int t = 0; t < T; ++t)
                for (int r = 0; r < R2; ++r) {
                    const int a = L::rbase_12(2 * t) + L::roff_12(r);       // one aligned 8-byte read: j2 = 2t, 2t + 1
                    CHECK(a % 2 == 0 && a + 1 < L::kElems, "1->2 pair t %d r %d not aligned", t, r);
                    for (int q = 0; q < 2; ++q) {
                        const int i = slot12_read(2 * t + q, r);
                        CHECK(a + q < L::kElems && slot_at[a + q] == i, "1->2 reader t %d q %d r %d", t, q, r);
                        CHECK(L::rbase_12(2 * t + q) + L::roff_12(r) == a + q, "1->2 second of the pair t %d r %d", t, r);
                        CHECK(!read[i], "1->2 slot %d read twice", i);
                        read[i] = 1;
                    }
                }
            // 4: ds_read_b64, 64 banks, 32-lane groups: every bank once
            for (int r = 0; r < R2; ++r)
                for (int g = 0; g < T / 32; ++g) {
                    unsigned long long banks = 0;
                    int hits = 0;
                    for (int l = 0; l < 32; ++l)
                        for (int q = 0; q < 2; ++q) {
                            const int b = (L::rbase_12(2 * (32 * g + l)) + L::roff_12(r) + q) % 64;
                            hits += (banks >> b) & 1;
                            banks |= 1ull << b;
                        }
                    CHECK(hits == 0 && banks == ~0ull, "1->2 read r %d group %d conflicts", r, g);
                }
        }
    }
    // 5: the instruction fields.  Offsets and M0 are 16-bit fields; the last lane's dword
    // (M0 + offset + 252) must lie inside the image.  (It cannot stay below 65536 as well: the
    // image is 69632 B and the last row of either layout ends beyond 64 KiB.)
    CHECK(max_off < 65536 && max_m0 < 65536, "fields %d %d", max_off, max_m0);
    CHECK(max_end + 4 <= L::kBytes, "last dword %d", max_end);
    // 6: two blocks per CU, image + pass-1 table each
    CHECK(2 * (L::kBytes + L::kTab1Bytes) <= 160 * 1024, "LDS %d", 2 * (L::kBytes + L::kTab1Bytes));
    CHECK(L::kBytes == 32 * 544 * 4 && WAVES == 8, "image bytes");
    std::printf("max_offset %d max_m0 %d max_m0_offset_252 %d image_bytes %d lds_two_blocks %d\n", max_off, max_m0,
                max_end, L::kBytes, 2 * (L::kBytes + L::kTab1Bytes));
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
