// Host check of the phase-amplitude coupling geometry (nw_shape.h), built with -fsanitize=address,undefined
// by tests/test_pac_cpu.py: every (epoch, pair, phase tile, amplitude tile) of a launch is computed by
// exactly one block of the grid pac_blocks gives, in both block orders, the padding slots lie past the
// chunk's epochs, in the XCD order the scale tiles of one (epoch, pair) are neighbours on one XCD, and the
// scale tiles cover every listed (phase, amplitude) position exactly once, partial tiles included.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ninwavelets_amd/csrc/nw_shape.h"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

int main() {
    for (int64_t ec : {1, 2, 3, 16})
        for (int npairs : {1, 2, 5, 9})
            for (int nph : {1, 4, 8, 9, 16, 17})
                for (int nam : {1, 5, 16, 17, 48})
                    for (int xcd = 0; xcd < 2; ++xcd) {
                        const int ntp = (int)nw::pac_tiles_ph(nph), nta = (int)nw::pac_tiles_am(nam);
                        const int ntiles = (int)nw::pac_tiles(nph, nam);
                        CHECK(ntp == (nph + nw::kPacPh - 1) / nw::kPacPh && nta == (nam + nw::kPacAm - 1) / nw::kPacAm);
                        CHECK(ntiles == ntp * nta);
                        const int64_t blocks = nw::pac_blocks(ec, npairs, ntiles, xcd != 0);
                        CHECK(blocks >= ec * npairs * ntiles && blocks < (ec * npairs + 8) * ntiles);
                        std::vector<int> hit((size_t)(ec * npairs * ntiles), 0);
                        // every listed (phase position, amplitude position) of every (epoch, pair)
                        std::vector<int> cell((size_t)(ec * npairs * nph * nam), 0);
                        for (int64_t b = 0; b < blocks; ++b) {
                            const nw::PacSlot s = nw::pac_slot(b, npairs, ntiles, nta, xcd != 0);
                            CHECK(s.e >= 0 && s.pair >= 0 && s.pair < npairs && s.tp >= 0 && s.tp < ntp && s.ta >= 0 &&
                                  s.ta < nta);
                            if (s.e >= ec) continue;   // padding: the block returns
                            ++hit[(size_t)(((s.e * npairs + s.pair) * ntp + s.tp) * nta + s.ta)];
                            // the tile's scales, as the kernel bounds them
                            const int p0 = s.tp * nw::kPacPh, a0 = s.ta * nw::kPacAm;
                            const int nphl = nph - p0 < nw::kPacPh ? nph - p0 : nw::kPacPh;
                            const int naml = nam - a0 < nw::kPacAm ? nam - a0 : nw::kPacAm;
                            CHECK(nphl >= 1 && naml >= 1);
                            for (int w = 0; w < nw::kPacWaves; ++w)
                                for (int k = 0; k < nw::kPacAmWave; ++k) {
                                    const int a = w * nw::kPacAmWave + k;
                                    if (a >= naml) continue;
                                    for (int q = 0; q < nphl; ++q)
                                        ++cell[(size_t)(((s.e * npairs + s.pair) * nph + p0 + q) * nam + a0 + a)];
                                }
                            if (xcd && (s.tp > 0 || s.ta > 0)) {   // the previous scale tile: 8 blocks back, same XCD
                                const nw::PacSlot prev = nw::pac_slot(b - 8, npairs, ntiles, nta, true);
                                CHECK(prev.e == s.e && prev.pair == s.pair && prev.tp * nta + prev.ta == s.tp * nta + s.ta - 1);
                            }
                        }
                        for (int h : hit) CHECK(h == 1);
                        for (int c : cell) CHECK(c == 1);
                    }
    // the partial tiles of the 9 x 17 case
    CHECK(nw::pac_tiles_ph(9) == 2 && nw::pac_tiles_am(17) == 2 && nw::pac_tiles(9, 17) == 4);
    CHECK(nw::pac_blocks(0, 3, 4, true) == 0 && nw::pac_blocks(0, 3, 4, false) == 0);
    // every wave stages whole slots: the staging slots w + q * kPacWaves cover each slot once
    for (int total : {nw::kPacPh, nw::kPacAm}) {
        std::vector<int> slot((size_t)total, 0);
        for (int w = 0; w < nw::kPacWaves; ++w)
            for (int q = 0; q < total / nw::kPacWaves; ++q) ++slot[(size_t)(w + q * nw::kPacWaves)];
        for (int s : slot) CHECK(s == 1);
    }
    std::printf("ok\n");
    return 0;
}
