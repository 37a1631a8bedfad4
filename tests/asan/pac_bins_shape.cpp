// Host check of the phase-binned coupling geometry (nw_shape.h), built with -fsanitize=address,undefined by
// tests/test_pac_bins_cpu.py: for every nbins class, every (epoch, pair, listed phase scale, amplitude tile) of a
// launch is computed by exactly one block of the grid pac_blocks gives, in both block orders, the padding slots
// lie past the chunk's epochs, the amplitude tiles cover every listed (phase, amplitude) position exactly once,
// partial tiles included, and the LDS a block declares fits a CU (two blocks of it).
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
    for (int nbins = -2; nbins <= 40; ++nbins) {
        const bool ok = nbins >= 2 && nbins <= NW_PAC_MAX_BINS && nbins % 2 == 0;
        CHECK(nw::pac_bins_valid(nbins) == ok);
        if (!ok) continue;
        const nw::PacBinsGeom g = nw::pac_bins_geom(nbins);
        CHECK(g.cap >= nbins && g.cap <= nw::kPacBinsMax && g.ka >= 1);
        CHECK(nw::pac_bins_am(nbins) == nw::kPacBinsWaves * g.ka);
        // the accumulators [wave][bin * ka + k][lane] in fp64, the bin indices [2][wave][lane] and the edge table
        const int64_t lds = (int64_t)nw::kPacBinsWaves * g.cap * g.ka * nw::kConnTileN * 8 +
                            2 * nw::kPacBinsWaves * nw::kConnTileN * 4 + g.cap * 16;
        CHECK(nw::pac_bins_lds(nbins) == lds);
        CHECK(lds <= 163840 && 2 * lds <= 163840);
        // the last accumulator a lane can address lies inside its wave's rows
        CHECK((nbins - 1) * g.ka + (g.ka - 1) < g.cap * g.ka);
    }
    CHECK(nw::pac_bins_lds(2) <= 163840 && nw::pac_bins_lds(18) <= 163840 && nw::pac_bins_lds(36) <= 163840);
    CHECK(nw::pac_bins_am(2) == 16 && nw::pac_bins_am(18) == 8 && nw::pac_bins_am(36) == 4);

    for (int nbins : {2, 8, 10, 18, 20, 36})
        for (int64_t ec : {1, 2, 3, 16})
            for (int npairs : {1, 2, 5, 9})
                for (int nph : {1, 4, 9})
                    for (int nam : {1, 4, 5, 8, 9, 16, 17, 48})
                        for (int xcd = 0; xcd < 2; ++xcd) {
                            const int am = nw::pac_bins_am(nbins), ka = nw::pac_bins_geom(nbins).ka;
                            const int nta = (int)nw::pac_bins_tiles_am(nam, nbins);
                            const int ntiles = (int)nw::pac_bins_tiles(nph, nam, nbins);
                            CHECK(nta == (nam + am - 1) / am && ntiles == nph * nta);
                            const int64_t blocks = nw::pac_blocks(ec, npairs, ntiles, xcd != 0);
                            CHECK(blocks >= ec * npairs * ntiles && blocks < (ec * npairs + 8) * ntiles);
                            std::vector<int> hit((size_t)(ec * npairs * ntiles), 0);
                            // every listed (phase position, amplitude position) of every (epoch, pair)
                            std::vector<int> cell((size_t)(ec * npairs * nph * nam), 0);
                            for (int64_t b = 0; b < blocks; ++b) {
                                const nw::PacSlot s = nw::pac_slot(b, npairs, ntiles, nta, xcd != 0);
                                CHECK(s.e >= 0 && s.pair >= 0 && s.pair < npairs && s.tp >= 0 && s.tp < nph && s.ta >= 0 &&
                                      s.ta < nta);
                                if (s.e >= ec) continue;   // padding: the block returns
                                ++hit[(size_t)(((s.e * npairs + s.pair) * nph + s.tp) * nta + s.ta)];
                                // the tile's amplitude scales, as the kernel bounds them
                                const int a0 = s.ta * am;
                                const int naml = nam - a0 < am ? nam - a0 : am;
                                CHECK(naml >= 1);
                                for (int w = 0; w < nw::kPacBinsWaves; ++w) {
                                    const int mine = naml - w * ka < ka ? naml - w * ka : ka;
                                    for (int k = 0; k < mine; ++k)
                                        ++cell[(size_t)(((s.e * npairs + s.pair) * nph + s.tp) * nam + a0 + w * ka + k)];
                                }
                                if (xcd && (s.tp > 0 || s.ta > 0)) {   // the previous tile: 8 blocks back, same XCD
                                    const nw::PacSlot prev = nw::pac_slot(b - 8, npairs, ntiles, nta, true);
                                    CHECK(prev.e == s.e && prev.pair == s.pair && prev.tp * nta + prev.ta == s.tp * nta + s.ta - 1);
                                }
                            }
                            for (int h : hit) CHECK(h == 1);
                            for (int c : cell) CHECK(c == 1);
                        }
    // the partial tiles of the 9 x 17 case, per class
    CHECK(nw::pac_bins_tiles(9, 17, 18) == 27 && nw::pac_bins_tiles(9, 17, 36) == 45 && nw::pac_bins_tiles(9, 17, 2) == 18);
    CHECK(nw::pac_blocks(0, 3, 27, true) == 0 && nw::pac_bins_tiles(0, 17, 18) == 0 && nw::pac_bins_tiles(9, 0, 18) == 0);
    std::printf("ok\n");
    return 0;
}
