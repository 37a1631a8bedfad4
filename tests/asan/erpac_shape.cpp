// Host check of the event-related phase-amplitude coupling geometry (nw_shape.h), built with
// -fsanitize=address,undefined by tests/test_erpac_cpu.py: every (pair, phase tile, amplitude tile, sample
// tile) of a launch is computed by exactly one block of the grid erpac_blocks gives, in both block orders,
// the padding slots lie past the last pair, in the XCD order the scale tiles of one (pair, sample tile) are
// neighbours on one XCD, and the tiles cover every listed (phase, amplitude) position at every window sample
// exactly once, partial scale tiles and the tail sample tile included.
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

static void check_map(int npairs, int nph, int nam, int64_t count, bool xcd) {
    const int ntp = (int)nw::pac_tiles_ph(nph), nta = (int)nw::pac_tiles_am(nam);
    const int ntiles = (int)nw::pac_tiles(nph, nam);
    const int64_t nst = nw::erpac_sample_tiles(count);
    CHECK(nst == (count + nw::kConnTileN - 1) / nw::kConnTileN && ntiles == ntp * nta);
    const int64_t blocks = nw::erpac_blocks(npairs, nst, ntiles, xcd);
    if (count == 0 || npairs == 0) {   // nothing to launch: the slot map is never asked
        CHECK(blocks == 0);
        return;
    }
    CHECK(blocks >= npairs * nst * ntiles && blocks < (npairs * nst + 8) * ntiles);
    std::vector<int> hit((size_t)(npairs * nst * ntiles), 0);
    // every listed (phase position, amplitude position) of every pair at every window sample
    std::vector<int> cell((size_t)((int64_t)npairs * nph * nam * count), 0);
    for (int64_t b = 0; b < blocks; ++b) {
        const nw::ErpacSlot s = nw::erpac_slot(b, nst, ntiles, nta, xcd);
        CHECK(s.pair >= 0 && s.st >= 0 && s.st < nst && s.tp >= 0 && s.tp < ntp && s.ta >= 0 && s.ta < nta);
        if (s.pair >= npairs) continue;   // padding: the block returns
        ++hit[(size_t)(((s.pair * nst + s.st) * ntp + s.tp) * nta + s.ta)];
        // the tile's scales and samples, as the kernel bounds them
        const int p0 = s.tp * nw::kPacPh, a0 = s.ta * nw::kPacAm;
        const int nphl = nph - p0 < nw::kPacPh ? nph - p0 : nw::kPacPh;
        const int naml = nam - a0 < nw::kPacAm ? nam - a0 : nw::kPacAm;
        CHECK(nphl >= 1 && naml >= 1);
        int live = 0;
        for (int lane = 0; lane < nw::kConnTileN; ++lane) {
            const int64_t j = s.st * nw::kConnTileN + lane;
            if (j >= count) continue;     // a lane past the window neither loads nor stores
            ++live;
            for (int w = 0; w < nw::kPacWaves; ++w)
                for (int k = 0; k < nw::kPacAmWave; ++k) {
                    const int a = w * nw::kPacAmWave + k;
                    if (a >= naml) continue;
                    for (int q = 0; q < nphl; ++q)
                        ++cell[(size_t)((((int64_t)s.pair * nph + p0 + q) * nam + a0 + a) * count + j)];
                }
        }
        CHECK(live >= 1 && (live == nw::kConnTileN || s.st == nst - 1));
        if (xcd && (s.tp > 0 || s.ta > 0)) {   // the previous scale tile: 8 blocks back, same XCD
            const nw::ErpacSlot prev = nw::erpac_slot(b - 8, nst, ntiles, nta, true);
            CHECK(prev.pair == s.pair && prev.st == s.st && prev.tp * nta + prev.ta == s.tp * nta + s.ta - 1);
        }
    }
    for (int h : hit) CHECK(h == 1);
    for (int c : cell) CHECK(c == 1);
}

int main() {
    for (int npairs : {0, 1, 2, 5})
        for (int nph : {1, 8, 9})
            for (int nam : {5, 16, 17, 48})
                for (int64_t count : {0, 1, 63, 64, 65, 1201})
                    for (int xcd = 0; xcd < 2; ++xcd) check_map(npairs, nph, nam, count, xcd != 0);
    // the partial tiles of the 9 x 17 case at n = 1201: 4 scale tiles, 19 sample tiles, the last of 49 samples
    CHECK(nw::pac_tiles(9, 17) == 4 && nw::erpac_sample_tiles(1201) == 19 && 1201 - 18 * nw::kConnTileN == 49);
    CHECK(nw::erpac_blocks(3, 19, 4, false) == 3 * 19 * 4 && nw::erpac_blocks(3, 19, 4, true) == 64 * 4);
    CHECK(nw::erpac_blocks(3, 0, 4, true) == 0 && nw::erpac_blocks(3, 19, int64_t(1) << 31, true) == -1);
    std::printf("ok\n");
    return 0;
}
