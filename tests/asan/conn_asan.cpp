// conn_asan.cpp — CPU driver for the host side of multi-channel connectivity, built with
// -fsanitize=address,undefined together with ninwavelets_amd/csrc/nw_host.cpp
// (tests/test_conn_cpu.py): the pair tiler nw::host::conn_tiles on all-pairs, seed, random and
// degenerate lists (every pair in one tile, slots inside the tile's channel list, limits kept, the
// m (m + 1) / 2 bound), and the kernel's block order nw::conn_slot (nw_shape.h): every (unit, tile)
// of a launch is computed by exactly one block of the grid conn_blocks gives, in both orders.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "../../ninwavelets_amd/csrc/nw_host.h"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static size_t check_tiling(const std::vector<int32_t>& ia, const std::vector<int32_t>& ib) {
    const int64_t np = (int64_t)ia.size();
    std::vector<int32_t> tile_of((size_t)np, -1);
    const std::vector<nw::ConnTile> tiles = nw::host::conn_tiles(ia.data(), ib.data(), np, tile_of.data());
    std::vector<int> seen((size_t)np, 0);
    for (size_t t = 0; t < tiles.size(); ++t) {
        const nw::ConnTile& tl = tiles[t];
        CHECK(tl.npairs >= 1 && tl.npairs <= nw::kConnPairs);
        CHECK(tl.nch >= 1 && tl.nch <= nw::kConnCh);
        std::set<int32_t> distinct(tl.ch, tl.ch + tl.nch);
        CHECK((int)distinct.size() == tl.nch);
        for (int k = 0; k < tl.npairs; ++k) {
            const int32_t p = tl.out[k];
            CHECK(p >= 0 && p < np);
            CHECK(tl.sa[k] >= 0 && tl.sa[k] < tl.nch && tl.sb[k] >= 0 && tl.sb[k] < tl.nch);
            CHECK(tl.ch[tl.sa[k]] == ia[(size_t)p] && tl.ch[tl.sb[k]] == ib[(size_t)p]);
            CHECK(tile_of[(size_t)p] == (int32_t)t);
            ++seen[(size_t)p];
        }
    }
    for (int64_t p = 0; p < np; ++p) CHECK(seen[(size_t)p] == 1);
    // null tile_of_pair
    CHECK(nw::host::conn_tiles(ia.data(), ib.data(), np, nullptr).size() == tiles.size());
    return tiles.size();
}

int main() {
    for (int c = 1; c <= 70; ++c) {   // all pairs a < b
        std::vector<int32_t> ia, ib;
        for (int a = 0; a < c; ++a)
            for (int b = a + 1; b < c; ++b) ia.push_back(a), ib.push_back(b);
        const size_t m = (size_t)(c + 7) / 8;
        const size_t n = check_tiling(ia, ib);
        CHECK(n <= m * (m + 1) / 2);
        CHECK((n == 0) == (c == 1));
    }
    {   // one seed against 40 channels: 15 partners per tile
        std::vector<int32_t> ia(40, 0), ib;
        for (int b = 0; b < 40; ++b) ib.push_back(b);
        CHECK(check_tiling(ia, ib) == 3);
    }
    std::mt19937 rng(12);
    for (int rep = 0; rep < 200; ++rep) {   // any list: repeats, a > b, a == b
        const int c = 1 + (int)(rng() % 90);
        const size_t np = rng() % 700;
        std::vector<int32_t> ia(np), ib(np);
        for (size_t p = 0; p < np; ++p) ia[p] = (int32_t)(rng() % c), ib[p] = (int32_t)(rng() % c);
        const size_t n = check_tiling(ia, ib);
        CHECK(n >= (np + nw::kConnPairs - 1) / nw::kConnPairs);
    }
    CHECK(check_tiling({}, {}) == 0);
    CHECK(check_tiling({5}, {5}) == 1);

    // the block order: a bijection from the live blocks onto units x tiles
    for (int xcd = 0; xcd < 2; ++xcd)
        for (int64_t nunits : {1, 7, 8, 9, 64, 171, 19 * 9})
            for (int ntiles : {1, 2, 3, 9, 36}) {
                const int64_t blocks = nw::conn_blocks(nunits, ntiles, xcd != 0);
                CHECK(blocks >= nunits * ntiles && blocks < nunits * ntiles + 8 * ntiles);
                std::vector<int> hit((size_t)(nunits * ntiles), 0);
                for (int64_t b = 0; b < blocks; ++b) {
                    const nw::ConnSlot s = nw::conn_slot(b, ntiles, xcd != 0);
                    CHECK(s.tile >= 0 && s.tile < ntiles && s.unit >= 0);
                    if (s.unit < nunits) ++hit[(size_t)(s.unit * ntiles + s.tile)];
                    // XCD order: the tiles of a unit sit on one XCD (b mod 8), consecutively
                    if (xcd && s.tile > 0) {
                        const nw::ConnSlot prev = nw::conn_slot(b - 8, ntiles, true);
                        CHECK(prev.unit == s.unit && prev.tile == s.tile - 1);
                    }
                }
                for (int h : hit) CHECK(h == 1);
            }
    CHECK(nw::conn_units(9, 1201) == 9 * 19 && nw::conn_units(3, 64) == 3 && nw::conn_units(3, 65) == 6);
    std::printf("ok\n");
    return 0;
}
