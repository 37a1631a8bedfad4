// Host check of the over-time connectivity geometry (nw_shape.h), built with -fsanitize=address,undefined
// by tests/test_conn_time_cpu.py: every (epoch, scale, pair tile) of a launch is computed by exactly one
// block of the grid conn_time_blocks gives, in both block orders, the padding slots lie past the chunk's
// epochs, and in the XCD order the pair tiles of one (e, f) are neighbours on one XCD; the window's
// sample count and the lane of a sample against their definitions.
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
        for (int nfreq : {1, 3, 9, 64})
            for (int ntiles : {1, 2, 3, 9})
                for (int xcd = 0; xcd < 2; ++xcd) {
                    const int64_t blocks = nw::conn_time_blocks(ec, nfreq, ntiles, xcd != 0);
                    CHECK(blocks >= ec * nfreq * ntiles && blocks < (ec * nfreq + 8) * ntiles);
                    std::vector<int> hit((size_t)(ec * nfreq * ntiles), 0);
                    for (int64_t b = 0; b < blocks; ++b) {
                        const nw::ConnTimeSlot s = nw::conn_time_slot(b, nfreq, ntiles, xcd != 0);
                        CHECK(s.e >= 0 && s.f >= 0 && s.f < nfreq && s.tile >= 0 && s.tile < ntiles);
                        if (s.e < ec) ++hit[(size_t)((s.e * nfreq + s.f) * ntiles + s.tile)];
                        if (xcd && s.tile > 0) {   // the previous pair tile of this (e, f): 8 blocks back, same XCD
                            const nw::ConnTimeSlot prev = nw::conn_time_slot(b - 8, nfreq, ntiles, true);
                            CHECK(prev.e == s.e && prev.f == s.f && prev.tile == s.tile - 1);
                        }
                    }
                    for (int h : hit) CHECK(h == 1);
                }
    for (int64_t step : {1, 2, 3, 4, 7})
        for (int64_t t0 = 0; t0 <= 70; ++t0)
            for (int64_t t1 = t0; t1 <= 200; t1 += 3) {
                int64_t count = 0;
                for (int64_t t = t0; t < t1; t += step) ++count;
                CHECK(nw::conn_time_count(t0, t1, step) == count);
                CHECK(count == 0 || t0 + (count - 1) * step < t1);
                CHECK(nw::conn_time_tiles(count) * nw::kConnTileN >= count &&
                      (nw::conn_time_tiles(count) - 1) * nw::kConnTileN < count + (count == 0 ? nw::kConnTileN : 0));
            }
    for (int64_t j = 0; j < 1000; ++j) CHECK(nw::conn_time_lane(j) == (int)(j & 63));
    std::printf("ok\n");
    return 0;
}
