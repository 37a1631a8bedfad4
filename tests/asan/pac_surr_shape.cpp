// Host check of the surrogate kernels' geometry (nw_shape.h), built with -fsanitize=address,undefined by
// tests/test_pac_surr_cpu.py: the staged planes tile the scratch exactly (every (signal, listed scale, plane,
// sample) has one slot and the staging launch's threads write each slot once), the circular shift
// pac_surr_wrap is (j + l) mod T and visits every amplitude sample once per lag in two contiguous runs, and
// the lanes pac_surr_cell_lane gives a wave's cells are distinct and cover nw_pac_kernel's cells of the tile.
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
    // the scratch: as nw_pac_stage_kernel writes it and nw_pac_surr_kernel reads it
    for (int64_t nsig : {1, 3, 10})
        for (int nph : {1, 4, 9})
            for (int nam : {1, 5, 17})
                for (int64_t T : {0, 1, 49, 64, 255, 256, 257, 964}) {
                    const int64_t total = nw::pac_surr_stage_doubles(nsig, nph, nam, T);
                    CHECK(total == nsig * (2 * nph + nam) * T);
                    std::vector<int> hit((size_t)total, 0);
                    const int64_t nrows = nsig * (nph + nam);
                    const int64_t tiles = nw::pac_surr_stage_tiles(T);
                    const int64_t blocks = nw::pac_surr_stage_blocks(nrows, T);
                    CHECK(tiles * nw::kPacSurrStageThreads >= T && (tiles == 0 || (tiles - 1) * nw::kPacSurrStageThreads < T));
                    CHECK(blocks == nrows * tiles);
                    for (int64_t b = 0; b < blocks; ++b)
                        for (int th = 0; th < nw::kPacSurrStageThreads; ++th) {
                            const int64_t row = b / tiles, j = (b % tiles) * nw::kPacSurrStageThreads + th;
                            CHECK(row >= 0 && row < nrows);
                            if (j >= T) continue;
                            const bool is_phase = row < nsig * nph;
                            const int64_t r = is_phase ? row : row - nsig * nph;
                            const int nl = is_phase ? nph : nam;
                            const int64_t sig = r / nl, pos = r % nl;
                            CHECK(sig >= 0 && sig < nsig);
                            if (is_phase) {
                                const int64_t at = nw::pac_surr_phase_at(sig, pos, 0, nph, T) + j;
                                CHECK(nw::pac_surr_phase_at(sig, pos, 1, nph, T) + j == at + T);
                                CHECK(at >= 0 && at + T < total);
                                ++hit[(size_t)at];
                                ++hit[(size_t)(at + T)];
                            } else {
                                const int64_t at = nw::pac_surr_amp_at(nsig, sig, pos, nph, nam, T) + j;
                                CHECK(at >= nsig * 2 * nph * T && at < total);
                                ++hit[(size_t)at];
                            }
                        }
                    for (int h : hit) CHECK(h == 1);
                }
    // the circular shift: (j + l) mod T without %, a permutation of the window per lag, two contiguous runs
    for (int64_t T : {1, 2, 49, 64, 65, 964})
        for (int64_t l = 0; l < T; ++l) {
            std::vector<int> seen((size_t)T, 0);
            int breaks = 0;
            for (int64_t j = 0; j < T; ++j) {
                const int64_t jj = nw::pac_surr_wrap(j, l, T);
                CHECK(jj >= 0 && jj < T && jj == (j + l) % T);
                ++seen[(size_t)jj];
                if (j > 0 && jj != nw::pac_surr_wrap(j - 1, l, T) + 1) ++breaks;
            }
            for (int s : seen) CHECK(s == 1);
            CHECK(breaks == (l > 0 ? 1 : 0));
        }
    // a wave's cells: one lane each, the cells nw_pac_kernel's wave keeps
    std::vector<int> lane(64, 0);
    for (int k = 0; k < nw::kPacAmWave; ++k)
        for (int q = 0; q < nw::kPacPh; ++q) {
            const int ln = nw::pac_surr_cell_lane(k, q);
            CHECK(ln >= 0 && ln < 64 && ln / nw::kPacPh == k && ln % nw::kPacPh == q);
            ++lane[(size_t)ln];
        }
    for (int ln = 0; ln < 64; ++ln) CHECK(lane[(size_t)ln] == (ln < nw::kPacAmWave * nw::kPacPh ? 1 : 0));
    std::printf("ok\n");
    return 0;
}
