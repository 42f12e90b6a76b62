// Host replay of wino6q_kernel's per-tile phase schedule (transeditor_amd/csrc/wino6_schedule.h): tests/test_wino6_schedule.py compiles
// and runs this program.  usage: wino6_schedule_check NTILE NSTAGE; exit status 0 = every property holds, 1 = a violation (printed).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "wino6_schedule.h"

using namespace wino6_sched;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++fails; std::printf("VIOLATION: " __VA_ARGS__); std::printf("\n"); } } while (0)

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int ntile = std::atoi(argv[1]), nstage = std::atoi(argv[2]);
    std::vector<Event> ev[2];
    for (int g = 0; g < 2; ++g) replay(g, nstage, ntile, [&](Event e) { ev[g].push_back(e); });
    // epochs: what a group does between two barriers.  Every wave of the block is somewhere inside the same epoch at any time.
    std::vector<std::vector<Event>> ep[2];
    for (int g = 0; g < 2; ++g) {
        ep[g].emplace_back();
        for (const Event& e : ev[g]) {
            if (e.kind == BARRIER) ep[g].emplace_back();
            else ep[g].back().push_back(e);
        }
    }
    CHECK(ep[0].size() == ep[1].size(), "barrier counts differ: group 0 %zu, group 1 %zu", ep[0].size() - 1, ep[1].size() - 1);
    if (fails) return 1;
    // per tile too: the epilogues of a tile lie in epochs that both groups reach
    struct Half { int tile = -1, img = -1; bool valid = false; } u[2];            // weight halves Ua, Ub: what they hold
    struct Tile { int tile = -1, stage = -1; } t[2];                                // half tiles T0, T1
    int epilogues[2] = {0, 0};
    for (size_t k = 0; k < ep[0].size(); ++k) {
        bool u_read[2] = {false, false}, u_dma[2] = {false, false}, t_read[2] = {false, false}, t_write[2] = {false, false};
        Half u_new[2]; Tile t_new[2];
        for (int g = 0; g < 2; ++g) {
            bool mine[2] = {false, false};           // halves whose DMA THIS group issued in this epoch and has not waited for: a wait
                                                     // completes a group's own DMAs only, never those of the other group
            for (const Event& e : ep[g][k]) {
                switch (e.kind) {
                case READ_UA: case READ_UB: {
                    const int h = e.kind == READ_UB;
                    u_read[h] = true;
                    CHECK(u[h].valid && u[h].tile == e.tile && u[h].img == e.idx, "epoch %zu: group %d reads U%c for (tile %d, image %d), it holds (%d, %d)%s",
                          k, g, "ab"[h], e.tile, e.idx, u[h].tile, u[h].img, u[h].valid ? "" : " [DMA not waited for]");
                    break;
                }
                case DMA_UA: case DMA_UB: {
                    const int h = e.kind == DMA_UB;
                    CHECK(!u_dma[h], "epoch %zu: U%c is renewed twice between the same two barriers", k, "ab"[h]);
                    u_dma[h] = true; mine[h] = true;
                    u_new[h].tile = e.tile; u_new[h].img = e.idx; u_new[h].valid = false;
                    break;
                }
                case DMA_WAIT:
                    for (int h = 0; h < 2; ++h) if (mine[h]) { u_new[h].valid = true; mine[h] = false; }
                    break;
                case READ_T:
                    t_read[g] = true;
                    CHECK(t[g].tile == e.tile && t[g].stage == e.idx, "epoch %zu: group %d reads T for (tile %d, stage %d), it holds (%d, %d)", k, g, e.tile, e.idx,
                          t[g].tile, t[g].stage);
                    break;
                case WRITE_T:
                    t_write[g] = true; t_new[g].tile = e.tile; t_new[g].stage = e.idx;
                    break;
                case EPILOGUE: ++epilogues[g]; break;
                }
            }
            CHECK(!mine[0] && !mine[1], "epoch %zu: group %d passes a barrier with a weight DMA in flight", k, g);
            // a group's waves are not in step inside an epoch: a half tile is never read and written between the same two barriers
            CHECK(!(t_read[g] && t_write[g]), "epoch %zu: group %d reads and writes its half tile between the same two barriers", k, g);
        }
        for (int h = 0; h < 2; ++h) {
            CHECK(!(u_read[h] && u_dma[h]), "epoch %zu: U%c is renewed while it can still be read", k, "ab"[h]);
            if (u_dma[h]) u[h] = u_new[h];
        }
        for (int g = 0; g < 2; ++g) if (t_write[g]) t[g] = t_new[g];
    }
    CHECK(epilogues[0] == ntile && epilogues[1] == ntile, "epilogues: %d, %d for %d tiles", epilogues[0], epilogues[1], ntile);
    // equal barrier counts per TILE (between consecutive epilogues), not only per block
    std::vector<int> per[2];
    for (int g = 0; g < 2; ++g) {
        int n = 0;
        for (const Event& e : ev[g]) { if (e.kind == BARRIER) ++n; if (e.kind == EPILOGUE) { per[g].push_back(n); n = 0; } }
    }
    for (size_t i = 0; i < per[0].size() && i < per[1].size(); ++i)
        CHECK(per[0][i] == per[1][i], "tile %zu: %d barriers in group 0, %d in group 1", i, per[0][i], per[1][i]);
    if (!fails) std::printf("ok: %d tiles x %d stages, %zu barriers per group\n", ntile, nstage, ep[0].size() - 1);
    return fails ? 1 : 0;
}
