// The per-tile phase schedule of wino6q_kernel (wino6.hip), written ONCE: who multiplies, who stages, which weight half a staging phase
// renews, which stage a multiplying phase fetches, and where the barriers are.  The kernel takes every such decision from the functions
// below; `replay` walks the same functions in the kernel's loop structure and emits one event per LDS access, DMA and barrier, so that a
// host program (tests/test_wino6_schedule.py compiles this header with the host compiler) can check what a GPU run must never be asked to
// find out: that the two wave groups of a block execute the same number of s_barriers whatever the tile list looks like (a mismatch is a
// hang), and that no weight half or half tile is read before it is complete or renewed while it can still be read.
//
// A block walks a list of tiles.  Per tile, with n = nstage channel stages and the weight images j = 2 s + m (stage s, 64-channel half m):
//     group 0:        [M0(s) SA M1(s) SB] x n   (+ 2 barriers if a tile follows)   epilogue
//     group 1:   S    [M0(s) SA M1(s) SB] x n   (the last SB only if a tile follows) epilogue
// Every phase has two barriers (mid, end); group 1 runs one phase behind group 0.  In the phase loop of a tile the local phase index ph
// (group 0: 0 .. 4 n - 1, group 1: 0 .. 4 n) names the pair of phases that run side by side.  A staging phase ph renews half of image
// cs = (ph + 1) / 2: group 1 (even ph) the second half, Ub, in FRONT of the mid barrier; group 0 (odd ph) the first half, Ua, BEHIND it.
// cs == 2 n is image 0 of the NEXT tile (same M block, so the same weights): the last SB of either group carries the next tile's weights
// in, and its write_res the next tile's T_g(0), whose fetch replaced the clamped re-fetch of the last stage.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define W6S_HD __host__ __device__ __forceinline__
#else
#define W6S_HD inline
#endif

namespace wino6_sched {

// group 1 opens every tile with a staging phase of its own (no work in it: two barriers beside group 0's M0(0))
W6S_HD constexpr bool lead_phase(int grp) { return grp == 1; }
// image whose half the staging phase `ph` renews
W6S_HD constexpr int renew_image(int ph) { return (ph + 1) >> 1; }
// ... and whether there is anything to renew: not image 0 of the block's first tile (the prologue brought it in), and the image behind the
// tile's last one only where a tile follows
W6S_HD constexpr bool renew_work(int cs, int nimg, bool has_next) { return cs >= 1 && (cs < nimg || has_next); }
// the stage the M0 phase of stage s fetches; `next_tile`: it is stage 0 of the next tile (the staging geometry is switched in front of
// that phase).  A list's last tile fetches its last stage again (the results are never written).
W6S_HD constexpr int fetch_stage(int s, int nstage, bool has_next, bool& next_tile) {
    next_tile = s == nstage - 1 && has_next;
    return s + 1 < nstage ? s + 1 : (has_next ? 0 : s);
}
// does the group run the SB phase of stage s?  (group 1 is one phase late: behind the list's last tile its last SB has no partner)
W6S_HD constexpr bool runs_sb(int grp, int s, int nstage, bool has_next) { return !(grp == 1 && s == nstage - 1) || has_next; }
// barriers group 0 executes behind its last SB, beside group 1's last SB, where a tile follows
W6S_HD constexpr int tail_barriers(int grp, bool has_next) { return grp == 0 && has_next ? 2 : 0; }

#if !defined(__HIP_DEVICE_COMPILE__)
enum Kind { BARRIER, READ_UA, READ_UB, DMA_UA, DMA_UB, DMA_WAIT, READ_T, WRITE_T, EPILOGUE };
// tile = position in the block's list, idx = weight image (2 s + m) or stage of the half tile; WRITE_T with tile < 0: stale data
struct Event { int kind, tile, idx; };

// the events of group `grp` of a block that walks `ntile` tiles of `nstage` stages, in program order (emit(Event))
template <class F>
void replay(int grp, int nstage, int ntile, F&& emit) {
    const int nimg = 2 * nstage;
    auto ev = [&](int k, int t = 0, int i = 0) { emit(Event{k, t, i}); };
    auto multiply = [&](int t, int s, int m) {
        ev(READ_T, t, s); ev(READ_UA, t, 2 * s + m);
        ev(BARRIER);
        ev(READ_T, t, s); ev(READ_UB, t, 2 * s + m);
        ev(BARRIER);
    };
    auto stage = [&](int t, int ph, bool has_next, bool write, int wt, int ws) {
        const int cs = renew_image(ph);
        const bool work = renew_work(cs, nimg, has_next);
        const int it = cs == nimg ? t + 1 : t, ii = cs == nimg ? 0 : cs;
        if (grp == 1 && work) ev(DMA_UB, it, ii);
        if (write) ev(WRITE_T, wt, ws);
        if (grp == 1 && work) ev(DMA_WAIT);
        ev(BARRIER);
        if (grp == 0 && work) { ev(DMA_UA, it, ii); ev(DMA_WAIT); }
        ev(BARRIER);
    };
    // prologue of the block's first tile
    if (grp == 0) { ev(DMA_UA, 0, 0); ev(DMA_UB, 0, 0); }
    ev(WRITE_T, 0, 0);
    ev(DMA_WAIT);
    ev(BARRIER);
    for (int t = 0; t < ntile; ++t) {
        const bool has_next = t + 1 < ntile;
        int ph = 0;
        if (lead_phase(grp)) { stage(t, 0, has_next, false, 0, 0); ph = 1; }
        for (int s = 0; s < nstage; ++s) {
            bool next_tile = false;
            const int fs = fetch_stage(s, nstage, has_next, next_tile);
            const bool stale = fs == s;
            multiply(t, s, 0);
            stage(t, ph + 1, has_next, false, 0, 0);
            multiply(t, s, 1);
            if (runs_sb(grp, s, nstage, has_next)) stage(t, ph + 3, has_next, true, stale ? -1 : t + (next_tile ? 1 : 0), fs);
            ph += 4;
        }
        for (int i = 0; i < tail_barriers(grp, has_next); ++i) ev(BARRIER);
        ev(EPILOGUE, t);
    }
}
#endif

}  // namespace wino6_sched
