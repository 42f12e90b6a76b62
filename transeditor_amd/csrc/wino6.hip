// F1w6: the 1-D Winograd F(2,3) form of the 3x3 / stride 1 / pad 1 convolution (wino.hip) with its multiply-adds on the BF16 matrix
// pipe and fp32-equivalent results (round 4, kind TE_CONV_3X3W6).
//
// Every fp32 operand x is split into three bf16 pieces  x = h + m + l  (h = bf16(x), m = bf16(x - h), l = bf16(x - h - m): 8 + 8 + 8
// mantissa bits, exact to 2^-25 relative).  A product of two bf16 numbers is exact in fp32, so
//     a b  =  ah bh + (ah bm + am bh) + (ah bl + am bm + al bh)  +  O(2^-24 |a b|)
// is six MFMAs of v_mfma_f32_32x32x16_bf16 accumulated in fp32 - the three dropped cross terms (am bl, al bm, al bl) are below the
// rounding unit of the fp32 product.  Measured on the MI355X (tools/exp/bf16x_probe.hip, profiles/experiments/r04_bf16_split_probe.log):
// a 64 x 64 x 1152 product against double: 5.3e-7 relative (L2) for the six-product form, 6.2e-7 for the native fp32 MFMA chain - the
// split form is not "reduced precision", it is fp32 arithmetic on a different pipe - while the bf16 pipe sustains 1 490 - 1 530 TFLOP/s
// with its operands coming from LDS one 16-byte read per MFMA, i.e. 250 fp32-equivalent TFLOP/s against the 134 the fp32 matrix
// instructions reach at the clock the chip sustains.  The tests that pin the fp32 kernels (tests/test_gpu_winograd.py: 5e-6 against fp64)
// pin this one at the same bar.
//
// Data flow per stage of 16 input channels (one MFMA K step):
//   weights  : packed by te_conv_pack_weights (TE_PACK_W6FWD / TE_PACK_W6DGRAD) as U = G w, split, in MFMA FRAGMENT order
//              U6[K/16][piece][ky][component][M/32][64 lanes][8 bf16]  ->  a stage's slots are copied 16 bytes per lane to LDS
//   input    : d = style scale * in, t = B^T d (fp32, as in wino.hip), split, two channels packed per dword, written to
//              T[piece][component][row][k half][pair][8 bf16]: a wave's B operand is one conflict-free ds_read_b128 per piece
//   products : per (tap row, component): 3 + 3 operand reads, 6 MFMAs into the component's accumulator tile
// Block: 512 threads, tile 64 output channels x 8 rows x 32 columns.  Epilogue = wino.hip's (output transform, demodulation scale, bias,
// leaky ReLU, residual, mask).
#include "split6_common.h"
#include "wino6_schedule.h"
#ifdef W6P_PROF      // experimental builds: per-wave cycle counts of the phases, read back with te_debug_w6p_prof (tools/w6p_phase_prof.py)
#define TE_PROF
#endif
#include "te_prof.h"

namespace {

constexpr int WT = 512, KC = 16, TW = 32, NP = TW / 2, BM = 64, TH = 8;
constexpr int U_CHUNKS = 36 * 2 * 64;                   // 16-byte chunks of a stage's weights: [piece 3][ky 3][c 4][mtile 2][64 lanes]

struct Wino6Args {
    float* out; const float* in; const u32x4* U; const float* isc; const float* osc; const float* bias; const float* res;
    const float* mref; float mgain; int act;
    int B, K, M, H, W, ntiles, mblocks, tiles_x, tiles_y, nt8;
    int lists;     // wino6q_kernel: runs per XCD the tile list is cut into (0 = one tile per block: split6_tile)
    int lgpw;      // log2 of the column PAIRS one sample contributes to a tile row: 4 (W >= 32); 3 (W == 16: two samples side by side, round 6)
};

// ---------------------------------------------------------------------------------------------------------------------------------
// Round 5: the PING-PONG form (wino6p_kernel).  The round-4 form alternated "all eight waves multiply" and "all eight waves stage"
// between two block-wide barriers, so the matrix pipe idled while the next stage was transformed, split and written (measured: 36 % of
// the kernel).  Double-buffering the whole stage does not fit (2 x 132 KB), so the tile is cut the other way:
//
//   * the 8-row tile is two HALF tiles of 4 rows (6 input rows each, 36 KB of transformed pieces per half: T0, T1); the weights of a
//     stage (72 KB) stay ONE image shared by both halves: 144 KB of LDS;
//   * waves 0-3 (group 0) own half 0, waves 4-7 (group 1) own half 1.  Waves w and w + 4 share a SIMD, so every SIMD holds one wave
//     of each group.  The groups run half a stage apart:
//         phase X(s): group 0 multiplies  T0(s) x U(s)   |  group 1 transforms / splits / writes T1(s)
//         phase Y(s): group 1 multiplies  T1(s) x U(s)   |  group 0 transforms / splits / writes T0(s + 1)
//     i.e. on every SIMD one wave feeds the matrix pipe while its partner does the vector-ALU / LDS-write / DMA work of staging
//     (the arrangement MI355X_MICROARCH.md "Two waves per SIMD" describes for attention: matrix beside memory, never matrix beside
//     matrix).  A half tile is private to its group, so the only hand-off between the groups is the weight image;
//   * the weight image is renewed in two halves without a second buffer.  A multiplying wave walks the 12 (tap row, component)
//     groups in order; the first six read Ua, the last six Ub.  Ua(s) is dead once group 1 is past the middle of Y(s): group 0 (then
//     staging) issues the DMA of Ua(s + 1) right behind that mid-phase barrier and waits for it before the end-of-phase barrier.
//     Ub(s - 1) is dead at the end of Y(s - 1): group 1 (staging in X(s)) issues Ub(s) first thing and waits before the mid-phase
//     barrier of X(s), behind which group 0 starts to read it.  Four barriers per stage (mid-X, end-X, mid-Y, end-Y), each of them a
//     point where the multiplying wave has its operands for the next six MFMAs in registers already;
//   * the mid-phase barrier sits in front of group 5's MFMAs (whose operands were read before it) and in front of the first Ub read.
// Same arithmetic, same packed weights and same epilogue as the round-4 form.
constexpr int PH = 4, PR = PH + 2;
constexpr int TP_PLANE = PR * 2 * NP * 4;                 // dwords of one (piece, component) plane of a half tile
constexpr int TP_DWORDS = 12 * TP_PLANE;                  // 9 216 dwords = 36 KB
constexpr int GT = WT / 2;                                // threads of a group
constexpr int P_IN = (PR * NP * 8) / GT;                  // (row, pair, channel pair) items per thread and stage: 768 / 256 = 3
static_assert(PR * NP * 8 == P_IN * GT, "items must divide over the group");

PROF_BUFFER(w6p, 2048 * 8 * 8)
constexpr int SLOT0 = 21;    // MFMA slot behind which the staging arithmetic starts (72 slots, the program has 51): the fetch it
                             // consumes is issued half a phase earlier by group 1

// ISC: the launch carries style scales.  A template parameter, and the fetch of the staging role is unconditional (clamped to the last
// stage): with `if (iscb)` / `if (fetch)` around the loads the compiler kept two copies of the 26 fetch registers and moved them twice per
// staging phase - ~40 vector-ALU instructions in the wave whose instructions cost 10 - 27 cycles each (found in s2s6.hip's phase
// profile, profiles/experiments/r05_s2s6_phase_profile.log; the ISA of the staging role now has no register move at all).
// (Round 6, tried and NOT taken: a NARROW form for M == 32 - the 32 -> 32 layer at 1024^2 of the FFHQ-1024 generator - in which the block's
//  second 32-channel tile is padding, its weight slots are not fetched and the waves that own it skip MFMAs and stores.  Correct at the
//  5e-6 bar, but 1 121 us against the 769 us of the fp32 Winograd kernel wino3x3_kernel<32>: with K = 32 a block lives for two stages, one
//  block per CU (144 KB of LDS), so in this kernel - which has no tile walk, unlike wino6q_kernel - the prologue's HBM latency and the
//  epilogue are not overlapped by anything;
//  profiles/experiments/r06_g1024_kernel_stats_with_wino6p_narrow.txt, r06_wino6p_narrow.patch.)
template <bool ISC>
__global__ __launch_bounds__(WT, 2) void wino6p_kernel(const Wino6Args p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u32x4* ul = reinterpret_cast<u32x4*>(smem_raw);                                   // weights, 16-byte chunks
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave-uniform by construction: keep the role branches scalar
    const int grp = wid >> 2, wq = wid & 3, wm = wq >> 1, wrl = wq & 1, gt = tid & (GT - 1);
    unsigned* tl = reinterpret_cast<unsigned*>(smem_raw + U_CHUNKS * 16) + grp * TP_DWORDS;      // this group's half tile
    const u32x4* tl4 = reinterpret_cast<const u32x4*>(tl);
    int tile, mb;
    if (!split6_tile(p.ntiles, p.nt8, p.mblocks, tile, mb)) return;
    // W == 16 (round 6): a tile row holds TWO samples side by side - pairs 0-7 = sample b, pairs 8-15 = sample b + 1 (lgpw = 3); every
    // column pair is transformed from its own four input columns, so only the staging geometry and the output addresses know about it
    const int pwm = (1 << p.lgpw) - 1;
    const int tx = tile % p.tiles_x, ty = (tile / p.tiles_x) % p.tiles_y, b = (tile / (p.tiles_x * p.tiles_y)) << (4 - p.lgpw);
    const int x0 = tx * TW, y0 = ty * TH, yh = y0 + PH * grp;
    const float* inb = p.in + (size_t)b * p.K * p.H * p.W;
    const float* iscb = ISC ? p.isc + (size_t)b * p.K : nullptr;
    // block-uniform edge flags: interior tiles skip the patches of arith() by scalar branches (an empty asm statement inside each
    // branch keeps the compiler from turning them back into 96 selects per phase that every tile pays: a vector-ALU instruction in
    // the MFMA stream costs ~4.5 cycles, profiles/experiments/r05_wgrad6.log)
    const bool has_left = x0 == 0, has_right = x0 + TW >= p.W, has_rowout = (yh == 0) || (yh + PH == p.H);

    f32x16 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

    // staging geometry of this group's half: item e = gt + 256 i -> (pair jj = e % 16, channel pair q = (e / 16) % 8, row = e / 128)
    unsigned g_off[P_IN];          // (never negative: the left-border item is moved one column to the right)
    int l_off[P_IN], e_flag[P_IN];
#pragma unroll
    for (int i = 0; i < P_IN; ++i) {
        const int e = gt + GT * i;
        const int jj = e & 15, q = (e >> 4) & 7, row = e >> 7;
        const int gy = yh - 1 + row;
        const int sj = jj >> p.lgpw, jl = jj & pwm;                       // sample of the tile row, pair inside the sample's row
        const bool left = x0 == 0 && jl == 0, right = x0 + TW >= p.W && jl == pwm, rowout = gy < 0 || gy >= p.H;
        e_flag[i] = (left ? 1 : 0) | (right ? 2 : 0) | (rowout ? 4 : 0);
        const int gyc = gy < 0 ? 0 : (gy >= p.H ? p.H - 1 : gy);
        g_off[i] = (unsigned)(sj * p.K * p.H * p.W + (2 * q * p.H + gyc) * p.W + x0 + 2 * jl - 1 + (left ? 1 : 0) - (right ? 1 : 0));
        l_off[i] = ((row * 2 + (q >> 2)) * NP + jj) * 4 + (q & 3);                        // + (piece * 4 + c) * TP_PLANE
    }
    const unsigned q2 = 2u * ((gt >> 4) & 7) + (unsigned)(((gt & 15) >> p.lgpw) * p.K);      // (+ the style-scale row of this thread's sample:
                                                                                              //  a thread's items share their pair index)
    const size_t plane = (size_t)p.H * p.W;
    const int MT = p.M >> 5;
    f32x4 rin[P_IN][2];
    f32x2 rsc = {1.f, 1.f};        // style scales of this thread's channel pair (the same pair for its three items: 256 % 128 == 0)
    const int nstage = p.K / KC;
    // fetch of stage s, item by item (uniform base pointer + unsigned 32-bit per-thread offset: the scalar-base addressing form, no
    // 64-bit address registers).  Inside the loop the fetch is issued by the MULTIPLYING role, each item right behind the last slot of
    // the arithmetic that reads its registers: the fetch registers are then written and read in one role only.  Issued by the staging
    // role - as the first ping-pong versions did - they came out of the register allocator as two sets with 12 - 18 64-bit moves per
    // staging phase between them (and with them conditional on `fetch`, twice that), in the wave whose vector-ALU instructions cost
    // 10 - 27 cycles each; found in s2s6.hip's phase profile, profiles/experiments/r05_s2s6_phase_profile.log.
    auto fetch_scales = [&](int s) {
        if (ISC) rsc = *reinterpret_cast<const f32x2u*>(iscb + s * KC + q2);
    };
    auto fetch_item = [&](int i, int s) {
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
            rin[i][h2] = *reinterpret_cast<const f32x4u*>(inb + ((size_t)s * KC + h2) * plane + g_off[i]);
    };
    auto issue = [&](int s) {
        fetch_scales(s);
#pragma unroll
        for (int i = 0; i < P_IN; ++i) fetch_item(i, s);
    };
    // weight half `uh` of stage s: 36 fragment slots (3 pieces x 6 (tap row, component) groups x 2 M tiles), 9 per wave of the group
    auto issue_u = [&](int uh, int s) {
        const u32x4* us = p.U + (size_t)s * 36 * MT * 64;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const int j = wq * 9 + r, piece = j / 12, rem = j % 12, kc = (rem >> 1) + 6 * uh, mt = rem & 1;
            const int pk = piece * 12 + kc;                                   // == (piece * 3 + ky) * 4 + c
            const u32x4* g = us + ((size_t)pk * MT + 2 * mb + mt) * 64 + (unsigned)lane;      // uniform base + 32-bit lane offset
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                             (__attribute__((address_space(3))) void*)(ul + (pk * 2 + mt) * 64), 16, 0, 0);
        }
    };
    // ---- the arithmetic of staging (style scale, B^T d, three-piece split) as a PROGRAM OF 51 SLOTS that the multiplying wave runs
    // behind its own MFMAs (one slot per MFMA; all slot indices are compile-time after unrolling).  Measured with the first
    // ping-pong version (profiles/experiments/r05_w6p_phase_profile.log): the same ~50 vector-ALU instructions per item issued by the
    // PARTNER wave of a SIMD that streams MFMAs cost 10 (older wave) to 27 (younger wave) cycles apiece - more than the multiplying
    // phase lasts - while instructions of the multiplying wave itself issue in the shadow of its own MFMAs (32 cycles each).
    //   slots 0..2         : item k: edge patch, style scale (in place in rin)
    //   slots 3 + 4 u + j  : unit u = item * 4 + component, step j:  0: t = (B^T d)_c for the channel pair, h = bf16x2(t)
    //                        1: t -= h    2: m = bf16x2(t), unpack m    3: t -= m, l = bf16x2(t)
    // The results wait in `res` (36 registers) for the staging phase, which only moves them to LDS.
    unsigned res[P_IN][4][3];
    float te = 0.f, to = 0.f, fe = 0.f, fo = 0.f;
    constexpr int N_SLOT = 3 + 4 * 4 * P_IN;
    auto arith = [&](int k) {
        if (k < 0) {
        } else if (k < P_IN) {
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                f32x4 v = rin[k][h2];
                const int f = e_flag[k];
                if (has_left) {
                    asm volatile("" ::: "memory");
                    if (f & 1) { v[3] = v[2]; v[2] = v[1]; v[1] = v[0]; v[0] = 0.f; }        // loaded from column 0: element 0 is column -1
                }
                if (has_right) {
                    asm volatile("" ::: "memory");
                    if (f & 2) { v[0] = v[1]; v[1] = v[2]; v[2] = v[3]; v[3] = 0.f; }        // loaded one column early: element 3 is column W
                }
                if (has_rowout) {
                    asm volatile("" ::: "memory");
                    if (f & 4) { v[0] = 0.f; v[1] = 0.f; v[2] = 0.f; v[3] = 0.f; }
                }
                rin[k][h2] = ISC ? v * rsc[h2] : v;
                asm volatile("" : "+v"(rin[k][h2]));
            }
        } else if (k < N_SLOT) {
            const int u = (k - P_IN) >> 2, j = (k - P_IN) & 3, i = u >> 2, c = u & 3;
            float ve = 0.f, vo = 0.f;
            if (j == 0) {
                const f32x4 e = rin[i][0], o = rin[i][1];                         // even / odd channel of the pair
                ve = c == 0 ? e[0] - e[2] : (c == 1 ? e[1] + e[2] : (c == 2 ? e[2] - e[1] : e[1] - e[3]));
                vo = c == 0 ? o[0] - o[2] : (c == 1 ? o[1] + o[2] : (c == 2 ? o[2] - o[1] : o[1] - o[3]));
            }
            split6_step4(j, ve, vo, te, to, fe, fo, res[i][c][0], res[i][c][1], res[i][c][2]);
        }
    };
    auto write_res = [&]() {
#pragma unroll
        for (int i = 0; i < P_IN; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) tl[l_off[i] + (pc * 4 + c) * TP_PLANE] = res[i][c][pc];
    };
    const int rr = l31 >> 4, jj = l31 & 15;
    const int b_chunk = ((2 * wrl + rr) * 2 + half) * NP + jj;          // + ((piece * 4 + c) * PR + ky) * 2 * NP       (16-byte chunks)
    const int a_chunk = wm * 64 + lane;                                 // + ((piece * 3 + ky) * 4 + c) * 128

    // prologue: every group transforms and writes its half of stage 0 and fetches stage 1; group 0 brings in the whole weight image
    issue(0);
    if (grp == 0) { issue_u(0, 0); issue_u(1, 0); }
#pragma unroll
    for (int k = 0; k < N_SLOT; ++k) arith(k);
    write_res();
    issue(1);
    // (only the weight DMA has to have landed at the barrier: a COUNTED wait in group 0 leaves the fetch of stage 1 - 7 loads, 6 without
    //  style scales - in flight; waiting for it too cost every block one HBM latency, ~2 of the ~8 us a block spends outside its stages)
    if (grp == 0) {
        if (ISC) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    }
    split6_barrier();
    const int nphase = 2 * nstage;
    PROF_ONLY(unsigned long long pc[8] = {0, 0, 0, 0, 0, 0, 0, 0};)
    PROF_ONLY(const unsigned long long pstart = __builtin_readcyclecounter(), rstart = __builtin_amdgcn_s_memrealtime();)
    for (int ph = 0; ph < nphase; ++ph) {
        const bool last = ph == nphase - 1;
        PROF_T(t0);
        if ((ph & 1) == grp) {
            // ---- multiply this group's half of stage ph / 2; behind the MFMAs: the arithmetic of stage ph / 2 + 1 (rin -> res)
            // (in a group's last multiplying phase the arithmetic runs on the stale registers of the last fetch and its results are never
            //  written: ONE copy of the MFMA stream instead of two with their own register allocation and 64 moves between them)
            bf16x8 av[2][3], bv[2][3];
            const int fs2 = min((ph >> 1) + 2, nstage - 1);
            auto rd1 = [&](int g, int slot, int q) {
                const int ky = g >> 2, c = g & 3;
                if (q < 3) av[slot][q] = __builtin_bit_cast(bf16x8, ul[a_chunk + ((q * 3 + ky) * 4 + c) * 128]);
                else bv[slot][q - 3] = __builtin_bit_cast(bf16x8, tl4[b_chunk + (((q - 3) * 4 + c) * PR + ky) * 2 * NP]);
            };
#pragma unroll
            for (int q = 0; q < 6; ++q) rd1(0, 0, q);
            // a wave raises its priority while it multiplies (+1 - 1.5 % over none; a static priority for group 1 instead: -3 %)
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int g = 0; g < 12; ++g) {
                const int slot = g & 1, c = g & 3;
                // mid-phase barrier (every phase, the last one too: no branch in the MFMA stream)
                if (g == 5) { PROF_T(ta); split6_barrier(); PROF_T(tb); PROF_ACC(pc[0], t0, ta); PROF_ACC(pc[1], ta, tb); PROF_ONLY(pc[2] -= tb;) }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    split6_product(q, av[slot], bv[slot], acc[c], acc[c]);
                    if (g + 1 < 12 && q < 3) { rd1(g + 1, slot ^ 1, 2 * q); rd1(g + 1, slot ^ 1, 2 * q + 1); }
                    arith(g * 6 + q - SLOT0);
                    {   // the fetch of the stage after next, item by item behind the last slot that reads the item's registers
                        constexpr int LASTQ = 71 - SLOT0;                      // slot of the last MFMA
                        const int k = g * 6 + q - SLOT0;
                        if (k == P_IN - 1) fetch_scales(fs2);
#pragma unroll
                        for (int i = 0; i < P_IN; ++i)
                            if (k == (P_IN + 16 * i + 12 < LASTQ ? P_IN + 16 * i + 12 : LASTQ)) fetch_item(i, fs2);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __builtin_amdgcn_s_setprio(0);
            PROF_ONLY({ asm volatile("s_nop 0" ::: "memory"); PROF_T(tc); pc[2] += tc; })
        } else {
            // ---- stage: move this group's half of stage cs = (ph + 1) / 2 to LDS, fetch stage cs + 1, renew a half of the weight image
            const int cs = (ph + 1) >> 1;
            const bool work = cs >= 1 && cs < nstage;
            // group 1 renews Ub in front of the mid-phase barrier (the partner reads it right behind): DMA first, the LDS writes of
            // this half tile in its shadow, then the wait for the DMA; group 0 renews Ua behind the barrier.  (The fetch of the next
            // stage is not issued here any more: see fetch_item.)  The LDS writes are unconditional: in group 1's first phase they
            // repeat what the prologue wrote, in group 0's last phase they put stale results in a tile nobody reads any more.
            if (grp == 1 && work) issue_u(1, cs);
            __builtin_amdgcn_sched_barrier(0);
            write_res();
            if (grp == 1 && work) split6_wait_vm();
            PROF_T(ta);
            split6_barrier();
            PROF_T(tb);
            if (grp == 0 && work) {
                issue_u(0, cs);
                split6_wait_vm();
            }
            PROF_T(tc);
            PROF_ACC(pc[3], t0, ta); PROF_ACC(pc[4], ta, tb); PROF_ACC(pc[5], tb, tc);
        }
        PROF_T(t8);
        if (!last) split6_barrier();
        PROF_T(t9);
        PROF_ACC(pc[6], t8, t9);
    }
    PROF_ONLY(if (lane == 0 && blockIdx.x < 2048) {
        unsigned long long* d = te_w6p_prof_buf + ((size_t)blockIdx.x * 8 + wid) * 8;
        _Pragma("unroll")
        for (int i = 0; i < 6; ++i) d[i] = pc[i];
        d[6] = pc[6] | ((__builtin_amdgcn_s_memrealtime() - rstart) << 40);          // (100 MHz counter: the shader clock follows)
        d[7] = ((unsigned long long)nstage << 48) | ((__builtin_readcyclecounter() - pstart) & 0xFFFFFFFFFFFFull);
    })
    // epilogue: as wino.hip (output transform, demodulation scale, bias, leaky ReLU, residual, mask); group 0 is here one phase early
    const int wr = grp * 2 + wrl;
    const int mbase = mb * BM + wm * 32;
    const int bo = b + (jj >> p.lgpw);                                  // this lane's output sample
    const size_t off0 = ((size_t)bo * p.M + mbase) * plane + (size_t)(y0 + 2 * wr + rr) * p.W + x0 + 2 * (jj & pwm);
    const float g_pos = p.act == 3 ? 1.4142135623730951f : 1.f;
    float scv[16], biv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = mbase + (r & 3) + 8 * (r >> 2) + 4 * half;
        scv[r] = p.osc ? p.osc[(size_t)bo * p.M + m] : 1.f;
        biv[r] = p.bias ? p.bias[m] : 0.f;
    }
    f32x2 resv[16], mrefv[16];
    if (p.res) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            resv[r] = *reinterpret_cast<const f32x2*>(p.res + off0 + (size_t)((r & 3) + 8 * (r >> 2) + 4 * half) * plane);
    }
    if (p.mref) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            mrefv[r] = *reinterpret_cast<const f32x2*>(p.mref + off0 + (size_t)((r & 3) + 8 * (r >> 2) + 4 * half) * plane);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int dm = (r & 3) + 8 * (r >> 2) + 4 * half;
        float v0 = acc[0][r] + acc[1][r] + acc[2][r];
        float v1 = acc[1][r] - acc[2][r] - acc[3][r];
        const float sc = scv[r], bi = biv[r];
        v0 = v0 * sc + bi;
        v1 = v1 * sc + bi;
        if (p.act >= 3) {
            v0 = (v0 > 0.f ? v0 : v0 * 0.2f) * g_pos;
            v1 = (v1 > 0.f ? v1 : v1 * 0.2f) * g_pos;
        }
        const size_t o = off0 + (size_t)dm * plane;
        if (p.res) { v0 += resv[r][0]; v1 += resv[r][1]; }
        if (p.mref) {
            v0 *= mrefv[r][0] > 0.f ? p.mgain : 0.2f * p.mgain;
            v1 *= mrefv[r][1] > 0.f ? p.mgain : 0.2f * p.mgain;
        }
        f32x2 v; v[0] = v0; v[1] = v1;
        *reinterpret_cast<f32x2*>(p.out + o) = v;
    }
}


// ---------------------------------------------------------------------------------------------------------------------------------
// Round 6: TWO 64-channel weight images per staged half tile (wino6q_kernel, form 2, taken when M % 128 == 0).
//
// What the round-6 power / clock telemetry says about wino6p_kernel (profiles/r06_power_clock_*.txt, 3-second loops, 1 400 W cap): the
// product kernel sits AT the cap (1 364 - 1 389 W, PPT residency 60 - 75 % of the samples) at 1.99 - 2.04 GHz; with the staging arithmetic
// and its LDS writes compiled out the same MFMA stream runs 21 - 26 % faster at the same power (0.96 - 1.10 pJ per executed FLOP against
// 1.23 - 1.40), and the staging alone (MFMAs compiled out) needs MORE shader cycles than the MFMAs alone (2.16 M against 1.92 M kilocycles
// at 128 -> 128 @256^2).  The block tile of wino6p is 64 output channels, so the style scale, B^T d and the three-piece split of every
// input element are re-done by every M block: twice at 128 channels, four times at 256, eight times at 512.  Here a block owns 128
// output channels: each half tile T_g(s) is staged ONCE and multiplied by the two weight images (s, m = 0) and (s, m = 1) in two
// multiplying phases with their own accumulators (2 x 64 registers) - half the staging instructions, LDS writes and fetches per MFMA, same LDS
// budget (one 72 KB weight image, two 36 KB half tiles), same weight-image hand-over protocol with the "stage" index replaced by the
// image index j = 2 s + m:
//     phase p (0 .. 4 nstage - 1): group p & 1 multiplies with image j = p >> 1; the other group is in its staging role
//     group 0:            M0(s)  SA  M1(s)  SB          group 1:   S  M0(s)  SA  M1(s)  SB   (one phase behind)
//     M0: 72 MFMAs + the fetch of stage s + 1 (consumed one multiplying phase later)    SA: weight DMA only
//     M1: 72 MFMAs + the staging arithmetic (rin -> res) behind them                       SB: weight DMA + res -> T_g(s + 1)
// Both groups run the SAME straight-line loop body (M0 SA M1 SB), group 1 one staging phase late: no role branch around the MFMA streams, two
// copies of the stream (one per accumulator set).  Same products in the same order per output element as wino6p: bit-identical.
//
// THE TILE WALK.  One block owns a CU (144 KB of LDS), and outside its channel stages the matrix pipe of that CU idles: a launch whose
// blocks live for 8 stages (K = 128) spent 14.7 % of its time there, one with 32 stages 4.1 % (tools/block_overhead_probe.py,
// profiles/experiments/r05_w6p_phase_profile.log step 5).  A block therefore takes a RUN of consecutive tiles of its XCD with one M block
// (split6_tile_list: the order split6_tile defines, so neighbours keep sharing halo rows in one L2) and carries the pipeline across them:
//   * at a tile's last stage the fetch of the M0 phase - which used to fetch the last stage a second time and drop it - fetches stage 0
//     of the NEXT tile (the staging geometry, one set of registers, is switched to the next tile in front of that phase: its last user
//     was the M1 phase before); the M1 phase splits it, the SB phase writes the next tile's T_g(0) (group 1 runs its last SB then);
//   * the weight hand-over simply goes on: the image behind the tile's last one is image 0 again (same M block), Ua renewed by group 0
//     in its last SB, Ub by group 1 in its last SB, beside which group 0 only executes the phase's two barriers;
//   * between two tiles stands the epilogue alone, OUTSIDE the phase loop, with pointers and geometry live beside the accumulators, which
//     are zeroed behind it.  Its stores drain under the next tile's stages.  A run's last tile ends, its first tile begins as before.
// The phase body exists once.  The schedule - who multiplies, who stages, which weight half is renewed, the barriers - is written down in
// wino6_schedule.h, from which this kernel takes every such decision and which tests/test_wino6_schedule.py replays on the host: equal
// barrier counts of the two groups for every run length are checked THERE, not by a GPU run.  (The fully persistent form of round 5 put
// the epilogue inside the phase loop: 256 VGPRs, 51 - 60 spilled, 1.4 - 1.7x slower; profiles/experiments/r05_w6p_phase_profile.log.)
// To fit beside what the next tile keeps live, the epilogue addresses through a block-uniform base per channel plus one 32-bit lane
// offset and handles four of a lane's sixteen rows at a time.
template <bool ISC>
__global__ __launch_bounds__(WT, 2) void wino6q_kernel(const Wino6Args p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u32x4* ul = reinterpret_cast<u32x4*>(smem_raw);                                   // weights, 16-byte chunks
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wid >> 2, wq = wid & 3, wm = wq >> 1, wrl = wq & 1, gt = tid & (GT - 1);
    unsigned* tl = reinterpret_cast<unsigned*>(smem_raw + U_CHUNKS * 16) + grp * TP_DWORDS;      // this group's half tile
    const u32x4* tl4 = reinterpret_cast<const u32x4*>(tl);
    int tile, tile_end, tile_step, mbq;               // (mblocks = M / 128 for this form)
    if (!split6_tile_list(p.ntiles, p.nt8, p.mblocks, p.lists, tile, tile_end, tile_step, mbq)) return;
    // staging geometry of ONE tile: the current one, and from the top of a tile's last stage on (whose M0 phase fetches stage 0 of the
    // next tile) the next one - set_tile.  Block-uniform parts are scalars; the epilogue decodes `tile` again for its own addresses.
    const float* inb;
    const float* iscb = nullptr;
    bool has_left, has_right, has_rowout;

    f32x16 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][c][r] = 0.f;

    unsigned g_off[P_IN];
    int l_off[P_IN], e_flag[P_IN];
    // What only the switch to a tile (set_tile) and the epilogue need of the launch arguments - pointers, image and tile-grid sizes - is
    // read there from the kernel-argument segment (scalar loads that hit the constant cache), through a pointer the compiler cannot see
    // through: held in scalar registers from the kernel's entry they do not fit beside what the phase loop keeps, and spill to lanes.
    typedef const __attribute__((address_space(4))) Wino6Args* KArgs;
    auto kargs = [&]() {
        KArgs k = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();                                  // (the kernel's only argument: offset 0)
        asm volatile("" : "+s"(k));
        return k;
    };
    auto set_tile = [&](int t) {
        const KArgs a = kargs();
        const int aH = a->H, aW = a->W, atx = a->tiles_x, aty = a->tiles_y, aK = a->K;
        const int tx = t % atx, ty = (t / atx) % aty, b = t / (atx * aty);
        const int x0 = tx * TW, yh = ty * TH + PH * grp;
        inb = a->in + (size_t)b * aK * aH * aW;
        if (ISC) iscb = a->isc + (size_t)b * aK;
        has_left = x0 == 0; has_right = x0 + TW == aW; has_rowout = (yh == 0) || (yh + PH == aH);
        // (opaque, as the epilogue's lane index: the tile-independent parts of the offsets are recomputed per tile, not kept - and spilled -
        //  across the phase loop)
        int gto = gt;
        asm volatile("" : "+v"(gto));
#pragma unroll
        for (int i = 0; i < P_IN; ++i) {
            const int e = gto + GT * i;
            const int jj = e & 15, q = (e >> 4) & 7, row = e >> 7;
            const int gy = yh - 1 + row;
            const bool left = x0 == 0 && jj == 0, right = x0 + TW == aW && jj == NP - 1, rowout = gy < 0 || gy >= aH;
            e_flag[i] = (left ? 1 : 0) | (right ? 2 : 0) | (rowout ? 4 : 0);
            const int gyc = gy < 0 ? 0 : (gy >= aH ? aH - 1 : gy);
            g_off[i] = (unsigned)((2 * q * aH + gyc) * aW + x0 + 2 * jj - 1 + (left ? 1 : 0) - (right ? 1 : 0));
        }
    };
    set_tile(tile);
#pragma unroll
    for (int i = 0; i < P_IN; ++i) {
        const int e = gt + GT * i;
        const int jj = e & 15, q = (e >> 4) & 7, row = e >> 7;
        l_off[i] = ((row * 2 + (q >> 2)) * NP + jj) * 4 + (q & 3);                        // + (piece * 4 + c) * TP_PLANE
    }
    const unsigned q2 = 2u * ((gt >> 4) & 7);
    const size_t plane = (size_t)p.H * p.W;
    const int MT = p.M >> 5;
    f32x4 rin[P_IN][2];
    f32x2 rsc = {1.f, 1.f};
    const int nstage = p.K / KC, nimg = 2 * nstage;
    auto fetch_scales = [&](int s) {
        if (ISC) rsc = *reinterpret_cast<const f32x2u*>(iscb + s * KC + q2);
    };
    auto fetch_item = [&](int i, int s) {
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
            rin[i][h2] = *reinterpret_cast<const f32x4u*>(inb + ((size_t)s * KC + h2) * plane + g_off[i]);
    };
    // weight half `uh` of image j = 2 s + m: 36 fragment slots (3 pieces x 6 (tap row, component) groups x 2 M tiles), 9 per wave: wave wq
    // takes slots 3 wq .. 3 wq + 2 of the twelve of EVERY piece, so that a slot's global and LDS addresses are one of three wave-dependent
    // bases plus a compile-time multiple of the piece stride.  The wave index is made opaque per call: with wino6p_kernel's assignment
    // (nine consecutive slots, piece and slot by division) the eighteen 64-bit slot offsets were hoisted out of the phase loop and, beside
    // the tile walk's scalars, spilled to lanes.
    auto issue_u = [&](int uh, int j) {
        int wqo = wq;
        asm volatile("" : "+s"(wqo));
        const u32x4* us = p.U + ((size_t)(j >> 1) * 36 * MT + 2 * (2 * mbq + (j & 1))) * 64;
        const unsigned pstride = 12u * (unsigned)MT * 64u;                     // chunks from piece to piece
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int rem = wqo * 3 + t, kc = (rem >> 1) + 6 * uh, mt = rem & 1;
            const u32x4* g0 = us + (unsigned)(kc * MT + mt) * 64u;              // uniform base of slot (piece 0, kc, mt)
            u32x4* l0 = ul + (kc * 2 + mt) * 64;
#pragma unroll
            for (int piece = 0; piece < 3; ++piece) {
                const u32x4* g = g0 + piece * pstride + (unsigned)lane;         // uniform base + 32-bit lane offset
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                                 (__attribute__((address_space(3))) void*)(l0 + piece * 24 * 64), 16, 0, 0);
            }
        }
    };
    // the staging arithmetic as a program of 51 slots (wino6p_kernel: arith), run behind the MFMAs of the m = 1 phase
    unsigned res[P_IN][4][3];
    float te = 0.f, to = 0.f, fe = 0.f, fo = 0.f;
    constexpr int N_SLOT = 3 + 4 * 4 * P_IN;
    auto arith = [&](int k) {
        if (k < 0) {
        } else if (k < P_IN) {
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                f32x4 v = rin[k][h2];
                // (the flag is made opaque INSIDE each branch: otherwise the nine lane masks (f & bit) != 0 are hoisted out of the loop
                //  as 18 scalar registers, which - with two accumulator sets - spill to v_writelane / v_readlane pairs in the MFMA stream)
                if (has_left) {
                    int f = e_flag[k];
                    asm volatile("" : "+v"(f) :: "memory");
                    if (f & 1) { v[3] = v[2]; v[2] = v[1]; v[1] = v[0]; v[0] = 0.f; }
                }
                if (has_right) {
                    int f = e_flag[k];
                    asm volatile("" : "+v"(f) :: "memory");
                    if (f & 2) { v[0] = v[1]; v[1] = v[2]; v[2] = v[3]; v[3] = 0.f; }
                }
                if (has_rowout) {
                    int f = e_flag[k];
                    asm volatile("" : "+v"(f) :: "memory");
                    if (f & 4) { v[0] = 0.f; v[1] = 0.f; v[2] = 0.f; v[3] = 0.f; }
                }
                rin[k][h2] = ISC ? v * rsc[h2] : v;
                asm volatile("" : "+v"(rin[k][h2]));
            }
        } else if (k < N_SLOT) {
            const int u = (k - P_IN) >> 2, j = (k - P_IN) & 3, i = u >> 2, c = u & 3;
            float ve = 0.f, vo = 0.f;
            if (j == 0) {
                const f32x4 e = rin[i][0], o = rin[i][1];
                ve = c == 0 ? e[0] - e[2] : (c == 1 ? e[1] + e[2] : (c == 2 ? e[2] - e[1] : e[1] - e[3]));
                vo = c == 0 ? o[0] - o[2] : (c == 1 ? o[1] + o[2] : (c == 2 ? o[2] - o[1] : o[1] - o[3]));
            }
            split6_step4(j, ve, vo, te, to, fe, fo, res[i][c][0], res[i][c][1], res[i][c][2]);
        }
    };
    auto write_res = [&]() {
#pragma unroll
        for (int i = 0; i < P_IN; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) tl[l_off[i] + (pc * 4 + c) * TP_PLANE] = res[i][c][pc];
    };
    const int rr = l31 >> 4, jj = l31 & 15;
    const int b_chunk = ((2 * wrl + rr) * 2 + half) * NP + jj;
    const int a_chunk = wm * 64 + lane;

    // one multiplying phase with accumulator set MSET; behind the MFMAs: MSET 0 the fetch of stage `fs`, MSET 1 the staging arithmetic
    // (wino6_sched::replay restates this phase as events - reads of the first weight half and the half tile, the mid barrier, reads of
    //  the second half, the end barrier: a barrier or a first read of either weight half moved here must move THERE in the same change)
    auto multiply = [&](auto mset_tag, int fs) {
        constexpr int MSET = decltype(mset_tag)::value;
        bf16x8 av[2][3], bv[2][3];
        auto rd1 = [&](int g, int slot, int q) {
            const int ky = g >> 2, c = g & 3;
            if (q < 3) av[slot][q] = __builtin_bit_cast(bf16x8, ul[a_chunk + ((q * 3 + ky) * 4 + c) * 128]);
            else bv[slot][q - 3] = __builtin_bit_cast(bf16x8, tl4[b_chunk + (((q - 3) * 4 + c) * PR + ky) * 2 * NP]);
        };
#pragma unroll
        for (int q = 0; q < 6; ++q) rd1(0, 0, q);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int g = 0; g < 12; ++g) {
            const int slot = g & 1, c = g & 3;
            if (g == 5) split6_barrier();             // mid-phase barrier
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                split6_product(q, av[slot], bv[slot], acc[MSET][c], acc[MSET][c]);
                if (g + 1 < 12 && q < 3) { rd1(g + 1, slot ^ 1, 2 * q); rd1(g + 1, slot ^ 1, 2 * q + 1); }
                const int k = g * 6 + q;
                if (MSET == 0) {
                    // the fetch of the next stage, an item every twelve slots from the sixth on (rin is free: the m = 1 phase consumed it)
                    if (k == 5) fetch_scales(fs);
#pragma unroll
                    for (int i = 0; i < P_IN; ++i)
                        if (k == 6 + 12 * i) fetch_item(i, fs);
                } else {
                    arith(k - SLOT0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        split6_barrier();                             // end of phase
    };
    // one phase in the staging role.  ph = phase index inside the tile; image cs = (ph + 1) >> 1 is the one whose half this phase renews
    // (cs == nimg: image 0 of the next tile, where the list has one): group 1 (even ph) renews Ub(cs) in FRONT of the mid-phase barrier
    // (its partner reads it right behind), group 0 (odd ph) renews Ua(cs) BEHIND it (the partner is past the last read of Ua(cs - 1)
    // there).  WRITE: this is the phase behind the group's m = 1 multiply: the parked results go to the half tile (nobody reads it until
    // the group's next m = 0 phase).  (wino6_sched::replay's `stage` restates this order - DMA, write, wait, barrier, DMA, wait, barrier -
    // and must be changed in the same change as this lambda: the host test sees the kernel only through it.)
    auto stage = [&](int ph, bool write, bool has_next) {
        const int cs = wino6_sched::renew_image(ph);
        const bool work = wino6_sched::renew_work(cs, nimg, has_next);
        const int ci = cs == nimg ? 0 : cs;
        if (grp == 1 && work) issue_u(1, ci);
        __builtin_amdgcn_sched_barrier(0);
        if (write) write_res();
        if (grp == 1 && work) split6_wait_vm();
        split6_barrier();                             // mid-phase
        if (grp == 0 && work) {
            issue_u(0, ci);
            split6_wait_vm();
        }
        split6_barrier();                             // end of phase
    };

    // prologue: every group transforms and writes its half of stage 0; group 0 brings in the whole weight image 0
    fetch_scales(0);
#pragma unroll
    for (int i = 0; i < P_IN; ++i) fetch_item(i, 0);
    if (grp == 0) { issue_u(0, 0); issue_u(1, 0); }
#pragma unroll
    for (int k = 0; k < N_SLOT; ++k) arith(k);
    write_res();
    split6_wait_vm();
    split6_barrier();
    // the tile walk (wino6_schedule.h holds the schedule; tests/test_wino6_schedule.py replays it).  ONE phase loop for every tile of the
    // list; between two tiles only the epilogue, with nothing but pointers and geometry live beside the accumulators.
    for (;;) {
        const bool has_next = tile + tile_step < tile_end;
        int ph = 0;
        if (wino6_sched::lead_phase(grp)) { stage(0, false, has_next); ph = 1; }
        for (int s = 0; s < nstage; ++s) {
            bool next_tile;
            const int fs = wino6_sched::fetch_stage(s, nstage, has_next, next_tile);
            if (next_tile) set_tile(tile + tile_step);      // (rin, res and the old geometry are dead here: M1 of stage s - 1 used them last)
            multiply(std::integral_constant<int, 0>{}, fs);
            stage(ph + 1, false, has_next);
            multiply(std::integral_constant<int, 1>{}, fs);
            if (wino6_sched::runs_sb(grp, s, nstage, has_next)) stage(ph + 3, true, has_next);
            ph += 4;
        }
        for (int i = 0; i < wino6_sched::tail_barriers(grp, has_next); ++i) split6_barrier();

        // epilogue: as wino6p_kernel, once per accumulator set
        const KArgs e = kargs();
        const int tx = tile % e->tiles_x, ty = (tile / e->tiles_x) % e->tiles_y, b = tile / (e->tiles_x * e->tiles_y);
        const int x0 = tx * TW, y0 = ty * TH;
        // (the lane index is made opaque for every tile: everything per-lane the epilogue derives from it - output offsets, the bias values -
        //  would otherwise be hoisted out of the tile loop and stay live, in ~100 registers, through the phase loop)
        int elane = lane;
        asm volatile("" : "+v"(elane));
        const int ehalf = elane >> 5, err = (elane & 31) >> 4, ejj = elane & 15;
        const int wr = grp * 2 + wrl;
        // (the plane size too is taken from there: of `plane` the 32 block-uniform channel offsets (channel x plane, 64 bits each) are
        //  computed once in front of the tile loop and kept, spilled to lanes, through it)
        const int eM = e->M, eW = e->W, eact = e->act;
        const size_t eplane = (size_t)e->H * eW;
        const float emgain = e->mgain;
        const float g_pos = eact == 3 ? 1.4142135623730951f : 1.f;
        float* const eout = e->out;
        const float* const eosc = e->osc; const float* const ebias = e->bias; const float* const eres = e->res; const float* const emref = e->mref;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int mbase = (2 * mbq + m) * BM + wm * 32;
            // addresses = a block-uniform base per output channel (scalar registers) + ONE 32-bit per-lane offset, fetch_item's form: the
            // 64-bit per-lane addresses of 48 loads and stores do not fit beside the accumulators and what the next tile keeps live
            const size_t off0 = ((size_t)b * eM + mbase) * eplane + (size_t)(y0 + 2 * wr) * eW + x0;
            const unsigned lo = (unsigned)(err * eW + 2 * ejj) + 4u * (unsigned)ehalf * (unsigned)eplane;
            // (four of the sixteen rows at a time: scales, biases, residuals and mask references of all sixteen are 96 registers)
#pragma unroll
            for (int r0 = 0; r0 < 16; r0 += 4) {
                float scv[4], biv[4];
#pragma unroll
                for (int r = r0; r < r0 + 4; ++r) {
                    const int mm = mbase + (r & 3) + 8 * (r >> 2) + 4 * ehalf;
                    scv[r - r0] = eosc ? eosc[(size_t)b * eM + mm] : 1.f;
                    biv[r - r0] = ebias ? ebias[mm] : 0.f;
                }
                f32x2 resv[4], mrefv[4];
                if (eres) {
#pragma unroll
                    for (int r = r0; r < r0 + 4; ++r)
                        resv[r - r0] = *reinterpret_cast<const f32x2*>(eres + off0 + (size_t)((r & 3) + 8 * (r >> 2)) * eplane + lo);
                }
                if (emref) {
#pragma unroll
                    for (int r = r0; r < r0 + 4; ++r)
                        mrefv[r - r0] = *reinterpret_cast<const f32x2*>(emref + off0 + (size_t)((r & 3) + 8 * (r >> 2)) * eplane + lo);
                }
#pragma unroll
                for (int r = r0; r < r0 + 4; ++r) {
                    float v0 = acc[m][0][r] + acc[m][1][r] + acc[m][2][r];
                    float v1 = acc[m][1][r] - acc[m][2][r] - acc[m][3][r];
                    const float sc = scv[r - r0], bi = biv[r - r0];
                    v0 = v0 * sc + bi;
                    v1 = v1 * sc + bi;
                    if (eact >= 3) {
                        v0 = (v0 > 0.f ? v0 : v0 * 0.2f) * g_pos;
                        v1 = (v1 > 0.f ? v1 : v1 * 0.2f) * g_pos;
                    }
                    if (eres) { v0 += resv[r - r0][0]; v1 += resv[r - r0][1]; }
                    if (emref) {
                        v0 *= mrefv[r - r0][0] > 0.f ? emgain : 0.2f * emgain;
                        v1 *= mrefv[r - r0][1] > 0.f ? emgain : 0.2f * emgain;
                    }
                    f32x2 v; v[0] = v0; v[1] = v1;
                    *reinterpret_cast<f32x2*>(eout + off0 + (size_t)((r & 3) + 8 * (r >> 2)) * eplane + lo) = v;
                }
            }
        }
        if (!has_next) break;
        tile += tile_step;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][c][r] = 0.f;
    }
}

}  // namespace

// kernel form of TE_CONV_3X3W6, a test and tool hook (te_hip.h): 1 = ping-pong (wino6p_kernel, round 5); 2 (round 6, default) = the
// two-image form wino6q_kernel where M % 128 == 0 and the grid still gives every CU a block (it has half as many blocks as the ping-pong
// form: measured slower on small grids, e.g. 39 against 22 us at 3 x 64 -> 256 @16x64), the ping-pong form elsewhere; 3 = the two-image
// form wherever M % 128 == 0 (tests).  All forms give the same results bit for bit (same products, same accumulation order per output
// element).
static std::atomic<int> g_w6_form{2};
extern "C" int te_conv_wino6_form(int form) {
    const int old = g_w6_form.load(std::memory_order_relaxed);
    if (form >= 1 && form <= 3) g_w6_form.store(form, std::memory_order_relaxed);
    return old;
}

// tiles per block of wino6q_kernel, a test and tool hook (te_hip.h): 0 = automatic (te_wino6_launch), 1 = one tile per block, n >= 2 =
// lists of at most n tiles.  Results are bit-identical across its values.
constexpr int W6_MAX_TPB = 4096;
static std::atomic<int> g_w6_tpb{0};
extern "C" int te_conv_wino6_tiles_per_block(int n) {
    const int old = g_w6_tpb.load(std::memory_order_relaxed);
    if (n >= 0 && n <= W6_MAX_TPB) g_w6_tpb.store(n, std::memory_order_relaxed);
    return old;
}

// automatic choice: runs of at most FOUR tiles, fewer where four would leave CUs without a block, one tile per block where even two would.
// Measured per launch with style scales, us, 20 launches per sample, fastest / slowest of 10 samples in two alternating visits per build on
// one machine (profiles/r07_w6_tile_walk_launch.jsonl; "before" = the kernel before the tile walk, n = tiles per block):
//     shape (K -> M @ H^2, batch)   before          n = 1           n = 2           n = 3           n = 4 (= automatic here)
//     128 -> 128 @ 256^2, 16        1191 / 1243     1096 / 1123     1104 / 1119     1181 / 1186     1100 / 1106
//     128 -> 128 @ 256^2, 32        2399 / 2440     2220 / 2244     2198 / 2214     2228 / 2251     2182 / 2202
//     256 -> 256 @ 128^2, 16        1104 / 1120     1036 / 1053     1020 / 1037     1078 / 1094     1020 / 1036
//     256 -> 256 @ 128^2, 32        2210 / 2240     2081 / 2105     2050 / 2063     2210 / 2225     2048 / 2062
//     512 -> 512 @ 64^2,  16        1060 / 1092      994 / 1015      992 / 1011     1298 / 1300      989 / 1010
//     512 -> 512 @ 64^2,  32        2145 / 2171     2004 / 2028     2018 / 2037     2141 / 2195     2014 / 2028
// (n = 1 against "before" is the epilogue's new addressing and its four-row batches: most of the gain; the walk itself adds 1 - 2 % at
// 256 channels and at 128 channels at batch 32, and nothing at 512, where a block lives for 32 stages.)  n = 3 shows what the second condition below is for: its
// runs do not divide the XCD's tiles into whole rounds over the CUs (352 blocks of three tile times against 256 of four at 512 -> 512 @64^2).
// A resident walk - one block per CU walking its whole share - was measured on an earlier state of this kernel and lost 1 - 3 % against
// n = 4 at the 256^2 shapes: the hardware hands a free CU the next run, and blocks drift apart instead of storing in lock step.
static int w6_auto_tpb(int nt8c, int mblocks) {
    // (a run of n tiles occupies its CU n tile times: where the blocks of the walk need more tile times in all - rounds over the CUs times n -
    //  than one-tile blocks need rounds, the coarser grain loses more at the launch's tail than the walk wins inside a block)
    const int64_t rounds1 = te::cdiv((int64_t)8 * nt8c * mblocks, te::kNumCU);
    for (int n = 4; n >= 2; --n) {
        const int64_t blocks = (int64_t)8 * te::cdiv(nt8c, n) * mblocks;
        if (blocks >= te::kNumCU && te::cdiv(blocks, te::kNumCU) * n <= rounds1) return n;
    }
    return 1;
}

PROF_READBACK(w6p)

extern "C" int te_conv_wino6_supported(int B, int K, int M, int H, int W) {
    if (!(B > 0 && K >= 32 && K % 32 == 0 && M >= BM && M % BM == 0 && H >= TH && H % TH == 0)) return 0;
    // W % 32 == 0, or (round 6) W == 16 with an even batch: two samples side by side in a 32-column tile row - the 16 x 16 layers of both
    // networks (512 channels: 32 stages per block) leave the fp32 pipe; 8 x 8 and 4 x 4 images give too few blocks and stay there
    const bool wide = W >= TW && W % TW == 0, pair16 = W == 16 && B % 2 == 0;
    if (!wide && !pair16) return 0;
    const int64_t tiles = wide ? (int64_t)B * (H / TH) * (W / TW) : (int64_t)(B / 2) * (H / TH);
    // (16-column images: only from half a block per CU up - measured at 512 -> 512 @16x16: 163 against 357 us at batch 32, 123 against 166 at
    //  batch 16, but 111 against 92 at batch 8, where the direct kernel's split over K fills the chip better than 64 blocks do)
    if (!wide && tiles * (M / BM) < te::kNumCU / 2) return 0;
    return ((int64_t)K * H * W * 4 * (wide ? 1 : 2) < 0x7FFFFFFF && tiles * (M / BM) < 0x7FFFFFF0) ? 1 : 0;
}

// The planning half of te_wino6_launch: everything of the launch that does not touch the device.  Fills the geometry of `a` and the plan `f`;
// the launch dispatches on `f` and on nothing else, te_wino6_split_form reports it.
static int wino6_plan(Wino6Args& a, Split6Form& f, int B, int K, int M, int H, int W) {
    TE_REQUIRE(te_conv_wino6_supported(B, K, M, H, W), TE_ERR_UNSUPPORTED,
               "te_conv_f32(TE_CONV_3X3W6): needs K %% 32 == 0, M %% 64 == 0, W %% 32 == 0 (or W == 16 and an even batch), H %% 8 == 0 (te_conv_wino6_supported)");
    a.B = B; a.K = K; a.M = M; a.H = H; a.W = W;
    a.lgpw = W >= TW ? 4 : 3;
    a.tiles_x = W >= TW ? W / TW : 1; a.tiles_y = H / TH; a.mblocks = M / BM;
    a.ntiles = (W >= TW ? B : B / 2) * a.tiles_x * a.tiles_y;
    a.nt8 = te::xcd_banded() ? (int)te::cdiv(a.ntiles, 8) : 0;
    int64_t blocks = te::cdiv(a.ntiles, 8) * 8 * a.mblocks;
    const int form = g_w6_form.load(std::memory_order_relaxed);
    const int64_t blocks_q = te::cdiv(a.ntiles, 8) * 8 * (M / (2 * BM));
    f = Split6Form{};
    f.pair16 = W < TW;
    if (W >= TW && split6_two_image(form - 1, M, blocks_q)) {     // (forms 2 / 3 of te_conv_wino6_form; W == 16: the ping-pong kernel only)
        f.two_image = 1;
        a.mblocks = M / (2 * BM);
        // the tile walk: a block takes a run of consecutive tiles of its XCD and carries the pipeline across them (wino6q_kernel).
        const int nt8c = (int)te::cdiv(a.ntiles, 8);                   // tiles of the fullest XCD
        int tpb = g_w6_tpb.load(std::memory_order_relaxed);
        if (tpb == 0) tpb = w6_auto_tpb(nt8c, a.mblocks);
        a.lists = tpb >= 2 ? (int)te::cdiv(nt8c, tpb) : 0;
        blocks = a.lists ? (int64_t)8 * a.lists * a.mblocks : blocks_q;
        f.tpb = tpb; f.lists = a.lists;
    }
    f.mblocks = a.mblocks; f.ntiles = a.ntiles; f.blocks = (int)blocks;
    f.idle = (int)split6_idle_blocks(a.ntiles, a.nt8, a.mblocks, a.lists);
    f.lds = (int)((size_t)U_CHUNKS * 16 + 2 * (size_t)TP_DWORDS * 4);
    return 0;
}

int te_wino6_split_form(int B, int K, int M, int H, int W, Split6Form& f) {
    Wino6Args a{};
    return wino6_plan(a, f, B, K, M, H, W);
}

int te_wino6_launch(float* out, const float* in, const float* U, const float* isc, const float* osc, const float* bias, const float* res,
                    const float* mask_ref, float mask_gain, int act, int B, int K, int M, int H, int W, hipStream_t s) {
    Wino6Args a{};
    Split6Form f;
    const int rc = wino6_plan(a, f, B, K, M, H, W);
    if (rc) return rc;
    TE_REQUIRE(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(U) | reinterpret_cast<uintptr_t>(res) |
                 reinterpret_cast<uintptr_t>(mask_ref)) & 15) == 0 && (reinterpret_cast<uintptr_t>(in) & 3) == 0, TE_ERR_UNSUPPORTED,
               "te_conv_f32(TE_CONV_3X3W6): 16-byte aligned tensors required");
    a.out = out; a.in = in; a.U = reinterpret_cast<const u32x4*>(U); a.isc = isc; a.osc = osc; a.bias = bias; a.res = res;
    a.mref = mask_ref; a.mgain = mask_gain; a.act = act;
    if (f.two_image) SPLIT6_LAUNCH_ISC(wino6q_kernel, isc, dim3((unsigned)f.blocks), WT, (size_t)f.lds, s, a);
    else SPLIT6_LAUNCH_ISC(wino6p_kernel, isc, dim3((unsigned)f.blocks), WT, (size_t)f.lds, s, a);
    return te::launch_status("te_conv_f32(TE_CONV_3X3W6)");
}
