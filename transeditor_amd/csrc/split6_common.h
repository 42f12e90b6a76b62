// Shared by the six-product split-bf16 kernels (wino6.hip, s2s6.hip, t2s6.hip, p1s6.hip, wgrad6.hip): what carries the
// numeric contract of the family - the three-piece split and the order of the six piece products - and the pieces of
// plumbing every file used to re-declare (vector types, barrier pair, XCD-banded tile decode, the big-LDS launch).  A kernel file keeps
// its tile geometry, its LDS layout and its phase schedule; the phase-profiler plumbing is te_prof.h.
#pragma once
#include "conv_common.h"

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split6_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void split6_wait_vm() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ---- the three-piece split: an fp32 value v = h + m + l with h = bf16(v), m = bf16(v - h), l = bf16(v - h - m) (8 + 8 + 8 mantissa
// bits; both subtractions are exact in fp32).  Two values are split at once, the even and the odd channel of a pair: v_cvt_pk_bf16_f32
// packs (even, odd) into one dword, which is the LDS element the MFMA fragments are read from.  An Inf operand gives h = Inf and
// v - h = NaN: the result is NaN, as the project's contract asks.
// The split is written as STEPS so that a kernel can place one step behind each MFMA of its multiplying phase (the slot programs
// `arith`).  Every step ends in a register pin: the values have no use before the staging phase, and the compiler otherwise sinks
// the whole program behind the mid-phase barrier.
// State of a split in flight, four registers the kernel owns: (te, to) = what is left of the (even, odd) value, (fe, fo) = the piece
// taken last, widened back to fp32.  (Plain floats passed by reference, not a struct: with a struct the register allocator numbers the
// even / odd registers the other way round in every kernel - same instructions, but no longer the code that was measured.)
__device__ __forceinline__ unsigned split6_piece(float te, float to) {
    const f32x2 t = {te, to};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(t, bf16x2));
}
__device__ __forceinline__ unsigned split6_take(float te, float to, float& fe, float& fo) {      // the next piece, remembered for the subtraction
    const unsigned h = split6_piece(te, to);
    fe = __builtin_bit_cast(float, h << 16);
    fo = __builtin_bit_cast(float, h & 0xFFFF0000u);
    return h;
}
__device__ __forceinline__ void split6_pin(float& te, float& to, float& fe, float& fo) { asm volatile("" : "+v"(te), "+v"(to), "+v"(fe), "+v"(fo)); }
// step j = 0..3 of the four-step form (one vector-ALU group per MFMA slot):  0: h = bf16x2(v)   1: v -= h   2: m = bf16x2(v)
// 3: v -= m, l = bf16x2(v).  (ve, vo) is read in step 0 only.  PIN_LOW: the low piece is pinned too (the slot programs that park
// their results in registers until the staging phase)
template <bool PIN_LOW = true>
__device__ __forceinline__ void split6_step4(int j, float ve, float vo, float& te, float& to, float& fe, float& fo, unsigned& h, unsigned& m, unsigned& l) {
    if (j == 0) {
        te = ve; to = vo;
        h = split6_take(te, to, fe, fo);
    } else if (j == 1) {
        te -= fe; to -= fo;
    } else if (j == 2) {
        m = split6_take(te, to, fe, fo);
    } else {
        te -= fe; to -= fo;
        l = split6_piece(te, to);
        if (PIN_LOW) asm volatile("" : "+v"(l));
    }
    split6_pin(te, to, fe, fo);
}
// step j = 0..2 of the three-step form (wgrad6.hip's row kernels: a subtraction shares its slot with the conversion behind it)
__device__ __forceinline__ void split6_step3(int j, float ve, float vo, float& te, float& to, float& fe, float& fo, unsigned& h, unsigned& m, unsigned& l) {
    if (j == 0) {
        te = ve; to = vo;
        h = split6_take(te, to, fe, fo);
    } else if (j == 1) {
        te -= fe; to -= fo;
        m = split6_take(te, to, fe, fo);
    } else {
        te -= fe; to -= fo;
        l = split6_piece(te, to);
    }
    split6_pin(te, to, fe, fo);
}

// ---- the six piece products of a multiply-add, small terms first: mm, hl, lh, hm, mh, hh (piece 0 = h, 1 = m, 2 = l of the A / B
// operand).  The five small products go to `small`, hh to `big`: kept apart, the big sum is rounded once per K step instead of six
// times (s2s6.hip: measured 3.3x the fp32 kernel's deviation from fp64 at 512 channels with one accumulator).  Kernels whose
// accumulators are transform components (wino6.hip) or that hold one tile per weight image (p1s6.hip) pass the same register twice.
__device__ __forceinline__ void split6_product(int q, const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16& big, f32x16& small) {
    constexpr int PA[6] = {1, 0, 2, 0, 1, 0}, PB[6] = {1, 2, 0, 1, 0, 0};
    f32x16& d = q < 5 ? small : big;
    d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA[q]], b[PB[q]], d, 0, 0, 0);
}

// ---- tile and M block of this workgroup.  Workgroup ids go round-robin over the 8 XCDs; banded order (nt8 = ceil(ntiles / 8), the
// default: te::xcd_banded) gives XCD x the x-th eighth of the tile list, interleaved order (nt8 = 0) tiles x, x + 8, ...  The grid is
// 8 ceil(ntiles / 8) mblocks: false = this workgroup has no tile (return at once).
__device__ __forceinline__ bool split6_tile(int ntiles, int nt8, int mblocks, int& tile, int& mb) {
    const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3;
    const int tq = jx / mblocks;
    mb = jx % mblocks;
    tile = nt8 ? (int)(((int64_t)xcd * ntiles) >> 3) + tq : tq * 8 + xcd;
    return tile < (nt8 ? (int)(((int64_t)(xcd + 1) * ntiles) >> 3) : ntiles);
}

// ---- a LIST of consecutive tiles for a workgroup that walks several (wino6q_kernel).  The tiles of an XCD, in the order split6_tile
// defines (so that neighbouring tiles keep sharing halo rows in one L2), are cut into `lists` runs whose lengths differ by at most one;
// the grid is 8 lists mblocks.  The run is tile, tile + step, ... < end (step 1 in banded order, 8 in interleaved order); false = an empty
// run.  lists == 0: one tile per workgroup, exactly split6_tile's assignment.
__device__ __forceinline__ bool split6_tile_list(int ntiles, int nt8, int mblocks, int lists, int& tile, int& end, int& step, int& mb) {
    step = nt8 ? 1 : 8;
    if (lists == 0) {
        const bool has = split6_tile(ntiles, nt8, mblocks, tile, mb);
        end = tile + step;
        return has;
    }
    const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3;
    const int lq = jx / mblocks;
    mb = jx % mblocks;
    const int first = nt8 ? (int)(((int64_t)xcd * ntiles) >> 3) : xcd;
    const int nb = nt8 ? (int)(((int64_t)(xcd + 1) * ntiles) >> 3) - first : (ntiles - xcd + 7) >> 3;          // tiles of this XCD
    const int lo = (int)((int64_t)lq * nb / lists), hi = (int)((int64_t)(lq + 1) * nb / lists);
    tile = first + step * lo;
    end = first + step * hi;
    return lo < hi;
}

// ---- a body shared by two kernels (s2s6.hip: the ping-pong and the two-image form of the kind are one function template, the kernels
// the runtime sees are thin __global__ wrappers; wgrad6.hip: the 64 x 64, masked and wide forms of the transposed kind).  The body is declared `__device__ __attribute__((optnone))` and called as
// `[[clang::always_inline]] body<...>(p);` (the attribute at the call takes precedence): the optimiser leaves the stand-alone function
// alone, lambdas included, and the code is optimised once, inside its kernel, as if it had been written there.  A plain __forceinline__
// body is optimised on its own first and again after inlining; the passes are not idempotent, and the kernels came out further from
// the code that was measured (s2s6_kernel<false>: 156 VGPRs against 163, 49 s_waitcnt against 37; profiles/refactor_split6_forms_isa.txt
// has every form that was tried and what is left with this one).  t2s6.hip keeps its two kernels written out: merged the same way, its
// two-image kernel was 0.7 - 0.9 % slower in small launches in both timing visits (profiles/refactor_split6_forms_time.txt), and a
// second attempt that went for the written-out kernels' instruction streams did not reach them (profiles/refactor_t2s6_isa.txt).
// The inlined body meets the kernel's passes later than code written in the kernel: a subexpression that two places are to share has to
// be visible to the first common-subexpression pass (not behind a short-circuit `&&`, not in a loop still to be unrolled) - wgrad6t_body's
// `active` (profiles/refactor_wgrad6t_isa.txt: with that, all of wgrad6.hip's kernels are the instruction streams of the written-out code).
// Why, and what else follows from it (refactor_t2s6_isa.txt has the evidence).  The mandatory inliner runs inside the call-graph walk,
// BEHIND the module's early passes (simplifycfg, sroa, early-cse; ipsccp; mem2reg, one instcombine).  Code written in a kernel goes
// through those early passes while its lambdas are still calls and threadIdx.x is still an opaque call, and once more through sroa /
// early-cse / value propagation / instcombine after the lambdas are inlined; the top-level code of an inlined body sees only the second
// round, with the lambdas' code already around it.  The lambdas themselves are treated alike in both forms.  So:
//  - only top-level expressions over locals that no lambda captures by reference can come out differently; what a lambda computes is safe;
//  - write such an expression as the early instcombine would leave it.  `readfirstlane(tid >> 6)` becomes `readfirstlane(tid) >> 6` there
//    (the shift is hoisted while the sign of tid is unknown, and `wid >> 2` stays an arithmetic shift of the readfirstlane - one sign
//    extension later on): written that way in the body, the decode of the wave index is the kernel's.  A single-use `2 * (wq & 1)` becomes
//    `(wq << 1) & 2` before a lambda's `wq & 1` can be merged with it: write the doubled form where it is first used;
//  - a temporary array that a lambda of the kernel declares must stay in that lambda (sroa gives it the type of the first pass that
//    sees it: `bf16x8 av[2][3]` moved from `multiply` to the body turned 108 LDS reads from <8 x i16> plus a cast into <8 x bfloat>);
//  - the body is compiled as at -O0 by the front end: `a * b + c` is `llvm.fmuladd` without the `contract` flag instead of fmul / fadd
//    `contract`.  The instructions are the same fused ones; only the IR differs;
//  - integer ranges are the limit: the kernel's value propagation narrows `rest / 20`, `rest % 5` to 8-bit divisions after the early
//    instcombine has simplified `gt < 200 ? gt : 0`; in the inlined body both happen in the other order and a later pass repairs most, not
//    all, of it.  No source form was found for that one, nor for which of two equal `wq >> 1` the weight DMA's address ends up sharing.

// ---- host: which form of a kind to launch.  form_sel = the kind's form hook counted from its two-image default: 0 = ping-pong, 1 = the
// two-image form where M % 128 == 0 and its grid (blocks_q: half as many blocks) still gives every CU a block, 2 = the two-image form
// wherever M % 128 == 0 (tests)
inline bool split6_two_image(int form_sel, int M, int64_t blocks_q) { return form_sel >= 1 && M % 128 == 0 && (form_sel == 2 || blocks_q >= te::kNumCU); }

// ---- host: the blocks that split6_tile (lists == 0: a grid of 8 ceil(ntiles / 8) mblocks) or split6_tile_list (8 lists mblocks) leaves
// without a tile, by the same arithmetic: an XCD with nb tiles fills min(nb, slots) of its slots
inline int64_t split6_idle_blocks(int ntiles, int nt8, int mblocks, int lists) {
    const int64_t slots = lists ? lists : te::cdiv(ntiles, 8);
    int64_t idle = 0;
    for (int xcd = 0; xcd < 8; ++xcd) {
        const int first = nt8 ? (int)(((int64_t)xcd * ntiles) >> 3) : xcd;
        const int nb = nt8 ? (int)(((int64_t)(xcd + 1) * ntiles) >> 3) - first : (ntiles - xcd + 7) >> 3;
        idle += slots - std::min<int64_t>(nb, slots);
    }
    return idle * mblocks;
}

// ---- host: one launch of a kernel that needs more than 64 KB of dynamic LDS.  hipFuncSetAttribute is done once per (kernel, device):
// one flag per instantiation of this template, i.e. per kernel.
template <auto KERNEL, class Args>
inline void split6_launch(dim3 grid, int threads, size_t lds, hipStream_t s, const Args& a) {
    static std::atomic<uint64_t> attr_done{0};
    te::allow_big_lds(attr_done, (const void*)KERNEL, 160 * 1024);
    KERNEL<<<grid, threads, lds, s>>>(a);
}
// ... and the choice between the two instantiations of a kernel template over ISC (the launch carries style scales)
#define SPLIT6_LAUNCH_ISC(kernel, isc, blocks, threads, lds, s, a) \
    ((isc) ? split6_launch<kernel<true>>(blocks, threads, lds, s, a) : split6_launch<kernel<false>>(blocks, threads, lds, s, a))
