/*
 * te_hip.h — C ABI of libte_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * TransEditor generator hot path.
 *
 * Conventions (SURVEY §8b "What a C-ABI replacement must export"):
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless stated; the CALLER owns every
 *     buffer (the Python host allocates through the torch caching allocator);
 *   - functions only ENQUEUE work on `stream` (a hipStream_t passed as void*): no allocation,
 *     no synchronisation; safe to call from several host threads.  The process-wide mutable state behind this ABI is:
 *       - te_wgrad_split_bf16 (initialised from TE_SPLIT_BF16; the Python layer writes it): selects the split bf16 or the fp32
 *         weight-gradient kernel and with it the slab partition - results are fp32-equivalent, not bit-identical, across its values;
 *       - five test and tool hooks, te_conv_wino6_form, te_conv_wino6_tiles_per_block, te_conv_s2s6_form, te_conv_t2s6_form and
 *         te_wgrad_t2_wide, which select between kernels of one kind, or between grids of one kernel, with bit-identical results
 *         (tests compare the two live kernels of a kind on one input); te_conv_split_form and te_wgrad6_form name the kernel that a launch takes under them;
 *       - TE_XCD_INTERLEAVED, read once from the environment: the order in which the convolution launches hand tiles to the XCDs
 *         (te_common.h); results are bit-identical;
 *       - the per-thread last-error string;
 *   - return 0 on success, a negative TE_ERR_* for argument validation failures, or a positive
 *     hipError_t if the launch failed; nothing throws across the ABI.  te_last_error_string()
 *     describes the calling thread's most recent failure.
 *
 * Each entry point names the reference interface it replaces (paths relative to the
 * BillyXYB/TransEditor repository root).
 *
 * Precision: the model path is fp32 (suffix _f32).  The reference's two CUDA ops dispatch over half / float / double
 * (AT_DISPATCH_FLOATING_TYPES_AND_HALF, fused_bias_act_kernel.cu:79, upfirdn2d_kernel.cu:196); the TransEditor scripts
 * only ever run them in fp32 (no autocast / .half() anywhere on the path), so the tuned kernels are fp32, and K1 / K2 —
 * the two ops that ARE the reference's native boundary — also exist as te_bias_act_f16 / _f64 and te_upfirdn2d_f16 / _f64
 * (plain kernels, same semantics).  Every other entry point is fp32 only: the Python wrappers raise on any other dtype
 * instead of silently casting (tests/test_gpu_generator.py::test_non_contiguous_and_wrong_dtype_inputs).
 *
 * Run-to-run reproducibility.  EVERY result of this library is bit-reproducible from run to run (same inputs, same
 * library, same device): there is no atomic add on any path.  Reductions that span thread blocks go through per-block
 * partials in a caller-owned workspace and a fixed-order second pass: the split-K convolution (te_conv_ws_f32 /
 * te_conv_res_f32; te_conv_f32, which has no workspace argument, does not split), te_small_gemm_splitk_f32, the
 * per-(sample, chunk) correlation slabs of te_wgrad_f32 / te_rgb_wgrad_f32, the bias gradient of te_bias_act_bwd_f32 /
 * te_bias_act_bwd_rgb_f32 (workspace: te_bias_act_bwd_ws_floats), the per-tile bias-gradient partials of te_blur_actgrad_f32 /
 * te_blur_gradact_f32, all three outputs of te_wgrad_reduce_f32 (workspace: te_wgrad_reduce_ws_floats), te_chan_dot_f32, the
 * layer / pixel norm and minibatch-stddev kernels.  The library is built WITHOUT -munsafe-fp-atomics.
 * (tests/test_gpu_determinism.py runs the 256-px generator and discriminator backward twice and compares bit for bit.)
 */
#ifndef TE_HIP_H
#define TE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TE_ABI_VERSION 3

#define TE_ERR_NULL -1      /* required pointer is NULL              */
#define TE_ERR_SHAPE -2     /* non-positive / inconsistent dimension */
#define TE_ERR_UNSUPPORTED -3
#define TE_ERR_WORKSPACE -4 /* workspace too small                   */

typedef void* te_stream_t;

int te_version(void);
const char* te_last_error_string(void);
/* name of the code-object architecture this library was built for ("gfx950") */
const char* te_arch(void);

/* ---------------------------------------------------------------------------------------------
 * K1  fused bias + activation.  Replaces pybind `fused.fused_bias_act(input, bias, refer, act,
 * grad, alpha, scale)` — utils/op/fused_bias_act.cpp:11-21, kernel fused_bias_act_kernel.cu:18-49.
 *   x' = x + b[(i / step_b) % size_b]     (b may be NULL = no bias; integer index math bit-exact)
 *   act*10+grad: 10/11 linear, 12 -> 0, 30 lrelu(x'), 31 x' * (ref>0 ? 1 : alpha), 32 -> 0
 *   out = y * scale.   `ref` may be NULL (treated as 0).  In-place (out == x) is allowed.
 */
int te_bias_act_f32(float* out, const float* x, const float* b, const float* ref, int act, int grad,
                    float alpha, float scale, int64_t size_x, int64_t step_b, int64_t size_b,
                    te_stream_t stream);
/* The reference dispatches this op over half / float / double (AT_DISPATCH_FLOATING_TYPES_AND_HALF,
 * fused_bias_act_kernel.cu:79) and converts its float `alpha` / `scale` to scalar_t; same here.  Half buffers are IEEE
 * binary16 (`__half` / torch.float16) passed as void*; arithmetic in fp32 with one rounding at the store. */
int te_bias_act_f16(void* out, const void* x, const void* b, const void* ref, int act, int grad,
                    float alpha, float scale, int64_t size_x, int64_t step_b, int64_t size_b,
                    te_stream_t stream);
int te_bias_act_f64(double* out, const double* x, const double* b, const double* ref, int act, int grad,
                    float alpha, float scale, int64_t size_x, int64_t step_b, int64_t size_b,
                    te_stream_t stream);

/* Backward of the fused lrelu in ONE pass — replaces FusedLeakyReLUFunctionBackward.forward,
 * utils/op/fused_act.py:18-38 (kernel call + grad_input.sum(dim)):
 *   gi[n,c,i] = g[n,c,i] * (ref[n,c,i] > 0 ? 1 : alpha) * scale ;  gb[c] = sum_{n,i} gi[n,c,i]
 * Layout [outer][C][inner].  gb (may be NULL) is WRITTEN (no zero fill needed).  The streaming form combines per-block partial
 * sums through the caller's workspace `ws` of te_bias_act_bwd_ws_floats(outer, C, inner) floats (0: none needed, ws may be
 * NULL) and a fixed-order second pass: bit-reproducible, no atomics.  */
int64_t te_bias_act_bwd_ws_floats(int64_t outer, int64_t C, int64_t inner);
int te_bias_act_bwd_f32(float* gi, float* gb, float* ws, const float* g, const float* ref, float alpha, float scale,
                        int64_t outer, int64_t C, int64_t inner, te_stream_t stream);
/* te_bias_act_bwd_f32 with the data gradient of a ToRGB layer (1x1 modulated convolution to 3 channels, ToRGB.forward,
 * model_spatial_query.py:416-425) folded in — te_rgb_dgrad_f32, the gradient-accumulation add and the activation gradient
 * in one pass over the activation-sized tensors:
 *     gi = ( g + wscale * srgb[n,c] * sum_o wrgb[o,c] * grgb[n,o,:] ) * (ref > 0 ? 1 : alpha) * scale ,   gb[c] = sum gi
 * g [outer,C,inner] may be NULL (nothing but ToRGB consumes the activation), grgb [outer,3,inner], wrgb [3,C], srgb [outer,C] or
 * NULL; gb written or NULL (needs ws, same size as above).  te_bias_act_bwd_rgb_supported: inner % 4 == 0 and inner >= 1024. */
int te_bias_act_bwd_rgb_supported(int64_t outer, int64_t C, int64_t inner);
int te_bias_act_bwd_rgb_f32(float* gi, float* gb, float* ws, const float* g, const float* ref, const float* grgb, const float* wrgb,
                            const float* srgb, float wscale, float alpha, float scale, int64_t outer, int64_t C, int64_t inner,
                            te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K2  upfirdn2d.  Replaces pybind `upfirdn2d_op.upfirdn2d(input[major,H,W,minor], kernel, up_x,
 * up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)` — utils/op/upfirdn2d.cpp:12-23, kernel
 * upfirdn2d_kernel.cu:52-137.  Output dims follow upfirdn2d.py:101-102:
 *   out_h = (in_h*up_y + pad_y0 + pad_y1 - kh) / down_y + 1 (same for w); caller allocates
 *   out[major, out_h, out_w, minor].  True convolution (taps flipped), zero fill outside the
 *   input.  Unlike the reference (6 template modes, garbage otherwise) every (up, down, k) works.
 * Optional fused epilogue (b != NULL or act != 0), minor must be 1: channel = major_index % size_b,
 *   out = act(out + b[channel]) * scale with act 0 = linear, 3 = lrelu(alpha).
 */
int te_upfirdn2d_f32(float* out, const float* x, const float* k, int64_t major, int in_h, int in_w,
                     int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0,
                     int pad_x1, int pad_y0, int pad_y1, const float* b, int64_t size_b, int act,
                     float alpha, float scale, te_stream_t stream);
/* half / double forms of the same op (upfirdn2d_kernel.cu:57-58 dispatches over both): every (up, down, taps), no fused
 * epilogue (the reference op has none); taps in the tensors' own type; accumulation in fp32 / double. */
int te_upfirdn2d_f16(void* out, const void* x, const void* k, int64_t major, int in_h, int in_w,
                     int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0,
                     int pad_x1, int pad_y0, int pad_y1, te_stream_t stream);
int te_upfirdn2d_f64(double* out, const double* x, const double* k, int64_t major, int in_h, int in_w,
                     int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0,
                     int pad_x1, int pad_y0, int pad_y1, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * F1  modulated convolution family (reference: ModulatedConv2d.forward, model_spatial_query.py:
 * 296-337, which the reference runs as stock grouped F.conv2d / F.conv_transpose2d with B
 * materialised weight copies).  Here ONE shared weight tensor is used and the per-sample style
 * modulation / demodulation are row/column scalings fused into the kernel:
 *     out[b,m,:,:] = act( osc[b,m] * conv(isc[b,k] * in[b,k,:,:], W)[m] + bias[m] )
 *
 * Weights are consumed in a packed layout  Wp[tap][Kp][Mp]  (Kp = K rounded up to 16, Mp = M
 * rounded up to 128, zero padded) produced by te_conv_pack_weights_f32.
 */

/* kind of convolution executed by te_conv_f32 */
#define TE_CONV_3X3 0    /* 3x3, stride 1, pad 1           in [B,K,H,W]       -> out [B,M,H,W]        */
#define TE_CONV_T2 1     /* 3x3 transposed, stride 2, pad 0 in [B,K,H,W]       -> out [B,M,2H+1,2W+1]  */
#define TE_CONV_S2 2     /* 3x3, stride 2, pad 0           in [B,K,2H+1,2W+1] -> out [B,M,H,W]        */
#define TE_CONV_1X1 3    /* 1x1                            in [B,K,H,W]       -> out [B,M,H,W]        */
#define TE_CONV_3X3W 4   /* TE_CONV_3X3 through the 1-D Winograd F(2,3) kernel (2/3 of the MFMAs; same result to fp32 round-off).
                            Shapes: te_conv_wino_supported; weights packed TE_PACK_WFWD / TE_PACK_WDGRAD; never split */
#define TE_CONV_3X3W6 5  /* the same Winograd form with its products on the bf16 matrix pipe: every fp32 operand split into three bf16
                            pieces, six exact piece products accumulated in fp32 - fp32-equivalent results (the dropped terms are below
                            2^-24 of the product; measured deviation from double not larger than the fp32 MFMA chain's).
                            Shapes: te_conv_wino6_supported; weights packed TE_PACK_W6FWD / TE_PACK_W6DGRAD; never split.
                            Range: finite operands of any fp32 magnitude up to ~1.7e38 (the transform adds two neighbours) behave as
                            in TE_CONV_3X3 (tests: scale sweep 1e-30 ... 1e+30 at the 5e-6 bar); below |x| ~ 1e-33 the third, then
                            the second piece of an element underflows and that element's products lose bits (relative error 2^-15
                            at 1e-36: contributions that small are below the rounding unit of any O(1e-30)+ sum anyway).
                            Non-finite operands: an Inf / NaN input element makes exactly the outputs whose 3x3 window contains it
                            non-finite - the same set as TE_CONV_3X3 - but as NaN where the direct kernel gives +-Inf
                            (inf = h, inf - h = NaN is the second piece).  TE_SPLIT_BF16=0 (host) selects TE_CONV_3X3W instead. */

#define TE_CONV_S2S6 6   /* TE_CONV_S2 with its products on the bf16 matrix pipe (three-piece split, six exact piece products per multiply-add,
                            fp32 accumulation: fp32-equivalent like TE_CONV_3X3W6, same range / non-finite behaviour).
                            Shapes: te_conv_s2s6_supported; weights packed TE_PACK_S6FWD / TE_PACK_S6SWAP; never split.
                            Reference: F.conv2d(stride 2) of ConvLayer(downsample=True), model_spatial_query.py:765-779, and the adjoint
                            of conv_transpose2d(stride 2), :318 */

#define TE_CONV_T2S6 7   /* TE_CONV_T2 with its products on the bf16 matrix pipe (three-piece split, fp32-equivalent like TE_CONV_3X3W6): the body
                            cells [0,H) x [0,W) by t2s6_kernel / t2s6q_kernel, the last output row and column by t2_edge_kernel (plain fp32
                            arithmetic on the fp32 copy of the weights in the same packed buffer), all in csrc/t2s6.hip.
                            Shapes: te_conv_t2s6_supported; weights packed TE_PACK_T6FWD / TE_PACK_T6SWAP; never split; no residual / mask.
                            Reference: conv_transpose2d(stride 2) of ModulatedConv2d.forward, model_spatial_query.py:310-321 */

#define TE_CONV_1X1S6 8   /* TE_CONV_1X1 with its products on the bf16 matrix pipe (round 6; three-piece split, six exact piece products per
                            multiply-add, fp32 accumulation: fp32-equivalent like TE_CONV_3X3W6, same range / non-finite behaviour): the
                            skip branch of the discriminator's ResBlocks and its data gradient.  Plain product + optional residual only
                            (isc, osc, bias, mask_ref must be NULL, act 0).  Shapes: te_conv_p1s6_supported; weights packed
                            TE_PACK_P6FWD / TE_PACK_P6DGRAD; never split.
                            Reference: F.conv2d of EqualConv2d (1x1) in ResBlock.skip, model_spatial_query.py:173-181, :780-798 */
#define TE_CONV_KINDS 9   /* number of kinds: valid values are 0 .. TE_CONV_KINDS - 1 */

/* how te_conv_pack_weights_f32 reads the source weight w[Co][Ci][kh][kw] (model layout,
 * ModulatedConv2d.weight[0]) */
#define TE_PACK_FWD 0    /* M = Co, K = Ci, taps as stored         (forward 3x3 / 1x1 / T2, and S2) */
#define TE_PACK_DGRAD 1  /* M = Ci, K = Co, taps flipped           (data gradient of 3x3 / 1x1)     */
#define TE_PACK_SWAP 2   /* M = Ci, K = Co, taps as stored         (S2 as data gradient of T2)       */
#define TE_PACK_WFWD 3   /* TE_CONV_3X3W forward:       U[K/8][ky][c][8][M], U[ky][c] = G w[.., ky, :]  (12 K M floats)  */
#define TE_PACK_WDGRAD 4 /* TE_CONV_3X3W data gradient: the same transform of the flipped, transposed taps (M = Ci)     */
#define TE_PACK_W6FWD 5  /* TE_CONV_3X3W6 forward: U = G w split into bf16 pieces, MFMA fragment order
                            U6[K/16][piece][ky][c][M/32][64 lanes][8 bf16]  (36 K M bf16 = 18 K M floats).  The packing accepts
                            Co % 32 == Ci % 32 == 0; the kernel (te_conv_wino6_supported) needs K % 32 == 0, M % 64 == 0                */
#define TE_PACK_W6DGRAD 6 /* TE_CONV_3X3W6 data gradient (flipped, transposed taps; M = Ci)                               */
#define TE_PACK_S6FWD 7  /* TE_CONV_S2S6, M = Co, K = Ci, taps as stored: three bf16 pieces per weight, MFMA fragment order
                            S6[K/16][piece][tap][M/32][64 lanes][8 bf16]  (27 K M bf16).  The packing accepts M % 32 == 0, K % 16 == 0;
                            the kernel (te_conv_s2s6_supported) needs M % 64 == 0, K % 16 == 0, K >= 32                                 */
#define TE_PACK_S6SWAP 8 /* TE_CONV_S2S6 as data gradient of the transposed kind: M = Ci, K = Co, taps as stored                  */
#define TE_PACK_T6FWD 9  /* TE_CONV_T2S6, M = Co, K = Ci: the TE_PACK_S6FWD layout followed (16-byte aligned) by the TE_PACK_FWD layout  */
#define TE_PACK_T6SWAP 10 /* TE_CONV_T2S6 as data gradient of the strided kind: TE_PACK_S6SWAP followed by TE_PACK_SWAP                   */
#define TE_PACK_P6FWD 11  /* TE_CONV_1X1S6, M = Co, K = Ci (1x1 weights): P6[K/16][piece][M/32][64 lanes][8 bf16] (3 K M bf16; Co % 32 == 0,
                             Ci % 16 == 0)                                                                                                */
#define TE_PACK_P6DGRAD 12 /* TE_CONV_1X1S6 as data gradient: M = Ci, K = Co (Ci % 32 == 0, Co % 16 == 0)                                  */
#define TE_PACK_KINDS 13   /* number of layouts: valid values are 0 .. TE_PACK_KINDS - 1 */

int64_t te_conv_packed_numel(int kind_pack, int Co, int Ci, int ksize);
int te_conv_pack_weights_f32(float* wp, const float* w, float wscale, int kind_pack, int Co, int Ci,
                             int ksize, te_stream_t stream);
/* two layouts of the same weight in one launch (a training forward packs the data-gradient layout along) */
int te_conv_pack_weights2_f32(float* wp_a, int kind_a, float* wp_b, int kind_b, const float* w, float wscale, int Co, int Ci,
                              int ksize, te_stream_t stream);

/* n (weight, layout) jobs in one launch per 64: job e packs w[e] [Co[e]][Ci[e]][ksize[e]]^2 into wp[e] with layout
 * kind_pack[e] and constant wscale[e] (host arrays).  The training step refreshes every packed layout of a model with it right
 * after the optimiser step (torch.optim.Adam's step, train_spatial_query.py:207 / :224) instead of ~60 tiny launches per iteration. */
int te_conv_pack_weights_multi_f32(int n, float* const* wp, const float* const* w, const float* wscale, const int* kind_pack,
                                   const int* Co, const int* Ci, const int* ksize, te_stream_t stream);

/* `H`,`W` are ALWAYS the low-resolution size (the H,W of the table above).  isc [B,K], osc [B,M],
 * bias [M] may be NULL.  act: 0 linear, 3 lrelu(0.2)*sqrt(2), 4 lrelu(0.2) with gain 1 (a residual branch that folds the
 * 1/sqrt(2) of `(out + skip) / sqrt(2)`, model_spatial_query.py:796) — applied after osc and bias. */
int te_conv_f32(float* out, const float* in, const float* wp, const float* isc, const float* osc,
                const float* bias, int act, int kind, int B, int K, int M, int H, int W,
                te_stream_t stream);
/* Small images (4x4 ... 16x16 layers) split the input-channel loop over the grid so every CU gets work.
 * te_conv_splitk_count returns the number of splits S of a problem (1 = no split).  te_conv_ws_f32 is te_conv_f32 with
 * a caller-owned workspace ws[S][B][M][Ho][Wo] (ignored / may be NULL when S == 1): each split writes its own slab and a
 * second kernel sums them in a fixed order (DETERMINISTIC, no atomics, no memset).  te_conv_f32 itself (no workspace)
 * never splits (same result up to summation order, slower on 4x4 ... 16x16 images). */
int te_conv_splitk_count(int kind, int B, int K, int M, int H, int W);
/* Which form of the fp32 direct kernel (conv_mfma_kernel<KIND, TC, HAS_ISC, MS, OCC, FAST, EPI>, csrc/conv.hip) a launch runs, on which
 * cell tiles and grid (host only, nothing is launched: the answer is the plan that te_conv_res_f32 itself makes and then launches).
 * kind: TE_CONV_3X3, TE_CONV_T2, TE_CONV_S2 or TE_CONV_1X1 (the other kinds: TE_ERR_UNSUPPORTED).  has_isc: style scales given;
 * epi: 0 none, 1 residual, 2 mask, 3 both; with_ws: a split-K workspace is given (te_conv_ws_f32 / te_conv_res_f32 with ws), 0 = te_conv_f32.
 * form[TE_CONV_FORM_INTS]:
 *   [0] tc            tile class that launches (0, 1, 2: the block tiles for M >= 96, >= 48, below; 3: the deep-stage 1x1, which exists as FAST only)
 *   [1] fast          the FAST kernel (whole stages, 16-byte row segments)        [2] ms   the kernel's multi-sample TEMPLATE flag
 *   [3] multi_sample  some tile holds more than one sample (with ms == 0: the plain kernel's run-time path)
 *   [4] occ           waves per SIMD the kernel is compiled for                   [5] ksplit  splits that launch (1 without workspace)
 *   [6] nreg          cell regions (T2 beyond the padded sizes: body, last column, last row)
 *   [7] ntiles  [8] nbody (tiles of the first region, dealt to the XCDs in 8 bands)  [9] mblocks  [10] grid x (blocks; some may have no tile)
 *   then per region r at TE_CONV_FORM_HEAD + r * TE_CONV_FORM_REGION: TW, TH, NS (samples a tile has room for), NSv (samples staged),
 *   tiles_x, tiles_y, tapmask, TH0 (rows of the tile before the staging budget halved them); zeros past nreg.
 * TE_ERR_NULL / TE_ERR_SHAPE on bad arguments, and the launch's own refusals with the launch's code (an epilogue with style scales or on
 * the strided / transposed kinds, a tile beyond the staging budget: TE_ERR_UNSUPPORTED); a refusal leaves form untouched. */
#define TE_CONV_FORM_HEAD 11
#define TE_CONV_FORM_REGION 8
#define TE_CONV_FORM_INTS (TE_CONV_FORM_HEAD + 3 * TE_CONV_FORM_REGION)
int te_conv_form(int kind, int B, int K, int M, int H, int W, int has_isc, int epi, int with_ws, int* form);
/* The same for the four split-bf16 kinds TE_CONV_3X3W6, TE_CONV_S2S6, TE_CONV_T2S6 and TE_CONV_1X1S6 (the other kinds:
 * TE_ERR_UNSUPPORTED): which kernel of the kind a launch runs and on which grid, under the current values of te_conv_wino6_form,
 * te_conv_wino6_tiles_per_block, te_conv_s2s6_form and te_conv_t2s6_form (host only, nothing is launched: the answer is the plan that the
 * kind's launch itself makes and then dispatches on).  has_isc: style scales given (the ISC instantiation; TE_CONV_1X1S6 takes none:
 * TE_ERR_UNSUPPORTED); with_scratch: TE_CONV_T2S6 is given its column scratch (te_conv_t2s6_ws_floats), ignored for the other kinds.
 * form[TE_CONV_SPLIT_FORM_INTS]:
 *   [0] two_image   the two-image kernel (a block owns 128 output channels; TE_CONV_1X1S6 has no other), 0 = the ping-pong kernel
 *   [1] pair16      TE_CONV_3X3W6 at W == 16: two samples side by side in a tile row
 *   [2] mblocks  [3] ntiles  [4] blocks (grid x)  [5] idle: blocks of the grid that get no tile (ntiles % 8 != 0, or runs that stay empty)
 *   [6] tpb, [7] lists   two-image TE_CONV_3X3W6: tiles per run as set or chosen automatically (1: a tile per block) and the runs per
 *                        XCD that follow from it (0: a tile per block); zeros elsewhere
 *   [8] lds         dynamic LDS bytes of the (body) kernel
 *   [9] edge_ct  [10] edge_line_tiles  [11] edge_blocks   TE_CONV_T2S6: t2_edge_kernel's CT (4 where H >= 64 and W >= 64, else 2), its line
 *                        tiles per (sample, 64 output channels) and its grid x; zeros elsewhere
 *   [12] scratch    TE_CONV_T2S6: the body kernel hands the last input column to the edge kernel through the scratch
 *   [13] isc        the ISC instantiation
 * TE_ERR_NULL / TE_ERR_SHAPE on bad arguments and the launch's own refusal with the launch's code (te_conv_*_supported: TE_ERR_UNSUPPORTED);
 * a refusal leaves form untouched.  Operand alignment is the launch's affair: the plan does not depend on it. */
#define TE_CONV_SPLIT_FORM_INTS 14
int te_conv_split_form(int kind, int B, int K, int M, int H, int W, int has_isc, int with_scratch, int* form);
/* 1 if TE_CONV_3X3W covers the problem: K % 8 == 0, W % 32 == 0, and M % 128 == 0 with H % 4 == 0, or M % 64 == 0 with
 * H % 8 == 0, or M % 32 == 0 with H % 16 == 0 (block tile = 128 / 64 / 32 output channels x 4 / 8 / 16 rows x 32 columns):
 * every 3x3 stride-1 layer of the generator and discriminator from 32x32 up incl. the 32 / 64-channel tail of FFHQ-1024; the
 * 513-channel final convolution of the discriminator and images narrower than 32 stay on TE_CONV_3X3.  Reference: the grouped F.conv2d of ModulatedConv2d.forward, model_spatial_query.py:331-333,
 * and EqualConv2d.forward :173-181. */
int te_conv_wino_supported(int B, int K, int M, int H, int W);
/* 1 if TE_CONV_3X3W6 covers the problem: K % 32 == 0, M % 64 == 0, H % 8 == 0, and W % 32 == 0 or (round 6) W == 16 with an even batch
 * (two samples side by side in a 32-column tile row) */
int te_conv_wino6_supported(int B, int K, int M, int H, int W);
/* 1 if TE_CONV_S2S6 covers the problem (H, W = OUTPUT size): K % 16 == 0 and K >= 32, M % 64 == 0, H % 8 == 0, W % 16 == 0 */
int te_conv_s2s6_supported(int B, int K, int M, int H, int W);
/* 1 if TE_CONV_T2S6 covers the problem (H, W = INPUT size): K % 16 == 0 and K >= 32, M % 64 == 0, H % 8 == 0, W % 16 == 0 */
int te_conv_t2s6_supported(int B, int K, int M, int H, int W);
/* 1 if TE_CONV_1X1S6 covers the problem: K % 64 == 0, M % 128 == 0, H * W % 256 == 0 and a grid of at least half the CUs */
int te_conv_p1s6_supported(int B, int K, int M, int H, int W);
/* Kernel form of TE_CONV_3X3W6 (a test and tool hook, process-wide; the results do not depend on it; returns the previous value;
 * anything but 1 .. 3 only queries):
 *   2 = two-image (round 6, default): as 1, but a block owns 128 output channels - every staged half tile is multiplied by two
 *       64-channel weight images, so the style scale / B^T d / three-piece split of an input element is done once per 128 output
 *       channels instead of once per 64; launches with M % 128 != 0, or whose grid would leave CUs without a block, run form 1
 *       (3 = the two-image form wherever M % 128 == 0, whatever the grid: tests);
 *   1 = ping-pong (round 5): the two waves of every SIMD work half a stage apart - one feeds the matrix pipe from its
 *       half tile while the other transforms / splits / writes the next half tile and renews half of the weight image.
 * All forms issue the same products in the same order per output element: results are bit-identical. */
int te_conv_wino6_form(int form);
/* Tiles per block of the two-image form of TE_CONV_3X3W6 (a test and tool hook, process-wide; returns the previous value; anything
 * but 0 .. 4096 only queries).  A block of that form walks a run of consecutive tiles of its XCD with one M block and carries its
 * pipeline across them: the fetch, the split arithmetic and the weight DMA of a tile's first stage run in the shadow of the previous
 * tile's last stage; only the epilogue stands between two tiles.
 *   0 = automatic (default): runs of at most four tiles, fewer (three, two) where four would leave CUs without a block or cost the
 *       launch more rounds of tile times over the CUs than one-tile blocks do; one tile per block where even two would;
 *   1 = one tile per block;
 *   n >= 2 = runs of at most n tiles (lengths differ by at most one within an XCD).
 * Every output element sees the same products in the same order whatever the value: results are bit-identical. */
int te_conv_wino6_tiles_per_block(int n);
/* Kernel form of TE_CONV_S2S6 (returns the previous value; anything but 0 .. 2 only queries), a test and tool hook like the one above:
 *   1 = (round 6, default) the two-image form: a block owns 128 output channels and multiplies every staged half tile by two
 *       64-channel weight images (half the fetches, split arithmetic and LDS writes per MFMA) where M % 128 == 0 and the grid
 *       still gives every CU a block, the ping-pong form elsewhere (2 = the two-image form wherever M % 128 == 0: tests);
 *   0 = ping-pong (round 5).
 * Same products in the same order per output element: results are bit-identical. */
int te_conv_s2s6_form(int form);
/* the same hook for TE_CONV_T2S6 (t2s6q_kernel / t2s6_kernel) */
int te_conv_t2s6_form(int form);
/* TE_CONV_T2S6 only: `ws` of te_conv_ws_f32 / te_conv_res_f32 is an OPTIONAL scratch of te_conv_t2s6_ws_floats(B, K, H) = B * K * H
 * floats through which the body kernel hands the (style-scaled) last input column to the kernel that computes the last output
 * row / column (round 6); NULL is legal - that kernel then gathers the column from `in` itself, one cache line per element. */
int64_t te_conv_t2s6_ws_floats(int B, int K, int H);
int te_conv_ws_f32(float* out, float* ws, const float* in, const float* wp, const float* isc, const float* osc,
                   const float* bias, int act, int kind, int B, int K, int M, int H, int W, te_stream_t stream);
/* te_conv_ws_f32 with two more epilogue stages (not for TE_CONV_T2; a split launch, S > 1, needs the workspace):
 *     out = ( act(osc * conv + bias) + res ) * (mask_ref > 0 ? mask_gain : 0.2 * mask_gain)
 * res (shaped like out, may be NULL) carries the sum of a ResBlock's two branches (model_spatial_query.py:796, forward) and
 * the sum of the two gradient branches that meet at the block's input (backward) without an extra elementwise pass;
 * mask_ref (shaped like out, may be NULL) is the saved output of a fused bias + leaky-ReLU(0.2) * mask_gain layer whose
 * OUTPUT this data gradient lands on: its activation gradient (fused_bias_act_kernel.cu:26-47, grad pass) in this epilogue. */
int te_conv_res_f32(float* out, float* ws, const float* in, const float* wp, const float* isc, const float* osc,
                    const float* bias, const float* res, const float* mask_ref, float mask_gain, int act, int kind, int B,
                    int K, int M, int H, int W, te_stream_t stream);

/* Weight-gradient correlation, per sample and per pixel chunk ("slabs"), NO modulation applied:
 *   slab[b][s][co][ci][tap] = sum_{pixels of chunk s} g[b,co,p (+) tap] * x[b,ci,p]
 * kind TE_CONV_3X3 / TE_CONV_1X1: g [B,Co,H,W], x [B,Ci,H,W];
 * kind TE_CONV_T2: g [B,Co,2H+1,2W+1], x [B,Ci,H,W]  (weight gradient of the transposed conv).
 * te_wgrad_slab_count returns S (chunks per sample) for the given problem; the caller allocates
 * slabs[B][S][Co][Ci][taps] and reduces them with te_wgrad_reduce_f32. */
int te_wgrad_slab_count(int kind, int B, int Co, int Ci, int H, int W);
/* 1 when te_wgrad_f32 / te_wgrad_group_f32 run this problem in the PAIR form (3x3 only: horizontal cell pairs, the three taps of
 * a kernel row from four products per pair - 1-D Winograd F(3,2) - i.e. 2/3 of the direct form's multiply-adds on the matrix
 * pipe for the same slabs), else 0.  Only a report for FLOP accounting (bench.py): results and slab layout do not depend on it. */
int te_wgrad_pair_form(int kind, int Co, int Ci, int H, int W);
/* Round 5: the 3x3 correlation on the bf16 matrix pipe (csrc/wgrad6.hip: pair form, every fp32 operand split into three bf16 pieces,
 * six exact piece products per multiply-add, fp32 accumulation - fp32-equivalent slabs, same layout, same reducers).
 * te_wgrad_split_supported: 1 where it applies (Co % 64 == 0, Ci % 64 == 0; kind TE_CONV_3X3: W % 32 == 0; kind TE_CONV_T2 - direct
 * form, nine taps x six products - W % 16 == 0; round 6: kind TE_CONV_1X1 with Co % 128 == 0, Ci % 128 == 0, W % 16 == 0).
 * te_wgrad_split_bf16(0 | 1): process-wide switch (environment TE_SPLIT_BF16 at load time), returns the previous value; any other
 * argument only queries.  With the switch on, te_wgrad_f32 / te_wgrad_group_f32 take the kernel where it applies and the fp32
 * kernel elsewhere; te_wgrad_slab_count and te_wgrad_group_plan plan their chunks for the kernel that te_wgrad6_form (below) names,
 * so they follow the same switch. */
int te_wgrad_split_supported(int kind, int Co, int Ci, int H, int W);
int te_wgrad_split_bf16(int on);
/* Round 6: form of the split transposed-kind kernel - 1 (default): a block owns 64 channels of the (2H+1) x (2W+1) tensor x 128 of the
 * H x W one where Ci % 128 == 0 (half the staging work and re-reads of the big tensor per MFMA), 0: 64 x 64 everywhere.  Bit-identical
 * slabs; returns the previous value, any other argument only queries.  A test and tool hook (see the conventions above). */
int te_wgrad_t2_wide(int on);
/* Kernel that te_wgrad_f32 (NB = 1) / te_wgrad_group_f32 (NB samples per slab) run for this problem under the current switches, for
 * 16-byte aligned g and x (misaligned operands take the fp32 kernel): TE_WG6_FP32 (the fp32 kernel) or one of the split forms.  The
 * launch dispatches on this function; a host query for tests. */
enum { TE_WG6_FP32 = 0, TE_WG6_3X3 = 1, TE_WG6_3X3_PAIR = 2, TE_WG6_T2_WIDE = 3, TE_WG6_T2 = 4, TE_WG6_T2_MASKED = 5, TE_WG6_1X1 = 6 };
int te_wgrad6_form(int kind, int B, int Co, int Ci, int H, int W, int NB);
/* The plan of a te_wgrad_f32 (NB = 1) / te_wgrad_group_f32 launch with S chunks per sample group (host only, nothing is launched: the
 * answer is the plan that the launch itself makes and then dispatches on).  The plan reads the kind, the dims, S, NB, the switches that
 * te_wgrad6_form reads and the two base addresses mod 16 (g_mod16, x_mod16: 0 ... 15), nothing else.
 * form[TE_WGRAD_FORM_INTS]: [0] the te_wgrad6_form code of the kernel that takes the launch - TE_WG6_FP32 also where te_wgrad6_form
 * names a split kernel but g or x is not 16-byte aligned.  The rest describes the launch of the fp32 kernel
 * wgrad_mfma_kernel<KIND, NWP, WINO> (csrc/wgrad.hip) and is all zeros when a split kernel takes the launch:
 * [1] nwp (waves along the plain operand's channels: 2 = 256 threads, 64 x 64 channels per block; 4 = 512 threads, 128 x 64)
 * [2] wino (the pair form, what te_wgrad_pair_form reports)  [3] vec (16-byte staging path)  [4] db (two LDS operand images)
 * [5] [6] TW, TH (cell tile)  [7] [8] tiles_x, tiles_y (cell tiles of one sample)  [9] [10] [11] grid x, y, z  [12] dynamic LDS bytes.
 * TE_ERR_NULL / TE_ERR_SHAPE / TE_ERR_UNSUPPORTED as the launch returns them for the same arguments (bad dims, a group size that does
 * not divide the batch, a grid too large, an image too large for a cell tile, a sample group of 2 GiB or more); a refusal leaves
 * form untouched. */
#define TE_WGRAD_FORM_INTS 13
int te_wgrad_form(int kind, int B, int Co, int Ci, int H, int W, int S, int NB, int g_mod16, int x_mod16, int* form);
int te_wgrad_f32(float* slabs, const float* g, const float* x, int kind, int B, int Co, int Ci, int H,
                 int W, int S, te_stream_t stream);
/* GROUPED form for the PLAIN (unmodulated) weight gradient of small images: NB consecutive samples share one slab
 * (slabs [B / NB][S][Co][Ci][taps]), a block walks the cell tiles of its NB samples.  te_wgrad_group_plan picks NB (a divisor
 * of B; 1 when grouping does not apply) and S.  Not for layers whose reducer needs per-sample slabs (style / demodulation
 * gradients of ModulatedConv2d): those keep te_wgrad_f32.  Replaces torch's conv2d weight gradient of the discriminator's
 * 4x4 ... 32x32 layers (model_spatial_query.py:731-798), where B slabs of 9.4 MB were the traffic. */
int te_wgrad_group_plan(int kind, int B, int Co, int Ci, int H, int W, int* NB, int* S);
int te_wgrad_group_f32(float* slabs, const float* g, const float* x, int kind, int B, int Co, int Ci, int H, int W, int S, int NB,
                       te_stream_t stream);

/* Combine slabs (SURVEY §7 step 6 "reductions for ds, dd"):
 *   gw[co,ci,t]  = wscale * sum_{b,s} osc[b,co]*isc[b,ci] * slab          (gw   may be NULL)
 *   gisc[b,ci]   = sum_{co,t,s} wscale*w[co,ci,t] * osc[b,co] * slab      (gisc may be NULL)
 *   gosc[b,co]   = sum_{ci,t,s} wscale*w[co,ci,t] * isc[b,ci] * slab      (gosc may be NULL)
 * isc / osc NULL = all ones.  All three outputs are WRITTEN.  Shares of different thread blocks (channel tiles, slab chunks,
 * samples) meet through the caller's workspace `ws` of te_wgrad_reduce_ws_floats(...) floats and a fixed-order second pass:
 * bit-reproducible, no atomics, no memset.  The launch plans once (path, counts, where each output's parts lie in `ws`) and
 * te_wgrad_reduce_ws_floats is the largest reservation over the plans a launch with the same wants (want_* = the output
 * pointer is not NULL) can take, whatever the alignment of its tensors and with or without an osc operand; a plan that would
 * carve more is refused with TE_ERR_SHAPE before anything is launched. */
int64_t te_wgrad_reduce_ws_floats(int B, int S, int Co, int Ci, int taps, int want_w, int want_isc, int want_osc);
int te_wgrad_reduce_f32(float* gw, float* gisc, float* gosc, float* ws, const float* slabs, const float* w,
                        float wscale, const float* isc, const float* osc, int B, int S, int Co, int Ci,
                        int taps, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M3  ToRGB: 1x1 modulated convolution to 3 channels (reference: ToRGB.forward, model_spatial_query.py:
 * 416-425 — grouped 1x1 F.conv2d, demodulate=False).  HBM-bound streaming kernels (x [B,K,HW] touched once):
 *   fwd   out[b,o,p] = sum_k wscale w[o,k] isc[b,k] x[b,k,p] + bias[o]   w [3,K], isc/bias may be NULL
 *   dgrad gx[b,k,p]  = wscale isc[b,k] sum_o w[o,k] g[b,o,p]
 *   wgrad slabs[b][c][o][k] = sum_{p in chunk c} g[b,o,p] x[b,k,p]       (finish with te_wgrad_reduce_f32, taps = 1)
 * te_rgb_supported: 1 if (M == 3, K <= 512, HW % 4 == 0), else use te_conv_f32(TE_CONV_1X1).
 */
int te_rgb_supported(int M, int K, int HW);
int te_rgb_fwd_f32(float* out, const float* x, const float* w, const float* isc, const float* bias, float wscale, int B,
                   int K, int HW, te_stream_t stream);
int te_rgb_dgrad_f32(float* gx, const float* g, const float* w, const float* isc, float wscale, int B, int K, int HW,
                     te_stream_t stream);
/* The same streaming form as the FORWARD of a 1x1 convolution from 3 channels (the discriminator's from-RGB stem,
 * ConvLayer(3, C, 1), model_spatial_query.py:815): out[b,k,p] = act(wscale * sum_o w[o,k] x3[b,o,p] + bias[k]),
 * w [3,K] (the [K,3] model weight transposed), bias [K] or NULL, act as te_conv_f32.  Its data gradient is te_rgb_fwd_f32,
 * its weight gradient te_rgb_wgrad_f32 with the two operands exchanged. */
int te_rgb_expand_f32(float* out, const float* x3, const float* w, const float* bias, int act, float wscale, int B, int K,
                      int HW, te_stream_t stream);
int te_rgb_wgrad_slab_count(int B, int K, int HW);
int te_rgb_wgrad_f32(float* slabs, const float* g, const float* x, int B, int K, int HW, int S, te_stream_t stream);
/* te_rgb_wgrad_f32 with a 4th slab row: slabs[b][c][3][k] = sum_{p in chunk c} x[b,k,p]  (slabs [B][S][4][K]).  With the
 * operands exchanged (g = the 3-channel image, x = the gradient of the from-RGB stem's pre-activation) rows 0-2 are the stem's
 * weight gradient and row 3 its bias gradient: one pass over the 128-channel gradient instead of two. */
int te_rgb_wgrad_sum_f32(float* slabs, const float* g, const float* x, int B, int K, int HW, int S, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * F2  attention core of the dual-space cross-attention block (reference: Attention.forward,
 * model_spatial_query.py:888-894): per sample and head,  sim = softmax(scale * q k^T),
 * o = sim v, with QK^T and sim.V on v_mfma_f32_16x16x4_f32.
 *   q [N, M, G*D], k,v [N, L, G*D] (token-major, as produced by the q/k/v linears), o [N, M, G*D],
 *   sim [N, G, M, L].  Supported: M == L == 16, D == 32 (the only shape the model produces).
 */
int te_attn_fwd_f32(float* o, float* sim, const float* q, const float* k, const float* v, float scale,
                    int N, int G, int M, int L, int D, te_stream_t stream);
int te_attn_bwd_f32(float* gq, float* gk, float* gv, const float* go, const float* gsim_or_null,
                    const float* q, const float* k, const float* v, const float* sim, float scale, int N,
                    int G, int M, int L, int D, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K2b  backward of "blur -> + bias -> leaky-ReLU * sqrt(2)" (the upsampling StyledConv tail, model_spatial_query.py:321 +
 * :401; reference backward = fused_bias_act_kernel.cu grad pass, then upfirdn2d with flipped taps) in ONE pass:
 *   gpre = g * (ref > 0 ? scale : alpha * scale)      ref = saved forward output, g / ref: [major, in_h, in_w]
 *   gx   = upfirdn2d(gpre, k, up = down = 1, pads)    k = the already flipped 4x4 taps, pads >= 0
 *   partial[plane][tile] = sum of gpre over the part of the plane the tile owns (bias gradient = sum over planes of the
 *   same channel and over tiles); te_blur_actgrad_tiles gives the tile count per plane.
 */
int te_blur_actgrad_tiles(int in_h, int in_w, int kh, int kw, int pad_x0, int pad_x1, int pad_y0, int pad_y1);
int te_blur_actgrad_f32(float* gx, float* partial, const float* g, const float* ref, const float* k, int64_t major, int in_h,
                        int in_w, int kh, int kw, int pad_x0, int pad_x1, int pad_y0, int pad_y1, float alpha, float scale,
                        te_stream_t stream);
/* K2c  the other order, backward of "conv + bias -> leaky-ReLU * scale -> blur" (first half of the discriminator's ResBlock,
 * model_spatial_query.py:744-768): the adjoint FIR first, the activation gradient in its epilogue —
 *   gx = upfirdn2d(g, k, up = down = 1, pads) * (ref > 0 ? scale : alpha * scale)    g [major, in_h, in_w],
 *   ref = the saved activation output, shaped like gx;  partial[plane][tile] = sum of the tile's gx (bias gradient).
 * Same tile count as te_blur_actgrad_tiles; in_w >= 4. */
int te_blur_gradact_f32(float* gx, float* partial, const float* g, const float* ref, const float* k, int64_t major, int in_h,
                        int in_w, int kh, int kw, int pad_x0, int pad_x1, int pad_y0, int pad_y1, float alpha, float scale,
                        te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Loop-trip queries (host only, nothing is launched; each calls the grid function of the launch it describes, and the three FIR plans
 * check their arguments with the validator of their launch).  Many kernels
 * launch fewer blocks than they have work and loop inside the block; these say how often, so that a test can assert the trips
 * it relies on (tests/loop_trips.py).
 *   te_upfirdn2d_plan / te_blur_actgrad_plan / te_blur_gradact_plan: what te_upfirdn2d_f32 / te_blur_actgrad_f32 /
 *     te_blur_gradact_f32 launch for the same arguments.  *zgroups = plane groups of the plane-walking kernels (blur44_kernel,
 *     fir_tile_kernel: the block of group pg filters the planes pg, pg + zgroups, ... < major), *tiles = tiles per plane; both 0
 *     where the direct kernel runs.
 *   te_*_cover: elements (outputs) that ONE trip of the kernel's full grid covers; a launch with more elements strides.
 *     te_upfirdn2d_direct_cover: fir_direct_kernel and the f16 / f64 entry points.  te_chan_scale_cover(rows, hw, aligned16).
 *     te_bias_act_f32_cover(size_x, step_b (0: no bias), aligned16, *vec = 1 on the 16-byte path); te_bias_act_any_cover: f16 /
 *     f64.  te_conv_finalize_cover: the split-K epilogue of te_conv_ws_f32 / te_conv_res_f32 over B M Ho Wo outputs.
 *     te_small_gemm_splitk_finish_cover: the second kernel of te_small_gemm_splitk_f32.
 *   te_conv_pack_plan: *blocks along x of a single-job te_conv_pack_weights_f32 launch, *tiles = 32 x 32 tiles of the job (a block
 *     walks the tiles blockIdx.x, blockIdx.x + *blocks, ...).
 *   te_wgrad_reduce_plan: second pass of the dW output of te_wgrad_reduce_f32 (16-byte aligned tensors): *parts partial tensors
 *     (1: no second pass), *cover elements per trip of its grid.
 * Negative TE_ERR_* on bad arguments.  The three FIR plans refuse what their launch refuses, with the launch's code (for example
 * TE_ERR_UNSUPPORTED for taps other than 4 x 4 in the two blur plans), and a launch of no planes (major == 0) with TE_ERR_SHAPE; the two
 * blur plans do not apply their launches' limits on the plane count and the plane size. */
int te_upfirdn2d_plan(int64_t major, int in_h, int in_w, int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                      int pad_x0, int pad_x1, int pad_y0, int pad_y1, int* zgroups, int* tiles);
int te_blur_actgrad_plan(int64_t major, int in_h, int in_w, int kh, int kw, int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                         int* zgroups, int* tiles);
int te_blur_gradact_plan(int64_t major, int in_h, int in_w, int kh, int kw, int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                         int* zgroups, int* tiles);
/* The plan of a FIR launch (host only, nothing is launched: the answer is the plan that the launch itself makes and then dispatches
 * on; te_upfirdn2d_plan, te_blur_actgrad_plan, te_blur_gradact_plan and te_blur_actgrad_tiles are views of the same plan).
 * op 0: te_upfirdn2d_f32, 1: te_blur_actgrad_f32, 2: te_blur_gradact_f32; the two blur ops ignore minor, up and down.
 * form[TE_FIR_FORM_INTS]: [0] the kernel (TE_FIR_*: fir_direct_kernel, blur44_kernel<MODE, D, EXT>, fir_tile_kernel<2,1,4,4>,
 * <1,2,4,4>, <1,1,4,4,AG>)  [1] [2] [3] MODE, D, EXT of blur44_kernel (0 for the other kernels)  [4] [5] ext_x, ext_y: the last tile
 * column / row also filters one more output column / row (the +1 rule)  [6] [7] rows and columns of an output tile (32 x 64 blur44,
 * 16 x 64 fir_tile, 0 x 0 direct)  [8] [9] tiles_x, tiles_y per plane  [10] zgroups (plane groups: the block of group pg filters the
 * planes pg, pg + zgroups, ... < major)  [11] grid x  [12] threads per block.  [4] ... [10] are 0 where the direct kernel runs.
 * Refuses what the launch refuses, with the launch's code (the epilogue arguments of te_upfirdn2d_f32 are not part of the plan), and a
 * launch of no planes (major == 0) with TE_ERR_SHAPE; a refusal leaves form untouched. */
enum { TE_FIR_DIRECT = 0, TE_FIR_BLUR44 = 1, TE_FIR_TILE_UP2 = 2, TE_FIR_TILE_DOWN2 = 3, TE_FIR_TILE_AG = 4 };
#define TE_FIR_FORM_INTS 13
int te_fir_form(int op, int64_t major, int in_h, int in_w, int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                int pad_x0, int pad_x1, int pad_y0, int pad_y1, int* form);
int64_t te_upfirdn2d_direct_cover(int64_t outputs);
int64_t te_chan_scale_cover(int64_t rows, int64_t hw, int aligned16);
int64_t te_bias_act_f32_cover(int64_t size_x, int64_t step_b, int aligned16, int* vec);
int64_t te_bias_act_any_cover(int64_t size_x);
int64_t te_conv_finalize_cover(int64_t outputs);
int64_t te_small_gemm_splitk_finish_cover(int I, int J);
int te_conv_pack_plan(int kind_pack, int Co, int Ci, int ksize, int* blocks, int* tiles);
int te_wgrad_reduce_plan(int B, int S, int Co, int Ci, int taps, int* parts, int64_t* cover);

/* ---------------------------------------------------------------------------------------------
 * G2/A2  small dense layers (reference: EqualLinear.forward, model_spatial_query.py:213-221 — F.linear on
 * weight * scale with bias * lr_mul, optional activation).  One fused launch on fp32 MFMA:
 *     C[i,j] = act( alpha * sum_k A(i,k) * B(k,j) + beta * bias[j] ) + residual[i,j]      C, residual, pre: [I,J] row-major
 * A(i,k) = a[i*sai + k*sak],  B(k,j) = b[k*sbk + j*sbj]  (element strides, so y = x W^T, dx = g W and dW = g^T x all map
 * onto it).  bias / residual / pre (pre-activation copy) may be NULL.  act: 0 none, 1 GELU(erf), 3 lrelu(0.2)*sqrt(2).
 * arowsum (may be NULL): arowsum[i] = rs_scale * sum_k A(i,k) — the bias gradient, for free, in the dW = g^T x call.
 */
int te_small_gemm_f32(float* c, float* pre, const float* a, const float* b, const float* bias, const float* residual,
                      float* arowsum, float rs_scale, int I, int J, int K, int64_t sai, int64_t sak, int64_t sbk,
                      int64_t sbj, float alpha, float beta, int act, te_stream_t stream);

/* the same GEMM for WIDE reductions (reference: the discriminator's EqualLinear(8192, 512, 'fused_lrelu'),
 * model_spatial_query.py:831-834): K is split into S chunks (K % S == 0, (K / S) % 8 == 0) that run as S x tiles blocks,
 * partial tiles go to the caller's workspace ws[S][I][J], a second kernel sums them in a fixed order and applies the
 * epilogue (deterministic, no atomics).  C / pre / residual are dense [I, J]. */
int te_small_gemm_splitk_f32(float* c, float* pre, float* ws, int S, const float* a, const float* b, const float* bias,
                             const float* residual, int I, int J, int K, int64_t sai, int64_t sak, int64_t sbk, int64_t sbj,
                             float alpha, float beta, int act, te_stream_t stream);

/* Which of the 20 instantiations small_gemm_kernel<NW, AV, BV> (csrc/linear.hip) a launch runs, and on which grid (host only, nothing
 * is launched: the answer is the plan that the three entry points themselves make and then dispatch on).  The plan reads the dims,
 * nz (1 for te_small_gemm_f32), the operand strides, the z strides za / zb, b_tab (NULL: the uniform form; else nz <= 16 offsets)
 * and the two base addresses mod 16 (a_mod16, b_mod16: 0 ... 15), nothing else.  splitk != 0: nz is S and K the whole reduction of
 * te_small_gemm_splitk_f32; the answer is the plan of its chunk launch (K / S per chunk, za = K / S * sak, zb = K / S * sbk; the
 * za, zb given are not read, b_tab must be NULL).
 * form[TE_SMALL_GEMM_FORM_INTS]: [0] nw (waves that split K: 1, 2, 4, 8, 16)  [1] av  [2] bv (16-byte loads of A / of B)
 * [3] [4] [5] grid x, y, z.  TE_ERR_NULL / TE_ERR_SHAPE / TE_ERR_UNSUPPORTED as the launches return them for the same arguments. */
#define TE_SMALL_GEMM_FORM_INTS 6
int te_small_gemm_form(int I, int J, int K, int nz, int64_t sai, int64_t sak, int64_t sbk, int64_t sbj, int64_t za, int64_t zb,
                       const int64_t* b_tab, int a_mod16, int b_mod16, int splitk, int* form);

/* D1  minibatch standard deviation + channel concat of the discriminator (reference: Discriminator.forward,
 * model_spatial_query.py:844-852) as one launch: with n = B / group, sample b = g * n + j belongs to set j;
 *   s_j = mean over the C*HW positions of sqrt(var_g x[g*n + j] + eps)      (biased variance over the `group` samples)
 *   y[b, :C] = x[b];  y[b, C, :] = s_{b mod n}                              x [B, C, HW], y [B, C + 1, HW]
 * backward: gx = gy[:, :C] + d s / d x * (sum of gy[:, C] over the set).  group <= 4, B % group == 0. */
int te_minibatch_stddev_fwd_f32(float* y, const float* x, int B, int group, int C, int HW, float eps, te_stream_t stream);
int te_minibatch_stddev_bwd_f32(float* gx, const float* gy, const float* x, int B, int group, int C, int HW, float eps,
                                te_stream_t stream);

/* A2  parameter-free layer norm over whole samples (reference: AttentionBlock.forward, model_spatial_query.py:924 / 931,
 * F.layer_norm(x, x.size()[1:]), eps 1e-5): x / y / g / gx are [R, N] rows; stats [R, 2] = (mean, rstd) saved for the
 * backward  gx = rstd * (g - mean(g) - y * mean(g * y)).  N % 4 == 0, N <= 16384, 16-byte aligned rows. */
int te_layer_norm_supported(int64_t R, int N);
int te_layer_norm_fwd_f32(float* y, float* stats, const float* x, int64_t R, int N, float eps, te_stream_t stream);
int te_layer_norm_bwd_f32(float* gx, const float* g, const float* y, const float* stats, int64_t R, int N, te_stream_t stream);

/* G1  PixelNorm over the channel axis of the [B, D, C] latent codes (reference: PixelNorm.forward, model_spatial_query.py:
 * 80-81, pixel_norm_op_dim = 1): y = x * rsqrt(mean_d x^2 + eps); r [B, C] = the factor, saved for the backward
 * gx = r * (g - y * mean_d(g * y)).  C must divide 256. */
int te_pixel_norm_supported(int64_t B, int D, int C);
int te_pixel_norm_fwd_f32(float* y, float* r, const float* x, int64_t B, int D, int C, float eps, te_stream_t stream);
int te_pixel_norm_bwd_f32(float* gx, const float* g, const float* y, const float* r, int64_t B, int D, int C, te_stream_t stream);

/* G2  the token-wise mapping loops (reference: Generator.forward, model_spatial_query.py:626-646 — for each of the 16
 * tokens its own EqualLinear + fused leaky-ReLU, 64 launches + 32 slice copies) as ONE launch: the same kernel batched
 * over blockIdx.z.  Operand z uses a + z*za, c + z*zc (uniform element strides) and either b + z*zb / bias + z*zbias or,
 * when the per-token parameters are separate allocations, b + b_tab[z] / bias + bias_tab[z] (host arrays of nz <= 16
 * element offsets, NULL for the uniform form).  C(i,j) = c[i*sci + j*scj], so the result can be written straight into the
 * [B, tokens, D] or [B, D, tokens] layout the next stage reads.  No pre / residual / row sums in this form. */
int te_small_gemm_batched_f32(float* c, const float* a, const float* b, const float* bias, int nz, int64_t za, int64_t zc,
                              int64_t zb, int64_t zbias, const int64_t* b_tab, const int64_t* bias_tab, int I, int J, int K,
                              int64_t sai, int64_t sak, int64_t sbk, int64_t sbj, int64_t sci, int64_t scj, float alpha,
                              float beta, int act, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M1  demodulation coefficients (reference: ModulatedConv2d.forward, model_spatial_query.py:300-304 —
 * rsqrt(sum (scale * W * style)^2 + 1e-8) over B materialised weight copies).  Shared-weight form:
 *   wsq[co,ci] = wscale^2 sum_t w[co,ci,t]^2            (output, kept for the backward)
 *   d[b,co]    = rsqrt(sum_ci s[b,ci]^2 wsq[co,ci] + eps)
 * backward, u = -gd d^3 / 2:  gw[co,ci,t] = 2 wscale^2 w sum_b u[b,co] s[b,ci]^2,  gs[b,ci] = 2 s sum_co u[b,co] wsq[co,ci]
 * T == 0 in the forward: `w` already IS wsq[Co,Ci] (kept by the host for frozen weights), wsq output unused (may be NULL).
 * (gw / gs may be NULL; B <= 64 in the backward).  w [Co,Ci,T], s [B,Ci], d / gd [B,Co].  accumulate != 0: the results are
 * ADDED to gw / gs (which then hold the convolution's own dW / d style from te_wgrad_reduce_f32).
 */
int te_demod_fwd_f32(float* d, float* wsq, const float* w, const float* s, float wscale, float eps, int B, int Co, int Ci,
                     int T, te_stream_t stream);
int te_demod_bwd_f32(float* gw, float* gs, const float* gd, const float* d, const float* w, const float* wsq,
                     const float* s, float wscale, int B, int Co, int Ci, int T, int accumulate, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * T2  multi-tensor optimiser kernels: ONE launch over every parameter tensor of a module (reference:
 * train_spatial_query.py:458-473 — two torch.optim.Adam over 257 / 38 tensors — and accumulate(), :56-61, the
 * g_ema update; hundreds of tiny launches per iteration there).
 * The tensors are described by DEVICE tables:
 *   te_mt_adam_f32: table[5][n] (int64) = param ptr, grad ptr (0 = no gradient: tensor skipped), exp_avg ptr,
 *                   exp_avg_sq ptr, numel;  te_mt_ema_f32: table[3][n] = dst ptr, src ptr, numel;
 *   chunks[2][n_chunks] (int32) = tensor index, chunk index within the tensor; chunk c covers elements
 *   [chunk_index * chunk_elems, +chunk_elems) of its tensor (chunk_elems % 4 == 0).
 * Adam (no weight decay, no amsgrad), same operation order as torch.optim.Adam:
 *   m = lerp(m, g, 1 - beta1);  v = beta2 v + (1 - beta2) g^2;  p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 *   (beta1 == 0, the reference's setting: m is written (= g) but never read).  Hyper-parameters arrive as doubles (the
 *   bias corrections are formed in double on the host, as torch does) and are applied in fp32.
 * EMA: dst = dst * decay + (1 - decay) * src.
 */
int te_mt_adam_f32(const int64_t* table, const int32_t* chunks, int n_tensors, int n_chunks, int chunk_elems, double lr,
                   double beta1, double beta2, double eps, int step, te_stream_t stream);
int te_mt_ema_f32(const int64_t* table, const int32_t* chunks, int n_tensors, int n_chunks, int chunk_elems, double decay,
                  te_stream_t stream);
/* Ranger = RAdam + Lookahead + gradient centralisation (reference pSp/training/ranger.py:79-165, the encoder's optimiser,
 * pSp/training/coach_new.py:225-233; one parameter at a time and about fifteen element-wise launches each there).
 *   table[7][n] (int64) = param ptr, grad ptr (0 = no gradient: tensor skipped), exp_avg ptr, exp_avg_sq ptr, slow_buffer ptr,
 *                         numel, L.  L = numel / shape[0] where the reference centralises the gradient (ranger.py:118-119: the mean
 *                         over every dim but the first is subtracted), 0 where it does not.
 *   work[3][n_work] (int32) = tensor index, first row, row count: a block owns whole rows of L elements (L == 0: "rows" of
 *                         tile_elems elements, no mean).  Rows of L <= tile_elems come in groups of at most tile_elems elements;
 *                         a longer row is an entry of its own.  Every row of a tensor must be in exactly one entry.
 * Per element, fp32, one rounding per operation (ranger.py:118-163):  g' = g - mean(row);  v = v beta2 + (1 - beta2) g' g';
 *   m = m beta1 + (1 - beta1) g';  decay != 0: p += -decay p;  rectified: p += -step_lr m / (sqrt(v) + eps), else p += -step_lr m;
 *   lookahead: slow += alpha (p - slow), p = slow (slow_buffer is neither read nor written otherwise).  p.grad is not modified.
 * The schedule is the caller's: step_lr = step_size * lr and decay = weight_decay * lr are formed in double on the host, as are
 * the two branch flags.  A row's sum is a fixed function of L and the element index (the order: csrc/optim.hip), so results do not
 * depend on alignment, on the work map's grouping, or on the other tensors.  16-byte accesses where every pointer of the tensor
 * sits at the same offset inside its 16 bytes.  tile_elems: a multiple of 4, 2048 <= tile_elems <= 8184; 0 <= beta < 1, eps > 0,
 * 0 <= alpha <= 1, else TE_ERR_SHAPE and nothing is launched. */
int te_mt_ranger_f32(const int64_t* table, const int32_t* work, int n_tensors, int n_work, int tile_elems, double step_lr,
                     double decay, double beta1, double beta2, double eps, double alpha, int rectified, int lookahead,
                     te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Per-(sample, channel) scaling of an activation tensor and its adjoint: the elementwise pieces of the any-order composite
 * of the modulated convolution (style scale on the input, demodulation on the output: model_spatial_query.py:299-304 moved
 * from B weight copies onto the activations), used when a backward pass is recorded (path-length regulariser).
 *   te_chan_scale_f32: out[r, j] = x[r, j] * s[r]           rows r = (sample, channel), hw pixels each
 *   te_chan_dot_f32  : out[r]    = sum_j a[r, j] * b[r, j]   (fixed summation order)
 */
int te_chan_scale_f32(float* out, const float* x, const float* s, int64_t rows, int64_t hw, te_stream_t stream);
int te_chan_dot_f32(float* out, const float* a, const float* b, int64_t rows, int64_t hw, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * L1  LPIPS-VGG perceptual distance (utils/lpips/__init__.py:12-39, networks_basic.py:21-87, pretrained_networks.py:98-136), the
 * pieces the convolution family does not cover (conv1_2 ... conv5_3 run as TE_CONV_3X3 / 3X3W / 3X3W6 with the bias in the epilogue
 * and ReLU as te_bias_act_f32 with alpha 0).  NCHW fp32 throughout.
 *
 * Stem: ScalingLayer (x - shift) / scale, shift (-.030, -.088, -.188), scale (.458, .448, .450), applied BEFORE the zero padding of
 * conv1_1 (nn.Conv2d(3, 64, 3, padding=1) on the scaled tensor), then bias and ReLU:
 *     out[n,o] = relu(b[o] + sum_{c,ky,kx} w[o,c,ky,kx] * s(x)[n,c,y+ky-1,x+kx-1])        w [64,3,3,3] (torchvision layout), b [64]
 * te_lpips_stem_dgrad_f32: the data gradient with the relu1_1 mask (y1 = the stem output) and the 1/scale fold:
 *     gx[n,c] = (1/scale[c]) * sum_{o,ky,kx} w[o,c,ky,kx] * (g * (y1 > 0))[n,o,y+1-ky,x+1-kx]
 */
int te_lpips_stem_fwd_f32(float* out, const float* x, const float* w, const float* b, int N, int H, int W, te_stream_t stream);
int te_lpips_stem_dgrad_f32(float* gx, const float* g, const float* y1, const float* w, int N, int H, int W, te_stream_t stream);
/* 2x2 / stride 2 max-pool (pretrained_networks.py: features[4, 9, 16, 23] = nn.MaxPool2d(2, 2)) over `planes` = N * C planes of
 * H x W (both even).  Window order row-major; torch's rule: an element replaces the running maximum if it is greater OR NaN (the
 * first of equal maxima wins, a NaN propagates).  The backward recomputes the window's index from x and writes ALL of gx (the
 * gradient at the index, 0 elsewhere; no zero fill needed). */
int te_maxpool2_fwd_f32(float* out, const float* x, int64_t planes, int H, int W, te_stream_t stream);
int te_maxpool2_bwd_f32(float* gx, const float* g, const float* x, int64_t planes, int H, int W, te_stream_t stream);
/* LPIPS head of one layer (networks_basic.py:65-73: normalize_tensor (utils/lpips/__init__.py:43-45), (f0 - f1)^2, lin = 1x1 conv
 * without bias (NetLinLayer, :99-108), spatial_average (:12-13)).
 *   te_lpips_normalize_f32: out = x / (sqrt(sum_c x^2) + 1e-10)   (normalise-only mode: the cached target features)
 *   te_lpips_head_fwd_f32 : partial[n, j] = sum over the j-th block of 256 pixels of sum_c w[c] (f[n,c,p] / (|f[n,:,p]| + 1e-10)
 *                           - t[nt,c,p])^2, j < te_lpips_head_blocks(HW); t are NORMALISED target features of batch Nt = N or 1
 *                           (nt = 0: one target broadcast over the pred batch, as the projector's --batch > 1 relies on)
 *   te_lpips_dist_f32     : d[n] = sum_{l < L} (sum_j partial_l[n, j]) / hw[l], layers in order (the reference's val += res[l]);
 *                           partial / hw are HOST arrays of L <= 8 entries
 *   te_lpips_head_bwd_f32 : gradient w.r.t. f given gd[N] (the gradient of d): with r = |f[n,:,p]|, u_c = 2 w_c (f_c / (r + eps)
 *                           - t_c) gd[n] / HW,
 *                               gf = u / (r + eps) - f (f . u) / (r (r + eps)^2)
 *                           then gf += gin (may be NULL: the max-pool gradient arriving at the same tap) and, if relu_mask, gf = 0
 *                           where f <= 0 (the tap is a ReLU output).  DEVIATION: at a pixel whose feature vector is exactly zero,
 *                           torch autograd of the reference formula gives NaN (sqrt backward 0/0); here the second term is 0 at r = 0,
 *                           so gf = u / eps there, the finite limit.
 * Fixed-order reductions only (per-block tree, then a sequential sum over blocks and layers): bit-reproducible. */
int te_lpips_normalize_f32(float* out, const float* x, int N, int C, int64_t HW, te_stream_t stream);
int te_lpips_head_blocks(int64_t HW);
int te_lpips_head_fwd_f32(float* partial, const float* f, const float* t, const float* w, int N, int Nt, int C, int64_t HW,
                          te_stream_t stream);
int te_lpips_dist_f32(float* d, const float* const* partial, const int64_t* hw, int L, int N, te_stream_t stream);
int te_lpips_head_bwd_f32(float* gf, const float* gin, const float* gd, const float* f, const float* t, const float* w, int N, int Nt,
                          int C, int64_t HW, int relu_mask, te_stream_t stream);
/* Paired head, forward only (metrics/evaluate_query.py:234-236: percept(image[::2], image[1::2]); replaces networks_basic.py:65-73 for
 * both images of a pair at once).  f [2N, C, HW]: the tap activations of an interleaved batch, images 2n and 2n+1 are a pair.
 *     partial[n, j] = sum over the j-th block of 256 pixels of
 *                     sum_c w[c] (f[2n,c,p] / (|f[2n,:,p]| + 1e-10) - f[2n+1,c,p] / (|f[2n+1,:,p]| + 1e-10))^2,  j < te_lpips_head_blocks(HW)
 * (the split of te_lpips_head_fwd_f32, so te_lpips_dist_f32 reduces the partials unchanged).  Both sides are normalised in the
 * kernel; no normalised tensor is written.  Each side's f * inv is rounded before the subtraction (no contraction) and the difference
 * is formed before squaring, so an identical pair gives exactly 0.  The channel loop is split over the block (CG = 4 slices for
 * HW >= 256, up to 16 for HW <= 64); a pixel's squared norm is summed in fp64 (slice sums added in slice order) and 1 / (norm + eps)
 * rounded to fp32 once, so it may differ from te_lpips_head_fwd_f32's fp32 chain in the last bit: at PPL's scale (sides 1e-4 apart)
 * the norm's error is the largest term of the result's.  Fixed-shape reductions, no atomics: bit-reproducible. */
int te_lpips_pair_head_fwd_f32(float* partial, const float* f, const float* w, int N, int C, int64_t HW, te_stream_t stream);
/* Crop + bilinear resize to the LPIPS input (metrics/evaluate_query.py:222-232: image[:, :, 3c:7c, 2c:6c], then
 * F.interpolate(size=(256, 256), mode='bilinear', align_corners=False) when the factor exceeds 1).
 *     out [B,3,h,w] from the window [y0:y0+hc, x0:x0+wc] of img [B,3,H,W] (contiguous; the window is read in place), hc = fy * h,
 *     wc = fx * w with integer fy, fx >= 1; per axis: src = f * (i + 0.5) - 0.5, taps floor(src) and the next sample inside the
 *     window, weights 1 - frac and frac, x mixed first, then y (torch's upsample_bilinear2d).  f = 1 is a windowed copy. */
int te_crop_resize_bilinear_f32(float* out, const float* img, int B, int H, int W, int y0, int x0, int hc, int wc, int h, int w,
                                te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * L2  noise regulariser of the projector (projector_optimization.py:21-49) over a whole list of n <= 32 noise maps [B,1,s,s]
 * (maps / sizes / grads are HOST arrays of device pointers and sizes; s a power of two or <= 8):
 *   te_noise_reg_fwd_f32  : loss[0] = sum over maps, and over scales s, s/2, ... down to the first <= 8, of
 *                           mean(n * roll(n,1,dims=3))^2 + mean(n * roll(n,1,dims=2))^2, the next scale being the 2x2 mean
 *                           (reshape + mean([3, 5])); ONE block in the reference's summation order.  `ws` (te_noise_reg_ws_floats) keeps
 *                           the per-scale means and the downsampled maps for the backward
 *   te_noise_reg_bwd_f32  : grads[i] = gloss[0] * d loss / d map i (written, one block per map); `tws` is a second workspace of the
 *                           same size; `ws` as the forward left it
 *   te_noise_normalize_f32: in place, map = (map - mean) / std, std unbiased over the whole map (noise_normalize_, :44-49)
 */
int64_t te_noise_reg_ws_floats(const int* sizes, int n, int B);
int te_noise_reg_fwd_f32(float* loss, float* ws, float* const* maps, const int* sizes, int n, int B, te_stream_t stream);
int te_noise_reg_bwd_f32(float* const* grads, float* tws, const float* gloss, const float* ws, float* const* maps, const int* sizes,
                         int n, int B, te_stream_t stream);
int te_noise_normalize_f32(float* const* maps, const int* sizes, int n, int B, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M1  precision / recall / density / coverage (metrics/prdc.py) of two feature sets x [N,D] (real) and y [M,D] (fake), fp32 row-major.
 * Every comparison is made on SQUARED distances
 *     d2(i,j) = max(nx[i] + ny[j] - 2 dot(x_i, y_j), 0),      nx / ny = the fp32 squared row norms,
 * with the dot product on the fp32-input MFMA (one fp32 fma chain in a fixed order of k, so dot(a, b) == dot(b, a) bit for bit).  No
 * N x M matrix is ever written: the reductions run in the epilogue of the 128 x 128 GEMM tile, per-tile partials go to the caller's
 * workspace and a second fixed-order kernel combines them.  No atomics; bit-reproducible.  Any D >= 1 (the k tail is zero-filled; the
 * 16-byte load path needs D % 4 == 0 and 16-byte aligned bases, anything else takes scalar loads), 1 <= k <= 15.
 *   te_prdc_ws_bytes   : bytes of workspace that serve te_prdc_knn_f32 on N rows, on M rows, and te_prdc_counts_f32 on N x M:
 *                        O((N + M) * number of 128-wide tile columns); negative on bad arguments
 *   te_row_sqnorm_f32  : out[i] = sum_k x[i,k]^2
 *   te_prdc_knn_f32    : r2[i] = element k of the ascending row {d2(i,j) : j < N} of the set against itself, the diagonal forced to
 *                        exactly 0 (prdc.py:41-51: the k+1 smallest of pairwise_distances(X, X), whose diagonal sklearn zeroes);
 *                        duplicates count separately.  N >= k + 1
 *   te_prdc_counts_f32 : col_count[j] = #{i : d2(i,j) < rr2[i]}   (prdc.py:75-78 as > 0: precision; :85-88: density)
 *                        row_any[i]   = any_j d2(i,j) < rf2[j]    (:80-83: recall)
 *                        row_min[i]   = min_j d2(i,j)             (:90-93: coverage, against rr2[i])
 *                        rr2 [N] / rf2 [M]: the squared radii of the real / fake set; both comparisons strict.  col_count and
 *                        row_any are int32.
 */
int64_t te_prdc_ws_bytes(int N, int M, int D, int k);
int te_row_sqnorm_f32(float* out, const float* x, int N, int D, te_stream_t stream);
int te_prdc_knn_f32(float* r2, const float* x, const float* nx, int N, int D, int k, void* ws, te_stream_t stream);
int te_prdc_counts_f32(int32_t* col_count, int32_t* row_any, float* row_min, const float* x, const float* nx, const float* rr2,
                       const float* y, const float* ny, const float* rf2, int N, int M, int D, void* ws, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M2  the VGG16 fc7 feature extractor of the PRDC metric (metrics/calc_prdc.py:101-104: torchvision vgg16 with classifier[:-1] on the
 * generator's [-1, 1] image, i.e. the 4096-d output of fc7 after its ReLU).  conv1_2 ... conv5_3 and the max-pools are L1's; here the
 * three pieces L1 does not have.  Forward only (the metric runs under no_grad in eval mode: Dropout is the identity).
 *
 * te_vgg_stem_fwd_f32 (calc_prdc.py:101-104; replaces torchvision vgg16.features[0:2] = Conv2d(3, 64, 3, padding=1) + ReLU): the kernel
 * of te_lpips_stem_fwd_f32 without the ScalingLayer, the raw input straight into conv1_1:
 *     out[n,o] = relu(b[o] + sum_{c,ky,kx} w[o,c,ky,kx] * x[n,c,y+ky-1,x+kx-1])            w [64,3,3,3], b [64], x zero outside the image
 *
 * te_adaptive_avgpool_f32 (calc_prdc.py:101-104; replaces torchvision vgg16.avgpool = AdaptiveAvgPool2d((7, 7)) and the flatten
 * behind it): over `planes` = N * C planes of H x W, torch's rule per axis: output o averages the window
 * [floor(o * H / OH), ceil((o + 1) * H / OH)), summed row-major in fp32 and divided by the window's element count.  out is
 * [planes, OH * OW] contiguous: for N x 512 planes and 7 x 7 that IS the flattened [N, 25088] layout fc6 reads.  Any H, W >= 1
 * (H < OH: windows repeat; H == OH: a bit-exact copy).
 *
 * te_fc_stream_f32 (calc_prdc.py:101-104; replaces torchvision vgg16.classifier[0:2] and [3:5] = Linear + ReLU): a weight-streaming
 * dense layer for FEW rows against a weight far larger than the caches (fc6: 25088 -> 4096, 411 MB):
 *     C[i,j] = act(sum_k A[i,k] * W[j,k] + bias[j])     A [I,K], W [J,K] (torch Linear layout), C [I,J] row-major; act 0 none, 1 ReLU
 * on the fp32-input MFMA (exact fp32).  A workgroup owns 64 output columns, up to 64 rows and one of S chunks of K: every weight
 * element is loaded once per 64-row block, 16 bytes at a time along K; A is re-read from cache.  The partial tiles go to the caller's
 * workspace ws[S][I][J] (te_fc_stream_ws_bytes), a second kernel sums them over s ascending and applies bias and activation: no
 * atomics, bit-reproducible.  S = te_fc_stream_splits(J, K) depends on (J, K) ONLY and a row's summation order does not depend on I,
 * so a row's result is bitwise the same whatever batch it is in.  Any I >= 1, J >= 1; K >= 4, K % 4 == 0 and 16-byte aligned a / w,
 * anything else is TE_ERR_SHAPE.  te_fc_stream_splits / te_fc_stream_ws_bytes return a negative TE_ERR_* on bad arguments.
 */
int te_vgg_stem_fwd_f32(float* out, const float* x, const float* w, const float* b, int N, int H, int W, te_stream_t stream);
int te_adaptive_avgpool_f32(float* out, const float* x, int64_t planes, int H, int W, int OH, int OW, te_stream_t stream);
int te_fc_stream_splits(int J, int K);
int64_t te_fc_stream_ws_bytes(int64_t I, int J, int K);
int te_fc_stream_f32(float* c, float* ws, const float* a, const float* w, const float* bias, int64_t I, int J, int K, int act,
                     te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M3  the feature moments behind the Frechet inception distance, streamed in fp64 on the device.  The FID needs no features, only
 * n, s = sum_k x_k and S = sum_k x_k x_k^T, which add across batches, calls and ranks.
 *
 * te_fid_moments_f64 (metrics/fid_query.py:38-40 and :162-163, metrics/calc_inception.py:69-71 and :110-111; replaces the per-batch
 * feat.to('cpu'), the torch.cat of all features on the host and the sums inside np.mean / np.cov): x [N,D] fp32 row-major on the
 * device (4-byte alignment suffices: the 16-byte load path needs D % 4 == 0 and a 16-byte aligned base, anything else takes scalar
 * loads), S [D,D] and s [D] fp64:
 *     S[i][j] (+)= sum_k x[k][i] * x[k][j]   for j >= i        s[j] (+)= sum_k x[k][j]
 * accumulate 0 overwrites, 1 adds to what is there.  ONLY THE UPPER TRIANGLE (j >= i) of S is defined afterwards.  The products run
 * on v_mfma_f64_16x16x4_f64 over 64 x 64 tiles with tj >= ti; every fp32 x fp32 product is exact in fp64, only the sums round.  For
 * small D the sample index is split and the partial tiles go to ws, combined in split order by a second kernel: no atomics, one
 * owner and one summation order per element, bit-reproducible.  1 <= D <= 8192, N >= 1.
 *
 * te_fid_moments_ws_bytes: the bytes of ws for (N, D); 0 where the sample index is not split (ws may then be NULL); negative on
 * bad arguments.  At most (2048 + T) * 32 KiB + 64 * (D + 63) bytes with T = the number of upper 64 x 64 tiles.
 *
 * te_fid_finalize_f64 (fid_query.py:162-163, calc_inception.py:110-111; replaces np.mean(features, 0) and
 * np.cov(features, rowvar=False)): mean = s / n, cov[i][j] = cov[j][i] = (S[i][j] - s[i] s[j] / n) / (n - 1) read from the upper
 * triangle of S (ddof = 1); both triangles of cov are written.  TE_ERR_SHAPE for n < 2.
 */
int64_t te_fid_moments_ws_bytes(int64_t N, int D);
int te_fid_moments_f64(double* S, double* s, void* ws, const float* x, int64_t N, int D, int accumulate, te_stream_t stream);
int te_fid_finalize_f64(double* mean, double* cov, const double* S, const double* s, int64_t n, int D, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * E1  the linear C-SVC behind an editing boundary (our_interfaceGAN/train_boundary.py), from the training rows on.  The reference
 * copies the rows to the host and calls sklearn's SVC(kernel='linear'), which is libsvm's SMO on the CPU; here the Gram matrix, the
 * solve and the weight vector stay on the device.
 *
 * te_gram_f32 (train_boundary.py:113-114; replaces libsvm's Kernel::k_function / SVC_Q::get_Q rows behind clf.fit): K [n,n] = x x^T
 * for row-major x [n,D], on the fp32-input MFMA with fp32 accumulation (libsvm's kernel cache, Qfloat, is fp32 too).  Only the
 * 128 x 128 tiles with tj >= ti are computed and every element is written to both triangles, so K[i][j] and K[j][i] are the same
 * bits.  One owner and one summation order per element, no atomics.  1 <= n <= 4194304, any D >= 1 (the k tail is zero-filled; the
 * 16-byte load path needs D % 4 == 0 and a 16-byte aligned base, anything else takes scalar loads).
 *
 * te_svm_smo_f64 (train_boundary.py:113-114; replaces libsvm's Solver::Solve behind clf.fit): the C-SVC dual
 *     min 1/2 a^T Q a - e^T a,   0 <= a_t <= C,   y^T a = 0,   Q_ij = y_i y_j K_ij
 * by libsvm's SMO WITHOUT shrinking: second-order working-set selection (i = argmax of -y_t G_t over I_up; j = argmin over I_low
 * with b = Gmax + y_t G_t > 0 of -b^2 / a, a = K_ii + K_tt - 2 K_it, a <= 0 replaced by 1e-12), libsvm's two-variable update with
 * its clipping order for y_i != y_j and y_i == y_j, G += Q_i da_i + Q_j da_j, stop when Gmax - Gmin < eps.  rho is libsvm's
 * calculate_rho on the final state: the mean of y_t G_t over the free variables (0 < a_t < C), or (ub + lb) / 2 of the two bound
 * sets where there is none; the decision function is sum_t a_t y_t K(x_t, x) - rho.  K [n,n] fp32 (te_gram_f32's; only rows are
 * read), alpha [n] and rho [1] fp64, info [2] int32: info[0] = the iterations (updates) run, info[1] = 1 if the stop criterion was
 * met, 0 if max_iter ended the solve (alpha is feasible either way).
 * y is a HOST array of n labels, each +1 or -1: it is validated on the host and reaches the kernel as kernel arguments.
 * ONE workgroup: gradient and alpha in fp64 registers of fixed owner threads, labels and the fp32 diagonal in LDS, two rows of K read
 * per iteration.  Ties in both selections go to the lowest index (libsvm keeps the highest), so the result is bit-reproducible.
 * LIMIT: 2 <= n <= 8192 (the reference's default, 150 000 samples at ratio 0.02 and split 0.7, needs n = 4200) with both labels
 * present, C > 0, eps > 0, max_iter >= 0; anything else is TE_ERR_SHAPE and nothing is launched.
 *
 * te_svm_coef_f32 (train_boundary.py:138; replaces classifier.coef_): w[d] = sum_i alpha_i y_i x[i,d], accumulated in fp64 over i
 * ascending by one owner thread per d and rounded once to fp32 (rows with alpha_i == 0 are passed over: they add an exact zero).
 * y as above (HOST); 1 <= n <= 8192, D >= 1.  The un-normalised coef_; the caller divides by its norm.
 */
int te_gram_f32(float* K, const float* x, int n, int D, te_stream_t stream);
int te_svm_smo_f64(double* alpha, double* rho, int32_t* info, const float* K, const int8_t* y, int n, double C, double eps,
                   int64_t max_iter, te_stream_t stream);
int te_svm_coef_f32(float* w, const float* x, const double* alpha, const int8_t* y, int n, int D, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M4  the Inception-v3 pool3 extractor of the FID (metrics/inception.py:16-163 InceptionV3 with use_fid_inception=True and
 * output_blocks=[3], built by metrics/calc_inception.py:55 and metrics/fid_query.py:86): a general forward convolution and the small
 * layers around it.  Forward only, NCHW fp32.  The final global average is te_adaptive_avgpool_f32 with OH = OW = 1.
 *
 * te_conv2d_f32 (inception.py:175-190; replaces every torchvision BasicConv2d of the network = Conv2d(bias=False) +
 * BatchNorm2d(eps=0.001) in eval mode + ReLU, the batch norm folded into w and bias by the caller, and the torch.cat at
 * inception.py:215, :243, :259, :267, :276, :292, :300, :310 and in torchvision's InceptionB / InceptionD):
 *     out[b, c0 + m, oy, ox] = act(bias[m] + sum_{c,ky,kx} w[m,c,ky,kx] * x[b, c, oy*s + ky - py, ox*s + kx - px])      x = 0 outside
 * x [B,Ci,H,W]; w [Co,Ci,kh,kw] (torch layout, read as it is: no packed form); bias [Co]; out is the channel slice [c0, c0 + Co) of a
 * contiguous [B,Ctot,Ho,Wo] tensor, Ho = (H + 2 py - kh) / s + 1 (floor), Wo likewise; act 0 none, 1 ReLU (a NaN propagates).
 * s = 1 or 2 and act = 0 or 1 (else TE_ERR_UNSUPPORTED), 1 <= kh, kw <= 7 (else TE_ERR_UNSUPPORTED), 0 <= py < kh, 0 <= px < kw,
 * Ho, Wo >= 1, 0 <= c0, c0 + Co <= Ctot, any B, Ci, Co, H, W >= 1 with Ci * H * W, Ci * kh * kw and Ho * Wo below 2^31 (else
 * TE_ERR_SHAPE); nothing is launched on a refusal.  An implicit GEMM on v_mfma_f32_32x32x2_f32, exact fp32: M = Co, N = the
 * B * Ho * Wo pixels flattened across the batch, K = Ci * kh * kw; the patch is gathered into LDS on the fly (no im2col tensor, no
 * workspace).  K is NOT split: each output element has one owner and is one fp32 fma chain over k in a fixed permutation that
 * depends on K only, never on B or on the tile, so an image's outputs are bitwise the same whatever batch it is in.  No atomics.
 *
 * te_pool3_f32 (inception.py:89, :98 nn.MaxPool2d(3, 2) and torchvision's InceptionB / InceptionD pool branch; inception.py:306
 * F.max_pool2d(x, 3, 1, 1); inception.py:210, :238, :271 F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)): 3 x 3 windows over
 * x [B,C,H,W] into the slice [c0, c0 + C) of a contiguous [B,Ctot,Ho,Wo] tensor.  mode 0: max, stride 2, no padding, floor
 * (Ho = (H - 3) / 2 + 1; H, W >= 3); mode 1: max, stride 1, pad 1, the padding never wins; mode 2: average, stride 1, pad 1, summed
 * row-major in fp32 and divided by the number of taps inside the image.  Max follows te_maxpool2_fwd_f32's rule: a greater value or
 * a NaN replaces.
 *
 * te_resize_bilinear_f32 (inception.py:147-150; replaces F.interpolate(size, mode='bilinear', align_corners=False)): planes of H x W
 * to OH x OW, any sizes up to 2^22, up- and downscaling, no antialiasing.  Per axis src = max((in / out) * (o + 0.5) - 0.5, 0), taps
 * floor(src) and the next sample inside the image, weights l1 = src - floor(src), l0 = 1 - l1; x is mixed first, then y, as
 * te_crop_resize_bilinear_f32 does.  src is evaluated exactly, as (in * (2 o + 1) - out) / (2 out) in integers (torch's fp32
 * coordinate is off by up to in * 2^-23 of a sample); equal sizes give a bit-exact copy.  1 <= planes <= 65535.
 */
int te_conv2d_f32(float* out, const float* x, const float* w, const float* bias, int B, int Ci, int Co, int H, int W, int kh, int kw,
                  int s, int py, int px, int Ctot, int c0, int act, te_stream_t stream);
int te_pool3_f32(float* out, const float* x, int B, int C, int H, int W, int mode, int Ctot, int c0, te_stream_t stream);
int te_resize_bilinear_f32(float* out, const float* x, int64_t planes, int H, int W, int OH, int OW, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M5  the two ends of the DEX age / gender scorer of attribute editing (our_interfaceGAN/ffhq_utils/dex/models.py:27-69: a VGG16 whose
 * last layer has 101 or 2 classes; ffhq_utils/dex/api.py:42-65; called from edit_all_noinversion_ffhq.py:113-131).  conv1_2 ...
 * conv5_3 and the max-pools are L1's, the two hidden fc layers are M2's te_fc_stream_f32; here the input and the output end.
 * Forward only (the scorer runs under no_grad in eval mode: Dropout is the identity).
 *
 * te_dex_stem_fwd_f32 (edit_all_noinversion_ffhq.py:113-116, api.py:47-65, models.py:11-12; replaces the channel flip, the
 * clamp / add / div / mul / round chain, the centre crop and Conv2d(3, 64, 3, padding=1) + ReLU): img [N,3,H,W] RGB, nominally in
 * [-1, 1]; w [64,3,3,3], b [64]; out [N,64,crop,crop].  With y0 = (H - crop) / 2, x0 = (W - crop) / 2 and
 *     v(t) = rint(((clamp(t, -1, 1) + 1) * 0.5) * 255)        each step rounded to fp32, ties to even: torch's result bit for bit
 *     out[n,o,y,x] = relu(b[o] + sum_{c,ky,kx} w[o,c,ky,kx] * v(img[n, 2 - c, y0 + y + ky - 1, x0 + x + kx - 1]))
 * where a tap with y + ky - 1 or x + kx - 1 outside [0, crop) is ZERO: the padding is that of the crop, image pixels outside the
 * window are never read.  A NaN pixel stays a NaN (torch's clamp) and a NaN propagates through the ReLU.  TE_ERR_SHAPE, nothing
 * launched, for crop < 1, crop > H or W, an odd H - crop or W - crop, or N >= 65536.  Deviation from the reference: api.py:50-52 slices
 * offset:-offset, which is empty at H == 224 and one pixel too large for an odd difference; an odd difference is refused here.
 *
 * te_cls_score_f32 (models.py:55-56 and api.py:42-44, :56-58, :64; replaces cls = nn.Linear, F.softmax(dim=1), the arange(1, 102)
 * weighting with its sum, and the [:, 0] slice): a [I,K], w [C,K] (torch Linear layout), bias [C]:
 *     p[i,:] = softmax(a[i,:] @ w.T + bias)     in fp32, the row maximum subtracted
 *     score[i] = sum_c (c + 1) * p[i,c]  (mode 0; the reference's weights start at 1)      score[i] = p[i,0]  (mode 1)
 * prob [I,C] receives p, or is NULL.  Shaped for latency: one workgroup per row, its waves split the classes, the lanes stride K with
 * 16-byte loads; all reductions are fixed-shape trees, no atomics; a row's result is bitwise independent of I.  1 <= C <= 1024,
 * K >= 4, K % 4 == 0, 16-byte aligned a and w, I >= 1, anything else is TE_ERR_SHAPE; another mode is TE_ERR_UNSUPPORTED; nothing is
 * launched on a refusal.
 */
int te_dex_stem_fwd_f32(float* out, const float* img, const float* w, const float* b, int N, int H, int W, int crop, te_stream_t stream);
int te_cls_score_f32(float* score, float* prob, const float* a, const float* w, const float* bias, int64_t I, int C, int K, int mode,
                     te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M6  the CelebA-HQ attribute classifier of attribute editing (our_interfaceGAN/celebahq_utils/dex/networks/classifiers/
 * attribute_classifier.py:152-215: D with fixed_size=True, use_mbstd=False, a progressive-GAN discriminator with one logit per
 * attribute; attribute_utils.py:8-60; called from edit_all_noinversion_celebahq.py:175-182).  Its 3x3 convolutions are F1's with bias
 * and act 4 (conv0, the 4x4 convolution) or act 0 (conv1), dense0 is M2's te_fc_stream_f32; here the input end, the downscale between
 * the blocks and the output end.  Forward only (the classifier runs under no_grad in eval mode), NCHW fp32, no atomics.  The constant
 * scales of the equalised learning rate (WScaleLayer, attribute_classifier.py:11-33) are folded into the weights by the caller.
 *
 * te_attr_stem_fwd_f32 (edit_all_noinversion_celebahq.py:175-177, attribute_utils.py:8-19, attribute_classifier.py:62-71, :201;
 * replaces the channel flip, the clamp / add / div / mul / round chain, the view + mean(dim=[3, 5]) box filter and fromrgb_lod0 =
 * Conv2d(3, C0, 1) * scale + bias + LeakyReLU(0.2)): img [N,3,S,S], w [C0,3] (scaled), b [C0], out [N,C0,R,R], f = S / R.
 *     preprocessed = 0: img is RGB, nominally in [-1, 1]:  v[n,c] = rint(((clamp(img[n, 2 - c], -1, 1) + 1) * 0.5) * 255), each step
 *                       rounded to fp32, ties to even: torch's result bit for bit (the chain of te_dex_stem_fwd_f32)
 *     preprocessed = 1: img is what the editing scripts hand over, BGR byte levels:  v[n,c] = img[n,c]
 *     m_c[y,x] = (sum over the f x f block at (f y, f x) of v[n,c], row-major in fp32, starting from 0) / (f * f)       (= v at f == 1)
 *     out[n,o,y,x] = lrelu_0.2(b[o] + sum_c w[o,c] * m_c[y,x])
 * The mean is taken of the byte levels, as the reference takes it, not of the raw image.  A NaN pixel stays a NaN (torch's clamp)
 * and reaches the one output pixel whose block holds it.  One thread per output pixel, the weights in LDS.  TE_ERR_SHAPE, nothing
 * launched, unless S is a positive multiple of R (S <= 32768), 1 <= C0 <= 1024 and 1 <= N < 65536; another value of preprocessed is
 * TE_ERR_UNSUPPORTED.
 *
 * te_avgpool2_act_f32 (attribute_classifier.py:74-80, :100-104; replaces nn.AvgPool2d(2, 2) and the LeakyReLU(0.2) after it):
 * x [planes,H,W] -> out [planes,H/2,W/2],
 *     out[p,y,x] = act((((x[p,2y,2x] + x[p,2y,2x+1]) + x[p,2y+1,2x]) + x[p,2y+1,2x+1]) * 0.25),    act(v) = v > 0 ? v : slope * v
 * so a NaN tap gives a NaN in its own output only and slope = 1 is the plain pool.  planes >= 1, H and W even and >= 2, at most 2^40
 * input elements, else TE_ERR_SHAPE.  Memory bound: where W % 4 == 0 (and x is 16-byte, out 8-byte aligned) a thread reads two
 * 16-byte row pieces and writes two outputs; elsewhere a thread reads four scalars and writes one.  The grid is NOT capped: one
 * thread per work item with 64-bit offsets, no thread loops.
 *
 * te_attr_score_f32 (attribute_classifier.py:147-148 and attribute_utils.py:28-32; replaces the LeakyReLU after dense0, dense1 =
 * Linear(K, 1) * scale + bias, torch.cat([logit, -logit], 1), Softmax(dim=1) and the [:, 1] slice): a [I,K] = dense0's output BEFORE
 * its activation, w [K] (scaled), bias [1]:
 *     logit[i] = bias[0] + sum_k w[k] * act(a[i,k])                         act as above
 *     score[i] = softmax([l, -l])[1] = 1 / (1 + exp(2 l))                   DECREASING in l, as the reference's is
 * evaluated as e / (1 + e), e = exp(-2 l), for l >= 0 and as 1 / (1 + exp(2 l)) for l < 0, so nothing overflows: never Inf, NaN only
 * from a NaN row; a score below FLT_MIN (l > 43.66) is returned as 0, so l = 50 gives exactly 0 and l = -50 exactly 1.  logit or
 * score may be NULL, not both.  Shaped for latency: one wave per row, its lanes stride K with 16-byte loads, the sum is a fixed-shape
 * butterfly; a row's result is bitwise independent of I.  I >= 1, K >= 4, K % 4 == 0, 16-byte aligned a and w, anything else is
 * TE_ERR_SHAPE; nothing is launched on a refusal.
 */
int te_attr_stem_fwd_f32(float* out, const float* img, const float* w, const float* b, int N, int S, int R, int C0, int preprocessed,
                         te_stream_t stream);
int te_avgpool2_act_f32(float* out, const float* x, int64_t planes, int H, int W, float slope, te_stream_t stream);
int te_attr_score_f32(float* logit, float* score, const float* a, const float* w, const float* bias, int64_t I, int K, float slope,
                      te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M7  the ResNet-18 pose classifier of attribute editing (our_interfaceGAN/ffhq_utils/dex/models.py:73-89: ClassifyModel = torchvision's
 * resnet18 without its fc, Linear(512, 2) and a softmax; ffhq_utils/dex/api.py:61-65 estimate_gender, which runs it after eval('pose'),
 * api.py:34-39; called from edit_all_noinversion_ffhq.py:113-131).  Every other convolution of the network (the first of each block,
 * the 3x3 and 1x1 stride-2 ones) is M4's te_conv2d_f32, the global average is M2's te_adaptive_avgpool_f32 with OH = OW = 1, and
 * extra_layer + softmax + [:, 0] is M5's te_cls_score_f32 mode 1; here the residual epilogue, the input end and the padded max pool.
 * Forward only (the classifier runs under no_grad in eval mode), NCHW fp32, no atomics, no workspace.  Every BatchNorm2d (eps 1e-5,
 * eval) is folded into its convolution's weight and bias by the caller.  Both convolutions below run te_conv2d_f32's main loop
 * (csrc/conv2d_body.h) with the same k permutation, so their accumulators are te_conv2d_f32's bit for bit.
 *
 * te_conv2d_res_f32 (torchvision BasicBlock.forward as models.py:74-75 builds it: conv2 + bn2, `out += identity`, ReLU; replaces the
 * second convolution of each of the eight blocks with its batch norm, the addition and the activation):
 *     out[b,m,oy,ox] = act((acc + bias[m]) + res[b,m,oy,ox])        acc = sum_{c,ky,kx} w[m,c,ky,kx] * x[b, c, oy*s + ky - py, ox*s + kx - px]
 * with two separately rounded fp32 additions in this order; act 0 none, 1 ReLU (a NaN propagates: a NaN in res reaches its own
 * element only).  x [B,Ci,H,W], w [Co,Ci,kh,kw], bias [Co]; out and res are contiguous [B,Co,Ho,Wo] (no channel slice); res may be
 * neither out nor overlap it.  For every input the result is bitwise relu(te_conv2d_f32(act = 0) + res), and an image's outputs
 * do not depend on the batch it is in.  Refusals are te_conv2d_f32's (s other than 1 or 2, act other than 0 or 1, a kernel above
 * 7 x 7: TE_ERR_UNSUPPORTED; padding >= the kernel, Ho or Wo < 1, a non-positive size, sizes past 31 bits: TE_ERR_SHAPE) plus a NULL
 * res (TE_ERR_NULL); nothing is launched on a refusal.
 *
 * te_pose_stem_fwd_f32 (edit_all_noinversion_ffhq.py:113-116, api.py:62 CenterCrop(224), resnet18's conv1 + bn1 + relu as models.py:75
 * keeps them; replaces the channel flip, the clamp / add / div / mul / round chain, the centre crop and Conv2d(3, Co, 7, stride=2,
 * padding=3, bias=False) + BatchNorm2d + ReLU): img [N,3,H,W]; w [Co,3,7,7] and b [Co] with the batch norm folded in; out [N,Co,Hc,Wc],
 * Hc = Wc = (crop - 1) / 2 + 1.  With y0 = (H - crop) / 2, x0 = (W - crop) / 2:
 *     preprocessed = 0: img is RGB, nominally in [-1, 1]:  v[n,c] = rint(((clamp(img[n, 2 - c], -1, 1) + 1) * 0.5) * 255), each step
 *                       rounded to fp32, ties to even: torch's result bit for bit (the chain of te_dex_stem_fwd_f32)
 *     preprocessed = 1: img is what the editing scripts hand over, BGR byte levels:  v[n,c] = img[n,c]
 *     out[n,o,y,x] = relu(b[o] + sum_{c,ky,kx} w[o,c,ky,kx] * v[n, c, y0 + 2y + ky - 3, x0 + 2x + kx - 3])
 * where a tap with 2y + ky - 3 or 2x + kx - 3 outside [0, crop) is ZERO: the padding is that of the crop, image pixels outside the
 * window are never read (as in te_dex_stem_fwd_f32).  A NaN pixel stays a NaN and reaches exactly the outputs whose 7 x 7 window
 * holds it.  An implicit GEMM with K = 147 whose gather does the preprocessing on the way into LDS; the result is bitwise
 * te_conv2d_f32(v of the crop, s = 2, padding 3, act 1).  TE_ERR_SHAPE, nothing launched, for crop < 1, crop > H or W, an odd H - crop
 * or W - crop (DEX's rule), N < 1 or N >= 65536, Co < 1; another value of preprocessed is TE_ERR_UNSUPPORTED.
 *
 * te_maxpool3s2p1_f32 (resnet18's maxpool as models.py:75 keeps it; replaces nn.MaxPool2d(3, 2, 1)): x [planes,H,W] ->
 * out [planes,Ho,Wo], Ho = (H - 1) / 2 + 1, Wo likewise; the window of output (y, x) is rows 2y - 1 ... 2y + 1 and columns
 * 2x - 1 ... 2x + 1 inside the plane.  The padding never wins (a plane of -inf stays -inf); a greater value or a NaN replaces, the
 * rule of te_maxpool2_fwd_f32, so a NaN tap gives a NaN in the outputs that see it.  planes, H, W >= 1 with H * W below 2^31 and at
 * most 2^40 input elements, else TE_ERR_SHAPE; nothing is launched on a refusal.  One thread per output element.
 */
int te_conv2d_res_f32(float* out, const float* x, const float* w, const float* bias, const float* res, int B, int Ci, int Co, int H, int W,
                      int kh, int kw, int s, int py, int px, int act, te_stream_t stream);
int te_pose_stem_fwd_f32(float* out, const float* img, const float* w, const float* b, int N, int H, int W, int crop, int Co,
                         int preprocessed, te_stream_t stream);
int te_maxpool3s2p1_f32(float* out, const float* x, int64_t planes, int H, int W, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M8  the AlexNet LPIPS of the diversity score (metrics/lpips.py:49-82 LPIPS.forward, called for all 780 pairs of a group of 40 images by
 * metrics/evaluate_query.py:82-91 calculate_lpips_given_images from :94-133 evaluate_lpips).  conv2 ... conv5 of torchvision's
 * alexnet().features are M4's te_conv2d_f32 with act 1, its max pools te_pool3_f32 mode 0; here the stem, the normalisation and the
 * head (csrc/lpips_alex.hip).  The reference runs the network on both images of every pair again (1 560 passes per group); here it
 * runs once over the group and the pairs are a property of the head.  Forward only, NCHW fp32, no atomics, fixed-order reductions:
 * results are bit-reproducible from run to run.
 *
 * te_alex_stem_fwd_f32 (lpips.py:73 (x - mu) / sigma and features[0:2] = Conv2d(3, 64, 11, stride=4, padding=2) + ReLU): x [N,3,H,W]
 * generator images, w [Co,3,11,11], b [Co]; out [N,Co,Ho,Wo], Ho = (H - 7) / 4 + 1, Wo likewise.
 *     s(x)[n,c] = (x[n,c] - mu[c]) / sigma[c]      mu (-0.03, -0.088, -0.188), sigma (0.458, 0.448, 0.450), each step rounded to fp32
 *     out[n,o,y,x] = relu(b[o] + sum_{c,ky,kx} w[o,c,ky,kx] * s(x)[n, c, 4y + ky - 2, 4x + kx - 2])
 * where a tap outside the image is ZERO: the padding is that of the scaled image, as in te_lpips_stem_fwd_f32.  An implicit GEMM with
 * K = 363 on te_conv2d_f32's main loop (csrc/conv2d_body.h) whose gather scales a tap on the way into LDS: the loop sees the fp32
 * values torch's (x - mu) / sigma would store, in te_conv2d_f32's order of k, so an image's outputs do not depend on its batch or its
 * tile.  A NaN pixel reaches exactly the outputs whose 11 x 11 window holds it.  The 11 x 11 kernel and the stride of 4 are this
 * entry point's own limits: te_conv2d_f32 keeps refusing them.  TE_ERR_NULL for a NULL pointer; TE_ERR_SHAPE for N < 1, N >= 65536,
 * H, W or Co < 1, H + 4 < 11 or W + 4 < 11, 3 * H * W past 31 bits; nothing is launched on a refusal.
 *
 * te_lpips_unit_f32 (lpips.py:16-17 normalize): out[n,c,p] = f[n,c,p] * rsqrt(sum_c f[n,c,p]^2 + 1e-10), f and out [N,C,HW]; out may
 * be f.  The eps sits INSIDE the root: this is the one place where this LPIPS differs from L1's te_lpips_normalize_f32, which is
 * f / (sqrt(sum) + 1e-10).  A pixel's sum of squares is taken in fp64 (channel slices added in slice order, as
 * te_lpips_pair_head_fwd_f32 does) and rsqrt rounded to fp32 once; a pixel that is zero on every channel gives exactly 0.
 *
 * The all-pairs head, for NORMALISED taps fh [N,C,HW] (te_lpips_unit_f32's output) and a head w [C] of either sign:
 *     te_lpips_allpairs_ws_floats(N, C, HW) : the floats of one layer's workspace (negative: a refused size)
 *     te_lpips_allpairs_fwd_f32             : the workspace's partials (one per pair, block of 256 pixels and slice of 32 channels) of
 *                                             sum_p sum_c w[c] (fh[i,c,p] - fh[j,c,p])^2 for all i <= j
 *     te_lpips_allpairs_dist_f32            : D[i,j] = sum_{l < L} (sum_b partial_l[(i,j), b]) / hw[l], D [N,N], the partials (pixel
 *                                             blocks, a block's channel slices inside it) and the layers in ascending order
 *                                             (lpips.py:77-81 `lpips_value +=`); partial / c / hw are HOST arrays of L <= 8 entries
 * The difference is formed before the square (never a^2 + b^2 - 2ab), w[c] * d is rounded, then one fma per term; a pair's sum is a
 * chain over a slice's channels per pixel, a fixed tree over the 256 pixels of a block, then the partials in order.  Hence: the
 * diagonal is exactly 0; D[i,j] == D[j,i] bit for bit; D[i,j] depends on images i and j, C and HW alone, not on N or on the other
 * images of the group; a NaN in image i reaches row i and column i only.  A workgroup takes 256 pixels, 32 channels and a tile of
 * 8 x 8 images, so a tap is read about N / 8 + 1 times, not N - 1.  1 <= N < 65536 (N = 1 gives [[0]]), C, HW >= 1,
 * HW <= 65535 * 256, C <= 65535 * 32, C * HW below 2^31, else TE_ERR_SHAPE; nothing is launched on a refusal.
 */
int te_alex_stem_fwd_f32(float* out, const float* x, const float* w, const float* b, int N, int H, int W, int Co, te_stream_t stream);
int te_lpips_unit_f32(float* out, const float* f, int N, int C, int64_t HW, te_stream_t stream);
int64_t te_lpips_allpairs_ws_floats(int N, int C, int64_t HW);
int te_lpips_allpairs_fwd_f32(float* partial, const float* fh, const float* w, int N, int C, int64_t HW, te_stream_t stream);
int te_lpips_allpairs_dist_f32(float* D, const float* const* partial, const int* c, const int64_t* hw, int L, int N, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M9  the ArcFace IR-SE50 identity network of edit evaluation (pSp/models/encoders/model_irse.py:10-49 Backbone with
 * pSp/models/encoders/helpers.py:16-120, applied by pSp/criteria/id_loss.py:8-21 behind the crop [35:223, 32:220] and
 * AdaptiveAvgPool2d((112, 112)); pSp/scripts/calc_id_loss_parallel.py:58-67 takes the paired dot products).  The second convolution of
 * a unit (3x3, stride 1 or 2, its batch norm folded in) and the 1x1 stride-s shortcut convolution are M4's te_conv2d_f32 with act 0,
 * the squeeze is M2's te_adaptive_avgpool_f32 with OH = OW = 1, and output_layer (BatchNorm2d, Dropout in eval mode, Flatten, Linear,
 * BatchNorm1d, folded exactly by the caller) is M2's te_fc_stream_f32 with act 0; here what is left (csrc/irse.hip).  The forward
 * pass (the backward pass with respect to the image, for IDLoss.forward as a loss, is M9b), NCHW fp32, no atomics, no workspace, bit-reproducible; an
 * image's result is bitwise independent of the batch it is in.  Nothing is launched on a refusal.
 *
 * te_conv2d_prelu_f32 (helpers.py:86-90, :108-112: BatchNorm2d(in_channel), Conv2d(in_channel, depth, 3, 1, 1, bias=False), PReLU(depth);
 * replaces the batch norm in FRONT of the zero-padded convolution, the convolution and the activation):
 *     v[b,c,iy,ix] = fma(in_scale[c], x[b,c,iy,ix], in_shift[c])   for a tap INSIDE the image (one fma: a single rounding),
 *                    exactly 0 for a tap of the padding          (in_scale == in_shift == NULL: v = x)
 *     t = acc + bias[m],  acc = sum_{c,ky,kx} w[m,c,ky,kx] * v[b, c, oy*s + ky - py, ox*s + kx - px];   out = t > 0 ? t : slope[m] * t
 * The shift cannot be folded into the bias: the padded taps do not carry it, so border outputs would differ.  x [B,Ci,H,W],
 * w [Co,Ci,kh,kw], bias, slope [Co], in_scale, in_shift [Ci]; out a contiguous [B,Co,Ho,Wo] (no channel slice, no `act`).  This is
 * te_conv2d_f32's main loop (csrc/conv2d_body.h) with another gather and another epilogue, the k permutation untouched: without the
 * affine the accumulators are te_conv2d_f32's bit for bit and the result is bitwise prelu(te_conv2d_f32(act = 0)); the product
 * slope[m] * t is one rounding.  A NaN propagates (it fails t > 0, and slope * NaN is a NaN): a NaN pixel reaches exactly the outputs
 * whose window holds it.  Kernel sizes, strides, padding rules and size limits are te_conv2d_f32's (s other than 1 or 2, a kernel above
 * 7 x 7: TE_ERR_UNSUPPORTED; padding >= the kernel, Ho or Wo < 1, a non-positive size, sizes past 31 bits: TE_ERR_SHAPE); a NULL out, x,
 * w, bias or slope, or exactly one of in_scale and in_shift: TE_ERR_NULL.
 *
 * te_id_stem_fwd_f32 (id_loss.py:18-19 and model_irse.py:21-23 input_layer; replaces the crop, AdaptiveAvgPool2d((Pn, Pn)) and
 * Conv2d(3, Co, 3, 1, 1, bias=False) + BatchNorm2d + PReLU, the batch norm folded into w and b by the caller): img [N,3,H,W],
 * w [Co,3,3,3], b, slope [Co]; out [N,Co,Pn,Pn].  With Lh = y1 - y0, Lw = x1 - x0:
 *     p[n,c,i,j] = (sum of img[n, c, y0 + floor(i Lh / Pn) : y0 + ceil((i + 1) Lh / Pn), x0 + floor(j Lw / Pn) : x0 + ceil((j + 1) Lw / Pn)],
 *                   row-major in fp32) / the count                                     torch's rule per axis, as te_adaptive_avgpool_f32
 *     t = b[o] + sum_{c,ky,kx} w[o,c,ky,kx] * p[n, c, y + ky - 1, x + kx - 1]   (0 outside the Pn x Pn plane);   out = t > 0 ? t : slope[o] * t
 * An implicit GEMM with K = 27 whose gather averages a tap's window on the way into LDS; image pixels outside the window are never
 * read.  The result is bitwise te_conv2d_prelu_f32(te_adaptive_avgpool_f32(the contiguous crop), NULL, NULL, ...).  TE_ERR_SHAPE for an
 * empty window (y1 <= y0 or x1 <= x0), a window outside the image, Pn < 1, Pn or a window side above 32768, N < 1 or N >= 65536,
 * Co < 1, 3 * H * W past 31 bits; TE_ERR_NULL for a NULL pointer.
 *
 * te_se_excite_f32 (helpers.py:57-72 SEModule without its final product; replaces fc1, ReLU, fc2 and the sigmoid on the pooled vector):
 *     gate[b,c] = sigmoid(sum_r w2[c,r] * relu(sum_k w1[r,k] * pooled[b,k]))
 * pooled [B,C] (te_adaptive_avgpool_f32 with OH = OW = 1), w1 [R,C], w2 [C,R], neither with a bias (helpers.py:61-63); gate [B,C].
 * Shaped for latency: one workgroup of four waves per image; a hidden unit is one wave's dot product (lane l takes k = l, l + 64, ...
 * as one fma chain, the lanes meet in a fixed butterfly), a gate one thread's fma chain over r in ascending order.  The sigmoid is
 * 1 / (1 + exp(-z)) for z >= 0 and e / (1 + e), e = exp(z), for z < 0, so nothing overflows: a logit of +-100 gives a finite gate in
 * [0, 1].  A NaN in pooled[b] makes the gates of image b NaN and no other (relu keeps a NaN); a row is bitwise independent of B.
 * B, C >= 1, 1 <= R <= 1024 (the hidden units live in LDS) and C * R below 2^31, else TE_ERR_SHAPE.
 *
 * te_se_scale_add_f32 (helpers.py:73 `module_input * x` and :92-95, :117-120 `res + shortcut`, with MaxPool2d(1, stride) at :80, :102):
 *     out[b,c,y,x] = res[b,c,y,x] * gate[b,c] + sc[b, c, s*y, s*x]
 * res, out [B,C,Ho,Wo], gate [B,C] or NULL (mode 'ir': out = res + sc), sc [B,C,Hs,Ws].  s = 1: the shortcut is the 1x1 convolution +
 * batch norm output; s = 2: it is the unit's input seen through MaxPool2d(1, 2).  The product and the sum are two separately rounded
 * fp32 operations (no fma).  Refused (TE_ERR_SHAPE) unless Ho == (Hs - 1) / s + 1 and Wo == (Ws - 1) / s + 1, all sizes positive, a plane
 * below 2^31 and the shortcut at most 2^40 elements; s other than 1 or 2 is TE_ERR_UNSUPPORTED.  Memory bound: where s == 1, Wo % 4 == 0
 * and out, res, sc are 16-byte aligned a thread moves 16 bytes of each; elsewhere one element.  One thread per work item with 64-bit
 * offsets, no thread loops (as te_avgpool2_act_f32).
 *
 * te_rows_unit_f32 (helpers.py:16-19 l2_norm): out[i,:] = a[i,:] / norm_i, norm_i = (float)sqrt(sum_d (double)a[i,d]^2): the squares
 * are exact in fp64, their sum is taken in fp64 (a chain per lane, a fixed butterfly over the 64 lanes), the root rounded to fp32
 * once, then one fp32 division per element.  A zero row gives NaN (0 / 0), as the reference's does.  out may be a.
 * te_rows_dot_f32 (id_loss.py:34-36, calc_id_loss_parallel.py:67): out[i] = sum_d a[i,d] * b[i,d], one wave per row: the products are
 * exact in fp64, summed in fp64 in the same fixed shape and rounded to fp32 once.  Both: a, b, out rows of D contiguous floats,
 * 1 <= I < 2^31, D >= 1, else TE_ERR_SHAPE; a row's result is bitwise independent of I.
 */
int te_conv2d_prelu_f32(float* out, const float* x, const float* w, const float* bias, const float* slope, const float* in_scale,
                        const float* in_shift, int B, int Ci, int Co, int H, int W, int kh, int kw, int s, int py, int px, te_stream_t stream);
int te_id_stem_fwd_f32(float* out, const float* img, const float* w, const float* b, const float* slope, int N, int H, int W, int y0, int y1,
                       int x0, int x1, int Pn, int Co, te_stream_t stream);
int te_se_excite_f32(float* gate, const float* pooled, const float* w1, const float* w2, int B, int C, int R, te_stream_t stream);
int te_se_scale_add_f32(float* out, const float* res, const float* gate, const float* sc, int B, int C, int Ho, int Wo, int Hs, int Ws, int s,
                        te_stream_t stream);
int te_rows_unit_f32(float* out, const float* a, int64_t I, int D, te_stream_t stream);
int te_rows_dot_f32(float* out, const float* a, const float* b, int64_t I, int D, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M9b  the identity network as a LOSS (pSp/criteria/id_loss.py:23-45 IDLoss.forward, one of the three losses of
 * pSp/training/coach_new.py): its backward pass with respect to the input image, which the reference leaves to torch autograd.  The
 * network is frozen: there is no weight gradient and no training-mode batch norm.  Every operator of M9 is linear in its input except
 * the PReLU, the SE gate and the final normalisation; the Linear backwards is M2's te_fc_stream_f32 on the transposed folded weight.
 * NCHW fp32, no atomics, bit-reproducible, an image's gradient is bitwise independent of the batch it is in; nothing is launched on a
 * refusal (csrc/irse_bwd.hip; the two *_keep entry points are csrc/irse.hip's).
 *
 * te_conv2d_prelu_keep_f32, te_id_stem_keep_f32 (the forward of a differentiable pass): te_conv2d_prelu_f32 and te_id_stem_fwd_f32 with
 * one more output, pre [B,Co,Ho,Wo] = t, the value the PReLU is applied to.  With a negative slope a positive output does not tell
 * the branch, so the backward pass reads it from pre.  out has the bits of the entry point without `_keep`; refusals are the same, and
 * a NULL pre is TE_ERR_NULL.
 *
 * te_conv2d_dgrad_f32 (replaces autograd's conv2d backward w.r.t. the input, with what follows it): the data gradient of te_conv2d_f32 /
 * te_conv2d_prelu_f32 for x [B,Ci,H,W], w [Co,Ci,kh,kw], stride s, padding (py, px); g [B,Co,Ho,Wo] -> gx [B,Ci,H,W]:
 *     acc[b,ci,y,x] = sum over (co,ky,kx) with y = s*oy - py + ky, x = s*ox - px + kx of g[b,co,oy,ox] * w[co,ci,ky,kx]
 *     pre != NULL :  gx = pre[b,ci,y,x] > 0 ? acc : acc * slope[ci]        PReLU' of the layer the gradient enters; torch's rule: 0, -0
 *                                                                           and NaN take the slope.  in_scale and add must be NULL
 *     pre == NULL :  gx = in_scale[ci] * acc + a                           each term optional (one fma where both are given);
 *                    a = add[b, ci, y / add_s, x / add_s] where add_s divides y and x, else 0:  add [B,Ci,(H-1)/add_s+1,(W-1)/add_s+1].
 *                    add_s = 2 is the adjoint of MaxPool2d(1, 2) (te_se_scale_add_f32's shortcut), add_s = 1 a plain tensor (the
 *                    convolution shortcut's gradient); in_scale is the leading batch norm's gradient (its shift and the zero padding
 *                    drop out)
 * The weight arrives as the adjoint GEMM reads it, made once by the caller.  Per axis and output parity r < s the taps that reach
 * rows y = s*yy + r are k = k0 + s*j, k0 = (r + p) % s, j < n = ceil((k_size - k0) / s).  wt holds, for (ry, rx) = (0,0), (0,1), (1,0), (1,1)
 * (s = 1: the one phase), a block [Ci, Co, ny, nx] with the taps flipped: wt[ci,co,jy,jx] = w[co, ci, k0y + s*(ny-1-jy), k0x + s*(nx-1-jx)].
 * Each phase is a dense stride-1 implicit GEMM over g on te_conv2d_f32's main loop (csrc/conv2d_body.h, the k order of the forward
 * family) with K = Co*ny*nx, stored with a pitch of s; a 3x3 stride-2 layer is the sub-kernels 1x1, 1x2, 2x1 and 2x2, none of whose
 * taps is a zero of the zero-inserted plane; a phase no tap reaches (the odd ones of a 1x1 stride-2 layer) receives the epilogue of 0.
 * A NaN in g reaches exactly the inputs whose window holds it.  1 <= kh, kw <= 7 and s in {1, 2}, else TE_ERR_UNSUPPORTED (also for
 * pre together with in_scale or add, and add_s outside {1, 2}); padding >= the kernel, Ho or Wo < 1, non-positive sizes, an image of g or
 * gx past 31 bits: TE_ERR_SHAPE; a NULL gx, g or wt, or exactly one of pre and slope: TE_ERR_NULL.
 *
 * te_se_bwd_f32 (helpers.py:57-73 SEModule backwards): out = r * gate + shortcut, gate = sigmoid(w2 relu(w1 pooled)), pooled = mean(r).
 *     ggate[b,c] = sum_hw gout * r                                  one wave per plane: a chain per lane, a fixed butterfly
 *     gh[b,r]    = hidden[b,r] > 0 ? sum_c w2[c,r] * ggate[b,c] * gate[b,c] * (1 - gate[b,c]) : 0      hidden recomputed as te_se_excite_f32
 *     gmean[b,c] = (sum_r w1[r,c] * gh[b,r]) / (Ho*Wo)              one latency-shaped workgroup per image, r ascending
 *     gr         = gout * gate[b,c] + gmean[b,c]                    one fma; 16 bytes per thread where Ho*Wo % 4 == 0 and aligned
 * gout, r, gr [B,C,Ho,Wo]; gate, pooled [B,C]; w1 [R,C], w2 [C,R]; ws 2*B*C floats (ggate, gmean).  The shortcut's gradient is gout
 * itself.  Limits are te_se_excite_f32's, a plane below 2^31 and 2^40 elements, else TE_ERR_SHAPE.
 *
 * te_id_stem_bwd_f32 (the adjoint of te_id_stem_fwd_f32): g [N,Co,Pn,Pn], pre the stem's kept pre-activation, wt the stem weight
 * [Co,3,3,3] in te_conv2d_dgrad_f32's layout ([3, Co*9], flipped); gimg [N,3,H,W]; ws N*3*Pn*Pn floats.  g * PReLU'(pre) (in the gather)
 * goes through the data gradient of the 3x3 convolution to the pooled plane in ws; then AdaptiveAvgPool2d and the crop backwards as a
 * GATHER: an image pixel inside the window sums the pooled windows [floor(i L / Pn), ceil((i + 1) L / Pn)) that contain it (at most
 * 2 x 2 where L >= Pn), each divided by its count, rows then columns ascending; a pixel outside the window is exactly 0.  Refusals
 * are te_id_stem_fwd_f32's.
 *
 * te_rows_unit_bwd_f32 (helpers.py:16-19 l2_norm backwards): e = a / norm; ga[i,:] = (ge[i,:] - e[i,:] * <e[i,:], ge[i,:]>) / norm_i, the
 * dot product and the norm's square in fp64 in te_rows_dot_f32's shape, each rounded to fp32 once.  Limits are te_rows_unit_f32's.
 */
int te_conv2d_prelu_keep_f32(float* out, float* pre, const float* x, const float* w, const float* bias, const float* slope,
                             const float* in_scale, const float* in_shift, int B, int Ci, int Co, int H, int W, int kh, int kw, int s, int py,
                             int px, te_stream_t stream);
int te_id_stem_keep_f32(float* out, float* pre, const float* img, const float* w, const float* b, const float* slope, int N, int H, int W,
                        int y0, int y1, int x0, int x1, int Pn, int Co, te_stream_t stream);
int te_conv2d_dgrad_f32(float* gx, const float* g, const float* wt, const float* pre, const float* slope, const float* in_scale,
                        const float* add, int B, int Ci, int Co, int H, int W, int kh, int kw, int s, int py, int px, int add_s,
                        te_stream_t stream);
int te_se_bwd_f32(float* gr, float* ws, const float* gout, const float* r, const float* gate, const float* pooled, const float* w1,
                  const float* w2, int B, int C, int R, int Ho, int Wo, te_stream_t stream);
int te_id_stem_bwd_f32(float* gimg, float* ws, const float* g, const float* wt, const float* pre, const float* slope, int N, int H, int W,
                       int y0, int y1, int x0, int x1, int Pn, int Co, te_stream_t stream);
int te_rows_unit_bwd_f32(float* ga, const float* ge, const float* e, const float* a, int64_t I, int D, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M8b  the AlexNet LPIPS as a LOSS (pSp/criteria/lpips/lpips.py:29-35 LPIPS('alex').forward with networks.py:35-84 and utils.py:6-8, the
 * lpips_lambda term of pSp/training/coach_new.py:285-320 calc_loss): its backward pass with respect to the first image, which the
 * reference leaves to torch autograd.  This LPIPS normalises a tap as x / (sqrt(sum_c x^2) + 1e-10), eps BESIDE the root: its heads are
 * L1's te_lpips_normalize_f32 / te_lpips_head_fwd_f32 / te_lpips_head_bwd_f32 (not M8's te_lpips_unit_f32), the forward trunk is M8's
 * te_alex_stem_fwd_f32 with M4's te_pool3_f32 and te_conv2d_f32, the data gradients of conv2 ... conv5 are M9b's te_conv2d_dgrad_f32;
 * here the two adjoints that are left (csrc/lpips_alex_bwd.hip).  The network is frozen: there is no weight gradient.  NCHW fp32, no
 * atomics, no workspace, fixed-order sums: bit-reproducible, and an image's gradient is bitwise independent of the batch it is in.
 * Nothing is launched on a refusal.
 *
 * te_pool3s2_max_bwd_f32 (the adjoint of te_pool3_f32 mode 0 = nn.MaxPool2d(3, 2), features[2] and [5] of torchvision's alexnet): x, gx
 * `planes` planes of H x W, g `planes` planes of Ho x Wo, Ho = (H - 3) / 2 + 1, Wo likewise.  The windows overlap, so this is a GATHER:
 * an input pixel lies in at most 2 x 2 windows; for each it recomputes the argmax from x and it sums the g of the windows whose argmax
 * it is, window rows then columns ascending, from 0.  The argmax rule is torch's: the scan is ky, then kx, ascending, and a later
 * element replaces the current one only if it is greater or is a NaN, so the first of equal maxima wins and the last NaN of a window
 * takes its gradient.  ALL of gx is written: a pixel that wins no window, and the last row / column where (H - 3) % 2 == 1 (W
 * likewise), which no window reaches, are exactly 0.  TE_ERR_NULL for a NULL pointer; TE_ERR_SHAPE for planes, H or W < 1, H < 3 or
 * W < 3 (as the forward), a plane past 31 bits or more than 2^31 - 1 blocks of 256 pixels.
 *
 * te_alex_stem_dgrad_f32 (the adjoint of te_alex_stem_fwd_f32 without its ReLU: the caller's g is already masked, which
 * te_lpips_head_bwd_f32 does): g [N,Co,Ho,Wo], Ho = (H - 7) / 4 + 1, Wo likewise; gimg [N,3,H,W], the gradient of the UNSCALED image:
 *     gimg[n,c,y,x] = (sum over (o,ky,kx) with y + 2 - ky = 4 oy, x + 2 - kx = 4 ox, 0 <= oy < Ho, 0 <= ox < Wo
 *                      of w[o,c,ky,kx] * g[n,o,oy,ox]) / sigma[c]             sigma (0.458, 0.448, 0.450)
 * the sum one fma chain from 0 over o, then ky, then kx ascending, the division one correctly rounded fp32 step (torch's backward of
 * (x - mu) / sigma; mu and the zero padding drop out).  Per axis and output parity r < 4 the taps that reach rows y = 4 yy + r are
 * k = k0 + 4 j, k0 = (r + 2) % 4, j < n = (3, 2, 3, 3)[r], read from the gradient rows yy + (r + 2) / 4 - j: 16 dense phases with
 * sub-kernels of 3 x 3 down to 2 x 2, never a walk over the zero-inserted plane.  wt holds, for ry = 0 ... 3, a block [Co, ny, 11, 3]:
 *     wt[ry][o, jy, kx, c] = w[o, c, k0(ry) + 4 jy, kx]                       363 Co floats, made once by the caller
 * (rows split by phase, columns whole: a lane owns the four column phases of its position, because together they read four
 * neighbouring gradient columns; the weight index is uniform over a wave, which owns one ry).  A pixel that no window reaches is
 * exactly 0 (column 29 of a 30-wide image: its taps kx = 3, 7 ask for ox = 7, 6 >= Wo = 6).  A NaN in g reaches exactly the pixels one
 * of whose taps reads it, on all three channels.  Limits are te_alex_stem_fwd_f32's: TE_ERR_NULL for a NULL pointer; TE_ERR_SHAPE for
 * N < 1, N >= 65536, H, W or Co < 1, H + 4 < 11 or W + 4 < 11, 3 * H * W or Co * Ho * Wo past 31 bits.
 */
int te_pool3s2_max_bwd_f32(float* gx, const float* g, const float* x, int64_t planes, int H, int W, te_stream_t stream);
int te_alex_stem_dgrad_f32(float* gimg, const float* g, const float* wt, int N, int H, int W, int Co, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M10  the dual-space pSp encoder of real-image inversion (pSp/models/encoders/psp_encoders_new.py:35-140
 * GradualStyleEncoder(50, 'ir_se'), applied by pSp/models/psp_new.py:90-109 pSp.forward).  input_layer and body are M9's
 * te_conv2d_prelu_f32 and IR-SE units, the two lateral 1x1 convolutions are M4's te_conv2d_f32; here what sits on the backbone
 * (csrc/psp_heads.hip).  Forward only, NCHW fp32, no atomics, bit-reproducible; an image's outputs are bitwise independent of the batch
 * it is in.  Every check is made before any launch; nothing is launched on a refusal.
 *
 * te_conv2d_heads_f32 (psp_encoders_new.py:11-32 GradualStyleBlock: Conv2d(512, 512, 3, stride=2, padding=1) + LeakyReLU(0.01) chains and
 * the EqualLinear behind them, :120-136 the loops over styles and spatials; replaces the 138 convolutions, their activations and the
 * 30 linears, head by head): G convolutions of one shape in one launch,
 *     out[b, c0 + g*Cg + m, oy, ox] = lrelu_slope(bias[g*Cg + m]
 *         + sum_{c,ky,kx} w[g, m, c, ky, kx] * x[b, xg(g)*Ci + c, oy*s + ky - py, ox*s + kx - px])                  x = 0 outside the image
 * xg(g) = 0 when shared != 0 (all heads read the same [B,Ci,H,W] input), else xg(g) = g and x is [B, G*Ci, H, W].  w [G,Cg,Ci,kh,kw],
 * bias [G*Cg]; out is the channel slice [c0, c0 + G*Cg) of a contiguous [B,Ctot,Ho,Wo]; lrelu_slope(v) = v > 0 ? v : v * slope
 * (slope = 1 is the identity, a NaN propagates).  kh = kw = 1 on a 1 x 1 plane is the grouped linear layer (the caller folds
 * EqualLinear's scale into w and bias).  Kernel sizes, strides, padding rules and size limits are te_conv2d_f32's, with Co = G * Cg;
 * Cg % 64 == 0, else TE_ERR_UNSUPPORTED: a workgroup's 64-channel block then never straddles two heads.
 * Two routes, chosen from (K = Ci*kh*kw, Ho*Wo) alone, never from B or G:
 *   unsplit (S = 1): te_conv2d_f32's main loop (csrc/conv2d_body.h) with a gather that adds the head's channel offset and the leaky
 *     ReLU as the epilogue; the k permutation is untouched, so for every head the result is bitwise
 *     leaky(te_conv2d_f32(x_g, w_g, b_g, act = 0)).  ws may be NULL.
 *   split (S > 1), for planes of a few pixels, where G * Cg / 64 workgroups would each walk all of K: the same loop over one of S
 *     ranges of k (whole 32-deep steps, the ranges in ascending order of k), the bare partial tiles go to the caller's workspace
 *     ws[S][B][G*Cg][Ho*Wo], a second kernel sums them over s ascending, then adds the bias and applies the leaky ReLU.  A NULL ws or
 *     ws_bytes below S * B * G*Cg * Ho*Wo * 4 is TE_ERR_WORKSPACE.
 * splits = 0 takes the rule, S = te_conv2d_heads_splits(Ci, kh, kw, Ho, Wo); splits = n in [1, 16] runs n ranges instead (for
 * measurements and tests; n ranges must all be non-empty, else TE_ERR_SHAPE).  te_conv2d_heads_ws_bytes is the rule's workspace
 * (0 where S = 1).  Both helpers return a negative TE_ERR_* on bad arguments.  A NaN input element reaches exactly the outputs of its
 * own head(s) and image whose window holds it, on both routes.
 *
 * te_upsample_add_f32 (psp_encoders_new.py:84-101 _upsample_add; replaces F.interpolate(x, size=(H, W), mode='bilinear',
 * align_corners=True) + y): x [planes,h,w], y and out [planes,H,W].  Per axis src = o * (in - 1) / (out - 1), and 0 where out == 1,
 * evaluated exactly in integers as te_resize_bilinear_f32 evaluates its rule: the quotient is the first tap, the remainder over
 * out - 1 the second tap's weight l1 (rounded once), l0 = 1 - l1; x is mixed first (l1 * b + (l0 * a) with one fma), then y, then
 * the sum with y[...].  A tap of weight 0 does not enter, so equal sizes give bitwise x + y.  1 <= planes <= 65535, sizes up to 32768,
 * else TE_ERR_SHAPE.
 *
 * te_psp_codes_f32 (psp_encoders_new.py:132-138 torch.stack, adjust_style = EqualLinear(14, 16) over the head axis and the permutes;
 * psp_new.py:99-107 the latent averages): lat [B, Ns + Np, D] are the heads' latents, the Ns styles first.
 *     z[b, c, t] = (bz[t] + sum_{j < Ns} A[t, j] * lat[b, j, c]) + z_avg[c, t]           j ascending, one fp32 fma chain from bz[t]
 *     p[b, c, u] = lat[b, Ns + u, c] + p_avg[c, u]
 * A [T,Ns] and bz [T] arrive with EqualLinear's scale and lr_mul folded in; z_avg [D,T] and p_avg [D,Np] may each be NULL (nothing is
 * added then); z is [B,D,T], p is [B,D,Np].  B, Ns, Np, D, T >= 1, else TE_ERR_SHAPE.
 */
int te_conv2d_heads_splits(int Ci, int kh, int kw, int Ho, int Wo);
int64_t te_conv2d_heads_ws_bytes(int64_t B, int G, int Cg, int Ci, int kh, int kw, int Ho, int Wo);
int te_conv2d_heads_f32(float* out, float* ws, int64_t ws_bytes, const float* x, const float* w, const float* bias, int B, int G, int Ci,
                        int Cg, int H, int W, int kh, int kw, int s, int py, int px, int Ctot, int c0, int shared, float slope, int splits,
                        te_stream_t stream);
int te_upsample_add_f32(float* out, const float* x, const float* y, int64_t planes, int h, int w, int H, int W, te_stream_t stream);
int te_psp_codes_f32(float* z, float* p, const float* lat, const float* A, const float* bz, const float* z_avg, const float* p_avg,
                     int64_t B, int Ns, int Np, int D, int T, te_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * M10b  training the heads of the dual-space pSp encoder (pSp/training/coach_new.py:128-135 loss.backward() through
 * psp_encoders_new.py:11-32 GradualStyleBlock, :84-101 _upsample_add and :120-138 the head loops, the stack and adjust_style, which the
 * reference leaves to torch autograd): the backward pass of everything M10 puts on the backbone, with the weight gradients (the
 * backbone itself needs training-mode batch norm and is not here).  csrc/psp_heads_bwd.hip.  NCHW fp32, no atomics, every sum a
 * fixed-order chain or a fixed-shape tree: bit-reproducible from run to run.  Every check is made before any launch; nothing is
 * launched on a refusal.
 *
 * te_conv2d_heads_dgrad_f32 (replaces autograd's conv2d backward w.r.t. the input and the LeakyReLU backward in front of it, head by
 * head): the data gradient of te_conv2d_heads_f32 with shared = 0.  g is the channel slice [gc0, gc0 + G*Cg) of a contiguous
 * [B,gCtot,Ho,Wo]; gx [B,G*Ci,H,W]:
 *     acc[b, h*Ci + ci, y, x] = sum over (co,ky,kx) with y = s*oy - py + ky, x = s*ox - px + kx of g[b, gc0 + h*Cg + co, oy, ox] * w[h,co,ci,ky,kx]
 *     gx = act == NULL ? acc : (act[b, h*Ci + ci, y, x] > 0 ? acc : acc * slope)
 * act [B,G*Ci,H,W] is the kept OUTPUT of the leaky layer the gradient enters: slope > 0, so its sign is the pre-activation's and the
 * forward pass keeps nothing extra; torch's rule holds at 0, -0 and NaN (they take the slope).  wt is te_conv2d_dgrad_f32's layout with
 * one block per head: for each phase (ry, rx), ry-major, the heads' blocks [Ci, Cg, ny, nx] one behind the other ([G*Ci, Cg*ny*nx] per
 * phase), taps flipped.  It is te_conv2d_dgrad_f32's launch with one more gather (the workgroup's 64-channel block of gx names its
 * head, the head the channel offset into g): a stride-2 layer is four dense stride-1 phases stored with a pitch of 2, and for every
 * head the result is bitwise te_conv2d_dgrad_f32 on that head alone with pre = the head's slice of act and slope[] filled with the
 * scalar.  kh = kw = 1 on a 1 x 1 plane is the grouped EqualLinear backwards.  A NaN in g reaches exactly the inputs of its own head
 * and image whose window holds it.  Ci % 64 != 0, slope <= 0 (or NaN), a kernel above 7 x 7, a stride outside {1, 2}: TE_ERR_UNSUPPORTED;
 * a NULL gx, g or wt: TE_ERR_NULL; sizes, padding and slice as te_conv2d_dgrad_f32 / te_conv2d_heads_f32: TE_ERR_SHAPE.
 * (The heads that read a SHARED feature need no entry point: the sum over heads of their data gradients is te_conv2d_dgrad_f32 with
 * Co = G*Cg on w viewed as [G*Cg,Ci,kh,kw], whose `add` accumulates the several consumers of one feature.)
 *
 * te_conv2d_heads_wgrad_f32 (replaces autograd's conv2d backward w.r.t. weight and bias): of te_conv2d_heads_f32 and, with G = 1, of
 * the lateral te_conv2d_f32.  g as above, already multiplied by the leaky ReLU' (what the data gradient of the layer above wrote);
 * x [B,Ci,H,W] (shared != 0) or [B,G*Ci,H,W]; gw [G,Cg,Ci,kh,kw], gb [G*Cg]:
 *     gw[h,m,c,ky,kx] = sum over (b,oy,ox), b-major then row-major, of g[b, gc0 + h*Cg + m, oy, ox] * x[b, (shared ? c : h*Ci + c), s*oy+ky-py, s*ox+kx-px]
 *     gb[h*Cg + m]    = sum over (b,oy,ox) of g[b, gc0 + h*Cg + m, oy, ox]
 * with x = 0 outside the plane.  A GEMM with M = Cg per head, N = Ci*kh*kw and the reduction r = (b,oy,ox) of length R = B*Ho*Wo on
 * the fp32-input MFMA, 64 x 64 tiles, 32-deep steps with the k permutation of csrc/conv2d_body.h; both operands are gathers.  Inside a
 * step r is summed in the MFMA's order, the steps ascend.  A tap that only ever sees padding is exactly +0 (finite g).  gb: one wave
 * per channel, lane l sums r = l, l + 64, ... ascending, the lanes meet in a fixed butterfly.  The grid depends on geometry alone.
 * Two routes, chosen from (M, N, R) alone, never from G: unsplit (S = 1; ws may be NULL), or R cut into S ranges of whole steps in
 * ascending order whose partial gw go to ws[S][G*Cg][N] and are summed over s ascending by a second kernel; a NULL ws or ws_bytes
 * below S * G*Cg * N * 4 is TE_ERR_WORKSPACE.  splits = 0 takes the rule, S = te_conv2d_heads_wgrad_splits(Cg, Ci, kh, kw, B, Ho, Wo)
 * (few tiles and a long R: the two laterals); splits = n in [1, 16] runs n ranges instead (tests and measurements; every range must be
 * non-empty, else TE_ERR_SHAPE).  te_conv2d_heads_wgrad_ws_bytes is the rule's workspace (0 where S = 1); both helpers return a
 * negative TE_ERR_* on bad arguments.  G heads in one launch give the bits of G launches of one head.  Cg % 64 != 0, a kernel above
 * 7 x 7, a stride outside {1, 2}: TE_ERR_UNSUPPORTED; a NULL gw, gb, g or x: TE_ERR_NULL; the rest as te_conv2d_f32: TE_ERR_SHAPE.
 *
 * te_upsample_add_bwd_f32 (the adjoint of te_upsample_add_f32 w.r.t. x; the gradient of y is g itself): g [planes,H,W], gx and the
 * optional add [planes,h,w].  A GATHER: source pixel (i, j) sums, output rows ascending, then columns ascending, g[oy,ox] * (wy * wx)
 * over the outputs whose tap reaches it, one fma chain opened by the first term, with the very weights the forward formed (the same
 * integer quotient and remainder, l1 rounded once, l0 = 1 - l1; wy * wx one rounding); then + add where add != NULL.  A tap of weight 0
 * contributes nothing, so equal sizes give gx = g bit for bit; h = 1 or w = 1 puts the whole row's / plane's sum on the one pixel.
 * Limits and refusals are te_upsample_add_f32's.
 *
 * te_psp_codes_bwd_f32 (the adjoint of te_psp_codes_f32; the latent averages are constants): gz [B,D,T], gp [B,D,Np], lat [B,Ns+Np,D],
 * A [T,Ns] (folded, as the forward takes it) -> glat [B,Ns+Np,D], gA [T,Ns], gbz [T]:
 *     glat[b, j, c]      = sum_t A[t, j] * gz[b, c, t]  (j < Ns)          t ascending, one fp64 fma chain, rounded once
 *     glat[b, Ns + u, c] = gp[b, c, u]                                    a copy
 *     gA[t, j]           = sum over (b, c) of gz[b, c, t] * lat[b, j, c]   one wave: lane l takes (b, c) = l, l + 64, ... (b-major) as one
 *     gbz[t]             = sum over (b, c) of gz[b, c, t]                  fp64 chain, a fixed fp64 butterfly, rounded once
 * gA is the gradient of the FOLDED A: the caller multiplies it by EqualLinear's scale to reach the stored parameter.  Limits are
 * te_psp_codes_f32's.
 */
int te_conv2d_heads_dgrad_f32(float* gx, const float* g, const float* wt, const float* act, int B, int G, int Ci, int Cg, int H, int W, int kh,
                              int kw, int s, int py, int px, int gCtot, int gc0, float slope, te_stream_t stream);
int te_conv2d_heads_wgrad_splits(int Cg, int Ci, int kh, int kw, int64_t B, int Ho, int Wo);
int64_t te_conv2d_heads_wgrad_ws_bytes(int64_t B, int G, int Cg, int Ci, int kh, int kw, int Ho, int Wo);
int te_conv2d_heads_wgrad_f32(float* gw, float* gb, float* ws, int64_t ws_bytes, const float* g, const float* x, int B, int G, int Ci, int Cg,
                              int H, int W, int kh, int kw, int s, int py, int px, int gCtot, int gc0, int shared, int splits,
                              te_stream_t stream);
int te_upsample_add_bwd_f32(float* gx, const float* g, const float* add, int64_t planes, int h, int w, int H, int W, te_stream_t stream);
int te_psp_codes_bwd_f32(float* glat, float* gA, float* gbz, const float* gz, const float* gp, const float* lat, const float* A, int64_t B,
                         int Ns, int Np, int D, int T, te_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TE_HIP_H */
