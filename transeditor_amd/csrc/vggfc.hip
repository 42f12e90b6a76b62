// The classifier end of the PRDC feature extractor (metrics/calc_prdc.py:101-104: torchvision vgg16 with classifier[:-1], i.e. the
// 4096-d output of fc7 after its ReLU), the two pieces behind pool5 that the convolution family does not cover:
//
//     te_adaptive_avgpool_f32 : vgg16.avgpool = nn.AdaptiveAvgPool2d((7, 7)) (+ torch.flatten: the output IS the flattened layout)
//     te_fc_stream_f32        : classifier[0] / classifier[3] = nn.Linear(25088, 4096) / nn.Linear(4096, 4096), each with the ReLU
//                               that follows it (classifier[1] / [4]); Dropout (classifier[2] / [5]) is the identity in eval mode
//
// te_fc_stream_f32 is a weight-STREAMING GEMM: C[i,j] = act(sum_k A[i,k] W[j,k] + bias[j]) for few rows (a batch of images) against a
// weight far larger than any cache (fc6: 411 MB).  A workgroup owns a strip of 64 output columns, a block of up to 64 rows and one
// chunk of K: it reads its 64 x Kc panel of W exactly once, with 16-byte non-temporal loads along K, and the matching panel of A (the
// small operand: L2-resident, re-read by every strip).  4 waves, each one 32 x 32 tile of v_mfma_f32_32x32x2_f32 (an fp32 fma chain in
// a fixed order of k: exact fp32).  K is cut into S chunks so that (strips x S) workgroups fill the chip; the partial tiles go to the
// caller's workspace ws[S][I][J], and a second kernel sums them over s ascending, adds the bias and applies the activation.  No
// atomics.  S and the chunk length depend on (J, K) only and an output element's fma chain depends on its own row of A only, so a
// row's result is bitwise the same whatever batch it is computed in.
#include "te_common.h"

namespace {

constexpr int BT = 64;           // tile rows = tile columns
constexpr int BK = 32;
constexpr int LD = 36;           // LDS row pitch in floats (csrc/prdc.hip: 16-byte aligned stores, conflict-free ds_read_b128)
constexpr int NT = 256;
constexpr int kTargetWG = 1024;  // 4 workgroups (one wave per SIMD each) per CU: three to hide one's barriers and load latency
constexpr int kMinChunk = 128;   // a chunk shorter than this is mostly prologue
constexpr int kMaxSplit = 32;
constexpr int64_t kMaxRows = 64 * 65535;

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

struct Plan {
    int strips, S, Kc;
};

// the split of K: a function of (J, K) alone.  Kc is a multiple of BK; the last chunk may be shorter (its tail is zero-filled)
inline Plan plan(int J, int K) {
    Plan p;
    p.strips = (J + BT - 1) / BT;
    int want = (kTargetWG + p.strips - 1) / p.strips;
    int most = K / kMinChunk < 1 ? 1 : K / kMinChunk;
    if (most > kMaxSplit) most = kMaxSplit;
    if (want > most) want = most;
    const int per = (K + want - 1) / want;
    p.Kc = (per + BK - 1) / BK * BK;
    p.S = (K + p.Kc - 1) / p.Kc;
    return p;
}

// 64 rows x 32 k of a row-major [nrows, K] operand -> two 16-byte loads per thread; rows >= nrows and k >= k1 are zeros
template <bool STREAM>
__device__ __forceinline__ void load_panel(f32x4 (&r)[2], const float* __restrict__ base, int row0, int64_t nrows, int K, int k0, int k1) {
    const int t = threadIdx.x;
    const int k = k0 + (t & 7) * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t row = (int64_t)row0 + (t >> 3) + 32 * i;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < nrows && k < k1) {                         // K % 4 == 0 and k1 % 4 == 0: the four are inside the chunk or all past it
            const f32x4* p = reinterpret_cast<const f32x4*>(base + row * K + k);
            v = STREAM ? __builtin_nontemporal_load(p) : *p;
        }
        r[i] = v;
    }
}

__device__ __forceinline__ void store_panel(float* s, const f32x4 (&r)[2]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(s + ((t >> 3) + 32 * i) * LD + (t & 7) * 4) = r[i];
}

// Workgroup p of blockIdx.x -> (chunk, strip).  Workgroup ids go round-robin over the 8 XCDs; the remap hands every XCD one contiguous
// eighth of the chunk-major list, so the workgroups that share an L2 read few chunks of A (fc6: two, 0.8 MB).
__device__ __forceinline__ void block_coords(int strips, int& chunk, int& strip) {
    const int nwg = gridDim.x, p = blockIdx.x;
    const int q = nwg / te::kNumXCD, r = nwg % te::kNumXCD, xcd = p % te::kNumXCD;
    const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + p / te::kNumXCD;
    chunk = id / strips;
    strip = id % strips;
}

// ws[chunk][i][j] = sum over the chunk's k of A[i,k] * W[j,k] for the workgroup's 64 x 64 tile
__global__ __launch_bounds__(NT) void fc_stream_kernel(float* __restrict__ ws, const float* __restrict__ a, const float* __restrict__ w,
                                                       int64_t I, int J, int K, int Kc, int strips) {
    __shared__ __attribute__((aligned(16))) float As[BT * LD];
    __shared__ __attribute__((aligned(16))) float Bs[BT * LD];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid >> 1, wn = wid & 1, c = lane & 31, h = lane >> 5;
    int chunk, strip;
    block_coords(strips, chunk, strip);
    const int row0 = blockIdx.y * BT, col0 = strip * BT;
    const int k0 = chunk * Kc, k1 = k0 + Kc < K ? k0 + Kc : K;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    f32x4 ra[2], rb[2];
    load_panel<false>(ra, a, row0, I, K, k0, k1);
    load_panel<true>(rb, w, col0, J, K, k0, k1);
    // lane (c, h) feeds k = 8q + 4h + u of every 32-deep step to MFMA (q, u), for A and W alike: one fixed permutation of k
    const float* ap = As + (wm * 32 + c) * LD + 4 * h;
    const float* bp = Bs + (wn * 32 + c) * LD + 4 * h;
    for (int kk = k0; kk < k1; kk += BK) {
        __syncthreads();                                     // the previous step's LDS reads are done
        store_panel(As, ra);
        store_panel(Bs, rb);
        __syncthreads();
        if (kk + BK < k1) {                                  // in flight behind the MFMAs below
            load_panel<false>(ra, a, row0, I, K, kk + BK, k1);
            load_panel<true>(rb, w, col0, J, K, kk + BK, k1);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(ap + 8 * q);
            const f32x4 y = *reinterpret_cast<const f32x4*>(bp + 8 * q);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, y.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, y.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, y.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, y.w, acc, 0, 0, 0);
        }
    }
    // accumulator register e of lane (c, h): row (e & 3) + 8 (e >> 2) + 4 h, column c of the wave's 32 x 32 tile
    const int col = col0 + wn * 32 + c;
    if (col < J) {
        float* dst = ws + (int64_t)chunk * I * J + col;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t row = (int64_t)row0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (row < I) dst[row * J] = acc[e];
        }
    }
}

// c[i,j] = act(((ws[0] + ws[1]) + ... + ws[S-1])[i,j] + bias[j]): one thread per element, s ascending
__global__ __launch_bounds__(256) void fc_reduce_kernel(float* __restrict__ c, const float* __restrict__ ws, const float* __restrict__ bias,
                                                        int64_t IJ, int J, int S, int act) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= IJ) return;
    float v = ws[o];
    for (int s = 1; s < S; ++s) v += ws[(int64_t)s * IJ + o];
    v += bias[o % J];
    if (act == 1) v = te::relu_nan(v);
    c[o] = v;
}

// out[p, oy, ox] = mean of x[p, floor(oy H / OH) : ceil((oy + 1) H / OH), floor(ox W / OW) : ceil((ox + 1) W / OW)], summed row-major
__global__ __launch_bounds__(256) void adaptive_avgpool_kernel(float* __restrict__ out, const float* __restrict__ x, int64_t total,
                                                               int H, int W, int OH, int OW) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int ox = (int)(o % OW), oy = (int)(o / OW % OH);
    const int64_t p = o / OW / OH;
    int y0, y1, x0, x1;
    te::adaptive_window<int64_t>(oy, H, OH, y0, y1);
    te::adaptive_window<int64_t>(ox, W, OW, x0, x1);
    const float* src = x + p * H * W;
    float s = 0.f;
    bool first = true;
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) {
            const float v = src[(int64_t)yy * W + xx];
            s = first ? v : s + v;                           // (a window of one element is copied bit for bit, -0 included)
            first = false;
        }
    out[o] = s / (float)((y1 - y0) * (x1 - x0));
}
inline bool fc_dims_ok(int J, int K) { return J >= 1 && K >= 4 && K % 4 == 0; }

}  // namespace

extern "C" int te_fc_stream_splits(int J, int K) {
    if (!fc_dims_ok(J, K)) return TE_ERR_SHAPE;
    return plan(J, K).S;
}

extern "C" int64_t te_fc_stream_ws_bytes(int64_t I, int J, int K) {
    if (!fc_dims_ok(J, K) || I < 1 || I > kMaxRows) return TE_ERR_SHAPE;
    return (int64_t)plan(J, K).S * I * J * 4;
}

extern "C" int te_fc_stream_f32(float* c, float* ws, const float* a, const float* w, const float* bias, int64_t I, int J, int K, int act,
                                te_stream_t stream) {
    TE_REQUIRE(c && ws && a && w && bias, TE_ERR_NULL, "te_fc_stream_f32: NULL pointer");
    TE_REQUIRE(I >= 1 && I <= kMaxRows && J >= 1, TE_ERR_SHAPE, "te_fc_stream_f32: 1 <= I <= %lld, J >= 1 (got %lld, %d)",
               (long long)kMaxRows, (long long)I, J);
    TE_REQUIRE(K >= 4 && K % 4 == 0, TE_ERR_SHAPE, "te_fc_stream_f32: K must be a positive multiple of 4 (got %d)", K);
    TE_REQUIRE(te::aligned16(a) && te::aligned16(w), TE_ERR_SHAPE, "te_fc_stream_f32: a and w must be 16-byte aligned");
    TE_REQUIRE(act == 0 || act == 1, TE_ERR_UNSUPPORTED, "te_fc_stream_f32: act must be 0 (none) or 1 (ReLU), got %d", act);
    hipStream_t st = (hipStream_t)stream;
    const Plan p = plan(J, K);
    const int64_t IJ = I * J;
    TE_REQUIRE(te::cdiv(IJ, 256) <= 0x7fffffff, TE_ERR_SHAPE, "te_fc_stream_f32: too many outputs (%lld)", (long long)IJ);
    fc_stream_kernel<<<dim3((unsigned)(p.strips * p.S), (unsigned)te::cdiv(I, BT)), NT, 0, st>>>(ws, a, w, I, J, K, p.Kc, p.strips);
    fc_reduce_kernel<<<(unsigned)te::cdiv(IJ, 256), 256, 0, st>>>(c, ws, bias, IJ, J, p.S, act);
    return te::launch_status("te_fc_stream_f32");
}

extern "C" int te_adaptive_avgpool_f32(float* out, const float* x, int64_t planes, int H, int W, int OH, int OW, te_stream_t stream) {
    TE_REQUIRE(out && x, TE_ERR_NULL, "te_adaptive_avgpool_f32: NULL pointer");
    TE_REQUIRE(planes >= 1 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1, TE_ERR_SHAPE,
               "te_adaptive_avgpool_f32: planes, H, W, OH, OW must be positive (got %lld, %d, %d, %d, %d)", (long long)planes, H, W, OH, OW);
    const int64_t total = planes * OH * OW;
    TE_REQUIRE(te::cdiv(total, 256) <= 0x7fffffff, TE_ERR_SHAPE, "te_adaptive_avgpool_f32: too many outputs (%lld)", (long long)total);
    adaptive_avgpool_kernel<<<(unsigned)te::cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(out, x, total, H, W, OH, OW);
    return te::launch_status("te_adaptive_avgpool_f32");
}
