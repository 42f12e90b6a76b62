// What a torchvision ResNet needs beyond te_conv2d_f32: the pose classifier of attribute editing (our_interfaceGAN/ffhq_utils/dex/
// models.py:73-89 ClassifyModel = resnet18 without its fc + Linear(512, 2) + softmax, called through api.py:61-65) is the first user.
//
//     te_conv2d_res_f32     : te_conv2d_f32 with the residual of a BasicBlock added before the ReLU (out = relu(bn2(conv2(.)) + identity))
//     te_pose_stem_fwd_f32  : the scorers' preprocessing (RGB [-1, 1] -> BGR byte levels), the centre crop and conv1 (7 x 7, stride 2,
//                             pad 3, the batch norm folded in) + ReLU in one pass over the image
//     te_maxpool3s2p1_f32   : nn.MaxPool2d(3, 2, 1)
//
// Both convolutions are the main loop of conv2d_body.h with another policy: the residual is an epilogue (the accumulators, hence the
// bits before the residual, are te_conv2d_f32's), the stem is a gather (a tap of the 147-deep patch is read from the window of the
// full image and, for a generator image, mapped to its byte level on the way into LDS; taps outside the WINDOW are the zero padding,
// the image around it is never read).  Forward only, no atomics, no workspace.
#include "te_common.h"
#include "byte_level.h"
#include "conv2d_body.h"

namespace {

using namespace te::conv2d;

struct ResArgs : ConvArgs {
    const float* res;            // [B,Co,Ho,Wo], the layout of out (Ctot == Co, c0 == 0)
};

struct StemArgs : ConvArgs {     // H = W = crop: the convolution sees the window
    int IH, IW, y0, x0;          // the image's size and the window's corner in it
};

// out = act((acc + bias) + res): two separately rounded additions
struct EpiResidual {
    static __device__ __forceinline__ float apply(const ResArgs& a, float v, const float* dst, int m, int HoWo) {
        v = v + a.res[(dst - a.out) + (int64_t)m * HoWo];
        if (a.act == 1) v = te::relu_nan(v);
        return v;
    }
};

// a tap of the centre window of img [N,3,IH,IW].  BYTE: the image is RGB in [-1, 1]: channel c reads plane 2 - c through
// te::to_byte_level; else it holds BGR byte levels already.
template <bool BYTE>
struct GatherCrop {
    static __device__ __forceinline__ const float* image(const StemArgs& a, int64_t b) {
        return a.x + b * 3 * a.IH * a.IW + a.y0 * a.IW + a.x0;
    }
    static __device__ __forceinline__ int plane(const StemArgs& a) { return a.IH * a.IW; }
    static __device__ __forceinline__ float tap(const float* img, const StemArgs& a, int HW, int c, int iy, int ix) {
        const float v = img[(BYTE ? 2 - c : c) * HW + iy * a.IW + ix];
        return BYTE ? te::to_byte_level(v) : v;
    }
};

// one thread per output element, lanes along ox; the first tap inside the plane starts the maximum (the centre tap always is), then
// a greater value or a NaN replaces (te_maxpool2_fwd_f32)
__global__ __launch_bounds__(256) void maxpool3s2p1_kernel(float* __restrict__ out, const float* __restrict__ x, int64_t total, int H, int W,
                                                           int Ho, int Wo) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int ox = (int)(o % Wo), oy = (int)(o / Wo % Ho);
    const int64_t plane = o / Wo / Ho;
    const float* src = x + plane * H * W;
    float v = 0.f;
    bool first = true;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * 2 - 1 + ky;
        if ((unsigned)iy >= (unsigned)H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * 2 - 1 + kx;
            if ((unsigned)ix >= (unsigned)W) continue;
            const float t = src[(int64_t)iy * W + ix];
            if (first || t > v || t != t) v = t;
            first = false;
        }
    }
    out[o] = v;
}

}  // namespace

extern "C" int te_conv2d_res_f32(float* out, const float* x, const float* w, const float* bias, const float* res, int B, int Ci, int Co, int H,
                                 int W, int kh, int kw, int s, int py, int px, int act, te_stream_t stream) {
    TE_REQUIRE(out && x && w && bias && res, TE_ERR_NULL, "te_conv2d_res_f32: NULL pointer");
    ResArgs a;
    a.out = out; a.x = x; a.w = w; a.bias = bias; a.res = res;
    if (const int rc = fill_args(a, "te_conv2d_res_f32", B, Ci, Co, H, W, kh, kw, s, py, px, Co, 0, act)) return rc;
    launch<GatherPlain, EpiResidual>(a, (hipStream_t)stream);
    return te::launch_status("te_conv2d_res_f32");
}

extern "C" int te_pose_stem_fwd_f32(float* out, const float* img, const float* w, const float* b, int N, int H, int W, int crop, int Co,
                                    int preprocessed, te_stream_t stream) {
    TE_REQUIRE(out && img && w && b, TE_ERR_NULL, "te_pose_stem_fwd_f32: NULL pointer");
    TE_REQUIRE(preprocessed == 0 || preprocessed == 1, TE_ERR_UNSUPPORTED,
               "te_pose_stem_fwd_f32: preprocessed must be 0 (RGB in [-1, 1]) or 1 (BGR byte levels), got %d", preprocessed);
    if (const int rc = te::check_centre_crop("te_pose_stem_fwd_f32", N, H, W, crop, Co)) return rc;
    TE_REQUIRE((int64_t)3 * H * W <= 0x7fffffff, TE_ERR_SHAPE, "te_pose_stem_fwd_f32: one image (3 * H * W) must fit 31 bits");
    StemArgs a;
    a.out = out; a.x = img; a.w = w; a.bias = b;
    if (const int rc = fill_args(a, "te_pose_stem_fwd_f32", N, 3, Co, crop, crop, 7, 7, 2, 3, 3, Co, 0, 1)) return rc;
    a.IH = H; a.IW = W; a.y0 = (H - crop) / 2; a.x0 = (W - crop) / 2;
    hipStream_t st = (hipStream_t)stream;
    if (preprocessed == 0) launch<GatherCrop<true>, EpiBiasAct, PartWhole, false>(a, st);        // K = 147: the unaligned weight path
    else launch<GatherCrop<false>, EpiBiasAct, PartWhole, false>(a, st);
    return te::launch_status("te_pose_stem_fwd_f32");
}

extern "C" int te_maxpool3s2p1_f32(float* out, const float* x, int64_t planes, int H, int W, te_stream_t stream) {
    TE_REQUIRE(out && x, TE_ERR_NULL, "te_maxpool3s2p1_f32: NULL pointer");
    TE_REQUIRE(planes >= 1 && H >= 1 && W >= 1, TE_ERR_SHAPE, "te_maxpool3s2p1_f32: planes, H, W must be positive (got %lld, %d, %d)",
               (long long)planes, H, W);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    TE_REQUIRE((int64_t)H * W <= 0x7fffffff && planes <= ((int64_t)1 << 40) / ((int64_t)H * W), TE_ERR_SHAPE,
               "te_maxpool3s2p1_f32: a plane must fit 31 bits and the input 2^40 elements (got %lld planes of %d x %d)", (long long)planes, H, W);
    const int64_t total = planes * Ho * Wo;
    TE_REQUIRE(te::cdiv(total, 256) <= 0x7fffffff, TE_ERR_SHAPE, "te_maxpool3s2p1_f32: too many outputs (%lld)", (long long)total);
    maxpool3s2p1_kernel<<<(unsigned)te::cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(out, x, total, H, W, Ho, Wo);
    return te::launch_status("te_maxpool3s2p1_f32");
}
