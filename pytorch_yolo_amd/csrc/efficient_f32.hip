// fp32 "reference-precision" forms of the element kernels of the depthwise encoder families (MobileNetV2, ShuffleNetV2,
// EfficientNet-B0) for gfx950 (MI355X): what conv_f32.hip is to the conv kernels.  float32 NHWC views (multiples of 4 channels:
// 16 bytes per lane is one f32x4), float32 arithmetic, expf and an IEEE division in the activations, explicit fmaf chains in a
// fixed order - the arithmetic of the reference's fp32 ATen ops up to summation order, independent of the grid.  The bf16 kernels
// (efficient.hip, pointwise.hip) are separate device code and stay what they are.
//   * depthwise k x k conv (k = 3 or 5) with an explicit leading pad and a caller-given output size: torch's pad 1
//     (torchvision InvertedResidual behind reference models/yolov3_tiny_mobilenet.py:11-34, the ShuffleNetV2 units behind
//     models/yolov3_tiny_shuffle.py:13-47) and TensorFlow "same" (efficientnet_pytorch 0.2.0 Conv2dSamePadding behind
//     models/yolov3_tiny_efficient.py:22-45: the odd pad row / column lies below / right); everything outside the image reads zero.
//     ONE form: a thread computes 4 channels of one output pixel, lanes run along the channels (coalesced 16-byte loads); the
//     taps of neighbouring pixels meet in L2.  A parity mode: no strip form was written.
//   * squeeze-and-excitation in three passes like yolo_se_fwd: partial sums over pixel ranges that meet in a fixed order, the two
//     FCs (swish between them, sigmoid after), the channel-wise rescale.  Deterministic from run to run.
//   * channel_shuffle(cat(a, b), 2) in the two-slot layout of yolo_channel_shuffle2_fwd.
#include "common.h"

namespace {

__device__ __forceinline__ float act_f(float v, int act) {
  if (act == YOLO_ACT_SWISH) return v / (1.f + expf(-v));          // x * sigmoid(x)
  if (act == YOLO_ACT_LEAKY01) return fmaxf(v, 0.1f * v);
  if (act == YOLO_ACT_RELU6) return fminf(fmaxf(v, 0.f), 6.f);
  if (act == YOLO_ACT_RELU) return fmaxf(v, 0.f);
  return v;
}

constexpr long kMaxThreads = 0x7fffffffL * 256;      // what a 1-D grid of 256-thread blocks can hold
inline unsigned blocks_for(long total) { return (unsigned)((total + 255) / 256); }

// one thread = 4 channels of one output pixel; w: f32 [k*k][c] tap-major, bias f32 [c].  acc = bias, then one fmaf per tap in
// tap order (kh, kw); a tap outside the image adds nothing.
__global__ __launch_bounds__(256) void dwconv_f32_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                         const float* __restrict__ bias, float* __restrict__ y, int h, int w, int c,
                                                         int in_ct, int in_co, int ho, int wo, int out_ct, int out_co, int k,
                                                         int stride, int pad, int act, long total) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int cg = c >> 2;
  const int g = (int)(t % cg);
  long p = t / cg;
  const int ow = (int)(p % wo);
  p /= wo;
  const int oh = (int)(p % ho);
  const long b = p / ho;
  f32x4 acc = *reinterpret_cast<const f32x4*>(bias + g * 4);
  for (int i = 0; i < k; ++i) {
    const int hi = oh * stride - pad + i;
    if ((unsigned)hi >= (unsigned)h) continue;
    for (int j = 0; j < k; ++j) {
      const int wi = ow * stride - pad + j;
      if ((unsigned)wi >= (unsigned)w) continue;
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((b * h + hi) * w + wi) * in_ct + in_co + g * 4);
      const f32x4 wv = *reinterpret_cast<const f32x4*>(wt + (long)(i * k + j) * c + g * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(v[e], wv[e], acc[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = act_f(acc[e], act);
  *reinterpret_cast<f32x4*>(y + ((b * ho + oh) * wo + ow) * out_ct + out_co + g * 4) = acc;
}

// ---- squeeze-and-excitation ---------------------------------------------------------------------------------------------
constexpr int kSeMaxSplits = 32;   // as efficient.hip: the workspace of yolo_se_workspace_bytes holds 32 partial rows per image

// (1) per (image, group of <= 32 4-channel chunks, pixel range): partial sums over the range.  Block = 256 threads:
//     thread = (pixel stripe t / cgb, chunk t % cgb); a stripe adds its pixels in ascending order, the stripes meet in LDS in
//     ascending order.
__global__ __launch_bounds__(256) void se_partial_f32_kernel(const float* __restrict__ x, float* __restrict__ partial, int hw, int c,
                                                             int in_ct, int in_co, int cgb, int splits) {
  __shared__ f32x4 part[256];
  const int cg = c >> 2;
  const int groups = (cg + cgb - 1) / cgb;
  int bid = blockIdx.x;
  const int sp = bid % splits;
  bid /= splits;
  const int b = bid / groups, grp = bid % groups;
  const int lc = threadIdx.x % cgb, stripe = threadIdx.x / cgb, nstripes = 256 / cgb;
  const int g = grp * cgb + lc;
  const int per = (hw + splits - 1) / splits, p_lo = sp * per, p_hi = min(hw, p_lo + per);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (g < cg)
    for (int p = p_lo + stripe; p < p_hi; p += nstripes) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((long)b * hw + p) * in_ct + in_co + g * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += v[e];
    }
  part[threadIdx.x] = s;
  __syncthreads();
  if (stripe == 0 && g < cg) {
    f32x4 tot = {0.f, 0.f, 0.f, 0.f};
    for (int st = 0; st < nstripes; ++st) {          // fixed order: deterministic
      const f32x4 v = part[st * cgb + lc];
#pragma unroll
      for (int e = 0; e < 4; ++e) tot[e] += v[e];
    }
    *reinterpret_cast<f32x4*>(partial + ((long)b * splits + sp) * c + g * 4) = tot;
  }
}

// (2) per image: mean = sum of the partials (in split order) / hw; hidden = swish(W1 mean + b1) (sq <= 64 values);
//     scale = sigmoid(W2 hidden + b2).  W1: f32 [sq][c], W2T: f32 [sq][c].
__global__ __launch_bounds__(1024) void se_fc_f32_kernel(const float* __restrict__ partial, float* __restrict__ mean,
                                                         const float* __restrict__ w1, const float* __restrict__ b1,
                                                         const float* __restrict__ w2t, const float* __restrict__ b2,
                                                         float* __restrict__ scale, int c, int sq, int splits, float hw) {
  __shared__ float hid[64];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* const m = mean + (long)b * c;
  for (int i = threadIdx.x; i < c; i += 1024) {
    float t = 0.f;
    for (int sp = 0; sp < splits; ++sp) t += partial[((long)b * splits + sp) * c + i];
    m[i] = t / hw;                                   // a division like the reference's mean, not a multiply by 1 / hw
  }
  __syncthreads();
  for (int j = wave; j < sq; j += 16) {              // one wave per hidden unit: lanes stride the channels
    float s = 0.f;
    for (int i = lane; i < c; i += 64) s = fmaf(w1[(long)j * c + i], m[i], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) {
      const float v = s + b1[j];
      hid[j] = v / (1.f + expf(-v));
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < c; i += 1024) {
    float s = b2[i];
    for (int j = 0; j < sq; ++j) s = fmaf(w2t[(long)j * c + i], hid[j], s);
    scale[(long)b * c + i] = 1.f / (1.f + expf(-s));
  }
}

// (3) y = x * scale[image][channel]
__global__ __launch_bounds__(256) void se_scale_f32_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                           float* __restrict__ y, int hw, int c, int in_ct, int in_co, int out_ct,
                                                           int out_co, long total) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int cg = c >> 2;
  const int g = (int)(t % cg);
  const long p = t / cg, b = p / hw;
  const f32x4 v = *reinterpret_cast<const f32x4*>(x + p * in_ct + in_co + g * 4);
  const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + b * c + g * 4);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = v[e] * sc[e];
  *reinterpret_cast<f32x4*>(y + p * out_ct + out_co + g * 4) = o;
}

// channel_shuffle(cat(a, b), 2) in the two-slot layout (see include/yolo_hip.h): thread = 4 physical output channels of a pixel;
// the pad channels of both slots are written as zero
__global__ __launch_bounds__(256) void shuffle2_f32_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           float* __restrict__ y, int half, int c_slot, int a_ct, int a_co, int b_ct,
                                                           int b_co, int y_ct, int y_co, long total) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int groups = 2 * c_slot / 4;
  const int g = (int)(t % groups);
  const long pix = t / groups;
  const float* const pa = a + pix * a_ct + a_co;
  const float* const pb = b + pix * b_ct + b_co;
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int pc = g * 4 + e, slot = pc / c_slot, r = pc - slot * c_slot;
    const int j = slot * half + r;                    // logical output channel (only read where r < half: j / 2 < half)
    o[e] = r < half ? ((j & 1) ? pb[j >> 1] : pa[j >> 1]) : 0.f;
  }
  *reinterpret_cast<f32x4*>(y + pix * y_ct + y_co + g * 4) = o;
}

}  // namespace

extern "C" int yolo_dwconv_f32_fwd(const float* x, const float* w, const float* bias, float* y, int n, int h, int w_, int c,
                                   int in_c_total, int in_c_offset, int ho, int wo, int out_c_total, int out_c_offset, int ksize,
                                   int stride, int pad, int act, yolo_stream_t s) {
  YOLO_REQUIRE(x && w && bias && y && n > 0 && h > 0 && w_ > 0 && c > 0 && c % 4 == 0, "dwconv_f32: bad arguments");
  YOLO_REQUIRE((ksize == 3 || ksize == 5) && (stride == 1 || stride == 2) && pad >= 0 && pad < ksize, "dwconv_f32: k %d stride %d pad %d",
               ksize, stride, pad);
  YOLO_REQUIRE(act >= YOLO_ACT_NONE && act <= YOLO_ACT_SWISH, "dwconv_f32: activation %d", act);
  // the last output's window must start inside the padded image and need at most k - 1 - pad rows of trailing zeros
  YOLO_REQUIRE(ho >= 1 && wo >= 1 && (ho - 1) * stride - pad < h && (wo - 1) * stride - pad < w_ &&
                   (ho - 1) * stride - pad + ksize <= h + ksize - 1 && (wo - 1) * stride - pad + ksize <= w_ + ksize - 1,
               "dwconv_f32: output size %dx%d inconsistent with input %dx%d k%d s%d pad %d", ho, wo, h, w_, ksize, stride, pad);
  YOLO_REQUIRE(in_c_total % 4 == 0 && in_c_offset % 4 == 0 && out_c_total % 4 == 0 && out_c_offset % 4 == 0 && in_c_offset >= 0 &&
                   out_c_offset >= 0 && in_c_offset + c <= in_c_total && out_c_offset + c <= out_c_total,
               "dwconv_f32: views must be 4-channel aligned");
  const long total = (long)n * ho * wo * (c / 4);
  YOLO_REQUIRE(total <= kMaxThreads, "dwconv_f32: grid too large");
  hipLaunchKernelGGL(dwconv_f32_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, x, w, bias, y, h, w_, c, in_c_total,
                     in_c_offset, ho, wo, out_c_total, out_c_offset, ksize, stride, pad, act, total);
  return yolo_check_launch("yolo_dwconv_f32_fwd");
}

extern "C" int yolo_se_f32_fwd(const float* x, float* y, int n, int h, int w_, int c, int in_c_total, int in_c_offset,
                               int out_c_total, int out_c_offset, const float* w1, const float* b1, const float* w2, const float* b2,
                               int squeeze, void* workspace, size_t ws_bytes, yolo_stream_t s) {
  YOLO_REQUIRE(x && y && w1 && b1 && w2 && b2 && workspace && n > 0 && h > 0 && w_ > 0 && c > 0 && c % 4 == 0, "se_f32: bad arguments");
  YOLO_REQUIRE(squeeze >= 1 && squeeze <= 64, "se_f32: %d squeezed channels (1..64)", squeeze);
  YOLO_REQUIRE(ws_bytes >= yolo_se_workspace_bytes(n, c), "se_f32: workspace too small");
  YOLO_REQUIRE(in_c_total % 4 == 0 && in_c_offset % 4 == 0 && out_c_total % 4 == 0 && out_c_offset % 4 == 0 && in_c_offset >= 0 &&
                   out_c_offset >= 0 && in_c_offset + c <= in_c_total && out_c_offset + c <= out_c_total,
               "se_f32: views must be 4-channel aligned");
  // the layout of yolo_se_fwd's workspace: means, scales, then up to kSeMaxSplits partial rows per image
  float* const mean = (float*)workspace;
  float* const scale = mean + (size_t)n * c;
  float* const partial = scale + (size_t)n * c;
  const int hw = h * w_, cg = c / 4;
  const int cgb = cg < 32 ? (cg >= 16 ? 16 : cg >= 8 ? 8 : cg >= 4 ? 4 : cg >= 2 ? 2 : 1) : 32;    // power of two <= 32: 256 % cgb == 0
  const int groups = (cg + cgb - 1) / cgb;
  int splits = 1;      // enough workgroups for the chip on the large maps; a range keeps >= 256 pixels
  while (splits < kSeMaxSplits && (long)n * groups * splits < 512 && hw / (splits * 2) >= 256) splits *= 2;
  const long total = (long)n * hw * cg;
  YOLO_REQUIRE((long)n * groups * splits <= 0x7fffffffL && total <= kMaxThreads, "se_f32: grid too large");
  hipLaunchKernelGGL(se_partial_f32_kernel, dim3((unsigned)(n * groups * splits)), dim3(256), 0, (hipStream_t)s, x, partial, hw, c,
                     in_c_total, in_c_offset, cgb, splits);
  int rc = yolo_check_launch("yolo_se_f32_fwd(pool)");
  if (rc) return rc;
  hipLaunchKernelGGL(se_fc_f32_kernel, dim3((unsigned)n), dim3(1024), 0, (hipStream_t)s, partial, mean, w1, b1, w2, b2, scale, c, squeeze,
                     splits, (float)hw);
  rc = yolo_check_launch("yolo_se_f32_fwd(fc)");
  if (rc) return rc;
  hipLaunchKernelGGL(se_scale_f32_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, x, scale, y, hw, c, in_c_total,
                     in_c_offset, out_c_total, out_c_offset, total);
  return yolo_check_launch("yolo_se_f32_fwd(scale)");
}

extern "C" int yolo_channel_shuffle2_f32_fwd(const float* a, const float* b, float* y, int n, int h, int w, int half, int c_slot,
                                             int a_c_total, int a_c_offset, int b_c_total, int b_c_offset, int y_c_total,
                                             int y_c_offset, yolo_stream_t s) {
  YOLO_REQUIRE(a && b && y && n > 0 && h > 0 && w > 0, "shuffle2_f32: bad arguments");
  YOLO_REQUIRE(half >= 1 && half <= c_slot && c_slot % 4 == 0, "shuffle2_f32: %d logical channels per slot of %d", half, c_slot);
  YOLO_REQUIRE(a_c_offset >= 0 && b_c_offset >= 0 && y_c_offset >= 0 && a_c_offset + c_slot <= a_c_total &&
                   b_c_offset + c_slot <= b_c_total && y_c_offset + 2 * c_slot <= y_c_total && y_c_offset % 4 == 0 && y_c_total % 4 == 0,
               "shuffle2_f32: bad views");
  const long total = (long)n * h * w * (2 * c_slot / 4);
  YOLO_REQUIRE(total <= kMaxThreads, "shuffle2_f32: grid too large");
  hipLaunchKernelGGL(shuffle2_f32_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, a, b, y, half, c_slot, a_c_total,
                     a_c_offset, b_c_total, b_c_offset, y_c_total, y_c_offset, total);
  return yolo_check_launch("yolo_channel_shuffle2_f32_fwd");
}
