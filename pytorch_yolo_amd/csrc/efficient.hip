// Element kernels the depthwise encoder families (MobileNetV2, ShuffleNetV2, EfficientNet-B0) need beyond the Darknet set
// (reference models/yolov3_tiny_efficient.py:13-72; the blocks themselves live in efficientnet_pytorch 0.2.0's MBConvBlock):
//   * depthwise k x k convolution (k = 3 or 5) with an explicit leading pad and a caller-given output size: torch's pad 1, or
//     TensorFlow "same" padding, which puts the odd pad row / column at the bottom / right (stride 2 on an even map: pad 0 + 1 for
//     k = 3, 1 + 2 for k = 5); everything beyond the image reads zero;
//   * squeeze-and-excitation: global average pool, the two 1x1 convs on the pooled vector (swish between them), sigmoid,
//     channel-wise rescale of the block's tensor.  Three passes, deterministic from run to run.
// All are HBM-bound 16-byte-per-lane streams over NHWC views like pointwise.hip, ONE template per kernel for both element types
// (Lanes<T>, common.h): bf16 (8 channels per lane) and, for model.precision = "fp32", float (4 channels per lane).  Arithmetic in
// fp32: expf and an IEEE division in the activations, explicit fmaf chains in a fixed order, independent of the grid - for float
// the arithmetic of the reference's fp32 ATen ops up to summation order.  Built with -ffp-contract=off (build.py) so that the
// float instances round every product they write as one.
#include "common.h"

namespace {

// one thread = V channels of one output pixel; w: f32 [k*k][c] tap-major, bias f32 [c].  acc = bias, then one fmaf per tap in
// tap order (kh, kw); a tap outside the image adds nothing.
template <typename T>
__global__ __launch_bounds__(256) void dwconv_kernel(const T* __restrict__ x, const float* __restrict__ wt,
                                                     const float* __restrict__ bias, T* __restrict__ y, int h, int w, int c,
                                                     int in_ct, int in_co, int ho, int wo, int out_ct, int out_co, int k, int stride,
                                                     int pad, int act, long total) {
  typedef Lanes<T> L;
  constexpr int V = L::V;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int cg = (unsigned)c / V;
  const int g = (int)(t % cg);
  long p = t / cg;
  const int ow = (int)(p % wo);
  p /= wo;
  const int oh = (int)(p % ho);
  const long b = p / ho;
  float acc[V];
#pragma unroll
  for (int q = 0; q < V; q += 4) {
    const f32x4 bq = *reinterpret_cast<const f32x4*>(bias + g * V + q);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[q + e] = bq[e];
  }
  for (int i = 0; i < k; ++i) {
    const int hi = oh * stride - pad + i;
    if ((unsigned)hi >= (unsigned)h) continue;
    for (int j = 0; j < k; ++j) {
      const int wi = ow * stride - pad + j;
      if ((unsigned)wi >= (unsigned)w) continue;
      const typename L::vec v = *reinterpret_cast<const typename L::vec*>(x + ((b * h + hi) * w + wi) * in_ct + in_co + g * V);
      const float* wp = wt + (long)(i * k + j) * c + g * V;
#pragma unroll
      for (int q = 0; q < V; q += 4) {
        const f32x4 wq = *reinterpret_cast<const f32x4*>(wp + q);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[q + e] = fmaf(L::widen(v[q + e]), wq[e], acc[q + e]);
      }
    }
  }
  typename L::vec o;
#pragma unroll
  for (int e = 0; e < V; ++e) o[e] = L::narrow(act_f(acc[e], act));
  *reinterpret_cast<typename L::vec*>(y + ((b * ho + oh) * wo + ow) * out_ct + out_co + g * V) = o;
}

// ---- squeeze-and-excitation ---------------------------------------------------------------------------------------------
constexpr int kSeMaxSplits = 32;   // pixel ranges a map is cut into for the pooling pass (partial sums, added in a fixed order)

// (1) per (image, group of <= 32 V-channel chunks, pixel range): partial sums over the range.  Block = 256 threads:
//     thread = (pixel stripe t / cgb, chunk t % cgb); a stripe adds its pixels in ascending order, the stripes meet in LDS in
//     ascending order.
template <typename T>
__global__ __launch_bounds__(256) void se_partial_kernel(const T* __restrict__ x, float* __restrict__ partial, int hw, int c,
                                                         int in_ct, int in_co, int cgb, int splits) {
  typedef Lanes<T> L;
  constexpr int V = L::V;
  __shared__ float part[256][V];
  const int cg = (unsigned)c / V;
  const int groups = (cg + cgb - 1) / cgb;
  int bid = blockIdx.x;
  const int sp = bid % splits;
  bid /= splits;
  const int b = bid / groups, grp = bid % groups;
  const int lc = threadIdx.x % cgb, stripe = threadIdx.x / cgb, nstripes = 256 / cgb;
  const int g = grp * cgb + lc;
  const int per = (hw + splits - 1) / splits, p_lo = sp * per, p_hi = min(hw, p_lo + per);
  float s[V] = {};
  if (g < cg)
    for (int p = p_lo + stripe; p < p_hi; p += nstripes) {
      const typename L::vec v = *reinterpret_cast<const typename L::vec*>(x + ((long)b * hw + p) * in_ct + in_co + g * V);
#pragma unroll
      for (int e = 0; e < V; ++e) s[e] += L::widen(v[e]);
    }
#pragma unroll
  for (int e = 0; e < V; ++e) part[threadIdx.x][e] = s[e];
  __syncthreads();
  if (stripe == 0 && g < cg) {
    float tot[V] = {};
    for (int st = 0; st < nstripes; ++st)            // fixed order: deterministic
#pragma unroll
      for (int e = 0; e < V; ++e) tot[e] += part[st * cgb + lc][e];
#pragma unroll
    for (int e = 0; e < V; ++e) partial[((long)b * splits + sp) * c + g * V + e] = tot[e];
  }
}

// (2) per image: mean = sum of the partials (in split order) over hw; hidden = swish(W1 mean + b1) (sq values);
//     scale = sigmoid(W2 hidden + b2).  W1: f32 [sq][c], W2T: f32 [sq][c] (the expand weight transposed: lanes read consecutive
//     channels); sq <= 64.  The one place where the two precisions round differently: the bf16 mode multiplies by
//     hw_term = 1 / hw, the fp32 mode (DIVIDE) divides by hw_term = hw like the reference's mean.
template <bool DIVIDE>
__global__ __launch_bounds__(1024) void se_fc_kernel(const float* __restrict__ partial, float* __restrict__ mean, const float* __restrict__ w1,
                                                     const float* __restrict__ b1, const float* __restrict__ w2t, const float* __restrict__ b2,
                                                     float* __restrict__ scale, int c, int sq, int splits, float hw_term) {
  __shared__ float hid[64];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* const m = mean + (long)b * c;
  for (int i = threadIdx.x; i < c; i += 1024) {
    float t = 0.f;
    for (int sp = 0; sp < splits; ++sp) t += partial[((long)b * splits + sp) * c + i];
    m[i] = DIVIDE ? t / hw_term : t * hw_term;
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
template <typename T>
__global__ __launch_bounds__(256) void se_scale_kernel(const T* __restrict__ x, const float* __restrict__ scale, T* __restrict__ y,
                                                       int hw, int c, int in_ct, int in_co, int out_ct, int out_co, long total) {
  typedef Lanes<T> L;
  constexpr int V = L::V;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int cg = (unsigned)c / V;
  const int g = (int)(t % cg);
  const long p = t / cg, b = p / hw;
  const typename L::vec v = *reinterpret_cast<const typename L::vec*>(x + p * in_ct + in_co + g * V);
  const float* sp = scale + b * c + g * V;
  typename L::vec o;
#pragma unroll
  for (int q = 0; q < V; q += 4) {
    const f32x4 sq = *reinterpret_cast<const f32x4*>(sp + q);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[q + e] = L::narrow(L::widen(v[q + e]) * sq[e]);
  }
  *reinterpret_cast<typename L::vec*>(y + p * out_ct + out_co + g * V) = o;
}

}  // namespace

// the host side of both precisions; fn = the entry point's name
template <typename T>
static int dwconv_fwd(const char* fn, const void* x, const float* w, const float* bias, void* y, int n, int h, int w_, int c,
                      int in_c_total, int in_c_offset, int ho, int wo, int out_c_total, int out_c_offset, int ksize, int stride, int pad,
                      int act, yolo_stream_t s) {
  constexpr int V = Lanes<T>::V;
  YOLO_REQUIRE(x && w && bias && y && n > 0 && h > 0 && w_ > 0 && c > 0 && c % V == 0, "%s: bad arguments", fn);
  YOLO_REQUIRE((ksize == 3 || ksize == 5) && (stride == 1 || stride == 2) && pad >= 0 && pad < ksize, "%s: k %d stride %d pad %d", fn,
               ksize, stride, pad);
  YOLO_REQUIRE(act >= YOLO_ACT_NONE && act <= YOLO_ACT_SWISH, "%s: activation %d", fn, act);
  // the last output's window must start inside the padded image and need at most k - 1 - pad rows of trailing zeros
  YOLO_REQUIRE(ho >= 1 && wo >= 1 && (ho - 1) * stride - pad < h && (wo - 1) * stride - pad < w_ &&
                   (ho - 1) * stride - pad + ksize <= h + ksize - 1 && (wo - 1) * stride - pad + ksize <= w_ + ksize - 1,
               "%s: output size %dx%d inconsistent with input %dx%d k%d s%d pad %d", fn, ho, wo, h, w_, ksize, stride, pad);
  YOLO_REQUIRE(yolo_view_ok(c, in_c_total, in_c_offset, V) && yolo_view_ok(c, out_c_total, out_c_offset, V),
               "%s: views must be %d-channel aligned and inside their buffers", fn, V);
  const long total = (long)n * ho * wo * (c / V);
  YOLO_REQUIRE(total <= kMaxThreads, "%s: grid too large", fn);
  hipLaunchKernelGGL(dwconv_kernel<T>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const T*)x, w, bias, (T*)y, h, w_, c,
                     in_c_total, in_c_offset, ho, wo, out_c_total, out_c_offset, ksize, stride, pad, act, total);
  return yolo_check_launch(fn);
}

// workspace of both precisions: means, scales, then up to kSeMaxSplits partial rows per image
extern "C" size_t yolo_se_workspace_bytes(int n, int c) { return (size_t)n * c * (2 + kSeMaxSplits) * sizeof(float); }

template <typename T>
static int se_fwd(const char* fn, const void* x, void* y, int n, int h, int w_, int c, int in_c_total, int in_c_offset, int out_c_total,
                  int out_c_offset, const float* w1, const float* b1, const float* w2, const float* b2, int squeeze, void* workspace,
                  size_t ws_bytes, yolo_stream_t s) {
  constexpr int V = Lanes<T>::V;
  constexpr bool kDivide = std::is_same<T, float>::value;
  YOLO_REQUIRE(x && y && w1 && b1 && w2 && b2 && workspace && n > 0 && h > 0 && w_ > 0 && c > 0 && c % V == 0, "%s: bad arguments", fn);
  YOLO_REQUIRE(squeeze >= 1 && squeeze <= 64, "%s: %d squeezed channels (1..64)", fn, squeeze);
  YOLO_REQUIRE(ws_bytes >= yolo_se_workspace_bytes(n, c), "%s: workspace too small", fn);
  YOLO_REQUIRE(yolo_view_ok(c, in_c_total, in_c_offset, V) && yolo_view_ok(c, out_c_total, out_c_offset, V),
               "%s: views must be %d-channel aligned and inside their buffers", fn, V);
  float* const mean = (float*)workspace;
  float* const scale = mean + (size_t)n * c;
  float* const partial = scale + (size_t)n * c;
  const int hw = h * w_, cg = c / V;
  const int cgb = cg < 32 ? (cg >= 16 ? 16 : cg >= 8 ? 8 : cg >= 4 ? 4 : cg >= 2 ? 2 : 1) : 32;    // power of two <= 32: 256 % cgb == 0
  const int groups = (cg + cgb - 1) / cgb;
  // enough workgroups for the chip: the 208x208 x 32-channel map of the first block is ONE channel group per image; a range
  // keeps >= 256 pixels
  int splits = 1;
  while (splits < kSeMaxSplits && (long)n * groups * splits < 512 && hw / (splits * 2) >= 256) splits *= 2;
  const long total = (long)n * hw * cg;
  YOLO_REQUIRE((long)n * groups * splits <= 0x7fffffffL && total <= kMaxThreads, "%s: grid too large", fn);
  hipLaunchKernelGGL(se_partial_kernel<T>, dim3((unsigned)(n * groups * splits)), dim3(256), 0, (hipStream_t)s, (const T*)x, partial, hw,
                     c, in_c_total, in_c_offset, cgb, splits);
  int rc = yolo_check_launch(fn, "(pool)");
  if (rc) return rc;
  hipLaunchKernelGGL(se_fc_kernel<kDivide>, dim3((unsigned)n), dim3(1024), 0, (hipStream_t)s, partial, mean, w1, b1, w2, b2, scale, c,
                     squeeze, splits, kDivide ? (float)hw : 1.f / (float)hw);
  rc = yolo_check_launch(fn, "(fc)");
  if (rc) return rc;
  hipLaunchKernelGGL(se_scale_kernel<T>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const T*)x, scale, (T*)y, hw, c,
                     in_c_total, in_c_offset, out_c_total, out_c_offset, total);
  return yolo_check_launch(fn, "(scale)");
}

extern "C" int yolo_dwconv_fwd(const void* x, const float* w, const float* bias, void* y, int n, int h, int w_, int c, int in_c_total,
                               int in_c_offset, int ho, int wo, int out_c_total, int out_c_offset, int ksize, int stride, int pad,
                               int act, yolo_stream_t s) {
  return dwconv_fwd<bf16_t>("yolo_dwconv_fwd", x, w, bias, y, n, h, w_, c, in_c_total, in_c_offset, ho, wo, out_c_total, out_c_offset, ksize, stride, pad, act, s);
}
extern "C" int yolo_dwconv_f32_fwd(const float* x, const float* w, const float* bias, float* y, int n, int h, int w_, int c,
                                   int in_c_total, int in_c_offset, int ho, int wo, int out_c_total, int out_c_offset, int ksize,
                                   int stride, int pad, int act, yolo_stream_t s) {
  return dwconv_fwd<float>("yolo_dwconv_f32_fwd", x, w, bias, y, n, h, w_, c, in_c_total, in_c_offset, ho, wo, out_c_total, out_c_offset, ksize, stride, pad, act, s);
}

extern "C" int yolo_se_fwd(const void* x, void* y, int n, int h, int w_, int c, int in_c_total, int in_c_offset, int out_c_total,
                           int out_c_offset, const float* w1, const float* b1, const float* w2, const float* b2, int squeeze,
                           void* workspace, size_t ws_bytes, yolo_stream_t s) {
  return se_fwd<bf16_t>("yolo_se_fwd", x, y, n, h, w_, c, in_c_total, in_c_offset, out_c_total, out_c_offset, w1, b1, w2, b2, squeeze, workspace, ws_bytes, s);
}
extern "C" int yolo_se_f32_fwd(const float* x, float* y, int n, int h, int w_, int c, int in_c_total, int in_c_offset,
                               int out_c_total, int out_c_offset, const float* w1, const float* b1, const float* w2, const float* b2,
                               int squeeze, void* workspace, size_t ws_bytes, yolo_stream_t s) {
  return se_fwd<float>("yolo_se_f32_fwd", x, y, n, h, w_, c, in_c_total, in_c_offset, out_c_total, out_c_offset, w1, b1, w2, b2, squeeze, workspace, ws_bytes, s);
}
