// The layers of a training step of YOLOv3-tiny/SqueezeNet that are no conv, bf16 mode: SqueezeNet 1.1's
// MaxPool2d(3, 2, ceil_mode=True) with its backward, and the two element passes of a Fire module's backward.  Dense NHWC maps, every
// channel count % 8 == 0, a thread owns one chunk of 8 channels (16 bytes of bf16) of one pixel:
//   maxpool3s2_fwd_kernel   y [n, ho, wo, c], ho = ceil((h - 3) / 2) + 1 = h / 2 for h >= 2: tap 3i + j of the window at (oy, ox) is the pixel
//                           (2oy + i, 2ox + j); pad 0, so tap 0 is always inside the map and the taps beyond it are -inf (ceil mode's partial
//                           last window of an even map)
//   maxpool3s2_bwd_kernel   dx[p] = bf16_rne(acc): acc = 0, then for the windows oy in [ceil((py - 2) / 2), py / 2] and [0, ho), ox likewise (at
//                           most four) in row-major (oy, ox) order: acc = acc + f32(dy[q]) where idx[q] == 3 (py - 2oy) + (px - 2ox)
//   fire_split_kernel       g1[p][c] = bf16_rne(f32(dy[p][c]) * (y_cat[p][c] > 0)) for c < e1, g3 the same for the other e3 channels: the dense
//                           operands of the two expand convs' gradients from the concat map, one pass
//   fire_join_kernel        g_s = bf16_rne((f32(d1) + f32(d3)) * (s_act > 0)): the sum of the two expand data gradients through the squeeze's ReLU
// idx (uint8, y's shape) is the tap number 3i + j of the window's FIRST maximum among its in-bounds taps in row-major order: a later tap
// replaces the running maximum only when strictly greater (torch's rule, yolo_maxpool_train_fwd's rule).  A NaN is never greater.
// No atomics, no workspace, no LDS, every output element written once, sums in a fixed order: two runs give the same bits.
// Built with -ffp-contract=off.
#include "common.h"

namespace {

struct Pool3Args {
  long total;            // threads: output pixels (forward) or input pixels (backward) x chunks
  int h, w, ho, wo, c, chunks;
};

__global__ __launch_bounds__(256) void maxpool3s2_fwd_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, uint8_t* __restrict__ idx,
                                                             const Pool3Args a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  const int ch = (int)(i % a.chunks);
  const long pix = i / a.chunks;                                             // (n, oy, ox) of the output map
  const int ox = (int)(pix % a.wo);
  const long t = pix / a.wo;
  const int oy = (int)(t % a.ho);
  const long n = t / a.ho;
  const bf16_t* xn = x + n * a.h * a.w * a.c + (long)ch * 8;
  bf16x8 best = {};
  int arg[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) arg[j] = -1;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int iy = 2 * oy + k / 3, ix = 2 * ox + k % 3;
    if (iy >= a.h || ix >= a.w) continue;                                    // (2oy < h and 2ox < w: tap 0 is inside)
    const bf16x8 tap = *reinterpret_cast<const bf16x8*>(xn + ((long)iy * a.w + ix) * a.c);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (arg[j] < 0 || (float)tap[j] > (float)best[j]) best[j] = tap[j], arg[j] = k;
  }
  u32x2 o = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j >> 2] |= (uint32_t)arg[j] << (8 * (j & 3));
  *reinterpret_cast<bf16x8*>(y + i * 8) = best;
  *reinterpret_cast<u32x2*>(idx + i * 8) = o;
}

__global__ __launch_bounds__(256) void maxpool3s2_bwd_kernel(const bf16_t* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                             bf16_t* __restrict__ dx, const Pool3Args a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  const int ch = (int)(i % a.chunks);
  const long pix = i / a.chunks;                                             // (n, py, px) of the input map
  const int px = (int)(pix % a.w);
  const long t = pix / a.w;
  const int py = (int)(t % a.h);
  const long n = t / a.h;
  const long out0 = n * a.ho * a.wo;
  const int oy0 = py > 0 ? (py - 1) >> 1 : 0, ox0 = px > 0 ? (px - 1) >> 1 : 0;      // ceil((p - 2) / 2), not below 0
  const int oy1 = min(py >> 1, a.ho - 1), ox1 = min(px >> 1, a.wo - 1);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int oy = oy0; oy <= oy1; ++oy)
    for (int ox = ox0; ox <= ox1; ++ox) {
      const long q = ((out0 + (long)oy * a.wo + ox) * a.chunks + ch) * 8;
      const u32x2 v = *reinterpret_cast<const u32x2*>(idx + q);
      const bf16x8 d = *reinterpret_cast<const bf16x8*>(dy + q);
      const uint32_t me = (uint32_t)(3 * (py - 2 * oy) + (px - 2 * ox));
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (((v[j >> 2] >> (8 * (j & 3))) & 0xffu) == me) acc[j] = acc[j] + (float)d[j];
    }
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16_t)acc[j];
  *reinterpret_cast<bf16x8*>(dx + i * 8) = o;
}

// 8 consecutive values of a dense dy as fp32: one 16-byte load of bf16, two of fp32
template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&v)[8]) {
  if constexpr (std::is_same<T, float>::value) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = a[j], v[4 + j] = b[j];
  } else {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)a[j];
  }
}

template <typename TDY>
__global__ __launch_bounds__(256) void fire_split_kernel(const TDY* __restrict__ dy, const bf16_t* __restrict__ y_cat, bf16_t* __restrict__ g1,
                                                         bf16_t* __restrict__ g3, long pixels, int e1, int e3) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int chunks = (e1 + e3) / 8;
  if (i >= pixels * chunks) return;
  const long p = i / chunks;
  const int c0 = (int)(i - p * chunks) * 8;
  float dv[8];
  load8(dy + i * 8, dv);
  const bf16x8 yv = *reinterpret_cast<const bf16x8*>(y_cat + i * 8);
  bf16x8 out;
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = (bf16_t)(dv[j] * ((float)yv[j] > 0.f ? 1.f : 0.f));
  bf16_t* const dst = c0 < e1 ? g1 + p * e1 + c0 : g3 + p * e3 + (c0 - e1);
  *reinterpret_cast<bf16x8*>(dst) = out;
}

__global__ __launch_bounds__(256) void fire_join_kernel(const bf16_t* __restrict__ d1, const bf16_t* __restrict__ d3,
                                                        const bf16_t* __restrict__ s_act, bf16_t* __restrict__ g_s, long chunks) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= chunks) return;
  const bf16x8 a = *reinterpret_cast<const bf16x8*>(d1 + i * 8), b = *reinterpret_cast<const bf16x8*>(d3 + i * 8);
  const bf16x8 sv = *reinterpret_cast<const bf16x8*>(s_act + i * 8);
  bf16x8 out;
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = (bf16_t)(((float)a[j] + (float)b[j]) * ((float)sv[j] > 0.f ? 1.f : 0.f));
  *reinterpret_cast<bf16x8*>(g_s + i * 8) = out;
}

bool al(const void* p, int n) { return (uintptr_t)p % n == 0; }

// the checks of both pool entries; fills the output map of (h, w)
int pool3_check(int n, int h, int w, int c, const char* fn, Pool3Args& a) {
  YOLO_REQUIRE(n > 0 && h > 0 && w > 0, "%s: empty shape (n %d, h %d, w %d)", fn, n, h, w);
  YOLO_REQUIRE(c > 0 && c % 8 == 0, "%s: c %d must be a positive multiple of 8", fn, c);
  YOLO_REQUIRE(h >= 2 && w >= 2, "%s: the 3/2 ceil-mode pool needs h >= 2 and w >= 2 (a %d x %d map)", fn, h, w);
  YOLO_REQUIRE(h <= (1 << 20) && w <= (1 << 20) && (long)n * h * w <= (1L << 40) / c && (long)n * h * w * (c / 8) < kMaxThreads,
               "%s: shape out of range (n %d, h %d, w %d, c %d)", fn, n, h, w, c);
  a.h = h, a.w = w, a.c = c, a.chunks = c / 8;
  a.ho = h / 2, a.wo = w / 2;              // ceil((h - 3) / 2) + 1 for h >= 2
  a.total = 0;
  return 0;
}

int fire_check(long long pixels, int c, const char* what, const char* fn) {
  YOLO_REQUIRE(pixels > 0, "%s: empty shape (pixels %lld)", fn, pixels);
  YOLO_REQUIRE(c > 0 && c % 8 == 0, "%s: %s %d must be a positive multiple of 8", fn, what, c);
  YOLO_REQUIRE(pixels <= (1LL << 40) / c, "%s: shape out of range (pixels %lld, %s %d)", fn, pixels, what, c);
  return 0;
}

}  // namespace

extern "C" int yolo_maxpool3s2_train_fwd(const void* x, void* y, void* idx, int n, int h, int w, int c, yolo_stream_t s) {
  Pool3Args a;
  if (const int rc = pool3_check(n, h, w, c, "maxpool3s2_train_fwd", a)) return rc;
  YOLO_REQUIRE(x && y && idx, "maxpool3s2_train_fwd: null pointer");
  YOLO_REQUIRE(al(x, 16) && al(y, 16) && al(idx, 8), "maxpool3s2_train_fwd: misaligned pointer");
  a.total = (long)n * a.ho * a.wo * a.chunks;
  hipLaunchKernelGGL(maxpool3s2_fwd_kernel, dim3(blocks_for(a.total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)x, (bf16_t*)y, (uint8_t*)idx, a);
  return yolo_check_launch("maxpool3s2_train_fwd");
}

extern "C" int yolo_maxpool3s2_bwd(const void* dy, const void* idx, void* dx, int n, int h, int w, int c, yolo_stream_t s) {
  Pool3Args a;
  if (const int rc = pool3_check(n, h, w, c, "maxpool3s2_bwd", a)) return rc;
  YOLO_REQUIRE(dy && idx && dx, "maxpool3s2_bwd: null pointer");
  YOLO_REQUIRE(al(dy, 16) && al(dx, 16) && al(idx, 8), "maxpool3s2_bwd: misaligned pointer");
  a.total = (long)n * h * w * a.chunks;
  hipLaunchKernelGGL(maxpool3s2_bwd_kernel, dim3(blocks_for(a.total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)dy, (const uint8_t*)idx,
                     (bf16_t*)dx, a);
  return yolo_check_launch("maxpool3s2_bwd");
}

extern "C" int yolo_fire_bwd_split(const void* dy, int dy_dtype, const void* y_cat, void* g1, void* g3, long long pixels, int e1, int e3,
                                   yolo_stream_t s) {
  if (const int rc = fire_check(pixels, e1, "e1", "fire_bwd_split")) return rc;
  if (const int rc = fire_check(pixels, e3, "e3", "fire_bwd_split")) return rc;
  YOLO_REQUIRE(dy_dtype == YOLO_DT_BF16 || dy_dtype == YOLO_DT_F32, "fire_bwd_split: dy_dtype %d (YOLO_DT_BF16 or YOLO_DT_F32)", dy_dtype);
  YOLO_REQUIRE(dy && y_cat && g1 && g3, "fire_bwd_split: null pointer");
  YOLO_REQUIRE(al(dy, 16) && al(y_cat, 16) && al(g1, 16) && al(g3, 16), "fire_bwd_split: misaligned pointer");
  const long total = (long)pixels * ((e1 + e3) / 8);
  YOLO_REQUIRE(total < kMaxThreads, "fire_bwd_split: too many elements");
  if (dy_dtype == YOLO_DT_F32)
    hipLaunchKernelGGL(fire_split_kernel<float>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const float*)dy, (const bf16_t*)y_cat,
                       (bf16_t*)g1, (bf16_t*)g3, (long)pixels, e1, e3);
  else
    hipLaunchKernelGGL(fire_split_kernel<bf16_t>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)dy, (const bf16_t*)y_cat,
                       (bf16_t*)g1, (bf16_t*)g3, (long)pixels, e1, e3);
  return yolo_check_launch("fire_bwd_split");
}

extern "C" int yolo_fire_bwd_join(const void* d1, const void* d3, const void* s_act, void* g_s, long long pixels, int sq, yolo_stream_t s) {
  if (const int rc = fire_check(pixels, sq, "sq", "fire_bwd_join")) return rc;
  YOLO_REQUIRE(d1 && d3 && s_act && g_s, "fire_bwd_join: null pointer");
  YOLO_REQUIRE(al(d1, 16) && al(d3, 16) && al(s_act, 16) && al(g_s, 16), "fire_bwd_join: misaligned pointer");
  const long total = (long)pixels * (sq / 8);
  YOLO_REQUIRE(total < kMaxThreads, "fire_bwd_join: too many elements");
  hipLaunchKernelGGL(fire_join_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)d1, (const bf16_t*)d3,
                     (const bf16_t*)s_act, (bf16_t*)g_s, total);
  return yolo_check_launch("fire_bwd_join");
}
