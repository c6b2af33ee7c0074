// The reference's MaxPool (models/yolo_base.py:60-80) as it trains, bf16 mode, with its backward: the two forms YOLOv3-tiny
// and LiteYOLOv3 use.  Dense NHWC maps, c % 8 == 0, a thread owns one chunk of 8 channels (16 bytes) of one pixel:
//   maxpool_fwd_kernel<2>   y [n, h/2, w/2, c] = MaxPool2d(2, 2)(x) (floor: an odd last row / column is dropped), taps (2oy + i, 2ox + j)
//   maxpool_fwd_kernel<1>   y [n, h, w, c] = MaxPool2d(2, 1, padding=1, dilation=2)(x), what MaxPool(2, 1) turns into: taps (y - 1 + 2i,
//                           x - 1 + 2j), the diagonal neighbours, out-of-bounds taps are -inf padding
//   maxpool_bwd_kernel<2>   dx[p] = dy[q] where idx[q] names p inside its own 2x2 block q, otherwise 0 (a copy: nothing is summed)
//   maxpool_bwd_kernel<1>   dx[p] = bf16_rne(acc): acc = 0, then for the window centres q = p + (-1,-1), (-1,+1), (+1,-1), (+1,+1) in that
//                           order (p is their tap 3, 2, 1, 0): acc = acc + f32(dy[q]) where q is in bounds and idx[q] names p
// idx (uint8, y's shape) is the tap number 2i + j of the window's FIRST maximum among its in-bounds taps in row-major order: a later tap
// replaces the running maximum only when strictly greater (torch's rule, yolo_spp_train_fwd's rule).  A NaN is never greater.
// No atomics, no workspace, no LDS, every output element written once, sums in a fixed order: two runs give the same bits.
// Built with -ffp-contract=off.
#include "common.h"

namespace {

struct PoolArgs {
  long total;            // threads: output pixels (forward) or input pixels (backward) x chunks
  int h, w, ho, wo, c, chunks;
};

// tap k = 2i + j of the window at output pixel (oy, ox): its input pixel, and whether that is inside the map
template <int STRIDE>
__device__ __forceinline__ bool tap_pixel(int oy, int ox, int k, int h, int w, int& iy, int& ix) {
  if (STRIDE == 2) {
    iy = 2 * oy + (k >> 1), ix = 2 * ox + (k & 1);
    return true;                                                             // ho = h / 2, wo = w / 2: always inside
  }
  iy = oy - 1 + 2 * (k >> 1), ix = ox - 1 + 2 * (k & 1);
  return iy >= 0 && iy < h && ix >= 0 && ix < w;
}

template <int STRIDE>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, uint8_t* __restrict__ idx,
                                                          const PoolArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  const int ch = (int)(i % a.chunks);
  const long pix = i / a.chunks;                                             // (n, oy, ox) of the output map
  const int ox = (int)(pix % a.wo);
  const long t = pix / a.wo;
  const int oy = (int)(t % a.ho);
  const long n = t / a.ho;
  const bf16_t* xn = x + n * a.h * a.w * a.c + (long)ch * 8;
  bf16x8 tap[4];
  bool ok[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int iy, ix;
    ok[k] = tap_pixel<STRIDE>(oy, ox, k, a.h, a.w, iy, ix);
    if (ok[k]) tap[k] = *reinterpret_cast<const bf16x8*>(xn + ((long)iy * a.w + ix) * a.c);
  }
  bf16x8 best = {};
  int arg[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) arg[j] = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!ok[k]) continue;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (arg[j] < 0 || (float)tap[k][j] > (float)best[j]) best[j] = tap[k][j], arg[j] = k;
  }
  u32x2 o = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j >> 2] |= (uint32_t)arg[j] << (8 * (j & 3));
  *reinterpret_cast<bf16x8*>(y + i * 8) = best;
  *reinterpret_cast<u32x2*>(idx + i * 8) = o;
}

template <int STRIDE>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const bf16_t* __restrict__ dy, const uint8_t* __restrict__ idx, bf16_t* __restrict__ dx,
                                                          const PoolArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  const int ch = (int)(i % a.chunks);
  const long pix = i / a.chunks;                                             // (n, py, px) of the input map
  const int px = (int)(pix % a.w);
  const long t = pix / a.w;
  const int py = (int)(t % a.h);
  const long n = t / a.h;
  const long out0 = n * a.ho * a.wo;
  bf16x8 o = {};
  if (STRIDE == 2) {
    const int qy = py >> 1, qx = px >> 1;
    if (qy < a.ho && qx < a.wo) {                                            // (a dropped odd row / column keeps 0)
      const long q = ((out0 + (long)qy * a.wo + qx) * a.chunks + ch) * 8;
      const u32x2 v = *reinterpret_cast<const u32x2*>(idx + q);
      const bf16x8 d = *reinterpret_cast<const bf16x8*>(dy + q);
      const uint32_t me = (uint32_t)((py & 1) * 2 + (px & 1));
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (((v[j >> 2] >> (8 * (j & 3))) & 0xffu) == me) o[j] = d[j];
    }
  } else {
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int qy = py - 1 + 2 * (k >> 1), qx = px - 1 + 2 * (k & 1);
      if (qy < 0 || qy >= a.ho || qx < 0 || qx >= a.wo) continue;
      const long q = ((out0 + (long)qy * a.wo + qx) * a.chunks + ch) * 8;
      const u32x2 v = *reinterpret_cast<const u32x2*>(idx + q);
      const bf16x8 d = *reinterpret_cast<const bf16x8*>(dy + q);
      const uint32_t me = (uint32_t)(3 - k);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (((v[j >> 2] >> (8 * (j & 3))) & 0xffu) == me) acc[j] = acc[j] + (float)d[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16_t)acc[j];
  }
  *reinterpret_cast<bf16x8*>(dx + i * 8) = o;
}

bool al(const void* p, int n) { return (uintptr_t)p % n == 0; }

// the checks of both entries; fills the output map of (h, w, stride)
int pool_check(int n, int h, int w, int c, int stride, const char* fn, PoolArgs& a) {
  YOLO_REQUIRE(stride == 1 || stride == 2, "%s: stride %d unsupported (2: MaxPool2d(2, 2); 1: MaxPool2d(2, 1, padding=1, dilation=2))", fn, stride);
  YOLO_REQUIRE(n > 0 && h > 0 && w > 0, "%s: empty shape (n %d, h %d, w %d)", fn, n, h, w);
  YOLO_REQUIRE(c > 0 && c % 8 == 0, "%s: c %d must be a positive multiple of 8", fn, c);
  if (stride == 1) YOLO_REQUIRE(h >= 2 && w >= 2, "%s: the stride-1 form needs h >= 2 and w >= 2 (a window of a %d x %d map can be all padding)", fn, h, w);
  else YOLO_REQUIRE(h >= 2 && w >= 2, "%s: empty output (the 2/2 pool of a %d x %d map)", fn, h, w);
  YOLO_REQUIRE(h <= (1 << 20) && w <= (1 << 20) && (long)n * h * w <= (1L << 40) / c && (long)n * h * w * (c / 8) < kMaxThreads,
               "%s: shape out of range (n %d, h %d, w %d, c %d)", fn, n, h, w, c);
  a.h = h, a.w = w, a.c = c, a.chunks = c / 8;
  a.ho = stride == 2 ? h / 2 : h, a.wo = stride == 2 ? w / 2 : w;
  a.total = 0;
  return 0;
}

}  // namespace

extern "C" int yolo_maxpool_train_fwd(const void* x, void* y, void* idx, int n, int h, int w, int c, int stride, yolo_stream_t s) {
  PoolArgs a;
  if (const int rc = pool_check(n, h, w, c, stride, "maxpool_train_fwd", a)) return rc;
  YOLO_REQUIRE(x && y && idx, "maxpool_train_fwd: null pointer");
  YOLO_REQUIRE(al(x, 16) && al(y, 16) && al(idx, 8), "maxpool_train_fwd: misaligned pointer");
  a.total = (long)n * a.ho * a.wo * a.chunks;
  if (stride == 2)
    hipLaunchKernelGGL(maxpool_fwd_kernel<2>, dim3(blocks_for(a.total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)x, (bf16_t*)y, (uint8_t*)idx, a);
  else
    hipLaunchKernelGGL(maxpool_fwd_kernel<1>, dim3(blocks_for(a.total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)x, (bf16_t*)y, (uint8_t*)idx, a);
  return yolo_check_launch("maxpool_train_fwd");
}

extern "C" int yolo_maxpool_bwd(const void* dy, const void* idx, void* dx, int n, int h, int w, int c, int stride, yolo_stream_t s) {
  PoolArgs a;
  if (const int rc = pool_check(n, h, w, c, stride, "maxpool_bwd", a)) return rc;
  YOLO_REQUIRE(dy && idx && dx, "maxpool_bwd: null pointer");
  YOLO_REQUIRE(al(dy, 16) && al(dx, 16) && al(idx, 8), "maxpool_bwd: misaligned pointer");
  a.total = (long)n * h * w * a.chunks;
  if (stride == 2)
    hipLaunchKernelGGL(maxpool_bwd_kernel<2>, dim3(blocks_for(a.total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)dy, (const uint8_t*)idx, (bf16_t*)dx,
                       a);
  else
    hipLaunchKernelGGL(maxpool_bwd_kernel<1>, dim3(blocks_for(a.total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)dy, (const uint8_t*)idx, (bf16_t*)dx,
                       a);
  return yolo_check_launch("maxpool_bwd");
}
