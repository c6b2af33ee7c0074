// The max-pools of the models as they train, bf16 mode, each with its backward: one forward and one backward
// kernel over the compile-time window (K, STRIDE, PAD, DIL), four instances behind six entries:
//   <2, 2, 0, 1>   yolo_maxpool_*(stride 2)   MaxPool2d(2, 2): y [n, h/2, w/2, c] (floor: an odd last row / column is dropped)
//   <2, 1, 1, 2>   yolo_maxpool_*(stride 1)   MaxPool2d(2, 1, padding=1, dilation=2), what the reference's MaxPool(2, 1) turns into: y [n, h, w, c],
//                                             the four diagonal neighbours
//   <3, 2, 0, 1>   yolo_maxpool3s2_*          MaxPool2d(3, 2, ceil_mode=True) of SqueezeNet 1.1: y [n, h/2, w/2, c] (ceil((h - 3) / 2) + 1 for
//                                             h >= 2; the last window of an even map is partial)
//   <3, 2, 1, 1>   yolo_maxpool3s2p1_*        MaxPool2d(3, 2, 1) of ShuffleNetV2: y [n, (h - 1)/2 + 1, (w - 1)/2 + 1, c]
// Dense NHWC maps, c % 8 == 0, a thread owns one chunk of 8 channels (16 bytes) of one pixel.  Tap K i + j of the window at output pixel
// (oy, ox) is the input pixel (STRIDE oy - PAD + DIL i, STRIDE ox - PAD + DIL j); a tap outside the map is no candidate (-inf, not 0), and
// every window of the four forms has a tap inside.
//   pool_fwd_kernel   y = the window's maximum; idx (uint8, y's shape) = the tap number of its FIRST maximum among the in-bounds taps in
//                     row-major order: a later tap replaces the running maximum only when strictly greater (torch's rule,
//                     yolo_spp_train_fwd's rule).  A NaN is never greater.
//   pool_bwd_kernel   dx[p] = bf16_rne(acc): acc = 0, then for the windows q that cover p, in row-major (oy, ox) order: acc = acc + f32(dy[q])
//                     where idx[q] names p.  Where the windows tile the map (2/2) at most one covers p and nothing is summed: dx[p] takes
//                     dy[q]'s bits (a -0.0 stays -0.0, which 0.f + d would not keep), and +0 where no window names it.
// No atomics, no workspace, no LDS, every output element written once, sums in a fixed order: two runs give the same bits.
// Built with -ffp-contract=off.
#include "common.h"

namespace {

struct PoolArgs {
  long total;            // threads: output pixels (forward) or input pixels (backward) x chunks
  int h, w, ho, wo, c, chunks;
};

// the windows tile the map: every tap is inside it (the output map is the floor one) and a pixel lies in at most one window
template <int K, int STRIDE, int PAD, int DIL>
constexpr bool kTiles = PAD == 0 && (K - 1) * DIL < STRIDE;

template <int K, int STRIDE, int PAD, int DIL>
__global__ __launch_bounds__(256) void pool_fwd_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, uint8_t* __restrict__ idx,
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
  bf16x8 best = {};
  int arg[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) arg[j] = -1;
#pragma unroll
  for (int k = 0; k < K * K; ++k) {
    const int iy = STRIDE * oy - PAD + DIL * (k / K), ix = STRIDE * ox - PAD + DIL * (k % K);
    if (!kTiles<K, STRIDE, PAD, DIL> && ((PAD > 0 && (iy < 0 || ix < 0)) || iy >= a.h || ix >= a.w)) continue;
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

template <int K, int STRIDE, int PAD, int DIL>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const bf16_t* __restrict__ dy, const uint8_t* __restrict__ idx, bf16_t* __restrict__ dx,
                                                       const PoolArgs a) {
  // Per axis, p is tap i of the window o where STRIDE o = p + PAD - DIL i: the taps i = i0, i0 + STRIDE, .. below K with
  // i0 = (p + PAD) % STRIDE (DIL 1; at STRIDE 1 every tap), at most NWIN of them; a descending i is an ascending o.
  static_assert(DIL == 1 || STRIDE == 1, "the taps that reach a pixel are found for a dilation of 1 or a stride of 1");
  constexpr int NWIN = (K - 1) / STRIDE + 1;
  constexpr bool kCopy = kTiles<K, STRIDE, PAD, DIL>;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  const int ch = (int)(i % a.chunks);
  const long pix = i / a.chunks;                                             // (n, py, px) of the input map
  const int px = (int)(pix % a.w);
  const long t = pix / a.w;
  const int py = (int)(t % a.h);
  const long n = t / a.h;
  const long out0 = n * a.ho * a.wo;
  const int i0 = (py + PAD) % STRIDE, j0 = (px + PAD) % STRIDE;
  bf16x8 o = {};
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
  for (int wy = NWIN - 1; wy >= 0; --wy) {
    const int ti = i0 + wy * STRIDE, sy = py + PAD - DIL * ti;               // sy = STRIDE oy
    if (ti >= K || sy < 0 || sy / STRIDE >= a.ho) continue;                  // (a dropped odd row / column of the 2/2 pool keeps 0)
#pragma unroll
    for (int wx = NWIN - 1; wx >= 0; --wx) {
      const int tj = j0 + wx * STRIDE, sx = px + PAD - DIL * tj;
      if (tj >= K || sx < 0 || sx / STRIDE >= a.wo) continue;
      const long q = ((out0 + (long)(sy / STRIDE) * a.wo + sx / STRIDE) * a.chunks + ch) * 8;
      const u32x2 v = *reinterpret_cast<const u32x2*>(idx + q);
      const bf16x8 d = *reinterpret_cast<const bf16x8*>(dy + q);
      const uint32_t me = (uint32_t)(K * ti + tj);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (((v[j >> 2] >> (8 * (j & 3))) & 0xffu) == me) {
          if (kCopy) o[j] = d[j];
          else acc[j] = acc[j] + (float)d[j];
        }
    }
  }
  if (!kCopy) {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16_t)acc[j];
  }
  *reinterpret_cast<bf16x8*>(dx + i * 8) = o;
}

bool al(const void* p, int n) { return (uintptr_t)p % n == 0; }

// The checks of all six entries, in one order, and the launch arguments.  (p0, p1): (x, y) forward, (dy, dx) backward; (ho, wo): the
// entry's output map; ``pixels``: the map a thread owns a pixel of.  A map below 2 x 2 is refused in the instance's own words; the 3/2/1
// pool takes any map (its centre tap is always inside).
template <int K, int STRIDE, int PAD, int DIL>
int pool_args(const char* fn, const void* p0, const void* p1, const void* idx, int n, int h, int w, int c, int ho, int wo, long pixels,
              PoolArgs& a) {
  YOLO_REQUIRE(n > 0 && h > 0 && w > 0, "%s: empty shape (n %d, h %d, w %d)", fn, n, h, w);
  YOLO_REQUIRE(c > 0 && c % 8 == 0, "%s: c %d must be a positive multiple of 8", fn, c);
  if (K == 2 && STRIDE == 2) YOLO_REQUIRE(h >= 2 && w >= 2, "%s: empty output (the 2/2 pool of a %d x %d map)", fn, h, w);
  if (K == 2 && STRIDE == 1)
    YOLO_REQUIRE(h >= 2 && w >= 2, "%s: the stride-1 form needs h >= 2 and w >= 2 (a window of a %d x %d map can be all padding)", fn, h, w);
  if (K == 3 && PAD == 0) YOLO_REQUIRE(h >= 2 && w >= 2, "%s: the 3/2 ceil-mode pool needs h >= 2 and w >= 2 (a %d x %d map)", fn, h, w);
  YOLO_REQUIRE(h <= (1 << 20) && w <= (1 << 20) && (long)n * h * w <= (1L << 40) / c && (long)n * h * w * (c / 8) < kMaxThreads,
               "%s: shape out of range (n %d, h %d, w %d, c %d)", fn, n, h, w, c);
  YOLO_REQUIRE(p0 && p1 && idx, "%s: null pointer", fn);
  YOLO_REQUIRE(al(p0, 16) && al(p1, 16) && al(idx, 8), "%s: misaligned pointer", fn);
  a.h = h, a.w = w, a.ho = ho, a.wo = wo, a.c = c, a.chunks = c / 8;
  a.total = n * pixels * a.chunks;
  return 0;
}

template <int K, int STRIDE, int PAD, int DIL>
int pool_fwd(const char* fn, const void* x, void* y, void* idx, int n, int h, int w, int c, int ho, int wo, yolo_stream_t s) {
  PoolArgs a;
  if (const int rc = pool_args<K, STRIDE, PAD, DIL>(fn, x, y, idx, n, h, w, c, ho, wo, (long)ho * wo, a)) return rc;
  hipLaunchKernelGGL((pool_fwd_kernel<K, STRIDE, PAD, DIL>), dim3(blocks_for(a.total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)x,
                     (bf16_t*)y, (uint8_t*)idx, a);
  return yolo_check_launch(fn);
}

template <int K, int STRIDE, int PAD, int DIL>
int pool_bwd(const char* fn, const void* dy, const void* idx, void* dx, int n, int h, int w, int c, int ho, int wo, yolo_stream_t s) {
  PoolArgs a;
  if (const int rc = pool_args<K, STRIDE, PAD, DIL>(fn, dy, dx, idx, n, h, w, c, ho, wo, (long)h * w, a)) return rc;
  hipLaunchKernelGGL((pool_bwd_kernel<K, STRIDE, PAD, DIL>), dim3(blocks_for(a.total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)dy,
                     (const uint8_t*)idx, (bf16_t*)dx, a);
  return yolo_check_launch(fn);
}

// the reference's MaxPool has two forms behind one entry
int maxpool_stride(const char* fn, int stride) {
  YOLO_REQUIRE(stride == 1 || stride == 2, "%s: stride %d unsupported (2: MaxPool2d(2, 2); 1: MaxPool2d(2, 1, padding=1, dilation=2))", fn, stride);
  return 0;
}

}  // namespace

extern "C" int yolo_maxpool_train_fwd(const void* x, void* y, void* idx, int n, int h, int w, int c, int stride, yolo_stream_t s) {
  const char* fn = "maxpool_train_fwd";
  if (const int rc = maxpool_stride(fn, stride)) return rc;
  return stride == 2 ? pool_fwd<2, 2, 0, 1>(fn, x, y, idx, n, h, w, c, h / 2, w / 2, s) : pool_fwd<2, 1, 1, 2>(fn, x, y, idx, n, h, w, c, h, w, s);
}

extern "C" int yolo_maxpool_bwd(const void* dy, const void* idx, void* dx, int n, int h, int w, int c, int stride, yolo_stream_t s) {
  const char* fn = "maxpool_bwd";
  if (const int rc = maxpool_stride(fn, stride)) return rc;
  return stride == 2 ? pool_bwd<2, 2, 0, 1>(fn, dy, idx, dx, n, h, w, c, h / 2, w / 2, s) : pool_bwd<2, 1, 1, 2>(fn, dy, idx, dx, n, h, w, c, h, w, s);
}

extern "C" int yolo_maxpool3s2_train_fwd(const void* x, void* y, void* idx, int n, int h, int w, int c, yolo_stream_t s) {
  return pool_fwd<3, 2, 0, 1>("maxpool3s2_train_fwd", x, y, idx, n, h, w, c, h / 2, w / 2, s);
}

extern "C" int yolo_maxpool3s2_bwd(const void* dy, const void* idx, void* dx, int n, int h, int w, int c, yolo_stream_t s) {
  return pool_bwd<3, 2, 0, 1>("maxpool3s2_bwd", dy, idx, dx, n, h, w, c, h / 2, w / 2, s);
}

extern "C" int yolo_maxpool3s2p1_train_fwd(const void* x, void* y, void* idx, int n, int h, int w, int c, yolo_stream_t s) {
  return pool_fwd<3, 2, 1, 1>("maxpool3s2p1_train_fwd", x, y, idx, n, h, w, c, (h - 1) / 2 + 1, (w - 1) / 2 + 1, s);
}

extern "C" int yolo_maxpool3s2p1_bwd(const void* dy, const void* idx, void* dx, int n, int h, int w, int c, yolo_stream_t s) {
  return pool_bwd<3, 2, 1, 1>("maxpool3s2p1_bwd", dy, idx, dx, n, h, w, c, (h - 1) / 2 + 1, (w - 1) / 2 + 1, s);
}
