// The layers between the convs of a training step of YOLOv3 / YOLOv3-SPP (reference models/yolov3_spp.py:75-77,129-137,
// models/yolo_layer.py:6-22), bf16 mode, each with its backward.  Dense NHWC maps, every channel count % 8 == 0, a thread
// owns one chunk of 8 channels (16 bytes) of one pixel:
//   spp_fwd_kernel     y = cat([maxpool5(x), maxpool9(x), maxpool13(x), x]) and the argmax planes idx (uint8 window offsets)
//   spp_bwd_kernel     dx as a gather: every pixel adds the dy of the windows whose argmax it is, then the pass-through slice
//   upcat_fwd_kernel   y = cat([nearest_x2(a), b]), or cat([b, nearest_x2(a)]) (YOLOv3-tiny's order): a channel offset
//   upcat_da_kernel    da = the 2x2 block sums of dy[..., :ca];  upcat_db_kernel  db = dy[..., ca:]
// The two SPP kernels run one workgroup per (image, chunk); maps of up to kSppLdsPixels pixels are staged in LDS first (x in the forward;
// the three pooled slices of dy and the three index planes in the backward), larger maps read global memory with the same code.
// No atomics, no scratch, every output element written once, sums in a fixed order: two runs give the same bits.
// Built with -ffp-contract=off: every fp32 operation is rounded on its own.
#include "common.h"

namespace {

constexpr int kSppLdsPixels = 1600;        // 40 x 40: the backward's 72 bytes a pixel are 112.5 KiB of LDS
constexpr int kSppLevels = 3;              // windows 5, 9, 13: radius 2 (level + 1)
constexpr int kNoIndex = 255;              // "no candidate yet" (window offsets end at 168)

struct u8x8 {
  u32x2 v;
  __device__ __forceinline__ int at(int j) const { return (int)((v[j >> 2] >> (8 * (j & 3))) & 0xffu); }
};

// ---- SPP forward --------------------------------------------------------------------------------------------------------------------------
// The argmax of a window is its first maximum in row-major order (torch's max_pool2d): candidates are visited in row-major order and
// replace the running maximum only when strictly greater.  idx holds (row offset)(2r + 1) + column offset inside the level's own window.
template <bool LDS>
__global__ __launch_bounds__(256) void spp_fwd_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, uint8_t* __restrict__ idx, int h,
                                                      int w, int c) {
  extern __shared__ bf16x8 spp_lds[];
  const int chunks = c / 8, hw = h * w;
  const int n = blockIdx.x / chunks, c0 = (blockIdx.x - n * chunks) * 8;
  const bf16_t* xn = x + (size_t)n * hw * c + c0;
  if (LDS) {
    for (int q = threadIdx.x; q < hw; q += 256) spp_lds[q] = *reinterpret_cast<const bf16x8*>(xn + (size_t)q * c);
    __syncthreads();
  }
  for (int p = threadIdx.x; p < hw; p += 256) {
    const int ph = p / w, pw = p - ph * w;
    float best[kSppLevels][8];
    int arg[kSppLevels][8];
#pragma unroll
    for (int l = 0; l < kSppLevels; ++l)
#pragma unroll
      for (int j = 0; j < 8; ++j) best[l][j] = -__builtin_inff(), arg[l][j] = kNoIndex;
    const int r_max = 2 * kSppLevels;
    const int h0 = ph - r_max > 0 ? ph - r_max : 0, h1 = ph + r_max < h - 1 ? ph + r_max : h - 1;
    const int w0 = pw - r_max > 0 ? pw - r_max : 0, w1 = pw + r_max < w - 1 ? pw + r_max : w - 1;
    bf16x8 centre = {};
    for (int qh = h0; qh <= h1; ++qh) {
      const int dh = qh - ph, adh = dh < 0 ? -dh : dh;
      for (int qw = w0; qw <= w1; ++qw) {
        const int dw = qw - pw, adw = dw < 0 ? -dw : dw;
        const int q = qh * w + qw;
        const bf16x8 v = LDS ? spp_lds[q] : *reinterpret_cast<const bf16x8*>(xn + (size_t)q * c);
        if (q == p) centre = v;
        const int reach = adh > adw ? adh : adw;
#pragma unroll
        for (int l = 0; l < kSppLevels; ++l) {
          const int r = 2 * (l + 1);
          if (reach > r) continue;
          const int off = (dh + r) * (2 * r + 1) + (dw + r);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float f = (float)v[j];
            if (arg[l][j] == kNoIndex || f > best[l][j]) best[l][j] = f, arg[l][j] = off;
          }
        }
      }
    }
    const size_t pix = (size_t)n * hw + p;
    bf16_t* yo = y + pix * 4 * c + c0;
    uint8_t* io = idx + pix * 3 * c + c0;
#pragma unroll
    for (int l = 0; l < kSppLevels; ++l) {
      bf16x8 o;
      u32x2 a = {0u, 0u};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        o[j] = (bf16_t)best[l][j];                                           // exact: the value of one input element
        a[j >> 2] |= (uint32_t)arg[l][j] << (8 * (j & 3));
      }
      *reinterpret_cast<bf16x8*>(yo + (size_t)l * c) = o;
      *reinterpret_cast<u32x2*>(io + (size_t)l * c) = a;
    }
    *reinterpret_cast<bf16x8*>(yo + (size_t)3 * c) = centre;
  }
}

// ---- SPP backward -------------------------------------------------------------------------------------------------------------------------
// dx[p] = bf16_rne(((sum over level 5, then 9, then 13, each over the window centres q in row-major order, of f32(dy_level[q]) where
// idx_level[q] names p) + f32(dy_pass[p])): one fp32 accumulator per channel, terms added one by one in that order.
template <bool LDS>
__global__ __launch_bounds__(256) void spp_bwd_kernel(const bf16_t* __restrict__ dy, const uint8_t* __restrict__ idx, bf16_t* __restrict__ dx,
                                                      int h, int w, int c) {
  extern __shared__ bf16x8 spp_lds[];
  const int chunks = c / 8, hw = h * w;
  const int n = blockIdx.x / chunks, c0 = (blockIdx.x - n * chunks) * 8;
  const bf16_t* dyn = dy + (size_t)n * hw * 4 * c + c0;
  const uint8_t* idn = idx + (size_t)n * hw * 3 * c + c0;
  bf16x8* const sdy = spp_lds;                                               // [level][pixel]
  u32x2* const sid = reinterpret_cast<u32x2*>(spp_lds + (LDS ? kSppLevels * hw : 0));   // [level][pixel]
  if (LDS) {
    for (int i = threadIdx.x; i < kSppLevels * hw; i += 256) {
      const int l = i / hw, q = i - l * hw;
      sdy[i] = *reinterpret_cast<const bf16x8*>(dyn + (size_t)q * 4 * c + (size_t)l * c);
      sid[i] = *reinterpret_cast<const u32x2*>(idn + (size_t)q * 3 * c + (size_t)l * c);
    }
    __syncthreads();
  }
  for (int p = threadIdx.x; p < hw; p += 256) {
    const int ph = p / w, pw = p - ph * w;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int l = 0; l < kSppLevels; ++l) {
      const int r = 2 * (l + 1), k = 2 * r + 1;
      const int h0 = ph - r > 0 ? ph - r : 0, h1 = ph + r < h - 1 ? ph + r : h - 1;
      const int w0 = pw - r > 0 ? pw - r : 0, w1 = pw + r < w - 1 ? pw + r : w - 1;
      for (int qh = h0; qh <= h1; ++qh) {
        for (int qw = w0; qw <= w1; ++qw) {
          const int q = qh * w + qw;
          const int off = (ph - qh + r) * k + (pw - qw + r);                 // p inside the window centred at q
          u8x8 a;
          bf16x8 d;
          if (LDS) {
            a.v = sid[l * hw + q], d = sdy[l * hw + q];
          } else {
            a.v = *reinterpret_cast<const u32x2*>(idn + (size_t)q * 3 * c + (size_t)l * c);
            d = *reinterpret_cast<const bf16x8*>(dyn + (size_t)q * 4 * c + (size_t)l * c);
          }
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (a.at(j) == off) acc[j] = acc[j] + (float)d[j];
        }
      }
    }
    const bf16x8 pass = *reinterpret_cast<const bf16x8*>(dyn + (size_t)p * 4 * c + (size_t)3 * c);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16_t)(acc[j] + (float)pass[j]);
    *reinterpret_cast<bf16x8*>(dx + ((size_t)n * hw + p) * c + c0) = o;
  }
}

// ---- nearest x2 upsample + concat ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void upcat_fwd_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ b, bf16_t* __restrict__ y,
                                                        long total, int h, int w, int ca, int cb, int a_first) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int chunks = (ca + cb) / 8;
  const int ch = (int)(i % chunks);
  const long pix = i / chunks;                                               // (n, oy, ox) of the [n, 2h, 2w] map
  const int ox = (int)(pix % (2 * w));
  const long t = pix / (2 * w);
  const int oy = (int)(t % (2 * h));
  const long n = t / (2 * h);
  const int cha = a_first ? ch : ch - cb / 8, chb = a_first ? ch - ca / 8 : ch;       // the chunk inside a's / b's slice
  bf16x8 v;
  if (cha >= 0 && cha < ca / 8) v = *reinterpret_cast<const bf16x8*>(a + ((n * h + oy / 2) * w + ox / 2) * ca + (long)cha * 8);
  else v = *reinterpret_cast<const bf16x8*>(b + pix * cb + (long)chb * 8);
  *reinterpret_cast<bf16x8*>(y + i * 8) = v;
}

// da = bf16_rne(((f32(dy00) + f32(dy01)) + f32(dy10)) + f32(dy11)): the block's pixels in row-major order
__global__ __launch_bounds__(256) void upcat_da_kernel(const bf16_t* __restrict__ dy, bf16_t* __restrict__ da, long total, int h, int w, int ca,
                                                       int cb, int a_off) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int chunks = ca / 8, ct = ca + cb;
  const int ch = (int)(i % chunks);
  const long pix = i / chunks;                                               // (n, y, x) of the [n, h, w] map
  const int x = (int)(pix % w);
  const long t = pix / w;                                                    // n h + y
  const bf16_t* src = dy + ((2 * t) * (2 * w) + 2 * x) * ct + a_off + (long)ch * 8;
  float acc[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + ((long)(k >> 1) * (2 * w) + (k & 1)) * ct);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = k == 0 ? (float)v[j] : acc[j] + (float)v[j];
  }
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16_t)acc[j];
  *reinterpret_cast<bf16x8*>(da + i * 8) = o;
}

__global__ __launch_bounds__(256) void upcat_db_kernel(const bf16_t* __restrict__ dy, bf16_t* __restrict__ db, long total, int ca, int cb,
                                                       int b_off) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int chunks = cb / 8;
  const int ch = (int)(i % chunks);
  const long pix = i / chunks;
  *reinterpret_cast<bf16x8*>(db + i * 8) = *reinterpret_cast<const bf16x8*>(dy + pix * (ca + cb) + b_off + (long)ch * 8);
}

bool al(const void* p, int n) { return (uintptr_t)p % n == 0; }

int spp_check(int n, int h, int w, int c, const char* fn) {
  YOLO_REQUIRE(n > 0 && h > 0 && w > 0, "%s: empty shape (n %d, h %d, w %d)", fn, n, h, w);
  YOLO_REQUIRE(c > 0 && c % 8 == 0, "%s: c %d must be a positive multiple of 8", fn, c);
  YOLO_REQUIRE((long)h * w <= 0x7fffffffL / 4 && (long)n * (c / 8) <= 0x7fffffffL && (long)n * h * w <= (1L << 40) / (4 * (long)c),
               "%s: shape out of range (n %d, h %d, w %d, c %d)", fn, n, h, w, c);
  return 0;
}

int upcat_check(int n, int h, int w, int ca, int cb, const char* fn) {
  YOLO_REQUIRE(n > 0 && h > 0 && w > 0, "%s: empty shape (n %d, h %d, w %d)", fn, n, h, w);
  YOLO_REQUIRE(ca > 0 && ca % 8 == 0 && cb > 0 && cb % 8 == 0, "%s: ca %d and cb %d must be positive multiples of 8", fn, ca, cb);
  YOLO_REQUIRE(h <= (1 << 20) && w <= (1 << 20) && (long)n * h * w <= (1L << 38) / ((long)ca + cb) &&
                   (long)n * h * w * 4 * ((ca + cb) / 8) < kMaxThreads,
               "%s: shape out of range (n %d, h %d, w %d, ca %d, cb %d)", fn, n, h, w, ca, cb);
  return 0;
}

}  // namespace

extern "C" int yolo_spp_train_fwd(const void* x, void* y, void* idx, int n, int h, int w, int c, yolo_stream_t s) {
  if (const int rc = spp_check(n, h, w, c, "spp_train_fwd")) return rc;
  YOLO_REQUIRE(x && y && idx, "spp_train_fwd: null pointer");
  YOLO_REQUIRE(al(x, 16) && al(y, 16) && al(idx, 8), "spp_train_fwd: misaligned pointer");
  const dim3 grid((unsigned)(n * (c / 8)));
  if (h * w <= kSppLdsPixels)
    hipLaunchKernelGGL(spp_fwd_kernel<true>, grid, dim3(256), (size_t)h * w * 16, (hipStream_t)s, (const bf16_t*)x, (bf16_t*)y, (uint8_t*)idx, h, w,
                       c);
  else
    hipLaunchKernelGGL(spp_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)s, (const bf16_t*)x, (bf16_t*)y, (uint8_t*)idx, h, w, c);
  return yolo_check_launch("spp_train_fwd");
}

extern "C" int yolo_spp_bwd(const void* dy, const void* idx, void* dx, int n, int h, int w, int c, yolo_stream_t s) {
  if (const int rc = spp_check(n, h, w, c, "spp_bwd")) return rc;
  YOLO_REQUIRE(dy && idx && dx, "spp_bwd: null pointer");
  YOLO_REQUIRE(al(dy, 16) && al(dx, 16) && al(idx, 8), "spp_bwd: misaligned pointer");
  const dim3 grid((unsigned)(n * (c / 8)));
  if (h * w <= kSppLdsPixels) {
    static std::atomic<uint64_t> lds_set{0};                 // per device (common.h)
    if (const int rc = yolo_max_dyn_lds(reinterpret_cast<const void*>(&spp_bwd_kernel<true>), kSppLdsPixels * kSppLevels * 24, lds_set, "spp_bwd"))
      return rc;
    hipLaunchKernelGGL(spp_bwd_kernel<true>, grid, dim3(256), (size_t)h * w * kSppLevels * 24, (hipStream_t)s, (const bf16_t*)dy,
                       (const uint8_t*)idx, (bf16_t*)dx, h, w, c);
  } else {
    hipLaunchKernelGGL(spp_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)s, (const bf16_t*)dy, (const uint8_t*)idx, (bf16_t*)dx, h, w, c);
  }
  return yolo_check_launch("spp_bwd");
}

// the two concat orders share the kernels: a_first says whether nearest_x2(a) takes the low channels (yolo_upsample2_concat_*) or the high
// ones (yolo_concat_upsample2_*)
static int upcat_fwd(const void* a, const void* b, void* y, int n, int h, int w, int ca, int cb, int a_first, yolo_stream_t s, const char* fn) {
  if (const int rc = upcat_check(n, h, w, ca, cb, fn)) return rc;
  YOLO_REQUIRE(a && b && y, "%s: null pointer", fn);
  YOLO_REQUIRE(al(a, 16) && al(b, 16) && al(y, 16), "%s: misaligned pointer", fn);
  const long total = (long)n * h * w * 4 * ((ca + cb) / 8);
  hipLaunchKernelGGL(upcat_fwd_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)a, (const bf16_t*)b, (bf16_t*)y, total, h,
                     w, ca, cb, a_first);
  return yolo_check_launch(fn);
}

static int upcat_bwd(const void* dy, void* da, void* db, int n, int h, int w, int ca, int cb, int a_first, yolo_stream_t s, const char* fn) {
  if (const int rc = upcat_check(n, h, w, ca, cb, fn)) return rc;
  YOLO_REQUIRE(dy && (da || db), "%s: null pointer (dy, or both of da and db)", fn);
  YOLO_REQUIRE(al(dy, 16) && al(da, 16) && al(db, 16), "%s: misaligned pointer", fn);
  if (da) {
    const long total = (long)n * h * w * (ca / 8);
    hipLaunchKernelGGL(upcat_da_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)dy, (bf16_t*)da, total, h, w, ca, cb,
                       a_first ? 0 : cb);
    if (const int rc = yolo_check_launch(fn, " (da)")) return rc;
  }
  if (db) {
    const long total = (long)n * h * w * 4 * (cb / 8);
    hipLaunchKernelGGL(upcat_db_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)dy, (bf16_t*)db, total, ca, cb,
                       a_first ? ca : 0);
    if (const int rc = yolo_check_launch(fn, " (db)")) return rc;
  }
  return 0;
}

extern "C" int yolo_upsample2_concat_fwd(const void* a, const void* b, void* y, int n, int h, int w, int ca, int cb, yolo_stream_t s) {
  return upcat_fwd(a, b, y, n, h, w, ca, cb, 1, s, "upsample2_concat_fwd");
}

extern "C" int yolo_upsample2_concat_bwd(const void* dy, void* da, void* db, int n, int h, int w, int ca, int cb, yolo_stream_t s) {
  return upcat_bwd(dy, da, db, n, h, w, ca, cb, 1, s, "upsample2_concat_bwd");
}

// y [n, 2h, 2w, cb + ca] = cat([b, nearest_x2(a)]): the order of YOLOv3-tiny (reference models/yolov3_tiny.py:73)
extern "C" int yolo_concat_upsample2_fwd(const void* b, const void* a, void* y, int n, int h, int w, int cb, int ca, yolo_stream_t s) {
  return upcat_fwd(a, b, y, n, h, w, ca, cb, 0, s, "concat_upsample2_fwd");
}

extern "C" int yolo_concat_upsample2_bwd(const void* dy, void* db, void* da, int n, int h, int w, int cb, int ca, yolo_stream_t s) {
  return upcat_bwd(dy, da, db, n, h, w, ca, cb, 0, s, "concat_upsample2_bwd");
}
