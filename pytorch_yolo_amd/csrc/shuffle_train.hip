// The layers of a training step of YOLOv3-tiny/ShuffleNetV2 that are no conv, bf16 mode: ShuffleNetV2's MaxPool2d(3, 2, 1)
// with its backward, and the backward of channel_shuffle(cat(a, b), 2) on the two-slot layout of yolo_channel_shuffle2_fwd.  NHWC maps, every
// physical channel count % 8 == 0, a thread owns one chunk of 8 channels (16 bytes of bf16) of one pixel:
//   maxpool3s2p1_fwd_kernel  y [n, ho, wo, c], ho = (h - 1) / 2 + 1: tap 3i + j of the window at (oy, ox) is the pixel (2oy - 1 + i, 2ox - 1 + j);
//                            a tap outside the map is no candidate (-inf, not 0); tap 4 (the centre) is always inside
//   maxpool3s2p1_bwd_kernel  dx[p] = bf16_rne(acc): acc = 0, then for the windows oy in [ceil((py - 1) / 2), (py + 1) / 2] and [0, ho), ox
//                            likewise (at most four) in row-major (oy, ox) order: acc = acc + f32(dy[q]) where
//                            idx[q] == 3 (py - 2oy + 1) + (px - 2ox + 1)
//   shuffle2_bwd_kernel      da[q] = dy_logical[2q], db[q] = dy_logical[2q + 1] for q < half, 0 for half <= q < c_slot; logical channel j of
//                            dy sits at physical (j / half) c_slot + j % half.  dy, da and db are channel views (c_total, c_offset); dy is
//                            read one channel at a time and its pad channels are never read; the outputs are written as whole chunks
// idx (uint8, y's shape) is the tap number 3i + j of the window's FIRST maximum among its in-bounds taps in row-major order: a later tap
// replaces the running maximum only when strictly greater (torch's rule, yolo_maxpool3s2_train_fwd's rule).  A NaN is never greater.
// No atomics, no workspace, no LDS, every output element written once, sums in a fixed order: two runs give the same bits.
// Built with -ffp-contract=off.
#include "common.h"

namespace {

struct Pool3p1Args {
  long total;            // threads: output pixels (forward) or input pixels (backward) x chunks
  int h, w, ho, wo, c, chunks;
};

__global__ __launch_bounds__(256) void maxpool3s2p1_fwd_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, uint8_t* __restrict__ idx,
                                                               const Pool3p1Args a) {
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
    const int iy = 2 * oy - 1 + k / 3, ix = 2 * ox - 1 + k % 3;
    if (iy < 0 || ix < 0 || iy >= a.h || ix >= a.w) continue;                // (2oy < h and 2ox < w: tap 4 is inside)
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

__global__ __launch_bounds__(256) void maxpool3s2p1_bwd_kernel(const bf16_t* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                               bf16_t* __restrict__ dx, const Pool3p1Args a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  const int ch = (int)(i % a.chunks);
  const long pix = i / a.chunks;                                             // (n, py, px) of the input map
  const int px = (int)(pix % a.w);
  const long t = pix / a.w;
  const int py = (int)(t % a.h);
  const long n = t / a.h;
  const long out0 = n * a.ho * a.wo;
  const int oy0 = py >> 1, ox0 = px >> 1;                                    // ceil((p - 1) / 2) for p >= 0
  const int oy1 = min((py + 1) >> 1, a.ho - 1), ox1 = min((px + 1) >> 1, a.wo - 1);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int oy = oy0; oy <= oy1; ++oy)
    for (int ox = ox0; ox <= ox1; ++ox) {
      const long q = ((out0 + (long)oy * a.wo + ox) * a.chunks + ch) * 8;
      const u32x2 v = *reinterpret_cast<const u32x2*>(idx + q);
      const bf16x8 d = *reinterpret_cast<const bf16x8*>(dy + q);
      const uint32_t me = (uint32_t)(3 * (py - 2 * oy + 1) + (px - 2 * ox + 1));
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (((v[j >> 2] >> (8 * (j & 3))) & 0xffu) == me) acc[j] = acc[j] + (float)d[j];
    }
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16_t)acc[j];
  *reinterpret_cast<bf16x8*>(dx + i * 8) = o;
}

struct Shuffle2BwdArgs {
  long total;            // threads: pixels x the 2 c_slot / 8 chunks of da and db
  int half, c_slot, chunks;
  int dy_ct, dy_co, da_ct, da_co, db_ct, db_co;
};

__global__ __launch_bounds__(256) void shuffle2_bwd_kernel(const bf16_t* __restrict__ dy, bf16_t* __restrict__ da, bf16_t* __restrict__ db,
                                                           const Shuffle2BwdArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  const int g = (int)(i % (2 * a.chunks));
  const long pix = i / (2 * a.chunks);
  const int odd = g >= a.chunks ? 1 : 0;                                     // 0: a chunk of da, 1: of db
  const int c0 = (g - odd * a.chunks) * 8;
  bf16_t* const out = odd ? db : da;
  if (!out) return;
  const bf16_t* const src = dy + pix * a.dy_ct + a.dy_co;
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int q = c0 + e;
    const int j = 2 * q + odd;                                               // logical channel of dy (only read where q < half: j < 2 half)
    const int slot = j >= a.half ? 1 : 0;
    o[e] = q < a.half ? src[slot * a.c_slot + (j - slot * a.half)] : (bf16_t)0.f;
  }
  *reinterpret_cast<bf16x8*>(out + pix * (odd ? a.db_ct : a.da_ct) + (odd ? a.db_co : a.da_co) + c0) = o;
}

bool al(const void* p, int n) { return (uintptr_t)p % n == 0; }

// the checks of both pool entries; fills the output map of (h, w)
int pool3p1_check(int n, int h, int w, int c, const char* fn, Pool3p1Args& a) {
  YOLO_REQUIRE(n > 0 && h > 0 && w > 0, "%s: empty shape (n %d, h %d, w %d)", fn, n, h, w);
  YOLO_REQUIRE(c > 0 && c % 8 == 0, "%s: c %d must be a positive multiple of 8", fn, c);
  YOLO_REQUIRE(h <= (1 << 20) && w <= (1 << 20) && (long)n * h * w <= (1L << 40) / c && (long)n * h * w * (c / 8) < kMaxThreads,
               "%s: shape out of range (n %d, h %d, w %d, c %d)", fn, n, h, w, c);
  a.h = h, a.w = w, a.c = c, a.chunks = c / 8;
  a.ho = (h - 1) / 2 + 1, a.wo = (w - 1) / 2 + 1;
  a.total = 0;
  return 0;
}

}  // namespace

extern "C" int yolo_maxpool3s2p1_train_fwd(const void* x, void* y, void* idx, int n, int h, int w, int c, yolo_stream_t s) {
  Pool3p1Args a;
  if (const int rc = pool3p1_check(n, h, w, c, "maxpool3s2p1_train_fwd", a)) return rc;
  YOLO_REQUIRE(x && y && idx, "maxpool3s2p1_train_fwd: null pointer");
  YOLO_REQUIRE(al(x, 16) && al(y, 16) && al(idx, 8), "maxpool3s2p1_train_fwd: misaligned pointer");
  a.total = (long)n * a.ho * a.wo * a.chunks;
  hipLaunchKernelGGL(maxpool3s2p1_fwd_kernel, dim3(blocks_for(a.total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)x, (bf16_t*)y,
                     (uint8_t*)idx, a);
  return yolo_check_launch("maxpool3s2p1_train_fwd");
}

extern "C" int yolo_maxpool3s2p1_bwd(const void* dy, const void* idx, void* dx, int n, int h, int w, int c, yolo_stream_t s) {
  Pool3p1Args a;
  if (const int rc = pool3p1_check(n, h, w, c, "maxpool3s2p1_bwd", a)) return rc;
  YOLO_REQUIRE(dy && idx && dx, "maxpool3s2p1_bwd: null pointer");
  YOLO_REQUIRE(al(dy, 16) && al(dx, 16) && al(idx, 8), "maxpool3s2p1_bwd: misaligned pointer");
  a.total = (long)n * h * w * a.chunks;
  hipLaunchKernelGGL(maxpool3s2p1_bwd_kernel, dim3(blocks_for(a.total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)dy, (const uint8_t*)idx,
                     (bf16_t*)dx, a);
  return yolo_check_launch("maxpool3s2p1_bwd");
}

extern "C" int yolo_channel_shuffle2_bwd(const void* dy, void* da, void* db, int n, int h, int w, int half, int c_slot, int dy_c_total,
                                         int dy_c_offset, int da_c_total, int da_c_offset, int db_c_total, int db_c_offset, yolo_stream_t s) {
  const char* fn = "channel_shuffle2_bwd";
  YOLO_REQUIRE(n > 0 && h > 0 && w > 0, "%s: empty shape (n %d, h %d, w %d)", fn, n, h, w);
  YOLO_REQUIRE(c_slot > 0 && c_slot % 8 == 0 && half >= 1 && half <= c_slot, "%s: %d logical channels per slot of %d (a multiple of 8)", fn,
               half, c_slot);
  YOLO_REQUIRE(c_slot <= (1 << 24) && h <= (1 << 20) && w <= (1 << 20), "%s: shape out of range (h %d, w %d, c_slot %d)", fn, h, w, c_slot);
  // dy is read one channel at a time: only the outputs' views have to start and end on chunks
  YOLO_REQUIRE(yolo_view_ok(2 * c_slot, dy_c_total, dy_c_offset, 1), "%s: bad view of dy (%d channels at %d of %d)", fn, 2 * c_slot, dy_c_offset,
               dy_c_total);
  YOLO_REQUIRE(yolo_view_ok(c_slot, da_c_total, da_c_offset, 8) && yolo_view_ok(c_slot, db_c_total, db_c_offset, 8),
               "%s: bad views of da / db (%d channels at %d of %d, at %d of %d; 8-channel aligned)", fn, c_slot, da_c_offset, da_c_total,
               db_c_offset, db_c_total);
  const long pixels = (long)n * h * w;
  const int widest = dy_c_total > da_c_total ? (dy_c_total > db_c_total ? dy_c_total : db_c_total)
                                             : (da_c_total > db_c_total ? da_c_total : db_c_total);
  YOLO_REQUIRE(pixels <= (1L << 40) / widest && pixels * (2 * c_slot / 8) < kMaxThreads, "%s: shape out of range (n %d, h %d, w %d)", fn, n, h, w);
  YOLO_REQUIRE(dy && (da || db), "%s: null pointer (dy, and at least one of da and db)", fn);
  YOLO_REQUIRE(al(dy, 2) && (!da || al(da, 16)) && (!db || al(db, 16)), "%s: misaligned pointer", fn);
  Shuffle2BwdArgs a;
  a.half = half, a.c_slot = c_slot, a.chunks = c_slot / 8;
  a.dy_ct = dy_c_total, a.dy_co = dy_c_offset, a.da_ct = da_c_total, a.da_co = da_c_offset, a.db_ct = db_c_total, a.db_co = db_c_offset;
  a.total = pixels * 2 * a.chunks;
  hipLaunchKernelGGL(shuffle2_bwd_kernel, dim3(blocks_for(a.total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)dy, (bf16_t*)da, (bf16_t*)db, a);
  return yolo_check_launch(fn);
}
