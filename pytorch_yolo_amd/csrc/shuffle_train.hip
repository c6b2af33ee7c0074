// The backward of channel_shuffle(cat(a, b), 2) on the two-slot layout of yolo_channel_shuffle2_fwd in a training step of
// YOLOv3-tiny/ShuffleNetV2, bf16 mode; the model's MaxPool2d(3, 2, 1) is an instance of csrc/pool_train.hip.  NHWC maps,
// every physical channel count % 8 == 0, a thread owns one chunk of 8 channels (16 bytes of bf16) of one pixel:
//   shuffle2_bwd_kernel      da[q] = dy_logical[2q], db[q] = dy_logical[2q + 1] for q < half, 0 for half <= q < c_slot; logical channel j of
//                            dy sits at physical (j / half) c_slot + j % half.  dy, da and db are channel views (c_total, c_offset); dy is
//                            read one channel at a time and its pad channels are never read; the outputs are written as whole chunks
// No atomics, no workspace, no LDS, every output element written once: two runs give the same bits.
// Built with -ffp-contract=off.
#include "common.h"

namespace {

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

}  // namespace

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
