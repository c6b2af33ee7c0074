// The two element passes of a Fire module's backward in a training step of YOLOv3-tiny/SqueezeNet, bf16 mode; the
// module's MaxPool2d(3, 2, ceil_mode=True) is an instance of csrc/pool_train.hip.  Dense NHWC maps, every channel count % 8 == 0, a thread
// owns one chunk of 8 channels (16 bytes of bf16) of one pixel:
//   fire_split_kernel       g1[p][c] = bf16_rne(f32(dy[p][c]) * (y_cat[p][c] > 0)) for c < e1, g3 the same for the other e3 channels: the dense
//                           operands of the two expand convs' gradients from the concat map, one pass
//   fire_join_kernel        g_s = bf16_rne((f32(d1) + f32(d3)) * (s_act > 0)): the sum of the two expand data gradients through the squeeze's ReLU
// No atomics, no workspace, no LDS, every output element written once: two runs give the same bits.
// Built with -ffp-contract=off.
#include "common.h"

namespace {

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

int fire_check(long long pixels, int c, const char* what, const char* fn) {
  YOLO_REQUIRE(pixels > 0, "%s: empty shape (pixels %lld)", fn, pixels);
  YOLO_REQUIRE(c > 0 && c % 8 == 0, "%s: %s %d must be a positive multiple of 8", fn, what, c);
  YOLO_REQUIRE(pixels <= (1LL << 40) / c, "%s: shape out of range (pixels %lld, %s %d)", fn, pixels, what, c);
  return 0;
}

}  // namespace

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
