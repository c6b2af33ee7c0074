// Go / no-go for porting the bf16-only kernels (t20 3x3 first) to fp16 operands: does v_mfma_f32_16x16x32_f16 / 32x32x16_f16 run at
// the rate of the _bf16 forms on this chip, under load and on random data (the clock the chip holds depends on the bits it toggles)?
//   hipcc --offload-arch=gfx950 -O3 -o tools/micro/mfma_f16_vs_bf16 tools/micro/mfma_f16_vs_bf16.hip && tools/micro/mfma_f16_vs_bf16
// (or tools/micro/run_mfma_f16_vs_bf16.sh).  A bare MFMA loop: 256 CUs x 8 waves, four independent accumulators per wave, operands
// loaded once from random normal data; the four forms are timed interleaved over five rounds, the median is reported in TFLOP/s.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define HIP_OK(e)                                                                  \
  do {                                                                             \
    hipError_t e_ = (e);                                                           \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));   \
      exit(1);                                                                     \
    }                                                                              \
  } while (0)

__device__ __forceinline__ f32x4 mma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mma(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mma(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mma(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// X8: operand vector, ACC: f32x4 (16x16x32) or f32x16 (32x32x16).  in: [4 operand vectors per lane][64 lanes] random values.
template <typename X8, typename ACC>
__global__ __launch_bounds__(512) void mfma_loop(const X8* __restrict__ in, float* __restrict__ out, int iters) {
  const int lane = threadIdx.x & 63;
  const X8 a0 = in[lane], a1 = in[64 + lane], b0 = in[128 + lane], b1 = in[192 + lane];
  ACC c0 = {}, c1 = {}, c2 = {}, c3 = {};
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      c0 = mma(a0, b0, c0);
      c1 = mma(a1, b0, c1);
      c2 = mma(a0, b1, c2);
      c3 = mma(a1, b1, c3);
    }
  }
  const ACC s = c0 + c1 + c2 + c3;
  if (s[0] == 12345.678f) out[blockIdx.x * blockDim.x + threadIdx.x] = s[1];   // keeps the loop alive; (almost) never true
}

template <typename X8, typename ACC>
static double run_ms(const void* in, float* out, int iters) {
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  HIP_OK(hipEventRecord(e0));
  hipLaunchKernelGGL((mfma_loop<X8, ACC>), dim3(256 * 2), dim3(512), 0, 0, (const X8*)in, out, iters);
  HIP_OK(hipEventRecord(e1));
  HIP_OK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  HIP_OK(hipEventDestroy(e0));
  HIP_OK(hipEventDestroy(e1));
  return ms;
}

int main() {
  std::mt19937 rng(1234);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::vector<uint16_t> hb(256 * 8), hf(256 * 8);
  for (size_t i = 0; i < hb.size(); ++i) {
    const float v = nd(rng);
    const __bf16 b = (__bf16)v;
    const _Float16 f = (_Float16)v;
    __builtin_memcpy(&hb[i], &b, 2);
    __builtin_memcpy(&hf[i], &f, 2);
  }
  void *db, *df;
  float* out;
  HIP_OK(hipMalloc(&db, hb.size() * 2));
  HIP_OK(hipMalloc(&df, hf.size() * 2));
  HIP_OK(hipMalloc((void**)&out, 256 * 2 * 512 * sizeof(float)));
  HIP_OK(hipMemcpy(db, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(df, hf.data(), hf.size() * 2, hipMemcpyHostToDevice));
  const int iters = 20000;                                     // x 32 MFMAs per wave
  const double waves = 256.0 * 2 * 8, mfmas = (double)iters * 32;
  const double flop16 = waves * mfmas * 2.0 * 16 * 16 * 32, flop32 = waves * mfmas * 2.0 * 32 * 32 * 16;   // 16,384 / 32,768 FLOP per instruction
  struct Form {
    const char* name;
    double (*fn)(const void*, float*, int);
    const void* in;
    double flop;
    std::vector<double> ms;
  } forms[] = {{"v_mfma_f32_16x16x32_bf16", run_ms<bf16x8, f32x4>, db, flop16, {}},
               {"v_mfma_f32_16x16x32_f16 ", run_ms<f16x8, f32x4>, df, flop16, {}},
               {"v_mfma_f32_32x32x16_bf16", run_ms<bf16x8, f32x16>, db, flop32, {}},
               {"v_mfma_f32_32x32x16_f16 ", run_ms<f16x8, f32x16>, df, flop32, {}}};
  for (auto& f : forms) f.fn(f.in, out, 2000);                 // warm-up
  for (int r = 0; r < 5; ++r)
    for (auto& f : forms) f.ms.push_back(f.fn(f.in, out, iters));
  printf("bare MFMA loop, 512 workgroups x 8 waves, random normal operands, 5 interleaved rounds (median; min .. max)\n");
  double tf[4];
  int k = 0;
  for (auto& f : forms) {
    std::sort(f.ms.begin(), f.ms.end());
    tf[k++] = f.flop / (f.ms[2] * 1e-3) / 1e12;
    printf("%s  %8.1f TFLOP/s   (%.1f .. %.1f)   %.2f ms\n", f.name, f.flop / (f.ms[2] * 1e-3) / 1e12, f.flop / (f.ms[4] * 1e-3) / 1e12,
           f.flop / (f.ms[0] * 1e-3) / 1e12, f.ms[2]);
  }
  printf("f16 / bf16: 16x16x32 %.3f, 32x32x16 %.3f\n", tf[1] / tf[0], tf[3] / tf[2]);
  return 0;
}
