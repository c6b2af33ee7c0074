// Training-mode batch norm between the conv and its backward (reference ConvBlock, models/yolo_base.py:19-44: Conv2d(bias=False) ->
// BatchNorm2d -> LeakyReLU(0.1)), bf16 mode.  z = bf16(conv(x, bf16(W))) is dense [M][C], M = n h w, C % 8 == 0:
//   stats_kernel + stats_finalize_kernel   S1 = sum z, S2 = sum z z in float64 -> saved = {mean, invstd, scale, shift}, running stats
//   eval_stats_kernel                      the same four vectors from the running statistics
//   act_fwd_kernel                         y = bf16(act(f32(z) scale + shift))
//   act_add_fwd_kernel                     the same with the residual add: y = bf16(act(..) + f32(residual)), y_preadd = bf16(act(..))
//   act_pool_fwd_kernel                    act_fwd_kernel's pass with MaxPool2d(2, 2) inside: the pooled y and its argmax plane (3.6g)
//   bwd_reduce_kernel + bwd_finalize_kernel  B = sum ga, G = sum ga xh in float64 -> dgamma, dbeta, c1, c2
//   act_bwd_kernel                         g = bf16(scale ((ga - c1) - xh c2)), the operand of yolo_conv2d_bwd_weight / _data
// yolo_bn_clamp_fwd / _bwd are act_fwd_kernel, bwd_reduce_kernel and act_bwd_kernel with the activation min(max(a, lo), hi)
// (ReLU6: lo 0, hi 6; ReLU: hi +inf) and the slope (a > lo && a < hi) ? 1 : 0 - BnAct below; everything else is shared.
// yolo_bn_add_rounded_fwd (add_rounded_fwd_kernel) is the linear bottleneck's add: y = bf16(f32(bf16(a)) + f32(residual)).
// Every pass is a stream of 16-byte loads; a thread owns one chunk of 8 channels.  The two reductions split the rows over blockIdx.x
// and write float64 partials [split][2][C] that one thread per channel adds in split order: no atomics, no read-modify-write, every
// output and every used workspace byte written once per call in an order fixed by (M, C, launch_cus).
// Built with -ffp-contract=off: every fp32 and fp64 operation below is rounded on its own (the tests restate them one by one).
#include "common.h"

namespace yolo_conv {
int launch_cus();   // conv_igemm.hip: compute units the coming launches may use
}

namespace {

constexpr int kTileChunks = 256;     // chunk columns of one column tile (2048 channels): blockIdx.y
constexpr int kUnroll = 8;           // rows a thread has in flight (16 or 32 bytes each; fp32 dy: half as many rows)
constexpr int kFinalBatch = 32;      // splits a finalize thread has in flight
constexpr int kMinPasses = 4;        // a split is worth a workgroup from this many passes on
constexpr int kWgPerCu = 1;          // row splits aimed at per compute unit (what was tried)
constexpr int kMaxSplits = 2048;

// The split rule: a pure function of (M, C, compute units).  A workgroup of 256 threads covers `width` chunk columns x `rows` rows per
// pass; the passes of the M rows are dealt to `splits` workgroups, `pps` passes each, the last one ragged.  No split is empty.
struct BnPick {
  int chunks, tiles_y, width, rows;
  long passes, pps;
  int splits;
};

BnPick choose_bn(long m, int c, int n_cu) {
  BnPick k;
  k.chunks = c / 8;
  k.tiles_y = (k.chunks + kTileChunks - 1) / kTileChunks;
  k.width = k.chunks < kTileChunks ? k.chunks : kTileChunks;
  k.rows = 256 / k.width;
  k.passes = (m + k.rows - 1) / k.rows;
  long want = ((long)kWgPerCu * n_cu + k.tiles_y - 1) / k.tiles_y;
  const long by_work = k.passes / kMinPasses > 1 ? k.passes / kMinPasses : 1;
  if (want > by_work) want = by_work;
  if (want > kMaxSplits) want = kMaxSplits;
  k.pps = (k.passes + want - 1) / want;
  k.splits = (int)((k.passes + k.pps - 1) / k.pps);
  return k;
}

// workspace: c1 | c2 (f32 [2][C], written by the backward's finalize), then the float64 partials [split][2][C]
size_t bn_ws_bytes(int c, int splits) { return (size_t)2 * c * sizeof(float) + (size_t)splits * 2 * c * sizeof(double); }

// The activation between the batch norm and the next layer: what the element passes apply and what slope the backward takes.
// kBnLeaky is LeakyReLU(0.1), kBnClamp is min(max(a, lo), hi) with the slope 0 at both bounds (torch's hardtanh_backward rule).
enum { kBnNone = 0, kBnLeaky = 1, kBnClamp = 2 };
struct BnAct {
  int kind;
  float lo, hi;
};

struct ReduceArgs {
  const bf16_t* z;
  const void* dy;          // backward only
  const float* saved;      // backward only
  double* part;            // [splits][2][c]
  long m, rows_per_split;
  int c, chunks, width, rows;
  BnAct act;
};

__device__ __forceinline__ void load8f(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = a[j], v[4 + j] = b[j];
}

template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&v)[8]) {
  if constexpr (std::is_same<T, float>::value) {
    load8f(p, v);
  } else {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)a[j];
  }
}

// 8 channels as they are loaded: what a reduction keeps in flight (4 registers of bf16, 8 of fp32), widened at use
template <typename T>
struct Raw8 {
  bf16x8 v;
  __device__ __forceinline__ void load(const T* p) { v = *reinterpret_cast<const bf16x8*>(p); }
  __device__ __forceinline__ float at(int j) const { return (float)v[j]; }
};
template <>
struct Raw8<float> {
  f32x4 a, b;
  __device__ __forceinline__ void load(const float* p) { a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4); }
  __device__ __forceinline__ float at(int j) const { return j < 4 ? a[j] : b[j - 4]; }
};

// the saved vectors of one chunk's 8 channels
struct BnVecs {
  float mean[8], invstd[8], scale[8], shift[8];
};

__device__ __forceinline__ float bn_slope(float a, const BnAct& t) {
  if (t.kind == kBnClamp) return (a > t.lo && a < t.hi) ? 1.f : 0.f;
  return (t.kind == kBnLeaky && !(a > 0.f)) ? 0.1f : 1.f;
}

__device__ __forceinline__ float bn_value(float a, const BnAct& t) {
  if (t.kind == kBnClamp) return fminf(fmaxf(a, t.lo), t.hi);
  return (t.kind != kBnLeaky || a > 0.f) ? a : 0.1f * a;
}

// adds the threads of a chunk column in row-slot order and writes the workgroup's partial
__device__ __forceinline__ void column_sums(double* lds, const double (&s1)[8], const double (&s2)[8], const ReduceArgs& a, int slot, int chunk0) {
  // lds[k][thread]: k = 0..7 the first sum of the chunk's channels, 8..15 the second; both the stores and the loads below are
  // conflict-free (consecutive threads, consecutive doubles)
  if (slot < a.rows) {
#pragma unroll
    for (int j = 0; j < 8; ++j) lds[j * 256 + threadIdx.x] = s1[j], lds[(8 + j) * 256 + threadIdx.x] = s2[j];
  }
  __syncthreads();
  double* out = a.part + (size_t)blockIdx.x * 2 * a.c;
  for (int o = threadIdx.x; o < a.width * 16; o += 256) {
    const int k = o / a.width, cc = o - k * a.width;
    if (chunk0 + cc >= a.chunks) continue;                    // the ragged last column tile
    double s = 0.0;
    for (int r = 0; r < a.rows; ++r) s += lds[k * 256 + r * a.width + cc];
    out[(size_t)(k >> 3) * a.c + (size_t)(chunk0 + cc) * 8 + (k & 7)] = s;
  }
}

__global__ __launch_bounds__(256) void stats_kernel(const ReduceArgs a) {
  __shared__ double lds[256 * 16];
  const int col = threadIdx.x % a.width, slot = threadIdx.x / a.width;
  const int chunk0 = blockIdx.y * kTileChunks;
  const bool active = slot < a.rows && chunk0 + col < a.chunks;
  const long r0 = (long)blockIdx.x * a.rows_per_split;
  const long r1 = r0 + a.rows_per_split < a.m ? r0 + a.rows_per_split : a.m;
  double s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = 0.0, s2[j] = 0.0;
  if (active) {
    const bf16_t* base = a.z + (size_t)(chunk0 + col) * 8;
    for (long row = r0 + slot; row < r1; row += (long)kUnroll * a.rows) {
      Raw8<bf16_t> v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const long r = row + (long)u * a.rows;
        if (r < r1) v[u].load(base + (size_t)r * a.c);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (row + (long)u * a.rows < r1) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float f = v[u].at(j);
            s1[j] += (double)f;
            s2[j] += (double)(f * f);          // exact in fp32: a bf16 value has 8 significant bits
          }
        }
      }
    }
  }
  column_sums(lds, s1, s2, a, slot, chunk0);
}

template <typename TDY>
__global__ __launch_bounds__(256) void bwd_reduce_kernel(const ReduceArgs a) {
  __shared__ double lds[256 * 16];
  const int col = threadIdx.x % a.width, slot = threadIdx.x / a.width;
  const int chunk0 = blockIdx.y * kTileChunks;
  const bool active = slot < a.rows && chunk0 + col < a.chunks;
  const long r0 = (long)blockIdx.x * a.rows_per_split;
  const long r1 = r0 + a.rows_per_split < a.m ? r0 + a.rows_per_split : a.m;
  double s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = 0.0, s2[j] = 0.0;
  if (active) {
    const size_t c0 = (size_t)(chunk0 + col) * 8;
    BnVecs p;
    load8f(a.saved + c0, p.mean), load8f(a.saved + a.c + c0, p.invstd);
    load8f(a.saved + 2 * (size_t)a.c + c0, p.scale), load8f(a.saved + 3 * (size_t)a.c + c0, p.shift);
    const TDY* dy = (const TDY*)a.dy;
    constexpr int U = std::is_same<TDY, float>::value ? kUnroll / 2 : kUnroll;
    for (long row = r0 + slot; row < r1; row += (long)U * a.rows) {
      Raw8<bf16_t> zr[U];
      Raw8<TDY> dr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long r = row + (long)u * a.rows;
        if (r < r1) zr[u].load(a.z + (size_t)r * a.c + c0), dr[u].load(dy + (size_t)r * a.c + c0);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (row + (long)u * a.rows < r1) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float zf = zr[u].at(j);
            const float act_in = zf * p.scale[j] + p.shift[j];
            const float ga = dr[u].at(j) * bn_slope(act_in, a.act);
            const float xh = (zf - p.mean[j]) * p.invstd[j];
            s1[j] += (double)ga;
            s2[j] += (double)(ga * xh);
          }
        }
      }
    }
  }
  column_sums(lds, s1, s2, a, slot, chunk0);
}

// a channel's two sums over the splits, in split order; kFinalBatch splits' loads are issued before the first add
__device__ __forceinline__ void sum_splits(const double* __restrict__ part, int splits, int c, int ch, double& s1, double& s2) {
  s1 = 0.0, s2 = 0.0;
  const double* p = part + ch;
  const size_t stride = (size_t)2 * c;
  int s = 0;
  for (; s + kFinalBatch <= splits; s += kFinalBatch, p += kFinalBatch * stride) {
    double a[kFinalBatch], b[kFinalBatch];
#pragma unroll
    for (int i = 0; i < kFinalBatch; ++i) a[i] = p[i * stride], b[i] = p[i * stride + c];
#pragma unroll
    for (int i = 0; i < kFinalBatch; ++i) s1 += a[i], s2 += b[i];
  }
  for (; s + 4 <= splits; s += 4, p += 4 * stride) {
    double a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = p[i * stride], b[i] = p[i * stride + c];
#pragma unroll
    for (int i = 0; i < 4; ++i) s1 += a[i], s2 += b[i];
  }
  for (; s < splits; ++s, p += stride) s1 += p[0], s2 += p[c];
}

// one thread per channel: the splits in split order, then the channel's four saved values and its running statistics
__global__ __launch_bounds__(256) void stats_finalize_kernel(const double* __restrict__ part, int splits, int c, long m, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, float momentum, float* __restrict__ rm,
                                                             float* __restrict__ rv, float* __restrict__ saved) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  double s1, s2;
  sum_splits(part, splits, c, ch, s1, s2);
  const double md = (double)m;
  const double mean64 = s1 / md;
  double var64 = s2 / md - mean64 * mean64;
  var64 = var64 > 0.0 ? var64 : 0.0;
  const float mean = (float)mean64;
  const float invstd = (float)(1.0 / sqrt(var64 + (double)eps));
  const float scale = gamma[ch] * invstd;
  saved[ch] = mean;
  saved[c + ch] = invstd;
  saved[2 * (size_t)c + ch] = scale;
  saved[3 * (size_t)c + ch] = beta[ch] - mean * scale;
  if (rm) rm[ch] = rm[ch] * (1.f - momentum) + momentum * mean;
  if (rv) rv[ch] = rv[ch] * (1.f - momentum) + momentum * (float)(var64 * md / (md - 1.0));      // torch's unbiased form
}

__global__ __launch_bounds__(256) void eval_stats_kernel(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ rm,
                                                         const float* __restrict__ rv, int c, float eps, float* __restrict__ saved) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  const float mean = rm[ch];
  const float invstd = (float)(1.0 / sqrt((double)rv[ch] + (double)eps));
  const float scale = gamma[ch] * invstd;
  saved[ch] = mean;
  saved[c + ch] = invstd;
  saved[2 * (size_t)c + ch] = scale;
  saved[3 * (size_t)c + ch] = beta[ch] - mean * scale;
}

__global__ __launch_bounds__(256) void bwd_finalize_kernel(const double* __restrict__ part, int splits, int c, long m, int batch_stats,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ c12) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  double b, g;
  sum_splits(part, splits, c, ch, b, g);
  if (dbeta) dbeta[ch] = (float)b;
  if (dgamma) dgamma[ch] = (float)g;
  c12[ch] = batch_stats ? (float)(b / (double)m) : 0.f;
  c12[c + ch] = batch_stats ? (float)(g / (double)m) : 0.f;
}

// ---- the two element streams: one thread per chunk of 8 channels of one row ---------------------------------------------------------
__global__ __launch_bounds__(256) void act_fwd_kernel(const bf16_t* __restrict__ z, const float* __restrict__ saved, bf16_t* __restrict__ y,
                                                      long total, int c, int chunks, const BnAct act) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c0 = (int)(idx % chunks) * 8;
  float zv[8], scale[8], shift[8];
  load8(z + idx * 8, zv);
  load8f(saved + 2 * (size_t)c + c0, scale), load8f(saved + 3 * (size_t)c + c0, shift);
  bf16x8 out;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float a = zv[j] * scale[j] + shift[j];
    out[j] = (bf16_t)bn_value(a, act);
  }
  *reinterpret_cast<bf16x8*>(y + idx * 8) = out;
}

// the same pass with the residual unit's add: t = act(a); y_preadd = bf16(t) (where wanted); y = bf16(t + f32(residual))
template <bool PREADD>
__global__ __launch_bounds__(256) void act_add_fwd_kernel(const bf16_t* __restrict__ z, const float* __restrict__ saved,
                                                          const bf16_t* __restrict__ res, bf16_t* __restrict__ y, bf16_t* __restrict__ y_preadd,
                                                          long total, int c, int chunks, int leaky) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c0 = (int)(idx % chunks) * 8;
  float zv[8], rv[8], scale[8], shift[8];
  load8(z + idx * 8, zv), load8(res + idx * 8, rv);
  load8f(saved + 2 * (size_t)c + c0, scale), load8f(saved + 3 * (size_t)c + c0, shift);
  bf16x8 out, pre;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float a = zv[j] * scale[j] + shift[j];
    const float t = (!leaky || a > 0.f) ? a : 0.1f * a;
    pre[j] = (bf16_t)t;
    out[j] = (bf16_t)(t + rv[j]);
  }
  *reinterpret_cast<bf16x8*>(y + idx * 8) = out;
  if (PREADD) *reinterpret_cast<bf16x8*>(y_preadd + idx * 8) = pre;
}

// The linear bottleneck's add: act none, and the normalised value is rounded to bf16 BEFORE the add, y = bf16(f32(bf16(a)) +
// f32(residual)) - bit-equal to act_fwd_kernel (act none) followed by a bf16 add (an fp32 add rounded once), in one pass.
__global__ __launch_bounds__(256) void add_rounded_fwd_kernel(const bf16_t* __restrict__ z, const float* __restrict__ saved,
                                                              const bf16_t* __restrict__ res, bf16_t* __restrict__ y, long total, int c, int chunks) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c0 = (int)(idx % chunks) * 8;
  float zv[8], rv[8], scale[8], shift[8];
  load8(z + idx * 8, zv), load8(res + idx * 8, rv);
  load8f(saved + 2 * (size_t)c + c0, scale), load8f(saved + 3 * (size_t)c + c0, shift);
  bf16x8 out;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bf16_t t = (bf16_t)(zv[j] * scale[j] + shift[j]);
    out[j] = (bf16_t)((float)t + rv[j]);
  }
  *reinterpret_cast<bf16x8*>(y + idx * 8) = out;
}

// act_fwd_kernel's pass with MaxPool2d(2, 2) inside it (the ConvPoolBlock as it trains): one thread per chunk of one POOLED
// pixel.  Each of the block's four taps is rounded to bf16 exactly as act_fwd_kernel would write it, then the four bf16 values are compared
// under the first-maximum rule of yolo_maxpool_train_fwd (gamma may be negative: the activated values are compared, not z).  Only the
// pooled y and idx are written; an odd last row / column of z is never read.
__global__ __launch_bounds__(256) void act_pool_fwd_kernel(const bf16_t* __restrict__ z, const float* __restrict__ saved, bf16_t* __restrict__ y,
                                                           uint8_t* __restrict__ idx, long total, int h, int w, int ho, int wo, int c, int chunks,
                                                           int leaky) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ch = (int)(i % chunks);
  const long pix = i / chunks;                                               // (n, oy, ox) of the pooled map
  const int ox = (int)(pix % wo);
  const long t = pix / wo;
  const int oy = (int)(t % ho);
  const long n = t / ho;
  const bf16_t* src = z + ((n * h + 2 * oy) * w + 2 * ox) * c + (long)ch * 8;
  bf16x8 tap[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) tap[k] = *reinterpret_cast<const bf16x8*>(src + ((long)(k >> 1) * w + (k & 1)) * c);
  float scale[8], shift[8];
  load8f(saved + 2 * (size_t)c + (size_t)ch * 8, scale), load8f(saved + 3 * (size_t)c + (size_t)ch * 8, shift);
  bf16x8 best;
  u32x2 arg = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    bf16_t b = (bf16_t)0.f;
    uint32_t at = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float a = (float)tap[k][j] * scale[j] + shift[j];
      const bf16_t v = (bf16_t)((!leaky || a > 0.f) ? a : 0.1f * a);
      if (k == 0 || (float)v > (float)b) b = v, at = (uint32_t)k;
    }
    best[j] = b;
    arg[j >> 2] |= at << (8 * (j & 3));
  }
  *reinterpret_cast<bf16x8*>(y + i * 8) = best;
  *reinterpret_cast<u32x2*>(idx + i * 8) = arg;
}

template <typename TDY>
__global__ __launch_bounds__(256) void act_bwd_kernel(const TDY* __restrict__ dy, const bf16_t* __restrict__ z, const float* __restrict__ saved,
                                                      const float* __restrict__ c12, bf16_t* __restrict__ g, long total, int c, int chunks,
                                                      const BnAct act) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const size_t c0 = (size_t)(idx % chunks) * 8;
  float zv[8], dv[8], c1[8], c2[8];
  BnVecs p;
  load8(z + idx * 8, zv), load8(dy + idx * 8, dv);
  load8f(saved + c0, p.mean), load8f(saved + c + c0, p.invstd);
  load8f(saved + 2 * (size_t)c + c0, p.scale), load8f(saved + 3 * (size_t)c + c0, p.shift);
  load8f(c12 + c0, c1), load8f(c12 + c + c0, c2);
  bf16x8 out;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float a = zv[j] * p.scale[j] + p.shift[j];
    const float ga = dv[j] * bn_slope(a, act);
    const float xh = (zv[j] - p.mean[j]) * p.invstd[j];
    out[j] = (bf16_t)(p.scale[j] * ((ga - c1[j]) - xh * c2[j]));
  }
  *reinterpret_cast<bf16x8*>(g + idx * 8) = out;
}

// what every entry asks of (pixels, c)
int bn_check(long long pixels, int c, const char* fn) {
  YOLO_REQUIRE(c > 0 && c % 8 == 0, "%s: c %d must be a positive multiple of 8", fn, c);
  YOLO_REQUIRE(pixels > 0, "%s: pixels %lld", fn, pixels);
  YOLO_REQUIRE(pixels <= (1LL << 40) / c && pixels * (c / 8) < kMaxThreads, "%s: shape out of range (pixels %lld, c %d)", fn, pixels, c);
  return 0;
}

int act_check(int act, const char* fn) {
  YOLO_REQUIRE(act == YOLO_ACT_NONE || act == YOLO_ACT_LEAKY01, "%s: act %d unsupported (none or LeakyReLU(0.1))", fn, act);
  return 0;
}

BnAct act_of(int act) { return BnAct{act == YOLO_ACT_LEAKY01 ? kBnLeaky : kBnNone, 0.f, 0.f}; }

// the bounds of the clamp entries: lo finite, hi finite or +inf, lo < hi (a NaN fails every comparison)
int clamp_check(float lo, float hi, const char* fn) {
  YOLO_REQUIRE(lo - lo == 0.f && hi == hi && lo < hi, "%s: clamp bounds lo %g, hi %g (lo finite, hi finite or +inf, lo < hi)", fn, (double)lo,
               (double)hi);
  return 0;
}

bool al(const void* p, int n) { return (uintptr_t)p % n == 0; }

ReduceArgs reduce_args(const BnPick& k, long m, int c) {
  ReduceArgs a;
  a.z = nullptr, a.dy = nullptr, a.saved = nullptr, a.part = nullptr;
  a.m = m, a.rows_per_split = k.pps * k.rows;
  a.c = c, a.chunks = k.chunks, a.width = k.width, a.rows = k.rows, a.act = BnAct{kBnNone, 0.f, 0.f};
  return a;
}

}  // namespace

extern "C" size_t yolo_bn_workspace_bytes(long long pixels, int c) {
  if (bn_check(pixels, c, "bn_workspace_bytes")) return 0;
  return bn_ws_bytes(c, choose_bn(pixels, c, yolo_conv::launch_cus()).splits);
}

extern "C" int yolo_bn_pick(long long pixels, int c, char* out, int out_len) {
  YOLO_REQUIRE(out && out_len > 0, "bn_pick: bad arguments");
  out[0] = 0;
  if (const int rc = bn_check(pixels, c, "bn_pick")) return rc;
  const BnPick k = choose_bn(pixels, c, yolo_conv::launch_cus());
  snprintf(out, (size_t)out_len, "bn_reduce<%dx%d> grid %dx%d passes %ld last %ld", k.rows, k.width, k.splits, k.tiles_y, k.pps,
           k.passes - (long)(k.splits - 1) * k.pps);
  return 0;
}

extern "C" int yolo_bn_train_stats(const void* z, long long pixels, int c, const float* gamma, const float* beta, float eps, float momentum,
                                   float* running_mean, float* running_var, float* saved, void* ws, size_t ws_bytes, yolo_stream_t s) {
  if (const int rc = bn_check(pixels, c, "bn_train_stats")) return rc;
  YOLO_REQUIRE(pixels >= 2, "bn_train_stats: batch statistics need more than one value per channel (pixels %lld)", pixels);
  YOLO_REQUIRE(eps >= 0.f && momentum >= 0.f && momentum <= 1.f, "bn_train_stats: eps %g / momentum %g out of range", (double)eps, (double)momentum);
  YOLO_REQUIRE(z && gamma && beta && saved && ws, "bn_train_stats: null pointer");
  YOLO_REQUIRE(al(z, 16) && al(saved, 16) && al(ws, 16) && al(gamma, 4) && al(beta, 4) && al(running_mean, 4) && al(running_var, 4),
               "bn_train_stats: misaligned pointer");
  const BnPick k = choose_bn(pixels, c, yolo_conv::launch_cus());
  const size_t need = bn_ws_bytes(c, k.splits);
  if (ws_bytes < need) return yolo_set_error(YOLO_E_WORKSPACE, "bn_train_stats: workspace %zu < %zu bytes", ws_bytes, need);
  ReduceArgs a = reduce_args(k, pixels, c);
  a.z = (const bf16_t*)z;
  a.part = reinterpret_cast<double*>((char*)ws + (size_t)2 * c * sizeof(float));
  hipLaunchKernelGGL(stats_kernel, dim3(k.splits, k.tiles_y), dim3(256), 0, (hipStream_t)s, a);
  if (const int rc = yolo_check_launch("bn_train_stats", " (reduce)")) return rc;
  hipLaunchKernelGGL(stats_finalize_kernel, dim3(blocks_for(c)), dim3(256), 0, (hipStream_t)s, (const double*)a.part, k.splits, c, (long)pixels,
                     gamma, beta, eps, momentum, running_mean, running_var, saved);
  return yolo_check_launch("bn_train_stats", " (finalize)");
}

extern "C" int yolo_bn_eval_stats(const float* gamma, const float* beta, const float* running_mean, const float* running_var, int c, float eps,
                                  float* saved, yolo_stream_t s) {
  if (const int rc = bn_check(1, c, "bn_eval_stats")) return rc;
  YOLO_REQUIRE(eps >= 0.f, "bn_eval_stats: eps %g out of range", (double)eps);
  YOLO_REQUIRE(gamma && beta && running_mean && running_var && saved, "bn_eval_stats: null pointer");
  YOLO_REQUIRE(al(saved, 16) && al(gamma, 4) && al(beta, 4) && al(running_mean, 4) && al(running_var, 4), "bn_eval_stats: misaligned pointer");
  hipLaunchKernelGGL(eval_stats_kernel, dim3(blocks_for(c)), dim3(256), 0, (hipStream_t)s, gamma, beta, running_mean, running_var, c, eps, saved);
  return yolo_check_launch("bn_eval_stats");
}

// yolo_bn_act_fwd and yolo_bn_clamp_fwd after their own activation check
static int bn_fwd(const char* fn, const void* z, const float* saved, void* y, long long pixels, int c, const BnAct& act, yolo_stream_t s) {
  YOLO_REQUIRE(z && saved && y, "%s: null pointer", fn);
  YOLO_REQUIRE(al(z, 16) && al(saved, 16) && al(y, 16), "%s: misaligned pointer", fn);
  const long total = (long)pixels * (c / 8);
  hipLaunchKernelGGL(act_fwd_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)z, saved, (bf16_t*)y, total, c, c / 8,
                     act);
  return yolo_check_launch(fn);
}

extern "C" int yolo_bn_act_fwd(const void* z, const float* saved, void* y, long long pixels, int c, int act, yolo_stream_t s) {
  if (const int rc = bn_check(pixels, c, "bn_act_fwd")) return rc;
  if (const int rc = act_check(act, "bn_act_fwd")) return rc;
  return bn_fwd("bn_act_fwd", z, saved, y, pixels, c, act_of(act), s);
}

extern "C" int yolo_bn_clamp_fwd(const void* z, const float* saved, void* y, long long pixels, int c, float lo, float hi, yolo_stream_t s) {
  if (const int rc = bn_check(pixels, c, "bn_clamp_fwd")) return rc;
  if (const int rc = clamp_check(lo, hi, "bn_clamp_fwd")) return rc;
  return bn_fwd("bn_clamp_fwd", z, saved, y, pixels, c, BnAct{kBnClamp, lo, hi}, s);
}

extern "C" int yolo_bn_act_pool_fwd(const void* z, const float* saved, void* y, void* idx, int n, int h, int w, int c, int act, yolo_stream_t s) {
  YOLO_REQUIRE(n > 0 && h > 0 && w > 0, "bn_act_pool_fwd: empty shape (n %d, h %d, w %d)", n, h, w);
  if (const int rc = bn_check((long long)n * h * w, c, "bn_act_pool_fwd")) return rc;
  if (const int rc = act_check(act, "bn_act_pool_fwd")) return rc;
  YOLO_REQUIRE(h >= 2 && w >= 2, "bn_act_pool_fwd: empty output (the 2/2 pool of a %d x %d map)", h, w);
  YOLO_REQUIRE(h <= (1 << 20) && w <= (1 << 20), "bn_act_pool_fwd: shape out of range (h %d, w %d)", h, w);
  YOLO_REQUIRE(z && saved && y && idx, "bn_act_pool_fwd: null pointer");
  YOLO_REQUIRE(al(z, 16) && al(saved, 16) && al(y, 16) && al(idx, 8), "bn_act_pool_fwd: misaligned pointer");
  const int ho = h / 2, wo = w / 2;
  const long total = (long)n * ho * wo * (c / 8);
  hipLaunchKernelGGL(act_pool_fwd_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)z, saved, (bf16_t*)y, (uint8_t*)idx,
                     total, h, w, ho, wo, c, c / 8, act == YOLO_ACT_LEAKY01);
  return yolo_check_launch("bn_act_pool_fwd");
}

extern "C" int yolo_bn_act_add_fwd(const void* z, const float* saved, const void* residual, void* y, void* y_preadd, long long pixels, int c,
                                   int act, yolo_stream_t s) {
  if (const int rc = bn_check(pixels, c, "bn_act_add_fwd")) return rc;
  if (const int rc = act_check(act, "bn_act_add_fwd")) return rc;
  YOLO_REQUIRE(z && saved && residual && y, "bn_act_add_fwd: null pointer");
  YOLO_REQUIRE(al(z, 16) && al(saved, 16) && al(residual, 16) && al(y, 16) && al(y_preadd, 16), "bn_act_add_fwd: misaligned pointer");
  const long total = (long)pixels * (c / 8);
  const int leaky = act == YOLO_ACT_LEAKY01;
  if (y_preadd)
    hipLaunchKernelGGL(act_add_fwd_kernel<true>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)z, saved,
                       (const bf16_t*)residual, (bf16_t*)y, (bf16_t*)y_preadd, total, c, c / 8, leaky);
  else
    hipLaunchKernelGGL(act_add_fwd_kernel<false>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)z, saved,
                       (const bf16_t*)residual, (bf16_t*)y, (bf16_t*)nullptr, total, c, c / 8, leaky);
  return yolo_check_launch("bn_act_add_fwd");
}

// yolo_bn_act_bwd and yolo_bn_clamp_bwd after their own activation check
static int bn_bwd(const char* fn, const void* dy, int dy_dtype, const void* z, const float* saved, long long pixels, int c, const BnAct& act,
                  int batch_stats, void* g, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, yolo_stream_t s) {
  YOLO_REQUIRE(dy_dtype == YOLO_DT_BF16 || dy_dtype == YOLO_DT_F32, "%s: dy_dtype %d (YOLO_DT_BF16 or YOLO_DT_F32)", fn, dy_dtype);
  YOLO_REQUIRE(batch_stats == 0 || batch_stats == 1, "%s: batch_stats %d (0 or 1)", fn, batch_stats);
  YOLO_REQUIRE(!batch_stats || pixels >= 2, "%s: batch statistics need more than one value per channel (pixels %lld)", fn, pixels);
  YOLO_REQUIRE(dy && z && saved && ws, "%s: null pointer", fn);
  YOLO_REQUIRE(al(dy, 16) && al(z, 16) && al(saved, 16) && al(g, 16) && al(ws, 16) && al(dgamma, 4) && al(dbeta, 4), "%s: misaligned pointer", fn);
  const BnPick k = choose_bn(pixels, c, yolo_conv::launch_cus());
  const size_t need = bn_ws_bytes(c, k.splits);
  if (ws_bytes < need) return yolo_set_error(YOLO_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
  float* const c12 = (float*)ws;
  ReduceArgs a = reduce_args(k, pixels, c);
  a.z = (const bf16_t*)z, a.dy = dy, a.saved = saved, a.act = act;
  a.part = reinterpret_cast<double*>((char*)ws + (size_t)2 * c * sizeof(float));
  const bool f32 = dy_dtype == YOLO_DT_F32;
  if (f32) hipLaunchKernelGGL(bwd_reduce_kernel<float>, dim3(k.splits, k.tiles_y), dim3(256), 0, (hipStream_t)s, a);
  else hipLaunchKernelGGL(bwd_reduce_kernel<bf16_t>, dim3(k.splits, k.tiles_y), dim3(256), 0, (hipStream_t)s, a);
  if (const int rc = yolo_check_launch(fn, " (reduce)")) return rc;
  hipLaunchKernelGGL(bwd_finalize_kernel, dim3(blocks_for(c)), dim3(256), 0, (hipStream_t)s, (const double*)a.part, k.splits, c, (long)pixels,
                     batch_stats, dgamma, dbeta, c12);
  if (const int rc = yolo_check_launch(fn, " (finalize)")) return rc;
  if (!g) return 0;                  // only dgamma / dbeta were asked for
  const long total = (long)pixels * (c / 8);
  if (f32)
    hipLaunchKernelGGL(act_bwd_kernel<float>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const float*)dy, (const bf16_t*)z, saved,
                       (const float*)c12, (bf16_t*)g, total, c, c / 8, act);
  else
    hipLaunchKernelGGL(act_bwd_kernel<bf16_t>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)dy, (const bf16_t*)z, saved,
                       (const float*)c12, (bf16_t*)g, total, c, c / 8, act);
  return yolo_check_launch(fn, " (apply)");
}

extern "C" int yolo_bn_add_rounded_fwd(const void* z, const float* saved, const void* residual, void* y, long long pixels, int c, yolo_stream_t s) {
  if (const int rc = bn_check(pixels, c, "bn_add_rounded_fwd")) return rc;
  YOLO_REQUIRE(z && saved && residual && y, "bn_add_rounded_fwd: null pointer");
  YOLO_REQUIRE(al(z, 16) && al(saved, 16) && al(residual, 16) && al(y, 16), "bn_add_rounded_fwd: misaligned pointer");
  const long total = (long)pixels * (c / 8);
  hipLaunchKernelGGL(add_rounded_fwd_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)z, saved,
                     (const bf16_t*)residual, (bf16_t*)y, total, c, c / 8);
  return yolo_check_launch("bn_add_rounded_fwd");
}

extern "C" int yolo_bn_act_bwd(const void* dy, int dy_dtype, const void* z, const float* saved, long long pixels, int c, int act, int batch_stats,
                               void* g, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, yolo_stream_t s) {
  if (const int rc = bn_check(pixels, c, "bn_act_bwd")) return rc;
  if (const int rc = act_check(act, "bn_act_bwd")) return rc;
  return bn_bwd("bn_act_bwd", dy, dy_dtype, z, saved, pixels, c, act_of(act), batch_stats, g, dgamma, dbeta, ws, ws_bytes, s);
}

extern "C" int yolo_bn_clamp_bwd(const void* dy, int dy_dtype, const void* z, const float* saved, long long pixels, int c, float lo, float hi,
                                 int batch_stats, void* g, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, yolo_stream_t s) {
  if (const int rc = bn_check(pixels, c, "bn_clamp_bwd")) return rc;
  if (const int rc = clamp_check(lo, hi, "bn_clamp_bwd")) return rc;
  return bn_bwd("bn_clamp_bwd", dy, dy_dtype, z, saved, pixels, c, BnAct{kBnClamp, lo, hi}, batch_stats, g, dgamma, dbeta, ws, ws_bytes, s);
}
