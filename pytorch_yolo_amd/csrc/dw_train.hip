// Backward of the depthwise 3x3 conv of an inverted residual as it trains (torchvision's ConvBNReLU with groups = channels: Conv2d(c, c, 3,
// stride, 1, groups=c, bias=False)), bf16 mode.  x [n, h, w, c], g [n, ho, wo, c] and dx [n, h, w, c] are dense bf16 NHWC,
// c % 8 == 0, ho = (h - 1) / stride + 1 (wo likewise), stride 1 or 2; w is fp32 [9][c], tap-major (yolo_dwconv3x3_fwd's layout), dw is fp32
// [c][3][3] (the parameter's layout).  The forward is yolo_dwconv3x3_fwd with act none and a zero bias.
//   dw_dgrad_kernel     a gather, one thread per chunk of 8 channels of one INPUT pixel: acc = 0; for the taps (kh, kw) in row-major order
//                       whose output pixel oh = (ih + 1 - kh) / stride, ow = (iw + 1 - kw) / stride is integral and inside the map:
//                       acc = fmaf(f32(g[n, oh, ow]), w[3 kh + kw], acc); dx = bf16_rne(acc).  Every dx element is written.
//   dw_wgrad_kernel     dw[ch][kh][kw] = sum_{n, oh, ow} f32(g[n, oh, ow, ch]) * f32(x[n, stride oh + kh - 1, stride ow + kw - 1, ch]) over the
//                       in-bounds taps: the products are exact in fp32 (two bf16 factors), the sums float64.  A workgroup is 3 x 256 threads:
//                       thread = (kh, pixel slot, chunk column) holds the 3 taps of its kernel row for its 8 channels - 24 float64
//                       accumulators, 48 registers; nine taps in one thread would be 144.  The output pixels are dealt to blockIdx.x in
//                       passes of `rows` pixels; the slots of a column meet in LDS, one kernel column (8 doubles a thread) at a time, and are
//                       added in slot order into the split's partial [9][c] of the caller's workspace.
//   dw_wgrad_finalize_kernel   one thread per (tap, channel): the partials in split order, one rounding to fp32.
// The two entries with a batch-normed operand take the expand conv's output zin and its saved [4][c] instead of the
// materialised activation: y = bf16_rne(fminf(fmaxf(fl(fl(f32(zin) * scale) + shift), lo), hi)) inside the map - yolo_bn_clamp_fwd's value,
// two fp32 roundings, no fma - and y = 0 outside it (the padding is a zero of y, not the clamp of a zero zin).
//   dw_bnin_strip_kernel   yolo_dwconv3x3_fwd's strip form (pointwise.hip) with act none and no bias: one thread = 8 channels of a strip of
//                       8 output rows, 72 weights and 16 floats of scale / shift in registers; load_row transforms what it loads, so the
//                       row slots hold packed bf16 y and the tap loop is that kernel's: acc = 0, the taps row by row, one fma a tap, one
//                       rounding.  z is bit-equal to yolo_dwconv3x3_fwd on the materialised y.
//   dw_wgrad_kernel<true>  dw_wgrad_kernel with the x operand transformed after the load; same split rule, workspace and finalize.
// No atomics, no read-modify-write; every output element and every used workspace byte is written once, in an order fixed by the shape and
// yolo_set_launch_cus: two runs give the same bits.  Built with -ffp-contract=off.
#include "common.h"

namespace yolo_conv {
int launch_cus();   // conv_igemm.hip: compute units the coming launches may use
}

namespace {

constexpr int kWgradThreads = 768;      // 3 kernel rows x 256 (pixel slot, chunk column) pairs
constexpr int kTileChunks = 256;        // chunk columns of one column tile (2048 channels): blockIdx.y
constexpr int kUnroll = 2;              // passes a thread has in flight (4 loads of 16 bytes each)
constexpr int kMinPixels = 32;          // output pixels a split is worth: its partial is 72 c bytes, its operands 4 c bytes a pixel
constexpr int kMaxSplits = 2048;
constexpr int kFinalBatch = 8;          // splits a finalize thread has in flight

struct DwShape {
  int n, h, w, c, stride, ho, wo, chunks;
  long m_out;                           // n ho wo
};

// The split rule of the weight gradient: a pure function of (shape, compute units).  A pass is `rows` consecutive output pixels x
// `width` chunk columns; the passes are dealt to `splits` workgroups, `pps` each, the last one ragged.  No split is empty.
struct DwPick {
  int tiles_y, width, rows;
  long passes, pps;
  int splits;
};

DwPick choose_dw(const DwShape& d, int n_cu) {
  DwPick k;
  k.tiles_y = (d.chunks + kTileChunks - 1) / kTileChunks;
  k.width = d.chunks < kTileChunks ? d.chunks : kTileChunks;
  k.rows = 256 / k.width;
  k.passes = (d.m_out + k.rows - 1) / k.rows;
  long want = (n_cu + k.tiles_y - 1) / k.tiles_y;
  const long by_work = d.m_out / kMinPixels > 1 ? d.m_out / kMinPixels : 1;
  if (want > by_work) want = by_work;
  if (want > kMaxSplits) want = kMaxSplits;
  if (want > k.passes) want = k.passes;
  if (want < 1) want = 1;
  k.pps = (k.passes + want - 1) / want;
  k.splits = (int)((k.passes + k.pps - 1) / k.pps);
  return k;
}

size_t dw_ws_bytes(int c, int splits) { return (size_t)splits * 9 * c * sizeof(double); }

struct DgradArgs {
  const bf16_t* g;
  const float* w;
  bf16_t* dx;
  long total;                           // n h w chunks
  int h, w_, ho, wo, c, chunks, stride;
};

__global__ __launch_bounds__(256) void dw_dgrad_kernel(const DgradArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  const int ch = (int)(i % a.chunks);
  const long pix = i / a.chunks;                                             // (n, ih, iw) of the input map
  const int iw = (int)(pix % a.w_);
  const long t = pix / a.w_;
  const int ih = (int)(t % a.h);
  const long n = t / a.h;
  const bf16_t* gn = a.g + (size_t)n * a.ho * a.wo * a.c + (size_t)ch * 8;
  const float* wc = a.w + (size_t)ch * 8;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int th = ih + 1 - kh;
    if (th < 0 || (th % a.stride) != 0) continue;
    const int oh = th / a.stride;
    if (oh >= a.ho) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int tw = iw + 1 - kw;
      if (tw < 0 || (tw % a.stride) != 0) continue;
      const int ow = tw / a.stride;
      if (ow >= a.wo) continue;
      const bf16x8 gv = *reinterpret_cast<const bf16x8*>(gn + ((size_t)oh * a.wo + ow) * a.c);
      const float* wp = wc + (size_t)(3 * kh + kw) * a.c;
      const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp), w1 = *reinterpret_cast<const f32x4*>(wp + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[j] = fmaf((float)gv[j], w0[j], acc[j]);
        acc[4 + j] = fmaf((float)gv[4 + j], w1[j], acc[4 + j]);
      }
    }
  }
  bf16x8 out;
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = (bf16_t)acc[j];
  *reinterpret_cast<bf16x8*>(a.dx + i * 8) = out;
}

struct WgradArgs {
  const bf16_t* x;
  const bf16_t* g;
  double* part;                         // [splits][9][c]
  long m_out, pixels_per_split;
  int h, w_, ho, wo, c, chunks, stride, width, rows;
  const float* saved;                   // BNIN only: [4][c] of the operand's batch norm, and its clamp
  float lo, hi;
};

// yolo_bn_clamp_fwd's value of 8 channels: two fp32 roundings (the file is built without contraction), the clamp, one rounding to bf16
__device__ __forceinline__ bf16x8 bnin8(const bf16x8 v, const float (&scale)[8], const float (&shift)[8], float lo, float hi) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float t = (float)v[j] * scale[j] + shift[j];
    o[j] = (bf16_t)fminf(fmaxf(t, lo), hi);
  }
  return o;
}

__device__ __forceinline__ void load_scale_shift(const float* saved, int c, size_t c0, float (&scale)[8], float (&shift)[8]) {
  const float* sc = saved + 2 * (size_t)c + c0;
  const float* sh = saved + 3 * (size_t)c + c0;
  const f32x4 a0 = *reinterpret_cast<const f32x4*>(sc), a1 = *reinterpret_cast<const f32x4*>(sc + 4);
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(sh), b1 = *reinterpret_cast<const f32x4*>(sh + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) scale[j] = a0[j], scale[4 + j] = a1[j], shift[j] = b0[j], shift[4 + j] = b1[j];
}

// BNIN: a.x is zin and every loaded operand goes through bnin8 (a tap outside the map is never loaded: it adds nothing, as a zero of y)
template <bool BNIN>
__global__ __launch_bounds__(kWgradThreads) void dw_wgrad_kernel(const WgradArgs a) {
  __shared__ double lds[8 * kWgradThreads];
  const int kh = threadIdx.x / 256, t256 = threadIdx.x % 256;
  const int col = t256 % a.width, slot = t256 / a.width;
  const int chunk0 = blockIdx.y * kTileChunks;
  const bool active = slot < a.rows && chunk0 + col < a.chunks;
  const long p0 = (long)blockIdx.x * a.pixels_per_split;
  const long p1 = p0 + a.pixels_per_split < a.m_out ? p0 + a.pixels_per_split : a.m_out;
  double acc[3][8];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = 0.0;
  if (active) {
    const size_t c0 = (size_t)(chunk0 + col) * 8;
    float scale[8], shift[8];
    if constexpr (BNIN) load_scale_shift(a.saved, a.c, c0, scale, shift);
    for (long p = p0 + slot; p < p1; p += (long)kUnroll * a.rows) {
      bf16x8 gv[kUnroll], xv[kUnroll][3];
      bool ok[kUnroll][3];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const long q = p + (long)u * a.rows;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) ok[u][kw] = false;
        if (q >= p1) continue;
        const int ow = (int)(q % a.wo);
        const long t = q / a.wo;
        const int oh = (int)(t % a.ho);
        const long n = t / a.ho;
        const int ih = a.stride * oh + kh - 1;
        if (ih < 0 || ih >= a.h) continue;                         // this kernel row is outside the map for this output row
        gv[u] = *reinterpret_cast<const bf16x8*>(a.g + (size_t)q * a.c + c0);
        const bf16_t* xr = a.x + ((size_t)n * a.h + ih) * a.w_ * a.c + c0;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int iw = a.stride * ow + kw - 1;
          ok[u][kw] = iw >= 0 && iw < a.w_;
          if (ok[u][kw]) {
            xv[u][kw] = *reinterpret_cast<const bf16x8*>(xr + (size_t)iw * a.c);
            if constexpr (BNIN) xv[u][kw] = bnin8(xv[u][kw], scale, shift, a.lo, a.hi);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          if (ok[u][kw]) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[kw][j] += (double)((float)gv[u][j] * (float)xv[u][kw][j]);   // exact in fp32: 8 x 8 significant bits
          }
        }
      }
    }
  }
  // the slots of a chunk column, added in slot order, one kernel column at a time: lds[j][thread] (consecutive threads, consecutive doubles)
  double* out = a.part + (size_t)blockIdx.x * 9 * a.c;
#pragma unroll
  for (int kw = 0; kw < 3; ++kw) {
    if (kw) __syncthreads();
    if (slot < a.rows) {
#pragma unroll
      for (int j = 0; j < 8; ++j) lds[j * kWgradThreads + threadIdx.x] = acc[kw][j];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 3 * 8 * a.width; o += kWgradThreads) {
      const int cc = o % a.width, r = o / a.width;                 // r = khh * 8 + j
      const int khh = r >> 3, j = r & 7;
      if (chunk0 + cc >= a.chunks) continue;                       // the ragged last column tile
      double s = 0.0;
      for (int sl = 0; sl < a.rows; ++sl) s += lds[j * kWgradThreads + khh * 256 + sl * a.width + cc];
      out[(size_t)(3 * khh + kw) * a.c + (size_t)(chunk0 + cc) * 8 + j] = s;
    }
  }
}

// one thread per (tap, channel), channels fastest: the splits in split order, kFinalBatch loads issued before the first add
__global__ __launch_bounds__(256) void dw_wgrad_finalize_kernel(const double* __restrict__ part, int splits, int c, float* __restrict__ dw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 9 * c) return;
  const int tap = i / c, ch = i - tap * c;
  const double* p = part + i;
  const size_t stride = (size_t)9 * c;
  double s = 0.0;
  int k = 0;
  for (; k + kFinalBatch <= splits; k += kFinalBatch, p += kFinalBatch * stride) {
    double v[kFinalBatch];
#pragma unroll
    for (int b = 0; b < kFinalBatch; ++b) v[b] = p[b * stride];
#pragma unroll
    for (int b = 0; b < kFinalBatch; ++b) s += v[b];
  }
  for (; k < splits; ++k, p += stride) s += p[0];
  dw[(size_t)ch * 9 + tap] = (float)s;
}

// ---- the forward on a batch-normed operand -----------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int kStripRows = 8;           // output rows of a thread: yolo_dwconv3x3_fwd's strip

template <int S, int R>
__global__ __launch_bounds__(256) void dw_bnin_strip_kernel(const bf16_t* __restrict__ zin, const float* __restrict__ saved, float lo, float hi,
                                                            const float* __restrict__ wt, bf16_t* __restrict__ z, int h, int w, int c, int ho,
                                                            int wo, int strips, long total) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int cg = c / 8;
  const int g = (int)(t % cg);
  long p = t / cg;
  const int ow = (int)(p % wo);
  p /= wo;
  const int oh0 = (int)(p % strips) * R;
  const long b = p / strips;
  f32x2 wv[9][4];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const f32x4 l = *reinterpret_cast<const f32x4*>(wt + (size_t)k * c + g * 8), u = *reinterpret_cast<const f32x4*>(wt + (size_t)k * c + g * 8 + 4);
    wv[k][0] = f32x2{l[0], l[1]}, wv[k][1] = f32x2{l[2], l[3]}, wv[k][2] = f32x2{u[0], u[1]}, wv[k][3] = f32x2{u[2], u[3]};
  }
  float scale[8], shift[8];
  load_scale_shift(saved, c, (size_t)g * 8, scale, shift);
  const bf16_t* const xb = zin + (b * h) * (long)w * c + g * 8;
  const int wi0 = ow * S - 1;
  // a slot holds y: the transformed operand inside the map, zero outside it
  auto load_row = [&](int hi_, u32x4 (&row)[3]) {
    const bool rok = (unsigned)hi_ < (unsigned)h;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int wi = wi0 + j;
      if (rok && (unsigned)wi < (unsigned)w) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(xb + ((long)hi_ * w + wi) * c);
        row[j] = __builtin_bit_cast(u32x4, bnin8(v, scale, shift, lo, hi));
      } else {
        row[j] = u32x4{0, 0, 0, 0};
      }
    }
  };
  // input rows of output row oh0 + k: (oh0 + k) * S - 1 + {0, 1, 2}
  u32x4 rows[3][3];
  load_row(oh0 * S - 1, rows[0]);
  if (S == 1) load_row(oh0, rows[1]);
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int oh = oh0 + k;
    if (oh >= ho) break;
    // slots: at stride 1 the window slides by one row, at stride 2 by two (the last row becomes the first)
    constexpr int NS = 3;
    const int s0 = (S == 1 ? k : 2 * k) % NS, s1 = (s0 + 1) % NS, s2 = (s0 + 2) % NS;
    if (S == 1) {
      load_row(oh + 1, rows[s2]);
    } else {
      load_row(oh * 2, rows[s1]);
      load_row(oh * 2 + 1, rows[s2]);
    }
    f32x2 acc[4] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}};
    const int sl[3] = {s0, s1, s2};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const u32x4 v = rows[sl[i]][j];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          acc[e] = __builtin_elementwise_fma(f32x2{__uint_as_float(v[e] << 16), __uint_as_float(v[e] & 0xffff0000u)}, wv[i * 3 + j][e], acc[e]);
      }
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (bf16_t)acc[e >> 1][e & 1];
    *reinterpret_cast<bf16x8*>(z + ((b * ho + oh) * wo + ow) * (long)c + g * 8) = o;
  }
}

template <int S>
void launch_bnin_strip(const bf16_t* zin, const float* saved, float lo, float hi, const float* w, bf16_t* z, const DwShape& d, hipStream_t s) {
  const int strips = (d.ho + kStripRows - 1) / kStripRows;
  const long total = (long)d.n * strips * d.wo * d.chunks;
  hipLaunchKernelGGL((dw_bnin_strip_kernel<S, kStripRows>), dim3(blocks_for(total)), dim3(256), 0, s, zin, saved, lo, hi, w, z, d.h, d.w, d.c,
                     d.ho, d.wo, strips, total);
}

bool al(const void* p, int n) { return (uintptr_t)p % n == 0; }

// the bounds of a clamp, yolo_bn_clamp_fwd's: lo finite, hi finite or +inf, lo < hi (a NaN fails every comparison)
int clamp_check(float lo, float hi, const char* fn) {
  YOLO_REQUIRE(lo - lo == 0.f && hi == hi && lo < hi, "%s: clamp bounds lo %g, hi %g (lo finite, hi finite or +inf, lo < hi)", fn, (double)lo,
               (double)hi);
  return 0;
}

// what every entry asks of the shape
int dw_check(int n, int h, int w_, int c, int stride, const char* fn, DwShape* d) {
  YOLO_REQUIRE(n > 0 && h > 0 && w_ > 0, "%s: empty shape (n %d, h %d, w %d)", fn, n, h, w_);
  YOLO_REQUIRE(c > 0 && c % 8 == 0, "%s: c %d must be a positive multiple of 8", fn, c);
  YOLO_REQUIRE(stride == 1 || stride == 2, "%s: stride %d (1 or 2)", fn, stride);
  YOLO_REQUIRE(h <= (1 << 20) && w_ <= (1 << 20) && (long long)n * h * w_ <= 0x7fffffffLL && (long long)n * h * w_ * (c / 8) < kMaxThreads &&
                   (long long)n * h * w_ <= (1LL << 40) / c,
               "%s: shape out of range (n %d, h %d, w %d, c %d)", fn, n, h, w_, c);
  d->n = n, d->h = h, d->w = w_, d->c = c, d->stride = stride, d->chunks = c / 8;
  d->ho = (h - 1) / stride + 1, d->wo = (w_ - 1) / stride + 1;
  d->m_out = (long)n * d->ho * d->wo;
  return 0;
}

}  // namespace

extern "C" int yolo_dwconv3x3_bwd_data(const void* g, const float* w, void* dx, int n, int h, int w_, int c, int stride, yolo_stream_t s) {
  DwShape d;
  if (const int rc = dw_check(n, h, w_, c, stride, "dwconv3x3_bwd_data", &d)) return rc;
  YOLO_REQUIRE(g && w && dx, "dwconv3x3_bwd_data: null pointer");
  YOLO_REQUIRE(al(g, 16) && al(dx, 16) && al(w, 16), "dwconv3x3_bwd_data: misaligned pointer");
  DgradArgs a;
  a.g = (const bf16_t*)g, a.w = w, a.dx = (bf16_t*)dx;
  a.total = (long)n * h * w_ * d.chunks;
  a.h = h, a.w_ = w_, a.ho = d.ho, a.wo = d.wo, a.c = c, a.chunks = d.chunks, a.stride = stride;
  hipLaunchKernelGGL(dw_dgrad_kernel, dim3(blocks_for(a.total)), dim3(256), 0, (hipStream_t)s, a);
  return yolo_check_launch("dwconv3x3_bwd_data");
}

extern "C" size_t yolo_dwconv3x3_bwd_weight_workspace_bytes(int n, int h, int w_, int c, int stride) {
  DwShape d;
  if (dw_check(n, h, w_, c, stride, "dwconv3x3_bwd_weight_workspace_bytes", &d)) return 0;
  return dw_ws_bytes(c, choose_dw(d, yolo_conv::launch_cus()).splits);
}

extern "C" int yolo_dwconv3x3_bwd_weight_pick(int n, int h, int w_, int c, int stride, char* out, int out_len) {
  YOLO_REQUIRE(out && out_len > 0, "dwconv3x3_bwd_weight_pick: bad arguments");
  out[0] = 0;
  DwShape d;
  if (const int rc = dw_check(n, h, w_, c, stride, "dwconv3x3_bwd_weight_pick", &d)) return rc;
  const DwPick k = choose_dw(d, yolo_conv::launch_cus());
  snprintf(out, (size_t)out_len, "dw_wgrad<3x%dx%d,s%d> grid %dx%d passes %ld last %ld", k.rows, k.width, stride, k.splits, k.tiles_y, k.pps,
           k.passes - (long)(k.splits - 1) * k.pps);
  return 0;
}

// the body of the two weight-gradient entries: x is the operand itself, or zin with saved / lo / hi where BNIN
template <bool BNIN>
int dw_bwd_weight(const char* fn, const void* x, const float* saved, float lo, float hi, const void* g, float* dw, void* ws, size_t ws_bytes,
                  int n, int h, int w_, int c, int stride, yolo_stream_t s) {
  DwShape d;
  if (const int rc = dw_check(n, h, w_, c, stride, fn, &d)) return rc;
  if (BNIN) {
    if (const int rc = clamp_check(lo, hi, fn)) return rc;
    YOLO_REQUIRE(saved, "%s: null pointer", fn);
    YOLO_REQUIRE(al(saved, 16), "%s: misaligned pointer", fn);
  }
  YOLO_REQUIRE(x && g && dw && ws, "%s: null pointer", fn);
  YOLO_REQUIRE(al(x, 16) && al(g, 16) && al(ws, 16) && al(dw, 4), "%s: misaligned pointer", fn);
  const DwPick k = choose_dw(d, yolo_conv::launch_cus());
  const size_t need = dw_ws_bytes(c, k.splits);
  if (ws_bytes < need) return yolo_set_error(YOLO_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
  WgradArgs a;
  a.x = (const bf16_t*)x, a.g = (const bf16_t*)g, a.part = (double*)ws;
  a.m_out = d.m_out, a.pixels_per_split = k.pps * k.rows;
  a.h = h, a.w_ = w_, a.ho = d.ho, a.wo = d.wo, a.c = c, a.chunks = d.chunks, a.stride = stride, a.width = k.width, a.rows = k.rows;
  a.saved = saved, a.lo = lo, a.hi = hi;
  hipLaunchKernelGGL(dw_wgrad_kernel<BNIN>, dim3(k.splits, k.tiles_y), dim3(kWgradThreads), 0, (hipStream_t)s, a);
  if (const int rc = yolo_check_launch(fn, " (reduce)")) return rc;
  hipLaunchKernelGGL(dw_wgrad_finalize_kernel, dim3(blocks_for(9L * c)), dim3(256), 0, (hipStream_t)s, (const double*)a.part, k.splits, c, dw);
  return yolo_check_launch(fn, " (finalize)");
}

extern "C" int yolo_dwconv3x3_bwd_weight(const void* x, const void* g, float* dw, void* ws, size_t ws_bytes, int n, int h, int w_, int c,
                                         int stride, yolo_stream_t s) {
  return dw_bwd_weight<false>("dwconv3x3_bwd_weight", x, nullptr, 0.f, 0.f, g, dw, ws, ws_bytes, n, h, w_, c, stride, s);
}

extern "C" int yolo_dwconv3x3_bnin_bwd_weight(const void* zin, const float* saved_in, float lo, float hi, const void* g, float* dw, void* ws,
                                              size_t ws_bytes, int n, int h, int w_, int c, int stride, yolo_stream_t s) {
  return dw_bwd_weight<true>("dwconv3x3_bnin_bwd_weight", zin, saved_in, lo, hi, g, dw, ws, ws_bytes, n, h, w_, c, stride, s);
}

extern "C" int yolo_dwconv3x3_bnin_fwd(const void* zin, const float* saved_in, float lo, float hi, const float* w, void* z, int n, int h, int w_,
                                       int c, int stride, yolo_stream_t s) {
  DwShape d;
  if (const int rc = dw_check(n, h, w_, c, stride, "dwconv3x3_bnin_fwd", &d)) return rc;
  if (const int rc = clamp_check(lo, hi, "dwconv3x3_bnin_fwd")) return rc;
  YOLO_REQUIRE(zin && saved_in && w && z, "dwconv3x3_bnin_fwd: null pointer");
  YOLO_REQUIRE(al(zin, 16) && al(saved_in, 16) && al(w, 16) && al(z, 16), "dwconv3x3_bnin_fwd: misaligned pointer");
  if (stride == 1)
    launch_bnin_strip<1>((const bf16_t*)zin, saved_in, lo, hi, w, (bf16_t*)z, d, (hipStream_t)s);
  else
    launch_bnin_strip<2>((const bf16_t*)zin, saved_in, lo, hi, w, (bf16_t*)z, d, (hipStream_t)s);
  return yolo_check_launch("dwconv3x3_bnin_fwd");
}
