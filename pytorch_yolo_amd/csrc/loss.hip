// Validation loss on the device for gfx950: build_targets, compute_loss and the gradient of compute_loss with respect to p.
//
// Replaces the ATen dispatches and the Python loop of compute_loss / build_targets / wh_iou (reference utils/utils.py:99-197) on the
// raw head tensors p that `io, p = model(x)` returns in eval mode.  The gradient (yolo_loss_bwd, at the end of this file) is d loss /
// d p and nothing else: it stops at p - nothing here propagates through a convolution -, and it is a first derivative only.
//
// Arithmetic contract
//   * the target assignment (which anchor, kept or not, which cell, txy) is a chain of single IEEE fp32 operations in the reference's
//     order - this file is compiled with -ffp-contract=off and divides with __fdiv_rn - so indices and txy equal the reference's bit
//     for bit; twh carries the rounding of logf (<= 1 ulp);
//   * every loss term is formed in fp32 (expf / log1pf / logf), every sum of terms in float64, in an order that depends on nothing but
//     the shapes: lane-strided per thread, a shuffle tree across the wave64, then the four waves through LDS in wave order.  No atomic,
//     no cross-workgroup handshake: bit-identical from run to run, independent of how workgroups are scheduled;
//   * a layer's contribution is formed the way the reference forms it: the mean rounded to fp32, times the fp32 gain k * h[...],
//     accumulated over the layers in fp32 (:146-154); loss = ((lxy + lwh) + lconf) + lcls (:155).
//
// Launches (all on the caller's stream, nothing synchronises with the host, every call re-initialises what it reads):
//   memset        the tconf map, one byte per (image, anchor, cell) of every layer
//   loss_assign   one thread per (layer, target): wh_iou against the layer's anchors, first maximum, iou > iou_thresh, cell and
//                 offsets; a fixed-slot record per (layer, target) - slot order is target order, so nothing is compacted - and an
//                 idempotent byte store of 1 into the tconf map (duplicate cells are harmless).  A kept target outside the batch /
//                 grid / class range is NOT assigned; its record carries a flag instead (the reference raises an IndexError there)
//   loss_conf     the hot part (806,400 rows for 32 YOLOv3-SPP 640 images): a workgroup owns kConfRows consecutive rows of one layer,
//                 reads word 4 of each row and the row's tconf byte - never the rest of the (5 + nc)-float row -, forms
//                 max(x, 0) - x t + log1pf(expf(-|x|)) and stores ONE float64 partial
//   loss_terms    one wave64 per record: the xy / wh terms and the class term of a kept target (the lanes share the class logits:
//                 maximum and sum of exponentials by shuffle trees), four float64 values per record.  Walking the records inside the
//                 one-workgroup finish kernel instead - a thread per record, 2 x nc dependent loads each - took 165 us of a 188 us
//                 call on the YOLOv3-SPP 640 x 32 shapes with 512 targets and nc = 80 (rocprofv3 kernel trace)
//   loss_finish   one workgroup: per layer the conf partials and the records' terms in a fixed order, the means and gains;
//                 writes out[5] = (lxy, lwh, lconf, lcls, loss) and status = (flagged targets, kept targets per layer)
//
// Launches of the gradient (yolo_loss_bwd; the same memset and loss_assign first: it uses nothing a forward call left behind):
//   loss_grad_dense  the hot part: writes EVERY element of every gradient tensor (274 MB on the shapes above).  The tensor of a layer
//                    is treated as one flat float array; a thread owns kGradVecs 16-byte pieces of it, 4 KiB apart, so a wave64 stores
//                    1 KiB of consecutive bytes per instruction whatever the row length (6, 8, 85 floats: rows are not 16-byte
//                    aligned, the pieces are).  A piece holds at most one word 4 (rows are >= 6 floats); only the lanes whose piece
//                    holds one read anything: that word of p and the row's tconf byte.  Every other word is +0.0
//   loss_grad_cells  one wave64 per record.  The records of a layer that share the cell (b, a, gj, gi) share the row of p; the one in
//                    the lowest slot owns the cell, the others leave.  The owner counts the layer's valid records and sums their class
//                    weights (float64, lane-strided, shuffle tree: the same bits in every wave), then sums the sharers' terms word by
//                    word in slot order (float64) and STORES words 0-3 and 5.. of the row - a plain store over the zeros of the dense
//                    pass, which ran before it on the stream; word 4 belongs to the dense pass.  No atomic anywhere: the result does
//                    not depend on how workgroups are scheduled.  Every wave walks the nt records of its layer twice or three times:
//                    quadratic in nt, 0.8 M record reads at nt = 512
// Gradient arithmetic: fp32 terms; G = *grad_loss is folded into the gain first (G * gain, then / n), so that a call with G and a
// call with G = 1 and the gains scaled by G agree bit for bit whenever G * gain is exact.
#include "common.h"

namespace {

constexpr int kMaxLayers = 4;
constexpr int kMaxAnchors = 8;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / YOLO_WAVE;
constexpr int kConfRows = 1024;      // rows of one loss_conf workgroup: four per thread
constexpr int kRecWords = 12;        // valid, b, a, gj, gi, cls, txy[2], twh[2], flagged, 0  (48 bytes)
constexpr int kTermWords = 4;        // float64 per record: xy terms, wh terms, class numerator, class denominator
constexpr int kGradVecs = 4;         // 16-byte stores of one loss_grad_dense thread
constexpr int kGradStep = kThreads * 4;               // floats between two of them: one store instruction of the workgroup
constexpr int kGradChunk = kGradStep * kGradVecs;     // floats of one loss_grad_dense workgroup (16 KiB)

struct Geom {
  int nl, bs, nc, nt;
  int na[kMaxLayers], ny[kMaxLayers], nx[kMaxLayers];
  int rows[kMaxLayers];              // bs * na * ny * nx
  int wg_first[kMaxLayers + 1];      // first loss_conf workgroup of a layer
  long tconf_off[kMaxLayers];        // first tconf byte of a layer
  float anchors[kMaxLayers][kMaxAnchors][2];
};
struct Heads {
  const float* p[kMaxLayers];
};
struct Gains {
  float xy, wh, cls, conf;
};
struct Grads {
  float* g[kMaxLayers];
};
struct GradGeom {
  int wg_first[kMaxLayers + 1];      // first loss_grad_dense workgroup of a layer
  unsigned step_rows, step_words;    // kGradStep floats = step_rows rows + step_words words
};

// workspace: records int32 [nl][max(nt, 1)][kRecWords] | tconf uint8 [sum rows, each layer on a 256-byte boundary] | partials f64
//            | terms f64 [nl][max(nt, 1)][kTermWords]
struct Carved {
  int32_t* rec;
  uint8_t* tconf;
  double* partials;
  double* terms;
  size_t tconf_bytes, bytes;
};
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

inline Carved carve(void* base, const Geom& g) {
  Carved c;
  char* p = (char*)base;
  c.rec = (int32_t*)p;
  p += align256((size_t)g.nl * (size_t)(g.nt > 0 ? g.nt : 1) * kRecWords * 4);
  c.tconf = (uint8_t*)p;
  c.tconf_bytes = 0;
  for (int l = 0; l < g.nl; ++l) c.tconf_bytes = (size_t)g.tconf_off[l] + align256((size_t)g.rows[l]);
  p += c.tconf_bytes;
  c.partials = (double*)p;
  p += align256((size_t)g.wg_first[g.nl] * 8);
  c.terms = (double*)p;
  p += align256((size_t)g.nl * (size_t)(g.nt > 0 ? g.nt : 1) * kTermWords * 8);
  c.bytes = (size_t)(p - (char*)base);
  return c;
}

// the small per-layer tables live in the kernel arguments; a select chain instead of an index keeps them out of scratch memory
template <typename T, int N>
__device__ __forceinline__ T pick(const T (&a)[N], int l) {
  static_assert(N >= kMaxLayers, "one entry per layer");
  T v = a[0];
#pragma unroll
  for (int i = 1; i < kMaxLayers; ++i) v = (l == i) ? a[i] : v;
  return v;
}

// sum over the workgroup in a fixed order: shuffle tree inside each wave64, then the waves in wave order; every thread gets the sum
__device__ __forceinline__ double block_sum(double v, double* s_w) {
#pragma unroll
  for (int off = YOLO_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
  __syncthreads();                                         // (s_w of the previous call has been read by everyone)
  if ((threadIdx.x & (YOLO_WAVE - 1)) == 0) s_w[threadIdx.x / YOLO_WAVE] = v;
  __syncthreads();
  double t = s_w[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) t += s_w[w];
  return t;
}

// BCEWithLogits of one element in the stable form
__device__ __forceinline__ float bce_logits(float x, float t) { return (fmaxf(x, 0.f) - x * t) + log1pf(expf(-fabsf(x))); }

// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void loss_assign_kernel(const Geom g, const float* __restrict__ targets, float iou_thresh,
                                                               int32_t* __restrict__ rec, uint8_t* __restrict__ tconf) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= g.nl * g.nt) return;
  const int l = idx / g.nt, t = idx - l * g.nt;
  const int na = pick(g.na, l), ny = pick(g.ny, l), nx = pick(g.nx, l);
  const float* tg = targets + (long)t * 6;
  const float img = tg[0], cls = tg[1], x = tg[2], y = tg[3], w = tg[4], h = tg[5];
  const float nxf = (float)nx, nyf = (float)ny;            // n_grids = (nx, ny), yolo_layer.py:111
  const float gw = w * nxf, gh = h * nyf;                  // :169
  float best = 0.f, baw = 1.f, bah = 1.f;
  int a = -1;
#pragma unroll
  for (int i = 0; i < kMaxAnchors; ++i) {
    if (i < na) {
      float aw = g.anchors[0][i][0], ah = g.anchors[0][i][1];
#pragma unroll
      for (int k = 1; k < kMaxLayers; ++k) {
        aw = (l == k) ? g.anchors[k][i][0] : aw;
        ah = (l == k) ? g.anchors[k][i][1] : ah;
      }
      const float inter = fminf(aw, gw) * fminf(ah, gh);                       // wh_iou, :116
      const float uni = ((aw * ah + 1e-16f) + gw * gh) - inter;                // :119
      const float iou = __fdiv_rn(inter, uni);                                 // :121
      if (i == 0 || iou > best) {                                              // first maximum, :172
        best = iou;
        baw = aw;
        bah = ah;
        a = i;
      }
    }
  }
  const bool kept = best > iou_thresh;                                         // :177
  const float bf = truncf(img), cf = truncf(cls);                              // .long(), :181
  const float gx = x * nxf, gy = y * nyf;                                      // :182
  const float gif = truncf(gx), gjf = truncf(gy);                              // :183
  // every comparison is false for a NaN: a NaN anywhere is out of range
  const bool in_range = bf >= 0.f && bf < (float)g.bs && cf >= 0.f && cf < (float)g.nc && gif >= 0.f && gif < nxf && gjf >= 0.f &&
                        gjf < nyf;
  const bool valid = kept && in_range;
  int32_t* r = rec + ((long)l * g.nt + t) * kRecWords;
  int b = 0, gi = 0, gj = 0, c = 0;
  float tx = 0.f, ty = 0.f, tw = 0.f, th = 0.f;
  if (valid) {
    b = (int)bf;
    c = (int)cf;
    gi = (int)gif;
    gj = (int)gjf;
    tx = gx - floorf(gx);                                                      // :187
    ty = gy - floorf(gy);
    tw = logf(__fdiv_rn(gw, baw));                                             // :190
    th = logf(__fdiv_rn(gh, bah));
    tconf[pick(g.tconf_off, l) + (((long)b * na + a) * ny + gj) * nx + gi] = 1;   // :144
  }
  r[0] = valid ? 1 : 0;
  r[1] = b;
  r[2] = valid ? a : 0;
  r[3] = gj;
  r[4] = gi;
  r[5] = c;
  r[6] = __float_as_int(tx);
  r[7] = __float_as_int(ty);
  r[8] = __float_as_int(tw);
  r[9] = __float_as_int(th);
  r[10] = (kept && !in_range) ? 1 : 0;
  r[11] = 0;
}

// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void loss_conf_kernel(const Geom g, const Heads hd, const uint8_t* __restrict__ tconf,
                                                             double* __restrict__ partials) {
  __shared__ double s_w[kWaves];
  const int wg = blockIdx.x;
  int l = 0;
#pragma unroll
  for (int i = 1; i < kMaxLayers; ++i) l = (i < g.nl && wg >= g.wg_first[i]) ? i : l;
  const int rows = pick(g.rows, l);
  const int r0 = (wg - pick(g.wg_first, l)) * kConfRows;
  const int r1 = min(r0 + kConfRows, rows);
  const float* __restrict__ pl = pick(hd.p, l);
  const uint8_t* __restrict__ tc = tconf + pick(g.tconf_off, l);
  const long no = g.nc + 5;
  double acc = 0.0;
  for (int r = r0 + (int)threadIdx.x; r < r1; r += kThreads)
    acc += (double)bce_logits(pl[(long)r * no + 4], tc[r] ? 1.f : 0.f);        // :154
  const double s = block_sum(acc, s_w);
  if (threadIdx.x == 0) partials[wg] = s;
}

// ---------------------------------------------------------------------------------------------------
// one wave64 per (layer, target) record; every branch below is wave-uniform
__global__ __launch_bounds__(kThreads) void loss_terms_kernel(const Geom g, const Heads hd, const int32_t* __restrict__ rec,
                                                              const float* __restrict__ class_weight, double* __restrict__ terms) {
  const int lane = threadIdx.x & (YOLO_WAVE - 1);
  const int slot = blockIdx.x * kWaves + (int)(threadIdx.x / YOLO_WAVE);
  if (slot >= g.nl * g.nt) return;
  const int l = slot / g.nt;
  const int32_t* r = rec + (long)slot * kRecWords;
  double* o = terms + (long)slot * kTermWords;
  if (!r[0]) {
    if (lane < kTermWords) o[lane] = 0.0;
    return;
  }
  const int na = pick(g.na, l), ny = pick(g.ny, l), nx = pick(g.nx, l);
  const int no = g.nc + 5;
  const float* __restrict__ pi = pick(hd.p, l) + ((((long)r[1] * na + r[2]) * ny + r[3]) * nx + r[4]) * no;      // :143
  const int c = r[5];
  double num, den = 1.0;
  if (g.nc > 1) {                                                              // CrossEntropyLoss, :150
    float m = -INFINITY;
    for (int k = lane; k < g.nc; k += YOLO_WAVE) m = fmaxf(m, pi[5 + k]);
#pragma unroll
    for (int off = YOLO_WAVE / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    double se = 0.0;
    for (int k = lane; k < g.nc; k += YOLO_WAVE) se += (double)expf(pi[5 + k] - m);
#pragma unroll
    for (int off = YOLO_WAVE / 2; off > 0; off >>= 1) se += __shfl_down(se, off);
    const float ce = (logf((float)se) + m) - pi[5 + c];                        // (lane 0 holds the whole sum)
    const float wc = class_weight ? class_weight[c] : 1.f;
    num = (double)(wc * ce);
    den = (double)wc;
  } else {                                                                     // BCEWithLogits on the class INDEX, :152
    num = (double)bce_logits(pi[5], (float)c);
  }
  if (lane == 0) {
    const float d0 = __fdiv_rn(1.f, 1.f + expf(-pi[0])) - __int_as_float(r[6]);
    const float d1 = __fdiv_rn(1.f, 1.f + expf(-pi[1])) - __int_as_float(r[7]);
    const float e0 = pi[2] - __int_as_float(r[8]), e1 = pi[3] - __int_as_float(r[9]);
    o[0] = (double)(d0 * d0) + (double)(d1 * d1);                              // :146
    o[1] = (double)(e0 * e0) + (double)(e1 * e1);                              // :147
    o[2] = num;
    o[3] = den;
  }
}

// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void loss_finish_kernel(const Geom g, const int32_t* __restrict__ rec,
                                                               const double* __restrict__ partials, const double* __restrict__ terms,
                                                               const Gains gains, float* __restrict__ out,
                                                               int32_t* __restrict__ status) {
  __shared__ double s_w[kWaves];
  const int tid = threadIdx.x;
  float lxy = 0.f, lwh = 0.f, lconf = 0.f, lcls = 0.f;
  for (int l = 0; l < g.nl; ++l) {
    // conf: the partials of this layer
    const int rows = pick(g.rows, l);
    const int w0 = pick(g.wg_first, l), w1 = w0 + (rows + kConfRows - 1) / kConfRows;
    double acc = 0.0;
    for (int i = w0 + tid; i < w1; i += kThreads) acc += partials[i];
    const double conf_sum = block_sum(acc, s_w);
    lconf = lconf + gains.conf * (float)(conf_sum / (double)rows);             // :154
    // the records of this layer (the terms of a record that is not valid are zero)
    double sxy = 0.0, swh = 0.0, snum = 0.0, sden = 0.0, cnt = 0.0;
    for (int t = tid; t < g.nt; t += kThreads) {
      const long slot = (long)l * g.nt + t;
      const double* o = terms + slot * kTermWords;
      sxy += o[0];
      swh += o[1];
      snum += o[2];
      sden += o[3];
      cnt += rec[slot * kRecWords] ? 1.0 : 0.0;
    }
    sxy = block_sum(sxy, s_w);
    swh = block_sum(swh, s_w);
    snum = block_sum(snum, s_w);
    sden = block_sum(sden, s_w);
    cnt = block_sum(cnt, s_w);
    if (cnt > 0.0) {                                                           // :142
      lxy = lxy + gains.xy * (float)(sxy / (2.0 * cnt));
      lwh = lwh + gains.wh * (float)(swh / (2.0 * cnt));
      lcls = lcls + gains.cls * (float)(snum / sden);
    }
    if (tid == 0) status[1 + l] = (int)cnt;
  }
  // targets the assignment refused on at least one layer
  double flagged = 0.0;
  for (int t = tid; t < g.nt; t += kThreads) {
    int f = 0;
    for (int l = 0; l < g.nl; ++l) f |= rec[((long)l * g.nt + t) * kRecWords + 10];
    flagged += f ? 1.0 : 0.0;
  }
  flagged = block_sum(flagged, s_w);
  if (tid == 0) {
    status[0] = (int)flagged;
    out[0] = lxy;
    out[1] = lwh;
    out[2] = lconf;
    out[3] = lcls;
    out[4] = ((lxy + lwh) + lconf) + lcls;                                     // :155
  }
}

// ---------------------------------------------------------------------------------------------------
// the gradient of compute_loss with respect to p
__device__ __forceinline__ float sigmoid_f32(float x) { return __fdiv_rn(1.f, 1.f + expf(-x)); }

__global__ __launch_bounds__(kThreads) void loss_grad_dense_kernel(const Geom g, const GradGeom gg, const Heads hd, const Grads gr,
                                                                   const uint8_t* __restrict__ tconf, float gain_conf,
                                                                   const float* __restrict__ grad_loss) {
  const int wg = blockIdx.x;
  int l = 0;
#pragma unroll
  for (int i = 1; i < kMaxLayers; ++i) l = (i < g.nl && wg >= gg.wg_first[i]) ? i : l;
  const int rows = pick(g.rows, l);
  const unsigned no = (unsigned)g.nc + 5u;
  const unsigned n = (unsigned)rows * no;                                      // < 2^31 (loss_geometry)
  const float* __restrict__ pl = pick(hd.p, l);
  float* __restrict__ gl = pick(gr.g, l);
  const uint8_t* __restrict__ tc = tconf + pick(g.tconf_off, l);
  const float coef = __fdiv_rn(grad_loss[0] * gain_conf, (float)rows);         // BCEWithLogits' mean over the rows, :154
  const unsigned e0 = (unsigned)(wg - pick(gg.wg_first, l)) * (unsigned)kGradChunk + threadIdx.x * 4u;
  unsigned row = e0 / no, w = e0 - row * no;                                   // the first word of this thread's first piece
  float x[kGradVecs];
  uint8_t t[kGradVecs];                                                        // (raw: converting here would wait for each load in turn)
  int k[kGradVecs];                                                            // where in the piece word 4 sits, or -1
#pragma unroll
  for (int u = 0; u < kGradVecs; ++u) {                                        // the loads of all pieces first
    const bool has = e0 + (unsigned)(u * kGradStep) < n && w >= 1u && w <= 4u; // (row < rows then, and row * no + 4 < n)
    k[u] = has ? 4 - (int)w : -1;
    x[u] = 0.f;
    t[u] = 0;
    if (has) {
      x[u] = pl[(size_t)row * no + 4];
      t[u] = tc[row];
    }
    row += gg.step_rows;
    w += gg.step_words;
    if (w >= no) {
      w -= no;
      ++row;
    }
  }
#pragma unroll
  for (int u = 0; u < kGradVecs; ++u) {
    const unsigned e = e0 + (unsigned)(u * kGradStep);
    const float v = coef * (sigmoid_f32(x[u]) - (t[u] ? 1.f : 0.f));
    const float4 o = make_float4(k[u] == 0 ? v : 0.f, k[u] == 1 ? v : 0.f, k[u] == 2 ? v : 0.f, k[u] == 3 ? v : 0.f);
    if (e + 4u <= n) {
      *reinterpret_cast<float4*>(gl + e) = o;                                  // (gl is 16-byte aligned: yolo_loss_bwd checks)
    } else {                                                                   // the last 1-3 floats of a layer
      if (e < n) gl[e] = o.x;
      if (e + 1u < n) gl[e + 1u] = o.y;
      if (e + 2u < n) gl[e + 2u] = o.z;
    }
  }
}

// one wave64 per (layer, target) record; every branch on the record, the slot or a ballot is wave-uniform
__global__ __launch_bounds__(kThreads) void loss_grad_cells_kernel(const Geom g, const Heads hd, const Grads gr,
                                                                   const int32_t* __restrict__ rec,
                                                                   const float* __restrict__ class_weight, const Gains gains,
                                                                   const float* __restrict__ grad_loss) {
  const int lane = threadIdx.x & (YOLO_WAVE - 1);
  const int slot = blockIdx.x * kWaves + (int)(threadIdx.x / YOLO_WAVE);
  if (slot >= g.nl * g.nt) return;
  const int l = slot / g.nt, t = slot - l * g.nt;
  const int32_t* __restrict__ rl = rec + (long)l * g.nt * kRecWords;           // the records of this layer
  const int32_t* r = rl + (long)t * kRecWords;
  if (!r[0]) return;
  const int b = r[1], a = r[2], gj = r[3], gi = r[4];
  const bool weighted = g.nc > 1 && class_weight != nullptr;
  // the layer's valid records: how many, the sum of their class weights, and whether an earlier one shares this cell
  int cnt = 0;
  double sw = 0.0;
  bool earlier = false;
  for (int u = lane; u < g.nt; u += YOLO_WAVE) {
    const int32_t* q = rl + (long)u * kRecWords;
    if (q[0]) {
      ++cnt;
      if (weighted) sw += (double)class_weight[q[5]];
      earlier |= u < t && q[1] == b && q[2] == a && q[3] == gj && q[4] == gi;
    }
  }
  if (__any(earlier)) return;                                                  // the lowest slot owns the cell
#pragma unroll
  for (int off = YOLO_WAVE / 2; off > 0; off >>= 1) {
    cnt += __shfl_down(cnt, off);
    sw += __shfl_down(sw, off);
  }
  const float nf = (float)__shfl(cnt, 0);
  const float den = weighted ? (float)__shfl(sw, 0) : nf;                      // CrossEntropyLoss(weight=) divides by the weights' sum
  const float G = grad_loss[0];
  const float cxy = __fdiv_rn(G * gains.xy, nf), cwh = __fdiv_rn(G * gains.wh, nf);     // MSELoss: 2 d / (2 n), :146-147
  const float ccls = __fdiv_rn(G * gains.cls, g.nc > 1 ? den : nf);
  const int na = pick(g.na, l), ny = pick(g.ny, l), nx = pick(g.nx, l);
  const int no = g.nc + 5;
  const long cell = ((((long)b * na + a) * ny + gj) * nx + gi) * no;
  const float* __restrict__ pi = pick(hd.p, l) + cell;
  float* __restrict__ go = pick(gr.g, l) + cell;
  float m = 0.f, sef = 1.f;
  if (g.nc > 1) {                                                              // the softmax of the row, as loss_terms forms it
    m = -INFINITY;
    for (int c = lane; c < g.nc; c += YOLO_WAVE) m = fmaxf(m, pi[5 + c]);
#pragma unroll
    for (int off = YOLO_WAVE / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    double se = 0.0;
    for (int c = lane; c < g.nc; c += YOLO_WAVE) se += (double)expf(pi[5 + c] - m);
#pragma unroll
    for (int off = YOLO_WAVE / 2; off > 0; off >>= 1) se += __shfl_down(se, off);
    sef = (float)__shfl(se, 0);
  }
  for (int w0 = 0; w0 < no; w0 += YOLO_WAVE) {
    const int w = w0 + lane;
    const bool live = w < no && w != 4;
    const float x = live ? pi[w] : 0.f;
    const float sg = sigmoid_f32(x);
    const float dsg = sg * (1.f - sg);
    const float sm = __fdiv_rn(expf(x - m), sef);
    double acc = 0.0;
    for (int u0 = 0; u0 < g.nt; u0 += YOLO_WAVE) {
      const int u = u0 + lane;
      bool same = false;
      if (u < g.nt) {
        const int32_t* q = rl + (long)u * kRecWords;
        same = q[0] && q[1] == b && q[2] == a && q[3] == gj && q[4] == gi;
      }
      unsigned long long sharers = __ballot(same);
      while (sharers) {                                                        // in slot order
        const int32_t* q = rl + (long)(u0 + __ffsll(sharers) - 1) * kRecWords;
        sharers &= sharers - 1;
        if (live) {
          float c;
          if (w < 2) {
            c = cxy * ((sg - __int_as_float(q[6 + w])) * dsg);
          } else if (w < 4) {
            c = cwh * (x - __int_as_float(q[6 + w]));
          } else if (g.nc > 1) {
            const float wc = weighted ? class_weight[q[5]] : 1.f;
            c = ccls * (wc * (sm - (w - 5 == q[5] ? 1.f : 0.f)));
          } else {
            c = ccls * (sg - (float)q[5]);                                     // BCEWithLogits on the class INDEX, :152
          }
          acc += (double)c;
        }
      }
    }
    if (live) go[w] = (float)acc;
  }
}

// ---------------------------------------------------------------------------------------------------
// argument checks shared by the entry points; fills g (anchors only when anchor_vec is given)
int loss_geometry(const char* who, int nl, const int32_t* na, const int32_t* ny, const int32_t* nx, const float* anchor_vec, int bs,
                  int nc, int nt, Geom* g) {
  YOLO_REQUIRE(na && ny && nx, "%s: null geometry array", who);
  YOLO_REQUIRE(nl >= 1 && nl <= kMaxLayers, "%s: %d YOLO layers not in [1, %d]", who, nl, kMaxLayers);
  YOLO_REQUIRE(bs > 0 && nc > 0, "%s: bad batch size %d / class count %d", who, bs, nc);
  YOLO_REQUIRE(nt >= 0, "%s: negative target count %d", who, nt);
  YOLO_REQUIRE((long)nt * nl < (1l << 30), "%s: %d targets unsupported", who, nt);
  *g = Geom{};
  g->nl = nl;
  g->bs = bs;
  g->nc = nc;
  g->nt = nt;
  long off = 0;
  int wg = 0, k = 0;
  for (int l = 0; l < nl; ++l) {
    YOLO_REQUIRE(na[l] >= 1 && na[l] <= kMaxAnchors, "%s: layer %d has %d anchors, not in [1, %d]", who, l, na[l], kMaxAnchors);
    YOLO_REQUIRE(ny[l] >= 1 && nx[l] >= 1, "%s: layer %d has a %d x %d grid", who, l, ny[l], nx[l]);
    const long rows = (long)bs * na[l] * ny[l] * nx[l];
    YOLO_REQUIRE(rows * (nc + 5) < (1l << 31), "%s: layer %d holds %ld rows of %d floats: more than 2^31 elements", who, l, rows, nc + 5);
    g->na[l] = na[l];
    g->ny[l] = ny[l];
    g->nx[l] = nx[l];
    g->rows[l] = (int)rows;
    g->wg_first[l] = wg;
    g->tconf_off[l] = off;
    wg += (int)((rows + kConfRows - 1) / kConfRows);
    off += (long)align256((size_t)rows);
    for (int a = 0; a < na[l]; ++a, ++k) {
      g->anchors[l][a][0] = anchor_vec ? anchor_vec[2 * k] : 1.f;
      g->anchors[l][a][1] = anchor_vec ? anchor_vec[2 * k + 1] : 1.f;
    }
  }
  for (int l = nl; l <= kMaxLayers; ++l) g->wg_first[l] = wg;
  return 0;
}

int launch_targets(const Geom& g, const Carved& c, const float* targets, float iou_thresh, hipStream_t st) {
  hipError_t e = hipMemsetAsync(c.tconf, 0, c.tconf_bytes, st);
  if (e != hipSuccess) return yolo_set_error((int)e, "loss: memset: %s", hipGetErrorString(e));
  if (g.nt == 0) return 0;                                   // (no launch with an empty grid)
  const unsigned blocks = (unsigned)(((long)g.nl * g.nt + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(loss_assign_kernel, dim3(blocks), dim3(kThreads), 0, st, g, targets, iou_thresh, c.rec, c.tconf);
  return yolo_check_launch("yolo_build_targets_fwd");
}

}  // namespace

extern "C" size_t yolo_loss_workspace_bytes(int nl, const int32_t* na, const int32_t* ny, const int32_t* nx, int bs, int nt) {
  Geom g;
  if (loss_geometry("loss_workspace_bytes", nl, na, ny, nx, nullptr, bs, 1, nt, &g)) return 0;
  return carve(nullptr, g).bytes;
}

extern "C" int yolo_build_targets_fwd(const float* targets, int nt, int nl, const int32_t* na, const int32_t* ny, const int32_t* nx,
                                      const float* anchor_vec, int bs, int nc, float iou_thresh, void* workspace,
                                      size_t workspace_bytes, yolo_stream_t s) {
  YOLO_REQUIRE(workspace && anchor_vec && (targets || nt == 0), "build_targets: null pointer");
  Geom g;
  if (int rc = loss_geometry("build_targets", nl, na, ny, nx, anchor_vec, bs, nc, nt, &g)) return rc;
  const Carved c = carve(workspace, g);
  if (workspace_bytes < c.bytes) return yolo_set_error(YOLO_E_WORKSPACE, "build_targets: workspace %zu < %zu bytes", workspace_bytes, c.bytes);
  return launch_targets(g, c, targets, iou_thresh, (hipStream_t)s);
}

extern "C" int yolo_loss_fwd(const float* const* p, const float* targets, int nt, int nl, const int32_t* na, const int32_t* ny,
                             const int32_t* nx, const float* anchor_vec, int bs, int nc, float iou_thresh, const float* gains,
                             const float* class_weight, void* workspace, size_t workspace_bytes, float* out, int32_t* status,
                             yolo_stream_t s) {
  YOLO_REQUIRE(p && workspace && anchor_vec && gains && out && status && (targets || nt == 0), "loss: null pointer");
  Geom g;
  if (int rc = loss_geometry("loss", nl, na, ny, nx, anchor_vec, bs, nc, nt, &g)) return rc;
  Heads hd{};
  for (int l = 0; l < nl; ++l) {
    YOLO_REQUIRE(p[l], "loss: null head tensor of layer %d", l);
    hd.p[l] = p[l];
  }
  const Carved c = carve(workspace, g);
  if (workspace_bytes < c.bytes) return yolo_set_error(YOLO_E_WORKSPACE, "loss: workspace %zu < %zu bytes", workspace_bytes, c.bytes);
  hipStream_t st = (hipStream_t)s;
  if (int rc = launch_targets(g, c, targets, iou_thresh, st)) return rc;
  hipLaunchKernelGGL(loss_conf_kernel, dim3((unsigned)g.wg_first[nl]), dim3(kThreads), 0, st, g, hd, c.tconf, c.partials);
  if (int rc = yolo_check_launch("yolo_loss_fwd(conf)")) return rc;
  if (nt > 0) {
    const unsigned blocks = (unsigned)(((long)nl * nt + kWaves - 1) / kWaves);
    hipLaunchKernelGGL(loss_terms_kernel, dim3(blocks), dim3(kThreads), 0, st, g, hd, c.rec, class_weight, c.terms);
    if (int rc = yolo_check_launch("yolo_loss_fwd(terms)")) return rc;
  }
  const Gains gn{gains[0], gains[1], gains[2], gains[3]};
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(kThreads), 0, st, g, c.rec, c.partials, c.terms, gn, out, status);
  return yolo_check_launch("yolo_loss_fwd(finish)");
}

extern "C" int yolo_loss_bwd(const float* const* p, const float* targets, int nt, int nl, const int32_t* na, const int32_t* ny,
                             const int32_t* nx, const float* anchor_vec, int bs, int nc, float iou_thresh, const float* gains,
                             const float* class_weight, void* workspace, size_t workspace_bytes, const float* grad_loss,
                             float* const* grad_p, yolo_stream_t s) {
  YOLO_REQUIRE(p && workspace && anchor_vec && gains && (targets || nt == 0), "loss_bwd: null pointer");
  YOLO_REQUIRE(grad_loss, "loss_bwd: null grad_loss");
  YOLO_REQUIRE(grad_p, "loss_bwd: null grad_p");
  Geom g;
  if (int rc = loss_geometry("loss_bwd", nl, na, ny, nx, anchor_vec, bs, nc, nt, &g)) return rc;
  Heads hd{};
  Grads gr{};
  GradGeom gg{};
  const long no = nc + 5;
  int wg = 0;
  for (int l = 0; l < nl; ++l) {
    YOLO_REQUIRE(p[l], "loss_bwd: null head tensor of layer %d", l);
    YOLO_REQUIRE(grad_p[l], "loss_bwd: null gradient tensor of layer %d", l);
    YOLO_REQUIRE(((uintptr_t)grad_p[l] & 15) == 0, "loss_bwd: the gradient tensor of layer %d is not 16-byte aligned", l);
    hd.p[l] = p[l];
    gr.g[l] = grad_p[l];
    gg.wg_first[l] = wg;
    wg += (int)((g.rows[l] * no + kGradChunk - 1) / kGradChunk);
  }
  for (int l = nl; l <= kMaxLayers; ++l) gg.wg_first[l] = wg;
  gg.step_rows = (unsigned)(kGradStep / no);
  gg.step_words = (unsigned)(kGradStep % no);
  const Carved c = carve(workspace, g);
  if (workspace_bytes < c.bytes) return yolo_set_error(YOLO_E_WORKSPACE, "loss_bwd: workspace %zu < %zu bytes", workspace_bytes, c.bytes);
  hipStream_t st = (hipStream_t)s;
  if (int rc = launch_targets(g, c, targets, iou_thresh, st)) return rc;
  hipLaunchKernelGGL(loss_grad_dense_kernel, dim3((unsigned)wg), dim3(kThreads), 0, st, g, gg, hd, gr, c.tconf, gains[3], grad_loss);
  if (int rc = yolo_check_launch("yolo_loss_bwd(dense)")) return rc;
  if (nt > 0) {
    const Gains gn{gains[0], gains[1], gains[2], gains[3]};
    const unsigned blocks = (unsigned)(((long)nl * nt + kWaves - 1) / kWaves);
    hipLaunchKernelGGL(loss_grad_cells_kernel, dim3(blocks), dim3(kThreads), 0, st, g, hd, gr, c.rec, class_weight, gn, grad_loss);
    if (int rc = yolo_check_launch("yolo_loss_bwd(cells)")) return rc;
  }
  return 0;
}
