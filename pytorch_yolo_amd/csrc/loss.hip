// Validation loss on the device for gfx950: build_targets and compute_loss, FORWARD VALUE ONLY (no gradient is formed anywhere).
//
// Replaces the ATen dispatches and the Python loop of compute_loss / build_targets / wh_iou (reference utils/utils.py:99-197) on the
// raw head tensors p that `io, p = model(x)` returns in eval mode.
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
#include "common.h"

namespace {

constexpr int kMaxLayers = 4;
constexpr int kMaxAnchors = 8;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / YOLO_WAVE;
constexpr int kConfRows = 1024;      // rows of one loss_conf workgroup: four per thread
constexpr int kRecWords = 12;        // valid, b, a, gj, gi, cls, txy[2], twh[2], flagged, 0  (48 bytes)
constexpr int kTermWords = 4;        // float64 per record: xy terms, wh terms, class numerator, class denominator

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
// argument checks shared by the three entry points; fills g (anchors only when anchor_vec is given)
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
