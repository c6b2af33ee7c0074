// COCO bbox evaluation on the device for gfx950: the IoU / matching of COCOeval.evaluateImg, the precision / recall sweep of
// COCOeval.accumulate and the per-group sums of the reference's "Mean IOU" (reference utils/utils.py:330-354 calls pycocotools).
//
// Arithmetic contract
//   * every value - box, area, IoU, recall, precision - is float64; this file is compiled with -ffp-contract=off and divides with
//     __ddiv_rn, so each step is ONE IEEE operation in the order of maskApi's bbIou / COCOeval and the results can be compared bit
//     for bit with a numpy restatement;
//   * the parameters (iouThrs, areaRng, recThrs) are read from device arrays the caller filled from numpy, never recomputed here;
//     their COUNTS are fixed: 10 IoU thresholds, 4 area ranges, 101 recall thresholds, 3 maxDets;
//   * counts (true / false positives, non-ignored GTs) are integers: scans and integer atomics, exact in any order;
//   * the one floating-point sum (IoU entries >= 0.3 of a group's D x G matrix) is formed in an order fixed by the shapes:
//     lane-strided over g, sequential over d, then a shuffle tree across the wave64.  Bit-identical from run to run.
//
// Launches (caller's stream, nothing synchronises with the host)
//   memset        npig [K, 4] and status [1]
//   coco_match    one wave64 per (image, category) group.  The lanes flag the GTs (bit a = ignored in area range a, bit 4 = crowd)
//                 and count the non-ignored ones into npig.  Then per detection d, in evaluation order: the lanes write the IoU
//                 row of d into LDS, lanes 0..39 run one (area range, IoU threshold) scan each over it - their matched-GT bit sets
//                 live in LDS -, and two ballots pack the 40 matched / ignore bits of d (bit a * 10 + t).  Matched flags are
//                 kept by GT slot, not by annotation id (pycocotools loses a match to a GT whose id is 0: the one deviation).
//                 A group with more than kMaxGt GTs is NOT evaluated: it is counted in status[0] and the caller raises
//   coco_sweep    one workgroup per (category, area range, maxDets, IoU threshold) over the category's detections in sweep order
//                 (descending score, stable; the caller's permutation), kChunk at a time.  Pass 1 counts tp / fp / entries.
//                 Pass 2 walks the chunks from the right: block scans rebuild the cumulative tp / fp of the chunk from the totals,
//                 a running maximum from the right makes the precision monotone, and an element at which the recall first reaches
//                 recThrs[r] - only true-positive steps and the first entry can - stores precision[r].  Nothing is kept per
//                 sweep outside LDS: the workspace (the in-group rank of each detection) is linear in nD.
#include "common.h"

namespace {

constexpr int kT = 10, kA = 4, kM = 3, kR = 101;
constexpr int kPairs = kA * kT;          // (area range, threshold) scans of a group: lanes 0..39
constexpr int kMaxGt = 1024;             // GTs of one (image, category) group (LDS: 8 KiB IoU row, 5 KiB bit sets, 1 KiB flags)
constexpr int kWords = kMaxGt / 32;
constexpr int kChunk = 256;              // detections of one sweep step = threads of a coco_sweep workgroup
constexpr int kWaves = kChunk / YOLO_WAVE;
constexpr int kCrowdBit = 16;

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t coco_ws_bytes(int n_dt) { return align256((size_t)(n_dt > 0 ? n_dt : 1) * 4); }

// maskApi bbIou for one pair; boxes are (x, y, w, h)
__device__ __forceinline__ double bb_iou(double dx, double dy, double dw, double dh, double gx, double gy, double gw, double gh,
                                         bool crowd) {
  const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
  const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
  if (w <= 0.0 || h <= 0.0) return 0.0;
  const double i = w * h;
  const double da = dw * dh;
  const double u = crowd ? da : (da + gw * gh) - i;
  return __ddiv_rn(i, u);
}

// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(YOLO_WAVE) void coco_match_kernel(const double* __restrict__ dt_box, const int32_t* __restrict__ dt_off,
                                                               const double* __restrict__ gt_box, const double* __restrict__ gt_area,
                                                               const uint8_t* __restrict__ gt_crowd, const int32_t* __restrict__ gt_off,
                                                               int n_cat, const double* __restrict__ iou_thrs,
                                                               const double* __restrict__ area_rng,
                                                               unsigned long long* __restrict__ dt_match,
                                                               unsigned long long* __restrict__ dt_ignore, int32_t* __restrict__ dt_rank,
                                                               int32_t* __restrict__ npig, double* __restrict__ iou_sum,
                                                               int32_t* __restrict__ iou_cnt, int32_t* __restrict__ status) {
  __shared__ double s_row[kMaxGt];
  __shared__ uint32_t s_bits[kWords * kPairs];             // word w of scan p at [w * kPairs + p]
  __shared__ uint8_t s_flag[kMaxGt];
  const int grp = blockIdx.x, lane = threadIdx.x;
  const int d0 = dt_off[grp], D = dt_off[grp + 1] - d0;
  const int g0 = gt_off[grp], G = gt_off[grp + 1] - g0;
  if (G > kMaxGt) {                                        // (wave-uniform) never truncated: reported
    if (lane == 0) {
      atomicAdd(&status[0], 1);
      iou_sum[grp] = 0.0;
      iou_cnt[grp] = 0;
    }
    return;
  }
  const int k = grp % n_cat;
  const bool scan = lane < kPairs;
  const int a = scan ? lane / kT : 0, t = scan ? lane - a * kT : 0;
  const double a0 = area_rng[2 * a], a1 = area_rng[2 * a + 1];
  const double thr = fmin(iou_thrs[t], 1.0 - 1e-10);

  // GT flags and npig
  int cnt[kA] = {0, 0, 0, 0};
  for (int g = lane; g < G; g += YOLO_WAVE) {
    const double area = gt_area[g0 + g];
    const bool crowd = gt_crowd[g0 + g] != 0;
    int f = crowd ? kCrowdBit : 0;
#pragma unroll
    for (int r = 0; r < kA; ++r) {
      const bool ig = crowd || area < area_rng[2 * r] || area > area_rng[2 * r + 1];
      f |= ig ? (1 << r) : 0;
      cnt[r] += ig ? 0 : 1;
    }
    s_flag[g] = (uint8_t)f;
  }
  if (G > 0) {
#pragma unroll
    for (int r = 0; r < kA; ++r) {
      int c = cnt[r];
#pragma unroll
      for (int off = YOLO_WAVE / 2; off > 0; off >>= 1) c += __shfl_down(c, off);
      if (lane == 0 && c) atomicAdd(&npig[k * kA + r], c);
    }
  }
  const int words = (G + 31) >> 5;
  if (scan)
    for (int w = 0; w < words; ++w) s_bits[w * kPairs + lane] = 0u;
  __syncthreads();

  double sum = 0.0;
  int n03 = 0;
  for (int d = 0; d < D; ++d) {
    const double* db = dt_box + (long)(d0 + d) * 4;
    const double dx = db[0], dy = db[1], dw = db[2], dh = db[3];
    for (int g = lane; g < G; g += YOLO_WAVE) {
      const double* gb = gt_box + (long)(g0 + g) * 4;
      const double v = bb_iou(dx, dy, dw, dh, gb[0], gb[1], gb[2], gb[3], (s_flag[g] & kCrowdBit) != 0);
      s_row[g] = v;
      if (v >= 0.3) {                                      // reference utils.py:342
        sum += v;
        n03 += 1;
      }
    }
    __syncthreads();
    bool mt = false, ig = false;
    if (scan) {
      int m = -1;
      double best = thr;
      for (int pass = 0; pass < 2; ++pass) {               // the non-ignored GTs, then the ignored ones: pycocotools' stable sort
        if (pass == 1 && m >= 0) break;                    // m names a non-ignored GT: stop at the first ignored one
        for (int g = 0; g < G; ++g) {
          const int f = s_flag[g];
          if (((f >> a) & 1) != pass) continue;
          if ((s_bits[(g >> 5) * kPairs + lane] >> (g & 31) & 1u) && !(f & kCrowdBit)) continue;
          const double v = s_row[g];
          if (v < best) continue;
          best = v;                                        // an equal IoU replaces the earlier match
          m = g;
        }
      }
      if (m >= 0) {
        s_bits[(m >> 5) * kPairs + lane] |= 1u << (m & 31);
        mt = true;
        ig = ((s_flag[m] >> a) & 1) != 0;
      } else {
        const double da = dw * dh;
        ig = da < a0 || da > a1;
      }
    }
    const unsigned long long mbits = __ballot(mt), ibits = __ballot(ig);
    if (lane == 0) {
      dt_match[d0 + d] = mbits;
      dt_ignore[d0 + d] = ibits;
      dt_rank[d0 + d] = d;
    }
    __syncthreads();                                       // (the row is rewritten by the next detection)
  }
#pragma unroll
  for (int off = YOLO_WAVE / 2; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off);
    n03 += __shfl_down(n03, off);
  }
  if (lane == 0) {
    iou_sum[grp] = sum;
    iou_cnt[grp] = n03;
  }
}

// ---------------------------------------------------------------------------------------------------
struct Cnt {
  int tp, fp, nv;
};
struct MaxDets {
  int m[kM];
};

// inclusive scan over the workgroup in thread order; *total = the workgroup's sum
__device__ __forceinline__ Cnt block_scan(Cnt v, int* s_w, Cnt* total) {
  const int lane = threadIdx.x & (YOLO_WAVE - 1), wave = threadIdx.x / YOLO_WAVE;
#pragma unroll
  for (int off = 1; off < YOLO_WAVE; off <<= 1) {
    const int x = __shfl_up(v.tp, off), y = __shfl_up(v.fp, off), z = __shfl_up(v.nv, off);
    if (lane >= off) {
      v.tp += x;
      v.fp += y;
      v.nv += z;
    }
  }
  __syncthreads();                                         // (s_w of the previous call has been read by everyone)
  if (lane == YOLO_WAVE - 1) {
    s_w[wave * 3 + 0] = v.tp;
    s_w[wave * 3 + 1] = v.fp;
    s_w[wave * 3 + 2] = v.nv;
  }
  __syncthreads();
  Cnt tot{0, 0, 0};
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int x = s_w[w * 3 + 0], y = s_w[w * 3 + 1], z = s_w[w * 3 + 2];
    if (w < wave) {
      v.tp += x;
      v.fp += y;
      v.nv += z;
    }
    tot.tp += x;
    tot.fp += y;
    tot.nv += z;
  }
  *total = tot;
  return v;
}

// maximum over this thread and every thread to its right; *all = the workgroup's maximum
__device__ __forceinline__ double block_max_from_right(double v, double* s_m, double* all) {
  const int lane = threadIdx.x & (YOLO_WAVE - 1), wave = threadIdx.x / YOLO_WAVE;
#pragma unroll
  for (int off = 1; off < YOLO_WAVE; off <<= 1) {
    const double x = __shfl_down(v, off);
    if (lane + off < YOLO_WAVE) v = fmax(v, x);
  }
  __syncthreads();
  if (lane == 0) s_m[wave] = v;
  __syncthreads();
  double top = s_m[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    const double x = s_m[w];
    if (w > wave) v = fmax(v, x);
    top = fmax(top, x);
  }
  *all = top;
  return v;
}

__global__ __launch_bounds__(kChunk) void coco_sweep_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ cat_off,
                                                            int n_cat, const unsigned long long* __restrict__ dt_match,
                                                            const unsigned long long* __restrict__ dt_ignore,
                                                            const int32_t* __restrict__ dt_rank, const int32_t* __restrict__ npig,
                                                            const double* __restrict__ rec_thrs, const MaxDets md, double eps,
                                                            double* __restrict__ precision, double* __restrict__ recall) {
  __shared__ double s_thr[kR], s_q[kR], s_m[kWaves];
  __shared__ int s_w[kWaves * 3];
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int t = b % kT;
  b /= kT;
  const int mi = b % kM;
  b /= kM;
  const int a = b % kA;
  const int k = b / kA;
  const int max_det = mi == 0 ? md.m[0] : (mi == 1 ? md.m[1] : md.m[2]);
  const int bit = a * kT + t;
  const int np = npig[k * kA + a];
  const long p_base = ((long)t * kR * n_cat + k) * (kA * kM) + a * kM + mi;      // precision[t, r, k, a, m]: + r * n_cat * kA * kM
  const long p_step = (long)n_cat * (kA * kM);
  double* rc_out = recall + ((long)t * n_cat + k) * (kA * kM) + a * kM + mi;
  if (np == 0) {                                           // (workgroup-uniform) no non-ignored GT: both stay at -1
    for (int r = tid; r < kR; r += kChunk) precision[p_base + r * p_step] = -1.0;
    if (tid == 0) *rc_out = -1.0;
    return;
  }
  for (int r = tid; r < kR; r += kChunk) {
    s_thr[r] = rec_thrs[r];
    s_q[r] = 0.0;
  }
  const int j0 = cat_off[k], n = cat_off[k + 1] - j0;
  const int chunks = (n + kChunk - 1) / kChunk;
  const double npd = (double)np;

  // pass 1: the totals
  Cnt mine{0, 0, 0};
  for (int j = tid; j < n; j += kChunk) {
    const int e = order[j0 + j];
    if (dt_rank[e] < max_det) {
      const bool mt = (dt_match[e] >> bit) & 1ull, ig = (dt_ignore[e] >> bit) & 1ull;
      mine.tp += (mt && !ig) ? 1 : 0;
      mine.fp += (!mt && !ig) ? 1 : 0;
      mine.nv += 1;
    }
  }
  Cnt total;
  block_scan(mine, s_w, &total);

  // pass 2: the chunks from the right
  Cnt after{0, 0, 0};
  double carry = -1.0;                                     // every precision is >= 0
  for (int c = chunks - 1; c >= 0; --c) {
    const int j = c * kChunk + tid;
    Cnt inc{0, 0, 0};
    if (j < n) {
      const int e = order[j0 + j];
      if (dt_rank[e] < max_det) {
        const bool mt = (dt_match[e] >> bit) & 1ull, ig = (dt_ignore[e] >> bit) & 1ull;
        inc.tp = (mt && !ig) ? 1 : 0;
        inc.fp = (!mt && !ig) ? 1 : 0;
        inc.nv = 1;
      }
    }
    Cnt sum;
    Cnt cum = block_scan(inc, s_w, &sum);
    const int tp = total.tp - after.tp - sum.tp + cum.tp;  // cumulative counts up to and including this entry
    const int fp = total.fp - after.fp - sum.fp + cum.fp;
    const int nv = total.nv - after.nv - sum.nv + cum.nv;
    const double tpd = (double)tp;
    const double pr = inc.nv ? __ddiv_rn(tpd, ((double)fp + tpd) + eps) : -1.0;
    double top;
    const double pm = fmax(block_max_from_right(pr, s_m, &top), carry);
    if (inc.nv && (inc.tp || nv == 1)) {                   // the recall moves here (or this is the first entry)
      const double rc = __ddiv_rn(tpd, npd);
      const double prev = nv == 1 ? -1.0 : __ddiv_rn((double)(tp - inc.tp), npd);
      for (int r = 0; r < kR; ++r) {
        const double th = s_thr[r];
        if (prev < th && th <= rc) s_q[r] = pm;            // first entry with rc >= recThrs[r]
      }
    }
    carry = fmax(carry, top);
    after.tp += sum.tp;
    after.fp += sum.fp;
    after.nv += sum.nv;
  }
  __syncthreads();
  for (int r = tid; r < kR; r += kChunk) precision[p_base + r * p_step] = s_q[r];
  if (tid == 0) *rc_out = total.nv ? __ddiv_rn((double)total.tp, npd) : 0.0;
}

}  // namespace

extern "C" int yolo_coco_sweep_chunk(void) { return kChunk; }

extern "C" int yolo_coco_max_gt(void) { return kMaxGt; }

extern "C" size_t yolo_coco_workspace_bytes(int n_dt) {
  if (n_dt < 0) {
    yolo_set_error(YOLO_E_ARG, "coco_workspace_bytes: negative detection count %d", n_dt);
    return 0;
  }
  return coco_ws_bytes(n_dt);
}

extern "C" int yolo_coco_match_fwd(const double* dt_box, const int32_t* dt_off, int n_dt, const double* gt_box, const double* gt_area,
                                   const uint8_t* gt_crowd, const int32_t* gt_off, int n_gt, int n_img, int n_cat, int max_gt,
                                   const double* iou_thrs, const double* area_rng, uint64_t* dt_match, uint64_t* dt_ignore,
                                   int32_t* npig, double* iou_sum, int32_t* iou_cnt, int32_t* status, void* workspace,
                                   size_t workspace_bytes, yolo_stream_t s) {
  YOLO_REQUIRE(n_dt >= 0 && n_gt >= 0, "coco_match: negative count (%d detections, %d GTs)", n_dt, n_gt);
  YOLO_REQUIRE(n_img >= 1 && n_cat >= 1 && (long)n_img * n_cat < (1l << 31) - 1, "coco_match: %d images x %d categories unsupported",
               n_img, n_cat);
  YOLO_REQUIRE(dt_off && gt_off && iou_thrs && area_rng && npig && iou_sum && iou_cnt && status && workspace, "coco_match: null pointer");
  YOLO_REQUIRE((dt_box && dt_match && dt_ignore) || n_dt == 0, "coco_match: null detection array");
  YOLO_REQUIRE((gt_box && gt_area && gt_crowd) || n_gt == 0, "coco_match: null GT array");
  YOLO_REQUIRE(max_gt >= 0 && max_gt <= n_gt, "coco_match: max_gt %d not in [0, %d]", max_gt, n_gt);
  if (max_gt > kMaxGt)
    return yolo_set_error(YOLO_E_UNSUPPORTED, "coco_match: a group of %d GTs exceeds the cap of %d per (image, category)", max_gt, kMaxGt);
  if (workspace_bytes < coco_ws_bytes(n_dt))
    return yolo_set_error(YOLO_E_WORKSPACE, "coco_match: workspace %zu < %zu bytes", workspace_bytes, coco_ws_bytes(n_dt));
  hipStream_t st = (hipStream_t)s;
  hipError_t e = hipMemsetAsync(npig, 0, (size_t)n_cat * kA * 4, st);
  if (e == hipSuccess) e = hipMemsetAsync(status, 0, 4, st);
  if (e != hipSuccess) return yolo_set_error((int)e, "coco_match: memset: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)(n_img * n_cat)), dim3(YOLO_WAVE), 0, st, dt_box, dt_off, gt_box, gt_area, gt_crowd,
                     gt_off, n_cat, iou_thrs, area_rng, (unsigned long long*)dt_match, (unsigned long long*)dt_ignore,
                     (int32_t*)workspace, npig, iou_sum, iou_cnt, status);
  return yolo_check_launch("yolo_coco_match_fwd");
}

extern "C" int yolo_coco_accumulate_fwd(const int32_t* order, const int32_t* cat_off, int n_dt, int n_cat, const uint64_t* dt_match,
                                        const uint64_t* dt_ignore, const int32_t* npig, const double* rec_thrs, const int32_t* max_dets,
                                        double eps, const void* workspace, size_t workspace_bytes, double* precision, double* recall,
                                        yolo_stream_t s) {
  YOLO_REQUIRE(n_dt >= 0, "coco_accumulate: negative detection count %d", n_dt);
  YOLO_REQUIRE(n_cat >= 1 && (long)n_cat * (kA * kM * kT) < (1l << 31) - 1, "coco_accumulate: %d categories unsupported", n_cat);
  YOLO_REQUIRE(cat_off && npig && rec_thrs && max_dets && workspace && precision && recall, "coco_accumulate: null pointer");
  YOLO_REQUIRE((order && dt_match && dt_ignore) || n_dt == 0, "coco_accumulate: null detection array");
  YOLO_REQUIRE(max_dets[0] >= 0 && max_dets[0] <= max_dets[1] && max_dets[1] <= max_dets[2], "coco_accumulate: maxDets (%d, %d, %d) not ascending",
               max_dets[0], max_dets[1], max_dets[2]);
  YOLO_REQUIRE(eps > 0.0, "coco_accumulate: eps must be np.spacing(1)");
  if (workspace_bytes < coco_ws_bytes(n_dt))
    return yolo_set_error(YOLO_E_WORKSPACE, "coco_accumulate: workspace %zu < %zu bytes", workspace_bytes, coco_ws_bytes(n_dt));
  const MaxDets md{{max_dets[0], max_dets[1], max_dets[2]}};
  hipLaunchKernelGGL(coco_sweep_kernel, dim3((unsigned)(n_cat * kA * kM * kT)), dim3(kChunk), 0, (hipStream_t)s, order, cat_off, n_cat,
                     (const unsigned long long*)dt_match, (const unsigned long long*)dt_ignore, (const int32_t*)workspace, npig, rec_thrs,
                     md, eps, precision, recall);
  return yolo_check_launch("yolo_coco_accumulate_fwd");
}
