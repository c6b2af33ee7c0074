// The weight-gradient GEMM of the conv backward, shared by conv_bwd.hip (stride 1) and conv_down_bwd.hip (the 3x3
// stride-2 downsample): wgrad_kernel<MI, STRIDE>, its second pass, the split rule and the bf16 rounding of the device
// packers.  Everything here has internal linkage: each of the two files holds its own instantiations.
#pragma once
#include "common.h"

namespace yolo_conv {
int launch_cus();   // conv_igemm.hip: compute units the coming launches may use
}

namespace {

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

__device__ __forceinline__ uint16_t dev_f32_to_bf16_rne(float f) {    // the host packer's formula, bit for bit
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x007fffffu)) return (uint16_t)((u >> 16) | 0x0040u);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// ---- wgrad ----------------------------------------------------------------------------------------------------------------
// GEMM  D[co][col] = sum_p g[p][co] * X[p][col],  col = tap * cin + ci,  X[p][col] = x[pixel p shifted by the tap][ci] or 0.
// A workgroup of 4 waves (2 x 2) owns a (64 MI) x 128 tile of D and the pixel range of its split.  Both operands are summed over
// their ROW index, so a stage of kBK pixel rows of each is staged in LDS as [pixel][128 x bf16] (256-byte rows, 16-byte chunks
// XOR-swizzled) and the MFMA fragments come from ds_read_b64_tr_b16: lane 4q+p of a 16-lane group addresses row q, columns 4p..4p+3 of
// a 4 x 16 block and receives its column (l & 15) - element j of an operand is pixel 8 (l >> 5) + j, as v_mfma_f32_32x32x16_bf16 wants.
// Out-of-range rows, channels and taps are zeroed BY INDEX at the load; nothing outside an operand is read.
// STRIDE 1: p runs over the n h w pixels of the map x and g share, and the x row of (p, tap) is p shifted by the tap.
// STRIDE 2: p runs over the n ho wo OUTPUT pixels (the rows of g), and the x row of pixel (nn, oh, ow) and tap (kh, kw) is input pixel
// (nn, 2 oh + kh - pad, 2 ow + kw - pad); (nn, oh, ow) is stepped over the output map like (oh, ow) at stride 1.
constexpr int kBK = 64;          // pixels per stage
constexpr int kStages = 1;       // stages of global loads in flight (in registers) over the MFMAs
constexpr int kTN = 128;         // columns of D per workgroup
constexpr int kRows = kBK / 16;  // rows of a stage one thread loads (of each operand)
constexpr int kMinSteps = 8;     // a split is worth a workgroup from 512 pixels on

__device__ __forceinline__ int lds_off(int row, int ch) {   // byte offset of 16-byte chunk ch (0..15) of row `row`
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

struct WgradArgs {
  const bf16_t* x;
  const bf16_t* g;
  float* ws;        // [splits][cout][ncol]
  float* ws_db;     // [splits][cout] or null
  int n, h, w, cin, x_total, x_offset, cout, cg, ksize, pad, ncol;
  long pixels;
  int steps_per_split;
  int step_h, step_w;   // 16 pixels further in (oh, ow): (16 / w) % h rows and 16 % w columns (of the map the pixels run over)
  int ho, wo, step_n;   // STRIDE 2 only: the output map, and the 16 / (ho wo) images 16 pixels skip
};

template <int MI, int STRIDE>
__global__ __launch_bounds__(256, 2) void wgrad_kernel(const WgradArgs a) {      // two waves per SIMD: <= 256 registers
  static_assert(STRIDE == 1 || STRIDE == 2, "wgrad_kernel: stride 1 or 2");
  constexpr int TM = 64 * MI;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kBK * 256];
  unsigned char* const lg = lds;                 // g stage  [kBK][128 co]
  unsigned char* const lx = lds + kBK * 256;     // x stage  [kBK][128 col]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int col0 = blockIdx.x * kTN, co0 = blockIdx.y * TM, split = blockIdx.z;
  const long p_begin = (long)split * a.steps_per_split * kBK;
  long p_end = p_begin + (long)a.steps_per_split * kBK;
  if (p_end > a.pixels) p_end = a.pixels;
  const bool want_db = a.ws_db != nullptr && blockIdx.x == 0;
  const int mh = STRIDE == 1 ? a.h : a.ho, mw = STRIDE == 1 ? a.w : a.wo;      // the map the pixels run over

  // what this thread stages: chunk `ch` of rows lr, lr + 16, ... of both operands
  const int ch = tid & 15, lr = tid >> 4;
  const int gco = co0 + ch * 8;
  const bool g_ok = ch * 8 < TM && gco < a.cg;
  const int col = col0 + ch * 8;
  const bool x_ok = col < a.ncol;
  const int tap = x_ok ? col / a.cin : 0;
  const int ci = col - tap * a.cin;
  const int dh = tap / a.ksize - a.pad, dw = tap % a.ksize - a.pad;
  const long x_shift = ((long)dh * a.w + dw) * a.x_total + a.x_offset + ci;      // STRIDE 1: from pixel p of x to its tap
  const int x_chan = a.x_offset + ci;                                            // STRIDE 2
  // the rows this thread loads are p_begin + lr + 16 j, j = 0, 1, ... across the stages: (oh, ow) is divided out once and stepped
  const int rem0 = (int)((p_begin + lr) % (mh * mw));
  int oh = rem0 / mw, ow = rem0 - oh * mw;
  [[maybe_unused]] int nn = (int)((p_begin + lr) / (mh * mw));                   // STRIDE 2: the image

  // One stage of this thread's loads.  Every load is issued unconditionally - from the operand's first 16 bytes where the index
  // says "zero" - and `ok` (bit i: row i of g, bit 8 + i: row i of x) selects when the stage is written to LDS: no branch between the
  // loads, so kStages stages can be in flight.
  struct Stage {
    u32x4 g[kRows], x[kRows];
    unsigned ok;
  };
  auto fetch = [&](Stage& st, long pbase) {
    st.ok = 0;
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      const long p = pbase + lr + 16 * i;
      const bool in = p < p_end;
      const bool gv = in && g_ok;
      if constexpr (STRIDE == 1) {
        const bool xv = in && x_ok && (unsigned)(oh + dh) < (unsigned)a.h && (unsigned)(ow + dw) < (unsigned)a.w;
        st.g[i] = *reinterpret_cast<const u32x4*>(gv ? a.g + p * a.cg + gco : a.g);
        st.x[i] = *reinterpret_cast<const u32x4*>(xv ? a.x + p * a.x_total + x_shift : a.x + a.x_offset);
        st.ok |= (gv ? 1u : 0u) << i | (xv ? 1u : 0u) << (8 + i);
        ow += a.step_w;
        oh += a.step_h;
        if (ow >= a.w) ow -= a.w, ++oh;
        if (oh >= a.h) oh -= a.h;
      } else {
        const int ih = 2 * oh + dh, iw = 2 * ow + dw;
        const bool xv = in && x_ok && (unsigned)ih < (unsigned)a.h && (unsigned)iw < (unsigned)a.w;
        st.g[i] = *reinterpret_cast<const u32x4*>(gv ? a.g + p * a.cg + gco : a.g);
        st.x[i] = *reinterpret_cast<const u32x4*>(xv ? a.x + (((long)nn * a.h + ih) * a.w + iw) * a.x_total + x_chan : a.x + a.x_offset);
        st.ok |= (gv ? 1u : 0u) << i | (xv ? 1u : 0u) << (8 + i);
        ow += a.step_w;
        oh += a.step_h;
        if (ow >= a.wo) ow -= a.wo, ++oh;
        if (oh >= a.ho) oh -= a.ho, ++nn;
        nn += a.step_n;
      }
    }
  };

  f32x16 acc[MI][2];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float dbv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) dbv[j] = 0.f;

  // transposed-read addresses of this lane: block rows 8 (l >> 5) + 4 t + q, block columns 16 ((l >> 4) & 1) + 4 p
  const int q = (lane & 15) >> 2, pp = lane & 3, khalf = lane >> 5, chalf = (lane >> 4) & 1;
  // (16 rows further down the swizzle repeats: k step ks adds the constant 16 * 256 * ks)
  int a_off[MI][2], b_off[2][2];     // [sub-tile][t]
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int row = 8 * khalf + 4 * t + q;
#pragma unroll
    for (int i = 0; i < MI; ++i) a_off[i][t] = lds_off(row, (wm * 32 * MI + 32 * i + 16 * chalf) / 8 + (pp >> 1)) + 8 * (pp & 1);
#pragma unroll
    for (int j = 0; j < 2; ++j) b_off[j][t] = lds_off(row, (wn * 64 + 32 * j + 16 * chalf) / 8 + (pp >> 1)) + 8 * (pp & 1);
  }

  // write a fetched stage to LDS (and add its g rows to db), then - behind the barrier - refill it kStages stages ahead and run the MFMAs
  auto stage = [&](Stage& st, long pnext) {
    const u32x4 zero = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      const u32x4 vg = (st.ok >> i) & 1u ? st.g[i] : zero, vx = (st.ok >> (8 + i)) & 1u ? st.x[i] : zero;
      *reinterpret_cast<u32x4*>(lg + lds_off(lr + 16 * i, ch)) = vg;
      *reinterpret_cast<u32x4*>(lx + lds_off(lr + 16 * i, ch)) = vx;
      if (want_db) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dbv[2 * j] += bf16_bits_to_f32(vg[j] & 0xffffu);
          dbv[2 * j + 1] += bf16_bits_to_f32(vg[j] >> 16);
        }
      }
    }
    __syncthreads();
    fetch(st, pnext);          // global loads fly under kStages stages of MFMAs (nothing is selected past p_end)
#pragma unroll
    for (int ks = 0; ks < kBK / 16; ++ks) {
      bf16x8 af[MI], bf[2];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(lg + a_off[i][0] + 4096 * ks));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(lg + a_off[i][1] + 4096 * ks));
        af[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(lx + b_off[j][0] + 4096 * ks));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(lx + b_off[j][1] + 4096 * ks));
        bf[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  };
  Stage st[kStages];
#pragma unroll
  for (int i = 0; i < kStages; ++i) fetch(st[i], p_begin + i * kBK);
  for (long pbase = p_begin; pbase < p_end;) {      // the fetches stay in stage order: (oh, ow) steps with them
#pragma unroll
    for (int i = 0; i < kStages; ++i) {
      if (pbase < p_end) stage(st[i], pbase + kStages * kBK);      // uniform
      pbase += kBK;
    }
  }

  // partial tile -> workspace: D row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5), D column = lane & 31
  float* const wsp = a.ws + (size_t)split * a.cout * a.ncol;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = col0 + wn * 64 + 32 * j + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + wm * 32 * MI + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (co < a.cout && c < a.ncol) wsp[(size_t)co * a.ncol + c] = acc[i][j][r];
      }
    }

  if (want_db) {      // the 16 row-threads of a chunk column meet in LDS and are added in row order
    float* const red = reinterpret_cast<float*>(lds);        // [16][128] floats = 8 KiB of the 16; the loop's last barrier freed the stages
#pragma unroll
    for (int j = 0; j < 8; ++j) red[lr * 128 + ch * 8 + j] = dbv[j];
    __syncthreads();
    if (tid < TM && co0 + tid < a.cout) {
      float s = 0.f;
      for (int r = 0; r < 16; ++r) s += red[r * 128 + tid];
      a.ws_db[(size_t)split * a.cout + co0 + tid] = s;
    }
  }
}

// Second pass: the splits' partials are added in split order and scattered to the parameter's OIHW layout; db likewise.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ ws_db,
                                                           float* __restrict__ dw, float* __restrict__ db, int splits, int cout, int cin,
                                                           int kk) {
  const int ncol = kk * cin;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long n_w = (long)cout * ncol;
  if (idx < n_w) {
    float s = 0.f;
    for (int i = 0; i < splits; ++i) s += ws[(size_t)i * n_w + idx];
    const int co = (int)(idx / ncol), c = (int)(idx - (long)co * ncol);
    const int t = c / cin, ci = c - t * cin;
    dw[((size_t)co * cin + ci) * kk + t] = s;
  } else if (db && idx < n_w + cout) {
    const int co = (int)(idx - n_w);
    float s = 0.f;
    for (int i = 0; i < splits; ++i) s += ws_db[(size_t)i * cout + co];
    db[co] = s;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
struct WgradPick {
  int mi;                 // 64 mi rows of D per workgroup
  int tiles_m, tiles_n;
  int splits, steps_per_split;
};

// The tile and the split of the pixel reduction.  No side effects.  Two workgroups per compute unit are wanted (16 KiB of LDS and
// <= 256 registers allow it); a split gets at least kMinSteps stages, and no split is empty.  d.n d.h d.w are the pixels the reduction
// runs over (the stride-2 caller passes the output map).
WgradPick choose_wgrad(const YoloConvDesc& d, int n_cu) {
  WgradPick k;
  k.mi = d.cout <= 64 ? 1 : 2;
  const int tm = 64 * k.mi, ncol = d.ksize * d.ksize * d.cin;
  k.tiles_m = (d.cout + tm - 1) / tm;
  k.tiles_n = (ncol + kTN - 1) / kTN;
  const long steps = ((long)d.n * d.h * d.w + kBK - 1) / kBK;
  const long tiles = (long)k.tiles_m * k.tiles_n;
  long want = (2L * n_cu + tiles - 1) / tiles;
  const long by_work = steps / kMinSteps > 1 ? steps / kMinSteps : 1;
  if (want > by_work) want = by_work;
  if (want > 64) want = 64;
  k.steps_per_split = (int)((steps + want - 1) / want);
  k.splits = (int)((steps + k.steps_per_split - 1) / k.steps_per_split);
  return k;
}

int roundup_i(int v, int m) { return (v + m - 1) / m * m; }

// what the backward entries of both strides ask of the forward's descriptor beside their own geometry: no epilogue the backward does
// not have, act none or LeakyReLU(0.1) (``relu_ok``: or ReLU), a non-empty shape in range, an input view on 8-channel groups
int bwd_check_shared(const YoloConvDesc& d, const char* fn, bool relu_ok) {
  YOLO_REQUIRE(!d.upsample2x, "%s: no backward of the upsampling store", fn);
  YOLO_REQUIRE(d.res_c_total == 0 && d.res_c_offset == 0 && d.aux_c_total == 0 && d.aux_c_offset == 0,
               "%s: no backward of the residual / pre-add epilogues", fn);
  YOLO_REQUIRE(d.act == YOLO_ACT_NONE || d.act == YOLO_ACT_LEAKY01 || (relu_ok && d.act == YOLO_ACT_RELU), "%s: act %d unsupported (none%s)", fn,
               d.act, relu_ok ? ", LeakyReLU(0.1) or ReLU" : " or LeakyReLU(0.1)");
  YOLO_REQUIRE(d.n > 0 && d.h > 0 && d.w > 0 && d.cout > 0, "%s: empty shape", fn);
  YOLO_REQUIRE(d.cin > 0 && d.cin % 8 == 0 && yolo_view_ok(d.cin, d.in_c_total, d.in_c_offset, 8),
               "%s: bad input view (cin %d, offset %d, total %d: multiples of 8)", fn, d.cin, d.in_c_offset, d.in_c_total);
  YOLO_REQUIRE((long)d.n * d.h * d.w < 0x7fffffffL / 4 && (long)d.ksize * d.ksize * d.cin * (long)d.cout < 0x7fffffffL,
               "%s: shape out of range", fn);
  return 0;
}

size_t wgrad_ws_bytes(const YoloConvDesc& d, int splits) {
  return (size_t)splits * d.cout * ((size_t)d.ksize * d.ksize * d.cin + 1) * sizeof(float);
}

// The two launches of a weight gradient.  d is the forward's descriptor; (mh, mw) the map the pixels run over (d.h, d.w at stride 1,
// d.ho, d.wo at stride 2); k = choose_wgrad on those pixels.
template <int STRIDE>
int launch_wgrad(const void* x, const void* g, float* dw_oihw, float* dbias, void* workspace, const YoloConvDesc& d, const WgradPick& k,
                 hipStream_t s, const char* fn) {
  const int mh = STRIDE == 1 ? d.h : d.ho, mw = STRIDE == 1 ? d.w : d.wo;
  WgradArgs a;
  a.x = (const bf16_t*)x;
  a.g = (const bf16_t*)g;
  a.ncol = d.ksize * d.ksize * d.cin;
  a.ws = (float*)workspace;
  float* const ws_db = a.ws + (size_t)k.splits * d.cout * a.ncol;
  a.ws_db = dbias ? ws_db : nullptr;
  a.n = d.n, a.h = d.h, a.w = d.w, a.cin = d.cin, a.x_total = d.in_c_total, a.x_offset = d.in_c_offset;
  a.cout = d.cout, a.cg = roundup_i(d.cout, 8), a.ksize = d.ksize, a.pad = d.pad;
  a.pixels = (long)d.n * mh * mw;
  a.steps_per_split = k.steps_per_split;
  a.step_h = (16 / mw) % mh, a.step_w = 16 % mw;
  a.ho = d.ho, a.wo = d.wo, a.step_n = 16 / (mh * mw);
  const dim3 grid(k.tiles_n, k.tiles_m, k.splits);
  if (k.mi == 1) hipLaunchKernelGGL((wgrad_kernel<1, STRIDE>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((wgrad_kernel<2, STRIDE>), grid, dim3(256), 0, s, a);
  if (const int rc = yolo_check_launch(fn, " (wgrad)")) return rc;
  const long total = (long)d.cout * a.ncol + d.cout;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks_for(total)), dim3(256), 0, s, (const float*)a.ws, (const float*)ws_db, dw_oihw,
                     dbias, k.splits, d.cout, d.cin, d.ksize * d.ksize);
  return yolo_check_launch(fn, " (reduce)");
}

}  // namespace
