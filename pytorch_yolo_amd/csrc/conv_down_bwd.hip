// Backward of the downsample: ConvBlock(3x3, stride 2, pad 1) of Darknet-53 (reference models/yolo_base.py:19-44), bf16 mode
// (DESIGN.md 3.6e).  g = bf16(dy * act'(y)) comes from yolo_conv2d_bwd_prepare on the output map; here:
//   dW = sum over the OUTPUT pixels of g[n,oh,ow][co] * x[n, 2 oh + kh - 1, 2 ow + kw - 1][ci], db     wgrad_kernel<MI, 2> (conv_wgrad.h) +
//                                                                                                       wgrad_reduce_kernel
//   dx[n,ih,iw][ci] = bf16(sum over co and the taps with ih + 1 - kh = 2 oh, iw + 1 - kw = 2 ow)        dgrad_parity_kernel
//   the dgrad operand [kh][kw][ci][co] bf16                                                             pack_weight_down_kernel
// No atomics and no read-modify-write: every element of dW, db, dx (its view) and of the used workspace is written once per call.
// The unpadded stride-2 first layer of SqueezeNet 1.1 (Conv2d(3, 64, 3, stride=2)) has the same weight gradient with pad 0
// - wgrad_kernel<MI, 2> takes the pad as an argument - behind the yolo_conv2d_stem_bwd_* entries; its input is the image: no data gradient.
#include "conv_wgrad.h"

namespace {

// out[kh][kw][ci][co] = bf16_rne(W[co][ci][kh][kw]): both operands of the data gradient are then contiguous along co
__global__ __launch_bounds__(256) void pack_weight_down_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, int cout, int cin) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 9L * cin * cout) return;
  const int co = (int)(idx % cout);
  const long r = idx / cout;
  const int ci = (int)(r % cin), t = (int)(r / cin);
  out[idx] = dev_f32_to_bf16_rne(w[((long)co * cin + ci) * 9 + t]);
}

// ---- parity dgrad ---------------------------------------------------------------------------------------------------------
// The input pixels fall into four classes by the parity (ph, pw) of (ih, iw).  A pixel (2 a + ph, 2 b + pw) of a class receives
//   ph = 0: kh = 1 from output row a            ph = 1: kh = 0 from output row a + 1 (if it exists) and kh = 2 from output row a
// and likewise along w: 1, 2, 2 or 4 taps, 9 per 2x2 block - the forward's FLOPs.  Per class one implicit GEMM
//   D[ci][m] = sum_{tap, co} Wp[tap][ci][co] * g[pixel of (m, tap)][co]          m = the class's pixels (n, a, b), K = taps * cout
// with both operands contiguous along K.  A workgroup of 4 waves (2 x 2) owns 128 pixels x (64 NJ) channels of one class; a stage is
// 64 couts of one tap: 128 rows of g and 64 NJ rows of Wp, 128 bytes each, in LDS with the 16-byte chunks XOR-swizzled, read back as
// whole 16-byte MFMA operands (v_mfma_f32_32x32x16_bf16: lane l holds row l & 31, k = 8 (l >> 5) .. + 7).  The weights are the MFMA's
// row operand, read in the row order perm() below, so that the 16 accumulators of a lane are two runs of 8 CONSECUTIVE channels of one
// pixel: two 16-byte stores.  Rows past the class, channels past cin / cout and output rows / columns past the map are zeroed BY INDEX
// at the load (redirected to the operand's first 16 bytes); nothing outside an operand is read.  Classes are laid out along grid.x,
// heaviest first: (1,1), (1,0), (0,1), (0,0); a class without pixels (h = 1 or w = 1) has no tiles.  (Interleaving the classes - workgroup
// 4 t + z = tile t of class z, so that the four classes of a stretch of pixels read the same rows of g side by side - was measured and
// is 1.1 - 1.6 x slower on the Darknet shapes: DESIGN.md 3.6e.)
constexpr int kDM = 128;     // pixels of a class per workgroup
constexpr int kDK = 64;      // couts per stage

struct DgradArgs {
  const bf16_t* g;      // [n][ho][wo][cout]
  const bf16_t* wp;     // [3][3][cin][cout]
  bf16_t* dx;           // [n][h][w][x_total], the view [x_offset, x_offset + cin)
  int n, h, w, ho, wo, cin, cout, x_total, x_offset;
  int tile_begin[5];    // first pixel tile of class z along grid.x; [4] = all tiles
};

__device__ __forceinline__ int dg_off(int row, int ch) {   // byte offset of 16-byte chunk ch (0..7) of the 128-byte row `row`
  return 128 * row + 16 * (ch ^ ((row >> 1) & 7));
}

template <int NJ>
__global__ __launch_bounds__(256, 2) void dgrad_parity_kernel(const DgradArgs a) {
  constexpr int TN = 64 * NJ;
  constexpr int kGRows = kDM / 32, kWRows = TN / 32;      // rows of a stage one thread loads
  __shared__ __attribute__((aligned(16))) unsigned char lds[(kDM + TN) * 128];
  unsigned char* const lg = lds;                  // g stage  [kDM][64 co]
  unsigned char* const lw = lds + kDM * 128;      // Wp stage [TN][64 co]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int z = 0;                                      // uniform
  while (z < 3 && (int)blockIdx.x >= a.tile_begin[z + 1]) ++z;
  const int ph = z < 2 ? 1 : 0, pw = (z & 1) ? 0 : 1;
  const int hc = (a.h + 1 - ph) >> 1, wc = (a.w + 1 - pw) >> 1;      // the class's rows and columns
  const int mtot = a.n * hc * wc;
  const int m0 = ((int)blockIdx.x - a.tile_begin[z]) * kDM;
  const int ci0 = blockIdx.y * TN;
  const int tw = 1 + pw, taps = (1 + ph) * tw;
  const int kchunks = (a.cout + kDK - 1) / kDK;
  const int steps = taps * kchunks;

  // what this thread stages: chunk `ch` of rows lr, lr + 32, ... of both operands; the rows are the same for every stage
  const int ch = tid & 7, lr = tid >> 3;
  int gpix[kGRows];          // g pixel (n, a, b) of the row
  unsigned gflag = 0;        // bit i: the row is in the class; bit 8 + i: output row a + 1 exists; bit 16 + i: output column b + 1 exists
#pragma unroll
  for (int i = 0; i < kGRows; ++i) {
    const int m = m0 + lr + 32 * i;
    const int nn = m / (hc * wc), rem = m - nn * (hc * wc);
    const int aa = rem / wc, bb = rem - aa * wc;
    gpix[i] = (nn * a.ho + aa) * a.wo + bb;
    gflag |= (m < mtot ? 1u : 0u) << i | (aa + 1 < a.ho ? 1u : 0u) << (8 + i) | (bb + 1 < a.wo ? 1u : 0u) << (16 + i);
  }

  struct Stage {
    u32x4 g[kGRows], w[kWRows];
    unsigned ok;             // bit i: row i of g, bit 8 + i: row i of Wp
  };
  auto fetch = [&](Stage& st, int tap, int kc) {      // tap, kc: uniform
    const int ti = tap / tw, tj = tap - ti * tw;
    const int doh = ph & (ti == 0), dow = pw & (tj == 0);
    const int kh = ph ? 2 * ti : 1, kw = pw ? 2 * tj : 1;
    const int co = kc * kDK + ch * 8;
    const bool c_ok = co < a.cout;
    st.ok = 0;
#pragma unroll
    for (int i = 0; i < kGRows; ++i) {
      const bool v = c_ok && ((gflag >> i) & 1u) && (!doh || ((gflag >> (8 + i)) & 1u)) && (!dow || ((gflag >> (16 + i)) & 1u));
      st.g[i] = *reinterpret_cast<const u32x4*>(v ? a.g + (long)(gpix[i] + doh * a.wo + dow) * a.cout + co : a.g);
      st.ok |= (v ? 1u : 0u) << i;
    }
#pragma unroll
    for (int i = 0; i < kWRows; ++i) {
      const int ci = ci0 + lr + 32 * i;
      const bool v = c_ok && ci < a.cin;
      st.w[i] = *reinterpret_cast<const u32x4*>(v ? a.wp + ((long)(kh * 3 + kw) * a.cin + ci) * a.cout + co : a.wp);
      st.ok |= (v ? 1u : 0u) << (8 + i);
    }
  };

  f32x16 acc[NJ][2];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][i][r] = 0.f;

  // MFMA row l & 31 of the weights is channel perm(l & 31) of the sub-tile: accumulator r of a lane is then channel
  // 16 (r >> 3) + 8 (l >> 5) + (r & 7)
  const int l31 = lane & 31, khalf = lane >> 5;
  const int prow = 16 * (l31 >> 4) + 8 * ((l31 >> 2) & 1) + 4 * ((l31 >> 3) & 1) + (l31 & 3);
  int w_off[NJ][2], g_off[2][2];      // [sub-tile][k step & 1]: the swizzle repeats every two k steps but for the chunk
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) w_off[j][t] = dg_off(wn * 32 * NJ + 32 * j + prow, 2 * t + khalf);
#pragma unroll
    for (int i = 0; i < 2; ++i) g_off[i][t] = dg_off(wm * 64 + 32 * i + l31, 2 * t + khalf);
  }

  Stage st;
  int tap = 0, kc = 0;
  fetch(st, tap, kc);
  for (int s = 0; s < steps; ++s) {
    const u32x4 zero = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < kGRows; ++i) *reinterpret_cast<u32x4*>(lg + dg_off(lr + 32 * i, ch)) = (st.ok >> i) & 1u ? st.g[i] : zero;
#pragma unroll
    for (int i = 0; i < kWRows; ++i) *reinterpret_cast<u32x4*>(lw + dg_off(lr + 32 * i, ch)) = (st.ok >> (8 + i)) & 1u ? st.w[i] : zero;
    __syncthreads();
    if (++kc == kchunks) kc = 0, ++tap;
    if (s + 1 < steps) fetch(st, tap, kc);      // uniform; the loads fly under this stage's MFMAs
#pragma unroll
    for (int ks = 0; ks < kDK / 16; ++ks) {
      // chunk 2 ks + khalf = (2 (ks & 1) + khalf) ^ (4 (ks >> 1)): bit 2 of the chunk is bit 2 of the XOR
      const int flip = 64 * (ks >> 1);
      bf16x8 wf[NJ], gf[2];
#pragma unroll
      for (int j = 0; j < NJ; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(lw + (w_off[j][ks & 1] ^ flip));
#pragma unroll
      for (int i = 0; i < 2; ++i) gf[i] = *reinterpret_cast<const bf16x8*>(lg + (g_off[i][ks & 1] ^ flip));
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[j], gf[i], acc[j][i], 0, 0, 0);
    }
    __syncthreads();
  }

  // D row (channel) = 16 (r >> 3) + 8 (lane >> 5) + (r & 7), D column (pixel) = lane & 31: two 16-byte stores per sub-tile
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + wm * 64 + 32 * i + l31;
    if (m >= mtot) continue;
    const int nn = m / (hc * wc), rem = m - nn * (hc * wc);
    const int aa = rem / wc, bb = rem - aa * wc;
    bf16_t* const px = a.dx + (((long)nn * a.h + 2 * aa + ph) * a.w + 2 * bb + pw) * a.x_total + a.x_offset;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int ci = ci0 + wn * 32 * NJ + 32 * j + 16 * half + 8 * khalf;
        if (ci >= a.cin) continue;
        bf16x8 out;
#pragma unroll
        for (int r = 0; r < 8; ++r) out[r] = (bf16_t)acc[j][i][8 * half + r];
        *reinterpret_cast<bf16x8*>(px + ci) = out;
      }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// what every entry point asks of the forward's descriptor
int down_check(const YoloConvDesc* dp, const char* fn) {
  YOLO_REQUIRE(dp, "%s: null descriptor", fn);
  const YoloConvDesc& d = *dp;
  YOLO_REQUIRE(d.ksize == 3, "%s: ksize %d unsupported (the downsample is 3x3)", fn, d.ksize);
  YOLO_REQUIRE(d.stride == 2, "%s: stride %d unsupported (stride 2; stride 1 is yolo_conv2d_bwd_*)", fn, d.stride);
  YOLO_REQUIRE(d.pad == 1 && d.ho == (d.h - 1) / 2 + 1 && d.wo == (d.w - 1) / 2 + 1,
               "%s: pad %d / output %dx%d: pad 1 and the symmetric output size (h - 1) / 2 + 1 only", fn, d.pad, d.ho, d.wo);
  YOLO_REQUIRE(d.out_dtype == YOLO_DT_BF16, "%s: out_dtype %d unsupported (a bf16 output)", fn, d.out_dtype);
  YOLO_REQUIRE(d.cout % 8 == 0 && d.out_c_offset >= 0 && (long)d.out_c_offset + d.cout <= d.out_c_total,
               "%s: bad output view (cout %d: a multiple of 8, offset %d, total %d)", fn, d.cout, d.out_c_offset, d.out_c_total);
  return bwd_check_shared(d, fn, false);
}

// choose_wgrad as it is, on the OUTPUT pixels
WgradPick choose_down_wgrad(const YoloConvDesc& d) {
  YoloConvDesc t = d;
  t.h = d.ho, t.w = d.wo;
  return choose_wgrad(t, yolo_conv::launch_cus());
}

// the unpadded first layer: 3x3, stride 2, pad 0, ho = (h - 3) / 2 + 1 (an even map's last row and column are never read)
int stem_check(const YoloConvDesc* dp, const char* fn) {
  YOLO_REQUIRE(dp, "%s: null descriptor", fn);
  const YoloConvDesc& d = *dp;
  YOLO_REQUIRE(d.ksize == 3 && d.stride == 2, "%s: ksize %d / stride %d unsupported (the unpadded first layer is 3x3 at stride 2)", fn, d.ksize,
               d.stride);
  YOLO_REQUIRE(d.h >= 3 && d.w >= 3, "%s: a %d x %d map has no unpadded 3x3 window", fn, d.h, d.w);
  YOLO_REQUIRE(d.pad == 0 && d.ho == (d.h - 3) / 2 + 1 && d.wo == (d.w - 3) / 2 + 1,
               "%s: pad %d / output %dx%d: pad 0 and the output size (h - 3) / 2 + 1 only (pad 1 is yolo_conv2d_down_bwd_*)", fn, d.pad, d.ho, d.wo);
  YOLO_REQUIRE(d.out_dtype == YOLO_DT_BF16, "%s: out_dtype %d unsupported (a bf16 output)", fn, d.out_dtype);
  YOLO_REQUIRE(d.cout % 8 == 0 && d.out_c_offset >= 0 && (long)d.out_c_offset + d.cout <= d.out_c_total,
               "%s: bad output view (cout %d: a multiple of 8, offset %d, total %d)", fn, d.cout, d.out_c_offset, d.out_c_total);
  return bwd_check_shared(d, fn, true);
}

struct DgradPick {
  int nj;               // 64 nj channels per workgroup
  int tiles_n;
  int tiles[4];         // pixel tiles of the classes (1,1), (1,0), (0,1), (0,0)
  int tile_begin[5];
};

DgradPick choose_dgrad(const YoloConvDesc& d) {
  DgradPick k;
  k.nj = d.cin <= 64 ? 1 : 2;
  k.tiles_n = (d.cin + 64 * k.nj - 1) / (64 * k.nj);
  k.tile_begin[0] = 0;
  for (int z = 0; z < 4; ++z) {
    const int ph = z < 2 ? 1 : 0, pw = (z & 1) ? 0 : 1;
    const long m = (long)d.n * ((d.h + 1 - ph) / 2) * ((d.w + 1 - pw) / 2);
    k.tiles[z] = (int)((m + kDM - 1) / kDM);
    k.tile_begin[z + 1] = k.tile_begin[z] + k.tiles[z];
  }
  return k;
}

}  // namespace

extern "C" size_t yolo_conv2d_down_bwd_workspace_bytes(const YoloConvDesc* d) {
  if (down_check(d, "conv2d_down_bwd_workspace_bytes")) return 0;
  return wgrad_ws_bytes(*d, choose_down_wgrad(*d).splits);
}

extern "C" int yolo_conv2d_down_bwd_pick(const YoloConvDesc* d, char* out, int out_len) {
  YOLO_REQUIRE(out && out_len > 0, "conv2d_down_bwd_pick: bad arguments");
  out[0] = 0;
  if (const int rc = down_check(d, "conv2d_down_bwd_pick")) return rc;
  const WgradPick k = choose_down_wgrad(*d);
  const DgradPick g = choose_dgrad(*d);
  snprintf(out, (size_t)out_len, "wgrad<%dx%d,BK%d,tr_b16,s2> grid %dx%d splits %d; dgrad<%dx%d,BK%d,parity> grid %dx%d tiles %d+%d+%d+%d",
           64 * k.mi, kTN, kBK, k.tiles_n, k.tiles_m, k.splits, kDM, 64 * g.nj, kDK, g.tile_begin[4], g.tiles_n, g.tiles[0], g.tiles[1],
           g.tiles[2], g.tiles[3]);
  return 0;
}

extern "C" int yolo_conv2d_down_bwd_weight(const void* x, const void* g, float* dw_oihw, float* dbias, void* workspace, size_t ws_bytes,
                                           const YoloConvDesc* dp, yolo_stream_t s) {
  if (const int rc = down_check(dp, "conv2d_down_bwd_weight")) return rc;
  const YoloConvDesc& d = *dp;
  YOLO_REQUIRE(x && g && dw_oihw && workspace, "conv2d_down_bwd_weight: null pointer");
  YOLO_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)g % 16 == 0 && (uintptr_t)workspace % 16 == 0 && (uintptr_t)dw_oihw % 4 == 0,
               "conv2d_down_bwd_weight: misaligned pointer");
  const WgradPick k = choose_down_wgrad(d);
  const size_t need = wgrad_ws_bytes(d, k.splits);
  if (ws_bytes < need) return yolo_set_error(YOLO_E_WORKSPACE, "conv2d_down_bwd_weight: workspace %zu < %zu bytes", ws_bytes, need);
  return launch_wgrad<2>(x, g, dw_oihw, dbias, workspace, d, k, (hipStream_t)s, "conv2d_down_bwd_weight");
}

// ---- the unpadded first layer: the same two launches with pad 0 ----------------------------------------------------------------------
extern "C" size_t yolo_conv2d_stem_bwd_workspace_bytes(const YoloConvDesc* d) {
  if (stem_check(d, "conv2d_stem_bwd_workspace_bytes")) return 0;
  return wgrad_ws_bytes(*d, choose_down_wgrad(*d).splits);
}

extern "C" int yolo_conv2d_stem_bwd_pick(const YoloConvDesc* d, char* out, int out_len) {
  YOLO_REQUIRE(out && out_len > 0, "conv2d_stem_bwd_pick: bad arguments");
  out[0] = 0;
  if (const int rc = stem_check(d, "conv2d_stem_bwd_pick")) return rc;
  const WgradPick k = choose_down_wgrad(*d);
  snprintf(out, (size_t)out_len, "wgrad<%dx%d,BK%d,tr_b16,s2,p0> grid %dx%d splits %d", 64 * k.mi, kTN, kBK, k.tiles_n, k.tiles_m, k.splits);
  return 0;
}

extern "C" int yolo_conv2d_stem_bwd_weight(const void* x, const void* g, float* dw_oihw, float* dbias, void* workspace, size_t ws_bytes,
                                           const YoloConvDesc* dp, yolo_stream_t s) {
  if (const int rc = stem_check(dp, "conv2d_stem_bwd_weight")) return rc;
  const YoloConvDesc& d = *dp;
  YOLO_REQUIRE(x && g && dw_oihw && workspace, "conv2d_stem_bwd_weight: null pointer");
  YOLO_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)g % 16 == 0 && (uintptr_t)workspace % 16 == 0 && (uintptr_t)dw_oihw % 4 == 0,
               "conv2d_stem_bwd_weight: misaligned pointer");
  const WgradPick k = choose_down_wgrad(d);
  const size_t need = wgrad_ws_bytes(d, k.splits);
  if (ws_bytes < need) return yolo_set_error(YOLO_E_WORKSPACE, "conv2d_stem_bwd_weight: workspace %zu < %zu bytes", ws_bytes, need);
  return launch_wgrad<2>(x, g, dw_oihw, dbias, workspace, d, k, (hipStream_t)s, "conv2d_stem_bwd_weight");
}

extern "C" int yolo_conv2d_down_bwd_data(const void* g, const void* w_packed_d, void* dx, const YoloConvDesc* dp, yolo_stream_t s) {
  if (const int rc = down_check(dp, "conv2d_down_bwd_data")) return rc;
  const YoloConvDesc& d = *dp;
  YOLO_REQUIRE(g && w_packed_d && dx, "conv2d_down_bwd_data: null pointer");
  YOLO_REQUIRE((uintptr_t)g % 16 == 0 && (uintptr_t)w_packed_d % 16 == 0 && (uintptr_t)dx % 16 == 0, "conv2d_down_bwd_data: misaligned pointer");
  const DgradPick k = choose_dgrad(d);
  DgradArgs a;
  a.g = (const bf16_t*)g, a.wp = (const bf16_t*)w_packed_d, a.dx = (bf16_t*)dx;
  a.n = d.n, a.h = d.h, a.w = d.w, a.ho = d.ho, a.wo = d.wo, a.cin = d.cin, a.cout = d.cout;
  a.x_total = d.in_c_total, a.x_offset = d.in_c_offset;
  for (int z = 0; z < 5; ++z) a.tile_begin[z] = k.tile_begin[z];
  const dim3 grid(k.tile_begin[4], k.tiles_n, 1);
  if (k.nj == 1) hipLaunchKernelGGL(dgrad_parity_kernel<1>, grid, dim3(256), 0, (hipStream_t)s, a);
  else hipLaunchKernelGGL(dgrad_parity_kernel<2>, grid, dim3(256), 0, (hipStream_t)s, a);
  return yolo_check_launch("conv2d_down_bwd_data");
}

extern "C" int yolo_pack_conv_weight_down_dev(const float* w_oihw, int cout, int cin, void* out, yolo_stream_t s) {
  YOLO_REQUIRE(w_oihw && out, "pack_down_dev: null pointer");
  YOLO_REQUIRE(cout > 0 && cin > 0 && cout % 8 == 0 && cin % 8 == 0 && 9L * cin * cout < 0x7fffffffL,
               "pack_down_dev: bad sizes (cout %d, cin %d: multiples of 8)", cout, cin);
  YOLO_REQUIRE((uintptr_t)w_oihw % 4 == 0 && (uintptr_t)out % 16 == 0, "pack_down_dev: misaligned pointer");
  hipLaunchKernelGGL(pack_weight_down_kernel, dim3(blocks_for(9L * cin * cout)), dim3(256), 0, (hipStream_t)s, w_oihw, (uint16_t*)out, cout,
                     cin);
  return yolo_check_launch("pack_down_dev");
}
