// Backward of the stride-1 ConvBlock / plain head convolutions (reference models/yolo_base.py:19-44), bf16 mode:
//   g  = bf16(dy * act'(y))                                  bwd_prepare_kernel, a 16-byte-per-lane stream; act' = 1 (none), y > 0 ? 1 : 0.1
//                                                            (LeakyReLU(0.1)) or y > 0 ? 1 : 0 (ReLU: SqueezeNet's convs)
//   dW = sum over pixels of g[p][co] * x[p + tap][ci], db    wgrad_kernel (conv_wgrad.h: MFMA, split over the pixels) + wgrad_reduce_kernel
//   dx = conv(g, flipped transposed W)                       the FORWARD dispatcher on a pack of pack_weight_kernel
// No atomics and no read-modify-write: every element of g, dW, db and of the used workspace is written once per call, in an order
// fixed by the shapes.
#include "conv_wgrad.h"

namespace {

// ---- g = bf16(dy * slope(y)) -----------------------------------------------------------------------------------------
// One thread owns 8 consecutive channels of one pixel of g (16 bytes).  dy is dense [pixels][cout]; y is the forward's output view.
// VEC: cout, the view of y and both bases allow whole 8-channel loads; otherwise element loads (a 255-channel head).
// leaky: the act looks at y; low: its slope where y <= 0 (0.1f LeakyReLU(0.1), 0.f ReLU).
template <typename TDY, typename TY, bool VEC>
__global__ __launch_bounds__(256) void bwd_prepare_kernel(const TDY* __restrict__ dy, const TY* __restrict__ y, bf16_t* __restrict__ g,
                                                          long pixels, int cout, int cg, int y_total, int y_offset, int leaky, float low) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int groups = cg / 8;
  if (idx >= pixels * groups) return;
  const long p = idx / groups;
  const int c0 = (int)(idx - p * groups) * 8;
  const TDY* dp = dy + p * cout + c0;
  const TY* yp = y + p * y_total + y_offset + c0;
  float dv[8], yv[8];
  if (VEC) {
    typedef TDY dvec __attribute__((ext_vector_type(8)));
    typedef TY yvec __attribute__((ext_vector_type(8)));
    const dvec a = *reinterpret_cast<const dvec*>(dp);
    yvec b;
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = (TY)1.f;
    if (leaky) b = *reinterpret_cast<const yvec*>(yp);                // act none never looks at y
#pragma unroll
    for (int j = 0; j < 8; ++j) dv[j] = (float)a[j], yv[j] = (float)b[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool in = c0 + j < cout;
      dv[j] = in ? (float)dp[j] : 0.f;
      yv[j] = in && leaky ? (float)yp[j] : 1.f;
    }
  }
  bf16x8 out;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float slope = (leaky && !(yv[j] > 0.f)) ? low : 1.f;       // torch's leaky_relu / relu backward: the low slope at y == 0
    out[j] = c0 + j < cout ? (bf16_t)(dv[j] * slope) : (bf16_t)0.f;
  }
  *reinterpret_cast<bf16x8*>(g + p * cg + c0) = out;
}

// ---- device twin of yolo_pack_conv_weight_f32 -----------------------------------------------------------------------------
// out[row][t * cin + c], zero elsewhere.  Plain: row = co, c = ci.  Transposed: row = ci, c = co, tap t reads tap kk - 1 - t.
__global__ __launch_bounds__(256) void pack_weight_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, int cout, int cin_w,
                                                          int kk, int cin, int cout_pad, int kpad, int transposed) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)cout_pad * kpad) return;
  const int row = (int)(idx / kpad), k = (int)(idx - (long)row * kpad);
  const int t = k / cin, c = k - t * cin;
  uint16_t v = 0;
  if (t < kk) {
    if (!transposed) {
      if (row < cout && c < cin_w) v = dev_f32_to_bf16_rne(w[((long)row * cin_w + c) * kk + t]);
    } else {
      if (row < cin_w && c < cout) v = dev_f32_to_bf16_rne(w[((long)c * cin_w + row) * kk + (kk - 1 - t)]);
    }
  }
  out[idx] = v;
}

// what every entry point asks of the forward's descriptor
int bwd_check(const YoloConvDesc* dp, const char* fn) {
  YOLO_REQUIRE(dp, "%s: null descriptor", fn);
  const YoloConvDesc& d = *dp;
  YOLO_REQUIRE(d.ksize == 1 || d.ksize == 3, "%s: ksize %d unsupported (1 or 3)", fn, d.ksize);
  YOLO_REQUIRE(d.stride == 1, "%s: stride %d unsupported (the backward covers stride 1)", fn, d.stride);
  YOLO_REQUIRE(d.pad == d.ksize / 2 && d.ho == d.h && d.wo == d.w, "%s: pad %d / output %dx%d: 'same' stride-1 convs only", fn, d.pad, d.ho, d.wo);
  YOLO_REQUIRE(d.out_dtype == YOLO_DT_BF16 || d.out_dtype == YOLO_DT_F32, "%s: out_dtype %d", fn, d.out_dtype);
  YOLO_REQUIRE(d.out_c_offset >= 0 && (long)d.out_c_offset + d.cout <= d.out_c_total, "%s: bad output view (cout %d, offset %d, total %d)", fn,
               d.cout, d.out_c_offset, d.out_c_total);
  return bwd_check_shared(d, fn, true);
}

constexpr int kZeroBias = 8192;
__device__ float g_zero_bias[kZeroBias];      // the data gradient's bias: never written

}  // namespace

// bytes = splits * cout * (k*k*cin + 1) floats: the splits' partial dW matrices, then their partial db rows
extern "C" size_t yolo_conv2d_bwd_workspace_bytes(const YoloConvDesc* d) {
  if (bwd_check(d, "conv2d_bwd_workspace_bytes")) return 0;
  return wgrad_ws_bytes(*d, choose_wgrad(*d, yolo_conv::launch_cus()).splits);
}

extern "C" int yolo_conv2d_bwd_pick(const YoloConvDesc* d, char* out, int out_len) {
  YOLO_REQUIRE(out && out_len > 0, "conv2d_bwd_pick: bad arguments");
  out[0] = 0;
  if (const int rc = bwd_check(d, "conv2d_bwd_pick")) return rc;
  const WgradPick k = choose_wgrad(*d, yolo_conv::launch_cus());
  snprintf(out, (size_t)out_len, "wgrad<%dx%d,BK%d,tr_b16> grid %dx%d splits %d", 64 * k.mi, kTN, kBK, k.tiles_n, k.tiles_m, k.splits);
  return 0;
}

template <typename TDY, typename TY>
static int launch_prepare(const void* dy, const void* y, void* g, const YoloConvDesc& d, int cg, hipStream_t s) {
  const long pixels = (long)d.n * d.h * d.w;
  const long total = pixels * (cg / 8);
  YOLO_REQUIRE(total < kMaxThreads, "conv2d_bwd_prepare: too many elements");
  const bool vec = d.cout % 8 == 0 && d.out_c_total % 8 == 0 && d.out_c_offset % 8 == 0 && (uintptr_t)dy % (8 * sizeof(TDY)) == 0 &&
                   (uintptr_t)y % (8 * sizeof(TY)) == 0;
  const int leaky = d.act != YOLO_ACT_NONE;
  const float low = d.act == YOLO_ACT_RELU ? 0.f : 0.1f;
  if (vec)
    hipLaunchKernelGGL((bwd_prepare_kernel<TDY, TY, true>), dim3(blocks_for(total)), dim3(256), 0, s, (const TDY*)dy, (const TY*)y,
                       (bf16_t*)g, pixels, d.cout, cg, d.out_c_total, d.out_c_offset, leaky, low);
  else
    hipLaunchKernelGGL((bwd_prepare_kernel<TDY, TY, false>), dim3(blocks_for(total)), dim3(256), 0, s, (const TDY*)dy, (const TY*)y,
                       (bf16_t*)g, pixels, d.cout, cg, d.out_c_total, d.out_c_offset, leaky, low);
  return yolo_check_launch("conv2d_bwd_prepare");
}

extern "C" int yolo_conv2d_bwd_prepare(const void* dy, int dy_dtype, const void* y, void* g, const YoloConvDesc* dp, yolo_stream_t s) {
  if (const int rc = bwd_check(dp, "conv2d_bwd_prepare")) return rc;
  const YoloConvDesc& d = *dp;
  YOLO_REQUIRE(dy && g && (y || d.act == YOLO_ACT_NONE), "conv2d_bwd_prepare: null pointer");
  YOLO_REQUIRE(dy_dtype == YOLO_DT_BF16 || dy_dtype == YOLO_DT_F32, "conv2d_bwd_prepare: dy_dtype %d (YOLO_DT_BF16 or YOLO_DT_F32)", dy_dtype);
  YOLO_REQUIRE((uintptr_t)g % 16 == 0 && (uintptr_t)dy % (dy_dtype == YOLO_DT_F32 ? 4 : 2) == 0, "conv2d_bwd_prepare: misaligned pointer");
  const int cg = roundup_i(d.cout, 8);
  const void* yy = y ? y : dy;      // act none never looks at the value
  const bool yf = y ? d.out_dtype == YOLO_DT_F32 : dy_dtype == YOLO_DT_F32;
  YoloConvDesc dd = d;
  if (!y) dd.out_c_total = d.cout, dd.out_c_offset = 0;
  if (dy_dtype == YOLO_DT_F32) return yf ? launch_prepare<float, float>(dy, yy, g, dd, cg, (hipStream_t)s) : launch_prepare<float, bf16_t>(dy, yy, g, dd, cg, (hipStream_t)s);
  return yf ? launch_prepare<bf16_t, float>(dy, yy, g, dd, cg, (hipStream_t)s) : launch_prepare<bf16_t, bf16_t>(dy, yy, g, dd, cg, (hipStream_t)s);
}

extern "C" int yolo_conv2d_bwd_weight(const void* x, const void* g, float* dw_oihw, float* dbias, void* workspace, size_t ws_bytes,
                                      const YoloConvDesc* dp, yolo_stream_t s) {
  if (const int rc = bwd_check(dp, "conv2d_bwd_weight")) return rc;
  const YoloConvDesc& d = *dp;
  YOLO_REQUIRE(x && g && dw_oihw && workspace, "conv2d_bwd_weight: null pointer");
  YOLO_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)g % 16 == 0 && (uintptr_t)workspace % 16 == 0 && (uintptr_t)dw_oihw % 4 == 0,
               "conv2d_bwd_weight: misaligned pointer");
  const WgradPick k = choose_wgrad(d, yolo_conv::launch_cus());
  const size_t need = wgrad_ws_bytes(d, k.splits);
  if (ws_bytes < need) return yolo_set_error(YOLO_E_WORKSPACE, "conv2d_bwd_weight: workspace %zu < %zu bytes", ws_bytes, need);
  return launch_wgrad<1>(x, g, dw_oihw, dbias, workspace, d, k, (hipStream_t)s, "conv2d_bwd_weight");
}

extern "C" int yolo_conv2d_bwd_data(const void* g, const void* w_packed_t, void* dx, const YoloConvDesc* dp, yolo_stream_t s) {
  if (const int rc = bwd_check(dp, "conv2d_bwd_data")) return rc;
  const YoloConvDesc& d = *dp;
  YOLO_REQUIRE(g && w_packed_t && dx, "conv2d_bwd_data: null pointer");
  YoloConvDesc t = d;                 // the transposed conv: g [n,h,w,roundup(cout,8)] -> the view of x
  t.cin = t.in_c_total = roundup_i(d.cout, 8);
  t.in_c_offset = 0;
  t.cout = d.cin, t.out_c_total = d.in_c_total, t.out_c_offset = d.in_c_offset;
  t.act = YOLO_ACT_NONE;
  t.out_dtype = YOLO_DT_BF16;
  t.kpad = roundup_i(d.ksize * d.ksize * t.cin, 64);
  t.cout_pad = roundup_i(d.cin, 128);
  YOLO_REQUIRE(t.cout_pad <= kZeroBias, "conv2d_bwd_data: cin %d beyond %d", d.cin, kZeroBias);
  float* zero = nullptr;
  const hipError_t e = hipGetSymbolAddress((void**)&zero, HIP_SYMBOL(g_zero_bias));
  if (e != hipSuccess) return yolo_set_error((int)e, "conv2d_bwd_data: hipGetSymbolAddress: %s", hipGetErrorString(e));
  return yolo_conv2d_launch(g, w_packed_t, zero, nullptr, dx, nullptr, &t, (hipStream_t)s);
}

extern "C" int yolo_pack_conv_weight_dev(const float* w_oihw, int cout, int cin_w, int ksize, int cin, int cout_pad, int kpad,
                                         int transposed, void* out, yolo_stream_t s) {
  YOLO_REQUIRE(w_oihw && out, "pack_dev: null pointer");
  YOLO_REQUIRE(cout > 0 && cin_w > 0 && (ksize == 1 || ksize == 3) && cin > 0 && (long)ksize * ksize * cin <= kpad, "pack_dev: bad sizes");
  if (transposed) YOLO_REQUIRE(cout <= cin && cin_w <= cout_pad, "pack_dev: transposed form needs cout <= cin and cin_w <= cout_pad");
  else YOLO_REQUIRE(cin_w <= cin && cout <= cout_pad, "pack_dev: bad sizes");
  const long total = (long)cout_pad * kpad;
  YOLO_REQUIRE(total < kMaxThreads, "pack_dev: too many elements");
  hipLaunchKernelGGL(pack_weight_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, w_oihw, (uint16_t*)out, cout, cin_w,
                     ksize * ksize, cin, cout_pad, kpad, transposed ? 1 : 0);
  return yolo_check_launch("pack_dev");
}
