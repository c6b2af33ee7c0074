/*
 * yolo_hip.h — C ABI of libyolo_hip.so: the MI355X (gfx950) YOLOv3 inference hot path.
 *
 * The reference (Dipet/pytorch_yolo) has no FFI: its seam is the nn.Module API.  Each entry
 * point below replaces the ATen dispatches of one reference function (file:line relative to
 * /root/reference/pytorch_yolo) and is what a ctypes stub on the reference side would bind
 * (INTEGRATION.md shows that stub).
 *
 * Conventions
 *  - plain pointers + sizes only; every device buffer is owned by the caller (torch tensors);
 *    the library never allocates, frees or retains device memory.  State it does keep (none of it numerics): the process-wide
 *    tuning knobs of yolo_set_tuning / yolo_set_launch_cus, per-device "LDS limit raised" flags, and the events / CU-masked streams
 *    a caller creates through yolo_event_create / yolo_stream_create_cu_mask and owns until it destroys them.
 *  - asynchronous launch on the caller's hipStream_t; no internal synchronisation; graph-capturable.
 *  - return 0 on success; >0 = hipError_t from the launch; <0 = YOLO_E_* argument error.
 *    yolo_last_error() returns a thread-local message for the last non-zero return.
 *  - activations are NHWC; "view" = (base pointer, c_offset, c_total): channel c of pixel p lives at
 *    base[p * c_total + c_offset + c].  bf16 activation channel counts/offsets are multiples of 8.
 */
#ifndef YOLO_HIP_H
#define YOLO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* yolo_stream_t; /* hipStream_t */

#if defined(__GNUC__)
#define YOLO_API __attribute__((visibility("default")))
#else
#define YOLO_API
#endif

enum { YOLO_E_ARG = -1, YOLO_E_UNSUPPORTED = -2, YOLO_E_WORKSPACE = -3 };
enum { YOLO_ACT_NONE = 0, YOLO_ACT_LEAKY01 = 1, YOLO_ACT_RELU6 = 2, YOLO_ACT_RELU = 3,
       YOLO_ACT_SWISH = 4 /* x * sigmoid(x): SwissActivation, models/yolov3_tiny_efficient.py:13-19 */ };
enum { YOLO_DT_BF16 = 0, YOLO_DT_F32 = 1, YOLO_DT_F16 = 2 /* IEEE half: the fp16-operand entry points below */ };

YOLO_API const char* yolo_last_error(void);
/* ABI version of this header: 2.  History: 1 -> 2 (round 5; the change itself dates from round 4): YoloOp's two former padding words
 * are head_filter_conf / head_filter_min_wh, and a HEAD_DECODE op with y == NULL and workspace != NULL now means the FILTER form
 * (yolo_head_decode_filter_fwd) - a caller built against version 1 that left y NULL or garbage in `workspace` on a head op would
 * silently change behaviour, so the number moved although no struct size did (yolo_abi_sizeof cannot see such a change);
 * YoloPipeStep / yolo_pipeline_step / yolo_event_* / yolo_pack_detections / yolo_nms_merge_compact were added. */
YOLO_API int yolo_abi_version(void);
/* Tuning / A-B hook (process-wide, not part of the numerics contract): overrides what the environment variables
 * YOLO_CONV_VARIANT (knob 0), YOLO_CONV_DEBUG (knob 1), YOLO_CONV_PP (knob 2), YOLO_RESUNIT_DEBUG (knob 3), YOLO_MBCONV_DEBUG (knob 4),
 * YOLO_STEM_DEBUG (knob 5), YOLO_STEM_ONE_ROLE (knob 6), YOLO_MBWIDE_DEBUG (knob 7), YOLO_MBWIDE_FORM (knob 8), YOLO_DWCONV_DEBUG
 * (knob 9), YOLO_SPP_NO_LINES (knob 10) and YOLO_RESUNIT_STAGGER (knob 11) set at the first use.  Returns the old value; any other
 * knob is YOLO_E_ARG.  pytorch_yolo_amd/csrc/tuning.h is the table of the knobs and names every bit of them. */
YOLO_API int yolo_set_tuning(int knob, int value);

/* ---- input packing: the `imgs.to(device)` + first-layer layout step (utils/utils.py:374) -----
 * x: f32 NCHW [n,c,h,w]  ->  y: bf16 NHWC [n,h,w,c_pad] (channels c..c_pad-1 zero). */
YOLO_API int yolo_pack_input_nchw_f32(const float* x, void* y, int n, int c, int h, int w, int c_pad,
                             yolo_stream_t s);

/* ---- ConvBlock.forward (models/yolo_base.py:19-44) with the BN already folded
 *      (utils/torch_utils.py:33-60), plain nn.Conv2d heads (models/yolov3_tiny.py:38,42),
 *      and the element-wise neighbours fused into the epilogue:
 *      Add (models/yolov3_spp.py:12-14), Upsample x2 (models/yolo_layer.py:6-13),
 *      Concat placement (models/yolo_layer.py:16-22).
 *
 *  y = act(conv(x, W) + bias);  if y_preadd: y_preadd = y;  if residual: y += residual;  store.
 *  Implicit GEMM on MFMA 32x32x16 bf16, fp32 accumulate.  groups == 1.
 */
typedef struct YoloConvDesc {
  int32_t n, h, w;                 /* input batch / spatial size                           */
  int32_t cin;                     /* logical input channels, multiple of 8                */
  int32_t in_c_total, in_c_offset; /* input view                                           */
  int32_t ho, wo;                  /* conv output spatial size (before optional upsample):
                                      (h + 2 pad - ksize) / stride + 1, or ONE more - the window of the last row /
                                      column then hangs over the bottom / right edge by one more zero (TensorFlow
                                      "same" padding of efficientnet_pytorch's Conv2dSamePadding at stride 2)       */
  int32_t cout;                    /* logical output channels                              */
  int32_t out_c_total, out_c_offset;
  int32_t ksize, stride, pad;      /* square kernel 1 or 3; zero padding                   */
  int32_t act;                     /* YOLO_ACT_*                                           */
  int32_t upsample2x;              /* 1: each output pixel is written to a 2x2 block of a
                                      [n,2ho,2wo,out_c_total] tensor                       */
  int32_t out_dtype;               /* YOLO_DT_BF16 | YOLO_DT_F32 (detection heads)         */
  int32_t kpad;                    /* packed K = roundup(ksize*ksize*cin, 64)              */
  int32_t cout_pad;                /* packed rows = roundup(cout, 128) (zero rows)         */
  int32_t res_c_total, res_c_offset; /* residual view (bf16), same spatial size as output  */
  int32_t aux_c_total, aux_c_offset; /* pre-add copy view (bf16)                           */
} YoloConvDesc;

/* Operand sizes.  The conv kernels address x and the packed weights with 32-bit byte offsets: the bytes behind the x VIEW,
 * n * h * w * in_c_total * 2, and cout_pad * kpad * 2 must stay below 0xF0000000 (3.75 GiB); from there on yolo_conv2d_fwd,
 * yolo_conv2d_f16_fwd, yolo_conv3x3_t20_f16_fwd, yolo_head_decode_*_fwd and yolo_resunit_fwd return YOLO_E_UNSUPPORTED
 * ("tensor larger than 3.75 GiB not supported"), and n * ho * wo must stay below 2^31 / 4 pixels ("M out of range").  y, the
 * residual and the pre-add copy have no such limit: at 0xF0000000 bytes (n * ho * wo * c_total * 2) the forms that address them
 * with 32-bit offsets step aside for one that writes through 64-bit pointers - the 20x20-tile 3x3 kernels (t20v2, t20s2) for the
 * halo or the gather kernel, the streaming 1x1 forms (stream1x1, stream1x1p) for the gather kernel - which yolo_conv2d_pick names.
 * tests/test_large_operands_cpu.py pins both sides of each bound, tests/test_large_operands_gpu.py runs every family on operands
 * of 0xEECC8000 bytes and the fallbacks on a y of 0x113898000 bytes. */

/* w_packed: bf16 [cout_pad][kpad], k = (kh*ksize + kw)*cin + c  (yolo_pack_conv_weight_f32).
 * bias: f32 [cout_pad].  residual / y_preadd may be NULL. */
YOLO_API int yolo_conv2d_fwd(const void* x, const void* w_packed, const float* bias, const void* residual,
                    void* y, void* y_preadd, const YoloConvDesc* d, yolo_stream_t s);

/* The kernel instance + grid yolo_conv2d_fwd would launch for d ("t20v2<...> grid 512"): nothing is launched and no GPU is
 * needed - the regression guard of the tile rules (tests pin the BASELINE shapes). */
YOLO_API int yolo_conv2d_pick(const YoloConvDesc* d, int has_residual, int has_preadd, char* out, int out_len);

/* Split-K form for layers with few pixels and a long K (3x3 256 -> 512 on 13x13, 3x3 1280 -> 64 on 13x13: fewer tiles than
 * half the CUs): `splits` workgroups share a tile's K range, write fp32 partials to `workspace` and the last one to
 * arrive (counters, zero-initialised once by the caller, self-resetting) sums them in split order and runs the normal
 * epilogue - deterministic.  yolo_conv2d_splitk_plan() says whether a layer takes it (splits >= 2) and how much
 * workspace / how many int32 counters it needs; layers it declines go through yolo_conv2d_fwd.
 * EXPERIMENTAL: exact, but slower than the plain launch on MI355X today (the partial exchange crosses XCD L2s); the
 * engine only uses it with YOLO_SPLITK=1. */
YOLO_API int yolo_conv2d_splitk_plan(const YoloConvDesc* d, int has_residual, int has_preadd, int* splits, size_t* ws_bytes,
                                     int* n_counters);
YOLO_API int yolo_conv2d_splitk_fwd(const void* x, const void* w_packed, const float* bias, const void* residual, void* y,
                                    void* y_preadd, const YoloConvDesc* d, int splits, void* workspace, size_t ws_bytes,
                                    int32_t* counters, yolo_stream_t s);

/* ---- backward of ConvBlock.forward / the plain heads (models/yolo_base.py:19-44, models/yolov3_tiny.py:38,42; what torch autograd
 *  does for the reference's nn.Conv2d + LeakyReLU), bf16 mode, STRIDE 1 (1x1 and 3x3 "same" convs): csrc/conv_bwd.hip.
 *  Every entry takes the FORWARD's descriptor d of  y = act(conv(x, bf16(W)) + bias)  and returns YOLO_E_ARG for stride != 1, ksize not
 *  in {1, 3}, pad != ksize / 2, upsample2x, a residual or pre-add view (res_* / aux_* non-zero), an act other than YOLO_ACT_NONE /
 *  YOLO_ACT_LEAKY01 / YOLO_ACT_RELU, or misaligned views.  Arithmetic, cg = roundup(cout, 8):
 *    g  = bf16_rne(fp32(dy) * (y > 0 ? 1 : 0.1f))  (act none: bf16_rne(dy); ReLU: the factor is y > 0 ? 1 : 0), bf16 NHWC [n,h,w,cg],
 *         channels cout..cg-1 zero;
 *    dW[co][ci][kh][kw] = sum_{n,oh,ow} g[n,oh,ow,co] * x[n,oh+kh-pad,ow+kw-pad,ci]  (taps outside the image add nothing), bf16
 *         operands, fp32 accumulation, fp32 in the parameter's OIHW layout [cout][cin][k][k];   db[co] = sum g, fp32;
 *    dx = bf16_rne(conv(g, Wt)),  Wt[ci][co][kh][kw] = bf16(W)[co][ci][k-1-kh][k-1-kw], same pad, fp32 accumulation.
 *  No atomics: two runs give the same bits.  Every element of g, dW, db and dx (its view) is written, never read-modify-written, and
 *  nothing in the workspace needs initialising.
 *  yolo_conv2d_bwd_workspace_bytes: splits * cout * (k*k*cin + 1) * 4 - the fp32 partial dW of each split of the pixel reduction, then
 *    the partial db rows (0 with a message for a descriptor the backward does not take).
 *  yolo_conv2d_bwd_pick: "wgrad<128x128,BK64,tr_b16> grid 9x2 splits 29" - tile, grid (column tiles x cout tiles) and split count of
 *    yolo_conv2d_bwd_weight; no launch, no GPU.
 *  yolo_conv2d_bwd_prepare: dy is DENSE [n,h,w,cout] of dy_dtype (YOLO_DT_BF16 | YOLO_DT_F32; any cout); y is the forward's output
 *    in d's output view and d->out_dtype (may be NULL for act none); writes g.
 *  yolo_conv2d_bwd_weight: x through d's input view; dbias may be NULL; the second pass adds the splits in split order.
 *  yolo_conv2d_bwd_data: runs yolo_conv2d_fwd's dispatcher on g with w_packed_t = yolo_pack_conv_weight_dev(..., transposed = 1, ...)
 *    of shape [roundup(cin,128)][roundup(k*k*cg,64)], act none, zero bias; dx = d's INPUT view (in_c_total / in_c_offset), the other
 *    channels of that buffer are left alone.
 *  yolo_pack_conv_weight_dev: device twin of yolo_pack_conv_weight_f32 - w_oihw f32 [cout][cin_w][k][k] ON THE DEVICE -> bf16
 *    [cout_pad][kpad], RNE, zero padding.  transposed = 0: row co, k = (kh*ks+kw)*cin + ci (cin_w <= cin, cout <= cout_pad);
 *    transposed = 1: the data gradient's matrix, row ci, k = (kh*ks+kw)*cin + co holding W[co][ci][ks-1-kh][ks-1-kw] - cin is then the
 *    channel count of g (cout <= cin), cout_pad >= cin_w. */
YOLO_API size_t yolo_conv2d_bwd_workspace_bytes(const YoloConvDesc* d);
YOLO_API int yolo_conv2d_bwd_pick(const YoloConvDesc* d, char* out, int out_len);
YOLO_API int yolo_conv2d_bwd_prepare(const void* dy, int dy_dtype, const void* y, void* g, const YoloConvDesc* d, yolo_stream_t s);
YOLO_API int yolo_conv2d_bwd_weight(const void* x, const void* g, float* dw_oihw, float* dbias, void* workspace, size_t ws_bytes,
                                    const YoloConvDesc* d, yolo_stream_t s);
YOLO_API int yolo_conv2d_bwd_data(const void* g, const void* w_packed_t, void* dx, const YoloConvDesc* d, yolo_stream_t s);
YOLO_API int yolo_pack_conv_weight_dev(const float* w_oihw, int cout, int cin_w, int ksize, int cin, int cout_pad, int kpad,
                                       int transposed, void* out, yolo_stream_t s);

/* ---- backward of the downsample: ConvBlock(3x3, stride 2, pad 1), the five stride-2 layers of Darknet-53 (models/yolo_base.py:19-44;
 *  what torch autograd does for the reference's nn.Conv2d(k=3, s=2, p=1) + LeakyReLU), bf16 mode: csrc/conv_down_bwd.hip, DESIGN.md 3.6e.
 *  Every entry takes the FORWARD's stride-2 descriptor d of  y = act(conv(x, bf16(W)) + bias)  (yolo_conv2d_fwd; ho = (h - 1) / 2 + 1,
 *  wo likewise: torch's output size for even and odd maps) and returns YOLO_E_ARG with a message for anything else: stride 1 (that is
 *  yolo_conv2d_bwd_*), ksize 1 or 5, pad != 1, the "one more row" ho of Conv2dSamePadding, upsample2x, a residual or pre-add view, an
 *  fp32 output, an act other than YOLO_ACT_NONE / YOLO_ACT_LEAKY01, cin % 8, cout % 8 or misaligned views.  Arithmetic:
 *    g  = bf16_rne(fp32(dy) * (y > 0 ? 1 : 0.1f)), dense bf16 [n,ho,wo,cout]: yolo_conv2d_bwd_prepare with the STRIDE-1 descriptor of the
 *         output map (h = ho, w = wo, ksize 1 or 3, the same output view and act) - there is no prepare entry here;
 *    dW[co][ci][kh][kw] = sum_{n,oh,ow} g[n,oh,ow,co] * x[n, 2 oh + kh - 1, 2 ow + kw - 1, ci]  (taps outside the image add nothing), bf16
 *         operands, fp32 accumulation, fp32 OIHW [cout][cin][3][3];   db[co] = sum g, fp32;
 *    dx[n,ih,iw,ci] = bf16_rne(sum g[n,oh,ow,co] * bf16(W)[co][ci][kh][kw]) over co and the (kh, kw) with ih + 1 - kh = 2 oh and
 *         iw + 1 - kw = 2 ow, 0 <= oh < ho, 0 <= ow < wo; fp32 accumulation.  By the parity of (ih, iw) a pixel has 1, 2 or 4 taps.
 *  No atomics: two runs give the same bits.  Every element of dW, db and dx (its view) is written exactly once, never
 *  read-modify-written, and nothing in the workspace needs initialising.
 *  yolo_conv2d_down_bwd_workspace_bytes: splits * cout * (9 cin + 1) * 4, the split rule of yolo_conv2d_bwd_weight applied to the n ho wo
 *    OUTPUT pixels (0 with a message for a descriptor these entries do not take).
 *  yolo_conv2d_down_bwd_pick: "wgrad<128x128,BK64,tr_b16,s2> grid 9x2 splits 29; dgrad<128x128,BK64,parity> grid 6400x1 tiles
 *    1600+1600+1600+1600" - the weight gradient's tile, grid and splits, then the data gradient's tile (pixels x channels), grid (pixel
 *    tiles of all classes x channel tiles) and the pixel tiles of the parity classes (ih, iw) = (odd, odd), (odd, even), (even, odd),
 *    (even, even) in launch order; no launch, no GPU.
 *  yolo_conv2d_down_bwd_weight: x through d's input view; dbias may be NULL; the second pass adds the splits in split order.
 *  yolo_conv2d_down_bwd_data: one launch for the four parity classes; w_packed_d from yolo_pack_conv_weight_down_dev; dx = d's INPUT
 *    view (in_c_total / in_c_offset), the other channels of that buffer are left alone.
 *  yolo_pack_conv_weight_down_dev: w_oihw f32 [cout][cin][3][3] ON THE DEVICE -> bf16 [3][3][cin][cout], RNE (the rounding of
 *    yolo_pack_conv_weight_f32): out holds exactly 9 * cin * cout bf16 = 18 * cin * cout bytes, no padding; cout % 8 == cin % 8 == 0. */
YOLO_API size_t yolo_conv2d_down_bwd_workspace_bytes(const YoloConvDesc* d);
YOLO_API int yolo_conv2d_down_bwd_pick(const YoloConvDesc* d, char* out, int out_len);
YOLO_API int yolo_conv2d_down_bwd_weight(const void* x, const void* g, float* dw_oihw, float* dbias, void* workspace, size_t ws_bytes,
                                         const YoloConvDesc* d, yolo_stream_t s);
YOLO_API int yolo_conv2d_down_bwd_data(const void* g, const void* w_packed_d, void* dx, const YoloConvDesc* d, yolo_stream_t s);
YOLO_API int yolo_pack_conv_weight_down_dev(const float* w_oihw, int cout, int cin, void* out, yolo_stream_t s);

/* ---- training-mode ConvBlock: the BatchNorm2d between the conv and the LeakyReLU(0.1) (models/yolo_base.py:19-44, Conv2d(bias=False)
 *  -> BatchNorm2d -> LeakyReLU(0.1)) with batch or running statistics, and its backward; bf16 mode: csrc/batchnorm.hip, DESIGN.md 3.6d.
 *  z = bf16(conv(x, bf16(W))) (yolo_conv2d_fwd with act none and a zero bias) is DENSE [pixels][c], pixels = n h w, c % 8 == 0.  Every
 *  fp32 and fp64 operation below is rounded on its own (no contraction):
 *    training statistics: S1 = sum z, S2 = sum z z over the pixels in float64; mean64 = S1 / pixels; var64 = max(S2 / pixels -
 *      mean64 mean64, 0); mean = f32(mean64); invstd = f32(1 / sqrt(var64 + (double)eps)); scale = gamma invstd; shift = beta - mean
 *      scale; running_mean <- running_mean (1 - momentum) + momentum mean; running_var <- running_var (1 - momentum) + momentum
 *      f32(var64 pixels / (pixels - 1))  (torch's unbiased form), both in fp32, in place, each only where its pointer is given.
 *    eval statistics: mean = running_mean, invstd = f32(1 / sqrt((double)running_var + (double)eps)), scale and shift as above.
 *    saved: f32 [4][c] = mean, invstd, scale, shift.
 *    forward: a = f32(z) scale + shift;  y = bf16_rne(a > 0 ? a : 0.1f a)  (act none: bf16_rne(a)).
 *    backward: slope = a > 0 ? 1 : 0.1f (act none: 1); ga = f32(dy) slope; xh = (f32(z) - mean) invstd; B = sum ga, G = sum ga xh
 *      (fp32 terms, float64 sums); dbeta = f32(B); dgamma = f32(G); c1 = f32(B / pixels), c2 = f32(G / pixels) (batch_stats = 0: both
 *      0); g = bf16_rne(scale ((ga - c1) - xh c2)), dense [pixels][c]: the operand yolo_conv2d_bwd_weight (dbias = NULL) and
 *      yolo_conv2d_bwd_data take with the act-none descriptor of the conv.
 *  The two reductions split the pixels over workgroups that write float64 partials into the caller's workspace; one thread per channel
 *  adds them in split order.  No atomics: two runs give the same bits; every output and every used workspace byte is written, never
 *  read-modify-written (running_mean / running_var are the one in-place update), and nothing in the workspace needs initialising.
 *  yolo_bn_workspace_bytes: 2 c floats (c1 | c2, written by yolo_bn_act_bwd and readable after it) followed by splits * 2 * c doubles;
 *    0 with a message for a shape the entries do not take.  The split count follows yolo_set_launch_cus.
 *  yolo_bn_pick: "bn_reduce<8x32> grid 256x1 passes 100 last 100" - rows x chunk columns of a pass, grid (row splits x column tiles of 2048
 *    channels), passes per split and those of the last split; no launch, no GPU.
 *  yolo_bn_train_stats: pixels >= 2; running_mean / running_var may be NULL.    yolo_bn_eval_stats: nothing is reduced or updated.
 *  yolo_bn_act_bwd: dy dense [pixels][c] of dy_dtype (YOLO_DT_BF16 | YOLO_DT_F32); batch_stats = 1 after yolo_bn_train_stats, 0 after
 *    yolo_bn_eval_stats; g, dgamma and dbeta may each be NULL (not wanted).
 *  YOLO_E_ARG (YOLO_E_WORKSPACE for a small workspace) before any launch for c % 8, an act other than YOLO_ACT_NONE / YOLO_ACT_LEAKY01,
 *  pixels < 2 with batch statistics, a null or misaligned pointer (z, y, dy, g, saved, ws: 16 bytes; the fp32 vectors: 4). */
YOLO_API size_t yolo_bn_workspace_bytes(long long pixels, int c);
YOLO_API int yolo_bn_pick(long long pixels, int c, char* out, int out_len);
YOLO_API int yolo_bn_train_stats(const void* z, long long pixels, int c, const float* gamma, const float* beta, float eps, float momentum,
                                 float* running_mean, float* running_var, float* saved, void* ws, size_t ws_bytes, yolo_stream_t s);
YOLO_API int yolo_bn_eval_stats(const float* gamma, const float* beta, const float* running_mean, const float* running_var, int c,
                                float eps, float* saved, yolo_stream_t s);
YOLO_API int yolo_bn_act_fwd(const void* z, const float* saved, void* y, long long pixels, int c, int act, yolo_stream_t s);
YOLO_API int yolo_bn_act_bwd(const void* dy, int dy_dtype, const void* z, const float* saved, long long pixels, int c, int act,
                             int batch_stats, void* g, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, yolo_stream_t s);

/* ---- the layers between the convs of a training step of YOLOv3 / YOLOv3-SPP, each with its backward; bf16 mode: csrc/route.hip and one
 *  entry of csrc/batchnorm.hip, DESIGN.md 3.6f.  Every map is bf16, DENSE NHWC, every channel count % 8 == 0 (16-byte accesses).  No
 *  atomics, no workspace; every output element is written exactly once and every sum has a fixed order, so two runs give the same bits.
 *  Every fp32 operation below is rounded on its own (no contraction).
 *  yolo_bn_act_add_fwd: yolo_bn_act_fwd's pass with the residual unit's add (models/yolov3_spp.py:12-14,42-46) fused in:
 *      a = f32(z) scale + shift;  t = a > 0 ? a : 0.1f a  (act none: t = a);  y_preadd = bf16_rne(t) (only where the pointer is given: the
 *      tensor the reference routes to the FPN from the last unit of down3 / down4);  y = bf16_rne(t + f32(residual)).
 *    The backward needs no entry of its own: dy (plus the gradient of y_preadd where it was routed) goes to yolo_bn_act_bwd, and dy
 *    unchanged is the residual's gradient.
 *  yolo_spp_train_fwd: y [n,h,w,4c] = cat([maxpool5(x), maxpool9(x), maxpool13(x), x], channel) of x [n,h,w,c] (models/yolov3_spp.py:75-77,
 *    129: stride 1, pad k / 2 with -inf), and idx [n,h,w,3c] uint8: the argmax of each window as (row offset) k + (column offset) inside
 *    the window (0 .. k k - 1; the centre is (k k - 1) / 2).  The argmax is the window's FIRST maximum in row-major order (torch's rule);
 *    a NaN is never greater, so x must hold no NaN.  Any h, w >= 1 (a map smaller than the windows included).
 *  yolo_spp_bwd: dx [n,h,w,c] from dy [n,h,w,4c] and idx, as a gather: acc = 0; for k = 5, 9, 13 in turn, for the window centres q within
 *    k / 2 of the pixel p in row-major order: acc = acc + f32(dy_k[q]) where idx_k[q] names p; dx[p] = bf16_rne(acc + f32(dy_pass[p])).
 *    Maps of up to 1600 pixels (40 x 40) are staged in LDS per (image, 8 channels); larger maps run the same code on global memory.
 *  yolo_upsample2_concat_fwd: y [n,2h,2w,ca+cb] = cat([nearest_x2(a), b], channel) of a [n,h,w,ca] and b [n,2h,2w,cb]
 *    (models/yolo_layer.py:6-22).
 *  yolo_upsample2_concat_bwd: da [n,h,w,ca] = bf16_rne(((f32(dy00) + f32(dy01)) + f32(dy10)) + f32(dy11)) over each 2x2 block of
 *    dy[..., :ca] (row-major), db [n,2h,2w,cb] = dy[..., ca:]; da or db may be NULL (not wanted), not both.
 *  YOLO_E_ARG before any launch for an empty shape, a channel count that is no positive multiple of 8, an act other than YOLO_ACT_NONE /
 *  YOLO_ACT_LEAKY01, a null or misaligned pointer (the bf16 maps and saved: 16 bytes; idx: 8). */
YOLO_API int yolo_bn_act_add_fwd(const void* z, const float* saved, const void* residual, void* y, void* y_preadd, long long pixels, int c,
                                 int act, yolo_stream_t s);
YOLO_API int yolo_spp_train_fwd(const void* x, void* y, void* idx, int n, int h, int w, int c, yolo_stream_t s);
YOLO_API int yolo_spp_bwd(const void* dy, const void* idx, void* dx, int n, int h, int w, int c, yolo_stream_t s);
YOLO_API int yolo_upsample2_concat_fwd(const void* a, const void* b, void* y, int n, int h, int w, int ca, int cb, yolo_stream_t s);
YOLO_API int yolo_upsample2_concat_bwd(const void* dy, void* da, void* db, int n, int h, int w, int ca, int cb, yolo_stream_t s);

/* ---- the max-pools of a training step of YOLOv3-tiny / LiteYOLOv3, with their backward; bf16 mode: csrc/pool_train.hip, one entry of
 *  csrc/batchnorm.hip and two of csrc/route.hip, DESIGN.md 3.6g.  The conventions of the block above: bf16, DENSE NHWC, c % 8 == 0, no
 *  atomics, no workspace, every output element written exactly once, every sum in a fixed order, no contraction.
 *  yolo_maxpool_train_fwd: the reference's MaxPool (models/yolo_base.py:60-66; inside ConvPoolBlock :69-80; nn.MaxPool2d(2, 2) at
 *    models/yolov3_tiny.py:26) of x [n,h,w,c].  stride 2: y [n,h/2,w/2,c] = MaxPool2d(2, 2)(x), floor: an odd last row or column is
 *    dropped; tap 2i + j of the window at (oy, ox) is the pixel (2oy + i, 2ox + j).  stride 1: y [n,h,w,c] = MaxPool2d(2, 1, padding=1,
 *    dilation=2)(x), the form MaxPool(2, 1) turns into (:62-64): tap 2i + j of the window at (y, x) is the diagonal neighbour
 *    (y - 1 + 2i, x - 1 + 2j), padded with -inf; h >= 2 and w >= 2 (on a smaller map a window can be all padding).  idx (uint8, y's
 *    shape) is the tap number 0..3 of the window's FIRST maximum among its in-bounds taps in row-major order: a later tap replaces the
 *    running maximum only when strictly greater (torch's rule, yolo_spp_train_fwd's).  A NaN is never greater: x must hold no NaN.
 *  yolo_maxpool_bwd: dx [n,h,w,c], every element written, from dy and idx (y's shape).  stride 2: dx[p] = dy[q] where idx[q] names p
 *    inside its own 2x2 block q, otherwise 0 (a dropped odd row or column: 0); a copy, nothing is summed.  stride 1: a gather over the
 *    four windows that can hold p, their centres q = p + (-1,-1), (-1,+1), (+1,-1), (+1,+1) in that order (p is their tap 3, 2, 1, 0):
 *    acc = 0; acc = acc + f32(dy[q]) where q is in bounds and idx[q] names p; dx[p] = bf16_rne(acc).
 *  yolo_bn_act_pool_fwd: yolo_bn_act_fwd's pass over z [n,h,w,c] with the stride-2 pool inside it (ConvPoolBlock as it trains): per tap
 *    t = bf16_rne(act(f32(z) scale + shift)); the four t of a block are compared as bf16 values under the first-maximum rule (the
 *    activated values, not z: gamma can be negative); y [n,h/2,w/2,c] and idx are written, the full-resolution activation never is.
 *    Bit-equal to yolo_bn_act_fwd followed by yolo_maxpool_train_fwd(stride 2).
 *  yolo_concat_upsample2_fwd / _bwd: yolo_upsample2_concat_* in the other order (models/yolov3_tiny.py:73):
 *    y [n,2h,2w,cb+ca] = cat([b, nearest_x2(a)], channel) of b [n,2h,2w,cb] and a [n,h,w,ca]; db = dy[..., :cb], da the same fixed 2x2
 *    sum of dy[..., cb:]; db or da may be NULL, not both.  The same kernels behind a channel offset.
 *  YOLO_E_ARG before any launch for an empty shape or empty output (h < 2 or w < 2), c % 8, a stride other than 1 or 2, an act other than
 *  YOLO_ACT_NONE / YOLO_ACT_LEAKY01, a null or misaligned pointer (the bf16 maps and saved: 16 bytes; idx: 8). */
YOLO_API int yolo_maxpool_train_fwd(const void* x, void* y, void* idx, int n, int h, int w, int c, int stride, yolo_stream_t s);
YOLO_API int yolo_maxpool_bwd(const void* dy, const void* idx, void* dx, int n, int h, int w, int c, int stride, yolo_stream_t s);
YOLO_API int yolo_bn_act_pool_fwd(const void* z, const float* saved, void* y, void* idx, int n, int h, int w, int c, int act, yolo_stream_t s);
YOLO_API int yolo_concat_upsample2_fwd(const void* b, const void* a, void* y, int n, int h, int w, int cb, int ca, yolo_stream_t s);
YOLO_API int yolo_concat_upsample2_bwd(const void* dy, void* db, void* da, int n, int h, int w, int cb, int ca, yolo_stream_t s);

/* ---- the layers of a training step of YOLOv3-tiny/SqueezeNet (SqueezeNet 1.1: biased convs with ReLU, MaxPool2d(3, 2, ceil_mode=True),
 *  the Fire module's concat; models/yolov3_tiny_squeeze.py), bf16 mode: csrc/fire_train.hip and three entries of csrc/conv_down_bwd.hip,
 *  DESIGN.md 3.6i.  The conventions of the two blocks above: bf16, DENSE NHWC, every channel count % 8 == 0, 16-byte accesses, no atomics,
 *  every output element written exactly once, every fp32 sum in a fixed order, no contraction; two runs give the same bits.
 *  ReLU in the conv backward: yolo_conv2d_bwd_pick / _workspace_bytes / _prepare / _weight / _data take YOLO_ACT_RELU beside none and
 *    LeakyReLU(0.1); yolo_conv2d_bwd_prepare then writes g = bf16_rne(fp32(dy) * (y > 0 ? 1 : 0)).  (yolo_conv2d_down_bwd_* and
 *    yolo_bn_act_* do not.)
 *  yolo_maxpool3s2_train_fwd: y [n,ho,wo,c] = MaxPool2d(3, 2, ceil_mode=True)(x) of x [n,h,w,c], pad 0: ho = ceil((h - 3) / 2) + 1 (= h / 2
 *    for h >= 2), wo likewise; h >= 2 and w >= 2.  Tap 3i + j of the window at (oy, ox) is the pixel (2oy + i, 2ox + j); with pad 0 the
 *    last window always starts inside the map, and its taps beyond the map (an even h or w) count as -inf.  idx (uint8, y's shape) is the
 *    tap number 0..8 of the window's FIRST maximum among its in-bounds taps in row-major order: a later tap replaces the running maximum
 *    only when strictly greater (torch's rule, yolo_maxpool_train_fwd's).  A NaN is never greater: x must hold no NaN.
 *  yolo_maxpool3s2_bwd: dx [n,h,w,c], every element written, from dy and idx (y's shape), as a gather: pixel (py, px) can sit in the
 *    windows oy in [ceil((py - 2) / 2), floor(py / 2)] and [0, ho), ox likewise - at most four.  acc = 0; for those windows in row-major
 *    (oy, ox) order: acc = acc + f32(dy[q]) where idx[q] == 3 (py - 2oy) + (px - 2ox); dx = bf16_rne(acc).
 *  yolo_fire_bwd_split: one pass over a Fire module's concat map y_cat [pixels][e1 + e3] (bf16, the forward's ReLU output) and its
 *    gradient dy (dense, the same shape, dy_dtype YOLO_DT_BF16 | YOLO_DT_F32): g1 [pixels][e1] = bf16_rne(f32(dy[p][c]) * (y_cat[p][c] > 0
 *    ? 1 : 0)) for c < e1, g3 [pixels][e3] the same for the other e3 channels.  Both are dense: the g operands yolo_conv2d_bwd_weight and
 *    yolo_conv2d_bwd_data take for the expand 1x1 and expand 3x3 convs.
 *  yolo_fire_bwd_join: g_s [pixels][sq] = bf16_rne((f32(d1) + f32(d3)) * (s_act > 0 ? 1 : 0)): d1, d3 the two expand convs' data
 *    gradients (bf16, as yolo_conv2d_bwd_data writes them), s_act the squeeze conv's ReLU output; g_s is the squeeze conv's g operand.
 *    Bit-equal to a bf16 add followed by yolo_conv2d_bwd_prepare (the add is an fp32 add rounded once, the factor is 0 or 1).
 *  yolo_conv2d_stem_bwd_*: the weight and bias gradient of the unpadded first layer Conv2d(cin, cout, 3, stride=2, padding=0) with ReLU,
 *    LeakyReLU(0.1) or no act: d is the FORWARD's descriptor (ksize 3, stride 2, pad 0, ho = (h - 3) / 2 + 1, wo likewise: an even map's
 *    last row and column are never read; h, w >= 3; cin % 8 == cout % 8 == 0, bf16 output).  g comes from yolo_conv2d_bwd_prepare on the
 *    stride-1 descriptor of the output map, as for the downsample.  dW[co][ci][kh][kw] = sum_{n,oh,ow} g[n,oh,ow,co] * x[n, 2 oh + kh,
 *    2 ow + kw, ci], db[co] = sum g: yolo_conv2d_down_bwd_weight's kernel, arithmetic and split order with pad 0.  _workspace_bytes:
 *    splits * cout * (9 cin + 1) * 4 (0 with a message for another descriptor); _pick: "wgrad<64x128,BK64,tr_b16,s2,p0> grid 1x1 splits
 *    43", no launch, no GPU.  There is no data gradient: the layer's input is the image.
 *  YOLO_E_ARG before any launch for an empty shape, h < 2 or w < 2 (the pool), a channel count that is no positive multiple of 8, a
 *  dy_dtype other than bf16 / fp32, a descriptor the entry does not take, a null or misaligned pointer (the maps: 16 bytes; idx: 8);
 *  YOLO_E_WORKSPACE for a small workspace. */
YOLO_API int yolo_maxpool3s2_train_fwd(const void* x, void* y, void* idx, int n, int h, int w, int c, yolo_stream_t s);
YOLO_API int yolo_maxpool3s2_bwd(const void* dy, const void* idx, void* dx, int n, int h, int w, int c, yolo_stream_t s);
YOLO_API int yolo_fire_bwd_split(const void* dy, int dy_dtype, const void* y_cat, void* g1, void* g3, long long pixels, int e1, int e3,
                                 yolo_stream_t s);
YOLO_API int yolo_fire_bwd_join(const void* d1, const void* d3, const void* s_act, void* g_s, long long pixels, int sq, yolo_stream_t s);
YOLO_API size_t yolo_conv2d_stem_bwd_workspace_bytes(const YoloConvDesc* d);
YOLO_API int yolo_conv2d_stem_bwd_pick(const YoloConvDesc* d, char* out, int out_len);
YOLO_API int yolo_conv2d_stem_bwd_weight(const void* x, const void* g, float* dw_oihw, float* dbias, void* workspace, size_t ws_bytes,
                                         const YoloConvDesc* d, yolo_stream_t s);

/* ---- the layers of a training step of MobileNetV2's inverted residual (torchvision's ConvBNReLU with ReLU6, dense and depthwise, and
 *  the linear bottleneck; models/yolov3_tiny_mobilenet.py:11-34), bf16 mode: three entries of csrc/batchnorm.hip and csrc/dw_train.hip,
 *  DESIGN.md 3.6j.  The conventions of the blocks above: bf16, DENSE NHWC, c % 8 == 0, a thread owns 8 channels (16 bytes) of a pixel, no
 *  atomics, every output element and every used workspace byte written exactly once, every sum in a fixed order, no contraction; two runs
 *  give the same bits.
 *  yolo_bn_clamp_fwd / yolo_bn_clamp_bwd: yolo_bn_act_fwd / yolo_bn_act_bwd with a clamp for the activation (ReLU6: lo 0, hi 6; ReLU: lo 0,
 *    hi +inf): a = f32(z) scale + shift; y = bf16_rne(min(max(a, lo), hi)).  Backward: slope = (a > lo && a < hi) ? 1 : 0 - zero AT both
 *    bounds, torch's hardtanh_backward rule -, ga = f32(dy) slope, and from there 3.6d's arithmetic (xh, the float64 sums B and G, dbeta,
 *    dgamma, c1, c2, g), workspace (yolo_bn_workspace_bytes), split rule (yolo_bn_pick) and NULL rules.  saved comes from
 *    yolo_bn_train_stats / yolo_bn_eval_stats as it is.  lo must be finite, hi finite or +inf, lo < hi.
 *  yolo_bn_add_rounded_fwd: the linear bottleneck's normalise pass with the block's add, act none: a = f32(z) scale + shift; y =
 *    bf16_rne(f32(bf16_rne(a)) + f32(residual)).  The normalised value is rounded to bf16 BEFORE the add, so the pass is bit-equal to
 *    yolo_bn_act_fwd(YOLO_ACT_NONE) followed by a bf16 add (an fp32 add rounded once) - unlike yolo_bn_act_add_fwd, which adds to the fp32
 *    value and rounds once.  The backward needs no entry: dy goes to yolo_bn_act_bwd(YOLO_ACT_NONE) and, unchanged, to the residual.
 *  The depthwise conv is Conv2d(c, c, 3, stride, 1, groups=c, bias=False), stride 1 or 2: x [n,h,w,c], z and g [n,ho,wo,c], ho = (h - 1) /
 *    stride + 1, wo likewise.  w is f32 [9][c], tap-major (yolo_dwconv3x3_fwd's layout; 16-byte aligned, it is read in vectors); the
 *    forward is yolo_dwconv3x3_fwd with act none and a zero bias.  The ops hand w over as bf16 values held in fp32, so that every fmaf
 *    below is an exact product and one fp32 add.
 *  yolo_dwconv3x3_bwd_data: dx [n,h,w,c], every element written, as a gather per INPUT pixel (ih, iw): acc = 0; for the taps (kh, kw) in
 *    row-major order for which oh = (ih + 1 - kh) / stride is integral and in [0, ho), ow likewise: acc = fmaf(f32(g[n,oh,ow]), w[3 kh +
 *    kw], acc); dx = bf16_rne(acc).
 *  yolo_dwconv3x3_bwd_weight: dw f32 [c][3][3] (the parameter's layout), dw[ch][kh][kw] = sum_{n,oh,ow} f32(g[n,oh,ow,ch]) * f32(x[n,
 *    stride oh + kh - 1, stride ow + kw - 1, ch]) over the in-bounds taps: fp32 products (exact: both factors are bf16 values), float64
 *    sums.  The output pixels are split over workgroups that write float64 partials [split][9][c] into the caller's workspace; one thread
 *    per (tap, channel) adds them in split order and rounds once to fp32.  Nothing in the workspace needs initialising.
 *  yolo_dwconv3x3_bwd_weight_workspace_bytes: splits * 9 * c doubles; 0 with a message for a shape the entries do not take.  The split
 *    count follows yolo_set_launch_cus.
 *  yolo_dwconv3x3_bwd_weight_pick: "dw_wgrad<3x128x2,s1> grid 157x1 passes 1 last 1" - kernel rows x pixel slots x chunk columns of a pass
 *    and the stride, grid (pixel splits x column tiles of 2048 channels), passes per split and those of the last split; no launch, no GPU.
 *  YOLO_E_ARG (YOLO_E_WORKSPACE for a small workspace) before any launch for an empty shape, c % 8, a stride other than 1 or 2, clamp
 *  bounds as above (a NaN included), pixels < 2 with batch statistics, a null or misaligned pointer (the maps, saved, w, ws: 16 bytes; the
 *  other fp32 vectors: 4). */
YOLO_API int yolo_bn_clamp_fwd(const void* z, const float* saved, void* y, long long pixels, int c, float lo, float hi, yolo_stream_t s);
YOLO_API int yolo_bn_clamp_bwd(const void* dy, int dy_dtype, const void* z, const float* saved, long long pixels, int c, float lo, float hi,
                               int batch_stats, void* g, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, yolo_stream_t s);
YOLO_API int yolo_bn_add_rounded_fwd(const void* z, const float* saved, const void* residual, void* y, long long pixels, int c, yolo_stream_t s);
YOLO_API int yolo_dwconv3x3_bwd_data(const void* g, const float* w, void* dx, int n, int h, int w_, int c, int stride, yolo_stream_t s);
YOLO_API size_t yolo_dwconv3x3_bwd_weight_workspace_bytes(int n, int h, int w_, int c, int stride);
YOLO_API int yolo_dwconv3x3_bwd_weight_pick(int n, int h, int w_, int c, int stride, char* out, int out_len);
YOLO_API int yolo_dwconv3x3_bwd_weight(const void* x, const void* g, float* dw, void* ws, size_t ws_bytes, int n, int h, int w_, int c,
                                       int stride, yolo_stream_t s);

/* ---- the depthwise conv of an expanding inverted residual on the expand conv's output, the batch norm and clamp of that output applied as
 *  the operand is loaded (csrc/dw_train.hip): the activation y between the two convs is never written.  zin [n,h,w,c] is
 *  the expand conv's bf16 output, saved_in f32 [4][c] = mean, invstd, scale, shift as yolo_bn_train_stats wrote it.  Both entries use ONE
 *  definition of the operand: inside the map a = fl(fl(f32(zin) * scale) + shift) - two fp32 roundings, no fma, yolo_bn_clamp_fwd's - and
 *  y = bf16_rne(fminf(fmaxf(a, lo), hi)); outside the map y = 0: the padding is a zero of y, NOT the clamp of a zero zin (clamp(shift)).
 *  yolo_dwconv3x3_bnin_fwd: z [n,ho,wo,c], bit-equal to yolo_dwconv3x3_fwd(y, w, zero bias, act none) on the materialised y: acc = 0, the
 *    taps row by row, one fmaf a tap, one rounding to bf16.  w as above (f32 [9][c]).
 *  yolo_dwconv3x3_bnin_bwd_weight: dw f32 [c][3][3], bit-equal to yolo_dwconv3x3_bwd_weight(y, g, ..): the same split rule, workspace
 *    (yolo_dwconv3x3_bwd_weight_workspace_bytes), pick (yolo_dwconv3x3_bwd_weight_pick) and finalize.
 *  The data gradient needs no entry: yolo_dwconv3x3_bwd_data gives the gradient with respect to y, yolo_bn_clamp_bwd takes it from there
 *  on zin and saved_in.  YOLO_E_ARG / YOLO_E_WORKSPACE before any launch as for the entries above; lo, hi as for yolo_bn_clamp_fwd; the
 *  maps, saved_in, w and ws 16-byte aligned. */
YOLO_API int yolo_dwconv3x3_bnin_fwd(const void* zin, const float* saved_in, float lo, float hi, const float* w, void* z, int n, int h, int w_,
                                     int c, int stride, yolo_stream_t s);
YOLO_API int yolo_dwconv3x3_bnin_bwd_weight(const void* zin, const float* saved_in, float lo, float hi, const void* g, float* dw, void* ws,
                                            size_t ws_bytes, int n, int h, int w_, int c, int stride, yolo_stream_t s);

/* ---- The layers of a training step of YOLOv3-tiny/ShuffleNetV2 that are no conv (models/yolov3_tiny_shuffle.py), bf16 mode:
 *  csrc/shuffle_train.hip, DESIGN.md 3.6l.  The conventions of the blocks above: bf16 NHWC, every physical channel count % 8 == 0, a
 *  thread per 8-channel chunk of a pixel, no atomics, no LDS, no workspace, every output element written exactly once, every fp32 sum in a
 *  fixed order, no contraction; two runs give the same bits.  The dense ConvBNReLU needs no entry: yolo_bn_clamp_fwd / _bwd with lo 0 and
 *  hi +inf are ReLU.
 *  yolo_maxpool3s2p1_train_fwd: y [n,ho,wo,c] = MaxPool2d(3, 2, padding=1)(x) of the dense x [n,h,w,c]: ho = (h - 1) / 2 + 1, wo likewise;
 *    any h, w >= 1.  Tap 3i + j of the window at (oy, ox) is the pixel (2oy - 1 + i, 2ox - 1 + j); a tap outside the map is never a
 *    candidate (it acts as -inf, not as 0: a map of negative values pools to negative values); tap 4, the centre, is always inside.  idx
 *    (uint8, y's shape) is the tap number 0..8 of the window's FIRST maximum among its in-bounds taps in row-major order: a later tap
 *    replaces the running maximum only when strictly greater (torch's rule, yolo_maxpool3s2_train_fwd's).  A NaN is never greater.
 *  yolo_maxpool3s2p1_bwd: dx [n,h,w,c], every element written, from dy and idx (y's shape), as a gather: pixel (py, px) can sit in the
 *    windows oy in [ceil((py - 1) / 2), floor((py + 1) / 2)] and [0, ho), ox likewise - at most four.  acc = 0; for those windows in
 *    row-major (oy, ox) order: acc = acc + f32(dy[q]) where idx[q] == 3 (py - 2oy + 1) + (px - 2ox + 1); dx = bf16_rne(acc).
 *  yolo_channel_shuffle2_bwd: the inverse of yolo_channel_shuffle2_fwd on its two-slot layout.  dy, da and db are channel views
 *    (c_total, c_offset) of NHWC buffers: dy 2 c_slot channels wide, da and db c_slot.  Logical channel j of dy (j < 2 half) sits at
 *    physical (j / half) c_slot + j % half.  For q < half: da[q] = dy_logical[2q], db[q] = dy_logical[2q + 1]; the channels [half, c_slot)
 *    of da and db are written as zero; the pad channels of dy are never read.  Any 1 <= half <= c_slot, c_slot % 8 == 0; dy is read one
 *    channel at a time (any view inside its buffer), the views of da and db start and end on 8 channels.  da or db may be null: that
 *    output is not written (not both).
 *  YOLO_E_ARG before any launch for an empty shape, a channel count that is no positive multiple of 8, half outside [1, c_slot], a view
 *  that leaves its buffer or (da, db) is not 8-channel aligned, a null or misaligned pointer (the maps: 16 bytes; idx: 8; dy of the
 *  shuffle: 2). */
YOLO_API int yolo_maxpool3s2p1_train_fwd(const void* x, void* y, void* idx, int n, int h, int w, int c, yolo_stream_t s);
YOLO_API int yolo_maxpool3s2p1_bwd(const void* dy, const void* idx, void* dx, int n, int h, int w, int c, yolo_stream_t s);
YOLO_API int yolo_channel_shuffle2_bwd(const void* dy, void* da, void* db, int n, int h, int w, int half, int c_slot, int dy_c_total,
                                       int dy_c_offset, int da_c_total, int da_c_offset, int db_c_total, int db_c_offset, yolo_stream_t s);

/* First layer fused with the input packing: x is the caller's f32 NCHW batch [n,cin_real,h,w] (cin_real <= 8),
 * w_packed / bias as for yolo_conv2d_fwd with d->cin = 8; 3x3 / pad 1, bf16 NHWC output: stride 1 with cout 16 or 32
 * (Darknet), or stride 2 with cout 32 (MobileNetV2's first layer). */
YOLO_API int yolo_conv1_nchw_f32_fwd(const float* x_nchw, int cin_real, const void* w_packed, const float* bias,
                                     void* y, const YoloConvDesc* d, yolo_stream_t s);
/* same, followed by MaxPool2d(2, 2) (the first ConvPoolBlock of YOLOv3-tiny, models/yolo_base.py:69-80 with
 * yolov3_tiny.py:26): y_pooled is the bf16 NHWC view of the POOLED map [n, h/2, w/2, ...]; d still describes the
 * conv (ho = h, wo = w).  cout 16 or 32. */
YOLO_API int yolo_conv1_pool_nchw_f32_fwd(const float* x_nchw, int cin_real, const void* w_packed, const float* bias,
                                          void* y_pooled, const YoloConvDesc* d, yolo_stream_t s);

/* host-side helper (CPU): OIHW f32 [cout,cin_w,k,k] -> packed bf16 (round-to-nearest-even);
 * cin_w <= cin (extra input channels, e.g. the RGB->8 pad, get zero weights). */
YOLO_API int yolo_pack_conv_weight_f32(const float* w_oihw, int cout, int cin_w, int ksize, int cin,
                              int cout_pad, int kpad, uint16_t* out);

/* ---- 3x3 / stride 1 / pad 1 ConvBlock with 16 or 32 input channels and 32 or 64 output channels, optionally followed by
 *  MaxPool2d(2, 2): the second and third ConvPoolBlock of YOLOv3-tiny (models/yolo_base.py:69-80, yolov3_tiny.py:26-29)
 *  in ONE launch; with pool != 0 y is the bf16 NHWC view of the POOLED map [n, h/2, w/2, ...] and the full-resolution
 *  conv output is never written.  x: bf16 NHWC view, w_packed / bias as for yolo_conv2d_fwd, d describes the conv. */
YOLO_API int yolo_conv3x3_pool_supported(int cin, int cout);
YOLO_API int yolo_conv3x3_pool_fwd(const void* x, const void* w_packed, const float* bias, void* y, const YoloConvDesc* d,
                                   int pool, yolo_stream_t s);

/* ---- depthwise 3x3 conv + bias + act (MobileNetV2 inverted residual; torchvision, see
 *      models/yolov3_tiny_mobilenet.py:11-34).  w: f32 [9][c] tap-major, bias f32 [c].  act: any YOLO_ACT_*, applied in fp32 to
 *      the sum before the one narrowing to bf16, with the operations of yolo_dwconv_fwd; a value outside the enum is YOLO_E_ARG. */
YOLO_API int yolo_dwconv3x3_fwd(const void* x, const float* w, const float* bias, void* y, int n, int h, int w_,
                       int c, int in_c_total, int in_c_offset, int ho, int wo, int out_c_total,
                       int out_c_offset, int stride, int act, yolo_stream_t s);

/* ---- depthwise k x k conv (k = 3 or 5) + bias + act with an explicit leading pad (rows above / columns left of the image);
 *      windows that hang over the bottom / right edge read zeros, so TensorFlow "same" padding (efficientnet_pytorch 0.2.0
 *      Conv2dSamePadding: stride 2 on an even map pads 0 + 1 for k = 3, 1 + 2 for k = 5) is pad = pad_total / 2 with the caller's
 *      ho x wo = ceil(h / stride) x ceil(w / stride).  EfficientNet-B0's MBConvBlock._depthwise_conv behind
 *      models/yolov3_tiny_efficient.py:22-45.  w: f32 [k*k][c] tap-major, bias f32 [c]. */
YOLO_API int yolo_dwconv_fwd(const void* x, const float* w, const float* bias, void* y, int n, int h, int w_, int c,
                             int in_c_total, int in_c_offset, int ho, int wo, int out_c_total, int out_c_offset, int ksize,
                             int stride, int pad, int act, yolo_stream_t s);

/* ---- squeeze-and-excitation of an MBConvBlock (efficientnet_pytorch 0.2.0 model.py, used through
 *      models/yolov3_tiny_efficient.py:47-56): y = x * sigmoid(W2 swish(W1 mean_hw(x) + b1) + b2), per image and channel.
 *      x, y: bf16 NHWC views of c channels (y may be x); w1: f32 [squeeze][c] (= _se_reduce.weight), b1 f32 [squeeze],
 *      w2: f32 [squeeze][c] (= _se_expand.weight TRANSPOSED: lanes read consecutive channels), b2 f32 [c];
 *      workspace: yolo_se_workspace_bytes(n, c) bytes (pooled means, scales and the pooling pass's partial sums, fp32;
 *      the means stay in its first n*c floats). */
YOLO_API size_t yolo_se_workspace_bytes(int n, int c);
YOLO_API int yolo_se_fwd(const void* x, void* y, int n, int h, int w, int c, int in_c_total, int in_c_offset, int out_c_total,
                         int out_c_offset, const float* w1, const float* b1, const float* w2, const float* b2, int squeeze,
                         void* workspace, size_t ws_bytes, yolo_stream_t s);

/* ---- ShuffleNetV2's channel_shuffle(cat(a, b), groups = 2) (torchvision shufflenetv2, used by
 *  models/yolov3_tiny_shuffle.py:13-47): a and b are bf16 NHWC views holding `half` logical channels each in slots of
 *  c_slot physical channels (zero beyond `half`); y gets logical channel j = (a, b)[j % 2][j / 2] in the same two-slot
 *  layout: logical [0, half) at [0, ...), logical [half, 2 half) at [c_slot, ...); its pad channels are left alone. */
YOLO_API int yolo_channel_shuffle2_fwd(const void* a, const void* b, void* y, int n, int h, int w, int half, int c_slot,
                                       int a_c_total, int a_c_offset, int b_c_total, int b_c_offset, int y_c_total,
                                       int y_c_offset, yolo_stream_t s);

/* ---- MaxPool (models/yolo_base.py:60-66): -inf padding; the (2,1) special is pad 1, dilation 2. */
YOLO_API int yolo_maxpool_fwd(const void* x, void* y, int n, int h, int w, int c, int in_c_total, int in_c_offset,
                     int ho, int wo, int out_c_total, int out_c_offset, int ksize, int stride, int pad,
                     int dilation, yolo_stream_t s);

/* ---- SPP pyramid (models/yolov3_spp.py:75-77,129): buf is the [n,h,w,4c] concat buffer whose
 *      slice [3c,4c) already holds x; writes pool5 -> [0,c), pool9 -> [c,2c), pool13 -> [2c,3c). */
YOLO_API int yolo_spp_fwd(void* buf, int n, int h, int w, int c, yolo_stream_t s);

/* ---- one Darknet residual unit in one launch (models/yolov3_spp.py:17-32: ConvBlock 1x1 C->C/2, ConvBlock 3x3
 *  C/2->C, Add):  y = x + act(conv3x3(act(conv1x1(x,W1)+b1), W2) + b2);  y_preadd (optional) = the 3x3 output
 *  before the add (the reference returns it from the last unit of a DownSample stage).
 *  d describes the 3x3/s1/p1 conv: cin = C/2, cout = C, kpad/cout_pad = packing of W2; its INPUT view fields
 *  (in_c_total/in_c_offset) describe x (C channels); res_* fields are ignored.  W1 is packed like any 1x1
 *  ([cout_pad1][kpad1]).  y must not alias x.  yolo_resunit_supported(): C in {64,128,256} on maps >= 80x80 that
 *  tile well by 16x16; other shapes use two yolo_conv2d_fwd calls.
 *  Operand sizes (see YoloConvDesc): x - the residual too - and the weights below 0xF0000000 bytes, else YOLO_E_UNSUPPORTED; a y or
 *  a pre-add copy of 0xF0000000 bytes and more hands the unit from the 20-pixel-wide tile kernels (resunit64_t20, resunit_t20w) to
 *  the 16x16-tile ones (resunit64, resunit), which write through 64-bit pointers. */
YOLO_API int yolo_resunit_supported(int c, int h, int w);
/** Which kernel yolo_resunit_fwd launches for a C-channel unit on n maps of h x w: 0 not supported, 1 the generic 16x16-tile kernel
 *  (slower than the two-launch path above C = 64: a planner should not fuse there), 2 the persistent 64-channel kernel, 3 the
 *  20-pixel-wide tile kernels (conv_resunit_t20.hip).  No launch, works without a GPU. */
YOLO_API int yolo_resunit_form(int c, int n, int h, int w);
/** The kernel + grid yolo_resunit_fwd would launch for d (the unit's 3x3) under the current tuning, in the style of yolo_conv2d_pick:
 *  "resunit64_t20<...> grid N", "resunit_t20w<C 128, ...> grid N", "resunit64<..., persistent> grid N" or "resunit<C 128, ...> grid N".
 *  Runs the checks of yolo_resunit_fwd that need no pointer; no launch, works without a GPU. */
YOLO_API int yolo_resunit_pick(const YoloConvDesc* d, int has_preadd, char* out, int out_len);
YOLO_API int yolo_resunit_fwd(const void* x, const void* w1_packed, const float* b1, const void* w2_packed,
                              const float* b2, void* y, void* y_preadd, const YoloConvDesc* d, int kpad1,
                              int cout_pad1, yolo_stream_t s);

/* ---- the Darknet stem in one launch (models/yolov3_spp.py:98 ConvBlock 3x3/s1 cin->32, then DownSample's
 *  ConvBlock 3x3/s2 32->64, :26-27):  y = act(conv_s2(act(conv_s1(x,W1)+b1), W2)+b2), x = float32 NCHW
 *  [n,cin_real,h,w] (1..8 channels), y = bf16 NHWC view at h/2 x w/2.  The 32-channel intermediate (the
 *  largest activation of the network) stays in LDS.  d describes the stride-2 conv (h,w = input size,
 *  cin 32, cout 64, kpad = packing of W2); W1 is packed as for yolo_conv1_nchw_f32_fwd (cin = 8, kpad1 >= 80).
 *  Operand sizes: stem2 addresses x and y with 32-bit offsets; from 0xF0000000 bytes of x (n * 3 * h * w * 4) or of y
 *  (n * ho * wo * out_c_total * 2) on the one-role kernel "stem<...,CIN 3,...>" runs instead, on 64-bit pointers. */
YOLO_API int yolo_stem_supported(int cin_real, int c1, int c2, int h, int w);
/** The kernel + grid yolo_stem_fwd would launch under the current tuning: "stem2<leaky,8x16 outputs> grid N" (3 input channels) or
 *  "stem<leaky,CIN 0,16x16 outputs> grid N" (CIN 3: three channels under knob 6 or beyond 32-bit offsets).  Runs the checks of
 *  yolo_stem_fwd that need no pointer; no launch, works without a GPU. */
YOLO_API int yolo_stem_pick(int cin_real, const YoloConvDesc* d, char* out, int out_len);
YOLO_API int yolo_stem_fwd(const float* x_nchw, int cin_real, const void* w1_packed, const float* b1, int kpad1,
                           const void* w2_packed, const float* b2, void* y, const YoloConvDesc* d, yolo_stream_t s);

/* ---- one MobileNetV2 inverted-residual block in one launch (torchvision InvertedResidual as the reference uses it,
 *  models/yolov3_tiny_mobilenet.py:14-46):  y = [x +] proj1x1(relu6(dw3x3_stride(relu6(expand1x1(x))))), BN folded.
 *  The expanded tensor (6x the input) and the depthwise output stay on the CU.  x, y: bf16 NHWC views.
 *  ce = hidden rounded up to 32, cout_pad = cout rounded up to 16, dstride = yolo_mbconv_dstride(ce) bytes.
 *    w_exp  bf16 [ce][48]: row = hidden channel, the first cin entries real, the rest zero (NULL: the block has
 *           no expand conv, hidden == cin);  b_exp f32 [ce]
 *    w_dw   f32 [9][ce] tap-major, b_dw f32 [ce]  (zero beyond hidden)
 *    w_proj bf16 [cout_pad][dstride/2]: row = output channel, the first hidden entries real;  b_proj f32 [cout_pad]
 *  has_res: y = x + ... (stride 1, cin == cout).
 *  yolo_mbconv_supported() returns the FORM that covers a block, which decides the weight images:
 *    1  cin <= 32, hidden <= 192, cout <= 64 (the blocks on the 208..52 maps of a 416x416 input): the images above;
 *    2  the wide blocks (csrc/conv_mbwide.hip: the hidden dimension streamed in chunks of 64 channels): cin a multiple of 32
 *       in 64..160 (stride 2: ..96), hidden a multiple of 64, cout <= 320, expand conv present.  Plain row-major matrices,
 *       read through buffer descriptors:  w_exp bf16 [hidden][cin], b_exp f32 [hidden], w_dw f32 [9][hidden], b_dw f32 [hidden],
 *       w_proj bf16 [cout_pad][hidden], b_proj f32 [cout_pad];
 *    0  not covered: the block runs as yolo_conv2d_fwd + yolo_dwconv3x3_fwd + yolo_conv2d_fwd.
 *  Operand sizes: forms 1 (tile and strip) use 64-bit pointers and have no byte limit; form 2 addresses x with a signed 32-bit
 *  count: from 2^31 bytes behind the x view (n * h * w * in_c_total * 2) on it returns YOLO_E_UNSUPPORTED ("... or a tensor of
 *  2 GB"). */
typedef struct YoloMbconvDesc {
  int32_t n, h, w, cin, in_c_total, in_c_offset, hidden, cout, out_c_total, out_c_offset, stride, has_expand, has_res, _pad;
} YoloMbconvDesc;
YOLO_API int yolo_mbconv_dstride(int ce);
YOLO_API int yolo_mbconv_supported(int cin, int hidden, int cout, int stride);
/** The kernel + grid yolo_mbconv_fwd would launch under the current tuning: "mbconv<S 1,8x8,expand,512 threads> grid N" (tile form),
 *  "mbstrip<S 1,expand,8 rows x 26> grid N" (knob 4 bit kMbStripForm, where the strip form can hold the block) or
 *  "mbwide<S 1,13x13,512 threads,MC 4> grid N".  Runs the checks of yolo_mbconv_fwd that need no pointer; no launch, works without
 *  a GPU. */
YOLO_API int yolo_mbconv_pick(const YoloMbconvDesc* d, char* out, int out_len);
YOLO_API int yolo_mbconv_fwd(const void* x, const void* w_exp, const float* b_exp, const float* w_dw, const float* b_dw,
                             const void* w_proj, const float* b_proj, void* y, const YoloMbconvDesc* d, yolo_stream_t s);

/* ---- YOLOLayer.forward eval branch (models/yolo_layer.py:57-69,90-111).
 *  head: f32 NHWC [bs,ny,nx,head_c_total], channel a*(5+nc)+k.
 *  io:   f32 [bs, io_rows_total, 5+nc]; this head fills rows [io_row_offset, +na*ny*nx).
 *  p:    f32 [bs,na,ny,nx,5+nc] or NULL.
 *  anchors_px: host array of na*2 floats (pixels).  stride_px = img_size / max(nx,ny). */
YOLO_API int yolo_decode_fwd(const float* head, int head_c_total, const float* anchors_px, int na, int nc, int bs,
                    int ny, int nx, float stride_px, float* io, int io_rows_total, int io_row_offset,
                    float* p, yolo_stream_t s);

/* ---- detection head in one launch: head conv (1x1 or 3x3, stride 1; bias; act none for the plain heads of
 *  yolov3_tiny.py:38,42, leaky for the ConvBlock heads of yolov3_spp.py:104) with YOLOLayer.forward's eval branch
 *  as its epilogue: p[bs,na,ny,nx,5+nc] = the raw head values, io rows = the decoded ones (see yolo_decode_fwd).
 *  The NHWC head tensor is never materialised.  d = the head conv (cout = na*(5+nc) <= 256; its output view is
 *  ignored).  yolo_head_decode_supported(): na <= 4, 5+nc <= 128; other heads use yolo_conv2d_fwd + yolo_decode_fwd. */
YOLO_API int yolo_head_decode_supported(int cout, int na, int nc);
/* The kernel instance + grid a head op would launch (yolo_conv2d_pick for yolo_head_decode_fwd / - filter != 0 - yolo_head_decode_filter_fwd):
 * "igemm<64x256,1x8 waves,BK64,2 stages,32x32x16,decode> grid 3200"; no launch, no GPU. */
YOLO_API int yolo_head_decode_pick(const YoloConvDesc* d, int na, int nc, int filter, char* out, int out_len);
YOLO_API int yolo_head_decode_fwd(const void* x, const void* w_packed, const float* bias, const YoloConvDesc* d,
                                  const float* anchors_px, int na, int nc, float stride_px, float* io,
                                  int io_rows_total, int io_row_offset, float* p, yolo_stream_t s);

/* ---- non_max_suppression, 'MERGE' style (utils/utils.py:200-293; xywh2xyxy :46-60, bbox_iou :63-96).
 *  pred: f32 [bs,rows,5+nc].  If mutate_conf != 0 column 4 is overwritten with obj*max_cls like the
 *  reference (:213); otherwise pred is read-only.
 *  out_dets [bs,cap,7] (x1,y1,x2,y2,conf,cls_conf,cls), out_idx [bs,cap] = pivot row of each output,
 *  out_count [bs].  Rows are ordered by conf descending (ties: class, then pivot order).
 *  cap >= min(rows, nc*max_per_class) guarantees nothing is dropped; if an image would exceed cap,
 *  out_count holds the true count and only the first cap rows are written.
 *  Staging rule: inside the workspace every image has a staging area of min(rows, nc*128) rows (128 = the largest max_per_class),
 *  which is every row the class loops can emit, so no kept row is ever lost before the final order - also when an image keeps more
 *  than 8192 rows (nc*max_per_class > 8192), in which case the final sort runs in the workspace instead of LDS. */
YOLO_API size_t yolo_nms_workspace_bytes(int bs, int rows, int nc);
YOLO_API int yolo_nms_merge(float* pred, int bs, int rows, int nc, float conf_thres, float nms_thres, float min_wh,
                   int max_per_class, int mutate_conf, float* out_dets, int32_t* out_idx,
                   int32_t* out_count, int cap, void* workspace, size_t workspace_bytes, yolo_stream_t s);

/* ---- the other suppression styles of the same function (utils/utils.py:240: nms_style = 'OR' (default) | 'AND' | 'MERGE' | 'SOFT').
 *  The reference hard-codes 'MERGE'; yolo_nms_styled takes the style as an argument and yolo_nms_merge is
 *  yolo_nms_styled(..., YOLO_NMS_MERGE, s).  Shared by all styles, unchanged: conf product and filters (:212-218), xywh2xyxy (:231),
 *  the sort by conf (:237), the per-class loop over ascending class ids (:241), a class of ONE row is kept as it is (:244-246, the
 *  length before the cap), only the first max_per_class rows of a class take part (:247-250), the final order (:291).  Per class:
 *    YOLO_NMS_MERGE (:266-275)  the head's box becomes the conf-weighted mean of the rows with iou > nms_thres, which leave with it.
 *    YOLO_NMS_OR    (:253-259)  greedy hard NMS: emit the head, keep the rows with iou < nms_thres (iou == nms_thres is removed).
 *    YOLO_NMS_AND   (:260-265)  as OR, but the head is emitted only if its largest iou with the remaining rows is > 0.5 (a
 *                               constant of the reference, not nms_thres); the last remaining row of a class is never emitted, so
 *                               an image may lose every row (out_count 0).
 *    YOLO_NMS_SOFT  (:277-287)  nothing is removed: row j is emitted with conf_j * prod_{i<j} exp(-iou(i,j)^2 / 0.5) (factors in
 *                               ascending i, one fp32 multiply each; rows are not re-sorted inside the loop); the final order uses
 *                               the decayed conf; class_conf (column 5) is untouched.  expf is the one step that is not bit-defined.
 *  In OR, AND and SOFT the box columns of an output row are the input row's corners, unchanged, and out_idx is that row.
 *  nms_thres >= 1 is refused for MERGE only (its loop would not terminate).  An unknown style returns YOLO_E_ARG.
 *  The one-call pipeline step (YoloPipeStep / yolo_pipeline_step) has no style field and stays MERGE-only. */
enum { YOLO_NMS_MERGE = 0, YOLO_NMS_OR = 1, YOLO_NMS_AND = 2, YOLO_NMS_SOFT = 3 };
YOLO_API int yolo_nms_styled(float* pred, int bs, int rows, int nc, float conf_thres, float nms_thres, float min_wh,
                   int max_per_class, int mutate_conf, float* out_dets, int32_t* out_idx,
                   int32_t* out_count, int cap, void* workspace, size_t workspace_bytes, int style, yolo_stream_t s);

/* ---- the compact form of the same post-process (round 4): detect() = non_max_suppression(forward(x)[0]) without ever writing io.
 *  The head convs filter their own decoded rows in their epilogue (yolo_head_decode_filter_fwd: the row filter of utils.py:212-218,
 *  operation for operation what yolo_nms_merge's first kernel does on a materialised io) and leave, in the workspace, ONE sort key
 *  per io row (~0 for a row that does not survive) plus a 32-byte record (x, y, w, h, class score) for the survivors; no atomics and
 *  nothing to initialise - every io row belongs to exactly one head.  yolo_nms_merge_compact gathers the keys and runs the same
 *  sort / MERGE / final order.  Saves the io store and its read-back (2 x 274 MB per 32 SPP-640 images) and one launch; the
 *  detections are bit-equal to yolo_nms_merge on the io the plain heads would have written.  Order per batch, on one stream or on
 *  ordered streams:  every head's yolo_head_decode_filter_fwd (together they must cover all `rows`) -> yolo_nms_merge_compact. */
YOLO_API size_t yolo_nms_compact_workspace_bytes(int bs, int rows, int nc);
YOLO_API int yolo_head_decode_filter_fwd(const void* x, const void* w_packed, const float* bias, const YoloConvDesc* d,
                                         const float* anchors_px, int na, int nc, float stride_px, int io_rows_total,
                                         int io_row_offset, float conf_thres, float min_wh, void* workspace, size_t workspace_bytes,
                                         float* p, yolo_stream_t s);
YOLO_API int yolo_nms_merge_compact(void* workspace, size_t workspace_bytes, int bs, int rows, int nc, float nms_thres,
                                    int max_per_class, float* out_dets, int32_t* out_idx, int32_t* out_count, int cap,
                                    yolo_stream_t s);
/* ... with the style of yolo_nms_styled (yolo_nms_merge_compact = YOLO_NMS_MERGE); the head epilogues' row filter is style-independent */
YOLO_API int yolo_nms_styled_compact(void* workspace, size_t workspace_bytes, int bs, int rows, int nc, float nms_thres,
                                     int max_per_class, float* out_dets, int32_t* out_idx, int32_t* out_count, int cap,
                                     int style, yolo_stream_t s);

/* ---- compute_loss / build_targets / wh_iou (utils/utils.py:99-197) on the raw head tensors p of `io, p = model(x)`: the forward
 *  value (yolo_loss_fwd) and its gradient with respect to p (yolo_loss_bwd); nothing else has a gradient (csrc/loss.hip).
 *  Geometry, all HOST arrays: na / ny / nx [nl] per YOLO layer (nl <= 4, na <= 8) and anchor_vec = the layers' anchor_vec values
 *  exactly as the Python layer holds them (anchors / stride, yolo_layer.py:109; never recomputed here), (w, h) pairs, layers back to
 *  back: 2 * sum(na) floats.  n_grids of layer l is (nx[l], ny[l]) (yolo_layer.py:111).
 *  targets: device f32 [nt, 6] = image, class, x, y, w, h (x..h normalised to the image); nt == 0 is legal (targets may be NULL).
 *  p: HOST array of nl device pointers, p[l] = f32 [bs, na, ny, nx, 5 + nc] contiguous.
 *  Target assignment per (layer, target), every step one IEEE fp32 operation in the reference's order: gwh = wh * n_grids (:169),
 *  wh_iou against each anchor (:116-121), the FIRST maximum (:172), kept iff iou > iou_thresh (:177), b / class / gi / gj by
 *  truncation (:181-183), txy = gxy - floor(gxy) (:187), twh = logf(gwh / anchor) (:190).  A kept target with image outside [0, bs),
 *  class outside [0, nc), gi outside [0, nx), gj outside [0, ny) or a NaN among them - the reference raises an IndexError there - is
 *  NOT assigned; its record is flagged and it is counted in status[0].
 *  workspace (yolo_loss_workspace_bytes; caller-owned, nothing in it needs initialising) starts with the records:
 *    int32 [nl][max(nt, 1)][12] = valid, b, a, gj, gi, class, txy[2], twh[2] (float bits), flagged, 0 - slot order is target order;
 *  the tconf map (one byte per row of every layer, cleared by every call), the float64 partial sums of the objectness pass and four
 *  float64 terms per record follow.
 *  yolo_build_targets_fwd: the map and the records (for callers who want the assignment).
 *  yolo_loss_fwd: the same, then the loss (:137-155).  gains: HOST f32 [4] = k * h['xy_loss'], k * h['wh_loss'], k * h['cls_loss'],
 *  k * h['conf_loss'] with k = bs (:136).  class_weight: device f32 [nc] or NULL (CrossEntropyLoss(weight=), :130; ignored for
 *  nc == 1, where the class term is BCEWithLogits against the class INDEX, :152).  out: device f32 [5] = lxy, lwh, lconf, lcls, loss
 *  (:157).  status: device int32 [1 + nl] = flagged targets, then the kept targets of each layer.
 *  No atomics: terms in fp32, sums in float64 in an order fixed by the shapes - bit-identical from run to run. */
YOLO_API size_t yolo_loss_workspace_bytes(int nl, const int32_t* na, const int32_t* ny, const int32_t* nx, int bs, int nt);
YOLO_API int yolo_build_targets_fwd(const float* targets, int nt, int nl, const int32_t* na, const int32_t* ny, const int32_t* nx,
                                    const float* anchor_vec, int bs, int nc, float iou_thresh, void* workspace,
                                    size_t workspace_bytes, yolo_stream_t s);
YOLO_API int yolo_loss_fwd(const float* const* p, const float* targets, int nt, int nl, const int32_t* na, const int32_t* ny,
                           const int32_t* nx, const float* anchor_vec, int bs, int nc, float iou_thresh, const float* gains,
                           const float* class_weight, void* workspace, size_t workspace_bytes, float* out, int32_t* status,
                           yolo_stream_t s);
/*  yolo_loss_bwd: d loss / d p of the loss above, a first derivative that stops at p.  It takes the inputs of yolo_loss_fwd (not
 *  its results out and status, which it neither reads nor writes) and
 *    grad_loss  device f32 [1]: the upstream gradient of loss, read on the device;
 *    grad_p     HOST array of nl device pointers, grad_p[l] = f32 of the shape of p[l], contiguous, 16-byte aligned.
 *  EVERY element of every grad_p[l] is written, whatever it held.  With G = *grad_loss, n_l = the kept valid targets of layer l and
 *  rows_l = bs na ny nx: word 4 of every row = G gains[3] / rows_l * (sigmoid(x4) - tconf); in the cell of a kept valid target, summed
 *  over the targets that share the cell in target order (the reference gathers the cell once per target): words 0-1
 *  G gains[0] (s - txy) s (1 - s) / n_l with s = sigmoid(x); words 2-3 G gains[1] (x - twh) / n_l; class word k, nc > 1,
 *  G gains[2] w_c (softmax_k - [k == c]) / sum over the layer's targets of w_c (w = class_weight or 1); nc == 1
 *  G gains[2] (sigmoid(x5) - c) / n_l; every other element +0.0.  Flagged targets are left out as in the forward.
 *  Stateless: it runs the memset and the assignment itself, in the same workspace layout (yolo_loss_workspace_bytes), and needs nothing
 *  an earlier call left there; no allocation, no host synchronisation, no retained pointer.  No atomics: bit-identical from run to
 *  run, cells shared by any number of targets included.  G is multiplied into the gain first. */
YOLO_API int yolo_loss_bwd(const float* const* p, const float* targets, int nt, int nl, const int32_t* na, const int32_t* ny,
                           const int32_t* nx, const float* anchor_vec, int bs, int nc, float iou_thresh, const float* gains,
                           const float* class_weight, void* workspace, size_t workspace_bytes, const float* grad_loss,
                           float* const* grad_p, yolo_stream_t s);

/* ---- COCO bbox evaluation (what utils/utils.py:330-354 asks of pycocotools: COCOeval.evaluate / accumulate, and the sums of the
 *  reference's "Mean IOU") in float64, one IEEE operation per step in pycocotools' order (csrc/coco_eval.hip).
 *  The parameter COUNTS are fixed: 10 IoU thresholds, 4 area ranges, 101 recall thresholds, 3 maxDets; their VALUES come from the
 *  caller (numpy): iou_thrs device f64 [10], area_rng device f64 [4][2], rec_thrs device f64 [101], max_dets HOST int32 [3]
 *  ascending, eps = np.spacing(1).
 *  Groups: g = image index * n_cat + category index, images and categories in ascending id order.  dt_off / gt_off: device int32
 *  [n_img * n_cat + 1], first element of each group (the last entry is n_dt / n_gt).  Boxes are (x, y, w, h).
 *  Detections (dt_box f64 [n_dt, 4]) stand group by group and, inside a group, in EVALUATION ORDER: descending score, ties in the
 *  order of the results list, cut to the first max_dets[2].  GTs (gt_box f64 [n_gt, 4], gt_area f64 [n_gt], gt_crowd u8 [n_gt]) stand
 *  group by group in annotation order.  max_gt = the largest GT count of a group (the caller knows it): above yolo_coco_max_gt()
 *  the call fails with YOLO_E_UNSUPPORTED before anything is launched; a group whose offsets nevertheless exceed the cap is skipped
 *  and counted in status[0] (device int32 [1]) - never truncated.
 *  yolo_coco_match_fwd: IoU (bbIou), then evaluateImg's greedy matching per group x area range a x threshold t.  Writes per
 *    detection dt_match / dt_ignore (device u64 [n_dt]: bit a * 10 + t), npig (device int32 [n_cat, 4]: non-ignored GTs), per group
 *    iou_sum f64 / iou_cnt int32 [n_img * n_cat] (entries >= 0.3 of the group's D x G IoU matrix), and into the workspace
 *    (yolo_coco_workspace_bytes(n_dt); nothing in it needs initialising) the rank of each detection inside its group.
 *    Matched flags are kept per GT slot; pycocotools keeps annotation ids and therefore loses a match to a GT whose id is 0.
 *  yolo_coco_accumulate_fwd: accumulate's sweep per category x area range x maxDets x threshold over the SAME dt_match / dt_ignore /
 *    npig / workspace.  order: device int32 [n_dt], the detection indices category by category (cat_off: device int32 [n_cat + 1])
 *    and inside a category by descending score, ties in (image, rank) order.  Writes precision f64 [10, 101, n_cat, 4, 3] and recall
 *    f64 [10, n_cat, 4, 3] (pycocotools' layout; -1 where a category has no non-ignored GT in the range), every element.
 *    The sweep walks yolo_coco_sweep_chunk() detections at a time. */
YOLO_API int yolo_coco_sweep_chunk(void);
YOLO_API int yolo_coco_max_gt(void);
YOLO_API size_t yolo_coco_workspace_bytes(int n_dt);
YOLO_API int yolo_coco_match_fwd(const double* dt_box, const int32_t* dt_off, int n_dt, const double* gt_box, const double* gt_area,
                                 const uint8_t* gt_crowd, const int32_t* gt_off, int n_gt, int n_img, int n_cat, int max_gt,
                                 const double* iou_thrs, const double* area_rng, uint64_t* dt_match, uint64_t* dt_ignore,
                                 int32_t* npig, double* iou_sum, int32_t* iou_cnt, int32_t* status, void* workspace,
                                 size_t workspace_bytes, yolo_stream_t s);
YOLO_API int yolo_coco_accumulate_fwd(const int32_t* order, const int32_t* cat_off, int n_dt, int n_cat, const uint64_t* dt_match,
                                      const uint64_t* dt_ignore, const int32_t* npig, const double* rec_thrs, const int32_t* max_dets,
                                      double eps, const void* workspace, size_t workspace_bytes, double* precision, double* recall,
                                      yolo_stream_t s);

/* ---- scale_coords (utils/utils.py:296-303): map kept boxes from the network-input frame back to each original
 *  image: dets [bs,cap,row_floats] (columns 0..3 = x1,y1,x2,y2) in place; params_dev: device f32 [bs][4] =
 *  {pad_x, pad_y, gain, n_rows}; do_round = the `.round()` of the caller at utils.py:313. */
YOLO_API int yolo_scale_coords(float* dets, int bs, int cap, int row_floats, const float* params_dev, int do_round,
                               yolo_stream_t s);

/* ---- pre-processing of one decoded image: LetterBox (utils/augs.py:7-94: cv2.resize
 *  INTER_AREA by resize_ratio to rh x rw, placed at (top,left) of a th x tw rectangle with BORDER_REPLICATE) and,
 *  when dst_f32 is given, _convert_img_for_net + equalize_shapes as well (utils/dataset_csv.py:79-87,146-171:
 *  float32 /255, HWC -> CHW, the rectangle at (off_y,off_x) of a dst_h x dst_w canvas filled with `fill` = 0.5).
 *  src: uint8 [h,w,c] interleaved, c <= 4, row pitch src_pitch bytes.  Exactly one destination:
 *  dst_u8 [th,tw,c] (= LetterBox.apply's image) or dst_f32 [c,dst_h,dst_w] (one image of the NCHW batch).
 *  The geometry (rh, rw, pads) is computed by the caller exactly as LetterBox.update_params does (augs.py:24-63;
 *  pytorch_yolo_amd.utils.augs.letterbox_params).  cv2 is not available to pin the resize: see oracle/preprocess.py. */
YOLO_API int yolo_letterbox_u8_fwd(const uint8_t* src, int h, int w, int c, int src_pitch, double resize_ratio, int rh,
                                   int rw, int top, int left, int th, int tw, uint8_t* dst_u8, float* dst_f32,
                                   int dst_h, int dst_w, int off_y, int off_x, float fill, yolo_stream_t s);

/* ---- fp32 "reference-precision" mode: the same operators with float32 NHWC activations and float32 weights, the
 *  contraction on v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation) - the arithmetic of the reference's fp32
 *  ATen ops up to summation order.  ~1/16 of the bf16 MFMA rate: a parity mode (model.precision = "fp32"), not the bench.
 *  yolo_conv2d_f32_fwd: ConvBlock.forward / plain heads / Add / Upsample / Concat placement exactly as yolo_conv2d_fwd
 *  (models/yolo_base.py:19-44, yolov3_tiny.py:38,42, yolov3_spp.py:12-14, yolo_layer.py:6-22); views are multiples of 4
 *  channels, w_packed f32 [cout_pad][kpad] (yolo_pack_conv_weight_f32_f32; kpad multiple of 32, cout_pad of 128),
 *  d->out_dtype is ignored (always f32), any odd ksize <= 7.
 *  yolo_maxpool_f32_fwd: MaxPool (models/yolo_base.py:60-66); the SPP pyramid (yolov3_spp.py:75-77) is three calls
 *  (5 / 9 / 13, stride 1) from slice [3c,4c) into slices [0,c) [c,2c) [2c,3c) of the concat buffer.
 *  yolo_pack_input_nchw_f32_nhwc: the layout step in front of the first conv, channels zero-padded to c_pad. */
YOLO_API int yolo_conv2d_f32_fwd(const float* x, const float* w_packed, const float* bias, const float* residual, float* y,
                                 float* y_preadd, const YoloConvDesc* d, yolo_stream_t s);
YOLO_API int yolo_maxpool_f32_fwd(const float* x, float* y, int n, int h, int w, int c, int in_c_total, int in_c_offset, int ho,
                                  int wo, int out_c_total, int out_c_offset, int ksize, int stride, int pad, int dilation,
                                  yolo_stream_t s);
YOLO_API int yolo_pack_input_nchw_f32_nhwc(const float* x, float* y, int n, int c, int h, int w, int c_pad, yolo_stream_t s);
YOLO_API int yolo_pack_conv_weight_f32_f32(const float* w_oihw, int cout, int cin_w, int ksize, int cin, int cout_pad, int kpad,
                                           float* out);

/* ---- fp32 mode, the depthwise encoder families (the float instances of csrc/efficient.hip and, for the shuffle,
 *  csrc/pointwise.hip; yolo_maxpool_f32_fwd and yolo_pack_input_nchw_f32_nhwc above live in pointwise.hip too): float32 NHWC views in multiples of 4 channels, float32
 *  arithmetic, expf and an IEEE division in the activations, fmaf chains in a fixed order (no result depends on the grid).
 *  yolo_dwconv_f32_fwd: depthwise k x k conv (k = 3 or 5, stride 1 or 2) + bias + act (any YOLO_ACT_*) with an explicit leading pad
 *  and the caller's ho x wo, everything outside the image reads zero - arguments and geometry rule of yolo_dwconv_fwd.  One entry
 *  point for torch's pad 1 (ksize 3, pad 1, ho = (h - 1) / stride + 1: torchvision's InvertedResidual behind
 *  models/yolov3_tiny_mobilenet.py:11-34 and the ShuffleNetV2 units behind models/yolov3_tiny_shuffle.py:13-47) and TensorFlow "same"
 *  (efficientnet_pytorch 0.2.0 Conv2dSamePadding, MBConvBlock._depthwise_conv behind models/yolov3_tiny_efficient.py:22-45:
 *  pad = pad_total / 2, ho = ceil(h / stride)).  w: f32 [k*k][c] tap-major, bias f32 [c]. */
YOLO_API int yolo_dwconv_f32_fwd(const float* x, const float* w, const float* bias, float* y, int n, int h, int w_, int c,
                                 int in_c_total, int in_c_offset, int ho, int wo, int out_c_total, int out_c_offset, int ksize,
                                 int stride, int pad, int act, yolo_stream_t s);
/* yolo_se_f32_fwd: squeeze-and-excitation of an MBConvBlock (efficientnet_pytorch 0.2.0 model.py, used through
 *  models/yolov3_tiny_efficient.py:47-56) exactly as yolo_se_fwd, on float32 views (y may be x); weights as there; workspace:
 *  yolo_se_workspace_bytes(n, c) bytes with the same layout (the pooled means stay in its first n*c floats).  The partial sums of
 *  the pooling pass meet in a fixed order: bit-identical from run to run. */
YOLO_API int yolo_se_f32_fwd(const float* x, float* y, int n, int h, int w, int c, int in_c_total, int in_c_offset, int out_c_total,
                             int out_c_offset, const float* w1, const float* b1, const float* w2, const float* b2, int squeeze,
                             void* workspace, size_t ws_bytes, yolo_stream_t s);
/* yolo_channel_shuffle2_f32_fwd: ShuffleNetV2's channel_shuffle(cat(a, b), groups = 2) (torchvision shufflenetv2, used by
 *  models/yolov3_tiny_shuffle.py:13-47) in the two-slot physical layout of yolo_channel_shuffle2_fwd, on float32 views; c_slot and
 *  the view of y are multiples of 4 channels; the pad channels of both slots of y are written as zero. */
YOLO_API int yolo_channel_shuffle2_f32_fwd(const float* a, const float* b, float* y, int n, int h, int w, int half, int c_slot,
                                           int a_c_total, int a_c_offset, int b_c_total, int b_c_offset, int y_c_total,
                                           int y_c_offset, yolo_stream_t s);

/* ---- fp16-operand mode (model.precision = "fp16"): the rounding points of the bf16 path with IEEE half instead - fp16 NHWC
 *  activations and packed weights (same bytes and layout as bf16), fp32 accumulation on v_mfma_f32_16x16x32_f16 /
 *  v_mfma_f32_32x32x16_f16, the residual sum formed in fp32 and stored once, fp32 head outputs.  Narrowing: round to nearest even; a
 *  FINITE value beyond +-65504 stores +-65504; NaN and +-inf stay.  Every launch is an instance of the gather kernel's fp16 table
 *  (csrc/conv_igemm.hip); there is no split-K form and the tuning word of yolo_set_tuning does not apply.
 *  yolo_conv2d_f16_fwd: as yolo_conv2d_fwd; d->out_dtype is YOLO_DT_F16 or YOLO_DT_F32; w_packed from yolo_pack_conv_weight_f32_f16
 *  (same sizes and k order as the bf16 packing).  yolo_conv2d_f16_pick / yolo_head_decode_f16_pick: the instance + grid
 *  ("igemm_f16<...> grid N"), no launch, no GPU.  yolo_head_decode_f16_fwd / yolo_head_decode_filter_f16_fwd: as their bf16 forms
 *  (the decode works on the fp32 accumulators).  yolo_maxpool_f16_fwd: MaxPool on fp16 views.  The SPP pyramid of an fp16 buffer is
 *  yolo_spp_fwd itself: it orders 16-bit sign-magnitude patterns, which IEEE half is too.
 *  yolo_pack_input_nchw_f32_f16: x f32 NCHW -> y fp16 NHWC [n,h,w,c_pad]. */
YOLO_API int yolo_conv2d_f16_fwd(const void* x, const void* w_packed, const float* bias, const void* residual, void* y,
                                 void* y_preadd, const YoloConvDesc* d, yolo_stream_t s);
/* The large 3x3 / pad 1 layers of the fp16 mode on the 20x20-output-tile kernels (stride 1 and stride 2; csrc/conv3x3_t20.h), the
 *  fp16 forms of the kernels yolo_conv2d_fwd runs such layers on: v_mfma_f32_16x16x32_f16, fp16 residual / pre-add copy, the
 *  narrowing above.  Arguments as yolo_conv2d_f16_fwd with d->out_dtype = YOLO_DT_F16.  yolo_conv2d_f16_fwd itself never
 *  dispatches here: whoever builds a launch list chooses per layer.
 *  yolo_conv3x3_t20_f16_supported: 1 when the shipped rule takes the layer - 3x3, pad 1, stride 1 or 2, cin % 32 == 0,
 *  cout % 128 == 0, no swish, no upsampling store, every view in multiples of 8 channels, the map covered >= 90 % by 20x20 tiles and
 *  tiles * cout / 128 >= CUs / 2 (stride 1) or >= 2 * CUs (stride 2), CUs = 256 or what yolo_set_launch_cus said.  A pure function
 *  of its arguments and that number; launches nothing, needs no GPU, and no yolo_set_tuning knob changes it.
 *  yolo_conv3x3_t20_f16_fwd: force = 0 returns YOLO_E_UNSUPPORTED where _supported says 0; force = 1 runs every layer the
 *  kernels can compute (everything above but the last two conditions; tests, A/B runs). */
YOLO_API int yolo_conv3x3_t20_f16_supported(const YoloConvDesc* d, int has_residual, int has_aux);
YOLO_API int yolo_conv3x3_t20_f16_fwd(const void* x, const void* w_packed, const float* bias, const void* residual, void* y,
                                      void* y_aux, const YoloConvDesc* d, int force, yolo_stream_t s);
YOLO_API int yolo_conv2d_f16_pick(const YoloConvDesc* d, int has_residual, int has_preadd, char* out, int out_len);
YOLO_API int yolo_head_decode_f16_pick(const YoloConvDesc* d, int na, int nc, int filter, char* out, int out_len);
YOLO_API int yolo_head_decode_f16_fwd(const void* x, const void* w_packed, const float* bias, const YoloConvDesc* d,
                                      const float* anchors_px, int na, int nc, float stride_px, float* io,
                                      int io_rows_total, int io_row_offset, float* p, yolo_stream_t s);
YOLO_API int yolo_head_decode_filter_f16_fwd(const void* x, const void* w_packed, const float* bias, const YoloConvDesc* d,
                                             const float* anchors_px, int na, int nc, float stride_px, int io_rows_total,
                                             int io_row_offset, float conf_thres, float min_wh, void* workspace,
                                             size_t workspace_bytes, float* p, yolo_stream_t s);
YOLO_API int yolo_maxpool_f16_fwd(const void* x, void* y, int n, int h, int w, int c, int in_c_total, int in_c_offset, int ho,
                                  int wo, int out_c_total, int out_c_offset, int ksize, int stride, int pad, int dilation,
                                  yolo_stream_t s);
YOLO_API int yolo_pack_input_nchw_f32_f16(const float* x, void* y, int n, int c, int h, int w, int c_pad, yolo_stream_t s);
YOLO_API int yolo_pack_conv_weight_f32_f16(const float* w_oihw, int cout, int cin_w, int ksize, int cin, int cout_pad, int kpad,
                                           uint16_t* out);

/* ---- batched launcher: run a recorded list of ops with one FFI crossing (host overhead only). */
enum { YOLO_OP_CONV = 1, YOLO_OP_MAXPOOL = 2, YOLO_OP_SPP = 3, YOLO_OP_DWCONV = 4, YOLO_OP_CONV1_NCHW = 5,
       YOLO_OP_RESUNIT = 6, YOLO_OP_STEM = 7, YOLO_OP_HEAD_DECODE = 8, YOLO_OP_CONV1_POOL = 9, YOLO_OP_MBCONV = 10,
       YOLO_OP_CONV_POOL = 11 /* yolo_conv3x3_pool_fwd with pool = 1: x = bf16 NHWC, y = the pooled map */,
       YOLO_OP_SHUFFLE = 12 /* yolo_channel_shuffle2_fwd: x = a, residual = b, conv.cin = c_slot, conv.cout = half, res_* = view of b */,
       YOLO_OP_CONV_F32 = 13 /* yolo_conv2d_f32_fwd */, YOLO_OP_MAXPOOL_F32 = 14 /* yolo_maxpool_f32_fwd, fields as MAXPOOL */,
       YOLO_OP_SE = 15 /* yolo_se_fwd: x / y views in conv (n, h, w, cin, in_*, out_*), w / bias = W1 / b1, w_pre / bias_pre = W2 / b2,
                          kpad_pre = squeezed channels, workspace / ws_bytes */,
       YOLO_OP_CONV_F16 = 16 /* yolo_conv2d_f16_fwd */, YOLO_OP_MAXPOOL_F16 = 17 /* yolo_maxpool_f16_fwd, fields as MAXPOOL */,
       YOLO_OP_HEAD_DECODE_F16 = 18 /* yolo_head_decode_f16_fwd / yolo_head_decode_filter_f16_fwd, fields as HEAD_DECODE */,
       YOLO_OP_CONV_T20_F16 = 19 /* yolo_conv3x3_t20_f16_fwd with force = 1 (the list's builder asked yolo_conv3x3_t20_f16_supported),
                                    fields as CONV_F16 */,
       YOLO_OP_DWCONV_F32 = 20 /* yolo_dwconv_f32_fwd, fields as DWCONV; conv.ksize / conv.pad always the real ones (3 / 1 for the
                                  torch-style layers): there is no ksize 0 form */,
       YOLO_OP_SE_F32 = 21 /* yolo_se_f32_fwd, fields as SE */, YOLO_OP_SHUFFLE_F32 = 22 /* yolo_channel_shuffle2_f32_fwd, fields as SHUFFLE */ };
typedef struct YoloOp {
  int32_t kind, _pad;
  const void* x; const void* w; const float* bias; const void* residual; void* y; void* y_aux;
  YoloConvDesc conv;             /* kind CONV; DWCONV/MAXPOOL/SPP reuse the geometry fields (DWCONV with ksize 0: the 3x3 / pad 1 form)
                                    (ksize/stride/pad, act, views); MAXPOOL dilation = upsample2x field;
                                    CONV1_NCHW: x = f32 NCHW input, res_c_total = real input channels;
                                    RESUNIT: the unit's 3x3 (w/bias = W2/b2), see yolo_resunit_fwd;
                                    STEM: the stride-2 conv (w/bias = W2/b2), x = f32 NCHW input,
                                    res_c_total = real input channels, see yolo_stem_fwd */
  const void* w_pre; const float* bias_pre;   /* RESUNIT / STEM: packed W1 / b1 of the leading conv */
  int32_t kpad_pre, cout_pad_pre;
  /* HEAD_DECODE (yolo_head_decode_fwd): y = io, y_aux = p (nullable), conv = the head conv.  y == NULL with workspace set:
     yolo_head_decode_filter_fwd into the compact NMS workspace (workspace / ws_bytes), thresholds head_filter_conf / head_filter_min_wh */
  float head_anchors_px[8]; float head_stride_px;
  int32_t head_na, head_nc, io_rows_total, io_row_offset; float head_filter_conf;
  /* MBCONV (yolo_mbconv_fwd): w/bias = W_proj/b_proj, w_pre/bias_pre = W_expand/b_expand (NULL: no expand conv),
     w_dw/bias_dw = the depthwise conv; geometry from conv (n,h,w,cin,views,cout,stride), hidden = kpad_pre,
     has_res = conv.res_c_total != 0 */
  const float* w_dw; const float* bias_dw;
  /* CONV with splits >= 2: yolo_conv2d_splitk_fwd */
  void* workspace; int32_t* counters; size_t ws_bytes; int32_t splits; float head_filter_min_wh;
} YoloOp;
YOLO_API int yolo_run_ops(const YoloOp* ops, int n_ops, yolo_stream_t s);

/* A HIP stream restricted to the compute units of cu_mask (bit i of the n_words x 32-bit vector = CU i; on MI355X CU i sits
 * on XCD i % 8).  The host mirror runs the sub-batches of one detect() call on disjoint CU sets (engine.StreamedPlan);
 * the reference has no counterpart (one torch stream, models/yolo_base.py forward).  Destroy with yolo_stream_destroy. */
YOLO_API int yolo_stream_create_cu_mask(const uint32_t* cu_mask, int n_words, yolo_stream_t* out);
YOLO_API int yolo_stream_destroy(yolo_stream_t s);
/* Tell the tile rules how many compute units the coming launches of THIS thread may use (default 256; a CU-masked stream's share
 * while launching on it): grids are sized against it.  Returns the previous value (<0: argument error). */
YOLO_API int yolo_set_launch_cus(int n_cu);

/* ---- one pipelined detect() step with ONE FFI crossing (round 4): what pytorch_yolo_amd.engine.StreamedPlan.launch_detect does
 *  for a whole-batch pipeline - the composition of reference utils/utils.py:374-378 (forward -> non_max_suppression) on a stream of
 *  batches - as a single call, because at YOLOv3-tiny rates (0.37 ms per 32 images) the Python between the launches was the
 *  bottleneck of detect_stream().  Order of what it enqueues:
 *    stream:      [wait wait_x] ops[0 .. k_io) [wait wait_io] ops[k_io .. n_ops) ; record heads_done
 *    nms_stream:  wait heads_done ; yolo_nms_merge(io ...) ; [count -> count_host, async] ; record nms_done ; [record done]
 *  wait_x: "the input batch is ready" (recorded by the caller on the stream that produced x); wait_io: the nms_done of the step that
 *  used this io buffer before (its NMS still reads io when the head launches - ops from k_io on - would overwrite it).
 *  Events are yolo_event_t (hipEvent_t, timing disabled) from yolo_event_create; NULL = skip.  nms_stream may equal stream.
 *  io == NULL selects the compact form: `workspace` is a yolo_nms_compact_workspace_bytes one, the head ops (already bound to it,
 *  YoloOp) filter into it behind wait_io and the NMS is yolo_nms_merge_compact.
 *  count_host: PINNED host memory for bs int32 (NULL: no copy): valid once `done` (or nms_done) has completed.
 *  Nothing is synchronised on the host; buffers stay owned by the caller as everywhere else. */
typedef void* yolo_event_t; /* hipEvent_t */
YOLO_API int yolo_event_create(yolo_event_t* out);
YOLO_API int yolo_event_destroy(yolo_event_t e);
YOLO_API int yolo_event_record(yolo_event_t e, yolo_stream_t s);
YOLO_API int yolo_event_synchronize(yolo_event_t e);
typedef struct YoloPipeStep {
  const YoloOp* ops; int32_t n_ops, k_io;
  yolo_stream_t stream, nms_stream;
  yolo_event_t wait_x, wait_io, heads_done, nms_done, done;
  float* io; int32_t bs, rows, nc, max_per_class; float conf_thres, nms_thres, min_wh; int32_t cap;
  float* out_dets; int32_t* out_idx; int32_t* out_count; void* workspace; size_t workspace_bytes;
  int32_t* count_host;
} YoloPipeStep;
YOLO_API int yolo_pipeline_step(const YoloPipeStep* st);
/* sizeof of the ABI's structs as the library was compiled (0 YoloConvDesc, 1 YoloOp, 2 YoloMbconvDesc, 3 YoloPipeStep; else -1):
 * a binding checks its own layout against it. */
YOLO_API int yolo_abi_sizeof(int which);
/* The kept rows of all images packed back to back (the reference returns one [n_i, 7] tensor per image, utils.py:293): image b's
 * min(count[b], cap) rows of dets [bs, cap, 7] go to packed rows [sum_{i<b} count'[i], ...), their pivot rows to packed_idx (nullable).
 * One launch, offsets computed on the device from `count` (the host knows the total from its copy of the counts). */
YOLO_API int yolo_pack_detections(const float* dets, const int32_t* idx, const int32_t* count, int bs, int cap, float* packed,
                                  int64_t* packed_idx, yolo_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* YOLO_HIP_H */
