// The IEEE-half instantiations of the 20x20-tile 3x3 kernels (conv3x3_t20.h) and their entry points: model.precision = "fp16"
// runs its large 3x3 layers - stride 1 and stride 2 - on them instead of the gather kernel (YOLO_OP_CONV_T20_F16; the planner asks
// yolo_conv3x3_t20_f16_supported per layer).  Same staging, weight stream, waits and epilogue structure as the bf16 forms; the MFMA is
// v_mfma_f32_16x16x32_f16, the residual and the pre-add copy are fp16, and the one narrowing is narrow<f16_t> (round to nearest even,
// a finite overflow stores +-65504, NaN / +-inf stay).  Rounding points are the fp16 gather kernel's: fp32 accumulate, bias,
// activation and residual in fp32.  The bf16 tuning word (yolo_set_tuning) does not reach these launches.
#include "conv3x3_t20.h"

using namespace yolo_conv;

namespace {

// What is wrong with the descriptor as an argument of these entry points (nullptr: nothing) - the checks of yolo_conv2d_fwd that
// bear on a 3x3 layer, and the output size of symmetric padding (the kernels have no "same"-padding form).
const char* desc_problem(const YoloConvDesc& d, bool has_res, bool has_aux) {
  if (d.n <= 0 || d.h <= 0 || d.w <= 0 || d.cout <= 0) return "empty tensor";
  if (d.cin <= 0 || d.cin % 8 != 0) return "cin must be a positive multiple of 8";
  if (d.in_c_offset < 0 || d.in_c_offset % 8 != 0 || d.in_c_total % 8 != 0 || d.in_c_offset + d.cin > d.in_c_total) return "bad input view";
  if (d.out_c_offset < 0 || d.out_c_offset % 4 != 0 || d.out_c_total % 4 != 0 || d.out_c_offset + d.cout > d.out_c_total) return "bad output view";
  if (d.ksize != 1 && d.ksize != 3) return "ksize unsupported (1 or 3)";
  if (d.stride != 1 && d.stride != 2) return "stride unsupported";
  if (d.kpad % 64 != 0 || d.kpad < d.ksize * d.ksize * d.cin) return "kpad must be a multiple of 64 that holds ksize * ksize * cin";
  if (d.cout_pad % 128 != 0 || d.cout_pad < d.cout) return "bad cout_pad";
  if (has_res && (d.res_c_offset < 0 || d.res_c_total % 4 != 0 || d.res_c_offset % 4 != 0 || d.res_c_offset + d.cout > d.res_c_total || d.upsample2x))
    return "bad residual view";
  if (has_aux && (d.aux_c_offset < 0 || d.aux_c_total % 4 != 0 || d.aux_c_offset % 4 != 0 || d.aux_c_offset + d.cout > d.aux_c_total)) return "bad aux view";
  if (conv_x_bytes(d) >= kOobOffset || conv_w_bytes(d) >= kOobOffset) return "tensor larger than 3.75 GiB not supported";
  const long M = (long)d.n * d.ho * d.wo;
  if (M <= 0 || M >= 0x7fffffffL / 4) return "M out of range";
  return nullptr;
}

// the output size the kernels compute: symmetric padding, nothing else
bool std_out(const YoloConvDesc& d) {
  return d.ho == (d.h + 2 * d.pad - d.ksize) / d.stride + 1 && d.wo == (d.w + 2 * d.pad - d.ksize) / d.stride + 1;
}

}  // namespace

// 1 when the shipped rule hands the layer to the fp16 20x20-tile kernels (t20_3x3_form: the rule of the bf16 kernels with
// d->out_dtype == YOLO_DT_F16), 0 otherwise.  A pure function of the arguments and launch_cus(); launches nothing, needs no GPU.
extern "C" int yolo_conv3x3_t20_f16_supported(const YoloConvDesc* d, int has_residual, int has_aux) {
  if (!d || desc_problem(*d, has_residual != 0, has_aux != 0) || !std_out(*d)) return 0;
  return t20_3x3_form(*d, has_residual != 0, has_aux != 0, YOLO_DT_F16, 0) != 0;
}

extern "C" int yolo_conv3x3_t20_f16_fwd(const void* x, const void* w_packed, const float* bias, const void* residual, void* y,
                                        void* y_aux, const YoloConvDesc* dp, int force, yolo_stream_t s) {
  YOLO_REQUIRE(x && w_packed && bias && y && dp, "conv3x3_t20_f16: null pointer");
  const YoloConvDesc& d = *dp;
  const char* const problem = desc_problem(d, residual != nullptr, y_aux != nullptr);
  YOLO_REQUIRE(!problem, "conv3x3_t20_f16: %s", problem);
  YOLO_REQUIRE(d.out_dtype == YOLO_DT_F16, "conv3x3_t20_f16: out_dtype %d (YOLO_DT_F16)", d.out_dtype);
  const int form = std_out(d) ? t20_3x3_form(d, residual != nullptr, y_aux != nullptr, YOLO_DT_F16, force ? 1 : 0) : 0;
  if (!form)
    return yolo_set_error(YOLO_E_UNSUPPORTED, force ? "conv3x3_t20_f16: not a layer the 20x20-tile kernels compute (3x3 / pad 1, stride 1 or 2, "
                                                      "cin %% 32 == 0, cout %% 128 == 0, no swish, no upsampling store, views in multiples of 8)"
                                                    : "conv3x3_t20_f16: the shipped rule does not take this layer (yolo_conv3x3_t20_f16_supported)");
  ConvArgs a = make_conv_args(x, w_packed, bias, residual, y, y_aux, d);
  a.debug = 0;                       // (as in the fp16 gather path: no tuning knob reaches these launches)
  YOLO_SET_STAMPS(a);
  return form == 2 ? launch_t20s2<f16_t>(a, (hipStream_t)s, "yolo_conv3x3_t20_f16_fwd(t20s2)")
                   : launch_t20v2<f16_t>(a, (hipStream_t)s, "yolo_conv3x3_t20_f16_fwd(t20v2)");
}
