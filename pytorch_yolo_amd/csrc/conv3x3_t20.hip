// The bf16 instantiations of the 20x20-tile 3x3 kernels (conv3x3_t20.h: stride 1 conv3x3_t20v2_kernel, stride 2
// conv3x3s2_t20_kernel) and their place in yolo_conv2d_fwd's dispatch.  The IEEE-half instantiations live in conv3x3_t20_f16.hip.
#include "conv3x3_t20.h"

using namespace yolo_conv;

// Returns 1 when this kernel does not take the layer (the caller goes on to the other kernels).
// force: 0 = the shipped rules, 1 = every layer the kernels can compute (t20_3x3_form).
int yolo_conv::launch_t20_3x3(const ConvArgs& a, int force, hipStream_t s) {
  switch (t20_3x3_form(a.d, a.res != nullptr, a.aux != nullptr, YOLO_DT_BF16, force)) {
    case 1: return launch_t20v2<bf16_t>(a, s, "yolo_conv2d_fwd(t20v2)");
    case 2: return launch_t20s2<bf16_t>(a, s, "yolo_conv2d_fwd(t20s2)");
    default: return 1;
  }
}
