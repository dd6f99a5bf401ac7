// bf16 instantiations of the MFMA direct convolution (see conv_mfma.hip)
#include "conv_mfma_impl.h"
int dh_conv_launch_bf16(const ConvArgs& a, const ConvPlan& p, hipStream_t st) { return launch_ks<bf16>(a, p, st); }
