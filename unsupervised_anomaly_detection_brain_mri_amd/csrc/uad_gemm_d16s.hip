// The lane = pixel D-kind k5 s2 kernels (uad_conv16s.inc), bf16x3 products, as a translation unit of their own (the family's fully unrolled instances
// dominate the library's compile time).  Interface: uad_d16s_takes / uad_d16s_t16 / uad_d16s_launch_v2 (uad_conv_launch.h).
#define UAD_D16S_NPL 2
#include "uad_gemm_d16s_body.inc"

bool uad_d16s_takes(const ConvGemmArgs& a) { return conv5_d16s_takes(a); }
// the instance list of launch_conv5_d16s_n: a fused final in its training form runs on 16 x 16 tiles
bool uad_d16s_t16(const ConvGemmArgs& a, int bn, int cst, int npl) {
    return a.ep.kind == UAD_EPI_FINAL && bn == 32 && cst == 32 && npl == 2 && conv5_d16s_t16(a);
}
