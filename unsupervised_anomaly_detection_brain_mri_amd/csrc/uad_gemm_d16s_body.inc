// Body of the two lane = pixel translation units (UAD_D16S_NPL = 2: uad_gemm_d16s.hip, bf16x3 products; 3: uad_gemm_d16s3.hip, bf16x6): 14 fully
// unrolled instances each (five channel ranges x {plain + activation on load, backward} + the fused final epilogue x {training, reconstruction} x two ranges).
#include "uad_gemm_common.h"

namespace {
#include "uad_conv16s.inc"
}  // namespace

#define UAD_D16S_CAT2(a, b) a##b
#define UAD_D16S_CAT(a, b) UAD_D16S_CAT2(a, b)

void UAD_D16S_CAT(uad_d16s_launch_v, UAD_D16S_NPL)(const ConvGemmArgs& a, dim3 grid, int bn, int cst, bool any_order, hipStream_t st) {
    if (bn == 64) {
        if (cst == 128) launch_conv5_d16s_bn64<128>(a, grid, any_order, st);
        else if (cst == 64) launch_conv5_d16s_bn64<64>(a, grid, any_order, st);
        else if (cst == 32) launch_conv5_d16s_bn64<32>(a, grid, any_order, st);
        else { fprintf(stderr, "uad: no lane = pixel instance for a %d-channel range\n", cst); abort(); }
    } else {
        if (cst == 64) launch_conv5_d16s_bn32<64>(a, grid, any_order, st);
        else if (cst == 32) launch_conv5_d16s_bn32<32>(a, grid, any_order, st);
        else { fprintf(stderr, "uad: no lane = pixel instance for a %d-channel range\n", cst); abort(); }
    }
}
