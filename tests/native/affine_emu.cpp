// Host emulation of uad_affine_spline3 (tests/test_rotate_kernels_host.py): the kernel source of csrc/uad_resample.hip is compiled for the
// CPU behind the shim of hip_host_emu.h -- the threads of a block are a plain loop where the kernel has no barrier and real threads around a
// std::barrier where it has one (zoom_rows_kernel) -- and driven by the launch geometry of uad_affine_spline3: the mirror or reflect
// prefilter, then affine_interp_kernel on 16 x 16 tiles with K transforms.
//   affine_emu in.f32 n h w H W xf.f64 K boundary out_kind out.bin          (xf.f64: K x 6 doubles; out.bin: [n,K,H,W] of 4-byte elements)
#include "hip_host_emu.h"
#include "../../unsupervised_anomaly_detection_brain_mri_amd/csrc/uad_resample.hip"

template <int INIT>
static void prefilter(const float* src, int n, int h, int w, int pad, double* c) {
    const int hp = h + 2 * pad, wp = w + 2 * pad, e = INIT == PREFILTER_REFLECT ? 0 : 1;
    const double z = std::sqrt(3.0) - 2.0, zny = std::pow(z, hp - e), znx = std::pow(z, wp - e);
    const size_t cols = (size_t)n * wp;
    const int rows = n * hp;
    launch_loop(dim3((unsigned)((cols + 255) / 256)), dim3(256), [&] { zoom_cols_kernel<INIT>(src, n, h, w, pad, hp, wp, z, zny, c); });
    launch_threads(dim3((unsigned)((rows + ZOOM_TILE - 1) / ZOOM_TILE)), dim3(ZOOM_TILE), [&] { zoom_rows_kernel<INIT>(c, rows, wp, z, znx); });
}

int main(int argc, char** argv) {
    if (argc != 12) return 1;
    const int n = atoi(argv[2]), h = atoi(argv[3]), w = atoi(argv[4]), H = atoi(argv[5]), W = atoi(argv[6]), K = atoi(argv[8]), boundary = atoi(argv[9]),
              out_kind = atoi(argv[10]);
    if (K < 1 || K > UAD_AFFINE_MAX_K) return 1;
    std::vector<float> in((size_t)n * h * w);
    AffineTable tab = {};
    if (!read_all(argv[1], in.data(), in.size()) || !read_all(argv[7], &tab.v[0][0], (size_t)K * 6)) return 2;
    std::vector<int> out((size_t)n * K * H * W);                // 4-byte elements either way
    // the launch sequence of uad_affine_spline3
    const int pad = zoom_pad(boundary);
    std::vector<double> coef((size_t)n * (h + 2 * pad) * (w + 2 * pad));
    double* c = coef.data();
    void* dst = out.data();
    if (pad) prefilter<PREFILTER_REFLECT>(in.data(), n, h, w, pad, c);
    else prefilter<PREFILTER_MIRROR>(in.data(), n, h, w, pad, c);
    launch_loop(dim3((W + 15) / 16, (H + 15) / 16, n < 2 ? n : 2), dim3(16, 16), [&] { affine_interp_kernel(c, n, K, pad, h, w, H, W, tab, out_kind, dst); });
    return write_all(argv[11], out.data(), out.size()) ? 0 : 3;
}
