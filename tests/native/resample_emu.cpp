// Host emulation of the three kernels of csrc/uad_resample.hip (tests/test_resample_kernels_host.py): the kernel source itself is compiled for
// the CPU behind the shim of hip_host_emu.h -- the threads of a block are a plain loop where the kernel has no barrier and real threads around
// a std::barrier where it has one (zoom_rows_kernel) -- and driven by the same launch geometry as uad_zoom_spline3.
//   resample_emu in.f32 n h w H W boundary out_kind out.bin
#include "hip_host_emu.h"
#include "../../unsupervised_anomaly_detection_brain_mri_amd/csrc/uad_resample.hip"

int main(int argc, char** argv) {
    if (argc != 10) return 1;
    const int n = atoi(argv[2]), h = atoi(argv[3]), w = atoi(argv[4]), H = atoi(argv[5]), W = atoi(argv[6]), boundary = atoi(argv[7]), out_kind = atoi(argv[8]);
    std::vector<float> in((size_t)n * h * w);
    if (!read_all(argv[1], in.data(), in.size())) return 2;
    std::vector<int> out((size_t)n * H * W);                    // 4-byte elements either way
    // the launch sequence of uad_zoom_spline3
    const int pad = zoom_pad(boundary), hp = h + 2 * pad, wp = w + 2 * pad;
    std::vector<double> coef((size_t)n * hp * wp);
    double* c = coef.data();
    const float* src = in.data();
    void* dst = out.data();
    const double z = std::sqrt(3.0) - 2.0;
    const double zy = H > 1 ? (double)(h - 1) / (double)(H - 1) : 1.0, zx = W > 1 ? (double)(w - 1) / (double)(W - 1) : 1.0;
    const double zny = std::pow(z, hp - 1), znx = std::pow(z, wp - 1);
    const size_t cols = (size_t)n * wp;
    const int rows = n * hp;
    launch_loop(dim3((unsigned)((cols + 255) / 256)), dim3(256), [&] { zoom_cols_kernel(src, n, h, w, pad, hp, wp, z, zny, c); });
    launch_threads(dim3((unsigned)((rows + ZOOM_TILE - 1) / ZOOM_TILE)), dim3(ZOOM_TILE), [&] { zoom_rows_kernel(c, rows, wp, z, znx); });
    launch_loop(dim3((W + 63) / 64, (H + 3) / 4, n < 2 ? n : 2), dim3(64, 4), [&] { zoom_interp_kernel(c, n, pad, hp, wp, H, W, zy, zx, out_kind, dst); });
    return write_all(argv[9], out.data(), out.size()) ? 0 : 3;
}
