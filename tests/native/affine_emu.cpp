// Host emulation of uad_affine_spline3 (tests/test_rotate_kernels_host.py): the kernel source of csrc/uad_resample.hip is compiled for the
// CPU behind the shim of tests/native/resample_emu.cpp -- blocks run one after the other; the threads of a block are a plain loop where the
// kernel has no barrier and real threads around a std::barrier where it has one (zoom_rows_kernel) -- and driven by the launch geometry of
// uad_affine_spline3: the mirror or reflect prefilter, then affine_interp_kernel on 16 x 16 tiles with K transforms.
//   affine_emu in.f32 n h w H W xf.f64 K boundary out_kind out.bin          (xf.f64: K x 6 doubles; out.bin: [n,K,H,W] of 4-byte elements)
#include <barrier>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
thread_local dim3 threadIdx, blockIdx;
dim3 blockDim, gridDim;
std::barrier<>* block_barrier = nullptr;
static void __syncthreads() { block_barrier->arrive_and_wait(); }
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __restrict__
#define UAD_RESAMPLE_HOST_EMULATION
#include "../../unsupervised_anomaly_detection_brain_mri_amd/csrc/uad_resample.hip"

template <class F>
static void launch_loop(dim3 g, dim3 b, F kernel) {
    gridDim = g; blockDim = b;
    for (unsigned bz = 0; bz < g.z; ++bz)
        for (unsigned by = 0; by < g.y; ++by)
            for (unsigned bx = 0; bx < g.x; ++bx)
                for (unsigned ty = 0; ty < b.y; ++ty)
                    for (unsigned tx = 0; tx < b.x; ++tx) { blockIdx = dim3(bx, by, bz); threadIdx = dim3(tx, ty, 0); kernel(); }
}

template <class F>
static void launch_threads(dim3 g, dim3 b, F kernel) {
    gridDim = g; blockDim = b;
    std::barrier<> bar(b.x);
    block_barrier = &bar;
    for (unsigned bx = 0; bx < g.x; ++bx) {
        std::vector<std::thread> threads;
        for (unsigned tx = 0; tx < b.x; ++tx) threads.emplace_back([=] { blockIdx = dim3(bx, 0, 0); threadIdx = dim3(tx, 0, 0); kernel(); });
        for (auto& t : threads) t.join();
    }
}

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
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    fclose(f);
    AffineTable tab = {};
    f = fopen(argv[7], "rb");
    if (!f || fread(&tab.v[0][0], 8, (size_t)K * 6, f) != (size_t)K * 6) return 2;
    fclose(f);
    std::vector<int> out((size_t)n * K * H * W);                // 4-byte elements either way
    // the launch sequence of uad_affine_spline3
    const int pad = zoom_pad(boundary);
    std::vector<double> coef((size_t)n * (h + 2 * pad) * (w + 2 * pad));
    double* c = coef.data();
    void* dst = out.data();
    if (pad) prefilter<PREFILTER_REFLECT>(in.data(), n, h, w, pad, c);
    else prefilter<PREFILTER_MIRROR>(in.data(), n, h, w, pad, c);
    launch_loop(dim3((W + 15) / 16, (H + 15) / 16, n < 2 ? n : 2), dim3(16, 16), [&] { affine_interp_kernel(c, n, K, pad, h, w, H, W, tab, out_kind, dst); });
    f = fopen(argv[11], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 3;
    fclose(f);
    return 0;
}
