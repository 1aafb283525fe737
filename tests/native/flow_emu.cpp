// Host emulation of uad_curvature_flow (tests/test_flow_kernels_host.py): the kernel source of csrc/uad_flow.hip is compiled for the CPU
// (with -ffp-contract=off, as the device build) behind the shim below.  Workgroups run one after the other; the threads of a workgroup
// are real threads around a std::barrier, because flow_sweep_kernel synchronises once a plane.  Driven by the library's own launch
// geometry (flow_grid / flow_block) and the ping-pong of uad_curvature_flow between the output and one workspace volume.
//   flow_emu in.bin in_is_f32 nz ny nx sx sy sz time_step iterations out.f64
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
#define UAD_FLOW_HOST_EMULATION
#include "../../unsupervised_anomaly_detection_brain_mri_amd/csrc/uad_flow.hip"

template <class F>
static void launch_threads(dim3 g, dim3 b, F kernel) {
    gridDim = g; blockDim = b;
    std::barrier<> bar(b.x * b.y);
    block_barrier = &bar;
    for (unsigned bz = 0; bz < g.z; ++bz)
        for (unsigned by = 0; by < g.y; ++by)
            for (unsigned bx = 0; bx < g.x; ++bx) {
                std::vector<std::thread> threads;
                for (unsigned ty = 0; ty < b.y; ++ty)
                    for (unsigned tx = 0; tx < b.x; ++tx)
                        threads.emplace_back([=] { blockIdx = dim3(bx, by, bz); threadIdx = dim3(tx, ty, 0); kernel(); });
                for (auto& t : threads) t.join();
            }
}

template <class T>
static void sweep(const T* src, int nz, int ny, int nx, const FlowScale& sc, double* dst) {
    launch_threads(flow_grid(nz, ny, nx), flow_block(), [&] { flow_sweep_kernel<T>(src, nz, ny, nx, sc, dst); });
}

int main(int argc, char** argv) {
    if (argc != 12) return 1;
    const int f32 = atoi(argv[2]), nz = atoi(argv[3]), ny = atoi(argv[4]), nx = atoi(argv[5]), iterations = atoi(argv[10]);
    if (nz <= 0 || ny <= 0 || nx <= 0 || iterations < 0) return 1;
    const size_t count = (size_t)nz * ny * nx;
    std::vector<double> in64(f32 ? 0 : count);
    std::vector<float> in32(f32 ? count : 0);
    FILE* f = fopen(argv[1], "rb");
    if (!f || (f32 ? fread(in32.data(), 4, count, f) : fread(in64.data(), 8, count, f)) != count) return 2;
    fclose(f);
    FlowScale sc;
    for (int i = 0; i < 3; ++i) sc.a[i] = 1.0 / strtod(argv[6 + i], nullptr);
    sc.time_step = strtod(argv[9], nullptr);
    std::vector<double> outv(count), wsv(count);
    double *out = outv.data(), *ws = wsv.data();
    // the launch sequence of uad_curvature_flow
    if (iterations == 0) {
        gridDim = dim3(1); blockDim = dim3(256);
        for (unsigned t = 0; t < 256; ++t) {
            blockIdx = dim3(0); threadIdx = dim3(t);
            if (f32) flow_copy_kernel<float>(in32.data(), count, out);
            else flow_copy_kernel<double>(in64.data(), count, out);
        }
    } else {
        double* dst = (iterations - 1) % 2 == 0 ? out : ws;
        if (f32) sweep(in32.data(), nz, ny, nx, sc, dst);
        else sweep(in64.data(), nz, ny, nx, sc, dst);
        for (int j = 1; j < iterations; ++j) {
            double* next = dst == out ? ws : out;
            sweep((const double*)dst, nz, ny, nx, sc, next);
            dst = next;
        }
    }
    f = fopen(argv[11], "wb");
    if (!f || fwrite(out, 8, count, f) != count) return 3;
    fclose(f);
    return 0;
}
