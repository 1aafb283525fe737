// Curvature-flow denoising of a volume on the device: nii.denoise() of the reference (utils/NII.py:85-87,
// sitk.CurvatureFlow(timeStep=0.125, numberOfIterations=3); called by dataloaders/MSLUB.py:242, MSISBI2015.py:231, MSSEG2008.py:241,246).
// The arithmetic is ITK's CurvatureFlowFunction::ComputeUpdate + DenseFiniteDifferenceImageFilter::ApplyUpdate as utils/curvature_flow.py
// states it: a 19-point stencil in fp64, a Jacobi sweep per iteration, neighbours clamped per axis.  It has not been compared with SimpleITK's
// own output.  Every operation is one IEEE add, multiply or divide in the order of the host statement; this file is compiled with
// -ffp-contract=off (build.py) and carries the pragma below, so that no multiply-add is fused and host and device agree bit for bit.
//
// flow_sweep_kernel, one launch per iteration, ping-pong between two fp64 volumes:
//   a workgroup of FLOW_TX x FLOW_TY threads owns one (y, x) tile and marches FLOW_ZC planes of z.  The tile of a plane plus a one-voxel
//   halo lives in LDS; four plane slots form a ring -- three live planes (z - 1, z, z + 1) and the one the next step fills -- so that one
//   barrier a plane suffices: the slot written in step k was last read in step k - 2, and the barrier of step k - 1 lies between.
//   Halo cells are loaded with CLAMPED global indices, which is the boundary rule; the loads of plane z + 2 are issued into registers before
//   the arithmetic of plane z and stored to LDS after it.  A lane is an x position: the 32 lanes of a half-wave read 256 contiguous bytes
//   of one LDS row whatever the tap offset, which covers the 64 banks once (ds_read_b64: no conflict).
// tests/native/flow_emu.cpp compiles the kernels of this file for the HOST (UAD_HOST_EMULATION: hip_host_emu.h supplies threadIdx & co., the
// launch layer at the end of the file is left out).
#include <cmath>
#include <cstddef>

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)   // a compile that is not a HIP one is a host emulation too
#include "uad_kernels.h"
#endif
#include "../../include/uad_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int FLOW_TX = 32;        // tile edge along x (lanes): one LDS row of a half-wave
constexpr int FLOW_TY = 8;         // tile edge along y
constexpr int FLOW_ZC = 16;        // planes of z a workgroup marches
constexpr int FLOW_THREADS = FLOW_TX * FLOW_TY;
constexpr int FLOW_LW = FLOW_TX + 2, FLOW_LH = FLOW_TY + 2;      // tile + halo
constexpr int FLOW_CELLS = FLOW_LW * FLOW_LH;
constexpr int FLOW_PER_THREAD = (FLOW_CELLS + FLOW_THREADS - 1) / FLOW_THREADS;
constexpr int FLOW_SLOTS = 4;
static_assert((FLOW_TX & (FLOW_TX - 1)) == 0 && (FLOW_TY & (FLOW_TY - 1)) == 0 && FLOW_TX <= 64 && FLOW_TY <= 64, "tile edges: powers of two <= 64");

struct FlowScale {
    double a[3];                   // 1 / spacing: x, y, z
    double time_step;
};

__device__ __forceinline__ int flow_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the halo cells this thread owns, of plane z (clamped), into registers
template <class T>
__device__ __forceinline__ void flow_fetch(const T* __restrict__ src, int nz, int ny, int nx, int z, int y0, int x0, int tid, double (&r)[FLOW_PER_THREAD]) {
    const size_t plane = (size_t)flow_clamp(z, nz - 1) * (size_t)ny;
#pragma unroll
    for (int k = 0; k < FLOW_PER_THREAD; ++k) {
        const int cell = tid + k * FLOW_THREADS;
        if (cell < FLOW_CELLS) {
            const int ly = cell / FLOW_LW, lx = cell - ly * FLOW_LW;
            const int y = flow_clamp(y0 + ly - 1, ny - 1), x = flow_clamp(x0 + lx - 1, nx - 1);
            r[k] = (double)src[(plane + (size_t)y) * (size_t)nx + (size_t)x];
        }
    }
}

__device__ __forceinline__ void flow_stash(double* slot, int tid, const double (&r)[FLOW_PER_THREAD]) {
#pragma unroll
    for (int k = 0; k < FLOW_PER_THREAD; ++k) {
        const int cell = tid + k * FLOW_THREADS;
        if (cell < FLOW_CELLS) slot[cell] = r[k];
    }
}

template <class T>
__global__ __launch_bounds__(FLOW_THREADS) void flow_sweep_kernel(const T* __restrict__ src, int nz, int ny, int nx, FlowScale sc, double* __restrict__ dst) {
    __shared__ double tile[FLOW_SLOTS][FLOW_CELLS];
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * FLOW_TX + tx;
    const int x0 = blockIdx.x * FLOW_TX, y0 = blockIdx.y * FLOW_TY, z0 = blockIdx.z * FLOW_ZC;
    const int planes = nz - z0 < FLOW_ZC ? nz - z0 : FLOW_ZC;
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < nx && y < ny;
    const int at = (ty + 1) * FLOW_LW + (tx + 1);
    const double ax = sc.a[0], ay = sc.a[1], az = sc.a[2];
    double r[FLOW_PER_THREAD];
    flow_fetch(src, nz, ny, nx, z0 - 1, y0, x0, tid, r);
    flow_stash(tile[0], tid, r);
    flow_fetch(src, nz, ny, nx, z0, y0, x0, tid, r);
    flow_stash(tile[1], tid, r);
    flow_fetch(src, nz, ny, nx, z0 + 1, y0, x0, tid, r);
    for (int k = 0; k < planes; ++k) {
        flow_stash(tile[(k + 2) & 3], tid, r);
        __syncthreads();
        if (k + 1 < planes) flow_fetch(src, nz, ny, nx, z0 + k + 2, y0, x0, tid, r);
        const double* lo = tile[k & 3] + at;            // plane z - 1
        const double* mid = tile[(k + 1) & 3] + at;     // plane z
        const double* hi = tile[(k + 2) & 3] + at;      // plane z + 1
        const double c = mid[0], c2 = 2.0 * c;
        // i = 0 (x), 1 (y), 2 (z), in ITK's order
        const double xp = mid[1], xm = mid[-1], yp = mid[FLOW_LW], ym = mid[-FLOW_LW], zp = hi[0], zm = lo[0];
        const double f0 = (0.5 * (xp - xm)) * ax;
        const double s0 = ((xp - c2) + xm) * (ax * ax);
        const double x01 = ((0.25 * (((mid[-FLOW_LW - 1] - mid[FLOW_LW - 1]) - mid[-FLOW_LW + 1]) + mid[FLOW_LW + 1])) * ax) * ay;
        const double x02 = ((0.25 * (((lo[-1] - hi[-1]) - lo[1]) + hi[1])) * ax) * az;
        const double f1 = (0.5 * (yp - ym)) * ay;
        const double s1 = ((yp - c2) + ym) * (ay * ay);
        const double x12 = ((0.25 * (((lo[-FLOW_LW] - hi[-FLOW_LW]) - lo[FLOW_LW]) + hi[FLOW_LW])) * ay) * az;
        const double f2 = (0.5 * (zp - zm)) * az;
        const double s2 = ((zp - c2) + zm) * (az * az);
        const double mag = ((0.0 + f0 * f0) + f1 * f1) + f2 * f2;
        double upd = 0.0;
        upd = upd + ((0.0 + s1) + s2) * (f0 * f0);
        upd = upd + ((0.0 + s0) + s2) * (f1 * f1);
        upd = upd + ((0.0 + s0) + s1) * (f2 * f2);
        upd = upd - ((2.0 * f0) * f1) * x01;
        upd = upd - ((2.0 * f0) * f2) * x02;
        upd = upd - ((2.0 * f1) * f2) * x12;
        upd = mag < 1e-9 ? 0.0 : upd / mag;
        if (inside) dst[((size_t)(z0 + k) * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)x] = c + upd * sc.time_step;
    }
}

// iterations = 0: a copy, fp32 widened exactly
template <class T>
__global__ __launch_bounds__(256) void flow_copy_kernel(const T* __restrict__ src, size_t count, double* __restrict__ dst) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) dst[i] = (double)src[i];
}

// the launch geometry of one sweep (shared with the host emulation)
inline dim3 flow_grid(int nz, int ny, int nx) { return dim3((nx + FLOW_TX - 1) / FLOW_TX, (ny + FLOW_TY - 1) / FLOW_TY, (nz + FLOW_ZC - 1) / FLOW_ZC); }
inline dim3 flow_block() { return dim3(FLOW_TX, FLOW_TY); }

}  // namespace

#if defined(__HIP__) && !defined(UAD_HOST_EMULATION)
#define fail uad_fail

namespace {
template <class T>
int flow_sweep(const T* src, int nz, int ny, int nx, const FlowScale& sc, double* dst, hipStream_t st) {
    hipLaunchKernelGGL(flow_sweep_kernel<T>, flow_grid(nz, ny, nx), flow_block(), 0, st, src, nz, ny, nx, sc, dst);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}
}  // namespace

extern "C" {

size_t uad_curvature_flow_workspace(int nz, int ny, int nx) {
    if (nz <= 0 || ny <= 0 || nx <= 0) return 0;
    return (size_t)nz * (size_t)ny * (size_t)nx * sizeof(double);
}

int uad_curvature_flow(const void* in, int in_is_f32, int nz, int ny, int nx, const double spacing_xyz[3], double time_step, int iterations,
                       double* out, void* workspace, void* stream) {
    if (nz <= 0 || ny <= 0 || nx <= 0) return fail(UAD_ERR_INVALID, "curvature_flow: dimensions must be positive, got %d x %d x %d", nz, ny, nx);
    if (iterations < 0) return fail(UAD_ERR_INVALID, "curvature_flow: iterations must not be negative, got %d", iterations);
    if (!spacing_xyz) return fail(UAD_ERR_INVALID, "curvature_flow: spacing is NULL");
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(spacing_xyz[i]) || !(spacing_xyz[i] > 0.0))
            return fail(UAD_ERR_INVALID, "curvature_flow: spacing[%d] = %g is not a positive finite number", i, spacing_xyz[i]);
    if (!std::isfinite(time_step)) return fail(UAD_ERR_INVALID, "curvature_flow: time_step is not finite");
    if (!in || !out) return fail(UAD_ERR_INVALID, "curvature_flow: in / out is NULL");
    if ((const void*)out == in) return fail(UAD_ERR_INVALID, "curvature_flow: out may not alias in");
    if (iterations >= 2 && !workspace) return fail(UAD_ERR_INVALID, "curvature_flow: %d iterations need the workspace", iterations);
    if (iterations >= 2 && (workspace == (void*)out || workspace == in)) return fail(UAD_ERR_INVALID, "curvature_flow: workspace may not alias in / out");
    if ((ny + FLOW_TY - 1) / FLOW_TY > 65535 || (nz + FLOW_ZC - 1) / FLOW_ZC > 65535) return fail(UAD_ERR_UNSUPPORTED, "curvature_flow: volume too large for one grid");
    hipStream_t st = (hipStream_t)stream;
    const size_t count = (size_t)nz * (size_t)ny * (size_t)nx;
    if (iterations == 0) {
        const unsigned blocks = (unsigned)((count + 255) / 256 < 65536 ? (count + 255) / 256 : 65536);
        if (in_is_f32) hipLaunchKernelGGL(flow_copy_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)in, count, out);
        else hipLaunchKernelGGL(flow_copy_kernel<double>, dim3(blocks), dim3(256), 0, st, (const double*)in, count, out);
        HIP_TRY(hipGetLastError());
        return UAD_OK;
    }
    FlowScale sc;
    for (int i = 0; i < 3; ++i) sc.a[i] = 1.0 / spacing_xyz[i];
    sc.time_step = time_step;
    // ping-pong between `out` and the workspace, started so that the last sweep lands in `out`
    double* ws = (double*)workspace;
    double* dst = (iterations - 1) % 2 == 0 ? out : ws;
    int rc = in_is_f32 ? flow_sweep((const float*)in, nz, ny, nx, sc, dst, st) : flow_sweep((const double*)in, nz, ny, nx, sc, dst, st);
    for (int j = 1; j < iterations && rc == UAD_OK; ++j) {
        double* next = dst == out ? ws : out;
        rc = flow_sweep((const double*)dst, nz, ny, nx, sc, next, st);
        dst = next;
    }
    return rc;
}

}  // extern "C"
#endif  // UAD_HOST_EMULATION
