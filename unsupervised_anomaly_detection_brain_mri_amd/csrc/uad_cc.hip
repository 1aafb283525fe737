// 26-connected component labelling of a binary [D,H,W] volume on the device, and the lesion-wise detection counts built on it
// (reference utils/Evaluation.py:130-172 compute_detection_rate: skimage label + regionprops in chunks of 20 slices).
//
// Union-find on ONE int32 array L that is the parent array during the passes and the label volume at the end:
//   L[v] = 0 for background, otherwise 1 + the linear index of v's parent; a root points at itself (L[r] == r + 1).
// Links only ever go to a SMALLER index (atomicMin), so every find walk is strictly decreasing and ends at a root, and the root
// of a finished component is its smallest linear index: the label is unique (no dependence on the order of the atomics) and is
// the component's first voxel in raster order, which is what regionprops(...)['coords'][0] is in the reference.
//
// Three kernels, ordered by kernel boundary on the caller's stream (no workgroup ever waits for another):
//   cc_tile_kernel    a 32 x 8 x 4 (x, y, z) tile per workgroup is resolved completely in LDS (4 KiB of parents, LDS atomicMin);
//                     every voxel leaves with the GLOBAL index of its tile-local root.  x rows of 32 floats = one 128-B line.
//   cc_merge_kernel   voxels that have a "backward" neighbour (one of the 13 with a smaller linear index) in another tile join the
//                     two trees with atomicMin on L in global memory.
//   cc_flatten_kernel every voxel walks to its root and stores it (writing a root into L[v] keeps L a valid parent array, so
//                     concurrent walkers may read either value); roots are counted.
// `slab`: two voxels are neighbours only if z / slab agrees, so groups of `slab` slices are labelled independently while the
// linear index (and with it the label) stays that of the whole volume.
#include "uad_kernels.h"
#include "../../include/uad_hip.h"

#define fail uad_fail

namespace {

constexpr int CC_TX = 32, CC_TY = 8, CC_TZ = 4, CC_TILE = CC_TX * CC_TY * CC_TZ, CC_THREADS = 256;

// ---- LDS union-find over tile-local indices (parent == own index: root; -1: background, never touched) ----
__device__ __forceinline__ int lds_find(int* p, int x) {
    int q;
    while ((q = __hip_atomic_load(&p[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != x) x = q;      // strictly decreasing
    return x;
}
__device__ __forceinline__ void lds_union(int* p, int a, int b) {
    for (;;) {                                   // every round either ends or replaces b by a strictly smaller node of its tree
        a = lds_find(p, a);
        b = lds_find(p, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&p[b], a);
        if (old == b) return;                    // b was still a root: linked
        b = old;                                 // b had been linked meanwhile (p[b] = min(old, a)): old and a are still to be joined
    }
}

// ---- the same on L in global memory, on the encoded values (index + 1) ----
__device__ __forceinline__ int g_find(int* L, int x) {
    int q;
    while ((q = __hip_atomic_load(&L[x - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x) x = q;
    return x;
}
__device__ __forceinline__ void g_union(int* L, int a, int b) {
    for (;;) {
        a = g_find(L, a);
        b = g_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[b - 1], a);
        if (old == b) return;
        b = old;
    }
}

// foreground = a != 0 (and b != 0 when b is given: the intersection volume is never materialised)
__global__ void __launch_bounds__(CC_THREADS) cc_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, int D, int H, int W,
                                                             int slab, int* __restrict__ L) {
    __shared__ int s_par[CC_TILE];
    const int x0 = blockIdx.x * CC_TX, y0 = blockIdx.y * CC_TY, z0 = blockIdx.z * CC_TZ;
    for (int i = threadIdx.x; i < CC_TILE; i += CC_THREADS) {
        const int x = x0 + (i & (CC_TX - 1)), y = y0 + ((i / CC_TX) & (CC_TY - 1)), z = z0 + i / (CC_TX * CC_TY);
        bool fg = false;
        if (x < W && y < H && z < D) {
            const size_t g = ((size_t)z * H + y) * W + x;
            fg = a[g] != 0.f && (b == nullptr || b[g] != 0.f);
        }
        s_par[i] = fg ? i : -1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CC_TILE; i += CC_THREADS) {
        if (s_par[i] < 0) continue;
        const int lx = i & (CC_TX - 1), ly = (i / CC_TX) & (CC_TY - 1), lz = i / (CC_TX * CC_TY);
        const int zs = (z0 + lz) / slab;
        // the 13 neighbours that precede this voxel in raster order
        for (int dz = -1; dz <= 0; ++dz) {
            const int nz = lz + dz;
            if (nz < 0 || (z0 + nz) / slab != zs) continue;
            for (int dy = -1; dy <= (dz < 0 ? 1 : 0); ++dy) {
                const int ny = ly + dy;
                if ((unsigned)ny >= (unsigned)CC_TY) continue;
                for (int dx = -1; dx <= ((dz < 0 || dy < 0) ? 1 : -1); ++dx) {
                    const int nx = lx + dx;
                    if ((unsigned)nx >= (unsigned)CC_TX) continue;
                    const int j = (nz * CC_TY + ny) * CC_TX + nx;
                    if (s_par[j] >= 0) lds_union(s_par, i, j);
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CC_TILE; i += CC_THREADS) {
        const int x = x0 + (i & (CC_TX - 1)), y = y0 + ((i / CC_TX) & (CC_TY - 1)), z = z0 + i / (CC_TX * CC_TY);
        if (x >= W || y >= H || z >= D) continue;
        int lab = 0;
        if (s_par[i] >= 0) {
            const int r = lds_find(s_par, i);
            const int rx = x0 + (r & (CC_TX - 1)), ry = y0 + ((r / CC_TX) & (CC_TY - 1)), rz = z0 + r / (CC_TX * CC_TY);
            lab = (rz * H + ry) * W + rx + 1;
        }
        L[((size_t)z * H + y) * W + x] = lab;
    }
}

__global__ void __launch_bounds__(CC_THREADS) cc_merge_kernel(int* L, int D, int H, int W, int slab) {
    const size_t total = (size_t)D * H * W;
    const size_t v = (size_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (v >= total || L[v] == 0) return;         // (background stays 0 and foreground never becomes 0)
    const int HW = H * W;
    const int z = (int)(v / HW), y = (int)((v - (size_t)z * HW) / W), x = (int)(v - (size_t)z * HW - (size_t)y * W);
    const int tx = x / CC_TX, ty = y / CC_TY, tz = z / CC_TZ, zs = z / slab;
    for (int dz = -1; dz <= 0; ++dz) {
        const int zz = z + dz;
        if (zz < 0 || zz / slab != zs) continue;
        for (int dy = -1; dy <= (dz < 0 ? 1 : 0); ++dy) {
            const int yy = y + dy;
            if ((unsigned)yy >= (unsigned)H) continue;
            for (int dx = -1; dx <= ((dz < 0 || dy < 0) ? 1 : -1); ++dx) {
                const int xx = x + dx;
                if ((unsigned)xx >= (unsigned)W) continue;
                if (xx / CC_TX == tx && yy / CC_TY == ty && zz / CC_TZ == tz) continue;        // joined in LDS already
                const int nb = (zz * H + yy) * W + xx;
                if (L[nb] == 0) continue;
                g_union(L, (int)v + 1, nb + 1);
            }
        }
    }
}

__global__ void __launch_bounds__(CC_THREADS) cc_flatten_kernel(int* L, size_t total, int* __restrict__ n_components) {
    __shared__ int s_roots;
    if (threadIdx.x == 0) s_roots = 0;
    __syncthreads();
    const size_t v = (size_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (v < total && L[v] != 0) {
        int x = (int)v + 1, q;
        while ((q = L[x - 1]) != x) x = q;       // ends at a root: parents are strictly smaller
        L[v] = x;
        if (n_components && x == (int)v + 1) atomicAdd(&s_roots, 1);
    }
    __syncthreads();
    if (n_components && threadIdx.x == 0 && s_roots) atomicAdd(n_components, s_roots);
}

// ---- lesion-wise counts on three finished labellings (Li: pred & gt, Lp: pred, Lg: gt) ----
__global__ void __launch_bounds__(256) dr_size_kernel(const int* __restrict__ Lp, int* __restrict__ psz, size_t total) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v < total && Lp[v] != 0) atomicAdd(&psz[Lp[v] - 1], 1);
}
// the root of an intersection component IS its first voxel: clear the predicted component (size := 0, so it can no longer reach
// min_voxels) and the ground-truth component (its root entry is negated) that contain it.  Every writer of one word writes the same value.
__global__ void __launch_bounds__(256) dr_mark_kernel(const int* __restrict__ Li, const int* __restrict__ Lp, int* Lg, int* psz, size_t total) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= total || Li[v] != (int)v + 1) return;
    psz[Lp[v] - 1] = 0;
    int rg = Lg[v];
    if (rg < 0) rg = -rg;                        // v itself may be a ground-truth root that another thread has marked already
    Lg[rg - 1] = -rg;
}
__global__ void __launch_bounds__(256) dr_count_kernel(const int* __restrict__ Li, const int* __restrict__ Lp, const int* __restrict__ Lg,
                                                       const int* __restrict__ psz, size_t total, int min_voxels,
                                                       unsigned long long* __restrict__ counts3) {
    __shared__ int s_c[3];
    if (threadIdx.x < 3) s_c[threadIdx.x] = 0;
    __syncthreads();
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v < total) {
        const int self = (int)v + 1;
        if (Li[v] == self) atomicAdd(&s_c[0], 1);
        if (Lp[v] == self && psz[v] >= min_voxels) atomicAdd(&s_c[1], 1);
        if (Lg[v] == self) atomicAdd(&s_c[2], 1);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_c[threadIdx.x]) atomicAdd(&counts3[threadIdx.x], (unsigned long long)s_c[threadIdx.x]);
}

// the three passes; n_components (device, optional) must have been zeroed by the caller
void launch_label(const float* a, const float* b, int D, int H, int W, int slab, int* L, int* n_components, hipStream_t st) {
    const size_t total = (size_t)D * H * W;
    const unsigned nb = (unsigned)((total + CC_THREADS - 1) / CC_THREADS);
    if (slab <= 0 || slab > D) slab = D;
    const dim3 tiles((W + CC_TX - 1) / CC_TX, (H + CC_TY - 1) / CC_TY, (D + CC_TZ - 1) / CC_TZ);
    hipLaunchKernelGGL(cc_tile_kernel, tiles, dim3(CC_THREADS), 0, st, a, b, D, H, W, slab, L);
    hipLaunchKernelGGL(cc_merge_kernel, dim3(nb), dim3(CC_THREADS), 0, st, L, D, H, W, slab);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(nb), dim3(CC_THREADS), 0, st, L, total, n_components);
}

int check_shape(const char* who, int D, int H, int W) {
    if (D <= 0 || H <= 0 || W <= 0) return fail(UAD_ERR_INVALID, "%s: bad arguments", who);
    const unsigned long long total = (unsigned long long)D * H * W;
    if (total >= 0x7fffffffULL) return fail(UAD_ERR_UNSUPPORTED, "%s: volume too large", who);
    if ((D + CC_TZ - 1) / CC_TZ > 65535 || (H + CC_TY - 1) / CC_TY > 65535) return fail(UAD_ERR_UNSUPPORTED, "%s: volume too large", who);
    return UAD_OK;
}

}  // namespace

extern "C" {

int uad_cc_label(const float* vol, int D, int H, int W, int slab, int* labels, int* n_components, void* stream) {
    if (!vol || !labels) return fail(UAD_ERR_INVALID, "cc_label: bad arguments");
    if (const int rc = check_shape("cc_label", D, H, W)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n_components) HIP_TRY(hipMemsetAsync(n_components, 0, sizeof(int), st));
    launch_label(vol, nullptr, D, H, W, slab, labels, n_components, st);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

int uad_detection_rate(const float* pred, const float* gt, int D, int H, int W, int slab, int min_voxels, long long* counts3, void* stream) {
    if (!pred || !gt || !counts3 || min_voxels < 1) return fail(UAD_ERR_INVALID, "detection_rate: bad arguments");
    if (const int rc = check_shape("detection_rate", D, H, W)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t total = (size_t)D * H * W;
    const unsigned nb = (unsigned)((total + 255) / 256);
    int* ws = nullptr;                           // Li | Lp | Lg | psz
    HIP_TRY(hipMalloc((void**)&ws, 4 * total * sizeof(int)));
    int *Li = ws, *Lp = ws + total, *Lg = ws + 2 * total, *psz = ws + 3 * total;
    hipError_t e = hipMemsetAsync(psz, 0, total * sizeof(int), st);
    if (e == hipSuccess) e = hipMemsetAsync(counts3, 0, 3 * sizeof(long long), st);
    if (e == hipSuccess) {
        launch_label(pred, gt, D, H, W, slab, Li, nullptr, st);
        launch_label(pred, nullptr, D, H, W, slab, Lp, nullptr, st);
        launch_label(gt, nullptr, D, H, W, slab, Lg, nullptr, st);
        hipLaunchKernelGGL(dr_size_kernel, dim3(nb), dim3(256), 0, st, (const int*)Lp, psz, total);
        hipLaunchKernelGGL(dr_mark_kernel, dim3(nb), dim3(256), 0, st, (const int*)Li, (const int*)Lp, Lg, psz, total);
        hipLaunchKernelGGL(dr_count_kernel, dim3(nb), dim3(256), 0, st, (const int*)Li, (const int*)Lp, (const int*)Lg, (const int*)psz, total, min_voxels,
                           (unsigned long long*)counts3);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);       // the workspace goes away below
    hipFree(ws);
    if (e != hipSuccess) return fail(UAD_ERR_HIP, "detection_rate: %s", hipGetErrorString(e));
    return UAD_OK;
}

}  // extern "C"
