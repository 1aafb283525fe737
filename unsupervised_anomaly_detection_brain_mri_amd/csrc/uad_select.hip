// Order statistics on the device without a sort (reference utils/NII.py:50-66 -- np.percentile(0 / 99.8) + max of a volume --,
// dataloaders/MSLUB.py:161 -- np.percentile(slice, 90) per slice --, utils/Evaluation.py:205 -- np.quantile(volume, 0.9) -- and :404-408 --
// np.percentile(variances >= 0, 99.8) + a 50-bin np.histogram).
//   1. select_pass_kernel  segmented radix SELECT: four passes over the 8-bit digits of uad_eval.hip's order-preserving key, most significant
//                          first.  A workgroup streams one tile of one segment (16-byte loads), counts the digit of every element whose higher
//                          digits equal a target's prefix into per-wave LDS histograms and folds them into the segment's global counters with
//                          integer atomics.  The last workgroup of a segment to arrive (ticket) scans the 256 bins per target, fixes the
//                          target's next digit and remaining rank, and zeroes the counters for the next pass.  Pass 0 counts every element that
//                          passes the filter, so its total is m and the target ranks are formed from it there: the bracket of numpy's 'linear'
//                          virtual index (m - 1) * q, in the float type numpy forms it in (one multiply, no contraction).
//                          No key array, no scatter, no second copy: 4 x 4 B x n of HBM reads per call, and integer atomics only, so the
//                          result is bit-reproducible and a segment's result does not depend on its neighbours.
//                          uad_select_quantiles_masked (utils/utils.py:44-50 under utils/Evaluation.py:399-402: the values of ONE class inside
//                          a value range, numpy's `a[keep]` of bins='auto') is the MASKED instantiation of the same kernel: the filter is
//                          labels[i] == class_id && lo <= v <= hi, everything after the filter is shared.
//   2. hist_edges_kernel   histogram over a caller-given edge table (binary search in LDS), per-wave LDS histograms, 64-bit integer atomics.
//   3. clamp_scale_kernel  out = clamp(v, lo, hi) * s as numpy's `v[v < lo] = lo; v[v > hi] = hi; v * s` writes it.
// Bandwidth- and latency-shaped work: no matrix cores, vector stores only.
#include <cmath>
#include <cstdint>

#include "uad_kernels.h"
#include "../../include/uad_hip.h"

#pragma clang fp contract(off)

#define fail uad_fail

namespace {

constexpr int SEL_THREADS = 256, SEL_WAVES = SEL_THREADS / 64, SEL_ROUNDS = 8;
constexpr int SEL_TILE = SEL_THREADS * 4 * SEL_ROUNDS;          // 8192 elements per workgroup
constexpr int SEL_TARGETS = 2 * UAD_SELECT_MAX_Q;               // a lower and an upper bracket per quantile
static_assert(SEL_TILE == UAD_SELECT_TILE, "include/uad_hip.h states the tile");

// per-segment state, written by the segment's last arriver of pass p and read by every workgroup of pass p + 1 (the next launch)
struct SelState {
    unsigned long long rank[SEL_TARGETS];   // rank of the target among the elements that share its prefix
    unsigned long long m;                   // elements that pass the filter
    unsigned prefix[SEL_TARGETS];           // the digits fixed so far (right-aligned)
    int slot[SEL_TARGETS];                  // targets with equal prefixes share the histogram of the first of them; -1: no target (m == 0)
    unsigned ticket;
    unsigned pad[5];
};
static_assert(sizeof(SelState) % 16 == 0, "the counters behind the states stay 16-byte aligned");

// the MASKED instantiation's filter (unused by the other one)
struct SelMask {
    const uint8_t* labels;
    float lo, hi;
    int class_id;
};

struct SelQ {
    double q[UAD_SELECT_MAX_Q];
    unsigned f32_mask;                      // bit j: numpy forms the virtual index of q[j] in float32
    int k;
};

// uad_eval.hip's f2key, with -0 folded onto +0 (they compare equal in numpy; the >= 0 filter becomes key >= 0x80000000)
__device__ __forceinline__ unsigned sel_key(float f) {
    unsigned u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_key_to_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// exclusive scan of one value per thread over the 256 threads (Hillis-Steele in LDS); *total = the sum
__device__ __forceinline__ unsigned long long scan256(unsigned long long v, unsigned long long* buf, unsigned long long* total) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < SEL_THREADS; d <<= 1) {
        const unsigned long long add = t >= d ? buf[t - d] : 0ull;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const unsigned long long incl = buf[t];
    *total = buf[SEL_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// the two order-statistic indices numpy's _get_indexes takes for the virtual index (m - 1) * q, in numpy's float type
__device__ __forceinline__ void bracket_ranks(unsigned long long m, double q, bool f32, unsigned long long* lo, unsigned long long* hi) {
    const long long last = (long long)m - 1;
    long long p, n;
    if (f32) {
        const float lastf = (float)(double)last;
        const float v = lastf * (float)q;
        if (v >= lastf) { p = n = last; }
        else { const float pf = floorf(v); p = (long long)pf; n = (long long)(pf + 1.0f); }
    } else {
        const double lastd = (double)last;
        const double v = lastd * q;
        if (v >= lastd) { p = n = last; }
        else { const double pd = floor(v); p = (long long)pd; n = (long long)(pd + 1.0); }
    }
    p = p < 0 ? 0 : (p > last ? last : p);
    n = n < 0 ? 0 : (n > last ? last : n);
    *lo = (unsigned long long)p;
    *hi = (unsigned long long)n;
}

template <bool MASKED>
__global__ void __launch_bounds__(SEL_THREADS) select_pass_kernel(const float* __restrict__ in, unsigned long long n_per_seg, int pass, int filter,
                                                                  SelQ qs, SelState* __restrict__ states, unsigned* __restrict__ counts,
                                                                  long long* __restrict__ out_m, float* __restrict__ out_vals, SelMask mk) {
    __shared__ unsigned hist[SEL_WAVES][SEL_TARGETS][256];       // 32 KB
    __shared__ unsigned long long scan_buf[SEL_THREADS];
    __shared__ unsigned long long s_rank[SEL_TARGETS];
    __shared__ unsigned s_prefix[SEL_TARGETS];
    __shared__ int s_slot[SEL_TARGETS];
    __shared__ int s_last;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned seg = blockIdx.y;
    const int nt = 2 * qs.k;
    SelState* st = states + seg;
    unsigned* cnt = counts + (size_t)seg * SEL_TARGETS * 256;

    // ---- this pass's targets: pass 0 has one histogram (slot 0) of everything that passes the filter
    unsigned prefix[SEL_TARGETS];
    bool owner[SEL_TARGETS];
#pragma unroll
    for (int k = 0; k < SEL_TARGETS; ++k) {
        prefix[k] = pass == 0 ? 0u : st->prefix[k];
        owner[k] = pass == 0 ? k == 0 : (k < nt && st->slot[k] == k);
    }
    for (int i = t; i < SEL_WAVES * SEL_TARGETS * 256; i += SEL_THREADS) (&hist[0][0][0])[i] = 0u;
    __syncthreads();

    // ---- stream the tile.  Chunks of four floats are taken relative to the 16-byte boundary at or below the segment's first element;
    // a chunk that lies wholly inside the segment is one 16-byte load, the (at most two) partial ones are guarded scalar loads.
    const float* seg_base = in + (size_t)seg * n_per_seg;
    const unsigned long long off = ((uintptr_t)seg_base >> 2) & 3u;
    const float* aligned = seg_base - off;
    const unsigned long long end = off + n_per_seg;
    const int shift = 24 - 8 * pass;
    const unsigned min_key = filter == UAD_SELECT_NONNEG ? 0x80000000u : 0u;
#pragma unroll 2
    for (int r = 0; r < SEL_ROUNDS; ++r) {
        const unsigned long long j0 = ((unsigned long long)blockIdx.x * (SEL_TILE / 4) + (unsigned long long)r * SEL_THREADS + t) * 4ull;
        float v[4];
        bool ok[4];
        if (j0 >= off && j0 + 4 <= end) {
            const float4 x = *reinterpret_cast<const float4*>(aligned + j0);
            v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            ok[0] = ok[1] = ok[2] = ok[3] = true;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ok[e] = j0 + e >= off && j0 + e < end;
                v[e] = ok[e] ? aligned[j0 + e] : 0.f;
            }
        }
        if constexpr (MASKED) {
            // one segment: element j of the aligned index space is value j - off, and so is its class id (read only where the value was)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                ok[e] = ok[e] && mk.labels[j0 + e - off] == (uint8_t)mk.class_id && v[e] >= mk.lo && v[e] <= mk.hi;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned key = sel_key(v[e]);
            const bool pass_f = ok[e] && key >= min_key;
            const unsigned dgt = (key >> shift) & 255u;
            const unsigned hi_digits = pass == 0 ? 0u : key >> (shift + 8);
#pragma unroll
            for (int k = 0; k < SEL_TARGETS; ++k) {
                if (!owner[k]) continue;                          // wave-uniform
                const bool hit = pass_f && hi_digits == prefix[k];
                const unsigned long long hits = __ballot(hit);
                if (hits == 0ull) continue;
                // runs of equal values (the zero background of a skull-stripped volume): one add for the wave instead of 64 to one address
                const unsigned first = __shfl(dgt, __ffsll((long long)hits) - 1);
                if (__ballot(hit && dgt == first) == hits) {
                    if (lane == 0) hist[wave][k][first] += (unsigned)__popcll(hits);
                } else if (hit) {
                    atomicAdd(&hist[wave][k][dgt], 1u);
                }
            }
        }
    }
    __syncthreads();
    // ---- fold: thread t owns bin t
#pragma unroll
    for (int k = 0; k < SEL_TARGETS; ++k) {
        if (!owner[k]) continue;
        unsigned c = 0;
#pragma unroll
        for (int w = 0; w < SEL_WAVES; ++w) c += hist[w][k][t];
        if (c) atomicAdd(&cnt[k * 256 + t], c);
    }
    // ---- ticket: every wave's counter adds are performed before the workgroup's arrival is
    __threadfence();
    __syncthreads();
    if (t == 0) {
        const unsigned arrived = __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = arrived == gridDim.x - 1;
        if (last) __hip_atomic_store(&st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = last ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

    // ---- the segment's last arriver: read and zero the counters (atomic exchange: performed where the adds were), fix the next digit
    unsigned long long rank[SEL_TARGETS];
    int slot[SEL_TARGETS];
#pragma unroll
    for (int k = 0; k < SEL_TARGETS; ++k) {
        rank[k] = pass == 0 ? 0ull : st->rank[k];
        slot[k] = pass == 0 ? 0 : st->slot[k];
    }
    if (t < SEL_TARGETS) { s_prefix[t] = 0u; s_rank[t] = 0ull; s_slot[t] = -1; }
    __syncthreads();
    unsigned long long m = pass == 0 ? 0ull : st->m;
#pragma unroll 1
    for (int s = 0; s < SEL_TARGETS; ++s) {
        if (!(pass == 0 ? s == 0 : (s < nt && slot[s] == s))) continue;        // uniform over the workgroup
        const unsigned long long c = atomicExch(&cnt[s * 256 + t], 0u);
        unsigned long long total;
        const unsigned long long excl = scan256(c, scan_buf, &total);
        if (pass == 0) {
            m = total;
            if (m > 0) {
#pragma unroll
                for (int j = 0; j < UAD_SELECT_MAX_Q; ++j) {
                    if (j >= qs.k) break;
                    bracket_ranks(m, qs.q[j], (qs.f32_mask >> j) & 1u, &rank[2 * j], &rank[2 * j + 1]);
                }
            }
        }
        if (total == 0) continue;                                              // m == 0: no target
#pragma unroll
        for (int k = 0; k < SEL_TARGETS; ++k) {
            if (k >= nt || slot[k] != s) continue;
            if (excl <= rank[k] && rank[k] < excl + c) {
                s_prefix[k] = (prefix[k] << 8) | (unsigned)t;
                s_rank[k] = rank[k] - excl;
                s_slot[k] = k;
            }
        }
    }
    __syncthreads();
    if (t == 0) {
        for (int k = 0; k < nt; ++k) {                                         // equal prefixes share the first one's histogram
            if (s_slot[k] < 0) continue;
            for (int j = 0; j < k; ++j)
                if (s_slot[j] == j && s_prefix[j] == s_prefix[k]) { s_slot[k] = j; break; }
        }
        for (int k = 0; k < SEL_TARGETS; ++k) {
            st->prefix[k] = s_prefix[k];
            st->rank[k] = s_rank[k];
            st->slot[k] = s_slot[k];
        }
        st->m = m;
        if (pass == 3) {
            out_m[seg] = (long long)m;
            for (int k = 0; k < nt; ++k)
                out_vals[(size_t)seg * nt + k] = s_slot[k] < 0 ? __uint_as_float(0x7fc00000u) : sel_key_to_float(s_prefix[k]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------
constexpr int HE_THREADS = 256, HE_WAVES = HE_THREADS / 64, HE_MAX_BLOCKS = 2048;

// bin of v in the edge table e[0 .. bins]: the last i < bins with e[i] <= v, provided v <= e[bins]; -1 otherwise (NaN included)
__device__ __forceinline__ int edge_bin(const float* e, int bins, float v) {
    if (!(v >= e[0]) || !(v <= e[bins])) return -1;
    int lo = 0, hi = bins;                 // invariant: e[lo] <= v, and (hi == bins or e[hi] > v)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(HE_THREADS) hist_edges_kernel(const float* __restrict__ in, unsigned long long n, const float* __restrict__ edges,
                                                                int bins, unsigned long long* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned he_smem[];
    float* e = reinterpret_cast<float*>(he_smem);                              // [bins + 1], padded to a multiple of 4
    unsigned* h = he_smem + ((bins + 1 + 3) & ~3);                             // [HE_WAVES][bins]
    const int t = threadIdx.x, wave = t >> 6;
    for (int i = t; i <= bins; i += HE_THREADS) e[i] = edges[i];
    for (int i = t; i < HE_WAVES * bins; i += HE_THREADS) h[i] = 0u;
    __syncthreads();
    unsigned* hw = h + wave * bins;
    const unsigned long long off = ((uintptr_t)in >> 2) & 3u;
    const float* aligned = in - off;
    const unsigned long long end = off + n, chunks = (end + 3) / 4;
    for (unsigned long long c = (unsigned long long)blockIdx.x * HE_THREADS + t; c < chunks; c += (unsigned long long)gridDim.x * HE_THREADS) {
        const unsigned long long j0 = c * 4ull;
        if (j0 >= off && j0 + 4 <= end) {
            const float4 x = *reinterpret_cast<const float4*>(aligned + j0);
            const float v[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int b = edge_bin(e, bins, v[k]);
                if (b >= 0) atomicAdd(&hw[b], 1u);
            }
        } else {
            for (int k = 0; k < 4; ++k) {
                if (j0 + k < off || j0 + k >= end) continue;
                const int b = edge_bin(e, bins, aligned[j0 + k]);
                if (b >= 0) atomicAdd(&hw[b], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = t; i < bins; i += HE_THREADS) {
        unsigned long long c = 0;
        for (int w = 0; w < HE_WAVES; ++w) c += h[w * bins + i];
        if (c) atomicAdd(&counts[i], c);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float clamp_scale1(float v, float lo, float hi, float s) {
    v = v < lo ? lo : v;            // numpy: v[v < lo] = lo (a -0 above a +0 bound stays -0)
    v = v > hi ? hi : v;
    return v * s;
}
// vec: in and out are 16-byte aligned -- n / 4 chunks of four and a scalar tail
__global__ void __launch_bounds__(256) clamp_scale_kernel(const float* in, unsigned long long n, float lo, float hi, float s, float* out, int vec) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256, g = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (vec) {
        const unsigned long long chunks = n / 4;
        for (unsigned long long c = g; c < chunks; c += stride) {
            float4 x = reinterpret_cast<const float4*>(in)[c];
            x.x = clamp_scale1(x.x, lo, hi, s); x.y = clamp_scale1(x.y, lo, hi, s);
            x.z = clamp_scale1(x.z, lo, hi, s); x.w = clamp_scale1(x.w, lo, hi, s);
            reinterpret_cast<float4*>(out)[c] = x;
        }
        const unsigned long long i = chunks * 4 + g;
        if (i < n) out[i] = clamp_scale1(in[i], lo, hi, s);
    } else {
        for (unsigned long long i = g; i < n; i += stride) out[i] = clamp_scale1(in[i], lo, hi, s);
    }
}

inline unsigned long long select_tiles(unsigned long long n_per_seg) { return (n_per_seg + 3 + SEL_TILE - 1) / SEL_TILE; }   // + 3: the alignment head

}  // namespace

extern "C" {

size_t uad_select_workspace(int n_seg) {
    if (n_seg <= 0) return 0;
    return (size_t)n_seg * (sizeof(SelState) + (size_t)SEL_TARGETS * 256 * sizeof(unsigned));
}

int uad_select_quantiles(const float* in, int n_seg, long long n_per_seg, const double* q, int k, unsigned f32_index_mask, int filter,
                         long long* m_out, float* bracket_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!in || !q || !m_out || !bracket_out || !workspace) return fail(UAD_ERR_INVALID, "select_quantiles: bad arguments");
    if (n_seg <= 0 || n_seg > 65535) return fail(UAD_ERR_INVALID, "select_quantiles: 1 .. 65535 segments, got %d", n_seg);
    if (n_per_seg <= 0 || n_per_seg > 0x7fffffffLL) return fail(UAD_ERR_INVALID, "select_quantiles: 1 .. 2^31 - 1 values per segment, got %lld", n_per_seg);
    if (k <= 0 || k > UAD_SELECT_MAX_Q) return fail(UAD_ERR_INVALID, "select_quantiles: 1 .. %d quantiles, got %d", UAD_SELECT_MAX_Q, k);
    if (filter != UAD_SELECT_ALL && filter != UAD_SELECT_NONNEG) return fail(UAD_ERR_INVALID, "select_quantiles: unknown filter %d", filter);
    if (((uintptr_t)in & 3) != 0) return fail(UAD_ERR_INVALID, "select_quantiles: input must be 4-byte aligned");
    SelQ qs;
    qs.k = k;
    qs.f32_mask = f32_index_mask;
    for (int j = 0; j < UAD_SELECT_MAX_Q; ++j) {
        qs.q[j] = j < k ? q[j] : 0.0;
        if (!(qs.q[j] >= 0.0 && qs.q[j] <= 1.0)) return fail(UAD_ERR_INVALID, "select_quantiles: q[%d] = %g is outside [0, 1]", j, qs.q[j]);
    }
    const size_t need = uad_select_workspace(n_seg);
    if (workspace_bytes < need) return fail(UAD_ERR_INVALID, "select_quantiles: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if (((uintptr_t)workspace & 15) != 0) return fail(UAD_ERR_INVALID, "select_quantiles: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    SelState* states = (SelState*)workspace;
    unsigned* counts = (unsigned*)(states + n_seg);
    // tickets and counters start every call at zero whatever the workspace held; between the passes the last arrivers keep them there
    HIP_TRY(hipMemsetAsync(workspace, 0, need, st));
    const dim3 grid((unsigned)select_tiles((unsigned long long)n_per_seg), (unsigned)n_seg);
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(select_pass_kernel<false>, grid, dim3(SEL_THREADS), 0, st, in, (unsigned long long)n_per_seg, pass, filter, qs, states, counts,
                           m_out, bracket_out, SelMask{nullptr, 0.f, 0.f, 0});
        HIP_TRY(hipGetLastError());
    }
    return UAD_OK;
}

int uad_select_quantiles_masked(const float* in, const uint8_t* labels, long long n, int class_id, float lo, float hi, const double* q, int k,
                                unsigned f32_index_mask, long long* m_out, float* bracket_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!in || !labels || !q || !m_out || !bracket_out || !workspace) return fail(UAD_ERR_INVALID, "select_quantiles_masked: bad arguments");
    if (n <= 0 || n > 0x7fffffffLL) return fail(UAD_ERR_INVALID, "select_quantiles_masked: 1 .. 2^31 - 1 values, got %lld", n);
    if (k <= 0 || k > UAD_SELECT_MAX_Q) return fail(UAD_ERR_INVALID, "select_quantiles_masked: 1 .. %d quantiles, got %d", UAD_SELECT_MAX_Q, k);
    if (class_id < 0 || class_id > 255) return fail(UAD_ERR_INVALID, "select_quantiles_masked: class ids are 0 .. 255, got %d", class_id);
    if (!(lo <= hi)) return fail(UAD_ERR_INVALID, "select_quantiles_masked: the range [%g, %g] is empty or not a number", (double)lo, (double)hi);
    if (((uintptr_t)in & 3) != 0) return fail(UAD_ERR_INVALID, "select_quantiles_masked: input must be 4-byte aligned");
    SelQ qs;
    qs.k = k;
    qs.f32_mask = f32_index_mask;
    for (int j = 0; j < UAD_SELECT_MAX_Q; ++j) {
        qs.q[j] = j < k ? q[j] : 0.0;
        if (!(qs.q[j] >= 0.0 && qs.q[j] <= 1.0)) return fail(UAD_ERR_INVALID, "select_quantiles_masked: q[%d] = %g is outside [0, 1]", j, qs.q[j]);
    }
    const size_t need = uad_select_workspace(1);
    if (workspace_bytes < need) return fail(UAD_ERR_INVALID, "select_quantiles_masked: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if (((uintptr_t)workspace & 15) != 0) return fail(UAD_ERR_INVALID, "select_quantiles_masked: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    SelState* states = (SelState*)workspace;
    unsigned* counts = (unsigned*)(states + 1);
    HIP_TRY(hipMemsetAsync(workspace, 0, need, st));
    const dim3 grid((unsigned)select_tiles((unsigned long long)n), 1u);
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(select_pass_kernel<true>, grid, dim3(SEL_THREADS), 0, st, in, (unsigned long long)n, pass, (int)UAD_SELECT_ALL, qs, states, counts,
                           m_out, bracket_out, SelMask{labels, lo, hi, class_id});
        HIP_TRY(hipGetLastError());
    }
    return UAD_OK;
}

int uad_histogram_edges(const float* in, long long n, const float* edges, int bins, long long* counts, void* stream) {
    if (!edges || !counts || (!in && n > 0)) return fail(UAD_ERR_INVALID, "histogram_edges: bad arguments");
    if (n < 0 || n > (1LL << 40)) return fail(UAD_ERR_INVALID, "histogram_edges: 0 .. 2^40 values, got %lld", n);
    if (bins <= 0 || bins > UAD_HISTOGRAM_MAX_BINS) return fail(UAD_ERR_INVALID, "histogram_edges: 1 .. %d bins, got %d", UAD_HISTOGRAM_MAX_BINS, bins);
    if (((uintptr_t)in & 3) != 0) return fail(UAD_ERR_INVALID, "histogram_edges: input must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(counts, 0, (size_t)bins * sizeof(long long), st));
    if (n == 0) return UAD_OK;
    const unsigned long long chunks = ((unsigned long long)n + 3 + 3) / 4;
    unsigned long long blocks = (chunks + HE_THREADS - 1) / HE_THREADS;
    if (blocks > HE_MAX_BLOCKS) blocks = HE_MAX_BLOCKS;
    const size_t lds = ((size_t)((bins + 1 + 3) & ~3) + (size_t)HE_WAVES * bins) * sizeof(unsigned);
    hipLaunchKernelGGL(hist_edges_kernel, dim3((unsigned)blocks), dim3(HE_THREADS), lds, st, in, (unsigned long long)n, edges, bins,
                       (unsigned long long*)counts);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

int uad_clamp_scale(const float* in, long long n, float lo, float hi, float scale, float* out, void* stream) {
    if (n < 0 || ((!in || !out) && n > 0)) return fail(UAD_ERR_INVALID, "clamp_scale: bad arguments");
    if (n == 0) return UAD_OK;
    const int vec = (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    const unsigned long long items = vec ? (unsigned long long)n / 4 + 3 : (unsigned long long)n;
    unsigned long long blocks = (items + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(clamp_scale_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, (unsigned long long)n, lo, hi, scale, out, vec);
    HIP_TRY(hipGetLastError());
    return UAD_OK;
}

}  // extern "C"
