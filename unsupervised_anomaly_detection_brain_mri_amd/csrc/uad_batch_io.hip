// What a step needs around the model: batch gather from the HBM-resident slice cache, the mask multiply, the counter-based noise fill (Philox, the generator
// of uad_kernels.h) and the shader-clock probe.  Built with the default contraction mode: uad_batch.hip (-ffp-contract=off) is another unit on purpose.
#include "uad_kernels.h"

namespace {

// Batch assembly from an HBM-resident slice cache: out[b] = src[idx[b]] (fp32 slices, 16-byte copies) and
// mask[b][p] = lut[labels[idx[b]][p]] (u8 label maps -> 0/1 brain masks, dataloaders/BRAINWEB.py:466-476).
__global__ void __launch_bounds__(256) gather_slices_kernel(const float* __restrict__ src, const int* __restrict__ idx,
                                                            long long slice_f4, float* __restrict__ out) {
    const int b = blockIdx.y;
    const float4* s = reinterpret_cast<const float4*>(src) + (size_t)idx[b] * slice_f4;
    float4* o = reinterpret_cast<float4*>(out) + (size_t)b * slice_f4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < slice_f4; i += (long long)gridDim.x * 256) o[i] = s[i];
}
__global__ void __launch_bounds__(256) gather_mask_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ idx,
                                                          long long slice_px, const unsigned char* __restrict__ lut,
                                                          float* __restrict__ out) {
    __shared__ float s_lut[256];
    s_lut[threadIdx.x] = lut ? (float)lut[threadIdx.x] : (float)threadIdx.x;
    __syncthreads();
    const int b = blockIdx.y;
    const unsigned char* l = labels + (size_t)idx[b] * slice_px;
    float* o = out + (size_t)b * slice_px;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < slice_px; i += (long long)gridDim.x * 256) o[i] = s_lut[l[i]];
}

__global__ void mul_kernel(const float* __restrict__ x, const float* __restrict__ mask, float* __restrict__ y, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = mask ? x[i] * mask[i] : x[i];
}

}  // namespace

void uad_launch_gather_slices(const float* src, const int* idx, int n, long long slice_elems, float* out, hipStream_t st) {
    const long long f4 = slice_elems / 4;
    int bx = (int)((f4 + 255) / 256); if (bx > 64) bx = 64; if (bx < 1) bx = 1;
    hipLaunchKernelGGL(gather_slices_kernel, dim3(bx, n), dim3(256), 0, st, src, idx, f4, out);
}
void uad_launch_gather_mask(const unsigned char* labels, const int* idx, int n, long long slice_px, const unsigned char* lut,
                            float* out, hipStream_t st) {
    int bx = (int)((slice_px + 255) / 256); if (bx > 64) bx = 64; if (bx < 1) bx = 1;
    hipLaunchKernelGGL(gather_mask_kernel, dim3(bx, n), dim3(256), 0, st, labels, idx, slice_px, lut, out);
}
void uad_launch_mul(const float* x, const float* mask, float* y, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(mul_kernel, dim3((n + 255) / 256), dim3(256), 0, st, x, mask, y, n);
}

// ------------------------------------------------------------------------------------------------
// Counter-based noise of one step (the reference draws eps / dropout masks inside the TF graph: tf.random_normal,
// keras Dropout; models/variational_autoencoder.py:34, customlayers.py / autoencoder.py dropout layers).  Philox4x32-10 keyed by
// the run seed; the counter is (element quad within the sample, GLOBAL sample index, step, stream id): a sample's noise does not
// depend on which rank draws it or on how the global batch is split, so data-parallel runs reproduce the single-process run
// (SURVEY.md section 8e).  kind 0: N(0,1) by Box-Muller on two 24-bit uniforms; kind 1: inverted-dropout keep mask
// (u >= rate ? 1/(1-rate) : 0, nn.dropout's rule).  One launch fills every array of the step (grid.y = job).
// ------------------------------------------------------------------------------------------------
namespace {
// philox4x32_10, uad_rng_quad and uad_box_muller live in uad_kernels.h: uad_batch.hip adds the same numbers to a batch
struct RngJobs { UadRngJob j[8]; };
__global__ void __launch_bounds__(256) rng_fill_kernel(RngJobs jobs, int n, unsigned k0, unsigned k1, unsigned step_lo, unsigned step_hi,
                                                       long long sample0) {
    const UadRngJob jb = jobs.j[blockIdx.y];
    const int quads = (jb.per_sample + 3) / 4;
    const long long total = (long long)n * quads;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long long)gridDim.x * blockDim.x) {
        const int s = (int)(q / quads), e4 = (int)(q % quads);
        const unsigned long long gs = (unsigned long long)(sample0 + s);
        unsigned r[4];
        uad_rng_quad((unsigned)e4, gs, step_lo, step_hi, jb.stream, k0, k1, r);
        float v[4];
        if (jb.kind == 0) {
#pragma unroll
            for (int h = 0; h < 2; ++h) uad_box_muller(r[2 * h], r[2 * h + 1], v[2 * h], v[2 * h + 1]);
        } else {
            const float keep = 1.0f / (1.0f - jb.rate);
#pragma unroll
            for (int h = 0; h < 4; ++h) v[h] = ((float)(r[h] >> 8) * 5.9604644775390625e-8f >= jb.rate) ? keep : 0.0f;
        }
        float* o = jb.out + (size_t)s * jb.per_sample + (size_t)e4 * 4;
#pragma unroll
        for (int h = 0; h < 4; ++h) if (e4 * 4 + h < jb.per_sample) o[h] = v[h];
    }
}
}  // namespace

void uad_launch_rng_fill(const UadRngJob* jobs, int njobs, int n, unsigned long long seed, unsigned long long step, long long sample0,
                         hipStream_t st) {
    RngJobs js;
    int maxq = 1;
    for (int i = 0; i < njobs; ++i) { js.j[i] = jobs[i]; const int q = (jobs[i].per_sample + 3) / 4; if (q > maxq) maxq = q; }
    long long blocks = ((long long)n * maxq + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(rng_fill_kernel, dim3((unsigned)blocks, njobs), dim3(256), 0, st, js, n, (unsigned)seed, (unsigned)(seed >> 32),
                       (unsigned)step, (unsigned)(step >> 32), sample0);
}

namespace {
// One wave that watches both clocks for `ticks` 100 MHz ticks: out[0] = shader cycles (s_memtime), out[1] = 100 MHz ticks (s_memrealtime).
// Launched on a stream of its own beside a workload it measures the clock the chip actually sustains under that load (DVFS: the 2.4 GHz the
// MFMA peaks are priced at is the ceiling, not what a power-limited kernel mix runs at).  It sleeps between samples: one wave slot, no issue pressure.
__global__ void __launch_bounds__(64) clock_probe_kernel(unsigned long long* out, unsigned long long ticks) {
    const unsigned long long r0 = wall_clock64();
    const unsigned long long c0 = (unsigned long long)clock64();
    unsigned long long r = r0;
    while (r - r0 < ticks) { __builtin_amdgcn_s_sleep(64); r = wall_clock64(); }
    const unsigned long long c1 = (unsigned long long)clock64();
    if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = r - r0; }
}
}  // namespace
void uad_launch_clock_probe(unsigned long long* out, unsigned long long ticks, hipStream_t st) {
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, st, out, ticks);
}
