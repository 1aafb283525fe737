// The optimizer updates over a flat parameter buffer, TF-1.15 rules: Adam, and SGD / Momentum / RMSProp in one kernel.  Both skip their update when the
// step's fault word is set.
#include "uad_kernels.h"

namespace {

// TF-1.15 AdamOptimizer update (trainers/DLMODEL.py:112-131): lr_t is computed on the host.
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, size_t n, float lr_t, float b1, float b2, float eps, float gscale, const unsigned* __restrict__ fault) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (fault && *fault) return;      // this step's gradients are invalid (timed-out bottleneck exchange): no update; the host reports it (uad_model.hip: check_fault)
    const float gi = g[i] * gscale;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = p[i] - lr_t * mi / (sqrtf(vi) + eps);
}

// The other optimizers of DLMODEL.create_optimizer (trainers/DLMODEL.py:113-123), TF-1.15 update rules:
//   kind 1 GradientDescentOptimizer            p -= lr g
//   kind 2 MomentumOptimizer(momentum)         a = momentum a + g ; p -= lr a                        (slot a = s1, zero-initialised)
//   kind 3 RMSPropOptimizer(decay .9, momentum, eps 1e-10)   ms = decay ms + (1 - decay) g^2 ; mom = momentum mom + lr g / sqrt(ms + eps) ; p -= mom
//                                                            (slots ms = s2, ONE-initialised by TF, mom = s1)
__global__ void optim_kernel(int kind, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1, float* __restrict__ s2, size_t n,
                             float lr, float momentum, float decay, float eps, float gscale, const unsigned* __restrict__ fault) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (fault && *fault) return;
    const float gi = g[i] * gscale;
    if (kind == 1) { p[i] -= lr * gi; return; }
    if (kind == 2) { const float a = momentum * s1[i] + gi; s1[i] = a; p[i] -= lr * a; return; }
    const float ms = decay * s2[i] + (1.f - decay) * gi * gi;
    const float mom = momentum * s1[i] + lr * gi / sqrtf(ms + eps);
    s2[i] = ms; s1[i] = mom;
    p[i] -= mom;
}

}  // namespace

void uad_launch_optim(int kind, float* p, const float* g, float* s1, float* s2, size_t n, float lr, float momentum, float decay, float eps,
                      float gscale, hipStream_t st, const unsigned* fault) {
    hipLaunchKernelGGL(optim_kernel, dim3((n + 255) / 256), dim3(256), 0, st, kind, p, g, s1, s2, n, lr, momentum, decay, eps, gscale, fault);
}
void uad_launch_adam(float* p, const float* g, float* m, float* v, size_t n, float lr_t, float beta1, float beta2,
                     float eps, float gscale, hipStream_t st, const unsigned* fault) {
    hipLaunchKernelGGL(adam_kernel, dim3((n + 255) / 256), dim3(256), 0, st, p, g, m, v, n, lr_t, beta1, beta2, eps,
                       gscale, fault);
}
