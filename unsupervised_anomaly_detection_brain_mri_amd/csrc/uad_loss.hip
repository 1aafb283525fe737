// The loss side of the AE / VAE step: the final 1x1 conv (C -> 1) fused with the L1 loss and its backward, reparameterisation / KL and its backward, the
// step's scalar losses (loss_finalize_kernel) and the spatial autoencoder latent.  HBM-bound streams with wavefront shuffle sums and deterministic
// per-block partials (no float atomics); the partials are summed in uad_reduce.hip.
#include "uad_kernels.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Final 1x1 conv (C -> 1) + L1 loss, fused with its backward.  C/4 lanes per pixel (float4 of channels each).
// reference: models/customlayers.py:37 (dec_Conv2D_final), trainers/VAE.py:36-37,40
// ------------------------------------------------------------------------------------------------
template <bool BWD>
__global__ void __launch_bounds__(256) final_kernel(const UadFinalArgs a, int pix_per_block) {
    __shared__ float red[4][200];  // per-wave partials: 3*C+2 values, C <= 64
    const int lpp = a.C / 4;               // lanes per pixel (8 for C=32)
    const int ppp = 256 / lpp;             // pixels per pass
    const int cl = threadIdx.x % lpp, slot = threadIdx.x / lpp;
    const int n = blockIdx.y;
    const int hw = a.H * a.W;
    const int p0 = blockIdx.x * pix_per_block;
    const int p1 = min(p0 + pix_per_block, hw);
    float4 sc = *reinterpret_cast<const float4*>(a.scale + cl * 4);
    sc.x *= a.mult; sc.y *= a.mult; sc.z *= a.mult; sc.w *= a.mult;
    const float4 sh = *reinterpret_cast<const float4*>(a.shift + cl * 4);
    const float4 wf = *reinterpret_cast<const float4*>(a.wf + cl * 4);
    const float bf = a.bf[0];
    float rec = 0.f, dbf = 0.f;
    float dw[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    // UNR pixels per thread and pass, all loads issued before any use: the kernel is a pure stream (read c, write d_c) and one
    // 16-byte load in flight per lane saturates at ~3.7 TB/s on this chip
    constexpr int UNR = 4;
    auto one_pixel = [&](const size_t pix, const float4 c, const float xv) {
        float bn[4] = {fmaf(c.x, sc.x, sh.x), fmaf(c.y, sc.y, sh.y), fmaf(c.z, sc.z, sh.z), fmaf(c.w, sc.w, sh.w)};
        float av[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) av[e] = bn[e] > 0.f ? bn[e] : bn[e] * a.alpha;
        float dot = av[0] * wf.x;
        dot = fmaf(av[1], wf.y, dot);
        dot = fmaf(av[2], wf.z, dot);
        dot = fmaf(av[3], wf.w, dot);
        for (int o = 1; o < lpp; o <<= 1) dot += __shfl_xor(dot, o);
        const float xh = dot + bf;
        const float diff = xh - xv;
        if (cl == 0) {
            a.x_hat[pix] = xh;
            if (a.l1_map) a.l1_map[pix] = fabsf(diff);
            rec += fabsf(diff);
        }
        if (BWD) {
            const float s = a.dxhat_in ? a.dxhat_in[pix] : (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f)) * a.inv_batch;
            const float wv[4] = {wf.x, wf.y, wf.z, wf.w};
            const float cv[4] = {c.x, c.y, c.z, c.w};
            const float scv[4] = {sc.x, sc.y, sc.z, sc.w};
            float dc[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float da = s * wv[e];
                const float dbn = bn[e] > 0.f ? da : da * a.alpha;
                dc[e] = dbn * scv[e];
                dw[e] = fmaf(s, av[e], dw[e]);
                s1[e] += dbn;
                s2[e] = fmaf(dbn, cv[e], s2[e]);
            }
            *reinterpret_cast<float4*>(a.d_c + pix * a.C + cl * 4) = make_float4(dc[0], dc[1], dc[2], dc[3]);
            if (cl == 0) dbf += s;
        }
    };
    for (int p = p0 + slot; p < p1; p += ppp * UNR) {
        float4 cv[UNR];
        float xv[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int pp = min(p + u * ppp, p1 - 1);
            const size_t pix = (size_t)n * hw + pp;
            cv[u] = *reinterpret_cast<const float4*>(a.c_last + pix * a.C + cl * 4);
            xv[u] = a.x[pix];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            if (p + u * ppp < p1) one_pixel((size_t)n * hw + p + u * ppp, cv[u], xv[u]);
    }
    // reduce over the pixel slots: lanes with equal cl inside the wave, then across the 4 waves
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = lpp; o < 64; o <<= 1) {
        rec += __shfl_xor(rec, o);
        if (BWD) {
            dbf += __shfl_xor(dbf, o);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dw[e] += __shfl_xor(dw[e], o);
                s1[e] += __shfl_xor(s1[e], o);
                s2[e] += __shfl_xor(s2[e], o);
            }
        }
    }
    if (lane < lpp) {
        if (BWD) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                red[wave][0 * a.C + lane * 4 + e] = dw[e];
                red[wave][1 * a.C + lane * 4 + e] = s1[e];
                red[wave][2 * a.C + lane * 4 + e] = s2[e];
            }
        }
        if (lane == 0) {
            red[wave][3 * a.C] = dbf;
            red[wave][3 * a.C + 1] = rec;
        }
    }
    __syncthreads();
    const int blk = blockIdx.y * gridDim.x + blockIdx.x;
    const int nred = 3 * a.C + 2;
    if ((int)threadIdx.x < nred) {
        const float v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if ((int)threadIdx.x == 3 * a.C + 1) a.rec_partial[blk] = v;
        else if (BWD) a.red_partial[(size_t)blk * (3 * a.C + 1) + threadIdx.x] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// VAE bottleneck elementwise: dropout masks, sigma = exp(log_sigma), z = mu + eps*sigma, KL per sample.
// reference: models/variational_autoencoder.py:31-34 ; trainers/VAE.py:38 (KL with log(sigma^2) = 2 log_sigma)
// one wavefront per sample
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) reparam_fwd_kernel(int zdim, int n_vae, const float* __restrict__ mu_raw,
                                                         const float* __restrict__ ls_raw,
                                                         const float* __restrict__ mask_mu,
                                                         const float* __restrict__ mask_ls,
                                                         const float* __restrict__ mask_mu_ce,
                                                         const float* __restrict__ eps, float* __restrict__ mu,
                                                         float* __restrict__ ls, float* __restrict__ sigma,
                                                         float* __restrict__ z, float* __restrict__ kl) {
    const int n = blockIdx.x;
    // samples >= n_vae are the ceVAE context branch: z = z_mu_ce, no sampling, no KL
    // (context_encoder_variational_autoencoder.py:37,43); their log-sigma head is never used.
    const bool ctx = n >= n_vae;
    float acc = 0.f;
    for (int k = threadIdx.x; k < zdim; k += 64) {
        const size_t i = (size_t)n * zdim + k;
        float m = mu_raw[i];
        if (ctx) {
            if (mask_mu_ce) m *= mask_mu_ce[(size_t)(n - n_vae) * zdim + k];
            mu[i] = m; ls[i] = 0.f; sigma[i] = 1.f; z[i] = m;
            continue;
        }
        float l = ls_raw[i];
        if (mask_mu) m *= mask_mu[i];
        if (mask_ls) l *= mask_ls[i];
        const float s = expf(l);
        const float e = eps ? eps[i] : 0.f;
        mu[i] = m; ls[i] = l; sigma[i] = s;
        z[i] = fmaf(e, s, m);
        acc += m * m + s * s - 2.f * l - 1.f;
    }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) kl[n] = 0.5f * acc;
}

__global__ void reparam_bwd_kernel(size_t total, int zdim, int n_vae, const float* __restrict__ dz,
                                   const float* __restrict__ mu, const float* __restrict__ sigma,
                                   const float* __restrict__ eps, const float* __restrict__ mask_mu,
                                   const float* __restrict__ mask_ls, const float* __restrict__ mask_mu_ce,
                                   float inv_batch, float* __restrict__ dmu_raw, float* __restrict__ dls_raw) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t n = i / zdim;
    const float g = dz[i];
    if (n >= (size_t)n_vae) {
        dmu_raw[i] = mask_mu_ce ? g * mask_mu_ce[i - (size_t)n_vae * zdim] : g;
        dls_raw[i] = 0.f;
        return;
    }
    const float s = sigma[i];
    const float e = eps ? eps[i] : 0.f;
    float dm = g + mu[i] * inv_batch;
    float dl = g * e * s + (s * s - 1.f) * inv_batch;
    if (mask_mu) dm *= mask_mu[i];
    if (mask_ls) dl *= mask_ls[i];
    dmu_raw[i] = dm;
    dls_raw[i] = dl;
}

// rec_per_sample[i] = sum_b rec_partial[i][b].  Samples [0,n_vae) carry the VAE-branch losses, [n_vae,n) the ceVAE context
// branch (none for AE/VAE).  scalars = {reconstructionLoss, kl, loss, 0, Rec_vae, Rec_ce, loss_vae, 0}, all divided by the
// user batch (inv_batch); reconstructionLoss = rec_scale * (Rec_vae + Rec_ce)   (trainers/ceVAE.py:45-50)
__global__ void __launch_bounds__(256) loss_finalize_kernel(const float* __restrict__ rec_partial, int n, int n_vae,
                                                            int bps, const float* __restrict__ kl, float inv_batch,
                                                            float rec_scale, float* __restrict__ rec_per_sample,
                                                            float* __restrict__ scalars) {
    __shared__ float sr[256], sc[256], sk[256];
    float ar = 0.f, ac = 0.f, ak = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        float r = 0.f;
        for (int b = 0; b < bps; ++b) r += rec_partial[(size_t)i * bps + b];
        rec_per_sample[i] = r;
        if (i < n_vae) { ar += r; if (kl) ak += kl[i]; }
        else ac += r;
    }
    sr[threadIdx.x] = ar;
    sc[threadIdx.x] = ac;
    sk[threadIdx.x] = ak;
    __syncthreads();
    if (threadIdx.x == 0) {
        float tr = 0.f, tc = 0.f, tk = 0.f;
        for (int i = 0; i < 256; ++i) { tr += sr[i]; tc += sc[i]; tk += sk[i]; }
        scalars[0] = rec_scale * (tr + tc) * inv_batch;
        scalars[1] = tk * inv_batch;
        scalars[2] = (tr + tk + tc) * inv_batch;
        scalars[3] = 0.f;
        scalars[4] = tr * inv_batch;
        scalars[5] = tc * inv_batch;
        scalars[6] = (tr + tk) * inv_batch;
        scalars[7] = 0.f;
    }
}

// Spatial autoencoder latent (models/autoencoder_spatial.py:13-17): z = mask * lrelu(gamma' c + beta) of the last encoder block,
// materialised because it is a graph output and the decoder input; backward: d c = d z * mask * lrelu' * gamma', with the
// per-block column sums the BN-gradient finalize expects (colpart[blk][0][ch] = sum d_bn, [1][ch] = sum d_bn * c).
__global__ void __launch_bounds__(256) spatial_z_fwd_kernel(const float* __restrict__ c, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float rs0, float alpha,
                                                            const float* __restrict__ mask, size_t total4, int C, float* __restrict__ z) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int ch = (int)((i * 4) % C);
    const float4 g = *reinterpret_cast<const float4*>(gamma + ch), b = *reinterpret_cast<const float4*>(beta + ch);
    const float4 v = reinterpret_cast<const float4*>(c)[i];
    float4 y = make_float4(fmaf(v.x, g.x * rs0, b.x), fmaf(v.y, g.y * rs0, b.y), fmaf(v.z, g.z * rs0, b.z), fmaf(v.w, g.w * rs0, b.w));
    y = make_float4(y.x > 0.f ? y.x : alpha * y.x, y.y > 0.f ? y.y : alpha * y.y, y.z > 0.f ? y.z : alpha * y.z, y.w > 0.f ? y.w : alpha * y.w);
    if (mask) { const float4 m = reinterpret_cast<const float4*>(mask)[i]; y = make_float4(y.x * m.x, y.y * m.y, y.z * m.z, y.w * m.w); }
    reinterpret_cast<float4*>(z)[i] = y;
}
__global__ void __launch_bounds__(256) spatial_z_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ c,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float rs0,
                                                            float alpha, const float* __restrict__ mask, int rows, int rows_per_block,
                                                            int C, float* __restrict__ dc, float* __restrict__ colpart) {
    __shared__ float r1[1024], r2[1024];
    const int Q = C / 4, RL = 256 / Q;
    const int cq = threadIdx.x % Q, rl = threadIdx.x / Q, ch = cq * 4;
    const float4 g0 = *reinterpret_cast<const float4*>(gamma + ch), b = *reinterpret_cast<const float4*>(beta + ch);
    const float4 g = make_float4(g0.x * rs0, g0.y * rs0, g0.z * rs0, g0.w * rs0);
    const int row0 = blockIdx.x * rows_per_block, row1 = min(rows, row0 + rows_per_block);
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    for (int row = row0 + rl; row < row1; row += RL) {
        const size_t o = (size_t)row * C + ch;
        const float4 cv = *reinterpret_cast<const float4*>(c + o);
        float4 d = *reinterpret_cast<const float4*>(dz + o);
        if (mask) { const float4 m = *reinterpret_cast<const float4*>(mask + o); d = make_float4(d.x * m.x, d.y * m.y, d.z * m.z, d.w * m.w); }
        const float4 dn = make_float4(fmaf(cv.x, g.x, b.x) > 0.f ? d.x : alpha * d.x, fmaf(cv.y, g.y, b.y) > 0.f ? d.y : alpha * d.y,
                                      fmaf(cv.z, g.z, b.z) > 0.f ? d.z : alpha * d.z, fmaf(cv.w, g.w, b.w) > 0.f ? d.w : alpha * d.w);
        *reinterpret_cast<float4*>(dc + o) = make_float4(dn.x * g.x, dn.y * g.y, dn.z * g.z, dn.w * g.w);
        s1 = make_float4(s1.x + dn.x, s1.y + dn.y, s1.z + dn.z, s1.w + dn.w);
        s2 = make_float4(fmaf(dn.x, cv.x, s2.x), fmaf(dn.y, cv.y, s2.y), fmaf(dn.z, cv.z, s2.z), fmaf(dn.w, cv.w, s2.w));
    }
    *reinterpret_cast<float4*>(r1 + rl * C + ch) = s1;
    *reinterpret_cast<float4*>(r2 + rl * C + ch) = s2;
    __syncthreads();
    for (int k = threadIdx.x; k < C; k += 256) {
        float a1 = 0.f, a2 = 0.f;
        for (int j = 0; j < RL; ++j) { a1 += r1[j * C + k]; a2 += r2[j * C + k]; }
        colpart[((size_t)blockIdx.x * 2 + 0) * C + k] = a1;
        colpart[((size_t)blockIdx.x * 2 + 1) * C + k] = a2;
    }
}

}  // namespace

int uad_final_blocks_per_sample(int H, int W) {
    const int hw = H * W;
    int bps = hw / 512;
    return bps < 1 ? 1 : bps;
}
void uad_launch_final_fwd_bwd(const UadFinalArgs& a, hipStream_t st) {
    const int bps = uad_final_blocks_per_sample(a.H, a.W);
    const int ppb = (a.H * a.W + bps - 1) / bps;
    dim3 grid(bps, a.N);
    if (a.d_c)
        hipLaunchKernelGGL((final_kernel<true>), grid, dim3(256), 0, st, a, ppb);
    else
        hipLaunchKernelGGL((final_kernel<false>), grid, dim3(256), 0, st, a, ppb);
}

void uad_launch_reparam_fwd(int n, int n_vae, int zdim, const float* mu_raw, const float* ls_raw, const float* mask_mu,
                            const float* mask_ls, const float* mask_mu_ce, const float* eps, float* mu, float* ls,
                            float* sigma, float* z, float* kl_per_sample, hipStream_t st) {
    hipLaunchKernelGGL(reparam_fwd_kernel, dim3(n), dim3(64), 0, st, zdim, n_vae, mu_raw, ls_raw, mask_mu, mask_ls,
                       mask_mu_ce, eps, mu, ls, sigma, z, kl_per_sample);
}
void uad_launch_reparam_bwd(int n, int n_vae, int zdim, const float* dz, const float* mu, const float* sigma,
                            const float* eps, const float* mask_mu, const float* mask_ls, const float* mask_mu_ce,
                            float inv_batch, float* dmu_raw, float* dls_raw, hipStream_t st) {
    const size_t total = (size_t)n * zdim;
    hipLaunchKernelGGL(reparam_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0, st, total, zdim, n_vae, dz, mu,
                       sigma, eps, mask_mu, mask_ls, mask_mu_ce, inv_batch, dmu_raw, dls_raw);
}
void uad_launch_loss_finalize(const float* rec_partial, int n, int n_vae, int bps, const float* kl_per_sample,
                              float inv_batch, float rec_scale, float* rec_per_sample, float* scalars, hipStream_t st) {
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, st, rec_partial, n, n_vae, bps, kl_per_sample,
                       inv_batch, rec_scale, rec_per_sample, scalars);
}
void uad_launch_spatial_z_fwd(const float* c, const float* gamma, const float* beta, float rs0, float alpha, const float* mask, int rows,
                              int C, float* z, hipStream_t st) {
    const size_t total4 = (size_t)rows * C / 4;
    hipLaunchKernelGGL(spatial_z_fwd_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, c, gamma, beta, rs0, alpha, mask, total4, C, z);
}
int uad_spatial_z_bwd_blocks(int rows) {      // blocks the backward launches (= colpart rows it writes)
    const int nb = rows < 512 ? rows : 512;
    const int rpb = (rows + nb - 1) / nb;
    return (rows + rpb - 1) / rpb;
}
void uad_launch_spatial_z_bwd(const float* dz, const float* c, const float* gamma, const float* beta, float rs0, float alpha,
                              const float* mask, int rows, int C, float* dc, float* colpart, hipStream_t st) {
    const int nb = uad_spatial_z_bwd_blocks(rows);
    const int rpb = (rows + nb - 1) / nb;
    hipLaunchKernelGGL(spatial_z_bwd_kernel, dim3(nb), dim3(256), 0, st, dz, c, gamma, beta, rs0, alpha, mask, rows, rpb, C, dc, colpart);
}
