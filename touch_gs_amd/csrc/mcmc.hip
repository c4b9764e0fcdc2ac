// mcmc.hip -- the per-step and the per-refinement kernel of the fixed-budget MCMC strategy (3DGS-MCMC, Kheradmand et
// al. 2024; touch_gs_amd/mcmc.py).  gfx950.
//
// k_mcmc_adam_geom: L1 regularisers on opacity and scale + Adam on the 11 geometry values of a Gaussian (the shared body
// adam_geom of tgs_adam.h, fed from registers) + the opacity-gated, covariance-shaped noise on the means, one thread per
// Gaussian, one launch.  Roofline: HBM; per Gaussian 11 x 28 B of Adam traffic + 12 B of noise + 12 B for the second
// store of the means (which hits the line the first one left in L2).
// k_mcmc_relocate: gsplat's compute_relocation in fp64, one thread per row, a few percent of the rows once per refinement.
//
// Built with -ffp-contract=off (build.sh): every product and sum of the regulariser and the noise term rounds on its own,
// as the fp32 NumPy emulation of tests/mcmc_ref.py evaluates them; adam1's multiply-adds are explicit fmaf either way.
#include "tgs_adam.h"

namespace {

struct McmcK {
  float c_opac;     // opacity_reg / N
  float c_scale;    // scale_reg / (3 N)
  float noise_lr, gate_k, gate_o0;
};

__global__ __launch_bounds__(256) void k_mcmc_adam_geom(AdamK a_in, McmcK mk, int N, float* __restrict__ params,
                                                        const float* __restrict__ grads, float* __restrict__ exp_avg,
                                                        float* __restrict__ exp_avg_sq, const float* __restrict__ noise) {
  if (a_in.guard && a_in.guard[1]) return;   // the frame overflowed its intersection buffers: no update
  const AdamK ad = adam_resolve(a_in);
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= N) return;
  const ParamSegs P = {params, params + ad.e_means, params + ad.e_scales, params + ad.e_quats, params + ad.e_opac};
  float m[3] = {P.means[3ll * g], P.means[3ll * g + 1], P.means[3ll * g + 2]};
  float ls[3] = {P.log_scales[3ll * g], P.log_scales[3ll * g + 1], P.log_scales[3ll * g + 2]};
  const float4 Q = ld4(P.quats + 4 * (size_t)g);
  float q[4] = {Q.x, Q.y, Q.z, Q.w};
  float ol = P.opac[g];
  // the gradients as adam_geom_flat reads them, plus d/d(ol, ls) of  lambda_o mean(sigmoid(ol)) + lambda_s mean(exp(ls))
  const float gm[3] = {grads[3ll * g], grads[3ll * g + 1], grads[3ll * g + 2]};
  float gls[3] = {grads[ad.e_means + 3ll * g], grads[ad.e_means + 3ll * g + 1], grads[ad.e_means + 3ll * g + 2]};
  const float4 G = ld4_nt(grads + ad.e_scales + 4ll * g);
  const float gq[4] = {G.x, G.y, G.z, G.w};
  float go = grads[ad.e_quats + g];
  if (mk.c_opac != 0.f) {     // (a zero weight adds nothing, not even +0 to a -0 gradient: the identity with k_adam is in bits)
    const float e = expf(-fabsf(ol)), d = 1.f + e;      // o (1 - o) = e / (1 + e)^2 without cancellation at either end
    go += mk.c_opac * (e / (d * d));
  }
  if (mk.c_scale != 0.f) {
#pragma unroll
    for (int j = 0; j < 3; j++) gls[j] += mk.c_scale * expf(ls[j]);
  }
  adam_geom<false>(ad, g, m, ls, q, ol, gm, gls, gq, go, P.means, P.log_scales, P.quats, P.opac, exp_avg, exp_avg_sq);
  if (noise == nullptr) return;
  // means += (noise_lr lr_means gate) R diag(s'^2) R^T n   from the UPDATED values in registers
  const float o = 1.f / (1.f + expf(-ol));
  const float t = mk.gate_k * (o - mk.gate_o0);
  const float gate = t > 80.f ? 0.f : 1.f / (1.f + expf(t));
  const float c = (mk.noise_lr * ad.lr_means) * gate;
  const float inv = 1.f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const float w = q[0] * inv, x = q[1] * inv, y = q[2] * inv, z = q[3] * inv;
  const float R[9] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - w * z), 2.f * (x * z + w * y),
                      2.f * (x * y + w * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - w * x),
                      2.f * (x * z - w * y), 2.f * (y * z + w * x), 1.f - 2.f * (x * x + y * y)};
  const float n[3] = {noise[3ll * g], noise[3ll * g + 1], noise[3ll * g + 2]};
  float v[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float s = expf(ls[k]);
    v[k] = (s * s) * ((R[k] * n[0] + R[3 + k] * n[1]) + R[6 + k] * n[2]);
  }
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float dlt = (R[3 * j] * v[0] + R[3 * j + 1] * v[1]) + R[3 * j + 2] * v[2];
    if (c != 0.f) P.means[3ll * g + j] = m[j] + c * dlt;     // (a closed gate or noise_lr 0 moves nothing: no second store)
  }
}

// S = sum_{k=0}^{r-1} C(r, k+1) (-1)^k x^(k+1) / sqrt(k+1): the double sum of gsplat's compute_relocation collapsed by the
// hockey-stick identity sum_{i=k+1}^{r} C(i-1, k) = C(r, k+1).
__global__ __launch_bounds__(256) void k_mcmc_relocate(int n, const int32_t* __restrict__ ratio, float* __restrict__ opac_logit,
                                                       float* __restrict__ log_scales, double min_opacity) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int r = ratio[i];
  if (r <= 1) return;
  r = min(r, 51);
  const double l = (double)opac_logit[i];
  const double log_1mo = -(l > 0 ? l + log1p(exp(-l)) : log1p(exp(l)));    // log(1 - o), o = sigmoid(l)
  const double o = 1.0 / (1.0 + exp(-l));
  const double x = -expm1(log_1mo / (double)r);                            // 1 - (1 - o)^(1/r)
  double S = 0.0, binom = (double)r, xp = x;
  for (int k = 0; k < r; k++) {
    const double term = binom * xp / sqrt((double)(k + 1));
    S += (k & 1) ? -term : term;
    binom = binom * (double)(r - k - 1) / (double)(k + 2);
    xp *= x;
  }
  const double xc = fmin(fmax(x, min_opacity), 1.0 - 0x1p-23);
  opac_logit[i] = (float)(log(xc) - log1p(-xc));
  const double dls = log(o / S);
#pragma unroll
  for (int j = 0; j < 3; j++) log_scales[3ll * i + j] = (float)((double)log_scales[3ll * i + j] + dls);
}

}  // namespace

extern "C" int tgs_mcmc_adam_geom(int N, int sh_stride, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                  const TgsAdamSpec* spec, float grad_scale, const TgsMcmcSpec* mcmc, const float* noise,
                                  const int32_t* skip_if_overflow, void* stream) {
  TGS_CHECK_ARG(N >= 0 && sh_stride >= 0, "negative size");
  TGS_CHECK_ARG(spec && mcmc, "null spec");
  TGS_CHECK_ARG(mcmc->opacity_reg >= 0.f && mcmc->scale_reg >= 0.f && mcmc->noise_lr >= 0.f && mcmc->gate_k >= 0.f,
                "opacity_reg, scale_reg, noise_lr and gate_k must be >= 0 (and not NaN)");
  TGS_CHECK_ARG(N <= (INT_MAX - 255) / 4, "too many Gaussians for the kernel's 32-bit row index");
  if (N == 0) return TGS_OK;
  TGS_CHECK_ARG(params && grads && exp_avg && exp_avg_sq, "null pointer");
  TGS_CHECK_ARG(((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0,
                "buffers must be 16-byte aligned");
  TGS_CHECK_ARG(noise == nullptr || (uintptr_t)noise % 4 == 0, "noise must be 4-byte aligned");
  AdamK a = make_adamk(N, sh_stride, spec, grad_scale);
  a.guard = skip_if_overflow;
  McmcK mk;
  mk.c_opac = mcmc->opacity_reg / (float)N;
  mk.c_scale = mcmc->scale_reg / (3.f * (float)N);
  mk.noise_lr = mcmc->noise_lr; mk.gate_k = mcmc->gate_k; mk.gate_o0 = mcmc->gate_o0;
  hipLaunchKernelGGL(k_mcmc_adam_geom, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, mk, N,
                     params, grads, exp_avg, exp_avg_sq, noise);
  TGS_CHECK_LAUNCH();
  return TGS_OK;
}

extern "C" int tgs_mcmc_relocate(int n, const int32_t* ratio, float* opac_logit, float* log_scales, float min_opacity,
                                 void* stream) {
  TGS_CHECK_ARG(n >= 0, "negative size");
  TGS_CHECK_ARG(min_opacity > 0.f && min_opacity < 1.f, "min_opacity must lie in (0, 1)");
  TGS_CHECK_ARG(n <= (INT_MAX - 255) / 4, "too many rows for the kernel's 32-bit row index");
  if (n == 0) return TGS_OK;
  TGS_CHECK_ARG(ratio, "ratio is null");
  TGS_CHECK_ARG(opac_logit && log_scales, "null pointer");
  hipLaunchKernelGGL(k_mcmc_relocate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, ratio,
                     opac_logit, log_scales, (double)min_opacity);
  TGS_CHECK_LAUNCH();
  return TGS_OK;
}
