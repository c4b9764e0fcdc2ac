// tgs_adam.h -- the Adam update (adam1) shared by K9 (optim.hip) and the optimizer kernels of project.hip, and the two
// traversals those four kernels share: adam_sh_stream (SH rows through an LDS image) and adam_geom (the other 11);
// the LDS SH image itself (ShImage: geometry, coalesced load and store, sh_image_bytes) and the flat layout's segments.
#pragma once
#include <math.h>
#include <stddef.h>
#include "tgs_common.h"

struct AdamK {
  long long e_means, e_scales, e_quats, e_opac, e_total;  // start of the NEXT segment (elements)
  long long e_begin, e_end;                               // element range updated by this launch
  unsigned sh_row;                                        // 3*K floats per Gaussian in the SH block
  unsigned row_step;                                      // (4 * grid stride) mod sh_row
  float lr_means, lr_scales, lr_quats, lr_opac, lr_dc, lr_rest;
  float b1, b2, eps, ibc1, isq_bc2, gscale;
  const float* dyn;   // device {bias_corr1, bias_corr2, lr_means} of the current step, or NULL
  const int32_t* guard;  // status word of the frame's binning ({n, overflow}), or NULL: overflow => no-op
};

static inline long long tgs_al4(long long x) { return (x + 3) & ~3ll; }

// Flat layout: means[3N] | log_scales[3N] | quats[4N] | opac_logit[N] | sh[N*K*3], every segment
// starting at a multiple of 4 floats (include/tgs.h, TgsAdamSpec).
static inline AdamK make_adamk(int N, int sh_stride, const TgsAdamSpec* spec, float grad_scale) {
  AdamK a;
  a.e_means = tgs_al4(3ll * N);
  a.e_scales = tgs_al4(a.e_means + 3ll * N);
  a.e_quats = a.e_scales + 4ll * N;
  a.e_opac = tgs_al4(a.e_quats + N);
  a.sh_row = sh_stride > 0 ? 3u * (unsigned)sh_stride : 4u;
  a.e_total = tgs_al4(a.e_opac + (long long)N * sh_stride * 3);
  a.e_begin = 0; a.e_end = a.e_total; a.row_step = 0;
  a.lr_means = spec->lr_means; a.lr_scales = spec->lr_scales; a.lr_quats = spec->lr_quats;
  a.lr_opac = spec->lr_opac; a.lr_dc = spec->lr_sh_dc; a.lr_rest = spec->lr_sh_rest;
  a.b1 = spec->beta1; a.b2 = spec->beta2; a.eps = spec->eps;
  a.ibc1 = 1.0f / spec->bias_corr1;
  a.isq_bc2 = 1.0f / sqrtf(spec->bias_corr2);
  a.gscale = grad_scale;
  a.dyn = spec->device_bias_corr;
  a.guard = nullptr;
  return a;
}

// The five segments of a flat parameter buffer (the moments and the all-reduced gradients have the same layout).
struct ParamSegs { float *means, *log_scales, *quats, *opac, *sh; };
static inline ParamSegs param_segs(float* params, const AdamK& a) {
  return {params, params + a.e_means, params + a.e_scales, params + a.e_quats, params + a.e_opac};
}

// Dynamic LDS of a kernel that stages the SH rows of its 256 Gaussians (ShImage below): [256][3 * sh_stride + 4] floats.
constexpr size_t sh_image_bytes(int sh_stride) { return 256 * (size_t)(3 * sh_stride + 4) * sizeof(float); }

#ifdef __HIPCC__
// The LDS SH image of a workgroup: the SH rows (ROW = 3 * bases floats = F4 float4s each) of the nrows <= 256
// consecutive Gaussians from g0 on, which are one contiguous block of `sh` starting at element blk, held as
// lds[row * RS + column]; the pad RS = ROW + 4 makes a thread's ds_read_b128 of its own row conflict-free.
// KS > 0: the number of stored bases is a compile-time constant of the kernel; KS = 0: it is sh_stride.
template <int KS>
struct ShImage {
  static constexpr int ROW = 3 * KS, RS = ROW + 4, F4 = ROW / 4;
  int g0, nrows;
  size_t blk;
};
template <>
struct ShImage<0> {
  int ROW, RS, F4;
  int g0, nrows;
  size_t blk;
};
template <int KS>
__device__ __forceinline__ ShImage<KS> sh_image(int sh_stride, int g0, int N) {
  ShImage<KS> im;
  if constexpr (KS == 0) { im.ROW = 3 * sh_stride; im.RS = im.ROW + 4; im.F4 = im.ROW / 4; }
  im.g0 = g0;
  im.nrows = min(256, N - g0);
  im.blk = (size_t)g0 * im.ROW;
  return im;
}

// sh -> image, fully coalesced, 4 float4 columns per thread and round.  CACHED: the rows are read again (by the Adam
// stream), keep them cached; otherwise this is the only read of the step.
template <bool CACHED, int KS>
__device__ __forceinline__ void sh_image_load(const ShImage<KS>& im, const float* sh, float* lds, int tid) {
  const int nf = im.nrows * im.F4;
  for (int f0 = tid; f0 < nf; f0 += 256 * 4) {
    float4 t[4];
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (f0 + 256 * u < nf) {
        const float* src = sh + im.blk + 4 * (size_t)(f0 + 256 * u);
        t[u] = CACHED ? ld4(src) : ld4_nt(src);
      }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int f = f0 + 256 * u;
      if (f < nf) { const int row = f / im.F4, c4 = f - row * im.F4; st4(lds + row * im.RS + 4 * c4, t[u]); }
    }
  }
}

// image -> the block's rows of `out` (the SH gradient), fully coalesced
template <int KS>
__device__ __forceinline__ void sh_image_store(const ShImage<KS>& im, const float* lds, float* out, int tid) {
  const int nf = im.nrows * im.F4;
  for (int f0 = tid; f0 < nf; f0 += 256 * 2) {
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int f = f0 + 256 * u;
      if (f < nf) { const int row = f / im.F4, c4 = f - row * im.F4; st4(out + im.blk + 4 * (size_t)f, ld4(lds + row * im.RS + 4 * c4)); }
    }
  }
}

// Bias corrections and the scheduled position learning rate kept in device memory (a captured hipGraph of the step is replayed with the
// current step's values): same IEEE division / square root as make_adamk does on the host.
__device__ __forceinline__ AdamK adam_resolve(AdamK a) {
  if (a.dyn) {
    a.ibc1 = 1.0f / a.dyn[0];
    a.isq_bc2 = 1.0f / sqrtf(a.dyn[1]);
    a.lr_means = a.dyn[2];   // the scheduled (exponentially decayed) position learning rate
  }
  return a;
}

// One Adam update.  Every multiply-add is an explicit fmaf: the same update is evaluated by several
// kernels (k_adam, the fused K8+Adam kernel, the gathered-SH kernel of the data-parallel step) that are
// tested to agree bit for bit, so no FMA formation is left to the compiler's per-kernel choice.
__device__ __forceinline__ void adam1(const AdamK& a, float lr, float& p, float g, float& m, float& v) {
  g *= a.gscale;
  m = fmaf(a.b1, m, (1.f - a.b1) * g);
  v = fmaf(a.b2, v, ((1.f - a.b2) * g) * g);
  const float denom = fmaf(sqrtf(v), a.isq_bc2, a.eps);
  p -= (lr * (m * a.ibc1)) / denom;
}

// Adam on the SH rows of a workgroup's image, whose gradients sit in it: the block of sh and of both moments is streamed
// fully coalesced, 2 float4 columns per thread and round so that 6 independent loads are in flight.
// keep: the updated coefficients replace the consumed gradient in the image (for a colour evaluation that follows).
// The ONE body of the fused K8+Adam kernel, k_adam_sh_gathered and k_adam_sh_geom_next (project.hip).
template <int KS>
__device__ __forceinline__ void adam_sh_stream(const AdamK& ad, float* sh, float* exp_avg, float* exp_avg_sq, float* lds,
                                               const ShImage<KS>& im, int tid, bool keep) {
  const int nf = im.nrows * im.F4;
  for (int f0 = tid; f0 < nf; f0 += 256 * 2) {
    float4 P[2], M[2], V[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int f = f0 + 256 * u;
      if (f < nf) {
        const size_t e = im.blk + 4 * (size_t)f;
        P[u] = ld4_nt(sh + e); M[u] = ld4_nt(exp_avg + ad.e_opac + e); V[u] = ld4_nt(exp_avg_sq + ad.e_opac + e);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int f = f0 + 256 * u;
      if (f < nf) {
        const int row = f / im.F4, c4 = f - row * im.F4;
        const float4 G = ld4(lds + row * im.RS + 4 * c4);
        const size_t e = im.blk + 4 * (size_t)f;
        const int c = 4 * c4;  // column of the first element inside the 3K-float row; DC = columns 0..2
        adam1(ad, c < 3 ? ad.lr_dc : ad.lr_rest, P[u].x, G.x, M[u].x, V[u].x);
        adam1(ad, c + 1 < 3 ? ad.lr_dc : ad.lr_rest, P[u].y, G.y, M[u].y, V[u].y);
        adam1(ad, c + 2 < 3 ? ad.lr_dc : ad.lr_rest, P[u].z, G.z, M[u].z, V[u].z);
        adam1(ad, ad.lr_rest, P[u].w, G.w, M[u].w, V[u].w);
        st4_nt(sh + e, P[u]); st4_nt(exp_avg + ad.e_opac + e, M[u]); st4_nt(exp_avg_sq + ad.e_opac + e, V[u]);
        if (keep) st4(lds + row * im.RS + 4 * c4, P[u]);
      }
    }
  }
}

// Adam on the 11 non-SH parameters of Gaussian g by its owner thread.  Parameters (m, ls, q, ol) and gradients
// (gm, gls, gq, go) come in registers; the moments are read and written here (flat-buffer offsets from the layout),
// the parameters are stored and their updated values stay in m / ls / q / ol for the caller's colour evaluation and K1.
// NT_Q: cache hint of the quaternion store (the callers differ; measured per kernel, not unified here).
template <bool NT_Q>
__device__ __forceinline__ void adam_geom(const AdamK& ad, int g, float* m, float* ls, float* q, float& ol,
                                          const float* gm, const float* gls, const float* gq, float go,
                                          float* means, float* log_scales, float* quats, float* opac_logit,
                                          float* exp_avg, float* exp_avg_sq) {
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const long long e = 3ll * g + j;
    float M = exp_avg[e], V = exp_avg_sq[e];
    adam1(ad, ad.lr_means, m[j], gm[j], M, V);
    means[3 * g + j] = m[j]; exp_avg[e] = M; exp_avg_sq[e] = V;
  }
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const long long e = ad.e_means + 3ll * g + j;
    float M = exp_avg[e], V = exp_avg_sq[e];
    adam1(ad, ad.lr_scales, ls[j], gls[j], M, V);
    log_scales[3 * g + j] = ls[j]; exp_avg[e] = M; exp_avg_sq[e] = V;
  }
  {
    const long long e = ad.e_scales + 4ll * g;
    float4 M = ld4_nt(exp_avg + e), V = ld4_nt(exp_avg_sq + e);
    adam1(ad, ad.lr_quats, q[0], gq[0], M.x, V.x); adam1(ad, ad.lr_quats, q[1], gq[1], M.y, V.y);
    adam1(ad, ad.lr_quats, q[2], gq[2], M.z, V.z); adam1(ad, ad.lr_quats, q[3], gq[3], M.w, V.w);
    const float4 Q = make_float4(q[0], q[1], q[2], q[3]);
    if constexpr (NT_Q) st4_nt(quats + 4 * (size_t)g, Q); else st4(quats + 4 * (size_t)g, Q);
    st4_nt(exp_avg + e, M); st4_nt(exp_avg_sq + e, V);
  }
  {
    const long long e = ad.e_quats + g;
    float M = exp_avg[e], V = exp_avg_sq[e];
    adam1(ad, ad.lr_opac, ol, go, M, V);
    opac_logit[g] = ol; exp_avg[e] = M; exp_avg_sq[e] = V;
  }
}

// The same with the gradients read from the flat (all-reduced) gradient buffer, which has the parameters' layout.
__device__ __forceinline__ void adam_geom_flat(const AdamK& ad, int g, float* m, float* ls, float* q, float& ol,
                                               const float* grads, float* means, float* log_scales, float* quats,
                                               float* opac_logit, float* exp_avg, float* exp_avg_sq) {
  const float gm[3] = {grads[3ll * g], grads[3ll * g + 1], grads[3ll * g + 2]};
  const float gls[3] = {grads[ad.e_means + 3ll * g], grads[ad.e_means + 3ll * g + 1], grads[ad.e_means + 3ll * g + 2]};
  const float4 G = ld4_nt(grads + ad.e_scales + 4ll * g);
  const float gq[4] = {G.x, G.y, G.z, G.w};
  adam_geom<false>(ad, g, m, ls, q, ol, gm, gls, gq, grads[ad.e_quats + g], means, log_scales, quats, opac_logit,
                   exp_avg, exp_avg_sq);
}
#endif
