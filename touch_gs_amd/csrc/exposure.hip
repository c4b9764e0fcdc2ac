// exposure.hip -- per-view exposure compensation C' = A C + b (E = [A | b], row-major 3x4) as an image-space op beside
// K6 / K7 (include/tgs.h, tgs_exposure_fwd / tgs_exposure_bwd).  The RGB loss is taken on C'; what goes to K7
// is v_rgb = A^T v', K7's own fused L1 term is switched off (TgsLossSpec.gt_rgb NULL).  gfx950.
//
// Three launches:
//   k_expo_fwd       : a pure stream, 12 floats = 4 pixels per thread and round (3 x 16 B in, 3 x 16 B out), scalar where
//                      the 4 pixels pass the end of the image or a pointer is not 16-byte aligned.  24 B per pixel.
//   k_expo_bwd_tiles : EXPO_CHUNK pixels per workgroup.  Reads rgb, gt, v_img (36 B per pixel), RECOMPUTES C' through
//                      expo_apply -- the function the forward calls; re-reading C' would be 48 B in -- forms
//                      v' = v_img + l1_weight sign(C' - gt) (K7's expression, sign(0) = 0), writes v_rgb (12 B) and sums
//                      G_A, G_b, their masses, sum |C' - gt| and the pixel count: per thread in pixel order, across the
//                      wave by DPP, across the four waves through LDS in wave order.  One 32-float row per workgroup.
//   k_expo_fold      : ONE workgroup sums the rows in fp64 in an order fixed by the thread count alone, writes out[32],
//                      and -- state given, frame valid -- adds the L2 pull and steps the 12 entries with adam1.
// No float atomics anywhere: the same inputs give the same bits.
//
// This translation unit is built with -ffp-contract=on (build.sh), and expo_apply spells its FMAs out besides: the forward
// and the backward must form the same bits of C', so that sign() decides on the image SSIM saw.
#include <math.h>
#include "tgs_adam.h"
#include "tgs_common.h"

namespace {

constexpr int EXPO_THREADS = 256;
constexpr int EXPO_ROUNDS = 2;                               // 4-pixel groups per thread
constexpr int EXPO_CHUNK = EXPO_THREADS * 4 * EXPO_ROUNDS;   // pixels per workgroup (touch_gs_amd/_lib.py EXPO_CHUNK)
constexpr int EXPO_WAVES = EXPO_THREADS / TGS_WAVE;
constexpr int EXPO_SUMS = 26;                                // G[12] | mass[12] | sum |C' - gt| | pixels
constexpr int FOLD_THREADS = 256;
constexpr int FOLD_LANES = FOLD_THREADS / TGS_EXPO_OUT;      // row groups of the fold

struct ExpoK { float e[12]; };

__device__ __forceinline__ ExpoK expo_load(const float* __restrict__ expo) {
  ExpoK k;
#pragma unroll
  for (int j = 0; j < 12; j++) k.e[j] = expo[j];
  return k;
}

// C'_c = A[c][0] r + A[c][1] g + A[c][2] b + b[c]: THE expression of the compensated colour, shared by both kernels.
__device__ __forceinline__ float expo_apply(const ExpoK& k, int c, float r, float g, float b) {
  return fmaf(k.e[4 * c + 2], b, fmaf(k.e[4 * c + 1], g, fmaf(k.e[4 * c], r, k.e[4 * c + 3])));
}

template <bool VEC>
__global__ __launch_bounds__(EXPO_THREADS) void k_expo_fwd(size_t npix, const float* __restrict__ rgb,
                                                           const float* __restrict__ expo, float* __restrict__ rgb_out) {
  const ExpoK k = expo_load(expo);
#pragma unroll
  for (int r = 0; r < EXPO_ROUNDS; r++) {
    const size_t p = (size_t)blockIdx.x * EXPO_CHUNK + (size_t)(r * EXPO_THREADS + threadIdx.x) * 4;
    if (p >= npix) continue;
    if (VEC && p + 4 <= npix) {
      // plain loads: rgb is read again by the backward and by K7 (ld4_nt is for data touched once, tgs_common.h)
      const float4 a = ld4(rgb + 3 * p), b = ld4(rgb + 3 * p + 4), c = ld4(rgb + 3 * p + 8);
      const float in[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
      float o[12];
#pragma unroll
      for (int q = 0; q < 4; q++)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) o[3 * q + ch] = expo_apply(k, ch, in[3 * q], in[3 * q + 1], in[3 * q + 2]);
      st4(rgb_out + 3 * p, make_float4(o[0], o[1], o[2], o[3]));   // (kept cached: SSIM and the backward read it next)
      st4(rgb_out + 3 * p + 4, make_float4(o[4], o[5], o[6], o[7]));
      st4(rgb_out + 3 * p + 8, make_float4(o[8], o[9], o[10], o[11]));
      continue;
    }
    const size_t e = p + 4 < npix ? p + 4 : npix;
    for (size_t i = p; i < e; i++) {
      const float cr = rgb[3 * i], cg = rgb[3 * i + 1], cb = rgb[3 * i + 2];
#pragma unroll
      for (int ch = 0; ch < 3; ch++) rgb_out[3 * i + ch] = expo_apply(k, ch, cr, cg, cb);
    }
  }
}

// One pixel of the backward: C = (cr, cg, cb), gt / vi = its 3 entries of gt / v_img (unused where the image is absent).
// Adds the pixel's products to s[] in a fixed order and returns v_rgb of the pixel in o[3].
template <bool HAS_GT, bool HAS_V>
__device__ __forceinline__ void expo_pixel(const ExpoK& k, float l1w, float cr, float cg, float cb, const float* gt,
                                           const float* vi, float* o, float* s) {
  const float C[3] = {cr, cg, cb};
  float vp[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float v = HAS_V ? vi[c] : 0.f;
    if (HAS_GT) {
      const float d = expo_apply(k, c, cr, cg, cb) - gt[c];
      v += l1w * ((d > 0.f) - (d < 0.f));   // raster.hip pixel_upstream's expression: the product is exact
      s[24] += fabsf(d);
    }
    vp[c] = v;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const float t = v * C[j];
      s[4 * c + j] += t;
      s[12 + 4 * c + j] += fabsf(t);
    }
    s[4 * c + 3] += v;
    s[12 + 4 * c + 3] += fabsf(v);
  }
  s[25] += 1.f;
#pragma unroll
  for (int j = 0; j < 3; j++) o[j] = fmaf(k.e[8 + j], vp[2], fmaf(k.e[4 + j], vp[1], k.e[j] * vp[0]));
}

// NT: the image is read by this launch alone (v_img: SSIM's gradient); rgb and gt are read again by K7 / the next step
template <bool NT>
__device__ __forceinline__ void expo_unpack(const float* p, float* o) {
  const float4 a = NT ? ld4_nt(p) : ld4(p), b = NT ? ld4_nt(p + 4) : ld4(p + 4), c = NT ? ld4_nt(p + 8) : ld4(p + 8);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  o[8] = c.x; o[9] = c.y; o[10] = c.z; o[11] = c.w;
}

template <bool VEC, bool HAS_GT, bool HAS_V>
__global__ __launch_bounds__(EXPO_THREADS) void k_expo_bwd_tiles(size_t npix, const float* __restrict__ rgb,
                                                                 const float* __restrict__ expo,
                                                                 const float* __restrict__ gt, float l1w,
                                                                 const float* __restrict__ v_img, float* __restrict__ v_rgb,
                                                                 float* __restrict__ partials) {
  __shared__ float sm[EXPO_WAVES][EXPO_SUMS];
  const ExpoK k = expo_load(expo);
  float s[EXPO_SUMS];
#pragma unroll
  for (int j = 0; j < EXPO_SUMS; j++) s[j] = 0.f;
  // no early exit: every lane takes part in the DPP sums below
#pragma unroll
  for (int r = 0; r < EXPO_ROUNDS; r++) {
    const size_t p = (size_t)blockIdx.x * EXPO_CHUNK + (size_t)(r * EXPO_THREADS + threadIdx.x) * 4;
    if (p >= npix) continue;
    if (VEC && p + 4 <= npix) {
      float in[12], g[12], vi[12], o[12];
      expo_unpack<false>(rgb + 3 * p, in);
      if (HAS_GT) expo_unpack<false>(gt + 3 * p, g);
      if (HAS_V) expo_unpack<true>(v_img + 3 * p, vi);
#pragma unroll
      for (int q = 0; q < 4; q++)
        expo_pixel<HAS_GT, HAS_V>(k, l1w, in[3 * q], in[3 * q + 1], in[3 * q + 2], g + 3 * q, vi + 3 * q, o + 3 * q, s);
      st4(v_rgb + 3 * p, make_float4(o[0], o[1], o[2], o[3]));     // (kept cached: K7 reads it next)
      st4(v_rgb + 3 * p + 4, make_float4(o[4], o[5], o[6], o[7]));
      st4(v_rgb + 3 * p + 8, make_float4(o[8], o[9], o[10], o[11]));
      continue;
    }
    const size_t e = p + 4 < npix ? p + 4 : npix;
    for (size_t i = p; i < e; i++) {
      float g[3] = {0.f, 0.f, 0.f}, vi[3] = {0.f, 0.f, 0.f}, o[3];
      if (HAS_GT) { g[0] = gt[3 * i]; g[1] = gt[3 * i + 1]; g[2] = gt[3 * i + 2]; }
      if (HAS_V) { vi[0] = v_img[3 * i]; vi[1] = v_img[3 * i + 1]; vi[2] = v_img[3 * i + 2]; }
      expo_pixel<HAS_GT, HAS_V>(k, l1w, rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], g, vi, o, s);
      v_rgb[3 * i] = o[0]; v_rgb[3 * i + 1] = o[1]; v_rgb[3 * i + 2] = o[2];
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < EXPO_SUMS; j++) {
    const float t = wave_sum_to_lane63(s[j]);
    if (lane == 63) sm[wave][j] = t;
  }
  __syncthreads();
  if (threadIdx.x < TGS_EXPO_OUT) {
    const int j = threadIdx.x;
    float t = 0.f;
    if (j < EXPO_SUMS) {
      t = sm[0][j];
#pragma unroll
      for (int w = 1; w < EXPO_WAVES; w++) t += sm[w][j];
    }
    // row = G[12] | mass[12] | 0 | sum |C' - gt| | pixels | 0...: the layout of out[]
    const int col = j < 24 ? j : (j < EXPO_SUMS ? j + 1 : (j == EXPO_SUMS ? 24 : j));
    partials[(size_t)blockIdx.x * TGS_EXPO_OUT + col] = t;
  }
}

__global__ __launch_bounds__(FOLD_THREADS) void k_expo_fold(int P, const float* __restrict__ partials, float l1w,
                                                            float* __restrict__ out, const int32_t* __restrict__ guard,
                                                            float* __restrict__ state, float lr, float b1, float b2,
                                                            float eps, float l2) {
  __shared__ double sm[FOLD_LANES][TGS_EXPO_OUT];
  __shared__ float G[12];
  const int tid = threadIdx.x;
  if (guard && guard[1]) {   // overflowed frame: all zeros, the state row keeps every bit
    if (tid < TGS_EXPO_OUT) out[tid] = 0.f;
    return;
  }
  const int j = tid & (TGS_EXPO_OUT - 1), r = tid / TGS_EXPO_OUT;
  double acc = 0.0;
  for (int i = r; i < P; i += FOLD_LANES) acc += (double)partials[(size_t)i * TGS_EXPO_OUT + j];
  sm[r][j] = acc;
  __syncthreads();
  if (tid < TGS_EXPO_OUT) {
    double t = sm[0][tid];
#pragma unroll
    for (int w = 1; w < FOLD_LANES; w++) t += sm[w][tid];
    float o = 0.f;
    if (tid < 24) o = (float)t;
    else if (tid == 24) o = 1.f;
    else if (tid == 25) o = (float)((double)l1w * t);
    else if (tid == 26) o = (float)t;
    out[tid] = o;
    if (tid < 12) G[tid] = o;
  }
  if (!state) return;   // (uniform)
  // t and the running products beta^t live in the row: read by all before thread 0 advances them
  const float p1 = state[37] * b1, p2 = state[38] * b2, steps = state[36];
  __syncthreads();
  if (tid < 12) {
    AdamK a = {};
    a.b1 = b1; a.b2 = b2; a.eps = eps; a.gscale = 1.f;
    a.ibc1 = 1.0f / (1.0f - p1);
    a.isq_bc2 = 1.0f / sqrtf(1.0f - p2);
    float e = state[tid], m = state[12 + tid], v = state[24 + tid];
    const float ident = (tid == 0 || tid == 5 || tid == 10) ? 1.f : 0.f;
    const float g = G[tid] + l2 * (e - ident);
    adam1(a, lr, e, g, m, v);
    state[tid] = e; state[12 + tid] = m; state[24 + tid] = v;
  } else if (tid == 12) {
    state[36] = steps + 1.f; state[37] = p1; state[38] = p2;
  }
}

}  // namespace

extern "C" int tgs_exposure_num_partials(int W, int H) {
  if (W < 1 || H < 1) return 0;
  return (int)(((size_t)W * H + EXPO_CHUNK - 1) / EXPO_CHUNK);
}

extern "C" int tgs_exposure_fwd(int W, int H, const float* rgb, const float* expo, float* rgb_out, void* stream) {
  TGS_CHECK_ARG(W >= 1 && H >= 1, "bad image size");
  TGS_CHECK_ARG(rgb && expo && rgb_out, "null rgb / expo / rgb_out");
  const size_t npix = (size_t)W * H;
  const unsigned blocks = (unsigned)tgs_exposure_num_partials(W, H);
  hipStream_t s = (hipStream_t)stream;
  if ((((uintptr_t)rgb | (uintptr_t)rgb_out) & 15) == 0)
    hipLaunchKernelGGL(k_expo_fwd<true>, dim3(blocks), dim3(EXPO_THREADS), 0, s, npix, rgb, expo, rgb_out);
  else
    hipLaunchKernelGGL(k_expo_fwd<false>, dim3(blocks), dim3(EXPO_THREADS), 0, s, npix, rgb, expo, rgb_out);
  TGS_CHECK_LAUNCH();
  return TGS_OK;
}

template <bool VEC>
static void expo_launch_tiles(unsigned blocks, hipStream_t s, size_t npix, const float* rgb, const float* expo, const float* gt,
                              float l1w, const float* v_img, float* v_rgb, float* partials) {
  if (gt && v_img)
    hipLaunchKernelGGL((k_expo_bwd_tiles<VEC, true, true>), dim3(blocks), dim3(EXPO_THREADS), 0, s, npix, rgb, expo, gt, l1w,
                       v_img, v_rgb, partials);
  else if (gt)
    hipLaunchKernelGGL((k_expo_bwd_tiles<VEC, true, false>), dim3(blocks), dim3(EXPO_THREADS), 0, s, npix, rgb, expo, gt, l1w,
                       v_img, v_rgb, partials);
  else if (v_img)
    hipLaunchKernelGGL((k_expo_bwd_tiles<VEC, false, true>), dim3(blocks), dim3(EXPO_THREADS), 0, s, npix, rgb, expo, gt, l1w,
                       v_img, v_rgb, partials);
  else
    hipLaunchKernelGGL((k_expo_bwd_tiles<VEC, false, false>), dim3(blocks), dim3(EXPO_THREADS), 0, s, npix, rgb, expo, gt, l1w,
                       v_img, v_rgb, partials);
}

extern "C" int tgs_exposure_bwd(int W, int H, const float* rgb, const float* expo, const float* gt, float l1_weight,
                                const float* v_img, float* v_rgb, float* partials, float* out, const int32_t* guard,
                                float* state, float lr, float beta1, float beta2, float eps, float l2, void* stream) {
  TGS_CHECK_ARG(W >= 1 && H >= 1, "bad image size");
  TGS_CHECK_ARG(rgb && expo && v_rgb, "null rgb / expo / v_rgb");
  TGS_CHECK_ARG(partials && out, "null partials / out");
  TGS_CHECK_ARG(!state || (beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f), "beta outside [0, 1)");
  const size_t npix = (size_t)W * H;
  const int P = tgs_exposure_num_partials(W, H);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = (((uintptr_t)rgb | (uintptr_t)gt | (uintptr_t)v_img | (uintptr_t)v_rgb) & 15) == 0;
  if (vec) expo_launch_tiles<true>((unsigned)P, s, npix, rgb, expo, gt, l1_weight, v_img, v_rgb, partials);
  else expo_launch_tiles<false>((unsigned)P, s, npix, rgb, expo, gt, l1_weight, v_img, v_rgb, partials);
  TGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_expo_fold, dim3(1), dim3(FOLD_THREADS), 0, s, P, partials, gt ? l1_weight : 0.f, out, guard, state, lr,
                     beta1, beta2, eps, l2);
  TGS_CHECK_LAUNCH();
  return TGS_OK;
}
