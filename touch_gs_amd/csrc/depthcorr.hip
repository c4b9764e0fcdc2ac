// depthcorr.hip -- scale-invariant (Pearson) monocular depth loss L = weight * (1 - rho(D_hat, M)) as an image-space op
// beside K6 / K7 (include/tgs.h, tgs_depth_corr_fwd_bwd): rho over the pixels with mono > 0 and 1 - final_T >= alpha_min
// between the expected depth x = out_depth / max(1 - final_T, 1e-10) and the raw monocular map y; the gradient images go
// to K7 as its upstream v_depth / v_alpha, the way K10's v_img does.  gfx950.
//
// Three launches, the image is read twice (3 planes read + 3 read and 2 written = 32 B per pixel):
//   k_dcorr_tiles : one wave per 16x16 tile, 4 px per lane in K7's prologue layout.  n, sum x, sum y by the wave
//                   reductions of tgs_common.h, the tile's own means, then the centred products about them while the pixels
//                   are still in registers -- variance after the mean, not from raw moments (DESIGN 5.1f on what the
//                   moment form costs in digits).  One record {n, mean_x, mean_y, M2x, M2y, Cxy, -, -} per tile.
//   k_dcorr_fold  : ONE workgroup combines the records pairwise (Chan et al.'s update) in fp64, in an order fixed by the
//                   thread count alone, and writes stats[8].
//   k_dcorr_grad  : one coalesced streaming pass; reads stats from memory, writes v_depth / v_alpha for EVERY pixel.
// No float atomics anywhere: the same inputs give the same bits.
#include <math.h>
#include "tgs_common.h"

namespace {

constexpr int REC = 8;              // floats per tile record (two 16-byte stores)
constexpr int TILE_WAVES = 4;       // tiles (= waves) per workgroup of k_dcorr_tiles
constexpr int FOLD_THREADS = 512;
constexpr int GRAD_THREADS = 256;

// The validity rule, in fp32 on the stored bits: references that read the same images make the same decision.
__device__ __forceinline__ bool dcorr_valid(float Tf, float m, float alpha_min) { return m > 0.f && (1.0f - Tf) >= alpha_min; }
__device__ __forceinline__ float dcorr_alpha(float Tf) { return fmaxf(1.0f - Tf, 1e-10f); }

__global__ __launch_bounds__(TILE_WAVES* TGS_WAVE) void k_dcorr_tiles(int W, int H, int TW, int T_total,
                                                                       const float* __restrict__ out_depth,
                                                                       const float* __restrict__ final_T,
                                                                       const float* __restrict__ mono, float alpha_min,
                                                                       float* __restrict__ tile_moments) {
  const int tile = blockIdx.x * TILE_WAVES + (threadIdx.x >> 6);   // wave-uniform
  if (tile >= T_total) return;
  const int lane = threadIdx.x & 63;
  const int ty = tile / TW, tx = tile - ty * TW;
  const int g = lane >> 4, lx = 4 * (g & 1) + (lane & 3), ly = 4 * (g >> 1) + ((lane >> 2) & 3);
  float x[4], y[4];
  bool ok[4];
  float cnt = 0.f, sx = 0.f, sy = 0.f;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int px = tx * TGS_BLOCK + 8 * (k & 1) + lx;
    const int py = ty * TGS_BLOCK + 8 * (k >> 1) + ly;
    ok[k] = false; x[k] = y[k] = 0.f;
    if (px < W && py < H) {
      const size_t p = (size_t)py * W + px;
      const float Tf = final_T[p], m = mono[p], od = out_depth[p];
      if (dcorr_valid(Tf, m, alpha_min)) {
        ok[k] = true;
        x[k] = od / dcorr_alpha(Tf);
        y[k] = m;
        cnt += 1.f; sx += x[k]; sy += y[k];
      }
    }
  }
  const float n = wave_sum(cnt);
  // a true division: the mean of n copies of one value is that value whenever their sum is exact (a constant image has no variance)
  const float den = fmaxf(n, 1.f);
  const float mx = wave_sum(sx) / den, my = wave_sum(sy) / den;
  float m2x = 0.f, m2y = 0.f, cxy = 0.f;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (ok[k]) {
      const float dx = x[k] - mx, dy = y[k] - my;
      m2x += dx * dx; m2y += dy * dy; cxy += dx * dy;
    }
  }
  m2x = wave_sum(m2x); m2y = wave_sum(m2y); cxy = wave_sum(cxy);
  if (lane == 0) {
    float* r = tile_moments + (size_t)tile * REC;
    st4(r, make_float4(n, mx, my, m2x));
    st4(r + 4, make_float4(m2y, cxy, 0.f, 0.f));
  }
}

struct Mom { double n, mx, my, m2x, m2y, cxy; };

// Chan, Golub & LeVeque's pairwise update of count, means and centred second moments.
__device__ __forceinline__ Mom dcorr_combine(const Mom& a, const Mom& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  Mom r;
  r.n = a.n + b.n;
  const double dx = b.mx - a.mx, dy = b.my - a.my, fb = b.n / r.n, w = a.n * fb;
  r.mx = a.mx + dx * fb;
  r.my = a.my + dy * fb;
  r.m2x = a.m2x + b.m2x + dx * dx * w;
  r.m2y = a.m2y + b.m2y + dy * dy * w;
  r.cxy = a.cxy + b.cxy + dx * dy * w;
  return r;
}

// The frame is degenerate (rho = 0, loss 0, all gradients 0) if n < 2 or vx * vy is not > 0 or not finite.  Decided on
// the fp32 values of stats[], in fp64 (the product of two floats neither overflows nor underflows there), so that
// k_dcorr_grad, which sees only stats[], decides the same.
__device__ __forceinline__ bool dcorr_degenerate(float n, float vx, float vy) {
  const double q = (double)vx * (double)vy;
  return !(n >= 2.f) || !(q > 0.0) || !isfinite(q);
}

__global__ __launch_bounds__(FOLD_THREADS) void k_dcorr_fold(int T_total, const float* __restrict__ tile_moments, float weight,
                                                             float* __restrict__ stats) {
  __shared__ Mom sm[FOLD_THREADS];
  const int t = threadIdx.x;
  Mom a = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = t; i < T_total; i += FOLD_THREADS) {
    const float4 r0 = ld4(tile_moments + (size_t)i * REC), r1 = ld4(tile_moments + (size_t)i * REC + 4);
    const Mom b = {(double)r0.x, (double)r0.y, (double)r0.z, (double)r0.w, (double)r1.x, (double)r1.y};
    a = dcorr_combine(a, b);
  }
  sm[t] = a;
  __syncthreads();
  for (int s = FOLD_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) sm[t] = dcorr_combine(sm[t], sm[t + s]);
    __syncthreads();
  }
  if (t == 0) {
    const Mom m = sm[0];
    const double inv = m.n > 0.0 ? 1.0 / m.n : 0.0;
    const double vx = m.m2x * inv, vy = m.m2y * inv, c = m.cxy * inv;
    const float nf = (float)m.n, vxf = (float)vx, vyf = (float)vy;
    float rho = 0.f, loss = 0.f;
    if (!dcorr_degenerate(nf, vxf, vyf)) {
      const double r = c / sqrt(vx * vy);
      rho = (float)r;
      loss = (float)((double)weight * (1.0 - r));
    }
    st4(stats, make_float4(nf, (float)m.mx, (float)m.my, vxf));
    st4(stats + 4, make_float4(vyf, (float)c, rho, loss));
  }
}

// g = -weight * d rho / d x = gs * ((y - my) - beta (x - mx)),  gs = -weight / (n sqrt(vx vy)),  beta = c / vx
struct GradK { float mx, my, beta, gs, alpha_min; };

__device__ __forceinline__ GradK dcorr_gradk(const float* __restrict__ stats, float weight, float alpha_min) {
  const float4 s0 = ld4(stats), s1 = ld4(stats + 4);
  GradK k;
  k.mx = s0.y; k.my = s0.z; k.alpha_min = alpha_min;
  const float n = s0.x, vx = s0.w, vy = s1.x, c = s1.y;
  if (dcorr_degenerate(n, vx, vy)) {
    k.beta = 0.f; k.gs = 0.f;
    k.alpha_min = __builtin_nanf("");   // no compare against it holds: no pixel is valid, exact zeros whatever the images hold
  } else {
    k.beta = c / vx;
    k.gs = (float)(-(double)weight / ((double)n * sqrt((double)vx * (double)vy)));
  }
  return k;
}

__device__ __forceinline__ void dcorr_pixel(const GradK& k, float od, float Tf, float m, float& vd, float& va) {
  vd = 0.f; va = 0.f;
  if (dcorr_valid(Tf, m, k.alpha_min)) {
    const float alpha = dcorr_alpha(Tf);
    const float x = od / alpha;
    const float gpix = k.gs * ((m - k.my) - k.beta * (x - k.mx));
    vd = gpix / alpha;
    va = -(gpix * x) / alpha;   // K7's convention: the gradient with respect to 1 - final_T
  }
}

// VEC: every image pointer is 16-byte aligned; a thread owns 4 consecutive pixels of the flat [H * W] image.
template <bool VEC>
__global__ __launch_bounds__(GRAD_THREADS) void k_dcorr_grad(size_t npix, const float* __restrict__ out_depth,
                                                             const float* __restrict__ final_T, const float* __restrict__ mono,
                                                             float alpha_min, float weight, const float* __restrict__ stats,
                                                             float* __restrict__ v_depth, float* __restrict__ v_alpha) {
  const GradK k = dcorr_gradk(stats, weight, alpha_min);
  const size_t i = ((size_t)blockIdx.x * GRAD_THREADS + threadIdx.x) * 4;
  if (i >= npix) return;
  if (VEC && i + 4 <= npix) {
    const float4 od = ld4(out_depth + i), Tf = ld4(final_T + i), m = ld4(mono + i);
    float4 vd, va;
    dcorr_pixel(k, od.x, Tf.x, m.x, vd.x, va.x);
    dcorr_pixel(k, od.y, Tf.y, m.y, vd.y, va.y);
    dcorr_pixel(k, od.z, Tf.z, m.z, vd.z, va.z);
    dcorr_pixel(k, od.w, Tf.w, m.w, vd.w, va.w);
    if (v_depth) st4(v_depth + i, vd);
    if (v_alpha) st4(v_alpha + i, va);
    return;
  }
  const size_t e = i + 4 < npix ? i + 4 : npix;
  for (size_t p = i; p < e; p++) {
    float vd, va;
    dcorr_pixel(k, out_depth[p], final_T[p], mono[p], vd, va);
    if (v_depth) v_depth[p] = vd;
    if (v_alpha) v_alpha[p] = va;
  }
}

}  // namespace

extern "C" int tgs_depth_corr_fwd_bwd(int W, int H, const float* out_depth, const float* final_T, const float* mono,
                                      float alpha_min, float weight, float* tile_moments, float* stats,
                                      float* v_depth, float* v_alpha, void* stream) {
  TGS_CHECK_ARG(W >= 1 && H >= 1, "bad image size");
  TGS_CHECK_ARG(out_depth && final_T && mono, "null image");
  TGS_CHECK_ARG(tile_moments && stats, "null tile_moments / stats");
  TGS_CHECK_ARG(alpha_min > 0.f && alpha_min <= 1.f, "alpha_min outside (0, 1]");
  TGS_CHECK_ARG(((uintptr_t)tile_moments & 15) == 0 && ((uintptr_t)stats & 15) == 0, "tile_moments / stats not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int TW = (W + TGS_BLOCK - 1) / TGS_BLOCK, TH = (H + TGS_BLOCK - 1) / TGS_BLOCK;
  const int T = TW * TH;
  hipLaunchKernelGGL(k_dcorr_tiles, dim3((T + TILE_WAVES - 1) / TILE_WAVES), dim3(TILE_WAVES * TGS_WAVE), 0, s, W, H, TW, T,
                     out_depth, final_T, mono, alpha_min, tile_moments);
  TGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_dcorr_fold, dim3(1), dim3(FOLD_THREADS), 0, s, T, tile_moments, weight, stats);
  TGS_CHECK_LAUNCH();
  if (v_depth || v_alpha) {
    const size_t npix = (size_t)W * H;
    const unsigned blocks = (unsigned)((npix + 4 * GRAD_THREADS - 1) / (4 * GRAD_THREADS));
    const bool vec = (((uintptr_t)out_depth | (uintptr_t)final_T | (uintptr_t)mono | (uintptr_t)v_depth | (uintptr_t)v_alpha) & 15) == 0;
    if (vec)
      hipLaunchKernelGGL(k_dcorr_grad<true>, dim3(blocks), dim3(GRAD_THREADS), 0, s, npix, out_depth, final_T, mono, alpha_min,
                         weight, stats, v_depth, v_alpha);
    else
      hipLaunchKernelGGL(k_dcorr_grad<false>, dim3(blocks), dim3(GRAD_THREADS), 0, s, npix, out_depth, final_T, mono, alpha_min,
                         weight, stats, v_depth, v_alpha);
    TGS_CHECK_LAUNCH();
  }
  return TGS_OK;
}
