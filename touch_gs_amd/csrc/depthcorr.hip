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
//
// The patch-wise (local) term (tgs_depth_corr_local_fwd_bwd) runs the first two launches unchanged, then
//   k_dcorr_patches    : one wave per patch of k x k tiles; the lanes combine the patch's <= 256 tile records with
//                        dcorr_combine in fp64 (a lane's records in order, then a tree over the lanes by 64-bit shuffles:
//                        an order fixed by the lane count alone), lane 0 applies the gates against stats[] and writes one
//                        32-byte patch record {active, mx, my, beta, 1 / (n sqrt(vx vy)), rho, n, counted}.
//   k_dcorr_patch_sum  : ONE workgroup sums rho_p, the active and the counted patches in fp64, fixed order -> stats[8..15].
//   k_dcorr_grad_local : the streaming pass of k_dcorr_grad with the patch's record (L2) added: global + local gradient
//                        in one pass, a thread owns 4 pixels of one row (one tile, one patch); activity is the stored flag.
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

// ---- patch-wise (local) term --------------------------------------------------------------------------------------------
constexpr int PATCH_WAVES = 4;      // patches (= waves) per workgroup of k_dcorr_patches
constexpr int PSUM_THREADS = 256;
constexpr int PREC = 8;             // floats per patch record (two 16-byte stores)

struct PatchGrid { int k, off_x, off_y, PW, PH; };

__device__ __forceinline__ Mom dcorr_shfl_down(const Mom& a, int s) {
  Mom r;
  r.n = __shfl_down(a.n, s); r.mx = __shfl_down(a.mx, s); r.my = __shfl_down(a.my, s);
  r.m2x = __shfl_down(a.m2x, s); r.m2y = __shfl_down(a.m2y, s); r.cxy = __shfl_down(a.cxy, s);
  return r;
}

__global__ __launch_bounds__(PATCH_WAVES* TGS_WAVE) void k_dcorr_patches(int TW, int TH, PatchGrid pg,
                                                                         const float* __restrict__ tile_moments,
                                                                         const float* __restrict__ stats, int min_count,
                                                                         float min_var_ratio, float* __restrict__ patch_stats) {
  const int patch = blockIdx.x * PATCH_WAVES + (threadIdx.x >> 6);   // wave-uniform
  if (patch >= pg.PW * pg.PH) return;
  const int lane = threadIdx.x & 63;
  const int py = patch / pg.PW, px = patch - py * pg.PW;
  const int tx0 = px * pg.k - pg.off_x, ty0 = py * pg.k - pg.off_y;   // (may be negative: a partial border patch)
  Mom a = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = lane; j < pg.k * pg.k; j += TGS_WAVE) {
    const int jy = j / pg.k, tx = tx0 + (j - jy * pg.k), ty = ty0 + jy;
    if (tx >= 0 && tx < TW && ty >= 0 && ty < TH) {
      const float* r = tile_moments + ((size_t)ty * TW + tx) * REC;
      const float4 r0 = ld4(r), r1 = ld4(r + 4);
      const Mom b = {(double)r0.x, (double)r0.y, (double)r0.z, (double)r0.w, (double)r1.x, (double)r1.y};
      a = dcorr_combine(a, b);
    }
  }
  // 64-bit moves built from 32-bit cross-lane moves; every lane runs the tree, lane 0 ends with ((0+32)+(16+48))+...
  for (int s = TGS_WAVE / 2; s > 0; s >>= 1) a = dcorr_combine(a, dcorr_shfl_down(a, s));
  if (lane == 0) {
    const float4 s0 = ld4(stats), s1 = ld4(stats + 4);
    const double inv = a.n > 0.0 ? 1.0 / a.n : 0.0;
    const double vx = a.m2x * inv, vy = a.m2y * inv, c = a.cxy * inv, q = vx * vy;
    const bool counted = a.n >= (double)min_count;   // counts are exact in fp32 and in fp64
    const bool active = counted && !dcorr_degenerate(s0.x, s0.w, s1.x) && vx >= (double)min_var_ratio * (double)s0.w &&
                        vy >= (double)min_var_ratio * (double)s1.x && q > 0.0 && isfinite(q);
    float beta = 0.f, gs = 0.f, rho = 0.f;
    if (active) {
      const double sq = sqrt(q);
      beta = (float)(c / vx); gs = (float)(1.0 / (a.n * sq)); rho = (float)(c / sq);
    }
    float* r = patch_stats + (size_t)patch * PREC;
    st4(r, make_float4(active ? 1.f : 0.f, (float)a.mx, (float)a.my, beta));
    st4(r + 4, make_float4(gs, rho, (float)a.n, counted ? 1.f : 0.f));
  }
}

__global__ __launch_bounds__(PSUM_THREADS) void k_dcorr_patch_sum(int P_total, const float* __restrict__ patch_stats,
                                                                  float weight_local, float* __restrict__ stats) {
  __shared__ double sm[3][PSUM_THREADS];
  const int t = threadIdx.x;
  double rho = 0.0, act = 0.0, cnt = 0.0;
  for (int i = t; i < P_total; i += PSUM_THREADS) {
    const float4 r0 = ld4(patch_stats + (size_t)i * PREC), r1 = ld4(patch_stats + (size_t)i * PREC + 4);
    if (r0.x != 0.f) { rho += (double)r1.y; act += 1.0; }
    cnt += (double)r1.w;
  }
  sm[0][t] = rho; sm[1][t] = act; sm[2][t] = cnt;
  __syncthreads();
  for (int s = PSUM_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) { sm[0][t] += sm[0][t + s]; sm[1][t] += sm[1][t + s]; sm[2][t] += sm[2][t + s]; }
    __syncthreads();
  }
  if (t == 0) {
    const double A = sm[1][0], mean = A > 0.0 ? sm[0][0] / A : 0.0;
    const float loc = A > 0.0 ? (float)((double)weight_local * (1.0 - mean)) : 0.f;
    st4(stats + 8, make_float4((float)sm[2][0], (float)A, (float)mean, loc));
    st4(stats + 12, make_float4(stats[7] + loc, 0.f, 0.f, 0.f));
  }
}

// The local part of a pixel's gradient on top of dcorr_pixel's global one: g = g_glob + gl ((y - my_p) - beta_p (x - mx_p)),
// gl = -(weight_local / A) / (n_p sqrt(vx_p vy_p)) on an active patch and 0 (nothing added) elsewhere.
struct PatchK { float mx, my, beta, gl; bool active; };

__device__ __forceinline__ void dcorr_pixel_local(const GradK& k, const PatchK& pk, float od, float Tf, float m, float& vd,
                                                  float& va) {
  vd = 0.f; va = 0.f;
  if (dcorr_valid(Tf, m, k.alpha_min)) {
    const float alpha = dcorr_alpha(Tf);
    const float x = od / alpha;
    float gpix = k.gs * ((m - k.my) - k.beta * (x - k.mx));
    if (pk.active) gpix += pk.gl * ((m - pk.my) - pk.beta * (x - pk.mx));
    vd = gpix / alpha;
    va = -(gpix * x) / alpha;
  }
}

// A thread owns 4 consecutive pixels of ONE row (W4 = ceil(W / 4) threads per row): one tile, one patch record.
// VEC: W % 4 == 0 and every image pointer is 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(GRAD_THREADS) void k_dcorr_grad_local(int W, int H, int W4, PatchGrid pg,
                                                                   const float* __restrict__ out_depth,
                                                                   const float* __restrict__ final_T,
                                                                   const float* __restrict__ mono, float alpha_min,
                                                                   float weight_global, float weight_local,
                                                                   const float* __restrict__ stats,
                                                                   const float* __restrict__ patch_stats,
                                                                   float* __restrict__ v_depth, float* __restrict__ v_alpha) {
  const GradK k = dcorr_gradk(stats, weight_global, alpha_min);
  const size_t t = (size_t)blockIdx.x * GRAD_THREADS + threadIdx.x;
  if (t >= (size_t)W4 * H) return;
  const int row = (int)(t / W4), px0 = 4 * (int)(t - (size_t)row * W4);
  const int patch = ((row >> 4) + pg.off_y) / pg.k * pg.PW + ((px0 >> 4) + pg.off_x) / pg.k;
  const float4 p0 = ld4(patch_stats + (size_t)patch * PREC);
  PatchK pk;
  pk.active = p0.x != 0.f;      // the stored decision: no gate is evaluated here
  pk.mx = p0.y; pk.my = p0.z; pk.beta = p0.w;
  pk.gl = -(weight_local / stats[9]) * patch_stats[(size_t)patch * PREC + 4];   // (read only where active: A >= 1 there)
  const size_t i = (size_t)row * W + px0;
  if (VEC) {
    const float4 od = ld4(out_depth + i), Tf = ld4(final_T + i), m = ld4(mono + i);
    float4 vd, va;
    dcorr_pixel_local(k, pk, od.x, Tf.x, m.x, vd.x, va.x);
    dcorr_pixel_local(k, pk, od.y, Tf.y, m.y, vd.y, va.y);
    dcorr_pixel_local(k, pk, od.z, Tf.z, m.z, vd.z, va.z);
    dcorr_pixel_local(k, pk, od.w, Tf.w, m.w, vd.w, va.w);
    if (v_depth) st4(v_depth + i, vd);
    if (v_alpha) st4(v_alpha + i, va);
    return;
  }
  const int e = px0 + 4 < W ? 4 : W - px0;
  for (int j = 0; j < e; j++) {
    float vd, va;
    dcorr_pixel_local(k, pk, out_depth[i + j], final_T[i + j], mono[i + j], vd, va);
    if (v_depth) v_depth[i + j] = vd;
    if (v_alpha) v_alpha[i + j] = va;
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

extern "C" int tgs_depth_corr_local_fwd_bwd(int W, int H, const float* out_depth, const float* final_T, const float* mono,
                                            float alpha_min, float weight_global, float weight_local, int patch_tiles,
                                            int off_x, int off_y, int min_count, float min_var_ratio, float* tile_moments,
                                            float* patch_stats, float* stats, float* v_depth, float* v_alpha, void* stream) {
  TGS_CHECK_ARG(W >= 1 && H >= 1, "bad image size");
  TGS_CHECK_ARG(out_depth && final_T && mono, "null image");
  TGS_CHECK_ARG(tile_moments && patch_stats && stats, "null tile_moments / patch_stats / stats");
  TGS_CHECK_ARG(alpha_min > 0.f && alpha_min <= 1.f, "alpha_min outside (0, 1]");
  TGS_CHECK_ARG(patch_tiles >= 1 && patch_tiles <= 16, "patch_tiles outside 1...16");
  TGS_CHECK_ARG(off_x >= 0 && off_x < patch_tiles && off_y >= 0 && off_y < patch_tiles, "patch offset outside [0, patch_tiles)");
  TGS_CHECK_ARG(min_count >= 2, "min_count < 2");
  TGS_CHECK_ARG(min_var_ratio >= 0.f && isfinite(min_var_ratio), "min_var_ratio negative or not finite");
  TGS_CHECK_ARG((((uintptr_t)tile_moments | (uintptr_t)patch_stats | (uintptr_t)stats) & 15) == 0,
                "tile_moments / patch_stats / stats not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int TW = (W + TGS_BLOCK - 1) / TGS_BLOCK, TH = (H + TGS_BLOCK - 1) / TGS_BLOCK;
  const int T = TW * TH;
  PatchGrid pg;
  pg.k = patch_tiles; pg.off_x = off_x; pg.off_y = off_y;
  pg.PW = (TW + off_x + patch_tiles - 1) / patch_tiles;
  pg.PH = (TH + off_y + patch_tiles - 1) / patch_tiles;
  const int P = pg.PW * pg.PH;
  // the first two launches are those of tgs_depth_corr_fwd_bwd: stats[0..7] hold the same bits
  hipLaunchKernelGGL(k_dcorr_tiles, dim3((T + TILE_WAVES - 1) / TILE_WAVES), dim3(TILE_WAVES * TGS_WAVE), 0, s, W, H, TW, T,
                     out_depth, final_T, mono, alpha_min, tile_moments);
  TGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_dcorr_fold, dim3(1), dim3(FOLD_THREADS), 0, s, T, tile_moments, weight_global, stats);
  TGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_dcorr_patches, dim3((P + PATCH_WAVES - 1) / PATCH_WAVES), dim3(PATCH_WAVES * TGS_WAVE), 0, s, TW, TH, pg,
                     tile_moments, stats, min_count, min_var_ratio, patch_stats);
  TGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_dcorr_patch_sum, dim3(1), dim3(PSUM_THREADS), 0, s, P, patch_stats, weight_local, stats);
  TGS_CHECK_LAUNCH();
  if (v_depth || v_alpha) {
    const int W4 = (W + 3) / 4;
    const unsigned blocks = (unsigned)(((size_t)W4 * H + GRAD_THREADS - 1) / GRAD_THREADS);
    const bool vec = (W & 3) == 0 &&
                     (((uintptr_t)out_depth | (uintptr_t)final_T | (uintptr_t)mono | (uintptr_t)v_depth | (uintptr_t)v_alpha) & 15) == 0;
    if (vec)
      hipLaunchKernelGGL(k_dcorr_grad_local<true>, dim3(blocks), dim3(GRAD_THREADS), 0, s, W, H, W4, pg, out_depth, final_T,
                         mono, alpha_min, weight_global, weight_local, stats, patch_stats, v_depth, v_alpha);
    else
      hipLaunchKernelGGL(k_dcorr_grad_local<false>, dim3(blocks), dim3(GRAD_THREADS), 0, s, W, H, W4, pg, out_depth, final_T,
                         mono, alpha_min, weight_global, weight_local, stats, patch_stats, v_depth, v_alpha);
    TGS_CHECK_LAUNCH();
  }
  return TGS_OK;
}
