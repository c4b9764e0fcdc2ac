// depthnormal.hip -- surface normals from the rendered depth and the normal-prior loss
//   L = weight * sum_i c_i (1 - n_i . p_i / |p_i|) / sum_i c_i
// as an image-space op beside K6 / K7 (include/tgs.h, tgs_depth_normal_fwd_bwd).  n = the unit normal of the
// surface through the back-projected expected depths of a pixel's four neighbours (central differences, facing the
// camera); the gradient images go to K7 as its upstream v_depth / v_alpha, the way the Pearson terms' do.  gfx950.
//
// Three launches, ordered by the launches alone:
//   k_dnorm_tiles : one wave per 16x16 tile.  x = out_depth / alpha and validity of the tile and a 1-pixel halo (18x18) are
//                   staged in LDS; a lane forms the normals of 4 centres, optionally writes them, and the wave reduces
//                   {formed, supervised, sum c, sum c (1 - cos)} by the DPP sums of tgs_common.h into one 16-byte record.
//   k_dnorm_fold  : ONE workgroup sums the records in fp64, in an order fixed by the thread count alone -> stats[8].
//   k_dnorm_grad  : one wave per tile with a 2-pixel halo: x and validity on 20x20, the centre terms g_tx, g_ty recomputed
//                   from them on the 18x18 centres (they never travel through HBM) and left in LDS as the four scalars
//                   r . g a centre hands its four neighbour pixels, then the GATHER form: a thread sums the four
//                   contributions its own pixel receives and writes (or adds to) v_depth / v_alpha.  All its global loads
//                   are issued ahead of the first barrier.
// No float atomics anywhere: the same inputs give the same bits.
//
// Lane layout: consecutive lanes own consecutive pixels of a row (16 lanes = one 64-byte row segment of the tile; the
// staging loops walk the halo tile row-major the same way), so every global access is contiguous across lanes whatever
// the alignment of the images -- there is no vector / scalar pair of kernels and unaligned views give the same bits by
// construction.  In LDS (pitch 24 floats) the two rows a 32-lane half reads are 2 rows apart: 48 floats = 16 banks, so
// the half covers all 32 banks once, also for the +-1 / +-pitch neighbour reads.
//
// Built with -ffp-contract=on (build.sh): dnorm_centre is inlined into k_dnorm_tiles AND k_dnorm_grad, and the two must
// decide "formed" alike and see the same n and |m|.
#include <math.h>
#include "tgs_common.h"

namespace {

constexpr int PITCH = 24;           // floats per LDS row: >= 20, see the bank note above
constexpr int TILE_WAVES = 4;       // tiles (= waves) per workgroup
constexpr int FOLD_THREADS = 512;
constexpr int HT = TGS_BLOCK + 2;   // staged rows / columns of k_dnorm_tiles
constexpr int HG = TGS_BLOCK + 4;   // ... of k_dnorm_grad; its centres are HT x HT

struct DnCam { float ifx, ify, cx, cy, pc; int W, H; };   // ifx, ify = 1.0f / fx, 1.0f / fy, rounded once on the host
struct V3 { float x, y, z; };

__device__ __forceinline__ V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return v3(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

__device__ __forceinline__ float dnorm_rx(const DnCam& c, int px) { return ((float)px + c.pc - c.cx) * c.ifx; }
__device__ __forceinline__ float dnorm_ry(const DnCam& c, int py) { return ((float)py + c.pc - c.cy) * c.ify; }

// Row of the tile that lane `lane` owns in pass k (0...3); its column is lane & 15.
__device__ __forceinline__ int dnorm_row(int lane, int k) { return 4 * k + 2 * ((lane >> 4) & 1) + (lane >> 5); }

// x and validity of the (TGS_BLOCK + 2 R)^2 pixels around the tile at (x0, y0); a pixel outside the image is invalid.
// The validity rule, in fp32 on the stored bits, is tgs_depth_corr_fwd_bwd's.
template <int R>
__device__ __forceinline__ void dnorm_stage(const DnCam& c, int x0, int y0, const float* __restrict__ out_depth,
                                            const float* __restrict__ final_T, float alpha_min, float* sx,
                                            unsigned char* sv, int lane) {
  constexpr int S = TGS_BLOCK + 2 * R;
  // the loads are unconditional, from a position clamped into the image, so that the passes' loads go out together
#pragma unroll
  for (int it = 0; it < (S * S + TGS_WAVE - 1) / TGS_WAVE; it++) {
    const int i = lane + it * TGS_WAVE, ic = min(i, S * S - 1);
    const int hy = ic / S, hx = ic - hy * S;
    const int px = x0 - R + hx, py = y0 - R + hy;
    const bool in = px >= 0 && px < c.W && py >= 0 && py < c.H;
    const size_t p = (size_t)min(max(py, 0), c.H - 1) * c.W + min(max(px, 0), c.W - 1);
    const float a = 1.0f - final_T[p];
    const float x = out_depth[p] / fmaxf(a, 1e-10f);
    if (i < S * S) {
      sx[hy * PITCH + hx] = in ? x : 0.f;
      sv[hy * PITCH + hx] = (in && a >= alpha_min) ? 1 : 0;
    }
  }
}

struct Centre { V3 tx, ty, n; float len; };

// |v| for a squared length that is a NORMAL fp32 number; false otherwise: a squared length that underflows fp32's normal
// range (a length below 1.1e-19) counts as 0, one that overflows as not finite.
__device__ __forceinline__ bool dnorm_length(V3 v, float& len) {
  const float q = dot(v, v);
  if (!(q >= 1.17549435e-38f) || !isfinite(q)) return false;
  len = sqrtf(q);
  return true;
}

// The normal at the centre with LDS index idx and pixel (px, py); false = not formed.  An image-border centre has an
// out-of-image (= invalid) neighbour, so "interior" needs no test of its own.
__device__ __forceinline__ bool dnorm_centre(const DnCam& c, const float* sx, const unsigned char* sv, int idx, int px, int py,
                                             float max_jump, Centre& o) {
  if (!(sv[idx] & sv[idx - 1] & sv[idx + 1] & sv[idx - PITCH] & sv[idx + PITCH])) return false;
  const float xi = sx[idx], xl = sx[idx - 1], xr = sx[idx + 1], xu = sx[idx - PITCH], xd = sx[idx + PITCH];
  if (max_jump > 0.f && !(fmaxf(fabsf(xr - xl), fabsf(xd - xu)) <= max_jump * xi)) return false;
  const float rxl = dnorm_rx(c, px - 1), rxc = dnorm_rx(c, px), rxr = dnorm_rx(c, px + 1);
  const float ryu = dnorm_ry(c, py - 1), ryc = dnorm_ry(c, py), ryd = dnorm_ry(c, py + 1);
  o.tx = v3(xr * rxr, xr * ryc, xr) - v3(xl * rxl, xl * ryc, xl);
  o.ty = v3(xd * rxc, xd * ryd, xd) - v3(xu * rxc, xu * ryu, xu);
  const V3 m = cross(o.ty, o.tx);
  if (!dnorm_length(m, o.len)) return false;
  o.n = m / o.len;   // true divisions: a plane at constant depth gives (0, 0, -1) exactly
  return true;
}

// The prior q with weight w: false = no supervision there (length 0 or not finite, see dnorm_length, or weight not > 0).
// The unit prior is q / pl; the callers divide once, after their dot product.
__device__ __forceinline__ bool dnorm_prior(V3 q, float w, float& pl) { return w > 0.f && dnorm_length(q, pl); }

__device__ __forceinline__ V3 dnorm_load_prior(const float* __restrict__ prior, size_t p) {
  return v3(prior[3 * p], prior[3 * p + 1], prior[3 * p + 2]);
}

__global__ __launch_bounds__(TILE_WAVES* TGS_WAVE) void k_dnorm_tiles(DnCam c, int TW, int T_total,
                                                                       const float* __restrict__ out_depth,
                                                                       const float* __restrict__ final_T,
                                                                       const float* __restrict__ prior,
                                                                       const float* __restrict__ conf, float alpha_min,
                                                                       float max_jump, float* __restrict__ tile_sums,
                                                                       float* __restrict__ normals) {
  __shared__ float sx_all[TILE_WAVES][HT * PITCH];
  __shared__ unsigned char sv_all[TILE_WAVES][HT * PITCH];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x * TILE_WAVES + wave;   // wave-uniform
  const bool live = tile < T_total;
  const int ty = tile / TW, tx = tile - ty * TW;
  const int x0 = tx * TGS_BLOCK, y0 = ty * TGS_BLOCK;
  float* sx = sx_all[wave];
  unsigned char* sv = sv_all[wave];
  if (live) dnorm_stage<1>(c, x0, y0, out_depth, final_T, alpha_min, sx, sv, lane);
  __syncthreads();
  if (!live) return;
  float formed = 0.f, sup = 0.f, sc = 0.f, sl = 0.f;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int row = dnorm_row(lane, k), col = lane & 15;
    const int px = x0 + col, py = y0 + row;
    if (px < c.W && py < c.H) {
      const size_t p = (size_t)py * c.W + px;
      Centre ce;
      const bool f = dnorm_centre(c, sx, sv, (row + 1) * PITCH + col + 1, px, py, max_jump, ce);
      if (normals) {
        normals[3 * p] = f ? ce.n.x : 0.f;
        normals[3 * p + 1] = f ? ce.n.y : 0.f;
        normals[3 * p + 2] = f ? ce.n.z : 0.f;
      }
      if (f) {
        formed += 1.f;
        float pl;
        const float w = conf ? conf[p] : 1.f;
        const V3 q = prior ? dnorm_load_prior(prior, p) : v3(0.f, 0.f, 0.f);
        if (dnorm_prior(q, w, pl)) {
          sup += 1.f;
          sc += w;
          sl += w * (1.f - dot(ce.n, q) / pl);
        }
      }
    }
  }
  formed = wave_sum(formed); sup = wave_sum(sup); sc = wave_sum(sc); sl = wave_sum(sl);
  if (lane == 0) st4(tile_sums + (size_t)tile * 4, make_float4(formed, sup, sc, sl));
}

__global__ __launch_bounds__(FOLD_THREADS) void k_dnorm_fold(int T_total, const float* __restrict__ tile_sums, float weight,
                                                             float* __restrict__ stats) {
  __shared__ double sm[4][FOLD_THREADS];
  const int t = threadIdx.x;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int i = t; i < T_total; i += FOLD_THREADS) {
    const float4 r = ld4(tile_sums + (size_t)i * 4);
    a0 += (double)r.x; a1 += (double)r.y; a2 += (double)r.z; a3 += (double)r.w;
  }
  sm[0][t] = a0; sm[1][t] = a1; sm[2][t] = a2; sm[3][t] = a3;
  __syncthreads();
  for (int s = FOLD_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int j = 0; j < 4; j++) sm[j][t] += sm[j][t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double C = sm[2][0];
    const bool any = sm[1][0] > 0.0 && C > 0.0;
    const double mean = any ? sm[3][0] / C : 0.0;
    st4(stats, make_float4((float)sm[0][0], (float)sm[1][0], (float)C, (float)mean));
    st4(stats + 4, make_float4(any ? (float)((double)weight * mean) : 0.f, 0.f, 0.f, 0.f));
  }
}

constexpr int CENTRE_PASSES = (HT * HT + TGS_WAVE - 1) / TGS_WAVE;   // 6: the 324 centres over the 64 lanes

template <bool ACC>
__global__ __launch_bounds__(TILE_WAVES* TGS_WAVE) void k_dnorm_grad(DnCam c, int TW, int T_total,
                                                                      const float* __restrict__ out_depth,
                                                                      const float* __restrict__ final_T,
                                                                      const float* __restrict__ prior,
                                                                      const float* __restrict__ conf, float alpha_min,
                                                                      float max_jump, float weight,
                                                                      const float* __restrict__ stats, float* v_depth,
                                                                      float* v_alpha) {
  __shared__ float sx_all[TILE_WAVES][HG * PITCH];
  __shared__ unsigned char sv_all[TILE_WAVES][HG * PITCH];
  // per centre of the 18 x 18 grid, what it hands its right / left / lower / upper neighbour pixel:
  //   r_right . g_tx,  -r_left . g_tx,  r_lower . g_ty,  -r_upper . g_ty   (the centre terms never travel through HBM)
  __shared__ float sg_all[TILE_WAVES][4][HT * PITCH];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x * TILE_WAVES + wave;   // wave-uniform
  const bool live = tile < T_total;
  const int ty = tile / TW, tx = tile - ty * TW;
  const int x0 = tx * TGS_BLOCK, y0 = ty * TGS_BLOCK;
  float* sx = sx_all[wave];
  unsigned char* sv = sv_all[wave];
  float(*sg)[HT * PITCH] = sg_all[wave];
  // weight / C from the fold's result; no supervised centre (or weight 0): every centre term is exactly 0
  const float C = stats[2];
  const float lamC = (stats[1] > 0.f && C > 0.f) ? weight / C : 0.f;
  // every global load of the kernel is issued here, ahead of the first barrier: one round trip to memory, not three
  V3 q[CENTRE_PASSES];
  float w[CENTRE_PASSES], fTp[4];
#pragma unroll
  for (int it = 0; it < CENTRE_PASSES; it++) {
    const int i = lane + it * TGS_WAVE, cy = i / HT, cx = i - cy * HT;
    const int px = x0 - 1 + cx, py = y0 - 1 + cy;
    q[it] = v3(0.f, 0.f, 0.f);
    w[it] = 0.f;
    if (live && lamC != 0.f && prior) {   // (uniform; the position is clamped into the image, the value dropped outside it)
      const bool in = i < HT * HT && px >= 0 && px < c.W && py >= 0 && py < c.H;
      const size_t p = (size_t)min(max(py, 0), c.H - 1) * c.W + min(max(px, 0), c.W - 1);
      const V3 ql = dnorm_load_prior(prior, p);
      const float wl = conf ? conf[p] : 1.f;
      if (in) { q[it] = ql; w[it] = wl; }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int px = x0 + (lane & 15), py = y0 + dnorm_row(lane, k);
    fTp[k] = (live && px < c.W && py < c.H) ? final_T[(size_t)py * c.W + px] : 1.f;
  }
  if (live) dnorm_stage<2>(c, x0, y0, out_depth, final_T, alpha_min, sx, sv, lane);
  __syncthreads();
  if (live) {
#pragma unroll
    for (int it = 0; it < CENTRE_PASSES; it++) {
      const int i = lane + it * TGS_WAVE;
      if (i < HT * HT) {
        const int cy = i / HT, cx = i - cy * HT;
        const int px = x0 - 1 + cx, py = y0 - 1 + cy;
        float to_r = 0.f, to_l = 0.f, to_d = 0.f, to_u = 0.f;
        Centre ce;
        float pl;
        // (a centre outside the image is not valid; a pixel without a loaded prior has q = 0: not supervised)
        if (dnorm_prior(q[it], w[it], pl) && dnorm_centre(c, sx, sv, (cy + 1) * PITCH + cx + 1, px, py, max_jump, ce)) {
          const V3 gn = (-(lamC * w[it]) / pl) * q[it];
          const float d = dot(gn, ce.n);
          const V3 gm = (1.0f / ce.len) * (gn - d * ce.n);
          const V3 gtx = cross(gm, ce.ty), gty = cross(ce.tx, gm);
          const float rxc = dnorm_rx(c, px), ryc = dnorm_ry(c, py);
          to_r = dot(v3(dnorm_rx(c, px + 1), ryc, 1.f), gtx);
          to_l = -dot(v3(dnorm_rx(c, px - 1), ryc, 1.f), gtx);
          to_d = dot(v3(rxc, dnorm_ry(c, py + 1), 1.f), gty);
          to_u = -dot(v3(rxc, dnorm_ry(c, py - 1), 1.f), gty);
        }
        const int o = cy * PITCH + cx;
        sg[0][o] = to_r; sg[1][o] = to_l; sg[2][o] = to_d; sg[3][o] = to_u;
      }
    }
  }
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int row = dnorm_row(lane, k), col = lane & 15;
    const int px = x0 + col, py = y0 + row;
    if (px < c.W && py < c.H) {
      const size_t p = (size_t)py * c.W + px;
      // pixel (row, col) is centre (row + 1, col + 1) of the 18 x 18 grid: it is the right neighbour of its left centre, ...
      const int L = (row + 1) * PITCH + col, R = L + 2, U = row * PITCH + col + 1, D = U + 2 * PITCH;
      const float G = ((sg[0][L] + sg[1][R]) + sg[2][U]) + sg[3][D];
      float vd = 0.f, va = 0.f;
      if (G != 0.f) {   // (a pixel that feeds no supervised centre has G = +-0: exact zeros whatever x holds)
        const float alpha = fmaxf(1.0f - fTp[k], 1e-10f);
        const float x = sx[(row + 2) * PITCH + col + 2];
        const float ia = 1.0f / alpha;
        vd = G * ia;
        va = -(G * x) * ia;   // K7's convention: the gradient with respect to 1 - final_T
      }
      if (v_depth) v_depth[p] = ACC ? v_depth[p] + vd : vd;
      if (v_alpha) v_alpha[p] = ACC ? v_alpha[p] + va : va;
    }
  }
}

}  // namespace

extern "C" int tgs_depth_normal_fwd_bwd(const TgsCamera* cam, const float* out_depth, const float* final_T, const float* prior,
                                        const float* conf, float alpha_min, float max_jump, float weight, float* tile_sums,
                                        float* stats, float* normals, float* v_depth, float* v_alpha, int accumulate,
                                        void* stream) {
  TGS_CHECK_ARG(cam, "null camera");
  TGS_CHECK_ARG(cam->W >= 1 && cam->H >= 1, "bad image size");
  TGS_CHECK_ARG(cam->fx > 0.f && cam->fy > 0.f && isfinite(cam->fx) && isfinite(cam->fy) && isfinite(cam->cx) &&
                    isfinite(cam->cy) && isfinite(cam->pix_center),
                "bad intrinsics");
  TGS_CHECK_ARG(out_depth && final_T, "null image");
  TGS_CHECK_ARG(prior || !conf, "conf without a prior");
  TGS_CHECK_ARG(tile_sums && stats, "null tile_sums / stats");
  TGS_CHECK_ARG(alpha_min > 0.f && alpha_min <= 1.f, "alpha_min outside (0, 1]");
  TGS_CHECK_ARG(isfinite(max_jump), "max_jump not finite");
  TGS_CHECK_ARG(isfinite(weight), "weight not finite");
  TGS_CHECK_ARG(accumulate == 0 || accumulate == 1, "accumulate not 0 / 1");
  TGS_CHECK_ARG(((uintptr_t)tile_sums & 15) == 0 && ((uintptr_t)stats & 15) == 0, "tile_sums / stats not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  DnCam c;
  c.ifx = 1.0f / cam->fx; c.ify = 1.0f / cam->fy; c.cx = cam->cx; c.cy = cam->cy; c.pc = cam->pix_center; c.W = cam->W; c.H = cam->H;
  const int TW = (c.W + TGS_BLOCK - 1) / TGS_BLOCK, TH = (c.H + TGS_BLOCK - 1) / TGS_BLOCK;
  const int T = TW * TH;
  const dim3 grid((T + TILE_WAVES - 1) / TILE_WAVES), block(TILE_WAVES * TGS_WAVE);
  hipLaunchKernelGGL(k_dnorm_tiles, grid, block, 0, s, c, TW, T, out_depth, final_T, prior, conf, alpha_min, max_jump, tile_sums,
                     normals);
  TGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_dnorm_fold, dim3(1), dim3(FOLD_THREADS), 0, s, T, tile_sums, weight, stats);
  TGS_CHECK_LAUNCH();
  if (v_depth || v_alpha) {
    if (accumulate)
      hipLaunchKernelGGL(k_dnorm_grad<true>, grid, block, 0, s, c, TW, T, out_depth, final_T, prior, conf, alpha_min, max_jump,
                         weight, stats, v_depth, v_alpha);
    else
      hipLaunchKernelGGL(k_dnorm_grad<false>, grid, block, 0, s, c, TW, T, out_depth, final_T, prior, conf, alpha_min, max_jump,
                         weight, stats, v_depth, v_alpha);
    TGS_CHECK_LAUNCH();
  }
  return TGS_OK;
}
