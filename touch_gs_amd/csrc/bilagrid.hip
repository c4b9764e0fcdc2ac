// bilagrid.hip -- per-view bilateral grid g[GH][GW][L][12] of affine colour transforms [A | b] (row-major 3x4), sliced
// trilinearly by pixel position and by the luminance of the rendered colour: C' = A(p) C + b(p), an image-space op beside
// K6 / K7 (include/tgs.h, tgs_bilagrid_fwd / tgs_bilagrid_bwd).  The RGB loss is taken on C'; what goes to K7
// is v_rgb, K7's own fused L1 term is switched off (TgsLossSpec.gt_rgb NULL).  gfx950.
//
// Four launches:
//   k_bg_fwd   : one pixel per thread; the 8 corners are gathered from the grid (96 KB at the default shape: L2).
//   k_bg_cells : one workgroup per (xy-cell, chunk of BG_CHUNK pixels of the cell's pixel rectangle).  The cell's 2 x 2 x L x 12
//                block sits in LDS.  Reads rgb, gt, v_img, RECOMPUTES C' through bg_slice / bg_apply -- the functions the
//                forward calls -- forms v' = v_img + l1_weight sign(C' - gt), writes v_rgb (guide term included) and keeps
//                v', C and the cell coordinates of its BG_PX pixels in registers.  Then, level by level, it sums
//                w v' C1 and |w v' C1| for the 4 corners x 12 entries: per thread in pixel order, across the wave by DPP,
//                across the four waves through LDS in wave order.  One row of 4 L 24 + 8 floats per workgroup.
//   k_bg_fold  : one thread per grid entry sums the rows of its <= 4 adjacent cells and their chunks in fp64 in a fixed
//                order, writes grad, forms G + tv_weight dTV/dg from the grid AS IT IS (nothing is stepped in this launch:
//                dTV reads the six neighbours) into the scratch, and the TV value per block.
//   k_bg_step  : block 0 sums the L1 / count / TV partials in fp64 and writes out[]; every entry takes its adam1 step.
// No float atomics anywhere: the shape of every sum depends on (W, H, GW, GH, L) alone, the same inputs give the same bits.
//
// This translation unit is built with -ffp-contract=off (build.sh): the cell coordinates (bg_axis, bg_guide) decide which
// cell a pixel is in and must come out bit-identical in the forward, in the backward, which recomputes them, and in the
// fp32 NumPy evaluation of tests/bilagrid_ref.py; every product and sum therefore rounds on its own.
#include <math.h>
#include "tgs_adam.h"
#include "tgs_common.h"

namespace {

constexpr int BG_THREADS = 256;
constexpr int BG_PX = 4;                                  // pixels per thread of k_bg_cells
constexpr int BG_CHUNK = BG_THREADS * BG_PX;              // pixels per workgroup (touch_gs_amd/_lib.py BILAGRID_CHUNK)
constexpr int BG_WAVES = BG_THREADS / TGS_WAVE;
constexpr int BG_ACC = 96;                                // 4 corners x (G[12] | mass[12]) of one level
constexpr int BG_TAIL = 8;                                // sum |C' - gt| | pixels | 0...
constexpr int BG_MAX_L = 64, BG_MAX_G = 4096;
constexpr int BG_HDR = 4;                                 // t + 1, beta1^(t+1), beta2^(t+1), 0

struct BgDims {
  int W, H, GW, GH, L;
  float sx, sy, sz;   // float(GW-1) / float(W), float(GH-1) / float(H), float(L-1): formed once, on the host
};

// THE expression of a pixel's cell and fraction along x or y: p = pixel index, s = sx or sy, last = GW-2 or GH-2.
__host__ __device__ __forceinline__ void bg_axis(int p, float s, int last, int& i, float& f) {
  const float g = ((float)p + 0.5f) * s;
  const int t = (int)g;
  i = t < last ? t : last;
  f = g - (float)i;
}

// THE expression of the guide: level, fraction, and whether the luminance is strictly inside (0, 1).
__device__ __forceinline__ void bg_guide(float r, float g, float b, float sz, int last, int& iz, float& fz, bool& inside) {
  const float luma = (0.299f * r + 0.587f * g) + 0.114f * b;
  const float z = fminf(fmaxf(luma, 0.f), 1.f) * sz;
  const int t = (int)z;
  iz = t < last ? t : last;
  fz = z - (float)iz;
  inside = luma > 0.f && luma < 1.f;
}

// first pixel of [0, n] whose cell is >= c (the cell index is monotone in the pixel index); n where there is none
__host__ __device__ __forceinline__ int bg_first(int c, int n, float s, int last) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    int i; float f;
    bg_axis(mid, s, last, i, f);
    if (i >= c) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The slice in lerp form a + f (b - a): cXY = the 24 floats (levels iz, iz + 1) of the corner (ix + X, iy + Y).
// A0 / A1 = the xy-bilinear blends at the two levels, A = their blend along z.  An identity grid gives the identity.
__device__ __forceinline__ void bg_slice(const float* c00, const float* c10, const float* c01, const float* c11, float fx,
                                         float fy, float fz, float* A0, float* A1, float* A) {
#pragma unroll
  for (int e = 0; e < 24; e++) {
    const float a = c00[e] + fx * (c10[e] - c00[e]);
    const float b = c01[e] + fx * (c11[e] - c01[e]);
    const float v = a + fy * (b - a);
    if (e < 12) A0[e] = v; else A1[e - 12] = v;
  }
#pragma unroll
  for (int e = 0; e < 12; e++) A[e] = A0[e] + fz * (A1[e] - A0[e]);
}

// C'_c = ((A[c][0] r + A[c][1] g) + A[c][2] b) + A[c][3]: THE expression of the corrected colour, shared by both kernels.
__device__ __forceinline__ float bg_apply(const float* A, int c, float r, float g, float b) {
  return ((A[4 * c] * r + A[4 * c + 1] * g) + A[4 * c + 2] * b) + A[4 * c + 3];
}

__global__ __launch_bounds__(BG_THREADS) void k_bg_fwd(BgDims d, const float* __restrict__ rgb,
                                                       const float* __restrict__ grid, float* __restrict__ rgb_out) {
  const size_t p = (size_t)blockIdx.x * BG_THREADS + threadIdx.x;
  if (p >= (size_t)d.W * d.H) return;
  const int py = (int)(p / d.W), px = (int)(p - (size_t)py * d.W);
  const float r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2];
  int ix, iy, iz; float fx, fy, fz; bool inside;
  bg_axis(px, d.sx, d.GW - 2, ix, fx);
  bg_axis(py, d.sy, d.GH - 2, iy, fy);
  bg_guide(r, g, b, d.sz, d.L - 2, iz, fz, inside);
  const size_t vs = (size_t)d.L * 12;   // floats per grid vertex column
  const float* c00 = grid + ((size_t)iy * d.GW + ix) * vs + iz * 12;
  const float* c01 = c00 + (size_t)d.GW * vs;
  float A0[12], A1[12], A[12];
  bg_slice(c00, c00 + vs, c01, c01 + vs, fx, fy, fz, A0, A1, A);
#pragma unroll
  for (int c = 0; c < 3; c++) rgb_out[3 * p + c] = bg_apply(A, c, r, g, b);
}

// MASS: also sum |w v' C1| (asked for with `grad`; a train step, which only steps the row, leaves them out: half the sums)
template <bool HAS_GT, bool HAS_V, bool MASS>
__global__ __launch_bounds__(BG_THREADS) void k_bg_cells(BgDims d, int K, const float* __restrict__ rgb,
                                                         const float* __restrict__ grid, const float* __restrict__ gt,
                                                         float l1w, const float* __restrict__ v_img,
                                                         float* __restrict__ v_rgb, float* __restrict__ partials) {
  extern __shared__ float cellg[];                 // [4 corners][L][12]: corner = 2 dy + dx
  __shared__ float sm[BG_WAVES][BG_ACC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = d.L * BG_ACC + BG_TAIL;
  float* row = partials + (size_t)blockIdx.x * R;
  const int cell = blockIdx.x / K, k = blockIdx.x - cell * K;
  const int cy = cell / (d.GW - 1), cx = cell - cy * (d.GW - 1);
  // the cell's pixel rectangle, by the forward's own expression
  const int x0 = bg_first(cx, d.W, d.sx, d.GW - 2), x1 = bg_first(cx + 1, d.W, d.sx, d.GW - 2);
  const int y0 = bg_first(cy, d.H, d.sy, d.GH - 2), y1 = bg_first(cy + 1, d.H, d.sy, d.GH - 2);
  const int w = x1 - x0;
  const long long n = (long long)w * (y1 - y0), start = (long long)k * BG_CHUNK;
  if (start >= n) {   // (uniform) an empty cell, or a chunk behind the cell's last pixel: a row of zeros
    for (int i = tid; i < R; i += BG_THREADS) row[i] = 0.f;
    return;
  }
  const int vs = d.L * 12;
  for (int i = tid; i < 4 * vs; i += BG_THREADS) {
    const int corner = i / vs, e = i - corner * vs;
    cellg[i] = grid[((size_t)(cy + (corner >> 1)) * d.GW + cx + (corner & 1)) * vs + e];
  }
  __syncthreads();

  // per pixel, kept for the level loop: v'[3], C[3], the fractions, the level (-2 = no pixel: no level matches)
  float vp[BG_PX][3], col[BG_PX][3], fxs[BG_PX], fys[BG_PX], fzs[BG_PX];
  int izs[BG_PX];
  float s_l1 = 0.f, s_cnt = 0.f;
#pragma unroll
  for (int q = 0; q < BG_PX; q++) {
    const long long li = start + q * BG_THREADS + tid;
    izs[q] = -2;
    fxs[q] = fys[q] = fzs[q] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; c++) vp[q][c] = col[q][c] = 0.f;
    if (li >= n) continue;
    const int ly = (int)(li / w), lx = (int)(li - (long long)ly * w);
    const int px = x0 + lx, py = y0 + ly;
    const size_t p = (size_t)py * d.W + px;
    const float r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2];
    int ix, iy, iz; float fx, fy, fz; bool inside;
    bg_axis(px, d.sx, d.GW - 2, ix, fx);   // ix == cx, iy == cy: the rectangle was found with this expression
    bg_axis(py, d.sy, d.GH - 2, iy, fy);
    bg_guide(r, g, b, d.sz, d.L - 2, iz, fz, inside);
    float A0[12], A1[12], A[12];
    const float* c00 = cellg + iz * 12;
    bg_slice(c00, c00 + vs, c00 + 2 * vs, c00 + 3 * vs, fx, fy, fz, A0, A1, A);
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float t = HAS_V ? v_img[3 * p + c] : 0.f;
      if (HAS_GT) {
        const float dlt = bg_apply(A, c, r, g, b) - gt[3 * p + c];
        t += l1w * (float)((dlt > 0.f) - (dlt < 0.f));   // raster.hip pixel_upstream's expression: the product is exact
        s_l1 += fabsf(dlt);
      }
      v[c] = t;
    }
    s_cnt += 1.f;
    // the gradient through the guide: sum_c v'[c] ((A1 - A0) C1)[c], times (L - 1) where the clamp is not active
    float gz = 0.f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float dz = (((A1[4 * c] - A0[4 * c]) * r + (A1[4 * c + 1] - A0[4 * c + 1]) * g) + (A1[4 * c + 2] - A0[4 * c + 2]) * b) +
                       (A1[4 * c + 3] - A0[4 * c + 3]);
      gz += v[c] * dz;
    }
    gz = inside ? gz * d.sz : 0.f;
    const float wl[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
    for (int j = 0; j < 3; j++) v_rgb[3 * p + j] = ((A[j] * v[0] + A[4 + j] * v[1]) + A[8 + j] * v[2]) + wl[j] * gz;
    vp[q][0] = v[0]; vp[q][1] = v[1]; vp[q][2] = v[2];
    col[q][0] = r; col[q][1] = g; col[q][2] = b;
    fxs[q] = fx; fys[q] = fy; fzs[q] = fz; izs[q] = iz;
  }

  for (int l = 0; l < d.L; l++) {
    bool hit = false;
#pragma unroll
    for (int q = 0; q < BG_PX; q++) hit |= (izs[q] == l) | (izs[q] + 1 == l);
    if (__builtin_amdgcn_ballot_w64(hit) == 0) {
      // (wave-uniform) no lane of the wave has weight at this level: exact zeros, as the sums would give
      if (lane == 63)
        for (int j = 0; j < BG_ACC; j++) sm[wave][j] = 0.f;
    } else {
      float acc[BG_ACC];
#pragma unroll
      for (int j = 0; j < BG_ACC; j++) acc[j] = 0.f;
#pragma unroll
      for (int q = 0; q < BG_PX; q++) {
        // the trilinear weight along z at level l: (1 - fz, fz) at (iz, iz + 1), zero elsewhere
        const float wz = izs[q] == l ? 1.f - fzs[q] : (izs[q] + 1 == l ? fzs[q] : 0.f);
        const float wx[2] = {1.f - fxs[q], fxs[q]}, wy[2] = {1.f - fys[q], fys[q]};
        float w4[4];
#pragma unroll
        for (int cn = 0; cn < 4; cn++) w4[cn] = (wx[cn & 1] * wy[cn >> 1]) * wz;
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const float t = j < 3 ? vp[q][c] * col[q][j] : vp[q][c];
            const float a = fabsf(t);
#pragma unroll
            for (int cn = 0; cn < 4; cn++) {
              acc[cn * 24 + 4 * c + j] += w4[cn] * t;
              if (MASS) acc[cn * 24 + 12 + 4 * c + j] += w4[cn] * a;
            }
          }
      }
#pragma unroll
      for (int j = 0; j < BG_ACC; j++) {
        if (!MASS && j % 24 >= 12) {   // (compile-time per j) the masses of a launch that sums none are zeros
          if (lane == 63) sm[wave][j] = 0.f;
          continue;
        }
        const float t = wave_sum_to_lane63(acc[j]);
        if (lane == 63) sm[wave][j] = t;
      }
    }
    __syncthreads();
    if (tid < BG_ACC) {
      float t = sm[0][tid];
#pragma unroll
      for (int wv = 1; wv < BG_WAVES; wv++) t += sm[wv][tid];
      row[l * BG_ACC + tid] = t;
    }
    __syncthreads();
  }
  {
    const float a = wave_sum_to_lane63(s_l1), b = wave_sum_to_lane63(s_cnt);
    if (lane == 63) { sm[wave][0] = a; sm[wave][1] = b; }
    __syncthreads();
    if (tid < BG_TAIL) {
      float t = 0.f;
      if (tid < 2) {
        t = sm[0][tid];
#pragma unroll
        for (int wv = 1; wv < BG_WAVES; wv++) t += sm[wv][tid];
      }
      row[d.L * BG_ACC + tid] = t;
    }
  }
}

// fixed-order sum of one double per thread; the result in every thread.  (256 threads)
__device__ __forceinline__ double bg_block_sum(double v, double* smd) {
  const int tid = threadIdx.x;
  __syncthreads();
  smd[tid] = v;
  __syncthreads();
  for (int o = BG_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) smd[tid] += smd[tid + o];
    __syncthreads();
  }
  return smd[0];
}

__global__ __launch_bounds__(BG_THREADS) void k_bg_fold(BgDims d, int K, int n, const float* __restrict__ partials,
                                                        const float* __restrict__ grid, float tvw,
                                                        float* __restrict__ grad, float* __restrict__ gstep,
                                                        float* __restrict__ tvpart, float* __restrict__ hdr,
                                                        const int32_t* __restrict__ guard, const float* __restrict__ state,
                                                        float b1, float b2) {
  __shared__ double smd[BG_THREADS];
  if (guard && guard[1]) return;   // overflowed frame: k_bg_step zeroes out[], nothing else is written
  const int i = blockIdx.x * BG_THREADS + threadIdx.x;
  const int R = d.L * BG_ACC + BG_TAIL;
  double tv = 0.0;
  if (i < n) {
    const int v = i / 12, e = i - 12 * v;
    const int l = v % d.L, vx = (v / d.L) % d.GW, vy = v / (d.L * d.GW);
    double g = 0.0, m = 0.0;
    for (int dy = 0; dy < 2; dy++) {
      const int cy = vy - dy;
      if (cy < 0 || cy > d.GH - 2) continue;
      for (int dx = 0; dx < 2; dx++) {
        const int cx = vx - dx;
        if (cx < 0 || cx > d.GW - 2) continue;
        const float* r = partials + (size_t)(cy * (d.GW - 1) + cx) * K * R + (l * 4 + 2 * dy + dx) * 24 + e;
        for (int k = 0; k < K; k++) {
          g += (double)r[(size_t)k * R];
          if (grad) m += (double)r[(size_t)k * R + 12];
        }
      }
    }
    if (grad) { grad[i] = (float)g; grad[n + i] = (float)m; }
    // TV(g) = sum over the axes of (1 / n_axis) sum (g[next] - g[this])^2, n_axis = differences along the axis (12 channels)
    const double gi = (double)grid[i];
    const int str[3] = {d.L * 12, d.GW * d.L * 12, 12}, pos[3] = {vx, vy, l}, len[3] = {d.GW, d.GH, d.L};
    double tg = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double inv = 1.0 / ((double)(n / len[a]) * (double)(len[a] - 1));
      if (pos[a] > 0) tg += 2.0 * inv * (gi - (double)grid[i - str[a]]);
      if (pos[a] + 1 < len[a]) {
        const double df = (double)grid[i + str[a]] - gi;
        tg -= 2.0 * inv * df;
        tv += inv * df * df;
      }
    }
    gstep[i] = (float)(g + (double)tvw * tg);
  }
  tv = bg_block_sum(tv, smd);
  if (threadIdx.x == 0) tvpart[blockIdx.x] = (float)tv;
  if (state && blockIdx.x == 0 && threadIdx.x == 0) {
    // t and the running products beta^t live behind the row's 3 n entries; advanced HERE, into the scratch, so that no
    // thread of k_bg_step reads a word of the row another one writes
    hdr[0] = state[3 * (size_t)n] + 1.f;
    hdr[1] = state[3 * (size_t)n + 1] * b1;
    hdr[2] = state[3 * (size_t)n + 2] * b2;
    hdr[3] = 0.f;
  }
}

__global__ __launch_bounds__(BG_THREADS) void k_bg_step(int P, int R, int FB, int n, const float* __restrict__ partials,
                                                        const float* __restrict__ gstep, const float* __restrict__ tvpart,
                                                        const float* __restrict__ hdr, float l1w, float* __restrict__ out,
                                                        const int32_t* __restrict__ guard, float* __restrict__ state,
                                                        float lr, float b1, float b2, float eps) {
  __shared__ double smd[BG_THREADS];
  const int tid = threadIdx.x;
  if (guard && guard[1]) {   // overflowed frame: all zeros, the state row keeps every bit
    if (blockIdx.x == 0 && tid < TGS_BILAGRID_OUT) out[tid] = 0.f;
    return;
  }
  if (blockIdx.x == 0) {
    double l1 = 0.0, cnt = 0.0, tv = 0.0;
    for (int i = tid; i < P; i += BG_THREADS) {
      l1 += (double)partials[(size_t)i * R + R - BG_TAIL];
      cnt += (double)partials[(size_t)i * R + R - BG_TAIL + 1];
    }
    for (int i = tid; i < FB; i += BG_THREADS) tv += (double)tvpart[i];
    l1 = bg_block_sum(l1, smd);
    cnt = bg_block_sum(cnt, smd);
    tv = bg_block_sum(tv, smd);
    if (tid < TGS_BILAGRID_OUT)
      out[tid] = tid == 0 ? 1.f : tid == 1 ? (float)((double)l1w * l1) : tid == 2 ? (float)cnt : tid == 3 ? (float)tv : 0.f;
  }
  if (!state) return;   // (uniform)
  const int i = blockIdx.x * BG_THREADS + tid;
  if (i < n) {
    AdamK a = {};
    a.b1 = b1; a.b2 = b2; a.eps = eps; a.gscale = 1.f;
    a.ibc1 = 1.0f / (1.0f - hdr[1]);
    a.isq_bc2 = 1.0f / sqrtf(1.0f - hdr[2]);
    float p = state[i], m = state[(size_t)n + i], v = state[2 * (size_t)n + i];
    adam1(a, lr, p, gstep[i], m, v);
    state[i] = p; state[(size_t)n + i] = m; state[2 * (size_t)n + i] = v;
  }
  if (blockIdx.x == 0 && tid < 3) state[3 * (size_t)n + tid] = hdr[tid];
}

// Validated dimensions and the launch shape they alone decide.
struct BgShape {
  BgDims d;
  int n, K, P, R, FB;
  size_t scratch;   // floats: P rows of R | gstep[n] | tvpart[FB] | hdr[BG_HDR]
};

bool bg_dims_ok(int W, int H, int GW, int GH, int L) {
  return W >= 1 && H >= 1 && (long long)W * H <= (1ll << 30) && GW >= 2 && GH >= 2 && L >= 2 && GW <= BG_MAX_G &&
         GH <= BG_MAX_G && L <= BG_MAX_L && (long long)GW * GH * L * 12 <= (1ll << 28);
}

int bg_max_extent(int npx, int G, float s) {
  int best = 0, prev = 0;
  for (int c = 1; c <= G - 1; c++) {
    const int nx = bg_first(c, npx, s, G - 2);
    if (nx - prev > best) best = nx - prev;
    prev = nx;
  }
  return best;
}

BgShape bg_shape(int W, int H, int GW, int GH, int L) {
  BgShape s;
  s.d = {W, H, GW, GH, L, (float)(GW - 1) / (float)W, (float)(GH - 1) / (float)H, (float)(L - 1)};
  s.n = GW * GH * L * 12;
  const long long big = (long long)bg_max_extent(W, GW, s.d.sx) * bg_max_extent(H, GH, s.d.sy);   // pixels of the largest cell
  s.K = (int)((big + BG_CHUNK - 1) / BG_CHUNK);
  if (s.K < 1) s.K = 1;
  s.P = (GW - 1) * (GH - 1) * s.K;
  s.R = L * BG_ACC + BG_TAIL;
  s.FB = (s.n + BG_THREADS - 1) / BG_THREADS;
  s.scratch = (size_t)s.P * s.R + (size_t)s.n + s.FB + BG_HDR;
  return s;
}

template <bool HAS_GT, bool HAS_V>
void bg_launch_cells(const BgShape& s, hipStream_t st, const float* rgb, const float* grid, const float* gt, float l1w,
                     const float* v_img, float* v_rgb, float* partials, bool mass) {
  const size_t lds = (size_t)4 * s.d.L * 12 * sizeof(float);
  if (mass)
    hipLaunchKernelGGL((k_bg_cells<HAS_GT, HAS_V, true>), dim3((unsigned)s.P), dim3(BG_THREADS), lds, st, s.d, s.K, rgb, grid, gt,
                       l1w, v_img, v_rgb, partials);
  else
    hipLaunchKernelGGL((k_bg_cells<HAS_GT, HAS_V, false>), dim3((unsigned)s.P), dim3(BG_THREADS), lds, st, s.d, s.K, rgb, grid, gt,
                       l1w, v_img, v_rgb, partials);
}

}  // namespace

extern "C" int tgs_bilagrid_num_partials(int W, int H, int GW, int GH, int L) {
  return bg_dims_ok(W, H, GW, GH, L) ? bg_shape(W, H, GW, GH, L).P : 0;
}

extern "C" size_t tgs_bilagrid_row_floats(int L) { return L >= 2 && L <= BG_MAX_L ? (size_t)L * BG_ACC + BG_TAIL : 0; }

extern "C" size_t tgs_bilagrid_scratch_floats(int W, int H, int GW, int GH, int L) {
  return bg_dims_ok(W, H, GW, GH, L) ? bg_shape(W, H, GW, GH, L).scratch : 0;
}

extern "C" int tgs_bilagrid_fwd(int W, int H, int GW, int GH, int L, const float* rgb, const float* grid, float* rgb_out,
                                void* stream) {
  TGS_CHECK_ARG(bg_dims_ok(W, H, GW, GH, L), "bad image or grid size (W, H >= 1; 2 <= GW, GH <= 4096; 2 <= L <= 64)");
  TGS_CHECK_ARG(rgb && grid && rgb_out, "null rgb / grid / rgb_out");
  const BgShape s = bg_shape(W, H, GW, GH, L);
  const unsigned blocks = (unsigned)(((size_t)W * H + BG_THREADS - 1) / BG_THREADS);
  hipLaunchKernelGGL(k_bg_fwd, dim3(blocks), dim3(BG_THREADS), 0, (hipStream_t)stream, s.d, rgb, grid, rgb_out);
  TGS_CHECK_LAUNCH();
  return TGS_OK;
}

extern "C" int tgs_bilagrid_bwd(int W, int H, int GW, int GH, int L, const float* rgb, const float* grid, const float* gt,
                                float l1_weight, const float* v_img, float tv_weight, float* v_rgb, float* scratch,
                                float* grad, float* out, const int32_t* guard, float* state, float lr, float beta1,
                                float beta2, float eps, void* stream) {
  TGS_CHECK_ARG(bg_dims_ok(W, H, GW, GH, L), "bad image or grid size (W, H >= 1; 2 <= GW, GH <= 4096; 2 <= L <= 64)");
  TGS_CHECK_ARG(rgb && grid && v_rgb, "null rgb / grid / v_rgb");
  TGS_CHECK_ARG(scratch && out, "null scratch / out");
  TGS_CHECK_ARG(!state || (beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f), "beta outside [0, 1)");
  const BgShape s = bg_shape(W, H, GW, GH, L);
  hipStream_t st = (hipStream_t)stream;
  float* gstep = scratch + (size_t)s.P * s.R;
  float* tvpart = gstep + s.n;
  float* hdr = tvpart + s.FB;
  const bool mass = grad != nullptr;   // the masses are read by the fold only where it writes them
  if (gt && v_img) bg_launch_cells<true, true>(s, st, rgb, grid, gt, l1_weight, v_img, v_rgb, scratch, mass);
  else if (gt) bg_launch_cells<true, false>(s, st, rgb, grid, gt, l1_weight, v_img, v_rgb, scratch, mass);
  else if (v_img) bg_launch_cells<false, true>(s, st, rgb, grid, gt, l1_weight, v_img, v_rgb, scratch, mass);
  else bg_launch_cells<false, false>(s, st, rgb, grid, gt, l1_weight, v_img, v_rgb, scratch, mass);
  TGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_bg_fold, dim3((unsigned)s.FB), dim3(BG_THREADS), 0, st, s.d, s.K, s.n, scratch, grid, tv_weight, grad,
                     gstep, tvpart, hdr, guard, state, beta1, beta2);
  TGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_bg_step, dim3((unsigned)s.FB), dim3(BG_THREADS), 0, st, s.P, s.R, s.FB, s.n, scratch, gstep, tvpart, hdr,
                     gt ? l1_weight : 0.f, out, guard, state, lr, beta1, beta2, eps);
  TGS_CHECK_LAUNCH();
  return TGS_OK;
}
