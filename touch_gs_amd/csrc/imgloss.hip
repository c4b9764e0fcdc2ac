// imgloss.hip -- K10 SSIM forward + gradient image (11x11 Gaussian window, sigma 1.5, zero
// padding), the (1-SSIM) term of the Splatfacto-style loss (1-l)*L1 + l*(1-SSIM) that the
// reference's `depth-gaussian-splatting` method trains with.  gfx950.
//
// Two separable-convolution kernels, row streaming:
//   k_ssim_fwd : 5 windowed moments -> SSIM map; writes the three adjoint maps
//                A = dm/dmu1 (total), B = dm/dE[x^2], C = dm/dE[xy] and a per-workgroup sum of the map
//   k_ssim_bwd : v_img = weight * (G*A + 2*img*(G*B) + gt*(G*C))
// A workgroup owns a strip of 64 columns x SEG rows, thread = (column, channel).  Input rows are
// staged 11 at a time in LDS exactly as they lie in memory (interleaved channels: coalesced loads,
// conflict-free ds_read with lane stride 1 / 3); every thread filters its row horizontally from LDS
// (11 taps) and keeps the last 11 horizontally-filtered rows in REGISTERS, so the vertical pass
// costs no LDS traffic and no barrier -- the first version staged 26x26 halo tiles per 16x16
// outputs (2.6x read amplification, 48 KB of LDS per workgroup, 3 workgroups per CU, 39-44 % LDS
// bank-conflict cycles; 77 + 80 us at 1080p).  Read amplification here: 74/64 horizontally,
// (SEG+10)/SEG vertically.  Roofline: HBM (9 adjoint planes written, then read).
// From 1080p on a gradient call runs k_ssim_fused instead (below): both filters in one pass over the same strips, the adjoint
// values in a two-row LDS ring instead of HBM.  The filter arithmetic of all three kernels is the shared device functions
// below (one copy of each body), which is what keeps every output bit-identical between them (ssim_impl).
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include "tgs_common.h"

namespace {

constexpr int WIN = 11, HALO = 5;
// The window weights as compile-time constants (11-tap Gaussian, sigma 1.5, normalised in double and rounded
// to fp32).  As kernel arguments they would sit in SGPRs, and on gfx950 a VALU instruction with an SGPR source
// is the most expensive form there is (v_mul / v_add 5.45 cycles, v_fma 4.5 - 5.5, against 2.8 - 3.0 with a
// literal: tools/ubench/valu_cost.hip) -- every FMA of the two filters is of that kind.
__device__ constexpr float WGT[WIN] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f,
                                       0x1.10656p-2f, 0x1.b43c4p-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f,
                                       0x1.0d956cp-10f};

constexpr int SW = 64;              // strip width (output columns per workgroup)
constexpr int NTH = 3 * SW;         // threads: (column, channel)
constexpr int RB = WIN;             // input rows per staged block = window height (phase p = row in block)
// blocks per segment (nblk, a launch argument): SEG = 11 nblk - 10 output rows per workgroup.  4 (34 rows)
// at 1080p and above; small images take shorter segments -- the kernels are latency chains over the
// blocks of a segment, and an 800x800 image has only 312 segments of 34 rows for 256 CUs.
__host__ __device__ constexpr int seg_rows(int nblk) { return RB * nblk - 2 * HALO; }

// Loads in flight per thread and staging round:
constexpr int FWD_B = 13;   // all 13 + 13 loads of a block in flight at once (round 5: 128 VGPRs, still 4 waves per SIMD); 7 = two rounds
constexpr int BWD_B = 20;   // two rounds of 20 instead of three of 13 (66 VGPRs); all 39 at once spills.  Both: 99.4 -> 97.7 us (r5_ab_runs.txt)

// Stages input rows [r0, r0 + RB) x columns [x0 - 5, x0 + SW + 5) of an interleaved [H, W, CH]
// image into LDS (zero outside the image), in rounds of B loads in flight per thread.
// stage and stage2 are one loop for one and for two images; as one template over the image count the forward kernel
// spilled 26 registers and the backward kernel's register and VALU counts moved (profiles/ssim_shared_isa.txt).
template <int CH>
struct RowBlock {
  static constexpr int ROWF = (SW + 2 * HALO) * CH;             // floats per staged row
  static constexpr int NIT = (RB * ROWF + NTH - 1) / NTH;
  template <int B>
  static __device__ __forceinline__ void stage(const float* __restrict__ src, float* __restrict__ lds,
                                               int W, int H, int x0, int r0, int tid) {
#pragma unroll 1
    for (int it0 = 0; it0 < NIT; it0 += B) {
      float v[B];
#pragma unroll
      for (int u = 0; u < B; u++) {
        const int i = tid + NTH * (it0 + u);
        const int j = i / ROWF, e = i - j * ROWF;
        const int gy = r0 + j, gxf = (x0 - HALO) * CH + e;
        v[u] = 0.f;
        if (i < RB * ROWF && gy >= 0 && gy < H && gxf >= 0 && gxf < W * CH) v[u] = src[(size_t)gy * W * CH + gxf];
      }
#pragma unroll
      for (int u = 0; u < B; u++) {
        const int i = tid + NTH * (it0 + u);
        if (i < RB * ROWF) lds[i] = v[u];
      }
    }
  }
  // Two images of the same geometry in one pass: the loads of both are in flight together, which halves
  // the number of load -> wait round trips per block (the forward kernel is a chain of them; staging them one after
  // the other in rounds of 8: forward + backward 118 -> 111 us at 1080p, same box).
  template <int B>
  static __device__ __forceinline__ void stage2(const float* __restrict__ src_a, const float* __restrict__ src_b,
                                                float* __restrict__ lds_a, float* __restrict__ lds_b,
                                                int W, int H, int x0, int r0, int tid) {
#pragma unroll 1
    for (int it0 = 0; it0 < NIT; it0 += B) {
      float va[B], vb[B];
#pragma unroll
      for (int u = 0; u < B; u++) {
        const int i = tid + NTH * (it0 + u);
        const int j = i / ROWF, e = i - j * ROWF;
        const int gy = r0 + j, gxf = (x0 - HALO) * CH + e;
        va[u] = 0.f; vb[u] = 0.f;
        if (it0 + u < NIT && i < RB * ROWF && gy >= 0 && gy < H && gxf >= 0 && gxf < W * CH) {
          const size_t o = (size_t)gy * W * CH + gxf;
          va[u] = src_a[o]; vb[u] = src_b[o];
        }
      }
#pragma unroll
      for (int u = 0; u < B; u++) {
        const int i = tid + NTH * (it0 + u);
        if (it0 + u < NIT && i < RB * ROWF) { lds_a[i] = va[u]; lds_b[i] = vb[u]; }
      }
    }
  }
};

// ---------------------------------------------------------------------------------------------
// The filter bodies: one copy each, used by k_ssim_fwd, k_ssim_bwd and k_ssim_fused
// ---------------------------------------------------------------------------------------------
// No floating-point operation here may change its order or its contraction: v_img is bit-identical between the
// two-kernel path and the one-pass kernel, and block_partials between forms 0 and 2 (tests/test_gpu_ssim_one_pass.py).

// Horizontal pass of one staged row of img (ra) and gt (rb) for this thread's (column, channel): the five moments.
__device__ __forceinline__ void moments_row(const float* ra, const float* rb, float (&w)[5]) {
  float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
  for (int k = 0; k < WIN; k++) {
    const float a = ra[3 * k], b = rb[3 * k];
    const float ga = WGT[k] * a, gb = WGT[k] * b;
    m1 += ga; m2 += gb;
    e11 = fmaf(ga, a, e11); e22 = fmaf(gb, b, e22); e12 = fmaf(ga, b, e12);
  }
  w[0] = m1; w[1] = m2; w[2] = e11; w[3] = e22; w[4] = e12;
}

// Horizontal pass of one adjoint row ([column][channel][3 maps]) for this thread's (column, channel).
__device__ __forceinline__ void adjoint_row(const float* r, float (&w)[3]) {
  float h0 = 0.f, h1 = 0.f, h2 = 0.f;
#pragma unroll
  for (int k = 0; k < WIN; k++) {
    h0 = fmaf(WGT[k], r[9 * k], h0);
    h1 = fmaf(WGT[k], r[9 * k + 1], h1);
    h2 = fmaf(WGT[k], r[9 * k + 2], h2);
  }
  w[0] = h0; w[1] = h1; w[2] = h2;
}

// Vertical pass over the register window after row p of a block went in: slots (p+1 .. p+11) mod 11 = oldest .. newest.
template <int Q>
__device__ __forceinline__ void vertical(const float (&w)[RB][Q], int p, float (&o)[Q]) {
#pragma unroll
  for (int q = 0; q < Q; q++) o[q] = 0.f;
#pragma unroll
  for (int k = 0; k < WIN; k++) {
#pragma unroll
    for (int q = 0; q < Q; q++) o[q] = fmaf(WGT[k], w[(p + 1 + k) % RB][q], o[q]);
  }
}

// The SSIM value m of one (pixel, channel) from its five filtered moments, with what the adjoint needs of it.
struct SsimPoint { float m, mu1, mu2, n1, n2, id1, id2; };
__device__ __forceinline__ SsimPoint ssim_point(const float (&o)[5]) {
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  const float mu1 = o[0], mu2 = o[1];
  const float s11 = o[2] - mu1 * mu1, s22 = o[3] - mu2 * mu2, s12 = o[4] - mu1 * mu2;
  const float n1 = 2.f * mu1 * mu2 + C1, n2 = 2.f * s12 + C2;
  const float d1 = mu1 * mu1 + mu2 * mu2 + C1, d2 = s11 + s22 + C2;
  // v_rcp_f32 (1 ulp) instead of the ~10-instruction IEEE division: d1, d2 >= C1, C2 > 0
  const float id1 = __builtin_amdgcn_rcpf(d1), id2 = __builtin_amdgcn_rcpf(d2);
  return {n1 * n2 * id1 * id2, mu1, mu2, n1, n2, id1, id2};
}

// A = dm/dmu1 (total), B = dm/dE[x^2], C = dm/dE[xy].  Apart from ssim_point: a forward-only call does not pay for it.
__device__ __forceinline__ void ssim_adjoint(const SsimPoint& s, float& A, float& B, float& C) {
  const float dm_ds12 = 2.f * s.n1 * s.id1 * s.id2;
  const float dm_ds11 = -s.m * s.id2;
  const float dm_dmu1 = 2.f * s.mu2 * s.n2 * s.id1 * s.id2 - s.m * 2.f * s.mu1 * s.id1;
  A = dm_dmu1 - 2.f * s.mu1 * dm_ds11 - s.mu2 * dm_ds12;
  B = dm_ds11;
  C = dm_ds12;
}

// v_img of one (pixel, channel) from its three filtered adjoint maps; x = img, y = gt there.
__device__ __forceinline__ float grad_value(float weight, const float (&o)[3], float x, float y) {
  return weight * (o[0] + 2.f * x * o[1] + y * o[2]);
}

// Workgroup sum of the map -> block_partials[workgroup]; the caller's buffer has one entry per 16x16 tile: the entries
// beyond the workgroup count are zeroed.  Three waves hold the sums (the fourth wave of k_ssim_fused holds no output column).
template <int NT>
__device__ __forceinline__ void store_block_sum(float v, float* __restrict__ block_partials, int n_partials, int tid) {
  __shared__ float red[NT / TGS_WAVE];
  const float tot = wave_sum(v);
  if ((tid & 63) == 0) red[tid >> 6] = tot;
  __syncthreads();
  const int wg = blockIdx.y * gridDim.x + blockIdx.x, nwg = gridDim.x * gridDim.y;
  if (tid == 0) block_partials[wg] = red[0] + red[1] + red[2];
  for (int i = nwg + wg * NT + tid; i < n_partials; i += nwg * NT) block_partials[i] = 0.f;
}

__global__ __launch_bounds__(NTH) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_ssim_fwd(int W, int H,
                                                  const float* __restrict__ img,
                                                  const float* __restrict__ gt,
                                                  float* __restrict__ adj /*[H,W,3,3] or null*/,
                                                  float* __restrict__ block_partials, int n_partials, int NBLK,
                                                  int y_lo, int y_hi, int c_lo, int c_hi) {
  // rows [y_lo, y_hi) of the map / adjoint maps are produced (the whole image, or one band of it plus the
  // 5-row halo its backward pass needs); rows [c_lo, c_hi) count towards the sum
  const int SEG = seg_rows(NBLK);
  constexpr int ROWF = RowBlock<3>::ROWF;
  __shared__ float sa[RB * ROWF], sb[RB * ROWF];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * SW, ys = y_lo + blockIdx.y * SEG;
  const int gx = x0 + tid / 3, c = tid - (tid / 3) * 3;
  const int ye = min(ys + SEG, y_hi);
  float w[RB][5];
#pragma unroll
  for (int p = 0; p < RB; p++)
#pragma unroll
    for (int q = 0; q < 5; q++) w[p][q] = 0.f;
  float msum = 0.f;
  for (int blk = 0; blk < NBLK; blk++) {
    const int r0 = ys - HALO + blk * RB;          // first input row of this block
    if (r0 - HALO >= ye) break;                   // no output row left (uniform)
    __syncthreads();                              // previous block fully consumed
    // no register prefetch of the next block: the window already holds 55 VGPRs per thread and
    // the other resident workgroups of the CU cover the load latency
    RowBlock<3>::stage2<FWD_B>(img, gt, sa, sb, W, H, x0, r0, tid);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < RB; p++) {
      moments_row(sa + p * ROWF + tid, sb + p * ROWF + tid, w[p]);     // input row r0 + p
      const int gy = r0 + p - HALO;               // output row
      if (gy >= ys && gy < ye) {                  // uniform
        float o[5];
        vertical(w, p, o);
        const SsimPoint s = ssim_point(o);
        if (gx < W) {
          if (gy >= c_lo && gy < c_hi) msum += s.m;
          if (adj) {
            float* o3 = adj + (((size_t)gy * W + gx) * 3 + c) * 3;
            ssim_adjoint(s, o3[0], o3[1], o3[2]);
          }
        }
      }
    }
  }
  store_block_sum<NTH>(msum, block_partials, n_partials, tid);
}

__global__ __launch_bounds__(NTH) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_ssim_bwd(int W, int H, float weight,
                                                  const float* __restrict__ img,
                                                  const float* __restrict__ gt,
                                                  const float* __restrict__ adj,
                                                  float* __restrict__ v_img, int NBLK, int y_lo, int y_hi) {
  const int SEG = seg_rows(NBLK);
  constexpr int ROWF = RowBlock<9>::ROWF;
  __shared__ float sadj[RB * ROWF];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * SW, ys = y_lo + blockIdx.y * SEG;
  const int gx = x0 + tid / 3;
  const int ye = min(ys + SEG, y_hi);
  float w[RB][3];
#pragma unroll
  for (int p = 0; p < RB; p++) { w[p][0] = 0.f; w[p][1] = 0.f; w[p][2] = 0.f; }
  for (int blk = 0; blk < NBLK; blk++) {
    const int r0 = ys - HALO + blk * RB;
    if (r0 - HALO >= ye) break;
    __syncthreads();
    RowBlock<9>::stage<BWD_B>(adj, sadj, W, H, x0, r0, tid);      // 38 loads per thread and block
    __syncthreads();
#pragma unroll
    for (int p = 0; p < RB; p++) {
      adjoint_row(sadj + p * ROWF + 3 * tid, w[p]);   // (pixel, channel) -> its three adjoint maps
      const int gy = r0 + p - HALO;
      if (gy >= ys && gy < ye) {
        float o[3];
        vertical(w, p, o);
        if (gx < W) {
          const size_t pidx = (size_t)gy * W * 3 + (size_t)x0 * 3 + tid;
          v_img[pidx] = grad_value(weight, o, img[pidx], gt[pidx]);
        }
      }
    }
  }
}


// ---------------------------------------------------------------------------------------------
// One pass: forward + backward of a strip without the adjoint planes in HBM
// ---------------------------------------------------------------------------------------------
// k_ssim_fwd writes nine adjoint values per pixel (75 MB at 1080p) that k_ssim_bwd reads back with its own halo
// (x 1.5): 351 MB of HBM traffic for 75 MB of compulsory bytes (img, gt in; v_img out), 10 % of the train step.
// Here a workgroup owns SWO output columns x SEG rows and keeps everything between the two filters on chip.  Its 256
// threads are (column, channel) pairs: the first 3 (SWO + 10) of them run phase 1 on the strip's adjoint columns
// [x0 - 5, x0 + SWO + 5), the first 3 SWO run phase 2 on its output columns.  Per staged input row r (11 to a block):
//   phase 1  = k_ssim_fwd's loop body, the shared functions: horizontal moments from LDS, the last 11 rows in registers,
//              SSIM map + the three adjoint values of (row r - 5, own column) -> LDS (zero outside the image: the
//              backward filter's zero padding);
//   barrier
//   phase 2  = k_ssim_bwd's loop body, the shared functions, on that ONE adjoint row: horizontal filter of the three
//              adjoint maps from LDS, the last 11 rows in registers, v_img of row r - 10.
// The backward's vertical window lives in registers, so only the row in flight has to be in LDS: a ring of two rows
// (phase 1 fills one while slower waves still read the other; one barrier per row) in place of the 11 rows x 64 x 9
// floats of the first one-pass kernel -- 27 KB of LDS instead of 45, 4 waves per SIMD instead of 2.
// Same arithmetic in the same order per value: v_img is bit-identical to the two-kernel path.  The map sum is too when
// the strips lie on the two-kernel path's grid (SWO = 64, segments of seg_rows(nblk) rows from the forward launch's
// first row): every map value is added by the thread index, in the row order and to the workgroup slot k_ssim_fwd
// adds it in (a thread of phase 1 sums its adjoint column; the sums move 15 threads down through LDS before the
// wave reduction).  Costs: phase 1 runs on (SWO + 10) / SWO x (SEG + 10) / SEG more pixels, img / gt are read with a
// 10-pixel halo, and with SWO = 64 the fourth wave has 30 lanes of phase 1 and nothing of phase 2.
constexpr int FT = 256;             // threads of the one-pass kernel
constexpr int SWO_OWN = SW - 2 * HALO;   // TGS_SSIM_FUSED=1: 54-column strips on the kernel's own grid
__host__ __device__ constexpr int fused_seg_rows(int nblk) { return RB * nblk - 4 * HALO; }

template <int SWO>
__global__ __launch_bounds__(FT) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_ssim_fused(
    int W, int H, float weight, const float* __restrict__ img, const float* __restrict__ gt,
    float* __restrict__ v_img, float* __restrict__ block_partials, int n_partials, int SEG,
    int y_base, int y_lo, int y_hi, int c_lo, int c_hi) {
  // segment by of the grid that starts at row y_base owns the output rows [ys, ye) it shares with [y_lo, y_hi)
  constexpr int NCA = SWO + 2 * HALO;                // adjoint columns of a strip
  constexpr int NT1 = 3 * NCA, NT2 = 3 * SWO;        // threads of phase 1 / phase 2
  constexpr int ROWF = (NCA + 2 * HALO) * 3;         // floats per staged input row: one per thread
  constexpr int ADJF = NCA * 9;                      // floats per adjoint row: [column][channel][3 maps]
  constexpr int SB = 6;                              // rows per staging round: 6 + 6 loads in flight beside the two windows
  static_assert(ROWF <= FT && NT1 <= FT && FT <= RB * ROWF, "one staged float, one adjoint (column, channel) per thread");
  __shared__ float sa[RB * ROWF], sb[RB * ROWF];
  __shared__ float sadj[2 * ADJF];
  const int tid = threadIdx.x;
  const unsigned ut = tid;                           // index of a global access: uniform base + 32-bit lane offset
  const int col = tid / 3;
  const int x0 = blockIdx.x * SWO;                   // first output column
  // phase 1: this thread's adjoint column is x0 - 5 + col; phase 2: its output column is x0 + col (bounds kept uniform)
  const bool own_col = col >= HALO && col < HALO + SWO;
  const bool adj_in = col >= HALO - x0 && col < W + HALO - x0;
  const bool out_in = tid < NT2 && col < W - x0;
  const int yseg = y_base + blockIdx.y * SEG;
  const int ys = max(yseg, y_lo), ye = min(yseg + SEG, y_hi);
  const int xf0 = (x0 - 2 * HALO) * 3;               // staging: thread tid brings float xf0 + tid of an interleaved image row
  const bool stage_x = tid < ROWF && tid >= -xf0 && tid < W * 3 - xf0;
  float w[RB][5], w2[RB][3];
#pragma unroll
  for (int p = 0; p < RB; p++) {
#pragma unroll
    for (int q = 0; q < 5; q++) w[p][q] = 0.f;
    w2[p][0] = 0.f; w2[p][1] = 0.f; w2[p][2] = 0.f;
  }
  float msum = 0.f;
  for (int r0 = ys - 2 * HALO; r0 - 2 * HALO < ye; r0 += RB) {   // r0 = first input row of the block; its output rows are r0 - 10 ..
    __syncthreads();                                 // previous block fully consumed (sa / sb, and sadj[0] by its last row)
#pragma unroll 1
    for (int j0 = 0; j0 < RB; j0 += SB) {
      float va[SB], vb[SB];
#pragma unroll
      for (int u = 0; u < SB; u++) {
        const int gy = r0 + j0 + u;
        va[u] = 0.f; vb[u] = 0.f;
        if (j0 + u < RB && stage_x && gy >= 0 && gy < H) {
          const ptrdiff_t o = (ptrdiff_t)gy * W * 3 + xf0;      // uniform
          va[u] = (img + o)[ut]; vb[u] = (gt + o)[ut];
        }
      }
#pragma unroll
      for (int u = 0; u < SB; u++)
        if (j0 + u < RB && tid < ROWF) { sa[(j0 + u) * ROWF + tid] = va[u]; sb[(j0 + u) * ROWF + tid] = vb[u]; }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < RB; p++) {
      const int gyo = r0 + p - 2 * HALO;              // phase 2: output row
      // ---- phase 1: moments -> SSIM map -> adjoint values of row r0 + p - 5 at column gxa
      if (tid < NT1) {
        moments_row(sa + p * ROWF + tid, sb + p * ROWF + tid, w[p]);
        const int gy = r0 + p - HALO;                // map / adjoint row
        float A = 0.f, B = 0.f, C = 0.f;
        if (gy >= ys - HALO && gy < ye + HALO && gy >= 0 && gy < H) {      // uniform
          float o[5];
          vertical(w, p, o);
          const SsimPoint s = ssim_point(o);
          if (adj_in) {
            if (own_col && gy >= ys && gy < ye && gy >= c_lo && gy < c_hi) msum += s.m;
            ssim_adjoint(s, A, B, C);
          }
        }
        float* o3 = sadj + (p & 1) * ADJF + tid * 3;
        o3[0] = A; o3[1] = B; o3[2] = C;
      }
      __syncthreads();                               // the row is in LDS; every wave is done with the row before the last
      // ---- phase 2: filtered adjoint maps -> v_img of row r0 + p - 10 at column gxo (adjoint columns col .. col + 10)
      if (tid < NT2) {
        adjoint_row(sadj + (p & 1) * ADJF + tid * 3, w2[p]);
        if (gyo >= ys && gyo < ye) {                 // uniform
          float o[3];
          vertical(w2, p, o);
          if (out_in) {
            const ptrdiff_t orow = (ptrdiff_t)gyo * W * 3 + (ptrdiff_t)x0 * 3;     // uniform
            (v_img + orow)[ut] = grad_value(weight, o, (img + orow)[ut], (gt + orow)[ut]);
          }
        }
      }
    }
  }
  // the sum of adjoint column col + 5 = output column col goes to the thread that owns that output column in k_ssim_fwd
  __syncthreads();
  sa[tid] = msum;
  __syncthreads();
  store_block_sum<FT>(tid < NT2 ? sa[tid + 3 * HALO] : 0.f, block_partials, n_partials, tid);
}

// No forward row to produce (an empty band): nothing counts, but the caller still sums block_partials.  A kernel rather
// than hipMemsetAsync, as in tgs_binning.h: an ordinary node when the step is captured into a hipGraph.
__global__ void k_ssim_zero_partials(float* __restrict__ block_partials, int n_partials) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_partials) block_partials[i] = 0.f;
}

}  // namespace

// the one-pass kernel counts a map pixel in the workgroup that owns its output row: the counted rows must be output rows
static inline bool count_inside(int y0, int y1, int c0, int c1) { return c0 >= c1 || (c0 >= y0 && c1 <= y1); }

// Which kernels a gradient call runs (tgs_set_ssim_form; environment TGS_SSIM_FUSED, read once at first use):
//   0  k_ssim_fwd + k_ssim_bwd, the adjoint planes in `scratch`
//   1  one pass on the kernel's own grid: 54-column strips, segments of 11 nblk - 20 rows from y0
//   2  one pass on the two-kernel path's grid (64-column strips, the forward launch's segments): the same block_partials,
//      bit for bit
//   3  (default) 2 where it is the faster one, 0 elsewhere
enum { SSIM_TWO_KERNELS = 0, SSIM_ONE_PASS_OWN_GRID = 1, SSIM_ONE_PASS = 2, SSIM_AUTO = 3 };
static TgsDefault g_ssim_form{"TGS_SSIM_FUSED", SSIM_AUTO, false, SSIM_AUTO};
// SSIM_AUTO: the one-pass kernel from this many pixels on (1080p; see DESIGN 5.4 for the sizes below it)
constexpr long long SSIM_ONE_PASS_MIN_PIXELS = 1920LL * 1080;

static int ssim_impl(int W, int H, const float* img, const float* gt, float weight,
                     float* block_partials, int n_partials, float* v_img, float* scratch,
                     int y0, int y1, int c0, int c1, void* stream) {
  TGS_CHECK_ARG(W > 0 && H > 0, "bad image size");
  TGS_CHECK_ARG(img && gt && block_partials, "null pointer");
  TGS_CHECK_ARG(!v_img || scratch, "gradient needs scratch");
  TGS_CHECK_ARG(0 <= y0 && y0 <= y1 && y1 <= H && y0 <= c0 && c0 <= c1 && c1 <= y1, "bad row range");
  static const int env_nblk = [] { const char* e = getenv("TGS_SSIM_NBLK"); return e ? max(2, min(16, atoi(e))) : 0; }();
  int form = g_ssim_form.get();
  if (form == SSIM_AUTO) form = (long long)W * H >= SSIM_ONE_PASS_MIN_PIXELS ? SSIM_ONE_PASS : SSIM_TWO_KERNELS;
  const bool one_pass = v_img && y1 > y0 && count_inside(y0, y1, c0, c1);
  if (one_pass && form == SSIM_ONE_PASS_OWN_GRID) {
    // `scratch` is not touched.  Strip = 54 columns x (11 nblk - 20) rows: long segments keep the vertical halo small
    // ((SEG + 20) / SEG input rows, (SEG + 10) / SEG of the forward arithmetic); the longest segment that still gives
    // 600 workgroups is taken
    const int fx = (W + SWO_OWN - 1) / SWO_OWN;
    auto wgs = [&](int nb) { return (long long)fx * ((y1 - y0 + fused_seg_rows(nb) - 1) / fused_seg_rows(nb)); };
    int nblk = 7;
    while (nblk > 3 && wgs(nblk) < 600) nblk--;
    if (env_nblk) nblk = max(3, env_nblk);
    while (nblk < 16 && wgs(nblk) > n_partials) nblk++;
    TGS_CHECK_ARG(wgs(nblk) <= n_partials, "block_partials too small");
    const int SEGF = fused_seg_rows(nblk);
    hipLaunchKernelGGL(k_ssim_fused<SWO_OWN>, dim3(fx, (y1 - y0 + SEGF - 1) / SEGF, 1), dim3(FT), 0, (hipStream_t)stream, W, H,
                       weight, img, gt, v_img, block_partials, n_partials, SEGF, y0, y0, y1, c0, c1);
    TGS_CHECK_LAUNCH();
    return TGS_OK;
  }
  // forward rows: the gradient rows plus the 5-row halo the backward filter reads (adjoint maps)
  const int f0 = v_img ? max(0, y0 - HALO) : y0, f1 = v_img ? min(H, y1 + HALO) : y1;
  const int rows = f1 - f0;
  if (rows <= 0) {
    // the contract of include/tgs.h holds for an empty band too: workgroup sums (none), the rest zero
    if (n_partials > 0) {
      hipLaunchKernelGGL(k_ssim_zero_partials, dim3((n_partials + 255) / 256), dim3(256), 0, (hipStream_t)stream, block_partials,
                         n_partials);
      TGS_CHECK_LAUNCH();
    }
    return TGS_OK;
  }
  const int sx = (W + SW - 1) / SW;
  auto wgs = [&](int nb) { return (long long)sx * ((rows + seg_rows(nb) - 1) / seg_rows(nb)); };
  int nblk = 4;
  while (nblk > 2 && wgs(nblk) < 3 * 256) nblk--;
  if (env_nblk) nblk = env_nblk;   // tuning override (read once, above)
  // one workgroup sum goes into each of the first entries of block_partials, the rest is zeroed
  while (nblk < 16 && wgs(nblk) > n_partials) nblk++;
  TGS_CHECK_ARG(wgs(nblk) <= n_partials, "block_partials too small");
  const int SEG = seg_rows(nblk);
  const dim3 block(NTH);
  hipStream_t s = (hipStream_t)stream;
  if (one_pass && form == SSIM_ONE_PASS) {
    // the forward launch's grid: a workgroup writes the rows of its segment that lie in [y0, y1) and the sum k_ssim_fwd's
    // workgroup of the same index would
    hipLaunchKernelGGL(k_ssim_fused<SW>, dim3(sx, (rows + SEG - 1) / SEG, 1), dim3(FT), 0, s, W, H, weight, img, gt, v_img,
                       block_partials, n_partials, SEG, f0, y0, y1, c0, c1);
    TGS_CHECK_LAUNCH();
    return TGS_OK;
  }
  hipLaunchKernelGGL(k_ssim_fwd, dim3(sx, (rows + SEG - 1) / SEG, 1), block, 0, s, W, H, img, gt,
                     v_img ? scratch : nullptr, block_partials, n_partials, nblk, f0, f1, c0, c1);
  TGS_CHECK_LAUNCH();
  if (v_img && y1 > y0) {
    hipLaunchKernelGGL(k_ssim_bwd, dim3(sx, (y1 - y0 + SEG - 1) / SEG, 1), block, 0, s, W, H, weight, img, gt,
                       scratch, v_img, nblk, y0, y1);
    TGS_CHECK_LAUNCH();
  }
  return TGS_OK;
}

extern "C" int tgs_ssim_fwd_bwd(int W, int H, const float* img, const float* gt, float weight,
                                float* block_partials, float* v_img, float* scratch,
                                void* stream) {
  // block_partials has one entry per 16x16 tile (the buffer contract of include/tgs.h)
  return ssim_impl(W, H, img, gt, weight, block_partials, ((W + 15) / 16) * ((H + 15) / 16), v_img, scratch,
                   0, H, 0, H, stream);
}

extern "C" int tgs_ssim_fwd_bwd_rows(int W, int H, const float* img, const float* gt, float weight,
                                     float* block_partials, int n_partials, float* v_img,
                                     float* scratch, int y0, int y1, int count_y0, int count_y1,
                                     void* stream) {
  return ssim_impl(W, H, img, gt, weight, block_partials, n_partials, v_img, scratch, y0, y1, count_y0,
                   count_y1, stream);
}

extern "C" int tgs_set_ssim_form(int form) {
  if (form >= 0) g_ssim_form.set(form);
  return g_ssim_form.get();
}
