// gpis.hip -- a Gaussian-process implicit surface ray-marched into one view: touch depth, posterior variance and the surface
// normal (include/tgs.h, tgs_gpis_render).  The device form of touch_gs_amd.gpis.GPIS.render_depth.  gfx950.
//
// Three launches, ordered by the launches alone:
//   k_gpis_fill     : depth = var = NaN, normal = 0 on every pixel of the image; zeroes the crossing counter.
//   k_gpis_march    : one lane per ray of the region of interest, one wave (= one workgroup) per 8 x 8 rays: neighbouring
//                     rays find their brackets within a few samples of each other, and the wave leaves the march when its
//                     last ray has one.  The posterior mean  m(q) = sf2 sum_j alpha_j e_j + prior (1 - max_j e_j),
//                     e_j = exp(-|q - x_j|^2 / 2 l^2), in fp32 at the n_steps samples until the first change from > 0 to <= 0,
//                     12 bisection rounds, the nearest touched point by brute force, the facing test, the gradient of the mean
//                     at the crossing.  A facing crossing writes its depth (and normal) and appends its pixel to the crossing
//                     list through an INTEGER counter; the list's order never reaches an output.
//   k_gpis_variance : one lane per listed crossing:  var = sf2 - k^T Kinv k  with k in fp32, widened, and fp64 accumulation
//                     in a fixed order.  O(n^2) per crossing, blocked: a lane keeps a strip of STRIP fp64 partial sums
//                     s_i = sum_j Kinv[j][i] k_j (j ascending) in registers, adds k_i s_i (i ascending) to its total when the
//                     strip is complete, and recomputes k_j for every strip (n^2 / STRIP exponentials against n^2 fp64 FMAs;
//                     an n x rays staging array does not fit in LDS).  k^T Kinv k = k^T Kinv^T k for ANY matrix, so the strip
//                     reads ROW j at columns i0 ... i0 + STRIP - 1: contiguous.  Then the clamp at 0, the max_var cut (depth
//                     and var back to NaN, normal to 0) and var_floor, in the reference's order.
// The point lists (x_j, alpha_j), P and the rows of Kinv are the same for every lane.  They are STAGED THROUGH LDS by ordinary
// per-lane loads, 64 points (and 64 rows x STRIP columns of Kinv) at a time, and read back at one address by all lanes (a
// broadcast); every staged loop is wave-uniform -- a ray that is done, or a lane past the end, computes along for nothing --
// so the barriers around the staging are legal, and with one wave per workgroup they cost nothing.  A first form indexed
// the lists by the loop counters alone and let the compiler fetch them through the scalar data cache; on the MI355X it read
// stale bytes from point lists uploaded into memory that an earlier call's images had occupied: dropped.
// No float atomics: every output is a function of its own pixel alone and comes out the same bits on every call.
//
// Coordinates are centred on the centroid of the touched points by the caller, in fp64, before they are rounded to fp32, and
// every squared distance is a sum of squared DIFFERENCES.
#include <math.h>
#include "tgs_common.h"

namespace {

constexpr int BISECT = 12;
constexpr float FACING = -0.05f;
constexpr int STRIP = 16;          // fp64 partial sums a lane of k_gpis_variance keeps: 32 VGPRs
constexpr int RAY_TILE = 8;        // a wave marches RAY_TILE x RAY_TILE rays of the (strided) region

struct GpisK {
  float R[9], t[3];                // camera axes in the world (row = world axis, column = camera axis), centred position
  float fx, fy, cx, cy;
  int W, H, u0, v0, nx, ny, stride;
  float z_lo, dz;
  int n_steps;
  float max_var, var_floor;
  float c_exp;                     // -log2(e) / (2 l^2):  e_j = exp2(c_exp |q - x_j|^2)
  float inv_l2, sf2, prior;
};

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }

// Direction of the ray through pixel (u, v), in the world, with camera-space z = 1 (render_depth's dirs_c @ R^T).
__device__ __forceinline__ V3 gpis_ray(const GpisK& g, int u, int v) {
  const float dx = ((float)u + 0.5f - g.cx) / g.fx, dy = ((float)v + 0.5f - g.cy) / g.fy;
  return v3(fmaf(g.R[0], dx, fmaf(g.R[1], dy, g.R[2])), fmaf(g.R[3], dx, fmaf(g.R[4], dy, g.R[5])),
            fmaf(g.R[6], dx, fmaf(g.R[7], dy, g.R[8])));
}
__device__ __forceinline__ V3 gpis_point(const GpisK& g, V3 d, float z) {
  return v3(fmaf(z, d.x, g.t[0]), fmaf(z, d.y, g.t[1]), fmaf(z, d.z, g.t[2]));
}

// e_j without the signal variance; a result below fp32's normal range comes out 0.
__device__ __forceinline__ float gpis_e(const GpisK& g, V3 q, float4 x) {
  const float dx = q.x - x.x, dy = q.y - x.y, dz = q.z - x.z;
  return __builtin_amdgcn_exp2f(g.c_exp * (dx * dx + dy * dy + dz * dz));
}

// The point lists are the same for every lane.  A wave (= a workgroup here) stages them through LDS CHUNK points at a time:
// lane l loads point j0 + l (one coalesced 1 KiB load), every lane then reads point after point at one address (a broadcast).
// All 64 lanes of the wave take part in every staged loop -- the callers keep their control flow wave-uniform --, so the
// barriers are legal; with one wave per workgroup they cost nothing.
constexpr int CHUNK = TGS_WAVE;

// The posterior mean, a wave-collective call.  The products alpha_j e_j are summed in fp32 over blocks of SUM_BLOCK points and
// the block sums in fp64: the running sum of a plain fp32 chain swings through tens (sum |alpha_j| is 60 ... 220 on the
// repository's fits) and every add rounds at that size -- measured, 9e-6 m of depth against 1e-6 m this way --, while a block
// sum stays at the size of its terms.  One conversion and one fp64 add per SUM_BLOCK points.
constexpr int SUM_BLOCK = 8;
__device__ __forceinline__ float gpis_mean(const GpisK& g, int n, const float4* __restrict__ X, float4* sX, int lane, V3 q) {
  double acc = 0.0;
  float emax = 0.f;
  for (int j0 = 0; j0 < n; j0 += CHUNK) {
    __syncthreads();
    sX[lane] = X[min(j0 + lane, n - 1)];
    __syncthreads();
    const int cnt = min(CHUNK, n - j0);
    for (int i0 = 0; i0 < cnt; i0 += SUM_BLOCK) {
      float part = 0.f;
      if (i0 + SUM_BLOCK <= cnt) {
#pragma unroll
        for (int i = 0; i < SUM_BLOCK; i++) {
          const float4 x = sX[i0 + i];
          const float e = gpis_e(g, q, x);
          part = fmaf(x.w, e, part);
          emax = fmaxf(emax, e);
        }
      } else {
        for (int i = i0; i < cnt; i++) {
          const float4 x = sX[i];
          const float e = gpis_e(g, q, x);
          part = fmaf(x.w, e, part);
          emax = fmaxf(emax, e);
        }
      }
      acc += (double)part;
    }
  }
  return fmaf(g.sf2, (float)acc, g.prior * (1.0f - emax));
}

__global__ __launch_bounds__(256) void k_gpis_fill(int npix, float* __restrict__ depth, float* __restrict__ var,
                                                    float* __restrict__ normal, int* __restrict__ hits) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) hits[0] = 0;
  if (i >= npix) return;
  const float nan = __builtin_nanf("");
  depth[i] = nan;
  if (var) var[i] = nan;
  if (normal) { normal[3 * (size_t)i] = 0.f; normal[3 * (size_t)i + 1] = 0.f; normal[3 * (size_t)i + 2] = 0.f; }
}

__global__ __launch_bounds__(TGS_WAVE) void k_gpis_march(GpisK g, int n, const float4* __restrict__ X, int n_p,
                                                          const float* __restrict__ P, const float* __restrict__ N,
                                                          int tiles_x, float* __restrict__ depth, float* __restrict__ normal,
                                                          int* __restrict__ hits) {
  __shared__ float4 sX[CHUNK];
  const int lane = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int ix = tx * RAY_TILE + (lane & (RAY_TILE - 1)), iy = ty * RAY_TILE + lane / RAY_TILE;
  // a lane outside the region marches the region's last ray along, for nothing: every loop below is wave-uniform
  const bool live = ix < g.nx && iy < g.ny;
  const int u = g.u0 + min(ix, g.nx - 1) * g.stride, v = g.v0 + min(iy, g.ny - 1) * g.stride;   // inside the image
  const V3 d = gpis_ray(g, u, v);
  // the first sample with m <= 0 behind a sample with m > 0
  float prev = 0.f, z_hi = 0.f;
  bool found = false, open = live;
  for (int k = 0; k < g.n_steps; k++) {
    if (!__any(open)) break;                                  // (uniform: every ray of the wave has its bracket)
    const float z = fmaf((float)k, g.dz, g.z_lo);
    const float m = gpis_mean(g, n, X, sX, lane, gpis_point(g, d, z));
    if (open && k > 0 && prev > 0.f && m <= 0.f) { found = true; open = false; z_hi = z; }
    prev = m;
  }
  if (!__any(found)) return;
  float lo = z_hi - g.dz, hi = z_hi;                          // (a lane without a bracket bisects [-dz, 0], for nothing)
  for (int it = 0; it < BISECT; it++) {
    const float mid = 0.5f * (lo + hi);
    const bool inside = gpis_mean(g, n, X, sX, lane, gpis_point(g, d, mid)) <= 0.f;
    hi = inside ? mid : hi;
    lo = inside ? lo : mid;
  }
  const float zhit = 0.5f * (lo + hi);
  const V3 q = gpis_point(g, d, zhit);
  // the nearest touched point, the lowest index on ties; P staged as {x, y, z, -}
  float best = INFINITY;
  int nn = 0;
  for (int j0 = 0; j0 < n_p; j0 += CHUNK) {
    __syncthreads();
    const int jl = min(j0 + lane, n_p - 1);
    sX[lane] = make_float4(P[3 * jl], P[3 * jl + 1], P[3 * jl + 2], 0.f);
    __syncthreads();
    const int cnt = min(CHUNK, n_p - j0);
    for (int i = 0; i < cnt; i++) {
      const float4 p = sX[i];
      const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (d2 < best) { best = d2; nn = j0 + i; }
    }
  }
  const float facing = (N[3 * nn] * d.x + N[3 * nn + 1] * d.y + N[3 * nn + 2] * d.z) / sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
  const bool counted = found && facing < FACING;
  const int pix = v * g.W + u;
  if (counted) {
    depth[pix] = zhit;
    hits[1 + atomicAdd(&hits[0], 1)] = pix;
  }
  if (!normal || !__any(counted)) return;
  // grad m = (sf2 / l^2) sum_j alpha_j e_j (x_j - q)  -  (prior / l^2) e_J (x_J - q),  J = argmax_j e_j (lowest index on ties)
  // (summed like the mean: fp32 inside a block of SUM_BLOCK points, fp64 across the blocks)
  double ax = 0.0, ay = 0.0, az = 0.0;
  float emax = -1.f, jx = 0.f, jy = 0.f, jz = 0.f;
  for (int j0 = 0; j0 < n; j0 += CHUNK) {
    __syncthreads();
    sX[lane] = X[min(j0 + lane, n - 1)];
    __syncthreads();
    const int cnt = min(CHUNK, n - j0);
    for (int i0 = 0; i0 < cnt; i0 += SUM_BLOCK) {
      float px = 0.f, py = 0.f, pz = 0.f;
      const int i1 = min(i0 + SUM_BLOCK, cnt);
      for (int i = i0; i < i1; i++) {
        const float4 x = sX[i];
        const float dx = x.x - q.x, dy = x.y - q.y, dz = x.z - q.z;
        const float e = __builtin_amdgcn_exp2f(g.c_exp * (dx * dx + dy * dy + dz * dz));
        const float w = x.w * e;
        px = fmaf(w, dx, px); py = fmaf(w, dy, py); pz = fmaf(w, dz, pz);
        if (e > emax) { emax = e; jx = dx; jy = dy; jz = dz; }
      }
      ax += (double)px; ay += (double)py; az += (double)pz;
    }
  }
  if (!counted) return;
  float gx = (float)ax, gy = (float)ay, gz = (float)az;
  const float a = g.sf2 * g.inv_l2, b = g.prior * g.inv_l2 * emax;
  gx = a * gx - b * jx; gy = a * gy - b * jy; gz = a * gz - b * jz;
  // into the camera's axes (n_c = R^T n_w), unit length; a gradient of length 0 or not finite leaves the 0 of the fill
  const float cxn = g.R[0] * gx + g.R[3] * gy + g.R[6] * gz, cyn = g.R[1] * gx + g.R[4] * gy + g.R[7] * gz,
              czn = g.R[2] * gx + g.R[5] * gy + g.R[8] * gz;
  const float len = sqrtf(cxn * cxn + cyn * cyn + czn * czn);
  if (len > 0.f && isfinite(len)) {
    normal[3 * (size_t)pix] = cxn / len;
    normal[3 * (size_t)pix + 1] = cyn / len;
    normal[3 * (size_t)pix + 2] = czn / len;
  }
}

constexpr int KPITCH = STRIP + 1;   // doubles per staged row of Kinv: lanes write whole rows, 17 x 8 B apart = 34 banks

__global__ __launch_bounds__(TGS_WAVE) void k_gpis_variance(GpisK g, int n, const float4* __restrict__ X,
                                                             const double* __restrict__ Kinv, int* __restrict__ hits,
                                                             float* __restrict__ depth, float* __restrict__ var,
                                                             float* __restrict__ normal) {
  __shared__ float4 sX[CHUNK];
  __shared__ double sK[CHUNK * KPITCH];
  const int lane = threadIdx.x;
  const int count = __hip_atomic_load(&hits[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (the march kernel's counter)
  const int c = blockIdx.x * TGS_WAVE + lane;
  if (blockIdx.x * TGS_WAVE >= count) return;           // (uniform)
  // a lane past the end works on the last crossing, for nothing: the loops below stay wave-uniform
  const int pix = hits[1 + min(c, count - 1)];
  const int v = pix / g.W, u = pix - v * g.W;
  const V3 q = gpis_point(g, gpis_ray(g, u, v), depth[pix]);
  double total = 0.0;
  for (int i0 = 0; i0 < n; i0 += STRIP) {
    double s[STRIP];
#pragma unroll
    for (int i = 0; i < STRIP; i++) s[i] = 0.0;
    for (int j0 = 0; j0 < n; j0 += CHUNK) {
      // lane l stages point j0 + l and row j0 + l of Kinv at the strip's columns; a column past the end reads column n - 1
      // and is dropped below, a row past the end is not used
      __syncthreads();
      const int jl = min(j0 + lane, n - 1);
      sX[lane] = X[jl];
      const double* row = Kinv + (size_t)jl * n;
#pragma unroll
      for (int i = 0; i < STRIP; i++) sK[lane * KPITCH + i] = row[min(i0 + i, n - 1)];
      __syncthreads();
      const int cnt = min(CHUNK, n - j0);
      for (int j = 0; j < cnt; j++) {
        const double kj = (double)(g.sf2 * gpis_e(g, q, sX[j]));
#pragma unroll
        for (int i = 0; i < STRIP; i++) s[i] = fma(sK[j * KPITCH + i], kj, s[i]);
      }
    }
    // k_i of the strip's own points: staged like the rest
    __syncthreads();
    if (lane < STRIP) sX[lane] = X[min(i0 + lane, n - 1)];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < STRIP; i++) {
      if (i0 + i < n) total = fma((double)(g.sf2 * gpis_e(g, q, sX[i])), s[i], total);
    }
  }
  if (c >= count) return;
  const double vv = fmax((double)g.sf2 - total, 0.0);
  if (g.max_var >= 0.f && vv > (double)g.max_var) {
    depth[pix] = __builtin_nanf("");   // var holds the fill's NaN
    if (normal) { normal[3 * (size_t)pix] = 0.f; normal[3 * (size_t)pix + 1] = 0.f; normal[3 * (size_t)pix + 2] = 0.f; }
    return;
  }
  var[pix] = (float)fmax(vv, (double)g.var_floor);
}

}  // namespace

extern "C" int tgs_gpis_render(int n, const float* X, int n_p, const float* P, const float* N, const double* Kinv, float l,
                               float sf2, float prior, const TgsGpisView* view, float* depth, float* var, float* normal,
                               int32_t* hits, void* stream) {
  TGS_CHECK_ARG(n >= 1 && n_p >= 1, "no points");
  TGS_CHECK_ARG(X && P && N, "null point list");
  TGS_CHECK_ARG(((uintptr_t)X & 15) == 0, "X not 16-byte aligned");
  TGS_CHECK_ARG(((uintptr_t)Kinv & 7) == 0, "Kinv not 8-byte aligned");
  TGS_CHECK_ARG(l > 0.f && isfinite(l) && sf2 > 0.f && isfinite(sf2) && isfinite(prior), "bad kernel constants");
  TGS_CHECK_ARG(view, "null view");
  TGS_CHECK_ARG(view->W >= 1 && view->H >= 1 && (int64_t)view->W * view->H <= INT_MAX / 4, "bad image size");
  TGS_CHECK_ARG(view->fx > 0.f && view->fy > 0.f && isfinite(view->fx) && isfinite(view->fy) && isfinite(view->cx) &&
                    isfinite(view->cy),
                "bad intrinsics");
  TGS_CHECK_ARG(view->u0 >= 0 && view->v0 >= 0 && view->u1 >= view->u0 && view->v1 >= view->v0 && view->u1 < view->W &&
                    view->v1 < view->H,
                "region of interest outside the image");
  TGS_CHECK_ARG(view->stride >= 1, "stride < 1");
  TGS_CHECK_ARG(view->n_steps >= 2 && view->n_steps <= 512, "n_steps outside [2, 512]");
  TGS_CHECK_ARG(isfinite(view->z_lo) && view->dz > 0.f && isfinite(view->dz), "bad march interval");
  TGS_CHECK_ARG(isfinite(view->max_var) && isfinite(view->var_floor), "max_var / var_floor not finite");
  TGS_CHECK_ARG(Kinv || view->max_var < 0.f, "max_var without Kinv");
  TGS_CHECK_ARG(depth && hits, "null depth / hits");
  TGS_CHECK_ARG(!Kinv || var, "Kinv without var");
  hipStream_t s = (hipStream_t)stream;
  GpisK g;
  for (int i = 0; i < 9; i++) g.R[i] = view->R[i];
  for (int i = 0; i < 3; i++) g.t[i] = view->t[i];
  g.fx = view->fx; g.fy = view->fy; g.cx = view->cx; g.cy = view->cy;
  g.W = view->W; g.H = view->H; g.u0 = view->u0; g.v0 = view->v0; g.stride = view->stride;
  g.nx = (view->u1 - view->u0) / view->stride + 1;
  g.ny = (view->v1 - view->v0) / view->stride + 1;
  g.z_lo = view->z_lo; g.dz = view->dz; g.n_steps = view->n_steps;
  g.max_var = view->max_var; g.var_floor = view->var_floor;
  g.c_exp = (float)(-1.4426950408889634 / (2.0 * (double)l * (double)l));
  g.inv_l2 = (float)(1.0 / ((double)l * (double)l));
  g.sf2 = sf2; g.prior = prior;
  const int npix = g.W * g.H;
  hipLaunchKernelGGL(k_gpis_fill, dim3((npix + 255) / 256), dim3(256), 0, s, npix, depth, var, normal, hits);
  TGS_CHECK_LAUNCH();
  const int tiles_x = (g.nx + RAY_TILE - 1) / RAY_TILE, tiles_y = (g.ny + RAY_TILE - 1) / RAY_TILE;
  hipLaunchKernelGGL(k_gpis_march, dim3(tiles_x * tiles_y), dim3(TGS_WAVE), 0, s, g, n, reinterpret_cast<const float4*>(X), n_p,
                     P, N, tiles_x, depth, normal, hits);
  TGS_CHECK_LAUNCH();
  if (Kinv) {
    const int rays = g.nx * g.ny;
    hipLaunchKernelGGL(k_gpis_variance, dim3((rays + TGS_WAVE - 1) / TGS_WAVE), dim3(TGS_WAVE), 0, s, g, n,
                       reinterpret_cast<const float4*>(X), Kinv, hits, depth, var, normal);
    TGS_CHECK_LAUNCH();
  }
  return TGS_OK;
}
