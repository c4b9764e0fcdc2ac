// knn.hip -- exact k nearest neighbours of 3-D points (include/tgs.h: tgs_knn_keys, tgs_knn_build, tgs_knn_query).
// gfx950.
//
//   k_knn_keys  : a thread per point: its 30-bit Morton key on a 1024^3 lattice over [lo, hi].  The caller sorts the keys.
//   k_knn_build : a workgroup per BOX = TGS_KNN_BOX consecutive points of the sorted order: gathers them into
//                 sorted_pts {x, y, z, original index} and reduces their bounding box.  Boxes of a Morton order are small
//                 where the cloud is dense and large where it is sparse: the structure adapts to the density by itself.
//   k_knn_query : a WAVE per 64 queries (a workgroup is one wave), a lane per query, queries taken in Morton order so that
//                 the 64 lanes want the same boxes.  (1) seed: the box whose FARTHEST corner is nearest to the wave's
//                 middle query, and its two neighbours in the sorted order, are searched first -- the k-th distance is tight
//                 from then on; (2) every other box, in chunks of 64 box records: a lane skips a box iff the box's lower
//                 bound exceeds its k-th distance, and the wave descends iff any lane did not skip.
//                 A lane's top-k sits in registers as an unrolled compare-and-shift chain (no dynamic index, no scratch).
//
// The definition (tgs.h):  d2 = (dx*dx + dy*dy) + dz*dz,  dx = qx - rx ..., every operation rounded to fp32 on its own
// (-ffp-contract=off, build.sh), the k smallest by (d2, original index).  The lower bound of a box is the SAME expression
// on the query's coordinates clamped into the box: for every point r of the box |q - clamp(q)| <= |q - r| per axis in the
// reals, and correctly rounded subtraction, product and sum are monotone, so bound <= d2(r) in fp32 as well; a box is
// skipped only on bound > worst, strictly -- at equality a lower index inside may still win.  So the result depends on
// neither the sort, the box size, the seed nor the launch shape.
//
// Box records and points were written by the launch before.  They reach the lanes through ordinary per-lane vector loads
// into LDS and wave-uniform LDS reads (a broadcast), never through loads indexed by loop counters alone, which the compiler
// would turn into scalar loads -- DESIGN 5.1j records stale reads from those on this chip.
#include <math.h>
#include "tgs_common.h"

namespace {

constexpr int KNN_BOX = TGS_KNN_BOX;
constexpr int KNN_EMPTY = INT_MAX;     // index of an empty slot while searching (so that a real d2 = +inf still enters); -1 on output

__device__ __forceinline__ unsigned knn_spread(unsigned v) {      // 10 bits -> every third bit
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

struct KnnQuant { float lo[3], scale[3]; };      // scale = 1024 / (hi - lo), or 0 where hi == lo (or hi - lo overflows)

__global__ __launch_bounds__(256) void k_knn_keys(int n, const float* __restrict__ pts, KnnQuant q, uint32_t* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  unsigned key = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float v = (pts[3 * (size_t)i + a] - q.lo[a]) * q.scale[a];
    const unsigned c = (unsigned)(int)fminf(fmaxf(v, 0.f), 1023.f);      // (NaN -> 0)
    key |= knn_spread(c) << a;
  }
  keys[i] = key;
}

__global__ __launch_bounds__(KNN_BOX) void k_knn_build(int n, const float* __restrict__ pts, const int32_t* __restrict__ order,
                                                        float* __restrict__ sorted_pts, float* __restrict__ boxes) {
  __shared__ float red[KNN_BOX / TGS_WAVE][6];
  const int pos = blockIdx.x * KNN_BOX + threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (pos < n) {
    const int o = min(max(order[pos], 0), n - 1);      // a permutation is the caller's promise; no index leaves pts either way
    float p[3];
#pragma unroll
    for (int a = 0; a < 3; a++) { p[a] = pts[3 * (size_t)o + a]; lo[a] = hi[a] = p[a]; }
    st4(sorted_pts + 4 * (size_t)pos, make_float4(p[0], p[1], p[2], __int_as_float(o)));
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], s));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], s));
    }
  }
  const int wave = threadIdx.x / TGS_WAVE;
  if (threadIdx.x % TGS_WAVE == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) { red[wave][a] = lo[a]; red[wave][3 + a] = hi[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int t = threadIdx.x;      // 0..2 min xyz, 3 pad, 4..6 max xyz, 7 pad
    float v = 0.f;
    if ((t & 3) != 3) {
      const int c = (t & 3) + (t >> 2) * 3;
      v = red[0][c];
#pragma unroll
      for (int w = 1; w < KNN_BOX / TGS_WAVE; w++) v = t < 4 ? fminf(v, red[w][c]) : fmaxf(v, red[w][c]);
    }
    boxes[8 * (size_t)blockIdx.x + t] = v;
  }
}

// (d2, index) order: the definition's
__device__ __forceinline__ bool knn_less(float ad, int ai, float bd, int bi) { return ad < bd || (ad == bd && ai < bi); }

template <int K>
struct KnnTop {
  float d[K];
  int i[K];
  float wd;      // slot k - 1: what a candidate must beat
  int wi;
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int j = 0; j < K; j++) { d[j] = INFINITY; i[j] = KNN_EMPTY; }
    wd = INFINITY; wi = KNN_EMPTY;
  }
  // (nd, ni) beats slot k - 1: shift it in.  Slots k .. K-1 keep further neighbours that nobody reads.
  __device__ __forceinline__ void insert(float nd, int ni, int k) {
#pragma unroll
    for (int j = K - 1; j > 0; j--) {
      const bool before_prev = knn_less(nd, ni, d[j - 1], i[j - 1]);
      const bool before_this = knn_less(nd, ni, d[j], i[j]);
      d[j] = before_prev ? d[j - 1] : (before_this ? nd : d[j]);
      i[j] = before_prev ? i[j - 1] : (before_this ? ni : i[j]);
    }
    if (knn_less(nd, ni, d[0], i[0])) { d[0] = nd; i[0] = ni; }
#pragma unroll
    for (int j = 0; j < K; j++)
      if (j == k - 1) { wd = d[j]; wi = i[j]; }
  }
};

struct KnnQuery { float x, y, z; int self; };      // self: the original index to skip, -1 = none

__device__ __forceinline__ float knn_d2(float qx, float qy, float qz, float rx, float ry, float rz) {
  const float dx = qx - rx, dy = qy - ry, dz = qz - rz;
  return (dx * dx + dy * dy) + dz * dz;
}

// The wave searches box b: its points go through LDS once, every lane tests all of them.
template <int K>
__device__ __forceinline__ void knn_search_box(int b, int n_ref, const float* __restrict__ sorted_pts, float4* stage, const KnnQuery& q,
                                               KnnTop<K>& top, int k) {
  const int lane = threadIdx.x, base = b * KNN_BOX, cnt = min(KNN_BOX, n_ref - base);
  __syncthreads();      // the last box's readers are done
#pragma unroll
  for (int e = 0; e < KNN_BOX / TGS_WAVE; e++) {
    const int j = e * TGS_WAVE + lane;
    if (j < cnt) stage[j] = ld4(sorted_pts + 4 * (size_t)(base + j));
  }
  __syncthreads();
#pragma unroll 4
  for (int j = 0; j < cnt; j++) {
    const float4 r = stage[j];
    const float d2 = knn_d2(q.x, q.y, q.z, r.x, r.y, r.z);
    const int ri = __float_as_int(r.w);
    if (knn_less(d2, ri, top.wd, top.wi) && ri != q.self) top.insert(d2, ri, k);
  }
}

template <int K>
__global__ __launch_bounds__(TGS_WAVE) void k_knn_query(int n_q, const float* __restrict__ queries, const int32_t* __restrict__ q_order,
                                                         int n_ref, const float* __restrict__ sorted_pts,
                                                         const float* __restrict__ boxes, int k, int exclude_self,
                                                         float* __restrict__ dist2, int32_t* __restrict__ idx) {
  __shared__ float4 stage[KNN_BOX];
  __shared__ float4 box_lo[TGS_WAVE], box_hi[TGS_WAVE];
  const int lane = threadIdx.x;
  const int t = blockIdx.x * TGS_WAVE + lane;
  // lanes past the last query repeat it and store nothing: no special case below
  const int tq = min(t, n_q - 1);
  const int qi = q_order ? min(max(q_order[tq], 0), n_q - 1) : tq;
  KnnQuery q;
  q.x = queries[3 * (size_t)qi]; q.y = queries[3 * (size_t)qi + 1]; q.z = queries[3 * (size_t)qi + 2];
  q.self = exclude_self ? qi : -1;
  KnnTop<K> top;
  top.init();
  const int nb = (n_ref + KNN_BOX - 1) / KNN_BOX;

  // (1) the seed: the box whose farthest corner is nearest to the query of lane 32 holds KNN_BOX points no farther than that
  const float mx = __shfl(q.x, 32), my = __shfl(q.y, 32), mz = __shfl(q.z, 32);
  float best = INFINITY;
  int seed = 0;
  for (int b = lane; b < nb; b += TGS_WAVE) {
    const float4 lo = ld4(boxes + 8 * (size_t)b), hi = ld4(boxes + 8 * (size_t)b + 4);
    const float fx = fmaxf(fabsf(mx - lo.x), fabsf(mx - hi.x)), fy = fmaxf(fabsf(my - lo.y), fabsf(my - hi.y)),
                fz = fmaxf(fabsf(mz - lo.z), fabsf(mz - hi.z));
    const float far2 = (fx * fx + fy * fy) + fz * fz;
    if (far2 < best) { best = far2; seed = b; }      // (ascending b: the lowest index among a lane's equals)
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const float ob = __shfl_xor(best, s);
    const int os = __shfl_xor(seed, s);
    if (ob < best || (ob == best && os < seed)) { best = ob; seed = os; }
  }
  seed = __builtin_amdgcn_readfirstlane(seed);      // (all lanes agree; an all-NaN-free input always has best < inf or nb boxes of it: seed 0)
  const int s0 = max(seed - 1, 0), s1 = min(seed + 1, nb - 1);
  for (int b = s0; b <= s1; b++) knn_search_box<K>(b, n_ref, sorted_pts, stage, q, top, k);

  // (2) every other box, 64 records at a time
  for (int c = 0; c < nb; c += TGS_WAVE) {
    __syncthreads();      // the last chunk's readers are done
    if (c + lane < nb) {
      box_lo[lane] = ld4(boxes + 8 * (size_t)(c + lane));
      box_hi[lane] = ld4(boxes + 8 * (size_t)(c + lane) + 4);
    }
    __syncthreads();
    const int m = min(TGS_WAVE, nb - c);
    for (int j = 0; j < m; j++) {
      const int b = c + j;
      if (b >= s0 && b <= s1) continue;
      const float4 lo = box_lo[j], hi = box_hi[j];
      const float bound = knn_d2(q.x, q.y, q.z, fminf(fmaxf(q.x, lo.x), hi.x), fminf(fmaxf(q.y, lo.y), hi.y),
                                 fminf(fmaxf(q.z, lo.z), hi.z));
      if (__ballot(!(bound > top.wd)) == 0ull) continue;
      knn_search_box<K>(b, n_ref, sorted_pts, stage, q, top, k);
    }
  }

  if (t < n_q) {
#pragma unroll
    for (int j = 0; j < K; j++) {
      if (j < k) {
        dist2[(size_t)qi * k + j] = top.d[j];
        idx[(size_t)qi * k + j] = top.i[j] == KNN_EMPTY ? -1 : top.i[j];
      }
    }
  }
}

}  // namespace

extern "C" int tgs_knn_keys(int n, const float* pts, const float* lo, const float* hi, uint32_t* keys, void* stream) {
  TGS_CHECK_ARG(n >= 1, "n < 1");
  TGS_CHECK_ARG(pts && keys, "null pts / keys");
  TGS_CHECK_ARG(lo && hi, "null lo / hi");
  KnnQuant q;
  for (int a = 0; a < 3; a++) {
    TGS_CHECK_ARG(isfinite(lo[a]) && isfinite(hi[a]), "non-finite lo / hi");
    TGS_CHECK_ARG(lo[a] <= hi[a], "inverted bounds (hi < lo)");
    const float ext = hi[a] - lo[a];
    q.lo[a] = lo[a];
    q.scale[a] = (ext > 0.f && isfinite(ext)) ? 1024.0f / ext : 0.f;      // hi == lo: the axis quantises to 0
    if (!isfinite(q.scale[a])) q.scale[a] = 0.f;                            // (a denormal extent)
  }
  hipLaunchKernelGGL(k_knn_keys, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, pts, q, keys);
  TGS_CHECK_LAUNCH();
  return TGS_OK;
}

extern "C" int tgs_knn_build(int n, const float* pts, const int32_t* order, float* sorted_pts, float* boxes, void* stream) {
  TGS_CHECK_ARG(n >= 1, "n < 1");
  TGS_CHECK_ARG(n <= INT_MAX / 4, "more points than the 32-bit index holds (n <= 2^29 - 1)");
  TGS_CHECK_ARG(pts && order, "null pts / order");
  TGS_CHECK_ARG(sorted_pts && boxes, "null sorted_pts / boxes");
  hipLaunchKernelGGL(k_knn_build, dim3((n + KNN_BOX - 1) / KNN_BOX), dim3(KNN_BOX), 0, (hipStream_t)stream, n, pts, order,
                     sorted_pts, boxes);
  TGS_CHECK_LAUNCH();
  return TGS_OK;
}

extern "C" int tgs_knn_query(int n_q, const float* queries, const int32_t* q_order, int n_ref, const float* sorted_pts,
                             const float* boxes, int k, int exclude_self, float* dist2, int32_t* idx, void* stream) {
  TGS_CHECK_ARG(n_q >= 1 && n_ref >= 1, "n_q / n_ref < 1");
  TGS_CHECK_ARG(n_ref <= INT_MAX / 4 && n_q <= INT_MAX / 4, "more points than the 32-bit index holds (n <= 2^29 - 1)");
  TGS_CHECK_ARG(k >= 1 && k <= TGS_KNN_MAX_K, "k outside [1, TGS_KNN_MAX_K]");
  TGS_CHECK_ARG(queries && sorted_pts && boxes, "null queries / sorted_pts / boxes");
  TGS_CHECK_ARG(dist2 && idx, "null dist2 / idx");
  TGS_CHECK_ARG(!exclude_self || n_q == n_ref, "exclude_self needs the queries to be the references (n_q == n_ref)");
  const dim3 grid((n_q + TGS_WAVE - 1) / TGS_WAVE), block(TGS_WAVE);
  if (k <= 4)
    hipLaunchKernelGGL(k_knn_query<4>, grid, block, 0, (hipStream_t)stream, n_q, queries, q_order, n_ref, sorted_pts, boxes, k,
                       exclude_self, dist2, idx);
  else
    hipLaunchKernelGGL(k_knn_query<16>, grid, block, 0, (hipStream_t)stream, n_q, queries, q_order, n_ref, sorted_pts, boxes, k,
                       exclude_self, dist2, idx);
  TGS_CHECK_LAUNCH();
  return TGS_OK;
}
