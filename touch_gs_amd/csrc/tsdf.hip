// tsdf.hip -- TSDF fusion of depth images into a voxel grid, and the grid's zero crossings as an oriented, coloured point
// cloud (include/tgs.h: tgs_tsdf_integrate, tgs_tsdf_extract_count, tgs_tsdf_extract_points).  gfx950.
//
//   k_tsdf_integrate : a GATHER.  A wave owns 256 consecutive voxels of the linear grid (x fastest) and walks them in four
//                      passes of 64: in a pass lane l holds voxel  wave * 256 + pass * 64 + l,  so the wave's loads and stores
//                      of S and Wt are one contiguous 256 B each (C: three of 256 B out of 768 contiguous bytes), and --
//                      what decides the time -- the 64 lanes of a gather look at 64 NEIGHBOURING voxels, which project to
//                      neighbouring pixels: a few cache lines per image read.  A first form gave a lane 4 consecutive
//                      voxels (16-byte loads and stores of the state): its lanes sat 4 voxels apart, every gather touched
//                      four times the lines, and it lost by 13 % (one view per launch) to 27 % (eight) at 256^3 / 720p
//                      (DESIGN 5.1k).  A voxel's (i, j, k) comes from its own linear index; nothing is stepped along a row,
//                      and rows of any length, the last partial wave included, take the same path.  Up to 8 views ride in
//                      the kernel arguments; a lane applies them to its voxels in array order, so a voxel's sequence of
//                      fp32 operations does not depend on how the views were batched.  Every voxel is read once and written
//                      once per launch by the one lane that owns it: no atomics, no order between lanes reaches an output.
//   k_tsdf_count     : a lane per voxel a: how many of its +x, +y, +z edges cross zero between two valid voxels.
//   k_tsdf_points    : a lane per voxel a: crossing m of the voxel (axis order) -> row offsets[a] + m.
//   k_tsdf_mesh_*    : the same level set as a triangle mesh, marching tetrahedra on the Kuhn split of every cell (include/tgs.h:
//                      tgs_tsdf_mesh_count, tgs_tsdf_mesh_emit): described where they stand, below.
//
// The depth, weight and colour images were written by earlier launches (the rasterizer).  They are read at a per-lane index
// through ordinary vector loads; the only values that come through the scalar cache are the kernel arguments themselves --
// DESIGN 5.1j records stale reads from compiler-chosen scalar loads of freshly written memory on this chip.
//
// Built with -ffp-contract=off (build.sh): every product and sum below rounds on its own, exactly as tests/tsdf_ref.py
// evaluates them with fp32 arrays; the emulation's error against fp64 is the kernel's.
#include <math.h>
#include "tgs_common.h"

namespace {

constexpr int TSDF_MAX_VIEWS = 8;
constexpr int TSDF_PER_LANE = 4;        // passes of a wave: voxels per lane
constexpr int TSDF_BLOCK = 256;

struct TsdfViewK {
  float R[9], t[3];
  float fx, fy, cx, cy;
  int W, H;
  float near_plane, pix_off;       // pix_off = 0.5 - pix_center
  const float* depth;
  const float* weight;
  const float* rgb;
};
struct TsdfViewsK { TsdfViewK v[TSDF_MAX_VIEWS]; };

__device__ __forceinline__ bool tsdf_pos_finite(float x) { return x > 0.f && x < INFINITY; }

// One view onto one voxel centre (X, Y, Z), grid-local.
__device__ __forceinline__ void tsdf_update(const TsdfViewK& vw, float X, float Y, float Z, float trunc, bool color, float& S,
                                            float& Wt, float& Cr, float& Cg, float& Cb) {
  const float pz = vw.R[6] * X + vw.R[7] * Y + vw.R[8] * Z + vw.t[2];
  if (!(pz > vw.near_plane)) return;
  const float px = vw.R[0] * X + vw.R[1] * Y + vw.R[2] * Z + vw.t[0];
  const float py = vw.R[3] * X + vw.R[4] * Y + vw.R[5] * Z + vw.t[1];
  const float fu = floorf(vw.fx * px / pz + vw.cx + vw.pix_off);
  const float fv = floorf(vw.fy * py / pz + vw.cy + vw.pix_off);
  if (!(fu >= 0.f && fu < (float)vw.W && fv >= 0.f && fv < (float)vw.H)) return;   // (NaN fails)
  const size_t pix = (size_t)(int)fv * vw.W + (int)fu;                              // inside the image
  const float D = vw.depth[pix];
  if (!tsdf_pos_finite(D)) return;
  const float w = vw.weight ? vw.weight[pix] : 1.0f;
  if (!tsdf_pos_finite(w)) return;
  const float sdf = D - pz;
  if (sdf < -trunc) return;
  const float d = fminf(sdf / trunc, 1.0f);
  S = S + w * d;
  Wt = Wt + w;
  if (color && vw.rgb) {
    Cr = Cr + w * vw.rgb[3 * pix];
    Cg = Cg + w * vw.rgb[3 * pix + 1];
    Cb = Cb + w * vw.rgb[3 * pix + 2];
  }
}

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_integrate(TsdfViewsK views, int n_views, int nx, int ny, int V, float vox,
                                                                float trunc, float* __restrict__ S, float* __restrict__ Wt,
                                                                float* __restrict__ C) {
  const int wave = (blockIdx.x * TSDF_BLOCK + threadIdx.x) / TGS_WAVE, lane = threadIdx.x % TGS_WAVE;
  const int base = wave * (TGS_WAVE * TSDF_PER_LANE) + lane;
  if (base >= V) return;
  float s[4], w[4], c[12], X[4], Y[4], Z[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int lin = base + e * TGS_WAVE;
    const bool in = lin < V;
    s[e] = in ? S[lin] : 0.f;
    w[e] = in ? Wt[lin] : 0.f;
#pragma unroll
    for (int q = 0; q < 3; q++) c[3 * e + q] = (in && C) ? C[3 * (size_t)lin + q] : 0.f;
    const int l2 = min(lin, V - 1);
    const int r = l2 / nx, i = l2 - r * nx, k = r / ny, j = r - k * ny;
    X[e] = ((float)i + 0.5f) * vox; Y[e] = ((float)j + 0.5f) * vox; Z[e] = ((float)k + 0.5f) * vox;
  }
  for (int v = 0; v < n_views; v++) {
    const TsdfViewK& vw = views.v[v];
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (base + e * TGS_WAVE < V) tsdf_update(vw, X[e], Y[e], Z[e], trunc, C != nullptr, s[e], w[e], c[3 * e], c[3 * e + 1], c[3 * e + 2]);
  }
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int lin = base + e * TGS_WAVE;
    if (lin < V) {
      S[lin] = s[e]; Wt[lin] = w[e];
      if (C) {
#pragma unroll
        for (int q = 0; q < 3; q++) C[3 * (size_t)lin + q] = c[3 * e + q];
      }
    }
  }
}

struct TsdfGridK { int nx, ny, nz, V; float vox, w_min; };

// f of a voxel; false = not valid (Wt < w_min, NaN included).
__device__ __forceinline__ bool tsdf_value(const float* __restrict__ S, const float* __restrict__ Wt, int lin, float w_min,
                                           float& f) {
  const float w = Wt[lin];
  if (!(w >= w_min)) return false;
  f = S[lin] / w;
  return true;
}

__device__ __forceinline__ bool tsdf_crosses(float fa, float fb) { return (fa < 0.f) != (fb < 0.f); }

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_count(TsdfGridK g, const float* __restrict__ S, const float* __restrict__ Wt,
                                                            int32_t* __restrict__ counts) {
  const int a = blockIdx.x * TSDF_BLOCK + threadIdx.x;
  if (a >= g.V) return;
  const int r = a / g.nx, i = a - r * g.nx, k = r / g.ny, j = r - k * g.ny;
  int cnt = 0;
  float fa, fb;
  if (tsdf_value(S, Wt, a, g.w_min, fa)) {
    if (i + 1 < g.nx && tsdf_value(S, Wt, a + 1, g.w_min, fb) && tsdf_crosses(fa, fb)) cnt++;
    if (j + 1 < g.ny && tsdf_value(S, Wt, a + g.nx, g.w_min, fb) && tsdf_crosses(fa, fb)) cnt++;
    if (k + 1 < g.nz && tsdf_value(S, Wt, a + g.nx * g.ny, g.w_min, fb) && tsdf_crosses(fa, fb)) cnt++;
  }
  counts[a] = cnt;
}

// d f / d (axis) at a VALID voxel `lin` (value f, index c of n along the axis, `step` voxels to the next): central where both
// neighbours are valid, one-sided where exactly one is, else 0.
__device__ __forceinline__ float tsdf_grad_axis(const TsdfGridK& g, const float* __restrict__ S, const float* __restrict__ Wt,
                                                int lin, float f, int c, int n, int step) {
  float fm = 0.f, fp = 0.f;
  const bool hm = c > 0 && tsdf_value(S, Wt, lin - step, g.w_min, fm);
  const bool hp = c + 1 < n && tsdf_value(S, Wt, lin + step, g.w_min, fp);
  if (hm && hp) return (fp - fm) / (2.0f * g.vox);
  if (hp) return (fp - f) / g.vox;
  if (hm) return (f - fm) / g.vox;
  return 0.f;
}

// The crossing between the VALID voxel a (value fa, indices idx, centre ca) and b = a + the offset `dm` (bit m set = +1
// along axis m; value fb) -> row `row` of points, normals and colours.  g(a) is formed at a's first crossing and kept in ga.
// One body for the point cloud (dm = one axis) and the mesh's seven edge classes: the same fp32 operations in the same order.
__device__ __forceinline__ void tsdf_vertex(const TsdfGridK& g, const float* __restrict__ S, const float* __restrict__ Wt,
                                            const float* __restrict__ C, int a, float fa, const int idx[3], const float ca[3],
                                            bool& have_ga, float ga[3], int b, float fb, int dm, int64_t row,
                                            float* __restrict__ points, float* __restrict__ normals, float* __restrict__ colors) {
  const int dim[3] = {g.nx, g.ny, g.nz}, step[3] = {1, g.nx, g.nx * g.ny};
  const float t = fa / (fa - fb);
  float p[3];
#pragma unroll
  for (int m = 0; m < 3; m++) p[m] = (dm >> m & 1) ? ca[m] + t * g.vox : ca[m];
  if (!have_ga) {
#pragma unroll
    for (int m = 0; m < 3; m++) ga[m] = tsdf_grad_axis(g, S, Wt, a, fa, idx[m], dim[m], step[m]);
    have_ga = true;
  }
  float nrm[3];
#pragma unroll
  for (int m = 0; m < 3; m++) {
    const float gb = tsdf_grad_axis(g, S, Wt, b, fb, idx[m] + (dm >> m & 1), dim[m], step[m]);
    nrm[m] = (1.0f - t) * ga[m] + t * gb;
  }
  const float len = sqrtf(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
  const bool ok = len > 0.f && len < INFINITY;
#pragma unroll
  for (int m = 0; m < 3; m++) {
    points[3 * row + m] = p[m];
    normals[3 * row + m] = ok ? nrm[m] / len : 0.f;
  }
  if (colors) {
    const float wa = Wt[a], wb = Wt[b];
#pragma unroll
    for (int m = 0; m < 3; m++) colors[3 * row + m] = (1.0f - t) * (C[3 * (size_t)a + m] / wa) + t * (C[3 * (size_t)b + m] / wb);
  }
}

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_points(TsdfGridK g, const float* __restrict__ S, const float* __restrict__ Wt,
                                                             const float* __restrict__ C, const int64_t* __restrict__ offsets,
                                                             float* __restrict__ points, float* __restrict__ normals,
                                                             float* __restrict__ colors, int64_t* __restrict__ edge_id) {
  const int a = blockIdx.x * TSDF_BLOCK + threadIdx.x;
  if (a >= g.V) return;
  float fa;
  if (!tsdf_value(S, Wt, a, g.w_min, fa)) return;
  const int r = a / g.nx, i = a - r * g.nx, k = r / g.ny, j = r - k * g.ny;
  const int idx[3] = {i, j, k}, dim[3] = {g.nx, g.ny, g.nz}, step[3] = {1, g.nx, g.nx * g.ny};
  const float ca[3] = {((float)i + 0.5f) * g.vox, ((float)j + 0.5f) * g.vox, ((float)k + 0.5f) * g.vox};
  int64_t row = offsets[a];
  bool have_ga = false;
  float ga[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
    if (idx[ax] + 1 >= dim[ax]) continue;
    const int b = a + step[ax];
    float fb;
    if (!tsdf_value(S, Wt, b, g.w_min, fb) || !tsdf_crosses(fa, fb)) continue;
    tsdf_vertex(g, S, Wt, C, a, fa, idx, ca, have_ga, ga, b, fb, 1 << ax, row, points, normals, colors);
    if (edge_id) edge_id[row] = 3 * (int64_t)a + ax;
    row++;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The triangle mesh: marching tetrahedra on the Kuhn split of every cell (include/tgs.h; the definition is
// tests/tsdf_mesh_ref.py).  Corner c of cell a, c = dx + 2 dy + 4 dz, is voxel a + dx + dy nx + dz nx ny.
//   k_tsdf_mesh_flags : a lane per voxel: one byte, bit 0 = valid, bit 1 = inside (f < 0) -- the later passes read one byte
//                       per corner instead of 8 bytes and a division.
//   k_tsdf_mesh_ntri  : a lane per cell a: the triangles of its six tetrahedra, 0 unless all eight corners are valid.
//   k_tsdf_mesh_vmask : a lane per voxel a: bit e set iff the edge a -> a + offset(e) has two valid ends, one of them inside,
//                       and lies in a cell with triangles (an active cell that holds a cut edge has at least one).
//   k_tsdf_mesh_emit  : a lane per voxel a: its vertices -> rows vert_offsets[a] ..., the triangles of cell a -> rows
//                       tri_offsets[a] ...; a vertex index is vert_offsets[a'] + popcount(vmask[a'] below the edge's bit).
// Lanes run along x: the byte loads and stores of a wave are 64 contiguous bytes.  No atomics, no order between lanes reaches
// an output.  flags, ntri and vmask were written by the launch before: they are read at per-lane indices (vector loads).
constexpr unsigned TSDF_F_VALID = 1u, TSDF_F_INSIDE = 2u;
constexpr unsigned TSDF_CLASS_BITS = 0x7563421u;     // hex digit e: the offset of edge class e as corner bits (x y z xy yz xz xyz)
constexpr unsigned TSDF_BITS_CLASS = 0x64523100u;    // hex digit d: the edge class of the offset with corner bits d
constexpr unsigned TSDF_TET_ODD = 0x26u;             // bit p: permutation p is odd
constexpr unsigned TSDF_EDGE_P = 0x211000u, TSDF_EDGE_Q = 0x332321u;   // hex digit n: the two corners of tetrahedron edge n

// [parity][inside mask, bit q = corner q of the tetrahedron] = {n, then n triangles of three tetrahedron-edge indices}:
// counter-clockwise seen from the outside.  Printed by tests/tsdf_mesh_ref.py (case_table_text); the CPU test compares.
__constant__ unsigned char TSDF_TET_CASES[2][16][7] = {
// TSDF_TET_CASES begin
  {{0, 0, 0, 0, 0, 0, 0}, {1, 0, 1, 2, 0, 0, 0}, {1, 0, 4, 3, 0, 0, 0}, {2, 1, 2, 4, 1, 4, 3},
   {1, 1, 3, 5, 0, 0, 0}, {2, 0, 3, 5, 0, 5, 2}, {2, 0, 4, 5, 0, 5, 1}, {1, 2, 4, 5, 0, 0, 0},
   {1, 2, 5, 4, 0, 0, 0}, {2, 0, 1, 5, 0, 5, 4}, {2, 0, 2, 5, 0, 5, 3}, {1, 1, 5, 3, 0, 0, 0},
   {2, 1, 3, 4, 1, 4, 2}, {1, 0, 3, 4, 0, 0, 0}, {1, 0, 2, 1, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0}},  // even
  {{0, 0, 0, 0, 0, 0, 0}, {1, 0, 2, 1, 0, 0, 0}, {1, 0, 3, 4, 0, 0, 0}, {2, 1, 4, 2, 1, 3, 4},
   {1, 1, 5, 3, 0, 0, 0}, {2, 0, 5, 3, 0, 2, 5}, {2, 0, 5, 4, 0, 1, 5}, {1, 2, 5, 4, 0, 0, 0},
   {1, 2, 4, 5, 0, 0, 0}, {2, 0, 5, 1, 0, 4, 5}, {2, 0, 5, 2, 0, 3, 5}, {1, 1, 3, 5, 0, 0, 0},
   {2, 1, 4, 3, 1, 2, 4}, {1, 0, 4, 3, 0, 0, 0}, {1, 0, 1, 2, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0}},  // odd
// TSDF_TET_CASES end
};

// hex digit q: corner q of the tetrahedron of permutation `tet` (xyz xzy yxz yzx zxy zyx) as corner bits
__device__ __forceinline__ unsigned tsdf_tet_corners(int tet) {
  constexpr unsigned c[6] = {0x7310u, 0x7510u, 0x7320u, 0x7620u, 0x7540u, 0x7640u};
  return c[tet];
}

__device__ __forceinline__ int tsdf_corner(const TsdfGridK& g, int a, int c) {
  return a + (c & 1) + (c >> 1 & 1) * g.nx + (c >> 2 & 1) * g.nx * g.ny;
}

// The inside bits of the eight corners of the EXISTING cell a (bit c = corner c); -1 if a corner is not valid.
__device__ __forceinline__ int tsdf_cell_inside(const TsdfGridK& g, const uint8_t* __restrict__ flags, int a) {
  unsigned all = TSDF_F_VALID, in = 0;
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const unsigned fl = flags[tsdf_corner(g, a, c)];
    all &= fl;
    in |= (fl >> 1 & 1u) << c;
  }
  return all ? (int)in : -1;
}

__device__ __forceinline__ unsigned tsdf_tet_case(unsigned in, int tet) {
  unsigned m = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) m |= (in >> (tsdf_tet_corners(tet) >> 4 * q & 7u) & 1u) << q;
  return m;
}

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_mesh_flags(TsdfGridK g, const float* __restrict__ S,
                                                                 const float* __restrict__ Wt, uint8_t* __restrict__ flags) {
  const int a = blockIdx.x * TSDF_BLOCK + threadIdx.x;
  if (a >= g.V) return;
  float f;
  const bool ok = tsdf_value(S, Wt, a, g.w_min, f);
  flags[a] = ok ? (uint8_t)(TSDF_F_VALID | (f < 0.f ? TSDF_F_INSIDE : 0u)) : (uint8_t)0;
}

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_mesh_ntri(TsdfGridK g, const uint8_t* __restrict__ flags,
                                                                uint8_t* __restrict__ ntri) {
  const int a = blockIdx.x * TSDF_BLOCK + threadIdx.x;
  if (a >= g.V) return;
  const int r = a / g.nx, i = a - r * g.nx, k = r / g.ny, j = r - k * g.ny;
  unsigned n = 0;
  if (i + 1 < g.nx && j + 1 < g.ny && k + 1 < g.nz) {
    const int in = tsdf_cell_inside(g, flags, a);
    if (in > 0 && in < 255) {
#pragma unroll
      for (int tet = 0; tet < 6; tet++) n += TSDF_TET_CASES[TSDF_TET_ODD >> tet & 1u][tsdf_tet_case(in, tet)][0];
    }
  }
  ntri[a] = (uint8_t)n;
}

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_mesh_vmask(TsdfGridK g, const uint8_t* __restrict__ flags,
                                                                 const uint8_t* __restrict__ ntri, uint8_t* __restrict__ vmask) {
  const int a = blockIdx.x * TSDF_BLOCK + threadIdx.x;
  if (a >= g.V) return;
  const int r = a / g.nx, i = a - r * g.nx, k = r / g.ny, j = r - k * g.ny;
  const unsigned fl = flags[a];
  unsigned vm = 0;
  if (fl & TSDF_F_VALID) {
#pragma unroll
    for (int e = 0; e < 7; e++) {
      const int dm = TSDF_CLASS_BITS >> 4 * e & 7;
      if (i + (dm & 1) >= g.nx || j + (dm >> 1 & 1) >= g.ny || k + (dm >> 2) >= g.nz) continue;
      const unsigned fb = flags[tsdf_corner(g, a, dm)];
      if (!(fb & TSDF_F_VALID) || !((fl ^ fb) & TSDF_F_INSIDE)) continue;
      // the cells a - s that hold the edge: s has no bit of dm
      bool held = false;
#pragma unroll
      for (int s = 0; s < 8; s++) {
        if (s & dm) continue;
        const int ci = i - (s & 1), cj = j - (s >> 1 & 1), ck = k - (s >> 2);
        if (ci < 0 || cj < 0 || ck < 0 || ci + 1 >= g.nx || cj + 1 >= g.ny || ck + 1 >= g.nz) continue;
        if (ntri[a - (tsdf_corner(g, a, s) - a)] != 0) held = true;
      }
      if (held) vm |= 1u << e;
    }
  }
  vmask[a] = (uint8_t)vm;
}

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_mesh_emit(TsdfGridK g, const float* __restrict__ S, const float* __restrict__ Wt,
                                                                const float* __restrict__ C, const uint8_t* __restrict__ flags,
                                                                const uint8_t* __restrict__ vmask,
                                                                const int64_t* __restrict__ vert_offsets,
                                                                const int64_t* __restrict__ tri_offsets, float* __restrict__ points,
                                                                float* __restrict__ normals, float* __restrict__ colors,
                                                                int64_t* __restrict__ edge_key, int32_t* __restrict__ faces) {
  const int a = blockIdx.x * TSDF_BLOCK + threadIdx.x;
  if (a >= g.V) return;
  const int r = a / g.nx, i = a - r * g.nx, k = r / g.ny, j = r - k * g.ny;
  const unsigned vm = vmask[a];
  float fa;
  if (vm && tsdf_value(S, Wt, a, g.w_min, fa)) {
    const int idx[3] = {i, j, k};
    const float ca[3] = {((float)i + 0.5f) * g.vox, ((float)j + 0.5f) * g.vox, ((float)k + 0.5f) * g.vox};
    int64_t row = vert_offsets[a];
    bool have_ga = false;
    float ga[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 7; e++) {
      if (!(vm >> e & 1u)) continue;
      const int dm = TSDF_CLASS_BITS >> 4 * e & 7;
      if (i + (dm & 1) >= g.nx || j + (dm >> 1 & 1) >= g.ny || k + (dm >> 2) >= g.nz) continue;   // (a mask from another grid)
      const int b = tsdf_corner(g, a, dm);
      float fb;
      if (!tsdf_value(S, Wt, b, g.w_min, fb)) continue;
      tsdf_vertex(g, S, Wt, C, a, fa, idx, ca, have_ga, ga, b, fb, dm, row, points, normals, colors);
      if (edge_key) edge_key[row] = 7 * (int64_t)a + e;
      row++;
    }
  }
  if (!(i + 1 < g.nx && j + 1 < g.ny && k + 1 < g.nz)) return;
  const int in = tsdf_cell_inside(g, flags, a);
  if (!(in > 0 && in < 255)) return;
  int64_t f = tri_offsets[a];
#pragma unroll
  for (int tet = 0; tet < 6; tet++) {
    const unsigned char* cs = TSDF_TET_CASES[TSDF_TET_ODD >> tet & 1u][tsdf_tet_case(in, tet)];
    const int n = cs[0];
    for (int tr = 0; tr < n; tr++) {
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const int te = cs[1 + 3 * tr + q];
        const int cp = tsdf_tet_corners(tet) >> 4 * (TSDF_EDGE_P >> 4 * te & 3u) & 7u;
        const int cq = tsdf_tet_corners(tet) >> 4 * (TSDF_EDGE_Q >> 4 * te & 3u) & 7u;
        const int owner = tsdf_corner(g, a, cp), cls = TSDF_BITS_CLASS >> 4 * (cq ^ cp) & 7u;
        faces[3 * f + q] = (int32_t)(vert_offsets[owner] + __popc((unsigned)vmask[owner] & ((1u << cls) - 1u)));
      }
      f++;
    }
  }
}

// dims, voxel size -> the voxel count; negative = refused (message set)
int tsdf_grid_ok(const char* who, int nx, int ny, int nz, float vox) {
  if (!(nx >= 1 && ny >= 1 && nz >= 1)) { tgs_set_error("%s: non-positive grid dims", who); return -1; }
  if (!(vox > 0.f && isfinite(vox))) { tgs_set_error("%s: voxel size not positive", who); return -1; }
  const int64_t V = (int64_t)nx * ny * nz;
  if (V > INT_MAX / 4) { tgs_set_error("%s: more voxels than the 32-bit index holds (nx ny nz <= 2^29 - 1)", who); return -1; }
  return (int)V;
}

}  // namespace

extern "C" int tgs_tsdf_integrate(int nx, int ny, int nz, float vox, float trunc, float* S, float* Wt, float* C, int n_views,
                                  const TgsTsdfView* views, void* stream) {
  const int V = tsdf_grid_ok(__func__, nx, ny, nz, vox);
  if (V < 0) return TGS_E_ARG;
  TGS_CHECK_ARG(trunc > 0.f && isfinite(trunc), "truncation distance not positive");
  TGS_CHECK_ARG(S && Wt, "null S / Wt");
  TGS_CHECK_ARG(n_views >= 1 && n_views <= TSDF_MAX_VIEWS, "n_views outside [1, 8]");
  TGS_CHECK_ARG(views, "null views");
  TsdfViewsK k;
  for (int v = 0; v < TSDF_MAX_VIEWS; v++) {
    const TgsTsdfView& s = views[v < n_views ? v : 0];
    if (v < n_views) {
      TGS_CHECK_ARG(s.depth, "view without a depth image");
      TGS_CHECK_ARG(s.W >= 1 && s.H >= 1 && (int64_t)s.W * s.H <= INT_MAX / 4, "bad image size");
      TGS_CHECK_ARG(s.fx > 0.f && s.fy > 0.f && isfinite(s.fx) && isfinite(s.fy) && isfinite(s.cx) && isfinite(s.cy),
                    "bad intrinsics");
      TGS_CHECK_ARG(isfinite(s.near_plane) && s.near_plane > 0.f && isfinite(s.pix_center), "bad near plane / pixel centre");
    }
    TsdfViewK& d = k.v[v];
    for (int i = 0; i < 9; i++) d.R[i] = s.R[i];
    for (int i = 0; i < 3; i++) d.t[i] = s.t[i];
    d.fx = s.fx; d.fy = s.fy; d.cx = s.cx; d.cy = s.cy; d.W = s.W; d.H = s.H;
    d.near_plane = s.near_plane; d.pix_off = 0.5f - s.pix_center;
    d.depth = s.depth; d.weight = s.weight; d.rgb = s.rgb;
  }
  const int lanes = (V + TSDF_PER_LANE - 1) / TSDF_PER_LANE;
  hipLaunchKernelGGL(k_tsdf_integrate, dim3((lanes + TSDF_BLOCK - 1) / TSDF_BLOCK), dim3(TSDF_BLOCK), 0, (hipStream_t)stream, k,
                     n_views, nx, ny, V, vox, trunc, S, Wt, C);
  TGS_CHECK_LAUNCH();
  return TGS_OK;
}

extern "C" int tgs_tsdf_extract_count(int nx, int ny, int nz, float vox, const float* S, const float* Wt, float w_min,
                                      int32_t* counts, void* stream) {
  const int V = tsdf_grid_ok(__func__, nx, ny, nz, vox);
  if (V < 0) return TGS_E_ARG;
  TGS_CHECK_ARG(w_min > 0.f && isfinite(w_min), "w_min not positive");
  TGS_CHECK_ARG(S && Wt && counts, "null S / Wt / counts");
  const TsdfGridK g = {nx, ny, nz, V, vox, w_min};
  hipLaunchKernelGGL(k_tsdf_count, dim3((V + TSDF_BLOCK - 1) / TSDF_BLOCK), dim3(TSDF_BLOCK), 0, (hipStream_t)stream, g, S, Wt,
                     counts);
  TGS_CHECK_LAUNCH();
  return TGS_OK;
}

extern "C" int tgs_tsdf_extract_points(int nx, int ny, int nz, float vox, const float* S, const float* Wt, const float* C,
                                       float w_min, const int64_t* offsets, float* points, float* normals, float* colors,
                                       int64_t* edge_id, void* stream) {
  const int V = tsdf_grid_ok(__func__, nx, ny, nz, vox);
  if (V < 0) return TGS_E_ARG;
  TGS_CHECK_ARG(w_min > 0.f && isfinite(w_min), "w_min not positive");
  TGS_CHECK_ARG(S && Wt && offsets, "null S / Wt / offsets");
  TGS_CHECK_ARG(points && normals, "null points / normals");
  TGS_CHECK_ARG(!colors || C, "colors without C");
  const TsdfGridK g = {nx, ny, nz, V, vox, w_min};
  hipLaunchKernelGGL(k_tsdf_points, dim3((V + TSDF_BLOCK - 1) / TSDF_BLOCK), dim3(TSDF_BLOCK), 0, (hipStream_t)stream, g, S, Wt, C,
                     offsets, points, normals, colors, edge_id);
  TGS_CHECK_LAUNCH();
  return TGS_OK;
}

extern "C" int tgs_tsdf_mesh_count(int nx, int ny, int nz, float vox, const float* S, const float* Wt, float w_min,
                                   uint8_t* vmask, uint8_t* ntri, uint8_t* flags, void* stream) {
  const int V = tsdf_grid_ok(__func__, nx, ny, nz, vox);
  if (V < 0) return TGS_E_ARG;
  TGS_CHECK_ARG(w_min > 0.f && isfinite(w_min), "w_min not positive");
  TGS_CHECK_ARG(S && Wt, "null S / Wt");
  TGS_CHECK_ARG(vmask && ntri && flags, "null vmask / ntri / flags");
  const TsdfGridK g = {nx, ny, nz, V, vox, w_min};
  const dim3 grid((V + TSDF_BLOCK - 1) / TSDF_BLOCK), block(TSDF_BLOCK);
  // (a grid with a dimension of 1 has no cells: the same three launches write zeros)
  hipLaunchKernelGGL(k_tsdf_mesh_flags, grid, block, 0, (hipStream_t)stream, g, S, Wt, flags);
  TGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_tsdf_mesh_ntri, grid, block, 0, (hipStream_t)stream, g, flags, ntri);
  TGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_tsdf_mesh_vmask, grid, block, 0, (hipStream_t)stream, g, flags, ntri, vmask);
  TGS_CHECK_LAUNCH();
  return TGS_OK;
}

extern "C" int tgs_tsdf_mesh_emit(int nx, int ny, int nz, float vox, const float* S, const float* Wt, const float* C, float w_min,
                                  const uint8_t* flags, const uint8_t* vmask, const int64_t* vert_offsets,
                                  const int64_t* tri_offsets, float* points, float* normals, float* colors, int64_t* edge_key,
                                  int32_t* faces, void* stream) {
  const int V = tsdf_grid_ok(__func__, nx, ny, nz, vox);
  if (V < 0) return TGS_E_ARG;
  TGS_CHECK_ARG(w_min > 0.f && isfinite(w_min), "w_min not positive");
  TGS_CHECK_ARG(S && Wt, "null S / Wt");
  TGS_CHECK_ARG(flags && vmask && vert_offsets && tri_offsets, "null flags / vmask / offsets");
  TGS_CHECK_ARG(points && normals && faces, "null points / normals / faces");
  TGS_CHECK_ARG(!colors || C, "colors without C");
  if (nx == 1 || ny == 1 || nz == 1) return TGS_OK;      // no cells: no vertex, no face, no launch
  const TsdfGridK g = {nx, ny, nz, V, vox, w_min};
  hipLaunchKernelGGL(k_tsdf_mesh_emit, dim3((V + TSDF_BLOCK - 1) / TSDF_BLOCK), dim3(TSDF_BLOCK), 0, (hipStream_t)stream, g, S, Wt,
                     C, flags, vmask, vert_offsets, tri_offsets, points, normals, colors, edge_key, faces);
  TGS_CHECK_LAUNCH();
  return TGS_OK;
}
