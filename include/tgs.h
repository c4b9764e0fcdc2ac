/* tgs.h -- C ABI of libtgs_hip.so: the MI355X (gfx950) Gaussian-splatting hot path of Touch-GS.
 *
 * This is the drop-in boundary of SURVEY.md section 8(b).  Nothing in the reference tree calls C
 * (the reference shells out to `ns-train depth-gaussian-splatting`, scripts/train_bunny_real.sh:52,
 * whose rasterizer lives in an un-vendored submodule, .gitmodules:7-9), so each entry point cites
 * the reference-side *operator* it stands behind: the gsplat-0.1-shaped ops that nerfstudio's
 * Splatfacto model calls and the INRIA-shaped GaussianRasterizer (App. A.1).
 * The ctypes binding a maintainer adds is shown in INTEGRATION.md and lives in
 * touch_gs_amd/_lib.py.
 *
 * Conventions
 *  - plain pointers + sizes only; all pointers are DEVICE pointers unless marked [host];
 *    the caller (PyTorch) owns every buffer; the library never allocates device memory.
 *  - all work is enqueued on `stream` (a hipStream_t passed as void*); no hidden sync.
 *  - returns 0 (TGS_OK) or a negative TgsStatus; message via tgs_last_error() (thread-local).
 *  - fp32 / int32, contiguous row-major.  No float atomics anywhere: results are
 *    bit-reproducible run to run.
 */
#ifndef TGS_H
#define TGS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGS_VERSION 320         /* 0.3.2 -- 320 (additions only, nothing of 310 changed meaning): TgsCamera gains a trailing long_run and
                                   TgsRasterOpts gains k6_split_floor / k6_split_heads at its end (callers that pass the structs must pass the
                                   new sizes; a zeroed long_run and -1 in the new fields keep the behaviour of 310): what the tgs_set_long_run /
                                   tgs_set_k6_split_shape defaults choose for the process can now be chosen per call.
                                   310 (additions only, nothing of 300 changed meaning): TgsRasterOpts gains a sixth field k7_blocks
                                   (callers that pass the struct must pass the new size), tgs_adam_sh_gathered_geom_project_next,
                                   tgs_calib_fma_stream.  300: every entry point that takes `tile_start` takes its length next to it (validated against
                                   tgs_tile_start_len: the rasterizer keeps 512 scratch ints behind the starts) and the rasterize calls declare it
                                   non-const (they write that scratch); tgs_rasterize_fwd / _bwd / _bwd_band take a per-call TgsRasterOpts.
                                   201: tile_start buffers are T+513 ints; adds tgs_set_k7_quad, tgs_set_k6_split.  200 broke the ABI of 100:
                                   tgs_rasterize_fwd / tgs_rasterize_bwd[_band] gained stop_pos; earlier (round 3, then unversioned): status is int32[4], the
                                   rasterize calls carry slot_ok, splat slots 0/1 are rect-relative */
#define TGS_BLOCK 16            /* tile edge in pixels */
#define TGS_SPLAT_FLOATS 12     /* floats per projected-splat record */
#define TGS_PARTIAL_FLOATS 12   /* floats per (tile,Gaussian) partial-gradient record */
#define TGS_GROUP 256           /* Gaussians per binning group */

typedef enum TgsStatus {
  TGS_OK = 0,
  TGS_E_ARG = -1,        /* bad argument */
  TGS_E_HIP = -2,        /* a HIP runtime call failed */
  TGS_E_CAPACITY = -3    /* intersection capacity too small (see tgs_bin_sort) */
} TgsStatus;

/* Camera + frame constants.  viewmat: row-major world->camera, OpenCV axes
 * (x right, y down, z forward). */
typedef struct TgsCamera {
  float viewmat[16];
  float fx, fy, cx, cy;
  int32_t W, H;
  float near_plane;   /* 0.01 */
  float pix_center;   /* 0.5  */
  float bg[3];
  float glob_scale;   /* 1.0  */
  int32_t long_run;   /* binning: a Gaussian whose rect holds more tiles than this is a long run (tgs_set_long_run).  0 = the
                         process-wide default; otherwise clamped to 1 .. 256.  Not a camera property: it rides here because every
                         entry point of the front half and K8 takes the block, and ONE frame must use one value throughout
                         (TGS_VERSION 320) */
} TgsCamera;

/* Fused training loss evaluated inside the compositing backward:
 *   L = l1_weight * sum|C - gt_rgb|  +  sum_{gt_depth>0} depth_weight * w(U) * (D/alpha - gt_depth)^2
 *   w(U) = 1 (SIMPLE_LOSS) or 1/(uncertainty_weight*U + eps) (DEPTH_UNCERTAINTY_WEIGHTED_LOSS).
 * The caller folds the means in: l1_weight = (1-ssim_lambda)/(3*H*W), depth_weight =
 * depth_loss_mult / #valid.  Any pointer may be NULL to drop its term. */
typedef struct TgsLossSpec {
  const float* gt_rgb;      /* [H,W,3] */
  const float* gt_depth;    /* [H,W]   (0 = no supervision) */
  const float* uncertainty; /* [H,W]   (NULL => SIMPLE_LOSS) */
  float l1_weight;
  float depth_weight;
  float uncertainty_weight;
  float eps;                /* 1e-6 */
} TgsLossSpec;

/* Adam hyper-parameters for tgs_adam_step: the flat parameter buffer is
 *   means[3N] | log_scales[3N] | quats[4N] | opac_logit[N] | sh[N*K*3]
 * where every segment starts at the next multiple of 4 floats (16-byte aligned views; the total
 * is rounded up to a multiple of 4 too), with one learning rate per group, SH split into DC (k=0)
 * and the rest.  Pad elements must carry zero gradient. */
typedef struct TgsAdamSpec {
  float lr_means, lr_scales, lr_quats, lr_opac, lr_sh_dc, lr_sh_rest;
  float beta1, beta2, eps;
  float bias_corr1, bias_corr2;   /* 1-beta1^t, 1-beta2^t */
  const float* device_bias_corr;  /* NULL, or device {bias_corr1, bias_corr2, lr_means} read by the
                                     kernel at run time instead of the three host fields: lets a
                                     captured hipGraph of the step be replayed with each step's
                                     values (lr_means follows an exponential decay schedule) */
} TgsAdamSpec;

int tgs_version(void);
const char* tgs_last_error(void);

/* Box calibration (bench.py): enqueues a plain v_fma_f32 stream (16 independent accumulators per lane, 4 waves per SIMD
 * on every CU) of n_iter iterations; *n_wave_instr (host, may be NULL) = wave instructions issued.  Time it with events on
 * `stream`: wave instructions / second = what the vector pipes sustain on this box under its power governor.  `sink`:
 * one device float (never written in practice). */
int tgs_calib_fma_stream(int n_iter, float* sink, int64_t* n_wave_instr /*[host]*/, void* stream);

/* Number of binning groups / tiles for sizing the caller's buffers. */
int tgs_num_groups(int N);                 /* ceil(N/TGS_GROUP) */
int tgs_num_tiles(int W, int H);           /* ceil(W/16)*ceil(H/16) */
int tgs_num_bands(int W, int H);           /* image bands of tgs_rasterize_bwd_band */
int tgs_band_tiles(int W, int H, int band, int* tile0, int* tile1);   /* row-major tile range of a band */
int tgs_tile_order_len(int W, int H);      /* 8 * 8 * ceil(ceil(tiles / 8) / 8) (one entry per K6/K7 block) */
int tgs_tile_counter_len(int W, int H);    /* int32 entries of the tile_cursor scratch: per-XCD counter rows + sub-list starts */
int64_t tgs_tile_start_len(int W, int H);  /* int32 entries of a tile_start buffer: tiles + 1 + the rasterizer's 512 scratch ints.  Every call that
                                              takes `tile_start` takes `tile_start_len` = the entries the caller allocated and fails with TGS_E_ARG
                                              if that is less (the kernels write the scratch: a T + 1 allocation would be written out of bounds) */
/* Bytes of scratch tgs_bin_sort needs for a given intersection capacity. */
size_t tgs_sort_scratch_bytes(int64_t capacity);

/* K1  projection + 3D->2D covariance + SH colour  (stands behind gsplat `project_gaussians`
 *     + `spherical_harmonics`; INRIA preprocess, App. A.1; spec App. B.1-B.5).
 * in : means[N,3] log_scales[N,3] quats[N,4] (w,x,y,z un-normalised) opac_logit[N]
 *      sh[N,sh_stride,3] (NULL or sh_deg<0 => colours taken from `colors_in`[N,3] or zero)
 * out: splats[N,12] = {x - 16 x0, y - 16 y0, depth, opacity, conic a, b, c, r, g, b, rect, 0} where
 *      rect (uint32 bits) = x0 | y0<<8 | w<<16 | h<<24 is the Gaussian's tile rectangle: the App. B.4
 *      rect intersected with the tiles in which alpha can reach 1/255 (output preserving; 0 = none);
 *      culled Gaussians have conic 0.  Image sides are limited to 4080 px (255 tiles).
 *      Slots 0, 1 hold the screen position (App. B.2, pixel units) RELATIVE to the origin of the tile
 *      rect, evaluated in compensated fp32 arithmetic: ~1e-5 px instead of the 2.4e-4 px ulp of an
 *      absolute 4K coordinate (absolute position = slot + 16 * {x0, y0}).  Callers that build records
 *      themselves (tgs_bin_sort + tgs_rasterize_*) follow the same convention.
 *      radii[N] (may be NULL) = the App. B.3 3-sigma pixel radius, 0 if culled. */
int tgs_project_fwd(const TgsCamera* cam /*[host]*/, int N, const float* means,
                    const float* log_scales, const float* quats, const float* opac_logit,
                    const float* sh, int sh_stride, int sh_deg, const float* colors_in,
                    float* splats, int32_t* radii, void* stream);

/* Stand-alone SH evaluation (stands behind gsplat `spherical_harmonics`):
 *   colors[N,3] = sum_k Y_k(dirs / |dirs|) coeffs[N,k,:]  (no +0.5, no clamp);  backward w.r.t. the
 *   coefficients only (v_coeffs[N,sh_stride,3], rows k >= (sh_deg+1)^2 are zeroed). */
int tgs_sh_fwd(int N, int sh_deg, int sh_stride, const float* dirs, const float* coeffs,
               float* colors, void* stream);
int tgs_sh_bwd(int N, int sh_deg, int sh_stride, const float* dirs, const float* v_colors,
               float* v_coeffs, void* stream);

/* K2-K5  tile binning + per-tile depth sort  (stands behind gsplat `map_gaussian_to_intersects`,
 *     the CUB radix sort and `get_tile_bin_edges` inside `rasterize_gaussians`; spec App. B.4, B.6).
 * in : splats[N,12] (slot 11 is overwritten with the in-group intersection offset)
 * out: group_base[G]    start of each 256-Gaussian group's contiguous range in the pair index
 *                       space (G = tgs_num_groups; ranges are disjoint, their order is arbitrary)
 *      tile_start[tgs_tile_start_len] [start,end) of every tile's list; tile_start[T] = #intersections; the 512 ints behind it are
 *                       scratch of the rasterizer: a pair of words per XCD, 256 B apart, that tgs_rasterize_fwd folds the
 *                       frame's deepest walk and the sum of its walks into (zeroed here) and tgs_rasterize_bwd reads --
 *                       tgs_set_k7_quad -- and, 128 B behind each pair, a slot counter of tgs_rasterize_bwd.  Since TGS_VERSION 201 the buffer is T+513 ints
 *      sorted_gid[cap]  Gaussian ids, per tile, front to back, ties by id
 *      tile_order[L]    (may be NULL; L = tgs_tile_order_len) tile visited by block b of K6 / K7:
 *                       block b runs on XCD b % 8; XCD x owns every 8th granule of 8 consecutive
 *                       tiles (balanced for any view) and visits its tiles longest list first inside
 *                       chunks of <= 1024; entry [i * 8 + x] = i-th visit of XCD x, T = "no tile"
 *      status[4]        {#intersections, overflow flag, sufficient capacity, longest list}.  The pair index
 *                       space [0, capacity) is cut into 8 equal regions, one per XCD: every K1 workgroup
 *                       takes its 256-Gaussian group's contiguous pair range from the region of the XCD
 *                       it runs on, or from the first other region with room.  A frame can therefore
 *                       overflow slightly before #intersections reaches capacity (ranges are not split
 *                       across regions) but never when capacity >= status[2] = #intersections + 8 x the
 *                       largest group total -- whatever XCD the workgroups happen to run on.  Size
 *                       buffers from status[2] (written every frame), not from status[0].  On overflow
 *                       nothing past the scans is written, overflow = 1 and status[0] = status[2]
 *                       (caller grows to it and retries)
 *      sticky_overflow  (may be NULL) one persistent int32: set to 1 by an overflowing frame and
 *                       never cleared by the library; while it is 1 every frame starts with
 *                       status[1] = 1 (empty lists).  Together with the `skip_if_overflow` argument of
 *                       the optimizer entry points this lets a caller read the status words late,
 *                       without a per-frame host sync: after an overflow nothing touches the model
 *                       until the caller has cleared the word, grown the buffers and replayed.
 *      max_list_hint    < 0: no promise (every sort class is launched).  >= 0: the caller vouches that no tile's
 *                       list is longer than this (e.g. 1.25 x the largest status[3] its recent frames of this scene
 *                       reported): the launches for list classes beyond it -- (1024, 4096] and (4096, ..) entries,
 *                       each ~4.6 us of the stream even when it finds nothing to sort -- are not issued.  A frame
 *                       that breaks the promise is VOID like one that overflowed: the unsorted ids of the long
 *                       lists are copied through (valid indices: the compositing kernels do not fault), status[1]
 *                       = 1, the sticky word is raised, status[3] = the longest list -- raise the hint and replay.
 * tmp: tile_cursor[tgs_tile_counter_len(W,H)], scratch (tgs_sort_scratch_bytes(capacity)). */
int tgs_bin_sort(const TgsCamera* cam /*[host]*/, int N, float* splats, int32_t* group_base,
                 int32_t* tile_start, int64_t tile_start_len, int32_t* tile_cursor, int32_t* sorted_gid,
                 int32_t* tile_order, int64_t capacity, void* scratch, int32_t* status,
                 int32_t* sticky_overflow, int32_t max_list_hint, void* stream);

/* K1 + K2-K5 in one call (the fast path): the projection workgroup IS the 256-Gaussian binning
 *     group, so it also builds the group scan and counts its tile intersections -- the records are
 *     not re-read and the pair offset is stored with the record.  Arguments as in tgs_project_fwd
 *     (without colors_in) followed by those of tgs_bin_sort. */
int tgs_project_bin_sort(const TgsCamera* cam /*[host]*/, int N, const float* means,
                         const float* log_scales, const float* quats, const float* opac_logit,
                         const float* sh, int sh_stride, int sh_deg, float* splats, int32_t* radii,
                         int32_t* group_base, int32_t* tile_start, int64_t tile_start_len, int32_t* tile_cursor,
                         int32_t* sorted_gid, int32_t* tile_order, int64_t capacity, void* scratch,
                         int32_t* status, int32_t* sticky_overflow, int32_t max_list_hint, void* stream);

/* Colour prefetch (single-process training loop): the Gaussians' 3K SH coefficients are needed by K1
 *     only for the colour they give from the camera.  tgs_project_bwd_adam_next (below) evaluates
 *     that colour for the NEXT view inside the optimizer kernel, where the updated row is on chip,
 *     and this variant of tgs_project_bin_sort takes it:
 *       colors_in[N,3]  colours written by tgs_project_bwd_adam_next for THIS camera
 *       color_tag       the device word that call was given; colors_in is used iff
 *                       *color_tag == tag_expect (the optimizer kernel stores its tag_value last --
 *                       a step skipped on an overflowed frame leaves the old tag), otherwise the
 *                       colours are evaluated from `sh` exactly as tgs_project_bin_sort does.
 *     Results are bit-identical to tgs_project_bin_sort either way; K1 reads 56 B instead of
 *     44 + 12K B per Gaussian. */
int tgs_project_bin_sort_colors(const TgsCamera* cam /*[host]*/, int N, const float* means,
                                const float* log_scales, const float* quats, const float* opac_logit,
                                const float* sh, int sh_stride, int sh_deg, float* splats,
                                int32_t* radii, int32_t* group_base, int32_t* tile_start, int64_t tile_start_len,
                                int32_t* tile_cursor, int32_t* sorted_gid, int32_t* tile_order,
                                int64_t capacity, void* scratch, int32_t* status,
                                int32_t* sticky_overflow, int32_t max_list_hint, const float* colors_in,
                                const int32_t* color_tag, int32_t tag_expect, void* stream);

/* Per-call choice of the compositing kernels' forms (tgs_rasterize_fwd / _bwd / _bwd_band; NULL = every field -1).
 * A field < 0 takes the process-wide default: the value of the matching tgs_set_* call, else of the environment
 * variable (read once), else the built-in one.  A caller that needs re-entrancy passes the struct and never touches
 * the setters; the setters exist for A/B runs and tests and are process-wide by definition. */
typedef struct TgsRasterOpts {
  int32_t k6_blocks;         /* 1 / 0: forward in 4x4-block / quadrant form (bit-identical images)      [TGS_K6_BLOCKS, 1] */
  int32_t k6_split;          /* tile_is_split factor of the forward, 0 = never (tgs_set_k6_split)        [TGS_K6_SPLIT, 2]  */
  int32_t k7_front_to_back;  /* 1: backward in the front-to-back form of TGS_VERSION 100                 [TGS_K7_F2B, 0]    */
  int32_t k7_quad;           /* chain-bound factor of the backward, 0 = one wave per tile (tgs_set_k7_quad) [TGS_K7_QUAD, 8] */
  int32_t k7_quad_min_walk;  /* walks up to this many entries stay with the one-wave kernel              [TGS_K7_QUAD_MIN, 16] */
  int32_t k7_blocks;         /* 1: backward in 4x4-block form (TGS_VERSION 310; measured, not the default) [TGS_K7_BLOCKS, 0] */
  int32_t k6_split_floor;    /* shortest list the forward splits, never below 64 (tgs_set_k6_split_shape; TGS_VERSION 320) [TGS_K6_FLOOR, 256] */
  int32_t k6_split_heads;    /* leading schedule entries that get the three extra blocks (same)          [TGS_K6_HEADS, 512] */
} TgsRasterOpts;

/* K6  per-tile front-to-back compositing of RGB + depth in ONE pass  (stands behind gsplat
 *     `rasterize_gaussians` fwd, called twice by Splatfacto for rgb and depth; spec App. B.6).
 * out: out_rgb[H,W,3] (incl. background)  out_depth[H,W] (= sum w*depth, NOT divided by alpha)
 *      final_T[H,W]  final_idx[H,W] (list position of the last contributor, -1 if none; may be
 *      NULL -- the backward does not need it)
 * in : tile_order (may be NULL = spatial order) as produced by tgs_bin_sort: scheduling only, the
 *      results do not depend on it */
int tgs_rasterize_fwd(const TgsCamera* cam /*[host]*/, const float* splats,
                      const int32_t* sorted_gid, int32_t* tile_start, int64_t tile_start_len,
                      const int32_t* tile_order, float* out_rgb, float* out_depth, float* final_T,
                      int32_t* final_idx /*may be NULL*/, int32_t* stop_pos /*may be NULL*/,
                      uint64_t* slot_ok /*may be NULL*/, const TgsRasterOpts* opts /*[host], may be NULL*/,
                      void* stream);
/* tile_start is NOT const: the forward folds the frame's walk statistics into the scratch ints behind the starts and
 * the backward keeps a slot counter there (tgs_tile_start_len).  The starts themselves are only read.
 * The statistics (deepest walk: a maximum; sum of walks: a sum) are zeroed by the scan of tgs_*bin_sort* and ACCUMULATE
 * over the forwards that follow on the same lists: issue ONE forward with stop_pos != NULL per backward.  A forward
 * with stop_pos == NULL (render only) neither stores stop positions nor touches the statistics; pixels outside the
 * image count as walk 0.  (A doubled sum can only move the chain-bound verdict of tgs_rasterize_bwd towards "one wave
 * per tile": the two forms of K7 differ by the rounding of one four-term sum, never in which pairs they visit.) */
/* stop_pos[H,W] (optional; REQUIRED by tgs_rasterize_bwd*): per pixel the list position (relative to the
 * tile's first entry) of the Gaussian whose T' <= 1e-4 stopped the pixel (App. B.6) -- every earlier position
 * with alpha >= 1/255 contributed, nothing else did -- or 0x7fffffff if the pixel never stopped.  The
 * backward walks the lists back to front from there (since TGS_VERSION 200). */
/* slot_ok[4 * tgs_slot_ok_len(W, H, capacity)] (optional): per batch of 64 list positions of a tile, four
 * 64-bit maps (one per 8x8 quadrant) of the Gaussians that changed the quadrant's state in the forward.
 * Handed to tgs_rasterize_bwd* (same splats and lists) the backward skips the other (Gaussian, quadrant)
 * evaluations; the results are bit-identical with and without it. */
size_t tgs_slot_ok_len(int W, int H, int64_t capacity);

/* K6s per-pixel depth statistics of a composited frame (an ADDITION within TGS_VERSION 320: no struct and no earlier
 *     signature changed).  Forward only, no gradients.  Walks the lists a tgs_rasterize_fwd composited once more, with the
 *     forward's arithmetic on the same bits -- every pixel includes exactly the entries the forward included, with the
 *     same weights w = alpha T -- and needs that forward's images:
 * in : splats, sorted_gid, tile_start, tile_order (may be NULL; scheduling only) as given to tgs_rasterize_fwd;
 *      out_depth[H,W] (= sum w d), final_T[H,W] of that forward; stop_pos[H,W] of that forward or NULL (it only bounds
 *      the walk: the outputs are bit-identical with and without it)
 * out: depth_var[H,W]     sum w (d - D)^2 / alpha with D = out_depth / max(1 - final_T, 1e-10), alpha = max(1 - final_T,
 *                         1e-10): the variance of depth along the ray in the units of depth squared, accumulated as
 *                         written (every term >= 0); 0 where nothing contributed
 *      median_depth[H,W]  depth (record slot 2, bit for bit) of the first contributing Gaussian, front to back, behind
 *                         which the transmittance is <= 1/2; 0 where the transmittance never gets there (alpha < 1/2)
 *      median_gid[H,W]    (may be NULL) that Gaussian's id, -1 if none
 * tile_start is const here: the pass neither reads nor writes the scratch ints behind the starts (walk statistics, slot
 * counters), so it may run between a forward and its backward; tile_start_len is validated like in the other rasterize
 * calls (it is the same buffer).  opts: k6_split / k6_split_floor / k6_split_heads choose which long tiles are walked by
 * four blocks, as in the forward (bit-identical either way); the other fields are not looked at. */
int tgs_rasterize_depth_stats(const TgsCamera* cam /*[host]*/, const float* splats, const int32_t* sorted_gid,
                              const int32_t* tile_start, int64_t tile_start_len, const int32_t* tile_order /*may be NULL*/,
                              const float* out_depth, const float* final_T, const int32_t* stop_pos /*may be NULL*/,
                              float* depth_var, float* median_depth, int32_t* median_gid /*may be NULL*/,
                              const TgsRasterOpts* opts /*[host], may be NULL*/, void* stream);

/* Developer switch (A/B runs, tests): k6_blocks_on 1 / 0 = K6 in 4x4-block / quadrant form,
 * k7_front_to_back 1 / 0 = K7 in the front-to-back form of TGS_VERSION 100 / back to front; -1 leaves a
 * setting as it is.  Defaults: environment TGS_K6_BLOCKS (1), TGS_K7_F2B (0), read once at first use.
 * Returns the settings in force: bit 0 = block-form K6, bit 1 = front-to-back K7.
 * PROCESS-WIDE (atomic words; they only set the defaults a NULL / -1 TgsRasterOpts falls back to): a caller that
 * runs several models in one process passes TgsRasterOpts per call instead.  Same for the two setters below. */
int tgs_set_raster_variant(int k6_blocks_on, int k7_front_to_back);

/* In a CHAIN-BOUND frame K7 gives every tile that walks more than min_walk list entries to a workgroup of FOUR waves
 * (one per 8x8 quadrant) instead of one wave: in an object-centric scene a few hundred tiles carry walks of 700 - 1600
 * entries while the whole frame would fit 100 - 200 per wave slot, and the launch lasted as long as its longest tile.
 * A walk = how far into its list a tile's pixels reach; tgs_rasterize_fwd leaves the frame's deepest walk and the sum
 * of all walks behind tile_start.  A frame is chain-bound if the deepest walk exceeds factor / 2 times the sum spread
 * evenly over K7's 4096 wave slots.  Defaults: factor 8 (object-centric scenes of 100 - 300 k Gaussians at 720p qualify:
 * K7 0.58 - 0.78 of its one-wave time; a uniform scene such as configs[2] or 1 M clustered Gaussians at 1080p do not),
 * min_walk 16 (48 until TGS_VERSION 310); environment TGS_K7_QUAD / TGS_K7_QUAD_MIN.  factor 0 = always one wave per tile; a negative argument
 * leaves that setting.  Returns factor | min_walk << 8 in effect.  Ranges: factor 0 .. 255, min_walk 0 .. 2^23 - 1; larger
 * values (arguments or environment) are clamped to them, so the packed value is never negative and decodes to the
 * setting in force.  Results of the two forms differ by the rounding of one four-term sum per (tile, Gaussian). */
int tgs_set_k7_quad(int factor, int min_walk);

/* The LONGEST tiles of a chain-bound frame (TGS_VERSION 310; an EXPERIMENT, off by default: measured, the chain of the deepest
 * tile is 3x shorter and the step is not faster -- DESIGN.md 5.8, profiles/r6_ab_runs.txt).  Tiles that walk more than min_walk
 * entries, among the first `heads` entries of the tile_order schedule (longest lists first), are composited by
 * tgs_rasterize_bwd's scan form instead of the four-wave form: 16 waves per tile, one per 4x4 block; 16 entries that touch the
 * block in the lanes of a DPP row, transmittance and the sum behind as prefix scans.  min_walk 0 = off; negative arguments leave
 * a setting.  Environment TGS_K7_SCAN_MIN / TGS_K7_SCAN_HEADS; TGS_K7_SCAN_SIDE (default 1): the scan form's launch goes to an
 * internal stream beside the other launches of the call (fork / join by events on the caller's stream; one stream per process:
 * set 0 when several host threads call the backward concurrently).  Returns min_walk | heads << 16.  Ranges: min_walk
 * 0 .. 65535, heads 0 .. 32767; larger values (arguments or environment) are clamped to them.  Same decisions; sums in
 * scan order (rounding only). */
int tgs_set_k7_scan(int min_walk, int heads);

/* Binning: a Gaussian whose tile rect holds more than `tiles` tiles is a LONG RUN (TGS_VERSION 310): its pairs stay outside its
 * binning group's aggregated counting box (counted with direct atomics) and its partial-gradient records are summed by the
 * whole workgroup in K8 instead of by its own thread.  Default 32 (environment TGS_LONG_RUN).  8 suits object-centric
 * models, where a few thousand table / background Gaussians hold most of the pairs; the trainer chooses per model and passes
 * its choice per call in TgsCamera.long_run (model.spatial_sort; the row order `optim.balanced_order` deals exactly these
 * Gaussians evenly over the groups), which takes precedence over this default.  A launch-shape parameter: lists,
 * images and gradients are the same up to the rounding of K8's sums, whose shape depends on (tiles covered, this value).
 * tiles < 1 leaves the setting; returns the value in effect (1 .. 256).  Process-wide, like the other tgs_set_* tuning calls:
 * the default a TgsCamera with long_run = 0 falls back to. */
int tgs_set_long_run(int tiles);

/* The forward's counterpart for tiles with LONG lists: a tile whose list is longer than max(256, factor * I / 4096) --
 * factor (default 2 -- 4 until TGS_VERSION 310 --, environment TGS_K6_SPLIT) times the per-slot load of an even spread -- among the first 512 entries
 * of the tile_order schedule is composited by FOUR blocks of the same launch, one 8x8 quadrant each (pixels are
 * independent: nothing to exchange; same images, final_T and stop positions bit for bit).  Block-form forward with a
 * tile_order only.  factor 0 = never; negative leaves it.  Returns the factor in effect. */
int tgs_set_k6_split(int factor);
/* The shape of that rule (TGS_VERSION 310): `floor` = the shortest list it splits (default 256, environment TGS_K6_FLOOR, never
 * below 64) and `heads` = how many leading entries of the schedule get the three extra blocks (default 512, TGS_K6_HEADS).  An
 * object-centric 720p frame composites faster with factor 1, floor 128, 2048 heads (its mid-size lists are single waves on an
 * under-occupied GPU: -1.7 % of the step), uniform frames do not (-1 %): the trainer's re-sort chooses per model and passes
 * its choice per call (TgsRasterOpts.k6_split / k6_split_floor / k6_split_heads; model.spatial_sort); this call sets the
 * process-wide defaults those fields fall back to.  Negative arguments leave a setting; returns floor | heads << 16.  Ranges: floor 0 .. 65535, heads
 * 0 .. 32767; larger values (arguments or environment) are clamped to them.  Bit-identical outputs. */
int tgs_set_k6_split_shape(int floor, int heads);

/* K7  compositing backward with the tactile depth/uncertainty loss fused in  (stands behind
 *     gsplat `rasterize_gaussians` bwd; spec App. B.7).
 * in : out_rgb, out_depth, final_T, stop_pos of the forward (required);
 *      v_rgb[H,W,3] v_depth[H,W] v_alpha[H,W] upstream grads (each may be NULL);
 *      loss (may be NULL) adds dL/d(out) of the fused loss computed from out_rgb/out_depth/final_T;
 * out: partials[#intersections,12] one record per (tile,Gaussian) pair, addressed by the pair's
 *      pre-sort index = group_base[g/256] + splat[g].slot11 + index of the tile in g's rect:
 *      {v_x, v_y, v_depth, v_opacity, v_a, v_b, v_c, v_r, v_g, v_b, 0, 0}
 *      tile_loss[T,2] (may be NULL) per-tile {sum|C-gt|*l1_weight, depth-term} of the fused loss */
int tgs_rasterize_bwd(const TgsCamera* cam /*[host]*/, const float* splats,
                      const int32_t* group_base, const int32_t* sorted_gid,
                      int32_t* tile_start, int64_t tile_start_len, const int32_t* tile_order /*may be NULL*/,
                      const float* out_rgb, const float* out_depth, const float* final_T,
                      const int32_t* stop_pos, const float* v_rgb, const float* v_depth, const float* v_alpha,
                      const TgsLossSpec* loss /*[host]*/, float* partials, float* tile_loss,
                      const uint64_t* slot_ok /*may be NULL*/, const TgsRasterOpts* opts /*[host], may be NULL*/,
                      void* stream);

/* K7 for ONE image band: the tiles [tile0, tile1) of tgs_band_tiles(W, H, band, ...) (a contiguous row-major
 *     range; tgs_num_bands(W, H) >= 4 bands cover the image).  Needs the tile_order of tgs_bin_sort.  The
 *     bands together write exactly what tgs_rasterize_bwd writes; a band only reads the v_rgb / v_depth /
 *     v_alpha rows of its own tiles, so the image gradient may be produced band by band on another stream
 *     while earlier bands composite (DepthGaussianSplattingModel: SSIM pipelined behind K7). */
int tgs_rasterize_bwd_band(const TgsCamera* cam /*[host]*/, const float* splats,
                      const int32_t* group_base, const int32_t* sorted_gid,
                      int32_t* tile_start, int64_t tile_start_len, const int32_t* tile_order /*may be NULL*/,
                      const float* out_rgb, const float* out_depth, const float* final_T,
                      const int32_t* stop_pos, const float* v_rgb, const float* v_depth, const float* v_alpha,
                      const TgsLossSpec* loss /*[host]*/, float* partials, float* tile_loss,
                      int band, const uint64_t* slot_ok /*may be NULL*/,
                      const TgsRasterOpts* opts /*[host], may be NULL*/, void* stream);

/* K8a segmented reduction of the partials to one gradient record per Gaussian
 *     out: v_splats[N,12] = {v_x, v_y, v_depth, v_opacity, v_a, v_b, v_c, v_r, v_g, v_b, 0, 0}. */
int tgs_reduce_partials(int N, const float* splats, const int32_t* group_base,
                        const TgsCamera* cam /*[host]*/, const float* partials, float* v_splats,
                        void* stream);

/* K8  projection + SH backward  (stands behind gsplat `project_gaussians` bwd +
 *     `spherical_harmonics` bwd; spec App. B.8).
 * in : either partials (+group_base) -> reduced on the fly, or v_splats[N,12] (partials NULL)
 * out: v_means[N,3] v_log_scales[N,3] v_quats[N,4] v_opac_logit[N] v_sh[N,sh_stride,3]
 *      (all overwritten; v_sh may be NULL), v_xy[N,2] (may be NULL) = screen-space mean gradient (the
 *      INRIA `means2D.grad`), used for densification statistics. */
int tgs_project_bwd(const TgsCamera* cam /*[host]*/, int N, const float* means,
                    const float* log_scales, const float* quats, const float* opac_logit,
                    const float* sh, int sh_stride, int sh_deg, const float* splats,
                    const int32_t* group_base, const float* partials, const float* v_splats,
                    float* v_means, float* v_log_scales, float* v_quats, float* v_opac_logit,
                    float* v_sh, float* v_xy,
                    const int32_t* skip_if_overflow /*status[2] of the frame, or NULL*/, void* stream);

/* Camera-pose gradient: dL/dV of rows 0-2 of the world->camera matrix, V = [R | p] (camera refinement).
 *     A stand-alone pair of launches beside K8: it reads what tgs_project_bwd reads (the same two input forms: partials
 *     + group_base, or v_splats with partials NULL; sh may be NULL) BEFORE the optimizer changes the parameters, and
 *     changes nothing but its two outputs.  No atomics, bit-reproducible; no host synchronisation.
 * out[TGS_POSE_OUT]: [0..11] the raw 3x4 gradient, row-major like viewmat rows 0-2 (G_R | G_p);
 *     [12..23] per entry the sum of the absolute values of the products that form it (the unit of its rounding error);
 *     [24] 1 = valid, 0 = the frame was void (skip_if_overflow[1] != 0: everything else is 0 too);
 *     [25] number of visible Gaussians (exact below 2^24); [26..31] 0.
 * block_scratch[tgs_num_groups(N), TGS_POSE_ROW]: one row per 256-Gaussian group = the 24 values above and the group's
 *     count of visible Gaussians; overwritten. */
#define TGS_POSE_ROW 25
#define TGS_POSE_OUT 32
int tgs_pose_grad(const TgsCamera* cam /*[host]*/, int N, const float* means, const float* log_scales,
                  const float* quats, const float* sh, int sh_stride, int sh_deg, const float* splats,
                  const int32_t* group_base, const float* partials /*or NULL*/, const float* v_splats /*or NULL*/,
                  float* block_scratch, float* out,
                  const int32_t* skip_if_overflow /*status[2] of the frame, or NULL*/, void* stream);

/* K8+K9 fused (single-process training): projection/SH backward whose gradients go straight
 *     through the Adam update of the flat parameter buffer `params` (layout of TgsAdamSpec) and
 *     its moment buffers -- the 59-float gradient of a Gaussian never touches HBM.  Requires an
 *     SH tensor that stores 4 or 16 bases per Gaussian (sh_stride 4 or 16); sh_deg may be any
 *     degree the storage holds (rows above it receive a zero gradient).
 *     Not usable when gradients must first be all-reduced across ranks. */
int tgs_project_bwd_adam(const TgsCamera* cam /*[host]*/, int N, int sh_stride, int sh_deg,
                         float* params, float* exp_avg, float* exp_avg_sq,
                         const TgsAdamSpec* spec /*[host]*/, const float* splats,
                         const int32_t* group_base, const float* partials, float* v_xy,
                         const int32_t* skip_if_overflow /*status[2] of the frame, or NULL*/,
                         void* stream);

/* tgs_project_bwd_adam + the colour prefetch for the next view (see tgs_project_bin_sort_colors):
 *     after the update, colors_next[N,3] = max(sum_k Y_k(dir) c_k + 0.5, 0) of the UPDATED
 *     coefficients and means, seen from next_cam, at the same active degree; then
 *     *color_tag = tag_value.  On an overflowed frame (skip_if_overflow) neither is written. */
int tgs_project_bwd_adam_next(const TgsCamera* cam /*[host]*/, int N, int sh_stride, int sh_deg,
                              float* params, float* exp_avg, float* exp_avg_sq,
                              const TgsAdamSpec* spec /*[host]*/, const float* splats,
                              const int32_t* group_base, const float* partials, float* v_xy,
                              const int32_t* skip_if_overflow /*status[2] of the frame, or NULL*/,
                              const TgsCamera* next_cam /*[host]*/, float* colors_next,
                              int32_t* color_tag, int32_t tag_value, void* stream);

/* Front prefetch (single-process training loop): tgs_project_bwd_adam_next + the NEXT view's K1.  The fused
 *     optimizer kernel holds every updated parameter of its 256 Gaussians in registers and its workgroup IS the
 *     binning group, so it also projects them for next_cam, writes their records (splats_next[N,12], radii_next
 *     [N] or NULL), allocates the group's pair range (group_base_next) and counts its tile intersections
 *     (tile_cursor_next, ranks inside scratch_next) -- K1 of the next frame, with the arithmetic of the
 *     stand-alone kernel on the same values, hence bit-identical.  The call clears tile_cursor_next / status_next
 *     first (sticky_overflow as in tgs_bin_sort).  capacity_next / scratch_next as for tgs_bin_sort.
 *     tgs_project_bin_sort_front completes that frame (scan, fill, sort) on the SAME buffers: if *tag_word ==
 *     tag_expect the records and counts are there; otherwise (the optimizer kernel was voided by its overflow
 *     guard, which leaves the counters cleared and the tag unchanged) K1 runs now, from the SH rows. */
int tgs_project_bwd_adam_next_front(const TgsCamera* cam /*[host]*/, int N, int sh_stride, int sh_deg,
                                    float* params, float* exp_avg, float* exp_avg_sq,
                                    const TgsAdamSpec* spec /*[host]*/, const float* splats,
                                    const int32_t* group_base, const float* partials, float* v_xy,
                                    const int32_t* skip_if_overflow /*status[2] of the frame, or NULL*/,
                                    const TgsCamera* next_cam /*[host]*/, float* colors_next,
                                    int32_t* tag_word, int32_t tag_value, float* splats_next,
                                    int32_t* radii_next, int32_t* group_base_next, int32_t* tile_cursor_next,
                                    int64_t capacity_next, void* scratch_next, int32_t* status_next,
                                    int32_t* sticky_overflow,
                                    int counters_cleared /*1: tgs_project_bin_sort_front cleared them*/, void* stream);
/* Data-parallel counterpart (the optimizer is not fused with K8 there): Adam on the 11 geometry parameters of every
 *     Gaussian from the all-reduced flat gradient `grads` (layout of `params`, scaled by grad_scale) -- what
 *     tgs_adam_step does on [0, start of the SH segment) -- and, on the result, the next view's K1 with the colours
 *     from the (already stepped) SH rows, into the next frame's buffers; then *tag_word = tag_value.
 *     tgs_project_bin_sort_front completes that frame.  No-op (tag unchanged) if skip_if_overflow[1] != 0. */
int tgs_adam_geom_project_next(const TgsCamera* next_cam /*[host]*/, int N, int sh_stride, int sh_deg,
                               float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                               const TgsAdamSpec* spec /*[host]*/, float grad_scale,
                               const int32_t* skip_if_overflow, int32_t* tag_word, int32_t tag_value,
                               float* splats_next, int32_t* radii_next, int32_t* group_base_next,
                               int32_t* tile_cursor_next, int64_t capacity_next, void* scratch_next,
                               int32_t* status_next, int32_t* sticky_overflow, int counters_cleared, void* stream);
/* The whole tail of a data-parallel step in one launch (TGS_VERSION 310): tgs_adam_step_sh_gathered_rows for every row
 *     chunk of the pipelined exchange + tgs_adam_geom_project_next -- the updated SH rows stay on chip for the next
 *     camera's colours, the geometry gradients are read once.  chunk_begin[n_chunks + 1] (host; consecutive ranges from 0 to N,
 *     every begin a multiple of TGS_GROUP, n_chunks <= 8), chunk_blocks[n_chunks] (host array of DEVICE pointers to the
 *     all-gathered colour blocks [world][3 rows + 4] of each chunk).  Bit-identical to the unfused sequence.  It can
 *     only start once the geometry all-reduce has landed; callers with real links keep the chunked SH Adam, which hides
 *     under it (parallel.GradSync.fused_tail). */
int tgs_adam_sh_gathered_geom_project_next(const TgsCamera* next_cam /*[host]*/, int world, int N, int sh_stride, int sh_deg,
                                           float* params, const float* grads, int n_chunks,
                                           const int32_t* chunk_begin /*[host]*/, const float* const* chunk_blocks /*[host]*/,
                                           float* exp_avg, float* exp_avg_sq, const TgsAdamSpec* spec /*[host]*/,
                                           float grad_scale, const int32_t* skip_if_overflow, int32_t* tag_word,
                                           int32_t tag_value, float* splats_next, int32_t* radii_next,
                                           int32_t* group_base_next, int32_t* tile_cursor_next, int64_t capacity_next,
                                           void* scratch_next, int32_t* status_next, int32_t* sticky_overflow,
                                           int counters_cleared, void* stream);
int tgs_project_bin_sort_front(const TgsCamera* cam /*[host]*/, int N, const float* means,
                               const float* log_scales, const float* quats, const float* opac_logit,
                               const float* sh, int sh_stride, int sh_deg, float* splats, int32_t* radii,
                               int32_t* group_base, int32_t* tile_start, int64_t tile_start_len, int32_t* tile_cursor,
                               int32_t* sorted_gid, int32_t* tile_order, int64_t capacity, void* scratch,
                               int32_t* status, int32_t* sticky_overflow, int32_t max_list_hint,
                               const int32_t* tag_word, int32_t tag_expect,
                               const TgsCamera* next_cam /*[host] or NULL*/, int32_t* next_tile_cursor /*or NULL*/,
                               int32_t* next_status /*or NULL*/, void* stream);
/* A tag mismatch (the fused kernel was voided by its overflow guard) VOIDS the frame -- empty lists, status[1] = 1,
 * sticky raised -- instead of re-running K1 (TGS_VERSION < 300 did, in a launch of its own): the parameter pointers
 * are kept in the signature but no longer read.  next_tile_cursor != NULL: extra workgroups of this call's scan launch
 * also clear the counters and the status word of the frame AFTER this one (next_cam's size; sticky_overflow as usual)
 * -- pass counters_cleared = 1 to the optimizer call that fills them.  tgs_front_can_clear_next is always true now: */
int tgs_front_can_clear_next(int N, int W, int H);

/* Direct bins (an ADDITION within TGS_VERSION 320: three new calls, nothing earlier changes).  The K1 that runs inside
 *     the fused optimizer kernel knows, when it counts a (Gaussian, tile) pair, everything about it except where the tile's list
 *     starts -- which is all the fill pass of tgs_project_bin_sort_front adds, in a pass of its own over the records.  Given
 *         bins[(xcc * T + tile) * cap + rank] = {gid, depth bits}        (8 bytes each; T = tgs_num_tiles, xcc in [0, 8))
 *     it stores the pair at its arrival rank in the bin of its (XCC, tile) instead of remembering the rank, and
 *     tgs_project_bin_sort_front_bins only scans and sorts: the sorts gather a tile's list from its 8 sub-bins.  Every output
 *     (tile_start, sorted_gid, tile_order, status) is what the pair of calls without bins gives.
 *     cap in [1, 4096] is the caller's bound on the longest tile LIST, as max_list_hint: a sub-list beyond it drops its pairs and
 *     a list beyond it is not sorted, and either voids the frame (status[1] = 1, sticky raised) -- max_list_hint only chooses
 *     the sort classes below cap.  Which of the two happened depends on where the groups ran: when a sub-list overflowed, the
 *     scan empties every list before it measures them and status[3] (the longest list) reads 0, not the length that broke the
 *     bound -- a caller that sizes its next bound from status[3] must take it from a frame binned without bins (the trainer's
 *     replay does: it withdraws the bound, hence the bins, until it has learned a new one).  bins_len (entries of 8 bytes) must be >= tgs_bins_len(T, cap) = 8 * T * cap, checked before
 *     any launch.  The bins need no clearing.  Both calls of a frame take the same bins and cap; scratch is still required (a
 *     replay through tgs_project_bin_sort uses it). */
int64_t tgs_bins_len(int T, int cap);
/* tgs_bin_sort on records that exist, through the direct bins: the counting pass stores the pairs in the bins as the fused K1 does
 *     (the same device code), then scan and sort.  For tests and A/B runs of the front half alone. */
int tgs_bin_sort_bins(const TgsCamera* cam /*[host]*/, int N, float* splats, int32_t* group_base, int32_t* tile_start,
                      int64_t tile_start_len, int32_t* tile_cursor, int32_t* sorted_gid, int32_t* tile_order,
                      int64_t capacity, void* scratch, int32_t* status, int32_t* sticky_overflow, int32_t max_list_hint,
                      void* bins, int64_t bins_len, int32_t cap, void* stream);
int tgs_project_bwd_adam_next_front_bins(const TgsCamera* cam /*[host]*/, int N, int sh_stride, int sh_deg,
                                         float* params, float* exp_avg, float* exp_avg_sq,
                                         const TgsAdamSpec* spec /*[host]*/, const float* splats,
                                         const int32_t* group_base, const float* partials, float* v_xy,
                                         const int32_t* skip_if_overflow, const TgsCamera* next_cam /*[host]*/,
                                         float* colors_next, int32_t* tag_word, int32_t tag_value, float* splats_next,
                                         int32_t* radii_next, int32_t* group_base_next, int32_t* tile_cursor_next,
                                         int64_t capacity_next, void* scratch_next, int32_t* status_next,
                                         int32_t* sticky_overflow, int counters_cleared,
                                         void* bins, int64_t bins_len, int32_t cap, void* stream);
int tgs_project_bin_sort_front_bins(const TgsCamera* cam /*[host]*/, int N, const float* means,
                                    const float* log_scales, const float* quats, const float* opac_logit,
                                    const float* sh, int sh_stride, int sh_deg, float* splats, int32_t* radii,
                                    int32_t* group_base, int32_t* tile_start, int64_t tile_start_len, int32_t* tile_cursor,
                                    int32_t* sorted_gid, int32_t* tile_order, int64_t capacity, void* scratch,
                                    int32_t* status, int32_t* sticky_overflow, int32_t max_list_hint,
                                    const int32_t* tag_word, int32_t tag_expect,
                                    const TgsCamera* next_cam /*[host] or NULL*/, int32_t* next_tile_cursor /*or NULL*/,
                                    int32_t* next_status /*or NULL*/, const void* bins, int64_t bins_len, int32_t cap,
                                    void* stream);

/* Data-parallel step (one view per rank, SURVEY section 8 row e).  The SH gradient of a rank is the
 *     outer product Y_k(dir(g)) x v_color[g,:], so the ranks exchange v_color (all-gather, 3 floats
 *     per Gaussian and rank) instead of all-reducing 3*sh_stride floats per Gaussian:
 *   tgs_project_bwd_color      = tgs_project_bwd (partials path) that writes, instead of v_sh, the
 *                                block v_color[3N+4] = clamp-gated colour gradients [N,3] followed
 *                                by this camera's position [3] and one zero pad;
 *   tgs_adam_step_sh_gathered  = Adam on the SH segment of `params` with the gradient
 *                                grad_scale * sum_r Y_k(dir_r(g)) * v_color_r[g,:], rebuilt in rank
 *                                order from v_color_all[world][3N+4] (the all-gathered blocks).
 *                                The means inside `params` must still be the ones the forward
 *                                pass used (step the geometry segments with tgs_adam_step
 *                                afterwards).  Requires 3*sh_stride % 4 == 0.
 *   Sync-free intersection budget under data parallelism: with `skip_if_overflow` (the frame's
 *   status word) tgs_project_bwd_color does nothing on an overflowed frame except setting the pad of
 *   its block to 1; after the all-gather tgs_dp_agree_overflow writes status_out = {0, any pad != 0}
 *   (identical on every rank) and raises the caller's sticky word, and the optimizer entry points
 *   take status_out as their `skip_if_overflow`. */
int tgs_project_bwd_color(const TgsCamera* cam /*[host]*/, int N, const float* means,
                          const float* log_scales, const float* quats, const float* opac_logit,
                          const float* sh, int sh_stride, int sh_deg, const float* splats,
                          const int32_t* group_base, const float* partials, float* v_means,
                          float* v_log_scales, float* v_quats, float* v_opac_logit, float* v_color,
                          float* v_xy, const int32_t* skip_if_overflow /*status[2] of the frame, or NULL*/,
                          void* stream);
/* Row-range forms (one chunk of a pipelined exchange; results bit-identical to the whole-model calls):
 *   tgs_project_bwd_color_rows      rows [row_begin, row_end) of the model, row_begin a multiple of TGS_GROUP;
 *                                   all arrays are the whole model's except v_color_rows = the CHUNK's block
 *                                   [3 (row_end - row_begin) + 4] (colour gradients | camera position | pad);
 *   tgs_adam_step_sh_gathered_rows  the SH rows [row_begin, row_end) from the all-gathered chunk blocks
 *                                   v_color_rows_all[world][3 (row_end - row_begin) + 4]. */
int tgs_project_bwd_color_rows(const TgsCamera* cam /*[host]*/, int N, int row_begin, int row_end,
                               const float* means, const float* log_scales, const float* quats,
                               const float* opac_logit, const float* sh, int sh_stride, int sh_deg,
                               const float* splats, const int32_t* group_base, const float* partials,
                               float* v_means, float* v_log_scales, float* v_quats, float* v_opac_logit,
                               float* v_color_rows, float* v_xy, const int32_t* skip_if_overflow, void* stream);
int tgs_adam_step_sh_gathered_rows(int world, int N, int row_begin, int row_end, int sh_stride, int sh_deg,
                                   float* params, const float* v_color_rows_all, float* exp_avg,
                                   float* exp_avg_sq, const TgsAdamSpec* spec /*[host]*/, float grad_scale,
                                   const int32_t* skip_if_overflow, void* stream);
int tgs_dp_agree_overflow(int world, int N, const float* v_color_all, int32_t* status_out,
                          int32_t* sticky_overflow /*may be NULL*/, void* stream);
int tgs_adam_step_sh_gathered(int world, int N, int sh_stride, int sh_deg, float* params,
                              const float* v_color_all, float* exp_avg, float* exp_avg_sq,
                              const TgsAdamSpec* spec /*[host]*/, float grad_scale,
                              const int32_t* skip_if_overflow /*status_out of tgs_dp_agree_overflow, or NULL*/,
                              void* stream);

/* Stores n <= 8 host floats into device memory; the values travel as launch arguments, so the call is
 * stream ordered without any host staging buffer.  Used to refresh TgsAdamSpec.device_bias_corr
 * before a captured step graph is replayed. */
int tgs_store_small(float* dst, const float* host_vals /*[host]*/, int n, void* stream);

/* K9  fused Adam over the flat parameter buffer (torch.optim.Adam semantics, no weight decay).
 *     Updates elements [elem_begin, elem_end) of the flat buffers (multiples of 4; pass 0, -1 for
 *     everything) so that chunks can be stepped as their gradient all-reduce completes. */
int tgs_adam_step(int N, int sh_stride, float* params, const float* grads, float* exp_avg,
                  float* exp_avg_sq, const TgsAdamSpec* spec /*[host]*/, float grad_scale,
                  int64_t elem_begin, int64_t elem_end,
                  const int32_t* skip_if_overflow /*status[2] of the frame, or NULL*/, void* stream);

/* Fixed-budget MCMC strategy (3DGS-MCMC, Kheradmand et al. 2024; an ADDITION within TGS_VERSION 320: a new struct and two
 *     new calls, nothing earlier changes; csrc/mcmc.hip, touch_gs_amd/mcmc.py).
 * tgs_mcmc_adam_geom: ONE launch, a thread per Gaussian, over the GEOMETRY segments of the flat layout (means, log_scales,
 *     quats, opac_logit); the SH segment, its moments and every pad are not written -- step them with
 *     tgs_adam_step(elem_begin = start of sh, elem_end = -1).  Per Gaussian, with o = sigmoid(ol) and s_j = exp(ls_j) of
 *     the parameters BEFORE the update:
 *        g_ol   += opacity_reg / N * o (1 - o)          g_ls_j += scale_reg / (3 N) * s_j
 *     (the gradients of opacity_reg * mean(o) + scale_reg * mean(s)); then the Adam update of tgs_adam_step on the 11 values
 *     with g' = grad_scale (g + reg) -- the same device function, so with both weights 0 and noise NULL the results equal
 *     tgs_adam_step(0, start of sh) bit for bit; then, if noise != NULL, from the UPDATED values o', s', q':
 *        t = gate_k (o' - gate_o0),  gate = 0 if t > 80, else 1 / (1 + exp(t)),  R = R(q' / |q'|)
 *        means += (noise_lr * lr_means * gate) * R diag(s'^2) R^T n,    n = noise[g] (standard normal draws of the caller)
 *     with lr_means the one the Adam update used (spec->device_bias_corr[2] where that is given).  A frame whose guard
 *     word has its overflow flag set makes the launch a no-op.  No atomics: the same inputs give the same bits.
 * tgs_mcmc_relocate: gsplat's compute_relocation for n rows, in place, a thread per row.  ratio[i] <= 1: row i is not
 *     touched.  Otherwise r = min(ratio[i], 51), o = sigmoid(ol):
 *        x = 1 - (1 - o)^(1/r),   S = sum_{i=1..r} sum_{k=0..i-1} C(i-1, k) (-1)^k x^(k+1) / sqrt(k+1)
 *        ol <- logit(clamp(x, min_opacity, 1 - 2^-23)),   ls_j <- ls_j + log(o / S)
 *     evaluated in fp64 from the fp32 inputs and rounded once (naive fp32 is wrong by 2e-4 relative at both ends of the
 *     opacity range: the sum cancels to 1 / 2.9e4 of its terms at o = 1 - 2^-23, r = 51).
 * Both check every argument before any launch; accuracy: tests/test_gpu_mcmc.py against tests/mcmc_ref.py. */
typedef struct TgsMcmcSpec {
  float opacity_reg;   /* lambda_o (gsplat: 0.01) */
  float scale_reg;     /* lambda_s (0.01) */
  float noise_lr;      /* 5e5; the noise is scaled by noise_lr * (the resolved lr_means of the Adam spec) */
  float gate_k;        /* 100 */
  float gate_o0;       /* 0.005 */
} TgsMcmcSpec;
int tgs_mcmc_adam_geom(int N, int sh_stride, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                       const TgsAdamSpec* spec /*[host]*/, float grad_scale, const TgsMcmcSpec* mcmc /*[host]*/,
                       const float* noise /*[N,3] standard normal, or NULL = no noise*/,
                       const int32_t* skip_if_overflow /*status[2] of the frame, or NULL*/, void* stream);
int tgs_mcmc_relocate(int n, const int32_t* ratio /*[n], >= 1*/, float* opac_logit /*[n], in place*/,
                      float* log_scales /*[n,3], in place*/, float min_opacity, void* stream);

/* K10 SSIM (11x11 Gaussian window, sigma 1.5, zero padding) forward + gradient image; the
 *     (1-SSIM) term of the Splatfacto-style loss.
 * out: block_partials[ceil(H/16)*ceil(W/16)] per-tile sums of the SSIM map (deterministic;
 *      mean SSIM = sum / (3*H*W)),
 *      v_img[H,W,3] = weight * d(sum of SSIM map)/d(img)   (NULL => forward only)
 * tmp: scratch[9*H*W] floats (needed when v_img != NULL).
 * Accuracy: the variances are formed as sigma = E[x^2] - mu^2 in fp32, and the map divides by sigma11 + sigma22 + C2
 *     (C2 = 9e-4).  The error of the map and of v_img is therefore bounded in units of the fp32 conditioning of that
 *     difference, per pixel u = 2^-24 ((E[x^2] + mu1^2 + E[y^2] + mu2^2 + 2|E[xy]| + 2|mu1 mu2| + C2) / (sigma11 + sigma22 + C2) + 8),
 *     NOT by a fixed 1e-5: u is ~1e-6 on textured images and ~4e-4 on flat bright ones.  On a constant region every pixel
 *     rounds alike, so the error of a sum of the map there is systematic and does not average out.  Bounds and measured
 *     figures: tests/test_gpu_ssim_oracle.py (reference and unit: tests/ssim_ref.py). */
int tgs_ssim_fwd_bwd(int W, int H, const float* img, const float* gt, float weight,
                     float* block_partials, float* v_img, float* scratch, void* stream);
/* The same for the image rows [y0, y1) only (one band of a pipelined step, see tgs_rasterize_bwd_band):
 *     v_img rows [y0, y1) are written; the SSIM map is summed over rows [count_y0, count_y1) (inside
 *     [y0, y1); the bands of an image partition its rows) into block_partials[n_partials] (first entries =
 *     workgroup sums, the rest zero); scratch rows [y0-5, y1+5) are overwritten.  Values are bit-identical to
 *     the whole-image call. */
int tgs_ssim_fwd_bwd_rows(int W, int H, const float* img, const float* gt, float weight,
                          float* block_partials, int n_partials, float* v_img, float* scratch,
                          int y0, int y1, int count_y0, int count_y1, void* stream);
/* Developer switch (A/B runs, tests; an ADDITION within TGS_VERSION 320): which kernels a gradient call of the two above runs.
 *     0 = two kernels with the adjoint planes in scratch; 1 = one pass on that kernel's own grid (54-column strips; scratch
 *     is not touched, the workgroup sums differ from form 0 by summation order); 2 = one pass on the grid of form 0 (scratch
 *     is not touched, block_partials bit-identical to form 0); 3 = the default: form 2 from 1920 x 1080 pixels on, form 0
 *     below.  v_img is bit-identical in all of them.  Environment TGS_SSIM_FUSED (read once at first use), a negative
 *     argument leaves the setting; returns the form in force.  PROCESS-WIDE, like tgs_set_raster_variant. */
int tgs_set_ssim_form(int form);

/* Scale-invariant monocular depth loss  L = weight * (1 - rho)  (an ADDITION within TGS_VERSION 320: no struct and no earlier
 *     signature changes; csrc/depthcorr.hip).  rho = the Pearson correlation, over the VALID pixels, of the expected depth
 *     x = out_depth / alpha, alpha = max(1 - final_T, 1e-10)  (out_depth, final_T: tgs_rasterize_fwd's outputs) and a raw
 *     monocular depth map y = mono of any positive scale and any shift.  A pixel is valid iff mono > 0 and
 *     (1.0f - final_T) >= alpha_min, compared in fp32; alpha_min in (0, 1].  Over the valid pixels: n = count, mx, my = means,
 *     vx, vy, c = centred second moments / n, rho = c / sqrt(vx vy), beta = c / vx and
 *         g_i = -weight * d rho / d x_i = -weight / (n sqrt(vx vy)) * ((y_i - my) - beta (x_i - mx)).
 * out: stats[8] = {n, mx, my, vx, vy, c, rho, weight * (1 - rho)};
 *      v_depth[H,W] = g / alpha and v_alpha[H,W] = -g x / alpha (the gradient with respect to 1 - final_T): the upstream images
 *      tgs_rasterize_bwd takes, which adds its own fused terms on top.  0 on invalid pixels; every pixel is written.  Either
 *      may be NULL; both NULL = forward only (two launches instead of three).
 * tmp: tile_moments[tgs_num_tiles * 8] floats.  stats and tile_moments are 16-byte aligned.
 * A DEGENERATE frame -- n < 2, or vx vy (of the fp32 values in stats) not > 0 or not finite -- has rho = 0, loss 0 and all
 * gradients 0; stats[0..5] are still written, nothing is NaN.  No float atomics: the same inputs give the same bits. */
int tgs_depth_corr_fwd_bwd(int W, int H, const float* out_depth, const float* final_T, const float* mono,
                           float alpha_min, float weight, float* tile_moments, float* stats,
                           float* v_depth /*may be NULL*/, float* v_alpha /*may be NULL*/, void* stream);

/* The same loss with a PATCH-WISE (local) term beside the global one (an ADDITION within TGS_VERSION 320):
 *         L = weight_global * (1 - rho) + weight_local * (1 - rho_bar),   rho_bar = mean of rho_p over the ACTIVE patches.
 *     Pixels, x, y, alpha and validity as above.  A patch is patch_tiles x patch_tiles (1...16) tiles of 16 x 16 pixels on a
 *     grid whose origin is shifted by (off_x, off_y) tiles, 0 <= off < patch_tiles: tile (tx, ty) belongs to patch
 *     ((tx + off_x) / patch_tiles, (ty + off_y) / patch_tiles), PW = ceil((TW + off_x) / patch_tiles) patches per row, PH
 *     likewise; border patches are partial.  Per patch, over its valid pixels: n_p, means, vx_p, vy_p, c_p (centred, / n_p),
 *     rho_p = c_p / sqrt(vx_p vy_p), beta_p = c_p / vx_p.  A patch is ACTIVE iff n_p >= min_count, vx_p >= min_var_ratio * vx and
 *     vy_p >= min_var_ratio * vy (vx, vy: the global variances stats[3], stats[4]), vx_p vy_p > 0 and finite, and the
 *     global frame is not degenerate.  The gates are constants of the gradient, as validity is:
 *         g_i = g_glob,i - (weight_local / A) ((y_i - my_p) - beta_p (x_i - mx_p)) / (n_p sqrt(vx_p vy_p))   on an active patch,
 *     A = the number of active patches; with A = 0 the local loss and its gradient are 0.
 * out: stats[16] = {[0..7] as tgs_depth_corr_fwd_bwd with weight = weight_global, bit for bit; [8] patches with
 *      n_p >= min_count; [9] A; [10] rho_bar; [11] weight_local * (1 - rho_bar); [12] = [7] + [11]; [13..15] 0};
 *      patch_stats[PW * PH * 8] = per patch {active (1 / 0), mx_p, my_p, beta_p, 1 / (n_p sqrt(vx_p vy_p)), rho_p, n_p,
 *      n_p >= min_count (1 / 0)}, beta / the scale / rho 0 on an inactive patch;  v_depth, v_alpha as above (both NULL =
 *      forward only: four launches instead of five).
 * tmp: tile_moments[tgs_num_tiles * 8] floats.  tile_moments, patch_stats and stats are 16-byte aligned.
 * min_count >= 2; min_var_ratio >= 0 and finite.  No float atomics: the same inputs give the same bits. */
int tgs_depth_corr_local_fwd_bwd(int W, int H, const float* out_depth, const float* final_T, const float* mono,
                                 float alpha_min, float weight_global, float weight_local, int patch_tiles, int off_x,
                                 int off_y, int min_count, float min_var_ratio, float* tile_moments, float* patch_stats,
                                 float* stats /*[16]*/, float* v_depth /*may be NULL*/, float* v_alpha /*may be NULL*/,
                                 void* stream);

/* Surface normals from the rendered depth, and the normal-prior loss (an ADDITION within TGS_VERSION 320: no struct and no
 *     earlier signature changes; csrc/depthnormal.hip).
 * in:  out_depth, final_T [H,W]: tgs_rasterize_fwd's outputs (out_depth is not divided by alpha); prior [H,W,3]: normals in
 *      OpenCV camera axes, any length, length 0 = no supervision there (NULL = none anywhere); conf [H,W] or NULL: weights
 *      >= 0 (NULL = 1 everywhere); cam: fx, fy, cx, cy, pix_center, W, H are read.
 * Per pixel:  a = 1.0f - final_T in fp32; the pixel is VALID iff a >= alpha_min, compared in fp32 on the stored bits as in
 *     tgs_depth_corr_fwd_bwd; alpha = max(a, 1e-10), x = out_depth / alpha; ray r(px, py) = ((px + pix_center - cx) / fx,
 *     (py + pix_center - cy) / fy, 1); point P = x r.
 * Centre i is FORMED iff it is an interior pixel (0 < px < W - 1, 0 < py < H - 1), it and its four neighbours l, r, u, d
 *     are valid, max(|x_r - x_l|, |x_d - x_u|) <= max_jump * x_i in fp32 (the depth-discontinuity gate; max_jump <= 0
 *     switches it off), and, with t_x = P_r - P_l, t_y = P_d - P_u, m = t_y x t_x, |m| > 0 and finite (decided on |m|^2 in
 *     fp32, which must be a normal number: lengths from 1.1e-19 to 1.8e19).  n = m / |m|: a fronto-parallel plane gives
 *     (0, 0, -1), the normal faces the camera.
 * Centre i is SUPERVISED iff it is formed, |prior_i| > 0 and finite (on |prior_i|^2 in fp32, likewise) and c_i > 0.  p^ = prior / |prior|,
 *     C = sum of c_i over the supervised centres,   L = weight * sum c_i (1 - n_i . p^_i) / C.
 * Gradient (validity, the gates and C are constants of it): on a supervised centre k
 *         g_n = -(weight c_k / C) p^_k,  g_m = (g_n - (g_n . n) n) / |m|,  g_tx = g_m x t_y,  g_ty = t_x x g_m    (0 elsewhere)
 *     and for a pixel j   G_j = r_j . (g_tx(left neighbour of j) - g_tx(right) + g_ty(upper) - g_ty(lower)).
 * out: stats[8] = {formed centres, supervised centres, C, sum c (1 - cos) / C, weight * [3], 0, 0, 0};
 *      normals[H,W,3] (may be NULL) = n on formed centres and exactly 0 elsewhere;
 *      v_depth[H,W] = G / alpha and v_alpha[H,W] = -G x / alpha (the gradient with respect to 1 - final_T): the upstream images
 *      tgs_rasterize_bwd takes.  Every pixel is written.  Either may be NULL; both NULL = forward only (two launches
 *      instead of three).  accumulate = 1: out = old + value, value = the bits the call with accumulate = 0 writes -- the
 *      term stacks on the images tgs_depth_corr_fwd_bwd wrote without an add of its own; the caller orders the two calls
 *      on one stream.
 * tmp: tile_sums[tgs_num_tiles * 4] floats.  stats and tile_sums are 16-byte aligned; the images need no alignment.
 * No supervised centre: loss 0, all gradients 0, nothing NaN.  No float atomics: the same inputs give the same bits.
 * Accuracy: |n - n_ref| and G are held to 16 units of kappa_i 2^-24 resp. S_j 2^-24 (the condition numbers of the
 * differences t_x, t_y; tests/depth_normal_ref.py, tests/test_gpu_depth_normal.py). */
int tgs_depth_normal_fwd_bwd(const TgsCamera* cam, const float* out_depth, const float* final_T,
                             const float* prior /*may be NULL*/, const float* conf /*may be NULL*/, float alpha_min,
                             float max_jump, float weight, float* tile_sums, float* stats /*[8]*/,
                             float* normals /*may be NULL*/, float* v_depth /*may be NULL*/, float* v_alpha /*may be NULL*/,
                             int accumulate, void* stream);

/* Per-view exposure compensation  C' = A C + b  (an ADDITION within TGS_VERSION 320: no struct and no earlier signature
 *     changes; csrc/exposure.hip).  E = [A | b] is row-major 3x4 in DEVICE memory, the identity = no change;
 *     rgb [H,W,3] is tgs_rasterize_fwd's out_rgb (background included); there is no clamp.
 * tgs_exposure_fwd: rgb_out[p][c] = sum_k A[c][k] rgb[p][k] + b[c].  One launch.
 * tgs_exposure_bwd: the RGB loss is taken on C' (recomputed here with the forward's bits, not read):
 *         v'[p][c] = v_img[p][c] + l1_weight * sign(C'[p][c] - gt[p][c]),  sign(0) = 0   (tgs_rasterize_bwd's fused L1 term);
 *     gt NULL = no L1 term, v_img NULL = no upstream image (e.g. SSIM's gradient with respect to C'), both NULL = zeros.
 *     v_rgb[p][k] = sum_c A[c][k] v'[p][c]: the upstream image tgs_rasterize_bwd takes, with TgsLossSpec.gt_rgb = NULL.
 *     out[TGS_EXPO_OUT]: [0..11] G = dL/dE row-major 3x4, G_A[c][k] = sum_p v'[p][c] rgb[p][k], G_b[c] = sum_p v'[p][c];
 *         [12..23] per entry the sum of the absolute values of those products (the unit of its rounding error);
 *         [24] 1 = valid, 0 = the frame was void (guard[1] != 0: everything else is 0 too, `state` keeps every bit);
 *         [25] l1_weight * sum |C' - gt|;  [26] W * H;  [27..31] 0.
 *     partials[tgs_exposure_num_partials(W, H), TGS_EXPO_OUT]: scratch, one row per workgroup; overwritten.
 *     state[TGS_EXPO_STATE] or NULL (gradient only): one view's optimizer row {[0..11] E, [12..23] exp_avg, [24..35]
 *         exp_avg_sq, [36] steps taken t, [37] beta1^t, [38] beta2^t (running products; 1 at t = 0), [39..47] 0}.  On a valid frame
 *         g = G + l2 (E - I), t and the products advance, and the 12 entries take one Adam step (the update of
 *         tgs_adam_step) with the bias corrections 1 - state[37], 1 - state[38].  expo may be state itself: the row is written
 *         by the last launch only.
 *     Three launches in all, no float atomics: the same inputs give the same bits.  No host synchronisation. */
#define TGS_EXPO_OUT   32   /* floats of the result */
#define TGS_EXPO_STATE 48   /* floats of one view's state row */
int tgs_exposure_num_partials(int W, int H);   /* workgroup rows of the scratch; a function of W, H alone */
int tgs_exposure_fwd(int W, int H, const float* rgb, const float* expo /*device [12]*/, float* rgb_out, void* stream);
int tgs_exposure_bwd(int W, int H, const float* rgb, const float* expo /*device [12]*/,
                     const float* gt /*may be NULL*/, float l1_weight, const float* v_img /*may be NULL*/,
                     float* v_rgb, float* partials /*[num_partials, 32]*/, float* out /*[32]*/,
                     const int32_t* guard /*may be NULL*/, float* state /*[48] or NULL = gradient only*/,
                     float lr, float beta1, float beta2, float eps, float l2, void* stream);

/* A Gaussian-process implicit surface (GPIS) ray-marched into one view: touch depth, posterior variance and surface normal
 *     (an ADDITION within TGS_VERSION 320: a new struct and a new call, nothing earlier changes; csrc/gpis.hip).
 *     The device form of touch_gs_amd.gpis.GPIS.render_depth, which stays the definition.
 * ALL coordinates (X, P, view->t) are CENTRED on the centroid of P by the caller, in fp64, before they are rounded to fp32.
 * in:  X [n,4] = {x, y, z, alpha}: the GP's points and weights (16-byte aligned); P, N [n_p,3]: the touched points and their
 *      outward unit normals; Kinv [n,n] fp64 = (K + noise I)^-1, NULL = no variance wanted (var, if given, is all NaN and
 *      max_var must be negative); l, sf2, prior: length scale, signal variance, the "far outside" prior mean.
 * view: the camera -- R = its OpenCV axes in the world, row-major (row = world axis, column = camera axis: a world direction
 *      is R d_cam), t = its centred position, fx, fy, cx, cy, W, H; pixel (u, v) looks along ((u + 0.5 - cx) / fx,
 *      (v + 0.5 - cy) / fy, 1) --, the region of interest u0 <= u <= u1, v0 <= v <= v1 (inside the image) of which every
 *      stride-th pixel from (u0, v0) is rendered, and the march: samples z_k = z_lo + k dz, k < n_steps (2 ... 512), of the
 *      camera-space depth; max_var < 0 = no cut; var_floor.
 * Per rendered ray:  m(q) = sum_j alpha_j k_j + prior (1 - max_j k_j / sf2),  k_j = sf2 exp(-|q - x_j|^2 / 2 l^2), in fp32, the
 *      squared distance as a sum of squared differences.  The first k >= 1 with m(z_{k-1}) > 0 and m(z_k) <= 0 brackets the
 *      crossing; 12 bisection rounds; z = the last bracket's midpoint.  The crossing counts iff the outward normal of the touched
 *      point nearest to it (brute force, lowest index on ties) has N . ray / |ray| < -0.05, and, with max_var >= 0, iff
 *      var <= max_var, where  var = max(sf2 - k^T Kinv k, 0)  (k in fp32, widened; fp64 accumulation in a fixed order).
 * out: depth [H,W] = z, var [H,W] = max(var, var_floor) on the counted crossings, NaN on every other pixel of the image;
 *      normal [H,W,3] (may be NULL) = grad m / |grad m| at the crossing, rotated into the camera's OpenCV axes (not flipped:
 *      m grows outwards), exactly 0 elsewhere;  grad m = sum_j alpha_j k_j (x_j - q) / l^2 - prior k_J (x_J - q) / (l^2 sf2),
 *      J = argmax_j k_j (lowest index on ties).
 * tmp: hits [1 + rays] int32, rays = ((u1 - u0) / stride + 1) ((v1 - v0) / stride + 1): the crossings, compacted through an
 *      integer counter; their order reaches no output.
 * Three launches (fill, march, variance; two without Kinv).  No float atomics: every output is a function of its own pixel
 * alone and comes out the same bits on every call.  Accuracy against the fp64 reference: tests/test_gpu_gpis.py. */
typedef struct TgsGpisView {
  float R[9];
  float t[3];
  float fx, fy, cx, cy;
  int32_t W, H;
  int32_t u0, v0, u1, v1, stride;
  float z_lo, dz;
  int32_t n_steps;
  float max_var, var_floor;
} TgsGpisView;
int tgs_gpis_render(int n, const float* X, int n_p, const float* P, const float* N, const double* Kinv /*may be NULL*/,
                    float l, float sf2, float prior, const TgsGpisView* view, float* depth, float* var /*may be NULL*/,
                    float* normal /*may be NULL*/, int32_t* hits, void* stream);

/* TSDF fusion of depth images into a voxel grid, and the grid's zero crossings as an oriented, coloured point cloud
 *     (an ADDITION within TGS_VERSION 320: a new struct and three new calls, nothing earlier changes; csrc/tsdf.hip,
 *     DESIGN 5.1k).  The definition is tests/tsdf_ref.py (fp64 NumPy); touch_gs_amd.tsdf.TsdfVolume is the caller.
 * GRID: nx x ny x nz voxels of side vox, x fastest in memory (voxel (i, j, k) at i + nx (j + ny k)), at most 2^29 - 1 of
 *      them.  Voxel (i, j, k) has its centre at ((i + 1/2) vox, (j + 1/2) vox, (k + 1/2) vox) in GRID-LOCAL coordinates, formed
 *      in fp32 from the indices themselves.  The grid's world origin never reaches the device: the caller forms each view's
 *      R (world -> camera, OpenCV axes, row-major) and t' = R origin + t in fp64 and rounds them once (the re-centring of
 *      tgs_gpis_render), so a scene far from the world origin loses no digits.
 * STATE: sums, not a running average, all fp32:  S [V] = sum w d,  Wt [V] = sum w,  C [V,3] = sum w rgb (may be NULL).  The
 *      TSDF value is f = S / Wt.  The caller zeroes them once; each call adds to them.
 * tgs_tsdf_integrate: 1 <= n_views <= 8 views per launch, `views` a HOST array (the structs travel as kernel arguments).
 *      A view: R, t (= t' above), fx, fy, cx, cy, W, H, near_plane, pix_center (pixel (x, y) has its centre at
 *      (x + pix_center, y + pix_center), as TgsCamera), and three DEVICE pointers: depth [H,W], weight [H,W] or NULL (= 1
 *      everywhere), rgb [H,W,3] or NULL (the view adds no colour).  The depth is CAMERA-SPACE z, what the rasterizer renders:
 *      K1 stores a Gaussian's depth as  R[6..8] . mean + t[2]  (csrc/project.hip, geom_eval: G.tz, splat slot 2) and K6
 *      composites that, so depth_acc / alpha -- and the median depth, which is one Gaussian's -- is z, not the distance
 *      along the ray.
 *      For each voxel, and each view in array order, with c the voxel's centre:
 *        p = R c + t;                                         skip the view if p.z <= near_plane
 *        u = fx p.x / p.z + cx,  v = fy p.y / p.z + cy;       pixel = (floor(u + 1/2 - pix_center), floor(v + 1/2 - pix_center)):
 *                                                             the NEAREST pixel, no interpolation across depth edges;
 *                                                             skip if it lies outside the image
 *        D = depth[pixel];                                    skip unless D is finite and > 0
 *        w = weight[pixel] (1 if NULL);                       skip unless w is finite and > 0
 *        sdf = D - p.z;                                       skip if sdf < -trunc
 *        d = min(sdf / trunc, 1);  S += w d;  Wt += w;  C += w rgb[pixel]
 *      Every product and sum rounds on its own (no contraction), in the order written.  One launch; every voxel is read and
 *      written once by the one lane that owns it, whatever n_views is: no atomics, and the sequence of fp32 operations on a
 *      voxel is the same whether eight views arrive in one call or in eight -- batching cannot be seen in the bits.
 * tgs_tsdf_extract_count: a voxel is VALID iff Wt >= w_min (w_min > 0).  For voxel a and its +x, +y, +z neighbour b the edge
 *      is a CROSSING iff both are valid and (f_a < 0) != (f_b < 0).  counts [V] int32 = the crossings of a, 0 ... 3.
 * tgs_tsdf_extract_points: offsets [V] int64 = the exclusive prefix sum of counts (the caller's; the rows must hold its
 *      total).  Crossing m of voxel a, in axis order, lands in row offsets[a] + m: the output order is a function of the grid
 *      alone.  Per crossing on axis k:
 *        t = f_a / (f_a - f_b)                                (the ends differ in sign: no cancellation)
 *        point  = centre_a + t vox e_k                        grid-local, fp32
 *        g(v)_m = central difference of f along axis m where both neighbours of v are valid, one-sided where exactly one
 *                 is, 0 otherwise (a voxel outside the grid is not valid)
 *        normal = normalize((1 - t) g(a) + t g(b)),           exactly 0 if that length is 0 or not finite; OUTWARD, because f
 *                                                             grows towards the observer
 *        colour = (1 - t) C_a / Wt_a + t C_b / Wt_b           (colors may be NULL; needs C)
 *        edge_id = 3 a + k, int64                             (may be NULL)
 *      points, normals, colors [total,3] fp32.
 * Every argument is checked before any launch (TGS_E_ARG and a tgs_last_error text): NULL required pointers, n_views outside
 * 1 ... 8, non-positive dims, vox, trunc or w_min, a view without depth or with a bad size / intrinsics / near plane, more
 * voxels than the 32-bit index holds.  Accuracy against the fp64 reference: tests/test_gpu_tsdf.py. */
typedef struct TgsTsdfView {
  float R[9];
  float t[3];
  float fx, fy, cx, cy;
  int32_t W, H;
  float near_plane, pix_center;
  const float* depth;
  const float* weight;
  const float* rgb;
} TgsTsdfView;
int tgs_tsdf_integrate(int nx, int ny, int nz, float vox, float trunc, float* S, float* Wt, float* C /*may be NULL*/,
                       int n_views, const TgsTsdfView* views, void* stream);
int tgs_tsdf_extract_count(int nx, int ny, int nz, float vox, const float* S, const float* Wt, float w_min, int32_t* counts,
                           void* stream);
int tgs_tsdf_extract_points(int nx, int ny, int nz, float vox, const float* S, const float* Wt, const float* C /*may be NULL*/,
                            float w_min, const int64_t* offsets, float* points, float* normals, float* colors /*may be NULL*/,
                            int64_t* edge_id /*may be NULL*/, void* stream);

/* The TSDF grid's zero level set as a TRIANGLE MESH: marching tetrahedra on the Kuhn (Freudenthal) split of every grid cell
 *     (an ADDITION within TGS_VERSION 320: two new calls, nothing earlier changes; csrc/tsdf.hip).  The
 *     definition is tests/tsdf_mesh_ref.py (fp64 NumPy); TsdfVolume.extract_mesh_local is the caller.  Grid, state, VALID
 *     (Wt >= w_min) and f = S / Wt as above; a voxel is INSIDE iff it is valid and f < 0 (f == 0 is outside).
 * CELL a = (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1: the eight voxel centres a + d, d in {0,1}^3; ACTIVE iff all eight are
 *      valid.  Six TETRAHEDRA per cell, one per permutation pi of (x, y, z) in the order xyz, xzy, yxz, yzx, zxy, zyx, with
 *      the corners 000 -> e_pi1 -> e_pi1 + e_pi2 -> 111; their edges are the corner pairs u <= v componentwise.
 * EDGE (a, e): from voxel a to a + offset(e), e = 0 ... 6: +x, +y, +z, +x+y, +y+z, +x+z, +x+y+z; key 7 a + e.  A VERTEX
 *      exists on it iff both ends are valid, exactly one is inside and an active cell contains the edge.  Its attributes
 *      are those of tgs_tsdf_extract_points with the edge's two ends a, b (one device function serves both):
 *      t = f_a / (f_a - f_b);  point_m = centre_a[m] + t vox where the offset has a 1 in m, centre_a[m] elsewhere;
 *      normal = normalize((1 - t) g(a) + t g(b)), exactly 0 if the length is 0 or not finite;  colour = (1 - t) C_a / Wt_a
 *      + t C_b / Wt_b.
 * FACES: per active cell and tetrahedron the 4-bit inside mask (bit q = corner q) selects 0, 1 or 2 triangles from a
 *      16-entry table that depends on the mask and on the permutation's parity alone (the quad's diagonal included),
 *      counter-clockwise seen from the outside (from larger f).  Degenerate triangles (a corner with f == 0: t = 0) are kept.
 * ORDER: vertices in key order, faces in (cell, tetrahedron, table) order: functions of the grid alone.  The index of the
 *      vertex on edge (a', e') is vert_offsets[a'] + popcount(vmask[a'] & ((1 << e') - 1)).
 * tgs_tsdf_mesh_count (three launches, a lane per voxel): flags [V] u8 (scratch that tgs_tsdf_mesh_emit reads again: bit 0
 *      valid, bit 1 inside), ntri [V] u8 = the triangles of cell a (0 ... 12; 0 where there is no such cell), vmask [V] u8 =
 *      the 7-bit mask of the vertices voxel a owns.  A grid with a dimension of 1 has no cells: all zeros.
 * tgs_tsdf_mesh_emit (one launch): vert_offsets, tri_offsets [V] int64 = the caller's exclusive prefix sums of
 *      popcount(vmask) and ntri; points, normals, colors (may be NULL; needs C) [n_vertices,3] fp32, edge_key [n_vertices]
 *      int64 (may be NULL), faces [n_triangles,3] int32.  flags and vmask must be those the count wrote for the same state
 *      and w_min.  No atomics; no order between lanes reaches an output.
 * Every argument is checked before any launch, as above.  Accuracy and equality against the reference:
 * tests/test_gpu_tsdf_mesh.py. */
int tgs_tsdf_mesh_count(int nx, int ny, int nz, float vox, const float* S, const float* Wt, float w_min, uint8_t* vmask,
                        uint8_t* ntri, uint8_t* flags, void* stream);
int tgs_tsdf_mesh_emit(int nx, int ny, int nz, float vox, const float* S, const float* Wt, const float* C /*may be NULL*/,
                       float w_min, const uint8_t* flags, const uint8_t* vmask, const int64_t* vert_offsets,
                       const int64_t* tri_offsets, float* points, float* normals, float* colors /*may be NULL*/,
                       int64_t* edge_key /*may be NULL*/, int32_t* faces, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Exact k nearest neighbours of 3-D points (csrc/knn.hip): the counterpart of the INRIA trainer's
 * simple_knn.distCUDA2 (touch_gs_amd.simple_knn), the initial scales of touch_gs_amd.train.init_params(knn="hip") and the
 * Chamfer / F-score of touch_gs_amd.tsdf.surface_metrics(device=...).  Additions within 320.  The library allocates nothing,
 * never syncs and uses no atomics; between the calls the CALLER finds the bounds and sorts the keys (touch_gs_amd.ops.knn:
 * amin / amax and one torch.sort).
 * DEFINITION.  d2(q, r) = (dx*dx + dy*dy) + dz*dz with dx = qx - rx, dy = qy - ry, dz = qz - rz, every operation rounded to
 *      fp32 on its own (no fused multiply-add).  Row q of dist2 holds the k smallest d2 over the eligible references in ascending
 *      order, equal d2 ordered by the lower ORIGINAL reference index; idx holds the original indices.  With fewer than k
 *      eligible references the trailing slots are +inf / -1.  So the result depends on neither the sort, the box size nor the
 *      launch shape, and repeats bit for bit.  Non-finite coordinates are the caller's to refuse (a NaN distance never enters).
 * tgs_knn_keys: keys[i] = the 30-bit Morton key of point i quantised to 1024^3 inside [lo, hi] (HOST floats [3]; bit 3 j + a =
 *      bit j of axis a's cell).  Points outside are clamped; an axis with hi == lo quantises to 0 (nothing is divided by zero).
 * tgs_knn_build: order [n] int32 = a permutation that sorts the keys (any permutation gives the same neighbours, a sorted one
 *      gives the speed); sorted_pts [n,4] = {x, y, z, original index bits} in that order; boxes [ceil(n / TGS_KNN_BOX), 8] =
 *      {min x y z, 0, max x y z, 0} of each run of TGS_KNN_BOX consecutive sorted points.
 * tgs_knn_query: thread t serves query q_order[t] (int32 [n_q], a permutation; NULL = t), so that the 64 lanes of a wave are
 *      spatial neighbours; rows of dist2 / idx [n_q,k] are the queries' own.  exclude_self != 0: the queries ARE the
 *      references in their ORIGINAL order (n_q == n_ref) and the reference whose original index equals the query's index is
 *      skipped -- by index, not by distance: duplicates of a point are its neighbours at distance 0.
 * Every argument is checked before any launch (TGS_E_ARG: n, n_q, n_ref < 1 or > 2^29 - 1; k outside 1 .. TGS_KNN_MAX_K; null
 * pointers; non-finite or inverted lo / hi; exclude_self with n_q != n_ref).  Equality with the brute-force reference:
 * tests/test_gpu_knn.py. */
#define TGS_KNN_MAX_K 16
#define TGS_KNN_BOX   256      /* reference points per box: one 4 KB LDS stage of a wave, four per lane; DESIGN 5.1p */
int tgs_knn_keys(int n, const float* pts /*[n,3]*/, const float* lo /*[host][3]*/, const float* hi /*[host][3]*/,
                 uint32_t* keys /*[n]*/, void* stream);
int tgs_knn_build(int n, const float* pts /*[n,3]*/, const int32_t* order /*[n]*/, float* sorted_pts /*[n,4]*/,
                  float* boxes /*[ceil(n/TGS_KNN_BOX),8]*/, void* stream);
int tgs_knn_query(int n_q, const float* queries /*[n_q,3]*/, const int32_t* q_order /*[n_q], may be NULL*/, int n_ref,
                  const float* sorted_pts, const float* boxes, int k, int exclude_self, float* dist2 /*[n_q,k]*/,
                  int32_t* idx /*[n_q,k]*/, void* stream);

/* Per-view bilateral grid: spatially varying colour correction  C'[p] = A(p) C[p] + b(p)  (an ADDITION within TGS_VERSION
 *     320: no struct and no earlier signature changes; csrc/bilagrid.hip).  The grid of one view is
 *     g[GH][GW][L][12] float32 in DEVICE memory, the last axis a row-major 3x4 [A | b]; every dimension >= 2 (GW, GH <= 4096,
 *     L <= 64); the identity everywhere = no change.  rgb [H,W,3] is tgs_rasterize_fwd's out_rgb; there is no clamp.
 * COORDINATES of pixel (px, py) with colour C, every operation rounded to fp32 on its own, in this order:
 *         gx = (float(px) + 0.5f) * sx,  sx = float(GW-1) / float(W);  gy likewise;
 *         luma = (0.299f r + 0.587f g) + 0.114f b;  z = min(max(luma, 0), 1) * float(L-1);
 *         ix = min(int(gx), GW-2), fx = gx - float(ix);  iy, fy and iz, fz likewise;  inside = luma > 0 && luma < 1.
 * tgs_bilagrid_fwd: A(p) = the trilinear blend of the 8 corners in lerp form a + f (b - a): along x, then y (giving A0, A1 at
 *     the levels iz, iz + 1), then z;  rgb_out[p][c] = ((A[c][0] r + A[c][1] g) + A[c][2] b) + A[c][3].  One launch.
 * tgs_bilagrid_bwd: the RGB loss is taken on C' (recomputed here with the forward's bits, not read):
 *         v'[p][c] = v_img[p][c] + l1_weight * sign(C'[p][c] - gt[p][c]),  sign(0) = 0;
 *     gt NULL = no L1 term, v_img NULL = no upstream image, both NULL = zeros (the conventions of tgs_exposure_bwd).
 *     v_rgb[p][k] = sum_c A[c][k] v'[p][c] + wl[k] (L-1) inside sum_c v'[p][c] ((A1 - A0) C1)[c],  C1 = (C, 1), wl the luma
 *         weights: the upstream image tgs_rasterize_bwd takes, with TgsLossSpec.gt_rgb = NULL.
 *     grad [2][n] or NULL, n = GH GW L 12: G[v][c][k] = sum_p w_v(p) v'[p][c] C1[p][k] (w_v the trilinear weight of vertex v,
 *         zero outside the pixel's cell), then per entry the sum of the absolute values of those products (the masses).
 *     out[TGS_BILAGRID_OUT]: [0] 1 = valid, 0 = the frame was void (guard[1] != 0: everything else is 0 too, `state` keeps
 *         every bit; v_rgb is still written); [1] l1_weight * sum |C' - gt|; [2] W * H; [3] TV(g), unweighted; [4..7] 0.
 *         TV(g) = sum over the axes x, y, z of (1 / n_axis) sum (g[next] - g[this])^2 over all 12 channels, n_axis the
 *         number of differences along the axis (gsplat's total_variation_loss of one grid).
 *     scratch[tgs_bilagrid_scratch_floats(...)]: tgs_bilagrid_num_partials(...) rows of tgs_bilagrid_row_floats(L) floats,
 *         one per workgroup, then the staged gradient and the value partials; overwritten.
 *     state[3 n + TGS_BILAGRID_TAIL] or NULL (gradient only): one view's optimizer row {[0,n) grid, [n,2n) exp_avg, [2n,3n)
 *         exp_avg_sq, [3n] steps taken t, [3n+1] beta1^t, [3n+2] beta2^t (running products; 1 at t = 0), then zeros}.  On a
 *         valid frame grad = G + tv_weight dTV/dg with dTV read from the grid BEFORE the step, t and the products advance,
 *         and every entry takes one Adam step (the update of tgs_adam_step) with the bias corrections from the products.
 *         grid may be state itself: the row is written by the last launch only.
 *     Three launches, no float atomics: the shape of every sum depends on (W, H, GW, GH, L) alone, the same inputs give the
 *     same bits.  No host synchronisation.  Every argument is checked before any launch (TGS_E_ARG). */
#define TGS_BILAGRID_OUT  8    /* floats of the result */
#define TGS_BILAGRID_TAIL 16   /* floats behind the 3 n entries of one view's state row */
int tgs_bilagrid_num_partials(int W, int H, int GW, int GH, int L);      /* rows of the scratch; 0 = bad dimensions */
size_t tgs_bilagrid_row_floats(int L);                                   /* floats of one such row: 4 L 24 + 8 */
size_t tgs_bilagrid_scratch_floats(int W, int H, int GW, int GH, int L); /* floats of the whole scratch */
int tgs_bilagrid_fwd(int W, int H, int GW, int GH, int L, const float* rgb, const float* grid, float* rgb_out, void* stream);
int tgs_bilagrid_bwd(int W, int H, int GW, int GH, int L, const float* rgb, const float* grid,
                     const float* gt /*may be NULL*/, float l1_weight, const float* v_img /*may be NULL*/, float tv_weight,
                     float* v_rgb, float* scratch, float* grad /*[2][n], may be NULL*/, float* out /*[8]*/,
                     const int32_t* guard /*may be NULL*/, float* state /*[3n+16] or NULL = gradient only*/,
                     float lr, float beta1, float beta2, float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Peer exchange: the data-parallel gradient exchange by direct stores into IPC-mapped peer memory (all 7 xGMI
 * links of a rank at once, no collective launch) -- the alternative to RCCL that touch_gs_amd.parallel selects
 * with TGS_DP_TRANSPORT=ipc (csrc/peer.hip).  The reference has no counterpart (single GPU).
 * tgs_peer_alloc: `bytes` of zeroed device memory of the first kind in `allow_kinds` (a mask of TGS_PEER_MEM_*, tried
 *     in the order uncached, fine-grained, plain) the driver grants + its 64-byte IPC handle (send it to the other
 *     processes by any means); *kind_out (may be NULL) = the kind obtained; TGS_E_HIP if none of the allowed kinds
 *     could be had -- there is no silent downgrade.  The transport's ordering argument (csrc/peer.hip) holds for
 *     uncached and fine-grained memory only: touch_gs_amd.parallel.PeerExchange asks for exactly those.
 *     tgs_peer_open maps another process's buffer; _close / _free undo them.
 * Flags are int32 words inside such buffers; `seq` must grow from call to call (compared as seq - flag <= 0);
 * `ticket` = a zeroed device int32 private to each (call site, stream).
 * tgs_peer_push:        src[0, bytes) -> dsts[i][0, bytes) for i < n_dst, then flags[i] = seq (release, system scope)
 * tgs_peer_scatter:     src[q * slice_bytes, ...) -> dsts[q][0, ...) for q < n_dst, then flags
 * tgs_peer_reduce_push: sum over r < world of srcs[r] in rank order -> every dsts[i], then flags
 * tgs_peer_wait:        the stream waits until all n flags (local memory) have reached seq; after timeout_s
 *     seconds (<= 0: 20 s) it gives up, sets *err = 1 + index of the missing flag and, if given, *poison_a = *poison_b = 1
 *     (device int32 words, may be NULL): hand it the sticky overflow word and word [1] of the verdict the optimizer
 *     kernels are guarded by (tgs_dp_agree_overflow ORs the sticky word in) and nothing behind a timed-out wait
 *     touches the model; the host reads *err with its per-step status copy.
 * All pointer arrays are HOST arrays of device pointers; at most 8 receivers; sizes and pointers are multiples of
 * 16 bytes (tgs_peer_push also takes multiples of 4 bytes, on a slower scalar path). */
#define TGS_PEER_MEM_UNCACHED 1     /* hipDeviceMallocUncached: peers' stores land in HBM behind the owner's L2 */
#define TGS_PEER_MEM_FINEGRAINED 2  /* hipDeviceMallocFinegrained: coherent at system scope */
#define TGS_PEER_MEM_PLAIN 4        /* hipMalloc: cached; the owner may read stale lines -- not used by PeerExchange */
int tgs_peer_alloc(size_t bytes, int allow_kinds, void** dptr, unsigned char* handle64, int* kind_out /*may be NULL*/);
int tgs_peer_open(const unsigned char* handle64, void** dptr);
int tgs_peer_close(void* dptr);
int tgs_peer_free(void* dptr);
int tgs_peer_push(int n_dst, void* const* dsts, int32_t* const* flags, const void* src, size_t bytes,
                  int32_t seq, int32_t* ticket, void* stream);
int tgs_peer_scatter(int n_dst, void* const* dsts, int32_t* const* flags, const void* src,
                     size_t slice_bytes, size_t total_bytes, int32_t seq, int32_t* ticket, void* stream);
int tgs_peer_reduce_push(int world, const void* const* srcs, int n_dst, void* const* dsts,
                         int32_t* const* flags, size_t bytes, int32_t seq, int32_t* ticket, void* stream);
 /* tgs_peer_signal: flags[i] = seq (release, system scope) as a launch of its own -- the conservative way to publish
 *     after a push / scatter / reduce_push that was given flags = NULL (the kernel boundary orders the data). */
int tgs_peer_signal(int n, int32_t* const* flags, int32_t seq, void* stream);
int tgs_peer_wait(int n, const int32_t* const* flags, int32_t seq, int32_t* err, float timeout_s,
                  int32_t* poison_a /*may be NULL*/, int32_t* poison_b /*may be NULL*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TGS_H */
