/*
 * dnsplat.h — C ABI of libdnsplat.so, the MI355X (gfx950) renderer that drops in
 * behind dn-splatter's DNSplatterModel.get_outputs().
 *
 * What it replaces.  The reference has no native code; its hot path is two calls
 * into the third-party CUDA package gsplat==1.0.0 (reference pin pyproject.toml:8):
 *   - gsplat.rendering.rasterization(...)   dn_splatter/dn_model.py:495-516
 *   - gsplat.rasterize_gaussians(...)       dn_splatter/dn_model.py:564-575
 * plus two helpers (dn_model.py:34-35).  The entry points below are the stages of
 * those two calls, cut where the reference's own
 * autograd graph is cut so that the Python binding in dn-splatter_amd/ can expose
 * exactly the tensors dn-splatter reads back (means2d incl. .grad/.absgrad, radii,
 * depths, conics, tiles_per_gauss — dn_model.py:517-524).
 *
 * Conventions.
 *   - Every pointer is a DEVICE pointer owned by the caller unless its name ends in
 *     _host.  Structs themselves live in host memory and are read during the call.
 *   - Kernels are enqueued on `stream`; no entry point allocates, frees or
 *     synchronises.  Workspaces are sized by the *_workspace_bytes queries.
 *   - Return value: 0 = ok, <0 = error (dnsplat_strerror).  No exceptions cross the ABI.
 *   - All floats are fp32, row-major, layouts as in the reference tensors:
 *     means[N,3], quats[N,4] (wxyz), scales[N,3], opacities[N], SH coefficients
 *     [N,K,3] (or split band-0 / rest, dn_model.py:466-468), viewmat[4,4] world->camera
 *     OpenCV, K[3,3].  Projection takes one camera per call (dn_model.py:421); binning and compositing also take
 *     batches of cameras (n_cameras).
 *   - The library keeps no global mutable state; calls are re-entrant across streams.
 *
 * Splat record.  Stage 1 packs what the compositing kernels gather per tile
 * intersection into one 64-byte record per Gaussian:
 *     [0]=x [1]=y [2..4]=conic(a,b,c) [5]=opacity [6..13]=up to 8 feature channels [14..15]=0
 * The gradient record written by dnsplat_raster_bwd mirrors it:
 *     [0..1]=v_xy [2..4]=v_conic [5]=v_opacity [6..13]=v_channels [14..15]=|v_xy| (absgrad, A11)
 */
#ifndef DNSPLAT_H
#define DNSPLAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct gains a field, a field changes meaning or an entry point is added; the Python binding refuses a
 * library of another version.  Round 4: 10 = dnsplat_raster_args.det_partials / dnsplat_det_reduce (deterministic gradient
 * scatter), 11 = dnsplat_scale_reg, 12 = dnsplat_proj_grads.sh_factors (the colour-gradient slab written by the projection
 * backward), 13 = dnsplat_proj_out.tile_boxes carries width | height << 16 and dnsplat_bin_args.tile_boxes takes the counts
 * from it.  Round 6: 14 = dnsplat_scene.colors_are_logit (the sh_degree == 0 branch of get_outputs in the fused pass),
 * dnsplat_proj_out.skip_culled_records, dnsplat_proj_grads.sh_grad_scale / sh_zero_state (own-camera SH rows in the exchange step;
 * gradient rows of persistently culled Gaussians are not re-zeroed), dnsplat_sh_grads_add_factors, the packed (visible rows only)
 * colour-gradient slabs: dnsplat_visible_index, dnsplat_proj_grads.sh_packed, dnsplat_sh_grads_from_packed; 15 = dnsplat_ssim (the
 * SSIM term alone, for a loss stack that otherwise stays in PyTorch), dnsplat_proj_grads.zero_state_geometry (zero gradient rows of
 * culled Gaussians skipped per workgroup), dnsplat_edge_aware_logl1, dnsplat_tv_loss.
 * Entry points added after 15 are purely additive — new symbols and new structs, no existing struct or call changes — and are found
 * by symbol: the version stays 15 and the binding refuses a library that lacks one (dnsplat_pose_partial_rows,
 * dnsplat_project_bwd_pose / dnsplat_pose_grads: the camera pose gradient; dnsplat_pearson_depth / dnsplat_pearson_scratch_bytes: the
 * Pearson depth losses; dnsplat_ags_normal_loss / dnsplat_ags_normal_scratch_bytes: the filtered normal loss of the AGS-Mesh strategy;
 * dnsplat_depth_edge_valid / dnsplat_sample_valid_pixels / dnsplat_backproject_points / dnsplat_backproject_args /
 * dnsplat_pointcloud_scratch_bytes: the oriented point cloud of the mesh exporter; dnsplat_eval_metrics / dnsplat_eval_metrics_args /
 * dnsplat_eval_metrics_scratch_bytes: the evaluation scores; dnsplat_knn_grid_dim / dnsplat_knn_index_bytes / dnsplat_knn_build /
 * dnsplat_knn_query / dnsplat_density_pack / dnsplat_density_eval / dnsplat_density_args: the Gaussian density field;
 * dnsplat_level_rays / dnsplat_level_points / dnsplat_level_rays_args / dnsplat_level_points_args: the level-set surface points;
 * dnsplat_mc_scratch_bytes / dnsplat_mc_count / dnsplat_mc_emit / dnsplat_mc_args: marching cubes on a lattice;
 * dnsplat_cloud_distances / dnsplat_cloud_distances_scratch_bytes / dnsplat_cloud_distances_args / dnsplat_mesh_areas /
 * dnsplat_mesh_sample / dnsplat_mesh_sample_args: the geometry scores; dnsplat_mesh_depth / dnsplat_mesh_depth_scratch_bytes /
 * dnsplat_mesh_depth_args / dnsplat_mesh_visibility / dnsplat_mesh_visibility_args / dnsplat_mesh_cut_scratch_bytes /
 * dnsplat_mesh_cut_count / dnsplat_mesh_cut_emit / dnsplat_mesh_cut_args: the mesh visibility culling in front of them;
 * dnsplat_tsdf_integrate / dnsplat_tsdf_args / dnsplat_tsdf_vertex_colors / dnsplat_mc_observed_scratch_bytes /
 * dnsplat_mc_count_observed / dnsplat_mc_emit_observed / dnsplat_mc_observed_args: TSDF fusion and the mesh of what was observed;
 * dnsplat_mesh_clusters / dnsplat_mesh_clusters_scratch_bytes / dnsplat_mesh_clusters_args / dnsplat_mesh_filter_scratch_bytes /
 * dnsplat_mesh_filter_count / dnsplat_mesh_filter_emit / dnsplat_mesh_filter_args: the connected-component filter behind that mesh;
 * dnsplat_cloud_outlier_scratch_bytes / dnsplat_cloud_neighbor_mean / dnsplat_cloud_outlier_stats / dnsplat_cloud_outlier_count /
 * dnsplat_cloud_outlier_emit / dnsplat_cloud_outlier_args / dnsplat_voxel_scratch_bytes / dnsplat_voxel_count / dnsplat_voxel_emit /
 * dnsplat_voxel_args: the point-cloud filters (statistical outlier removal, voxel down-sampling);
 * dnsplat_icp_scratch_bytes / dnsplat_icp_begin / dnsplat_icp_iterate / dnsplat_icp_run / dnsplat_icp_args /
 * dnsplat_transform_points / dnsplat_knn_points: the mesh alignment (point-to-point ICP) in front of the culling;
 * dnsplat_subdivide_scratch_bytes / dnsplat_subdivide_count / dnsplat_subdivide_emit / dnsplat_subdivide_args: the subdivision of
 * long triangles the culling starts with;
 * dnsplat_cloud_normals_scratch_bytes / dnsplat_cloud_normals / dnsplat_cloud_normals_args: the point-cloud normals (exact k-NN PCA);
 * dnsplat_bin_prepare_cells / dnsplat_bin_emit_sort_cells / dnsplat_bin_cells / dnsplat_raster_fwd_cells / dnsplat_raster_bwd_cells /
 * dnsplat_raster_cells / dnsplat_det_reduce_planes: the fused path's tile lists kept per cell of several tiles). */
#define DNSPLAT_ABI_VERSION 15
#define DNSPLAT_RECORD_FLOATS 16
#define DNSPLAT_MAX_CHANNELS 8

/* error codes */
#define DNSPLAT_OK 0
#define DNSPLAT_ERR_INVALID_ARG (-1)
#define DNSPLAT_ERR_WORKSPACE (-2)
#define DNSPLAT_ERR_LAUNCH (-3)
#define DNSPLAT_ERR_UNSUPPORTED (-4)

typedef void *dnsplat_stream_t; /* hipStream_t */

const char *dnsplat_strerror(int code);
int dnsplat_abi_version(void);

/* Appends the device's constant-rate wall clock (s_memrealtime ticks) to ring[(*cursor)++ % ring_size] from a one-thread kernel on
 * `stream`.  Works inside a frame captured into a HIP graph, where events cannot be recorded (ROCm 7.2): bench.py brackets the
 * dominant stage with two stamps per replay and calibrates the tick against HIP events. */
int dnsplat_stamp(uint64_t *ring, uint32_t *cursor, uint32_t ring_size, dnsplat_stream_t stream);

/* ------------------------------------------------------------------ stage 1
 * Fused per-Gaussian front end: activations (A0) + fully-fused projection (A1)
 * + tile count (A2a) + spherical harmonics (A5) + per-Gaussian normal (A7) +
 * record packing.  Replaces gsplat fully_fused_projection / spherical_harmonics
 * and the torch ops at dn_model.py:497-499, 543-560. */
typedef struct dnsplat_scene {
    int32_t N;
    const float *means;     /* [N,3] */
    const float *quats;     /* [N,4] wxyz, any norm (normalised inside, as gsplat does) */
    const float *scales;    /* [N,3] */
    const float *opacities; /* [N] */
    int32_t scales_are_log;       /* 1: apply exp()      (dn_model.py:498) */
    int32_t opacities_are_logit;  /* 1: apply sigmoid()  (dn_model.py:499) */
    /* colour source: SH if sh_degree >= 0, else direct colours */
    int32_t sh_degree;            /* active degree 0..3, or -1 */
    int32_t sh_K;                 /* number of SH bases held in storage (16 for degree-3 models); the
                                     K-1 higher bands live in shN, gradients of inactive bands are 0 */
    const float *sh0;             /* band 0, element g at sh0 + g*sh0_stride, 3 floats   */
    int32_t sh0_stride;
    const float *shN;             /* bands >= 1, element g at shN + g*shN_stride, 3*(K-1) floats */
    int32_t shN_stride;
    const float *colors;          /* direct colours [N, n_colors] when sh_degree < 0 */
    int32_t n_colors;             /* 0..8 */
    int32_t colors_are_logit;     /* 1 (ABI 14; direct colours only): apply sigmoid() — get_outputs with config.sh_degree == 0 feeds
                                     gsplat sigmoid(features_dc) and sh_degree = None (dn_model.py:486-493); the gradient written to
                                     v_colors is then w.r.t. the logits */
} dnsplat_scene;

typedef struct dnsplat_camera {
    const float *viewmat;      /* device [16] world->camera, row-major, OpenCV axes */
    const float *K;            /* device [9] */
    const float *normal_frame; /* device [12] or NULL: rows 0-8 = M with n_cam = M n_world
                                  (dn_model.py:560 `normals @ c2w[:3,:3]` => M = c2w[:3,:3]^T),
                                  9-11 = camera centre used for the facing flip (dn_model.py:550-556) */
    int32_t width, height, tile_size;
    float eps2d, near_plane, far_plane, radius_clip;
    int32_t antialiased;       /* rasterize_mode == "antialiased": opacity *= compensation */
    int32_t tight_tiles;       /* 0: tiles_per_gauss counts gsplat's 3-sigma tile box (A.3, what the drop-in calls return).
                                  1: the box of the part of the splat that can reach alpha >= 1/255 at a pixel centre, clipped
                                  to gsplat's box — shorter tile lists, same images and gradients; for callers that keep the
                                  lists to themselves (the fused get_outputs path).  dnsplat_bin_args.tight_tiles must match. */
} dnsplat_camera;

typedef struct dnsplat_proj_out {
    int32_t *radii;            /* [N] */
    float *means2d;            /* [N,2] */
    float *depths;             /* [N] */
    float *conics;             /* [N,3] */
    float *compensations;      /* [N] or NULL */
    int32_t *tiles_per_gauss;  /* [N] */
    float *splats;             /* [N,16] records, channels = colours | depth | normal */
    float *normals_world;      /* [N,3] or NULL: what dn_model.py:558 stores into gauss_params["normals"] */
    int32_t with_depth_channel;   /* append camera-space depth as a channel (RGB+D / RGB+ED) */
    int32_t with_normal_channels; /* append the 3 camera-frame normal channels (needs camera.normal_frame) */
    uint32_t *saturation_flag;    /* NULL, or a device word the caller zeroed; nonzero afterwards = "the careful compositing loops are
                                     required": set to 1 when a visible Gaussian's opacity (after the antialiasing compensation)
                                     exceeds 0.999, i.e. when alpha = min(0.999, o x vis) can clamp at all in this frame (A.5), or
                                     when a visible Gaussian's conic is not positive definite with a margin (b^2 <= (1 - 2^-12) a c,
                                     a, c in [2^-40, 2^40]), i.e. when a pair's exponent could round to a positive number.  Culled
                                     Gaussians never raise it.  dnsplat_raster_args.saturation_flag takes it. */
    int32_t *tiles_bin;           /* required iff camera.tight_tiles: [N] tile count over the TIGHT box (what dnsplat_bin_args.tiles_per_gauss
                                     must then be given); tiles_per_gauss itself always receives gsplat's count (A.3), which is what
                                     info["tiles_per_gauss"] / DNSplatterModel.num_tiles_hit (dn_model.py:524) report */
    int32_t *tile_boxes;          /* optional [N,2]: (id of the first tile, width | height << 16, in tiles; ABI 13) of the box the tile count
                                     was taken over — the tight one if camera.tight_tiles; width x height IS that count (0 | 0 for a culled
                                     Gaussian).  dnsplat_bin_args.tile_boxes takes it and saves the binning a gather of the records, the box
                                     arithmetic per Gaussian and the separate gather of the count */
    int32_t phase;                /* 0: everything in one launch.  SH colours only (scene.sh_degree >= 0): 1 = all outputs except the three
                                     colour channels of the records (left 0; no coefficient is read), 2 = those three channels for the
                                     Gaussians with radii > 0 (reads radii and the records' location only).  A caller may run 2 on
                                     another stream beside dnsplat_bin_*: binning reads nothing phase 2 writes. */
    int32_t skip_culled_records;  /* 1 (ABI 14): the 64-byte records of culled Gaussians (radii == 0) are NOT written (left as the caller
                                     allocated them): nothing downstream reads them — the tile lists hold visible Gaussians only — and
                                     they are 28 % of the record bytes on the benchmark scenes.  0: zero-filled, as before */
} dnsplat_proj_out;

int dnsplat_project_fwd(const dnsplat_scene *scene, const dnsplat_camera *cam,
                        const dnsplat_proj_out *out, dnsplat_stream_t stream);

/* Packs caller-provided 2-D splats into records; the front end of the legacy
 * gsplat.rasterize_gaussians call (dn_model.py:564-575) whose inputs are already
 * projected. colors [N,C], C <= 8. */
int dnsplat_pack_splats(int32_t N, const float *means2d, const float *conics, const float *opacities,
                        const float *colors, int32_t C, float *splats, dnsplat_stream_t stream);

/* ------------------------------------------------------------------ stage 2
 * Tile binning.  Replaces gsplat isect_tiles + radix sort + isect_offset_encode
 * (A2-A4) and, for the legacy call, map_gaussian_to_intersects + torch.sort +
 * get_tile_bin_edges (A8).  Produces the same ordering — ascending
 * (tile, depth bits), ties by Gaussian index — by (1) a stable 32-bit radix sort
 * of the Gaussians on depth, (2) emission of (tile, gaussian) pairs in that order
 * and (3) a stable radix sort on the tile id only. */
size_t dnsplat_bin_workspace_bytes(int32_t N, int64_t isect_capacity, int32_t n_tiles);

/* Byte offset, inside a workspace of that geometry, of a reserved 32-bit status word.  dnsplat_bin_emit_sort sets it to 0 and no
 * kernel of this build ever raises it: the tile sort has no inter-workgroup wait left that could time out (the decoupled look-back
 * of an earlier build, whose 20 ms bound this word reported, was removed — DESIGN.md 3.1).  Kept so that the workspace layout and
 * the symbol stay stable; tests read it after the large frames and expect 0. */
size_t dnsplat_bin_status_offset(int32_t N, int64_t isect_capacity);

typedef struct dnsplat_bin_args {
    int32_t N;                       /* entries = n_cameras x Gaussians; entry cam * (N / n_cameras) + g is Gaussian g seen by camera cam */
    int32_t n_cameras;               /* >= 1; images of one batch share width / height (gsplat rasterization with C cameras) */
    int32_t width, height, tile_size;
    const float *means2d;            /* [N,2] */
    const int32_t *radii;            /* [N] */
    const float *depths;             /* [N] */
    const int32_t *tiles_per_gauss;  /* [N] */
    int64_t isect_capacity;          /* entries flatten_ids can hold */
    int32_t *flatten_ids;            /* out [isect_capacity]: Gaussian index per sorted intersection */
    int32_t *tile_offsets;           /* out [n_cameras*n_tiles+1]: first sorted index per (camera, tile); last = n_isects */
    int64_t *n_isects;               /* out device scalar: true number of intersections (may exceed capacity) */
    int64_t *n_isects_host;          /* optional pinned host mirror, written by an async D2H copy; NULL to skip */
    void *workspace;
    size_t workspace_bytes;
    const float *splats;             /* [N,16] records of stage 1; read only when tight_tiles != 0 */
    int32_t tight_tiles;             /* as dnsplat_camera.tight_tiles of the projection that produced tiles_per_gauss */
    int32_t *tile_ends;              /* optional out [n_cameras*n_tiles]: one past the last sorted index of every non-empty tile (0 for an
                                        empty one).  dnsplat_raster_args.tile_ends takes it. */
    int32_t skip_offsets_fill;       /* with tile_ends: leave tile_offsets[t] of EMPTY tiles undefined (>= the tile's end) instead of
                                        giving them gsplat's value (the offset of the next non-empty tile) — one launch less */
    const int32_t *tile_boxes;       /* optional [N,2] = dnsplat_proj_out.tile_boxes of the projection that produced tiles_per_gauss (single
                                        camera or a batch; for camera c > 0 the kernel adds c * n_tiles to the first tile id).  With it the
                                        counts are taken from the boxes themselves (width x height, ABI 13): tiles_per_gauss must be the
                                        counts of exactly these boxes */
    int64_t *n_isects_max;           /* optional device scalar the caller zeroes once: running maximum of n_isects over the frames binned
                                        since.  For a host that never waits on a single frame's count (replayed HIP graphs). */
} dnsplat_bin_args;

/* 2a: depth sort + inclusive offsets + total.  After this (and a stream sync or
 * a look at n_isects_host) the caller knows how large flatten_ids must be. */
int dnsplat_bin_prepare(const dnsplat_bin_args *args, dnsplat_stream_t stream);
/* 2b: emit + tile sort + offsets.  If n_isects > isect_capacity nothing past the
 * capacity is written and tile_offsets are clamped: the caller must re-run with
 * a larger capacity (it detects this from n_isects). */
int dnsplat_bin_emit_sort(const dnsplat_bin_args *args, dnsplat_stream_t stream);
/* Reconstructs gsplat's 64-bit isect_ids (camera << (32 + tile bits) | tile << 32 | depth bits, tile bits =
 * floor(log2(n_tiles)) + 1) for the sorted list — only needed to populate the `isect_ids` entry of the info
 * dict.  n_tiles = tiles per camera. */
int dnsplat_bin_isect_ids(int32_t n_tiles, int32_t n_cameras, const int32_t *tile_offsets, const int32_t *flatten_ids,
                          const float *depths, int64_t *isect_ids, int64_t capacity, dnsplat_stream_t stream);

/* List cells (added after ABI 15, found by symbol).  dnsplat_bin_prepare_cells / dnsplat_bin_emit_sort_cells are dnsplat_bin_prepare /
 * dnsplat_bin_emit_sort with ONE SORTED LIST PER CELL of 2^shift_x x 2^shift_y tiles instead of one per tile; cells == NULL (or both
 * shifts 0 and no n_tile_pairs) is exactly the call without the suffix.  A consumer that re-tests every list entry against its own
 * part of the tile anyway (the fused compositing kernels: dnsplat_raster_fwd_cells / dnsplat_raster_bwd_cells) loses nothing by a
 * coarser list and the tile sort handles a Gaussian once per cell instead of once per tile.  The tile box [x0, x1) x [y0, y1) of a Gaussian
 * becomes the cell box [x0 >> shift_x, ((x1 - 1) >> shift_x) + 1) x [y0 >> shift_y, ((y1 - 1) >> shift_y) + 1) of a grid of
 * ceil(tiles_w / 2^shift_x) x ceil(tiles_h / 2^shift_y) cells per camera (the cell grids of a batch are stacked like its tile grids).
 * The list of a cell is the depth-ordered union of the lists its tiles would have had, every Gaussian once.  With cells
 *   - dnsplat_bin_args.tile_boxes is required (the cells are cut out of the projection's boxes; tiles_per_gauss is not read);
 *   - tile_offsets [n_cameras * n_cells + 1], tile_ends [n_cameras * n_cells] and flatten_ids are per cell; n_isects, isect_capacity
 *     and n_isects_host count (cell, Gaussian) pairs;
 *   - n_tile_pairs receives what n_isects would have been without cells, sum(width x height) over the boxes. */
typedef struct dnsplat_bin_cells {
    int32_t shift_x, shift_y;   /* 0..4 each */
    int64_t *n_tile_pairs;      /* optional device scalar.  If it is given together with dnsplat_bin_args.n_isects_host it must be
                                   n_isects + 1, and n_isects_host receives both words in one copy */
    int64_t *n_tile_pairs_max;  /* optional device scalar the caller zeroes once: running maximum of n_tile_pairs, as
                                   dnsplat_bin_args.n_isects_max is of n_isects (here: of the cell pairs) */
} dnsplat_bin_cells;
int dnsplat_bin_prepare_cells(const dnsplat_bin_args *args, const dnsplat_bin_cells *cells, dnsplat_stream_t stream);
int dnsplat_bin_emit_sort_cells(const dnsplat_bin_args *args, const dnsplat_bin_cells *cells, dnsplat_stream_t stream);

/* ------------------------------------------------------------------ stage 3/4
 * Per-tile front-to-back alpha compositing of D feature channels (A6 + A8 in one
 * pass) and its backward. */
/* Optional dn-splatter epilogue fused into the compositing kernels: the per-pixel
 * post-ops DNSplatterModel.get_outputs applies to the two gsplat results (dn_model.py:526-537, 577-578).
 * Only for the fused 7-channel layout rgb | expected depth | normal (D == 7, ed_channel == 3,
 * xy_split == 4, background == {0,0,0,0,1,1,1}).  Forward additionally writes
 *     rgb    = clamp(render_rgb + (1 - alpha) * background_rgb, 0, 1)          dn_model.py:526-528
 *     depth  = expected depth as composited (the alpha == 0 fill needs the image-wide maximum, which
 *              the forward reduces into *depth_max; dnsplat_dn_depth_normals applies it)  :533-537
 *     normal = (n / |n| + 1) / 2 with n the composited normal incl. its ones-background  :577-578
 * and backward takes the cotangents of those images (and of accumulation = alpha) instead of
 * v_render / v_alphas. */
typedef struct dnsplat_dn_post {
    const float *background_rgb; /* device [3] */
    float *rgb;                  /* out [H,W,3] */
    float *depth;                /* out [H,W] expected depth, unfilled */
    float *normal;               /* out [H,W,3] */
    float *depth_max;            /* device [n_cameras], caller zero-fills; receives max over each image of `depth` */
    const float *v_rgb;          /* backward: [H,W,3] */
    const float *v_depth;        /* backward: [H,W] cotangent of the FILLED depth image (masked by alpha > 0 inside) */
    const float *v_normal;       /* backward: [H,W,3] */
    const float *v_accumulation; /* backward: [H,W] or NULL */
} dnsplat_dn_post;

typedef struct dnsplat_raster_args {
    int32_t width, height, tile_size;   /* tile_size must be 16 */
    int32_t D;                          /* feature channels, 1..8 */
    const float *splats;                /* [N,16]; splats, flatten_ids and v_splats may be NULL iff every tile list is empty */
    const int32_t *flatten_ids;
    const int32_t *tile_offsets;        /* [n_tiles+1] */
    const float *background;            /* device [D] or NULL (gsplat v1: none; legacy normal pass: ones) */
    int32_t ed_channel;                 /* channel normalised by max(alpha,1e-10) ("ED"), or -1 */
    float *render;                      /* [H,W,D] */
    float *alphas;                      /* [H,W] */
    int32_t *last_ids;                  /* [H,W] where the backward starts its walk of the pixel's list: a sorted index >= that of the
                                           last splat applied such that no entry in between applies to the pixel (undefined where alpha == 0) */
    /* backward only */
    const float *v_render;              /* [H,W,D] */
    const float *v_alphas;              /* [H,W] or NULL */
    int32_t xy_split;                   /* channels >= xy_split do not feed v_xy/|v_xy|: the reference renders
                                           them with xys.detach() (dn_model.py:562). Use D for "all feed". */
    float *v_splats;                    /* [N,16] gradient records, accumulated into (caller zero-fills) */
    const dnsplat_dn_post *dn;          /* NULL, or the fused dn-splatter epilogue (then v_render / v_alphas are unused) */
    int32_t n_cameras;                  /* 0 or 1: one image.  C > 1: images [C,H,W,.] stacked, tile_offsets [C*n_tiles+1], splat /
                                           gradient records [C*N,16] (record cam*N + g), as produced by a dnsplat_bin_args batch */
    uint64_t *keep_masks;               /* NULL, or device [2 * keep_mask_stride] 64-bit words handed from the forward to the backward:
                                           for every 16x8 half tile and every batch of 64 consecutive list entries, which entries
                                           passed the forward's rectangle test (can reach alpha >= 1/255 somewhere in the half tile).
                                           Word of (list l = camera*n_tiles + tile, half h, batch b): [h * stride + (tile_offsets[l] >> 6) + l + b].
                                           The backward then skips its own test and never gathers the records of rejected entries. */
    int64_t keep_mask_stride;           /* >= (isect capacity >> 6) + n_cameras * n_tiles + 1 */
    uint64_t *pair_counters;            /* NULL, or device [8] (measurement builds of the fused pass, bench.py's VALU roofline), added to:
                                           forward  [0] list entries examined  [1] splats walked (kept by the rectangle test)
                                                    [2] live (pixel, splat) pairs evaluated  [3] pairs blended
                                           backward [4] (pixel, splat) slots issued (steps x 128)  [5] pairs replayed */
    const uint32_t *saturation_flag;    /* NULL, or dnsplat_proj_out.saturation_flag of the projection(s) behind `splats`: if the word
                                           is 0 no pair of this launch can clamp or have a positive exponent, and dnsplat_raster_bwd (only; the
                                           forward ignores it) runs its step loop without the clamp handling and without the exponent's
                                           sign test (same results, ~5 % fewer cycles); read on the device, no host sync.  A caller who
                                           writes records by hand passes a nonzero word (or NULL) unless they satisfy both conditions */
    const int32_t *tile_ends;           /* NULL: tile t's list is [tile_offsets[t], tile_offsets[t+1]).  Else dnsplat_bin_args.tile_ends:
                                           the list is [tile_offsets[t], tile_ends[t]) and empty where tile_ends[t] <= tile_offsets[t] */
    void *zero_fill;                    /* dnsplat_raster_fwd only: NULL, or a device buffer of zero_fill_bytes (multiple of 16) the launch clears
                                           on the way — meant for the v_splats buffer the backward of the same frame accumulates into */
    int64_t zero_fill_bytes;
    float *det_partials;                /* dnsplat_raster_bwd only: NULL (gradient records accumulated into v_splats with fp32 atomics, in arrival
                                           order), or a ZERO-FILLED device buffer [2, det_capacity, 16]: the deterministic mode.  The row a 16x8 half
                                           tile (half h) contributes to the splat at sorted list index i is then STORED at [h][i][:] and v_splats is
                                           not touched; dnsplat_det_reduce adds the rows up per gradient record in a fixed order */
    int64_t det_capacity;               /* >= the isect capacity of the lists (entries flatten_ids can hold) */
} dnsplat_raster_args;

int dnsplat_raster_fwd(const dnsplat_raster_args *args, dnsplat_stream_t stream);
int dnsplat_raster_bwd(const dnsplat_raster_args *args, dnsplat_stream_t stream);

/* The fused pass (args->dn != NULL) over the per-cell lists of dnsplat_bin_emit_sort_cells (added after ABI 15, found by symbol);
 * cells == NULL or both shifts 0 is the call without the suffix.  The list of a tile is the list of the cell it lies in: every 16x8
 * half tile takes it in batches of 64, runs its rectangle test on every entry and walks the survivors, as it does with a per-tile
 * list — entries whose own tile box leaves this tile out are dropped with the culled ones (dnsplat_raster_cells.tile_boxes), so the
 * splats a tile walks, their order and the images are the per-tile ones bit for bit.  With cells
 *   - tile_offsets / tile_ends / flatten_ids are per cell, last_ids are positions in the cell lists;
 *   - a half tile has a PLANE: p = ((tile_y & (2^shift_y - 1)) << shift_x | (tile_x & (2^shift_x - 1))) * 2 + half, one of
 *     P = 2 * 2^shift_x * 2^shift_y.  keep_masks is [P * keep_mask_stride], the word of (list l = camera * n_cells + cell, plane p,
 *     batch b) is [p * stride + (tile_offsets[l] >> 6) + l + b], keep_mask_stride >= (capacity >> 6) + n_cameras * n_cells + 1;
 *   - det_partials is [P, det_capacity, 16], the row of (plane p, list index i) at [p][i][:]; dnsplat_det_reduce_planes adds them up. */
typedef struct dnsplat_raster_cells {
    int32_t shift_x, shift_y;   /* as dnsplat_bin_cells */
    const int32_t *tile_boxes;  /* [entries, 2] dnsplat_bin_args.tile_boxes of the binning behind the lists (required with a nonzero shift).  A
                                   tile takes a list entry only if the entry's OWN tile box holds the tile: the box is clipped to gsplat's
                                   3-sigma box, beyond which a splat of opacity > 0.35 would still pass the alpha test — per-tile lists never
                                   hold it there, and neither may a cell's */
} dnsplat_raster_cells;
int dnsplat_raster_fwd_cells(const dnsplat_raster_args *args, const dnsplat_raster_cells *cells, dnsplat_stream_t stream);
int dnsplat_raster_bwd_cells(const dnsplat_raster_args *args, const dnsplat_raster_cells *cells, dnsplat_stream_t stream);

/* Deterministic reduction of the rows dnsplat_raster_bwd left in det_partials (test / debug mode, DNSPLAT_DETERMINISTIC=1 in the
 * Python binding): the sorted list is stably re-sorted by record id (hand-written LSD radix, as the binning), and each record g
 * that has list entries receives
 *     v_splats[g][:] = sum over its entries in ascending list order of (partials[0][entry] + partials[1][entry]),
 * accumulated in float64 and rounded once.  Rows of records without entries are left as they are (the caller zero-fills).  Same
 * inputs give the same bits in every run, whatever order the compositing workgroups finished in.  Enqueued on `stream`, no sync. */
typedef struct dnsplat_det_args {
    int32_t n_records;          /* gradient records (cameras x Gaussians) */
    int64_t capacity;           /* dnsplat_raster_args.det_capacity */
    const int64_t *n_isects;    /* device scalar: number of valid list entries (dnsplat_bin_args.n_isects); clamped to capacity */
    const int32_t *flatten_ids; /* [capacity] the sorted list the compositing walked */
    const float *partials;      /* [2, capacity, 16] */
    float *v_splats;            /* [n_records, 16] */
    void *workspace;            /* dnsplat_det_workspace_bytes(capacity) */
    size_t workspace_bytes;
} dnsplat_det_args;
size_t dnsplat_det_workspace_bytes(int64_t capacity);
int dnsplat_det_reduce(const dnsplat_det_args *args, dnsplat_stream_t stream);
/* dnsplat_det_reduce over `partials` [n_planes, capacity, 16] (added after ABI 15, found by symbol; dnsplat_raster_bwd_cells): per entry
 * the planes in ascending order.  n_planes == 2 is dnsplat_det_reduce. */
int dnsplat_det_reduce_planes(const dnsplat_det_args *args, int32_t n_planes, dnsplat_stream_t stream);

/* Depth fill + depth->normal stencil of get_outputs (dn_model.py:533-537 and 589-603 with
 * utils/normal_utils.py:9-48, utils/camera_utils.py:92-144, called with c2w = identity):
 *     depth_out      = alpha > 0 ? depth : *depth_max
 *     surface_normal = (1 + diag(1,-1,-1) * normalize(cross(right - left, top - bottom))) / 2 of the
 *                      back-projected (pixel centre + 0.5) depth_out; 0.5 on the one-pixel border.
 * No gradient flows through it in the reference (depth.detach(), dn_model.py:590). */
int dnsplat_dn_depth_normals(int32_t width, int32_t height, float fx, float fy, float cx, float cy,
                             const float *depth, const float *alphas, const float *depth_max,
                             float *depth_out /* [H,W] */, float *surface_normal /* [H,W,3] */,
                             dnsplat_stream_t stream);

/* nerfstudio get_viewmat + intrinsics + normal frame in one launch: from the camera-to-world matrix
 * c2w [3,4] (OpenGL axes, device) writes viewmat[16] (world->camera, OpenCV), K[9] and
 * normal_frame[12] (see dnsplat_camera).  Replaces ~20 tiny torch kernels per frame (dn_model.py:475-479).
 * zero_word (optional): n_zero_words (>= 1) device words set to 0 by the same launch — the frame's
 * dnsplat_proj_out.saturation_flag and dnsplat_dn_post.depth_max start here without fill launches of their own. */
int dnsplat_camera_prepare(const float *c2w, float fx, float fy, float cx, float cy,
                           float *viewmat, float *K, float *normal_frame, uint32_t *zero_word, int32_t n_zero_words,
                           dnsplat_stream_t stream);

/* Multi-view data parallelism, compact exchange of the SH gradients.  For one camera the gradient of Gaussian g's SH
 * coefficients is an outer product  v_coeff[g][k][c] = basis_k(dir_g) * v_colour[g][c]  (k < (degree+1)^2, c < 3), and the
 * direction dir_g = normalize(mean_g - camera position) is something every rank can work out for every camera: the means are
 * replicated and a camera position is 12 bytes.  So what travels per (camera, Gaussian) is the clamp-masked colour gradient
 * alone — 12 bytes instead of the 192 bytes of coefficient gradients: with one camera per GPU the ranks all-gather
 * [N,3] slabs (7 x 12 B received per Gaussian at 8 GPUs instead of ~2 x 7/8 x 192 B of an all-reduce) and every rank rebuilds
 *     v_coeff = scale * sum_views basis(normalize(mean - pos_view)) (x) v_colour_view
 * with dnsplat_sh_grads_from_factors.
 * factors: n_views slabs of 3 N + 4 floats: [N,3] colour gradients | camera position (3) | 0, as dnsplat_sh_factors writes one.
 * means: the [N,3] means of the scene.  Layouts of v_sh0 / v_shN as dnsplat_scene.sh0 / shN. */
int dnsplat_sh_grads_from_factors(int32_t N, int32_t n_views, const float *factors, const float *means, int32_t sh_degree,
                                  int32_t sh_K, float scale, float *v_sh0, int32_t v_sh0_stride, float *v_shN,
                                  int32_t v_shN_stride, dnsplat_stream_t stream);

/* One camera's slab (3 N + 4 floats, see above) from the forward's outputs (radii, viewmat of dnsplat_camera, splats =
 * dnsplat_proj_out.splats) and the gradient records of dnsplat_raster_bwd — without the rest of the projection backward, so
 * that the host can start the all-gather BEFORE dnsplat_project_bwd (called with sh_grads_skip = 1) and the exchange runs while
 * the geometry gradients are still being computed.  A colour that sits exactly on the clamp (c + 0.5 == 0) is masked. */
int dnsplat_sh_factors(int32_t N, const int32_t *radii, const float *viewmat, const float *splats, const float *v_splats,
                       float *factors, dnsplat_stream_t stream);

/* ABI 14.  As dnsplat_sh_grads_from_factors, but ADDS  scale * sum over the views v != skip_view  to rows that already hold the
 * (pre-scaled, dnsplat_proj_grads.sh_grad_scale) contribution of view skip_view — the rank's own camera, whose rows
 * dnsplat_project_bwd wrote itself as on a single GPU.  With n_views == 1 there is nothing to add and nothing is launched: the
 * exchange step costs a single rank no pass over the 192 B / Gaussian of coefficient gradients.  (At n_views >= 2 the read-modify-
 * write moves more bytes than rebuilding every row from the slabs — dp.ShFactorExchange picks per world size.) */
int dnsplat_sh_grads_add_factors(int32_t N, int32_t n_views, int32_t skip_view, const float *factors, const float *means,
                                 int32_t sh_degree, int32_t sh_K, float scale, float *v_sh0, int32_t v_sh0_stride, float *v_shN,
                                 int32_t v_shN_stride, dnsplat_stream_t stream);

/* ABI 14.  Slabs of visible rows only.  A camera sees ~72 % of the Gaussians of the benchmark scenes; the colour gradients of the
 * others are zero and need not travel.  One camera's PACKED slab (all ranks agree on `capacity` rows):
 *     header  [0] count of visible Gaussians (uint32; > capacity = overflow: rows beyond it were dropped, the caller must notice)
 *             [1..3] camera centre (float)        [4..7] reserved
 *     masks   ceil(N / 64) 64-bit words, bit = radii > 0
 *     offsets ceil(N / 64) uint32: visible Gaussians in front of the word's block (exclusive prefix sum of the popcounts)
 *     rows    capacity x 3 floats: the clamp-masked colour gradient of the k-th visible Gaussian
 * dnsplat_packed_slab_floats gives the size (in 4-byte words, a multiple of 4).  dnsplat_visible_index writes header, masks and
 * offsets from the forward's radii (two small launches; `scratch`: ceil(N / 64) uint32); dnsplat_project_bwd fills the rows
 * (dnsplat_proj_grads.sh_packed); dnsplat_sh_grads_from_packed is dnsplat_sh_grads_from_factors / _add_factors over n_views such slabs
 * laid out `slab_floats` words apart (skip_view < 0: rebuild every row; >= 0: add the other views to the rows in place). */
size_t dnsplat_packed_slab_floats(int32_t N, int32_t capacity);
int dnsplat_visible_index(int32_t N, int32_t capacity, const int32_t *radii, const float *viewmat, float *slab, uint32_t *scratch,
                          dnsplat_stream_t stream);
int dnsplat_sh_grads_from_packed(int32_t N, int32_t capacity, int32_t n_views, int32_t skip_view, const float *slabs,
                                 const float *means, int32_t sh_degree, int32_t sh_K, float scale, float *v_sh0, int32_t v_sh0_stride,
                                 float *v_shN, int32_t v_shN_stride, dnsplat_stream_t stream);

/* Densification statistics: the per-step accumulation nerfstudio's SplatfactoModel.after_train
 * performs on the renderer's outputs (called at dn_model.py:938-942, consumed by refinement_after dn_model.py:286-296):
 * for every Gaussian with radii > 0
 *     xys_grad_norm += |(gx, gy)|,  vis_counts += 1,  max_2Dsize = max(max_2Dsize, radii * inv_max_size),  inv_max_size = 1 / max(W, H).
 * xy_grads rows are grad_stride floats apart (2 for a [N,2] tensor, 16 to read the |v_xy| columns of the gradient
 * records in place: pass v_splats + 14). */
int dnsplat_densify_stats(int32_t N, const int32_t *radii, const float *xy_grads, int32_t grad_stride, float inv_max_size,
                          float *xys_grad_norm, float *vis_counts, float *max_2Dsize, dnsplat_stream_t stream);

/* Densification decisions of refinement_after (dn_model.py:271-386; cull rules of the inherited nerfstudio
 * SplatfactoModel.cull_gaussians), one flag byte per Gaussian.  do_densify = the `do_densification` branch is active;
 * screen_rules = step < stop_screen_size_at; cull_big = step > refine_every * reset_alpha_every.  Appended entries (split
 * children, duplicates) enter the cull with max_2Dsize = 0, children with scales log(exp(s) / 1.6).
 * Every comparison is the reference's, strictness included (>, <, and <= for the duplicate rule), and nan follows torch: a nan
 * log-scale makes the Gaussian's largest scale nan (torch's max propagates it), so none of its scale comparisons holds — it is
 * neither split, duplicated nor too big; a nan opacity is not low; 0 / 0 visibility is not a high gradient. */
#define DNSPLAT_DENSIFY_SPLIT 1       /* split into n_split_samples children; the parent is then pruned */
#define DNSPLAT_DENSIFY_DUP 2         /* duplicated once */
#define DNSPLAT_DENSIFY_CULL 4        /* the original entry is removed */
#define DNSPLAT_DENSIFY_CULL_CHILD 8  /* its split children would be removed right away */
#define DNSPLAT_DENSIFY_CULL_DUP 16   /* its duplicate would be removed right away */
typedef struct dnsplat_densify_args {
    int32_t N;
    const float *scales;        /* [N,3] log-scales */
    const float *opacities;     /* [N] logits */
    const float *xys_grad_norm; /* [N] accumulated by dnsplat_densify_stats (all-reduced over the ranks when data parallel) */
    const float *vis_counts;    /* [N] */
    const float *max_2Dsize;    /* [N] or NULL */
    int32_t do_densify, screen_rules, cull_big;
    float max_image_side;       /* max(H, W) of the last rendered frame (dn_model.py:296) */
    float densify_grad_thresh, densify_size_thresh, split_screen_size;
    float cull_alpha_thresh, cull_scale_thresh, cull_screen_size;
    uint8_t *flags;             /* out [N] */
} dnsplat_densify_args;
int dnsplat_densify_classify(const dnsplat_densify_args *args, dnsplat_stream_t stream);

/* Means and log-scales of the split children (nerfstudio split_gaussians): child j belongs to parent parents[j % n_parents]
 * (samples are laid out sample-major, as `repeat(samps, 1)` does):
 *     mean = mean_p + R(q_p / |q_p|) (exp(scale_p) * noise_j),   scale = log(exp(scale_p) / 1.6). */
int dnsplat_densify_split(int32_t n_children, int32_t n_parents, const int32_t *parents, const float *noise /* [n_children,3] */,
                          const float *means, const float *scales, const float *quats, float *new_means /* [n_children,3] */,
                          float *new_scales /* [n_children,3] */, dnsplat_stream_t stream);

/* dn-splatter's per-pixel training loss and its gradient w.r.t. the rendered images in two launches:
 *   loss = (1 - l) mean|rgb - gt| + l (1 - SSIM(rgb, gt))                       nerfstudio splatfacto RGB term, l = ssim_lambda
 *        + depth_weight (EdgeAwareLogL1_x + EdgeAwareLogL1_y)(depth, gt_depth)  losses.py:187-224, mask gt_depth > tolerance,
 *                                                                               depth_weight = 1 + depth_lambda (regularization_strategy.py:184)
 *        + mean|normal - gt_normal| + TV(normal)                                regularization_strategy.py:188-193, losses.py:279-295
 * (dn_model.py:614-729; the per-Gaussian min-scale term is added by the caller).  Outputs the cotangents v_rgb,
 * v_depth, v_normal of a unit loss gradient and, in sums[8], the partial sums
 *   {sum SSIM, sum|rgb-gt|, sum EA_x, sum EA_y, sum|n-gt_n|, sum TV_h, sum TV_w, 0} from which the loss value follows. */
typedef struct dnsplat_dn_loss_args {
    int32_t width, height;
    const float *rgb;          /* [H,W,3] rendered */
    const float *depth;        /* [H,W]   rendered (filled) depth */
    const float *normal;       /* [H,W,3] rendered normal image in [0,1] */
    const float *gt_rgb;       /* [H,W,3] */
    const float *gt_depth;     /* [H,W] or NULL (no depth loss) */
    const float *gt_normal;    /* [H,W,3] or NULL (no normal losses) */
    const float *depth_counts; /* device [2]: number of pixels with gt_depth > tolerance in columns < W-1, in rows < H-1 */
    float ssim_lambda, depth_weight, depth_tolerance;
    float *maps;               /* scratch, 9 H W + 512 floats (512 partial-sum words in front of three [H,W,3] maps) */
    float *v_rgb, *v_depth, *v_normal;   /* out, shapes of rgb / depth / normal */
    float *sums;               /* out device [8] */
} dnsplat_dn_loss_args;

int dnsplat_dn_loss(const dnsplat_dn_loss_args *args, dnsplat_stream_t stream);

/* ABI 15.  The SSIM term ALONE, for a loss stack that otherwise stays in PyTorch (BASELINE.json: "losses stay in PyTorch-ROCm"):
 * what nerfstudio splatfacto's `self.ssim(gt, pred)` computes inside the RGB term dn-splatter inherits (dn_model.py:624-627, :663) —
 * pytorch_msssim.SSIM(data_range=1, size_average=True, channel=3): 11-tap Gaussian sigma 1.5, valid padding, mean over the
 * (W-10)(H-10) windows of the 3 channels.  MIOpen runs the sixteen depthwise conv2d calls of that module and its backward at
 * 250-500 us each on a 1600 x 1200 image (profiles/r06_c5_torch_loss_kernel_stats.txt).
 *   sums[0] = sum of the per-window SSIM values (mean = sums[0] / (3 (W-10)(H-10))),
 *   v_x     = d(mean SSIM)/dx, [H,W,3], or NULL (value only);   x, y: [H,W,3] fp32;   maps: scratch, 9 H W + 512 floats. */
int dnsplat_ssim(int32_t width, int32_t height, const float *x, const float *y, float *maps, float *v_x, float *sums /* device [8] */,
                 dnsplat_stream_t stream);

/* ABI 15.  Two more MODULES of the reference's loss stack one by one (the rest stays PyTorch), behind drop-in nn.Modules
 * (fused_loss.EdgeAwareLogL1 / TVLoss, install_losses(model)):
 * dnsplat_edge_aware_logl1 — losses.py:187-224, "scalar" implementation, as DNRegularization.get_depth_loss calls it
 *   (regularization_strategy.py:162-170): pred, gt [H,W] fp32, rgb [H,W,3], mask [H,W] bytes (torch.bool) or NULL.
 *   sums[0..3] = { sum lambda_x log(1+|d|), sum lambda_y log(1+|d|), pixels counted in x, pixels counted in y }  (loss = s0/s2 + s1/s3;
 *   the reference's boolean-mask gathers `loss_x[mask]` have a data-dependent size = a host synchronisation per call: none here);
 *   v_x, v_y [H,W] (both or neither): d s0 / d pred, d s1 / d pred — the caller divides by the counts.
 * dnsplat_tv_loss — losses.py:279-295 on an [H,W,C] image: sums[0..1] = { sum |p - right|, sum |p - lower| },
 *   v_pred = d/d pred of the loss s0 / (H (W-1) C) + s1 / ((H-1) W C) (or NULL).
 * scratch: 512 floats; sums: device [8]. */
int dnsplat_edge_aware_logl1(int32_t width, int32_t height, const float *pred, const float *gt, const float *rgb, const uint8_t *mask,
                             float *v_x, float *v_y, float *scratch, float *sums, dnsplat_stream_t stream);
int dnsplat_tv_loss(int32_t width, int32_t height, int32_t channels, const float *pred, float *v_pred, float *scratch, float *sums,
                    dnsplat_stream_t stream);

/* Additive in ABI 15 (found by symbol).  The Pearson depth losses of depth_loss_type = PearsonDepth — losses.py:428-450
 * (PearsonDepthLoss) on the whole frame and :454-485 (LocalPearsonDepthLoss) on n_boxes windows of box x box pixels, as
 * regularization_strategy.py:167-177 combines them — value and gradient w.r.t. the prediction in at most five launches, where the
 * reference loops over the boxes in Python and slices each with device scalars.  Per region: both arguments centred
 * on their means, divided by the UNBIASED standard deviation + 1e-6, co = mean of the product, loss = 1 - co.
 *   pred, gt   [H,W] fp32.
 *   mask       [H,W] bytes (torch.bool) or NULL: only these pixels enter the whole-frame region (depth_loss(pred[mask], gt[mask])
 *              without the gather); needs whole != 0.  Boxes ignore it.
 *   whole      non-zero: the whole-frame region takes part.
 *   box_rows, box_cols   DEVICE int64 [n_boxes] (what torch.randint returns: passed on as drawn, never read on the host): the upper
 *              left corner of each box, 0 <= row <= H - box, 0 <= col <= W - box (values outside are clamped into that range).  Boxes
 *              may overlap and repeat; a repeated box counts twice.  Any n_boxes >= 0; any 2 <= box <= min(W, H) (a box of more than
 *              128 x 128 pixels is read twice instead of being kept in registers).
 *   sums       out, device [2]: sums[0] = 1 - co of the whole frame (0 without it), sums[1] = sum over the boxes of 1 - co_b (the
 *              caller divides by the number of boxes).
 *   v_pred     out [H,W] or NULL (values only): w_whole * d sums[0] / d pred + w_box * d sums[1] / d pred, each term rounded to fp32
 *              before the two products and the sum (the combined call equals the weighted sum of the two separate calls bit for bit).
 *   scratch    dnsplat_pearson_scratch_bytes(n_boxes) bytes, 8-byte aligned; contents need not survive.
 * Second moments are centred (two sweeps, sums in double), every reduction has a fixed order and there is no atomic: the result is
 * bit-reproducible.  A region of fewer than two pixels gives nan (value and gradient), as the reference's std.  A region whose
 * prediction is constant has the value 1 - 0, and the gradient autograd gives it: torch's backward of std() passes nothing through a
 * standard deviation of exactly 0, the path through the numerator remains.  No allocation, no synchronisation.
 * Returns without a launch: DNSPLAT_ERR_INVALID_ARG for a NULL pred / gt / scratch / sums, width < 1, height < 1, n_boxes < 0, a mask
 * with whole == 0, and with n_boxes > 0: NULL origins, box < 2, box > min(W, H); DNSPLAT_ERR_UNSUPPORTED for n_boxes > 0 and
 * box > 46340 (box * box is an int32).  With n_boxes == 0 neither box nor the origins are looked at: the whole-frame call has no box
 * to name and passes 0. */
size_t dnsplat_pearson_scratch_bytes(int32_t n_boxes);   /* 0 for n_boxes < 0 */
int dnsplat_pearson_depth(int32_t width, int32_t height, const float *pred, const float *gt, const uint8_t *mask, int32_t whole,
                          int32_t n_boxes, int32_t box, const int64_t *box_rows, const int64_t *box_cols, float w_whole, float w_box,
                          float *v_pred, void *scratch, float *sums, dnsplat_stream_t stream);

/* Additive in ABI 15 (found by symbol).  The filtered normal loss of the AGS-Mesh regularisation strategy —
 * AGSMeshRegularization.get_normal_loss (regularization_strategy.py:292-321) with find_edges (:40-96) and mean_angular_error (:11-26) —
 * in two launches, where the reference runs six one-channel conv2d calls and two boolean-mask gathers (a host synchronisation each).
 * With n the ground-truth normal in [-1, 1], per channel: r = 1 / (n + 1e-6), lap = up + down + left + right - 4 r with zeros outside
 * the frame, e = lap > 0.01, E = OR of e over the 3 x 3 neighbourhood (zeros outside); per pixel: C = not (dot(n, surf) < cos 0.1), the
 * reference's not (arccos(clip(dot, -1, 1)) > 0.1).  Plain IEEE fp32 in the order ((up + down) + left) + right - 4 r: a border pixel
 * with a negative component is an edge, a component of exactly -1e-6 gives inf, inf - inf is nan and nan > 0.01 is false; a nan dot
 * product is confident.
 *   surf, gt, pred   fp32 images of one frame: layout DNSPLAT_AGS_LAYOUT_CHW = [3,H,W] in [-1, 1] (what the method receives),
 *              DNSPLAT_AGS_LAYOUT_HWC = [H,W,3] in [0, 1] (what outputs / batch hold): 2 x - 1 is applied here, one rounding as torch's.
 *   mode       0: the mean of |surf - n| runs over the ELEMENTS with ~E; 1: over the three channels of the pixels with C.
 *   sums       out, device double [2]: sums[0] = sum over the selected elements of |surf - n|, sums[1] = sum over all 3 H W elements of
 *              |pred - n|.
 *   count      out, device int64 [1]: the number of selected elements (mode 1: 3 x the confident pixels).  The loss is
 *              weight * (sums[0] / count + sums[1] / (3 H W)); count == 0 gives 0 / 0 = nan, as the reference's mean of nothing.
 *   v_surf     out, the shape of surf, or NULL: weight * sgn(surf - n) on the selected elements, 0 elsewhere — d(weight * sums[0]) / d surf;
 *              the normaliser 1 / count exists on the device only, the caller divides there (as with dnsplat_edge_aware_logl1).
 *   v_pred     out, the shape of pred, or NULL: weight * sgn(pred - n) / (3 H W), the finished gradient of the second term.
 *              Both are w.r.t. the tensor as given: in the HWC layout they carry the factor 2 of 2 x - 1.
 *   selection  out or NULL, bytes (torch.bool): mode 0 [3,H,W] = ~E (planar in either layout), mode 1 [H,W] = C.
 *   scratch    dnsplat_ags_normal_scratch_bytes(width, height) bytes, 8-byte aligned; contents need not survive.
 * One partial per workgroup (sums in double, the count an integer), added by a second launch in a fixed order, no atomic: the result
 * is bit-reproducible.  No allocation, no synchronisation.
 * Returns without a launch: DNSPLAT_ERR_INVALID_ARG for a NULL surf / gt / pred / scratch / sums / count, width < 1, height < 1, a
 * layout or a mode other than the two above; DNSPLAT_ERR_UNSUPPORTED for a side above 2^30 or a frame of more than 2^31 - 1 tiles of 64 x 16 pixels. */
#define DNSPLAT_AGS_LAYOUT_CHW 0
#define DNSPLAT_AGS_LAYOUT_HWC 1
size_t dnsplat_ags_normal_scratch_bytes(int32_t width, int32_t height);   /* 0 for width < 1 or height < 1 */
int dnsplat_ags_normal_loss(int32_t width, int32_t height, const float *surf, const float *gt, const float *pred, int32_t layout,
                            int32_t mode, float weight, float *v_surf, float *v_pred, uint8_t *selection, void *scratch, double *sums,
                            int64_t *count, dnsplat_stream_t stream);

/* Additive in ABI 15 (found by symbol).  The per-frame tail of the reference's `gs-mesh dn` exporter (export_mesh.py:351-476
 * DepthAndNormalMapsPoisson; the `tsdf` exporter :824-927 back-projects the same way): an oriented, coloured point cloud from the
 * rendered depth, colour and surface-normal images of a camera.  Three calls that share one caller-owned scratch of
 * dnsplat_pointcloud_scratch_bytes(width, height, k) bytes (16-byte aligned; its contents need not survive from one call to the next).
 * None allocates, synchronises or uses an atomic; equal inputs (and seed) give equal bits.  A frame holds at most 2^31 - 1 pixels
 * (DNSPLAT_ERR_UNSUPPORTED beyond); NULL required pointers and non-positive sizes return DNSPLAT_ERR_INVALID_ARG; both without a launch.
 *
 * dnsplat_depth_edge_valid — find_depth_edges(depth, threshold, dilation_itr) < 0.2 (export_mesh.py:58-90, :379-386), two launches.
 *   inv = 1 / (depth + 1e-6) in IEEE fp32, lap = ((up + down) + left) + right - 4 inv with ZERO taps outside the frame (the reference's
 *   padding=1), edge = lap > threshold (a nan Laplacian is no edge), valid = no edge pixel within Chebyshev distance dilation_itr —
 *   what dilation_itr rounds of the 3 x 3 all-ones conv2d followed by `> 0` compute on a 0/1 map.  The threshold decisions travel as one
 *   64-bit word per 64 pixels of a row; a workgroup dilates DNSPLAT_EDGE_ROW_TILE rows x 8 words.
 *   depth [H,W] fp32; valid [H,W] bytes (torch.bool) out.  0 <= dilation_itr <= DNSPLAT_EDGE_MAX_DILATION, else DNSPLAT_ERR_UNSUPPORTED.
 *
 * dnsplat_sample_valid_pixels — pick_indices_at_random (export_mesh.py:50-55) without the nonzero / randperm round trip: m = min(k, n)
 *   of the n valid pixels, uniformly and without replacement; n never reaches the host.  Four launches.
 *   valid      [H,W] bytes, or NULL: then a pixel is valid iff !(depth == 0) — torch.nonzero of the depth image, the reference's
 *              `valid_mask = depth_map`; a nan depth is valid.  One of valid / depth must be given (valid wins).
 *   indices    out, int32 [k] (may be NULL for k == 0): rows [0, m) hold flat pixel indices y * width + x, rows [m, k) hold -1.
 *   counts     out, device int32 [2] = {n, m}.
 *   n <= k: all valid pixels in ascending order (the reference's behaviour).  n > k: indices[t] = compact[pi(t)], compact the ascending
 *   list of the valid pixels and pi a bijection of [0, n) keyed by `seed` (a kernel argument, no device state):
 *     bits = ceil(log2 n) (0 for n = 1), half = max(1, ceil(bits / 2)), mask = 2^half - 1; a balanced Feistel network on 2 half bits with
 *     DNSPLAT_SAMPLE_ROUNDS = 4 rounds  (L, R) <- (R, L ^ (mix32(R ^ key_r) & mask)),  x = L << half | R, starting from x = t, repeated
 *     while x >= n (cycle walking);  key_r = mix32(lo32(seed) ^ mix32(hi32(seed) + 0x9e3779b9 (r + 1))), r = 0 .. 3;
 *     mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (all in uint32).
 *   This is the reference's DISTRIBUTION from another stream: its draw is torch.randperm on the CPU generator, which needs n on the host.
 *   A caller who wants that very draw passes its own indices to dnsplat_backproject_points.
 *
 * dnsplat_backproject_points — get_colored_points_from_depth (utils/camera_utils.py:92-210) with the normal-map transform
 *   (export_mesh.py:411-428) and the crop (:462-468) for the selected pixels only; three launches.  One thread per row j of `indices`
 *   (rows [0, counts[1]) when counts is given, else all n_rows; indices == NULL: every pixel in raster order, the tsdf exporter's call):
 *     d = mask && !mask[i] ? 0 : depth[i]            the mask does not change which pixels were selected (:391-396)
 *     p = ((u + 0.5 - cx) * d / fx, (v + 0.5 - cy) * d / fy, d)            in that order of operations
 *     world_j = ((p_0 A_0j + p_1 A_1j) + p_2 A_2j) + t_j                   A = inverse of the OpenCV camera-to-world rotation, row-major
 *     color = rgb[i], bit for bit
 *     normal = R normalize(diag(1, -1, -1) (2 s - 1)),  normalize(x) = x / max(|x|, 1e-12): a stored (0.5, 0.5, 0.5) gives exactly 0
 *     kept iff |B_k0 w_0 + B_k1 w_1 + B_k2 w_2 + B_k3| < h_k for k = 0, 1, 2 (strict) when a crop box is given
 *   Kept rows are appended in the order of `indices` to points / colors / normals at the device cursor state[0], which moves by their
 *   number but not past capacity; a row that would land at or beyond capacity is not written and state[1] is set to 1.  An index outside
 *   [0, width * height) is dropped and sets state[2] to 1.  The caller zeroes state once.
 *   xform   DEVICE, 21 floats: A[9], t[3], R[9] (R the camera-to-world rotation itself) — on the device so that a pose that lives there
 *           never passes through the host.    crop   DEVICE, 15 floats: B[12] (world -> box, 3 x 4 row-major), h[3]; or NULL.
 *   normal / normals NULL together: no normals are written. */
#define DNSPLAT_EDGE_ROW_TILE 32
#define DNSPLAT_EDGE_MAX_DILATION 64
#define DNSPLAT_SAMPLE_ROUNDS 4
typedef struct dnsplat_backproject_args {
    int32_t width, height;
    const float *depth;      /* [H,W] */
    const float *rgb;        /* [H,W,3] */
    const float *normal;     /* [H,W,3] in [0, 1] (outputs["surface_normal"]) or NULL */
    const uint8_t *mask;     /* [H,W] bytes or NULL */
    const int32_t *indices;  /* [n_rows] flat pixel indices or NULL */
    const int32_t *counts;   /* device {n, m} of dnsplat_sample_valid_pixels or NULL */
    int32_t n_rows;          /* length of indices; ignored without indices */
    float fx, fy, cx, cy;
    const float *xform;      /* device [21] */
    const float *crop;       /* device [15] or NULL */
    float *points;           /* [capacity,3] */
    float *colors;           /* [capacity,3] */
    float *normals;          /* [capacity,3] or NULL */
    int64_t capacity;
    int64_t *state;          /* device int64 [3]: cursor, overflow, index out of range */
    void *scratch;
} dnsplat_backproject_args;
size_t dnsplat_pointcloud_scratch_bytes(int32_t width, int32_t height, int32_t k);   /* 0 for an invalid or unsupported size */
int dnsplat_depth_edge_valid(int32_t width, int32_t height, const float *depth, float threshold, int32_t dilation_itr, uint8_t *valid,
                             void *scratch, dnsplat_stream_t stream);
int dnsplat_sample_valid_pixels(int32_t width, int32_t height, const uint8_t *valid, const float *depth, int32_t k, uint64_t seed,
                                int32_t *indices, int32_t *counts, void *scratch, dnsplat_stream_t stream);
int dnsplat_backproject_points(const dnsplat_backproject_args *args, dnsplat_stream_t stream);

/* Additive in ABI 15 (found by symbol).  The evaluation scores of one frame — DNSplatterModel.get_image_metrics_and_images
 * (dn_model.py:809-926) and get_metrics_dict (:731-807): DepthMetrics.forward (metrics.py:130-149), NormalMetrics.forward (:171-183)
 * with mean_angular_error (:59-74), and the mse / psnr of torchmetrics' PeakSignalNoiseRatio(data_range=1.0) — in one call that reads
 * each given image once (plus the two normal images twice more for the median), where the reference runs about twenty boolean-mask
 * gathers (a host synchronisation each), a sort-based torch.median over 3 H W values and fourteen .item() reads.  SSIM is
 * dnsplat_ssim; LPIPS (a network) is not part of this library.
 * Three optional image PAIRS, fp32; both pointers of a pair are NULL or neither is, and at least one pair is given:
 *   rgb, gt_rgb         [H,W,3].  mse = mean over 3 H W of (gt - pred)^2, psnr = 10 log10(1 / mse) (mse == 0: inf).  The mse -> psnr
 *                       formula is torchmetrics' as published; torchmetrics itself was not at hand: PARITY UNPINNED.
 *   depth, gt_depth     [H,W], with depth_tolerance.  Over the pixels with gt > depth_tolerance (fp32; a nan is not above it):
 *                       t = max(gt / pred, pred / gt), two IEEE fp32 divisions; a1 / a2 / a3 = the share with t < 1.25, < 1.5625,
 *                       < 1.953125; rmse = sqrt(mean (gt - pred)^2); rmse_log = the mean over the NON-NAN terms of
 *                       sqrt((log gt - log pred)^2) — a mean absolute log difference, as the reference writes it under that name;
 *                       abs_rel = mean |gt - pred| / gt; sq_rel = mean (gt - pred)^2 / gt.  Plain IEEE: a nan t is below no
 *                       threshold; pred == 0 gives t = inf and rmse_log = inf; a NEGATIVE pred gives a negative t, which is below
 *                       all three thresholds, and a nan log term that is dropped; no pixel above the tolerance gives nan everywhere.
 *   normal, gt_normal   three channels, normal_layout as DNSPLAT_AGS_LAYOUT_*: HWC = [H,W,3] (what outputs / batch hold), CHW = [3,H,W]
 *                       (a contiguous copy of what the module receives).  Values are taken AS THEY ARE, in [0, 1]: the reference applies
 *                       no 2 x - 1 here.  mae = mean over the pixels of acos(clamp(dot, -1, 1)), dot = (g0 p0 + g1 p1) + g2 p2 in fp32;
 *                       rmse = sqrt(mean over 3 H W of (g - p)^2); mean_err = mean |g - p|; med_err = torch.median of the 3 H W values
 *                       |g - p|: the LOWER median, the element of rank (n - 1) / 2 of the sorted values, with inf sorting as a value
 *                       and nan if any value is nan.  It is the bit pattern of one of the differences: exact.
 *   metrics    out, device float [DNSPLAT_METRIC_COUNT], at the DNSPLAT_METRIC_* indices; the entries of an absent pair are nan, the
 *              unused tail is 0.  Sums in double, the divisions, square roots and log10 in double, rounded once.
 *   counts     out, device int64 [DNSPLAT_METRIC_COUNTS], at the DNSPLAT_METRIC_N_* indices (0 for an absent pair).
 *   sums       out or NULL, device double [DNSPLAT_METRIC_SUMS]: the numerators before any division, at DNSPLAT_METRIC_SUM_*.
 *   scratch    dnsplat_eval_metrics_scratch_bytes(width, height) bytes, 8-byte aligned.  No precondition on its contents (the call
 *              zeroes what it accumulates into), and they need not survive.
 * One partial per workgroup (sums in double, counts as integers) added in a fixed order; the median is a radix selection on the 31
 * value bits of |g - p| in three integer histogram rounds (11 + 11 + 9 bits); no floating-point atomic: the result is
 * bit-reproducible.  Up to seven launches, no allocation, no synchronisation; nothing is read on the host between the rounds.
 * Returns without a launch: DNSPLAT_ERR_INVALID_ARG for a NULL args / scratch / metrics / counts, width < 1, height < 1, half a pair, all
 * three pairs absent, or a normal pair with a layout other than the two above; DNSPLAT_ERR_UNSUPPORTED for more than 2^31 - 1 pixels. */
#define DNSPLAT_METRIC_RGB_MSE 0
#define DNSPLAT_METRIC_RGB_PSNR 1
#define DNSPLAT_METRIC_DEPTH_ABS_REL 2
#define DNSPLAT_METRIC_DEPTH_SQ_REL 3
#define DNSPLAT_METRIC_DEPTH_RMSE 4
#define DNSPLAT_METRIC_DEPTH_RMSE_LOG 5
#define DNSPLAT_METRIC_DEPTH_A1 6
#define DNSPLAT_METRIC_DEPTH_A2 7
#define DNSPLAT_METRIC_DEPTH_A3 8
#define DNSPLAT_METRIC_NORMAL_MAE 9
#define DNSPLAT_METRIC_NORMAL_RMSE 10
#define DNSPLAT_METRIC_NORMAL_MEAN_ERR 11
#define DNSPLAT_METRIC_NORMAL_MED_ERR 12
#define DNSPLAT_METRIC_USED 13
#define DNSPLAT_METRIC_COUNT 16
#define DNSPLAT_METRIC_N_DEPTH_MASKED 0    /* pixels with gt > depth_tolerance */
#define DNSPLAT_METRIC_N_DEPTH_A1 1        /* of them, t < 1.25 */
#define DNSPLAT_METRIC_N_DEPTH_A2 2        /* t < 1.5625 */
#define DNSPLAT_METRIC_N_DEPTH_A3 3        /* t < 1.953125 */
#define DNSPLAT_METRIC_N_DEPTH_LOG 4       /* non-nan log terms */
#define DNSPLAT_METRIC_N_NORMAL_NAN 5      /* nan values among the 3 H W differences |g - p| */
#define DNSPLAT_METRIC_COUNTS 8
#define DNSPLAT_METRIC_SUM_RGB_SQ 0           /* sum over 3 H W of (gt - pred)^2 */
#define DNSPLAT_METRIC_SUM_DEPTH_SQ 1         /* over the masked pixels: (gt - pred)^2 */
#define DNSPLAT_METRIC_SUM_DEPTH_ABS_REL 2    /* |gt - pred| / gt */
#define DNSPLAT_METRIC_SUM_DEPTH_SQ_REL 3     /* (gt - pred)^2 / gt */
#define DNSPLAT_METRIC_SUM_DEPTH_LOG 4        /* |log gt - log pred| where it is not nan */
#define DNSPLAT_METRIC_SUM_NORMAL_ANGLE 5     /* over the pixels: acos(clamp(dot, -1, 1)) */
#define DNSPLAT_METRIC_SUM_NORMAL_SQ 6        /* over 3 H W: (g - p)^2 */
#define DNSPLAT_METRIC_SUM_NORMAL_ABS 7       /* |g - p| */
#define DNSPLAT_METRIC_SUMS 8
typedef struct dnsplat_eval_metrics_args {
    int32_t width, height;
    const float *rgb, *gt_rgb;          /* [H,W,3] or both NULL */
    const float *depth, *gt_depth;      /* [H,W] or both NULL */
    float depth_tolerance;
    int32_t normal_layout;              /* DNSPLAT_AGS_LAYOUT_*; looked at only with a normal pair */
    const float *normal, *gt_normal;    /* three channels in that layout, or both NULL */
    void *scratch;
    float *metrics;                     /* device [DNSPLAT_METRIC_COUNT] */
    int64_t *counts;                    /* device [DNSPLAT_METRIC_COUNTS] */
    double *sums;                       /* device [DNSPLAT_METRIC_SUMS] or NULL */
} dnsplat_eval_metrics_args;
size_t dnsplat_eval_metrics_scratch_bytes(int32_t width, int32_t height);   /* 0 for an invalid size */
int dnsplat_eval_metrics(const dnsplat_eval_metrics_args *args, dnsplat_stream_t stream);

/* ------------------------------------------------------------------ Gaussian density field (added after ABI 15, found by symbol)
 * The reference's get_closest_gaussians / get_density / get_density_grad (dn_model.py:1061-1135, :1449-1494; utils/knn.py:29-43) for the
 * marching-cubes exporter, the density_grad branch of the point-cloud exporter and the 3-NN scale initialisation.  Everything is
 * caller-allocated and nothing is read on the host.
 *
 * dnsplat_knn_build — a spatial index over N means [N,3]: a uniform grid of dnsplat_knn_grid_dim(N) cells per axis (a host function of N
 *   alone, about two points per cell, at most DNSPLAT_KNN_MAX_GRID) over their bounding box, which stays in a 64-byte header on the
 *   device.  `index` holds dnsplat_knn_index_bytes(N) bytes, 16-byte aligned; the part behind the sorted copy is scratch of the build.
 *   An axis without extent gets one layer of cells.  In-cell order is ascending Gaussian index: equal inputs give equal bytes.
 *   Two memsets and six launches.
 * dnsplat_knn_query — for each of M queries [M,3] the neighbours of rank skip .. skip + k - 1 under the key (d2, index) ascending,
 *   d2 = fma(dz, dz, fma(dy, dy, dx dx)) in DOUBLE with dx = (double)q.x - (double)p.x: sklearn's fp64 ranking, index-exact.  skip = 1 is
 *   knn_sk's dropped first column.  out_idx int32 [M,k]; out_d2 fp32 [M,k] or NULL.  A query with a non-finite coordinate gets a row of
 *   -1 (d2 nan) and reads nothing.  k + skip <= DNSPLAT_KNN_MAX_K, else DNSPLAT_ERR_UNSUPPORTED; k + skip > N, k < 1, skip < 0:
 *   DNSPLAT_ERR_INVALID_ARG.  One launch.
 * dnsplat_density_pack — records [N,16]: mean, sigmoid(opacity), M = R(q / max(|q|, 1e-12)) diag(1 / max(exp(s), 1e-3)) row-major, 3 pad
 *   (scale_rot_to_inv_cov3d(..., return_sqrt=True), dn_model.py:1603-1611).
 * dnsplat_density_eval — per sample x, over its neighbours j in rank order:  v = M_j^T (x - mu_j),  m2 = clamp(|v|^2, 0, 1e8),
 *     density = sum_j o_j exp(-m2 / 2);  if density >= 1: density / (density + 1e-5);  max(density, 1e-4)
 *     normal  = -g / max(|g|, 1e-12),  g = sum over the first num_closest neighbours of m2 M_j v
 *   Samples: `samples` [M,3], or with samples == NULL the lattice X[Rx] x Y[Ry] x Z[Rz], row (ix Ry + iy) Rz + iz (meshgrid `ij`).
 *   mask (bytes, one per sample) == 0: density = fill, normal = 0, nothing evaluated.  Neighbours: `neighbors` [M,k] int32 or int64
 *   (any index outside [0, N) makes the row nan), or with neighbors == NULL the search of dnsplat_knn_query run in the same thread
 *   (index, k, skip) — no [M,k] tensor exists; both give equal bits.  density and normals are optional, not both NULL.  One launch. */
#define DNSPLAT_KNN_MAX_K 32
#define DNSPLAT_KNN_MAX_GRID 128
typedef struct dnsplat_density_args {
    int32_t N;
    const void *index;          /* dnsplat_knn_build's; may be NULL with neighbors */
    const float *records;       /* [N,16] of dnsplat_density_pack */
    int64_t M;                  /* rows of samples; ignored for a lattice */
    const float *samples;       /* [M,3] or NULL */
    const float *X, *Y, *Z;     /* device [Rx], [Ry], [Rz]; looked at without samples */
    int32_t Rx, Ry, Rz;
    const uint8_t *mask;        /* one byte per sample or NULL */
    float fill;
    const void *neighbors;      /* [M,k] or NULL */
    int32_t neighbors_int64;    /* 0: int32, 1: int64 */
    int32_t k, skip;            /* skip is ignored with neighbors */
    int32_t num_closest;        /* neighbours that enter the normal, 0 = k */
    float *density;             /* [M] or NULL */
    float *normals;             /* [M,3] or NULL */
} dnsplat_density_args;
int32_t dnsplat_knn_grid_dim(int32_t N);      /* 0 for N < 1 */
size_t dnsplat_knn_index_bytes(int32_t N);    /* 0 for N < 1 */
int dnsplat_knn_build(int32_t N, const float *means, void *index, dnsplat_stream_t stream);
int dnsplat_knn_query(int32_t N, const void *index, int64_t M, const float *queries, int32_t k, int32_t skip, int32_t *out_idx,
                      float *out_d2, dnsplat_stream_t stream);
int dnsplat_density_pack(int32_t N, const float *means, const float *scales_log, const float *quats, const float *opacities_logit,
                         float *records, dnsplat_stream_t stream);
int dnsplat_density_eval(const dnsplat_density_args *args, dnsplat_stream_t stream);

/* ------------------------------------------------------------------ level-set surface points (added after ABI 15, found by symbol)
 * The per-camera hot path of the reference's LevelSetExtractor (export_mesh.py:514-697), DNSplatterModel.compute_level_surface_points
 * (dn_model.py:1229-1447: the SuGaR ray search), one thread per pixel.  Everything is caller-allocated; nothing is read on the host,
 * allocated or synchronised; no atomic: equal inputs give equal bits.  Per pixel i = v W + u, in raster order:
 *   depth      d = mask && !mask[i] ? 0 : depth[i].  A pixel with d <= 0 takes no part.  A pixel with a non-finite d (or a non-finite
 *              point) takes no part either and reads nothing — OUR CHOICE: the reference would raise inside sklearn.
 *   point      p = the world point of dnsplat_backproject_points, same order of operations, bit-equal; o = t of xform (c2w[:3, 3]);
 *              dir = (p - o) / max(|p - o|, 1e-12).
 *   neighbours knn_sk(means, p, k = 16): dnsplat_knn_query with k = 16, skip = 1 — knn_sk asks for 17 and drops the nearest, so these are
 *              ranks 1 .. 16 (the reference's quirk, kept).  "The closest Gaussian" c is column 0 of that result, rank 1.
 *   ray step   std = | exp(s_c) * (R(q_c / |q_c|)^T w) |, w = (o - mu_c) / |o - mu_c| (:1266-1275), computed in the thread.  std and dir
 *              are formed in double from the fp32 inputs and rounded once.
 *   samples    x_j = p + (r_j std) dir, j = 0 .. 20, r = the caller's DNSPLAT_LEVEL_RANGE_POINTS floats (torch.linspace(-3, 3, 21)).
 *   densities  D_j = sum_k o_k exp(-clamp(|M_k^T (x_j - mu_k)|^2, 0, 1e8) / 2) over the 16 neighbours OF p in rank order (no search per
 *              sample; the records of dnsplat_density_pack, the evaluation of dnsplat_density_eval); if D_j >= 1: D_j / (D_j + 1e-5).
 *              There is NO 1e-4 floor here, unlike get_density.  x_j - mu_k is formed as (p - mu_k) + (r_j std) dir in fp32: x_j
 *              itself, rounded to an ulp of |p|, would cost more accuracy through M_k than the whole evaluation does.  The analytical
 *              normal forms x - mu_k the same way, (p - mu_k) + t dir.
 *   hit test   per level L: a = the first j with D_j > L (strict).  The pixel is EMPTY unless D_0 < L (strict) and such an a >= 1 exists.
 *   hit        t = ((L - D_{a-1}) / (D_a - D_{a-1})) (T_a - T_{a-1}) + T_{a-1},  T_j = r_j std, in that order in fp32 without contraction.
 *              The point is p + t dir, the colour rgb[i] bit for bit.
 *   normal     DNSPLAT_LEVEL_NORMAL_CLOSEST: row c of the model's `normals` parameter.  DNSPLAT_LEVEL_NORMAL_ANALYTICAL:
 *              -normalize(sum_k w_k M_k (M_k^T (x - mu_k))) at the hit point x, w_k the neighbour's term of the density sum (:1388-1418;
 *              NOT get_density_grad's weight m2).  normalize(x) = x / max(|x|, 1e-12).
 * dnsplat_level_rays — one launch: depth .. hit for up to DNSPLAT_LEVEL_MAX_LEVELS levels.
 *   t_hit [n_levels,P] (nan where empty), valid [n_levels,P] bytes, closest [P] int32 (-1 where the pixel took no part); optional
 *   first_above [n_levels,P] int32 (0 where empty) and densities [P,21] (nan where the pixel took no part).
 *   Neighbours: `neighbors` [P,16] int32 or int64 (read for the participating pixels; a row with an index outside [0, N) takes no part),
 *   or NULL: the search runs in the thread on `index`.  Both give equal bits.
 *   lane_map: DNSPLAT_LEVEL_MAP_BLOCK maps a wave to an 8 x 8 block of pixels (its lanes walk the same cells of the index, as the
 *   lattice's 4 x 4 x 4 bricks do), DNSPLAT_LEVEL_MAP_ROW to 64 consecutive pixels in raster order.  The results do not depend on it.
 * dnsplat_level_points — per level, for the rows of indices / counts as dnsplat_sample_valid_pixels leaves them for the level's validity
 *   bytes: point, colour, normal; the crop box, the append at the device cursor state[0] and the flags state[1] (overflow), state[2]
 *   (index outside the frame) exactly as dnsplat_backproject_points; a row whose t_hit is nan (an empty pixel) is dropped.  t_hit and
 *   closest are the level's [P] row and the [P] tensor of dnsplat_level_rays.  The analytical normal re-runs the search for the selected
 *   rows only.  scratch: dnsplat_pointcloud_scratch_bytes(width, height, n_rows) bytes.  Three launches.
 * Returns without a launch: DNSPLAT_ERR_INVALID_ARG for NULL required pointers, width or height < 1, n_levels outside 1 .. 8, N < 17, an
 * unknown lane_map or normal_mode; DNSPLAT_ERR_UNSUPPORTED for more than 2^31 - 1 pixels. */
#define DNSPLAT_LEVEL_RANGE_POINTS 21
#define DNSPLAT_LEVEL_MAX_LEVELS 8
#define DNSPLAT_LEVEL_KNN 16
#define DNSPLAT_LEVEL_MAP_BLOCK 0
#define DNSPLAT_LEVEL_MAP_ROW 1
#define DNSPLAT_LEVEL_NORMAL_CLOSEST 0
#define DNSPLAT_LEVEL_NORMAL_ANALYTICAL 1
typedef struct dnsplat_level_rays_args {
    int32_t width, height;
    const float *depth;         /* [H,W] */
    const uint8_t *mask;        /* [H,W] bytes or NULL */
    float fx, fy, cx, cy;
    const float *xform;         /* device [21], as dnsplat_backproject_args */
    const float *range;         /* device [DNSPLAT_LEVEL_RANGE_POINTS] */
    int32_t N;
    const void *index;          /* dnsplat_knn_build's; may be NULL with neighbors */
    const float *records;       /* [N,16] of dnsplat_density_pack */
    const float *scales_log;    /* [N,3] */
    const float *quats;         /* [N,4] wxyz, any norm */
    const void *neighbors;      /* [P,16] or NULL */
    int32_t neighbors_int64;    /* 0: int32, 1: int64 */
    int32_t n_levels;
    float levels[DNSPLAT_LEVEL_MAX_LEVELS];
    int32_t lane_map;           /* DNSPLAT_LEVEL_MAP_* */
    float *t_hit;               /* [n_levels,P] */
    uint8_t *valid;             /* [n_levels,P] */
    int32_t *closest;           /* [P] */
    int32_t *first_above;       /* [n_levels,P] or NULL */
    float *densities;           /* [P,21] or NULL */
} dnsplat_level_rays_args;
typedef struct dnsplat_level_points_args {
    int32_t width, height;
    const float *depth;         /* [H,W] */
    const float *rgb;           /* [H,W,3] */
    const uint8_t *mask;        /* [H,W] bytes or NULL */
    const int32_t *indices;     /* [n_rows] flat pixel indices */
    const int32_t *counts;      /* device {n, m} of dnsplat_sample_valid_pixels or NULL */
    int32_t n_rows;
    float fx, fy, cx, cy;
    const float *xform;         /* device [21] */
    const float *crop;          /* device [15] or NULL */
    const float *t_hit;         /* [P]: the level's row */
    const int32_t *closest;     /* [P] */
    int32_t normal_mode;        /* DNSPLAT_LEVEL_NORMAL_* */
    const float *gauss_normals; /* [N,3], the model's `normals`; CLOSEST only */
    int32_t N;
    const void *index;          /* ANALYTICAL only */
    const float *records;       /* ANALYTICAL only */
    float *points, *colors, *normals;   /* [capacity,3] */
    int64_t capacity;
    int64_t *state;             /* device int64 [3]: cursor, overflow, index out of range */
    void *scratch;
} dnsplat_level_points_args;
int dnsplat_level_rays(const dnsplat_level_rays_args *args, dnsplat_stream_t stream);
int dnsplat_level_points(const dnsplat_level_points_args *args, dnsplat_stream_t stream);

/* ------------------------------------------------------------------ marching cubes (added after ABI 15, found by symbol)
 * The step between the density lattice and the mesh of the reference's MarchingCubesMesh (export_mesh.py:778, mcubes.marching_cubes on
 * the CPU there).  The output is a canonical, bit-reproducible function of (volume, level):
 *   above      a lattice point is above iff v > level, one fp32 comparison (NaN is not above, +-inf behave as their values).
 *   vertices   one per lattice edge whose two ends differ in that test.  The edge from point p along axis a belongs to p, the end
 *              with the lower index; vertices are numbered in ascending (flat index of p, a).  Lattice coordinates, float32:
 *              t = (level - v(p)) / (v(p + e_a) - v(p)), component a = float(p_a) + t, the other two are the integers; correctly
 *              rounded, no contraction.  A non-finite t is written as the arithmetic gives it, a NaN as the quiet NaN 0x7FC00000.
 *   triangles  int32 vertex ids.  Cells in ascending flat index of their lowest corner, within a cell in the order of the case table
 *              (csrc/mc_table.h, generated by tools/gen_mc_table.py from contours traced on the cube's faces); the right-hand normal
 *              points towards decreasing value.  A corner equal to `level` gives t = 0 or 1: the zero-area triangles are kept.
 * volume is [nx,ny,nz] contiguous, the last axis fastest (meshgrid(indexing="ij"), as dnsplat_density_eval writes its lattice).
 * dnsplat_mc_count — masks, counts and their scan into `scratch` (dnsplat_mc_scratch_bytes(nx, ny, nz) bytes); counts = {V, T}.  Four
 *   launches.  The caller reads the two counts to size the buffers, or passes capacities it knows to suffice and reads nothing.
 * dnsplat_mc_emit — after dnsplat_mc_count with the same volume, level, sizes, scratch and counts: the first min(V, cap_v) vertices and
 *   min(T, cap_t) triangles; nothing is written past either capacity.  *status = DNSPLAT_MC_STATUS_VERTICES if V > cap_v, |
 *   DNSPLAT_MC_STATUS_TRIANGLES if T > cap_t, else 0 (capacities above 2^31 - 1 count as 2^31 - 1: ids are int32).  Two launches.
 * An axis shorter than 2 has no cells: counts = {0, 0}, status = 0, return 0, scratch may be NULL.  No atomics: equal inputs give equal
 * bytes.  Returns without touching the device: DNSPLAT_ERR_INVALID_ARG for NULL args / volume / counts / scratch (/ status, / a buffer
 * whose capacity is positive), a size < 1, nx ny nz >= 2^31 or a negative capacity; DNSPLAT_ERR_WORKSPACE for a short scratch. */
#define DNSPLAT_MC_STATUS_VERTICES 1
#define DNSPLAT_MC_STATUS_TRIANGLES 2
typedef struct dnsplat_mc_args {
    const float *volume;        /* device [nx,ny,nz] */
    int32_t nx, ny, nz;
    float level;
    void *scratch;
    size_t scratch_bytes;
    int64_t *counts;            /* device int64 [2]: V, T; written by count, read by emit */
    int64_t cap_v, cap_t;       /* emit: rows of vertices / triangles */
    float *vertices;            /* emit: [cap_v,3] */
    int32_t *triangles;         /* emit: [cap_t,3] */
    int32_t *status;            /* emit: device int32 [1] */
} dnsplat_mc_args;
size_t dnsplat_mc_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);   /* 0 for an invalid size */
int dnsplat_mc_count(const dnsplat_mc_args *args, dnsplat_stream_t stream);
int dnsplat_mc_emit(const dnsplat_mc_args *args, dnsplat_stream_t stream);

/* The same extraction over the OBSERVED part of a lattice (added after ABI 15, found by symbol): Open3D's rule for a TSDF volume, "a
 * cell is extracted only if all eight corners carry weight", which filling the unseen voxels with NaN does not give (such a cell still
 * emits its other triangles, and vertices with a NaN coordinate).  A lattice point is observed iff weight > min_weight, one fp32
 * comparison (NaN is not observed).  The rules are those above with three changes:
 *   an edge owns a vertex iff its two ends are BOTH OBSERVED and differ in the `above` test;
 *   a cell has its table case iff ALL EIGHT corners are observed, else case 0 (no triangle);
 *   the value of an unobserved point is never read into a result: any fill — NaN, inf, 1e30 — gives the same bytes.
 * Numbering and order are unchanged.  Every triangle's vertices exist (the edges of a valid cell have observed ends).  At the rim of the
 * observed region a vertex may be referenced by no triangle; it is part of the canonical output and is not compacted away.  `weight` is
 * [nx,ny,nz] like the volume; scratch is dnsplat_mc_observed_scratch_bytes(nx, ny, nz) bytes — the layout of dnsplat_mc_scratch_bytes
 * plus one mask word per 64 points.  dnsplat_mc_count / dnsplat_mc_emit are untouched: their bytes, launches and scratch are as before.
 * Errors as above, and DNSPLAT_ERR_INVALID_ARG for a NULL weight. */
typedef struct dnsplat_mc_observed_args {
    dnsplat_mc_args mc;
    const float *weight;        /* device [nx,ny,nz] */
    float min_weight;           /* observed iff weight > min_weight */
} dnsplat_mc_observed_args;
size_t dnsplat_mc_observed_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);   /* 0 for an invalid size */
int dnsplat_mc_count_observed(const dnsplat_mc_observed_args *args, dnsplat_stream_t stream);
int dnsplat_mc_emit_observed(const dnsplat_mc_observed_args *args, dnsplat_stream_t stream);

/* ------------------------------------------------------------------ TSDF fusion (added after ABI 15, found by symbol)
 * The frames -> volume step of the reference's Open3DTSDFFusion exporter (export_mesh.py:931-1047; `gs-mesh o3dtsdf`, the exporter its
 * README recommends), which copies every rendered depth and colour frame to the host and fuses it there with Open3D, and the colours of
 * the mesh that dnsplat_mc_count_observed / dnsplat_mc_emit_observed extract from the volume.  The rule is restated from memory of
 * Open3D's UniformTSDFVolume::Integrate as the exporter calls it (depth_scale = 1, RGB8, convert_rgb_to_intensity = False): IT IS THIS
 * PROJECT'S DEFINITION, PARITY UNPINNED AGAINST Open3D, which is not available where this was written.  torch_tsdf.py states it in
 * PyTorch; the kernels are held to that file with exact equality.
 * Volume: tsdf and weight are float32 [nx,ny,nz], color is float32 [nx,ny,nz,3] or NULL, the last axis fastest; the sample point of
 * voxel (i, j, k) is origin + voxel * (i, j, k) in float64, the lattice coordinates of the marching cubes above.  The caller zeroes the
 * arrays once; calls accumulate.  Frames: C cameras per call, w2c float64 [C,12] = the rows of the OpenCV world-to-camera [R | t], one
 * fx, fy, cx, cy for the batch, depth float32 [C,H,W], rgb float32 [C,H,W,3] or NULL (with color: both or neither), ray_scale float32
 * [H,W] = sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1) at integer (u, v): Open3D's depth-to-camera-distance multiplier, a table so
 * that the kernel has no sqrt.  Per voxel, the cameras of the call in ascending order, no contraction:
 *   1  p_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k in float64; skip if !(p.z > 0).
 *   2  uf = ((fx p.x) / p.z + cx) + pixel_offset, vf likewise, float64; skip unless 0.0001 <= uf < W - 0.0001 and 0.0001 <= vf < H - 0.0001
 *      (a NaN skips); u = (int)uf, v = (int)vf.  pixel_offset = 0.5 is Open3D's pixel-centres-at-integers rule, i.e. the exporter as
 *      written; 0.0 matches this library's renderer, whose centres are at + 0.5.
 *   3  d = depth[c,v,u]; skip if !(d > 0) or d > depth_trunc (a NaN skips).
 *   4  in float32: sdf = (d - (float)p.z) * ray_scale[v,u]; skip if !(sdf > -sdf_trunc); f = fminf(1, sdf / sdf_trunc);
 *      tsdf = (tsdf * w + f) / (w + 1); per channel q = truncf(fminf(fmaxf(rgb * 255, 0), 255)) — the exporter's uint8 cast —
 *      color = (color * w + q) / (w + 1); w = w + 1.
 * A voxel that no frame of the call updates is not written.  One thread owns a voxel for the whole call and there are no atomics: two
 * calls with C1 and C2 cameras leave the bytes of one call with their concatenation.  One launch.
 * Returns without a launch: DNSPLAT_ERR_INVALID_ARG for NULL args / tsdf / weight / w2c / depth / ray_scale, color without rgb or rgb
 * without color, a size < 1, nx ny nz >= 2^31, or voxel, sdf_trunc or depth_trunc not > 0; DNSPLAT_ERR_UNSUPPORTED for W H > 2^31 - 1.
 * dnsplat_tsdf_vertex_colors — out[V,3] = the colour volume sampled at the lattice coordinates of `vertices` [V,3] by the trilinear
 *   formula, / 255: base corner min(floor(x), n - 2) per axis (not below 0), fraction x - base, blends (1 - f) a + f b in float32 along
 *   i, then j, then k.  On a lattice edge that is the linear blend of the edge's two ends, exact at t = 0 and t = 1.  A vertex with a
 *   non-finite coordinate gets zeros.  One launch.  DNSPLAT_ERR_INVALID_ARG for a NULL pointer, V < 0, an axis shorter than 2 or
 *   nx ny nz >= 2^31; DNSPLAT_ERR_UNSUPPORTED for V > 2^31 - 1.
 * Open3D's connected-component filter (:1021-1039) is dnsplat_mesh_clusters / dnsplat_mesh_filter_count / dnsplat_mesh_filter_emit below.
 * Out of scope: vdbfusion's space carving and its min_weight = 5 beyond the min_weight of the extraction, sparse or hashed volumes, quadric decimation, PLY output, per-camera intrinsics within one call. */
typedef struct dnsplat_tsdf_args {
    float *tsdf;                /* device [nx,ny,nz], read and written */
    float *weight;              /* device [nx,ny,nz], read and written */
    float *color;               /* NULL or device [nx,ny,nz,3], read and written */
    int32_t nx, ny, nz;
    double origin[3];
    double voxel;
    int32_t C, width, height;
    const double *w2c;          /* device [C,12] */
    double fx, fy, cx, cy;
    double pixel_offset;
    const float *depth;         /* device [C,height,width] */
    const float *rgb;           /* NULL or device [C,height,width,3] */
    const float *ray_scale;     /* device [height,width] */
    float sdf_trunc, depth_trunc;
} dnsplat_tsdf_args;
int dnsplat_tsdf_integrate(const dnsplat_tsdf_args *args, dnsplat_stream_t stream);
int dnsplat_tsdf_vertex_colors(const float *color, int32_t nx, int32_t ny, int32_t nz, const float *vertices, int64_t V, float *out,
                               dnsplat_stream_t stream);

/* ------------------------------------------------------------------ geometry scores (added after ABI 15, found by symbol)
 * The reference's point-cloud and mesh scores: PDMetrics / calculate_accuracy / calculate_completeness (metrics.py:11-56) and
 * compute_metrics with distance_p2p and get_threshold_percentage (eval/eval_mesh_vis_cull.py:290-397, the same function in
 * eval_mesh_mushroom_vis_cull.py:25-142), where the reference builds a scipy cKDTree on the CPU per direction and samples the meshes
 * with trimesh.  Everything is caller-allocated; nothing is read on the host, allocated or synchronised; no floating-point atomic:
 * equal inputs give equal bits.
 *
 * dnsplat_cloud_distances — ONE direction of distance_p2p with every scalar the callers take from it.  Per source point m of M, one
 *   thread:
 *   nearest    the target of lowest (d2, index) among the N points `index` was built over (dnsplat_knn_build), d2 as dnsplat_knn_query
 *              forms it, in DOUBLE: fma(dz, dz, fma(dy, dy, dx dx)).  A tie goes to the lowest index (scipy leaves ties unspecified).
 *   absdot     with both normal arrays: | n_src / |n_src| . n_tgt[idx] / |n_tgt[idx]| | in double, |n| = sqrt((x x + y y) + z z), the dot
 *              (a + b) + c, plain IEEE without contraction: a zero normal gives nan, as in the reference.
 *   outputs    dist2 [M] double (required: the selection reads it back), idx [M] int32 or NULL, absdot [M] double or NULL.
 *   non-finite a source point with a nan or inf coordinate reads nothing: idx = -1, dist2 = absdot = nan; it counts in N_NONFINITE and
 *              makes the means, the percentile, min and max nan (numpy's behaviour on a nan distance).  The same holds for a point
 *              that no target can be compared with: a target with a nan or inf coordinate (d2 nan or inf) is nobody's neighbour, so
 *              finite targets win over it, and where every target has one, every source point is such a row (scipy refuses the data).
 *   scalars    device double [DNSPLAT_GEOM_COUNT] at the DNSPLAT_GEOM_* indices: the means of d = sqrt(d2), of d2 and of absdot (nan
 *              without normals), the percentile, the shares d < threshold (calculate_completeness) and d <= threshold
 *              (get_threshold_percentage: precision and recall), min d, max d, and the two order statistics of d2 the percentile was
 *              interpolated from.  The unused tail is 0.
 *   counts     device int64 [DNSPLAT_GEOM_COUNTS]: n = M, the two threshold counts, the non-finite rows.
 *   percentile numpy's default method (`linear`) on d: h = (n - 1) (q / 100) in double, the order statistics of rank floor(h) and
 *              min(floor(h) + 1, n - 1) found EXACTLY by a radix selection on the 64-bit patterns of d2 (non-negative doubles order as
 *              their patterns, so the order of d2 is the order of d) in six integer histogram rounds (11 + 11 + 11 + 11 + 10 + 10 bits)
 *              for both ranks at once; then a = sqrt(lo), b = sqrt(hi), g = h - floor(h) and numpy's _lerp: g >= 0.5 ? b - (b - a) (1 - g)
 *              : a + (b - a) g, in double.  h depends on M and q alone: the ranks are arguments of the kernels.
 *   sums       one partial per workgroup of 256 points (sums in double, counts as integers), folded in a fixed order.
 *   scratch    dnsplat_cloud_distances_scratch_bytes(M) bytes (a host function; 0 for M outside 1 .. 2^31 - 1), 8-byte aligned.  No
 *              precondition on its contents, and they need not survive.
 *   One memset and thirteen launches.  Returns without a launch: DNSPLAT_ERR_INVALID_ARG for a NULL args / index / src / dist2 / scalars /
 *   counts / scratch, M < 1, N < 1, half a normal pair, a percentile outside [0, 100] (a nan included); DNSPLAT_ERR_UNSUPPORTED for
 *   M > 2^31 - 1 (N is an int32).
 *
 * dnsplat_mesh_areas — per triangle of `triangles` [T,3] int32 over `vertices` [V,3] fp32: area = |cross(v1 - v0, v2 - v0)| / 2 in double
 *   from the exactly converted vertices, and the unit face normal cross / |cross| rounded to fp32 [T,3].  A zero-area face gets normal 0;
 *   a triangle with an index outside [0, V), or with a non-finite cross product, gets area 0 and normal 0 and reads nothing out of
 *   bounds.  One launch.  The inclusive prefix sum of the areas is the caller's (any double scan; the Python layer uses torch.cumsum).
 *
 * dnsplat_mesh_sample — mesh.sample(count, return_index=True) as a canonical function of (mesh, cdf, seed).  Sample i of S, one thread:
 *   words      mix(x) = the mix32 of the pixel sampler (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16).
 *              key = mix((uint32)seed ^ mix((uint32)(seed >> 32) + 0x9e3779b9)); c = mix((uint32)i ^ key);
 *              w_k = mix(c + (k + 1) 0x9e3779b9), k = 0, 1, 2 (uint32 arithmetic): a counter-based integer hash, no state.
 *   face       t = ((double)w_0 + 0.5) / 2^32 * cdf[T - 1]; f = the first index with cdf[f] > t (binary search).  A face whose cdf entry
 *              equals its predecessor's (area 0) can therefore never be drawn.
 *   point      u = w_1 >> 8, v = w_2 >> 8; if u + v > 2^24 both are reflected to 2^24 - u, 2^24 - v; r1 = u / 2^24, r2 = v / 2^24 (exact
 *              in fp32); p = (v0 + r1 (v1 - v0)) + r2 (v2 - v0) in fp32 in that order, no contraction.
 *   outputs    points [S,3] fp32, normals [S,3] fp32 (a copy of face_normals[f]), faces [S] int32.
 *   A cdf whose last entry is not a positive finite number (no face can be drawn) gives points nan, normals 0, faces -1.  Whatever cdf is
 *   given, the vertex indices of the drawn face are tested against V before anything is read through them (point nan, normal 0, the
 *   face index kept).  One launch.  PARITY UNPINNED against trimesh, whose draws come from numpy's global generator.
 *   Returns without a launch: DNSPLAT_ERR_INVALID_ARG for NULL args / cdf / vertices / triangles / face_normals (/ an output with S > 0),
 *   S < 0, V < 1, T < 1; DNSPLAT_ERR_UNSUPPORTED for S > 2^31 - 1.  S == 0 returns 0. */
#define DNSPLAT_GEOM_MEAN_D 0          /* mean of d */
#define DNSPLAT_GEOM_MEAN_D2 1         /* mean of d^2 */
#define DNSPLAT_GEOM_MEAN_ABSDOT 2     /* mean of |n_src . n_tgt|; nan without normals */
#define DNSPLAT_GEOM_PERCENTILE 3      /* numpy.percentile(d, percentile) */
#define DNSPLAT_GEOM_SHARE_LT 4        /* share with d < threshold */
#define DNSPLAT_GEOM_SHARE_LE 5        /* share with d <= threshold */
#define DNSPLAT_GEOM_MIN_D 6
#define DNSPLAT_GEOM_MAX_D 7
#define DNSPLAT_GEOM_ORDER_LO_D2 8     /* d^2 of rank floor(h) */
#define DNSPLAT_GEOM_ORDER_HI_D2 9     /* d^2 of rank min(floor(h) + 1, n - 1) */
#define DNSPLAT_GEOM_COUNT 12
#define DNSPLAT_GEOM_N 0
#define DNSPLAT_GEOM_N_LT 1
#define DNSPLAT_GEOM_N_LE 2
#define DNSPLAT_GEOM_N_NONFINITE 3
#define DNSPLAT_GEOM_COUNTS 4
typedef struct dnsplat_cloud_distances_args {
    int32_t N;                  /* points the index was built over */
    const void *index;          /* dnsplat_knn_build's, over the TARGET points */
    int64_t M;                  /* source points */
    const float *src;           /* [M,3] */
    const float *src_normals;   /* [M,3] or NULL */
    const float *tgt_normals;   /* [N,3] or NULL; both or neither */
    double threshold;
    double percentile;          /* in [0, 100] */
    double *dist2;              /* [M] */
    int32_t *idx;               /* [M] or NULL */
    double *absdot;             /* [M] or NULL */
    double *scalars;            /* device [DNSPLAT_GEOM_COUNT] */
    int64_t *counts;            /* device [DNSPLAT_GEOM_COUNTS] */
    void *scratch;
} dnsplat_cloud_distances_args;
typedef struct dnsplat_mesh_sample_args {
    int64_t S;                  /* samples */
    uint64_t seed;
    int32_t V, T;
    const double *cdf;          /* device [T]: the inclusive prefix sums of dnsplat_mesh_areas' areas */
    const float *vertices;      /* [V,3] */
    const int32_t *triangles;   /* [T,3] */
    const float *face_normals;  /* [T,3] of dnsplat_mesh_areas */
    float *points;              /* [S,3] */
    float *normals;             /* [S,3] */
    int32_t *faces;             /* [S] */
} dnsplat_mesh_sample_args;
size_t dnsplat_cloud_distances_scratch_bytes(int64_t M);   /* 0 for an invalid size */
int dnsplat_cloud_distances(const dnsplat_cloud_distances_args *args, dnsplat_stream_t stream);
int dnsplat_mesh_areas(int32_t V, const float *vertices, int32_t T, const int32_t *triangles, double *areas, float *face_normals,
                       dnsplat_stream_t stream);
int dnsplat_mesh_sample(const dnsplat_mesh_sample_args *args, dnsplat_stream_t stream);

/* ------------------------------------------------------------------ mesh visibility culling (added after ABI 15, found by symbol)
 * cull_mesh of the reference (eval/eval_mesh_vis_cull.py:176-266, the step in front of compute_metrics): the double-sided depth renders
 * of the mesh (pyrender through OpenGL there), the per-vertex votes of cull_from_one_pose summed over the poses, the triangle rule with
 * remove_unreferenced_vertices.  Everything is caller-allocated; nothing is read on the host, allocated or synchronised; no
 * floating-point atomic: equal inputs give equal bits.  Double arithmetic, every sum associated as written, no contraction.
 * w2c is device double [C,12]: the rows of the OpenCV world-to-camera [R | t] per camera (the binding derives it from the reference's
 * OpenGL camera-to-world poses: columns 1 and 2 negated, then the analytic inverse).
 *
 * dnsplat_mesh_depth — depth[c][v][u] (float32 [C,H,W]) = the smallest camera-space z in [znear, zfar] at which the ray through the pixel
 *   centre (u + 0.5, v + 0.5) meets a triangle, either winding; 0 where there is none.  Per (camera, triangle):
 *   p_i = ((R_k0 x + R_k1 y) + R_k2 z) + t_k from the exactly converted vertices; c0 = p1 x p2, c1 = p2 x p0, c2 = p0 x p1,
 *   n = (c1 + c2) + c0, D = (p0.x c0.x + p0.y c0.y) + p0.z c0.z.  Per pixel: d = (((u + 0.5) - cx) / fx, ((v + 0.5) - cy) / fy),
 *   E_i = (c_i.x d.x + c_i.y d.y) + c_i.z and S likewise from n; inside iff (every E_i >= 0 or every E_i <= 0) and S != 0; z = D / S;
 *   a hit iff znear <= z <= zfar; the map holds the minimum of float32(z), taken as an unsigned integer minimum of its bits (the
 *   buffer starts as +inf; a last pass writes 0 where +inf remained).  Triangles crossing z = 0 need no clipping: their z is rejected.
 *   Swapping two indices of a triangle changes no bit; neither does the order of the triangles.  A triangle with an index outside
 *   [0, V), a repeated index, a non-finite vertex or an area (dnsplat_mesh_areas') that is not positive and finite covers nothing.
 *   Each triangle searches a pixel box that bounds its part with z >= znear, widened by a pixel: a search window, not part of the result.
 *   scratch: dnsplat_mesh_depth_scratch_bytes(width, height) bytes, 8-byte aligned (the pixel rays).  stats: NULL, or device uint64 [3]
 *   to which the call ADDS {triangle setups with a non-empty box, accepted fragments, issued atomics} (a measurement aid).
 *   Four launches.  PARITY UNPINNED against pyrender, whose 24-bit z-buffer quantises what this states exactly.
 *   Returns without a launch: DNSPLAT_ERR_INVALID_ARG for a NULL args / vertices / triangles / w2c / depth / scratch, V, T, C, width or
 *   height < 1, fx or fy 0 or nan, not 0 < znear <= zfar < inf; DNSPLAT_ERR_UNSUPPORTED for width height > 2^31 - 1 or C > 65535;
 *   DNSPLAT_ERR_WORKSPACE for a misaligned scratch.
 *
 * dnsplat_mesh_visibility — get_grid_culling_pattern: per vertex, one thread, over the C cameras: p as above,
 *   q_k = (K_k0 p.x + K_k1 p.y) + K_k2 p.z, pz = q_2 + 1e-8, px = q_0 / pz, py = q_1 / pz;
 *   in_frustum = 0 <= px <= W - 1 and 0 <= py <= H - 1 and pz > 0; u, v = px, py truncated;
 *   obs += in_frustum and (remove_occlusion ? pz < (double)(rendered[c][v][u] + 0.02f) : 1)     (numpy adds to a float32 map in float32)
 *   invalid += in_frustum and remove_missing_depth and depth_gt[c][v][u] <= 0.
 *   obs / invalid are int32 [V] and ACCUMULATE: the caller zeroes them once and chains camera batches.  One launch.
 *   Returns without a launch: DNSPLAT_ERR_INVALID_ARG for a NULL args / vertices / w2c / obs / invalid, a map whose flag is set and
 *   whose pointer is NULL, V, C, width or height < 1; DNSPLAT_ERR_UNSUPPORTED for width height > 2^31 - 1.
 *
 * dnsplat_mesh_cut_count / dnsplat_mesh_cut_emit — the rule of :251-260 and remove_unreferenced_vertices.  A triangle is kept iff some
 *   vertex has obs > obs_threshold and not every vertex has (double)invalid > invalid_share * (double)obs; a triangle with an index
 *   outside [0, V) is not kept.  Kept triangles stay in their order, the vertices they reference stay in theirs, indices are remapped.
 *   count: counts = {V', T'} (device int64 [2]) and the marks, flags and scanned block counts in scratch
 *   (dnsplat_mesh_cut_scratch_bytes(V, T) bytes, 4-byte aligned).  One memset and three launches.
 *   emit, after count with the same arguments: the first min(V', cap_v) vertices and min(T', cap_t) triangles, nothing past a capacity;
 *   *status = DNSPLAT_MESH_CUT_STATUS_VERTICES if V' > cap_v | DNSPLAT_MESH_CUT_STATUS_TRIANGLES if T' > cap_t.  Two launches; it may
 *   be repeated.  Integers only, no atomics.  Returns without a launch: DNSPLAT_ERR_INVALID_ARG for a NULL args / vertices / triangles /
 *   obs / invalid / scratch / counts (emit: / status, / a buffer whose capacity is positive), V or T < 1, a negative capacity;
 *   DNSPLAT_ERR_WORKSPACE for a short or misaligned scratch. */
#define DNSPLAT_MESH_CUT_STATUS_VERTICES 1
#define DNSPLAT_MESH_CUT_STATUS_TRIANGLES 2
typedef struct dnsplat_mesh_depth_args {
    int32_t V, T, C;
    int32_t width, height;
    const float *vertices;      /* [V,3] */
    const int32_t *triangles;   /* [T,3] */
    const double *w2c;          /* [C,12] */
    double fx, fy, cx, cy;
    double znear, zfar;
    float *depth;               /* [C,height,width] */
    void *scratch;
    uint64_t *stats;            /* NULL or device [3], added to */
} dnsplat_mesh_depth_args;
typedef struct dnsplat_mesh_visibility_args {
    int32_t V, C;
    int32_t width, height;
    const float *vertices;      /* [V,3] */
    const double *w2c;          /* [C,12] */
    double K[9];                /* row-major 3x3 */
    const float *rendered;      /* [C,height,width]; read iff remove_occlusion */
    const float *depth_gt;      /* [C,height,width]; read iff remove_missing_depth */
    int32_t remove_occlusion, remove_missing_depth;
    int32_t *obs;               /* [V], added to */
    int32_t *invalid;           /* [V], added to */
} dnsplat_mesh_visibility_args;
typedef struct dnsplat_mesh_cut_args {
    int32_t V, T;
    const float *vertices;      /* [V,3] */
    const int32_t *triangles;   /* [T,3] */
    const int32_t *obs;         /* [V] */
    const int32_t *invalid;     /* [V] */
    int32_t obs_threshold;      /* the reference: 3 */
    double invalid_share;       /* the reference: 0.7 */
    void *scratch;
    size_t scratch_bytes;
    int64_t *counts;            /* device int64 [2]: V', T'; written by count, read by emit */
    int64_t cap_v, cap_t;       /* emit: rows of out_vertices / out_triangles */
    float *out_vertices;        /* emit: [cap_v,3] */
    int32_t *out_triangles;     /* emit: [cap_t,3] */
    int32_t *status;            /* emit: device int32 [1] */
} dnsplat_mesh_cut_args;
size_t dnsplat_mesh_depth_scratch_bytes(int32_t width, int32_t height);   /* 0 for an invalid size */
int dnsplat_mesh_depth(const dnsplat_mesh_depth_args *args, dnsplat_stream_t stream);
int dnsplat_mesh_visibility(const dnsplat_mesh_visibility_args *args, dnsplat_stream_t stream);
size_t dnsplat_mesh_cut_scratch_bytes(int32_t V, int32_t T);   /* 0 for an invalid size */
int dnsplat_mesh_cut_count(const dnsplat_mesh_cut_args *args, dnsplat_stream_t stream);
int dnsplat_mesh_cut_emit(const dnsplat_mesh_cut_args *args, dnsplat_stream_t stream);

/* ------------------------------------------------------------------ mesh cluster filter (added after ABI 15, found by symbol)
 * The step the reference's recommended exporter ends with (Open3DTSDFFusion, export_mesh.py:1021-1039): Open3D's
 * cluster_connected_triangles, n = max(np.sort(cluster_n_triangles)[-50], 50), every triangle of a cluster with fewer than n triangles
 * removed, remove_unreferenced_vertices, remove_degenerate_triangles.  Topology only: triangle indices in, integers out.  Open3D is not
 * at hand: the rule below is restated from its documented behaviour, IT IS THIS PROJECT'S DEFINITION, PARITY UNPINNED AGAINST Open3D.
 * Everything is caller-allocated; nothing is read on the host, allocated or synchronised; integers only, no floating-point atomic:
 * the output is a canonical function of (triangles, V, keep_largest, min_triangles) — equal inputs give equal bytes, whatever the order
 * in which the atomics land.  triangles is int32 [T,3] over V vertices.
 *   valid      a triangle is valid iff all three indices are in [0, V).  An invalid one belongs to no cluster, has label -1 and is never
 *              kept.
 *   edges      a valid triangle (a, b, c) has the undirected edges {a,b}, {b,c}, {c,a}; an edge with equal ends is ignored.
 *   connection two valid triangles are connected iff they share an undirected edge (Open3D: "connected via edges").  A shared vertex
 *              alone does not connect; winding does not matter; duplicate rows are connected; an edge that three or more triangles
 *              share connects all of them.
 *   clusters   the connected components.  A cluster's root is its lowest triangle index; clusters are numbered 0 .. n_clusters - 1 in
 *              ascending order of root — the order a breadth-first search from triangle 0 upwards discovers them in, as Open3D's does.
 *              labels[t] is the number of t's cluster, sizes[c] the number of its valid triangles, degenerate ones (a repeated index)
 *              included.  cluster_area, the third result of Open3D's call, is not produced: the reference's filter never reads it.
 *   threshold  with n_clusters >= keep_largest: max(min_triangles, the keep_largest-th largest of sizes); with fewer clusters:
 *              min_triangles (there the reference's [-50] raises IndexError; this is defined).  The reference's values are 50 and 50.
 *   kept       a triangle is kept iff it is valid, has three distinct indices and sizes[labels[t]] >= threshold: ties at the threshold
 *              are all kept (the reference removes with <).  A vertex is kept iff a kept triangle references it.  ONE DEVIATION: Open3D
 *              compacts the vertices before it drops degenerate triangles and can leave a vertex only a degenerate triangle
 *              referenced; this leaves none.  Kept triangles and kept vertices stay in their order, indices are remapped: the
 *              convention of dnsplat_mesh_cut_count / dnsplat_mesh_cut_emit.
 *
 * dnsplat_mesh_clusters — labels int32 [T], sizes int32 [T] (rows n_clusters and up are written 0), counts device int64 [2] =
 *   {n_clusters, the number of valid triangles}, status device int32 [1]: 0, or DNSPLAT_MESH_CLUSTERS_STATUS_INTERNAL if a bounded loop
 *   (a probe of the edge table, at most its capacity; a walk to a root, at most T links; a union, at most T rounds) ran out — which
 *   cannot happen on a correct build; the outputs mean nothing then.  An open-addressing table of the edges (64-bit keys claimed by
 *   compare-and-swap, the lowest triangle of each edge by an integer minimum), a union-find whose only write is an integer minimum,
 *   a flatten, a scan.  scratch: dnsplat_mesh_clusters_scratch_bytes(V, T) bytes, 8-byte aligned — 60 bytes per triangle (a table of 4 T
 *   slots of 12 bytes, a load of at most 0.75 when all 3 T edges are distinct, and three int32 per triangle) + 4 per 256 triangles + 8;
 *   0 for V < 1, T < 1 or T > (2^31 - 1) / 4, where the table leaves its int32 index.  No precondition on its contents, and they need
 *   not survive.  Eight launches.
 * dnsplat_mesh_filter_count — from labels, sizes and the DEVICE counts of dnsplat_mesh_clusters (cluster_counts; n_clusters is never
 *   read on the host): threshold device int32 [1] by a radix selection on the sizes (three integer histogram rounds), counts device
 *   int64 [2] = {V', T'}, and the marks, flags and scanned block counts in scratch (dnsplat_mesh_filter_scratch_bytes(V, T) bytes, 8-byte
 *   aligned).  One memset and nine launches.
 * dnsplat_mesh_filter_emit — after count with the same arguments: vertex_index int32 [V'], the old id of each kept vertex (any
 *   per-vertex attribute — float64 world positions, float32 lattice positions, colours — is gathered with it; NO coordinates are
 *   written), and the remapped triangles int32 [T',3]; the first min(V', cap_v) / min(T', cap_t) rows, nothing past a capacity;
 *   *status = DNSPLAT_MESH_FILTER_STATUS_VERTICES if V' > cap_v | DNSPLAT_MESH_FILTER_STATUS_TRIANGLES if T' > cap_t.  Two launches; it
 *   may be repeated.
 * All three return without touching the device: DNSPLAT_ERR_INVALID_ARG for a NULL args or a NULL required pointer (emit: / status,
 * / a buffer whose capacity is positive), V < 1, T < 1, keep_largest < 1, min_triangles < 1, a negative capacity;
 * DNSPLAT_ERR_UNSUPPORTED for T > (2^31 - 1) / 4 (clusters); DNSPLAT_ERR_WORKSPACE for a short or misaligned scratch.
 * Out of scope: cluster_area, vertex merging by position (the clusters are over indices; dnsplat_mc_emit writes one vertex per lattice
 * edge, so its meshes need none), quadric decimation, PLY output. */
#define DNSPLAT_MESH_CLUSTERS_STATUS_INTERNAL 1
#define DNSPLAT_MESH_FILTER_STATUS_VERTICES 1
#define DNSPLAT_MESH_FILTER_STATUS_TRIANGLES 2
typedef struct dnsplat_mesh_clusters_args {
    int32_t V, T;
    const int32_t *triangles;   /* [T,3] */
    void *scratch;
    size_t scratch_bytes;
    int32_t *labels;            /* [T] */
    int32_t *sizes;             /* [T] */
    int64_t *counts;            /* device int64 [2]: n_clusters, valid triangles */
    int32_t *status;            /* device int32 [1] */
} dnsplat_mesh_clusters_args;
typedef struct dnsplat_mesh_filter_args {
    int32_t V, T;
    const int32_t *triangles;   /* [T,3] */
    const int32_t *labels;      /* [T] of dnsplat_mesh_clusters */
    const int32_t *sizes;       /* [T] of dnsplat_mesh_clusters */
    const int64_t *cluster_counts; /* device int64 [2] of dnsplat_mesh_clusters */
    int32_t keep_largest;       /* the reference: 50 */
    int32_t min_triangles;      /* the reference: 50 */
    void *scratch;
    size_t scratch_bytes;
    int32_t *threshold;         /* device int32 [1]; written by count */
    int64_t *counts;            /* device int64 [2]: V', T'; written by count, read by emit */
    int64_t cap_v, cap_t;       /* emit: rows of vertex_index / out_triangles */
    int32_t *vertex_index;      /* emit: [cap_v] */
    int32_t *out_triangles;     /* emit: [cap_t,3] */
    int32_t *status;            /* emit: device int32 [1] */
} dnsplat_mesh_filter_args;
size_t dnsplat_mesh_clusters_scratch_bytes(int32_t V, int32_t T);   /* 0 for an invalid size */
int dnsplat_mesh_clusters(const dnsplat_mesh_clusters_args *args, dnsplat_stream_t stream);
size_t dnsplat_mesh_filter_scratch_bytes(int32_t V, int32_t T);     /* 0 for an invalid size */
int dnsplat_mesh_filter_count(const dnsplat_mesh_filter_args *args, dnsplat_stream_t stream);
int dnsplat_mesh_filter_emit(const dnsplat_mesh_filter_args *args, dnsplat_stream_t stream);

/* ------------------------------------------------------------------ point-cloud filters (added after ABI 15, found by symbol)
 * The two Open3D filters the reference runs on the CPU between the clouds and their consumers: remove_statistical_outlier(
 * nb_neighbors = 20, std_ratio), the last step before the solver of GaussiansToPoisson, DepthAndNormalMapsPoisson and LevelSetExtractor
 * (export_mesh.py:287-291, :487-491, :640), and voxel_down_sample(voxel_size) (eval_pd.py:82 before calculate_accuracy /
 * calculate_completeness; export_mesh.py:284-285).  Open3D is not at hand: both rules are restated from memory of
 * PointCloud::RemoveStatisticalOutliers and PointCloud::VoxelDownSample, THEY ARE THIS PROJECT'S DEFINITION, PARITY UNPINNED AGAINST Open3D.
 * Everything is caller-allocated; nothing is read on the host, allocated or synchronised; no floating-point atomic: equal inputs give
 * equal bytes.
 *
 * STATISTICAL OUTLIER REMOVAL of points fp32 [N,3] with `index` = dnsplat_knn_build over the SAME points.  K = min(nb_neighbors, N).
 *   avg        avg[i] = (sqrt(d2_0) + sqrt(d2_1) + ... + sqrt(d2_{K-1})) / K over the K nearest points under dnsplat_knn_query's key
 *              (d2, index) with d2 in double — the point itself included, so the first term is 0 — the square roots in double and
 *              correctly rounded (IEEE), added in ascending rank from 0.  A row with a non-finite coordinate gets avg = -1: it is not valid, nobody's neighbour and never
 *              kept.  With fewer than K comparable points the missing ranks have d2 = inf.
 *   moments    n_valid = the rows with avg >= 0 (those that were searched); sum = the sum of avg over avg > 0; mean = sum / n_valid;
 *              std = sqrt((the sum of (avg - mean)^2 over avg > 0) / (n_valid - 1)); threshold = mean + std_ratio * std.  Two folds in
 *              double in the one fixed order of the score kernels (per block of 256 rows, then the partials), the second after the first
 *              has finished, as Open3D's two passes.  With n_valid <= 1: std = 0 and threshold = 0 (mean = 0 with n_valid = 0).
 *   kept       row i iff avg[i] > 0 && avg[i] < threshold.  The kept indices ascend: Open3D's `ind`.
 * dnsplat_cloud_neighbor_mean — avg double [N].  One launch, one thread per point.  nb_neighbors < 1: DNSPLAT_ERR_INVALID_ARG; above
 *   DNSPLAT_KNN_MAX_K: DNSPLAT_ERR_UNSUPPORTED.
 * dnsplat_cloud_outlier_stats — from avg (any double [N] under the conventions above): the record `stats`, device, 64 bytes, 8-byte
 *   aligned: double {mean, std, threshold, sum}, int64 {n_valid, n_kept, 0, 0}.  n_kept is written 0.  Four launches.
 * dnsplat_cloud_outlier_count — stats.n_kept, and the scanned kept rows per block in scratch; threshold is read on the device.  Two launches.
 * dnsplat_cloud_outlier_emit — after count with the same arguments: ind int64, the first min(n_kept, capacity) kept indices, nothing past
 *   the capacity.  One launch; it may be repeated.
 * scratch: dnsplat_cloud_outlier_scratch_bytes(N) bytes, 8-byte aligned (36 per 256 points; 0 for N < 1); neighbor_mean needs none.
 * All four return without touching the device: DNSPLAT_ERR_INVALID_ARG for a NULL args or a NULL required pointer, N < 1, a nan
 * std_ratio (stats), a negative capacity or a positive one without ind (emit); DNSPLAT_ERR_WORKSPACE for a short or misaligned scratch.
 *
 * VOXEL DOWN-SAMPLING of points fp32 [N,3] with optional normals and colors fp32 [N,3]; all arithmetic in double.
 *   voxel      lo[a] = min_i p[i][a] - voxel_size / 2;  ref = (p - lo) / voxel_size;  idx = floor(ref) per axis.  idx[a] >= 2^21 sets
 *              DNSPLAT_VOXEL_STATUS_EXTENT (the three indices pack into one 63-bit key), a non-finite coordinate
 *              DNSPLAT_VOXEL_STATUS_NONFINITE.
 *   order      voxels are numbered in order of first appearance: v precedes w iff its lowest point index is lower.  (Open3D's order is
 *              that of a hash map.)
 *   mean       an exact integer sum: a position adds q = llrint((ref - idx) * 2^31) per axis to an int64 S, the voxel's n points are
 *              counted, and p' = (lo + idx * voxel_size) + (voxel_size * ((double)S / n)) / 2^31.  A normal or colour component c adds
 *              llrint(c * 2^30); |c| > 2 or a nan sets DNSPLAT_VOXEL_STATUS_ATTRIBUTE; the mean is ((double)S / n) / 2^30, NOT
 *              re-normalised, as in Open3D.  With N < 2^31 no sum overflows.
 * dnsplat_voxel_count — counts device int64 [2] = {V, status} and voxel_of int32 [N], the voxel of each point (-1 for a row that has
 *   none under a non-zero status; the outputs mean nothing then).  An open-addressing table of 2 N slots (64-bit keys claimed by
 *   compare-and-swap, each voxel's lowest point by an integer minimum), a flag-and-scan over the points that numbers the voxels, integer
 *   sums per voxel — added once per voxel per wave where lanes share one.  Every probe is bounded by the table;
 *   DNSPLAT_VOXEL_STATUS_INTERNAL if one ran out, which cannot happen on a correct build.  Eight launches.
 * dnsplat_voxel_emit — after count with the same arguments: the first min(V, cap_v) rows of out_points / out_normals / out_colors double
 *   [cap_v,3] and out_counts int32 [cap_v] (may be NULL).  One launch; it may be repeated.
 * scratch: dnsplat_voxel_scratch_bytes(N, the number of attribute arrays) bytes, 8-byte aligned: 32 + 28 N + 8 (4 + 3 attributes) N +
 *   4 per 256 points + 3072; 0 for N < 1, N > (2^31 - 1) / 2 or attributes outside [0, 2].
 * Both return without touching the device: DNSPLAT_ERR_INVALID_ARG for a NULL args or required pointer, N < 1, voxel_size not in
 * (0, inf), a negative cap_v or a positive one without the buffer of an array that was given; DNSPLAT_ERR_UNSUPPORTED for
 * N > (2^31 - 1) / 2; DNSPLAT_ERR_WORKSPACE for a short or misaligned scratch.
 * Out of scope: remove_radius_outlier, voxel_down_sample_and_trace's matrix form, PLY input and output. */
#define DNSPLAT_CLOUD_OUTLIER_STATS_BYTES 64
#define DNSPLAT_VOXEL_STATUS_INTERNAL 1
#define DNSPLAT_VOXEL_STATUS_NONFINITE 2
#define DNSPLAT_VOXEL_STATUS_EXTENT 4
#define DNSPLAT_VOXEL_STATUS_ATTRIBUTE 8
typedef struct dnsplat_cloud_outlier_args {
    int32_t N;
    int32_t nb_neighbors;       /* neighbor_mean; Open3D's callers: 20 */
    const float *points;        /* neighbor_mean: [N,3] */
    const void *index;          /* neighbor_mean: dnsplat_knn_build's, over the same points */
    double std_ratio;           /* stats */
    void *scratch;
    size_t scratch_bytes;
    double *avg;                /* [N]; written by neighbor_mean, read by the others */
    void *stats;                /* device, DNSPLAT_CLOUD_OUTLIER_STATS_BYTES */
    int64_t capacity;           /* emit: rows of ind */
    int64_t *ind;               /* emit: [capacity] */
} dnsplat_cloud_outlier_args;
typedef struct dnsplat_voxel_args {
    int32_t N;
    const float *points;        /* [N,3] */
    const float *normals;       /* [N,3] or NULL */
    const float *colors;        /* [N,3] or NULL */
    double voxel_size;
    void *scratch;
    size_t scratch_bytes;
    int64_t *counts;            /* device int64 [2]: V, status */
    int32_t *voxel_of;          /* [N] */
    int64_t cap_v;              /* emit: rows of the outputs */
    double *out_points;         /* emit: [cap_v,3] */
    double *out_normals;        /* emit: [cap_v,3] with normals */
    double *out_colors;         /* emit: [cap_v,3] with colors */
    int32_t *out_counts;        /* emit: [cap_v] or NULL */
} dnsplat_voxel_args;
size_t dnsplat_cloud_outlier_scratch_bytes(int32_t N);   /* 0 for an invalid size */
int dnsplat_cloud_neighbor_mean(const dnsplat_cloud_outlier_args *args, dnsplat_stream_t stream);
int dnsplat_cloud_outlier_stats(const dnsplat_cloud_outlier_args *args, dnsplat_stream_t stream);
int dnsplat_cloud_outlier_count(const dnsplat_cloud_outlier_args *args, dnsplat_stream_t stream);
int dnsplat_cloud_outlier_emit(const dnsplat_cloud_outlier_args *args, dnsplat_stream_t stream);
size_t dnsplat_voxel_scratch_bytes(int32_t N, int32_t n_attributes);   /* 0 for an invalid size */
int dnsplat_voxel_count(const dnsplat_voxel_args *args, dnsplat_stream_t stream);
int dnsplat_voxel_emit(const dnsplat_voxel_args *args, dnsplat_stream_t stream);

/* ------------------------------------------------------------------ mesh alignment: point-to-point ICP (added after ABI 15, found by symbol)
 * get_align_transformation (eval/eval_mesh_vis_cull.py:269-287, called at :427-431): Open3D's registration_icp(source, target,
 * threshold = 0.1, identity, TransformationEstimationPointToPoint) of the predicted mesh's vertices onto the ground truth's, whose
 * result main() applies to the predicted mesh before it culls and scores both.  Open3D is not at hand: the rule is restated from memory
 * of RegistrationICP / GetRegistrationResultAndCorrespondences / Eigen::umeyama(..., with_scaling = false), IT IS THIS PROJECT'S
 * DEFINITION, PARITY UNPINNED AGAINST Open3D.  Everything is caller-allocated; the host reads nothing, allocates nothing and never
 * synchronises; no floating-point atomic, every loop bounded by its sizes: equal inputs give equal bytes.
 *
 * Inputs: source points s_m fp32 [M,3]; the target points g fp32 [N,3] with `index` = dnsplat_knn_build over them; r = max_dist;
 * a start transform T_0, 4 x 4 double row-major (identity when NULL); relative_fitness, relative_rmse (Open3D: 1e-6), max_iteration (30).
 *   transform  THE RULE, for q and for dnsplat_transform_points: coordinate a of T p is ((T[a][0] x + T[a][1] y) + T[a][2] z) + T[a][3]
 *              in double, plain IEEE without contraction, then ONE rounding to fp32; a rotation alone drops the last term.
 * PASS k = 0, 1, ... on the accumulated T_k:
 *   1 q_m = fl32(T_k s_m).  Every pass transforms the ORIGINAL source by the accumulated T_k.  (Open3D transforms the already
 *     transformed cloud again by each update, so its roundings pile up in the points; ours do not.)
 *   2 row m is a correspondence iff the search of dnsplat_knn_query finds a nearest target j(m) of q_m — lowest (d2, index), d2 =
 *     fma(dz, dz, fma(dy, dy, dx dx)) in double — and d2 <= r * r, the product taken in double.  A source row with a non-finite
 *     coordinate (or whose q is not finite) is never a correspondence and still counts in M.
 *   3 n_k = the correspondences; fitness_k = n_k / M; rmse_k = sqrt((sum of d2) / n_k), 0 when n_k == 0.
 *   4 stop, T_k is the result, when  n_k == 0 (status |= DNSPLAT_ICP_STATUS_NO_CORRESPONDENCE),  or  k == max_iteration,  or
 *     k >= 1 && |fitness_k - fitness_{k-1}| < relative_fitness && |rmse_k - rmse_{k-1}| < relative_rmse.
 *   5 otherwise T_{k+1} = U_k T_k, rows ((R[a][0] T[0][b] + R[a][1] T[1][b]) + R[a][2] T[2][b]) (+ t[a] for b = 3), U_k = [R t] the
 *     Umeyama / Kabsch solve of the pairs (q, g) without scale: with the means mu_q, mu_g and Sigma = (1 / n) sum (g - mu_g)(q - mu_q)^T,
 *     R is the proper rotation (det = +1) that maximises tr(R^T Sigma) and t = mu_g - R mu_q.
 * moments    per workgroup of 256 rows one partial: n as an int64, and in double the sums of d2, q - c (3), g - c (3) and
 *            (g - c)(q - c)^T (9), c = (lo + hi) * 0.5 the centre of the index's bounding box (lo, hi the fp32 extremes of the target,
 *            the sum and the product in double): the raw moments do not cancel against the scene's offset.  The partials are added in
 *            the one fixed order of the score kernels.  mu_q - c = S_q / n, mu_g - c = S_g / n,
 *            Sigma[a][b] = S_gq[a][b] / n - (S_g[a] / n) (S_q[b] / n).
 * solve      Horn's closed form (J. Opt. Soc. Am. A 4, 1987): the unit quaternion (w, x, y, z) of R is the eigenvector of the largest
 *            eigenvalue of the symmetric 4 x 4 matrix, with S_xy = Sigma[1][0] (the source's x against the target's y) and so on,
 *              [ (Sxx+Syy)+Szz  Syz-Szy        Szx-Sxz        Sxy-Syx       ]
 *              [ .              (Sxx-Syy)-Szz  Sxy+Syx        Szx+Sxz       ]
 *              [ .              .              (Syy-Sxx)-Szz  Syz+Szy       ]
 *              [ .              .              .              (Szz-Sxx)-Syy ]
 *            a proper rotation by construction.  Eigenvectors by a cyclic Jacobi: exactly 10 sweeps over the planes (0,1) (0,2) (0,3)
 *            (1,2) (1,3) (2,3), V = I at the start.  A plane with a_pq == 0 is skipped; otherwise theta = (a_qq - a_pp) / (2 a_pq),
 *            t = sign(theta) / (|theta| + sqrt(theta theta + 1)) with sign(0) = +1, c = 1 / sqrt(t t + 1), s = t c;
 *            a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0; for the other rows r: (a_rp, a_rq) <- (c a_rp - s a_rq, s a_rp + c a_rq), both
 *            triangles kept; for every row r of V: (v_rp, v_rq) <- (c v_rp - s v_rq, s v_rp + c v_rq).  Only + - * / sqrt.  The
 *            eigenvalues are the diagonal; l1 is the largest and l2 the largest of the rest, ties to the lower column.  The column of
 *            l1 is divided by its length sqrt(((w w + x x) + y y) + z z);
 *              R = [ 1 - 2 (y y + z z)   2 (x y - w z)       2 (x z + w y)     ]
 *                  [ 2 (x y + w z)       1 - 2 (x x + z z)   2 (y z - w x)     ]
 *                  [ 2 (x z - w y)       2 (y z + w x)       1 - 2 (x x + y y) ]
 *            t[a] = (S_g[a] / n + c[a]) - ((R[a][0] m0 + R[a][1] m1) + R[a][2] m2), m = S_q / n + c.
 *            With the singular values sigma_1 >= sigma_2 >= sigma_3 of Sigma and s = sign(det Sigma): l1 - l2 = 2 (sigma_2 + s sigma_3)
 *            and l1 + l2 = 2 sigma_1.  status |= DNSPLAT_ICP_STATUS_DEGENERATE (advisory: the rotation is not determined; the pass
 *            proceeds) when (l1 - l2) * 0.5 <= 2^-26 * ((l1 + l2) * 0.5).  A zero Sigma (one pair) gives R = I, a pure translation.
 * state      device, DNSPLAT_ICP_STATE_BYTES, 8-byte aligned: double T[16] (row-major), fitness, rmse (of the last pass that ran);
 *            int64 n, iterations (the k of the result: updates applied), done, status (0 on success), passes (rows of trace written), 0.
 * dnsplat_icp_begin — writes the state: T = init (it travels as a kernel argument; NULL: identity), the rest 0.  One launch.
 * dnsplat_icp_iterate — one pass on whatever T the state holds: icp_corr_kernel (one thread per source row) and icp_solve_kernel (one
 *   workgroup).  Both read `done` first and return at once when it is set.  Optional outputs: idx int32 [M] (-1: no correspondence) and
 *   dist2 double [M] (nan likewise) of the LAST pass that ran; trace double [max_iteration + 1][4], row k = (n_k, fitness_k, rmse_k,
 *   stopped) — the rows past `passes` are not written.
 * dnsplat_icp_run — begin, then max_iteration + 1 iterates: 3 + 2 max_iteration launches, the idle ones return at their first load.
 * dnsplat_transform_points — out fp32 [N,3] = fl32(T p) under the rule above, T device double [16] (the head of a state is one); with
 *   rotate_only the rotation block alone, for normals.  N = 0 is a no-op.  One launch.
 * dnsplat_knn_points — out fp32 [N,3]: the points `index` was built over, in their own order, bit for bit, from its sorted copy.  N MUST be
 *   the N of that dnsplat_knn_build: the buffer does not record it and nothing here can check it.  With another N the sorted copy is looked
 *   for at the wrong offset of the buffer; rows whose index word is outside [0, N) are skipped, so nothing is written outside `out`, but
 *   what is written means nothing (and the read may leave a buffer that was sized for a smaller N).  One launch.
 * scratch: dnsplat_icp_scratch_bytes(M) = 136 ceil(M / 256) bytes, 8-byte aligned; 0 for M < 1 or M > 2^31 - 1.
 * All return before a device is touched: DNSPLAT_ERR_INVALID_ARG for a NULL args or required pointer, M < 1, N < 1, max_dist not in
 * (0, inf), a nan tolerance, max_iteration < 0, a non-finite init; DNSPLAT_ERR_UNSUPPORTED for M > 2^31 - 1; DNSPLAT_ERR_WORKSPACE for
 * a short or misaligned scratch or a misaligned state.
 * Out of scope: point-to-plane and coloured ICP, scaling, RANSAC / global registration, mesh file input and output. */
#define DNSPLAT_ICP_STATE_BYTES 192
#define DNSPLAT_ICP_STATUS_NO_CORRESPONDENCE 1
#define DNSPLAT_ICP_STATUS_DEGENERATE 2
typedef struct dnsplat_icp_args {
    int64_t M;                  /* source points */
    const float *source;        /* [M,3] */
    int32_t N;                  /* points the index was built over */
    const float *target;        /* [N,3], the points themselves */
    const void *index;          /* dnsplat_knn_build's, over the target */
    double max_dist;            /* r */
    double relative_fitness;
    double relative_rmse;
    int32_t max_iteration;
    void *state;                /* device, DNSPLAT_ICP_STATE_BYTES */
    double *trace;              /* [max_iteration + 1][4] or NULL */
    int32_t *idx;               /* [M] or NULL */
    double *dist2;              /* [M] or NULL */
    void *scratch;
    size_t scratch_bytes;
} dnsplat_icp_args;
size_t dnsplat_icp_scratch_bytes(int64_t M);   /* 0 for an invalid size */
int dnsplat_icp_begin(const dnsplat_icp_args *args, const double *init16_host_or_null, dnsplat_stream_t stream);
int dnsplat_icp_iterate(const dnsplat_icp_args *args, dnsplat_stream_t stream);
int dnsplat_icp_run(const dnsplat_icp_args *args, const double *init16_host_or_null, dnsplat_stream_t stream);
int dnsplat_transform_points(int64_t N, const float *p, const double *T_device, float *out, int rotate_only, dnsplat_stream_t stream);
int dnsplat_knn_points(int32_t N, const void *index, float *out, dnsplat_stream_t stream);

/* ------------------------------------------------------------------ mesh subdivision (added after ABI 15, found by symbol)
 * The first step of the reference's cull_mesh (eval_mesh_vis_cull.py:190-193, subdivide=True for both meshes at :439-464):
 * trimesh.remesh.subdivide_to_size(vertices, triangles, max_edge = 0.015, max_iter = 10).  The cull votes per vertex and keeps a
 * triangle if one of its vertices was seen often enough, so a wall triangle metres long survives on one visible corner unless it is
 * split first.  trimesh is not at hand and the reference holds no code for the step: the rule below is restated from trimesh's
 * documented behaviour, IT IS THIS PROJECT'S DEFINITION, PARITY UNPINNED AGAINST trimesh.  torch_subdivide.py restates it on the CPU
 * and the kernels are held to that file with exact equality.
 *   state      the current vertices cv double [Vc,3], the current triangles cf int32 [Tc,3] and the origin ci int32 [Tc] of each
 *              current triangle, at first arange(T).  float32 vertices are promoted exactly; all arithmetic and all outputs are double.
 *   a round    r = 0 .. max_iter, ONE dnsplat_subdivide_count and ONE dnsplat_subdivide_emit:
 *   lengths    per triangle and per edge e (0: 0->1, 1: 1->2, 2: 2->0), d = b - a per component,
 *              L = sqrt((dx dx + dy dy) + dz dz) in this order of operations, no contraction to a fused multiply-add.
 *   long       a triangle is long iff some L > max_edge; strictly: L == max_edge is not long, a nan is not long.
 *   done       the other triangles leave in this round: the vertices they reference in ascending index order, their indices
 *              remapped (the cut of dnsplat_mesh_cut_count / dnsplat_mesh_cut_emit), their ci rows with them; appended to the
 *              output, vertices below vertices, triangle indices raised by the number of vertices emitted before (vertex_base).  A
 *              vertex that done triangles of several rounds reference appears once per such round, as in trimesh.
 *   stop       no long triangle: the end.  Long triangles in round max_iter: the caller fails ("max_iter exceeded", as trimesh
 *              does) and returns nothing.
 *   midpoints  every distinct undirected edge {lo, hi} of the long triangles gets ONE midpoint (cv[lo] + cv[hi]) / 2.  An edge with
 *              equal ends is an edge like any other; its midpoint is the vertex's own position.  Midpoints are numbered in order of
 *              first appearance over the slots 3 t + e of the long triangles, t ascending, and stand below ALL current vertices:
 *              next cv = [cv; midpoints], Vc + n_mid rows.  (trimesh numbers by a row hash; as a triangle soup the result does not
 *              depend on the numbering.)
 *   children   a long triangle (a, b, c) with the midpoints m0, m1, m2 of its edges 0, 1, 2 becomes (a, m0, m2), (m0, b, m1),
 *              (m2, m1, c), (m0, m1, m2), in the order of their parents; each child's origin is its parent's.
 *
 * dnsplat_subdivide_count — an open-addressing table of the long triangles' edges (keys lo << 32 | hi, lo <= hi, claimed by a
 *   64-bit compare-and-swap, linear probing, the lowest slot 3 t + e of each edge by an integer minimum; 4 Tc entries, a load of at
 *   most 0.75), the marks of the done triangles' vertices, flag ranks per block of 256 and one workgroup of scans: counts device
 *   int64 [4] = {V_done, T_done, n_long, n_mid}.  Six launches.  Everything emit needs stays in scratch.
 * dnsplat_subdivide_emit — after count with the same arguments and the capacities the host took from counts: the done vertices
 *   double [cap_v,3], the done triangles int32 [cap_t,3] (+ vertex_base) and their origins int32 [cap_t]; with cap_long > 0 also
 *   next_vertices double [V + cap_mid,3] (the rows of cv, then the midpoints), next_triangles int32 [4 cap_long,3] and next_origin
 *   int32 [4 cap_long].  Nothing is written past a capacity.  Two launches, four with cap_long > 0; it may be repeated.
 * status: device int32 [1], zeroed by the CALLER before the first round; the calls OR bits into it and it stays 0 on a correct build
 *   with valid indices: DNSPLAT_SUBDIVIDE_STATUS_INTERNAL — a probe of the table ran through its whole capacity, or an edge was not
 *   found in it (cannot happen); DNSPLAT_SUBDIVIDE_STATUS_INDEX — a triangle has an index outside [0, V): it is neither done nor long
 *   and vanishes; DNSPLAT_SUBDIVIDE_STATUS_CAPACITY — a count exceeds the capacity emit was given.
 * Integers decide every order, there is no floating-point atomic: equal inputs give equal bytes, whatever the order the atomics land
 * in.  Nothing is read on the host, allocated or synchronised.
 * scratch: dnsplat_subdivide_scratch_bytes(V, T) = 64 T + 4 V + 4 (2 ceil(T / 256) + ceil(V / 256) + ceil(3 T / 256)) bytes, 8-byte
 *   aligned (the table 48 T, the midpoint of each slot 12 T, a kind byte per triangle and a first-appearance byte per slot 4 T, the marks
 *   4 V, the block counts); 0 for V < 1, T < 1 or T > (2^31 - 1) / 4, where the table leaves its int32 index.
 * Both return before anything touches a device: DNSPLAT_ERR_INVALID_ARG for a NULL args or required pointer (emit: a buffer whose
 *   capacity is positive), V < 1, T < 1, max_edge not in (0, inf) (a nan included), a negative capacity or vertex_base;
 *   DNSPLAT_ERR_UNSUPPORTED for T > (2^31 - 1) / 4, and in emit for 4 cap_long > (2^31 - 1) / 4 children (the next round's table),
 *   V + cap_mid > 2^31 - 1 or vertex_base + cap_v > 2^31 - 1; DNSPLAT_ERR_WORKSPACE for a short or misaligned scratch.
 * Out of scope: vertex attributes through the subdivision beyond the origin (face_index), Loop smoothing, welding the duplicated
 * vertices, mesh files. */
#define DNSPLAT_SUBDIVIDE_STATUS_INTERNAL 1
#define DNSPLAT_SUBDIVIDE_STATUS_INDEX 2
#define DNSPLAT_SUBDIVIDE_STATUS_CAPACITY 4
typedef struct dnsplat_subdivide_args {
    int32_t V, T;               /* the current round's Vc, Tc */
    const double *vertices;     /* cv [V,3] */
    const int32_t *triangles;   /* cf [T,3] */
    const int32_t *origin;      /* ci [T] */
    double max_edge;
    void *scratch;
    size_t scratch_bytes;
    int64_t *counts;            /* device int64 [4]: V_done, T_done, n_long, n_mid; written by count, read by emit */
    int32_t *status;            /* device int32 [1]; the caller zeroes it before the first round */
    int64_t vertex_base;        /* emit: the vertices earlier rounds emitted */
    int64_t cap_v, cap_t;       /* emit: rows of out_vertices / out_triangles and out_index */
    int64_t cap_long, cap_mid;  /* emit: long triangles and midpoints the next_* buffers hold */
    double *out_vertices;       /* emit: [cap_v,3] */
    int32_t *out_triangles;     /* emit: [cap_t,3] */
    int32_t *out_index;         /* emit: [cap_t] */
    double *next_vertices;      /* emit, cap_long > 0: [V + cap_mid,3] */
    int32_t *next_triangles;    /* emit, cap_long > 0: [4 cap_long,3] */
    int32_t *next_origin;       /* emit, cap_long > 0: [4 cap_long] */
} dnsplat_subdivide_args;
size_t dnsplat_subdivide_scratch_bytes(int32_t V, int32_t T);   /* 0 for an invalid size */
int dnsplat_subdivide_count(const dnsplat_subdivide_args *args, dnsplat_stream_t stream);
int dnsplat_subdivide_emit(const dnsplat_subdivide_args *args, dnsplat_stream_t stream);

/* ------------------------------------------------------------------ point-cloud normals (added after ABI 15, found by symbol)
 * Open3D's PointCloud.estimate_normals, which the reference calls in two places: the seed normals of its dataparsers
 * (_load_points3D_normals in normal_nerfstudio.py:85-101, replica_dataparser.py:381, nrgbd_dataparser.py:378,
 * scannetpp_dataparser.py:593, mushroom_dataparser.py:758, coolermap_dataparser.py:334, g_sdfstudio_dataparser.py:270:
 * KDTreeSearchParamHybrid(radius = 0.1, max_nn = 30), from which dn_model.py:196-215 initialises the Gaussians' normals), and the normals
 * of a sensor depth frame (scripts/depth_to_normal.py:150-213, scripts/depth_normal_consistency.py:171-221: KDTreeSearchParamKNN(200)
 * over every pixel).  Open3D is not at hand: the rule is restated from memory of PointCloud::EstimateNormals and
 * OrientNormalsTowardsCameraLocation, IT IS THIS PROJECT'S DEFINITION, PARITY UNPINNED AGAINST Open3D.  torch_normals.py restates it on
 * the CPU.  Everything is caller-allocated; nothing is read on the host, allocated or synchronised; no floating-point atomic, every
 * loop bounded by the sizes: equal inputs give equal bytes.
 *
 * For point i of points fp32 [N,3], with `index` = dnsplat_knn_build over the SAME points:
 *   neighbours K = min(knn, N).  The K points with the smallest key (d2, index) under dnsplat_knn_query's d2 — coordinates widened to
 *              double, d2 = fma(dz, dz, fma(dy, dy, dx dx)) — the point itself included; equal d2 go to the lowest index, so the set is
 *              canonical.  With a radius (Open3D's hybrid search) of those K the ones with d2 < radius radius are kept, the product in
 *              double: a strict test, as Open3D takes a lower bound on the sorted squared distances.  n = the number kept.  A row
 *              with a non-finite coordinate has n = 0 and is nobody's neighbour.
 *   moments    in double, over the kept neighbours in ascending (d2, index) rank t = 0 .. n - 1, by ONE FIXED TREE: the partial of
 *              lane l = t mod 64 adds its terms t = l, l + 64, l + 128, l + 192 in this order from 0; the 64 partials are then
 *              added pairwise, v[l] = v[l] + v[l xor o] for o = 32, 16, 8, 4, 2, 1.  The mean m = (sum of p_j) / n; then the six sums
 *              of (p_j - m)(p_j - m)^T in the order xx, xy, xz, yy, yz, zz by the same tree, C = sum / n.  Two passes about the mean,
 *              NOT Open3D's cumulants: a deliberate deviation, better conditioned at no cost here.  No contraction to a fused
 *              multiply-add.  n = 0: C = 0.
 *   normal     the unit eigenvector of the smallest eigenvalue of C: 8 cyclic Jacobi sweeps in double over the planes (0,1), (0,2),
 *              (1,2), the rotation of dnsplat_icp's solve (theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| +
 *              sqrt(theta theta + 1)), c = 1 / sqrt(t t + 1), s = t c); an a_pq that is zero, or that changes neither |a_pp| nor |a_qq|
 *              when its magnitude is added to them, is set to zero without a rotation.  The column of the smallest diagonal entry,
 *              equal ones to the lowest column, divided once by sqrt((e0 e0 + e1 e1) + e2 e2).  n < 3, or a C whose six entries are
 *              all zero: (0, 0, 1), Open3D's fallback.
 *   sign       without orient: canonical — the component of largest magnitude is positive, the lowest axis on equal magnitudes
 *              (Open3D leaves the sign arbitrary).  With orient (orient_normals_towards_camera_location(toward)): the normal is
 *              negated iff (n0 (c0 - p0) + n1 (c1 - p1)) + n2 (c2 - p2) < 0 in double, p the point widened; a product of exactly 0
 *              does not flip.  The fallback is oriented like any other normal.
 * dnsplat_cloud_normals — ONE launch, one wave of 64 lanes per point: the cube rings of dnsplat_knn_query's search read row by row
 *   as coalesced runs of the index, the candidates below the threshold appended to a buffer of 2 KP entries in the wave's LDS (KP = knn
 *   rounded up to a power of two, at least 64), a bitonic sort of that buffer keeping the K lowest whenever a batch of 64 would not fit
 *   and at the end of each ring that left K or more; the search ends as dnsplat_knn_query's does (the K-th d2 below the bound of what
 *   lies outside the cube, with the same 1 -+ 4e-7 factors), or when that bound is not below radius radius.  Outputs: normals double
 *   [N,3]; optional (NULL to skip, the normals are the same bytes either way) covariance double [N,6], neighbors int32 [N,knn]
 *   ascending by (d2, index) with -1 past n, count int32 [N] = n.
 * status: device int32 [1], zeroed by the CALLER; it stays 0 on a correct build: DNSPLAT_NORMALS_STATUS_INTERNAL — the rings ran out
 *   before the cube covered the grid (cannot happen).
 * scratch: dnsplat_cloud_normals_scratch_bytes(N, knn) = 16 bytes, 8-byte aligned, zeroed by the CALLER: int32 [4] = {the widest ring a
 *   query reached, the most selections one query ran, 0, 0}, two integer maxima for tests and timing; 0 for N < 1 or knn outside
 *   [3, DNSPLAT_NORMALS_MAX_K].
 * Returns before anything touches a device: DNSPLAT_ERR_INVALID_ARG for a NULL args or required pointer, N < 1, a nan radius (radius <= 0
 *   or +inf: no radius), orient outside {0, 1}, a nan in toward with orient; DNSPLAT_ERR_UNSUPPORTED for knn outside
 *   [3, DNSPLAT_NORMALS_MAX_K]; DNSPLAT_ERR_WORKSPACE for a short or misaligned scratch.
 * Known limit: a far, isolated point widens its cube ring by ring until the K-th neighbour is certain (or, with a radius, only until the
 *   bound passes it).  Infinite coordinates are not supported by the index (its box loses its extent); nan rows are.
 * Out of scope: a pure radius search with unbounded count, orient_normals_consistent_tangent_plane, covariance-weighted or
 * fast-approximate normals, Poisson reconstruction, PLY input and output, a k-NN index for thin shells, widening dnsplat_knn_query
 * beyond DNSPLAT_KNN_MAX_K. */
#define DNSPLAT_NORMALS_MAX_K 256
#define DNSPLAT_NORMALS_STATUS_INTERNAL 1
typedef struct dnsplat_cloud_normals_args {
    int32_t N;
    int32_t knn;                /* Open3D's knn / max_nn: 3 .. DNSPLAT_NORMALS_MAX_K */
    const float *points;        /* [N,3] */
    const void *index;          /* dnsplat_knn_build's, over the same points */
    double radius;              /* the hybrid search's radius; <= 0 or +inf: none */
    int32_t orient;             /* 1: towards `toward`; 0: the canonical sign */
    double toward[3];
    void *scratch;
    size_t scratch_bytes;
    double *normals;            /* [N,3] */
    double *covariance;         /* [N,6] xx, xy, xz, yy, yz, zz, or NULL */
    int32_t *neighbors;         /* [N,knn], or NULL */
    int32_t *count;             /* [N], or NULL */
    int32_t *status;            /* device int32 [1]; the caller zeroes it */
} dnsplat_cloud_normals_args;
size_t dnsplat_cloud_normals_scratch_bytes(int32_t N, int32_t knn);   /* 0 for an invalid size */
int dnsplat_cloud_normals(const dnsplat_cloud_normals_args *args, dnsplat_stream_t stream);

/* The per-Gaussian term of the same loss (regularization_strategy.py:195-199): mean_g min_k exp(scales[g][k]).  Adds
 * weight * sum_g min_k exp(s_gk) to *sum (device scalar, caller zeroes it) and WRITES the gradient rows
 * v_scales[g][k] = [k == argmin_k] * weight * exp(s_gk); weight = 1 / N gives the mean.  Replaces torch's exp / min / mean and their
 * five backward kernels over [N,3] tensors. */
int dnsplat_scale_reg(int32_t N, const float *scales_log, float weight, float *v_scales /* [N,3] */, float *sum, dnsplat_stream_t stream);

/* ------------------------------------------------------------------ stage 5
 * Fused per-Gaussian back end: gradient record -> parameter gradients.
 * Replaces gsplat fully_fused_projection_bwd (A10), spherical_harmonics bwd (A5),
 * the autograd of dn_model.py:543-560 (A7) and of the activations (A0). */
typedef struct dnsplat_proj_grads {
    const int32_t *radii;        /* [N] from the forward */
    const float *v_splats;       /* [N,16] gradient records */
    const float *v_means2d;      /* optional [N,2]: if non-NULL REPLACES record columns 0-1 (the binding
                                    routes means2d through autograd so callers may add their own terms) */
    const float *v_depths;       /* optional [N], added */
    const float *v_conics;       /* optional [N,3], added */
    const float *v_compensations;/* optional [N] */
    float *v_means;              /* [N,3] */
    float *v_quats;              /* [N,4] */
    float *v_scales;             /* [N,3] w.r.t. the tensor passed in (log-scales if scales_are_log) */
    float *v_opacities;          /* [N]   w.r.t. the tensor passed in */
    float *v_sh0; int32_t v_sh0_stride;   /* like scene.sh0 / shN; NULL to skip */
    float *v_shN; int32_t v_shN_stride;
    float *v_colors;             /* [N,n_colors] when sh_degree < 0; NULL to skip */
    int32_t sh_grads_skip;       /* non-zero: the SH coefficient gradients are not written — the caller took the colour gradients
                                    with dnsplat_sh_factors before this launch and rebuilds the rows from the gathered slabs
                                    (dnsplat_sh_grads_from_factors) */
    float *sh_factors;           /* optional [3 N + 4] (ABI 12; SH scenes only): this launch ALSO writes the slab dnsplat_sh_factors
                                    produces — per Gaussian the three colour gradients behind the clamp (zeros when culled), then the
                                    camera centre and a pad word — from the values it holds anyway, which saves that kernel's launch
                                    and its 128 B / Gaussian of reads.  For callers whose exchange starts after this launch (a
                                    captured step: graph.GraphedDpStep); dnsplat_sh_factors stays for those that start it before */
    float sh_grad_scale;         /* ABI 14.  0 or 1: as before.  Otherwise the SH coefficient gradient rows this launch writes (v_sh0 / v_shN)
                                    are multiplied by it — 1 / world size when the rank writes its OWN camera's rows itself and
                                    dnsplat_sh_grads_add_factors adds the other cameras' (the mean over cameras; geometry gradients are not
                                    scaled: their all-reduce averages) */
    uint64_t *sh_zero_state;     /* ABI 14.  NULL, or device [ceil(N / 64)] words owned by whoever owns the v_sh0 / v_shN buffers (split or
                                    [N,16,3] layout, K = 16): bit g % 64 of word g / 64 set = "the coefficient-gradient row of Gaussian g
                                    is zero in memory".  The launch skips the stores of rows that are culled now AND known zero, and
                                    leaves the word describing what memory holds afterwards (culled rows: zero).  Contract: nobody else
                                    writes non-zero values into those rows without clearing the words (dp.GradArena.invalidate_sh_state).
                                    Ignored with sh_grads_skip. */
    float *sh_packed;            /* ABI 14.  NULL, or this camera's PACKED slab, whose header / masks / offsets dnsplat_visible_index wrote for
                                    the same radii (see there): the launch fills its rows — the colour gradients of the VISIBLE Gaussians
                                    only, row offsets[g / 64] + popcount(mask bits below g % 64) — beside or instead of sh_factors.  Whole
                                    scenes only (the slices of dp.SlicedShExchange keep dense slabs). */
    int32_t zero_state_geometry; /* ABI 15.  1: the words of sh_zero_state describe ALL gradient rows of a Gaussian that this launch writes —
                                    v_means / v_quats / v_scales / v_opacities beside the coefficient rows (their owner keeps the same
                                    contract for them).  Rows are then skipped per WORKGROUP of 64 Gaussians, all or nothing: a workgroup
                                    whose rows are all culled now and all known zero writes nothing at all (236 B per Gaussian); any other
                                    workgroup stores its whole span as without the state.  Pays when the rows follow a space-filling
                                    curve (densify.spatial_order: a camera's culled Gaussians are then runs of rows). */
} dnsplat_proj_grads;

int dnsplat_project_bwd(const dnsplat_scene *scene, const dnsplat_camera *cam,
                        const dnsplat_proj_out *fwd, const dnsplat_proj_grads *grads,
                        dnsplat_stream_t stream);

/* Camera pose gradient (added after ABI 15, found by symbol).  dnsplat_project_bwd_pose does everything dnsplat_project_bwd does —
 * same dnsplat_proj_grads semantics, the parameter gradients come out bit-equal — and ALSO reduces the gradient of the loss with
 * respect to camera.viewmat, which gsplat's rasterization() returns as viewmats.grad and a camera optimiser trains the pose with
 * (dn_model.py:114-116, 475).  Every workgroup of 64 Gaussians sums its share in registers (no atomics) into one row of
 * `partials`; two small launches add the rows in a fixed order in fp64.  The result is bit-reproducible for equal inputs, with
 * or without dnsplat_raster_args.det_partials.  Three launches, no allocation, no synchronisation. */
typedef struct dnsplat_pose_grads {
    float *partials;       /* workspace: dnsplat_pose_partial_rows(N) rows of 16 floats, 16-byte aligned; contents need not survive */
    float *v_viewmat;      /* out, device [16] row-major 4x4.  Rows 0-2: rotation block and translation column.  Row 3: the camera
                              centre enters the SH view direction as inverse(viewmat)[:3,3] (gsplat), whose derivative reaches the
                              bottom row too: -(c . G) [c_x, c_y, c_z, 1], c the centre, G its gradient; zero without SH colours */
    const float *c2w;      /* optional device [12]: the nerfstudio camera-to-world rows dnsplat_camera_prepare made viewmat from */
    float *v_c2w;          /* optional device [12] (both or neither): v_viewmat chained through dnsplat_camera_prepare's viewmat
                              (column flip, transpose, -R^T T); the normal frame and K carry no gradient */
} dnsplat_pose_grads;

size_t dnsplat_pose_partial_rows(int32_t N);   /* >= ceil(N / 64), monotone in N */
int dnsplat_project_bwd_pose(const dnsplat_scene *scene, const dnsplat_camera *cam, const dnsplat_proj_out *fwd,
                             const dnsplat_proj_grads *grads, const dnsplat_pose_grads *pose, dnsplat_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DNSPLAT_H */
