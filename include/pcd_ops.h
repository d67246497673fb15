/*
 * pcd_ops.h -- C ABI of libpcdops_hip.so: the MI355X (gfx950) implementation of the sparse-voxel
 * hot path the reference (ZZY816/COM, an OpenPCDet fork) inherits from `spconv` + a few torch modules.
 *
 * Conventions (the reference's own binder convention is
 * pcdet/ops/pointnet2/pointnet2_stack/src/ball_query.cpp:29-45: caller-allocated outputs, int return,
 * raw pointers, contiguous int32 / float32 tensors):
 *   - every function returns 0 on success or a negative PCD_ERR_* code (never exit()s);
 *   - every pointer is a DEVICE pointer unless the name ends in _host; host arrays are read
 *     before the function returns;
 *   - the caller owns every buffer (outputs, workspaces); the library never allocates or frees
 *     device memory and keeps no pointer after returning; all work is enqueued on `stream`
 *     (a hipStream_t, may be NULL for the default stream) and NOT synchronised;
 *   - functions keep no state between calls and may be called from several host threads; the ONLY process-wide state is the
 *     tuning-option table (pcd_set_option: set before the first launch, read unsynchronised at launch time);
 *   - index tensors are int32, coordinates are (batch, z, y, x) rows of 4 int32.
 *
 * Device-side row counts: wherever a function takes a row count `n` together with a `const int32_t *n_dev`
 * argument, `n` is the CAPACITY (buffer strides, grid size) and, when n_dev != NULL, the kernels process
 * min(*n_dev, n) rows.  A caller can therefore chain the whole path (voxelise -> rulebooks -> convs -> BEV)
 * without ever reading a data-dependent size back to the host, i.e. inside one captured hipGraph.
 *
 * Feature element types: PCD_BF16 (MFMA path, fp32 accumulate) for sparse-conv features,
 * PCD_F32 for point / voxel payloads.  A feature row has `c_pad` elements, c_pad % 8 == 0,
 * padding channels must be zero.
 */
#ifndef PCD_OPS_H_
#define PCD_OPS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCD_OK 0
#define PCD_ERR_INVALID_ARG (-1)  /* NULL pointer, negative size, bad enum                       */
#define PCD_ERR_UNSUPPORTED (-2)  /* shape / dtype combination this build has no kernel for      */
#define PCD_ERR_KEYSPACE (-3)     /* batch * D * H * W does not fit the 32-bit coordinate key    */
#define PCD_ERR_WORKSPACE (-4)    /* workspace too small                                         */
#define PCD_ERR_LAUNCH (-5)       /* hipGetLastError() != hipSuccess after a launch              */

#define PCD_F32 0
#define PCD_BF16 1

/* Row order of a sparse level whose rows are numbered by a linear coordinate key (the key-ordered voxeliser, the strided
 * rulebook builds and the rank-map SubM builds take it as `row_order`).  Every consumer of the path is invariant to the
 * order (spconv itself numbers GPU-built levels by hash / atomics order); the VOXEL SETS and, through the row permutation,
 * the rulebooks are identical in both.
 *   PCD_ROWS_ZYX  key = ((b*D + z)*H + y)*W + x   x fastest -- spconv's / torch.unique's sorted order
 *   PCD_ROWS_YXZ  key = ((b*H + y)*W + x)*D + z   z fastest: the voxels of a BEV column are consecutive rows and the 27
 *                 neighbours of a run of rows lie in three short runs of rows (BEV rows y-1, y, y+1) -- what the window
 *                 gather-GEMM (pcd_sparse_conv_subm_window) stages in LDS */
#define PCD_ROWS_ZYX 0
#define PCD_ROWS_YXZ 1

/* ---- library info -------------------------------------------------------------------------- */
int pcd_version(void);                    /* 10000*major + 100*minor + patch; 0.2.0: the two entry points of the
                                             plane-form dense weight gradient left the ABI; 0.3.0: the entry points whose
                                             successors take a superset of their arguments left it; 0.4.0: the
                                             pcd_voxel2pinds_* / pcd_voxel_pool_* entry points joined; 0.5.0: the
                                             pcd_vector_pool_* entry points joined; 0.6.0: pcd_point_head_assign_targets
                                             left it (pcd_point_head_assign_targets_full does its work).  A
                                             missing lower version number (pcd_adam_flat_step_v4 without _v3,
                                             pcd_sparse_conv_wgrad_v2 without the unsuffixed form, _ld / _bn / _dir / _full
                                             without the plain form) means "retired": the survivors keep their names */
const char *pcd_error_string(int code);
const char *pcd_build_arch(void);         /* "gfx950" */
/* text of the HIP runtime error behind the calling thread's last PCD_ERR_LAUNCH */
const char *pcd_last_hip_error_string(void);
void pcd_set_last_hip_error(int code);    /* internal use */
/* *id_out = 0 when `stream` is not being captured into a hipGraph, else the id of that capture (host-side keying of
 * per-graph resources; no reference counterpart: the reference has no graph capture) */
int pcd_stream_capture_id(void *stream, unsigned long long *id_out);

/* ---- tuning options --------------------------------------------------------------------------
 * Integer knobs of the kernel dispatch (tile shapes, kernel variants).  They select between
 * implementations that produce the same results; the defaults are the measured optima and nothing in the product sets them.
 * Explicit and inspectable (no environment reads anywhere in the library): pcd_set_option returns PCD_ERR_INVALID_ARG for an
 * unknown key.  Process-wide, not synchronised: set them before the first call that uses them.  (No reference counterpart.)
 *   "gg_resident_kb" 32   packed weight up to this size stays resident in LDS in gather_gemm_kernel
 *   "ggw" 1               LDS-DMA gather-GEMM (ggw_kernel) for C_in = 128, C_out = 64 / 128 (0: gather_gemm_kernel, the only
 *                         kernel for those widths over a packed table or with kvol > 52)
 *   "subm_window" 23      window gather-GEMM for SubM 3x3x3 layers over PCD_ROWS_YXZ rows: bit 0 = 64 channels, bit 1 = 32,
 *                         bit 2 = 16, bit 3 = 128 (retired: its dense 27-offset MFMA work made it slower than the
 *                         step-skipping generic kernel there, 61.6 vs 49.0 us; ignored), bit 4 = layers with FEWER input than output
 *                         channels run on zero-padded rows (conv_input 5 -> 16; forward + weight gradient, no data gradient)
 *                         (0: generic kernels) -- read by the host-side layer, the C entry points take any of these widths
 *   "subm_window_wgrad" 6 the same bits for the window weight gradient (pcd_sparse_conv_subm_window_wgrad); 64 channels off:
 *                         its 80 partial slabs (35 MB per layer) cost the training step more than the kernel saves
 *   "wg128" 1             equal-pair weight-gradient kernel at 128 x 128 channels (0: the generic kernel, the only one there
 *                         for padded x rows (cin_pad != 128), kvol > 343 and pcd_sparse_conv_wgrad_classes)
 *   "wg128_chunks" 512    its workgroup count
 *   "wg_rows" 6144        row-range split of the generic weight-gradient kernel
 *   "conv2d_wg_blocks" 128 workgroups of the dense 3x3 weight-gradient kernel
 *   "fps_g" 0             workgroups per frame of the cooperative farthest point sampling (0: from the device's CU count)
 *   "subm_window_half" 0  4-wave window configurations (256 threads, <= 80 KB of LDS: two workgroups per CU): bit 1 = 32 channels,
 *                         bit 2 = 16 channels.  Set it before the first plan is built: plans, packs and launches of a width must agree
 *   "subm_window_grid" 256   workgroups of a window launch (a multiple of 8, <= 256); fewer leave CUs to other streams --
 *                         measured: no gain (240 / 224 / 192: 0 / -0.5 / -1 % in the step)
 *   "vox_grid" 0          workgroup cap of the voxeliser's point passes (hash insert; column-map marks) (0: one per 256 points)
 *   "cm_direct_blocks" 4096   column-map builds: up to this many scan blocks add up the block sums themselves, beyond it a
 *                             spine launch runs (tests lower it to reach the spine path on small inputs) */
int pcd_set_option(const char *key, int value);
int pcd_get_option(const char *key, int *value_out);

/* ============================================================================================
 * (a1) hard voxelisation -- replaces spconv.utils.VoxelGeneratorV2.generate /
 *      Point2VoxelCPU3d.point_to_voxel as called from
 *      pcdet/datasets/processor/data_processor.py:44-60 (+ the batch collation of
 *      pcdet/datasets/dataset.py:252-259), and optionally fuses MeanVFE
 *      (pcdet/models/backbones_3d/vfe/mean_vfe.py:25-29).
 *
 * points: rows of `point_stride` floats; the C features copied into voxels start at column
 * `feat_offset` and begin with x, y, z (feat_offset = 1 for collated (b,x,y,z,..) rows).
 * Frame b owns point rows [frame_offsets[b], frame_offsets[b+1]).
 * Semantics per frame = reference: point order, coordinate floor((p-min)/vsize) in IEEE f32,
 * voxel ids in first-appearance order, at most max_voxels voxels, first max_points points kept.
 * Output rows are compacted over frames: frame b starts at sum_{b'<b} M_b'.
 *   voxels      [cap][max_points][C] f32, zero padded (may be NULL)
 *   coords      [cap][4] i32 (b, z, y, x)
 *   num_points  [cap] i32
 *   mean_f32    [cap][C] f32 = sum / max(num,1)  (may be NULL)
 *   mean_bf16   [cap][mean_bf16_stride] bf16, zero padded channels (may be NULL)
 *   voxel_counts[batch+1] i32: M_b per frame, last = total rows written
 * cap = capacity in rows of the outputs (>= min(n_points, batch*max_voxels) is always enough).
 * ============================================================================================ */
size_t pcd_voxelize_hard_workspace_bytes(int n_points, int max_points, int batch);
int pcd_voxelize_hard(const float *points, int n_points, int point_stride, int feat_offset,
                      int num_features, const int32_t *frame_offsets, int batch,
                      const float *range_host /*[6]*/, const float *vsize_host /*[3]*/,
                      int max_points, int max_voxels, int cap, float *voxels, int32_t *coords,
                      int32_t *num_points, float *mean_f32, void *mean_bf16, int mean_bf16_stride,
                      int32_t *voxel_counts, void *workspace, size_t workspace_bytes, void *stream);

/* Same operation, same kept set (the first max_voxels voxels per frame in first-appearance order, their first
 * max_points points in point order -- data_processor.py:44-60), rows numbered by ascending (b, z, y, x) key instead of
 * by first appearance: the order torch.unique (dynamic_mean_vfe.py:57-66) and spconv's strided convs give their rows.
 * Every consumer of the hot path (mean_vfe.py:25-29 -> spconv_backbone.py:239-246) is invariant to the row order;
 * with training's shuffled points (data_processor.py:103-113) the first-appearance order is random in space, the key
 * order keeps the 27 neighbours of a level-1 row in nearby rows.  Needs batch*gz*gy*gx < 2^32 - 1024 (PCD_ERR_KEYSPACE
 * otherwise); the workspace holds an occupancy bitmap of that many bits.
 *   rank_bitmap / rank_prefix (both or neither): caller-owned buffers of pcd_voxelize_hard_sorted_rank_words() words
 *   that receive the coordinate -> row map of the output -- bit (key) of rank_bitmap set for every kept voxel,
 *   rank_prefix[g] = number of set bits in front of the 128-bit group g -- the map pcd_rulebook_subm_ranked4 builds the
 *   level-1 SubM rulebook from (no hash table).  NULL: the map lives in the workspace and dies with the call.
 *   key_depth: z extent D of the key space (PCD_ROWS_* above with H = gy, W = gx); 0 = gz.  The 3D backbones use
 *   sparse_shape = grid_size[::-1] + [1, 0, 0] (spconv_backbone.py:87,187): pass gz + 1 so that the map has the layout
 *   the rulebook of that shape addresses.  The row ORDER does not depend on it.
 *   row_order: PCD_ROWS_ZYX / PCD_ROWS_YXZ. */
size_t pcd_voxelize_hard_sorted_workspace_bytes(int n_points, int max_points, int batch,
                                                const float *range_host /*[6]*/, const float *vsize_host /*[3]*/,
                                                int key_depth);
int pcd_voxelize_hard_sorted_rank_words(int batch, const float *range_host /*[6]*/, const float *vsize_host /*[3]*/,
                                        int key_depth, size_t *bitmap_words, size_t *prefix_words);
int pcd_voxelize_hard_sorted(const float *points, int n_points, int point_stride, int feat_offset,
                             int num_features, const int32_t *frame_offsets, int batch,
                             const float *range_host /*[6]*/, const float *vsize_host /*[3]*/,
                             int max_points, int max_voxels, int cap, float *voxels, int32_t *coords,
                             int32_t *num_points, float *mean_f32, void *mean_bf16, int mean_bf16_stride,
                             int32_t *voxel_counts, int key_depth, int row_order, uint32_t *rank_bitmap,
                             int32_t *rank_prefix, void *workspace, size_t workspace_bytes, void *stream);
/* pcd_voxelize_hard_sorted with row_order PCD_ROWS_YXZ whose coordinate -> row map is the level's COLUMN MAP ("Column maps"
 * below): `colmap` is a caller-owned buffer of pcd_colmap_bytes(batch, (max(gz, key_depth), gy, gx), cap) bytes that the
 * rulebook builds of level 1 read (pcd_rulebook_subm_cm, pcd_rulebook_conv_cm_*; pass the same `cap`).  Same voxels, same
 * rows as pcd_voxelize_hard_sorted(PCD_ROWS_YXZ); the ranks come from two order-free marks (BEV occupancy bit, z bit of the
 * column's mask) and two small scans instead of a bitmap over the (b, y, x, z) key space (46 MB zero-filled, scanned and
 * probed per 4-frame Waymo batch) -- and no separate pcd_colmap_from_rows pass.  key depth <= 62, batch <= 256
 * (PCD_ERR_UNSUPPORTED / 0 bytes otherwise: use pcd_voxelize_hard_sorted + pcd_colmap_from_rows).
 * Replaces the same call site (pcdet/datasets/processor/data_processor.py:44-60,125-153). */
/* Host-side variant for ONE frame: what the reference calls inside forked DataLoader worker processes
 * (pcdet/datasets/processor/data_processor.py:44-60,130-141), where a HIP call is impossible.  HOST pointers, no stream, no GPU
 * work: the sequential algorithm of SURVEY.md A.1 with the kernels' own coordinate arithmetic -- first-appearance voxel ids,
 * the first max_points points of every voxel, the max_voxels cut.  voxels [max_voxels][max_points][num_features] (rows used
 * are zero padded), coords [max_voxels][3] (z, y, x), num_points [max_voxels]; *num_voxels_out = M.  Same results as
 * pcd_voxelize_hard on one frame, bit for bit. */
int pcd_voxelize_hard_host(const float *points_host, int n_points, int point_stride, int num_features,
                           const float *range_host, const float *vsize_host, int max_points, int max_voxels,
                           float *voxels_host, int32_t *coords_host, int32_t *num_points_host, int32_t *num_voxels_out);
size_t pcd_voxelize_hard_yxz_workspace_bytes(int n_points, int max_points, int batch, const float *range_host,
                                             const float *vsize_host, int key_depth, int cap);
int pcd_voxelize_hard_yxz(const float *points, int n_points, int point_stride, int feat_offset, int num_features,
                          const int32_t *frame_offsets, int batch, const float *range_host, const float *vsize_host,
                          int max_points, int max_voxels, int cap, float *voxels, int32_t *coords, int32_t *num_points,
                          float *mean_f32, void *mean_bf16, int mean_bf16_stride, int32_t *voxel_counts, int key_depth,
                          void *colmap, size_t colmap_bytes, void *workspace, size_t workspace_bytes, void *stream);
/* (a4) MeanVFE on materialised voxels: mean_vfe.py:25-29.  out [m][C] f32. */
int pcd_mean_vfe(const float *voxels, const int32_t *num_points, int m, int max_points,
                 int num_features, float *out, void *stream);

/* ============================================================================================
 * (a5) dynamic voxelisation + mean -- replaces torch.unique + torch_scatter.scatter_mean in
 *      pcdet/models/backbones_3d/vfe/dynamic_mean_vfe.py:53-72.
 * points_b rows = (batch_idx, x, y, z, f3, ...) with 1 + C floats.  Output sorted by the
 * reference key b*XYZ + cx*YZ + cy*Z + cz; coords (b, z, y, x); no caps.
 *   features [cap][C] f32, coords [cap][4], counts [cap] (may be NULL), num_voxels [1] i32.
 * ============================================================================================ */
size_t pcd_voxelize_dynamic_workspace_bytes(int n_points, int num_features, int batch,
                                            const float *range_host, const float *vsize_host);
int pcd_voxelize_dynamic_mean(const float *points_b, int n_points, int num_features, int batch,
                              const float *range_host, const float *vsize_host, int cap,
                              float *features, int32_t *coords, int32_t *counts,
                              int32_t *num_voxels, int32_t *point_voxel, void *workspace,
                              size_t workspace_bytes, void *stream);
/* point_voxel (may be NULL) [n_points] i32: output row of every point (-1: dropped) = `unq_inv` of the
 * torch.unique(..., return_inverse=True) call of the dynamic VFEs (dynamic_mean_vfe.py:63,
 * dynamic_pillar_vfe.py:103).
 *
 * (a6) dynamic pillar encoder -- replaces torch_scatter.scatter_max in PFNLayerV2 (dynamic_pillar_vfe.py:36-47).
 *   pcd_segment_max:  out[s][ch] = max over the points i with seg[i] == s of x[i][ch]  (f32; seg < 0 skipped),
 *   arg[s][ch] = the smallest such i attaining it (deterministic; torch_scatter leaves ties unspecified).
 *   pcd_segment_max_backward:  grad_x [n][c] = 0 except grad_x[arg[s][ch]][ch] = grad_out[s][ch]. */
size_t pcd_segment_max_workspace_bytes(int m, int c);
int pcd_segment_max(const float *x, const int32_t *seg, int n, int c, int m, float *out, int32_t *arg,
                    void *workspace, size_t workspace_bytes, void *stream);
int pcd_segment_max_backward(const float *grad_out, const int32_t *arg, int n, int c, int m, float *grad_x,
                             void *stream);

/* ============================================================================================
 * (a8) SubMConv3d rulebook -- replaces spconv's get_indice_pairs(subm=True) behind
 *      spconv.SubMConv3d (pcdet/models/backbones_3d/spconv_backbone.py:12,38-45).
 * indices [n][4].  K = kd*kh*kw, offsets enumerated k = (kd*KH+kh)*KW+kw,
 * in_pos = out_pos - (ksize/2)*dil + k_idx*dil.
 *   nbr      [K][n] i32: nbr[k][o] = input row feeding output row o through offset k, or -1.
 *            (SubM symmetry: the input-stationary view is nbr_in[k] = nbr[K-1-k].)
 *   pairs    [K][2][n] i32 (may be NULL): spconv's indice_pairs, canonical order = ascending input
 *            row within each k, -1 padded.
 *   pair_num [K] i32 (required iff pairs != NULL)
 *   pad_pairs != 0: entries of pairs beyond pair_num[k] are set to -1 (spconv's padding; costs a memset
 *            of the whole table -- the compute kernels never read them)
 * ============================================================================================ */
size_t pcd_rulebook_subm_workspace_bytes(int n, int kvol);
int pcd_rulebook_subm(const int32_t *indices, int n, int batch, const int *shape_host /*[3]*/,
                      const int *ksize_host, const int *dil_host, int32_t *nbr, int32_t *pairs,
                      int32_t *pair_num, int pad_pairs, const int32_t *n_dev, void *workspace,
                      size_t workspace_bytes, void *stream);

/* ============================================================================================
 * (a9) SparseConv3d (strided) rulebook -- replaces get_indice_pairs(subm=False) behind
 *      spconv.SparseConv3d (spconv_backbone.py:14-15,205-229).  Two phases because the number of
 *      output rows is data dependent:
 *   phase 1 `_count`: marks the active output cells, ranks them (sorted by the linear key of
 *           `row_order`, PCD_ROWS_*) and writes n_out to n_out_dev[0]; state lives in `workspace`.
 *   phase 2 `_fill` : (after the caller read n_out and allocated) emits
 *           out_indices [n_out][4], nbr_in [K][n] (output row fed by input i, or -1),
 *           nbr_out [K][n_out] (input row feeding output o, or -1),
 *           pairs [K][2][n] + pair_num [K] (may be NULL/NULL).
 *   The same `workspace` (untouched in between) must be passed to both phases.
 * out_shape_host [3] receives floor((in + 2p - d(k-1) - 1)/s) + 1.
 * ============================================================================================ */
size_t pcd_rulebook_conv_workspace_bytes(int n, int batch, const int *in_shape_host,
                                         const int *ksize_host, const int *stride_host,
                                         const int *pad_host, const int *dil_host);
int pcd_conv_out_shape(const int *in_shape_host, const int *ksize_host, const int *stride_host,
                       const int *pad_host, const int *dil_host, int *out_shape_host);
int pcd_rulebook_conv_count(const int32_t *indices, int n, int batch, const int *in_shape_host,
                            const int *ksize_host, const int *stride_host, const int *pad_host,
                            const int *dil_host, int32_t *n_out_dev, const int32_t *n_dev, void *workspace,
                            size_t workspace_bytes, void *stream, int row_order);
int pcd_rulebook_conv_fill(const int32_t *indices, int n, int batch, const int *in_shape_host,
                           const int *ksize_host, const int *stride_host, const int *pad_host,
                           const int *dil_host, int n_out, int32_t *out_indices, int32_t *nbr_in,
                           int32_t *nbr_out, int32_t *pairs, int32_t *pair_num, int pad_pairs,
                           const int32_t *n_dev, void *workspace, size_t workspace_bytes, void *stream,
                           int row_order);

/* Both phases (+ the parity classes of pcd_rulebook_conv_classes when perm != NULL) in ONE call for callers that
 * bound the number of output rows on the host (`n_out_cap`: buffers are sized for it, rows beyond it are dropped and
 * n_out_dev[0] still receives the real count -- static plans / hipGraph capture, nothing is read back).  Same
 * results as _count + _fill + _classes; six dependent launches (five without pair lists) instead of fifteen:
 * fill, mark (+ class counts), pack + block sums, scan + emit + 0xFF fills + class offsets, neighbour tables
 * (+ class permutation), pair lists.  Workspace: pcd_rulebook_conv_workspace_bytes.
 * Replaces the same get_indice_pairs(subm=False) call (spconv_backbone.py:14-15,205-229). */
int pcd_rulebook_conv_build(const int32_t *indices, int n, int batch, const int *in_shape_host,
                            const int *ksize_host, const int *stride_host, const int *pad_host,
                            const int *dil_host, int n_out_cap, int32_t *n_out_dev, int32_t *out_indices,
                            int32_t *nbr_in, int32_t *nbr_out, int32_t *pairs, int32_t *pair_num, int pad_pairs,
                            int cls_tile, int32_t *perm, int vcap, int32_t *vstart_dev, const int32_t *n_dev,
                            void *workspace, size_t workspace_bytes, void *stream, int row_order);

/* indice_pairs / indice_pair_num of a SubM rulebook from its nbr table [kvol][n] alone -- for rulebooks built with
 * pairs == NULL (the forward and the output-stationary kernels only need nbr) whose pairs are wanted later. */
size_t pcd_rulebook_subm_pairs_workspace_bytes(int n, int kvol);
int pcd_rulebook_subm_pairs(const int32_t *nbr, int n, int kvol, int32_t *pairs, int32_t *pair_num, int pad_pairs,
                            const int32_t *n_dev, void *workspace, size_t workspace_bytes, void *stream);
/* ... and of a STRIDED rulebook from its nbr_in table [kvol][n] (same workspace size): the training step builds strided
 * rulebooks without pair lists (pcd_sparse_conv_wgrad_classes reads the pairs off the parity classes); whoever still wants
 * spconv's indice_pairs (spconv/pytorch/ops.py get_indice_pairs' outputs) derives them here, same values as the build's. */
int pcd_rulebook_conv_pairs(const int32_t *nbr_in, int n, int kvol, int32_t *pairs, int32_t *pair_num, int pad_pairs,
                            const int32_t *n_dev, void *workspace, size_t workspace_bytes, void *stream);
/* The rank structure the strided build leaves in its workspace is exactly a coordinate -> row map of the OUTPUT
 * level (row id = rank of the linear key): the SubM rulebook of that level (the 'subm2..4' keys that follow
 * every strided conv of spconv_backbone.py:205-229) can use it instead of building and probing a hash table.
 *   pcd_rulebook_conv_rank_layout: byte offsets of the occupancy bitmap (u32 [nwords]) and of its exclusive
 *       popcount prefix (i32 [nwords]) inside a workspace of pcd_rulebook_conv_workspace_bytes(same arguments);
 *       valid after pcd_rulebook_conv_count, for as long as the caller keeps that workspace untouched.
 *   pcd_rulebook_subm_ranked: same outputs (bit for bit) as pcd_rulebook_subm for indices == the out_indices of
 *       that strided build, shape_host == its output shape; 3x3x3 kernels only (PCD_ERR_UNSUPPORTED otherwise).
 *       Ranks >= n (rows dropped by a static capacity) count as missing neighbours. */
int pcd_rulebook_conv_rank_layout(int n, int batch, const int *in_shape_host, const int *ksize_host,
                                  const int *stride_host, const int *pad_host, const int *dil_host,
                                  size_t *bitmap_offset, size_t *prefix_offset, size_t *nwords);
size_t pcd_rulebook_subm_ranked_workspace_bytes(int n, int kvol);
/* pcd_rulebook_subm_ranked4: the same for the map pcd_voxelize_hard_sorted hands out (one prefix per group of 4 bitmap
 * words): the SubM rulebook of level 1 (spconv_backbone.py:199-203, 'subm1' / 'res1') without a hash table. */
int pcd_rulebook_subm_ranked4(const int32_t *indices, int n, int batch, const int *shape_host,
                              const int *ksize_host, const int *dil_host, const uint32_t *bitmap,
                              const int32_t *prefix, int32_t *nbr, int32_t *pairs, int32_t *pair_num,
                              int pad_pairs, const int32_t *n_dev, void *workspace, size_t workspace_bytes,
                              void *stream, int row_order);
int pcd_rulebook_subm_ranked(const int32_t *indices, int n, int batch, const int *shape_host,
                             const int *ksize_host, const int *dil_host, const uint32_t *bitmap,
                             const int32_t *prefix, int32_t *nbr, int32_t *pairs, int32_t *pair_num,
                             int pad_pairs, const int32_t *n_dev, void *workspace, size_t workspace_bytes,
                             void *stream, int row_order);

/* ---- Column maps: the coordinate -> row map of a level whose rows are numbered z-fastest (PCD_ROWS_YXZ) ----------
 * In (b, y, x, z) order the rows of one BEV cell (a COLUMN) are consecutive and ordered by z, so a level's map is
 *     words  [B*H*W / 32]: { occupancy bits of 32 BEV cells, occupied cells in front of the word }       (8 bytes each)
 *     columns [<= rows]   : { z mask (64 bits), first row, rows }                                        (16 bytes each)
 * -- O(BEV area / 32) + O(rows) bytes instead of a bitmap over the (b, y, x, z) key space (371 M cells at level 1 of a
 * 4-frame Waymo batch).  The map lives in ONE caller-owned buffer of pcd_colmap_bytes(batch, shape (D, H, W), n_cap)
 * bytes (n_cap = row capacity of the level = column capacity; the same n_cap must be passed wherever the buffer is read).
 * D <= 62; the builds below cover dilation 1, kernels 3x3x3 and (3,1,1), strides 1 / 2 per axis (every conv of
 * pcdet/models/backbones_3d/spconv_backbone.py:69-293) and return PCD_ERR_UNSUPPORTED otherwise (0 from the
 * _workspace_bytes query): callers then take pcd_rulebook_conv_* / pcd_rulebook_subm.
 *   pcd_colmap_from_rows: the map of a row set given in (b, y, x, z) order (level 1: the key-ordered voxeliser's output).
 *   pcd_rulebook_subm_cm: pcd_rulebook_subm's outputs (bit for bit) for a 3x3x3 SubM conv (spconv_backbone.py:12-13) from
 *       the level's map: nine column lookups per row serve the 27 offsets; no hash table, no atomics.
 *   pcd_rulebook_conv_cm_{count,fill,build}: pcd_rulebook_conv_{count,fill,build}'s outputs for a strided conv
 *       (spconv_backbone.py:14-15,205-229) with row_order PCD_ROWS_YXZ, from the INPUT level's map; additionally writes
 *       the OUTPUT level's map (out_colmap, sized for n_out / n_out_cap rows).  An output column exists iff one of its
 *       kh x kw input columns does; its z mask is the OR of theirs, shifted by the padding, smeared over the kd taps and
 *       compressed by the stride: one thread per output BEV cell, no atomics, no map of the output volume.  Launches:
 *       count (+ class counts) -> emit map + coordinates (+ class offsets) -> both neighbour tables (+ class
 *       permutation) -> pair lists.  _count / _fill share one untouched workspace (the host reads n_out in between). */
size_t pcd_colmap_bytes(int batch, const int *shape_host, int n_cap);
/* Byte offset, inside a buffer of pcd_colmap_bytes(batch, shape, n_cap) bytes, of the map's counters {columns, rows} (two int32,
 * written by the build that produced the map); *ncol_cap_out receives its column capacity.  A strided build whose output z
 * range does not cover every input z numbers columns WITHOUT rows, so columns > rows is possible: check columns <= capacity
 * (com_amd.ops does: it rebuilds with a larger map in eager mode and records the count with the static plan's overflow guard). */
size_t pcd_colmap_counts_offset(int batch, const int *shape_host, int n_cap, int *ncol_cap_out);
size_t pcd_colmap_from_rows_workspace_bytes(int batch, const int *shape_host);
int pcd_colmap_from_rows(const int32_t *indices, int n, const int32_t *n_dev, int batch, const int *shape_host,
                         void *colmap, size_t colmap_bytes, void *workspace, size_t workspace_bytes, void *stream);
size_t pcd_rulebook_subm_cm_workspace_bytes(int n);
int pcd_rulebook_subm_cm(const int32_t *indices, int n, int batch, const int *shape_host, const void *colmap,
                         size_t colmap_bytes, int colmap_cap, int32_t *nbr, int32_t *pairs, int32_t *pair_num,
                         int pad_pairs, const int32_t *n_dev, void *workspace, size_t workspace_bytes, void *stream);
size_t pcd_rulebook_conv_cm_workspace_bytes(int n, int batch, const int *in_shape_host, const int *ksize_host,
                                            const int *stride_host, const int *pad_host);
int pcd_rulebook_conv_cm_count(int n, int batch, const int *in_shape_host, const int *ksize_host,
                               const int *stride_host, const int *pad_host, const void *in_colmap,
                               size_t in_colmap_bytes, int in_cap, int32_t *n_out_dev, void *workspace,
                               size_t workspace_bytes, void *stream);
int pcd_rulebook_conv_cm_fill(const int32_t *indices, int n, int batch, const int *in_shape_host,
                              const int *ksize_host, const int *stride_host, const int *pad_host,
                              const void *in_colmap, size_t in_colmap_bytes, int in_cap, int n_out,
                              int32_t *out_indices, void *out_colmap, size_t out_colmap_bytes, int32_t *nbr_in,
                              int32_t *nbr_out, int32_t *pairs, int32_t *pair_num, int pad_pairs,
                              const int32_t *n_dev, void *workspace, size_t workspace_bytes, void *stream);
int pcd_rulebook_conv_cm_build(const int32_t *indices, int n, int batch, const int *in_shape_host,
                               const int *ksize_host, const int *stride_host, const int *pad_host,
                               const void *in_colmap, size_t in_colmap_bytes, int in_cap, int n_out_cap,
                               int32_t *n_out_dev, int32_t *out_indices, void *out_colmap, size_t out_colmap_bytes,
                               int32_t *nbr_in, int32_t *nbr_out, int32_t *pairs, int32_t *pair_num, int pad_pairs,
                               int cls_tile, int32_t *perm, int vcap, int32_t *vstart_dev, const int32_t *n_dev,
                               void *workspace, size_t workspace_bytes, void *stream);
/* The same one-call build with COMPACT neighbour tables and no pair lists -- what a training step needs of a strided rulebook
 * (replaces the indice_pairs / indice_pair_num that spconv/pytorch/ops.py get_indice_pairs hands to SparseConv3d,
 * spconv_backbone.py:205,212,219, for kernel depth 3 and at most 8 stride-parity classes):
 *   nbr_out_packed [kh * kw][n_out_cap] u32: per (ky, kx) the three kz neighbours of an output row -- consecutive rows of one input
 *       column, rows being z-fastest -- as { first present row : 29 bits, presence of kz = 0, 1, 2 : 3 bits } (0 = none);
 *       read by pcd_sparse_conv_gather_gemm_packed;
 *   nbr_cls [8][vcap] i32: entry (j, v) = output row reached from input row perm[v] through the j-th kernel offset its class can
 *       use (ascending k), or -1: 27 / 8 entries per row on average; read by pcd_sparse_conv_dgrad_classes_v2 and
 *       pcd_sparse_conv_wgrad_classes (nbr_compact = 1).
 * 4 x 9 + 4 x 27 / 8 = 50 bytes per row instead of 2 x 108 (+ 8 per pair).  pcd_rulebook_conv_expand_nbr_out / _nbr_in rebuild
 * the 27-wide tables (nbr_out [3 kq][n_out], nbr_in [kvol][n]) for whoever wants them: same values as pcd_rulebook_conv_cm_build's. */
int pcd_rulebook_conv_cm_build_compact(const int32_t *indices, int n, int batch, const int *in_shape_host,
                                       const int *ksize_host, const int *stride_host, const int *pad_host,
                                       const void *in_colmap, size_t in_colmap_bytes, int in_cap, int n_out_cap,
                                       int32_t *n_out_dev, int32_t *out_indices, void *out_colmap, size_t out_colmap_bytes,
                                       uint32_t *nbr_out_packed, int32_t *nbr_cls, int cls_tile, int32_t *perm, int vcap,
                                       int32_t *vstart_dev, const int32_t *n_dev, void *workspace, size_t workspace_bytes,
                                       void *stream);
int pcd_rulebook_conv_expand_nbr_out(const uint32_t *nbr_out_packed, int kq, int n_out, const int32_t *n_out_dev,
                                     int32_t *nbr_out, void *stream);
int pcd_rulebook_conv_expand_nbr_in(const int32_t *nbr_cls, int vcap, const int32_t *perm, const int32_t *vstart_dev,
                                    const int *ksize_host, const int *stride_host, int n, int32_t *nbr_in, void *stream);

/* Optional per-channel reductions of the OUTPUT tile in the epilogue of pcd_sparse_conv_gather_gemm /
 * pcd_sparse_conv_dgrad_classes_v2 (bf16 outputs only; NULL or mode 0 = off).  The BatchNorm1d that follows every conv of
 * the reference backbones (spconv_backbone.py:21-25,50-66) needs these sums; taking them while the values are still in
 * registers replaces one streaming pass per BatchNorm and direction:
 *   mode 1 (forward)       partial[t] = { sum y, sum y^2 } of the rounded outputs  -> pcd_bn_forward_ld(ext_partial)
 *   mode 2 (data gradient) the output is dy of the BatchNorm(+ReLU) whose output was the conv's input:
 *                          partial[t] = { sum dz, sum dz*xhat }, dz = relu ? dy*(y > 0) : dy, xhat = (x-mean)*invstd;
 *                          y = that BatchNorm's output = the conv's own input features (required when relu)
 *                                                                               -> pcd_bn_backward_ld(ext_partial)
 * One row [2][c_out] per workgroup tile t; partial_rows must be >= pcd_sparse_conv_gather_gemm_tiles_dir(..) /
 * pcd_sparse_conv_dgrad_classes_tiles(..), which is also the row count to hand to the BatchNorm call.
 * mean / invstd must be 16-byte aligned.  Fixed summation order (deterministic). */
typedef struct PcdBnReduce {
    int mode;
    int relu;
    const void *x;            /* mode 2: BatchNorm input  [rows][c_out] bf16 */
    const void *y;            /* mode 2: BatchNorm output [rows][c_out] bf16 (NULL when relu == 0) */
    const float *mean, *invstd;
    float *partial;           /* out: [partial_rows][2][c_out] f32 */
    int partial_rows;
    /* Optional: the launch itself folds the partial rows into the PCD_BN_MID_ROWS rows the BatchNorm apply passes start
     * from (otherwise pcd_bn_forward_ld / pcd_bn_backward_ld run a small kernel for that -- one more dependent launch on the chain):
     * mid [PCD_BN_MID_ROWS][2][c_out] f64, handed to the BatchNorm call as ext_partial with ext_rows = PCD_BN_EXT_MID;
     * counters [PCD_BN_MID_ROWS * PCD_BN_COUNTER_STRIDE] i32 (one counter per 128-byte line) must be ZERO when the launch
     * starts and are zero again when it ends (keep them in a buffer zeroed once); partial_rows must then equal the
     * tile count exactly. */
    double *mid;
    int32_t *counters;
} PcdBnReduce;
#define PCD_BN_MID_ROWS 16
#define PCD_BN_COUNTER_STRIDE 32
#define PCD_BN_EXT_MID (-1)

/* Parity classes of the input rows of a strided conv, for its data gradient: input coordinate c reaches an output
 * cell through kernel index k only if (c + p - k*d) is a multiple of the stride, so the residues ((c + p) mod s) of
 * the three axes select the 1..8 offsets (of 27 for k = 3, s = 2) a row can use at all.
 *   perm   [vcap] i32 : virtual row -> input row (stable inside a class), -1 = padding; every class starts at a
 *                       multiple of `tile`; vcap >= round_up(n, tile) + (sd*sh*sw) * tile
 *   vstart [sd*sh*sw + 1] i32 on the DEVICE: first virtual row of every class, last entry = end.
 * pcd_sparse_conv_dgrad_classes_v2 then runs, per class, only that class's offsets (bit-identical to
 * pcd_sparse_conv_gather_gemm on nbr_in; c_dy >= 32, a power of two; tile must be 256). */
size_t pcd_rulebook_conv_classes_workspace_bytes(int n);
int pcd_rulebook_conv_classes(const int32_t *indices, int n, const int *stride_host, const int *pad_host, int tile,
                              int32_t *perm, int vcap, int32_t *vstart_dev, const int32_t *n_dev, void *workspace,
                              size_t workspace_bytes, void *stream);
/* nbr_compact = 1 reads the class-compact table nbr_cls [8][nbr_stride] (pcd_rulebook_conv_cm_build_compact; nbr_stride = the
 * permutation's capacity) instead of nbr_in [kvol][nbr_stride]: coalesced table reads instead of a gather through perm. */
int pcd_sparse_conv_dgrad_classes_v2(const void *dy, int n_dy_rows, int c_dy, const void *packed_w, const int32_t *nbr_in,
                                     int nbr_stride, int nbr_compact, const int *ksize_host, const int *stride_host,
                                     const int *pad_host, const int *dil_host, const int32_t *perm, const int32_t *vstart_dev,
                                     int vcap, int n_rows_in, int c_in, void *dx, int dx_dtype, const void *addend,
                                     const PcdBnReduce *bn_reduce, void *stream);
/* The forward of a strided conv over the PACKED output-side table nbr_out_packed [kvol / 3][nbr_stride] of
 * pcd_rulebook_conv_cm_build_compact; otherwise pcd_sparse_conv_gather_gemm (bit-identical result). */
int pcd_sparse_conv_gather_gemm_packed(const void *x, int n_rows_in, int c_in, const void *packed_w, const float *bias,
                                       const uint32_t *nbr_out_packed, int nbr_stride, int kvol, int n_rows_out,
                                       const int32_t *n_rows_out_dev, int c_out, void *y, int y_dtype, const void *addend,
                                       const PcdBnReduce *bn_reduce, void *stream);
int pcd_sparse_conv_dgrad_classes_tiles(int vcap, int n_rows_in);

/* ============================================================================================
 * (a8-a10) sparse convolution arithmetic -- replaces spconv's indice_conv fwd/bwd.
 *
 * Weights: the module parameter keeps spconv-2.x layout  weight [Cout][K][Cin] f32
 * (pcdet/models/detectors/detector3d_template.py:341-348).  pcd_pack_weight converts it to the
 * bf16 MFMA-fragment order the kernels read (call after every weight update):
 *   mode 0 (forward):  contraction over (k, cin),  outputs cout
 *   mode 1 (dgrad):    contraction over (k, cout), outputs cin
 * packed size in bytes = pcd_packed_weight_bytes(K, c_contract_pad, c_out_pad_to_16).
 * ============================================================================================ */
size_t pcd_packed_weight_bytes(int kvol, int cin, int cout, int mode);
int pcd_pack_weight(const float *weight, int kvol, int cin, int cout, int mode, void *packed,
                    void *stream);
/* The same conversion for a whole list of weights in ONE launch (a backbone re-packs ~40 small weights after
 * every optimizer step).  `table` is DEVICE memory, int64 [n][8], row i =
 *   { weight pointer, packed pointer, kvol, cin, cout, mode, first_block_i, 0 },
 * first_block_0 = 0, first_block_{i+1} = first_block_i + ceil(pcd_packed_weight_bytes(..)/2 / 2048)   (2048 packed elements per block);
 * total_blocks = first_block_n.  The table can be built once and reused while the pointers stay valid. */
int pcd_pack_weights_batched(const void *table, int n, int total_blocks, void *stream);

/* y[o] = bias + sum_k x[nbr[k'][o]] @ W[k],  k' = flip_k ? K-1-k : k.
 * Output-stationary gather-GEMM (no atomics, deterministic).  Used for
 *   forward : x = features [n_in][cin_pad] bf16, nbr = nbr_out [K][n_out], packed mode 0;
 *   dgrad   : x = dY [n_out][cout_pad], nbr = nbr_in [K][n_in] (SubM: nbr with flip_k = 1),
 *             packed mode 1.
 * n_rows_in = rows of x (bounds of the gathers), c_in = contraction channels (row stride of x, a power
 * of two >= 8), c_out = output channels (% 16 == 0),
 * nbr_stride = row stride (elements) of the nbr table.  y dtype PCD_BF16 or PCD_F32; bias f32 or NULL.
 * addend (NULL or [n_rows_out][c_out] of y's dtype) is added before the single rounding of y: the gradient of the
 * residual branch in the dgrad of a SparseBasicBlock's first conv (spconv_backbone.py:56-63) -- replaces the
 * elementwise add autograd would launch. */
int pcd_sparse_conv_gather_gemm(const void *x, int n_rows_in, int c_in, const void *packed_w, const float *bias,
                                const int32_t *nbr, int nbr_stride, int kvol, int flip_k,
                                int n_rows_out, const int32_t *n_rows_out_dev, int c_out, void *y,
                                int y_dtype, const void *addend, const PcdBnReduce *bn_reduce, void *stream);
/* number of workgroup tiles (= partial rows of bn_reduce) of that launch; < 0: error code.  is_dgrad: the launch is a DATA
 * GRADIENT (flip_k != 0 or bn_reduce->mode == 2): the library may pick a different kernel (tile height) for the two directions */
int pcd_sparse_conv_gather_gemm_tiles_dir(int n_rows_in, int c_in, int kvol, int n_rows_out, int c_out, int is_dgrad);
/* which kernel that launch runs: 0 = gather_gemm_kernel (fragment loads), 1 = ggw_kernel (LDS-DMA, loader / consumer
 * waves); for profiling tools that group launches by kernel name */
int pcd_sparse_conv_gather_gemm_variant(int n_rows_in, int c_in, int kvol, int n_rows_out, int c_out, int is_dgrad);

/* dW[cout][k][cin] = sum_{(i,o) in pairs[k]} dY[o][cout] * X[i][cin]   (f32, parameter layout).
 * Two launches: pcd_sparse_conv_wgrad_v2 fills partial results in `workspace` (MFMA kernel) -- per row-range slabs, or at
 * 128 x 128 channels one tile per (equal-pair chunk, offset) behind a small header --,
 * pcd_sparse_conv_wgrad_reduce sums them in a fixed order into dweight (deterministic, no atomics).
 * `dweight` of the first call is only used when pmax == 0 (it is zeroed); it may be NULL otherwise.
 * pairs[k][0] (rows of x, n_x_rows of them) must be ascending inside each k (canonical order): the
 * kernel partitions the work by ranges of x rows and binary-searches the pair list. */
size_t pcd_sparse_conv_wgrad_workspace_bytes(int kvol, int cin, int cout, int pmax);
/* n_x = rows of x; n_x_dev (may be NULL) = device-side count of the real rows of x when n_x is a capacity (static-shape mode): the
 * row-range splits then partition the real rows, so no workgroup -- and no XCD -- is left with an empty range */
int pcd_sparse_conv_wgrad_v2(const void *x, int n_x, const int32_t *n_x_dev, int cin_pad, int cin, const void *dy,
                             int n_dy, int cout, const int32_t *pairs, const int32_t *pair_num, int kvol, int pmax,
                             float *dweight, void *workspace, size_t workspace_bytes, void *stream);
/* The weight gradient of a STRIDED conv without pair lists (replaces the indice_pairs argument of spconv's
 * indice_conv_backward, spconv/pytorch/ops.py, for SparseConv3d layers spconv_backbone.py:205,212,219): every kernel offset
 * k is usable by the input rows of exactly one stride-parity class, and for those rows it (almost) always has an output, so
 * the pairs of offset k are {(i, nbr_in[k][i]) : i in class(k)} -- read off `perm` / `vstart_dev` (pcd_rulebook_conv_cm_build /
 * pcd_rulebook_conv_classes) and nbr_in [kvol][nbr_stride]; a missing output gathers a zero row.  Same workspace
 * (pcd_sparse_conv_wgrad_workspace_bytes(kvol, cin, cout, n_x)), same reduction (pmax = n_x); the result equals
 * pcd_sparse_conv_wgrad_v2's over the rulebook's pair lists to fp32 summation order (a cut output holds a slot with a zero row).  kvol <= 27, at most 8 classes, not 128 x 128 channels (unless option "wg128" = 0). */
int pcd_sparse_conv_wgrad_classes(const void *x, int n_x, const int32_t *n_x_dev, int cin_pad, int cin, const void *dy,
                                  int n_dy, int cout, const int32_t *nbr_in, int nbr_stride, const int *ksize_host,
                                  const int *stride_host, const int *dil_host, const int32_t *perm,
                                  const int32_t *vstart_dev, float *dweight, void *workspace, size_t workspace_bytes,
                                  void *stream, int nbr_compact);
/* nbr_compact = 1: `nbr_in` is the class-compact table nbr_cls [8][nbr_stride] of pcd_rulebook_conv_cm_build_compact (entry
 * (j, v): the j-th usable offset of the class, permutation slot v) -- the pairs of an offset are then two plain arrays. */
int pcd_sparse_conv_wgrad_reduce(int kvol, int cin, int cout, int pmax, float *dweight,
                                 const void *workspace, void *stream);
/* The same reduction for up to PCD_WGRAD_MAX_JOBS layers in ONE launch (each layer then needs its own workspace
 * until the call; jobs_host is read during the call, the jobs travel as kernel arguments). */
#define PCD_WGRAD_MAX_JOBS 32
typedef struct PcdWgradReduceJob {
    const void *workspace;
    float *dweight;
    int kvol, cin, cout, pmax;
    int splits;              /* 0: as planned by pcd_sparse_conv_wgrad_v2; > 0: slabs written by pcd_sparse_conv_wgrad_os */
    int layout;              /* of dweight: 0 = [cout][K][cin] (spconv weights), 1 = [cout][cin][K] (nn.Conv2d weights
                              * [cout, cin, 3, 3]: the dense 3x3 convs of the BEV stack write straight into .grad) */
    int cout_write;          /* 0 = cout; else only the first cout_write output channels are reduced and written (dweight
                              * holds cout_write rows): convs run with zero-padded output channels (the 1-3 channel
                              * final convs of the head towers, padded to 32) */
    int cin_write;           /* 0 = cin; else (layout 0, splits > 0) the slabs carry cin input channels per (co, k) and dweight
                              * only the first cin_write: a layer run on zero-padded input rows (conv_input 5 -> 16 on the window
                              * tiles: pcd_sparse_conv_subm_window_wgrad with c = 16) */
} PcdWgradReduceJob;
int pcd_sparse_conv_wgrad_reduce_batched(const PcdWgradReduceJob *jobs_host, int n_jobs, void *stream);
/* Output-stationary form for layers with 16 output channels (cin_pad 8 or 16, 3x3x3): walks the OUTPUT rows, reads dY in
 * order once and gathers only X through nbr_out [K][n_out] -- half the gathered rows of the pair form, which binds at
 * this width.  Writes pcd_sparse_conv_wgrad_os_splits(..) slabs [cout][K][cin] into `workspace` (splits * cout * K * cin
 * floats); reduce with pcd_sparse_conv_wgrad_reduce_batched (job.splits).  0 splits / PCD_ERR_UNSUPPORTED: not covered. */
int pcd_sparse_conv_wgrad_os_splits(int n_out_rows, int kvol, int cin_pad, int cout);
int pcd_sparse_conv_wgrad_os(const void *x, int n_x_rows, int cin_pad, int cin, const void *dy, int n_out_rows,
                             const int32_t *n_out_dev, int cout, const int32_t *nbr_out, int nbr_stride, int kvol,
                             void *workspace, size_t workspace_bytes, void *stream);

/* ============================================================================================
 * (a13/a14) BEV scatter -- replaces SparseConvTensor.dense() + the view in
 * pcdet/models/backbones_2d/map_to_bev/height_compression.py:20-25 and the per-batch loop of
 * pointpillar_scatter.py:17-37 (D == 1).   out [B][C*D][H][W], channel index c*D + z, every
 * element written (zeros included; no separate memset).  dtype: PCD_F32 or PCD_BF16 for both
 * features [n][c_stride] and out.  `gather` is the backward: dfeat[r][c] = dout[b][c*D+z][y][x].
 * workspace: pcd_bev_workspace_bytes(B, D, H, W) (a dense int32 row map).
 * ============================================================================================ */
size_t pcd_bev_workspace_bytes(int batch, int d, int h, int w);
int pcd_bev_scatter(const void *features, int c, int c_stride, int dtype, const int32_t *indices,
                    int n, const int32_t *n_dev, int batch, int d, int h, int w, void *out,
                    void *workspace, size_t workspace_bytes, void *stream);
int pcd_bev_gather(const void *dout, int c, int c_stride, int dtype, const int32_t *indices, int n,
                   const int32_t *n_dev, int batch, int d, int h, int w, void *dfeatures, void *stream);
/* channels-last variants: out / dout are [batch][h][w][c * d] (channel = c * d + z), i.e. the
 * torch.channels_last layout of the [batch, c * d, h, w] tensor HeightCompression returns
 * (height_compression.py:20-25) -- what MIOpen's bf16 convolutions of BaseBEVBackbone / CenterHead
 * (base_bev_backbone.py:30-112, center_head.py:75-99) consume without a layout change.  c % 8 == 0 (bf16) / 4 (f32),
 * d <= 8. */
int pcd_bev_scatter_nhwc(const void *features, int c, int c_stride, int dtype, const int32_t *indices, int n,
                         const int32_t *n_dev, int batch, int d, int h, int w, void *out, void *workspace,
                         size_t workspace_bytes, void *stream);
int pcd_bev_gather_nhwc(const void *dout, int c, int c_stride, int dtype, const int32_t *indices, int n,
                        const int32_t *n_dev, int batch, int d, int h, int w, void *dfeatures, void *stream);

/* ============================================================================================
 * (a11) fused sparse epilogue -- replaces the nn.BatchNorm1d(eps=1e-3, momentum=0.01) -> (+ residual)
 * -> nn.ReLU chains that SparseSequential / SparseBasicBlock apply to `.features` between convs
 * (pcdet/models/backbones_3d/spconv_backbone.py:21-25,50-66,73).
 *   forward : y = relu?( (x - mean) * invstd * gamma + beta + residual? ),  x/y/residual [n][c] of `dtype`;
 *             training != 0: batch statistics (biased var for normalisation, unbiased for running_var,
 *             running = (1-momentum)*running + momentum*batch), saved to save_mean / save_invstd [c];
 *             training == 0: running statistics.
 *   backward: dz = relu ? dy * (y > 0) : dy; dresidual = dz (may be NULL); dgamma, dbeta [c];
 *             dx = gamma*invstd*(dz - dbeta/n - xhat*dgamma/n)   (training) or gamma*invstd*dz (eval).
 *             y may be NULL when relu != 0 and the forward had NO residual: the mask is then recomputed from
 *             x, gamma, beta (required in that case), save_mean, save_invstd exactly as the forward computed
 *             it, which saves one [n][c] read in each of the two backward passes.
 * ext_partial (NULL = compute here): [ext_rows][2][c] sums already taken by a conv epilogue (PcdBnReduce); the
 *             statistics / reduction pass is then skipped.
 * c % 8 == 0 (bf16) / c % 4 == 0 (f32), c/piece a power of two <= 256.  Deterministic (no atomics).
 * ============================================================================================ */
size_t pcd_bn_workspace_bytes(int c);
/* out[c] = sum over the n rows of x [n][c] (bias gradient); workspace = pcd_bn_workspace_bytes(c). */
int pcd_col_sum(const void *x, int dtype, int n, int c, float *out, const int32_t *n_dev, void *workspace,
                size_t workspace_bytes, void *stream);
/* The OUTPUT (forward) / output GRADIENT (backward) of the BatchNorm may be a column block of a wider row-major matrix:
 * y_ld / dy_ld = row stride in elements (>= c, a multiple of the 16-byte piece; c for a matrix of its own).  Lets the two
 * deblock BatchNorms of BaseBEVBackbone write straight into the concatenated map and read their halves of its
 * gradient (base_bev_backbone.py:103-108 torch.cat) without a copy either way. */
int pcd_bn_forward_ld(const void *x, const void *residual, int dtype, int n, int c, const float *gamma,
                      const float *beta, float eps, float momentum, int training, float *running_mean,
                      float *running_var, int relu, void *y, int y_ld, float *save_mean, float *save_invstd,
                      const int32_t *n_dev, const float *ext_partial, int ext_rows, void *workspace,
                      size_t workspace_bytes, void *stream);
/* The statistics half of pcd_bn_forward_ld's training form alone, for an apply pass that lives elsewhere
 * (pcd_unet_bn_pairadd): mid [PCD_BN_MID_ROWS][2][c] f64 receives the folded column sums (sum x, sum x^2) of the n (> 0) rows
 * of x, taken by the same launches; ext_partial / ext_rows (>= 0) as there, x is then not read. */
int pcd_bn_stats_mid(const void *x, int dtype, int n, int c, const int32_t *n_dev, const float *ext_partial, int ext_rows,
                     double *mid, void *workspace, size_t workspace_bytes, void *stream);
int pcd_bn_backward_ld(const void *dy, int dy_ld, const void *x, const void *y, int dtype, int n, int c,
                       const float *gamma, const float *beta, const float *save_mean, const float *save_invstd,
                       int relu, int training, void *dx, void *dresidual, float *dgamma, float *dbeta,
                       const int32_t *n_dev, const float *ext_partial, int ext_rows, float *colsum_partial,
                       void *workspace, size_t workspace_bytes, void *stream);
/* colsum_partial (NULL = off): [pcd_bn_backward_colsum_rows(dtype, n, c)][c] f32, per-workgroup column sums of dx as
 * stored.  dx is dy of the conv in front of the BatchNorm, its column sum that conv's bias gradient
 * (spconv_backbone.py:37-44, bias=True inside SparseBasicBlock): pcd_col_sum_finalize adds the rows up in a fixed
 * order and replaces the pcd_col_sum pass over dx. */
int pcd_bn_backward_colsum_rows(int dtype, int n, int c);
/* up to PCD_COLSUM_MAX_JOBS column sums in ONE launch (jobs_host is read during the call; the jobs travel as kernel
 * arguments): a backbone finishes all its bias gradients at the end of the backward pass with a single kernel */
#define PCD_COLSUM_MAX_JOBS 32
typedef struct PcdColsumJob {
    const float *partial;   /* [rows][c] */
    float *out;             /* [c] */
    int rows, c;
} PcdColsumJob;
int pcd_col_sum_finalize(const PcdColsumJob *jobs_host, int n_jobs, void *stream);

/* ============================================================================================
 * (a15) update end of the data-parallel step: gradient-norm clipping + Adam on ONE flat fp32 buffer
 * (tools/train.py:165-166 DDP, tools/train_utils/train_utils.py:93-96 clip_grad_norm_ + optimizer.step();
 * torch.optim.Adam semantics: L2 weight decay added to the gradient, bias-corrected moments).
 *   grad holds the SUM of the ranks' gradients, pre_divisor = world size (1 on a single GPU): the update uses
 *   g = grad / pre_divisor * min(1, max_norm / (||grad / pre_divisor|| + 1e-6))   (max_norm <= 0: no clipping).
 *   step_dev[0] (device float) = number of updates done so far; incremented by the call.  norm_out (may be NULL)
 *   receives the gradient norm.  n % 4 == 0, buffers 16-byte aligned.  Two passes over the buffers, 3 launches.
 * ============================================================================================ */
size_t pcd_adam_flat_workspace_bytes(void);
/* decoupled_wd != 0 gives the reference's adam_onecycle rule -- OptimWrapper(true_wd=True, bn_wd=True),
 * tools/train_utils/optimization/__init__.py:19-32 + fastai_optim.py:135-150: every parameter is first multiplied
 * by (1 - lr * weight_decay), then Adam runs WITHOUT a weight-decay term; decoupled_wd == 0 is torch.optim.Adam's L2
 * form.  hyper_dev (may be NULL): device float[2] = {lr, beta1} of THIS step, overriding the host arguments, so a
 * OneCycle schedule (learning_schedules_fastai.py:60-77: lr and MOMS vary every step) can drive a replayed hipGraph;
 * the bias correction uses the current beta1 like torch.optim.Adam does.
 * schedule_dev (may be NULL): the WHOLE OneCycle schedule as a device table schedule_dev[schedule_len][2] = {lr, beta1} per
 * update (learning_schedules_fastai.py:60-77 evaluated once on the host): the kernel reads row min(*step_dev, len - 1) itself
 * -- no lookup launches in front of the step -- and mirrors the pair into hyper_dev.
 * zero_grad != 0: the gradient buffer is cleared as it is consumed (the next step's zero_grad without a fill launch). */
int pcd_adam_flat_step_v4(float *param, float *grad, int zero_grad, float *exp_avg, float *exp_avg_sq, size_t n, float lr,
                          float beta1, float beta2, float eps, float weight_decay, float max_norm, float pre_divisor,
                          int decoupled_wd, float *hyper_dev, const float *schedule_dev, int schedule_len, float *step_dev,
                          float *norm_out, void *workspace, size_t workspace_bytes, void *stream);

/* ============================================================================================
 * (f2) CenterHead target assignment on the device -- replaces the per-object Python / CPU loop of
 *      pcdet/models/dense_heads/center_head.py:104-161 (assign_target_of_single_head) for one head, all batch
 *      elements at once (the caller's loop :163-225), incl. centernet_utils.py:46-107 (Gaussian radius, drawing).
 *   gt_boxes [batch][n_boxes][code] f32 (x, y, z, dx, dy, dz, heading, ..., class), class 0 = padding;
 *   class_map_host[n_class_map]: dataset class id -> 1-based id inside this head, 0 = not in this head;
 *   outputs: heatmap [batch][head_classes][fm_h][fm_w] f32, ret_boxes [batch][num_max_objs][code] f32,
 *   inds / mask [batch][num_max_objs] int64 (the reference's dtypes); all zero-filled by the call.
 * ============================================================================================ */
size_t pcd_centerhead_assign_workspace_bytes(int batch, int num_max_objs);
int pcd_centerhead_assign_targets(const float *gt_boxes, int batch, int n_boxes, int code_size, const int *class_map_host,
                                  int n_class_map, int head_classes, int fm_w, int fm_h, int feature_map_stride,
                                  const float *voxel_size_xy_host, const float *range_xy_host, int num_max_objs,
                                  float gaussian_overlap, int min_radius, float *heatmap, float *ret_boxes,
                                  long long *inds, long long *mask, void *workspace, size_t workspace_bytes, void *stream);

/* (f2) CenterHead.get_loss of one head (center_head.py:226-262): cls_weight * neg_loss_cornernet(clamp(sigmoid(hm)),
 *      heatmap) (loss_utils.py:611-643) + loc_weight * sum_d code_weights[d] * RegLossCenterNet_d (loss_utils.py:
 *      1317-1390) -- and its gradients -- in 2 + 2 launches instead of ~100 elementwise launches, without the
 *      reference's host round trips (`if num_pos == 0`, `.item()`).  Predictions are addressed through element
 *      strides {batch, channel, y, x} (NCHW or channels-last), dtype PCD_F32 / PCD_BF16; arithmetic in fp32.
 *   forward : out[0] = loss, [1] = hm_loss, [2] = loc_loss, [3] = mean confidence at the positives (nan without any,
 *             as the reference), [4] = num_pos, [5] = number of objects, [6 .. 6 + D) = L1 per code dimension
 *   backward: d_hm / reg_grads (same layout and dtype as the predictions; every element is written) for an upstream
 *             gradient *grad_out (device scalar).  `out` is the forward's.
 *   regression branches in HEAD_ORDER (their channels concatenated give the D code dimensions of target_boxes). */
size_t pcd_centerhead_loss_workspace_bytes(int code_dims);
int pcd_centerhead_loss_forward(const void *hm, int hm_dtype, const long long *hm_strides_host /*[4]*/,
                                const float *gt_heatmap, int batch, int num_classes, int height, int width,
                                const void *const *reg_ptrs_host, const int *reg_channels_host, int reg_dtype,
                                const long long *reg_strides_host /*[n_reg][4]*/, int n_reg, const long long *inds,
                                const long long *masks, const float *target_boxes, int num_max_objs,
                                const float *code_weights /*device [D]*/, float cls_weight, float loc_weight,
                                float *out /*device [6 + D]*/, void *workspace, size_t workspace_bytes, void *stream);
int pcd_centerhead_loss_backward(const void *hm, void *d_hm, int hm_dtype, const long long *hm_strides_host,
                                 const float *gt_heatmap, int batch, int num_classes, int height, int width,
                                 const void *const *reg_ptrs_host, void *const *reg_grads_host,
                                 const int *reg_channels_host, int reg_dtype, const long long *reg_strides_host,
                                 int n_reg, const long long *inds, const long long *masks, const float *target_boxes,
                                 int num_max_objs, const float *code_weights, float cls_weight, float loc_weight,
                                 const float *out, const float *grad_out, void *stream);

/* ============================================================================================
 * (f3) AnchorHeadSingle on the device (the dense head of PointPillars, SECOND and the first stage of PV-RCNN:
 *      tools/cfgs/waymo_models/{pointpillar_1x,second,pv_rcnn}.yaml) -- com_amd/csrc/anchorhead.hip.
 *      AxisAlignedTargetAssigner (MATCH_HEIGHT False, POS_FRACTION < 0, NORM_BY_NUM_EXAMPLES False) + ResidualCoder (7 codes)
 *      + WeightedSmoothL1Loss + direction classifier.  Every entry point takes a stream, allocates nothing, reads nothing
 *      back and launches a fixed number of kernels (3 / 2 / 1 / 1).
 *
 *   Anchors are described, never stored: anchor n of a frame is (y, x, kind) = (n / (W * A), n / A % W, n % A) -- the
 *   reference's (y, x, class, size, rotation) order, i.e. the channel order of conv_cls -- with
 *     kinds   device f32 [A][PCD_ANCHOR_KIND_FLOATS]: dx, dy, dz, heading, z of the centre (bottom height + dz / 2),
 *             class slot, half extents along x and y of the axis-aligned BEV box (box_utils.py:322-324 evaluated on the
 *             host), diagonal sqrt(dx^2 + dy^2), 0;  A <= PCD_ANCHOR_MAX_KINDS
 *     classes device f32 [n_classes][PCD_ANCHOR_CLASS_FLOATS]: matched_threshold, unmatched_threshold, 1-based class id
 *             of the ground-truth boxes that compete for this class's anchors, 0;  n_classes <= PCD_ANCHOR_MAX_CLASSES
 *     shifts  device f32 [n_classes][W + H]: the host generator's x table, then its y table (anchor_generator.py:34-39),
 *             so that the device uses bit-identical anchor coordinates and not a re-derived origin + i * stride
 *   Prediction maps: [B, H, W, C] views addressed through element strides {batch, channel, y, x} (three rows: cls, box,
 *   dir), one dtype (PCD_F32 / PCD_BF16) for the three, arithmetic in fp32; channel of (kind k, item j) = k * items + j.
 *
 *   pcd_anchor_assign_targets  axis_aligned_target_assigner.py:36-210 for the whole batch and all classes.
 *     gt_boxes [B][M][8] f32 (x, y, z, dx, dy, dz, heading, 1-based class id; zero rows = padding, anywhere).
 *     box_cls_labels int32 [B][N] (-1 ignore, 0 background, class id), box_reg_targets f32 [B][N][7] (ResidualCoder.
 *     encode_torch at the positives, 0 elsewhere), reg_weights f32 [B][N], gt_index int32 [B][N] (the box a positive
 *     regresses to = its arg-max box, -1 elsewhere; may be NULL), num_pos int32 [B].  Nearest-BEV IoU in fp32 in the
 *     reference's operation order without contraction; per anchor the maximum over its class's boxes (lowest index on
 *     ties); every anchor whose IoU with a box EQUALS that box's non-zero maximum is positive with ITS OWN arg-max box
 *     (:155-158); maximum >= matched: positive; else < unmatched: background; else ignore.
 *   pcd_anchor_loss_forward   anchor_head_template.py:102-227: out[0] = rpn_loss, [1] = rpn_loss_cls, [2] = rpn_loss_loc,
 *     [3] = rpn_loss_dir (weighted, device f32[4]).  Sums: per-workgroup partials, then one ordered pass (no float atomics).
 *     num_class == 1: class-agnostic labels (:114-116).  dir_preds NULL: no direction classifier.
 *   pcd_anchor_loss_backward  gradients with respect to the three maps (same layout and dtype, every element written)
 *     for an upstream gradient *grad_out (device scalar).
 *   pcd_anchor_decode         generate_predicted_boxes (:229-276): batch_box_preds f32 [B][N][7] (ResidualCoder.
 *     decode_torch + the direction-bin correction), batch_cls_preds f32 [B][N][num_class] (the logits).
 * ============================================================================================ */
#define PCD_ANCHOR_KIND_FLOATS 10
#define PCD_ANCHOR_CLASS_FLOATS 4
#define PCD_ANCHOR_MAX_KINDS 32
#define PCD_ANCHOR_MAX_CLASSES 16
size_t pcd_anchor_assign_workspace_bytes(int batch, int n_boxes);
int pcd_anchor_assign_targets(const float *gt_boxes, int batch, int n_boxes, const float *kinds, int n_kinds,
                              const float *classes, int n_classes, const float *shifts, int height, int width,
                              int *box_cls_labels, float *box_reg_targets, float *reg_weights, int *gt_index, int *num_pos,
                              void *workspace, size_t workspace_bytes, void *stream);
size_t pcd_anchor_loss_workspace_bytes(int batch, int height, int width, int n_kinds);
int pcd_anchor_loss_forward(const void *cls_preds, const void *box_preds, const void *dir_preds, int dtype,
                            const long long *strides_host /*[3][4]*/, const int *box_cls_labels,
                            const float *box_reg_targets, const int *num_pos, int batch, int height, int width, int n_kinds,
                            int num_class, int num_dir_bins, const float *kinds, const float *code_weights /*device [7]*/,
                            float cls_weight, float loc_weight, float dir_weight, float dir_offset, float *out /*device [4]*/,
                            void *workspace, size_t workspace_bytes, void *stream);
int pcd_anchor_loss_backward(const void *cls_preds, const void *box_preds, const void *dir_preds, void *d_cls, void *d_box,
                             void *d_dir, int dtype, const long long *strides_host, const int *box_cls_labels,
                             const float *box_reg_targets, const int *num_pos, int batch, int height, int width, int n_kinds,
                             int num_class, int num_dir_bins, const float *kinds, const float *code_weights, float cls_weight,
                             float loc_weight, float dir_weight, float dir_offset, const float *grad_out, void *stream);
int pcd_anchor_decode(const void *cls_preds, const void *box_preds, const void *dir_preds, int dtype,
                      const long long *strides_host, int batch, int height, int width, int n_kinds, int n_classes,
                      int num_class, int num_dir_bins, const float *kinds, const float *shifts, float dir_offset,
                      float dir_limit_offset, float *batch_box_preds, float *batch_cls_preds, void *stream);

/* ============================================================================================
 * (f3m) AnchorHeadMulti on the device (the dense head of tools/cfgs/nuscenes_models/cbgs_{second,pp}_multihead.yaml,
 *       lyft_models/cbgs_second{,-nores}_multihead.yaml, kitti_models/second_multihead.yaml; USE_MULTIHEAD +
 *       SEPARATE_MULTIHEAD) -- com_amd/csrc/anchorhead_multi.hip.  The assignment rule, the focal / smooth-L1 / direction
 *       arithmetic and the ordered sums are those of (f3); what differs is the anchor order, per-head prediction maps,
 *       ResidualCoder in full (any code size, sin/cos heading), WeightedL1Loss and pos_cls_weight / neg_cls_weight.
 *       Every entry point takes a stream, allocates nothing, reads nothing back and launches a fixed number of kernels
 *       (3 / 2 / 1 / 1); one launch covers all heads.
 *
 *   Anchor order (axis_aligned_target_assigner.py:69, anchor_head_template.py:244): every class's anchors permuted to
 *   (size, rotation, z, y, x), classes concatenated: anchor n = (g * H + y) * W + x with g the GLOBAL kind (class in
 *   ANCHOR_GENERATOR_CONFIG order, then size, then rotation); N = n_kinds * H * W.  Head h owns the kinds
 *   [kind0, kind0 + n_kinds) and the classes [class0, class0 + num_class); the heads tile both ranges in order.
 *     kinds   device f32 [n_kinds][PCD_ANCHOR_MULTI_KIND_FLOATS]: the PCD_ANCHOR_KIND_FLOATS of (f3), then cos and sin of
 *             the heading as torch computes them on the host (so that the sin/cos codes use the reference's anchor values)
 *     classes, shifts: as in (f3)
 *   Prediction maps: one PcdAnchorMultiHead per head (host array, passed by value to the kernels): cls / box / dir map
 *   pointers (dir NULL in every head: no direction classifier), their gradients, element strides {batch, channel, y, x};
 *   one dtype for all maps.  Channel of (local anchor a, item j) = a * items + j with items = num_class of the head, `code`
 *   or the number of bins -- the reference's view(-1, A_h, items, H, W) (anchor_head_multi.py:124-137).  For a head with
 *   SEPARATE_REG_CONFIG the box map is the channel concatenation of its branches in REG_LIST order; the same formula then
 *   cuts across the branches when A_h > 1, as the reference's view does.
 *
 *   pcd_anchor_multi_assign_targets  gt_boxes [B][M][code_gt + 1] (code_gt 7 | 9; the 1-based class id last; zero rows =
 *     padding, anywhere).  box_reg_targets f32 [B][N][code], code = code_gt + sincos: six position / size codes, then
 *     rg - ra | (cos rg - cos ra, sin rg - sin ra), then the extra columns (box_coder_utils.py:13-43).  The other outputs
 *     as pcd_anchor_assign_targets; num_pos counts the positives of all heads.
 *   pcd_anchor_multi_loss_forward / _backward  anchor_head_multi.py:245-373.  Focal weight of an anchor = (pos_cls_weight |
 *     neg_cls_weight) / max(num_pos[b], 1); a head's one-hot target is its class slice of the global one-hot; num_class == 1
 *     (all heads together): class-agnostic.  reg_l1 == 0: WeightedSmoothL1Loss (beta 1/9), 1: WeightedL1Loss; with
 *     direction maps the sin-difference substitution on code 6 and the direction cross entropy.  code_weights device
 *     f32 [code].  out device f32[4] = rpn_loss, _cls, _loc, _dir over all heads, weighted; per-workgroup partials + one
 *     ordered pass.  The backward writes every element of every head's gradient maps.
 *   pcd_anchor_multi_decode  batch_box_preds f32 [B][N][code - sincos] (decode_torch: atan2(sint + sin ra, cost + cos ra)
 *     when sincos; + the direction-bin correction with direction maps); cls_out_host[h]: device f32 [B][N_h][num_class_h],
 *     the logits of head h (N_h = n_kinds_h * H * W).
 * ============================================================================================ */
#define PCD_ANCHOR_MULTI_KIND_FLOATS 12
#define PCD_ANCHOR_MULTI_MAX_HEADS 8
#define PCD_ANCHOR_MULTI_MAX_CODE 10
typedef struct PcdAnchorMultiHead {
    const void *map[3];                       /* cls, box, dir (or NULL) */
    void *grad[3];                            /* their gradients (backward only) */
    long long strides[3][4];                  /* element strides {batch, channel, y, x} of each map */
    int kind0, n_kinds, class0, num_class;
} PcdAnchorMultiHead;
size_t pcd_anchor_multi_assign_workspace_bytes(int batch, int n_boxes);
int pcd_anchor_multi_assign_targets(const float *gt_boxes, int batch, int n_boxes, int code_gt, int sincos,
                                    const float *kinds, int n_kinds, const float *classes, int n_classes,
                                    const float *shifts, int height, int width, int *box_cls_labels, float *box_reg_targets,
                                    float *reg_weights, int *gt_index, int *num_pos, void *workspace, size_t workspace_bytes,
                                    void *stream);
size_t pcd_anchor_multi_loss_workspace_bytes(int batch, int height, int width, int n_kinds);
int pcd_anchor_multi_loss_forward(const PcdAnchorMultiHead *heads, int n_heads, int dtype, const int *box_cls_labels,
                                  const float *box_reg_targets, const int *num_pos, int batch, int height, int width,
                                  int n_kinds, int num_class, int code, int reg_l1, int num_dir_bins, const float *kinds,
                                  const float *code_weights, float pos_cls_weight, float neg_cls_weight, float cls_weight,
                                  float loc_weight, float dir_weight, float dir_offset, float *out /*device [4]*/,
                                  void *workspace, size_t workspace_bytes, void *stream);
int pcd_anchor_multi_loss_backward(const PcdAnchorMultiHead *heads, int n_heads, int dtype, const int *box_cls_labels,
                                   const float *box_reg_targets, const int *num_pos, int batch, int height, int width,
                                   int n_kinds, int num_class, int code, int reg_l1, int num_dir_bins, const float *kinds,
                                   const float *code_weights, float pos_cls_weight, float neg_cls_weight, float cls_weight,
                                   float loc_weight, float dir_weight, float dir_offset, const float *grad_out, void *stream);
int pcd_anchor_multi_decode(const PcdAnchorMultiHead *heads, int n_heads, int dtype, int batch, int height, int width,
                            int n_kinds, int n_classes, int code, int sincos, int num_dir_bins, const float *kinds,
                            const float *shifts, float dir_offset, float dir_limit_offset, float *batch_box_preds,
                            float *const *cls_out_host, void *stream);

/* ============================================================================================
 * (f3b) The COM curriculum on the anchor head: CurriculumAnchorHeadSingle and its head_zoo variants (_x1, _car, _car_x2)
 *       over AnchorHeadCurriculum / CurriculumAxisAlignedTargetAssigner / CurriculumSigmoidFocalClassificationLoss --
 *       com_amd/csrc/anchorhead_cur.hip.  Tables, maps and labels as in (f3); every entry point takes a stream, allocates
 *       nothing and reads nothing back.
 *
 *   pcd_anchor_cur_cluster   pcdet/models/dense_heads/curri_anchor_head_single.py:43-96 (PCD_ANCHOR_CUR_CLUSTER_BASE) and
 *     head_zoo.py:12-65 (_X1), :68-104 (_CAR), :107-140 (_CAR_X2): group int64 [B][M], the value each box holds after all of
 *     the reference's overwriting assignments.  BASE and X1 branch on `class_id.max() == 1` over the whole batch
 *     (:81, head_zoo.py:50,59): the maximum is reduced on the device in the same (single-block) launch.
 *   pcd_anchor_cur_groups    target_assigner/curri_axis_aligned_target_assigner.py:246-311 (POS_FRACTION < 0): groups int32
 *     [B][N] = group[b][gt_index] at the positives, 0 where box_cls_labels == 0, -1 at ignored anchors.
 *   pcd_anchor_cur_loss_forward   anchor_head_curriculum.py:103-256 (get_cls_layer_loss, get_box_reg_layer_loss, get_loss)
 *     with pcdet/utils/loss_utils.py:79-331.  num_class must be 1 (PCD_ERR_UNSUPPORTED otherwise: the reference's
 *     get_box_reg_layer_loss multiplies (B, N) by (B, N, C)).  Four launches:
 *       statistics (:150-181, :200-214)  over the grouped positives: sigmoid sum, sum of squares, count; the 96 group
 *         sums and counts -- 64-bit fixed-point integer atomics into accum (order independent, bit-identical runs)
 *       state (:183-197, :240-247)  one block: state double[4] = {mean, std, stored flag, 0} (first update stores, later
 *         ones are an EMA with factor cur->ema; untouched without a grouped positive or with ucl == 0); conf_sum /
 *         conf_num f32 [96] of this step (confidence_all), added to epoch_conf / epoch_num; saved f32 [8] = threshold,
 *         variance, then the epoch_table row; accum cleared for the next step (accum: 195 x u64, zero before the first)
 *       loss (:236-300 weight, times the focal term, the smooth-L1 weights and the direction weights) + ordered finish:
 *         out as pcd_anchor_loss_forward.  ucl == 0: weight 1, bit-identical to pcd_anchor_loss_forward.
 *     epoch_table device f32 [4] = {height, elongation, SME gate (epoch >= SME), 0} of class 0 at the current epoch:
 *     everything that depends on the epoch (START / END / INV / FIXED / CUT are folded into the height by the host).
 *   pcd_anchor_cur_loss_backward  weight x the plain anchor gradient (the weight is detached, :298); reads the `saved`
 *     of its forward, never the live state.
 * ============================================================================================ */
#define PCD_ANCHOR_CUR_GROUPS 96
#define PCD_ANCHOR_CUR_ACCUM (3 + 2 * PCD_ANCHOR_CUR_GROUPS)
#define PCD_ANCHOR_CUR_CLUSTER_BASE 0
#define PCD_ANCHOR_CUR_CLUSTER_X1 1
#define PCD_ANCHOR_CUR_CLUSTER_CAR 2
#define PCD_ANCHOR_CUR_CLUSTER_CAR_X2 3
typedef struct PcdAnchorCurriculum {        /* LOSS_CURRICULUM as CurriculumSigmoidFocalClassificationLoss.__init__ reads it */
    int ucl, oto, sm, sma, norm;
    float smt, pos_norm, neg_norm;          /* SMT; 0.5 / (1 - cdf(OFFSET)) * POSW; 0.5 / cdf(OFFSET) */
    double offset, ema;                     /* OFFSET; the EMA factor (the reference uses the focal alpha, 0.25) */
} PcdAnchorCurriculum;
int pcd_anchor_cur_cluster(const float *gt_boxes, int batch, int n_boxes, int code_size, const float *true_object,
                           const float *occupancy_ratio, const float *facade_type, int variant, long long *group,
                           void *stream);
int pcd_anchor_cur_groups(const int *box_cls_labels, const int *gt_index, const long long *group, int batch, int n_anchors,
                          int n_boxes, int *groups, void *stream);
size_t pcd_anchor_cur_loss_workspace_bytes(int batch, int height, int width, int n_kinds);
int pcd_anchor_cur_loss_forward(const void *cls_preds, const void *box_preds, const void *dir_preds, int dtype,
                                const long long *strides_host /*[3][4]*/, const int *box_cls_labels,
                                const float *box_reg_targets, const int *num_pos, const int *groups, int batch, int height,
                                int width, int n_kinds, int num_class, int num_dir_bins, const float *kinds,
                                const float *code_weights, float cls_weight, float loc_weight, float dir_weight,
                                float dir_offset, const PcdAnchorCurriculum *cur, const float *epoch_table, double *state,
                                unsigned long long *accum, float *conf_sum, float *conf_num, float *epoch_conf,
                                float *epoch_num, float *saved /*device [8]*/, float *out /*device [4]*/, void *workspace,
                                size_t workspace_bytes, void *stream);
int pcd_anchor_cur_loss_backward(const void *cls_preds, const void *box_preds, const void *dir_preds, void *d_cls, void *d_box,
                                 void *d_dir, int dtype, const long long *strides_host, const int *box_cls_labels,
                                 const float *box_reg_targets, const int *num_pos, const int *groups, int batch, int height,
                                 int width, int n_kinds, int num_class, int num_dir_bins, const float *kinds,
                                 const float *code_weights, float cls_weight, float loc_weight, float dir_weight,
                                 float dir_offset, const PcdAnchorCurriculum *cur, const float *saved, const float *grad_out,
                                 void *stream);

/* ============================================================================================
 * (f2, BASELINE config 3) The COM curriculum head on the device.  Replaces, for one head and the whole batch:
 *   pcd_com_cluster_groups   CurriculumCenterHead.cluster         pcdet/models/dense_heads/curriculum_center_head.py:414-459
 *   pcd_com_assign_targets   assign_targets / assign_target_of_single_head  same file :108-307 (+ centernet_utils.py:46-106)
 *   pcd_com_loss_forward     CurriculumCenterHead.get_loss of one head (:309-358) = FocalLossCenterCurriculum.neg_loss
 *                            (pcdet/utils/loss_utils.py:1178-1310) incl. confidence_of_all_groups (:1134-1176: the
 *                            conf_shape (3, 96) sums / counts a 288-iteration host loop produces every step), the
 *                            average-confidence EMA (:1214), the UCL per-object weights (:1231-1291, drawn into
 *                            heatmap_mask and box_mask in place as the reference does) + RegLossCenterNet with the
 *                            float box mask (:1317-1390)
 *   pcd_com_loss_backward    autograd of the above w.r.t. the heat-map logits and the regression maps
 * No host synchronisation anywhere (the reference: one .item() per object and per head, torch.where per group).
 *
 *   gt_boxes [B][M][code] f32, last column = 1-based class id (0 = padding); true_object / occupancy_ratio /
 *   facade_type / num_points_in_gt [B][M] f32 (load_data_to_gpu casts everything to float); group [B][M] i64.
 *   radius_map [B][num_max][cols] i64, cols = 5: (class in head, centre x, centre y, radius, group), 4 without groups.
 *   mask / box_mask [B][num_max] f32 (the reference's float `masks`), heatmap_mask [B][C][H][W] f32.
 *   owner [B][C][H][W] i32: scratch, zeroed ONCE by its owner (the kernels return it to zero); mask_sum [C][H][W] f32:
 *   written by the forward pass for the backward pass (both only touched when cur.ucl != 0; may be NULL otherwise).
 *   state double[2]: {EMA of the average confidence (in/out), this step's average confidence (out)}.
 *   out f32[6 + dims]: loss, hm_loss, loc_loss, avg_confidence, num_pos (mask-weighted), sum of box_mask, L1 per dim.
 *   conf_all / num_all f32[conf_classes * conf_groups]: this step's sums / counts; conf_epoch / num_epoch (may be NULL):
 *   += them (the epoch sums train_utils.py:111-112,208 builds from a Python list).
 * The [B, 1, C, H, W] mask broadcast of loss_utils.py:1293-1297 (every frame's term weighted by the frame-SUM of the
 * mask) is reproduced as it stands -- fixture G12 holds the reference's numbers. */
#define PCD_COM_CLUSTER_X5 0        /* CurriculumCenterHead.cluster (used by CurriculumCenterHead_x5, head_zoo.py:145-149) */
typedef struct PcdComCurriculum {   /* MODEL.DENSE_HEAD.LOSS_CURRICULUM as FocalLossCenterCurriculum.__init__ reads it */
    int ucl;                        /* UCL (default True) */
    int fix_threshold;              /* FIX */
    int straight;                   /* STRAIGHT */
    int tuning;                     /* TUNING */
    int only_center;                /* CENTER */
    int apply;                      /* START <= epoch <= END, evaluated by the caller */
    int add;                        /* ADD */
    int radius;                     /* RADIUS (0 = the object's own Gaussian radius + ADD) */
    double k_straight;              /* K */
    double elongation;              /* ELONGATION */
    double height;                  /* HEIGHT */
    double alpha;                   /* ALPHA */
    double threshold;               /* self.threshold: 0.5 (loss_utils.py:1054; the YAML's THRESHOLD key is not read) */
    int conf_classes, conf_groups;  /* conf_shape; 0, 0 = None */
} PcdComCurriculum;
int pcd_com_cluster_groups(const float *gt_boxes, int batch, int n_boxes, int code_size, const float *true_object,
                           const float *occupancy_ratio, const float *facade_type, int variant, long long *group,
                           void *stream);
size_t pcd_com_assign_workspace_bytes(int batch, int num_max_objs);
/* gate_min_points = (epoch <= EPOCH_THRED): objects with num_points_in_gt < min_points are skipped (:178-179);
 * class_map_host as for pcd_centerhead_assign_targets; group may be NULL (radius_map column 4 = 0) */
int pcd_com_assign_targets(const float *gt_boxes, int batch, int n_boxes, int code_size, const int *class_map_host,
                           int n_class_map, int head_classes, int fm_w, int fm_h, int feature_map_stride,
                           const float *voxel_size_xy_host, const float *range_xy_host, int num_max_objs,
                           float gaussian_overlap, int min_radius, const float *num_points_in_gt, const long long *group,
                           int gate_min_points, float min_points, float *heatmap, float *ret_boxes, long long *inds,
                           float *mask, long long *radius_map, int radius_map_cols, float *heatmap_mask, void *workspace,
                           size_t workspace_bytes, void *stream);
size_t pcd_com_loss_workspace_bytes(int batch, int num_max_objs);
int pcd_com_loss_forward(const void *hm, int hm_dtype, const long long *hm_strides_host, const float *gt_heatmap, int batch,
                         int num_classes, int height, int width, const void *const *reg_ptrs_host,
                         const int *reg_channels_host, int reg_dtype, const long long *reg_strides_host, int n_reg,
                         const long long *inds, float *box_mask, const float *target_boxes, const long long *radius_map,
                         int radius_map_cols, int num_max_objs, float *heatmap_mask, int32_t *owner, float *mask_sum,
                         const PcdComCurriculum *cur_host, const float *code_weights, float cls_weight, float loc_weight,
                         double *state, float *out, float *conf_all, float *num_all, float *conf_epoch, float *num_epoch,
                         void *workspace, size_t workspace_bytes, void *stream);
int pcd_com_loss_backward(const void *hm, void *d_hm, int hm_dtype, const long long *hm_strides_host,
                          const float *gt_heatmap, int batch, int num_classes, int height, int width,
                          const void *const *reg_ptrs_host, void *const *reg_grads_host, const int *reg_channels_host,
                          int reg_dtype, const long long *reg_strides_host, int n_reg, const long long *inds,
                          const float *box_mask, const float *target_boxes, int num_max_objs, const float *mask_sum,
                          const float *code_weights, float cls_weight, float loc_weight, const float *out,
                          const float *grad_out, void *stream);

/* ============================================================================================
 * (f4) PV-RCNN stage-2 natives -- the stacked-batch PointNet++ ops of pcdet/ops/pointnet2/pointnet2_stack (binder
 *      src/pointnet2_api.cpp; Python callers pointnet2_utils.py:8-303, voxel_query_utils.py:9-47).  "Stacked": the
 *      points of all batch elements are concatenated, *_batch_cnt[B] (device int32) give the counts.  Semantics are
 *      the reference kernels' (first nsample hits in ascending index, their tie rules); float32 / int32.
 *   pcd_ball_query_stack        ball_query_gpu.cu:16-66   idx [M][nsample]; row 0 = -1 when the ball is empty
 *   pcd_group_points_stack      group_points_gpu.cu:76-107 out [M][C][nsample] (+ _grad: scatter-add, atomics)
 *   pcd_stack_farthest_point_sampling  sampling_gpu.cu:188-327 (temp must be filled with 1e10 by the caller)
 *   pcd_three_nn_stack          interpolate_gpu.cu:16-76  dist2 [N][3] (squared), idx [N][3] (global row ids)
 *   pcd_three_interpolate_stack interpolate_gpu.cu:100-117 (+ _grad :140-155, atomics)
 *   pcd_voxel_query_stack       voxel_query_gpu.cu:10-88
 * ============================================================================================ */
int pcd_ball_query_stack(int B, int M, float radius, int nsample, const float *new_xyz, const int32_t *new_xyz_batch_cnt,
                         const float *xyz, const int32_t *xyz_batch_cnt, int32_t *idx, void *stream);
int pcd_group_points_stack(int B, int M, int C, int nsample, const float *features, const int32_t *features_batch_cnt,
                           const int32_t *idx, const int32_t *idx_batch_cnt, float *out, void *stream);
int pcd_group_points_stack_grad(int B, int M, int C, int nsample, const float *grad_out, const int32_t *idx,
                                const int32_t *idx_batch_cnt, const int32_t *features_batch_cnt,
                                float *grad_features_zeroed, void *stream);
int pcd_stack_farthest_point_sampling(int B, const float *xyz, float *temp_1e10, const int32_t *xyz_batch_cnt,
                                      int32_t *idxs, const int32_t *num_sampled_points, void *stream);
/* cooperative form for large frames (4096 keypoints of ~160 k raw points, voxel_set_abstraction.py:236-263): 256 / B (<= 64)
 * workgroups share a frame, same selected points (same total order of the argmax); PCD_ERR_UNSUPPORTED when B > 128 or a
 * frame's slice does not fit LDS -- fall back to the call above.  max_cnt_host >= every frame's point count. */
/* Bucket-pruned EXACT form for large frames (round 6; the default of com_amd.pointnet2_stack): the frame's points are binned
 * once along a Z-curve into buckets of 64..256 points that keep their bounding box and their farthest point; a new centre only visits the buckets
 * whose box is closer than their largest running distance -- provably the only ones that can change, in float arithmetic --
 * so an iteration touches ~5 k of 160 k points and needs no inter-workgroup exchange (one workgroup per frame).  Same selected
 * points as pcd_stack_farthest_point_sampling, ties included (sampling_gpu.cu:188-348).  total_points = rows of xyz;
 * max_cnt_host >= every frame's point count (PCD_ERR_UNSUPPORTED beyond 2048 x 256 points per frame). */
size_t pcd_stack_fps_buckets_workspace_bytes(int B, int total_points);
int pcd_stack_farthest_point_sampling_buckets(int B, const float *xyz, const int32_t *xyz_batch_cnt, int32_t *idxs,
                                              const int32_t *num_sampled_points, int total_points, int max_cnt_host,
                                              void *workspace, size_t workspace_bytes, void *stream);
size_t pcd_stack_fps_coop_workspace_bytes(int B);
int pcd_stack_farthest_point_sampling_coop(int B, const float *xyz, const int32_t *xyz_batch_cnt, int32_t *idxs,
                                           const int32_t *num_sampled_points, int max_cnt_host, void *workspace,
                                           size_t workspace_bytes, void *stream);
int pcd_three_nn_stack(int B, int N, const float *unknown, const int32_t *unknown_batch_cnt, const float *known,
                       const int32_t *known_batch_cnt, float *dist2, int32_t *idx, void *stream);
int pcd_three_interpolate_stack(int N, int C, const float *features, const int32_t *idx, const float *weight, float *out,
                                void *stream);
int pcd_three_interpolate_stack_grad(int N, int C, const float *grad_out, const int32_t *idx, const float *weight,
                                     float *grad_features_zeroed, void *stream);
int pcd_voxel_query_stack(int M, int R1, int R2, int R3, int nsample, float radius, int z_range, int y_range, int x_range,
                          const float *new_xyz, const float *xyz, const int32_t *new_coords, const int32_t *point_indices,
                          int32_t *idx, void *stream);

/* ============================================================================================
 * (f5) Voxel R-CNN's RoI-grid pooling -- the hot path of NeighborVoxelSAModuleMSG
 *      (pcdet/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py:70-130) as query + fused gather / max-pool, with no
 *      [M][C][nsample] tensor anywhere.  Row numbers are GLOBAL rows of the stacked level (no per-frame offsets, no
 *      *_batch_cnt); float32 / int32; every call is capturable (no host read-back).
 *
 *   pcd_voxel2pinds_scatter / _clear   common_utils.py:244-252 (generate_voxel2pinds -> spconv's scatter_point_inds):
 *      indices [N][4] (b, z, y, x), map int32 [B][Z][Y][X]; scatter writes the row number, clear writes -1 at the same
 *      cells (a map filled with -1 ONCE stays reusable at the cost of N stores per step instead of a fill of the volume).
 *      num_rows: optional device int32[1], the real row count when N is a capacity; rows at or beyond it, and rows whose
 *      coordinates lie outside the map, are ignored by both.
 *
 *   pcd_voxel_pool_query   voxel_query_gpu.cu:10-88 (first nsample hits in (dz, dy, dx) scan order, probes clipped at the
 *      grid borders, new_coords [M][4] (b, z, y, x) anywhere -- also outside the grid; a frame index outside [0, B) is an
 *      empty ball) + voxel_query_utils.py:39-40,85-91 + the statistics voxel_pool_modules.py:104-109 feeds to BatchNorm2d.
 *      PCD_VOXEL_POOL_GROUP lanes share a query and probe consecutive cells of the scan order (ballot + prefix popcount
 *      keep the order; a group stops once it has nsample hits).  nsample <= PCD_VOXEL_POOL_MAX_NSAMPLE.
 *        idx [M][nsample]  global rows; slots behind the last hit repeat the first hit; an empty ball is all 0
 *        cnt [M]           distinct hits, capped at nsample (0: empty ball)
 *        partial           double [pcd_div_up(M, PCD_VOXEL_POOL_QUERIES_PER_WG)][9]: per-workgroup sums over the slots of
 *                          r = xyz[idx] - new_xyz (a repeated slot as often as it is repeated, an empty ball as r = 0):
 *                          x, y, z, xx, xy, xz, yy, yz, zz
 *        moments           double [9]: the partials joined in a fixed order (bit-reproducible)
 *
 *   pcd_voxel_pool_fwd     voxel_pool_modules.py:99-116 behind mlps_in, with mlps_pos (Conv2d(3, C) + BatchNorm2d) folded
 *      to the affine A [C][3], b [C]:  out[m][c] = max_s relu(fin[idx[m][s]][c] + (A_c . r[m][s] + b_c)) over the cnt[m]
 *      distinct slots, strict > in ascending s (what max_pool2d selects over the padded row); an empty ball gives
 *      relu(b_c).  arg [M][C] uint8: the winning slot.  1 <= C <= PCD_VOXEL_POOL_MAX_C; lanes run along c.
 *
 *   pcd_voxel_pool_bwd     its gradient through the saved winner: where out[m][c] > 0, d_fin[idx[m][arg]][c] += g[m][c]
 *      (non-empty balls only: voxel_pool_modules.py:99 zeroes the grouped features of an empty one in place; fp32 atomics
 *      into the caller-zeroed d_fin), dA_c += g r*, db_c += g -- these through per-workgroup partials
 *      float [pcd_div_up(M, PCD_VOXEL_POOL_BWD_QUERIES_PER_WG)][C][4] joined in a fixed order into dA [C][3], db [C].
 * ============================================================================================ */
#define PCD_VOXEL_POOL_GROUP 16
#define PCD_VOXEL_POOL_QUERIES_PER_WG 16
#define PCD_VOXEL_POOL_BWD_QUERIES_PER_WG 128
#define PCD_VOXEL_POOL_MAX_NSAMPLE 64
#define PCD_VOXEL_POOL_MAX_C 128
int pcd_voxel2pinds_scatter(const int32_t *indices, int N, const int32_t *num_rows, int32_t *map, int B, int Z, int Y, int X,
                            void *stream);
int pcd_voxel2pinds_clear(const int32_t *indices, int N, const int32_t *num_rows, int32_t *map, int B, int Z, int Y, int X,
                          void *stream);
int pcd_voxel_pool_query(int M, int N, int B, int Z, int Y, int X, int nsample, float radius, int z_range, int y_range,
                         int x_range, const float *new_xyz, const float *xyz, const int32_t *new_coords, const int32_t *map,
                         int32_t *idx, int32_t *cnt, double *partial, double *moments, void *stream);
int pcd_voxel_pool_fwd(int M, int N, int C, int nsample, const float *fin, const float *A, const float *b, const float *xyz,
                       const float *new_xyz, const int32_t *idx, const int32_t *cnt, float *out, unsigned char *arg,
                       void *stream);
int pcd_voxel_pool_bwd(int M, int N, int C, int nsample, const float *g, const float *out, const unsigned char *arg,
                       const float *xyz, const float *new_xyz, const int32_t *idx, const int32_t *cnt, float *d_fin_zeroed,
                       float *partial, float *dA, float *db, void *stream);

/* ============================================================================================
 * (f6) PV-RCNN++'s VectorPool aggregation -- the five natives of pcdet/ops/pointnet2/pointnet2_stack/src/vector_pool_gpu.cu
 *      behind VectorPoolAggregationModuleMSG (pointnet2_modules.py:160-470), without a neighbour list in global memory, an
 *      atomic counter, a read-back or a buffer sized by the data: every call is capturable.  Stacked batches: rows of frame b
 *      are the xyz_batch_cnt[b] rows behind those of frame b - 1; a query sees the rows of ITS frame only.  float32 / int32.
 *      M == 0 or N == 0: success without a launch (the caller's buffers hold the empty result).
 *
 *   pcd_vector_pool_three_nn   query_stacked_local_neighbor_idxs_kernel + query_three_nn_by_stacked_local_idxs_kernel
 *      (vector_pool_gpu.cu:19-205) and the resize loop of pointnet2_utils.py:331-347, fused.  A query's list is the first
 *      min(PCD_VECTOR_POOL_MAX_NEIGHBORS, nsample > 0 ? nsample : PCD_VECTOR_POOL_MAX_NEIGHBORS) rows of its frame within
 *      query_distance (the caller passes max_neighbour_distance * neighbor_distance_multiplier), in ascending row order;
 *      neighbor_type 1 is the ball test dx^2 + dy^2 + dz^2 > r^2, anything else the cube test |d| > r per axis, both on
 *      local = support - new in f32.  Per grid centre: the three smallest d = (cx-x)*(cx-x) + (cy-y)*(cy-y) + (cz-z)*(cz-z)
 *      (f32, left to right, no contraction), ties to the earlier list position -- ordered by (d, position), which is what the
 *      reference's sequential strict `<` yields.  One neighbour fills slots 2 and 3 with slot 1, two fill slot 3 with slot 1.
 *      One wave per query: a cooperative coalesced scan (ballot + prefix popcount keep the row order, the scan ends at the
 *      cap), the list as xyz + row in LDS, all G centres served from there.
 *        idx [M][G][3]      global rows; all three -1 when the list is empty
 *        dist2 [M][G][3]    squared distances; +inf when the list is empty (the reference's 1e40 stored as float)
 *        neighbor_cnt [M]   length of the list
 *
 *   pcd_vector_pool_interpolate_forward / _backward   pointnet2_modules.py:220-238 (weights, three_interpolate, the nine
 *      centre - neighbour coordinates, cat, new_features[empty_mask] = 0) as one pass:  out [M][G * (C + 9)], per cell the C
 *      interpolated channels, then centre - neighbour_j in slot order; w_j = (1 / (sqrt(d2_j) + 1e-8)) / max(sum, 1e-8); an
 *      empty cell (idx -1) is all zeros.  Backward: grad_support_features_zeroed [N][C] += w_j * grad_out[m][g][c] (fp32
 *      atomics: not bit-reproducible; lanes run along c); idx and dist2 carry no gradient (pointnet2_modules.py:212).
 *
 *   pcd_vector_pool_voxel_query_forward / _backward   vector_pool_kernel_stack / vector_pool_grad_kernel_stack
 *      (vector_pool_gpu.cu:243-458) for pooling_type 1 ("voxel_random_choice": the lowest row of each sub-voxel).  Cube / ball
 *      test as above with r = max_neighbour_distance; grid_size_a = max_neighbour_distance * 2 / num_grid_a; cell =
 *      floorf((local_a + r) / grid_size_a) per axis, combined x-major and THEN clamped to [0, G - 1]; a query stops once
 *      min(G, nsample > 0 ? nsample : G) cells are filled.  G <= PCD_VECTOR_POOL_MAX_GRIDS.  pooling_type 0 and
 *      num_c_in != num_c_out_each_grid are PCD_ERR_INVALID_ARG.  One wave per query, the frame's xyz staged through LDS.
 *        new_features [M][G * c], new_local_xyz [M][3 * G] (0 where a cell is empty), point_cnt_of_grid [M][G] (0 / 1),
 *        src_row [M][G] global row of the cell's point, -1: none (replaces the reference's grouped_idxs list)
 *      Backward: grad_support_features_zeroed[src_row[m][g]][:] += grad_new_features[m][g][:] (fp32 atomics).
 * ============================================================================================ */
#define PCD_VECTOR_POOL_MAX_NEIGHBORS 1000
#define PCD_VECTOR_POOL_MAX_GRIDS 64
#define PCD_VECTOR_POOL_NN_QUERIES_PER_WG 2
#define PCD_VECTOR_POOL_VQ_QUERIES_PER_WG 8
int pcd_vector_pool_three_nn(int B, int M, int N, int G, const float *support_xyz, const int32_t *xyz_batch_cnt,
                             const float *new_xyz, const float *new_xyz_grid_centers, const int32_t *new_xyz_batch_cnt,
                             float query_distance, int nsample, int neighbor_type, int32_t *idx, float *dist2,
                             int32_t *neighbor_cnt, void *stream);
int pcd_vector_pool_interpolate_forward(int M, int N, int G, int C, const int32_t *idx, const float *dist2,
                                        const float *support_xyz, const float *support_features,
                                        const float *new_xyz_grid_centers, float *out, void *stream);
int pcd_vector_pool_interpolate_backward(int M, int N, int G, int C, const int32_t *idx, const float *dist2,
                                         const float *grad_out, float *grad_support_features_zeroed, void *stream);
int pcd_vector_pool_voxel_query_forward(int B, int M, int N, int num_c_in, int num_c_out_each_grid, int num_grid_x,
                                        int num_grid_y, int num_grid_z, float max_neighbour_distance, int nsample,
                                        int neighbor_type, int pooling_type, const float *support_xyz,
                                        const int32_t *xyz_batch_cnt, const float *support_features, const float *new_xyz,
                                        const int32_t *new_xyz_batch_cnt, float *new_features, float *new_local_xyz,
                                        int32_t *point_cnt_of_grid, int32_t *src_row, void *stream);
int pcd_vector_pool_voxel_query_backward(int M, int N, int G, int C, const float *grad_new_features, const int32_t *src_row,
                                         float *grad_support_features_zeroed, void *stream);

/* ============================================================================================
 * (g) fp8 feature path (BASELINE config 5; build-side precision, the reference is fp32): OCP e4m3 activations and
 *     weights with per-tensor scales, fp32 accumulation (v_mfma_f32_16x16x32_fp8_fp8), for the INFERENCE form of
 *     post_act_block (spconv_backbone.py:8-27): conv + eval BatchNorm + ReLU + quantisation of the next layer's
 *     input in ONE kernel.
 *   pcd_fp8_pack_weight: weight [Cout][K][Cin] f32 -> e4m3(weight * scale_inv) in MFMA fragment order;
 *       cin_pad = power of two >= 16 (the fp8 row width of the input features).
 *   pcd_fp8_quantize: x [n][c] (PCD_F32 / PCD_BF16, row stride c_stride) -> e4m3(x * scale_inv) [n][cb], zero padded.
 *   pcd_fp8_dequantize: count e4m3 bytes -> f32 * scale.
 *   pcd_sparse_conv_gather_gemm_fp8: y[o][c] = q( relu?( (sum_k x8[nbr[k][o]] . w8[k][:, c]) * alpha[c] + beta[c] ) ),
 *       alpha = x_scale * w_scale * gamma / sqrt(var + eps), beta = bn_beta - mean * gamma / sqrt(var + eps) (or any
 *       per-channel affine); y_kind 0: f32, 1: bf16, 2: e4m3(value * out_scale_inv); y_stride in elements.
 * ============================================================================================ */
size_t pcd_fp8_packed_weight_bytes(int kvol, int cin_pad, int cout);
int pcd_fp8_pack_weight(const float *weight, int kvol, int cin, int cin_pad, int cout, float scale_inv, void *packed,
                        void *stream);
int pcd_fp8_quantize(const void *x, int dtype, int n, const int32_t *n_dev, int c, int c_stride, int cb,
                     float scale_inv, void *out, void *stream);
int pcd_fp8_dequantize(const void *x8, size_t count, float scale, float *out, void *stream);
int pcd_sparse_conv_gather_gemm_fp8(const void *x8, int n_rows_in, int cin_pad, const void *packed_w, const int32_t *nbr,
                                    int nbr_stride, int kvol, int flip_k, int n_rows_out,
                                    const int32_t *n_rows_out_dev, int c_out, const float *alpha, const float *beta,
                                    int relu, float out_scale_inv, void *y, int y_kind, int y_stride, void *stream);

/* ============================================================================================
 * (a6) PillarVFE pieces -- pcdet/models/backbones_3d/vfe/pillar_vfe.py:94-118 (decoration + padding mask) and the
 *      ReLU / max-over-points / concatenation half of PFNLayer (pillar_vfe.py:40-49).  float32.
 *   pcd_pillar_decorate: voxels [m][T][C] (zero padded), num_points [m], coords [m][4] (b, z, y, x) ->
 *       out [m][T][C' ], C' = (use_absolute_xyz ? C : C - 3) + 6 (+ 1 with_distance): point features, xyz - pillar mean
 *       (sum over the T slots / num_points, not clamped), xyz - pillar centre (coord * voxel_size + offset, offset =
 *       voxel_size / 2 + range_min), optional |xyz|; padding slots (t >= num_points) zeroed.
 *   pcd_pfn_relu_pool: x [m][T][C] (BatchNorm / Linear output) -> last_layer: out [m][C] = max_t relu(x);
 *       else out [m][T][2C] = [relu(x), broadcast max].  arg [m][C] = first maximal slot (for the backward).
 *   pcd_pfn_relu_pool_backward: grad_x [m][T][C] from grad_out of that layout.
 * ============================================================================================ */
int pcd_pillar_decorate(const float *voxels, const int32_t *num_points, const int32_t *coords, int m, int T, int C,
                        int use_absolute_xyz, int with_distance, const float *voxel_size_host,
                        const float *offset_host, float *out, void *stream);
int pcd_pfn_relu_pool(const float *x, int m, int T, int C, int last_layer, float *out, int32_t *arg, void *stream);
int pcd_pfn_relu_pool_backward(const float *grad_out, const float *x, const int32_t *arg, int m, int T, int C,
                               int last_layer, float *grad_x, void *stream);

/* ============================================================================================
 * (f3) Rotated BEV overlap / IoU and NMS -- replaces pcdet/ops/iou3d_nms (binder: src/iou3d_nms_api.cpp:12-16;
 *      kernels src/iou3d_nms_kernel.cu:236-413; host reduction src/iou3d_nms.cpp:60-188; Python callers
 *      iou3d_nms_utils.py:31-116).  Boxes are rows of 7 float32 (x, y, z, dx, dy, dz, heading).
 *   pcd_boxes_overlap_bev: out[a][b] = area of the BEV intersection (want_iou == 0; boxes_overlap_bev_gpu) or
 *                          the BEV IoU (want_iou != 0; boxes_iou_bev_gpu), out = [num_a][num_b] f32.
 *   pcd_nms_bev: greedy NMS over boxes ALREADY SORTED by descending score (as nms_gpu / nms_normal_gpu receive them):
 *                box i suppresses every later box whose IoU with it exceeds thresh (normal != 0: axis-aligned IoU of
 *                nms_normal_gpu).  keep = int64[num_boxes] receives the kept indices in ascending order,
 *                *num_keep_dev (device int32) their number; both stay on the device (the reference returns the
 *                count through a host loop over a mask it copies back).  workspace: pcd_nms_workspace_bytes(n).
 *   pcd_boxes_iou_bev_host: the reference's CPU variant boxes_iou_bev_cpu (iou3d_nms_utils.py:12-28 ->
 *                src/iou3d_cpu.cpp:232-252), called by COMAug's database sampler per frame inside DataLoader workers
 *                (datasets/augmentor/database_sampler_v2.py:600-601).  HOST pointers, synchronous, touches no GPU state
 *                (safe in forked workers); out_host = [num_a][num_b] f32 IoU.  Same float arithmetic as the reference
 *                file, bit for bit (fixture G13).
 * ============================================================================================ */
int pcd_boxes_iou_bev_host(const float *boxes_a_host, int num_a, const float *boxes_b_host, int num_b,
                           float *out_host);
int pcd_boxes_overlap_bev(const float *boxes_a, int num_a, const float *boxes_b, int num_b, float *out, int want_iou,
                          void *stream);
size_t pcd_nms_workspace_bytes(int num_boxes);
int pcd_nms_bev(const float *boxes, int num_boxes, float thresh, int normal, long long *keep, int32_t *num_keep_dev,
                void *workspace, size_t workspace_bytes, void *stream);

/* ============================================================================================
 * (f4) Static post-processing of CenterPoint-style heads -- replaces the eval half of the dense head:
 *      CenterHead.generate_predicted_boxes (center_head.py:266-317) -> decode_bbox_from_heatmap (centernet_utils.py:199-257;
 *      its two torch.topk calls at 199-214) -> class_agnostic_nms (model_nms_utils.py:15-27) -> nms_gpu / nms_normal_gpu
 *      (iou3d_nms_utils.py:85-116).  Every (frame, head) pair of a batch in a fixed number of launches, no host read-back,
 *      no allocation, grids from the shapes alone: capturable.
 *   Maps of head h: hm [B, C_h, H, W], center [B, 2, H, W], center_z [B, 1, H, W], dim [B, 3, H, W] (log sizes),
 *   rot [B, 2, H, W] (cos, sin), vel [B, 2, H, W] (NULL in every head or in none), f32 or bf16, arbitrary element strides
 *   {batch, channel, y, x}; arithmetic in fp32.
 *   Per frame and head:
 *     select   the top K = max_obj scores over the whole C x H x W map (score = fp32 sigmoid of the map value) among the
 *              pixels with score > score_thresh (when use_score_thresh).  ORDER: score descending, then flat index
 *              c*H*W + y*W + x ascending -- a total order, ties included (torch.topk leaves ties unordered).
 *     decode   x = ((x_px + center0) * feature_map_stride) * voxel_x + pc_x (y alike), z = center_z, dims = exp(dim),
 *              heading = atan2(sin, cos), [vx, vy] -- the torch code's fp32 operations in its order.
 *     mask     POST_CENTER_LIMIT_RANGE on x, y, z, inclusive on both ends; survivors keep the score order.
 *     nms      greedy class-agnostic NMS over the first min(count, nms_pre) survivors with the geometry of pcd_nms_bev
 *              (nms_normal: the axis-aligned IoU of nms_normal_gpu): same keep lists, bit for bit; then the first nms_post.
 *   Outputs (per frame, heads concatenated in head order, M = num_heads * nms_post rows, zeros behind count):
 *     boxes f32 [B, M, 7 | 9], scores f32 [B, M], labels int64 [B, M] (= head.label[c], i.e.
 *     class_id_mapping_each_head[h][c] + 1), count int32 [B].
 *   Refused (PCD_ERR_UNSUPPORTED; the workspace query returns 0): max_obj or nms_pre above PCD_POSTPROC_MAX_K (the
 *   per-problem sort runs in LDS), more than PCD_POSTPROC_MAX_HEADS heads or PCD_POSTPROC_MAX_CLASSES classes in a head,
 *   C * H * W or a map's element span beyond int32.  circle_nms has no entry (the reference asserts False).
 *   workspace: pcd_centerhead_postproc_workspace_bytes(heads, cfg) bytes, 256-byte aligned.
 * ============================================================================================ */
#define PCD_POSTPROC_MAX_HEADS 8
#define PCD_POSTPROC_MAX_CLASSES 16
#define PCD_POSTPROC_MAX_K 4096
typedef struct PcdPostprocHead {
    const void *map[6];                       /* hm, center, center_z, dim, rot, vel (or NULL) */
    long long strides[6][4];                  /* element strides {batch, channel, y, x} of each map */
    int dtype[6];                             /* PCD_F32 | PCD_BF16 */
    int num_class;                            /* C_h of hm */
    int label[PCD_POSTPROC_MAX_CLASSES];      /* output label of class c of this head */
} PcdPostprocHead;
typedef struct PcdPostprocConfig {
    int batch, num_heads, height, width;
    int max_obj;                              /* MAX_OBJ_PER_SAMPLE */
    int nms_pre, nms_post;                    /* NMS_PRE_MAXSIZE, NMS_POST_MAXSIZE */
    int nms_normal;                           /* 0: nms_gpu, 1: nms_normal_gpu */
    int use_score_thresh;
    float score_thresh, nms_thresh;
    float limit[6];                           /* POST_CENTER_LIMIT_RANGE */
    float feature_map_stride, voxel_x, voxel_y, pc_x, pc_y;
} PcdPostprocConfig;
size_t pcd_centerhead_postproc_workspace_bytes(const PcdPostprocHead *heads, const PcdPostprocConfig *cfg);
int pcd_centerhead_postproc(const PcdPostprocHead *heads, const PcdPostprocConfig *cfg, float *boxes, float *scores,
                            long long *labels, int32_t *count, void *workspace, size_t workspace_bytes, void *stream);

/* ============================================================================================
 * (f4a) Static post-processing of AnchorHeadSingle -- com_amd/csrc/anchor_postproc.hip.  Replaces the eval half of an
 *       anchor-head detector: generate_predicted_boxes (anchor_head_template.py:229-276) for every anchor, then the
 *       single-head class-agnostic branch of Detector3DTemplate.post_processing (detector3d_template.py:178-290) with
 *       class_agnostic_nms (model_nms_utils.py:6-25).  One selection problem per frame; a fixed number of launches (11), no
 *       host read-back, no allocation, grids from the shapes alone: capturable.  No [B, N, 7] and no [B, N, num_class]
 *       tensor exists on this path: only the selected anchors are decoded.
 *   Inputs: those of pcd_anchor_decode (f3) -- the three [B, H, W, C] maps through element strides {batch, channel, y, x},
 *   one dtype (PCD_F32 / PCD_BF16; dir_preds may be NULL), kinds, shifts, anchor n = (y * W + x) * A + kind.
 *   Per frame:
 *     score    score_c = fp32 sigmoid of the class logit (a bf16 logit widened first); the anchor's score is the maximum over
 *              its num_class scores, its label the LOWEST class index that attains the maximum, plus 1.
 *     pass     with use_score_thresh an anchor passes iff score >= score_thresh -- INCLUSIVE (model_nms_utils.py:9; the
 *              centre path (f4) is exclusive); without it every anchor passes.  A NaN score never passes: the one deliberate
 *              difference from torch.topk, which ranks NaN first.
 *     select   the first min(nms_pre, passing) anchors by score descending, then anchor index n ascending -- a total order
 *              (torch.topk leaves ties unordered; with distinct scores the two agree).
 *     decode   ResidualCoder.decode_torch + the direction-bin correction for the selected anchors only: the same device
 *              function as pcd_anchor_decode (anchorhead_common.h), hence the same bits.
 *     nms      greedy class-agnostic NMS over the selected boxes in that order, columns 0:7, with the geometry of
 *              pcd_nms_bev (nms_normal: the axis-aligned IoU of nms_normal_gpu); then the first nms_post survivors.
 *   Outputs: boxes f32 [B][nms_post][7], scores f32 [B][nms_post], labels int64 [B][nms_post], count int32 [B]; rows behind
 *   count are zero.
 *   Refused (PCD_ERR_UNSUPPORTED; the workspace query returns 0): nms_pre above PCD_POSTPROC_MAX_K (the per-frame sort runs
 *   in LDS), H * W * A beyond the int32 flat index, batch / height / width / nms_pre / nms_post below 1, more kinds than
 *   PCD_ANCHOR_MAX_KINDS or classes than PCD_ANCHOR_MAX_CLASSES, a batch above 65535 (the grid's y extent), with dir_preds
 *   a num_dir_bins outside 1 .. 8.  PCD_ERR_INVALID_ARG: a NULL config, map, table or output, nms_normal outside {0, 1} (the workspace query
 *   returns 0 for it too), a dtype other than PCD_F32 / PCD_BF16, a negative stride.
 *   workspace: pcd_anchor_postproc_workspace_bytes(cfg) bytes, 256-byte aligned.
 * ============================================================================================ */
typedef struct PcdAnchorPostprocConfig {
    int batch, height, width;
    int n_kinds;                              /* A: anchors per location */
    int n_classes;                            /* rows of `shifts` (anchor classes) */
    int num_class;                            /* class logits per anchor */
    int num_dir_bins;                         /* ignored when dir_preds is NULL */
    int nms_pre, nms_post;                    /* NMS_PRE_MAXSIZE, NMS_POST_MAXSIZE */
    int nms_normal;                           /* 0: nms_gpu, 1: nms_normal_gpu */
    int use_score_thresh;
    float score_thresh, nms_thresh;
    float dir_offset, dir_limit_offset;
} PcdAnchorPostprocConfig;
size_t pcd_anchor_postproc_workspace_bytes(const PcdAnchorPostprocConfig *cfg);
int pcd_anchor_postproc(const void *cls_preds, const void *box_preds, const void *dir_preds, int dtype,
                        const long long *strides_host, const float *kinds, const float *shifts,
                        const PcdAnchorPostprocConfig *cfg, float *boxes, float *scores, long long *labels, int32_t *count,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ============================================================================================
 * (f4b) Static post-processing of AnchorHeadMulti -- com_amd/csrc/anchor_multi_postproc.hip.  Replaces the eval half of a
 *       multi-head anchor detector: generate_predicted_boxes with use_multihead (anchor_head_template.py:229-276) for every
 *       anchor, then the MULTI_CLASSES_NMS branch of Detector3DTemplate.post_processing (detector3d_template.py:224-249)
 *       with multi_classes_nms (model_nms_utils.py:28-66).  P = B * num_class independent selection problems; a fixed
 *       number of launches (11), no host read-back, no allocation, grids from the shapes alone: capturable.  No [B, N, D]
 *       and no [B, N_h, C_h] tensor exists on this path: only the selected anchors are decoded.
 *   Inputs: those of pcd_anchor_multi_decode (f3m) -- the PcdAnchorMultiHead array (gradient pointers ignored), one dtype
 *   (PCD_F32 / PCD_BF16; dir maps in every head or in none), kinds [n_kinds][PCD_ANCHOR_MULTI_KIND_FLOATS], shifts.
 *   Problem p = b * num_class + c, c the GLOBAL class index; head h owns the classes [class0_h, class0_h + num_class_h),
 *   k = c - class0_h.  Its elements are the local anchors i in [0, N_h) of that head, N_h = n_kinds_h * H * W,
 *   i = (a * H + y) * W + x with a the head-local kind: the row order of batch_cls_preds[h] (f3m); the global anchor is
 *   n = kind0_h * H * W + i.
 *     score    fp32 sigmoid of the logit at channel a * num_class_h + k of head h's cls map, cell (y, x); a bf16 logit is
 *              widened first.
 *     pass     with use_score_thresh an element passes iff score >= score_thresh -- INCLUSIVE (model_nms_utils.py:42);
 *              without it every non-NaN score passes.  A NaN score never passes (torch.topk would rank it first).
 *     order    score descending, then i ascending -- a total order (torch.topk leaves ties unordered).
 *     select   the first min(nms_pre, passing) elements.
 *     decode   only the selected anchors, with the device function of pcd_anchor_multi_decode (anchorhead_common.h) under
 *              the kind-major geometry of n, hence the same bits; D = code - sincos columns (7 | 9).  An anchor selected
 *              under two classes of one head is decoded twice and appears twice, as in the reference.
 *     nms      greedy NMS per problem over the selected boxes in that order, columns 0:7, with the geometry of pcd_nms_bev
 *              (nms_normal: the axis-aligned IoU of nms_normal_gpu); then the first nms_post survivors.
 *   Outputs, per frame: the problems' survivors concatenated in global class order (head order, then class order inside
 *   the head; detector3d_template.py:233-249): boxes f32 [B][M][D], scores f32 [B][M], labels int64 [B][M] (= cfg.label[c],
 *   multihead_label_mapping[h][k]), count int32 [B]; M = num_class * nms_post; rows behind count are zero.
 *   Refused (PCD_ERR_UNSUPPORTED; the workspace query returns 0): nms_pre above PCD_POSTPROC_MAX_K (the per-problem sort
 *   runs in LDS), B * num_class above 65535 (a grid extent), H * W * n_kinds beyond the int32 flat index, batch / height /
 *   width / nms_pre / nms_post below 1, a code
 *   width other than 7 | 9 (+ sincos), more kinds than PCD_ANCHOR_MAX_KINDS or classes than PCD_ANCHOR_MAX_CLASSES, with
 *   direction maps a num_dir_bins outside 1 .. 8.  PCD_ERR_INVALID_ARG (the workspace query returns 0 too): a NULL config
 *   or head array, more than PCD_ANCHOR_MULTI_MAX_HEADS heads, heads that do not tile the kinds [0, n_kinds) and the
 *   classes [0, num_class) in order, a NULL cls / box map, direction maps given by some heads only, a negative stride,
 *   nms_normal outside {0, 1}; at the launch also a NULL table or output and a dtype other than PCD_F32 / PCD_BF16.
 *   workspace: pcd_anchor_multi_postproc_workspace_bytes(heads, n_heads, cfg) bytes, 256-byte aligned.
 * ============================================================================================ */
typedef struct PcdAnchorMultiPostprocConfig {
    int batch, height, width;
    int n_kinds;                              /* global kinds of all heads */
    int n_classes;                            /* rows of `shifts` (anchor classes) */
    int num_class;                            /* classes of all heads: problems per frame */
    int code, sincos;                         /* code size (sincos counted), encode_angle_by_sincos */
    int num_dir_bins;                         /* ignored without direction maps */
    int nms_pre, nms_post;                    /* NMS_PRE_MAXSIZE, NMS_POST_MAXSIZE */
    int nms_normal;                           /* 0: nms_gpu, 1: nms_normal_gpu */
    int use_score_thresh;
    float score_thresh, nms_thresh;
    float dir_offset, dir_limit_offset;
    int label[PCD_ANCHOR_MAX_CLASSES];        /* output label of global class c */
} PcdAnchorMultiPostprocConfig;
size_t pcd_anchor_multi_postproc_workspace_bytes(const PcdAnchorMultiHead *heads, int n_heads,
                                                 const PcdAnchorMultiPostprocConfig *cfg);
int pcd_anchor_multi_postproc(const PcdAnchorMultiHead *heads, int n_heads, int dtype, const float *kinds,
                              const float *shifts, const PcdAnchorMultiPostprocConfig *cfg, float *boxes, float *scores,
                              long long *labels, int32_t *count, void *workspace, size_t workspace_bytes, void *stream);

/* ============================================================================================
 * (f4c) Static proposal layer of a RoI head over an AnchorHeadSingle -- com_amd/csrc/roi_proposals.hip.  Replaces
 *       RoIHeadTemplate.proposal_layer (roi_head_template.py:45-102) over the output of generate_predicted_boxes
 *       (anchor_head_template.py:229-276), WITHOUT that output: no [B, N, 7] and no [B, N, num_class] tensor is written; only
 *       the <= NMS_PRE_MAXSIZE selected anchors of a frame are decoded.  One selection problem per frame; a fixed number of
 *       launches (11), no host read-back, no allocation, grids from the shapes alone: capturable.
 *   Inputs: those of pcd_anchor_decode (f3) / pcd_anchor_postproc (f4a); anchor n = (y * W + x) * A + kind.
 *   Per frame:
 *     score    the RAW LOGIT (roi_scores of the reference are logits: cls_preds_normalized is False); a bf16 logit is widened
 *              to f32 first.  The anchor's score is the maximum of its num_class logits, its label the LOWEST class index
 *              that attains the maximum, plus 1.
 *     pass     every anchor (the proposal layer has no score threshold).  An anchor whose maximum is NaN never takes part:
 *              the one deliberate difference from torch.topk, which ranks NaN first.
 *     order    score descending (-0.0 and +0.0 are one score), then n ascending -- a total order (torch.topk leaves ties
 *              unordered; with distinct scores the two agree).
 *     select   the first min(nms_pre, N) anchors; only those are decoded, with the device function of pcd_anchor_decode
 *              (anchorhead_common.h), hence its bits.
 *     nms      greedy class-agnostic NMS over the selected boxes in that order, columns 0:7 (nms_normal: the axis-aligned IoU
 *              of nms_normal_gpu); then the first nms_post survivors.
 *   Outputs: rois f32 [B][nms_post][7], roi_scores f32 [B][nms_post] (the logit's own bits), roi_labels int64 [B][nms_post],
 *   count int32 [B].  Rows behind count are what the reference leaves there: boxes 0, scores 0, LABELS 1 (it adds 1 to a
 *   zero-initialised tensor, roi_head_template.py:98).
 *   Refused (PCD_ERR_UNSUPPORTED; the workspace query returns 0): nms_pre above PCD_POSTPROC_MAX_K (the per-frame sort runs
 *   in LDS; this covers the 9000 of the TRAIN blocks, whose forward keeps the eager proposal_layer), H * W * A beyond the
 *   int32 flat index, batch / height / width / nms_pre / nms_post below 1, more kinds than PCD_ANCHOR_MAX_KINDS or classes
 *   than PCD_ANCHOR_MAX_CLASSES, a batch above 65535, with dir_preds a num_dir_bins outside 1 .. 8.  PCD_ERR_INVALID_ARG: a
 *   NULL config, map, table or output, nms_normal outside {0, 1} (the workspace query returns 0 for it too), a dtype other
 *   than PCD_F32 / PCD_BF16, a negative stride.
 *   workspace: pcd_anchor_proposals_workspace_bytes(cfg) bytes, 256-byte aligned.
 * ============================================================================================ */
typedef struct PcdAnchorProposalsConfig {
    int batch, height, width;
    int n_kinds;                              /* A: anchors per location */
    int n_classes;                            /* rows of `shifts` (anchor classes) */
    int num_class;                            /* class logits per anchor */
    int num_dir_bins;                         /* ignored when dir_preds is NULL */
    int nms_pre, nms_post;                    /* NMS_PRE_MAXSIZE, NMS_POST_MAXSIZE of ROI_HEAD.NMS_CONFIG.TEST */
    int nms_normal;                           /* 0: nms_gpu, 1: nms_normal_gpu */
    float nms_thresh;
    float dir_offset, dir_limit_offset;
} PcdAnchorProposalsConfig;
size_t pcd_anchor_proposals_workspace_bytes(const PcdAnchorProposalsConfig *cfg);
int pcd_anchor_proposals(const void *cls_preds, const void *box_preds, const void *dir_preds, int dtype,
                         const long long *strides_host, const float *kinds, const float *shifts,
                         const PcdAnchorProposalsConfig *cfg, float *rois, float *roi_scores, long long *roi_labels,
                         int32_t *count, void *workspace, size_t workspace_bytes, void *stream);

/* ============================================================================================
 * (f4d) Static post-processing of a RoI head -- com_amd/csrc/roi_proposals.hip.  Replaces the class-agnostic branch of
 *       Detector3DTemplate.post_processing (detector3d_template.py:178-290, with roi_labels) and
 *       SECONDNetIoU.post_processing (second_net_iou.py:75-177) with class_agnostic_nms (model_nms_utils.py:6-25): the
 *       per-frame loop, the boolean-mask selection and the read-back of the survivor count inside nms_gpu.  One selection
 *       problem per frame over its R RoI rows -- ALL of them, the zero rows behind the proposal count included, as in the
 *       reference; a fixed number of launches (12), no host read-back, no allocation, grids from the shapes alone.
 *   Inputs: batch_box_preds f32 [B][R][7], batch_cls_preds f32 [B][R] (one value per RoI: logits, probabilities with
 *   `normalized`), roi_scores f32 [B][R], roi_labels int64 [B][R] (NULL without has_class_labels), point_counts int32 [B][R]
 *   (pcd_points_in_boxes_count; PCD_ROIPP_SCORE_NUM_PTS only, else NULL); all contiguous.
 *   Score of row r, in fp32 with separate products and sums; iou = batch_cls_preds, cls = roi_scores, each through the fp32
 *   sigmoid unless `normalized`:
 *     PCD_ROIPP_SCORE_RCNN      iou (Detector3DTemplate.post_processing; cls is not read, no cls_scores / iou_scores)
 *     PCD_ROIPP_SCORE_IOU       iou                        PCD_ROIPP_SCORE_CLS   cls
 *     PCD_ROIPP_SCORE_WEIGHTED  weight_iou * iou + weight_cls * cls
 *     PCD_ROIPP_SCORE_BY_CLASS  label l = roi_labels (1 without has_class_labels) clamped to 0 .. num_class; D = the number of
 *                             distinct clamped labels in the frame; 1 <= l <= D: by_class_iou[l - 1] ? iou : cls, else 0 --
 *                             the reference's loop runs over range(number of distinct labels), a quirk kept
 *     PCD_ROIPP_SCORE_NUM_PTS   n = point count; alpha = n >= pts_iou_thresh ? 1 : n > pts_cls_thresh ? (n - 10) *
 *                             (1 / pts_span) : 0, pts_span = SCORE_THRESH.iou - SCORE_THRESH.cls; (1 - alpha) * cls +
 *                             alpha * iou -- the literal 10 is the reference's, a quirk kept
 *   pass     with use_score_thresh iff score >= score_thresh, INCLUSIVE (-0.0 equals +0.0); else every row.  A NaN never.
 *   order    score descending, then row index ascending; the first K = min(nms_pre, R) go through NMS on columns 0:7; the
 *            first nms_post survivors are written.
 *   Outputs (M = nms_post): boxes f32 [B][M][7], scores f32 [B][M] (the NMS score), labels int64 [B][M] (roi_labels of the
 *   row with has_class_labels, else 1), count int32 [B]; cls_scores / iou_scores f32 [B][M] (pred_cls_scores /
 *   pred_iou_scores of the reference's record; both NULL for PCD_ROIPP_SCORE_RCNN, both required otherwise).  Rows behind count
 *   are zero.
 *   Refused (PCD_ERR_UNSUPPORTED; the workspace query returns 0): R above PCD_POSTPROC_MAX_K, batch / rois / nms_pre /
 *   nms_post below 1, a batch above 65535, num_class outside 1 .. PCD_POSTPROC_MAX_CLASSES with PCD_ROIPP_SCORE_BY_CLASS, an
 *   unknown score_type, pts_iou_thresh below pts_cls_thresh.  PCD_ERR_INVALID_ARG: a NULL config, input or output (as
 *   required above), nms_normal outside {0, 1}.
 *   workspace: pcd_roi_postproc_workspace_bytes(cfg) bytes, 256-byte aligned.
 * ============================================================================================ */
#define PCD_ROIPP_SCORE_RCNN 0
#define PCD_ROIPP_SCORE_IOU 1
#define PCD_ROIPP_SCORE_CLS 2
#define PCD_ROIPP_SCORE_WEIGHTED 3
#define PCD_ROIPP_SCORE_BY_CLASS 4
#define PCD_ROIPP_SCORE_NUM_PTS 5
typedef struct PcdRoiPostprocConfig {
    int batch, rois;                          /* B, R */
    int score_type;                           /* PCD_ROIPP_SCORE_* */
    int normalized;                           /* cls_preds_normalized: no sigmoid */
    int has_class_labels;
    int num_class;                            /* len(class_names): entries of by_class_iou */
    int by_class_iou[PCD_POSTPROC_MAX_CLASSES];   /* SCORE_BY_CLASS of class c + 1: 1 'iou', 0 'cls' */
    int nms_pre, nms_post;                    /* NMS_PRE_MAXSIZE, NMS_POST_MAXSIZE */
    int nms_normal;                           /* 0: nms_gpu, 1: nms_normal_gpu */
    int use_score_thresh;
    float score_thresh, nms_thresh;
    float weight_iou, weight_cls;             /* SCORE_WEIGHTS */
    float pts_cls_thresh, pts_iou_thresh;     /* NMS_CONFIG.SCORE_THRESH.cls / .iou */
    float pts_span;                           /* .iou - .cls, subtracted by the caller */
} PcdRoiPostprocConfig;
size_t pcd_roi_postproc_workspace_bytes(const PcdRoiPostprocConfig *cfg);
int pcd_roi_postproc(const float *batch_box_preds, const float *batch_cls_preds, const float *roi_scores,
                     const long long *roi_labels, const int32_t *point_counts, const PcdRoiPostprocConfig *cfg, float *boxes,
                     float *scores, long long *labels, int32_t *count, float *cls_scores, float *iou_scores, void *workspace,
                     size_t workspace_bytes, void *stream);

/* ============================================================================================
 * Static-shape execution guard.  Buffers of a captured step are allocated at CAPACITIES (see "Device-side row
 * counts" above) and the kernels clamp to them, so a batch denser than the capacity would be truncated silently.
 * pcd_static_overflow_check enqueues a one-thread kernel that compares up to PCD_COUNT_CHECK_MAX device-side counts
 * with their capacities: flag[0] |= 1 (sticky) and flag[1] = max(flag[1], count - capacity) on overflow.  The
 * table is passed by value (host struct); flag is a device int32[2] the caller zeroes once and polls.
 * ============================================================================================ */
#define PCD_COUNT_CHECK_MAX 24
typedef struct PcdCountCheck {
    const int32_t *count[PCD_COUNT_CHECK_MAX];   /* device pointers to the counts */
    int32_t cap[PCD_COUNT_CHECK_MAX];            /* capacities                      */
} PcdCountCheck;
int pcd_static_overflow_check(const PcdCountCheck *table_host, int n, int32_t *flag, void *stream);

/* ============================================================================================
 * fp32-exact forms of the sparse convolution (features, weights, results in fp32; v_mfma_f32_16x16x4_f32).  The
 * reference runs fp32 end to end (spconv with fp32 weights behind spconv_backbone.py:12-15, pcdet/utils/spconv_utils.py:3-6);
 * these entry points exist for PARITY work -- reproducing a reference checkpoint's activations to fp32 accuracy and
 * checking a whole backbone end to end at 1e-3 without bf16 rounding noise -- not for speed.
 *   weight  [c_out][kvol][c_in] f32 (the parameter layout, no packing); for a data gradient pass the transposed
 *           weight [c_in][kvol][c_out] as `weight` and dy as `x` (flip_k as pcd_sparse_conv_gather_gemm)
 *   wgrad   dweight [c_out][kvol][c_in], pairs in canonical order; fixed summation order (deterministic)
 * c_out <= 128 per call. */
int pcd_sparse_conv_gather_gemm_f32(const float *x, int n_rows_in, int c_in, const float *weight, const float *bias,
                                    const int32_t *nbr, int nbr_stride, int kvol, int flip_k, int n_rows_out,
                                    const int32_t *n_rows_out_dev, int c_out, float *y, const float *addend,
                                    void *stream);
int pcd_sparse_conv_wgrad_f32(const float *x, int n_x_rows, int c_in, const float *dy, int n_dy_rows, int c_out,
                              const int32_t *pairs, const int32_t *pair_num, int kvol, int pmax, float *dweight,
                              void *stream);

/* ============================================================================================
 * (f1) Dense 3x3 convolution, stride 1, padding 1, over channels-last bf16 maps: the nn.Conv2d(k = 3, padding = 1) layers
 *      of BaseBEVBackbone / CenterHead (pcdet/models/backbones_2d/base_bev_backbone.py:30-112,
 *      dense_heads/center_head.py:11-46; MIOpen in the reference).  Implicit GEMM on MFMA, fp32 accumulate.
 *   weight  [cout][cin][3][3] f32 (torch OIHW); pcd_conv2d_pack_weight(mode 0) -> forward pack,
 *           (mode 1) -> data-gradient pack: run the SAME conv entry point on dy with cin / cout swapped
 *   x, y    [batch][height][width][channels] bf16 (torch.channels_last storage of an NCHW tensor)
 * cin % 32 == 0; packs pad the output channels with zeros to a multiple of 32 (run the conv with that padded count:
 * the data gradient contracts over it in steps of 32). */
size_t pcd_conv2d_packed_weight_bytes(int cin, int cout, int mode);
int pcd_conv2d_pack_weight(const float *weight, int cin, int cout, int mode, void *packed, void *stream);
/* all packs of a model in one launch: `table` = n device rows of 8 int64 {weight ptr, packed ptr, cin, cout,
 * cout padded to 32, mode, first workgroup, 16-byte pieces = packed bytes / 16}, total_blocks = sum of
 * ceil(pieces / 256) (rows ordered by first workgroup) */
int pcd_conv2d_pack_weights_batched(const void *table, int n, int total_blocks, void *stream);
/* The conv on CHANNEL BLOCKS of wider maps: x_cs / y_cs = channels per pixel of the buffers x / y point into
 * (>= cin / cout, multiples of 8; cin / cout for maps of their own): the five branches of a SeparateHead (center_head.py:11-46)
 * read their 64 channels of one 320-channel activation and their data gradients fill its gradient block by block -- no slice
 * copies, no adds.
 * bn_reduce (NULL = off; y_cs == cout required): the BatchNorm sums of the sparse path's PcdBnReduce taken in the epilogue: mode 1
 * on the forward launch for the BatchNorm behind the conv, mode 2 on the data-gradient launch for the BatchNorm whose output
 * was the conv's input (x / y = that BatchNorm's input / output as [pixels][cout] bf16).  partial_rows must equal
 * pcd_conv2d_3x3_tiles(batch, height, width); hand partial / mid to pcd_bn_forward_ld / pcd_bn_backward_ld as ext_partial. */
int pcd_conv2d_3x3_tiles(int batch, int height, int width);
int pcd_conv2d_3x3_nhwc_bn(const void *x, int x_cs, int batch, int height, int width, int cin, const void *packed_w,
                           int cout, const float *bias, void *y, int y_cs, const PcdBnReduce *bn_reduce, void *stream);
/* Weight gradient of that conv without pair lists: x [b][h][w][cin] (pixel stride x_cs channels), dy [b][h][w][cout]
 * contiguous, cin % 64 == 0, cout % 32 == 0 (zero-padded output channels allowed).  Writes
 * pcd_conv2d_wgrad_3x3_splits(..) slabs [cout][9][cin] f32 into `slabs`; finish with
 * pcd_sparse_conv_wgrad_reduce_batched (job.kvol = 9, job.splits = that count, job.pmax = 1, layout 1 for an
 * nn.Conv2d .grad, cout_write for padded convs).  0 splits / PCD_ERR_UNSUPPORTED: shape not covered (use the pair form). */
int pcd_conv2d_wgrad_3x3_splits(int batch, int height, int width, int cin, int cout);
int pcd_conv2d_wgrad_3x3_nhwc(const void *x, int x_cs, const void *dy, int batch, int height, int width, int cin, int cout,
                              void *slabs, size_t slab_bytes, void *stream);
/* The other three layers of BaseBEVBackbone (base_bev_backbone.py:36-75; MIOpen in the reference), forward and data
 * gradient, as per-parity-plane stencils on the same tiles.  pack modes (pcd_conv2d_pack_weight / _packed_weight_bytes /
 * the batched table take them too; cin / cout are the LAYER's channel counts, the weight is the torch parameter):
 *   2  Conv2d(cin, cout, 3, stride 2, padding 1) forward          x [b][hi][wi][cin]  -> y [b][ho][wo][cout], ho = (hi-1)/2+1
 *   3  its data gradient                                           dy [b][hi][wi][cout] -> dx [b][ho][wo][cin], hi = (ho-1)/2+1
 *   4  ConvTranspose2d(cin, cout, 2, stride 2) forward             x [b][hi][wi][cin]  -> y [b][2hi][2wi][cout]
 *   5  its data gradient                                           dy [b][hi][wi][cout] -> dx [b][hi/2][wi/2][cin]
 *   6 / 7  ConvTranspose2d(cin, cout, 1, stride 1) forward / data gradient (a 1 x 1 conv)
 * `cin` / `cout` of THIS call are the channel counts of x and y (i.e. swapped for the data gradients); both % 32 == 0. */
int pcd_conv2d_planes_nhwc(int pack_mode, const void *x, int batch, int hi, int wi, int cin, const void *packed_w,
                           int cout, const float *bias, void *y, int ho, int wo, void *stream);

/* (a3, dataset.py:252-259 + pcdet/models/__init__.py:23-34: collate + .cuda()) the host -> device hop INSIDE a captured step:
 * `host_ptr_table_dev` = n_slots device-side entries holding the addresses of PINNED host buffers (each >= bytes); the kernel
 * copies buffer (*counter_dev % n_slots) into dst over PCIe.  No copy engine, no second stream, no host call per step: a
 * replayed hipGraph pulls a different batch every time because the counter (pcd_counter_add, also a graph node) moves.
 * bytes % 16 == 0, dst 16-byte aligned; `workgroups` <= 0: 64. */
int pcd_pull_from_host(const void *host_ptr_table_dev, int n_slots, const int32_t *counter_dev, void *dst, size_t bytes,
                       int workgroups, void *stream);
int pcd_counter_add(int32_t *counter_dev, int delta, void *stream);

/* <a, b> of two bf16 vectors (fp32 products, fp64 partial sums) -> out[0], and y = bf16(a * scale_dev[0]): forward and
 * backward of a fixed linear functional of the BEV map -- bench.py's stand-in for the dense head's loss when only the
 * sparse hot path is timed (no reference counterpart).  n % 8 == 0, 16-byte aligned. */
size_t pcd_dot_bf16_workspace_bytes(void);
int pcd_dot_bf16(const void *a, const void *b, size_t n, float *out, void *workspace, size_t workspace_bytes, void *stream);
int pcd_scale_bf16(const void *a, const float *scale_dev, size_t n, void *y, void *stream);

/* Diagnostics: the device clock (100 MHz) into slot[0] at this point of the stream -- a time point inside a replayed
 * hipGraph, which events cannot give and a profiler perturbs (tools/exp_stamps.py).  No reference counterpart. */
int pcd_debug_stamp(uint64_t *slot, void *stream);
/* Diagnostics (tools/exp_cu_mask.py): a stream restricted to the compute units of `cu_mask` (hipExtStreamCreateWithCUMask;
 * the caller owns it), and a launch of `blocks` 1024-thread workgroups that each stay busy for `ticks` ticks of the 100 MHz
 * clock (xcc_seen, optional: bit x set when a workgroup ran on XCD x) -- the duration of 256 of them tells how many CUs the
 * launch was given, eagerly and as a replayed hipGraph node.  No reference counterpart. */
int pcd_debug_stream_create_cu_mask(const uint32_t *cu_mask, int words, void **stream_out);
int pcd_debug_spin(int blocks, unsigned long long ticks, uint32_t *xcc_seen, void *stream);
int pcd_debug_spin_shape(int blocks, int threads, int lds_bytes, int vgprs, unsigned long long ticks, void *stream);

/* ============================================================================================
 * (a8) SubMConv3d arithmetic over z-fastest rows: the WINDOW gather-GEMM (spconv_win.hip) -- forward and data gradient of
 *      spconv.SubMConv3d (spconv_backbone.py:12,38-45) for 3x3x3 kernels with c_in == c_out in {16, 32, 64, 128}, bf16 features.
 * Same operation as pcd_sparse_conv_gather_gemm on a SubM neighbour table: y[o] = bias + sum_k W_k x[nbr[k][o]] (+ addend)
 * with weights packed in mode 0; with weights packed in mode 1 the data gradient dx[i] = sum_k W_k^T dy[nbr[26 - k][i]]
 * (+ addend) -- the k flip of the rulebook view is folded into that pack, the launch has no flip argument.  Results agree
 * with the generic kernels up to the fp32 summation order.  It is FAST when the rows are numbered
 * PCD_ROWS_YXZ (the 27 neighbours of a tile of consecutive rows then lie in three short runs of rows that are staged in LDS
 * once per tile) and correct, only slow, for any other numbering.
 *   pcd_subm_window_tile_rows      rows per tile T of the (c_in, c_out) kernel; 0 = no window kernel for these widths
 *   pcd_subm_window_plan           per tile of T rows the three runs of neighbour rows + the tile's table of LDS operand slots
 *                                  (u16, 32 per row): plan = pcd_subm_window_plan_bytes(n, c_in, c_out) bytes, built once per rulebook
 *                                  (every conv of the indice_key, forward and backward, uses it)
 *   pcd_subm_window_pack_weight    weight [c_out][27][c_in] f32 -> the kernel's register-resident slices (mode 0 forward,
 *                                  1 data gradient: transposed, offsets reversed), pcd_subm_window_packed_weight_bytes bytes;
 *                                  _batched: table rows of 8 x i64
 *                                  {weight ptr, packed ptr, c_in, mode, first 256-thread block, 0, 0, 0}
 *   pcd_subm_window_partial_rows   rows of PcdBnReduce.partial a launch of these widths writes (one per persistent workgroup: 256, or 512
 *                                  for the 4-wave configurations of option "subm_window_half")
 * ============================================================================================ */
int pcd_subm_window_tile_rows(int c_in, int c_out);
int pcd_subm_window_partial_rows(int c_in, int c_out);
size_t pcd_subm_window_plan_bytes(int n_cap, int c_in, int c_out);
int pcd_subm_window_plan(const int32_t *nbr, int nbr_stride, int n_cap, const int32_t *n_dev, int c_in, int c_out,
                         void *plan, void *stream);
/* The same plan built STRAIGHT from the level's column map (rows numbered PCD_ROWS_YXZ; `indices` [n_cap][4], colmap as handed
 * out by pcd_voxelize_hard_yxz / pcd_rulebook_conv_cm_* / pcd_colmap_from_rows) -- what pcd_rulebook_subm_cm + pcd_subm_window_plan
 * produce together, in ONE pass and without the 27 x 4 B per row of neighbour table in between (spconv_backbone.py:38-45,199-218:
 * the SubM rulebooks of levels whose convs all run on window tiles).  nbr [27][n_cap] must be a buffer of that size:
 *   nbr_full != 0  the complete table is written too (bit-identical to pcd_rulebook_subm_cm's), for consumers that read it;
 *   nbr_full == 0  only the columns of tiles whose run exceeds the window (header.passes > 1) are written -- all that
 *                  pcd_sparse_conv_subm_window / _wgrad ever read of it; the rest of the buffer is left untouched. */
int pcd_subm_window_plan_cm(const int32_t *indices, int n_cap, const int32_t *n_dev, int batch, const int *shape_host,
                            const void *colmap, size_t colmap_bytes, int colmap_cap, int c_in, int c_out, int32_t *nbr,
                            int nbr_full, void *plan, void *stream);
size_t pcd_subm_window_packed_weight_bytes(int c_in, int c_out);
int pcd_subm_window_pack_weight(const float *weight, int c_in, int c_out, int mode, void *packed, void *stream);
int pcd_subm_window_pack_weights_batched(const void *table, int n, int total_blocks, void *stream);
/* Weight gradient over the same tiles: slab[s][c_out][27][c_in] f32 for s < pcd_subm_window_wgrad_splits() partial sums
 * (slab_bytes >= splits * 27 * c * c * 4), to be summed over s in order -- pcd_sparse_conv_wgrad_reduce_batched with
 * job.splits = that count does it (same job as pcd_sparse_conv_wgrad_os).  x, dy: bf16 [n_rows][c]; nbr / plan as above. */
int pcd_subm_window_wgrad_splits(int c);
int pcd_sparse_conv_subm_window_wgrad(const void *x, const void *dy, int n_rows, int c, const int32_t *nbr, int nbr_stride,
                                      const int32_t *n_rows_dev, const void *plan, void *slab, size_t slab_bytes,
                                      void *stream);
int pcd_sparse_conv_subm_window(const void *x, int n_rows, int c_in, const void *packed_w, const float *bias,
                                const int32_t *nbr, int nbr_stride, const int32_t *n_rows_dev,
                                const void *plan, int c_out, void *y, const void *addend,
                                const PcdBnReduce *bn_reduce, void *stream);
/* The same launch that ALSO writes y_f32 [n_rows][c_out]: the fp32 sums (bias and addend included) every bf16 output is
 * rounded from -- what the parity tests compare with the oracle at the 1e-3 bar of BASELINE.json (the bf16 rounding of y
 * alone is 2^-9 relative per element).  Not used by the training step. */
int pcd_sparse_conv_subm_window_f32(const void *x, int n_rows, int c_in, const void *packed_w, const float *bias,
                                    const int32_t *nbr, int nbr_stride, const int32_t *n_rows_dev, const void *plan,
                                    int c_out, void *y, float *y_f32, const void *addend, void *stream);

/* ============================================================================================
 * (f5) Point-in-box tests, RoI-aware pooling and the point heads' targets / losses / decoding -- replaces pcdet/ops/roiaware_pool3d
 *      (binder src/roiaware_pool3d.cpp:172-177; kernels src/roiaware_pool3d_kernel.cu; Python callers
 *      roiaware_pool3d_utils.py:9-107) and the host loops of pcdet/models/dense_heads/point_head_template.py.
 *      Boxes are rows of 7 float32 (x, y, z, dx, dy, dz, heading); the arithmetic of the test is the reference's, step by
 *      step (com_amd/csrc/roiaware_geom.h): z test first, cos / sin of -heading in float, the xy comparison in double.
 *   pcd_points_in_boxes_host: points_in_boxes_cpu (roiaware_pool3d.cpp:121-168), which box_utils.remove_points_in_boxes3d
 *                (box_utils.py:117-131) calls per frame inside the DataLoader workers of COMAug's database samplers
 *                (datasets/augmentor/database_sampler_v2.py:538, database_sampler.py:458).  HOST pointers, synchronous,
 *                touches no GPU state (safe in forked workers).  out_host = [num_boxes][num_pts] int32 0 / 1, every box
 *                tested on its own (no first-match rule); MARGIN 1e-2.
 *   pcd_points_in_boxes: points_in_boxes_gpu (roiaware_pool3d.cpp:98-118, roiaware_pool3d_kernel.cu:313-359).  boxes
 *                [batch][num_boxes][7], pts [batch][num_pts][3]; box_idx_of_pts [batch][num_pts] int32 receives the LOWEST
 *                index of a box that contains the point, -1 for a point in no box (every element written); MARGIN 1e-5.
 *   The point heads (com_amd/csrc/pointhead.hip) have ONE targets entry for PointHeadSimple, PointHeadBox and
 *   PointIntraPartOffsetHead.  (Retired: pcd_point_head_assign_targets, which was that entry with both label pointers NULL.)
 *   pcd_point_head_assign_targets_full: the targets of PointHeadSimple (point_head_simple.py:21-48), PointHeadBox
 *                (point_head_box.py:32-59) and PointIntraPartOffsetHead (point_intra_part_head.py:39-66) = enlarge_box3d
 *                (box_utils.py:187-200) + assign_stack_targets with set_ignore_flag (point_head_template.py:49-129), one launch
 *                for the whole stacked batch.  point_coords [num_points][4] rows of (bs_idx, x, y, z); gt_boxes
 *                [batch][n_boxes][8] (7 box floats + class, zero rows = padding); extra_x / _y / _z =
 *                TARGET_CONFIG.GT_EXTRA_WIDTH, added to dx, dy, dz of EVERY row (padding rows included, as the reference
 *                does).  point_cls_labels int64 [num_points]: the class of the first box that contains the point (1 when
 *                num_class == 1), -1 where foreground XOR inside-any-enlarged-box, 0 otherwise.  *num_pos (device int32) =
 *                number of labels > 0 (integer atomics: deterministic).  No read-back: capturable.
 *                point_box_labels f32 [num_points][8] (ret_box_labels; NULL: not wanted; 16-byte aligned) =
 *                PointResidualCoder.encode_torch (box_coder_utils.py:153-187) of the first containing box at the
 *                point: sizes clamped to 1e-5; mean_size (DEVICE f32 [num_mean][3], num_mean <= 16; NULL / 0 =
 *                use_mean_size False) is indexed by (int)column 7 - 1 of the GT row even when num_class == 1, CLAMPED to
 *                [0, num_mean - 1] (the reference asserts class <= num_mean and wraps class 0 to the last row).
 *                point_part_labels f32 [num_points][3] (ret_part_labels; NULL: not wanted) = the point in the box's frame /
 *                (dx, dy, dz) + 0.5 (:114-122; the clamped sizes when box labels are written too, as encode_torch clamps in
 *                place).  Both are zero on every point that is not foreground; every row is written.  Both NULL
 *                (PointHeadSimple): the kernel instantiation without the row bookkeeping runs.
 *   pcd_point_head_loss_forward / _backward: PointHeadSimple's get_cls_layer_loss (point_head_template.py:131-155):
 *                SigmoidFocalClassificationLoss(alpha 0.25, gamma 2; loss_utils.py:10-74) over logits [num_points][num_class]
 *                (f32 or bf16, rows row_stride elements apart) with weights ((label == 0) + (label > 0)) / max(*num_pos, 1),
 *                summed in a fixed order (bit-reproducible) and multiplied by cls_weight.  out = 4 device floats: out[0] =
 *                out[1] = the loss, out[2] = out[3] = 0 (the ordered finish pass of the anchor heads is reused).  backward:
 *                d_logits (layout and dtype of logits, every element written) = *grad_out (ONE device f32) x d loss /
 *                d logits.  The _full entries below compute the same bits with NULL branches; this pair stays because
 *                PointHeadSimple's replayed training step measured slower through them: this backward takes
 *                the one upstream gradient as autograd delivers it, the _full backward wants four floats assembled.
 *   pcd_point_head_full_loss_forward / _backward: get_cls_layer_loss + get_box_layer_loss + get_part_layer_loss
 *                (point_head_template.py:131-191) in one pass.  Predictions f32 or bf16 (one dtype), rows *_stride elements
 *                apart; box_preds / part_preds NULL = the head has no such branch (its labels, code_weights and gradient
 *                pointer may be NULL too).  cls: as pcd_point_head_loss_forward.
 *                box: WeightedSmoothL1Loss (loss_utils.py:338-399; nan targets ignored, code_weights = 8 device floats, beta
 *                1/9) with weights (label > 0) / max(*num_pos, 1), x box_weight.  part: F.binary_cross_entropy(sigmoid(p), t)
 *                over the 3 columns of the positives / (3 max(*num_pos, 1)) x part_weight, computed from the LOGIT as
 *                t softplus(-p) + (1 - t) softplus(p) with each log term capped at 100: the reference in EXACT arithmetic
 *                (its fp32 path rounds sigmoid(p) to 0 or 1 near |p| = 17 and then differs; this does not).  out = 4 device
 *                floats: cls + (box + part), cls, box, part (0 for an absent branch), summed in a fixed order
 *                (bit-reproducible; the ordered finish pass of the anchor heads).  Both branches NULL:
 *                out[0] = out[1] = the classification loss, out[2] = out[3] = 0.  backward:
 *                d_cls / d_box / d_part (layout and dtype of the predictions, every element written: zeros on ignored points
 *                for cls, on non-positive points and nan targets for box / part); grad_out = 4 device floats, the upstream
 *                gradients of out[0..4): a term is scaled by grad_out[0] + grad_out[1 + term].
 *   pcd_point_head_decode: generate_predicted_boxes (point_head_template.py:193-207) + PointResidualCoder.decode_torch
 *                (box_coder_utils.py:189-222).  box_encodings [num_points][8] (f32 / bf16, rows enc_stride apart), points f32
 *                rows (x, y, z) point_stride apart, boxes f32 [num_points][7].  The class that picks the mean size is
 *                pred_classes[n] (int64, 1-based) when given, else 1 + the FIRST maximum of the point's num_class logits
 *                (dtype of the encodings); its index is clamped into the table.  PCD_ERR_UNSUPPORTED: num_mean > 16, or
 *                num_class > num_mean without pred_classes.
 *   pcd_roiaware_pool3d_forward: roiaware_pool3d_gpu (roiaware_pool3d.cpp:29-66).  rois [num_rois][7], pts [num_pts][3],
 *                pts_feature [num_pts][channels] f32.  pts_idx_of_voxels int32 [num_rois][out_x][out_y][out_z]
 *                [max_pts_each_voxel]: slot 0 = count, then the ASCENDING indices of the voxel's points, cut after
 *                max_pts_each_voxel - 1 entries, unused slots 0 (every element written).  pool_method 0 = max: pooled_features
 *                f32 [num_rois][out_x][out_y][out_z][channels] and argmax int32 (same shape) = first strict maximum in list
 *                order, -1 / 0.0 for an empty voxel; 1 = avg: the sum in list order / count (argmax may be NULL).  No
 *                [num_rois][num_pts] mask is allocated.  PCD_ERR_UNSUPPORTED: an out size above 255, more than 8192 voxels
 *                per RoI, more than 65535 RoIs.
 *   pcd_roiaware_pool3d_backward: roiaware_pool3d_gpu_backward (:68-96).  grad_in f32 [num_pts][channels] is cleared and
 *                receives grad_out through argmax (max) or grad_out / max(count, 1) over the lists (avg).  Float atomics:
 *                the order of the additions into one point's row is not fixed.
 * ============================================================================================ */
int pcd_points_in_boxes_host(const float *boxes_host, int num_boxes, const float *pts_host, int num_pts, int *out_host);
int pcd_points_in_boxes(const float *boxes, const float *pts, int batch, int num_boxes, int num_pts, int *box_idx_of_pts,
                        void *stream);
int pcd_point_head_assign_targets_full(const float *point_coords, int num_points, const float *gt_boxes, int batch, int n_boxes,
                                       float extra_x, float extra_y, float extra_z, int num_class, const float *mean_size,
                                       int num_mean, long long *point_cls_labels, float *point_box_labels,
                                       float *point_part_labels, int *num_pos, void *stream);
size_t pcd_point_head_loss_workspace_bytes(int num_points);
int pcd_point_head_loss_forward(const void *logits, int dtype, long long row_stride, const long long *point_cls_labels,
                                const int *num_pos, int num_points, int num_class, float cls_weight, float *out,
                                void *workspace, size_t workspace_bytes, void *stream);
int pcd_point_head_loss_backward(const void *logits, void *d_logits, int dtype, long long row_stride,
                                 const long long *point_cls_labels, const int *num_pos, int num_points, int num_class,
                                 float cls_weight, const float *grad_out, void *stream);
size_t pcd_point_head_full_loss_workspace_bytes(int num_points);
int pcd_point_head_full_loss_forward(const void *cls_preds, long long cls_stride, const void *box_preds, long long box_stride,
                                     const void *part_preds, long long part_stride, int dtype,
                                     const long long *point_cls_labels, const float *point_box_labels,
                                     const float *point_part_labels, const int *num_pos, const float *code_weights,
                                     int num_points, int num_class, float cls_weight, float box_weight, float part_weight,
                                     float *out, void *workspace, size_t workspace_bytes, void *stream);
int pcd_point_head_full_loss_backward(const void *cls_preds, void *d_cls, long long cls_stride, const void *box_preds, void *d_box,
                                      long long box_stride, const void *part_preds, void *d_part, long long part_stride, int dtype,
                                      const long long *point_cls_labels, const float *point_box_labels,
                                      const float *point_part_labels, const int *num_pos, const float *code_weights,
                                      int num_points, int num_class, float cls_weight, float box_weight, float part_weight,
                                      const float *grad_out, void *stream);
int pcd_point_head_decode(const void *cls_preds, long long cls_stride, int num_class, const long long *pred_classes,
                          const void *box_encodings, long long enc_stride, int dtype, const float *points, long long point_stride,
                          const float *mean_size, int num_mean, int num_points, float *boxes, void *stream);
int pcd_roiaware_pool3d_forward(const float *rois, int num_rois, const float *pts, int num_pts, const float *pts_feature,
                                int channels, int out_x, int out_y, int out_z, int max_pts_each_voxel, int pool_method,
                                int *pts_idx_of_voxels, int *argmax, float *pooled_features, void *stream);
int pcd_roiaware_pool3d_backward(const int *pts_idx_of_voxels, const int *argmax, const float *grad_out, int num_rois, int out_x,
                                 int out_y, int out_z, int channels, int max_pts_each_voxel, int pool_method, int num_pts,
                                 float *grad_in, void *stream);

/* ============================================================================================
 * (f6) The second half of PVRCNNHead: proposal targets, the RoI loss, box decoding -- replaces the host loops of
 *      pcdet/models/roi_heads/target_assigner/proposal_target_layer.py and pcdet/models/roi_heads/roi_head_template.py.
 *      code_size is 7: rois [batch][num_rois][7], gt_boxes [batch][num_gt][8] (7 box floats + class), all f32 and dense.
 *      No entry point reads anything back, allocates or has a data-dependent shape: all are capturable.
 *   pcd_roi_head_max_overlaps: proposal_target_layer.py:89-105 (the trailing-zero-row scan, boxes_iou3d_gpu + torch.max)
 *                and :195-228 (get_max_iou_with_same_class).  Per frame the valid GT rows are those up to the last row whose
 *                eight values do not sum to 0 (none: ONE all-zero box).  max_overlaps f32 / gt_assignment int32
 *                [batch][num_rois]: the largest rotated 3-D IoU (iou3d_nms_utils.py:49-82, clamp 1e-6; the BEV overlap is
 *                the code of pcd_boxes_overlap_bev) and the LOWEST index of a GT row that attains it.  same_class != 0: only
 *                GT rows with (long)class == roi_labels[.] compete; a RoI without one gets 0.0 and index 0.
 *   pcd_roi_head_sample_targets: proposal_target_layer.py:13-62, :107-192 (subsample_rois, sample_bg_inds, gather, labels)
 *                + roi_head_template.py:104-134 (canonical transformation).  One workgroup per frame.  Lists in ascending RoI
 *                order: fg (iou >= min(reg_fg, cls_fg)), hard bg (cls_bg_lo <= iou < reg_fg), easy bg (iou < cls_bg_lo).
 *                uniforms f32 [batch][num_rois + rois_per_image] in [0, 1): the first num_rois are one key per RoI -- the
 *                k foreground RoIs with the smallest keys fill the first k slots in ascending key order (ties by index); the
 *                last rois_per_image are one per slot j -- a slot drawn with replacement takes
 *                list[min(int(u_j * n), n - 1)] (f32 product).  hard_bg_table int32 [rois_per_image + 1] (device):
 *                entry bg = int(bg * HARD_BG_RATIO), computed on the host.  Slots: fg, hard bg, easy bg.  Outputs for the
 *                slots: sampled_inds int32 [batch][R], rois [..][7], roi_scores, roi_labels int64, gt_iou_of_rois,
 *                gt_of_rois_src [..][8], gt_of_rois [..][8] (centre and heading relative to the RoI, rotated by -ry, heading
 *                folded into [-pi/2, pi/2]), reg_valid_mask int64 (iou > reg_fg), rcnn_cls_labels: f32 soft labels
 *                (PCD_ROI_SCORE_ROI_IOU) or int64 with -1 (PCD_ROI_SCORE_CLS).  given_inds != 0: sampled_inds is an INPUT
 *                (clamped to the RoIs) and only the gather runs (uniforms / hard_bg_table may be NULL).  A frame with
 *                neither fg nor bg (NaN IoUs; the reference raises) takes RoI 0 for every slot and adds 1 to *status
 *                (device int32, cleared by the caller).  PCD_ERR_UNSUPPORTED: num_rois or rois_per_image above 2048.
 *   pcd_roi_head_loss_forward / _backward: roi_head_template.py:136-231.  rcnn_cls [num_rows] (elements cls_stride
 *                apart), rcnn_reg [num_rows][7] (rows reg_stride apart), f32 or bf16; rcnn_cls_labels f32, reg_valid_mask
 *                int64, rois / gt_of_rois / gt_of_rois_src as written by pcd_roi_head_sample_targets.  BinaryCrossEntropy on
 *                the f32 sigmoid with both logs clamped at -100, rows with label >= 0, / max(count, 1); smooth-L1 (beta 1/9,
 *                code_weights_host: 7 HOST floats, nan target -> prediction) on ResidualCoder targets against the RoI with
 *                centre and heading zeroed (sizes clamped at 1e-5) over rows with reg_valid_mask > 0, / max(fg_sum, 1);
 *                corner_loss != 0: + the corner regulariser (decode, rotate by the RoI heading, + centre; min over the GT and
 *                its pi-flipped copy of the eight corner distances, smooth-L1 beta 1, mean), 0 when fg_sum == 0.  out = 5
 *                device floats: rcnn_loss, rcnn_loss_cls, rcnn_loss_reg (corner included), rcnn_loss_corner, fg_sum.  aux =
 *                4 device floats the backward reads: max(valid rows, 1), max(fg_sum, 1), the smooth-L1 term alone (what the
 *                reference logs as rcnn_loss_reg), 0.  One workgroup, fixed summation order, no atomics: bit-reproducible.
 *                backward: d_rcnn_cls / d_rcnn_reg (layout and dtype of the inputs, every element written) = *grad_out x the
 *                derivative; the derivative through a zero corner distance is 0.
 *   pcd_roi_head_decode: generate_predicted_boxes (roi_head_template.py:233-261): ResidualCoder.decode_torch against the RoI
 *                with its centre zeroed, rotation by the RoI heading, + centre.  box_preds [num_rows][7] f32 or bf16 (rows
 *                row_stride apart), rois [num_rows][7]; batch_box_preds f32 [num_rows][7].
 * ============================================================================================ */
#define PCD_ROI_SCORE_ROI_IOU 0
#define PCD_ROI_SCORE_CLS 1
struct PcdRoiSampler {
    int batch, num_rois, num_gt, rois_per_image;
    int fg_rois_per_image;      /* int(np.round(FG_RATIO * ROI_PER_IMAGE)) */
    int score_type;             /* PCD_ROI_SCORE_* */
    int given_inds;
    float reg_fg_thresh, cls_fg_thresh, cls_bg_thresh, cls_bg_thresh_lo;
    float cls_span;             /* CLS_FG_THRESH - CLS_BG_THRESH, the difference taken in double */
};
int pcd_roi_head_max_overlaps(const float *rois, const long long *roi_labels, const float *gt_boxes, int batch, int num_rois,
                              int num_gt, int same_class, float *max_overlaps, int *gt_assignment, void *stream);
int pcd_roi_head_sample_targets(const struct PcdRoiSampler *cfg, const float *rois, const float *roi_scores,
                                const long long *roi_labels, const float *gt_boxes, const float *max_overlaps,
                                const int *gt_assignment, const float *uniforms, const int *hard_bg_table, int *sampled_inds,
                                float *out_rois, float *out_roi_scores, long long *out_roi_labels, float *out_gt_iou_of_rois,
                                float *out_gt_of_rois_src, float *out_gt_of_rois, long long *out_reg_valid_mask,
                                void *out_rcnn_cls_labels, int *status, void *stream);
int pcd_roi_head_loss_forward(const void *rcnn_cls, int cls_dtype, long long cls_stride, const void *rcnn_reg, int reg_dtype,
                              long long reg_stride, const float *rcnn_cls_labels, const long long *reg_valid_mask,
                              const float *rois, const float *gt_of_rois, const float *gt_of_rois_src, int num_rows,
                              const float *code_weights_host, float cls_weight, float reg_weight, float corner_weight,
                              int corner_loss, float *out, float *aux, void *stream);
int pcd_roi_head_loss_backward(const void *rcnn_cls, int cls_dtype, long long cls_stride, const void *rcnn_reg, int reg_dtype,
                               long long reg_stride, const float *rcnn_cls_labels, const long long *reg_valid_mask,
                               const float *rois, const float *gt_of_rois, const float *gt_of_rois_src, int num_rows,
                               const float *code_weights_host, float cls_weight, float reg_weight, float corner_weight,
                               int corner_loss, const float *aux, const float *grad_out, void *d_rcnn_cls, void *d_rcnn_reg,
                               void *stream);
int pcd_roi_head_decode(const float *rois, const void *box_preds, int dtype, long long row_stride, int num_rows,
                        float *batch_box_preds, void *stream);

/* ============================================================================================
 * (f7) SECONDHead, the IoU-rectification stage of SECOND-IoU -- replaces the per-frame loop of
 *      pcdet/models/roi_heads/second_head.py:63-120, its loss (:163-188) and the host round trip of
 *      pcdet/models/detectors/second_net_iou.py:133-138.  No entry point reads anything back, allocates or has a
 *      data-dependent shape: all are capturable.
 *   pcd_bev_roi_grid_pool: roi_grid_pool (second_head.py:87-113: theta, affine_grid and grid_sample with align_corners=True,
 *                bilinear, zero padding, over a stride-0 expand of the frame's map) for the whole batch in one launch.
 *                features [batch][channels][height][width] f32 or bf16 with element strides {b, c, y, x} (NCHW and
 *                channels-last are both native; any positive strides are read correctly); rois f32 [batch][num_rois] rows
 *                of >= 7 floats, roi_stride elements apart; cell_x / cell_y = voxel size x DOWNSAMPLE_RATIO.  With
 *                cx = (x - min_x) / cell_x, hx = dx / 2 / cell_x (y alike), u_j = -1 + 2 j / (G - 1), v_i alike, sample
 *                (i, j) lies at ix = cx + hx (cos a u_j - sin a v_i), iy = cy + hy (sin a u_j + cos a v_i) pixels
 *                (sincosf, fp32); its value is the sum over the four neighbours of (floor ix, floor iy) inside the map,
 *                weighted (1 - |ix - X|)(1 - |iy - Y|).  A neighbour outside the map is not read.  pooled
 *                [batch * num_rois][channels][G][G] dense, in the feature dtype (c-major: shared_fc_layer[0].weight
 *                indexes c * G * G + p).  Both layouts give the same bits.  PCD_ERR_UNSUPPORTED: G < 2,
 *                G > PCD_SECOND_POOL_MAX_G, height or width < 2, more than 65535 RoIs.  There is no backward: the
 *                reference pools from detached features and RoIs (second_head.py:74-75).
 *   pcd_second_head_iou_loss_forward / _backward: get_box_iou_layer_loss (second_head.py:163-188).  logits [n] f32 or bf16,
 *                `stride` elements apart; labels f32 [n]; kind = PCD_SECOND_IOU_LOSS_BCE (binary_cross_entropy_with_logits
 *                in its stable form), _L2 (mse_loss) or _SMOOTH_L1 (loss_utils.py:363-370, beta 1 / 9) over the rows with
 *                label >= 0.  out = 2 device floats: sum / max(valid, 1) x weight, and the valid count.  One workgroup,
 *                fp64 partial sums joined by a fixed tree: bit-reproducible.  backward: d_logits (layout and dtype of
 *                logits, every element written) = *grad_out (device f32) x the derivative; `out` is the forward's.
 *                ('focalbce' calls loss_utils.sigmoid_focal_cls_loss, which the reference does not define: no kind.)
 *   pcd_points_in_boxes_count: points_in_boxes_cpu(points of frame b, boxes[b]).sum(dim=1) for every frame
 *                (second_net_iou.py:133-138).  points [num_points][4] rows of (bs_idx, x, y, z), in any order; boxes
 *                [batch][num_boxes][7]; counts int32 [batch][num_boxes], zeroed by the call.  A point counts for every box
 *                that contains it; the test is that of pcd_points_in_boxes_host (MARGIN 1e-2).  Integer atomics only
 *                (LDS, then one global add per workgroup and box): the result does not depend on the order.
 * ============================================================================================ */
#define PCD_SECOND_POOL_MAX_G 16
#define PCD_SECOND_IOU_LOSS_BCE 0
#define PCD_SECOND_IOU_LOSS_L2 1
#define PCD_SECOND_IOU_LOSS_SMOOTH_L1 2
int pcd_bev_roi_grid_pool(const void *features, int dtype, int batch, int channels, int height, int width,
                          long long stride_b, long long stride_c, long long stride_y, long long stride_x, const float *rois,
                          int num_rois, long long roi_stride, int grid_size, float min_x, float min_y, float cell_x,
                          float cell_y, void *pooled, void *stream);
int pcd_second_head_iou_loss_forward(const void *logits, int dtype, long long stride, const float *labels, int n, int kind,
                                     float weight, float *out, void *stream);
int pcd_second_head_iou_loss_backward(const void *logits, int dtype, long long stride, const float *labels, int n, int kind,
                                      float weight, const float *out, const float *grad_out, void *d_logits, void *stream);
int pcd_points_in_boxes_count(const float *points, int num_points, const float *boxes, int batch, int num_boxes, int *counts,
                              void *stream);

/* ============================================================================================
 * (f8) PartA2FCHead's RoI-aware pooling for the whole stacked batch, straight to sparse rows -- replaces roiaware_pool
 *      (pcdet/models/roi_heads/partA2_head.py:104-151: a host loop over frames, RoIAwarePool3d 'avg' over the part features
 *      and 'max' over the RPN features per frame) and the nonzero() / gather of forward (:184-195).  The list contract is
 *      that of pcd_roiaware_pool3d_forward: a voxel's points in ascending index within the frame, cut after
 *      max_pts_each_voxel - 1 entries; avg = sum in list order / number listed, max = first strict maximum.  No
 *      [RoIs][voxels][max_pts] list, no [RoIs][points] mask and no dense pooled tensor is allocated; a fixed number of
 *      launches serves the batch.  rois f32 [batch][num_rois][7]; point_coords f32 [num_points][4] rows of (bs_idx, x, y, z),
 *      in any order; point_part rows of 3 f32, part_stride elements apart (point_part_offset, or point_coords + 1 with
 *      stride 4 for DISABLE_PART); point_scores f32 [num_points].  The part features of a point are (part[0..3), score) with
 *      the first three zeroed where score < score_thresh (strict, :125).
 *   pcd_parta2_pool_plan: the counting pass.  voxels int32 [batch * num_rois][pool_size^3] receives the number listed per
 *                voxel, | 1 << 30 where the voxel is a ROW: the fp32 sum ((p0 + p1) + p2) + p3 of its four pooled part
 *                features is non-zero (:185).  roi_counts int32 [2][batch * num_rois] (rows, listed points) and offsets
 *                int32 [2][batch * num_rois + 1] (their exclusive scans, totals last) are scratch for the forward.  state =
 *                PCD_PARTA2_STATE_WORDS device int32: [0] the row count clamped to max_rows (the n_dev of the sparse
 *                tensors), [1] the row count, [2] the number of list entries, [3] 1 on the fake path.  Fewer than three rows
 *                (:186-191): the fake path, one row per RoI at cell (0, 0, 0) with whatever was pooled there, row count =
 *                batch * num_rois.  max_rows / max_listed = the capacities the forward will be given (INT_MAX: the caller
 *                reads state back and allocates); *status (device int32, may be NULL, cleared by the caller) |= 1 when the
 *                rows, 2 when the list entries do not fit.
 *   pcd_parta2_pool_forward: coords int32 [max_rows][4] rows of (roi, x, y, z) in the ascending order nonzero() gives,
 *                part_rows f32 [max_rows][4], rpn_rows f32 [max_rows][channels], and the record the backward reads:
 *                row_entries int32 [max_rows][2] (start, count) into entries int32 [max_listed] (point indices in list
 *                order), argmax int32 [max_rows][channels] (-1: empty).  Rows behind state[0] are cleared (argmax -1); rows
 *                and entries that do not fit are dropped.  coords and part_rows 16-byte aligned.
 *   pcd_parta2_pool_backward: grad_part f32 [num_points][3] (NULL: not wanted) and grad_features f32
 *                [num_points][channels], every element written: grad_part_rows[.][0..3) / count over the entries whose score
 *                is not below the threshold (none to the score), grad_rpn_rows through argmax.  Float atomics: the order of
 *                the additions into one point's row is not fixed.
 *   PCD_ERR_UNSUPPORTED: pool_size above PCD_PARTA2_MAX_POOL, more than 65535 RoIs, or RoIs x min(num_points, pool_size^3 x
 *                (max_pts_each_voxel - 1)), the bound of the list entries (int32 offsets), not below 2^31.  No entry point reads
 *                anything back.
 * ============================================================================================ */
#define PCD_PARTA2_MAX_POOL 14
#define PCD_PARTA2_STATE_WORDS 4
int pcd_parta2_pool_plan(const float *rois, int batch, int num_rois, const float *point_coords, int num_points,
                         const float *point_part, long long part_stride, const float *point_scores, float score_thresh,
                         int pool_size, int max_pts_each_voxel, int max_rows, int max_listed, int *voxels, int *roi_counts,
                         int *offsets, int *state, int *status, void *stream);
int pcd_parta2_pool_forward(const float *rois, int batch, int num_rois, const float *point_coords, int num_points,
                            const float *point_part, long long part_stride, const float *point_scores, float score_thresh,
                            const float *point_features, int channels, int pool_size, int max_pts_each_voxel, int max_rows,
                            int max_listed, const int *voxels, const int *offsets, const int *state, int *coords,
                            float *part_rows, float *rpn_rows, int *row_entries, int *entries, int *argmax, void *stream);
int pcd_parta2_pool_backward(const float *grad_part_rows, const float *grad_rpn_rows, int channels, int num_points, int max_rows,
                             const int *state, const int *row_entries, const int *entries, const int *argmax,
                             const float *point_scores, float score_thresh, float *grad_part, float *grad_features,
                             void *stream);

/* ---- UNetV2's UR block and point outputs (unet.hip; pcdet/models/backbones_3d/spconv_unet.py:135-160,206-211) ----------
 * Matrices are row-major [n][c] of PCD_F32 / PCD_BF16 with c * element size a multiple of 16 that divides 4096, 16-byte
 * aligned; n is the capacity and *n_dev (optional) the row count on the device: rows behind it are neither read nor written
 * (but for the padding rows of pcd_unet_point_outputs).  fp32 arithmetic, one rounding to the storage type.
 *   pcd_unet_merge_cat       cat [n][2c]: cat[r] = (bottom[r], trans[r]), both [n][c]; bit copies.
 *   pcd_unet_bn_pairadd      out[r][j] = relu(x[r][j] * scale[j] + shift[j]) + (cat[r][2j] + cat[r][2j+1]), x and out [n][c],
 *                            cat [n][2c]; scale = gamma * invstd, shift = beta - mean * gamma * invstd.  Training form: mid =
 *                            the rows pcd_bn_stats_mid (or a conv launch: PcdBnReduce.mid) left; mean / invstd are finished
 *                            from them as pcd_bn_forward_ld does, written to save_mean / save_invstd, and the running
 *                            statistics (optional) are updated.  mid == NULL: running_mean / running_var are the statistics.
 *                            The backward pass is pcd_bn_backward_ld's (relu, y == NULL: the mask from x).
 *   pcd_unet_merge_backward  d_bottom[r][q] = d_cat[r][q] + dy[r][q >> 1], d_trans[r][q] = d_cat[r][c + q] + dy[r][(c + q) >> 1];
 *                            d_cat [n][2c], the others [n][c].
 *   pcd_unet_point_outputs   indices int32 [n][4] = (b, z, y, x) -> coords f32 [n][4] = (b, cx, cy, cz), c = (idx + 0.5) * v + c0
 *                            with the product and the sum rounded separately.  With n_dev, rows [*n_dev, n) of coords become
 *                            (-1, 0, 0, 0) and those rows of features (optional, feature_row_bytes each, a multiple of 16)
 *                            become zero.  coords == NULL (needs n_dev and features): only that, indices is not read. */
/* dst [cout][kvol][cin] f32 = the transpose of src [cin][kvol][cout] f32 (distinct buffers): the weight gradient of an inverse
 * conv taken by the strided conv's class weight-gradient kernel with the two operands swapped, into parameter layout. */
int pcd_unet_transpose_wgrad(const float *src, int cin, int kvol, int cout, float *dst, void *stream);
int pcd_unet_merge_cat(const void *bottom, const void *trans, int dtype, int n, int c, const int32_t *n_dev, void *cat,
                       void *stream);
int pcd_unet_bn_pairadd(const void *x, const void *cat, int dtype, int n, int c, const float *gamma, const float *beta,
                        float eps, float momentum, const double *mid, float *running_mean, float *running_var,
                        float *save_mean, float *save_invstd, const int32_t *n_dev, void *out, void *stream);
int pcd_unet_merge_backward(const void *d_cat, const void *dy, int dtype, int n, int c, const int32_t *n_dev, void *d_bottom,
                            void *d_trans, void *stream);
int pcd_unet_point_outputs(const int32_t *indices, int n, const int32_t *n_dev, float vx, float vy, float vz, float x0,
                           float y0, float z0, float *coords, void *features, int feature_row_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PCD_OPS_H_ */
