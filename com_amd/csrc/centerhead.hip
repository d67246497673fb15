// CenterHead target assignment on the GPU (SURVEY.md 8f #2 "host-side step overheads"): the reference builds the
// training targets with a Python loop over ground-truth boxes, on CPU tensors, with one `.item()` and one numpy ->
// torch -> device copy per box (pcdet/models/dense_heads/center_head.py:104-161, :163-225 and
// pcdet/models/model_utils/centernet_utils.py:46-107) -- a per-step host stall that grows with the number of
// objects.  Here: one wave per batch element compacts the boxes of the head's classes (ballot prefix keeps their
// order), computes centre / Gaussian radius / regression targets with the reference's float32 formulas, and a second
// kernel draws every Gaussian with an order-free atomic max (heat-map values are >= 0, so their float bits order like
// integers) -- deterministic, no host round trip.
#include "centerhead_common.h"

namespace {

__global__ __launch_bounds__(64) void assign_rows_kernel(const float *__restrict__ gt, int n, AssignGeom G,
                                                         float *__restrict__ ret_boxes, long long *__restrict__ inds,
                                                         long long *__restrict__ mask, int4 *__restrict__ draw) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float *rows = gt + (size_t)b * n * G.code;
    int count = 0;
    for (int base = 0; base < n && count < G.num_max; base += 64) {
        const int r = base + lane;
        const int local = assign_class(rows, r, n, G);
        int total;
        const int k = count + wave_rank(local > 0, total);
        count += total;
        if (local <= 0 || k >= G.num_max) continue;
        const float *q = rows + (size_t)r * G.code;
        const AssignRow a = assign_row(q, G);
        const size_t at = (size_t)b * G.num_max + k;
        int4 d = make_int4(-1, 0, 0, 0);
        if (a.valid) {
            inds[at] = (long long)a.iy * G.W + a.ix;
            mask[at] = 1;
            encode_box(q, a, G.code, ret_boxes + at * G.code);
            d = make_int4(local - 1, a.ix, a.iy, a.radius);
        }
        draw[at] = d;
    }
}

}  // namespace

extern "C" size_t pcd_centerhead_assign_workspace_bytes(int batch, int num_max_objs) {
    if (batch <= 0 || num_max_objs <= 0) return 0;
    return ws_piece((size_t)batch * num_max_objs, sizeof(int4));
}

extern "C" int pcd_centerhead_assign_targets(const float *gt_boxes, int batch, int n_boxes, int code_size,
                                             const int *class_map_host, int n_class_map, int head_classes, int fm_w, int fm_h,
                                             int feature_map_stride, const float *voxel_size_xy_host,
                                             const float *range_xy_host, int num_max_objs, float gaussian_overlap,
                                             int min_radius, float *heatmap, float *ret_boxes, long long *inds,
                                             long long *mask, void *workspace, size_t workspace_bytes, void *stream) {
    PCD_ENTER();
    if (batch <= 0 || n_boxes < 0 || code_size < 8 || !class_map_host || n_class_map <= 0 || n_class_map > 16 ||
        head_classes <= 0 || fm_w <= 0 || fm_h <= 0 || feature_map_stride <= 0 || num_max_objs <= 0 || !voxel_size_xy_host ||
        !range_xy_host)
        return PCD_ERR_INVALID_ARG;
    if (!heatmap || !ret_boxes || !inds || !mask) return PCD_ERR_INVALID_ARG;
    if (n_boxes > 0 && !gt_boxes) return PCD_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < pcd_centerhead_assign_workspace_bytes(batch, num_max_objs)) return PCD_ERR_WORKSPACE;
    const AssignGeom G = assign_geom(range_xy_host, voxel_size_xy_host, feature_map_stride, fm_w, fm_h, num_max_objs,
                                     min_radius, code_size, head_classes, gaussian_overlap, class_map_host, n_class_map);
    hipStream_t st = (hipStream_t)stream;
    int4 *draw = (int4 *)workspace;
    pcd_fill(heatmap, 0, (size_t)batch * head_classes * fm_h * fm_w * sizeof(float), st);
    pcd_fill(ret_boxes, 0, (size_t)batch * num_max_objs * code_size * sizeof(float), st);
    pcd_fill(inds, 0, (size_t)batch * num_max_objs * sizeof(long long), st);
    pcd_fill(mask, 0, (size_t)batch * num_max_objs * sizeof(long long), st);
    pcd_fill(draw, 0xFF, (size_t)batch * num_max_objs * sizeof(int4), st);
    assign_rows_kernel<<<batch, 64, 0, st>>>(gt_boxes, n_boxes, G, ret_boxes, inds, mask, draw);
    draw_gaussian_kernel<<<(unsigned)((size_t)batch * num_max_objs), 64, 0, st>>>(draw, G, heatmap);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

// =============================================================================================================
// CenterHead.get_loss of one head in four launches (center_head.py:226-262; loss_utils.py:611-643 neg_loss_cornernet,
// :1317-1390 RegLossCenterNet / _transpose_and_gather_feat) instead of ~100 elementwise / reduction launches:
//   forward : partial sums per workgroup (focal terms, number of positives, confidence; L1 sums per code dimension,
//             number of objects) -> one finalising workgroup -> out[] (loss, hm_loss, loc_loss, confidence, ...)
//   backward: d loss / d hm logits (dense) and zeros for the regression maps, then the <= B x M object positions
//             scattered into the regression gradients (objects sharing a pixel are summed by the first of them, in
//             object order: no atomics, deterministic).
// Same arithmetic as the reference in fp32: p = clamp(sigmoid(x), 1e-4, 1 - 1e-4), the clamp's gradient is 1 inside
// [1e-4, 1 - 1e-4] (inclusive) and 0 outside, |.|'s gradient is sign(.) with sign(0) = 0.  Sums are taken in a fixed
// order of this kernel's own (per-thread strided -> wave -> workgroup -> 256 partials in order).
// Predictions are addressed through element strides (NCHW or channels-last, bf16 or f32).
namespace {

// partial[blk][0..3] = pos_loss, neg_loss, num_pos, sum of p at the positives; [4 .. 4 + dims) = L1 sums; [4 + dims] =
// number of objects (the regression part by block 0 only)
__global__ __launch_bounds__(256) void chl_forward_kernel(ChlMap hm, const float *__restrict__ gt, int B, int C, int H,
                                                          int W, ChlRegs regs, const long long *__restrict__ ind,
                                                          const long long *__restrict__ mask,
                                                          const float *__restrict__ target, int M,
                                                          double *__restrict__ partial, int pstride) {
    __shared__ double lds[4];
    const long long total = (long long)B * C * H * W;
    double pos = 0.0, neg = 0.0, npos = 0.0, conf = 0.0;
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < (unsigned)total; e += CHL_BLOCKS * 256u) {
        const float g = gt[e];
        const float p = chl_pred(hm, chl_at_linear(hm, e, C, H, W));
        if (g == 1.0f) {
            pos += (double)focal_pos(p);
            npos += 1.0;
            conf += (double)p;
        } else if (g < 1.0f) {
            neg += (double)focal_neg(p, g);
        }
    }
    double *row = partial + (size_t)blockIdx.x * pstride;
    const double s0 = chl_block_sum(pos, lds), s1 = chl_block_sum(neg, lds), s2 = chl_block_sum(npos, lds),
                 s3 = chl_block_sum(conf, lds);
    if (threadIdx.x == 0) {
        row[0] = s0; row[1] = s1; row[2] = s2; row[3] = s3;
    }
    chl_reg_partials(regs, B, W, ind, mask, target, M, row + 4, lds);
}

// out[0] = loss, [1] = hm_loss, [2] = loc_loss, [3] = confidence, [4] = num_pos, [5] = num_obj, [6 .. 6 + dims) = L1 per dim
__global__ __launch_bounds__(256) void chl_finalize_kernel(const double *__restrict__ partial, int pstride, int dims,
                                                           const float *__restrict__ code_weights, float cls_weight,
                                                           float loc_weight, float *__restrict__ out) {
    __shared__ double tot[4 + CHL_MAX_DIM + 1];
    if ((int)threadIdx.x < 4 + dims + 1) {
        double s = 0.0;
        for (int b = 0; b < CHL_BLOCKS; ++b) s += partial[(size_t)b * pstride + threadIdx.x];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float pos = (float)tot[0], neg = (float)tot[1], npos = (float)tot[2], conf = (float)tot[3];
    const float hm_loss = -(pos + neg) / fmaxf(npos, 1.0f) * cls_weight;
    const float nobj = (float)tot[4 + dims];
    float loc = 0.0f;
    for (int d = 0; d < dims; ++d) {
        const float l = (float)tot[4 + d] / fmaxf(nobj, 1.0f);
        out[6 + d] = l;
        loc += l * code_weights[d];
    }
    loc *= loc_weight;
    out[0] = hm_loss + loc;
    out[1] = hm_loss;
    out[2] = loc;
    out[3] = conf / npos;          // (nan without positives, as in the reference)
    out[4] = npos;
    out[5] = nobj;
}

// d loss / d hm logits for every element; the regression gradients are zeroed here and filled by chl_scatter_kernel
__global__ __launch_bounds__(256) void chl_backward_kernel(ChlMap hm, const float *__restrict__ gt, int B, int C, int H,
                                                           int W, ChlRegs regs, const float *__restrict__ out,
                                                           const float *__restrict__ grad_out, float cls_weight) {
    const long long total = (long long)B * C * H * W;
    const float scale = -cls_weight / fmaxf(out[4], 1.0f) * grad_out[0];
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < (unsigned)total; e += gridDim.x * 256u) {
        const float g = gt[e];
        const long long off = chl_at_linear(hm, e, C, H, W);
        const float s = sigmoid_f32(chl_load(hm, off));
        const bool inside = s >= 1e-4f && s <= 1.0f - 1e-4f;
        const float p = focal_clamp(s);
        float dp = 0.0f;
        if (g == 1.0f) dp = focal_pos_grad(p);
        else if (g < 1.0f) dp = focal_neg_grad(p, g);
        chl_store_grad(hm, off, inside ? scale * dp * (s * (1.0f - s)) : 0.0f);
    }
    chl_zero_reg_grads(regs, B, H, W);
}

}  // namespace

extern "C" size_t pcd_centerhead_loss_workspace_bytes(int code_dims) {
    if (code_dims < 0 || code_dims > CHL_MAX_DIM) return 0;
    return (size_t)CHL_BLOCKS * (4 + CHL_MAX_DIM + 2) * sizeof(double);
}

extern "C" int pcd_centerhead_loss_forward(const void *hm, int hm_dtype, const long long *hm_strides_host,
                                           const float *gt_heatmap, int batch, int num_classes, int height, int width,
                                           const void *const *reg_ptrs_host, const int *reg_channels_host, int reg_dtype,
                                           const long long *reg_strides_host, int n_reg, const long long *inds,
                                           const long long *masks, const float *target_boxes, int num_max_objs,
                                           const float *code_weights, float cls_weight, float loc_weight, float *out,
                                           void *workspace, size_t workspace_bytes, void *stream) {
    PCD_ENTER();
    if (num_max_objs < 0 || !workspace || (num_max_objs > 0 && n_reg > 0 && (!inds || !masks || !target_boxes || !code_weights)))
        return PCD_ERR_INVALID_ARG;
    ChlMap H_;
    ChlRegs R;
    int rc = chl_pack(batch, num_classes, height, width, gt_heatmap, out, hm, nullptr, hm_dtype, hm_strides_host,
                      reg_ptrs_host, nullptr, reg_channels_host, reg_dtype, reg_strides_host, n_reg, &H_, &R);
    if (rc != PCD_OK) return rc;
    if (workspace_bytes < pcd_centerhead_loss_workspace_bytes(R.dims)) return PCD_ERR_WORKSPACE;
    rc = chl_check_limits(batch, num_classes, height, width, num_max_objs, 4294967295.0);   // (M: the backward pass could not follow)
    if (rc != PCD_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int pstride = 4 + CHL_MAX_DIM + 2;
    chl_forward_kernel<<<CHL_BLOCKS, 256, 0, st>>>(H_, gt_heatmap, batch, num_classes, height, width, R, inds, masks,
                                                   target_boxes, num_max_objs, (double *)workspace, pstride);
    chl_finalize_kernel<<<1, 256, 0, st>>>((const double *)workspace, pstride, R.dims, code_weights, cls_weight,
                                           loc_weight, out);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_centerhead_loss_backward(const void *hm, void *d_hm, int hm_dtype, const long long *hm_strides_host,
                                            const float *gt_heatmap, int batch, int num_classes, int height, int width,
                                            const void *const *reg_ptrs_host, void *const *reg_grads_host,
                                            const int *reg_channels_host, int reg_dtype,
                                            const long long *reg_strides_host, int n_reg, const long long *inds,
                                            const long long *masks, const float *target_boxes, int num_max_objs,
                                            const float *code_weights, float cls_weight, float loc_weight,
                                            const float *out, const float *grad_out, void *stream) {
    PCD_ENTER();
    if (num_max_objs < 0 || !grad_out || !d_hm ||
        (num_max_objs > 0 && n_reg > 0 && (!inds || !masks || !target_boxes || !code_weights)))
        return PCD_ERR_INVALID_ARG;
    ChlMap H_;
    ChlRegs R;
    int rc = chl_pack(batch, num_classes, height, width, gt_heatmap, out, hm, d_hm, hm_dtype, hm_strides_host,
                      reg_ptrs_host, reg_grads_host, reg_channels_host, reg_dtype, reg_strides_host, n_reg, &H_, &R);
    if (rc != PCD_OK) return rc;
    rc = chl_check_limits(batch, num_classes, height, width, num_max_objs, 4294967295.0);
    if (rc != PCD_OK) return rc;
    if ((double)height * width >= 2147483647.0) return PCD_ERR_UNSUPPORTED;   // (chl_scatter_kernel keeps pixels as int)
    hipStream_t st = (hipStream_t)stream;
    chl_backward_kernel<<<1024, 256, 0, st>>>(H_, gt_heatmap, batch, num_classes, height, width, R, out, grad_out,
                                              cls_weight);
    if (n_reg > 0 && num_max_objs > 0)
        chl_scatter_kernel<long long><<<batch, 256, 0, st>>>(R, width, inds, masks, target_boxes, num_max_objs,
                                                             code_weights, out, grad_out, loc_weight);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
