// AnchorHeadMulti on the device (gfx950): target assignment, fused loss, box decoding for per-head prediction maps.
// C ABI: include/pcd_ops.h (f3m).
//
//   pcd_anchor_multi_assign_targets  axis_aligned_target_assigner.py:36-210 with use_multihead (:68-69, :92-101) +
//                                    box_coder_utils.py:13-43 in full (any code size, sin/cos heading)
//   pcd_anchor_multi_loss_forward /  pcdet/models/dense_heads/anchor_head_multi.py:245-373 with loss_utils.py:10-74
//   pcd_anchor_multi_loss_backward   (sigmoid focal), :338-441 (weighted smooth-L1 | weighted L1), :444-469 (cross entropy)
//   pcd_anchor_multi_decode          anchor_head_template.py:229-276 with use_multihead + box_coder_utils.py:45-77
//
// The kernels are the anchor heads' one core (anchorhead_common.h) under its KIND-MAJOR layout: anchor n =
// (g * H + y) * W + x, g the global kind; head h owns a contiguous run of kinds; every thread resolves its own head from
// a kind -> head table in LDS, beside a copy of the head descriptors; one launch covers all heads.  The assignment, the
// loss and the coder are therefore the single head's, bit for bit (tests/test_gpu_anchor_multi.py holds one head against
// AnchorHeadSingle).  This file holds the entry points: argument checks, the head table, the config, the launches.
// What this head sets in the core's configs: box rows of 8 or 10 floats, 7 to 10 codes, smooth-L1 | L1, the
// sin-difference on the heading only with direction maps, pos / neg classification weights.  Compiled with
// -ffp-contract=off like anchorhead.hip, for the same reason.
#include "anchorhead_common.h"

namespace {

// the config of both loss entries (has_dir as the first head shows it: am_fill_heads, which runs after the checks here,
// holds every head to it)
bool am_loss_cfg(AncLossCfg &c, const PcdAnchorMultiHead *heads, int dtype, int batch, int height, int width, int n_kinds,
                 int num_class, int code, int reg_l1, int num_dir_bins, float pos_w, float neg_w, float cls_weight,
                 float loc_weight, float dir_weight, float dir_offset) {
    const bool has_dir = heads && heads[0].map[2] != nullptr;
    return loss_cfg(c, dtype, batch, height, width, n_kinds, num_class, code, reg_l1, num_dir_bins, has_dir, has_dir, pos_w, neg_w,
                    cls_weight, loc_weight, has_dir ? dir_weight : 0.f, dir_offset);
}

}  // namespace

extern "C" size_t pcd_anchor_multi_assign_workspace_bytes(int batch, int n_boxes) {
    return assign_workspace_bytes(batch, n_boxes);
}

extern "C" int pcd_anchor_multi_assign_targets(const float *gt_boxes, int batch, int n_boxes, int code_gt, int sincos,
                                               const float *kinds, int n_kinds, const float *classes, int n_classes,
                                               const float *shifts, int height, int width, int *box_cls_labels,
                                               float *box_reg_targets, float *reg_weights, int *gt_index, int *num_pos,
                                               void *workspace, size_t workspace_bytes, void *stream) {
    PCD_ENTER();
    if (!kinds || !classes || !shifts || !box_cls_labels || !box_reg_targets || !reg_weights || !num_pos || n_boxes < 0 ||
        (n_boxes > 0 && !gt_boxes))
        return PCD_ERR_INVALID_ARG;
    if (!am_code_ok(code_gt + sincos, sincos) || !shape_ok(batch, height, width, n_kinds, code_gt + sincos) || n_classes < 1 ||
        n_classes > ANC_MAX_CLASSES || (long long)batch * n_boxes >= (1ll << 27))
        return PCD_ERR_UNSUPPORTED;
    WsCarver ws(workspace, workspace_bytes);
    const size_t bm = (size_t)batch * (size_t)(n_boxes > 0 ? n_boxes : 1);
    float *pb = ws.take<float>(bm * ANC_BOXF);
    u32 *box_max = ws.take<u32>(bm);
    if (!ws.ok) return PCD_ERR_WORKSPACE;
    launch_assign<KindMajor>(assign_cfg(height, width, n_kinds, n_classes, n_boxes, code_gt, sincos), batch, gt_boxes, pb, box_max,
                             kinds, classes, shifts, box_cls_labels, box_reg_targets, reg_weights, gt_index, num_pos,
                             (hipStream_t)stream);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" size_t pcd_anchor_multi_loss_workspace_bytes(int batch, int height, int width, int n_kinds) {
    return loss_workspace_bytes(batch, height, width, n_kinds);
}

extern "C" int pcd_anchor_multi_loss_forward(const PcdAnchorMultiHead *heads, int n_heads, int dtype, const int *box_cls_labels,
                                             const float *box_reg_targets, const int *num_pos, int batch, int height, int width,
                                             int n_kinds, int num_class, int code, int reg_l1, int num_dir_bins,
                                             const float *kinds, const float *code_weights, float pos_cls_weight,
                                             float neg_cls_weight, float cls_weight, float loc_weight, float dir_weight,
                                             float dir_offset, float *out, void *workspace, size_t workspace_bytes,
                                             void *stream) {
    PCD_ENTER();
    KindMajor hd;
    AncLossCfg c;
    bool has_dir = false;
    if (!box_cls_labels || !box_reg_targets || !num_pos || !kinds || !code_weights || !out) return PCD_ERR_INVALID_ARG;
    if (!am_loss_cfg(c, heads, dtype, batch, height, width, n_kinds, num_class, code, reg_l1, num_dir_bins, pos_cls_weight,
                     neg_cls_weight, cls_weight, loc_weight, dir_weight, dir_offset))
        return PCD_ERR_UNSUPPORTED;
    if (!am_fill_heads(hd, heads, n_heads, n_kinds, num_class, false, has_dir)) return PCD_ERR_INVALID_ARG;
    WsCarver ws(workspace, workspace_bytes);
    dim3 grid(pcd_div_up(height * width * n_kinds, 256), batch);
    float *partials = ws.take<float>((size_t)grid.x * grid.y * 3);
    if (!ws.ok) return PCD_ERR_WORKSPACE;
    launch_loss_forward(hd, c, grid, box_cls_labels, box_reg_targets, num_pos, kinds, code_weights, partials, out, AncNoCur(),
                        (hipStream_t)stream);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_anchor_multi_loss_backward(const PcdAnchorMultiHead *heads, int n_heads, int dtype, const int *box_cls_labels,
                                              const float *box_reg_targets, const int *num_pos, int batch, int height,
                                              int width, int n_kinds, int num_class, int code, int reg_l1, int num_dir_bins,
                                              const float *kinds, const float *code_weights, float pos_cls_weight,
                                              float neg_cls_weight, float cls_weight, float loc_weight, float dir_weight,
                                              float dir_offset, const float *grad_out, void *stream) {
    PCD_ENTER();
    KindMajor hd;
    AncLossCfg c;
    bool has_dir = false;
    if (!box_cls_labels || !box_reg_targets || !num_pos || !kinds || !code_weights || !grad_out) return PCD_ERR_INVALID_ARG;
    if (!am_loss_cfg(c, heads, dtype, batch, height, width, n_kinds, num_class, code, reg_l1, num_dir_bins, pos_cls_weight,
                     neg_cls_weight, cls_weight, loc_weight, dir_weight, dir_offset))
        return PCD_ERR_UNSUPPORTED;
    if (!am_fill_heads(hd, heads, n_heads, n_kinds, num_class, true, has_dir)) return PCD_ERR_INVALID_ARG;
    dim3 grid(pcd_div_up(height * width * n_kinds, 256), batch);
    anc_loss_kernel<true, KindMajor, AncNoCur><<<grid, 256, 0, (hipStream_t)stream>>>(
        hd, c, box_cls_labels, box_reg_targets, num_pos, kinds, code_weights, grad_out, nullptr, AncNoCur());
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_anchor_multi_decode(const PcdAnchorMultiHead *heads, int n_heads, int dtype, int batch, int height, int width,
                                       int n_kinds, int n_classes, int code, int sincos, int num_dir_bins, const float *kinds,
                                       const float *shifts, float dir_offset, float dir_limit_offset, float *batch_box_preds,
                                       float *const *cls_out_host, void *stream) {
    PCD_ENTER();
    KindMajor hd;
    bool has_dir = false;
    if (!kinds || !shifts || !batch_box_preds || !cls_out_host || (dtype != PCD_F32 && dtype != PCD_BF16))
        return PCD_ERR_INVALID_ARG;
    if (!am_code_ok(code, sincos) || !shape_ok(batch, height, width, n_kinds, code) || n_classes < 1 ||
        n_classes > ANC_MAX_CLASSES)
        return PCD_ERR_UNSUPPORTED;
    if (!heads || n_heads < 1 || n_heads > ANC_MAX_HEADS) return PCD_ERR_INVALID_ARG;
    int num_class = 0;
    for (int h = 0; h < n_heads; ++h) num_class += heads[h].num_class;
    if (num_class > PCD_ANCHOR_MAX_CLASSES) return PCD_ERR_UNSUPPORTED;
    if (!am_fill_heads(hd, heads, n_heads, n_kinds, num_class, false, has_dir)) return PCD_ERR_INVALID_ARG;
    if (!bins_ok(has_dir, num_dir_bins)) return PCD_ERR_UNSUPPORTED;
    for (int h = 0; h < n_heads; ++h) {
        if (!cls_out_host[h]) return PCD_ERR_INVALID_ARG;
        if ((long long)batch * height * width * heads[h].n_kinds * heads[h].num_class >= (1ll << 31)) return PCD_ERR_UNSUPPORTED;
        hd.cls_out[h] = cls_out_host[h];
    }
    const AncDecodeCfg c = decode_cfg(dtype, height, width, n_kinds, n_classes, code, sincos, num_dir_bins, has_dir, dir_offset,
                                      dir_limit_offset);
    dim3 grid(pcd_div_up(height * width * n_kinds, 256), batch);
    anc_decode_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(hd, c, kinds, shifts, batch_box_preds);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
