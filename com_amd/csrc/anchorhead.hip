// AnchorHeadSingle on the device (gfx950): target assignment, fused loss, box decoding.  C ABI: include/pcd_ops.h (f3).
//
//   pcd_anchor_assign_targets   pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py:36-210 for the
//                               whole batch and all anchor classes (+ pcdet/utils/box_utils.py:291-340 nearest-BEV IoU,
//                               pcdet/utils/box_coder_utils.py:13-43 ResidualCoder.encode_torch)
//   pcd_anchor_loss_forward /   pcdet/models/dense_heads/anchor_head_template.py:102-227 with pcdet/utils/loss_utils.py:
//   pcd_anchor_loss_backward    10-74 (sigmoid focal), :338-401 (weighted smooth-L1), :444-469 (weighted cross entropy)
//   pcd_anchor_decode           anchor_head_template.py:229-276 (generate_predicted_boxes) + box_coder_utils.py:45-77
//
// The kernels are the anchor heads' one core (anchorhead_common.h) under its CELL-MAJOR layout; this file holds the entry
// points: argument checks, the config, the launches.  Anchors are never materialised: anchor n of a frame is (y, x, kind) =
// (n / (W * A), n / A % W, n % A), the reference's (y, x, class, size, rotation) order; its centre comes from the host
// generator's shift tables (bit-identical to the reference's torch.arange), its size / heading / z from the kind table.
// The assignment is ANCHOR-driven: one thread per anchor walks the frame's boxes, staged in LDS in chunks of 256 (no cap on
// the number of boxes), and only divides for the pairs that intersect.  Three launches: box preparation, per-box maximum
// (integer atomic max on the bit pattern of a non-negative float: exact and order independent), labels + targets (the IoU
// recomputed with the same instructions, so `== maximum` means what it means in the reference).  No [N, M] matrix, no
// read-back.  What this head fixes in the core's configs: 8-float box rows and 7 codes, smooth-L1, the sin-difference on
// the heading always, classification weights 1.  This file is compiled with -ffp-contract=off (Makefile): labels depend on
// `==` and `>=` of fp32 values evaluated in the reference's order.
#include "anchorhead_common.h"

extern "C" size_t pcd_anchor_assign_workspace_bytes(int batch, int n_boxes) { return assign_workspace_bytes(batch, n_boxes); }

extern "C" int pcd_anchor_assign_targets(const float *gt_boxes, int batch, int n_boxes, const float *kinds, int n_kinds,
                                         const float *classes, int n_classes, const float *shifts, int height, int width,
                                         int *box_cls_labels, float *box_reg_targets, float *reg_weights, int *gt_index,
                                         int *num_pos, void *workspace, size_t workspace_bytes, void *stream) {
    PCD_ENTER();
    if (!kinds || !classes || !shifts || !box_cls_labels || !box_reg_targets || !reg_weights || !num_pos || n_boxes < 0 ||
        (n_boxes > 0 && !gt_boxes))
        return PCD_ERR_INVALID_ARG;
    if (!shape_ok(batch, height, width, n_kinds) || n_classes < 1 || n_classes > ANC_MAX_CLASSES ||
        (long long)batch * n_boxes >= (1ll << 27))
        return PCD_ERR_UNSUPPORTED;
    WsCarver ws(workspace, workspace_bytes);
    const size_t bm = (size_t)batch * (size_t)(n_boxes > 0 ? n_boxes : 1);
    float *pb = ws.take<float>(bm * ANC_BOXF);
    u32 *box_max = ws.take<u32>(bm);
    if (!ws.ok) return PCD_ERR_WORKSPACE;
    launch_assign<CellMajor>(assign_cfg(height, width, n_kinds, n_classes, n_boxes, 7, 0), batch, gt_boxes, pb, box_max, kinds,
                             classes, shifts, box_cls_labels, box_reg_targets, reg_weights, gt_index, num_pos,
                             (hipStream_t)stream);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" size_t pcd_anchor_loss_workspace_bytes(int batch, int height, int width, int n_kinds) {
    return loss_workspace_bytes(batch, height, width, n_kinds);
}

extern "C" int pcd_anchor_loss_forward(const void *cls_preds, const void *box_preds, const void *dir_preds, int dtype,
                                       const long long *strides_host, const int *box_cls_labels, const float *box_reg_targets,
                                       const int *num_pos, int batch, int height, int width, int n_kinds, int num_class,
                                       int num_dir_bins, const float *kinds, const float *code_weights, float cls_weight,
                                       float loc_weight, float dir_weight, float dir_offset, float *out, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    PCD_ENTER();
    CellMajor m;
    AncLossCfg c;
    if (!fill_maps(m, cls_preds, box_preds, dir_preds, nullptr, nullptr, nullptr, dtype, strides_host, n_kinds, num_class) ||
        !box_cls_labels || !box_reg_targets || !num_pos || !kinds || !code_weights || !out)
        return PCD_ERR_INVALID_ARG;
    if (!loss_cfg(c, dtype, batch, height, width, n_kinds, num_class, 7, 0, num_dir_bins, dir_preds != nullptr, true, 1.f, 1.f,
                  cls_weight, loc_weight, dir_weight, dir_offset))
        return PCD_ERR_UNSUPPORTED;
    WsCarver ws(workspace, workspace_bytes);
    dim3 grid(pcd_div_up(height * width * n_kinds, 256), batch);
    float *partials = ws.take<float>((size_t)grid.x * grid.y * 3);
    if (!ws.ok) return PCD_ERR_WORKSPACE;
    launch_loss_forward(m, c, grid, box_cls_labels, box_reg_targets, num_pos, kinds, code_weights, partials, out, AncNoCur(),
                        (hipStream_t)stream);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_anchor_loss_backward(const void *cls_preds, const void *box_preds, const void *dir_preds, void *d_cls,
                                        void *d_box, void *d_dir, int dtype, const long long *strides_host,
                                        const int *box_cls_labels, const float *box_reg_targets, const int *num_pos, int batch,
                                        int height, int width, int n_kinds, int num_class, int num_dir_bins, const float *kinds,
                                        const float *code_weights, float cls_weight, float loc_weight, float dir_weight,
                                        float dir_offset, const float *grad_out, void *stream) {
    PCD_ENTER();
    CellMajor m;
    AncLossCfg c;
    if (!fill_maps(m, cls_preds, box_preds, dir_preds, d_cls, d_box, d_dir, dtype, strides_host, n_kinds, num_class) || !d_cls ||
        !d_box || (dir_preds && !d_dir) || !box_cls_labels || !box_reg_targets || !num_pos || !kinds || !code_weights || !grad_out)
        return PCD_ERR_INVALID_ARG;
    if (!loss_cfg(c, dtype, batch, height, width, n_kinds, num_class, 7, 0, num_dir_bins, dir_preds != nullptr, true, 1.f, 1.f,
                  cls_weight, loc_weight, dir_weight, dir_offset))
        return PCD_ERR_UNSUPPORTED;
    dim3 grid(pcd_div_up(height * width * n_kinds, 256), batch);
    anc_loss_kernel<true, CellMajor, AncNoCur><<<grid, 256, 0, (hipStream_t)stream>>>(
        m, c, box_cls_labels, box_reg_targets, num_pos, kinds, code_weights, grad_out, nullptr, AncNoCur());
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_anchor_decode(const void *cls_preds, const void *box_preds, const void *dir_preds, int dtype,
                                 const long long *strides_host, int batch, int height, int width, int n_kinds, int n_classes,
                                 int num_class, int num_dir_bins, const float *kinds, const float *shifts, float dir_offset,
                                 float dir_limit_offset, float *batch_box_preds, float *batch_cls_preds, void *stream) {
    PCD_ENTER();
    CellMajor m;
    if (!fill_maps(m, cls_preds, box_preds, dir_preds, nullptr, nullptr, nullptr, dtype, strides_host, n_kinds, num_class) ||
        !kinds || !shifts || !batch_box_preds || !batch_cls_preds)
        return PCD_ERR_INVALID_ARG;
    if (!shape_ok(batch, height, width, n_kinds) || n_classes < 1 || n_classes > ANC_MAX_CLASSES || num_class < 1 ||
        num_class > PCD_ANCHOR_MAX_CLASSES || !bins_ok(dir_preds != nullptr, num_dir_bins) ||
        (long long)batch * height * width * n_kinds * num_class >= (1ll << 31))
        return PCD_ERR_UNSUPPORTED;
    m.cls_out = batch_cls_preds;
    const AncDecodeCfg c = decode_cfg(dtype, height, width, n_kinds, n_classes, 7, 0, num_dir_bins, dir_preds != nullptr,
                                      dir_offset, dir_limit_offset);
    dim3 grid(pcd_div_up(height * width * n_kinds, 256), batch);
    anc_decode_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(m, c, kinds, shifts, batch_box_preds);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
