"""Numpy transcription of the four natives of the reference's roiaware_pool3d extension (roiaware_pool3d.cpp:29-168,
roiaware_pool3d_kernel.cu:16-359): points_in_boxes_cpu, points_in_boxes_gpu, forward, backward -- float32 where the C
code computes in float, float64 where it computes in double, statement by statement.  The reference ships no CPU build
of them, so tests/golden/make_golden_point_head.py stubs `roiaware_pool3d_cuda` with `stub_module()` and runs the
reference's own Python (roiaware_pool3d_utils, box_utils, PointHeadSimple) on top: the torch-side logic of fixtures
g26-g29 is the reference's, the natives are this transcription (cross-pinned, not pinned).  Also here: the boundary
band the tests leave out, and a plain-torch restatement of get_cls_layer_loss.  Test infrastructure only."""
import types

import numpy as np
import torch

F32 = np.float32
MARGIN_GPU = 1e-5     # roiaware_pool3d_kernel.cu:27
MARGIN_CPU = 1e-2     # roiaware_pool3d.cpp:131


def check_pt_in_box3d(pts, box, margin):
    """check_pt_in_box3d for every row of pts (P, 3) float32 against one box (7,) float32 ->
    (in_flag bool (P,), z_ok bool (P,), local_x, local_y float32 (P,))."""
    pts = np.asarray(pts, F32)
    box = np.asarray(box, F32)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    cx, cy, cz, dx, dy, dz, rz = box
    z_ok = ~(np.abs(z - cz).astype(np.float64) > np.float64(dz) / 2.0)          # fabsf(z - cz) > dz / 2.0
    cosa, sina = np.cos(F32(-rz)), np.sin(F32(-rz))                             # cos(-rot_angle), sin(-rot_angle) in float
    sx, sy = x - cx, y - cy
    lx = sx * cosa + sy * (-sina)
    ly = sx * sina + sy * cosa
    m = np.float64(F32(margin))                                                 # const float MARGIN
    in_xy = (np.abs(lx).astype(np.float64) < np.float64(dx) / 2.0 + m) & (np.abs(ly).astype(np.float64) < np.float64(dy) / 2.0 + m)
    return z_ok & in_xy, z_ok, lx.astype(F32), ly.astype(F32)


def points_in_boxes_cpu(boxes, pts):
    """roiaware_pool3d.cpp:143-168: (N, P) int32 0 / 1, every box on its own"""
    boxes, pts = np.asarray(boxes, F32), np.asarray(pts, F32)
    out = np.zeros((boxes.shape[0], pts.shape[0]), np.int32)
    for i in range(boxes.shape[0]):
        out[i] = check_pt_in_box3d(pts, boxes[i], MARGIN_CPU)[0]
    return out


def points_in_boxes_gpu(boxes, pts):
    """roiaware_pool3d_kernel.cu:313-336: boxes (B, N, 7), pts (B, P, 3) -> (B, P) int32, the first box that contains the
    point, -1 for none"""
    boxes, pts = np.asarray(boxes, F32), np.asarray(pts, F32)
    out = -np.ones(pts.shape[:2], np.int32)
    for b in range(boxes.shape[0]):
        for k in range(boxes.shape[1] - 1, -1, -1):                              # descending: the lowest index wins
            out[b][check_pt_in_box3d(pts[b], boxes[b, k], MARGIN_GPU)[0]] = k
    return out


def band_mask(boxes, pts, margin, tol=1e-5):
    """(P,) bool: the points the comparisons leave out -- |local_x| or |local_y| within `tol` of d / 2 + margin for some box
    (N, 7) whose z test the point passes (device, libm and numpy cosf may differ in the last place)."""
    boxes, pts = np.asarray(boxes, F32), np.asarray(pts, F32)
    out = np.zeros(pts.shape[0], bool)
    for box in boxes:
        _, z_ok, lx, ly = check_pt_in_box3d(pts, box, margin)
        bx = np.float64(box[3]) / 2.0 + margin
        by = np.float64(box[4]) / 2.0 + margin
        out |= z_ok & ((np.abs(np.abs(lx).astype(np.float64) - bx) <= tol) | (np.abs(np.abs(ly).astype(np.float64) - by) <= tol))
    return out


def voxel_coords(pts, roi, out_size):
    """generate_pts_mask_for_box3d (roiaware_pool3d_kernel.cu:39-75): (inside bool (P,), flat voxel index int (P,),
    the three float quotients (P, 3) before truncation)"""
    ox, oy, oz = out_size
    roi = np.asarray(roi, F32)
    inside, _, lx, ly = check_pt_in_box3d(pts, roi, MARGIN_GPU)
    lz = np.asarray(pts, F32)[:, 2] - roi[2]
    q = []
    idx = []
    for loc, d, o in ((lx, roi[3], ox), (ly, roi[4], oy), (lz, roi[5], oz)):
        res = F32(d) / F32(o)
        quot = ((loc + F32(d) / F32(2)) / res).astype(F32)
        q.append(quot)
        i = np.where(inside, quot, 0).astype(np.int32).astype(np.uint32)        # unsigned int x_idx = int(...)
        idx.append(np.minimum(np.maximum(i, np.uint32(0)), np.uint32(o - 1)).astype(np.int64))
    return inside, (idx[0] * oy + idx[1]) * oz + idx[2], np.stack(q, 1)


def roiaware_pool3d_forward(rois, pts, feat, out_size, max_pts_each_voxel, pool_method):
    """roiaware_pool3d_launcher (:193-233), pool_method 0 = max, 1 = avg, in feat's dtype ->
    (pooled (N, ox, oy, oz, C), argmax int32 (same shape; zeros for avg), pts_idx_of_voxels int32 (N, ox, oy, oz, mpv))"""
    ox, oy, oz = out_size
    rois, pts = np.asarray(rois, F32), np.asarray(pts, F32)
    feat = np.asarray(feat)
    n, c, nvox, mpv = rois.shape[0], feat.shape[1], ox * oy * oz, max_pts_each_voxel
    lists = np.zeros((n, nvox, mpv), np.int32)
    pooled = np.zeros((n, nvox, c), feat.dtype)
    argmax = np.zeros((n, nvox, c), np.int32)
    for b in range(n):
        inside, vox, _ = voxel_coords(pts, rois[b], out_size)
        for k in np.nonzero(inside)[0]:                                         # collect_inside_pts_for_box3d: k ascending
            cnt = lists[b, vox[k], 0]
            if cnt < mpv - 1:
                lists[b, vox[k], cnt + 1] = k
                lists[b, vox[k], 0] += 1
        for v in range(nvox):
            total = lists[b, v, 0]
            if pool_method == 0:
                arg = -np.ones(c, np.int32)
                mx = np.full(c, -np.inf, feat.dtype)                            # (float)-1e50
                for k in lists[b, v, 1:total + 1]:
                    better = feat[k] > mx
                    mx = np.where(better, feat[k], mx)
                    arg = np.where(better, k, arg).astype(np.int32)
                pooled[b, v] = np.where(arg != -1, mx, 0)
                argmax[b, v] = arg
            elif total > 0:
                s = np.zeros(c, feat.dtype)
                for k in lists[b, v, 1:total + 1]:
                    s = s + feat[k]
                pooled[b, v] = s / feat.dtype.type(total)
    shape = (n, ox, oy, oz)
    return pooled.reshape(shape + (c,)), argmax.reshape(shape + (c,)), lists.reshape(shape + (mpv,))


def roiaware_pool3d_backward(lists, argmax, grad_out, num_pts, pool_method):
    """roiaware_pool3d_backward_launcher (:289-310) in grad_out's dtype (the order of the atomic additions is not fixed in
    the reference; here: box, voxel, list order)"""
    grad_out = np.asarray(grad_out)
    c = grad_out.shape[-1]
    mpv = lists.shape[-1]
    go = grad_out.reshape(-1, c)
    grad_in = np.zeros((num_pts, c), grad_out.dtype)
    if pool_method == 0:
        am = argmax.reshape(-1, c)
        rows, cols = np.nonzero(am != -1)
        np.add.at(grad_in, (am[rows, cols], cols), go[rows, cols])
    else:
        ls = lists.reshape(-1, mpv)
        for v in np.nonzero(ls[:, 0] > 0)[0]:
            total = ls[v, 0]
            cur = grad_out.dtype.type(1) / max(grad_out.dtype.type(total), grad_out.dtype.type(1))
            for k in ls[v, 1:total + 1]:
                grad_in[k] += go[v] * cur
    return grad_in


def stub_module():
    """what `from . import roiaware_pool3d_cuda` finds: the four natives with the binder's signatures (torch tensors, results
    written into the tensors the caller allocated)"""
    def cpu(boxes, pts, out):
        out.copy_(torch.from_numpy(points_in_boxes_cpu(boxes.numpy(), pts.numpy())))
        return 1

    def gpu(boxes, pts, out):
        out.copy_(torch.from_numpy(points_in_boxes_gpu(boxes.numpy(), pts.numpy())))
        return 1

    def forward(rois, pts, feat, argmax, lists, pooled, pool_method):
        p, a, l = roiaware_pool3d_forward(rois.numpy(), pts.numpy(), feat.detach().numpy(), tuple(lists.shape[1:4]),
                                          lists.shape[4], pool_method)
        pooled.copy_(torch.from_numpy(p))
        argmax.copy_(torch.from_numpy(a))
        lists.copy_(torch.from_numpy(l))
        return 1

    def backward(lists, argmax, grad_out, grad_in, pool_method):
        grad_in.copy_(torch.from_numpy(roiaware_pool3d_backward(lists.numpy(), argmax.numpy(), grad_out.numpy(),
                                                                 grad_in.shape[0], pool_method)))
        return 1

    return types.SimpleNamespace(points_in_boxes_cpu=cpu, points_in_boxes_gpu=gpu, forward=forward, backward=backward)


def assign_stack_targets(point_coords, gt_boxes, extra_width, num_class):
    """PointHeadSimple.assign_targets (point_head_simple.py:21-48, point_head_template.py:73-103) over the transcription:
    point_coords (N, 4), gt_boxes (B, M, 8) -> int64 labels (N,)"""
    pc, gt = np.asarray(point_coords, F32), np.asarray(gt_boxes, F32)
    ext = gt.copy()
    ext[:, :, 3:6] += np.asarray(extra_width, F32)[None, None, :]
    labels = np.zeros(pc.shape[0], np.int64)
    for k in range(gt.shape[0]):
        m = pc[:, 0] == k
        p = pc[m][:, 1:4]
        idx = points_in_boxes_gpu(gt[k:k + 1, :, :7], p[None])[0]
        eidx = points_in_boxes_gpu(ext[k:k + 1, :, :7], p[None])[0]
        fg = idx >= 0
        single = np.zeros(p.shape[0], np.int64)
        single[fg ^ (eidx >= 0)] = -1
        single[fg] = 1 if num_class == 1 else gt[k][idx[fg]][:, -1].astype(np.int64)
        labels[m] = single
    return labels


def cls_layer_loss(preds, labels, num_class, cls_weight):
    """get_cls_layer_loss (point_head_template.py:131-148 with loss_utils.py:41-74) in plain torch, in the dtype of preds;
    differentiable"""
    dt = preds.dtype
    labels = labels.long()
    cared = labels >= 0
    w = cared.to(dt) / torch.clamp((labels > 0).sum().to(dt), min=1.0)
    one_hot = torch.nn.functional.one_hot(labels * cared, num_class + 1)[..., 1:].to(dt)
    p = torch.sigmoid(preds)
    alpha_w = one_hot * 0.25 + (1 - one_hot) * 0.75
    pt = one_hot * (1.0 - p) + (1.0 - one_hot) * p
    bce = torch.clamp(preds, min=0) - preds * one_hot + torch.log1p(torch.exp(-torch.abs(preds)))
    return (alpha_w * pt ** 2 * bce * w.unsqueeze(-1)).sum() * cls_weight
