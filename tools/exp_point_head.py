"""Time of the PointHeadSimple targets + loss and of the roiaware ops on one MI355X, against the reference's formulation.

Config-4 size (PV-RCNN on Waymo): 4 frames x 4096 keypoints, 128 padded GT rows, 3 classes.
  (a) the reference's formulation, transcribed here: the per-frame host loop of assign_stack_targets
      (point_head_template.py:73-103: boolean-mask indexing, `bs_mask.sum()`, two points_in_boxes_gpu calls per frame) and
      the torch chain of get_cls_layer_loss (:131-155, with its two `.item()` calls) + backward -- calling this project's
      points_in_boxes_gpu, so (a) pays nothing for the reference's own point-in-box kernel;
  (b) the fused assign + loss + backward (pcd_point_head_*), eager and replayed from a captured graph.
The same size through the box + part head (PointIntraPartOffsetHead with all three branches): (a) additionally encodes the
box labels (encode_torch as a dozen elementwise launches per frame), rotates the part labels and runs get_part_layer_loss
and get_box_layer_loss with their three `.item()` calls; (b) is pcd_point_head_assign_targets_full +
pcd_point_head_full_loss_forward / _backward.
Also: points_in_boxes_gpu on one 160 k-point frame (128 boxes), and RoIAwarePool3d forward / backward at PartA2 size
(128 RoIs, 16384 points, 128 channels, out_size 12), max and avg.

Every figure is a host clock around ITERS calls that end in a device synchronise, after WARM warm-up calls of the same
shapes; the variants alternate inside each of ROUNDS rounds and the median / minimum / maximum over the rounds is
printed.  One JSON line at the end.  Needs the GPU (no fallback)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ITERS, ROUNDS = 10, 50, 7


def reference_assign(points, gt_boxes, extend_gt_boxes, num_class, points_in_boxes_gpu):
    """point_head_template.py:73-103 (set_ignore_flag branch), statement by statement"""
    import torch  # noqa: F401
    batch_size = gt_boxes.shape[0]
    bs_idx = points[:, 0]
    point_cls_labels = points.new_zeros(points.shape[0]).long()
    for k in range(batch_size):
        bs_mask = (bs_idx == k)
        points_single = points[bs_mask][:, 1:4]
        point_cls_labels_single = point_cls_labels.new_zeros(bs_mask.sum())
        box_idxs_of_pts = points_in_boxes_gpu(points_single.unsqueeze(dim=0), gt_boxes[k:k + 1, :, 0:7].contiguous()
                                              ).long().squeeze(dim=0)
        box_fg_flag = (box_idxs_of_pts >= 0)
        extend_box_idxs_of_pts = points_in_boxes_gpu(points_single.unsqueeze(dim=0), extend_gt_boxes[k:k + 1, :, 0:7].contiguous()
                                                     ).long().squeeze(dim=0)
        fg_flag = box_fg_flag
        ignore_flag = fg_flag ^ (extend_box_idxs_of_pts >= 0)
        point_cls_labels_single[ignore_flag] = -1
        gt_box_of_fg_points = gt_boxes[k][box_idxs_of_pts[fg_flag]]
        point_cls_labels_single[fg_flag] = 1 if num_class == 1 else gt_box_of_fg_points[:, -1].long()
        point_cls_labels[bs_mask] = point_cls_labels_single
    return point_cls_labels


def reference_cls_loss(point_cls_preds, point_cls_labels, num_class, weight):
    """point_head_template.py:131-155 with loss_utils.py:41-74, statement by statement (the two .item() calls included)"""
    import torch
    positives = (point_cls_labels > 0)
    negative_cls_weights = (point_cls_labels == 0) * 1.0
    cls_weights = (negative_cls_weights + 1.0 * positives).float()
    pos_normalizer = positives.sum(dim=0).float()
    cls_weights /= torch.clamp(pos_normalizer, min=1.0)
    one_hot_targets = point_cls_preds.new_zeros(*list(point_cls_labels.shape), num_class + 1)
    one_hot_targets.scatter_(-1, (point_cls_labels * (point_cls_labels >= 0).long()).unsqueeze(dim=-1).long(), 1.0)
    one_hot_targets = one_hot_targets[..., 1:]
    pred_sigmoid = torch.sigmoid(point_cls_preds)
    alpha_weight = one_hot_targets * 0.25 + (1 - one_hot_targets) * 0.75
    pt = one_hot_targets * (1.0 - pred_sigmoid) + (1.0 - one_hot_targets) * pred_sigmoid
    focal_weight = alpha_weight * torch.pow(pt, 2.0)
    bce_loss = torch.clamp(point_cls_preds, min=0) - point_cls_preds * one_hot_targets + \
        torch.log1p(torch.exp(-torch.abs(point_cls_preds)))
    loss = focal_weight * bce_loss * cls_weights.unsqueeze(-1)
    point_loss_cls = loss.sum() * weight
    tb = {'point_loss_cls': point_loss_cls.item(), 'point_pos_num': pos_normalizer.item()}
    return point_loss_cls, tb


def reference_assign_full(points, gt_boxes, extend_gt_boxes, num_class, points_in_boxes_gpu, mean_size):
    """point_head_template.py:73-129 with ret_box_labels and ret_part_labels (set_ignore_flag branch), statement by statement;
    encode_torch (box_coder_utils.py:162-187) and rotate_points_along_z (common_utils.py) written out"""
    import torch
    batch_size = gt_boxes.shape[0]
    bs_idx = points[:, 0]
    point_cls_labels = points.new_zeros(points.shape[0]).long()
    point_box_labels = gt_boxes.new_zeros((points.shape[0], 8))
    point_part_labels = gt_boxes.new_zeros((points.shape[0], 3))
    for k in range(batch_size):
        bs_mask = (bs_idx == k)
        points_single = points[bs_mask][:, 1:4]
        point_cls_labels_single = point_cls_labels.new_zeros(bs_mask.sum())
        box_idxs_of_pts = points_in_boxes_gpu(points_single.unsqueeze(dim=0), gt_boxes[k:k + 1, :, 0:7].contiguous()
                                              ).long().squeeze(dim=0)
        box_fg_flag = (box_idxs_of_pts >= 0)
        extend_box_idxs_of_pts = points_in_boxes_gpu(points_single.unsqueeze(dim=0), extend_gt_boxes[k:k + 1, :, 0:7].contiguous()
                                                     ).long().squeeze(dim=0)
        fg_flag = box_fg_flag
        ignore_flag = fg_flag ^ (extend_box_idxs_of_pts >= 0)
        point_cls_labels_single[ignore_flag] = -1
        gt_box_of_fg_points = gt_boxes[k][box_idxs_of_pts[fg_flag]]
        point_cls_labels_single[fg_flag] = 1 if num_class == 1 else gt_box_of_fg_points[:, -1].long()
        point_cls_labels[bs_mask] = point_cls_labels_single
        if gt_box_of_fg_points.shape[0] > 0:
            point_box_labels_single = point_box_labels.new_zeros((bs_mask.sum(), 8))
            boxes, pts, gt_classes = gt_box_of_fg_points[:, :-1], points_single[fg_flag], gt_box_of_fg_points[:, -1].long()
            boxes[:, 3:6] = torch.clamp_min(boxes[:, 3:6], min=1e-5)
            xg, yg, zg, dxg, dyg, dzg, rg = torch.split(boxes, 1, dim=-1)
            xa, ya, za = torch.split(pts, 1, dim=-1)
            assert gt_classes.max() <= mean_size.shape[0]
            point_anchor_size = mean_size[gt_classes - 1]
            dxa, dya, dza = torch.split(point_anchor_size, 1, dim=-1)
            diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
            xt = (xg - xa) / diagonal
            yt = (yg - ya) / diagonal
            zt = (zg - za) / dza
            dxt = torch.log(dxg / dxa)
            dyt = torch.log(dyg / dya)
            dzt = torch.log(dzg / dza)
            point_box_labels_single[fg_flag] = torch.cat([xt, yt, zt, dxt, dyt, dzt, torch.cos(rg), torch.sin(rg)], dim=-1)
            point_box_labels[bs_mask] = point_box_labels_single
        point_part_labels_single = point_part_labels.new_zeros((bs_mask.sum(), 3))
        transformed_points = points_single[fg_flag] - gt_box_of_fg_points[:, 0:3]
        angle = -gt_box_of_fg_points[:, 6]
        cosa, sina = torch.cos(angle), torch.sin(angle)
        zeros, ones = angle.new_zeros(angle.shape[0]), angle.new_ones(angle.shape[0])
        rot_matrix = torch.stack((cosa, sina, zeros, -sina, cosa, zeros, zeros, zeros, ones), dim=1).view(-1, 3, 3).float()
        transformed_points = torch.matmul(transformed_points.view(-1, 1, 3), rot_matrix).view(-1, 3)
        offset = torch.tensor([0.5, 0.5, 0.5]).view(1, 3).type_as(transformed_points)
        point_part_labels_single[fg_flag] = (transformed_points / gt_box_of_fg_points[:, 3:6]) + offset
        point_part_labels[bs_mask] = point_part_labels_single
    return point_cls_labels, point_box_labels, point_part_labels


def reference_box_part_loss(point_cls_labels, point_box_preds, point_box_labels, point_part_preds, point_part_labels, code_weights,
                            box_weight, part_weight):
    """get_part_layer_loss and get_box_layer_loss (point_head_template.py:157-191, loss_utils.py:372-399), statement by
    statement, their three .item() calls included"""
    import torch
    import torch.nn.functional as F
    pos_mask = point_cls_labels > 0
    pos_normalizer = max(1, (pos_mask > 0).sum().item())
    point_loss_part = F.binary_cross_entropy(torch.sigmoid(point_part_preds), point_part_labels, reduction='none')
    point_loss_part = (point_loss_part.sum(dim=-1) * pos_mask.float()).sum() / (3 * pos_normalizer)
    point_loss_part = point_loss_part * part_weight
    tb = {'point_loss_part': point_loss_part.item()}
    reg_weights = pos_mask.float()
    pos_normalizer = pos_mask.sum().float()
    reg_weights /= torch.clamp(pos_normalizer, min=1.0)
    inp, target, weights = point_box_preds[None, ...], point_box_labels[None, ...], reg_weights[None, ...]
    target = torch.where(torch.isnan(target), inp, target)
    diff = inp - target
    diff = diff * code_weights.view(1, 1, -1)
    n = torch.abs(diff)
    beta = 1.0 / 9.0
    loss = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    loss = loss * weights.unsqueeze(-1)
    point_loss_box = loss.sum() * box_weight
    tb['point_loss_box'] = point_loss_box.item()
    return point_loss_part, point_loss_box, tb


def timed(fn, iters=ITERS):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def compare(variants):
    """{name: fn} -> {name: (median, min, max) us per call}; warm-up, then ROUNDS rounds in which the variants alternate"""
    for fn in variants.values():
        for _ in range(WARM):
            fn()
    samples = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            samples[k].append(timed(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def main():
    import numpy as np
    import torch
    from com_amd import roiaware_pool3d as RP
    from com_amd.hotpath import point_head as PH
    assert torch.cuda.is_available(), "tools/exp_point_head.py measures on the GPU"
    r = np.random.default_rng(0)
    result = {"device": torch.cuda.get_device_name(0), "warm": WARM, "iters": ITERS, "rounds": ROUNDS}
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    # ---- config-4 size: 4 x 4096 keypoints, 128 padded GT rows (40 real), 3 classes
    B, P, M, NC, W = 4, 4096, 128, 3, 1.0
    gt = np.zeros((B, M, 8), np.float32)
    for b in range(B):
        n = 40
        gt[b, :n, 0:2] = r.uniform(-70, 70, (n, 2))
        gt[b, :n, 2] = r.uniform(-1, 1, n)
        gt[b, :n, 3:6] = r.uniform(0.6, 5.0, (n, 3))
        gt[b, :n, 6] = r.uniform(-3.14, 3.14, n)
        gt[b, :n, 7] = r.integers(1, NC + 1, n)
    pcs = []
    for b in range(B):
        near = gt[b, r.integers(0, 40, P // 2), :3] + r.uniform(-2.5, 2.5, (P // 2, 3))
        far = np.concatenate([r.uniform(-75, 75, (P - P // 2, 2)), r.uniform(-2, 4, (P - P // 2, 1))], 1)
        pcs.append(np.concatenate([np.full((P, 1), b), np.concatenate([near, far])], 1))
    pc, gtd = cu(np.concatenate(pcs)), cu(gt)
    extra = [0.2, 0.2, 0.2]
    logits = torch.randn(B * P, NC, device="cuda", requires_grad=True)

    def ref_step():
        ext = gtd.clone()
        ext[:, :, 3:6] += gtd.new_tensor(extra)[None, None, :]                  # enlarge_box3d
        labels = reference_assign(pc, gtd, ext, NC, RP.points_in_boxes_gpu)
        loss, tb = reference_cls_loss(logits, labels, NC, W)
        (g,) = torch.autograd.grad(loss, logits)
        return labels, loss, g

    def fused_step():
        labels, num_pos = PH.assign_targets(pc, gtd, extra, NC)
        loss = PH.point_cls_loss(logits, labels, num_pos, NC, W)
        (g,) = torch.autograd.grad(loss, logits)
        return labels, loss, g

    la, lossa, ga = ref_step()
    lb, lossb, gb = fused_step()
    assert torch.equal(la, lb), "the fused labels differ from the reference formulation's"
    assert abs(float(lossa) - float(lossb)) <= 1e-5 * abs(float(lossa)) and float((ga - gb).abs().max()) <= 1e-6 * float(ga.abs().max())
    result["point_head_positives"] = int((lb > 0).sum())
    result["point_head_ignored"] = int((lb < 0).sum())
    # no autograd graph of an eager step may be alive during capture (tests/test_gpu_static.py): keep detached values only
    lossb = lossb.detach().clone()
    del la, lossa, ga, gb
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fused_step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static[0], lb) and torch.equal(static[1], lossb)
    t = compare({"reference_formulation": ref_step, "fused_eager": fused_step, "fused_graph": graph.replay})
    for k, v in t.items():
        result[f"point_head_{k}_us"] = [round(x, 1) for x in v]
        print(f"point head, assign + loss + backward, {k:22s}: median {v[0]:8.1f} us  (min {v[1]:.1f}, max {v[2]:.1f})")

    # ---- the same size through the box + part head (PointIntraPartOffsetHead with all three branches, Part-A2-free):
    #      targets with box and part labels + the three losses + backward
    mean_cpu = torch.tensor([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])
    mean_dev = mean_cpu.cuda()
    code_w = torch.ones(8, device="cuda")
    WB, WP = 1.0, 1.0
    box_preds = torch.randn(B * P, 8, device="cuda", requires_grad=True)
    part_preds = torch.randn(B * P, 3, device="cuda", requires_grad=True)
    preds = [logits, box_preds, part_preds]

    def ref_full_step():
        ext = gtd.clone()
        ext[:, :, 3:6] += gtd.new_tensor(extra)[None, None, :]
        labels, bl, pl = reference_assign_full(pc, gtd, ext, NC, RP.points_in_boxes_gpu, mean_dev)
        loss_cls, _ = reference_cls_loss(logits, labels, NC, W)
        loss_part, loss_box, _ = reference_box_part_loss(labels, box_preds, bl, part_preds, pl, code_w, WB, WP)
        loss = loss_cls + loss_part
        loss += loss_box
        return labels, loss, torch.autograd.grad(loss, preds)

    def fused_full_step():
        labels, bl, pl, num_pos = PH.assign_targets_full(pc, gtd, extra, NC, mean_size=mean_dev, ret_box_labels=True,
                                                         ret_part_labels=True)
        out = PH.point_head_loss(logits, labels, num_pos, NC, W, box_preds=box_preds, box_labels=bl, code_weights=code_w,
                                 box_weight=WB, part_preds=part_preds, part_labels=pl, part_weight=WP)
        return labels, out[0], torch.autograd.grad(out[0], preds)

    la, lossa, ga = ref_full_step()
    lb2, lossb2, gb = fused_full_step()
    assert torch.equal(la, lb2), "the fused labels differ from the reference formulation's"
    assert abs(float(lossa) - float(lossb2)) <= 1e-5 * abs(float(lossa))
    assert all(float((p - q).abs().max()) <= 1e-5 * float(p.abs().max()) for p, q in zip(ga, gb))
    lossb2 = lossb2.detach().clone()
    del la, lossa, ga, gb
    torch.cuda.synchronize()
    graph_full = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_full):
        static_full = fused_full_step()
    graph_full.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_full[0], lb2) and torch.equal(static_full[1], lossb2)
    t = compare({"reference_formulation": ref_full_step, "fused_eager": fused_full_step, "fused_graph": graph_full.replay})
    for k, v in t.items():
        result[f"point_head_box_part_{k}_us"] = [round(x, 1) for x in v]
        print(f"box + part head, assign + 3 losses + backward, {k:22s}: median {v[0]:8.1f} us  (min {v[1]:.1f}, max {v[2]:.1f})")

    # ---- one 160 k-point frame through points_in_boxes_gpu
    P1 = 160000
    near = gt[0, r.integers(0, 40, P1 // 4), :3] + r.uniform(-2.5, 2.5, (P1 // 4, 3))
    far = np.concatenate([r.uniform(-75, 75, (P1 - P1 // 4, 2)), r.uniform(-2, 4, (P1 - P1 // 4, 1))], 1)
    frame, boxes = cu(np.concatenate([near, far]))[None], gtd[:1, :, :7].contiguous()
    t = compare({"points_in_boxes_gpu_160k": lambda: RP.points_in_boxes_gpu(frame, boxes)})
    v = t["points_in_boxes_gpu_160k"]
    result["points_in_boxes_gpu_160k_us"] = [round(x, 1) for x in v]
    result["points_in_boxes_gpu_160k_inside"] = int((RP.points_in_boxes_gpu(frame, boxes) >= 0).sum())
    print(f"points_in_boxes_gpu, 160 k points x 128 boxes       : median {v[0]:8.1f} us  (min {v[1]:.1f}, max {v[2]:.1f})")

    # ---- RoI-aware pooling at PartA2 size
    N, P2, C, OUT = 128, 16384, 128, 12
    rois = np.zeros((N, 7), np.float32)
    rois[:, 0:2] = r.uniform(-40, 40, (N, 2))
    rois[:, 3:6] = r.uniform(1.5, 5.0, (N, 3))
    rois[:, 6] = r.uniform(-3.14, 3.14, N)
    near = rois[r.integers(0, N, P2 // 2), :3] + r.uniform(-2.0, 2.0, (P2 // 2, 3))
    far = np.concatenate([r.uniform(-45, 45, (P2 // 2, 2)), r.uniform(-2, 2, (P2 // 2, 1))], 1)
    roisd, ptsd = cu(rois), cu(np.concatenate([near, far]))
    feat = torch.randn(P2, C, device="cuda", requires_grad=True)
    pool = RP.RoIAwarePool3d(OUT, 128)
    grad_out = torch.randn(N, OUT, OUT, OUT, C, device="cuda")
    variants = {}
    for method in ("max", "avg"):
        variants[f"forward_{method}"] = (lambda m: lambda: pool(roisd, ptsd, feat.detach(), pool_method=m))(method)
        variants[f"forward_backward_{method}"] = (lambda m: lambda: torch.autograd.grad(pool(roisd, ptsd, feat, pool_method=m), feat,
                                                                                        grad_out))(method)
    lists = pool(roisd, ptsd, feat, pool_method="max").grad_fn.roiaware_pool3d_for_backward[0]
    result["roiaware_points_listed"] = int(lists[..., 0].sum())
    t = compare(variants)
    for k, v in t.items():
        result[f"roiaware_{k}_us"] = [round(x, 1) for x in v]
        print(f"RoIAwarePool3d 128 x 12^3 x 128, {k:24s}: median {v[0]:8.1f} us  (min {v[1]:.1f}, max {v[2]:.1f})")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
