#!/usr/bin/env python3
"""Generate the anchor-head fixtures under tests/golden/ (run once, where the reference lies at /root/reference; not
needed at test time).  In the style of make_golden.py: the reference's own files are imported from their read-only
location under stand-in parent packages, with a `.cuda()` identity patch, and run on the CPU; only arrays and short
labels (data) are stored.

  g19_anchor_generator   AnchorGenerator for the SECOND (188 x 188) and PointPillars (468 x 468) Waymo settings: the
                         shift rows, a sample of anchor rows and a checksum of every anchor tensor
  g20_anchor_targets     AxisAlignedTargetAssigner: the full-size case (B = 4 with 100 / 37 / 1 / 0 boxes, 212 064 anchors
                         per frame, stored sparsely) and a 48 x 40 map whose frames pin the quirks; a class-agnostic case
  g21_anchor_loss        the reference's loss classes driven as get_loss drives them, fp32 and fp64, scalars + gradients
  g22_anchor_decode      generate_predicted_boxes with and without direction classifier

Usage: python tests/golden/make_golden_anchor.py
"""
import hashlib
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/pcdet"
manifest = {}


def _ns(name, path=None, **attrs):
    m = types.ModuleType(name)
    if path:
        m.__path__ = [path]
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def ref_modules():
    _ns("pcdet", REF)
    _ns("pcdet.ops", REF + "/ops")
    _ns("pcdet.ops.iou3d_nms", None, iou3d_nms_utils=types.SimpleNamespace())
    _ns("pcdet.ops.roiaware_pool3d", None, roiaware_pool3d_utils=types.SimpleNamespace())
    _ns("pcdet.models", REF + "/models")
    _ns("pcdet.models.dense_heads", REF + "/models/dense_heads")
    _ns("pcdet.models.dense_heads.target_assigner", REF + "/models/dense_heads/target_assigner")
    _ns("pcdet.models.model_utils", None, centernet_utils=types.SimpleNamespace())
    for name in ("SharedArray", "scipy", "scipy.spatial"):
        try:
            importlib.import_module(name)
        except Exception:
            _ns(name, None, Delaunay=None)
    torch.Tensor.cuda = lambda self, *a, **k: self
    imp = importlib.import_module
    return types.SimpleNamespace(
        ag=imp("pcdet.models.dense_heads.target_assigner.anchor_generator"),
        aa=imp("pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner"),
        bc=imp("pcdet.utils.box_coder_utils"), bu=imp("pcdet.utils.box_utils"), lu=imp("pcdet.utils.loss_utils"),
        cu=imp("pcdet.utils.common_utils"))


class D(dict):
    __getattr__ = dict.__getitem__


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h


def save(name, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    manifest[name] = {"sha256": sha(*[arrays[k] for k in sorted(arrays)]).hexdigest(),
                      "arrays": {k: [str(np.asarray(v).dtype), list(np.asarray(v).shape)] for k, v in arrays.items()},
                      "bytes": os.path.getsize(path)}
    print(f"{name}: {manifest[name]['bytes']} bytes")
    assert manifest[name]["bytes"] < 1 << 20


SIZES = {"Vehicle": [4.7, 2.1, 1.7], "Pedestrian": [0.91, 0.86, 1.73], "Cyclist": [1.78, 0.84, 1.78]}
THRESH = {"Vehicle": (0.55, 0.4), "Pedestrian": (0.5, 0.35), "Cyclist": (0.5, 0.35)}
NAMES = ["Vehicle", "Pedestrian", "Cyclist"]


def anchor_cfgs(names, stride, align_center=False):
    return [D(class_name=n, anchor_sizes=[SIZES[n]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[0],
              align_center=align_center, feature_map_stride=stride, matched_threshold=THRESH[n][0],
              unmatched_threshold=THRESH[n][1]) for n in names]


def model_cfg(cfgs):
    return D(ANCHOR_GENERATOR_CONFIG=cfgs, TARGET_ASSIGNER_CONFIG=D(POS_FRACTION=-1.0, SAMPLE_SIZE=512,
             NORM_BY_NUM_EXAMPLES=False), get=lambda k, d=None: d)


def g19(R):
    out = {}
    for tag, rng, grid, stride, align in (("second", [-75.2, -75.2, -2, 75.2, 75.2, 4], [1504, 1504], 8, False),
                                          ("pillar", [-74.88, -74.88, -2, 74.88, 74.88, 4.0], [468, 468], 1, False),
                                          ("aligned", [0, -39.68, -3, 69.12, 39.68, 1], [432, 496], 2, True)):
        cfgs = anchor_cfgs(NAMES, stride, align)
        gen = R.ag.AnchorGenerator(rng, cfgs)
        anchors, per = gen.generate_anchors([np.array(grid) // stride] * 3)
        out[f"{tag}_range"] = np.array(rng, np.float64)
        out[f"{tag}_grid"] = np.array(grid, np.int64)
        out[f"{tag}_stride"] = np.array([stride], np.int64)
        out[f"{tag}_align"] = np.array([int(align)], np.int64)
        out[f"{tag}_per_location"] = np.array(per, np.int64)
        for c, a in enumerate(anchors):
            a = a.numpy()
            out[f"{tag}_shape{c}"] = np.array(a.shape, np.int64)
            out[f"{tag}_sha{c}"] = np.frombuffer(sha(a).digest(), np.uint8)
            flat = a.reshape(-1, 7)
            out[f"{tag}_rows{c}"] = flat[::997].copy()
            out[f"{tag}_xrow{c}"] = a[0, 0, :, 0, 0, 0].copy()
            out[f"{tag}_yrow{c}"] = a[0, :, 0, 0, 0, 1].copy()
    save("g19_anchor_generator", **out)


def assign_case(R, names, class_names, rng, grid, stride, gt):
    """the reference's assigner on gt [B, M, 8] + the box index of every positive (the arg-max of the reference's own
    IoU function over the class's boxes, mapped back to the frame's rows)."""
    cfgs = anchor_cfgs(names, stride)
    anchors, _ = R.ag.AnchorGenerator(rng, cfgs).generate_anchors([np.array(grid) // stride] * len(names))
    ta = R.aa.AxisAlignedTargetAssigner(model_cfg(cfgs), class_names, R.bc.ResidualCoder(), False)
    out = ta.assign_targets(anchors, torch.from_numpy(gt.copy()))
    labels = out["box_cls_labels"].numpy().astype(np.int32)
    targets = out["box_reg_targets"].numpy()
    weights = out["reg_weights"].numpy()
    B = gt.shape[0]
    N = labels.shape[1]
    A = 2 * len(names)
    gt_index = -np.ones((B, N), np.int32)
    for b in range(B):
        for c, name in enumerate(names):
            cid = class_names.index(name) + 1
            rows = np.nonzero(gt[b, :, 7] == cid)[0]
            if rows.size == 0:
                continue
            flat = anchors[c].view(-1, 7)
            iou = R.bu.boxes3d_nearest_bev_iou(flat, torch.from_numpy(gt[b, rows, :7].copy()))
            arg = rows[iou.argmax(dim=1).numpy()]
            idx = (np.arange(flat.shape[0]) // 2) * A + c * 2 + (np.arange(flat.shape[0]) % 2)   # (y, x, class, rot) order
            pos = labels[b, idx] > 0
            gt_index[b, idx[pos]] = arg[pos]
    assert ((gt_index >= 0) == (labels > 0)).all()
    all_anchors = torch.cat(anchors, dim=-3).view(-1, 7).numpy()
    return labels, targets, weights, gt_index, all_anchors


def sparse_targets(prefix, labels, targets, weights, gt_index, out):
    assert labels.min() >= -1 and labels.max() < 127
    out[prefix + "_labels"] = labels.astype(np.int8)
    pos = np.nonzero(labels > 0)
    assert (targets[labels <= 0] == 0).all() and (weights == (labels > 0)).all()
    out[prefix + "_pos"] = np.stack(pos, 1).astype(np.int32)
    out[prefix + "_pos_targets"] = targets[pos]
    out[prefix + "_pos_gt"] = gt_index[pos]


def full_size_boxes():
    r = np.random.default_rng(7)
    B, M = 4, 128
    gt = np.zeros((B, M, 8), np.float32)
    sizes = np.array([SIZES[n] for n in NAMES], np.float32)
    for b, n in enumerate([100, 37, 1, 0]):
        c = r.integers(1, 4, n)
        gt[b, :n, 0:2] = r.uniform(-74, 74, (n, 2))
        gt[b, :n, 2] = r.uniform(-1, 1, n)
        gt[b, :n, 3:6] = sizes[c - 1] * r.uniform(.8, 1.25, (n, 3))
        gt[b, :n, 6] = r.uniform(-np.pi, np.pi, n)
        gt[b, :n, 7] = c
    return gt


SMALL_RANGE = [0.0, -15.6, -2, 37.6, 15.6, 4]        # 48 x 40 cells of 0.8 m
SMALL_GRID = [48, 40]


def quirk_boxes():
    r = np.random.default_rng(20)
    B, M = 5, 40
    gt = np.zeros((B, M, 8), np.float32)
    f = gt[0]
    f[0] = [8.0, 0.0, 0.2, 4.5, 2.0, 1.6, 0.0, 1]            # two vehicles with the same best anchor
    f[1] = [8.05, 0.02, 0.1, 4.0, 1.9, 1.5, 0.05, 1]
    f[2] = [20.0, 8.0, 0.0, 12.0, 3.5, 3.0, 0.0, 1]          # best IoU below unmatched_threshold: forced positives
    f[3] = [16.0, -8.0, 0.0, 0.9, 0.85, 1.7, 0.3, 2]         # two identical pedestrians: anchors tied between them
    f[4] = [16.0, -8.0, 0.0, 0.9, 0.85, 1.7, 0.3, 2]
    f[5] = [100.0, 3.0, 0.0, 1.8, 0.8, 1.7, 0.0, 3]          # a cyclist far outside the anchors: maximum 0, forces nothing
    f[6] = [30.0, 0.0, 0.0, 4.6, 2.0, 1.7, np.pi / 4 - 1e-3, 1]   # headings on both sides of pi / 4
    f[7] = [30.0, 8.0, 0.0, 4.6, 2.0, 1.7, np.pi / 4 + 1e-3, 1]
    f[8] = [30.0, -8.0, 0.0, 4.6, 2.0, 1.7, 3.5, 1]          # beyond pi
    f[9] = [24.0, -12.0, 0.0, 1.8, 0.85, 1.7, -4.0, 3]
    f[10] = [12.0, 10.0, 0.0, 1.7, 0.8, 1.8, 7.0, 3]
    # (row 11 stays zero: padding in the middle)
    f[12] = [4.0, 12.0, 0.0, 0.95, 0.9, 1.8, 1.57, 2]
    gt[1, 0] = [18.4, 0.4, 0.0, 4.7, 2.1, 1.7, 1.57, 1]      # a frame with one box
    # frame 2: none
    sizes = np.array([SIZES[n] for n in NAMES], np.float32)
    for b, n in ((3, 30), (4, 40)):
        c = r.integers(1, 4, n)
        gt[b, :n, 0:2] = np.stack([r.uniform(0, 37.6, n), r.uniform(-15.6, 15.6, n)], 1)
        gt[b, :n, 2] = r.uniform(-1, 1, n)
        gt[b, :n, 3:6] = sizes[c - 1] * r.uniform(.8, 1.25, (n, 3))
        gt[b, :n, 6] = r.uniform(-2 * np.pi, 2 * np.pi, n)
        gt[b, :n, 7] = c
    return gt


def g20(R):
    out = {}
    gt = full_size_boxes()
    lab, tg, w, gi, _ = assign_case(R, NAMES, NAMES, [-75.2, -75.2, -2, 75.2, 75.2, 4], [1504, 1504], 8, gt)
    print("full size: positives", (lab > 0).sum(1), "ignored", (lab < 0).sum(1))
    out["full_gt_boxes"] = gt
    sparse_targets("full", lab, tg, w, gi, out)
    gt = quirk_boxes()
    lab, tg, w, gi, _ = assign_case(R, NAMES, NAMES, SMALL_RANGE, SMALL_GRID, 1, gt)
    print("small: positives", (lab > 0).sum(1), "ignored", (lab < 0).sum(1))
    out["small_gt_boxes"] = gt
    out["small_range"] = np.array(SMALL_RANGE, np.float64)
    out["small_grid"] = np.array(SMALL_GRID, np.int64)
    sparse_targets("small", lab, tg, w, gi, out)
    # class agnostic: one anchor class, class_names == ['Vehicle']
    gt1 = gt[[0, 3, 2]].copy()
    gt1[gt1[..., 7] != 1] = 0
    lab, tg, w, gi, _ = assign_case(R, ["Vehicle"], ["Vehicle"], SMALL_RANGE, SMALL_GRID, 1, gt1)
    out["single_gt_boxes"] = gt1
    sparse_targets("single", lab, tg, w, gi, out)
    save("g20_anchor_targets", **out)


LOSS_RANGE = [0.0, -4.4, -2, 12.0, 4.4, 4]           # 16 x 12 cells of 0.8 m
LOSS_GRID = [16, 12]
DIR_OFFSET, DIR_LIMIT_OFFSET, NUM_DIR_BINS = 0.78539, 0.0, 2
LOSS_WEIGHTS = dict(cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])


def loss_boxes(names):
    r = np.random.default_rng(21)
    B, M = 3, 12
    gt = np.zeros((B, M, 8), np.float32)
    sizes = np.array([SIZES[n] for n in names], np.float32)
    for b, n in ((0, 10), (2, 5)):                     # frame 1 has no box: no positives
        c = r.integers(1, len(names) + 1, n)
        gt[b, :n, 0:2] = np.stack([r.uniform(0, 12, n), r.uniform(-4.4, 4.4, n)], 1)
        gt[b, :n, 2] = r.uniform(-1, 1, n)
        gt[b, :n, 3:6] = sizes[c - 1] * r.uniform(.8, 1.25, (n, 3))
        gt[b, :n, 6] = r.uniform(-2 * np.pi, 2 * np.pi, n)
        gt[b, :n, 7] = c
    return gt


def g21_g22(R):
    # the template's static methods and loss drivers: the class itself needs its whole package; take the functions
    _ns("pcdet.models.dense_heads.target_assigner.atss_target_assigner", None, ATSSTargetAssigner=None)
    tpl = importlib.import_module("pcdet.models.dense_heads.anchor_head_template").AnchorHeadTemplate
    out21, out22 = {}, {}
    for tag, names in (("multi", NAMES), ("single", ["Vehicle"])):
        num_class = len(names)
        A = 2 * num_class
        gt = loss_boxes(names)
        labels, targets, _, _, all_anchors = assign_case(R, names, names, LOSS_RANGE, LOSS_GRID, 1, gt)
        B, N = labels.shape
        H, W = LOSS_GRID[1], LOSS_GRID[0]
        r = np.random.default_rng(22 + num_class)
        cls = r.normal(0, 2.0, (B, H, W, A * num_class)).astype(np.float32)
        box = r.normal(0, 0.4, (B, H, W, A * 7)).astype(np.float32)
        dirp = r.normal(0, 1.5, (B, H, W, A * NUM_DIR_BINS)).astype(np.float32)
        out21[f"{tag}_gt_boxes"] = gt
        out21[f"{tag}_labels"] = labels.astype(np.int8)
        out21[f"{tag}_targets"] = targets
        out21[f"{tag}_cls"], out21[f"{tag}_box"], out21[f"{tag}_dir"] = cls, box, dirp
        for dt, dtag in ((torch.float32, "f32"), (torch.float64, "f64")):
            me = types.SimpleNamespace(
                forward_ret_dict={}, num_class=num_class, use_multihead=False, num_anchors_per_location=A,
                anchors=[torch.from_numpy(all_anchors).to(dt).view(1, H, W, A, 1, 7)],
                model_cfg=D(LOSS_CONFIG=D(LOSS_WEIGHTS=LOSS_WEIGHTS), DIR_OFFSET=DIR_OFFSET, NUM_DIR_BINS=NUM_DIR_BINS),
                cls_loss_func=R.lu.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0),
                reg_loss_func=R.lu.WeightedSmoothL1Loss(code_weights=LOSS_WEIGHTS["code_weights"]),
                dir_loss_func=R.lu.WeightedCrossEntropyLoss(),
                add_sin_difference=tpl.add_sin_difference, get_direction_target=tpl.get_direction_target)
            me.reg_loss_func.code_weights = me.reg_loss_func.code_weights.to(dt)
            t = [torch.from_numpy(a).to(dt).requires_grad_(True) for a in (cls, box, dirp)]
            me.forward_ret_dict = dict(cls_preds=t[0], box_preds=t[1], dir_cls_preds=t[2],
                                       box_cls_labels=torch.from_numpy(labels.copy()),
                                       box_reg_targets=torch.from_numpy(targets).to(dt))
            old_item = torch.Tensor.item
            cls_loss, tb = tpl.get_cls_layer_loss(me)
            me.forward_ret_dict["box_cls_labels"] = torch.from_numpy(labels.copy())   # (:116 edits the labels in place)
            box_loss, tb2 = tpl.get_box_reg_layer_loss(me)
            assert torch.Tensor.item is old_item
            loss = cls_loss + box_loss
            loss.backward()
            out21[f"{tag}_{dtag}_scalars"] = np.array([float(loss), tb["rpn_loss_cls"], tb2["rpn_loss_loc"],
                                                       tb2["rpn_loss_dir"]], np.float64)
            for name, x in zip(("dcls", "dbox", "ddir"), t):
                out21[f"{tag}_{dtag}_{name}"] = x.grad.numpy()
        # decoding (anchor_head_template.py:229-276) on the same maps, with and without direction classifier
        me = types.SimpleNamespace(anchors=[torch.from_numpy(all_anchors).view(1, H, W, A, 1, 7)], use_multihead=False,
                                   box_coder=R.bc.ResidualCoder(),
                                   model_cfg=D(DIR_OFFSET=DIR_OFFSET, DIR_LIMIT_OFFSET=DIR_LIMIT_OFFSET,
                                               NUM_DIR_BINS=NUM_DIR_BINS))
        tc, tb_, td = (torch.from_numpy(a) for a in (cls, box, dirp))
        c1, b1 = tpl.generate_predicted_boxes(me, B, tc, tb_.clone(), td)
        c0, b0 = tpl.generate_predicted_boxes(me, B, tc, tb_.clone(), None)
        out22[f"{tag}_cls"], out22[f"{tag}_box"], out22[f"{tag}_dir"] = cls, box, dirp
        out22[f"{tag}_batch_cls_preds"] = c1.numpy()
        out22[f"{tag}_batch_box_preds_dir"] = b1.numpy()
        out22[f"{tag}_batch_box_preds_nodir"] = b0.numpy()
        out22[f"{tag}_anchors"] = all_anchors
    for o in (out21, out22):
        o["range"] = np.array(LOSS_RANGE, np.float64)
        o["grid"] = np.array(LOSS_GRID, np.int64)
        o["dir"] = np.array([DIR_OFFSET, DIR_LIMIT_OFFSET, NUM_DIR_BINS], np.float64)
    out21["loss_weights"] = np.array([LOSS_WEIGHTS["cls_weight"], LOSS_WEIGHTS["loc_weight"], LOSS_WEIGHTS["dir_weight"]])
    save("g21_anchor_loss", **out21)
    save("g22_anchor_decode", **out22)


if __name__ == "__main__":
    R = ref_modules()
    g19(R)
    g20(R)
    g21_g22(R)
    with open(os.path.join(HERE, "MANIFEST_anchor.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
