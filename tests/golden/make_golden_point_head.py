#!/usr/bin/env python3
"""Generate the point-head / roiaware fixtures under tests/golden/ (run once, where the reference lies at
/root/reference; not needed at test time).  In the style of make_golden_anchor.py: the reference's own files are imported
from their read-only location under stand-in parent packages and run on the CPU; only arrays (data) are stored.  The
reference's `roiaware_pool3d_cuda` extension has no CPU build: it is stubbed by the numpy transcription of its four
natives in tests/point_head_ref.py, and everything above it -- roiaware_pool3d_utils (points_in_boxes_cpu / _gpu,
RoIAwarePool3dFunction), box_utils.enlarge_box3d, box_utils.remove_points_in_boxes3d, PointHeadSimple.assign_targets and
get_cls_layer_loss -- is the reference's own code.

  g26_points_in_boxes     both margins: points_in_boxes_cpu (N, P), points_in_boxes_gpu at B = 1 and B = 4, and the rows
                          remove_points_in_boxes3d keeps
  g27_point_head_targets  PointHeadSimple.assign_targets, num_class 1 and 3: padded GT rows, overlapping boxes of
                          different classes (first match), points in the ignore shell and around the origin (the enlarged
                          zero rows)
  g28_point_head_loss     get_cls_layer_loss under autograd, f32 and f64: loss, d logits, tb scalars
  g29_roiaware_pool       RoIAwarePool3d max / avg: lists, argmax, pooled features, grad_in; a max_pts_each_voxel = 4 case
                          that overflows the cap

Every fixture is generated under its own conditions (asserted below): at most 0.1 % of the points in the 1e-5 boundary
band, no pooled point in the band or within 1e-4 of a voxel boundary.

Usage: python tests/golden/make_golden_point_head.py
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
sys.path.insert(0, os.path.dirname(HERE))
import point_head_ref as PR  # noqa: E402

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
    stub = PR.stub_module()
    pkg = _ns("pcdet.ops.roiaware_pool3d", REF + "/ops/roiaware_pool3d", roiaware_pool3d_cuda=stub)
    sys.modules["pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda"] = stub
    _ns("pcdet.models", REF + "/models")
    _ns("pcdet.models.dense_heads", REF + "/models/dense_heads")
    _ns("pcdet.models.model_utils", None, centernet_utils=types.SimpleNamespace())
    for name in ("SharedArray", "scipy", "scipy.spatial"):
        try:
            importlib.import_module(name)
        except Exception:
            _ns(name, None, Delaunay=None)
    imp = importlib.import_module
    R = types.SimpleNamespace(ru=imp("pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils"), bu=imp("pcdet.utils.box_utils"),
                              lu=imp("pcdet.utils.loss_utils"), ph=imp("pcdet.models.dense_heads.point_head_simple"))
    assert pkg.roiaware_pool3d_utils is R.ru and R.ru.roiaware_pool3d_cuda is stub
    return R


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
    assert manifest[name]["bytes"] < 600 * 1024


def random_boxes(r, n, lo, hi, classes=3):
    """n boxes (8 columns) of 0.5 m and more with centres in [lo, hi]^2; every third box overlaps its predecessor"""
    b = np.zeros((n, 8), np.float32)
    b[:, 0:2] = r.uniform(lo, hi, (n, 2))
    b[:, 2] = r.uniform(-1, 1, n)
    b[:, 3] = r.uniform(0.5, 5.0, n)
    b[:, 4] = r.uniform(0.5, 2.5, n)
    b[:, 5] = r.uniform(0.5, 2.0, n)
    b[:, 6] = r.uniform(-2 * np.pi, 2 * np.pi, n)
    b[:, 7] = r.integers(1, classes + 1, n)
    for k in range(2, n, 3):
        b[k, 0:3] = b[k - 1, 0:3] + r.uniform(-0.4, 0.4, 3).astype(np.float32)
        b[k, 7] = b[k - 1, 7] % classes + 1                  # another class: first match decides the label
    return b


def points_around(r, boxes, n_near, n_far, lo, hi, spread=0.75):
    """n_near points scattered over the boxes (some inside, some in a shell around them), n_far over the scene"""
    k = r.integers(0, boxes.shape[0], n_near)
    u = r.uniform(-spread, spread, (n_near, 3)).astype(np.float32) * boxes[k, 3:6]
    c, s = np.cos(boxes[k, 6]), np.sin(boxes[k, 6])
    near = np.stack([boxes[k, 0] + u[:, 0] * c - u[:, 1] * s, boxes[k, 1] + u[:, 0] * s + u[:, 1] * c, boxes[k, 2] + u[:, 2]], 1)
    far = np.concatenate([r.uniform(lo, hi, (n_far, 2)), r.uniform(-2, 2, (n_far, 1))], 1)
    p = np.concatenate([near, far]).astype(np.float32)
    return p[r.permutation(p.shape[0])]


def band_fraction(boxes, pts, margin):
    return float(PR.band_mask(boxes, pts, margin).mean())


def g26(R):
    r = np.random.default_rng(26)
    out = {}
    boxes = random_boxes(r, 24, -30, 30)[:, :7].copy()
    pts = points_around(r, boxes, 6000, 6000, -32, 32)
    for margin in (PR.MARGIN_CPU, PR.MARGIN_GPU):
        f = band_fraction(boxes, pts, margin)
        print(f"g26 single: band fraction at margin {margin}: {f:.2e}")
        assert f <= 1e-3
    mask = R.ru.points_in_boxes_cpu(pts, boxes)
    assert isinstance(mask, np.ndarray) and mask.dtype == np.int32 and mask.shape == (24, 12000)
    assert (mask.sum(0) > 1).any(), "no point in two boxes"
    idx = R.ru.points_in_boxes_gpu(torch.from_numpy(pts)[None], torch.from_numpy(boxes)[None]).numpy()
    extra = r.uniform(0, 1, (pts.shape[0], 2)).astype(np.float32)          # (num_points, 3 + C)
    kept = R.bu.remove_points_in_boxes3d(np.concatenate([pts, extra], 1), boxes)
    keep_idx = np.nonzero(mask.sum(0) == 0)[0].astype(np.int32)
    assert np.array_equal(kept[:, :3], pts[keep_idx])
    print(f"g26 single: {int((mask.sum(0) > 0).sum())} points in a box, {int((mask.sum(0) > 1).sum())} in two, "
          f"{int((idx >= 0).sum())} at the device margin")
    out.update(single_boxes=boxes, single_pts=pts, single_extra=extra, single_mask_cpu=mask.astype(np.int8), single_idx_gpu=idx,
               single_keep_idx=keep_idx)
    B, M, P = 4, 32, 4096
    bb = np.zeros((B, M, 7), np.float32)
    pp = np.zeros((B, P, 3), np.float32)
    for b, n in enumerate([32, 20, 9, 1]):
        bx = random_boxes(r, max(n, 3), -20, 20)[:n, :7]
        bb[b, :n] = bx
        pp[b] = points_around(r, bx, P // 2, P // 2, -22, 22)
        assert band_fraction(bb[b], pp[b], PR.MARGIN_GPU) <= 1e-3
    idx4 = R.ru.points_in_boxes_gpu(torch.from_numpy(pp), torch.from_numpy(bb)).numpy()
    out.update(batch_boxes=bb, batch_pts=pp, batch_idx_gpu=idx4)
    save("g26_points_in_boxes", **out)


EXTRA_WIDTH = [0.2, 0.2, 0.2]


def head_cfg():
    return D(CLS_FC=[32, 32], CLASS_AGNOSTIC=False, USE_POINT_FEATURES_BEFORE_FUSION=False,
             TARGET_CONFIG=D(GT_EXTRA_WIDTH=EXTRA_WIDTH), LOSS_CONFIG=D(LOSS_REG='smooth-l1', LOSS_WEIGHTS={'point_cls_weight': 1.5}))


def g27_g28(R):
    r = np.random.default_rng(27)
    B, M, P = 4, 20, 2048
    gt = np.zeros((B, M, 8), np.float32)
    pcs = []
    for b, n in enumerate([16, 11, 6, 3]):
        gt[b, :n] = random_boxes(r, n, -20, 20)
        p = points_around(r, gt[b, :n, :7], P // 2 - 64, P // 2, -22, 22, spread=0.62)
        origin = r.uniform(-0.25, 0.25, (64, 3)).astype(np.float32)          # around the enlarged zero rows
        p = np.concatenate([p, origin])[r.permutation(P)]
        pcs.append(np.concatenate([np.full((P, 1), b, np.float32), p], 1))
    pc = np.concatenate(pcs)
    ext = gt.copy()
    ext[..., 3:6] += np.asarray(EXTRA_WIDTH, np.float32)
    for b in range(B):
        f = max(band_fraction(gt[b, :, :7], pc[pc[:, 0] == b, 1:], PR.MARGIN_GPU),
                band_fraction(ext[b, :, :7], pc[pc[:, 0] == b, 1:], PR.MARGIN_GPU))
        print(f"g27 frame {b}: band fraction {f:.2e}")
        assert f <= 1e-3
    out27 = dict(point_coords=pc, gt_boxes=gt, extra_width=np.asarray(EXTRA_WIDTH, np.float64))
    out28 = dict(point_cls_weight=np.array([1.5]))
    for num_class in (1, 3):
        head = R.ph.PointHeadSimple(num_class=num_class, input_channels=8, model_cfg=head_cfg())
        td = head.assign_targets({'point_coords': torch.from_numpy(pc), 'gt_boxes': torch.from_numpy(gt)})
        labels = td['point_cls_labels'].numpy()
        assert labels.dtype == np.int64 and td['point_box_labels'] is None
        assert np.array_equal(labels, PR.assign_stack_targets(pc, gt, EXTRA_WIDTH, num_class))
        for b in range(B):
            lb = labels[pc[:, 0] == b]
            assert (lb > 0).any() and (lb == 0).any() and (lb == -1).any(), "a frame without one of the three labels"
        print(f"g27 num_class {num_class}: positives {(labels > 0).sum()}, ignored {(labels < 0).sum()}")
        out27[f"labels_c{num_class}"] = labels.astype(np.int8)
        # the loss on every second point
        sub = labels[::2].copy()
        logits = r.normal(0, 2.0, (sub.shape[0], num_class)).astype(np.float32)
        out28[f"c{num_class}_labels"] = sub.astype(np.int8)
        out28[f"c{num_class}_logits"] = logits
        for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            x = torch.from_numpy(logits).to(dt).requires_grad_(True)
            head.forward_ret_dict = {'point_cls_labels': torch.from_numpy(sub), 'point_cls_preds': x}
            loss, tb = head.get_loss()
            loss.backward()
            ours = PR.cls_layer_loss(x.detach(), torch.from_numpy(sub), num_class, 1.5)
            assert abs(float(ours) - float(loss)) <= 1e-5 * abs(float(loss))
            out28[f"c{num_class}_{tag}_scalars"] = np.array([float(loss), tb['point_loss_cls'], tb['point_pos_num']], np.float64)
            out28[f"c{num_class}_{tag}_dlogits"] = x.grad.numpy()
    # first match is exercised: a foreground point inside two boxes of different classes
    first = 0
    for b in range(B):
        p = pc[pc[:, 0] == b, 1:]
        m = np.stack([PR.check_pt_in_box3d(p, box, PR.MARGIN_GPU)[0] for box in gt[b, :, :7]])
        two = m.sum(0) > 1
        cls_first = gt[b, m.argmax(0), 7]
        cls_last = gt[b, M - 1 - m[::-1].argmax(0), 7]
        first += int((two & (cls_first != cls_last)).sum())
    print("g27: points whose label depends on first match:", first)
    assert first > 0
    save("g27_point_head_targets", **out27)
    save("g28_point_head_loss", **out28)


def g29(R):
    r = np.random.default_rng(29)
    out = {}
    N, P, C = 6, 3000, 8
    while True:
        rois = random_boxes(r, N, -6, 6)[:, :7].copy()
        rois[:, 3:6] *= np.float32(1.6)
        pts = points_around(r, rois, 2200, 800, -8, 8, spread=0.6)
        ok = band_fraction(rois, pts, PR.MARGIN_GPU) == 0.0
        for size in ((3, 4, 5), (2, 2, 2)):
            for roi in rois:
                inside, _, q = PR.voxel_coords(pts, roi, size)
                ok &= not (np.abs(q[inside] - np.round(q[inside])) < 1e-4).any()
        if ok:
            break
        print("g29: a point in the band or on a voxel boundary, drawing again")
    feat = r.normal(0, 1, (P, C)).astype(np.float32)
    feat[:, :3] = np.round(feat[:, :3] * 2) / 2                 # ties for the maximum
    out.update(rois=rois, pts=pts, feat=feat)
    for tag, size, mpv in (("full", (3, 4, 5), 128), ("cap", (2, 2, 2), 4)):
        pool = R.ru.RoIAwarePool3d(out_size=size, max_pts_each_voxel=mpv)
        grad_out = r.normal(0, 1, (N,) + size + (C,)).astype(np.float32)
        out[f"{tag}_size"] = np.array(size + (mpv,), np.int64)
        out[f"{tag}_grad_out"] = grad_out
        for method in ("max", "avg"):
            x = torch.from_numpy(feat).requires_grad_(True)
            y = pool(torch.from_numpy(rois), torch.from_numpy(pts), x, pool_method=method)
            ctx = y.grad_fn.roiaware_pool3d_for_backward
            y.backward(torch.from_numpy(grad_out))
            lists, argmax = ctx[0].numpy(), ctx[1].numpy()
            out[f"{tag}_{method}_pooled"] = y.detach().numpy()
            out[f"{tag}_{method}_grad_in"] = x.grad.numpy()
            if method == "max":
                out[f"{tag}_lists"] = lists
                out[f"{tag}_argmax"] = argmax
                n_in = sum(int(PR.voxel_coords(pts, roi, size)[0].sum()) for roi in rois)
                print(f"g29 {tag}: {n_in} points inside, fullest voxel {lists[..., 0].max()}, listed {int(lists[..., 0].sum())}")
                if tag == "cap":
                    assert lists[..., 0].max() == mpv - 1 and int(lists[..., 0].sum()) < n_in, "the cap is not exceeded"
                else:
                    assert int(lists[..., 0].sum()) == n_in and (lists[..., 0] == 0).any()
    save("g29_roiaware_pool", **out)


if __name__ == "__main__":
    R = ref_modules()
    g26(R)
    g27_g28(R)
    g29(R)
    with open(os.path.join(HERE, "MANIFEST_point_head.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
