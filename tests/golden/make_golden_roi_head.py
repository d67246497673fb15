#!/usr/bin/env python3
"""Generate the RoI-head fixtures under tests/golden/ (run once, where the reference lies at /root/reference; not needed at
test time).  In the style of make_golden_point_head.py: the reference's own proposal_target_layer.py, roi_head_template.py,
box_coder_utils.py, loss_utils.py, box_utils.py and common_utils.py are imported from their read-only location under stand-in
parent packages, with a `.cuda()` identity patch, and run on the CPU; only arrays (data) are stored.  `iou3d_nms_utils.boxes_iou3d_gpu` is stubbed with the
reference's formula (iou3d_nms_utils.py:49-82) over the BEV overlaps of the C oracle (oracle.boxes_pairwise_bev, the
restatement of iou3d_cpu.cpp the iou3d tests use).  The reference's `subsample_rois` runs as it is under np.random.seed /
torch.manual_seed; the indices it returns are recorded.

For the fp64 values the reference's code runs with `Tensor.float()` left as the identity on fp64 tensors:
common_utils.rotate_points_along_z casts its rotation matrix with .float(), which would make the fp64 run fail in matmul.

  g30_roi_overlaps   max_overlaps / gt_assignment of both scenes, with and without SAMPLE_ROI_BY_EACH_CLASS
  g31_roi_targets    the recorded sampled_inds and all seven ProposalTargetLayer outputs plus gt_of_rois / gt_of_rois_src
                     after RoIHeadTemplate.assign_targets: scene A (roi_iou, by class), scene B (cls, class agnostic)
  g32_roi_loss       get_loss under autograd in f32 and f64 on the targets of scene A: scalars, d rcnn_cls, d rcnn_reg, with
                     and without the corner term, on bf16-rounded inputs, and frame 1 alone (fg_sum == 0)
  g33_roi_decode     generate_predicted_boxes

B = 3, N = 96 RoIs, M = 12 GT rows, R = 32, three classes.
  scene A  frame 0: trailing zero GT rows, fewer foreground RoIs than FG_RATIO * R; frame 1: no valid GT row (bg only, easy
           only); frame 2: RoIs of a class without GT, a GT class without RoIs
  scene B  frame 0: foreground only (every RoI a jittered copy of a GT); frame 1: foreground + easy bg (no hard bg);
           frame 2: foreground + hard bg (no easy bg)
Headings: negative, beyond 2 pi, and RoI / GT pairs facing opposite ways.  Every RoI is drawn until (asserted again from the
stored arrays by tests/test_roi_head_cpu.py): its maximum IoU is more than 1e-4 from each of the four thresholds, its best and
second-best IoU differ by more than 1e-4 unless both are 0, and its canonical heading is more than 1e-4 from pi/2, pi, 3pi/2
before folding.

Usage: python tests/golden/make_golden_roi_head.py
"""
import contextlib
import hashlib
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import oracle as O  # noqa: E402
import roi_head_ref as RR  # noqa: E402

REF = "/root/reference/pcdet"
manifest = {}
B, N, M, R = 3, 96, 12, 32
THRESH = dict(REG_FG_THRESH=0.55, CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1)
MARGIN = 1e-4


class D(dict):
    __getattr__ = dict.__getitem__


def target_cfg(score_type, by_class):
    return D(BOX_CODER='ResidualCoder', ROI_PER_IMAGE=R, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=by_class,
             CLS_SCORE_TYPE=score_type, HARD_BG_RATIO=0.8, **THRESH)


def model_cfg(score_type='roi_iou', by_class=True, corner=True):
    return D(NAME='PVRCNNHead', CLASS_AGNOSTIC=True, SHARED_FC=[32, 32], CLS_FC=[16, 16], REG_FC=[16, 16], DP_RATIO=0.3,
             ROI_GRID_POOL=D(GRID_SIZE=2, MLPS=[[8, 8], [8, 8]], POOL_RADIUS=[0.8, 1.6], NSAMPLE=[4, 4], POOL_METHOD='max_pool'),
             NMS_CONFIG=D(TRAIN=D(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=64, NMS_POST_MAXSIZE=32, NMS_THRESH=0.8),
                          TEST=D(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=64, NMS_POST_MAXSIZE=16, NMS_THRESH=0.7)),
             TARGET_CONFIG=target_cfg(score_type, by_class),
             LOSS_CONFIG=D(CLS_LOSS='BinaryCrossEntropy', REG_LOSS='smooth-l1', CORNER_LOSS_REGULARIZATION=corner,
                           LOSS_WEIGHTS={'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.5, 'rcnn_corner_weight': 0.75,
                                         'code_weights': [1.0, 1.0, 1.2, 1.0, 0.9, 1.0, 1.1]}))


def _ns(name, path=None, **attrs):
    m = types.ModuleType(name)
    if path:
        m.__path__ = [path]
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def iou3d_np(a, b):
    """iou3d_nms_utils.py:49-82 in float32 over the oracle's BEV overlap"""
    a, b = np.ascontiguousarray(a[:, :7], np.float32), np.ascontiguousarray(b[:, :7], np.float32)
    f = np.float32
    a_max, a_min = (a[:, 2] + a[:, 5] / f(2))[:, None], (a[:, 2] - a[:, 5] / f(2))[:, None]
    b_max, b_min = (b[:, 2] + b[:, 5] / f(2))[None, :], (b[:, 2] - b[:, 5] / f(2))[None, :]
    bev = O.boxes_pairwise_bev(a, b, False)
    h = np.clip(np.minimum(a_max, b_max) - np.maximum(a_min, b_min), f(0), None)
    o3 = bev * h
    va, vb = (a[:, 3] * a[:, 4] * a[:, 5])[:, None], (b[:, 3] * b[:, 4] * b[:, 5])[None, :]
    return (o3 / np.clip(va + vb - o3, f(1e-6), None)).astype(np.float32)


def boxes_iou3d_stub(boxes_a, boxes_b):
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    return torch.from_numpy(iou3d_np(boxes_a.detach().numpy(), boxes_b.detach().numpy()))


def ref_modules():
    torch.Tensor.cuda = lambda self, *a, **k: self         # (WeightedSmoothL1Loss moves its code weights with .cuda())
    _ns("pcdet", REF)
    _ns("pcdet.ops", REF + "/ops")
    _ns("pcdet.ops.iou3d_nms", None, iou3d_nms_utils=types.SimpleNamespace(boxes_iou3d_gpu=boxes_iou3d_stub))
    _ns("pcdet.ops.roiaware_pool3d", None, roiaware_pool3d_utils=types.SimpleNamespace())
    _ns("pcdet.models", REF + "/models")
    mu = _ns("pcdet.models.model_utils", None, centernet_utils=types.SimpleNamespace())
    mu.model_nms_utils = _ns("pcdet.models.model_utils.model_nms_utils", None, class_agnostic_nms=None)
    _ns("pcdet.models.roi_heads", REF + "/models/roi_heads")
    _ns("pcdet.models.roi_heads.target_assigner", REF + "/models/roi_heads/target_assigner")
    for name in ("SharedArray", "scipy", "scipy.spatial"):
        try:
            importlib.import_module(name)
        except Exception:
            _ns(name, None, Delaunay=None)
    imp = importlib.import_module
    return types.SimpleNamespace(ptl=imp("pcdet.models.roi_heads.target_assigner.proposal_target_layer"),
                                 tmpl=imp("pcdet.models.roi_heads.roi_head_template"))


@contextlib.contextmanager
def keep_double():
    """Tensor.float() as the identity on fp64 tensors (module docstring)"""
    orig = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self if self.dtype == torch.float64 else orig(self, *a, **k)
    try:
        yield
    finally:
        torch.Tensor.float = orig


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


# ---------------------------------------------------------------------------------------------------------------------
def gt_rows(r, n, classes):
    """n well separated GT boxes (8 columns), headings in [-2 pi, 2 pi]"""
    b = np.zeros((n, 8), np.float32)
    cells = r.permutation(36)[:n]
    b[:, 0] = (cells % 6) * 12.0 - 30.0 + r.uniform(-1, 1, n)
    b[:, 1] = (cells // 6) * 12.0 - 30.0 + r.uniform(-1, 1, n)
    b[:, 2] = r.uniform(-1, 1, n)
    b[:, 3] = r.uniform(2.0, 5.0, n)
    b[:, 4] = r.uniform(1.2, 2.5, n)
    b[:, 5] = r.uniform(1.2, 2.0, n)
    b[:, 6] = r.uniform(-2 * np.pi, 2 * np.pi, n)
    b[:, 7] = np.asarray(classes)[r.integers(0, len(classes), n)]
    return b


JITTER = {'fg': 0.04, 'hard': 0.22, 'easy': 0.75}
BANDS = {'fg': (0.55, 1.01), 'hard': (0.1, 0.55), 'easy': (-1.0, 0.1)}


def canonical_heading(roi, g):
    two_pi = np.float32(2 * np.pi)
    return np.float32((np.float32(g[6]) - np.float32(roi[6]) % two_pi) % two_pi)


def roi_is_clean(roi, label, gt, by_class_too):
    """the three fixture conditions for one RoI, under both assignment modes"""
    ious = iou3d_np(roi[None], gt)[0]
    modes = [np.ones(len(gt), bool)] + ([gt[:, 7].astype(np.int64) == label] if by_class_too else [])
    out = []
    for mask in modes:
        v = np.where(mask, ious, -1.0)
        order = np.argsort(-v, kind='stable')
        best = max(float(v[order[0]]), 0.0) if mask.any() else 0.0
        second = max(float(v[order[1]]), 0.0) if mask.sum() > 1 else 0.0
        if any(abs(best - t) <= 10 * MARGIN for t in THRESH.values()):
            return None
        if not (best == 0.0 and second == 0.0) and best - second <= 10 * MARGIN:
            return None
        g = gt[order[0]] if mask.any() else gt[0]                  # (torch.max: the first of equal values)
        h = canonical_heading(roi, g)
        if any(abs(float(h) - t) <= 10 * MARGIN for t in (np.pi / 2, np.pi, 3 * np.pi / 2)):
            return None
        out.append(best)
    return out


def make_roi(r, gt_valid, gt_all, band, label_of, by_class):
    """one RoI in the wanted IoU band (of the mode the scene is sampled in): a jittered copy of a GT row"""
    lo, hi = BANDS[band]
    for _ in range(2000):
        g = gt_valid[r.integers(0, len(gt_valid))] if len(gt_valid) else None
        if g is None or (band == 'easy' and r.random() < 0.5):
            roi = gt_rows(r, 1, [1])[0, :7]
            label = label_of(int(r.integers(1, 4)))
        else:
            j = JITTER[band] * r.uniform(0.3, 1.0)
            roi = g[:7].copy()
            roi[0:3] += (r.uniform(-j, j, 3) * g[3:6]).astype(np.float32)
            roi[3:6] *= (1 + r.uniform(-j, j, 3) * 0.5).astype(np.float32)
            roi[6] += np.float32(r.uniform(-j, j) * 0.5)
            flip = r.random()
            if flip < 0.25:
                roi[6] += np.float32(np.pi)                       # faces the other way: the flip branch
            elif flip < 0.4:
                roi[6] += np.float32(2 * np.pi * r.choice([-1, 1]))
            label = label_of(int(g[7]))
        clean = roi_is_clean(roi, label, gt_all, True)
        if clean is None:
            continue
        v = clean[1] if by_class else clean[0]
        if lo + 1e-3 < v < hi - 1e-3 or (band == 'easy' and v < hi - 1e-3):
            return roi, label
    raise RuntimeError(f"no RoI in band {band}")


def make_frame(r, n_valid, classes, bands, by_class, label_of=lambda c: c):
    gt = np.zeros((M, 8), np.float32)
    gt[:n_valid] = gt_rows(r, n_valid, classes)
    rois, labels = np.zeros((N, 7), np.float32), np.zeros((N,), np.int64)
    want = [b for b, cnt in bands for _ in range(cnt)]
    assert len(want) == N
    for i, band in enumerate([want[q] for q in r.permutation(N)]):
        rois[i], labels[i] = make_roi(r, gt[:n_valid], gt[:max(n_valid, 1)], band, label_of, by_class)
    return gt, rois, labels


def scenes():
    r = np.random.default_rng(30)
    swap = lambda c: 3 if c == 2 else c                              # noqa: E731  (class-2 GT rows get class-3 RoIs)
    A = [make_frame(r, 8, [1, 2, 3], [('fg', 9), ('hard', 30), ('easy', 57)], True),
         make_frame(r, 0, [1], [('easy', 96)], True),
         make_frame(r, 12, [1, 2], [('fg', 40), ('hard', 26), ('easy', 30)], True, label_of=swap)]
    Bs = [make_frame(r, 12, [1, 2, 3], [('fg', 96)], False),
          make_frame(r, 10, [1, 2, 3], [('fg', 30), ('easy', 66)], False),
          make_frame(r, 11, [1, 2, 3], [('fg', 20), ('hard', 76)], False)]
    a2_gt, a2_lab = set(A[2][0][:, 7].astype(int)), set(A[2][2].tolist())
    assert 2 in a2_gt and 2 not in a2_lab and 3 in a2_lab and 3 not in a2_gt, (a2_gt, a2_lab)
    assert (A[0][0][8:] == 0).all() and (A[0][0][7] != 0).any()
    out = {}
    for tag, frames in (("A", A), ("B", Bs)):
        out[tag] = dict(gt_boxes=np.stack([f[0] for f in frames]), rois=np.stack([f[1] for f in frames]),
                        roi_labels=np.stack([f[2] for f in frames]),
                        roi_scores=r.uniform(0, 1, (B, N)).astype(np.float32))
    return out


def batch_dict(s):
    return {'batch_size': B, 'rois': torch.from_numpy(s['rois']).clone(), 'roi_scores': torch.from_numpy(s['roi_scores']).clone(),
            'roi_labels': torch.from_numpy(s['roi_labels']).clone(), 'gt_boxes': torch.from_numpy(s['gt_boxes']).clone()}


def g30(Rm, S):
    out = {}
    for tag, s in S.items():
        out.update({f"{tag}_{k}": v for k, v in s.items()})
        for by_class in (False, True):
            layer = Rm.ptl.ProposalTargetLayer(target_cfg('roi_iou', by_class))
            ovs, gas = [], []
            for b in range(B):
                gt = torch.from_numpy(s['gt_boxes'][b])
                k = M - 1
                while k >= 0 and gt[k].sum() == 0:
                    k -= 1
                gt = gt[:k + 1]
                gt = gt.new_zeros((1, 8)) if len(gt) == 0 else gt
                rois, lab = torch.from_numpy(s['rois'][b]), torch.from_numpy(s['roi_labels'][b])
                if by_class:
                    ov, ga = layer.get_max_iou_with_same_class(rois=rois, roi_labels=lab, gt_boxes=gt[:, 0:7], gt_labels=gt[:, -1].long())
                else:
                    ov, ga = torch.max(Rm.ptl.iou3d_nms_utils.boxes_iou3d_gpu(rois, gt[:, 0:7]), dim=1)
                ovs.append(ov.numpy())
                gas.append(ga.numpy())
            key = "by_class" if by_class else "any_class"
            out[f"{tag}_{key}_max_overlaps"] = np.stack(ovs).astype(np.float32)
            out[f"{tag}_{key}_gt_assignment"] = np.stack(gas).astype(np.int32)
    save("g30_roi_overlaps", **out)
    return out


TARGET_KEYS = ('rois', 'gt_of_rois', 'gt_iou_of_rois', 'roi_scores', 'roi_labels', 'reg_valid_mask', 'rcnn_cls_labels')


def g31(Rm, S, g30_out):
    out = dict(thresholds=np.array([THRESH[k] for k in ('REG_FG_THRESH', 'CLS_FG_THRESH', 'CLS_BG_THRESH', 'CLS_BG_THRESH_LO')]),
               sampler=np.array([R, 0.5, 0.8]))
    heads = {}
    for tag, score_type, by_class in (("A", "roi_iou", True), ("B", "cls", False)):
        head = Rm.tmpl.RoIHeadTemplate(num_class=1, model_cfg=model_cfg(score_type, by_class))
        recorded = []
        inner = head.proposal_target_layer.subsample_rois
        head.proposal_target_layer.subsample_rois = lambda max_overlaps, _f=inner, _r=recorded: _r.append(_f(max_overlaps=max_overlaps)) or _r[-1]
        np.random.seed(31)
        torch.manual_seed(31)
        td = head.assign_targets(batch_dict(S[tag]))
        inds = np.stack([t.numpy() for t in recorded]).astype(np.int32)
        assert inds.shape == (B, R)
        out[f"{tag}_sampled_inds"] = inds
        for k in TARGET_KEYS + ('gt_of_rois_src',):
            out[f"{tag}_{k}"] = td[k].numpy()
        # the same transformation in fp64 (the bar of the test must hold for the reference's own f32 values): the reference's
        # assign_targets over the fp64 copies of what its ProposalTargetLayer returned
        td_in = {k: td[k].clone() for k in TARGET_KEYS}
        td_in['gt_of_rois'] = td['gt_of_rois_src'].clone()
        td_in = {k: (v.double() if v.is_floating_point() else v) for k, v in td_in.items()}
        layer_forward = head.proposal_target_layer.forward
        head.proposal_target_layer.forward = lambda batch_dict, _t=td_in: _t
        with keep_double():
            td64 = head.assign_targets({'batch_size': B})
        head.proposal_target_layer.forward = layer_forward
        out[f"{tag}_gt_of_rois_f64"] = td64['gt_of_rois'].numpy()
        mo = g30_out[f"{tag}_{'by_class' if by_class else 'any_class'}_max_overlaps"]
        counts = []
        for b in range(B):
            fg, hard, easy = RR.category_lists(mo[b], model_cfg(score_type, by_class).TARGET_CONFIG)
            k = RR.slot_counts(len(fg), len(hard), len(easy), model_cfg(score_type, by_class).TARGET_CONFIG)
            assert np.isin(inds[b, :k[0]], fg).all() and np.isin(inds[b, k[0]:k[0] + k[1]], hard).all() \
                and np.isin(inds[b, k[0] + k[1]:], easy).all()
            counts.append([len(fg), len(hard), len(easy), k[0], k[1], k[2]])
            print(f"g31 {tag} frame {b}: fg {len(fg)} hard {len(hard)} easy {len(easy)} -> slots {k}")
        out[f"{tag}_counts"] = np.asarray(counts, np.int64)
        heads[tag] = (head, td)
    cA, cB = out["A_counts"], out["B_counts"]
    assert 0 < cA[0, 0] < 16 and cA[1, 0] == 0 and cA[1, 1] == 0 and cA[2, 0] > 16
    assert cB[0, 1] == 0 and cB[0, 2] == 0 and cB[1, 1] == 0 and cB[1, 2] > 0 and cB[2, 2] == 0 and cB[2, 1] > 0
    save("g31_roi_targets", **out)
    return heads


def bf16_round(a):
    return torch.from_numpy(np.asarray(a, np.float32)).bfloat16().float().numpy()


def run_loss(Rm, td, rcnn_cls, rcnn_reg, corner, dt, rows=None):
    head = Rm.tmpl.RoIHeadTemplate(num_class=1, model_cfg=model_cfg('roi_iou', True, corner))
    f = {}
    for k, v in td.items():
        v = v.clone()
        if rows is not None:
            v = v[rows]
        f[k] = v.to(dt) if v.is_floating_point() else v
    x = torch.from_numpy(rcnn_cls).to(dt).requires_grad_(True)
    y = torch.from_numpy(rcnn_reg).to(dt).requires_grad_(True)
    f['rcnn_cls'], f['rcnn_reg'] = x, y
    head.forward_ret_dict = f
    ctx = keep_double() if dt == torch.float64 else contextlib.nullcontext()
    with ctx:
        loss, tb = head.get_loss()
        loss.backward()
    scal = np.array([float(loss), tb['rcnn_loss_cls'], tb['rcnn_loss_reg'], tb.get('rcnn_loss_corner', 0.0)], np.float64)
    assert abs(tb['rcnn_loss'] - float(loss)) < 1e-12
    return scal, x.grad.numpy(), (y.grad.numpy() if y.grad is not None else np.zeros(rcnn_reg.shape))


def g32(Rm, heads):
    r = np.random.default_rng(32)
    _, td = heads["A"]
    n = B * R
    rcnn_cls = r.normal(0, 2.0, (n, 1)).astype(np.float32)
    rcnn_reg = r.normal(0, 0.3, (n, 7)).astype(np.float32)
    out = dict(rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg, rcnn_cls_bf16=bf16_round(rcnn_cls), rcnn_reg_bf16=bf16_round(rcnn_reg),
               weights=np.array([1.0, 1.5, 0.75]), code_weights=np.array([1.0, 1.0, 1.2, 1.0, 0.9, 1.0, 1.1]))
    cases = (("corner", True, rcnn_cls, rcnn_reg, None), ("plain", False, rcnn_cls, rcnn_reg, None),
             ("bf16", True, out["rcnn_cls_bf16"], out["rcnn_reg_bf16"], None),
             ("nofg", True, rcnn_cls[R:2 * R], rcnn_reg[R:2 * R], slice(1, 2)))
    for tag, corner, xc, xr, rows in cases:
        for dt, dtag in ((torch.float32, "f32"), (torch.float64, "f64")):
            scal, dc, dr = run_loss(Rm, td, xc, xr, corner, dt, rows)
            out[f"{tag}_{dtag}_scalars"], out[f"{tag}_{dtag}_dcls"], out[f"{tag}_{dtag}_dreg"] = scal, dc, dr
            print(f"g32 {tag} {dtag}: loss {scal[0]:.6f} cls {scal[1]:.6f} reg {scal[2]:.6f} corner {scal[3]:.6f}")
    assert out["nofg_f64_scalars"][2] == 0 and out["nofg_f64_scalars"][3] == 0 and not out["nofg_f64_dreg"].any()
    assert out["corner_f64_scalars"][3] > 0
    save("g32_roi_loss", **out)


def g33(Rm, S):
    r = np.random.default_rng(33)
    head = Rm.tmpl.RoIHeadTemplate(num_class=1, model_cfg=model_cfg())
    rois = S["A"]["rois"]
    box = r.normal(0, 0.3, (B * N, 7)).astype(np.float32)
    cls = r.normal(0, 1, (B * N, 1)).astype(np.float32)
    out = dict(rois=rois, box_preds=box, cls_preds=cls)
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        with (keep_double() if dt == torch.float64 else contextlib.nullcontext()):
            c, b = head.generate_predicted_boxes(B, torch.from_numpy(rois).to(dt), torch.from_numpy(cls).to(dt),
                                                 torch.from_numpy(box).to(dt))
        assert tuple(c.shape) == (B, N, 1)
        out[f"batch_box_preds_{tag}"] = b.numpy()
    save("g33_roi_decode", **out)


def state_dict_keys():
    """names and shapes of the state dict of the REFERENCE's PVRCNNHead for model_cfg() and 16 input channels: its
    pvrcnn_head.py and pointnet2_modules.py imported as they stand, over a parameter-free stand-in for the compiled
    pointnet2_utils.QueryAndGroup"""
    class QueryAndGroup(torch.nn.Module):
        def __init__(self, radius, nsample, use_xyz=True):
            super().__init__()
    stub = _ns("pcdet.ops.pointnet2.pointnet2_stack.pointnet2_utils", None, QueryAndGroup=QueryAndGroup)
    _ns("pcdet.ops.pointnet2", REF + "/ops/pointnet2")
    _ns("pcdet.ops.pointnet2.pointnet2_stack", REF + "/ops/pointnet2/pointnet2_stack", pointnet2_utils=stub)
    mod = importlib.import_module("pcdet.models.roi_heads.pvrcnn_head")
    head = mod.PVRCNNHead(input_channels=16, model_cfg=model_cfg(), num_class=1)
    return {k: list(v.shape) for k, v in head.state_dict().items()}


if __name__ == "__main__":
    Rm = ref_modules()
    S = scenes()
    o30 = g30(Rm, S)
    heads = g31(Rm, S, o30)
    g32(Rm, heads)
    g33(Rm, S)
    with open(os.path.join(HERE, "roi_head_state_dict_keys.json"), "w") as f:
        json.dump(state_dict_keys(), f, indent=1)
    with open(os.path.join(HERE, "MANIFEST_roi_head.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
