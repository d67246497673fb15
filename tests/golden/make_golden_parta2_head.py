#!/usr/bin/env python3
"""Generate the PartA2FCHead fixtures under tests/golden/ (run once, where the reference lies at /root/reference; not needed
at test time).  In the style of make_golden_roi_head.py: the reference's own partA2_head.py and roi_head_template.py (with
box_coder_utils.py, loss_utils.py, box_utils.py, common_utils.py) are imported from their read-only location under stand-in
parent packages and run on the CPU; only arrays (data) are stored.

  * `spconv` is a stand-in that runs a SubMConv3d as a dense conv3d over the scattered rows, masked back to the active
    cells, in the dtype of the features (fp64 for the reference values); the weight keeps spconv 2.x's layout
    [Cout, kd, kh, kw, Cin], so the stored state dict is what a checkpoint of the reference holds.
  * `roiaware_pool3d_utils.RoIAwarePool3d` is tests/parta2_head_ref.py's literal CPU transcription of
    roiaware_pool3d_kernel.cu's contract.
  * The proposal targets are given (ProposalTargetLayer has its own fixtures, g30 / g31): the reference's assign_targets
    runs its canonical transformation over them.

For the fp64 values the reference's code runs with `Tensor.float()` left as the identity on fp64 tensors.

  g50_parta2_pool4   the scene, pooled at POOL_SIZE 4: coords, part_rows / rpn_rows in fp64 and as the reference's own fp32
                     gives them, the same with DISABLE_PART, and the fp64 gradients of random upstream gradients
  g51_parta2_pool6   the same scene (stored in g50) at POOL_SIZE 6
  g52_parta2_module  the head at POOL_SIZE 4: state dict, targets, training forward + get_loss (loss scalars, rcnn_cls,
                     rcnn_reg, d point_part_offset) and the eval predictions in fp64, each with the largest deviation of the
                     reference's own fp32 run (`dev_...`)
  g53_parta2_edges   the gradients of that run (first-layer weights, point_features), the fake path (fewer than three
                     rows: labels -1; its made-up rows carry distinct RPN features, conditioning asserted) through the head, and the head with DISABLE_PART, all with g52's state dict

The scene: B = 2 frames of 600 and 400 points (interleaved in the stacked arrays), 8 RoIs per frame, MAX_POINTS_PER_VOXEL 4,
C = 16.  It holds (asserted here and again, from the stored arrays, by tests/test_parta2_head_cpu.py): a voxel with more than
3 points, a point inside several RoIs, a RoI with no point, an all-zero padding RoI, negative headings and headings beyond
2 pi, scores below the threshold and one exactly at it, a voxel whose points all have four exactly-zero part features.  Every
point lies at least 1e-4 of a cell from a voxel face and a box face; every non-zero voxel sum is at least 1e-6 from 0.

Usage: python tests/golden/make_golden_parta2_head.py
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
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import parta2_head_ref as PR  # noqa: E402

REF = "/root/reference/pcdet"
manifest = {}
B, N, C, MPV = 2, 8, 16, 4
NPTS = (600, 400)
THRESH = 0.3
CELL_MARGIN, SUM_MARGIN = 1e-4, 1e-6
F = np.float32


class D(dict):
    __getattr__ = dict.__getitem__


def model_cfg(pool=4, disable_part=False):
    cfg = D(NAME='PartA2FCHead', CLASS_AGNOSTIC=True, SHARED_FC=[32, 32], CLS_FC=[32, 32], REG_FC=[32, 32], DP_RATIO=0.0,
            SEG_MASK_SCORE_THRESH=THRESH,
            ROI_AWARE_POOL=D(POOL_SIZE=pool, NUM_FEATURES=16, MAX_POINTS_PER_VOXEL=MPV),
            NMS_CONFIG=D(TRAIN=D(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=64, NMS_POST_MAXSIZE=N, NMS_THRESH=0.8),
                         TEST=D(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=64, NMS_POST_MAXSIZE=N, NMS_THRESH=0.7)),
            TARGET_CONFIG=D(BOX_CODER='ResidualCoder', ROI_PER_IMAGE=N, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True,
                            CLS_SCORE_TYPE='roi_iou', CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1,
                            HARD_BG_RATIO=0.8, REG_FG_THRESH=0.65),
            LOSS_CONFIG=D(CLS_LOSS='BinaryCrossEntropy', REG_LOSS='smooth-l1', CORNER_LOSS_REGULARIZATION=True,
                          LOSS_WEIGHTS={'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                        'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}))
    if disable_part:
        cfg['DISABLE_PART'] = True
    return cfg


# ---------------------------------------------------------------------------------------------------------------------
# stand-ins
class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape, batch_size):
        self.features, self.indices = features, indices
        self.spatial_shape, self.batch_size = [int(v) for v in spatial_shape], int(batch_size)

    def dense(self):
        i = self.indices.long()
        out = self.features.new_zeros((self.batch_size, self.features.shape[1], *self.spatial_shape))
        out[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]] = self.features
        return out


class SubMConv3d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, bias=False, indice_key=None):
        super().__init__()
        assert kernel_size == 3 and not bias
        self.weight = nn.Parameter(torch.empty(out_channels, 3, 3, 3, in_channels))
        nn.init.normal_(self.weight, 0, (2.0 / (27 * in_channels)) ** 0.5)

    def forward(self, x):
        y = torch.nn.functional.conv3d(x.dense(), self.weight.permute(0, 4, 1, 2, 3), padding=1)
        i = x.indices.long()
        return SparseConvTensor(y[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]], x.indices, x.spatial_shape, x.batch_size)


class SparseSequential(nn.Sequential):
    def forward(self, x):
        for m in self:
            if isinstance(m, (SubMConv3d, SparseSequential)):
                x = m(x)
            else:
                x = SparseConvTensor(m(x.features), x.indices, x.spatial_shape, x.batch_size)
        return x


def _ns(name, path=None, **attrs):
    m = types.ModuleType(name)
    if path:
        m.__path__ = [path]
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def ref_modules():
    torch.Tensor.cuda = lambda self, *a, **k: self
    # the CPU binary_cross_entropy refuses the label -1 of the fake path, which the reference multiplies by a zero mask
    # afterwards (roi_head_template.py:206-208; the CUDA op does not check): clamp the target of such rows
    bce = torch.nn.functional.binary_cross_entropy
    torch.nn.functional.binary_cross_entropy = lambda input, target, *a, **k: bce(input, target.clamp(0, 1), *a, **k)
    sp = types.SimpleNamespace(SparseSequential=SparseSequential, SubMConv3d=SubMConv3d, SparseConvTensor=SparseConvTensor)
    _ns("pcdet", REF)
    _ns("pcdet.utils", REF + "/utils")
    _ns("pcdet.utils.spconv_utils", None, spconv=sp)
    _ns("pcdet.ops", REF + "/ops")
    _ns("pcdet.ops.iou3d_nms", None, iou3d_nms_utils=types.SimpleNamespace(boxes_iou3d_gpu=None))
    _ns("pcdet.ops.roiaware_pool3d", None, roiaware_pool3d_utils=types.SimpleNamespace(RoIAwarePool3d=PR.RoIAwarePool3d))
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
    return importlib.import_module("pcdet.models.roi_heads.partA2_head")


@contextlib.contextmanager
def keep_double():
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
# the scene
def frame_rois(r, shift):
    """8 RoIs: 0 / 1 overlap, 2 heads beyond 2 pi, 1 / 3 head negatively, 5 holds no point, 7 is padding"""
    rois = np.array([[5.0, 2.0, 0.0, 4.0, 1.8, 1.6, 0.4],
                     [6.0, 2.5, 0.1, 3.6, 1.7, 1.5, -0.7],
                     [-6.0, 8.0, -0.3, 4.4, 1.9, 1.7, 2 * np.pi + 0.9],
                     [12.0, -7.0, 0.2, 0.9, 0.8, 1.8, -2.5],
                     [-10.0, -5.0, 0.0, 3.9, 1.6, 1.5, 3.0],
                     [22.0, 22.0, 0.0, 4.0, 1.8, 1.6, 1.0],
                     [1.0, -10.0, 0.1, 2.2, 2.0, 1.4, 7.5],
                     [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], np.float64)
    rois[:7, 0:2] += shift
    rois[:7, 0:3] += r.uniform(-0.2, 0.2, (7, 3))
    rois[:7, 6] += r.uniform(-0.1, 0.1, 7)
    return rois.astype(F)


def to_world(roi, u, out=4):
    """a point at cell coordinates u (of the POOL_SIZE-`out` grid) of the RoI"""
    roi = roi.astype(np.float64)
    loc = u / out * roi[3:6] - roi[3:6] / 2
    c, s = np.cos(roi[6]), np.sin(roi[6])
    return np.array([roi[0] + loc[0] * c - loc[1] * s, roi[1] + loc[0] * s + loc[1] * c, roi[2] + loc[2]])


def clean(rois_b, p):
    """the margins of one point against the RoIs of its frame, at both pool sizes"""
    pc = np.concatenate([[0.0], p])[None].astype(F)
    for out in (4, 6):
        cell, box = PR.margins(rois_b[None], pc, out)
        if min(cell, box) < 20 * CELL_MARGIN:
            return False
    return PR.zero_box_clearance(rois_b[None], pc) > 1e-2


def cells_of(roi, p, out=4):
    roi = roi.astype(np.float64)
    c, s = np.cos(-roi[6]), np.sin(-roi[6])
    sx, sy = p[0] - roi[0], p[1] - roi[1]
    loc = np.array([sx * c - sy * s, sx * s + sy * c, p[2] - roi[2]])
    return (loc + roi[3:6] / 2) / (roi[3:6] / out)


def make_frame(r, b, n, special):
    rois = frame_rois(r, np.array([0.0, 0.0]) if b == 0 else np.array([1.5, -1.0]))
    pts, scores = [], []

    def add(p, score=None):
        p = np.asarray(p, np.float64).astype(F).astype(np.float64)
        if not clean(rois, p):
            return False
        pts.append(p)
        scores.append(r.uniform(0, 1) if score is None else score)
        return True

    if special:
        for k in range(6):                                    # more than 3 points in one voxel of RoI 3 (both grids)
            while not add(to_world(rois[3], np.array([1.5, 1.5, 1.5]) + r.uniform(-0.1, 0.1, 3)), r.uniform(0.4, 1.0)):
                pass
        for k in range(2):                                    # a voxel of RoI 4 whose points have four zero features
            while not add(to_world(rois[4], np.array([1.5, 1.5, 1.5]) + r.uniform(-0.1, 0.1, 3)), 0.0):
                pass
        while not add(to_world(rois[6], np.array([2.5, 0.5, 3.5]) + r.uniform(-0.1, 0.1, 3)), float(F(THRESH))):
            pass                                              # the score exactly at the threshold, alone in its voxel
    while len(pts) < n:
        if r.random() < 0.7:
            k = int(r.choice([0, 1, 2, 3, 4, 6]))
            u = r.uniform(0.02, 3.98, 3)
            p = to_world(rois[k], u)
        else:
            p = np.array([r.uniform(-16, 16), r.uniform(-16, 16), r.uniform(-1.5, 1.5)])
        if special:
            u4, u6 = cells_of(rois[4], p), cells_of(rois[6], p)
            if ((u4 > 0.95) & (u4 < 2.05)).all() or ((u6 > [1.95, -0.05, 2.95]) & (u6 < [3.05, 1.05, 4.05])).all():
                continue                                      # keep the two special voxels to their special points
        add(p)
    order = r.permutation(n)
    return rois, np.asarray(pts)[order].astype(F), np.asarray(scores)[order].astype(F)


def make_scene(seed=50, special=True, npts=NPTS):
    r = np.random.default_rng(seed)
    rois, coords, scores = [], [], []
    for b in range(B):
        ro, p, s = make_frame(r, b, npts[b], special and b == 0)
        rois.append(ro)
        coords.append(np.concatenate([np.full((len(p), 1), b, F), p], axis=1))
        scores.append(s)
    coords, scores = np.concatenate(coords), np.concatenate(scores)
    order = r.permutation(len(coords))                         # the frames interleaved
    coords, scores = coords[order], scores[order]
    P = len(coords)
    return dict(rois=np.stack(rois), point_coords=coords, point_cls_scores=scores,
                point_features=r.normal(0, 1, (P, C)).astype(F), point_part_offset=r.uniform(0, 1, (P, 3)).astype(F))


def check_scene(s):
    """the properties the module docstring lists, at both pool sizes"""
    for out in (4, 6):
        cell, box = PR.margins(s['rois'], s['point_coords'], out)
        assert min(cell, box) >= CELL_MARGIN, (out, cell, box)
        for part in (s['point_part_offset'], s['point_coords'][:, 1:4]):
            ref = PR.sparse_rows(s['rois'], s['point_coords'], s['point_features'], part, s['point_cls_scores'], THRESH, out, MPV)
            sums = ref['sums']
            assert np.abs(sums[sums != 0]).min() >= SUM_MARGIN
            full = [(PR.voxel_of_points(s['rois'][b], s['point_coords'][s['point_coords'][:, 0] == b, 1:4], out)) for b in range(B)]
            counts = [np.stack([np.bincount(v[v >= 0], minlength=out ** 3) for v in f]) for f in full]
            assert max(c.max() for c in counts) > MPV - 1                        # the cut
            assert max(((f >= 0).sum(0)).max() for f in full) > 1                # a point inside several RoIs
            assert all((f[5] < 0).all() and (f[7] < 0).all() for f in full)      # a RoI with no point, the padding RoI
            listed = np.concatenate([l[:, :, 0] for l in ref['lists']]).reshape(sums.shape)
            assert ((listed > 0) & (sums == 0)).any()                            # points, four zero features: not a row
            assert not ref['fake'] and ref['rows_nonzero'] >= 3
    sc = s['point_cls_scores']
    assert (sc == F(THRESH)).sum() == 1 and (sc < F(THRESH)).sum() > 50 and (sc == 0).sum() == 2
    h = s['rois'][:, :, 6]
    assert (h < 0).any() and (h > 2 * np.pi).any() and (s['rois'][:, 7] == 0).all()
    assert sorted(np.bincount(s['point_coords'][:, 0].astype(int)).tolist()) == sorted(NPTS)


# ---------------------------------------------------------------------------------------------------------------------
def pool_case(s, out, disable_part, dt, grads=None):
    """roiaware_pool + nonzero + gather of the reference's formulation under autograd in dtype dt"""
    feats = torch.from_numpy(s['point_features']).to(dt).requires_grad_(True)
    src = s['point_coords'][:, 1:4] if disable_part else s['point_part_offset']
    part_src = torch.from_numpy(np.ascontiguousarray(src)).to(dt).requires_grad_(True)
    scores = torch.from_numpy(s['point_cls_scores']).to(dt)
    part = torch.cat((part_src, scores.view(-1, 1).detach()), dim=1)
    part[part[:, -1] < THRESH, 0:3] = 0
    layer = PR.RoIAwarePool3d(out, MPV)
    pc = torch.from_numpy(s['point_coords'])
    pp, pr = [], []
    for b in range(B):
        m = pc[:, 0] == b
        roi = torch.from_numpy(s['rois'][b])
        pp.append(layer(roi, pc[m, 1:4], part[m], 'avg'))
        pr.append(layer(roi, pc[m, 1:4], feats[m], 'max'))
    pp, pr = torch.cat(pp), torch.cat(pr)
    idx = pp.sum(dim=-1).nonzero()
    part_rows = pp[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]
    rpn_rows = pr[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]
    res = dict(coords=idx.numpy().astype(np.int32), part_rows=part_rows.detach().numpy(), rpn_rows=rpn_rows.detach().numpy())
    if grads is not None:
        (part_rows * torch.from_numpy(grads[0]).to(dt)).sum().add((rpn_rows * torch.from_numpy(grads[1]).to(dt)).sum()).backward()
        res['d_part'], res['d_feat'] = part_src.grad.numpy(), feats.grad.numpy()
    return res


def pool_fixture(name, s, out, with_scene):
    r = np.random.default_rng(out)
    arrays = dict(s) if with_scene else {}
    arrays['meta'] = np.array([out, MPV, THRESH], np.float64)
    for tag, disable in (("", False), ("nopart_", True)):
        rows = pool_case(s, out, disable, torch.float64)['coords'].shape[0]
        g = (r.normal(0, 1, (rows, 4)), r.normal(0, 1, (rows, C)))
        f64 = pool_case(s, out, disable, torch.float64, g)
        f32 = pool_case(s, out, disable, torch.float32)
        assert (f64['coords'] == f32['coords']).all()
        keep = {"coords": f64['coords'], "part_rows_f64": f64['part_rows'], "part_rows_f32": f32['part_rows'],
                "g_part_rows": g[0], "d_part_f64": f64['d_part']}
        if not disable:                                        # (the max pooling does not depend on DISABLE_PART)
            keep.update({"rpn_rows_f64": f64['rpn_rows'], "rpn_rows_f32": f32['rpn_rows'], "g_rpn_rows": g[1],
                         "d_feat_f64": f64['d_feat']})
        arrays.update({tag + k: v for k, v in keep.items()})
        print(f"{name} {tag or 'part'}: {rows} rows, |f32 - f64| part {np.abs(f32['part_rows'] - f64['part_rows']).max():.2e}")
    save(name, **arrays)


# ---------------------------------------------------------------------------------------------------------------------
def targets_for(r, s):
    """a given targets dict (the seven keys of ProposalTargetLayer): RoIs as they are, GT rows = jittered RoIs"""
    rois = s['rois']
    gt = np.zeros((B, N, 8), F)
    gt[:, :, :7] = rois
    gt[:, :, 0:3] += r.uniform(-0.3, 0.3, (B, N, 3))
    gt[:, :, 3:6] *= 1 + r.uniform(-0.1, 0.1, (B, N, 3))
    gt[:, :, 6] += r.uniform(-0.3, 0.3, (B, N))
    gt[:, :, 7] = r.integers(1, 4, (B, N))
    valid = (r.random((B, N)) < 0.6).astype(np.int64)
    valid[:, [5, 7]] = 0
    valid[:, 0] = 1
    labels = r.uniform(0, 1, (B, N)).astype(F)
    return dict(rois=rois.copy(), gt_of_rois=gt, gt_iou_of_rois=r.uniform(0, 1, (B, N)).astype(F),
                roi_scores=r.uniform(0, 1, (B, N)).astype(F), roi_labels=r.integers(1, 4, (B, N)).astype(np.int64),
                reg_valid_mask=valid, rcnn_cls_labels=labels)


def build_head(mod, cfg, seed):
    torch.manual_seed(seed)
    head = mod.PartA2FCHead(input_channels=C, model_cfg=cfg, num_class=1)
    g = torch.Generator().manual_seed(seed + 1)
    for m in head.modules():
        if isinstance(m, nn.BatchNorm1d):
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
    with torch.no_grad():                                      # (std 0.001 would leave rcnn_reg at the level of fp32 noise)
        head.reg_layers[-1].weight.normal_(0, 0.05, generator=g)
    return head


FIRST = ('conv_part.0.0.weight', 'conv_rpn.0.0.weight', 'shared_fc_layer.0.weight')


def run_head(mod, cfg, sd, s, td, dt, training):
    head = mod.PartA2FCHead(input_channels=C, model_cfg=cfg, num_class=1)
    head.load_state_dict(sd, strict=True)
    head = head.to(dt)
    head.train(training)
    feats = torch.from_numpy(s['point_features']).to(dt).requires_grad_(training)
    part = torch.from_numpy(s['point_part_offset']).to(dt).requires_grad_(training)
    bd = {'batch_size': B, 'rois': torch.from_numpy(s['rois']).to(dt), 'roi_scores': torch.from_numpy(td['roi_scores']).to(dt),
          'roi_labels': torch.from_numpy(td['roi_labels']), 'point_coords': torch.from_numpy(s['point_coords']).to(dt),
          'point_features': feats, 'point_part_offset': part, 'point_cls_scores': torch.from_numpy(s['point_cls_scores']).to(dt)}
    given = {k: (torch.from_numpy(v).to(dt) if v.dtype.kind == 'f' else torch.from_numpy(v)) for k, v in td.items()}
    head.proposal_target_layer.forward = lambda batch_dict: {k: v.clone() for k, v in given.items()}
    ctx = keep_double() if dt == torch.float64 else contextlib.nullcontext()
    out = {}
    with ctx:
        if not training:
            with torch.no_grad():
                bd = head(bd)
            return dict(batch_cls_preds=bd['batch_cls_preds'].numpy(), batch_box_preds=bd['batch_box_preds'].numpy())
        head(bd)
        f = head.forward_ret_dict
        out['gt_of_rois'] = f['gt_of_rois'].detach().numpy()
        out['gt_of_rois_src'] = f['gt_of_rois_src'].detach().numpy()
        out['rcnn_cls_labels'], out['reg_valid_mask'] = f['rcnn_cls_labels'].numpy(), f['reg_valid_mask'].numpy()
        out['rcnn_cls'], out['rcnn_reg'] = f['rcnn_cls'].detach().numpy(), f['rcnn_reg'].detach().numpy()
        loss, tb = head.get_loss()
        loss.backward()
    out['scalars'] = np.array([float(loss.detach()), tb['rcnn_loss_cls'], tb['rcnn_loss_reg'], tb.get('rcnn_loss_corner', 0.0)], np.float64)
    params = dict(head.named_parameters())
    for k in FIRST:
        out['d_' + k] = params[k].grad.numpy()
    out['d_point_features'] = feats.grad.numpy()
    out['d_point_part_offset'] = part.grad.numpy() if part.grad is not None else np.zeros(tuple(part.shape))
    return out


BIG = tuple('d_' + k for k in FIRST) + ('d_point_features',)


def module_arrays(mod, cfg, sd, s, td, tag="", grads=True):
    """the fp64 results (the large gradient arrays rounded to float32: 6e-8 relative, far below any bar) and, per array, the
    largest deviation of the reference's own fp32 run from them (`dev_...`)"""
    arrays = {}
    res = {}
    for dt, dtag in ((torch.float64, "f64"), (torch.float32, "f32")):
        res[dtag] = {f"train_{k}": v for k, v in run_head(mod, cfg, sd, s, td, dt, True).items()}
        res[dtag].update({f"eval_{k}": v for k, v in run_head(mod, cfg, sd, s, td, dt, False).items()})
        print(f"{tag or 'module '}{dtag}: loss {res[dtag]['train_scalars']}")
    for k, v in res["f64"].items():
        if k[6:] in BIG and not grads:
            continue
        arrays[f"{tag}{k}"] = v.astype(F) if k[6:] in BIG else v
        arrays[f"{tag}dev_{k}"] = np.array(np.abs(res["f32"][k].astype(np.float64) - v).max())
    return arrays


if __name__ == "__main__":
    mod = ref_modules()
    S = make_scene()
    check_scene(S)
    pool_fixture("g50_parta2_pool4", S, 4, True)
    pool_fixture("g51_parta2_pool6", S, 6, False)

    r = np.random.default_rng(52)
    td = targets_for(r, S)
    head = build_head(mod, model_cfg(4), 52)
    sd = {k: v.clone() for k, v in head.state_dict().items()}
    arrays = {f"sd.{k}": v.numpy() for k, v in sd.items()}
    arrays.update({f"td_{k}": v for k, v in td.items()})
    main = module_arrays(mod, model_cfg(4), sd, S, td)
    arrays.update({k: v for k, v in main.items() if not any(k.endswith(b) for b in BIG)})
    save("g52_parta2_module", **arrays)

    # g53: the gradients of the main run, then the edges -- all with g52's state dict
    arrays = {k: v for k, v in main.items() if any(k.endswith(b) for b in BIG)}
    # the fake path: one scoring point per frame -> two rows -> fewer than three.  Cell (0, 0, 0) of every RoI but the padding
    # one holds a point of score 0 (four zero part features: no row), so the rows the fake path makes up carry distinct RPN
    # features and the batch-statistics BatchNorms of the training step see distinct samples
    rE = np.random.default_rng(53)
    roisE = make_scene(seed=53, special=False, npts=(1, 1))['rois']
    pts, sc = [], []
    for b in range(B):
        pts.append([b, *to_world(roisE[b, 3], np.array([1.5, 2.5, 0.5]))])
        sc.append(0.8)
        for k in range(7):
            pts.append([b, *to_world(roisE[b, k], np.array([0.5, 0.5, 0.5]) + rE.uniform(-0.2, 0.2, 3))])
            sc.append(0.0)
    P_E = len(pts)
    E = dict(rois=roisE, point_coords=np.asarray(pts, F), point_cls_scores=np.asarray(sc, F),
             point_features=rE.normal(0, 1, (P_E, C)).astype(F), point_part_offset=rE.uniform(0, 1, (P_E, 3)).astype(F))
    ref = PR.sparse_rows(E['rois'], E['point_coords'], E['point_features'], E['point_part_offset'], E['point_cls_scores'], THRESH, 4, MPV)
    assert ref['fake'] and ref['rows_nonzero'] == 2 and ref['coords'].shape[0] == B * N
    assert (np.abs(ref['rpn_rows']).sum(1) > 0).sum() == 14 and not ref['part_rows'].any()
    cell, box = PR.margins(E['rois'], E['point_coords'], 4)
    assert min(cell, box) >= CELL_MARGIN and PR.zero_box_clearance(E['rois'], E['point_coords']) > 1e-2
    tdE = targets_for(r, E)
    arrays.update({f"fake_{k}": v for k, v in E.items()})
    arrays.update({f"fake_td_{k}": v for k, v in tdE.items()})
    arrays.update(fake_coords=ref['coords'], fake_part_rows_f64=ref['part_rows'], fake_rpn_rows_f64=ref['rpn_rows'])
    arrays.update(module_arrays(mod, model_cfg(4), sd, E, tdE, "fake_", grads=False))
    assert (arrays["fake_train_rcnn_cls_labels"] == -1).all() and (arrays["fake_train_reg_valid_mask"] == -1).all()
    # conditioning of the fake scene's TRAINING forward: features moved by 1e-6 (relative) may move the outputs by at most 20
    # times that, so fp32 rounding of another summation order stays far below the 1e-4 bar
    E2 = dict(E, point_features=(E['point_features'].astype(np.float64) * (1 + 1e-6 * rE.normal(0, 1, E['point_features'].shape))))
    a = run_head(mod, model_cfg(4), sd, E, tdE, torch.float64, True)
    b2 = run_head(mod, model_cfg(4), sd, E2, tdE, torch.float64, True)
    moved = max(np.abs(a[k] - b2[k]).max() for k in ('rcnn_cls', 'rcnn_reg'))
    print(f"fake scene: a 1e-6 perturbation of point_features moves rcnn_cls / rcnn_reg by {moved:.2e}")
    assert moved <= 2e-5
    arrays["fake_sensitivity"] = np.array(moved)
    # DISABLE_PART through the head, on the main scene
    arrays.update(module_arrays(mod, model_cfg(4, True), sd, S, td, "nopart_", grads=False))
    save("g53_parta2_edges", **arrays)
    with open(os.path.join(HERE, "MANIFEST_parta2_head.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
