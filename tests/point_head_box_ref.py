"""fp64 restatements of what PointHeadBox / PointIntraPartOffsetHead compute above the point-in-box test: the box labels
(PointResidualCoder.encode_torch, box_coder_utils.py:153-187), the part labels (point_head_template.py:114-122), the three
losses (point_head_template.py:131-191 with loss_utils.py:41-74, :338-399) and the decoding (box_coder_utils.py:189-222).
The point-in-box decision itself is the transcription of tests/point_head_ref.py.  Used by
tests/golden/make_golden_point_head_box.py (where the reference's own classes produce the fp32 values these are compared
with) and by the tests.  Test infrastructure only."""
import numpy as np
import torch

try:
    from tests import point_head_ref as PR
except ImportError:                                   # run from tests/golden/ with tests/ on sys.path
    import point_head_ref as PR

KITTI_MEAN_SIZE = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
EXTRA_WIDTH = [0.2, 0.2, 0.2]
CODE_WEIGHTS = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 0.5]       # not all ones (g48)
LOSS_WEIGHTS = dict(point_cls_weight=1.5, point_box_weight=0.7, point_part_weight=2.5)


def head_cfg(name, box=True, part=False, use_mean_size=True, cls_fc=(32,), reg_fc=(32,), part_fc=(32,), **over):
    """a model_cfg (plain dicts) of PointHeadBox / PointIntraPartOffsetHead the way tools/cfgs writes it"""
    target = dict(GT_EXTRA_WIDTH=list(EXTRA_WIDTH))
    weights = dict(point_cls_weight=LOSS_WEIGHTS['point_cls_weight'])
    c = dict(NAME=name, CLS_FC=list(cls_fc), CLASS_AGNOSTIC=False, USE_POINT_FEATURES_BEFORE_FUSION=False)
    if box:
        target.update(BOX_CODER='PointResidualCoder', BOX_CODER_CONFIG=dict(use_mean_size=use_mean_size, mean_size=KITTI_MEAN_SIZE))
        weights.update(point_box_weight=LOSS_WEIGHTS['point_box_weight'], code_weights=list(CODE_WEIGHTS))
        c['REG_FC'] = list(reg_fc)
    if part:
        weights.update(point_part_weight=LOSS_WEIGHTS['point_part_weight'])
        c['PART_FC'] = list(part_fc)
    c.update(TARGET_CONFIG=target, LOSS_CONFIG=dict(LOSS_REG='WeightedSmoothL1Loss', LOSS_WEIGHTS=weights))
    c.update(over)
    return c


def winning_boxes(point_coords, gt_boxes):
    """(N,) int: the row of the first GT box of its frame that contains the point (-1: none, or a bs_idx that names no
    frame) -- the transcription of points_in_boxes_gpu"""
    pc, gt = np.asarray(point_coords, np.float32), np.asarray(gt_boxes, np.float32)
    win = -np.ones(pc.shape[0], np.int64)
    for k in range(gt.shape[0]):
        m = pc[:, 0] == k
        if m.any() and gt.shape[1]:
            win[m] = PR.points_in_boxes_gpu(gt[k:k + 1, :, :7], pc[m][None, :, 1:4])[0]
    return win


def box_labels_f64(point_coords, gt_boxes, win, mean_size=None):
    """encode_torch in float64 from the float32 inputs: (N, 8), zeros where win < 0"""
    pc, gt = np.asarray(point_coords, np.float64), np.asarray(gt_boxes, np.float64)
    out = np.zeros((pc.shape[0], 8))
    fg = np.nonzero(win >= 0)[0]
    g = gt[pc[fg, 0].astype(np.int64), win[fg]]
    p = pc[fg, 1:4]
    size = np.maximum(g[:, 3:6], 1e-5)
    if mean_size is not None:
        ms = np.asarray(np.asarray(mean_size, np.float32), np.float64)          # the table is float32 in the reference too
        a = ms[g[:, 7].astype(np.int64) - 1]
        diagonal = np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2)
        out[fg, 0] = (g[:, 0] - p[:, 0]) / diagonal
        out[fg, 1] = (g[:, 1] - p[:, 1]) / diagonal
        out[fg, 2] = (g[:, 2] - p[:, 2]) / a[:, 2]
        out[fg, 3:6] = np.log(size / a)
    else:
        out[fg, 0:3] = g[:, 0:3] - p
        out[fg, 3:6] = np.log(size)
    out[fg, 6] = np.cos(g[:, 6])
    out[fg, 7] = np.sin(g[:, 6])
    return out


def part_labels_f64(point_coords, gt_boxes, win):
    """(p - centre) rotated by -heading / (dx, dy, dz) + 0.5 in float64: (N, 3), zeros where win < 0"""
    pc, gt = np.asarray(point_coords, np.float64), np.asarray(gt_boxes, np.float64)
    out = np.zeros((pc.shape[0], 3))
    fg = np.nonzero(win >= 0)[0]
    g = gt[pc[fg, 0].astype(np.int64), win[fg]]
    s = pc[fg, 1:4] - g[:, 0:3]
    cosa, sina = np.cos(-g[:, 6]), np.sin(-g[:, 6])                               # rotate_points_along_z(points, -heading)
    out[fg, 0] = (s[:, 0] * cosa - s[:, 1] * sina) / g[:, 3] + 0.5
    out[fg, 1] = (s[:, 0] * sina + s[:, 1] * cosa) / g[:, 4] + 0.5
    out[fg, 2] = s[:, 2] / g[:, 5] + 0.5
    return out


def full_loss(cls_preds, labels, num_class, weights, box_preds=None, box_labels=None, code_weights=None, part_preds=None,
              part_labels=None):
    """the three losses in plain torch in the dtype of cls_preds, differentiable: (total, cls, box, part); the part term in
    the stable logit form = F.binary_cross_entropy(sigmoid(p), t) in exact arithmetic"""
    dt = cls_preds.dtype
    labels = labels.long()
    pos = (labels > 0).to(dt)
    norm = torch.clamp(pos.sum(), min=1.0)
    l_cls = PR.cls_layer_loss(cls_preds, labels, num_class, weights['point_cls_weight'])
    l_box = l_part = torch.zeros((), dtype=dt, device=cls_preds.device)
    if box_preds is not None:
        target = torch.where(torch.isnan(box_labels.to(dt)), box_preds.detach(), box_labels.to(dt))
        diff = (box_preds - target) * torch.as_tensor(code_weights, dtype=dt, device=cls_preds.device).view(1, -1)
        n = diff.abs()
        beta = 1.0 / 9.0
        el = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
        l_box = (el * (pos / norm).unsqueeze(-1)).sum() * weights['point_box_weight']
    if part_preds is not None:
        t = part_labels.to(dt)
        sp = torch.nn.functional.softplus
        el = t * torch.clamp(sp(-part_preds), max=100.0) + (1 - t) * torch.clamp(sp(part_preds), max=100.0)
        l_part = (el.sum(dim=-1) * pos).sum() / (3 * norm) * weights['point_part_weight']
    return l_cls + l_box + l_part, l_cls, l_box, l_part


def decode_f64(box_encodings, points, classes, mean_size=None):
    """decode_torch in float64: (N, 7); classes (N,) in [1, K]"""
    t, p = np.asarray(box_encodings, np.float64), np.asarray(points, np.float64)
    out = np.zeros((t.shape[0], 7))
    if mean_size is not None:
        a = np.asarray(np.asarray(mean_size, np.float32), np.float64)[np.asarray(classes, np.int64) - 1]
        diagonal = np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2)
        out[:, 0] = t[:, 0] * diagonal + p[:, 0]
        out[:, 1] = t[:, 1] * diagonal + p[:, 1]
        out[:, 2] = t[:, 2] * a[:, 2] + p[:, 2]
        out[:, 3:6] = np.exp(t[:, 3:6]) * a
    else:
        out[:, 0:3] = t[:, 0:3] + p
        out[:, 3:6] = np.exp(t[:, 3:6])
    out[:, 6] = np.arctan2(t[:, 7], t[:, 6])
    return out


def heading_difference(a, b):
    """|a - b| modulo 2 pi"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)
