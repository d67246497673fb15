"""CPU restatement of AnchorHeadTemplate.get_loss (anchor_head_template.py:102-227 with loss_utils.py:10-74, :338-401,
:444-469) in plain torch, in the dtype of its inputs: what the anchor-head tests evaluate in fp64 (checked against the
reference's own fp64 outputs in fixture g21 by tests/test_anchor_head_cpu.py).  Test infrastructure only."""
import numpy as np
import torch


def small_cfg(names, stride=1, sizes=None, thresholds=None):
    sizes = sizes or {"Vehicle": [4.7, 2.1, 1.7], "Pedestrian": [0.91, 0.86, 1.73], "Cyclist": [1.78, 0.84, 1.78]}
    thresholds = thresholds or {"Vehicle": (0.55, 0.4), "Pedestrian": (0.5, 0.35), "Cyclist": (0.5, 0.35)}
    return [dict(class_name=n, anchor_sizes=[sizes[n]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[0],
                 align_center=False, feature_map_stride=stride, matched_threshold=thresholds[n][0],
                 unmatched_threshold=thresholds[n][1]) for n in names]


def head_cfg(names, stride=1, use_dir=True, **over):
    cfg = dict(CLASS_AGNOSTIC=False, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
               ANCHOR_GENERATOR_CONFIG=small_cfg(names, stride),
               TARGET_ASSIGNER_CONFIG=dict(NAME='AxisAlignedTargetAssigner', POS_FRACTION=-1.0, SAMPLE_SIZE=512,
                                           NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False, BOX_CODER='ResidualCoder'),
               LOSS_CONFIG=dict(LOSS_WEIGHTS={'cls_weight': 1.0, 'loc_weight': 2.0, 'dir_weight': 0.2,
                                              'code_weights': [1.0] * 7}))
    if use_dir:
        cfg['USE_DIRECTION_CLASSIFIER'] = True
    cfg.update(over)
    return cfg


def get_loss(cls, box, dirp, labels, targets, anchor_rot, num_class, weights=(1.0, 2.0, 0.2), dir_offset=0.78539,
             num_bins=2, code_weights=None):
    """cls [B, N, num_class], box [B, N, 7], dirp [B, N, bins] or None, labels int [B, N], targets [B, N, 7], anchor_rot [N]
    -> (rpn_loss, cls_loss, loc_loss, dir_loss), differentiable."""
    dt = cls.dtype
    B = cls.shape[0]
    labels = labels.long()
    positives, cared = labels > 0, labels >= 0
    norm = torch.clamp(positives.sum(1, keepdim=True).to(dt), min=1.0)
    cls_w = cared.to(dt) / norm
    reg_w = positives.to(dt) / norm
    lab = torch.where(positives, torch.ones_like(labels), labels) if num_class == 1 else labels
    one_hot = torch.nn.functional.one_hot(lab * cared, num_class + 1)[..., 1:].to(dt)
    p = torch.sigmoid(cls)
    alpha_w = one_hot * 0.25 + (1 - one_hot) * 0.75
    pt = one_hot * (1.0 - p) + (1.0 - one_hot) * p
    bce = torch.clamp(cls, min=0) - cls * one_hot + torch.log1p(torch.exp(-torch.abs(cls)))
    cls_loss = (alpha_w * pt ** 2 * bce * cls_w.unsqueeze(-1)).sum() / B * weights[0]
    tg = targets.to(dt)
    b_in = torch.cat([box[..., :6], torch.sin(box[..., 6:7]) * torch.cos(tg[..., 6:7])], -1)
    b_tg = torch.cat([tg[..., :6], torch.cos(box[..., 6:7]) * torch.sin(tg[..., 6:7])], -1)
    diff = b_in - b_tg
    if code_weights is not None:
        diff = diff * code_weights.to(dt).view(1, 1, -1)
    n = diff.abs()
    beta = 1.0 / 9.0
    sl1 = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    loc_loss = (sl1 * reg_w.unsqueeze(-1)).sum() / B * weights[1]
    dir_loss = torch.zeros((), dtype=dt)
    if dirp is not None:
        rot_gt = tg[..., 6] + anchor_rot.to(dt).view(1, -1)
        v = rot_gt - dir_offset
        off = v - torch.floor(v / (2 * np.pi)) * (2 * np.pi)
        bins = torch.clamp(torch.floor(off / (2 * np.pi / num_bins)).long(), 0, num_bins - 1)
        ce = torch.nn.functional.cross_entropy(dirp.permute(0, 2, 1), bins, reduction='none')
        dir_loss = (ce * reg_w).sum() / B * weights[2]
    return cls_loss + loc_loss + dir_loss, cls_loss, loc_loss, dir_loss
