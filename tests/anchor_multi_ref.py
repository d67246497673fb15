"""CPU restatement of AnchorHeadMulti.get_loss (anchor_head_multi.py:245-373 with loss_utils.py:10-74, :338-441, :444-469)
in plain torch, in the dtype of its inputs: what the multi-head tests evaluate in fp64 (checked against the reference's own
fp64 outputs in fixture g39 by tests/test_anchor_multi_cpu.py) -- and the two small configurations (case N: nuScenes form,
case K: KITTI form) the fixtures g38-g42 were made with.  Test infrastructure only."""
import numpy as np
import torch

RANGE = [0.0, -7.6, -2.0, 18.4, 7.6, 4.0]      # 24 x 20 cells of 0.8 m: H * W = 480 is no multiple of 256
GRID = [24, 20, 1]
IN_CHANNELS = 8
SIZES = {"car": [4.7, 2.1, 1.7], "truck": [6.9, 2.5, 2.8], "bus": [10.5, 2.9, 3.5], "pedestrian": [0.91, 0.86, 1.73],
         "cyclist": [1.78, 0.84, 1.78]}
THRESH = {"car": (0.6, 0.45), "truck": (0.55, 0.4), "bus": (0.5, 0.35), "pedestrian": (0.5, 0.35), "cyclist": (0.5, 0.35)}
BOTTOM = {"car": -1.0, "truck": -0.6, "bus": -0.3, "pedestrian": -0.9, "cyclist": -0.9}
CASES = {"N": dict(names=["car", "truck", "bus", "pedestrian"], heads=[["car"], ["truck", "bus"], ["pedestrian"]], code_gt=9),
         "K": dict(names=["car", "pedestrian", "cyclist"], heads=[["car"], ["pedestrian"], ["cyclist"]], code_gt=7)}
POST_PROCESSING = dict(SCORE_THRESH=0.3, OUTPUT_RAW_SCORE=False, RECALL_THRESH_LIST=[0.5],
                       NMS_CONFIG=dict(MULTI_CLASSES_NMS=True, NMS_TYPE='nms_gpu', NMS_THRESH=0.2, NMS_PRE_MAXSIZE=30,
                                       NMS_POST_MAXSIZE=10))


def anchor_cfgs(names):
    return [dict(class_name=n, anchor_sizes=[SIZES[n]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[BOTTOM[n]],
                 align_center=False, feature_map_stride=1, matched_threshold=THRESH[n][0], unmatched_threshold=THRESH[n][1])
            for n in names]


def model_cfg(case, **over):
    """the DENSE_HEAD block of case "N" / "K" as plain dicts"""
    c = CASES[case]
    cfg = dict(NAME='AnchorHeadMulti', CLASS_AGNOSTIC=False, USE_MULTIHEAD=True, SEPARATE_MULTIHEAD=True,
               ANCHOR_GENERATOR_CONFIG=anchor_cfgs(c["names"]), RPN_HEAD_CFGS=[dict(HEAD_CLS_NAME=h) for h in c["heads"]],
               TARGET_ASSIGNER_CONFIG=dict(NAME='AxisAlignedTargetAssigner', POS_FRACTION=-1.0, SAMPLE_SIZE=512,
                                           NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False, BOX_CODER='ResidualCoder'))
    if case == "N":
        cfg.update(DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2, SHARED_CONV_NUM_FILTER=16,
                   SEPARATE_REG_CONFIG=dict(NUM_MIDDLE_CONV=1, NUM_MIDDLE_FILTER=16,
                                            REG_LIST=['reg:2', 'height:1', 'size:3', 'angle:2', 'velo:2']),
                   LOSS_CONFIG=dict(REG_LOSS_TYPE='WeightedL1Loss',
                                    LOSS_WEIGHTS={'pos_cls_weight': 1.0, 'neg_cls_weight': 2.0, 'cls_weight': 1.0,
                                                  'loc_weight': 0.25, 'dir_weight': 0.2, 'code_weights': [1.0] * 8 + [0.2, 0.2]}))
        cfg['TARGET_ASSIGNER_CONFIG']['BOX_CODER_CONFIG'] = {'code_size': 9, 'encode_angle_by_sincos': True}
    else:
        cfg.update(USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
                   LOSS_CONFIG=dict(LOSS_WEIGHTS={'cls_weight': 1.0, 'loc_weight': 2.0, 'dir_weight': 0.2,
                                                  'code_weights': [1.0] * 7}))
    cfg.update(over)
    return cfg


def head_layout(case):
    """(kind0, n_kinds, class0, num_class) per head: two rotations of one size per class"""
    out, k, c = [], 0, 0
    for h in CASES[case]["heads"]:
        out.append((k, 2 * len(h), c, len(h)))
        k, c = k + 2 * len(h), c + len(h)
    return out


def to_anchor_major(m, n_anchors):
    """a head's [B, A * items, H, W] map -> [B, A * H * W, items]: the reference's view(-1, A, items, H, W) + permute"""
    B, ch, H, W = m.shape
    return m.reshape(B, n_anchors, ch // n_anchors, H, W).permute(0, 1, 3, 4, 2).reshape(B, n_anchors * H * W, ch // n_anchors)


def get_loss(cls_maps, box_maps, dir_maps, labels, targets, anchor_rot, layout, num_class, reg_l1, pos_w=1.0, neg_w=1.0,
             weights=(1.0, 2.0, 0.2), dir_offset=0.78539, num_bins=2, code_weights=None):
    """cls_maps / box_maps / dir_maps (or None): per-head [B, A_h * items, H, W]; labels int [B, N], targets [B, N, code],
    anchor_rot [N] (the multi-head anchor order) -> (rpn_loss, cls_loss, loc_loss, dir_loss), differentiable."""
    dt = cls_maps[0].dtype
    B = cls_maps[0].shape[0]
    labels = labels.long()
    positives, negatives = labels > 0, labels == 0
    norm = torch.clamp(positives.sum(1, keepdim=True).to(dt), min=1.0)
    cls_w = (negatives.to(dt) * neg_w + positives.to(dt) * pos_w) / norm
    reg_w = positives.to(dt) / norm
    lab = torch.where(positives, torch.ones_like(labels), labels) if num_class == 1 else labels
    one_hot_all = torch.nn.functional.one_hot(torch.clamp(lab, min=0), num_class + 1)[..., 1:].to(dt)
    tg = targets.to(dt)
    cw = torch.ones(tg.shape[-1], dtype=dt) if code_weights is None else code_weights.to(dt)
    cls_loss = loc_loss = dir_loss = torch.zeros((), dtype=dt)
    start = 0
    for h, (kind0, nk, class0, nc) in enumerate(layout):
        cls = to_anchor_major(cls_maps[h], nk)
        box = to_anchor_major(box_maps[h], nk)
        n_h = cls.shape[1]
        sl = slice(start, start + n_h)
        one_hot = one_hot_all[:, sl, class0:class0 + nc]
        p = torch.sigmoid(cls)
        alpha_w = one_hot * 0.25 + (1 - one_hot) * 0.75
        pt = one_hot * (1.0 - p) + (1.0 - one_hot) * p
        bce = torch.clamp(cls, min=0) - cls * one_hot + torch.log1p(torch.exp(-torch.abs(cls)))
        cls_loss = cls_loss + (alpha_w * pt ** 2 * bce * cls_w[:, sl].unsqueeze(-1)).sum() / B * weights[0]
        t_h = tg[:, sl]
        b_in, b_tg = box, t_h
        if dir_maps is not None:
            b_in = torch.cat([box[..., :6], torch.sin(box[..., 6:7]) * torch.cos(t_h[..., 6:7]), box[..., 7:]], -1)
            b_tg = torch.cat([t_h[..., :6], torch.cos(box[..., 6:7]) * torch.sin(t_h[..., 6:7]), t_h[..., 7:]], -1)
        n = ((b_in - b_tg) * cw.view(1, 1, -1)).abs()
        beta = 1.0 / 9.0
        el = n if reg_l1 else torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
        loc_loss = loc_loss + (el * reg_w[:, sl].unsqueeze(-1)).sum() / B * weights[1]
        if dir_maps is not None:
            dirp = to_anchor_major(dir_maps[h], nk)
            v = t_h[..., 6] + anchor_rot.to(dt)[sl].view(1, -1) - dir_offset
            off = v - torch.floor(v / (2 * np.pi)) * (2 * np.pi)
            bins = torch.clamp(torch.floor(off / (2 * np.pi / num_bins)).long(), 0, num_bins - 1)
            ce = torch.nn.functional.cross_entropy(dirp.permute(0, 2, 1), bins, reduction='none')
            dir_loss = dir_loss + (ce * reg_w[:, sl]).sum() / B * weights[2]
        start += n_h
    return cls_loss + loc_loss + dir_loss, cls_loss, loc_loss, dir_loss
