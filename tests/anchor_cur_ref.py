"""CPU restatement of AnchorHeadCurriculum.get_loss with CurriculumSigmoidFocalClassificationLoss
(anchor_head_curriculum.py:103-256, loss_utils.py:79-331) for one class, in plain torch and in the dtype of its inputs:
what the anchor-curriculum tests evaluate in fp64 (checked against the reference's own fp64 outputs in fixture g25 by
tests/test_anchor_curriculum_cpu.py).  Test infrastructure only."""
import math

import numpy as np
import torch

from tests import anchor_ref as AR

NUM_GROUPS = 96


def head_cfg(names, curriculum, stride=1, **over):
    return AR.head_cfg(names, stride, LOSS_CURRICULUM=dict(curriculum), **over)


def get_loss(cls, box, dirp, labels, targets, anchor_rot, cw, weights=(1.0, 2.0, 0.2), dir_offset=0.78539, num_bins=2):
    """AR.get_loss for num_class == 1 with the anchor weight cw [B, N] on the three terms."""
    dt = cls.dtype
    B = cls.shape[0]
    labels = labels.long()
    positives, cared = labels > 0, labels >= 0
    # the reference normalises the classification and regression weights in float32 whatever the dtype of the predictions
    # (`positives.float()`, anchor_head_curriculum.py:122-131, :201-203), the direction weights in their dtype (:238-239)
    norm = torch.clamp(positives.sum(1, keepdim=True).float(), min=1.0)
    cls_w = (cared.float() / norm).to(dt) * cw
    reg_w = (positives.float() / norm).to(dt) * cw
    dir_w = positives.to(dt) / torch.clamp(positives.sum(1, keepdim=True).to(dt), min=1.0) * cw
    one_hot = positives.to(dt).unsqueeze(-1)
    p = torch.sigmoid(cls)
    alpha_w = one_hot * 0.25 + (1 - one_hot) * 0.75
    pt = one_hot * (1.0 - p) + (1.0 - one_hot) * p
    bce = torch.clamp(cls, min=0) - cls * one_hot + torch.log1p(torch.exp(-torch.abs(cls)))
    cls_loss = (alpha_w * pt ** 2 * bce * cls_w.unsqueeze(-1)).sum() / B * weights[0]
    tg = targets.to(dt)
    b_in = torch.cat([box[..., :6], torch.sin(box[..., 6:7]) * torch.cos(tg[..., 6:7])], -1)
    b_tg = torch.cat([tg[..., :6], torch.cos(box[..., 6:7]) * torch.sin(tg[..., 6:7])], -1)
    n = (b_in - b_tg).abs()
    beta = 1.0 / 9.0
    sl1 = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    loc_loss = (sl1 * reg_w.unsqueeze(-1)).sum() / B * weights[1]
    v = tg[..., 6] + anchor_rot.to(dt).view(1, -1) - dir_offset
    off = v - torch.floor(v / (2 * np.pi)) * (2 * np.pi)
    bins = torch.clamp(torch.floor(off / (2 * np.pi / num_bins)).long(), 0, num_bins - 1)
    ce = torch.nn.functional.cross_entropy(dirp.permute(0, 2, 1), bins, reduction='none')
    dir_loss = (ce * dir_w).sum() / B * weights[2]
    return cls_loss + loc_loss + dir_loss, cls_loss, loc_loss, dir_loss


class CurriculumLossRef:
    """the loss object's state (mean / std of class 0) and one step of it"""

    def __init__(self, curriculum, alpha=0.25):
        self.cur, self.alpha = dict(curriculum), alpha
        self.mean = self.std = None
        cdf = 0.5 * (1.0 + math.erf(self.cur.get('OFFSET', 0) / math.sqrt(2.0)))
        self.pos_norm, self.neg_norm = 0.5 / (1.0 - cdf) * self.cur.get('POSW', 1), 0.5 / cdf

    def weight(self, p, positives, grouped, epoch):
        g = self.cur.get
        w = torch.ones_like(p)
        if not g('UCL', True):
            return w
        one = lambda v: v[0] if type(v) is list else v
        if self.mean is None:
            thr, var = 0.5, 0.2
        else:
            thr, var = self.mean + g('OFFSET', 0) * self.std, self.std
        if g('NORM', False) is False:
            var = 1
        h, end = one(g('HEIGHT', 1)), one(g('END', 30))
        height = h * ((end - epoch) if g('INV', False) else max(end - epoch, 0)) / (end - g('START', 0))
        if g('FIXED', False):
            height = h
        if epoch > g('CUT', 10000):
            height = 0
        smt, gate = g('SMT', 0.15), epoch >= g('SME', 20)
        if g('SM', False):
            mask = (grouped if g('OTO', False) else positives) & (p <= smt)
            return torch.where(mask & gate, torch.full_like(p, 0.5), w)
        if g('SMA', False):
            mask = positives & ~grouped & (p <= smt)
            return torch.where(mask & gate, torch.full_like(p, 0.5), w)
        mask = grouped if g('OTO', False) else positives
        v = height / (1 + torch.exp(one(g('ELONGATION', -10)) * (p - thr) / var)) + 1 - height / 2
        v = v * torch.where(p > thr, torch.full_like(p, self.pos_norm), torch.full_like(p, self.neg_norm))
        return torch.where(mask, v, w)

    def step(self, cls, box, dirp, labels, targets, groups, anchor_rot, epoch, **kw):
        """cls [B, N, 1], box [B, N, 7], dirp [B, N, bins], labels / groups int [B, N] -> (losses, weight [B, N],
        conf_sum [96], conf_num [96])"""
        p = torch.sigmoid(cls.detach())[..., 0]
        positives = labels > 0
        grouped = positives & (groups > 0)
        if self.cur.get('UCL', True) and bool(grouped.any()):
            s = p[grouped]
            n = s.numel()
            mean = s.sum() / n
            v = (s ** 2).sum() + n * mean ** 2 - 2 * mean * s.sum()
            std = torch.sqrt(v / n) if v > 0 else torch.zeros_like(v)
            mean, std = float(mean), float(std)
            if self.mean is None:
                self.mean, self.std = mean, std
            else:
                self.mean = (1 - self.alpha) * self.mean + self.alpha * mean
                self.std = (1 - self.alpha) * self.std + self.alpha * std
        w = self.weight(p, positives, grouped, epoch)
        idx = (groups[grouped] - 1).long()
        conf_sum = torch.zeros(NUM_GROUPS, dtype=p.dtype).index_add_(0, idx, p[grouped])
        conf_num = torch.zeros(NUM_GROUPS, dtype=p.dtype).index_add_(0, idx, torch.ones_like(p[grouped]))
        return get_loss(cls, box, dirp, labels, targets, anchor_rot, w, **kw), w, conf_sum, conf_num


# the option sets of fixture g25 (tests/golden/make_golden_anchor_curriculum.py: OPTION_SETS)
OPTION_SETS = {
    "off": dict(UCL=False),
    "sig": dict(UCL=True, OFFSET=0.5, NORM=True, INV=True, HEIGHT=1.0, START=0, END=30, ELONGATION=-10, POSW=1.5),
    "oto": dict(UCL=True, OTO=True, HEIGHT=0.8, END=30),
    "sm": dict(UCL=True, SM=True, SME=20, SMT=0.3),
    "sma": dict(UCL=True, SMA=True, SME=0, SMT=0.4),
    "cut": dict(UCL=True, CUT=4, OFFSET=-0.2, HEIGHT=1.0, END=30),
    "hlist": dict(UCL=True, HEIGHT=[0.6], END=[20], ELONGATION=[-6.0], OFFSET=0.25),
}
STEPS = 4


def step_tensors(g, s, dtype, bf16=False):
    """(cls [B, N, 1], box [B, N, 7], dir [B, N, 2]) leaves of step s, labels, targets, groups"""
    maps = [torch.from_numpy(g[f"step{s}_{k}"]) for k in ("cls", "box", "dir")]
    if bf16:
        maps = [m.bfloat16() for m in maps]
    B = maps[0].shape[0]
    x = [m.to(dtype).reshape(B, -1, c).requires_grad_(True) for m, c in zip(maps, (1, 7, 2))]
    return x, torch.from_numpy(g["labels"].astype(np.int64)), torch.from_numpy(g["targets"]), \
        torch.from_numpy(g[f"step{s}_groups"].astype(np.int64))
