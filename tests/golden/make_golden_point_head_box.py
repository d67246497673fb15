#!/usr/bin/env python3
"""Generate the PointHeadBox / PointIntraPartOffsetHead fixtures under tests/golden/ (run once, where the reference lies at
/root/reference; not needed at test time).  In the manner of make_golden_point_head.py, whose stand-in packages and helpers
are imported: the reference's own point_head_box.py, point_intra_part_head.py, point_head_template.py, box_coder_utils.py
and loss_utils.py run on the CPU over the numpy stub of `roiaware_pool3d_cuda`; only arrays (data) are stored.
PointResidualCoder.__init__ and WeightedSmoothL1Loss.__init__ call .cuda(): for the duration of this script
torch.Tensor.cuda returns self.

  g47_point_head_box_targets  on the inputs of g27 (loaded, not copied): PointHeadBox.assign_targets with the three KITTI
                              mean sizes and with use_mean_size False, PointIntraPartOffsetHead.assign_targets with and
                              without BOX_CODER.  Label rows of the foreground points only (the rest is asserted zero), in
                              f32 (the reference) and as an fp64 restatement (tests/point_head_box_ref.py)
  g48_point_head_box_loss     on every second point: the three losses, their total, tb_dict and the three gradients under
                              autograd, f32 and f64; code_weights not all ones, a handful of nan box targets, three
                              different weights.  CONDITION: part logits ~ N(0, 2) clipped to |p| <= 10, where the
                              reference's fp32 sigmoid-then-log agrees with exact arithmetic (asserted against fp64)
  g49_point_head_box_decode   generate_predicted_boxes, num_class 1 and 3, with and without mean sizes, f32 and f64.
                              CONDITIONS: no row with two equal maximal logits; no row with cos < 0 and |sin| < 1e-3 (the
                              atan2 branch cut, where one ulp flips the heading by 2 pi)

Usage: python tests/golden/make_golden_point_head_box.py
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden_point_head as G  # noqa: E402
import point_head_box_ref as BR  # noqa: E402

BAR = 1e-4


def to_cfg(d):
    return G.D({k: to_cfg(v) if isinstance(v, dict) and k != 'LOSS_WEIGHTS' else v for k, v in d.items()})


def heads():
    G.ref_modules()
    imp = importlib.import_module
    return imp("pcdet.models.dense_heads.point_head_box").PointHeadBox, \
        imp("pcdet.models.dense_heads.point_intra_part_head").PointIntraPartOffsetHead


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max())


def g47(Box, Part):
    g = dict(np.load(os.path.join(HERE, "g27_point_head_targets.npz")))
    pc, gt = g["point_coords"], g["gt_boxes"]
    inp = {'point_coords': torch.from_numpy(pc), 'gt_boxes': torch.from_numpy(gt)}
    gt_before = gt.copy()
    win = BR.winning_boxes(pc, gt)
    out = {}
    runs = {
        "box": Box(3, 8, to_cfg(BR.head_cfg('PointHeadBox'))),
        "box_c1": Box(1, 8, to_cfg(BR.head_cfg('PointHeadBox'))),
        "box_nomean": Box(3, 8, to_cfg(BR.head_cfg('PointHeadBox', use_mean_size=False))),
        "part": Part(3, 8, to_cfg(BR.head_cfg('PointIntraPartOffsetHead', box=False, part=True))),
        "both": Part(3, 8, to_cfg(BR.head_cfg('PointIntraPartOffsetHead', box=True, part=True))),
    }
    td = {k: h.assign_targets(inp) for k, h in runs.items()}
    assert np.array_equal(gt, gt_before)
    for k, t in td.items():
        labels = t['point_cls_labels'].numpy()
        assert np.array_equal(labels, g["labels_c1" if k == "box_c1" else "labels_c3"].astype(np.int64)), k     # g27's labels
        assert np.array_equal(labels > 0, win >= 0)
    fg = np.nonzero(win >= 0)[0]
    rest = np.nonzero(win < 0)[0]
    out["fg_idx"] = fg.astype(np.int32)
    assert td["box"]['point_part_labels'] is None and td["part"]['point_box_labels'] is None
    assert torch.equal(td["box"]['point_box_labels'], td["both"]['point_box_labels'])
    assert torch.equal(td["box"]['point_box_labels'], td["box_c1"]['point_box_labels'])      # column 7 picks the mean size
    assert torch.equal(td["part"]['point_part_labels'], td["both"]['point_part_labels'])
    for tag, arr, f64 in (("box_mean", td["box"]['point_box_labels'], BR.box_labels_f64(pc, gt, win, BR.KITTI_MEAN_SIZE)),
                          ("box_nomean", td["box_nomean"]['point_box_labels'], BR.box_labels_f64(pc, gt, win, None)),
                          ("part", td["part"]['point_part_labels'], BR.part_labels_f64(pc, gt, win))):
        arr = arr.numpy()
        assert arr.dtype == np.float32 and (arr[rest] == 0).all() and (f64[rest] == 0).all()
        err = rel(arr, f64)
        print(f"g47 {tag}: {fg.size} foreground rows, the reference's f32 within {err:.2e} of the fp64 restatement")
        assert err < BAR
        out[f"{tag}_f32"] = arr[fg]
        out[f"{tag}_f64"] = f64[fg]
    out["mean_size"] = np.asarray(BR.KITTI_MEAN_SIZE, np.float64)
    G.save("g47_point_head_box_targets", **out)
    return g, td


def g48(Box, Part, g, td):
    r = np.random.default_rng(48)
    labels = td["both"]['point_cls_labels'].numpy()[::2].copy()
    box_labels = td["both"]['point_box_labels'].numpy()[::2].copy()
    part_labels = td["both"]['point_part_labels'].numpy()[::2].copy()
    n = labels.shape[0]
    pos = np.nonzero(labels > 0)[0]
    nan_rows = r.choice(pos, 9, replace=False)
    nan_cols = r.integers(0, 8, 9)
    box_labels[nan_rows, nan_cols] = np.nan                                       # a handful of nan box targets
    cls = r.normal(0, 2.0, (n, 3)).astype(np.float32)
    box = (box_labels_guess(box_labels) + r.normal(0, 0.3, (n, 8))).astype(np.float32)
    part = np.clip(r.normal(0, 2.0, (n, 3)), -10, 10).astype(np.float32)          # the condition of this fixture
    out = dict(labels=labels.astype(np.int8), pos_idx=pos.astype(np.int32), box_labels_pos=box_labels[pos],
               part_labels_pos=part_labels[pos], cls_preds=cls, box_preds=box, part_preds=part,
               code_weights=np.asarray(BR.CODE_WEIGHTS, np.float64),
               weights=np.asarray([BR.LOSS_WEIGHTS[k] for k in ('point_cls_weight', 'point_box_weight', 'point_part_weight')]))
    assert (box_labels[labels <= 0] == 0).all() and (part_labels[labels <= 0] == 0).all()
    both = Part(3, 8, to_cfg(BR.head_cfg('PointIntraPartOffsetHead', box=True, part=True)))
    only_box = Box(3, 8, to_cfg(BR.head_cfg('PointHeadBox')))
    only_part = Part(3, 8, to_cfg(BR.head_cfg('PointIntraPartOffsetHead', box=False, part=True)))
    res = {}
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        x = [torch.from_numpy(a).to(dt).requires_grad_(True) for a in (cls, box, part)]
        frd = {'point_cls_labels': torch.from_numpy(labels), 'point_cls_preds': x[0], 'point_box_preds': x[1],
               'point_part_preds': x[2], 'point_box_labels': torch.from_numpy(box_labels).to(dt),
               'point_part_labels': torch.from_numpy(part_labels).to(dt)}
        both.forward_ret_dict = frd
        loss, tb = both.get_loss()
        loss.backward()
        assert set(tb) == {'point_loss_cls', 'point_pos_num', 'point_loss_part', 'point_loss_box'}
        scal = np.array([float(loss.detach()), tb['point_loss_cls'], tb['point_loss_box'], tb['point_loss_part'], tb['point_pos_num']], np.float64)
        grads = [t.grad.numpy().copy() for t in x]
        assert (grads[1][labels <= 0] == 0).all() and (grads[2][labels <= 0] == 0).all() and (grads[0][labels < 0] == 0).all()
        assert (grads[1][nan_rows, nan_cols] == 0).all()
        # the two-branch heads give the same terms
        only_box.forward_ret_dict = frd
        lb, tbb = only_box.get_loss()
        only_part.forward_ret_dict = frd
        lp, tbp = only_part.get_loss()
        assert abs(float(lb.detach()) - (scal[1] + scal[2])) <= 1e-6 * abs(scal[0]) and set(tbb) == {'point_loss_cls', 'point_pos_num', 'point_loss_box'}
        assert abs(float(lp.detach()) - (scal[1] + scal[3])) <= 1e-6 * abs(scal[0]) and set(tbp) == {'point_loss_cls', 'point_pos_num', 'point_loss_part'}
        # ... and the restatement of tests/point_head_box_ref.py (the part term from the logit) agrees
        ours = BR.full_loss(x[0].detach(), torch.from_numpy(labels), 3, BR.LOSS_WEIGHTS, x[1].detach(), frd['point_box_labels'],
                            BR.CODE_WEIGHTS, x[2].detach(), frd['point_part_labels'])
        tol = 1e-5 if dt == torch.float32 else 1e-6     # (the reference keeps its 1 / num_pos weights in float32 either way)
        assert all(abs(float(a) - b) <= tol * abs(b) for a, b in zip(ours, scal[:4])), (tag, [float(a) - b for a, b in zip(ours, scal[:4])])
        res[tag] = (scal, grads)
        out[f"{tag}_scalars"] = scal
        for name, gr in zip(("dcls", "dbox", "dpart"), grads):
            out[f"{tag}_{name}"] = gr
    s32, g32 = res["f32"]
    s64, g64 = res["f64"]
    for k, name in enumerate(("total", "cls", "box", "part")):
        e = abs(s32[k] - s64[k]) / abs(s64[k])
        print(f"g48 {name}: {s64[k]:.6f}, the reference's f32 within {e:.2e} relative")
        assert e < BAR                                                            # the bar the tests hold both to
    for name, a, b in zip(("dcls", "dbox", "dpart"), g32, g64):
        e = np.abs(a - b).max() / np.abs(b).max()
        print(f"g48 {name}: the reference's f32 within {e:.2e} of the largest element")
        assert e < BAR
    assert np.abs(part).max() <= 10.0
    print(f"g48: {pos.size} positives of {n}, {int((labels < 0).sum())} ignored")
    G.save("g48_point_head_box_loss", **out)


def box_labels_guess(box_labels):
    """predictions near the targets (zeros where the target is nan), so that both sides of smooth-L1's beta are met"""
    return np.where(np.isnan(box_labels), 0.0, box_labels)


def g49(Box):
    r = np.random.default_rng(49)
    n = 1000
    pts = np.concatenate([r.uniform(-40, 40, (n, 2)), r.uniform(-2, 2, (n, 1))], 1).astype(np.float32)
    cls3 = r.normal(0, 2.0, (n, 3)).astype(np.float32)
    ang = r.uniform(-np.pi, np.pi, n)
    scale = r.uniform(0.5, 1.5, n)
    enc = np.concatenate([r.normal(0, 0.5, (n, 3)), r.normal(0, 0.3, (n, 3)), (scale * np.cos(ang))[:, None],
                          (scale * np.sin(ang))[:, None]], 1).astype(np.float32)
    top = np.sort(cls3, 1)
    assert (top[:, 2] > top[:, 1]).all(), "a row with two equal maximal logits"
    assert not ((enc[:, 6] < 0) & (np.abs(enc[:, 7]) < 1e-3)).any(), "a row on the atan2 branch cut"
    out = dict(points=pts, cls_preds=cls3, box_preds=enc, mean_size=np.asarray(BR.KITTI_MEAN_SIZE, np.float64))
    for num_class in (1, 3):
        for mean in (True, False):
            head = Box(num_class, 8, to_cfg(BR.head_cfg('PointHeadBox', use_mean_size=mean)))
            tag = f"c{num_class}_{'mean' if mean else 'nomean'}"
            classes = cls3[:, :num_class].argmax(1) + 1
            want = BR.decode_f64(enc, pts, classes, BR.KITTI_MEAN_SIZE if mean else None)
            for dt, t in ((torch.float32, "f32"), (torch.float64, "f64")):
                c, b = head.generate_predicted_boxes(torch.from_numpy(pts).to(dt), torch.from_numpy(cls3[:, :num_class]).to(dt),
                                                     torch.from_numpy(enc).to(dt))
                b = b.numpy()
                assert b.shape == (n, 7)
                err = max(rel(b[:, :6], want[:, :6]), float(BR.heading_difference(b[:, 6], want[:, 6]).max()))
                assert err < (BAR if dt == torch.float32 else 1e-6), (tag, t, err)       # (its diagonal stays float32 either way)
                if dt == torch.float32:
                    print(f"g49 {tag}: the reference's f32 within {err:.2e} of fp64")
                out[f"{tag}_{t}"] = b
    G.save("g49_point_head_box_decode", **out)


if __name__ == "__main__":
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        Box, Part = heads()
        g, td = g47(Box, Part)
        g48(Box, Part, g, td)
        g49(Box)
    finally:
        torch.Tensor.cuda = cuda
    with open(os.path.join(HERE, "MANIFEST_point_head_box.json"), "w") as f:
        json.dump(G.manifest, f, indent=1, sort_keys=True)
