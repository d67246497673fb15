#!/usr/bin/env python3
"""Generate the anchor-curriculum fixtures under tests/golden/ (run once, on a machine that holds the reference where
make_golden_anchor.py expects it; not needed at test time).  In the manner of make_golden_anchor.py, whose helpers it
imports: the reference's own files are imported from their read-only location under stand-in parent packages and run on
the CPU; only arrays are stored.

  g23_anchor_cur_groups   the four `cluster` methods (CurriculumAnchorHeadSingle, _x1, _car, _car_x2) on boxes that hit
                          every distance / length / facade / occupancy bin and every bin edge, in a batch whose class
                          maximum is 1 and one whose class maximum is 3
  g24_anchor_cur_targets  CurriculumAxisAlignedTargetAssigner with groups: the quirk frames of g20 and the full-size case
                          (stored sparsely), a class-agnostic case
  g25_anchor_cur_loss     CurriculumSigmoidFocalClassificationLoss + WeightedSmoothL1Loss + WeightedCrossEntropyLoss driven
                          as AnchorHeadCurriculum.get_loss drives them, four consecutive steps on ONE loss object per
                          option set (step 2 has no grouped positive), fp32 and fp64: scalars, gradients (fp64),
                          confidence_all and the state after every step

Usage: python tests/golden/make_golden_anchor_curriculum.py
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_anchor as MG  # noqa: E402

D = MG.D
VARIANTS = ("base", "x1", "car", "car_x2")


def cur_modules():
    R = MG.ref_modules()
    MG._ns("pcdet.models.dense_heads.target_assigner.atss_target_assigner", None, ATSSTargetAssigner=None)
    mu = sys.modules["pcdet.models.model_utils"]
    mu.model_nms_utils = types.SimpleNamespace()
    imp = importlib.import_module
    R.ahc = imp("pcdet.models.dense_heads.anchor_head_curriculum").AnchorHeadCurriculum
    R.cta = imp("pcdet.models.dense_heads.target_assigner.curri_axis_aligned_target_assigner")
    zoo = imp("pcdet.models.dense_heads.head_zoo")
    R.heads = dict(base=zoo.CurriculumAnchorHeadSingle, x1=zoo.CurriculumAnchorHeadSingle_x1,
                   car=zoo.CurriculumAnchorHeadSingle_car, car_x2=zoo.CurriculumAnchorHeadSingle_car_x2)
    return R


def ref_cluster(R, variant, gt, tru, occ, fac):
    t = [torch.from_numpy(np.ascontiguousarray(a)) for a in (gt, tru, occ, fac)]
    return R.heads[variant].cluster(None, t[0], t[1], t[2], t[3]).numpy()


def g23(R):
    """a full product of representative and edge values of every binned quantity, per class"""
    f32 = np.float32
    dist = [0.0, 10.0, 15.0, np.nextafter(f32(15), f32(16)), 22.0, 30.0, np.nextafter(f32(30), f32(31)), 40.0, 45.0,
            np.nextafter(f32(45), f32(46)), 50.0, np.nextafter(f32(50), f32(51)), 55.0, 60.0, np.nextafter(f32(60), f32(61)), 70.0]
    length = [4.5, 6.0, np.nextafter(f32(6), f32(7)), 9.0]
    facade = [0.0, 1.0, 2.0, 3.0]
    edges = [0.21 * 5 / 12, 0.41 * 5 / 12, 0.61 * 5 / 12, 0.81 * 5 / 12, 0.25, 0.5, 0.7, 0.21, 0.41, 0.61, 0.81]
    occ = [0.0, 0.05, 0.12, 0.2, 0.3, 0.45, 0.55, 0.65, 0.75, 0.9, 1.0]
    for e in edges:
        e32 = f32(e)
        occ += [e32, np.nextafter(e32, f32(0)), np.nextafter(e32, f32(1))]
    rows = []
    r = np.random.default_rng(23)
    for d in dist:
        for ln in length:
            for fa in facade:
                for oc in occ:
                    ang = r.uniform(0, 2 * np.pi)
                    rows.append((d, ang, ln, fa, oc))
    rows = np.array(rows, np.float64)
    n = rows.shape[0]
    out = {}
    for tag, classes in (("max1", [0, 1]), ("max3", [0, 1, 2, 3])):
        B = 4
        M = -(-n * len(classes) // B)
        M += 3
        gt = np.zeros((B * M, 8), f32)
        tru = np.zeros((B * M,), f32)
        occ_a = np.zeros((B * M,), f32)
        fac_a = np.zeros((B * M,), f32)
        k = 0
        for c in classes:
            for d, ang, ln, fa, oc in rows:
                # exact distances on the axes for the edge values: (d, 0) or (0, d)
                gt[k, 0:2] = (d, 0.0) if k % 2 == 0 else (0.0, -d)
                gt[k, 2] = 0.3
                gt[k, 3:6] = (ln, 2.0, 1.6)
                gt[k, 6] = ang
                gt[k, 7] = c
                tru[k] = [1.0, 1.0, 1.0, 2.0, 0.0][k % 5]
                occ_a[k] = oc
                fac_a[k] = fa
                k += 1
        gt, tru, occ_a, fac_a = gt.reshape(B, M, 8), tru.reshape(B, M), occ_a.reshape(B, M), fac_a.reshape(B, M)
        # some boxes off the axes (the distance is a rounded square root)
        extra = r.uniform(-60, 60, (B, 3, 2)).astype(f32)
        gt[:, -3:, 0:2] = extra
        gt[:, -3:, 3:6] = (4.0, 2.0, 1.5)
        gt[:, -3:, 7] = max(classes)
        tru[:, -3:] = 1.0
        occ_a[:, -3:] = r.random((B, 3)).astype(f32)
        fac_a[:, -3:] = r.integers(0, 4, (B, 3)).astype(f32)
        out[f"{tag}_gt_boxes"], out[f"{tag}_true_object"] = gt, tru
        out[f"{tag}_occupancy_ratio"], out[f"{tag}_facade_type"] = occ_a, fac_a
        for v in VARIANTS:
            g = ref_cluster(R, v, gt, tru, occ_a, fac_a)
            assert g.dtype == np.int64 and g.min() >= 0
            out[f"{tag}_{v}"] = g.astype(np.int16)
            print(f"g23 {tag} {v}: {np.unique(g).size} distinct groups, max {g.max()}")
    MG.save("g23_anchor_cur_groups", **out)


def cur_assign(R, names, class_names, rng, grid, stride, gt, group):
    cfgs = MG.anchor_cfgs(names, stride)
    anchors, _ = R.ag.AnchorGenerator(rng, cfgs).generate_anchors([np.array(grid) // stride] * len(names))
    ta = R.cta.CurriculumAxisAlignedTargetAssigner(MG.model_cfg(cfgs), class_names, R.bc.ResidualCoder(), False)
    out = ta.assign_targets(anchors, torch.from_numpy(gt.copy()), group=torch.from_numpy(group.copy()))
    return (out["box_cls_labels"].numpy().astype(np.int32), out["box_reg_targets"].numpy(), out["reg_weights"].numpy(),
            out["groups"].numpy().astype(np.int32))


def frame_extras(r, gt):
    B, M = gt.shape[:2]
    tru = np.where(r.random((B, M)) < 0.75, 1.0, 2.0).astype(np.float32)
    return tru, r.random((B, M)).astype(np.float32), r.integers(0, 4, (B, M)).astype(np.float32)


def g24(R):
    out = {}
    r = np.random.default_rng(24)
    for tag, names, rng, grid, stride, gt in (
            ("full", MG.NAMES, [-75.2, -75.2, -2, 75.2, 75.2, 4], [1504, 1504], 8, MG.full_size_boxes()),
            ("small", MG.NAMES, MG.SMALL_RANGE, MG.SMALL_GRID, 1, MG.quirk_boxes())):
        tru, occ, fac = frame_extras(r, gt)
        group = ref_cluster(R, "x1", gt, tru, occ, fac)
        lab0, tg0, w0, gi, _ = MG.assign_case(R, names, names, rng, grid, stride, gt)
        lab, tg, w, groups = cur_assign(R, names, names, rng, grid, stride, gt, group)
        assert (lab == lab0).all() and (tg == tg0).all() and (w == w0).all()
        # the rule the device applies: positive -> its box's group, label 0 -> 0, ignored -> -1
        rule = np.where(lab > 0, np.take_along_axis(group, np.maximum(gi, 0).astype(np.int64), 1), np.where(lab == 0, 0, -1))
        assert (rule == groups).all()
        print(f"g24 {tag}: positives {(lab > 0).sum(1)}, grouped {(groups > 0).sum(1)}")
        out[f"{tag}_gt_boxes"], out[f"{tag}_true_object"] = gt, tru
        out[f"{tag}_occupancy_ratio"], out[f"{tag}_facade_type"], out[f"{tag}_group"] = occ, fac, group.astype(np.int16)
        MG.sparse_targets(tag, lab, tg, w, gi, out)
        out[f"{tag}_pos_groups"] = groups[lab > 0].astype(np.int16)
        assert (groups[lab == 0] == 0).all() and (groups[lab < 0] == -1).all()
    out["small_range"] = np.array(MG.SMALL_RANGE, np.float64)
    out["small_grid"] = np.array(MG.SMALL_GRID, np.int64)
    gt1 = MG.quirk_boxes()[[0, 3, 2]].copy()
    gt1[gt1[..., 7] != 1] = 0
    tru, occ, fac = frame_extras(r, gt1)
    group = ref_cluster(R, "car", gt1, tru, occ, fac)
    lab0, tg0, w0, gi, _ = MG.assign_case(R, ["Vehicle"], ["Vehicle"], MG.SMALL_RANGE, MG.SMALL_GRID, 1, gt1)
    lab, tg, w, groups = cur_assign(R, ["Vehicle"], ["Vehicle"], MG.SMALL_RANGE, MG.SMALL_GRID, 1, gt1, group)
    assert (lab == lab0).all()
    out["single_gt_boxes"], out["single_true_object"] = gt1, tru
    out["single_occupancy_ratio"], out["single_facade_type"], out["single_group"] = occ, fac, group.astype(np.int16)
    MG.sparse_targets("single", lab, tg, w, gi, out)
    out["single_pos_groups"] = groups[lab > 0].astype(np.int16)
    assert (groups[lab == 0] == 0).all() and (groups[lab < 0] == -1).all()
    MG.save("g24_anchor_cur_targets", **out)


CUR_RANGE = [0.0, -6.4, -2, 19.2, 6.4, 4]            # 24 x 16 cells of 0.8 m
CUR_GRID = [24, 16]
STEPS = 4
UNGROUPED_STEP = 2
# (tag, LOSS_CURRICULUM, epoch of each step)
OPTION_SETS = (
    ("off", dict(UCL=False), [0, 0, 1, 1]),
    ("sig", dict(UCL=True, OFFSET=0.5, NORM=True, INV=True, HEIGHT=1.0, START=0, END=30, ELONGATION=-10, POSW=1.5), [5, 5, 35, 35]),
    ("oto", dict(UCL=True, OTO=True, HEIGHT=0.8, END=30), [3, 3, 3, 4]),
    ("sm", dict(UCL=True, SM=True, SME=20, SMT=0.3), [10, 19, 20, 25]),
    ("sma", dict(UCL=True, SMA=True, SME=0, SMT=0.4), [1, 1, 1, 1]),
    ("cut", dict(UCL=True, CUT=4, OFFSET=-0.2, HEIGHT=1.0, END=30), [6, 6, 6, 6]),
    ("hlist", dict(UCL=True, HEIGHT=[0.6], END=[20], ELONGATION=[-6.0], OFFSET=0.25), [4, 4, 4, 4]),
)


def cur_boxes():
    r = np.random.default_rng(25)
    B, M = 2, 24
    gt = np.zeros((B, M, 8), np.float32)
    size = np.array(MG.SIZES["Vehicle"], np.float32)
    for b, n in ((0, 20), (1, 9)):
        gt[b, :n, 0:2] = np.stack([r.uniform(0, 19.2, n), r.uniform(-6.4, 6.4, n)], 1)
        gt[b, :n, 2] = r.uniform(-1, 1, n)
        gt[b, :n, 3:6] = size * r.uniform(.8, 1.25, (n, 3))
        gt[b, :n, 6] = r.uniform(-2 * np.pi, 2 * np.pi, n)
        gt[b, :n, 7] = 1
    tru = np.where(r.random((B, M)) < 0.7, 1.0, 2.0).astype(np.float32)
    return gt, tru, r.random((B, M)).astype(np.float32), r.integers(0, 4, (B, M)).astype(np.float32)


def g25(R):
    out = {}
    names = ["Vehicle"]
    A = 2
    gt, tru, occ, fac = cur_boxes()
    H, W = CUR_GRID[1], CUR_GRID[0]
    labels, targets, _, gi, all_anchors = MG.assign_case(R, names, names, CUR_RANGE, CUR_GRID, 1, gt)
    B, N = labels.shape
    r = np.random.default_rng(26)
    steps = []
    for s in range(STEPS):
        t = np.zeros_like(tru) if s == UNGROUPED_STEP else tru
        group = ref_cluster(R, "car", gt, t, occ, fac)
        lab, tg, _, groups = cur_assign(R, names, names, CUR_RANGE, CUR_GRID, 1, gt, group)
        assert (lab == labels).all() and (tg == targets).all()
        cls = r.normal(0, 1.6, (B, H, W, A)).astype(np.float32)
        # the positives' scores keep clear of every comparison edge (SMT 0.3 / 0.4, thresholds between 0.4 and 0.75):
        # drawn from [0.04, 0.27], [0.33, 0.37] and [0.78, 0.97]
        npos = int((labels > 0).sum())
        band = r.integers(0, 4, npos)
        score = np.where(band == 0, r.uniform(0.04, 0.27, npos), np.where(band == 1, r.uniform(0.33, 0.37, npos),
                                                                          r.uniform(0.78, 0.97, npos)))
        cls.reshape(-1)[labels.reshape(-1) > 0] = np.log(score / (1 - score)).astype(np.float32)
        box = r.normal(0, 0.4, (B, H, W, A * 7)).astype(np.float32)
        dirp = r.normal(0, 1.5, (B, H, W, A * MG.NUM_DIR_BINS)).astype(np.float32)
        steps.append((t, group, groups, cls, box, dirp))
        out[f"step{s}_true_object"], out[f"step{s}_groups"] = t, groups.astype(np.int8)
        out[f"step{s}_cls"], out[f"step{s}_box"], out[f"step{s}_dir"] = cls, box, dirp
        print(f"g25 step {s}: positives {(labels > 0).sum()}, grouped {(groups > 0).sum()}")
    assert (steps[UNGROUPED_STEP][2] > 0).sum() == 0 and (steps[0][2] > 0).sum() > 0
    out["gt_boxes"], out["occupancy_ratio"], out["facade_type"] = gt, occ, fac
    out["labels"], out["targets"] = labels.astype(np.int8), targets
    out["range"], out["grid"] = np.array(CUR_RANGE, np.float64), np.array(CUR_GRID, np.int64)
    out["dir"] = np.array([MG.DIR_OFFSET, MG.DIR_LIMIT_OFFSET, MG.NUM_DIR_BINS], np.float64)
    lw = MG.LOSS_WEIGHTS
    out["loss_weights"] = np.array([lw["cls_weight"], lw["loc_weight"], lw["dir_weight"]])
    pos = labels.reshape(-1) > 0
    for tag, cur, epochs in OPTION_SETS:
        out[f"{tag}_epochs"] = np.array(epochs, np.int64)
        weighted = 0
        for dt, dtag in ((torch.float32, "f32"), (torch.float64, "f64")):
            torch.set_default_dtype(dt)       # (the loss builds its weight tensor in the default dtype)
            me = types.SimpleNamespace(
                forward_ret_dict={}, num_class=1, use_multihead=False, num_anchors_per_location=A, epoch=0,
                anchors=[torch.from_numpy(all_anchors).to(dt).view(1, H, W, A, 1, 7)],
                model_cfg=D(LOSS_CONFIG=D(LOSS_WEIGHTS=lw), DIR_OFFSET=MG.DIR_OFFSET, NUM_DIR_BINS=MG.NUM_DIR_BINS),
                cls_loss_func=R.lu.CurriculumSigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0,
                                                                           model_config=D(LOSS_CURRICULUM=D(cur))),
                reg_loss_func=R.lu.WeightedSmoothL1Loss(code_weights=lw["code_weights"]),
                dir_loss_func=R.lu.WeightedCrossEntropyLoss(),
                add_sin_difference=R.ahc.add_sin_difference, get_direction_target=R.ahc.get_direction_target)
            me.reg_loss_func.code_weights = me.reg_loss_func.code_weights.to(dt)
            lf = me.cls_loss_func
            if dtag == "f64":
                out[f"{tag}_norms"] = np.array([lf.pos_norm, lf.neg_norm], np.float64)
            for s, (t, group, groups, cls, box, dirp) in enumerate(steps):
                me.epoch = epochs[s]
                x = [torch.from_numpy(a).to(dt).requires_grad_(True) for a in (cls, box, dirp)]
                me.forward_ret_dict = dict(cls_preds=x[0], box_preds=x[1], dir_cls_preds=x[2],
                                           box_cls_labels=torch.from_numpy(labels.copy()),
                                           box_reg_targets=torch.from_numpy(targets).to(dt),
                                           groups=torch.from_numpy(groups.copy()))
                cls_loss, tb, cw = R.ahc.get_cls_layer_loss(me)
                me.forward_ret_dict["box_cls_labels"] = torch.from_numpy(labels.copy())
                box_loss, tb2 = R.ahc.get_box_reg_layer_loss(me, cw.squeeze(-1))
                loss = cls_loss + box_loss
                loss.backward()
                out[f"{tag}_{dtag}_scalars{s}"] = np.array([float(loss), tb["rpn_loss_cls"], tb2["rpn_loss_loc"],
                                                            tb2["rpn_loss_dir"]], np.float64)
                if dtag == "f32":
                    continue
                p = torch.sigmoid(x[0].detach()).reshape(-1).numpy()[pos]
                cwn = cw.detach().reshape(-1).numpy()
                assert (cwn[~pos] == 1).all()
                weighted += int((cwn != 1).sum())
                out[f"{tag}_weights{s}"] = cwn[pos]
                out[f"{tag}_dcls{s}"] = x[0].grad.numpy()
                out[f"{tag}_dbox{s}"] = x[1].grad.numpy().reshape(-1, 7)[pos]
                out[f"{tag}_ddir{s}"] = x[2].grad.numpy().reshape(-1, MG.NUM_DIR_BINS)[pos]
                assert (x[1].grad.numpy().reshape(-1, 7)[~pos] == 0).all() and (x[2].grad.numpy().reshape(-1, 2)[~pos] == 0).all()
                conf = lf.confidence_all
                out[f"{tag}_conf_sum{s}"] = conf[0].numpy().astype(np.float64)
                out[f"{tag}_conf_num{s}"] = conf[1].numpy().astype(np.float64)
                if lf.means is None:
                    state = np.array([np.nan, np.nan])
                else:
                    assert s > 0 or lf.means[0] is not None, "the first UCL step needs a grouped positive"
                    state = np.array([float(lf.means[0]), float(lf.stds[0])])
                out[f"{tag}_state{s}"] = state
                if cur.get("UCL", True):          # nothing may sit on a comparison's edge
                    table = cur.get("SM", False) or cur.get("SMA", False)
                    for edge in ([cur.get("SMT", 0.15)] if table else [state[0] + cur.get("OFFSET", 0) * state[1]]):
                        assert np.abs(p - edge).min() > 1e-3, (tag, s, edge, np.abs(p - edge).min())
            torch.set_default_dtype(torch.float32)
        print(f"g25 {tag}: {weighted} anchor weights differ from 1")
        assert weighted >= 20 or not cur.get("UCL", True), tag
    MG.save("g25_anchor_cur_loss", **out)


if __name__ == "__main__":
    R = cur_modules()
    g23(R)
    g24(R)
    g25(R)
    with open(os.path.join(HERE, "MANIFEST_anchor_curriculum.json"), "w") as f:
        json.dump(MG.manifest, f, indent=1, sort_keys=True)
