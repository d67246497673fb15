#!/usr/bin/env python3
"""Generate the multi-head anchor-head fixtures under tests/golden/ (run once, where the reference lies at /root/reference
and oracle/_ref holds its compiled iou3d_cpu; not needed at test time).  In the style of make_golden_anchor.py, whose
stand-in packages it uses: the reference's own anchor_head_multi.py is imported from its read-only location (BaseBEVBackbone
loaded from its file under a stand-in pcdet.models.backbones_2d), with a `.cuda()` identity patch, and run on the CPU; only
arrays and short labels (data) are stored.  Cases N (nuScenes form) and K (KITTI form): tests/anchor_multi_ref.py.

  g38_anchor_multi_targets   AnchorHeadMulti.assign_targets on B = 3 frames (every class + the quirks / one box / none):
                             labels, targets and the box index of every positive, all anchors
  g39_anchor_multi_loss_N|K  get_cls_layer_loss + get_box_reg_layer_loss on drawn per-head maps, fp32 and fp64: scalars and
                             the gradient of every head's maps
  g40_anchor_multi_decode_N|K  generate_predicted_boxes on drawn maps (two frames)
  g41_anchor_multi_postproc  Detector3DTemplate.post_processing (MULTI_CLASSES_NMS) with `nms_gpu` bound to a greedy NMS
                             over the reference's compiled iou3d_cpu (case N)
  g42_anchor_multi_module    the reference module's state dict, an input map, and the rpn_loss of its own forward + get_loss

Usage: python tests/golden/make_golden_anchor_multi.py
"""
import importlib
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import anchor_multi_ref as AR  # noqa: E402
import make_golden_anchor as G  # noqa: E402
from oracle import oracle as O  # noqa: E402

REF = G.REF
D, save = G.D, G.save


def deep(cfg):
    if isinstance(cfg, dict):
        return D({k: deep(v) for k, v in cfg.items()})
    if isinstance(cfg, list):
        return [deep(v) for v in cfg]
    return cfg


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def ref_nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    """iou3d_nms_utils.nms_gpu with the kernel replaced by a greedy pass over the reference's own boxes_iou_bev_cpu"""
    order = scores.sort(0, descending=True)[1]
    if pre_maxsize is not None:
        order = order[:pre_maxsize]
    b = boxes[order].contiguous().numpy()
    iou = O.ref_boxes_iou_bev_cpu(b, b)
    dead = np.zeros(len(b), bool)
    keep = []
    for i in range(len(b)):
        if dead[i]:
            continue
        keep.append(i)
        dead |= iou[i] > thresh
    ref_nms_gpu.ious.append(iou)
    return order[torch.tensor(keep, dtype=torch.int64)].contiguous(), None


ref_nms_gpu.ious = []


def ref_classes():
    R = G.ref_modules()
    G._ns("pcdet.models.dense_heads.target_assigner.atss_target_assigner", None, ATSSTargetAssigner=None)
    bev = _load("pcdet.models.backbones_2d.base_bev_backbone", REF + "/models/backbones_2d/base_bev_backbone.py")
    G._ns("pcdet.models.backbones_2d", None, BaseBEVBackbone=bev.BaseBEVBackbone, map_to_bev=types.SimpleNamespace())
    sys.modules["pcdet.models.backbones_2d.map_to_bev"] = sys.modules["pcdet.models.backbones_2d"].map_to_bev
    R.multi = importlib.import_module("pcdet.models.dense_heads.anchor_head_multi")
    # Detector3DTemplate.post_processing: the class needs its whole package; stand-ins for what its module imports
    G._ns("pcdet.utils.spconv_utils", None, find_all_spconv_keys=None)
    b3 = G._ns("pcdet.models.backbones_3d", None, pfe=types.SimpleNamespace(), vfe=types.SimpleNamespace())
    sys.modules["pcdet.models.backbones_3d.pfe"], sys.modules["pcdet.models.backbones_3d.vfe"] = b3.pfe, b3.vfe
    G._ns("pcdet.models.roi_heads", None)
    sys.modules["pcdet.ops.iou3d_nms"].iou3d_nms_utils.nms_gpu = ref_nms_gpu
    nms = _load("pcdet.models.model_utils.model_nms_utils", REF + "/models/model_utils/model_nms_utils.py")
    sys.modules["pcdet.models.model_utils"].model_nms_utils = nms
    G._ns("pcdet.models.detectors", REF + "/models/detectors")
    R.det = _load("pcdet.models.detectors.detector3d_template", REF + "/models/detectors/detector3d_template.py")
    return R


def boxes_for(case):
    """gt_boxes [3, 16, code_gt + 1]: frame 0 every class + the quirks, frame 1 one box, frame 2 none"""
    names, code_gt = AR.CASES[case]["names"], AR.CASES[case]["code_gt"]
    r = np.random.default_rng(38)
    gt = np.zeros((3, 16, code_gt + 1), np.float32)
    rows = []
    for ci, n in enumerate(names):                                      # two ordinary boxes per class
        for _ in range(2):
            size = np.array(AR.SIZES[n]) * r.uniform(0.85, 1.15, 3)
            rows.append([r.uniform(2, 16), r.uniform(-6, 6), AR.BOTTOM[n] + size[2] / 2 + r.uniform(-.2, .2), *size,
                         r.uniform(-2 * np.pi, 2 * np.pi), ci + 1])
    s = AR.SIZES[names[0]]
    rows.append([9.0, 1.0, 0.0, 3.2 * s[0], 2.2 * s[1], s[2], 0.02, 1])   # positive only through its per-box maximum
    rows.append([100.0, 3.0, 0.0, *AR.SIZES[names[1]], 0.3, 2])          # zero IoU with every anchor of its class
    rows.append([12.0, -3.0, -0.2, *AR.SIZES[names[-1]], np.pi / 4 + 1e-3, len(names)])
    at = [0, 1, 2, 4, 5, 6, 7, 9, 10, 11, 13, 14, 15][:len(rows)]       # rows 3, 8, 12 stay zero: padding in the middle
    assert len(at) == len(rows)
    for i, row in zip(at, rows):
        gt[0, i, :7], gt[0, i, -1] = row[:7], row[7]
        if code_gt == 9:
            gt[0, i, 7:9] = r.uniform(-3, 3, 2)
    n = names[0]
    gt[1, 0, :7], gt[1, 0, -1] = [8.4, 0.4, AR.BOTTOM[n] + AR.SIZES[n][2] / 2, *AR.SIZES[n], 1.57], 1
    if code_gt == 9:
        gt[1, 0, 7:9] = [1.5, -0.5]
    return gt


def build_head(R, case, seed):
    torch.manual_seed(seed)
    c = AR.CASES[case]
    head = R.multi.AnchorHeadMulti(deep(AR.model_cfg(case)), AR.IN_CHANNELS, len(c["names"]), c["names"], np.array(AR.GRID),
                                   AR.RANGE, predict_boxes_when_training=True)
    g = torch.Generator().manual_seed(seed + 1)
    for m in head.modules():                                            # non-trivial BatchNorm parameters / statistics
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.uniform_(0.6, 1.4, generator=g)
            m.bias.data.uniform_(-0.3, 0.3, generator=g)
            m.running_mean.uniform_(-0.2, 0.2, generator=g)
            m.running_var.uniform_(0.7, 1.3, generator=g)
    for hd in head.rpn_heads:                                           # box convs of the 1 x 1 form start at std 1e-3
        if isinstance(hd.conv_box, torch.nn.Conv2d):
            hd.conv_box.weight.data.normal_(0, 0.05, generator=g)
    return head


def gt_index_of(R, head, case, gt, labels):
    names = AR.CASES[case]["names"]
    gi = -np.ones(labels.shape, np.int32)
    for b in range(gt.shape[0]):
        start = 0
        for ci, anchors in enumerate(head.anchors):
            flat = anchors.permute(3, 4, 0, 1, 2, 5).contiguous().view(-1, anchors.shape[-1])
            rows = np.nonzero(gt[b, :, -1] == ci + 1)[0]
            if rows.size:
                iou = R.bu.boxes3d_nearest_bev_iou(flat[:, :7], torch.from_numpy(gt[b, rows, :7].copy()))
                arg = rows[iou.argmax(dim=1).numpy()]
                idx = start + np.arange(flat.shape[0])
                pos = labels[b, idx] > 0
                gi[b, idx[pos]] = arg[pos]
            start += flat.shape[0]
        assert start == labels.shape[1]
    assert ((gi >= 0) == (labels > 0)).all() and len(names) == len(head.anchors)
    return gi


def draw_maps(case, rng, B, for_decode):
    """per-head [B, A_h * items, H, W] maps (cls, box, dir | None)"""
    W, H = AR.GRID[0], AR.GRID[1]
    code = AR.CASES[case]["code_gt"] + (1 if case == "N" else 0)
    cls, box, dr = [], [], []
    for _, nk, _, nc in AR.head_layout(case):
        cls.append(rng.normal(-1.0, 2.0, (B, nk * nc, H, W)).astype(np.float32))
        bx = rng.normal(0, 0.4, (B, nk, code, H, W)).astype(np.float32)
        if case == "N" and for_decode:                                  # keep atan2 away from the origin
            bx[:, :, 6:8] = rng.uniform(-0.3, 0.3, (B, nk, 2, H, W))
        box.append(bx.reshape(B, nk * code, H, W))
        dr.append(rng.normal(0, 1.5, (B, nk * 2, H, W)).astype(np.float32))
    return cls, box, (dr if case == "K" else None)


def ref_lists(case, maps, dt=None, grad=False):
    """the reference's [B, N_h, items] lists from the maps (its own view + permute, anchor_head_multi.py:124-137)"""
    leaves, lists = [], []
    for group in maps:
        if group is None:
            leaves.append(None)
            lists.append(None)
            continue
        lv = [torch.from_numpy(m).to(dt or torch.float32).requires_grad_(grad) for m in group]
        leaves.append(lv)
        lists.append([AR.to_anchor_major(t, nk).contiguous() for t, (_, nk, _, _) in zip(lv, AR.head_layout(case))])
    return leaves, lists


def main():
    R = ref_classes()
    out38, out39, out40, out41, out42 = {}, {}, {}, {}, {}
    for case in ("N", "K"):
        names = AR.CASES[case]["names"]
        head = build_head(R, case, 42 + len(names))
        gt = boxes_for(case)
        B = gt.shape[0]
        # ---- g38
        tg = head.assign_targets(torch.from_numpy(gt.copy()))
        labels = tg["box_cls_labels"].numpy().astype(np.int32)
        targets = tg["box_reg_targets"].numpy()
        assert (tg["reg_weights"].numpy() == (labels > 0)).all() and (targets[labels <= 0] == 0).all()
        gi = gt_index_of(R, head, case, gt, labels)
        print(case, "positives", (labels > 0).sum(1), "ignored", (labels < 0).sum(1), "N", labels.shape[1])
        forced_row, far_row = 10, 11                                     # boxes_for: rows.append order -> `at`
        cls0 = names[0]
        assert (gi[0] == forced_row).any(), "the per-box-maximum box has no positive"
        assert not (gi[0] == far_row).any()
        out38.update({f"{case}_gt_boxes": gt, f"{case}_labels": labels.astype(np.int8), f"{case}_targets": targets,
                      f"{case}_gt_index": gi, f"{case}_num_pos": (labels > 0).sum(1).astype(np.int32)})
        anchors = torch.cat([a.permute(3, 4, 0, 1, 2, 5).contiguous().view(-1, a.shape[-1]) for a in head.anchors], 0)
        out38[f"{case}_anchors"] = anchors.numpy()
        # ---- g39
        rng = np.random.default_rng(39 + len(names))
        maps = draw_maps(case, rng, B, False)
        for q, name in enumerate(("cls", "box", "dir")):
            if maps[q] is not None:
                for h, m in enumerate(maps[q]):
                    out39[f"{case}_{name}{h}"] = m
        for dt, dtag in ((torch.float32, "f32"), (torch.float64, "f64")):
            leaves, lists = ref_lists(case, maps, dt, grad=True)
            head.reg_loss_func.code_weights = head.reg_loss_func.code_weights.to(dt)
            head.forward_ret_dict = dict(cls_preds=lists[0], box_preds=lists[1], box_cls_labels=torch.from_numpy(labels.copy()),
                                         box_reg_targets=torch.from_numpy(targets).to(dt))
            if lists[2] is not None:
                head.forward_ret_dict["dir_cls_preds"] = lists[2]
            cls_loss, tb = head.get_cls_layer_loss()
            box_loss, tb2 = head.get_box_reg_layer_loss()
            loss = cls_loss + box_loss
            loss.backward()
            out39[f"{case}_{dtag}_scalars"] = np.array([float(loss), tb["rpn_loss_cls"], tb2["rpn_loss_loc"],
                                                        tb2.get("rpn_loss_dir", 0.0)], np.float64)
            for q, name in enumerate(("dcls", "dbox", "ddir")):
                if leaves[q] is not None:
                    for h, t in enumerate(leaves[q]):
                        out39[f"{case}_{dtag}_{name}{h}"] = t.grad.numpy()
        head.reg_loss_func.code_weights = head.reg_loss_func.code_weights.float()
        # ---- g40
        rng = np.random.default_rng(40 + len(names))
        B40 = 2                                                          # (two frames keep each file under 1 MB)
        maps = draw_maps(case, rng, B40, True)
        _, lists = ref_lists(case, maps)
        with torch.no_grad():
            cls_list, boxes = head.generate_predicted_boxes(B40, lists[0], [t.clone() for t in lists[1]], lists[2])
        if case == "N":
            enc = torch.cat(lists[1], 1)
            ra = anchors[:, 6].view(1, -1)
            hyp = torch.hypot(enc[..., 6] + torch.cos(ra), enc[..., 7] + torch.sin(ra))
            assert float(hyp.min()) >= 0.5, float(hyp.min())
        for q, name in enumerate(("cls", "box", "dir")):
            if maps[q] is not None:
                for h, m in enumerate(maps[q]):
                    out40[f"{case}_{name}{h}"] = m
        out40[f"{case}_batch_box_preds"] = boxes.numpy()
        for h, t in enumerate(cls_list):
            out40[f"{case}_batch_cls_preds{h}"] = t.numpy()
        # ---- g42: the module itself (training mode: batch statistics), its own loss
        x = np.random.default_rng(42 + len(names)).normal(0, 1.0, (B, AR.IN_CHANNELS, AR.GRID[1], AR.GRID[0])).astype(np.float32)
        state = {k: v.detach().clone() for k, v in head.state_dict().items()}
        head.train()
        head.forward_ret_dict = {}
        dd = head({"spatial_features_2d": torch.from_numpy(x), "gt_boxes": torch.from_numpy(gt.copy()), "batch_size": B})
        loss, tb = head.get_loss()
        out42[f"{case}_input"] = x
        out42[f"{case}_rpn_loss"] = np.array([float(loss), tb["rpn_loss_cls"], tb["rpn_loss_loc"], tb.get("rpn_loss_dir", 0.0)],
                                             np.float64)
        out42[f"{case}_keys"] = np.array(list(state))
        for k, v in state.items():
            out42[f"{case}_state_{k}"] = v.numpy()
        out42[f"{case}_batch_box_preds"] = dd["batch_box_preds"].detach().numpy()
        print(case, "module rpn_loss", out42[f"{case}_rpn_loss"])
        # ---- g41 (case N): post-processing of drawn logits over the decoded boxes of g40
        if case == "N":
            pp = deep(AR.POST_PROCESSING)
            nms = pp.NMS_CONFIG
            for seed in range(410, 470):
                rng = np.random.default_rng(seed)
                logits = [rng.normal(-2.5, 1.6, t.shape).astype(np.float32) for t in cls_list]
                logits[1][..., 1] = rng.normal(-6.0, 0.5, logits[1][..., 1].shape)   # bus: nothing above the threshold
                me = types.SimpleNamespace(model_cfg=D(POST_PROCESSING=pp), num_class=len(names),
                                           generate_recall_record=R.det.Detector3DTemplate.generate_recall_record)
                ref_nms_gpu.ious = []
                bd = {"batch_size": B40, "batch_box_preds": boxes.clone(), "batch_cls_preds": [torch.from_numpy(a) for a in logits],
                      "multihead_label_mapping": [hd.head_label_indices for hd in head.rpn_heads], "cls_preds_normalized": False}
                preds, _ = R.det.Detector3DTemplate.post_processing(me, bd)
                ok = all((np.abs(i[np.triu_indices_from(i, 1)] - nms.NMS_THRESH) > 1e-3).all() for i in ref_nms_gpu.ious)
                cut = none_above = False
                for b in range(B40):
                    for lg in logits:
                        s = 1.0 / (1.0 + np.exp(-lg[b].astype(np.float64)))
                        ok = ok and (np.abs(s - pp.SCORE_THRESH) > 1e-6).all()
                        for k in range(s.shape[1]):
                            above = torch.sigmoid(torch.from_numpy(lg[b, :, k]))
                            above = above[above >= pp.SCORE_THRESH].numpy()
                            ok = ok and np.unique(above).size == above.size
                            none_above = none_above or above.size == 0
                    lab = preds[b]["pred_labels"].numpy()
                    cut = cut or (np.bincount(lab, minlength=len(names) + 1) == nms.NMS_POST_MAXSIZE).any()
                near = sum(int((np.abs(i[np.triu_indices_from(i, 1)] - nms.NMS_THRESH) <= 1e-3).sum()) for i in ref_nms_gpu.ious)
                print("g41 seed", seed, "pairs near the threshold", near, "ok", bool(ok), "cut", bool(cut), "none", none_above)
                if ok and cut and none_above:
                    break
            else:
                raise AssertionError("no seed met the g41 conditions")
            print("g41 seed", seed, "detections per frame", [len(p["pred_scores"]) for p in preds])
            for h, a in enumerate(logits):
                out41[f"N_batch_cls_preds{h}"] = a
            out41["N_batch_box_preds"] = boxes.numpy()
            for b, p in enumerate(preds):
                out41[f"N_pred_boxes{b}"] = p["pred_boxes"].numpy()
                out41[f"N_pred_scores{b}"] = p["pred_scores"].numpy()
                out41[f"N_pred_labels{b}"] = p["pred_labels"].numpy()
    save("g38_anchor_multi_targets", **out38)
    for case in ("N", "K"):                                              # (one file per case: each stays under 1 MB)
        save(f"g39_anchor_multi_loss_{case}", **{k: v for k, v in out39.items() if k.startswith(case + "_")})
    for case in ("N", "K"):
        save(f"g40_anchor_multi_decode_{case}", **{k: v for k, v in out40.items() if k.startswith(case + "_")})
    save("g41_anchor_multi_postproc", **out41)
    save("g42_anchor_multi_module", **out42)
    with open(os.path.join(HERE, "MANIFEST_anchor_multi.json"), "w") as f:
        json.dump(G.manifest, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
