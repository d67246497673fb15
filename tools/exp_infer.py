"""Inference frames/s of the adopted stock CenterPoint detector (tools/stock_detector.py "centerpoint") at Waymo size
(B = 4 x 160 k synth points), three forms in one process, timed alternately (synchronised host clock per batch):

  eager_reference   model.eval() + no_grad, voxelise -> module_list forward -> the existing eager post-processing
                    (generate_predicted_boxes -> class_agnostic_nms -> nms_gpu): the reference's eval loop body
                    (tools/eval_utils/eval_utils.py:58-80) on the fused modules
  eager_static      the same forward, static post-processing (com_amd.postprocess) instead
  captured          com_amd.infer.CapturedInference replays (voxelise + forward + static post-processing, one graph)

plus the post-processing alone on one batch's head maps, eager vs static.  Writes JSON to --out (profiles/infer_fps.json).

With --kind second the anchor-head counterpart (tools/stock_detector.py "second", writes profiles/infer_anchor_fps.json):

  post_eager        AnchorHeadSingle's eager chain, decode_boxes (every anchor: [B, N, 7] + [B, N, num_class]) + post_processing
                    (sigmoid, max, mask, topk, nms_gpu per frame, with the reference's read-backs)
  post_static       com_amd.postprocess.anchor_predictions_static on the same maps
                    -- both on random bf16 maps of pointpillar_1x's head: B = 4, 468 x 468 x 6 anchors, 3 classes, the strided
                       channel blocks of one fused tensor
  captured          com_amd.infer.CapturedInference replays of the adopted "second" detector (frames/s), with SCORE_THRESH
                    lowered and BatchNorm variances set so that a fresh model sends NMS_PRE_MAXSIZE anchors per frame through
                    the chain; the pre-NMS and kept counts of the captured run are written to the JSON

With --kind second_multihead the same report for AnchorHeadMulti with MULTI_CLASSES_NMS (tools/stock_detector.py
"second_multihead": three one-class heads; writes profiles/infer_anchor_multi_fps.json):

  post_eager        decode_boxes (every anchor) + AnchorHeadMulti.post_processing: the loop over frames x heads x classes with a
                    mask gather, a topk and an nms_gpu with its read-back each
  post_static       com_amd.postprocess.anchor_multi_predictions_static on the same maps (those of one eager forward)
  eager_reference   voxelise -> module_list forward -> decode_boxes -> post_processing: the eval loop body
  eager_static / captured   the same forward with the static post-processing, launch by launch / as one graph replay

With --kind second_iou the same report for the two-stage SECOND-IoU (tools/stock_detector.py "second_iou": AnchorHeadSingle ->
SECONDHead; writes profiles/infer_second_iou_fps.json): the eager proposal layer vs pcd_anchor_proposals, eager
second_head.post_processing vs pcd_roi_postproc, the eager eval loop body of the adopted detector vs captured replays.

    python tools/exp_infer.py [--batches 200] [--out profiles/infer_fps.json]
    python tools/exp_infer.py --kind second [--batches 200] [--out profiles/infer_anchor_fps.json]
    python tools/exp_infer.py --kind second_multihead [--batches 200] [--out profiles/infer_anchor_multi_fps.json]
    python tools/exp_infer.py --replay-only          (capture, pause, ONE replay: for rocprofv3 --kernel-trace --stats)
    python tools/exp_infer.py --kind second_iou [--batches 200] [--out profiles/infer_second_iou_fps.json]
    python tools/exp_infer.py --kernel-table <kernel_trace.csv>    (host only: the kernels of that last replay as a table)
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _short(name):
    """kernel name without its parameter list (the parenthesis matching the final one)"""
    if name.endswith(")"):
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += {")": 1, "(": -1}.get(name[i], 0)
            if depth == 0:
                name = name[:i]
                break
    return name.replace("(anonymous namespace)::", "")[:110]


def kernel_table(path):
    """Kernels of the last burst of a rocprofv3 kernel trace (the replay after --replay-only's pause), in launch order."""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    start = 0
    for i in range(1, len(rows)):
        if int(rows[i]["Start_Timestamp"]) - int(rows[i - 1]["End_Timestamp"]) > 200_000_000:     # > 0.2 s gap
            start = i
    rows = rows[start:]
    t0, t1 = int(rows[0]["Start_Timestamp"]), max(int(r["End_Timestamp"]) for r in rows)
    lines = [f"one CapturedInference replay: {len(rows)} kernels, {(t1 - t0) / 1e6:.3f} ms first start -> last end",
             f"{'start_us':>9} {'dur_us':>8}  kernel"]
    agg = {}
    for r in rows:
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        name = _short(r["Kernel_Name"])
        lines.append(f"{(s - t0) / 1e3:9.1f} {(e - s) / 1e3:8.1f}  {name}")
        a = agg.setdefault(name, [0, 0])
        a[0] += 1
        a[1] += e - s
    lines += ["", "by kernel (sum of durations):", f"{'calls':>5} {'sum_us':>9}  kernel"]
    for name, (n, d) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        lines.append(f"{n:5d} {d / 1e3:9.1f}  {name}")
    return "\n".join(lines)


def _summary(times, B, fps_for=()):
    res = {}
    for name, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        res[name] = {"ms_median": round(med * 1e3, 3), "ms_p10": round(ts[len(ts) // 10] * 1e3, 3),
                     "ms_p90": round(ts[(9 * len(ts)) // 10] * 1e3, 3)}
        if name in fps_for:
            res[name]["frames_per_s"] = round(B / med, 1)
    return res


def main_second(a):
    """--kind second: the anchor head's post-processing alone (eager chain vs static) at pointpillar_1x's head size, and
    frames/s of the captured "second" detector."""
    import numpy as np
    import torch
    import stock_detector as SD
    from com_amd import hotpath, postprocess, train
    from com_amd.adopt import adopt_model
    from com_amd.hotpath import anchor_head as AH
    from com_amd.infer import CapturedInference
    from com_amd.utils import synth

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    B = a.batch
    cfg = SD.model_cfg("second")
    post_cfg = cfg.POST_PROCESSING
    # ---- the post-processing alone: pointpillar_1x's head (468 x 468 cells x 6 anchors, stride 1 over 0.32 m pillars)
    head_cfg = SD._cfg(dict(SD.SECOND_MODEL["DENSE_HEAD"]))
    for c in head_cfg.ANCHOR_GENERATOR_CONFIG:
        c["feature_map_stride"] = 1
    head = hotpath.AnchorHeadSingle(head_cfg, 64, 3, list(SD.CLASS_NAMES), np.array([468, 468, 1]), synth.PILLAR_RANGE).to(dev)
    tab = head.tables(dev)
    nc, nb = tab.A * 3, tab.A * 7
    fused = torch.randn(B, tab.H, tab.W, nc + nb + tab.A * 2, device=dev)
    fused[..., :nc] = fused[..., :nc] * 1.5 - 4.0                       # a few per cent of the anchors above SCORE_THRESH
    fused[..., nc:nc + nb] *= 0.1
    fused = fused.bfloat16()
    maps = (fused[..., :nc], fused[..., nc:nc + nb], fused[..., nc + nb:])

    def post_eager(_):
        scores, boxes = AH.decode_boxes(tab, *maps)
        return AH.post_processing({"batch_size": B, "batch_cls_preds": scores, "batch_box_preds": boxes,
                                   "cls_preds_normalized": False}, post_cfg)

    def post_static(_):
        return postprocess.anchor_predictions_static(head, *maps, post_cfg)

    # ---- the captured detector
    # Fresh weights: the class logits sit at the bias of -4.6 (scores near 0.01), so with the config's SCORE_THRESH of 0.1
    # NOTHING would pass and the timed chain would sort, decode and suppress zero boxes.  The threshold is lowered below
    # that, and the BatchNorm running variances are set to 0.13 so that the signal of this residual-free stack survives to
    # the head and the logits depend on the input: every frame then sends NMS_PRE_MAXSIZE anchors through sort, decode and
    # NMS (the counts are recorded below).
    model = SD.build_detector("second")
    model.model_cfg.POST_PROCESSING['SCORE_THRESH'] = 0.005
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith("running_var"):
                v.fill_(0.13)
    model = model.to(dev)
    adopt_model(model)
    batches = [hotpath.collate_points([synth.synth_cloud(B * i + f) for f in range(B)], dev) for i in range(3)]
    vox = train.VoxelizeConfig(synth.WAYMO_RANGE, synth.WAYMO_VOXEL, synth.WAYMO_MAX_POINTS, synth.WAYMO_MAX_VOXELS)
    inf = CapturedInference(model, vox, B)
    inf.capture(batches[0], validate=batches[1:])
    allf = {"post_eager": post_eager, "post_static": post_static, "eager_static": lambda b: inf.eager(b), "captured": lambda b: inf(b)}
    times = {k: [] for k in allf}
    for fn in allf.values():
        for i in range(a.warmup):
            fn(batches[i % 3])
    torch.cuda.synchronize()
    rounds, per = 10, max(1, a.batches // 10)
    for r in range(rounds):
        for name, fn in allf.items():
            for i in range(per):
                t0 = time.perf_counter()
                fn(batches[(r * per + i) % 3])
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
    inf.check()
    static_count = post_static(None)["count"].tolist()
    # what the captured chain worked on: anchors passing SCORE_THRESH, capped at NMS_PRE_MAXSIZE, and the boxes kept
    pp = model.model_cfg.POST_PROCESSING
    cap_counts = {"pre_nms": [], "kept": [], "distinct_scores_kept": []}
    for b in batches:
        out = inf(b)
        torch.cuda.synchronize()
        cap_counts["kept"].append(out["count"].tolist())
        cap_counts["distinct_scores_kept"].append([int(out["scores"][f, :int(n)].unique().numel())
                                                   for f, n in enumerate(out["count"].tolist())])
        inf.eager(b)
        logits = model.dense_head.forward_ret_dict["cls_preds"].float().reshape(B, -1, 3)
        passing = (torch.sigmoid(logits).max(-1)[0] >= pp.SCORE_THRESH).sum(1)
        cap_counts["pre_nms"].append(passing.clamp(max=pp.NMS_CONFIG.NMS_PRE_MAXSIZE).tolist())
    res = {"unit": "ms per batch (median over timed batches), frames/s = B / median", "device": torch.cuda.get_device_name(0),
           "batch": B, "points_per_frame": int(batches[0][0].shape[0] // B), "timed_batches_per_form": rounds * per,
           "warmup": a.warmup, "clock": "host perf_counter around each call + torch.cuda.synchronize()",
           "post_maps": f"random bf16, fused [{B}, {tab.H}, {tab.W}, {fused.shape[3]}], {tab.A} anchors per cell, 3 classes; "
                        f"kept per frame {static_count}",
           "model": "tools/stock_detector.py second, adopt_model(), fresh weights, BatchNorm running_var 0.13, SCORE_THRESH "
                    f"{pp.SCORE_THRESH} (the config's 0.1 lets nothing of a fresh model pass)",
           "captured_counts_per_batch": cap_counts}
    res.update(_summary(times, B, fps_for=("eager_static", "captured")))
    res["post_eager_over_post_static"] = round(res["post_eager"]["ms_median"] / res["post_static"]["ms_median"], 3)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main_second_multihead(a):
    """--kind second_multihead: AnchorHeadMulti's per-class post-processing alone (eager loop vs static) on the maps of one
    forward of the "second_multihead" detector, and frames/s of its eval loop body, eager and captured."""
    import torch
    import stock_detector as SD
    from com_amd import hotpath, postprocess, train
    from com_amd.adopt import adopt_model
    from com_amd.hotpath import anchor_head_multi as AM
    from com_amd.infer import CapturedInference
    from com_amd.utils import synth

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    B = a.batch
    # (fresh weights: SCORE_THRESH lowered and BatchNorm variances set as in main_second, so that every class of every frame
    #  sends NMS_PRE_MAXSIZE anchors through sort, decode and NMS; the counts are recorded below)
    model = SD.build_detector("second_multihead")
    model.model_cfg.POST_PROCESSING['SCORE_THRESH'] = 0.005
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith("running_var"):
                v.fill_(0.13)
    model = model.to(dev)
    adopt_model(model)
    pp = model.model_cfg.POST_PROCESSING
    head = model.dense_head
    batches = [hotpath.collate_points([synth.synth_cloud(B * i + f) for f in range(B)], dev) for i in range(3)]
    vox = train.VoxelizeConfig(synth.WAYMO_RANGE, synth.WAYMO_VOXEL, synth.WAYMO_MAX_POINTS, synth.WAYMO_MAX_VOXELS)
    fs = train.feature_stride(model, vox)
    inf = CapturedInference(model, vox, B)
    inf.capture(batches[0], validate=batches[1:])

    def eager_reference(batch):
        pts, offs = batch
        model.eval()
        with torch.no_grad():
            bd = train.voxelize_batch(vox, B, fs, pts, offs)[1]
            bd = {k: v for k, v in bd.items() if k != "_result"}
            for m in model.module_list:
                bd = m(bd)
            return head.post_processing(bd, pp)

    inf.eager(batches[0])
    f = head.forward_ret_dict
    maps = tuple([t.clone() for t in f[k]] for k in ("cls_preds", "box_preds", "dir_cls_preds"))
    tab = head.tables(dev)
    mapping = [hd.head_label_indices for hd in head.rpn_heads]

    def post_eager(_):
        logits, boxes = AM.decode_boxes(tab, *maps)
        return AM.post_processing({"batch_size": B, "batch_cls_preds": logits, "batch_box_preds": boxes,
                                   "multihead_label_mapping": mapping, "cls_preds_normalized": False}, pp)

    def post_static(_):
        return postprocess.anchor_multi_predictions_static(head, *maps, pp)

    allf = {"post_eager": post_eager, "post_static": post_static, "eager_reference": eager_reference,
            "eager_static": lambda b: inf.eager(b), "captured": lambda b: inf(b)}
    times = {k: [] for k in allf}
    for fn in allf.values():
        for i in range(a.warmup):
            fn(batches[i % 3])
    torch.cuda.synchronize()
    rounds, per = 10, max(1, a.batches // 10)
    for r in range(rounds):
        for name, fn in allf.items():
            for i in range(per):
                t0 = time.perf_counter()
                fn(batches[(r * per + i) % 3])
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
    inf.check()
    static = post_static(None)
    eager = post_eager(None)
    same = [bool(torch.equal(static["boxes"][b, :int(n)], e["pred_boxes"])) for b, (n, e) in
            enumerate(zip(static["count"].tolist(), eager))]
    passing = [[int(v) for v in (torch.sigmoid(t.float()) >= pp.SCORE_THRESH).flatten(2).sum(2).sum(1).tolist()] for t in maps[0]]
    res = {"unit": "ms per batch (median over timed batches), frames/s = B / median", "device": torch.cuda.get_device_name(0),
           "batch": B, "points_per_frame": int(batches[0][0].shape[0] // B), "timed_batches_per_form": rounds * per,
           "warmup": a.warmup, "clock": "host perf_counter around each call + torch.cuda.synchronize()",
           "post_maps": f"the maps of one forward ({maps[0][0].dtype}): {len(maps[0])} heads of {tab.H} x {tab.W} cells; logits "
                        f"passing SCORE_THRESH per head and frame {passing} (NMS_PRE_MAXSIZE {pp.NMS_CONFIG.NMS_PRE_MAXSIZE}); "
                        f"kept per frame {static['count'].tolist()}; static boxes == eager boxes per frame {same}",
           "model": "tools/stock_detector.py second_multihead, adopt_model(), fresh weights, BatchNorm running_var 0.13, "
                    f"SCORE_THRESH {pp.SCORE_THRESH} (the config's 0.1 lets nothing of a fresh model pass)"}
    res.update(_summary(times, B, fps_for=("eager_reference", "eager_static", "captured")))
    res["post_eager_over_post_static"] = round(res["post_eager"]["ms_median"] / res["post_static"]["ms_median"], 3)
    res["captured_over_eager_reference"] = round(res["eager_reference"]["ms_median"] / res["captured"]["ms_median"], 3)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main_second_iou(a):
    """--kind second_iou: the two static halves of the two-stage path alone (the eager proposal layer vs pcd_anchor_proposals on
    the detector's own head size; eager second_head.post_processing vs pcd_roi_postproc on one forward's RoI outputs), and
    frames/s of the eager eval loop body of the adopted "second_iou" detector vs captured replays."""
    import torch
    import stock_detector as SD
    from com_amd import hotpath, postprocess, train
    from com_amd.adopt import adopt_model
    from com_amd.hotpath import anchor_head as AH
    from com_amd.hotpath import second_head as SH
    from com_amd.hotpath.roi_head import RoIHeadTemplate
    from com_amd.infer import CapturedInference
    from com_amd.utils import synth

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    B = a.batch
    # Fresh weights; the BatchNorm running variances are set to 0.13 so that the signal of this residual-free stack survives
    # to the heads and the logits depend on the input (tools/exp_infer.py --kind second does the same).  The proposal layer
    # has no score threshold, and the IoU head's fresh logits sit near 0 (scores near 0.5, above the config's 0.1).
    model = SD.build_detector("second_iou")
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith("running_var"):
                v.fill_(0.13)
    model = model.to(dev)
    adopt_model(model)
    post_cfg, prop_cfg = model.model_cfg.POST_PROCESSING, model.roi_head.model_cfg.NMS_CONFIG.TEST
    names = list(SD.CLASS_NAMES)
    # ---- the proposal layer alone: random bf16 maps of the detector's own head (188 x 188 cells x 6 anchors)
    head = model.dense_head
    tab = head.tables(dev)
    nc, nb = tab.A * 3, tab.A * 7
    fused = torch.randn(B, tab.H, tab.W, nc + nb + tab.A * 2, device=dev)
    fused[..., :nc] = fused[..., :nc] * 1.5 - 4.0
    fused[..., nc:nc + nb] *= 0.1
    fused = fused.bfloat16()
    maps = (fused[..., :nc], fused[..., nc:nc + nb], fused[..., nc + nb:])

    def proposals_eager(_):
        scores, boxes = AH.decode_boxes(tab, *maps)
        return RoIHeadTemplate.proposal_layer(None, {"batch_size": B, "batch_cls_preds": scores, "batch_box_preds": boxes}, prop_cfg)

    def proposals_static(_):
        return postprocess.anchor_proposals_static(head, *maps, prop_cfg)

    batches = [hotpath.collate_points([synth.synth_cloud(B * i + f) for f in range(B)], dev) for i in range(3)]
    vox = train.VoxelizeConfig(synth.WAYMO_RANGE, synth.WAYMO_VOXEL, synth.WAYMO_MAX_POINTS, synth.WAYMO_MAX_VOXELS)
    inf = CapturedInference(model, vox, B)

    def eager_loop(batch):
        """the body of the reference's eval loop on the adopted model: module_list forward, then SECONDNetIoU.post_processing"""
        pts, offs = train._split_batch(batch)
        with inf._Eval(model), torch.no_grad():
            bd = {k: v for k, v in inf._voxelize(pts, offs).items() if k != "_result"}
            for m in model.module_list:
                bd = m(bd)
            return bd, model.roi_head.post_processing(bd, post_cfg, names)

    # ---- the final post-processing alone: the RoI outputs of one eager forward
    roi_bd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in eager_loop(batches[0])[0].items()
              if k in ("batch_size", "batch_box_preds", "batch_cls_preds", "roi_scores", "roi_labels", "has_class_labels",
                       "cls_preds_normalized")}

    def post_eager(_):
        return SH.post_processing(roi_bd, post_cfg, names)

    def post_static(_):
        return postprocess.roi_predictions_static(roi_bd, post_cfg, class_names=names, second_iou=True)

    inf.capture(batches[0], validate=batches[1:])
    allf = {"proposals_eager": proposals_eager, "proposals_static": proposals_static, "post_eager": post_eager,
            "post_static": post_static, "eager_loop": eager_loop, "eager_static": lambda b: inf.eager(b), "captured": lambda b: inf(b)}
    times = {k: [] for k in allf}
    for fn in allf.values():
        for i in range(a.warmup):
            fn(batches[i % 3])
    torch.cuda.synchronize()
    rounds, per = 10, max(1, a.batches // 10)
    for r in range(rounds):
        for name, fn in allf.items():
            for i in range(per):
                t0 = time.perf_counter()
                fn(batches[(r * per + i) % 3])
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
    inf.check()
    kept = []
    for b in batches:
        out = inf(b)
        torch.cuda.synchronize()
        kept.append(out["count"].tolist())
    res = {"unit": "ms per batch (median over timed batches), frames/s = B / median", "device": torch.cuda.get_device_name(0),
           "batch": B, "points_per_frame": int(batches[0][0].shape[0] // B), "timed_batches_per_form": rounds * per,
           "warmup": a.warmup, "clock": "host perf_counter around each call + torch.cuda.synchronize()",
           "proposal_maps": f"random bf16, fused [{B}, {tab.H}, {tab.W}, {fused.shape[3]}], {tab.A} anchors per cell, 3 classes; "
                            f"NMS_CONFIG.TEST {dict(prop_cfg)}; proposals per frame {proposals_static(None)['count'].tolist()}",
           "post_rois": f"{roi_bd['batch_box_preds'].shape[1]} RoIs per frame of one eager forward; kept per frame "
                        f"{post_static(None)['count'].tolist()}",
           "model": "tools/stock_detector.py second_iou, adopt_model(), fresh weights, BatchNorm running_var 0.13; eager_loop = "
                    "module_list forward + second_head.post_processing, eager_static = the captured body launch by launch",
           "captured_kept_per_batch": kept}
    res.update(_summary(times, B, fps_for=("eager_loop", "eager_static", "captured")))
    res["proposals_eager_over_static"] = round(res["proposals_eager"]["ms_median"] / res["proposals_static"]["ms_median"], 3)
    res["post_eager_over_post_static"] = round(res["post_eager"]["ms_median"] / res["post_static"]["ms_median"], 3)
    res["captured_over_eager_loop"] = round(res["eager_loop"]["ms_median"] / res["captured"]["ms_median"], 3)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=["centerpoint", "second", "second_multihead", "second_iou"], default="centerpoint")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--batches", type=int, default=200, help="timed batches per form")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--replay-only", action="store_true")
    ap.add_argument("--kernel-table")
    a = ap.parse_args()
    if a.kernel_table:
        print(kernel_table(a.kernel_table))
        return
    names = {"centerpoint": "infer_fps.json", "second": "infer_anchor_fps.json", "second_multihead": "infer_anchor_multi_fps.json",
             "second_iou": "infer_second_iou_fps.json"}
    a.out = a.out or os.path.join(ROOT, "profiles", names[a.kind])
    if a.kind == "second":
        return main_second(a)
    if a.kind == "second_multihead":
        return main_second_multihead(a)
    if a.kind == "second_iou":
        return main_second_iou(a)

    import torch
    import stock_detector as SD
    from com_amd import hotpath, postprocess, train
    from com_amd.adopt import adopt_model
    from com_amd.infer import CapturedInference
    from com_amd.utils import synth

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    B = a.batch
    model = SD.build_detector("centerpoint").to(dev)
    adopt_model(model)
    batches = [hotpath.collate_points([synth.synth_cloud(B * i + f) for f in range(B)], dev) for i in range(3)]
    vox = train.VoxelizeConfig(synth.WAYMO_RANGE, synth.WAYMO_VOXEL, synth.WAYMO_MAX_POINTS, synth.WAYMO_MAX_VOXELS)
    inf = CapturedInference(model, vox, B)
    inf.capture(batches[0], validate=batches[1:])
    if a.replay_only:
        torch.cuda.synchronize()
        time.sleep(1.0)
        inf(batches[1])
        torch.cuda.synchronize()
        print("replay-only: one replay done")
        return

    fs = train.feature_stride(model, vox)
    head = model.dense_head

    def eager(batch, static):
        pts, offs = batch
        model.eval()
        with torch.no_grad():
            bd = train.voxelize_batch(vox, B, fs, pts, offs)[1]
            bd = {k: v for k, v in bd.items() if k != "_result"}
            if static:
                bd["static_predictions"] = True
            for m in model.module_list:
                bd = m(bd)
        return bd["final_box_tensors"] if static else bd["final_box_dicts"]

    forms = {"eager_reference": lambda b: eager(b, False), "eager_static": lambda b: eager(b, True),
             "captured": lambda b: inf(b)}
    # the post-processing alone, on the head maps of one eager forward
    eager(batches[0], True)
    maps = [{k: v.clone() for k, v in pd.items()} for pd in head.forward_ret_dict["pred_dicts"]]
    post = {"post_eager": lambda b: head.generate_predicted_boxes(B, maps),
            "post_static": lambda b: postprocess.decode_predictions_static(maps, head)}
    times = {k: [] for k in list(forms) + list(post)}
    allf = dict(forms, **post)
    for name, fn in allf.items():
        for i in range(a.warmup):
            fn(batches[i % 3])
    torch.cuda.synchronize()
    rounds, per = 10, max(1, a.batches // 10)
    for r in range(rounds):
        for name, fn in allf.items():
            for i in range(per):
                t0 = time.perf_counter()
                fn(batches[(r * per + i) % 3])
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
    inf.check()
    res = {"unit": "ms per batch (median over timed batches), frames/s = B / median", "device": torch.cuda.get_device_name(0),
           "batch": B, "points_per_frame": int(batches[0][0].shape[0] // B), "timed_batches_per_form": rounds * per,
           "warmup": a.warmup, "clock": "host perf_counter around each call + torch.cuda.synchronize()",
           "model": "tools/stock_detector.py centerpoint, adopt_model(), fresh weights (every pixel passes SCORE_THRESH)"}
    for name, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        res[name] = {"ms_median": round(med * 1e3, 3), "ms_p10": round(ts[len(ts) // 10] * 1e3, 3),
                     "ms_p90": round(ts[(9 * len(ts)) // 10] * 1e3, 3)}
        if name in forms:
            res[name]["frames_per_s"] = round(B / med, 1)
    res["captured_over_eager_reference"] = round(res["eager_reference"]["ms_median"] / res["captured"]["ms_median"], 3)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
