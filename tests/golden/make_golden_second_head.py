#!/usr/bin/env python3
"""Generate the SECONDHead fixtures under tests/golden/ (run once, where the reference lies at /root/reference; not needed at
test time).  In the style of make_golden_roi_head.py, whose stand-in packages it reuses: the reference's own second_head.py,
roi_head_template.py, proposal_target_layer.py, loss_utils.py and second_net_iou.py are imported from their read-only location
with the `.cuda()` identity patch and run on the CPU; only arrays (data) are stored.  For the fp64 values `Tensor.float()` is
left as the identity on fp64 tensors (second_head.py:102 casts theta with .float()).

  g43_second_pool      roi_grid_pool on B = 2, C = 70, H = 13, W = 11, N = 13 at G = 7 and G = 3, from f32 features and from
                       their bf16-rounded copy.  C = 70: a full chunk of 64 channels plus a tail.  The fp64 results are
                       stored ROUNDED TO FLOAT32 (89180 + 16380 elements, twice: as fp64 they would be 1.7 MB, above what
                       a committed file may hold).  |feature| <= 4 and the four weights sum to 1, so |value| <= 4 and the
                       rounding moves a value by at most half an ulp below 4, 2.4e-7 (asserted here): the tests take
                       2.5e-7 OFF their bars.  Of the reference's own f32 result the largest distance from its fp64
                       result is stored, per grid size.
  g44_second_loss      get_box_iou_layer_loss under autograd in f32 and f64: three IOU_LOSS values x five cases
  g45_second_module    a small head: state dict, eval forward from given rois, train forward + get_loss + backward on the
                       targets g31 recorded for scene A (DP_RATIO 0)
  g46_second_postproc  SECONDNetIoU.post_processing for the five score types (and SCORE_TYPE absent) on B = 2, K = 24 boxes of
                       three classes; `nms_gpu` bound to a greedy pass over the BEV IoU of the C oracle, per-box point counts
                       from this project's points_in_boxes_cpu (which g26 pins to the reference)

Usage: python tests/golden/make_golden_second_head.py
"""
import contextlib
import importlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_roi_head as G  # noqa: E402
import second_head_ref as SR  # noqa: E402
from oracle import oracle as O  # noqa: E402

REF = G.REF
D = G.D
manifest = {}
MARGIN = 1e-4


def deep(cfg):
    if isinstance(cfg, dict):
        return D({k: deep(v) for k, v in cfg.items()})
    if isinstance(cfg, list):
        return [deep(v) for v in cfg]
    return cfg


def save(name, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    manifest[name] = {"sha256": G.sha(*[arrays[k] for k in sorted(arrays)]).hexdigest(),
                      "arrays": {k: [str(np.asarray(v).dtype), list(np.asarray(v).shape)] for k, v in arrays.items()},
                      "bytes": os.path.getsize(path)}
    print(f"{name}: {manifest[name]['bytes']} bytes")
    assert manifest[name]["bytes"] < 1024 * 1024


def dbl(dt):
    return G.keep_double() if dt == torch.float64 else contextlib.nullcontext()


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def bev_iou(b):
    """[n, n] rotated BEV IoU over the C oracle's overlap (iou3d_nms_kernel.cu: / max(sa + sb - s, EPS))"""
    b = np.ascontiguousarray(b[:, :7], np.float32)
    ov = O.boxes_pairwise_bev(b, b, False).astype(np.float64)
    area = (b[:, 3] * b[:, 4]).astype(np.float64)
    return ov / np.maximum(area[:, None] + area[None, :] - ov, 1e-8)


def ref_nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    """iou3d_nms_utils.nms_gpu with the kernel replaced by a greedy pass (the stub of make_golden_anchor_multi.py, over the C
    oracle's BEV IoU)"""
    order = scores.sort(0, descending=True)[1]
    if pre_maxsize is not None:
        order = order[:pre_maxsize]
    iou = bev_iou(boxes[order].contiguous().numpy())
    dead = np.zeros(len(iou), bool)
    keep = []
    for i in range(len(iou)):
        if dead[i]:
            continue
        keep.append(i)
        dead |= iou[i] > thresh
    return order[torch.tensor(keep, dtype=torch.int64)].contiguous(), None


def ref_classes():
    from com_amd import roiaware_pool3d
    R = G.ref_modules()
    R.head = importlib.import_module("pcdet.models.roi_heads.second_head")
    sys.modules["pcdet.ops.iou3d_nms"].iou3d_nms_utils.nms_gpu = ref_nms_gpu
    nms = _load("pcdet.models.model_utils.model_nms_utils", REF + "/models/model_utils/model_nms_utils.py")
    sys.modules["pcdet.models.model_utils"].model_nms_utils = nms
    sys.modules["pcdet.ops.roiaware_pool3d"].roiaware_pool3d_utils.points_in_boxes_cpu = roiaware_pool3d.points_in_boxes_cpu

    class Detector3DTemplate:                                              # what SECONDNetIoU.post_processing takes from it
        def generate_recall_record(self, box_preds, recall_dict, batch_index, data_dict=None, thresh_list=None):
            return recall_dict

    G._ns("pcdet.models.detectors", REF + "/models/detectors")
    G._ns("pcdet.models.detectors.detector3d_template", None, Detector3DTemplate=Detector3DTemplate)
    R.det = importlib.import_module("pcdet.models.detectors.second_net_iou")
    return R


def ref_head(R, cfg, in_channels=6):
    return R.head.SECONDHead(input_channels=in_channels, model_cfg=deep(cfg), num_class=1)


# ---------------------------------------------------------------------------------------------------------------------
def pool_rois(r, H, W):
    """[2, 13, 7]: the rows the pooling can go wrong on (module docstring of tests/test_second_head_cpu.py re-asserts them)"""
    g = SR.POOL_GEOM
    cell = g['voxel'] * g['ratio']
    X = lambda px: g['min_x'] + px * cell                                  # noqa: E731  world x of pixel column px
    Y = lambda py: g['min_y'] + py * cell                                  # noqa: E731

    def box(px, py, dx, dy, a):
        return [X(px), Y(py), r.uniform(-1, 1), dx, dy, r.uniform(1, 2), a]

    f0 = [[0.0] * 7,                                                       # the proposal layer's padding
          box(40.0, 35.0, 4.0, 2.0, 0.3),                                  # wholly outside the map
          box(0.2, 5.1, 3.6, 2.2, 0.4), box(-0.7, 9.3, 4.1, 1.8, -1.1),     # left edge
          box(W - 1.3, 4.2, 3.9, 2.1, 2.0), box(W - 0.4, 8.8, 4.4, 1.7, 0.9),
          box(3.3, 0.4, 3.7, 2.4, -0.6), box(7.6, -0.8, 4.2, 2.0, 1.3),     # top edge
          box(2.9, H - 1.2, 3.5, 1.9, 2.6), box(6.4, H - 0.3, 4.0, 2.3, -2.2),
          [X(W - 1), Y(H - 1), 0.0, 0.0, 0.0, 0.0, 0.7],                    # zero size, centre exactly pixel (W - 1, H - 1)
          [X(5), Y(6), 0.0, 6.0, 6.0, 1.5, 0.0],                           # every sample on a pixel centre (G = 7 and G = 3)
          box(5.4, 6.3, 3.1, 1.6, 0.8)]
    f1 = [box(r.uniform(-1, W), r.uniform(-1, H), r.uniform(1.5, 5), r.uniform(1, 3), r.uniform(-np.pi, np.pi)) for _ in range(9)]
    f1 += [box(4.2, 5.5, 4.8, 2.2, -4.0), box(6.1, 7.7, 3.3, 1.9, 7.5),      # headings below 0 and above 2 pi
           box(W - 1.0, 3.0, 2.0, 2.0, np.pi / 2), box(0.0, 0.0, 5.0, 5.0, -np.pi / 4)]
    return np.asarray([f0, f1], np.float32)


def g43(R):
    r = np.random.default_rng(43)
    B, C, H, W, N = 2, 70, 13, 11, 13
    g = SR.POOL_GEOM
    feats = np.clip(r.normal(0, 1, (B, C, H, W)), -4, 4).astype(np.float32)
    feats_bf16 = G.bf16_round(feats)
    rois = pool_rois(r, H, W)
    assert rois.shape == (B, N, 7)
    ds = deep(SR.dataset_cfg([g['min_x'], g['min_y'], -3, g['min_x'] + W, g['min_y'] + H, 1], [g['voxel'], g['voxel'], 4]))
    out = dict(features=feats, rois=rois)
    for G_ in (7, 3):
        head = ref_head(R, SR.model_cfg(grid=G_, in_channel=C), C)
        res = {}
        for tag, x, dt in (("f32", feats, torch.float32), ("f64", feats, torch.float64), ("bf16_f64", feats_bf16, torch.float64)):
            bd = {'batch_size': B, 'rois': torch.from_numpy(rois).to(dt), 'spatial_features_2d': torch.from_numpy(x).to(dt),
                  'dataset_cfg': ds}
            with dbl(dt):
                res[tag] = head.roi_grid_pool(bd).numpy()
            assert res[tag].shape == (B * N, C, G_, G_) and res[tag].dtype == (np.float64 if dt == torch.float64 else np.float32)
        cell = g['voxel'] * g['ratio']
        mine = SR.roi_grid_pool(feats, rois, G_, g['min_x'], g['min_y'], cell, cell)
        print(f"g43 G={G_}: restatement vs reference f64 {np.abs(mine - res['f64']).max():.2e}, reference f32 vs f64 "
              f"{np.abs(res['f32'] - res['f64']).max():.2e}")
        out[f"pool_f64_G{G_}"] = res['f64'].astype(np.float32)
        out[f"pool_bf16_f64_G{G_}"] = res['bf16_f64'].astype(np.float32)
        out[f"ref_f32_max_err_G{G_}"] = np.array(np.abs(res['f32'] - res['f64']).max())
        assert np.abs(out[f"pool_f64_G{G_}"] - res['f64']).max() <= 2.5e-7
    save("g43_second_pool", **out)


# ---------------------------------------------------------------------------------------------------------------------
def g44(R):
    r = np.random.default_rng(44)
    n = 96
    logits = r.normal(0, 2.0, (n, 1)).astype(np.float32)
    labels = r.uniform(0, 1, n).astype(np.float32)
    labels[r.permutation(n)[:10]] = r.choice([0.0, 1.0], 10)                 # the ends of the roi_iou ramp
    some = labels.copy()
    some[r.permutation(n)[:37]] = -1.0
    sat = logits.copy()
    sat[r.permutation(n)[:24], 0] = r.choice([-40.0, 40.0], 24)
    cases = {'plain': (logits, labels), 'some_ignored': (logits, some), 'all_ignored': (logits, np.full(n, -1.0, np.float32)),
             'saturated': (sat, labels), 'bf16': (G.bf16_round(logits), labels)}
    assert tuple(cases) == SR.LOSS_CASES
    out = {}
    for case, (x, t) in cases.items():
        out[f"{case}_logits"], out[f"{case}_labels"] = x, t
    for kind, weight in SR.LOSS_WEIGHTS.items():
        head = ref_head(R, SR.model_cfg(iou_loss=kind, weight=weight))
        for case, (x, t) in cases.items():
            for dt, dtag in ((torch.float32, "f32"), (torch.float64, "f64")):
                xt = torch.from_numpy(x).to(dt).requires_grad_(True)
                with dbl(dt):
                    loss, tb = head.get_box_iou_layer_loss({'rcnn_iou': xt, 'rcnn_cls_labels': torch.from_numpy(t).to(dt)})
                    loss.backward()
                assert abs(tb['rcnn_loss_iou'] - float(loss)) < 1e-12
                out[f"{kind}_{case}_{dtag}_loss"] = np.array(float(loss), np.float64)
                out[f"{kind}_{case}_{dtag}_dlogits"] = xt.grad.numpy()
            mine = SR.iou_loss(x, t, kind, weight)
            print(f"g44 {kind} {case}: loss {float(out[f'{kind}_{case}_f64_loss']):.6f}, restatement off by "
                  f"{abs(mine[0] - float(out[f'{kind}_{case}_f64_loss'])):.1e} / "
                  f"{np.abs(mine[2] - out[f'{kind}_{case}_f64_dlogits'].reshape(-1)).max():.1e}")
        assert out[f"{kind}_all_ignored_f64_loss"] == 0 and not out[f"{kind}_all_ignored_f64_dlogits"].any()
    save("g44_second_loss", **out)


# ---------------------------------------------------------------------------------------------------------------------
def g45(R):
    g30, g31 = dict(np.load(os.path.join(HERE, "g30_roi_overlaps.npz"))), dict(np.load(os.path.join(HERE, "g31_roi_targets.npz")))
    r = np.random.default_rng(45)
    torch.manual_seed(45)
    cfg = SR.model_cfg()
    head = ref_head(R, cfg)
    gen = torch.Generator().manual_seed(46)
    for m in head.modules():                                                # non-trivial BatchNorm parameters / statistics
        if isinstance(m, torch.nn.BatchNorm1d):
            m.weight.data.uniform_(0.6, 1.4, generator=gen)
            m.bias.data.uniform_(-0.3, 0.3, generator=gen)
            m.running_mean.uniform_(-0.2, 0.2, generator=gen)
            m.running_var.uniform_(0.7, 1.3, generator=gen)
    sd = {k: v.clone() for k, v in head.state_dict().items()}
    side = int(round((SR.MODULE_RANGE[3] - SR.MODULE_RANGE[0]) / (SR.MODULE_VOXEL[0] * 8)))
    feats = np.clip(r.normal(0, 1, (3, 6, side, side)), -4, 4).astype(np.float32)
    ds = deep(SR.dataset_cfg(SR.MODULE_RANGE, SR.MODULE_VOXEL))
    out = dict(features=feats, sd_keys=np.array(list(sd.keys())))
    for k, v in sd.items():
        out["sd::" + k] = v.numpy()
    td = {k: torch.from_numpy(g31["A_" + k]) for k in G.TARGET_KEYS + ('gt_of_rois_src',)}
    for dt, dtag in ((torch.float32, "f32"), (torch.float64, "f64")):
        def fresh():
            h = ref_head(R, cfg)
            h.load_state_dict(sd, strict=True)
            return h.to(dt)
        x = torch.from_numpy(feats).to(dt)
        h = fresh().eval()
        bd = {'batch_size': 3, 'rois': torch.from_numpy(g30["A_rois"]).to(dt), 'roi_scores': torch.from_numpy(g30["A_roi_scores"]),
              'roi_labels': torch.from_numpy(g30["A_roi_labels"]), 'spatial_features_2d': x, 'dataset_cfg': ds}
        with dbl(dt), torch.no_grad():
            ev = h(bd)
        assert tuple(ev['batch_cls_preds'].shape) == (3, 96, 1) and ev['batch_box_preds'] is bd['rois'] and not ev['cls_preds_normalized']
        out[f"eval_{dtag}_batch_cls_preds"] = ev['batch_cls_preds'].numpy()
        h = fresh().train()
        tdt = {k: (v.clone().to(dt) if v.is_floating_point() else v.clone()) for k, v in td.items()}
        h.assign_targets = lambda batch_dict, _t=tdt: _t                   # the targets the reference recorded in g31
        bd = {'batch_size': 3, 'rois': torch.from_numpy(g30["A_rois"]).to(dt), 'roi_scores': torch.from_numpy(g30["A_roi_scores"]),
              'roi_labels': torch.from_numpy(g30["A_roi_labels"]), 'gt_boxes': torch.from_numpy(g30["A_gt_boxes"]).to(dt),
              'spatial_features_2d': x, 'dataset_cfg': ds}
        with dbl(dt):
            h(bd)
            loss, tb = h.get_loss()
            loss.backward()
        assert set(tb) == {'rcnn_loss_iou', 'rcnn_loss'} and abs(tb['rcnn_loss'] - float(loss)) < 1e-12
        out[f"train_{dtag}_rcnn_iou"] = h.forward_ret_dict['rcnn_iou'].detach().numpy()
        out[f"train_{dtag}_loss"] = np.array(float(loss), np.float64)
        for k, p in h.named_parameters():
            out[f"train_{dtag}_grad::{k}"] = p.grad.numpy()
        print(f"g45 {dtag}: loss {float(loss):.6f}, rcnn_iou in [{float(out[f'train_{dtag}_rcnn_iou'].min()):.3f}, "
              f"{float(out[f'train_{dtag}_rcnn_iou'].max()):.3f}]")
    save("g45_second_module", **out)


# ---------------------------------------------------------------------------------------------------------------------
def postproc_scene(r):
    """B = 2, K = 24: twelve boxes on a grid and, beside each, a close copy (IoU far above NMS_THRESH; different cells: 0)"""
    B, K = 2, 24
    boxes = np.zeros((B, K, 7), np.float32)
    # points: a wanted count inside each pair (below SCORE_THRESH.cls = 5, between 5 and 10 -- where the literal 10 makes
    # alpha negative --, between 10 and 60, above SCORE_THRESH.iou = 60), the rest scattered; 1000 in all
    want = np.array([[0, 2, 4, 6, 8, 9, 12, 25, 40, 59, 61, 75], [1, 3, 7, 0, 11, 14, 30, 64, 5, 8, 20, 90]])
    pts = []
    for b in range(B):
        cells = r.permutation(16)[:12]
        for k, cell in enumerate(cells):
            base = np.array([(cell % 4) * 10.0 + r.uniform(-1, 1), (cell // 4) * 10.0 - 15.0 + r.uniform(-1, 1), r.uniform(-1, 0),
                             r.uniform(3, 4.5), r.uniform(1.5, 2.2), r.uniform(1.4, 1.9), r.uniform(-2 * np.pi, 2 * np.pi)])
            twin = base.copy()
            twin[0:2] += r.uniform(-0.15, 0.15, 2)
            twin[3:6] *= r.uniform(0.95, 1.05, 3)
            twin[6] += r.uniform(-0.05, 0.05)
            boxes[b, k], boxes[b, 12 + k] = base, twin
            n = int(want[b, k])
            loc = r.uniform(-0.5, 0.5, (n, 3)) * base[3:6]                  # (near the faces some lie in one of the two only)
            ca, sa = np.cos(base[6]), np.sin(base[6])
            xy = np.stack([loc[:, 0] * ca - loc[:, 1] * sa, loc[:, 0] * sa + loc[:, 1] * ca], 1) + base[0:2]
            pts.append(np.concatenate([np.full((n, 1), b), xy, loc[:, 2:3] + base[2]], 1))
        boxes[b] = boxes[b, r.permutation(K)]
        n_bg = 500 - int(want[b].sum())
        pts.append(np.concatenate([np.full((n_bg, 1), b), r.uniform(-5, 35, (n_bg, 1)), r.uniform(-20, 20, (n_bg, 1)),
                                   r.uniform(-2, 1, (n_bg, 1))], 1))
    labels = np.stack([r.integers(1, 4, K), r.choice([1, 3], K)]).astype(np.int64)
    assert set(labels[0]) == {1, 2, 3} and set(labels[1]) == {1, 3}
    pts = np.concatenate(pts).astype(np.float32)
    pts = pts[r.permutation(len(pts))]                                      # frames interleaved
    for b in range(B):                                                      # the fixture condition: no point near a face
        m = pts[:, 0] == b
        while True:
            d = SR.box_face_distance(pts[m, 1:4], boxes[b]).min(axis=0)
            bad = np.nonzero(m)[0][d <= 10 * MARGIN]
            if not len(bad):
                break
            pts[bad, 1:4] += r.uniform(-0.05, 0.05, (len(bad), 3)).astype(np.float32)
    assert len(pts) == 1000
    iou_logits = r.normal(0.3, 1.5, (B, K, 1)).astype(np.float32)
    cls_logits = r.normal(0.3, 1.5, (B, K)).astype(np.float32)
    return boxes, labels, pts, iou_logits, cls_logits


def g46(R):
    from com_amd import roiaware_pool3d
    r = np.random.default_rng(46)
    names = SR.CLASS_NAMES
    while True:
        boxes, labels, pts, iou_logits, cls_logits = postproc_scene(r)
        counts = np.stack([roiaware_pool3d.points_in_boxes_cpu(pts[pts[:, 0] == b][:, 1:4], boxes[b]).sum(axis=1) for b in range(2)])
        ok = True
        for st in SR.SCORE_TYPES:
            cfg = SR.post_process_cfg(st)
            for b in range(2):
                s = SR.nms_scores(st, iou_logits[b, :, 0], cls_logits[b], labels[b], counts[b], cfg['NMS_CONFIG'], names)
                ok = ok and (np.abs(s - cfg['SCORE_THRESH']) > 10 * MARGIN).all()
                ok = ok and (np.diff(np.sort(s[s > 0])) > 1e-5).all()         # no tie decides an order
        for b in range(2):
            iou = bev_iou(boxes[b])
            ok = ok and (np.abs(iou[np.triu_indices(24, 1)] - SR.post_process_cfg(None)['NMS_CONFIG']['NMS_THRESH']) > 10 * MARGIN).all()
        if ok:
            break
    c = counts.reshape(-1)
    assert (c < 5).any() and ((c > 5) & (c < 10)).any() and ((c > 10) & (c < 60)).any() and (c >= 60).any(), c
    det = object.__new__(R.det.SECONDNetIoU)
    det.num_class, det.class_names = 3, names
    picked = []
    inner = R.det.class_agnostic_nms
    R.det.class_agnostic_nms = lambda **kw: picked.append(inner(**kw)) or picked[-1]
    out = dict(boxes=boxes, labels=labels, points=pts, iou_logits=iou_logits, cls_logits=cls_logits, counts=counts.astype(np.int32))
    for st in SR.SCORE_TYPES:
        det.model_cfg = D(POST_PROCESSING=deep(SR.post_process_cfg(st)))
        bd = {'batch_size': 2, 'batch_box_preds': torch.from_numpy(boxes), 'batch_cls_preds': torch.from_numpy(iou_logits),
              'roi_scores': torch.from_numpy(cls_logits), 'roi_labels': torch.from_numpy(labels), 'has_class_labels': True,
              'cls_preds_normalized': False, 'points': torch.from_numpy(pts), 'rois': torch.from_numpy(boxes)}
        del picked[:]
        pred, _ = det.post_processing(bd)
        for b in range(2):
            tag = f"{st or 'absent'}_{b}"
            out[f"{tag}_selected"] = picked[b][0].numpy().astype(np.int64)
            for k in ('pred_boxes', 'pred_scores', 'pred_labels', 'pred_cls_scores', 'pred_iou_scores'):
                out[f"{tag}_{k}"] = pred[b][k].numpy()
            assert np.array_equal(out[f"{tag}_pred_boxes"], boxes[b][out[f"{tag}_selected"]])
            print(f"g46 {tag}: {len(out[f'{tag}_selected'])} boxes kept, labels {sorted(set(out[f'{tag}_pred_labels'].tolist()))}")
    assert 3 not in out["score_by_class_1_pred_labels"] and 3 in out["iou_1_pred_labels"]       # the loop-bound quirk
    assert not np.array_equal(out["num_pts_iou_cls_0_pred_scores"], out["cls_0_pred_scores"])
    save("g46_second_postproc", **out)


if __name__ == "__main__":
    R = ref_classes()
    g43(R)
    g44(R)
    g45(R)
    g46(R)
    with open(os.path.join(HERE, "MANIFEST_second_head.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
