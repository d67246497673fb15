#!/usr/bin/env python3
"""Generate the Voxel R-CNN fixtures under tests/golden/ (run once, where the reference lies at /root/reference; not needed
at test time).  In the style of make_golden_roi_head.py: the reference's own voxel_pool_modules.py, voxelrcnn_head.py,
roi_head_template.py and common_utils.py are imported from their read-only location under stand-in parent packages and run
on the CPU; only arrays (data) are stored.  The compiled `voxel_query_utils` is replaced by a stand-in written here: the
query is oracle.voxel_query_stack, the grouping is plain indexing with the global rows it returns.

  g34_voxel_pool        the inputs of the two NeighborVoxelSAModuleMSG of the head below (one per level, two scales each) as the
                        reference's roi_grid_pool hands them over, idx / empty mask per (level, scale), the module outputs in
                        training and eval mode, the running statistics after the training step and the gradients of
                        sum(out * probe) with respect to `features` and every parameter -- in f32 and fp64
  g35_voxel_rcnn_head   the reference's VoxelRCNNHead from a stored state dict (DP_RATIO 0) on given rois / roi_targets_dict:
                        pooled features, rcnn_cls, rcnn_reg in training and eval mode, decoded boxes, loss scalars and
                        parameter gradients -- in f32 and fp64

B = 2, levels x_conv1 (5, 12, 14) at stride 1 and x_conv2 (3, 6, 7) at stride 2, 6 RoIs per frame, GRID_SIZE 3: M = 324.
Scales: (nsample 16, 32 channels, range [4, 4, 4]) and (nsample 5, 24 channels, range [1, 2, 3]).

Drawn again until (the last four re-asserted from the stored arrays by tests/test_voxel_pool_cpu.py): every (level, scale) has
queries with 0 hits, with 1 .. nsample hits and with more than nsample hits; grid points leave the grid on each of its six
sides; every squared distance of a probed voxel is more than 1e-4 from radius^2; every grid-point coordinate is more than
1e-4 of a voxel from a cell boundary; per (m, c) the best and second-best activation among the distinct slots are more than
1e-4 apart when the best is positive, and the best is more than 1e-4 from 0 (training and eval mode, fp64).

For the fp64 values the reference's code runs with `Tensor.float()` left as the identity on fp64 tensors.

Usage: python tests/golden/make_golden_voxel_rcnn.py
"""
import contextlib
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import oracle as O  # noqa: E402
import make_golden_roi_head as G  # noqa: E402  (stand-in packages, keep_double, save, D)

REF = G.REF
D = G.D
MARGIN = 1e-4
B, R, GRID = 2, 6, 3
PCR = [0.0, 0.0, 0.0, 7.0, 6.0, 3.0]
VOXEL = [0.5, 0.5, 0.6]
LEVELS = {'x_conv1': dict(stride=1, shape=(5, 12, 14), channels=6, radii=[1.2, 0.9]),
          'x_conv2': dict(stride=2, shape=(3, 6, 7), channels=10, radii=[2.4, 1.8])}
SCALES = [dict(nsample=16, mid=32, rng=[4, 4, 4]), dict(nsample=5, mid=24, rng=[1, 2, 3])]
OUT_WIDTH = 8


def model_cfg():
    layers = D({src: D(MLPS=[[s['mid'], OUT_WIDTH] for s in SCALES], QUERY_RANGES=[s['rng'] for s in SCALES],
                       POOL_RADIUS=list(lv['radii']), NSAMPLE=[s['nsample'] for s in SCALES], POOL_METHOD='max_pool')
                for src, lv in LEVELS.items()})
    c = G.model_cfg()
    c.update(NAME='VoxelRCNNHead', SHARED_FC=[16, 16], CLS_FC=[16, 16], REG_FC=[16, 16], DP_RATIO=0.0,
             ROI_GRID_POOL=D(FEATURES_SOURCE=list(LEVELS), GRID_SIZE=GRID, POOL_LAYERS=layers))
    c['TARGET_CONFIG'] = D(c['TARGET_CONFIG'], ROI_PER_IMAGE=R)
    return c


def plain(cfg):
    """the configuration as plain dicts / lists (stored in the fixture as JSON: settings only)"""
    if isinstance(cfg, dict):
        return {k: plain(v) for k, v in cfg.items()}
    return [plain(v) for v in cfg] if isinstance(cfg, (list, tuple)) else cfg


# ---------------------------------------------------------------------------------------------------------------------
QUERIES = []            # what the stand-in recorded: (max_range, radius, nsample, idx, empty)
_CACHE = {}


class VoxelQueryAndGrouping(torch.nn.Module):
    """stand-in for voxel_query_utils.VoxelQueryAndGrouping (voxel_query_utils.py:51-100): oracle query, indexing"""

    def __init__(self, max_range, radius, nsample):
        super().__init__()
        self.max_range, self.radius, self.nsample = max_range, radius, nsample

    def forward(self, new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, voxel2point_indices):
        args = (xyz.detach().float().numpy(), new_xyz.detach().float().numpy(), new_coords.numpy(), voxel2point_indices.numpy())
        key = (tuple(self.max_range), self.radius, self.nsample) + tuple(a.tobytes() for a in args)
        if key not in _CACHE:
            _CACHE[key] = O.voxel_query_stack(self.max_range, self.radius, self.nsample, *args)
        idx, empty = _CACHE[key]
        QUERIES.append((tuple(self.max_range), self.radius, self.nsample, idx, empty))
        rows = torch.from_numpy(idx).long()
        return features[rows].permute(0, 2, 1).contiguous(), xyz[rows].permute(0, 2, 1).contiguous(), torch.from_numpy(empty)


def ref_modules():
    Rm = G.ref_modules()
    stub = G._ns("pcdet.ops.pointnet2.pointnet2_stack.voxel_query_utils", None, VoxelQueryAndGrouping=VoxelQueryAndGrouping)
    G._ns("pcdet.ops.pointnet2", REF + "/ops/pointnet2")
    G._ns("pcdet.ops.pointnet2.pointnet2_stack", REF + "/ops/pointnet2/pointnet2_stack", voxel_query_utils=stub)
    Rm.pool = importlib.import_module("pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules")
    Rm.head = importlib.import_module("pcdet.models.roi_heads.voxelrcnn_head")
    Rm.cu = importlib.import_module("pcdet.utils.common_utils")
    return Rm


# ---------------------------------------------------------------------------------------------------------------------
def draw_geometry(r):
    levels = {}
    Z, Y, X = LEVELS['x_conv1']['shape']
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij')
    rows = []
    for b in range(B):
        p = np.where(xx < 8, 0.62, 0.07)
        keep = r.random((Z, Y, X)) < p
        rows.append(np.stack([np.full(keep.sum(), b), zz[keep], yy[keep], xx[keep]], 1))
    c1 = np.concatenate(rows).astype(np.int32)
    c2 = np.unique(np.concatenate([c1[:, :1], c1[:, 1:] // 2], 1), axis=0).astype(np.int32)
    for src, c in (('x_conv1', c1), ('x_conv2', c2)):
        c = c[r.permutation(len(c))]                                  # rows in no particular order (hash order on the device)
        levels[src] = dict(indices=c, features=r.normal(0, 1, (len(c), LEVELS[src]['channels'])).astype(np.float32))
    return levels


def draw_roi(r, side):
    """one RoI; side 0..5: its centre just outside the range at x-, x+, y-, y+, z-, z+ (grid points leave the grid there)"""
    roi = np.array([r.uniform(0.3, 6.7), r.uniform(0.3, 5.7), r.uniform(0.3, 2.7), r.uniform(1.0, 3.0), r.uniform(0.8, 2.4),
                    r.uniform(0.8, 2.0), r.uniform(-np.pi, np.pi)], np.float32)
    if side is not None:
        roi[side // 2] = (PCR[3 + side // 2] + 0.15) if side % 2 else -0.15
    return roi


def draw_rois(Rm, head, levels, r):
    """RoI after RoI, each drawn until its grid points keep the margins to the cell boundaries and the radii"""
    rois = np.zeros((B, R, 7), np.float32)
    for b in range(B):
        for i in range(R):
            for _ in range(500):
                cand = draw_roi(r, i if b == 0 else None)
                trial = np.broadcast_to(cand, (B, R, 7)).copy()
                if margins_ok(pool_inputs(Rm, head, levels, trial, torch.float32)) is None:
                    rois[b, i] = cand
                    break
            else:
                raise RuntimeError("no RoI")
    return rois


def sp_tensors(levels, dt):
    return {src: types.SimpleNamespace(indices=torch.from_numpy(lv['indices']), features=torch.from_numpy(lv['features']).to(dt),
                                       spatial_shape=list(LEVELS[src]['shape']), batch_size=B) for src, lv in levels.items()}


def hits_all(xyz, new_xyz, new_coords, v2p, rng, radius):
    """per query: every squared distance of a voxel in the clipped window (numpy restatement of the probe loop)"""
    out = []
    Bn, R1, R2, R3 = v2p.shape
    for q in range(len(new_coords)):
        b, cz, cy, cx = [int(v) for v in new_coords[q]]
        z0, z1 = max(cz - rng[0], 0), min(cz + rng[0], R1 - 1)
        y0, y1 = max(cy - rng[1], 0), min(cy + rng[1], R2 - 1)
        x0, x1 = max(cx - rng[2], 0), min(cx + rng[2], R3 - 1)
        if z0 > z1 or y0 > y1 or x0 > x1:
            out.append(np.zeros(0))
            continue
        nb = v2p[b, z0:z1 + 1, y0:y1 + 1, x0:x1 + 1].reshape(-1)
        nb = nb[nb >= 0]
        d = xyz[nb].astype(np.float64) - new_xyz[q].astype(np.float64)
        out.append((d * d).sum(1))
    return out


def build_head(Rm, dt, state=None):
    head = Rm.head.VoxelRCNNHead(backbone_channels={s: lv['channels'] for s, lv in LEVELS.items()}, model_cfg=model_cfg(),
                                 point_cloud_range=PCR, voxel_size=VOXEL, num_class=1)
    if state is not None:
        head.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return head.to(dt)


def draw_state(Rm):
    """a state dict away from the initialisation: BatchNorm scales, shifts and running statistics drawn, the last layers
    large enough for the loss to see them"""
    torch.manual_seed(35)
    head = build_head(Rm, torch.float32)
    g = torch.Generator().manual_seed(36)
    sd = head.state_dict()
    for k, v in sd.items():
        if k.endswith('running_mean') or (k.endswith('.bias') and v.dim() == 1 and 'pred_layer' not in k):
            v.copy_(torch.randn(v.shape, generator=g) * 0.3)
        elif k.endswith('running_var'):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif k.endswith('.weight') and v.dim() == 1:
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif 'pred_layer.weight' in k:
            v.copy_(torch.randn(v.shape, generator=g) * 0.2)
    return {k: v.numpy().copy() for k, v in sd.items()}


def pool_inputs(Rm, head, levels, rois, dt):
    """the keyword arguments the reference's roi_grid_pool passes to each pool layer"""
    calls = []
    originals = [m.forward for m in head.roi_grid_pool_layers]
    for m in head.roi_grid_pool_layers:
        m.forward = lambda _c=calls, **kw: _c.append(kw) or torch.zeros((kw['new_xyz'].shape[0], 2 * OUT_WIDTH), dtype=dt)
    head.roi_grid_pool({'batch_size': B, 'rois': torch.from_numpy(rois).to(dt), 'multi_scale_3d_features': sp_tensors(levels, dt),
                        'multi_scale_3d_strides': {s: lv['stride'] for s, lv in LEVELS.items()}})
    for m, f in zip(head.roi_grid_pool_layers, originals):
        m.forward = f
    return calls


def margins_ok(calls):
    new_xyz = calls[0]['new_xyz'].numpy()
    frac = (new_xyz - np.asarray(PCR[:3], np.float32)) / np.asarray(VOXEL, np.float32)
    frac = frac - np.floor(frac)
    if (np.minimum(frac, 1 - frac) <= 3 * MARGIN).any():
        return "grid point on a cell boundary"
    for call, lv in zip(calls, LEVELS.values()):
        xyz, nc, v2p = call['xyz'].numpy(), call['new_coords'].numpy()[:, [0, 3, 2, 1]], call['voxel2point_indices'].numpy()
        for s, radius in zip(SCALES, lv['radii']):
            d2 = hits_all(xyz, call['new_xyz'].numpy(), nc, v2p, s['rng'], radius)
            if any((np.abs(d - radius * radius) <= 3 * MARGIN).any() for d in d2):
                return "distance on the radius"
    return None


def geometry_ok(calls):
    why = margins_ok(calls)
    if why:
        return why
    c = calls[0]['new_coords'].numpy()                                  # (b, x, y, z) at level 0
    Z, Y, X = LEVELS['x_conv1']['shape']
    sides = [(c[:, 1] < 0).any(), (c[:, 1] >= X).any(), (c[:, 2] < 0).any(), (c[:, 2] >= Y).any(), (c[:, 3] < 0).any(),
             (c[:, 3] >= Z).any()]
    if not all(sides):
        return f"sides {sides}"
    for call, (src, lv) in zip(calls, LEVELS.items()):
        xyz, nc, v2p = call['xyz'].numpy(), call['new_coords'].numpy()[:, [0, 3, 2, 1]], call['voxel2point_indices'].numpy()
        for s, radius in zip(SCALES, lv['radii']):
            d2 = hits_all(xyz, call['new_xyz'].numpy(), nc, v2p, s['rng'], radius)
            n = np.array([(d <= radius * radius).sum() for d in d2])
            if not ((n == 0).any() and ((n >= 1) & (n <= s['nsample'])).any() and (n > s['nsample']).any()):
                return f"{src} nsample {s['nsample']}: hit counts {np.bincount(np.minimum(n, s['nsample'] + 1))}"
    return None


def activations(layer, call):
    """pre-ReLU activations [C, M, nsample] per scale of one forward of a reference pool layer (a hook on its ReLU)"""
    got = []
    h = layer.relu.register_forward_hook(lambda m, i, o: got.append(i[0].detach()[0].numpy().copy()))
    out = layer(**call)
    h.remove()
    return out, got


def margins(act, idx, empty, nsample):
    """per (m, c): the best activation among the distinct slots and its distance to the second best (inf when there is one)"""
    C, M, _ = act.shape
    first = idx[:, :1]
    cnt = np.where(empty, 1, 1 + (idx[:, 1:] != first).sum(1))          # distinct hits are distinct rows
    live = np.arange(nsample)[None, :] < cnt[:, None]
    a = np.where(live[None], act, -np.inf)
    srt = np.sort(a, axis=2)
    best, second = srt[:, :, -1], srt[:, :, -2] if nsample > 1 else np.full((C, M), -np.inf)
    return best.T, (best - second).T, cnt, np.argmax(a, axis=2).T


def bad_entries(best, gap):
    return (np.abs(best) <= 1.1 * MARGIN) | ((best > 0) & (gap <= 1.1 * MARGIN))


def repair_features(Rm, state, levels, rois, r):
    """redraw the feature rows behind an activation that is too close to the runner-up or to 0 until none is left (training
    mode, then eval mode with the statistics that step left, fp64)"""
    for it in range(400):
        head = build_head(Rm, torch.float64, state)
        with G.keep_double():
            calls = pool_inputs(Rm, head, levels, rois, torch.float64)
            bad_rows = {src: set() for src in LEVELS}
            for layer, call, src in zip(head.roi_grid_pool_layers, calls, LEVELS):
                for mode in (True, False):
                    layer.train(mode)
                    QUERIES.clear()
                    _, acts = activations(layer, call)
                    for act, (_, _, ns, idx, empty) in zip(acts, list(QUERIES)):
                        best, gap, _, win = margins(act, idx, empty, ns)
                        for m, c in zip(*np.nonzero(bad_entries(best, gap))):
                            bad_rows[src].add(int(idx[m, win[m, c]]))        # the winner's row (an empty ball: BN(0), row 0)
        n_bad = sum(len(v) for v in bad_rows.values())
        print(f"repair {it}: rows to redraw {n_bad}")
        if n_bad == 0:
            return
        for src, rows in bad_rows.items():
            rows = sorted(rows)
            levels[src]['features'][rows] = r.normal(0, 1, (len(rows), LEVELS[src]['channels'])).astype(np.float32)
    raise RuntimeError("repair did not converge")


def targets(rois, r):
    """what ProposalTargetLayer would return for rois that are all kept: jittered GT rows, half of them regression targets"""
    gt = np.zeros((B, R, 8), np.float32)
    gt[..., :7] = rois
    gt[..., 0:3] += r.normal(0, 0.15, (B, R, 3)).astype(np.float32)
    gt[..., 3:6] *= (1 + r.normal(0, 0.08, (B, R, 3))).astype(np.float32)
    gt[..., 6] += r.normal(0, 0.2, (B, R)).astype(np.float32)
    gt[..., 6] += np.where(r.random((B, R)) < 0.3, np.pi, 0).astype(np.float32)
    gt[..., 7] = 1
    iou = r.uniform(0.05, 0.95, (B, R)).astype(np.float32)
    return {'rois': torch.from_numpy(rois.copy()), 'gt_of_rois': torch.from_numpy(gt), 'gt_iou_of_rois': torch.from_numpy(iou),
            'roi_scores': torch.from_numpy(r.uniform(0, 1, (B, R)).astype(np.float32)),
            'roi_labels': torch.ones((B, R), dtype=torch.int64), 'reg_valid_mask': torch.from_numpy((iou > 0.55).astype(np.int64)),
            'rcnn_cls_labels': torch.from_numpy(np.clip((iou - 0.25) / 0.5, 0, 1).astype(np.float32))}


def run_pool(Rm, state, levels, rois, probes, dt, out):
    tag = "f32" if dt == torch.float32 else "f64"
    head = build_head(Rm, dt, state)
    calls = pool_inputs(Rm, head, levels, rois, dt)
    for k, (layer, call, src) in enumerate(zip(head.roi_grid_pool_layers, calls, LEVELS)):
        feats = call['features'].clone().requires_grad_(True)
        call = dict(call, features=feats)
        layer.train()
        QUERIES.clear()
        y = layer(**call)
        if tag == "f32":
            for s, (_, _, ns, idx, empty) in enumerate(list(QUERIES)):
                out[f"{src}_idx{s}"], out[f"{src}_empty{s}"] = idx, empty
            out[f"{src}_xyz"], out[f"{src}_new_coords"] = call['xyz'].numpy(), call['new_coords'].numpy()
            out[f"{src}_v2p"] = call['voxel2point_indices'].numpy().astype(np.int32)
            out["new_xyz"] = call['new_xyz'].numpy()
        (y * torch.from_numpy(probes[src]).to(dt)).sum().backward()
        out[f"{src}_train_{tag}"] = y.detach().numpy()
        out[f"{src}_dfeatures_{tag}"] = feats.grad.numpy()
        for name, p in layer.named_parameters():
            out[f"{src}_grad.{name}_{tag}"] = p.grad.numpy()
        for name, b in layer.named_buffers():
            out[f"{src}_after.{name}_{tag}"] = b.detach().numpy().copy()
        layer.eval()
        out[f"{src}_eval_{tag}"] = layer(**call).detach().numpy()


def run_head(Rm, state, levels, rois, td, dt, out):
    tag = "f32" if dt == torch.float32 else "f64"
    head = build_head(Rm, dt, state)
    head.train()
    td_in = {k: (v.clone().to(dt) if v.is_floating_point() else v.clone()) for k, v in td.items()}
    head.proposal_target_layer.forward = lambda batch_dict, _t=td_in: dict(_t)
    pooled = []
    inner = head.roi_grid_pool
    head.roi_grid_pool = lambda bd: pooled.append(inner(bd)) or pooled[-1]

    def bd():
        return {'batch_size': B, 'rois': torch.from_numpy(rois).to(dt), 'roi_scores': td_in['roi_scores'].clone(),
                'roi_labels': td_in['roi_labels'].clone(), 'multi_scale_3d_features': sp_tensors(levels, dt),
                'multi_scale_3d_strides': {s: lv['stride'] for s, lv in LEVELS.items()}}
    head(bd())
    f = head.forward_ret_dict
    loss, tb = head.get_loss()
    loss.backward()
    out[f"train_pooled_{tag}"], out[f"train_rcnn_cls_{tag}"] = pooled[0].detach().numpy(), f['rcnn_cls'].detach().numpy()
    out[f"train_rcnn_reg_{tag}"] = f['rcnn_reg'].detach().numpy()
    out[f"scalars_{tag}"] = np.array([float(loss), tb['rcnn_loss_cls'], tb['rcnn_loss_reg'], tb['rcnn_loss_corner']], np.float64)
    for name, p in head.named_parameters():
        out[f"grad.{name}_{tag}"] = p.grad.numpy()
    for name, b in head.named_buffers():
        out[f"after.{name}_{tag}"] = b.detach().numpy().copy()
    if tag == "f32":
        for k in ('rois', 'gt_of_rois', 'gt_of_rois_src', 'reg_valid_mask', 'rcnn_cls_labels', 'roi_labels'):
            out[f"targets_{k}"] = f[k].detach().numpy()
    head.eval()
    ev = head(bd())
    out[f"eval_pooled_{tag}"], out[f"eval_box_preds_{tag}"] = pooled[1].detach().numpy(), ev['batch_box_preds'].detach().numpy()
    out[f"eval_cls_preds_{tag}"] = ev['batch_cls_preds'].detach().numpy()


if __name__ == "__main__":
    Rm = ref_modules()
    state = draw_state(Rm)
    for seed in range(34, 200):
        r = np.random.default_rng(seed)
        levels = draw_geometry(r)
        probe_head = build_head(Rm, torch.float32, state)
        rois = draw_rois(Rm, probe_head, levels, r)
        why = geometry_ok(pool_inputs(Rm, probe_head, levels, rois, torch.float32))
        print(f"seed {seed}: {why or 'geometry ok'}")
        if why is None:
            break
    else:
        raise RuntimeError("no geometry")
    repair_features(Rm, state, levels, rois, r)
    probes = {src: r.normal(0, 1, (B * R * GRID ** 3, 2 * OUT_WIDTH)).astype(np.float32) for src in LEVELS}
    cfg_json = np.frombuffer(json.dumps(plain(model_cfg())).encode(), np.uint8)
    g34 = dict(rois=rois, model_cfg_json=cfg_json, radii=np.array([lv['radii'] for lv in LEVELS.values()]))
    for src, lv in levels.items():
        g34[f"{src}_indices"], g34[f"{src}_features"], g34[f"{src}_probe"] = lv['indices'], lv['features'], probes[src]
    for k, v in state.items():
        if k.startswith("roi_grid_pool_layers."):
            g34["state." + k[len("roi_grid_pool_layers."):]] = v
    for dt in (torch.float32, torch.float64):
        with (G.keep_double() if dt == torch.float64 else contextlib.nullcontext()):
            run_pool(Rm, state, levels, rois, probes, dt, g34)
    G.save("g34_voxel_pool", **g34)
    td = targets(rois, r)
    g35 = dict(rois=rois, model_cfg_json=cfg_json, state_keys_json=np.frombuffer(json.dumps(
        {k: list(v.shape) for k, v in state.items()}).encode(), np.uint8))
    g35.update({"state." + k: v for k, v in state.items()})
    for dt in (torch.float32, torch.float64):
        with (G.keep_double() if dt == torch.float64 else contextlib.nullcontext()):
            run_head(Rm, state, levels, rois, td, dt, g35)
    G.save("g35_voxel_rcnn_head", **g35)
    print("g35 scalars f64", g35["scalars_f64"], "f32 - f64", g35["scalars_f32"] - g35["scalars_f64"])
    with open(os.path.join(HERE, "MANIFEST_voxel_rcnn.json"), "w") as f:
        json.dump(G.manifest, f, indent=1, sort_keys=True)
