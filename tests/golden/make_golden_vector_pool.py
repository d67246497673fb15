#!/usr/bin/env python3
"""Generate the VectorPool fixtures under tests/golden/ (run once, where the reference lies at /root/reference; not needed at
test time).  In the style of make_golden_voxel_rcnn.py: the reference's own pointnet2_modules.py and pointnet2_utils.py are
imported from their read-only location under stand-in parent packages and run on the CPU; only arrays and the JSON
configurations (data) are stored.  The compiled `pointnet2_stack_cuda` is replaced by a stand-in written here over
tests/vector_pool_ref.py (the numpy restatement of vector_pool_gpu.cu) plus a plain three-interpolate.

  g36_vector_pool_ops       B = 2 frames of 1150 and 90 support rows, 41 and 23 queries; per configuration of
                            vector_pool_ref.OPS the three-NN (idx, dist2, neighbor_cnt, at 2 x the distance) and the voxel query
                            (new_features, new_local_xyz, point_cnt_of_grid, src_row) of the restatement
  g37_vector_pool_modules   the reference's VectorPoolAggregationModuleMSG, two groups, as local_interpolation (6 -> 3 channels)
                            and as voxel_random_choice (4 channels, NEIGHBOR_NSAMPLE 32) from stored state dicts on that
                            geometry: outputs in training and eval mode, the running statistics after the step, the gradients of
                            sum(out * probe) with respect to `features` and every parameter -- in f32 and fp64

Support rows are drawn again (the rows behind a violation only) until: every |local_a| and every squared distance lies more
than 1e-5 (relative) from the query distances; every (local_a + R) / grid_size_a of a hit is more than 1e-5 from an integer;
per (m, g) the four smallest distances of the list differ pairwise by more than 1e-6 relative.  By construction, and checked:
queries with 0, 1, 2, 3 and more neighbours, one with more than 1000 rows within the distance, one whose neighbours all lie in
the other frame.

For the fp64 values the reference's code runs with `Tensor.float()` left as the identity on fp64 tensors.

Usage: python tests/golden/make_golden_vector_pool.py
"""
import contextlib
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_roi_head as G  # noqa: E402  (stand-in packages, keep_double, save, D)
import vector_pool_ref as V  # noqa: E402

REF = G.REF
F = np.float32
CNT, NEW_CNT = [1150, 90], [41, 23]
CA, CB = np.array([2.0, 3.0, 1.0]), np.array([12.0, 3.0, 1.0])       # the dense cluster of frame 0, the loose one of frame 1
ISLES = [np.array([-6.0, -6.0, 0.0]), np.array([-6.0, 0.0, 0.0]), np.array([-6.0, 6.0, 0.0])]   # 1, 2 and 3 rows, far from all


class D(dict):
    """EasyDict enough for the reference's constructors (attribute access, nested)"""

    def __init__(self, d):
        super().__init__({k: D(v) if isinstance(v, dict) else v for k, v in d.items()})

    __getattr__ = dict.__getitem__


# ---------------------------------------------------------------------------------------------------------------------
class Stub:
    """pointnet2_stack_cuda: the wrappers pointnet2_utils.py calls, over the numpy restatement"""

    @staticmethod
    def query_stacked_local_neighbor_idxs_wrapper_stack(sxyz, cnt, nxyz, ncnt, stack, start_len, cumsum, avg, dist, nsample, ntype):
        lists, _ = V.neighbor_lists(sxyz.numpy().astype(F), cnt.numpy(), nxyz.numpy().astype(F), ncnt.numpy(), F(dist), nsample, ntype)
        at = 0
        for m, rows in enumerate(lists):
            start_len[m, 0], start_len[m, 1] = at, len(rows)
            if at + len(rows) <= stack.shape[0]:
                stack[at:at + len(rows)] = torch.from_numpy(rows.astype(np.int32))
            at += len(rows)
        cumsum[0] = at

    @staticmethod
    def query_three_nn_by_stacked_local_idxs_wrapper_stack(sxyz, nxyz, centers, idxs, dist2, stack, start_len, M, G):
        for m in range(M):
            s, n = int(start_len[m, 0]), int(start_len[m, 1])
            if n == 0:
                dist2[m] = float("inf")                                  # (the kernel's 1e40 stored as float)
                continue
            rows = stack[s:s + n].long()
            c, p = centers[m][:, None, :], sxyz[rows][None, :, :]
            d = ((c[..., 0] - p[..., 0]) * (c[..., 0] - p[..., 0]) + (c[..., 1] - p[..., 1]) * (c[..., 1] - p[..., 1])) \
                + (c[..., 2] - p[..., 2]) * (c[..., 2] - p[..., 2])
            order = torch.from_numpy(np.argsort(d.numpy(), axis=1, kind="stable")[:, :3])
            if order.shape[1] < 3:
                order = torch.cat([order, order[:, :1].repeat(1, 3 - order.shape[1])], dim=1)
            idxs[m] = rows[order].int()
            dist2[m] = torch.gather(d, 1, order)

    @staticmethod
    def three_interpolate_wrapper(features, idx, weight, out):
        out.copy_(V.three_interpolate(features, idx.long(), weight))

    @staticmethod
    def three_interpolate_grad_wrapper(grad_out, idx, weight, grad_features):
        for k in range(3):
            grad_features.index_add_(0, idx[:, k].long(), grad_out * weight[:, k:k + 1])

    @staticmethod
    def vector_pool_wrapper(sxyz, cnt, feats, nxyz, ncnt, new_features, new_local_xyz, point_cnt, grouped, gx, gy, gz, dist, use_xyz,
                            num_max_sum_points, nsample, ntype, pooling_type):
        assert pooling_type == 1 and use_xyz
        dt = np.float64 if feats.dtype == torch.float64 else F
        out, loc, pc, src = V.voxel_query(sxyz.numpy(), cnt.numpy(), feats.detach().numpy(), nxyz.numpy(), ncnt.numpy(), (gx, gy, gz),
                                          dist, nsample, ntype, dtype=dt)
        new_features.copy_(torch.from_numpy(out)), new_local_xyz.copy_(torch.from_numpy(loc)), point_cnt.copy_(torch.from_numpy(pc))
        m, g = np.nonzero(src >= 0)
        n = len(m)
        if n <= grouped.shape[0]:
            grouped[:n] = torch.from_numpy(np.stack([src[m, g], m, g], 1).astype(np.int32))
        return n

    @staticmethod
    def vector_pool_grad_wrapper(grad_new, point_cnt, grouped, grad_support):
        G_ = point_cnt.shape[1]
        c = grad_new.shape[1] // G_
        g3 = grad_new.view(grad_new.shape[0], G_, c)
        grad_support.index_add_(0, grouped[:, 0].long(), g3[grouped[:, 1].long(), grouped[:, 2].long()])


def ref_modules():
    G._ns("pcdet", REF)
    G._ns("pcdet.ops", REF + "/ops")
    G._ns("pcdet.ops.pointnet2", REF + "/ops/pointnet2")
    stub = G._ns("pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda", None,
                 **{k: getattr(Stub, k) for k in dir(Stub) if not k.startswith("_")})
    G._ns("pcdet.ops.pointnet2.pointnet2_stack", REF + "/ops/pointnet2/pointnet2_stack", pointnet2_stack_cuda=stub)
    return importlib.import_module("pcdet.ops.pointnet2.pointnet2_stack.pointnet2_modules")


# ---------------------------------------------------------------------------------------------------------------------
def draw_row(r, i):
    """support row i: frame 0 = the dense cluster (1060 rows in a box of side 0.8: all within every doubled distance of its
    centre), the isles of 1 / 2 / 3 rows, a sparse field; frame 1 = a loose cluster, a sparse field"""
    if i < 1060:
        return CA + r.uniform(-0.4, 0.4, 3)
    if i < 1066:
        isle = ISLES[[0, 1, 1, 2, 2, 2][i - 1060]]
        return isle + r.uniform(-0.3, 0.3, 3)
    if i < CNT[0]:
        return np.array([r.uniform(4.5, 9.5), r.uniform(-2, 8), r.uniform(-0.5, 2.5)])
    if i < CNT[0] + 60:
        return CB + r.uniform(-0.7, 0.7, 3)
    return np.array([r.uniform(14, 18), r.uniform(-2, 8), r.uniform(-0.5, 2.5)])


def draw_queries(r):
    q0 = [CA + r.uniform(-0.02, 0.02, 3)]                                               # sees more than 1000 rows
    q0 += [isle + r.uniform(-0.05, 0.05, 3) for isle in ISLES]                          # 1, 2, 3 neighbours
    q0 += [np.array([-12.0, -12.0, 5.0])]                                               # none
    q0 += [CA + r.uniform(-0.9, 0.9, 3) for _ in range(16)]
    q0 += [np.array([r.uniform(4.5, 9.5), r.uniform(-2, 8), r.uniform(-0.5, 2.5)]) for _ in range(NEW_CNT[0] - len(q0))]
    q1 = [CA + r.uniform(-0.02, 0.02, 3)]                                               # every neighbour in the other frame
    q1 += [CB + r.uniform(-1.0, 1.0, 3) for _ in range(14)]
    q1 += [np.array([r.uniform(14, 18), r.uniform(-2, 8), r.uniform(-0.5, 2.5)]) for _ in range(NEW_CNT[1] - len(q1))]
    return np.array(q0 + q1, F)


def draw_geometry(r):
    new_xyz = draw_queries(r)
    sxyz = np.array([draw_row(r, i) for i in range(sum(CNT))], F)
    for it in range(200):
        bad = V.fixture_violations(sxyz, CNT, new_xyz, NEW_CNT)
        print(f"repair {it}: rows to redraw {len(bad)}")
        if not bad:
            return sxyz, new_xyz
        for i in bad:
            sxyz[i] = draw_row(r, i)
    raise RuntimeError("repair did not converge")


def counts_ok(sxyz, new_xyz):
    for num_grid, dist, ntype, nsample in V.OPS:
        _, full = V.neighbor_lists(sxyz, CNT, new_xyz, NEW_CNT, F(V.MULTIPLIER * dist), -1, ntype)
        assert all((full == k).any() for k in (0, 1, 2, 3)) and (full > 3).any() and (full > V.CAP).any(), np.bincount(np.minimum(full, 5))
        assert full[NEW_CNT[0]] == 0
        _, other = V.neighbor_lists(sxyz, [sum(CNT)], new_xyz[NEW_CNT[0]:NEW_CNT[0] + 1], [1], F(V.MULTIPLIER * dist), -1, ntype)
        assert other[0] > V.CAP


# ---------------------------------------------------------------------------------------------------------------------
def draw_state(Rm, c_in, cfg, seed):
    torch.manual_seed(seed)
    mod = Rm.VectorPoolAggregationModuleMSG(input_channels=c_in, config=D(json.loads(json.dumps(cfg))))
    g = torch.Generator().manual_seed(seed + 1)
    sd = mod.state_dict()
    for k, v in sd.items():
        if k.endswith('running_mean') or (k.endswith('.bias') and v.dim() == 1):
            v.copy_(torch.randn(v.shape, generator=g) * 0.3)
        elif k.endswith('running_var') or (k.endswith('.weight') and v.dim() == 1):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
    return {k: v.numpy().copy() for k, v in sd.items()}


def run_module(Rm, kind, c_in, cfg, state, geo, feats, probe, dt, out):
    tag = "f32" if dt == torch.float32 else "f64"
    mod = Rm.VectorPoolAggregationModuleMSG(input_channels=c_in, config=D(json.loads(json.dumps(cfg))))
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    mod = mod.to(dt)
    f = torch.from_numpy(feats).to(dt).requires_grad_(True)
    kw = dict(xyz=torch.from_numpy(geo[0]).to(dt), xyz_batch_cnt=torch.tensor(CNT, dtype=torch.int32),
              new_xyz=torch.from_numpy(geo[1]).to(dt), new_xyz_batch_cnt=torch.tensor(NEW_CNT, dtype=torch.int32), features=f)
    mod.train()
    _, y = mod(**kw)
    (y * torch.from_numpy(probe).to(dt)).sum().backward()
    out[f"{kind}_train_{tag}"] = y.detach().numpy()
    out[f"{kind}_dfeatures_{tag}"] = f.grad.numpy()
    for name, p in mod.named_parameters():
        out[f"{kind}_grad.{name}_{tag}"] = p.grad.numpy()
    for name, b in mod.named_buffers():
        out[f"{kind}_after.{name}_{tag}"] = b.detach().numpy().copy()
    mod.eval()
    out[f"{kind}_eval_{tag}"] = mod(**kw)[1].detach().numpy()


if __name__ == "__main__":
    Rm = ref_modules()
    r = np.random.default_rng(36)
    sxyz, new_xyz = draw_geometry(r)
    counts_ok(sxyz, new_xyz)
    feats = r.normal(0, 1, (sum(CNT), V.OP_CHANNELS)).astype(F)
    g36 = dict(support_xyz=sxyz, xyz_batch_cnt=np.array(CNT, np.int32), new_xyz=new_xyz, new_xyz_batch_cnt=np.array(NEW_CNT, np.int32),
               support_features=feats, ops_json=np.frombuffer(json.dumps(V.OPS).encode(), np.uint8))
    for k, (num_grid, dist, ntype, nsample) in enumerate(V.OPS):
        centers = new_xyz[:, None, :] + V.dense_offsets(dist, num_grid)[None]
        g36[f"op{k}_centers"] = centers
        g36[f"op{k}_idx"], g36[f"op{k}_dist2"], g36[f"op{k}_neighbor_cnt"] = V.three_nn(
            sxyz, CNT, new_xyz, centers, NEW_CNT, F(V.MULTIPLIER * dist), nsample, ntype)
        (g36[f"op{k}_new_features"], g36[f"op{k}_new_local_xyz"], g36[f"op{k}_point_cnt_of_grid"],
         g36[f"op{k}_src_row"]) = V.voxel_query(sxyz, CNT, feats, new_xyz, NEW_CNT, num_grid, dist, nsample, ntype)
    G.save("g36_vector_pool_ops", **g36)
    g37 = {}
    for seed, (kind, (c_in, cfg)) in enumerate(V.module_cfgs().items()):
        state = draw_state(Rm, c_in, cfg, 370 + 10 * seed)
        mfeats = r.normal(0, 1, (sum(CNT), c_in)).astype(F)
        probe = r.normal(0, 1, (sum(NEW_CNT), cfg["MSG_POST_MLPS"][-1])).astype(F)
        g37[f"{kind}_cfg_json"] = np.frombuffer(json.dumps(cfg).encode(), np.uint8)
        g37[f"{kind}_state_keys_json"] = np.frombuffer(json.dumps({k: list(v.shape) for k, v in state.items()}).encode(), np.uint8)
        g37[f"{kind}_features"], g37[f"{kind}_probe"] = mfeats, probe
        g37.update({f"{kind}_state.{k}": v for k, v in state.items()})
        for dt in (torch.float32, torch.float64):
            with (G.keep_double() if dt == torch.float64 else contextlib.nullcontext()):
                run_module(Rm, kind, c_in, cfg, state, (sxyz, new_xyz), mfeats, probe, dt, g37)
        print(kind, "train f32 - f64", np.abs(g37[f"{kind}_train_f32"] - g37[f"{kind}_train_f64"]).max())
    G.save("g37_vector_pool_modules", **g37)
    with open(os.path.join(HERE, "MANIFEST_vector_pool.json"), "w") as f:
        json.dump(G.manifest, f, indent=1, sort_keys=True)
