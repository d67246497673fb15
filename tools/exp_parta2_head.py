"""Time of PartA2FCHead's pooling on one MI355X: `parta2_pool` (com_amd/csrc/parta2.hip: the whole stacked batch straight to
sparse rows) against (a) the reference's formulation over this project's existing ops (partA2_head.py:104-151, :184-195: per
frame RoIAwarePool3d 'avg' over the part features and 'max' over the RPN features, cat, sum(-1).nonzero(), gather), on the
same inputs, forward and forward + backward; the fused path eager (one read-back of the row count), with a static row
capacity (no read-back) and replayed from a captured graph.  Separately: the first shared FC as the head runs it, dense()
+ Conv1d(NUM_FEATURES * POOL_SIZE^3 -> 256) over the pooled rows, forward and forward + backward (the sparse form that was
measured against it and lost is described in DESIGN.md section 4.14).

Size of tools/cfgs/kitti_models/PartA2.yaml in training: B = 2 frames x 128 RoIs, 16 384 points per frame, 128 channels,
POOL_SIZE 12, MAX_POINTS_PER_VOXEL 128, NUM_FEATURES 128.  The scene is synthetic: car-sized RoIs over a 70 m x 80 m area, 60 %
of the points drawn inside RoIs; its number of rows and of listed points is printed.

Every figure comes from device events around a window of ITERS calls, ITERS chosen so that a window lasts at least
WINDOW_S; WARM warm-up calls per variant; the variants alternate inside each of ROUNDS rounds; median / minimum / maximum over
the rounds.  One JSON line at the end.  Needs the GPU (no fallback).  Started without --run, the tool runs its one GPU step
as a child process under `timeout`."""
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, ROUNDS, WINDOW_S = 3, 7, 0.3
LIMIT_S = 420
B, N, P, C, POOL, MPV, NUM_FEATURES, FC_OUT, THRESH = 2, 128, 16384, 128, 12, 128, 128, 256, 0.3


def window_ms(fn, iters):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def compare(variants):
    """{name: fn} -> {name: (median, min, max) us per call, iters}"""
    iters = {}
    for k, fn in variants.items():
        for _ in range(WARM):
            fn()
        per_call = window_ms(fn, 3) / 3
        iters[k] = max(3, math.ceil(WINDOW_S * 1e3 / max(per_call, 1e-3)))
    samples = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            samples[k].append(window_ms(fn, iters[k]) / iters[k] * 1e3)
    return {k: (statistics.median(v), min(v), max(v), iters[k]) for k, v in samples.items()}


def scene(dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *s: torch.rand(*s, device=dev, generator=g)          # noqa: E731
    rois = torch.zeros(B, N, 7, device=dev)
    rois[..., 0] = rand(B, N) * 70.0
    rois[..., 1] = rand(B, N) * 80.0 - 40.0
    rois[..., 2] = rand(B, N) * 1.0 - 1.5
    rois[..., 3:6] = torch.tensor([3.9, 1.6, 1.56], device=dev) * (0.8 + 0.4 * rand(B, N, 1))
    rois[..., 6] = (rand(B, N) - 0.5) * 4 * math.pi
    coords = []
    for b in range(B):
        n_in = int(0.6 * P)
        pick = torch.randint(0, N, (n_in,), device=dev, generator=g)
        r = rois[b, pick]
        loc = (rand(n_in, 3) - 0.5) * r[:, 3:6]
        c, s = torch.cos(r[:, 6]), torch.sin(r[:, 6])
        inside = torch.stack([r[:, 0] + loc[:, 0] * c - loc[:, 1] * s, r[:, 1] + loc[:, 0] * s + loc[:, 1] * c, r[:, 2] + loc[:, 2]], 1)
        free = torch.stack([rand(P - n_in) * 70.0, rand(P - n_in) * 80.0 - 40.0, rand(P - n_in) * 3.0 - 2.5], 1)
        xyz = torch.cat([inside, free])[torch.randperm(P, device=dev, generator=g)]
        coords.append(torch.cat([torch.full((P, 1), float(b), device=dev), xyz], 1))
    return dict(rois=rois, point_coords=torch.cat(coords).contiguous(), point_features=torch.randn(B * P, C, device=dev, generator=g),
                point_part_offset=rand(B * P, 3), point_cls_scores=rand(B * P))


def main():
    import torch
    import torch.nn as nn
    from com_amd import roiaware_pool3d
    from com_amd.hotpath import parta2_pool
    from com_amd.spconv import functional as Fsp
    assert torch.cuda.is_available(), "tools/exp_parta2_head.py measures on the GPU"
    dev = "cuda"
    s = scene(dev)
    feats, part = s['point_features'].requires_grad_(True), s['point_part_offset'].requires_grad_(True)
    layer = roiaware_pool3d.RoIAwarePool3d(POOL, MPV)
    result = {"device": torch.cuda.get_device_name(0), "shape": [B, N, P, C, POOL, MPV], "warm": WARM, "rounds": ROUNDS,
              "window_s": WINDOW_S}

    def composed():
        pf = torch.cat((part, s['point_cls_scores'].view(-1, 1)), dim=1)
        pf[pf[:, -1] < THRESH, 0:3] = 0
        batch_idx, xyz = s['point_coords'][:, 0], s['point_coords'][:, 1:4]
        pp, pr = [], []
        for b in range(B):
            m = batch_idx == b
            roi = s['rois'][b].contiguous()
            pp.append(layer.forward(roi, xyz[m], pf[m], pool_method='avg'))
            pr.append(layer.forward(roi, xyz[m], feats[m], pool_method='max'))
        pp, pr = torch.cat(pp), torch.cat(pr)
        idx = pp.sum(dim=-1).nonzero()
        return idx.int(), pp[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]], pr[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]

    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def fused(**kw):
        return parta2_pool(s['rois'], s['point_coords'], feats, part, s['point_cls_scores'], THRESH, POOL, MPV, **kw)[:3]

    with torch.no_grad():
        want, got = composed(), fused()
        state = parta2_pool(s['rois'], s['point_coords'], feats, part, s['point_cls_scores'], THRESH, POOL, MPV)[3].tolist()
    rows, listed = state[1], state[2]
    assert torch.equal(want[0], got[0]) and torch.equal(want[2], got[2]) and float((want[1] - got[1]).abs().max()) <= 1e-6
    result.update(rows=rows, listed_points=listed, cells=B * N * POOL ** 3)
    print(f"{rows} rows of {B * N * POOL ** 3} cells ({100.0 * rows / (B * N * POOL ** 3):.1f} %), {listed} listed points; "
          "the fused rows equal the composition's")
    cap = dict(max_rows=int(rows * 1.25) // 64 * 64 + 64, max_listed=int(listed * 1.25) + 64, status=status)
    g_part, g_rpn = torch.randn(rows, 4, device=dev), torch.randn(rows, C, device=dev)
    gs_part, gs_rpn = torch.randn(cap['max_rows'], 4, device=dev), torch.randn(cap['max_rows'], C, device=dev)

    def fwd_bwd(fn, gp, gr):
        def run():
            feats.grad = part.grad = None
            _, pr, rr = fn()
            ((pr * gp).sum() + (rr * gr).sum()).backward()
        return run

    def no_grad(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    graphs = {}
    for name, fn in (("fwd", no_grad(lambda: fused(**cap))), ("fwd_bwd", fwd_bwd(lambda: fused(**cap), gs_part, gs_rpn))):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            fn()
    t = compare({"a_composed_fwd": no_grad(composed), "a_composed_fwd_bwd": fwd_bwd(composed, g_part, g_rpn),
                 "b_fused_eager_fwd": no_grad(fused), "b_fused_eager_fwd_bwd": fwd_bwd(fused, g_part, g_rpn),
                 "b_fused_static_fwd": no_grad(lambda: fused(**cap)),
                 "b_fused_static_fwd_bwd": fwd_bwd(lambda: fused(**cap), gs_part, gs_rpn),
                 "b_fused_replay_fwd": graphs["fwd"].replay, "b_fused_replay_fwd_bwd": graphs["fwd_bwd"].replay})
    assert int(status) == 0
    # the first shared FC as the head runs it: dense() + Conv1d over the pooled rows (x_rpn | x_part, NUM_FEATURES wide)
    coords = got[0]
    merged = torch.randn(rows, NUM_FEATURES, device=dev, requires_grad=True)
    fc = nn.Conv1d(NUM_FEATURES * POOL ** 3, FC_OUT, kernel_size=1, bias=False).to(dev)
    g_fc = torch.randn(B * N, FC_OUT, 1, device=dev)

    def dense_fc():
        return fc(Fsp.bev_dense(merged, coords, B * N, [POOL] * 3, None).view(B * N, -1, 1))

    def dense_fc_fwd_bwd():
        merged.grad = fc.weight.grad = None
        (dense_fc() * g_fc).sum().backward()

    t.update(compare({"fc_dense_fwd": no_grad(dense_fc), "fc_dense_fwd_bwd": dense_fc_fwd_bwd}))
    for k, (med, lo, hi, iters) in t.items():
        result[f"{k}_us"] = [round(med, 1), round(lo, 1), round(hi, 1)]
        print(f"{k:26s}: median {med:10.1f} us  (min {lo:.1f}, max {hi:.1f}; windows of {iters} calls)")
    print(json.dumps(result))


if __name__ == "__main__":
    if "--run" in sys.argv:
        main()
    else:
        sys.exit(subprocess.call(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--run"]))
