"""Frames/s of a STOCK detector object (tools/stock_detector.py, shaped like the reference's build_networks output) at three
levels of integration, on one GPU, beside bench.py's own assembly of the same workload:

  stock_eager       the stock detector as built: torch.optim.Adam + clip_grad_norm_, eager launches, the reference's loop
  adopted_eager     com_amd.adopt.adopt_model + com_amd.train.prepare_training, CapturedStep without capture()
  adopted_captured  the same after capture()
  bench_captured    bench.build_workload's step (bench.py's own assembly), captured, timed the same way in this process
  bench_py          a child run `bench.py --light [--dense-head --com]`: the `value` bench.py reports on this box

    python tools/exp_adopt.py [--model 3d|com|both] [--steps 100] [--batch 4] [--out profiles/adopt_fps.json]

The 3-D model trains with bench.py's stand-in loss (its model_func); the COM model through the detector's own forward and
get_training_loss with bench.py's fixed ground truth handed in per batch (CapturedStep batch_keys)."""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402
import stock_detector as SD  # noqa: E402
from com_amd import hotpath, train  # noqa: E402
from com_amd.adopt import adopt_model  # noqa: E402
from com_amd.spconv import functional as Fsp  # noqa: E402

OPTIMIZATION = dict(OPTIMIZER="adam_onecycle", LR=0.003, WEIGHT_DECAY=0.01, MOMS=[0.95, 0.85], PCT_START=0.4,
                    DIV_FACTOR=10, GRAD_NORM_CLIP=10)


def _args(a, com):
    return argparse.Namespace(batch=a.batch, distinct_batches=a.distinct_batches, same_shard=True, dense_head=com, com=com,
                              com_ucl=False, config5=False)


def _time_step(step, batches, steps, B, capture):
    step.observe(batches, steps=3)
    if capture:
        step.capture(batches[0], validate=batches[:3])
    step.prime(batches[0])
    for i in range(3):
        step(batches[(i + 1) % len(batches)])
    torch.cuda.synchronize()
    gc.collect()
    t0 = time.perf_counter()
    train.train_one_epoch(step, batches, steps, accumulated_iter=step.lr_scheduler.last_iter + 1, gc_collect=False)
    torch.cuda.synchronize()
    step.check()
    return round(B * steps / (time.perf_counter() - t0), 1)


def _stock_eager(kind, state, W, batches, steps, model_func, epoch):
    dev = W.flat_param.device
    m = SD.build_detector(kind).to(dev).train()
    m.load_state_dict(state, strict=False)
    if epoch is not None:
        m.dense_head.epoch = epoch
    optim = torch.optim.Adam(m.parameters(), lr=3e-4, betas=(0.9, 0.99))
    c = W.step.vox_cfg

    def one(batch):
        bd = hotpath.transform_points_to_voxels({"points": batch["points"], "frame_offsets": batch["frame_offsets"],
                                                 "batch_size": W.B}, c.point_cloud_range, c.voxel_size,
                                                c.max_points_per_voxel, c.max_voxels, fuse_mean=True)
        bd = {"voxel_features": bd["voxel_features"], "voxel_coords": bd["voxel_coords"], "batch_size": W.B,
              **{k: v for k, v in batch.items() if k not in ("points", "frame_offsets")}}
        optim.zero_grad()
        out = model_func(m, bd)
        (out[0] if isinstance(out, tuple) else out).backward()
        Fsp.join_deferred_wgrad()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 10.0)
        optim.step()
    for i in range(3):
        one(batches[i % len(batches)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        one(batches[i % len(batches)])
    torch.cuda.synchronize()
    return round(W.B * steps / (time.perf_counter() - t0), 1)


def _bench_py(a, com):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--light", "--gpus", "1", "--steps", str(a.steps), "--warmup", "20",
           "--batch", str(a.batch), "--distinct-batches", str(a.distinct_batches)] + (["--dense-head", "--com"] if com else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"error": f"rc {r.returncode}: {r.stderr[-400:]}"}
    return json.loads(lines[-1])["value"]


def measure(a, com):
    kind = "com" if com else "3d"
    W = bench.build_workload(_args(a, com), 0, 1, torch.device("cuda", 0))
    state = {k: v.detach().clone() for k, v in W.model.state_dict().items()}
    out = {"model": "full CenterPoint + COM head (CurriculumCenterHead_x5)" if com else "3-D (vfe + VoxelResBackBone8x + "
           "HeightCompression, bench.py's stand-in loss)", "batch": W.B, "steps": a.steps}
    epoch, model_func = None, W.step.model_func
    if com:
        cl = dict(zip(model_func.__code__.co_freevars, (c.cell_contents for c in model_func.__closure__)))   # (all set with --com)
        gt = dict(gt_boxes=cl["gt_boxes"], num_points_in_gt=cl["com_npgt"], true_object=cl["com_true"],
                  occupancy_ratio=cl["com_occ"], facade_type=cl["com_facade"])
        epoch, model_func = cl["com_epoch"], train.model_fn_decorator()
    else:
        gt = {}
    batches = [dict(points=p, frame_offsets=o, **gt) for p, o in W.batches]
    out["bench_captured"] = _time_step(W.step, W.batches, a.steps, W.B, True)
    W.step.release()
    if com:
        stock_func = model_func
    else:                                                    # the stand-in loss over the stock fp32 NCHW BEV map
        lw = model_func.__closure__[model_func.__code__.co_freevars.index("loss_w")].cell_contents.float()
        stock_func = lambda m, bd: (m.map_to_bev_module(m.backbone_3d(m.vfe(bd)))["spatial_features"].float()
                                    .reshape(-1) * lw).sum()
    try:
        out["stock_eager"] = _stock_eager(kind, state, W, batches, max(10, a.steps // 5), stock_func, epoch)
    except Exception as exc:                                 # (the figure beside it is what matters)
        out["stock_eager_error"] = f"{type(exc).__name__}: {exc}"[:400]
    for name, capture in (("adopted_eager", False), ("adopted_captured", True)):
        m = SD.build_detector(kind).to(W.flat_param.device)
        m.load_state_dict(state, strict=False)
        adopt_model(m)
        if epoch is not None:
            m.dense_head.epoch = epoch
        _, _, step = train.prepare_training(m, OPTIMIZATION, 30 * 1000, W.step.vox_cfg, W.B, max_gt=96,
                                            model_func=None if com else W.step.model_func)
        out[name] = _time_step(step, batches, a.steps if capture else max(10, a.steps // 5), W.B, capture)
        step.release()
        del m, step
    out["adopted_captured_over_bench_captured"] = round(out["adopted_captured"] / out["bench_captured"], 4)
    del W
    gc.collect()
    torch.cuda.empty_cache()
    if not a.no_bench_py:
        out["bench_py"] = _bench_py(a, com)
        if isinstance(out["bench_py"], float):
            out["adopted_captured_over_bench_py"] = round(out["adopted_captured"] / out["bench_py"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("3d", "com", "both"), default="both")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--distinct-batches", type=int, default=16)
    ap.add_argument("--no-bench-py", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"unit": "frames/s", "device": torch.cuda.get_device_name(0)}
    for com in ((False, True) if a.model == "both" else ((a.model == "com"),)):
        res["com" if com else "3d"] = measure(a, com)
        print(json.dumps(res["com" if com else "3d"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
