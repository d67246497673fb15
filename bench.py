#!/usr/bin/env python3
"""bench.py -- training frames/sec of the sparse-voxel hot path on N MI355X (one process per GPU).

One "step" = one pass of the hot path over one batch of B synthetic Waymo-shaped frames per GPU
(SURVEY.md section 8d): hard voxelisation (+ fused MeanVFE) of the HBM-resident point buffer ->
VoxelResBackBone8x forward (9 rulebook builds, 21 sparse convs, BN/ReLU/residual) -> HeightCompression
BEV scatter -> loss -> backward (dgrad + wgrad of every conv, BEV gather) -> DDP gradient all-reduce
(N > 1, RCCL over xGMI) -> grad-norm clip (centerpoint.yaml:96) -> Adam step.

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run does only what that line's
headline needs: set-up, warm-up, the timed steps, `--dump-outputs` / `--dump-state`, the line.  `--full`
measures the rest as well and adds it to the line: `h2d_inclusive` and `ragged` (two more timed loops),
`roofline` (dominant kernel, timed live with HIP events on the launch stream) and, at N = 1, its rulebook
regime, `seam_path`, `cpu_baseline` (the CPU oracle port: every conv fwd+bwd, rulebook and BatchNorm of
the batch, median of 3 passes), `stage2`, and the child runs `full_model` (the complete CenterPoint step
with the COM curriculum head, `bench.py --dense-head --com`), `config5_300k` and `n_gt_1_form`.
"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402   (importing torch does not touch the GPU; nothing below does before main() decides to spawn)
import torch.distributed as dist  # noqa: E402

from com_amd import hotpath, ops  # noqa: E402   (the HIP library is loaded lazily, on the first op)
from com_amd import dist as cdist  # noqa: E402
from com_amd import train  # noqa: E402
from com_amd.utils import synth  # noqa: E402

METRIC = "training frames/sec, CenterPoint-VoxelNet Waymo 160k-pt clouds, 1/2/4/8 MI355X"

HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_BF16_PEAK_TF = 2500.0     # dense bf16 MFMA peak


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4, help="frames per GPU (centerpoint.yaml:78)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run every secondary measurement (each --no-* switch leaves one out); "
                         "without it only the headline is measured")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--stage-times", action="store_true", help="print per-stage GPU times to stderr")
    ap.add_argument("--mode", choices=["graph", "eager"], default="graph",
                    help="graph: replay the captured step (default); eager: one launch per kernel from Python")
    ap.add_argument("--no-h2d", action="store_true", help="skip the secondary (PCIe-inclusive) timed loop")
    ap.add_argument("--dump-state", default=None, metavar="PATH",
                    help="after the timed loop write sha256 of the flat parameters / gradients (rank 0) to PATH")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed loop write what its last step computed (parameters, Adam moments, grad norm, "
                         "BatchNorm statistics; rank 0) as DIR/<name>.npy, float32 / float64, at most 64 MB in all")
    ap.add_argument("--same-shard", action="store_true",
                    help="validation: every rank processes rank 0's frames (the rank mean then equals one rank's gradient)")
    ap.add_argument("--dense-head", action="store_true",
                    help="the complete CenterPoint step: BaseBEVBackbone + CenterHead towers (bf16, channels-last; "
                         "hand-written 3x3 convs) + device-side targets and losses behind the hot path instead of the "
                         "linear-functional stand-in")
    ap.add_argument("--com", action="store_true",
                    help="with --dense-head (implied): the COM curriculum head of BASELINE config 3 -- cluster(), "
                         "curriculum targets with radius_map / groups, FocalLossCenterCurriculum with the (3, 96) "
                         "group-confidence sums, epoch all_gather after the timed loop")
    ap.add_argument("--com-ucl", action="store_true", help="with --com: LOSS_CURRICULUM.UCL = True (per-object weights)")
    ap.add_argument("--distinct-batches", type=int, default=16, help="distinct global batches the timed loop cycles through")
    ap.add_argument("--no-ragged", action="store_true", help="skip the secondary loop over frames with 0-20 %% ray drop-out")
    ap.add_argument("--config5", action="store_true",
                    help="BASELINE config 5 as a TRAINING step: SECOND's plain VoxelBackBone8x on 300k-point clouds "
                         "(120 beams x 2500 az) with the fp8 (e4m3) forward convs of com_amd.spconv.fp8, bf16 backward")
    ap.add_argument("--no-fp8", action="store_true", help="skip the child run that measures --config5")
    ap.add_argument("--no-regime", action="store_true", help="skip the rulebook bandwidth-regime child run (B = 4 and B = 32)")
    ap.add_argument("--no-stage2", action="store_true", help="skip the PV-RCNN stage-2 (config 4) secondary figure")
    ap.add_argument("--no-full-model", action="store_true", help="skip the child run that measures the full CenterPoint + COM step")
    ap.add_argument("--no-n-gt-1", action="store_true", help="skip the two child runs that measure the N > 1 execution form on one GPU")
    ap.add_argument("--no-seam-path", action="store_true", help="skip the stock-eager / fused-eager / captured comparison")
    ap.add_argument("--light", action="store_true",
                    help="only the timed loop, even with --full: every --no-* switch at once (experiment scripts)")
    ap.add_argument("--launch-timeout", type=float, default=900.0,
                    help="N > 1 without a launcher: seconds after which this process stops the ranks it started and fails")
    ap.add_argument("--rank-timeout", type=float, default=840.0,
                    help="N > 1: seconds after which a rank ends ITSELF with code 124 (a hung collective cannot unwind)")
    ap.add_argument("--init-timeout", type=float, default=180.0,
                    help="N > 1: deadline for rendezvous + communicator set-up + the first all-reduce, per rank")
    ap.add_argument("--selftest-hang", type=int, default=-1, metavar="RANK",
                    help="with --selftest-launch: this rank never joins the first all-reduce (watchdog test)")
    ap.add_argument("--selftest-launch", action="store_true",
                    help="CPU plumbing test of the launcher / result assembly: gloo ranks, no GPU work")
    a = ap.parse_args()
    if a.light or not a.full:
        a.no_cpu_baseline = a.no_roofline = a.no_h2d = a.no_ragged = a.no_stage2 = a.no_full_model = a.no_fp8 = True
        a.no_regime = a.no_n_gt_1 = a.no_seam_path = True
    return a


class HotPath(torch.nn.Module):
    """vfe -> backbone_3d -> map_to_bev of CenterPoint-VoxelNet (tools/cfgs/waymo_models/centerpoint.yaml:9-17);
    dense_head=True appends backbone_2d + the conv towers of dense_head (centerpoint.yaml:19-46) in bf16 /
    channels_last."""

    def __init__(self, dense_head=False, plain=False):
        super().__init__()
        grid = ops.grid_size(synth.WAYMO_RANGE, synth.WAYMO_VOXEL)
        self.vfe = hotpath.MeanVFE({}, 5)
        # plain=True: SECOND's backbone (tools/cfgs/waymo_models/second.yaml:13-14 -> VoxelBackBone8x), config 5
        self.backbone_3d = (hotpath.VoxelBackBone8x if plain else hotpath.VoxelResBackBone8x)({}, 5, grid)
        # spatial_features [B, C*D, H, W] is handed over in torch.channels_last memory format (MAP_TO_BEV.CHANNELS_LAST: same
        # shape, same values; a voxel's 128 channels are one 512-byte run instead of 128 two-byte elements 141 KB apart) -- the
        # layout the dense stack reads; PCD_BEV_NHWC=0: NCHW-contiguous, the reference's .dense().view() (scatter 32 -> 12 us,
        # gather 23 -> 5 us on the single-stream stretch between forward and backward: 3.09 -> 3.06 ms)
        self.map_to_bev_module = hotpath.HeightCompression({"NUM_BEV_FEATURES": 256,
                                                            "CHANNELS_LAST": dense_head or os.environ.get("PCD_BEV_NHWC", "1") != "0"})
        if dense_head:
            from com_amd.hotpath import dense2d
            self.backbone_2d = dense2d.BaseBEVBackbone(dense2d.CENTERPOINT_BACKBONE_2D, 256)
            self.dense_head = dense2d.CenterHeadTowers(dense2d.CENTERPOINT_HEAD, self.backbone_2d.num_bev_features,
                                                       [['Vehicle', 'Pedestrian', 'Cyclist']])

    def forward(self, voxel_features, voxel_coords, batch_size):
        bd = {"voxel_features": voxel_features, "voxel_coords": voxel_coords, "batch_size": batch_size}
        bd = self.map_to_bev_module(self.backbone_3d(self.vfe(bd)))
        return bd["spatial_features"], bd


DUMP_BUDGET_BYTES = 64 * 2 ** 20


def dump_outputs(path, W):
    """`--dump-outputs`: what the timed step hands its caller -- the updated flat parameters, the Adam moments, the
    gradient norm of the step and the BatchNorm running statistics -- as <path>/<name>.npy (float32; float64 stays
    float64).  Above DUMP_BUDGET_BYTES in all, the large arrays are cut to a fixed seeded sample of their elements (the
    same positions in every run with the same arguments)."""
    def host(t):
        t = t.detach()
        return t.cpu().numpy() if t.dtype == torch.float64 else t.float().cpu().numpy()

    torch.cuda.synchronize()
    arrays = {"parameters": host(W.flat_param), "adam_exp_avg": host(W.opt.exp_avg),
              "adam_exp_avg_sq": host(W.opt.exp_avg_sq), "grad_norm": host(W.opt.grad_norm)}
    stats = [host(b).ravel() for b in W.model.buffers() if b.is_floating_point()]
    if stats:
        arrays["batchnorm_stats"] = np.concatenate(stats)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_BUDGET_BYTES:
        rng = np.random.default_rng(0)
        keep = DUMP_BUDGET_BYTES / total * 0.99
        for k, a in arrays.items():
            if a.size > 4096:
                idx = np.sort(rng.choice(a.size, int(a.size * keep), replace=False))
                arrays[k] = a.ravel()[idx]
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), a)


TRAFFIC_FILE = os.path.join("profiles", "r06_pmc_traffic.json")


def _pmc_traffic(kernel):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 --pmc passes of this same command
    (FETCH_SIZE doubled per MI355X_MICROARCH.md, + WRITE_SIZE) -- PMC counters cannot be read from inside the timed
    process.  Returns (bytes or None, source description incl. the git blob hash of the file that was read)."""
    import hashlib
    for rel in (TRAFFIC_FILE, os.path.join("profiles", "r04_pmc_traffic.json")):
        path = os.path.join(ROOT, rel)
        try:
            data = open(path, "rb").read()
            k = json.loads(data)["kernels"]
        except Exception:
            continue
        blob = hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()[:12]
        # (the summary keeps the template arguments only where several instantiations of a kernel run in the step)
        hit = [v for name, v in k.items() if name == kernel or name.startswith(kernel + "<") or name.startswith(kernel + " ")
               or kernel.startswith(name + "<")]
        val = hit[0]["hbm_bytes_per_launch_corrected"] if hit else None
        return val, f"{rel}@{blob} (offline rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE; not measured in this run)"
    return None, None


def _rocprof_avg_us(kernel):
    """Average launch duration of `kernel` in the newest committed `rocprofv3 --kernel-trace --stats` summary of this
    same command (profiles/*_kernel_stats_eager.txt), reported BESIDE the live HIP-event figure: (us, file) or (None, None)."""
    import glob
    import re
    m = re.match(r"(\w+)<NB=(\d+)>", kernel)
    mw = re.match(r"(subm_win_kernel|subm_wgrad_win_kernel)<(\d+)>", kernel)
    if mw:
        pat = re.compile(mw.group(1) + r"<.*WinCfg<" + mw.group(2) + r",")
    else:
        pat = re.compile(re.escape(m.group(1)) + r"<" + m.group(2) + r",") if m else re.compile(re.escape(kernel.split(" ")[0]) + r"[<(]")
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_kernel_stats_eager.txt")),
                   key=lambda f: [int(x) for x in re.findall(r"\d+", os.path.basename(f))])
    for path in reversed(files):
        try:
            for line in open(path):
                parts = line.split(None, 4)
                if len(parts) == 5 and parts[0].isdigit() and pat.search(parts[4]):
                    return float(parts[2]), os.path.relpath(path, ROOT)
        except Exception:
            continue
    return None, None


def _event_overhead_ms():
    """What a HIP-event bracket measures around NOTHING (record, record on the launch stream): subtracted from every
    bracketed launch, so that the per-launch figures are kernel durations (what rocprofv3 --kernel-trace reports for
    the same launches) and not duration + the cost of the second event."""
    vals = []
    for _ in range(32):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        e1.record()
        vals.append((e0, e1))
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in vals)
    return t[len(t) // 2]


EVENT_OVERHEAD_MS = [None]


def _profiled_groups(step_fn):
    """One extra step with HIP events around every instrumented launch -> per-kernel-group totals."""
    ops.PROFILE = []
    try:
        step_fn()
        torch.cuda.synchronize()
        recs = ops.PROFILE
    finally:
        ops.PROFILE = None
    if EVENT_OVERHEAD_MS[0] is None:
        EVENT_OVERHEAD_MS[0] = _event_overhead_ms()
    groups = {}
    for key, e0, e1, meta in recs:
        name = key.split(" ")[0] + (" " + key.split(" ")[1] if key.startswith("wgrad") else "")
        g = groups.setdefault(name, dict(ms=0.0, bytes=0, flops=0, launches=0))
        g["ms"] += max(e0.elapsed_time(e1) - EVENT_OVERHEAD_MS[0], 0.0)
        g["bytes"] += meta["bytes"]
        g["flops"] += meta["flops"]
        g["launches"] += 1
    return groups


RIDGE = MFMA_BF16_PEAK_TF * 1e12 / (HBM_PEAK_GBS * 1e9)      # 312 flop/B


def _group_roofline(name, g):
    secs = max(g["ms"], 1e-9) * 1e-3           # (every launch of a group can clamp to 0 after the event-overhead subtraction)
    ai = g["flops"] / max(g["bytes"], 1)
    tf = g["flops"] / secs / 1e12
    gbs = g["bytes"] / secs / 1e9
    mfma_bound = ai > RIDGE
    return {"kernel": name, "bound": "mfma" if mfma_bound else "hbm",
            "achieved": round(tf if mfma_bound else gbs, 2),
            "peak": MFMA_BF16_PEAK_TF if mfma_bound else HBM_PEAK_GBS,
            "unit": "TFLOP/s" if mfma_bound else "GB/s",
            "frac": round((tf / MFMA_BF16_PEAK_TF) if mfma_bound else (gbs / HBM_PEAK_GBS), 4),
            "launches_per_step": g["launches"], "avg_launch_us": round(1e3 * g["ms"] / g["launches"], 2),
            "ms_per_step": round(g["ms"], 3),
            "algorithmic_bytes_per_launch": int(g["bytes"] / g["launches"]),
            "algorithmic_flops_per_launch": int(g["flops"] / g["launches"]),
            "arithmetic_intensity_flop_per_byte": round(ai, 1),
            "other_frac": {"hbm": round(gbs / HBM_PEAK_GBS, 4), "mfma": round(tf / MFMA_BF16_PEAK_TF, 4)}}


def measure_roofline(step_fn, ms_per_step):
    """Roofline, measured LIVE: one extra training step runs with HIP events (on the launch stream) around every
    instrumented launch (com_amd.ops.PROFILE); launches are grouped by kernel instantiation (the name rocprofv3
    reports).  Algorithmic bytes / flops per launch are SURVEY.md 8d's: conv (N_in*Cin + N_out*Cout)*2 + 8*P +
    K*Cin*Cout*e bytes and 2*P*Cin*Cout flops, rulebook 16*N_in + 8*P (+16*N_out), voxelise 24*N + 36*M,
    BatchNorm 2..3*N*C*e per pass, BEV N5*(C*e+16) + B*C*D*H*W*e.  The headline object is the group with the
    largest total time; `kernels` lists every group above 2 % of the instrumented time the same way; `step` is
    SURVEY 8d's graded figure: the sum of ALL algorithmic bytes / flops of one step over the measured (graph-mode)
    step time."""
    groups = _profiled_groups(step_fn)
    if not groups:
        return None
    conv_like = {k: v for k, v in groups.items() if k.startswith(("gather_gemm", "ggw", "wgrad", "subm_win", "subm_wgrad"))}
    name, g = max(conv_like.items() or groups.items(), key=lambda kv: kv[1]["ms"])
    out = _group_roofline(name, g)
    traffic, source = _pmc_traffic(name)
    out["traffic"] = traffic
    out["traffic_source"] = source
    out["event_overhead_us"] = round(1e3 * EVENT_OVERHEAD_MS[0], 2)      # (already subtracted per launch)
    rp, rp_src = _rocprof_avg_us(name)
    if rp is not None:           # the profiler's figure for the same kernel (another box, another run): both are reported,
        # named, at the top level: `frac` = HIP events of THIS run (they bracket a launch on the stream and read ~10 % longer
        # than the profiler's kernel duration), `frac_rocprof` = the same algorithmic work over the committed profile's average
        out["rocprof"] = {"avg_launch_us": rp, "frac": round(out["frac"] * out["avg_launch_us"] / rp, 4), "source": rp_src}
        out["frac_rocprof"] = out["rocprof"]["frac"]
        out["frac_source"] = "HIP events in this run (avg_launch_us); frac_rocprof: " + rp_src
    total_ms = sum(v["ms"] for v in groups.values())
    out["kernels"] = [_group_roofline(k, v) for k, v in sorted(groups.items(), key=lambda kv: -kv[1]["ms"])
                      if v["ms"] >= 0.02 * total_ms]
    for kr in out["kernels"]:
        for drop in ("peak", "unit", "algorithmic_bytes_per_launch", "algorithmic_flops_per_launch", "other_frac"):
            kr.pop(drop, None)
    # which regime these per-launch figures are: NOT the profile's (profiles/*_kernel_stats_graph.txt = kernel durations inside
    # the replayed graph) and not isolated launches
    out["kernels_regime"] = ("HIP-event brackets around every launch of ONE eager step, the weight-gradient stream overlapping the "
                             "data gradients (event overhead subtracted); rocprofv3's in-graph kernel durations are in "
                             "profiles/, isolated launches in `isolated` / tools/exp_subm_win.py")
    tb, tfl = sum(v["bytes"] for v in groups.values()), sum(v["flops"] for v in groups.values())
    secs = ms_per_step * 1e-3
    out["step"] = {"alg_bytes": int(tb), "alg_flops": int(tfl), "ms_per_step": round(ms_per_step, 4),
                   "hbm_frac": round(tb / secs / 1e9 / HBM_PEAK_GBS, 4),
                   "mfma_frac": round(tfl / secs / 1e12 / MFMA_BF16_PEAK_TF, 4),
                   "rulebook_alg_bytes": int(sum(v["bytes"] for k, v in groups.items() if k.startswith("rulebook"))),
                   "rulebook_ms_eager": round(sum(v["ms"] for k, v in groups.items() if k.startswith("rulebook")), 3)}
    # the same kernel WITHOUT a concurrent weight-gradient kernel on the second stream (in the step the data
    # gradient and the weight gradient of a layer overlap and stretch each other; this is the kernel by itself)
    from com_amd.spconv import functional as Fsp
    keep = Fsp.OVERLAP_WGRAD
    Fsp.OVERLAP_WGRAD = False
    try:
        alone = _profiled_groups(step_fn).get(name)
    finally:
        Fsp.OVERLAP_WGRAD = keep
    if alone and alone["ms"] > 0:
        iso = _group_roofline(name, alone)
        out["isolated"] = {"avg_launch_us": iso["avg_launch_us"], "achieved": iso["achieved"], "frac": iso["frac"]}
    return out


def measure_cpu_baseline():
    """CPU baseline ("port"): the C oracle (oracle/pcd_oracle.c, spconv's native gather-GEMM-scatter algorithm,
    fp32, compiled -O3 -march=native) on the host's cores, timed on the B = 4 batch of whole synthetic frames the GPU figure
    is quoted on, unsampled, frame by frame: voxelise, MeanVFE, all 9 rulebooks, all 21 convs of VoxelResBackBone8x
    (spconv_backbone.py:191-232) forward + backward, 21 BatchNorm+ReLU fwd+bwd (torch-CPU), BEV dense + its gradient.
    value = 4 / median of 3 batch passes behind one warm-up pass (`protocol` says how that differs from BASELINE.md's).
    The conv arithmetic and BN run on `cores` threads (OpenMP over the pairs of a kernel offset / torch intra-op).  The
    rulebook builders' per-offset loops can run on threads too (orc_set_rulebook_threads): they are timed once sequentially
    and once on min(cores, 27) threads and the faster setting is used and reported (`rulebook_threads`; hash probes bound by
    memory latency -- on the 8-core build container threads LOSE: 0.07 s vs 0.10-0.13 s for the level-1 SubM build).
    Voxelisation (first-appearance order: sequential by definition) and the BEV scatter run on one core.  One single-core
    pass is timed too (`single_core_value`).  `cores` = min(host cores, 64) is a cap, not a measured optimum: the baseline
    is a reported figure, never the target (`host_cores_available` says what the box had)."""
    from oracle import oracle as O          # cpu_baseline leg only
    mt = max(1, min(os.cpu_count() or 1, 64))
    RB_THREADS[0] = _pick_rulebook_threads(O, min(mt, 27))
    B = 4                                    # centerpoint.yaml:78 -- the batch of the GPU figure
    def batch_pass(threads):
        per = [_cpu_frame(O, threads, f) for f in range(B)]
        parts = {}
        for _, p in per:
            for k, v in p.items():
                parts[k] = parts.get(k, 0.0) + v
        return sum(t for t, _ in per), parts
    batch_pass(mt)                           # warm-up (page faults of the big buffers, OpenMP pool, torch's CPU kernels)
    passes = [batch_pass(mt) for _ in range(3)]
    passes.sort(key=lambda t: t[0])
    per_batch, parts = passes[1]
    st_total = _cpu_frame(O, 1, 0)[0] if mt > 1 else per_batch / B
    return {"value": round(B / per_batch, 4), "unit": "frames/s", "cores": mt, "kind": "port",
            "host_cores_available": os.cpu_count(), "single_core_value": round(1.0 / st_total, 4),
            "rulebook_threads": RB_THREADS[0],
            "passes_s": [round(t[0], 3) for t in passes],
            "protocol": f"B = {B} frames per pass (frames 0-{B - 1} of the GPU run's generator), fp32, 1 warm-up pass + median of 3 timed "
                        "passes -- BASELINE.md section 2 asks for 5 warm-ups + >= 20 iterations; bounded here to ~20 s of CPU work "
                        "as the bench contract requires (a pass is ~4 s on 64 cores); the single-core figure is ONE frame, one pass",
            "sample": f"{B} whole synthetic 160k-pt frames (unsampled), fp32 C oracle (spconv native gather-GEMM-scatter): "
                      "voxelize + MeanVFE + 9 rulebooks + all 21 VoxelResBackBone8x convs fwd+bwd + 21 BN/ReLU fwd+bwd "
                      f"(torch-CPU) + BEV dense fwd+bwd per frame; conv and BN on {mt} threads, rulebooks on "
                      f"{RB_THREADS[0]} (the faster of 1 / {min(mt, 27)}), the rest on 1; per pass: " + ", ".join(f"{k} {v:.2f}s" for k, v in parts.items())
                      + f"; all on one core: {st_total:.2f}s per frame"}


RB_THREADS = [1]


def _pick_rulebook_threads(O, cand):
    """1 or `cand`: whichever builds the level-1 SubM rulebook of a frame faster (median of 3)."""
    if cand <= 1:
        return 1
    pts = synth.synth_cloud(0)
    _, c, _ = O.voxelize_hard(pts, synth.WAYMO_RANGE, synth.WAYMO_VOXEL, synth.WAYMO_MAX_POINTS, synth.WAYMO_MAX_VOXELS)
    idx = np.concatenate([np.zeros((c.shape[0], 1), np.int32), c], 1)
    best = (None, 1)
    for th in (1, cand):
        O.set_rulebook_threads(th)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            O.rulebook_subm(idx, (41, 1504, 1504))
            ts.append(time.perf_counter() - t0)
        med = sorted(ts)[1]
        if best[0] is None or med < best[0]:
            best = (med, th)
    O.set_rulebook_threads(1)
    return best[1]


def _cpu_frame(O, threads, frame=0):
    torch.set_num_threads(threads)
    O.set_rulebook_threads(RB_THREADS[0] if threads > 1 else 1)
    rng = np.random.default_rng(0)
    t_total = {}
    if threads > 1:      # start the OpenMP thread pool outside the timed region
        tiny = {"K": 1, "n_in": 1, "n_out": 1, "pairs": np.zeros((1, 2, 1), np.int32), "pair_num": np.ones((1,), np.int32)}
        O.conv_fwd(np.ones((1, 8), np.float32), np.ones((1, 8, 8), np.float32), None, tiny, threads=threads)

    def timed(name, fn):
        t0 = time.perf_counter()
        r = fn()
        t_total[name] = t_total.get(name, 0.0) + (time.perf_counter() - t0)
        return r

    pts = synth.synth_cloud(frame)
    v, c, n = timed("voxelize", lambda: O.voxelize_hard(pts, synth.WAYMO_RANGE, synth.WAYMO_VOXEL, 5, 150000))
    timed("mean_vfe", lambda: O.mean_vfe(v, n))
    idx = np.pad(c, ((0, 0), (1, 0))).astype(np.int32)
    shape = (41, 1504, 1504)
    levels = [(16, dict(k=3, s=2, p=1), 32), (32, dict(k=3, s=2, p=1), 64), (64, dict(k=3, s=2, p=(0, 1, 1)), 128),
              (128, dict(k=(3, 1, 1), s=(2, 1, 1), p=0), 128)]

    def conv_fb(rb, cin, cout):
        x = rng.normal(size=(rb["n_in"], cin)).astype(np.float32)
        w = (rng.normal(size=(rb["K"], cin, cout)) * 0.1).astype(np.float32)
        y = timed("conv", lambda: O.conv_fwd(x, w, None, rb, threads=threads))
        timed("conv", lambda: O.conv_bwd(x, w, y, rb, threads=threads))

    def bn_relu(nrows, ch):
        x = torch.randn(nrows, ch, requires_grad=True)
        bn = torch.nn.BatchNorm1d(ch, eps=1e-3, momentum=0.01)

        def f():
            y = torch.relu(bn(x))
            y.sum().backward()
        timed("bn_relu", f)

    first = True
    for cl, geo, cnext in levels:
        rb = timed("rulebook", lambda: O.rulebook_subm(idx, shape))
        if first:
            conv_fb(rb, 5, 16)                       # conv_input
            bn_relu(rb["n_out"], 16)
            first = False
        for _ in range(4):                           # 2 SparseBasicBlocks = 4 SubM convs + 4 BatchNorms
            conv_fb(rb, cl, cl)
            bn_relu(rb["n_out"], cl)
        rc = timed("rulebook", lambda: O.rulebook_conv(idx, shape, geo["k"], geo["s"], geo["p"]))
        conv_fb(rc, cl, cnext)
        bn_relu(rc["n_out"], cnext)
        idx, shape = rc["out_indices"], tuple(int(s) for s in rc["out_shape"])
    feat = rng.normal(size=(idx.shape[0], 128)).astype(np.float32)
    timed("bev", lambda: O.dense_bev(feat, idx, 1, shape))
    timed("bev", lambda: O.dense_bev(feat, idx, 1, shape))       # its gradient moves the same bytes
    return sum(t_total.values()), dict(t_total)


# ---------------------------------------------------------------------------------------------
def launch_self(args):
    """`python bench.py --gpus N` without a launcher: THIS process (which has not touched the GPU) starts N child
    ranks of the same command line and forwards rank 0's JSON line (children inherit stdout); nothing is exec'ed
    over a process that initialised HIP.  Non-zero exit if any rank fails."""
    if not (args.selftest_launch or os.environ.get("PCD_DIST_ONE_GPU")):
        have = torch.cuda.device_count()          # counting devices does not initialise the GPU
        if have < args.gpus:
            print(f"[bench] --gpus {args.gpus} but only {have} GPU(s) visible", file=sys.stderr)
            return 2
    # the launcher's own deadline: whatever happens inside the ranks, `python bench.py --gpus N` returns within it
    codes = cdist.launch_local_ranks(args.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:],
                                     timeout=args.launch_timeout)
    bad = [(r, c) for r, c in enumerate(codes) if c != 0]
    if bad:
        print(f"[bench] ranks failed (rank, exit code): {bad}", file=sys.stderr)
        return 1
    return 0


def selftest_launch(args, rank, world):
    """CPU plumbing check used by tests/test_distributed_cpu.py: the launcher, the rank environment, the frame
    sharding, the max-over-ranks timing and the result line, over gloo; no GPU work and no numbers of record."""
    import datetime
    whole = cdist.Watchdog(args.rank_timeout, "the whole run")
    with cdist.Watchdog(args.init_timeout, "rendezvous"):
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=args.init_timeout))
    if rank == args.selftest_hang:
        time.sleep(3600)                                     # a peer that never arrives: every other rank's watchdog fires
    first = cdist.first_all_reduce("cpu", args.init_timeout)
    assert first == world * (world + 1) / 2
    # the real exchange of a step: the flat gradient bucket of the sparse backbone (10.78 MB fp32), summed over the ranks
    from com_amd.hotpath import VoxelResBackBone8x
    torch.manual_seed(666)
    bucket = cdist.FlatGradBucket(VoxelResBackBone8x({}, 5, [1504, 1504, 40]).parameters())
    bucket.flat.fill_(float(rank + 1))
    bucket.all_reduce_sum()
    bucket_ok = bool((bucket.flat == world * (world + 1) / 2).all())
    t = torch.tensor([float(rank + 1)])
    dist.all_reduce(t)
    frames = cdist.shard_frames(0, rank, world, args.batch)
    gathered = [None] * world
    dist.all_gather_object(gathered, frames)
    slowest = cdist.max_over_ranks(1.0 + rank)
    if rank == 0:
        print(json.dumps({"metric": METRIC, "selftest": True, "n_gpus": world, "rccl_ranks": dist.get_world_size(),
                          "allreduce_sum": float(t.item()), "frames": gathered, "slowest": slowest,
                          "bucket_MB": round(bucket.flat.numel() * 4 / 1e6, 2), "bucket_sum_ok": bucket_ok,
                          "steps": args.steps, "warmup": args.warmup}), flush=True)
    # the closing barrier as an all-reduce of a CPU tensor: dist.barrier() asks the HIP runtime for its devices, which opens
    # the GPU in every rank of a job that must not touch it
    dist.all_reduce(torch.zeros(1))
    dist.destroy_process_group()
    whole.disarm()


class ResidentSource:
    """Batches resident in HBM before the timed region (the contract's `value`)."""

    def __init__(self, batches):
        self.batches = batches

    def get(self, j):
        return self.batches[j % len(self.batches)]

    def release(self, j):
        pass


class H2DSource:
    """a3 inside the step (dataset.py:252-259 + load_data_to_gpu, pcdet/models/__init__.py:23-34): the collated
    points of every batch start in PINNED HOST memory and are copied host -> device on a copy stream, two batches
    ahead, overlapped with the compute of the steps in between; the consumer waits on the batch's event only.
    This loop is BIMODAL on the gpurun boxes: the same command gives 3.45 or 4.0-4.8 ms per step (PCD_BENCH_DEBUG=1 prints
    where the launching thread's time goes: replaying the step's hipGraph costs it 1.5 ms, the rest of the slow mode is spent
    in `get()` waiting for the slot's copy, although a 15.4 MB copy takes 0.29 ms on the GPU clock beside the step).
    Neither binding the process to either socket's cores, nor a helper thread that enqueues the copies (PCD_H2D_THREAD=1),
    nor more slots (PCD_H2D_DEPTH) removes the slow mode; the HBM-resident `value` never shows it.  What does: choosing the
    copy STREAM (the caller tries several for a few steps each -- the stream -> hardware queue mapping is what differs).  In BOTH modes the launching
    thread spends its time waiting in `get()` (2.6 vs 3.8 ms per step) and 0.5 ms replaying the graph: the loop is GPU-bound,
    the replayed step itself runs longer in the slow mode; a HIGH-priority copy stream (PCD_H2D_PRIO=-1) makes every run
    slow (6.6-7.7 ms) -- how the copy queue is arbitrated against the graph's queues decides, not the 0.29 ms copy."""

    def __init__(self, batches, dev, stream=None, host=None):
        import queue
        import threading
        self.host = host or [(p.cpu().pin_memory(), o.cpu().pin_memory()) for p, o in batches]
        self.depth = D = max(2, int(os.environ.get('PCD_H2D_DEPTH', '2')))   # batches in flight ahead of the consumer
        self.stage = [(torch.empty_like(batches[0][0]), torch.empty_like(batches[0][1])) for _ in range(D)]
        self.ready = [torch.cuda.Event() for _ in range(D)]
        self.stream = stream or torch.cuda.Stream(device=dev, priority=int(os.environ.get('PCD_H2D_PRIO', '0')))
        self.stream.wait_stream(torch.cuda.current_stream())
        self.dev = dev
        self.issued = self.taken = 0
        self.copy_events = []
        self.threaded = bool(os.environ.get('PCD_H2D_THREAD'))
        self.jobs, self.done = queue.Queue(), [threading.Event() for _ in range(D)]
        self.error = None
        if self.threaded:
            self.worker = threading.Thread(target=self._work, daemon=True)
            self.worker.start()
        for _ in range(D):
            self._issue(None)

    def _copy(self, k, after):
        hp, ho = self.host[k % len(self.host)]
        with torch.cuda.stream(self.stream):
            if after is not None:
                self.stream.wait_event(after)                # the consumer's reads of this slot's previous batch
            timed = os.environ.get('PCD_BENCH_DEBUG') and k >= 8 and len(self.copy_events) < 24
            if timed:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record(self.stream)
            self.stage[k % self.depth][0].copy_(hp, non_blocking=True)       # 15.4 MB host -> device
            self.stage[k % self.depth][1].copy_(ho, non_blocking=True)
            if timed:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record(self.stream)
                self.copy_events.append((e0, e1))
            self.ready[k % self.depth].record(self.stream)

    def _work(self):
        torch.cuda.set_device(self.dev)
        while True:
            job = self.jobs.get()
            if job is None:
                return
            k, after = job
            try:
                self._copy(k, after)
            except Exception as exc:                        # surfaced by the next get()
                self.error = exc
            self.done[k % self.depth].set()

    def _issue(self, after):
        k = self.issued
        self.issued += 1
        if self.threaded:
            self.done[k % self.depth].clear()
            self.jobs.put((k, after))
        else:
            self._copy(k, after)

    def get(self, j):
        """Next batch in sequence (batches alternate; `j` is the consumer's step counter, informational)."""
        k = self.taken
        self.taken += 1
        assert self.issued == k + self.depth, "one release() per get()"
        if self.threaded:
            self.done[k % self.depth].wait()                          # the helper thread has enqueued this slot's copies
            if self.error is not None:
                raise self.error
        if os.environ.get('PCD_H2D_STREAM_WAIT'):
            torch.cuda.current_stream().wait_event(self.ready[k % self.depth])
        else:
            # the copy was issued two steps ago: the HOST waits for it (it has long finished; this only keeps the
            # host from running more than two steps ahead) instead of putting a cross-queue barrier in front of
            # every step on the compute stream
            self.ready[k % self.depth].synchronize()
        return self.stage[k % self.depth]

    def release(self, j):
        """The consumer's reads of the batch just taken have been issued on the current stream: refill its slot."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self._issue(ev)

    def close(self):
        if self.threaded:
            self.jobs.put(None)
            self.worker.join(timeout=10)


class PullSource:
    """a3 inside the captured step, without a copy stream: the batches sit in pinned host memory, a device-side table holds
    their addresses, and a kernel of the step's OWN graph (pcd_pull_from_host, a parallel branch from the start of the
    step) reads batch (counter % n) over PCIe into the buffer the step's voxeliser reads at its end; pcd_counter_add moves
    the counter.  The host replays the graph and does nothing else."""

    def __init__(self, batches, dev):
        rows = batches[0][0].shape[0]
        assert all(p.shape == batches[0][0].shape for p, _ in batches) and (rows * batches[0][0].shape[1] * 4) % 16 == 0
        self.host = []
        for p, o in batches:
            o8 = torch.zeros(8, dtype=torch.int32)
            o8[:o.numel()] = o.cpu()
            self.host.append((p.cpu().pin_memory(), o8.pin_memory()))
        self.tab_p = torch.tensor([h[0].data_ptr() for h in self.host], dtype=torch.int64, device=dev)
        self.tab_o = torch.tensor([h[1].data_ptr() for h in self.host], dtype=torch.int64, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.n = len(self.host)
        self.dev = dev
        self.copy_events = []

    def enqueue(self, s_pts, s_offs8):
        """current stream (also under capture): s_pts / s_offs8 <- host batch (counter % n); counter += 1"""
        from com_amd import _lib as L
        lib = L.lib()
        L.check(lib.pcd_pull_from_host(L.ptr(self.tab_p), self.n, L.ptr(self.counter), L.ptr(s_pts),
                                       s_pts.numel() * s_pts.element_size(), 128, L.stream_ptr()), "pcd_pull_from_host")
        L.check(lib.pcd_pull_from_host(L.ptr(self.tab_o), self.n, L.ptr(self.counter), L.ptr(s_offs8), 32, 1,
                                       L.stream_ptr()), "pcd_pull_from_host")
        L.check(lib.pcd_counter_add(L.ptr(self.counter), 1, L.stream_ptr()), "pcd_counter_add")

    def prime(self, s_pts, s_offs8):
        """batch 0 by the same kernel, eagerly (counter 0 -> 1), into the step's static input buffers"""
        self.counter.zero_()
        self.enqueue(s_pts, s_offs8)

    # the ResidentSource / H2DSource protocol, unused by the pull form of the step
    def get(self, j):
        raise RuntimeError("PullSource feeds the graph itself")

    def release(self, j):
        pass


def measure_stage2(B, dev):
    """`stage2` (BASELINE config 4 as a workload): PV-RCNN's second stage over the hot path's outputs at the sizes of
    pv_rcnn.yaml:87-118,161-166 -- VoxelBackBone8x on the same B x 160k-point frames, then (timed) farthest point sampling
    of 4096 keypoints per frame, ball-query set abstraction over raw points / x_conv3 / x_conv4 + BEV interpolation, and
    RoI-grid pooling for 128 RoIs x 6^3 grid points per frame (com_amd.hotpath.pvrcnn_stage2 over the HIP natives of
    com_amd.pointnet2_stack; tests/test_gpu_stage2.py checks every index tensor against the oracle at this size)."""
    from com_amd.hotpath import pvrcnn_stage2 as S2
    try:
        frames = [synth.synth_cloud(f) for f in range(B)]
        pts, offs = hotpath.collate_points(frames, dev)
        bd = hotpath.transform_points_to_voxels({"points": pts, "frame_offsets": offs, "batch_size": B}, synth.WAYMO_RANGE,
                                                synth.WAYMO_VOXEL, synth.WAYMO_MAX_POINTS, synth.WAYMO_MAX_VOXELS,
                                                fuse_mean=True)
        grid = ops.grid_size(synth.WAYMO_RANGE, synth.WAYMO_VOXEL)
        backbone = hotpath.VoxelBackBone8x({}, 5, grid).to(dev).eval()
        to_bev = hotpath.HeightCompression({"NUM_BEV_FEATURES": 256})
        vsa = S2.VoxelSetAbstraction(synth.WAYMO_VOXEL, synth.WAYMO_RANGE, 256, 5, backbone.backbone_channels).to(dev).eval()
        pool = S2.RoIGridPool(vsa.num_point_features).to(dev).eval()
        rs = np.random.default_rng(7)
        rois = np.zeros((B, 128, 7), np.float32)
        rois[..., 0:2] = rs.uniform(-60, 60, (B, 128, 2))
        rois[..., 2] = rs.uniform(-0.5, 1.5, (B, 128))
        rois[..., 3:6] = np.stack([rs.uniform(0.6, 10, (B, 128)), rs.uniform(0.5, 2.8, (B, 128)), rs.uniform(1, 3, (B, 128))], -1)
        rois[..., 6] = rs.uniform(-np.pi, np.pi, (B, 128))
        with torch.no_grad():
            bd = to_bev(backbone(bd))
            keep = ((pts[:, 1] >= synth.WAYMO_RANGE[0]) & (pts[:, 1] <= synth.WAYMO_RANGE[3]) &
                    (pts[:, 2] >= synth.WAYMO_RANGE[1]) & (pts[:, 2] <= synth.WAYMO_RANGE[4]))
            bd["points"] = pts[keep].contiguous()
            bd["point_frame_counts"] = torch.bincount(bd["points"][:, 0].long(), minlength=B).to(torch.int32)
            bd["spatial_features_stride"] = 8
            bd["rois"] = torch.from_numpy(rois).to(dev)
            scores = None

            def run():
                nonlocal scores
                out = vsa(bd)
                if scores is None:
                    scores = torch.sigmoid(torch.randn(out["point_features"].shape[0], device=dev))
                out["point_cls_scores"] = scores
                return pool(out)
            for _ in range(2):
                run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 5
            for _ in range(n):
                run()
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / n
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            S2.sample_keypoints(bd["points"], bd["point_frame_counts"], 4096)
            e1.record()
            torch.cuda.synchronize()
            # the reference's other sampler (SAMPLE_METHOD 'SPC', PV-RCNN++): points around the proposals, then SectorFPS
            # (6 azimuth sectors as one stacked FPS) -- per frame, as VoxelSetAbstraction.get_sampled_points loops
            xyz_all, fr = bd["points"][:, 1:4].contiguous(), bd["points"][:, 0].long()
            per_frame = [xyz_all[fr == b].contiguous() for b in range(B)]

            def run_spc():          # all B x 6 sectors in ONE stacked FPS (the reference: a Python loop over the frames)
                return S2.sectorized_proposal_centric_sampling_batch([bd["rois"][b] for b in range(B)], per_frame, 4096, 1.6, 6)
            run_spc()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            kp_spc = run_spc()
            torch.cuda.synchronize()
            ms_spc = 1e3 * (time.perf_counter() - t1)
            n_spc = [int(k.shape[0]) for k in kp_spc]
        # the same stage in the metric's direction: training-mode modules, forward + backward (gradients into every MLP /
        # BatchNorm parameter and back into the backbone's x_conv3 / x_conv4 features and the BEV map through the grouping
        # kernels' gradient, pcd_group_points_stack_grad; tests/test_gpu_stage2.py checks them against a torch restatement)
        vsa.train()
        pool.train()
        ms_feats = {}
        for name, t in bd["multi_scale_3d_features"].items():
            ms_feats[name] = t.replace_feature(t.features.detach().float().clone().requires_grad_(True))
        bdt = dict(bd)
        bdt["multi_scale_3d_features"] = ms_feats
        bdt["spatial_features"] = bd["spatial_features"].detach().float().clone().requires_grad_(True)

        def run_train():
            for q in list(vsa.parameters()) + list(pool.parameters()):
                q.grad = None
            out = vsa(dict(bdt))
            out["point_cls_scores"] = scores
            pooled = pool(out)
            (pooled * pooled).mean().backward()
        for _ in range(2):
            run_train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            run_train()
        torch.cuda.synchronize()
        ms_train = 1e3 * (time.perf_counter() - t0) / n
        return {"ms_per_batch": round(ms, 3), "frames_per_s": round(B / ms * 1e3, 1), "frames": B,
                "fps_4096_keypoints_ms": round(e0.elapsed_time(e1), 3),
                "spc_sampling": {"ms_per_batch": round(ms_spc, 3), "keypoints_per_frame": n_spc,
                                 "what": "SAMPLE_METHOD SPC instead of FPS: RoI-centric point filter (radius 1.6 m) + SectorFPS over 6 "
                                         "sectors, 4096 keypoints asked per frame, the sectors of ALL frames in one stacked FPS "
                                         "(frame by frame as the reference loops: 18.4 ms in round 4; not what the timed stage uses)"},
                "stage2_train": {"ms_per_batch": round(ms_train, 3), "frames_per_s": round(B / ms_train * 1e3, 1),
                                 "what": "the same stage in training mode, forward + backward (eager launches)"},
                "what": "PV-RCNN stage 2 (eval forward): FPS 4096 keypoints/frame from raw points (bucket-pruned exact kernel: one "
                        "workgroup per frame, ~13 of 1250 buckets touched per sample) + set abstraction over raw points, x_conv3, "
                        "x_conv4 + BEV + RoI-grid pooling 128 RoIs x 216 points/frame"}
    except Exception as exc:
        return {"error": f"{type(exc).__name__}: {exc}"}


def measure_seam_path(W, captured_fps, dev, steps=20):
    """`seam_path`: frames/s of the SAME workload at the three levels of integration INTEGRATION.md describes, measured in
    this run -- what a user of each seam gets:
      stock_eager   seams 1-3 only: a backbone written like a stock model file (tools/seam1_model.py: spconv.* names, torch
                    BatchNorm1d / ReLU / residual add, fp32 features), the reference's loop with torch.optim.Adam +
                    clip_grad_norm_, eager launches;
      fused_eager   + seam 3a (com_amd.hotpath backbone) + the flat bucket / FlatAdam, com_amd.train.CapturedStep WITHOUT
                    capture(): the same loop, one launch per kernel from Python;
      captured      the same object after capture(): the headline `value`."""
    import seam1_model as S
    B, batches = W.B, W.batches
    out = {"unit": "frames/s", "captured": round(captured_fps, 1), "steps": steps}
    try:
        step = W.step
        step.release()
        step.prime(batches[0])
        for i in range(3):
            step(batches[(i + 1) % len(batches)])
        torch.cuda.synchronize()
        gc.collect()
        t0 = time.perf_counter()
        train.train_one_epoch(step, batches, steps, accumulated_iter=step.lr_scheduler.last_iter + 1, gc_collect=False)
        torch.cuda.synchronize()
        out["fused_eager"] = round(B * steps / (time.perf_counter() - t0), 1)
    except Exception as exc:
        out["fused_eager_error"] = f"{type(exc).__name__}: {exc}"
    try:
        grid = ops.grid_size(synth.WAYMO_RANGE, synth.WAYMO_VOXEL)
        torch.manual_seed(666)
        backbone = S.StockVoxelResBackBone8x(5, grid).to(dev).train()
        to_bev = hotpath.HeightCompression({"NUM_BEV_FEATURES": 256})
        optim = torch.optim.Adam(backbone.parameters(), lr=3e-4, betas=(0.9, 0.99))
        loss_w = (torch.randn(B * 256 * 188 * 188, device=dev) * 1e-3)
        from com_amd.spconv import functional as Fsp

        def stock_step(batch):
            pts, offs = batch
            bd = hotpath.transform_points_to_voxels({"points": pts, "frame_offsets": offs, "batch_size": B}, synth.WAYMO_RANGE,
                                                    synth.WAYMO_VOXEL, synth.WAYMO_MAX_POINTS, synth.WAYMO_MAX_VOXELS, fuse_mean=True)
            optim.zero_grad()
            bd = to_bev(backbone(bd))
            loss = (bd["spatial_features"].float().reshape(-1) * loss_w).sum()
            loss.backward()
            Fsp.join_deferred_wgrad()
            torch.nn.utils.clip_grad_norm_(backbone.parameters(), 10.0)
            optim.step()
        for i in range(3):
            stock_step(batches[i % len(batches)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            stock_step(batches[i % len(batches)])
        torch.cuda.synchronize()
        out["stock_eager"] = round(B * steps / (time.perf_counter() - t0), 1)
    except Exception as exc:
        out["stock_eager_error"] = f"{type(exc).__name__}: {exc}"
    out["what"] = ("same B x 160k-point batches, whole training step (voxelise -> backbone -> BEV -> loss -> backward -> clip -> "
                   "Adam): stock model file over import seams 1-3 with torch's optimizer, eager | fused backbone + flat "
                   "optimizer through com_amd.train.CapturedStep without capture, eager | the same object captured (= value)")
    return out


def measure_regime():
    """`roofline.rulebook`: the rulebook chain of one forward pass (9 builds) at B = 4 (reference batch) and B = 32 (the
    bandwidth regime SURVEY 8d asks for), algorithmic bytes 16 N_in + 8 P (+ 16 N_out) over the time of the builds
    replayed from a hipGraph, as fractions of the 8 TB/s HBM peak -- tools/regime.py run as a child process."""
    import subprocess
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "regime.py"), "4", "32"], cwd=ROOT,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        rows = [json.loads(l) for l in out.stdout.decode().splitlines() if l.startswith("{")]
        if out.returncode != 0 or not rows:
            return {"error": f"rc {out.returncode}: {out.stderr.decode()[-300:]}"}
        res = {"unit": "fraction of 8 TB/s over SURVEY 8d's algorithmic bytes", "north_star_floor": 0.60}
        for r in rows:
            res[f"B{r['frames']}"] = {"chain_us_graph": r["rulebook_chain_graph_us"], "chain_us_eager": r["rulebook_chain_us"],
                                      "alg_MB": r["alg_MB"], "GBps_graph": r["graph_GBps"], "frac": r["graph_frac_of_8TBps"],
                                      # (the same chain with pair lists only where the step builds them: levels 3 and 4 + strided)
                                      "chain_us_graph_as_built": r.get("as_built_chain_graph_us"),
                                      "frac_as_built": r.get("as_built_frac_of_8TBps"),
                                      "builds_us_graph": {f"{b['kind']}_L{b['level']}": b["graph_us"] for b in r["builds"]}}
        return res
    except Exception as exc:
        return {"error": f"{type(exc).__name__}: {exc}"}


def measure_full_model(args, flags=("--dense-head", "--com"), what=None, extra_env=None):
    """`full_model`: the complete CenterPoint-VoxelNet + COM-head training step (what a user of the reference would
    run), measured by a CHILD process (`bench.py --dense-head --com`, same batch / steps) after this process's own
    loops have finished; the child is a new process, nothing is exec'ed over this one, and it is a plain run (no
    `--full`).  (`config5_300k` reuses this with `--config5`.)"""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), *flags, "--gpus", "1", "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--batch", str(args.batch), "--distinct-batches", str(args.distinct_batches)]
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(extra_env or {})
    try:
        t0 = time.perf_counter()
        out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        line = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
        if out.returncode != 0 or not line:
            return {"error": f"child rc {out.returncode}: {out.stderr.decode()[-400:]}"}
        r = json.loads(line[-1])
        return {"value": r["value"], "unit": r["unit"], "ms_per_step": r["ms_per_step"], "steps": r["steps"],
                "config": r["config"]["workload"], "com": r.get("com"), "child_wall_s": round(time.perf_counter() - t0, 1),
                "points_per_frame": r["config"].get("points_per_frame"), "voxels_per_frame": r["config"].get("voxels_per_frame"),
                "what": what or "child run `bench.py --dense-head --com`: hot path + BaseBEVBackbone + CenterHead towers + "
                        "COM curriculum targets / FocalLossCenterCurriculum / RegLoss, one hipGraph per step"}
    except Exception as exc:                                  # never lose the headline
        return {"error": f"{type(exc).__name__}: {exc}"}


class _SourceFeed:
    """A ResidentSource / H2DSource as the iterator com_amd.train.train_one_epoch draws from: batch k + 1 while the step
    trains on batch k (the data side runs one batch ahead); `staged` refills the source's slot once the step has enqueued
    its copies of the batch."""

    def __init__(self, source):
        self.source, self.k = source, 0

    def __iter__(self):
        return self

    def __next__(self):
        self.k += 1
        return self.source.get(self.k)

    def staged(self):
        self.source.release(self.k)


class _Repeat:
    """(pull form: the graph fetches its own batches -- the loop has nothing to hand over)"""

    def __init__(self, value):
        self.value = value

    def __iter__(self):
        return self

    def __next__(self):
        return self.value

    def staged(self):
        pass


class Workload:
    pass


def build_workload(args, rank, world, dev, rccl_world1=False):
    """Model, synthetic batches, optimizer and the com_amd.train.CapturedStep of one rank -- everything main() times, also
    what tests/test_gpu_train_step.py drives from its own reference-shaped loop."""
    W = Workload()
    W.B = B = args.batch
    torch.manual_seed(666 + (0 if args.same_shard else rank))   # cf. tools/train.py:86-87
    # frames sharded by rank with DistributedSampler striding (pcdet/datasets/__init__.py:65-72 ->
    # com_amd.dist.shard_frames); `--distinct-batches` (16) global batches of DISTINCT full 160k-point frames cycle
    # through the timed loop: voxel / row counts differ from step to step (M = 80..87 k per frame), the static
    # capacities are sized from the warm-up steps only, and a denser batch would trip the overflow guard
    W.n_batches = n_batches = max(2, args.distinct_batches)
    BEAMS = 120 if args.config5 else 64                       # 120 x 2500 = 300 000 points per frame (config 5)

    def make_batches(drop=None):
        out = []
        for j in range(n_batches):
            ids = cdist.shard_frames(j, 0, 1, B) if args.same_shard else cdist.shard_frames(j, rank, world, B)
            frames = [synth.synth_cloud(f, BEAMS, 2500) for f in ids]
            if drop is not None:                             # ragged variant: 0-20 % of every frame's rays are lost
                frames = [f[:int(round(f.shape[0] * (1.0 - drop.uniform(0.0, 0.2))))] for f in frames]
            pts, offs = hotpath.collate_points(frames, dev)  # resident in HBM before the timed region
            out.append((pts, torch.tensor(offs, dtype=torch.int32, device=dev)))
        return out

    def pad_batches(bs, rows):
        return [(torch.nn.functional.pad(p, (0, 0, 0, rows - p.shape[0])) if p.shape[0] < rows else p, o) for p, o in bs]

    batches = make_batches()
    # the static graph reads ONE point buffer: batches are padded to a common row count (offsets say what is real)
    W.nmax = nmax = (max(p.shape[0] for p, _ in batches) + 1) // 2 * 2     # (even: whole 16-byte pieces for the in-graph host pull)
    W.batches = batches = pad_batches(batches, nmax)
    W.make_batches, W.pad_batches = make_batches, pad_batches
    W.resident = ResidentSource(batches)

    ops.WGRAD_OS = os.environ.get('PCD_WGRAD_OS', '1') != '0'            # output-stationary wgrad at 16 channels
    W.model = model = HotPath(dense_head=args.dense_head, plain=args.config5).to(dev)
    model.train()
    if world > 1:                                            # what DDP does at construction (tools/train.py:165-166)
        for t in list(model.parameters()) + list(model.buffers()):
            dist.broadcast(t.data, 0)
    params = [p for p in model.parameters() if p.requires_grad]
    if args.dense_head and os.environ.get('PCD_HEAD_BATCHED', '1') != '0':
        # the head branches' first-stage parameters back to back in the flat buffers: their batched path (dense2d.py)
        from com_amd.hotpath import dense2d as _d2
        params = [p for p in _d2.batched_param_order(model) if p.requires_grad]
    # all gradients live in ONE flat fp32 buffer: the per-step exchange is a single RCCL all-reduce (10.8 MB); so do the
    # parameters: clipping + Adam are two passes over the flat buffers (pcd_adam_flat_step_v4) with the reference's
    # adam_onecycle rule: decoupled weight decay, betas (MOMS, 0.99), lr / momentum from the OneCycle schedule
    # (tools/train_utils/optimization/__init__.py:19-32,53-56; centerpoint.yaml:81-96), GRAD_NORM_CLIP 10
    total_iters = 30 * 1000                                  # schedule length only shapes lr(it) / mom(it)
    lr0, mom0 = cdist.one_cycle(0, total_iters)
    W.opt = opt = train.build_optimizer(params, lr=lr0, weight_decay=0.01, moms=(mom0, 0.85), grad_norm_clip=10.0, world=world)
    W.bucket = bucket = opt.bucket
    bucket.force_collective = rccl_world1
    W.flat_param = bucket.flat_param
    # OneCycle as a device table indexed by the optimizer's own step counter (looked up inside the replayed graph): no
    # 8-byte host -> device copy in front of every step (PCD_DEVICE_SCHEDULE=0: set_hyper per step)
    lr_scheduler = train.OneCycle(opt, total_iters, device_table=os.environ.get('PCD_DEVICE_SCHEDULE', '1') != '0')
    # stand-in for the dense head when only the hot path is timed: loss = <spatial_features, fixed random tensor>
    # (ops.LinearFunctionalLoss: pcd_dot_bf16 forward, pcd_scale_bf16 backward -- 2 + 1 HIP launches)
    loss_w = (torch.randn(B * 256 * 188 * 188, device=dev) * 1e-3).to(torch.bfloat16)

    CLASS_NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']
    after_update = [model.backbone_3d.pack_after_update]
    if args.dense_head:
        from com_amd.hotpath import center_loss, dense2d, targets
        # get_loss in four HIP launches per head (centerhead.hip); PCD_LOSS_TORCH=1: the elementwise torch chain
        loss_cls = center_loss.CenterHeadLoss if os.environ.get('PCD_LOSS_TORCH') else center_loss.FusedCenterHeadLoss
        head_loss = loss_cls(dense2d.CENTERPOINT_HEAD['SEPARATE_HEAD_CFG']['HEAD_ORDER'],
                             cls_weight=1.0, loc_weight=2.0).to(dev)                        # centerpoint.yaml:52-58
        from com_amd.hotpath import conv2d_fast
        conv_packs = conv2d_fast.Conv3x3Packs(model)       # all dense 3x3 weight packs in one launch per step
        after_update.append(conv_packs.run)
        rs = np.random.default_rng(1234 + (0 if args.same_shard else rank))
        gtb = np.zeros((B, 96, 8), np.float32)             # [x, y, z, dx, dy, dz, heading, class], 0 = padding
        for b in range(B):
            n = int(rs.integers(40, 90))
            cls = rs.integers(1, 4, n)
            gtb[b, :n, 0:2] = rs.uniform(-74, 74, (n, 2))
            gtb[b, :n, 2] = rs.uniform(-1, 2, n)
            gtb[b, :n, 3] = np.where(cls == 1, rs.uniform(3.5, 12, n), rs.uniform(0.5, 2.0, n))
            gtb[b, :n, 4] = np.where(cls == 1, rs.uniform(1.6, 3.0, n), rs.uniform(0.4, 1.0, n))
            gtb[b, :n, 5] = rs.uniform(1.0, 3.0, n)
            gtb[b, :n, 6] = rs.uniform(-np.pi, np.pi, n)
            gtb[b, :n, 7] = cls
        gt_boxes = torch.from_numpy(gtb).to(dev)
        if args.com:
            # BASELINE config 3: CurriculumCenterHead_x5 (head_zoo.py:145-149) on the voxel backbone's stride-8 map, the
            # LOSS_CURRICULUM of tools/cfgs/waymo_models/com/centercurriculum_pillar_3cls_b2_com.yaml:168-173 (UCL False,
            # FIX True) unless --com-ucl; per-object attributes COMAug's dataloader provides, synthetic here
            from com_amd.hotpath import com_head
            W.com_cur = com_cur = dict(UCL=bool(args.com_ucl), THRESHOLD=0.2, ELONGATION=-10, HEIGHT=1, FIX=True)
            head_loss = com_head.CurriculumCenterHeadLoss(dense2d.CENTERPOINT_HEAD['SEPARATE_HEAD_CFG']['HEAD_ORDER'],
                                                          com_cur, conf_shape=(3, 96), cls_weight=1.0, loc_weight=2.0).to(dev)
            valid = gtb[..., 7] > 0
            com_npgt = torch.from_numpy(np.where(valid, rs.integers(1, 400, valid.shape), 0).astype(np.float32)).to(dev)
            com_true = torch.from_numpy(np.where(valid, rs.choice([1, 1, 1, 2], valid.shape), 0).astype(np.float32)).to(dev)
            com_occ = torch.from_numpy(np.where(valid, rs.random(valid.shape), 0).astype(np.float32)).to(dev)
            com_facade = torch.from_numpy(np.where(valid, rs.integers(0, 4, valid.shape), 0).astype(np.float32)).to(dev)
            com_epoch = 5
        W.head_loss = head_loss

    def model_func(model, bd):
        """model_func of the reference's loop (pcdet/models/__init__.py:37-51): batch_dict -> loss.
        MeanVFE -> VoxelResBackBone8x -> HeightCompression (-> BaseBEVBackbone -> CenterHead / COM head) -> loss"""
        bd = model.map_to_bev_module(model.backbone_3d(model.vfe(bd)))
        if ops.STAMPS is not None and bd["spatial_features"].requires_grad:
            bd["spatial_features"].register_hook(lambda g: ops.stamp("dense_bwd_end"))
        if args.dense_head:
            # BaseBEVBackbone + CenterHead towers (bf16 / channels_last, conv2d.hip kernels), then the REAL CenterHead step of the
            # reference: target assignment for this batch's boxes (centerhead.hip, on the device, inside the graph)
            # and get_loss = focal(hm) + L1(boxes) (center_head.py:163-262) without its host round trips
            preds = model.dense_head(model.backbone_2d(bd))["pred_dicts"]
            ops.stamp("dense_fwd_end")
            if args.com:
                # CurriculumCenterHead.forward / get_loss (curriculum_center_head.py:461-487,313-358) on the device
                group = com_head.cluster(gt_boxes, com_true, com_occ, com_facade)
                tg = com_head.assign_targets(gt_boxes, (188, 188), CLASS_NAMES, [CLASS_NAMES], synth.WAYMO_RANGE,
                                             synth.WAYMO_VOXEL, 8, com_npgt, true_object=group, num_max_objs=500,
                                             gaussian_overlap=0.1, min_radius=2, epoch=com_epoch, epoch_threshold=100,
                                             min_points=0)
                loss, _ = head_loss(preds, tg, epoch=com_epoch)
            else:
                tg = targets.assign_targets(gt_boxes, (188, 188), CLASS_NAMES, [CLASS_NAMES], synth.WAYMO_RANGE,
                                            synth.WAYMO_VOXEL, 8, num_max_objs=500, gaussian_overlap=0.1, min_radius=2)
                loss, _ = head_loss(preds, tg)
        else:
            # stand-in for the dense head's loss: a fixed random projection of the BEV map (non-trivial dense gradient)
            loss = ops.LinearFunctionalLoss.apply(bd["spatial_features"], loss_w)
        return loss

    # voxel rows numbered by (b, y, x, z) -- z fastest, PCD_ROWS_YXZ: the same voxels as the reference's voxeliser (the caps are
    # decided by first appearance), every level of the chain numbered the same way, the SubM layers through the window
    # gather-GEMM; PCD_ROW_ORDER=key = (b, z, y, x) (torch.unique / spconv's sorted order), first = first-appearance ids
    vox = train.VoxelizeConfig(synth.WAYMO_RANGE, synth.WAYMO_VOXEL, synth.WAYMO_MAX_POINTS, synth.WAYMO_MAX_VOXELS,
                               row_order=os.environ.get('PCD_ROW_ORDER', 'yxz'))
    if world == 1 and not os.environ.get('PCD_FORCE_3GRAPH') and not rccl_world1:   # (the switches exercise the N > 1 form on one GPU)
        form = "one_graph"
    else:
        form = "three_graph" if os.environ.get('PCD_N_GT_1_FORM', 'early') == '3graph' else "n_gt_1"
    hook_at = os.environ.get('PCD_HOOK_AT', 'conv3')
    W.step = train.CapturedStep(model, model_func, opt, vox, B, lr_scheduler=lr_scheduler, world=world, form=form,
                                hook_at=None if hook_at == "units" else hook_at, after_update=after_update,
                                options={"WGRAD_JOIN_LAG": int(os.environ.get('PCD_WGRAD_LAG', '32')),
                                         "FUSE_BN_REDUCTIONS": os.environ.get('PCD_FUSE_BN', '1') != '0'})
    return W


def main():
    args = parse()
    if args.com:
        args.dense_head = True
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_self(args))             # before anything touches the GPU
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"[bench] WORLD_SIZE={world} but --gpus {args.gpus}: launch one rank per GPU "
              f"(python -m torch.distributed.run --nproc-per-node {args.gpus} bench.py --gpus {args.gpus} ...)",
              file=sys.stderr)
        sys.exit(2)
    cdist.apply_rank_affinity()                              # (opt-in pinning of launch_local_ranks, before any GPU call)
    if args.selftest_launch:
        return selftest_launch(args, rank, world)
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    if os.environ.get("PCD_DIST_ONE_GPU"):                   # validation of the multi-rank control flow on a 1-GPU box
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # experiment switches of the sweep scripts (PCD_OPT_*, PCD_RB_*, ...): the product modules read no environment variable
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import env_switches
    env_switches.apply()
    # (opt-in, PCD_BIND_GPU_NUMA=1: launch thread + pinned staging buffers on the GPU's own NUMA node.  Measured on a
    #  2-socket gpurun box: the HBM-resident loop is unchanged (3.39 ms) and the H2D-inclusive loop gets SLOWER when bound to
    #  the node sysfs reports as local -- 4.8 vs 3.47 ms per step -- so it is off)
    if os.environ.get("PCD_BIND_CPUS"):                      # experiments: "a-b" CPU range for this process
        a_, b_ = os.environ["PCD_BIND_CPUS"].split("-")
        os.sched_setaffinity(0, set(range(int(a_), int(b_) + 1)))
    if os.environ.get("PCD_BIND_GPU_NUMA") and not os.environ.get("PCD_DIST_ONE_GPU"):
        cdist.bind_to_gpu_numa(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))))
    rccl_world1 = world == 1 and bool(os.environ.get("PCD_RCCL_WORLD1"))
    whole_run = None
    if world > 1:
        # No phase of a multi-rank run may hang the job: the process group carries a collective timeout (torch's RCCL watchdog
        # ends a rank whose collective exceeds it), rendezvous + communicator set-up + the first all-reduce run under a deadline
        # of their own, and so does the whole run -- a rank that misses one exits with code 124 (fresh child processes only,
        # nothing re-exec'ed); the launcher / torch.distributed.run then stops the others.
        import datetime
        whole_run = cdist.Watchdog(args.rank_timeout, "the whole run")
        backend = os.environ.get("PCD_DIST_BACKEND", "nccl")   # nccl == RCCL on ROCm (gloo only for that validation)
        with cdist.Watchdog(args.init_timeout, "rendezvous / init_process_group"):
            dist.init_process_group(backend, timeout=datetime.timedelta(seconds=args.init_timeout),
                                    **({"device_id": dev} if backend == "nccl" else {}))
        cdist.first_all_reduce(dev if backend == "nccl" else "cpu", args.init_timeout)
    elif rccl_world1:
        # validation on a 1-GPU box: a real RCCL communicator of ONE rank; the N > 1 three-graph form then runs with the
        # real dist.all_reduce of the flat bucket between the graph replays (sum over one rank = identity)
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)

    W = build_workload(args, rank, world, dev, rccl_world1)
    B, model, step, batches, resident, nmax = W.B, W.model, W.step, W.batches, W.resident, W.nmax
    bucket, opt, flat_param, n_batches, make_batches, pad_batches = W.bucket, W.opt, W.flat_param, W.n_batches, W.make_batches, W.pad_batches
    use_graph = args.mode == "graph"

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    # eager warm-up steps: real training steps that also observe the data-dependent row counts for the step's plan
    for i in range(max(args.warmup, 2)):
        step.lr_scheduler.step()
        step.eager(resident.get(i))
        if args.config5 and i == 0 and not os.environ.get('PCD_CONFIG5_BF16'):   # (the switch: same workload, bf16 forward)
            # calibrate on the first batch (amax of every conv input / weight -> static e4m3 scales), then every
            # sparse conv with >= 16 input channels runs its FORWARD in fp8 (backward: bf16, straight-through)
            from com_amd.spconv import fp8 as fp8mod
            with torch.no_grad():
                bd0 = {k: v for k, v in step.last_voxel_batch.items() if k != "_result"}
                scales = fp8mod.enable_fp8_training(model.backbone_3d, model.vfe(bd0))
            W.fp8_layers = len(scales)

    def timed_loop(steps, source, pull=False):
        """(elapsed seconds, host-issue seconds) of `steps` steps bracketed by barrier + synchronize: the loop is
        com_amd.train.train_one_epoch -- the reference's loop body (train_utils.py:78-95) over the step object."""
        if pull:
            step.prime(None)
            feed = _Repeat(None)
        else:
            step.prime(source.get(0), staged=lambda: source.release(0))
            feed = _SourceFeed(source)
        gc.collect()                                         # (tens of milliseconds: outside the timed region)
        sync()
        t0 = time.perf_counter()
        train.train_one_epoch(step, feed, steps, accumulated_iter=step.lr_scheduler.last_iter + 1, on_staged=feed.staged,
                              gc_collect=False)
        host_issue = time.perf_counter() - t0
        sync()
        return time.perf_counter() - t0, host_issue

    if use_graph:
        try:
            step.capture(batches[0], validate=batches[:3])
        except Exception as exc:                             # never lose the measurement: fall back to eager
            print(f"[bench] hipGraph capture failed ({type(exc).__name__}: {exc}); running eagerly", file=sys.stderr)
            use_graph = False
            step.release()
            torch.cuda.synchronize()

    if os.environ.get('PCD_STAMPS'):
        # time points inside the replayed graph (device clock, 100 MHz), averaged over the timed steps
        ops.STAMPS = {"buf": torch.zeros((128,), dtype=torch.int64, device=dev), "names": [],
                      "sparse": os.environ.get('PCD_STAMPS') == 'sparse'}     # (per-layer dgrad / wgrad time points)
        if os.environ.get('PCD_STAMPS') == 'few':
            ops.STAMPS["only"] = {"fwd_begin", "conv1", "conv2", "conv3", "conv4", "loss_end", "bwd_end", "step_end"}
        if use_graph:
            step.release()
            step.capture(batches[0])                         # (again: the stamp kernels are nodes of the graph)
        step.prime(resident.get(0))
        acc = None
        for i in range(10):
            step(resident.get(i + 1))
            torch.cuda.synchronize()
            v = ops.STAMPS["buf"].cpu().numpy().astype(np.float64)[:len(ops.STAMPS["names"])]
            if i >= 2:
                d = (v - v[0]) / 100.0
                acc = d if acc is None else acc + d
        print("[stamps us] " + "  ".join(f"{n}={a / 8:.0f}" for n, a in zip(ops.STAMPS["names"], acc)), file=sys.stderr)
    elapsed, host_issue = timed_loop(args.steps, resident)
    if os.environ.get('PCD_BENCH_DEBUG'):
        print(f"[bench] host issue {1e3 * host_issue / max(args.steps, 1):.3f} ms/step, "
              f"wall {1e3 * elapsed / max(args.steps, 1):.3f} ms/step", file=sys.stderr)
    local_ms = 1e3 * elapsed / max(args.steps, 1)
    elapsed = cdist.max_over_ranks(elapsed, dev)
    ms_per_step = 1e3 * elapsed / max(args.steps, 1)
    fps = world * B * args.steps / elapsed
    step.check()                                             # no replay exceeded a capacity (sticky flag + last counts)
    rank_ms = [local_ms]
    if world > 1:
        t = torch.tensor([local_ms], dtype=torch.float64, device=dev)
        allt = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        rank_ms = [float(x.item()) for x in allt]

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, W)
    if args.dump_state and rank == 0:
        import hashlib
        torch.cuda.synchronize()
        with open(args.dump_state, "w") as f:
            json.dump({"param_sha256": hashlib.sha256(flat_param.data.cpu().numpy().tobytes()).hexdigest(),
                       "grad_sha256": hashlib.sha256(bucket.flat.cpu().numpy().tobytes()).hexdigest(),
                       "grad_norm": float(opt.grad_norm.item()), "steps": args.steps, "world": world,
                       "param_sum": float(flat_param.data.double().sum().item())}, f)

    # secondary figure: the same loop with the points arriving from pinned host memory (a3 inside the step)
    h2d = None
    if not args.no_h2d:
        try:
            one_graph = use_graph and step.form == "one_graph"
            h2d_form = "copy stream"
            trial_ms = []
            pulled = bool(one_graph and os.environ.get('PCD_H2D_PULL'))
            if pulled:
                # (opt-in) the step's own graph pulls the next batch from pinned host memory (PullSource): no copy stream, no
                # events, nothing bimodal -- but the hipGraph executor runs the extra branch IN SERIES with the step (it keeps
                # two branches concurrent, and the step already has two everywhere): + 0.33 ms = the PCIe time of 15.4 MB
                src = PullSource(batches, dev)
                step.release()
                step.capture(batches[0], pull=src)
                h2d_form = "pulled by a kernel of the step's graph"
            else:
                # Which hardware queue the copy stream shares with the replayed graph's internal streams decides between
                # 3.5 and 4.2-4.8 ms per step (see H2DSource); the mapping is fixed per stream, so: try a few streams for a
                # handful of steps each and keep the best one for the timed loop
                host = None
                cands = [torch.cuda.Stream(device=dev) for _ in range(int(os.environ.get('PCD_H2D_CANDIDATES', '6')))]
                best = (None, None)
                trial_ms = []
                for st_ in cands if len(cands) > 1 else []:
                    trial = H2DSource(batches, dev, stream=st_, host=host)
                    host = trial.host
                    t_el, _ = timed_loop(8, trial)
                    trial.close()
                    trial_ms.append(round(1e3 * t_el / 8, 3))
                    if best[0] is None or t_el < best[0]:
                        best = (t_el, st_)
                src = H2DSource(batches, dev, stream=best[1], host=host)
                if trial_ms:
                    h2d_form = f"copy stream (best of {len(cands)} candidate streams, 8-step trials: {trial_ms} ms/step)"
            el, h2d_host = timed_loop(args.steps, src, pull=pulled)
            if pulled:
                step.check()
                step.release()
                step.capture(batches[0])                     # the resident form again for the loops below
                src.close = lambda: None
            if os.environ.get('PCD_BENCH_DEBUG') and src.copy_events:
                torch.cuda.synchronize()
                cms = sorted(a.elapsed_time(b) for a, b in src.copy_events)
                print(f"[bench] h2d copies on the GPU clock (15.4 MB each, beside the step): median {cms[len(cms) // 2]:.3f} ms, "
                      f"max {cms[-1]:.3f} ms", file=sys.stderr)
            if os.environ.get('PCD_BENCH_DEBUG'):
                print(f"[bench] h2d loop: host issue {1e3 * h2d_host / max(args.steps, 1):.3f} ms/step, "
                      f"wall {1e3 * el / max(args.steps, 1):.3f} ms/step", file=sys.stderr)
            src.close()
            el = cdist.max_over_ranks(el, dev)
            h2d = {"value": round(world * B * args.steps / el, 3), "unit": "frames/s",
                   "ms_per_step": round(1e3 * el / max(args.steps, 1), 4), "form": h2d_form,
                   # what a user gets WITHOUT trying streams: the first stream created (8-step trial), beside the best-of-N
                   "first_stream_ms_per_step": (trial_ms[0] if (not os.environ.get('PCD_H2D_PULL') and trial_ms) else None),
                   "worst_stream_ms_per_step": (max(trial_ms) if (not os.environ.get('PCD_H2D_PULL') and trial_ms) else None),
                   "what": "same timed loop, points of every batch arriving from PINNED HOST memory inside the step (15.4 MB "
                           "/ step / GPU) on a copy stream two batches ahead, overlapped with compute; `value` above is the "
                           "HBM-resident figure the contract asks for"}
            step.check()
        except Exception as exc:
            print(f"[bench] H2D-inclusive loop failed ({type(exc).__name__}: {exc})", file=sys.stderr)
            torch.cuda.synchronize()
    # secondary figure: frames that lost 0-20 % of their rays (every frame a different fraction): row counts vary by up
    # to 20 % from step to step under the SAME captured graph / capacities; a capacity overflow (sticky device flag)
    # re-captures with larger buffers and is counted
    ragged = None
    if not args.no_ragged:
        try:
            rb = pad_batches(make_batches(np.random.default_rng(4242 + rank)), nmax)
            rsrc = ResidentSource(rb)
            el = None
            for attempt in range(3):
                try:
                    el, _ = timed_loop(args.steps, rsrc)
                    step.check()
                    break
                except ops.L.PcdError:
                    step.recapture()
            if el is not None:
                el = cdist.max_over_ranks(el, dev)
                real = [int(o[-1].item()) for _, o in rb]
                ragged = {"value": round(world * B * args.steps / el, 3), "unit": "frames/s",
                          "ms_per_step": round(1e3 * el / max(args.steps, 1), 4),
                          "points_per_batch_min_max": [min(real), max(real)],
                          "what": "same captured step over batches whose frames lost 0-20 % of their rays (variable row "
                                  "counts under static capacities); NOT the headline workload"}
        except Exception as exc:
            print(f"[bench] ragged loop failed ({type(exc).__name__}: {exc})", file=sys.stderr)
            torch.cuda.synchronize()
    com_report = None
    if args.com:
        # COM's per-epoch exchange (train_utils.py:269-287): all_gather of the (3, 96) epoch sums -> what COMAug's sampler gets
        torch.cuda.synchronize()
        st_ = W.head_loss.hm_loss_func
        conf = cdist.gather_group_confidence(st_.epoch_confidence, st_.epoch_num)
        com_report = {"head": "CurriculumCenterHead_x5 (conf_shape (3, 96)), LOSS_CURRICULUM " + json.dumps(W.com_cur),
                      "groups_seen": int((st_.epoch_num > 0).sum().item()),
                      "objects_counted": float(st_.epoch_num.sum().item()),
                      "avg_confidence_ema": round(st_.avg_confidence, 6),
                      "confidence_groups_mean": round(float(conf[conf > 0].mean()) if (conf > 0).any() else 0.0, 6),
                      "epoch_gather": "all_gather of 2 x (3, 96) float32 over " + ("RCCL" if world > 1 else "1 rank (no process group)")}
    execution = step.describe()
    step.release()                                           # the instrumented steps below run eagerly

    if args.stage_times:
        marks = []

        def rec(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e, time.perf_counter()))

        step.eager(resident.get(0), rec)
        torch.cuda.synchronize()
        for (n0, e0, h0), (n1, e1, h1) in zip(marks[:-1], marks[1:]) if rank == 0 else []:
            print(f"[stage] {n0:10s} gpu {e0.elapsed_time(e1):8.3f} ms   host {1e3 * (h1 - h0):8.3f} ms", file=sys.stderr)

    result = {
        "metric": METRIC,
        "value": round(fps, 3), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16", "data": "synthetic",
        "rccl_ranks": dist.get_world_size() if (world > 1 and dist.is_initialized()) else 1,
        "collective_backend": (dist.get_backend() if dist.is_initialized() else None),
        "ms_per_step_ranks": [round(v, 4) for v in rank_ms],
        "config": {"workload": "CenterPoint-VoxelNet hot path (hard voxelize+MeanVFE -> VoxelResBackBone8x fwd+bwd -> "
                               "HeightCompression fwd+bwd -> grad all-reduce -> clip -> Adam), Waymo-shaped 160k-pt "
                               "synthetic clouds, 64 beams x 2500 az, grid (41,1504,1504)",
                   "frames_per_gpu": B, "global_batch": B * world, "points_per_frame": 160000,
                   "voxels_per_frame": int(step.last_voxels / B), "parallelism": f"dp{world}",
                   "optimizer": "adam_onecycle (decoupled wd 0.01, betas (OneCycle MOMS, 0.99), clip 10)",
                   "bev_layout": ("channels_last storage of spatial_features [B, C*D, H, W] (MAP_TO_BEV.CHANNELS_LAST)"
                                  if (args.dense_head or os.environ.get("PCD_BEV_NHWC", "1") != "0") else "NCHW-contiguous"),
                   "dense_head": bool(args.dense_head), "com_head": bool(args.com),
                   "distinct_batches": n_batches, "recaptures": step.recaptures,
                   "execution": execution,
                   "step_object": "com_amd.train.CapturedStep driven by com_amd.train.train_one_epoch"},
    }
    if h2d is not None:
        result["h2d_inclusive"] = h2d
    if ragged is not None:
        result["ragged"] = ragged
    if com_report is not None:
        result["com"] = com_report
    if args.config5:
        result["config"]["workload"] = ("SECOND / VoxelNet hot path (hard voxelize+MeanVFE -> VoxelBackBone8x fwd+bwd -> "
                                        "HeightCompression fwd+bwd -> clip -> Adam), fp8 (e4m3) FORWARD convs on "
                                        f"{getattr(W, 'fp8_layers', 0)} layers, bf16 backward, 300k-pt synthetic clouds "
                                        "(120 beams x 2500 az), MAX_NUMBER_OF_VOXELS 150000 per frame")
        result["config"]["points_per_frame"] = 300000
        result["dtype"] = "fp8 forward (e4m3, fp32 accumulate) / bf16 backward"
    if args.dense_head:
        result["config"]["workload"] = ("FULL CenterPoint-VoxelNet step (hot path + BaseBEVBackbone + CenterHead towers + "
                                        + ("COM curriculum head: cluster / radius_map targets / FocalLossCenterCurriculum"
                                           if args.com else "CenterHead targets / focal + L1 losses")
                                        + "), Waymo-shaped 160k-pt synthetic clouds")

    if not args.no_roofline:
        roof = measure_roofline(lambda: step.eager(resident.get(0)), ms_per_step)   # every rank runs the extra step (collectives inside)
        if rank == 0:
            result["roofline"] = roof
    if rank == 0 and world == 1 and not args.no_regime and not args.no_roofline and not args.dense_head and not args.config5 \
            and result.get("roofline"):
        torch.cuda.synchronize()
        result["roofline"]["rulebook"] = measure_regime()
    if rank == 0 and world == 1 and not args.no_seam_path and use_graph and not args.dense_head and not args.config5:
        result["seam_path"] = measure_seam_path(W, fps, dev)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        result["cpu_baseline"] = measure_cpu_baseline()
    if rank == 0 and world == 1 and not args.no_stage2 and not args.dense_head and not args.config5:
        result["stage2"] = measure_stage2(B, dev)
    if rank == 0 and world == 1 and not args.no_full_model and not args.dense_head and not args.config5:
        torch.cuda.synchronize()
        result["full_model"] = measure_full_model(args)
    if rank == 0 and world == 1 and not args.no_fp8 and not args.dense_head and not args.config5:
        # BASELINE config 5's workload (SECOND / VoxelBackBone8x, 300k-point clouds).  Its FAST path on gfx950 is bf16: the
        # non-scaled fp8 MFMA (v_mfma_f32_16x16x32_fp8_fp8) issues at the bf16 rate (MI355X_MICROARCH.md: only the MX-scaled
        # K = 128 form reaches the 5 PF fp8 peak, and a per-offset contraction over 16..64 channels cannot feed it), so e4m3
        # features buy bandwidth only -- and the bf16 window kernels already stage every row once.  `config5_300k.value` is
        # therefore the bf16 step; the fp8-forward step (parity-tested: tests/test_fp8.py, test_gpu_fp8_train.py) is kept
        # beside it as `fp8_forward_parity_path`, with the ratio -- DESIGN.md section 0 row g.
        bf = measure_full_model(args, flags=("--config5",),
                                what="child run `bench.py --config5` with bf16 forward convs: BASELINE config 5's workload as a "
                                     "TRAINING step -- SECOND's VoxelBackBone8x on 300k-point clouds, window kernels where they "
                                     "apply, batch-statistics BatchNorm; one hipGraph per step",
                                extra_env={"PCD_CONFIG5_BF16": "1"})
        result["config5_300k"] = bf
        f8 = measure_full_model(
            args, flags=("--config5",),
            what="the same child run with fp8 (e4m3, v_mfma_f32_16x16x32_fp8_fp8) FORWARD convs, static per-tensor scales, "
                 "bf16 backward")
        if isinstance(bf, dict) and isinstance(f8, dict) and "value" in f8:
            bf["fp8_forward_parity_path"] = {k: f8[k] for k in ("value", "unit", "ms_per_step", "config") if k in f8}
            if "value" in bf:
                bf["fp8_over_bf16"] = round(f8["value"] / bf["value"], 4)
    if rank == 0 and world == 1 and not args.no_n_gt_1 and not args.dense_head and not args.config5 \
            and not os.environ.get("PCD_FORCE_3GRAPH") and not os.environ.get("PCD_RCCL_WORLD1"):
        # what N > 1 GPUs run, measured on this one GPU: ONE graph for forward + backward (the next batch voxelised mid-forward),
        # the all-reduce of the flat gradient bucket, clip + Adam as plain launches -- with a real RCCL communicator of ONE
        # rank, and the same form without the collective: the difference is what the exchange step costs a rank before any
        # byte crosses xGMI
        a = measure_full_model(args, flags=(), what="N > 1 form + dist.all_reduce over a one-rank RCCL communicator",
                               extra_env={"PCD_RCCL_WORLD1": "1"})
        b = measure_full_model(args, flags=(), what="N > 1 form, no collective", extra_env={"PCD_FORCE_3GRAPH": "1"})
        # (... and the one-graph form as a child run of the same kind: the parent's own figure comes from a process that has
        #  been on the device for a minute, the children's from fresh ones -- the forms are compared child against child)
        c = measure_full_model(args, flags=(), what="one-graph form, child run", extra_env={"PCD_NO_N_GT_1": "1"})
        if "error" in a or "error" in b:
            result["n_gt_1_form"] = {"error": a.get("error") or b.get("error")}
        else:
            result["n_gt_1_form"] = {
                "ms_per_step": a["ms_per_step"], "ms_per_step_no_collective": b["ms_per_step"],
                "ms_allreduce_exposed": round(a["ms_per_step"] - b["ms_per_step"], 4),
                "ms_per_step_one_graph_child": c.get("ms_per_step"),
                "ms_over_one_graph_child": (round(a["ms_per_step"] - c["ms_per_step"], 4) if "ms_per_step" in c else None),
                "ms_per_step_one_graph": result["ms_per_step"], "bucket_MB": round(bucket.flat.numel() * 4 / 1e6, 2),
                "what": "the N > 1 execution form on ONE GPU (child runs): [forward+backward graph incl. the mid-forward "
                        "voxelisation of the next batch] | all-reduce | clip+Adam as plain launches (until round 4: voxelise-graph | "
                        "forward+backward-graph, PCD_N_GT_1_FORM=3graph); a one-rank RCCL all-reduce moves no bytes, so "
                        "ms_allreduce_exposed is the launch / synchronisation cost of the exchange step only -- the wire "
                        "time of 2 (N-1)/N x bucket over xGMI comes on top at N > 1 (DESIGN.md section 6)"}
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
    if dist.is_initialized():
        dist.destroy_process_group()
    if whole_run is not None:
        whole_run.disarm()


if __name__ == "__main__":
    main()
