"""What tests/test_gpu_backward_schedule.py and tests/golden/make_backward_schedule_trace.py share: two small models (one
sparse, one dense), and a tracer that logs every `pcd_*` entry point with the stream it was given, together with every
Event.record / wait_event / wait_stream, during one forward + backward + join_deferred_wgrad().

The fixture tests/golden/backward_schedule_trace.json holds what this module logged on the commit BEFORE the backward
schedule became one function (functional.scheduled_backward); it is never regenerated from the code under test."""
import ctypes
import hashlib
from functools import partial

import numpy as np
import torch
from torch import nn

DEV = "cuda"
# (switches of com_amd.spconv.functional; the DIRECT_GRAD settings run with pre-allocated fp32 .grad buffers)
SETTINGS = {
    "defaults": {},
    "no_overlap": {"OVERLAP_WGRAD": False},
    "direct_lag32": {"DIRECT_GRAD": True, "WGRAD_JOIN_LAG": 32},
    "direct_lag0": {"DIRECT_GRAD": True, "WGRAD_JOIN_LAG": 0},
}


def _side_stream(dev):
    from com_amd.spconv import functional as Fsp
    return (getattr(Fsp, "side_stream", None) or Fsp._side_stream)(dev)      # (the name before it became public)


class _TracedLib:
    """Stands in for the loaded library handle: every pcd_* call is logged as (name, stream tag) and passed on."""

    def __init__(self, handle, log, tag):
        self._handle, self._log, self._tag = handle, log, tag

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        if not name.startswith("pcd_"):
            return fn

        def call(*args):
            streams = [self._tag(a.value) for a in args if isinstance(a, ctypes.c_void_p) and a.value]
            hit = [t for t in streams if t != "other"]
            self._log.append([name, hit[-1] if hit else "other"])
            return fn(*args)
        return call


def traced(run, monkeypatch):
    """run() on a fresh non-default stream ("main"); returns the ordered log.  Events are numbered in the order of their
    first record."""
    from com_amd import _lib as L
    L.lib()
    log, n_events = [], [0]
    main = torch.cuda.Stream()
    side = _side_stream(torch.device(DEV, torch.cuda.current_device()))
    handles = {main.cuda_stream: "main", side.cuda_stream: "side"}
    tag = lambda h: handles.get(h, "other")
    rec, wev, wst = torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream

    def record(self, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream()
        if not hasattr(self, "_trace_no"):
            self._trace_no, n_events[0] = n_events[0], n_events[0] + 1
        log.append([f"Event.record#{self._trace_no}", tag(s.cuda_stream)])
        return rec(self, s)

    def wait_event(self, event):
        log.append([f"wait_event#{getattr(event, '_trace_no', '?')}", tag(self.cuda_stream)])
        return wev(self, event)

    def wait_stream(self, other):
        log.append([f"wait_stream<-{tag(other.cuda_stream)}", tag(self.cuda_stream)])
        return wst(self, other)

    main.wait_stream(torch.cuda.current_stream())
    with monkeypatch.context() as m:
        m.setattr(torch.cuda.Event, "record", record)
        m.setattr(torch.cuda.Stream, "wait_event", wait_event)
        m.setattr(torch.cuda.Stream, "wait_stream", wait_stream)
        m.setattr(L, "_lib", _TracedLib(L._lib, log, tag))
        with torch.cuda.stream(main):
            run()
    torch.cuda.current_stream().wait_stream(main)
    torch.cuda.synchronize()
    return log


def _sha(t):
    return hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()


def _prepare_grads(params, direct):
    for p in params:
        p.grad = torch.full_like(p, 123.0, dtype=torch.float32) if direct else None


def sparse_case():
    """SubM 5 -> 16 input conv (no dx), a SubM 16 -> 16 residual pair with BatchNorm, a 3x3x3 stride-2 conv 16 -> 32 (parity
    classes), a SubM 32 -> 32 with bias; 2 frames of 300 voxels in a 16 x 16 x 8 grid, rows z-fastest with their column map.
    Returns (named parameters, step): step() = forward + backward + join."""
    from com_amd import ops, spconv
    from com_amd.hotpath.backbone3d import SparseBasicBlock
    from com_amd.spconv import functional as Fsp
    shape, batch = [8, 16, 16], 2
    rng = np.random.default_rng(5)
    cells = np.concatenate([np.stack([np.full(300, b), *np.unravel_index(rng.choice(8 * 16 * 16, 300, replace=False), shape)], 1)
                            for b in range(batch)]).astype(np.int32)
    idx = np.ascontiguousarray(cells[np.lexsort((cells[:, 1], cells[:, 3], cells[:, 2], cells[:, 0]))])
    idx_t = torch.from_numpy(idx).to(DEV)
    g = torch.Generator().manual_seed(11)
    feats = torch.randn((idx.shape[0], 5), generator=g).to(DEV).bfloat16()
    norm = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
    torch.manual_seed(12)
    net = spconv.SparseSequential(
        spconv.SubMConv3d(5, 16, 3, padding=1, bias=False, indice_key="subm1"), norm(16), nn.ReLU(),
        SparseBasicBlock(16, 16, norm_fn=norm, indice_key="res1"),
        spconv.SparseConv3d(16, 32, 3, stride=2, padding=1, bias=False, indice_key="spconv2"), norm(32), nn.ReLU(),
        spconv.SubMConv3d(32, 32, 3, padding=1, bias=True, indice_key="subm2")).to(DEV)
    cmap = ops.colmap_from_rows(idx_t, batch, shape)
    gout = None

    def step():
        nonlocal gout
        x = spconv.SparseConvTensor(feats, idx_t, shape, batch)
        x.chain.row_order = ops.ROWS_YXZ
        x.chain.add_rank(cmap)
        y = net(x).features
        if gout is None:
            gout = torch.randn(y.shape, generator=torch.Generator().manual_seed(13)).to(DEV).to(y.dtype)
        y.backward(gout)
        Fsp.join_deferred_wgrad()

    return dict(net.named_parameters()), step


def dense_case():
    """Conv3x3 32 -> 32 + BatchNormReLU2d, Conv3x3S2 32 -> 64, UpConvT 64 -> 32, and the two-branch _BranchConvsFunction
    (64 -> 2 and 64 -> 3, bias) on the two copies of the stride-2 map; B = 1, H = W = 16."""
    from com_amd.hotpath import conv2d_fast as C
    from com_amd.spconv import functional as Fsp
    torch.manual_seed(21)
    net = nn.ModuleDict(dict(
        conv=C.Conv3x3(32, 32, 3, padding=1, bias=False), bn=C.BatchNormReLU2d(32, eps=1e-3, momentum=0.01, relu=True),
        down=C.Conv3x3S2(32, 64, 3, stride=2, padding=1, bias=False), up=C.UpConvT(64, 32, 2, stride=2, bias=False),
        b0=C.Conv3x3(64, 2, 3, padding=1, bias=True), b1=C.Conv3x3(64, 3, 3, padding=1, bias=True))).to(DEV)
    net["conv"].bn_follows = True
    g = torch.Generator().manual_seed(22)
    rand = lambda *s: torch.randn(s, generator=g).to(DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    x0, g_up, g0, g1 = rand(1, 32, 16, 16), rand(1, 32, 16, 16), rand(1, 2, 8, 8), rand(1, 3, 8, 8)

    def step():
        x = x0.clone().requires_grad_(True)
        mid = net["down"](net["bn"](net["conv"](x)))
        up = net["up"](mid)
        a = torch.cat([mid, mid], 1)
        o0, o1 = C._BranchConvsFunction.apply(a, 64, [(None, None), (None, None)], net["b0"].weight, net["b0"].bias,
                                              net["b1"].weight, net["b1"].bias)
        torch.autograd.backward([up, o0, o1], [g_up, g0, g1])
        Fsp.join_deferred_wgrad()

    return dict(net.named_parameters()), step


CASES = {"sparse": sparse_case, "dense": dense_case}


def record(case, setting, monkeypatch):
    """{"log": [[name, stream], ...], "grads": {parameter: sha256}} of one case under one switch setting."""
    from com_amd.spconv import functional as Fsp
    params, step = CASES[case]()
    switches = {"OVERLAP_WGRAD": True, "DIRECT_GRAD": False, "WGRAD_JOIN_LAG": 0, **SETTINGS[setting]}
    with monkeypatch.context() as m:
        for k, v in switches.items():
            m.setattr(Fsp, k, v)
        Fsp.reset_deferred()
        _prepare_grads(params.values(), switches["DIRECT_GRAD"])
        step()                                   # (first use: plans, pair lists and caches are built outside the log)
        _prepare_grads(params.values(), switches["DIRECT_GRAD"])
        log = traced(step, monkeypatch)
    return {"log": log, "grads": {n: _sha(p.grad) for n, p in params.items()}}
