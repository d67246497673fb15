"""The one backward schedule of the sparse and dense convs (com_amd.spconv.functional.scheduled_backward) without a device:
streams, events and the side stream are small recording fakes, the three callbacks are stubs that log where they ran and
return CPU tensors.  Every case asserts the exact ordered log -- WHEN and WHERE each piece is issued is what the captured
step's speed depends on ("The backward schedule")."""
import contextlib

import pytest
import torch

from com_amd import ops
from com_amd.spconv import functional as F

SPARSE = dict(direct_without_deferral=True, flush=True, sparse_stamps=True)     # what SparseConvFunction.backward passes
DENSE = {}                                                                      # what hotpath.conv2d_fast passes


class _Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_event(self, ev):
        self.log.append(("wait_event", self.name, ev.name))

    def wait_stream(self, other):
        self.log.append(("wait_stream", self.name, other.name))


class _Sched:
    """The fakes + the stub callbacks of one test; `log` is the ordered record."""

    def __init__(self, monkeypatch):
        self.log = log = []
        self.main, self.side = _Stream("main", log), _Stream("side", log)
        self.cur = self.main
        self.events = 0
        self.job_bytes = 0          # > 0: a deferred wgrad stub queues a slab job of this many bytes (and bsum a colsum job)
        sched = self

        class Event:
            def __init__(self, *a, **k):
                sched.events += 1
                self.name = f"e{sched.events}"

            def record(self, stream=None):
                log.append(("record", self.name, (stream or sched.cur).name))

        @contextlib.contextmanager
        def stream(s):
            prev, sched.cur = sched.cur, s
            try:
                yield
            finally:
                sched.cur = prev

        monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: sched.cur)
        monkeypatch.setattr(torch.cuda, "Event", Event)
        monkeypatch.setattr(torch.cuda, "stream", stream)
        monkeypatch.setattr(F, "side_stream", lambda device, role="wgrad": self.side)
        monkeypatch.setattr(ops, "wgrad_reduce_batched",
                            lambda jobs: log.append(("wgrad_reduce_batched", sched.cur.name, len(jobs))))
        monkeypatch.setattr(ops, "col_sum_finalize_batched",
                            lambda jobs: log.append(("col_sum_finalize_batched", sched.cur.name, len(jobs))))
        for name, value in dict(OVERLAP_WGRAD=True, WGRAD_JOIN_LAG=0, DIRECT_GRAD=False,
                                WGRAD_FLUSH_BYTES=32 << 20).items():
            monkeypatch.setattr(F, name, value)
        self.set = lambda **kw: [monkeypatch.setattr(F, k, v) for k, v in kw.items()]

    def grad(self, tag):
        t = torch.zeros(2)
        t.record_stream = lambda s: self.log.append(("record_stream", tag, s.name))
        return t

    def dgrad(self):
        self.log.append(("dgrad", self.cur.name))
        return self.grad("dx")

    def wgrad(self, direct, jobs):
        self.log.append(("wgrad", self.cur.name, direct, jobs is not None))
        if jobs is not None and self.job_bytes:
            jobs.append(ops.WgradJob(torch.empty(self.job_bytes, dtype=torch.uint8), torch.zeros(1), 1, 1, 1, 0))
        return None if direct else self.grad("dw")

    def bsum(self, direct, jobs):
        self.log.append(("bsum", self.cur.name, direct, jobs is not None))
        if jobs is not None and self.job_bytes:
            jobs.append((torch.zeros(1, 2), 1, torch.zeros(2)))
        return None if direct else self.grad("db")

    def run(self, need_dx=True, wp=None, bp=None, wgrad=None, bsum=None, **mode):
        """One conv backward wanting dx (unless need_dx=False), dw and db; returns this call's slice of the log."""
        start = len(self.log)
        keep = [torch.zeros(1), torch.zeros(1)]
        out = F.scheduled_backward(need_dx, True, True, wp, bp, self.dgrad, wgrad or self.wgrad, bsum or self.bsum, keep,
                                   **mode)
        return out, self.log[start:]


_ALIVE = []     # the parameters of one test: claims go by id(), which a freed parameter would hand to the next one


@pytest.fixture
def sched(monkeypatch):
    F.reset_deferred()
    yield _Sched(monkeypatch)
    F.reset_deferred()
    _ALIVE.clear()


def _param(dtype=torch.float32, grad=True):
    p = torch.nn.Parameter(torch.zeros(4, dtype=dtype))
    if grad:
        p.grad = torch.zeros(4, dtype=dtype)
    _ALIVE.append(p)
    return p


def _eager(ready="e1", direct=False, joined=("dw", "db")):
    """Case A: fork from an event recorded before dgrad, both callbacks on the side stream, eager join."""
    return [("record", ready, "main"), ("dgrad", "main"), ("wait_event", "side", ready),
            ("wgrad", "side", direct, False), ("bsum", "side", direct, False), ("wait_stream", "main", "side")] \
        + [("record_stream", tag, "main") for tag in joined]


@pytest.mark.parametrize("mode", [SPARSE, DENSE], ids=["sparse", "dense"])
def test_a_eager_overlap(sched, mode):
    (dx, dw, db), log = sched.run(**mode)
    assert log == _eager() and dx is not None and dw is not None and db is not None
    assert not F._PENDING


def test_a_list_valued_gradients_are_each_recorded_on_the_main_stream(sched):
    """The branch convs return lists of gradients (None for a dead branch)."""
    def wgrad(direct, jobs):
        sched.log.append(("wgrad", sched.cur.name, direct, jobs is not None))
        return [sched.grad("dw0"), None, sched.grad("dw2")]

    _, log = sched.run(wgrad=wgrad)
    assert log == _eager(joined=("dw0", "dw2", "db"))


@pytest.mark.parametrize("mode", [SPARSE, DENSE], ids=["sparse", "dense"])
def test_b_without_overlap_everything_runs_on_the_main_stream(sched, mode):
    sched.set(OVERLAP_WGRAD=False, DIRECT_GRAD=True, WGRAD_JOIN_LAG=2)       # (no side stream: never deferred either)
    _, log = sched.run(wp=_param(grad=False), bp=_param(grad=False), **mode)
    assert log == [("dgrad", "main"), ("wgrad", "main", False, False), ("bsum", "main", False, False)]


@pytest.mark.parametrize("mode", [SPARSE, DENSE], ids=["sparse", "dense"])
def test_c_no_input_gradient_no_fork(sched, mode):
    (dx, _, _), log = sched.run(need_dx=False, **mode)
    assert dx is None and log == [("wgrad", "main", False, False), ("bsum", "main", False, False)]


@pytest.mark.parametrize("mode", [SPARSE, DENSE], ids=["sparse", "dense"])
@pytest.mark.parametrize("queue_jobs", [True, False])
def test_d_deferred_and_lagged(sched, mode, queue_jobs):
    sched.set(DIRECT_GRAD=True, WGRAD_JOIN_LAG=2)
    sched.job_bytes = 16 if queue_jobs else 0
    for i in range(4):
        ready, ev = f"e{2 * i + 1}", f"e{2 * i + 2}"
        (dx, dw, db), log = sched.run(wp=_param(), bp=_param(), **mode)
        want = [("record", ready, "main"), ("dgrad", "main"), ("wait_event", "side", ready),
                ("wgrad", "side", True, True), ("bsum", "side", True, True), ("record", ev, "side")]
        if i >= 2:                                   # layer i - 2's side work is joined now: e2 in call 3, e4 in call 4
            want.append(("wait_event", "main", f"e{2 * (i - 2) + 2}"))
        assert log == want and dx is not None and dw is None and db is None
        assert len(F._PENDING) <= 2
    start = len(sched.log)
    F.join_deferred_wgrad()
    if queue_jobs:
        assert sched.log[start:] == [("wgrad_reduce_batched", "side", 4), ("col_sum_finalize_batched", "side", 4),
                                     ("record", "e9", "side"), ("wait_event", "main", "e9")]
    else:
        assert sched.log[start:] == [("wait_event", "main", "e8")]           # the last pending event only
    assert not (F._PENDING or F._WGRAD_JOBS or F._COLSUM_JOBS or F._WGRAD_KEEP or F._DIRECT_WRITTEN)


def test_d_the_keep_list_a_callback_extended_stays_pending(sched):
    sched.set(DIRECT_GRAD=True, WGRAD_JOIN_LAG=2)
    partial = torch.zeros(3)
    keep = [torch.zeros(1)]

    def bsum(direct, jobs):
        keep.append(partial)                         # the sparse bias path: the BatchNorm partial it consumed

    F.scheduled_backward(True, True, True, _param(), _param(), sched.dgrad, sched.wgrad, bsum, keep, **SPARSE)
    assert F._PENDING[-1][1][-1] is partial


def test_e_direct_without_deferral_sparse_claims_the_parameter(sched):
    sched.set(DIRECT_GRAD=True)
    wp, bp = _param(), _param()
    (_, dw, db), log = sched.run(wp=wp, bp=bp, **SPARSE)
    assert log == _eager(direct=True, joined=())
    assert dw is None and db is None
    with pytest.raises(RuntimeError, match="second gradient contribution"):
        sched.run(wp=wp, bp=_param(), **SPARSE)
    F.join_deferred_wgrad()
    sched.run(wp=wp, bp=bp, **SPARSE)                # accepted again after the join


def test_e_direct_without_deferral_dense_stays_indirect(sched):
    sched.set(DIRECT_GRAD=True)
    wp, bp = _param(), _param()
    for ready in ("e1", "e2"):                       # twice: nothing is claimed
        _, log = sched.run(wp=wp, bp=bp, **DENSE)
        assert log == _eager(ready)
        assert not F._DIRECT_WRITTEN


@pytest.mark.parametrize("mode", [SPARSE, DENSE], ids=["sparse", "dense"])
@pytest.mark.parametrize("dtype", [None, torch.float16], ids=["no-grad", "fp16-grad"])
def test_f_unusable_grad_is_neither_direct_nor_deferred(sched, mode, dtype):
    sched.set(DIRECT_GRAD=True, WGRAD_JOIN_LAG=2)
    wp, bp = (_param(grad=False), _param(grad=False)) if dtype is None else (_param(dtype), _param(dtype))
    _, log = sched.run(wp=wp, bp=bp, **mode)
    assert log == _eager()
    assert not (F._PENDING or F._DIRECT_WRITTEN)


@pytest.mark.parametrize("mode,limit,flushes", [(SPARSE, 64, True), (DENSE, 64, False), (SPARSE, 0, False),
                                                (DENSE, 0, False)], ids=["sparse", "dense", "sparse-0", "dense-0"])
def test_g_flush(sched, mode, limit, flushes):
    sched.set(DIRECT_GRAD=True, WGRAD_JOIN_LAG=8, WGRAD_FLUSH_BYTES=limit)
    sched.job_bytes = 32
    _, log = sched.run(wp=_param(), bp=_param(), **mode)                     # 32 bytes queued: below the limit
    assert not any(e[0] == "wgrad_reduce_batched" for e in log) and len(F._WGRAD_JOBS) == 1
    _, log = sched.run(wp=_param(), bp=_param(), **mode)                     # 64 bytes: the sparse caller flushes
    if flushes:
        assert log[3:] == [("wgrad", "side", True, True), ("bsum", "side", True, True),
                           ("wgrad_reduce_batched", "side", 2), ("record", "e4", "side")]
        assert not F._WGRAD_JOBS and len(F._WGRAD_KEEP) == 2
    else:
        assert log[3:] == [("wgrad", "side", True, True), ("bsum", "side", True, True), ("record", "e4", "side")]
        assert len(F._WGRAD_JOBS) == 2 and not F._WGRAD_KEEP
    assert len(F._COLSUM_JOBS) == 2


def test_h_reset_deferred_drops_everything_without_a_launch(sched):
    sched.set(DIRECT_GRAD=True, WGRAD_JOIN_LAG=8, WGRAD_FLUSH_BYTES=16)
    sched.job_bytes = 16
    sched.run(wp=_param(), bp=_param(), **SPARSE)    # flushed: one kept job, one colsum job, one pending entry, two claims
    sched.run(wp=_param(), bp=_param(), **DENSE)
    assert F._PENDING and F._COLSUM_JOBS and F._WGRAD_KEEP and F._WGRAD_JOBS and F._DIRECT_WRITTEN
    start = len(sched.log)
    F.reset_deferred()
    assert sched.log[start:] == []
    assert not (F._PENDING or F._WGRAD_JOBS or F._COLSUM_JOBS or F._WGRAD_KEEP or F._DIRECT_WRITTEN)
