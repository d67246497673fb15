"""com_amd/csrc/fused.hip (fused BatchNorm1d (+ residual) (+ ReLU) forward / backward, pcd_col_sum, pcd_col_sum_finalize) against
the fp64 reference tests/bn_ref.py, PER ELEMENT, with bounds derived from the arithmetic (class Bounds) and no element excused.

The reference follows the kernel's contract: inputs are values already rounded to the kernel's dtype, the ReLU mask of the
backward is `y_stored > 0` of the output the kernel itself stored, and the backward is evaluated with the statistics the kernel
saved (their error is judged once, in the forward).  The library is built with -ffp-contract=off, so a product and the sum it feeds
are two roundings; u = 2^-24 below.

Sizes are the smallest that reach each path of fused.hip: the reduction passes always run MAX_BLOCKS = 512 workgroups of up to 256
threads over 16-byte pieces (8 bf16 / 4 f32), so bn_stats_kernel's 4-way loop needs more than 3 * 131072 pieces and
bn_bwd_reduce_kernel's 2-way loop more than 131072; the apply passes give a thread BN_PPT = 4 pieces until their grid reaches
MAX_APPLY_BLOCKS = 2048 (past 2048 * 256 * 4 pieces).

Every judged quantity prints error / bound; the worst ratio per quantity over the module is printed when the module ends (-s)."""
import numpy as np
import pytest
import torch

from tests import bn_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
EPS = float(np.float32(1e-3))           # the kernels take eps / momentum as C floats
MOMENTUM = float(np.float32(0.01))
ROWS = (1, 2, 3, 255, 256, 257, 4099)
WORST = {}                              # quantity -> (error / bound, where)


def _ops():
    from com_amd import ops
    return ops


def _L():
    from com_amd import _lib
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    print("\nworst error / bound per quantity (test_gpu_fused_bn.py):")
    for name in sorted(WORST):
        print(f"  {name:<16s} {WORST[name][0]:.4f}   at {WORST[name][1]}")


def _judge(name, where, got, ref, bound):
    """|got - ref| <= bound on EVERY element (fp64 CPU tensors); the worst ratio is printed and recorded."""
    got, ref = got.detach().cpu().double(), ref.double()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    assert got.shape == ref.shape, (name, where, got.shape, ref.shape)
    if ref.numel() == 0:
        return
    assert torch.isfinite(got).all(), f"{name} at {where}: not finite"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)      # (a zero bound allows a zero error only)
    worst = float(ratio.max())
    if worst > WORST.get(name, (-1.0, ""))[0]:
        WORST[name] = (worst, where)
    print(f"{name:<16s} {where}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.4f}")
    assert worst <= 1.0, f"{name} at {where}: error / bound = {worst:.4f}"


class Bounds:
    """Every tolerance of this module.  SUM = 16 u = 2^-20 relative to the sum of the absolute values of the terms: a reduction adds
    a handful of fp32 terms per thread (4 or fewer pieces up to 4099 rows of 1024 channels; 12 and 16 at the 12289- and 16385-row
    cases), then a fixed tree of at most 10 more fp32 additions, the rest is double -- roughly 12 roundings, 16 granted.  (The
    worst case of the two largest shapes is above 16 u, but roundings do not all point one way: the largest ratio measured over
    the module is 0.19, for a dgamma at n = 3.)  ELEM = 8 u = 2^-21 relative to the sum of the
    absolute values of the terms of a per-element expression: the longest chain (the xhat * dgamma / n term of dx: xhat 2, dgamma / n
    2, their product 1, the subtraction 1, gamma * invstd 1, the last product 1) is 8 roundings."""
    SUM = 2.0 ** -20
    ELEM = 2.0 ** -21
    HALF_BF16 = 2.0 ** -8               # half a bf16 ulp relative to the value: the one rounding of a stored bf16

    @staticmethod
    def mean(xd):
        return Bounds.SUM * xd.abs().mean(0) if xd.shape[0] else torch.zeros(xd.shape[1], dtype=torch.float64)

    @staticmethod
    def var(xd):
        # E[x^2] carries SUM * mean(x^2); mean^2 twice the relative error of the mean, and mean(|x|)^2 <= mean(x^2)
        return Bounds.SUM * 3 * xd.square().mean(0) if xd.shape[0] else torch.zeros(xd.shape[1], dtype=torch.float64)

    @staticmethod
    def invstd(var_bound, invstd_ref, roundings=2):
        # d invstd / d var = -invstd^3 / 2; the double -> float conversion and its own sqrt / divide: 2 u relative
        return 0.5 * invstd_ref ** 3 * var_bound + roundings * U * invstd_ref

    @staticmethod
    def running(momentum, stat_bound, old, stat_ref):
        # (1 - m) * old + m * stat in fp32: one rounding per product, one for the sum
        return momentum * stat_bound + 2 * U * (((1.0 - momentum) * old).abs() + (momentum * stat_ref).abs())

    @staticmethod
    def output(xd, resd, gamma, beta, mean_ref, invstd_ref, mean_bound, invstd_bound, y_ref, dtype):
        scale = gamma * invstd_ref
        a = (xd * scale).abs() + (mean_ref * scale).abs() + beta.abs()
        if resd is not None:
            a = a + resd.abs()
        delta = Bounds.ELEM * a + gamma.abs() * ((xd - mean_ref).abs() * invstd_bound + invstd_ref * mean_bound)
        return delta + (Bounds.HALF_BF16 * y_ref.abs() if dtype == BF16 else 0.0), delta

    @staticmethod
    def dbeta(b):
        return Bounds.SUM * b.dz.abs().sum(0)

    @staticmethod
    def dgamma(b):
        return Bounds.SUM * (b.dz * b.xhat).abs().sum(0)

    @staticmethod
    def dx(b, gamma, invstd, training, n, dtype):
        gi = (gamma * invstd).abs()
        if training:
            inv_n = 1.0 / n if n else 0.0
            terms = gi * (b.dz.abs() + b.dbeta.abs() * inv_n + (b.xhat * b.dgamma).abs() * inv_n)
            carried = gi * inv_n * (Bounds.dbeta(b) + b.xhat.abs() * Bounds.dgamma(b))
        else:
            terms, carried = gi * b.dz.abs(), 0.0
        return Bounds.ELEM * terms + carried + (Bounds.HALF_BF16 * b.dx.abs() if dtype == BF16 else 0.0)


# ---------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a).cpu(), _bits(b).cpu()), f"{what}: stored bits differ"


SENTINEL = {BF16: 0x7B7B, F32: 0x7B7B7B7B}


def _sentinel(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    _bits(t).fill_(SENTINEL[dtype])
    return t


def _is_sentinel(t):
    return bool((_bits(t) == SENTINEL[t.dtype]).all())


def _inputs(n, c, dtype, seed, mean=0.3, std=1.7):
    """The distribution of the existing BatchNorm tests, rounded to the dtype (CPU tensors of that dtype; parameters f32)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c, generator=g) * std + mean).to(dtype)
    res = torch.randn(n, c, generator=g).to(dtype)
    dy = torch.randn(n, c, generator=g).to(dtype)
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g) * 0.3
    return x, res, dy, gamma, beta


def _padded(t, n, cap, fill=float("nan")):
    """[cap, c] device tensor: rows [0, n) of t, the tail poisoned."""
    out = torch.full((cap, t.shape[1]), fill, dtype=t.dtype, device=DEV)
    out[:n] = t[:n].to(DEV)
    return out


def _fresh_running(c):
    return torch.zeros(c, device=DEV), torch.ones(c, device=DEV)


def _forward(x, res, gamma, beta, training, rm, rv, relu, n_dev=None, out=None):
    return _ops().bn_forward(x, res, gamma, beta, EPS, MOMENTUM, training, rm, rv, relu, n_dev=n_dev, out=out)


def _raw_forward(x, res, gamma, beta, training, rm, rv, relu, y, y_ld, sm, si, n, c, n_dev=None):
    """pcd_bn_forward_ld with every buffer the caller's; returns the status code."""
    L = _L()
    lib = L.lib()
    ws = L.workspace(lib.pcd_bn_workspace_bytes(c), x.device)
    return lib.pcd_bn_forward_ld(L.ptr(x), L.ptr(res), L.dtype_code(x), n, c, L.ptr(gamma), L.ptr(beta), EPS, MOMENTUM,
                                 int(training), L.ptr(rm), L.ptr(rv), int(relu), L.ptr(y), int(y_ld), L.ptr(sm), L.ptr(si),
                                 L.ptr(n_dev), None, 0, L.ptr(ws), ws.numel(), L.stream_ptr())


def _raw_backward(dy, x, y, gamma, beta, sm, si, relu, training, dx, dres, dgamma, dbeta, n, c, n_dev=None):
    """pcd_bn_backward_ld with dx / dresidual buffers of the caller's (ops.bn_backward allocates its own)."""
    L = _L()
    lib = L.lib()
    ws = L.workspace(lib.pcd_bn_workspace_bytes(c), x.device)
    return lib.pcd_bn_backward_ld(L.ptr(dy), c, L.ptr(x), L.ptr(y), L.dtype_code(x), n, c, L.ptr(gamma), L.ptr(beta), L.ptr(sm),
                                  L.ptr(si), int(relu), int(training), L.ptr(dx), L.ptr(dres), L.ptr(dgamma), L.ptr(dbeta),
                                  L.ptr(n_dev), None, 0, None, L.ptr(ws), ws.numel(), L.stream_ptr())


def _check_forward(where, dtype, x, res, gamma, beta, relu, n, y, sm, si, rm0, rv0, rm1, rv1, training=True):
    """Every quantity the forward returns, against the reference on the first n rows of the CPU tensors x / res.  Returns
    (reference, delta): delta is the bound of the pre-activation BEFORE the output rounding."""
    ref = bn_ref.forward(x, res, gamma, beta, EPS, MOMENTUM, training, rm0, rv0, relu, n=n)
    xd = x[:n].double()
    resd = res[:n].double() if res is not None else None
    if training:
        mean_b, var_b = Bounds.mean(xd), Bounds.var(xd)
        invstd_b = Bounds.invstd(var_b, ref.invstd)
        _judge("mean", where, sm, ref.mean, mean_b)
        _judge("invstd", where, si, ref.invstd, invstd_b)
        unbias = n / (n - 1) if n > 1 else 1.0
        _judge("running_mean", where, rm1, ref.running_mean, Bounds.running(MOMENTUM, mean_b, rm0.cpu().double(), ref.mean))
        _judge("running_var", where, rv1, ref.running_var,
               Bounds.running(MOMENTUM, var_b * unbias, rv0.cpu().double(), ref.var * unbias))
    else:
        # eval: invstd = 1 / sqrtf(running_var + eps) in fp32: the sum, the root and the quotient round once each
        mean_b, invstd_b = torch.zeros_like(ref.mean), Bounds.invstd(0.0, ref.invstd, roundings=3)
        assert torch.equal(rm1.cpu(), rm0.cpu()) and torch.equal(rv1.cpu(), rv0.cpu()), "eval mode moved the running statistics"
    bound, delta = Bounds.output(xd, resd, gamma.double(), beta.double(), ref.mean, ref.invstd, mean_b, invstd_b, ref.y, dtype)
    _judge(f"y {_id(dtype)}", where, y[:n], ref.y, bound)
    return ref, delta


def _check_backward(where, dtype, dy, x, y_stored, gamma, sm, si, training, n, dx, dres, dgamma, dbeta):
    """y_stored: the kernel's own forward output (None: no ReLU).  dres None: not asked for."""
    mask = (y_stored.cpu().float() > 0) if y_stored is not None else None
    b = bn_ref.backward(dy, x, mask, gamma, sm, si, training, n=n)
    _judge("dbeta", where, dbeta, b.dbeta, Bounds.dbeta(b))
    _judge("dgamma", where, dgamma, b.dgamma, Bounds.dgamma(b))
    if dres is not None:
        _same_bits(dres[:n].cpu(), b.dresidual.to(dtype), f"dresidual at {where}")     # dy or 0: exact in the dtype
    _judge(f"dx {_id(dtype)}", where, dx[:n], b.dx, Bounds.dx(b, gamma.double(), si.cpu().double(), training, n, dtype))
    return b


# --------------------------------------------------------------------------------------------- 1. shape matrix
MATRIX = [(BF16, c, n) for c in (8, 16, 40, 96, 128, 320, 1024) for n in ROWS] + \
         [(F32, c, n) for c in (4, 12, 64, 1024) for n in ROWS] + \
         [(BF16, 1024, 3073), (BF16, 1024, 12289),   # 393344 / 1572992 pieces: the 4-way / 2-way reduction loops with a tail
          (BF16, 1024, 16385), (BF16, 128, 24577)]   # past 2048 * 256 * 4 pieces: the apply grid at its cap
ALL_VARIANTS = [(relu, res, dres) for relu in (True, False) for res in (True, False) for dres in (True, False)]
LARGE_VARIANTS = [(True, True, True), (True, False, False)]


def _id(v):
    return {BF16: "bf16", F32: "f32"}.get(v, str(v))


@pytest.mark.parametrize("dtype,c,n", MATRIX, ids=lambda v: _id(v))
def test_training_forward_and_backward_over_the_shape_matrix(dtype, c, n):
    ops = _ops()
    x, res, dy, gamma, beta = _inputs(n, c, dtype, 100003 * c + n)
    xg, rg, dyg, gg, bg = (t.to(DEV) for t in (x, res, dy, gamma, beta))
    for relu, with_res, want_dres in (ALL_VARIANTS if n * c <= 4099 * 1024 else LARGE_VARIANTS):
        where = f"{_id(dtype)} c={c} n={n} relu={int(relu)} res={int(with_res)} dres={int(want_dres)}"
        rm, rv = _fresh_running(c)
        rm0, rv0 = rm.clone(), rv.clone()
        y, sm, si = _forward(xg, rg if with_res else None, gg, bg, True, rm, rv, relu)
        _check_forward(where, dtype, x, res if with_res else None, gamma, beta, relu, n, y, sm, si, rm0, rv0, rm, rv)
        # the production choice of the mask source (FusedBNFunction): recomputed from x when no residual was added
        from_x = relu and not with_res
        y_arg = None if (from_x or not relu) else y
        dx, dres, dgamma, dbeta = ops.bn_backward(dyg, xg, y_arg, gg, sm, si, relu, True, want_dres,
                                                  beta=bg if from_x else None)
        assert (dres is not None) == want_dres
        _check_backward(where, dtype, dy, x, y if relu else None, gamma, sm, si, True, n, dx, dres, dgamma, dbeta)


# --------------------------------------------------------------------------------------------- 2. n = 0, static shapes
@pytest.mark.parametrize("dtype,c", [(BF16, 16), (F32, 64)], ids=lambda v: _id(v))
def test_no_rows_from_the_host(dtype, c):
    """n = 0 as a host argument: PCD_OK, zero parameter gradients, the statistics of an empty batch, nothing launched that fails."""
    ops = _ops()
    e = torch.empty(0, c, dtype=dtype, device=DEV)
    _, _, _, gamma, beta = _inputs(1, c, dtype, 7)
    gg, bg = gamma.to(DEV), beta.to(DEV)
    rm, rv = _fresh_running(c)
    y, sm, si = _forward(e, e.clone(), gg, bg, True, rm, rv, True)
    assert y.shape == (0, c)
    ref = bn_ref.forward(e, None, gamma, beta, EPS, MOMENTUM, True, torch.zeros(c), torch.ones(c), True)
    assert not sm.cpu().any()
    _judge("invstd", f"{_id(dtype)} c={c} n=0", si, ref.invstd, Bounds.invstd(0.0, ref.invstd))
    _judge("running_var", f"{_id(dtype)} c={c} n=0", rv, ref.running_var, 2 * U * ref.running_var)
    assert not rm.cpu().any()
    dgo, dbo = torch.full((c,), 7.0, device=DEV), torch.full((c,), 7.0, device=DEV)
    dx, dres, dgamma, dbeta = ops.bn_backward(e, e, e, gg, sm, si, True, True, True, dgamma_out=dgo, dbeta_out=dbo)
    torch.cuda.synchronize()
    assert dx.shape == (0, c) and dres.shape == (0, c)
    assert dgamma.data_ptr() == dgo.data_ptr() and not dgamma.cpu().any() and not dbeta.cpu().any()


@pytest.mark.parametrize("n", [0, 1, 257, 4099])
@pytest.mark.parametrize("dtype,c", [(BF16, 16), (BF16, 96), (BF16, 128), (F32, 64)], ids=lambda v: _id(v))
def test_device_side_row_count_below_the_capacity(dtype, c, n):
    """What CapturedStep runs: buffers of a fixed capacity, the row count in a device int32, a poisoned tail (n_dev = 0 is an empty
    frame).  Rows [0, n) of every output and all statistics are BIT-identical to the exact-size call (the reduction grids do not
    depend on the capacity: comment above grid_for), the rows past n are not written, and 1 / n is taken from n."""
    ops = _ops()
    cap = n + n // 4 + 3
    x, res, dy, gamma, beta = _inputs(cap, c, dtype, 31 * c + n)
    gg, bg = gamma.to(DEV), beta.to(DEV)
    n_dev = torch.tensor([n], dtype=torch.int32, device=DEV)
    for with_res in (True, False):
        where = f"{_id(dtype)} c={c} n_dev={n} cap={cap} res={int(with_res)}"
        # exact size
        xe, re_, dye = (t[:n].contiguous().to(DEV) for t in (x, res, dy))
        rme, rve = _fresh_running(c)
        ye, sme, sie = _forward(xe, re_ if with_res else None, gg, bg, True, rme, rve, True)
        dxe, drese, dge, dbe = ops.bn_backward(dye, xe, ye if with_res else None, gg, sme, sie, True, True, with_res,
                                               beta=None if with_res else bg)
        # capacity buffers
        xs, rs, dys = (_padded(t, n, cap) for t in (x, res, dy))
        ys = _sentinel((cap, c), dtype)
        rms, rvs = _fresh_running(c)
        y2, sms, sis = _forward(xs, rs if with_res else None, gg, bg, True, rms, rvs, True, n_dev=n_dev, out=ys)
        assert y2.data_ptr() == ys.data_ptr()
        y_saved = ys.clone()
        y_saved[n:] = float("nan")
        dxs, dress = _sentinel((cap, c), dtype), _sentinel((cap, c), dtype)
        dgs, dbs = torch.full((c,), 7.0, device=DEV), torch.full((c,), 7.0, device=DEV)
        code = _raw_backward(dys, xs, y_saved if with_res else None, gg, None if with_res else bg, sms, sis, True, True, dxs,
                             dress if with_res else None, dgs, dbs, cap, c, n_dev=n_dev)
        assert code == 0, code
        torch.cuda.synchronize()
        for name, a, b in (("save_mean", sms, sme), ("save_invstd", sis, sie), ("running_mean", rms, rme),
                           ("running_var", rvs, rve), ("dgamma", dgs, dge), ("dbeta", dbs, dbe)):
            assert torch.isfinite(a).all(), (name, where)
            _same_bits(a, b, f"{name} at {where}")
        _same_bits(ys[:n], ye, f"y at {where}")
        _same_bits(dxs[:n], dxe, f"dx at {where}")
        assert _is_sentinel(ys[n:]) and _is_sentinel(dxs[n:]), f"rows past n_dev were written at {where}"
        if with_res:
            _same_bits(dress[:n], drese, f"dresidual at {where}")
            assert _is_sentinel(dress[n:]), f"dresidual rows past n_dev were written at {where}"
        # ... and against the reference with n rows (running_var by n / (n - 1) of n, never of the capacity)
        _check_forward(where, dtype, x, res if with_res else None, gamma, beta, True, n, ys, sms, sis,
                       torch.zeros(c), torch.ones(c), rms, rvs)
        _check_backward(where, dtype, dy, x, ys[:n], gamma, sms, sis, True, n, dxs, dress if with_res else None, dgs, dbs)
        if n == 0:
            assert not sms.cpu().any() and not dgs.cpu().any() and not dbs.cpu().any()
            assert float((sis.cpu().double() - 1.0 / EPS ** 0.5).abs().max()) <= 2 * U / EPS ** 0.5


# --------------------------------------------------------------------------------------------- 3. column blocks
@pytest.mark.parametrize("static", [False, True], ids=["host_n", "n_dev"])
@pytest.mark.parametrize("c", [64, 96])
def test_output_and_gradient_as_column_blocks_of_wider_matrices(c, static):
    """y written into columns [c, 2c) of a [rows, 3c] matrix (y_ld = 3c) and dy read from the same block of a wider gradient
    (dy_ld = 3c): values against the reference, bits equal to the contiguous call, the other two thirds untouched / unread."""
    ops = _ops()
    dtype, n = BF16, 4099
    cap = n + n // 4 + 3 if static else n
    x, _, dy, gamma, beta = _inputs(cap, c, dtype, 17 * c + static)
    gg, bg = gamma.to(DEV), beta.to(DEV)
    n_dev = torch.tensor([n], dtype=torch.int32, device=DEV) if static else None
    where = f"bf16 c={c} n={n} cap={cap} block of {3 * c}"
    xs, dys = _padded(x, n, cap), _padded(dy, n, cap)
    rm, rv = _fresh_running(c)
    y0, sm0, si0 = _forward(xs, None, gg, bg, True, rm, rv, True, n_dev=n_dev)
    dx0, _, dg0, db0 = ops.bn_backward(dys, xs, None, gg, sm0, si0, True, True, False, n_dev=n_dev, beta=bg)
    wide_y = _sentinel((cap, 3 * c), dtype)
    rm1, rv1 = _fresh_running(c)
    y1, sm1, si1 = _forward(xs, None, gg, bg, True, rm1, rv1, True, n_dev=n_dev, out=wide_y[:, c:2 * c])
    wide_dy = torch.full((cap, 3 * c), float("nan"), dtype=dtype, device=DEV)
    wide_dy[:, c:2 * c] = dys
    block = wide_dy[:, c:2 * c]
    assert block.stride(0) == 3 * c and block.data_ptr() % 16 == 0
    dx1, _, dg1, db1 = ops.bn_backward(block, xs, None, gg, sm1, si1, True, True, False, n_dev=n_dev, beta=bg)
    _same_bits(wide_y[:n, c:2 * c], y0[:n], "y block")
    assert _is_sentinel(wide_y[:, :c]) and _is_sentinel(wide_y[:, 2 * c:]) and _is_sentinel(wide_y[n:, c:2 * c])
    for a, b, what in ((sm1, sm0, "save_mean"), (si1, si0, "save_invstd"), (rm1, rm, "running_mean"), (rv1, rv, "running_var"),
                       (dg1, dg0, "dgamma"), (db1, db0, "dbeta"), (dx1[:n], dx0[:n], "dx")):
        _same_bits(a, b, f"{what} at {where}")
    yb = wide_y[:, c:2 * c]
    _check_forward(where, dtype, x, None, gamma, beta, True, n, yb, sm1, si1, torch.zeros(c), torch.ones(c), rm1, rv1)
    _check_backward(where, dtype, dy, x, yb[:n], gamma, sm1, si1, True, n, dx1, None, dg1, db1)


# --------------------------------------------------------------------------------------------- 4. degenerate channels
@pytest.mark.parametrize("dtype,c", [(BF16, 16), (F32, 8)], ids=lambda v: _id(v))
def test_degenerate_channels_among_ordinary_ones(dtype, c):
    """channel 1 constant (var = 0); 2: gamma = beta = 0; 4: gamma = 0, beta > 0; 6: beta so negative that the ReLU closes everywhere."""
    ops = _ops()
    n = 4099
    x, _, dy, gamma, beta = _inputs(n, c, dtype, 4 * c)
    x[:, 1] = 0.75
    gamma[2], beta[2] = 0.0, 0.0
    gamma[4], beta[4] = 0.0, 0.625
    beta[6] = -50.0
    xg, dyg, gg, bg = (t.to(DEV) for t in (x, dy, gamma, beta))
    rm, rv = _fresh_running(c)
    y, sm, si = _forward(xg, None, gg, bg, True, rm, rv, True)
    where = f"{_id(dtype)} c={c} n={n} degenerate"
    ref, _ = _check_forward(where, dtype, x, None, gamma, beta, True, n, y, sm, si, torch.zeros(c), torch.ones(c), rm, rv)
    assert float(ref.var[1]) == 0.0
    yc = y.cpu()
    assert float(sm[1]) == 0.75 and float(ref.invstd[1]) == 1.0 / EPS ** 0.5       # (invstd itself was judged just above)
    assert not _bits(yc[:, 2]).any(), "gamma = beta = 0: the pre-activation is exactly +0"
    _same_bits(yc[:, 4], torch.full((n,), 0.625, dtype=dtype), "gamma = 0: y = beta")
    assert not _bits(yc[:, 6]).any(), "the ReLU is closed on the whole channel"
    results = []
    for y_arg, b_arg in ((None, bg), (y, None)):                     # mask recomputed from x / read from the stored y
        dx, dres, dgamma, dbeta = ops.bn_backward(dyg, xg, y_arg, gg, sm, si, True, True, True, beta=b_arg)
        _check_backward(where, dtype, dy, x, y, gamma, sm, si, True, n, dx, dres, dgamma, dbeta)
        dxc, drc, dgc, dbc = dx.cpu(), dres.cpu(), dgamma.cpu(), dbeta.cpu()
        mag = 0x7FFF if dtype == BF16 else 0x7FFFFFFF                # gamma * invstd = 0: dx is a zero of either sign
        for ch in (2, 4, 6):
            assert not (_bits(dxc[:, ch]) & mag).any(), f"dx of channel {ch} is not zero"
        for ch in (2, 6):                                            # the mask is closed: dz = +0, and so are the sums
            assert not _bits(drc[:, ch]).any() and float(dgc[ch]) == 0.0 and float(dbc[ch]) == 0.0
        _same_bits(drc[:, 4], dy[:, 4].contiguous(), "gamma = 0, beta > 0: the mask is open")
        assert abs(float(dbc[4]) - float(dy[:, 4].double().sum())) <= Bounds.SUM * float(dy[:, 4].double().abs().sum())
        results.append((dxc, drc, dgc, dbc))
    for a, b in zip(*results):
        _same_bits(a, b, "mask from x against mask from y")


# --------------------------------------------------------------------------------------------- 5. mask recomputation
@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted_by_one_float"])
@pytest.mark.parametrize("dtype,c", [(BF16, 16), (BF16, 128), (F32, 64)], ids=lambda v: _id(v))
def test_mask_recomputed_from_x_is_the_mask_the_forward_stored(dtype, c, shifted):
    """pcd_ops.h: with y = NULL the backward recomputes the ReLU mask `exactly as the forward computed it`.  x lies on a small
    lattice and beta puts the pre-activation of one lattice value per channel at 0 up to rounding, so thousands of elements sit
    where x * scale + shift evaluated differently (another association, a fused multiply-add) in bn_apply_kernel,
    bn_bwd_reduce_kernel or bn_bwd_apply_kernel would flip the mask; the lattice values are drawn unevenly (mean ~ -0.7) so
    that the mean * gamma * invstd inside the shift is as large as the shift itself.  A positive fp32 value never rounds to a bf16 zero, so the
    two masks must agree exactly."""
    ops = _ops()
    n = 4099
    g = torch.Generator().manual_seed(55 * c + shifted)
    # skewed over the lattice: a mean near 0 would leave mean * gamma * invstd too small for its rounding to reach the shift
    x = ((torch.rand(n, c, generator=g).square() * 17).floor().clamp(max=16) / 4 - 2).to(dtype)
    dy = torch.randn(n, c, generator=g).to(dtype)
    gamma = torch.rand(c, generator=g) + 0.5
    v = (torch.randint(2, 9, (c,), generator=g).double() / 4) * (torch.randint(0, 2, (c,), generator=g).double() * 2 - 1)
    st = bn_ref.forward(x, None, gamma, None, EPS, MOMENTUM, True, None, None, False)
    beta = (-gamma.double() * (v - st.mean) * st.invstd).float()
    ref = bn_ref.forward(x, None, gamma, beta, EPS, MOMENTUM, True, None, None, True)
    shift = beta.double() - st.mean * gamma.double() * st.invstd
    near = ref.pre.abs() <= 8 * U * shift.abs()
    assert float(near.double().mean()) >= 0.01, "the inputs do not put 1 % of the elements at a pre-activation of ~0"

    flat = torch.zeros(2 * c + 8, device=DEV)                              # as test_fused_batchnorm_unaligned_parameter_views
    off = 1 if shifted else 0
    gg, bg = flat[off:off + c], flat[c + 4 + off:c + 4 + off + c]
    gg.copy_(gamma); bg.copy_(beta)
    assert (gg.data_ptr() % 16 == 0) == (not shifted) and (bg.data_ptr() % 16 == 0) == (not shifted)
    xg, dyg = x.to(DEV), dy.to(DEV)
    rm, rv = _fresh_running(c)
    y, sm, si = _forward(xg, None, gg, bg, True, rm, rv, True)
    where = f"{_id(dtype)} c={c} n={n} lattice {'shifted' if shifted else 'aligned'}"
    ref, delta = _check_forward(where, dtype, x, None, gamma, beta, True, n, y, sm, si, torch.zeros(c), torch.ones(c), rm, rv)
    stored = y.cpu().float() > 0
    far = ref.pre.abs() > delta
    assert torch.equal(stored[far], (ref.pre > 0)[far]), "the stored mask is wrong away from 0"
    print(f"{where}: {int(near.sum())} elements within 8 u |shift| of 0, {int((~far).sum())} within delta, "
          f"{int((stored & near).sum())} of the near ones stored > 0")
    from_x = ops.bn_backward(dyg, xg, None, gg, sm, si, True, True, True, beta=bg)
    from_y = ops.bn_backward(dyg, xg, y, gg, sm, si, True, True, True)
    for a, b, what in zip(from_x, from_y, ("dx", "dresidual", "dgamma", "dbeta")):
        _same_bits(a, b, f"{what}, mask from x against mask from the stored y, at {where}")
    _check_backward(where, dtype, dy, x, y, gamma, sm, si, True, n, *from_x)


# --------------------------------------------------------------------------------------------- 6. eval mode
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("dtype,c", [(BF16, 32), (F32, 64)], ids=lambda v: _id(v))
def test_eval_mode_forward_and_backward(dtype, c, with_res):
    """training = 0: running statistics in the forward; the backward with save_mean = running_mean and save_invstd =
    rsqrt(running_var + eps) as FusedBNFunction passes them: dx = gamma * invstd * dz, dgamma / dbeta as sums."""
    ops = _ops()
    n = 4099
    x, res, dy, gamma, beta = _inputs(n, c, dtype, 6 * c + with_res)
    g = torch.Generator().manual_seed(c)
    rm_c, rv_c = torch.randn(c, generator=g) * 0.5, torch.rand(c, generator=g) * 2 + 0.25
    xg, rg, dyg, gg, bg, rm, rv = (t.to(DEV) for t in (x, res, dy, gamma, beta, rm_c, rv_c))
    for relu in (True, False):
        where = f"{_id(dtype)} c={c} n={n} eval relu={int(relu)} res={int(with_res)}"
        y, _, _ = _forward(xg, rg if with_res else None, gg, bg, False, rm, rv, relu)
        _check_forward(where, dtype, x, res if with_res else None, gamma, beta, relu, n, y, None, None, rm_c, rv_c, rm, rv,
                       training=False)
        si = torch.rsqrt(rv + EPS)
        dx, dres, dgamma, dbeta = ops.bn_backward(dyg, xg, y if relu else None, gg, rm, si, relu, False, with_res)
        _check_backward(where, dtype, dy, x, y if relu else None, gamma, rm, si, False, n, dx, dres, dgamma, dbeta)


# --------------------------------------------------------------------------------------------- 7. offset inputs
@pytest.mark.parametrize("m", [0, 10, 100])
@pytest.mark.parametrize("dtype,c", [(F32, 64), (BF16, 128)], ids=lambda v: _id(v))
def test_single_pass_variance_with_an_offset_mean(dtype, c, m):
    """x ~ N(m, 1): the variance is E[x^2] - mean^2 in double over fp32 per-thread partial sums, so its error grows with
    (m / std)^2.  The bounds scale with E[x^2]: this asserts an honest single-pass fp32 sum and no worse.  The worst relative
    invstd error is printed beside that of torch's own fp32 batch norm on the same input (table in DESIGN.md)."""
    ops = _ops()
    n = 4099
    x, _, dy, gamma, beta = _inputs(n, c, dtype, 7 * c + m, mean=float(m), std=1.0)
    xg, dyg, gg, bg = (t.to(DEV) for t in (x, dy, gamma, beta))
    rm, rv = _fresh_running(c)
    y, sm, si = _forward(xg, None, gg, bg, True, rm, rv, True)
    where = f"{_id(dtype)} c={c} n={n} x ~ N({m}, 1)"
    ref, _ = _check_forward(where, dtype, x, None, gamma, beta, True, n, y, sm, si, torch.zeros(c), torch.ones(c), rm, rv)
    dx, _, dgamma, dbeta = ops.bn_backward(dyg, xg, None, gg, sm, si, True, True, False, beta=bg)
    _check_backward(where, dtype, dy, x, y, gamma, sm, si, True, n, dx, None, dgamma, dbeta)
    t_inv = torch.native_batch_norm(xg.float(), gg, bg, torch.zeros(c, device=DEV), torch.ones(c, device=DEV), True,
                                    MOMENTUM, EPS)[2]
    ours = float(((si.cpu().double() - ref.invstd) / ref.invstd).abs().max())
    theirs = float(((t_inv.cpu().double() - ref.invstd) / ref.invstd).abs().max())
    print(f"invstd relative error, {where}: fused.hip {ours:.3e}, torch fp32 {theirs:.3e}")


# --------------------------------------------------------------------------------------------- 8. column sums
@pytest.mark.parametrize("static", [False, True], ids=["host_n", "n_dev"])
@pytest.mark.parametrize("n,c", [(1, 8), (257, 40), (4099, 128), (12289, 1024)])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda v: _id(v))
def test_col_sum_against_the_fp64_column_sum(dtype, n, c, static):
    ops = _ops()
    cap = n + n // 4 + 3 if static else n
    x = _inputs(cap, c, dtype, 8 * c + n)[0]
    n_dev = torch.tensor([n], dtype=torch.int32, device=DEV) if static else None
    out = ops.col_sum(_padded(x, n, cap), n_dev=n_dev)
    xd = x[:n].double()
    _judge("col_sum", f"{_id(dtype)} n={n} c={c} cap={cap}", out, xd.sum(0), Bounds.SUM * xd.abs().sum(0))


@pytest.mark.parametrize("dtype,c,n", [(BF16, 40, 1), (F32, 12, 257), (BF16, 128, 4099), (BF16, 128, 24577), (BF16, 1024, 3073)],
                         ids=lambda v: _id(v))
def test_backward_column_sums_of_dx_as_stored(dtype, c, n):
    """bn_backward(colsum=True) + col_sum_finalize = the column sums of the dx the kernel STORED (the bias gradient of the conv in
    front); 24577 rows of 128 channels put the apply grid, whose workgroups own one partial row each, at its cap."""
    ops = _ops()
    x, res, dy, gamma, beta = _inputs(n, c, dtype, 9 * c + n)
    xg, rg, dyg, gg, bg = (t.to(DEV) for t in (x, res, dy, gamma, beta))
    rm, rv = _fresh_running(c)
    y, sm, si = _forward(xg, rg, gg, bg, True, rm, rv, True)
    dx, _, _, _, (partial, rows) = ops.bn_backward(dyg, xg, y, gg, sm, si, True, True, False, colsum=True)
    assert rows == min(2048, -(-n * (c // (8 if dtype == BF16 else 4)) // 1024)) and partial.shape == (rows, c)
    out = ops.col_sum_finalize(partial, rows)
    dxd = dx.cpu().double()
    _judge("colsum_of_dx", f"{_id(dtype)} n={n} c={c} rows={rows}", out, dxd.sum(0), Bounds.SUM * dxd.abs().sum(0))


def test_col_sum_finalize_batched_over_two_launches():
    """33 jobs of mixed (rows, c): the second launch of the 32-job chunking runs; rows 0 (nothing read) and 1, c up to 1024."""
    ops = _ops()
    g = torch.Generator().manual_seed(33)
    shapes = [(0, 16), (1, 8), (1, 1024), (2, 40), (7, 12), (15, 1024), (16, 128), (17, 96), (33, 1000), (127, 320), (128, 64),
              (129, 4), (511, 128), (512, 256), (513, 24), (2048, 1024)]
    shapes = (shapes * 3)[:32] + [(5, 72)]
    assert len(shapes) == 33 > _L().COLSUM_MAX_JOBS
    jobs, refs = [], []
    for rows, c in shapes:
        part = torch.randn(max(rows, 1), c, generator=g) * 3 + 0.5
        if rows == 0:
            part[:] = float("nan")
        refs.append(part[:rows].double())
        jobs.append((part.to(DEV), rows, torch.full((c,), float("nan"), device=DEV)))
    ops.col_sum_finalize_batched(jobs)
    for i, ((rows, c), ref, job) in enumerate(zip(shapes, refs, jobs)):
        _judge("colsum_batched", f"job {i} rows={rows} c={c}", job[2], ref.sum(0), Bounds.SUM * ref.abs().sum(0))


# --------------------------------------------------------------------------------------------- 9. autograd wiring
def test_autograd_wiring_of_batch_norm_act():
    """functional.batch_norm_act on an nn.BatchNorm1d: training with a residual (the saved-y path), training without (the mask from
    x), eval mode with gradients for x and the affine parameters: every gradient, the running statistics and num_batches_tracked
    against bn_ref under the bounds of the direct calls."""
    from com_amd.spconv import functional as Fsp
    ops = _ops()
    dtype, c, n = BF16, 32, 4099
    x, res, dy, gamma, beta = _inputs(n, c, dtype, 99)
    bn = torch.nn.BatchNorm1d(c, eps=1e-3, momentum=0.01).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    steps = 0
    for training, with_res in ((True, True), (True, False), (False, True), (False, False)):
        where = f"batch_norm_act training={int(training)} res={int(with_res)}"
        bn.train(training)
        bn.weight.grad = bn.bias.grad = None
        xg = x.to(DEV).requires_grad_(True)
        rg = res.to(DEV).requires_grad_(True) if with_res else None
        rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
        y = Fsp.batch_norm_act(bn, xg, rg, True)
        assert y.dtype == dtype and y.grad_fn is not None
        y.backward(dy.to(DEV))
        steps += training
        assert int(bn.num_batches_tracked) == steps
        if training:       # the statistics the function saved: the same call again (the kernels are deterministic)
            _, sm, si = _forward(xg.detach(), rg.detach() if with_res else None, bn.weight.detach(), bn.bias.detach(), True,
                                 rm0.clone(), rv0.clone(), True)
        else:
            sm, si = bn.running_mean, torch.rsqrt(bn.running_var + bn.eps)
        _check_forward(where, dtype, x, res if with_res else None, gamma, beta, True, n, y, sm, si, rm0, rv0,
                       bn.running_mean, bn.running_var, training=training)
        _check_backward(where, dtype, dy, x, y.detach(), gamma, sm, si, training, n, xg.grad, rg.grad if with_res else None,
                        bn.weight.grad, bn.bias.grad)


# --------------------------------------------------------------------------------------------- 10. refusals
def test_unsupported_width_and_short_row_stride_are_refused_before_any_launch():
    L = _L()
    n = 4
    for c, y_ld, want in ((2048, 2048, L.CONSTANTS["PCD_ERR_UNSUPPORTED"]), (16, 8, L.CONSTANTS["PCD_ERR_INVALID_ARG"])):
        x = torch.randn(n, c, device=DEV).bfloat16()
        y = _sentinel((n, c), BF16)
        gamma, beta = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
        rm, rv = _fresh_running(c)
        sm, si = torch.full((c,), 7.0, device=DEV), torch.full((c,), 7.0, device=DEV)
        assert _raw_forward(x, None, gamma, beta, True, rm, rv, True, y, y_ld, sm, si, n, c) == want
        torch.cuda.synchronize()
        assert _is_sentinel(y) and bool((sm == 7.0).all()) and bool((si == 7.0).all())
        assert not rm.any() and bool((rv == 1.0).all())
