"""tests/bn_ref.py (the fp64 reference the fused BatchNorm kernels are held to in test_gpu_fused_bn.py) against
torch.nn.BatchNorm1d in float64 with autograd, on the CPU.  Both sides are fp64 and differ by summation order only: 1e-12.
For these comparisons only, the ReLU mask is the reference's own pre-activation > 0 (what torch's relu differentiates)."""
import pytest
import torch

from tests import bn_ref

EPS, MOMENTUM = 1e-3, 0.01
RTOL = 1e-12


def _close(got, want, what):
    want = want.detach()
    scale = float(want.abs().max()) if want.numel() else 0.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= RTOL * max(scale, 1e-300), f"{what}: |diff| {err:.3e} against max |ref| {scale:.3e}"


def _inputs(n, c, res, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g, dtype=torch.float64) * 1.7 + 0.3
    r = torch.randn(n, c, generator=g, dtype=torch.float64) if res else None
    dy = torch.randn(n, c, generator=g, dtype=torch.float64)
    gamma = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(c, generator=g, dtype=torch.float64) * 0.3
    rm = torch.randn(c, generator=g, dtype=torch.float64)
    rv = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    return x, r, dy, gamma, beta, rm, rv


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("c", [4, 40])
@pytest.mark.parametrize("n", [2, 3, 257])
def test_reference_matches_torch_batchnorm_in_float64(n, c, training, res, relu):
    x, r, dy, gamma, beta, rm, rv = _inputs(n, c, res, 1000 * n + 10 * c + 2 * res + relu)
    bn = torch.nn.BatchNorm1d(c, eps=EPS, momentum=MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    bn.train(training)
    xt = x.clone().requires_grad_(True)
    rt = r.clone().requires_grad_(True) if res else None
    yt = bn(xt)
    if res:
        yt = yt + rt
    if relu:
        yt = torch.relu(yt)
    yt.backward(dy)

    f = bn_ref.forward(x, r, gamma, beta, EPS, MOMENTUM, training, rm, rv, relu)
    _close(f.y, yt, "y")
    _close(f.running_mean, bn.running_mean, "running_mean")
    _close(f.running_var, bn.running_var, "running_var")
    if training:
        _close(f.var, x.var(0, unbiased=False), "biased var")
        _close(f.invstd, (x.var(0, unbiased=False) + EPS).rsqrt(), "invstd")
    else:
        assert torch.equal(f.running_mean, rm) and torch.equal(f.running_var, rv) and torch.equal(f.mean, rm)
    b = bn_ref.backward(dy, x, (f.pre > 0) if relu else None, gamma, f.mean, f.invstd, training)
    _close(b.dx, xt.grad, "dx")
    _close(b.dgamma, bn.weight.grad, "dgamma")
    _close(b.dbeta, bn.bias.grad, "dbeta")
    if res:
        _close(b.dresidual, rt.grad, "dresidual")
    assert torch.equal(b.dresidual, b.dz)


def test_handed_in_statistics_replace_the_batch_statistics():
    """mean= / invstd= are used for the output and leave the returned batch statistics alone."""
    x, r, dy, gamma, beta, rm, rv = _inputs(33, 8, False, 5)
    f0 = bn_ref.forward(x, None, gamma, beta, EPS, MOMENTUM, True, rm, rv, False)
    m, i = f0.mean + 0.25, f0.invstd * 1.5
    f1 = bn_ref.forward(x, None, gamma, beta, EPS, MOMENTUM, True, rm, rv, False, mean=m, invstd=i)
    assert torch.equal(f1.mean, f0.mean) and torch.equal(f1.invstd, f0.invstd) and torch.equal(f1.running_var, f0.running_var)
    _close(f1.y, (x - m) * i * gamma + beta, "y from the given statistics")


def test_row_count_below_the_capacity_ignores_the_tail():
    x, r, dy, gamma, beta, rm, rv = _inputs(40, 8, True, 6)
    f0 = bn_ref.forward(x[:29], r[:29], gamma, beta, EPS, MOMENTUM, True, rm, rv, True)
    xp, rp, dyp = x.clone(), r.clone(), dy.clone()
    xp[29:] = float("nan"); rp[29:] = float("nan"); dyp[29:] = float("nan")
    f1 = bn_ref.forward(xp, rp, gamma, beta, EPS, MOMENTUM, True, rm, rv, True, n=29)
    for a, b in zip(f0, f1):
        assert torch.equal(a, b)
    b0 = bn_ref.backward(dy[:29], x[:29], f0.pre > 0, gamma, f0.mean, f0.invstd, True)
    mask = torch.zeros(40, 8, dtype=torch.bool)
    mask[:29] = f0.pre > 0
    b1 = bn_ref.backward(dyp, xp, mask, gamma, f0.mean, f0.invstd, True, n=29)
    for a, b in zip(b0, b1):
        assert torch.equal(a, b)


@pytest.mark.parametrize("c", [4, 40])
def test_single_row_in_training_mode_follows_the_documented_guard(c):
    """torch raises at n = 1 in training mode; the kernel documents var = 0, invstd = 1 / sqrt(eps) and a running_var updated with
    the biased value (0).  Pinned by the formula."""
    x, r, dy, gamma, beta, rm, rv = _inputs(1, c, False, 7 + c)
    f = bn_ref.forward(x, None, gamma, beta, EPS, MOMENTUM, True, rm, rv, True)
    assert torch.equal(f.mean, x[0])
    assert torch.equal(f.var, torch.zeros(c, dtype=torch.float64))
    assert torch.equal(f.invstd, torch.full((c,), 1.0 / EPS ** 0.5, dtype=torch.float64))
    assert torch.equal(f.running_var, (1.0 - MOMENTUM) * rv + MOMENTUM * 0.0)
    assert torch.equal(f.running_mean, (1.0 - MOMENTUM) * rm + MOMENTUM * x[0])
    _close(f.y, beta.clamp(min=0.0).expand(1, c), "y = relu(beta)")
    b = bn_ref.backward(dy, x, f.pre > 0, gamma, f.mean, f.invstd, True)
    assert torch.equal(b.dx, torch.zeros(1, c, dtype=torch.float64))      # dz - dbeta / 1 - 0 * dgamma
    assert torch.equal(b.dgamma, torch.zeros(c, dtype=torch.float64))


def test_no_rows_in_training_mode():
    """An empty frame: mean = var = 0, invstd = 1 / sqrt(eps), zero gradients (the running statistics decay towards 0, as the
    kernel's n == 0 branch has it)."""
    c = 8
    _, _, _, gamma, beta, rm, rv = _inputs(1, c, False, 9)
    e = torch.zeros(0, c, dtype=torch.float64)
    f = bn_ref.forward(e, None, gamma, beta, EPS, MOMENTUM, True, rm, rv, True)
    assert f.y.shape == (0, c) and not f.mean.any() and not f.var.any()
    assert torch.equal(f.invstd, torch.full((c,), 1.0 / EPS ** 0.5, dtype=torch.float64))
    b = bn_ref.backward(e, e, None, gamma, f.mean, f.invstd, True)
    assert b.dx.shape == (0, c) and not b.dgamma.any() and not b.dbeta.any()
