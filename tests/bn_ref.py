"""fp64 restatement of the fused BatchNorm1d (+ residual) (+ ReLU) of include/pcd_ops.h (a11), for test_bn_ref_cpu.py (which pins it
to torch.nn.BatchNorm1d in float64) and test_gpu_fused_bn.py (which holds com_amd/csrc/fused.hip to it).

It follows the kernel's CONTRACT, not its arithmetic: every input is a value already rounded to the kernel's dtype and widened to
float64, nothing is rounded on the way, and the ReLU mask of the backward is an ARGUMENT -- the GPU tests hand in `y_stored > 0` of
the output the kernel itself stored, so that no element has to be excused for lying within a rounding of zero.  `mean` / `invstd`
may be handed in as well (the statistics the kernel saved): their error is judged once, in the forward.

  forward : pre = (x - mean) * invstd * gamma + beta (+ residual);  y = max(pre, 0) with relu
            training: mean, BIASED var over the n rows, invstd = 1 / sqrt(var + eps);
                      running = (1 - momentum) * running + momentum * batch, the batch variance UNBIASED (n / (n - 1)) when n > 1,
                      the biased value at n == 1 (the kernel's guard; torch raises there); n == 0: mean = var = 0
            eval    : mean = running_mean, var = running_var, running statistics unchanged
  backward: dz = dy * mask (no mask: dy); dresidual = dz; dbeta = sum dz; dgamma = sum dz * xhat;
            dx = gamma * invstd * (dz - dbeta / n - xhat * dgamma / n)  (training)  or  gamma * invstd * dz  (eval)
"""
from collections import namedtuple

import torch

Forward = namedtuple("Forward", "y pre mean var invstd running_mean running_var")
Backward = namedtuple("Backward", "dz dx dgamma dbeta dresidual xhat")


def _f64(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().double()


def forward(x, residual, gamma, beta, eps, momentum, training, running_mean, running_var, relu, n=None, mean=None, invstd=None):
    """x / residual [rows >= n, c]; only the first n rows count (n = None: all of them).  gamma / beta None: 1 / 0."""
    x = _f64(x)
    n = x.shape[0] if n is None else int(n)
    x = x[:n]
    c = x.shape[1]
    gamma = torch.ones(c, dtype=torch.float64) if gamma is None else _f64(gamma)
    beta = torch.zeros(c, dtype=torch.float64) if beta is None else _f64(beta)
    rm, rv = _f64(running_mean), _f64(running_var)
    if training:
        if n > 0:
            bmean = x.mean(0)
            var = (x - bmean).square().mean(0)
        else:
            bmean = torch.zeros(c, dtype=torch.float64)
            var = torch.zeros(c, dtype=torch.float64)
        unbiased = var * n / (n - 1) if n > 1 else var
        new_rm = None if rm is None else (1.0 - momentum) * rm + momentum * bmean
        new_rv = None if rv is None else (1.0 - momentum) * rv + momentum * unbiased
    else:
        bmean, var = rm, rv
        new_rm, new_rv = rm, rv
    binv = 1.0 / torch.sqrt(var + eps)
    use_mean = bmean if mean is None else _f64(mean)
    use_inv = binv if invstd is None else _f64(invstd)
    pre = (x - use_mean) * use_inv * gamma + beta
    if residual is not None:
        pre = pre + _f64(residual)[:n]
    y = pre.clamp(min=0.0) if relu else pre
    return Forward(y, pre, bmean, var, binv, new_rm, new_rv)


def backward(dy, x, mask, gamma, mean, invstd, training, n=None):
    """mask: bool [rows, c] (True = the ReLU let the element through) or None (no ReLU)."""
    x, dy = _f64(x), _f64(dy)
    n = x.shape[0] if n is None else int(n)
    x, dy = x[:n], dy[:n]
    c = x.shape[1]
    gamma = torch.ones(c, dtype=torch.float64) if gamma is None else _f64(gamma)
    mean, invstd = _f64(mean), _f64(invstd)
    dz = dy if mask is None else torch.where(torch.as_tensor(mask).cpu()[:n], dy, torch.zeros_like(dy))   # (+0 where closed)
    xhat = (x - mean) * invstd
    dbeta = dz.sum(0)
    dgamma = (dz * xhat).sum(0)
    if training:
        inv_n = 1.0 / n if n > 0 else 0.0
        dx = gamma * invstd * (dz - dbeta * inv_n - xhat * (dgamma * inv_n))
    else:
        dx = gamma * invstd * dz
    return Backward(dz, dx, dgamma, dbeta, dz, xhat)
