"""What the dense heads' host code shares: how prediction maps and their gradients are handed to the C ABI (element
strides, float32 / bfloat16), and the class table of one head."""
import ctypes
from types import SimpleNamespace

import torch

from .. import _lib as L

dtype_code = L.dtype_code


def like(t):
    """an uninitialised tensor with EXACTLY t's strides (torch.empty_like densifies a non-dense view, e.g. the 1-3 real
    channels of a prediction map that was computed with zero-padded channels)."""
    return torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device)


def pack_maps(hm, regs, grads=None):
    """The map arguments of pcd_centerhead_loss_* / pcd_com_loss_*: heat map `hm` and regression maps `regs` [B, c, H, W]
    behind any strides (`grads`: the regression gradients, same layout).  The arrays live as long as the returned object:
    keep it referenced until the call has returned."""
    assert all(r.dtype == regs[0].dtype for r in regs)
    n = len(regs)
    m = SimpleNamespace(
        n=n, hm_dtype=dtype_code(hm), hm_strides=(ctypes.c_longlong * 4)(*hm.stride()),
        reg_dtype=dtype_code(regs[0]) if regs else L.PCD_F32,
        reg_ptrs=(ctypes.c_void_p * n)(*[r.data_ptr() for r in regs]),
        reg_ch=(ctypes.c_int * n)(*[int(r.shape[1]) for r in regs]),
        reg_strides=(ctypes.c_longlong * (4 * n))(*[v for r in regs for v in r.stride()]))
    if grads is not None:
        assert all(d.stride() == r.stride() for d, r in zip(grads, regs))
        m.reg_grads = (ctypes.c_void_p * n)(*[d.data_ptr() for d in grads])
    return m


def head_class_map(class_names, head_names):
    """dataset class id (1-based; 0 = padding) -> 1-based id inside the head, 0 = not in the head"""
    head_names = list(head_names)
    return [0] + [head_names.index(name) + 1 if name in head_names else 0 for name in class_names]
