"""Point-in-box tests and RoI-aware pooling with the function names and signatures of the reference's
pcdet/ops/roiaware_pool3d/roiaware_pool3d_utils.py:9-107, over com_amd/csrc/roiaware.hip:

    from com_amd import roiaware_pool3d as roiaware_pool3d_utils

`points_in_boxes_cpu` is the host-side variant that box_utils.remove_points_in_boxes3d (box_utils.py:117-131) calls per
frame inside the DataLoader workers of COMAug's database samplers (database_sampler_v2.py:538, database_sampler.py:458):
numpy arrays / CPU tensors in, the library's host entry point pcd_points_in_boxes_host underneath (no GPU call: usable in
forked workers).  `points_in_boxes_gpu` and `RoIAwarePool3d` take HIP device tensors and refuse anything else."""
import ctypes

import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib as L


def _host_array(a):
    if isinstance(a, np.ndarray):
        return np.ascontiguousarray(a, dtype=np.float32)
    assert not a.is_cuda, 'Only support CPU tensors'
    return np.ascontiguousarray(a.detach().float().numpy())


def points_in_boxes_cpu(points, boxes):
    """roiaware_pool3d_utils.py:9-25: points (num_points, 3), boxes (N, 7) -> point_indices (N, num_points) int32 0 / 1;
    numpy in -> numpy out, tensor in -> tensor out (the reference's check_numpy_to_torch convention)."""
    assert boxes.shape[1] == 7
    assert points.shape[1] == 3
    is_numpy = isinstance(boxes, np.ndarray)                   # (the reference keeps the flag of its second conversion)
    p, b = _host_array(points), _host_array(boxes)
    out = np.zeros((b.shape[0], p.shape[0]), np.int32)
    L.check(L.lib().pcd_points_in_boxes_host(b.ctypes.data_as(ctypes.c_void_p), b.shape[0], p.ctypes.data_as(ctypes.c_void_p),
                                             p.shape[0], out.ctypes.data_as(ctypes.c_void_p)), "pcd_points_in_boxes_host")
    return out if is_numpy else torch.from_numpy(out)


def _device(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.PcdError(f"{what} needs HIP device tensors (there is no CPU fallback)")
    return t.contiguous().float()


def points_in_boxes_gpu(points, boxes):
    """roiaware_pool3d_utils.py:28-41: points (B, M, 3), boxes (B, T, 7) -> box_idxs_of_pts (B, M) int32, the lowest
    index of a box that contains the point, -1 for background."""
    p, b = _device(points, "points_in_boxes_gpu"), _device(boxes, "points_in_boxes_gpu")
    assert b.shape[0] == p.shape[0]
    assert b.shape[2] == 7 and p.shape[2] == 3
    batch_size, num_points, _ = p.shape
    out = torch.empty((batch_size, num_points), dtype=torch.int32, device=p.device)
    L.check(L.lib().pcd_points_in_boxes(L.ptr(b), L.ptr(p), batch_size, int(b.shape[1]), num_points, L.ptr(out),
                                        L.stream_ptr()), "pcd_points_in_boxes")
    return out


class RoIAwarePool3d(nn.Module):
    """roiaware_pool3d_utils.py:44-52"""

    def __init__(self, out_size, max_pts_each_voxel=128):
        super().__init__()
        self.out_size = out_size
        self.max_pts_each_voxel = max_pts_each_voxel

    def forward(self, rois, pts, pts_feature, pool_method='max'):
        assert pool_method in ['max', 'avg']
        return RoIAwarePool3dFunction.apply(rois, pts, pts_feature, self.out_size, self.max_pts_each_voxel, pool_method)


def roiaware_pool3d_forward(rois, pts, pts_feature, out_size, max_pts_each_voxel, pool_method):
    """pcd_roiaware_pool3d_forward: (pooled_features (N, ox, oy, oz, C), pts_idx_of_voxels int32 (N, ox, oy, oz,
    max_pts_each_voxel), argmax int32 (N, ox, oy, oz, C) or None for 'avg')."""
    assert rois.shape[1] == 7 and pts.shape[1] == 3
    if isinstance(out_size, int):
        out_x = out_y = out_z = out_size
    else:
        assert len(out_size) == 3
        for k in range(3):
            assert isinstance(out_size[k], int)
        out_x, out_y, out_z = out_size
    method = {'max': 0, 'avg': 1}[pool_method]
    r, p, f = (_device(t, "RoIAwarePool3d") for t in (rois, pts, pts_feature))
    assert f.dim() == 2 and f.shape[0] == p.shape[0]
    n, c = int(r.shape[0]), int(f.shape[1])
    pooled = torch.empty((n, out_x, out_y, out_z, c), dtype=torch.float32, device=f.device)
    argmax = torch.empty((n, out_x, out_y, out_z, c), dtype=torch.int32, device=f.device) if method == 0 else None
    lists = torch.empty((n, out_x, out_y, out_z, int(max_pts_each_voxel)), dtype=torch.int32, device=f.device)
    L.check(L.lib().pcd_roiaware_pool3d_forward(L.ptr(r), n, L.ptr(p), int(p.shape[0]), L.ptr(f), c, out_x, out_y, out_z,
                                                int(max_pts_each_voxel), method, L.ptr(lists), L.ptr(argmax), L.ptr(pooled),
                                                L.stream_ptr()), "pcd_roiaware_pool3d_forward")
    return pooled, lists, argmax


class RoIAwarePool3dFunction(Function):
    """roiaware_pool3d_utils.py:55-107: the gradient flows to pts_feature only."""

    @staticmethod
    def forward(ctx, rois, pts, pts_feature, out_size, max_pts_each_voxel, pool_method):
        pooled, lists, argmax = roiaware_pool3d_forward(rois, pts, pts_feature, out_size, max_pts_each_voxel, pool_method)
        ctx.roiaware_pool3d_for_backward = (lists, argmax, {'max': 0, 'avg': 1}[pool_method], int(pts.shape[0]),
                                            int(pts_feature.shape[-1]))
        return pooled.to(pts_feature.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        lists, argmax, method, num_pts, num_channels = ctx.roiaware_pool3d_for_backward
        g = grad_out.contiguous().float()
        grad_in = torch.empty((num_pts, num_channels), dtype=torch.float32, device=g.device)
        n, ox, oy, oz, mpv = (int(v) for v in lists.shape)
        L.check(L.lib().pcd_roiaware_pool3d_backward(L.ptr(lists), L.ptr(argmax), L.ptr(g), n, ox, oy, oz, num_channels, mpv,
                                                     method, num_pts, L.ptr(grad_in), L.stream_ptr()),
                "pcd_roiaware_pool3d_backward")
        return None, None, grad_in.to(grad_out.dtype), None, None, None
