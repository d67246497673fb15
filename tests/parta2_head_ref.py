"""A CPU restatement of what PartA2FCHead pools (pcdet/models/roi_heads/partA2_head.py:104-151, :184-195) over a literal
transcription of the contract of pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu; it shares no code with the kernels.

    voxel_of_points     generate_pts_mask_for_box3d (:39-75) with check_pt_in_box3d (:23-36): float32 arithmetic, the xy
                        comparison in double, the voxel index int((local + d / 2) / res) clamped to the grid
    collect             collect_inside_pts_for_box3d (:78-108): per voxel the ascending point indices, cut after
                        max_pts_each_voxel - 1 entries; slot 0 is the count
    RoIAwarePool3d      the stand-in for roiaware_pool3d_utils.RoIAwarePool3d the fixtures' generator hands to the reference's
                        head: the lists above, 'avg' = sum in list order / count (:160-190), 'max' = first strict maximum
                        (:111-157), differentiable in the features, in whatever dtype they come
    sparse_rows         roiaware_pool + nonzero + gather of the head's forward in numpy (fp64 pooling unless told otherwise)
    margins             how far the points of a scene lie from the faces that decide a case, in cells

The geometry is evaluated in float32 exactly as the kernel does it; the fixtures keep every point at least 1e-4 of a cell away
from a voxel face and a box face, so no rounding of cos / sin can move a point into another voxel."""
import numpy as np
import torch

F = np.float32


def _local(rois, pts):
    """(inside [N, P] bool, local x / y / z [N, P] float32) -- check_pt_in_box3d + lidar_to_local_coords"""
    rois, pts = np.asarray(rois, F), np.asarray(pts, F)
    x, y, z = pts[None, :, 0], pts[None, :, 1], pts[None, :, 2]
    cx, cy, cz = rois[:, 0:1], rois[:, 1:2], rois[:, 2:3]
    dx, dy, dz, rz = rois[:, 3:4], rois[:, 4:5], rois[:, 5:6], rois[:, 6:7]
    z_ok = ~(np.abs(z - cz).astype(np.float64) > dz.astype(np.float64) / 2.0)
    cosa, sina = np.cos(-rz).astype(F), np.sin(-rz).astype(F)
    sx, sy = (x - cx).astype(F), (y - cy).astype(F)
    lx = ((sx * cosa).astype(F) + (sy * (-sina)).astype(F)).astype(F)
    ly = ((sx * sina).astype(F) + (sy * cosa).astype(F)).astype(F)
    margin = np.float64(F(1e-5))
    in_xy = (np.abs(lx).astype(np.float64) < dx.astype(np.float64) / 2.0 + margin) & \
            (np.abs(ly).astype(np.float64) < dy.astype(np.float64) / 2.0 + margin)
    return z_ok & in_xy, lx, ly, (z - cz).astype(F)


def voxel_of_points(rois, pts, out):
    """[N, P] int64: the flat voxel (x * out + y) * out + z of a point inside the RoI, -1 outside"""
    rois = np.asarray(rois, F)
    inside, lx, ly, lz = _local(rois, pts)
    idx = []
    with np.errstate(divide='ignore', invalid='ignore'):
        for loc, d in ((lx, rois[:, 3:4]), (ly, rois[:, 4:5]), (lz, rois[:, 5:6])):
            res = (d / F(out)).astype(F)
            q = ((loc + (d / F(2)).astype(F)).astype(F) / res).astype(F)
            q = np.where(np.isfinite(q), q, 0)
            idx.append(np.clip(np.trunc(q).astype(np.int64), 0, out - 1))
    flat = (idx[0] * out + idx[1]) * out + idx[2]
    return np.where(inside, flat, -1)


def collect(vox, nvox, mpv):
    """lists int32 [N, nvox, mpv]: slot 0 the count, then ascending point indices, at most mpv - 1"""
    n = vox.shape[0]
    lists = np.zeros((n, nvox, mpv), np.int32)
    for b in range(n):
        for k in np.nonzero(vox[b] >= 0)[0]:
            v = vox[b, k]
            cnt = lists[b, v, 0]
            if cnt < mpv - 1:
                lists[b, v, cnt + 1] = k
                lists[b, v, 0] += 1
    return lists


class RoIAwarePool3d(torch.nn.Module):
    """roiaware_pool3d_utils.RoIAwarePool3d on the CPU: (N, out, out, out, C), differentiable in pts_feature"""

    def __init__(self, out_size, max_pts_each_voxel=128):
        super().__init__()
        self.out_size, self.max_pts_each_voxel = int(out_size), int(max_pts_each_voxel)

    def forward(self, rois, pts, pts_feature, pool_method='max'):
        assert pool_method in ('max', 'avg')
        out, mpv = self.out_size, self.max_pts_each_voxel
        n, c = rois.shape[0], pts_feature.shape[1]
        vox = voxel_of_points(rois.detach().float().numpy(), pts.detach().float().numpy(), out)
        lists = collect(vox, out ** 3, mpv)
        cnt = torch.from_numpy(lists[:, :, 0].astype(np.int64))
        pooled = pts_feature.new_zeros((n, out ** 3, c))
        if pool_method == 'avg':
            for k in range(1, mpv):                           # list order
                idx = torch.from_numpy(lists[:, :, k].astype(np.int64))
                live = (cnt >= k).unsqueeze(-1).to(pts_feature.dtype)
                pooled = pooled + pts_feature[idx] * live
            pooled = pooled / cnt.clamp(min=1).unsqueeze(-1).to(pts_feature.dtype)
        else:
            with torch.no_grad():
                best = pts_feature.new_full((n, out ** 3, c), -float('inf'))
                arg = torch.full((n, out ** 3, c), -1, dtype=torch.int64)
                for k in range(1, mpv):
                    idx = torch.from_numpy(lists[:, :, k].astype(np.int64))
                    val = pts_feature[idx]
                    take = (cnt >= k).unsqueeze(-1) & (val > best)    # the first strict maximum
                    best = torch.where(take, val, best)
                    arg = torch.where(take, idx.unsqueeze(-1).expand_as(arg), arg)
            chan = torch.arange(c).view(1, 1, c).expand_as(arg)
            pooled = torch.where(arg >= 0, pts_feature[arg.clamp(min=0), chan], pooled)
        return pooled.view(n, out, out, out, c)


def part_features(point_part, point_scores, thresh):
    """partA2_head.py:121-125 in the dtype of point_part; the threshold compares in float32, as torch compares a float32
    tensor with a Python scalar"""
    part = np.concatenate([np.asarray(point_part), np.asarray(point_scores).reshape(-1, 1).astype(np.asarray(point_part).dtype)], axis=1)
    part[np.asarray(point_scores, F) < F(thresh), 0:3] = 0
    return part


def sparse_rows(rois, point_coords, point_features, point_part, point_scores, thresh, out, mpv, dtype=np.float64):
    """dict(coords int32 [rows, 4], part_rows, rpn_rows, fake, sums, lists per frame) -- roiaware_pool (:104-151) and the
    nonzero / gather of forward (:184-195), pooled in `dtype`"""
    rois = np.asarray(rois, F)
    B, N = rois.shape[:2]
    pc = np.asarray(point_coords, F)
    part = part_features(np.asarray(point_part, dtype), point_scores, thresh)
    feats = np.asarray(point_features, dtype)
    pooled_part, pooled_rpn, all_lists = [], [], []
    layer = RoIAwarePool3d(out, mpv)
    for b in range(B):
        m = pc[:, 0] == b
        r, p = torch.from_numpy(rois[b, :, :7].copy()), torch.from_numpy(pc[m, 1:4].copy())
        pooled_part.append(layer(r, p, torch.from_numpy(part[m]), 'avg').numpy())
        pooled_rpn.append(layer(r, p, torch.from_numpy(feats[m]), 'max').numpy())
        all_lists.append(collect(voxel_of_points(rois[b, :, :7], pc[m, 1:4], out), out ** 3, mpv))
    pooled_part, pooled_rpn = np.concatenate(pooled_part), np.concatenate(pooled_rpn)
    sums = pooled_part.sum(-1)
    idx = np.stack(np.nonzero(sums), axis=1)
    fake = idx.shape[0] < 3
    if fake:                                                  # fake_sparse_idx (:153-161)
        idx = np.concatenate([np.arange(B * N).reshape(-1, 1), np.zeros((B * N, 3), np.int64)], axis=1)
    sel = tuple(idx[:, k] for k in range(4))
    return dict(coords=idx.astype(np.int32), part_rows=pooled_part[sel], rpn_rows=pooled_rpn[sel], fake=fake, sums=sums,
                lists=all_lists, rows_nonzero=int(np.count_nonzero(sums)))


def margins(rois, point_coords, out):
    """(cell, box): the smallest distance, in cells, of a point inside a RoI of its frame to a voxel face, and of any point
    to a face of a RoI it is not clearly outside of along another axis.  RoIs with a zero extent are skipped (they hold a
    point only within 1e-5 m of their centre plane: see zero_box_clearance)."""
    rois, pc = np.asarray(rois, np.float64), np.asarray(point_coords, np.float64)
    cell, box = np.inf, np.inf
    for b in range(rois.shape[0]):
        p = pc[pc[:, 0] == b, 1:4]
        for r in rois[b]:
            if (r[3:6] <= 0).any():
                continue
            c, s = np.cos(-r[6]), np.sin(-r[6])
            sx, sy = p[:, 0] - r[0], p[:, 1] - r[1]
            loc = np.stack([sx * c - sy * s, sx * s + sy * c, p[:, 2] - r[2]], axis=1)
            u = (loc + r[3:6] / 2) / (r[3:6] / out)            # cells: [0, out] inside
            outside_by = np.maximum(-u, u - out)               # > 0 outside along that axis
            clearly_out = (outside_by > 1e-3).any(axis=1)
            face = np.abs(outside_by)
            near = ~clearly_out
            if near.any():
                box = min(box, face[near].min())
                inner = u[near]
                cell = min(cell, np.abs(inner - np.round(inner)).min())
    return cell, box


def zero_box_clearance(rois, point_coords):
    """the smallest distance (metres, the larger of |z| and the xy radius) of a point to the centre of a RoI with a zero
    extent in its frame"""
    rois, pc = np.asarray(rois, np.float64), np.asarray(point_coords, np.float64)
    best = np.inf
    for b in range(rois.shape[0]):
        p = pc[pc[:, 0] == b, 1:4]
        for r in rois[b]:
            if (r[3:6] <= 0).any() and len(p):
                d = np.maximum(np.abs(p[:, 2] - r[2]), np.hypot(p[:, 0] - r[0], p[:, 1] - r[1]))
                best = min(best, d.min())
    return best
