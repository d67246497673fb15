"""GPU: com_amd.roiaware_pool3d (com_amd/csrc/roiaware.hip) against fixtures g26 / g29 = the reference's
roiaware_pool3d_utils run over the numpy transcription of its natives (tests/golden/make_golden_point_head.py).

Boundary band: device and numpy cosf may differ in the last place, so a point is left out of a comparison only if its
|local_x| or |local_y| lies within 1e-5 m of d / 2 + MARGIN for some box whose z test it passes; that may leave out at
most 0.1 % of the points (asserted), everything else must be equal.  The pooling fixture holds no point in the band and
none within 1e-4 of a voxel boundary, so its lists and argmax must be equal everywhere."""
import numpy as np
import pytest
import torch

from com_amd import roiaware_pool3d as RP
from tests import point_head_ref as PR

pytestmark = pytest.mark.gpu
BAND_CAP = 1e-3


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _outside_band(boxes, pts):
    band = np.stack([PR.band_mask(boxes[b], pts[b], PR.MARGIN_GPU) for b in range(boxes.shape[0])])
    print(f"[band] {int(band.sum())} of {band.size} points left out")
    assert band.mean() <= BAND_CAP
    return ~band


@pytest.mark.parametrize("tag", ["single", "batch"])
def test_points_in_boxes_gpu_matches_fixture(golden, tag):
    g = golden("g26_points_in_boxes")
    boxes, pts = g[f"{tag}_boxes"], g[f"{tag}_pts"]
    if tag == "single":
        boxes, pts = boxes[None], pts[None]
    out = RP.points_in_boxes_gpu(_cu(pts), _cu(boxes))
    assert out.dtype == torch.int32 and tuple(out.shape) == pts.shape[:2]
    got, ref = out.cpu().numpy(), g[f"{tag}_idx_gpu"]
    keep = _outside_band(boxes, pts)
    print(f"[points_in_boxes {tag}] B = {boxes.shape[0]}: mismatches outside the band {int((got != ref)[keep].sum())}, "
          f"inside {int((got != ref)[~keep].sum())}; {int((ref >= 0).sum())} points in a box")
    np.testing.assert_array_equal(got[keep], ref[keep])


def test_points_in_boxes_gpu_has_no_cap_on_the_number_of_boxes(golden):
    """300 boxes per frame (three LDS chunks): 200 far-away boxes in front of the fixture's rows shift every index by 200"""
    g = golden("g26_points_in_boxes")
    boxes, pts = g["batch_boxes"], g["batch_pts"]
    far = np.tile(np.array([500.0, 500.0, 0.0, 4.0, 2.0, 1.5, 0.3], np.float32), (boxes.shape[0], 200, 1))
    tail = np.zeros((boxes.shape[0], 68, 7), np.float32)
    got = RP.points_in_boxes_gpu(_cu(pts), _cu(np.concatenate([far, boxes, tail], 1))).cpu().numpy()
    ref = np.where(g["batch_idx_gpu"] >= 0, g["batch_idx_gpu"] + 200, -1)
    keep = _outside_band(boxes, pts)
    np.testing.assert_array_equal(got[keep], ref[keep])


def test_points_in_boxes_gpu_160k_points_and_first_match():
    """one 160 k-point frame against 64 boxes, a third of them overlapping their predecessor: the index is the LOWEST box
    that contains the point (membership per box from the transcription), and doubling the box list changes nothing"""
    r = np.random.default_rng(160)
    n = 64
    boxes = np.zeros((n, 7), np.float32)
    boxes[:, 0:2] = r.uniform(-60, 60, (n, 2))
    boxes[:, 2] = r.uniform(-1, 1, n)
    boxes[:, 3:6] = r.uniform(0.5, 6.0, (n, 3))
    boxes[:, 6] = r.uniform(-2 * np.pi, 2 * np.pi, n)
    boxes[2::3, 0:3] = boxes[1::3][:boxes[2::3].shape[0], 0:3] + 0.3
    near = boxes[r.integers(0, n, 60000), :3] + r.uniform(-3, 3, (60000, 3))
    far = np.concatenate([r.uniform(-75, 75, (100000, 2)), r.uniform(-2, 4, (100000, 1))], 1)
    pts = np.concatenate([near, far]).astype(np.float32)
    member = np.stack([PR.check_pt_in_box3d(pts, b, PR.MARGIN_GPU)[0] for b in boxes])
    want = np.where(member.any(0), member.argmax(0), -1)
    keep = _outside_band(boxes[None], pts[None])[0]
    got = RP.points_in_boxes_gpu(_cu(pts)[None], _cu(boxes)[None])[0].cpu().numpy()
    multi = member.sum(0) > 1
    print(f"[160k] {int(member.any(0).sum())} points in a box, {int(multi.sum())} in more than one; mismatches outside the band "
          f"{int((got != want)[keep].sum())}")
    assert multi.sum() > 100
    np.testing.assert_array_equal(got[keep], want[keep])
    twice = RP.points_in_boxes_gpu(_cu(pts)[None], _cu(np.concatenate([boxes, boxes]))[None])[0].cpu().numpy()
    np.testing.assert_array_equal(twice, got)
    # reversed box order: a point in several boxes now reports the mirror of its HIGHEST box
    rev = RP.points_in_boxes_gpu(_cu(pts)[None], _cu(boxes[::-1])[None])[0].cpu().numpy()
    last = np.where(member.any(0), n - 1 - member[::-1].argmax(0), -1)
    np.testing.assert_array_equal(np.where(rev >= 0, n - 1 - rev, -1)[keep], last[keep])


def _dense_restatement(feat, lists, argmax, method):
    """the pooled features as plain torch indexing of `feat` through the fixture's lists / argmax (differentiable)"""
    c = feat.shape[1]
    if method == "max":
        am = argmax.long()
        picked = feat[am.clamp(min=0), torch.arange(c, device=feat.device)]
        return torch.where(am >= 0, picked, torch.zeros_like(picked))
    cnt = lists[..., 0].long()
    idx = lists[..., 1:].long()
    mask = torch.arange(idx.shape[-1], device=feat.device) < cnt.unsqueeze(-1)
    total = (feat[idx] * mask.unsqueeze(-1).to(feat.dtype)).sum(-2)
    return total / cnt.clamp(min=1).unsqueeze(-1).to(feat.dtype)


@pytest.mark.parametrize("tag", ["full", "cap"])
@pytest.mark.parametrize("method", ["max", "avg"])
def test_roiaware_pool3d_matches_fixture(golden, tag, method):
    g = golden("g29_roiaware_pool")
    size, mpv = tuple(int(v) for v in g[f"{tag}_size"][:3]), int(g[f"{tag}_size"][3])
    rois, pts = _cu(g["rois"]), _cu(g["pts"])
    feat = _cu(g["feat"]).requires_grad_(True)
    pool = RP.RoIAwarePool3d(out_size=size, max_pts_each_voxel=mpv)
    y = pool(rois, pts, feat, pool_method=method)
    assert tuple(y.shape) == (rois.shape[0],) + size + (feat.shape[1],) and y.dtype == torch.float32
    lists, argmax = y.grad_fn.roiaware_pool3d_for_backward[:2]
    np.testing.assert_array_equal(lists.cpu().numpy(), g[f"{tag}_lists"])                   # order, cap, count in slot 0
    ref = g[f"{tag}_{method}_pooled"]
    if method == "max":
        np.testing.assert_array_equal(argmax.cpu().numpy(), g[f"{tag}_argmax"])
        am = g[f"{tag}_argmax"]
        gathered = np.where(am >= 0, g["feat"][np.maximum(am, 0), np.arange(g["feat"].shape[1])], 0).astype(np.float32)
        np.testing.assert_array_equal(y.detach().cpu().numpy(), gathered)                   # exactly the gathered inputs
        np.testing.assert_array_equal(gathered, ref)
    else:
        err = np.abs(y.detach().cpu().numpy() - ref).max() / np.abs(ref).max()
        print(f"[pool {tag} avg] max |y - reference| / max |reference| = {err:.2e}")
        np.testing.assert_allclose(y.detach().cpu().numpy(), ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())
    grad_out = _cu(g[f"{tag}_grad_out"])
    (grad_in,) = torch.autograd.grad(y, feat, grad_out)
    ref_g = g[f"{tag}_{method}_grad_in"]
    print(f"[pool {tag} {method}] max |grad_in - fixture| = {np.abs(grad_in.cpu().numpy() - ref_g).max():.2e}")
    np.testing.assert_allclose(grad_in.cpu().numpy(), ref_g, rtol=1e-5, atol=1e-5)
    feat64 = _cu(g["feat"]).double().requires_grad_(True)
    dense = _dense_restatement(feat64, _cu(g[f"{tag}_lists"]), _cu(g[f"{tag}_argmax"]), method)
    (dense_g,) = torch.autograd.grad(dense, feat64, grad_out.double())
    np.testing.assert_allclose(grad_in.cpu().numpy(), dense_g.cpu().numpy(), rtol=1e-5, atol=1e-5)


def test_roiaware_pool3d_int_out_size_and_no_rois(golden):
    g = golden("g29_roiaware_pool")
    rois, pts, feat = _cu(g["rois"]), _cu(g["pts"]), _cu(g["feat"])
    y = RP.RoIAwarePool3d(out_size=2, max_pts_each_voxel=4)(rois, pts, feat, pool_method="max")
    np.testing.assert_array_equal(y.cpu().numpy(), g["cap_max_pooled"])
    y0 = RP.RoIAwarePool3d(out_size=3)(rois[:0], pts, feat, pool_method="avg")
    assert tuple(y0.shape) == (0, 3, 3, 3, feat.shape[1])
