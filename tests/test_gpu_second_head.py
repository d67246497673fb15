"""GPU: SECONDHead on the device (com_amd/csrc/secondhead.hip, com_amd/hotpath/second_head.py) against fixtures g43 - g46 =
the reference's own second_head.py / second_net_iou.py run on the CPU (tests/golden/make_golden_second_head.py) and against
the fp64 restatement tests/second_head_ref.py (which tests/test_second_head_cpu.py holds to the same fixtures).

Bars: pooled features, loss scalars, rcnn_iou at 1e-4 per element, the project's dense-op bar; gradients at 1e-4 of the largest
element of the fp64 gradient tensor; results stored in bf16 get half a bf16 ulp (2^-8 of the value) on top.  g43 holds its fp64
results rounded to float32, at most 2.5e-7 from the fp64 values: that is taken off the pooling bar.  Point counts, selected
boxes and labels are compared for equality: the fixtures keep every decision 1e-4 away from its threshold, so no element is
left out.  The reference's own f32 values meet the same bars against its fp64 values (tests/test_second_head_cpu.py).

Measured on an MI355X: pooled features within 4.1e-6 of fp64 (G = 7; 3.0e-6 at G = 3; the reference's own f32: 5.8e-6), the
same bits in both layouts; bf16 within 1.1e-6 of half an ulp; G = 16 / C = 1 / the 2 x 2 map within 1.2e-6; loss scalars
within 3.2e-7 (saturated L2, a loss of 283: 1.6e-5), f32 gradients within 4.4e-8 and bf16 gradients within 2.0e-4 of a largest
element of 7.0e-2 (half an ulp there: 2.7e-4); point counts equal; module: batch_cls_preds 1.5e-6, rcnn_iou 4.5e-6, loss 2.8e-9,
parameter gradients 2.9e-6 of each tensor's largest element; post-processing scores within 6.0e-8.  Each test prints its
figures."""
import numpy as np
import pytest
import torch

from com_amd import roiaware_pool3d
from com_amd.hotpath import SECONDHead
from com_amd.hotpath import second_head as SH
from tests import second_head_ref as SR

pytestmark = pytest.mark.gpu
BAR = 1e-4
F32_STORE = 2.5e-7
HALF_ULP_BF16 = 2.0 ** -8


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pool(feats, rois, G, layout):
    geo = SR.POOL_GEOM
    cell = geo['voxel'] * geo['ratio']
    x = feats.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else feats.contiguous()
    return SH.bev_roi_grid_pool(x, rois, G, geo['min_x'], geo['min_y'], cell, cell)


@pytest.mark.parametrize("G", [7, 3])
def test_pool_matches_reference_f64_in_both_layouts(golden, G):
    g = golden("g43_second_pool")
    feats, rois = _cu(g["features"]), _cu(g["rois"])
    want = g[f"pool_f64_G{G}"].astype(np.float64)
    outs = {layout: _pool(feats, rois, G, layout) for layout in ("nchw", "channels_last")}
    for layout, out in outs.items():
        assert out.dtype == torch.float32 and tuple(out.shape) == (26, 70, G, G) and out.is_contiguous()
        err = np.abs(out.cpu().numpy().astype(np.float64) - want).max()
        print(f"[pool G={G} f32 {layout}] max |out - f64| {err:.2e}")
        assert err <= BAR - F32_STORE
    assert torch.equal(outs["nchw"], outs["channels_last"])
    want = g[f"pool_bf16_f64_G{G}"].astype(np.float64)
    b16 = {layout: _pool(feats.bfloat16(), rois, G, layout) for layout in ("nchw", "channels_last")}
    for layout, out in b16.items():
        assert out.dtype == torch.bfloat16 and tuple(out.shape) == (26, 70, G, G)
        d = np.abs(out.float().cpu().numpy().astype(np.float64) - want)
        print(f"[pool G={G} bf16 {layout}] max |out - f64| {d.max():.2e}, largest excess over half an ulp "
              f"{(d - HALF_ULP_BF16 * np.abs(want)).max():.2e}")
        assert (d <= BAR - F32_STORE + HALF_ULP_BF16 * np.abs(want)).all()
    assert torch.equal(b16["nchw"], b16["channels_last"])


@pytest.mark.parametrize("B, N, C, H, W, G", [(1, 1, 1, 13, 11, 7), (1, 3, 70, 5, 4, 16), (2, 2, 65, 2, 2, 2)])
def test_pool_small_and_largest_shapes_against_the_restatement(golden, B, N, C, H, W, G):
    """one RoI of one channel; the largest grid (the 64 KiB tile of the channels-last form); the smallest map and grid; RoIs
    given as a [B, N, 9] tensor (a row stride) with NaN in one row"""
    r = np.random.default_rng(G)
    feats = np.clip(r.normal(0, 1, (B, C, H, W)), -4, 4).astype(np.float32)
    rois = np.zeros((B, N, 9), np.float32)
    rois[..., 0] = r.uniform(-5, -5 + W, (B, N))
    rois[..., 1] = r.uniform(-6, -6 + H, (B, N))
    rois[..., 3:5] = r.uniform(1, 6, (B, N, 2))
    rois[..., 6] = r.uniform(-7, 7, (B, N))
    rois[..., 7:] = 1e30
    geo = SR.POOL_GEOM
    want = SR.roi_grid_pool(feats, rois, G, geo['min_x'], geo['min_y'], 1.0, 1.0)
    outs = [_pool(_cu(feats), _cu(rois), G, layout) for layout in ("nchw", "channels_last")]
    err = np.abs(outs[0].cpu().numpy() - want).max()
    print(f"[pool {B}x{N}x{C} {H}x{W} G={G}] max |out - f64| {err:.2e}")
    assert err <= BAR and torch.equal(outs[0], outs[1]) and tuple(outs[0].shape) == (B * N, C, G, G)
    if N > 1:                                                                # a row that is not finite pools to zeros
        rois[0, 1, 0] = np.nan
        out = _pool(_cu(feats), _cu(rois), G, "channels_last")
        assert not out[1].any() and torch.equal(out[0], outs[0][0])
    assert SH.bev_roi_grid_pool(_cu(feats), _cu(rois[:, :0]), G, -5.0, -6.0, 1.0, 1.0).shape == (0, C, G, G)


def test_pool_reads_strided_roi_views_of_every_shape(golden):
    """views of one [B, 13, 7] tensor whose strides no single row stride describes, or only the frame stride does: one RoI per
    frame (B = 2, N = 1: strides (91, 7, 1)), a run of RoIs per frame, every other RoI, one frame, and a frame repeated by
    expand -- each equals, bit for bit, the rows of the pooling of the whole tensor"""
    g = golden("g43_second_pool")
    feats, rois = _cu(g["features"]), _cu(g["rois"])
    full = _pool(feats, rois, 3, "channels_last").view(2, 13, 70, 3, 3)
    for k in (0, 4, 12):
        view = rois[:, k:k + 1]
        assert tuple(view.shape) == (2, 1, 7) and not view.is_contiguous()
        assert torch.equal(_pool(feats, view, 3, "channels_last").view(2, 1, 70, 3, 3), full[:, k:k + 1])
        assert torch.equal(_pool(feats, view, 3, "nchw").view(2, 1, 70, 3, 3), full[:, k:k + 1])
    assert torch.equal(_pool(feats, rois[:, 2:9], 3, "nchw").view(2, 7, 70, 3, 3), full[:, 2:9])
    assert torch.equal(_pool(feats, rois[:, ::2], 3, "nchw").view(2, 7, 70, 3, 3), full[:, ::2])
    assert torch.equal(_pool(feats[1:], rois[1:, 5:6], 3, "nchw").view(1, 70, 3, 3), full[1, 5:6])
    same = rois[0:1, 3:4].expand(2, 1, 7)                                     # frame stride 0: RoI (0, 3) on both maps
    got = _pool(feats, same, 3, "nchw")
    assert torch.equal(got[0], full[0, 3]) and torch.equal(got[1], _pool(feats[1:], rois[0:1, 3:4], 3, "nchw")[0])
    wide = torch.zeros(2, 13, 9, device="cuda")
    wide[..., :7] = rois
    assert torch.equal(_pool(feats, wide[:, 6:7, :8], 3, "nchw").view(2, 1, 70, 3, 3), full[:, 6:7])


def _loss_and_grad(x, t, kind, weight):
    x = x.clone().requires_grad_(True)
    out = SH.iou_loss(x, t, kind, weight)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2,) and out.is_cuda
    (d,) = torch.autograd.grad(out[0] * 1.0, [x])
    return out.detach(), d


@pytest.mark.parametrize("kind", list(SR.LOSS_WEIGHTS))
def test_loss_matches_reference_f64(golden, kind):
    g = golden("g44_second_loss")
    weight = SR.LOSS_WEIGHTS[kind]
    for case in SR.LOSS_CASES:
        x, t = _cu(g[f"{case}_logits"]), _cu(g[f"{case}_labels"])
        l64, d64 = float(g[f"{kind}_{case}_f64_loss"]), g[f"{kind}_{case}_f64_dlogits"].astype(np.float64)
        top = np.abs(d64).max()
        for dt in ((torch.float32, torch.bfloat16) if case == 'bf16' else (torch.float32,)):
            out, d = _loss_and_grad(x.to(dt), t, kind, weight)
            assert d.dtype == dt and tuple(d.shape) == (96, 1)
            dd = np.abs(d.float().cpu().numpy().astype(np.float64) - d64)
            slack = HALF_ULP_BF16 * np.abs(d64) if dt == torch.bfloat16 else 0.0
            print(f"[loss {kind} {case} {dt}] |loss - f64| {abs(float(out[0]) - l64):.2e}, gradient off by {dd.max():.2e} "
                  f"(largest element {top:.2e})")
            assert abs(float(out[0]) - l64) <= BAR and int(out[1]) == int((g[f"{case}_labels"] >= 0).sum())
            assert (dd <= BAR * top + slack).all()
            if case == 'all_ignored':
                assert float(out[0]) == 0 and int(out[1]) == 0 and not d.any()
            out2, d2 = _loss_and_grad(x.to(dt), t, kind, weight)             # a fixed summation order
            assert torch.equal(out, out2) and torch.equal(d, d2)


@pytest.mark.parametrize("kind", list(SR.LOSS_WEIGHTS))
@pytest.mark.parametrize("n", [1, 300])
def test_loss_one_row_and_a_partial_workgroup_against_the_restatement(kind, n):
    """n = 300: more than one wave and a partial workgroup in the backward; the logits are a column of a wider tensor (a row
    stride of 3) and the incoming gradient is not 1"""
    r = np.random.default_rng(n)
    wide = r.normal(0, 2, (n, 3)).astype(np.float32)
    t = r.uniform(0, 1, n).astype(np.float32)
    t[3::7] = -1.0
    loss, valid, d = SR.iou_loss(wide[:, 1], t, kind, 0.8)
    assert valid == n - len(t[3::7])
    w = _cu(wide).requires_grad_(True)
    out = SH.iou_loss(w[:, 1:2], _cu(t), kind, 0.8)
    (dw,) = torch.autograd.grad(out[0] * 2.5, [w])
    dw = dw.cpu().numpy()
    print(f"[loss {kind} n={n}] |loss - f64| {abs(float(out[0]) - loss):.2e}, gradient off by {np.abs(dw[:, 1] - 2.5 * d).max():.2e}")
    assert abs(float(out[0]) - loss) <= BAR and int(out[1]) == valid
    assert np.abs(dw[:, 1] - 2.5 * d).max() <= BAR * np.abs(2.5 * d).max()
    assert not dw[:, 0].any() and not dw[:, 2].any()


def test_point_counts_equal_points_in_boxes_cpu(golden):
    g = golden("g46_second_postproc")
    pts, boxes = g["points"], g["boxes"]
    counts = SH.points_in_boxes_count(_cu(pts), _cu(boxes))
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (2, 24)
    want = np.stack([roiaware_pool3d.points_in_boxes_cpu(pts[pts[:, 0] == b][:, 1:4], boxes[b]).sum(axis=1) for b in range(2)])
    print(f"[counts] {counts.cpu().numpy().tolist()}")
    np.testing.assert_array_equal(counts.cpu().numpy(), want)
    np.testing.assert_array_equal(want, g["counts"])
    assert want.max() >= 60 and (want == 0).any()
    assert torch.equal(SH.points_in_boxes_count(_cu(pts), _cu(boxes)), counts)              # zeroed by the op, order-free
    only0 = SH.points_in_boxes_count(_cu(pts[pts[:, 0] == 0]), _cu(boxes))                  # a frame with no points
    assert torch.equal(only0[0], counts[0]) and not only0[1].any()
    assert tuple(SH.points_in_boxes_count(_cu(pts), _cu(boxes[:, :0])).shape) == (2, 0)     # K = 0
    assert not SH.points_in_boxes_count(_cu(pts[:0]), _cu(boxes)).any()                     # P = 0
    many = np.tile(boxes, (1, 6, 1))                                                        # 144 boxes: two passes of the LDS chunk
    got = SH.points_in_boxes_count(_cu(pts), _cu(many)).cpu().numpy()
    np.testing.assert_array_equal(got, np.tile(want, (1, 6)))


def _head(g45, **kw):
    head = SECONDHead(input_channels=6, model_cfg=SR.model_cfg(), num_class=1, **kw)
    head.load_state_dict({str(k): torch.from_numpy(g45["sd::" + str(k)]) for k in g45["sd_keys"]}, strict=True)
    return head.cuda()


def _scene(g30, g45):
    return {'batch_size': 3, 'rois': _cu(g30["A_rois"]), 'roi_scores': _cu(g30["A_roi_scores"]), 'roi_labels': _cu(g30["A_roi_labels"]),
            'gt_boxes': _cu(g30["A_gt_boxes"]), 'spatial_features_2d': _cu(g45["features"])}


def test_module_eval_forward_matches_reference(golden):
    g30, g45 = golden("g30_roi_overlaps"), golden("g45_second_module")
    head = _head(g45).eval()
    bd = _scene(g30, g45)
    bd['dataset_cfg'] = SR.dataset_cfg(SR.MODULE_RANGE, SR.MODULE_VOXEL)
    with torch.no_grad():
        out = head(bd)
    assert tuple(out['batch_cls_preds'].shape) == (3, 96, 1) and out['batch_box_preds'] is bd['rois']
    assert out['cls_preds_normalized'] is False
    err = np.abs(out['batch_cls_preds'].cpu().numpy() - g45["eval_f64_batch_cls_preds"]).max()
    print(f"[module eval] max |batch_cls_preds - f64| {err:.2e}")
    assert err <= BAR
    kw = _head(g45, point_cloud_range=SR.MODULE_RANGE, voxel_size=SR.MODULE_VOXEL).eval()    # geometry from the constructor
    with torch.no_grad():
        assert torch.equal(kw(_scene(g30, g45))['batch_cls_preds'], out['batch_cls_preds'])


def test_module_train_forward_loss_and_gradients_match_reference(golden):
    g30, g31, g45 = golden("g30_roi_overlaps"), golden("g31_roi_targets"), golden("g45_second_module")
    head = _head(g45, point_cloud_range=SR.MODULE_RANGE, voxel_size=SR.MODULE_VOXEL).train()
    bd = _scene(g30, g45)
    td = head.assign_targets(bd, sampled_inds=_cu(g31["A_sampled_inds"]))
    # (the soft labels come from the device IoU: tests/test_gpu_roi_head.py holds them to g31 at the IoU bar)
    np.testing.assert_allclose(td['rcnn_cls_labels'].cpu().numpy(), g31["A_rcnn_cls_labels"], atol=BAR, rtol=0)
    bd.update(rois=td['rois'], roi_labels=td['roi_labels'], roi_targets_dict=td)
    head(bd)
    assert head.forward_ret_dict is td and tuple(td['rcnn_iou'].shape) == (96, 1)
    loss, tb = head.get_loss()
    assert set(tb) == {'rcnn_loss_iou', 'rcnn_loss'} and all(v.is_cuda and v.dim() == 0 and not v.requires_grad for v in tb.values())
    loss.backward()
    e_iou = np.abs(td['rcnn_iou'].detach().cpu().numpy() - g45["train_f64_rcnn_iou"]).max()
    e_loss = abs(float(loss) - float(g45["train_f64_loss"]))
    print(f"[module train] rcnn_iou off by {e_iou:.2e}, loss by {e_loss:.2e}")
    assert e_iou <= BAR and e_loss <= BAR and float(tb['rcnn_loss']) == float(loss) == float(tb['rcnn_loss_iou'])
    worst = 0.0
    for k, p in head.named_parameters():
        want = g45["train_f64_grad::" + k]
        rel = np.abs(p.grad.cpu().numpy() - want).max() / np.abs(want).max()
        worst = max(worst, rel)
        assert rel <= BAR, (k, rel)
    print(f"[module train] parameter gradients within {worst:.2e} of the largest element of each tensor")


@pytest.mark.parametrize("score_type", SR.SCORE_TYPES)
def test_post_processing_matches_reference(golden, score_type):
    g = golden("g46_second_postproc")
    bd = {'batch_size': 2, 'batch_box_preds': _cu(g["boxes"]), 'batch_cls_preds': _cu(g["iou_logits"]), 'roi_scores': _cu(g["cls_logits"]),
          'roi_labels': _cu(g["labels"]), 'has_class_labels': True, 'cls_preds_normalized': False, 'points': _cu(g["points"])}
    pred = SH.post_processing(bd, SR.post_process_cfg(score_type), SR.CLASS_NAMES)
    assert len(pred) == 2
    for b in range(2):
        tag = f"{score_type or 'absent'}_{b}"
        got = {k: v.cpu().numpy() for k, v in pred[b].items()}
        assert set(got) == {'pred_boxes', 'pred_scores', 'pred_labels', 'pred_cls_scores', 'pred_iou_scores'}
        np.testing.assert_array_equal(got['pred_boxes'], g["boxes"][b][g[f"{tag}_selected"]])            # the same boxes, in order
        np.testing.assert_array_equal(got['pred_labels'], g[f"{tag}_pred_labels"])
        errs = [np.abs(got[k] - g[f"{tag}_{k}"]).max() for k in ('pred_scores', 'pred_cls_scores', 'pred_iou_scores')]
        print(f"[postproc {tag}] {len(got['pred_labels'])} boxes, scores off by {max(errs):.2e}")
        assert max(errs) <= 1e-6


def _step(head, bd, uniforms=None):
    td = head.assign_targets(bd, uniforms=uniforms)
    head(dict(bd, rois=td['rois'], roi_labels=td['roi_labels'], roi_targets_dict=td))
    loss, tb = head.get_loss()
    d_iou, *d_params = torch.autograd.grad(loss, [td['rcnn_iou']] + list(head.parameters()))
    return loss.detach(), td['rcnn_iou'].detach(), d_iou, tb, td['sampled_inds'], d_params


def test_training_step_is_capturable(golden):
    """assign_targets (own generator) + pooling + the FC stack + get_loss + backward in ONE graph with fixed shapes, replayed
    twice; nothing is read back (a read-back fails the capture).  Of a replay, everything this project's kernels write --
    the sampled indices, rcnn_iou, the loss and its gradient with respect to rcnn_iou -- equals, bit for bit, an eager run fed
    the uniforms the replay drew, and so do the gradients of the BatchNorm parameters and the conv bias.  The weight gradients
    of the five Conv1d layers are held to the gradient bar only: torch's convolution weight-gradient kernels do not reproduce
    their own bits from one EAGER run to the next on the same inputs (measured on an MI355X: two eager runs differ by
    1.8e-8 .. 8.9e-8 of the largest element in those five tensors and in no other; a replay differs from an eager run by the
    same amounts).  The test prints both sets of figures."""
    g30, g45 = golden("g30_roi_overlaps"), golden("g45_second_module")
    head = _head(g45, point_cloud_range=SR.MODULE_RANGE, voxel_size=SR.MODULE_VOXEL).train()
    layer = head.proposal_target_layer.manual_seed(9)
    bd = _scene(g30, g45)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(head, bd)                                                       # warm-up: tables, status word, library workspaces
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    drawn = []
    draw = layer.draw_uniforms
    layer.draw_uniforms = lambda *a: drawn.append(draw(*a)) or drawn[-1]
    graph = torch.cuda.CUDAGraph()
    graph.register_generator_state(layer.generator)
    with torch.cuda.graph(graph):
        out = _step(head, bd)
    assert len(drawn) == 1
    runs = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        u = drawn[0].clone()
        got = [out[0].clone(), out[1].clone(), out[2].clone(), out[4].clone()] + [p.clone() for p in out[5]]
        eager = _step(head, bd, uniforms=u)
        assert torch.equal(got[3], eager[4]) and torch.equal(got[1], eager[1])
        assert torch.equal(got[0], eager[0]) and torch.equal(got[2], eager[2])
        again = _step(head, bd, uniforms=u)                                   # eager against eager: torch's own run-to-run figure
        names = [k for k, _ in head.named_parameters()]
        rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())  # noqa: E731
        off = {k: rel(a, b) for k, a, b in zip(names, got[4:], eager[5]) if not torch.equal(a, b)}
        off_eager = {k: rel(a, b) for k, a, b in zip(names, again[5], eager[5]) if not torch.equal(a, b)}
        print(f"[capture] parameter gradients, replay against eager, not bit-equal: {off}")
        print(f"[capture] parameter gradients, eager against eager, not bit-equal: {off_eager}")
        conv_w = {f"{k}.weight" for k, m in head.named_modules() if isinstance(m, torch.nn.Conv1d)}
        assert set(off) <= conv_w and all(v <= BAR for v in off.values())     # every other gradient: bit for bit
        runs.append(got)
    assert not torch.equal(runs[0][3], runs[1][3])                                # philox moves on between replays
    assert all(v.is_cuda for v in out[3].values()) and torch.isfinite(runs[1][0])
    assert layer.check_status() == 0
