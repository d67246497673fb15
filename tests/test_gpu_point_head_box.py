"""GPU: PointHeadBox, PointIntraPartOffsetHead and PointResidualCoder on the device (com_amd/csrc/roiaware.hip,
com_amd/hotpath/point_head.py) against fixtures g47 - g49 = the reference's own classes run on the CPU over the numpy
transcription of points_in_boxes_gpu (tests/golden/make_golden_point_head_box.py), and their fp64 restatements
(tests/point_head_box_ref.py).

Labels: as in test_gpu_point_head.py, equal outside the boundary band (at most 0.1 % of the points, asserted).  Box and part
labels, the loss terms, the gradients and the decoded boxes: the per-element 1e-4 bar of the dense ops against fp64 (loss
terms relative, gradients relative to the largest magnitude of their tensor, headings modulo 2 pi; README / DESIGN.md
section 3); the reference's own fp32 values must lie within the same bar.

Measured on an MI355X (ours / the reference's own fp32, both against fp64): labels equal for all 8 192 points of every head
(1 point in the band, it agrees too); box labels 2.1e-7 / 9.5e-8 with mean sizes, 1.5e-7 / 6.0e-8 without; part labels
1.1e-7 / 1.1e-7; loss terms cls 1.8e-8 / 4.9e-8, box 1.4e-8 / 9.2e-8, part 2.9e-8 / 6.0e-8, total 1.4e-8 / 7.7e-9; gradients
d cls 8.1e-7 / 7.1e-7, d box 7.9e-8 / 4.4e-8, d part 1.6e-7 / 1.9e-7; decoded boxes 2.1e-6 / 2.1e-6 (coordinates up to
40 m: one float32 ulp is 3.8e-6)."""
import numpy as np
import pytest
import torch

from com_amd import _lib as L
from com_amd.hotpath import PointHeadBox, PointIntraPartOffsetHead, PointResidualCoder
from com_amd.hotpath import point_head as PH
from tests import point_head_box_ref as BR
from tests import point_head_ref as PR

pytestmark = pytest.mark.gpu
BAND_CAP = 1e-3
BAR = 1e-4
MEAN = BR.KITTI_MEAN_SIZE


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def targets(golden):
    """g27's inputs, the band, and g47's label rows scattered back to all N points (computed once, never changed)"""
    g, t = golden("g27_point_head_targets"), golden("g47_point_head_box_targets")
    pc, gt = g["point_coords"], g["gt_boxes"]
    ext = gt.copy()
    ext[..., 3:6] += g["extra_width"].astype(np.float32)
    band = np.zeros(pc.shape[0], bool)
    for b in range(gt.shape[0]):
        m = pc[:, 0] == b
        band[m] = PR.band_mask(gt[b, :, :7], pc[m, 1:], PR.MARGIN_GPU) | PR.band_mask(ext[b, :, :7], pc[m, 1:], PR.MARGIN_GPU)
    print(f"[band] {int(band.sum())} of {band.size} points left out")
    assert band.mean() <= BAND_CAP
    full = {}
    for tag in ("box_mean", "box_nomean", "part"):
        for prec in ("f32", "f64"):
            a = np.zeros((pc.shape[0], t[f"{tag}_{prec}"].shape[1]), np.float64)
            a[t["fg_idx"]] = t[f"{tag}_{prec}"]
            a.setflags(write=False)
            full[f"{tag}_{prec}"] = a
    return dict(pc=pc, gt=gt, keep=~band, labels={1: g["labels_c1"].astype(np.int64), 3: g["labels_c3"].astype(np.int64)}, **full)


HEADS = {
    "box": (PointHeadBox, 3, dict(name='PointHeadBox'), "box_mean", None),
    "box_c1": (PointHeadBox, 1, dict(name='PointHeadBox'), "box_mean", None),
    "box_nomean": (PointHeadBox, 3, dict(name='PointHeadBox', use_mean_size=False), "box_nomean", None),
    "part": (PointIntraPartOffsetHead, 3, dict(name='PointIntraPartOffsetHead', box=False, part=True), None, "part"),
    "both": (PointIntraPartOffsetHead, 3, dict(name='PointIntraPartOffsetHead', box=True, part=True), "box_mean", "part"),
}


def _head(which, **kw):
    cls, num_class, c, _, _ = HEADS[which]
    return cls(num_class, 32, BR.head_cfg(**c), **kw).cuda()


def _check_rows(what, got, ref32, ref64, labels_got, rows):
    """label rows `got` (tensor [N, w]) on the compared foreground rows against fp64, zero elsewhere"""
    got = got.cpu().numpy().astype(np.float64)
    assert (got[labels_got <= 0] == 0).all(), f"{what}: a row that is not foreground is not zero"
    e = np.abs(got - ref64)[rows].max()
    r = np.abs(ref32 - ref64)[rows].max()
    print(f"[{what}] ours vs fp64 {e:.2e}; the reference's fp32 vs fp64 {r:.2e} ({int(rows.sum())} rows)")
    assert r < BAR                                                               # the bar is fair
    assert e < BAR


@pytest.mark.parametrize("which", list(HEADS))
def test_targets_match_reference_fixture(targets, which):
    _, num_class, _, box_tag, part_tag = HEADS[which]
    head = _head(which)
    td = head.assign_targets({'point_coords': _cu(targets["pc"]), 'gt_boxes': _cu(targets["gt"])})
    labels = td['point_cls_labels']
    n = targets["pc"].shape[0]
    assert labels.dtype == torch.int64 and tuple(labels.shape) == (n,)
    got, ref, keep = labels.cpu().numpy(), targets["labels"][num_class], targets["keep"]
    print(f"[labels {which}] mismatches outside the band {int((got != ref)[keep].sum())}, inside {int((got != ref)[~keep].sum())}")
    np.testing.assert_array_equal(got[keep], ref[keep])
    num_pos = td['point_pos_num']
    assert num_pos.is_cuda and num_pos.dtype == torch.int32 and int(num_pos[0]) == int((got > 0).sum())
    rows = keep & (ref > 0) & (got > 0)
    if box_tag is None:
        assert td['point_box_labels'] is None
    else:
        assert td['point_box_labels'].dtype == torch.float32 and tuple(td['point_box_labels'].shape) == (n, 8)
        _check_rows(f"box labels {which}", td['point_box_labels'], targets[box_tag + "_f32"], targets[box_tag + "_f64"], got, rows)
    if part_tag is None:
        assert td['point_part_labels'] is None
    else:
        assert td['point_part_labels'].dtype == torch.float32 and tuple(td['point_part_labels'].shape) == (n, 3)
        _check_rows(f"part labels {which}", td['point_part_labels'], targets["part_f32"], targets["part_f64"], got, rows)


def _assign(pc, gt, box=True, part=True, num_class=3):
    """(labels, box labels, part labels, num_pos) as numpy through the module-level entry, KITTI mean sizes"""
    lb, bx, pt, num_pos = PH.assign_targets_full(_cu(pc), _cu(gt), BR.EXTRA_WIDTH, num_class,
                                                 mean_size=_cu(np.asarray(MEAN, np.float32)) if box else None,
                                                 ret_box_labels=box, ret_part_labels=part)
    torch.cuda.synchronize()
    return lb.cpu().numpy(), None if bx is None else bx.cpu().numpy(), None if pt is None else pt.cpu().numpy(), int(num_pos[0])


def _same(targets, got, sel, rows):
    """outputs of _assign for the points `sel` (indices into the fixture's points), compared on the rows `rows` of them"""
    lb, bx, pt, num_pos = got
    ref = targets["labels"][3][sel]
    np.testing.assert_array_equal(lb[rows], ref[rows])
    assert num_pos == int((lb > 0).sum())
    fg = rows & (ref > 0) & (lb > 0)
    for arr, tag in ((bx, "box_mean"), (pt, "part")):
        if arr is not None:
            assert (arr[lb <= 0] == 0).all()
            assert np.abs(arr - targets[tag + "_f64"][sel])[fg].max() < BAR


def test_targets_unsorted_points_many_boxes_foreign_rows_and_odd_sizes(targets):
    """the shapes at which the kernel can still go wrong: the points permuted (a workgroup walks several frames); 300 GT rows
    per frame with the real rows at 200... and 254... (the winning box lies in the second and third LDS chunk: its row
    index must survive the chunk loop); rows whose bs_idx names no frame; N not a multiple of 256; N = 0; M = 0; each output alone"""
    pc, gt, keep = targets["pc"], targets["gt"], targets["keep"]
    n = pc.shape[0]
    everything = np.arange(n)
    perm = np.random.default_rng(5).permutation(n)
    _same(targets, _assign(pc[perm], gt), perm, keep[perm])
    big = np.zeros((gt.shape[0], 300, 8), np.float32)
    big[:, 200:205] = gt[:, :5]                                                  # the real rows in their order: second chunk ...
    big[:, 254:254 + gt.shape[1] - 5] = gt[:, 5:]                                # ... and across 256 into the third
    big[:, 10:150] = [500.0, 500.0, 0.0, 4.0, 2.0, 1.5, 0.3, 2]
    big[:, 290:296] = gt[:, :6]                                                  # later copies of real boxes: never the first match
    win = BR.winning_boxes(pc, gt)
    assert ((win >= 0) & (win < 5)).any() and (win >= 7).any()                   # winners in both chunks
    _same(targets, _assign(pc, big), everything, keep)
    foreign = pc.copy()
    foreign[::7, 0] = 9.0
    foreign[3::7, 0] = 0.5
    foreign[5::7, 0] = -1.0
    moved = foreign[:, 0] != pc[:, 0]
    got = _assign(foreign, gt)
    assert (got[0][moved] == 0).all() and (got[1][moved] == 0).all() and (got[2][moved] == 0).all()
    _same(targets, got, everything, keep & ~moved)
    odd = n - 37
    _same(targets, _assign(pc[:odd], gt), everything[:odd], keep[:odd])
    _same(targets, _assign(pc, gt, box=False), everything, keep)                 # part-only
    _same(targets, _assign(pc, gt, part=False), everything, keep)                # box-only
    lb, bx, pt, num_pos = _assign(pc[:0], gt)
    assert lb.shape == (0,) and bx.shape == (0, 8) and pt.shape == (0, 3) and num_pos == 0
    lb, bx, pt, num_pos = _assign(pc, gt[:, :0])
    assert (lb == 0).all() and (bx == 0).all() and (pt == 0).all() and num_pos == 0


@pytest.fixture(scope="module")
def loss_case(golden):
    l = golden("g48_point_head_box_loss")
    n = l["labels"].shape[0]
    box_labels = np.zeros((n, 8), np.float32)
    box_labels[l["pos_idx"]] = l["box_labels_pos"]
    part_labels = np.zeros((n, 3), np.float32)
    part_labels[l["pos_idx"]] = l["part_labels_pos"]
    return dict(l=l, labels=l["labels"].astype(np.int64), box_labels=box_labels, part_labels=part_labels)


def _ret_dict(case, preds, labels=None, with_count=True):
    labels = _cu(case["labels"]) if labels is None else labels
    f = {'point_cls_labels': labels, 'point_cls_preds': preds[0], 'point_box_preds': preds[1], 'point_part_preds': preds[2],
         'point_box_labels': _cu(case["box_labels"]), 'point_part_labels': _cu(case["part_labels"])}
    if with_count:
        f['point_pos_num'] = (labels > 0).sum().to(torch.int32).reshape(1)
    return f


# which of (cls, box, part) a head has, and the key of its gradient in the fixture
TERMS = {"both": (0, 1, 2), "box": (0, 1), "part": (0, 2)}
GRAD_KEYS = ("dcls", "dbox", "dpart")
TB_KEYS = ("point_loss_cls", "point_loss_box", "point_loss_part")


@pytest.mark.parametrize("which", ["both", "box", "part"])
def test_loss_and_gradients_against_fp64(loss_case, which):
    """the three-branch head, the box head without part branch, the part head without box branch"""
    l = loss_case["l"]
    head = _head(which)
    x = [_cu(l[k]).requires_grad_(True) for k in ("cls_preds", "box_preds", "part_preds")]
    head.forward_ret_dict = _ret_dict(loss_case, x)
    loss, tb = head.get_loss()
    mine = [x[k] for k in TERMS[which]]
    grads = torch.autograd.grad(loss, mine)
    s64, s32 = l["f64_scalars"], l["f32_scalars"]
    # tb_dict: device scalars (the reference calls .item() on each)
    assert set(tb) == {'point_pos_num'} | {TB_KEYS[k] for k in TERMS[which]}
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 for v in tb.values())
    assert float(tb['point_pos_num']) == s64[4]
    want = sum(s64[1 + k] for k in TERMS[which])
    pairs = [("total", float(loss.detach()), want, sum(s32[1 + k] for k in TERMS[which]))]
    pairs += [(TB_KEYS[k], float(tb[TB_KEYS[k]]), s64[1 + k], s32[1 + k]) for k in TERMS[which]]
    for name, got, w64, w32 in pairs:
        e, r = abs(got - w64) / abs(w64), abs(w32 - w64) / abs(w64)
        print(f"[loss {which}] {name}: ours vs fp64 {e:.2e}; the reference's fp32 vs fp64 {r:.2e}")
        assert r < BAR and e < BAR
    labels = loss_case["labels"]
    for k, d in zip(TERMS[which], grads):
        d64, d32 = l["f64_" + GRAD_KEYS[k]], l["f32_" + GRAD_KEYS[k]]
        d = d.cpu().numpy()
        e, r = np.abs(d - d64).max() / np.abs(d64).max(), np.abs(d32 - d64).max() / np.abs(d64).max()
        print(f"[loss {which}] {GRAD_KEYS[k]}: ours vs fp64 {e:.2e}; the reference's fp32 vs fp64 {r:.2e}")
        assert r < BAR and e < BAR
        assert (d[labels < 0] == 0).all() if k == 0 else (d[labels <= 0] == 0).all()
        if k == 1:
            assert (d[np.isnan(loss_case["box_labels"])] == 0).all() and np.isnan(loss_case["box_labels"]).sum() >= 5
    # the separate methods read the same call's scalars; labels without a stored count give the same loss
    for k in TERMS[which]:
        term, tbk = getattr(head, ("get_cls_layer_loss", "get_box_layer_loss", "get_part_layer_loss")[k])()
        assert torch.equal(term.detach(), tb[TB_KEYS[k]]) and TB_KEYS[k] in tbk
    head.forward_ret_dict = _ret_dict(loss_case, x, with_count=False)
    assert torch.equal(head.get_loss()[0], loss)
    # an upstream factor scales all the gradients
    loss2, _ = head.get_loss()
    for d2, d in zip(torch.autograd.grad(loss2 * 3.0, mine), grads):
        np.testing.assert_allclose(d2.cpu().numpy(), 3.0 * d.cpu().numpy(), rtol=1e-6, atol=0)


def test_bf16_predictions_and_no_positives(loss_case):
    l = loss_case["l"]
    head = _head("both")
    labels = _cu(loss_case["labels"])
    x = [_cu(l[k]).bfloat16().requires_grad_(True) for k in ("cls_preds", "box_preds", "part_preds")]
    head.forward_ret_dict = _ret_dict(loss_case, x)
    loss, tb = head.get_loss()
    grads = torch.autograd.grad(loss, x)
    xr = [t.detach().double().requires_grad_(True) for t in x]
    ref = BR.full_loss(xr[0], labels, 3, BR.LOSS_WEIGHTS, xr[1], _cu(loss_case["box_labels"]), BR.CODE_WEIGHTS, xr[2],
                       _cu(loss_case["part_labels"]))
    ref_grads = torch.autograd.grad(ref[0], xr)
    for got, want in zip((loss, tb['point_loss_cls'], tb['point_loss_box'], tb['point_loss_part']), ref):
        assert abs(float(got) - float(want)) < BAR * abs(float(want))
    for d, dr in zip(grads, ref_grads):
        assert d.dtype == torch.bfloat16
        assert float((d.double() - dr).abs().max() / dr.abs().max()) < 2 ** -8       # stored in bf16: one ulp is 2^-8 relative
    # num_pos = 0: the normaliser clamps to 1, the box and part terms and their gradients vanish
    none = torch.where(labels > 0, torch.zeros_like(labels), labels)
    y = [_cu(l[k]).requires_grad_(True) for k in ("cls_preds", "box_preds", "part_preds")]
    head.forward_ret_dict = _ret_dict(loss_case, y, labels=none)
    loss0, tb0 = head.get_loss()
    g0 = torch.autograd.grad(loss0, y)
    ref0 = PR.cls_layer_loss(y[0].detach().double(), none, 3, BR.LOSS_WEIGHTS['point_cls_weight'])
    assert float(tb0['point_pos_num']) == 0 and float(tb0['point_loss_box']) == 0 and float(tb0['point_loss_part']) == 0
    assert abs(float(loss0) - float(ref0)) < BAR * abs(float(ref0))
    assert not g0[1].any() and not g0[2].any() and g0[0].any()


@pytest.mark.parametrize("num_class,mean", [(1, True), (1, False), (3, True), (3, False)])
def test_decoded_boxes_against_fp64(golden, num_class, mean):
    d = golden("g49_point_head_box_decode")
    tag = f"c{num_class}_{'mean' if mean else 'nomean'}"
    head = PointHeadBox(num_class, 8, BR.head_cfg('PointHeadBox', use_mean_size=mean)).cuda()
    pts, cls, enc = _cu(d["points"]), _cu(d["cls_preds"][:, :num_class]), _cu(d["box_preds"])
    coords = torch.cat([torch.zeros(pts.shape[0], 1, device="cuda"), pts], 1)
    cls_out, boxes = head.generate_predicted_boxes(points=coords[:, 1:4], point_cls_preds=cls, point_box_preds=enc)   # a strided view
    assert cls_out is cls and boxes.dtype == torch.float32 and tuple(boxes.shape) == (pts.shape[0], 7)
    got, w64, w32 = boxes.cpu().numpy().astype(np.float64), d[tag + "_f64"], d[tag + "_f32"].astype(np.float64)
    e = max(np.abs(got - w64)[:, :6].max(), BR.heading_difference(got[:, 6], w64[:, 6]).max())
    r = max(np.abs(w32 - w64)[:, :6].max(), BR.heading_difference(w32[:, 6], w64[:, 6]).max())
    print(f"[decode {tag}] ours vs fp64 {e:.2e}; the reference's fp32 vs fp64 {r:.2e}")
    assert r < BAR and e < BAR
    # a bare decode_torch with the classes given: the same boxes
    coder = PointResidualCoder(use_mean_size=mean, mean_size=MEAN)
    classes = cls.argmax(dim=-1) + 1
    assert torch.equal(coder.decode_torch(enc, pts, classes), boxes)
    assert torch.equal(coder.decode_torch(enc[None], pts[None], classes[None])[0], boxes)


def test_more_classes_than_mean_sizes_is_unsupported(golden):
    d = golden("g49_point_head_box_decode")
    four = _cu(np.concatenate([d["cls_preds"], d["cls_preds"][:, :1]], 1))
    with pytest.raises(L.PcdError, match="pcd_point_head_decode"):
        PH.decode_boxes(_cu(d["box_preds"]), _cu(d["points"]), _cu(np.asarray(MEAN, np.float32)), cls_preds=four)


def test_eval_forward_writes_the_reference_keys(targets):
    pc = _cu(targets["pc"][:1000])
    feats = torch.randn(1000, 32, device="cuda")
    for which in ("box", "both", "part"):
        head = _head(which).eval()
        out = head({'point_features': feats, 'point_coords': pc, 'batch_size': 4})
        f = head.forward_ret_dict
        assert 'point_cls_labels' not in f and tuple(out['point_cls_scores'].shape) == (1000,)
        assert torch.equal(out['point_cls_scores'], torch.sigmoid(f['point_cls_preds']).max(dim=-1)[0])
        if which == "part":
            assert 'batch_box_preds' not in out and 'batch_cls_preds' not in out
        else:
            assert out['batch_cls_preds'] is f['point_cls_preds'] and out['cls_preds_normalized'] is False
            assert torch.equal(out['batch_index'], pc[:, 0]) and tuple(out['batch_box_preds'].shape) == (1000, 7)
            want = BR.decode_f64(f['point_box_preds'].detach().cpu().numpy(), targets["pc"][:1000, 1:4],
                                 f['point_cls_preds'].argmax(dim=-1).cpu().numpy() + 1, MEAN)
            got = out['batch_box_preds'].cpu().numpy()
            assert np.abs(got - want)[:, :6].max() < BAR and BR.heading_difference(got[:, 6], want[:, 6]).max() < BAR
        if which != "box":
            assert torch.equal(out['point_part_offset'], torch.sigmoid(f['point_part_preds']))
    train = _head("box").train()                                                 # training without predict_boxes_when_training
    out = train({'point_features': feats, 'point_coords': pc, 'gt_boxes': _cu(targets["gt"]), 'batch_size': 4})
    assert 'batch_box_preds' not in out and 'point_box_labels' in train.forward_ret_dict


def _step(head, feats, pc, gt):
    out = head({'point_features': feats, 'point_coords': pc, 'gt_boxes': gt, 'batch_size': gt.shape[0]})
    loss, tb = head.get_loss()
    grads = torch.autograd.grad(loss, [feats] + [p for p in head.parameters()])
    f = head.forward_ret_dict
    label_tensors = [f[k] for k in ('point_cls_labels', 'point_box_labels', 'point_part_labels') if f.get(k) is not None]
    return loss.detach(), grads, label_tensors, tb, out['batch_box_preds']


@pytest.mark.parametrize("which", ["box", "both"])
def test_training_step_is_capturable_replays_bit_identically_and_follows_gt_boxes(targets, which):
    """forward (training mode, proposals included) + get_loss + backward of each head in ONE graph with a fixed number of
    points: two replays give bit-identical loss, gradients and labels, and gt_boxes changed in place change the labels"""
    pc, gt = _cu(targets["pc"]), _cu(targets["gt"])
    torch.manual_seed(3)
    head = _head(which, predict_boxes_when_training=True).train()
    feats = torch.randn(pc.shape[0], 32, device="cuda", requires_grad=True)
    eager = _step(head, feats, pc, gt)
    assert torch.isfinite(eager[0]) and float(eager[0]) > 0
    eager = (eager[0], None, [t.clone() for t in eager[2]], None, None)            # no autograd graph alive during capture
    static_gt = gt.clone()
    head.forward_ret_dict = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _step(head, feats, pc, static_gt)
    runs = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        runs.append((out[0].clone(), [p.clone() for p in out[1]], [t.clone() for t in out[2]], out[4].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][3], runs[1][3])
    for p, q in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert torch.equal(p, q)
    assert len(runs[0][2]) == (2 if which == "box" else 3)
    for p, q in zip(runs[0][2], eager[2]):
        assert torch.equal(p, q)                                                 # the labels of the eager run
    assert abs(float(runs[0][0]) - float(eager[0])) <= 1e-5 * abs(float(eager[0]))   # (the eager Linear may pick another GEMM)
    keep = torch.from_numpy(targets["keep"]).cuda()
    assert torch.equal(runs[0][2][0][keep], _cu(targets["labels"][3])[keep])
    assert all(v.is_cuda for v in out[3].values())
    static_gt.zero_()                                                            # no boxes: no foreground any more
    graph.replay()
    torch.cuda.synchronize()
    assert int((out[2][0] > 0).sum()) == 0 and float(out[3]['point_pos_num']) == 0
    assert all(not t.any() for t in out[2][1:]) and not torch.equal(out[0], runs[0][0])
    static_gt.copy_(gt)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], runs[0][0]) and all(torch.equal(p, q) for p, q in zip(out[2], runs[0][2]))
