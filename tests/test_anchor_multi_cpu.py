"""CPU: the host side of AnchorHeadMulti (com_amd/hotpath/anchor_head_multi.py) against fixtures g38-g42 = the reference's
own AnchorHeadMulti run on the CPU (tests/golden/make_golden_anchor_multi.py): state-dict layout, the coder, the fp64
restatement the GPU tests lean on (tests/anchor_multi_ref.py), the refusals, the C struct's ctypes mirror."""
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from com_amd import _lib as L
from com_amd.hotpath import anchor_head_multi as AM
from tests import anchor_multi_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _head(case, cfg=None, class_names=None):
    names = class_names or AR.CASES[case]["names"]
    return AM.AnchorHeadMulti(cfg or AR.model_cfg(case), AR.IN_CHANNELS, len(names), names, np.array(AR.GRID), AR.RANGE)


@pytest.mark.parametrize("case", ["N", "K"])
def test_state_dict_layout_is_the_references(golden, case):
    g = golden("g42_anchor_multi_module")
    head = _head(case)
    sd = head.state_dict()
    keys = [str(k) for k in g[f"{case}_keys"]]
    assert list(sd) == keys
    ref = {k: torch.from_numpy(g[f"{case}_state_{k}"]) for k in keys}
    for k in keys:
        assert tuple(sd[k].shape) == tuple(ref[k].shape) and sd[k].dtype == ref[k].dtype, k
    head.load_state_dict(ref, strict=True)
    for hd, names in zip(head.rpn_heads, AR.CASES[case]["heads"]):
        assert hd.head_label_indices.dtype == torch.int64 and len(hd.blocks) == 0 and len(hd.deblocks) == 0
        assert hd.head_label_indices.tolist() == [AR.CASES[case]["names"].index(n) + 1 for n in names]
    if case == "N":
        bn = head.shared_conv[1]
        assert bn.eps == 1e-3 and bn.momentum == 0.01 and head.rpn_heads[0].conv_dir_cls is None
    else:
        assert head.shared_conv is None and head.rpn_heads[0].conv_dir_cls is not None


def test_initialisation_follows_the_reference():
    head = _head("N")
    for hd in head.rpn_heads:
        assert torch.all(hd.conv_cls[-1].bias == float(-np.log(99.0)))
        for name in hd.conv_box_names:
            assert torch.all(hd.conv_box[name][-1].bias == 0)
    # an explicit False still creates the conv (anchor_head_multi.py:86); loss and decoding ignore it
    head = _head("K", AR.model_cfg("K", USE_DIRECTION_CLASSIFIER=False))
    assert head.rpn_heads[0].conv_dir_cls is not None and not head.use_dir and not head._loss.has_dir


@pytest.mark.parametrize("case", ["N", "K"])
def test_coder_against_the_fixtures(golden, case):
    g38 = golden("g38_anchor_multi_targets")
    g40 = golden(f"g40_anchor_multi_decode_{case}")
    head = _head(case)
    coder = head.box_coder
    assert coder.code_size == (10 if case == "N" else 7) and coder.encode_angle_by_sincos == (case == "N")
    anchors = torch.from_numpy(g38[f"{case}_anchors"])
    gt, gi, ref = g38[f"{case}_gt_boxes"], g38[f"{case}_gt_index"], g38[f"{case}_targets"]
    b, n = np.nonzero(gi >= 0)
    assert b.size > 20
    boxes = torch.from_numpy(gt[b, gi[b, n], :-1])
    keep = boxes.clone()
    enc = coder.encode_torch(boxes, anchors[n])
    assert torch.equal(boxes, keep)
    np.testing.assert_allclose(enc.numpy(), ref[b, n], rtol=1e-6, atol=1e-6)
    # decoding: the fixture's maps in the reference's anchor-major form
    lay = AR.head_layout(case)
    codes = torch.cat([AR.to_anchor_major(torch.from_numpy(g40[f"{case}_box{h}"]), nk) for h, (_, nk, _, _) in enumerate(lay)], 1)
    dec = coder.decode_torch(codes, anchors.unsqueeze(0)).numpy()
    want = g40[f"{case}_batch_box_preds"]
    cols = [0, 1, 2, 3, 4, 5, 7, 8] if case == "N" else [0, 1, 2, 3, 4, 5]     # (case K's heading: direction bins on top)
    np.testing.assert_allclose(dec[..., cols], want[..., cols], rtol=1e-6, atol=1e-6)
    if case == "N":
        d = dec[..., 6] - want[..., 6]
        assert np.abs(d - np.round(d / (2 * np.pi)) * 2 * np.pi).max() <= 1e-6


def _restated(g, case, dt, labels, targets, anchors):
    lay = AR.head_layout(case)
    maps = []
    for name in ("cls", "box", "dir"):
        maps.append([torch.from_numpy(g[f"{case}_{name}{h}"]).to(dt).requires_grad_(True) for h in range(len(lay))]
                    if f"{case}_{name}0" in g else None)
    cfg = AR.model_cfg(case)
    lw = cfg["LOSS_CONFIG"]["LOSS_WEIGHTS"]
    r = AR.get_loss(maps[0], maps[1], maps[2], torch.from_numpy(labels.astype(np.int64)), torch.from_numpy(targets),
                    torch.from_numpy(anchors[:, 6]), lay, len(AR.CASES[case]["names"]),
                    cfg["LOSS_CONFIG"].get("REG_LOSS_TYPE") == "WeightedL1Loss", lw.get("pos_cls_weight", 1.0),
                    lw.get("neg_cls_weight", 1.0), (lw["cls_weight"], lw["loc_weight"], lw["dir_weight"]),
                    code_weights=torch.tensor(lw["code_weights"]))
    return maps, r


@pytest.mark.parametrize("case", ["N", "K"])
def test_restatement_matches_the_references_fp64(golden, case):
    g38, g = golden("g38_anchor_multi_targets"), golden(f"g39_anchor_multi_loss_{case}")
    maps, r = _restated(g, case, torch.float64, g38[f"{case}_labels"], g38[f"{case}_targets"], g38[f"{case}_anchors"])
    r[0].backward()
    got = np.array([float(v.detach()) for v in r])
    # (1e-6 and not round-off of fp64: the reference's anchor weights stay fp32 in its fp64 run, as in test_anchor_head_cpu)
    np.testing.assert_allclose(got, g[f"{case}_f64_scalars"], rtol=1e-6, atol=1e-14)
    assert got[0] > 0.1 and got[2] > 0.01 and (got[3] > 0) == (case == "K")
    for name, group in zip(("dcls", "dbox", "ddir"), maps):
        for h, t in enumerate(group or []):
            ref = g[f"{case}_f64_{name}{h}"]
            assert np.abs(t.grad.numpy() - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1e-30), (name, h)
    # and in fp32 it is the reference's fp32 figure up to summation order
    _, r32 = _restated(g, case, torch.float32, g38[f"{case}_labels"], g38[f"{case}_targets"], g38[f"{case}_anchors"])
    np.testing.assert_allclose(np.array([float(v.detach()) for v in r32]), g[f"{case}_f32_scalars"], rtol=2e-5, atol=1e-7)


def _over(case, path, value):
    cfg = copy.deepcopy(AR.model_cfg(case))
    node = cfg
    for k in path[:-1]:
        node = node[k]
    node[path[-1]] = value
    return cfg


REFUSALS = [
    ("SEPARATE_MULTIHEAD", ("SEPARATE_MULTIHEAD",), False),
    ("USE_MULTIHEAD", ("USE_MULTIHEAD",), False),
    ("TARGET_ASSIGNER_CONFIG.NAME", ("TARGET_ASSIGNER_CONFIG", "NAME"), "ATSS"),
    ("MATCH_HEIGHT", ("TARGET_ASSIGNER_CONFIG", "MATCH_HEIGHT"), True),
    ("POS_FRACTION", ("TARGET_ASSIGNER_CONFIG", "POS_FRACTION"), 0.5),
    ("NORM_BY_NUM_EXAMPLES", ("TARGET_ASSIGNER_CONFIG", "NORM_BY_NUM_EXAMPLES"), True),
    ("BOX_CODER", ("TARGET_ASSIGNER_CONFIG", "BOX_CODER"), "PreviousResidualDecoder"),
    ("encode_angle_by_sincos", ("TARGET_ASSIGNER_CONFIG", "BOX_CODER_CONFIG"), {"encode_angle_by_sincos": True}),
    ("code_size", ("TARGET_ASSIGNER_CONFIG", "BOX_CODER_CONFIG"), {"code_size": 8}),
    ("REG_LOSS_TYPE", ("LOSS_CONFIG", "REG_LOSS_TYPE"), "WeightedBinaryCrossEntropyLoss"),
    ("NUM_DIR_BINS", ("NUM_DIR_BINS",), 12),
]


@pytest.mark.parametrize("key,path,value", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_their_key(key, path, value):
    with pytest.raises(L.PcdError, match=key):
        _head("K", _over("K", path, value))


def test_refusals_of_the_anchor_layout_name_their_key():
    cfg = AR.model_cfg("K")
    cfg["ANCHOR_GENERATOR_CONFIG"][1]["feature_map_stride"] = 2
    with pytest.raises(L.PcdError, match="feature_map_stride"):
        _head("K", cfg)
    cfg = AR.model_cfg("K")
    cfg["ANCHOR_GENERATOR_CONFIG"][0]["anchor_bottom_heights"] = [-1.0, 0.0]
    with pytest.raises(L.PcdError, match="anchor_bottom_heights"):
        _head("K", cfg)
    cfg = AR.model_cfg("N")                                             # heads in another order than the classes
    cfg["RPN_HEAD_CFGS"] = [dict(HEAD_CLS_NAME=h) for h in (["truck", "bus"], ["car"], ["pedestrian"])]
    with pytest.raises(L.PcdError, match="HEAD_CLS_NAME"):
        _head("N", cfg)
    with pytest.raises(L.PcdError, match="HEAD_CLS_NAME"):               # class_names in another order
        _head("N", class_names=["truck", "car", "bus", "pedestrian"])
    cfg = AR.model_cfg("K")                                             # over the kernel limits: 3 x 12 = 36 kinds
    for c in cfg["ANCHOR_GENERATOR_CONFIG"]:
        c["anchor_rotations"] = [0.1 * i for i in range(12)]
    with pytest.raises(L.PcdError, match="ANCHOR_GENERATOR_CONFIG"):
        _head("K", cfg)
    cfg = AR.model_cfg("N")
    cfg["SEPARATE_REG_CONFIG"]["REG_LIST"] = ['reg:2', 'height:1', 'size:3', 'angle:2']
    with pytest.raises(L.PcdError, match="REG_LIST"):
        _head("N", cfg)
    cfg = AR.model_cfg("K")
    cfg["LOSS_CONFIG"]["LOSS_WEIGHTS"]["code_weights"] = [1.0] * 8
    with pytest.raises(L.PcdError, match="code_weights"):
        _head("K", cfg)
    with pytest.raises(L.PcdError, match="MULTI_CLASSES_NMS"):
        AM.post_processing({}, dict(NMS_CONFIG=dict(MULTI_CLASSES_NMS=False)))


def test_tables_describe_the_references_anchors(golden):
    """kind rows + shift tables reproduce every anchor of the multi-head order, bit for bit; cos / sin are torch's"""
    g38 = golden("g38_anchor_multi_targets")
    for case in ("N", "K"):
        tab = _head(case)._tables_host
        ref = g38[f"{case}_anchors"]
        k = tab.kinds
        assert k.shape == (tab.G, AM.KIND_FLOATS) and tab.N == ref.shape[0] and tab.heads == AR.head_layout(case)
        assert torch.equal(k[:, 10], torch.cos(k[:, 3])) and torch.equal(k[:, 11], torch.sin(k[:, 3]))
        n = np.arange(tab.N)
        gk, y, x = n // (tab.H * tab.W), n // tab.W % tab.H, n % tab.W
        slot = k[:, 5].long().numpy()[gk]
        sh = tab.shifts.numpy()
        built = np.stack([sh[slot, x], sh[slot, tab.W + y], k[:, 4].numpy()[gk], k[:, 0].numpy()[gk], k[:, 1].numpy()[gk],
                          k[:, 2].numpy()[gk], k[:, 3].numpy()[gk]], 1)
        np.testing.assert_array_equal(built, ref[:, :7])
        assert (ref[:, 7:] == 0).all()


def test_struct_matches_its_ctypes_mirror(tmp_path):
    """PcdAnchorMultiHead as gcc lays it out from include/pcd_ops.h == the mirror in anchor_head_multi.py"""
    st = AM.PcdAnchorMultiHead
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pcd_ops.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(PcdAnchorMultiHead));']
    lines += [f'printf("{f} %zu\\n", offsetof(PcdAnchorMultiHead, {f}));' for f, _ in st._fields_]
    lines += ['return 0; }']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {ln.split()[0]: int(ln.split()[1]) for ln in subprocess.check_output([str(exe)]).decode().split("\n") if ln}
    assert got["size"] == ctypes.sizeof(st)
    for f, _ in st._fields_:
        assert got[f] == getattr(st, f).offset, f
    assert L.PCD_ANCHOR_MULTI_KIND_FLOATS == 12 and L.PCD_ANCHOR_MULTI_MAX_HEADS == 8
    for name in ("pcd_anchor_multi_assign_targets", "pcd_anchor_multi_loss_forward", "pcd_anchor_multi_loss_backward",
                 "pcd_anchor_multi_decode"):
        assert name in L.PROTOTYPES and hasattr(L.lib(), name)


def test_the_old_heads_are_exported_unchanged():
    import com_amd.hotpath as H
    from com_amd.hotpath import anchor_head
    assert H.AnchorHeadSingle is anchor_head.AnchorHeadSingle and H.ResidualCoder is anchor_head.ResidualCoder
    assert H.AnchorGenerator is anchor_head.AnchorGenerator
    assert H.AnchorHeadMulti is AM.AnchorHeadMulti and H.SingleHead is AM.SingleHead
    with pytest.raises(L.PcdError, match="encode_angle_by_sincos"):
        H.ResidualCoder(encode_angle_by_sincos=True)
    from tests import anchor_ref
    with pytest.raises(L.PcdError, match="USE_MULTIHEAD"):
        H.AnchorHeadSingle(anchor_ref.head_cfg(["Vehicle"], USE_MULTIHEAD=True), 8, 1, ["Vehicle"], np.array([48, 40, 1]),
                           [0.0, -15.6, -2, 37.6, 15.6, 4])


def test_there_is_no_cpu_fallback():
    head = _head("K")
    with pytest.raises(L.PcdError, match="HIP device"):
        head.assign_targets(torch.zeros(1, 4, 8))
