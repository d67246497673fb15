"""CPU: the host side of the anchor head (com_amd/hotpath/anchor_head.py) against fixtures g19-g22 = the reference's own
AnchorGenerator / AxisAlignedTargetAssigner / ResidualCoder / loss classes run on the CPU by
tests/golden/make_golden_anchor.py.  The device kernels are checked by tests/test_gpu_anchor_head.py."""
import hashlib

import numpy as np
import pytest
import torch

from com_amd import _lib as L
from com_amd.hotpath import AnchorGenerator, AnchorHeadSingle, ResidualCoder
from com_amd.hotpath import anchor_head as AH
from tests import anchor_ref as AR

NAMES = ["Vehicle", "Pedestrian", "Cyclist"]


def _sha(a):
    h = hashlib.sha256()
    a = np.ascontiguousarray(a)
    h.update(str(a.dtype).encode())
    h.update(str(a.shape).encode())
    h.update(a.tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def test_fixtures_are_whole(golden):
    g = golden("g20_anchor_targets")
    assert g["full_labels"].shape == (4, 212064) and g["full_labels"].dtype == np.int8
    assert [(g["full_labels"][b] > 0).sum() for b in range(4)] == [164, 75, 1, 0]
    assert [(g["full_labels"][b] < 0).sum() for b in range(4)] == [144, 61, 2, 0]
    assert g["full_pos"].shape[0] == g["full_pos_targets"].shape[0] == g["full_pos_gt"].shape[0] == 240
    small = g["small_labels"]
    assert small.shape == (5, 48 * 40 * 6) and (small[2] == 0).all() and (small[1] > 0).sum() > 0
    assert (g["single_labels"].max() == 1) and g["single_labels"].shape == (3, 48 * 40 * 2)
    g21 = golden("g21_anchor_loss")
    assert (g21["multi_labels"][1] <= 0).all() and (g21["multi_labels"][0] > 0).any()      # one frame without positives
    for k in ("multi_f32_scalars", "multi_f64_scalars", "single_f64_scalars"):
        assert np.isfinite(g21[k]).all() and g21[k][0] > 0


@pytest.mark.parametrize("tag", ["second", "pillar", "aligned"])
def test_anchor_generator_equals_the_reference_bit_for_bit(golden, tag):
    g = golden("g19_anchor_generator")
    stride, align = int(g[f"{tag}_stride"][0]), bool(g[f"{tag}_align"][0])
    cfgs = AR.small_cfg(NAMES, stride)
    for c in cfgs:
        c["align_center"] = align
    gen = AnchorGenerator(list(g[f"{tag}_range"]), cfgs)
    anchors, per = gen.generate_anchors([g[f"{tag}_grid"] // stride] * 3)
    assert per == list(g[f"{tag}_per_location"])
    for c, a in enumerate(anchors):
        a = a.numpy()
        assert a.dtype == np.float32 and list(a.shape) == list(g[f"{tag}_shape{c}"])
        np.testing.assert_array_equal(a[0, 0, :, 0, 0, 0], g[f"{tag}_xrow{c}"])
        np.testing.assert_array_equal(a[0, :, 0, 0, 0, 1], g[f"{tag}_yrow{c}"])
        np.testing.assert_array_equal(a.reshape(-1, 7)[::997], g[f"{tag}_rows{c}"])
        np.testing.assert_array_equal(_sha(a), g[f"{tag}_sha{c}"])


def test_residual_coder_round_trip_and_fixture(golden):
    g = golden("g22_anchor_decode")
    anchors = torch.from_numpy(g["multi_anchors"])
    B = g["multi_box"].shape[0]
    enc = torch.from_numpy(g["multi_box"]).view(B, -1, 7)
    dec = ResidualCoder().decode_torch(enc, anchors.view(1, -1, 7).repeat(B, 1, 1))
    np.testing.assert_array_equal(dec.numpy(), g["multi_batch_box_preds_nodir"])
    back = ResidualCoder().encode_torch(dec.view(-1, 7), anchors.repeat(B, 1))
    np.testing.assert_allclose(back.numpy(), enc.view(-1, 7).numpy(), rtol=1e-5, atol=1e-5)
    g20 = golden("g20_anchor_targets")                      # encode against the assigner's targets of the small case
    gen = AnchorGenerator(list(g20["small_range"]), AR.small_cfg(NAMES))
    all_a = torch.cat(gen.generate_anchors([g20["small_grid"]] * 3)[0], dim=-3).view(-1, 7)
    pos = g20["small_pos"]
    boxes = torch.from_numpy(g20["small_gt_boxes"][pos[:, 0], g20["small_pos_gt"], :7])
    t = ResidualCoder().encode_torch(boxes, all_a[pos[:, 1]])
    np.testing.assert_array_equal(t.numpy(), g20["small_pos_targets"])
    with pytest.raises(L.PcdError, match="encode_angle_by_sincos"):
        ResidualCoder(encode_angle_by_sincos=True)


REFUSED = [("USE_MULTIHEAD", dict(USE_MULTIHEAD=True)),
           ("NAME", dict(TARGET_ASSIGNER_CONFIG=dict(NAME='ATSS', POS_FRACTION=-1.0, NORM_BY_NUM_EXAMPLES=False,
                                                     MATCH_HEIGHT=False, BOX_CODER='ResidualCoder', TOPK=9))),
           ("MATCH_HEIGHT", "MATCH_HEIGHT"), ("POS_FRACTION", "POS_FRACTION"), ("NORM_BY_NUM_EXAMPLES", "NORM_BY_NUM_EXAMPLES"),
           ("BOX_CODER", "BOX_CODER"), ("encode_angle_by_sincos", "BOX_CODER_CONFIG"),
           ("REG_LOSS_TYPE", dict(LOSS_CONFIG=dict(REG_LOSS_TYPE='WeightedL1Loss', LOSS_WEIGHTS={
               'cls_weight': 1.0, 'loc_weight': 2.0, 'dir_weight': 0.2, 'code_weights': [1.0] * 7})))]


@pytest.mark.parametrize("key,change", REFUSED, ids=[k for k, _ in REFUSED])
def test_configurations_outside_the_scope_are_refused_by_name(key, change):
    cfg = AR.head_cfg(NAMES, stride=8)
    if isinstance(change, dict):
        cfg.update(change)
    else:
        value = {"MATCH_HEIGHT": True, "POS_FRACTION": 0.5, "NORM_BY_NUM_EXAMPLES": True, "BOX_CODER": "PreviousResidualDecoder",
                 "BOX_CODER_CONFIG": {"encode_angle_by_sincos": True}}[change]
        cfg["TARGET_ASSIGNER_CONFIG"] = dict(cfg["TARGET_ASSIGNER_CONFIG"], **{change: value})
    with pytest.raises(L.PcdError, match=key):
        AnchorHeadSingle(cfg, 64, 3, NAMES, np.array([1504, 1504, 40]), [-75.2, -75.2, -2, 75.2, 75.2, 4])


def test_reference_shaped_state_dict_loads_strictly_and_there_is_no_cpu_fallback():
    head = AnchorHeadSingle(AR.head_cfg(NAMES, stride=8), 384, 3, NAMES, np.array([1504, 1504, 40]),
                            [-75.2, -75.2, -2, 75.2, 75.2, 4])
    assert head.num_anchors_per_location == 6 and len(head.anchors) == 3 and head.anchors[0].shape == (1, 188, 188, 1, 2, 7)
    ref = {"conv_cls.weight": torch.randn(18, 384, 1, 1), "conv_cls.bias": torch.randn(18),
           "conv_box.weight": torch.randn(42, 384, 1, 1), "conv_box.bias": torch.randn(42),
           "conv_dir_cls.weight": torch.randn(12, 384, 1, 1), "conv_dir_cls.bias": torch.randn(12)}
    head.load_state_dict(ref, strict=True)
    assert set(head.state_dict()) == set(ref)
    assert float(AnchorHeadSingle(AR.head_cfg(NAMES, stride=8), 8, 3, NAMES, np.array([1504, 1504, 40]),
                                  [-75.2, -75.2, -2, 75.2, 75.2, 4]).conv_cls.bias[0]) == pytest.approx(-np.log(99.0))
    nodir = AnchorHeadSingle(AR.head_cfg(NAMES, stride=8, use_dir=False), 8, 3, NAMES, np.array([1504, 1504, 40]),
                             [-75.2, -75.2, -2, 75.2, 75.2, 4])
    assert nodir.conv_dir_cls is None and set(nodir.state_dict()) == {k for k in ref if "dir" not in k}
    with pytest.raises(L.PcdError, match="no CPU fallback"):
        head.assign_targets(torch.zeros((1, 4, 8)))
    with pytest.raises(L.PcdError, match="no CPU fallback"):
        head.eval()({"spatial_features_2d": torch.zeros((1, 384, 188, 188)), "batch_size": 1})


def test_new_symbols_are_bound():
    names = ["pcd_anchor_assign_workspace_bytes", "pcd_anchor_assign_targets", "pcd_anchor_loss_workspace_bytes",
             "pcd_anchor_loss_forward", "pcd_anchor_loss_backward", "pcd_anchor_decode"]
    lib = L.lib()
    for n in names:
        assert n in L.PROTOTYPES and hasattr(lib, n)
    assert lib.pcd_anchor_assign_workspace_bytes(4, 128) >= 4 * 128 * 7 * 4
    assert lib.pcd_anchor_loss_workspace_bytes(4, 188, 188, 6) >= 4 * 829 * 3 * 4
    assert lib.pcd_anchor_loss_workspace_bytes(4, 188, 188, AH.MAX_KINDS + 1) == 0


@pytest.mark.parametrize("tag,num_class", [("multi", 3), ("single", 1)])
def test_fp32_reference_losses_and_the_restatement_meet_the_fp64_bar(golden, tag, num_class):
    """The bar of the GPU test (1e-4 relative to fp64 arithmetic on the same inputs; gradients relative to the largest
    magnitude of the tensor) is one the reference's own fp32 evaluation meets, and tests/anchor_ref.py in fp64 IS the
    reference's fp64 evaluation (so it may stand in for it on bf16-rounded inputs)."""
    g = golden("g21_anchor_loss")
    s32, s64 = g[f"{tag}_f32_scalars"], g[f"{tag}_f64_scalars"]
    np.testing.assert_allclose(s32, s64, rtol=1e-4)
    for name in ("dcls", "dbox", "ddir"):
        d32, d64 = g[f"{tag}_f32_{name}"], g[f"{tag}_f64_{name}"]
        assert np.abs(d32 - d64).max() <= 1e-4 * np.abs(d64).max()
    B = g[f"{tag}_cls"].shape[0]
    A = 2 * num_class
    t = [torch.from_numpy(g[f"{tag}_{k}"]).double().requires_grad_(True) for k in ("cls", "box", "dir")]
    names = NAMES[:num_class]
    head = AnchorHeadSingle(AR.head_cfg(names), 8, num_class, names, np.array([16, 12, 1]), list(g["range"]))
    rot = head._tables_host.kinds[:, 3].repeat(16 * 12)
    labels = torch.from_numpy(g[f"{tag}_labels"].astype(np.int64))
    targets = torch.from_numpy(g[f"{tag}_targets"])
    out = AR.get_loss(t[0].view(B, -1, num_class), t[1].view(B, -1, 7), t[2].view(B, -1, 2), labels, targets, rot, num_class)
    np.testing.assert_allclose([float(v.detach()) for v in out], s64, rtol=1e-6)   # (the reference's anchor weights stay fp32)
    out[0].backward()
    for name, x in zip(("dcls", "dbox", "ddir"), t):
        ref = g[f"{tag}_f64_{name}"]
        assert np.abs(x.grad.numpy() - ref).max() <= 1e-6 * np.abs(ref).max()

