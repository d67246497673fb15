"""CPU: com_amd.adopt.adopt_model on a detector object shaped like the reference's build_networks output
(tools/stock_detector.py) -- the fused modules take over the stock modules' own Parameter / buffer objects, state-dict
keys and values do not move, anything unrecognised is refused with its module path -- and the host-side capacity check of
the step's ground-truth staging."""
import os
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from com_amd import _lib as L  # noqa: E402
from com_amd import hotpath, train  # noqa: E402
from com_amd.adopt import adopt_model  # noqa: E402

SLOTS = ("vfe", "backbone_3d", "map_to_bev_module", "backbone_2d", "dense_head")


def _stock(kind):
    import stock_detector as SD
    torch.manual_seed(0)
    m = SD.build_detector(kind)
    with torch.no_grad():                                    # non-trivial BN statistics / counters
        for b in m.buffers():
            if b.is_floating_point():
                b.uniform_(0.5, 1.5)
            else:
                b.fill_(7)
    return m


@pytest.mark.parametrize("kind", ["3d", "centerpoint", "com"])
def test_adopt_keeps_state_and_objects(kind):
    m = _stock(kind)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    tensors = {k: v for k, v in m.state_dict(keep_vars=True).items()}
    params = list(m.parameters())
    rep = adopt_model(m)
    assert len(rep.replaced) == (3 if kind == "3d" else 5) and not rep.unrecognised
    after = m.state_dict(keep_vars=True)
    assert list(after) == list(before)
    for k, v in before.items():
        assert after[k] is tensors[k], k                      # the same Parameter / buffer objects (BN stats included)
        assert after[k].shape == v.shape and torch.equal(after[k].detach(), v), k
    assert [id(p) for p in m.parameters()] == [id(p) for p in params]
    for i, name in enumerate(n for n in SLOTS if getattr(m, n, None) is not None):
        assert m.module_list[i] is getattr(m, name)
        assert type(m.module_list[i]).__module__.startswith("com_amd.hotpath")
    assert isinstance(m.backbone_3d, hotpath.VoxelResBackBone8x)
    assert m.map_to_bev_module.channels_last
    if kind == "centerpoint":
        assert isinstance(m.dense_head, hotpath.CenterHead)
    if kind == "com":
        assert isinstance(m.dense_head, hotpath.CurriculumCenterHead_x5)
    rep2 = adopt_model(m)                                    # adopting twice: a no-op
    assert not rep2.replaced and len(rep2.kept) == len(rep.replaced)
    assert all(after[k] is t for k, t in m.state_dict(keep_vars=True).items())


def _refused(m, *fragments):
    with pytest.raises(L.PcdError) as ei:
        adopt_model(m)
    for f in fragments:
        assert f in str(ei.value), str(ei.value)


def test_extra_child_in_basic_block_is_refused():
    m = _stock("3d")
    m.backbone_3d.conv2[1].extra = nn.ReLU()
    _refused(m, "backbone_3d.conv2.1.extra", "unexpected child")


def test_changed_indice_key_and_stride_are_refused():
    m = _stock("3d")
    m.backbone_3d.conv3[1].conv1.indice_key = "res9"
    _refused(m, "backbone_3d.conv3.1.conv1", "indice_key")
    m = _stock("3d")
    m.backbone_3d.conv2[0]._modules["0"].stride = [1, 1, 1]
    _refused(m, "backbone_3d.conv2.0.0", "stride")
    m = _stock("centerpoint")
    m.backbone_2d.blocks[1][1].stride = (1, 1)
    _refused(m, "backbone_2d.blocks.1.1", "stride")


def test_changed_batchnorm_is_refused():
    m = _stock("centerpoint")
    m.dense_head.shared_conv[1].eps = 1e-3
    _refused(m, "dense_head.shared_conv.1", "eps")


class FancyBEV(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(256, 512, 1)

    def forward(self, d):
        return d


def test_unknown_class_refused_or_listed():
    m = _stock("centerpoint")
    m.backbone_2d = FancyBEV()
    m.module_list[3] = m.backbone_2d
    _refused(m, "backbone_2d", "unknown module class FancyBEV")
    rep = adopt_model(m, strict=False)
    assert rep.unrecognised and rep.unrecognised[0][0] == "backbone_2d"
    assert type(m.backbone_2d) is FancyBEV and m.module_list[3] is m.backbone_2d
    assert isinstance(m.dense_head, hotpath.CenterHead)     # the rest is adopted


def test_syncbn_under_two_ranks_is_refused(monkeypatch):
    m = _stock("centerpoint")
    old = m.backbone_2d.blocks[0][2]
    sync = nn.SyncBatchNorm(old.num_features, eps=old.eps, momentum=old.momentum)
    m.backbone_2d.blocks[0][2] = sync
    m.train()
    monkeypatch.setattr(torch.distributed, "is_available", lambda: True)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    _refused(m, "backbone_2d.blocks.0.2", "SyncBatchNorm")
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 1)
    adopt_model(m)                                           # one rank: a SyncBatchNorm is a BatchNorm
    assert m.backbone_2d.blocks[0][2].weight is sync.weight


def test_prepare_training_needs_an_adopted_model():
    m = _stock("3d")
    with pytest.raises(L.PcdError, match="adopt_model"):
        train.prepare_training(m, {"OPTIMIZER": "adam_onecycle"}, 10, None, 2)


def test_ground_truth_capacity_is_checked_on_the_host():
    st = train._LabelStage(train.COM_GT_KEYS, 2, 96)
    ok = {k: torch.zeros(2, 96, 8) if k == "gt_boxes" else torch.zeros(2, 96) for k in train.COM_GT_KEYS}
    st.check(ok)
    big = dict(ok, gt_boxes=torch.zeros(2, 97, 8))
    with pytest.raises(L.PcdError, match="max_gt=96"):
        st.check(big)
    with pytest.raises(L.PcdError, match="facade_type"):
        st.check({k: v for k, v in ok.items() if k != "facade_type"})
    with pytest.raises(L.PcdError, match="max_gt"):
        train.CapturedStep(nn.Linear(1, 1), None, _FakeOpt(), None, 2, batch_keys=("gt_boxes",))


def test_too_many_boxes_raise_before_any_device_work():
    """The eager and captured step raise from the shape alone: nothing of the batch is touched (a tensor whose data
    cannot be read would fail on the first copy, the check comes before it)."""
    step = train.CapturedStep(nn.Linear(1, 1), None, _FakeOpt(), None, 2, batch_keys=("gt_boxes",), max_gt=64)
    batch = {"points": torch.empty(0, 5, device="meta"), "frame_offsets": torch.empty(3, device="meta"),
             "gt_boxes": torch.empty(2, 65, 8, device="meta")}
    with pytest.raises(L.PcdError, match="65 rows"):
        step(batch)
    with pytest.raises(L.PcdError, match="65 rows"):
        step.prime(batch)
    assert step._pending is None


class _FakeOpt:
    class bucket:
        force_collective = False
