"""GPU: com_amd.infer.CapturedInference on the stock CenterPoint and COM detectors of tools/stock_detector.py, adopted with
com_amd.adopt.adopt_model:

  5. the captured head maps are bit-identical to the eager eval forward's pred_dicts, the captured outputs to the eager
     forward + static post-processing, and two replays of one batch to each other;
  6. different batches give different predictions (the staging reaches the graph);
  7. load_state_dict of another seed, in place, after the capture: the next replay is the eager forward with the new weights;
  8. a plan that observed half the rows raises the sticky flag, and recapture() recovers.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
DEV = "cuda:0"
B = 2


def _batches(n=3, beams=32, azimuth=2500):
    from com_amd import hotpath
    from com_amd.utils import synth
    return [hotpath.collate_points([synth.synth_cloud(10 * i + f, beams, azimuth) for f in range(B)], DEV) for i in range(n)]


def _model(kind, seed=0):
    import stock_detector as SD
    from com_amd.adopt import adopt_model
    torch.manual_seed(seed)
    m = SD.build_detector(kind).to(DEV)
    assert adopt_model(m).complete
    return m


def _vox():
    from com_amd import train
    from com_amd.utils import synth
    return train.VoxelizeConfig(synth.WAYMO_RANGE, synth.WAYMO_VOXEL, synth.WAYMO_MAX_POINTS, synth.WAYMO_MAX_VOXELS)


def _clone(out):
    return {k: v.clone() for k, v in out.items()}


def _equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("boxes", "scores", "labels", "count"))


def _maps(head):
    return [{k: v.clone() for k, v in pd.items()} for pd in head.forward_ret_dict['pred_dicts']]


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("kind", ["centerpoint", "com"])
def test_captured_inference_is_the_eager_eval_forward(kind):
    from com_amd.infer import CapturedInference
    m = _model(kind)
    m.train()
    batches = _batches()
    inf = CapturedInference(m, _vox(), B)
    inf.capture(batches[0], validate=batches[1:])
    assert inf.captured and m.training and all(x.training for x in m.modules())    # the flags are restored
    out0 = _clone(inf(batches[0]))
    maps_g = _maps(m.dense_head)
    out0b = _clone(inf(batches[0]))
    assert _equal(out0, out0b), "two replays of one batch differ"
    eager = _clone(inf.eager(batches[0]))
    maps_e = _maps(m.dense_head)
    for a, b in zip(maps_g, maps_e):
        for k in a:
            assert torch.equal(a[k], b[k]), f"captured head map {k} differs from the eager eval forward"
    assert _equal(out0, eager), "captured outputs differ from the eager forward + static post-processing"
    assert int(out0["count"].min()) > 0
    # 6. different batches -> different predictions
    out1 = _clone(inf(batches[1]))
    assert not _equal(out0, out1)
    assert _equal(out1, inf.eager(batches[1]))
    preds = inf.pred_dicts(out1)
    assert len(preds) == B and all(p["pred_boxes"].shape[1] == 7 for p in preds)
    inf.check()


@pytest.mark.timeout(1800)
def test_replay_reads_live_weights():
    from com_amd import _lib as L
    from com_amd.infer import CapturedInference
    m = _model("centerpoint", seed=0)
    other = _model("centerpoint", seed=1).state_dict()
    with torch.no_grad():                                   # BatchNorm statistics of their own
        for k, v in other.items():
            if k.endswith("running_mean"):
                v.normal_(0, 0.05)
            elif k.endswith("running_var"):
                v.uniform_(0.5, 1.5)
    batches = _batches()
    inf = CapturedInference(m, _vox(), B)
    inf.capture(batches[0], validate=batches[1:])
    before = _clone(inf(batches[0]))
    m.load_state_dict(other)                                # in place: same storages
    after = _clone(inf(batches[0]))
    assert not _equal(before, after), "the replay did not see the new weights"
    assert _equal(after, inf.eager(batches[0])), "the replay with the new weights differs from the eager forward"
    assert inf.recaptures == 0
    # a parameter whose storage moved is refused
    p = m.dense_head.heads_list[0].hm[1].weight
    p.data = p.data.clone()
    with pytest.raises(L.PcdError, match="moved"):
        inf(batches[0])


@pytest.mark.timeout(1800)
def test_overflow_flag_and_recapture():
    from com_amd import _lib as L
    from com_amd.infer import CapturedInference
    m = _model("centerpoint")
    batches = _batches()
    inf = CapturedInference(m, _vox(), B)
    for b in batches:
        inf.eager(b)                                        # observe the row counts
    for k in inf.plan.caps:
        inf.plan.caps[k] = inf.plan.caps[k] // 2
    inf.capture(batches[0])
    inf(batches[1])
    torch.cuda.synchronize()
    with pytest.raises(L.PcdError):
        inf.check()
    inf.recapture()
    inf.recapture()                                         # x 1.5 twice: above the real counts again
    out = _clone(inf(batches[1]))
    inf.check()
    assert inf.recaptures == 2
    assert _equal(out, inf.eager(batches[1]))


def test_refusals():
    from com_amd import _lib as L
    from com_amd.adopt import adopt_model
    from com_amd.infer import CapturedInference
    import stock_detector as SD
    with pytest.raises(L.PcdError, match="adopt_model"):
        CapturedInference(SD.build_detector("centerpoint"), _vox(), B)
    m = SD.build_detector("3d")
    adopt_model(m)
    with pytest.raises(L.PcdError, match="centre head"):
        CapturedInference(m, _vox(), B)
    m = SD.build_detector("centerpoint")
    m.dense_head.model_cfg['POST_PROCESSING']['NMS_CONFIG']['NMS_TYPE'] = 'circle_nms'
    adopt_model(m)
    with pytest.raises(L.PcdError, match="circle_nms"):
        CapturedInference(m, _vox(), B)
