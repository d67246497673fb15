"""CPU: the two static halves of a two-stage detector's eval forward (com_amd.postprocess.anchor_proposals_static /
roi_predictions_static, C ABI pcd_anchor_proposals / pcd_roi_postproc) -- numpy oracles of both selection rules, the RoI
oracle pinned to the reference's own results (tests/golden/g46_second_postproc.npz), the settings functions and their refusals
by key name, the header's declarations, adopt_model on the "second_iou" stock detector of tools/stock_detector.py and the
refusals of CapturedInference / CapturedStep that need no device.

The oracles (`oracle_proposals`, `oracle_roi`) are also what tests/test_gpu_roi_postprocess.py holds the kernels to.

  proposals   score = the maximum LOGIT of the anchor (no sigmoid), label = the lowest class at the maximum + 1; every anchor
              takes part but one whose maximum is NaN; score descending (-0.0 == +0.0), then anchor index ascending; the first
              min(NMS_PRE_MAXSIZE, N) go through NMS, the first NMS_POST_MAXSIZE survivors are kept; behind them boxes 0,
              scores 0, labels 1.
  RoI rows    given the NMS score of every row: passes iff score >= SCORE_THRESH (inclusive, -0.0 == +0.0; every row
              without a threshold; a NaN never); score descending, then row ascending; min(NMS_PRE_MAXSIZE, R) through NMS,
              the first NMS_POST_MAXSIZE survivors; zero rows behind them."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import test_postprocess_cpu as O  # noqa: E402
from tests import second_head_ref as SR  # noqa: E402

F32 = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ------------------------------------------------------------------------------------------------------------ helpers
def nms_cfg(nms_type='nms_gpu', nms_thresh=0.7, nms_pre=1024, nms_post=100, multi=False):
    """One block of ROI_HEAD.NMS_CONFIG (kitti_models/second_iou.yaml:102-107)."""
    return dict(NMS_TYPE=nms_type, MULTI_CLASSES_NMS=multi, NMS_PRE_MAXSIZE=nms_pre, NMS_POST_MAXSIZE=nms_post,
                NMS_THRESH=nms_thresh)


def post_cfg(score_thresh=0.1, nms_type='nms_gpu', nms_thresh=0.01, nms_pre=4096, nms_post=500, multi=False, raw=False, **nms_keys):
    """The POST_PROCESSING block of SECOND-IoU (kitti_models/second_iou.yaml:136-148); nms_keys: SCORE_TYPE and its keys."""
    return dict(RECALL_THRESH_LIST=[0.3, 0.5, 0.7], SCORE_THRESH=score_thresh, OUTPUT_RAW_SCORE=raw, EVAL_METRIC='kitti',
                NMS_CONFIG=dict(MULTI_CLASSES_NMS=multi, NMS_TYPE=nms_type, NMS_THRESH=nms_thresh, NMS_PRE_MAXSIZE=nms_pre,
                                NMS_POST_MAXSIZE=nms_post, **nms_keys))


def _descending(score, idx):
    """idx ordered by score descending (-0.0 == +0.0: `+ 0.0` folds the sign), then index ascending"""
    return idx[np.lexsort((idx, -(score[idx].astype(np.float64) + 0.0)))]


def oracle_proposal_select(logits, nms_pre):
    """logits [N, num_class] of one frame -> (anchor indices in selection order, their scores, their 1-based labels)"""
    logits = np.asarray(logits, F32)
    score = logits.max(axis=1)                               # (np.max propagates NaN, as torch.max does)
    label = np.argmax(np.where(np.isnan(logits), np.inf, logits), axis=1) + 1      # the lowest class at the maximum
    idx = _descending(score, np.nonzero(~np.isnan(score))[0])[:nms_pre]
    return idx, score[idx], label[idx]


def oracle_proposals(logits, boxes, cfg):
    """The proposal layer in numpy from the logits [B, N, num_class] and the DECODED boxes of every anchor [B, N, 7] under
    one NMS_CONFIG block: {'rois', 'roi_scores', 'roi_labels', 'count', 'index'} as anchor_proposals_static (+ the kept
    anchors' indices, -1 behind)."""
    from com_amd.postprocess import roi_proposal_settings
    s = roi_proposal_settings(cfg)
    B, M = logits.shape[0], s["nms_post"]
    out = dict(rois=np.zeros((B, M, 7), F32), roi_scores=np.zeros((B, M), F32), roi_labels=np.ones((B, M), np.int64),
               count=np.zeros((B,), np.int32), index=np.full((B, M), -1, np.int64))
    for b in range(B):
        idx, sc, lab = oracle_proposal_select(logits[b], s["nms_pre"])
        keep = O.oracle_nms(boxes[b][idx], s["nms_thresh"], s["nms_normal"])[:M]
        k = len(keep)
        out["rois"][b, :k], out["roi_scores"][b, :k], out["roi_labels"][b, :k] = boxes[b][idx][keep], sc[keep], lab[keep]
        out["index"][b, :k] = idx[keep]
        out["count"][b] = k
    return out


def oracle_roi(scores, boxes, nms_pre, nms_post, score_thresh, nms_thresh, normal=False):
    """One frame: the NMS scores [R] (any float dtype; compared as they are) and boxes [R, 7] -> the kept rows, in order"""
    scores = np.asarray(scores)
    with np.errstate(invalid='ignore'):
        ok = ~np.isnan(scores) if score_thresh is None else scores >= scores.dtype.type(score_thresh)
    idx = _descending(scores, np.nonzero(ok)[0])[:nms_pre]
    keep = O.oracle_nms(np.asarray(boxes, F32)[idx], nms_thresh, normal)[:nms_post]
    return idx[keep]


def _far_boxes(N):
    boxes = np.zeros((N, 7), F32)
    boxes[:, 0] = 10.0 * np.arange(N, dtype=F32)
    boxes[:, 3:6] = 1.0
    return boxes


# ------------------------------------------------------------------------------------------------------------ oracles
def test_proposal_oracle_rules():
    logits = np.full((12, 3), -9.0, F32)
    logits[3] = [-2.0, -3.0, -2.0]          # two classes at the maximum: the lower label
    logits[7] = [-4.0, -1.0, -5.0]
    logits[5] = [-4.0, -6.0, -1.0]          # the same score as 7: the lower index first
    logits[9] = [0.0, -5.0, -5.0]
    logits[2] = [-5.0, -0.0, -5.0]          # -0.0 == +0.0: a tie with 9, the lower index first
    logits[10] = [np.nan, 9.0, 9.0]         # NaN: never takes part
    logits[1] = [0.5, 0.25, -1.0]
    idx, sc, lab = oracle_proposal_select(logits, 100)
    assert list(idx[:6]) == [1, 2, 9, 5, 7, 3] and list(lab[:6]) == [1, 2, 1, 3, 2, 1]
    assert list(idx[6:]) == [0, 4, 6, 8, 11] and 10 not in idx          # every other anchor takes part: no threshold
    assert sc[0] == F32(0.5) and np.signbit(sc[1]) and sc[3] == F32(-1.0)   # the logit itself, its own bits
    assert list(oracle_proposal_select(logits, 4)[0]) == [1, 2, 9, 5]


def test_proposal_oracle_caps_padding_and_nms():
    rng = np.random.default_rng(0)
    B, N = 2, 300
    logits = rng.integers(-16, 0, (B, N, 3)).astype(F32) * F32(0.5)      # negative, full of exact ties
    boxes = np.stack([_far_boxes(N)] * B)
    out = oracle_proposals(logits, boxes, nms_cfg(nms_pre=50, nms_post=20))
    sel, sc, lab = oracle_proposal_select(logits[0], 50)
    assert list(out["count"]) == [20, 20] and list(out["index"][0]) == list(sel[:20])
    for a in range(49):
        assert sc[a] > sc[a + 1] or (sc[a] == sc[a + 1] and sel[a] < sel[a + 1])
    out = oracle_proposals(logits, boxes, nms_cfg(nms_pre=10, nms_post=20))
    assert out["count"][0] == 10
    assert not out["rois"][0, 10:].any() and not out["roi_scores"][0, 10:].any() and (out["roi_labels"][0, 10:] == 1).all()
    boxes[0, sel[1]] = boxes[0, sel[0]]                                  # the second box suppressed by the first
    out = oracle_proposals(logits, boxes, nms_cfg(nms_pre=10, nms_post=20))
    assert out["count"][0] == 9 and list(out["index"][0, :9]) == [sel[0]] + list(sel[2:10])
    out = oracle_proposals(logits, boxes, nms_cfg(nms_pre=1000, nms_post=400))    # pre above N: every anchor
    assert out["count"][1] == N


def test_roi_oracle_rules():
    boxes = _far_boxes(8)
    s = np.array([0.3, -0.0, 0.5, np.nan, 0.3, -1.5, 0.0, 2.5], F32)     # composed scores: negative and above 1
    assert list(oracle_roi(s, boxes, 100, 100, None, 0.1)) == [7, 2, 0, 4, 1, 6, 5]            # no threshold: all but NaN
    assert list(oracle_roi(s, boxes, 100, 100, 0.0, 0.1)) == [7, 2, 0, 4, 1, 6]                # -0.0 >= 0.0
    assert list(oracle_roi(s, boxes, 100, 100, 0.3, 0.1)) == [7, 2, 0, 4]                      # inclusive
    assert list(oracle_roi(s, boxes, 3, 100, None, 0.1)) == [7, 2, 0]
    assert list(oracle_roi(s, boxes, 100, 2, None, 0.1)) == [7, 2]
    assert list(oracle_roi(s, boxes, 100, 100, 3.0, 0.1)) == []
    boxes[2] = boxes[7]
    assert list(oracle_roi(s, boxes, 100, 100, 0.3, 0.1)) == [7, 0, 4]


@pytest.mark.parametrize("score_type", SR.SCORE_TYPES)
def test_roi_oracle_reproduces_the_reference(score_type):
    """g46: the reference's own SECONDNetIoU.post_processing for every SCORE_TYPE -- from its inputs and the NMS scores of
    tests/second_head_ref.py the oracle selects the same rows in the same order, both frames"""
    from com_amd.postprocess import roi_static_settings
    g = np.load(os.path.join(GOLDEN, "g46_second_postproc.npz"))
    cfg = SR.post_process_cfg(score_type)
    s = roi_static_settings(cfg, second_iou=True)
    assert s["score_type"] == (score_type or 'iou')
    for b in range(2):
        scores = SR.nms_scores(score_type, g["iou_logits"][b, :, 0], g["cls_logits"][b], g["labels"][b], g["counts"][b],
                               cfg['NMS_CONFIG'], SR.CLASS_NAMES)
        keep = oracle_roi(scores, g["boxes"][b], s["nms_pre"], s["nms_post"], s["score_thresh"], s["nms_thresh"], s["nms_normal"])
        tag = f"{score_type or 'absent'}_{b}"
        np.testing.assert_array_equal(keep, g[f"{tag}_selected"])
        np.testing.assert_allclose(scores[keep], g[f"{tag}_pred_scores"], atol=1e-6, rtol=0)


# ------------------------------------------------------------------------------------------------------------ settings
def test_proposal_settings_and_refusals_name_the_key():
    from com_amd import _lib as L
    from com_amd.postprocess import roi_proposal_settings
    s = roi_proposal_settings(nms_cfg())
    assert s == dict(nms_pre=1024, nms_post=100, nms_thresh=0.7, nms_normal=0)
    assert roi_proposal_settings(nms_cfg(nms_type='nms_normal_gpu', nms_pre=L.POSTPROC_MAX_K))["nms_normal"] == 1
    for key, bad in (("MULTI_CLASSES_NMS", nms_cfg(multi=True)), ("NMS_TYPE", nms_cfg(nms_type='circle_nms')),
                     ("NMS_PRE_MAXSIZE", nms_cfg(nms_pre=9000)), ("NMS_PRE_MAXSIZE", nms_cfg(nms_pre=0)),
                     ("NMS_POST_MAXSIZE", nms_cfg(nms_post=0)), ("NMS_CONFIG", None)):
        with pytest.raises(L.PcdError, match=key):
            roi_proposal_settings(bad)


def test_roi_settings_and_refusals_name_the_key():
    from com_amd import _lib as L
    from com_amd.postprocess import roi_static_settings
    s = roi_static_settings(post_cfg(), second_iou=True)
    assert (s["score_type"], s["score_thresh"], s["nms_pre"], s["nms_post"], s["nms_thresh"], s["nms_normal"]) == \
        ('iou', 0.1, 4096, 500, 0.01, 0)
    assert roi_static_settings(post_cfg(SCORE_TYPE='cls'), second_iou=False)["score_type"] == 'rcnn'
    assert roi_static_settings(post_cfg(score_thresh=None), second_iou=False)["score_thresh"] is None
    s = roi_static_settings(post_cfg(SCORE_TYPE='weighted_iou_cls', SCORE_WEIGHTS=dict(iou=0.7, cls=0.3)), second_iou=True)
    assert s["score_type"] == 'weighted_iou_cls' and s["weights"] == (0.7, 0.3)
    by = dict(Car='iou', Pedestrian='cls')
    assert roi_static_settings(post_cfg(SCORE_TYPE='score_by_class', SCORE_BY_CLASS=by), second_iou=True)["by_class"] == by
    s = roi_static_settings(post_cfg(SCORE_TYPE='num_pts_iou_cls', SCORE_THRESH=dict(cls=5, iou=60)), second_iou=True)
    assert s["pts"] == (5, 60)
    for key, bad in (("MULTI_CLASSES_NMS", post_cfg(multi=True)), ("OUTPUT_RAW_SCORE", post_cfg(raw=True)),
                     ("NMS_TYPE", post_cfg(nms_type='circle_nms')), ("NMS_PRE_MAXSIZE", post_cfg(nms_pre=L.POSTPROC_MAX_K + 1)),
                     ("NMS_PRE_MAXSIZE", post_cfg(nms_pre=0)), ("NMS_POST_MAXSIZE", post_cfg(nms_post=-1)),
                     ("SCORE_TYPE", post_cfg(SCORE_TYPE='max')), ("SCORE_TYPE", post_cfg(SCORE_TYPE='rcnn')),
                     ("SCORE_BY_CLASS", post_cfg(SCORE_TYPE='score_by_class')),
                     ("SCORE_BY_CLASS.Car", post_cfg(SCORE_TYPE='score_by_class', SCORE_BY_CLASS=dict(Car='max'))),
                     ("SCORE_WEIGHTS", post_cfg(SCORE_TYPE='weighted_iou_cls')),
                     ("SCORE_THRESH", post_cfg(SCORE_TYPE='num_pts_iou_cls')),
                     ("SCORE_THRESH.iou", post_cfg(SCORE_TYPE='num_pts_iou_cls', SCORE_THRESH=dict(cls=60, iou=5)))):
        with pytest.raises(L.PcdError, match=key):
            roi_static_settings(bad, second_iou=True)
    with pytest.raises(L.PcdError, match="POST_PROCESSING"):
        roi_static_settings(None, second_iou=True)


def _roi_batch(R=8, device="cpu"):
    return {'batch_size': 2, 'batch_box_preds': torch.zeros(2, R, 7, device=device), 'batch_cls_preds': torch.zeros(2, R, 1, device=device),
            'roi_scores': torch.zeros(2, R, device=device), 'roi_labels': torch.ones(2, R, dtype=torch.long, device=device),
            'has_class_labels': True, 'cls_preds_normalized': False}


def test_static_functions_refuse_host_tensors_and_stacked_predictions():
    from com_amd import _lib as L
    from com_amd import postprocess
    with pytest.raises(L.PcdError, match="no CPU fallback"):
        postprocess.roi_predictions_static(_roi_batch(), post_cfg(), second_iou=True)
    with pytest.raises(L.PcdError, match="MULTI_CLASSES_NMS"):                 # (the settings are checked first)
        postprocess.roi_predictions_static(_roi_batch(), post_cfg(multi=True), second_iou=True)
    bd = _roi_batch()
    bd['batch_index'] = torch.zeros(16, dtype=torch.long)
    with pytest.raises(L.PcdError, match="batch_index"):
        postprocess.roi_predictions_static(bd, post_cfg(), second_iou=True)
    z = torch.zeros(1, 2, 2, 6)
    with pytest.raises(L.PcdError, match="no CPU fallback"):
        postprocess.anchor_proposals_static(None, z, z, None, nms_cfg())
    with pytest.raises(L.PcdError, match="NMS_PRE_MAXSIZE"):
        postprocess.anchor_proposals_static(None, z, z, None, nms_cfg(nms_pre=9000))


def test_to_pred_dicts_carries_the_second_iou_record():
    from com_amd.postprocess import to_pred_dicts
    static = {"boxes": torch.arange(2 * 3 * 7, dtype=torch.float32).view(2, 3, 7), "scores": torch.rand(2, 3),
              "labels": torch.ones(2, 3, dtype=torch.long), "count": torch.tensor([2, 0], dtype=torch.int32)}
    assert set(to_pred_dicts(static)[0]) == {'pred_boxes', 'pred_scores', 'pred_labels'}
    static.update(cls_scores=torch.rand(2, 3), iou_scores=torch.rand(2, 3))
    pred = to_pred_dicts(static)
    assert set(pred[0]) == {'pred_boxes', 'pred_scores', 'pred_labels', 'pred_cls_scores', 'pred_iou_scores'}
    assert torch.equal(pred[0]['pred_iou_scores'], static["iou_scores"][0, :2]) and pred[1]['pred_cls_scores'].numel() == 0


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_the_entry_points():
    from com_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "pcd_ops.h")).read()
    for name in ("pcd_anchor_proposals", "pcd_anchor_proposals_workspace_bytes", "pcd_roi_postproc",
                 "pcd_roi_postproc_workspace_bytes"):
        assert name + "(" in text and name in L.PROTOTYPES
    assert L.PROTOTYPES["pcd_anchor_proposals_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_void_p])
    assert L.PROTOTYPES["pcd_roi_postproc_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_void_p])
    assert len(L.PROTOTYPES["pcd_anchor_proposals"][1]) == 15 and len(L.PROTOTYPES["pcd_roi_postproc"][1]) == 15
    assert "typedef struct PcdAnchorProposalsConfig" in text and "typedef struct PcdRoiPostprocConfig" in text
    assert [L.CONSTANTS[k] for k in ("PCD_ROIPP_SCORE_RCNN", "PCD_ROIPP_SCORE_IOU", "PCD_ROIPP_SCORE_CLS", "PCD_ROIPP_SCORE_WEIGHTED",
                                     "PCD_ROIPP_SCORE_BY_CLASS", "PCD_ROIPP_SCORE_NUM_PTS")] == list(range(6))
    assert "roi_proposals.hip" in open(os.path.join(ROOT, "com_amd", "csrc", "Makefile")).read()


def _proposal_cfg(**kw):
    from com_amd.postprocess import PcdAnchorProposalsConfig
    cfg = PcdAnchorProposalsConfig()
    cfg.batch, cfg.height, cfg.width, cfg.n_kinds, cfg.n_classes, cfg.num_class, cfg.num_dir_bins = 2, 23, 37, 6, 3, 3, 2
    cfg.nms_pre, cfg.nms_post, cfg.nms_normal, cfg.nms_thresh = 1024, 100, 0, 0.7
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _roi_cfg(**kw):
    from com_amd.postprocess import PcdRoiPostprocConfig
    cfg = PcdRoiPostprocConfig()
    cfg.batch, cfg.rois, cfg.score_type, cfg.num_class = 2, 100, 1, 3
    cfg.nms_pre, cfg.nms_post, cfg.nms_normal, cfg.nms_thresh = 4096, 500, 0, 0.01
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_c_abi_workspace_queries_refuse():
    from com_amd import _lib as L
    lib = L.lib()
    q = lambda fn, cfg: int(fn(ctypes.cast(ctypes.pointer(cfg), ctypes.c_void_p)))
    pw, rw = lib.pcd_anchor_proposals_workspace_bytes, lib.pcd_roi_postproc_workspace_bytes
    assert q(pw, _proposal_cfg()) > 0 and q(pw, _proposal_cfg()) % 256 == 0
    assert q(pw, _proposal_cfg(nms_pre=L.POSTPROC_MAX_K)) > 0
    assert q(pw, _proposal_cfg(height=2, width=2)) < q(pw, _proposal_cfg())       # K = min(nms_pre, N)
    for bad in (dict(nms_pre=L.POSTPROC_MAX_K + 1), dict(nms_pre=9000), dict(nms_pre=0), dict(nms_post=0), dict(batch=0),
                dict(height=0), dict(nms_normal=2), dict(num_class=0), dict(n_kinds=0)):
        assert q(pw, _proposal_cfg(**bad)) == 0, bad
    assert int(pw(None)) == 0 and int(rw(None)) == 0
    assert q(rw, _roi_cfg()) > 0 and q(rw, _roi_cfg()) % 256 == 0
    assert q(rw, _roi_cfg(rois=L.POSTPROC_MAX_K)) > 0 and q(rw, _roi_cfg(rois=1)) > 0
    for bad in (dict(rois=L.POSTPROC_MAX_K + 1), dict(rois=0), dict(nms_pre=0), dict(nms_post=0), dict(batch=0), dict(nms_normal=-1),
                dict(score_type=6), dict(score_type=-1), dict(score_type=4, num_class=0), dict(score_type=4, num_class=17),
                dict(score_type=5, pts_cls_thresh=60.0, pts_iou_thresh=5.0)):
        assert q(rw, _roi_cfg(**bad)) == 0, bad


# ------------------------------------------------------------------------------------------------------------ adoption
def test_adopt_second_iou_detector():
    import stock_detector as SD
    from com_amd import adopt, hotpath
    from com_amd.hotpath.second_head import SECONDHead
    torch.manual_seed(0)
    model = SD.build_detector("second_iou")
    assert type(model.roi_head).__name__ == "SECONDHead" and not isinstance(model.roi_head, SECONDHead)
    assert model.module_list[-1] is model.roi_head
    reference = {k: v.clone() for k, v in model.state_dict().items()}
    before = {k: v for k, v in model.state_dict(keep_vars=True).items()}
    assert any(k.startswith("roi_head.shared_fc_layer.") for k in before) and "roi_head.iou_layers.7.bias" in before
    report = adopt.adopt_model(model)
    assert report.complete and ("roi_head", "SECONDHead", "com_amd.hotpath.SECONDHead") in report.replaced
    assert type(model.roi_head) is SECONDHead and model.module_list[-1] is model.roi_head
    assert isinstance(model.dense_head, hotpath.AnchorHeadSingle)
    after = {k: v for k, v in model.state_dict(keep_vars=True).items()}
    assert list(after) == list(before)
    for k, t in before.items():
        assert after[k] is t and tuple(after[k].shape) == tuple(t.shape), k
    head = model.roi_head
    assert (head.grid_size, head.in_channel, head.num_class) == (7, 512, 1)
    # (the geometry of the BEV map: the detector keeps its range in fp32, as the reference's dataset does)
    assert head.point_cloud_range == [float(F32(v)) for v in SD.synth.WAYMO_RANGE] and head.voxel_size == list(SD.synth.WAYMO_VOXEL)
    again = adopt.adopt_model(model)                                              # adopting twice is a no-op
    assert not again.replaced and ("roi_head", "SECONDHead") in again.kept and model.roi_head is head
    model.load_state_dict(reference, strict=True)                                 # a reference-shaped state dict still loads


def test_adopt_refuses_a_second_head_it_cannot_match():
    import stock_detector as SD
    from com_amd import _lib as L
    from com_amd import adopt
    model = SD.build_detector("second_iou")
    model.roi_head.iou_layers[7] = torch.nn.Conv1d(256, 2, kernel_size=1)
    with pytest.raises(L.PcdError, match=r"roi_head\.iou_layers\.7"):
        adopt.adopt_model(model)
    report = adopt.adopt_model(model, strict=False)
    assert not report.complete and report.unrecognised[0][0].startswith("roi_head")


# ------------------------------------------------------------------------------------------------------------ refusals
def _vox():
    import stock_detector as SD
    from com_amd import train
    return train.VoxelizeConfig(SD.synth.WAYMO_RANGE, SD.synth.WAYMO_VOXEL, 5, 150000)


def test_captured_inference_refusals_without_a_device():
    import stock_detector as SD
    from com_amd import _lib as L
    from com_amd import adopt, infer
    model = SD.build_detector("second_iou")
    with pytest.raises(L.PcdError, match="roi_head"):                          # unadopted: the stock classes
        infer.CapturedInference(model, _vox(), 2)
    adopt.adopt_model(model)
    inf = infer.CapturedInference(model, _vox(), 2)                            # both settings blocks are accepted
    assert inf.proposal_cfg is model.roi_head.model_cfg.NMS_CONFIG.TEST and inf.post_cfg is model.model_cfg.POST_PROCESSING
    assert inf.class_names == SD.CLASS_NAMES
    model.roi_head.model_cfg.NMS_CONFIG.TEST['NMS_PRE_MAXSIZE'] = 9000
    with pytest.raises(L.PcdError, match="NMS_PRE_MAXSIZE"):
        infer.CapturedInference(model, _vox(), 2)
    model.roi_head.model_cfg.NMS_CONFIG.TEST['NMS_PRE_MAXSIZE'] = 1024
    nms = model.model_cfg.POST_PROCESSING.NMS_CONFIG
    nms['MULTI_CLASSES_NMS'] = True
    with pytest.raises(L.PcdError, match="MULTI_CLASSES_NMS"):
        infer.CapturedInference(model, _vox(), 2)
    nms['MULTI_CLASSES_NMS'] = False
    nms['SCORE_TYPE'] = 'max'
    with pytest.raises(L.PcdError, match="SCORE_TYPE"):
        infer.CapturedInference(model, _vox(), 2)
    nms.update(SCORE_TYPE='num_pts_iou_cls', SCORE_THRESH=dict(cls=5, iou=60))
    with pytest.raises(L.PcdError, match="num_pts_iou_cls"):
        infer.CapturedInference(model, _vox(), 2)
    del nms['SCORE_TYPE'], nms['SCORE_THRESH']
    roi = model.roi_head
    model.roi_head = torch.nn.Identity()
    with pytest.raises(L.PcdError, match="roi_head"):
        infer.CapturedInference(model, _vox(), 2)
    model.roi_head = roi
    model.point_head = torch.nn.Identity()
    with pytest.raises(L.PcdError, match="point_head"):
        infer.CapturedInference(model, _vox(), 2)
    model.point_head = None
    model.dense_head = None
    with pytest.raises(L.PcdError, match="roi_head"):                          # a RoI head with no anchor head in front
        infer.CapturedInference(model, _vox(), 2)
    model.roi_head = None
    with pytest.raises(L.PcdError, match="centre head"):
        infer.CapturedInference(model, _vox(), 2)


def test_captured_step_refuses_a_roi_head_by_name():
    import stock_detector as SD
    from com_amd import _lib as L
    from com_amd import adopt, train
    model = SD.build_detector("second_iou")
    adopt.adopt_model(model)
    with pytest.raises(L.PcdError, match="roi_head"):
        train.CapturedStep(model, None, None, _vox(), 2)


def test_heads_without_the_keys_are_unchanged():
    """the RoI heads' helper is a no-op without `static_predictions`; the anchor head pops `static_proposal_cfg` in training
    mode without honouring it (checked on the GPU); the helper demands the detector's POST_PROCESSING block"""
    from com_amd import _lib as L
    from com_amd.hotpath.second_head import SECONDHead
    head = SECONDHead(6, SR.model_cfg(), num_class=1)
    bd = _roi_batch()
    assert head.static_post_processing(bd, second_iou=True) is bd and 'final_box_tensors' not in bd
    bd['static_predictions'] = True
    with pytest.raises(L.PcdError, match="post_process_cfg"):
        head.static_post_processing(bd, second_iou=True)
    assert 'static_predictions' not in bd
