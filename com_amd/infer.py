"""The inference step of the hot path as a product object: the body of the reference's eval loop
(tools/eval_utils/eval_utils.py:58-80)

    model.eval()
    with torch.no_grad():
        pred_dicts, ret_dict = model(batch_dict)        ->  out = infer(batch)      -- ONE graph replay
    (CenterHead.generate_predicted_boxes -> class_agnostic_nms -> nms_gpu inside the forward; for an anchor-head detector
     AnchorHeadSingle / AnchorHeadMulti.generate_predicted_boxes, then Detector3DTemplate.post_processing after it -- for
     the multi head its per-frame, per-head, per-class multi_classes_nms loop; for SECOND-IoU -- AnchorHeadSingle ->
     SECONDHead -- RoIHeadTemplate.proposal_layer inside the RoI head's forward and SECONDNetIoU.post_processing after it)
                                                         ->  preds = infer.pred_dicts(out)   (final_box_dicts)

`CapturedInference` mirrors com_amd.train.CapturedStep and reuses its pieces (VoxelizeConfig, ops.StaticPlan, the in-graph
voxeliser): capacities are observed during eager warm-up forwards, then voxelise -> `module_list` forward (eval mode,
no_grad, `static_predictions=True`) -> the static post-processing of com_amd.postprocess is captured as one hipGraph.  A
two-stage detector is handed `static_proposal_cfg` too: its anchor head writes the RoIs straight from its maps
(pcd_anchor_proposals), its RoI head the final boxes (pcd_roi_postproc).
Every replay predicts the batch handed to that call (no one-behind staging as in training).

Weights and BatchNorm statistics are read live by every replay: the captured forward packs the sparse and dense weight packs
from the parameters inside the graph (packs left behind by a training step are dropped before the capture), so an in-place
update (an optimizer step, load_state_dict, copy_) reaches the next replay without a recapture.  A parameter or buffer whose
storage moved raises.  The eval forward runs `model.module_list` (Detector3DTemplate.forward's loop) rather than
`model.forward`, whose post_processing / recall statistics read results back to the host."""
import torch

from . import _lib as L
from . import adopt, ops, postprocess, train
from .hotpath.anchor_head import AnchorHeadSingle
from .hotpath.anchor_head_multi import AnchorHeadMulti
from .hotpath.center_head import BoxDecodeMixin
from .hotpath.dense2d import _get
from .hotpath.second_head import SECONDHead


def _offsets(offs, dev):
    """frame offsets as the graph's int32 device tensor (a batch may carry a list, as hotpath.collate_points returns it)"""
    if torch.is_tensor(offs):
        return offs.to(device=dev, dtype=torch.int32)
    return torch.tensor(list(offs), dtype=torch.int32).to(dev)


class CapturedInference:
    """model      a detector adopted with com_amd.adopt.adopt_model whose `dense_head` offers the static post-processing: a
               centre head (BoxDecodeMixin; its own POST_PROCESSING), an AnchorHeadSingle / curriculum anchor head
               (class-agnostic NMS) or an AnchorHeadMulti (MULTI_CLASSES_NMS: per-class NMS as B x num_class selection
               problems); the anchor heads take the detector's `model_cfg.POST_PROCESSING`, handed to every forward as
               `post_process_cfg`.  One two-stage form is accepted: a fused SECONDHead as `roi_head` behind a fused
               AnchorHeadSingle (SECOND-IoU); both settings blocks -- the RoI head's NMS_CONFIG.TEST, handed to every
               forward as `static_proposal_cfg`, and POST_PROCESSING with its SCORE_TYPE -- are validated before anything
               runs, and the output carries `cls_scores` / `iou_scores` too.  Any other `roi_head`, a `point_head`, and an
               AnchorHeadMulti that is not the fused class are refused.
    voxelize   com_amd.train.VoxelizeConfig.
    batch_size frames per call.
    margin     capacity over the observed row counts (ops.StaticPlan)."""

    def __init__(self, model, voxelize, batch_size, margin=1.25):
        head = getattr(model, "dense_head", None)
        roi_head = getattr(model, "roi_head", None)
        if getattr(model, "point_head", None) is not None:
            raise L.PcdError(f"CapturedInference: the model has a point_head ({type(model.point_head).__name__}): "
                             "point-based second stages are not supported")
        if roi_head is not None and not (type(roi_head) is SECONDHead and isinstance(head, AnchorHeadSingle)):
            raise L.PcdError(f"CapturedInference: the model has a roi_head ({type(roi_head).__name__}) behind a "
                             f"{type(head).__name__}: the only two-stage detector supported is a fused SECONDHead behind a "
                             "fused AnchorHeadSingle (adopt_model(model) first)")
        if type(head).__name__ == "AnchorHeadMulti" and not isinstance(head, AnchorHeadMulti):
            raise L.PcdError("CapturedInference: the dense head is an AnchorHeadMulti that is not com_amd.hotpath's (the stock "
                             "class has no static post-processing): adopt_model(model) first")
        report = adopt.adopt_report(model)
        if report is None:
            raise L.PcdError("CapturedInference: adopt_model(model) first")
        if report.unrecognised:
            raise L.PcdError(f"CapturedInference: the model has modules adopt_model() left unfused: {report.unrecognised}")
        self.post_cfg = self.proposal_cfg = self.class_names = None
        if isinstance(head, BoxDecodeMixin):
            postprocess.static_settings(head)                # (refuses circle_nms / oversize K before anything runs)
        elif isinstance(head, (AnchorHeadSingle, AnchorHeadMulti)):
            self.post_cfg = _get(getattr(model, "model_cfg", None), "POST_PROCESSING", None)
            if self.post_cfg is None:
                raise L.PcdError("CapturedInference: an anchor-head detector needs model.model_cfg.POST_PROCESSING")
            # (refuse before anything runs: the single head MULTI_CLASSES_NMS, the multi head its absence; oversize K)
            if roi_head is not None:
                # both settings blocks of the two-stage path: the RoI head's proposals, the detector's final NMS
                self.proposal_cfg = _get(_get(roi_head.model_cfg, "NMS_CONFIG"), "TEST")
                postprocess.roi_proposal_settings(self.proposal_cfg)
                s = postprocess.roi_static_settings(self.post_cfg, second_iou=True)
                if s["score_type"] == "num_pts_iou_cls":
                    raise L.PcdError("CapturedInference: NMS_CONFIG.SCORE_TYPE = 'num_pts_iou_cls' is not supported (it counts "
                                     "batch_dict['points'] rows with a batch column; the in-graph voxeliser hands the model "
                                     "none)")
                if int(_get(self.proposal_cfg, "NMS_POST_MAXSIZE")) > L.POSTPROC_MAX_K:
                    raise L.PcdError(f"CapturedInference: roi_head NMS_CONFIG.TEST.NMS_POST_MAXSIZE above the cap "
                                     f"{L.POSTPROC_MAX_K} (the RoI rows of a frame are sorted in LDS)")
                self.class_names = list(getattr(model, "class_names", None) or getattr(head, "class_names", []))
            elif isinstance(head, AnchorHeadMulti):
                postprocess.anchor_multi_static_settings(self.post_cfg)
            else:
                postprocess.anchor_static_settings(self.post_cfg)
        else:
            raise L.PcdError("CapturedInference: the model needs a dense_head with a static post-processing (a centre head, "
                             f"an AnchorHeadSingle or an AnchorHeadMulti), got {type(head).__name__}")
        self.model, self.head, self.vox_cfg, self.batch_size = model, head, voxelize, int(batch_size)
        self.plan = ops.StaticPlan(margin=margin)
        self.feature_stride = train.feature_stride(model, voxelize)
        self.captured = False
        self.recaptures = 0
        self._g = {}
        self._example = None

    # ------------------------------------------------------------------ pieces
    def _voxelize(self, pts, offs):
        return train.voxelize_batch(self.vox_cfg, self.batch_size, self.feature_stride, pts, offs)[1]

    def _forward(self, bd2):
        """module_list forward in eval mode under no_grad with the static post-processing -> its padded tensors"""
        bd = {k: v for k, v in bd2.items() if k != "_result"}
        bd["static_predictions"] = True
        if self.post_cfg is not None:
            bd["post_process_cfg"] = self.post_cfg
        if self.proposal_cfg is not None:
            bd["static_proposal_cfg"] = self.proposal_cfg
            bd["class_names"] = self.class_names
        with torch.no_grad():
            modules = getattr(self.model, "module_list", None)
            if modules is None:
                out = self.model(bd)
                bd = out[0] if isinstance(out, tuple) else out
            else:
                for m in modules:
                    bd = m(bd)
        if "final_box_tensors" not in bd:
            raise L.PcdError("CapturedInference: the heads did not produce final_box_tensors")
        return bd["final_box_tensors"]

    def _drop_packs_ahead(self):
        """Weight packs a training step made ahead (backbone pack_after_update, Conv3x3Packs.run) are used by the next
        forward instead of packing: drop them, so that the forward -- and the graph -- packs from the live parameters."""
        for m in self.model.modules():
            if hasattr(m, "forget_packs_ahead"):
                m.forget_packs_ahead()
            if getattr(m, "_packs_ahead", None) is not None:
                m._packs_ahead = None

    class _Eval:
        """eval mode for the duration; every module's own `training` flag restored afterwards"""

        def __init__(self, model):
            self.model, self.flags = model, None

        def __enter__(self):
            self.flags = [(m, m.training) for m in self.model.modules()]
            self.model.eval()
            return self

        def __exit__(self, *exc):
            for m, t in self.flags:
                m.training = t
            return False

    def _state_ptrs(self):
        return [(n, t.data_ptr()) for n, t in list(self.model.named_parameters()) + list(self.model.named_buffers())]

    # ------------------------------------------------------------------ eager execution
    def eager(self, batch):
        """Voxelise -> eval forward -> static post-processing with one launch per kernel (observes the row counts for the
        plan while it is not active).  Returns the padded dict (decode_predictions_static)."""
        pts, offs = train._split_batch(batch)
        with self._Eval(self.model), self.plan:
            self._drop_packs_ahead()
            return self._forward(self._voxelize(pts, offs))

    # ------------------------------------------------------------------ capture
    def capture(self, example_batch, validate=None, attempts=3):
        """Eager warm-up forwards over the example (and `validate`) batches observe the row counts (unless earlier eager()
        calls did), then one graph is captured for batches of up to `example_batch`'s point rows.  `validate` batches are
        replayed right after the capture; a capacity overflow among them grows the plan (x 1.5) and captures again, up to
        `attempts` times."""
        if not self.plan.caps:                               # (nothing observed yet: eager() calls before capture() count)
            for b in [example_batch] + list(validate or []):
                self.eager(b)
        self._example = example_batch
        for _ in range(attempts):
            self._build(example_batch)
            if not validate:
                return self
            for b in validate:
                self(b)
            torch.cuda.synchronize()
            if not self.plan.poll(wait=True):
                break
            self.recaptures += 1                             # a batch denser than the observed ones: larger capacities
            self.release()
            self.plan.grow(1.5)
        self.plan.check()
        return self

    def recapture(self):
        """After an overflow (`poll()` returned True / `check()` raised): larger capacities, capture again."""
        self.recaptures += 1
        self.release()
        self.plan.grow(1.5)
        self._build(self._example)

    def release(self):
        self.plan.active = False
        self.captured = False
        self._g = {}

    def _build(self, example_batch):
        pts0, offs0 = train._split_batch(example_batch)
        dev = pts0.device
        plan, g = self.plan, {}
        plan.active = True
        plan.prepare(dev)                                    # the sticky flag lives outside the graph's pool
        g["s_pts"] = s_pts = pts0.clone()
        g["s_offs"] = s_offs = _offsets(offs0, dev).clone()
        with self._Eval(self.model), plan:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                    # static-shape forwards outside a capture: allocator + caches warm
                for _ in range(2):
                    self._drop_packs_ahead()
                    self._forward(self._voxelize(s_pts, s_offs))
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            plan.recorded.clear()
            self._drop_packs_ahead()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                g["out"] = self._forward(self._voxelize(s_pts, s_offs))
                plan.arm()                                   # sticky overflow check of every replay, inside the graph
        g["graph"] = graph
        g["ptrs"] = self._state_ptrs()
        self._g = g
        self.captured = True

    # ------------------------------------------------------------------ the loop's calls
    def _stage(self, batch):
        g = self._g
        pts, offs = train._split_batch(batch)
        n = pts.shape[0]
        if n > g["s_pts"].shape[0]:
            raise L.PcdError(f"CapturedInference: batch has {n} point rows, the graph was captured for "
                             f"{g['s_pts'].shape[0]}")
        offs = _offsets(offs, g["s_offs"].device)
        if offs.numel() != g["s_offs"].numel():
            raise L.PcdError(f"CapturedInference: {offs.numel() - 1} frames, captured for {g['s_offs'].numel() - 1}")
        (g["s_pts"] if n == g["s_pts"].shape[0] else g["s_pts"][:n]).copy_(pts, non_blocking=True)
        g["s_offs"].copy_(offs, non_blocking=True)           # (rows behind offs[-1] are never read)

    def __call__(self, batch):
        """Predictions for `batch`: the padded dict of com_amd.postprocess (device tensors, valid until the next call)."""
        if not self.captured:
            return self.eager(batch)
        g = self._g
        if self._state_ptrs() != g["ptrs"]:
            moved = [n for (n, p), (_, q) in zip(self._state_ptrs(), g["ptrs"]) if p != q]
            raise L.PcdError(f"CapturedInference: parameters / buffers moved since the capture ({moved[:4]}...): "
                             "update them in place (copy_, load_state_dict) or recapture()")
        self._stage(batch)
        g["graph"].replay()
        return g["out"]

    @staticmethod
    def pred_dicts(out):
        """The reference's final_box_dicts from a call's output (one device -> host copy of the counts)."""
        return postprocess.to_pred_dicts(out)

    def poll(self):
        """Sticky device-side overflow flag, read without stalling: True (overflow seen), False, or None (no result yet)."""
        return self.plan.poll() if self.captured else False

    def check(self):
        """Synchronous form: raises PcdError if any replay exceeded a capacity."""
        return self.plan.check() if self.captured else True
