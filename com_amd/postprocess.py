"""Static post-processing of a centre head: the eval half of CenterHead / CurriculumCenterHead (center_head.py:266-317 ->
centernet_utils.py:199-257 -> model_nms_utils.py:15-27 -> iou3d_nms_utils.py:85-116) for ALL frames and heads of a batch in
one call into com_amd/csrc/postproc.hip: fixed launches, nothing read back, nothing allocated but the outputs and the
workspace -- so it can sit inside a captured inference graph (com_amd.infer.CapturedInference).

    static = decode_predictions_static(pred_dicts, head)   # padded device tensors
    final_box_dicts = to_pred_dicts(static)                 # the reference's per-frame list (one device -> host copy)

`static` holds boxes f32 [B, M, 7 | 9], scores f32 [B, M], labels int64 [B, M] (class_id_mapping_each_head[h][c] + 1) and
count int32 [B]; M = number of heads x NMS_POST_MAXSIZE, rows behind count are zero, each frame's rows are its heads' kept
boxes in head order, each head's in score order.  Selection order: score descending, then flat index c*H*W + y*W + x
ascending (torch.topk leaves ties unordered; with distinct scores both agree).

The anchor-head counterpart (AnchorHeadSingle and its curriculum forms; com_amd/csrc/anchor_postproc.hip) replaces
generate_predicted_boxes + Detector3DTemplate.post_processing (anchor_head_template.py:229-276, detector3d_template.py:178-290,
model_nms_utils.py:6-25) the same way, one selection problem per frame:

    static = anchor_predictions_static(head, cls_preds, box_preds, dir_cls_preds, post_process_cfg)

with the same dict layout (M = NMS_POST_MAXSIZE, boxes [B, M, 7]), so `to_pred_dicts` serves both.  Its rules, as a total
order: score_c = fp32 sigmoid of the class logit (bf16 widened first); an anchor's score is the maximum over its num_class
scores and its label the lowest class index that attains it, + 1; with SCORE_THRESH an anchor passes iff score >=
SCORE_THRESH (INCLUSIVE, model_nms_utils.py:9 -- the centre path above is exclusive), without it every anchor passes; a NaN
score never passes (the one deliberate difference from torch.topk, which ranks NaN first); the first
min(NMS_PRE_MAXSIZE, passing) anchors are taken by score descending, then anchor index n = (y * W + x) * A + kind ascending;
only those are decoded (the arithmetic of pcd_anchor_decode: one device function); nms_gpu / nms_normal_gpu runs over them in
that order on columns 0:7 and the first NMS_POST_MAXSIZE survivors are written in keep order.  No [B, N, 7] and no
[B, N, num_class] tensor exists on this path.

The multi-head anchor counterpart (AnchorHeadMulti with MULTI_CLASSES_NMS; com_amd/csrc/anchor_multi_postproc.hip) replaces
the per-frame, per-head, per-class loop of detector3d_template.py:224-249 / model_nms_utils.py:28-66 by B x num_class
selection problems in the same fixed launches:

    static = anchor_multi_predictions_static(head, cls_maps, box_maps, dir_maps, post_process_cfg)

M = num_class x NMS_POST_MAXSIZE, boxes [B, M, 7 | 9]; per frame the classes' kept boxes in global class order (head order,
then class order inside the head).  Per (frame, class) the elements are the head's local anchors i = (a * H + y) * W + x (the
row order of batch_cls_preds[h]); score = fp32 sigmoid of the class logit; score >= SCORE_THRESH passes (inclusive, a NaN
never); order: score descending, then i ascending; the first min(NMS_PRE_MAXSIZE, passing) are decoded (the arithmetic of
pcd_anchor_multi_decode) and go through NMS; an anchor selected under two classes of a head appears twice, as in the
reference; labels through multihead_label_mapping.

The two-stage counterparts (a RoI head behind an AnchorHeadSingle; com_amd/csrc/roi_proposals.hip) replace the two host loops
of a RoI head's eval forward:

    prop = anchor_proposals_static(head, cls_preds, box_preds, dir_cls_preds, nms_config)      # ROI_HEAD.NMS_CONFIG.TEST
    static = roi_predictions_static(batch_dict, post_process_cfg, class_names, second_iou)

The first is RoIHeadTemplate.proposal_layer (roi_head_template.py:45-102) straight from the anchor head's maps: `rois`
[B, POST, 7], `roi_scores` [B, POST] (the anchor's maximum LOGIT, its own bits -- no sigmoid), `roi_labels` [B, POST] (1-based,
the lowest class at the maximum) and `count` [B]; no score threshold, a NaN never takes part, score descending then anchor
index, rows behind count are boxes 0 / scores 0 / labels 1 as the reference leaves them.  The second is the final
post-processing over ALL R RoI rows of a frame (detector3d_template.py:178-290 with roi_labels: score type 'rcnn'; or
second_net_iou.py:75-177: the five SCORE_TYPEs, both quirks of the reference kept): the same dict layout as above plus
`cls_scores` / `iou_scores` [B, M] for SECOND-IoU, which `to_pred_dicts` returns as pred_cls_scores / pred_iou_scores."""
import ctypes

import torch

from . import _lib as L
from .hotpath.dense2d import _get

MAPS = ("hm", "center", "center_z", "dim", "rot", "vel")
NMS_TYPES = {"nms_gpu": 0, "nms_normal_gpu": 1}
INDEX_LIMIT = 2 ** 31 - 4096          # C * H * W of a head map: flat indices are int32 on the device


def static_settings(head):
    """POST_PROCESSING of `head` as the kernel takes it; PcdError for what the static path refuses (circle_nms, other NMS
    types, MAX_OBJ_PER_SAMPLE or NMS_PRE_MAXSIZE above the LDS cap, too many heads / classes per head)."""
    pp = _get(head.model_cfg, 'POST_PROCESSING')
    nms = _get(pp, 'NMS_CONFIG')
    kind = _get(nms, 'NMS_TYPE')
    if kind == 'circle_nms':
        raise L.PcdError("static post-processing: NMS_TYPE circle_nms is not supported (the reference asserts False)")
    if kind not in NMS_TYPES:
        raise L.PcdError(f"static post-processing: NMS_TYPE {kind!r} (supported: {sorted(NMS_TYPES)})")
    s = dict(K=int(_get(pp, 'MAX_OBJ_PER_SAMPLE')), nms_pre=int(_get(nms, 'NMS_PRE_MAXSIZE')),
             nms_post=int(_get(nms, 'NMS_POST_MAXSIZE')), nms_thresh=float(_get(nms, 'NMS_THRESH')), nms_normal=NMS_TYPES[kind],
             score_thresh=_get(pp, 'SCORE_THRESH', None), limit=[float(v) for v in _get(pp, 'POST_CENTER_LIMIT_RANGE')],
             vel='vel' in _get(head.separate_head_cfg, 'HEAD_ORDER'), mapping=[list(m) for m in head.class_id_mapping_each_head])
    for key, v in (("MAX_OBJ_PER_SAMPLE", s["K"]), ("NMS_PRE_MAXSIZE", s["nms_pre"])):
        if v > L.POSTPROC_MAX_K:
            raise L.PcdError(f"static post-processing: {key} = {v} above the cap {L.POSTPROC_MAX_K} (the per-problem sort "
                             "runs in LDS)")
        if v < 1:
            raise L.PcdError(f"static post-processing: {key} = {v}")
    if s["nms_post"] < 1:
        raise L.PcdError(f"static post-processing: NMS_POST_MAXSIZE = {s['nms_post']}")
    if len(s["mapping"]) > L.POSTPROC_MAX_HEADS or any(len(m) > L.POSTPROC_MAX_CLASSES for m in s["mapping"]):
        raise L.PcdError(f"static post-processing: at most {L.POSTPROC_MAX_HEADS} heads of {L.POSTPROC_MAX_CLASSES} classes")
    if len(s["limit"]) != 6:
        raise L.PcdError("static post-processing: POST_CENTER_LIMIT_RANGE needs 6 values")
    return s


def _config(head, s, batch, height, width):
    cfg = L.PcdPostprocConfig()
    cfg.batch, cfg.num_heads, cfg.height, cfg.width = int(batch), len(s["mapping"]), int(height), int(width)
    cfg.max_obj, cfg.nms_pre, cfg.nms_post, cfg.nms_normal = s["K"], s["nms_pre"], s["nms_post"], s["nms_normal"]
    cfg.use_score_thresh = int(s["score_thresh"] is not None)
    cfg.score_thresh = float(s["score_thresh"]) if s["score_thresh"] is not None else 0.0
    cfg.nms_thresh = s["nms_thresh"]
    for i, v in enumerate(s["limit"]):
        cfg.limit[i] = v
    # (ctypes rounds each double to float: what torch does with a Python scalar in an fp32 op)
    cfg.feature_map_stride = float(head.feature_map_stride)
    cfg.voxel_x, cfg.voxel_y = float(head.voxel_size[0]), float(head.voxel_size[1])
    cfg.pc_x, cfg.pc_y = float(head.point_cloud_range[0]), float(head.point_cloud_range[1])
    return cfg


def decode_predictions_static(pred_dicts, head):
    """pred_dicts: the towers' per-head maps ({'hm', 'center', 'center_z', 'dim', 'rot'[, 'vel']}: [B, C, H, W] device
    tensors, f32 or bf16, any strides); head: the centre head (its POST_PROCESSING, feature_map_stride, voxel_size,
    point_cloud_range, class_id_mapping_each_head, HEAD_ORDER).  Returns {'boxes', 'scores', 'labels', 'count'} (module
    docstring)."""
    s = static_settings(head)
    if len(pred_dicts) != len(s["mapping"]):
        raise L.PcdError(f"static post-processing: {len(pred_dicts)} heads of maps, the head has {len(s['mapping'])}")
    hm0 = pred_dicts[0]['hm']
    B, H, W = hm0.shape[0], hm0.shape[2], hm0.shape[3]
    heads = (L.PcdPostprocHead * len(pred_dicts))()
    for h, (pd, mapping) in enumerate(zip(pred_dicts, s["mapping"])):
        C = pd['hm'].shape[1]
        if C != len(mapping):
            raise L.PcdError(f"static post-processing: head {h} has {C} heat-map channels, {len(mapping)} classes")
        if C * H * W > INDEX_LIMIT:
            raise L.PcdError(f"static post-processing: C*H*W = {C * H * W} does not fit the int32 flat index")
        for m, name in enumerate(MAPS):
            if name == 'vel' and not s["vel"]:
                continue
            t = pd[name]
            if not t.is_cuda:
                raise L.PcdError("static post-processing needs HIP device tensors (there is no CPU fallback)")
            if t.dim() != 4 or t.shape[0] != B or tuple(t.shape[2:]) != (H, W) or t.dtype not in (torch.float32, torch.bfloat16):
                raise L.PcdError(f"static post-processing: map {name!r} {tuple(t.shape)} {t.dtype}, want [{B}, c, {H}, {W}] "
                                 "f32 / bf16")
            heads[h].map[m] = t.data_ptr()
            for d in range(4):
                heads[h].strides[m][d] = t.stride(d)
            heads[h].dtype[m] = L.PCD_BF16 if t.dtype == torch.bfloat16 else L.PCD_F32
        heads[h].num_class = C
        for c, cls in enumerate(mapping):
            heads[h].label[c] = int(cls) + 1
    cfg = _config(head, s, B, H, W)
    lib = L.lib()
    hp, cp = ctypes.cast(heads, ctypes.c_void_p), ctypes.cast(ctypes.pointer(cfg), ctypes.c_void_p)
    nbytes = int(lib.pcd_centerhead_postproc_workspace_bytes(hp, cp))
    if nbytes == 0:
        raise L.PcdError("static post-processing: configuration refused by pcd_centerhead_postproc (include/pcd_ops.h)")
    dev = hm0.device
    M = len(pred_dicts) * s["nms_post"]
    D = 9 if s["vel"] else 7
    out = {"boxes": torch.empty((B, M, D), dtype=torch.float32, device=dev),
           "scores": torch.empty((B, M), dtype=torch.float32, device=dev),
           "labels": torch.empty((B, M), dtype=torch.int64, device=dev),
           "count": torch.empty((B,), dtype=torch.int32, device=dev)}
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    L.check(lib.pcd_centerhead_postproc(hp, cp, L.ptr(out["boxes"]), L.ptr(out["scores"]), L.ptr(out["labels"]),
                                        L.ptr(out["count"]), L.ptr(ws), nbytes, L.stream_ptr()), "pcd_centerhead_postproc")
    return out


class PcdAnchorPostprocConfig(ctypes.Structure):
    """include/pcd_ops.h: struct PcdAnchorPostprocConfig (POST_PROCESSING of an anchor-head detector + the head's
    shapes); the mirror lives beside its one user."""
    _fields_ = [("batch", ctypes.c_int), ("height", ctypes.c_int), ("width", ctypes.c_int), ("n_kinds", ctypes.c_int),
                ("n_classes", ctypes.c_int), ("num_class", ctypes.c_int), ("num_dir_bins", ctypes.c_int),
                ("nms_pre", ctypes.c_int), ("nms_post", ctypes.c_int), ("nms_normal", ctypes.c_int),
                ("use_score_thresh", ctypes.c_int), ("score_thresh", ctypes.c_float), ("nms_thresh", ctypes.c_float),
                ("dir_offset", ctypes.c_float), ("dir_limit_offset", ctypes.c_float)]


def _anchor_settings(pp, what, multi):
    """the keys both anchor heads read from a POST_PROCESSING block; `multi`: the value MULTI_CLASSES_NMS must have"""
    if pp is None:
        raise L.PcdError(f"{what}: no POST_PROCESSING block")
    nms = _get(pp, 'NMS_CONFIG')
    if bool(_get(nms, 'MULTI_CLASSES_NMS', False)) != multi:
        why = "per-head class scores have no class-agnostic maximum" if multi else "class-agnostic NMS only"
        raise L.PcdError(f"{what}: NMS_CONFIG.MULTI_CLASSES_NMS = {not multi} is not supported ({why})")
    if _get(pp, 'OUTPUT_RAW_SCORE', False):
        raise L.PcdError(f"{what}: OUTPUT_RAW_SCORE = True is not supported")
    kind = _get(nms, 'NMS_TYPE')
    if kind not in NMS_TYPES:
        raise L.PcdError(f"{what}: NMS_TYPE {kind!r} (supported: {sorted(NMS_TYPES)})")
    s = dict(nms_pre=int(_get(nms, 'NMS_PRE_MAXSIZE')), nms_post=int(_get(nms, 'NMS_POST_MAXSIZE')),
             nms_thresh=float(_get(nms, 'NMS_THRESH')), nms_normal=NMS_TYPES[kind], score_thresh=_get(pp, 'SCORE_THRESH', None))
    if s["nms_pre"] > L.POSTPROC_MAX_K:
        raise L.PcdError(f"{what}: NMS_PRE_MAXSIZE = {s['nms_pre']} above the cap {L.POSTPROC_MAX_K} (the per-problem sort runs "
                         "in LDS)")
    for key, v in (("NMS_PRE_MAXSIZE", s["nms_pre"]), ("NMS_POST_MAXSIZE", s["nms_post"])):
        if v < 1:
            raise L.PcdError(f"{what}: {key} = {v}")
    return s


def anchor_static_settings(post_process_cfg):
    """The POST_PROCESSING block of an anchor-head detector as pcd_anchor_postproc takes it; PcdError naming the key for what
    the static path refuses (MULTI_CLASSES_NMS, OUTPUT_RAW_SCORE, other NMS types, NMS_PRE_MAXSIZE above the LDS cap)."""
    return _anchor_settings(post_process_cfg, "static anchor post-processing", multi=False)


def anchor_postproc_config(s, tab, batch):
    """PcdAnchorPostprocConfig of settings `s` (anchor_static_settings) for the anchor tables `tab` of a head"""
    cfg = PcdAnchorPostprocConfig()
    cfg.batch, cfg.height, cfg.width, cfg.n_kinds, cfg.n_classes = int(batch), tab.H, tab.W, tab.A, tab.C
    cfg.num_class, cfg.num_dir_bins = tab.num_class, tab.num_dir_bins
    cfg.nms_pre, cfg.nms_post, cfg.nms_normal = s["nms_pre"], s["nms_post"], s["nms_normal"]
    cfg.use_score_thresh = int(s["score_thresh"] is not None)
    cfg.score_thresh = float(s["score_thresh"]) if s["score_thresh"] is not None else 0.0
    cfg.nms_thresh = s["nms_thresh"]
    cfg.dir_offset, cfg.dir_limit_offset = tab.dir_offset, tab.dir_limit_offset
    return cfg


def anchor_predictions_static(head, cls_preds, box_preds, dir_cls_preds, post_process_cfg):
    """head: an AnchorHeadSingle (its anchor tables); cls_preds / box_preds / dir_cls_preds: the [B, H, W, C] prediction maps
    of its forward (device tensors, f32 or bf16, any strides -- the channel blocks of the fused tensor are fine;
    dir_cls_preds None without a direction classifier); post_process_cfg: the detector's POST_PROCESSING block.  Returns
    {'boxes' [B, M, 7], 'scores' [B, M], 'labels' [B, M], 'count' [B]} with M = NMS_POST_MAXSIZE (module docstring)."""
    from .hotpath.anchor_head import _strides3
    s = anchor_static_settings(post_process_cfg)
    maps = [cls_preds, box_preds, dir_cls_preds]
    if any(m is not None and not (torch.is_tensor(m) and m.is_cuda) for m in maps) or cls_preds is None or box_preds is None:
        raise L.PcdError("static anchor post-processing needs HIP device tensors (there is no CPU fallback)")
    if cls_preds.dtype not in (torch.float32, torch.bfloat16):
        raise L.PcdError(f"static anchor post-processing: prediction maps of dtype {cls_preds.dtype} (f32 / bf16)")
    if any(m is not None and (m.dtype != cls_preds.dtype or m.dim() != 4 or m.shape[:3] != cls_preds.shape[:3]) for m in maps):
        raise L.PcdError("static anchor post-processing: the three prediction maps must share dtype and [B, H, W]")
    tab = head.tables(cls_preds.device)
    if (cls_preds.shape[1], cls_preds.shape[2]) != (tab.H, tab.W) or cls_preds.shape[3] != tab.A * tab.num_class \
            or box_preds.shape[3] != tab.A * 7 or (dir_cls_preds is not None and dir_cls_preds.shape[3] != tab.A * tab.num_dir_bins):
        raise L.PcdError(f"static anchor post-processing: prediction maps {tuple(cls_preds.shape)} / {tuple(box_preds.shape)} "
                         f"do not match the {tab.H} x {tab.W} x {tab.A} anchors")
    B = int(cls_preds.shape[0])
    cfg = anchor_postproc_config(s, tab, B)
    lib = L.lib()
    cp = ctypes.cast(ctypes.pointer(cfg), ctypes.c_void_p)
    nbytes = int(lib.pcd_anchor_postproc_workspace_bytes(cp))
    if nbytes == 0:
        raise L.PcdError("static anchor post-processing: configuration refused by pcd_anchor_postproc (include/pcd_ops.h)")
    dev, M = cls_preds.device, s["nms_post"]
    out = {"boxes": torch.empty((B, M, 7), dtype=torch.float32, device=dev),
           "scores": torch.empty((B, M), dtype=torch.float32, device=dev),
           "labels": torch.empty((B, M), dtype=torch.int64, device=dev),
           "count": torch.empty((B,), dtype=torch.int32, device=dev)}
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    L.check(lib.pcd_anchor_postproc(L.ptr(cls_preds), L.ptr(box_preds), L.ptr(dir_cls_preds), L.dtype_code(cls_preds),
                                    _strides3(maps), L.ptr(tab.kinds), L.ptr(tab.shifts), cp, L.ptr(out["boxes"]),
                                    L.ptr(out["scores"]), L.ptr(out["labels"]), L.ptr(out["count"]), L.ptr(ws), nbytes,
                                    L.stream_ptr()), "pcd_anchor_postproc")
    return out


class PcdAnchorMultiPostprocConfig(ctypes.Structure):
    """include/pcd_ops.h: struct PcdAnchorMultiPostprocConfig (POST_PROCESSING of a multi-head anchor detector + the head's
    shapes and its per-class label table); the mirror lives beside its one user."""
    _fields_ = [("batch", ctypes.c_int), ("height", ctypes.c_int), ("width", ctypes.c_int), ("n_kinds", ctypes.c_int),
                ("n_classes", ctypes.c_int), ("num_class", ctypes.c_int), ("code", ctypes.c_int), ("sincos", ctypes.c_int),
                ("num_dir_bins", ctypes.c_int), ("nms_pre", ctypes.c_int), ("nms_post", ctypes.c_int),
                ("nms_normal", ctypes.c_int), ("use_score_thresh", ctypes.c_int), ("score_thresh", ctypes.c_float),
                ("nms_thresh", ctypes.c_float), ("dir_offset", ctypes.c_float), ("dir_limit_offset", ctypes.c_float),
                ("label", ctypes.c_int * L.PCD_ANCHOR_MAX_CLASSES)]


def anchor_multi_static_settings(post_process_cfg):
    """The POST_PROCESSING block of a multi-head anchor detector as pcd_anchor_multi_postproc takes it (the keys of
    anchor_static_settings); PcdError naming the key for what the static path refuses: MULTI_CLASSES_NMS = False (per-head
    class scores have no class-agnostic maximum; the eager post_processing refuses it too), OUTPUT_RAW_SCORE, other NMS
    types, NMS_PRE_MAXSIZE above the LDS cap, sizes below 1."""
    return _anchor_settings(post_process_cfg, "static multi-head anchor post-processing", multi=True)


def anchor_multi_postproc_config(s, tab, batch, labels):
    """PcdAnchorMultiPostprocConfig of settings `s` (anchor_multi_static_settings) for the tables `tab` (MultiTables) of a
    head; labels: the output label of every global class (multihead_label_mapping, heads concatenated)."""
    num_class = sum(nc for _, _, _, nc in tab.heads)
    if len(labels) != num_class or num_class > L.PCD_ANCHOR_MAX_CLASSES:
        raise L.PcdError(f"static multi-head anchor post-processing: {len(labels)} labels for {num_class} classes (at most "
                         f"{L.PCD_ANCHOR_MAX_CLASSES})")
    cfg = PcdAnchorMultiPostprocConfig()
    cfg.batch, cfg.height, cfg.width, cfg.n_kinds, cfg.n_classes, cfg.num_class = int(batch), tab.H, tab.W, tab.G, tab.C, num_class
    cfg.code, cfg.sincos, cfg.num_dir_bins = tab.code, tab.sincos, tab.num_dir_bins
    cfg.nms_pre, cfg.nms_post, cfg.nms_normal = s["nms_pre"], s["nms_post"], s["nms_normal"]
    cfg.use_score_thresh = int(s["score_thresh"] is not None)
    cfg.score_thresh = float(s["score_thresh"]) if s["score_thresh"] is not None else 0.0
    cfg.nms_thresh = s["nms_thresh"]
    cfg.dir_offset, cfg.dir_limit_offset = tab.dir_offset, tab.dir_limit_offset
    for c, v in enumerate(labels):
        cfg.label[c] = int(v)
    return cfg


def anchor_multi_predictions_static(head, cls_maps, box_maps, dir_maps, post_process_cfg):
    """head: an AnchorHeadMulti (its anchor tables and `head_labels`); cls_maps / box_maps / dir_maps: the per-head
    [B, A_h * items, H, W] prediction maps of its forward (lists of device tensors, f32 or bf16, any strides; dir_maps None
    without a direction classifier); post_process_cfg: the detector's POST_PROCESSING block.  Returns {'boxes' [B, M, D],
    'scores' [B, M], 'labels' [B, M], 'count' [B]} with M = num_class x NMS_POST_MAXSIZE and D = 7 | 9: per frame the
    classes' kept boxes in global class order (head order, then class order inside the head), each class's in score order.
    Per (frame, class): score = fp32 sigmoid of the class logit; passes iff score >= SCORE_THRESH (inclusive; a NaN never);
    the first min(NMS_PRE_MAXSIZE, passing) local anchors by score descending, then local anchor index ascending; only
    those are decoded (the arithmetic of pcd_anchor_multi_decode); NMS on columns 0:7; the first NMS_POST_MAXSIZE."""
    from .hotpath.anchor_head_multi import _head_structs
    s = anchor_multi_static_settings(post_process_cfg)
    tensors = list(cls_maps) + list(box_maps) + list(dir_maps or [])
    if not tensors or any(not (torch.is_tensor(t) and t.is_cuda) for t in tensors):
        raise L.PcdError("static multi-head anchor post-processing needs HIP device tensors (there is no CPU fallback)")
    if cls_maps[0].dtype not in (torch.float32, torch.bfloat16):
        raise L.PcdError(f"static multi-head anchor post-processing: prediction maps of dtype {cls_maps[0].dtype} (f32 / bf16)")
    dev = cls_maps[0].device
    tab = head.tables(dev)
    heads, dtype, B = _head_structs(tab, list(cls_maps), list(box_maps), list(dir_maps) if dir_maps is not None else None)
    cfg = anchor_multi_postproc_config(s, tab, B, head.head_labels)
    lib = L.lib()
    cp = ctypes.cast(ctypes.pointer(cfg), ctypes.c_void_p)
    n = len(tab.heads)
    nbytes = int(lib.pcd_anchor_multi_postproc_workspace_bytes(heads, n, cp))
    if nbytes == 0:
        raise L.PcdError("static multi-head anchor post-processing: configuration refused by pcd_anchor_multi_postproc "
                         "(include/pcd_ops.h)")
    M, D = cfg.num_class * s["nms_post"], tab.code_gt
    out = {"boxes": torch.empty((B, M, D), dtype=torch.float32, device=dev),
           "scores": torch.empty((B, M), dtype=torch.float32, device=dev),
           "labels": torch.empty((B, M), dtype=torch.int64, device=dev),
           "count": torch.empty((B,), dtype=torch.int32, device=dev)}
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    L.check(lib.pcd_anchor_multi_postproc(heads, n, dtype, L.ptr(tab.kinds), L.ptr(tab.shifts), cp, L.ptr(out["boxes"]),
                                          L.ptr(out["scores"]), L.ptr(out["labels"]), L.ptr(out["count"]), L.ptr(ws), nbytes,
                                          L.stream_ptr()), "pcd_anchor_multi_postproc")
    return out


class PcdAnchorProposalsConfig(ctypes.Structure):
    """include/pcd_ops.h: struct PcdAnchorProposalsConfig (NMS_CONFIG.TEST of a RoI head + the anchor head's shapes); the
    mirror lives beside its one user."""
    _fields_ = [("batch", ctypes.c_int), ("height", ctypes.c_int), ("width", ctypes.c_int), ("n_kinds", ctypes.c_int),
                ("n_classes", ctypes.c_int), ("num_class", ctypes.c_int), ("num_dir_bins", ctypes.c_int),
                ("nms_pre", ctypes.c_int), ("nms_post", ctypes.c_int), ("nms_normal", ctypes.c_int),
                ("nms_thresh", ctypes.c_float), ("dir_offset", ctypes.c_float), ("dir_limit_offset", ctypes.c_float)]


def _nms_keys(nms, what):
    """the four NMS keys of an NMS_CONFIG block and the refusals every static path shares; PcdError naming the key"""
    if nms is None:
        raise L.PcdError(f"{what}: no NMS_CONFIG block")
    if _get(nms, 'MULTI_CLASSES_NMS', False):
        raise L.PcdError(f"{what}: NMS_CONFIG.MULTI_CLASSES_NMS = True is not supported (class-agnostic NMS only)")
    kind = _get(nms, 'NMS_TYPE', None)
    if kind not in NMS_TYPES:
        raise L.PcdError(f"{what}: NMS_TYPE {kind!r} (supported: {sorted(NMS_TYPES)})")
    s = dict(nms_pre=int(_get(nms, 'NMS_PRE_MAXSIZE')), nms_post=int(_get(nms, 'NMS_POST_MAXSIZE')),
             nms_thresh=float(_get(nms, 'NMS_THRESH')), nms_normal=NMS_TYPES[kind])
    if s["nms_pre"] > L.POSTPROC_MAX_K:
        raise L.PcdError(f"{what}: NMS_PRE_MAXSIZE = {s['nms_pre']} above the cap {L.POSTPROC_MAX_K} (the per-frame sort runs in "
                         "LDS)")
    for key, v in (("NMS_PRE_MAXSIZE", s["nms_pre"]), ("NMS_POST_MAXSIZE", s["nms_post"])):
        if v < 1:
            raise L.PcdError(f"{what}: {key} = {v}")
    return s


def roi_proposal_settings(nms_config):
    """One block of a RoI head's NMS_CONFIG (TEST) as pcd_anchor_proposals takes it; PcdError naming the key for what the
    static proposal layer refuses: MULTI_CLASSES_NMS, other NMS types, NMS_PRE_MAXSIZE above the LDS cap (the 9000 of the
    TRAIN blocks: the training forward keeps the eager proposal_layer), sizes below 1."""
    return _nms_keys(nms_config, "static proposal layer")


def anchor_proposals_static(head, cls_preds, box_preds, dir_cls_preds, nms_config):
    """RoIHeadTemplate.proposal_layer (roi_head_template.py:45-102) straight from the prediction maps of an
    AnchorHeadSingle (`head`: its anchor tables; the maps as anchor_predictions_static takes them), one call into
    pcd_anchor_proposals: no [B, N, 7] and no [B, N, num_class] tensor.  Per frame: an anchor's score is the maximum of its
    num_class LOGITS (no sigmoid; bf16 widened first), its label the lowest class index at the maximum, + 1; every anchor
    takes part but one whose maximum is NaN; the first min(NMS_PRE_MAXSIZE, N) by score descending, then anchor index
    n = (y * W + x) * A + kind ascending, are decoded (the arithmetic of pcd_anchor_decode) and go through NMS on columns 0:7;
    the first NMS_POST_MAXSIZE survivors are kept.  Returns {'rois' f32 [B, POST, 7], 'roi_scores' f32 [B, POST],
    'roi_labels' int64 [B, POST], 'count' int32 [B]}; rows behind count are what the reference leaves there: boxes 0,
    scores 0, labels 1."""
    from .hotpath.anchor_head import _strides3
    what = "static proposal layer"
    s = roi_proposal_settings(nms_config)
    maps = [cls_preds, box_preds, dir_cls_preds]
    if any(m is not None and not (torch.is_tensor(m) and m.is_cuda) for m in maps) or cls_preds is None or box_preds is None:
        raise L.PcdError(f"{what} needs HIP device tensors (there is no CPU fallback)")
    if cls_preds.dtype not in (torch.float32, torch.bfloat16):
        raise L.PcdError(f"{what}: prediction maps of dtype {cls_preds.dtype} (f32 / bf16)")
    if any(m is not None and (m.dtype != cls_preds.dtype or m.dim() != 4 or m.shape[:3] != cls_preds.shape[:3]) for m in maps):
        raise L.PcdError(f"{what}: the three prediction maps must share dtype and [B, H, W]")
    tab = head.tables(cls_preds.device)
    if (cls_preds.shape[1], cls_preds.shape[2]) != (tab.H, tab.W) or cls_preds.shape[3] != tab.A * tab.num_class \
            or box_preds.shape[3] != tab.A * 7 or (dir_cls_preds is not None and dir_cls_preds.shape[3] != tab.A * tab.num_dir_bins):
        raise L.PcdError(f"{what}: prediction maps {tuple(cls_preds.shape)} / {tuple(box_preds.shape)} do not match the "
                         f"{tab.H} x {tab.W} x {tab.A} anchors")
    B = int(cls_preds.shape[0])
    cfg = PcdAnchorProposalsConfig()
    cfg.batch, cfg.height, cfg.width, cfg.n_kinds, cfg.n_classes = B, tab.H, tab.W, tab.A, tab.C
    cfg.num_class, cfg.num_dir_bins = tab.num_class, tab.num_dir_bins
    cfg.nms_pre, cfg.nms_post, cfg.nms_normal, cfg.nms_thresh = s["nms_pre"], s["nms_post"], s["nms_normal"], s["nms_thresh"]
    cfg.dir_offset, cfg.dir_limit_offset = tab.dir_offset, tab.dir_limit_offset
    lib = L.lib()
    cp = ctypes.cast(ctypes.pointer(cfg), ctypes.c_void_p)
    nbytes = int(lib.pcd_anchor_proposals_workspace_bytes(cp))
    if nbytes == 0:
        raise L.PcdError(f"{what}: configuration refused by pcd_anchor_proposals (include/pcd_ops.h)")
    dev, M = cls_preds.device, s["nms_post"]
    out = {"rois": torch.empty((B, M, 7), dtype=torch.float32, device=dev),
           "roi_scores": torch.empty((B, M), dtype=torch.float32, device=dev),
           "roi_labels": torch.empty((B, M), dtype=torch.int64, device=dev),
           "count": torch.empty((B,), dtype=torch.int32, device=dev)}
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    L.check(lib.pcd_anchor_proposals(L.ptr(cls_preds), L.ptr(box_preds), L.ptr(dir_cls_preds), L.dtype_code(cls_preds),
                                     _strides3(maps), L.ptr(tab.kinds), L.ptr(tab.shifts), cp, L.ptr(out["rois"]),
                                     L.ptr(out["roi_scores"]), L.ptr(out["roi_labels"]), L.ptr(out["count"]), L.ptr(ws), nbytes,
                                     L.stream_ptr()), "pcd_anchor_proposals")
    return out


class PcdRoiPostprocConfig(ctypes.Structure):
    """include/pcd_ops.h: struct PcdRoiPostprocConfig (POST_PROCESSING of a two-stage detector + the RoI head's shapes); the
    mirror lives beside its one user."""
    _fields_ = [("batch", ctypes.c_int), ("rois", ctypes.c_int), ("score_type", ctypes.c_int), ("normalized", ctypes.c_int),
                ("has_class_labels", ctypes.c_int), ("num_class", ctypes.c_int),
                ("by_class_iou", ctypes.c_int * L.PCD_POSTPROC_MAX_CLASSES), ("nms_pre", ctypes.c_int),
                ("nms_post", ctypes.c_int), ("nms_normal", ctypes.c_int), ("use_score_thresh", ctypes.c_int),
                ("score_thresh", ctypes.c_float), ("nms_thresh", ctypes.c_float), ("weight_iou", ctypes.c_float),
                ("weight_cls", ctypes.c_float), ("pts_cls_thresh", ctypes.c_float), ("pts_iou_thresh", ctypes.c_float),
                ("pts_span", ctypes.c_float)]


ROI_SCORE_TYPES = {"rcnn": L.PCD_ROIPP_SCORE_RCNN, "iou": L.PCD_ROIPP_SCORE_IOU, "cls": L.PCD_ROIPP_SCORE_CLS,
                   "weighted_iou_cls": L.PCD_ROIPP_SCORE_WEIGHTED, "score_by_class": L.PCD_ROIPP_SCORE_BY_CLASS,
                   "num_pts_iou_cls": L.PCD_ROIPP_SCORE_NUM_PTS}


def roi_static_settings(post_process_cfg, second_iou):
    """The POST_PROCESSING block of a two-stage detector as pcd_roi_postproc takes it.  second_iou False: the class-agnostic
    branch of Detector3DTemplate.post_processing (score type 'rcnn': the sigmoid of the RoI head's one logit); True:
    SECONDNetIoU.post_processing with NMS_CONFIG.SCORE_TYPE ('iou' when the key is absent) and the keys that type reads
    (SCORE_WEIGHTS.iou / .cls, SCORE_BY_CLASS per class name -- checked against `class_names` at the call --,
    NMS_CONFIG.SCORE_THRESH.cls / .iou).  PcdError naming the key for what the static path refuses: MULTI_CLASSES_NMS,
    OUTPUT_RAW_SCORE, an unknown NMS_TYPE / SCORE_TYPE, SCORE_BY_CLASS missing, NMS_PRE_MAXSIZE above the LDS cap, sizes
    below 1."""
    what = "static RoI post-processing"
    if post_process_cfg is None:
        raise L.PcdError(f"{what}: no POST_PROCESSING block")
    nms = _get(post_process_cfg, 'NMS_CONFIG', None)
    s = _nms_keys(nms, what)
    if _get(post_process_cfg, 'OUTPUT_RAW_SCORE', False):
        raise L.PcdError(f"{what}: OUTPUT_RAW_SCORE = True is not supported")
    s["score_thresh"] = _get(post_process_cfg, 'SCORE_THRESH', None)
    s["score_type"] = "rcnn"
    s["weights"], s["by_class"], s["pts"] = (0.0, 0.0), None, (0.0, 0.0)
    if second_iou:
        kind = _get(nms, 'SCORE_TYPE', None)
        kind = 'iou' if kind is None else kind
        if kind not in ROI_SCORE_TYPES or kind == "rcnn":
            raise L.PcdError(f"{what}: NMS_CONFIG.SCORE_TYPE = {kind!r} is not supported (supported: "
                             f"{[k for k in ROI_SCORE_TYPES if k != 'rcnn']})")
        s["score_type"] = kind
        if kind == 'weighted_iou_cls':
            w = _get(nms, 'SCORE_WEIGHTS', None)
            if w is None or _get(w, 'iou', None) is None or _get(w, 'cls', None) is None:
                raise L.PcdError(f"{what}: NMS_CONFIG.SCORE_WEIGHTS (.iou, .cls) missing beside SCORE_TYPE = 'weighted_iou_cls'")
            s["weights"] = (float(_get(w, 'iou')), float(_get(w, 'cls')))
        elif kind == 'score_by_class':
            by = _get(nms, 'SCORE_BY_CLASS', None)
            if not by:
                raise L.PcdError(f"{what}: NMS_CONFIG.SCORE_BY_CLASS missing beside SCORE_TYPE = 'score_by_class'")
            for name in by:
                if _get(by, name) not in ('iou', 'cls'):
                    raise L.PcdError(f"{what}: NMS_CONFIG.SCORE_BY_CLASS.{name} = {_get(by, name)!r} is not supported "
                                     "(supported: 'iou', 'cls')")
            s["by_class"] = {name: _get(by, name) for name in by}
        elif kind == 'num_pts_iou_cls':
            t = _get(nms, 'SCORE_THRESH', None)
            if t is None or _get(t, 'cls', None) is None or _get(t, 'iou', None) is None:
                raise L.PcdError(f"{what}: NMS_CONFIG.SCORE_THRESH (.cls, .iou) missing beside SCORE_TYPE = 'num_pts_iou_cls'")
            s["pts"] = (_get(t, 'cls'), _get(t, 'iou'))
            if not s["pts"][1] >= s["pts"][0]:
                raise L.PcdError(f"{what}: NMS_CONFIG.SCORE_THRESH.iou = {s['pts'][1]} below .cls = {s['pts'][0]} (the "
                                 "reference asserts)")
    return s


def roi_predictions_static(batch_dict, post_process_cfg, class_names=None, second_iou=False):
    """The final post-processing of a two-stage detector from the RoI head's eval outputs in `batch_dict`
    (batch_box_preds [B, R, 7], batch_cls_preds [B, R, 1], cls_preds_normalized, roi_labels + has_class_labels; with
    second_iou also roi_scores and, for SCORE_TYPE 'num_pts_iou_cls', `points` or ready `roi_point_counts` int32 [B, R]), one
    call into pcd_roi_postproc.  All R rows take part, the zero rows behind the proposal count included.  Returns {'boxes'
    [B, M, 7], 'scores' [B, M] (the NMS score), 'labels' [B, M], 'count' [B]} and with second_iou 'cls_scores' / 'iou_scores'
    [B, M]; M = NMS_POST_MAXSIZE, rows behind count are zero.  Order: score descending, then RoI row ascending; a row passes
    iff score >= SCORE_THRESH (inclusive; every row without one; a NaN never)."""
    what = "static RoI post-processing"
    s = roi_static_settings(post_process_cfg, second_iou)
    if batch_dict.get('batch_index', None) is not None:
        raise L.PcdError(f"{what}: batch_index (stacked predictions) is not supported; the RoI heads write [B, R, .] predictions")
    boxes, iou = batch_dict['batch_box_preds'], batch_dict['batch_cls_preds']
    has_labels = bool(batch_dict.get('has_class_labels', False))
    tensors = [boxes, iou] + ([batch_dict['roi_scores']] if second_iou else []) + ([batch_dict['roi_labels']] if has_labels else [])
    if any(not (torch.is_tensor(t) and t.is_cuda) for t in tensors):
        raise L.PcdError(f"{what} needs HIP device tensors (there is no CPU fallback)")
    if boxes.dim() != 3 or boxes.shape[2] != 7 or iou.dim() != 3 or iou.shape[2] != 1 or iou.shape[:2] != boxes.shape[:2]:
        raise L.PcdError(f"{what}: batch_box_preds {tuple(boxes.shape)}, batch_cls_preds {tuple(iou.shape)}; want [B, R, 7] and "
                         "[B, R, 1]")
    B, R = int(boxes.shape[0]), int(boxes.shape[1])
    if R > L.POSTPROC_MAX_K or R < 1 or B < 1:
        raise L.PcdError(f"{what}: {R} RoIs per frame (1 .. {L.POSTPROC_MAX_K}: the per-frame sort runs in LDS), batch {B}")
    cfg = PcdRoiPostprocConfig()
    cfg.batch, cfg.rois, cfg.score_type = B, R, ROI_SCORE_TYPES[s["score_type"]]
    cfg.normalized, cfg.has_class_labels = int(bool(batch_dict.get('cls_preds_normalized', False))), int(has_labels)
    counts = None
    if s["score_type"] == 'score_by_class':
        names = list(class_names or [])
        if not 1 <= len(names) <= L.PCD_POSTPROC_MAX_CLASSES:
            raise L.PcdError(f"{what}: SCORE_TYPE 'score_by_class' needs class_names (1 .. {L.PCD_POSTPROC_MAX_CLASSES})")
        for c, name in enumerate(names):
            if name not in s["by_class"]:
                raise L.PcdError(f"{what}: NMS_CONFIG.SCORE_BY_CLASS.{name} missing")
            cfg.by_class_iou[c] = int(s["by_class"][name] == 'iou')
        cfg.num_class = len(names)
    elif s["score_type"] == 'num_pts_iou_cls':
        counts = batch_dict.get('roi_point_counts', None)
        if counts is None:
            from .hotpath.second_head import points_in_boxes_count
            counts = points_in_boxes_count(batch_dict['points'], boxes)
        if not counts.is_cuda or counts.dtype != torch.int32 or tuple(counts.shape) != (B, R):
            raise L.PcdError(f"{what}: roi_point_counts {tuple(counts.shape)} {counts.dtype}, want int32 [{B}, {R}] on the device")
        counts = counts.contiguous()
        cfg.pts_cls_thresh, cfg.pts_iou_thresh = float(s["pts"][0]), float(s["pts"][1])
        cfg.pts_span = float(s["pts"][1] - s["pts"][0])
    cfg.nms_pre, cfg.nms_post, cfg.nms_normal, cfg.nms_thresh = s["nms_pre"], s["nms_post"], s["nms_normal"], s["nms_thresh"]
    cfg.use_score_thresh = int(s["score_thresh"] is not None)
    cfg.score_thresh = float(s["score_thresh"]) if s["score_thresh"] is not None else 0.0
    cfg.weight_iou, cfg.weight_cls = s["weights"]
    boxes = boxes.detach().float().contiguous()
    iou = iou.detach().float().contiguous()
    cls = batch_dict['roi_scores'].detach().float().contiguous() if second_iou else None
    labels = batch_dict['roi_labels'].detach().long().contiguous() if has_labels else None
    if (cls is not None and tuple(cls.shape) != (B, R)) or (labels is not None and tuple(labels.shape) != (B, R)):
        raise L.PcdError(f"{what}: roi_scores / roi_labels are not [{B}, {R}]")
    lib = L.lib()
    cp = ctypes.cast(ctypes.pointer(cfg), ctypes.c_void_p)
    nbytes = int(lib.pcd_roi_postproc_workspace_bytes(cp))
    if nbytes == 0:
        raise L.PcdError(f"{what}: configuration refused by pcd_roi_postproc (include/pcd_ops.h)")
    dev, M = boxes.device, s["nms_post"]
    out = {"boxes": torch.empty((B, M, 7), dtype=torch.float32, device=dev),
           "scores": torch.empty((B, M), dtype=torch.float32, device=dev),
           "labels": torch.empty((B, M), dtype=torch.int64, device=dev),
           "count": torch.empty((B,), dtype=torch.int32, device=dev)}
    if second_iou:
        out["cls_scores"] = torch.empty((B, M), dtype=torch.float32, device=dev)
        out["iou_scores"] = torch.empty((B, M), dtype=torch.float32, device=dev)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    L.check(lib.pcd_roi_postproc(L.ptr(boxes), L.ptr(iou), L.ptr(cls), L.ptr(labels), L.ptr(counts), cp, L.ptr(out["boxes"]),
                                 L.ptr(out["scores"]), L.ptr(out["labels"]), L.ptr(out["count"]), L.ptr(out.get("cls_scores")),
                                 L.ptr(out.get("iou_scores")), L.ptr(ws), nbytes, L.stream_ptr()), "pcd_roi_postproc")
    return out


def to_pred_dicts(static):
    """The reference's final_box_dicts (pred_boxes, pred_scores, pred_labels per frame; pred_cls_scores / pred_iou_scores too
    when the static dict has them: the record of SECONDNetIoU.post_processing) from the padded tensors: one device -> host
    copy of `count`, then views of each frame's first count rows."""
    count = static["count"].cpu().tolist()
    keys = [("pred_boxes", "boxes"), ("pred_scores", "scores"), ("pred_labels", "labels")]
    keys += [(k, v) for k, v in (("pred_cls_scores", "cls_scores"), ("pred_iou_scores", "iou_scores")) if v in static]
    return [{k: static[v][b, :n] for k, v in keys} for b, n in enumerate(count)]
