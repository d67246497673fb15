"""`CurriculumCenterHead` / `CurriculumCenterHead_x5` -- the COM dense head as a registry drop-in
(pcdet/models/dense_heads/__init__.py:15-32; reference classes: curriculum_center_head.py:48-511, head_zoo.py:145-149).

Same constructor arguments, `forward(data_dict)` contract (`spatial_features_2d`, `gt_boxes`, `num_points_in_gt`,
`true_object`, `occupancy_ratio`, `facade_type` in; `rois` / `roi_scores` / `roi_labels` or `final_box_dicts` out),
`get_loss()`, `generate_predicted_boxes()` and module names (`shared_conv`, `heads_list`: state-dict compatible) -- with
the towers on the hand-written 3x3 conv kernels (bf16 channels-last), `cluster` / `assign_targets` / the curriculum
loss on the device (com_head.py) and NMS through com_amd.iou3d_nms.  `self.epoch` is set by the training loop as in the
reference (train_utils.py pushes it every epoch)."""
import torch.nn as nn

from . import com_head
from .center_head import BoxDecodeMixin, class_agnostic_nms, decode_bbox_from_heatmap  # noqa: F401
from .dense2d import CenterHeadTowers, _get


class CurriculumCenterHead(BoxDecodeMixin, nn.Module):
    conf_shape = None            # base class: FocalLossCenterCurriculum(conf_shape=None), curriculum_center_head.py:103-105

    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size,
                 predict_boxes_when_training=True):
        super().__init__()
        self.model_cfg, self.num_class, self.class_names = model_cfg, num_class, list(class_names)
        self.grid_size, self.point_cloud_range, self.voxel_size = grid_size, list(point_cloud_range), list(voxel_size)
        ta = _get(model_cfg, 'TARGET_ASSIGNER_CONFIG')
        self.feature_map_stride = _get(ta, 'FEATURE_MAP_STRIDE', None)
        self.epoch, self.cur_iter = 0, 0
        self.epoch_thredhold = _get(ta, 'EPOCH_THRED', 100)
        self.min_points = _get(ta, 'MIN_POINTS', 1)
        self.class_names_each_head = [[x for x in names if x in self.class_names]
                                      for names in _get(model_cfg, 'CLASS_NAMES_EACH_HEAD')]
        assert sum(len(x) for x in self.class_names_each_head) == len(self.class_names)
        self.class_id_mapping_each_head = [[self.class_names.index(x) for x in names] for names in self.class_names_each_head]
        towers = CenterHeadTowers(model_cfg, input_channels, self.class_names_each_head)
        self.shared_conv, self.heads_list = towers.shared_conv, towers.heads_list      # (reference module names)
        self._towers = [towers]                                                        # not a submodule: no duplicate keys
        self.separate_head_cfg = _get(model_cfg, 'SEPARATE_HEAD_CFG')
        self.predict_boxes_when_training = predict_boxes_when_training
        self.forward_ret_dict = {}
        lw = _get(_get(model_cfg, 'LOSS_CONFIG'), 'LOSS_WEIGHTS')
        self.loss = com_head.CurriculumCenterHeadLoss(
            _get(self.separate_head_cfg, 'HEAD_ORDER'), _get(model_cfg, 'LOSS_CURRICULUM', None), conf_shape=self.conf_shape,
            cls_weight=lw['cls_weight'], loc_weight=lw['loc_weight'], code_weights=lw['code_weights'])

    @property
    def hm_loss_func(self):
        """What train_utils.py:111-112 reads (`hm_loss_func.confidence_all`) -- the device-side state."""
        return self.loss.hm_loss_func

    def assign_targets(self, gt_boxes, feature_map_size=None, npgt=None, true_object=None, **kwargs):
        ta = _get(self.model_cfg, 'TARGET_ASSIGNER_CONFIG')
        return com_head.assign_targets(
            gt_boxes, feature_map_size, self.class_names, self.class_names_each_head, self.point_cloud_range,
            self.voxel_size, _get(ta, 'FEATURE_MAP_STRIDE'), npgt, true_object=true_object,
            num_max_objs=_get(ta, 'NUM_MAX_OBJS'), gaussian_overlap=_get(ta, 'GAUSSIAN_OVERLAP'),
            min_radius=_get(ta, 'MIN_RADIUS'), epoch=self.epoch, epoch_threshold=self.epoch_thredhold,
            min_points=self.min_points)

    def cluster(self, gt_boxes, true_object, occupancy_ratio, facade_type):
        return com_head.cluster(gt_boxes, true_object, occupancy_ratio, facade_type)

    def get_loss(self):
        return self.loss(self.forward_ret_dict['pred_dicts'], self.forward_ret_dict['target_dicts'], epoch=self.epoch)

    def forward(self, data_dict):
        """curriculum_center_head.py:461-487.  `static_predictions` (popped): in eval mode, store the padded static
        post-processing as data_dict['final_box_tensors'] instead of running generate_predicted_boxes."""
        static = data_dict.pop('static_predictions', False)
        sf = data_dict['spatial_features_2d']
        pred_dicts = self._towers[0]({'spatial_features_2d': sf})['pred_dicts']
        if self.training:
            group = self.cluster(data_dict['gt_boxes'], data_dict.get('true_object', None), data_dict['occupancy_ratio'],
                                 data_dict['facade_type'])
            self.forward_ret_dict['target_dicts'] = self.assign_targets(
                data_dict['gt_boxes'], feature_map_size=sf.size()[2:], npgt=data_dict['num_points_in_gt'], true_object=group)
        self.forward_ret_dict['pred_dicts'] = pred_dicts
        if static and not self.training:
            # per-call opt-in (com_amd.infer.CapturedInference): padded device tensors instead of the eager decode
            data_dict['final_box_tensors'] = self.generate_predicted_boxes_static(data_dict['batch_size'], pred_dicts)
        elif not self.training or self.predict_boxes_when_training:
            boxes = self.generate_predicted_boxes(data_dict['batch_size'], pred_dicts)
            if self.predict_boxes_when_training:
                rois, roi_scores, roi_labels = self.reorder_rois_for_refining(data_dict['batch_size'], boxes)
                data_dict.update(rois=rois, roi_scores=roi_scores, roi_labels=roi_labels, has_class_labels=True)
            else:
                data_dict['final_box_dicts'] = boxes
        return data_dict


class CurriculumCenterHead_x5(CurriculumCenterHead):
    """head_zoo.py:145-149: the (3, 96) group-confidence pass that feeds COMAug."""
    conf_shape = (3, 96)
