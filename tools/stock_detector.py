"""A detector object shaped the way the reference's `Detector3DTemplate.build_networks` builds one (test infrastructure,
like tools/seam1_model.py): the modules of `module_topology` registered as attributes (`vfe`, `backbone_3d`,
`map_to_bev_module`, `backbone_2d`, `dense_head`; None where the config has none), `module_list` a plain list of them,
a `global_step` buffer, `forward` iterating `module_list` and then `get_training_loss()` reading `self.dense_head`.

Every module is written the way a stock model file is written -- plain torch (`nn.Conv2d`, `nn.BatchNorm2d`, `nn.ReLU`,
`nn.ZeroPad2d`, `nn.ConvTranspose2d`) over the import seams (`spconv.*` names for the sparse backbone, the target
assignment and losses of com_amd.hotpath for the heads) -- with the reference's constructor arguments, module names and
state-dict keys.  `com_amd.adopt.adopt_model` turns such an object into the fused one in place.

    build_detector("3d")           MeanVFE -> VoxelResBackBone8x -> HeightCompression (bench.py's hot path)
    build_detector("centerpoint")  + BaseBEVBackbone + CenterHead                     (waymo_models/centerpoint.yaml)
    build_detector("com")          + BaseBEVBackbone + CurriculumCenterHead_x5         (the COM head, bench.py --com)
"""
import copy

import numpy as np
import torch
from torch import nn

import seam1_model
from com_amd import ops
from com_amd.utils import synth

CLASS_NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']


class Cfg(dict):
    """EasyDict-like config node: attribute and item access."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as exc:
            raise AttributeError(k) from exc


def _cfg(d):
    if isinstance(d, dict):
        return Cfg({k: _cfg(v) for k, v in d.items()})
    if isinstance(d, list):
        return [_cfg(v) for v in d]
    return d


# ---------------------------------------------------------------------------------------------------------- 3-D part
class MeanVFE(nn.Module):
    def __init__(self, model_cfg, num_point_features, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_point_features = num_point_features

    def get_output_feature_dim(self):
        return self.num_point_features

    def forward(self, batch_dict, **kwargs):
        if batch_dict.get('voxels', None) is None:
            return batch_dict                    # the voxeliser already emitted the per-voxel mean
        voxels, num = batch_dict['voxels'], batch_dict['voxel_num_points']
        mean = voxels.sum(dim=1) / torch.clamp_min(num.view(-1, 1), 1.0).type_as(voxels)
        batch_dict['voxel_features'] = mean.contiguous()
        return batch_dict


class VoxelResBackBone8x(seam1_model.StockVoxelResBackBone8x):
    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__(input_channels, grid_size)
        self.model_cfg = model_cfg
        self.num_point_features = 128
        self.backbone_channels = {'x_conv1': 16, 'x_conv2': 32, 'x_conv3': 64, 'x_conv4': 128}


class HeightCompression(nn.Module):
    def __init__(self, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = model_cfg['NUM_BEV_FEATURES']

    def forward(self, batch_dict):
        sp = batch_dict['encoded_spconv_tensor']
        spatial_features = sp.dense()
        N, C, D, H, W = spatial_features.shape
        batch_dict['spatial_features'] = spatial_features.view(N, C * D, H, W)
        batch_dict['spatial_features_stride'] = batch_dict['encoded_spconv_tensor_stride']
        return batch_dict


# ---------------------------------------------------------------------------------------------------------- dense part
class BaseBEVBackbone(nn.Module):
    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        layer_nums, layer_strides, num_filters = model_cfg['LAYER_NUMS'], model_cfg['LAYER_STRIDES'], model_cfg['NUM_FILTERS']
        upsample_strides, num_upsample_filters = model_cfg['UPSAMPLE_STRIDES'], model_cfg['NUM_UPSAMPLE_FILTERS']
        c_in_list = [input_channels, *num_filters[:-1]]
        self.blocks, self.deblocks = nn.ModuleList(), nn.ModuleList()
        for idx in range(len(layer_nums)):
            layers = [nn.ZeroPad2d(1),
                      nn.Conv2d(c_in_list[idx], num_filters[idx], kernel_size=3, stride=layer_strides[idx], padding=0,
                                bias=False),
                      nn.BatchNorm2d(num_filters[idx], eps=1e-3, momentum=0.01), nn.ReLU()]
            for _ in range(layer_nums[idx]):
                layers += [nn.Conv2d(num_filters[idx], num_filters[idx], kernel_size=3, padding=1, bias=False),
                           nn.BatchNorm2d(num_filters[idx], eps=1e-3, momentum=0.01), nn.ReLU()]
            self.blocks.append(nn.Sequential(*layers))
            s = upsample_strides[idx]
            self.deblocks.append(nn.Sequential(
                nn.ConvTranspose2d(num_filters[idx], num_upsample_filters[idx], s, stride=s, bias=False),
                nn.BatchNorm2d(num_upsample_filters[idx], eps=1e-3, momentum=0.01), nn.ReLU()))
        self.num_bev_features = sum(num_upsample_filters)

    def forward(self, data_dict):
        spatial_features = data_dict['spatial_features']
        ups, x = [], spatial_features
        for i in range(len(self.blocks)):
            x = self.blocks[i](x)
            stride = int(spatial_features.shape[2] / x.shape[2])
            data_dict['spatial_features_%dx' % stride] = x
            ups.append(self.deblocks[i](x))
        data_dict['spatial_features_2d'] = torch.cat(ups, dim=1)
        return data_dict


class SeparateHead(nn.Module):
    def __init__(self, input_channels, sep_head_dict, init_bias=-2.19, use_bias=False):
        super().__init__()
        self.sep_head_dict = sep_head_dict
        for cur_name in self.sep_head_dict:
            output_channels = self.sep_head_dict[cur_name]['out_channels']
            fc_list = []
            for _ in range(self.sep_head_dict[cur_name]['num_conv'] - 1):
                fc_list.append(nn.Sequential(
                    nn.Conv2d(input_channels, input_channels, kernel_size=3, stride=1, padding=1, bias=use_bias),
                    nn.BatchNorm2d(input_channels), nn.ReLU()))
            fc_list.append(nn.Conv2d(input_channels, output_channels, kernel_size=3, stride=1, padding=1, bias=True))
            fc = nn.Sequential(*fc_list)
            if 'hm' in cur_name:
                fc[-1].bias.data.fill_(init_bias)
            else:
                for m in fc.modules():
                    if isinstance(m, nn.Conv2d):
                        nn.init.kaiming_normal_(m.weight.data)
                        if m.bias is not None:
                            nn.init.constant_(m.bias, 0)
            self.__setattr__(cur_name, fc)

    def forward(self, x):
        return {name: self.__getattr__(name)(x) for name in self.sep_head_dict}


class CenterHead(nn.Module):
    """The plain CenterHead: towers in fp32 torch; target assignment and the focal + L1 loss of com_amd.hotpath (the
    elementwise torch form of the loss, `center_loss.CenterHeadLoss`, registered as `hm_loss_func`)."""

    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size,
                 predict_boxes_when_training=True):
        super().__init__()
        self.model_cfg, self.num_class, self.grid_size = model_cfg, num_class, grid_size
        self.point_cloud_range, self.voxel_size = point_cloud_range, voxel_size
        self.feature_map_stride = model_cfg.TARGET_ASSIGNER_CONFIG.get('FEATURE_MAP_STRIDE', None)
        self.class_names = class_names
        self.class_names_each_head = [[x for x in names if x in class_names] for names in model_cfg.CLASS_NAMES_EACH_HEAD]
        self.epoch = 0
        use_bias = model_cfg.get('USE_BIAS_BEFORE_NORM', False)
        self.shared_conv = nn.Sequential(
            nn.Conv2d(input_channels, model_cfg.SHARED_CONV_CHANNEL, 3, stride=1, padding=1, bias=use_bias),
            nn.BatchNorm2d(model_cfg.SHARED_CONV_CHANNEL), nn.ReLU())
        self.heads_list = nn.ModuleList()
        self.separate_head_cfg = model_cfg.SEPARATE_HEAD_CFG
        for names in self.class_names_each_head:
            d = copy.deepcopy(self.separate_head_cfg.HEAD_DICT)
            d['hm'] = dict(out_channels=len(names), num_conv=model_cfg.NUM_HM_CONV)
            self.heads_list.append(SeparateHead(model_cfg.SHARED_CONV_CHANNEL, d, init_bias=-2.19, use_bias=use_bias))
        self.predict_boxes_when_training = predict_boxes_when_training
        self.forward_ret_dict = {}
        self.build_losses()

    def build_losses(self):
        from com_amd.hotpath import center_loss
        lw = self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS
        self.add_module('hm_loss_func', center_loss.CenterHeadLoss(
            self.separate_head_cfg.HEAD_ORDER, cls_weight=lw['cls_weight'], loc_weight=lw['loc_weight'],
            code_weights=lw['code_weights']))

    def assign_targets(self, data_dict, feature_map_size):
        from com_amd.hotpath import targets
        ta = self.model_cfg.TARGET_ASSIGNER_CONFIG
        return targets.assign_targets(data_dict['gt_boxes'], feature_map_size, self.class_names, self.class_names_each_head,
                                      self.point_cloud_range, self.voxel_size, ta.FEATURE_MAP_STRIDE,
                                      num_max_objs=ta.NUM_MAX_OBJS, gaussian_overlap=ta.GAUSSIAN_OVERLAP,
                                      min_radius=ta.MIN_RADIUS)

    def get_loss(self):
        return self.hm_loss_func(self.forward_ret_dict['pred_dicts'], self.forward_ret_dict['target_dicts'])

    def forward(self, data_dict):
        sf = data_dict['spatial_features_2d']
        x = self.shared_conv(sf)
        pred_dicts = [head(x) for head in self.heads_list]
        if self.training:
            self.forward_ret_dict['target_dicts'] = self.assign_targets(data_dict, sf.size()[2:])
        self.forward_ret_dict['pred_dicts'] = pred_dicts
        data_dict['pred_dicts'] = pred_dicts
        return data_dict


class CurriculumCenterHead(CenterHead):
    conf_shape = None

    def build_losses(self):
        from com_amd.hotpath import com_head
        lw = self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS
        self.add_module('hm_loss_func', com_head.CurriculumCenterHeadLoss(
            self.separate_head_cfg.HEAD_ORDER, self.model_cfg.get('LOSS_CURRICULUM', None), conf_shape=self.conf_shape,
            cls_weight=lw['cls_weight'], loc_weight=lw['loc_weight'], code_weights=lw['code_weights']))

    def assign_targets(self, data_dict, feature_map_size):
        from com_amd.hotpath import com_head
        ta = self.model_cfg.TARGET_ASSIGNER_CONFIG
        group = com_head.cluster(data_dict['gt_boxes'], data_dict.get('true_object', None), data_dict['occupancy_ratio'],
                                 data_dict['facade_type'])
        return com_head.assign_targets(
            data_dict['gt_boxes'], feature_map_size, self.class_names, self.class_names_each_head, self.point_cloud_range,
            self.voxel_size, ta.FEATURE_MAP_STRIDE, data_dict['num_points_in_gt'], true_object=group,
            num_max_objs=ta.NUM_MAX_OBJS, gaussian_overlap=ta.GAUSSIAN_OVERLAP, min_radius=ta.MIN_RADIUS, epoch=self.epoch,
            epoch_threshold=ta.get('EPOCH_THRED', 100), min_points=ta.get('MIN_POINTS', 1))

    def get_loss(self):
        return self.hm_loss_func(self.forward_ret_dict['pred_dicts'], self.forward_ret_dict['target_dicts'], epoch=self.epoch)


class CurriculumCenterHead_x5(CurriculumCenterHead):
    conf_shape = (3, 96)


# ---------------------------------------------------------------------------------------------------------- detector
class StockDetector(nn.Module):
    """Detector3DTemplate + CenterPoint's forward / get_training_loss.  (tb_dict keeps the losses as device tensors: the
    reference's `.item()` there is a host read that a captured step cannot contain.)"""

    def __init__(self, model_cfg, num_class, class_names, grid_size, point_cloud_range, voxel_size, num_point_features=5):
        super().__init__()
        self.model_cfg, self.num_class, self.class_names = model_cfg, num_class, class_names
        self.register_buffer('global_step', torch.LongTensor(1).zero_())
        self.module_topology = ['vfe', 'backbone_3d', 'map_to_bev_module', 'pfe', 'backbone_2d', 'dense_head',
                                'point_head', 'roi_head']
        self._info = dict(grid_size=np.array(grid_size), point_cloud_range=np.array(point_cloud_range, np.float32),
                          voxel_size=list(voxel_size), num_point_features=num_point_features)
        self.module_list = self.build_networks()

    def update_global_step(self):
        self.global_step += 1

    def build_networks(self):
        cfg, info, module_list = self.model_cfg, self._info, []
        c = info['num_point_features']
        for name in self.module_topology:
            m = None
            if name == 'vfe' and cfg.get('VFE'):
                m = MeanVFE(cfg.VFE, c)
                c = m.get_output_feature_dim()
            elif name == 'backbone_3d' and cfg.get('BACKBONE_3D'):
                m = VoxelResBackBone8x(cfg.BACKBONE_3D, c, info['grid_size'])
                c = m.num_point_features
            elif name == 'map_to_bev_module' and cfg.get('MAP_TO_BEV'):
                m = HeightCompression(cfg.MAP_TO_BEV)
                c = m.num_bev_features
            elif name == 'backbone_2d' and cfg.get('BACKBONE_2D'):
                m = BaseBEVBackbone(cfg.BACKBONE_2D, c)
                c = m.num_bev_features
            elif name == 'dense_head' and cfg.get('DENSE_HEAD'):
                cls = {'CenterHead': CenterHead, 'CurriculumCenterHead': CurriculumCenterHead,
                       'CurriculumCenterHead_x5': CurriculumCenterHead_x5}[cfg.DENSE_HEAD.NAME]
                m = cls(cfg.DENSE_HEAD, c, self.num_class, self.class_names, info['grid_size'], info['point_cloud_range'],
                        info['voxel_size'], predict_boxes_when_training=False)
            if m is not None:
                module_list.append(m)
            self.add_module(name, m)
        return module_list

    def forward(self, batch_dict):
        for cur_module in self.module_list:
            batch_dict = cur_module(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {'loss': loss}, tb_dict, disp_dict
        return batch_dict, {}

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        return loss_rpn, {'loss_rpn': loss_rpn.detach(), **tb_dict}, {}


def model_cfg(kind, com_curriculum=None):
    """MODEL block of waymo_models/centerpoint.yaml (kind "centerpoint"), its 3-D part alone ("3d"), or with the COM head
    of com/centercurriculum_*_com.yaml ("com"); head hyper-parameters as bench.py uses them."""
    from com_amd.hotpath import dense2d
    d = {'NAME': 'CenterPoint', 'VFE': {'NAME': 'MeanVFE'}, 'BACKBONE_3D': {'NAME': 'VoxelResBackBone8x'},
         'MAP_TO_BEV': {'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 256}}
    if kind in ('centerpoint', 'com'):
        d['BACKBONE_2D'] = dict(NAME='BaseBEVBackbone', **dense2d.CENTERPOINT_BACKBONE_2D)
        head = copy.deepcopy(dense2d.CENTERPOINT_HEAD)
        head.update(NAME='CenterHead', CLASS_AGNOSTIC=False, CLASS_NAMES_EACH_HEAD=[list(CLASS_NAMES)],
                    TARGET_ASSIGNER_CONFIG=dict(FEATURE_MAP_STRIDE=8, NUM_MAX_OBJS=500, GAUSSIAN_OVERLAP=0.1, MIN_RADIUS=2),
                    LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(cls_weight=1.0, loc_weight=2.0, code_weights=[1.0] * 8)),
                    POST_PROCESSING=dict(SCORE_THRESH=0.1, POST_CENTER_LIMIT_RANGE=[-80, -80, -10.0, 80, 80, 10.0],
                                         MAX_OBJ_PER_SAMPLE=500,
                                         NMS_CONFIG=dict(NMS_TYPE='nms_gpu', NMS_THRESH=0.7, NMS_PRE_MAXSIZE=4096,
                                                         NMS_POST_MAXSIZE=500)))
        if kind == 'com':
            head['NAME'] = 'CurriculumCenterHead_x5'
            head['TARGET_ASSIGNER_CONFIG'].update(EPOCH_THRED=100, MIN_POINTS=0)
            head['LOSS_CURRICULUM'] = dict(com_curriculum or dict(UCL=False, THRESHOLD=0.2, ELONGATION=-10, HEIGHT=1,
                                                                  FIX=True))
        d['DENSE_HEAD'] = head
    return _cfg(d)


def build_detector(kind="3d", com_curriculum=None):
    """The stock detector on the CPU, Waymo grid of bench.py (move it with .to(device))."""
    grid = ops.grid_size(synth.WAYMO_RANGE, synth.WAYMO_VOXEL)
    return StockDetector(model_cfg(kind, com_curriculum), len(CLASS_NAMES), list(CLASS_NAMES), grid, synth.WAYMO_RANGE,
                         synth.WAYMO_VOXEL)
