"""A detector object shaped the way the reference's `Detector3DTemplate.build_networks` builds one (test infrastructure,
like tools/seam1_model.py): the modules of `module_topology` registered as attributes (`vfe`, `backbone_3d`,
`map_to_bev_module`, `backbone_2d`, `dense_head`, `roi_head`; None where the config has none), `module_list` a plain list of them,
a `global_step` buffer, `forward` iterating `module_list` and then `get_training_loss()` reading `self.dense_head`.

Every module is written the way a stock model file is written -- plain torch (`nn.Conv2d`, `nn.BatchNorm2d`, `nn.ReLU`,
`nn.ZeroPad2d`, `nn.ConvTranspose2d`) over the import seams (`spconv.*` names for the sparse backbone, the target
assignment and losses of com_amd.hotpath for the heads) -- with the reference's constructor arguments, module names and
state-dict keys.  `com_amd.adopt.adopt_model` turns such an object into the fused one in place.

    build_detector("3d")           MeanVFE -> VoxelResBackBone8x -> HeightCompression (bench.py's hot path)
    build_detector("centerpoint")  + BaseBEVBackbone + CenterHead                     (waymo_models/centerpoint.yaml)
    build_detector("com")          + BaseBEVBackbone + CurriculumCenterHead_x5         (the COM head, bench.py --com)
    build_detector("second")       MeanVFE -> VoxelBackBone8x -> HeightCompression -> BaseBEVBackbone -> AnchorHeadSingle,
                                   POST_PROCESSING on the detector                     (waymo_models/second.yaml)
    build_detector("second_multihead")  the same with AnchorHeadMulti: three one-class heads behind a shared conv,
                                   MULTI_CLASSES_NMS                                   (kitti_models/second_multihead.yaml)
    build_detector("second_iou")   "second" + the RoI head SECONDHead and the POST_PROCESSING of SECOND-IoU
                                                                                       (kitti_models/second_iou.yaml)
"""
import copy
import types
from functools import partial

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


class VoxelBackBone8x(nn.Module):
    """The plain (non-residual) sparse backbone of SECOND: conv -> BatchNorm1d -> ReLU triples (`post_act_block`), the norm
    and the activation applied by hand on `.features`; module names and state-dict keys of the stock file."""

    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        spconv, seq = seam1_model.spconv, seam1_model._PlainSeq
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        g = [int(v) for v in grid_size]
        self.sparse_shape = [g[2] + 1, g[1], g[0]]

        def subm(cin, cout, key, **kw):            # (the stock block hands a SubM conv no padding: it needs none)
            return seq(spconv.SubMConv3d(cin, cout, 3, bias=False, indice_key=key, **kw), norm_fn(cout))

        def down(cin, cout, key, k=3, s=2, p=1):
            return seq(spconv.SparseConv3d(cin, cout, k, stride=s, padding=p, bias=False, indice_key=key), norm_fn(cout))
        self.conv_input = subm(input_channels, 16, 'subm1', padding=1)
        self.conv1 = spconv.SparseSequential(subm(16, 16, 'subm1'))
        self.conv2 = spconv.SparseSequential(down(16, 32, 'spconv2'), subm(32, 32, 'subm2'), subm(32, 32, 'subm2'))
        self.conv3 = spconv.SparseSequential(down(32, 64, 'spconv3'), subm(64, 64, 'subm3'), subm(64, 64, 'subm3'))
        self.conv4 = spconv.SparseSequential(down(64, 64, 'spconv4', p=(0, 1, 1)), subm(64, 64, 'subm4'), subm(64, 64, 'subm4'))
        self.conv_out = down(64, 128, 'spconv_down2', k=(3, 1, 1), s=(2, 1, 1), p=0)
        self.num_point_features = 128
        self.backbone_channels = {'x_conv1': 16, 'x_conv2': 32, 'x_conv3': 64, 'x_conv4': 64}

    def forward(self, batch_dict):
        x = seam1_model.spconv.SparseConvTensor(features=batch_dict['voxel_features'].float(),
                                                indices=batch_dict['voxel_coords'].int(), spatial_shape=self.sparse_shape,
                                                batch_size=batch_dict['batch_size'])
        x = self.conv_input(x)
        x1 = self.conv1(x)
        x2 = self.conv2(x1)
        x3 = self.conv3(x2)
        x4 = self.conv4(x3)
        out = self.conv_out(x4)
        batch_dict.update({'encoded_spconv_tensor': out, 'encoded_spconv_tensor_stride': 8,
                           'multi_scale_3d_features': {'x_conv1': x1, 'x_conv2': x2, 'x_conv3': x3, 'x_conv4': x4}})
        return batch_dict


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


class _LossSlot(nn.Module):
    """Where the stock anchor head registers a loss module (`cls_loss_func`, `reg_loss_func`, `dir_loss_func`): no state;
    the three losses are computed together by com_amd.hotpath.anchor_head.anchor_loss."""


class AnchorHeadSingle(nn.Module):
    """The plain single anchor head: three 1 x 1 convs in fp32 torch over the NCHW map, permuted to [B, H, W, C]; the
    anchors kept as the template keeps them (`anchors`: one [1, H, W, sizes, rotations, 7] tensor per class,
    `num_anchors_per_location`, `box_coder`); target assignment, loss and box decoding of com_amd.hotpath.anchor_head."""

    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range,
                 predict_boxes_when_training=True, **kwargs):
        super().__init__()
        from com_amd.hotpath import anchor_head as AH
        self.model_cfg, self.num_class, self.class_names = model_cfg, num_class, class_names
        self.predict_boxes_when_training = predict_boxes_when_training
        self.use_multihead = model_cfg.get('USE_MULTIHEAD', False)
        ta = model_cfg.TARGET_ASSIGNER_CONFIG
        self.box_coder = AH.ResidualCoder(num_dir_bins=ta.get('NUM_DIR_BINS', 6), **ta.get('BOX_CODER_CONFIG', {}))
        ag_cfg = model_cfg.ANCHOR_GENERATOR_CONFIG
        grid_xy = np.asarray(grid_size)[:2]
        gen = AH.AnchorGenerator(point_cloud_range, ag_cfg)
        self.anchors, per_location = gen.generate_anchors([grid_xy // c['feature_map_stride'] for c in ag_cfg])
        self.num_anchors_per_location = sum(per_location)
        self.num_dir_bins = model_cfg.NUM_DIR_BINS
        kinds, classes, shifts, H, W = AH.anchor_tables(ag_cfg, list(class_names), point_cloud_range, grid_xy)
        self._tables_host = AH.AnchorTables(kinds, classes, shifts, H, W, num_class, self.num_dir_bins, model_cfg.DIR_OFFSET,
                                            model_cfg.DIR_LIMIT_OFFSET)
        self._tables = {}
        A = self.num_anchors_per_location
        self.conv_cls = nn.Conv2d(input_channels, A * num_class, kernel_size=1)
        self.conv_box = nn.Conv2d(input_channels, A * self.box_coder.code_size, kernel_size=1)
        self.conv_dir_cls = nn.Conv2d(input_channels, A * self.num_dir_bins, kernel_size=1)
        nn.init.constant_(self.conv_cls.bias, -np.log((1 - 0.01) / 0.01))
        nn.init.normal_(self.conv_box.weight, mean=0, std=0.001)
        self.forward_ret_dict = {}
        for name in ('cls_loss_func', 'reg_loss_func', 'dir_loss_func'):
            self.add_module(name, _LossSlot())

    def tables(self, device):
        from com_amd.hotpath import anchor_head as AH
        return AH.cached_tables(self, device)

    def get_loss(self):
        from com_amd.hotpath import anchor_head as AH
        f = self.forward_ret_dict
        preds = torch.cat([f['cls_preds'], f['box_preds'], f['dir_cls_preds']], dim=-1)
        lw = self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS
        code_weights = torch.tensor(lw['code_weights'], dtype=torch.float32, device=preds.device)
        loss, out = AH.anchor_loss(preds, f, self.tables(preds.device), code_weights, lw['cls_weight'], lw['loc_weight'],
                                   lw['dir_weight'])
        return loss, {'rpn_loss_cls': out[1], 'rpn_loss_loc': out[2], 'rpn_loss_dir': out[3], 'rpn_loss': out[0]}

    def forward(self, data_dict):
        from com_amd.hotpath import anchor_head as AH
        x = data_dict['spatial_features_2d']
        cls_preds = self.conv_cls(x).permute(0, 2, 3, 1).contiguous()
        box_preds = self.conv_box(x).permute(0, 2, 3, 1).contiguous()
        dir_cls_preds = self.conv_dir_cls(x).permute(0, 2, 3, 1).contiguous()
        self.forward_ret_dict = {'cls_preds': cls_preds, 'box_preds': box_preds, 'dir_cls_preds': dir_cls_preds}
        tab = self.tables(x.device)
        if self.training:
            self.forward_ret_dict.update(AH.assign_targets(tab, data_dict['gt_boxes']))
        if not self.training or self.predict_boxes_when_training:
            with torch.no_grad():
                batch_cls_preds, batch_box_preds = AH.decode_boxes(tab, cls_preds, box_preds, dir_cls_preds)
            data_dict['batch_cls_preds'] = batch_cls_preds
            data_dict['batch_box_preds'] = batch_box_preds
            data_dict['cls_preds_normalized'] = False
        return data_dict


def _plain_stack(c_in, c_mid, n_mid, c_out):
    """(conv3x3 without bias, BatchNorm2d, ReLU) x n_mid + conv3x3 with bias: a branch of a SEPARATE_REG_CONFIG head"""
    layers = []
    for _ in range(n_mid):
        layers += [nn.Conv2d(c_in, c_mid, kernel_size=3, stride=1, padding=1, bias=False), nn.BatchNorm2d(c_mid), nn.ReLU()]
        c_in = c_mid
    layers.append(nn.Conv2d(c_in, c_out, kernel_size=3, stride=1, padding=1, bias=True))
    return nn.Sequential(*layers)


class SingleHead(nn.Module):
    """One head of the plain multi-head anchor head: a (here always empty) BaseBEVBackbone tower -- `blocks` / `deblocks`
    stay in the module tree -- then `conv_cls`, `conv_box` (1 x 1 convs, or 3 x 3 stacks per SEPARATE_REG_CONFIG branch in
    a ModuleDict) and `conv_dir_cls`, buffer `head_label_indices`.  forward returns the maps as the convs write them,
    [B, A * items, H, W] (box branches concatenated in REG_LIST order): the layout com_amd.hotpath.anchor_head_multi's
    functions address with the stock view(-1, A, items, H, W) channel rule."""

    def __init__(self, model_cfg, input_channels, num_class, num_anchors_per_location, code_size, rpn_head_cfg=None,
                 head_label_indices=None, separate_reg_config=None):
        super().__init__()
        if rpn_head_cfg is not None and rpn_head_cfg.get('LAYER_NUMS'):
            raise NotImplementedError("stock SingleHead: a head tower (LAYER_NUMS) is not part of this test model")
        self.blocks, self.deblocks = nn.ModuleList(), nn.ModuleList()
        self.num_anchors_per_location, self.num_class, self.code_size = num_anchors_per_location, num_class, code_size
        self.model_cfg, self.separate_reg_config = model_cfg, separate_reg_config
        self.register_buffer('head_label_indices', head_label_indices)
        A = num_anchors_per_location
        if separate_reg_config is not None:
            n_mid, c_mid = separate_reg_config['NUM_MIDDLE_CONV'], separate_reg_config['NUM_MIDDLE_FILTER']
            self.conv_box = nn.ModuleDict()
            self.conv_box_names = []
            self.conv_cls = _plain_stack(input_channels, c_mid, n_mid, A * num_class)
            for reg_config in separate_reg_config['REG_LIST']:
                reg_name, reg_channel = reg_config.split(':')
                self.conv_box[f'conv_{reg_name}'] = _plain_stack(input_channels, c_mid, n_mid, A * int(reg_channel))
                self.conv_box_names.append(f'conv_{reg_name}')
            for m in self.conv_box.modules():
                if isinstance(m, nn.Conv2d):
                    nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                    if m.bias is not None:
                        nn.init.constant_(m.bias, 0)
        else:
            self.conv_cls = nn.Conv2d(input_channels, A * num_class, kernel_size=1)
            self.conv_box = nn.Conv2d(input_channels, A * code_size, kernel_size=1)
        if model_cfg.get('USE_DIRECTION_CLASSIFIER', None) is not None:
            self.conv_dir_cls = nn.Conv2d(input_channels, A * model_cfg['NUM_DIR_BINS'], kernel_size=1)
        else:
            self.conv_dir_cls = None
        last = self.conv_cls if isinstance(self.conv_cls, nn.Conv2d) else self.conv_cls[-1]
        nn.init.constant_(last.bias, -np.log((1 - 0.01) / 0.01))

    def forward(self, x):
        if self.separate_reg_config is None:
            box_preds = self.conv_box(x)
        else:
            box_preds = torch.cat([self.conv_box[name](x) for name in self.conv_box_names], dim=1)
        return {'cls_preds': self.conv_cls(x), 'box_preds': box_preds,
                'dir_cls_preds': self.conv_dir_cls(x) if self.conv_dir_cls is not None else None}


class AnchorHeadMulti(nn.Module):
    """The plain multi-head anchor head (USE_MULTIHEAD + SEPARATE_MULTIHEAD): `shared_conv` (conv3x3, BatchNorm2d, ReLU) and
    one SingleHead per RPN_HEAD_CFGS entry in fp32 torch; the anchors kept as the template keeps them (`anchors`: one tensor
    per class, `num_anchors_per_location`: one count per class, `box_coder`); target assignment, loss and box decoding of
    com_amd.hotpath.anchor_head_multi; the eager per-class post-processing is that module's `post_processing`."""

    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range,
                 predict_boxes_when_training=True, **kwargs):
        super().__init__()
        from com_amd.hotpath import anchor_head as AH, anchor_head_multi as AM
        self.model_cfg, self.num_class, self.class_names = model_cfg, num_class, class_names
        self.predict_boxes_when_training = predict_boxes_when_training
        self.use_multihead, self.separate_multihead = True, True
        self.use_dir = bool(model_cfg.get('USE_DIRECTION_CLASSIFIER', False))
        ta, ag_cfg, head_cfgs = model_cfg['TARGET_ASSIGNER_CONFIG'], model_cfg['ANCHOR_GENERATOR_CONFIG'], model_cfg['RPN_HEAD_CFGS']
        self.box_coder = AM.ResidualCoder(num_dir_bins=ta.get('NUM_DIR_BINS', 6), **(ta.get('BOX_CODER_CONFIG', None) or {}))
        sincos = self.box_coder.encode_angle_by_sincos
        grid_xy = np.asarray(grid_size)[:2]
        gen = AH.AnchorGenerator(point_cloud_range, ag_cfg)
        anchors, self.num_anchors_per_location = gen.generate_anchors([grid_xy // c['feature_map_stride'] for c in ag_cfg])
        if self.box_coder.code_size != 7:
            anchors = [torch.cat((a, a.new_zeros([*a.shape[:-1], self.box_coder.code_size - 7])), dim=-1) for a in anchors]
        self.anchors = anchors
        self.num_dir_bins = int(model_cfg.get('NUM_DIR_BINS', 2)) if self.use_dir else 1
        self._tables_host = AM.multi_tables(
            ag_cfg, list(class_names), point_cloud_range, grid_xy, [len(h['HEAD_CLS_NAME']) for h in head_cfgs],
            self.box_coder.code_size - int(sincos), sincos, self.num_dir_bins,
            model_cfg.get('DIR_OFFSET', 0.0) if self.use_dir else 0.0, model_cfg.get('DIR_LIMIT_OFFSET', 0.0) if self.use_dir else 0.0)
        self._tables = {}
        if model_cfg.get('SHARED_CONV_NUM_FILTER', None) is not None:
            c = model_cfg['SHARED_CONV_NUM_FILTER']
            self.shared_conv = nn.Sequential(nn.Conv2d(input_channels, c, 3, stride=1, padding=1, bias=False),
                                             nn.BatchNorm2d(c, eps=1e-3, momentum=0.01), nn.ReLU())
        else:
            self.shared_conv, c = None, input_channels
        names = [n for h in head_cfgs for n in h['HEAD_CLS_NAME']]
        heads = []
        for cfg in head_cfgs:
            per_location = sum(self.num_anchors_per_location[names.index(n)] for n in cfg['HEAD_CLS_NAME'])
            label_indices = torch.from_numpy(np.array([list(class_names).index(n) + 1 for n in cfg['HEAD_CLS_NAME']]))
            heads.append(SingleHead(model_cfg, c, len(cfg['HEAD_CLS_NAME']), per_location, self.box_coder.code_size, cfg,
                                    head_label_indices=label_indices,
                                    separate_reg_config=model_cfg.get('SEPARATE_REG_CONFIG', None)))
        self.rpn_heads = nn.ModuleList(heads)
        self.forward_ret_dict = {}
        for name in ('cls_loss_func', 'reg_loss_func', 'dir_loss_func'):
            self.add_module(name, _LossSlot())

    def tables(self, device):
        from com_amd.hotpath import anchor_head as AH
        return AH.cached_tables(self, device)

    def get_loss(self):
        from com_amd.hotpath import anchor_head_multi as AM
        f = self.forward_ret_dict
        dev = f['cls_preds'][0].device
        lc = self.model_cfg['LOSS_CONFIG']
        lw = lc['LOSS_WEIGHTS']
        settings = AM.LossSettings(self.num_class, lc.get('REG_LOSS_TYPE', None) == 'WeightedL1Loss', lw.get('pos_cls_weight', 1.0),
                                   lw.get('neg_cls_weight', 1.0), lw['cls_weight'], lw['loc_weight'], lw.get('dir_weight', 0.0),
                                   self.use_dir)
        code_weights = torch.tensor(lw['code_weights'], dtype=torch.float32, device=dev)
        loss, out = AM.multi_loss(f['cls_preds'], f['box_preds'], f.get('dir_cls_preds'), f, self.tables(dev), code_weights,
                                  settings)
        tb = {'rpn_loss_cls': out[1], 'rpn_loss_loc': out[2], 'rpn_loss': out[0]}
        if self.use_dir:
            tb['rpn_loss_dir'] = out[3]
        return loss, tb

    def forward(self, data_dict):
        from com_amd.hotpath import anchor_head_multi as AM
        x = data_dict['spatial_features_2d']
        if self.shared_conv is not None:
            x = self.shared_conv(x)
        rets = [head(x) for head in self.rpn_heads]
        ret = {'cls_preds': [r['cls_preds'] for r in rets], 'box_preds': [r['box_preds'] for r in rets]}
        if self.use_dir:
            ret['dir_cls_preds'] = [r['dir_cls_preds'] for r in rets]
        self.forward_ret_dict.update(ret)
        tab = self.tables(x.device)
        if self.training:
            self.forward_ret_dict.update(AM.assign_targets(tab, data_dict['gt_boxes']))
        if not self.training or self.predict_boxes_when_training:
            with torch.no_grad():
                batch_cls_preds, batch_box_preds = AM.decode_boxes(tab, ret['cls_preds'], ret['box_preds'],
                                                                   ret.get('dir_cls_preds', None))
            data_dict['multihead_label_mapping'] = [head.head_label_indices for head in self.rpn_heads]
            data_dict['batch_cls_preds'] = batch_cls_preds
            data_dict['batch_box_preds'] = batch_box_preds
            data_dict['cls_preds_normalized'] = False
        return data_dict


class SECONDHead(nn.Module):
    """The plain IoU head of SECOND-IoU: `shared_fc_layer` (Conv1d, BatchNorm1d, ReLU[, Dropout] per SHARED_FC width) and
    `iou_layers` (the same per IOU_FC width, then a Conv1d to one logit) in fp32 torch, xavier-initialised; the proposal
    layer, the BEV RoI grid pooling and the score rectification of com_amd.hotpath (the eager forms).  Inference only: the
    stock training half (target layer, IoU loss) is not rebuilt here."""

    def __init__(self, input_channels, model_cfg, num_class=1, point_cloud_range=None, voxel_size=None, **kwargs):
        super().__init__()
        self.model_cfg, self.num_class = model_cfg, num_class
        self.point_cloud_range, self.voxel_size = point_cloud_range, voxel_size
        pool = model_cfg.ROI_GRID_POOL
        c = pool.IN_CHANNEL * pool.GRID_SIZE * pool.GRID_SIZE
        layers = []
        for k, width in enumerate(model_cfg.SHARED_FC):
            layers += [nn.Conv1d(c, width, kernel_size=1, bias=False), nn.BatchNorm1d(width), nn.ReLU()]
            c = width
            if k != len(model_cfg.SHARED_FC) - 1 and model_cfg.DP_RATIO > 0:
                layers.append(nn.Dropout(model_cfg.DP_RATIO))
        self.shared_fc_layer = nn.Sequential(*layers)
        layers = []
        for width in model_cfg.IOU_FC:
            layers += [nn.Conv1d(c, width, kernel_size=1, bias=False), nn.BatchNorm1d(width), nn.ReLU()]
            c = width
            if model_cfg.DP_RATIO >= 0 and len(layers) == 3:
                layers.append(nn.Dropout(model_cfg.DP_RATIO))
        layers.append(nn.Conv1d(c, 1, kernel_size=1, bias=True))
        self.iou_layers = nn.Sequential(*layers)
        for m in self.modules():
            if isinstance(m, nn.Conv1d):
                nn.init.xavier_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def forward(self, batch_dict):
        from com_amd.hotpath import roi_head as RH
        from com_amd.hotpath import second_head as SH
        if self.training:
            raise NotImplementedError("the stock SECONDHead here is an inference module")
        RH.RoIHeadTemplate.proposal_layer(self, batch_dict, nms_config=self.model_cfg.NMS_CONFIG.TEST)
        pool = self.model_cfg.ROI_GRID_POOL
        pcr, vs = self.point_cloud_range, self.voxel_size
        pooled = SH.bev_roi_grid_pool(batch_dict['spatial_features_2d'], batch_dict['rois'], pool.GRID_SIZE, pcr[0], pcr[1],
                                      vs[0] * pool.DOWNSAMPLE_RATIO, vs[1] * pool.DOWNSAMPLE_RATIO)
        shared = self.shared_fc_layer(pooled.view(pooled.shape[0], -1, 1).float())
        rcnn_iou = self.iou_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        batch_dict['batch_cls_preds'] = rcnn_iou.view(batch_dict['batch_size'], -1, rcnn_iou.shape[-1])
        batch_dict['batch_box_preds'] = batch_dict['rois']
        batch_dict['cls_preds_normalized'] = False
        return batch_dict

    def post_processing(self, batch_dict, post_process_cfg, class_names):
        from com_amd.hotpath import second_head as SH
        return SH.post_processing(batch_dict, post_process_cfg, class_names)


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
        # (Detector3DTemplate keeps its dataset; an anchor head's grid_size / point_cloud_range are read from it)
        self.dataset = types.SimpleNamespace(class_names=class_names, grid_size=self._info['grid_size'],
                                             point_cloud_range=self._info['point_cloud_range'], voxel_size=list(voxel_size))
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
                cls = {'VoxelResBackBone8x': VoxelResBackBone8x, 'VoxelBackBone8x': VoxelBackBone8x}[cfg.BACKBONE_3D.NAME]
                m = cls(cfg.BACKBONE_3D, c, info['grid_size'])
                c = m.num_point_features
            elif name == 'map_to_bev_module' and cfg.get('MAP_TO_BEV'):
                m = HeightCompression(cfg.MAP_TO_BEV)
                c = m.num_bev_features
            elif name == 'backbone_2d' and cfg.get('BACKBONE_2D'):
                m = BaseBEVBackbone(cfg.BACKBONE_2D, c)
                c = m.num_bev_features
            elif name == 'dense_head' and cfg.get('DENSE_HEAD') and cfg.DENSE_HEAD.NAME in ('AnchorHeadSingle', 'AnchorHeadMulti'):
                cls = {'AnchorHeadSingle': AnchorHeadSingle, 'AnchorHeadMulti': AnchorHeadMulti}[cfg.DENSE_HEAD.NAME]
                m = cls(cfg.DENSE_HEAD, c, self.num_class, self.class_names, info['grid_size'], info['point_cloud_range'],
                        predict_boxes_when_training=False)
            elif name == 'dense_head' and cfg.get('DENSE_HEAD'):
                cls = {'CenterHead': CenterHead, 'CurriculumCenterHead': CurriculumCenterHead,
                       'CurriculumCenterHead_x5': CurriculumCenterHead_x5}[cfg.DENSE_HEAD.NAME]
                m = cls(cfg.DENSE_HEAD, c, self.num_class, self.class_names, info['grid_size'], info['point_cloud_range'],
                        info['voxel_size'], predict_boxes_when_training=False)
            elif name == 'roi_head' and cfg.get('ROI_HEAD'):
                m = {'SECONDHead': SECONDHead}[cfg.ROI_HEAD.NAME](
                    c, cfg.ROI_HEAD, num_class=self.num_class if not cfg.ROI_HEAD.CLASS_AGNOSTIC else 1,
                    point_cloud_range=[float(v) for v in info['point_cloud_range']], voxel_size=info['voxel_size'])
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


def _anchor_class(name, size, matched, unmatched):
    return dict(class_name=name, anchor_sizes=[size], anchor_rotations=[0, 1.57], anchor_bottom_heights=[0],
                align_center=False, feature_map_stride=8, matched_threshold=matched, unmatched_threshold=unmatched)


# MODEL block of waymo_models/second.yaml
SECOND_MODEL = dict(
    NAME='SECONDNet', VFE=dict(NAME='MeanVFE'), BACKBONE_3D=dict(NAME='VoxelBackBone8x'),
    MAP_TO_BEV=dict(NAME='HeightCompression', NUM_BEV_FEATURES=256),
    BACKBONE_2D=dict(NAME='BaseBEVBackbone', LAYER_NUMS=[5, 5], LAYER_STRIDES=[1, 2], NUM_FILTERS=[128, 256],
                     UPSAMPLE_STRIDES=[1, 2], NUM_UPSAMPLE_FILTERS=[256, 256]),
    DENSE_HEAD=dict(
        NAME='AnchorHeadSingle', CLASS_AGNOSTIC=False, USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539,
        DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
        ANCHOR_GENERATOR_CONFIG=[_anchor_class('Vehicle', [4.7, 2.1, 1.7], 0.55, 0.4),
                                 _anchor_class('Pedestrian', [0.91, 0.86, 1.73], 0.5, 0.35),
                                 _anchor_class('Cyclist', [1.78, 0.84, 1.78], 0.5, 0.35)],
        TARGET_ASSIGNER_CONFIG=dict(NAME='AxisAlignedTargetAssigner', POS_FRACTION=-1.0, SAMPLE_SIZE=512,
                                    NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False, BOX_CODER='ResidualCoder'),
        LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, code_weights=[1.0] * 7))),
    POST_PROCESSING=dict(RECALL_THRESH_LIST=[0.3, 0.5, 0.7], SCORE_THRESH=0.1, OUTPUT_RAW_SCORE=False, EVAL_METRIC='waymo',
                         NMS_CONFIG=dict(MULTI_CLASSES_NMS=False, NMS_TYPE='nms_gpu', NMS_THRESH=0.7, NMS_PRE_MAXSIZE=4096,
                                         NMS_POST_MAXSIZE=500)))


def _second_multihead_model():
    """SECOND_MODEL with the dense head and POST_PROCESSING of kitti_models/second_multihead.yaml on the three classes here:
    three one-class heads behind a 64-channel shared conv, direction classifier, per-class NMS."""
    d = copy.deepcopy(SECOND_MODEL)
    head = d['DENSE_HEAD']
    head.update(NAME='AnchorHeadMulti', USE_MULTIHEAD=True, SEPARATE_MULTIHEAD=True, SHARED_CONV_NUM_FILTER=64,
                RPN_HEAD_CFGS=[dict(HEAD_CLS_NAME=[n]) for n in CLASS_NAMES])
    d['POST_PROCESSING'].update(MULTI_CLASSES_NMS=True, SCORE_THRESH=0.1)
    d['POST_PROCESSING']['NMS_CONFIG'].update(MULTI_CLASSES_NMS=True, NMS_TYPE='nms_gpu', NMS_THRESH=0.1, NMS_PRE_MAXSIZE=4096,
                                              NMS_POST_MAXSIZE=500)
    return d


def _second_iou_model():
    """SECOND_MODEL with ROI_HEAD and POST_PROCESSING of kitti_models/second_iou.yaml on the three classes here (detector
    SECONDNetIoU: AnchorHeadSingle -> SECONDHead, the score rectification of SECONDNetIoU.post_processing)."""
    d = copy.deepcopy(SECOND_MODEL)
    d['NAME'] = 'SECONDNetIoU'
    nms = dict(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False)
    d['ROI_HEAD'] = dict(
        NAME='SECONDHead', CLASS_AGNOSTIC=True, SHARED_FC=[256, 256], IOU_FC=[256, 256], DP_RATIO=0.3,
        NMS_CONFIG=dict(TRAIN=dict(nms, NMS_PRE_MAXSIZE=9000, NMS_POST_MAXSIZE=512, NMS_THRESH=0.8),
                        TEST=dict(nms, NMS_PRE_MAXSIZE=1024, NMS_POST_MAXSIZE=100, NMS_THRESH=0.7)),
        ROI_GRID_POOL=dict(GRID_SIZE=7, IN_CHANNEL=512, DOWNSAMPLE_RATIO=8),
        TARGET_CONFIG=dict(BOX_CODER='ResidualCoder', ROI_PER_IMAGE=128, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True,
                           CLS_SCORE_TYPE='roi_iou', CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1,
                           HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55),
        LOSS_CONFIG=dict(IOU_LOSS='BinaryCrossEntropy', LOSS_WEIGHTS=dict(rcnn_iou_weight=1.0, code_weights=[1.0] * 7)))
    d['POST_PROCESSING'] = dict(RECALL_THRESH_LIST=[0.3, 0.5, 0.7], SCORE_THRESH=0.1, OUTPUT_RAW_SCORE=False, EVAL_METRIC='kitti',
                                NMS_CONFIG=dict(MULTI_CLASSES_NMS=False, NMS_TYPE='nms_gpu', NMS_THRESH=0.01,
                                                NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=500))
    return d


def model_cfg(kind, com_curriculum=None):
    """MODEL block of waymo_models/centerpoint.yaml (kind "centerpoint"), its 3-D part alone ("3d"), with the COM head
    of com/centercurriculum_*_com.yaml ("com"), of waymo_models/second.yaml ("second"), or that with the multi-head dense
    head of kitti_models/second_multihead.yaml ("second_multihead") or with the RoI head of kitti_models/second_iou.yaml
    ("second_iou"); head hyper-parameters as bench.py uses them."""
    from com_amd.hotpath import dense2d
    if kind == 'second':
        return _cfg(SECOND_MODEL)
    if kind == 'second_multihead':
        return _cfg(_second_multihead_model())
    if kind == 'second_iou':
        return _cfg(_second_iou_model())
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
