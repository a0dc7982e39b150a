"""PointPillarFuseBEVT — the LiDAR leg of CoBEVT from real voxels: PillarVFE -> PointPillarScatter -> regroup -> FuseBEVT
(SwapFusionEncoder), i.e. opencood's pillar_vfe.py / point_pillar_scatter.py / fuse_utils.regroup in front of
fusion_modules/swap_fusion_modules.py.  OpenCOOD projects every agent's points into the ego frame before voxelisation, so there is
no STTF warp here.

args: voxel_size [x, y, z]; lidar_range [x0, y0, z0, x1, y1, z1]; max_cav; pillar_vfe {use_norm, with_distance, use_absolute_xyz,
num_filters: [64]}; point_pillar_scatter {num_features: 64, grid_size: [nx, ny, 1]}; fax_fusion: SwapFusionEncoder's arguments;
optionally preprocess {args: {voxel_size, max_points_per_voxel, max_voxel_train, max_voxel_test}, cav_lidar_range}: SpVoxelPreprocessor's
arguments (its grid must be the scatter's).  With it a batch may carry raw points, batch_dict['lidar_points'] (M, 4) fp32 and
batch_dict['lidar_point_offsets'] (N + 1,) on the device, INSTEAD of processed_lidar: the forward voxelises them on the device
(ops.voxelize_points, voxel cap by train() / eval()) and continues with that dict, in both modes.

forward(batch_dict): batch_dict['processed_lidar'] = {voxel_features (P, T <= 32, 4) fp32, voxel_coords (P, 4) [n, z, y, x],
voxel_num_points (P,)} and batch_dict['record_len'] (B,) -> {'fused_feature': (B, 64, ny, nx)} fp32.  The front end is ONE operator
call (two launches) from the voxels straight into the (B, max_cav, ny, nx, 64) canvas FuseBEVT reads; rows whose batch index is
negative are skipped, which is how a caller pads P to a fixed size for graph replay.  In train() mode the forward is the differentiable
graph of host/training.point_pillar_fusebevt (batch statistics over the pillars the operator writes; parameter gradients).

Optional args['anchor_number'] = A adds the detection head OpenCOOD's PointPillar models carry: cls_head (64 -> A, 1 x 1, bias) and
reg_head (64 -> 7A), and the forward adds 'psm' (B, A, ny, nx) and 'rm' (B, 7A, ny, nx) in fp32 - both from ONE dense product of the
concatenated weights over the fused rows (ops.linear) - for host.VoxelPostprocessor.post_process.  In train() mode on ROCm tensors
both heads run as autograd.conv2d and take the gradient host.PointPillarLoss returns; on CPU tensors train() with the argument set
raises.  Without the argument the state_dict and the outputs are unchanged.

Optional args['base_bev_backbone'] = model_cfg (BaseBEVBackbone's: layer_nums, layer_strides, num_filters, upsample_strides,
num_upsample_filter) puts OpenCOOD's 2-D backbone, parameters under backbone.*, on the fused (B, ny, nx, 64) map, between FuseBEVT and
the heads.  The reference ships no model that wires this class behind FuseBEVT, so the position is this package's choice, for two
reasons: FuseBEVT's kernels are built for 64 / 128 channels (not the backbone's 384), and after fusion the backbone runs on B maps
instead of B * max_cav.  With it cls_head / reg_head take backbone.num_bev_features inputs, psm / rm come out at the backbone's
resolution (the standard layer_strides [2, 2, 2] / upsample_strides [1, 2, 4] give ny / 2 x nx / 2, what VoxelPostprocessor's default
feature_stride = 2 expects), the output gains 'spatial_features_2d' (B, num_bev_features, H', W') fp32 and 'fused_feature' is
unchanged.  In train() mode on ROCm tensors the backbone runs as host/training.base_bev_backbone on the fused map (batch statistics,
autograd.deconv); on CPU tensors train() with the argument set raises.  Without the argument the state_dict, the outputs and the
launch sequence are unchanged."""
import torch
import torch.nn as nn

from .. import ops
from ..lib import CobevtHipError
from . import runtime as rt
from . import training
from .base_bev_backbone import BaseBEVBackbone
from .pillar_vfe import PillarVFE
from .point_pillar_scatter import PointPillarScatter
from .runtime import HipModule
from .sp_voxel_preprocessor import SpVoxelPreprocessor
from .swap_fusion_modules import SwapFusionEncoder


class PointPillarFuseBEVT(HipModule):
    def __init__(self, args):
        super().__init__()
        self.max_cav = args["max_cav"]
        vfe_cfg = dict(args["pillar_vfe"])
        if "max_points_per_voxel" in args and "max_points_per_voxel" not in vfe_cfg:
            vfe_cfg["max_points_per_voxel"] = args["max_points_per_voxel"]
        pre = args.get("preprocess")
        if pre is not None and "max_points_per_voxel" not in vfe_cfg:
            vfe_cfg["max_points_per_voxel"] = pre["args"]["max_points_per_voxel"]
        self.pillar_vfe = PillarVFE(vfe_cfg, num_point_features=4, voxel_size=args["voxel_size"],
                                    point_cloud_range=args["lidar_range"])
        self.scatter = PointPillarScatter(args["point_pillar_scatter"])
        self.fusion_net = SwapFusionEncoder(args["fax_fusion"])
        c = self.pillar_vfe.get_output_feature_dim()
        if self.scatter.num_bev_features != c or args["fax_fusion"]["input_dim"] != c:
            raise CobevtHipError("PointPillarFuseBEVT: point_pillar_scatter.num_features and fax_fusion.input_dim must equal the "
                                 "PFN layer's %d channels" % c)
        if self.max_cav < 1:
            raise CobevtHipError("PointPillarFuseBEVT: max_cav must be at least 1")
        self.backbone = None
        if args.get("base_bev_backbone") is not None:
            self.backbone = BaseBEVBackbone(args["base_bev_backbone"], c)
            c = self.backbone.num_bev_features
        self.anchor_number = args.get("anchor_number")
        if self.anchor_number is not None:
            if int(self.anchor_number) < 1:
                raise CobevtHipError("PointPillarFuseBEVT: anchor_number must be at least 1, got %r" % (self.anchor_number,))
            self.anchor_number = int(self.anchor_number)
            self.cls_head = nn.Conv2d(c, self.anchor_number, kernel_size=1)
            self.reg_head = nn.Conv2d(c, 7 * self.anchor_number, kernel_size=1)
        # plain objects without parameters: the state_dict is the same with and without `preprocess`
        self.preprocessors = None
        if pre is not None:
            self.preprocessors = {train: SpVoxelPreprocessor(pre, train) for train in (False, True)}
            grid = tuple(self.preprocessors[False].grid_size)
            if grid != (self.scatter.nx, self.scatter.ny, self.scatter.nz):
                raise CobevtHipError("PointPillarFuseBEVT: preprocess gives the grid %r (round((cav_lidar_range hi - lo) / voxel_size)), "
                                     "point_pillar_scatter.grid_size is %r" % (list(grid), [self.scatter.nx, self.scatter.ny, self.scatter.nz]))

    def with_voxels(self, batch_dict):
        """batch_dict as it is when it carries processed_lidar; otherwise a copy with processed_lidar voxelised from lidar_points /
        lidar_point_offsets on the device"""
        if "processed_lidar" in batch_dict:
            return batch_dict
        if "lidar_points" not in batch_dict or "lidar_point_offsets" not in batch_dict:
            raise CobevtHipError("PointPillarFuseBEVT: the batch carries neither processed_lidar nor lidar_points + lidar_point_offsets")
        if self.preprocessors is None:
            raise CobevtHipError("PointPillarFuseBEVT: lidar_points need the model's args['preprocess'] section (voxel_size, "
                                 "max_points_per_voxel, max_voxel_train / max_voxel_test, cav_lidar_range); without it pass processed_lidar")
        out = dict(batch_dict)
        out["processed_lidar"] = self.preprocessors[bool(self.training)].preprocess_batch(batch_dict["lidar_points"],
                                                                                          batch_dict["lidar_point_offsets"])
        return out

    def front_end(self, batch_dict, out=None):
        """voxels -> (canvas (B, max_cav, ny, nx, 64) in the compute dtype, cav_mask (B, max_cav) fp32): one operator call"""
        lidar = self.with_voxels(batch_dict)["processed_lidar"]
        vf, coords, npts = lidar["voxel_features"], lidar["voxel_coords"], lidar["voxel_num_points"]
        self._require_inference(vf, coords, npts)
        rl = torch.as_tensor(batch_dict["record_len"]).to(device=vf.device, dtype=torch.int32)
        w, shift = self.pillar_vfe.pfn_layers[0].folded()
        return ops.pillar_vfe_scatter(vf, npts, coords, w, shift, self.pillar_vfe.geom(), (self.scatter.ny, self.scatter.nx),
                                      rt.get_compute_dtype(), use_absolute_xyz=self.pillar_vfe.use_absolute_xyz,
                                      with_distance=self.pillar_vfe.with_distance, record_len=rl, max_cav=self.max_cav, out=out)

    def _head_plan(self):
        """cls_head and reg_head as one (8A, C) dense layer"""
        tensors = [self.cls_head.weight, self.cls_head.bias, self.reg_head.weight, self.reg_head.bias]

        def build(dt, dev):
            w = torch.cat([self.cls_head.weight.detach().flatten(1), self.reg_head.weight.detach().flatten(1)])
            return ops.ConvPlan(w, torch.cat([self.cls_head.bias.detach(), self.reg_head.bias.detach()]), dtype=dt, device=dev)
        return self._plan("det_head", tensors, build)

    @staticmethod
    def on_device(batch_dict):
        """whether the batch's voxels (or raw points) are ROCm tensors: what a train()-mode forward needs"""
        lidar = batch_dict.get("processed_lidar")
        t = lidar.get("voxel_features") if isinstance(lidar, dict) else batch_dict.get("lidar_points")
        return torch.is_tensor(t) and t.is_cuda

    def forward(self, batch_dict):
        trains = self.training and self.on_device(batch_dict)
        if self.training and not trains and self.anchor_number is not None:
            raise CobevtHipError("PointPillarFuseBEVT: the detection head (args['anchor_number']) is inference only - the reference has no "
                                 "detection loss to train it with; call .eval(), or build the model without anchor_number to train")
        if self.training and not trains and self.backbone is not None:
            raise CobevtHipError("PointPillarFuseBEVT: the 2-D backbone (args['base_bev_backbone']) is inference only - its transposed "
                                 "convolutions have no backward; call .eval(), or build the model without base_bev_backbone to train")
        batch_dict = self.with_voxels(batch_dict)
        if self.training and training.lidar_trains(self.pillar_vfe.pfn_layers[0], batch_dict["processed_lidar"]["voxel_features"]):
            return training.point_pillar_fusebevt(self, batch_dict)
        self._require_inference()
        x, cav_mask = self.front_end(batch_dict)
        b, l, h, w, _ = x.shape
        # the agent mask as CorpBEVT.fuse_and_decode builds it without an ROI mask (corpbevt.py:125-128)
        com_mask = cav_mask[:, None, None, None, :].expand(b, h, w, 1, l).contiguous()
        fused = self.fusion_net.forward_blhwc(x, com_mask)                      # (B, ny, nx, 64)
        out = {"fused_feature": rt.nchw_view(fused).float()}
        feat = fused
        if self.backbone is not None:
            feat = self.backbone.forward_nhwc(fused)                            # (B, H', W', num_bev_features)
            out["spatial_features_2d"] = rt.nchw_view(feat).float()
        if self.anchor_number is not None:
            a = self.anchor_number
            maps = rt.nchw_view(ops.linear(feat, self._head_plan())).float()    # (B, 8A, H', W'): A class maps, then 7A deltas
            out["psm"] = maps[:, :a].contiguous()
            out["rm"] = maps[:, a:].contiguous()
        return out
