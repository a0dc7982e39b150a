"""PointPillarIntermediate — OpenCOOD's intermediate-fusion LiDAR detector, PointPillar with attentive fusion
(opencood/models/point_pillar_intermediate.py upstream; the reference tree carries its parts, not the model file):
PillarVFE -> PointPillarScatter -> AttBEVBackbone -> cls_head / reg_head, under OpenCOOD's attribute names (pillar_vfe, scatter,
backbone, cls_head, reg_head), so an OpenCOOD checkpoint's keys load.  OpenCOOD projects every agent's points into the ego frame
before voxelisation, so there is no warp.

args: voxel_size, lidar_range, pillar_vfe {...}, point_pillar_scatter {num_features: 64, grid_size: [nx, ny, 1]}, base_bev_backbone
(AttBEVBackbone's model_cfg, with the optional `compression`), anchor_number; optionally `preprocess` as in PointPillarFuseBEVT (a
batch may then carry raw lidar_points / lidar_point_offsets instead of processed_lidar).

forward(batch_dict): processed_lidar {voxel_features (P, T <= 32, 4), voxel_coords (P, 4) [n, z, y, x], voxel_num_points (P,)} and
record_len (B,) -> {'psm' (B, A, H', W'), 'rm' (B, 7A, H', W'), 'spatial_features_2d' (B, num_bev_features, H', W')} in fp32.
The front end is ops.pillar_vfe_scatter WITHOUT regrouping: one canvas per agent, (N, ny, nx, 64); the backbone fuses the agents at
each of its levels; both heads are one ops.linear over the fused rows.  The canvas's N = sum(record_len) is an allocation size, so
the host has to know it: a record_len that lives on the host (a list, a CPU tensor, as the dataset's collate makes it) is summed
there; with a device record_len the batch carries it as batch_dict['num_agents'] (a host integer).  Either way the forward performs
no host synchronisation and can be captured in a HIP graph.  In train() mode on ROCm tensors the forward is the differentiable graph of
host/training.point_pillar_intermediate (the pillar front end with batch statistics, the attentive backbone, both heads), whose psm /
rm take the gradient host.PointPillarLoss returns; on CPU tensors a train()-mode forward raises."""
import torch
import torch.nn as nn

from .. import ops
from ..lib import CobevtHipError
from . import runtime as rt
from . import training
from .att_bev_backbone import AttBEVBackbone
from .pillar_vfe import PillarVFE
from .point_pillar_fusebevt import PointPillarFuseBEVT
from .point_pillar_scatter import PointPillarScatter
from .runtime import HipModule
from .self_attn import record_len_i32
from .sp_voxel_preprocessor import SpVoxelPreprocessor


class PointPillarIntermediate(HipModule):
    def __init__(self, args):
        super().__init__()
        vfe_cfg = dict(args["pillar_vfe"])
        pre = args.get("preprocess")
        if "max_points_per_voxel" in args and "max_points_per_voxel" not in vfe_cfg:
            vfe_cfg["max_points_per_voxel"] = args["max_points_per_voxel"]
        if pre is not None and "max_points_per_voxel" not in vfe_cfg:
            vfe_cfg["max_points_per_voxel"] = pre["args"]["max_points_per_voxel"]
        self.pillar_vfe = PillarVFE(vfe_cfg, num_point_features=4, voxel_size=args["voxel_size"], point_cloud_range=args["lidar_range"])
        self.scatter = PointPillarScatter(args["point_pillar_scatter"])
        c = self.pillar_vfe.get_output_feature_dim()
        if self.scatter.num_bev_features != c:
            raise CobevtHipError("PointPillarIntermediate: point_pillar_scatter.num_features must equal the PFN layer's %d channels" % c)
        self.backbone = AttBEVBackbone(args["base_bev_backbone"], c)
        self.anchor_number = int(args["anchor_number"])
        if self.anchor_number < 1:
            raise CobevtHipError("PointPillarIntermediate: anchor_number must be at least 1, got %r" % (args["anchor_number"],))
        self.cls_head = nn.Conv2d(self.backbone.num_bev_features, self.anchor_number, kernel_size=1)
        self.reg_head = nn.Conv2d(self.backbone.num_bev_features, 7 * self.anchor_number, kernel_size=1)
        # plain objects without parameters: the state_dict is the same with and without `preprocess`
        self.preprocessors = None
        if pre is not None:
            self.preprocessors = {train: SpVoxelPreprocessor(pre, train) for train in (False, True)}
            grid = tuple(self.preprocessors[False].grid_size)
            if grid != (self.scatter.nx, self.scatter.ny, self.scatter.nz):
                raise CobevtHipError("PointPillarIntermediate: preprocess gives the grid %r, point_pillar_scatter.grid_size is %r"
                                     % (list(grid), [self.scatter.nx, self.scatter.ny, self.scatter.nz]))

    # the same batch convention and the same fused head as the FuseBEVT model: its code, not a copy
    with_voxels = PointPillarFuseBEVT.with_voxels
    _head_plan = PointPillarFuseBEVT._head_plan

    @staticmethod
    def num_agents(batch_dict):
        """sum(record_len) without touching the device"""
        if batch_dict.get("num_agents") is not None:
            return int(batch_dict["num_agents"])
        rl = batch_dict["record_len"]
        if isinstance(rl, torch.Tensor) and rl.is_cuda:
            raise CobevtHipError("PointPillarIntermediate: record_len is on the device, and its sum sizes the agents' canvas: pass "
                                 "batch_dict['num_agents'] (a host integer) with it, or a host record_len - the forward does not synchronise")
        return int(torch.as_tensor(rl).sum())

    def front_end(self, batch_dict, out=None):
        """voxels -> one canvas per agent, (N, ny, nx, 64) in the compute dtype: one operator call"""
        lidar = self.with_voxels(batch_dict)["processed_lidar"]
        vf, coords, npts = lidar["voxel_features"], lidar["voxel_coords"], lidar["voxel_num_points"]
        self._require_inference(vf, coords, npts)
        w, shift = self.pillar_vfe.pfn_layers[0].folded()
        canvas, _ = ops.pillar_vfe_scatter(vf, npts, coords, w, shift, self.pillar_vfe.geom(), (self.scatter.ny, self.scatter.nx),
                                           rt.get_compute_dtype(), use_absolute_xyz=self.pillar_vfe.use_absolute_xyz,
                                           with_distance=self.pillar_vfe.with_distance, num_agents=self.num_agents(batch_dict), out=out)
        return canvas

    def forward(self, batch_dict):
        if self.training and PointPillarFuseBEVT.on_device(batch_dict):
            batch_dict = self.with_voxels(batch_dict)
            if training.lidar_trains(self.pillar_vfe.pfn_layers[0], batch_dict["processed_lidar"]["voxel_features"]):
                return training.point_pillar_intermediate(self, batch_dict)
        self._require_inference()
        batch_dict = self.with_voxels(batch_dict)
        x = self.front_end(batch_dict)
        feat = self.backbone.forward_nhwc(x, record_len_i32(batch_dict["record_len"], x.device))      # (B, H', W', num_bev_features)
        a = self.anchor_number
        maps = rt.nchw_view(ops.linear(feat, self._head_plan())).float()                               # (B, 8A, H', W'): A class maps, then 7A deltas
        return {"psm": maps[:, :a].contiguous(), "rm": maps[:, a:].contiguous(), "spatial_features_2d": rt.nchw_view(feat).float()}
