"""PFNLayer / PillarVFE — mirror of opv2v/opencood/models/sub_modules/pillar_vfe.py (:10-53, :56-146): constructor arguments,
attributes and state_dict keys (`pfn_layers.0.linear.weight`, `pfn_layers.0.norm.*`), `get_output_feature_dim`, and
forward(batch_dict) -> batch_dict['pillar_features'].

The HIP operator (csrc/pillar_vfe.hip) implements ONE PFN layer of 64 output channels on pillars of at most 32 points with 4 point
features; every other configuration raises CobevtHipError at construction.  The eval-mode BatchNorm1d (eps as stored) is folded into
the bias-free Linear when the plan is built: W (K, 64), shift (64), both fp32 - the operator's arithmetic is fp32 in every compute
mode, only its store converts.  In train() mode the forward runs host/training.pillar_vfe: BatchNorm1d on batch statistics (or, after
norm.eval(), the frozen running ones) with HIP kernels in both directions (csrc/train_pillar.hip), parameter gradients only."""
import torch
import torch.nn as nn

from .. import ops
from ..lib import CobevtHipError
from . import runtime as rt
from . import training
from .runtime import HipModule


class PFNLayer(HipModule):
    """pillar_vfe.py:10-53.  Parameter container of the fused operator: Linear (+ BatchNorm1d) -> ReLU -> max over the points."""

    def __init__(self, in_channels, out_channels, use_norm=True, last_layer=False):
        super().__init__()
        self.last_vfe = last_layer
        self.use_norm = use_norm
        if not self.last_vfe:
            raise CobevtHipError("PFNLayer: only the last layer of a PFN stack has a HIP kernel (limit: one PFN layer, "
                                 "last_layer=True); a layer that concatenates its maximum back onto the points is not supported")
        if out_channels != ops.PILLAR_CHANNELS:
            raise CobevtHipError("PFNLayer: the HIP kernel has %d output channels (limit), got %d" % (ops.PILLAR_CHANNELS, out_channels))
        if self.use_norm:
            self.linear = nn.Linear(in_channels, out_channels, bias=False)
            self.norm = nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01)
        else:
            self.linear = nn.Linear(in_channels, out_channels, bias=True)
        self.part = 50000

    def folded(self):
        """(W (K, 64), shift (64)) fp32 on the parameters' device: y = relu(f @ W + shift)"""
        def build(dt, dev):
            w = self.linear.weight.detach().double()                                   # (64, K)
            if self.use_norm:
                scale, shift = ops.bn_affine(self.norm)
                w = w * scale[:, None]
            else:
                shift = self.linear.bias.detach().double()
            return (w.t().to(device=dev, dtype=torch.float32).contiguous(), shift.to(device=dev, dtype=torch.float32).contiguous())
        return self._plan("folded", rt.module_tensors(self), build)

    def forward(self, inputs):
        self._require_inference(inputs)
        raise CobevtHipError("PFNLayer has no stand-alone HIP forward: the layer runs fused with the point decoration inside "
                             "PillarVFE.forward / PointPillarFuseBEVT.forward (csrc/pillar_vfe.hip)")


class PillarVFE(HipModule):
    """pillar_vfe.py:56-146.  model_cfg: use_norm, with_distance, use_absolute_xyz, num_filters (and, optionally,
    max_points_per_voxel: checked against the kernel's limit of 32 at construction)."""

    def __init__(self, model_cfg, num_point_features, voxel_size, point_cloud_range):
        super().__init__()
        self.model_cfg = model_cfg
        self.use_norm = self.model_cfg["use_norm"]
        self.with_distance = self.model_cfg["with_distance"]
        self.use_absolute_xyz = self.model_cfg["use_absolute_xyz"]
        if num_point_features != 4:
            raise CobevtHipError("PillarVFE: the HIP kernel reads F = 4 point features (x, y, z, intensity: one 16-byte load per "
                                 "point), got num_point_features = %r" % (num_point_features,))
        num_point_features += 6 if self.use_absolute_xyz else 3
        if self.with_distance:
            num_point_features += 1
        self.num_filters = self.model_cfg["num_filters"]
        assert len(self.num_filters) > 0
        if len(self.num_filters) != 1:
            raise CobevtHipError("PillarVFE: the HIP kernel implements one PFN layer (limit), got num_filters = %r"
                                 % (list(self.num_filters),))
        t = self.model_cfg.get("max_points_per_voxel") if hasattr(self.model_cfg, "get") else None
        if t is not None and t > ops.PILLAR_MAX_POINTS:
            raise CobevtHipError("PillarVFE: at most T = %d points per pillar (limit: a pillar sits on one half-wave), got "
                                 "max_points_per_voxel = %d" % (ops.PILLAR_MAX_POINTS, t))
        num_filters = [num_point_features] + list(self.num_filters)
        pfn_layers = []
        for i in range(len(num_filters) - 1):
            pfn_layers.append(PFNLayer(num_filters[i], num_filters[i + 1], self.use_norm, last_layer=(i >= len(num_filters) - 2)))
        self.pfn_layers = nn.ModuleList(pfn_layers)
        self.voxel_x = voxel_size[0]
        self.voxel_y = voxel_size[1]
        self.voxel_z = voxel_size[2]
        self.x_offset = self.voxel_x / 2 + point_cloud_range[0]
        self.y_offset = self.voxel_y / 2 + point_cloud_range[1]
        self.z_offset = self.voxel_z / 2 + point_cloud_range[2]

    def get_output_feature_dim(self):
        return self.num_filters[-1]

    def geom(self):
        return (self.voxel_x, self.voxel_y, self.voxel_z, self.x_offset, self.y_offset, self.z_offset)

    def forward(self, batch_dict):
        """batch_dict: voxel_features (P, T, 4) fp32, voxel_num_points (P,), voxel_coords (P, 4) [n, z, y, x] ->
        batch_dict['pillar_features'] (P, 64), always two-dimensional (the reference's squeeze() collapses P = 1).  train(): fp32,
        differentiable in the layer's parameters (not in the points)"""
        if self.training and training.lidar_trains(self.pfn_layers[0], batch_dict["voxel_features"]):
            return training.pillar_vfe(self, batch_dict)
        vf, npts, coords = batch_dict["voxel_features"], batch_dict["voxel_num_points"], batch_dict["voxel_coords"]
        self._require_inference(vf, npts, coords)
        w, shift = self.pfn_layers[0].folded()
        rows = ops.pillar_vfe_rows(vf, npts, coords, w, shift, self.geom(), rt.get_compute_dtype(),
                                   use_absolute_xyz=self.use_absolute_xyz, with_distance=self.with_distance)
        batch_dict["pillar_features"] = rt.like_input(rows, vf)
        return batch_dict
