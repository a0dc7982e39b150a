"""PointPillarScatter — mirror of opv2v/opencood/models/sub_modules/point_pillar_scatter.py:5-47: pillar rows -> the BEV pseudo-image,
cell z + y * nx + x of agent n (y is the row).  The map is channels-last on the device; `spatial_features` is its NCHW view."""
from .. import ops
from ..lib import CobevtHipError
from . import runtime as rt
from . import training
from .runtime import HipModule


class PointPillarScatter(HipModule):
    def __init__(self, model_cfg):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = self.model_cfg["num_features"]
        self.nx, self.ny, self.nz = model_cfg["grid_size"]
        if self.nz != 1:
            raise CobevtHipError("PointPillarScatter: pillars span the whole height - nz = 1 is the limit (the reference asserts it), "
                                 "got grid_size = %r" % (list(model_cfg["grid_size"]),))

    def forward(self, batch_dict):
        """batch_dict: pillar_features (P, C), voxel_coords (P, 4) [n, z, y, x] -> batch_dict['spatial_features'] (N, C, ny, nx), an
        NCHW view of a channels-last tensor in the caller's dtype.  N is batch_dict['batch_size'] when present (a host integer: no
        synchronisation); otherwise it is derived as the reference derives it, `coords[:, 0].max() + 1` - the ONE synchronising
        path of the LiDAR front end.  Every cell without a pillar is exactly 0; rows with n outside [0, N) or y / x outside the
        grid are skipped.  train(): the same map in fp32, differentiable in pillar_features (the backward gathers each row's cell)."""
        if self.training and training.lidar_trains(None, batch_dict["pillar_features"].detach()):
            return training.point_pillar_scatter(self, batch_dict)
        rows, coords = batch_dict["pillar_features"], batch_dict["voxel_coords"]
        self._require_inference(rows, coords)
        if rows.dim() != 2 or rows.shape[1] != self.num_bev_features:
            raise CobevtHipError("PointPillarScatter: pillar_features must be (P, %d), got %s" % (self.num_bev_features, tuple(rows.shape)))
        if "batch_size" in batch_dict:
            batch_size = int(batch_dict["batch_size"])
        else:
            batch_size = int(coords[:, 0].max().int().item()) + 1          # point_pillar_scatter.py:18 (host synchronisation)
        canvas = ops.scatter_rows(rt.as_compute(rows), coords, batch_size, (self.ny, self.nx))
        batch_dict["spatial_features"] = rt.like_input(rt.nchw_view(canvas), rows)
        return batch_dict
