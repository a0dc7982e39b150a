"""BevPreprocessor — OpenCOOD's data_utils/pre_processor/bev_preprocessor.py on the device: raw points -> PIXOR's `bev_input`, a
binary height-slice occupancy volume plus one mean-intensity channel, for every agent in one operator call (ops.bev_points,
csrc/bev_points.hip) without a host synchronisation.  The reference is a Python loop over the points of one cloud.

preprocess_params: {'cav_lidar_range': [x0, y0, z0, x1, y1, z1], 'geometry_param': {L1, L2, W1, W2, H1, H2, res, input_shape
(nx, ny, C), label_shape, downsample_rate}}, optionally 'range_mask' / 'ego_mask' as on SpVoxelPreprocessor
(pcd_utils.mask_points_by_range / mask_ego_points applied first, as the dataset does).  A plain object without parameters.

Two things differ from the reference on purpose: the mean intensity does not depend on the order of the points (integer atomics
on a fixed-point sum, see ops.bev_points for its error bound), and a point whose index falls outside the map is dropped where the
reference wraps a negative index or writes a height hit into the intensity channel."""
import math

import torch

from .. import ops
from ..lib import CobevtHipError


class BevPreprocessor(object):
    def __init__(self, preprocess_params, train):
        self.params = preprocess_params
        self.train = train
        self.lidar_range = [float(v) for v in preprocess_params["cav_lidar_range"]]
        g = self.geometry_param = preprocess_params["geometry_param"]
        self.range_mask = bool(preprocess_params.get("range_mask", False))
        self.ego_mask = bool(preprocess_params.get("ego_mask", False))
        missing = [k for k in ("L1", "L2", "W1", "W2", "H1", "H2", "res", "input_shape") if k not in g]
        if missing:
            raise CobevtHipError("BevPreprocessor: geometry_param lacks %s" % ", ".join(missing))
        self.res = float(g["res"])
        shape = tuple(int(v) for v in g["input_shape"])
        if len(shape) != 3 or not self.res > 0.0:
            raise CobevtHipError("BevPreprocessor: input_shape = (nx, ny, C) and res > 0, got %r and %r" % (g["input_shape"], g["res"]))
        # the occupancy slices cover [H1, H2) and the last channel is the intensity
        want = tuple(int(math.floor((float(g[hi]) - float(g[lo])) / self.res + 0.5)) for lo, hi in (("L1", "L2"), ("W1", "W2"), ("H1", "H2")))
        want = (want[0], want[1], want[2] + 1)
        if shape != want or min(shape) < 1 or shape[2] < 2:
            raise CobevtHipError("BevPreprocessor: input_shape %r disagrees with the ranges and res: (L2 - L1, W2 - W1, H2 - H1) / res "
                                 "plus the intensity channel gives %r" % (list(shape), list(want)))
        self.input_shape = shape
        self.origin = (float(g["L1"]), float(g["W1"]), float(g["H1"]))

    def preprocess_batch(self, points, point_offsets, out=None, channels_last=False):
        """points (M, 4) fp32 [x, y, z, intensity], the agents' clouds concatenated; point_offsets (N + 1,) int32 / int64 on the device
        -> {'bev_input': (N, C, nx, ny) fp32} (ops.bev_points); channels_last: (N, nx, ny, C).  ops.prepare_points makes such a cloud
        from per-agent sensor-frame clouds and their matrices."""
        bev = ops.bev_points(points, point_offsets, self.lidar_range, self.origin, self.res, self.input_shape, self.range_mask,
                             self.ego_mask, channels_last=channels_last, out=out)
        return {"bev_input": bev}

    def preprocess(self, pcd_raw):
        """one cloud (M, 4) fp32 on the device -> {'bev_input': (C, nx, ny)}, the reference's per-sample signature"""
        ops._need_cuda(pcd_raw)
        offsets = torch.tensor([0, pcd_raw.shape[0]], dtype=torch.int32, device=pcd_raw.device)
        return {"bev_input": self.preprocess_batch(pcd_raw, offsets)["bev_input"][0]}

    @staticmethod
    def _stack(items):
        items = [torch.as_tensor(x) for x in items]
        ops._need_cuda(*items)
        return {"bev_input": torch.stack(items)}

    def collate_batch(self, batch):
        """a list of {'bev_input': (C, nx, ny)} or a dict {'bev_input': [(C, nx, ny), ...]} of device tensors -> {'bev_input':
        (B, C, nx, ny)}"""
        if isinstance(batch, list):
            return self._stack([x["bev_input"] for x in batch])
        if isinstance(batch, dict):
            return self._stack(batch["bev_input"])
        raise CobevtHipError("BevPreprocessor: collate_batch takes a list or a dict, got %s" % type(batch).__name__)
