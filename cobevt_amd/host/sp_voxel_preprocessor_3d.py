"""SpVoxelPreprocessor3D — SpVoxelPreprocessor on a grid with any nz >= 1: spconv's VoxelGenerator.generate per agent, collated
agent-major with the agent index in front of the (z, y, x) coordinates, on the device: raw points -> the voxel dict MeanVFE and
VoxelBackBone8x read, in one operator call (ops.voxelize_points_3d, csrc/voxelize.hip) without a host synchronisation.

preprocess_params and `train` as SpVoxelPreprocessor: {'args': {voxel_size [x, y, z], max_points_per_voxel, max_voxel_train,
max_voxel_test}, 'cav_lidar_range': [x0, y0, z0, x1, y1, z1]}, optionally 'range_mask' / 'ego_mask'.  A plain object without
parameters.  The dict has a fixed capacity of N * max_voxels rows: agent a's voxels start at row a * max_voxels, rows without a voxel
carry voxel_coords [-1, 0, 0, 0] / voxel_num_points 0 (MeanVFE and the backbone skip them) and their voxel_features are NOT written.
'batch_size' = N is in the dict, so vfe(batch) and backbone(batch) take it as it is; grid_size (nx, ny, nz) is VoxelBackBone8x's."""
from .. import ops
from ..lib import CobevtHipError


class SpVoxelPreprocessor3D(object):
    def __init__(self, preprocess_params, train):
        self.params = preprocess_params
        self.train = train
        args = preprocess_params["args"]
        self.lidar_range = [float(v) for v in preprocess_params["cav_lidar_range"]]
        self.voxel_size = [float(v) for v in args["voxel_size"]]
        self.max_points_per_voxel = int(args["max_points_per_voxel"])
        self.max_voxels = int(args["max_voxel_train"] if train else args["max_voxel_test"])
        self.range_mask = bool(preprocess_params.get("range_mask", False))
        self.ego_mask = bool(preprocess_params.get("ego_mask", False))
        self.grid_size = ops.voxel_grid_size(self.lidar_range, self.voxel_size)          # (nx, ny, nz)
        if min(self.grid_size) < 1 or self.max_voxels < 1:
            raise CobevtHipError("SpVoxelPreprocessor3D: empty grid %r or voxel cap %d" % (list(self.grid_size), self.max_voxels))
        if self.max_points_per_voxel < 1 or self.max_points_per_voxel > ops.PILLAR_MAX_POINTS:
            raise CobevtHipError("SpVoxelPreprocessor3D: 1 <= max_points_per_voxel <= T = %d is supported, got %d"
                                 % (ops.PILLAR_MAX_POINTS, self.max_points_per_voxel))

    def preprocess_batch(self, points, point_offsets, out=None):
        """points (M, 4) fp32 [x, y, z, intensity], the agents' clouds concatenated in the ego frame; point_offsets (N + 1,) int32 /
        int64 on the device -> {'voxel_features', 'voxel_coords', 'voxel_num_points', 'num_voxels', 'batch_size'}
        (ops.voxelize_points_3d).  ops.prepare_points makes such a cloud from per-agent sensor-frame clouds and their matrices."""
        vf, coords, npts, nvox = ops.voxelize_points_3d(points, point_offsets, self.lidar_range, self.voxel_size, self.max_points_per_voxel,
                                                        self.max_voxels, self.range_mask, self.ego_mask, out=out)
        return {"voxel_features": vf, "voxel_coords": coords, "voxel_num_points": npts, "num_voxels": nvox, "batch_size": nvox.shape[0]}
