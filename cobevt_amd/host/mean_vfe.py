"""MeanVFE - the voxel feature encoder of OpenCOOD's SECOND-style models (opencood/models/sub_modules/mean_vfe.py): the mean of a
voxel's points, one cobevt_mean_vfe launch (ops.mean_vfe).  No parameters.

forward(batch_dict) is the reference's contract: reads 'voxel_features' (P, T, C) fp32 and 'voxel_num_points' (P,), writes
'voxel_features' (P, C).  Two things differ from the reference's tensor, neither in value: it is in the compute dtype, and it is the
[:, :C] view of a (P, row) buffer whose rows are whole 32-byte groups with zeros behind the C channels - the row
VoxelBackBone8x's first convolution reads, so nothing is copied between the two.  The reference sums all T slots; this sums the first
voxel_num_points of them, the same whenever the unused slots are zero, which spconv's voxel generator guarantees.  Rows with a
negative batch index in 'voxel_coords' (the padding rows of a fixed-size voxel dict, SpVoxelPreprocessor's convention) give zeros.
In train() mode the forward raises; host.training.mean_vfe is the same launch with fp32 rows (no parameters, no graph)."""
from .. import ops
from . import runtime as rt
from .runtime import HipModule


class MeanVFE(HipModule):
    def __init__(self, model_cfg, num_point_features, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_point_features = num_point_features

    def get_output_feature_dim(self):
        return self.num_point_features

    def forward(self, batch_dict, **kwargs):
        vf, npts = batch_dict["voxel_features"], batch_dict["voxel_num_points"]
        self._require_inference(vf, npts)
        dt = rt.get_compute_dtype()
        c = vf.shape[2]
        rows = ops.mean_vfe(vf, npts, batch_dict.get("voxel_coords"), dtype=dt, channels=ops.sparse_row_channels(c, dt))
        batch_dict["voxel_features"] = rows[:, :c]
        return batch_dict
