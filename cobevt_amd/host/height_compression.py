"""HeightCompression (opencood/models/sub_modules/height_compression.py): the sparse output of VoxelBackBone8x as a BEV map,
dense() (N, C, D, H, W) viewed as (N, C D, H, W) - channel c D + d.  ops.sparse_dense writes that map in one launch into a zero-filled
channels-last buffer, so the view costs nothing and host.BaseBEVBackbone.forward reads it without a copy.

forward(batch_dict) is the reference's contract: reads 'encoded_spconv_tensor' and 'encoded_spconv_tensor_stride', writes
'spatial_features' (N, C D, H, W), in the compute dtype, and 'spatial_features_stride'.  No parameters, no host synchronisation.
In train() mode the forward raises; host.training.height_compression is the differentiable form (autograd.SparseDenseFn)."""
from .runtime import HipModule


class HeightCompression(HipModule):
    def __init__(self, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = self.model_cfg["feature_num"]

    def forward(self, batch_dict):
        x = batch_dict["encoded_spconv_tensor"]
        self._require_inference(x.features)
        spatial_features = x.dense()
        n, c, d, h, w = spatial_features.shape
        batch_dict["spatial_features"] = spatial_features.view(n, c * d, h, w)
        batch_dict["spatial_features_stride"] = batch_dict["encoded_spconv_tensor_stride"]
        return batch_dict
