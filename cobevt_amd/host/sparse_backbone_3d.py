"""VoxelBackBone8x - the sparse 3-D backbone of OpenCOOD's SECOND-style LiDAR models (opencood/models/sub_modules/sparse_backbone_3d.py):
twelve spconv layers, each followed by BatchNorm1d(eps 1e-3) + ReLU, over the active voxels only.

    conv_input  SubMConv3d(C <= 8 -> 16)                                      sparse shape (nz + 1, ny, nx)
    conv1       SubMConv3d(16 -> 16)
    conv2       SparseConv3d(16 -> 32, 3, stride 2, pad 1)       + 2 x SubMConv3d(32 -> 32)
    conv3       SparseConv3d(32 -> 64, 3, stride 2, pad 1)       + 2 x SubMConv3d(64 -> 64)
    conv4       SparseConv3d(64 -> 64, 3, stride 2, pad (0, 1, 1)) + 2 x SubMConv3d(64 -> 64)
    conv_out    SparseConv3d(64 -> 128, (3, 1, 1), stride (2, 1, 1), pad 0)

spconv is not a dependency: SubMConv3d / SparseConv3d below are parameter containers with spconv 2.x's weight layout
(Cout, kz, ky, kx, Cin), and the nn.Sequentials sit at the reference's indices, so the state_dict has the keys and shapes a
spconv.SparseSequential gives (conv_input.0.weight, conv_input.1.running_mean, conv2.0.0.weight, ..., conv_out.1.bias).  Every layer
is ONE cobevt_sparse_conv launch (ops.sparse_conv3d) with the BatchNorm folded into its weights; the five active sets are built on the
device (ops.sparse_index, ops.sparse_downsample).  What is assumed about spconv - read from its documentation, not executed here - is
in DESIGN.md: the weight layout, the cross-correlation orientation, SubMConv3d's output set = input set, SparseConv3d's output set =
every cell with an active input in its receptive field.

forward(batch_dict) is the reference's contract: reads 'voxel_features' (P, C) (MeanVFE's output; anything else is cast and padded
to the kernel's row first), 'voxel_coords' (P, 4) [b, z, y, x] and 'batch_size'; writes 'encoded_spconv_tensor' (ops.SparseConvTensor:
features, indices, num, spatial_shape, batch_size, dense()), 'encoded_spconv_tensor_stride' = 8, 'multi_scale_3d_features' and
'multi_scale_3d_strides'.  Rows of voxel_coords with b < 0 are padding.  Row buffers have fixed capacities - by default the provable
bound min(cells of the level, 8 x the previous level's capacity) (2 x for conv_out), P for the input level - so nothing can be dropped
and nothing is read back: no host synchronisation, the forward can be captured in a HIP graph and replayed on clouds of any size up to
P rows.  `level_capacities` (five ints: the input level, conv2, conv3, conv4, conv_out; None entries keep the default) trades memory
for the risk of dropping rows, which num[1] of each tensor counts.  This forward is the inference path: in train() mode it raises, and
the module trains through host.training.voxel_backbone8x (batch statistics over the live rows, dgrad and wgrad on fp32 rows: DESIGN.md 3v)."""
import math

import torch
import torch.nn as nn

from .. import ops
from ..lib import CobevtHipError
from . import runtime as rt
from .runtime import HipModule


class _SparseConv(nn.Module):
    """parameter container in spconv 2.x's layout: weight (Cout, kz, ky, kx, Cin), no bias"""
    subm = False

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=False, indice_key=None):
        super().__init__()
        if bias:
            raise CobevtHipError("%s: bias=True is not supported (the reference's layers have none)" % type(self).__name__)
        self.in_channels, self.out_channels, self.indice_key = in_channels, out_channels, indice_key
        self.kernel_size, self.stride, self.padding = ops._triple(kernel_size), ops._triple(stride), ops._triple(padding)
        self.weight = nn.Parameter(torch.empty((out_channels,) + self.kernel_size + (in_channels,)))
        bound = 1.0 / math.sqrt(in_channels * self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2])
        nn.init.uniform_(self.weight, -bound, bound)


class SubMConv3d(_SparseConv):
    subm = True


class SparseConv3d(_SparseConv):
    pass


def post_act_block(in_channels, out_channels, kernel_size, indice_key=None, stride=1, padding=0, conv_type="subm", norm_fn=None):
    if conv_type == "subm":
        conv = SubMConv3d(in_channels, out_channels, kernel_size, padding=padding, bias=False, indice_key=indice_key)
    elif conv_type == "spconv":
        conv = SparseConv3d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=False, indice_key=indice_key)
    else:
        raise NotImplementedError(conv_type)
    return nn.Sequential(conv, norm_fn(out_channels), nn.ReLU())


def _bn(c):
    return nn.BatchNorm1d(c, eps=1e-3, momentum=0.01)


class VoxelBackBone8x(HipModule):
    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        nx, ny, nz = (int(v) for v in grid_size)
        self.sparse_shape = [nz + 1, ny, nx]                   # grid_size[::-1] + [1, 0, 0]
        if not 1 <= input_channels <= 8:
            raise CobevtHipError("VoxelBackBone8x: 1 .. 8 input channels are supported, got %d" % input_channels)
        self.conv_input = nn.Sequential(SubMConv3d(input_channels, 16, 3, padding=1, bias=False, indice_key="subm1"), _bn(16), nn.ReLU())
        block = post_act_block
        self.conv1 = nn.Sequential(block(16, 16, 3, norm_fn=_bn, padding=1, indice_key="subm1"))
        self.conv2 = nn.Sequential(block(16, 32, 3, norm_fn=_bn, stride=2, padding=1, indice_key="spconv2", conv_type="spconv"),
                                   block(32, 32, 3, norm_fn=_bn, padding=1, indice_key="subm2"),
                                   block(32, 32, 3, norm_fn=_bn, padding=1, indice_key="subm2"))
        self.conv3 = nn.Sequential(block(32, 64, 3, norm_fn=_bn, stride=2, padding=1, indice_key="spconv3", conv_type="spconv"),
                                   block(64, 64, 3, norm_fn=_bn, padding=1, indice_key="subm3"),
                                   block(64, 64, 3, norm_fn=_bn, padding=1, indice_key="subm3"))
        self.conv4 = nn.Sequential(block(64, 64, 3, norm_fn=_bn, stride=2, padding=(0, 1, 1), indice_key="spconv4", conv_type="spconv"),
                                   block(64, 64, 3, norm_fn=_bn, padding=1, indice_key="subm4"),
                                   block(64, 64, 3, norm_fn=_bn, padding=1, indice_key="subm4"))
        self.conv_out = nn.Sequential(SparseConv3d(64, 128, (3, 1, 1), stride=(2, 1, 1), padding=0, bias=False, indice_key="spconv_down2"),
                                      _bn(128), nn.ReLU())
        self.num_point_features = 128
        self.backbone_channels = {"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 64}
        self.level_capacities = model_cfg.get("level_capacities") if hasattr(model_cfg, "get") else None
        shapes = self.level_shapes()
        if min(min(s) for s in shapes) < 1:
            raise CobevtHipError("VoxelBackBone8x: grid (%d, %d, %d) is too shallow: the sparse shapes of the five levels would be %s"
                                 % (nx, ny, nz, ", ".join(str(s) for s in shapes)))

    def _layers(self):
        """the twelve (name, conv, bn) in forward order"""
        out = [("conv_input", self.conv_input[0], self.conv_input[1])]
        for name in ("conv1", "conv2", "conv3", "conv4"):
            out += [("%s.%d" % (name, i), blk[0], blk[1]) for i, blk in enumerate(getattr(self, name))]
        return out + [("conv_out", self.conv_out[0], self.conv_out[1])]

    def level_shapes(self):
        """the sparse shapes (D, H, W) of the input level, conv2, conv3, conv4 and conv_out"""
        shapes = [tuple(self.sparse_shape)]
        for _, conv, _ in self._layers():
            if not conv.subm:
                shapes.append(ops.sparse_out_shape(shapes[-1], conv.kernel_size, conv.stride, conv.padding))
        return shapes

    def _conv_plan(self, name, conv, bn):
        def build(dt, dev):
            return ops.SparseConvPlan(conv.weight, bn, conv.stride, conv.padding, conv.subm, dt, dev)
        return self._plan(name, rt.module_tensors(conv, bn), build)

    @staticmethod
    def _input_rows(vf, dt):
        """(P, C) -> contiguous (P, row) in the compute dtype, zeros behind the C channels; MeanVFE's output already is the [:, :C] view of one"""
        p, c = vf.shape
        row = ops.sparse_row_channels(c, dt)
        base = vf._base
        if vf.dtype == dt and base is not None and tuple(base.shape) == (p, row) and base.is_contiguous() and base.data_ptr() == vf.data_ptr() \
                and vf.stride() == (row, 1):
            return base
        rows = torch.zeros((p, row), device=vf.device, dtype=dt)
        rows[:, :c] = vf
        return rows

    def forward(self, batch_dict):
        vf, coords = batch_dict["voxel_features"], batch_dict["voxel_coords"]
        self._require_inference(vf, coords)
        layers = self._layers()
        if vf.dim() != 2 or vf.shape[1] != layers[0][1].in_channels or coords.shape[0] != vf.shape[0]:
            raise CobevtHipError("VoxelBackBone8x: voxel_features must be (P, %d) with one row per row of voxel_coords, got %s / %s"
                                 % (layers[0][1].in_channels, tuple(vf.shape), tuple(coords.shape)))
        caps = list(self.level_capacities or [None] * 5)
        if len(caps) != 5:
            raise CobevtHipError("VoxelBackBone8x: level_capacities has five entries (the input level, conv2, conv3, conv4, conv_out), got %r" % (caps,))
        dt = rt.get_compute_dtype()
        x = ops.sparse_index(coords, batch_dict["batch_size"], self.sparse_shape, features=self._input_rows(vf, dt), capacity=caps[0])
        level, feats = 0, {}
        for name, conv, bn in layers:
            if not conv.subm:
                level += 1
            x = ops.sparse_conv3d(x, self._conv_plan(name, conv, bn), capacity=None if conv.subm else caps[level])
            feats[name] = x
        batch_dict.update({"encoded_spconv_tensor": x, "encoded_spconv_tensor_stride": 8})
        batch_dict.update({"multi_scale_3d_features": {"x_conv1": feats["conv1.0"], "x_conv2": feats["conv2.2"], "x_conv3": feats["conv3.2"],
                                                       "x_conv4": feats["conv4.2"]}})
        batch_dict.update({"multi_scale_3d_strides": {"x_conv1": 1, "x_conv2": 2, "x_conv3": 4, "x_conv4": 8}})
        return batch_dict
