"""The sparse 3-D backbone (host.MeanVFE, host.VoxelBackBone8x, host.HeightCompression; csrc/sparse_conv.hip) without a device: the
dense restatement tests/sparse_ref.py is pinned against a brute-force per-voxel, per-tap loop (so that the mask-convolution
construction is not its own witness), the shape chain, the case generator, the state_dict, the lowered weights, the workspace size,
the refusals (CPU tensors, train(), the C ABI's argument validation before any launch) and the launch traces."""
import ctypes

import numpy as np
import pytest
import torch

import launch_trace as lt
import launch_trace_sparse_backbone as lts
import sparse_ref as sr
from cobevt_amd import host, lib, ops, synth
from cobevt_amd.lib import CobevtHipError


# ---------------------------------------------------------------------------------------------- the restatement against brute force
@pytest.mark.parametrize("kernel,stride,padding,subm", [((3, 3, 3), (1, 1, 1), (1, 1, 1), True), ((3, 3, 3), (2, 2, 2), (1, 1, 1), False),
                                                        ((3, 3, 3), (2, 2, 2), (0, 1, 1), False), ((3, 1, 1), (2, 1, 1), (0, 0, 0), False)])
def test_restatement_is_the_per_voxel_per_tap_loop(kernel, stride, padding, subm):
    rng = np.random.RandomState(7)
    batch, shape, cin, cout = 2, (7, 6, 9), 3, 5
    cells = np.stack(np.unravel_index(rng.permutation(batch * 7 * 6 * 9)[:60], (batch,) + shape), axis=1)
    feats = rng.uniform(-1, 1, (60, cin))
    w5 = torch.from_numpy(rng.uniform(-1, 1, (cout,) + kernel + (cin,)))
    scale, shift = torch.from_numpy(rng.uniform(0.5, 1.5, cout)), torch.from_numpy(rng.uniform(-0.3, 0.3, cout))
    x, mask = sr.to_dense(cells, feats, batch, shape)
    y, m = sr.layer(x, mask, w5, scale, shift, kernel, stride, padding, subm)
    brute = sr.brute_layer(cells, feats, batch, shape, w5, scale, shift, kernel, stride, padding, subm)
    idx, rows = sr.rows_of(y, m)
    assert [tuple(int(v) for v in r) for r in idx] == sorted(brute)                  # the same active set, in cell order
    assert 0 < len(brute) < m.numel()
    want = torch.stack([brute[k] for k in sorted(brute)])
    assert float((rows - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))
    assert float((y * (~m).double()).abs().max()) == 0.0
    # an active cell whose convolution is zero still carries relu(shift): the mask is not redundant
    assert (want > 0).any() and (want == 0).any()


def test_duplicates_padding_and_out_of_range_rows_in_the_restatement():
    coords = np.array([[0, 1, 1, 1], [0, 1, 1, 1], [-1, 0, 0, 0], [0, 9, 0, 0], [1, 0, 0, 2]])
    x, mask = sr.to_dense(coords, np.arange(5, dtype=np.float64)[:, None] + 1, 2, (3, 3, 3))
    assert int(mask.sum()) == 2 and float(x[0, 0, 1, 1, 1]) == 1.0 and float(x[1, 0, 0, 0, 2]) == 5.0


# ---------------------------------------------------------------------------------------------- shapes and cases
CHAINS = {(48, 32, 40): [(41, 32, 48), (21, 16, 24), (11, 8, 12), (5, 4, 6), (2, 4, 6)],
          (45, 31, 24): [(25, 31, 45), (13, 16, 23), (7, 8, 12), (3, 4, 6), (1, 4, 6)],
          (21, 13, 40): [(41, 13, 21), (21, 7, 11), (11, 4, 6), (5, 2, 3), (2, 2, 3)]}


@pytest.mark.parametrize("grid", sr.GRIDS)
def test_shape_chain(grid):
    m = host.VoxelBackBone8x({}, 4, list(grid))
    assert m.sparse_shape == [grid[2] + 1, grid[1], grid[0]]
    assert m.level_shapes() == CHAINS[grid] == sr.shape_chain(grid)
    assert m.num_point_features == 128 and m.backbone_channels == {"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 64}
    assert host.VoxelBackBone8x({}, 4, np.array(grid)).sparse_shape == m.sparse_shape        # the reference passes an array


def test_a_grid_that_is_too_shallow_raises_at_construction():
    host.VoxelBackBone8x({}, 4, [8, 8, 24])                  # nz = 24 is the smallest grid for which conv_out has an output
    with pytest.raises(CobevtHipError, match="too shallow"):
        host.VoxelBackBone8x({}, 4, [8, 8, 23])
    with pytest.raises(CobevtHipError, match="too shallow"):
        host.VoxelBackBone8x({}, 4, [48, 32, 8])
    with pytest.raises(CobevtHipError, match="input channels"):
        host.VoxelBackBone8x({}, 9, [48, 32, 40])


@pytest.mark.parametrize("grid", sr.GRIDS)
def test_case_generator_leaves_every_level_partly_active(grid):
    coords = sr.clustered_coords(grid, 2, sr.SEEDS[grid])
    assert len(np.unique(coords, axis=0)) == len(coords) and coords.dtype == np.int32
    sd = synth.fill_module_(host.VoxelBackBone8x({}, 4, list(grid)), 0).state_dict()
    levels, out = sr.backbone(sd, coords, sr.features_for(coords, 4), 2, grid, "f64")
    sr.assert_case_is_sparse_everywhere(levels)
    assert list(levels) == [name for name, _, _ in host.VoxelBackBone8x({}, 4, list(grid))._layers()] and len(levels) == 12
    d, h, w = CHAINS[grid][-1]
    assert tuple(out.shape) == (2, 128 * d, h, w) and float(out.max()) > 0.1



@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", sorted(sr.KERNEL_CASES))
def test_kernel_cases_exercise_the_relu_and_the_active_set(name, dtype):
    """what the GPU test asserts about its float64 reference, checked where the reference is computed: the ReLU cuts between 5 % and
    95 % of the outputs, max|ref| > 0.1, the tile-edge cases have the row counts they are named for and unique cells"""
    c = sr.kernel_case(name)
    plan = ops.SparseConvPlan(c["weight"], sr.bn_module(c["bn"]), c["stride"], c["padding"], c["subm"], dtype, "cpu")
    idx, ref, s, k = sr.kernel_reference(c["feats"].to(dtype), c["coords"], sr.KERNEL_BATCH, sr.KERNEL_SHAPE, plan.wgt, plan.shift, c["cin"],
                                         c["cout"], c["kernel"], c["stride"], c["padding"], c["subm"])
    assert len(torch.unique(c["coords"], dim=0)) == len(c["coords"]) and tuple(ref.shape) == (len(idx), c["cout"]) == tuple(s.shape)
    assert float(ref.abs().max()) > 0.1 and 0.05 < float((ref == 0).double().mean()) < 0.95
    assert float(k.min()) >= c["cin"] and float(k.max()) <= c["cin"] * plan.taps and float(s.min()) >= 0
    rows = {"rows_1": 1, "rows_tile_minus_1": sr.TILE - 1, "rows_tile_plus_1": sr.TILE + 1, "rows_block_plus_1": 4 * sr.TILE + 1,
            "two_samples_one_tile": 24}
    if name in rows:
        assert len(idx) == rows[name] and ops.SPARSE_TILE_ROWS == sr.TILE and ops.SPARSE_BLOCK_ROWS == 4 * sr.TILE
        assert float(k.max()) <= 3 * c["cin"] * (4 if name == "rows_block_plus_1" else 1)          # most taps are absent for every row
    if name == "two_samples_one_tile":
        assert sorted(set(int(b) for b in idx[:, 0])) == [0, 1]
    if not c["subm"]:
        assert len(idx) != len(c["coords"])


# ---------------------------------------------------------------------------------------------- state_dict, plans
def test_state_dict_keys_and_shapes():
    sd = host.VoxelBackBone8x({}, 4, [48, 32, 40]).state_dict()
    convs = {"conv_input.0": (16, 3, 3, 3, 4), "conv1.0.0": (16, 3, 3, 3, 16), "conv2.0.0": (32, 3, 3, 3, 16), "conv2.1.0": (32, 3, 3, 3, 32),
             "conv2.2.0": (32, 3, 3, 3, 32), "conv3.0.0": (64, 3, 3, 3, 32), "conv3.1.0": (64, 3, 3, 3, 64), "conv3.2.0": (64, 3, 3, 3, 64),
             "conv4.0.0": (64, 3, 3, 3, 64), "conv4.1.0": (64, 3, 3, 3, 64), "conv4.2.0": (64, 3, 3, 3, 64), "conv_out.0": (128, 3, 1, 1, 64)}
    want = {}
    for conv, shape in convs.items():
        want[conv + ".weight"] = shape
        bn = conv[:-1] + "1"
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            want["%s.%s" % (bn, leaf)] = (shape[0],)
        want[bn + ".num_batches_tracked"] = ()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want and len(want) == 72
    assert list(sd)[:6] == ["conv_input.0.weight", "conv_input.1.weight", "conv_input.1.bias", "conv_input.1.running_mean",
                            "conv_input.1.running_var", "conv_input.1.num_batches_tracked"]
    assert host.MeanVFE({}, 4).state_dict() == {} and host.HeightCompression({"feature_num": 256}).state_dict() == {}
    assert host.MeanVFE({}, 4).get_output_feature_dim() == 4 and host.HeightCompression({"feature_num": 256}).num_bev_features == 256


@pytest.mark.parametrize("dtype,row", [(torch.float32, 8), (torch.bfloat16, 16)])
def test_plan_folds_the_batchnorm_and_orders_the_taps(dtype, row):
    m = synth.fill_module_(host.VoxelBackBone8x({}, 4, [48, 32, 40]), 0).eval()
    conv, bn = m.conv_input[0], m.conv_input[1]
    plan = ops.SparseConvPlan(conv.weight, bn, conv.stride, conv.padding, True, dtype, "cpu")
    assert tuple(plan.wgt.shape) == (27, 32, row) and plan.wgt.dtype == dtype and tuple(plan.shift.shape) == (32,)
    scale, shift = sr.bn_affine(m.state_dict(), "conv_input.1.")
    for kz, ky, kx in ((0, 0, 0), (1, 2, 0), (2, 2, 2)):
        want = (conv.weight.detach().double()[:, kz, ky, kx, :] * scale[:, None]).float().to(dtype)
        assert torch.equal(plan.wgt[(kz * 3 + ky) * 3 + kx, :16, :4], want)
    assert float(plan.wgt[:, 16:].abs().max()) == 0.0 and float(plan.wgt[:, :, 4:].abs().max()) == 0.0
    assert torch.equal(plan.shift[:16], shift.float()) and float(plan.shift[16:].abs().max()) == 0.0
    out = m.conv_out[0]
    p2 = ops.SparseConvPlan(out.weight, m.conv_out[1], out.stride, out.padding, False, dtype, "cpu")
    assert (p2.kernel, p2.stride, p2.padding, p2.taps, tuple(p2.wgt.shape)) == ((3, 1, 1), (2, 1, 1), (0, 0, 0), 3, (3, 128, 64))
    w = torch.zeros(16, 3, 3, 3, 16)
    for bad in (dict(stride=3), dict(padding=2), dict(stride=2, subm=True), dict(padding=(1, 0, 0))):
        with pytest.raises(CobevtHipError, match="supported"):
            ops.SparseConvPlan(w, None, **dict(dict(stride=1, padding=1, subm=False, dtype=dtype, device="cpu"), **bad))
    for shape in ((16, 3, 3, 3, 9), (48, 3, 3, 3, 16), (16, 5, 3, 3, 16), (16, 3, 1, 1, 16)):
        with pytest.raises(CobevtHipError, match="supported"):
            ops.SparseConvPlan(torch.zeros(shape), None, 1, 1, False, dtype, "cpu")
    with pytest.raises(CobevtHipError, match="weight must be"):
        ops.SparseConvPlan(torch.zeros(16, 16, 3, 3), None, 1, 1, True, dtype, "cpu")


# ---------------------------------------------------------------------------------------------- workspace, C ABI
def _ws_ints(n, d, h, w):
    blocks = max(1, -(-(-(-(n * d * h * w) // 32)) // 1024))
    return 2 * 1024 * blocks + blocks + 1


def test_workspace_size():
    assert ops.sparse_workspace_ints(2, (41, 32, 48)) == _ws_ints(2, 41, 32, 48) == 2 * 4096 + 4 + 1
    assert ops.sparse_workspace_ints(1, (1, 1, 1)) == 2 * 1024 + 2
    assert ops.sparse_workspace_ints(1, (41, 1600, 1408)) == _ws_ints(1, 41, 1600, 1408)        # the KITTI grid: 2 x 11.5 MB
    assert ops.sparse_out_shape((41, 1600, 1408), (3, 3, 3), (2, 2, 2), (1, 1, 1)) == (21, 800, 704)
    assert ops.sparse_row_channels(4, torch.float32) == 8 and ops.sparse_row_channels(4, torch.bfloat16) == 16
    assert ops.sparse_row_channels(64, torch.float32) == 64 and ops.sparse_row_channels(17, torch.bfloat16) == 32
    for bad in ((0, (4, 4, 4)), (1, (4, 4)), (1, (4, 0, 4))):
        with pytest.raises(CobevtHipError, match="spatial_shape"):
            ops.sparse_workspace_ints(*bad)
    with pytest.raises(CobevtHipError, match="cobevt_sparse_scratch failed"):
        ops.sparse_workspace_ints(1, (2048, 2048, 2048))                                          # a cell index past 2^31


def test_c_abi_validates_arguments_before_any_launch():
    """null pointers (COBEVT_ERR_ARG = 1), unsupported kernel / stride / pad / channels, negative counts and misaligned buffers
    (COBEVT_ERR_SHAPE = 2) are refused without touching a device"""
    l = lib.load()
    buf = (ctypes.c_float * 64)()                               # host memory: only its address is looked at
    base = (ctypes.addressof(buf) + 15) & ~15
    ptr, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    longs = lambda *v: (ctypes.c_long * len(v))(*v)             # noqa: E731
    need = ctypes.c_long(0)
    # scratch
    assert l.cobevt_sparse_scratch(None, ctypes.byref(need)) == 1 and l.cobevt_sparse_scratch(longs(1, 4, 4, 4), None) == 1
    for bad in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, -1, 4), (70000, 4, 4, 4), (1, 2 ** 11, 2 ** 10, 2 ** 10), (2, 2 ** 40, 1, 1)):
        assert l.cobevt_sparse_scratch(longs(*bad), ctypes.byref(need)) == 2, bad
    # mean_vfe: dims = [dtype, P, T, C, Cpad]
    assert l.cobevt_mean_vfe(ptr, ptr, None, ptr, None, None) == 1
    assert l.cobevt_mean_vfe(None, ptr, None, ptr, longs(1, 10, 5, 4, 8), None) == 1
    assert l.cobevt_mean_vfe(ptr, ptr, None, None, longs(1, 10, 5, 4, 8), None) == 1
    for bad in ((2, 10, 5, 4, 8), (1, -1, 5, 4, 8), (1, 10, 0, 4, 8), (1, 10, 5, 0, 8), (1, 10, 5, 9, 8), (1, 10, 5, 4, 65), (1, 2 ** 40, 5, 4, 8)):
        assert l.cobevt_mean_vfe(ptr, ptr, None, ptr, longs(*bad), None) == 2, bad
    assert l.cobevt_mean_vfe(ptr, ptr, off, ptr, longs(1, 10, 5, 4, 8), None) == 2                 # voxel_coords not 16-byte aligned
    assert l.cobevt_mean_vfe(None, None, None, None, longs(1, 0, 5, 4, 8), None) == 0              # no rows: nothing to launch
    # index: dims = [N, D, H, W, P, capacity]
    ok = (2, 41, 13, 21, 100, 100)
    assert l.cobevt_sparse_index(ptr, ptr, ptr, ptr, ptr, None, None) == 1
    for hole in range(1, 5):
        args = [ptr] * 5
        args[hole] = None
        assert l.cobevt_sparse_index(*(args + [longs(*ok), None])) == 1
    assert l.cobevt_sparse_index(None, ptr, ptr, ptr, ptr, longs(*ok), None) == 1                  # P > 0 without coordinates
    for bad in ((0, 41, 13, 21, 100, 100), (2, 41, 13, 21, -1, 100), (2, 41, 13, 21, 100, 0), (2, 41, 13, 21, 2 ** 31, 100),
                (2, 41, 13, 21, 100, 2 ** 31), (2, 2 ** 12, 2 ** 10, 2 ** 10, 100, 100)):
        assert l.cobevt_sparse_index(ptr, ptr, ptr, ptr, ptr, longs(*bad), None) == 2, bad
    for hole in range(3):
        args = [ptr] * 5
        args[hole] = off
        assert l.cobevt_sparse_index(*(args + [longs(*ok), None])) == 2
    # downsample: dims = [N, D, H, W, input capacity, output capacity, kernel, stride, pad]
    geo = (3, 3, 3, 2, 2, 2, 1, 1, 1)
    assert l.cobevt_sparse_downsample(ptr, ptr, ptr, ptr, ptr, None, None) == 1
    for hole in range(5):
        args = [ptr] * 5
        args[hole] = None
        assert l.cobevt_sparse_downsample(*(args + [longs(2, 41, 13, 21, 100, 800, *geo), None])) == 1
    for bad in ((2, 41, 13, 21, 0, 800) + geo, (2, 41, 13, 21, 100, -5) + geo, (2, 41, 13, 21, 100, 800, 5, 3, 3, 2, 2, 2, 1, 1, 1),
                (2, 41, 13, 21, 100, 800, 3, 3, 3, 3, 3, 3, 1, 1, 1), (2, 41, 13, 21, 100, 800, 3, 3, 3, 2, 2, 2, 2, 2, 2),
                (2, 41, 13, 21, 100, 800, 3, 1, 1, 2, 1, 1, 1, 1, 1), (2, 41, 13, 21, 100, 800, 3, 3, 3, 1, 2, 2, 1, 1, 1),
                (2, 2, 13, 21, 100, 800, 3, 3, 3, 2, 2, 2, 0, 0, 0)):                              # ... and a level without an output
        assert l.cobevt_sparse_downsample(ptr, ptr, ptr, ptr, ptr, longs(*bad), None) == 2, bad
    assert l.cobevt_sparse_downsample(off, ptr, ptr, ptr, ptr, longs(2, 41, 13, 21, 100, 800, *geo), None) == 2
    # conv: dims = [dtype, N, D, H, W, input rows, output capacity, input row in channels, Cout, kernel, stride, pad]
    sub = (3, 3, 3, 1, 1, 1, 1, 1, 1)
    good = (1, 2, 41, 13, 21, 100, 100, 16, 16) + sub
    assert l.cobevt_sparse_conv(ptr, ptr, ptr, None, ptr, ptr, ptr, ptr, ptr, None, None) == 1
    for hole in (0, 1, 2, 4, 5, 6, 7, 8):
        args = [ptr] * 9
        args[3] = None
        args[hole] = None
        assert l.cobevt_sparse_conv(*(args + [longs(*good), None])) == 1
    for cin, cout, code in ((16, 16, 0), (16, 32, 0), (32, 32, 1), (32, 64, 0), (64, 64, 1), (64, 128, 0), (8, 16, 1)):
        assert l.cobevt_sparse_conv(off, ptr, ptr, None, ptr, ptr, ptr, ptr, ptr, longs(code, 2, 41, 13, 21, 100, 100, cin, cout, *sub), None) == 2
    for bad in ((2,) + good[1:], good[:5] + (0,) + good[6:], good[:6] + (-1,) + good[7:], good[:7] + (16, 64) + sub, good[:7] + (32, 16) + sub,
                good[:7] + (64, 32) + sub, good[:7] + (16, 24) + sub, good[:7] + (12, 16) + sub, good[:7] + (128, 128) + sub,
                (0, 2, 41, 13, 21, 100, 100, 8, 16) + sub,                                          # bf16 rows are 16 channels at least
                good[:9] + (3, 3, 1, 1, 1, 1, 1, 1, 1), good[:9] + (3, 3, 3, 4, 4, 4, 1, 1, 1), good[:9] + (3, 3, 3, 1, 1, 1, 3, 3, 3)):
        assert l.cobevt_sparse_conv(ptr, ptr, ptr, None, ptr, ptr, ptr, ptr, ptr, longs(*bad), None) == 2, bad
    # dense: dims = [dtype, N, D, H, W, capacity, C]
    assert l.cobevt_sparse_dense(ptr, ptr, ptr, ptr, None, None) == 1
    for hole in range(4):
        args = [ptr] * 4
        args[hole] = None
        assert l.cobevt_sparse_dense(*(args + [longs(1, 2, 2, 4, 6, 100, 128), None])) == 1
    for bad in ((3, 2, 2, 4, 6, 100, 128), (1, 2, 2, 4, 6, 0, 128), (1, 2, 2, 4, 6, 100, 0), (1, 0, 2, 4, 6, 100, 128), (1, 2, 2, 4, 6, 2 ** 31, 128)):
        assert l.cobevt_sparse_dense(ptr, ptr, ptr, ptr, longs(*bad), None) == 2, bad
    assert l.cobevt_sparse_dense(ptr, off, ptr, ptr, longs(1, 2, 2, 4, 6, 100, 128), None) == 2


# ---------------------------------------------------------------------------------------------- refusals of the host layer
def _voxel_dict(p=10, t=5, c=4):
    return {"voxel_features": torch.zeros(p, t, c), "voxel_num_points": torch.ones(p, dtype=torch.int32),
            "voxel_coords": torch.zeros(p, 4, dtype=torch.int32), "batch_size": 1}


def test_cpu_tensors_are_refused():
    d = _voxel_dict()
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        ops.mean_vfe(d["voxel_features"], d["voxel_num_points"])
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        ops.sparse_index(d["voxel_coords"], 1, (41, 13, 21))
    x = ops.SparseConvTensor(torch.zeros(10, 16), torch.zeros(10, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), (41, 13, 21), 1,
                             torch.zeros(8, dtype=torch.int32))
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        ops.sparse_downsample(x, 3, 2, 1)
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        ops.sparse_conv3d(x, ops.SparseConvPlan(torch.zeros(16, 3, 3, 3, 16), None, 1, 1, True, torch.float32, "cpu"))
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        x.dense()
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        host.MeanVFE({}, 4).eval()(dict(d))
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        host.VoxelBackBone8x({}, 4, [21, 13, 40]).eval()(dict(d, voxel_features=torch.zeros(10, 4)))
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        host.HeightCompression({"feature_num": 256}).eval()({"encoded_spconv_tensor": x, "encoded_spconv_tensor_stride": 8})


def test_train_mode_forward_raises():
    d = _voxel_dict()
    x = ops.SparseConvTensor(torch.zeros(10, 16), None, None, (2, 2, 3), 1, None)
    for module, data in ((host.MeanVFE({}, 4), dict(d)), (host.VoxelBackBone8x({}, 4, [21, 13, 40]), dict(d, voxel_features=torch.zeros(10, 4))),
                         (host.HeightCompression({"feature_num": 256}), {"encoded_spconv_tensor": x, "encoded_spconv_tensor_stride": 8})):
        assert module.training
        with pytest.raises(CobevtHipError, match="fused inference path: call .eval\\(\\) first"):
            module(data)


def test_argument_checks(monkeypatch):
    """the checks of the ops in front of their launches, with the device guard off (tests/launch_trace.py) on CPU tensors"""
    rec = lt.Recorder()
    lt.install(monkeypatch.setattr, rec)
    ws = torch.zeros(64, dtype=torch.int32)
    d = _voxel_dict()
    assert tuple(ops.mean_vfe(d["voxel_features"], d["voxel_num_points"].long(), d["voxel_coords"].long(), torch.bfloat16, 16).shape) == (10, 16)
    for bad in (torch.zeros(10, 5, 4).double(), torch.zeros(10, 4), torch.zeros(10, 5, 8)[:, :, :4]):
        with pytest.raises(CobevtHipError, match="voxel_features must be contiguous fp32"):
            ops.mean_vfe(bad, d["voxel_num_points"])
    with pytest.raises(CobevtHipError, match="channels <= 64"):
        ops.mean_vfe(d["voxel_features"], d["voxel_num_points"], channels=3)
    with pytest.raises(CobevtHipError, match="voxel_num_points must be \\(P,\\)"):
        ops.mean_vfe(d["voxel_features"], torch.ones(9, dtype=torch.int32))
    with pytest.raises(CobevtHipError, match="int32"):
        ops.mean_vfe(d["voxel_features"], torch.ones(10))
    with pytest.raises(CobevtHipError, match="voxel_coords"):
        ops.mean_vfe(d["voxel_features"], d["voxel_num_points"], torch.zeros(10, 3, dtype=torch.int32))
    x = ops.sparse_index(d["voxel_coords"], 1, (41, 13, 21), features=torch.zeros(10, 8), workspace=ws)
    assert x.capacity == 10 and tuple(x.row_map.shape) == (10,) and tuple(x.num.shape) == (2,)
    with pytest.raises(CobevtHipError, match="spatial_shape"):
        ops.sparse_index(d["voxel_coords"], 1, (41, 13), workspace=ws)
    with pytest.raises(CobevtHipError, match="capacity"):
        ops.sparse_index(d["voxel_coords"], 1, (41, 13, 21), capacity=0, workspace=ws)
    with pytest.raises(CobevtHipError, match="features must be contiguous"):
        ops.sparse_index(d["voxel_coords"], 1, (41, 13, 21), features=torch.zeros(9, 8), workspace=ws)
    with pytest.raises(CobevtHipError, match="workspace= must be"):
        ops.sparse_index(d["voxel_coords"], 1, (41, 13, 21), workspace=torch.zeros(64))
    plan = ops.SparseConvPlan(torch.zeros(16, 3, 3, 3, 4), None, 1, 1, True, torch.float32, "cpu")
    y = ops.sparse_conv3d(x, plan)
    assert tuple(y.features.shape) == (10, 16) and y.indices is x.indices and y.num is x.num and y.row_map is None
    with pytest.raises(CobevtHipError, match="x.features must be contiguous"):
        ops.sparse_conv3d(y, plan)                                                           # 16 channels into a 4-channel plan
    down = ops.SparseConvPlan(torch.zeros(32, 3, 3, 3, 16), None, 2, 1, False, torch.float32, "cpu")
    z = ops.sparse_conv3d(y, down, workspace=ws)
    assert z.spatial_shape == (21, 7, 11) and z.capacity == 80 and tuple(z.features.shape) == (80, 32)      # 8 x the input capacity
    assert ops.sparse_conv3d(y, down, capacity=7, workspace=ws).capacity == 7
    with pytest.raises(CobevtHipError, match="out_level is"):
        ops.sparse_conv3d(y, down, out_level=x)
    with pytest.raises(CobevtHipError, match="has no output"):
        ops.sparse_downsample(ops.SparseConvTensor(None, x.indices, x.num, (2, 4, 4), 1, ws), (3, 3, 3), 2, 0)
    last = ops.SparseConvTensor(torch.zeros(10, 128), x.indices, x.num, (2, 2, 3), 1, ws)
    dense = last.dense()
    assert tuple(dense.shape) == (1, 128, 2, 2, 3) and tuple(dense.view(1, 256, 2, 3).shape) == (1, 256, 2, 3)
    assert dense.view(1, 256, 2, 3).is_contiguous(memory_format=torch.channels_last)
    with pytest.raises(CobevtHipError, match="row order"):
        ops.sparse_dense(x)
    calls = [r[1] for r in rec.records]
    assert calls.count("cobevt_sparse_conv") == 3 and calls.count("cobevt_sparse_downsample") == 2 and calls.count("cobevt_sparse_dense") == 1


def test_backbone_takes_meanvfe_rows_without_a_copy():
    rows = torch.zeros(10, 8)
    assert host.VoxelBackBone8x._input_rows(rows[:, :4], torch.float32) is rows
    padded = host.VoxelBackBone8x._input_rows(torch.ones(10, 4), torch.bfloat16)
    assert tuple(padded.shape) == (10, 16) and padded.dtype == torch.bfloat16 and float(padded[:, 4:].abs().max()) == 0 and float(padded[:, :4].min()) == 1
    other = torch.zeros(10, 16)[:, :4]                     # a view of something else: copied
    assert host.VoxelBackBone8x._input_rows(other, torch.float32) is not other._base


# ---------------------------------------------------------------------------------------------- launch traces
@pytest.mark.parametrize("name", sorted(lts.CASES))
def test_launch_trace(monkeypatch, name):
    records = lts.trace(name, monkeypatch.setattr)
    assert records == lts.read_fixture(name)
    calls = [r[1] for r in records]
    assert calls == ["cobevt_mean_vfe", "cobevt_sparse_scratch", "cobevt_sparse_index", "cobevt_sparse_conv", "cobevt_sparse_conv"] + \
        ["cobevt_sparse_scratch", "cobevt_sparse_downsample", "cobevt_sparse_conv", "cobevt_sparse_conv", "cobevt_sparse_conv"] * 3 + \
        ["cobevt_sparse_scratch", "cobevt_sparse_downsample", "cobevt_sparse_conv", "cobevt_sparse_dense"]
    # the sparse kernels are library-independent objects: every mode launches them with the same arguments but the dtype code
    assert {r[0] for r in records} == {"f32s" if name == "fp32_split" else ""}
    if name == "fp32_split":
        assert [r[1:] for r in records] == [r[1:] for r in lts.read_fixture("fp32")]
    caps = [r[2][-1][6] for r in records if r[1] == "cobevt_sparse_conv"]
    p = len(sr.clustered_coords(lts.GRID, lts.BATCH, 1))
    if name == "fp32_capped":
        assert caps == [p, p, 300, 300, 300, 528, 528, 528, 40, 40, 40, 24]
    else:
        assert caps == [p, p] + [min(2 * 21 * 7 * 11, 8 * p)] * 3 + [528] * 3 + [60] * 3 + [24]
