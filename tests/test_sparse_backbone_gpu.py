"""GPU: the sparse 3-D backbone - the active-set index (ops.sparse_index / ops.sparse_downsample), cobevt_sparse_conv at kernel level
(ops.SparseConvPlan / ops.sparse_conv3d), cobevt_mean_vfe, and host.MeanVFE -> host.VoxelBackBone8x -> host.HeightCompression
(-> host.BaseBEVBackbone) against the dense restatement tests/sparse_ref.py (spconv is not installed: nothing here is the reference's
own output).

Index: indices, counts, row_map and dropped-row counters are compared exactly.

Kernel-level gates are derived per output element from a float64 evaluation of the operands the kernel gets (sparse_ref.kernel_reference:
the plan's folded weights, the input rounded to the storage dtype), with S = sum |x| |w'| over the taps present and K = Cin x (taps
present) the number of products:
    fp32   K 2^-23 S + 2^-23 |ref|       fp32 accumulation of K exact-to-fp32 products in any order, one rounding for the shift add
    bf16   ... + 2^-8 |ref|              the rounding of the stored result (bf16 products are exact in the fp32 accumulator)
MeanVFE: T 2^-23 sum |x| per element.

Module-level gates cannot be derived (twelve layers), so they are measured on the CPU (sparse_ref.module_gates): d32 = max-norm
deviation of the fp32 restatement from the float64 one, d16 = that of the restatement with the folded weights and every layer's output
rounded to bf16, both relative to max|out|; the gates are 4 d32 and 4 d16 (the MFMA's accumulation order differs from the CPU's
and both numbers are one sample):

    grid (nx, ny, nz)   voxels   d32        d16        max|out|   fp32 gate   bf16 gate
    (48, 32, 40)        589      2.931e-07  3.879e-03  0.5918     1.172e-06   1.552e-02
    (45, 31, 24)        572      2.680e-07  3.524e-03  0.6349     1.072e-06   1.410e-02
    (21, 13, 40)        527      2.388e-07  4.687e-03  0.5608     9.552e-07   1.875e-02
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import bev_backbone_ref as br
import sparse_ref as sr
from cobevt_amd import host, lib, ops
from cobevt_amd.synth import fill_module_

pytestmark = pytest.mark.gpu

# grid -> (d32, d16, max|out|), measured on the CPU by sparse_ref.module_gates on sparse_ref.module_case(grid)
DEVIATIONS = {(48, 32, 40): (2.931e-07, 3.879e-03, 0.5918), (45, 31, 24): (2.680e-07, 3.524e-03, 0.6349), (21, 13, 40): (2.388e-07, 4.687e-03, 0.5608)}
FACTOR = 4.0
SENTINEL = {torch.bfloat16: (torch.int16, 0x7FC1), torch.float32: (torch.int32, 0x7FC12345), torch.int32: (torch.int32, 0x7B7B7B7B)}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
DOWN = [(k, s, p) for _, _, _, k, s, p, subm in sr.LAYERS if not subm]          # the four strided layers' geometry


def _sentinel(shape, dtype, dev):
    idt, bits = SENTINEL[dtype]
    return torch.full(shape, bits, dtype=idt, device=dev).view(dtype)


def _is_sentinel(t):
    idt, bits = SENTINEL[t.dtype]
    return t.view(idt) == bits


def _mask_chain(coords, batch, shape):
    """the restatement's active sets of the five levels"""
    mask = sr.to_dense(coords, np.zeros((len(coords), 1)), batch, shape)[1]
    masks = [mask]
    for k, s, p in DOWN:
        masks.append(sr.out_mask(masks[-1], k, s, p, False))
    return masks


def _rows(mask):
    return mask[:, 0].nonzero().to(torch.int32)


def _level_chain(x, caps=(None,) * 4):
    levels = [x]
    for (k, s, p), cap in zip(DOWN, caps):
        levels.append(ops.sparse_downsample(levels[-1], k, s, p, capacity=cap, workspace=torch.empty(
            ops.sparse_workspace_ints(x.batch_size, ops.sparse_out_shape(levels[-1].spatial_shape, k, s, p)), dtype=torch.int32, device=x.indices.device)))
    return levels


# ---------------------------------------------------------------------------------------------- the index
@pytest.mark.parametrize("grid", sr.GRIDS)
def test_index_of_every_level_equals_the_restatement(cuda, grid):
    shape = sr.sparse_shape(grid)
    coords = sr.clustered_coords(grid, 2, sr.SEEDS[grid])
    masks = _mask_chain(coords, 2, shape)
    levels = _level_chain(ops.sparse_index(torch.from_numpy(coords).to(cuda), 2, shape))
    torch.cuda.synchronize()
    assert [lv.spatial_shape for lv in levels] == sr.shape_chain(grid)
    for lv, mask in zip(levels, masks):
        want = _rows(mask)
        assert lv.num.cpu().tolist() == [len(want), 0]                        # default capacities: nothing is dropped
        assert lv.capacity >= len(want) and torch.equal(lv.indices[:len(want)].cpu(), want)
    # row_map: the input row of every level-0 row
    src = {tuple(c): i for i, c in enumerate(coords.tolist())}
    assert levels[0].row_map[:len(coords)].cpu().tolist() == [src[tuple(r)] for r in _rows(masks[0]).tolist()]


def test_padding_out_of_range_and_duplicate_rows(cuda):
    grid = sr.GRIDS[2]
    shape = sr.sparse_shape(grid)
    base = sr.clustered_coords(grid, 2, sr.SEEDS[grid])
    d, h, w = shape
    extra = np.array([[-1, 0, 0, 0], [2, 0, 0, 0], [0, d, 0, 0], [0, 0, h, 0], [0, 0, 0, w], [1, -1, 3, 3], [0, 3, -2, 3], [1, 3, 3, -1],
                      base[5], base[5], base[0]], dtype=np.int32)              # three duplicates of earlier rows, at the end
    coords = np.concatenate([base[:40], extra[:4], base[40:], extra[4:]])
    want = _rows(_mask_chain(base, 2, shape)[0])
    x = ops.sparse_index(torch.from_numpy(coords).to(cuda), 2, shape)
    torch.cuda.synchronize()
    assert x.capacity == len(coords) and x.num.cpu().tolist() == [len(base), 0]
    assert torch.equal(x.indices[:len(base)].cpu(), want)
    first = {}
    for i, c in enumerate(coords.tolist()):
        first.setdefault(tuple(c), i)                                          # of duplicate cells the lowest input row wins
    assert x.row_map[:len(base)].cpu().tolist() == [first[tuple(r)] for r in want.tolist()]
    # no rows at all: an empty level, and every later one
    none = ops.sparse_index(torch.from_numpy(extra[:8]).to(cuda), 2, shape)
    levels = _level_chain(none)
    torch.cuda.synchronize()
    assert all(lv.num.cpu().tolist() == [0, 0] for lv in levels)


def test_overflow_with_an_explicit_capacity_drops_the_high_end(cuda):
    """level 1 gets a capacity below its active set: the kept rows are exactly the lowest-ranked ones, the counter holds the excess,
    nothing is written past the capacity (sentinel-filled buffers through the C ABI), and later levels see only the kept rows"""
    grid = sr.GRIDS[0]
    shape = sr.sparse_shape(grid)
    coords = sr.clustered_coords(grid, 2, sr.SEEDS[grid])
    masks = _mask_chain(coords, 2, shape)
    want1 = _rows(masks[1])
    cap, guard = len(want1) - 197, 64
    assert cap > 100
    x = ops.sparse_index(torch.from_numpy(coords).to(cuda), 2, shape)
    k, s, p = DOWN[0]
    so = ops.sparse_out_shape(shape, k, s, p)
    ws = torch.empty(ops.sparse_workspace_ints(2, so), dtype=torch.int32, device=cuda)
    indices, num = _sentinel((cap + guard, 4), torch.int32, cuda), _sentinel((2 + guard,), torch.int32, cuda)
    dims = (ctypes.c_long * 15)(2, *(shape + (x.capacity, cap) + k + s + p))
    lib.call("cobevt_sparse_downsample", ops._p(x.indices), ops._p(x.num), ops._p(ws), ops._p(indices), ops._p(num), dims, ops._stream())
    torch.cuda.synchronize()
    assert num[:2].cpu().tolist() == [cap, 197] and bool(_is_sentinel(num[2:]).all())
    assert torch.equal(indices[:cap].cpu(), want1[:cap]) and bool(_is_sentinel(indices[cap:]).all())
    # a convolution onto the capped level: rows below the capacity are those of the uncapped run, bit for bit; nothing past them
    c = sr.kernel_case("down_16_32_pad1")
    feats = torch.randn(len(coords), 16, generator=torch.Generator().manual_seed(3)).to(cuda)
    plan = ops.SparseConvPlan(c["weight"], sr.bn_module(c["bn"]), 2, 1, False, torch.float32, cuda)
    x.features = feats
    full = ops.sparse_conv3d(x, plan)
    capped = ops.SparseConvTensor(None, indices[:cap], num[:2], so, 2, ws)
    out = _sentinel((cap + guard, 32), torch.float32, cuda)
    dims = (ctypes.c_long * 18)(1, 2, *(shape + (len(coords), cap, 16, 32) + k + s + p))
    lib.call("cobevt_sparse_conv", ops._p(feats), ops._p(x.workspace), ops._p(x.num), ops._p(x.row_map), ops._p(capped.indices), ops._p(capped.num),
             ops._p(plan.wgt), ops._p(plan.shift), ops._p(out), dims, ops._stream())
    torch.cuda.synchronize()
    assert full.num.cpu().tolist() == [len(want1), 0]
    assert torch.equal(out[:cap], full.features[:cap]) and bool(_is_sentinel(out[cap:]).all()) and not bool(_is_sentinel(out[:cap]).any())
    # the next level is built from the kept rows only
    kept = torch.zeros_like(masks[1])
    kept[want1[:cap, 0].long(), 0, want1[:cap, 1].long(), want1[:cap, 2].long(), want1[:cap, 3].long()] = True
    k2, s2, p2 = DOWN[1]
    nxt = ops.sparse_downsample(capped, k2, s2, p2)
    want2 = _rows(sr.out_mask(kept, k2, s2, p2, False))
    torch.cuda.synchronize()
    assert nxt.num.cpu().tolist() == [len(want2), 0] and torch.equal(nxt.indices[:len(want2)].cpu(), want2)
    assert len(want2) < int(masks[2].sum())                                   # the drop is visible one level down


# ---------------------------------------------------------------------------------------------- the convolution kernel
@pytest.fixture(scope="module")
def kernel_refs():
    """(case, storage dtype) -> the case, its CPU plan and its float64 reference, computed once"""
    out = {}
    for name in sr.KERNEL_CASES:
        c = sr.kernel_case(name)
        for dt in (torch.bfloat16, torch.float32):
            plan = ops.SparseConvPlan(c["weight"], sr.bn_module(c["bn"]), c["stride"], c["padding"], c["subm"], dt, "cpu")
            out[name, dt] = (c, plan) + sr.kernel_reference(c["feats"].to(dt), c["coords"], sr.KERNEL_BATCH, sr.KERNEL_SHAPE, plan.wgt, plan.shift,
                                                           c["cin"], c["cout"], c["kernel"], c["stride"], c["padding"], c["subm"])
    return out


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(sr.KERNEL_CASES))
def test_sparse_conv_kernel(cuda, kernel_refs, name, mode):
    dt = DTYPES[mode]
    c, cpu_plan, idx, ref, mag, k = kernel_refs[name, dt]
    rows = torch.zeros((len(c["coords"]), cpu_plan.cin_pad), dtype=dt)
    rows[:, :c["cin"]] = c["feats"].to(dt)
    plan = copy.copy(cpu_plan)
    plan.wgt, plan.shift = cpu_plan.wgt.to(cuda), cpu_plan.shift.to(cuda)
    x = ops.sparse_index(c["coords"].to(cuda), sr.KERNEL_BATCH, sr.KERNEL_SHAPE, features=rows.to(cuda))
    y = ops.sparse_conv3d(x, plan)
    torch.cuda.synchronize()
    n = len(idx)
    assert y.num.cpu().tolist() == [n, 0] and torch.equal(y.indices[:n].cpu(), idx) and y.features.dtype == dt
    assert (y.indices is x.indices) == c["subm"] and tuple(y.features.shape) == (y.capacity, c["cout"])
    got = y.features[:n].cpu().double()
    assert bool(torch.isfinite(got).all())
    bound = k * 2.0 ** -23 * mag + 2.0 ** -23 * ref.abs() + (2.0 ** -8 * ref.abs() if mode == "bf16" else 0.0)
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-30)).max())
    print("sparse_conv %s %s: %d rows, max|err| %.3e, max err / bound %.3f, max|ref| %.3f, %.0f %% cut by the ReLU"
          % (mode, name, n, float(err.max()), ratio, float(ref.abs().max()), 100 * float((ref == 0).double().mean())))
    assert float(ref.abs().max()) > 0.1 and 0.05 < float((ref == 0).double().mean()) < 0.95
    assert bool((err <= bound).all()), "max err / bound = %.3f" % ratio


# ---------------------------------------------------------------------------------------------- MeanVFE
@pytest.mark.parametrize("slots", [5, 32])
def test_mean_vfe(cuda, slots):
    g = torch.Generator().manual_seed(slots)
    p, c = 203, 4
    vf = (torch.rand(p, slots, c, generator=g) - 0.5) * 4.0
    npts = torch.randint(0, slots + 1, (p,), generator=g, dtype=torch.int32)
    npts[:4] = torch.tensor([0, slots, 1, slots])
    used = torch.arange(slots)[None, :] < npts[:, None]
    clean = vf * used[:, :, None]
    dirty = torch.where(used[:, :, None], vf, torch.full_like(vf, float("nan")))          # garbage in the unused slots
    dirty[1::2] = torch.where(used[1::2, :, None], vf[1::2], torch.full_like(vf[1::2], 1e30))
    coords = torch.zeros(p, 4, dtype=torch.int32)
    coords[7], coords[8] = torch.tensor([-1, 0, 0, 0]), torch.tensor([-1, 0, 0, 0])      # padding rows
    ref = clean.double().sum(dim=1) / npts.clamp_min(1).double()[:, None]
    ref[7:9] = 0
    gate = slots * 2.0 ** -23 * clean.double().abs().sum(dim=1)
    out = ops.mean_vfe(dirty.to(cuda), npts.to(cuda), coords.to(cuda))
    padded = ops.mean_vfe(dirty.to(cuda), npts.to(cuda), coords.to(cuda), channels=8)
    half = ops.mean_vfe(dirty.to(cuda), npts.to(cuda), coords.to(cuda), dtype=torch.bfloat16, channels=16)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (p, c) and out.dtype == torch.float32
    err = (out.cpu().double() - ref).abs()
    print("mean_vfe T=%d: max err / gate %.3f" % (slots, float((err / gate.clamp_min(1e-30)).max())))
    assert bool((err <= gate).all()) and float(out[0].abs().max()) == 0 and float(out[7:9].abs().max()) == 0
    assert torch.equal(padded[:, :c], out) and float(padded[:, c:].abs().max()) == 0
    assert torch.equal(half[:, :c], out.to(torch.bfloat16)) and float(half[:, c:].float().abs().max()) == 0


# ---------------------------------------------------------------------------------------------- the modules
def _modules(grid, cuda, caps=None):
    vfe = host.MeanVFE({}, 4).eval()
    backbone = fill_module_(host.VoxelBackBone8x({"level_capacities": caps}, 4, list(grid)), 0).eval()
    sd = backbone.state_dict()
    return vfe, backbone.to(cuda), host.HeightCompression({"feature_num": 128 * sr.shape_chain(grid)[-1][0]}).eval(), sd


def _forward(mods, data, mode, cuda):
    vfe, backbone, to_bev, _ = mods
    batch = {k: v.to(cuda) for k, v in data.items()}
    batch["batch_size"] = 2
    with torch.no_grad(), host.compute_dtype(mode):
        out = to_bev(backbone(vfe(batch)))
    assert out is batch
    return out


@pytest.fixture(scope="module")
def module_refs():
    """grid -> (voxel dict, state_dict, the restatement's levels, its float64 spatial_features), computed once"""
    out = {}
    for grid in sr.GRIDS:
        data, mean = sr.module_case(grid)
        sd = fill_module_(host.VoxelBackBone8x({}, 4, list(grid)), 0).state_dict()
        levels, ref = sr.backbone(sd, data["voxel_coords"].numpy(), mean, 2, grid, "f64")
        out[grid] = (data, sd, levels, ref)
    return out


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("grid", sr.GRIDS)
def test_backbone_matches_the_restatement(cuda, module_refs, grid, mode):
    data, sd, levels, ref = module_refs[grid]
    d32, d16, scale = DEVIATIONS[grid]
    gate = FACTOR * (d16 if mode == "bf16" else d32)
    out = _forward(_modules(grid, cuda), data, mode, cuda)
    torch.cuda.synchronize()
    y, enc = out["spatial_features"], out["encoded_spconv_tensor"]
    d, h, w = sr.shape_chain(grid)[-1]
    assert tuple(y.shape) == (2, 128 * d, h, w) == tuple(ref.shape) and y.dtype == DTYPES[mode]
    assert out["spatial_features_stride"] == out["encoded_spconv_tensor_stride"] == 8
    assert out["multi_scale_3d_strides"] == {"x_conv1": 1, "x_conv2": 2, "x_conv3": 4, "x_conv4": 8}
    # the active set of every level
    for key, name in (("x_conv1", "conv1.0"), ("x_conv2", "conv2.2"), ("x_conv3", "conv3.2"), ("x_conv4", "conv4.2"), (None, "conv_out")):
        t = enc if key is None else out["multi_scale_3d_features"][key]
        want = _rows(levels[name][1])
        assert t.num.cpu().tolist() == [len(want), 0] and torch.equal(t.indices[:len(want)].cpu(), want)
        assert t.spatial_shape == tuple(levels[name][1].shape[2:]) and t.batch_size == 2
    # the channel order c D + d of spatial_features, straight from the rows
    n = int(enc.num[0])
    idx, f = enc.indices[:n].long().cpu(), enc.features[:n].cpu()
    yc = y.cpu()
    for r in (0, n // 2, n - 1):
        b, z, yy, xx = idx[r].tolist()
        assert torch.equal(yc[b, z::d, yy, xx], f[r])                           # channels c * D + z, c = 0 .. 127
    assert int((yc != 0).any(dim=1).sum()) <= n
    dense = enc.dense()
    assert tuple(dense.shape) == (2, 128, d, h, w) and torch.equal(dense.reshape(2, 128 * d, h, w), y)
    err = float((yc.double() - ref).abs().max()) / float(ref.abs().max())
    print("VoxelBackBone8x %s %s: max-norm rel err %.3e (gate %.3e)" % (grid, mode, err, gate))
    assert abs(float(ref.abs().max()) - scale) < 1e-3 * scale
    assert err <= gate, "%s %s: %.3e > %.3e" % (grid, mode, err, gate)


def test_fp32_split_runs_the_same_kernel_and_permuted_rows_change_nothing(cuda, module_refs):
    grid = sr.GRIDS[2]
    data = module_refs[grid][0]
    mods = _modules(grid, cuda)
    first = _forward(mods, data, "fp32", cuda)["spatial_features"].clone()
    again = _forward(mods, data, "fp32", cuda)
    split = _forward(mods, data, "fp32_split", cuda)["spatial_features"]
    perm = torch.randperm(len(data["voxel_coords"]), generator=torch.Generator().manual_seed(5))
    moved = _forward(mods, {k: v[perm] for k, v in data.items()}, "fp32", cuda)
    torch.cuda.synchronize()
    assert torch.equal(again["spatial_features"], first) and torch.equal(split, first)        # two runs; the library-independent object
    assert torch.equal(moved["spatial_features"], first)
    for key in ("x_conv1", "x_conv2", "x_conv3", "x_conv4"):
        a, b = again["multi_scale_3d_features"][key], moved["multi_scale_3d_features"][key]
        n = int(a.num[0])
        assert torch.equal(a.num, b.num) and torch.equal(a.indices[:n], b.indices[:n]) and torch.equal(a.features[:n], b.features[:n])
    half = [_forward(mods, d, "bf16", cuda)["spatial_features"].clone() for d in (data, {k: v[perm] for k, v in data.items()}, data)]
    torch.cuda.synchronize()
    assert torch.equal(half[0], half[1]) and torch.equal(half[0], half[2])


def test_captured_forward_replays_on_a_second_cloud(cuda, module_refs):
    """the forward captured in a HIP graph on one cloud and replayed on another with different counts: fixed-size voxel dict, padding rows"""
    grid = sr.GRIDS[2]
    first, _ = sr.module_case(grid, pad_rows=100)
    data_b, mean_b = sr.module_case(grid)
    # the second cloud: a different subset of voxels (every third one dropped), so that every level's count differs
    keep = torch.arange(len(data_b["voxel_coords"])) % 3 != 0
    second = {k: torch.cat([v[keep], first[k][int(keep.sum()):]]) for k, v in data_b.items()}
    second["voxel_coords"][int(keep.sum()):] = torch.tensor([-1, 0, 0, 0], dtype=torch.int32)
    assert all(second[k].shape == first[k].shape for k in first)
    mods = _modules(grid, cuda)
    static = {k: v.to(cuda) for k, v in first.items()}
    static["batch_size"] = 2

    def run():
        with torch.no_grad(), host.compute_dtype("fp32"):
            return mods[2](mods[1](mods[0](dict(static))))

    eager_a = run()["spatial_features"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["spatial_features"], eager_a)
    for k, v in second.items():
        static[k].copy_(v.to(cuda))
    graph.replay()
    torch.cuda.synchronize()
    replay_b = out["spatial_features"].clone()
    nums_b = [out["multi_scale_3d_features"][k].num.cpu().tolist() for k in ("x_conv1", "x_conv2", "x_conv3", "x_conv4")]
    nums_b.append(out["encoded_spconv_tensor"].num.cpu().tolist())
    eager_b = run()
    torch.cuda.synchronize()
    assert torch.equal(replay_b, eager_b["spatial_features"]) and not torch.equal(replay_b, eager_a)
    means = np.concatenate([mean_b[keep.numpy()], np.zeros((len(first["voxel_coords"]) - int(keep.sum()), 4))])
    levels, ref, d32, _ = sr.module_gates(mods[3], second["voxel_coords"].numpy(), means, 2, grid)
    live = [int(levels[name][1].sum()) for name in ("conv1.0", "conv2.2", "conv3.2", "conv4.2")]
    assert nums_b == [[n, 0] for n in live] + [[int(levels["conv_out"][1].sum()), 0]] and live[0] == int(keep.sum())
    assert live[0] != int(module_refs[grid][2]["conv1.0"][1].sum()) and live[1] != int(module_refs[grid][2]["conv2.2"][1].sum())
    err = float((replay_b.cpu().double() - ref).abs().max()) / float(ref.abs().max())
    print("captured VoxelBackBone8x, second cloud: max-norm rel err %.3e (gate %.3e, measured for this cloud)" % (err, FACTOR * d32))
    assert err <= FACTOR * d32


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_composition_into_base_bev_backbone(cuda, module_refs, mode):
    """spatial_features is what host.BaseBEVBackbone.forward reads: the two run back to back and match the restatement feeding
    tests/bev_backbone_ref.mirror"""
    grid = sr.GRIDS[0]
    data, sd, levels, ref = module_refs[grid]
    coords, mean = data["voxel_coords"].numpy(), sr.module_case(grid)[1]
    cfg = {"layer_nums": [1, 1], "layer_strides": [1, 2], "num_filters": [32, 64], "upsample_strides": [1, 2], "num_upsample_filter": [32, 32]}
    bev = fill_module_(host.BaseBEVBackbone(copy.deepcopy(cfg), ref.shape[1]), 0).eval()
    bev_sd = bev.state_dict()
    bev = bev.to(cuda)
    out = _forward(_modules(grid, cuda), data, mode, cuda)
    with torch.no_grad(), host.compute_dtype(mode):
        y = bev(out)["spatial_features_2d"]
    torch.cuda.synchronize()
    with torch.no_grad():
        want = br.mirror(bev_sd, cfg, ref, torch.float64)
        # the chain's own measured deviation: the fp32 (bf16-storage) restatement feeding the fp32 (bf16-rounded) mirror
        if mode == "bf16":
            low = br.mirror(bev_sd, cfg, sr.backbone(sd, coords, mean, 2, grid, "bf16")[1], torch.float64, bf16=True)
        else:
            low = br.mirror(bev_sd, cfg, sr.backbone(sd, coords, mean, 2, grid, "f32")[1], torch.float32)
    scale = float(want.abs().max())
    gate = FACTOR * float((low.double() - want).abs().max()) / scale
    err = float((y.cpu().double() - want).abs().max()) / scale
    print("VoxelBackBone8x -> BaseBEVBackbone %s: max-norm rel err %.3e (gate %.3e), max|out| %.3f" % (mode, err, gate, scale))
    assert tuple(y.shape) == tuple(want.shape) == (2, 64, 4, 6) and scale > 0.1 and err <= gate
