"""The voxeliser on the GPU: cobevt_voxelize_points (csrc/voxelize.hip) through ops.voxelize_points, host.SpVoxelPreprocessor and
PointPillarFuseBEVT fed raw points, against the sequential restatement tests/voxel_ref.py (itself pinned to the reference's point masks
and to a hand-written example by tests/test_voxelize.py).

Every comparison is exact: voxel_coords, voxel_num_points and num_voxels over all N * max_voxels rows, voxel_features bit for bit over
the used rows (the operator does not write the others).  There is no tolerance in this file.  Each case asserts its own preconditions
on the restatement's output."""
import copy

import numpy as np
import pytest
import torch

import cases_pillar as cp
import cases_voxel as cv
import voxel_ref as vr
from cobevt_amd import host, ops
from cobevt_amd.host import pipeline
from cobevt_amd.synth import fill_module_

pytestmark = pytest.mark.gpu


def _dev(pts, offs, dev):
    return torch.from_numpy(np.ascontiguousarray(pts)).to(dev), torch.from_numpy(np.asarray(offs, dtype=np.int32)).to(dev)


def _run(dev, pts, offs, rng, t, mv, **kw):
    p, o = _dev(pts, offs, dev)
    out = ops.voxelize_points(p, o, rng, cv.VOXEL_SIZE, t, mv, **kw)
    torch.cuda.synchronize()
    return out


def _bits(x):
    return x.contiguous().view(torch.int32)


def _check(got, ref, what=""):
    vf, coords, npts, nvox = [g.cpu() for g in got]
    assert torch.equal(nvox, torch.from_numpy(ref["num_voxels"])), what + " num_voxels"
    assert torch.equal(coords, torch.from_numpy(ref["voxel_coords"])), what + " voxel_coords"
    assert torch.equal(npts, torch.from_numpy(ref["voxel_num_points"])), what + " voxel_num_points"
    used = torch.from_numpy(ref["voxel_num_points"] > 0)
    assert tuple(vf.shape) == ref["voxel_features"].shape
    assert torch.equal(_bits(vf[used]), _bits(torch.from_numpy(ref["voxel_features"])[used])), what + " voxel_features"


# ---------------------------------------------------------------------------------------------- 1. counts
@pytest.fixture(scope="module")
def counts_data():
    return cv.counts_case()


@pytest.mark.parametrize("t", [32, 5])
def test_counts(cuda, counts_data, t):
    """5 x 7 cells, 3 agents, about 3 000 shuffled points each: cells of exactly 1, 31, 32, 33, 64, 65 and more than 200 points"""
    pts, offs, rng = counts_data
    mv = 35
    ref = vr.voxelize(pts, offs, rng, cv.VOXEL_SIZE, t, mv)
    used = ref["voxel_num_points"] > 0
    counts = ref["cell_count"][used]
    assert all(2800 <= int(offs[a + 1] - offs[a]) <= 3200 for a in range(3))
    for c in (1, 31, 32, 33, 64, 65):
        assert bool((counts == c).any()), c
    assert bool((counts > 200).any()) and float((counts > t).mean()) >= 0.2
    _check(_run(cuda, pts, offs, rng, t, mv), ref, "counts T=%d" % t)


# ---------------------------------------------------------------------------------------------- 2. the voxel cap
def test_max_voxels_cap(cuda):
    pts, offs, rng = cv.cap_case()
    mv, t = cv.CAP_MAX_VOXELS, 32
    ref = vr.voxelize(pts, offs, rng, cv.VOXEL_SIZE, t, mv)
    over = [a for a in range(3) if len(ref["dropped_cells"][a]) > 0]
    assert len(over) >= 2 and int((ref["num_voxels"] < mv).sum()) >= 1 and all(int(ref["num_voxels"][a]) == mv for a in over)
    # a dropped cell has points later in the input than points of a kept cell, and a kept cell goes on accepting points after a
    # dropped cell's first point (spconv's `continue`)
    keep, ys, xs = vr.classify(pts, rng, cv.VOXEL_SIZE)
    a = over[0]
    idx = np.arange(offs[a], offs[a + 1])
    dropped = np.array([(int(ys[i]), int(xs[i])) in ref["dropped_cells"][a] for i in idx])
    assert idx[dropped].max() > idx[~dropped].min() and idx[~dropped].max() > idx[dropped].min()
    _check(_run(cuda, pts, offs, rng, t, mv), ref, "cap")


# ---------------------------------------------------------------------------------------------- 3. scan seams
@pytest.fixture(scope="module")
def seam_data():
    pts, offs, rng = cv.seam_case()
    return pts, offs, rng, vr.voxelize(pts, offs, rng, cv.VOXEL_SIZE, 32, 600)


def test_scan_seams(cuda, seam_data):
    """70 000 points (more than 256 x 256) on 24 x 24 cells; the agents' boundary at 33 333, one agent without points"""
    pts, offs, rng, ref = seam_data
    assert len(pts) == 70000 > 65536 and offs[1] % 256 != 0 and offs[1] % 1024 != 0 and offs[1] == offs[2]
    assert ref["num_voxels"].tolist()[1] == 0 and ref["num_voxels"][0] > 500 and ref["num_voxels"][2] > 500
    _check(_run(cuda, pts, offs, rng, 32, 600), ref, "seams")


def test_no_points(cuda):
    pts, offs = np.zeros((0, 4), dtype=np.float32), np.zeros(3, dtype=np.int32)
    rng = cv.lidar_range(*cv.SEAM_GRID)
    ref = vr.voxelize(pts, offs, rng, cv.VOXEL_SIZE, 32, 20)
    assert ref["num_voxels"].tolist() == [0, 0] and bool((ref["voxel_coords"][:, 0] == -1).all())
    _check(_run(cuda, pts, offs, rng, 32, 20), ref, "M = 0")


def test_rows_past_the_last_offset_are_ignored(cuda, seam_data):
    """offsets[N] < M: the tail rows hold valid points with a marker intensity; none of them reaches the output"""
    pts, offs, rng, _ = seam_data
    pts, offs = pts.copy(), offs.copy()
    offs[3] = 60001
    pts[60001:, 3] = 777.0
    ref = vr.voxelize(pts, offs, rng, cv.VOXEL_SIZE, 32, 600)
    keep, _, _ = vr.classify(pts[60001:], rng, cv.VOXEL_SIZE)
    assert bool(keep.all()) and not bool((ref["voxel_features"][..., 3] == 777.0).any())
    got = _run(cuda, pts, offs, rng, 32, 600)
    _check(got, ref, "tail")
    used = torch.from_numpy(ref["voxel_num_points"] > 0)
    assert not bool((got[0].cpu()[used][..., 3] == 777.0).any())


# ---------------------------------------------------------------------------------------------- 4. edges
@pytest.mark.parametrize("range_mask,ego_mask", [(False, False), (True, False), (False, True), (True, True)])
def test_edges(cuda, range_mask, ego_mask):
    """the golden cloud (points on every range face and ego-box edge), NaN / inf coordinates, points on lo, hi and interior cell edges,
    and points whose cell a reciprocal multiply would get wrong; voxel_size 0.4"""
    pts, offs, rng, sx, sy = cv.edge_case()
    nx = cv.GOLDEN_GRID[1]
    assert len(sx) >= 10 and len(sy) >= 10
    assert all(bool((pts[:, 0] == x).any()) for x in sx) and all(bool((pts[:, 1] == y).any()) for y in sy)
    v, lo = np.float32(cv.VOXEL_SIZE[0]), np.float32(rng[0])
    assert bool((np.floor((sx - lo) / v) != np.floor((sx - lo) * (np.float32(1) / v))).all())
    assert int(np.isnan(pts[:, :3]).any(1).sum()) >= 3 and int(np.isinf(pts[:, :3]).any(1).sum()) >= 6
    for axis in (0, 1):
        assert bool((pts[:, axis] == np.float32(rng[axis])).any()) and bool((pts[:, axis] == np.float32(rng[3 + axis])).any())
        assert bool((pts[:, axis] == np.float32(rng[axis] + (nx // 2) * cv.VOXEL_SIZE[axis])).any())
    ref = vr.voxelize(pts, offs, rng, cv.VOXEL_SIZE, 32, 700, range_mask, ego_mask)
    plain = vr.voxelize(pts, offs, rng, cv.VOXEL_SIZE, 32, 700)
    if range_mask or ego_mask:
        assert int(ref["voxel_num_points"].sum()) < int(plain["voxel_num_points"].sum())
    assert bool((ref["voxel_coords"][:, 3] == 0).any())                      # the points on lo are kept by the cell test
    _check(_run(cuda, pts, offs, rng, 32, 700, range_mask=range_mask, ego_mask=ego_mask), ref, "edges")


# ---------------------------------------------------------------------------------------------- 5. determinism and bounds
def test_determinism_and_bounds(cuda, counts_data):
    """two runs are bit-identical; outputs and workspace are the interiors of larger buffers whose margins keep a marker; the
    features of rows without a voxel stay exactly as the caller filled them"""
    pts, offs, rng = counts_data
    t, mv, margin = 32, 40, 256
    ref = vr.voxelize(pts, offs, rng, cv.VOXEL_SIZE, t, mv)
    assert int((ref["voxel_num_points"] == 0).sum()) == 3 * (mv - 35)
    p, o = _dev(pts, offs, cuda)
    first = ops.voxelize_points(p, o, rng, cv.VOXEL_SIZE, t, mv)
    torch.cuda.synchronize()
    ws_ints = ops.voxelize_workspace_ints(len(pts), 3, (7, 5, 1), t, mv)
    shapes = [((3 * mv, t, 4), torch.float32, 7.0), ((3 * mv, 4), torch.int32, 77), ((3 * mv,), torch.int32, 77), ((3,), torch.int32, 77)]
    bigs, outs = [], []
    for shape, dtype, mark in shapes:
        n = int(np.prod(shape))
        big = torch.full((n + 2 * margin,), mark, device=cuda, dtype=dtype)
        bigs.append((big, n, mark))
        outs.append(big[margin:margin + n].view(shape))
    big_ws = torch.full((ws_ints + 2 * margin,), 77, device=cuda, dtype=torch.int32)
    got = ops.voxelize_points(p, o, rng, cv.VOXEL_SIZE, t, mv, out=outs, workspace=big_ws[margin:margin + ws_ints])
    torch.cuda.synchronize()
    assert all(g.data_ptr() == w.data_ptr() for g, w in zip(got, outs))
    _check(got, ref, "bounds")
    for big, n, mark in bigs:
        assert bool((big[:margin] == mark).all()) and bool((big[margin + n:] == mark).all())
    assert bool((big_ws[:margin] == 77).all()) and bool((big_ws[margin + ws_ints:] == 77).all())
    unused = torch.from_numpy(ref["voxel_num_points"] == 0)
    assert bool((got[0].cpu()[unused] == 7.0).all())
    used = ~unused
    assert torch.equal(_bits(first[0].cpu()[used]), _bits(got[0].cpu()[used]))
    assert all(torch.equal(a, b) for a, b in zip(first[1:], got[1:]))


# ---------------------------------------------------------------------------------------------- 6. the model
MODEL_MAX_VOXELS = 256


def _model_args():
    fusion = copy.deepcopy(cp.FUSION)
    fusion["drop_out"] = 0.0
    args = cp.model_args(fusion=fusion)
    args["preprocess"] = cv.preprocess_params(cp.GRID, 32, MODEL_MAX_VOXELS, MODEL_MAX_VOXELS)
    return args


def _model_cloud(tag, sizes):
    ny, nx = cp.GRID
    clouds = []
    for a, m in enumerate(sizes):
        u = cv.uniform("%s.cell.%d" % (tag, a), (m,))
        cell = np.where(u < 0.4, (u * 2.5 * 9).astype(np.int64) * 29 % (ny * nx), (u * 6007).astype(np.int64) % (ny * nx))
        clouds.append(cv.points_in_cells("%s.%d" % (tag, a), cell // nx, cell % nx, cp.GRID))
    return cv.concat(clouds)


def _ref_dict(pts, offs, dev):
    ref = vr.voxelize(pts, offs, cp.LIDAR_RANGE, cp.VOXEL_SIZE, 32, MODEL_MAX_VOXELS)
    assert bool((ref["cell_count"] > 32).any()) and bool((ref["voxel_num_points"] == 0).any())
    return {k: torch.from_numpy(ref[k]).to(dev) for k in ("voxel_features", "voxel_coords", "voxel_num_points")}


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_model_from_points(cuda, mode):
    assert cv.lidar_range(*cp.GRID) == cp.LIDAR_RANGE and cv.VOXEL_SIZE == cp.VOXEL_SIZE
    m = fill_module_(host.PointPillarFuseBEVT(_model_args()), cp.SEED).eval().to(cuda)
    pts, offs = _model_cloud("model", [1500, 1100, 1300])
    p, o = _dev(pts, offs, cuda)
    rl = torch.tensor(cp.RECORD_LEN, dtype=torch.int32, device=cuda)
    with torch.no_grad(), host.compute_dtype(mode):
        got = m({"lidar_points": p, "lidar_point_offsets": o.long(), "record_len": rl})["fused_feature"]
        ref = m({"processed_lidar": _ref_dict(pts, offs, cuda), "record_len": rl})["fused_feature"]
    torch.cuda.synchronize()
    assert tuple(got.shape) == (2, 64, 16, 16) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    assert torch.equal(got, ref)


def test_model_trains_from_points(cuda):
    """one train() forward + backward from points against the same model fed the restatement's dict: the output, the running
    statistics and the gradients of the pillar encoder's parameters - everything the voxel dict feeds, through kernels without
    floating-point atomics - are bit-identical.  The gradients of fusion_net's parameters are required finite and
    non-zero only: its LayerNorm, attention-bias and convolution weight-gradient kernels (csrc/train_rows.hip, attention_bwd.hip) add
    their partial sums with floating-point atomics, so they differ in the last bits between two runs of one and the same batch
    (measured here on the first run: fusion_net.layers.0.window_attention.norm.weight), whatever produced the voxels."""
    pts, offs = _model_cloud("model", [1500, 1100, 1300])
    p, o = _dev(pts, offs, cuda)
    rl = torch.tensor(cp.RECORD_LEN, dtype=torch.int32, device=cuda)
    w = None
    results = []
    with torch.enable_grad(), host.compute_dtype("fp32"):
        for feed in ("points", "dict"):
            m = fill_module_(host.PointPillarFuseBEVT(_model_args()), cp.SEED).train().to(cuda)
            batch = {"lidar_points": p, "lidar_point_offsets": o, "record_len": rl} if feed == "points" else \
                {"processed_lidar": _ref_dict(pts, offs, cuda), "record_len": rl}
            out = m(batch)["fused_feature"]
            if w is None:
                w = torch.linspace(-1.0, 1.0, out.numel(), device=cuda).reshape(out.shape)
            (out * w).sum().backward()
            torch.cuda.synchronize()
            results.append((out.detach(), {k: q.grad.detach().clone() for k, q in m.named_parameters()},
                            {k: b.detach().clone() for k, b in m.named_buffers()}))
    (out_a, grad_a, buf_a), (out_b, grad_b, buf_b) = results
    assert torch.equal(out_a, out_b) and bool(torch.isfinite(out_a).all())
    assert set(grad_a) == set(grad_b) and len(grad_a) > 0
    front = [k for k in grad_a if k.startswith("pillar_vfe.")]
    assert len(front) == 3, front
    for k in grad_a:
        assert bool(torch.isfinite(grad_a[k]).all()) and bool(torch.isfinite(grad_b[k]).all()), k
        if k in front:
            assert torch.equal(grad_a[k], grad_b[k]) and float(grad_a[k].abs().max()) > 0, k
    assert any(float(g.abs().max()) > 0 for k, g in grad_a.items() if k not in front)
    assert int(buf_a["pillar_vfe.pfn_layers.0.norm.num_batches_tracked"]) == 1
    for k in buf_a:
        assert torch.equal(buf_a[k], buf_b[k]), k


def test_graph_replay_from_points(cuda):
    """pipeline.CapturedCall over the forward from points at a fixed M with device-side offsets: the second cloud has fewer points
    (offsets[N] < M), each replay equals its eager run"""
    m = fill_module_(host.PointPillarFuseBEVT(_model_args()), cp.SEED).eval().to(cuda)
    m_fixed = 4000
    sets = []
    for tag, sizes in (("replay.a", [1500, 1200, 1300]), ("replay.b", [900, 1700, 1000])):
        pts, offs = _model_cloud(tag, sizes)
        pad = np.full((m_fixed - len(pts), 4), 0.1, dtype=np.float32)
        sets.append(_dev(np.concatenate([pts, pad]), offs, cuda))
    rl = torch.tensor(cp.RECORD_LEN, dtype=torch.int32, device=cuda)

    def fn(points, offsets, record_len):
        return m({"lidar_points": points, "lidar_point_offsets": offsets, "record_len": record_len})
    with torch.no_grad(), host.compute_dtype("bf16"):
        eager = [fn(p, o, rl)["fused_feature"].clone() for p, o in sets]
        run = pipeline.CapturedCall(fn, sets[0][0], sets[0][1], rl)
        assert run.graph is not None
        for i in (0, 1, 0):
            got = run.step(sets[i][0], sets[i][1], rl)["fused_feature"]
            torch.cuda.synchronize()
            assert torch.equal(got, eager[i]), i
    assert not torch.equal(eager[0], eager[1])


# ---------------------------------------------------------------------------------------------- 7. full size, once
def test_full_size(cuda):
    """8 agents x 65 536 points on 256 x 256 cells, T = 32, max_voxels = 32 000, against the vectorised restatement (pinned to the
    literal loop by tests/test_voxelize.py)"""
    pts, offs, rng = cv.full_case()
    ref = vr.voxelize_fast(pts, offs, rng, cv.VOXEL_SIZE, 32, cv.FULL_MAX_VOXELS)
    assert len(pts) == 8 * 65536 and int(ref["num_voxels"].min()) > 20000 and int(ref["cell_count"].max()) > 200
    _check(_run(cuda, pts, offs, rng, 32, cv.FULL_MAX_VOXELS), ref, "full size")
