"""The 3-D voxeliser on the GPU: cobevt_voxelize3d_points (csrc/voxelize.hip) through ops.voxelize_points_3d and
host.SpVoxelPreprocessor3D, against the sequential restatement tests/voxel3d_ref.py (itself pinned to a hand-written example, to its
literal loop and to voxel_ref.py by tests/test_voxelize3d.py, which also asserts what each cloud of cases_voxel3d holds).

Every comparison is exact: voxel_coords, voxel_num_points and num_voxels over all N * max_voxels rows, voxel_features bit for bit over
the used rows (the operator does not write the others).  There is no tolerance in this file."""
import numpy as np
import pytest
import torch

import cases_voxel as cv
import cases_voxel3d as c3
import sparse_ref as sr
import voxel3d_ref as v3
import voxel_ref as vr
from cobevt_amd import host, ops
from cobevt_amd.lib import CobevtHipError
from cobevt_amd.synth import fill_module_

pytestmark = pytest.mark.gpu


def _dev(pts, offs, dev):
    return torch.from_numpy(np.ascontiguousarray(pts)).to(dev), torch.from_numpy(np.asarray(offs, dtype=np.int32)).to(dev)


def _run(dev, pts, offs, rng, vs, t, mv, **kw):
    p, o = _dev(pts, offs, dev)
    out = ops.voxelize_points_3d(p, o, rng, vs, t, mv, **kw)
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


def _check_same(got, other, ref, what=""):
    """two runs of the operator: all four outputs bit-equal (features over the used rows)"""
    used = torch.from_numpy(ref["voxel_num_points"] > 0)
    assert torch.equal(_bits(got[0].cpu()[used]), _bits(other[0].cpu()[used])), what + " voxel_features"
    assert all(torch.equal(a, b) for a, b in zip(got[1:], other[1:])), what


@pytest.fixture(scope="module")
def refs():
    """name -> (points, offsets, range, voxel size, max_voxels, the restatement at T = 32), computed once and left unchanged"""
    out = {}
    for name, case, vs, mv in (("counts", c3.counts_case(), c3.VOXEL_SIZE, 105), ("cap", c3.cap_case(), c3.VOXEL_SIZE, c3.CAP_MAX_VOXELS),
                               ("full table", c3.full_table_case(), c3.VOXEL_SIZE, 2100), ("seams", c3.seam_case(), c3.VOXEL_SIZE, c3.SEAM_MAX_VOXELS)):
        pts, offs, rng = case
        out[name] = (pts, offs, rng, vs, mv, v3.voxelize_fast(pts, offs, rng, vs, 32, mv))
    return out


# ---------------------------------------------------------------------------------------------- 1. counts
@pytest.mark.parametrize("t", [32, 5])
def test_counts(cuda, refs, t):
    """3 x 5 x 7 cells, all populated (so every (y, x) column holds three voxels), 2 agents, about 2 800 shuffled points each: cells of
    exactly 1, 31, 32, 33, 64, 65 and 250 points"""
    pts, offs, rng, vs, mv, ref = refs["counts"]
    if t != 32:
        ref = v3.voxelize_fast(pts, offs, rng, vs, t, mv)
    counts = ref["cell_count"][ref["voxel_num_points"] > 0]
    for c in cv.COUNTS_REQUIRED:
        assert bool((counts == c).any()), c
    xy = {}
    for a, z, y, x in ref["voxel_coords"].tolist():
        xy.setdefault((a, y, x), set()).add(z)
    assert all(zs == {0, 1, 2} for zs in xy.values()) and int((counts > t).sum()) >= 16
    _check(_run(cuda, pts, offs, rng, vs, t, mv), ref, "counts T=%d" % t)


# ---------------------------------------------------------------------------------------------- 2. the voxel cap
def test_max_voxels_cap(cuda, refs):
    pts, offs, rng, vs, mv, ref = refs["cap"]
    assert [len(d) for d in ref["dropped_cells"]] == [60, 0, 20] and ref["num_voxels"].tolist() == [mv, mv, mv] and c3.CAP_CELLS[1] == mv
    # a dropped cell has points later in the input than points of a kept cell, and a kept cell goes on accepting points after a
    # dropped cell's first point (spconv's `continue`)
    keep, zs, ys, xs = v3.classify(pts, rng, vs)
    idx = np.arange(offs[0], offs[1])
    dropped = np.array([(int(zs[i]), int(ys[i]), int(xs[i])) in ref["dropped_cells"][0] for i in idx])
    assert idx[dropped].max() > idx[~dropped].min() and idx[~dropped].max() > idx[dropped].min()
    # none of a dropped cell's points is anywhere in the output (their intensities are no kept point's)
    lost = torch.from_numpy(pts[idx[dropped]][:, 3])
    used = torch.from_numpy(ref["voxel_num_points"] > 0)
    assert len(lost) > 100 and not bool(torch.isin(torch.from_numpy(ref["voxel_features"])[used][..., 3], lost).any())
    got = _run(cuda, pts, offs, rng, vs, 32, mv)
    _check(got, ref, "cap")
    assert not bool(torch.isin(got[0].cpu()[used][..., 3], lost).any())


# ---------------------------------------------------------------------------------------------- 3. probe chains and wrap-around
@pytest.mark.parametrize("name", ["counts", "cap", "full table"])
def test_smallest_table(cuda, refs, name):
    """the smallest table the operator takes (the power of two above M): long probe sequences that run over the table's end - at
    M = 2^12 - 1 points in as many cells, a load of 0.9998 - against the restatement and, bit for bit, against the default table"""
    pts, offs, rng, vs, mv, ref = refs[name]
    slots = c3.table_above(len(pts))
    assert slots // 2 <= len(pts) < slots < ops.voxelize3d_table_slots(len(pts))
    small = _run(cuda, pts, offs, rng, vs, 32, mv, table_slots=slots)
    _check(small, ref, name + " smallest table")
    _check_same(small, _run(cuda, pts, offs, rng, vs, 32, mv), ref, name)
    with pytest.raises(CobevtHipError, match="table_slots"):
        _run(cuda, pts, offs, rng, vs, 32, mv, table_slots=slots // 2)


# ---------------------------------------------------------------------------------------------- 4. same cells in different agents
def test_same_cells_in_three_agents(cuda):
    pts, offs, rng = c3.same_cells_case()
    ref = v3.voxelize_fast(pts, offs, rng, c3.VOXEL_SIZE, 32, 105)
    assert ref["num_voxels"].tolist() == [105] * 3 and np.array_equal(ref["voxel_coords"][:105, 1:], ref["voxel_coords"][210:, 1:])
    got = _run(cuda, pts, offs, rng, c3.VOXEL_SIZE, 32, 105)
    _check(got, ref, "same cells")
    vf = got[0].cpu()
    assert torch.equal(_bits(vf[:105]), _bits(vf[105:210])) and torch.equal(_bits(vf[:105]), _bits(vf[210:]))


# ---------------------------------------------------------------------------------------------- 5. keys past 32 bits
def test_keys_past_32_bits(cuda):
    """the backbone's grid (1408, 1600, 41) with 48 agents - 4.4e9 cells, keys up to 2^32.05 - and about 300 points per agent: the
    workspace, and with it the work, is that of the small cases"""
    pts, offs, rng = c3.big_case()
    nz, ny, nx = c3.BIG_GRID
    mv = c3.BIG_MAX_VOXELS
    ref = v3.voxelize_fast(pts, offs, rng, c3.BIG_VOXEL_SIZE, 32, mv)
    rows = ref["voxel_coords"].tolist()
    for a in (0, c3.BIG_AGENTS - 1):
        assert [a, 0, 0, 0] in rows and [a, nz - 1, ny - 1, nx - 1] in rows
    assert c3.BIG_AGENTS * nx * ny * nz > 2 ** 32 and bool((ref["num_voxels"] == mv).all())
    assert ops.voxelize3d_workspace_ints(len(pts), c3.BIG_AGENTS, 32, mv) < 300000
    _check(_run(cuda, pts, offs, rng, c3.BIG_VOXEL_SIZE, 32, mv), ref, "big grid")


# ---------------------------------------------------------------------------------------------- 6. edges
@pytest.mark.parametrize("range_mask,ego_mask", [(False, False), (True, False), (False, True), (True, True)])
def test_edges(cuda, range_mask, ego_mask):
    """cases_voxel's edge cloud (points on every range face and ego-box edge, NaN / inf coordinates, points on lo, hi and interior cell
    edges of x and y) on 40 cells over the height, + z values whose cell a reciprocal multiply would get wrong; voxel 0.4 x 0.4 x 0.1"""
    pts, offs, rng, sz = c3.edge_case()
    vs = c3.EDGE_VOXEL_SIZE
    assert len(sz) >= 3 and all(bool((pts[:, 2] == z).any()) for z in sz)
    assert bool((pts[:, 2] == np.float32(rng[2])).any()) and bool((pts[:, 2] == np.float32(rng[5])).any())
    ref = v3.voxelize_fast(pts, offs, rng, vs, 32, 2000, range_mask, ego_mask)
    plain = v3.voxelize_fast(pts, offs, rng, vs, 32, 2000)
    if range_mask or ego_mask:
        assert int(ref["voxel_num_points"].sum()) < int(plain["voxel_num_points"].sum())
    live = plain["voxel_coords"][plain["voxel_num_points"] > 0]
    assert bool((live[:, 1] == 0).any()) and bool((live[:, 1] == 39).any()) and bool((live[:, 3] == 0).any()) and int(live[:, 1:].min()) == 0
    assert int(ref["num_voxels"].max()) < 2000
    _check(_run(cuda, pts, offs, rng, vs, 32, 2000, range_mask=range_mask, ego_mask=ego_mask), ref, "edges")


# ---------------------------------------------------------------------------------------------- 7. scan seams
def test_scan_seams(cuda, refs):
    """70 000 points (more than 256 x 256) on 5 x 24 x 24 cells; the agents' boundary at 33 333, one agent without points"""
    pts, offs, rng, vs, mv, ref = refs["seams"]
    assert len(pts) == 70000 and offs.tolist() == cv.SEAM_OFFSETS and offs[1] % 1024 != 0 and offs[1] == offs[2]
    assert ref["num_voxels"].tolist()[1] == 0 and 2000 < ref["num_voxels"][0] < mv and 2000 < ref["num_voxels"][2] < mv
    _check(_run(cuda, pts, offs, rng, vs, 32, mv), ref, "seams")


def test_no_points(cuda):
    pts, offs = np.zeros((0, 4), dtype=np.float32), np.zeros(3, dtype=np.int32)
    rng = c3.lidar_range(c3.SEAM_GRID)
    ref = v3.voxelize(pts, offs, rng, c3.VOXEL_SIZE, 32, 20)
    assert ref["num_voxels"].tolist() == [0, 0] and bool((ref["voxel_coords"][:, 0] == -1).all())
    _check(_run(cuda, pts, offs, rng, c3.VOXEL_SIZE, 32, 20), ref, "M = 0")
    _check(_run(cuda, pts, offs, rng, c3.VOXEL_SIZE, 32, 20, table_slots=1), ref, "M = 0, one slot")


def test_rows_past_the_last_offset_are_ignored(cuda, refs):
    """offsets[N] < M: the tail rows hold valid points with a marker intensity; none of them reaches the output"""
    pts, offs, rng, vs, mv, _ = refs["seams"]
    pts, offs = pts.copy(), offs.copy()
    offs[3] = 60001
    pts[60001:, 3] = 777.0
    ref = v3.voxelize_fast(pts, offs, rng, vs, 32, mv)
    keep, _, _, _ = v3.classify(pts[60001:], rng, vs)
    assert bool(keep.all()) and not bool((ref["voxel_features"][..., 3] == 777.0).any())
    got = _run(cuda, pts, offs, rng, vs, 32, mv)
    _check(got, ref, "tail")
    used = torch.from_numpy(ref["voxel_num_points"] > 0)
    assert not bool((got[0].cpu()[used][..., 3] == 777.0).any())


# ---------------------------------------------------------------------------------------------- 8. the 2-D operator
@pytest.mark.parametrize("name", ["counts", "cap", "seams", "edges"])
def test_one_cell_over_the_height_equals_the_2d_operator(cuda, name):
    pts, offs, rng = {"counts": cv.counts_case, "cap": cv.cap_case, "seams": cv.seam_case, "edges": lambda: cv.edge_case()[:3]}[name]()
    mv = {"counts": 35, "cap": cv.CAP_MAX_VOXELS, "seams": 600, "edges": 700}[name]
    masks = name == "edges"
    assert vr.grid_size(rng, cv.VOXEL_SIZE)[2] == 1
    p, o = _dev(pts, offs, cuda)
    flat = ops.voxelize_points(p, o, rng, cv.VOXEL_SIZE, 32, mv, range_mask=masks, ego_mask=masks)
    deep = ops.voxelize_points_3d(p, o, rng, cv.VOXEL_SIZE, 32, mv, range_mask=masks, ego_mask=masks)
    torch.cuda.synchronize()
    used = flat[2].cpu() > 0
    assert int(used.sum()) > 30 and int(flat[3].sum()) == int(used.sum())
    assert torch.equal(_bits(flat[0].cpu()[used]), _bits(deep[0].cpu()[used]))
    assert all(torch.equal(a, b) for a, b in zip(flat[1:], deep[1:]))


# ---------------------------------------------------------------------------------------------- 9. reproducibility and bounds
def test_determinism_and_bounds(cuda, refs):
    """three runs are bit-identical; outputs and workspace are the interiors of larger buffers whose margins keep a marker; the
    features of rows without a voxel stay exactly as the caller filled them"""
    pts, offs, rng, vs, _, _ = refs["counts"]
    t, mv, margin = 32, 120, 256
    ref = v3.voxelize_fast(pts, offs, rng, vs, t, mv)
    assert int((ref["voxel_num_points"] == 0).sum()) == 2 * (mv - 105)
    p, o = _dev(pts, offs, cuda)
    ws_ints = ops.voxelize3d_workspace_ints(len(pts), 2, t, mv)
    shapes = [((2 * mv, t, 4), torch.float32, 7.0), ((2 * mv, 4), torch.int32, 77), ((2 * mv,), torch.int32, 77), ((2,), torch.int32, 77)]
    runs = []
    for _ in range(3):
        bigs, outs = [], []
        for shape, dtype, mark in shapes:
            n = int(np.prod(shape))
            big = torch.full((n + 2 * margin,), mark, device=cuda, dtype=dtype)
            bigs.append((big, n, mark))
            outs.append(big[margin:margin + n].view(shape))
        big_ws = torch.full((ws_ints + 2 * margin,), 77, device=cuda, dtype=torch.int32)
        got = ops.voxelize_points_3d(p, o, rng, vs, t, mv, out=outs, workspace=big_ws[margin:margin + ws_ints])
        torch.cuda.synchronize()
        assert all(g.data_ptr() == w.data_ptr() for g, w in zip(got, outs))
        _check(got, ref, "bounds")
        for big, n, mark in bigs:
            assert bool((big[:margin] == mark).all()) and bool((big[margin + n:] == mark).all())
        assert bool((big_ws[:margin] == 77).all()) and bool((big_ws[margin + ws_ints:] == 77).all())
        unused = torch.from_numpy(ref["voxel_num_points"] == 0)
        assert bool((got[0].cpu()[unused] == 7.0).all())
        runs.append([g.cpu() for g in got])
    for other in runs[1:]:
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(runs[0], other))       # whole buffers, the sentinel rows included
    # a workspace off the 8-byte boundary, or too small, is refused
    with pytest.raises(CobevtHipError, match="8-byte"):
        ops.voxelize_points_3d(p, o, rng, vs, t, mv, workspace=big_ws[margin + 1:margin + 1 + ws_ints])
    with pytest.raises(CobevtHipError, match="at least %d" % ws_ints):
        ops.voxelize_points_3d(p, o, rng, vs, t, mv, workspace=big_ws[:ws_ints - 1])


# ---------------------------------------------------------------------------------------------- 10. from points to the encoder
ENC_GRID = sr.GRIDS[0]
ENC_MAX_VOXELS = 512
ENC_POINTS = 6000


def _encoder_clouds():
    """two clouds of different sizes on sparse_ref's first grid, in a buffer of ENC_POINTS rows (the tail: valid points past offsets[N])"""
    sets = []
    for tag, seed in (("enc.a", sr.SEEDS[ENC_GRID]), ("enc.b", sr.SEEDS[ENC_GRID] + 3)):
        pts, offs = c3.encoder_cloud(tag, sr.clustered_coords(ENC_GRID, 2, seed), ENC_GRID, 2)
        assert len(pts) < ENC_POINTS
        sets.append((np.concatenate([pts, np.full((ENC_POINTS - len(pts), 4), 0.1, dtype=np.float32)]), offs))
    assert sets[0][1][-1] != sets[1][1][-1]
    return sets


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_from_points_to_the_encoder(cuda, mode):
    """SpVoxelPreprocessor3D -> MeanVFE -> VoxelBackBone8x -> HeightCompression, eagerly and as ONE captured graph replayed on a second
    cloud of another size, against the same modules fed the restatement's voxel dict: bit-equal"""
    nx, ny, nz = ENC_GRID
    rng, vs = c3.encoder_range(ENC_GRID), c3.ENCODER_VOXEL_SIZE
    prm = {"core_method": "SpVoxelPreprocessor3D", "cav_lidar_range": rng,
           "args": {"voxel_size": vs, "max_points_per_voxel": 5, "max_voxel_train": ENC_MAX_VOXELS, "max_voxel_test": ENC_MAX_VOXELS}}
    pre = host.SpVoxelPreprocessor3D(prm, train=False)
    assert tuple(pre.grid_size) == ENC_GRID
    vfe = host.MeanVFE({}, 4).eval()
    backbone = fill_module_(host.VoxelBackBone8x({}, 4, list(pre.grid_size)), 0).eval().to(cuda)
    to_bev = host.HeightCompression({"feature_num": 128 * sr.shape_chain(ENC_GRID)[-1][0]}).eval()
    sets = _encoder_clouds()
    want = []
    with torch.no_grad(), host.compute_dtype(mode):
        for pts, offs in sets:
            ref = v3.voxelize_fast(pts, offs, rng, vs, 5, ENC_MAX_VOXELS)
            assert bool((ref["cell_count"] > 5).any()) and 100 < int(ref["num_voxels"].min()) and int(ref["num_voxels"].max()) < ENC_MAX_VOXELS
            batch = {k: torch.from_numpy(ref[k]).to(cuda) for k in ("voxel_features", "voxel_coords", "voxel_num_points")}
            batch["batch_size"] = 2
            want.append((to_bev(backbone(vfe(batch)))["spatial_features"].clone(), torch.from_numpy(ref["num_voxels"])))
        assert float(want[0][0].float().abs().max()) > 0 and not torch.equal(want[0][0], want[1][0])
        p, o = _dev(*sets[0], cuda)

        def run():
            batch = pre.preprocess_batch(p, o)
            assert batch["batch_size"] == 2
            return to_bev(backbone(vfe(batch)))

        eager = run()
        torch.cuda.synchronize()
        assert torch.equal(eager["spatial_features"], want[0][0]) and torch.equal(eager["num_voxels"].cpu(), want[0][1])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = run()
        for i in (0, 1, 0):
            p.copy_(torch.from_numpy(sets[i][0]))
            o.copy_(torch.from_numpy(sets[i][1]))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out["spatial_features"], want[i][0]) and torch.equal(out["num_voxels"].cpu(), want[i][1]), i
