"""The 3-D voxeliser (ops.voxelize_points_3d, host.SpVoxelPreprocessor3D) without a GPU: the test-side restatement
tests/voxel3d_ref.py - its vectorised form against the literal loop, both against a hand-written example and, on nz = 1 grids, against
voxel_ref.py -, the conditions the GPU cases rely on, the error paths of the host layer and the argument checks of the C entry points."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import cases_voxel as cv
import cases_voxel3d as c3
import voxel3d_ref as v3
import voxel_ref as vr
from cobevt_amd import host, lib, ops, registry
from cobevt_amd.lib import CobevtHipError

KEYS = ("voxel_features", "voxel_coords", "voxel_num_points", "num_voxels", "cell_count")


def _same(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _cases():
    """(name, points, offsets, range, voxel size, max_voxels, masks): every cloud of the GPU file"""
    edge = c3.edge_case()
    return [("counts", *c3.counts_case(), c3.VOXEL_SIZE, 105, False), ("cap", *c3.cap_case(), c3.VOXEL_SIZE, c3.CAP_MAX_VOXELS, False),
            ("full table", *c3.full_table_case(), c3.VOXEL_SIZE, 2100, False), ("same cells", *c3.same_cells_case(), c3.VOXEL_SIZE, 105, False),
            ("big", *c3.big_case(), c3.BIG_VOXEL_SIZE, c3.BIG_MAX_VOXELS, False), ("edges", *edge[:3], c3.EDGE_VOXEL_SIZE, 2000, True),
            ("seams", *c3.seam_case(), c3.VOXEL_SIZE, c3.SEAM_MAX_VOXELS, False)]


@pytest.mark.parametrize("t", [32, 5])
def test_vectorised_restatement_equals_the_loop(t):
    for name, pts, offs, rng, vs, mv, masks in _cases():
        if name == "seams" and t == 5:
            continue                                                  # 70 000 points through the loop: once
        a = v3.voxelize(pts, offs, rng, vs, t, mv, masks, masks)
        b = v3.voxelize_fast(pts, offs, rng, vs, t, mv, masks, masks)
        _same(a, b)
        assert a["dropped_cells"] == b["dropped_cells"], name
        assert int(a["num_voxels"].sum()) > 0, name


def _hand_example():
    nan = float("nan")
    xyz = [(0.5, 0.5, 0.5), (0.5, 0.5, 1.5), (0.2, 0.3, 0.9), (1.5, 0.5, 0.5), (0.7, 0.1, 1.0), (0.5, 0.5, nan), (0.5, 0.5, 2.0),
           (0.0, 0.0, 0.0), (0.6, 0.6, 1.1),
           (1.5, 1.5, 1.5), (1.5, 1.5, 0.5), (1.0, 1.0, 1.0), (0.5, 1.2, 0.5), (1.9, 1.9, 0.1)]
    pts = np.array([[x, y, z, 0.1 * (i + 1)] for i, (x, y, z) in enumerate(xyz)], dtype=np.float32)
    return pts, [0, 9, 14], [0.0, 0.0, 0.0, 2.0, 2.0, 2.0], [1.0, 1.0, 1.0]


@pytest.mark.parametrize("fn", [v3.voxelize, v3.voxelize_fast])
def test_hand_written_example(fn):
    """14 points, 2 x 2 x 2 cells, T = 2, max_voxels = 3, two agents (points 0-8 and 9-13).
    agent 0: point 0 opens (z 0, y 0, x 0); 1 has the same (x, y) and z = 1.5: it opens (1, 0, 0); 2 joins (0, 0, 0); 3 opens (0, 0, 1);
    4 sits on the interior face z = 1 and joins (1, 0, 0); 5 has a NaN z; 6 sits on z = hi; 7 sits on lo and is the third point of
    (0, 0, 0) - past T; 8 is the third point of (1, 0, 0) - past T.
    agent 1: 9 opens (1, 1, 1), 10 - same (x, y) - opens (0, 1, 1), 11 sits on three interior faces and joins (1, 1, 1), 12 would open
    (0, 1, 0) ... and does, as the third voxel; 13 joins (0, 1, 1)."""
    pts, offs, rng, vs = _hand_example()
    assert vr.grid_size(rng, vs) == (2, 2, 2)
    out = fn(pts, offs, rng, vs, 2, 3)
    z = np.zeros(4, dtype=np.float32)
    assert out["num_voxels"].tolist() == [3, 3]
    assert out["voxel_coords"].tolist() == [[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [1, 1, 1, 1], [1, 0, 1, 1], [1, 0, 1, 0]]
    assert out["voxel_num_points"].tolist() == [2, 2, 1, 2, 2, 1]
    assert np.array_equal(out["voxel_features"], np.array([[pts[0], pts[2]], [pts[1], pts[4]], [pts[3], z],
                                                           [pts[9], pts[11]], [pts[10], pts[13]], [pts[12], z]]))
    assert out["cell_count"].tolist() == [3, 3, 1, 2, 2, 1]
    assert out["dropped_cells"] == [set(), set()]
    # a cap of 2: the third cell of either agent is dropped with its points, the open cells go on accepting theirs
    out = fn(pts, offs, rng, vs, 2, 2)
    assert out["num_voxels"].tolist() == [2, 2] and out["dropped_cells"] == [{(0, 0, 1)}, {(0, 1, 0)}]
    assert out["voxel_coords"].tolist() == [[0, 0, 0, 0], [0, 1, 0, 0], [1, 1, 1, 1], [1, 0, 1, 1]]
    assert out["cell_count"].tolist() == [3, 3, 2, 2]
    # a cap of 4: an unused row per agent, marked as the padding rows are
    out = fn(pts, offs, rng, vs, 2, 4)
    assert out["num_voxels"].tolist() == [3, 3] and out["voxel_coords"][3].tolist() == [-1, 0, 0, 0] and out["voxel_num_points"][3] == 0


@pytest.mark.parametrize("t", [32, 5])
def test_on_one_cell_over_the_height_it_is_the_2d_restatement(t):
    for (pts, offs, rng), mv, masks in ((cv.counts_case(), 35, False), (cv.cap_case(), cv.CAP_MAX_VOXELS, False),
                                        (cv.edge_case()[:3], 700, True)):
        a = vr.voxelize(pts, offs, rng, cv.VOXEL_SIZE, t, mv, masks, masks)
        for fn in (v3.voxelize, v3.voxelize_fast):
            b = fn(pts, offs, rng, cv.VOXEL_SIZE, t, mv, masks, masks)
            _same(a, b)
            assert [{(y, x) for _, y, x in d} for d in b["dropped_cells"]] == a["dropped_cells"]
            assert not bool(b["voxel_coords"][:, 1].any())


def test_the_cases_hold_what_the_gpu_tests_rely_on():
    # counts: every required population, and cells that differ only in z
    pts, offs, rng = c3.counts_case()
    ref = v3.voxelize_fast(pts, offs, rng, c3.VOXEL_SIZE, 32, 105)
    assert vr.grid_size(rng, c3.VOXEL_SIZE) == (7, 5, 3) and ref["num_voxels"].tolist() == [105, 105]
    assert set(cv.COUNTS_REQUIRED) <= set(ref["cell_count"][:105].tolist()) and set(cv.COUNTS_REQUIRED) <= set(ref["cell_count"][105:].tolist())
    # the cap: two agents past it, one exactly at it
    pts, offs, rng = c3.cap_case()
    ref = v3.voxelize_fast(pts, offs, rng, c3.VOXEL_SIZE, 32, c3.CAP_MAX_VOXELS)
    assert vr.grid_size(rng, c3.VOXEL_SIZE) == (16, 16, 4) and ref["num_voxels"].tolist() == [40, 40, 40]
    assert [len(d) for d in ref["dropped_cells"]] == [60, 0, 20]
    # the full table: 2^12 - 1 points, as many cells
    pts, offs, rng = c3.full_table_case()
    ref = v3.voxelize_fast(pts, offs, rng, c3.VOXEL_SIZE, 32, 2100)
    assert len(pts) == 4095 and c3.table_above(len(pts)) == 4096 and ref["num_voxels"].tolist() == c3.FULL_TABLE_SIZES
    # keys past 32 bits: the lowest and the highest cell of the grid in the first and in the last agent, the cap in force
    pts, offs, rng = c3.big_case()
    nz, ny, nx = c3.BIG_GRID
    assert vr.grid_size(rng, c3.BIG_VOXEL_SIZE) == (nx, ny, nz) and c3.BIG_AGENTS * nx * ny * nz > 2 ** 32
    ref = v3.voxelize_fast(pts, offs, rng, c3.BIG_VOXEL_SIZE, 32, c3.BIG_MAX_VOXELS)
    rows = ref["voxel_coords"].tolist()
    for a in (0, c3.BIG_AGENTS - 1):
        assert [a, 0, 0, 0] in rows and [a, nz - 1, ny - 1, nx - 1] in rows
        assert (a * nz * ny * nx + nz * ny * nx - 1 >= 2 ** 32) == (a > 0)
    assert all(200 <= int(offs[a + 1] - offs[a]) <= 400 for a in range(c3.BIG_AGENTS))
    assert bool((ref["num_voxels"] == c3.BIG_MAX_VOXELS).all()) and all(len(d) > 0 for d in ref["dropped_cells"])
    # edges: z on lo is kept, z on hi dropped, and z values a reciprocal multiply would move to the next cell
    pts, offs, rng, sz = c3.edge_case()
    assert vr.grid_size(rng, c3.EDGE_VOXEL_SIZE) == (32, 32, 40) and len(sz) >= 3 and all(bool((pts[:, 2] == z).any()) for z in sz)
    v, lo = np.float32(c3.EDGE_VOXEL_SIZE[2]), np.float32(rng[2])
    assert bool((np.floor((sz - lo) / v) != np.floor((sz - lo) * (np.float32(1) / v))).all())
    keep, zs, _, _ = v3.classify(pts, rng, c3.EDGE_VOXEL_SIZE)
    inside = (np.abs(pts[:, :2]).max(1) < 6.0)
    on_lo, on_hi = (pts[:, 2] == np.float32(rng[2])) & inside, (pts[:, 2] == np.float32(rng[5])) & inside
    assert bool(on_lo.any()) and bool(keep[on_lo].all()) and bool(on_hi.any()) and not bool(keep[on_hi].any())
    assert bool((zs[keep] == 39).any()) and bool((zs[keep] == 0).any())


def test_preprocessor_contract_and_registry():
    prm = cv.preprocess_params((5, 7), 32, 11, 13)
    prm["args"]["voxel_size"] = list(c3.VOXEL_SIZE)
    prm["core_method"] = "SpVoxelPreprocessor3D"
    pre = registry.build_preprocessor(prm, train=True)
    assert type(pre) is host.SpVoxelPreprocessor3D and pre.train is True and pre.params is prm
    assert tuple(pre.grid_size) == (7, 5, 10) and pre.max_voxels == 11 and pre.max_points_per_voxel == 32
    assert host.SpVoxelPreprocessor3D(prm, train=False).max_voxels == 13
    assert not isinstance(pre, torch.nn.Module)
    # one cell over the height is as good as any other
    assert tuple(host.SpVoxelPreprocessor3D(cv.preprocess_params((5, 7)), False).grid_size) == (7, 5, 1)
    # the 2-D class goes on refusing this grid
    with pytest.raises(CobevtHipError, match="nz = 1"):
        host.SpVoxelPreprocessor(prm, False)


def test_error_paths(monkeypatch):
    prm = cv.preprocess_params((16, 16))
    prm["args"]["voxel_size"] = list(c3.VOXEL_SIZE)
    bad = copy.deepcopy(prm); bad["args"]["max_points_per_voxel"] = 33                                    # noqa: E702
    with pytest.raises(CobevtHipError, match="T = 32"):
        host.SpVoxelPreprocessor3D(bad, False)
    bad = copy.deepcopy(prm); bad["args"]["voxel_size"] = [0.4, 0.4, 9.0]                                 # noqa: E702
    with pytest.raises(CobevtHipError, match="empty grid"):
        host.SpVoxelPreprocessor3D(bad, False)
    pre = host.SpVoxelPreprocessor3D(prm, False)
    cpu = (torch.zeros(10, 4), torch.tensor([0, 10], dtype=torch.int32))
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        pre.preprocess_batch(*cpu)
    rng = prm["cav_lidar_range"]
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        ops.voxelize_points_3d(*cpu, rng, c3.VOXEL_SIZE, 32, 8)
    # the operator's own argument checks, with its device test switched off: whatever it raises on these comes from them
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)
    meta = (torch.zeros(10, 4, device="meta"), torch.tensor([0, 10], dtype=torch.int32, device="meta"))
    for kw, match in ((dict(max_points=33, max_voxels=8), "T = 32"), (dict(max_points=0, max_voxels=8), "T = 32"),
                      (dict(), "max_voxels"), (dict(max_voxels=0), "max_voxels")):
        with pytest.raises(CobevtHipError, match=match):
            ops.voxelize_points_3d(*meta, rng, c3.VOXEL_SIZE, **kw)
    with pytest.raises(CobevtHipError, match="empty grid"):
        ops.voxelize_points_3d(*meta, rng, [0.4, 0.4, 9.0], max_voxels=8)
    for slots in (3, 8, 10, 0, -16):
        with pytest.raises(CobevtHipError, match="table_slots"):
            ops.voxelize_points_3d(*cpu, rng, c3.VOXEL_SIZE, 32, 8, table_slots=slots)
    # ... and the 2-D operator goes on refusing this grid
    with pytest.raises(CobevtHipError, match="nz = 1"):
        ops.voxelize_points(*meta, rng, c3.VOXEL_SIZE, 32, 8)


def test_c_abi_validates_arguments_before_any_launch():
    """cobevt_voxelize3d_scratch / cobevt_voxelize3d_points reject null pointers (COBEVT_ERR_ARG = 1) and unsupported shapes, ranges,
    tables and alignments (COBEVT_ERR_SHAPE = 2) without touching a device"""
    l = lib.load()

    def dims(m=10, n=1, t=32, mv=4, nx=2, ny=2, nz=3, slots=0):
        return (ctypes.c_long * 10)(m, n, t, mv, nx, ny, nz, 0, 0, slots)
    need = ctypes.c_long(0)
    assert l.cobevt_voxelize3d_scratch(dims(), ctypes.byref(need)) == 0
    assert need.value == 6 * 64 + 4 + 2 * 10 + 2 * 2 + 2                                       # the default table's floor
    assert l.cobevt_voxelize3d_scratch(dims(slots=16), ctypes.byref(need)) == 0 and need.value == 6 * 16 + 4 + 2 * 10 + 2 * 2 + 2
    assert l.cobevt_voxelize3d_scratch(dims(m=1000), ctypes.byref(need)) == 0 and need.value == 6 * 2048 + 4 + 2 * 1000 + 2 * 2 + 2
    # the grid is not in it
    assert l.cobevt_voxelize3d_scratch(dims(m=1000, nx=1408, ny=1600, nz=41, n=48), ctypes.byref(need)) == 0
    assert need.value == 6 * 2048 + 48 * 4 + 2 * 1000 + 2 * 2 + 49
    assert l.cobevt_voxelize3d_scratch(None, ctypes.byref(need)) == 1 and l.cobevt_voxelize3d_scratch(dims(), None) == 1
    for bad in (dims(t=33), dims(t=0), dims(nz=0), dims(nz=-1), dims(m=-1), dims(m=2 ** 31), dims(mv=0), dims(n=0), dims(nx=0), dims(ny=0),
                dims(n=1000, mv=2 ** 30), dims(slots=3), dims(slots=10), dims(slots=8), dims(slots=-16), dims(slots=2 ** 32),
                dims(nx=2 ** 24 + 1), dims(nz=2 ** 25), dims(n=4, nx=2 ** 21, ny=2 ** 21, nz=2 ** 19)):
        assert l.cobevt_voxelize3d_scratch(bad, ctypes.byref(need)) == 2, list(bad)
    for good in (dims(slots=16), dims(m=15, slots=16), dims(n=4, nx=2 ** 20, ny=2 ** 20, nz=2 ** 20), dims(nz=1), dims(m=0, slots=1)):
        assert l.cobevt_voxelize3d_scratch(good, ctypes.byref(need)) == 0, list(good)
    assert l.cobevt_voxelize3d_scratch(dims(m=16, slots=16), ctypes.byref(need)) == 2                        # slots = M
    geom = (ctypes.c_float * 9)(0, 0, 0, 2, 2, 3, 1, 1, 1)
    buf = (ctypes.c_float * 64)()                               # host memory: only its address is looked at
    base = (ctypes.addressof(buf) + 15) & ~15
    ptr = ctypes.c_void_p(base)
    f = l.cobevt_voxelize3d_points
    assert f(None, None, None, None, None, None, None, dims(), geom, None) == 1
    for k in range(1, 7):                                       # each pointer on its own
        args = [ptr] * 7
        args[k] = None
        assert f(*args, dims(), geom, None) == 1, k
    assert f(ptr, ptr, ptr, ptr, ptr, ptr, ptr, None, geom, None) == 1
    assert f(ptr, ptr, ptr, ptr, ptr, ptr, ptr, dims(), None, None) == 1
    assert f(None, ptr, ptr, ptr, ptr, ptr, ptr, dims(), geom, None) == 1                                    # M > 0 without points
    for bad in (dims(t=33), dims(nz=0), dims(slots=3), dims(slots=10), dims(m=16, slots=16), dims(n=4, nx=2 ** 21, ny=2 ** 21, nz=2 ** 19)):
        assert f(ptr, ptr, ptr, ptr, ptr, ptr, ptr, bad, geom, None) == 2, list(bad)
    off = ctypes.c_void_p(base + 4)
    assert f(off, ptr, ptr, ptr, ptr, ptr, ptr, dims(), geom, None) == 2                                     # points not 16-byte aligned
    assert f(ptr, ptr, off, ptr, ptr, ptr, ptr, dims(), geom, None) == 2                                     # voxel_features
    assert f(ptr, ptr, ptr, off, ptr, ptr, ptr, dims(), geom, None) == 2                                     # voxel_coords
    assert f(ptr, ptr, ptr, ptr, ptr, ptr, off, dims(), geom, None) == 2                                     # workspace not 8-byte aligned
    for j in (6, 7, 8):
        g = [0, 0, 0, 2, 2, 3, 1, 1, 1]
        g[j] = 0
        assert f(ptr, ptr, ptr, ptr, ptr, ptr, ptr, dims(), (ctypes.c_float * 9)(*g), None) == 2             # voxel size 0
    g = (ctypes.c_float * 9)(0, 0, 0, 2, 2, 3, 1, 1, float("nan"))
    assert f(ptr, ptr, ptr, ptr, ptr, ptr, ptr, dims(), g, None) == 2


def test_the_2d_entry_points_keep_their_workspace_and_their_refusal():
    l = lib.load()
    need = ctypes.c_long(0)
    assert l.cobevt_voxelize_scratch((ctypes.c_long * 9)(10, 1, 32, 4, 2, 2, 1, 0, 0), ctypes.byref(need)) == 0
    assert need.value == 4 * 4 + 4 + 2 * 10 + 2 * 2 + 2
    assert l.cobevt_voxelize_scratch((ctypes.c_long * 9)(10, 1, 32, 4, 2, 2, 3, 0, 0), ctypes.byref(need)) == 2


@pytest.mark.parametrize("m,n,t,mv,slots", [(10, 1, 32, 4, None), (0, 2, 5, 20, None), (70000, 3, 32, 3000, None), (4095, 2, 32, 2100, 4096),
                                            (300 * 48, 48, 32, 64, None)])
def test_workspace_ints_is_what_the_scratch_call_returns(m, n, t, mv, slots):
    need = ctypes.c_long(0)
    dims = (ctypes.c_long * 10)(m, n, t, mv, 1408, 1600, 41, 1, 1, slots or 0)
    assert lib.load().cobevt_voxelize3d_scratch(dims, ctypes.byref(need)) == 0
    table = ops.voxelize3d_table_slots(m, slots)
    assert table == (slots or max(64, c3.table_above(2 * m - 1)))
    assert ops.voxelize3d_workspace_ints(m, n, t, mv, slots) == need.value == 6 * table + n * mv + 2 * m + 2 * ((m + 1023) // 1024 or 1) + 2 + n + 1


def test_the_workspace_size_follows_its_key_not_the_grid():
    """the default workspace is cached on (M, N, T, max_voxels, table): the grid, which the key leaves out, must not move the size"""
    m, n, t, mv, slots = 5000, 2, 32, 700, 16384
    sizes = [ops._scratch("cobevt_voxelize3d_scratch", ops._longs(m, n, t, mv, nx, ny, nz, 0, 0, slots)) for nx, ny, nz in ((16, 12, 1), (160, 120, 41))]
    assert sizes[0] == sizes[1] == ops.voxelize3d_workspace_ints(m, n, t, mv, slots)
    default = [ops._scratch("cobevt_voxelize3d_scratch", ops._longs(m, n, t, mv, nx, ny, nz, 0, 0, 0)) for nx, ny, nz in ((16, 12, 1), (160, 120, 41))]
    assert default[0] == default[1] == ops.voxelize3d_workspace_ints(m, n, t, mv)
