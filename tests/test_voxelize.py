"""The voxeliser (ops.voxelize_points, host.SpVoxelPreprocessor, PointPillarFuseBEVT fed raw points) without a GPU: the test-side
restatement tests/voxel_ref.py against the reference's point masks (fixture gv23) and against a hand-written example, its vectorised
form against the literal loop, and the error paths of the host classes."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import cases_pillar as cp
import cases_voxel as cv
import voxel_ref as vr
from cobevt_amd import host, lib, ops
from cobevt_amd.lib import CobevtHipError
from cobevt_amd.synth import fill_module_
from util import golden

KEYS = ("voxel_features", "voxel_coords", "voxel_num_points", "num_voxels", "cell_count")


def test_drop_predicates_equal_the_reference_masks():
    """mask_points_by_range / mask_ego_points of the reference on the golden cloud, points exactly on every face and edge included"""
    fx = golden("gv23_voxel")
    pts = cv.golden_cloud()
    rng = cv.lidar_range(*cv.GOLDEN_GRID)
    assert len(pts) == int(fx["points"])
    for axis in range(3):
        for bound in (rng[axis], rng[3 + axis]):
            assert bool((pts[:, axis] == np.float32(bound)).any())
    for axis, edges in ((0, cv.EGO_EDGES[:2]), (1, cv.EGO_EDGES[2:])):
        for e in edges:
            assert bool((pts[:, axis] == np.float32(e)).any())
    assert np.array_equal(vr.range_keep(pts, rng), fx["range_keep"])
    assert np.array_equal(vr.ego_keep(pts), fx["ego_keep"])
    # through classify: the masks come on top of the cell test (a point strictly below hi can still divide to the cell index n)
    cell_keep, _, _ = vr.classify(pts, rng, cv.VOXEL_SIZE)
    keep, _, _ = vr.classify(pts, rng, cv.VOXEL_SIZE, range_mask=True, ego_mask=True)
    assert np.array_equal(keep, fx["range_keep"] & fx["ego_keep"] & cell_keep)
    assert int((fx["range_keep"] & ~cell_keep).sum()) <= 3 and not bool((cell_keep & ~fx["range_keep"] & (np.abs(pts[:, :2]).max(1) < 6.3)
                                                                          & (pts[:, 2] > -2.9) & (pts[:, 2] < 0.9)).any())
    # the cell test alone keeps the points on lo and drops those on hi
    interior = (np.abs(pts[:, 1]) < 6) & (pts[:, 2] > -2.9) & (pts[:, 2] < 0.9)
    on_lo, on_hi = pts[:, 0] == np.float32(rng[0]), pts[:, 0] == np.float32(rng[3])
    assert bool((on_lo & interior).any()) and bool(cell_keep[on_lo & interior].all()) and not bool(fx["range_keep"][on_lo].any())
    assert bool(on_hi.any()) and not bool(cell_keep[on_hi].any())


def _hand_example():
    nan = float("nan")
    xy = [(0.5, 0.5), (1.5, 0.5), (0.2, 0.3), (0.5, 1.5), (0.7, 0.1), (nan, 0.5), (2.0, 0.5), (0.0, 0.0),
          (1.5, 1.5), (1.0, 0.9), (0.5, 1.2), (1.1, 0.1)]
    pts = np.array([[x, y, 0.5, 0.1 * (i + 1)] for i, (x, y) in enumerate(xy)], dtype=np.float32)
    return pts, [0, 8, 12], [0.0, 0.0, 0.0, 2.0, 2.0, 1.0], [1.0, 1.0, 1.0]


@pytest.mark.parametrize("fn", [vr.voxelize, vr.voxelize_fast])
def test_hand_written_example(fn):
    """12 points, 2 x 2 cells, T = 2, max_voxels = 2, two agents (points 0-7 and 8-11).
    agent 0: point 0 opens (y 0, x 0), 1 opens (0, 1), 2 joins (0, 0), 3 would open (1, 0) - third voxel, dropped -, 4 is the third point
    of (0, 0) - past T -, 5 has a NaN, 6 sits on x = hi, 7 sits on lo and is the fourth point of (0, 0).
    agent 1: 8 opens (1, 1), 9 sits on the interior edge x = 1 and opens (0, 1), 10 would open (1, 0) - dropped -, 11 joins (0, 1)."""
    pts, offs, rng, vs = _hand_example()
    out = fn(pts, offs, rng, vs, 2, 2)
    z = np.zeros(4, dtype=np.float32)
    assert out["num_voxels"].tolist() == [2, 2]
    assert out["voxel_coords"].tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [1, 0, 1, 1], [1, 0, 0, 1]]
    assert out["voxel_num_points"].tolist() == [2, 1, 1, 2]
    assert np.array_equal(out["voxel_features"], np.array([[pts[0], pts[2]], [pts[1], z], [pts[8], z], [pts[9], pts[11]]]))
    assert out["cell_count"].tolist() == [4, 1, 1, 2]
    assert out["dropped_cells"] == [{(1, 0)}, {(1, 0)}]
    # a cap of 3: agent 0 has an unused row, marked as the front end's padding rows are
    out = fn(pts, offs, rng, vs, 2, 3)
    assert out["num_voxels"].tolist() == [3, 3]
    out = fn(pts, offs, rng, vs, 2, 4)
    assert out["num_voxels"].tolist() == [3, 3] and out["voxel_coords"][3].tolist() == [-1, 0, 0, 0] and out["voxel_num_points"][3] == 0


@pytest.mark.parametrize("t", [32, 5])
def test_vectorised_restatement_equals_the_loop(t):
    """voxelize_fast (the full-size GPU test's yardstick) against the literal loop on the counts, cap and edge clouds"""
    for (pts, offs, rng), mv, masks in ((cv.counts_case(), 35, False), (cv.cap_case(), cv.CAP_MAX_VOXELS, False),
                                        (cv.edge_case()[:3], 700, True)):
        a = vr.voxelize(pts, offs, rng, cv.VOXEL_SIZE, t, mv, masks, masks)
        b = vr.voxelize_fast(pts, offs, rng, cv.VOXEL_SIZE, t, mv, masks, masks)
        for k in KEYS:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert a["dropped_cells"] == b["dropped_cells"]
        assert int(a["num_voxels"].sum()) > 0


def test_grid_size_and_preprocessor_contract():
    pre = host.SpVoxelPreprocessor(cv.preprocess_params((5, 7), 32, 11, 13), train=True)
    assert tuple(pre.grid_size) == (7, 5, 1) == vr.grid_size(cv.lidar_range(5, 7), cv.VOXEL_SIZE) == ops.voxel_grid_size(cv.lidar_range(5, 7), cv.VOXEL_SIZE)
    assert pre.max_voxels == 11 and pre.max_points_per_voxel == 32
    assert host.SpVoxelPreprocessor(cv.preprocess_params((5, 7), 32, 11, 13), train=False).max_voxels == 13
    assert not isinstance(pre, torch.nn.Module)


def test_preprocessor_error_paths():
    prm = cv.preprocess_params((16, 16))
    bad = copy.deepcopy(prm); bad["args"]["voxel_size"] = [0.4, 0.4, 2]                                   # noqa: E702
    with pytest.raises(CobevtHipError, match="nz = 1"):
        host.SpVoxelPreprocessor(bad, False)
    bad = copy.deepcopy(prm); bad["args"]["max_points_per_voxel"] = 33                                    # noqa: E702
    with pytest.raises(CobevtHipError, match="T = 32"):
        host.SpVoxelPreprocessor(bad, False)
    pre = host.SpVoxelPreprocessor(prm, False)
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        pre.preprocess_batch(torch.zeros(10, 4), torch.tensor([0, 10], dtype=torch.int32))
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        ops.voxelize_points(torch.zeros(10, 4), torch.tensor([0, 10], dtype=torch.int32), prm["cav_lidar_range"], cv.VOXEL_SIZE, 32, 8)


def _args(**pre_kw):
    a = cp.model_args()
    a["preprocess"] = cv.preprocess_params(cp.GRID, **pre_kw)
    return a


def test_model_error_paths():
    a = _args(); a["preprocess"]["cav_lidar_range"] = cv.lidar_range(16, 20)                              # noqa: E702
    with pytest.raises(CobevtHipError, match="grid"):
        host.PointPillarFuseBEVT(a)
    a = _args(); a["preprocess"]["args"]["voxel_size"] = [0.4, 0.4, 2]                                    # noqa: E702
    with pytest.raises(CobevtHipError, match="nz = 1"):
        host.PointPillarFuseBEVT(a)
    with pytest.raises(CobevtHipError, match="T = 32"):
        host.PointPillarFuseBEVT(_args(max_points=64))
    batch = {"lidar_points": torch.zeros(10, 4), "lidar_point_offsets": torch.tensor([0, 4, 7, 10], dtype=torch.int32),
             "record_len": torch.tensor(cp.RECORD_LEN)}
    plain = fill_module_(host.PointPillarFuseBEVT(cp.model_args()), cp.SEED).eval()
    with pytest.raises(CobevtHipError, match="preprocess"):
        plain(batch)
    m = fill_module_(host.PointPillarFuseBEVT(_args()), cp.SEED).eval()
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        m(batch)
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        m.train()(batch)
    with pytest.raises(CobevtHipError, match="neither processed_lidar nor lidar_points"):
        m({"record_len": torch.tensor(cp.RECORD_LEN)})


def test_state_dict_is_the_same_with_and_without_preprocess():
    a = fill_module_(host.PointPillarFuseBEVT(cp.model_args()), cp.SEED).state_dict()
    b = fill_module_(host.PointPillarFuseBEVT(_args()), cp.SEED).state_dict()
    assert list(a.keys()) == list(b.keys())
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_c_abi_validates_arguments_before_any_launch():
    """cobevt_voxelize_scratch / cobevt_voxelize_points reject null pointers (COBEVT_ERR_ARG = 1) and unsupported shapes, ranges and
    alignments (COBEVT_ERR_SHAPE = 2) without touching a device"""
    l = lib.load()

    def dims(m=10, n=1, t=32, mv=4, nx=2, ny=2, nz=1):
        return (ctypes.c_long * 9)(m, n, t, mv, nx, ny, nz, 0, 0)
    need = ctypes.c_long(0)
    assert l.cobevt_voxelize_scratch(dims(), ctypes.byref(need)) == 0
    assert need.value == 4 * 4 + 4 + 2 * 10 + 2 * 2 + 2 == ops.voxelize_workspace_ints(10, 1, (2, 2, 1), 32, 4)
    assert l.cobevt_voxelize_scratch(None, ctypes.byref(need)) == 1 and l.cobevt_voxelize_scratch(dims(), None) == 1
    for bad in (dims(t=33), dims(t=0), dims(nz=2), dims(m=-1), dims(m=2 ** 31), dims(mv=0), dims(n=0), dims(nx=0),
                dims(nx=2 ** 20, ny=2 ** 20), dims(n=1000, mv=2 ** 30)):
        assert l.cobevt_voxelize_scratch(bad, ctypes.byref(need)) == 2, list(bad)
    geom = (ctypes.c_float * 9)(0, 0, 0, 2, 2, 1, 1, 1, 1)
    buf = (ctypes.c_float * 64)()                               # host memory: only its address is looked at
    base = (ctypes.addressof(buf) + 15) & ~15
    ptr = ctypes.c_void_p(base)
    assert l.cobevt_voxelize_points(None, None, None, None, None, None, None, dims(), geom, None) == 1
    assert l.cobevt_voxelize_points(ptr, ptr, ptr, ptr, ptr, ptr, ptr, None, geom, None) == 1
    assert l.cobevt_voxelize_points(ptr, ptr, ptr, ptr, ptr, ptr, ptr, dims(), None, None) == 1
    assert l.cobevt_voxelize_points(None, ptr, ptr, ptr, ptr, ptr, ptr, dims(), geom, None) == 1           # M > 0 without points
    assert l.cobevt_voxelize_points(ptr, ptr, ptr, ptr, ptr, ptr, ptr, dims(t=33), geom, None) == 2
    assert l.cobevt_voxelize_points(ptr, ptr, ptr, ptr, ptr, ptr, ptr, dims(nz=2), geom, None) == 2
    off = ctypes.c_void_p(base + 4)
    assert l.cobevt_voxelize_points(off, ptr, ptr, ptr, ptr, ptr, ptr, dims(), geom, None) == 2              # points not 16-byte aligned
    assert l.cobevt_voxelize_points(ptr, ptr, off, ptr, ptr, ptr, ptr, dims(), geom, None) == 2              # voxel_features
    zero = (ctypes.c_float * 9)(0, 0, 0, 2, 2, 1, 1, 0, 1)
    assert l.cobevt_voxelize_points(ptr, ptr, ptr, ptr, ptr, ptr, ptr, dims(), zero, None) == 2              # voxel size 0
