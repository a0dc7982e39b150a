"""ops.prepare_points / host.DataAugmentor without a device: the fixture gv29_cloud_prep.npz (the reference's own run, written by
tests/golden/make_golden_cloud.py) is reproduced by the restatement tests/cloud_ref.py, the seed replay of DataAugmentor.draw gives
the parameters the reference drew, the queue order decides the number of operator calls (launch traces), and the host layer
validates its arguments and refuses CPU tensors.

Gates.  Masks, flips, scaling, intensity, kept sets, offsets and box sizes / headings: exact.  Projected coordinates: equal after
rounding to fp32, except that at most 1e-4 of them may differ by one fp32 ulp (np.dot is BLAS-ordered); the generator stores the count.
Rotated coordinates: |ref - mine| <= 3 * 2^-24 * (|x c| + |y s|), resp. (|x s| + |y c|) - two product roundings and one sum rounding
in any fp32 evaluation order of the reference's matmul, plus the one rounding of the restatement, each at most 2^-24 of a term bounded
by that sum.  In the "all" case the rotation's inputs are projected coordinates: the bound holds there because the fixture records
that none of them differs from the restatement's (asserted with the gate).  Where a scaling follows, the bound is multiplied by the fp32
scale and nothing is added for the scaling's own rounding."""
import numpy as np
import pytest
import torch

import cases_cloud as cc
import cloud_ref as cr
import launch_trace as lt
import launch_trace_cloud_prep as ltc
from cobevt_amd import host, ops
from cobevt_amd.lib import CobevtHipError
from util import golden


@pytest.fixture(scope="module")
def gv():
    return golden("gv29_cloud_prep")


# ---------------------------------------------------------------------------------------------- the fixture against the restatement
@pytest.mark.parametrize("name", sorted(cc.GOLDEN))
def test_fixture(gv, name):
    case = cc.golden_case(name)
    out, out_offs, keep, boxes = cc.restated(case)
    cc.check_against_reference(gv, name, out, out_offs, boxes)
    if case["masks"]:
        pts, _ = cc.concat(case["clouds"])
        assert 0 < keep.sum() < len(pts)
        assert all(float(cc.margin(p, t, True, case["world"]).min()) >= cc.MARGIN for p, t in zip(case["clouds"], case["transforms"]))
        # each mask removes something
        only_ego = cr.prepare_points(pts, cc.concat(case["clouds"])[1], case["transforms"], ego_mask=True)[2]
        assert keep.sum() < only_ego.sum() < len(pts)
    assert sum(len(c) for c in case["clouds"]) <= 3100


def test_case_design():
    """what the cases are for: both flips on, a flip pattern that tells x from y, and edge points on every limit"""
    assert cc.draw("flips")[1] == {"flip_x": True, "flip_y": True}
    w = cc.draw("all")[1]
    assert w["flip_x"] and not w["flip_y"] and abs(w["rot"]) > 0.1 and abs(w["scale"] - 1) > 0.01
    p = cc.edge_points()
    lim = np.asarray(cc.LIDAR_RANGE, dtype=np.float64).astype(np.float32)
    assert all((p[:, j] == lim[j]).any() and (p[:, j] == lim[3 + j]).any() for j in range(3))
    assert all((p[:, 0] == v).any() for v in cr.EGO[:2]) and all((p[:, 1] == v).any() for v in cr.EGO[2:])
    keep = cr.prepare_points(p, [0, len(p)], ego_mask=True, lidar_range=cc.LIDAR_RANGE)[2]
    assert 0 < keep.sum() < len(p)
    # a NaN survives the ego mask and fails the range mask; on a limit: inside the ego box (closed), outside the range (open)
    assert cr.ego_keep(p)[np.isnan(p[:, 0])].all() and not keep[np.isnan(p[:, :3]).any(axis=1)].any()
    assert not cr.ego_keep(p)[(p[:, 0] == cr.EGO[0]) & (p[:, 1] == 0)].any()
    assert not cr.range_keep(p, cc.LIDAR_RANGE)[p[:, 0] == lim[3]].any()
    # the documented deviation: 140.7999999 is below 140.8 in fp64 and ON the fp32 limit
    assert 140.7999999 < 140.8 and np.float32(140.7999999) == lim[3] and not keep[-1]


# ---------------------------------------------------------------------------------------------- DataAugmentor on the host
@pytest.mark.parametrize("name", ["augmentor", "all"])
def test_draw_replays_the_reference(gv, name):
    seed, world, params = cc.draw(name)
    mine = host.DataAugmentor(cc.AUG_CONFIG).draw(np.random.RandomState(seed))
    assert mine == params
    flat = [float(on) for _, on in mine[0]] + [mine[1], mine[2]]
    assert np.array_equal(np.asarray(flat), gv[name + "_drawn"])
    np.random.seed(seed)                                  # the default generator is the reference's: the global one
    assert host.DataAugmentor(cc.AUG_CONFIG).draw() == params


def test_draw_rules():
    aug = host.DataAugmentor([{"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [1.0, 1.0005]},
                              {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": 0.5}])
    r = np.random.RandomState(3)
    p = aug.draw(r)
    assert p[0] is None and p[1] == np.random.RandomState(3).uniform(-0.5, 0.5)        # a narrow scale range draws nothing
    assert aug.worlds(p) == [{"scale": None}, {"rot": p[1]}]
    with pytest.raises(CobevtHipError, match="unknown augmentation"):
        host.DataAugmentor([{"NAME": "random_world_shear"}])
    with pytest.raises(CobevtHipError, match="ALONG_AXIS_LIST"):
        host.DataAugmentor([{"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["z"]}])
    with pytest.raises(CobevtHipError, match="params has"):
        aug.worlds([None])


def test_queue_order():
    aug = host.DataAugmentor(cc.AUG_CONFIG)
    assert aug.worlds([[("x", True), ("y", False)], 0.25, None]) == [{"flip_x": True, "flip_y": False, "rot": 0.25, "scale": None}]
    assert host.DataAugmentor(cc.AUG_CONFIG[1:]).worlds([0.25, 1.5]) == [{"rot": 0.25, "scale": 1.5}]
    assert host.DataAugmentor(cc.AUG_CONFIG[::-1]).worlds([1.5, 0.25, [("x", True), ("y", True)]]) == \
        [{"scale": 1.5}, {"rot": 0.25}, {"flip_x": True, "flip_y": True}]
    yx = host.DataAugmentor([{"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["y", "x"]}])
    assert yx.worlds([[("y", True), ("x", False)]]) == [{"flip_y": True}, {"flip_x": False}]
    # why: the two heading rules do not commute bitwise
    b, m = cc.boxes("order", 4, 4)
    xy = cr.boxes(cr.boxes(b, m, {"flip_x": True}), m, {"flip_y": True})
    assert np.array_equal(xy, cr.boxes(b, m, {"flip_x": True, "flip_y": True}))
    assert not np.array_equal(xy, cr.boxes(cr.boxes(b, m, {"flip_y": True}), m, {"flip_x": True}))


@pytest.mark.parametrize("name", sorted(ltc.CASES))
def test_launch_trace(monkeypatch, name):
    records = ltc.trace(name, monkeypatch.setattr)
    assert records == ltc.read_fixture(name)
    calls = [r for r in records if r[1] == "cobevt_prepare_points"]
    assert len(calls) == {"canonical": 1, "reversed": 3, "flip_y_before_x": 3, "rotation_twice": 2}[name]
    assert all(r[1] in ("cobevt_prepare_points", "cobevt_prepare_points_scratch") for r in records)


def test_train_false_passes_through():
    d = {"lidar_np": torch.zeros(3, 4), "object_bbx_center": torch.zeros(2, 7), "object_bbx_mask": torch.ones(2)}
    keep = dict(d)
    out = host.DataAugmentor(cc.AUG_CONFIG, train=False).forward(d)
    assert out is d and all(out[k] is keep[k] for k in keep)
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        host.DataAugmentor(cc.AUG_CONFIG, train=True).forward(d)


# ---------------------------------------------------------------------------------------------- argument checks
def test_cpu_tensors_are_refused():
    p, o = torch.zeros(10, 4), torch.tensor([0, 10], dtype=torch.int32)
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        ops.prepare_points(p, o)
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        host.shuffle_order(o, 10)


def test_argument_checks(monkeypatch):
    """every check of ops.prepare_points in front of the launch, with the device guard off (tests/launch_trace.py) on CPU tensors"""
    rec = lt.Recorder()
    lt.install(monkeypatch.setattr, rec)
    p, o = torch.zeros(10, 4), torch.tensor([0, 4, 10], dtype=torch.int32)
    ws = torch.empty(64, dtype=torch.int64).view(torch.int32)
    f = ops.prepare_points
    f(p, o, workspace=ws)
    f(p, o.long(), torch.zeros(2, 4, 4), order=torch.arange(10), workspace=ws, boxes=torch.zeros(128, 7), box_mask=torch.zeros(128))
    assert [r[1] for r in rec.records].count("cobevt_prepare_points") == 2
    for bad in (p.double(), torch.zeros(10, 3), torch.zeros(10, 8)[:, :4], torch.zeros(10)):
        with pytest.raises(CobevtHipError, match="points must be contiguous fp32"):
            f(bad, o, workspace=ws)
    with pytest.raises(CobevtHipError, match="int32"):
        f(p, o.float(), workspace=ws)
    for bad in (torch.tensor([0], dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32)):
        with pytest.raises(CobevtHipError, match="point_offsets must be"):
            f(p, bad, workspace=ws)
    for bad in (torch.zeros(3, 4, 4, dtype=torch.float64), torch.zeros(2, 3, 4, dtype=torch.float64), torch.zeros(2, 4, 4, dtype=torch.float16)):
        with pytest.raises(CobevtHipError, match="transforms must be"):
            f(p, o, bad, workspace=ws)
    with pytest.raises(CobevtHipError, match="order must be an int32"):
        f(p, o, order=torch.zeros(10), workspace=ws)
    with pytest.raises(CobevtHipError, match="order must be \\(M,\\)"):
        f(p, o, order=torch.zeros(9, dtype=torch.int64), workspace=ws)
    with pytest.raises(CobevtHipError, match="lidar_range"):
        f(p, o, lidar_range=[0, 1, 2], workspace=ws)
    with pytest.raises(CobevtHipError, match="world = dict"):
        f(p, o, world={"flip_z": True}, workspace=ws)
    with pytest.raises(CobevtHipError, match="finite numbers"):
        f(p, o, world={"rot": float("nan")}, workspace=ws)
    with pytest.raises(CobevtHipError, match="at most G = 128"):
        f(p, o, boxes=torch.zeros(129, 7), box_mask=torch.zeros(129), workspace=ws)
    with pytest.raises(CobevtHipError, match="same dtype"):
        f(p, o, boxes=torch.zeros(5, 7), box_mask=torch.zeros(5, dtype=torch.float64), workspace=ws)
    for b, m in ((torch.zeros(5, 6), torch.zeros(5)), (torch.zeros(5, 7), None), (None, torch.zeros(5)), (torch.zeros(5, 7).half(), torch.zeros(5).half())):
        with pytest.raises(CobevtHipError, match="boxes must be"):
            f(p, o, boxes=b, box_mask=m, workspace=ws)
    with pytest.raises(CobevtHipError, match="box_mask must be"):
        f(p, o, boxes=torch.zeros(5, 7), box_mask=torch.zeros(4), workspace=ws)
    with pytest.raises(CobevtHipError, match="workspace= must be"):
        f(p, o, workspace=torch.empty(64))
    with pytest.raises(CobevtHipError, match="out= is"):
        f(p, o, workspace=ws, out=(torch.zeros(10, 4),))
    with pytest.raises(CobevtHipError, match="out= must be"):
        f(p, o, workspace=ws, out=(torch.zeros(9, 4), torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(CobevtHipError, match="out= must be"):
        f(p, o, workspace=ws, out=(torch.zeros(10, 4), torch.zeros(3, dtype=torch.int64)))
    big = torch.zeros(15, 4)
    for bad in (p, big[5:]):                                 # the same storage, and a window that shares rows 5 .. 9 with the input
        with pytest.raises(CobevtHipError, match="must not overlap"):
            f(big[:10] if bad is not p else p, o, workspace=ws, out=(bad, torch.zeros(3, dtype=torch.int32)))
    f(big[:5], torch.tensor([0, 5], dtype=torch.int32), workspace=ws, out=(big[5:10], torch.zeros(2, dtype=torch.int32)))   # adjacent: fine


def test_rotation_cos_sin_is_the_reference_chain():
    a = 0.5045855243760693
    t = torch.from_numpy(np.array([a])).float()
    assert ops.rotation_cos_sin(a) == (float(torch.cos(t)[0]), float(torch.sin(t)[0]))
    c, s = ops.rotation_cos_sin(a)
    assert np.float32(c) == c and np.float32(s) == s


def test_the_workspace_size_follows_its_key():
    """the default workspace is cached on M alone: the agent count, which the key leaves out, must not move the size"""
    assert ops.prepare_points_workspace_ints(1000, 1) == ops.prepare_points_workspace_ints(1000, 7) == ops.prepare_points_workspace_ints(1000)
