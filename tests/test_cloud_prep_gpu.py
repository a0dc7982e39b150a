"""ops.prepare_points / host.DataAugmentor / host.shuffle_order on the device: bit-exact against the restatement tests/cloud_ref.py
across block seams, empty agents, keep patterns, stages and `order`; rows past the end; edge points; boxes; composition with
voxelize_points; the golden cases under the gates of tests/test_cloud_prep.py; determinism; graph capture."""
import numpy as np
import pytest
import torch

import cases_cloud as cc
import cases_voxel as cv
import cloud_ref as cr
from cobevt_amd import host, ops
from cobevt_amd.host import pipeline
from util import golden

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
WORLD = {"flip_x": True, "flip_y": True, "rot": 0.61, "scale": 1.04}
# per-agent counts from {0, 1, 1023, 1024, 1025, 2051}: block seams, an empty agent first / middle / last, an agent boundary inside a
# 1024-block, M = 0
COUNTS = [(0,), (1,), (1023,), (1024,), (1025,), (2051,), (0, 1025), (1023, 0, 2051), (2051, 1024, 0), (1, 1023, 1025), (1025, 2051, 1024),
          (0, 0, 0)]
STAGES = {
    "ego": dict(ego_mask=True), "range": dict(lidar_range=cc.LIDAR_RANGE), "project": dict(project=True),
    "flip": dict(world={"flip_x": True, "flip_y": True}), "rot": dict(world={"rot": -0.4}), "scale": dict(world={"scale": 0.97}),
    "all": dict(ego_mask=True, lidar_range=cc.LIDAR_RANGE, project=True, world=WORLD),
}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _cloud(tag, counts, pattern, ego):
    """the agents' clouds concatenated, with the keep pattern built in: a kept row lies in front of the vehicle and well inside the
    range, a dropped one inside the ego box (when the ego mask is the stage under test) or far outside the range"""
    m = sum(counts)
    u = cc.uniform("%s.%s.%d" % (tag, pattern, m), (max(m, 1), 4))[:m]
    keep = {"all": np.ones(m, bool), "none": np.zeros(m, bool), "alternating": np.arange(m) % 2 == 0,
            "random": cc.uniform("%s.keep.%d" % (tag, m), (max(m, 1),))[:m] < 0.5}[pattern]
    inside = np.stack([5 + 25 * u[:, 0], -15 + 30 * u[:, 1], -2 + 2 * u[:, 2], u[:, 3]], axis=1)
    if ego:
        outside = np.stack([-1.5 + 4 * u[:, 0], -1 + 2 * u[:, 1], -2 + 2 * u[:, 2], u[:, 3]], axis=1)
    else:
        outside = np.stack([200 + 100 * u[:, 0], -15 + 30 * u[:, 1], -2 + 2 * u[:, 2], u[:, 3]], axis=1)
    pts = np.where(keep[:, None], inside, outside).astype(np.float32)
    return np.ascontiguousarray(pts), np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), keep


def _order(offs, m):
    """a fixed permutation within every agent's rows (rows past offsets[N] stay where they are)"""
    order = np.arange(m, dtype=np.int64)
    r = np.random.RandomState(5)
    for a in range(len(offs) - 1):
        order[offs[a]:offs[a + 1]] = offs[a] + r.permutation(offs[a + 1] - offs[a])
    return order


def _run(dev, pts, offs, stage, order=None, transforms=None, **kw):
    """the device's and the restatement's (out, out_offsets); the device's `out` is prefilled with the sentinel"""
    stage = dict(stage)
    t = transforms if stage.pop("project", False) else None
    world = stage.get("world")
    c, s = cc.cos_sin(world)
    ref = cr.prepare_points(pts, offs, t, order, stage.get("ego_mask", False), stage.get("lidar_range"), world, c, s)
    out = (torch.full((len(pts), 4), SENTINEL, device=dev), torch.full((len(offs),), -7, dtype=torch.int32, device=dev))
    got = ops.prepare_points(torch.from_numpy(pts).to(dev), torch.from_numpy(offs).to(dev),
                             None if t is None else torch.from_numpy(t).to(dev),
                             order=None if order is None else torch.from_numpy(order).to(dev), out=out, **stage, **kw)
    assert got[0] is out[0] and got[1] is out[1]
    torch.cuda.synchronize()
    return got[0].cpu().numpy(), got[1].cpu().numpy(), ref


def _check(got_pts, got_offs, ref, what):
    out, out_offs, _ = ref
    k = len(out)
    assert np.array_equal(got_offs, out_offs), (what, got_offs, out_offs)
    assert np.array_equal(_bits(got_pts[:k]), _bits(out)), what
    assert (got_pts[k:] == SENTINEL).all(), "%s: rows at or past out_offsets[N] were written" % what


# ---------------------------------------------------------------------------------------------- 1. seams, patterns, stages, order
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_seams(cuda, stage):
    masked = stage in ("ego", "range", "all")
    for counts in COUNTS:
        transforms = np.stack([cc.transform("seam.%d" % a) for a in range(len(counts))])
        for pattern in (("all", "none", "alternating", "random") if masked else ("random",)):
            pts, offs, keep = _cloud("seam", counts, pattern, stage == "ego")
            for order in (None, _order(offs, len(pts))):
                got_pts, got_offs, ref = _run(cuda, pts, offs, STAGES[stage], order, transforms)
                _check(got_pts, got_offs, ref, (stage, counts, pattern, order is not None))
                if stage in ("ego", "range"):              # the pattern is what the mask makes of the cloud
                    assert np.array_equal(ref[2], keep if order is None else keep[order])
                elif not masked:
                    assert ref[2].all()
    if stage == "all":                                     # every stage decides something there
        pts, offs, _ = _cloud("seam", (1025, 2051, 1024), "random", False)
        k = _run(cuda, pts, offs, STAGES[stage], None, np.stack([cc.transform("seam.%d" % a) for a in range(3)]))[2][2]
        assert 0 < k.sum() < len(pts)


def test_order_shuffles_within_agents(cuda):
    """host.shuffle_order: a permutation that maps each agent's rows onto themselves; with it the output is the ordered gather"""
    pts, offs, _ = _cloud("shuffle", (1500, 0, 1100), "random", False)
    m = len(pts) + 37                                      # rows past offsets[N]
    pts = np.concatenate([pts, np.full((37, 4), 3.0, dtype=np.float32)])
    g = torch.Generator(device=cuda)
    g.manual_seed(11)
    order = host.shuffle_order(torch.from_numpy(offs).to(cuda), m, generator=g)
    o = order.cpu().numpy().astype(np.int64)
    assert order.dtype == torch.int32 and np.array_equal(np.sort(o), np.arange(m))
    for a in range(len(offs) - 1):
        assert np.array_equal(np.sort(o[offs[a]:offs[a + 1]]), np.arange(offs[a], offs[a + 1]))
    assert np.array_equal(np.sort(o[offs[-1]:]), np.arange(offs[-1], m)) and not np.array_equal(o, np.arange(m))
    g.manual_seed(11)
    assert torch.equal(order, host.shuffle_order(torch.from_numpy(offs).to(cuda).long(), m, generator=g))
    got_pts, got_offs, ref = _run(cuda, pts, offs, STAGES["range"], o)
    _check(got_pts, got_offs, ref, "shuffle")
    assert np.array_equal(_bits(ref[0]), _bits(pts[o][:offs[-1]][ref[2][:offs[-1]]]))


# ---------------------------------------------------------------------------------------------- 2. rows past the end
def test_rows_past_the_end(cuda):
    """rows at or past offsets[N] and in front of offsets[0] are ignored, offsets past M are clamped, an order entry outside [0, M)
    drops its row; the rows of out at or past out_offsets[N] keep the sentinel"""
    pts, _, _ = _cloud("past", (3000,), "random", False)
    for offs in ([0, 1000, 2500], [100, 1024, 2048], [0, 2000, 5000], [0, 0, 0]):
        offs = np.asarray(offs, dtype=np.int32)
        got_pts, got_offs, ref = _run(cuda, pts, offs, STAGES["range"])
        _check(got_pts, got_offs, ref, offs)
        o = np.clip(offs, 0, len(pts))
        assert not ref[2][o[-1]:].any() and not ref[2][:o[0]].any()
    offs = np.asarray([0, 3000], dtype=np.int32)
    order = np.arange(3000, dtype=np.int64)
    order[[0, 1500, 2999]] = [-1, 3000, 2 ** 31 - 1]
    got_pts, got_offs, ref = _run(cuda, pts, offs, {}, order)
    _check(got_pts, got_offs, ref, "order outside")
    assert len(ref[0]) == 2997


# ---------------------------------------------------------------------------------------------- 3. edge points
@pytest.mark.parametrize("ego,rng", [(True, False), (False, True), (True, True)])
def test_edge_points(cuda, ego, rng):
    p = np.ascontiguousarray(cc.edge_points())
    offs = np.asarray([0, len(p)], dtype=np.int32)
    stage = dict(ego_mask=ego, **({"lidar_range": cc.LIDAR_RANGE} if rng else {}))
    got_pts, got_offs, ref = _run(cuda, p, offs, stage)
    assert np.array_equal(got_offs, ref[1]) and 0 < ref[1][1] < len(p)
    k = int(ref[1][1])
    assert np.array_equal(_bits(got_pts[:k]), _bits(ref[0])) and (got_pts[k:] == SENTINEL).all()
    assert np.isnan(ref[0][:, :3]).any() == (not rng)      # a NaN survives the ego mask and fails the range mask


# ---------------------------------------------------------------------------------------------- 4. boxes
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("g,valid,hole", [(0, 0, None), (1, 1, None), (1, 0, None), (128, 128, None), (128, 40, None), (128, 40, 7)])
def test_boxes(cuda, dtype, g, valid, hole):
    pts, offs, _ = _cloud("boxes", (100,), "all", False)
    for world in (WORLD, {"flip_x": True}, {"flip_y": True}, {"rot": -1.2}, {"scale": 1.05}, {}):
        b, m = cc.boxes("gpu", g, valid, dtype, hole)
        c, s = cc.cos_sin(world)
        ref = cr.boxes(b, m, world, c, s)
        tb, tm = torch.from_numpy(b.copy()).to(cuda), torch.from_numpy(m).to(cuda)
        ops.prepare_points(torch.from_numpy(pts).to(cuda), torch.from_numpy(offs).to(cuda), world=world, boxes=tb, box_mask=tm)
        torch.cuda.synchronize()
        got = tb.cpu().numpy()
        assert got.dtype == dtype and np.array_equal(_bits(got), _bits(ref)), (world, np.abs(got - ref).max(initial=0))
        assert np.array_equal(_bits(got[m != 1]), _bits(b[m != 1])) and np.array_equal(tm.cpu().numpy(), m)
        if world and valid:
            assert not np.array_equal(got[m == 1], b[m == 1])


# ---------------------------------------------------------------------------------------------- 5. composition with the voxeliser
def test_composition_with_voxelize(cuda):
    """without projection and augmentation, prepare_points (ego and range masks) then voxelize_points without masks is
    voxelize_points with both masks on the raw points: all four outputs, bitwise, on the rows that hold a voxel"""
    grid = (32, 32)
    rng = cv.lidar_range(*grid)
    counts = (1500, 0, 2051)
    m = sum(counts)
    u = cc.uniform("compose", (m, 4))
    pts = np.ascontiguousarray(np.stack([-8 + 16 * u[:, 0], -8 + 16 * u[:, 1], -3.5 + 5 * u[:, 2], u[:, 3]], axis=1).astype(np.float32))
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    p, o = torch.from_numpy(pts).to(cuda), torch.from_numpy(offs).to(cuda)
    direct = ops.voxelize_points(p, o, rng, cv.VOXEL_SIZE, 32, 1024, range_mask=True, ego_mask=True)
    q, qo = ops.prepare_points(p, o, ego_mask=True, lidar_range=rng)
    staged = ops.voxelize_points(q, qo, rng, cv.VOXEL_SIZE, 32, 1024)
    torch.cuda.synchronize()
    kept = int(qo[-1])
    assert 0 < kept < m and int(direct[3].min()) == 0 and int(direct[3].max()) > 100
    for a, b in zip(direct[1:], staged[1:]):
        assert torch.equal(a, b)
    rows = direct[1][:, 0] >= 0
    assert int(rows.sum()) == int(direct[3].sum())
    assert torch.equal(direct[0][rows].view(torch.int32), staged[0][rows].view(torch.int32))


# ---------------------------------------------------------------------------------------------- 6. the golden cases
@pytest.mark.parametrize("name", sorted(cc.GOLDEN))
def test_golden(cuda, name):
    gv = golden("gv29_cloud_prep")
    case = cc.golden_case(name)
    pts, offs = cc.concat(case["clouds"])
    p, o = torch.from_numpy(pts).to(cuda), torch.from_numpy(offs).to(cuda)
    boxes = None if case["boxes"] is None else torch.from_numpy(case["boxes"].copy()).to(cuda)
    mask = None if case["boxes"] is None else torch.from_numpy(case["box_mask"]).to(cuda)
    if name == "augmentor":                                # through the host mirror, with the parameters replayed from the seed
        aug = host.DataAugmentor(cc.AUG_CONFIG)
        d = aug.forward({"lidar_np": p, "object_bbx_center": boxes, "object_bbx_mask": mask},
                        params=aug.draw(np.random.RandomState(case["seed"])))
        out, out_offs = d["lidar_np"], o
        assert d["object_bbx_center"] is boxes and d["object_bbx_mask"] is mask
    else:
        out, out_offs = ops.prepare_points(p, o, None if case["transforms"] is None else torch.from_numpy(case["transforms"]).to(cuda),
                                           ego_mask=case["masks"], lidar_range=cc.LIDAR_RANGE if case["masks"] else None,
                                           world=case["world"], boxes=boxes, box_mask=mask)
    torch.cuda.synchronize()
    out_offs = out_offs.cpu().numpy()
    out = out.cpu().numpy()[:int(out_offs[-1])]
    mine = cc.restated(case)
    assert np.array_equal(_bits(out), _bits(mine[0])) and np.array_equal(out_offs, mine[1])
    cc.check_against_reference(gv, name, out, out_offs, None if boxes is None else boxes.cpu().numpy())


# ---------------------------------------------------------------------------------------------- 7. determinism
def test_determinism(cuda):
    counts = (20000, 17001, 23000, 0, 19999)
    pts, offs, _ = _cloud("twice", counts, "random", False)
    t = torch.from_numpy(np.stack([cc.transform("twice.%d" % a) for a in range(len(counts))])).to(cuda)
    p, o = torch.from_numpy(pts).to(cuda), torch.from_numpy(offs).to(cuda)
    order = host.shuffle_order(o, len(pts))
    runs = []
    for _ in range(2):
        out = (torch.zeros(len(pts), 4, device=cuda), torch.zeros(len(offs), dtype=torch.int32, device=cuda))
        ops.prepare_points(p, o, t, order=order, ego_mask=True, lidar_range=cc.LIDAR_RANGE, world=WORLD, out=out)
        runs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert 0 < int(runs[0][1][-1]) < len(pts)
    ref = cr.prepare_points(pts, offs, t.cpu().numpy(), order.cpu().numpy().astype(np.int64), True, cc.LIDAR_RANGE, WORLD,
                            *cc.cos_sin(WORLD))
    k = len(ref[0])
    assert np.array_equal(runs[0][1].cpu().numpy(), ref[1]) and np.array_equal(_bits(runs[0][0].cpu().numpy()[:k]), _bits(ref[0]))


# ---------------------------------------------------------------------------------------------- 8. graph capture
def test_graph_replay(cuda):
    """pipeline.CapturedCall over prepare_points -> SpVoxelPreprocessor.preprocess_batch at a fixed M with device-side offsets and
    matrices: each replay equals its eager run, bit for bit"""
    grid = (32, 32)
    pre = host.SpVoxelPreprocessor(cv.preprocess_params(grid, max_voxel_test=1024), train=False)
    rng = cv.lidar_range(*grid)
    m_fixed = 4000
    sets = []
    for tag, sizes in (("replay.a", (1500, 1200, 1300)), ("replay.b", (900, 1700, 1000))):
        m = sum(sizes)
        u = cc.uniform(tag, (m_fixed, 4))
        pts = np.stack([-9 + 18 * u[:, 0], -9 + 18 * u[:, 1], -3.5 + 5 * u[:, 2], u[:, 3]], axis=1).astype(np.float32)
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        t = np.stack([cc.transform("%s.%d" % (tag, a)) for a in range(3)])
        t[:, :3, 3] *= 0.1                                  # (the grid is 12.8 m wide)
        sets.append((torch.from_numpy(np.ascontiguousarray(pts)).to(cuda), torch.from_numpy(offs).to(cuda), torch.from_numpy(t).to(cuda)))
        assert m <= m_fixed

    def fn(points, offsets, transforms):
        q, qo = ops.prepare_points(points, offsets, transforms, ego_mask=True, lidar_range=rng, world={"flip_x": True, "rot": 0.3, "scale": 0.98})
        d = pre.preprocess_batch(q, qo)
        return d["voxel_features"], d["voxel_coords"], d["voxel_num_points"], d["num_voxels"], qo

    def snapshot(res):
        rows = res[1][:, 0] >= 0
        return [res[0][rows].clone().view(torch.int32)] + [r.clone() for r in res[1:]]
    eager = [snapshot(fn(*s)) for s in sets]
    run = pipeline.CapturedCall(fn, *sets[0])
    assert run.graph is not None
    for i in (0, 1, 0):
        got = snapshot(run.step(*sets[i]))
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, eager[i])), i
    assert not torch.equal(eager[0][4], eager[1][4]) and int(eager[0][3].min()) > 50
