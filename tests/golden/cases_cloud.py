"""The cases of ops.prepare_points shared by make_golden_cloud.py (gv29_cloud_prep.npz), tests/test_cloud_prep.py and
tests/test_cloud_prep_gpu.py: procedural sensor-frame clouds, matrices and boxes (cobevt_amd.synth; never stored).  The golden cases
keep every coordinate that meets a mask limit at least MARGIN away from it (rows that come closer are left out of the input), so that
the fp32-against-fp64 compare of the range mask cannot decide anything; points ON the limits are a case of their own (edge_points),
checked against the restatement only."""
import os
import sys

import numpy as np

from cobevt_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import cloud_ref as cr  # noqa: E402

LIDAR_RANGE = [-140.8, -40, -3, 140.8, 40, 1]            # OPV2V's cav_lidar_range
MARGIN = 1e-3
AUG_CONFIG = [{"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x", "y"]},
              {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
              {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.95, 1.05]}]
ROT_RANGE, SCALE_RANGE = AUG_CONFIG[1]["WORLD_ROT_ANGLE"], AUG_CONFIG[2]["WORLD_SCALE_RANGE"]
SEED = 7
MAX_BOXES, VALID_BOXES = 100, 17                         # the reference's max_num and a prefix of valid rows

# name -> per-agent sizes before the margin filter, masks / projection, augmentation ("flips" | "rot" | "scale" | "full" | None)
GOLDEN = {
    "project": dict(sizes=[1100, 900, 1000], masks=True, aug=None),
    "flips": dict(sizes=[1500], masks=False, aug="flips"),
    "rotation": dict(sizes=[3000], masks=False, aug="rot"),
    "scaling": dict(sizes=[1500], masks=False, aug="scale"),
    "augmentor": dict(sizes=[2000], masks=False, aug="full"),
    "all": dict(sizes=[1000, 1100, 1000], masks=True, aug="full"),
}
FLIPS_WANTED = {"flips": (True, True), "augmentor": (True, True), "all": (True, False)}


def uniform(tag, shape, lo=0.0, hi=1.0, seed=0):
    return synth.procedural_input("cloud." + tag, shape, seed, lo, hi).numpy().astype(np.float64)


def raw_cloud(tag, n):
    """(n, 4) fp32 in a sensor frame: an eighth of the points around the ego vehicle's box, the rest past the range on every side"""
    u = uniform(tag, (max(n, 1), 4))[:n]
    near = np.arange(n) < n // 8
    x = np.where(near, -4.0 + 9.0 * u[:, 0], -170.0 + 340.0 * u[:, 0])
    y = np.where(near, -2.5 + 5.0 * u[:, 1], -60.0 + 120.0 * u[:, 1])
    return np.stack([x, y, -4.0 + 6.0 * u[:, 2], u[:, 3]], axis=1).astype(np.float32)


def transform(tag):
    """a 4 x 4 fp64 pose difference: yaw anywhere, small roll / pitch, a shift of some metres; the entries are rounded to multiples of
    2^-20, so that the last bit of a libm cosine cannot move the case"""
    u = uniform(tag + ".pose", (6,))
    yaw, pitch, roll = np.pi * (2 * u[0] - 1), 0.05 * (2 * u[1] - 1), 0.05 * (2 * u[2] - 1)
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    t = np.eye(4)
    t[:3, :3] = rz @ ry @ rx
    t[:3, 3] = [30.0 * (2 * u[3] - 1), 15.0 * (2 * u[4] - 1), 0.5 * (2 * u[5] - 1)]
    return np.round(t * 2.0 ** 20) / 2.0 ** 20


def boxes(tag, g=MAX_BOXES, valid=VALID_BOXES, dtype=np.float64, hole=None):
    """object_bbx_center (g, 7) [x, y, z, dx, dy, dz, heading] with zero rows past `valid`, and its prefix mask (row `hole` cleared)"""
    u = uniform(tag + ".boxes", (max(g, 1), 7))[:g]
    b = np.stack([200 * u[:, 0] - 100, 80 * u[:, 1] - 40, -2 + 2 * u[:, 2], 1 + 4 * u[:, 3], 1 + 2 * u[:, 4], 1 + 1.5 * u[:, 5],
                  np.pi * (2 * u[:, 6] - 1)], axis=1)
    mask = (np.arange(g) < valid).astype(np.float64)
    b[mask == 0] = 0
    if hole is not None:
        mask[hole] = 0                                   # (the row keeps its values: it must come back untouched)
    return b.astype(dtype), mask.astype(dtype)


def aug_seed(want):
    """the first NumPy seed whose two flip draws are `want`"""
    for seed in range(1000):
        r = np.random.RandomState(seed)
        if tuple(bool(r.choice([False, True], replace=False, p=[0.5, 0.5])) for _ in range(2)) == tuple(want):
            return seed
    raise AssertionError(want)


def draw(name):
    """(seed, world, params in DataAugmentor.draw's format or None) of a golden case, replayed from the seed with the reference's calls"""
    aug = GOLDEN[name]["aug"]
    if aug is None:
        return None, None, None
    if aug == "rot":
        return SEED, {"rot": float(np.random.RandomState(SEED).uniform(ROT_RANGE[0], ROT_RANGE[1]))}, None
    if aug == "scale":
        return SEED, {"scale": float(np.random.RandomState(SEED).uniform(SCALE_RANGE[0], SCALE_RANGE[1]))}, None
    seed = aug_seed(FLIPS_WANTED[name])
    r = np.random.RandomState(seed)
    fx, fy = (bool(r.choice([False, True], replace=False, p=[0.5, 0.5])) for _ in range(2))
    if aug == "flips":
        return seed, {"flip_x": fx, "flip_y": fy}, None
    rot, scale = float(r.uniform(ROT_RANGE[0], ROT_RANGE[1])), float(r.uniform(SCALE_RANGE[0], SCALE_RANGE[1]))
    return seed, {"flip_x": fx, "flip_y": fy, "rot": rot, "scale": scale}, [[("x", fx), ("y", fy)], rot, scale]


def cos_sin(world):
    from cobevt_amd import ops
    return ops.rotation_cos_sin(world["rot"]) if world and world.get("rot") is not None else (None, None)


def margin(p, t, masks, world):
    """per row: the smallest distance of a coordinate that a mask compares from that mask's limit (inf without masks)"""
    if not masks:
        return np.full(len(p), np.inf)
    c, s = cos_sin(world)
    _, _, xyz = cr.stages(p, t, True, LIDAR_RANGE, world, c, s)
    ego = np.min(np.abs(np.stack([p[:, 0] - cr.EGO[0], p[:, 0] - cr.EGO[1], p[:, 1] - cr.EGO[2], p[:, 1] - cr.EGO[3]])), axis=0)
    lim = np.asarray(LIDAR_RANGE, dtype=np.float64)
    rng = np.min(np.abs(np.concatenate([xyz - lim[:3], xyz - lim[3:]], axis=1)), axis=1)
    return np.minimum(ego, rng)


def golden_case(name):
    """-> dict(clouds [fp32 (n_a, 4)], transforms (N, 4, 4) | None, masks, world | None, seed, params, boxes, box_mask)"""
    spec = GOLDEN[name]
    seed, world, params = draw(name)
    clouds, mats = [], []
    for a, n in enumerate(spec["sizes"]):
        p = raw_cloud("%s.%d" % (name, a), n)
        t = transform("%s.%d" % (name, a)) if spec["masks"] else None
        p = p[margin(p, t, spec["masks"], world) >= MARGIN]
        clouds.append(p)
        mats.append(t)
    b, bm = boxes(name) if spec["aug"] else (None, None)
    return dict(clouds=clouds, transforms=np.stack(mats) if spec["masks"] else None, masks=spec["masks"], world=world, seed=seed,
                params=params, boxes=b, box_mask=bm)


def concat(clouds):
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    pts = np.concatenate(clouds).astype(np.float32) if sum(len(c) for c in clouds) else np.zeros((0, 4), dtype=np.float32)
    return np.ascontiguousarray(pts), offs


def restated(case):
    """the restatement's (out, out_offsets, keep, boxes) of a golden case"""
    pts, offs = concat(case["clouds"])
    c, s = cos_sin(case["world"])
    out, out_offs, keep = cr.prepare_points(pts, offs, case["transforms"], None, case["masks"], LIDAR_RANGE if case["masks"] else None,
                                            case["world"], c, s)
    b = cr.boxes(case["boxes"], case["box_mask"], case["world"], c, s) if case["boxes"] is not None else None
    return out, out_offs, keep, b


# ---------------------------------------------------------------------------------------------- the gates against the fixture
EPS = 2.0 ** -24


def ulps32(a, b):
    ia, ib = (np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(v < 0, -(v & 0x7fffffff), v) for v in (ia, ib))
    return np.abs(ia - ib)


def rotation_gate(case, keep):
    """(n, 3) bound on |reference - restatement| of the kept output points of a case with a rotation (derived in tests/test_cloud_prep.py's docstring)"""
    world = case["world"]
    c, s = cos_sin(world)
    pts, offs = concat(case["clouds"])
    pre = []
    for a in range(len(offs) - 1):
        xyz = pts[offs[a]:offs[a + 1], :3].astype(np.float64)
        if case["masks"]:
            xyz = cr.project(xyz, case["transforms"][a])
        pre.append(cr.augment(xyz, {k: world.get(k) for k in ("flip_x", "flip_y")}))
    x, y = (np.concatenate(pre)[keep][:, j].astype(np.float32).astype(np.float64) for j in (0, 1))
    e = 3.0 * EPS
    gate = np.stack([e * (np.abs(x * c) + np.abs(y * s)), e * (np.abs(x * s) + np.abs(y * c)), np.zeros_like(x)], axis=1)
    return gate, world.get("scale")


def check_against_reference(gv, name, out, out_offs, boxes):
    """`out` / `out_offs` / `boxes` (the restatement's, or the device's) against the fixture, under the gates of tests/test_cloud_prep.py's docstring"""
    case = golden_case(name)
    ref, ref_offs = gv[name + "_points"], gv[name + "_offsets"]
    assert ref.dtype == np.float32 and out.dtype == np.float32 and np.array_equal(ref_offs, out_offs) and ref.shape == out.shape
    assert np.array_equal(ref[:, 3], out[:, 3])
    world = case["world"]
    if world is None or world.get("rot") is None:
        u = ulps32(ref[:, :3], out[:, :3])
        diff, total = (int(v) for v in gv[name + "_proj_diff"])
        assert int(u.max(initial=0)) <= (1 if case["masks"] else 0)
        assert int((u != 0).sum()) <= 1e-4 * max(total, 1) and diff <= 1e-4 * max(total, 1)
    else:
        keep = restated(case)[2]
        gate, scale = rotation_gate(case, keep)
        assert int(gv[name + "_proj_diff"][0]) == 0       # the gate's premise: the rotation's inputs are the reference's, bit for bit
        if scale is not None:
            gate = gate * float(np.float32(scale))
        err = np.abs(ref[:, :3].astype(np.float64) - out[:, :3])
        assert (err <= gate).all(), (name, float((err - gate).max()))
        assert len(ref) > 500 and err.max() > 0          # the fp32 matmul is not the restatement's arithmetic: the gate is in use
    if case["boxes"] is not None:
        rb = gv[name + "_boxes"]
        assert rb.dtype == boxes.dtype == np.float64 and np.array_equal(rb[:, 3:], boxes[:, 3:])
        assert np.array_equal(rb[VALID_BOXES:], boxes[VALID_BOXES:]) and not rb[VALID_BOXES:].any()
        if world.get("rot") is None:
            assert np.array_equal(rb, boxes)
        else:
            c, s = cos_sin(world)
            pre = cr.augment(case["boxes"][:VALID_BOXES, :3], {k: world.get(k) for k in ("flip_x", "flip_y")})
            x, y = (pre[:, j].astype(np.float32).astype(np.float64) for j in (0, 1))
            sc = 1.0 if world.get("scale") is None else float(world["scale"])
            gate = 3.0 * EPS * sc * np.stack([np.abs(x * c) + np.abs(y * s), np.abs(x * s) + np.abs(y * c), np.zeros_like(x)], axis=1)
            gate = gate + 2.0 ** -52 * np.abs(rb[:VALID_BOXES, :3])               # (the scaling's fp64 rounding of each side)
            assert (np.abs(rb[:VALID_BOXES, :3] - boxes[:VALID_BOXES, :3]) <= gate).all()


def edge_points():
    """one agent's fp32 points ON and next to the ego and range limits (no projection), a NaN and infinities among them"""
    f = np.float32
    rows = []
    lim = np.asarray(LIDAR_RANGE, dtype=np.float64).astype(f)
    for v in cr.EGO[:2]:
        for d in (-1, 0, 1):
            x = np.nextafter(v, f(np.inf) * d) if d else v
            rows += [[x, 0.0, 0.0, 0.1], [x, cr.EGO[2], 0.0, 0.2], [x, np.nextafter(cr.EGO[3], f(np.inf)), 0.0, 0.3]]
    for v in cr.EGO[2:]:
        for d in (-1, 0, 1):
            rows.append([1.0, np.nextafter(v, f(np.inf) * d) if d else v, 0.0, 0.4])
    for j in range(3):
        for v in (lim[j], lim[3 + j]):
            for d in (-1, 0, 1):
                p = [10.0, 10.0, -1.0, 0.5]
                p[j] = np.nextafter(v, f(np.inf) * d) if d else v
                rows.append(p)
    rows += [[np.nan, 0.0, 0.0, 0.6], [5.0, np.nan, 0.0, 0.6], [np.inf, 0.0, 0.0, 0.7], [-np.inf, 5.0, 0.0, 0.7], [5.0, 5.0, np.inf, 0.8],
             [10.0, 10.0, -1.0, np.nan], [140.7999999, 0.0, 0.0, 0.9]]
    return np.asarray(rows, dtype=f)
