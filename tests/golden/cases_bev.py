"""The LiDAR BEV (PIXOR) cases shared by make_golden_bev.py (gv28_lidar_bev.npz), tests/test_lidar_bev.py and
tests/test_lidar_bev_gpu.py: procedural and seeded (cobevt_amd.synth); inputs are never stored.

Geometry: res = 0.25 and downsample_rate = 4, so all grid arithmetic is exact in binary; input_shape (96, 80, 9), label_shape
(24, 20, 7); the cut case of the post-processing uses a 40 x 32 map.  `*_conditions` assert that no decision of a case sits on a
rounding edge, except where a case is designed to (exact hits, which are exact in every arithmetic)."""
import math

import numpy as np

from cobevt_amd import synth

RES, RATE = 0.25, 4
GEOM = dict(L1=-12.0, L2=12.0, W1=-10.0, W2=10.0, H1=-1.25, H2=0.75, res=RES, input_shape=(96, 80, 9), label_shape=(24, 20, 7),
            downsample_rate=RATE)
GEOM_CUT = dict(L1=-20.0, L2=20.0, W1=-16.0, W2=16.0, H1=-1.25, H2=0.75, res=RES, input_shape=(160, 128, 9), label_shape=(40, 32, 7),
                downsample_rate=RATE)
LIDAR_RANGE = [-10.0, -8.0, -1.0, 10.0, 8.0, 0.5]         # narrower than the map, so that range_mask removes points
SCORE_THRESHOLD = 0.5
NMS_THRESH = 0.15
TARGET_MEAN = (0.008, 0.001, 0.202, 0.2, 0.43, 1.368)
TARGET_STD_DEV = (0.866, 0.5, 0.954, 0.668, 0.09, 0.111)
MAX_NUM = 8


def uniform(tag, shape, seed=0):
    return synth.procedural_input("bev." + tag, shape, seed, 0.0, 1.0).numpy().astype(np.float64)


def permutation(tag, n, seed=0):
    return np.argsort(uniform(tag + ".perm", (max(n, 1),), seed)[:n], kind="stable")


def pre_params(range_mask=False, ego_mask=False, geom=GEOM):
    return dict(core_method="BevPreprocessor", cav_lidar_range=list(LIDAR_RANGE), geometry_param=dict(geom), range_mask=range_mask,
                ego_mask=ego_mask)


def post_params(geom=GEOM, order="lwh"):
    return dict(core_method="BevPostprocessor", order=order, nms_thresh=NMS_THRESH, max_num=MAX_NUM,
                target_args=dict(score_threshold=SCORE_THRESHOLD), geometry_param=dict(geom))


# ---------------------------------------------------------------------------------------------- preprocessor
def points_main():
    """2 agents of 4000 / 3900 points, uniform over a box a little larger than the map; a coordinate closer than 1e-3 cells to a
    cell boundary is moved by 0.05 cells"""
    clouds = []
    for a, m in enumerate((4000, 3900)):
        u = uniform("pre.main.%d" % a, (m, 4))
        p = np.stack([-12.5 + 25.0 * u[:, 0], -10.5 + 21.0 * u[:, 1], -1.4 + 2.3 * u[:, 2], u[:, 3]], axis=1).astype(np.float32)
        origin = np.array([GEOM["L1"], GEOM["W1"], GEOM["H1"]])
        q = (p[:, :3].astype(np.float64) - origin) / RES
        near = np.abs(q - np.round(q)) < 1e-3
        p[:, :3] = np.where(near, p[:, :3] + np.float32(0.05 * RES), p[:, :3])
        clouds.append(np.ascontiguousarray(p))
    return clouds


def points_boundary():
    """designed rows: points exactly on cell faces, in (origin - res, origin) (truncation maps them to cell 0), on and just below
    the upper faces, at and below origin - res, non-finite values, intensities outside the summed domain, negative and tiny ones,
    several points in one cell, points inside the ego box and between the lidar range and the map's border"""
    g = GEOM
    nan, inf = float("nan"), float("inf")
    below = float(np.nextafter(np.float32(g["L2"]), np.float32(0)))
    rows = [
        # on lower faces of cells (exact in fp32 and in the fp64 index arithmetic)
        (g["L1"], g["W1"], g["H1"], 0.5), (g["L1"] + 5 * RES, g["W1"] + 7 * RES, g["H1"] + 3 * RES, 0.25),
        (g["L1"] + 95 * RES, g["W1"] + 79 * RES, g["H1"] + 7 * RES, 0.75), (0.0, 0.0, 0.0, 0.125),
        # in (origin - res, origin): cell 0 on that axis
        (g["L1"] - 0.1, 3.1, 0.1, 0.3), (g["L1"] - 0.2499, 3.1, 0.1, 0.6), (4.1, g["W1"] - 0.2, 0.1, 0.4), (4.1, 3.1, g["H1"] - 0.1, 0.9),
        # at and below origin - res: dropped
        (g["L1"] - RES, 3.1, 0.1, 0.3), (g["L1"] - 0.26, 3.1, 0.1, 0.3), (4.1, g["W1"] - 1.0, 0.1, 0.3), (4.1, 3.1, g["H1"] - RES, 0.3),
        # the upper faces: dropped; just below: the last cell
        (g["L2"], 3.1, 0.1, 0.3), (4.1, g["W2"], 0.1, 0.3), (4.1, 3.1, g["H2"], 0.3), (below, 3.1, 0.1, 0.35), (4.1, 3.1, 0.7499, 0.45),
        # non-finite values and intensities outside the domain
        (nan, 3.1, 0.1, 0.3), (4.1, inf, 0.1, 0.3), (4.1, 3.1, -inf, 0.3), (4.1, 3.1, 0.1, nan), (4.1, 3.1, 0.1, inf),
        (6.1, 3.1, 0.1, 300.0), (6.1, 3.1, 0.1, -256.0),
        # one cell, many intensities: negative, tiny (below 2^-9), exactly 2^-9, just below 256
        (6.1, 5.1, 0.1, -0.5), (6.2, 5.2, 0.1, 1e-5), (6.15, 5.15, 0.3, 2.0 ** -9), (6.12, 5.01, -0.9, 255.5), (6.01, 5.24, 0.6, 0.7),
        # inside the ego box (-1.95 .. 2.95, -1.1 .. 1.1), its border included
        (0.5, 0.5, 0.1, 0.2), (-1.95, -1.1, 0.1, 0.3), (2.95, 1.1, 0.1, 0.4), (2.96, 1.1, 0.1, 0.5),
        # inside the map, outside the lidar range (its border is outside: strict inequalities)
        (11.1, 3.1, 0.1, 0.2), (10.0, 3.1, 0.1, 0.3), (4.1, -9.1, 0.1, 0.4), (4.1, 3.1, 0.6, 0.5), (4.1, 3.1, -1.1, 0.6),
    ]
    a0 = np.asarray(rows, dtype=np.float32)
    a1 = a0[::-1].copy()
    a1[:, 3] *= np.float32(0.5)
    return [np.ascontiguousarray(a0), np.ascontiguousarray(a1)]


def pre_conditions(margin, designed):
    """every coordinate at least 1e-6 cells from a cell boundary, except in the designed boundary case (exact hits)"""
    assert designed or margin >= 1e-6, margin


def concat(clouds):
    """-> points (M, 4) fp32, offsets (N + 1,) int32"""
    return np.concatenate(clouds), np.cumsum([0] + [len(c) for c in clouds]).astype(np.int32)


# ---------------------------------------------------------------------------------------------- labels
def _gt(rows):
    gt = np.zeros((MAX_NUM, 7), dtype=np.float32)
    mask = np.zeros((MAX_NUM,), dtype=np.float32)
    for k, (box, m) in enumerate(rows):
        gt[k], mask[k] = box, m
    return gt, mask


def labels_main():
    """B = 2.  Sample 0: two overlapping boxes (the later one wins the shared pixels), a masked box between valid ones that would
    cover pixels of its own, a box partly outside the map, a box on its own; sample 1: the same boxes, none valid"""
    rows = [((-4.3, -2.2, -0.3, 4.4, 2.3, 1.5, 0.31), 1), ((-2.9, -1.1, -0.3, 4.1, 2.2, 1.6, -0.42), 1),
            ((5.2, 4.3, -0.3, 4.3, 2.1, 1.5, 1.13), 0), ((11.3, -8.7, -0.3, 4.6, 2.4, 1.5, 0.77), 1),
            ((4.6, -5.4, -0.2, 3.7, 2.6, 1.4, 2.51), 1)]
    gt, mask = _gt(rows)
    return np.stack([gt, gt]), np.stack([mask, np.zeros_like(mask)])


def labels_axis():
    """B = 1, yaw = 0, centres and sizes in whole label pixels (1 m): every edge is hit exactly and must be inclusive"""
    rows = [((-4.0, -3.0, -0.3, 4.0, 2.0, 1.5, 0.0), 1), ((3.0, 4.0, -0.3, 2.0, 2.0, 1.5, 0.0), 1)]
    gt, mask = _gt(rows)
    return gt[None], mask[None]


def labels_e2e():
    """four separate boxes inside the map, for the end-to-end check"""
    rows = [((-6.2, -4.1, -0.3, 4.2, 2.1, 1.5, 0.35), 1), ((3.4, 4.3, -0.3, 3.9, 1.9, 1.5, -0.8), 1),
            ((5.1, -5.2, -0.3, 4.4, 2.2, 1.5, 1.7), 0), ((5.1, -5.2, -0.3, 4.4, 2.2, 1.5, 1.2), 1), ((-5.3, 5.4, -0.3, 3.6, 2.0, 1.4, 2.9), 1)]
    gt, mask = _gt(rows)
    return gt[None], mask[None]


def label_conditions(out, axis_aligned):
    """no projection length within 1e-6 of 0 or 1, except the exact hits of the axis-aligned case"""
    assert out["l_margin"] >= 1e-6, out["l_margin"]
    assert (out["edge_hits"] > 0) == axis_aligned, out["edge_hits"]


# ---------------------------------------------------------------------------------------------- post_process
def matrix(yaw, t):
    c, s = math.cos(yaw), math.sin(yaw)
    m = np.eye(4)
    m[:2, :2] = [[c, -s], [s, c]]
    m[:3, 3] = t
    return m.astype(np.float32)


def _maps(tag, geom, n_cand, size=(3.9, 1.6), ladder=(0.3, 3.0), seed=0):
    """one cav's (cls, reg): n_cand pixels carry a box near their own cell with a logit of a shuffled ladder above the threshold;
    every other pixel stays below it"""
    lx, ly, _ = geom["label_shape"]
    n = lx * ly
    u = uniform(tag + ".box", (n, 6), seed)
    logits = -4.0 + 3.5 * uniform(tag + ".bg", (n,), seed)
    chosen = np.sort(permutation(tag + ".chosen", n, seed)[:n_cand])
    logits[chosen] = np.linspace(ladder[0], ladder[1], max(n_cand, 2))[:n_cand][permutation(tag + ".rank", n_cand, seed)]
    yaw = -math.pi + 2 * math.pi * u[:, 0]
    tgt = np.stack([np.cos(yaw), np.sin(yaw), 0.9 * (u[:, 1] - 0.5), 0.9 * (u[:, 2] - 0.5), np.log(size[0] * (0.9 + 0.2 * u[:, 3])),
                    np.log(size[1] * (0.9 + 0.2 * u[:, 4]))], axis=1)
    reg = (tgt - np.asarray(TARGET_MEAN)) / np.asarray(TARGET_STD_DEV)
    cls = np.ascontiguousarray(logits.reshape(1, 1, lx, ly), dtype=np.float32)
    reg = np.ascontiguousarray(reg.T.reshape(1, 6, lx, ly), dtype=np.float32)
    return cls, reg


def post_two_cavs():
    """2 cavs with non-trivial matrices, 70 and 50 candidates on the 24 x 20 map"""
    mats = [matrix(0.1, [1.5, -0.7, 0.05]), matrix(-2.0, [-3.0, 4.0, 0.1])]
    ladders = [(0.3, 3.0), (0.313, 2.971)]                     # no score of one cav equals a score of the other
    return [_maps("post.two.%d" % c, GEOM, n, ladder=ladders[c]) + (mats[c],) for c, n in enumerate((70, 50))]


def post_nothing():
    cls, reg = _maps("post.none", GEOM, 0)
    return [(cls, reg, matrix(0.3, [1.0, 2.0, 0.0]))]


def post_out_of_range():
    """candidates exist, every one leaves GT_RANGE (|y| <= 40) after the projection"""
    cls, reg = _maps("post.range", GEOM, 30)
    return [(cls, reg, matrix(0.2, [5.0, 100.0, 0.0]))]


CUT_CANDIDATES = 1100


def post_cut():
    """a 40 x 32 map of which 1100 pixels are candidates with small boxes: exercises the cut at the 1000 best"""
    cls, reg = _maps("post.cut", GEOM_CUT, CUT_CANDIDATES, size=(0.8, 0.5))
    return [(cls, reg, matrix(0.05, [0.3, -0.2, 0.0]))]


def post_conditions(out, expect_none=False):
    """distinct candidate scores, none on the threshold, no pair's IoU within 1e-4 of nms_thresh, no corner on the range border"""
    assert out["score_margin"] >= 1e-4, out["score_margin"]
    assert out["none"] == expect_none
    if out["none"]:
        return
    assert out["score_gap"] > 0.0, out["score_gap"]
    assert out["iou_margin"] >= 1e-4, out["iou_margin"]
    assert out["range_margin"] >= 1e-3, out["range_margin"]
