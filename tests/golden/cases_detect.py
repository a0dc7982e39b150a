"""The detection-output cases shared by make_golden_detect.py (gv24_voxel_postprocess.npz), tests/test_voxel_postprocess.py,
tests/test_voxel_postprocess_gpu.py and tools/detect_probe.py: procedural head maps (cobevt_amd.synth; never stored).

A case lists designed boxes in the ego frame; each is given to one anchor of one cav (a fixed permutation picks it), moved into that
cav's frame by the inverse of the cav's matrix and ENCODED against the anchor (the inverse of delta_to_boxes3d, in float64, rounded
to fp32), so the head map decodes to the designed box whatever anchor carries it.  Every other anchor keeps its own box with a logit
below the threshold.  Candidate logits are a shuffled, evenly spaced ladder (no two scores closer than 1e-5, none within 1e-4 of the
threshold).  `conditions(out)` asserts that no decision of a case sits on a rounding edge, on the restatement's float64 diagnostics."""
import math

import numpy as np

from cobevt_amd import synth

SCORE_THRESHOLD = 0.2
NMS_THRESH = 0.15
LOGIT_THR = math.log(SCORE_THRESHOLD / (1.0 - SCORE_THRESHOLD))
L, W, H = 3.9, 1.6, 1.56                                  # OPV2V's anchor


def uniform(tag, shape, seed=0):
    return synth.procedural_input("detect." + tag, shape, seed, 0.0, 1.0).numpy().astype(np.float64)


def permutation(tag, n, seed=0):
    return np.argsort(uniform(tag + ".perm", (max(n, 1),), seed)[:n], kind="stable")


def anchor_params(grid, order, x_half, y_half, stride=None):
    """VoxelPostprocessor's parameters for a (rows, cols) anchor grid over [-x_half, x_half] x [-y_half, y_half]"""
    rows, cols = grid
    s = 2 if stride is None else stride
    args = dict(W=cols * s, H=rows * s, l=L, w=W, h=H, r=[0, 90], vw=0.4, vh=0.4, num=2,
                cav_lidar_range=[-x_half, -y_half, -3, x_half, y_half, 1])
    if stride is not None:
        args["feature_stride"] = stride
    return dict(core_method="VoxelPostprocessor", anchor_args=args, order=order, nms_thresh=NMS_THRESH,
                target_args=dict(score_threshold=SCORE_THRESHOLD, pos_threshold=0.6, neg_threshold=0.45))


def matrix(yaw, t, tilt=0.0, reflect=False):
    """z rotation `yaw`, a small tilt about x that moves z, translation t; reflect: y -> -y first (flips every winding)"""
    cz, sz, ct, st = math.cos(yaw), math.sin(yaw), math.cos(tilt), math.sin(tilt)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    rx = np.array([[1.0, 0, 0], [0, ct, -st], [0, st, ct]])
    m = np.eye(4)
    m[:3, :3] = rz @ rx @ (np.diag([1.0, -1.0, 1.0]) if reflect else np.eye(3))
    m[:3, 3] = t
    return m.astype(np.float32)


def to_cav_frame(box, m):
    """designed ego-frame box (x, y, z, l, w, h, yaw) -> the same box in the frame of the cav with matrix m (tilt ignored for the yaw)"""
    m = m.astype(np.float64)
    p = np.linalg.inv(m[:3, :3]) @ (np.asarray(box[:3]) - m[:3, 3])
    d = np.linalg.inv(m[:3, :3]) @ np.array([math.cos(box[6]), math.sin(box[6]), 0.0])
    return [p[0], p[1], p[2], box[3], box[4], box[5], math.atan2(d[1], d[0])]


def encode(box_lwh, anchor, order):
    """the deltas delta_to_boxes3d turns back into the box (x, y, z, l, w, h, yaw); anchor (7,) in `order`"""
    x, y, z, l, w, h, yaw = box_lwh
    sizes = [h, w, l] if order == "hwl" else [l, w, h]             # what the three size columns must decode to
    diag = math.sqrt(anchor[4] ** 2 + anchor[5] ** 2)
    return [(x - anchor[0]) / diag, (y - anchor[1]) / diag, (z - anchor[2]) / anchor[3]] + \
        [math.log(sizes[k] / anchor[3 + k]) for k in range(3)] + [yaw - anchor[6]]


def build(tag, anchors_per_cav, matrices, order, designed, background_logit=(-4.0, LOGIT_THR - 0.3), top_logit=3.0):
    """designed: [(cav, ego box (x, y, z, l, w, h, yaw), rank)] - rank orders the scores (higher rank = higher score); a box with
    rank None is placed with a background logit.  -> [(psm, rm, anchors fp32, matrix)] per cav and the global anchor index of each
    designed box"""
    ncav = len(anchors_per_cav)
    psm, rm, slots = [], [], []
    for c in range(ncav):
        a = np.asarray(anchors_per_cav[c], dtype=np.float64)
        rows, cols, na, _ = a.shape
        n = rows * cols * na
        lo, hi = background_logit
        logits = lo + (hi - lo) * uniform("%s.bg.%d" % (tag, c), (n,))
        psm.append(logits)
        rm.append(np.zeros((n, 7)))
        slots.append(list(permutation("%s.slot.%d" % (tag, c), n)))
    ranked = sorted([i for i, d in enumerate(designed) if d[2] is not None], key=lambda i: designed[i][2])
    ladder = np.linspace(LOGIT_THR + 0.3, top_logit, max(len(ranked), 2))
    start = np.cumsum([0] + [len(p) for p in psm])
    where = []
    for i, (c, box, rank) in enumerate(designed):
        flat = int(slots[c].pop(0))
        a = np.asarray(anchors_per_cav[c], dtype=np.float64).reshape(-1, 7)[flat]
        rm[c][flat] = encode(to_cav_frame(box, matrices[c]), a, order)
        if rank is not None:
            psm[c][flat] = ladder[ranked.index(i)]
        where.append(int(start[c]) + flat)
    cavs = []
    for c in range(ncav):
        rows, cols, na, _ = np.asarray(anchors_per_cav[c]).shape
        p = psm[c].reshape(rows, cols, na).transpose(2, 0, 1)[None]
        r = rm[c].reshape(rows, cols, na * 7).transpose(2, 0, 1)[None]
        cavs.append((np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(r, dtype=np.float32),
                     np.asarray(anchors_per_cav[c], dtype=np.float32), matrices[c]))
    return cavs, where


def conditions(out, require_candidates=True):
    """no decision on a rounding edge (the restatement's float64 diagnostics)"""
    assert out["score_margin"] >= 1e-4, out["score_margin"]
    if out["none"]:
        assert not require_candidates
        return
    assert out["score_gap"] >= 1e-5, out["score_gap"]
    assert out["filter_margin"] >= 1e-3, out["filter_margin"]
    assert out["iou_margin"] >= 1e-3, out["iou_margin"]
    assert out["range_margin"] >= 1e-3, out["range_margin"]


# ---------------------------------------------------------------------------------------------- A: 2 x 3 x 2 anchors, by hand
A_GRID = (2, 3)
A_MATRIX = matrix(0.0, [10.0, -5.0, 0.25])
# in the ego frame; ranks give the score order.  0 and 1 overlap (1 is suppressed), 2 stands alone, 3 is 7 m long, 4 pokes above
# z = 1, 5 lies beside 2 without touching it and is kept, 6 stays below the score threshold
A_DESIGNED = [
    (0, (12.0, -3.0, -1.0, 4.0, 2.0, 1.5, 0.0), 6),
    (0, (12.5, -2.8, -1.0, 4.0, 2.0, 1.5, 0.1), 5),
    (0, (2.0, -9.0, -1.1, 3.6, 1.8, 1.6, 0.8), 4),
    (0, (20.0, 0.0, -1.0, 7.0, 2.0, 1.5, 0.0), 3),
    (0, (16.0, -12.0, 0.4, 4.0, 2.0, 1.5, 0.0), 2),
    (0, (2.0, -5.9, -1.1, 3.6, 1.8, 1.6, 0.8), 1),
    (0, (5.0, 5.0, -1.0, 4.0, 2.0, 1.5, 0.3), None),
]
A_EXPECTED = [0, 2, 5]                                    # designed boxes that come out, in score order


def case_a(anchors, nothing=False):
    """anchors: generate_anchor_box() of anchor_params(A_GRID, 'hwl', 6.0, 4.0).  nothing: every logit below the threshold"""
    designed = [(c, b, None if nothing else r) for c, b, r in A_DESIGNED]
    return build("A", [anchors], [A_MATRIX], "hwl", designed)


# ---------------------------------------------------------------------------------------------- B: 16 x 16 x 2, two cavs
B_GRID = (16, 16)
B_HALF = (25.6, 25.6)
B_SEED = 0


def b_matrices(reflect=False):
    return [matrix(0.1, [1.5, -0.7, 0.05], 0.004), matrix(-2.0, [-12.0, 24.0, 0.1], -0.006, reflect)]


def b_clusters(seed=B_SEED):
    """-> [(centre x, centre y, yaw)] of the dozen clusters, and the procedural numbers their members are drawn from"""
    u = uniform("B.cluster", (12, 8, 8), seed)
    return [(-18.0 + 9.0 * (k % 5) + 2.0 * (k // 5), -14.0 + 9.0 * (k // 5), -math.pi + 2 * math.pi * u[k, 0, 7]) for k in range(12)], u


def b_designed(seed=B_SEED):
    """a dozen clusters of overlapping boxes with varied yaw spread over both cavs, and the special boxes"""
    out = []
    clusters, u = b_clusters(seed)
    for k, (cx, cy, yaw0) in enumerate(clusters):
        for j in range(4 + k % 4):
            r = u[k, j]
            box = (cx + 1.6 * (r[0] - 0.5), cy + 1.6 * (r[1] - 0.5), -1.0 + 0.2 * (r[2] - 0.5), L * (0.9 + 0.2 * r[3]), W * (0.9 + 0.2 * r[4]),
                   H * (0.9 + 0.2 * r[5]), yaw0 + 0.6 * (r[6] - 0.5))
            out.append(((k + j) % 2, box, 100 + 8 * k + j))
    n = len(out)
    ranks = permutation("B.rank", n, seed)
    out = [(c, b, 10 + int(ranks[i])) for i, (c, b, _) in enumerate(out)]
    # boxes over 6 m (x extent, y extent), boxes outside the z band
    out.append((0, (-20.0, 18.0, -1.0, 7.5, 1.6, 1.5, 0.05), 500))
    out.append((1, (-10.0, 18.0, -1.0, 7.0, 1.6, 1.5, 1.5), 501))
    out.append((0, (0.0, 18.0, 0.5, 3.9, 1.6, 1.56, 0.3), 502))
    out.append((1, (10.0, 18.0, -2.6, 3.9, 1.6, 1.56, -0.4), 503))
    # leaves GT_RANGE (|y| <= 40) only after projection - it lies well inside cav 1's own range - and, scored higher, suppresses an
    # in-range box; a second out-of-range box stands alone
    out.append((1, (-6.0, 39.9, -1.0, 3.9, 1.6, 1.56, 0.0), 600))
    out.append((1, (-6.0, 39.0, -1.0, 3.9, 1.6, 1.56, 0.0), 5))
    out.append((1, (6.0, 40.5, -1.0, 3.9, 1.6, 1.56, 0.2), 6))
    return out


B_SUPPRESSOR, B_SUPPRESSED = -3, -2                       # positions of that pair in b_designed()


def case_b(anchors, order, reflect=False):
    mats = b_matrices(reflect)
    return build("B", [anchors, anchors], mats, order, b_designed())


# ---------------------------------------------------------------------------------------------- C: 24 x 32 x 2, the cut at 1000
C_GRID = (24, 32)
C_HALF = (51.2, 38.4)
C_MATRIX = matrix(0.0, [0.3, -0.2, 0.02], 0.002)
C_CANDIDATES = 1250


def case_c(anchors):
    """1250 of the 1536 anchors carry their own box, slightly moved (every pair IoU stays near 0, 0.085 or 0.26); the ladder puts
    the 1000th and the 1001st score 2e-3 logits apart"""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    n = len(a)
    u = uniform("C.jitter", (n, 7))
    chosen = np.sort(permutation("C.chosen", n)[:C_CANDIDATES])
    ranks = permutation("C.rank", C_CANDIDATES)
    logits = -4.0 + (LOGIT_THR - 0.3 + 4.0) * uniform("C.bg", (n,))
    ladder = np.linspace(LOGIT_THR + 0.3, 3.0, C_CANDIDATES)
    rm = np.zeros((n, 7))
    rm[:, :3] = 0.02 * (u[:, :3] - 0.5)
    rm[:, 3:6] = 0.04 * (u[:, 3:6] - 0.5)
    rm[:, 6] = 0.04 * (u[:, 6] - 0.5)
    logits[chosen] = ladder[ranks]
    rows, cols = C_GRID
    p = logits.reshape(rows, cols, 2).transpose(2, 0, 1)[None]
    r = rm.reshape(rows, cols, 14).transpose(2, 0, 1)[None]
    return [(np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(r, dtype=np.float32),
             np.asarray(anchors, dtype=np.float32), C_MATRIX)]


# ---------------------------------------------------------------------------------------------- D: rotated IoU, 40 x 24 quads
def rect(cx, cy, l, w, yaw, clockwise=False):
    c, s = math.cos(yaw), math.sin(yaw)
    pts = [(cx + c * dx - s * dy, cy + s * dx + c * dy) for dx, dy in ((l / 2, -w / 2), (l / 2, w / 2), (-l / 2, w / 2), (-l / 2, -w / 2))]
    return pts[::-1] if clockwise else pts


def case_d():
    """a (40, 4, 2), b (24, 4, 2) fp32: b[j] relates to a[j] - identical, identical with the other winding, touching along an edge,
    contained, containing, disjoint, then partial overlaps at varied yaw; coordinates up to 150, areas above 1"""
    u = uniform("D.a", (40, 6))
    a, b = [], []
    for i in range(40):
        cx, cy = -130.0 + 260.0 * u[i, 0], -38.0 + 76.0 * u[i, 1]
        if i == 2:
            cx, cy = 8.0, -4.0
        l, w, yaw = 2.0 + 4.0 * u[i, 2], 1.2 + 1.5 * u[i, 3], (0.0 if i == 2 else -math.pi + 2 * math.pi * u[i, 4])
        if i in (2, 3):
            l, w = 4.0, 2.0
        a.append(rect(cx, cy, l, w, yaw, clockwise=i % 3 == 1))
        if i < 24:
            v = uniform("D.b.%d" % i, (5,))
            if i == 0:
                q = rect(cx, cy, l, w, yaw, clockwise=False)
            elif i == 1:
                q = rect(cx, cy, l, w, yaw, clockwise=False)              # a[1] is clockwise: the same quad, other winding
            elif i == 2:
                q = rect(cx + l, cy, l, w, yaw)                           # shares the edge x = cx + l / 2 (axis-aligned, exact)
            elif i == 3:
                q = rect(cx, cy, 0.5 * l, 0.5 * w, yaw + 0.1)
            elif i == 4:
                q = rect(cx, cy, 3.0 * l, 3.0 * w, yaw - 0.2, clockwise=True)
            elif i == 5:
                q = rect(cx + 20.0, cy, l, w, yaw)
            else:
                q = rect(cx + 1.5 * (v[0] - 0.5), cy + 1.5 * (v[1] - 0.5), l * (0.8 + 0.4 * v[2]), w * (0.8 + 0.4 * v[3]),
                         yaw + 1.2 * (v[4] - 0.5), clockwise=i % 2 == 1)
            b.append(q)
    return np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)


# ---------------------------------------------------------------------------------------------- E: ground truth for case B
def case_e_gt():
    """10 ground-truth boxes (10, 8, 3) in the ego frame: eight near cluster centres of case B at varied offsets, two with no detection"""
    from detect_ref import boxes_to_corners
    import torch
    clusters, _ = b_clusters()
    u = uniform("E.gt", (10, 4))
    boxes = []
    for g in range(8):
        cx, cy, yaw0 = clusters[g + (g // 3)]
        boxes.append([cx + 1.0 * (u[g, 0] - 0.5), cy + 1.0 * (u[g, 1] - 0.5), -1.0, L, W, H, yaw0 + 0.3 * (u[g, 2] - 0.5)])
    boxes.append([30.0, -30.0, -1.0, L, W, H, 0.4])
    boxes.append([-35.0, 30.0, -1.0, L, W, H, -1.0])
    return boxes_to_corners(torch.tensor(boxes, dtype=torch.float64), "lwh", np.eye(4), torch.float64).numpy().astype(np.float32)


EVAL_IOUS = (0.3, 0.5, 0.7)


# ---------------------------------------------------------------------------------------------- box_utils.nms_rotated on its own
def case_nms(flat=False):
    """case B's designed boxes as given corners in the ego frame, (N, 8, 3) fp32 or with flat=True (N, 4, 2), with procedural scores of
    both signs (no two closer than 1e-5: a shuffled ladder)"""
    from detect_ref import boxes_to_corners
    import torch
    boxes = torch.tensor([b for _, b, _ in b_designed()], dtype=torch.float64)
    corners = boxes_to_corners(boxes, "lwh", np.eye(4), torch.float64).numpy().astype(np.float32)
    n = len(corners)
    scores = np.linspace(-1.0, 1.0, n)[permutation("nms.rank", n)].astype(np.float32)
    return (np.ascontiguousarray(corners[:, :4, :2]) if flat else corners), scores
