"""Float64 restatement of the reference's LiDAR BEV (PIXOR) pre- and post-processor - BevPreprocessor.preprocess,
LidarBevPostprocessor.generate_label and post_process - for tests/test_lidar_bev.py, tests/test_lidar_bev_gpu.py and
tests/golden/make_golden_bev.py.  numpy only.  Where the reference rounds to fp32 (the corners of boxes_to_corners_3d, the rotation
and projection of post_process) `faithful=True` rounds in the same places; `faithful=False` keeps float64 throughout.

Each function also returns the decision margins the case conditions are asserted on (tests/golden/cases_bev.py)."""
import numpy as np

import detect_ref as dr

GT_RANGE_XY = (140.0, 40.0)
F32 = np.float32


# ---------------------------------------------------------------------------------------------- preprocessor
def kept_mask(points, geom, lidar_range, range_mask=False, ego_mask=False):
    """the rule of csrc/bev_points.hip -> (kept (M,) bool, indices (M, 3) int64 (garbage where not kept), the smallest distance of a
    FINITE in-map coordinate to a cell boundary, in cells)"""
    p = np.asarray(points)
    assert p.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(p).all(axis=1) & (np.abs(p[:, 3]) < 256.0)
        origin = np.array([geom["L1"], geom["W1"], geom["H1"]], dtype=np.float64)
        q = (p[:, :3].astype(np.float64) - origin) / float(geom["res"])
        t = np.trunc(q)
        nx, ny, c = geom["input_shape"]
        hi = np.array([nx, ny, c - 1], dtype=np.float64)
        inside = ((t >= 0) & (t < hi)).all(axis=1)
        keep = finite & inside
        if range_mask:
            r = np.asarray(lidar_range, dtype=np.float32)
            keep &= ((p[:, :3] > r[:3]) & (p[:, :3] < r[3:])).all(axis=1)
        if ego_mask:
            keep &= ~((p[:, 0] >= F32(-1.95)) & (p[:, 0] <= F32(2.95)) & (p[:, 1] >= F32(-1.1)) & (p[:, 1] <= F32(1.1)))
        idx = np.where(keep[:, None], t, 0).astype(np.int64)
        fq = q[np.isfinite(q).all(axis=1) & ((q > -1.5) & (q < hi + 0.5)).all(axis=1)]
        margin = float(np.abs(fq - np.round(fq)).min()) if len(fq) else np.inf
    return keep, idx, margin


def bev_points(clouds, geom, lidar_range, range_mask=False, ego_mask=False):
    """clouds: one (M_a, 4) fp32 array per agent -> (N, C, nx, ny) float64: occupancy and the exact float64 mean intensity"""
    nx, ny, c = geom["input_shape"]
    out = np.zeros((len(clouds), nx, ny, c), dtype=np.float64)
    for a, p in enumerate(clouds):
        keep, idx, _ = kept_mask(p, geom, lidar_range, range_mask, ego_mask)
        idx, inten = idx[keep], p[keep, 3].astype(np.float64)
        out[a, idx[:, 0], idx[:, 1], idx[:, 2]] = 1.0
        total = np.zeros((nx, ny))
        count = np.zeros((nx, ny))
        np.add.at(total, (idx[:, 0], idx[:, 1]), inten)          # float64 sums of fp32 values below 256: error far below the gates
        np.add.at(count, (idx[:, 0], idx[:, 1]), 1.0)
        out[a, :, :, c - 1] = np.where(count > 0, total / np.maximum(count, 1.0), 0.0)
    return out.transpose(0, 3, 1, 2)


def intensity_bound(mean):
    """the kernel's stated bound against the exact mean: 2^-33 + 2^-24 |mean| (1 + 2^-20)"""
    return 2.0 ** -33 + 2.0 ** -24 * np.abs(mean) * (1.0 + 2.0 ** -20)


# ---------------------------------------------------------------------------------------------- labels
def corners_fp32(gt):
    """corners 0 .. 3 of boxes_to_corners_3d(order = 'lwh') as the reference's torch fp32 chain makes them: separately rounded fp32
    products and sums, cos / sin correctly rounded -> (n, 4, 2) fp32"""
    gt = np.asarray(gt, dtype=np.float32)
    out = np.zeros((len(gt), 4, 2), dtype=np.float32)
    for n, b in enumerate(gt):
        sx, sy = b[3] * F32(0.5), b[4] * F32(0.5)
        cs, sn = F32(np.cos(np.float64(b[6]))), F32(np.sin(np.float64(b[6])))
        for k, (tx, ty) in enumerate(((1, -1), (1, 1), (-1, 1), (-1, -1))):
            x, y = F32(tx) * sx, F32(ty) * sy
            out[n, k, 0] = F32(F32(x * cs) + F32(y * -sn)) + b[0]
            out[n, k, 1] = F32(F32(x * sn) + F32(y * cs)) + b[1]
    return out


def corners_f64(gt):
    gt = np.asarray(gt, dtype=np.float64)
    out = np.zeros((len(gt), 4, 2))
    for n, b in enumerate(gt):
        cs, sn = np.cos(b[6]), np.sin(b[6])
        for k, (tx, ty) in enumerate(((1, -1), (1, 1), (-1, 1), (-1, -1))):
            x, y = tx * b[3] / 2, ty * b[4] / 2
            out[n, k] = (x * cs - y * sn + b[0], x * sn + y * cs + b[1])
    return out


def generate_label(gt, mask, geom, mean, std, faithful=True):
    """gt (G, 7) with fp32-representable values, mask (G,) -> {'label_map' (7, lx, ly) float64 (before the cast to fp32),
    'bev_corners' (n, 4, 2) (fp32 when faithful), 'l_margin': the smallest distance of a DECIDING projection length to 0 or 1,
    'edge_hits': the number of pixels accepted with a length exactly 0 or 1}"""
    gt = np.asarray(gt, dtype=np.float64)
    valid = gt[np.asarray(mask) == 1]
    corners = corners_fp32(valid) if faithful else corners_f64(valid)
    res, rate = float(geom["res"]), geom["downsample_rate"]
    lx, ly, _ = geom["label_shape"]
    origin = np.array([geom["L1"], geom["W1"]], dtype=np.float64).reshape(1, -1)
    dist = (corners.astype(np.float64) - origin) / res / rate
    origin_dist = origin / res / rate
    ii, jj = np.meshgrid(np.arange(lx), np.arange(ly), indexing="ij")
    pts = np.stack([ii.reshape(-1), jj.reshape(-1)], axis=-1)
    label = np.zeros((lx, ly, 7))
    l_margin, edge_hits = np.inf, 0
    for n in range(len(valid)):
        c0, e1, e2 = dist[n, 0], dist[n, 1] - dist[n, 0], dist[n, 3] - dist[n, 0]
        n1, n2 = e1[0] * e1[0] + e1[1] * e1[1], e2[0] * e2[0] + e2[1] * e2[1]
        if not (n1 > 1e-6 and n2 > 1e-6):
            continue                                             # the reference asserts; the kernel skips the box
        rel = pts - c0.reshape(1, -1)
        l1 = (rel[:, 0] * e1[0] + rel[:, 1] * e1[1]) / n1
        l2 = (rel[:, 0] * e2[0] + rel[:, 1] * e2[1]) / n2
        in1, in2 = (l1 >= 0) & (l1 <= 1), (l2 >= 0) & (l2 <= 1)
        inside = in1 & in2
        for la, other in ((l1, in2), (l2, in1)):
            d = np.minimum(np.abs(la), np.abs(la - 1))[other]
            edge_hits += int((d[(la[other] >= 0) & (la[other] <= 1)] == 0).sum())
            d = d[d != 0]
            if len(d):
                l_margin = min(l_margin, float(d.min()))
        p_in = pts[inside]
        cont = (p_in + origin_dist) * res * rate
        yaw, x, y, dx, dy = valid[n, 6], valid[n, 0], valid[n, 1], valid[n, 3], valid[n, 4]
        tgt = np.repeat(np.array([np.cos(yaw), np.sin(yaw), x, y, dx, dy]).reshape(1, -1), len(p_in), axis=0)
        tgt[:, 2:4] = tgt[:, 2:4] - cont
        tgt[:, 4:] = np.log(tgt[:, 4:])
        label[p_in[:, 0], p_in[:, 1], 0] = 1.0
        label[p_in[:, 0], p_in[:, 1], 1:] = tgt
    label[..., 1:] = (label[..., 1:] - np.asarray(mean)) / np.asarray(std)
    return {"label_map": label.transpose(2, 0, 1), "bev_corners": corners, "l_margin": l_margin, "edge_hits": edge_hits}


# ---------------------------------------------------------------------------------------------- post_process
def decode(cls, reg, matrix, geom, mean, std, faithful):
    """cls (1, 1, lx, ly), reg (1, 6, lx, ly) fp32, matrix (4, 4) -> prob (lx ly,) and corners (lx ly, 4, 2) of EVERY pixel in (i, j)
    order; fp32 arrays when faithful, float64 otherwise"""
    cls, reg = np.asarray(cls), np.asarray(reg)
    lx, ly = cls.shape[2:]
    if faithful:
        x32 = cls.reshape(-1).astype(np.float32)
        prob = (F32(1) / (F32(1) + np.exp(-x32).astype(np.float32))).astype(np.float32)
    else:
        prob = 1.0 / (1.0 + np.exp(-cls.reshape(-1).astype(np.float64)))
    v = reg[0].reshape(6, -1).T.astype(np.float64) * np.asarray(std) + np.asarray(mean)
    yaw = np.arctan2(v[:, 1], v[:, 0])
    dx, dy = np.exp(v[:, 4]), np.exp(v[:, 5])
    cell = float(geom["res"]) * geom["downsample_rate"]
    gx, gy = geom["L1"] + np.arange(lx) * cell, geom["W1"] + np.arange(ly) * cell
    if faithful:
        gx, gy = gx.astype(np.float32).astype(np.float64), gy.astype(np.float32).astype(np.float64)
    cx, cy = np.repeat(gx, ly) + v[:, 2], np.tile(gy, lx) + v[:, 3]
    m = np.asarray(matrix)
    dt = np.float32 if faithful else np.float64
    out = np.zeros((lx * ly, 4, 2), dtype=dt)
    cs, sn, hx, hy, m = np.cos(yaw).astype(dt), np.sin(yaw).astype(dt), (dx * 0.5).astype(dt), (dy * 0.5).astype(dt), m.astype(dt)
    for k, (tx, ty) in enumerate(((1, -1), (1, 1), (-1, 1), (-1, -1))):
        x, y = dt(tx) * hx, dt(ty) * hy
        rx, ry = x * cs + y * -sn, x * sn + y * cs               # numpy keeps each operation in dt: separately rounded
        X, Y = (rx.astype(np.float64) + cx).astype(dt), (ry.astype(np.float64) + cy).astype(dt)
        for q in range(2):
            out[:, k, q] = m[q, 0] * X + m[q, 1] * Y + m[q, 3]
    return prob, out


def post_process(cavs, geom, mean, std, score_threshold, nms_thresh, faithful=True):
    """cavs: [(cls, reg, matrix)] -> {'none', 'boxes' (K, 4, 2), 'scores' (K), 'index' (K) global pixel indices in pick order,
    'candidates', 'picked_all' (before the range mask) and the margins 'score_margin', 'score_gap', 'iou_margin', 'range_margin'}"""
    corners, scores, index = [], [], []
    start, score_margin = 0, np.inf
    for cls, reg, matrix in cavs:
        prob, c = decode(cls, reg, matrix, geom, mean, std, faithful)
        score_margin = min(score_margin, float(np.abs(prob.astype(np.float64) - score_threshold).min()))
        above = (prob > (F32(score_threshold) if faithful else score_threshold)) & np.isfinite(c.reshape(len(c), -1)).all(axis=1)
        corners.append(c[above]); scores.append(prob[above]); index.append(np.nonzero(above)[0] + start)
        start += len(prob)
    corners, scores, index = np.concatenate(corners), np.concatenate(scores), np.concatenate(index)
    out = {"none": len(index) == 0, "score_margin": score_margin, "score_gap": np.inf, "iou_margin": np.inf, "range_margin": np.inf,
           "candidates": index.astype(np.int32)}
    if out["none"]:
        return out
    s = np.sort(scores.astype(np.float64))
    if len(s) > 1:
        out["score_gap"] = float(np.diff(s).min())
    picks, out["iou_margin"] = dr.nms_rotated(corners, scores, nms_thresh)
    picked = corners[picks]
    lim = np.array(GT_RANGE_XY)
    if len(picks):
        out["range_margin"] = float(np.abs(np.abs(picked.astype(np.float64)) - lim).min())
    inside = (np.abs(picked[:, :, 0]) <= GT_RANGE_XY[0]).all(1) & (np.abs(picked[:, :, 1]) <= GT_RANGE_XY[1]).all(1)
    sel = picks[inside]
    out["picked_all"] = index[picks].astype(np.int32)
    out["boxes"], out["scores"], out["index"] = corners[sel], scores[sel], index[sel].astype(np.int32)
    return out
