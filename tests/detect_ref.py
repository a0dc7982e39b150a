"""Restatement of the LiDAR detection output's specification (OpenCOOD's VoxelPostprocessor.post_process with the box_utils helpers
it calls, and eval_utils' matching), in torch on the CPU: the yardstick of tests/test_voxel_postprocess.py and
tests/test_voxel_postprocess_gpu.py, itself pinned to the reference's own run by tests/golden/gv24_voxel_postprocess.npz.

Every function takes `dt`: torch.float32 restates the reference's arithmetic (a chain of fp32 tensor operations), torch.float64 gives
the value the fp32 results are measured against.  The polygon arithmetic (the part the reference leaves to shapely) is always float64:
a Sutherland-Hodgman clip of one convex quad against another, written here independently of the kernel's and of the generator's
shapely stand-in.  `post_process` also returns every quantity a decision was taken on, so that the cases can assert that none of their
decisions sits on a rounding edge."""
import numpy as np
import torch

TOP = 1000
GT_RANGE_XY = (140.0, 40.0)


def delta_to_boxes3d(rm, anchors, dt):
    """rm (N, 7A, H, W), anchors (H, W, A, 7) -> (N, H W A, 7)"""
    rm = torch.as_tensor(rm).to(dt)
    n = rm.shape[0]
    d = rm.permute(0, 2, 3, 1).reshape(n, -1, 7)
    a = torch.as_tensor(anchors).to(dt).reshape(1, -1, 7)
    diag = torch.sqrt(a[..., 4] * a[..., 4] + a[..., 5] * a[..., 5])
    out = torch.zeros_like(d)
    out[..., 0] = d[..., 0] * diag + a[..., 0]
    out[..., 1] = d[..., 1] * diag + a[..., 1]
    out[..., 2] = d[..., 2] * a[..., 3] + a[..., 2]
    out[..., 3:6] = torch.exp(d[..., 3:6]) * a[..., 3:6]
    out[..., 6] = d[..., 6] + a[..., 6]
    return out


TEMPLATE = [[1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, -1], [1, -1, 1], [1, 1, 1], [-1, 1, 1], [-1, -1, 1]]


def boxes_to_corners(boxes, order, matrix, dt):
    """boxes (n, 7) -> (n, 8, 3) corners projected by the 4 x 4 matrix"""
    b = boxes.to(dt)
    sizes = b[:, [5, 4, 3]] if order == "hwl" else b[:, 3:6]
    t = torch.tensor(TEMPLATE, dtype=dt) / 2
    c = sizes[:, None, :] * t[None]
    cs, sn = torch.cos(b[:, 6])[:, None], torch.sin(b[:, 6])[:, None]
    x = c[..., 0] * cs + c[..., 1] * (-sn) + b[:, None, 0]
    y = c[..., 0] * sn + c[..., 1] * cs + b[:, None, 1]
    z = c[..., 2] + b[:, None, 2]
    m = torch.as_tensor(matrix).to(dt)
    return torch.stack([m[r, 0] * x + m[r, 1] * y + m[r, 2] * z + m[r, 3] for r in range(3)], dim=-1)


# ---------------------------------------------------------------------------------------------- float64 polygons
def _signed_area(p):
    x, y = p[:, 0], p[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def _clip(subject, a, b):
    """the part of the polygon `subject` (list of points) on the left of the directed line a -> b"""
    out = []
    ex, ey = b[0] - a[0], b[1] - a[1]
    side = [ex * (p[1] - a[1]) - ey * (p[0] - a[0]) for p in subject]
    for k in range(len(subject)):
        p, q = subject[k - 1], subject[k]
        sp, sq = side[k - 1], side[k]
        if (sq >= 0) != (sp >= 0):
            u = sp / (sp - sq)
            out.append((p[0] + u * (q[0] - p[0]), p[1] + u * (q[1] - p[1])))
        if sq >= 0:
            out.append(q)
    return out


def quad_iou(qa, qb):
    """IoU of two convex quads (4, 2) in float64, either winding; no union area -> 0"""
    qa, qb = np.asarray(qa, dtype=np.float64), np.asarray(qb, dtype=np.float64)
    area_a, area_b = _signed_area(qa), _signed_area(qb)
    if area_a < 0:
        qa, area_a = qa[::-1], -area_a
    if area_b < 0:
        qb, area_b = qb[::-1], -area_b
    poly = [tuple(p) for p in qa]
    for k in range(4):
        if len(poly) < 3:
            break
        poly = _clip(poly, qb[k], qb[(k + 1) % 4])
    inter = abs(_signed_area(np.asarray(poly))) if len(poly) >= 3 else 0.0
    union = area_a + area_b - inter
    return inter / union if union > 0 else 0.0


def iou_matrix(a, b):
    """a (N, >= 4, >= 2), b (M, >= 4, >= 2): corners 0 .. 3 in xy -> (N, M) float64; pairs with disjoint bounding boxes are 0"""
    a = np.asarray(a, dtype=np.float64)[:, :4, :2]
    b = np.asarray(b, dtype=np.float64)[:, :4, :2]
    out = np.zeros((len(a), len(b)))
    if len(a) == 0 or len(b) == 0:
        return out
    alo, ahi, blo, bhi = a.min(1), a.max(1), b.min(1), b.max(1)
    near = ((alo[:, None] < bhi[None]) & (blo[None] < ahi[:, None])).all(-1)
    for i, j in zip(*np.nonzero(near)):
        out[i, j] = quad_iou(a[i], b[j])
    return out


def nms_rotated(boxes, scores, threshold):
    """box_utils.nms_rotated -> (picked input rows in pick order, |iou - threshold| of the closest comparison made)"""
    boxes = np.asarray(boxes)
    scores = np.asarray(scores)
    n = len(scores)
    if n == 0:
        return np.zeros(0, dtype=np.int32), np.inf
    # descending score, lower index first among equal scores (the project's rule; the cases have no equal scores)
    order = np.lexsort((np.arange(n), -scores.astype(np.float64)))[:TOP]
    iou = iou_matrix(boxes[order], boxes[order])
    removed = np.zeros(len(order), dtype=bool)
    picks, margin = [], np.inf
    for i in range(len(order)):
        if removed[i]:
            continue
        picks.append(order[i])
        later = np.nonzero(~removed[i + 1:])[0] + i + 1
        if len(later):
            margin = min(margin, float(np.abs(iou[i, later] - threshold).min()))
            removed[later[iou[i, later].astype(np.float32) > np.float32(threshold)]] = True
    return np.asarray(picks, dtype=np.int32), margin


def post_process(cavs, score_threshold, nms_thresh, order, dt=torch.float32):
    """cavs: [(psm (1, A, H, W), rm (1, 7A, H, W), anchors (H, W, A, 7), matrix (4, 4))] ->
    {'none': nothing passed the score threshold, 'boxes' (K, 8, 3), 'scores' (K), 'index' (K) global anchor indices in pick order,
     'candidates': global indices that entered the selection, and the decision margins 'score_margin', 'score_gap', 'filter_margin',
     'iou_margin', 'range_margin'}"""
    corners, scores, index = [], [], []
    start, score_margin, filter_margin = 0, np.inf, np.inf
    any_above = False
    for psm, rm, anchors, matrix in cavs:
        psm = torch.as_tensor(psm).to(dt)
        prob = torch.sigmoid(psm.permute(0, 2, 3, 1)).reshape(-1)
        score_margin = min(score_margin, float((prob.double() - score_threshold).abs().min()))
        boxes = delta_to_boxes3d(rm, anchors, dt)[0]
        above = prob > score_threshold
        n_all = prob.numel()
        if bool(above.any()):
            any_above = True
            c = boxes_to_corners(boxes[above], order, matrix, dt)
            lo, hi = c.min(dim=1).values, c.max(dim=1).values
            x_len, y_len = hi[:, 0] - lo[:, 0], hi[:, 1] - lo[:, 1]
            # the reference's z_len is the y extent, used as a truth value
            keep = (x_len <= 6) & (y_len <= 6) & (y_len != 0) & (lo[:, 2] >= -3) & (hi[:, 2] <= 1)
            q = torch.stack([x_len - 6, y_len - 6, y_len, lo[:, 2] + 3, hi[:, 2] - 1], dim=1).double().abs()
            filter_margin = min(filter_margin, float(q.min()))
            corners.append(c[keep])
            scores.append(prob[above][keep])
            index.append(torch.nonzero(above).reshape(-1)[keep] + start)
        start += n_all
    out = {"none": not any_above, "score_margin": score_margin, "filter_margin": filter_margin, "score_gap": np.inf,
           "iou_margin": np.inf, "range_margin": np.inf}
    if not any_above:
        return out
    corners, scores, index = torch.cat(corners), torch.cat(scores), torch.cat(index)
    out["candidates"] = index.numpy().astype(np.int32)
    s = np.sort(scores.double().numpy())
    if len(s) > 1:
        out["score_gap"] = float(np.diff(s).min())
    picks, out["iou_margin"] = nms_rotated(corners.numpy(), scores.numpy(), nms_thresh)
    picked = corners[torch.from_numpy(picks.astype(np.int64))]
    xy = picked[:, :, :2].double().abs()
    lim = torch.tensor(GT_RANGE_XY, dtype=torch.float64)
    if len(picks):
        out["range_margin"] = float((xy - lim).abs().min())
    inside = (picked[:, :, 0].abs() <= GT_RANGE_XY[0]).all(1) & (picked[:, :, 1].abs() <= GT_RANGE_XY[1]).all(1)
    sel = torch.from_numpy(picks.astype(np.int64))[inside]
    out["boxes"], out["scores"], out["index"] = corners[sel].numpy(), scores[sel].numpy(), index[sel].numpy().astype(np.int32)
    out["suppressors_out_of_range"] = int((~inside).sum())
    return out


# ---------------------------------------------------------------------------------------------- eval_utils
def tp_fp(det_boxes, det_scores, gt_boxes, iou_thresh):
    """eval_utils.caluclate_tp_fp on one frame -> (fp list, tp list, gt count, |max iou - threshold| closest to 0)"""
    fp, tp, margin = [], [], np.inf
    gt = len(gt_boxes)
    if det_boxes is not None:
        iou = iou_matrix(det_boxes, gt_boxes).astype(np.float32)
        remaining = list(range(gt))
        for d in np.argsort(-np.asarray(det_scores)):
            row = iou[d, remaining]
            if len(remaining):
                margin = min(margin, abs(float(row.max()) - iou_thresh))
            if len(remaining) == 0 or row.max() < iou_thresh:
                fp.append(1)
                tp.append(0)
                continue
            fp.append(0)
            tp.append(1)
            remaining.pop(int(np.argmax(row)))
    return fp, tp, gt, margin


def average_precision(fp, tp, gt_total):
    """eval_utils.calculate_ap + voc_ap -> (ap, mrec, mpre)"""
    cfp, ctp = np.cumsum(fp).tolist(), np.cumsum(tp).tolist()
    rec = [0.0] + [float(t) / gt_total for t in ctp] + [1.0]
    pre = [0.0] + [float(t) / (f + t) for f, t in zip(cfp, ctp)] + [0.0]
    for i in range(len(pre) - 2, -1, -1):
        pre[i] = max(pre[i], pre[i + 1])
    ap = 0.0
    for i in range(1, len(rec)):
        if rec[i] != rec[i - 1]:
            ap += (rec[i] - rec[i - 1]) * pre[i]
    return ap, rec, pre
