"""Restatement of the detection targets (VoxelPostprocessor.generate_label with box_overlaps.bbox_overlaps) and of the PointPillar
detection loss, in numpy / torch, for fp32 and float64.  No GPU, no reference import.

numpy applies one correctly rounded operation per written operation and never fuses a multiply with an add, so `bbox_overlaps(...,
np.float32)` reproduces the compiled reference's mixed float / double arithmetic: the yardstick the kernel's IoU has to match bit for
bit.  The float64 runs carry the margins the fixture generator checks (tests/golden/cases_labels.py conditions)."""
import numpy as np
import torch

BETA = 1.0 / 9.0


def standup(boxes, dtype=np.float64):
    """(n, 7) 'hwl' boxes -> (n, 4) [x1, y1, x2, y2]: boxes_to_corners_3d + corner2d_to_standup_box, every operation in `dtype`"""
    b = np.asarray(boxes).astype(dtype).reshape(-1, 7)
    half = dtype(0.5)
    sx, sy = b[:, 5] * half, b[:, 4] * half
    cs, sn = np.cos(b[:, 6]), np.sin(b[:, 6])
    xs, ys = [], []
    for kx, ky in ((1, -1), (1, 1), (-1, 1), (-1, -1)):
        x, y = sx * dtype(kx), sy * dtype(ky)
        xs.append((x * cs + y * -sn) + b[:, 0])
        ys.append((x * sn + y * cs) + b[:, 1])
    xs, ys = np.stack(xs, 1), np.stack(ys, 1)
    return np.stack([xs.min(1), ys.min(1), xs.max(1), ys.max(1)], 1).astype(dtype)


def bbox_overlaps(boxes, query, dtype=np.float32):
    """box_overlaps.bbox_overlaps: (N, 4), (K, 4) -> (N, K) with the `+1` convention, operation by operation as the C that Cython
    generates from the reference's .pyx evaluates it on `dtype` = float32 boxes: a difference of two coordinates is a float
    operation, but the `+ 1` is written `+ 1.0`, a double - so the two areas and the union are formed in double from those float
    differences (with box_area and iw * ih rounded to float first) and rounded to float once; the final division is float."""
    f = dtype
    a = np.asarray(boxes).astype(f)[:, None, :]
    q = np.asarray(query).astype(f)[None, :, :]
    d = lambda x: x.astype(np.float64)                                                          # noqa: E731
    iw = (d(np.minimum(a[..., 2], q[..., 2]) - np.maximum(a[..., 0], q[..., 0])) + 1.0).astype(f)
    ih = (d(np.minimum(a[..., 3], q[..., 3]) - np.maximum(a[..., 1], q[..., 1])) + 1.0).astype(f)
    box_area = ((d(q[..., 2] - q[..., 0]) + 1.0) * (d(q[..., 3] - q[..., 1]) + 1.0)).astype(f)
    inter = iw * ih
    ua = ((d(a[..., 2] - a[..., 0]) + 1.0) * (d(a[..., 3] - a[..., 1]) + 1.0) + d(box_area) - d(inter)).astype(f)
    hit = (iw > 0) & (ih > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(hit, inter / np.where(hit, ua, f(1)), f(0))
    return out.astype(f).reshape(a.shape[0], q.shape[1])


def generate_label(gt_box_center, anchors, mask, pos_threshold, neg_threshold, dtype=np.float64, anchor_standup=None, gt_standup=None,
                   rule="first"):
    """-> dict: pos_equal_one (H, W, A), neg_equal_one (H, W, A), targets (H, W, 7A) in `dtype`, num_pos, matched (M,) the VALID index
    each positive anchor takes its box from (-1 elsewhere), iou (M, n) and the float margins.

    The rules of the operator: column k = the k-th valid box; highest anchor per gt = np.argmax, kept when its iou > 0; positive =
    any iou > pos_threshold or a kept highest; matched gt = the lowest k with iou > pos_threshold, else the lowest k the anchor is
    the kept highest of; negative = every iou < neg_threshold, cleared for kept highest anchors; targets from the matched VALID box.
    anchor_standup / gt_standup (valid boxes only): use these standup boxes instead of computing them.  rule="max" matches a
    positive anchor to its max-iou gt instead: NOT the reference's rule, there for the test that tells the two apart."""
    anchors = np.asarray(anchors)
    h, w, a = anchors.shape[:3]
    m = h * w * a
    an = anchors.reshape(m, 7).astype(dtype)
    valid = np.nonzero(np.asarray(mask) == 1)[0]
    gt = np.asarray(gt_box_center).astype(dtype)[valid]
    n = len(gt)
    ast = standup(an, dtype) if anchor_standup is None else np.asarray(anchor_standup)
    gst = standup(gt, dtype) if gt_standup is None else np.asarray(gt_standup)
    iou = bbox_overlaps(ast, gst.reshape(n, 4), dtype)
    pos_t, neg_t = dtype(pos_threshold), dtype(neg_threshold)
    matched = np.full(m, -1, dtype=np.int64)
    highest = np.zeros(m, dtype=bool)
    gap = np.inf
    if n:
        id_highest = np.argmax(iou, axis=0)
        best = iou[id_highest, np.arange(n)]
        for k in range(n - 1, -1, -1):                 # descending, so that the lowest k is written last
            if best[k] > 0:
                matched[id_highest[k]] = k
                highest[id_highest[k]] = True
        if m > 1:
            part = np.sort(iou, axis=0)
            gaps = np.where(part[-1] > 0, part[-1] - part[-2], np.inf)
            gap = float(gaps.min())
        over = iou > pos_t
        first = np.where(over.any(1), over.argmax(1), -1)
        if rule == "max":
            first = np.where(over.any(1), iou.argmax(1), -1)
        matched = np.where(first >= 0, first, matched)
    positive = matched >= 0
    negative = (iou < neg_t).all(1) & ~highest
    targets = np.zeros((m, 7), dtype=dtype)
    if positive.any():
        g, p = gt[matched[positive]], an[positive]
        d = np.sqrt(p[:, 4] ** 2 + p[:, 5] ** 2)
        targets[positive] = np.stack([(g[:, 0] - p[:, 0]) / d, (g[:, 1] - p[:, 1]) / d, (g[:, 2] - p[:, 2]) / p[:, 3],
                                      np.log(g[:, 3] / p[:, 3]), np.log(g[:, 4] / p[:, 4]), np.log(g[:, 5] / p[:, 5]),
                                      g[:, 6] - p[:, 6]], 1)
    margin = float(min(np.abs(iou - pos_t).min(), np.abs(iou - neg_t).min())) if n else np.inf
    return {"pos_equal_one": positive.astype(dtype).reshape(h, w, a), "neg_equal_one": negative.astype(dtype).reshape(h, w, a),
            "targets": targets.reshape(h, w, 7 * a), "num_pos": int(positive.sum()), "matched": matched, "iou": iou,
            "threshold_margin": margin, "best_gap": gap, "anchor_standup": ast, "gt_standup": gst}


def generate_label_batch(gt, mask, anchors, pos_threshold, neg_threshold, dtype=np.float64):
    outs = [generate_label(g, anchors, k, pos_threshold, neg_threshold, dtype) for g, k in zip(gt, mask)]
    return {k: np.stack([o[k] for o in outs]) for k in ("pos_equal_one", "neg_equal_one", "targets", "num_pos")}


def point_pillar_loss(psm, rm, pos_equal_one, targets, cls_weight, reg):
    """upstream OpenCOOD's PointPillarLoss on torch tensors, in their dtype, differentiable in psm / rm -> (total, conf_loss, reg_loss).
    psm (B, A, H, W), rm (B, 7A, H, W), pos_equal_one (B, H, W, A), targets (B, H, W, 7A)"""
    b = psm.shape[0]
    x = psm.permute(0, 2, 3, 1).reshape(b, -1)
    t = pos_equal_one.reshape(b, -1).to(x.dtype)
    positives = (t > 0).to(x.dtype)
    p_b = torch.clamp(positives.sum(1, keepdim=True), min=1.0)
    bce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-torch.abs(x)))
    sig = torch.sigmoid(x)
    pt = t * (1.0 - sig) + (1.0 - t) * sig
    conf = (0.25 * t + 0.75 * (1.0 - t)) * pt * pt * bce / p_b
    conf_loss = cls_weight * conf.sum() / b
    r = rm.permute(0, 2, 3, 1).reshape(b, -1, 7)
    g = targets.reshape(b, -1, 7).to(x.dtype)
    pred = torch.cat([r[..., :6], torch.sin(r[..., 6:]) * torch.cos(g[..., 6:])], -1)
    tgt = torch.cat([g[..., :6], torch.cos(r[..., 6:]) * torch.sin(g[..., 6:])], -1)
    tgt = torch.where(torch.isnan(tgt), pred, tgt)
    d = pred - tgt
    ad = torch.abs(d)
    l1 = torch.where(ad < BETA, 0.5 * d * d / BETA, ad - 0.5 * BETA)
    reg_loss = reg * (l1 * (positives / p_b)[..., None]).sum() / b
    return conf_loss + reg_loss, conf_loss, reg_loss


def loss_and_grads(psm, rm, pos_equal_one, targets, cls_weight, reg, dtype=torch.float64):
    """numpy in -> ([total, conf, reg], d total / d psm, d total / d rm) as numpy, computed in `dtype` by autograd"""
    with torch.enable_grad():
        p = torch.tensor(np.asarray(psm), dtype=dtype, requires_grad=True)
        r = torch.tensor(np.asarray(rm), dtype=dtype, requires_grad=True)
        total, conf, regl = point_pillar_loss(p, r, torch.tensor(np.asarray(pos_equal_one), dtype=dtype),
                                              torch.tensor(np.asarray(targets), dtype=dtype), cls_weight, reg)
        total.backward()
    return np.array([total.item(), conf.item(), regl.item()]), p.grad.numpy(), r.grad.numpy()
