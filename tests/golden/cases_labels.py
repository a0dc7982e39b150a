"""The detection-target and detection-loss cases shared by make_golden_labels.py (gv27_detect_labels.npz), tests/test_detect_targets.py
and tests/test_detect_targets_gpu.py: procedural ground truth on small anchor grids (cobevt_amd.synth; inputs are never stored).

A ground-truth box is an anchor's own box, moved, resized and turned a little ("jittered"), so that it has ONE best anchor: with
bbox_overlaps' `+1` convention a freely placed rotated box usually contains several anchors' hulls at exactly the same IoU, and the
reference's choice among them is fp32 rounding noise.  `conditions(out)` asserts on the float64 restatement that no decision of a
host-level case sits on a rounding edge: no IoU within 1e-4 of a threshold, every valid gt's best and second-best IoU at least 1e-4
apart (or the best 0).  The seeds below were picked so that this holds.  Case T is the opposite on purpose - dense anchors, steeply
rotated boxes, ties everywhere - and is used at kernel level only, where the kernel is fed the reference's own fp32 standup boxes.

  case  grid        what it exercises
  c1    5x7x2       70 anchors: below one wave multiple; 3 gt in 5 slots
  c2    24x32x2     1536 anchors, several workgroups; plus the three designed boxes: `beyond` lies more than 1 m outside the grid
                    (best IoU 0: unassigned), `weak` has its best IoU below neg_threshold (its anchor is positive and not negative),
                    and `pair_lo` / `pair_hi` both exceed pos_threshold at one anchor whose max-IoU gt is the HIGHER index
  c3    37x41x2     3034 anchors, no dimension a multiple of anything: the per-gt maximum crosses workgroups; 11 gt in 16 slots
  c4    8x12x1      one anchor per cell
  c5    16x16x2     B = 3, 100 slots: no valid box, one valid box in slot 3 (a NON-PREFIX mask), all 100 valid
  T     20x24x2     0.8 m pitch, six boxes turned by 0.6 .. 1.2 rad: tie-heavy, kernel level only
"""
import numpy as np

from cobevt_amd import synth

POS_T, NEG_T = 0.6, 0.45
L, W, H = 3.9, 1.6, 1.56                                  # OPV2V's anchor
VW = 0.4
EPS32 = 2.0 ** -24

# name -> (grid rows, cols), anchor yaws in degrees, pitch in metres, slots per sample, seed
CASES = {
    "c1": ((5, 7), (0, 90), 1.6, 5, 0),
    "c2": ((24, 32), (0, 90), 1.6, 16, 0),
    "c3": ((37, 41), (0, 90), 1.6, 16, 0),
    "c4": ((8, 12), (0,), 1.6, 8, 0),
    "c5": ((16, 16), (0, 90), 1.6, 100, 1),
    "T": ((20, 24), (0, 90), 0.8, 8, 0),
    "e2e": ((8, 12), (0, 90), 1.6, 8, 0),       # the head maps' grid of the end-to-end GPU test: not in the fixture
}
HOST_CASES = ("c1", "c2", "c3", "c4", "c5")
C2_BEYOND, C2_WEAK, C2_PAIR_LO, C2_PAIR_HI = 0, 1, 2, 3    # slots of the designed boxes of c2
C2_WEAK_CELL, C2_PAIR_CELL = (5, 6), (17, 22)              # the (row, col) of the anchor (a = 0) each is designed against


def uniform(tag, shape, seed=0):
    return synth.procedural_input("labels." + tag, shape, seed, 0.0, 1.0).numpy().astype(np.float64)


def permutation(tag, n, seed=0):
    return np.argsort(uniform(tag + ".perm", (max(n, 1),), seed)[:n], kind="stable")


def anchor_params(name, order="hwl"):
    """VoxelPostprocessor's parameters for the case's anchor grid (centres `pitch` apart, symmetric about the origin)"""
    (rows, cols), yaws, pitch, _, _ = CASES[name]
    xh, yh = VW + pitch * (cols - 1) / 2.0, VW + pitch * (rows - 1) / 2.0
    args = dict(W=cols * 2, H=rows * 2, l=L, w=W, h=H, r=list(yaws), vw=VW, vh=VW, num=len(yaws),
                cav_lidar_range=[-xh, -yh, -3, xh, yh, 1])
    return dict(core_method="VoxelPostprocessor", anchor_args=args, order=order, nms_thresh=0.15,
                target_args=dict(score_threshold=0.2, pos_threshold=POS_T, neg_threshold=NEG_T))


def jittered(tag, anchors, n, seed, shift=(0.6, 0.5), turn=0.3):
    """n boxes, each the box of a distinct anchor moved by up to `shift` metres, resized by up to 10 % and turned by up to `turn` rad"""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    pick = permutation(tag + ".cell", len(a), seed)[:n]
    u = uniform(tag + ".u", (n, 7), seed)
    gt = a[pick].copy()
    gt[:, 0] += shift[0] * (2 * u[:, 0] - 1)
    gt[:, 1] += shift[1] * (2 * u[:, 1] - 1)
    gt[:, 2] += 0.2 * (u[:, 2] - 0.5)
    gt[:, 3:6] *= 0.9 + 0.2 * u[:, 3:6]
    gt[:, 6] += turn * (2 * u[:, 6] - 1)
    return gt


def _pad(gt, slots):
    out = np.zeros((slots, 7))
    out[:len(gt)] = gt
    mask = np.zeros(slots)
    mask[:len(gt)] = 1
    return out, mask


def case(name, anchors):
    """-> gt_box_center (B, slots, 7) float64 in 'hwl' order and mask (B, slots)"""
    _, _, _, slots, seed = CASES[name]
    a = np.asarray(anchors, dtype=np.float64)
    if name == "c1":
        gt, mask = _pad(jittered("c1", a, 3, seed), slots)
        return gt[None], mask[None]
    if name == "c2":
        own = lambda cell, dx, dy: a[cell[0], cell[1], 0] + np.array([dx, dy, 0.0, 0.0, 0.0, 0.0, 0.0])    # noqa: E731
        special = np.stack([np.array([a[..., 0].max() + 8.0, 0.3, -1.0, H, W, L, 0.2]),
                            own(C2_WEAK_CELL, 0.7, 0.78), own(C2_PAIR_CELL, 0.5, 0.2), own(C2_PAIR_CELL, 0.1, 0.05)])
        gt, mask = _pad(np.concatenate([special, jittered("c2", a, 8, seed)]), slots)
        return gt[None], mask[None]
    if name == "c3":
        gt, mask = _pad(jittered("c3", a, 11, seed), slots)
        return gt[None], mask[None]
    if name in ("c4", "e2e"):
        gt, mask = _pad(jittered(name, a, 4, seed), slots)
        return gt[None], mask[None]
    if name == "c5":
        gts = np.stack([jittered("c5.%d" % b, a, slots, seed + b, shift=(0.4, 0.3), turn=0.15) for b in range(3)])
        mask = np.zeros((3, slots))
        mask[1, 3] = 1
        mask[2] = 1
        return gts, mask
    if name == "T":
        u = uniform("T.u", (6, 4), seed)
        gt = np.zeros((6, 7))
        gt[:, 0] = (a[..., 0].min() + 2.0) + (a[..., 0].max() - a[..., 0].min() - 4.0) * u[:, 0]
        gt[:, 1] = (a[..., 1].min() + 2.0) + (a[..., 1].max() - a[..., 1].min() - 4.0) * u[:, 1]
        gt[:, 2] = -1.0
        gt[:, 3:6] = [H, W, L]
        gt[:, 6] = np.where(u[:, 2] < 0.5, -1.0, 1.0) * (0.6 + 0.6 * u[:, 3])
        gt, mask = _pad(gt, slots)
        return gt[None], mask[None]
    raise KeyError(name)


def compacted(gt, mask):
    """one sample's valid boxes moved to the front (a prefix mask): what the documented mask rule makes of a non-prefix mask"""
    valid = np.nonzero(mask == 1)[0]
    return _pad(gt[valid], len(gt))


def conditions(out):
    """no decision on a rounding edge (one sample's float64 restatement)"""
    assert out["threshold_margin"] >= 1e-4, out["threshold_margin"]
    assert out["best_gap"] >= 1e-4, out["best_gap"]


def c2_designed(out, anchors):
    """the designed boxes of c2 do what they were designed for (one sample's float64 restatement)"""
    iou, matched = out["iou"], out["matched"]
    cols, na = anchors.shape[1], anchors.shape[2]
    flat = lambda cell: (cell[0] * cols + cell[1]) * na                                       # noqa: E731
    assert iou[:, C2_BEYOND].max() == 0.0
    weak = flat(C2_WEAK_CELL)
    assert iou[:, C2_WEAK].argmax() == weak and 0.0 < iou[weak, C2_WEAK] < NEG_T - 1e-3
    assert matched[weak] == C2_WEAK and out["pos_equal_one"].reshape(-1)[weak] == 1 and out["neg_equal_one"].reshape(-1)[weak] == 0
    pair = flat(C2_PAIR_CELL)
    assert iou[pair, C2_PAIR_HI] > iou[pair, C2_PAIR_LO] + 0.05 > POS_T + 0.05
    assert matched[pair] == C2_PAIR_LO
    return weak, pair


# ---------------------------------------------------------------------------------------------- gates
def rel_dev(x, ref, scale):
    """max |x - ref| / (|ref| + scale)"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(x - ref) / (np.abs(ref) + scale)).max()) if ref.size else 0.0


def gate(dev):
    """the relative gate of a quantity from the recorded deviation of its fp32 restatement: 4 x the worst, the margin being there
    because device log / sin / division and summation order may differ from numpy's by a few ulps; never below 4 fp32 half-ulps
    (a restatement that happens to hit the reference's bits says nothing about how close another fp32 evaluation can come)"""
    return 4.0 * max(float(dev), EPS32)


# ---------------------------------------------------------------------------------------------- loss inputs
LOSS_ARGS = {"cls_weight": 1.0, "reg": 2.0}
LOSS_CASES = ("c2", "c5")                                   # B = 1; B = 3 with a sample without positives


def loss_inputs(name, pos_equal_one, targets):
    """head maps for the labels of a case -> psm (B, A, H, W), rm (B, 7A, H, W), targets (B, H, W, 7A), all fp32.
    rm = the targets plus noise of up to 0.3, so |d| lies on both sides of beta = 1 / 9; on the first positive anchors of the batch
    (where there are any): logits of +30 and -30 (also on the first two negatives), yaw differences of +3.5 and -4.0 rad (beyond
    +-pi), and one NaN target in a size component."""
    pos = np.asarray(pos_equal_one, dtype=np.float32)
    tg = np.array(targets, dtype=np.float32)
    b, h, w, a = pos.shape
    psm = (-4.0 + 6.0 * uniform("loss.%s.psm" % name, (b, h, w, a))).astype(np.float32)
    rm = (tg.astype(np.float64) + 0.3 * (2 * uniform("loss.%s.rm" % name, (b, h, w, 7 * a)) - 1)).astype(np.float32)
    flat_p, flat_r, flat_t = psm.reshape(-1), rm.reshape(-1, 7), tg.reshape(-1, 7)
    where_pos, where_neg = np.nonzero(pos.reshape(-1) > 0)[0], np.nonzero(pos.reshape(-1) == 0)[0]
    assert len(where_pos) >= 5 and len(where_neg) >= 2
    flat_p[where_pos[0]], flat_p[where_pos[1]], flat_p[where_neg[0]], flat_p[where_neg[1]] = 30.0, -30.0, 30.0, -30.0
    flat_r[where_pos[2], 6] = flat_t[where_pos[2], 6] + 3.5
    flat_r[where_pos[3], 6] = flat_t[where_pos[3], 6] - 4.0
    flat_t[where_pos[4], 3] = np.nan
    nchw = lambda t: np.ascontiguousarray(t.transpose(0, 3, 1, 2))                              # noqa: E731
    return nchw(psm), nchw(rm), tg
