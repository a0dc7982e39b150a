"""Float64 restatement of what the pairwise-fusion glue kernels (cobevt_amd/csrc/pairwise_fusion.hip) compute, written the way the
reference does it (fusion_modules/v2v_fuse.py:72-144, disconet_fuse.py:35-42,106-168, torch_transformation_utils.py:77-134,254-355):
a Python loop over sample b, target agent i and source agents j, on a TRANSPOSED + FLIPPED copy of every map
('b c h w -> b c w h', flip), with a ROI mask that is NOT transposed / flipped, everything un-flipped at the very end.  It shares no
index algebra with the kernels, which work on the maps in their original orientation.

All tensors are channels-last and shaped like the arguments of the ops: x (N, H, W, C) un-grouped agent maps, pairwise
(B, L, L, 4, 4), nb / msg (B, L, L, H, W, C), roi (B, L, L, H, W), record_len a list of ints.  Every function computes in float64
(oracle.sttf.discretized_matrix casts to float32; here nothing does).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------------
# the affine warp of torch_transformation_utils.py, generic in the floating type
# ---------------------------------------------------------------------------------------------------------------------------
def _discretized(pairwise, res, ds, dtype):
    """:108-134 - rows 0..1, columns 0, 1, 3 of each 4x4 matrix, translation in feature cells; (..., 4, 4) -> (..., 2, 3)"""
    m = pairwise.to(dtype)[..., :2, :][..., [0, 1, 3]].clone()
    m[..., 2] = m[..., 2] / (res * ds)
    return m


def _recentred(M, H, W):
    """:254-297 - rotation about (W/2, H/2) plus translation; M (n, 2, 3)"""
    n = M.shape[0]
    eye = torch.eye(3, dtype=M.dtype).repeat(n, 1, 1)
    shift, shift_inv, rot = eye.clone(), eye.clone(), eye.clone()
    shift[:, 0, 2], shift[:, 1, 2] = W / 2, H / 2
    shift_inv[:, 0, 2], shift_inv[:, 1, 2] = -W / 2, -H / 2
    rot[:, :2, :2] = M[:, :, :2]
    T = (shift @ rot @ shift_inv)[:, :2, :].clone()
    T[:, :, 2] += M[:, :, 2]
    return T


def _normalise(H, W, dtype):
    """:160-191 - pixel coordinates -> [-1, 1]"""
    t = torch.eye(3, dtype=dtype)
    t[0, 0], t[1, 1] = 2.0 / (W - 1.0), 2.0 / (H - 1.0)
    t[0, 2] = t[1, 2] = -1.0
    return t[None]


def _grid(M, H, W):
    """:317-355 up to the sampling: the normalised grid_sample grid (n, H, W, 2) of warp_affine(src (n, ., H, W), M, (H, W))"""
    n = M.shape[0]
    M3 = torch.cat([M, torch.zeros(n, 1, 3, dtype=M.dtype)], dim=1)
    M3[:, 2, 2] = 1.0
    nrm = _normalise(H, W, M.dtype)
    theta = torch.inverse(nrm @ (M3 @ torch.inverse(nrm)))[:, :2, :]
    return F.affine_grid(theta, [n, 1, H, W], align_corners=True)


def _pixels(grid, H, W):
    """grid_sample's un-normalisation (align_corners=True): sample coordinates in cells, x along W and y along H"""
    return (grid[..., 0] + 1) / 2 * (W - 1), (grid[..., 1] + 1) / 2 * (H - 1)


def _warp_affine(src, M, mode):
    H, W = src.shape[-2:]
    return F.grid_sample(src, _grid(M, H, W), mode=mode, padding_mode="zeros", align_corners=True)


def _unflip(t):
    """back from the reference's layout: flip, '... w h -> ... h w'"""
    return t.flip(-1).transpose(-1, -2)


def _offsets(record_len):
    lens = [int(v) for v in record_len]
    offs = [sum(lens[:b]) for b in range(len(lens))]
    return lens, offs


# ---------------------------------------------------------------------------------------------------------------------------
# the five operations
# ---------------------------------------------------------------------------------------------------------------------------
def warp(x, pairwise, record_len, L, res, ds):
    """x (N, H, W, C) -> nb (B, L, L, H, W, C): nb[b, i, j] = agent j of sample b in agent i's frame, and roi (B, L, L, H, W): the mask
    value that multiplies output pixel (h, w) of that pair.  Zero where i >= N_b or j >= N_b.  Differentiable in x."""
    N, H, W, C = x.shape
    assert H == W, "the reference multiplies a (W, H) map by a (H, W) mask: square maps only"
    lens, offs = _offsets(record_len)
    B = len(lens)
    pm = _discretized(pairwise, res, ds, F64)                                        # (B, L, L, 2, 3)
    ones = torch.ones(1, 1, H, W, dtype=F64)
    xc = x.to(F64).permute(0, 3, 1, 2)                                               # (N, C, H, W)
    nb_rows, roi_rows = [], []
    for b in range(B):
        n = lens[b]
        f = xc[offs[b]:offs[b] + n].permute(0, 1, 3, 2).flip(3)                      # 'b c h w -> b c w h', flip
        for i in range(L):
            nb_i = torch.zeros(L, H, W, C, dtype=F64)
            roi_i = torch.zeros(L, H, W, dtype=F64)
            if i < n:
                M = pm[b, :n, i]                                                     # source j -> target i
                warped = _warp_affine(f, _recentred(M, H, W), "bilinear")            # (n, C, ., .) in the flipped layout
                mask = _warp_affine(ones.expand(n, 1, H, W), M, "nearest")           # (n, 1, H, W), not flipped, not re-centred
                nb_i = torch.cat([_unflip(warped).permute(0, 2, 3, 1), nb_i[n:]], dim=0)
                roi_i = torch.cat([_unflip(mask[:, 0]), roi_i[n:]], dim=0)
            nb_rows.append(nb_i)
            roi_rows.append(roi_i)
    return torch.stack(nb_rows).reshape(B, L, L, H, W, C), torch.stack(roi_rows).reshape(B, L, L, H, W)


def message_reduce(msg, ego, roi, record_len, mode):
    """v2v_fuse.py:108-119 with the message convolution split as the host does: out[off_b + i] = mean | max over the N_b agents of
    sample b of (msg[b, i, j] + ego[off_b + i]) * roi[b, i, j]"""
    lens, offs = _offsets(record_len)
    out = torch.zeros(ego.shape, dtype=F64)
    for b, n in enumerate(lens):
        for i in range(n):
            m = (msg[b, i, :n].to(F64) + ego[offs[b] + i].to(F64)[None]) * roi[b, i, :n].to(F64)[..., None]
            if mode == "avg":
                out[offs[b] + i] = m.mean(dim=0)
            elif mode == "max":
                out[offs[b] + i] = m.max(dim=0)[0]
            else:
                raise ValueError("agg_operator has wrong value")
    return out


def gru_zero(x):
    """convgru.py:57-78 with h_cur = 0: (1 - update) * 0 + update * tanh(candidate); x (..., 2C) = [update | candidate]"""
    c = x.shape[-1] // 2
    x = x.to(F64)
    return torch.sigmoid(x[..., :c]) * torch.tanh(x[..., c:])


def softmax_sum(score_col0, nb, roi, record_len, use_mask):
    """disconet_fuse.py:35-42,141-150: score_col0 (B, L, L, H, W) already ReLU'ed -> (N, H, W, C)"""
    lens, offs = _offsets(record_len)
    H, W, C = nb.shape[3:]
    out = torch.zeros(sum(lens), H, W, C, dtype=F64)
    for b, n in enumerate(lens):
        for i in range(n):
            mask = roi[b, i, :n].to(F64)[..., None]                                  # (n, H, W, 1)
            y = score_col0[b, i, :n].to(F64)[..., None]
            if use_mask:
                y = y.masked_fill(mask == 0, -float("inf"))
            w = y.softmax(dim=0)
            out[offs[b] + i] = (w * nb[b, i, :n].to(F64) * mask).sum(0)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# stress poses: large rotations, neighbours partly and wholly out of view (the models' tests stay within 2 cells of identity)
# ---------------------------------------------------------------------------------------------------------------------------
STRESS_POSES = ((0.0, 0.0, 0.0), (37.0, 11.0, -7.3), (-158.0, -9.0, 14.0), (95.0, 20.0, -16.0))      # (yaw deg, x m, y m)
# On the kernels' 32 x 32 production map these poses leave one ROI sample 3.2e-5 cell from an in / out edge, too close for fp32
# coordinates to decide.  At that size alone two poses are nudged (agent 1: y -7.3 -> -8.3 m, agent 2: y 14 -> 13.9 m), which moves
# the nearest sample to 2.6e-3 cell; tests/test_pairwise_fusion.py asserts the margin of every size.
STRESS_POSES_32 = (STRESS_POSES[0], (37.0, 11.0, -8.3), (-158.0, -9.0, 13.9), STRESS_POSES[3])
MAP_METRES, DOWNSAMPLE = 100.0, 8
SIZES = (5, 8, 16, 32)                                                               # H = W of the GPU warp test
BATCHES = ((1, 4, (4,)), (3, 4, (3, 1, 2)), (2, 1, (1, 1)))                          # (B, L, record_len) of the GPU tests
# ((H, W), (Ho, Wo)) of the GPU resize test; the CPU test shows fp32 and float64 pick the same nearest source at each
RESIZES = (((7, 5), (14, 10)), ((7, 5), (5, 9)), ((8, 8), (1, 1)), ((1, 1), (4, 4)), ((6, 10), (13, 7)))


def resolution(H):
    """metres per input cell so that the H x H feature map (downsample rate 8) is 100 m across"""
    return MAP_METRES / (DOWNSAMPLE * H)


def _pose(yaw, x, y):
    a = math.radians(yaw)
    c, s = math.cos(a), math.sin(a)
    rz = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    t = np.eye(4, dtype=np.float64)
    t[:2, 3] = (x, y)
    return rz @ t


def stress_poses(H):
    return STRESS_POSES_32 if H == 32 else STRESS_POSES


def stress_pairwise(L, record_len, H):
    """(B, L, L, 4, 4) fp32 for H x H maps as the dataset writes it (intermediate_fusion_dataset.py:110-150): pairwise[b, i, j] = inv(T_j) T_i for
    the valid agents of sample b, identity on the diagonal and in the padded slots.  Sample b takes the poses from the b-th on, so
    that the samples of a batch differ."""
    B, poses = len(record_len), stress_poses(H)
    pw = np.tile(np.eye(4, dtype=np.float64), (B, L, L, 1, 1))
    for b, n in enumerate(record_len):
        T = [_pose(*poses[(b + a) % len(poses)]) for a in range(n)]
        for i in range(n):
            for j in range(n):
                if i != j:
                    pw[b, i, j] = np.linalg.inv(T[j]) @ T[i]
    return torch.from_numpy(pw.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------
# how decidable a pose set is
# ---------------------------------------------------------------------------------------------------------------------------
def sample_coords(pairwise, H, res, ds, dtype=F64):
    """Sample coordinates in cells, evaluated in `dtype` from the start, of every pair matrix in `pairwise` (..., 4, 4):
    (roi_x, roi_y) of the nearest-neighbour ROI warp and (feat_x, feat_y) of the bilinear feature warp, each (P, H, H)."""
    m = _discretized(pairwise.reshape(-1, 4, 4), res, ds, dtype)
    return _pixels(_grid(m, H, H), H, H) + _pixels(_grid(_recentred(m, H, H), H, H), H, H)


def margins(pairwise, H, res, ds):
    """-> (margin (P, H, H), coord_diff): for every ROI sample coordinate its distance in cells to the nearest in / out decision
    edge (-0.5 or H - 0.5, on either axis: the nearest-neighbour sample is inside iff both rounded coordinates are in [0, H-1]), and
    the largest difference between float32 and float64 evaluation of the ROI and the feature sample coordinates.  The float32
    coordinates are torch's (`inverse` and `affine_grid` in float32); the kernel inverts its 2 x 2 block in closed form, which is
    other fp32 arithmetic with errors of the same order.  The 100 x ratio between margin and coordinate difference is therefore
    strong evidence that a correct fp32 implementation decides every ROI pixel as float64 does, not a proof for the device code:
    the GPU test still compares the ROI itself."""
    c64 = sample_coords(pairwise, H, res, ds, F64)
    c32 = sample_coords(pairwise, H, res, ds, torch.float32)
    rx, ry = c64[0], c64[1]
    edge = lambda t: torch.minimum((t + 0.5).abs(), (t - (H - 0.5)).abs())
    diff = max(float((a.to(F64) - b).abs().max()) for a, b in zip(c32, c64))
    return torch.minimum(edge(rx), edge(ry)), diff
