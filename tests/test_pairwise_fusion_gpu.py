"""Kernel-level tests of the pairwise-fusion glue kernels (csrc/pairwise_fusion.hip: pairwise_warp, pairwise_warp_bwd,
agent_message_reduce, gru_zero_state, agent_softmax_sum) and of three lone element-wise entry points (invert_small, resize_nhwc,
channel_affine), each against a float64 computation of the same operation on the operands the kernel sees (bf16 mode: inputs
rounded to bf16 first).

The reference of the pairwise kernels is tests/pairwise_ref.py; tests/test_pairwise_fusion.py ties it to the oracle and shows that
the stress poses used here are decidable (ROI margin >= 1e-3 cell, fp32 coordinates within 1e-5 cell of float64), which is what
entitles the ROI comparison to demand bit-identity.

Gates.  fp32: 2e-4 of the scale, bf16 (reduce, GRU, softmax, resize): 1e-2 of the scale - the project's kernel gates (`tol()` in
tests/test_kernels_gpu.py).  Warp in bf16: |err| <= 2^-8 |ref| + 2e-4 scale per element: the kernel accumulates in fp32 and rounds
once to nearest - half a bf16 ulp, which is 2^-9 |ref| at the top of a binade and 2^-8 |ref| at its bottom - plus the fp32 term; a
correct kernel can therefore sit close to this gate, a truncating one cannot pass it.  invert_small: 2^-23 max|inv| per matrix (fp64 arithmetic, one rounding to fp32);
channel_affine: 2^-23 (|x scale| + |ref|) (one fp32 rounding of a fused or an unfused multiply-add).  None comes from the code
under test; every comparison prints measured / gate (pytest -s) and enters the run's gate-headroom summary.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cobevt_amd import autograd as ag
from cobevt_amd import ops
from cobevt_amd.lib import CobevtHipError
from cobevt_amd.synth import _CAM2EGO_AXES, _rz, _trans, procedural_input
import pairwise_ref as pr
from util import GATE_RATIOS

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
F64 = torch.float64
NAN = float("nan")


def tol(dtype):
    return 2e-4 if dtype == torch.float32 else 1e-2


def rnd(t, dtype):
    """value the kernel actually sees (bf16 rounding of operands in bf16 mode)"""
    return t.to(dtype).to(torch.float32)


def gate(got, ref, bound, what):
    """|got - ref| <= bound element by element (bound: a positive number or tensor); prints and records measured / gate"""
    got = got.detach().to(F64).cpu()
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), "%s: non-finite output" % what
    err = (got - ref).abs()
    ratio = (err / bound).max().item()
    k = int((err / bound).argmax())
    measured = err.reshape(-1)[k].item()
    allowed = measured / ratio if ratio > 0 else float(torch.as_tensor(bound).min())
    print("%s: worst |err| %.3e at a gate of %.3e (ratio %.3f)" % (what, measured, allowed, ratio))
    GATE_RATIOS.append((ratio, "max", measured, allowed, what, os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]))
    assert ratio <= 1.0, "%s: |err| %.3e > %.3e" % (what, measured, allowed)
    return ratio


def warp_bound(ref, scale, dtype):
    return 2e-4 * scale if dtype == torch.float32 else 2.0 ** -8 * ref.abs() + 2e-4 * scale


def _rl(record_len, cuda):
    return torch.tensor(record_len, dtype=torch.int32, device=cuda)


def _valid(B, L, record_len):
    """(B, L, L) bool: i < N_b and j < N_b"""
    n = torch.tensor(record_len)[:, None]
    a = torch.arange(L)[None] < n
    return a[:, :, None] & a[:, None, :]


# ---------------------------------------------------------------------------------------------------------------------------
# pairwise_warp
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,L,record_len", pr.BATCHES)
@pytest.mark.parametrize("C", [8, 128, 512])                                         # G = 1, 16, 64 channel groups
@pytest.mark.parametrize("H", pr.SIZES)
def test_pairwise_warp_features_and_roi(cuda, H, C, B, L, record_len, dtype):
    N = sum(record_len)
    res, ds = pr.resolution(H), pr.DOWNSAMPLE
    pw = pr.stress_pairwise(L, record_len, H)
    x = rnd(procedural_input("pwf.x.%d.%d.%d" % (H, C, N), (N, H, H, C)), dtype)
    nb, roi = ops.pairwise_warp(x.to(cuda).to(dtype), pw.to(cuda), _rl(record_len, cuda), L, res, ds)
    torch.cuda.synchronize()
    ref_nb, ref_roi = pr.warp(x, pw, record_len, L, res, ds)
    what = "pairwise_warp H%d C%d %s %s" % (H, C, record_len, dtype)
    bad = roi.cpu().to(F64) != ref_roi
    assert not bad.any(), "%s: ROI differs in %d cells, first at (b, i, j, h, w) = %s" % (what, bad.sum(), bad.nonzero()[0].tolist())
    scale = x.abs().max().item()
    gate(nb, ref_nb, warp_bound(ref_nb, scale, dtype), what + " nb")
    pad = ~_valid(B, L, record_len)
    assert (nb.cpu()[pad] == 0).all() and (roi.cpu()[pad] == 0).all(), "%s: a padded pair is not exactly zero" % what
    # the pair (i, i) carries the identity matrix: the whole map is in view and comes back as it went in.  The sample coordinates
    # are within 1e-5 cell of the integers (tests/test_pairwise_fusion.py) and |x| changes by at most 2 scale per cell: 2e-5 scale,
    # plus the output rounding in bf16.
    ego = [(b, i) for b, n in enumerate(record_len) for i in range(n)]               # agent row off_b + i, in order
    assert all((roi[b, i, i] == 1).all() for b, i in ego), "%s: an ego ROI has holes" % what
    xi = x.to(F64)
    gate(torch.stack([nb[b, i, i] for b, i in ego]), xi, 2e-5 * scale + (0.0 if dtype == torch.float32 else 2.0 ** -8) * xi.abs(),
         what + " identity pairs")


def test_pairwise_warp_refuses_unsupported_shapes(cuda):
    """G = C / 8 must be a power of two <= 64 and the maps square: the entry point returns its shape error before any launch"""
    pw = pr.stress_pairwise(2, (2,), 4).to(cuda)
    rl = _rl((2,), cuda)
    for shape in ((2, 4, 4, 24), (2, 4, 4, 1024), (2, 4, 6, 8)):
        x = torch.zeros(shape, device=cuda)
        with pytest.raises(CobevtHipError, match="code 2"):
            ops.pairwise_warp(x, pw, rl, 2, pr.resolution(4), pr.DOWNSAMPLE)
        with pytest.raises(CobevtHipError, match="code 2"):
            leaf = x.clone().requires_grad_(True)
            ag.PairwiseWarpFn.apply(leaf, pw, rl, 2, pr.resolution(4), pr.DOWNSAMPLE)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,C,B,L,record_len", [(8, 8, 1, 4, (4,)), (5, 128, 3, 4, (3, 1, 2))])
def test_pairwise_warp_backward_vs_float64_autograd(cuda, H, C, B, L, record_len, dtype):
    """dx of autograd.PairwiseWarpFn element by element against torch.autograd through the float64 restatement.  fp32: the atomics
    change the summation order only (at most 4 L terms per element): 2e-4 of max|dx_ref|.  bf16: the reference takes the
    bf16-rounded dnb and dx is rounded once on the way out.  x carries one agent row more than record_len covers: no valid pair
    reads it, so its dx is exactly zero."""
    N = sum(record_len)
    res, ds = pr.resolution(H), pr.DOWNSAMPLE
    pw = pr.stress_pairwise(L, record_len, H)
    x = rnd(procedural_input("pwf.bx.%d.%d" % (H, C), (N + 1, H, H, C)), dtype)
    dnb = rnd(procedural_input("pwf.bg.%d.%d" % (H, C), (B, L, L, H, H, C)), dtype)     # non-zero in the padded slots too
    leaf = x.to(cuda).to(dtype).requires_grad_(True)
    with torch.enable_grad():
        nb = ag.PairwiseWarpFn.apply(leaf, pw.to(cuda), _rl(record_len, cuda), L, res, ds)
        nb.backward(dnb.to(cuda).to(dtype))
    torch.cuda.synchronize()
    dx = leaf.grad
    assert dx.dtype == dtype and dx.shape == leaf.shape
    xr = x.to(F64).requires_grad_(True)
    with torch.enable_grad():
        ref_nb, _ = pr.warp(xr, pw, record_len, L, res, ds)
        ref = torch.autograd.grad(ref_nb, xr, dnb.to(F64))[0]
    assert ref[:N].abs().max() > 0 and ref[N].abs().max() == 0
    what = "pairwise_warp_bwd H%d C%d %s %s" % (H, C, record_len, dtype)
    gate(dx, ref, warp_bound(ref, ref.abs().max().item(), dtype), what)
    assert (dx[N] == 0).all(), "%s: dx of an agent no valid pair reads is not exactly zero" % what


# ---------------------------------------------------------------------------------------------------------------------------
# agent_message_reduce, agent_softmax_sum, gru_zero_state
# ---------------------------------------------------------------------------------------------------------------------------
# (H, C, (B, L, record_len)): 100 work items (below one block), 4800 and 24576 (ragged / whole last block), G = 1, 16, 64
REDUCE_SHAPES = [(5, 8, pr.BATCHES[0]), (5, 128, pr.BATCHES[1]), (8, 512, pr.BATCHES[2]), (16, 128, pr.BATCHES[1]), (8, 8, pr.BATCHES[1])]


def _roi_pattern(key, B, L, H, record_len):
    """procedural 0 / 1 mask (B, L, L, H, H): ego pairs all 1, every non-ego source masked on the first map row, NaN in the
    padded slots"""
    roi = (procedural_input(key, (B, L, L, H, H), 0, 0, 1) > 0.45).float()
    eye = torch.eye(L, dtype=torch.bool)
    roi[:, ~eye, 0, :] = 0
    roi[:, eye] = 1
    roi[~_valid(B, L, record_len)] = NAN
    return roi


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["avg", "max"])
@pytest.mark.parametrize("H,C,batch", REDUCE_SHAPES)
def test_agent_message_reduce(cuda, H, C, batch, mode, dtype):
    """NaN in every padded slot of msg and roi: a finite result that equals the reference proves that the kernel never reads a
    padded slot and divides by N_b, not L.  msg + ego < 0 on the left half of the map: there a masked source's 0 wins the max."""
    B, L, record_len = batch
    N = sum(record_len)
    key = "pwf.red.%d.%d.%d" % (H, C, B)
    roi = _roi_pattern(key + ".roi", B, L, H, record_len)
    msg = rnd(procedural_input(key + ".msg", (B, L, L, H, H, C)), dtype)
    msg[~_valid(B, L, record_len)] = NAN
    ego = procedural_input(key + ".ego", (N, H, H, C))
    ego[:, :, :H // 2] -= 2.5                                                        # msg + ego in [-4.5, -0.5)
    ego = rnd(ego, dtype)
    out = ops.agent_message_reduce(msg.to(cuda).to(dtype), ego.to(cuda).to(dtype), roi.to(cuda), _rl(record_len, cuda), mode)
    torch.cuda.synchronize()
    ref = pr.message_reduce(msg, ego, roi, record_len, mode)
    if L > 1 and mode == "max":
        assert (ref[:, :, :H // 2] == 0).any(), "no pixel where a masked source's 0 wins the max"
    gate(out, ref, tol(dtype) * ref.abs().max().item(), "agent_message_reduce %s H%d C%d %s %s" % (mode, H, C, record_len, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use_mask", [True, False])
@pytest.mark.parametrize("H,C,batch", REDUCE_SHAPES)
def test_agent_softmax_sum(cuda, H, C, batch, use_mask, dtype):
    """score column 0: ReLU-like (exact zeros, ties on a 0.5 grid) with a band of 80 .. 100 that overflows exp without the
    max-subtraction; columns 1..7 and every padded slot of score, nb and roi hold NaN"""
    B, L, record_len = batch
    N = sum(record_len)
    key = "pwf.sm.%d.%d.%d" % (H, C, B)
    valid = _valid(B, L, record_len)
    roi = _roi_pattern(key + ".roi", B, L, H, record_len)
    s = (procedural_input(key + ".s", (B, L, L, H, H), 0, -2, 2).clamp_min(0) * 2).round() / 2
    band = procedural_input(key + ".band", (B, L, L, H, H), 0, 0, 1)
    s = torch.where(band > 0.7, 80 + (band * 40).round() / 2, s)                     # 94 .. 100 on 30 % of the entries
    s[:, :, :, 1, :] = 80 + (procedural_input(key + ".row", (B, L, L, H), 0, 0, 20)).round()      # a whole row inside the band
    s = rnd(s, dtype)
    assert (s == 0).any() and (s >= 80).any() and s.max() <= 100
    s[~valid] = NAN
    score = torch.full((B * L * L * H * H, 8), NAN)
    score[:, 0] = s.reshape(-1)
    nb = rnd(procedural_input(key + ".nb", (B, L, L, H, H, C)), dtype)
    nb[~valid] = NAN
    out = ops.agent_softmax_sum(score.to(cuda).to(dtype), nb.to(cuda).to(dtype), roi.to(cuda), _rl(record_len, cuda), N, use_mask)
    torch.cuda.synchronize()
    ref = pr.softmax_sum(s, nb, roi, record_len, use_mask)
    assert torch.isfinite(ref).all()
    gate(out, ref, tol(dtype) * ref.abs().max().item(), "agent_softmax_sum mask=%s H%d C%d %s %s" % (use_mask, H, C, record_len, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 128])
@pytest.mark.parametrize("rows", [1, 37, 400])
def test_gru_zero_state(cuda, rows, C, dtype):
    """[update | candidate] with different distributions in the two halves (update in [-6, 6), candidate in [-6, 1.5)), which pins
    the split, and +-30, +-87, +-100 planted in both: sigmoid and tanh saturate there and must stay finite.  Outputs lie in
    [-1, 1]: the gates are absolute."""
    x = torch.cat([procedural_input("pwf.gru.u.%d.%d" % (rows, C), (rows, C), 0, -6, 6),
                   procedural_input("pwf.gru.c.%d.%d" % (rows, C), (rows, C), 0, -6, 1.5)], dim=1)
    planted = torch.tensor([30.0, -30.0, 87.0, -87.0, 100.0, -100.0])
    x[0, 0:6] = planted                                                              # update half of the first row ...
    x[0, C + 2:C + 8] = planted.flip(0)                                              # ... and its candidate half, shifted by two
    x[rows - 1, C - 6:C] = -planted                                                  # the last row (the same row when rows = 1: every
    x[rows - 1, 2 * C - 8:2 * C - 2] = planted                                       # planted value still occurs in both halves)
    x = rnd(x, dtype)
    out = ops.gru_zero_state(x.to(cuda).to(dtype))
    torch.cuda.synchronize()
    assert out.shape == (rows, C)
    gate(out, pr.gru_zero(x), tol(dtype), "gru_zero_state rows%d C%d %s" % (rows, C, dtype))


# ---------------------------------------------------------------------------------------------------------------------------
# the lone element-wise entry points
# ---------------------------------------------------------------------------------------------------------------------------
def _small_matrices(n, d):
    """camera intrinsics, rz(yaw) trans cam->ego extrinsics (zero diagonal at yaw 0: the elimination must pivot), and matrices
    whose first pivot is in the last row"""
    u = procedural_input("pwf.inv.%d.%d" % (n, d), (n, d, d)).numpy().astype(np.float64)
    out = np.zeros((n, d, d))
    for k in range(n):
        kind = k % 3
        if kind == 0:
            m = _rz(90.0 * (k // 3) + (0.0 if k % 2 == 0 else 17.0 * k)) @ _trans(1.5 + u[k, 0, 0], u[k, 0, 1], 1.8) @ _CAM2EGO_AXES
            out[k] = m[:d, :d]
        elif kind == 1:
            f, m = 128.0 + 300.0 * abs(u[k, 0, 0]), np.eye(d)
            m[:3, :3] = [[f, 0, 256.0 + 20 * u[k, 0, 1]], [0, f * (1 + 0.1 * u[k, 1, 1]), 256.0 + 20 * u[k, 0, 2]], [0, 0, 1]]
            out[k] = m
        else:
            m = u[k] + np.eye(d)[::-1] * 0.5
            m[d - 1, 0] = 5.0
            out[k] = m
    return torch.from_numpy(out.astype(np.float32))


@pytest.mark.parametrize("d", [3, 4])
@pytest.mark.parametrize("n", [1, 65, 200])
def test_invert_small(cuda, n, d):
    m = _small_matrices(n, d)
    assert (m[0].diagonal()[:3] == 0).all(), "the first matrix has a zero diagonal in its rotation block"
    if n > 2:
        assert m[2, :, 0].abs().argmax() == d - 1, "the third matrix pivots on its last row"
    out = ops.invert_small(m.to(cuda))
    torch.cuda.synchronize()
    ref = torch.from_numpy(np.linalg.inv(m.numpy().astype(np.float64)))
    bound = 2.0 ** -23 * ref.abs().amax(dim=(1, 2), keepdim=True).expand_as(ref)
    gate(out, ref, bound, "invert_small n%d %dx%d" % (n, d, d))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 128])
@pytest.mark.parametrize("src,dst", pr.RESIZES)
@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
def test_resize_nhwc(cuda, mode, src, dst, C, dtype):
    (H, W), (Ho, Wo) = src, dst
    x = rnd(procedural_input("pwf.rs.%d.%d.%d" % (H, W, C), (2, H, W, C)), dtype)
    out = ops.resize_nhwc(x.to(cuda).to(dtype), Ho, Wo, mode)
    torch.cuda.synchronize()
    xc = x.to(F64).permute(0, 3, 1, 2)
    what = "resize_nhwc %s %s->%s C%d %s" % (mode, src, dst, C, dtype)
    if mode == "nearest":
        # fp32 and float64 pick the same source at every one of these sizes (tests/test_pairwise_fusion.py), so nearest is exact
        ref = F.interpolate(xc, size=(Ho, Wo), mode="nearest").permute(0, 2, 3, 1)
        assert torch.equal(out.cpu().to(F64), ref), "%s: nearest is not exact" % what
    else:
        ref = F.interpolate(xc, size=(Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        gate(out, ref, tol(dtype) * ref.abs().max().item(), what)


@pytest.mark.parametrize("N,C,HW", [(2, 3, 1000), (1, 5, 1)])
def test_channel_affine(cuda, N, C, HW):
    x = procedural_input("pwf.ca.x.%d" % HW, (N, C, HW), 0, -3, 3)
    scale = procedural_input("pwf.ca.s.%d" % HW, (C,), 0, 0.5, 4.0)
    shift = procedural_input("pwf.ca.b.%d" % HW, (C,), 0, -2, 2)
    out = ops.channel_affine(x.to(cuda), scale.to(cuda), shift.to(cuda))
    torch.cuda.synchronize()
    prod = x.to(F64) * scale.to(F64)[None, :, None]
    ref = prod + shift.to(F64)[None, :, None]
    bound = (2.0 ** -23 * (prod.abs() + ref.abs())).clamp_min(1e-300)
    gate(out, ref, bound, "channel_affine (%d, %d, %d)" % (N, C, HW))
