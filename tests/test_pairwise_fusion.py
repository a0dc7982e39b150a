"""CPU side of the pairwise-fusion kernel tests (tests/test_pairwise_fusion_gpu.py): the float64 restatement tests/pairwise_ref.py
is tied to the oracle the model tests already trust, and the stress poses are shown to be decidable - every ROI sample sits far
enough from an in / out edge that fp32 coordinates cannot move it across, which is what makes "ROI bit-identical" a fair demand."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cobevt_amd import synth
from cobevt_amd.synth import procedural_input
import oracle.v2v as o_v2v
import pairwise_ref as pr


def _oracle_case():
    """the project's existing poses on a 32 x 32 map, the oracle's common head, and both in the ops' layout"""
    batch = synth.opv2v_batch(agents=3, cams=1, image=64, max_cav=5, batch=2)
    pw, rl = batch["pairwise_t_matrix"], batch["record_len"]
    args = {"resolution": 0.390625, "downsample_rate": 8}
    x = procedural_input("pwf.cpu.x", (6, 8, 32, 32))                                # (N, C, H, W)
    feats, lens, pm, roi = o_v2v._pairwise(x, rl, pw, args)
    nb, mask = pr.warp(x.permute(0, 2, 3, 1), pw, lens, 5, args["resolution"], args["downsample_rate"])
    return x, feats, lens, pm, roi, nb, mask


def _unflip_nhwc(t):
    """(n, C, W, H) of the reference's flipped layout -> (n, H, W, C)"""
    return t.flip(3).permute(0, 3, 2, 1)


def test_restatement_reproduces_the_oracle_warp_and_roi():
    x, feats, lens, pm, roi, nb, mask = _oracle_case()
    H = W = 32
    seen = 0
    for b, n in enumerate(lens):
        for i in range(n):
            _, o_nb = o_v2v._neighbours(feats[b], pm[b], i, n, H, W)
            ref = _unflip_nhwc(o_nb)                                                 # [j] = agent j in agent i's frame
            err = (nb[b, i, :n].float() - ref).abs().max().item()
            assert err <= 2e-5, "nb[%d, %d]: %.3e" % (b, i, err)                     # |x| <= 1; fp32 coordinates move by < 1e-5 cell
            o_mask = roi[b, :n, i, 0]                                                # multiplies the flipped-domain pixels
            assert torch.equal(mask[b, i, :n].float(), o_mask.flip(2).transpose(1, 2)), "roi[%d, %d]" % (b, i)
            seen += int(o_mask.sum())
        assert nb[b, n:].abs().max() == 0 and nb[b, :, n:].abs().max() == 0 and mask[b, n:].sum() == 0 and mask[b, :, n:].sum() == 0
    assert 0 < seen < 18 * H * W, "the ROI of the project's poses is neither empty nor full"


@pytest.mark.parametrize("mode", ["avg", "max"])
def test_restatement_reproduces_the_oracle_message_loop(mode):
    """v2vnet_fusion's inner loop with the message convolution split into its neighbour and ego halves, as the host does"""
    x, feats, lens, pm, roi, nb, mask = _oracle_case()
    C, H, W, L = 8, 32, 32, 5
    wt = procedural_input("pwf.cpu.msgw", (C, 2 * C, 3, 3)) * 0.2
    bias = procedural_input("pwf.cpu.msgb", (C,), 0, -0.3, 0.3)
    msg = torch.zeros(2, L, L, H, W, C)
    ego, want = torch.zeros(6, H, W, C), torch.zeros(6, H, W, C)
    off = 0
    for b, n in enumerate(lens):
        for i in range(n):
            f, o_nb = o_v2v._neighbours(feats[b], pm[b], i, n, H, W)
            m = F.conv2d(torch.cat([o_nb, f[i][None].repeat(n, 1, 1, 1)], dim=1), wt, bias, padding=1) * roi[b, :n, i]
            want[off + i] = _unflip_nhwc((m.mean(dim=0) if mode == "avg" else m.max(dim=0)[0])[None])[0]
            msg[b, i, :n] = _unflip_nhwc(F.conv2d(o_nb, wt[:, :C], None, padding=1))
            ego[off + i] = _unflip_nhwc(F.conv2d(f[i][None], wt[:, C:], bias, padding=1))[0]
        off += n
    got = pr.message_reduce(msg, ego, mask, lens, mode)
    assert (got.float() - want).abs().max().item() <= 1e-5 * want.abs().max().item()


@pytest.mark.parametrize("use_mask", [True, False])
def test_restatement_reproduces_the_oracle_softmax_loop(use_mask):
    """disconet_fusion's inner loop: oracle.v2v.pixel_weighted_fusion on [neighbour | ego], then (w * nb * mask).sum(0)"""
    x, feats, lens, pm, roi, nb, mask = _oracle_case()
    C, H, W, L = 8, 32, 32, 5
    sd, cin = {}, 2 * C
    for k, cout in (("1_1", 8), ("1_2", 4), ("1_3", 4), ("1_4", 1)):
        sd["p.conv%s.weight" % k] = procedural_input("pwf.cpu.w" + k, (cout, cin, 1, 1))
        sd["p.conv%s.bias" % k] = procedural_input("pwf.cpu.b" + k, (cout,), 0, -0.2, 0.6)
        if k != "1_4":
            sd["p.bn%s.weight" % k], sd["p.bn%s.bias" % k] = torch.ones(cout), torch.zeros(cout)
            sd["p.bn%s.running_mean" % k], sd["p.bn%s.running_var" % k] = torch.zeros(cout), torch.ones(cout)
        cin = cout
    score = torch.zeros(2, L, L, H, W)
    want = torch.zeros(6, H, W, C)
    off = 0
    for b, n in enumerate(lens):
        for i in range(n):
            f, o_nb = o_v2v._neighbours(feats[b], pm[b], i, n, H, W)
            cat = torch.cat([o_nb, f[i][None].repeat(n, 1, 1, 1)], dim=1)
            m = roi[b, :n, i]
            wgt = o_v2v.pixel_weighted_fusion(sd, "p.", cat, m if use_mask else None)
            want[off + i] = _unflip_nhwc((wgt * o_nb * m).sum(0)[None])[0]
            score[b, i, :n] = _unflip_nhwc(F.relu(_scores(sd, cat)))[..., 0]
        off += n
    assert score.max() > 0 and (score == 0).any()
    got = pr.softmax_sum(score, nb, mask, lens, use_mask)
    assert (got.float() - want).abs().max().item() <= 2e-5 * want.abs().max().item()


def _scores(sd, x):
    """the pre-softmax, pre-ReLU score of pixel_weighted_fusion (identity BatchNorms)"""
    y = x
    for k in ("1_1", "1_2", "1_3"):
        y = F.relu(F.batch_norm(F.conv2d(y, sd["p.conv%s.weight" % k], sd["p.conv%s.bias" % k]), sd["p.bn%s.running_mean" % k],
                                sd["p.bn%s.running_var" % k], sd["p.bn%s.weight" % k], sd["p.bn%s.bias" % k], False, 0.0, 1e-5))
    return F.conv2d(y, sd["p.conv1_4.weight"], sd["p.conv1_4.bias"])


def test_gru_zero_is_the_oracle_gru_step_without_its_convolutions():
    """conv_gru_step with h = 0 reduces to sigmoid(beta) * tanh(candidate); pinned with identity-like 3x3 convolutions"""
    c = 4
    x = procedural_input("pwf.cpu.gru", (1, 2 * c, 5, 5), 0, -6, 6)                  # [update | candidate] pre-activations
    gates = torch.zeros(2 * c, 3 * c, 3, 3)                                          # comb = [x (2c) | h (c)]; gates -> [gamma | beta]
    can = torch.zeros(c, 3 * c, 3, 3)
    for k in range(c):
        gates[c + k, k, 1, 1] = 1.0                                                  # beta_k = x_k
        can[k, c + k, 1, 1] = 1.0                                                    # candidate_k = x_{c + k}
    sd = {"g.cell_list.0.conv_gates.weight": gates, "g.cell_list.0.conv_gates.bias": torch.zeros(2 * c),
          "g.cell_list.0.conv_can.weight": can, "g.cell_list.0.conv_can.bias": torch.zeros(c)}
    want = o_v2v.conv_gru_step(sd, "g.", x)
    got = pr.gru_zero(x.permute(0, 2, 3, 1))
    assert (got.float() - want.permute(0, 2, 3, 1)).abs().max().item() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# the stress poses
# ---------------------------------------------------------------------------------------------------------------------------
CASES = [(H, L, rl) for H in pr.SIZES for _, L, rl in pr.BATCHES]


@pytest.mark.parametrize("H,L,record_len", CASES)
def test_stress_poses_are_decidable(H, L, record_len):
    """A condition, not a tolerance: the nearest ROI sample is >= 1e-3 cell away from an in / out edge and fp32 evaluation moves a
    sample coordinate by <= 1e-5 cell, so no correct fp32 implementation can decide a ROI pixel differently from float64."""
    margin, diff = pr.margins(pr.stress_pairwise(L, record_len, H), H, pr.resolution(H), pr.DOWNSAMPLE)
    print("H=%d L=%d %s: smallest ROI margin %.3e cell, fp32-vs-fp64 coordinates %.3e cell" % (H, L, record_len, margin.min(), diff))
    assert margin.min().item() >= 1e-3
    assert diff <= 1e-5


@pytest.mark.parametrize("H", pr.SIZES)
def test_stress_poses_hide_no_failure_behind_a_degenerate_case(H):
    pw = pr.stress_pairwise(4, (4,), H)
    x = torch.ones(4, H, H, 1, dtype=torch.float64)
    _, roi = pr.warp(x, pw, (4,), 4, pr.resolution(H), pr.DOWNSAMPLE)
    cover = roi[0].mean(dim=(2, 3))                                                  # (i, j)
    off_diag = cover[~torch.eye(4, dtype=torch.bool)]
    assert torch.equal(cover.diagonal(), torch.ones(4, dtype=torch.float64)), "an agent sees all of its own map"
    assert ((off_diag > 0.1) & (off_diag < 0.9)).any(), "no pair is partly in view: %s" % off_diag
    assert (off_diag == 0).any(), "no pair is fully out of view: %s" % off_diag
    _, _, fx, fy = pr.sample_coords(pw[0].transpose(0, 1), H, pr.resolution(H), pr.DOWNSAMPLE)
    x0, y0 = torch.floor(fx), torch.floor(fy)
    oob = ((x0 < 0) | (x0 + 1 > H - 1) | (y0 < 0) | (y0 + 1 > H - 1)).reshape(4, 4, H, H)
    frac = oob[~torch.eye(4, dtype=torch.bool)].double().mean().item()               # the identity pairs are left out
    print("H=%d: ROI coverage %s, %.1f %% of the off-diagonal bilinear samples have an out-of-range tap" % (H, off_diag.tolist(), 100 * frac))
    assert frac >= 0.10


# ---------------------------------------------------------------------------------------------------------------------------
# resize_nhwc, nearest
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", pr.RESIZES)
def test_nearest_resize_sources_agree_in_fp32_and_float64(src, dst):
    """The kernel picks source min(floor(dst * (in / out)), in - 1) in fp32; F.interpolate's float64 pick is floor(dst * in / out).
    Only where the two agree for every destination index may the GPU test demand that nearest resizing is exact."""
    for n_in, n_out in zip(src, dst):
        i32 = np.floor(np.arange(n_out, dtype=np.float32) * (np.float32(n_in) / np.float32(n_out))).astype(np.int64)
        i64 = np.floor(np.arange(n_out, dtype=np.float64) * n_in / n_out).astype(np.int64)
        assert np.array_equal(np.minimum(i32, n_in - 1), i64), "%d -> %d: fp32 and float64 pick different sources" % (n_in, n_out)
