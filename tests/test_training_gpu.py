"""Gradient parity of the training slice (-m gpu): train()-mode HIP forward + backward kernels against torch autograd through the
CPU oracle (oracle/ restates the reference modules functionally, so autograd through it is the reference's own training
graph, train_camera.py:143-179) on the gv2 / gv5 / gv9 golden cases.  fp32, tolerance 1e-3 of each tensor's scale."""
import numpy as np
import pytest
import torch

import cases
from cobevt_amd import autograd as ag
from cobevt_amd import host, ops, synth
from cobevt_amd.lib import CobevtHipError
from cobevt_amd.synth import fill_module_
import oracle.fax as o_fax
import oracle.swap_fusion as o_swap
from util import assert_close, focal_reference, golden

pytestmark = pytest.mark.gpu
TOL = 1e-3


def _train_module(m, cuda):
    return fill_module_(m, cases.SEED).train().to(cuda)


def _oracle_sd(m):
    """CPU leaf copies of the module's parameters (requires_grad) + its buffers, keyed like the state_dict"""
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    for k, p in m.named_parameters():
        sd[k] = p.detach().cpu().clone().requires_grad_(True)
    return sd


def _compare(m, sd, out, out_ref, inputs, inputs_ref, what, grad_tol=TOL, rms_tol=None):
    """backward of sum(out * w) on both sides, then outputs, input gradients and every parameter gradient.  rms_tol: additionally (and
    with a looser max-norm grad_tol) gate ||got - ref||_2 / ||ref||_2 per tensor - the metric for deep ReLU networks, see the caller"""
    w = synth.procedural_input("train.w." + what, tuple(out_ref.shape), cases.SEED)
    (out_ref * w).sum().backward()
    (out * w.to(out.device)).sum().backward()
    assert_close(out, out_ref, TOL, what + " forward")
    for i, (a, b) in enumerate(zip(inputs, inputs_ref)):
        if b is not None and b.grad is not None:
            assert_close(a.grad, b.grad, TOL, "%s d input %d" % (what, i))
    n = 0
    # a gradient that is analytically zero (e.g. the key LayerNorm's bias: softmax ignores a constant added to every key) is
    # rounding noise on both sides: each tensor is compared on its own scale, floored at 1e-3 of the largest gradient
    floor = 1e-3 * max(float(t.grad.abs().max()) for t in sd.values() if t.grad is not None)
    for k, p in m.named_parameters():
        ref = sd[k].grad
        if ref is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, "no gradient for " + k
        assert torch.isfinite(p.grad).all(), k
        err = float((p.grad.cpu() - ref).abs().max()) / max(float(ref.abs().max()), floor)
        assert err <= grad_tol, "%s d %s: rel err %.3e > %.1e" % (what, k, err, grad_tol)
        if rms_tol is not None:
            rms = float((p.grad.cpu() - ref).double().norm()) / max(float(ref.double().norm()), floor * ref.numel() ** 0.5)
            assert rms <= rms_tol, "%s d %s: rms rel err %.3e > %.1e" % (what, k, rms, rms_tol)
        n += 1
    assert n > 0


def _leaf(t, cuda=None):
    if t is None:
        return None
    t = t.detach().clone()
    if cuda is not None:
        t = t.to(cuda)
    return t.requires_grad_(True)


@pytest.mark.parametrize("name", sorted(cases.CROSS_WIN))
def test_cross_win_attention_gradients(cuda, name):
    c = cases.CROSS_WIN[name]
    m = _train_module(host.CrossWinAttention(c["dim"], c["heads"], c["dim_head"], c["qkv_bias"]), cuda)
    sd = _oracle_sd(m)
    ins = cases.cross_win_inputs(name)
    with torch.enable_grad():
        ref_in = [_leaf(t) for t in ins]
        out_ref = o_fax.cross_win_attention(sd, "", *ref_in, c["heads"], c["dim_head"])
        dev_in = [_leaf(t, cuda) for t in ins]
        out = m(*dev_in)
        # the train() forward is the same function as the eval() one (and the golden vector)
        assert_close(out, golden("gv2_cross_win_attention")[name], TOL, "train-mode forward vs golden")
        _compare(m, sd, out, out_ref, dev_in, ref_in, "CrossWinAttention." + name)


@pytest.mark.parametrize("name", sorted(cases.CVSA))
def test_cross_view_swap_attention_gradients(cuda, name):
    """gv3: both cross attentions (window x window, window x dilated grid), the padded key / value maps, the camera mean, MLPs and
    norms under autograd.  BatchNorms frozen (.eval(), the fine-tuning recipe) so that the oracle's running-statistics
    BatchNorm is the same function; in full train() mode they take batch statistics like torch's."""
    c = cases.CVSA[name]
    fd, fh, fw = c["feat"]
    m = _train_module(host.CrossViewSwapAttention(fh, fw, fd, c["dim"], c["index"], c["image"][0], c["image"][1], **c["kwargs"]), cuda)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eval()
    bev = host.BEVEmbedding(c["dim"], **c["bev_embedding"]).to(cuda)
    sd = _oracle_sd(m)
    x, feat, I_inv, E = cases.cvsa_inputs(name)
    grid = getattr(bev, "grid%d" % c["index"]).detach().cpu()
    with torch.enable_grad():
        xr, fr = _leaf(x), _leaf(feat)
        out_ref = o_fax.cross_view_swap_attention(sd, "", dict(c["kwargs"], image_height=c["image"][0], image_width=c["image"][1]),
                                                  c["index"], xr, grid, fr, I_inv, E)
        xd, fdv = _leaf(x, cuda), _leaf(feat, cuda)
        out = m(c["index"], xd, bev, fdv, I_inv.to(cuda), E.to(cuda))
        assert_close(out, golden("gv3_cross_view_swap_attention")[name], TOL, "train-mode forward vs golden")
        _compare(m, sd, out, out_ref, [xd, fdv], [xr, fr], "CrossViewSwapAttention." + name)
    # full train() mode: batch statistics, running statistics updated
    m.train()
    before = m.feature_linear[0].running_mean.clone()
    with torch.enable_grad():
        out2 = m(c["index"], x.to(cuda), bev, feat.to(cuda), I_inv.to(cuda), E.to(cuda))
        out2.square().mean().backward()
    assert torch.isfinite(out2).all() and not torch.equal(before, m.feature_linear[0].running_mean)


def test_global_attention_gradients(cuda):
    c = cases.GLOBAL_ATTN
    m = _train_module(host.FaxAttention(c["dim"], c["dim_head"], 0.0, c["window_size"]), cuda)
    sd = _oracle_sd(m)
    x = synth.procedural_input("gv9.x", (c["b"], c["dim"], c["window_size"], c["window_size"]), cases.SEED)
    with torch.enable_grad():
        xr, xd = _leaf(x), _leaf(x, cuda)
        out_ref = o_fax.global_attention(sd, "", xr, c["dim_head"], c["window_size"])
        out = m(xd)
        assert_close(out, golden("gv9_global_attention")["out"], TOL, "train-mode forward vs golden")
        _compare(m, sd, out, out_ref, [xd], [xr], "FAX global attention")


@pytest.mark.parametrize("use_mask", [True, False])
def test_swap_fusion_encoder_gradients(cuda, use_mask):
    c = cases.SWAP
    x, mask = cases.swap_inputs()
    args = dict(input_dim=c["dim"], mlp_dim=c["mlp_dim"], agent_size=c["agent_size"], window_size=c["window_size"],
                dim_head=c["dim_head"], drop_out=0.0, depth=c["depth"], mask=use_mask)
    m = _train_module(host.SwapFusionEncoder(dict(args)), cuda)
    sd = _oracle_sd(m)
    with torch.enable_grad():
        xr, xd = _leaf(x), _leaf(x, cuda)
        out_ref = o_swap.swap_fusion_encoder(sd, "", args, xr, mask if use_mask else None)
        out = m(xd, mask.to(cuda) if use_mask else None)
        assert_close(out, golden("gv5_swap_fusion")["encoder_mask" if use_mask else "encoder_nomask"], TOL,
                     "train-mode forward vs golden")
        _compare(m, sd, out, out_ref, [xd], [xr], "SwapFusionEncoder mask=%s" % use_mask)


def test_swap_block_and_attention_gradients(cuda):
    c = cases.SWAP
    x, mask = cases.swap_inputs()
    w, b, L, d, hw = c["window_size"], c["b"], c["agent_size"], c["dim"], c["hw"]
    blk = _train_module(host.SwapFusionBlockMask(d, c["mlp_dim"], c["dim_head"], w, L, 0.0), cuda)
    sd = _oracle_sd(blk)
    with torch.enable_grad():
        xr, xd = _leaf(x), _leaf(x, cuda)
        names = o_swap.block_names("", 0, True)
        names = {k: v.replace("layers.0.", "") for k, v in names.items()} if isinstance(names, dict) else \
            [n.replace("layers.0.", "") for n in names]
        out_ref = o_swap.swap_fusion_block(sd, names, xr, mask, c["dim_head"], L, w)
        out = blk(xd, mask.to(cuda))
        _compare(blk, sd, out, out_ref, [xd], [xr], "SwapFusionBlockMask")
    att = _train_module(host.SwapAttention(d, c["dim_head"], 0.0, L, w), cuda)
    sd = _oracle_sd(att)
    xw = x.permute(0, 1, 3, 4, 2).reshape(b, L, hw // w, w, hw // w, w, d).permute(0, 1, 2, 4, 3, 5, 6).contiguous()
    mw = mask.reshape(b, hw // w, w, hw // w, w, 1, L).permute(0, 1, 3, 2, 4, 5, 6).contiguous()
    with torch.enable_grad():
        xr, xd = _leaf(xw), _leaf(xw, cuda)
        out_ref = o_swap.swap_attention(sd, "", xr, mw, c["dim_head"], L, w)
        out = att(xd, mask=mw.to(cuda))
        _compare(att, sd, out, out_ref, [xd], [xr], "swap Attention (stored partition, mask)")


def _dense_attention(q, k, v, qrows, krows, bias, mask_keys, heads, scale):
    """torch reference of the gathered attention: rows (B, L, N) index maps, bias (Nq, Nk, heads) | None,
    mask_keys (B, L, Nk) bool | None -> per-window outputs (B, L, Nq, d)"""
    B, L, Nq = qrows.shape
    Nk = krows.shape[2]
    d = q.shape[1]
    qg = q[qrows.reshape(-1)].reshape(B, L, Nq, heads, 32).permute(0, 1, 3, 2, 4)
    kg = k[krows.reshape(-1)].reshape(B, L, Nk, heads, 32).permute(0, 1, 3, 2, 4)
    vg = v[krows.reshape(-1)].reshape(B, L, Nk, heads, 32).permute(0, 1, 3, 2, 4)
    s = scale * qg @ kg.transpose(-1, -2)
    if bias is not None:
        s = s + bias.permute(2, 0, 1)
    if mask_keys is not None:
        s = s.masked_fill(~mask_keys[:, :, None, None, :], -float("inf"))
    o = s.softmax(-1) @ vg
    return o.permute(0, 1, 3, 2, 4).reshape(B, L, Nq, d)


@pytest.mark.parametrize("mode,ncam,H,W,w1,w2,heads,use_bias,use_mask", [
    (0, 3, 12, 20, 6, 5, 2, True, True),      # Nq = Nk = 90: ragged 32-tiles, 3-D bias, key mask
    (1, 2, 8, 8, 4, 4, 4, True, False),       # dilated grid
    (0, 1, 10, 10, 5, 5, 1, False, False),    # Nq = 25 < one tile
    (1, 5, 14, 14, 7, 7, 2, True, True),      # 245 tokens: eight 32-key tiles, two query rounds per wave
])
def test_window_attention_backward_vs_dense_torch(cuda, mode, ncam, H, W, w1, w2, heads, use_bias, use_mask):
    """the kernel pair alone, on shapes the module cases do not reach; the reference is dense torch attention over the index
    maps the forward kernels are tested against bit-exactly (cobevt_attention_index_map)"""
    B, d = 2, heads * 32
    tm = ops.tokmap(mode, ncam, H, W, w1, w2)
    rows_n = B * ncam * H * W
    g = torch.Generator().manual_seed(5)
    q0, k0, v0 = (torch.randn(rows_n, d, generator=g) for _ in range(3))
    table0 = torch.randn((2 * ncam - 1) * (2 * w1 - 1) * (2 * w2 - 1), heads, generator=g) if use_bias else None
    mask = None
    if use_mask:
        mask = (torch.rand(B, H, W, ncam, generator=g) > 0.3).float()
        mask[..., 0] = 1.0                                        # the ego agent is always visible
        mask = mask.to(cuda)
    rows = ops.attention_index_map(tm, B, cuda).long()
    bidx = ops.attention_bias_index(tm, tm, ncam, cuda).long() if use_bias else None
    wgt = torch.randn(rows_n, d, generator=g).to(cuda)
    with torch.enable_grad():
        q, k, v = (_leaf(t, cuda) for t in (q0, k0, v0))
        table = _leaf(table0, cuda)
        out = ag.window_attention(q, k, v, tm, tm, tm, B, heads, 0.37, rows_n, bias_table=table, bias_L=ncam, mask=mask)
        (out * wgt).sum().backward()
        qr, kr, vr = (_leaf(t, cuda) for t in (q0, k0, v0))
        tr = _leaf(table0, cuda)
        mk = None
        if use_mask:
            # mask (B, H, W, ncam) -> per token of the (B * ncam, H, W) matrix -> gathered per window
            tok = mask.permute(0, 3, 1, 2).reshape(-1)
            mk = tok[rows.reshape(-1)].reshape(rows.shape) != 0
        o = _dense_attention(qr, kr, vr, rows, rows, tr[bidx] if use_bias else None, mk, heads, 0.37)
        ref = torch.zeros(rows_n, d, device=cuda).index_copy(0, rows.reshape(-1), o.reshape(-1, d))
        (ref * wgt).sum().backward()
    assert_close(out, ref, 1e-4, "forward")
    assert_close(q.grad, qr.grad, TOL, "dq")
    assert_close(k.grad, kr.grad, TOL, "dk")
    assert_close(v.grad, vr.grad, TOL, "dv")
    if use_bias:
        assert_close(table.grad, tr.grad, TOL, "dbias")


@pytest.mark.parametrize("mode,ncam,H,W,w1,w2,heads,use_bias,use_mask", [
    (0, 3, 12, 20, 6, 5, 2, True, True), (1, 2, 8, 8, 4, 4, 4, True, False), (0, 1, 10, 10, 5, 5, 1, False, False),
    (1, 5, 14, 14, 7, 7, 2, True, True), (0, 4, 16, 16, 8, 8, 4, False, True)])
def test_window_attention_backward_bf16_matrix_path(cuda, mode, ncam, H, W, w1, w2, heads, use_bias, use_mask):
    """inside a bf16 autocast region the backward kernels run their five products on the bf16 matrix path (tiles rounded to bf16 as they
    are staged, the row-contracting products fed through transposing LDS reads): against the fp32-MFMA backward of the same call on bf16
    operands, 1e-2 of each gradient's scale (dO, P and dZ are rounded to bf16, as autocast's own backward rounds them); the forward output
    is the same tensor either way"""
    B, d = 2, heads * 32
    tm = ops.tokmap(mode, ncam, H, W, w1, w2)
    rows_n = B * ncam * H * W
    g = torch.Generator().manual_seed(6)
    q0, k0, v0 = (torch.randn(rows_n, d, generator=g).to(torch.bfloat16).float() for _ in range(3))
    table0 = torch.randn((2 * ncam - 1) * (2 * w1 - 1) * (2 * w2 - 1), heads, generator=g) if use_bias else None
    mask = None
    if use_mask:
        mask = (torch.rand(B, H, W, ncam, generator=g) > 0.3).float()
        mask[..., 0] = 1.0
        mask = mask.to(cuda)
    wgt = torch.randn(rows_n, d, generator=g).to(cuda)
    res = []
    for amp in (False, True, True):
        with torch.enable_grad():
            q, k, v = (_leaf(t, cuda) for t in (q0, k0, v0))
            table = _leaf(table0, cuda)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                out = ag.window_attention(q, k, v, tm, tm, tm, B, heads, 0.37, rows_n, bias_table=table, bias_L=ncam, mask=mask)
            assert out.dtype == torch.float32
            (out * wgt).sum().backward()
        res.append((out.detach(), q.grad, k.grad, v.grad, table.grad if use_bias else None))
    assert torch.equal(res[0][0], res[1][0])
    # dq / dk / dv rows are written by one workgroup each in a fixed order: two runs agree to the bit (the bias-table gradient is atomics)
    for a, b in zip(res[1][1:4], res[2][1:4]):
        assert torch.equal(a, b)
    for a, b, what in zip(res[1][1:], res[0][1:], ("dq", "dk", "dv", "dbias")):
        if a is not None:
            assert_close(a, b, 1e-2, "bf16 matrix path " + what)
            assert float((a - b).abs().max()) > 0, "the bf16 path did not run"


@pytest.mark.parametrize("amp", [False, True])
def test_window_self_attention_on_the_fused_projection(cuda, amp):
    """ag.window_self_attention(qkv) = ag.window_attention on the three column blocks of the fused (rows, 3 d) projection: same kernels reading
    / writing the blocks in place (row stride 3 d), one gradient tensor; bit-identical output, dqkv equal to the concatenated dq | dk | dv
    (exactly in fp32; inside a bf16 autocast region up to the bf16 rounding of the returned gradient)"""
    B, heads, ncam, H, W, w1, w2 = 2, 2, 3, 12, 20, 6, 5
    d = heads * 32
    tm = ops.tokmap(0, ncam, H, W, w1, w2)
    rows_n = B * ncam * H * W
    g = torch.Generator().manual_seed(8)
    qkv0 = torch.randn(rows_n, 3 * d, generator=g).to(torch.bfloat16).float()
    table0 = torch.randn((2 * ncam - 1) * (2 * w1 - 1) * (2 * w2 - 1), heads, generator=g)
    mask = (torch.rand(B, H, W, ncam, generator=g) > 0.3).float()
    mask[..., 0] = 1.0
    mask = mask.to(cuda)
    wgt = torch.randn(rows_n, d, generator=g).to(cuda)
    res = []
    for fused in (False, True):
        with torch.enable_grad():
            qkv = _leaf(qkv0, cuda)
            table = _leaf(table0, cuda)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                src = qkv.to(torch.bfloat16) if amp else qkv            # what a projection hands over inside the region
                if fused:
                    out = ag.window_self_attention(src, tm, B, heads, 0.37, rows_n, bias_table=table, bias_L=ncam, mask=mask)
                else:
                    out = ag.window_attention(src[:, :d], src[:, d:2 * d], src[:, 2 * d:], tm, tm, tm, B, heads, 0.37, rows_n, bias_table=table,
                                              bias_L=ncam, mask=mask)
            (out.float() * wgt).sum().backward()
        res.append((out.detach().float(), qkv.grad.clone(), table.grad.clone()))
    assert torch.equal(res[0][0], res[1][0])
    if amp:
        assert_close(res[1][1], res[0][1], 1e-2, "dqkv")
    else:
        assert torch.equal(res[1][1], res[0][1])
    assert_close(res[1][2], res[0][2], 1e-2 if amp else 1e-5, "dbias")
    if amp:
        # both of the above ran with bf16 q / k / v / out / gradients end to end (WindowAttentionHalfFn: bf16 forward kernel, bf16 storage in the
        # backward); against the fp32-storage Functions on the same bf16 operands
        ag.USE_ATTN_HALF_IO = False
        try:
            with torch.enable_grad():
                qkv = _leaf(qkv0, cuda)
                table = _leaf(table0, cuda)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    out = ag.window_self_attention(qkv.to(torch.bfloat16), tm, B, heads, 0.37, rows_n, bias_table=table, bias_L=ncam, mask=mask)
                assert out.dtype == torch.float32
                (out.float() * wgt).sum().backward()
        finally:
            ag.USE_ATTN_HALF_IO = True
        assert res[1][0].dtype == torch.float32          # (converted above; the Function's own output was bf16)
        assert_close(res[1][0], out.detach(), 1e-2, "bf16-storage forward vs fp32-storage forward")
        assert_close(res[1][1], qkv.grad, 1e-2, "bf16-storage dqkv vs fp32-storage dqkv")
        assert_close(res[1][2], table.grad, 1e-2, "bf16-storage dbias vs fp32-storage dbias")


def test_layernorm_and_gelu_backward(cuda):
    g = torch.Generator().manual_seed(3)
    for rows, C in ((1000, 128), (37, 64), (5000, 256), (16, 512), (20001, 128)):      # >= 16,384 narrow rows: the 16-wave workgroups
        x0 = torch.randn(rows, C, generator=g) * 2 + 0.5
        ln = torch.nn.LayerNorm(C).to(cuda)
        with torch.no_grad():
            ln.weight.copy_(torch.randn(C, generator=g))
            ln.bias.copy_(torch.randn(C, generator=g))
        w = torch.randn(rows, C, generator=g).to(cuda)
        with torch.enable_grad():
            x = _leaf(x0, cuda)
            (ag.layernorm(x, ln) * w).sum().backward()
            got = (x.grad.clone(), ln.weight.grad.clone(), ln.bias.grad.clone())
            ln.zero_grad()
            xr = _leaf(x0, cuda)
            (ln(xr) * w).sum().backward()
        for a, b, what in zip(got, (xr.grad, ln.weight.grad, ln.bias.grad), ("dx", "dgamma", "dbeta")):
            assert_close(a, b, 1e-4, "LayerNorm %s (%d x %d)" % (what, rows, C))
        with torch.enable_grad():
            x = _leaf(x0, cuda)
            y = ag.gelu(x)
            (y * w).sum().backward()
            xr = _leaf(x0, cuda)
            yr = torch.nn.functional.gelu(xr)
            (yr * w).sum().backward()
        assert_close(y, yr, 1e-5, "GELU")
        assert_close(x.grad, xr.grad, 1e-5, "GELU backward")


def test_layernorm_and_gelu_inside_bf16_autocast(cuda):
    """inside a bf16 autocast region: LayerNorm -> projection writes the projection's bf16 operand directly (for_projection) and reads the
    bf16 gradient coming back, GELU runs on the projection's bf16 output; both against torch's own autocast graph of the same modules
    (layer_norm in fp32 + cast, gelu in bf16) - forward to one bf16 step on <= 0.1 % of the elements, gradients to bf16 rounding"""
    g = torch.Generator().manual_seed(9)
    for rows, C in ((1000, 128), (40, 256)):
        x0 = torch.randn(rows, C, generator=g) * 2 + 0.5
        ln = torch.nn.LayerNorm(C).to(cuda)
        lin = torch.nn.Linear(C, 2 * C).to(cuda)
        with torch.no_grad():
            ln.weight.copy_(torch.randn(C, generator=g))
            ln.bias.copy_(torch.randn(C, generator=g))
        w = torch.randn(rows, 2 * C, generator=g).to(cuda)
        with torch.enable_grad():
            x = _leaf(x0, cuda)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                xn = ag.layernorm(x, ln, for_projection=True)
                assert xn.dtype == torch.bfloat16
                h = ag.gelu(ag.linear(xn, lin))
                assert h.dtype == torch.bfloat16
                keep = ag.layernorm(x, ln)
                assert keep.dtype == torch.float32                  # not for a projection: fp32 like torch's autocast
            (h.float() * w).sum().backward()
            got = (x.grad.clone(), ln.weight.grad.clone(), ln.bias.grad.clone(), lin.weight.grad.clone())
            ln.zero_grad()
            lin.zero_grad()
            xr = _leaf(x0, cuda)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                xnr = ln(xr)
                hr = torch.nn.functional.gelu(torch.nn.functional.linear(xnr, lin.weight, lin.bias))
            (hr.float() * w).sum().backward()
        # = torch's fp32 layer_norm + cast up to fp32 rounding of the statistics: the odd element lands on the neighbouring bf16 value
        assert float((xn != xnr.to(torch.bfloat16)).float().mean()) <= 1e-3, "LayerNorm written as bf16"
        assert_close(xn.float(), xnr, 1e-2, "LayerNorm written as bf16")
        assert_close(keep, xnr, 1e-5, "LayerNorm fp32 result inside the region")
        assert_close(h.float(), hr.float(), 1e-2, "projection + GELU (bf16)")
        for a, b, what in zip(got, (xr.grad, ln.weight.grad, ln.bias.grad, lin.weight.grad), ("dx", "dgamma", "dbeta", "dW")):
            assert a.dtype == torch.float32
            assert_close(a, b, 1e-2, "bf16 autocast LayerNorm/GELU chain %s (%d x %d)" % (what, rows, C))


def test_training_slice_fails_loudly(cuda):
    m = _train_module(host.SwapAttention(64, 32, 0.0, 3, 4), cuda)
    x = torch.zeros(1, 3, 2, 2, 4, 4, 64)
    with pytest.raises(CobevtHipError):
        m(x)                                                       # CPU tensor
    with pytest.raises(CobevtHipError):
        m(x.to(cuda).to(torch.bfloat16))                           # bf16 is the inference layout
    # modules without a training forward keep refusing train() mode (the nuScenes decoder)
    from cobevt_amd.host import nuscenes as nu
    dec = nu.Decoder(128, [128, 64]).train().to(cuda)
    with pytest.raises(CobevtHipError):
        dec(torch.zeros(1, 128, 8, 8, device=cuda))


def test_one_optimizer_step_reduces_the_loss(cuda):
    """train_camera.py:143-179 in miniature: forward, loss, backward, Adam step on the masked swap-fusion encoder"""
    c = cases.SWAP
    x, mask = cases.swap_inputs()
    args = dict(input_dim=c["dim"], mlp_dim=c["mlp_dim"], agent_size=c["agent_size"], window_size=c["window_size"],
                dim_head=c["dim_head"], drop_out=0.1, depth=c["depth"], mask=True)
    m = _train_module(host.SwapFusionEncoder(args), cuda)
    target = synth.procedural_input("train.target", (c["b"], c["dim"], c["hw"], c["hw"]), cases.SEED).to(cuda)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = []
    torch.manual_seed(0)
    with torch.enable_grad():
        for _ in range(8):
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(m(x.to(cuda), mask.to(cuda)), target)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    # eval() after training: the inference plans follow the updated parameters
    m.eval()
    with torch.no_grad(), host.compute_dtype(torch.float32):
        y_eval = m(x.to(cuda), mask.to(cuda))
    m.train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    with torch.no_grad():
        y_train = m(x.to(cuda), mask.to(cuda))
    assert_close(y_eval, y_train, TOL, "eval() forward after optimizer steps vs train-mode graph")


@pytest.mark.parametrize("cin,cout,k,stride,pad,h,w,bias", [
    (64, 64, 3, 1, 1, 12, 20, False), (64, 128, 3, 2, 1, 16, 16, False), (64, 128, 1, 2, 0, 16, 16, False), (3, 64, 7, 2, 3, 32, 32, False),
    (32, 2, 3, 1, 1, 9, 11, True), (128, 32, 1, 1, 0, 8, 8, True), (16, 24, 3, 2, 1, 15, 13, True)])
def test_conv2d_forward_backward_vs_torch(cuda, cin, cout, k, stride, pad, h, w, bias):
    """the training conv (fp32 implicit-GEMM forward and input gradient, library-GEMM weight gradient) against torch's conv2d
    autograd: the ResNet / decoder / head shapes incl. strided, odd sizes, 3 input and 2 output channels"""
    g = torch.Generator().manual_seed(7)
    conv = torch.nn.Conv2d(cin, cout, k, stride, pad, bias=bias).to(cuda)
    x0 = torch.randn(2, cin, h, w, generator=g)
    with torch.enable_grad():
        x = _leaf(x0, cuda)
        y = ag.conv2d(x, conv)
        wgt = torch.randn(y.shape, generator=g).to(cuda)
        (y * wgt).sum().backward()
        got = (y.detach().clone(), x.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone() if bias else None)
        conv.zero_grad()
        xr = _leaf(x0, cuda)
        yr = conv(xr)
        (yr * wgt).sum().backward()
    assert_close(got[0], yr, 1e-4, "conv forward")
    assert_close(got[1], xr.grad, 1e-4, "conv dX")
    assert_close(got[2], conv.weight.grad, 1e-4, "conv dW")
    if bias:
        assert_close(got[3], conv.bias.grad, 1e-4, "conv db")


@pytest.mark.parametrize("cin,cout,k,stride,pad,h,w,bias", [
    (64, 64, 3, 1, 1, 12, 20, False), (64, 128, 3, 2, 1, 16, 16, False), (64, 128, 1, 2, 0, 16, 16, False), (3, 64, 7, 2, 3, 32, 32, False),
    (32, 2, 3, 1, 1, 9, 11, True), (128, 32, 1, 1, 0, 8, 8, True), (24, 40, 3, 2, 1, 15, 13, True),
    # 3x3 / pad 1 with 64 | Cin: forward (and, stride 1 with 64 | Cout, the input gradient) on the inference strip kernels - a biased
    # 128 -> 64, the 32-cout four-wave tiles, 256 / 512 channels, a stride-2 whose input gradient stays on the implicit GEMM, a
    # 64 -> 72 whose input gradient does (Cout off 64), and a map large enough for the LDS-staged kernel (variant 0) both ways
    (128, 64, 3, 1, 1, 20, 36, True), (64, 32, 3, 1, 1, 16, 48, False), (256, 256, 3, 1, 1, 8, 8, False), (512, 512, 3, 1, 1, 6, 10, False),
    (128, 256, 3, 2, 1, 18, 30, True), (64, 72, 3, 1, 1, 10, 16, False), (64, 64, 3, 1, 1, 256, 256, False),
    # 16 | W with 32 | channel counts: the weight gradient straight from the channels-last maps (csrc/wgrad3.hip) - 16- and 32-pixel
    # segments, several segments per row, odd heights, fewer rows than waves
    (128, 128, 3, 1, 1, 32, 32, False), (256, 64, 3, 1, 1, 16, 16, True), (64, 128, 3, 1, 1, 9, 64, False), (32, 32, 3, 1, 1, 5, 16, False),
    (32, 96, 3, 1, 1, 1, 48, False), (512, 512, 3, 1, 1, 16, 16, False)])
def test_conv2d_bf16_autocast_forward_backward_vs_torch(cuda, cin, cout, k, stride, pad, h, w, bias):
    """inside a bf16 autocast region the training conv runs on the bf16 implicit-GEMM kernel in forward and input gradient (the
    gather path for channel counts off the 16-byte chunk, incl. the 2-channel head whose input gradient has 2 'input' channels) and
    accumulates the weight gradient in fp32 from bf16 operands; fp32 master weights receive fp32 gradients.  Against torch's fp32
    conv2d autograd on the bf16-rounded operands, 1e-2 of each tensor's scale (BASELINE.md section 2's bf16 gate)"""
    g = torch.Generator().manual_seed(11)
    conv = torch.nn.Conv2d(cin, cout, k, stride, pad, bias=bias).to(cuda)
    x0 = torch.randn(2, cin, h, w, generator=g)
    with torch.enable_grad():
        x = _leaf(x0, cuda)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = ag.conv2d(x, conv)
        assert y.dtype == torch.bfloat16
        wgt = torch.randn(y.shape, generator=g).to(cuda)
        (y.float() * wgt).sum().backward()
        assert x.grad.dtype == torch.float32 and conv.weight.grad.dtype == torch.float32
        got = (y.detach().float(), x.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone() if bias else None)
        conv.zero_grad()
        rnd = lambda t: t.to(torch.bfloat16).float()      # noqa: E731
        xr = _leaf(rnd(x0), cuda)
        yr = torch.nn.functional.conv2d(xr, rnd(conv.weight), conv.bias, stride, pad)
        (yr * wgt).sum().backward(inputs=[xr, conv.weight] + ([conv.bias] if bias else []))
    assert_close(got[0], yr, 1e-2, "bf16 conv forward")
    assert_close(got[1], xr.grad, 1e-2, "bf16 conv dX")
    assert_close(got[2], conv.weight.grad, 1e-2, "bf16 conv dW")
    if bias:
        assert_close(got[3], conv.bias.grad, 1e-2, "bf16 conv db")


def _freeze_bn(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eval()
    return m


def test_corpbevt_trains_end_to_end_gradients_vs_oracle(cuda):
    """The whole reduced CorpBEVT (gv8 config: ResNet encoder, FAX pyramid, STTF, swap fusion, decoder, head) in train() mode
    against torch autograd through the oracle: logits and the gradient of every parameter (BatchNorms frozen so that the
    oracle's running-statistics BatchNorm is the same function)."""
    import copy
    import oracle.corpbevt as o_model
    cfg = synth.corpbevt_small_config()
    cfg["fax"]["self_attn"]["dropout"] = 0.0          # dropout off everywhere: the oracle is the eval-mode function
    cfg["fax_fusion"]["drop_out"] = 0.0
    m = _freeze_bn(_train_module(host.CorpBEVT(copy.deepcopy(cfg)), cuda))
    sd = _oracle_sd(m)
    batch = synth.opv2v_batch(agents=2, cams=2, image=128, max_cav=3, seed=cases.SEED)
    with torch.enable_grad():
        out_ref = o_model.corpbevt_forward(sd, cfg, dict(batch))["dynamic_seg"]
        out = m({k: v.to(cuda) for k, v in batch.items()})["dynamic_seg"]
        assert_close(out, golden("gv8_corpbevt_small")["dynamic_seg"], TOL, "train-mode forward vs golden")
        # The whole model is a deep ReLU network: its activations agree with the CPU oracle's to ~1e-6, which is enough to put a
        # handful of the ~3 M pre-activations on the other side of zero, and one flipped ReLU moves one row of one weight gradient by up
        # to ~1 % of that tensor's largest entry (tools/train_grad_diag.py, tools/bn_flip_probe.py: the mismatching elements are one
        # channel of one layer, forward outputs identical to 3e-6, and WHICH layers are hit changes with any 1e-7 perturbation - it
        # moved when the stem BatchNorm went from torch's formula to x * scale + shift, whose outputs are equally close to fp64).
        # So: logits to 1e-3; per-tensor gradients to 5e-3 in the rms norm and 2e-2 in the max norm.  The module-level gradient
        # tests above (no ReLU between the parameter and the loss, or few) keep the 1e-3 max-norm gate.
        _compare(m, sd, out, out_ref, [], [], "CorpBEVT (reduced)", grad_tol=2e-2, rms_tol=5e-3)


def test_corpbevt_optimizer_steps(cuda):
    """train_camera.py:143-179 in miniature on the whole model: full train() mode (BatchNorm batch statistics), cross-entropy on the
    dynamic head, Adam; the loss goes down and the bf16 inference path follows the updated parameters"""
    import copy
    cfg = synth.corpbevt_small_config()
    m = _train_module(host.CorpBEVT(copy.deepcopy(cfg)), cuda)
    batch = {k: v.to(cuda) for k, v in synth.opv2v_batch(agents=2, cams=2, image=128, max_cav=3, seed=3).items()}
    gt = None
    opt = torch.optim.Adam(m.parameters(), lr=2e-4)
    losses = []
    with torch.enable_grad():
        for _ in range(6):
            opt.zero_grad()
            logits = m(dict(batch))["dynamic_seg"][:, 0]
            if gt is None:
                gt = (synth.procedural_input("train.gt", (logits.shape[0],) + tuple(logits.shape[2:]), cases.SEED) > 0.3).long().to(cuda)
            loss = torch.nn.functional.cross_entropy(logits, gt)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    m.eval()
    with torch.no_grad():
        y = m(dict(batch))["dynamic_seg"]
    assert torch.isfinite(y).all()


def test_corpbevt_mixed_precision_step_with_grad_scaler(cuda):
    """train_camera.py:123-124,157-160,174-177 (`--half`): forward under torch autocast, GradScaler around backward / step.  The HIP
    Functions take their inputs as fp32 inside the region (autograd._amp_fwd), the torch ops in between run in half: the loss and
    every parameter gradient stay close to the fp32 run, the scaler unscales to fp32 gradients, steps, and skips a step whose
    gradients overflow"""
    import copy
    cfg = synth.corpbevt_small_config()
    cfg["fax"]["self_attn"]["dropout"] = 0.0
    cfg["fax_fusion"]["drop_out"] = 0.0
    m = _freeze_bn(_train_module(host.CorpBEVT(copy.deepcopy(cfg)), cuda))
    batch = {k: v.to(cuda) for k, v in synth.opv2v_batch(agents=2, cams=2, image=128, max_cav=3, seed=5).items()}
    gt = None

    def loss_of(amp_dtype):
        nonlocal gt
        with torch.autocast("cuda", dtype=amp_dtype, enabled=amp_dtype is not None):
            logits = m(dict(batch))["dynamic_seg"][:, 0]
            if gt is None:
                gt = (synth.procedural_input("amp.gt", (logits.shape[0],) + tuple(logits.shape[2:]), cases.SEED) > 0.3).long().to(cuda)
            return torch.nn.functional.cross_entropy(logits.float(), gt)

    with torch.enable_grad():
        m.zero_grad()
        ref_loss = loss_of(None)
        ref_loss.backward()
        ref = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        for amp_dtype in (torch.float16, torch.bfloat16):
            m.zero_grad()
            scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
            loss = loss_of(amp_dtype)
            scaler.scale(loss).backward()
            assert abs(float(loss.detach()) - float(ref_loss.detach())) < 2e-2 * abs(float(ref_loss.detach())), (float(loss.detach()), float(ref_loss.detach()))
            opt = torch.optim.SGD(m.parameters(), lr=0.0)
            scaler.unscale_(opt)
            worst = 0.0
            for n, p in m.named_parameters():
                if n in ref:
                    assert p.grad is not None and p.grad.dtype == torch.float32, n
                    scale = float(ref[n].abs().max())
                    if scale > 1e-3 * max(float(r.abs().max()) for r in ref.values()):
                        worst = max(worst, float((p.grad - ref[n]).abs().max()) / scale)
            # worst parameter, max-norm relative: the half-precision projections in between carry 11 (fp16) / 8 (bf16) mantissa bits
            assert worst < (8e-2 if amp_dtype == torch.float16 else 3e-1), "%s autocast gradients differ from the fp32 run: %.3g" % (amp_dtype, worst)
        # an overflowing gradient: the step is skipped and the scale backs off
        before = [p.detach().clone() for p in m.parameters()]
        opt = torch.optim.SGD(m.parameters(), lr=1.0)
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
        m.zero_grad()
        scaler.scale(loss_of(torch.float16)).backward()
        next(iter(m.parameters())).grad.view(-1)[0] = float("inf")
        scaler.step(opt)
        scaler.update()
        assert scaler.get_scale() == 512.0
        assert all(torch.equal(a, b) for a, b in zip(before, m.parameters()))


def test_attention_dropout_device_seed_word(cuda):
    """the dropout mask of the attention probabilities = hash(host seed + the device word autograd.dropout_step): bumping the word
    changes the mask while the host seed (what a captured HIP graph would freeze) stays the same; forward and backward agree on it"""
    B, heads, hw, d = 1, 2, 8, 64
    tm = ops.tokmap(0, 1, hw, hw, hw, hw)
    n = hw * hw
    g = torch.Generator().manual_seed(3)
    q0, k0, v0 = (torch.randn(B * n, d, generator=g) for _ in range(3))

    def run():
        torch.manual_seed(1234)                        # the same host seed every time
        with torch.enable_grad():
            q, k, v = _leaf(q0, cuda), _leaf(k0, cuda), _leaf(v0, cuda)
            o = ag.window_attention(q, k, v, tm, tm, tm, B, heads, 0.2, B * n, drop_p=0.4)
            o.sum().backward()
        return o.detach().clone(), v.grad.clone()
    word = ag.dropout_step(cuda)
    start = int(word.item())
    o1, g1 = run()
    o2, g2 = run()
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    word.add_(1)
    o3, g3 = run()
    assert not torch.equal(o1, o3)
    # forward and backward regenerate the same mask: with v = 1 and dout = 1, sum(out) and sum(dv) are both 32 x the sum of the
    # kept, rescaled probabilities of every head
    with torch.enable_grad():
        torch.manual_seed(1234)
        q, k, v = _leaf(q0, cuda), _leaf(k0, cuda), _leaf(torch.ones_like(v0), cuda)
        o = ag.window_attention(q, k, v, tm, tm, tm, B, heads, 0.2, B * n, drop_p=0.4)
        o.sum().backward()
    assert abs(float(o.detach().sum()) - float(v.grad.sum())) < 1e-4 * abs(float(o.detach().sum()))
    assert abs(float(o.detach().sum()) / (B * n * d) - 1.0) < 0.1           # E[kept / (1 - p)] = 1
    word.fill_(start)
    o4, _ = run()
    assert torch.equal(o1, o4)


def test_attention_probability_dropout(cuda):
    """nn.Dropout on the attention probabilities (FAX global attention in train mode, fax_modules.py:114,161) inside the kernels: the
    keep mask is a counter-based hash, dumped by the test hook; forward and all gradients must equal dense torch attention with
    that same mask; the mask has the right density and changes with the seed"""
    B, heads, hw, d = 2, 2, 8, 64
    tm = ops.tokmap(0, 1, hw, hw, hw, hw)
    n = hw * hw
    g = torch.Generator().manual_seed(9)
    q0, k0, v0 = (torch.randn(B * n, d, generator=g) for _ in range(3))
    table0 = torch.randn((2 * hw - 1) ** 2, heads, generator=g)
    wgt = torch.randn(B * n, d, generator=g).to(cuda)
    p_drop, seed = 0.3, 12345
    keep = ag.attention_dropout_mask(B, 1, heads, n, n, p_drop, seed, cuda)               # (B, 1, heads, n, n)
    frac = float(keep.float().mean())
    assert abs(frac - (1 - p_drop)) < 0.01, frac
    assert not torch.equal(keep, ag.attention_dropout_mask(B, 1, heads, n, n, p_drop, seed + 1, cuda))
    rows = ops.attention_index_map(tm, B, cuda).long()
    bidx = ops.attention_bias_index(tm, tm, 1, cuda).long()
    with torch.enable_grad():
        q, k, v, table = (_leaf(t, cuda) for t in (q0, k0, v0, table0))
        out = ag.window_attention(q, k, v, tm, tm, tm, B, heads, 0.21, B * n, bias_table=table, bias_L=1, drop_p=p_drop,
                                  drop_seed=seed)
        (out * wgt).sum().backward()
        qr, kr, vr, tr = (_leaf(t, cuda) for t in (q0, k0, v0, table0))
        qg = qr[rows.reshape(-1)].reshape(B, 1, n, heads, 32).permute(0, 1, 3, 2, 4)
        kg = kr[rows.reshape(-1)].reshape(B, 1, n, heads, 32).permute(0, 1, 3, 2, 4)
        vg = vr[rows.reshape(-1)].reshape(B, 1, n, heads, 32).permute(0, 1, 3, 2, 4)
        s = 0.21 * qg @ kg.transpose(-1, -2) + tr[bidx].permute(2, 0, 1)
        pm = s.softmax(-1) * keep.float() / (1 - p_drop)
        o = (pm @ vg).permute(0, 1, 3, 2, 4).reshape(B, 1, n, d)
        ref = torch.zeros(B * n, d, device=cuda).index_copy(0, rows.reshape(-1), o.reshape(-1, d))
        (ref * wgt).sum().backward()
    assert_close(out, ref, 1e-4, "dropout forward")
    for a, b_, what in ((q.grad, qr.grad, "dq"), (k.grad, kr.grad, "dk"), (v.grad, vr.grad, "dv"), (table.grad, tr.grad, "dbias")):
        assert_close(a, b_, TOL, "dropout " + what)
    # p = 0 in eval-like use and the module route: train() with the shipped dropout runs and differs between calls
    m = _train_module(host.FaxAttention(64, 32, 0.1, 8), cuda)
    x = torch.randn(2, 64, 8, 8, generator=g).to(cuda)
    with torch.no_grad():
        y1, y2 = m(x), m(x)
    assert torch.isfinite(y1).all() and not torch.equal(y1, y2)


def test_vanilla_seg_loss_backward(cuda):
    """VanillaSegLoss (vanilla_seg_loss.py:7-76) with predictions that require grad: value and d loss / d logits against torch's
    nn.CrossEntropyLoss(weight), both heads, ignore label -100 included"""
    g = torch.Generator().manual_seed(2)
    crit = host.VanillaSegLoss({"d_weights": 75.0, "s_weights": 15.0, "l_weights": 50, "d_coe": 2.0, "s_coe": 0.5, "target": "both"})
    dyn0, sta0 = torch.randn(2, 1, 2, 24, 20, generator=g), torch.randn(2, 1, 3, 24, 20, generator=g)
    gd, gs = torch.randint(0, 2, (2, 1, 24, 20), generator=g), torch.randint(0, 3, (2, 1, 24, 20), generator=g)
    gd[0, 0, :3] = -100
    with torch.enable_grad():
        dyn, sta = _leaf(dyn0, cuda), _leaf(sta0, cuda)
        loss = crit({"dynamic_seg": dyn, "static_seg": sta}, {"gt_dynamic": gd.to(cuda), "gt_static": gs.to(cuda)})
        loss.backward()
        dr, sr = _leaf(dyn0, cuda), _leaf(sta0, cuda)
        ce = torch.nn.functional.cross_entropy
        ref = 2.0 * ce(dr.flatten(0, 1), gd.flatten(0, 1).to(cuda), torch.tensor([1.0, 75.0], device=cuda)) + \
            0.5 * ce(sr.flatten(0, 1), gs.flatten(0, 1).to(cuda), torch.tensor([1.0, 15.0, 50.0], device=cuda))
        ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-5 * abs(float(ref.detach()))
    assert_close(dyn.grad, dr.grad, 1e-4, "d loss / d dynamic logits")
    assert_close(sta.grad, sr.grad, 1e-4, "d loss / d static logits")
    # the common AMP pattern: forward inside the autocast region, criterion OUTSIDE it - the head then hands over bf16 logits and no
    # ambient autocast state casts them (this used to raise "the training slice is fp32")
    with torch.enable_grad():
        d16, s16 = _leaf(dyn0.to(torch.bfloat16), cuda), _leaf(sta0.to(torch.bfloat16), cuda)
        loss16 = crit({"dynamic_seg": d16, "static_seg": s16}, {"gt_dynamic": gd.to(cuda), "gt_static": gs.to(cuda)})
        loss16.backward()
    assert d16.grad is not None and d16.grad.dtype == torch.bfloat16 and torch.isfinite(d16.grad.float()).all()
    assert abs(float(loss16.detach()) - float(ref.detach())) <= 2e-2 * abs(float(ref.detach()))


def _dp_worker(rank, world, port, ret):
    import os
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1",
                       "MASTER_PORT": str(port)})
    import torch.distributed as dist
    from cobevt_amd import dist as cdist
    dist.init_process_group("gloo", rank=rank, world_size=world)          # gloo moves CUDA tensors through the host: one GPU is enough
    dev = torch.device("cuda:0")
    c = cases.SWAP
    args = dict(input_dim=c["dim"], mlp_dim=c["mlp_dim"], agent_size=c["agent_size"], window_size=c["window_size"],
                dim_head=c["dim_head"], drop_out=0.0, depth=c["depth"], mask=True)
    m = fill_module_(host.SwapFusionEncoder(args), cases.SEED).train().to(dev)          # identical initial weights on every rank
    red = cdist.GradAllReducer(m.parameters(), bucket_bytes=64 << 10)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    x, mask = cases.swap_inputs()
    x = (x + 0.1 * rank).to(dev)                                                       # a different batch per rank
    target = synth.procedural_input("dp.target.%d" % rank, (c["b"], c["dim"], c["hw"], c["hw"]), cases.SEED).to(dev)
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.mse_loss(m(x, mask.to(dev)), target)
        loss.backward()
        red.finish()
        opt.step()
        losses.append(float(loss.detach()))
    flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    both = [torch.empty_like(flat) for _ in range(world)]
    dist.all_gather(both, flat)
    ret[rank] = (float((both[0] - both[1]).abs().max()), losses, len(red.buckets))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_training_two_ranks_one_gpu(cuda):
    """train_camera.py:105-110 (DistributedDataParallel) with the package's pieces: two processes (gloo, sharing the one GPU),
    identical initial weights, different batches, GradAllReducer between backward and the optimizer step: the replicas'
    parameters stay bit-identical and the losses go down"""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ret = mp.Manager().dict()
    mp.spawn(_dp_worker, args=(2, port, ret), nprocs=2, join=True)
    assert sorted(ret.keys()) == [0, 1]
    for r in (0, 1):
        diff, losses, nb = ret[r]
        assert diff == 0.0, "replicas diverged by %g" % diff
        assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
        assert nb > 1


# ----------------------------------------------------------------------------------------------
# training glue kernels (csrc/train_glue.hip) against torch's own differentiable ops
# ----------------------------------------------------------------------------------------------
def _grads(fn, leaves, wgt=None):
    with torch.enable_grad():
        y = fn()
        w = wgt if wgt is not None else torch.randn(y.shape, generator=torch.Generator().manual_seed(3)).to(y.device)
        (y.float() * w).sum().backward()
    return y.detach().clone(), [None if (t is None or t.grad is None) else t.grad.detach().clone() for t in leaves], w


@pytest.mark.parametrize("c,h,w,training,relu,res", [(64, 12, 20, True, True, True), (64, 12, 20, False, True, True),
                                                     (128, 9, 7, True, False, False), (32, 16, 16, True, True, False),
                                                     (512, 4, 4, False, False, True), (8, 5, 3, True, True, True)])
def test_batch_norm_act_vs_torch(cuda, c, h, w, training, relu, res):
    """relu(bn(x) + residual) with batch statistics (+ running-stat update) and with frozen statistics: forward, dx, d residual,
    dgamma, dbeta and the updated running statistics against F.batch_norm + add + relu (what BasicBlock / Bottleneck / NaiveDecoder
    run under train_camera.py:143-179)"""
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(3, c, h, w, generator=g) * 2.0 + 0.7
    r0 = torch.randn(3, c, h, w, generator=g) if res else None
    bns = []
    for _ in range(2):
        bn = torch.nn.BatchNorm2d(c, eps=1e-3, momentum=0.07).to(cuda)
        with torch.no_grad():
            bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(c, generator=g) * 0.3)
            bn.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
            bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
        bn.train(training)
        bns.append(bn)
    bns[1].load_state_dict(bns[0].state_dict())
    x, r = _leaf(x0, cuda), _leaf(r0, cuda)
    got, gg, wgt = _grads(lambda: ag.batch_norm_act(x, bns[0], residual=r, relu=relu), [x, r, bns[0].weight, bns[0].bias])
    xr, rr = _leaf(x0, cuda), _leaf(r0, cuda)

    def ref_fn():
        y = bns[1](xr)
        if rr is not None:
            y = y + rr
        return torch.relu(y) if relu else y
    ref, rg, _ = _grads(ref_fn, [xr, rr, bns[1].weight, bns[1].bias], wgt)
    assert_close(got, ref, 1e-5, "bn forward")
    for name, a, b in zip(("dx", "dres", "dgamma", "dbeta"), gg, rg):
        if b is not None:
            assert_close(a, b, 1e-4, "bn " + name)
    assert_close(bns[0].running_mean, bns[1].running_mean, 1e-5, "running_mean")
    assert_close(bns[0].running_var, bns[1].running_var, 1e-5, "running_var")
    assert int(bns[0].num_batches_tracked) == int(bns[1].num_batches_tracked)


def test_pool_shuffle_upsample_linear_vs_torch(cuda):
    """MaxPool2d(3, 2, 1) (with ties), PixelUnshuffle(2), nearest x2 up-sampling and nn.Linear through the implicit-GEMM kernels:
    forward and every gradient against torch's ops"""
    F = torch.nn.functional
    g = torch.Generator().manual_seed(5)
    x0 = torch.randint(-3, 4, (2, 16, 13, 10), generator=g).float()                  # integer values: ties inside the windows
    x = _leaf(x0, cuda)
    xr = _leaf(x0, cuda)
    got, gg, wgt = _grads(lambda: ag.max_pool3x3s2(x), [x])
    ref, rg, _ = _grads(lambda: F.max_pool2d(xr, 3, 2, 1), [xr], wgt)
    assert torch.equal(got, ref), "max-pool forward"
    # same arg-max (first maximum of a window wins); overlapping windows add into one pixel in a different order (atomics)
    assert torch.equal(gg[0] != 0, rg[0] != 0) and float((gg[0] - rg[0]).abs().max()) <= 1e-5, "max-pool backward"
    x0 = torch.randn(2, 24, 12, 8, generator=g)
    for ours, theirs, what in ((ag.pixel_unshuffle2, lambda t: F.pixel_unshuffle(t, 2), "pixel_unshuffle"),
                               (ag.upsample_nearest2, lambda t: F.interpolate(t, scale_factor=2, mode="nearest"), "upsample")):
        x, xr = _leaf(x0, cuda), _leaf(x0, cuda)
        got, gg, wgt = _grads(lambda: ours(x), [x])
        ref, rg, _ = _grads(lambda: theirs(xr), [xr], wgt)
        assert torch.equal(got, ref), what
        assert_close(gg[0], rg[0], 1e-6, what + " backward")
    for k, n, bias in ((128, 384, False), (128, 256, True), (64, 8, True)):
        lin = torch.nn.Linear(k, n, bias=bias).to(cuda)
        x0 = torch.randn(3, 37, k, generator=g)
        x = _leaf(x0, cuda)
        got, gg, wgt = _grads(lambda: ag.linear(x, lin), [x, lin.weight] + ([lin.bias] if bias else []))
        lin.zero_grad()
        xr = _leaf(x0, cuda)
        ref, rg, _ = _grads(lambda: F.linear(xr, lin.weight, lin.bias), [xr, lin.weight] + ([lin.bias] if bias else []), wgt)
        assert_close(got, ref, 1e-4, "linear forward")
        for name, a, b in zip(("dx", "dW", "db"), gg, rg):
            assert_close(a, b, 1e-4, "linear " + name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n,h,w,c", [(2, 9, 15, 16), (1, 1, 1, 8), (3, 16, 12, 64), (1, 7, 2, 24)])
def test_maxpool_backward_block_kernel_matches_pixel_kernel(cuda, dtype, n, h, w, c):
    """cobevt_maxpool3x3s2_bwd_t (a thread per 2 x 2 input block, dx in the map's type) against cobevt_maxpool3x3s2_bwd (a thread per pixel,
    fp32 dx): the same first-maximum rule with ties, odd sizes, one-pixel maps; bit-identical after the cast"""
    g = torch.Generator().manual_seed(h * 31 + w)
    x = torch.randint(-2, 3, (n, h, w, c), generator=g).float().to(dtype).to(cuda)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dy = torch.randn(n, ho, wo, c, generator=g).to(dtype).to(cuda)
    lib = ag._L.load()
    old = torch.empty((n, h, w, c), device=cuda, dtype=torch.float32)
    new = torch.full((n, h, w, c), float("nan"), device=cuda, dtype=dtype)
    code = ops.dcode(dtype)
    ag._L.check(lib.cobevt_maxpool3x3s2_bwd(ag._p(x), ag._p(dy), ag._p(old), code, n, h, w, c, ag._stream()), "cobevt_maxpool3x3s2_bwd")
    ag._L.check(lib.cobevt_maxpool3x3s2_bwd_t(ag._p(x), ag._p(dy), ag._p(new), code, n, h, w, c, ag._stream()), "cobevt_maxpool3x3s2_bwd_t")
    assert torch.equal(new, old.to(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_group_mean_vs_torch(cuda, dtype):
    """ag.group_mean (the camera mean of CrossWinAttention) in both directions against torch's mean(dim=1)"""
    g = torch.Generator().manual_seed(4)
    for shape in ((2, 4, 33, 128), (1, 3, 5, 7, 8), (3, 1, 9, 16)):
        x0 = torch.randn(*shape, generator=g).to(dtype)
        w = torch.randn(shape[:1] + shape[2:], generator=g).to(cuda)
        with torch.enable_grad():
            x = x0.to(cuda).requires_grad_(True)
            y = ag.group_mean(x)
            (y.float() * w).sum().backward()
            xr = x0.to(cuda).requires_grad_(True)
            yr = xr.mean(dim=1)
            (yr.float() * w).sum().backward()
        assert y.dtype == dtype and x.grad.dtype == dtype
        assert_close(y.float(), yr.float(), 1e-6 if dtype == torch.float32 else 4e-3, "group mean")
        assert_close(x.grad.float(), xr.grad.float(), 1e-6 if dtype == torch.float32 else 4e-3, "group mean backward")


@pytest.mark.parametrize("amp", [False, True])
@pytest.mark.parametrize("B,n,H,W", [(2, 4, 16, 16), (1, 6, 5, 9), (3, 1, 8, 8)])
def test_fax_bev_query_vs_torch(cuda, amp, B, n, H, W):
    """ag.fax_bev_query (embedding, normalisation, + x, channels-last: one kernel per direction) against the torch graph it replaces
    (fax_modules.py:344-372: 1x1 conv of the grid - camera embedding, / (norm + 1e-7), + x, permute): output and the gradients of x, the
    convolution's weight / bias and the camera embedding; fp32 1e-5, inside a bf16 autocast region 1e-2 (the same roundings are applied)"""
    d = 128
    g = torch.Generator().manual_seed(B * 10 + n)
    conv = torch.nn.Conv2d(2, d, 1).to(cuda)
    x0 = torch.randn(B, d, H, W, generator=g)
    c0 = torch.randn(B * n, d, 1, 1, generator=g)
    grid = (torch.randn(3, H, W, generator=g) * 20).to(cuda)
    wgt = torch.randn(B, n, H, W, d, generator=g).to(cuda)
    res = []
    for fused in (True, False):
        conv.zero_grad()
        with torch.enable_grad():
            x, c = _leaf(x0, cuda), _leaf(c0, cuda)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                ce = c.to(torch.bfloat16) if amp else c                 # the camera embedding is a bf16 projection inside the region
                if fused:
                    q = ag.fax_bev_query(x.permute(0, 2, 3, 1).contiguous(), grid[:2], conv, ce.reshape(B * n, d), n)
                else:
                    e = torch.nn.functional.conv2d(grid[:2][None], conv.weight, conv.bias) - ce
                    e = e / (e.norm(dim=1, keepdim=True) + 1e-7)
                    q = (e.reshape(B, n, d, H, W) + x[:, None]).permute(0, 1, 3, 4, 2).contiguous()
            assert q.shape == (B, n, H, W, d) and q.dtype == torch.float32
            (q * wgt).sum().backward()
        res.append((q.detach(), x.grad.clone(), c.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone()))
    tol = 1e-2 if amp else 1e-5
    for a, b_, what in zip(res[0], res[1], ("query", "dx", "dc", "dW", "dbias")):
        assert_close(a, b_, tol, "fax_bev_query " + what)


@pytest.mark.parametrize("amp", [False, True])
@pytest.mark.parametrize("BN,h,w", [(8, 16, 16), (3, 5, 9)])
def test_fax_img_embed_vs_torch(cuda, amp, BN, h, w):
    """ag.fax_img_embed (the key-side image embedding of CrossViewSwapAttention: 1x1 convolution of the per-camera ray directions - camera
    embedding, normalised, channels-last) against the torch graph it replaces (fax_modules.py:330-343)"""
    d = 128
    g = torch.Generator().manual_seed(BN * 7 + h)
    conv = torch.nn.Conv2d(4, d, 1, bias=False).to(cuda)
    c0 = torch.randn(BN, d, 1, 1, generator=g)
    dd = torch.randn(BN, 4, h, w, generator=g).to(cuda)
    wgt = torch.randn(BN, h, w, d, generator=g).to(cuda)
    res = []
    for fused in (True, False):
        conv.zero_grad()
        with torch.enable_grad():
            c = _leaf(c0, cuda)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                ce = c.to(torch.bfloat16) if amp else c
                if fused:
                    assert ag.fax_img_embed_fusable(dd, conv)
                    q = ag.fax_img_embed(dd, conv, ce.reshape(BN, d))
                else:
                    e = torch.nn.functional.conv2d(dd, conv.weight) - ce
                    q = (e / (e.norm(dim=1, keepdim=True) + 1e-7)).permute(0, 2, 3, 1).contiguous()
            assert q.shape == (BN, h, w, d) and q.dtype == torch.float32
            (q * wgt).sum().backward()
        res.append((q.detach(), c.grad.clone(), conv.weight.grad.clone()))
    tol = 1e-2 if amp else 1e-5
    for a, b_, what in zip(res[0], res[1], ("embedding", "dc", "dW")):
        assert_close(a, b_, tol, "fax_img_embed " + what)


def test_sttf_warp_backward_is_the_adjoint(cuda):
    """<warp(x), g> == <x, warp^T(g)> for the regrouping STTF warp (a linear map of x), and the forward equals the inference kernel:
    cobevt_sttf_warp_bwd scatters through the same sample positions cobevt_sttf_warp gathers from"""
    g = torch.Generator().manual_seed(9)
    batch = synth.opv2v_batch(agents=3, cams=1, image=64, max_cav=4, seed=cases.SEED, batch=2)
    tm = batch["transformation_matrix"].to(cuda).float().contiguous()
    rl = torch.tensor([3, 3], dtype=torch.int32, device=cuda)
    x0 = torch.randn(6, 12, 16, 32, generator=g)
    x = _leaf(x0, cuda)
    with torch.enable_grad():
        y = ag.sttf_warp(x, tm, rl, 4, 0.390625, 8)
        gy = torch.randn(y.shape, generator=g).to(cuda)
        (y * gy).sum().backward()
    ref, _, _ = ops.sttf_warp(x0.to(cuda).contiguous(), tm, None, 0.390625, 8, want_mask=False, record_len=rl, max_cav=4)
    assert torch.equal(y.detach(), ref)
    # adjoint identity with a second, independent x
    x2 = torch.randn(6, 12, 16, 32, generator=g).to(cuda)
    y2, _, _ = ops.sttf_warp(x2.contiguous(), tm, None, 0.390625, 8, want_mask=False, record_len=rl, max_cav=4)
    lhs, rhs = float((y2.double() * gy.double()).sum()), float((x2.double() * x.grad.double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(lhs)), (lhs, rhs)
    assert float(x.grad.abs().max()) > 0


def test_naive_compressor_trains(cuda):
    """NaiveCompressor (naive_compress.py:5-31) in train() mode: forward / gradients against the torch module built from the same
    containers (batch statistics)"""
    comp = _train_module(host.NaiveCompressor(32, 4), cuda)
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(3, 32, 12, 16, generator=g)
    x = _leaf(x0, cuda)
    params = list(comp.parameters())
    got, gg, wgt = _grads(lambda: comp(x), [x] + params)
    state = {k: v.clone() for k, v in comp.state_dict().items()}
    comp.zero_grad()
    ref_mod = torch.nn.Sequential(*comp.encoder, *comp.decoder)          # plain torch forward over the same parameter containers
    fresh = _train_module(host.NaiveCompressor(32, 4), cuda)            # running stats as they were before the first forward
    for (k, v), (_, v0) in zip(comp.state_dict().items(), fresh.state_dict().items()):
        if "running" in k or "num_batches" in k:
            v.copy_(v0)
    xr = _leaf(x0, cuda)
    ref, rg, _ = _grads(lambda: ref_mod(xr), [xr] + params, wgt)
    assert_close(got, ref, 1e-4, "compressor forward")
    # (a conv bias in front of a batch-statistics BatchNorm has an analytically zero gradient: compared on the scale of the largest one)
    floor = 1e-3 * max(float(b.abs().max()) for b in rg)
    for i, (a, b) in enumerate(zip(gg, rg)):
        err = float((a - b).abs().max()) / max(float(b.abs().max()), floor)
        assert err <= 2e-4, "compressor grad %d: %.3e" % (i, err)
    for k, v in comp.state_dict().items():
        if "running" in k:
            assert_close(v, state[k], 1e-5, k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cout,cin,k", [(128, 64, 3), (64, 3, 7), (2, 130, 1), (24, 40, 3), (32, 128, 1)])
def test_conv_weight_rows_kernel_matches_torch_specification(cuda, dtype, cout, cin, k):
    """cobevt_conv_weight_rows (one launch per convolution and step: fp32 master weight -> forward rows AND flipped / transposed
    input-gradient rows in the compute type) is bit-identical to the torch-op construction it replaces (cast, permute, pad, flip,
    transpose, contiguous: autograd._weight_rows), incl. K not a multiple of the k-tile (zero columns) and the 3- / 2-channel ends"""
    g = torch.Generator().manual_seed(cout * 131 + cin)
    w = torch.randn(cout, cin, k, k, generator=g).to(cuda)
    rf, rd = ag.conv_weight_rows(w, dtype, True, True)
    wd = w.to(dtype)
    sf, sd = ag._weight_rows(wd)[0], ag._weight_rows(wd.flip(2, 3).transpose(0, 1))[0]
    assert rf.shape == sf.shape and rd.shape == sd.shape and rf.dtype == dtype
    assert torch.equal(rf, sf) and torch.equal(rd, sd)
    only_f = ag.conv_weight_rows(w, dtype, True, False)
    assert only_f[1] is None and torch.equal(only_f[0], sf)


@pytest.mark.parametrize("cout,cin", [(128, 64), (64, 128), (72, 64), (32, 192), (512, 256)])
def test_conv3_weight_operand_kernel_matches_plan_layouts(cuda, cout, cin):
    """cobevt_conv3_weight_operands (fp32 master weight -> the bf16 fragment table / LDS-staged rows the inference 3x3 kernels read, for the
    forward convolution and for its input gradient = flipped taps, swapped channel roles) is bit-identical to ops.ConvPlan's tables"""
    from cobevt_amd import ops
    g = torch.Generator().manual_seed(cout * 7 + cin)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    wd = w.to(cuda)
    plan = ops.ConvPlan(w, None, stride=1, pad=1, act=0, dtype=torch.bfloat16, device=cuda)
    assert torch.equal(ag.conv3_weight_operand(wd, 150, False).reshape(-1), plan.wfrag.reshape(-1))
    assert torch.equal(ag.conv3_weight_operand(wd, 0, False).reshape(-1), plan.wgt3.reshape(-1))
    if cout % 64 == 0:
        pland = ops.ConvPlan(w.flip(2, 3).transpose(0, 1).contiguous(), None, stride=1, pad=1, act=0, dtype=torch.bfloat16, device=cuda)
        assert torch.equal(ag.conv3_weight_operand(wd, 143, True).reshape(-1), pland.wfrag.reshape(-1))
        assert torch.equal(ag.conv3_weight_operand(wd, 0, True).reshape(-1), pland.wgt3.reshape(-1))
        # both directions from one launch, every combination of the two layouts
        for vf, vd in ((150, 143), (0, 0), (131, 0), (0, 152)):
            f, d = ag.conv3_weight_operand_pair(wd, vf, vd)
            assert torch.equal(f.reshape(-1), (plan.wfrag if vf else plan.wgt3).reshape(-1))
            assert torch.equal(d.reshape(-1), (pland.wfrag if vd else pland.wgt3).reshape(-1))
    f, d = ag.conv3_weight_operand_pair(wd, 150, -1)
    assert d is None and torch.equal(f.reshape(-1), plan.wfrag.reshape(-1))


@pytest.mark.parametrize("n,h,w,cin,cout", [(3, 7, 32, 64, 32), (1, 4, 16, 32, 64), (2, 33, 128, 64, 64), (20, 16, 16, 128, 96)])
def test_conv_wgrad3_matches_blocked_weight_gradient(cuda, n, h, w, cin, cout):
    """cobevt_conv_wgrad3 (operands transposed by the LDS read, partial tiles summed by a second launch: deterministic) against fp64 torch on
    the same bf16 operands at fp32 rounding level, and bit-identical between two runs"""
    g = torch.Generator().manual_seed(n * 1000 + w)
    x = torch.randn(n, h, w, cin, generator=g).to(torch.bfloat16).to(cuda)
    dy = torch.randn(n, h, w, cout, generator=g).to(torch.bfloat16).to(cuda)
    lib = ag._L.load()
    chunks = lib.cobevt_conv_wgrad3_chunks(ag._ints([n, h, w, cin, cout]))
    assert chunks >= 1
    outs = []
    for _ in range(2):
        dw = torch.full((cout, cin, 3, 3), float("nan"), device=cuda)
        scratch = torch.empty((chunks, cout * cin * 9), device=cuda)
        ag._L.check(lib.cobevt_conv_wgrad3(ag._p(x), ag._p(dy), ag._p(dw), ag._p(scratch), ag._ints([n, h, w, cin, cout, chunks]), ag._stream()),
                    "cobevt_conv_wgrad3")
        outs.append(dw)
    assert torch.equal(outs[0], outs[1])
    ref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (cout, cin, 3, 3), dy.double().permute(0, 3, 1, 2), padding=1)
    assert_close(outs[0], ref.float(), 2e-5, "wgrad3 vs fp64 torch")
    # shapes it does not serve are refused, not mangled
    assert lib.cobevt_conv_wgrad3_chunks(ag._ints([n, h, w + 8, cin, cout])) < 0
    assert lib.cobevt_conv_wgrad3_chunks(ag._ints([n, h, w, cin + 8, cout])) < 0


@pytest.mark.parametrize("rows,cin,cout", [(5120, 128, 128), (1000, 128, 384), (81920, 128, 256), (777, 512, 128), (64, 256, 256), (3, 128, 128)])
def test_linear_wgrad_matches_fp64(cuda, rows, cin, cout):
    """cobevt_linear_wgrad (dy^T x over bf16 rows with the operands transposed by the LDS read; row counts off the 64-row step, fewer
    rows than one step, several output tiles) against fp64 torch, bit-identical between two runs, and through autograd.linear"""
    g = torch.Generator().manual_seed(rows + cin)
    x = torch.randn(rows, cin, generator=g).to(torch.bfloat16).to(cuda)
    dy = torch.randn(rows, cout, generator=g).to(torch.bfloat16).to(cuda)
    lib = ag._L.load()
    import ctypes
    chunks = lib.cobevt_linear_wgrad_chunks((ctypes.c_long * 3)(rows, cin, cout))
    assert chunks >= 1
    outs = []
    for _ in range(2):
        dw = torch.full((cout, cin), float("nan"), device=cuda)
        scratch = torch.empty((chunks, cout * cin), device=cuda)
        ag._L.check(lib.cobevt_linear_wgrad(ag._p(x), ag._p(dy), ag._p(dw), ag._p(scratch), (ctypes.c_long * 4)(rows, cin, cout, chunks),
                                            ag._stream()), "cobevt_linear_wgrad")
        outs.append(dw)
    assert torch.equal(outs[0], outs[1])
    ref = dy.double().t() @ x.double()
    assert_close(outs[0], ref.float(), 2e-5, "linear wgrad vs fp64 torch")
    assert lib.cobevt_linear_wgrad_chunks((ctypes.c_long * 3)(rows, cin + 64, cout)) < 0
    # the autograd path takes it inside a bf16 autocast region
    lin = torch.nn.Linear(cin, cout).to(cuda)
    xin = x.float().requires_grad_(True)
    with torch.enable_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = ag.linear(xin, lin)
    y.backward(dy.to(y.dtype))
    assert_close(lin.weight.grad, ref.float(), 1e-2, "autograd.linear dW (bf16 autocast)")


@pytest.mark.parametrize("n,k", [(128, 128), (384, 128), (128, 512), (72, 40), (8, 8)])
def test_linear_weight_frags_kernel_matches_plan_layout(cuda, n, k):
    """cobevt_linear_weight_frags (fp32 master weight -> the bf16 fragment table of the inference row GEMM, for the projection and, transposed,
    for its input gradient) is bit-identical to ops.ConvPlan's wfrag_rows"""
    from cobevt_amd import ops
    g = torch.Generator().manual_seed(n * 3 + k)
    w = torch.randn(n, k, generator=g)
    wd = w.to(cuda)
    plan = ops.ConvPlan(w[:, :, None, None], None, stride=1, pad=0, act=0, dtype=torch.bfloat16, device=cuda)
    f, t = ag.linear_weight_frags(wd, True, True)
    assert torch.equal(f.reshape(-1), plan.wfrag_rows.reshape(-1))
    plant = ops.ConvPlan(w.t().contiguous()[:, :, None, None], None, stride=1, pad=0, act=0, dtype=torch.bfloat16, device=cuda)
    assert torch.equal(t.reshape(-1), plant.wfrag_rows.reshape(-1))
    only = ag.linear_weight_frags(wd, False, True)
    assert only[0] is None and torch.equal(only[1], t)


def test_zero_pool_hands_out_disjoint_zeroed_slices(cuda):
    """autograd._zeros: small gradient buffers are slices of one zero-filled chunk (one fill launch per 16 MiB instead of one per tensor):
    zero, disjoint, handed out once, 256-byte aligned; large ones and captures outside begin/end_capture_zero_pool() keep their own fill"""
    a = ag._zeros((3, 5), cuda, torch.float32)
    b = ag._zeros(7, cuda, torch.float32)
    c = ag._zeros((2, 4), cuda, torch.bfloat16)
    assert a.shape == (3, 5) and b.shape == (7,) and c.dtype == torch.bfloat16
    assert not a.any() and not b.any() and not c.any()
    ptrs = sorted([(t.data_ptr(), t.numel() * t.element_size()) for t in (a, b, c)])
    assert all(p0 + n0 <= p1 for (p0, n0), (p1, _) in zip(ptrs, ptrs[1:])) and all(p % 256 == 0 for p, _ in ptrs)
    assert a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() == c.untyped_storage().data_ptr()
    a.add_(1.0)
    assert not ag._zeros((3, 5), cuda, torch.float32).any()
    big = ag._zeros((1 << 20) + 1, cuda, torch.float32)
    assert big.untyped_storage().data_ptr() != a.untyped_storage().data_ptr() and not big.any()
    ag.USE_ZERO_POOL = False
    try:
        d = ag._zeros(5, cuda, torch.float32)
        assert d.untyped_storage().nbytes() < 4096
    finally:
        ag.USE_ZERO_POOL = True


@pytest.mark.parametrize("k,pad,n,cin,cout,h,w", [(3, 1, 2, 64, 128, 6, 11), (1, 0, 1, 8, 16, 4, 16), (3, 1, 2, 5, 2, 7, 21), (1, 0, 3, 12, 24, 5, 9),
                                                  (3, 1, 1, 128, 32, 32, 32)])
def test_wgrad_block_operand_kernel_matches_torch_specification(cuda, k, pad, n, cin, cout, h, w):
    """cobevt_wgrad_block_operand (pad + 8 x 8 transpose in one launch per operand) is bit-identical to autograd._blocked_operands, the
    torch construction tests/test_weight_layouts.py pins against conv2d autograd: widths off the 8-pixel block, channel counts on
    (16-byte path) and off (per-channel path) the 8-channel group, 3x3 / pad 1 and 1x1 / pad 0"""
    g = torch.Generator().manual_seed(k * 17 + w)
    xl = torch.randn(n, h, w, cin, generator=g).to(torch.bfloat16).to(cuda)
    dyl = torch.randn(n, h + 2 * pad - k + 1, w + 2 * pad - k + 1, cout, generator=g).to(torch.bfloat16).to(cuda)
    got = ag.blocked_operands(xl, dyl, k, pad)
    ref = ag._blocked_operands(xl, dyl, k, pad)
    assert got[2:] == ref[2:]
    # the kernel's layout carries a plane axis ([n][row][block][plane][c][8]); one plane for a stride-1 convolution
    assert got[0].shape[3] == 1 and got[1].shape[3] == 1
    assert torch.equal(got[0].squeeze(3), ref[0]) and torch.equal(got[1].squeeze(3), ref[1])


@pytest.mark.parametrize("k,stride,pad,n,cin,h,w", [(3, 2, 1, 2, 64, 9, 13), (1, 2, 0, 1, 16, 8, 15), (7, 2, 3, 2, 3, 12, 18), (3, 2, 1, 1, 24, 16, 32),
                                                    (3, 2, 1, 2, 128, 64, 64)])
def test_strided_wgrad_block_operand_kernel_matches_specification(cuda, k, stride, pad, n, cin, h, w):
    """cobevt_wgrad_block_operand with planes / a pixel stride (the stride-2 and stem forms of cobevt_conv_wgrad_blocked) is bit-identical to
    autograd._blocked_x_general, which tests/test_weight_layouts.py::test_strided_blocked_weight_gradient_operands pins against conv2d autograd"""
    g = torch.Generator().manual_seed(k * 31 + w)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    xl = torch.randn(n, h, w, cin, generator=g).to(torch.bfloat16).to(cuda)
    dyl = torch.randn(n, ho, wo, 8, generator=g).to(torch.bfloat16).to(cuda)
    mode = ag.wgrad_blocked_mode(k, stride, pad, cin)
    xb, db, hp, nxb, ndb = ag.blocked_operands(xl, dyl, k, pad, stride, mode)
    _, _, _, planes, sx = ag._blocked_geometry(h, w, ho, wo, k, pad, stride, mode)
    assert torch.equal(xb, ag._blocked_x_general(xl, hp, nxb, pad, planes, sx))
    assert torch.equal(db, ag._blocked_x_general(dyl, ho, ndb, 0, 1, 1))


@pytest.mark.parametrize("amp", [False, True])
def test_captured_train_step_follows_eager(cuda, amp):
    """host.CapturedTrainStep (train_camera.py:143-179 - zero_grad, forward, criterion, backward, optimizer.step - as ONE replayed HIP graph)
    against the same steps run eagerly from the same initial state, on two alternating batches: per-step losses, the accumulated parameter
    update, BatchNorm running statistics and num_batches_tracked.  Same kernels on the same data; what differs is the order of the fp32
    atomics in the weight gradients and the occasional ReLU flip that follows from it, so the update is compared in the rms
    norm (2e-2 of the update's rms; measured ~1e-3) and the losses to 5e-3: two EAGER runs from the same state differ by up to 2.3e-3 at
    step 4 of the bf16 run (profiles/r04_train_eager_repro.txt; steps 1-3 agree to the last digit)."""
    import copy
    cfg = synth.corpbevt_small_config()
    cfg["fax"]["self_attn"]["dropout"] = 0.0          # the eager step draws its masks from host seeds, the replay from the device word
    cfg["fax_fusion"]["drop_out"] = 0.0
    batches = [{k: v.to(cuda) for k, v in synth.opv2v_batch(agents=2, cams=2, image=128, max_cav=3, seed=s).items()} for s in (3, 4)]
    crit = host.VanillaSegLoss({"d_weights": 75.0, "s_weights": 15.0, "l_weights": 50, "d_coe": 2.0, "s_coe": 0.0, "target": "dynamic"})
    models = [_train_module(host.CorpBEVT(copy.deepcopy(cfg)), cuda) for _ in range(2)]
    with torch.no_grad():
        shp = models[0].eval()(dict(batches[0]))["dynamic_seg"].shape
    models[0].train()
    for i, b in enumerate(batches):
        g = torch.Generator().manual_seed(50 + i)
        b["gt_dynamic"] = (torch.rand(shp[:2] + shp[3:], generator=g) > 0.8).long().to(cuda)
        b["gt_static"] = torch.zeros(shp[:2] + shp[3:], dtype=torch.long, device=cuda)
    init = {k: v.detach().clone() for k, v in models[0].state_dict().items()}
    # lr 2e-3: with 1e-2 two EAGER bf16 runs of this small model drift apart by 5e-3 in the step-4 loss (2e-2 by step 6) once the attention
    # backward runs on the bf16 matrix path - its bias-table gradient is accumulated with atomics whose order now varies between runs
    # (profiles/r04_train_eager_repro.txt); the smaller step keeps that noise from being amplified through the updates
    opts = [torch.optim.SGD(m.parameters(), lr=2e-3 if amp else 1e-2, momentum=0.9) for m in models]
    dt = torch.bfloat16 if amp else None
    steps = 4
    eager_losses = []
    for i in range(steps):
        opts[0].zero_grad(set_to_none=True)
        with torch.enable_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            loss = crit(models[0](dict(batches[i % 2])), batches[i % 2])
        loss.backward()
        opts[0].step()
        eager_losses.append(float(loss.detach()))
    cap = host.CapturedTrainStep(models[1], lambda o, b: crit(o, b), opts[1], batches[0], autocast_dtype=dt)
    # the warm-up steps inside the constructor must not leave a trace in the model
    for k, v in models[1].state_dict().items():
        assert torch.equal(v, init[k]), "state %s changed by the capture" % k
    cap_losses = [float(cap.step(batches[i % 2])) for i in range(steps)]
    for a, b in zip(eager_losses, cap_losses):
        assert abs(a - b) <= 5e-3 * max(1.0, abs(a)), (eager_losses, cap_losses)
    assert cap_losses[-1] < cap_losses[0]
    se, sc = models[0].state_dict(), models[1].state_dict()
    num = den = 0.0
    for k in se:
        if k.endswith("num_batches_tracked"):
            assert int(se[k]) == int(sc[k]) == int(init[k]) + steps, k
            continue
        de, dc = (se[k] - init[k]).double(), (sc[k] - init[k]).double()
        num += float(((de - dc) ** 2).sum())
        den += float((de ** 2).sum())
    assert den > 0 and (num / den) ** 0.5 <= 2e-2, (num / den) ** 0.5
    # a batch of another shape is refused, not silently mis-replayed
    bad = dict(batches[0])
    bad["inputs"] = bad["inputs"][:1]
    with pytest.raises(CobevtHipError):
        cap.step(bad)


def test_captured_train_step_keeps_existing_optimizer_state(cuda):
    """an optimizer that already carries state (an eager step taken before the capture, resumed momentum) keeps it
    through CapturedTrainStep's warm-up steps; only state the warm-up itself creates is reset"""
    import copy
    cfg = synth.corpbevt_small_config()
    cfg["fax"]["self_attn"]["dropout"] = 0.0
    cfg["fax_fusion"]["drop_out"] = 0.0
    batch = {k: v.to(cuda) for k, v in synth.opv2v_batch(agents=2, cams=2, image=128, max_cav=3, seed=3).items()}
    crit = host.VanillaSegLoss({"d_weights": 75.0, "s_weights": 15.0, "l_weights": 50, "d_coe": 2.0, "s_coe": 0.0, "target": "dynamic"})
    model = _train_module(host.CorpBEVT(copy.deepcopy(cfg)), cuda)
    with torch.no_grad():
        shp = model.eval()(dict(batch))["dynamic_seg"].shape
    model.train()
    batch["gt_dynamic"] = (torch.rand(shp[:2] + shp[3:], generator=torch.Generator().manual_seed(5)) > 0.8).long().to(cuda)
    batch["gt_static"] = torch.zeros(shp[:2] + shp[3:], dtype=torch.long, device=cuda)
    opt = torch.optim.SGD(model.parameters(), lr=1e-2, momentum=0.9)
    with torch.enable_grad():
        loss = crit(model(dict(batch)), batch)
    loss.backward()
    opt.step()
    del loss
    opt.zero_grad(set_to_none=True)
    mom = {id(p): st["momentum_buffer"].clone() for p, st in opt.state.items() if st.get("momentum_buffer") is not None}
    assert mom and any(float(v.abs().max()) > 0 for v in mom.values())
    host.CapturedTrainStep(model, lambda o, b: crit(o, b), opt, batch)
    for p, st in opt.state.items():
        if id(p) in mom:
            assert torch.equal(st["momentum_buffer"], mom[id(p)])


def test_cvt_cross_attention_gradients(cuda):
    """cvt_modules.CrossAttention in train() mode (per-camera attentions merged by a softmax over their log-sum-exp, the lse gradient
    entering the attention backward kernels) against torch autograd through the oracle's single softmax over all cameras' keys
    (oracle.cvt.cross_attention, cvt_modules.py:116-170): output, input gradients and every parameter gradient"""
    import oracle.cvt as o_cvt
    from cobevt_amd.host import training
    g = torch.Generator().manual_seed(21)
    b, n, d, H, W, h, w, heads = 2, 3, 64, 8, 12, 6, 10, 2
    m = _train_module(host.CrossAttention(d, heads, 32, True), cuda)
    sd = _oracle_sd(m)
    q0, k0, v0 = torch.randn(b, n, d, H, W, generator=g), torch.randn(b, n, d, h, w, generator=g), torch.randn(b, n, d, h, w, generator=g)
    s0 = torch.randn(b, d, H, W, generator=g)
    with torch.enable_grad():
        ins_ref = [_leaf(t) for t in (q0, k0, v0, s0)]
        out_ref = o_cvt.cross_attention(sd, "", *ins_ref, heads, 32)
        ins = [_leaf(t, cuda) for t in (q0, k0, v0, s0)]
        tok = lambda t: t.reshape(t.shape[0], t.shape[1], d, -1).permute(0, 1, 3, 2)
        z = training.cvt_cross_attention(m, tok(ins[0]).contiguous(), tok(ins[1]).contiguous(), tok(ins[2]).contiguous(),
                                         ins[3].reshape(b, d, H * W).permute(0, 2, 1))
        out = z.reshape(b, H, W, d).permute(0, 3, 1, 2)
        _compare(m, sd, out, out_ref, ins, ins_ref, "CVT CrossAttention")


@pytest.mark.parametrize("kind,core,fwd", [("single", "cross_view_transformer", "cross_view_transformer_forward"),
                                           ("swap_fuse", "cross_view_transformer_swap_fuse", "cross_view_transformer_swap_fuse_forward"),
                                           ("fcooper", "cross_view_transformer_fcooper", "cross_view_transformer_fcooper_forward"),
                                           ("att_fuse", "cross_view_transformer_att_fuse", "cross_view_transformer_att_fuse_forward")])
def test_cvt_baselines_train_gradients_vs_oracle(cuda, kind, core, fwd):
    """The CVT baselines in train() mode - ResNet encoder, CrossViewModule (camera-paired cross attention),
    STTF warp, the model's fusion (swap fusion / F-Cooper max / per-pixel agent attention), decoder, head - against torch autograd
    through the oracle: logits and every parameter gradient (BatchNorms frozen, dropout off: the oracle is the eval-mode function).
    Same gates as the whole-model CorpBEVT test: a deep ReLU network, gradients to 5e-3 rms / 2e-2 max."""
    import copy
    import oracle.cvt as o_cvt
    from cobevt_amd.registry import create_model
    cfg = synth.cvt_small_config(kind)
    for key in ("swap_fusion", "base_transformer"):
        if key in cfg:
            for dk in ("drop_out", "dropout"):
                if dk in cfg[key]:
                    cfg[key][dk] = 0.0
    m = _freeze_bn(_train_module(create_model({"model": {"core_method": core, "args": copy.deepcopy(cfg)}}), cuda))
    sd = _oracle_sd(m)
    batch = synth.opv2v_batch(agents=1 if kind == "single" else 2, cams=2, image=128, max_cav=3, seed=cases.SEED)
    with torch.enable_grad():
        out_ref = getattr(o_cvt, fwd)(sd, cfg, dict(batch))["dynamic_seg"]
        out = m({k: v.to(cuda) for k, v in batch.items()})["dynamic_seg"]
        assert_close(out, golden("gv17_cvt_baselines")[kind + "_dynamic_seg"], TOL, "train-mode forward vs the reference's logits")
        _compare(m, sd, out, out_ref, [], [], "CVT " + kind, grad_tol=2e-2, rms_tol=5e-3)


@pytest.mark.parametrize("kind,core,fwd", [("v2vnet", "cross_view_transformer_v2vnet", "cross_view_transformer_v2vnet_forward"),
                                           ("disconet", "cross_view_transformer_disconet", "cross_view_transformer_disconet_forward")])
def test_cvt_pairwise_baselines_train_gradients_vs_oracle(cuda, kind, core, fwd):
    """V2VNet (ConvGRU message passing) and DiscoNet (pixel-weighted softmax fusion) on the CVT encoder in train() mode: the pairwise warp
    with its adjoint kernel, the flipped-domain 3x3 convolutions as re-indexed views of the parameters, against torch autograd through
    oracle/v2v.py (the reference's transposed + flipped formulation): logits and every parameter gradient, BatchNorms frozen"""
    import copy
    import oracle.v2v as o_v2v
    from cobevt_amd.registry import create_model
    cfg = synth.cvt_small_config(kind)
    m = _freeze_bn(_train_module(create_model({"model": {"core_method": core, "args": copy.deepcopy(cfg)}}), cuda))
    sd = _oracle_sd(m)
    batch = synth.opv2v_batch(agents=2, cams=2, image=128, max_cav=3, seed=cases.SEED)
    with torch.enable_grad():
        out_ref = getattr(o_v2v, fwd)(sd, cfg, dict(batch))["dynamic_seg"]
        out = m({k: v.to(cuda) for k, v in batch.items()})["dynamic_seg"]
        assert_close(out, golden("gv17_cvt_baselines")[kind + "_dynamic_seg"], TOL, "train-mode forward vs the reference's logits")
        _compare(m, sd, out, out_ref, [], [], "CVT " + kind, grad_tol=2e-2, rms_tol=5e-3)


def _fwd_bwd(fn, x0, w):
    x = x0.clone().requires_grad_(True)
    y = fn(x)
    (y.float() * w).sum().backward()
    return y.detach(), x.grad.detach().clone()


def test_swish_depthwise_resize_vs_torch(cuda):
    """the nuScenes-path Functions of csrc/train_nusc.hip against torch's own differentiable ops on the device: swish (fp32 / bf16),
    the depthwise convolution with TensorFlow-"same" static padding (3x3 / 5x5, stride 1 / 2, odd sizes, a pad that leaves input rows
    unused), the align_corners bilinear resize (its backward is the adjoint kernel)"""
    F = torch.nn.functional
    g = torch.Generator().manual_seed(31)
    with torch.enable_grad():
        # swish
        for dt, tol in ((torch.float32, 1e-5), (torch.bfloat16, 1e-2)):
            x0 = (torch.randn(2, 24, 7, 9, generator=g) * 3).to(cuda).to(dt).contiguous(memory_format=torch.channels_last)
            w = torch.randn(x0.shape, generator=g).to(cuda)
            got = _fwd_bwd(lambda t: ag.swish(t).float(), x0, w)
            ref = _fwd_bwd(lambda t: (t.float() * torch.sigmoid(t.float())), x0, w)
            assert_close(got[0], ref[0], tol, "swish forward %s" % dt)
            assert_close(got[1].float(), ref[1].float(), tol, "swish backward %s" % dt)
        # depthwise
        for c, k, stride, pad, h, w_ in ((16, 3, 1, (1, 1), 9, 11), (24, 5, 2, (1, 2), 12, 15), (8, 3, 2, (0, 1), 10, 13), (32, 5, 1, (2, 2), 7, 8),
                                         (8, 3, 2, (0, 0), 10, 10)):
            conv = torch.nn.Conv2d(c, c, k, stride=stride, groups=c, bias=False).to(cuda)
            x0 = torch.randn(2, c, h, w_, generator=g).to(cuda)
            def run(fn):
                conv.zero_grad()
                x = x0.clone().requires_grad_(True)
                y = fn(x)
                wgt = synth.procedural_input("dw.w%d%d" % (c, k), tuple(y.shape), 3).to(cuda)
                (y * wgt).sum().backward()
                return y.detach(), x.grad.clone(), conv.weight.grad.clone()
            got = run(lambda x: ag.depthwise_conv2d(x, conv, pad))
            ref = run(lambda x: F.conv2d(F.pad(x, (pad[0], pad[1], pad[0], pad[1])), conv.weight, None, stride=stride, groups=c))
            for a, b, what in zip(got, ref, ("forward", "dX", "dW")):
                assert_close(a, b, 1e-4, "depthwise %dx%d s%d pad %s %s" % (k, k, stride, pad, what))
        # bilinear resize
        x0 = torch.randn(2, 16, 5, 7, generator=g).to(cuda)
        w = torch.randn(2, 16, 10, 14, generator=g).to(cuda)
        got = _fwd_bwd(lambda t: ag.resize_bilinear(t, 10, 14), x0, w)
        ref = _fwd_bwd(lambda t: F.interpolate(t, size=(10, 14), mode="bilinear", align_corners=True), x0, w)
        assert_close(got[0], ref[0], 1e-5, "bilinear resize forward")
        assert_close(got[1], ref[1], 1e-5, "bilinear resize backward (adjoint)")


def test_sigmoid_focal_losses_backward(cuda):
    """BinarySegmentationLoss (grouped labels, visibility mask, alpha) and CenterLoss (soft labels) of the nuScenes experiments: value and
    gradient w.r.t. the logits against the torch restatement; MultipleLoss sums them and back-propagates"""
    from cobevt_amd.host import nuscenes as nu
    g = torch.Generator().manual_seed(8)
    b, h, w = 2, 20, 24
    pred_bev, pred_ctr = torch.randn(b, 1, h, w, generator=g) * 2, torch.randn(b, 1, h, w, generator=g) * 2
    label = (torch.rand(b, 12, h, w, generator=g) > 0.7).float()
    center = torch.rand(b, 1, h, w, generator=g)
    vis = torch.randint(0, 5, (b, h, w), generator=g).to(torch.uint8)
    batch = {"bev": label.to(cuda), "center": center.to(cuda), "visibility": vis.to(cuda)}
    losses = nu.MultipleLoss({"bev": nu.BinarySegmentationLoss(label_indices=[[4, 5, 6, 7, 8, 10, 11]], min_visibility=2, alpha=0.25, gamma=2.0),
                              "bev_weight": 1.0, "center": nu.CenterLoss(min_visibility=2, alpha=-1.0, gamma=2.0), "center_weight": 0.1})
    with torch.enable_grad():
        pb, pc = _leaf(pred_bev, cuda), _leaf(pred_ctr, cuda)
        total, parts = losses({"bev": pb, "center": pc}, batch)
        total.backward()
        rb, rc = _leaf(pred_bev), _leaf(pred_ctr)
        ref_b = focal_reference(rb, label, vis, [[4, 5, 6, 7, 8, 10, 11]], 2, 0.25, 2.0)
        ref_c = focal_reference(rc, center, vis, None, 2, -1.0, 2.0)
        (ref_b + 0.1 * ref_c).backward()
    assert abs(float(parts["bev"]) - float(ref_b)) <= 1e-5 * max(1.0, abs(float(ref_b)))
    assert abs(float(parts["center"]) - float(ref_c)) <= 1e-5 * max(1.0, abs(float(ref_c)))
    assert_close(pb.grad, rb.grad, 1e-4, "d BinarySegmentationLoss / d logits")
    assert_close(pc.grad, rc.grad, 1e-4, "d CenterLoss / d logits")


def _nuscenes_model(cuda):
    import copy
    from cobevt_amd.host import nuscenes as nu
    c = cases.NUSCENES
    backbone = nu.EfficientNetExtractor(["reduction_2", "reduction_3", "reduction_4"], *c["image"])
    enc = nu.PyramidAxialEncoder(backbone, **copy.deepcopy(c["encoder"]))
    return _train_module(nu.CrossViewTransformer(enc, nu.Decoder(**c["decoder"]), c["dim_last"], c["outputs"]), cuda)


def test_nuscenes_sinbevt_trains_gradients_vs_oracle(cuda):
    """The nuScenes SinBEVT model (BASELINE configs[1]: 6 cameras 224 x 480, EfficientNet-B4 extractor, PyramidAxialEncoder, Decoder, two
    heads) in train() mode against torch autograd through the oracles (oracle/efficientnet.py + oracle/nuscenes.py): logits and every
    parameter gradient.  BatchNorms frozen and drop-connect off (the oracles are the eval-mode function); gates as for CorpBEVT."""
    import oracle.efficientnet as o_eff
    import oracle.nuscenes as o_nu
    c = cases.NUSCENES
    m = _freeze_bn(_nuscenes_model(cuda))
    for group in list(m.encoder.backbone.layers)[1:]:
        group.args = [[0.0] for _ in group.args]
    sd = _oracle_sd(m)
    _, image, intr, ext = cases.nuscenes_inputs()
    with torch.enable_grad():
        feats = o_eff.efficientnet_extractor(sd, "encoder.backbone.", ["reduction_2", "reduction_3", "reduction_4"], o_nu.normalize(image.flatten(0, 1)))
        ref = o_nu.cross_view_transformer(sd, c["encoder"], len(c["decoder"]["blocks"]), c["outputs"], feats, intr, ext)
        out = m({"image": image.to(cuda), "intrinsics": intr.to(cuda), "extrinsics": ext.to(cuda)})
        out_ref = torch.cat([ref["bev"], ref["center"]], 1)
        _compare(m, sd, torch.cat([out["bev"], out["center"]], 1), out_ref, [], [], "nuScenes SinBEVT", grad_tol=2e-2, rms_tol=5e-3)


def test_nuscenes_training_steps(cuda):
    """model_module.py:35-60 in miniature: full train() mode (BatchNorm batch statistics, drop-connect, attention dropout), MultipleLoss of
    BinarySegmentationLoss + CenterLoss, backward, AdamW; the loss goes down and the bf16 inference path follows the updated parameters"""
    from cobevt_amd.host import nuscenes as nu
    m = _nuscenes_model(cuda)
    _, image, intr, ext = cases.nuscenes_inputs()
    batch = {"image": image.to(cuda), "intrinsics": intr.to(cuda), "extrinsics": ext.to(cuda)}
    g = torch.Generator().manual_seed(4)
    batch["bev"] = (torch.rand(1, 12, 200, 200, generator=g) > 0.8).float().to(cuda)
    batch["center"] = torch.rand(1, 1, 200, 200, generator=g).to(cuda)
    batch["visibility"] = torch.randint(0, 5, (1, 200, 200), generator=g).to(torch.uint8).to(cuda)
    losses = nu.MultipleLoss({"bev": nu.BinarySegmentationLoss(label_indices=[[4, 5, 6, 7, 8, 10, 11]], min_visibility=2, alpha=-1.0, gamma=2.0),
                              "bev_weight": 1.0, "center": nu.CenterLoss(min_visibility=2, alpha=-1.0, gamma=2.0), "center_weight": 0.1})
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    seen = []
    with torch.enable_grad():
        for _ in range(5):
            opt.zero_grad(set_to_none=True)
            total, _ = losses(m(batch), batch)
            total.backward()
            opt.step()
            seen.append(float(total.detach()))
    assert np.isfinite(seen).all() and seen[-1] < seen[0], seen
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters() if p.requires_grad)
    m.eval()
    with torch.no_grad():
        y = m(batch)
    assert torch.isfinite(y["bev"]).all() and tuple(y["bev"].shape) == (1, 1, 200, 200)
