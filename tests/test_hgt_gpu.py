"""GPU: cobevt_typed_linear and cobevt_hgt_attention_nhwc against the per-element float64 intervals of tests/hgt_ref.py (its docstring
derives them; no constant is fitted to a kernel), in bf16 and fp32 storage, at the smallest shapes that can break them; host.HGTCavAttention
against the reference's float64 outputs (tests/golden/gv31_hgt.npz), against host.CavAttention where the two are the same function,
and inside a captured graph whose replays follow types, delays and mask rewritten in place.

Module-level gates are multiples of the REFERENCE's own deviation from its float64 run on the same case, recorded in the fixture by
tests/golden/make_golden_hgt.py (max abs over the layer PreNorm(HGTCavAttention)(x) + x):

    case    max|out|   reference fp32   bf16 autocast     fp32 gate (4 x)   bf16 gate (2 x)
    d64     5.6789     1.994e-06        3.697e-02         7.976e-06         7.394e-02
    d128    5.3538     1.796e-06        2.808e-02         7.184e-06         5.616e-02

4 x in fp32: sums of the same length in fp32 in another order.  2 x in bf16: the storage roundings fall at other places than autocast's.
Every test prints the fraction it uses.
"""
import pytest
import torch

import hgt_ref as hr
from cobevt_amd.host import CavPositionalEncoding, HGTCavAttention, RelTemporalEncoding, RTE  # noqa: F401  (absent: every test here fails at import)
from cobevt_amd import host, ops
from conv_bounds_ref import F64, store_dtype

pytestmark = pytest.mark.gpu

MODES = ("bf16", "fp32")
SENTINEL = {torch.bfloat16: (torch.int16, 0x7FC1), torch.float32: (torch.int32, 0x7FC12345)}        # two NaN payloads no kernel produces
GUARD = 64                                                                                           # rows behind the output that must keep the sentinel
FP32_FACTOR, BF16_FACTOR = 4.0, 2.0


def _sentinel(shape, dt, device):
    it, word = SENTINEL[dt]
    return torch.full(shape, word, dtype=it, device=device).view(dt)


def _untouched(t):
    it, word = SENTINEL[t.dtype]
    return bool((t.view(it) == word).all())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(hr.LINEAR_CASES))
def test_typed_linear_inside_its_intervals(cuda, name, mode):
    dt = store_dtype(mode)
    o = hr.linear_operands(name, dt)
    iv = hr.linear_interval(name, mode)
    B, L, H, W = o["shape"]
    m, n = o["x"].shape[0], o["w"].shape[1]
    x = o["x"].to(dt).to(cuda).reshape(B, L, H, W, -1)
    w, b, ty = o["w"].to(dt).to(cuda), o["b"].float().to(cuda), o["types"].to(cuda)
    res = None if o["residual"] is None else o["residual"].to(dt).to(cuda).reshape(B, L, H, W, n)
    runs = []
    for _ in range(2):
        buf = _sentinel((m + GUARD, n), dt, cuda)
        out = ops.typed_linear(x, w, b, ty, o["rows"], residual=res, ln_eps=o["ln_eps"], out=buf[:m].view(B, L, H, W, n))
        assert out.data_ptr() == buf.data_ptr() and _untouched(buf[m:])            # a tail tile stores nothing behind its group
        runs.append(buf[:m].clone())
    assert torch.equal(runs[0].view(SENTINEL[dt][0]), runs[1].view(SENTINEL[dt][0]))     # bit-identical
    got = runs[0].cpu().to(F64)
    assert bool(torch.isfinite(got).all())
    print("%s %s: used %.3f of e, %d of %d outside" % (name, mode, hr.used(got, iv), hr.outside(got, iv), got.numel()))
    assert hr.outside(got, iv) == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(hr.ATTENTION_CASES))
def test_hgt_attention_inside_its_intervals(cuda, name, mode):
    dt = store_dtype(mode)
    o = hr.attention_operands(name, dt)
    iv = hr.attention_case_interval(name, mode)
    proj = o["proj"].to(dt).to(cuda)
    B, L, H, W, _ = proj.shape
    inner = 32 * o["heads"]
    ty = o["types"].to(cuda)
    mask = None if o["mask"] is None else o["mask"].to(cuda)
    runs = []
    for _ in range(2):
        buf = _sentinel((B * L * H * W + GUARD, inner), dt, cuda)
        out = ops.hgt_attention(proj, ty, o["heads"], o["T"], mask=mask, out=buf[:B * L * H * W].view(B, L, H, W, inner))
        assert out.data_ptr() == buf.data_ptr() and _untouched(buf[B * L * H * W:])
        runs.append(out.clone())
    assert torch.equal(runs[0].view(SENTINEL[dt][0]), runs[1].view(SENTINEL[dt][0]))
    got = runs[0].cpu().to(F64)
    assert bool(torch.isfinite(got).all())
    print("%s %s: used %.3f of e, %d of %d outside" % (name, mode, hr.used(got, iv), hr.outside(got, iv), got.numel()))
    assert hr.outside(got, iv) == 0
    if hr.ATTENTION_CASES[name][7] == "dead":
        assert bool((got[-1, :, -1, -1] == 0).all())                               # a query whose keys are all masked: zeros, not NaN


def _layer(name, cuda):
    c = hr.MODULE_CASES[name]
    m = hr.fill_hgt_(host.PreNorm(c["dim"], host.HGTCavAttention(c["dim"], c["heads"], num_types=c["T"], num_relations=c["R"], dim_head=32)), 0)
    return m.eval().to(cuda)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(hr.MODULE_CASES))
def test_module_against_the_reference(cuda, name, mode):
    g = hr.load_golden()
    d32, d16, top = (float(v) for v in g[name + ".dev"])
    gate = FP32_FACTOR * d32 if mode == "fp32" else BF16_FACTOR * d16
    x, mask, prior, _ = hr.module_inputs(name)
    layer = _layer(name, cuda)
    with torch.no_grad(), host.compute_dtype(mode):
        y = layer(x.to(cuda), mask=mask.to(cuda), prior_encoding=prior.to(cuda)) + x.to(cuda)
        assert y.dtype == torch.float32
        fused = layer.fn.forward_fused(host.runtime.as_compute(x.to(cuda)), residual=host.runtime.as_compute(x.to(cuda)), ln=layer.norm,
                                       mask=mask.to(cuda), prior_encoding=prior.to(cuda))
    want = torch.from_numpy(g[name + ".layer64"])
    err = float((y.cpu().double() - want).abs().max())
    errf = float((fused.cpu().double() - want).abs().max())
    print("%s %s: max|err| %.3e = %.3f of the gate %.3e (max|out| %.4f); residual inside the kernel: %.3e = %.3f" % (name, mode, err, err / gate, gate, top, errf, errf / gate))
    assert err <= gate
    if mode == "fp32":
        assert errf <= gate                                                        # (bf16: the input itself is rounded to bf16 on this path)
        # the kernels do not depend on the library: the other fp32 modes give the same bits
        with torch.no_grad(), host.compute_dtype("fp32_split"):
            y2 = layer(x.to(cuda), mask=mask.to(cuda), prior_encoding=prior.to(cuda)) + x.to(cuda)
        assert torch.equal(y, y2)


@pytest.mark.parametrize("mode", MODES)
def test_one_type_with_identity_relations_is_cav_attention(cuda, mode):
    """T = 1, identity relation matrices and zero biases: HGTCavAttention computes CavAttention's function with the same weights.  Neither
    module has a closed bound of its own; each is held to ITS module gate - the factor of this file times the deviation of torch's run of
    the reference's procedure in that precision from its float64 run, on this case - and the two outputs differ by at most the sum."""
    dim, heads, B, L, H, W = 64, 2, 2, 3, 3, 5
    inner = 32 * heads
    cav = hr.fill_hgt_(host.PreNorm(dim, host.CavAttention(dim, heads, dim_head=32)), 0).eval()
    hgt = host.PreNorm(dim, host.HGTCavAttention(dim, heads, num_types=1, num_relations=1, dim_head=32)).eval()
    with torch.no_grad():
        cav.fn.to_out[0].bias.zero_()
        wq, wk, wv = cav.fn.to_qkv.weight.chunk(3, 0)
        for lin, w in ((hgt.fn.q_linears[0], wq), (hgt.fn.k_linears[0], wk), (hgt.fn.v_linears[0], wv), (hgt.fn.a_linears[0], cav.fn.to_out[0].weight)):
            lin.weight.copy_(w)
            lin.bias.zero_()
        eye = torch.eye(32).expand(1, heads, 32, 32)
        hgt.fn.relation_att.copy_(eye)
        hgt.fn.relation_msg.copy_(eye)
        hgt.norm.load_state_dict(cav.norm.state_dict())
    assert tuple(wq.shape) == (inner, dim)
    x = hr.procedural_input("hgt.cav.x", (B, L, H, W, dim), 0, -2.0, 2.0)
    mask = hr.make_mask("padded", B, L, H, W)
    prior = torch.zeros(B, L, H, W, 3)
    # the float64 reference and torch's own deviation from it in the precision of the mode
    sd = hr.state64(hgt.fn)
    ln = hr.LN(hgt.norm.weight.detach().double(), hgt.norm.bias.detach().double(), hgt.norm.eps)
    want = hr.layer_restatement(sd, ln, x.double(), mask.double(), prior.double(), heads)
    sd32 = {k: v.float() for k, v in sd.items()}
    ln32 = hr.LN(ln.weight.float(), ln.bias.float(), ln.eps)
    if mode == "fp32":
        dev = FP32_FACTOR * float((hr.layer_restatement(sd32, ln32, x, mask, prior, heads).double() - want).abs().max())
    else:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            dev = BF16_FACTOR * float((hr.layer_restatement(sd32, ln32, x, mask, prior, heads).double() - want).abs().max())
    cav, hgt = cav.to(cuda), hgt.to(cuda)
    with torch.no_grad(), host.compute_dtype(mode):
        a = cav(x.to(cuda), mask=mask.to(cuda)) + x.to(cuda)
        b = hgt(x.to(cuda), mask=mask.to(cuda), prior_encoding=prior.to(cuda)) + x.to(cuda)
    ea, eb, d = (float(t.abs().max()) for t in (a.cpu().double() - want, b.cpu().double() - want, (a - b).cpu().double()))
    print("%s: gate %.3e each; CavAttention %.3e, HGTCavAttention %.3e, between them %.3e" % (mode, dev, ea, eb, d))
    assert ea <= dev and eb <= dev and d <= 2.0 * dev


def test_two_layer_stack_replays_from_a_graph(cuda):
    """RTE, then two [PreNorm(HGTCavAttention) + x, PreNorm(FeedForward) + x] layers, captured once.  types and delays live in
    prior_encoding, the mask in its own buffer: replays after rewriting them in place equal the eager run on the new values bit for bit."""
    dim, heads, T, B, L, H, W = 64, 2, 2, 2, 3, 3, 5
    torch.manual_seed(0)
    rte = hr.fill_hgt_(host.RTE(dim, 2), 0).eval().to(cuda)
    layers = [(hr.fill_hgt_(host.PreNorm(dim, host.HGTCavAttention(dim, heads, num_types=T, num_relations=T * T, dim_head=32)), i).eval().to(cuda),
               hr.fill_hgt_(host.PreNorm(dim, host.FeedForward(dim, 2 * dim)), 10 + i).eval().to(cuda)) for i in range(2)]
    x = hr.procedural_input("hgt.graph.x", (B, L, H, W, dim), 0, -2.0, 2.0).to(cuda)

    def prior_of(types, dts):
        p = torch.zeros(B, L, H, W, 3)
        p[..., 1] = dts.float()[:, :, None, None]
        p[..., 2] = types.float()[:, :, None, None]
        return p

    settings = [(prior_of(hr.make_types("mixed", B, L, T), torch.tensor([[0, 1, 2], [3, 0, 1]])), hr.make_mask("pixel", B, L, H, W)),
                (prior_of(hr.make_types("equal", B, L, T), torch.tensor([[5, 0, 7], [0, 2, 2]])), hr.make_mask("dead", B, L, H, W)),
                (prior_of(1 - hr.make_types("mixed", B, L, T), torch.tensor([[1, 1, 0], [4, 9, 0]])), hr.make_mask("pixel", B, L, H, W).flip(0))]
    prior, mask = settings[0][0].clone().to(cuda), settings[0][1].clone().to(cuda)

    def run():
        y = host.runtime.as_compute(rte(x, prior[:, :, 0, 0, 1]))
        for attn, ff in layers:
            y = attn.fn.forward_fused(y, residual=y, ln=attn.norm, mask=mask, prior_encoding=prior)
            y = ff.fn.forward_fused(y, residual=y, ln=ff.norm)
        return y

    with torch.no_grad(), host.compute_dtype("fp32"):
        eager = []
        for p, m in settings:
            prior.copy_(p)
            mask.copy_(m)
            eager.append(run().clone())
        assert not torch.equal(eager[0], eager[1]) and not torch.equal(eager[0], eager[2])
        prior.copy_(settings[0][0])
        mask.copy_(settings[0][1])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = run()
        for i in (0, 1, 2, 0):
            prior.copy_(settings[i][0])
            mask.copy_(settings[i][1])
            graph.replay()
            assert torch.equal(out, eager[i]), i
        torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    del graph
