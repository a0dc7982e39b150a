"""CPU: the typed agent attention (host.HGTCavAttention, RTE, RelTemporalEncoding, CavPositionalEncoding) against the reference's float64
outputs (tests/golden/gv31_hgt.npz, written by tests/golden/make_golden_hgt.py), the folding algebra, ops.hgt_fold, the state-dict
contract, the error paths, the C ABI's argument checks, the launch sequence, and the intervals of tests/hgt_ref.py themselves: torch's
fp32 evaluation of the kernels' formulas stays inside them, four planted faults leave them."""
import ctypes
import json

import pytest
import torch

import hgt_ref as hr
from cobevt_amd.host import CavPositionalEncoding, HGTCavAttention, RelTemporalEncoding, RTE  # noqa: F401  (absent: every test here fails at import)
import launch_trace as lt
import launch_trace_hgt as lth
from cobevt_amd import host, lib, ops
from cobevt_amd.lib import CobevtHipError
from conv_bounds_ref import F64, store_dtype

GOLDEN = hr.load_golden()


def _layer(name):
    c = hr.MODULE_CASES[name]
    return hr.fill_hgt_(host.PreNorm(c["dim"], host.HGTCavAttention(c["dim"], c["heads"], num_types=c["T"], num_relations=c["R"], dim_head=32)), 0).eval()


def _ln64(layer):
    return hr.LN(layer.norm.weight.detach().double(), layer.norm.bias.detach().double(), layer.norm.eps)


def _g(key):
    return torch.from_numpy(GOLDEN[key])


@pytest.mark.parametrize("name", sorted(hr.MODULE_CASES))
def test_restatement_equals_the_reference(name):
    c = hr.MODULE_CASES[name]
    x, mask, prior, types = hr.module_inputs(name)
    assert torch.equal(x, _g(name + ".x")) and torch.equal(mask, _g(name + ".mask")) and torch.equal(prior, _g(name + ".prior"))
    layer = _layer(name)
    sd = hr.state64(layer.fn)
    att = hr.unfolded(sd, x.double(), mask.double(), types, c["heads"])
    assert float((att - _g(name + ".attention64")).abs().max()) <= 1e-12
    y = hr.layer_restatement(sd, _ln64(layer), x.double(), mask.double(), prior.double(), c["heads"])
    assert float((y - _g(name + ".layer64")).abs().max()) <= 1e-12
    assert bool((mask.expand(c["B"], c["H"], c["W"], 1, c["L"])[..., 0] != 0).all())      # key 0 stays on: the reference is finite everywhere


def test_encodings_equal_the_reference():
    x, dts = hr.rte_inputs()
    m = hr.fill_hgt_(host.RTE(hr.RTE_CASE["dim"], hr.RTE_CASE["ratio"]), 0).eval()
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == json.loads(str(GOLDEN["rte.keys"]))
    assert set(m.state_dict()) == {"emb.emb.weight", "emb.lin.weight", "emb.lin.bias"}
    with torch.no_grad():
        assert float((hr.rte(hr.state64(m), x.double(), dts, 2) - _g("rte.out64")).abs().max()) <= 1e-12
        m64 = m.double()
        assert float((m64(x.double(), dts) - _g("rte.out64")).abs().max()) <= 1e-12
        assert float((m64.emb(x[0, 1].double(), dts[0, 1]) - _g("rel.out64")).abs().max()) <= 1e-12
        assert float((hr.rel_temporal(hr.state64(m64.emb), x[0, 1].double(), dts[0, 1], 2) - _g("rel.out64")).abs().max()) <= 1e-12
    p = host.CavPositionalEncoding(hr.POS_CASE["dim"], hr.POS_CASE["cav_num"])
    assert {k: list(v.shape) for k, v in p.state_dict().items()} == json.loads(str(GOLDEN["pos.keys"]))
    xp = hr.pos_inputs()
    assert float((p.double()(xp.double()) - _g("pos.out64")).abs().max()) <= 1e-12
    assert float((hr.cav_pos(hr.state64(p), xp.double()) - _g("pos.out64")).abs().max()) <= 1e-12
    with pytest.raises(CobevtHipError, match="whole table"):
        p(xp[:, :2])
    with pytest.raises(CobevtHipError, match="dts"):
        m(x, dts[:, :2])


@pytest.mark.parametrize("name", sorted(hr.MODULE_CASES))
def test_folded_form_equals_the_unfolded(name):
    c = hr.MODULE_CASES[name]
    x, mask, prior, types = hr.module_inputs(name)
    layer = _layer(name)
    sd, ln = hr.state64(layer.fn), _ln64(layer)
    y = hr.layer_restatement(sd, ln, x.double(), mask.double(), prior.double(), c["heads"])
    yf = hr.folded(hr.fold64(sd, ln), x.double(), mask, types, c["heads"], c["T"], ln_eps=ln.eps, residual=x.double())
    assert float((y - yf).abs().max()) <= 1e-12
    # each planted fault is the same function in both forms (the fold carries the first two, the attention the others) and is no small change
    right = hr.unfolded(sd, x.double(), mask.double(), types, c["heads"])
    for fault in hr.FAULTS:
        in_fold = fault in ("relation_index", "msg_not_transposed")
        bad = hr.unfolded(sd, x.double(), mask.double(), types, c["heads"], fault=fault)
        badf = hr.folded(hr.fold64(sd, None, fault if in_fold else None), x.double(), mask, types, c["heads"], c["T"], fault=None if in_fold else fault)
        assert float((bad - badf).abs().max()) <= 1e-12, fault
        assert float((bad - right).abs().max()) > 0.1, fault


@pytest.mark.parametrize("with_ln", (False, True))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_hgt_fold_matches_a_float64_fold(with_ln, dtype):
    layer = _layer("d128")
    ln = layer.norm if with_ln else None
    want = hr.fold64(hr.state64(layer.fn), _ln64(layer) if with_ln else None)
    got = ops.hgt_fold(layer.fn, ln=ln, dtype=dtype)
    c = hr.MODULE_CASES["d128"]
    inner = c["heads"] * 32
    assert tuple(got.w_in.shape) == (c["T"], (1 + 2 * c["T"]) * inner, c["dim"]) and tuple(got.w_out.shape) == (c["T"], c["dim"], inner)
    assert got.w_in.dtype == dtype and got.w_out.dtype == dtype and got.b_in.dtype == torch.float32 and got.b_out.dtype == torch.float32
    assert (got.num_types, got.heads) == (c["T"], c["heads"])
    for g, w, dt in zip(got[:4], want, (dtype, torch.float32, dtype, torch.float32)):
        assert torch.equal(g.double(), hr.rne(w, dt))                              # ONE rounding of the float64 fold (through fp32, as every plan here)
    # the state dict form gives the same tensors
    sd = {k: v.detach().clone() for k, v in layer.fn.state_dict().items()}
    again = ops.hgt_fold(sd, ln=ln, dtype=dtype)
    assert all(torch.equal(a, b) for a, b in zip(again[:4], got[:4]))


def test_hgt_fold_is_cached_per_parameter_objects():
    layer = _layer("d64")
    a = ops.hgt_fold(layer.fn, ln=layer.norm)
    assert ops.hgt_fold(layer.fn, ln=layer.norm) is a
    assert ops.hgt_fold(layer.fn) is not a                                       # without the LayerNorm: another entry
    with torch.no_grad():
        layer.fn.relation_att.mul_(2.0)                                          # an in-place update moves the version counter
    b = ops.hgt_fold(layer.fn, ln=layer.norm)
    assert b is not a and not torch.equal(b.w_in, a.w_in)
    with torch.no_grad():
        layer.norm.bias.add_(1.0)
    c = ops.hgt_fold(layer.fn, ln=layer.norm)
    assert c is not b and torch.equal(c.w_in, b.w_in) and not torch.equal(c.b_in, b.b_in)
    n = len(ops._HGT_FOLDS)
    del layer, a, b, c
    assert len(ops._HGT_FOLDS) < n                                               # the entries go with their parameters


def test_state_dict_contract():
    for name, c in hr.MODULE_CASES.items():
        m = _layer(name).fn
        want = json.loads(str(GOLDEN[name + ".keys"]))
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == want
        assert len(want) == 2 + 8 * c["T"]
        fresh = host.HGTCavAttention(c["dim"], c["heads"], num_types=c["T"], num_relations=c["R"], dim_head=32)
        fresh.load_state_dict({k: torch.full(s, 0.25) for k, s in want.items()}, strict=True)
        assert float(fresh.relation_msg.detach().min()) == 0.25
    assert len(json.loads(str(GOLDEN["d64.keys"]))) == 18
    # the reference's signature, by position
    m = host.HGTCavAttention(64, 2, 2, 4, 32, 0.1)
    assert (m.heads, m.num_types, tuple(m.relation_att.shape), m.drop_out.p) == (2, 2, (4, 2, 32, 32), 0.1)


def test_constructor_mask_and_mode_errors(monkeypatch):
    with pytest.raises(CobevtHipError, match="dim_head = 32"):
        host.HGTCavAttention(64, 2)                                              # the reference's default dim_head = 64
    with pytest.raises(CobevtHipError, match="num_relations=3"):
        host.HGTCavAttention(64, 2, num_types=2, num_relations=3, dim_head=32)
    host.HGTCavAttention(64, 2, num_types=2, num_relations=6, dim_head=32)       # more relations than T^2: the first T^2 are used
    with pytest.raises(CobevtHipError, match="dim=48"):
        host.HGTCavAttention(48, 2, dim_head=32)
    x, mask, prior, _ = hr.module_inputs("d64")
    layer = _layer("d64")
    with pytest.raises(CobevtHipError, match="ROCm device"):
        layer.fn(x, mask, prior)                                                 # a CPU tensor: no fallback
    layer.train()
    with pytest.raises(CobevtHipError, match="eval"):
        layer(x, mask=mask, prior_encoding=prior)
    with pytest.raises(CobevtHipError, match="inference-only"):
        layer.fn.forward_fused(x, mask=mask, prior_encoding=prior)
    layer.eval()
    rec = lt.Recorder()
    lt.install(monkeypatch.setattr, rec)
    c = hr.MODULE_CASES["d64"]
    with torch.no_grad(), host.compute_dtype("fp32"):
        with pytest.raises(CobevtHipError, match=r"ends in \(L, 1\)"):
            layer(x, mask=torch.ones(c["B"], c["H"], c["W"], c["L"], 1), prior_encoding=prior)       # the shape the reference's comment names
        with pytest.raises(CobevtHipError, match="not broadcastable"):
            layer(x, mask=torch.ones(c["B"], c["L"] + 1), prior_encoding=prior)
        with pytest.raises(CobevtHipError, match="prior_encoding"):
            layer(x, mask=mask, prior_encoding=None)
        with pytest.raises(CobevtHipError, match="prior_encoding"):
            layer(x, mask=mask, prior_encoding=prior[..., :2])
        assert rec.records == []
        for ok in (mask, torch.ones(c["B"], 1, 1, 1, c["L"]), None):               # what CavAttention accepts
            layer(x, mask=ok, prior_encoding=prior)
        assert len(rec.records) == 9


def test_ops_preconditions(monkeypatch):
    """all raised before the device check and before any launch: CPU tensors reach them"""
    rec = lt.Recorder()
    monkeypatch.setattr("cobevt_amd.lib.load", rec.load)
    x, w, b = torch.zeros(2, 3, 5, 64), torch.zeros(2, 96, 64), torch.zeros(2, 96)
    ty = torch.zeros(2, dtype=torch.int32)
    for bad, match in ((dict(x=torch.zeros(2, 3, 5, 64).transpose(1, 2)), "contiguous"), (dict(w=w.bfloat16()), "w must"), (dict(w=torch.zeros(2, 96, 32)), "w must"),
                       (dict(w=torch.zeros(2, 80, 64), b=torch.zeros(2, 80)), "multiples of 32"), (dict(b=torch.zeros(2, 64)), "bias must"),
                       (dict(ty=ty.long()), "types must"), (dict(rows=7), "groups of"), (dict(res=torch.zeros(2, 3, 5, 64)), "residual must"),
                       (dict(out=torch.zeros(2, 3, 5, 96).bfloat16()), "out must"), (dict(eps=-1.0), "ln_eps")):
        a = dict(x=x, w=w, b=b, ty=ty, rows=15, res=None, out=None, eps=None)
        a.update(bad)
        with pytest.raises(CobevtHipError, match=match):
            ops.typed_linear(a["x"], a["w"], a["b"], a["ty"], a["rows"], residual=a["res"], ln_eps=a["eps"], out=a["out"])
    with pytest.raises(CobevtHipError, match="K=1024"):
        ops.typed_linear(torch.zeros(1, 4, 1024), torch.zeros(1, 32, 1024), torch.zeros(1, 32), ty[:1], 4, ln_eps=1e-5)
    with pytest.raises(CobevtHipError, match="ROCm device"):
        ops.typed_linear(x, w, b, ty, 15)
    proj = torch.zeros(2, 3, 3, 5, 5 * 64)
    ty = torch.zeros(2, 3, dtype=torch.int32)
    for bad, match in ((dict(proj=proj[..., :300].contiguous()), "not \\(1 \\+ 2 T\\)"), (dict(T=3), "not \\(1 \\+ 2 T\\)"), (dict(ty=ty[:1]), "types must"),
                       (dict(mask=torch.ones(2, 3, 5, 1, 3)), "mask must"), (dict(mask=torch.ones(2, 3, 5, 3).double()), "mask must"),
                       (dict(proj=torch.zeros(1, 9, 1, 1, 320), ty=torch.zeros(1, 9, dtype=torch.int32)), "9 agents"),
                       (dict(out=torch.zeros(2, 3, 3, 5, 32)), "out= must")):
        a = dict(proj=proj, ty=ty, T=2, mask=None, out=None)
        a.update(bad)
        with pytest.raises(CobevtHipError, match=match):
            ops.hgt_attention(a["proj"], a["ty"], 2, a["T"], mask=a["mask"], out=a["out"])
    with pytest.raises(CobevtHipError, match="ROCm device"):
        ops.hgt_attention(proj, ty, 2, 2)
    assert rec.records == []


def test_c_abi_validates_arguments_before_any_launch():
    """both entries reject null pointers, unknown codes (COBEVT_ERR_ARG = 1), shapes they do not serve (COBEVT_ERR_SHAPE = 2) and sizes beyond
    their limits (COBEVT_ERR_UNSUPPORTED = 4) without touching a device, in all three libraries (one shared object)"""
    buf = (ctypes.c_float * 64)()                               # host memory: only its address is looked at
    addr = (ctypes.addressof(buf) + 15) // 16 * 16
    ptr, odd = ctypes.c_void_p(addr), ctypes.c_void_p(addr + 4)
    for variant in ("", "f32s", "f32h"):
        f = lib.load(variant).cobevt_typed_linear

        def lin(x=ptr, w=ptr, b=ptr, ty=ptr, res=None, out=ptr, dims=(0, 2, 15, 64, 96, 2, 1), eps=1e-5, no_dims=False):
            return f(x, w, b, ty, res, out, None if no_dims else (ctypes.c_long * 7)(*dims), ctypes.c_float(eps), None)
        assert lin(x=None) == 1 and lin(w=None) == 1 and lin(b=None) == 1 and lin(ty=None) == 1 and lin(out=None) == 1 and lin(no_dims=True) == 1
        assert lin(dims=(2, 2, 15, 64, 96, 2, 1)) == 1 and lin(dims=(0, 2, 15, 64, 96, 2, 2)) == 1 and lin(eps=-1.0) == 1 and lin(eps=float("nan")) == 1
        for bad in ((0, 0, 15, 64, 96, 2, 1), (0, 65536, 15, 64, 96, 2, 1), (0, 2, 0, 64, 96, 2, 1), (0, 2, 15, 48, 96, 2, 1), (0, 2, 15, 0, 96, 2, 1),
                    (0, 2, 15, 64, 80, 2, 1), (0, 2, 15, 64, 0, 2, 1), (0, 2, 15, 64, 96, 0, 1), (0, 2, 2 ** 31, 64, 96, 2, 1), (0, 2, 2 ** 36, 64, 96, 2, 1),
                    (0, 2, -1, 64, 96, 2, 1), (0, 2, 15, 64, 2 ** 20 + 32, 2, 1), (0, 2, 15, 64, 96, 65536, 1)):
            assert lin(dims=bad) == 2, bad
        assert lin(x=odd) == 2 and lin(out=odd) == 2 and lin(res=odd) == 2
        assert lin(dims=(0, 2, 15, 544, 96, 2, 1)) == 4 and lin(dims=(1, 2, 15, 1056, 96, 2, 0)) == 4
        g = lib.load(variant).cobevt_hgt_attention_nhwc

        def att(proj=ptr, ty=ptr, mask=None, out=ptr, dtype=0, b=2, l=3, hw=15, heads=2, t=2):
            return g(proj, ty, mask, out, dtype, b, l, hw, heads, t, ctypes.c_float(0.1767767), None)
        assert att(proj=None) == 1 and att(ty=None) == 1 and att(out=None) == 1 and att(dtype=2) == 1
        for bad in (dict(b=0), dict(l=0), dict(hw=0), dict(hw=-1), dict(heads=0), dict(t=0), dict(b=16384, l=4), dict(proj=odd), dict(out=odd)):
            assert att(**bad) == 2, bad
        assert att(l=9) == 4 and att(heads=65) == 4 and att(t=65) == 4


@pytest.mark.parametrize("mode", lt.MODES)
def test_launch_trace(mode, monkeypatch):
    """PreNorm(HGTCavAttention) + x: three launches - typed projection with the LayerNorm, attention, typed output projection - in the
    active library, the scalar arguments pinned"""
    got = json.loads(json.dumps(lth.trace(mode, monkeypatch.setattr)))
    assert got == lth.read_fixture(mode)
    assert [r[1] for r in got] == ["cobevt_typed_linear", "cobevt_hgt_attention_nhwc", "cobevt_typed_linear"]
    c = hr.MODULE_CASES[lth.CASE]
    code = 0 if mode == "bf16" else 1
    rows, inner = c["H"] * c["W"], 32 * c["heads"]
    assert got[0][2][6] == [code, c["B"] * c["L"], rows, c["dim"], (1 + 2 * c["T"]) * inner, c["T"], 1]
    assert got[2][2][6] == [code, c["B"] * c["L"], rows, inner, c["dim"], c["T"], 0] and got[2][2][4] == "null"
    assert got[1][2][4:10] == [code, c["B"], c["L"], rows, c["heads"], c["T"]]


def test_residual_goes_into_the_third_launch(monkeypatch):
    rec = lt.Recorder()
    lt.install(monkeypatch.setattr, rec)
    x, mask, prior, _ = hr.module_inputs("d64")
    layer = _layer("d64")
    with torch.no_grad(), host.compute_dtype("fp32"):
        layer.fn.forward_fused(x, residual=x, ln=layer.norm, mask=mask, prior_encoding=prior)
    assert [r[1] for r in rec.records] == ["cobevt_typed_linear", "cobevt_hgt_attention_nhwc", "cobevt_typed_linear"]
    assert rec.records[0][2][4] == "null" and rec.records[2][2][4] == "ptr"


# ---------------------------------------------------------------------------------------------- the intervals
def _lin_f32(name, mode):
    """torch's fp32 evaluation of the kernel's formulas on the case's operands, rounded once to the storage type"""
    dt = store_dtype(mode)
    o = hr.linear_operands(name, dt)
    B, L, H, W = o["shape"]
    y = hr.typed_rows(o["x"].float().reshape(B, L, H * W, -1), o["w"].float(), o["b"].float(), o["types"].reshape(B, L), o["ln_eps"],
                      None if o["residual"] is None else o["residual"].float().reshape(B, L, H * W, -1), store=dt)
    return y.to(dt).to(F64).reshape(B * L * H * W, -1)


def _att_f32(name, mode, fault=None):
    dt = store_dtype(mode)
    o = hr.attention_operands(name, dt)
    return hr.attention_rows(o["proj"].float(), o["types"], o["mask"], o["heads"], o["T"], fault).to(dt).to(F64)


@pytest.mark.parametrize("mode", ("bf16", "fp32"))
@pytest.mark.parametrize("name", sorted(hr.LINEAR_CASES))
def test_fp32_evaluation_stays_inside_the_gemm_intervals(name, mode):
    iv = hr.linear_interval(name, mode)
    got = _lin_f32(name, mode)
    assert hr.outside(got, iv) == 0
    if mode == "fp32":
        assert hr.used(got, iv) < 1.0


@pytest.mark.parametrize("mode", ("bf16", "fp32"))
@pytest.mark.parametrize("name", sorted(hr.ATTENTION_CASES))
def test_fp32_evaluation_stays_inside_the_attention_intervals(name, mode):
    iv = hr.attention_case_interval(name, mode)
    got = _att_f32(name, mode)
    assert hr.outside(got, iv) == 0
    if mode == "fp32":
        assert hr.used(got, iv) < 1.0
    if hr.ATTENTION_CASES[name][7] == "dead":
        assert bool((iv.lo[-1, :, -1, -1] == 0).all()) and bool((iv.hi[-1, :, -1, -1] == 0).all())      # a query without a key: exactly 0


@pytest.mark.parametrize("mode", ("bf16", "fp32"))
@pytest.mark.parametrize("fault", hr.FAULTS)
def test_planted_faults_leave_the_intervals(fault, mode):
    """the two faults of the fold leave the projection's interval (computed with the right fold), the two of the attention the attention's,
    on most of the elements they touch"""
    dt = store_dtype(mode)
    if fault in ("relation_index", "msg_not_transposed"):
        c = hr.MODULE_CASES["d64"]
        x, _, _, types = hr.module_inputs("d64")
        layer = _layer("d64")
        sd, ln = hr.state64(layer.fn), _ln64(layer)
        inner = 32 * c["heads"]
        rnd = lambda f: (hr.rne(f[0], dt), f[1].float().double())                        # noqa: E731  (the fold as ops.hgt_fold stores it)
        w, b = rnd(hr.fold64(sd, ln))
        wb, bb = rnd(hr.fold64(sd, ln, fault))
        x64 = hr.rne(x.double(), dt).reshape(-1, c["dim"])
        rows = c["H"] * c["W"]
        iv = hr.typed_linear_interval(x64, w, b, types.reshape(-1), rows, mode, ln.eps)
        ev = lambda w_, b_: hr.typed_rows(x64.float().reshape(c["B"], c["L"], rows, -1), w_.float(), b_.float(), types, ln.eps, store=dt).to(dt).to(F64).reshape(-1, w.shape[1])   # noqa: E731
        assert hr.outside(ev(w, b), iv) == 0
        bad = ev(wb, bb)
        out = (bad < iv.lo) | (bad > iv.hi)
        # what the fault touches.  relation_index: a T + b = b T + a where a = b, so of a row of type b the key and value variants a != b;
        # msg_not_transposed: every value column.  Everything else is the same function and stays inside
        a_col = (torch.arange(w.shape[1]) // inner - 1) % c["T"]
        b_row = types.reshape(-1).long().repeat_interleave(rows)
        touched = torch.arange(w.shape[1])[None, :] >= ((1 + c["T"]) * inner if fault == "msg_not_transposed" else inner)
        if fault == "relation_index":
            touched = touched & (a_col[None, :] != b_row[:, None])
        touched = touched.expand_as(out)
        assert float(out[touched].double().mean()) > 0.9 and int(touched.sum()) * 4 >= out.numel()
        assert int(out[~touched].sum()) == 0
        assert int(out[:, :inner].sum()) == 0                                            # the query columns are the same function
    else:
        name = "l3_33_padded" if fault == "mask_queries" else "l5_3x5_h8_t3"
        iv = hr.attention_case_interval(name, mode)
        bad = _att_f32(name, mode, fault)
        out = (bad < iv.lo) | (bad > iv.hi)
        if fault == "mask_queries":
            assert float(out[0].double().mean()) > 0.9                                   # sample 0 has a masked agent; sample 1 has none
            assert int(out[1].sum()) == 0
        else:
            assert float(out.double().mean()) > 0.5
