"""CPU: the launch sequence of every model (tests/launch_trace.py) against the fixtures under tests/golden/launch_traces/, and the
call path / library selection / COBEVT_FLAGS behaviour the routing code rests on.  No GPU and no built library: lib.load is a fake."""
import json
import math

import pytest
import torch

import launch_trace as lt
from cobevt_amd import autograd, host, lib, ops
from cobevt_amd.lib import CobevtHipError


@pytest.mark.parametrize("case", sorted(lt.CASES))
def test_launch_trace_matches_fixture(case, monkeypatch):
    """same symbols, same library per launch, same scalar arguments, in the same order as the fixture"""
    got = json.loads(json.dumps(lt.trace(case, monkeypatch.setattr)))
    want = lt.read_fixture(case)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            print("launch %d differs\n  traced:  %s\n  fixture: %s" % (i, json.dumps(g), json.dumps(w)))
            assert g == w, "%s: launch %d differs from the fixture" % (case, i)
    assert len(got) == len(want), "%s: %d launches traced, %d in the fixture" % (case, len(got), len(want))


def test_fast_mode_trace_splits_the_libraries():
    """fp32_fast: the encoder's and the attention launches in the third library, everything else in the second"""
    by_variant = {}
    for variant, name, _ in lt.read_fixture("corpbevt_small.fp32_fast"):
        by_variant.setdefault(variant, set()).add(name)
    assert sorted(by_variant) == ["f32h", "f32s"]
    assert {"cobevt_window_attention", "cobevt_stem_conv7x7s2_pool", "cobevt_basicblock_nhwc"} <= by_variant["f32h"]
    assert "cobevt_window_attention" not in by_variant["f32s"] and "cobevt_sttf_warp" in by_variant["f32s"]


def test_conv2d_table_launches_every_conv_entry_point():
    """the routing table reaches all eight kernels of ops.conv2d (the model traces never launch two of them)"""
    assert len(ops.CONV_SYMBOLS) == 8
    assert set(ops.CONV_SYMBOLS.values()) <= {name for _, name, _ in lt.read_fixture("conv2d_table")}


def test_conv_route_agrees_with_the_recorded_table(monkeypatch):
    """ops.conv_route names, for every conv2d / linear row of the table, the entry point the fixture (recorded before conv_route
    existed) shows launched, with the recorded library, LayerNorm placement, strip variant and rows per workgroup - and takes the
    library from its argument alone, whatever lib.get_variant() says meanwhile"""
    import cases_conv as cv
    launched = []
    for record in lt.read_fixture("conv2d_table"):
        if record[1] == "row":
            launched.append([])
        else:
            launched[-1].append(record)
    routes = {}
    for r, records in zip(cv.ROWS, launched):
        plan = cv.plan(r)
        n, h, w = (1, 1, math.prod(r["x"][:-1])) if len(r["w"]) == 2 else r["x"][:3]
        with monkeypatch.context() as m:
            for knob, value in r["knobs"].items():
                m.setattr(ops, knob, value)
            got = set()
            for ambient in lib.VARIANTS:
                m.setattr(lib, "_variant", ambient)
                got.add(ops.conv_route(plan, n, h, w, r["out"], r["res"], r["lib"]))
        assert len(got) == 1, "%s: the route moves with lib.get_variant(): %s" % (r["name"], got)
        route = routes[r["name"]] = got.pop()
        separate_ln = plan.has_ln and not route.ln_fused
        want = ["cobevt_layernorm"] * separate_ln + [ops.CONV_SYMBOLS[route.kernel]]
        assert [name for _, name, _ in records] == want, r["name"]
        assert {variant for variant, _, _ in records} == {r["lib"]}, r["name"]
        dims = next((v for v in records[-1][2] if isinstance(v, list)), None)
        if route.kernel == "strips":
            assert route.variant == dims[11] > 0, r["name"]
        else:
            assert route.variant == 0, r["name"]
        if route.kernel == "rows_small_k":
            assert (route.rows, int(route.ln_fused)) == (dims[13], dims[7]), r["name"]
        elif route.kernel in ("rows", "rows_wfrag"):
            assert int(route.ln_fused) == dims[12], r["name"]
        assert not (route.ln_fused and not plan.has_ln), r["name"]
    # one stride-2 fp32 plan, three libraries, three routes: the library is an input of the decision like any other
    assert [routes["c3_s2.fp32.lib" + v][::2] for v in ("native", "f32s", "f32h")] == [("strips", 131), ("igemm", 0), ("strips", 130)]


# the entry point behind every word of autograd.train_conv_route ("chunked": by kernel size; it asks <symbol>_chunks first)
TRAIN_SYMBOLS = {"rows": "cobevt_linear_rows_small_k", "strips": "cobevt_conv3x3_wfrag_nhwc", "conv3": "cobevt_conv3x3_nhwc",
                 "igemm": "cobevt_conv2d_nhwc", "frags": "cobevt_linear_weight_frags", "pair": "cobevt_conv3_weight_operands2",
                 "weight_rows": "cobevt_conv_weight_rows", "operand": "cobevt_conv3_weight_operands", "blocked": "cobevt_conv_wgrad_blocked",
                 "generic": "cobevt_conv_wgrad", "chunked": {1: "cobevt_linear_wgrad", 3: "cobevt_conv_wgrad3"}}
TRAIN_SWITCHES = ("USE_TRAIN_ROWS_GEMM", "USE_TRAIN_STRIPS", "USE_WGRAD3", "USE_WGRAD_BLOCKED", "USE_WGRAD_BLOCKED_STRIDED")


def _dims(args):
    """the integer vector among a launch's recorded arguments"""
    return next((v for v in args if isinstance(v, list) and v and isinstance(v[0], int)), None)


def _train_table():
    """[(row of cases_conv.TRAIN_ROWS, its launches in the fixture)]"""
    import cases_conv as cv
    launched = []
    for record in lt.read_fixture("train_conv_table"):
        if record[1] == "row":
            launched.append([])
        else:
            launched[-1].append(record)
    assert [r["name"] for r in cv.TRAIN_ROWS] == [rec[2][0] for rec in lt.read_fixture("train_conv_table") if rec[1] == "row"]
    return list(zip(cv.TRAIN_ROWS, launched))


def _train_route(m, r, **switches):
    """autograd.train_conv_route for a row under its own switches and strip pin, then `switches`"""
    import cases_conv as cv
    for knob, value in dict(r["knobs"], **switches).items():
        m.setattr(autograd, knob, value)
    m.setattr(ops, "CONV3_VARIANT", r["variant"])
    return autograd.train_conv_route(ops.dcode(cv.DTYPES[r["dt"]]), *cv.train_conv_args(r))


def test_train_conv_route_agrees_with_the_recorded_table(monkeypatch):
    """autograd.train_conv_route names, for every row of the training table, exactly what the fixture (recorded before the function
    existed) shows launched, in order: the operand preparation, the forward kernel and its strip variant, the input-gradient kernel and
    its variant, the weight-gradient entry point under the row's chunk answers (with the blocked form at dims[9]) - all in the native
    library, whichever one is the ambient one"""
    import cases_conv as cv
    for r, records in _train_table():
        got = set()
        for ambient in lib.VARIANTS:
            with monkeypatch.context() as m:
                m.setattr(lib, "_variant", ambient)
                got.add(_train_route(m, r))
        assert len(got) == 1, "%s: the route moves with lib.get_variant(): %s" % (r["name"], got)
        route = got.pop()
        k, cout = r["k"], cv.train_conv_args(r)[4]
        torch_prep = r["knobs"].get("USE_TORCH_OPERAND_PREP", False)       # the torch-op specifications launch nothing
        want = [(TRAIN_SYMBOLS[route.prep[0]], None), (TRAIN_SYMBOLS[route.fwd], route.var_f)]
        want += [(TRAIN_SYMBOLS[call], None) for call in route.prep[1:]]
        if torch_prep:
            want = [item for item in want if item[0] != TRAIN_SYMBOLS["weight_rows"]]
        if route.dgrad is not None:
            want.append((TRAIN_SYMBOLS[route.dgrad], route.var_d))
        for form in route.wgrad:
            if form == "chunked":
                want.append((TRAIN_SYMBOLS[form][k] + "_chunks", None))
                if r["chunks"].get(want[-1][0], 0) > 0:
                    want.append((TRAIN_SYMBOLS[form][k], None))
                    break
            else:
                want += [("cobevt_wgrad_block_operand", None)] * (0 if (torch_prep or form != "blocked") else 2)
                want.append((TRAIN_SYMBOLS[form], route.wgrad_mode))
        if r["bias"] and r["w_grad"]:
            want += [("cobevt_channel_sums", None)] + [("cobevt_f64_to_f32", None)] * bool(cout % 8)
        assert [name for _, name, _ in records] == [name for name, _ in want], r["name"]
        assert {variant for variant, _, _ in records} == {""}, r["name"]
        for (_, name, args), (_, detail) in zip(records, want):
            dims = _dims(args)
            if name == TRAIN_SYMBOLS["strips"]:
                assert detail == dims[11] > 0, r["name"]
            elif name == TRAIN_SYMBOLS["conv3"]:
                assert detail == 0, r["name"]
            elif name == TRAIN_SYMBOLS["blocked"]:
                assert detail == dims[9] and detail is not None, r["name"]
            elif name == TRAIN_SYMBOLS["generic"]:
                assert detail is None, r["name"]
        if r["linear"]:       # the rows arrive as the H x W map the table states
            maps = [_dims(args)[1:3] for _, name, args in records if name in ("cobevt_wgrad_block_operand", TRAIN_SYMBOLS["generic"])]
            assert maps[0] == list(r["as_conv"][:2]), r["name"]
    # the table reaches every word of the route and every blocked form
    routes = [_train_route(monkeypatch, r) for r, _ in _train_table()]
    words = {w for rt in routes for w in (rt.fwd, rt.dgrad) + rt.prep + rt.wgrad}
    assert words == set(TRAIN_SYMBOLS) | {None} and {rt.wgrad_mode for rt in routes} == {None, 0, 1, 2}


@pytest.mark.parametrize("switch", TRAIN_SWITCHES)
def test_train_conv_route_moves_only_where_a_switch_governs(switch, monkeypatch):
    """planted fault: with ONE switch off (all others at their defaults) the route changes for exactly the rows whose shape the fixture
    shows on that switch's kernels - evidence from the rows recorded under default switches - and for no other row"""
    import cases_conv as cv
    evidence = {"USE_TRAIN_ROWS_GEMM": lambda name, dims: name == TRAIN_SYMBOLS["rows"],
                "USE_TRAIN_STRIPS": lambda name, dims: name in (TRAIN_SYMBOLS["strips"], TRAIN_SYMBOLS["conv3"]),
                "USE_WGRAD3": lambda name, dims: name.endswith("_chunks"),
                "USE_WGRAD_BLOCKED": lambda name, dims: name == TRAIN_SYMBOLS["blocked"],
                "USE_WGRAD_BLOCKED_STRIDED": lambda name, dims: name == TRAIN_SYMBOLS["blocked"] and dims[9] in (1, 2)}[switch]
    key = lambda r: (r["dt"], r["variant"]) + cv.train_conv_args(r)          # noqa: E731  (what the route may depend on besides the switches)
    governed = set()
    for r, records in _train_table():
        if not r["knobs"] and any(evidence(name, _dims(args)) for _, name, args in records):
            governed.add(key(r))
    assert governed, switch
    defaults = {s: getattr(autograd, s) for s in TRAIN_SWITCHES}
    moved = {}
    for r, _ in _train_table():
        plain = dict(r, knobs={})
        with monkeypatch.context() as m:
            before = _train_route(m, plain, **defaults)
            after = _train_route(m, plain, **dict(defaults, **{switch: False}))
        moved.setdefault(key(r), set()).add(before != after)
    assert {k for k, v in moved.items() if v == {True}} == governed and all(len(v) == 1 for v in moved.values()), switch


def test_failing_key_split_launch_names_its_own_symbol(monkeypatch):
    """one 32 x 32 window = 1024 keys on a small grid takes cobevt_window_attention_ksplit: its failure is reported under that name"""
    rec = lt.Recorder(status={"cobevt_window_attention_ksplit": 1})
    lt.install(monkeypatch.setattr, rec)
    B, heads, d = 2, 4, 128
    qmap = ops.tokmap(0, 1, 32, 32, 32, 32)
    q, k, v, out = (torch.zeros(B * 1024, d, dtype=torch.bfloat16) for _ in range(4))
    with pytest.raises(CobevtHipError, match=r"^cobevt_window_attention_ksplit failed: .* \(code 1\)$"):
        ops.window_attention(q, k, v, out, qmap, qmap, qmap, B, heads, 32 ** -0.5, d, d, d, d, ksplit=2)
    assert [r[1] for r in rec.records] == ["cobevt_window_attention_ksplit"]


def test_compute_mode_set_inside_encoder_scope_survives_it():
    with host.compute_dtype("fp32_fast"):
        with lib.encoder_scope():
            assert lib.get_variant() == "f32h"
            host.set_compute_dtype("fp32")
            assert lib.get_variant() == ""
        assert lib.get_variant() == "" and host.get_compute_mode() == "fp32"
    assert lib.get_variant() == "" and host.get_compute_mode() == "bf16"


def test_cobevt_flags_round_trip(monkeypatch):
    knobs = ("CONV3_VARIANT", "BASICBLOCK_TILE_ROWS", "ROW_CHAIN_ROWS", "GEMM_ROWS3_MIN_M", "GEMM_ROWS3_MAX_K", "GEMM_ROWS3_STRIDED",
             "GEMM_ROWS3_ROWS64_MIN_M", "BASICBLOCK_MAX_C", "ATTN_VARIANT", "ATTN_QSPLIT", "ATTN_KSPLIT")
    for k in knobs + ("USE_EMBED_GEMM",):
        monkeypatch.setattr(ops, k, getattr(ops, k))            # restored when the test ends
    monkeypatch.setenv("COBEVT_FLAGS", ",".join("%s=%d" % (k, 7 + i) for i, k in enumerate(knobs)) + ", USE_EMBED_GEMM=1")
    ops._apply_env_flags()
    assert [getattr(ops, k) for k in knobs] == [7 + i for i in range(len(knobs))]
    assert ops.USE_EMBED_GEMM is True
    monkeypatch.setenv("COBEVT_FLAGS", "USE_EMBED_GEMM=0")
    ops._apply_env_flags()
    assert ops.USE_EMBED_GEMM is False
    for bad in ("NO_SUCH_KNOB=1", "BF16=1", "PILLAR_CHANNELS=32"):         # unknown, and module constants that are not switches
        monkeypatch.setenv("COBEVT_FLAGS", bad)
        with pytest.raises(CobevtHipError, match="unknown switch"):
            ops._apply_env_flags()
