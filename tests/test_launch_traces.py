"""CPU: the launch sequence of every model (tests/launch_trace.py) against the fixtures under tests/golden/launch_traces/, and the
call path / library selection / COBEVT_FLAGS behaviour the routing code rests on.  No GPU and no built library: lib.load is a fake."""
import json

import pytest
import torch

import launch_trace as lt
from cobevt_amd import host, lib, ops
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
