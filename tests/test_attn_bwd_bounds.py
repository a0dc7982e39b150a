"""CPU: the float64 interval reference of the window-attention backward kernels (tests/attn_bwd_ref.py) is
neither too tight nor vacuous.

  - the restated index arithmetic (token maps, relative-bias index, key visibility, dropout hash) equals small hand-computed values and
    a scalar transcription of the hash; tests/test_attn_bwd_bounds_gpu.py ties it to the library's hooks;
  - for every (case, path) and every summation order a CPU model of a correct kernel lies inside [lo, hi] for dq, dk, dv and dbias;
  - every bf16 path keeps a useful interval (the width condition of section 3u); the widths of all paths are printed;
  - the same model with one injected fault leaves the interval at >= 1 % of the elements the fault touches on the case the list names
    (a fault a case hides says so by name, with the share it reaches), and truncating P / dZ to bf16 trips the signed bias statistic.
"""
import numpy as np
import pytest
import torch

import attn_bwd_ref as ab

PARAMS = dict(argnames="cp", argvalues=ab.CASE_PATHS, ids=[ab.case_id(cp) for cp in ab.CASE_PATHS])
NAMES = ("dq", "dk", "dv", "dbias")
MIN_SHARE = 0.01


# ----------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------
def test_token_maps_by_hand():
    """token 7 of window 3 of batch 1, two cameras of a 4 x 6 map in 2 x 3 windows: camera 1, (i, j) = (0, 1); window (x, y) = (1, 1)"""
    assert [int(v) for v in ab.tok_coord((0, 2, 4, 6, 2, 3, 2, 2), np.int64(7))] == [1, 0, 1]
    rows = {}
    for mode in (0, 1, 2):
        m = (mode, 2, 4, 6, 2, 3, 2, 2)
        idx = ab.index_map(m, 2)
        assert idx.shape == (2, 4, 12) and sorted(idx.reshape(-1).tolist()) == list(range(96))
        rows[mode] = int(idx[1, 3, 7])
    # mode 0: pixel (1 * 2 + 0, 1 * 3 + 1) = (2, 4), row ((1 * 2 + 1) * 4 + 2) * 6 + 4;  mode 1: pixel (0 * 2 + 1, 1 * 2 + 1) = (1, 3);
    # mode 2: (((1 * 2 + 1) * 4 + 3) * 2 + 0) * 3 + 1
    assert rows == {0: 88, 1: 81, 2: 91}


def test_bias_index_by_hand():
    """((dl + L - 1)(2 w1 - 1) + di + w1 - 1)(2 w2 - 1) + dj + w2 - 1 with the KEY map's window: query (1, 0, 1), key (0, 1, 2) of 2 x 3
    windows, L = 2: dl, di, dj = 1, -1, -1 -> ((1 + 1) 3 + 0) 5 + 1 = 31; the extreme pairs reach 0 and rows - 1"""
    m = (0, 2, 4, 6, 2, 3, 2, 2)
    idx = ab.bias_index(m, m, 2)
    assert idx.shape == (12, 12) and int(idx[7, 5]) == 31
    assert int(idx.min()) == 0 and int(idx.max()) == ab.bias_rows(m, 2) - 1 == 3 * 3 * 5 - 1
    # a cross map: the window extents are the key map's (6 x 6), whatever the query map's (4 x 4)
    c = ab.BY_NAME["cross_48_108"]
    idx = ab.bias_index(c.qmap, c.kmap, 3)
    assert int(idx[0, 0]) == ((0 + 2) * 11 + 5) * 11 + 5 and int(idx[47, 107]) == ((2 + 2) * 11 + 3 + 5) * 11 + 3 + 5 - ((2 * 11 + 5) * 11 + 5)


def test_key_visible_layouts_by_hand():
    """modes 0 / 1 read (B, HH, WW, ncam) at the token's pixel, mode 2 reads (B, L, w1, w2, ncam) at the token's place in its window"""
    for mode in (0, 1, 2):
        m = (mode, 2, 4, 6, 2, 3, 2, 2)
        mask = np.ones((2, 4, 2, 3, 2) if mode == 2 else (2, 4, 6, 2), dtype=np.float32)
        if mode == 2:
            mask[1, 3, 0, 1, 1] = 0
        else:
            mask[(1,) + {0: (2, 4), 1: (1, 3)}[mode] + (1,)] = 0
        vis = ab.key_visible(mask, m, 2)
        assert vis.shape == (2, 4, 12) and int((~vis).sum()) == 1 and not vis[1, 3, 7]


def _mix_scalar(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def test_dropout_hash_by_hand():
    """the murmur3 finaliser's known values, and attn_keep against a scalar transcription of csrc/attn_common.hpp"""
    assert [int(v) for v in ab.mix32(np.array([0, 1], dtype=np.uint64))] == [0, 0x514E28B7]
    B, L, H, nq, nk, p, seed = 2, 3, 2, 5, 7, 0.3, 0xFFFFFFF0 + 0x31
    keep = ab.attn_keep(B, L, H, nq, nk, p, seed)
    assert keep.shape == (B, L, H, nq, nk) and 0.55 < keep.mean() < 0.85
    for b, l, h, tq, tk in ((0, 0, 0, 0, 0), (1, 2, 1, 4, 6), (1, 0, 1, 3, 2), (0, 2, 0, 1, 5)):
        row = ((b * L + l) * H + h) * nq + tq
        hrow = _mix_scalar((row & 0xFFFFFFFF) ^ _mix_scalar((row >> 32) ^ (seed & 0xFFFFFFFF)))
        u = _mix_scalar(hrow ^ ((tk * 0x9E3779B1) & 0xFFFFFFFF))
        assert bool(keep[b, l, h, tq, tk]) == bool(np.float32(u) * np.float32(2.0 ** -32) >= np.float32(p))


def test_case_table_conditions():
    """the operand conditions the builder asserts hold for both storage types, and the tile counts are the ones the rows are there for"""
    for c in ab.CASES:
        for store in sorted({ab.store_of(ab.PATHS[p][1]) for p in c.paths}, key=str):
            op = ab.operands(c, store)
            print("%s %s: logit std %.2f, Nq %d, Nk %d, L %d" % (c.name, store, op["logit_std"], c.Nq, c.Nk, c.L))
    n = ab.BY_NAME
    assert (n["one_tile_25"].Nq, n["ragged_90"].Nk, n["grid_245"].Nq, n["cross_48_108"].Nq, n["cross_48_108"].Nk) == (25, 90, 245, 48, 108)
    assert n["many_windows"].L == 2304 and n["many_windows"].bias_rows == 49 and n["dropout_64_128"].Nk == 128


# ----------------------------------------------------------------------------------------------
# the emulator and the width
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**PARAMS)
def test_honest_model_is_inside(cp):
    case, path = cp
    ref = ab.reference(case, path)
    for order in ab.ORDERS:
        got = ab.emulate(case, path, order)
        for name in NAMES:
            iv = ref[name]
            if iv is None:
                assert got[name] is None
                continue
            assert got[name].shape == iv.ref.shape and bool((iv.lo <= iv.hi).all()) and bool(torch.isfinite(iv.lo).all() & torch.isfinite(iv.hi).all())
            out = ab.outside(got[name], iv)
            print("%s %s %s %s: position in the interval %.3f" % (case.name, path, order, name, ab.position(got[name], iv)))
            assert out == 0, "%s %s: %d of %d elements of a correct kernel outside" % (order, name, out, got[name].numel())


@pytest.mark.parametrize(**PARAMS)
def test_interval_width(cp):
    """median of (hi - lo) / |ref| and the share wider than 2^-5 |ref| + 2^-8 max|ref|; asserted (<= 2^-6, <= 5 %) on the bf16 paths, for
    all four destinations (many_windows meets it for dbias through its operands: attn_bwd_ref._coherent_dp)"""
    case, path = cp
    ref = ab.reference(case, path)
    for name in NAMES:
        if ref[name] is None:
            continue
        med, share = ab.width_stats(ref[name])
        print("%s %s %s: median width %.3e of |ref|, %.4f of the elements wide" % (case.name, path, name, med, share))
        if path != "fp32":
            assert med <= ab.WIDTH_MEDIAN and share <= ab.WIDTH_SHARE, (name, med, share)


# ----------------------------------------------------------------------------------------------
# the faults
# ----------------------------------------------------------------------------------------------
# (letter of the list in section 3z, fault, case, path).  "elements it touches" = those a faulty model stores differently from the
# correct model in the same summation order.
FAULT_ROWS = [("a", "drop_last_q_tile", "ragged_90", "fp32"), ("b", "pad_keys_visible", "one_tile_25", "fp32"),
              ("b+", "pad_keys_visible", "ragged_90", "fp32"), ("c", "mask_cam_ignored", "grid_245", "fp32"),
              ("d", "bias_qmap_window", "cross_48_108", "fp32"), ("e", "dlse_sign", "cross_48_108", "fp32"),
              ("f", "lse_natural", "one_tile_25", "fp32"), ("g", "dv_without_keep", "dropout_64", "fp32"),
              ("h", "dk_no_scale", "ragged_90", "fp32"), ("j", "dbias_second_window", "many_windows", "fp32"),
              ("j+", "dbias_second_window", "many_windows", "bf16st"), ("k", "dscr_next_head", "ragged_90", "bf16st_scr"),
              ("l", "mask_mode0_index", "stored_partition", "fp32")]
# (b) on one_tile_25 is INVISIBLE, share 0 of 0 touched: a pad key has K = V = 0, so its dZ = -P D multiplies a zero K row in dQ, its own
# dK / dV rows are never stored, and the case has no bias table to collect it.  Row b+ shows the same fault on ragged_90 (Nk = 90, six pad
# keys, a table): it lands in dbias at the rows of (query, token 0).
HIDDEN = {"b"}


def _fault_shares(fault, case, path):
    ref, good, bad = ab.reference(case, path), ab.emulate(case, path), ab.emulate(case, path, fault=fault)
    touched = outside = 0
    per = {}
    for name in NAMES:
        if ref[name] is None:
            continue
        t = bad[name] != good[name]
        o = t & ((bad[name] < ref[name].lo) | (bad[name] > ref[name].hi))
        per[name] = (int(o.sum()), int(t.sum()))
        touched, outside = touched + int(t.sum()), outside + int(o.sum())
    return touched, outside, per


@pytest.mark.parametrize("letter,fault,name,path", FAULT_ROWS, ids=["%s-%s-%s-%s" % r for r in FAULT_ROWS])
def test_fault_leaves_the_interval(letter, fault, name, path):
    touched, outside, per = _fault_shares(fault, ab.BY_NAME[name], path)
    print("fault (%s) %s on %s %s: %d of %d touched elements outside  %s" % (letter, fault, name, path, outside, touched, per))
    if letter in HIDDEN:
        assert touched == 0 and outside == 0, "no longer hidden: move the row out of HIDDEN"
        return
    assert touched > 0 and outside >= MIN_SHARE * touched
    for o, t in per.values():                                             # ... and in every destination the fault reaches
        assert t == 0 or o >= MIN_SHARE * t, per


@pytest.mark.parametrize("name,path", [("ragged_90", "bf16mm"), ("grid_245", "bf16st_scr")])
def test_truncated_pack_trips_the_bias_statistic(name, path):
    """fault (i): P and dZ truncated instead of rounded to bf16 before the row-contracting products.  Truncation pulls every term of
    dV, dK and dQ towards zero, whatever its sign, so each result shrinks by about 2^-9 ln 2 ... 2^-8 of itself: the signed statistic of
    conv_bounds_ref.bias_stat (limit 2^-11, destinations of >= 2000 elements) on all three, fp32 store and bf16 store"""
    case = ab.BY_NAME[name]
    ref = ab.reference(case, path)
    good, bad = ab.emulate(case, path), ab.emulate(case, path, fault="trunc_bf16")
    for label, got in (("correct", good), ("truncated", bad)):
        for dest in ("dq", "dk", "dv"):
            mean, n = ab.bias_stat(got[dest], ref[dest].ref)
            print("%s %s %s %s: signed bias %.3e over %d elements (limit %.3e)" % (name, path, label, dest, mean, n, ab.BIAS_LIMIT))
            assert n >= ab.BIAS_MIN_N
            if label == "correct":
                assert abs(mean) <= ab.BIAS_LIMIT
    assert all(ab.bias_stat(bad[d], ref[d].ref)[0] < -ab.BIAS_LIMIT for d in ("dq", "dk", "dv"))
