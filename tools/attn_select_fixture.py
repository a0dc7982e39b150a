"""The fixtures of tests/test_attn_select.py: tests/golden/attn_select/cases.txt and expected.jsonl.

    python tools/attn_select_fixture.py cases                 rewrite cases.txt: the table below + every distinct attention record
                                                              of the launch-trace fixtures
    python tools/attn_select_fixture.py record --rev COMMIT   rewrite expected.jsonl from what COMMIT's entry point launches

`record` never runs csrc/attn_select.hpp: it takes attention.hip / attention_resident.hip and their headers from COMMIT (git show),
compiles them for the host with attn_select_shim.hpp force-included and attn_select_oracle.cpp as main, and runs that program once
per gate setting (default, COBEVT_ATTN_BIG=0, COBEVT_ATTN_PERSIST=0).  It needs no GPU: without one the device query fails and the
entry point assumes 256 compute units, so every case is recorded at cus = 256.
"""
import argparse
import glob
import gzip
import json
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import select_fixture as sf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_select")
CASES = os.path.join(GOLDEN, "cases.txt")
EXPECTED = os.path.join(GOLDEN, "expected.jsonl")
TRACES = os.path.join(ROOT, "tests", "golden", "launch_traces")
FORWARD = ("cobevt_window_attention", "cobevt_window_attention_ksplit", "cobevt_window_attention_lse")


def tmap(ncam, w1, w2, X=8, Y=8, mode=0):
    return [mode, ncam, X * w1, Y * w2, w1, w2, X, Y]


def case(name, k, q=None, o=None, B=1, heads=4, L=None, dtype=0, variant=0, qsplit=0, bias=0, bias_rows=None, bias_L=None, mask=0, lse=0,
         mean_q=0, drop_p=0.0, ksplit=1, parts=None, part_rows=None, big=1, persist=1, ld=None, off=(0, 0, 0, 0), bias_mode=None):
    """One line of cases.txt.  k / q / o: token maps (q, o default to k, o to q); bias: a table is passed, with the row count the
    resident kernel expects unless bias_rows says otherwise."""
    q = k if q is None else q
    o = q if o is None else o
    ld = [heads * 32] * 4 if ld is None else ld
    bias_L = k[1] if bias_L is None else bias_L
    if bias_rows is None:
        bias_rows = (2 * bias_L - 1) * (2 * k[4] - 1) * (2 * k[5] - 1) if bias else 0
    dims = [dtype | variant << 8 | qsplit << 16, B, q[6] * q[7] if L is None else L, heads] + list(ld) + list(off) + \
        [bias if bias_mode is None else bias_mode, bias_rows, bias_L, mean_q] + q + k + o
    parts = int(ksplit > 1) if parts is None else parts
    part_rows = (B * o[1] * o[2] * o[3] if ksplit > 1 else 0) if part_rows is None else part_rows
    return " ".join([name] + [str(d) for d in dims] + [str(v) for v in (bias, mask, lse, repr(float(drop_p)), ksplit, parts, part_rows, big, persist, 256)])


def table():
    c = []
    # ---- resident eligibility by key count (self attention, 64 windows x 4 heads), plain and with the big gate off
    for nk, (n, w1, w2) in [(64, (1, 8, 8)), (65, (1, 5, 13)), (128, (2, 8, 8)), (192, (3, 8, 8)), (320, (5, 8, 8)), (512, (8, 8, 8)),
                            (513, (3, 9, 19)), (576, (1, 24, 24)), (768, (3, 16, 16)), (1000, (1, 25, 40)), (1024, (1, 32, 32)),
                            (1025, (1, 25, 41))]:
        assert n * w1 * w2 == nk
        c.append(case("keys%d" % nk, tmap(n, w1, w2)))
        c.append(case("keys%d.big0" % nk, tmap(n, w1, w2), big=0))
    # ---- resident variants
    k320 = tmap(5, 4, 16)
    c.append(case("bias320", k320, bias=1))
    c.append(case("mask320", k320, mask=1))
    c.append(case("biasmask320", k320, bias=1, mask=1))
    for n in (2, 8):
        c.append(case("w8.bias%d" % (n * 64), tmap(n, 8, 8), bias=1))
        c.append(case("w8.biasmask%d" % (n * 64), tmap(n, 8, 8), bias=1, mask=1))
    c.append(case("bias.w2mod4", tmap(5, 8, 6), bias=1))
    c.append(case("bias.rows_wrong", k320, bias=1, bias_rows=1952))
    c.append(case("mean256", tmap(4, 8, 8), q=tmap(4, 8, 8), o=tmap(1, 8, 8), mean_q=1))
    c.append(case("mean192.ragged", tmap(3, 8, 8), q=tmap(4, 8, 8), o=tmap(1, 8, 8), mean_q=1))
    c.append(case("mean.bias", tmap(4, 8, 8), q=tmap(4, 8, 8), o=tmap(1, 8, 8), mean_q=1, bias=1))
    c.append(case("mean.mask", tmap(4, 8, 8), q=tmap(4, 8, 8), o=tmap(1, 8, 8), mean_q=1, mask=1))
    c.append(case("big576.bias", tmap(1, 24, 24), bias=1))
    c.append(case("big576.mask", tmap(1, 24, 24), mask=1))
    c.append(case("big576.mean", tmap(2, 18, 16), o=tmap(1, 18, 16), mean_q=1))
    c.append(case("ocam_differs", tmap(2, 8, 8), o=tmap(1, 8, 8)))
    c.append(case("mean.ocam2", tmap(2, 8, 8), mean_q=1))
    # ---- waves and persistence (512-key 8 x 8 x 8 windows, bias + mask: 134 KB of LDS)
    k512 = tmap(8, 8, 8)
    c.append(case("waves8.q512", k512, bias=1, mask=1))
    c.append(case("waves4.q480", k512, q=tmap(1, 20, 24), bias=1, mask=1))
    k256 = tmap(4, 8, 8)
    c.append(case("lds40k.at", k256, q=tmap(1, 28, 32)))                # 33792 + 896 * 8 = 40960: not above
    c.append(case("lds40k.above", k256, q=tmap(1, 29, 31)))             # 899 queries
    c.append(case("lds80k.at", k512, q=tmap(1, 32, 56)))                # 67584 + 1792 * 8 = 81920: not above
    c.append(case("lds80k.above", k512, q=tmap(1, 26, 69)))             # 1794 queries
    c.append(case("lds80k.above.L128", tmap(8, 8, 8, 8, 16), q=tmap(1, 26, 69, 8, 16)))
    for name, X, Y, heads in [("persist.L128", 8, 16, 4), ("persist.L120", 8, 15, 4), ("persist.L129", 3, 43, 4), ("persist.L127", 1, 127, 4),
                              ("persist.h3.L160", 8, 20, 3), ("persist.h3.L152", 8, 19, 3), ("persist.h3.L171", 9, 19, 3),
                              ("persist.h3.L170", 10, 17, 3)]:
        c.append(case(name, tmap(8, 8, 8, X, Y), heads=heads, bias=1, mask=1))
    c.append(case("persist.gate0", tmap(8, 8, 8, 8, 16), bias=1, mask=1, persist=0))
    # ---- query split
    k128, q64 = tmap(2, 8, 8), tmap(1, 8, 8)
    c.append(case("items255.q64", tmap(2, 8, 8, 15, 17), q=tmap(1, 8, 8, 15, 17), heads=1))
    c.append(case("items256.q64", tmap(2, 8, 8, 16, 16), q=tmap(1, 8, 8, 16, 16), heads=1))
    c.append(case("items255.q128", tmap(2, 8, 8, 15, 17), heads=1))
    c.append(case("items4.big1024", tmap(1, 32, 32, 1, 1)))
    c.append(case("items4.keys512", tmap(8, 8, 8, 1, 1)))
    c.append(case("info_split.bias", tmap(5, 4, 16, 4, 4), bias=1))
    c.append(case("info_split.mask", tmap(5, 4, 16, 4, 4), mask=1))
    c.append(case("info_split.plain", tmap(5, 4, 16, 4, 4)))
    for hint in (1, 2, 4, 9):
        c.append(case("hint%d" % hint, k128, qsplit=hint))
    c.append(case("hint2.items4", tmap(2, 8, 8, 1, 1), qsplit=2))
    c.append(case("grid_y65535", tmap(1, 8, 16, 1, 1), B=65535))
    c.append(case("grid_y65536", tmap(1, 8, 16, 1, 1), B=65536))
    # ---- streaming
    c.append(case("stream.variant1", tmap(5, 8, 8), variant=1))
    c.append(case("stream.variant2", tmap(5, 8, 8), variant=2))
    c.append(case("wide.keys255", tmap(1, 15, 17), variant=1))
    c.append(case("wide.keys256", tmap(1, 16, 16), variant=1))
    c.append(case("wide.grid1024", tmap(1, 16, 16), q=tmap(1, 16, 32), variant=1))
    c.append(case("wide.grid1025", tmap(1, 16, 16, 1, 41), q=tmap(1, 24, 24, 1, 41), heads=5, variant=1))
    c.append(case("fp32", tmap(5, 8, 8), dtype=1))
    c.append(case("fp32.biasmask", k320, dtype=1, bias=1, mask=1))
    for n in (3, 4, 6, 8, 9):
        c.append(case("stream.mean%d" % n, tmap(n, 8, 8), o=tmap(1, 8, 8), mean_q=1, variant=1))
    c.append(case("paired", tmap(4, 16, 16, 1, 1), o=tmap(1, 16, 16, 1, 1), mean_q=2))
    c.append(case("paired.ksplit4", tmap(4, 16, 16, 1, 1), o=tmap(1, 16, 16, 1, 1), mean_q=2, ksplit=4))
    c.append(case("paired.bias", tmap(4, 16, 16, 1, 1), o=tmap(1, 16, 16, 1, 1), mean_q=2, bias=1))
    c.append(case("paired.kcam", tmap(3, 16, 16, 1, 1), q=tmap(4, 16, 16, 1, 1), o=tmap(1, 16, 16, 1, 1), mean_q=2))
    c.append(case("klinear.on", tmap(1, 32, 32, 1, 1), variant=1))
    c.append(case("klinear.off.bias", tmap(1, 32, 32, 1, 1), variant=1, bias=1))
    c.append(case("klinear.off.mode2", tmap(1, 32, 32, 1, 1, mode=2), variant=1))
    c.append(case("lds64k.below", tmap(1, 60, 60, 1, 1), dtype=1, mask=1))       # 36352 + 3600 * 8 = 65152
    c.append(case("lds64k.above", tmap(1, 60, 61, 1, 1), dtype=1, mask=1))       # 36352 + 3660 * 8 = 65632
    c.append(case("rows2g", tmap(1, 128, 128, 2, 2), B=32768, variant=1))        # 2^31 rows: the key table is 32-bit
    k4096 = tmap(1, 64, 64, 1, 1)
    for ks in (2, 16, 17):
        c.append(case("ksplit%d" % ks, k4096, q=tmap(1, 32, 32, 1, 1), ksplit=ks))
    c.append(case("ksplit2.keys1024", tmap(1, 32, 32, 1, 1), ksplit=2))
    c.append(case("ksplit16.tiles8", tmap(1, 32, 32, 1, 1), ksplit=16))
    c.append(case("ksplit2.fp32", tmap(1, 32, 32, 1, 1), ksplit=2, dtype=1))
    c.append(case("ksplit2.no_parts", tmap(1, 32, 32, 1, 1), ksplit=2, parts=0))
    c.append(case("ksplit2.rows0", tmap(1, 32, 32, 1, 1), ksplit=2, part_rows=0))
    c.append(case("ksplit2.lse", tmap(1, 32, 32, 1, 1), ksplit=2, lse=1, dtype=1))
    c.append(case("ksplit2.mean", tmap(2, 16, 16, 1, 1), o=tmap(1, 16, 16, 1, 1), mean_q=1, ksplit=2))
    c.append(case("ksplit2.ocam", tmap(2, 32, 16, 1, 1), o=tmap(1, 32, 16, 1, 1), ksplit=2))
    c.append(case("lse", tmap(5, 8, 8), dtype=1, lse=1))
    c.append(case("lse.bf16", tmap(5, 8, 8), lse=1))
    c.append(case("lse.mean", tmap(4, 8, 8), o=tmap(1, 8, 8), dtype=1, lse=1, mean_q=1))
    for name, b, m in [("plain", 0, 0), ("bias", 1, 0), ("mask", 0, 1), ("biasmask", 1, 1)]:
        c.append(case("drop." + name, k320, dtype=1, lse=1, drop_p=0.1, bias=b, mask=m))
    c.append(case("drop.bf16", k320, lse=1, drop_p=0.1))
    c.append(case("drop.no_lse", k320, dtype=1, drop_p=0.1))
    c.append(case("drop.p1", k320, dtype=1, lse=1, drop_p=1.0))
    c.append(case("drop.negative", k320, dtype=1, lse=1, drop_p=-0.5))
    # ---- argument errors
    c.append(case("dtype2", k320, dtype=2))
    c.append(case("ld.bf16", k320, ld=[128, 132, 128, 128]))
    c.append(case("off.bf16", k320, off=(0, 0, 4, 0)))
    c.append(case("ld.fp32", k320, dtype=1, ld=[128, 128, 128, 130]))
    c.append(case("off.fp32", k320, dtype=1, off=(2, 0, 0, 0)))
    c.append(case("off.fp32.ok", k320, dtype=1, off=(4, 0, 0, 4)))
    bad = {"mode3": (0, 3), "ncam0": (1, 0), "w1_0": (4, 0), "w2_0": (5, 0), "X0": (6, 0), "Y0": (7, 0), "HH": (2, 33), "WW": (3, 127),
           "w1_256": (4, 256), "ncam32768": (1, 32768)}
    for name, (i, v) in sorted(bad.items()):
        m = list(k320)
        m[i] = v
        if name == "w1_256":
            m[2] = 8 * 256
        c.append(case("map." + name, m, q=k320, L=64))
    c.append(case("map.q", k320, q=[3] + k320[1:], L=64))
    c.append(case("map.o", k320, o=[3] + k320[1:]))
    c.append(case("map.mode2.HH", [2, 5, 1, 1, 4, 16, 8, 8]))           # stored-partitioned rows: HH / WW are not checked
    c.append(case("L.dims", k320, L=63))
    c.append(case("L.kmap", tmap(5, 4, 16, 8, 4), q=k320))
    c.append(case("B0", k320, B=0))
    c.append(case("heads0", k320, heads=0, ld=[128] * 4))
    c.append(case("bias.no_table", k320, bias=0, bias_mode=1, bias_rows=1953))
    c.append(case("bias.rows0", k320, bias=1, bias_rows=0))
    c.append(case("bias.L0", k320, bias=1, bias_L=0, bias_rows=1953))
    c.append(case("mean3", tmap(4, 8, 8), o=tmap(1, 8, 8), mean_q=3))
    c.append(case("mean.negative", tmap(4, 8, 8), o=tmap(1, 8, 8), mean_q=-1))
    c.append(case("mean.one_camera", tmap(5, 8, 8), q=tmap(1, 8, 8), mean_q=1))
    return c


def trace_cases():
    """Every distinct forward attention record of the launch-trace fixtures (full dims, null-ness of bias / mask / lse, dropout,
    key split) as a case line, named trace<NN> in sorted order."""
    seen = set()
    for path in sorted(glob.glob(os.path.join(TRACES, "*.jsonl.gz"))):
        with gzip.open(path, "rt") as f:
            for line in f:
                _, sym, args = json.loads(line)
                if sym not in FORWARD:
                    continue
                has = lambda a: int(a == "ptr")
                if sym == "cobevt_window_attention":
                    bias, mask, dims = has(args[4]), has(args[5]), args[6]
                    rest = (bias, mask, 0, 0.0, 1, 0, 0)
                elif sym == "cobevt_window_attention_ksplit":
                    bias, mask, dims = has(args[4]), has(args[5]), args[8]
                    rest = (bias, mask, 0, 0.0, args[10], int(has(args[6]) and has(args[7])), args[11])
                else:
                    bias, mask, dims = has(args[5]), has(args[6]), args[7]
                    rest = (bias, mask, has(args[4]), args[9], 1, 0, 0)
                seen.add((tuple(dims), rest))
    lines = []
    for i, (dims, rest) in enumerate(sorted(seen)):
        bias, mask, lse, drop_p, ksplit, parts, part_rows = rest
        lines.append(" ".join(["trace%02d" % i] + [str(d) for d in dims] +
                              [str(v) for v in (bias, mask, lse, repr(float(drop_p)), ksplit, parts, part_rows, 1, 1, 256)]))
    return lines


def write_cases():
    lines = table() + trace_cases()
    names = [ln.split()[0] for ln in lines]
    assert len(set(names)) == len(names) and all(len(ln.split()) == 51 for ln in lines)
    os.makedirs(GOLDEN, exist_ok=True)
    with open(CASES, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d cases (%d from the launch traces) -> %s" % (len(lines), len(trace_cases()), CASES))


_RES = re.compile(r"attn_resident_kernel<(\d+), (\d+), (\w+), (\w+), (\w+), (\w+), (\w+), (\w+)>")
_STREAM = re.compile(r"attn_gather_kernel<(cobevt::bf16_t|float), (\w+), (\w+), (\d+), (\w+)>")
_MERGE = re.compile(r"attn_ksplit_merge_kernel<(cobevt::bf16_t|float)>")


def to_json(name, launches, rc):
    """One expected.jsonl line in the exact text tests/attn_select_main.cpp prints."""
    if not launches:
        assert rc != 0
        return '{"name": "%s", "status": %d}' % (name, rc)
    assert rc == 0 and len(launches) <= 2
    sym, nums = launches[0]
    gx, gy, gz, block, lds, qsplit = nums
    f = dict(NT=0, NW=0, MEAN="false", BIAS="false", MASK="false", RAGGED="false", W8="false", PERSIST="false", dtype=0, KT=0)
    merge = 0
    m = _RES.search(sym)
    if m:
        f.update(NT=int(m.group(1)), NW=int(m.group(2)), MEAN=m.group(3), BIAS=m.group(4), MASK=m.group(5), RAGGED=m.group(6), W8=m.group(7),
                 PERSIST=m.group(8))
        family = "RESIDENT_BIG" if f["NT"] > 8 else "RESIDENT"
        assert len(launches) == 1
    else:
        m = _STREAM.search(sym)
        f.update(dtype=int(m.group(1) == "float"), BIAS=m.group(2), MASK=m.group(3), KT=int(m.group(4)))
        family = "STREAM_DROP" if m.group(5) == "true" else "STREAM"
        if len(launches) == 2:
            mm = _MERGE.search(launches[1][0])
            assert int(mm.group(1) == "float") == f["dtype"] and launches[1][1][1:] == [1, 1, 256, 0, 0]
            merge = launches[1][1][0]
    return ('{"name": "%s", "status": 0, "family": "%s", "NT": %d, "NW": %d, "MEAN": %s, "BIAS": %s, "MASK": %s, "RAGGED": %s, "W8": %s, '
            '"PERSIST": %s, "dtype": %d, "KT": %d, "grid": [%d, %d, %d], "block": %d, "lds": %d, "qsplit": %d, "merge_grid": %d}'
            % (name, family, f["NT"], f["NW"], f["MEAN"], f["BIAS"], f["MASK"], f["RAGGED"], f["W8"], f["PERSIST"], f["dtype"], f["KT"],
               gx, gy, gz, block, lds, qsplit, merge))


def parse_oracle(text):
    out, name, launches = {}, None, []
    for line in text.splitlines():
        kind, _, rest = line.partition(" ")
        if kind == "case":
            name, launches = rest, []
        elif kind == "launch":
            sym, _, nums = rest.rpartition(" | ")
            launches.append((sym, [int(v) for v in nums.split()]))
        elif kind == "rc":
            out[name] = to_json(name, launches, int(rest))
    return out


def record(rev):
    with tempfile.TemporaryDirectory() as tmp:
        sf.checkout(rev, tmp)
        exe = sf.build_oracle(tmp, [os.path.join(ROOT, "tools", "attn_select_oracle.cpp")])
        cases = open(CASES).read()
        runs = {}
        for gates, env in [((1, 1), {}), ((0, 1), {"COBEVT_ATTN_BIG": "0"}), ((1, 0), {"COBEVT_ATTN_PERSIST": "0"})]:
            runs[gates] = parse_oracle(sf.run_twice(exe, cases, "COBEVT_ATTN_", env))
    lines = []
    for ln in cases.splitlines():
        tok = ln.split()
        assert tok[-1] == "256", "recorded without a GPU: cus = 256 only"
        lines.append(runs[(int(tok[-3]), int(tok[-2]))][tok[0]])
    with open(EXPECTED, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d records from %s -> %s" % (len(lines), rev, EXPECTED))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("what", choices=("cases", "record"))
    ap.add_argument("--rev", help="record: the commit whose attention entry point is the reference")
    a = ap.parse_args()
    if a.what == "cases":
        write_cases()
    elif not a.rev:
        ap.error("record needs --rev")
    else:
        record(a.rev)
