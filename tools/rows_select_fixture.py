"""The fixtures of tests/test_rows_select.py: tests/golden/rows_select/cases.txt and expected.jsonl.

    python tools/rows_select_fixture.py cases                 rewrite cases.txt: the table below + every distinct record of the five
                                                              row-local entry points in the launch-trace fixtures
    python tools/rows_select_fixture.py record --rev COMMIT   rewrite expected.jsonl from what COMMIT's entry points launch
                                                              (--rev WORKTREE: the files on disk; --out FILE: write elsewhere)

`record` never runs csrc/rows_select.hpp on its own: it takes the eight kernel files behind cobevt_attn_mlp_chain, cobevt_proj_chain
and cobevt_{,bev_embed_,mean_}linear_rows_small_k and their headers from COMMIT (git show), compiles them for the host with
attn_select_shim.hpp force-included and rows_select_oracle.cpp as main, and runs that program once per gate setting (GATES).
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

ROOT = sf.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "rows_select")
CASES = os.path.join(GOLDEN, "cases.txt")
EXPECTED = os.path.join(GOLDEN, "expected.jsonl")
TRACES = os.path.join(ROOT, "tests", "golden", "launch_traces")
UNITS = ["row_chain.hip", "row_chain64.hip", "row_chain_f32.hip", "proj_chain128.hip", "gemm_rows3.hip", "gemm_rows3_f32.hip",
         "ln_linear64.hip", "bev_query.hip"]
DEFAULT = (1, 1, 1536)      # rc64_prefetch, ln_linear64, ln64_blocks
GATES = [(DEFAULT, {}), ((0, 1, 1536), {"COBEVT_RC64_PREFETCH": "0"}), ((2, 1, 1536), {"COBEVT_RC64_PREFETCH": "2"}),
         ((1, 0, 1536), {"COBEVT_LN_LINEAR64": "0"}), ((1, 1, 512), {"COBEVT_LN64_BLOCKS": "512"})]


def line(name, entry, dims, flags, gates=DEFAULT):
    return " ".join([name, entry, str(len(dims))] + [str(d) for d in dims] + [str(len(flags))] + [str(int(f)) for f in flags] + [str(g) for g in gates])


def chain(name, M=1000, C=128, Hd=256, Hdp=None, Nn=0, next_ln=1, next_act=0, rows=0, skip_rows=0, dtype=0, req=1, skip=1, post=(0, 0),
          nxt=None, gates=DEFAULT):
    Hdp = (128 if Hd <= 128 else 256) if Hdp is None else Hdp
    nxt = ((1, 1) if Nn else (0, 0)) if nxt is None else nxt
    return line("chain." + name, "chain", [dtype, M, C, Hd, Hdp, Nn, next_ln, next_act, rows, skip_rows], [req, skip, post[0], post[1], nxt[0], nxt[1]], gates)


def c64(name, M=16384, **kw):
    return chain("c64." + name, M=M, C=64, Hd=128, **kw)


def proj(name, M=1000, C=128, Nn=256, next_ln=1, next_act=0, skip_rows=0, pre_relu=1, variant=0, dtype=0, req=1, pre=(1, 1), skip=1):
    return line("proj." + name, "proj", [dtype, M, C, Nn, next_ln, next_act, skip_rows, pre_relu, variant], [req, pre[0], pre[1], skip])


def small_k(name, M=1000, N=128, K=128, lda=None, pre_relu=0, act=0, ln=0, in_stride=1, src=(1, 1), inn=(1, 1), rows=0, dtype=0, req=1, res=0,
            pre=(0, 0), gates=DEFAULT):
    lda = K if lda is None else lda
    return line("small_k." + name, "small_k", [dtype, M, N, K, lda, pre_relu, act, ln, in_stride, src[0], src[1], inn[0], inn[1], rows],
                [req, res, pre[0], pre[1]], gates)


def ln64(name, M=65536, N=192, **kw):
    return small_k("ln64." + name, M=M, N=N, K=64, ln=1, **kw)


def bev(name, B=1, n=4, hw=64, D=128, N=128, ln=1, xb=0, dtype=0, req=1):
    return line("bev." + name, "bev", [dtype, B, n, hw, D, N, ln, xb], [req])


def mean(name, B=2, L=3, R=256, K=64, N=64, ln=1, act=0, dtype=0, req=1):
    return line("mean." + name, "mean", [dtype, B, L, R, K, N, ln, act], [req])


def table():
    c = []
    # ---- row chain, bf16: the generic kernel's eight forms, pinned by the rows hint
    for rows in (32, 64):
        for Hd in (128, 256):
            for C in (64, 128):
                c.append(chain("generic.rows%d.hd%d.c%d" % (rows, Hd, C), rows=rows, Hd=Hd, C=C))
    for hint in (0, 16, 32, 64):
        c.append(chain("hint%d" % hint, rows=hint))
    c.append(chain("hd128.at", Hd=128))
    c.append(chain("hd136", Hd=136))
    c.append(chain("c120", C=120))
    # ---- the 64-channel persistent form: map size, skip, next projection width, hidden padding, hint, prefetch gate, grid cap
    c.append(c64("m16383", M=16383))
    c.append(c64("m16384"))
    c.append(c64("skip_null", skip=0))
    c.append(c64("skip_bcast", skip_rows=8192))
    c.append(c64("skip_full_explicit", skip_rows=16384))
    for Nn in (32, 64, 96, 128, 160, 192, 224):
        c.append(c64("nn%d" % Nn, Nn=Nn))
    c.append(c64("nn64.no_next", Nn=64, nxt=(0, 0)))
    c.append(c64("hdp256", Hdp=256))
    c.append(chain("c64.hd64", M=16384, C=64, Hd=64))
    c.append(chain("c64.hd120", M=16384, C=64, Hd=120))
    c.append(chain("c56.hd128", M=16384, C=56, Hd=128))
    for hint in (16, 32, 64):
        c.append(c64("hint%d" % hint, rows=hint))
    for pf in (0, 2):
        for Nn in (0, 64, 128, 192):
            c.append(c64("pf%d.nn%d" % (pf, Nn), Nn=Nn, gates=(pf, 1, 1536)))
    for M in (65408, 65536, 65537):                  # four waves: 511, 512, 513 -> 512 workgroups
        c.append(c64("cap.m%d" % M, M=M))
    for M in (98112, 98304, 98305):                  # six waves: 511, 512, 513 -> 512
        c.append(c64("cap.pf0.m%d" % M, M=M, gates=(0, 1, 1536)))
    # ---- argument checks
    for C in (7, 8, 12, 128, 136):
        c.append(chain("c%d" % C, C=C))
    for Hd in (4, 8, 12, 256, 264):
        c.append(chain("hd%d" % Hd, Hd=Hd, Hdp=256 if Hd > 128 else 128))
    c.append(chain("hdp0", Hd=128, Hdp=0))
    c.append(chain("hdp128.hd136", Hd=136, Hdp=128))
    c.append(chain("hdp192", Hd=128, Hdp=192))
    c.append(chain("hdp384", Hd=256, Hdp=384))
    c.append(chain("hdp256.hd128", Hd=128, Hdp=256))
    c.append(chain("m0", M=0))
    c.append(chain("skip_rows.above", skip_rows=1001))
    c.append(chain("skip_rows.no_divisor", skip_rows=300))
    c.append(chain("skip_rows.divisor", skip_rows=250))
    for name, post, nxt in [("post_g", (1, 0), (0, 0)), ("post_b", (0, 1), (0, 0)), ("post", (1, 1), (0, 0)), ("wnext", (0, 0), (1, 0)),
                            ("out_next", (0, 0), (0, 1))]:
        c.append(chain("only." + name, post=post, nxt=nxt))
        c.append(chain("only.%s.c7" % name, post=post, nxt=nxt, C=7))                  # SHAPE is checked first
        c.append(chain("f32.only." + name, post=post, nxt=nxt, dtype=1))
        c.append(chain("f32.only.%s.m0" % name, post=post, nxt=nxt, dtype=1, M=0))      # fp32: ARG is checked first
    for Nn in (4, 8, 12, 768, 776):
        c.append(chain("nn%d" % Nn, Nn=Nn))
    for act in (-1, 0, 1, 2, 3):
        c.append(chain("next_act%d" % act, Nn=128, next_act=act))
    c.append(chain("next_act3.no_next", next_act=3))
    c.append(chain("null_required", req=0))
    c.append(chain("null_dims", req=2))
    c.append(chain("dtype2", dtype=2))
    # ---- row chain, fp32 storage
    c.append(chain("f32", dtype=1))
    c.append(chain("f32.rows64", dtype=1, rows=64))
    c.append(chain("f32.c64", dtype=1, C=64, Hd=128))
    c.append(chain("f32.c120", dtype=1, C=120))
    c.append(chain("f32.hd128", dtype=1, Hd=128, Hdp=256))
    c.append(chain("f32.hdp128", dtype=1, Hd=256, Hdp=128))
    for Nn in (4, 6, 384, 768, 772):
        c.append(chain("f32.nn%d" % Nn, dtype=1, Nn=Nn))
    c.append(chain("f32.nn6.no_next", dtype=1, Nn=6, nxt=(0, 0)))
    c.append(chain("f32.m0", dtype=1, M=0))
    c.append(chain("f32.skip_rows.above", dtype=1, skip_rows=1001))
    c.append(chain("f32.skip_rows.no_divisor", dtype=1, skip_rows=300))
    c.append(chain("f32.next_act3", dtype=1, Nn=128, next_act=3))
    c.append(chain("f32.next_act-1", dtype=1, Nn=128, next_act=-1))
    c.append(chain("f32.next_act3.c64", dtype=1, Nn=128, next_act=3, C=64))             # SHAPE before UNSUPPORTED
    # ---- projection chain
    c.append(proj("m32767", M=32767))
    c.append(proj("m32768", M=32768))
    for Nn in (64, 96, 128, 256, 288):
        c.append(proj("big.nn%d" % Nn, M=32768 + 77, Nn=Nn))
    c.append(proj("big.next_act1", M=32768, next_act=1))
    c.append(proj("big.variant1", M=32768, variant=1))
    c.append(proj("big.no_pre.no_skip", M=32768, pre=(0, 0), skip=0))
    for M in (65280, 65536, 65537):                  # eight waves: 255, 256, 257 -> 256 workgroups
        c.append(proj("cap.m%d" % M, M=M))
    c.append(proj("small"))
    c.append(proj("null_required", req=0))
    c.append(proj("null_dims", req=2))
    c.append(proj("only.pre_scale", pre=(1, 0)))
    c.append(proj("only.pre_shift", pre=(0, 1)))
    c.append(proj("only.pre_scale.dtype1", pre=(1, 0), dtype=1))                        # ARG before UNSUPPORTED
    c.append(proj("dtype1", dtype=1))
    c.append(proj("dtype1.m0", dtype=1, M=0))
    c.append(proj("m0", M=0))
    c.append(proj("c64", C=64))
    for Nn in (4, 8, 12, 768, 776):
        c.append(proj("nn%d" % Nn, Nn=Nn))
    for act in (-1, 2, 3):
        c.append(proj("next_act%d" % act, next_act=act))
    c.append(proj("skip_rows.above", skip_rows=1001))
    c.append(proj("skip_rows.no_divisor", skip_rows=300))
    c.append(proj("skip_rows.divisor", skip_rows=250))
    # ---- small-K row GEMM: every check in bf16 and fp32
    for dt, tag in ((0, "bf16"), (1, "f32")):
        k = lambda name, **kw: small_k("%s.%s" % (tag, name), dtype=dt, **kw)
        c.append(k("plain"))
        c.append(k("m0", M=0))
        for N in (2, 4, 8, 12, 4096, 4100, 4104):
            c.append(k("n%d" % N, N=N))
        for K in (2, 4, 8, 12, 64, 72, 512, 516, 520):
            c.append(k("k%d" % K, K=K))
        c.append(k("lda.below", K=128, lda=120))
        c.append(k("lda.plus4", K=128, lda=132))
        c.append(k("lda.plus8", K=128, lda=136))
        for K in (64, 128, 136):
            c.append(k("ln.k%d" % K, K=K, ln=1))
        c.append(k("stride0", in_stride=0))
        c.append(k("stride2", M=1024, in_stride=2, src=(16, 16), inn=(32, 32)))
        c.append(k("stride2.src0", M=1024, in_stride=2, src=(0, 16), inn=(32, 32)))
        c.append(k("stride2.in0", M=1024, in_stride=2, src=(16, 16), inn=(32, 0)))
        c.append(k("stride2.rows", M=1000, in_stride=2, src=(16, 16), inn=(32, 32)))
        c.append(k("stride2.residual", M=1024, in_stride=2, src=(16, 16), inn=(32, 32), res=1))
        c.append(k("residual", res=1))
        c.append(k("pre", pre=(1, 1), pre_relu=1))
        c.append(k("only.pre_scale", pre=(1, 0)))
        c.append(k("only.pre_shift", pre=(0, 1)))
        c.append(k("ln.pre", ln=1, pre=(1, 1)))
        c.append(k("ln.only.pre_scale", ln=1, pre=(1, 0)))                              # the pair check comes first
        for act in (-1, 4, 5):
            c.append(k("act%d" % act, act=act))
        c.append(k("rows64", rows=64))
        c.append(k("rows16", rows=16))
        c.append(k("largest", K=512, N=4096, rows=64))
        c.append(k("null_required", req=0))
        c.append(k("null_dims", req=2))
        c.append(k("big64.ln", M=65536, N=192, K=64, ln=1))
    c.append(small_k("dtype2", dtype=2))
    c.append(small_k("dtype2.m0", dtype=2, M=0))
    # ---- ... its wave-level LayerNorm + Linear form
    c.append(ln64("m65535", M=65535))
    c.append(ln64("m65536"))
    c.append(ln64("lda128", lda=128))
    for N in (16, 32, 48, 64, 96, 128, 160, 192, 224):
        c.append(ln64("n%d" % N, N=N))
    c.append(ln64("act2", act=2))
    c.append(ln64("rows64", rows=64))
    c.append(ln64("residual", res=1))
    c.append(ln64("pre", pre=(1, 1)))
    c.append(ln64("pre_relu", pre_relu=1))
    c.append(ln64("stride2", in_stride=2, src=(128, 128), inn=(256, 256)))
    c.append(small_k("ln64.ln0", M=65536, N=192, K=64))
    c.append(small_k("ln64.k128", M=65536, N=192, K=128, ln=1))
    c.append(ln64("gate0", gates=(1, 0, 1536)))
    for M in (196480, 196608, 196609):               # 1535, 1536, 1537 -> 1536 workgroups
        c.append(ln64("cap.m%d" % M, M=M))
    for M in (65536, 65537):                         # COBEVT_LN64_BLOCKS=512: 512, 513 -> 512
        c.append(ln64("cap512.m%d" % M, M=M, gates=(1, 1, 512)))
    # ---- BEV-embedding GEMM
    c.append(bev("hw32", hw=32))
    c.append(bev("hw48", hw=48))
    c.append(bev("hw64"))
    c.append(bev("xbcast", xb=1))
    c.append(bev("d64", D=64))
    c.append(bev("n64", N=64))
    c.append(bev("ln0", ln=0))
    c.append(bev("d64.hw48", D=64, hw=48))
    c.append(bev("cams32", B=8, n=4))
    c.append(bev("cams33", B=11, n=3))
    for hw in (4064, 4096, 4128):                    # 762, 768, 774 -> 768 workgroups
        c.append(bev("cap.hw%d" % hw, B=4, n=6, hw=hw))
    c.append(bev("hw0", hw=0))                       # reaches the wave-level kernel with an empty grid (a launch error on the GPU)
    c.append(bev("hw0.d64", hw=0, D=64))
    c.append(bev("b0", B=0))
    c.append(bev("cams0", n=0))
    c.append(bev("rows2g", B=4, n=8, hw=1 << 26))
    c.append(bev("rows2g.d64", B=4, n=8, hw=1 << 26, D=64))
    for N in (4, 12, 4096, 4104):
        c.append(bev("n%d" % N, N=N))
    for D in (4, 8, 12, 136):
        c.append(bev("d%d" % D, D=D))
    c.append(bev("dtype1", dtype=1))
    c.append(bev("null_required", req=0))
    c.append(bev("null_dims", req=2))
    # ---- agent-mean GEMM
    c.append(mean("plain"))
    for L in (0, 1, 64, 65):
        c.append(mean("l%d" % L, L=L))
    for K in (4, 8, 12, 128, 136):
        c.append(mean("k%d" % K, K=K))
    for N in (4, 12, 4096, 4104):
        c.append(mean("n%d" % N, N=N))
    for act in (-1, 4, 5):
        c.append(mean("act%d" % act, act=act))
    c.append(mean("ln0", ln=0))
    c.append(mean("b0", B=0))
    c.append(mean("r0", R=0))
    c.append(mean("rows2g", B=65536, R=32768))
    c.append(mean("dtype1", dtype=1))
    c.append(mean("null_required", req=0))
    c.append(mean("null_dims", req=2))
    return c


# entry point -> (case entry, index of dims, indices of the required pointers, indices of the nullable pointers the routing looks at)
TRACED = {"cobevt_attn_mlp_chain": ("chain", 14, (0, 2, 3, 5, 6, 7, 8), (1, 9, 10, 11, 13)),
          "cobevt_proj_chain": ("proj", 10, (0, 4, 7, 8, 9), (1, 2, 3)),
          "cobevt_linear_rows_small_k": ("small_k", 7, (0, 1, 6), (3, 4, 5)),
          "cobevt_bev_embed_linear_rows_small_k": ("bev", 9, (0, 1, 2, 3, 4, 5, 6, 8), ()),
          "cobevt_mean_linear_rows_small_k": ("mean", 4, (0, 1, 3), ())}


def trace_cases():
    """Every distinct record [library variant, symbol, arguments] of the five entry points in the launch-trace fixtures as a case
    line (dims, null-ness of the pointers the routing looks at), named trace.<entry>.<variant>.<NNN> in sorted order.  The routing
    does not depend on the library, so two variants' records of one call give the same line under two names."""
    seen = set()
    for path in sorted(glob.glob(os.path.join(TRACES, "*.jsonl.gz"))):
        with gzip.open(path, "rt") as f:
            for ln in f:
                variant, sym, args = json.loads(ln)
                if sym in TRACED:
                    seen.add((TRACED[sym][0], variant or "native", json.dumps(args), sym))
    lines = []
    for i, (entry, variant, args, sym) in enumerate(sorted(seen)):
        args, (_, d, required, optional) = json.loads(args), TRACED[sym]
        flags = [int(all(args[j] == "ptr" for j in required))] + [int(args[j] == "ptr") for j in optional]
        lines.append(line("trace.%s.%s.%03d" % (entry, variant, i), entry, args[d], flags))
    return lines


def write_cases():
    lines = table() + trace_cases()
    names = [ln.split()[0] for ln in lines]
    assert len(set(names)) == len(names)
    os.makedirs(GOLDEN, exist_ok=True)
    with open(CASES, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d cases (%d from the launch traces) -> %s" % (len(lines), len(trace_cases()), CASES))


_KERNEL = re.compile(r"(\w+_kernel)(<[^>]*>)?")


def parse_oracle(text):
    """{case name: its expected.jsonl line, in the exact text tests/rows_select_main.cpp prints}"""
    out, name, launches = {}, None, []
    for ln in text.splitlines():
        kind, _, rest = ln.partition(" ")
        if kind == "case":
            name, launches = rest, []
        elif kind == "launch":
            sym, _, nums = rest.rpartition(" | ")
            m = _KERNEL.search(sym)
            launches.append((m.group(1) + (m.group(2) or ""), [int(v) for v in nums.split()]))
        elif kind == "rc":
            rc = int(rest)
            if not launches:
                assert rc != 0
                out[name] = '{"name": "%s", "status": %d}' % (name, rc)
            else:
                assert rc == 0 and len(launches) == 1
                kernel, (gx, gy, gz, block, lds, nblk) = launches[0]
                out[name] = ('{"name": "%s", "status": 0, "kernel": "%s", "grid": [%d, %d, %d], "block": %d, "lds": %d, "nblk": %d}'
                             % (name, kernel, gx, gy, gz, block, lds, nblk))
    return out


def record(rev, out):
    with tempfile.TemporaryDirectory() as tmp:
        csrc = sf.checkout(rev, tmp)
        exe = sf.build_oracle(tmp, [os.path.join(ROOT, "tools", "rows_select_oracle.cpp")] + [os.path.join(csrc, u) for u in UNITS])
        cases = open(CASES).read()
        runs = {gates: parse_oracle(sf.run_twice(exe, cases, "COBEVT_", env)) for gates, env in GATES}
    lines = []
    for ln in cases.splitlines():
        tok = ln.split()
        lines.append(runs[tuple(int(v) for v in tok[-3:])][tok[0]])
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d records from %s -> %s" % (len(lines), rev, out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("what", choices=("cases", "record"))
    ap.add_argument("--rev", help="record: the commit whose entry points are the reference")
    ap.add_argument("--out", default=EXPECTED)
    a = ap.parse_args()
    if a.what == "cases":
        write_cases()
    elif not a.rev:
        ap.error("record needs --rev")
    else:
        record(a.rev, a.out)
