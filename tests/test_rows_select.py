"""CPU: the row-local routing of csrc/rows_select.hpp (row chain, projection chain, small-K row GEMMs) against tests/golden/rows_select/.

tests/rows_select_main.cpp is compiled as plain host C++ with the compiler the build uses and run as a child process over every
line of cases.txt; its output must equal expected.jsonl line for line.  The expected lines were recorded from the five entry points
of the commit BEFORE the routing moved into the header (tools/rows_select_fixture.py: their launches intercepted on the CPU, one
process per setting of the environment gates), never from the header itself."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rows_select_fixture as fx  # noqa: E402
from test_attn_select import _cxx  # noqa: E402
from cobevt_amd import build  # noqa: E402

HEADER = os.path.join(build.CSRC, "rows_select.hpp")

# every instantiation the five entry points can launch
KERNELS = (["row_chain_kernel<%d, %d, %s, true>" % (npass, rows, full) for npass in (1, 2) for rows in (32, 64) for full in ("false", "true")]
           + ["row_chain_kernel<1, 32, true, false>"]
           + ["row_chain64_kernel<%d, %s>" % (nnt, form) for nnt in (0, 2, 4, 6) for form in ("4, true", "6, true", "6, false")]
           + ["row_chain_f32_kernel", "proj_chain128_kernel<4, 8>", "proj_chain128_kernel<8, 8>"]
           + ["ln_linear64_kernel<%d, 4>" % nnt for nnt in range(1, 7)]
           + ["gemm_rows3_kernel<false, 32>", "gemm_rows3_kernel<false, 64>", "gemm_rows3_kernel<true, 32>", "gemm_rows3_f32_kernel",
              "bev_query_kernel<4>"])
# every status other than OK an entry can return without launching (1 ARG, 2 SHAPE, 4 UNSUPPORTED)
ERRORS = {"chain": {1, 2, 4}, "proj": {1, 2, 4}, "small_k": {1, 2, 4}, "bev": {1, 2, 4}, "mean": {1, 2, 4}}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rows_select") / "rows_select_main")
    _cxx(["-O1", os.path.join(ROOT, "tests", "rows_select_main.cpp"), "-o", exe])
    return exe


def test_every_case_selects_what_the_parent_launched(program):
    cases = open(fx.CASES).read()
    want = open(fx.EXPECTED).read().splitlines()
    p = subprocess.run([program], input=cases.encode(), stdout=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    got = p.stdout.decode().splitlines()
    assert len(cases.splitlines()) == len(want) > 500
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


def test_cases_file_is_the_table_plus_every_trace_record():
    """cases.txt is what the tool writes today: no case of the table left out, every distinct record of the five entry points in the
    launch-trace fixtures in it (294 at present: 20 attn_mlp_chain, 272 linear_rows_small_k, 2 mean_linear_rows_small_k)"""
    assert open(fx.CASES).read().splitlines() == fx.table() + fx.trace_cases()


def test_expected_covers_every_instantiation_and_error():
    records = [json.loads(ln) for ln in open(fx.EXPECTED)]
    entries = [ln.split()[1] for ln in open(fx.CASES)]
    assert len(KERNELS) == 9 + 12 + 1 + 2 + 6 + 3 + 1 + 1
    assert {r["kernel"] for r in records if r["status"] == 0} == set(KERNELS)
    for entry, codes in ERRORS.items():
        assert {r["status"] for r, e in zip(records, entries) if e == entry} - {0} == codes, entry


def test_header_compiles_on_its_own(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "%s"\n' % HEADER)
    _cxx(["-fsyntax-only", str(src)])
