"""CPU: the attention routing of csrc/attn_select.hpp (attn_parse + attn_select) against tests/golden/attn_select/.

tests/attn_select_main.cpp is compiled as plain host C++ with the compiler the build uses and run as a child process over every
line of cases.txt; its output must equal expected.jsonl line for line.  The expected lines were recorded from the attention entry
point of the commit BEFORE the routing moved into the header (tools/attn_select_fixture.py: its launches intercepted on the CPU),
never from the header itself.  That recording ran without a GPU, where the entry point assumes 256 compute units - the MI355X's
count - so the table pins cus = 256 only."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import attn_select_fixture as fx  # noqa: E402
from cobevt_amd import build  # noqa: E402

HEADER = os.path.join(build.CSRC, "attn_select.hpp")


def _cxx(args):
    """hipcc as a host-only C++17 compiler; a missing compiler is a failure, not a skip"""
    try:
        hipcc = build._hipcc()
    except RuntimeError as e:
        pytest.fail("no compiler for the CPU test: %s" % e)
    # the public header the status codes come from declares its entry points with hipStream_t: the HIP API header's directory, nothing more
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(hipcc) or hipcc))), "include")
    p = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-Wno-comment", "-D__HIP_PLATFORM_AMD__=1", "-isystem", rocm_include]
                       + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attn_select") / "attn_select_main")
    _cxx(["-O1", os.path.join(ROOT, "tests", "attn_select_main.cpp"), "-o", exe])
    return exe


def test_every_case_selects_what_the_parent_launched(program):
    cases = open(fx.CASES).read()
    want = open(fx.EXPECTED).read().splitlines()
    p = subprocess.run([program], input=cases.encode(), stdout=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    got = p.stdout.decode().splitlines()
    assert len(cases.splitlines()) == len(want) > 200
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


def test_cases_file_is_the_table_plus_every_trace_record():
    """cases.txt is what the tool writes today: no case of the table left out, every distinct forward attention record of the 43
    launch-trace fixtures in it (57 at present: 40 plain, 8 key-split, 9 lse)"""
    assert open(fx.CASES).read().splitlines() == fx.table() + fx.trace_cases()


def test_header_compiles_on_its_own(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "%s"\n' % HEADER)
    _cxx(["-fsyntax-only", str(src)])
