"""CPU launch traces of one PreNorm(HGTCavAttention) + x layer (hgt_ref.MODULE_CASES["d64"]), recorded with the recorder of
tests/launch_trace.py.  The fixtures live in their own directory, tests/golden/launch_traces_hgt/ (launch_trace.py's CASES and
directory stay as they are); `python tests/launch_trace_hgt.py` rewrites them."""
import gzip
import json
import os
import sys

import torch

import launch_trace as lt
from cobevt_amd import host

import hgt_ref as hr

FIXTURES = os.path.join(lt.ROOT, "tests", "golden", "launch_traces_hgt")
CASE = "d64"


def run(mode):
    c = hr.MODULE_CASES[CASE]
    x, mask, prior, _ = hr.module_inputs(CASE)
    layer = hr.fill_hgt_(host.PreNorm(c["dim"], host.HGTCavAttention(c["dim"], c["heads"], num_types=c["T"], num_relations=c["R"], dim_head=32)), 0).eval()
    with torch.no_grad(), host.compute_dtype(mode):
        return layer(x, mask=mask, prior_encoding=prior) + x


def trace(mode, setattr_):
    rec = lt.Recorder()
    lt.install(setattr_, rec)
    run(mode)
    return rec.records


def fixture_path(mode):
    return os.path.join(FIXTURES, "prenorm_hgt.%s.jsonl.gz" % mode)


def read_fixture(mode):
    with gzip.open(fixture_path(mode), "rt") as f:
        return [json.loads(line) for line in f]


if __name__ == "__main__":
    os.makedirs(FIXTURES, exist_ok=True)
    for mode in (sys.argv[1:] or lt.MODES):
        first = lt.dumps(trace(mode, setattr))
        if lt.dumps(trace(mode, setattr)) != first:
            raise SystemExit("%s: two runs gave different traces" % mode)
        with open(fixture_path(mode), "wb") as f:
            f.write(gzip.compress(first.encode(), mtime=0))
        print("%-12s %5d launches  %7d bytes" % (mode, first.count("\n"), len(first)))
