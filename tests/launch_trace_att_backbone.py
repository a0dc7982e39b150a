"""CPU launch traces of PointPillarIntermediate (pillar front end -> AttBEVBackbone -> heads), recorded with the recorder of
tests/launch_trace.py.  The fixtures live in their own directory, tests/golden/launch_traces_att_backbone/ (launch_trace.py's CASES
and directory stay as they are); `python tests/launch_trace_att_backbone.py` rewrites them."""
import gzip
import json
import os
import sys

import torch

import launch_trace as lt
from cobevt_amd import host, synth

import att_backbone_ref as ar

FIXTURES = os.path.join(lt.ROOT, "tests", "golden", "launch_traces_att_backbone")


def run(mode):
    torch.manual_seed(0)
    model = synth.fill_module_(host.PointPillarIntermediate(ar.pillar_args()), 0).eval()
    with torch.no_grad(), host.compute_dtype(mode):
        return model({"processed_lidar": ar.pillar_voxels(), "record_len": torch.tensor(ar.PILLAR_RECORD_LEN, dtype=torch.int32)})


def trace(mode, setattr_):
    rec = lt.Recorder()
    lt.install(setattr_, rec)
    run(mode)
    return rec.records


def fixture_path(mode):
    return os.path.join(FIXTURES, "point_pillar_intermediate.%s.jsonl.gz" % mode)


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
