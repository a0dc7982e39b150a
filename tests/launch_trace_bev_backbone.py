"""CPU launch traces of PointPillarFuseBEVT with the BaseBEVBackbone and the detection head, recorded with the recorder of
tests/launch_trace.py.  The fixtures live in their own directory, tests/golden/launch_traces_bev_backbone/ (launch_trace.py's CASES and
directory stay as they are); `python tests/launch_trace_bev_backbone.py` rewrites them."""
import copy
import gzip
import json
import os
import sys

import torch

import launch_trace as lt
from cobevt_amd import host, synth

import bev_backbone_ref as br
import cases_pillar as cp

FIXTURES = os.path.join(lt.ROOT, "tests", "golden", "launch_traces_bev_backbone")
GRID = (16, 24)
COUNTS = [22, 18]              # two agents, 40 pillars


def model_args():
    fusion = copy.deepcopy(cp.FUSION)
    fusion.update(agent_size=2, depth=1, drop_out=0.0)
    args = cp.model_args(grid=GRID, max_cav=2, fusion=fusion)
    args["base_bev_backbone"] = copy.deepcopy(br.GOLDEN_CFG)         # on the 64-channel fused map: 96 channels at 8 x 12
    args["anchor_number"] = 2
    return args


def voxels():
    return cp.voxels(counts=COUNTS, grid=GRID, tag="gv25")


def run(mode):
    torch.manual_seed(0)
    model = synth.fill_module_(host.PointPillarFuseBEVT(model_args()), 0).eval()
    with torch.no_grad(), host.compute_dtype(mode):
        return model({"processed_lidar": voxels(), "record_len": torch.tensor([2], dtype=torch.int32)})


def trace(mode, setattr_):
    rec = lt.Recorder()
    lt.install(setattr_, rec)
    run(mode)
    return rec.records


def fixture_path(mode):
    return os.path.join(FIXTURES, "point_pillar_bev_backbone.%s.jsonl.gz" % mode)


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
