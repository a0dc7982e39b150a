"""CPU launch traces of one training step (forward + backward, fp32) of the two LiDAR detectors, recorded with the recorder of
tests/launch_trace.py: PointPillarIntermediate (tests/att_backbone_ref.pillar_args) and PointPillarFuseBEVT with the BaseBEVBackbone and
the detection head (tests/launch_trace_bev_backbone.model_args).  On CPU tensors the modules' train()-mode forwards refuse, so the
host.training functions are called directly.  The fixtures live in their own directory, tests/golden/launch_traces_detector_train/
(launch_trace.py's CASES and directory stay as they are: tools/attn_select_fixture.py and tools/rows_select_fixture.py enumerate every
file there); `python tests/launch_trace_detector_train.py` rewrites them."""
import gzip
import json
import os
import sys

import torch

import launch_trace as lt
from cobevt_amd import host, synth
from cobevt_amd.host import training

import att_backbone_ref as ar
import launch_trace_bev_backbone as ltb

FIXTURES = os.path.join(lt.ROOT, "tests", "golden", "launch_traces_detector_train")
CHUNKS = 3          # what the fake library answers for cobevt_deconv_wgrad_chunks (a size, not a status)
CASES = ("point_pillar_intermediate_train.fp32", "point_pillar_bev_backbone_train.fp32")


def _step(out):
    (out["psm"].float().sum() + out["rm"].float().sum()).backward()


def run(case):
    torch.manual_seed(0)
    with torch.enable_grad(), host.compute_dtype("fp32"):
        if case.startswith("point_pillar_intermediate"):
            model = synth.fill_module_(host.PointPillarIntermediate(ar.pillar_args()), 0).train()
            _step(training.point_pillar_intermediate(model, {"processed_lidar": ar.pillar_voxels(), "record_len": ar.PILLAR_RECORD_LEN}))
        else:
            model = synth.fill_module_(host.PointPillarFuseBEVT(ltb.model_args()), 0).train()
            _step(training.point_pillar_fusebevt(model, {"processed_lidar": ltb.voxels(), "record_len": torch.tensor([2], dtype=torch.int32)}))
    return model


def trace(case, setattr_):
    rec = lt.Recorder({"cobevt_deconv_wgrad_chunks": CHUNKS})
    lt.install(setattr_, rec)
    run(case)
    return rec.records


def fixture_path(case):
    return os.path.join(FIXTURES, case + ".jsonl.gz")


def read_fixture(case):
    with gzip.open(fixture_path(case), "rt") as f:
        return [json.loads(line) for line in f]


if __name__ == "__main__":
    os.makedirs(FIXTURES, exist_ok=True)
    for case in (sys.argv[1:] or CASES):
        first = lt.dumps(trace(case, setattr))
        if lt.dumps(trace(case, setattr)) != first:
            raise SystemExit("%s: two runs gave different traces" % case)
        with open(fixture_path(case), "wb") as f:
            f.write(gzip.compress(first.encode(), mtime=0))
        print("%-44s %5d launches  %7d bytes" % (case, first.count("\n"), len(first)))
