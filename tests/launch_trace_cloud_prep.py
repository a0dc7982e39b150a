"""CPU launch traces of host.DataAugmentor.forward, recorded with the recorder of tests/launch_trace.py: a queue in the operator's own
order (flip, rotation, scaling) is ONE cobevt_prepare_points call, any other queue one call per entry, in queue order.  The fixtures
live in their own directory, tests/golden/launch_traces_cloud_prep/ (launch_trace.py's CASES and directory stay as they are);
`python tests/launch_trace_cloud_prep.py` rewrites them."""
import gzip
import json
import os

import numpy as np
import torch

import launch_trace as lt
from cobevt_amd import host, ops

import cases_cloud as cc

FIXTURES = os.path.join(lt.ROOT, "tests", "golden", "launch_traces_cloud_prep")
# fixed parameters (DataAugmentor.draw's format), so that the traces do not depend on a random generator
CASES = {
    "canonical": (cc.AUG_CONFIG, [[("x", True), ("y", False)], 0.25, 1.03125]),
    "reversed": (cc.AUG_CONFIG[::-1], [1.03125, 0.25, [("x", True), ("y", False)]]),
    "flip_y_before_x": ([{"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["y", "x"]}, cc.AUG_CONFIG[2]], [[("y", True), ("x", True)], None]),
    "rotation_twice": ([cc.AUG_CONFIG[1], cc.AUG_CONFIG[1]], [0.25, -0.5]),
}
POINTS, OFFSETS = 2500, [0, 1000, 2500]


def run(name):
    config, params = CASES[name]
    b, m = cc.boxes("trace")
    data = {"lidar_np": torch.from_numpy(cc.raw_cloud("trace", POINTS)), "object_bbx_center": torch.from_numpy(b),
            "object_bbx_mask": torch.from_numpy(m), "point_offsets": torch.tensor(OFFSETS, dtype=torch.int32)}
    ops._CLOUD_WS.clear()          # the default workspace is cached per shape: every run starts with the question for its size
    try:
        out = host.DataAugmentor(config, train=True).forward(data, params=params)
    finally:
        ops._CLOUD_WS.clear()      # (sized by the fake library)
    assert out is data and tuple(out["lidar_np"].shape) == (POINTS, 4) and np.array_equal(out["object_bbx_mask"].numpy(), m)


def trace(name, setattr_):
    rec = lt.Recorder()
    lt.install(setattr_, rec)
    run(name)
    return rec.records


def fixture_path(name):
    return os.path.join(FIXTURES, "data_augmentor.%s.jsonl.gz" % name)


def read_fixture(name):
    with gzip.open(fixture_path(name), "rt") as f:
        return [json.loads(line) for line in f]


if __name__ == "__main__":
    os.makedirs(FIXTURES, exist_ok=True)
    for case in sorted(CASES):
        first = lt.dumps(trace(case, setattr))
        if lt.dumps(trace(case, setattr)) != first:
            raise SystemExit("%s: two runs gave different traces" % case)
        with open(fixture_path(case), "wb") as f:
            f.write(gzip.compress(first.encode(), mtime=0))
        print("%-20s %5d launches  %7d bytes" % (case, first.count("\n"), len(first)))
