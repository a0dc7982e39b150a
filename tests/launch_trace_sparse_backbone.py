"""CPU launch traces of host.MeanVFE -> host.VoxelBackBone8x -> host.HeightCompression, recorded with the recorder of
tests/launch_trace.py: one cobevt_mean_vfe, one cobevt_sparse_index, four cobevt_sparse_downsample, twelve cobevt_sparse_conv and one
cobevt_sparse_dense per forward, with the shapes, capacities and layer geometry each of them is given.  The fixtures live in their own
directory, tests/golden/launch_traces_sparse_backbone/ (launch_trace.py's CASES and directory stay as they are);
`python tests/launch_trace_sparse_backbone.py` rewrites them."""
import gzip
import json
import os

import torch

import launch_trace as lt
from cobevt_amd import host, ops

import sparse_ref as sr

FIXTURES = os.path.join(lt.ROOT, "tests", "golden", "launch_traces_sparse_backbone")
GRID, BATCH, SLOTS = (21, 13, 40), 2, 5
# name -> (compute mode, level_capacities)
CASES = {
    "bf16": ("bf16", None),
    "fp32": ("fp32", None),
    "fp32_split": ("fp32_split", None),
    "fp32_capped": ("fp32", [None, 300, None, 40, None]),
}


def run(name):
    mode, caps = CASES[name]
    coords = torch.from_numpy(sr.clustered_coords(GRID, BATCH, 1))
    p = coords.shape[0]
    data = {"voxel_features": torch.zeros(p, SLOTS, 4), "voxel_num_points": torch.ones(p, dtype=torch.int32), "voxel_coords": coords,
            "batch_size": BATCH}
    vfe = host.MeanVFE({}, 4).eval()
    backbone = host.VoxelBackBone8x({"level_capacities": caps}, 4, list(GRID)).eval()
    to_bev = host.HeightCompression({"feature_num": 256}).eval()
    ops._SPARSE_WS.clear()         # the default workspaces are cached per shape: every run starts with the question for their size
    try:
        with torch.no_grad(), host.compute_dtype(mode):
            out = to_bev(backbone(vfe(data)))
    finally:
        ops._SPARSE_WS.clear()     # (sized by the fake library)
    d, h, w = backbone.level_shapes()[-1]
    assert out is data and tuple(out["spatial_features"].shape) == (BATCH, 128 * d, h, w) and out["spatial_features_stride"] == 8


def trace(name, setattr_):
    rec = lt.Recorder()
    lt.install(setattr_, rec)
    run(name)
    return rec.records


def fixture_path(name):
    return os.path.join(FIXTURES, "voxel_backbone8x.%s.jsonl.gz" % name)


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
