#!/usr/bin/env python
"""ops.prepare_points (csrc/cloud_prep.hip) on one GPU at the workload's own shape: 5 agents x 65 536 points, every stage on (ego
mask, fp64 projection, flip / rotation / scaling, range mask, compaction), against the same steps written with torch indexing on the
device - an fp64 matmul per agent, boolean masks, `cat` - in the same job.  HIP events after warm-up, `--steps` batches of 20 calls
between one event pair each, medians; next to the operator's time an upper bound on the HBM bytes it moves per point (scatter counted as
loading every point again) and the rate that bound would give against the stream-copy bandwidth bench.box_calibration measures in the
same run.
Usage (GPU box): python tools/time_cloud_prep.py [--steps 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import cases_cloud as cc  # noqa: E402
import cloud_ref as cr  # noqa: E402
from cobevt_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda")
torch.set_grad_enabled(False)
AGENTS, POINTS = 5, 65536
WORLD = {"flip_x": True, "flip_y": False, "rot": 0.5, "scale": 1.03}


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def timed(step):
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            step()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / 20)
    return median(ts)


def main():
    try:
        cal = bench.box_calibration(dev)
    except Exception as exc:
        cal = {"unavailable": repr(exc)}
    print(json.dumps({"box_calibration": cal}), flush=True)
    clouds = [cc.raw_cloud("time.%d" % a, POINTS) for a in range(AGENTS)]
    pts, offs = cc.concat(clouds)
    mats = np.stack([cc.transform("time.%d" % a) for a in range(AGENTS)])
    p, o, t = torch.from_numpy(pts).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(mats).to(dev)
    c, s = ops.rotation_cos_sin(WORLD["rot"])
    out = (torch.empty(len(pts), 4, device=dev), torch.empty(AGENTS + 1, dtype=torch.int32, device=dev))

    def ours():
        return ops.prepare_points(p, o, t, ego_mask=True, lidar_range=cc.LIDAR_RANGE, world=WORLD, out=out)

    lo = torch.tensor(cc.LIDAR_RANGE[:3], device=dev, dtype=torch.float32)
    hi = torch.tensor(cc.LIDAR_RANGE[3:], device=dev, dtype=torch.float32)
    rot = torch.tensor([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]], device=dev, dtype=torch.float32)
    bounds = offs.tolist()

    def indexed():
        """the same steps with torch indexing: the result's size is data-dependent, so every boolean index synchronises"""
        parts = []
        for a in range(AGENTS):
            q = p[bounds[a]:bounds[a + 1]]
            ego = (q[:, 0] >= -1.95) & (q[:, 0] <= 2.95) & (q[:, 1] >= -1.1) & (q[:, 1] <= 1.1)
            q = q[~ego]
            xyz = (torch.cat([q[:, :3].double(), torch.ones(len(q), 1, device=dev, dtype=torch.float64)], dim=1) @ t[a].T)[:, :3]
            xyz[:, 1] = -xyz[:, 1]
            xyz = (xyz.float() @ rot) * WORLD["scale"]
            keep = ((xyz > lo) & (xyz < hi)).all(dim=1)
            parts.append(torch.cat([xyz, q[:, 3:]], dim=1)[keep])
        return torch.cat(parts)

    got = ours()
    torch.cuda.synchronize()
    ref = cr.prepare_points(pts, offs, mats, None, True, cc.LIDAR_RANGE, WORLD, c, s)
    kept = int(got[1][-1])
    exact = np.array_equal(got[1].cpu().numpy(), ref[1]) and np.array_equal(got[0][:kept].cpu().numpy().view(np.int32), ref[0].view(np.int32))
    same_rows = tuple(indexed().shape) == (kept, 4)
    us_ours, us_indexed = timed(ours), timed(indexed)
    m = len(pts)
    # an UPPER bound on the traffic: classify reads, scatter reading every point again (it loads only the kept ones, a cache line of
    # eight points at a time), scatter writes, the flag bits twice
    moved = 16.0 * m + 16.0 * m + 16.0 * kept + m / 4.0
    print("shape: %d agents x %d points, every stage on: %d of %d points kept; equal to the restatement bit for bit: %s; the indexed "
          "form keeps the same number of rows: %s" % (AGENTS, POINTS, kept, m, exact, same_rows))
    line = "prepare_points (3 launches, eager, 20 calls per event pair):  %8.1f us   at most %.1f bytes per point move -> at most %.0f GB/s" \
        % (us_ours, moved / m, moved / us_ours / 1e3)
    if "hbm_copy_gbs" in cal:
        line += " = %.0f %% of the stream copy (%.0f GB/s)" % (100 * moved / us_ours / 1e3 / cal["hbm_copy_gbs"], cal["hbm_copy_gbs"])
    print(line)
    print("torch indexing (fp64 matmul, boolean masks, cat):             %8.1f us   = %.1f x" % (us_indexed, us_indexed / us_ours))


if __name__ == "__main__":
    main()
