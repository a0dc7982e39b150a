#!/usr/bin/env python
"""The voxeliser (csrc/voxelize.hip) on one GPU at full size: 8 agents x 65 536 points on 256 x 256 cells, T = 32, max_voxels = 32 000
(the full-size case of tests/test_voxelize_gpu.py).  Times the whole call with HIP events - warm-up, then `--steps` batches of 20 calls
between one event pair each, median - and each of its seven launches from torch.profiler's device-side kernel records over the same
calls (median per kernel name).  Next to each time: the HBM bytes the launch has to move and the rate that gives, against the stream-copy
bandwidth bench.box_calibration measures in the same run; for the classify and fill launches the integer atomics per second.
Usage (GPU box): python tools/voxel_probe.py [--steps 20]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import cases_voxel as cv  # noqa: E402
import voxel_ref as vr  # noqa: E402
from cobevt_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda")
torch.set_grad_enabled(False)
T = 32
KERNELS = ["voxel_clear", "voxel_classify", "voxel_reduce", "voxel_scan", "voxel_apply", "voxel_fill", "voxel_select"]


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    cal = bench.box_calibration(dev)
    copy = cal["hbm_copy_gbs"]
    pts, offs, rng = cv.full_case()
    ref = vr.voxelize_fast(pts, offs, rng, cv.VOXEL_SIZE, T, cv.FULL_MAX_VOXELS)
    p, o = torch.from_numpy(pts).to(dev), torch.from_numpy(offs).to(dev)

    def step():
        return ops.voxelize_points(p, o, rng, cv.VOXEL_SIZE, T, cv.FULL_MAX_VOXELS)
    out = step()
    torch.cuda.synchronize()
    exact = all(torch.equal(g.cpu(), torch.from_numpy(ref[k])) for g, k in zip(out[1:], ("voxel_coords", "voxel_num_points", "num_voxels")))
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
    us_call = median(ts)

    per = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(max(20, args.steps)):
                step()
            torch.cuda.synchronize()
        for ev in prof.events():
            for k in KERNELS:
                if k + "_kernel" in ev.name:
                    per.setdefault(k, []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
    except Exception as exc:                                    # the profiler is optional: the whole-call time stands on its own
        print("per-launch times unavailable (torch.profiler: %s)" % (exc,))

    m, n = len(pts), cv.FULL_AGENTS
    cells = n * cv.FULL_GRID[0] * cv.FULL_GRID[1]
    pcap = n * cv.FULL_MAX_VOXELS
    used = int(ref["num_voxels"].sum())
    kept = int(ref["cell_count"].sum())
    in_rows = int(ref["voxel_num_points"].sum())
    nb = (m + 1023) // 1024
    # bytes each launch must move (reads + writes), 4-byte table entries
    need = {
        "voxel_clear": 12 * cells + 4 * pcap,
        "voxel_classify": 16 * m + 4 * m + 8 * kept,                            # points in, cell index out, two table atomics per kept point
        "voxel_reduce": 4 * m + 8 * used + 8 * nb,                              # cell index, first + count of the leaders' cells
        "voxel_scan": 16 * nb,
        "voxel_apply": 4 * m + 8 * used + 8 * nb + 8 * used,                    # + start and the voxel -> cell map
        "voxel_fill": 4 * m + 4 * kept + 4 * kept + 4 * kept,                   # cell index, start, fill atomic, bucket entry
        "voxel_select": 4 * pcap + 8 * used + 4 * kept + 16 * in_rows + 16 * T * used + 20 * pcap,
    }
    atomics = {"voxel_classify": 2 * kept, "voxel_fill": kept}
    total = sum(need.values())
    print("box: stream copy %.0f GB/s (read + write), %s" % (copy, torch.cuda.get_device_name(0)))
    print("shape: %d points over %d agents, %d x %d cells, T = %d, max_voxels = %d: %d voxels used of %d rows, %d points kept, %d in rows; "
          "largest cell %d points; coords / counts / num_voxels equal the restatement: %s"
          % (m, n, cv.FULL_GRID[0], cv.FULL_GRID[1], T, cv.FULL_MAX_VOXELS, used, pcap, kept, in_rows, int(ref["cell_count"].max()), exact))
    print("whole call (7 launches, eager, 20 calls per event pair):  %8.1f us   %.1f MB must move -> %.0f GB/s = %.0f %% of the stream copy"
          % (us_call, total / 1e6, total / us_call / 1e3, 100 * total / us_call / 1e3 / copy))
    for k in KERNELS:
        if k not in per:
            continue
        us = median(per[k])
        line = "  %-15s %8.1f us   %6.2f MB -> %5.0f GB/s" % (k, us, need[k] / 1e6, need[k] / us / 1e3)
        if k in atomics:
            line += "   %.2f G integer atomics/s (%d)" % (atomics[k] / us / 1e3, atomics[k])
        print(line)
    if per:
        print("  sum of the launches %8.1f us" % sum(median(per[k]) for k in KERNELS if k in per))


if __name__ == "__main__":
    main()
