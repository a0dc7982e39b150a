#!/usr/bin/env python
"""The LiDAR detection output (csrc/detect_post.hip) on one GPU at a full-frame size: one cav, 256 x 256 x 2 = 131 072 anchors, about
2 000 of them above the score threshold and through the box filters, so the cut at 1000 applies.  Times ONE
VoxelPostprocessor.post_process_device call with HIP events (warm-up discarded, one event pair per call, median of `--steps` >= 20
calls), the same call as a graph replay, and each launch from torch.profiler's device-side kernel records (median per kernel name),
and checks the picked indices against the CPU restatement tests/detect_ref.py.
Usage (GPU box): python tools/detect_probe.py [--steps 40]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases_detect as cd  # noqa: E402
import detect_ref as dr  # noqa: E402
from cobevt_amd import host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40)
args = ap.parse_args()
dev = torch.device("cuda")
torch.set_grad_enabled(False)
GRID, HALF, CANDIDATES = (256, 256), (140.8, 140.8), 2000
KERNELS = ["det_decode", "det_select", "det_mask", "det_greedy"]


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def full_case(anchors):
    """every anchor keeps its own box, slightly moved; CANDIDATES of them carry a ladder logit above the threshold"""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    n = len(a)
    u = cd.uniform("probe.jitter", (n, 7))
    chosen = cd.permutation("probe.chosen", n)[:CANDIDATES]
    logits = -4.0 + (cd.LOGIT_THR - 0.3 + 4.0) * cd.uniform("probe.bg", (n,))
    logits[chosen] = np.linspace(cd.LOGIT_THR + 0.3, 3.0, CANDIDATES)[cd.permutation("probe.rank", CANDIDATES)]
    rm = np.concatenate([0.3 * (u[:, :3] - 0.5), 0.1 * (u[:, 3:6] - 0.5), 0.6 * (u[:, 6:] - 0.5)], axis=1)
    p = logits.reshape(GRID[0], GRID[1], 2).transpose(2, 0, 1)[None]
    r = rm.reshape(GRID[0], GRID[1], 14).transpose(2, 0, 1)[None]
    return [(np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(r, dtype=np.float32), np.asarray(anchors, dtype=np.float32),
             cd.matrix(0.05, [0.3, -0.2, 0.02], 0.002))]


def main():
    post = host.VoxelPostprocessor(cd.anchor_params(GRID, "hwl", *HALF), train=False)
    cavs = full_case(post.generate_anchor_box())
    ref = dr.post_process(cavs, cd.SCORE_THRESHOLD, cd.NMS_THRESH, "hwl", torch.float32)
    psm, rm, anchors, matrix = [torch.from_numpy(x).to(dev) for x in cavs[0]]
    data, output = {0: {"anchor_box": anchors, "transformation_matrix": matrix}}, {0: {"psm": psm, "rm": rm}}
    outs = None

    def step():
        return post.post_process_device(data, output, out=outs)
    outs = [t.clone() for t in step()]
    torch.cuda.synchronize()
    k = int(outs[3][0])
    same = k == len(ref["index"]) and np.array_equal(outs[2][:k].cpu().numpy(), ref["index"])
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(max(20, args.steps)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(10):
        graph.replay()
    torch.cuda.synchronize()
    tg = []
    for _ in range(max(20, args.steps)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        tg.append(e0.elapsed_time(e1) * 1e3)
    replay_same = all(torch.equal(a, b) for a, b in zip(outs, step()))
    per = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(20):
                step()
            torch.cuda.synchronize()
        for ev in prof.events():
            for name in KERNELS:
                if name + "_kernel" in ev.name:
                    per.setdefault(name, []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
    except Exception as exc:                                    # the profiler is optional: the whole-call time stands on its own
        print("per-launch times unavailable (torch.profiler: %s)" % (exc,))
    print("%s; %d anchors, %d candidates after the filters, %d enter NMS, %d boxes out; indices equal the restatement: %s; replay equals "
          "eager: %s" % (torch.cuda.get_device_name(0), psm.numel(), len(ref["candidates"]), min(1000, len(ref["candidates"])), k, same,
                         replay_same))
    print("one post_process_device call, eager (memset + 4 launches, one event pair per call, median of %d): %8.1f us  (min %.1f, max %.1f)"
          % (len(ts), median(ts), min(ts), max(ts)))
    print("the same call as a graph replay (median of %d):                                              %8.1f us  (min %.1f, max %.1f)"
          % (len(tg), median(tg), min(tg), max(tg)))
    for name in KERNELS:
        if name in per:
            print("  %-12s %8.1f us" % (name, median(per[name])))
    if per:
        print("  sum of the launches %8.1f us" % sum(median(per[n]) for n in KERNELS if n in per))
    del graph
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
