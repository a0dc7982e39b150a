#!/usr/bin/env python
"""ops.resize_pil_bilinear (csrc/image_ingest.hip) on one GPU at the nuScenes shape: six decoded 900 x 1600 frames -> (6, 3, 224, 480)
fp32 (resize to 270 x 480, top 46 rows cut, ToTensor), one launch.  HIP events after warm-up, `--steps` batches of `--calls` calls
between one event pair each, the median - eager (the host's per-call work included) and replayed from one captured graph of the same
`--calls` calls (the device's time, us_per_call); next to the time the bytes the call has to move (every source byte once, every output byte
once) and the rate that gives against the stream-copy bandwidth bench.box_calibration (csrc/calibrate.hip) measures in the same run.
The result is checked against the restatement tests/ingest_ref.py first.  Where Pillow is importable, the host time of the thing
replaced - Image.resize + crop of the same six frames on one core, median of `--steps` - is reported too; otherwise the line says it
was not measured.  One JSON line, printed and written to --out (default profiles/nusc_ingest_timing.json).
Usage (GPU box): python tools/ingest_timing.py [--steps 30] [--calls 20] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CAMERAS, SRC, RESIZED, TOP = 6, (900, 1600), (270, 480), 46


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nusc_ingest_timing.json"))
    args = ap.parse_args()
    import bench
    import ingest_ref as ir
    from cobevt_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("ingest_timing: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda")
    torch.set_grad_enabled(False)
    try:
        cal = bench.box_calibration(dev)
    except Exception as exc:
        cal = {"unavailable": repr(exc)}
    img = ir.make_images(0, CAMERAS, *SRC)
    x = torch.from_numpy(img).to(dev)
    size = (RESIZED[1], RESIZED[0])
    out = torch.empty(CAMERAS, 3, RESIZED[0] - TOP, RESIZED[1], device=dev)

    def step():
        ops.resize_pil_bilinear(x, size, TOP, out=out)

    step()
    torch.cuda.synchronize()
    exact = bool(np.array_equal(out[:1].cpu().numpy().view(np.int32), ir.resize(img[:1], size, TOP).view(np.int32)))
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            step()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / args.calls)
    us_eager = median(ts)
    # the same calls replayed from a captured graph: the device's time without the host's per-call work (argument checks, ctypes)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(args.calls):
            step()
    graph.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / args.calls)
    us = median(ts)
    moved = float(x.numel() + out.numel() * 4)
    line = {"what": "resize_pil_bilinear 6 x 900 x 1600 x 3 uint8 -> (6, 3, 224, 480) fp32, one launch; us_per_call: replayed from a captured graph",
            "device": torch.cuda.get_device_name(0), "steps": args.steps, "calls_per_event_pair": args.calls,
            "us_per_eager_call": round(us_eager, 2),
            "us_per_call": round(us, 2), "us_per_frame": round(us / CAMERAS, 2), "us_per_call_min": round(min(ts), 2),
            "us_per_call_max": round(max(ts), 2), "bytes_moved": moved, "achieved_gbs": round(moved / us / 1e3, 1),
            "equal_to_restatement": exact}
    if "hbm_copy_gbs" in cal:
        line["stream_copy_gbs"] = cal["hbm_copy_gbs"]
        line["share_of_stream_copy"] = round(moved / us / 1e3 / cal["hbm_copy_gbs"], 3)
    else:
        line["stream_copy_gbs"] = "not measured: %s" % cal.get("unavailable", "no hbm_copy_gbs in the calibration")
    try:
        from PIL import Image
    except Exception:
        line["pillow_host_ms_six_frames"] = "not measured here: Pillow is not importable on this machine"
    else:
        frames = [Image.fromarray(f) for f in img]
        hs = []
        for _ in range(max(args.steps // 3, 3)):
            t0 = time.perf_counter()
            for f in frames:
                r = f.resize(size, resample=Image.BILINEAR)
                np.asarray(r.crop((0, TOP, r.width, r.height)))
            hs.append((time.perf_counter() - t0) * 1e3)
        line["pillow_host_ms_six_frames"] = round(median(hs), 2)
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
