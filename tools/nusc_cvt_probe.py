#!/usr/bin/env python
"""nuScenes CVT (config/model/cvt.yaml) on one GPU: frames/s of the whole model from images (Normalize -> EfficientNet-B4 extractor
-> Encoder -> Decoder -> heads, batch 1 x 6 cameras 224 x 480) replayed from one captured graph (pipeline.CapturedCall), and the two
camera-paired cross-view attention launches with and without the key split, in the same process (ops.LaunchProfile, median over
`--reps` eager forwards).  Usage (GPU box): python tools/nusc_cvt_probe.py [--reps 20] [--steps 50] [--dtype bf16]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import cases_nusc_cvt as cc  # noqa: E402
from cobevt_amd import host, ops  # noqa: E402
from cobevt_amd.host import nuscenes as nu  # noqa: E402
from cobevt_amd.host import pipeline  # noqa: E402
from cobevt_amd.synth import fill_module_  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp32_split", "fp32_fast"])
args = ap.parse_args()
dev = torch.device("cuda")
torch.set_grad_enabled(False)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def attention_us(run, reps):
    """{launch name: median us} of the attention launches of one forward"""
    per = {}
    for _ in range(reps):
        with ops.LaunchProfile() as prof:
            run()
        for k, v in prof.summary(by_shape=True).items():
            if k.startswith("attention|"):
                per.setdefault(k, []).append(v["ms"] * 1e3 / v["calls"])
    return {k: median(v) for k, v in per.items()}


def main():
    host.set_compute_dtype(args.dtype)
    m = fill_module_(cc.build(nu, nu.EfficientNetExtractor(cc.LAYER_NAMES, *cc.IMAGE)), cc.SEED).to(dev)
    _, image, intr, ext = cc.inputs()
    batch = {"image": image.to(dev), "intrinsics": intr.to(dev), "extrinsics": ext.to(dev)}
    run = pipeline.CapturedCall(lambda im, ii, ee: m({"image": im, "intrinsics": ii, "extrinsics": ee}),
                                batch["image"], batch["intrinsics"], batch["extrinsics"])
    for _ in range(5):
        run.step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run.step()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ms = median(ts)
    print("nuScenes CVT from images (%s, captured graph): %.3f ms / frame median, %.1f frames/s" % (args.dtype, ms, 1e3 / ms))

    eager = lambda: m(batch)                                    # noqa: E731
    split = attention_us(eager, args.reps)
    nu.CrossViewAttention.key_split = False                    # the single-pass launch the OPV2V baselines run
    try:
        single = attention_us(eager, args.reps)
    finally:
        nu.CrossViewAttention.key_split = True
    for lvl, (nq, nk) in enumerate(((3750, 40320), (3750, 2520))):
        tag = " Nq%d Nk%d" % (nq, nk)
        a = [(k, v) for k, v in split.items() if tag in k]
        b = [(k, v) for k, v in single.items() if tag in k]
        for (ka, va), (kb, vb) in zip(a, b):
            print("level %d attention: %-48s %8.1f us | %-44s %8.1f us | %.2fx" % (lvl + 1, ka, va, kb, vb, vb / va))


if __name__ == "__main__":
    main()
