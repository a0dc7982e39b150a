"""Time BaseBEVBackbone's deblock stage (cobevt_deconv_nhwc: three launches into one concatenated map) and the whole backbone against
torch-ROCm's own ConvTranspose2d + BatchNorm2d + ReLU + cat / the same containers run by torch, in the same dtype, in one process:

    python tools/bev_backbone_probe.py [--batch 1 8] [--iters 50] [--rounds 5]

Standard OpenCOOD PointPillar backbone (num_filters [64, 128, 256] -> 3 x 128 channels at 128 x 128, from a 256 x 256 canvas of 64
channels).  The two sides alternate in rounds of `iters` calls between device events; the figure is the median round.  torch runs in
both memory formats (NCHW as the reference does, channels_last as its best case).  Prints one JSON line per measurement, first the
box calibration of bench.py."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cobevt_amd import host, ops  # noqa: E402
from cobevt_amd.synth import fill_module_  # noqa: E402

CFG = dict(layer_nums=[3, 5, 8], layer_strides=[2, 2, 2], num_filters=[64, 128, 256], upsample_strides=[1, 2, 4],
           num_upsample_filter=[128, 128, 128])


def timed(fns, iters, rounds):
    """fns: {name: callable} -> {name: median ms per call}; the callables alternate round by round"""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for name, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / iters)
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}, {k: [round(x, 4) for x in v] for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    try:
        import bench
        print(json.dumps({"box_calibration": bench.box_calibration(dev)}), flush=True)
    except Exception as e:      # the calibration is context, not the measurement
        print(json.dumps({"box_calibration": "unavailable: %r" % (e,)}), flush=True)
    model = fill_module_(host.BaseBEVBackbone(copy.deepcopy(CFG), 64), 0).eval().to(dev)
    for mode, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        tmodel = copy.deepcopy(model).to(dt)
        for b in a.batch:
            with host.compute_dtype(mode):
                # ---- the deblock stage alone, on level outputs of the right shapes
                torch.manual_seed(b)
                levels = [torch.rand((b, 128 >> i, 128 >> i, c), device=dev).to(dt) for i, c in enumerate(CFG["num_filters"])]
                nchw = [x.permute(0, 3, 1, 2).contiguous() for x in levels]
                clast = [x.permute(0, 3, 1, 2) for x in levels]              # NHWC memory, NCHW shape
                plans = [model._deconv_plan("d%d" % i, model.deblocks[i][0], model.deblocks[i][1]) for i in range(3)]
                cat = torch.empty((b, 128, 128, 384), device=dev, dtype=dt)

                def fused():
                    for i in range(3):
                        ops.deconv_into(levels[i], plans[i], cat, 128 * i)
                    return cat

                def torch_on(xs):
                    return lambda: torch.cat([tmodel.deblocks[i](xs[i]) for i in range(3)], dim=1)
                want = torch_on(nchw)().float()
                diff = float((fused().permute(0, 3, 1, 2).float() - want).abs().max() / want.abs().max())
                med, all_ = timed({"fused": fused, "torch_nchw": torch_on(nchw), "torch_channels_last": torch_on(clast)}, a.iters, a.rounds)
                out_bytes = cat.numel() * cat.element_size()
                print(json.dumps({"what": "deblock stage", "mode": mode, "batch": b, "ms": med, "rounds": all_, "max_rel_diff_vs_torch": diff,
                                  "fused_output_GBps": round(out_bytes / med["fused"] / 1e6, 1)}), flush=True)
                # ---- the whole backbone
                x = torch.rand((b, 256, 256, 64), device=dev).to(dt)
                x_nchw = x.permute(0, 3, 1, 2).contiguous()
                x_cl = x.permute(0, 3, 1, 2)

                def torch_backbone(t):
                    def run():
                        ups, y = [], t
                        for i in range(3):
                            y = tmodel.blocks[i](y)
                            ups.append(tmodel.deblocks[i](y))
                        return torch.cat(ups, dim=1)
                    return run
                want = torch_backbone(x_nchw)().float()
                diff = float((model.forward_nhwc(x).permute(0, 3, 1, 2).float() - want).abs().max() / want.abs().max())
                med, all_ = timed({"hip": lambda: model.forward_nhwc(x), "torch_nchw": torch_backbone(x_nchw),
                                   "torch_channels_last": torch_backbone(x_cl)}, max(a.iters // 5, 5), a.rounds)
                print(json.dumps({"what": "whole backbone", "mode": mode, "batch": b, "ms": med, "rounds": all_, "max_rel_diff_vs_torch": diff}),
                      flush=True)


if __name__ == "__main__":
    main()
