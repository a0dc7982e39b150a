"""Time BaseBEVBackbone's deblock stage (cobevt_deconv_nhwc: three launches into one concatenated map) and the whole backbone against
torch-ROCm's own ConvTranspose2d + BatchNorm2d + ReLU + cat / the same containers run by torch, in the same dtype, in one process:

    python tools/bev_backbone_probe.py [--batch 1 8] [--iters 50] [--rounds 5]

Standard OpenCOOD PointPillar backbone (num_filters [64, 128, 256] -> 3 x 128 channels at 128 x 128, from a 256 x 256 canvas of 64
channels).  The two sides alternate in rounds of `iters` calls between device events; the figure is the median round.  torch runs in
both memory formats (NCHW as the reference does, channels_last as its best case).  Prints one JSON line per measurement, first the
box calibration of bench.py.

    python tools/bev_backbone_probe.py --train [--out profiles/detector_train_timing.json]

times the training path instead (fp32, device events, median of 20 single calls): one forward + backward of the standard backbone at
B = 1 through host.training.base_bev_backbone against torch's autograd on the same containers; cobevt_deconv_wgrad against
cobevt_conv_wgrad with the roles swapped (autograd.USE_DECONV_WGRAD = False) at the three standard deblock shapes; and
cobevt_att_fuse_bwd_nhwc in GB/s of (2 N + B) HW C floats at OPV2V's three levels (5 agents in one sample).  Also the eval forward
of the backbone (fp32), for comparison across commits.  The chunk counts and grids are untuned."""
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


def median_ms(f, n=20):
    """median of n single calls between device events, after three warm-up calls"""
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(statistics.median(ms), 4), [round(min(ms), 4), round(max(ms), 4)]


def train(dev, out_path):
    from cobevt_amd import autograd as ag
    from cobevt_amd.host import training
    res = {}
    try:
        import bench
        res["box_calibration"] = bench.box_calibration(dev)
    except Exception as e:
        res["box_calibration"] = "unavailable: %r" % (e,)
    model = fill_module_(host.BaseBEVBackbone(copy.deepcopy(CFG), 64), 0).to(dev)
    torch.manual_seed(0)
    x = torch.rand((1, 64, 256, 256), device=dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), host.compute_dtype("fp32"):
        model.eval()
        res["eval_forward_fp32_ms"] = median_ms(lambda: model.forward_nhwc(x.permute(0, 2, 3, 1)))
    model.train()
    tmodel = copy.deepcopy(model)

    def hip_step():
        model.zero_grad(set_to_none=True)
        training.base_bev_backbone(model, x).sum().backward()

    def torch_step(t):
        def run():
            tmodel.zero_grad(set_to_none=True)
            ups, y = [], t
            for i in range(3):
                y = tmodel.blocks[i](y)
                ups.append(tmodel.deblocks[i](y))
            torch.cat(ups, dim=1).sum().backward()
        return run
    with torch.enable_grad():
        res["backbone_fwd_bwd_ms"] = {"hip": median_ms(hip_step), "torch_channels_last": median_ms(torch_step(x)),
                                      "torch_nchw": median_ms(torch_step(x.contiguous()))}
    res["deconv_wgrad_ms"] = []
    for i, (cin, s) in enumerate(zip(CFG["num_filters"], CFG["upsample_strides"])):
        hw = 128 >> i
        xi, dz = torch.rand((1, hw, hw, cin), device=dev), torch.rand((1, hw * s, hw * s, 128), device=dev)
        dw = torch.zeros((cin, 128, s, s), device=dev)

        def atomics():
            dw.zero_()
            ag._launch_conv_wgrad(dz, xi, dw, s, s, 0)
        new = ops.deconv_wgrad(xi, dz, s)
        atomics()
        res["deconv_wgrad_ms"].append({"s": s, "cin": cin, "cout": 128, "pixels": hw * hw, "chunks": ops.deconv_wgrad_chunks(1, hw, hw, cin, 128, s),
                                       "chunked": median_ms(lambda: ops.deconv_wgrad(xi, dz, s)), "atomics_with_zero_fill": median_ms(atomics),
                                       "max_rel_diff": float((new - dw).abs().max() / dw.abs().max())})
    res["att_fuse_bwd"] = []
    rl = torch.tensor([5], dtype=torch.int32, device=dev)
    for c, h, w in ((64, 100, 352), (128, 50, 176), (256, 25, 88)):
        xa, g = torch.rand((5, h, w, c), device=dev) - 0.5, torch.rand((1, h, w, c), device=dev) - 0.5
        ms = median_ms(lambda: ops.att_fuse_bwd(xa, rl, g))
        res["att_fuse_bwd"].append({"C": c, "H": h, "W": w, "ms": ms, "GBps": round((2 * 5 + 1) * h * w * c * 4 / ms[0] / 1e6, 1)})
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--train", action="store_true", help="time the training path (see the module docstring)")
    ap.add_argument("--out", default=None, help="--train: also write the result as JSON to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.train:
        return train(dev, a.out)
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
