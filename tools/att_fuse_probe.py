"""Time AttBEVBackbone's agent fusion (cobevt_att_fuse_nhwc) against the reference's AttFusion composed from torch-ROCm ops on the same
device, in the same dtype, in one process:

    python tools/att_fuse_probe.py [--batch 1 4] [--iters 50] [--rounds 5]

OPV2V's PointPillar shapes: 5 agents per sample, levels of 64 x 100 x 352, 128 x 50 x 176 and 256 x 25 x 88.  Three measurements per
dtype and batch: ops.att_fuse alone per level (with the bytes the op has to move, n C in + C out per pixel, over its time, next to
the box's stream-copy rate from bench.box_calibration); the three-level fuse + deblock stage (three att_fuse and three deconv_into
launches into the one 384-channel map); and torch's composition of the same fusion (per sample: view, permute, bmm, / sqrt(C), softmax,
bmm, permute, row 0 - on NCHW maps as the reference holds them, with record_len already on the host, which spares torch the
reference's own synchronisation).  The sides alternate in rounds of `iters` calls between device events; the figure is the median
round.  Every call of a level reads the next of several input copies (more than 512 MB together), so no side finds its input in the
last-level cache.  Prints one JSON line per measurement, first the box calibration."""
import argparse
import copy
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cobevt_amd import host, ops  # noqa: E402
from cobevt_amd.synth import fill_module_  # noqa: E402

AGENTS = 5
LEVELS = [(64, 100, 352), (128, 50, 176), (256, 25, 88)]
CFG = dict(layer_nums=[3, 5, 8], layer_strides=[2, 2, 2], num_filters=[64, 128, 256], upsample_strides=[1, 2, 4],
           num_upsample_filter=[128, 128, 128])
FOOTPRINT = 512 << 20


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


def torch_att_fusion(x, record_len):
    """the reference's AttFusion.forward (self_attn.py:41-52) on (N, C, H, W), record_len a host list"""
    c, h, w = x.shape[1:]
    out, off = [], 0
    for n in record_len:
        xx = x[off:off + n].view(n, c, -1).permute(2, 0, 1)
        score = torch.bmm(xx, xx.transpose(1, 2)) / math.sqrt(c)
        ctx = torch.bmm(torch.softmax(score, -1), xx)
        out.append(ctx.permute(1, 2, 0).view(n, c, h, w)[0:1])
        off += n
    return torch.cat(out, dim=0)


class Rotating(object):
    """hands out the next of several equal tensors per call"""

    def __init__(self, make, nbytes):
        self.items = [make(i) for i in range(max(2, -(-FOOTPRINT // nbytes)))]
        self.i = 0

    def next(self):
        self.i = (self.i + 1) % len(self.items)
        return self.items[self.i]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 4])
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
    model = fill_module_(host.AttBEVBackbone(copy.deepcopy(CFG), 64), 0).eval().to(dev)
    for mode, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        esz = 2 if dt == torch.bfloat16 else 4
        for b in a.batch:
            n = AGENTS * b
            rl_host = [AGENTS] * b
            rl = torch.tensor(rl_host, dtype=torch.int32, device=dev)
            with host.compute_dtype(mode):
                # ---- the fusion alone, level by level
                for c, h, w in LEVELS:
                    nbytes = n * h * w * c * esz
                    gen = torch.Generator(device=dev).manual_seed(c + b)
                    nhwc = Rotating(lambda i: (torch.rand((n, h, w, c), device=dev, generator=gen) * 2 - 1).to(dt), nbytes)
                    nchw = Rotating(lambda i: nhwc.items[i].permute(0, 3, 1, 2).contiguous(), nbytes)
                    out = torch.empty((b, h, w, c), device=dev, dtype=dt)
                    want = torch_att_fusion(nchw.items[0], rl_host).float()
                    got = ops.att_fuse(nhwc.items[0], rl).permute(0, 3, 1, 2).float()
                    diff = float((got - want).abs().max() / want.abs().max())
                    med, all_ = timed({"att_fuse": lambda: ops.att_fuse(nhwc.next(), rl, out=out),
                                       "torch": lambda: torch_att_fusion(nchw.next(), rl_host)}, a.iters, a.rounds)
                    moved = (n + b) * h * w * c * esz
                    print(json.dumps({"what": "att_fuse alone", "mode": mode, "batch": b, "level": [c, h, w], "ms": med, "rounds": all_,
                                      "max_rel_diff_vs_torch": diff, "bytes_moved": moved,
                                      "att_fuse_GBps": round(moved / med["att_fuse"] / 1e6, 1),
                                      "torch_over_att_fuse": round(med["torch"] / med["att_fuse"], 2)}), flush=True)
                    del nhwc, nchw
                # ---- the three-level fuse + deblock stage
                torch.manual_seed(b)
                levels = [(torch.rand((n, h, w, c), device=dev) * 2 - 1).to(dt) for c, h, w in LEVELS]
                plans = [model._deconv_plan("d%d" % i, model.deblocks[i][0], model.deblocks[i][1]) for i in range(3)]
                cat = torch.empty((b, 100, 352, 384), device=dev, dtype=dt)
                tmodel = copy.deepcopy(model).to(dt)
                nchw = [x.permute(0, 3, 1, 2).contiguous() for x in levels]

                def fused():
                    for i in range(3):
                        ops.deconv_into(ops.att_fuse(levels[i], rl), plans[i], cat, 128 * i)
                    return cat

                def torch_stage():
                    return torch.cat([tmodel.deblocks[i](torch_att_fusion(nchw[i], rl_host)) for i in range(3)], dim=1)
                want = torch_stage().float()
                diff = float((fused().permute(0, 3, 1, 2).float() - want).abs().max() / want.abs().max())
                med, all_ = timed({"hip": fused, "torch": torch_stage}, max(a.iters // 2, 5), a.rounds)
                print(json.dumps({"what": "fuse + deblock stage", "mode": mode, "batch": b, "ms": med, "rounds": all_,
                                  "max_rel_diff_vs_torch": diff, "torch_over_hip": round(med["torch"] / med["hip"], 2)}), flush=True)
                del levels, nchw, cat, tmodel


if __name__ == "__main__":
    main()
