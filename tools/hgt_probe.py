"""Time one PreNorm(HGTCavAttention) + x layer (three launches: csrc/att_fuse.hip) against torch-ROCm running the vectorised restatement
of the reference's procedure (tests/hgt_ref.layer_restatement: no Python loop over agents, no host read - what the reference itself
does is slower still) on the same device, in the same storage dtype, in one process:

    python tools/hgt_probe.py [--iters 20] [--rounds 7] [--out profiles/hgt_timing.json]

Two sizes, T = 2, mixed types, padded agents masked: dim 128 / 8 heads / L = 5 / 32 x 32 (the fusion size of cvt_att_fuse.yaml) and
dim 256 / 8 heads / L = 5 / 48 x 176.  The sides alternate in rounds of `iters` calls between device events after a warm-up; the
figure is the median round, all rounds are kept.  Each side's outputs are compared once (max abs difference, next to max |out|)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cobevt_amd import host  # noqa: E402
from cobevt_amd.host import runtime as rt  # noqa: E402
import hgt_ref as hr  # noqa: E402

SIZES = [dict(dim=128, heads=8, L=5, H=32, W=32), dict(dim=256, heads=8, L=5, H=48, W=176)]
T = 2


def timed(fns, iters, rounds):
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    results = []
    for s in SIZES:
        dim, heads, L, H, W = s["dim"], s["heads"], s["L"], s["H"], s["W"]
        layer = hr.fill_hgt_(host.PreNorm(dim, host.HGTCavAttention(dim, heads, num_types=T, num_relations=T * T, dim_head=32)), 0).eval().to(dev)
        x32 = hr.procedural_input("hgt.probe.x%d" % dim, (1, L, H, W, dim), 0, -2.0, 2.0).to(dev)
        types = hr.make_types("mixed", 1, L, T)
        prior = torch.zeros(1, L, H, W, 3)
        prior[..., 2] = types.float()[:, :, None, None]
        prior = prior.to(dev)
        mask = hr.make_mask("padded", 1, L, H, W).to(dev)
        for mode, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
            with host.compute_dtype(mode):
                x, prior_dt = x32.to(dt), prior.to(dt)
                sd = {k: v.detach().to(dt) for k, v in layer.fn.state_dict().items()}
                ln = hr.LN(layer.norm.weight.detach().to(dt), layer.norm.bias.detach().to(dt), layer.norm.eps)
                ours = lambda: layer.fn.forward_fused(x, residual=x, ln=layer.norm, mask=mask, prior_encoding=prior)          # noqa: E731
                theirs = lambda: hr.layer_restatement(sd, ln, x, mask, prior_dt, heads)                                       # noqa: E731
                diff = float((ours().float() - theirs().float()).abs().max())
                med, rounds = timed({"hip": ours, "torch": theirs}, a.iters, a.rounds)
                rec = dict(s, T=T, mode=mode, ms=med, rounds=rounds, torch_over_hip=round(med["torch"] / med["hip"], 2), max_abs_diff=diff,
                           max_abs_out=float(ours().float().abs().max()))
                print(json.dumps(rec), flush=True)
                results.append(rec)
        del layer
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "one PreNorm(HGTCavAttention) + x layer, three HIP launches, against torch-ROCm on the vectorised restatement",
                       "device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds, "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
