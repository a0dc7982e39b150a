#!/usr/bin/env python
"""LiDAR pillar front end on one GPU, at the size of the LiDAR benchmark leg: 8 agents x 256 x 256 cells, T = 32, 60 000 pillars
(uneven over the agents), bf16 by default.  Times, each as one captured graph (pipeline.CapturedCall), 20 replays back to back between one pair of HIP
events, median over `--steps` such batches:
  * the front end alone (cobevt_pillar_vfe: the canvas clear + the row pass), and the clear alone (the same canvas, no pillars);
  * front end + FuseBEVT (PointPillarFuseBEVT.forward with bench.py's LIDAR_ARGS encoder), and that encoder alone on the canvas;
  * for comparison, the restatement (tests/pillar_ref.py) run as torch ops on the same GPU, eager.
The front end's bytes moved / time is set against the stream-copy bandwidth bench.box_calibration measures in the same run.
--train: the train-mode front end (csrc/train_pillar.hip) at the same shape in fp32 instead - the statistics pass, the forward and the
backward each as its own captured graph, and the torch restatement's (tests/pillar_train_ref.py) forward + backward on the same GPU.
Usage (GPU box): python tools/pillar_probe.py [--steps 20] [--dtype bf16] [--train]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import cases_pillar as cp  # noqa: E402
import pillar_ref as pr  # noqa: E402
import pillar_train_ref as ptr  # noqa: E402
from cobevt_amd import autograd as ag  # noqa: E402
from cobevt_amd import host, ops  # noqa: E402
from cobevt_amd.host import pipeline  # noqa: E402
from cobevt_amd.synth import fill_module_  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
ap.add_argument("--train", action="store_true", help="time the train-mode statistics pass, forward and backward instead")
args = ap.parse_args()
dev = torch.device("cuda")
torch.set_grad_enabled(False)

COUNTS = [12000, 9000, 8000, 7500, 7000, 6500, 5500, 4500]
GRID = (256, 256)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def timed(step, steps, warm=5, batch=20):
    """us per call: `batch` calls back to back between ONE event pair (a replay of a 30-80 us graph is too short for a pair of its
    own: the launch gap would be a sizeable share), median over `steps` batches"""
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            step()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / batch)
    return median(ts)


def main():
    host.set_compute_dtype(args.dtype)
    dt = host.get_compute_dtype()
    cal = bench.box_calibration(dev)
    margs = cp.model_args(grid=GRID, max_cav=8, fusion=dict(bench.LIDAR_ARGS))
    m = fill_module_(host.PointPillarFuseBEVT(margs), 0).eval().to(dev)
    vox = {k: v.to(dev) for k, v in cp.voxels(counts=COUNTS, grid=GRID, stride=40503, tag="full").items()}
    rl = torch.tensor([8], dtype=torch.int32, device=dev)
    vf, coords, npts = vox["voxel_features"], vox["voxel_coords"], vox["voxel_num_points"]
    p, t = vf.shape[:2]

    def batch(a, b, c, r):
        return {"processed_lidar": {"voxel_features": a, "voxel_coords": b, "voxel_num_points": c}, "record_len": r}
    front = pipeline.CapturedCall(lambda a, b, c, r: m.front_end(batch(a, b, c, r)), vf, coords, npts, rl)
    canvas, cav = front.step()
    clear = pipeline.CapturedCall(lambda a, b, c, r: m.front_end(batch(a, b, c, r)), vf[:0], coords[:0], npts[:0], rl)
    whole = pipeline.CapturedCall(lambda a, b, c, r: m(batch(a, b, c, r))["fused_feature"], vf, coords, npts, rl)
    com = cav[:, None, None, None, :].expand(1, GRID[0], GRID[1], 1, 8).contiguous()
    fuse = pipeline.CapturedCall(lambda x, k: m.fusion_net.forward_blhwc(x, k), canvas, com)
    us_front, us_clear = timed(front.step, args.steps), timed(clear.step, args.steps)
    us_whole, us_fuse = timed(whole.step, args.steps), timed(fuse.step, args.steps)

    w, s = m.pillar_vfe.pfn_layers[0].folded()
    g = m.pillar_vfe.geom()

    def torch_ops():
        return pr.canvas(vf, npts, coords, w, s, g, GRID[0], GRID[1], [8], 8)
    ref, _ = torch_ops()
    us_torch = timed(torch_ops, max(5, args.steps // 5), warm=2, batch=1)
    err = float((canvas.float() - ref).abs().max() / ref.abs().max())

    canvas_bytes = canvas.numel() * canvas.element_size()
    row_bytes = p * ops.PILLAR_CHANNELS * canvas.element_size()
    moved = 16 * p * t + 20 * p + canvas_bytes + row_bytes
    copy = cal["hbm_copy_gbs"]
    print("box: stream copy %.0f GB/s (read + write), %s" % (copy, torch.cuda.get_device_name(0)))
    print("shape: %d pillars x T = %d over 8 agents (%s), canvas (1, 8, %d, %d, 64) %s = %.1f MB, voxels %.1f MB"
          % (p, t, "/".join(str(c) for c in COUNTS), GRID[0], GRID[1], args.dtype, canvas_bytes / 1e6, 16 * p * t / 1e6))
    print("front end (clear + rows, one graph):      %8.1f us   %.1f MB moved -> %.0f GB/s = %.0f %% of the stream copy"
          % (us_front, moved / 1e6, moved / us_front / 1e3, 100 * moved / us_front / 1e3 / copy))
    print("  zero fill: clear launch alone           %8.1f us   %.1f MB -> %.0f GB/s written (the only zero-fill variant built)"
          % (us_clear, canvas_bytes / 1e6, canvas_bytes / us_clear / 1e3))
    print("  row pass (front end - clear)            %8.1f us   %.1f MB read + %.1f MB written, %.2f GFLOP"
          % (us_front - us_clear, (16 * p * t + 20 * p) / 1e6, row_bytes / 1e6, 2.0 * p * t * 10 * 64 / 1e9))
    print("front end + FuseBEVT (one graph):         %8.1f us   = %.1f frames/s" % (us_whole, 1e6 / us_whole))
    print("FuseBEVT alone on the canvas (one graph): %8.1f us   -> the front end is %.1f %% of the LiDAR frame"
          % (us_fuse, 100 * us_front / us_whole))
    print("restatement as torch ops on this GPU:     %8.1f us   (eager, fp32; %.0fx the operator); max-rel of the operator against it %.2e"
          % (us_torch, us_torch / us_front, err))


def train():
    host.set_compute_dtype("fp32")
    margs = cp.model_args(grid=GRID, max_cav=8, fusion=dict(bench.LIDAR_ARGS))
    m = fill_module_(host.PointPillarFuseBEVT(margs), 0).train().to(dev)
    vox = {k: v.to(dev) for k, v in cp.voxels(counts=COUNTS, grid=GRID, stride=40503, tag="full").items()}
    rl = torch.tensor([8], dtype=torch.int32, device=dev)
    vf, coords, npts = vox["voxel_features"], vox["voxel_coords"], vox["voxel_num_points"]
    p, t = vf.shape[:2]
    vfe, pfn = m.pillar_vfe, m.pillar_vfe.pfn_layers[0]
    cfg = (vfe.geom(), vfe.use_absolute_xyz, vfe.with_distance, GRID, 8, None)

    def stats(a, b, c, r):
        return ag.pillar_train_stats(pfn.linear.weight, pfn.norm.weight, pfn.norm.bias, a, c, b, r, pfn.norm, cfg)
    state = stats(vf, coords, npts, rl)
    canvas, _ = ag.pillar_train_forward(state, cfg)
    dcanvas = torch.randn(canvas.shape, device=dev, generator=torch.Generator(dev).manual_seed(0))
    bwd_args = (state["dims"], state["geom"], state["mode"], state["n_bwd"], state["k"], True, True)
    g_stats = pipeline.CapturedCall(lambda a, b, c, r: stats(a, b, c, r)["tensors"][6], vf, coords, npts, rl)
    g_fwd = pipeline.CapturedCall(lambda w_, s_: ag.pillar_train_forward(dict(state, tensors=state["tensors"][:6] + (w_, s_)), cfg)[0],
                                  state["tensors"][6], state["tensors"][7])
    g_bwd = pipeline.CapturedCall(lambda d: ag.pillar_train_backward(state["tensors"], *bwd_args, d)[0], dcanvas)
    us_stats, us_fwd, us_bwd = timed(g_stats.step, args.steps), timed(g_fwd.step, args.steps), timed(g_bwd.step, args.steps)

    # the torch restatement, forward + backward, eager fp32 on this GPU; and the operator's step against it
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}

    def torch_step():
        prm = ptr.params(sd, "pillar_vfe.pfn_layers.0.", True)
        with torch.enable_grad():
            x, _ = ptr.canvas(prm, vf, npts, coords, cfg[0], GRID[0], GRID[1], [8], 8)
            (x * dcanvas).sum().backward()
        return x.detach(), prm
    ref, prm = torch_step()
    us_torch = timed(torch_step, max(3, args.steps // 5), warm=1, batch=1)
    dw = ag.pillar_train_backward(state["tensors"], *bwd_args, dcanvas)[0]
    torch.cuda.synchronize()
    e_fwd = float((canvas - ref).abs().max() / ref.abs().max())
    e_dw = float((dw - prm["linear.weight"].grad).abs().max() / prm["linear.weight"].grad.abs().max())
    total = us_stats + us_fwd + us_bwd
    print("box: %s" % torch.cuda.get_device_name(0))
    print("shape: %d pillars x T = %d over 8 agents, canvas (1, 8, %d, %d, 64) fp32 = %.1f MB, voxels %.1f MB; train mode, batch statistics"
          % (p, t, GRID[0], GRID[1], canvas.numel() * 4 / 1e6, 16 * p * t / 1e6))
    print("statistics pass (compaction + fp64 sums + finish, one graph): %8.1f us   one %.1f MB read" % (us_stats, 16 * p * t / 1e6))
    print("forward (the inference operator on the folded operands, fp32): %7.1f us" % us_fwd)
    print("backward (recompute + winners + partials, finish, one graph): %8.1f us" % us_bwd)
    print("training front end, sum of the three:                         %8.1f us" % total)
    print("restatement forward + backward as torch ops on this GPU:      %8.1f us   (eager, fp32; %.0fx); operator against it: "
          "forward max-rel %.2e, d linear.weight %.2e" % (us_torch, us_torch / total, e_fwd, e_dw))


if __name__ == "__main__":
    if args.train:
        torch.set_grad_enabled(False)
        train()
    else:
        main()
