#!/usr/bin/env python
"""host.MeanVFE -> host.VoxelBackBone8x -> host.HeightCompression (csrc/sparse_conv.hip) on one GPU at the grid of the reference class's
own comment: sparse shape (41, 1600, 1408), one agent, a synthetic clustered scene of about 40 k voxels (Gaussian clusters of voxels near
the ground, sigma (1.5, 4, 4) cells - no recorded cloud is part of this repository).  Per compute mode (bf16, fp32):
  * rows per level, and the share of (32-row tile, tap) pairs the convolution skips because no row of the tile has the tap - counted
    with torch from the indices the forward returns, per layer;
  * per-layer times: ops.LaunchProfile's HIP events around every C-ABI call of an eager forward, per launch family and level shape
    (layers of one shape on one level share a line), median of `--steps` forwards, with the fitted capacities;
  * the whole forward: HIP events around `--steps` eager forwards, and around replays of one captured graph of it (the device's
    time, without the host's per-call work), medians - with the default (provable) capacities and with capacities fitted to the scene
    (1.25 x the live rows), which is what sizes every launch;
  * from points: the same scene as a cloud - every voxel's 1 .. 5 points placed inside its cell, shuffled, about 120 k points -
    through host.SpVoxelPreprocessor3D (csrc/voxelize.hip's hash-table form) on the (1408, 1600, 41) grid: the voxelisation alone,
    and voxelisation -> MeanVFE -> VoxelBackBone8x -> HeightCompression as one eager forward and one captured graph.
There is nothing to compare with: spconv is not installed and the dense restatement does not fit at this size.  One JSON line, printed
and written to --out (default profiles/sparse_backbone_timing.json).
Usage (GPU box): python tools/sparse_timing.py [--steps 20] [--voxels 40000] [--out PATH]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = (1408, 1600, 40)          # (nx, ny, nz)
SLOTS, CHANNELS = 5, 4


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def scene(voxels, dev, seed=0):
    """voxel dict of one agent: unique cells of Gaussian clusters, in a random order"""
    g = torch.Generator().manual_seed(seed)
    nx, ny, nz = GRID
    clusters = max(voxels // 80, 1)
    centre = torch.stack([3 + 12 * torch.rand(clusters, generator=g), ny * torch.rand(clusters, generator=g), nx * torch.rand(clusters, generator=g)], 1)
    pts = centre[:, None, :] + torch.randn(clusters, 130, 3, generator=g) * torch.tensor([1.5, 4.0, 4.0])
    pts = pts.reshape(-1, 3).round().long()
    ok = (pts >= 0).all(1) & (pts[:, 0] <= nz) & (pts[:, 1] < ny) & (pts[:, 2] < nx)
    cells = torch.unique(pts[ok], dim=0)
    cells = cells[torch.randperm(len(cells), generator=g)][:voxels]
    coords = torch.cat([torch.zeros(len(cells), 1, dtype=torch.long), cells], 1).to(torch.int32)
    npts = torch.randint(1, SLOTS + 1, (len(cells),), generator=g, dtype=torch.int32)
    vf = torch.rand(len(cells), SLOTS, CHANNELS, generator=g) * (torch.arange(SLOTS)[None, :, None] < npts[:, None, None])
    return {"voxel_features": vf.to(dev), "voxel_num_points": npts.to(dev), "voxel_coords": coords.to(dev), "batch_size": 1}


VOXEL_SIZE = [0.05, 0.05, 0.1]
LIDAR_RANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.1]          # (1408, 1600, 41) cells: the sparse shape, whose top plane the scene may use


def cloud(data, dev, seed=1):
    """the scene's voxel dict as raw points: voxel_num_points points inside every cell, in a random order -> (points, offsets)"""
    g = torch.Generator().manual_seed(seed)
    coords, npts = data["voxel_coords"].cpu(), data["voxel_num_points"].cpu()
    cell = coords[:, [3, 2, 1]].repeat_interleave(npts.long(), 0).double()
    frac = 0.1 + 0.8 * torch.rand(len(cell), 3, generator=g, dtype=torch.float64)
    xyz = torch.tensor(LIDAR_RANGE[:3], dtype=torch.float64) + (cell + frac) * torch.tensor(VOXEL_SIZE, dtype=torch.float64)
    pts = torch.cat([xyz, torch.rand(len(cell), 1, generator=g, dtype=torch.float64)], 1).float()
    pts = pts[torch.randperm(len(pts), generator=g)].contiguous()
    return pts.to(dev), torch.tensor([0, len(pts)], dtype=torch.int32, device=dev)


def skipped_share(x_in, x_out, conv, tile):
    """share of (tile, tap) pairs of one layer without any present input row"""
    d, h, w = x_in.spatial_shape
    n_in, n_out = int(x_in.num[0]), int(x_out.num[0])
    dense = torch.zeros(x_in.batch_size * d * h * w, dtype=torch.bool, device=x_in.indices.device)
    i = x_in.indices[:n_in].long()
    dense[((i[:, 0] * d + i[:, 1]) * h + i[:, 2]) * w + i[:, 3]] = True
    o = x_out.indices[:n_out].long()
    k, s, p = conv.kernel_size, conv.stride, conv.padding
    present = []
    for kz in range(k[0]):
        for ky in range(k[1]):
            for kx in range(k[2]):
                z, y, x = o[:, 1] * s[0] - p[0] + kz, o[:, 2] * s[1] - p[1] + ky, o[:, 3] * s[2] - p[2] + kx
                ok = (z >= 0) & (z < d) & (y >= 0) & (y < h) & (x >= 0) & (x < w)
                cell = ((o[:, 0] * d + z.clamp(0, d - 1)) * h + y.clamp(0, h - 1)) * w + x.clamp(0, w - 1)
                present.append(ok & dense[cell])
    present = torch.stack(present, 1)
    pad = (-n_out) % tile
    present = torch.cat([present, present.new_zeros(pad, present.shape[1])]).view(-1, tile, present.shape[1]).any(1)
    return 1.0 - float(present.float().mean())


def train_main(args):
    """--train: host.training.mean_vfe -> voxel_backbone8x -> height_compression on the same scene with a sum-of-products loss, forward +
    backward, fp32 rows, capacities fitted to the scene (1.25 x the live rows): eager and as ONE captured graph (side stream, two warm-up
    steps, as host/train_graph.py does), median of --steps with HIP events; the fp32 inference forward of the same module measured in
    the same run with the same capacities; the per-launch split of an eager step (ops.LaunchProfile, by family and level shape).  One JSON
    line, APPENDED to the output file."""
    from cobevt_amd import autograd as ag
    from cobevt_amd import host, ops
    from cobevt_amd.host import training
    from cobevt_amd.synth import fill_module_
    if not torch.cuda.is_available():
        raise SystemExit("sparse_timing: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda")
    out_path = args.out if args.out != os.path.join(ROOT, "profiles", "sparse_backbone_timing.json") else \
        os.path.join(ROOT, "profiles", "sparse_backbone_train_timing.json")
    data = scene(args.voxels, dev)
    vfe, to_bev = host.MeanVFE({}, CHANNELS), host.HeightCompression({"feature_num": 256})
    backbone = fill_module_(host.VoxelBackBone8x({}, CHANNELS, list(GRID)), 0).to(dev)

    def timed(fn):
        ts = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return round(median(ts), 4), round(min(ts), 4), round(max(ts), 4)

    def infer():
        with torch.no_grad(), host.compute_dtype("fp32"):
            return to_bev(backbone(vfe(dict(data))))

    for mod in (vfe, backbone, to_bev):
        mod.eval()
    out = infer()
    torch.cuda.synchronize()
    levels = [out["multi_scale_3d_features"][k] for k in ("x_conv1", "x_conv2", "x_conv3", "x_conv4")] + [out["encoded_spconv_tensor"]]
    rows = [int(t.num[0]) for t in levels]
    backbone.level_capacities = [max(int(1.25 * r), 128) for r in rows]
    for _ in range(3):
        infer()
    torch.cuda.synchronize()
    infer_eager = timed(infer)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        infer()
    graph.replay()
    torch.cuda.synchronize()
    infer_graph = timed(graph.replay)
    del graph
    for mod in (vfe, backbone, to_bev):
        mod.train()
    d, h, w = backbone.level_shapes()[-1]
    weights = torch.rand((1, 128 * d, h, w), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) - 0.5

    def step():
        sf = training.height_compression(to_bev, training.voxel_backbone8x(backbone, training.mean_vfe(vfe, dict(data))))["spatial_features"]
        (sf * weights).sum().backward()

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        eager = timed(step)
        per = {}
        for _ in range(args.steps):
            with ops.LaunchProfile() as prof:
                step()
                fams = prof.summary(by_shape=True)
            for fam, v in fams.items():
                per.setdefault(fam, []).append((v["ms"], v["calls"]))
        for p in backbone.parameters():
            p.grad = None
        graph = torch.cuda.CUDAGraph()
        ag.begin_capture_zero_pool()
        try:
            with torch.cuda.graph(graph, stream=stream):
                step()
        finally:
            ag.end_capture_zero_pool()
        graph.replay()
        torch.cuda.synchronize()
        replay = timed(graph.replay)
    torch.cuda.current_stream().wait_stream(stream)
    split = {fam: {"calls": v[0][1], "ms": round(median([m for m, _ in v]), 4)} for fam, v in per.items()}
    line = {"what": "training.mean_vfe -> voxel_backbone8x -> height_compression, forward + backward, fp32 rows, sparse shape (41, 1600, 1408), "
                    "one agent, synthetic clustered scene, capacities 1.25 x the live rows; ms: median of --steps (min, max); "
                    "ms_per_family: all calls of a launch family and level shape in one eager step",
            "device": torch.cuda.get_device_name(0), "steps": args.steps, "voxels": int(data["voxel_coords"].shape[0]), "rows_per_level": rows,
            "capacities": backbone.level_capacities, "inference_fp32_ms": {"eager": infer_eager, "graph_replay": infer_graph},
            "train_step_ms": {"eager": eager, "graph_replay": replay},
            "train_graph_over_inference_graph": round(replay[0] / infer_graph[0], 2), "ms_per_family": split}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--voxels", type=int, default=40000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_backbone_timing.json"))
    ap.add_argument("--train", action="store_true", help="time one training step (forward + backward) instead; appends to "
                                                         "profiles/sparse_backbone_train_timing.json unless --out is given")
    args = ap.parse_args()
    if args.train:
        return train_main(args)
    from cobevt_amd import host, ops
    from cobevt_amd.synth import fill_module_
    if not torch.cuda.is_available():
        raise SystemExit("sparse_timing: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda")
    torch.set_grad_enabled(False)
    data = scene(args.voxels, dev)
    vfe = host.MeanVFE({}, CHANNELS).eval()
    backbone = fill_module_(host.VoxelBackBone8x({}, CHANNELS, list(GRID)), 0).eval().to(dev)
    to_bev = host.HeightCompression({"feature_num": 256}).eval()

    def forward():
        return to_bev(backbone(vfe(dict(data))))

    points, offsets = cloud(data, dev)
    voxels = int(data["voxel_coords"].shape[0])
    pre = host.SpVoxelPreprocessor3D({"cav_lidar_range": LIDAR_RANGE, "args": {"voxel_size": VOXEL_SIZE, "max_points_per_voxel": SLOTS,
                                                                              "max_voxel_train": voxels, "max_voxel_test": voxels}}, False)
    assert tuple(pre.grid_size) == (GRID[0], GRID[1], GRID[2] + 1)

    def voxelise():
        return pre.preprocess_batch(points, offsets)

    def from_points():
        return to_bev(backbone(vfe(voxelise())))

    def timed(fn):
        ts = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return round(median(ts), 4), round(min(ts), 4), round(max(ts), 4)

    line = {"what": "MeanVFE -> VoxelBackBone8x -> HeightCompression, sparse shape (41, 1600, 1408), one agent, synthetic clustered scene; "
                    "ms: median of --steps (min, max); skipped: share of (32-row tile, tap) pairs without a present input row",
            "device": torch.cuda.get_device_name(0), "steps": args.steps, "voxels": voxels, "points": int(points.shape[0]), "modes": {}}
    layers = [name for name, _, _ in backbone._layers()]
    for mode in ("bf16", "fp32"):
        res = {}
        with host.compute_dtype(mode):
            backbone.level_capacities = None
            out = forward()
            torch.cuda.synchronize()
            levels = [out["multi_scale_3d_features"][k] for k in ("x_conv1", "x_conv2", "x_conv3", "x_conv4")] + [out["encoded_spconv_tensor"]]
            res["rows_per_level"] = [int(t.num[0]) for t in levels]
            res["dropped"] = [int(t.num[1]) for t in levels]
            res["default_capacities"] = [t.capacity for t in levels]
            if mode == "bf16":
                # the inputs of the twelve layers: level 0 twice, then (previous level, own level, own level) per stage, conv_out
                ins = [levels[0], levels[0]] + [t for a, b in zip(levels[:3], levels[1:4]) for t in (a, b, b)] + [levels[3]]
                outs = [levels[0], levels[0]] + [t for b in levels[1:4] for t in (b, b, b)] + [levels[4]]
                convs = [conv for _, conv, _ in backbone._layers()]
                line["taps_skipped_per_layer"] = {n: round(skipped_share(i, o, c, ops.SPARSE_TILE_ROWS), 4)
                                                  for n, i, o, c in zip(layers, ins, outs, convs)}
            for label, caps in (("default_capacities", None), ("fitted_capacities", [max(int(1.25 * r), 128) for r in res["rows_per_level"]])):
                backbone.level_capacities = caps
                for _ in range(3):
                    forward()
                torch.cuda.synchronize()
                eager = timed(forward)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    forward()
                graph.replay()
                torch.cuda.synchronize()
                res["forward_ms_%s" % label] = {"eager": eager, "graph_replay": timed(graph.replay)}
                del graph
                torch.cuda.synchronize()
            per = {}
            for _ in range(args.steps):
                with ops.LaunchProfile() as prof:
                    forward()
                    fams = prof.summary(by_shape=True)
                for fam, d in fams.items():
                    per.setdefault(fam, []).append(d["ms"] / d["calls"])
            res["ms_per_call_fitted_capacities"] = {fam: round(median(v), 4) for fam, v in per.items()}
            backbone.level_capacities = None
            res["from_points"] = {}
            for label, fn in (("voxelize_ms", voxelise), ("forward_ms", from_points)):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                eager = timed(fn)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    fn()
                graph.replay()
                torch.cuda.synchronize()
                res["from_points"][label] = {"eager": eager, "graph_replay": timed(graph.replay)}
                del graph
                torch.cuda.synchronize()
            res["from_points"]["voxels"] = int(voxelise()["num_voxels"][0])
        line["modes"][mode] = res
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
