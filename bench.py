#!/usr/bin/env python
"""bench.py — BEV frames/s of the MI355X-native CoBEVT hot path on synthetic OPV2V-shaped inputs.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dtype bf16|fp32] [--agents 5] [--workload camera|lidar]
                    [--mode throughput|latency] [--frames-in-flight 3|4|1] [--no-graph] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

`--workload camera` (default; the configuration BASELINE.json's metric is quoted on): one "step" = one full CorpBEVT forward
per GPU: `agents` x 4 cameras x 512x512 fp32 images (resident in HBM) -> ResNet-34 -> FAX pyramid -> [all-gather of agent
features] -> STTF -> swap fusion -> decoder -> 256x256 logits, through cobevt_amd.host.pipeline (HIP graphs, three frames
in flight).  N > 1: the headline is the same quantity ("throughput" mode, "weak" scaling): N frames per step, the N*agents
agent tasks dealt round-robin over the ranks and exchanged ONCE before fusion; value = N frames / step time, so
value_N / (N x value_1) is the agent-shard scaling efficiency.  With --full the line carries `latency_mode` ("strong" scaling, the
north-star's partition): ONE frame per step, rank r encodes agents r, r+N, .., one all-gather, fusion replicated, with its
`frame_latency_ms`; `--mode latency` makes that the headline.
`--workload lidar` (BASELINE configs[4]): one step = SwapFusionEncoder(64 ch, 8 agents, window 8, depth 3, mask) on
x (1, 8, 64, 256, 256); N > 1 throughput = one frame per rank (replicas), latency = the map row-sharded over the ranks with
an all-to-all between the window and grid halves of every block (cobevt_amd/dist.py).
Rank 0 prints ONE JSON line.  Timing: W warm-up steps, then K steps between barrier + synchronize, MAX over ranks; the per-step
median / p95 come from HIP events recorded after every step.  `--dump-outputs DIR`: what the timed path returned from its last
step, one DIR/<name>.npy per output tensor (float32; the inputs and weights are seeded, so two builds compare output for output).

A plain run sets up, warms up, times the K steps and prints the line.  `--full` adds everything else: the correctness checks of
the timed runner against the un-pipelined / single-process forward, `box_calibration`, the latency-mode / exchange /
single-GPU-reference legs at N > 1, the LiDAR roofline, and these extra legs at N = 1 (rank 0): `one_frame_at_a_time`, `eager_model_call` (the plain `model(batch)` a drop-in user calls),
`fp32_parity_mode` (same frame in the exact-fp32 mode), `other_configs` (the captured bf16 training step of the same model and frame, 2-agent OPV2V, nuScenes SinBEVT, LiDAR FuseBEVT), `roofline` (+ the
level-0 FAX attention launch on its own) from HIP-event timings of one eager frame and the committed rocprofv3 PMC summary
(profiles/pmc_*.json), `cpu_baseline` (the oracle on the host cores, kind "port") and `parity` against it.
"""
import argparse
import copy
import glob
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cobevt_amd import dist as cdist  # noqa: E402
from cobevt_amd import host, ops, synth  # noqa: E402
from cobevt_amd.host import pipeline  # noqa: E402

PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3}     # dense MFMA peaks, /opt/skills/guides/MI355X_MICROARCH.md
# algorithmic FLOPs per frame (SURVEY.md §8a ledger, de-duplicated query replicas): per agent ResNet-34 x4 cams
# 153.1 GF + FAX 34.65 GF; per frame fusion 13.12 GF + decoder/head 5.21 GF
GF_PER_AGENT, GF_PER_FRAME = 153.1 + 34.65, 13.12 + 5.21
LIDAR_GF = 619.0                                  # SwapFusionEncoder on (1, 8, 64, 256, 256) as implemented
LIDAR_ARGS = dict(input_dim=64, mlp_dim=128, agent_size=8, window_size=8, dim_head=32, drop_out=0.1, depth=3, mask=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)     # SURVEY.md §8d protocol: 50 warm-up, 200 timed, median and p95
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--workload", default="camera", choices=["camera", "lidar"])
    ap.add_argument("--mode", default=None, choices=["throughput", "latency", "both"],
                    help="N > 1: throughput = N frames in flight, their agents dealt over the GPUs + one exchange (weak scaling; the "
                         "same quantity as the N = 1 headline), latency = ONE frame over N GPUs, one agent per GPU + one all-gather "
                         "(strong scaling; BASELINE.json's partitioning), both (default at N > 1) = throughput as the headline `value` "
                         "with `latency_mode` (frame_latency_ms) in the same JSON line.  N = 1: throughput")
    ap.add_argument("--gather", default="rccl", choices=["rccl", "direct"],
                    help="latency mode: the agent all-gather through RCCL (torch.distributed, default) or the one-shot direct "
                         "peer-window exchange over xGMI (csrc/peer_gather.hip); the other one is reported next to it")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying captured HIP graphs")
    ap.add_argument("--frames-in-flight", type=int, default=3, choices=[1, 3, 4],
                    help="single-GPU software pipeline: 3 = encoder / FAX query / fusion+decoder of three consecutive frames "
                         "overlap on three HIP streams (throughput mode, default); 1 = one frame at a time")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beside the headline: correctness checks of the timed runner, box calibration, the "
                         "one-frame / eager / ingest / other-precision / other-config legs, roofline, CPU baseline and parity at N = 1; "
                         "the latency-mode, exchange and single-GPU reference legs at N > 1.  Off: set up, warm up, time, print")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned from its last step as DIR/<name>.npy "
                         "(float32, float64 kept; at most 64 MB in all, a fixed seeded sample of larger outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline and parity legs")
    ap.add_argument("--no-roofline", action="store_true", help="--full: skip the roofline legs")
    ap.add_argument("--no-extra", action="store_true", help="--full: skip the eager / fp32 / other-config legs")
    ap.add_argument("--no-ingest", action="store_true", help="--full: skip the host-to-device ingest leg (`ingest`, `value_with_h2d`)")
    ap.add_argument("--direct-probe", action="store_true", help=argparse.SUPPRESS)   # the isolated child job of direct_probe_child()
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


# ----------------------------------------------------------------------------------------------
# timing
# ----------------------------------------------------------------------------------------------
def timed_loop(step, warmup, steps, world, dev, keep=None):
    """W warm-up steps, then exactly K steps between barrier + synchronize; MAX over ranks.  Returns (elapsed seconds,
    per-step milliseconds from HIP events recorded after each step).  keep: a list that receives host copies of what the last
    timed step returned (host_arrays), made after the clock has stopped."""
    for _ in range(warmup):
        step()
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    events = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    events[0].record()
    for i in range(steps):
        out = step()
        events[i + 1].record()
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    elapsed = time.perf_counter() - t0
    if keep is not None:
        keep.append(host_arrays(out))
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = t.item()
    per = sorted(events[i].elapsed_time(events[i + 1]) for i in range(steps))
    return elapsed, per


def host_arrays(out, name="output"):
    """what a step returned -> {name: numpy array}: the tensors of a dict by key, of a tuple / list by position, a lone tensor as
    `output`; float64 stays float64, every other dtype becomes float32"""
    if out is None:
        raise RuntimeError("the timed step returned no output (a pipelined runner that has not filled yet)")
    if torch.is_tensor(out):
        t = out.detach()
        return {name: (t.double() if t.dtype == torch.float64 else t.float()).cpu().numpy()}
    if isinstance(out, dict):
        items = [(str(k), v) for k, v in out.items()]
    elif isinstance(out, (tuple, list)):
        items = [("%s_%d" % (name, i), v) for i, v in enumerate(out)]
    else:
        return {}
    res = {}
    for k, v in items:
        if torch.is_tensor(v) or isinstance(v, (dict, tuple, list)):
            res.update(host_arrays(v, k))
    return res


def dump_outputs(arrays, dirname, limit=64 << 20):
    """DIR/<name>.npy for every array.  If they hold more than `limit` bytes in all, each is replaced by the same share of its
    flattened elements, picked by numpy.random.default_rng(0) and kept in index order: the same sample on every run"""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    for k, a in sorted(arrays.items()):
        if total > limit:
            n = a.size
            m = max(1, int(n * (limit / float(total))))
            idx = np.sort(np.random.default_rng(0).choice(n, size=m, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, k.replace(os.sep, "_") + ".npy"), a)
    return sorted(arrays)


def pct(sorted_ms, q):
    return sorted_ms[min(len(sorted_ms) - 1, int(round(q * (len(sorted_ms) - 1))))]


def safe(result, key, fn):
    """side legs must never cost the main measurement: record the error instead"""
    try:
        result[key] = fn()
    except Exception as e:  # noqa: BLE001
        result[key] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
        torch.cuda.synchronize()


def quick(step, warmup=3, steps=20):
    """small timed loop for the side legs -> {ms_median, ms_p95, frames_per_sec (1 / median)}"""
    _, per = timed_loop(step, warmup, steps, 1, None)
    med = pct(per, 0.5)
    return {"ms_median": round(med, 4), "ms_p95": round(pct(per, 0.95), 4), "frames_per_sec": round(1e3 / med, 2), "steps": steps}


# ----------------------------------------------------------------------------------------------
# box calibration
# ----------------------------------------------------------------------------------------------
def box_calibration(dev):
    """What THIS box delivers, measured in-process in ~100 ms (csrc/calibrate.hip): the dense issue rate of
    v_mfma_f32_32x32x16_bf16 (four waves per SIMD, no operand traffic), the shader clock under that load, and an HBM stream copy.
    Boxes of the pool differ by +-6..10 %: with these three numbers in the line a roofline fraction can be normalised by the
    box it was measured on, and a few-% frames/s difference between two runs can be attributed."""
    import ctypes
    from cobevt_amd import lib as L
    lib = L.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    blocks, iters = 1024, 16000
    out = torch.empty(blocks * 256, device=dev, dtype=torch.float32)
    clk = torch.zeros(2, device=dev, dtype=torch.int64)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for _ in range(3):
        e0.record()
        L.check(lib.cobevt_calibrate_mfma(ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(clk.data_ptr()), blocks, iters, stream),
                "cobevt_calibrate_mfma")
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if best is None or ms < best[0]:
            best = (ms, [int(v) for v in clk.tolist()])
    flops = blocks * 4 * iters * 4 * 2.0 * 32 * 32 * 16
    wall, smax = ctypes.c_int(), ctypes.c_int()
    L.check(lib.cobevt_calibrate_clock_khz(ctypes.byref(wall), ctypes.byref(smax)), "cobevt_calibrate_clock_khz")
    sclk = best[1][0] / max(1, best[1][1]) * wall.value / 1e3
    n = 1 << 30
    src = torch.empty(n, device=dev, dtype=torch.uint8).fill_(1)
    dst = torch.empty(n, device=dev, dtype=torch.uint8)
    cms = None
    for _ in range(5):
        e0.record()
        L.check(lib.cobevt_calibrate_copy(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), n, stream), "cobevt_calibrate_copy")
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1)
        cms = t if cms is None or t < cms else cms
    del src, dst
    return {"mfma_bf16_tflops": round(flops / (best[0] * 1e-3) / 1e12, 1), "sclk_mhz_under_mfma_load": round(sclk, 0),
            "sclk_max_mhz": round(smax.value / 1e3, 0), "hbm_copy_gbs": round(2.0 * n / (cms * 1e-3) / 1e9, 1),
            "note": "csrc/calibrate.hip, best of 3 / 5 launches: 1024 workgroups x 4 waves x %d x 4 independent bf16 32x32x16 MFMAs; "
                    "shader clock = s_memtime / wall-clock ticks of workgroup 0 inside that loop; 1 GiB streaming copy "
                    "(read + write bytes)" % iters}


# ----------------------------------------------------------------------------------------------
# roofline leg
# ----------------------------------------------------------------------------------------------
MFMA_FAMILIES = ("conv3x3", "basicblock", "bottleneck", "gemm_rows", "row_chain", "igemm", "attention", "stem7x7", "head3x3", "swap_stage")
HBM_BOUND_FAMILIES = ("gemm_rows", "stem7x7", "head3x3", "bottleneck")   # AI below the ridge
# the row chains issue ~25 VALU instructions per MFMA (LayerNorm, GELU, bias / residual epilogues of four chained
# GEMMs): neither the matrix pipe (0.14 busy) nor HBM (0.16-0.3 of peak) is what they wait for.  Their entry is priced against
# the VALU issue rate: wave-instructions per second (SQ_INSTS_VALU of the committed PMC pass / this run's launch time) over
# 1024 SIMDs x 2.4 GHz / 4 cycles per wave64 instruction
VALU_BOUND_FAMILIES = ("row_chain",)
PEAK_VALU_GINST = 1024 * 2.4 / 4.0      # 614.4 G wave-instructions / s
PEAK_HBM_GBS = 8000.0      # MI355X_MICROARCH.md: 8 TB/s peak (about 6.3 TB/s achievable)


def load_pmc(dtype_name):
    """newest committed rocprofv3 PMC summary (tools/pmc_collect.sh -> tools/pmc_roofline.py), or the round-1 traffic file"""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "pmc_r*.json")))
    if files and dtype_name == "bf16":
        d = json.load(open(files[-1]))
        return d.get("families", {}), d.get("attention_launches", {}), os.path.basename(files[-1])
    old = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(old):
        t = json.load(open(old)).get(dtype_name, {})
        return {k: {"hbm_bytes": v} for k, v in t.items()}, {}, "pmc_traffic.json"
    return {}, {}, None


def roofline_leg(runner, dtype_name):
    """HIP events (launch stream) around every C-ABI call of one eager frame, best of 3 frames.  Returns the roofline
    entry of the kernel family with the largest measured time ("dominant kernel"), one entry per other family, and the
    level-0 FAX attention launch (the north-star's kernel) on its own."""
    best, best_tot, best_shapes = None, None, None
    runner.model.overlap_streams = False       # time every launch alone (side-stream K/V work would share the CUs)
    for _ in range(3):
        with ops.LaunchProfile() as prof:
            runner.eager_step()
        summ = prof.summary()
        tot = sum(d["ms"] for d in summ.values())
        if best is None or tot < best_tot:
            best, best_tot, best_shapes = summ, tot, prof.summary(by_shape=True)
    runner.model.overlap_streams = True
    peak = PEAK_TFLOPS[dtype_name]
    fam_pmc, attn_pmc, pmc_file = load_pmc(dtype_name)

    def entry(name, d, pmc, bound=None):
        tf = d["flops"] / (d["ms"] * 1e-3) / 1e12
        gbs = d["bytes"] / (d["ms"] * 1e-3) / 1e9
        e = {"kernel": name, "traffic": pmc.get("hbm_bytes"), "mfma_util_pmc": pmc.get("mfma_util"),
             "launches_per_frame": d["calls"],
             "avg_launch_us": round(d["ms"] * 1e3 / d["calls"], 2),
             # `traffic` / `mfma_util_pmc` come from the committed rocprofv3 PMC run (another box): its own average launch
             # duration beside this run's HIP-event figure, so a reader sees how far the two runs are apart
             "avg_duration_us_profiled": pmc.get("avg_duration_us_profiled"),
             "total_ms_per_frame": round(d["ms"], 3),
             "algorithmic_gflop_per_launch": round(d["flops"] / 1e9 / d["calls"], 2),
             "algorithmic_mbyte_per_launch": round(d["bytes"] / 1e6 / d["calls"], 2),
             "algorithmic_tflop_s": round(tf, 2), "algorithmic_gbyte_s": round(gbs, 1)}
        hbm = (name in HBM_BOUND_FAMILIES) if bound is None else bound == "hbm"
        insts = (pmc.get("counters_per_launch") or {}).get("SQ_INSTS_VALU")
        if bound is None and name in VALU_BOUND_FAMILIES and insts:
            gi = insts * d["calls"] / (d["ms"] * 1e-3) / 1e9
            e.update({"bound": "valu", "achieved": round(gi, 1), "peak": round(PEAK_VALU_GINST, 1), "unit": "G wave-instructions/s",
                      "frac": round(gi / PEAK_VALU_GINST, 4), "valu_insts_per_launch_pmc": round(insts),
                      "hbm_frac": round(gbs / PEAK_HBM_GBS, 4), "mfma_frac": round(tf / peak, 4)})
        elif hbm or (bound is None and name in VALU_BOUND_FAMILIES):      # K <= 512 GEMMs / the image stem: arithmetic intensity below the ridge
            e.update({"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                      "frac": round(gbs / PEAK_HBM_GBS, 4)})
        else:
            e.update({"bound": "mfma", "achieved": round(tf, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(tf / peak, 4)})
        return e

    fams = [f for f in MFMA_FAMILIES if f in best]
    fams.sort(key=lambda f: -best[f]["ms"])
    dom = entry(fams[0], best[fams[0]], fam_pmc.get(fams[0], {}))
    dom["pmc_source"] = pmc_file
    # the family's launches by shape (largest first): the family figure above averages 64-channel, 512-channel and tiny
    # decoder launches; a rocprofv3 --kernel-trace row is one tile variant, i.e. close to one of these lines
    shp = sorted(((k, v) for k, v in best_shapes.items() if k.startswith(fams[0] + "|")), key=lambda kv: -kv[1]["ms"])
    dom["by_launch_shape"] = [
        {"shape": k.split("|", 1)[1], "launches_per_frame": v["calls"], "avg_launch_us": round(v["ms"] * 1e3 / v["calls"], 2),
         "achieved": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1), "frac": round(v["flops"] / (v["ms"] * 1e-3) / 1e12 / peak, 4)}
        for k, v in shp[:6]]
    others = [entry(f, best[f], fam_pmc.get(f, {})) for f in fams[1:]]
    # the largest attention launch = level-0 cross attention #1 (64 windows x 4 cameras x 256 queries x 256 keys per agent)
    attn = {k: v for k, v in best_shapes.items() if k.startswith("attention|")}
    fax0 = None
    if attn:
        k0 = max(attn, key=lambda k: attn[k]["flops"] / attn[k]["calls"])
        pm = {}
        big = [v for kk, v in attn_pmc.items() if v.get("counters_per_launch")]
        if big:                   # the PMC record with the most MFMA work per launch is the same launch
            pm = max(big, key=lambda v: v["counters_per_launch"].get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0))
        fax0 = entry("fax_attention_level0 (%s)" % k0.split("|", 1)[1], attn[k0], pm, bound="mfma")
        # two different numbers: `useful_mfma_frac` = algorithmic FLOP/s / dense peak (= `frac`);
        # `mfma_util_pmc` = matrix-pipe BUSY share, which also counts the row-sum MFMAs (ones x P^T, 4 of every 12
        # matrix instructions of a 64-key tile: csrc/attention_resident.hip) - VALU work moved onto the idle matrix pipe, not
        # useful FLOPs.  SQ_INSTS_MFMA per launch vs the count the algorithmic FLOPs need states the overhead.
        fax0["useful_mfma_frac"] = fax0["frac"]
        need = attn[k0]["flops"] / attn[k0]["calls"] / (2.0 * 32 * 32 * 16)
        have = (pm.get("counters_per_launch") or {}).get("SQ_INSTS_MFMA")
        fax0["mfma_insts_needed_per_launch"] = round(need)
        fax0["mfma_insts_issued_per_launch_pmc"] = None if have is None else round(have)
        fax0["mfma_inst_overhead"] = None if not have else round(have / need, 3)
    return dom, others, fax0, round(best_tot, 3)


def cpu_baseline_leg(model, cfg, batch_cpu, gpu_out):
    """Time the oracle (CPU restatement, parity-pinned to the reference's golden vectors) on the bench frame and use its
    output as the parity reference for the GPU logits."""
    import numpy as np
    import oracle.corpbevt as o_model
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    # intra-op threads: all cores up to 32 (PyTorch's CPU kernels slow down badly when oversubscribed across
    # the 256 hardware threads / NUMA domains of the GPU box: 118 s/frame at 256 threads)
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    reps = 3                                    # ~15-20 s of CPU work on the GPU box's host
    t0 = time.time()
    with torch.no_grad():
        for _ in range(reps):
            ref = o_model.corpbevt_forward(sd, cfg, batch_cpu)["dynamic_seg"]
    dt = (time.time() - t0) / reps
    base = {"value": round(1.0 / dt, 4), "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": "%d frames (%d agents x 4 cams x 512x512 -> 256x256 BEV) of the bench workload, fp32, oracle/ "
                      "(plain PyTorch CPU restatement of the reference forward), %.1f s per frame" % (reps, batch_cpu["inputs"].shape[0], dt)}

    def parity(out):
        got = out["dynamic_seg"].detach().float().cpu()
        rel = ((got - ref).abs().max() / ref.abs().max()).item()
        rms = ((got - ref).double().square().sum().sqrt() / ref.double().square().sum().sqrt()).item()
        pa, pr = got.argmax(2).numpy(), ref.argmax(2).numpy()
        ious = [float(v) for v in o_model.mean_iu(pa[0, 0], pr[0, 0])]
        top2 = ref.topk(2, dim=2).values
        margin = ((top2[:, :, 0] - top2[:, :, 1]) / ref.abs().max()).numpy()
        same = pa == pr
        decisive = margin > 0.02
        return {"logits_rel_err_vs_oracle": float("%.3e" % rel), "logits_rms_rel_err_vs_oracle": float("%.3e" % rms),
                "argmax_agreement": round(float(same.mean()), 5),
                "argmax_agreement_decisive": round(float(same[decisive].mean()) if decisive.any() else 1.0, 5),
                "decisive_fraction": round(float(decisive.mean()), 4),
                "worst_flipped_margin": round(float(margin[~same].max()) if (~same).any() else 0.0, 5),
                "class_support_oracle": [int((pr == c).sum()) for c in range(ref.shape[2])],
                "iou_per_class_vs_oracle_argmax": [round(v, 5) for v in ious],
                "miou_vs_oracle_argmax": round(float(np.mean(ious)), 5),
                "metric": "max|got - ref| / max|ref| and ||got - ref||_2 / ||ref||_2 over the logits; arg-max agreement over all pixels and "
                          "over the decisive ones (oracle top-2 margin > 2 % of the logit scale); per-class IoU of the arg-max maps "
                          "(seg_utils.py:25-51).  The procedural head is class-balanced (cobevt_amd.synth.balance_seg_head_): half "
                          "of the map sits within a few % of a tie, so agreement here is a worst case"}
    par = {k: parity(v) for k, v in gpu_out.items()}
    # what the REFERENCE's own bf16 run (torch.autocast) does on this very frame (fixture made by running the reference,
    # tests/golden/make_golden.py gv18): the yardstick of the bf16 figures above
    try:
        g = np.load(os.path.join(ROOT, "tests", "golden", "gv18_reference_bf16_autocast.npz"))
        key = "CorpBEVT.full %d agents balanced head" % batch_cpu["inputs"].shape[0]
        if "bf16" in par and key in g.files:
            par["bf16"]["reference_bf16_autocast_on_this_frame"] = {
                "logits_rel_err_vs_fp32": float("%.3e" % g[key][0]), "logits_rms_rel_err_vs_fp32": float("%.3e" % g[key][1]),
                "argmax_agreement": round(float(g[key][2]), 5), "source": "tests/golden/gv18_reference_bf16_autocast.npz[%r]" % key}
    except Exception:  # noqa: BLE001
        pass
    return base, par


# ----------------------------------------------------------------------------------------------
# workloads
# ----------------------------------------------------------------------------------------------
def lidar_inputs(dev, seed=0):
    x = synth.procedural_input("lidar.x", (1, 8, 64, 256, 256), seed).to(dev)
    mask = torch.ones(1, 256, 256, 1, 8)
    mask[0, :, :, :, 6:] = 0
    ii, jj = torch.meshgrid(torch.arange(256), torch.arange(256), indexing="ij")
    mask[0, :, :, 0, 3] = (jj > ii // 2).float()
    return x, mask.to(dev)


def rt_nchw(y):
    """(b, h, w, d) channels-last -> (b, d, h, w) view"""
    return y.permute(0, 3, 1, 2)


def run_lidar(args, rank, world, dev, keep=None):
    enc = synth.fill_module_(host.SwapFusionEncoder(dict(LIDAR_ARGS)), 0).eval().to(dev)
    x, mask = lidar_inputs(dev, seed=rank)
    note = "SwapFusionEncoder.forward(x fp32 (1,8,64,256,256), mask) incl. the layout / dtype conversion at the module boundary"
    if world > 1 and args.mode == "latency":
        from cobevt_amd.host import swap_fusion_modules as sfm
        stages, head = sfm.sharded_stages(enc)
        pipe = cdist.RowShardedFuseBEVT(stages, head, rank, world, LIDAR_ARGS["window_size"])
        xf, _ = lidar_inputs(dev, seed=0)                      # every rank works on the SAME frame; rank r owns its agents
        per = 8 // world
        mine = sfm._to_blhwc(xf[:, rank * per:(rank + 1) * per].contiguous())
        step = lambda: pipe.step(mine, mask)                   # noqa: E731
        frames_per_step, scaling = 1, "strong"
        if args.full:
            with torch.no_grad():   # the sharded result must equal the single-process encoder on the whole map (bf16 rounding apart)
                ref = enc(xf, mask)
                got = rt_nchw(pipe.step(mine, mask))
                torch.cuda.synchronize()
                err = float(((got.float() - ref.float()).abs().max() / ref.float().abs().max()).item())
            if err > 3e-2:
                raise RuntimeError("rank %d: row-sharded FuseBEVT differs from the single-process encoder (rel %.3e)" % (rank, err))
        par = "row-sharded x%d: agent->band all-to-all, band<->grid all-to-all per half block, all-gather of fused bands" % world
        note = "channels-last compute-dtype agent maps resident on their owner GPU (agent-per-GPU), eager launches"
    else:
        run = pipeline.CapturedCall(lambda a, m: enc(a, m), x, mask, use_graph=not args.no_graph)
        step = run.step
        frames_per_step, scaling = world, "weak"
        par = "single GPU" if world == 1 else "replicas x%d (one LiDAR frame per GPU, no collective)" % world
    elapsed, per_ms = timed_loop(step, args.warmup, args.steps, world, dev, keep=keep)
    ms = elapsed / args.steps * 1e3
    fps = frames_per_step / (ms * 1e-3)
    res = {"metric": "bev_frames_per_sec", "value": round(fps, 3), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(ms, 4), "ms_per_step_median": round(pct(per_ms, 0.5), 4),
           "ms_per_step_p95": round(pct(per_ms, 0.95), 4), "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
           "dtype": args.dtype, "data": "synthetic",
           "config": {"workload": "OPV2V-LiDAR FuseBEVT: SwapFusionEncoder(input_dim 64, 8 agents, window 8, depth 3, mask) on "
                                  "voxel-BEV features (1, 8, 64, 256, 256) -> (1, 64, 256, 256)", "parallelism": par,
                      "hip_graph": not args.no_graph and not (world > 1 and args.mode == "latency"), "timed": note,
                      "weights": "procedural (cobevt_amd.synth)"},
           "achieved_tflops_end_to_end": round(LIDAR_GF * frames_per_step / (ms * 1e-3) / 1e3, 2)}
    if rank == 0 and world == 1 and args.full and not args.no_roofline:
        ent = lidar_roofline(enc, x, mask, args.dtype)
        res["roofline"], res["roofline_other_kernels"] = ent[0], ent[1:]
    return res


def lidar_roofline(enc, x, mask, dtype_name):
    """HIP events around every launch of one eager SwapFusionEncoder forward -> one roofline entry per kernel family, largest first"""
    with ops.LaunchProfile() as prof:
        enc(x, mask)
    summ = prof.summary()
    peak = PEAK_TFLOPS[dtype_name]
    fams = sorted(summ, key=lambda f: -summ[f]["ms"])
    # `traffic` / `mfma_util_pmc`: this workload's own rocprofv3 PMC passes (tools/pmc_collect.sh <out> <tag> lidar), newest committed file
    pmc, pmc_file = {}, None
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "pmc_lidar_r*.json")))
    if files and dtype_name == "bf16":
        pmc, pmc_file = json.load(open(files[-1])).get("families", {}), os.path.basename(files[-1])
    ent = []
    for f in fams:
        d = summ[f]
        tf, gbs = d["flops"] / (d["ms"] * 1e-3) / 1e12, d["bytes"] / (d["ms"] * 1e-3) / 1e9
        hbm = f in HBM_BOUND_FAMILIES
        pf = pmc.get(f, {})
        ent.append({"kernel": f, "traffic": pf.get("hbm_bytes"), "mfma_util_pmc": pf.get("mfma_util"),
                    "avg_duration_us_profiled": pf.get("avg_duration_us_profiled"), "pmc_source": pmc_file,
                    "algorithmic_mbyte_per_launch": round(d["bytes"] / 1e6 / d["calls"], 2),
                    "launches_per_frame": d["calls"], "avg_launch_us": round(d["ms"] * 1e3 / d["calls"], 2),
                    "bound": "hbm" if hbm else "mfma", "achieved": round(gbs if hbm else tf, 2),
                    "peak": PEAK_HBM_GBS if hbm else peak, "unit": "GB/s" if hbm else "TFLOP/s",
                    "frac": round((gbs / PEAK_HBM_GBS) if hbm else (tf / peak), 4)})
    return ent


def maybe_spawn(args):
    """`python bench.py --gpus N` with no launcher around it: start the N ranks ourselves (one process per GPU under
    torch.distributed.run, rendezvous on 127.0.0.1) and hand their exit code back.  Under torchrun (WORLD_SIZE set) this is
    a no-op."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    import socket
    import subprocess
    n_dev = torch.cuda.device_count()
    gloo = os.environ.get("COBEVT_DIST_BACKEND") == "gloo"
    if n_dev < args.gpus and not gloo:
        raise SystemExit("bench.py --gpus %d: this node has %d GPU(s); RCCL needs one GPU per rank "
                         "(COBEVT_DIST_BACKEND=gloo dry-runs the multi-rank control flow on fewer GPUs)" % (args.gpus, n_dev))
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


def rank_table(rank, world, dev):
    """what the process group actually is: backend, world size and the GPU every rank sits on (read back from the ranks)"""
    props = torch.cuda.get_device_properties(dev)
    me = {"rank": rank, "pid": os.getpid(), "device_index": dev.index, "name": props.name,
          "uuid": str(getattr(props, "uuid", "")), "pci_bus_id": getattr(props, "pci_bus_id", None)}
    if world == 1:
        return {"backend": None, "world_size": 1, "ranks": [me]}
    rows = [None] * world
    torch.distributed.all_gather_object(rows, me)
    return {"backend": torch.distributed.get_backend(), "world_size": torch.distributed.get_world_size(), "ranks": rows,
            "distinct_gpus": len({(r["device_index"], r["uuid"], r["pci_bus_id"]) for r in rows})}


def gather_latency_leg(model, batch, rank, world, A, dev, which=("rccl", "direct")):
    """the exchange on its own: microseconds per agent all-gather of the (A, 32, 32, 128) blocks (HIP events over 200 back-to-back
    exchanges, max over ranks) through RCCL and / or the direct peer-window path"""
    feats = model.encode_agents(cdist.take_agents(batch, [0]))
    block, dt = tuple(feats.shape[1:]), feats.dtype
    mine = cdist.agents_of_rank(rank, world, A)
    local = torch.zeros((max(1, len(mine)),) + block, device=dev, dtype=dt)
    staging = torch.zeros((cdist.slots_per_rank(world, A),) + block, device=dev, dtype=dt)
    full = torch.empty((A,) + block, device=dev, dtype=dt)

    def timed(fn, n=200):
        for _ in range(20):
            fn()
        torch.distributed.barrier()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t = torch.tensor([e0.elapsed_time(e1) * 1e3 / n], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        return round(t.item(), 2)

    out = {"bytes_per_agent_block": int(local[0].numel() * local.element_size())}
    if "rccl" in which:
        out["rccl_all_gather_into_tensor"] = timed(lambda: cdist.exchange_features_strong(local, len(mine), rank, world, A, out=full,
                                                                                          staging=staging))
    if "direct" in which:
        ex = cdist.DirectExchange(block, dt, A, rank, world, device=dev).plan(*cdist.direct_plan_strong(rank, world, A))
        out["direct_peer_write"] = timed(lambda: ex(local))
        st, _ = ex.status()
        if st:
            out["direct_peer_write_status"] = st
        ex.close()
    return out


def direct_probe_child(args, world):
    """The direct peer-window legs (latency mode over the hipIpc windows, the exchange microbenchmark) as a job of their own: rank 0 of
    the finished main job starts a second `torch.distributed.run` with --direct-probe and merges its JSON line.  The path maps other GPUs'
    memory into every rank and polls flags in it; it has run between processes on ONE GPU and in the gloo dry run only, so on the first
    real multi-GPU node a fault in it (a GPU page fault aborts the process, nothing to catch) must not take the RCCL headline down with
    it.  Returns the child's dict, or {"error": ...}."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    drop = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "GROUP_WORLD_SIZE", "ROLE_RANK", "ROLE_WORLD_SIZE", "ROLE_NAME",
            "MASTER_ADDR", "MASTER_PORT")
    env = {k: v for k, v in os.environ.items() if k not in drop and not k.startswith("TORCHELASTIC_")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), "--gpus", str(world), "--steps", str(args.steps), "--warmup",
           str(args.warmup), "--dtype", args.dtype, "--agents", str(args.agents), "--direct-probe", "--full"] + (["--no-graph"] if args.no_graph else [])
    # its own session / process group, so that a hung rank (a peer that never arrives leaves the others in bounded GPU polls, then in
    # a host-side barrier) can be killed as a whole; the limit is generous for a healthy job (~60-120 s) and short enough not to
    # eat the driver's window around the bench
    limit = int(os.environ.get("COBEVT_DIRECT_PROBE_TIMEOUT", "360"))
    import signal
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(proc.pid, signal.SIGKILL)
        except OSError:
            pass
        proc.communicate()
        return {"error": "direct-exchange probe job killed after %d s (COBEVT_DIRECT_PROBE_TIMEOUT): a rank of the peer-window "
                         "exchange stalled; the RCCL figures of this line are unaffected" % limit}
    p = subprocess.CompletedProcess(cmd, proc.returncode, out, err)
    for line in reversed(p.stdout.splitlines()):
        if line.startswith("{"):
            try:
                return json.loads(line)
            except ValueError:
                break
    return {"error": "direct-exchange probe job failed (exit code %d): %s" % (p.returncode, p.stderr.strip()[-400:])}


def camera_leg(args, mode, model, cfg, rank, world, dev, gather="rccl", depth=None, keep=None):
    """build the runner of one mode, check it against the plain forward (--full), time it -> (result fields, runner, timed, batch,
    full, frames in flight); keep: see timed_loop"""
    A = args.agents
    strong = world > 1 and mode == "latency"
    # throughput mode: this rank's A agent tasks (images differ per rank) + the pose / record_len of frame `rank`;
    # latency mode: every rank sees frame 0 and encodes only its agents
    full = synth.opv2v_batch(agents=A, max_cav=cfg["max_cav"], seed=0 if strong else rank)
    batch = {k: v.to(dev) for k, v in full.items()}
    in_flight, pipeline_note, graph_ok = 1, "none", False

    if strong:
        mine = cdist.agents_of_rank(rank, world, A)
        sub = dict(cdist.take_agents(batch, mine if mine else [0]), transformation_matrix=batch["transformation_matrix"],
                   record_len=batch["record_len"])
        depth = 2 if depth is None else depth
        timed = pipeline.FrameShardedCorpBEVT(model, sub, batch, rank, world, A, use_graph=not args.no_graph, gather=gather, depth=depth)
        graph_ok = timed.graphs is not None
        runner = timed
        frames_per_step = 1
        in_flight = depth
        pipeline_note = ("rank r encodes agents r, r+%d, ..; %s; fusion + decoder replicated on every rank%s" % (
            world, "one RCCL all_gather_into_tensor between graph replays" if gather == "rccl" else
            "one direct peer-window exchange (csrc/peer_gather.hip) inside the captured graph",
            "; the tail of frame i-1 runs on a second stream under the encoder of frame i" if depth == 2 else ""))
        # --full: every rank must reproduce the un-sharded forward of the whole frame (agents are a pure batch dimension up to the
        # gather; not bit for bit in bf16: the conv tile shapes - hence the summation order - are chosen per batch size)
        ref = model(dict(batch))["dynamic_seg"] if args.full else None
        for _ in range(depth):
            got = timed.step()
        got = got["dynamic_seg"]
        torch.cuda.synchronize()
        timed.status()
        if args.full:
            shard_check = float(((got - ref).abs().max() / ref.abs().max()).item())
            if shard_check > (5e-2 if args.dtype == "bf16" else 1e-4):
                raise RuntimeError("rank %d: frame-sharded output differs from the single-process forward (rel %.3e)" % (rank, shard_check))
    else:
        runner = pipeline.CapturedCorpBEVT(model, batch, rank, world, A, use_graph=False)
        ref_out = {k: v.clone() for k, v in runner.eager_step().items()} if args.full else None
        torch.cuda.synchronize()
        if not args.no_graph:
            try:
                runner.capture()
                graph_ok = True
            except Exception as e:  # noqa: BLE001 — fall back to eager launches, say so in the JSON
                runner.graphs = None
                if rank == 0:
                    print("HIP graph capture failed (%s: %s); running eagerly" % (type(e).__name__, e), file=sys.stderr)
                torch.cuda.synchronize()
        timed = runner
        # default: three frames in flight (software pipeline over the three stages of a frame)
        if args.frames_in_flight in (3, 4) and graph_ok:
            try:
                timed = pipeline.PipelinedCorpBEVT(model, batch, rank, world, A, depth=args.frames_in_flight)
                for _ in range(2 * args.frames_in_flight + 2):
                    out = timed.step()
                torch.cuda.synchronize()
                for k in (ref_out or {}):          # --full: steady state == un-pipelined forward, bit for bit
                    if not torch.equal(out[k], ref_out[k]):
                        raise RuntimeError("pipelined frame differs from the un-pipelined forward in %r" % k)
                in_flight = args.frames_in_flight
                pipeline_note = ("%s of %d consecutive frames on %d HIP streams in one captured graph; one frame in, one frame "
                                 "out per step%s" %
                                 ("S1 encoder + K/V | S2 FAX query | S3 fusion + decoder" if in_flight == 3 else
                                  "S1 encoder + K/V | S2a FAX level 0 | S2b FAX levels 1-2 + global attention | S3 fusion + decoder",
                                  in_flight, in_flight,
                                  "; steady-state output checked bit-identical to the un-pipelined forward" if ref_out else ""))
            except Exception as e:  # noqa: BLE001 — never lose the measurement: fall back to one frame at a time, say so
                if world == 1:
                    raise
                timed, in_flight = runner, 1
                pipeline_note = "pipelined mode failed (%s: %s); one frame at a time" % (type(e).__name__, e)
                torch.cuda.synchronize()
        if world > 1:                              # every rank must take the same path
            flag = torch.tensor([in_flight], device=dev)
            torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
            if int(flag.item()) != in_flight:
                timed, in_flight = runner, 1
                pipeline_note = "pipelined mode failed on another rank; one frame at a time"
        frames_per_step = world

    elapsed, per_ms = timed_loop(timed.step, args.warmup, args.steps, world, dev, keep=keep)
    if strong:
        timed.status()
    ms_per_step = elapsed / args.steps * 1e3
    fps = frames_per_step / (ms_per_step * 1e-3)
    res = {
        "metric": "bev_frames_per_sec", "value": round(fps, 3), "unit": "frames/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
        "ms_per_step_median": round(pct(per_ms, 0.5), 4), "ms_per_step_p95": round(pct(per_ms, 0.95), 4),
        "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": args.dtype,
        "data": "synthetic", "mode": "latency" if strong else "throughput", "frames_per_sec_per_gpu": round(fps / world, 3),
        "config": {"workload": "OPV2V-camera CoBEVT (corpbevt.yaml): %d agents x 4 cams x 512x512 -> 256x256 BEV, "
                               "ResNet-34 + FAX + swap fusion, batch 1 frame per GPU" % A,
                   "agents": A, "frames_in_flight": in_flight if strong else world * in_flight,
                   "frame_latency_steps": getattr(timed, "latency_steps", 1),
                   "pipeline": pipeline_note,
                   "parallelism": ("single GPU" if world == 1 else
                                   "one frame over %d GPUs: agent a on GPU a mod %d; 1 all-gather (%s); fusion replicated" % (world, world, gather)
                                   if strong else "%d frames in flight, their agents dealt round-robin over the GPUs + 1 all-gather; "
                                                  "every GPU fuses its own frame" % world),
                   "runner": type(timed).__module__ + "." + type(timed).__name__,
                   "hip_graph": graph_ok, "weights": "procedural (cobevt_amd.synth)"},
        "achieved_tflops_end_to_end": round((GF_PER_AGENT * A + GF_PER_FRAME) * frames_per_step / (ms_per_step * 1e-3) / 1e3, 2),
    }
    return res, runner, timed, batch, full, in_flight


def main():
    args = parse()
    maybe_spawn(args)
    rank, world, local_rank = cdist.init_from_env()
    if world != args.gpus:
        if rank == 0:
            print("warning: --gpus %d but WORLD_SIZE=%d; using WORLD_SIZE" % (args.gpus, world), file=sys.stderr)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the HIP path)")
    local_rank %= torch.cuda.device_count()          # (several ranks share a GPU only in the gloo dry-run mode of cobevt_amd/dist.py)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    torch.set_grad_enabled(False)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    host.set_compute_dtype(dtype)

    if args.workload == "lidar":
        if args.mode in (None, "both"):
            args.mode = "throughput"
        keep = [] if args.dump_outputs else None
        result = run_lidar(args, rank, world, dev, keep=keep)
        result["rccl_ranks"] = rank_table(rank, world, dev)
        if rank == 0:
            if keep:
                result["dumped_outputs"] = dump_outputs(keep[0], args.dump_outputs)
            print(json.dumps(result), flush=True)
        if world > 1:
            torch.distributed.destroy_process_group()
        return

    A = args.agents
    cfg = synth.corpbevt_config(max_cav=max(5, A))
    model = synth.fill_module_(host.CorpBEVT(copy.deepcopy(cfg)), 0).eval()
    synth.balance_seg_head_(model, A)
    model = model.to(dev)
    # N = 1: the three-frames-in-flight single-GPU pipeline.  N > 1, default ("both"): the headline is BASELINE.json's
    # partitioning - ONE frame over the GPUs, one agent per GPU, one all-gather in front of FuseBEVT ("latency", strong
    # scaling) - and the same line carries the throughput mode (N frames in flight, weak scaling) and the exchange's own
    # latency over RCCL and over the direct peer-window path.
    mode = args.mode or ("throughput" if world == 1 else "both")
    ranks = rank_table(rank, world, dev)
    if args.direct_probe:                   # the child job of direct_probe_child(): only the direct peer-window legs
        if world < 2:
            raise SystemExit("--direct-probe is the multi-rank child job of bench.py")
        probe = {}
        try:
            r = camera_leg(args, "latency", model, cfg, rank, world, dev, gather="direct")
            probe["latency_mode_direct_gather"] = {k: r[0][k] for k in ("value", "unit", "ms_per_step", "ms_per_step_median", "scaling", "mode", "config")}
            safe(probe, "all_gather_us", lambda: gather_latency_leg(model, r[3], rank, world, A, dev, which=("direct",)))
        except Exception as e:  # noqa: BLE001
            torch.cuda.synchronize()
            probe["latency_mode_direct_gather"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
        probe["rccl_ranks"] = ranks
        if rank == 0:
            print(json.dumps(probe), flush=True)
        torch.distributed.destroy_process_group()
        return
    isolate_direct = False
    keep = [] if args.dump_outputs else None
    if world > 1 and ranks.get("backend") == "nccl" and ranks.get("distinct_gpus") != world:
        raise SystemExit("bench.py: RCCL process group of %d ranks sits on %s distinct GPU(s) - one GPU per rank is required "
                         "(rank table: %s)" % (world, ranks.get("distinct_gpus"), ranks["ranks"]))
    if world > 1:
        # Headline at N > 1: the SAME quantity as at N = 1 - whole-job frames/s with frames in flight ("throughput"
        # mode, weak scaling: N frames per step, their N x A agent tasks dealt round-robin over the GPUs, ONE exchange of the agent
        # blocks in front of FuseBEVT) - so the driver's value_N / (N x value_1) IS the agent-shard scaling efficiency.  The
        # north-star's one-frame partition (one agent per GPU, "latency" mode, strong scaling) rides in the same line as
        # `latency_mode` with its `frame_latency_ms`: with 5 agents it cannot use more than 5 GPUs, so its frames/s per GPU falls
        # as 1/N by construction and is not the scaling figure.  `--mode latency` makes it the headline explicitly.
        def side(**kw):
            try:
                r, _, t, _, _, _ = camera_leg(args, kw.pop("mode", "latency"), model, cfg, rank, world, dev, **kw)
                out = {k: r[k] for k in ("value", "unit", "ms_per_step", "ms_per_step_median", "scaling", "mode", "config")}
                if r["mode"] == "latency":
                    out["frame_latency_ms"] = round(r["ms_per_step"] * r["config"]["frame_latency_steps"], 4)
                return out
            except Exception as e:  # noqa: BLE001
                torch.cuda.synchronize()
                return {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
        head_mode = "latency" if mode == "latency" else "throughput"
        result, runner, timed, batch, full, in_flight = camera_leg(args, head_mode, model, cfg, rank, world, dev, keep=keep,
                                                                   **({"gather": args.gather} if head_mode == "latency" else {}))
        if head_mode == "latency":
            result["frame_latency_ms"] = round(result["ms_per_step"] * result["config"]["frame_latency_steps"], 4)
        other_gather = "direct" if args.gather == "rccl" else "rccl"
        if mode == "both" and args.full:
            result["latency_mode"] = side(gather=args.gather)                      # depth 2: the tail of frame i-1 under frame i
            result["latency_mode_unpipelined"] = side(gather=args.gather, depth=1)
            # the direct peer-window legs run in a job of their own after this one (direct_probe_child) unless the direct exchange
            # IS the requested gather (--gather direct): a fault there must not cost the RCCL numbers
            isolate_direct = args.gather == "rccl"
            if isolate_direct:
                safe(result, "all_gather_us", lambda: gather_latency_leg(model, batch, rank, world, A, dev, which=("rccl",)))
            else:
                result["latency_mode_%s_gather" % other_gather] = side(gather=other_gather)
                safe(result, "all_gather_us", lambda: gather_latency_leg(model, batch, rank, world, A, dev))
        # --full: the N = 1 figures of the same box, measured by rank 0 alone while the other ranks wait at the barrier below: what
        # the per-GPU numbers above are to be compared with
        torch.distributed.barrier()
        if rank == 0 and args.full:
            def single():
                r1, run1, _, _, _, _ = camera_leg(args, "throughput", model, cfg, 0, 1, dev)
                lat = quick(run1.step, 3, 20)
                return {"frames_per_sec": r1["value"], "ms_per_step": r1["ms_per_step"], "one_frame_at_a_time_ms": lat["ms_median"]}
            safe(result, "single_gpu_reference", single)
            ref1 = result["single_gpu_reference"]
            if "error" not in ref1:
                tp = result if head_mode == "throughput" else result.get("throughput_mode", {})
                sc = {}
                if "value" in tp:
                    sc["throughput_frames_per_sec_per_gpu"] = round(tp["value"] / world, 3)
                    sc["throughput_scaling_efficiency_vs_n1"] = round(tp["value"] / world / ref1["frames_per_sec"], 4)
                lm = result if head_mode == "latency" else result.get("latency_mode", {})
                if "frame_latency_ms" in lm:
                    sc["frame_latency_ms"] = lm["frame_latency_ms"]
                    sc["frame_latency_speedup_vs_n1"] = round(ref1["one_frame_at_a_time_ms"] / lm["frame_latency_ms"], 4)
                sc["note"] = ("SCALE reads `value` (throughput mode at every N): efficiency = value_N / (N x value_1); the latency "
                              "mode's figure of merit is frame_latency_ms, not frames/s per GPU")
                result["scaling_summary"] = sc
        torch.distributed.barrier()
    else:
        result, runner, timed, batch, full, in_flight = camera_leg(args, "throughput", model, cfg, rank, world, dev, keep=keep)
    result["rccl_ranks"] = ranks
    graph_ok_main = bool(result["config"].get("hip_graph"))
    if rank == 0 and keep:
        result["dumped_outputs"] = dump_outputs(keep[0], args.dump_outputs)

    if rank == 0 and args.full:
        safe(result, "box_calibration", lambda: box_calibration(dev))
    if rank == 0 and world == 1 and args.full:
        if in_flight > 1:
            safe(result, "one_frame_at_a_time", lambda: dict(
                quick(runner.step, 5, 50), note="cobevt_amd.host.pipeline.CapturedCorpBEVT: the same forward from captured graphs "
                                               "without the cross-frame pipeline = the latency of a frame"))
        if not args.no_ingest and in_flight > 1 and args.agents <= 5:
            def ingest():
                """The reference's loop moves every frame to the device before the forward (inference_camera.py:56-61); `value` above
                replays frames that already sit in HBM.  Here the frames come from PINNED HOST memory every step: uint8 camera frames
                (the data loader's format after cv2.resize; /255, (x - mean) / std of rgb_preprocessor.py:14-31 folded into the stem
                kernel's gather as a table lookup, ResnetEncoder.set_rgb_normalisation) pulled over PCIe by a fetch kernel inside every
                step's captured graph (host.pipeline.HostFrameFeeder), three frames in flight as in `value`.  Beside it: the same loop on the
                fp32 image the reference uploads (63 MB per 5-agent frame instead of 15.7)."""
                A = args.agents
                b8c, b32c = synth.opv2v_batch_u8(agents=A, max_cav=cfg["max_cav"], seed=0)
                model.encoder.set_rgb_normalisation(synth.OPV2V_RGB_MEAN, synth.OPV2V_RGB_STD)
                b8, b32 = {k: v.to(dev) for k, v in b8c.items()}, {k: v.to(dev) for k, v in b32c.items()}
                o32 = {k: v.clone() for k, v in pipeline.CapturedCorpBEVT(model, b32, use_graph=False).eager_step().items()}
                o8 = pipeline.CapturedCorpBEVT(model, b8, use_graph=False).eager_step()
                same = all(torch.equal(o8[k], o32[k]) for k in o32)
                out = {"uint8_path_bit_identical_to_fp32_image_path": bool(same),
                       "h2d_mbyte_per_frame_uint8": round(b8c["inputs"].numel() / 1e6, 2),
                       "h2d_mbyte_per_frame_fp32_image": round(b32c["inputs"].numel() * 4 / 1e6, 2)}
                W, K = 10, max(20, min(args.steps, 100))
                for tag, bc, bd in (("uint8", b8c, b8), ("fp32_image", b32c, b32)):
                    if tag == "uint8":         # the frames resident (no pull): the same pipeline as `value` on bytes
                        res = pipeline.PipelinedCorpBEVT(model, bd, depth=in_flight)
                        el, _ = timed_loop(res.step, W, K, 1, dev)
                        out["value_uint8_frames_resident"] = round(K / el, 3)
                        del res
                    run = pipeline.PipelinedCorpBEVT(model, bd, depth=in_flight, host_ingest=True)
                    for r_ in range(in_flight):          # one distinct frame per pinned ring slot (the images rolled by 7 r_ rows)
                        run.pinned[r_].copy_(torch.roll(bc["inputs"], shifts=7 * r_, dims=3))
                    small = {k: v.pin_memory() for k, v in bc.items() if torch.is_tensor(v) and k != "inputs"}      # (pageable sources make the copies synchronous)
                    small["record_len"] = bc["record_len"].to(torch.int32).pin_memory()
                    feeder = pipeline.HostFrameFeeder(run)
                    feeder.put(dict(small, inputs=feeder.host_slot()))

                    def step():
                        # the frame is already in its ring slot (a loader decodes into host_slot()): put() only takes it over
                        feeder.put(dict(small, inputs=feeder.host_slot()))
                        feeder.step()
                    el, per = timed_loop(step, W, K, 1, dev)
                    out["value_with_h2d_" + tag] = round(K / el, 3)
                    out["ms_per_step_with_h2d_" + tag] = round(el / K * 1e3, 4)
                    out["ms_per_step_median_with_h2d_" + tag] = round(pct(per, 0.5), 4)
                    out["ms_per_step_max_with_h2d_" + tag] = round(per[-1], 4)
                    # the pull on its own: what the link delivers for this frame through the fetch kernel, and through the copy engine
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    dst = run.slots[0]["inputs"]
                    for which in ("fetch_kernel", "copy_engine"):
                        torch.cuda.synchronize()
                        e0.record()
                        for r_ in range(8):
                            if which == "fetch_kernel":
                                ops.host_fetch(run.pinned[r_ % in_flight], dst)
                            else:
                                dst.copy_(run.pinned[r_ % in_flight], non_blocking=True)
                        e1.record()
                        torch.cuda.synchronize()
                        ms = e0.elapsed_time(e1) / 8
                        out["h2d_ms_per_frame_%s_%s" % (tag, which)] = round(ms, 4)
                        out["h2d_gbyte_s_%s_%s" % (tag, which)] = round(dst.numel() * dst.element_size() / (ms * 1e-3) / 1e9, 2)
                    del run, feeder
                out["steps"], out["warmup"] = K, W
                out["note"] = ("frames/s of the same three-frames-in-flight pipeline as `value` with every step pulling the next frame's images "
                               "out of a ring of pinned host buffers inside the timed loop (a fetch kernel captured in the step's graph, "
                               "host.pipeline.HostFrameFeeder; one distinct frame per ring slot, the loader's decode into the ring is host work "
                               "outside this figure)")
                return out
            safe(result, "ingest", ingest)
            if isinstance(result.get("ingest"), dict) and "value_with_h2d_uint8" in result["ingest"]:
                result["value_with_h2d"] = result["ingest"]["value_with_h2d_uint8"]
        if not args.no_extra:
            safe(result, "eager_model_call", lambda: dict(
                quick(lambda: model(dict(batch)), 3, 20), note="plain `model(batch_dict)` as INTEGRATION.md §1 documents it: ~90 "
                                                                "ctypes launches per frame from Python, no HIP graph"))

            def graph_call():
                model.enable_graphs()
                try:
                    return dict(quick(lambda: model(batch), 3, 30), note="the same drop-in call after `model.enable_graphs()`: eval-mode "
                                "forward served from a captured plan per frame shape (host.pipeline.AgentCountPlans)")
                finally:
                    model.enable_graphs(False)
            safe(result, "model_call_with_graphs", graph_call)
        if not args.no_roofline:
            def roof():
                dom, others, fax0, timed_ms = roofline_leg(runner, args.dtype)
                result["roofline_other_kernels"] = others
                if fax0 is not None:
                    result["roofline_fax_attention"] = fax0
                result["timed_launch_ms_per_frame"] = timed_ms
                return dom
            safe(result, "roofline", roof)
        outs = {args.dtype: {k: v.clone() for k, v in runner.eager_step().items()}}
        if not args.no_extra:
            other = "fp32" if args.dtype == "bf16" else "bf16"

            def other_dtype():
                with host.compute_dtype(torch.float32 if other == "fp32" else torch.bfloat16):
                    r2 = pipeline.CapturedCorpBEVT(model, batch, use_graph=not args.no_graph)
                    q = dict(quick(r2.step, 2, 10), note="one frame at a time from captured graphs, %s storage + %s MFMA" %
                             (other, "exact v_mfma_f32_32x32x2_f32" if other == "fp32" else "v_mfma_f32_32x32x16_bf16"))
                    outs[other] = {k: v.clone() for k, v in r2.step().items()}
                return q
            if other == "fp32":
                # fp32 storage on the SPLIT-bf16 matrix path (host.set_compute_dtype("fp32_split"), libcobevt_hip_f32s.so): the mode that
                # meets the north-star's 1e-3 gate without the 16x-slower fp32 MFMA - `fp32_parity_mode`; the exact-fp32-MFMA mode
                # (v_mfma_f32_32x32x2_f32 everywhere) stays beside it as `fp32_exact_mode`
                def split_mode():
                    with host.compute_dtype("fp32_split"):
                        r2 = pipeline.CapturedCorpBEVT(model, batch, use_graph=not args.no_graph)
                        q = dict(quick(r2.step, 2, 20), note="one frame at a time from captured graphs, fp32 storage + split-bf16 MFMA: every matrix "
                                 "product as two v_mfma_f32_32x32x16_bf16 over (hi, lo) bf16 halves of both operands, all four cross terms "
                                 "(csrc/common.hpp COBEVT_F32_SPLIT); parity in `parity_fp32_split`")
                        outs["fp32_split"] = {k: v.clone() for k, v in r2.step().items()}
                        if graph_ok_main:
                            r3 = pipeline.PipelinedCorpBEVT(model, batch, depth=3)
                            for _ in range(8):
                                r3.step()
                            p3 = quick(r3.step, 3, 30)
                            q["three_frames_in_flight"] = {"ms_median": p3["ms_median"], "frames_per_sec": p3["frames_per_sec"]}
                    return q
                safe(result, "fp32_parity_mode", split_mode)

                # "fp32_fast" (round 6): fp32_split with the ResNet encoder's convolutions - 80 % of the frame's flops - on fp16 MFMAs with
                # fp16 operands out of fp32 storage (weights one fp16 term; activations one fp16 value in the packed form - two k-groups per
                # MFMA - or an fp16 (hi, lo) pair, converted once at patch staging; libcobevt_hip_f32h.so).  Still inside the north-star's
                # 1e-3 (parity in `parity_fp32_fast`), not the 1e-5 of fp32_split.
                def fast_mode():
                    with host.compute_dtype("fp32_fast"):
                        r2 = pipeline.CapturedCorpBEVT(model, batch, use_graph=not args.no_graph)
                        q = dict(quick(r2.step, 2, 20), note="one frame at a time from captured graphs; fp32 storage everywhere, ResNet encoder "
                                 "convolutions on v_mfma_f32_32x32x16_f16 with fp16 operands (csrc/common.hpp COBEVT_F32_SPLIT == 2), "
                                 "everything else on the split-bf16 path of fp32_parity_mode; parity in `parity_fp32_fast`")
                        outs["fp32_fast"] = {k: v.clone() for k, v in r2.step().items()}
                        if graph_ok_main:
                            r3 = pipeline.PipelinedCorpBEVT(model, batch, depth=3)
                            for _ in range(8):
                                r3.step()
                            p3 = quick(r3.step, 3, 30)
                            q["three_frames_in_flight"] = {"ms_median": p3["ms_median"], "frames_per_sec": p3["frames_per_sec"]}
                    return q
                safe(result, "fp32_fast_mode", fast_mode)
                safe(result, "fp32_exact_mode", other_dtype)
            else:
                safe(result, "bf16_mode", other_dtype)

            # the other single-GPU configurations of BASELINE.json (parity-tested in tests/; timed here for SURVEY.md §8d)
            def two_agents():
                b2 = {k: v.to(dev) for k, v in synth.opv2v_batch(agents=2, max_cav=cfg["max_cav"], seed=0).items()}
                r3 = pipeline.CapturedCorpBEVT(model, b2, use_graph=not args.no_graph)
                return dict(quick(r3.step, 3, 30), config="OPV2V-camera CoBEVT: 2 agents x 4 cams 512x512, 256x256 BEV, one frame at "
                                                           "a time", algorithmic_gflop=round(GF_PER_AGENT * 2 + GF_PER_FRAME, 1))

            def nuscenes(from_images):
                """BASELINE configs[1]: 1 ego x 6 cams 224x480 -> 200x200 BEV.  from_images: the whole model - Normalize ->
                EfficientNet-B4 extractor mirror (host/nuscenes/efficientnet.py) -> PyramidAxialEncoder -> Decoder -> heads - as the
                reference's benchmark times it (nuscenes/scripts/benchmark.py:42-55: batch 1, forward only); otherwise the FAX encoder
                + decoder on synthetic backbone features (SURVEY.md 8d's original leg, kept for continuity)"""
                from cobevt_amd.host import nuscenes as nu
                c = synth.nuscenes_config()
                feats, image, intr, ext = synth.nuscenes_inputs("bench.nuscenes", 0)
                if from_images:
                    from cobevt_amd.host.nuscenes.efficientnet import EfficientNetExtractor
                    backbone = EfficientNetExtractor(["reduction_2", "reduction_3", "reduction_4"], *c["image"])   # cvt_pyramid_axial.yaml:19
                else:
                    backbone = synth.FeatureMapBackbone(feats)
                encn = nu.PyramidAxialEncoder(backbone, **copy.deepcopy(c["encoder"]))
                sin = synth.fill_module_(nu.CrossViewTransformer(encn, nu.Decoder(**c["decoder"]), c["dim_last"], c["outputs"]), 0)
                sin = sin.eval().to(dev)
                r4 = pipeline.CapturedCall(lambda im, ii, ee: sin({"image": im, "intrinsics": ii, "extrinsics": ee}),
                                           image.to(dev), intr.to(dev), ext.to(dev), use_graph=not args.no_graph)
                if from_images:
                    return dict(quick(r4.step, 3, 30), config="nuScenes SinBEVT (BASELINE configs[1]): 1 ego x 6 cams 224x480 images -> "
                                "EfficientNet-B4 extractor -> FAX pyramid -> decoder -> 200x200 BEV, whole model from images, one "
                                "frame at a time from a captured graph (EfficientNet arithmetic restated: parity unpinned, DESIGN.md 4)")
                return dict(quick(r4.step, 3, 30), config="nuScenes SinBEVT: FAX encoder + decoder only, on synthetic "
                            "EfficientNet-B4-shaped backbone features (SURVEY.md 8d)", algorithmic_gflop=26.2)

            def lidar():
                """BASELINE configs[4] on one GPU: SwapFusionEncoder (64 ch, 8 agents, window 8, depth 3, mask) on the
                (1, 8, 64, 256, 256) voxel-BEV map, with the roofline of its kernels (`bench.py --workload lidar` is this leg alone)"""
                enc = synth.fill_module_(host.SwapFusionEncoder(dict(LIDAR_ARGS)), 0).eval().to(dev)
                x, mask = lidar_inputs(dev, seed=0)
                run = pipeline.CapturedCall(lambda a, m: enc(a, m), x, mask, use_graph=not args.no_graph)
                out = dict(quick(run.step, 3, 20), config="OPV2V-LiDAR FuseBEVT (BASELINE configs[4], one GPU): SwapFusionEncoder(64 ch, "
                           "8 agents, window 8, depth 3, mask) on (1, 8, 64, 256, 256)", algorithmic_gflop=LIDAR_GF)
                out["achieved_tflops_end_to_end"] = round(LIDAR_GF / out["ms_median"], 2)
                out["roofline"] = lidar_roofline(enc, x, mask, args.dtype)
                return out
            def train_step():
                """one optimisation step of train_camera.py:143-179 (forward, VanillaSegLoss, backward, AdamW) of the
                same corpbevt.yaml model on the same 5-agent frame, bf16 autocast, replayed from a captured HIP graph
                (host.CapturedTrainStep; tools/train_graph_probe.py is this leg with its eager and fp32 counterparts)"""
                from cobevt_amd.host.train_graph import CapturedTrainStep
                tm = synth.fill_module_(host.CorpBEVT(copy.deepcopy(cfg)), 0).train().to(dev)
                tb = {k: v.clone() for k, v in batch.items() if torch.is_tensor(v)}
                shp = outs[args.dtype]["dynamic_seg"].shape
                tb["gt_dynamic"] = (torch.rand(shp[:2] + shp[3:], device=dev) > 0.9).long()
                tb["gt_static"] = torch.zeros(shp[:2] + shp[3:], device=dev, dtype=torch.long)
                crit = host.VanillaSegLoss({"d_weights": 75.0, "s_weights": 15.0, "l_weights": 50, "d_coe": 2.0, "s_coe": 0.0, "target": "dynamic"})
                opt = torch.optim.AdamW(tm.parameters(), lr=2e-4, capturable=True)
                cap = CapturedTrainStep(tm, lambda o, b: crit(o, b), opt, tb, autocast_dtype=torch.bfloat16)
                q = quick(lambda: cap.step(), 2, 10)
                return dict(q, loss=round(float(cap.step()), 4), config="OPV2V-camera CoBEVT training step: 5 agents x 4 cams 512x512, forward + "
                            "VanillaSegLoss + backward + AdamW under bf16 autocast, one captured HIP graph per step; steps_per_sec = frames_per_sec")
            oc = {}
            safe(oc, "train_step_bf16_autocast", train_step)
            safe(oc, "opv2v_2_agents", two_agents)
            safe(oc, "nuscenes_sinbevt_from_images", lambda: nuscenes(True))
            safe(oc, "nuscenes_sinbevt", lambda: nuscenes(False))
            safe(oc, "lidar_fusebevt", lidar)
            result["other_configs"] = oc
        if not args.no_cpu_baseline:
            base, parity = cpu_baseline_leg(model, cfg, dict(full), outs)
            result["cpu_baseline"] = base
            result["parity"] = parity[args.dtype]
            for k, v in parity.items():
                if k != args.dtype:
                    result["parity_" + k] = v
    if world > 1:
        torch.distributed.barrier()
        torch.cuda.synchronize()
        torch.distributed.destroy_process_group()
    if rank == 0 and isolate_direct:
        # ranks 1.. have left; their GPUs are free for the probe job's ranks
        probe = direct_probe_child(args, world)
        if "error" in probe and "latency_mode_direct_gather" not in probe:
            result["latency_mode_direct_gather"] = probe
        else:
            result["latency_mode_direct_gather"] = probe.get("latency_mode_direct_gather")
            if isinstance(probe.get("all_gather_us"), dict) and isinstance(result.get("all_gather_us"), dict):
                result["all_gather_us"].update({k: v for k, v in probe["all_gather_us"].items() if k.startswith("direct")})
        result["direct_exchange_note"] = ("measured by a second torch.distributed.run job started by rank 0 after the main job "
                                          "(bench.py --direct-probe): isolated from the RCCL legs")
    if rank == 0:
        finish_line(result, world)
        print(json.dumps(result), flush=True)


def finish_line(result, world):
    """top-level copies of the other configs' figures (the driver summary shows top-level keys), every roofline fraction also against
    what THIS box delivers (box_calibration), and the definition of the headline"""
    oc = result.get("other_configs") or {}
    for key, src in (("lidar_fusebevt_frames_per_sec", "lidar_fusebevt"), ("nuscenes_sinbevt_from_images_frames_per_sec", "nuscenes_sinbevt_from_images"),
                     ("opv2v_2_agents_frames_per_sec", "opv2v_2_agents"), ("train_steps_per_sec_bf16_autocast", "train_step_bf16_autocast")):
        if isinstance(oc.get(src), dict) and "frames_per_sec" in oc[src]:
            result[key] = oc[src]["frames_per_sec"]
    for key, src in (("fp32_parity_mode_frames_per_sec", "fp32_parity_mode"), ("fp32_fast_mode_frames_per_sec", "fp32_fast_mode"),
                     ("one_frame_at_a_time_frames_per_sec", "one_frame_at_a_time")):
        if isinstance(result.get(src), dict) and "frames_per_sec" in result[src]:
            result[key] = result[src]["frames_per_sec"]
            tf = result[src].get("three_frames_in_flight")
            if isinstance(tf, dict) and "frames_per_sec" in tf:
                result[key.replace("_frames_per_sec", "_three_in_flight_frames_per_sec")] = tf["frames_per_sec"]
    # the fastest mode INSIDE the north-star's floating-point tolerance (1e-3 rel fp32), in one place: which mode, its rates, its measured error
    cand = [(m, result.get(k), result.get("parity_" + m)) for m, k in (("fp32_fast", "fp32_fast_mode"), ("fp32_split", "fp32_parity_mode"), ("fp32", "fp32_exact_mode"))]
    cand = [(m, q, pr) for m, q, pr in cand if isinstance(q, dict) and isinstance(pr, dict) and "frames_per_sec" in q
            and pr.get("logits_rel_err_vs_oracle") is not None and pr["logits_rel_err_vs_oracle"] <= 1e-3]
    if cand:
        m, q, pr = max(cand, key=lambda t: t[1]["frames_per_sec"])
        result["within_1e-3_mode"] = {"compute_mode": m, "frames_per_sec": q["frames_per_sec"],
                                      "three_frames_in_flight_frames_per_sec": (q.get("three_frames_in_flight") or {}).get("frames_per_sec"),
                                      "logits_rel_err_vs_oracle": pr["logits_rel_err_vs_oracle"],
                                      "logits_rms_rel_err_vs_oracle": pr.get("logits_rms_rel_err_vs_oracle"),
                                      "note": "host.set_compute_dtype(%r); `value` is the bf16 mode (1e-2)" % m}
    cal = result.get("box_calibration") or {}
    ents = [result.get("roofline"), result.get("roofline_fax_attention")] + list(result.get("roofline_other_kernels") or [])
    lid = (oc.get("lidar_fusebevt") or {}).get("roofline") if isinstance(oc.get("lidar_fusebevt"), dict) else None
    for e in ents + list(lid or []):
        if not isinstance(e, dict) or "achieved" not in e:
            continue
        if e.get("bound") == "mfma" and cal.get("mfma_bf16_tflops") and result.get("dtype") == "bf16":
            e["frac_of_box_calibrated_peak"] = round(e["achieved"] / cal["mfma_bf16_tflops"], 4)
        elif e.get("bound") == "hbm" and cal.get("hbm_copy_gbs"):
            e["frac_of_box_calibrated_peak"] = round(e["achieved"] / cal["hbm_copy_gbs"], 4)
        elif e.get("bound") == "valu" and cal.get("sclk_mhz_under_mfma_load"):
            e["frac_of_box_calibrated_peak"] = round(e["achieved"] / (1024 * cal["sclk_mhz_under_mfma_load"] / 4.0 / 1e3), 4)
    if isinstance(result.get("roofline_fax_attention"), dict) and "frac_of_box_calibrated_peak" in result["roofline_fax_attention"]:
        result["roofline_fax_attention"]["useful_mfma_frac_of_box_calibrated_peak"] = result["roofline_fax_attention"]["frac_of_box_calibrated_peak"]
    if result.get("config", {}).get("workload", "").startswith("OPV2V-camera"):
        tp = result.get("mode") == "throughput"
        result["headline_definition"] = (
            "v2 (round 4 on): `value` = whole-job frames/s of the throughput mode at EVERY N (weak scaling: N frames per step, frames in "
            "flight, their agents dealt over the GPUs + one exchange); the one-frame-over-N-GPUs partition is `latency_mode` (frame_latency_ms). "
            "v1 (rounds 1-3, SCALE_r03 and earlier) reported the latency mode as `value` at N > 1 with the throughput mode under "
            "`throughput_mode`: not like-for-like with v2 at N > 1; identical at N = 1." if tp else
            "`--mode latency`: `value` = frames/s of ONE frame over the N GPUs (strong scaling); the throughput mode is not in this line")
        result["headline_version"] = 2
        if tp and world > 1:          # the v1 key, kept as an alias of the headline so that tools written against v1 find the same quantity
            result["throughput_mode"] = {k: result[k] for k in ("value", "unit", "ms_per_step", "ms_per_step_median", "scaling", "mode") if k in result}


if __name__ == "__main__":
    main()
