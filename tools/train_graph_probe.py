#!/usr/bin/env python
"""Times cobevt_amd.host.train_graph.CapturedTrainStep (one optimisation step of train_camera.py:143-179 captured into a HIP graph)
against the eager step, fp32 and inside a bf16 autocast region, and the optimizer variants against each other.

History: round 2 measured 47.0 -> 43.9 ms (2 agents, fp32) and kept the class out of the package because replays differed from eager
steps by up to 1.5 % of the update norm at one stride-2 encoder block.  Round 3 traced that kind of difference to isolated ReLU flips
(tools/train_grad_diag.py, tools/bn_flip_probe.py) - two eager runs with 1e-7 perturbations show it too - so the class now
lives in the package with a test that bounds the drift (tests/test_training_gpu.py::test_captured_train_step_follows_eager).

Usage on the GPU box:
  python tools/train_graph_probe.py [agents] [--optimizer torch|torch_fused|fused]     eager vs captured step with that optimizer
  python tools/train_graph_probe.py [agents] --ab                                      the optimizer A/B of DESIGN.md 3x: (a) optimizer.step()
      alone on the corpbevt.yaml parameter set with synthetic gradients as a replayed graph, the three variants alternated, and the
      node count of each graph; (b) the whole captured bf16-autocast step, `torch` (the step as it was before host.FusedAdamW) run
      twice for the spread
"""
import argparse
import copy
import os
import re
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cobevt_amd import host, synth  # noqa: E402
from cobevt_amd.host.train_graph import CapturedTrainStep  # noqa: E402

OPTIMIZERS = ("torch", "torch_fused", "fused")
HBM_BYTES_PER_S = 6.3e12        # achievable HBM rate of an MI355X (a float4 copy), the bound of the streaming update


def make_optimizer(kind, params):
    """AdamW as every shipped yaml sets it up (lr 2e-4, eps 1e-10, weight_decay 1e-2)"""
    kw = dict(lr=2e-4, eps=1e-10, weight_decay=1e-2)
    if kind == "fused":
        return host.FusedAdamW(params, **kw)
    if kind == "torch_fused":
        return torch.optim.AdamW(params, capturable=True, fused=True, **kw)
    return torch.optim.AdamW(params, capturable=True, **kw)


def _time(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def _time_window(fn, seconds=0.6):
    """ms per call over a window of at least `seconds` (the call count comes from a short first measurement)"""
    est = _time(fn, 10, 3)
    return _time(fn, max(10, int(seconds * 1e3 / max(est, 1e-3)) + 1), 0)


def _graph_nodes(graph_factory):
    """node count of a captured graph from its DOT dump (None when the runtime writes none)"""
    try:
        g = torch.cuda.CUDAGraph()
        g.enable_debug_mode()
        graph_factory(g)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "graph.dot")
            g.debug_dump(path)
            text = open(path).read()
        return len([ln for ln in text.splitlines() if "label" in ln and "->" not in ln and not re.match(r"\s*(sub)?graph", ln)])
    except Exception as err:        # noqa: BLE001  (a diagnostic: report and go on)
        print("graph node count unavailable: %s" % err)
        return None


def _capture_optimizer_step(opt, graph=None):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                  # creates the state (and FusedAdamW's device words) before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = graph or torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.step()
    torch.cuda.synchronize()
    return g


def optimizer_alone(cfg, rounds=3):
    model = synth.fill_module_(host.CorpBEVT(copy.deepcopy(cfg)), 0).train().cuda()
    params = [p for p in model.parameters() if p.requires_grad]
    elements = sum(p.numel() for p in params)
    gen = torch.Generator(device="cuda").manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 1e-3
    print("(a) optimizer.step() alone, replayed graph: %d tensors, %d elements" % (len(params), elements))
    graphs, opts = {}, {}
    for kind in OPTIMIZERS:
        try:
            opts[kind] = make_optimizer(kind, params)
            graphs[kind] = _capture_optimizer_step(opts[kind])
        except Exception as err:    # noqa: BLE001
            print("  %-12s does not construct / capture here: %s" % (kind, err))
            opts.pop(kind, None)
    nodes = {kind: _graph_nodes(lambda g, o=opts[kind]: _capture_optimizer_step(o, g)) for kind in graphs}
    times = {kind: [] for kind in graphs}
    for _ in range(rounds):         # alternated: box-to-box and minute-to-minute drift hits every variant alike
        for kind, g in graphs.items():
            times[kind].append(_time_window(g.replay))
    for kind in graphs:
        best = min(times[kind])
        line = "  %-12s %s ms per step (rounds: %s), graph nodes: %s" % (kind, "%.4f" % best, ", ".join("%.4f" % t for t in times[kind]), nodes[kind])
        if kind == "fused":
            line += "; 28 B x %d / %.4f ms = %.2f TB/s = %.0f %% of %.1f TB/s (the whole graph: prepare + update launches and their boundaries)" % (
                elements, best, 28.0 * elements / (best * 1e-3) / 1e12, 100.0 * 28.0 * elements / (best * 1e-3) / HBM_BYTES_PER_S, HBM_BYTES_PER_S / 1e12)
        print(line)


def _frame(cfg, agents):
    model = synth.fill_module_(host.CorpBEVT(copy.deepcopy(cfg)), 0).train().cuda()
    batch = {k: v.cuda() for k, v in synth.opv2v_batch(agents=agents).items()}
    with torch.no_grad():
        shp = model.eval()(dict(batch))["dynamic_seg"].shape
    batch["gt_dynamic"] = (torch.rand(shp[:2] + shp[3:], device="cuda") > 0.9).long()
    batch["gt_static"] = torch.zeros(shp[:2] + shp[3:], device="cuda", dtype=torch.long)
    del model
    return batch


def whole_step(cfg, agents, crit, batch):
    print("(b) whole captured bf16-autocast step, %d agents; `torch` = the step before host.FusedAdamW, run twice for the spread" % agents)
    results = []
    for kind in ("torch", "fused", "torch_fused", "torch"):
        model = synth.fill_module_(host.CorpBEVT(copy.deepcopy(cfg)), 0).train().cuda()
        try:
            opt = make_optimizer(kind, [p for p in model.parameters() if p.requires_grad])
            cap = CapturedTrainStep(model, lambda o, b: crit(o, b), opt, batch, autocast_dtype=torch.bfloat16)
        except Exception as err:    # noqa: BLE001
            print("  %-12s does not construct / capture here: %s" % (kind, err))
            continue
        t = _time_window(lambda: cap.step(), 1.0)
        results.append((kind, t))
        print("  %-12s %.3f ms per step, loss %.4f" % (kind, t, float(cap.step())))
        del cap, opt, model
    base = [t for k, t in results if k == "torch"]
    if len(base) == 2:
        spread = abs(base[0] - base[1])
        for kind, t in results:
            if kind != "torch":
                d = t - sum(base) / 2
                print("  %-12s %+.3f ms against torch (spread of the two torch runs %.3f ms): %s" % (
                    kind, d, spread, "no difference" if abs(d) <= spread else ("faster" if d < 0 else "slower")))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("agents", nargs="?", type=int, default=2)
    ap.add_argument("--optimizer", choices=OPTIMIZERS, default="torch")
    ap.add_argument("--ab", action="store_true", help="the optimizer A/B: step alone (a) and whole captured step (b)")
    args = ap.parse_args()
    cfg = synth.corpbevt_config()
    crit = host.VanillaSegLoss({"d_weights": 75.0, "s_weights": 15.0, "l_weights": 50, "d_coe": 2.0, "s_coe": 0.0, "target": "dynamic"})
    if args.ab:
        optimizer_alone(cfg)
        whole_step(cfg, args.agents, crit, _frame(cfg, args.agents))
        sys.exit(0)
    batch = _frame(cfg, args.agents)
    out = {}
    for name, dt in (("fp32", None), ("bf16_autocast", torch.bfloat16)):
        model = synth.fill_module_(host.CorpBEVT(copy.deepcopy(cfg)), 0).train().cuda()
        opt = make_optimizer(args.optimizer, [p for p in model.parameters() if p.requires_grad])

        def eager():
            opt.zero_grad(set_to_none=True)
            with torch.enable_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt is not None):
                loss = crit(model(dict(batch)), batch)
            loss.backward()
            opt.step()
        t_eager = _time(eager, 5, 2)
        cap = CapturedTrainStep(model, lambda o, b: crit(o, b), opt, batch, autocast_dtype=dt)
        t_graph = _time(lambda: cap.step(), 10, 2)
        out[name] = {"eager_ms": round(t_eager, 2), "captured_ms": round(t_graph, 2), "loss": round(float(cap.step()), 4)}
        del cap, opt, model
    print("CorpBEVT corpbevt.yaml, %d agents, AdamW (%s) step: %s" % (args.agents, args.optimizer, out))
