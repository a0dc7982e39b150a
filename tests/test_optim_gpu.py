"""GPU: host.FusedAdamW / FusedAdam (cobevt_adam_prepare + cobevt_multi_adam, csrc/train_glue.hip) against the float64 intervals of
tests/optim_ref.py - every element of p, exp_avg and exp_avg_sq after a step lies inside the interval started from the values stored
before it - and the behaviour the feature exists for: a captured step that follows the learning rate."""
import copy

import numpy as np
import pytest
import torch

import optim_ref as ref
from cobevt_amd import host, synth
from cobevt_amd.lib import CobevtHipError
from cobevt_amd.synth import fill_module_

pytestmark = pytest.mark.gpu
BETAS = (0.9, 0.999)
SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8199, 70001)
SAMPLE = 1024       # whole-model test: elements checked at either end of every tensor (12 M parameters: the float64 reference of all of them takes 5 s a step)


def _grad(n, gen, scale=1.0):
    """normal, every seventh element exactly zero, every fifth scaled by 1e-4"""
    g = torch.randn(n, generator=gen) * scale
    g[::7] = 0.0
    g[3::5] *= 1e-4
    return g


def _pick(t, sample=None):
    """a tensor's elements as a flat CPU array; with `sample`, only the first and the last `sample` of a longer tensor (the update is
    element-wise: the whole-model test checks the two ends of every tensor, the kernel tests above check every element)"""
    flat = t.detach().reshape(-1)
    if sample is not None and flat.numel() > 2 * sample:
        flat = torch.cat([flat[:sample], flat[-sample:]])
    return flat.cpu().numpy().copy()


def _snapshot(opt, params, sample=None):
    """(p, m, v, step) of every parameter as stored now (zeros where the state does not exist yet)"""
    out = []
    for p in params:
        st = opt.state.get(p, {})
        p0 = _pick(p, sample)
        m = _pick(st["exp_avg"], sample) if "exp_avg" in st else np.zeros_like(p0)
        v = _pick(st["exp_avg_sq"], sample) if "exp_avg_sq" in st else np.zeros_like(p0)
        out.append((p0, m, v, float(st["step"]) if "step" in st else 0.0))
    return out


def _check(opt, params, before, grads, adamw, grad_scale=None, sample=None):
    """every parameter with a gradient inside its interval, its step advanced by one -> the largest used fraction"""
    worst = 0.0
    group_of = {id(p): g for g in opt.param_groups for p in g["params"]}
    for i, (p, (p0, m0, v0, s0), g) in enumerate(zip(params, before, grads)):
        st = opt.state.get(p, {})
        if g is None:
            assert np.array_equal(_pick(p, sample), p0) and (not st or float(st["step"]) == s0), "parameter %d moved without a gradient" % i
            continue
        grp = group_of[id(p)]
        P, M, V, e_p, e_m, e_v = ref.step_bounds(p0, _pick(g, sample), m0, v0, s0 + 1, grp["lr"], grp["betas"][0], grp["betas"][1], grp["eps"],
                                                 grp["weight_decay"], adamw, grad_scale)
        assert float(st["step"]) == s0 + 1, "parameter %d: step %r after %r" % (i, float(st["step"]), s0)
        for name, got, x, e in (("p", p, P, e_p), ("exp_avg", st["exp_avg"], M, e_m), ("exp_avg_sq", st["exp_avg_sq"], V, e_v)):
            u = ref.used(_pick(got, sample), x, e)
            worst = max(worst, u)
            assert u <= 1.0, "parameter %d (%d elements): %s uses %.3f of the half-width" % (i, p.numel(), name, u)
    return worst


def _make(sizes, cuda, gen, view=None):
    params = [torch.randn(n, generator=gen).to(cuda).requires_grad_() for n in sizes]
    if view is not None:          # a view starting one float into a larger buffer: no 16-byte alignment, the element-by-element path
        buf = torch.randn(view + 9, generator=gen).to(cuda)
        params.append(buf[1:1 + view].requires_grad_())
        assert params[-1].data_ptr() % 16 == 4 and params[-1].is_contiguous()
    return params


@pytest.mark.parametrize("eps", [1e-10, 1e-8])
@pytest.mark.parametrize("adamw", [True, False], ids=["adamw", "adam"])
def test_kernel_against_the_reference(cuda, adamw, eps):
    gen = torch.Generator().manual_seed(11)
    params = _make(SIZES, cuda, gen, view=4099)
    skipped = torch.randn(37, generator=gen).to(cuda).requires_grad_()
    params.insert(4, skipped)
    cls = host.FusedAdamW if adamw else host.FusedAdam
    opt = cls(params, lr=2e-4, betas=BETAS, eps=eps, weight_decay=1e-2)
    worst = 0.0
    for k in range(3):
        grads = [None if p is skipped else _grad(p.numel(), gen) for p in params]
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.to(cuda)
        before = _snapshot(opt, params)
        opt.step()
        worst = max(worst, _check(opt, params, before, grads, adamw))
    assert skipped not in opt.state or not opt.state[skipped]
    print("%s eps %g: used %.3f" % (cls.__name__, eps, worst))


@pytest.mark.parametrize("count", [1, 64, 65, 130])
def test_group_boundaries(cuda, count):
    gen = torch.Generator().manual_seed(count)
    params = _make([5] * count, cuda, gen)
    grads = [_grad(5, gen) + 0.5 for _ in params]
    for p, g in zip(params, grads):
        p.grad = g.to(cuda)
    opt = host.FusedAdamW(params, lr=1e-3, eps=1e-8, weight_decay=1e-2)
    before = _snapshot(opt, params)
    opt.step()
    print("%d tensors: used %.3f" % (count, _check(opt, params, before, grads, True)))
    assert all(float(opt.state[p]["step"]) == 1.0 for p in params)


def test_two_param_groups(cuda):
    gen = torch.Generator().manual_seed(5)
    a, b = _make([4097, 3], cuda, gen), _make([5000, 1], cuda, gen)
    opt = host.FusedAdamW([{"params": a, "lr": 1e-3, "weight_decay": 1e-2}, {"params": b, "lr": 2e-5, "weight_decay": 0.3}], eps=1e-8)
    params = a + b
    for k in range(2):
        grads = [_grad(p.numel(), gen) for p in params]
        for p, g in zip(params, grads):
            p.grad = g.to(cuda)
        before = _snapshot(opt, params)
        opt.step()
        print("two groups step %d: used %.3f" % (k + 1, _check(opt, params, before, grads, True)))


def _state_bits(opt, params):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), opt.state[p]["step"].clone()) for p in params]


def _same_bits(a, b):
    return all(torch.equal(x, y) for ta, tb in zip(a, b) for x, y in zip(ta, tb))


def test_grad_scaler_protocol(cuda):
    gen = torch.Generator().manual_seed(9)
    sizes = (5, 4096, 4099)
    init = [torch.randn(n, generator=gen) for n in sizes]
    grads = [[_grad(n, gen) for n in sizes] for _ in range(3)]

    def fresh():
        params = [w.clone().to(cuda).requires_grad_() for w in init]
        return params, host.FusedAdamW(params, lr=1e-3, eps=1e-8, weight_decay=1e-2)

    def run(params, opt, gs, factor=1.0):
        for p, g in zip(params, gs):
            p.grad = (g * factor).to(cuda)
        opt.step()

    # found_inf = 1: nothing moves, bit for bit, the step counters included
    params, opt = fresh()
    run(params, opt, grads[0])
    kept = _state_bits(opt, params)
    opt.grad_scale, opt.found_inf = torch.full((), 4.0, device=cuda), torch.ones((), device=cuda)
    run(params, opt, grads[1])
    del opt.grad_scale, opt.found_inf
    assert _same_bits(kept, _state_bits(opt, params))
    # grad_scale = 1024 on gradients times 1024 = the unscaled run (a power of two), bit for bit
    run(params, opt, grads[1])
    params2, opt2 = fresh()
    run(params2, opt2, grads[0])
    opt2.grad_scale, opt2.found_inf = torch.full((), 1024.0, device=cuda), torch.zeros((), device=cuda)
    run(params2, opt2, grads[1], 1024.0)
    del opt2.grad_scale, opt2.found_inf
    assert _same_bits(_state_bits(opt, params), _state_bits(opt2, params2))
    # a real GradScaler: three iterations, an inf planted in the second - that one changes nothing and halves the scale
    params, opt = fresh()
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    weights = [[g.to(cuda) for g in gs] for gs in grads]
    for k in range(3):
        opt.zero_grad(set_to_none=True)
        with torch.enable_grad():                             # (other modules of the suite switch autograd off globally)
            loss = sum((p * w).sum() for p, w in zip(params, weights[k]))
            scaler.scale(loss).backward()                     # p.grad = weights[k] * scale
        scale = scaler.get_scale()
        if k == 1:
            params[1].grad[17] = float("inf")
        before = _snapshot(opt, params)
        bits = _state_bits(opt, params) if k else None
        scaler.step(opt)
        scaler.update()
        if k == 1:
            assert _same_bits(bits, _state_bits(opt, params)) and scaler.get_scale() == scale / 2 == 512.0
        else:
            assert scaler.get_scale() == scale
            gs = [p.grad.detach().cpu() for p in params]
            print("GradScaler iteration %d: used %.3f" % (k, _check(opt, params, before, gs, True, grad_scale=scale)))
    assert all(float(opt.state[p]["step"]) == 2.0 for p in params)
    assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")


def _captured_step(opt, params, cuda):
    """one eager warm-up step on a side stream (it creates the state), everything put back, then optimizer.step() alone in a graph"""
    p0 = [p.detach().clone() for p in params]
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        opt.step()
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize(cuda)
    with torch.no_grad():
        for p, w in zip(params, p0):
            p.copy_(w)
            for t in opt.state[p].values():
                t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize(cuda)
    return graph


def test_captured_step_follows_the_learning_rate(cuda, monkeypatch):
    """optimizer.step() alone in a HIP graph, replayed with param_group['lr'] = 1e-3, 1e-4, 0: FusedAdamW follows (each replay inside
    the reference's interval for that lr; lr = 0 leaves p bit for bit, the decay factor being 1), torch.optim.AdamW(capturable=True)
    with its float lr does not - the reason this optimizer exists"""
    gen = torch.Generator().manual_seed(21)
    sizes = (5, 4097, 9000)
    init = [torch.randn(n, generator=gen) for n in sizes]
    grads = [_grad(n, gen) for n in sizes]
    lrs = (1e-3, 1e-4, 0.0)

    def fresh(cls, **kw):
        params = [w.clone().to(cuda).requires_grad_() for w in init]
        for p, g in zip(params, grads):
            p.grad = g.to(cuda)
        return params, cls(params, lr=1e-3, betas=BETAS, eps=1e-8, weight_decay=1e-2, **kw)

    params, opt = fresh(host.FusedAdamW)
    with monkeypatch.context() as mp:               # a capture before the state exists is refused (before any launch), not replayed from zero
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(CobevtHipError):
            opt.step()
    graph = _captured_step(opt, params, cuda)
    for k, lr in enumerate(lrs):
        opt.param_groups[0]["lr"] = lr
        opt.sync_hyperparameters()
        before = _snapshot(opt, params)
        graph.replay()
        torch.cuda.synchronize(cuda)
        assert float(opt.lr_words()[0]) == lr
        print("replay %d, lr %g: used %.3f" % (k, lr, _check(opt, params, before, grads, True)))
        if lr == 0.0:
            for p, (p0, m0, _, _) in zip(params, before):
                assert np.array_equal(p.detach().cpu().numpy(), p0)                                    # 1 - 0 * wd = 1, step_size = 0
                assert not np.array_equal(opt.state[p]["exp_avg"].cpu().numpy(), m0)                 # the moments still move
    # torch's capturable AdamW: the float lr is baked into the graph, writing param_group['lr'] between replays changes nothing
    try:
        runs = []
        for change in (True, False):
            tp, topt = fresh(torch.optim.AdamW, capturable=True)
            tgraph = _captured_step(topt, tp, cuda)
            for lr in lrs:
                if change:
                    topt.param_groups[0]["lr"] = lr
                tgraph.replay()
            torch.cuda.synchronize(cuda)
            runs.append([p.detach().clone() for p in tp])
    except RuntimeError as err:                       # torch's class cannot be captured on this machine: only this half is left out
        print("torch.optim.AdamW(capturable=True) could not be captured: %s" % err)
        return
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "torch's captured AdamW followed param_group['lr']"
    assert not any(torch.equal(a.cpu(), p.detach().cpu()) for a, p in zip(runs[0], params))


def test_captured_train_step_with_a_schedule(cuda):
    """host.CapturedTrainStep on the small CorpBEVT with setup_optimizer / setup_lr_schedular ('cosineannealwarm'): four replayed steps
    with step_update between them as in train_camera.py.  The device lr words equal the scheduler's values, and an eager FusedAdamW
    fed the gradients each replay left behind, on a cloned parameter set, agrees within the reference's intervals (backward's atomics
    are not run-to-run identical, so the gradients are recorded, not recomputed)."""
    cfg = synth.corpbevt_small_config()
    cfg["fax"]["self_attn"]["dropout"] = 0.0
    cfg["fax_fusion"]["drop_out"] = 0.0
    batch = {k: v.to(cuda) for k, v in synth.opv2v_batch(agents=2, cams=2, image=128, max_cav=3, seed=3).items()}
    crit = host.VanillaSegLoss({"d_weights": 75.0, "s_weights": 15.0, "l_weights": 50, "d_coe": 2.0, "s_coe": 0.0, "target": "dynamic"})
    model = fill_module_(host.CorpBEVT(copy.deepcopy(cfg)), 1234).train().to(cuda)
    with torch.no_grad():
        shp = model.eval()(dict(batch))["dynamic_seg"].shape
    model.train()
    batch["gt_dynamic"] = (torch.rand(shp[:2] + shp[3:], generator=torch.Generator().manual_seed(50)) > 0.8).long().to(cuda)
    batch["gt_static"] = torch.zeros(shp[:2] + shp[3:], dtype=torch.long, device=cuda)
    hypes = {"optimizer": {"core_method": "AdamW", "lr": 2e-4, "args": {"eps": 1e-10, "weight_decay": 1e-2}},
             "lr_scheduler": {"core_method": "cosineannealwarm", "epoches": 3, "warmup_lr": 2e-5, "warmup_epoches": 1, "lr_min": 5e-6}}
    opt = host.setup_optimizer(hypes, model)
    assert type(opt) is host.FusedAdamW
    params = opt.param_groups[0]["params"]
    clones = [p.detach().clone().requires_grad_() for p in params]
    eager = host.FusedAdamW(clones, lr=2e-4, eps=1e-10, weight_decay=1e-2)
    cap = host.CapturedTrainStep(model, lambda o, b: crit(o, b), opt, batch)
    sched = host.setup_lr_schedular(hypes, opt, 2)           # 2 warm-up steps, then the cosine over 6
    assert opt.param_groups[0]["lr"] == 2e-5
    seen = []
    for i in range(4):
        lr = opt.param_groups[0]["lr"]
        seen.append(lr)
        before = _snapshot(opt, params, SAMPLE)
        loss = cap.step()
        torch.cuda.synchronize(cuda)
        assert np.isfinite(float(loss))
        assert float(opt.lr_words()[0]) == lr
        grads = [None if p.grad is None else p.grad.detach().clone() for p in params]
        u_cap = _check(opt, params, before, grads, True, sample=SAMPLE)
        eager.param_groups[0]["lr"] = lr
        before_e = _snapshot(eager, clones, SAMPLE)
        for q, g in zip(clones, grads):
            q.grad = g
        eager.step()
        u_eager = _check(eager, clones, before_e, grads, True, sample=SAMPLE)
        print("step %d, lr %.3e: captured used %.3f, eager used %.3f" % (i + 1, lr, u_cap, u_eager))
        sched.step_update(i + 1)
    assert seen[0] == 2e-5 and seen[1] == pytest.approx(1.1e-4) and seen[2] > seen[3] > 5e-6
    with_grad = [p for p, g in zip(params, grads) if g is not None]
    assert len(with_grad) > 50
    assert all(float(opt.state[p]["step"]) == 4.0 and bool(torch.isfinite(p).all()) for p in with_grad)
