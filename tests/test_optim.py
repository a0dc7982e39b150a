"""CPU: the float64 Adam / AdamW reference of tests/optim_ref.py (torch's own fp32 step must lie inside its intervals, six planted
faults must leave them), the launch plan and launch trace of host.FusedAdamW, the cosine schedule and the reference's two setup
functions.  No GPU and no built library."""
import copy
import json
import math

import numpy as np
import pytest
import torch

import launch_trace_optim as lto
import optim_ref as ref
from cobevt_amd import host, ops
from cobevt_amd.lib import CobevtHipError

N = 65536
LR, WD, BETAS = 2e-4, 1e-2, (0.9, 0.999)
EPS = (1e-10, 1e-8)
SCALES = (1.0, 1e-3, 1e-6)


def _inputs(scale, seed=0):
    """p, and five gradients: normal times `scale`, every seventh element exactly zero"""
    rng = np.random.RandomState(seed)
    p = rng.standard_normal(N).astype(np.float32)
    gs = []
    for _ in range(5):
        g = (rng.standard_normal(N) * scale).astype(np.float32)
        g[::7] = 0.0
        gs.append(g)
    return p, gs


@pytest.mark.parametrize("adamw", [True, False], ids=["adamw", "adam"])
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("scale", SCALES)
def test_torch_stays_inside_the_intervals(adamw, eps, scale):
    """torch.optim.AdamW / Adam (single-tensor, fp32, CPU) for five steps, each step's interval started from torch's stored values:
    the reference is right and its bound is fair (it was not fitted to the kernel)"""
    p0, gs = _inputs(scale)
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    cls = torch.optim.AdamW if adamw else torch.optim.Adam
    opt = cls([param], lr=LR, betas=BETAS, eps=eps, weight_decay=WD, foreach=False)
    m = v = np.zeros(N, np.float32)
    worst = 0.0
    for k, g in enumerate(gs):
        p = param.detach().numpy().copy()
        want = ref.step_bounds(p, g, m, v, k + 1, LR, BETAS[0], BETAS[1], eps, WD, adamw)
        param.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[param]
        m, v = st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
        for name, got, x, e in (("p", param.detach().numpy(), want[0], want[3]), ("m", m, want[1], want[4]), ("v", v, want[2], want[5])):
            u = ref.used(got, x, e)
            worst = max(worst, u)
            assert u <= 1.0, "step %d: torch's %s uses %.3f of the half-width" % (k + 1, name, u)
    print("torch %s eps %g scale %g: used %.3f" % (cls.__name__, eps, scale, worst))


def _faulted(fault, adamw, eps=1e-8, scale=1e-3, grad_scale=1024.0):
    """two clean emulated steps, then a third with `fault`: -> fraction of the elements with a non-zero gradient that leave the
    interval of p, m or v"""
    p, gs = _inputs(scale, seed=1)
    m = v = np.zeros(N, np.float32)
    kw = dict(lr=LR, beta1=BETAS[0], beta2=BETAS[1], eps=eps, weight_decay=WD, adamw=adamw, grad_scale=grad_scale)
    for k in range(2):
        p, m, v = ref.emulate(p, gs[k] * np.float32(grad_scale), m, v, k, **kw)
    g = gs[2] * np.float32(grad_scale)
    P, M, V, e_p, e_m, e_v = ref.step_bounds(p, g, m, v, 3, **kw)
    p2, m2, v2 = ref.emulate(p, g, m, v, 2, fault=fault, **kw)
    out = ref.outside(p2, P, e_p) | ref.outside(m2, M, e_m) | ref.outside(v2, V, e_v)
    return float(out[g != 0].mean())


def test_emulation_without_a_fault_is_inside():
    for adamw in (True, False):
        assert _faulted(None, adamw) == 0.0


@pytest.mark.parametrize("fault", ref.FAULTS)
def test_planted_fault_leaves_the_interval(fault):
    """each of the six faults, planted in the fp32 emulation of the kernel, leaves the interval on at least half of the elements that
    have a gradient (gradients of scale 1e-3 under a GradScaler factor of 1024, eps 1e-8: the setting in which all six matter)"""
    frac = _faulted(fault, adamw=True)
    print("%s: %.3f of the elements outside" % (fault, frac))
    assert frac >= 0.5
    if fault not in ("l2_in_adamw",):
        assert _faulted(fault, adamw=False) >= 0.5


# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 64, 65, 130])
@pytest.mark.parametrize("size", [1, 4095, 4096, 4097])
def test_adam_groups_covers_every_tensor_once(count, size):
    numels = [size + (i % 3) * 4096 for i in range(count)]
    launches = ops.adam_groups(numels)
    assert len(launches) == math.ceil(count / 64)
    nxt = 0
    for la in launches:
        assert la.first == nxt and 1 <= la.count <= ops.ADAM_MAX_TENSORS and len(la.chunks) == la.count      # order kept, no gap
        for i, c in zip(range(la.first, la.first + la.count), la.chunks):
            # the chunks of a tensor tile its elements exactly once: (c - 1) full chunks and a last one of 1 .. 4096
            assert (c - 1) * ops.ADAM_CHUNK < numels[i] <= c * ops.ADAM_CHUNK
        nxt += la.count
    assert nxt == count


def test_adam_groups_rejects_an_empty_tensor_and_splits_a_huge_grid():
    with pytest.raises(CobevtHipError):
        ops.adam_groups([4, 0])
    big = 4096 * (2 ** 30)
    launches = ops.adam_groups([big, big, 5])                    # two tensors of 2^30 chunks each do not fit one grid
    assert [la.count for la in launches] == [1, 2] and sum(launches[1].chunks) < 2 ** 31


# ----------------------------------------------------------------------------------------------
def test_launch_trace_of_one_step(monkeypatch):
    got = json.loads(json.dumps(lto.trace(monkeypatch.setattr)))
    assert got == lto.read_fixture()
    names = [name for _, name, _ in got]
    want = []
    for n, _, _, _, _ in lto.GROUPS:
        n_grad = n - (1 if n == lto.GROUPS[0][0] else 0)
        want += ["cobevt_adam_prepare"] * math.ceil(n_grad / 448) + ["cobevt_multi_adam"] * math.ceil(n_grad / 64)
    assert names == want and len(got) == 5
    prepares = [args for _, name, args in got if name == "cobevt_adam_prepare"]
    for (n, _, lr, wd, _), args in zip(lto.GROUPS, prepares):
        # steps, n, coef, adamw, beta1, beta2, weight_decay, lr, lr_dev, grad_scale, found_inf
        assert args[1] == len(args[0]) and args[3:8] == [1, 0.9, 0.999, wd, lr]        # lr by value ...
        assert args[8:] == ["null", "null", "null"]                                      # ... and no device word in eager mode
    updates = [args for _, name, args in got if name == "cobevt_multi_adam"]
    assert [a[5] for a in updates] == [64, 35, 30]
    assert [a[10] for a in updates] == [1e-10, 1e-10, 1e-8]
    sizes = [lto.GROUPS[0][1](i) for i in range(100) if i != lto.NO_GRAD]
    assert updates[0][4] == sizes[:64] and updates[1][4] == sizes[64:]


def test_unsupported_arguments_raise():
    w = [torch.nn.Parameter(torch.zeros(4))]
    for kw in ({"amsgrad": True}, {"maximize": True}, {"differentiable": True}, {"betas": (1.0, 0.9)}, {"lr": -1.0}):
        with pytest.raises(CobevtHipError):
            host.FusedAdamW(w, **kw)
    with pytest.raises(CobevtHipError):
        host.FusedAdam(w, decoupled_weight_decay=True)
    opt = host.FusedAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    opt.param_groups[0]["params"][0].grad = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(CobevtHipError):
        opt.step()


# ----------------------------------------------------------------------------------------------
class _Opt(object):
    def __init__(self, lrs):
        self.param_groups = [{"lr": lr} for lr in lrs]


def _closed(t, t_initial, base, lr_min):
    return lr_min + 0.5 * (base - lr_min) * (1.0 + math.cos(math.pi * t / t_initial))


def test_cosine_scheduler():
    opt = _Opt([2e-4, 1e-3])
    s = host.CosineLRScheduler(opt, t_initial=100, lr_min=5e-6, warmup_lr_init=2e-5, warmup_t=10, cycle_limit=1, t_in_epochs=False)
    assert [g["lr"] for g in opt.param_groups] == [2e-5, 2e-5] and [g["initial_lr"] for g in opt.param_groups] == [2e-4, 1e-3]
    s.step(3)
    assert [g["lr"] for g in opt.param_groups] == [2e-5, 2e-5]                   # step(epoch) is inert
    prev = None
    for t in range(10):
        s.step_update(t)
        lr = opt.param_groups[0]["lr"]
        assert lr == pytest.approx(2e-5 + t * (2e-4 - 2e-5) / 10, rel=1e-12)
        assert prev is None or lr > prev
        prev = lr
    for t in (10, 50, 99):
        s.step_update(t)
        assert opt.param_groups[0]["lr"] == pytest.approx(_closed(t, 100, 2e-4, 5e-6), rel=1e-12)
        assert opt.param_groups[1]["lr"] == pytest.approx(_closed(t, 100, 1e-3, 5e-6), rel=1e-12)
    s.step_update(50)
    assert opt.param_groups[0]["lr"] == pytest.approx(5e-6 + 0.5 * (2e-4 - 5e-6), rel=1e-12)      # the midpoint: cos = 0
    for t in (100, 101, 10 ** 6):
        s.step_update(t)
        assert [g["lr"] for g in opt.param_groups] == [5e-6, 5e-6]
    s.step(7)
    assert [g["lr"] for g in opt.param_groups] == [5e-6, 5e-6]
    with pytest.raises(ValueError):
        host.CosineLRScheduler(opt, t_initial=100, cycle_limit=2)


# the optimizer: and lr_scheduler: blocks of every yaml under hypes_yaml/opcamera/ that has them (values as the reference's yaml
# loader reads them: floats), copied here as data
_OPT = {"core_method": "AdamW", "lr": 2e-4, "args": {"eps": 1e-10, "weight_decay": 1e-2}}
_SCHED = {"core_method": "cosineannealwarm", "epoches": 151, "warmup_lr": 2e-5, "warmup_epoches": 10, "lr_min": 5e-6}
YAMLS = {name: (_OPT, dict(_SCHED, epoches=91) if name == "cvt_static" else _SCHED) for name in (
    "corpbevt", "corpbevt_static", "cvt", "cvt_att_fuse", "cvt_att_fuse_static", "cvt_disconet", "cvt_disconet_static", "cvt_fcooper",
    "cvt_fcooper_static", "cvt_static", "cvt_swap_fuse", "cvt_swap_fuse_static", "cvt_v2vnet", "cvt_v2vnet_static", "fax")}


def test_cosine_scheduler_on_corpbevt_yaml_numbers():
    """corpbevt.yaml with 7 iterations an epoch: 70 warm-up steps from 2e-5, the cosine over 1057 steps down to 5e-6"""
    opt = _Opt([2e-4])
    s = host.setup_lr_schedular({"lr_scheduler": YAMLS["corpbevt"][1]}, opt, 7)
    assert isinstance(s, host.CosineLRScheduler) and (s.t_initial, s.warmup_t) == (1057, 70)
    want = {0: 2e-5, 35: 1.1e-4, 69: 2e-5 + 69 * 1.8e-4 / 70, 70: _closed(70, 1057, 2e-4, 5e-6), 528: _closed(528, 1057, 2e-4, 5e-6),
            1056: _closed(1056, 1057, 2e-4, 5e-6), 1057: 5e-6, 2000: 5e-6}
    for t, lr in want.items():
        s.step_update(t)
        assert opt.param_groups[0]["lr"] == pytest.approx(lr, rel=1e-12), t
    assert 1.97e-4 < want[70] < 2e-4 and 5e-6 < want[1056] < 5.001e-6


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(3, 2)
        self.frozen = torch.nn.Parameter(torch.zeros(2), requires_grad=False)


@pytest.mark.parametrize("name", sorted(YAMLS))
def test_setup_functions_on_the_shipped_yaml_blocks(name, monkeypatch):
    opt_block, sched_block = YAMLS[name]
    hypes = {"optimizer": opt_block, "lr_scheduler": sched_block}
    net = _Net()
    cpu = host.setup_optimizer(hypes, net)
    assert type(cpu) is torch.optim.AdamW                       # a CPU model: torch's class, as in the reference
    # what a ROCm model gets (the device test is the parameters' own is_cuda)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    opt = host.setup_optimizer(hypes, net)
    monkeypatch.undo()
    assert type(opt) is host.FusedAdamW
    for o in (cpu, opt):
        g, = o.param_groups
        assert (g["lr"], g["eps"], g["weight_decay"], g["betas"]) == (2e-4, 1e-10, 1e-2, (0.9, 0.999))
        assert [id(p) for p in g["params"]] == [id(net.a.weight), id(net.a.bias)]          # the frozen parameter is left out
    s = host.setup_lr_schedular(hypes, opt, 13)
    assert isinstance(s, host.CosineLRScheduler)
    assert (s.t_initial, s.warmup_t, s.lr_min, s.warmup_lr_init) == (sched_block["epoches"] * 13, 130, 5e-6, 2e-5)
    assert opt.param_groups[0]["lr"] == 2e-5 and opt.param_groups[0]["initial_lr"] == 2e-4


def test_setup_functions_other_names(monkeypatch):
    net = _Net()
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    assert type(host.setup_optimizer({"optimizer": {"core_method": "Adam", "lr": 1e-3}}, net)) is host.FusedAdam
    rms = host.setup_optimizer({"optimizer": {"core_method": "RMSprop", "lr": 1e-3, "args": {"alpha": 0.9}}}, net)
    amsgrad = host.setup_optimizer({"optimizer": {"core_method": "AdamW", "lr": 1e-3, "args": {"amsgrad": True}}}, net)
    monkeypatch.undo()
    assert type(rms) is torch.optim.RMSprop and rms.param_groups[0]["alpha"] == 0.9
    assert type(amsgrad) is torch.optim.AdamW and amsgrad.param_groups[0]["amsgrad"]       # an argument the kernels lack: torch's class
    with pytest.raises(ValueError):
        host.setup_optimizer({"optimizer": {"core_method": "NoSuchOptimizer", "lr": 1e-3}}, net)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    L = torch.optim.lr_scheduler
    assert type(host.setup_lr_schedular({"lr_scheduler": {"core_method": "step", "step_size": 10, "gamma": 0.1}}, opt, 5)) is L.StepLR
    ms = host.setup_lr_schedular({"lr_scheduler": {"core_method": "multistep", "step_size": [15, 30], "gamma": 0.1}}, opt, 5)
    assert type(ms) is L.MultiStepLR and sorted(ms.milestones) == [15, 30]
    ex = host.setup_lr_schedular({"lr_scheduler": {"core_method": "exponential", "gamma": 0.5}}, opt, 5)
    assert type(ex) is L.ExponentialLR and ex.gamma == 0.5
    with pytest.raises(ValueError):
        host.setup_lr_schedular({"lr_scheduler": {"core_method": "nope"}}, opt, 5)


def test_to_device():
    out = host.to_device({"a": [torch.zeros(2), 3, "s"], "b": {"c": torch.ones(1), "d": 1.5}}, "cpu")
    assert out["a"][1:] == [3, "s"] and out["b"]["d"] == 1.5 and out["b"]["c"].device.type == "cpu"


# ----------------------------------------------------------------------------------------------
def test_state_dict_exchange_with_torch(monkeypatch):
    """both directions, on CPU state tensors: torch.optim.AdamW -> FusedAdamW keeps stepping from torch's moments and step count
    (the launch goes to the fake library; what is checked is the state the kernels would be handed), and a FusedAdamW state_dict
    drives torch.optim.AdamW to the same result as torch's own state"""
    import launch_trace as lt
    torch.manual_seed(0)
    w0 = [torch.randn(5), torch.randn(3, 2)]
    grads = [[torch.randn_like(w) for w in w0] for _ in range(3)]

    def fresh(cls, **kw):
        ps = [torch.nn.Parameter(w.clone()) for w in w0]
        return ps, cls(ps, lr=1e-3, eps=1e-8, weight_decay=1e-2, **kw)

    def run(ps, opt, k):
        for p, g in zip(ps, grads[k]):
            p.grad = g.clone()
        opt.step()

    ps_t, torch_opt = fresh(torch.optim.AdamW)
    run(ps_t, torch_opt, 0)
    run(ps_t, torch_opt, 1)
    # torch -> ours
    ps_f, fused = fresh(host.FusedAdamW)
    fused.load_state_dict(copy.deepcopy(torch_opt.state_dict()))      # (a checkpoint: load_state_dict alone shares the tensors)
    rec = lt.Recorder()
    lt.install(monkeypatch.setattr, rec)
    run(ps_f, fused, 2)
    monkeypatch.undo()
    assert [name for _, name, _ in rec.records] == ["cobevt_adam_prepare", "cobevt_multi_adam"]
    for pf, pt in zip(ps_f, ps_t):
        sf, st = fused.state[pf], torch_opt.state[pt]
        assert sf["step"].dtype == torch.float32 and sf["step"].dim() == 0 and float(sf["step"]) == 2.0     # the fake launch moved nothing
        assert torch.equal(sf["exp_avg"], st["exp_avg"]) and torch.equal(sf["exp_avg_sq"], st["exp_avg_sq"])
    assert (fused.param_groups[0]["lr"], fused.param_groups[0]["eps"]) == (1e-3, 1e-8)
    # ours -> torch: a third step from the exchanged state equals torch's own third step
    sd = copy.deepcopy(fused.state_dict())
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    ps_2, torch_2 = fresh(torch.optim.AdamW)
    with torch.no_grad():
        for p2, pt in zip(ps_2, ps_t):
            p2.copy_(pt)
    torch_2.load_state_dict(sd)
    run(ps_2, torch_2, 2)
    run(ps_t, torch_opt, 2)
    for p2, pt in zip(ps_2, ps_t):
        assert torch.equal(p2, pt)
        assert float(torch_2.state[p2]["step"]) == 3.0


def test_c_entry_points_validate_before_any_launch():
    """the real library, no device: null pointers are status 1; counts, ranges and alignment status 2"""
    import ctypes
    from cobevt_amd import lib
    l = lib.load()
    vp = ctypes.c_void_p
    one = (vp * 1)(64)                                   # an aligned non-null address that is never dereferenced: every call below is refused
    many = (vp * 65)(*([64] * 65))
    numel = (ctypes.c_long * 65)(*([8] * 65))
    assert l.cobevt_adam_prepare(None, 1, vp(64), 1, 0.9, 0.999, 0.0, 1e-3, None, None, None, None) == 1
    assert l.cobevt_adam_prepare(one, 1, None, 1, 0.9, 0.999, 0.0, 1e-3, None, None, None, None) == 1
    assert l.cobevt_adam_prepare((vp * 1)(None), 1, vp(64), 1, 0.9, 0.999, 0.0, 1e-3, None, None, None, None) == 1
    assert l.cobevt_adam_prepare(one, 0, vp(64), 1, 0.9, 0.999, 0.0, 1e-3, None, None, None, None) == 2
    assert l.cobevt_adam_prepare(one, 1, vp(68), 1, 0.9, 0.999, 0.0, 1e-3, None, None, None, None) == 2        # coef not 16-byte aligned
    assert l.cobevt_adam_prepare(one, 1, vp(64), 2, 0.9, 0.999, 0.0, 1e-3, None, None, None, None) == 2
    assert l.cobevt_adam_prepare(one, 1, vp(64), 1, 1.0, 0.999, 0.0, 1e-3, None, None, None, None) == 2        # beta1 = 1
    assert l.cobevt_adam_prepare(one, 1, vp(64), 1, 0.9, 0.999, -1.0, 1e-3, None, None, None, None) == 2
    assert l.cobevt_adam_prepare(one, 1, vp(64), 1, 0.9, 0.999, 0.0, -1e-3, None, None, None, None) == 2
    assert l.cobevt_adam_prepare(one, 1, vp(64), 1, 0.9, 0.999, 0.0, float("nan"), None, None, None, None) == 2
    assert l.cobevt_multi_adam(None, one, one, one, numel, 1, vp(64), 1, 0.9, 0.999, 1e-8, None) == 1
    assert l.cobevt_multi_adam(one, one, one, (vp * 1)(None), numel, 1, vp(64), 1, 0.9, 0.999, 1e-8, None) == 1
    assert l.cobevt_multi_adam(one, one, one, one, numel, 1, None, 1, 0.9, 0.999, 1e-8, None) == 1
    assert l.cobevt_multi_adam(many, many, many, many, numel, 65, vp(64), 1, 0.9, 0.999, 1e-8, None) == 2     # more than 64 tensors
    assert l.cobevt_multi_adam(one, one, one, one, numel, 0, vp(64), 1, 0.9, 0.999, 1e-8, None) == 2
    assert l.cobevt_multi_adam(one, one, one, one, (ctypes.c_long * 1)(0), 1, vp(64), 1, 0.9, 0.999, 1e-8, None) == 2
    assert l.cobevt_multi_adam(one, (vp * 1)(66), one, one, numel, 1, vp(64), 1, 0.9, 0.999, 1e-8, None) == 2   # a pointer that is no float address
    assert l.cobevt_multi_adam(one, one, one, one, numel, 1, vp(64), 1, 0.9, 0.999, -1e-8, None) == 2
    with pytest.raises(CobevtHipError):
        lib.call("cobevt_multi_adam", many, many, many, many, numel, 65, vp(64), 1, 0.9, 0.999, 1e-8, None)
