"""The LiDAR pillar front end in train() mode on the GPU (csrc/train_pillar.hip through autograd.PillarVfeFn / ScatterRowsFn,
host/training.point_pillar_fusebevt) against the reference fixture gv22 and the test-side restatement tests/pillar_train_ref.py
(itself pinned to the reference's module in train() to 1e-5).

Gates: forward 1e-5 max-rel (the suite's fp32 pillar tolerance; the reference's fp32 arithmetic is 6e-7 from fp64 on such inputs);
parameter gradients 1e-3 of each tensor's scale with test_training_gpu._compare's floor (the suite's training TOL); running mean and
variance 1e-5, num_batches_tracked exact."""
import copy

import pytest
import torch

import cases_pillar as cp
import pillar_ref as pr
import pillar_train_ref as ptr
from cobevt_amd import autograd as ag
from cobevt_amd import host, synth
from cobevt_amd.registry import create_model
from cobevt_amd.synth import fill_module_
from util import assert_close, golden

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL, STAT_TOL = 1e-5, 1e-3, 1e-5
PREFIX = "pillar_vfe.pfn_layers.0."
CASES = [(a, d, True) for a, d in cp.COMBOS] + [(True, False, False)]


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other modules of the suite switch autograd off globally; these tests differentiate"""
    with torch.enable_grad():
        yield


def _fusion():
    f = copy.deepcopy(cp.FUSION)
    f["drop_out"] = 0.0
    return f


def _args(*combo, **kw):
    kw.setdefault("fusion", _fusion())
    return cp.model_args(*combo, **kw)


def _model(dev, *combo, **kw):
    return fill_module_(host.PointPillarFuseBEVT(_args(*combo, **kw)), cp.SEED).train().to(dev)


def _to(vox, dev):
    return {k: v.to(dev) for k, v in vox.items()}


def _check_grads(got, ref, what):
    """got / ref: {name: gradient}; each tensor on its own scale, floored at 1e-3 of the largest reference gradient (_compare's rule)"""
    assert set(got) == set(ref) and len(ref) > 0, (sorted(got), sorted(ref))
    floor = 1e-3 * max(float(t.abs().max()) for t in ref.values())
    for k, r in ref.items():
        g = got[k]
        assert g is not None, "no gradient for " + k
        g, r = g.detach().double().cpu(), r.detach().double().cpu()
        assert torch.isfinite(g).all(), k
        err = float((g - r).abs().max()) / max(float(r.abs().max()), floor)
        print("%s d %s: rel err %.3e (gate %.1e)" % (what, k, err, GRAD_TOL))
        assert err <= GRAD_TOL, "%s d %s: rel err %.3e > %.1e" % (what, k, err, GRAD_TOL)


def _check_buffers(pfn, ref, what, steps=1):
    assert_close(pfn.norm.running_mean, ref["norm.running_mean"], STAT_TOL, what + " running_mean")
    assert_close(pfn.norm.running_var, ref["norm.running_var"], STAT_TOL, what + " running_var")
    assert int(pfn.norm.num_batches_tracked) == int(ref["norm.num_batches_tracked"]) == steps


def _grads(pfn):
    return {k: p.grad for k, p in pfn.named_parameters()}


def _front(model, vox, form, record_len, weights=None):
    """one front-end call in `form`; returns (rows of the valid pillars in pillar order (P, 64) - gathered from the canvas in the
    canvas form -, the loss sum(rows * weights))"""
    sc = model.scatter
    if form == "rows":
        rows = model.pillar_vfe(dict(vox))["pillar_features"]
    else:
        canvas, mask = _canvas_call(model, vox, record_len)
        assert canvas.dtype == torch.float32 and tuple(canvas.shape) == (len(record_len), model.max_cav, sc.ny, sc.nx, 64)
        assert torch.equal(mask.cpu(), pr.regroup(torch.zeros(sum(record_len), 1), record_len, model.max_cav)[1])
        rows = canvas.reshape(-1, 64)[_dest(vox["voxel_coords"], record_len, model.max_cav, sc.ny, sc.nx)]
    assert rows.dtype == torch.float32
    loss = None if weights is None else (rows * weights).sum()
    return rows, loss


def _dest(coords, record_len, max_cav, ny, nx):
    """canvas row of every (valid) pillar: slot of its agent after regroup, cell z + y nx + x"""
    slot, off = {}, 0
    for b, r in enumerate(record_len):
        for i in range(r):
            slot[off + i] = b * max_cav + i
        off += r
    c = coords.long().cpu()
    s = torch.tensor([slot[int(n)] for n in c[:, 0]])
    return (s * ny * nx + c[:, 1] + c[:, 2] * nx + c[:, 3]).to(coords.device)


# ---------------------------------------------------------------------------------------------- 1. fixture parity
@pytest.mark.parametrize("form", ["rows", "canvas"])
@pytest.mark.parametrize("use_abs,dist,use_norm", CASES)
def test_fixture_parity(cuda, use_abs, dist, use_norm, form):
    fx = golden("gv22_point_pillar_train")
    name = cp.combo_name(use_abs, dist, use_norm)
    m = _model(cuda, use_abs, dist, use_norm)
    vox = _to(cp.voxels(), cuda)
    ref = torch.from_numpy(fx["pillar_features/" + name])
    w = synth.procedural_input("train.w.pillar_train", tuple(ref.shape), cp.SEED).to(cuda)
    rows, loss = _front(m, vox, form, cp.RECORD_LEN, w)
    loss.backward()
    torch.cuda.synchronize()
    assert_close(rows, ref, FWD_TOL, "train pillar_features %s %s" % (name, form))
    pfn = m.pillar_vfe.pfn_layers[0]
    _check_grads(_grads(pfn), {k.split("/")[-1]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("grad/%s/" % name)},
                 "%s %s" % (name, form))
    if use_norm:
        _check_buffers(pfn, {k.split("/")[-1]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("buffer/%s/" % name)}, name)


# ---------------------------------------------------------------------------------------------- 2. the model
def test_model_trains_against_the_fixture(cuda):
    fx = golden("gv22_point_pillar_train")
    m = create_model({"model": {"core_method": "point_pillar_fusebevt", "args": _args()}})
    assert type(m) is host.PointPillarFuseBEVT
    m = fill_module_(m, cp.SEED).train().to(cuda)
    batch = {"processed_lidar": _to(cp.voxels(), cuda), "record_len": torch.tensor(cp.RECORD_LEN)}
    ref = torch.from_numpy(fx["fused_feature"])
    w = synth.procedural_input("train.w.pillar_fuse", tuple(ref.shape), cp.SEED).to(cuda)
    out = m(dict(batch))["fused_feature"]
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 64, 16, 16)
    loss0 = (out * w).sum()
    loss0.backward()
    torch.cuda.synchronize()
    assert_close(out, ref, FWD_TOL, "train fused_feature")
    _check_grads({k: p.grad for k, p in m.named_parameters()},
                 {k[len("model_grad/"):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("model_grad/")}, "model")
    _check_buffers(m.pillar_vfe.pfn_layers[0], {k[len("model_buffer/" + PREFIX):]: torch.from_numpy(fx[k]) for k in fx.files
                                                if k.startswith("model_buffer/")}, "model")
    # two SGD steps, each 0.1 % of the parameters' norm along the first gradient's scale, reduce the loss
    pn = sum(float(p.detach().double().square().sum()) for p in m.parameters()) ** 0.5
    gn = sum(float(p.grad.double().square().sum()) for p in m.parameters()) ** 0.5
    opt = torch.optim.SGD(m.parameters(), lr=1e-3 * pn / gn)
    losses = [float(loss0.detach())]
    for _ in range(2):
        opt.step()
        opt.zero_grad(set_to_none=True)
        loss = (m(dict(batch))["fused_feature"] * w).sum()
        loss.backward()
        losses.append(float(loss.detach()))
    assert losses[2] < losses[1] < losses[0], losses
    assert int(m.pillar_vfe.pfn_layers[0].norm.num_batches_tracked) == 3


# ---------------------------------------------------------------------------------------------- 3. shapes against the restatement
def _ref_run(sd, args, vox, ok, weights, dtype=torch.float64, training=True):
    """pillar_train_ref on the CPU in `dtype` over the pillars `ok` -> (their rows, parameter leaves + buffers after the step)"""
    cfg = args["pillar_vfe"]
    g = pr.geom(args["voxel_size"], args["lidar_range"])
    p = ptr.params(sd, PREFIX, cfg["use_norm"], dtype)
    vf, npts, coords = vox["voxel_features"].to(dtype), vox["voxel_num_points"], vox["voxel_coords"]
    rows = ptr.pillar_features(p, vf[ok], npts[ok], coords[ok], g, cfg["use_absolute_xyz"], cfg["with_distance"], cfg["use_norm"], training)
    (rows * weights.to(dtype)).sum().backward()
    return rows.detach(), p


def _canvas_call(m, dv, record_len):
    vfe, sc = m.pillar_vfe, m.scatter
    rl = torch.tensor(record_len, dtype=torch.int32, device=dv["voxel_features"].device)
    return ag.pillar_vfe(vfe.pfn_layers[0], dv["voxel_features"], dv["voxel_num_points"], dv["voxel_coords"], vfe.geom(),
                         vfe.use_absolute_xyz, vfe.with_distance, grid=(sc.ny, sc.nx), record_len=rl, max_cav=m.max_cav)


def _shape_case(cuda, counts, t, grid, record_len, max_cav, combo, form, vox=None, tag="shape"):
    """one training step of the front end on the GPU against the fp64 restatement on the CPU, at the module's gates"""
    args = _args(*combo, grid=grid, max_cav=max_cav)
    m = fill_module_(host.PointPillarFuseBEVT(args), cp.SEED).train().to(cuda)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    vox = cp.voxels(counts, t, grid, tag=tag) if vox is None else vox
    p_all = vox["voxel_features"].shape[0]
    w_all = synth.procedural_input("train.w." + tag, (p_all, 64), cp.SEED)
    ok = _ok_mask(args, vox, form, record_len)
    rows_ref, p = _ref_run(sd, args, vox, ok, w_all[ok])
    dv = _to(vox, cuda)
    if form == "rows":
        rows = m.pillar_vfe(dict(dv))["pillar_features"]
        (rows * w_all.to(cuda)).sum().backward()
        got = rows[ok.to(cuda)]
        if bool((~ok).any()):
            assert float(rows[~ok.to(cuda)].abs().max()) == 0.0
    else:
        canvas, _ = _canvas_call(m, dv, record_len)
        got = canvas.reshape(-1, 64)[_dest(dv["voxel_coords"][ok.to(cuda)], record_len, max_cav, grid[0], grid[1])]
        (got * w_all[ok].to(cuda)).sum().backward()
        assert int((canvas != 0).any(-1).sum()) <= int(ok.sum())
    torch.cuda.synchronize()
    what = "%s P%d T%d %s" % (tag, p_all, t, form)
    assert_close(got, rows_ref, FWD_TOL, what + " forward")
    pfn = m.pillar_vfe.pfn_layers[0]
    _check_grads(_grads(pfn), {k: v.grad for k, v in p.items() if v.requires_grad}, what)
    _check_buffers(pfn, p, what)


def _ok_mask(args, vox, form, record_len):
    nx, ny, _ = args["point_pillar_scatter"]["grid_size"]
    if form == "rows":
        return vox["voxel_num_points"] > 0
    return ptr.valid_rows(vox["voxel_coords"], vox["voxel_num_points"], record_len, args["max_cav"], ny, nx)


# (pillars per agent, T, (ny, nx), record_len, max_cav, (use_absolute_xyz, with_distance)): P = 1, 7, 65 (one pillar; fewer than the
# 8 half-waves of a workgroup; more than the 64 pillars of a backward workgroup) x T = 1, 5, 32
SHAPES = {
    "P7_T1": ([4, 3], 1, (5, 7), [2], 2, (True, False)),
    "P65_T1": ([30, 20, 15], 1, (8, 24), [2, 1], 3, (False, True)),
    "P1_T5": ([1], 5, (5, 7), [1], 1, (True, True)),
    "P7_T5": ([3, 2, 2], 5, (5, 7), [2, 1], 3, (False, False)),
    "P1_T32": ([1], 32, (5, 7), [1], 2, (False, False)),
    "P65_T32": ([33, 32], 32, (8, 24), [1, 1], 2, (True, True)),
}


@pytest.mark.parametrize("form", ["rows", "canvas"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shapes_against_restatement(cuda, shape, form):
    counts, t, grid, record_len, max_cav, combo = SHAPES[shape]
    _shape_case(cuda, counts, t, grid, record_len, max_cav, combo, form, tag=shape)


@pytest.mark.parametrize("form", ["rows", "canvas"])
def test_every_pillar_full(cuda, form):
    """every n_p = T: no masked row anywhere, so no relu(shift) term and no zero rows in the Gram sums"""
    vox = cp.voxels([40, 30], 32, (8, 24), dirty=True, tag="full")
    vox["voxel_num_points"] = torch.full_like(vox["voxel_num_points"], 32)
    _shape_case(cuda, [40, 30], 32, (8, 24), [2], 2, (True, False), form, vox=vox, tag="full")


def _padded_batch():
    """4 agents as record_len [3, 1] with max_cav 2: agent 2 regroups to a slot past max_cav.  Skipped rows - agent index -1, n_p = 0,
    y outside the grid, the pillars of agent 2 - sit in front of, between and behind the valid ones."""
    grid, t = (8, 24), 32
    base = cp.voxels([30, 25, 20, 22], t, grid, tag="pad")
    vf, co, n_p = base["voxel_features"], base["voxel_coords"], base["voxel_num_points"]
    p = vf.shape[0]
    pick = torch.arange(0, p, 4)                                            # every fourth pillar gets a skipped twin in front of it
    tw_vf, tw_co, tw_n = vf[pick].clone(), co[pick].clone(), n_p[pick].clone()
    kind = torch.arange(pick.numel()) % 3
    tw_co[kind == 0, 0] = -1
    tw_n[kind == 1] = 0
    tw_co[kind == 2, 2] = grid[0] + 3
    order = torch.cat([torch.arange(p) * 2 + 1, pick * 2])                  # twin of pillar i at 2 i, pillar i at 2 i + 1
    perm = torch.argsort(order)
    cat = lambda a, b: torch.cat([a, b])[perm]                              # noqa: E731
    padded = {"voxel_features": cat(vf, tw_vf), "voxel_coords": cat(co, tw_co), "voxel_num_points": cat(n_p, tw_n)}
    # trailing padding to a fixed P, as a caller pads for graph replay
    k = 19
    padded["voxel_features"] = torch.cat([padded["voxel_features"], torch.zeros(k, t, 4)])
    padded["voxel_coords"] = torch.cat([padded["voxel_coords"], torch.full((k, 4), -1, dtype=co.dtype)])
    padded["voxel_num_points"] = torch.cat([padded["voxel_num_points"], torch.zeros(k, dtype=n_p.dtype)])
    return padded, grid, t, [3, 1], 2


def test_padded_batch_equals_the_batch_without_its_skipped_rows(cuda):
    padded, grid, t, record_len, max_cav = _padded_batch()
    _shape_case(cuda, None, t, grid, record_len, max_cav, (True, False), "canvas", vox=padded, tag="pad")
    ok = _ok_mask(_args(grid=grid, max_cav=max_cav), padded, "canvas", record_len)
    assert int(ok.sum()) == 30 + 25 + 22 and ok.numel() > 140 and int((padded["voxel_coords"][:, 0] == 2).sum()) >= 20
    clean = {k: v[ok] for k, v in padded.items()}
    # the same canvas gradient for both batches: canvas, parameter gradients and updated statistics must be bitwise equal
    wc = synth.procedural_input("train.w.pad.canvas", (len(record_len), max_cav, grid[0], grid[1], 64), cp.SEED).to(cuda)
    res = []
    for vox in (padded, clean):
        m = _model(cuda, True, False, True, grid=grid, max_cav=max_cav)
        canvas, mask = _canvas_call(m, _to(vox, cuda), record_len)
        (canvas * wc).sum().backward()
        torch.cuda.synchronize()
        norm = m.pillar_vfe.pfn_layers[0].norm
        res.append((canvas.detach(), _grads(m.pillar_vfe.pfn_layers[0]), norm.running_mean.clone(), norm.running_var.clone(),
                    int(norm.num_batches_tracked)))
    a, b = res
    assert torch.equal(a[0], b[0]) and float(a[0].abs().max()) > 0
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]) and float(a[1][k].abs().max()) > 0, k
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and a[4] == b[4] == 1


def test_no_valid_pillar_updates_nothing(cuda):
    m = _model(cuda)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    vox = _to(cp.voxels(), cuda)
    vox["voxel_coords"] = vox["voxel_coords"].clone()
    vox["voxel_coords"][:, 0] = -1
    out = m({"processed_lidar": vox, "record_len": torch.tensor(cp.RECORD_LEN)})["fused_feature"]
    out.sum().backward()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    pfn = m.pillar_vfe.pfn_layers[0]
    for k, p in pfn.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0, k
    for k, v in m.state_dict().items():
        if k.startswith(PREFIX + "norm.running") or k.endswith("num_batches_tracked"):
            assert torch.equal(v, before[k]), k


# ---------------------------------------------------------------------------------------------- 4. far range
def test_far_range_statistics(cuda):
    """+-140.8 m in x: x^2 reaches 2e4 and E[z^2] - mean^2 cancels; fp64 restatement"""
    _shape_case(cuda, [1500, 1500], 32, (200, 704), [2], 2, (True, False), "rows", tag="far")


# ---------------------------------------------------------------------------------------------- 5. frozen BatchNorm
@pytest.mark.parametrize("form", ["rows", "canvas"])
def test_frozen_batch_norm(cuda, form):
    """norm.eval() inside a training model: the running statistics are used and stay as they are"""
    args = _args()
    m = _model(cuda)
    pfn = m.pillar_vfe.pfn_layers[0]
    pfn.norm.eval()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    vox = cp.voxels()
    w = synth.procedural_input("train.w.frozen", (300, 64), cp.SEED)
    rows_ref, p = _ref_run(sd, args, vox, torch.ones(300, dtype=torch.bool), w, training=False)
    rows, loss = _front(m, _to(vox, cuda), form, cp.RECORD_LEN, w.to(cuda))
    loss.backward()
    torch.cuda.synchronize()
    assert_close(rows, rows_ref, FWD_TOL, "frozen forward " + form)
    _check_grads(_grads(pfn), {k: v.grad for k, v in p.items() if v.requires_grad}, "frozen " + form)
    for k in ("running_mean", "running_var", "num_batches_tracked"):
        assert torch.equal(getattr(pfn.norm, k).cpu(), sd[PREFIX + "norm." + k]), k


# ---------------------------------------------------------------------------------------------- 6. reproducibility
def test_backward_is_bitwise_reproducible(cuda):
    vox = _to(cp.voxels(), cuda)
    w = synth.procedural_input("train.w.repro", (300, 64), cp.SEED).to(cuda)
    runs = []
    for _ in range(2):
        m = _model(cuda)
        rows, loss = _front(m, vox, "canvas", cp.RECORD_LEN, w)
        loss.backward()
        torch.cuda.synchronize()
        pfn = m.pillar_vfe.pfn_layers[0]
        runs.append((rows.detach(), _grads(pfn), pfn.norm.running_mean.clone(), pfn.norm.running_var.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][3], runs[1][3])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]) and float(runs[0][1][k].abs().max()) > 0, k


# ---------------------------------------------------------------------------------------------- 7. inference after a step
def test_inference_follows_the_updated_statistics(cuda):
    """after a training step, .eval(): the forward equals the restatement folded with the UPDATED running statistics (the folded plan
    is keyed on the buffers' version counters, which the Function bumps after the kernel wrote them)"""
    m = _model(cuda).eval()
    vox = _to(cp.voxels(), cuda)
    with torch.no_grad(), host.compute_dtype(torch.float32):
        stale = m.pillar_vfe(dict(vox))["pillar_features"].clone()          # builds the folded plan on the initial statistics
    m.train()
    rows = m.pillar_vfe(dict(vox))["pillar_features"]
    rows.sum().backward()
    m.eval()
    with torch.no_grad(), host.compute_dtype(torch.float32):
        got = m.pillar_vfe(dict(vox))["pillar_features"]
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    args = _args()
    w, s = pr.fold(sd, PREFIX, True)
    cpu = cp.voxels()
    ref = pr.pillar_features(cpu["voxel_features"], cpu["voxel_num_points"], cpu["voxel_coords"], w, s,
                             pr.geom(args["voxel_size"], args["lidar_range"]), True, False)
    assert_close(got, ref, FWD_TOL, "eval after a training step")
    assert float((got - stale).abs().max()) > 1e-4                          # the step did move the statistics


# ---------------------------------------------------------------------------------------------- 8. the stand-alone scatter
def test_scatter_mirror_backward_gathers(cuda):
    m = _model(cuda)
    vox = _to(cp.voxels(), cuda)
    vox["voxel_coords"] = vox["voxel_coords"].clone()
    vox["voxel_coords"][5, 0] = -1                                           # a skipped row: zero gradient
    rows = torch.randn(300, 64, device=cuda, generator=torch.Generator(cuda).manual_seed(1)).requires_grad_(True)
    sp = m.scatter({"pillar_features": rows, "voxel_coords": vox["voxel_coords"], "batch_size": cp.AGENTS})["spatial_features"]
    assert tuple(sp.shape) == (3, 64, 16, 16)
    g = torch.randn(3, 64, 16, 16, device=cuda, generator=torch.Generator(cuda).manual_seed(2))
    (sp * g).sum().backward()
    ref_rows = rows.detach().cpu().clone().requires_grad_(True)
    ref = pr.scatter(ref_rows, vox["voxel_coords"].cpu(), cp.AGENTS, 16, 16).permute(0, 3, 1, 2)
    (ref * g.cpu()).sum().backward()
    assert torch.equal(sp.detach().cpu(), ref.detach())
    assert torch.equal(rows.grad.cpu(), ref_rows.grad) and float(rows.grad[5].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- 9. the captured step
def test_captured_train_step_follows_eager(cuda):
    """host.CapturedTrainStep on PointPillarFuseBEVT (the voxels sit in the nested 'processed_lidar' dict; the second batch is padded to
    the captured P with rows of agent index -1): three replayed steps against three eager steps from the same state, at the gates of
    test_training_gpu.test_captured_train_step_follows_eager - losses to 5e-3, the accumulated update to 2e-2 of its rms,
    num_batches_tracked exact"""
    full = cp.voxels()
    short = cp.voxels([100, 60, 90], tag="gv21.b")
    pad = 300 - short["voxel_features"].shape[0]
    short = {"voxel_features": torch.cat([short["voxel_features"], torch.zeros(pad, cp.T, 4)]),
             "voxel_coords": torch.cat([short["voxel_coords"], torch.full((pad, 4), -1, dtype=torch.int32)]),
             "voxel_num_points": torch.cat([short["voxel_num_points"], torch.zeros(pad, dtype=torch.int32)])}
    batches = [{"processed_lidar": _to(v, cuda), "record_len": torch.tensor(cp.RECORD_LEN, dtype=torch.int32, device=cuda)} for v in (full, short)]
    w = synth.procedural_input("train.w.pillar_fuse", (2, 64, 16, 16), cp.SEED).to(cuda)
    crit = lambda o, b: (o["fused_feature"] * w).sum()                       # noqa: E731
    models = [_model(cuda) for _ in range(2)]
    init = {k: v.detach().clone() for k, v in models[0].state_dict().items()}
    pn = sum(float(p.detach().double().square().sum()) for p in models[0].parameters()) ** 0.5
    out = models[0](dict(batches[0]))["fused_feature"]
    crit({"fused_feature": out}, None).backward()
    gn = sum(float(p.grad.double().square().sum()) for p in models[0].parameters()) ** 0.5
    models[0].load_state_dict(init)
    opts = [torch.optim.SGD(m.parameters(), lr=1e-3 * pn / gn, momentum=0.9) for m in models]
    steps = 3
    eager = []
    for i in range(steps):
        opts[0].zero_grad(set_to_none=True)
        loss = crit(models[0](dict(batches[i % 2])), batches[i % 2])
        loss.backward()
        opts[0].step()
        eager.append(float(loss.detach()))
    cap = host.CapturedTrainStep(models[1], crit, opts[1], batches[0])
    for k, v in models[1].state_dict().items():
        assert torch.equal(v, init[k]), "state %s changed by the capture" % k
    replayed = [float(cap.step(batches[i % 2])) for i in range(steps)]
    for a, b in zip(eager, replayed):
        assert abs(a - b) <= 5e-3 * max(1.0, abs(a)), (eager, replayed)
    se, sc = models[0].state_dict(), models[1].state_dict()
    num = den = 0.0
    for k in se:
        if k.endswith("num_batches_tracked"):
            assert int(se[k]) == int(sc[k]) == int(init[k]) + steps, k
            continue
        de, dc = (se[k] - init[k]).double(), (sc[k] - init[k]).double()
        num += float(((de - dc) ** 2).sum())
        den += float((de ** 2).sum())
    assert den > 0 and (num / den) ** 0.5 <= 2e-2, (num / den) ** 0.5
