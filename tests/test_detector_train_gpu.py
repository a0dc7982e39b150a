"""GPU: training of the PointPillar detectors - cobevt_deconv_wgrad, the raw transposed convolution and its input gradient and
cobevt_att_fuse_bwd_nhwc at kernel level, host.training.deblock at layer level, BaseBEVBackbone / AttBEVBackbone at module level and
both registry detectors end to end, against tests/detector_train_ref.py.

Kernel-level gates, per element, from the operands as stored:
    wgrad, raw forward, dgrad   K 2^-23 S + 2^-23 |ref|  (S = sum |a| |b|, K = N H W, Cin, s s Cout products: fp32 accumulation in any
                                order; wgrad's fp64 addition of the fp32 chunk partials is inside it)
    att_fuse_bwd                4 x the deviation of fp32 autograd from float64 autograd of att_backbone_ref.att_fusion
                                (tests/golden/gv30_att_fuse_bwd_d32.json), max-norm relative to max |dx_f64|
Layer and module level: float64 autograd of the restatement FORCED to the GPU's own ReLU masks (y > 0).  A quantity's gate is 4 x the
deviation of the CPU fp32 restatement under the same forced masks (max-norm, relative to the float64 maximum); at LAYER level it is
not taken below 2^-20 (about sixteen fp32 roundings lie on the path conv -> statistics -> ReLU -> BatchNorm backward -> dgrad / wgrad
of one layer, and a layer case is one small sample of the CPU's own error); the module level has no floor.  Where the GPU's mask
disagrees with the sign of the float64 pre-activation, that pre-activation lies within 4 x the fp32 restatement's deviation of that
layer's pre-activations; at most 8 such elements per case (the restatement alone gives 0: tests/test_detector_train.py).
Running statistics: 1e-5 relative.

Measured on an MI355X with this file's seeds (`pytest -s` prints every figure; gate in brackets; DESIGN.md §3w carries the same table):
    wgrad / raw / dgrad, six kernel cases               err / bound at most 0.251 / 0.047 / 0.053 (the 1961-pixel case: 31 chunks)
    att_fuse_bwd, 26 cases                              1.1e-07 ... 2.7e-07 (4.6e-07 ... 9.9e-07); one-agent samples 0 (0); large scores 7.1e-06 (2.0e-05)
    deblock layer s = 1, 2, 4, frozen                   running statistics 4.4e-08 (1e-5), 0 mask disagreements
    BaseBEVBackbone / AttBEVBackbone, 9 module cases    worst quantity / gate 0.65 (d blocks.0.2.bias 8.0e-07 (1.24e-06)); running statistics 4.4e-08;
                                                        0 mask disagreements; the same figures under bf16 and fp32_split (the graph is native fp32)
    detectors, eval after one SGD step                  psm / rm 2.1e-07 (1.1e-06) / 4.2e-07 (1.7e-06) intermediate, 3.7e-07 (9.7e-07) / 4.3e-07 (2.5e-06)
                                                        FuseBEVT tail; moved by 0.83 ... 1.03 of the maximum
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import att_backbone_ref as ar
import bev_backbone_ref as br
import cases_labels as cl
import detector_train_ref as dr
import launch_trace_bev_backbone as ltb
from cobevt_amd import autograd as ag
from cobevt_amd import host, lib, ops
from cobevt_amd.host import training
from cobevt_amd.registry import create_loss, create_model
from cobevt_amd.synth import fill_module_

pytestmark = pytest.mark.gpu

FACTOR, FLOOR, MAX_FLIPS = 4.0, 2.0 ** -20, 8
SENTINEL, GUARD = 12345.0, 4096


@pytest.fixture(autouse=True)
def _grad_mode():
    with torch.enable_grad():
        yield


def _guarded(shape, cuda):
    """(view of `shape`, the whole buffer): GUARD sentinel floats behind the view"""
    n = int(np.prod(shape))
    whole = torch.full((n + GUARD,), SENTINEL, device=cuda, dtype=torch.float32)
    return whole[:n].view(shape), whole


def _intact(whole, shape):
    return bool((whole[int(np.prod(shape)):] == SENTINEL).all())


def _check(what, got, ref, s, k):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), what
    bound = dr.accumulation_gate(k, s, ref)
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-30)).max())
    print("%s: max|err| %.3e, max err / bound %.3f, max|ref| %.3f" % (what, float(err.max()), ratio, float(ref.abs().max())))
    assert bool((err <= bound).all()), "%s: max err / bound %.3f" % (what, ratio)


def _rel(got, ref):
    return float((got.double().cpu() - ref.double()).abs().max()) / max(float(ref.double().abs().max()), 1e-300)


# ---------------------------------------------------------------------------------------------- wgrad, raw forward, dgrad
@pytest.mark.parametrize("case", dr.kernel_cases(), ids=lambda c: "s%d_%d_%d_n%d_%dx%d" % c[:6])
def test_deconv_wgrad_raw_dgrad_kernels(cuda, case):
    s, cin, cout, n, h, w = case[:6]
    weight, x, dz = dr.kernel_operands(case)
    xg, zg = x.to(cuda), dz.to(cuda)
    fwd, rows = ops.deconv_train_weights(weight.to(cuda))
    # weight gradient: own buffers with sentinels behind dW and behind the partial sums
    chunks = ops.deconv_wgrad_chunks(n, h, w, cin, cout, s)
    pshape = (chunks, s * s, (cin + 31) // 32 * 32, cout)
    (dw, dw_all), (partial, p_all) = _guarded((cin, cout, s, s), cuda), _guarded(pshape, cuda)
    dims = ops._ints([n, h, w, cin, cout, s, chunks])
    lib.call("cobevt_deconv_wgrad", ops._p(xg), ops._p(zg), ops._p(partial), ops._p(dw), dims, ops._stream(), variant="")
    torch.cuda.synchronize()
    ref, mag = dr.wgrad_f64(x, dz, s)
    print("wgrad %s: %d chunks" % (case[:6], chunks))
    _check("wgrad %s" % (case[:6],), dw, ref, mag, n * h * w)
    assert _intact(dw_all, (cin, cout, s, s)) and _intact(p_all, pshape)
    again = ops.deconv_wgrad(xg, zg, s)
    assert again.is_contiguous() and torch.equal(again, dw), "the weight gradient is not bit-reproducible"
    # raw forward
    z, z_all = _guarded((n, s * h, s * w, cout), cuda)
    lib.call("cobevt_deconv_nhwc", ops._p(xg), ops._p(fwd), ops._p(ops._zero_shift(xg.device, cout)), ops._p(z),
             ops._ints([ops.FP32, n, h, w, cin, cout, fwd.shape[1], s, 0, cout, 0]), ops._stream(), variant="")
    torch.cuda.synchronize()
    ref, mag = dr.raw_f64(x, weight)
    _check("raw %s" % (case[:6],), z, ref, mag, cin)
    assert _intact(z_all, z.shape) and torch.equal(ops.deconv_raw(xg, fwd, cout, s), z)
    # input gradient: the launch of autograd._igemm_rows into a guarded buffer
    dx, dx_all = _guarded((n, h, w, cin), cuda)
    ops._launch_conv2d_nhwc(zg, rows, None, None, None, None, None, dx, h, w, s, s, stride=s, pad=0, variant="")
    torch.cuda.synchronize()
    ref, mag = dr.dgrad_f64(dz, weight)
    _check("dgrad %s" % (case[:6],), dx, ref, mag, s * s * cout)
    assert _intact(dx_all, dx.shape) and torch.equal(ag._igemm_rows(zg, rows, cin, cout, s, s, None, s, 0, h, w), dx)


def test_wgrad_switch_reaches_the_atomics_path(cuda, monkeypatch):
    """autograd.USE_DECONV_WGRAD = False: cobevt_conv_wgrad with the roles swapped gives the same tensor to the same bound"""
    case = dr.kernel_cases()[1]
    s, cin, cout, n, h, w = case[:6]
    weight, x, dz = dr.kernel_operands(case)
    conv = torch.nn.ConvTranspose2d(cin, cout, s, stride=s, bias=False).to(cuda)
    ref, mag = dr.wgrad_f64(x, dz, s)
    for flag in (True, False):
        monkeypatch.setattr(ag, "USE_DECONV_WGRAD", flag)
        conv.weight.grad = None
        with torch.no_grad():
            conv.weight.copy_(weight)
        y = ag.deconv(x.to(cuda).permute(0, 3, 1, 2), conv)
        y.backward(dz.to(cuda).permute(0, 3, 1, 2))
        _check("DeconvFn dW, USE_DECONV_WGRAD=%s" % flag, conv.weight.grad, ref, mag, n * h * w)


# ---------------------------------------------------------------------------------------------- the agent attention's backward
def _att_bwd(x, rl, dout, cuda, rows=None):
    """one cobevt_att_fuse_bwd_nhwc launch into a guarded dx of `rows` (default: x's) agent rows -> (dx on the CPU, sentinels intact)"""
    n, hw, c = x.shape
    rows = n if rows is None else rows
    dx, whole = _guarded((rows, hw, c), cuda)
    xg, rg, gg = x.to(cuda), torch.tensor(rl, dtype=torch.int32, device=cuda), dout.to(cuda)      # held until the launch has run
    lib.call("cobevt_att_fuse_bwd_nhwc", ops._p(xg), ops._p(rg), ops._p(gg), ops._p(dx), len(rl), rows, hw, c, ctypes.c_float(1.0 / c ** 0.5),
             ops._stream(), variant="")
    torch.cuda.synchronize()
    return dx.cpu(), _intact(whole, (rows, hw, c))


@pytest.mark.parametrize("name,x,rl", dr.att_cases(), ids=[c[0] for c in dr.att_cases()])
def test_att_fuse_bwd_kernel(cuda, name, x, rl):
    d = dr.load_att_bwd_d32()[name]
    dout = dr.att_dout(x, rl)
    ref = dr.att_fuse_bwd_ref(x, rl, dout, torch.float64)
    got, intact = _att_bwd(x, rl, dout, cuda)
    assert intact and bool(torch.isfinite(got).all())
    err, gate = _rel(got, ref), FACTOR * d["d32"] / d["max_dx"]
    print("att_fuse_bwd %s: %.3e (gate %.3e)" % (name, err, gate))
    assert err <= gate
    again, _ = _att_bwd(x, rl, dout, cuda)
    assert torch.equal(again, got), "not bit-reproducible"
    n, hw, c = x.shape
    pub = ops.att_fuse_bwd(x.to(cuda).reshape(n, hw, 1, c), torch.tensor(rl, dtype=torch.int32, device=cuda), dout.to(cuda).reshape(len(rl), hw, 1, c))
    assert torch.equal(pub.cpu().reshape(n, hw, c), got)
    if tuple(rl) == (1, 1):
        assert torch.equal(got, dout), "a sample of one agent must return dx = dout exactly"
    # through the Function: the same bits
    xg = x.to(cuda).reshape(n, hw, 1, c).requires_grad_(True)
    ag.att_fuse(xg, torch.tensor(rl, dtype=torch.int32, device=cuda)).backward(dout.to(cuda).reshape(len(rl), hw, 1, c))
    assert torch.equal(xg.grad.cpu().reshape(n, hw, c), got)


def test_att_fuse_bwd_rows_outside_every_sample(cuda):
    """N > sum(record_len): the surplus rows are exactly 0; a too-large record_len is clamped to the rows there are; an empty sample
    owns no row; nothing outside dx is touched in either case"""
    c, hw, rl = ar.MODULE_CASE
    x, key = ar.kernel_input(c, hw, rl), ar.case_key(c, hw, rl, torch.float32)
    d = dr.load_att_bwd_d32()[key]
    gate = FACTOR * d["d32"] / d["max_dx"]
    dout = dr.att_dout(x, rl)
    ref = dr.att_fuse_bwd_ref(x, rl, dout, torch.float64)
    g = torch.Generator().manual_seed(5)
    more = torch.cat([x, torch.rand(2, hw, c, generator=g)])
    got, intact = _att_bwd(more, rl, dout, cuda)
    assert intact and float(got[sum(rl):].abs().max()) == 0.0 and _rel(got[:sum(rl)], ref) <= gate
    big = (rl[0], rl[1] + 4)
    got, intact = _att_bwd(x, big, dout, cuda)
    assert intact and _rel(got, ref) <= gate
    got, intact = _att_bwd(x, (rl[0], rl[1], 7, 1), torch.cat([dout, dout]), cuda)       # samples that start at or past N own nothing
    assert intact and _rel(got, ref) <= gate
    c, hw, rl = ar.EMPTY_SAMPLE_CASE
    x = ar.kernel_input(c, hw, rl)
    got, intact = _att_bwd(torch.cat([x, x[:1]]), rl, dr.att_dout(x, rl), cuda)
    assert intact and float(got[sum(rl):].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- layer level
def _record_masks(monkeypatch):
    """every ag.batch_norm_act with a ReLU appends its output's mask (y > 0), in call order"""
    masks, real = [], ag.batch_norm_act

    def wrapped(x, bn, residual=None, relu=False):
        y = real(x, bn, residual=residual, relu=relu)
        if relu:
            masks.append((y.detach() > 0).cpu())
        return y
    monkeypatch.setattr(ag, "batch_norm_act", wrapped)
    return masks


def _compare(what, got, ref, r32, floor, worst):
    """got (GPU), ref (float64), r32 (fp32 restatement, same masks): err <= max(4 x the restatement's deviation, floor)"""
    err, gate = _rel(got, ref), max(FACTOR * _rel(r32, ref), floor)
    print("    %-44s %.3e (gate %.3e)" % (what, err, gate))
    assert err <= gate, "%s: %.3e over the gate %.3e" % (what, err, gate)
    if err / gate > worst[0]:
        worst[:] = [err / gate, what, err, gate]


def _flips(tape64, tape32, masks):
    """elements where the GPU's mask is not the sign of the float64 pre-activation: each within that layer's forward gate"""
    total = 0
    for a64, a32, m in zip(tape64.pre, tape32.pre, masks):
        bad = (a64 > 0) != m
        total += int(bad.sum())
        if bad.any():
            gate = FACTOR * float((a32.double() - a64).abs().max())
            assert float(a64[bad].abs().max()) <= gate, "a flipped pre-activation of %.3e lies outside the layer's forward gate %.3e" % (
                float(a64[bad].abs().max()), gate)
    assert total <= MAX_FLIPS
    return total


def _deblock_fn(p, s, x, tape):
    return dr.deblock(x, p, "", tape, s)


@pytest.mark.parametrize("s,cin,cout,frozen", [(1, 32, 32, False), (2, 64, 32, False), (4, 24, 64, False), (2, 32, 32, True)])
def test_deblock_layer(cuda, monkeypatch, s, cin, cout, frozen):
    torch.manual_seed(10 * s + cin)
    seq = torch.nn.Sequential(torch.nn.ConvTranspose2d(cin, cout, s, stride=s, bias=False), torch.nn.BatchNorm2d(cout, eps=1e-3, momentum=0.01), torch.nn.ReLU())
    fill_module_(seq, 3)
    seq.train()
    if frozen:
        seq[1].eval()
    x = (torch.rand(2, cin, 5, 7) - 0.5) * 4.0
    sd0 = {k: v.clone() for k, v in seq.state_dict().items()}
    dev = copy.deepcopy(seq).to(cuda)
    masks = _record_masks(monkeypatch)
    xg = x.to(cuda).requires_grad_(True)
    y = training.deblock(dev, xg)
    w = dr.loss_weight(tuple(y.shape), seed=s)
    (y * w.to(cuda).float()).sum().backward()
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and len(masks) == 1
    fr = ["1."] if frozen else []
    r64 = dr.run(sd0, s, x, None, torch.float64, masks, fr, w, fn=_deblock_fn)
    r32 = dr.run(sd0, s, x, None, torch.float32, masks, fr, w, fn=_deblock_fn)
    worst = [0.0, "", 0.0, 0.0]
    print("deblock s=%d %d->%d%s:" % (s, cin, cout, " frozen" if frozen else ""))
    _compare("forward", y.detach(), r64["out"], r32["out"], FLOOR, worst)
    _compare("dx", xg.grad, r64["dx"], r32["dx"], FLOOR, worst)
    for k, p in dev.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32, k
        _compare("d " + k, p.grad, r64["grads"][k], r32["grads"][k], FLOOR, worst)
    flips = _flips(r64["tape"], r32["tape"], masks)
    sd1 = dev.state_dict()
    if frozen:
        assert torch.equal(sd1["1.running_mean"].cpu(), sd0["1.running_mean"]) and torch.equal(sd1["1.running_var"].cpu(), sd0["1.running_var"])
        assert int(sd1["1.num_batches_tracked"]) == int(sd0["1.num_batches_tracked"])
    else:
        rm, rv = r64["tape"].running["1."]
        stat = max(_rel(sd1["1.running_mean"], rm), _rel(sd1["1.running_var"], rv))
        print("    running statistics %.3e (1e-5), mask disagreements %d" % (stat, flips))
        assert stat <= 1e-5 and int(sd1["1.num_batches_tracked"]) == int(sd0["1.num_batches_tracked"]) + 1


# ---------------------------------------------------------------------------------------------- module level
MODULE_CASES = [(name, att) for name in sorted(dr.MODULE_SEEDS) for att in (True, False) if att or name != "compression"]


@pytest.fixture(scope="module")
def module_refs():
    return {}


def _module_step(module, x, rl, w, cuda, masks):
    dev = copy.deepcopy(module).to(cuda)                   # in train() mode, each BatchNorm with the flag the case gave it
    del masks[:]
    xg = x.to(cuda).requires_grad_(True)
    data = {"spatial_features": xg}
    if rl is not None:
        data["record_len"] = torch.tensor(rl)
    out = dev(data)["spatial_features_2d"]
    if w is None:
        w = dr.loss_weight(tuple(out.shape))
    (out * w.to(cuda).float()).sum().backward()
    torch.cuda.synchronize()
    return dev, out.detach(), xg.grad, w, list(masks)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32_split"])
@pytest.mark.parametrize("name,att", MODULE_CASES)
def test_backbone_modules(cuda, monkeypatch, name, att, mode):
    """forward, every parameter gradient, the input gradient, the running statistics and num_batches_tracked of one training step
    through the module's own forward, under each compute dtype (the training graph is fp32 under all of them)"""
    module, cfg, x, rl = dr.module_case(name, att)
    sd0 = {k: v.clone() for k, v in module.state_dict().items()}
    masks = _record_masks(monkeypatch)
    with host.compute_dtype(mode):
        dev, out, dx, w, gmasks = _module_step(module, x, rl, None, cuda, masks)
    assert out.dtype == torch.float32
    r64 = dr.run(sd0, cfg, x, rl, torch.float64, gmasks, (), w)
    r32 = dr.run(sd0, cfg, x, rl, torch.float32, gmasks, (), w)
    assert len(gmasks) == len(r64["tape"].pre)
    worst = [0.0, "", 0.0, 0.0]
    print("%s %s (%s):" % ("AttBEVBackbone" if att else "BaseBEVBackbone", name, mode))
    _compare("forward", out, r64["out"], r32["out"], 0.0, worst)
    _compare("dx", dx, r64["dx"], r32["dx"], 0.0, worst)
    params = dict(dev.named_parameters())
    assert set(params) == set(r64["grads"])
    for k, p in params.items():
        assert p.grad is not None and p.grad.dtype == torch.float32, k
        _compare("d " + k, p.grad, r64["grads"][k], r32["grads"][k], 0.0, worst)
    flips = _flips(r64["tape"], r32["tape"], gmasks)
    sd1, stat = dev.state_dict(), 0.0
    for prefix, (rm, rv) in r64["tape"].running.items():
        stat = max(stat, _rel(sd1[prefix + "running_mean"], rm), _rel(sd1[prefix + "running_var"], rv))
        assert int(sd1[prefix + "num_batches_tracked"]) == int(sd0[prefix + "num_batches_tracked"]) + 1
    print("    worst %s %.3e (%.3e); running statistics %.3e (1e-5); mask disagreements %d" % (worst[1], worst[2], worst[3], stat, flips))
    assert stat <= 1e-5


def test_frozen_batchnorm_inside_a_training_backbone(cuda, monkeypatch):
    """a BatchNorm with its own .training flag off uses its running statistics and leaves them alone"""
    module, cfg, x, rl = dr.module_case("golden", False)
    module.blocks[1][2].eval()
    module.deblocks[2][1].eval()
    frozen = ["blocks.1.2.", "deblocks.2.1."]
    sd0 = {k: v.clone() for k, v in module.state_dict().items()}
    masks = _record_masks(monkeypatch)
    dev, out, dx, w, gmasks = _module_step(module, x, rl, None, cuda, masks)
    r64 = dr.run(sd0, cfg, x, rl, torch.float64, gmasks, frozen, w)
    r32 = dr.run(sd0, cfg, x, rl, torch.float32, gmasks, frozen, w)
    worst = [0.0, "", 0.0, 0.0]
    print("BaseBEVBackbone golden, two frozen BatchNorms:")
    _compare("forward", out, r64["out"], r32["out"], 0.0, worst)
    _compare("dx", dx, r64["dx"], r32["dx"], 0.0, worst)
    for k, p in dev.named_parameters():
        _compare("d " + k, p.grad, r64["grads"][k], r32["grads"][k], 0.0, worst)
    _flips(r64["tape"], r32["tape"], gmasks)
    sd1 = dev.state_dict()
    for prefix in frozen:
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            assert torch.equal(sd1[prefix + k].cpu(), sd0[prefix + k])


def test_mismatched_level_sizes_raise_on_the_device(cuda):
    model = host.BaseBEVBackbone(copy.deepcopy(br.GOLDEN_CFG), 32).to(cuda).train()
    with pytest.raises(lib.CobevtHipError, match="a 10 x 24 input gives 5 x 12, 6 x 12, 8 x 12"):
        model({"spatial_features": torch.zeros(2, 32, 10, 24, device=cuda)})


# ---------------------------------------------------------------------------------------------- the detectors
def _intermediate(cuda):
    args, vox = ar.pillar_args(), ar.pillar_voxels()
    model = fill_module_(create_model({"model": {"core_method": "point_pillar_intermediate", "args": copy.deepcopy(args)}}), 0).to(cuda).train()
    batch = {"processed_lidar": {k: v.to(cuda) for k, v in vox.items()}, "record_len": torch.tensor(ar.PILLAR_RECORD_LEN)}
    return model, batch, args, vox


def _fusebevt(cuda):
    args, vox = ltb.model_args(), ltb.voxels()
    model = fill_module_(create_model({"model": {"core_method": "point_pillar_fusebevt", "args": copy.deepcopy(args)}}), 0).to(cuda).train()
    batch = {"processed_lidar": {k: v.to(cuda) for k, v in vox.items()}, "record_len": torch.tensor([2], dtype=torch.int32, device=cuda)}
    return model, batch, args, vox


def _labels(cuda):
    post = host.VoxelPostprocessor(cl.anchor_params("e2e"), train=True)
    anchors = post.generate_anchor_box()
    gt, mask = cl.case("e2e", anchors)
    return post.generate_label_batch(torch.from_numpy(gt).to(cuda), torch.from_numpy(mask).to(cuda), anchors)


def _by_hand(model, batch, intermediate):
    """the model's train() forward from its parts"""
    lidar = batch["processed_lidar"]
    vfe, sc = model.pillar_vfe, model.scatter
    common = (vfe.pfn_layers[0], lidar["voxel_features"], lidar["voxel_num_points"], lidar["voxel_coords"], vfe.geom(), vfe.use_absolute_xyz, vfe.with_distance)
    dev = lidar["voxel_features"].device
    if intermediate:
        x, _ = ag.pillar_vfe(*common, grid=(sc.ny, sc.nx), num_agents=int(sum(ar.PILLAR_RECORD_LEN)))
        rl = torch.tensor(ar.PILLAR_RECORD_LEN, dtype=torch.int32, device=dev)
        feat = training.att_bev_backbone(model.backbone, x.permute(0, 3, 1, 2), rl)
    else:
        rl = batch["record_len"].to(device=dev, dtype=torch.int32)
        x, cav = ag.pillar_vfe(*common, grid=(sc.ny, sc.nx), record_len=rl, max_cav=model.max_cav)
        b, l, h, w, _ = x.shape
        fused = training.swap_fusion_encoder_blhwc(model.fusion_net, x, cav[:, None, None, None, :].expand(b, h, w, 1, l).contiguous())
        feat = training.base_bev_backbone(model.backbone, fused)
    return ag.conv2d(feat, model.cls_head).float(), ag.conv2d(feat, model.reg_head).float()


@pytest.mark.parametrize("kind", ["point_pillar_intermediate", "point_pillar_fusebevt"])
def test_detectors_train_end_to_end(cuda, kind):
    intermediate = kind == "point_pillar_intermediate"
    model, batch, args, vox = (_intermediate if intermediate else _fusebevt)(cuda)
    twin = copy.deepcopy(model)
    crit = create_loss({"loss": {"core_method": "point_pillar_loss", "args": dict(cl.LOSS_ARGS)}})
    labels = _labels(cuda)

    def evaluate():
        model.eval()
        with torch.no_grad(), host.compute_dtype("fp32"):
            out = {k: v.float().cpu() for k, v in model(batch).items()}
        model.train()
        return out

    first = evaluate()                       # fills the plan cache before the step
    out = model(batch)
    assert sorted(out) == sorted(first) and all(out[k].dtype == torch.float32 and out[k].shape == first[k].shape for k in out)
    assert tuple(out["psm"].shape) == (1, 2, 8, 12) and tuple(out["rm"].shape) == (1, 14, 8, 12)
    psm, rm = _by_hand(twin, batch, intermediate)
    assert torch.equal(out["psm"], psm) and torch.equal(out["rm"], rm), "the model's forward is not its parts"
    total = crit(out, labels)
    total.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(total)) and int(labels["num_pos"][0]) == 4
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, k
    for k, b in model.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == 1, k
    torch.optim.SGD(model.parameters(), lr=0.05).step()
    got = evaluate()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    if intermediate:
        r64 = ar.pillar_intermediate(sd, args, vox, ar.PILLAR_RECORD_LEN, torch.float64)
        r32 = ar.pillar_intermediate(sd, args, vox, ar.PILLAR_RECORD_LEN, torch.float32)
    else:
        # the FuseBEVT encoder has its own tests: the backbone and the heads are restated on the model's own fused map
        def tail(dtype):
            bsd = {k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}
            feat = br.mirror(bsd, args["base_bev_backbone"], got["fused_feature"], dtype)
            return [torch.einsum("nchw,oc->nohw", feat, sd[h + ".weight"].to(dtype).flatten(1)) + sd[h + ".bias"].to(dtype)[None, :, None, None]
                    for h in ("cls_head", "reg_head")]
        r64, r32 = tail(torch.float64), tail(torch.float32)
    for i, k in enumerate(("psm", "rm")):
        d32 = _rel(r32[i], r64[i])
        dev, moved = _rel(got[k], r64[i]), float((got[k] - first[k]).abs().max()) / float(r64[i].abs().max())
        print("%s eval after one step, %s: deviation %.3e (gate %.3e), moved by %.3e" % (kind, k, dev, FACTOR * d32, moved))
        assert dev <= FACTOR * d32 and moved > 100 * FACTOR * d32


@pytest.mark.parametrize("kind", ["point_pillar_intermediate", "point_pillar_fusebevt"])
def test_detectors_under_bf16_autocast(cuda, kind):
    model, batch, _, _ = (_intermediate if kind == "point_pillar_intermediate" else _fusebevt)(cuda)
    crit = create_loss({"loss": {"core_method": "point_pillar_loss", "args": dict(cl.LOSS_ARGS)}})
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = model(batch)
        total = crit(out, _labels(cuda))
    total.backward()
    torch.cuda.synchronize()
    assert out["psm"].dtype == torch.float32 and out["rm"].dtype == torch.float32 and bool(torch.isfinite(total))
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), k
