"""GPU: training of the sparse 3-D backbone - the cobevt_sparse_* training entries at kernel level, autograd.SparseConvBnReluFn at layer
level and host.training.mean_vfe -> voxel_backbone8x -> height_compression at module level, against tests/sparse_train_ref.py (the
train-mode dense restatement and the per-element float64 references of single launches; spconv is not installed).

Kernel-level gates, per element, from the operands as stored:
    raw conv, dgrad, wgrad     K 2^-23 S + 2^-23 |ref|   (S = sum |a| |b| over the products present, K their number: fp32 accumulation in
                                                          any order; wgrad's fp64 addition of the fp32 chunk partials is inside it)
    statistics, running stats  1e-5 (max-norm relative) of float64 computed from the GPU's own z
    BatchNorm backward dz      4 u |gamma rstd| (|g| + (|dbeta| + |xhat dgamma|) / n), u = 2^-24
    dgamma / dbeta             k u sum |terms| with k = the rows of one partial (the sums themselves are fp64: one rounding at the end)

Layer and module level: float64 autograd of the restatement FORCED to the GPU's own ReLU masks (y > 0).  A gradient's gate is
4 x the deviation of the CPU fp32 restatement under the same forced masks (max-norm, relative to max|grad_f64|).  At LAYER level
only - a few dozen rows, one sample of the CPU's own error - it is not taken below 2^-20: about sixteen fp32 roundings lie on the path
conv -> statistics -> ReLU -> BatchNorm backward -> dgrad / wgrad of one layer.  The module level has no floor.  Where the GPU's mask
disagrees with the float64 pre-activation's sign, that pre-activation must lie within the forward gate of that element (layer level:
derived per element, see the test; module level: 4 x the fp32 restatement's deviation of that layer's pre-activations); at most 8
such elements per case (the restatement alone gives 0 on both grids with these seeds).

Measured on an MI355X with this file's seeds (`pytest -s` prints every figure; gate in brackets):
    raw conv / dgrad / wgrad, eleven kernel cases     err / bound at most 0.069 / 0.062 / 0.230
    statistics and running statistics                 below 1e-6 (1e-5), channel offsets of 100-200 standard deviations included
    BatchNorm backward dz, n = 2 ... 2500             err / bound 0.22 ... 0.60
    layer level (7 pairs + frozen)                    forward 2.5e-7 ... 1.5e-6 (1.2e-6 ... 6.6e-6), gradients 1.7e-8 ... 8.2e-7 (9.5e-7 ... 3.2e-6)
    grid (nx, ny, nz)   forward               worst of the 36 gradients                      running statistics   mask disagreements
    (21, 13, 40)        2.553e-06 (1.018e-05)  conv_input.0.weight 2.839e-06 (8.130e-06)      5.68e-08 (1e-5)      0
    (48, 32, 40)        2.323e-06 (9.232e-06)  conv2.2.1.weight    1.732e-06 (4.898e-06)      4.46e-08 (1e-5)      0
    (21, 13, 40) capped 5.200e-06 (1.919e-05)  conv_out.1.weight   4.488e-06 (8.932e-06)      8.53e-08 (1e-5)      0
    the tightest module-level gate, conv_out.1.bias: 4.82e-08 (3.86e-07), 5.21e-08 (3.65e-07), 2.86e-08 (3.43e-07)
The CPU restatement alone (fp32 against float64, free masks) has 0 mask disagreements on both grids with these seeds.
"""
import ctypes

import numpy as np
import pytest
import torch

import sparse_ref as sr
import sparse_train_ref as tr
from cobevt_amd import autograd as ag
from cobevt_amd import host, lib, ops
from cobevt_amd.host import training
from cobevt_amd.lib import CobevtHipError
from cobevt_amd.synth import fill_module_

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FACTOR, FLOOR, MAX_FLIPS = 4.0, 2.0 ** -20, 8
GRIDS = ((21, 13, 40), (48, 32, 40))
NAN = float("nan")


@pytest.fixture(autouse=True)
def _grad_mode():
    """autograd on, whatever an earlier test of the session left as the global grad mode"""
    with torch.enable_grad():
        yield


def _maxrel(got, ref):
    return float((got.double().cpu() - ref.double()).abs().max()) / max(float(ref.double().abs().max()), 1e-300)


def _absmax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _level(x):
    """the level of a SparseConvTensor without features or row_map"""
    return ops.SparseConvTensor(None, x.indices, x.num, x.spatial_shape, x.batch_size, x.workspace)


def _kernel_setup(c, cuda, capacity=None):
    cin_pad = ops.sparse_row_channels(c["cin"], torch.float32)
    rows = torch.zeros((len(c["coords"]), cin_pad))
    rows[:, :c["cin"]] = c["feats"]
    x = ops.sparse_index(c["coords"].to(cuda), sr.KERNEL_BATCH, sr.KERNEL_SHAPE, features=rows.to(cuda))
    level = x if c["subm"] else ops.sparse_downsample(x, c["kernel"], c["stride"], c["padding"], capacity=capacity, workspace=torch.empty(
        ops.sparse_workspace_ints(sr.KERNEL_BATCH, ops.sparse_out_shape(sr.KERNEL_SHAPE, c["kernel"], c["stride"], c["padding"])), dtype=torch.int32,
        device=cuda))
    return x, level, ops.sparse_train_weights(c["weight"].to(cuda))


def _geom(c):
    return c["kernel"], c["stride"], c["padding"], c["subm"]


def _check(what, got, ref, s, k):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), what
    bound = k * 2.0 ** -23 * s + 2.0 ** -23 * ref.abs()
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-30)).max())
    print("%s: max|err| %.3e, max err / bound %.3f, max|ref| %.3f" % (what, float(err.max()), ratio, float(ref.abs().max())))
    assert bool((err <= bound).all()), "%s: max err / bound %.3f" % (what, ratio)


# ---------------------------------------------------------------------------------------------- raw conv, dgrad, wgrad
@pytest.mark.parametrize("name", sorted(sr.KERNEL_CASES))
def test_raw_conv_dgrad_wgrad_kernels(cuda, name):
    c = sr.kernel_case(name)
    x, level, (wf, wt) = _kernel_setup(c, cuda)
    z = ops.sparse_conv_raw(x, level, wf, c["cout"], *_geom(c))
    idx, ref, s, k = tr.raw_reference(c["feats"], c["coords"], sr.KERNEL_BATCH, sr.KERNEL_SHAPE, c["weight"], *_geom(c))
    n = len(idx)
    assert level.num.cpu().tolist() == [n, 0] and torch.equal(level.indices[:n].cpu(), idx) and tuple(z.shape) == (level.capacity, c["cout"])
    _check("raw %s" % name, z[:n], ref, s, k)
    assert _absmax(z[n:]) == 0.0             # rows behind the live count are written as 0
    # a gradient of the output rows, NaN at and past num[0]: never read there
    g = torch.Generator().manual_seed(len(name))
    dz_rows = (torch.rand(n, c["cout"], generator=g) - 0.5) * 2.0
    dz = torch.full((level.capacity, c["cout"]), NAN)
    dz[:n] = dz_rows
    dz = dz.to(cuda)
    dw = ops.sparse_conv_wgrad(x, level, dz, c["cin"], *_geom(c))
    wref, ws, wk = tr.wgrad_reference(c["feats"], c["coords"], dz_rows, idx, sr.KERNEL_BATCH, sr.KERNEL_SHAPE, c["cin"], *_geom(c))
    assert tuple(dw.shape) == tuple(c["weight"].shape) and dw.is_contiguous()
    _check("wgrad %s" % name, dw, wref, ws, wk)
    if c["cin"] >= 16:
        dx = ops.sparse_conv_dgrad(dz, _level(x), level, wt, c["cin"], *_geom(c))
        didx, dref, ds, dk = tr.dgrad_reference(dz_rows, idx, c["coords"], sr.KERNEL_BATCH, sr.KERNEL_SHAPE, c["weight"], *_geom(c))
        q = len(didx)
        assert torch.equal(x.indices[:q].cpu(), didx) and x.num.cpu().tolist() == [q, 0]
        _check("dgrad %s" % name, dx[:q], dref, ds, dk)
    else:
        with pytest.raises(CobevtHipError, match="cobevt_sparse_conv_dgrad failed"):   # conv_input has no input gradient: the pair is refused
            ops.sparse_conv_dgrad(dz, _level(x), level, torch.zeros(27, 32, 16, device=cuda), 8, *_geom(c))


def test_dgrad_is_exactly_zero_without_a_contributing_output(cuda):
    """the output level keeps 5 rows of its active set: input rows whose outputs were all dropped get exactly 0, the others their sums"""
    c = sr.kernel_case("down_16_32_pad1")
    x, level, (wf, wt) = _kernel_setup(c, cuda, capacity=5)
    torch.cuda.synchronize()
    assert level.num.cpu()[0] == 5 and int(level.num.cpu()[1]) > 20
    dz_rows = (torch.rand(5, 32, generator=torch.Generator().manual_seed(2)) - 0.5) * 2.0
    dx = ops.sparse_conv_dgrad(dz_rows.to(cuda), _level(x), level, wt, 16, *_geom(c))
    didx, dref, ds, dk = tr.dgrad_reference(dz_rows, level.indices[:5].cpu(), c["coords"], sr.KERNEL_BATCH, sr.KERNEL_SHAPE, c["weight"], *_geom(c))
    q = len(didx)
    _check("dgrad onto 5 live outputs", dx[:q], dref, ds, dk)
    none = dk[:, 0] == 0
    assert 0 < int(none.sum()) < q and float(dx[:q].cpu()[none].abs().max()) == 0.0 and _absmax(dx[q:]) == 0.0


def test_wgrad_with_more_rows_than_one_tile_per_chunk_and_a_ragged_last_chunk(cuda):
    """3000 live rows: the chunk length is ceil(ceil(3000 / 64) / 32) * 32 = 64 rows, 47 chunks, the last one of 56 rows; the same bits from
    a larger capacity (the chunking comes from num[0])"""
    g = torch.Generator().manual_seed(9)
    d, h, w = sr.KERNEL_SHAPE
    cells = torch.randperm(sr.KERNEL_BATCH * d * h * w, generator=g)[:3000]
    coords = torch.stack([cells // (d * h * w), cells // (h * w) % d, cells // w % h, cells % w], dim=1).to(torch.int32)
    assert 3000 > ops.SPARSE_ROW_CHUNKS * 32 and 3000 % 64 == 56
    c = dict(sr.kernel_case("subm_16_16"), coords=coords, feats=(torch.rand(3000, 16, generator=g) - 0.5) * 2.0)
    x, level, _ = _kernel_setup(c, cuda)
    dz_rows = (torch.rand(3000, 16, generator=g) - 0.5) * 2.0
    dw = ops.sparse_conv_wgrad(x, level, dz_rows.to(cuda), 16, *_geom(c))
    idx = sr.rows_of(*sr.to_dense(coords, c["feats"], sr.KERNEL_BATCH, sr.KERNEL_SHAPE))[0]
    wref, ws, wk = tr.wgrad_reference(c["feats"], coords, dz_rows, idx, sr.KERNEL_BATCH, sr.KERNEL_SHAPE, 16, *_geom(c))
    _check("wgrad 3000 rows", dw, wref, ws, wk)
    pad = torch.cat([coords, torch.tensor([[-1, 0, 0, 0]] * 1111, dtype=torch.int32)])
    rows = torch.cat([c["feats"], torch.full((1111, 16), NAN)])
    x2 = ops.sparse_index(pad.to(cuda), sr.KERNEL_BATCH, sr.KERNEL_SHAPE, features=rows.to(cuda), workspace=torch.empty_like(x.workspace))
    dz2 = torch.cat([dz_rows, torch.full((1111, 16), NAN)]).to(cuda)
    assert x2.capacity == 4111 and torch.equal(ops.sparse_conv_wgrad(x2, x2, dz2, 16, *_geom(c)), dw)


# ---------------------------------------------------------------------------------------------- BatchNorm + ReLU, forward and backward
def _bn_case(n, c, cap, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.full((cap, c), NAN)
    z[:n] = torch.randn(n, c, generator=g) * (0.5 + torch.rand(c, generator=g)) + offset * (1.0 + torch.rand(c, generator=g))
    bn = torch.nn.BatchNorm1d(c, eps=sr.EPS, momentum=tr.MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(0.8 + 0.4 * torch.rand(c, generator=g))
        bn.bias.copy_((torch.rand(c, generator=g) - 0.5) * 0.6)
        bn.running_mean.copy_((torch.rand(c, generator=g) - 0.5) * 0.4)
        bn.running_var.copy_(0.6 + 0.8 * torch.rand(c, generator=g))
    dy = torch.full((cap, c), NAN)
    dy[:n] = torch.randn(n, c, generator=g)
    return z, bn, dy


@pytest.mark.parametrize("n,c,cap,frozen", [(33, 16, 40, False), (300, 64, 300, False), (2500, 128, 2600, False), (129, 32, 200, True), (2, 64, 7, False)])
def test_bn_relu_forward_and_backward_kernels(cuda, n, c, cap, frozen):
    z, bn, dy = _bn_case(n, c, cap, n + c)
    before = (bn.running_mean.clone().double(), bn.running_var.clone().double())
    bn = bn.to(cuda)
    num = torch.tensor([n, 0], dtype=torch.int32, device=cuda)
    zg = z.to(cuda)
    stat, y = ops.sparse_bn_relu(zg, num, bn.weight, bn.bias, bn, frozen)
    mean, var, rstd, scale, shift = tr.bn_reference(z[:n], bn.weight.detach().cpu(), bn.bias.detach().cpu())
    if frozen:
        mean, var = before
        rstd = 1.0 / torch.sqrt(var + sr.EPS)
        scale = bn.weight.detach().cpu().double() * rstd
        shift = bn.bias.detach().cpu().double() - mean * scale
    errs = [_maxrel(stat[j], r) for j, r in enumerate((mean, rstd, scale, shift))]
    rm, rv = before if frozen else tr.running_update(before[0], before[1], mean, var, n)
    errs += [_maxrel(bn.running_mean, rm), _maxrel(bn.running_var, rv)]
    print("bn n %d C %d frozen %d: mean / rstd / scale / shift / running_mean / running_var max-rel %s" % (n, c, frozen, " ".join("%.2e" % e for e in errs)))
    assert max(errs) <= 1e-5 and int(bn.num_batches_tracked) == (0 if frozen else 1)
    if frozen:
        assert torch.equal(bn.running_mean.cpu().double(), before[0]) and torch.equal(bn.running_var.cpu().double(), before[1])
    sc, sh = stat[2].cpu(), stat[3].cpu()
    assert torch.equal(y[:n].cpu(), torch.relu(torch.addcmul(sh, z[:n], sc))) or \
        float((y[:n].cpu().double() - torch.relu(z[:n].double() * sc.double() + sh.double())).abs().max()) <= 2 * U * float((z[:n].abs() * sc.abs() + sh.abs()).max())
    assert _absmax(y[n:]) == 0.0 and 0.05 < float((y[:n] == 0).float().mean()) < 0.95
    # backward, from the operands as stored
    dz, dg, db = ops.sparse_bn_relu_bwd(dy.to(cuda), y, zg, num, bn.weight, stat, frozen)
    m32, r32 = stat[0].cpu().double(), stat[1].cpu().double()
    gam = bn.weight.detach().cpu().double()
    g = dy[:n].double() * (y[:n].cpu() > 0).double()
    xhat = (z[:n].double() - m32) * r32
    dgamma, dbeta = (g * xhat).sum(0), g.sum(0)
    rows = -(-(-(-n // 64)) // 32) * 32                                                # the rows of one partial
    assert bool(((dg.cpu().double() - dgamma).abs() <= rows * U * (g * xhat).abs().sum(0) + 1e-300).all())
    assert bool(((db.cpu().double() - dbeta).abs() <= rows * U * g.abs().sum(0) + 1e-300).all())
    k = gam * r32
    ref = k * g if frozen else k * (g - (dbeta + xhat * dgamma) / n)
    bound = 4 * U * k.abs() * (g.abs() + (0.0 if frozen else (dbeta.abs() + (xhat * dgamma).abs()) / n))
    err = (dz[:n].cpu().double() - ref).abs()
    print("bn backward n %d C %d: max err / bound %.3f" % (n, c, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()) and _absmax(dz[n:]) == 0.0 and bool(torch.isfinite(dz).all())


def test_statistics_of_mean_dominated_channels_and_of_zero_and_one_rows(cuda):
    """channel offsets of 100 standard deviations through the stand-alone statistics call (no y); n = 0 and n = 1 update nothing"""
    n, c = 1000, 32
    z, bn, _ = _bn_case(n, c, n, 5, offset=100.0)
    before = (bn.running_mean.clone().double(), bn.running_var.clone().double())
    bn = bn.to(cuda)
    stat, y = ops.sparse_bn_relu(z.to(cuda), torch.tensor([n, 0], dtype=torch.int32, device=cuda), bn.weight, bn.bias, bn, want_y=False)
    mean, var, rstd, scale, shift = tr.bn_reference(z, bn.weight.detach().cpu(), bn.bias.detach().cpu())
    assert y is None and float((mean.abs() / var.sqrt()).min()) > 30
    rm, rv = tr.running_update(before[0], before[1], mean, var, n)
    errs = [_maxrel(stat[0], mean), _maxrel(stat[1], rstd), _maxrel(stat[2], scale), _maxrel(bn.running_mean, rm), _maxrel(bn.running_var, rv)]
    print("mean-dominated statistics: max-rel %s" % " ".join("%.2e" % e for e in errs))
    assert max(errs) <= 1e-5
    for rows in (0, 1):
        z, bn, dy = _bn_case(rows, 16, 6, 3)
        before = (bn.running_mean.clone(), bn.running_var.clone())
        bn = bn.to(cuda)
        num = torch.tensor([rows, 0], dtype=torch.int32, device=cuda)
        stat, y = ops.sparse_bn_relu(z.to(cuda), num, bn.weight, bn.bias, bn)
        dz, dg, db = ops.sparse_bn_relu_bwd(dy.to(cuda), y, z.to(cuda), num, bn.weight, stat)
        assert all(bool(torch.isfinite(t).all()) for t in (stat, y, dz, dg, db)) and _absmax(y[rows:]) == 0 and _absmax(dz[rows:]) == 0
        if rows:            # one row: xhat = 0 and d beta = g, so d z = k g - k g up to the two roundings the gate allows
            k = (bn.weight.detach() * stat[1]).abs()
            assert bool((dz[0].abs() <= 4 * U * k * 2 * dy[0].to(cuda).abs()).all()) and bool((db == dy[0].to(cuda) * (y[0] > 0)).all())
        assert torch.equal(bn.running_mean.cpu(), before[0]) and torch.equal(bn.running_var.cpu(), before[1]) and int(bn.num_batches_tracked) == 0
        assert torch.equal(stat[1].cpu(), torch.full((16,), float(1.0 / np.sqrt(np.float64(np.float32(sr.EPS)))), dtype=torch.float64).float())
        if rows:
            assert torch.equal(stat[0].cpu(), z[0])


def test_outputs_stay_inside_their_capacity(cuda):
    """every output buffer pre-filled with a sentinel behind its capacity, through the C ABI: sentinels intact, results finite"""
    c = sr.kernel_case("down_16_32_pad1")
    x, level, (wf, wt) = _kernel_setup(c, cuda)
    torch.cuda.synchronize()
    n, cap, guard = int(level.num[0]), level.capacity, 64
    sent = lambda rows, ch: torch.full((rows + guard, ch), 12345.0, device=cuda)      # noqa: E731
    k, s, p = c["kernel"], c["stride"], c["padding"]
    z = sent(cap, 32)
    lib.call("cobevt_sparse_conv_raw", ops._p(x.features), ops._p(x.workspace), ops._p(x.num), ops._p(x.row_map), ops._p(level.indices), ops._p(level.num),
             ops._p(wf), ops._p(z), (ctypes.c_long * 17)(2, *(sr.KERNEL_SHAPE + (x.features.shape[0], cap, 16, 32) + k + s + p)), ops._stream())
    z[n:cap] = NAN
    bn = torch.nn.BatchNorm1d(32, eps=sr.EPS, momentum=tr.MOMENTUM).to(cuda)
    doubles = ops.sparse_train_scratch(16, 32, 27)[1]
    partial = torch.empty(doubles, dtype=torch.float64, device=cuda)
    stat, y, dzb, coef, dgb = sent(0, 4 * 32).view(-1), sent(cap, 32), sent(cap, 32), sent(0, 3 * 32).view(-1), sent(0, 64).view(-1)
    dims = (ctypes.c_long * 4)(cap, 32, 0, doubles)
    lib.call("cobevt_sparse_bn_relu", ops._p(z), ops._p(level.num), ops._p(bn.weight), ops._p(bn.bias), ops._p(bn.running_mean), ops._p(bn.running_var),
             ops._p(bn.num_batches_tracked), ops._p(stat), ops._p(partial), ops._p(y), dims, ctypes.c_float(sr.EPS), ctypes.c_float(0.01), ops._stream())
    dy = torch.full((cap, 32), NAN, device=cuda)
    dy[:n] = 1.0
    lib.call("cobevt_sparse_bn_relu_bwd", ops._p(dy), ops._p(y), ops._p(z), ops._p(level.num), ops._p(bn.weight), ops._p(stat), ops._p(partial), ops._p(dgb),
             ops._p(dgb[32:]), ops._p(coef), ops._p(dzb), dims, ops._stream())
    dx = sent(x.capacity, 16)
    lib.call("cobevt_sparse_conv_dgrad", ops._p(dzb), ops._p(level.workspace), ops._p(level.num), ops._p(x.indices), ops._p(x.num), ops._p(wt), ops._p(dx),
             (ctypes.c_long * 17)(2, *(sr.KERNEL_SHAPE + (x.capacity, cap, 16, 32) + k + s + p)), ops._stream())
    floats = ops.sparse_train_scratch(16, 32, 27)[0]
    wpart, dw = torch.empty(floats, device=cuda), sent(0, 32 * 27 * 16).view(-1)
    lib.call("cobevt_sparse_conv_wgrad", ops._p(x.features), ops._p(x.workspace), ops._p(x.num), ops._p(x.row_map), ops._p(level.indices), ops._p(level.num),
             ops._p(dzb), ops._p(wpart), ops._p(dw), (ctypes.c_long * 19)(2, *(sr.KERNEL_SHAPE + (x.features.shape[0], cap, 16, 16, 32) + k + s + p + (floats,))),
             ops._stream())
    so = level.spatial_shape
    dcanvas = torch.randn(2, so[1], so[2], 32 * so[0], device=cuda)
    dfeat = sent(cap, 32)
    lib.call("cobevt_sparse_dense_bwd", ops._p(dcanvas), ops._p(level.indices), ops._p(level.num), ops._p(dfeat), (ctypes.c_long * 6)(2, *(so + (cap, 32))),
             ops._stream())
    torch.cuda.synchronize()
    for name, t, used in (("z", z, cap * 32), ("stat", stat, 128), ("y", y, cap * 32), ("dz", dzb, cap * 32), ("coef", coef, 96), ("dgamma dbeta", dgb, 64),
                          ("dx", dx, x.capacity * 16), ("dw", dw, 32 * 27 * 16), ("dfeat", dfeat, cap * 32)):
        flat = t.reshape(-1)
        assert bool((flat[used:] == 12345.0).all()), name
        if name != "z":
            assert bool(torch.isfinite(flat[:used]).all()), name
    idx = level.indices[:n].long()
    want = dcanvas.view(2, so[1], so[2], 32, so[0])[idx[:, 0], idx[:, 2], idx[:, 3], :, idx[:, 1]]
    assert torch.equal(dfeat[:n], want) and _absmax(dfeat[n:cap]) == 0.0


# ---------------------------------------------------------------------------------------------- one layer through autograd
class _Conv(object):
    def __init__(self, c, weight):
        self.kernel_size, self.stride, self.padding, self.subm, self.weight = c["kernel"], c["stride"], c["padding"], c["subm"], weight
        self.in_channels, self.out_channels = c["cin"], c["cout"]


def _dense_rows(t, rows, batch, shape):
    n = int(t.num[0])
    return tr._dense_of_rows(t.indices[:n].cpu(), rows[:n].detach().cpu(), batch, shape)


def _flips(what, gpu_mask, levels64, levels32, element_gates=None):
    """the elements whose GPU mask disagrees with the sign of the float64 pre-activation -> their number.  Each must lie within the
    forward gate of that element: element_gates[name] where the caller has one (a single layer: the inputs of the GPU and of the
    float64 run are the same numbers, so the bound is derived per element), else 4 x the fp32 restatement's deviation of that layer's
    pre-activations (the module: a layer's inputs already differ by the error of the layers before it, which has no derivation)"""
    total = 0
    for name, (_, m, pre) in levels64.items():
        act = m.expand_as(pre)
        diff = ((pre > 0).double() != gpu_mask[name]) & act
        gate = FACTOR * float((levels32[name][2].double() - pre)[act].abs().max())
        if bool(diff.any()):
            worst = float(pre[diff].abs().max())
            print("%s %s: %d mask disagreements, worst |pre| %.3e, gate %.3e" % (what, name, int(diff.sum()), worst, gate))
            if element_gates is not None:
                assert bool((pre[diff].abs() <= element_gates[name][diff]).all())
            else:
                assert worst <= gate
        total += int(diff.sum())
    assert total <= MAX_FLIPS, "%s: %d mask disagreements" % (what, total)
    return total


LAYER_CASES = ["subm_4_16", "subm_16_16", "down_16_32_pad1", "rows_tile_plus_1", "two_samples_one_tile", "subm_64_64", "down_64_64_pad011",
               "down_64_128_k311"]


@pytest.mark.parametrize("name,frozen", [(n, False) for n in LAYER_CASES] + [("down_16_32_pad1", True)])
def test_sparse_conv_bn_relu_fn(cuda, name, frozen):
    c = sr.kernel_case(name)
    assert (ops.sparse_row_channels(c["cin"], torch.float32), c["cout"]) in ops.SPARSE_TRAIN_PAIRS
    x, _, _ = _kernel_setup(c, cuda)
    bn = sr.bn_module(c["bn"]).to(cuda)
    bn.momentum = tr.MOMENTUM
    bn.train(not frozen)
    before = (bn.running_mean.clone().cpu().double(), bn.running_var.clone().cpu().double())
    weight = torch.nn.Parameter(c["weight"].to(cuda))
    if c["cin"] >= 16:                                  # the features in the level's own row order: an input gradient is offered
        x = ops.SparseConvTensor(x.features[x.row_map.long()].requires_grad_(True), x.indices, x.num, x.spatial_shape, x.batch_size, x.workspace)
    y = ag.sparse_conv_bn_relu(x, _Conv(c, weight), bn)
    so = y.spatial_shape
    g = torch.Generator().manual_seed(7)
    lw = (torch.rand((sr.KERNEL_BATCH, c["cout"]) + so, generator=g) - 0.5) * 2.0
    n = int(y.num[0])
    idx = y.indices[:n].cpu().long()
    dy = torch.zeros_like(y.features)
    dy[:n] = lw[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]].to(cuda)
    y.features.backward(dy)
    gpu_mask = {"l": _dense_rows(y, (y.features > 0).double(), sr.KERNEL_BATCH, so)}
    fz = (before[0], before[1]) if frozen else None

    def run(dt):
        xd, mask = sr.to_dense(c["coords"], c["feats"], sr.KERNEL_BATCH, sr.KERNEL_SHAPE, dt)
        xd.requires_grad_(True)
        p = [t.detach().to(dt).clone().requires_grad_(True) for t in (c["weight"], c["bn"]["weight"], c["bn"]["bias"])]
        out, m, pre, st = tr.train_layer(xd, mask, p[0], p[1], p[2], *_geom(c), forced=gpu_mask["l"], frozen=fz)
        (out * lw.to(dt)).sum().backward()
        return out.detach(), m, pre.detach(), st, [t.grad for t in p] + [sr.rows_of(xd.grad, mask)[1]]

    o64, m, pre64, st, g64 = run(torch.float64)
    o32, _, pre32, _, g32 = run(torch.float32)
    # the forward gate of one pre-activation gamma rstd (z - mean) + beta: the convolution's K 2^-23 S, mean and rstd stored in fp32 and
    # the two fused multiply-adds (2^-22 (|z| + |mean|) covers them), scaled by |gamma rstd|, and the rounding of the result
    xd64, mask64 = sr.to_dense(c["coords"], c["feats"], sr.KERNEL_BATCH, sr.KERNEL_SHAPE)
    z64 = sr.conv(xd64, c["weight"].double(), c["stride"], c["padding"], c["subm"])
    s64 = sr.conv(xd64.abs(), c["weight"].double().abs(), c["stride"], c["padding"], c["subm"])
    k64 = sr.conv(mask64.double(), torch.ones((1,) + tuple(c["kernel"]) + (1,), dtype=torch.float64), c["stride"], c["padding"], c["subm"]) * c["cin"]
    mean64, var64 = (fz[0], fz[1]) if frozen else (st[0].detach(), st[1].detach())
    v = lambda t: t.double().view(1, -1, 1, 1, 1)         # noqa: E731
    krs = (v(c["bn"]["weight"]) / torch.sqrt(v(var64) + sr.EPS)).abs()
    egate = krs * (k64 * 2.0 ** -23 * s64 + 2.0 ** -22 * (z64.abs() + v(mean64).abs())) + 2.0 ** -23 * pre64.abs()
    flips = _flips(name, gpu_mask, {"l": (o64, m, pre64)}, {"l": (o32, m, pre32)}, {"l": egate})
    assert torch.equal(y.indices[:n].cpu(), sr.rows_of(o64, m)[0]) and n == st[2]
    scale = float(o64.abs().max())
    fwd = float((sr.rows_of(o64, m)[1] - y.features[:n].detach().cpu().double()).abs().max()) / scale
    fgate = max(FACTOR * float((o32.double() - o64).abs().max()) / scale, FLOOR)
    got = [weight.grad, bn.weight.grad, bn.bias.grad] + ([x.features.grad] if c["cin"] >= 16 else [])
    line = []
    for what, a, r64, r32 in zip(("dW", "dgamma", "dbeta", "dx"), got, g64, g32):
        den = float(r64.abs().max())
        dev, gate = _maxrel(a, r64), max(FACTOR * float((r32.double() - r64).abs().max()) / den, FLOOR)
        line.append("%s %.2e (%.2e)" % (what, dev, gate))
        assert dev <= gate, "%s %s: %.3e > %.3e" % (name, what, dev, gate)
    print("layer %s frozen %d: %d rows, %d flips, forward %.2e (%.2e), %s" % (name, frozen, n, flips, fwd, fgate, ", ".join(line)))
    assert fwd <= fgate and 0.05 < float((o64 == 0)[m.expand_as(o64)].double().mean()) < 0.95
    if frozen:
        assert torch.equal(bn.running_mean.cpu().double(), before[0]) and int(bn.num_batches_tracked) == 0
    else:
        rm, rv = tr.running_update(before[0], before[1], st[0].detach(), st[1].detach(), n)
        assert _maxrel(bn.running_mean, rm) <= 1e-5 and _maxrel(bn.running_var, rv) <= 1e-5 and int(bn.num_batches_tracked) == 1


# ---------------------------------------------------------------------------------------------- the module
def _module(grid, cuda, caps=None):
    return fill_module_(host.VoxelBackBone8x({"level_capacities": caps}, 4, list(grid)), 0).to(cuda).train()


def _loss_weights(grid):
    d, h, w = sr.shape_chain(grid)[-1]
    return (torch.rand((2, 128 * d, h, w), generator=torch.Generator().manual_seed(123)) - 0.5) * 2.0


def _step(m, data, lw, cuda, keep=True):
    """one forward + backward -> (batch_dict, spatial_features, {parameter name: gradient})"""
    d = {k: v.to(cuda) for k, v in data.items()}
    d["batch_size"] = 2
    for p in m.parameters():
        p.grad = None
    out = training.height_compression(host.HeightCompression({"feature_num": 256}).train(),
                                      training.voxel_backbone8x(m, training.mean_vfe(host.MeanVFE({}, 4).train(), d), keep_layers=keep))
    sf = out["spatial_features"]
    (sf * lw.to(cuda)).sum().backward()
    return out, sf.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}


def _gpu_masks(out, grid):
    shapes = iter(sr.shape_chain(grid))
    shape, masks, active = next(shapes), {}, {}
    for (name, _, _, _, _, _, subm), t in zip(sr.LAYERS, out["sparse_layer_outputs"]):
        if not subm:
            shape = next(shapes)
        masks[name] = _dense_rows(t, (t.features > 0).double(), 2, shape)
        active[name] = _dense_rows(t, torch.ones(t.capacity, 1), 2, shape) > 0
    return masks, active


def _reference(sd, mean, coords, grid, lw, forced, drops=None):
    res = {}
    for dt in (torch.float64, torch.float32):
        params = tr.params_of(sd, dt)
        levels, sf, stats = tr.backbone_train(params, coords, mean, 2, grid, dt, forced=forced, drops=drops)
        (sf * lw.to(dt)).sum().backward()
        res[dt] = (levels, sf.detach(), stats, {k: p.grad for k, p in params.items()})
    return res


def _compare(what, m, sd0, out, sf, grads, ref, grid):
    (l64, s64, st64, g64), (l32, s32, _, g32) = ref[torch.float64], ref[torch.float32]
    flips = _flips(what, _gpu_masks(out, grid)[0], {k: tuple(t.detach() for t in v) for k, v in l64.items()},
                   {k: tuple(t.detach() for t in v) for k, v in l32.items()})
    scale = float(s64.abs().max())
    fwd, fgate = float((sf.cpu().double() - s64).abs().max()) / scale, FACTOR * float((s32.double() - s64).abs().max()) / scale
    worst = (0.0, None, 0.0, 0.0)
    for k in g64:
        den = float(g64[k].abs().max())
        dev, gate = _maxrel(grads[k], g64[k]), FACTOR * float((g32[k].double() - g64[k]).abs().max()) / den
        print("%s %s: %.3e (gate %.3e)" % (what, k, dev, gate))
        assert dev <= gate, "%s %s: %.3e > %.3e" % (what, k, dev, gate)
        if dev / gate > worst[0]:
            worst = (dev / gate, k, dev, gate)
    stat_err = 0.0
    for name, _, bn in m._layers():
        mean, var, n = st64[name]
        _, bnp = sr.keys(name)
        rm, rv = tr.running_update(sd0[bnp + "running_mean"], sd0[bnp + "running_var"], mean.detach(), var.detach(), n)
        stat_err = max(stat_err, _maxrel(bn.running_mean, rm), _maxrel(bn.running_var, rv))
        assert int(bn.num_batches_tracked) == int(sd0[bnp + "num_batches_tracked"]) + 1
    print("%s: forward %.3e (gate %.3e), %d gradients, worst %s %.3e (gate %.3e), %d mask disagreements, running statistics %.2e"
          % (what, fwd, fgate, len(g64), worst[1], worst[2], worst[3], flips, stat_err))
    assert fwd <= fgate and len(g64) == 36 and stat_err <= 1e-5


@pytest.fixture(scope="module")
def cases():
    return {grid: sr.module_case(grid) for grid in GRIDS}


@pytest.mark.parametrize("grid", GRIDS)
def test_module_forward_and_all_parameter_gradients(cuda, cases, grid):
    data, mean = cases[grid]
    m = _module(grid, cuda)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    lw = _loss_weights(grid)
    out, sf, grads = _step(m, data, lw, cuda)
    assert sf.dtype == torch.float32 and out["spatial_features"].is_contiguous(memory_format=torch.channels_last) and len(grads) == 36
    assert all(g.dtype == torch.float32 and g.is_contiguous() and g.shape == p.shape for g, p in zip(grads.values(), m.parameters()))
    ref = _reference(sd0, mean, data["voxel_coords"].numpy(), grid, lw, _gpu_masks(out, grid)[0])
    sr.assert_case_is_sparse_everywhere({k: (v[0], v[1]) for k, v in ref[torch.float64][0].items()})
    _compare("module %s" % (grid,), m, sd0, out, sf, grads, ref, grid)
    # bitwise: a second run, fitted capacities, a permutation of the input rows, padding rows, the other compute dtypes
    after = {k: v.clone() for k, v in m.state_dict().items()}
    fitted = [int(t.num[0]) for t in [out["sparse_layer_outputs"][i] for i in (0, 2, 5, 8, 11)]]
    assert all(int(t.num[1]) == 0 for t in out["sparse_layer_outputs"])
    perm = torch.randperm(len(data["voxel_coords"]), generator=torch.Generator().manual_seed(4))
    padded = sr.module_case(grid, pad_rows=37)[0]
    runs = {"again": (None, data, None), "fitted capacities": (fitted, data, None), "permuted rows": (None, {k: v[perm] for k, v in data.items()}, None),
            "padding rows": (None, padded, None), "fp32_split": (None, data, "fp32_split"), "bf16": (None, data, "bf16")}
    for what, (caps, dd, mode) in runs.items():
        m2 = _module(grid, cuda, caps)
        m2.load_state_dict(sd0)
        with host.compute_dtype(mode or "fp32"):
            _, sf2, grads2 = _step(m2, dd, lw, cuda, keep=False)
        assert torch.equal(sf2, sf), what
        assert all(torch.equal(grads2[k], grads[k]) for k in grads), what
        assert all(torch.equal(v, after[k]) for k, v in m2.state_dict().items()), what


def test_module_with_a_capacity_below_the_active_set(cuda, cases):
    """conv2's level keeps 300 rows of 438 and conv4's 20 of the 37 that are left: forward, statistics and gradients are those of the restatement without the dropped
    cells (the high end of the cell order), and num[1] counts them"""
    grid = GRIDS[0]
    data, mean = cases[grid]
    m = _module(grid, cuda, [None, 300, None, 20, None])
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    lw = _loss_weights(grid)
    out, sf, grads = _step(m, data, lw, cuda)
    masks, active = _gpu_masks(out, grid)
    drops = {name: ~a for name, a in active.items()}
    ref = _reference(sd0, mean, data["voxel_coords"].numpy(), grid, lw, masks, drops)
    l64 = ref[torch.float64][0]
    dropped = {}
    prev = sr.to_dense(data["voxel_coords"].numpy(), np.zeros((len(mean), 1)), 2, sr.sparse_shape(grid))[1]
    for (name, _, _, k, s, p, subm), t in zip(sr.LAYERS, out["sparse_layer_outputs"]):
        full = sr.out_mask(prev, k, s, p, subm)
        n = int(t.num[0])
        assert torch.equal(t.indices[:n].cpu(), full[:, 0].nonzero().to(torch.int32)[:n]) and int(l64[name][1].sum()) == n     # the LOW end is kept
        dropped[name] = int(full.sum()) - n
        assert subm or int(t.num[1]) == dropped[name]                      # (a SubM layer shares its level's counters)
        prev = l64[name][1]
    assert dropped["conv2.0"] > 0 and dropped["conv4.0"] > 0 and sum(dropped.values()) == dropped["conv2.0"] + dropped["conv4.0"]
    _compare("module %s capped" % (grid,), m, sd0, out, sf, grads, ref, grid)


def test_eval_forward_after_a_step_uses_the_updated_state(cuda, cases):
    """one SGD step on the parameters plus the running-statistics update, then the EVAL forward of the same module: the cached plans
    were rebuilt (the first eval forward, before the step, filled the cache)"""
    grid = GRIDS[0]
    data, mean = cases[grid]
    m = _module(grid, cuda)
    d = {k: v.to(cuda) for k, v in data.items()}
    d["batch_size"] = 2
    vfe, hc = host.MeanVFE({}, 4).eval(), host.HeightCompression({"feature_num": 256}).eval()

    def evaluate():
        m.eval()
        with torch.no_grad(), host.compute_dtype("fp32"):
            y = hc(m(vfe(dict(d))))["spatial_features"].float().cpu()
        m.train()
        return y

    first = evaluate()
    _step(m, data, _loss_weights(grid), cuda, keep=False)
    torch.optim.SGD(m.parameters(), lr=0.05).step()
    got = evaluate()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    _, ref, d32, _ = sr.module_gates(sd, data["voxel_coords"].numpy(), mean, 2, grid)
    dev = float((got.double() - ref).abs().max()) / float(ref.abs().max())
    moved = float((got - first).abs().max()) / float(ref.abs().max())
    print("eval after one step: deviation %.3e (gate %.3e), moved by %.3e" % (dev, FACTOR * d32, moved))
    assert dev <= FACTOR * d32 and moved > 100 * FACTOR * d32


def test_captured_step_replays_on_a_cloud_of_another_size(cuda, cases):
    """forward + backward captured once as a HIP graph (host/train_graph.py's conventions: a side stream, warm-up steps on it, the zero
    pool inside the capture), replayed twice on a second cloud of another size padded to the same P: bitwise the eager step"""
    grid = GRIDS[0]
    data, _ = cases[grid]
    p = len(data["voxel_coords"])
    other, _ = sr.module_case(grid, pad_rows=0)
    keep = torch.randperm(p, generator=torch.Generator().manual_seed(8))[:p - 101]
    other = {k: torch.cat([v[keep], (torch.tensor([[-1, 0, 0, 0]] * 101, dtype=v.dtype) if k == "voxel_coords" else torch.zeros((101,) + v.shape[1:], dtype=v.dtype))])
             for k, v in other.items()}
    lw = _loss_weights(grid).to(cuda)
    m = _module(grid, cuda)
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    static = {k: v.to(cuda).clone() for k, v in data.items()}
    vfe, hc = host.MeanVFE({}, 4).train(), host.HeightCompression({"feature_num": 256}).train()

    def step():
        d = dict(static, batch_size=2)
        sf = training.height_compression(hc, training.voxel_backbone8x(m, training.mean_vfe(vfe, d)))["spatial_features"]
        (sf * lw).sum().backward()
        return sf

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(2):
            step()
        for prm in m.parameters():
            prm.grad = None
        graph = torch.cuda.CUDAGraph()
        ag.begin_capture_zero_pool()
        try:
            with torch.cuda.graph(graph, stream=stream):
                sf_static = step()
        finally:
            ag.end_capture_zero_pool()
    torch.cuda.current_stream().wait_stream(stream)
    grads_static = {k: prm.grad for k, prm in m.named_parameters()}
    for rep in range(2):
        m.load_state_dict(sd0)
        for k, v in other.items():
            static[k].copy_(v.to(cuda))
        graph.replay()
        torch.cuda.synchronize()
        got_sf, got = sf_static.clone(), {k: g.clone() for k, g in grads_static.items()}
        got_state = {k: v.clone() for k, v in m.state_dict().items()}
        m2 = _module(grid, cuda)
        m2.load_state_dict(sd0)
        _, sf2, grads2 = _step(m2, other, lw, cuda, keep=False)
        assert torch.equal(got_sf, sf2) and all(torch.equal(got[k], grads2[k]) for k in got), rep
        assert all(torch.equal(got_state[k], v) for k, v in m2.state_dict().items()), rep


def test_gradient_reaches_the_backbone_from_behind_the_bev_backbone(cuda, cases):
    grid = GRIDS[1]                                     # its last level is 4 x 6 cells: the two deblock outputs share one H x W
    data, _ = cases[grid]
    m = _module(grid, cuda)
    d = {k: v.to(cuda) for k, v in data.items()}
    d["batch_size"] = 2
    out = training.height_compression(host.HeightCompression({"feature_num": 256}).train(),
                                      training.voxel_backbone8x(m, training.mean_vfe(host.MeanVFE({}, 4).train(), d)))
    # host.BaseBEVBackbone's own forward is inference only; its blocks / deblocks are plain nn.Sequentials, run here by torch in train()
    cfg = {"layer_nums": [1, 1], "layer_strides": [1, 2], "num_filters": [32, 64], "upsample_strides": [1, 2], "num_upsample_filter": [32, 32]}
    bev = fill_module_(host.BaseBEVBackbone(cfg, 256), 1).to(cuda).train()
    x, ups = out["spatial_features"], []
    for block, deblock in zip(bev.blocks, bev.deblocks):
        x = block(x)
        ups.append(deblock(x))
    y = torch.cat(ups, dim=1)
    (y.float() ** 2).sum().backward()
    assert all(p.grad is not None for p in bev.parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in m.parameters())
    x3 = out["multi_scale_3d_features"]["x_conv3"]
    assert x3.features.requires_grad and x3.features.dtype == torch.float32
