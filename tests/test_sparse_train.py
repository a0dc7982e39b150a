"""Training of the sparse 3-D backbone (host.training.mean_vfe / voxel_backbone8x / height_compression, autograd.SparseConvBnReluFn /
SparseDenseFn, the cobevt_sparse_* training entries of csrc/sparse_conv.hip) without a device: the train-mode restatement
tests/sparse_train_ref.py against a brute-force per-voxel, per-tap loop with torch.nn.BatchNorm1d (forward, dW by the explicit double
sum, the running-statistics update), the pair tables, the weight lowering, the scratch formula, every refusal of every new C entry
point with host pointers, the host layer's refusals, and the launch trace of one forward + backward."""
import ctypes

import numpy as np
import pytest
import torch

import launch_trace as lt
import sparse_ref as sr
import sparse_train_ref as tr
from cobevt_amd import autograd as ag
from cobevt_amd import host, lib, ops
from cobevt_amd.host import training
from cobevt_amd.lib import CobevtHipError

TYPES = [((3, 3, 3), (1, 1, 1), (1, 1, 1), True), ((3, 3, 3), (2, 2, 2), (1, 1, 1), False), ((3, 3, 3), (2, 2, 2), (0, 1, 1), False),
         ((3, 1, 1), (2, 1, 1), (0, 0, 0), False)]


@pytest.fixture(autouse=True)
def _grad_mode():
    """autograd on, whatever an earlier test of the session left as the global grad mode"""
    with torch.enable_grad():
        yield


# ---------------------------------------------------------------------------------------------- the restatement against brute force
@pytest.mark.parametrize("kernel,stride,padding,subm", TYPES)
def test_train_restatement_is_the_per_voxel_loop_with_batchnorm1d(kernel, stride, padding, subm):
    rng = np.random.RandomState(11)
    batch, shape, cin, cout = 2, (7, 6, 9), 3, 5
    cells = np.stack(np.unravel_index(rng.permutation(batch * 7 * 6 * 9)[:60], (batch,) + shape), axis=1)
    feats = rng.uniform(-1, 1, (60, cin))
    w5 = torch.from_numpy(rng.uniform(-1, 1, (cout,) + kernel + (cin,))).requires_grad_(True)
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, cout)).requires_grad_(True)
    beta = torch.from_numpy(rng.uniform(-0.3, 0.3, cout)).requires_grad_(True)
    so = shape if subm else sr.out_shape(shape, kernel, stride, padding)
    weights = torch.from_numpy(rng.uniform(-1, 1, (batch, cout) + tuple(so)))
    x, mask = sr.to_dense(cells, feats, batch, shape)
    y, m, pre, (mean, var, n) = tr.train_layer(x, mask, w5, gamma, beta, kernel, stride, padding, subm)
    (y * weights).sum().backward()

    def dy_of(cs, c):
        return torch.stack([weights[b, :, z, yy, xx] for (b, z, yy, xx) in cs])

    bcells, by, bdw, bn = tr.brute_train_layer(cells, feats, batch, shape, w5.detach(), gamma.detach(), beta.detach(), kernel, stride, padding,
                                               subm, dy_of)
    idx, rows = sr.rows_of(y.detach(), m)
    assert [tuple(int(v) for v in r) for r in idx] == bcells and n == len(bcells) and 1 < n < m.numel()
    assert float((rows - by).abs().max()) <= 1e-12 * max(1.0, float(by.abs().max()))
    assert float((w5.grad - bdw).abs().max()) <= 1e-11 * max(1.0, float(bdw.abs().max())) and float(bdw.abs().max()) > 1e-3
    assert float((gamma.grad - bn.weight.grad).abs().max()) <= 1e-11 and float((beta.grad - bn.bias.grad).abs().max()) <= 1e-11
    rm, rv = tr.running_update(torch.zeros(cout), torch.ones(cout), mean.detach(), var.detach(), n)
    assert float((rm - bn.running_mean).abs().max()) <= 1e-13 and float((rv - bn.running_var).abs().max()) <= 1e-13
    assert int(bn.num_batches_tracked) == 1 and (by > 0).any() and (by == 0).any()
    # a forced mask equal to the run's own mask changes nothing; a dropped cell leaves the statistics
    y2 = tr.train_layer(x, mask, w5, gamma, beta, kernel, stride, padding, subm, forced=(pre > 0).double())[0]
    assert torch.equal(y2, y)
    drop = torch.zeros_like(m)
    b, z, yy, xx = bcells[-1]
    drop[b, 0, z, yy, xx] = True
    y3, m3, _, (_, _, n3) = tr.train_layer(x, mask, w5, gamma, beta, kernel, stride, padding, subm, drop=drop)
    assert n3 == n - 1 and int(m3.sum()) == n - 1 and float(y3.detach()[b, :, z, yy, xx].abs().max()) == 0.0


@pytest.mark.parametrize("kernel,stride,padding,subm", TYPES)
def test_single_launch_references_against_autograd_of_the_restatement(kernel, stride, padding, subm):
    rng = np.random.RandomState(5)
    batch, shape, cin, cout = 2, (7, 6, 9), 3, 5
    cells = np.stack(np.unravel_index(rng.permutation(batch * 7 * 6 * 9)[:50], (batch,) + shape), axis=1)
    feats = torch.from_numpy(rng.uniform(-1, 1, (50, cin)))
    w5 = torch.from_numpy(rng.uniform(-1, 1, (cout,) + kernel + (cin,)))
    idx, ref, s, k = tr.raw_reference(feats, cells, batch, shape, w5, kernel, stride, padding, subm)
    assert float(s.min()) >= 0 and bool((ref.abs() <= s + 1e-12).all()) and float(k.min()) >= cin
    dz = torch.from_numpy(rng.uniform(-1, 1, (len(idx), cout)))
    didx, dref, ds, dk = tr.dgrad_reference(dz, idx, cells, batch, shape, w5, kernel, stride, padding, subm)
    wref, ws, wk = tr.wgrad_reference(feats, cells, dz, idx, batch, shape, cin, kernel, stride, padding, subm)
    # the adjoint identities: <dz, conv(x)> = <dx, x> = <dW, W>
    xrows = sr.rows_of(*sr.to_dense(cells, feats, batch, shape))[1]
    lhs = float((dz * ref).sum())
    assert abs(lhs - float((dref * xrows).sum())) <= 1e-10 and abs(lhs - float((wref * w5).sum())) <= 1e-10 and abs(lhs) > 1e-3
    assert len(didx) == 50 and bool((dref.abs() <= ds + 1e-12).all()) and bool((wref.abs() <= ws + 1e-12).all())
    assert float(wk.sum()) * cin == float(k.sum()) and float(dk.sum()) * cin == float(k.sum()) * cout        # the same products, counted three ways


# ---------------------------------------------------------------------------------------------- tables, lowering, scratch
def test_pair_tables_lowering_and_scratch():
    assert ops.SPARSE_TRAIN_PAIRS == ((8, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128)) and ops.SPARSE_ROW_CHUNKS == 64
    layers = host.VoxelBackBone8x({}, 4, [21, 13, 40])._layers()
    assert [(ops.sparse_row_channels(c.in_channels, torch.float32), c.out_channels) for _, c, _ in layers] == \
        [(8, 16), (16, 16), (16, 32), (32, 32), (32, 32), (32, 64), (64, 64), (64, 64), (64, 64), (64, 64), (64, 64), (64, 128)]
    for cin_pad, cout in ops.SPARSE_TRAIN_PAIRS:
        for taps in (27, 3):
            floats, doubles = ops.sparse_train_scratch(cin_pad, cout, taps)
            assert floats == 64 * taps * ((cout + 31) // 32 * 32) * cin_pad and doubles == 64 * 2 * 128 == ops.SPARSE_STAT_DOUBLES
    assert ops.sparse_train_scratch(64, 64, 27)[0] * 4 == 28311552                   # the largest: 28 MB, whatever the grid
    for bad in ((16, 64, 27), (32, 16, 27), (12, 16, 27), (64, 64, 9)):
        with pytest.raises(CobevtHipError, match="cobevt_sparse_train_scratch failed"):
            ops.sparse_train_scratch(*bad)
    g = torch.Generator().manual_seed(0)
    w = torch.rand((16, 3, 3, 3, 4), generator=g)
    fwd, trn = ops.sparse_train_weights(w)
    assert tuple(fwd.shape) == (27, 32, 8) and tuple(trn.shape) == (27, 32, 16) and fwd.dtype == trn.dtype == torch.float32
    for kz, ky, kx in ((0, 0, 0), (1, 2, 0), (2, 2, 2)):
        t = (kz * 3 + ky) * 3 + kx
        assert torch.equal(fwd[t, :16, :4], w[:, kz, ky, kx, :]) and torch.equal(trn[t, :4, :], w[:, kz, ky, kx, :].t())
    assert float(fwd[:, 16:].abs().max()) == 0 and float(fwd[:, :, 4:].abs().max()) == 0 and float(trn[:, 4:].abs().max()) == 0
    # cached per weight object on its version counter: the same tensors until the weight changes in place; a detached alias is
    # another object and is lowered anew (callers hand over the Parameter itself); the entry goes with the weight
    assert ops.sparse_train_weights(w)[0] is fwd and ops.sparse_train_weights(w.detach())[0] is not fwd
    w.mul_(2.0)
    again = ops.sparse_train_weights(w)[0]
    assert again is not fwd and torch.equal(again[0, :16, :4], w[:, 0, 0, 0, :])
    w2 = torch.rand((128, 3, 1, 1, 64), generator=g)
    f2, t2 = ops.sparse_train_weights(w2)
    assert tuple(f2.shape) == (3, 128, 64) and tuple(t2.shape) == (3, 64, 128) and torch.equal(t2[2], w2[:, 2, 0, 0, :].t())
    for shape in ((16, 3, 3, 3, 9), (48, 3, 3, 3, 16), (16, 5, 3, 3, 16)):
        with pytest.raises(CobevtHipError, match="supported"):
            ops.sparse_train_weights(torch.zeros(shape))
    with pytest.raises(CobevtHipError, match="weight must be"):
        ops.sparse_train_weights(torch.zeros(16, 16, 3, 3))
    key = id(w2)
    assert key in ops._SPARSE_TRAIN_WEIGHTS
    del w2, f2, t2
    assert key not in ops._SPARSE_TRAIN_WEIGHTS


# ---------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_validates_arguments_before_any_launch():
    """null pointers (code 1); misaligned buffers, unsupported pairs / geometry, capacity 0 and a scratch that is too small (code 2):
    refused with host pointers, before anything touches a device"""
    l = lib.load()
    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    ptr, off, off8 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 8)
    longs = lambda *v: (ctypes.c_long * len(v))(*v)             # noqa: E731
    f = ctypes.c_float
    sub = (3, 3, 3, 1, 1, 1, 1, 1, 1)
    down = (3, 3, 3, 2, 2, 2, 1, 1, 1)
    bad_geo = ((3, 3, 1, 1, 1, 1, 1, 1, 1), (3, 3, 3, 4, 4, 4, 1, 1, 1), (3, 3, 3, 1, 1, 1, 3, 3, 3), (3, 1, 1, 2, 1, 1, 1, 1, 1))
    sizes = (ctypes.c_long * 2)()
    # scratch
    assert l.cobevt_sparse_train_scratch(None, sizes) == 1 and l.cobevt_sparse_train_scratch(longs(16, 16, 27), None) == 1
    for bad in ((16, 64, 27), (8, 32, 27), (0, 16, 27), (64, 64, 1)):
        assert l.cobevt_sparse_train_scratch(longs(*bad), sizes) == 2, bad
    # raw conv: dims = [N, D, H, W, input rows, output capacity, input row, Cout, kernel, stride, pad]
    good = (2, 41, 13, 21, 100, 100, 16, 16) + sub
    assert l.cobevt_sparse_conv_raw(ptr, ptr, ptr, None, ptr, ptr, ptr, ptr, None, None) == 1
    for hole in (0, 1, 2, 4, 5, 6, 7):
        args = [ptr] * 8
        args[3] = None
        args[hole] = None
        assert l.cobevt_sparse_conv_raw(*(args + [longs(*good), None])) == 1, hole
    for hole in (0, 1, 4, 6, 7):
        args = [ptr] * 8
        args[hole] = off
        assert l.cobevt_sparse_conv_raw(*(args + [longs(*good), None])) == 2, hole
    for bad in (good[:4] + (0,) + good[5:], good[:5] + (0,) + good[6:], good[:6] + (16, 64) + sub, good[:6] + (32, 16) + sub, good[:6] + (12, 16) + sub,
                good[:6] + (8, 32) + sub, (0,) + good[1:]) + tuple(good[:8] + g for g in bad_geo):
        assert l.cobevt_sparse_conv_raw(ptr, ptr, ptr, None, ptr, ptr, ptr, ptr, longs(*bad), None) == 2, bad
    # dgrad: dims = [N, D, H, W of the input, input capacity, output capacity, Cin, Cout, kernel, stride, pad]
    good = (2, 41, 13, 21, 100, 800, 16, 32) + down
    assert l.cobevt_sparse_conv_dgrad(ptr, ptr, ptr, ptr, ptr, ptr, ptr, None, None) == 1
    for hole in range(7):
        args = [ptr] * 7
        args[hole] = None
        assert l.cobevt_sparse_conv_dgrad(*(args + [longs(*good), None])) == 1, hole
    for hole in (0, 1, 3, 5, 6):
        args = [ptr] * 7
        args[hole] = off
        assert l.cobevt_sparse_conv_dgrad(*(args + [longs(*good), None])) == 2, hole
    for bad in (good[:4] + (0,) + good[5:], good[:5] + (0,) + good[6:], good[:6] + (8, 16) + down, good[:6] + (64, 32) + down,
                good[:6] + (16, 64) + down, (2, 2, 13, 21, 100, 800, 64, 64, 3, 3, 3, 2, 2, 2, 0, 0, 0)) + tuple(good[:8] + g for g in bad_geo):
        assert l.cobevt_sparse_conv_dgrad(ptr, ptr, ptr, ptr, ptr, ptr, ptr, longs(*bad), None) == 2, bad
    # BatchNorm forward: dims = [capacity, C, mode, doubles of partial]
    need = 64 * 2 * 128
    good = (100, 32, 0, need)
    bn = lambda args, dims: l.cobevt_sparse_bn_relu(*(args + [None if dims is None else longs(*dims), f(1e-3), f(0.01), None]))     # noqa: E731
    assert bn([ptr] * 10, None) == 1
    for hole in (0, 1, 2, 3, 7, 8):
        args = [ptr] * 10
        args[hole] = None
        assert bn(args, good) == 1, hole
    assert bn([ptr] * 4 + [None, None, None] + [ptr] * 3, (100, 32, 1, need)) == 1                       # frozen without running statistics
    for hole, o in ((0, off), (7, off), (9, off), (8, off), (6, off)):
        args = [ptr] * 10
        args[hole] = o
        assert bn(args, good) == 2, hole
    for bad in ((0, 32, 0, need), (100, 24, 0, need), (100, 256, 0, need), (100, 32, 2, need), (100, 32, 0, need - 1), (2 ** 31, 32, 0, need)):
        assert bn([ptr] * 10, bad) == 2, bad
    assert l.cobevt_sparse_bn_relu(*([ptr] * 10 + [longs(*good), f(0.0), f(0.01), None])) == 2
    assert l.cobevt_sparse_bn_relu(*([ptr] * 10 + [longs(*good), f(1e-3), f(1.5), None])) == 2
    # BatchNorm backward
    assert l.cobevt_sparse_bn_relu_bwd(*([ptr] * 11 + [None, None])) == 1
    for hole in range(11):
        args = [ptr] * 11
        args[hole] = None
        assert l.cobevt_sparse_bn_relu_bwd(*(args + [longs(*good), None])) == 1, hole
    for hole in (0, 1, 2, 5, 6, 9, 10):
        args = [ptr] * 11
        args[hole] = off
        assert l.cobevt_sparse_bn_relu_bwd(*(args + [longs(*good), None])) == 2, hole
    for bad in ((0, 32, 0, need), (100, 48, 0, need), (100, 32, 3, need), (100, 32, 0, 10)):
        assert l.cobevt_sparse_bn_relu_bwd(*([ptr] * 11 + [longs(*bad), None])) == 2, bad
    # wgrad: dims = [N, D, H, W, input rows, output capacity, Cin, input row, Cout, kernel, stride, pad, floats of partial]
    floats = 64 * 27 * 32 * 16
    good = (2, 41, 13, 21, 100, 100, 16, 16, 16) + sub + (floats,)
    assert l.cobevt_sparse_conv_wgrad(*([ptr] * 9 + [None, None])) == 1
    for hole in (0, 1, 2, 4, 5, 6, 7, 8):
        args = [ptr] * 9
        args[3] = None
        args[hole] = None
        assert l.cobevt_sparse_conv_wgrad(*(args + [longs(*good), None])) == 1, hole
    for hole in (0, 1, 4, 6, 7, 8):
        args = [ptr] * 9
        args[hole] = off
        assert l.cobevt_sparse_conv_wgrad(*(args + [longs(*good), None])) == 2, hole
    for bad in (good[:4] + (0,) + good[5:], good[:5] + (0,) + good[6:], good[:6] + (16, 16, 64) + good[9:], good[:6] + (12, 16, 16) + good[9:],
                good[:6] + (9, 8, 16) + good[9:], good[:6] + (0, 8, 16) + good[9:], good[:18] + (floats - 1,),
                good[:6] + (64, 64, 64) + sub + (floats,)) + tuple(good[:9] + g + (floats,) for g in bad_geo):
        assert l.cobevt_sparse_conv_wgrad(*([ptr] * 9 + [longs(*bad), None])) == 2, bad
    # dense backward: dims = [N, D, H, W, capacity, C]
    assert l.cobevt_sparse_dense_bwd(ptr, ptr, ptr, ptr, None, None) == 1
    for hole in range(4):
        args = [ptr] * 4
        args[hole] = None
        assert l.cobevt_sparse_dense_bwd(*(args + [longs(2, 2, 4, 6, 100, 128), None])) == 1
    for bad in ((2, 2, 4, 6, 0, 128), (2, 2, 4, 6, 100, 0), (0, 2, 4, 6, 100, 128), (2, 2, 4, 6, 2 ** 31, 128)):
        assert l.cobevt_sparse_dense_bwd(ptr, ptr, ptr, ptr, longs(*bad), None) == 2, bad
    assert l.cobevt_sparse_dense_bwd(ptr, off, ptr, ptr, longs(2, 2, 4, 6, 100, 128), None) == 2
    assert off8.value % 8 == 0


# ---------------------------------------------------------------------------------------------- refusals of the host layer
def _voxel_dict(p=10, t=5, c=4):
    return {"voxel_features": torch.zeros(p, t, c), "voxel_num_points": torch.ones(p, dtype=torch.int32),
            "voxel_coords": torch.zeros(p, 4, dtype=torch.int32), "batch_size": 1}


def test_cpu_tensors_are_refused_in_training():
    d = _voxel_dict()
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        training.mean_vfe(host.MeanVFE({}, 4), dict(d))
    m = host.VoxelBackBone8x({}, 4, [21, 13, 40])
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        training.voxel_backbone8x(m, dict(d, voxel_features=torch.zeros(10, 4)))
    x = ops.SparseConvTensor(torch.zeros(10, 128), torch.zeros(10, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), (2, 2, 3), 1,
                             torch.zeros(8, dtype=torch.int32))
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        training.height_compression(host.HeightCompression({"feature_num": 256}), {"encoded_spconv_tensor": x, "encoded_spconv_tensor_stride": 8})
    lvl = ops.SparseConvTensor(torch.zeros(10, 16), x.indices, x.num, (41, 13, 21), 1, x.workspace)
    w = torch.zeros(16, 3, 3, 3, 16)
    fwd, trn = ops.sparse_train_weights(w)
    for call in (lambda: ops.sparse_conv_raw(lvl, lvl, fwd, 16, 3, 1, 1, True),
                 lambda: ops.sparse_bn_relu(torch.zeros(10, 16), x.num, torch.ones(16), torch.zeros(16)),
                 lambda: ops.sparse_bn_relu_bwd(torch.zeros(10, 16), torch.zeros(10, 16), torch.zeros(10, 16), x.num, torch.ones(16), torch.zeros(4, 16)),
                 lambda: ops.sparse_conv_dgrad(torch.zeros(10, 16), lvl, lvl, trn, 16, 3, 1, 1, True),
                 lambda: ops.sparse_conv_wgrad(lvl, lvl, torch.zeros(10, 16), 16, 3, 1, 1, True),
                 lambda: ops.sparse_dense_bwd(torch.zeros(1, 2, 3, 256), x, 128)):
        with pytest.raises(CobevtHipError, match="no CPU fallback"):
            call()


def test_training_refusals(monkeypatch):
    """what the training graph does not offer raises before anything is launched (device guard off: tests/launch_trace.py)"""
    rec = lt.Recorder()
    lt.install(monkeypatch.setattr, rec)
    d = _voxel_dict()
    with pytest.raises(CobevtHipError, match="no gradient with respect to voxel_features"):
        training.mean_vfe(host.MeanVFE({}, 4), dict(d, voxel_features=torch.zeros(10, 5, 4, requires_grad=True)))
    m = host.VoxelBackBone8x({}, 4, [21, 13, 40])
    with pytest.raises(CobevtHipError, match="no gradient with respect to voxel_features"):
        training.voxel_backbone8x(m, dict(d, voxel_features=torch.zeros(10, 4, requires_grad=True)))
    with pytest.raises(CobevtHipError, match="voxel_features must be"):
        training.voxel_backbone8x(m, dict(d, voxel_features=torch.zeros(10, 5)))
    m.conv3[1][1].momentum = None
    with pytest.raises(CobevtHipError, match="momentum=None"):
        training.voxel_backbone8x(m, dict(d, voxel_features=torch.zeros(10, 4)))
    assert rec.records == []                                                         # nothing was launched
    m.conv3[1][1].momentum = 0.01
    m.conv3[1][1].eval()                                                             # a frozen BatchNorm1d inside a training module is fine
    out = training.height_compression(host.HeightCompression({"feature_num": 256}), training.voxel_backbone8x(m, dict(d, voxel_features=torch.zeros(10, 4))))
    sf = out["spatial_features"]
    assert tuple(sf.shape) == (1, 256, 2, 3) and sf.dtype == torch.float32 and sf.is_contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="shape|size"):
        sf.backward(torch.zeros(1, 256, 2, 4))                                       # torch itself refuses a wrong-shaped gradient
    x = out["encoded_spconv_tensor"]
    with pytest.raises(CobevtHipError, match="gradient must be contiguous fp32"):
        ops.sparse_dense_bwd(torch.zeros(1, 2, 3, 255), x, 128)
    with pytest.raises(CobevtHipError, match="dy must be contiguous fp32"):
        ops.sparse_bn_relu_bwd(torch.zeros(23, 128), x.features.detach(), x.features.detach(), x.num, torch.ones(128), torch.zeros(4, 128))
    lvl = ops.SparseConvTensor(torch.zeros(10, 16), torch.zeros(10, 4, dtype=torch.int32), x.num, (41, 13, 21), 1, x.workspace)
    with pytest.raises(CobevtHipError, match="dz must be contiguous fp32"):
        ops.sparse_conv_wgrad(lvl, lvl, torch.zeros(9, 16), 16, 3, 1, 1, True)
    with pytest.raises(CobevtHipError, match="dz must be contiguous fp32"):
        ops.sparse_conv_dgrad(torch.zeros(10, 32), lvl, lvl, torch.zeros(27, 32, 16), 16, 3, 1, 1, True)
    with pytest.raises(CobevtHipError, match="supported"):
        ops.sparse_conv_wgrad(lvl, lvl, torch.zeros(10, 64), 16, 3, 1, 1, True)
    with pytest.raises(CobevtHipError, match="supported"):
        ops.sparse_conv_raw(lvl, lvl, torch.zeros(27, 32, 16), 16, 3, 2, 1, True)
    with pytest.raises(CobevtHipError, match="frozen statistics need"):
        ops.sparse_bn_relu(torch.zeros(10, 16), x.num, torch.ones(16), torch.zeros(16), torch.nn.BatchNorm1d(16, track_running_stats=False), frozen=True)


# ---------------------------------------------------------------------------------------------- the launch trace
GRID, BATCH = (21, 13, 40), 2


def test_launch_trace_of_one_training_step(monkeypatch):
    rec = lt.Recorder()
    lt.install(monkeypatch.setattr, rec)
    coords = torch.from_numpy(sr.clustered_coords(GRID, BATCH, 1))
    p = coords.shape[0]
    data = {"voxel_features": torch.zeros(p, 5, 4), "voxel_num_points": torch.ones(p, dtype=torch.int32), "voxel_coords": coords, "batch_size": BATCH}
    m = host.VoxelBackBone8x({}, 4, list(GRID)).train()
    versions = [bn.running_mean._version for _, _, bn in m._layers()]
    ops._SPARSE_WS.clear()
    ops._SPARSE_TRAIN_WS.clear()
    try:
        with host.compute_dtype("bf16"):                                             # training is fp32 rows whatever the inference mode
            out = training.height_compression(host.HeightCompression({"feature_num": 256}),
                                              training.voxel_backbone8x(m, training.mean_vfe(host.MeanVFE({}, 4), data), keep_layers=True))
        n_fwd = len(rec.records)
        out["spatial_features"].sum().backward()
    finally:
        ops._SPARSE_WS.clear()
        ops._SPARSE_TRAIN_WS.clear()
    calls = [r[1] for r in rec.records]
    conv_bn = ["cobevt_sparse_conv_raw", "cobevt_sparse_bn_relu"]
    down = ["cobevt_sparse_scratch", "cobevt_sparse_downsample"]
    assert calls[:n_fwd] == ["cobevt_mean_vfe", "cobevt_sparse_scratch", "cobevt_sparse_index"] + conv_bn * 2 + (down + conv_bn * 3) * 3 + \
        down + conv_bn + ["cobevt_sparse_dense"]
    layer_bwd = ["cobevt_sparse_bn_relu_bwd", "cobevt_sparse_conv_dgrad", "cobevt_sparse_train_scratch", "cobevt_sparse_conv_wgrad"]
    first_bwd = [c for c in layer_bwd if c != "cobevt_sparse_conv_dgrad"]           # conv_input: a weight gradient, no input gradient
    assert calls[n_fwd:] == ["cobevt_sparse_dense_bwd"] + layer_bwd * 11 + first_bwd
    assert "cobevt_sparse_conv" not in calls                                         # no launch on folded weights in training
    assert {r[0] for r in rec.records} == {""}
    # the geometry and the pairs each backward launch is given, last layer first
    want = [(ops.sparse_row_channels(c.in_channels, torch.float32), c.out_channels, c.kernel_size + c.stride + c.padding) for _, c, _ in m._layers()]
    got_w = [(r[2][-1][7], r[2][-1][8], tuple(r[2][-1][9:18])) for r in rec.records if r[1] == "cobevt_sparse_conv_wgrad"]
    got_d = [(r[2][-1][6], r[2][-1][7], tuple(r[2][-1][8:17])) for r in rec.records if r[1] == "cobevt_sparse_conv_dgrad"]
    got_f = [(r[2][-1][6], r[2][-1][7], tuple(r[2][-1][8:17])) for r in rec.records if r[1] == "cobevt_sparse_conv_raw"]
    assert got_f == want and got_w == want[::-1] and got_d == want[:0:-1]
    assert [r[2][-3][2] for r in rec.records if r[1] == "cobevt_sparse_bn_relu"] == [0] * 12
    # outputs: fp32 rows with the graph, twelve kept layers, the running statistics' version counters bumped
    assert len(out["sparse_layer_outputs"]) == 12 and all(t.features.dtype == torch.float32 and t.features.requires_grad for t in out["sparse_layer_outputs"])
    assert out["sparse_layer_outputs"][-1] is out["encoded_spconv_tensor"] and out["multi_scale_3d_features"]["x_conv4"] is out["sparse_layer_outputs"][10]
    assert [bn.running_mean._version for _, _, bn in m._layers()] == [v + 1 for v in versions]
    for _, conv, bn in m._layers():
        assert tuple(conv.weight.grad.shape) == tuple(conv.weight.shape) and conv.weight.grad.dtype == torch.float32 and conv.weight.grad.is_contiguous()
        assert tuple(bn.weight.grad.shape) == tuple(bn.bias.grad.shape) == (conv.out_channels,)
    assert isinstance(ag.SparseConvBnReluFn, type) and isinstance(ag.SparseDenseFn, type)


def _layer_tables(out):
    """the transposed weight table each of the twelve layers saved for its backward (SparseConvBnReluFn saves x, z, y, stat, gamma, wt)"""
    return [t.features.grad_fn.saved_tensors[5] for t in out["sparse_layer_outputs"]]


def test_weight_tables_are_reused_until_a_weight_changes(monkeypatch):
    """through training.voxel_backbone8x: a second step with unchanged weights lowers nothing, under autocast too; after an in-place
    update of one weight (what an optimiser step is) that layer, and only that one, is lowered again"""
    rec = lt.Recorder()
    lt.install(monkeypatch.setattr, rec)
    coords = torch.from_numpy(sr.clustered_coords(GRID, BATCH, 1))
    p = coords.shape[0]
    data = {"voxel_features": torch.zeros(p, 4), "voxel_coords": coords, "batch_size": BATCH}
    m = host.VoxelBackBone8x({}, 4, list(GRID)).train()
    lowered = []
    real = ops.sparse_train_weights
    zeros = torch.zeros

    def counting_zeros(*a, **k):
        if len(a[0]) == 3:                     # the operand tables are the only 3-D zero fills of a step
            lowered.append(a[0])
        return zeros(*a, **k)

    ops._SPARSE_WS.clear()
    ops._SPARSE_TRAIN_WS.clear()
    try:
        first = _layer_tables(training.voxel_backbone8x(m, dict(data), keep_layers=True))
        monkeypatch.setattr(torch, "zeros", counting_zeros)
        second = _layer_tables(training.voxel_backbone8x(m, dict(data), keep_layers=True))
        with torch.autocast("cpu", dtype=torch.bfloat16):
            third = _layer_tables(training.voxel_backbone8x(m, dict(data), keep_layers=True))
        assert lowered == [] and all(a.data_ptr() == b.data_ptr() == c.data_ptr() for a, b, c in zip(first, second, third))
        with torch.no_grad():
            m.conv3[1][0].weight.mul_(0.5)
        fourth = _layer_tables(training.voxel_backbone8x(m, dict(data), keep_layers=True))
    finally:
        monkeypatch.setattr(torch, "zeros", zeros)
        ops._SPARSE_WS.clear()
        ops._SPARSE_TRAIN_WS.clear()
    names = [name for name, _, _ in m._layers()]
    assert [n for n, a, b in zip(names, first, fourth) if a.data_ptr() != b.data_ptr()] == ["conv3.1"] and len(lowered) == 2
    assert torch.equal(fourth[6][13, :64, :], m.conv3[1][0].weight.detach()[:, 1, 1, 1, :].t()) and real is ops.sparse_train_weights
