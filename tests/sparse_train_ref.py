"""Train-mode dense restatement of the sparse 3-D backbone in plain torch on the CPU - the yardstick of tests/test_sparse_train*.py,
built on tests/sparse_ref.py (levels as dense tensors that are zero off the active set, plus boolean masks).

A layer in train() mode: the raw convolution, BatchNorm1d with BATCH statistics over the active cells of the output mask (biased
variance, eps 1e-3), ReLU, the mask.  Everything is differentiable torch, so float64 autograd gives the reference gradients and float32
the fp32 deviation.  Two knobs the GPU tests need:
    forced   per layer a 0 / 1 tensor: y = pre . forced in place of relu(pre).  Between an fp32 and a float64 run the sign of a
             pre-activation near zero can differ; ONE such flip moves a parameter gradient by 1e-2 of its max-norm, against 3e-6
             without it, so a free comparison would test luck.  The float64 run is forced to the masks of the run under test, and the
             flips themselves are checked separately (a flipped element's float64 pre-activation must lie within the forward gate).
    drops    per layer a set of output cells removed from the active set: what a capacity smaller than the active set does.
brute_train_layer is the per-voxel, per-tap loop with torch.nn.BatchNorm1d in train() on the gathered rows and dW by the explicit double
sum, which the construction is pinned against (tests/test_sparse_train.py).

raw_reference / dgrad_reference / wgrad_reference: per-element float64 references of single launches from the operands as stored, each
with S = sum |a| |b| over the products present and K = their number, in the style of sparse_ref.kernel_reference."""
import torch
import torch.nn.functional as F

import sparse_ref as sr

EPS = sr.EPS
MOMENTUM = 0.01


def active_rows(t, mask):
    """(N, C, D, H, W) -> (R, C) over the mask's active cells in cell order"""
    idx = mask[:, 0].nonzero()
    return t[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]]


def train_layer(x, mask, w5, gamma, beta, kernel, stride, padding, subm, forced=None, drop=None, frozen=None):
    """conv + BatchNorm (batch statistics over the active output cells; frozen = (running_mean, running_var): those instead) + ReLU in
    x's dtype -> (y, mask_out, pre, (mean, biased var, n))"""
    m = sr.out_mask(mask, kernel, stride, padding, subm)
    if drop is not None:
        m = m & ~drop
    z = sr.conv(x, w5, stride, padding, subm)
    rows = active_rows(z, m)
    n = rows.shape[0]
    if frozen is not None:
        mean, var = frozen[0].to(x.dtype), frozen[1].to(x.dtype)
    else:
        mean = rows.mean(0)
        var = ((rows - mean) ** 2).mean(0)
    v = lambda t: t.to(x.dtype).view(1, -1, 1, 1, 1)         # noqa: E731
    pre = (z - v(mean)) / torch.sqrt(v(var) + EPS) * v(gamma) + v(beta)
    y = pre * forced.to(x.dtype) if forced is not None else torch.relu(pre)
    return y * m.to(x.dtype), m, pre, (mean, var, n)


def params_of(sd, dtype, requires_grad=True):
    """the 36 parameters of a VoxelBackBone8x state_dict as leaves in `dtype`: {key: tensor}"""
    out = {}
    for name, *_ in sr.LAYERS:
        wkey, bnp = sr.keys(name)
        for key in (wkey, bnp + "weight", bnp + "bias"):
            out[key] = sd[key].detach().to(dtype).clone().requires_grad_(requires_grad)
    return out


def backbone_train(params, coords, feats, batch, grid, dtype, forced=None, drops=None, frozen=None):
    """VoxelBackBone8x + HeightCompression in train() mode on the CPU.  forced / drops / frozen: {layer name: ...} as train_layer takes.
    -> (levels {name: (y, mask, pre)}, spatial_features (N, C D, H, W), stats {name: (mean, var, n)})"""
    x, mask = sr.to_dense(coords, feats, batch, sr.sparse_shape(grid), dtype)
    levels, stats = {}, {}
    for name, _, _, k, s, p, subm in sr.LAYERS:
        wkey, bnp = sr.keys(name)
        x, mask, pre, st = train_layer(x, mask, params[wkey], params[bnp + "weight"], params[bnp + "bias"], k, s, p, subm,
                                       None if forced is None else forced[name], None if drops is None else drops.get(name),
                                       None if frozen is None else frozen.get(name))
        levels[name], stats[name] = (x, mask, pre), st
    n, c, d, h, w = x.shape
    return levels, x.reshape(n, c * d, h, w), stats


def running_update(running_mean, running_var, mean, var, n, momentum=MOMENTUM):
    """nn.BatchNorm1d's update in float64: the variance with n / (n - 1); n <= 1 updates nothing"""
    if n <= 1:
        return running_mean.double(), running_var.double()
    return ((1 - momentum) * running_mean.double() + momentum * mean.double(),
            (1 - momentum) * running_var.double() + momentum * var.double() * n / (n - 1))


def masks_of(levels):
    """the ReLU masks of a run as forced-mask tensors: {name: (pre > 0) as 0 / 1}"""
    return {name: (pre > 0).to(torch.float64) for name, (_, _, pre) in levels.items()}


# ---------------------------------------------------------------------------------------------- brute force
def brute_train_layer(coords, feats, batch, shape, w5, gamma, beta, kernel, stride, padding, subm, dy_of):
    """The same layer as a per-voxel, per-tap loop in float64 over unique coords, torch.nn.BatchNorm1d in train() on the gathered rows.
    dy_of(cells, C) -> the (R, C) gradient of the loss with respect to the layer's output rows.
    -> (cells sorted, y rows (R, C), dW by the explicit double sum (Cout, kz, ky, kx, Cin), the BatchNorm1d after the step)"""
    table = {tuple(int(v) for v in c): torch.as_tensor(f).double() for c, f in zip(coords, feats)}
    so = tuple(shape) if subm else sr.out_shape(shape, kernel, stride, padding)
    pad, st = ((1, 1, 1), (1, 1, 1)) if subm else (padding, stride)
    outs = set()
    for (b, z, y, x) in table:
        if subm:
            outs.add((b, z, y, x))
            continue
        for kz in range(kernel[0]):
            for ky in range(kernel[1]):
                for kx in range(kernel[2]):
                    n = (z + pad[0] - kz, y + pad[1] - ky, x + pad[2] - kx)
                    if all(v >= 0 and v % s == 0 and v // s < lim for v, s, lim in zip(n, st, so)):
                        outs.add((b,) + tuple(v // s for v, s in zip(n, st)))
    cells = sorted(outs)
    w5 = w5.double()
    cout, cin = w5.shape[0], w5.shape[4]
    zrows, nbrs = [], []
    for (b, oz, oy, ox) in cells:
        acc = torch.zeros(cout, dtype=torch.float64)
        here = []
        for kz in range(kernel[0]):
            for ky in range(kernel[1]):
                for kx in range(kernel[2]):
                    src = (b, oz * st[0] - pad[0] + kz, oy * st[1] - pad[1] + ky, ox * st[2] - pad[2] + kx)
                    if src in table:
                        acc += w5[:, kz, ky, kx, :] @ table[src]
                        here.append(((kz, ky, kx), src))
        zrows.append(acc)
        nbrs.append(here)
    z = torch.stack(zrows).requires_grad_(True)
    bn = torch.nn.BatchNorm1d(cout, eps=EPS, momentum=MOMENTUM).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma.double())
        bn.bias.copy_(beta.double())
    y = torch.relu(bn(z))
    (y * dy_of(cells, cout)).sum().backward()
    dz = z.grad
    dw = torch.zeros_like(w5)
    for o, here in enumerate(nbrs):
        for (kz, ky, kx), src in here:
            dw[:, kz, ky, kx, :] += dz[o][:, None] * table[src][None, :]
    return cells, y.detach(), dw, bn


# ---------------------------------------------------------------------------------------------- single launches, in float64
def _ones_w(kernel):
    return torch.ones((1,) + tuple(kernel) + (1,), dtype=torch.float64)


def raw_reference(x_rows, coords, batch, shape, w5, kernel, stride, padding, subm):
    """z = conv(x) per output row.  x_rows (P, Cin) / w5 (Cout, kz, ky, kx, Cin): the operands as stored.
    -> (indices (R, 4), ref (R, Cout), S (R, Cout) = sum |x| |w| over the taps present, K (R, 1) = number of products)"""
    cin = w5.shape[4]
    x, mask = sr.to_dense(coords, torch.as_tensor(x_rows)[:, :cin].double(), batch, shape)
    w5 = w5.double()
    m = sr.out_mask(mask, kernel, stride, padding, subm)
    md = m.double()
    ref = sr.conv(x, w5, stride, padding, subm) * md
    s = sr.conv(x.abs(), w5.abs(), stride, padding, subm) * md
    k = sr.conv(mask.double(), _ones_w(kernel), stride, padding, subm) * cin
    idx, ref_rows = sr.rows_of(ref, m)
    return idx, ref_rows, sr.rows_of(s, m)[1], sr.rows_of(k, m)[1]


def _dense_of_rows(idx, rows, batch, shape):
    t = torch.zeros((batch, rows.shape[1]) + tuple(shape), dtype=torch.float64)
    i = idx.long()
    t[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]] = rows.double()
    return t


def dgrad_reference(dz_rows, out_idx, coords, batch, shape, w5, kernel, stride, padding, subm):
    """dx per INPUT row (cell order of the input level) from dz_rows (R, Cout) by the output level's rows out_idx.
    -> (input indices (Q, 4), ref (Q, Cin), S, K (Q, 1))"""
    cin, cout = w5.shape[4], w5.shape[0]
    _, mask = sr.to_dense(coords, torch.zeros(len(coords), 1), batch, shape)
    so = tuple(shape) if subm else sr.out_shape(shape, kernel, stride, padding)
    dz = _dense_of_rows(out_idx, dz_rows, batch, so)
    live = _dense_of_rows(out_idx, torch.ones(len(out_idx), 1), batch, so)

    def pull(w, g, c):
        x = torch.zeros((batch, c) + tuple(shape), dtype=torch.float64, requires_grad=True)
        sr.conv(x, w, stride, padding, subm).backward(g)
        return x.grad * mask.double()

    w5 = w5.double()
    ref, s = pull(w5, dz, cin), pull(w5.abs(), dz.abs(), cin)
    k = pull(_ones_w(kernel), live, 1) * cout
    idx, ref_rows = sr.rows_of(ref, mask)
    return idx, ref_rows, sr.rows_of(s, mask)[1], sr.rows_of(k, mask)[1]


def wgrad_reference(x_rows, coords, dz_rows, out_idx, batch, shape, cin, kernel, stride, padding, subm):
    """dW (Cout, kz, ky, kx, Cin) from the stored x rows and dz rows -> (ref, S, K (1, kz, ky, kx, 1) = (row, neighbour) pairs per tap)"""
    x, mask = sr.to_dense(coords, torch.as_tensor(x_rows)[:, :cin].double(), batch, shape)
    so = tuple(shape) if subm else sr.out_shape(shape, kernel, stride, padding)
    dz = _dense_of_rows(out_idx, dz_rows, batch, so)
    live = _dense_of_rows(out_idx, torch.ones(len(out_idx), 1), batch, so)
    cout = dz_rows.shape[1]

    def pull(xx, g, co, ci):
        w = torch.zeros((co,) + tuple(kernel) + (ci,), dtype=torch.float64, requires_grad=True)
        sr.conv(xx, w, stride, padding, subm).backward(g)
        return w.grad

    return pull(x, dz, cout, cin), pull(x.abs(), dz.abs(), cout, cin), pull(mask.double(), live, 1, 1)


def bn_reference(z_rows, gamma, beta, eps=EPS):
    """float64 statistics of z (n, C) as stored -> (mean, biased var, rstd, scale, shift)"""
    z = z_rows.double()
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.double() * rstd
    return mean, var, rstd, scale, beta.double() - mean * scale
