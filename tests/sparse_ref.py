"""Dense restatement of the sparse 3-D backbone in plain torch on the CPU - the yardstick of tests/test_sparse_backbone*.py.  spconv is
not installed, so nothing here comes from the reference's own modules; what is assumed about spconv (weight layout
(Cout, kz, ky, kx, Cin), cross-correlation, SubMConv3d's output set = input set, SparseConv3d's output set = every cell with an active
input in its receptive field) is read from its documentation and listed in DESIGN.md.

A level is a dense tensor x (N, C, D, H, W) that is zero off the active set, plus a boolean mask (N, 1, D, H, W):
    SubM     conv3d(x, w, padding=1) . mask_in
    strided  conv3d(x, w, stride, padding), masked by conv3d(mask, ones, stride, padding) > 0
with w = weight.permute(0, 4, 1, 2, 3); then the BatchNorm affine, ReLU, and the mask again (an active cell whose convolution is
zero still carries relu(shift)).  brute_layer is the per-voxel, per-tap loop the construction is pinned against."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3
# (name, Cin (None: the input's), Cout, kernel, stride, padding, subm) in forward order: VoxelBackBone8x
LAYERS = (("conv_input", None, 16, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),
          ("conv1.0", 16, 16, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),
          ("conv2.0", 16, 32, (3, 3, 3), (2, 2, 2), (1, 1, 1), False),
          ("conv2.1", 32, 32, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),
          ("conv2.2", 32, 32, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),
          ("conv3.0", 32, 64, (3, 3, 3), (2, 2, 2), (1, 1, 1), False),
          ("conv3.1", 64, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),
          ("conv3.2", 64, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),
          ("conv4.0", 64, 64, (3, 3, 3), (2, 2, 2), (0, 1, 1), False),
          ("conv4.1", 64, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),
          ("conv4.2", 64, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),
          ("conv_out", 64, 128, (3, 1, 1), (2, 1, 1), (0, 0, 0), False))
GRIDS = ((48, 32, 40), (45, 31, 24), (21, 13, 40))          # (nx, ny, nz)


def keys(name):
    """(conv weight key, BatchNorm key prefix) of a layer in the module's state_dict"""
    return name + ".0.weight", name + ".1."


def sparse_shape(grid):
    nx, ny, nz = grid
    return (nz + 1, ny, nx)


def out_shape(shape, kernel, stride, padding):
    return tuple((n + 2 * p - k) // s + 1 for n, k, s, p in zip(shape, kernel, stride, padding))


def shape_chain(grid):
    """the sparse shapes of the input level, conv2, conv3, conv4, conv_out"""
    shapes = [sparse_shape(grid)]
    for _, _, _, k, s, p, subm in LAYERS:
        if not subm:
            shapes.append(out_shape(shapes[-1], k, s, p))
    return shapes


# ---------------------------------------------------------------------------------------------- cases
def clustered_coords(grid, batch=2, seed=0, points=170, sigma=(2.0, 2.5, 2.5)):
    """voxel_coords (P, 4) int32 [b, z, y, x], unique, in a seeded random order: two Gaussian clusters of voxels per sample, sigma
    about (2, 2.5, 2.5) cells.  Uniformly scattered voxels would saturate the coarse levels and hide active-set mistakes there."""
    rng = np.random.RandomState(seed)
    d, h, w = sparse_shape(grid)
    rows = []
    for b in range(batch):
        for _ in range(2):
            centre = np.array([rng.uniform(3, d - 4), rng.uniform(3, h - 4), rng.uniform(3, w - 4)])
            pts = np.round(centre + rng.randn(points, 3) * np.asarray(sigma)).astype(np.int64)
            ok = ((pts >= 0) & (pts < np.array([d, h, w]))).all(axis=1)
            rows.append(np.concatenate([np.full((int(ok.sum()), 1), b), pts[ok]], axis=1))
    coords = np.unique(np.concatenate(rows), axis=0)
    return coords[rng.permutation(len(coords))].astype(np.int32)


def features_for(coords, channels, seed=0):
    rng = np.random.RandomState(seed + 1000)
    return rng.uniform(-1.0, 1.0, size=(len(coords), channels)).astype(np.float32)


def to_dense(coords, feats, batch, shape, dtype=torch.float64):
    """rows -> (x (N, C, D, H, W), mask (N, 1, D, H, W) bool); rows with b < 0 or a coordinate outside the shape are ignored, of
    duplicate cells the lowest row wins"""
    coords = np.asarray(coords).astype(np.int64)
    feats = torch.as_tensor(feats).to(dtype)
    x = torch.zeros((batch, feats.shape[1]) + tuple(shape), dtype=dtype)
    mask = torch.zeros((batch, 1) + tuple(shape), dtype=torch.bool)
    ok = (coords[:, 0] >= 0) & (coords[:, 0] < batch)
    for j in range(3):
        ok &= (coords[:, 1 + j] >= 0) & (coords[:, 1 + j] < shape[j])
    for i in np.nonzero(ok)[0][::-1]:                       # descending: the lowest row is written last
        b, z, y, xx = coords[i]
        x[b, :, z, y, xx] = feats[i]
        mask[b, 0, z, y, xx] = True
    return x, mask


def rows_of(x, mask):
    """(indices (R, 4) int32 [b, z, y, x] in cell order, features (R, C)) of a dense level"""
    idx = mask[:, 0].nonzero()                              # lexicographic in (b, z, y, x): the cell order
    return idx.to(torch.int32), x[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]]


# ---------------------------------------------------------------------------------------------- one layer
def out_mask(mask, kernel, stride, padding, subm):
    if subm:
        return mask
    ones = torch.ones((1, 1) + tuple(kernel), dtype=torch.float32)
    return F.conv3d(mask.float(), ones, stride=stride, padding=padding) > 0


def conv(x, w5, stride, padding, subm):
    """the raw convolution of a level: w5 (Cout, kz, ky, kx, Cin), the spconv 2.x layout"""
    w = w5.permute(0, 4, 1, 2, 3).to(x.dtype)
    return F.conv3d(x, w, padding=1) if subm else F.conv3d(x, w, stride=stride, padding=padding)


def layer(x, mask, w5, scale, shift, kernel, stride, padding, subm):
    """conv + BatchNorm affine + ReLU of one layer in x's dtype -> (y, mask_out)"""
    m = out_mask(mask, kernel, stride, padding, subm)
    y = conv(x, w5, stride, padding, subm)
    y = y * scale.to(x.dtype).view(1, -1, 1, 1, 1) + shift.to(x.dtype).view(1, -1, 1, 1, 1)
    return torch.relu(y) * m.to(x.dtype), m


def brute_layer(coords, feats, batch, shape, w5, scale, shift, kernel, stride, padding, subm):
    """the same layer as a per-voxel, per-tap loop in float64 over unique coords -> {(b, z, y, x): output vector}"""
    table = {tuple(int(v) for v in c): torch.as_tensor(f).double() for c, f in zip(coords, feats)}
    so = tuple(shape) if subm else out_shape(shape, kernel, stride, padding)
    outs = set()
    for (b, z, y, x) in table:
        if subm:
            outs.add((b, z, y, x))
            continue
        for kz in range(kernel[0]):
            for ky in range(kernel[1]):
                for kx in range(kernel[2]):
                    n = (z + padding[0] - kz, y + padding[1] - ky, x + padding[2] - kx)
                    if all(v >= 0 and v % s == 0 and v // s < lim for v, s, lim in zip(n, stride, so)):
                        outs.add((b,) + tuple(v // s for v, s in zip(n, stride)))
    result = {}
    w5 = w5.double()
    pad = (1, 1, 1) if subm else padding
    st = (1, 1, 1) if subm else stride
    for (b, oz, oy, ox) in sorted(outs):
        acc = torch.zeros(w5.shape[0], dtype=torch.float64)
        for kz in range(kernel[0]):
            for ky in range(kernel[1]):
                for kx in range(kernel[2]):
                    src = (b, oz * st[0] - pad[0] + kz, oy * st[1] - pad[1] + ky, ox * st[2] - pad[2] + kx)
                    if src in table:
                        acc += w5[:, kz, ky, kx, :] @ table[src]
        result[(b, oz, oy, ox)] = torch.relu(acc * scale.double() + shift.double())
    return result


# ---------------------------------------------------------------------------------------------- the backbone
def bn_affine(sd, prefix):
    s = sd[prefix + "weight"].double() / torch.sqrt(sd[prefix + "running_var"].double() + EPS)
    return s, sd[prefix + "bias"].double() - sd[prefix + "running_mean"].double() * s


def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def backbone(sd, coords, feats, batch, grid, mode="f64"):
    """VoxelBackBone8x + HeightCompression on the CPU.  mode "f64" / "f32": every layer in that precision, as written above.
    "bf16": the input features, the weights with the BatchNorm scale folded in (in float64, then rounded) and every layer's output
    rounded to bf16, products and sums in fp32 - the arithmetic of bf16 storage.
    -> (levels: {layer name: (x, mask)}, spatial_features (N, C D, H, W))"""
    dt = torch.float64 if mode == "f64" else torch.float32
    x, mask = to_dense(coords, feats, batch, sparse_shape(grid), dt)
    if mode == "bf16":
        x = _bf16(x)
    levels = {}
    for name, _, _, k, s, p, subm in LAYERS:
        wkey, bnp = keys(name)
        scale, shift = bn_affine(sd, bnp)
        if mode == "bf16":
            w5 = _bf16((sd[wkey].double() * scale.view(-1, 1, 1, 1, 1)).float())
            m = out_mask(mask, k, s, p, subm)
            y = conv(x, w5, s, p, subm) + shift.float().view(1, -1, 1, 1, 1)
            x, mask = _bf16(torch.relu(y)) * m.float(), m
        else:
            x, mask = layer(x, mask, sd[wkey], scale, shift, k, s, p, subm)
        levels[name] = (x, mask)
    n, c, d, h, w = x.shape
    return levels, x.reshape(n, c * d, h, w)


def assert_case_is_sparse_everywhere(levels):
    """every one of the twelve layers has both active and inactive cells"""
    for name, (_, mask) in levels.items():
        active, cells = int(mask.sum()), mask.numel()
        assert 0 < active < cells, "%s: %d of %d cells active" % (name, active, cells)


def module_gates(sd, coords, feats, batch, grid):
    """(reference (f64 spatial_features), d32, d16): the max-norm deviation of the fp32 restatement, and of the bf16-storage one,
    from the float64 one, relative to max|out|.  The GPU tests gate at 4 x these."""
    levels, ref = backbone(sd, coords, feats, batch, grid, "f64")
    assert_case_is_sparse_everywhere(levels)
    scale = float(ref.abs().max())
    d32 = float((backbone(sd, coords, feats, batch, grid, "f32")[1].double() - ref).abs().max()) / scale
    d16 = float((backbone(sd, coords, feats, batch, grid, "bf16")[1].double() - ref).abs().max()) / scale
    return levels, ref, d32, d16


SEEDS = {(48, 32, 40): 0, (45, 31, 24): 0, (21, 13, 40): 1}          # per grid: a seed whose clusters leave every level partly active
SLOTS = 5


def module_case(grid, batch=2, pad_rows=0):
    """the voxel dict of a grid's case as the reference's collate gives it - voxel_features (P, T, 4) fp32 with 1 .. T points per voxel
    and zeros in the unused slots, voxel_num_points, voxel_coords - and the float64 mean per voxel.  pad_rows: that many padding rows
    (batch index -1) appended, the fixed-size dict of a captured graph."""
    coords = clustered_coords(grid, batch, SEEDS[grid])
    rng = np.random.RandomState(SEEDS[grid] + 77)
    p = len(coords)
    npts = rng.randint(1, SLOTS + 1, size=p).astype(np.int32)
    vf = rng.uniform(-1.0, 1.0, size=(p, SLOTS, 4)).astype(np.float32)
    vf[np.arange(SLOTS)[None, :] >= npts[:, None]] = 0.0
    mean = vf.astype(np.float64).sum(axis=1) / npts[:, None]
    if pad_rows:
        coords = np.concatenate([coords, np.tile(np.array([[-1, 0, 0, 0]], dtype=np.int32), (pad_rows, 1))])
        npts = np.concatenate([npts, np.zeros(pad_rows, dtype=np.int32)])
        vf = np.concatenate([vf, rng.uniform(-1.0, 1.0, size=(pad_rows, SLOTS, 4)).astype(np.float32)])      # garbage: never read
    return {"voxel_features": torch.from_numpy(vf), "voxel_num_points": torch.from_numpy(npts), "voxel_coords": torch.from_numpy(coords)}, mean


# ---------------------------------------------------------------------------------------------- kernel cases
KERNEL_SHAPE, KERNEL_BATCH = (9, 10, 40), 2
TILE = 32
_SUB, _K3 = ((1, 1, 1), (1, 1, 1)), (3, 3, 3)


def _line(n, b=0, z=4, y=5, x0=2):
    return [[b, z, y, x0 + i] for i in range(n)]


def _cluster(seed, points=90):
    nx, ny, nz = KERNEL_SHAPE[2], KERNEL_SHAPE[1], KERNEL_SHAPE[0] - 1
    return clustered_coords((nx, ny, nz), KERNEL_BATCH, seed, points, (1.2, 1.5, 2.5)).tolist()


# name -> (Cin, Cout, kernel, stride, padding, subm, coordinates [b, z, y, x])
KERNEL_CASES = {
    "subm_4_16": (4, 16, _K3, *_SUB, True, _cluster(1)),
    "subm_16_16": (16, 16, _K3, *_SUB, True, _cluster(2)),
    "subm_64_64": (64, 64, _K3, *_SUB, True, _cluster(3)),
    "down_16_32_pad1": (16, 32, _K3, (2, 2, 2), (1, 1, 1), False, _cluster(4)),
    "down_64_64_pad011": (64, 64, _K3, (2, 2, 2), (0, 1, 1), False, _cluster(5)),
    "down_64_128_k311": (64, 128, (3, 1, 1), (2, 1, 1), (0, 0, 0), False, _cluster(6)),
    # tile edges: one row, tile - 1, tile + 1 rows; a line along x, so that every tap off the line is absent for all rows of a tile
    "rows_1": (16, 16, _K3, *_SUB, True, _line(1)),
    "rows_tile_minus_1": (16, 16, _K3, *_SUB, True, _line(TILE - 1)),
    "rows_tile_plus_1": (32, 32, _K3, *_SUB, True, _line(TILE + 1)),
    "rows_block_plus_1": (16, 16, _K3, *_SUB, True, _line(36, z=3) + _line(36, z=4) + _line(36, z=5) + _line(21, z=6)),      # 4 x 32 + 1
    # one tile whose rows belong to two samples
    "two_samples_one_tile": (32, 64, _K3, *_SUB, True, _line(12, b=0, y=9, x0=27) + _line(12, b=1, y=0, x0=0)),
}


def kernel_case(name):
    """-> dict: coords (P, 4) int32 in a seeded random order, feats (P, Cin) fp32, weight (Cout, kz, ky, kx, Cin) fp32, bn (the
    BatchNorm1d state as fp32 tensors) and the layer's geometry"""
    cin, cout, kernel, stride, padding, subm, cells = KERNEL_CASES[name]
    g = torch.Generator().manual_seed(sum(ord(c) for c in name))
    coords = torch.tensor(cells, dtype=torch.int32)
    coords = coords[torch.randperm(len(cells), generator=g)]
    taps = kernel[0] * kernel[1] * kernel[2]
    weight = (torch.rand((cout,) + tuple(kernel) + (cin,), generator=g) - 0.5) * 2.0 * (12.0 / (cin * taps)) ** 0.5
    bn = {"weight": 0.8 + 0.4 * torch.rand(cout, generator=g), "bias": (torch.rand(cout, generator=g) - 0.5) * 0.6,
          "running_mean": (torch.rand(cout, generator=g) - 0.5) * 0.4, "running_var": 0.6 + 0.8 * torch.rand(cout, generator=g)}
    feats = (torch.rand(len(cells), cin, generator=g) - 0.5) * 2.0
    return {"coords": coords, "feats": feats, "weight": weight, "bn": bn, "cin": cin, "cout": cout, "kernel": kernel, "stride": stride,
            "padding": padding, "subm": subm}


def bn_module(bn):
    m = torch.nn.BatchNorm1d(bn["weight"].numel(), eps=EPS)
    m.load_state_dict({**bn, "num_batches_tracked": torch.tensor(0)})
    return m.eval()


# ---------------------------------------------------------------------------------------------- one kernel launch, in float64
def kernel_reference(x_rows, coords, batch, shape, wgt, shift, cin, cout, kernel, stride, padding, subm):
    """The float64 reference of ONE cobevt_sparse_conv launch and its per-element gate.  x_rows (P, >= cin): the operands as stored
    (already rounded to the storage dtype), wgt [taps][Cout padded][Cin padded] / shift: the plan's tensors.
    -> (indices (R, 4), ref (R, cout), S (R, cout) = sum |x| |w'| over the taps present, K (R, 1) = number of products)"""
    x, mask = to_dense(coords, torch.as_tensor(x_rows)[:, :cin].double(), batch, shape)
    w5 = wgt.double()[:, :cout, :cin].reshape(tuple(kernel) + (cout, cin)).permute(3, 0, 1, 2, 4)
    m = out_mask(mask, kernel, stride, padding, subm)
    y = conv(x, w5, stride, padding, subm) + shift.double()[:cout].view(1, -1, 1, 1, 1)
    ref = torch.relu(y) * m.double()
    s = conv(x.abs(), w5.abs(), stride, padding, subm)
    k = conv(mask.double(), torch.ones((1,) + tuple(kernel) + (1,), dtype=torch.float64), stride, padding, subm) * cin
    idx, ref_rows = rows_of(ref, m)
    return idx, ref_rows, rows_of(s, m)[1], rows_of(k, m)[1]
