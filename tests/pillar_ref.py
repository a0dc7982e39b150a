"""Plain-torch restatement of the LiDAR pillar front end, in the folded form the HIP operator computes: point decoration ->
relu(f @ W + s) -> max over ALL T rows -> scatter at z + y * nx + x -> regroup.  Test-side only; pinned to the reference's outputs by
tests/golden/make_golden_pillar.py (to 1e-5) and replayed against the fixture by tests/test_point_pillar.py.

Reference: opv2v/opencood/models/sub_modules/pillar_vfe.py:31-53, 105-146; point_pillar_scatter.py:14-47; fuse_utils.py:8-61."""
import torch

CHANNELS = 64


def fold(sd, prefix, use_norm, eps=1e-3):
    """state_dict entries of one PFN layer -> (W (K, 64), s (64)): eval BatchNorm1d folded into the bias-free Linear (float64 fold)"""
    w = sd[prefix + "linear.weight"].double()                                  # (64, K)
    if use_norm:
        scale = sd[prefix + "norm.weight"].double() / torch.sqrt(sd[prefix + "norm.running_var"].double() + eps)
        shift = sd[prefix + "norm.bias"].double() - sd[prefix + "norm.running_mean"].double() * scale
        w = w * scale[:, None]
    else:
        shift = sd[prefix + "linear.bias"].double()
    return w.t().float().contiguous(), shift.float().contiguous()


def geom(voxel_size, lidar_range):
    """(voxel x, y, z, offset x, y, z) as PillarVFE.__init__ forms them (Python floats)"""
    return (voxel_size[0], voxel_size[1], voxel_size[2], voxel_size[0] / 2 + lidar_range[0], voxel_size[1] / 2 + lidar_range[1],
            voxel_size[2] / 2 + lidar_range[2])


def decorate(vf, npts, coords, g, use_absolute_xyz, with_distance):
    """(P, T, 4) points -> (P, T, K) decorated features, rows t >= n_p multiplied by 0"""
    xyz = vf[:, :, :3]
    mean = xyz.sum(dim=1, keepdim=True) / npts.to(vf.dtype).view(-1, 1, 1)        # over all T rows
    cf = coords.to(vf.dtype)
    centre = torch.stack([cf[:, 3] * g[0] + g[3], cf[:, 2] * g[1] + g[4], cf[:, 1] * g[2] + g[5]], dim=-1)
    feats = [vf if use_absolute_xyz else vf[..., 3:], xyz - mean, xyz - centre[:, None, :]]
    if with_distance:
        feats.append(torch.norm(xyz, 2, 2, keepdim=True))
    f = torch.cat(feats, dim=-1)
    on = torch.arange(vf.shape[1], device=vf.device)[None, :] < npts.view(-1, 1)
    return f * on[..., None].to(vf.dtype)


def pillar_features(vf, npts, coords, w, s, g, use_absolute_xyz=True, with_distance=False):
    """-> (P, 64): a masked row is all zeros and still contributes relu(s) to the maximum"""
    f = decorate(vf, npts, coords, g, use_absolute_xyz, with_distance)
    return torch.relu(f @ w + s).max(dim=1).values


def valid_rows(coords, n, ny, nx, npts=None):
    """the rows the operator writes: batch index in [0, n), y / x inside the grid, (with npts) n_p > 0"""
    c = coords.long()
    ok = (c[:, 0] >= 0) & (c[:, 0] < n) & (c[:, 2] >= 0) & (c[:, 2] < ny) & (c[:, 3] >= 0) & (c[:, 3] < nx)
    if npts is not None:
        ok = ok & (npts > 0)
    return ok


def scatter(rows, coords, n, ny, nx, npts=None):
    """(P, C) rows -> (n, ny, nx, C) channels-last, cell z + y * nx + x (y is the row); other cells 0; invalid rows skipped"""
    ok = valid_rows(coords, n, ny, nx, npts)
    c = coords.long()[ok]
    out = torch.zeros(n, ny * nx, rows.shape[1], dtype=rows.dtype, device=rows.device)
    out[c[:, 0], c[:, 1] + c[:, 2] * nx + c[:, 3]] = rows[ok]
    return out.view(n, ny, nx, rows.shape[1])


def regroup(x, record_len, max_cav):
    """(N, ...) -> ((B, max_cav, ...) zero-padded, mask (B, max_cav) fp32); agents past max_cav of a sample are dropped"""
    out = torch.zeros((len(record_len), max_cav) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    mask = torch.zeros(len(record_len), max_cav, device=x.device)
    off = 0
    for b, r in enumerate(int(v) for v in record_len):
        k = min(r, max_cav)
        out[b, :k] = x[off:off + k]
        mask[b, :r] = 1.0
        off += r
    return out, mask


def canvas(vf, npts, coords, w, s, g, ny, nx, record_len, max_cav, use_absolute_xyz=True, with_distance=False):
    """the fused operator: -> ((B, max_cav, ny, nx, 64), cav_mask (B, max_cav))"""
    n = int(sum(int(v) for v in record_len))
    ok = valid_rows(coords, n, ny, nx, npts)
    rows = pillar_features(vf[ok], npts[ok], coords[ok], w, s, g, use_absolute_xyz, with_distance)
    return regroup(scatter(rows, coords[ok], n, ny, nx), record_len, max_cav)


def fused_map(sd, args, vf, npts, coords, record_len):
    """PointPillarFuseBEVT on a state_dict: front end -> agent mask -> oracle.swap_fusion -> (B, 64, ny, nx)"""
    import oracle.swap_fusion as o_swap
    cfg = args["pillar_vfe"]
    w, s = fold(sd, "pillar_vfe.pfn_layers.0.", cfg["use_norm"])
    nx, ny, _ = args["point_pillar_scatter"]["grid_size"]
    x, mask = canvas(vf, npts, coords, w, s, geom(args["voxel_size"], args["lidar_range"]), ny, nx, record_len, args["max_cav"],
                     cfg["use_absolute_xyz"], cfg["with_distance"])
    com_mask = mask[:, None, None, None, :].expand(mask.shape[0], ny, nx, 1, mask.shape[1]).contiguous()
    fsd = {k[len("fusion_net."):]: v for k, v in sd.items() if k.startswith("fusion_net.")}
    return o_swap.swap_fusion_encoder(fsd, "", args["fax_fusion"], x.permute(0, 1, 4, 2, 3), com_mask)
