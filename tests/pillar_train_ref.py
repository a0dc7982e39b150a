"""Plain-torch restatement of the LiDAR pillar front end in train() mode: point decoration (pillar_ref.decorate) -> Linear ->
F.batch_norm(training=True) over all P * T rows (masked all-zero rows included) -> ReLU -> max over T -> scatter -> regroup.
Differentiable in the parameters; runs in the dtype of its inputs (fp32 or fp64).  Test-side only; pinned to the reference's module in
train() by tests/golden/make_golden_pillar_train.py (to 1e-5) and replayed against the fixture by tests/test_point_pillar_train.py.

Reference: opv2v/opencood/models/sub_modules/pillar_vfe.py:31-53 (PFNLayer.forward), :105-146; point_pillar_scatter.py:14-47."""
import torch

import pillar_ref as pr

F = torch.nn.functional
EPS, MOMENTUM = 1e-3, 0.01


def params(sd, prefix, use_norm, dtype=torch.float32, device=None):
    """leaf copies of one PFN layer's parameters (requires_grad) and clones of its buffers, keyed by the state_dict's suffixes"""
    keys = ["linear.weight"] + (["norm.weight", "norm.bias"] if use_norm else ["linear.bias"])
    p = {k: sd[prefix + k].detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for k in keys}
    if use_norm:
        p["norm.running_mean"] = sd[prefix + "norm.running_mean"].detach().to(device=device, dtype=dtype).clone()
        p["norm.running_var"] = sd[prefix + "norm.running_var"].detach().to(device=device, dtype=dtype).clone()
        p["norm.num_batches_tracked"] = sd[prefix + "norm.num_batches_tracked"].detach().to(device=device).clone()
    return p


def pillar_features(p, vf, npts, coords, g, use_absolute_xyz=True, with_distance=False, use_norm=True, training=True):
    """-> (P, 64).  training: batch statistics over the P * T rows, and the running statistics in `p` are updated in place as
    nn.BatchNorm1d does (momentum 0.01, unbiased variance, num_batches_tracked + 1); else the running statistics are used"""
    f = pr.decorate(vf.to(p["linear.weight"].dtype), npts, coords, g, use_absolute_xyz, with_distance)        # (P, T, K)
    rows, t, k = f.shape
    z = f.reshape(rows * t, k) @ p["linear.weight"].t()
    if use_norm:
        z = F.batch_norm(z, p["norm.running_mean"], p["norm.running_var"], p["norm.weight"], p["norm.bias"], training, MOMENTUM, EPS)
        if training:
            p["norm.num_batches_tracked"] += 1
    else:
        z = z + p["linear.bias"]
    return torch.relu(z).reshape(rows, t, pr.CHANNELS).max(dim=1).values


def valid_rows(coords, npts, record_len, max_cav, ny, nx):
    """the pillars the fused operator writes: agent inside record_len's agents and in a regrouped slot < max_cav, y / x inside the
    grid, n_p > 0"""
    n = int(sum(int(v) for v in record_len))
    ok = pr.valid_rows(coords, n, ny, nx, npts)
    slot_ok = torch.zeros(max(n, 1), dtype=torch.bool, device=coords.device)
    off = 0
    for r in (int(v) for v in record_len):
        slot_ok[off:off + min(r, max_cav)] = True
        off += r
    return ok & slot_ok[coords[:, 0].long().clamp(0, max(n, 1) - 1)]


def canvas(p, vf, npts, coords, g, ny, nx, record_len, max_cav, use_absolute_xyz=True, with_distance=False, use_norm=True, training=True):
    """the fused front end: -> ((B, max_cav, ny, nx, 64), cav_mask (B, max_cav)); statistics over the valid pillars only"""
    n = int(sum(int(v) for v in record_len))
    ok = valid_rows(coords, npts, record_len, max_cav, ny, nx)
    rows = pillar_features(p, vf[ok], npts[ok], coords[ok], g, use_absolute_xyz, with_distance, use_norm, training)
    return pr.regroup(pr.scatter(rows, coords[ok], n, ny, nx), record_len, max_cav)
