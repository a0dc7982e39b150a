"""Generate gv21_point_pillar.npz by running the REFERENCE's LiDAR pillar front end (sub_modules/pillar_vfe.py PillarVFE,
point_pillar_scatter.py PointPillarScatter, fuse_utils.regroup) and its composition with SwapFusionEncoder, in the build container
like make_golden.py:

    python tests/golden/make_golden_pillar.py

Procedural voxels and weights (cases_pillar.py); stored are reference OUTPUTS only: `pillar_features` for the four
(use_absolute_xyz, with_distance) combinations with use_norm, one combination without, one with non-zero rows past n_p (pins "the
mean sums all T rows"); `spatial_features`; regroup's output and mask; the fused map of PillarVFE -> PointPillarScatter -> regroup ->
SwapFusionEncoder with its state_dict schema; and the reference's own bf16-autocast deviation of the fusion net on this canvas
(make_golden._dev, weight sets 0..3; the front end stays fp32).  The test-side restatement tests/pillar_ref.py is checked against the
reference on the spot (1e-5), and so are the conditions without which a test on these inputs would hide failures: the folded shift
has both signs in at least a quarter of the channels each, and the relu(shift) contribution of the masked rows decides between 10 %
and 70 % of the outputs of the pillars with n_p < T."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

import make_golden as mg                      # first: puts the repository, this directory and the stand-ins in place
import cases_pillar as cp
from cobevt_amd.synth import fill_module_

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import pillar_ref as pr  # noqa: E402

from opencood.models.sub_modules.pillar_vfe import PillarVFE as R_PillarVFE  # noqa: E402
from opencood.models.sub_modules.point_pillar_scatter import PointPillarScatter as R_PointPillarScatter  # noqa: E402

REF = types.SimpleNamespace(PillarVFE=R_PillarVFE, PointPillarScatter=R_PointPillarScatter, SwapFusionEncoder=mg.R_swap.SwapFusionEncoder)


class Composition(nn.Module):
    """the reference's modules under PointPillarFuseBEVT's attribute names (state_dict keys, procedural fill)"""

    def __init__(self, args):
        super().__init__()
        self.pillar_vfe, self.scatter, self.fusion_net = cp.build(REF, args)


def _batch(vox):
    return {k: v.clone() for k, v in vox.items()}


def _front(comp, vox):
    """-> (pillar_features (P, 64), spatial_features (N, 64, ny, nx), per-row layer outputs before the ReLU (P, T, 64)) of the reference"""
    seen = {}
    pfn = comp.pillar_vfe.pfn_layers[0]
    h = pfn.register_forward_hook(lambda mod, i, o: seen.__setitem__("in", i[0].clone()))
    bd = comp.pillar_vfe(_batch(vox))
    h.remove()
    rows = bd["pillar_features"]
    bd = comp.scatter(bd)
    x = pfn.linear(seen["in"])
    if pfn.use_norm:
        x = pfn.norm(x.permute(0, 2, 1)).permute(0, 2, 1)
    return rows, bd["spatial_features"], x


def _conditions(name, comp, vox, rows, pre):
    n_p = vox["voxel_num_points"].long()
    t = pre.shape[1]
    part = n_p < t
    # the shift: the layer's response to a masked (all-zero) row, before the ReLU - the same in every masked row
    masked = pre[part][:, t - 1, :]
    s = masked[0]
    assert torch.equal(masked, s[None, :].expand_as(masked))
    per_row = torch.relu(pre)
    pos, neg = float((s > 0).float().mean()), float((s <= 0).float().mean())
    real = torch.arange(t)[None, :, None] < n_p[:, None, None]
    m_real = torch.where(real, per_row, torch.full_like(per_row, -1.0)).max(dim=1).values
    decided = (torch.relu(s)[None, :] > m_real)[part]
    assert torch.equal(rows[part][decided], torch.relu(s)[None, :].expand_as(m_real)[part][decided])
    frac = float(decided.float().mean())
    print("  %-22s shift > 0 in %.0f %% of the channels, <= 0 in %.0f %%; relu(shift) decides %.1f %% of the outputs of pillars with n_p < T"
          % (name, 100 * pos, 100 * neg, 100 * frac))
    assert pos >= 0.25 and neg >= 0.25, "the shift must have both signs in a quarter of the channels each"
    assert 0.10 <= frac <= 0.70, "the masked rows' term must decide between 10 % and 70 % of the outputs"


def gv21():
    out = {}
    vox = cp.voxels()
    n_p = vox["voxel_num_points"]
    assert int((n_p == cp.T).sum()) >= 50 and int((n_p == 1).sum()) >= 1 and int(((n_p > 1) & (n_p < cp.T)).sum()) >= 1
    ny, nx = cp.GRID
    cases = [(a, d, True, False) for a, d in cp.COMBOS] + [(True, False, False, False), (True, False, True, True)]
    for use_abs, dist, use_norm, dirty in cases:
        name = cp.combo_name(use_abs, dist, use_norm) + ("_dirty" if dirty else "")
        args = cp.model_args(use_abs, dist, use_norm)
        comp = fill_module_(Composition(args), cp.SEED)
        v = cp.voxels(dirty=True) if dirty else vox
        rows, spatial, per_row = _front(comp, v)
        if not dirty:
            _conditions(name, comp, v, rows, per_row)
        sd = comp.state_dict()
        w, s = pr.fold(sd, "pillar_vfe.pfn_layers.0.", use_norm)
        g = pr.geom(args["voxel_size"], args["lidar_range"])
        got = pr.pillar_features(v["voxel_features"], v["voxel_num_points"], v["voxel_coords"], w, s, g, use_abs, dist)
        mg._close("PillarVFE " + name, got, rows, tol=1e-5)
        out["pillar_features/" + name] = mg._np(rows)
        if dirty:
            clean = _front(comp, vox)[0]
            assert float((rows - clean).abs().max()) > 1e-3, "non-zero rows past n_p must move the mean"
        if (use_abs, dist, use_norm, dirty) != (True, False, True, False):
            continue
        # the default configuration (OpenCOOD's point-pillar yaml): scatter, regroup, fused map, schema, bf16 deviation
        mg._close("PointPillarScatter", pr.scatter(got, v["voxel_coords"], cp.AGENTS, ny, nx).permute(0, 3, 1, 2), spatial, tol=1e-5)
        out["spatial_features"] = mg._np(spatial)
        record_len = torch.tensor(cp.RECORD_LEN)
        grouped, mask = mg.R_regroup(spatial, record_len, cp.MAX_CAV)
        rg, rm = pr.regroup(spatial, cp.RECORD_LEN, cp.MAX_CAV)
        mg._close("regroup", rg, grouped, tol=0.0)
        assert torch.equal(rm, mask.float())
        out["regroup"], out["regroup_mask"] = mg._np(grouped), mg._np(mask)
        com_mask = mask[:, None, None, None, :].expand(mask.shape[0], ny, nx, 1, cp.MAX_CAV).contiguous()
        fused = comp.fusion_net(grouped, com_mask)
        mg._close("PointPillarFuseBEVT fused map",
                  pr.fused_map(sd, args, v["voxel_features"], v["voxel_num_points"], v["voxel_coords"], cp.RECORD_LEN), fused, tol=1e-5)
        out["fused_feature"] = mg._np(fused)
        out["keys"] = np.array(list(sd.keys()))
        out["shapes"] = np.array([",".join(str(int(d)) for d in t.shape) for t in sd.values()])
        dev = {}

        def build(seed):
            c = fill_module_(Composition(args), seed)
            _, sp, _ = _front(c, vox)
            gr, mk = mg.R_regroup(sp, record_len, cp.MAX_CAV)
            cm = mk[:, None, None, None, :].expand(mk.shape[0], ny, nx, 1, cp.MAX_CAV).contiguous()
            return lambda: c.fusion_net(gr, cm)
        mg._dev(dev, "PointPillarFuseBEVT", build)
        for k, val in dev.items():
            out["bf16_autocast/" + k] = val
    mg.save("gv21_point_pillar", **out)


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    gv21()
