"""The LiDAR pillar front end (PillarVFE + PointPillarScatter + regroup in front of FuseBEVT) without a GPU: registry, module schema
and contract against the reference fixture gv21, and the test-side restatement (tests/pillar_ref.py) against the reference's outputs."""
import copy

import pytest
import torch

import cases_pillar as cp
import pillar_ref as pr
from cobevt_amd import host
from cobevt_amd.lib import CobevtHipError
from cobevt_amd.registry import create_model
from cobevt_amd.synth import fill_module_
from util import golden, rel_err

CASES = [(a, d, True, False) for a, d in cp.COMBOS] + [(True, False, False, False), (True, False, True, True)]


def _model(*combo):
    return create_model({"model": {"core_method": "point_pillar_fusebevt", "args": cp.model_args(*combo)}})


def test_create_model_finds_point_pillar_fusebevt():
    m = _model()
    assert type(m) is host.PointPillarFuseBEVT
    assert isinstance(m.pillar_vfe, host.PillarVFE) and isinstance(m.scatter, host.PointPillarScatter)
    assert isinstance(m.fusion_net, host.SwapFusionEncoder) and isinstance(m.pillar_vfe.pfn_layers[0], host.PFNLayer)
    assert m.pillar_vfe.get_output_feature_dim() == 64 and (m.scatter.nx, m.scatter.ny, m.scatter.nz) == (16, 16, 1)
    assert m.pillar_vfe.x_offset == 0.4 / 2 - 3.2 and m.pillar_vfe.z_offset == 4 / 2 - 3.0


def test_state_dict_schema_matches_reference():
    fx = golden("gv21_point_pillar")
    sd = _model().state_dict()
    assert list(sd.keys()) == [str(k) for k in fx["keys"]]
    assert [",".join(str(int(d)) for d in v.shape) for v in sd.values()] == [str(s) for s in fx["shapes"]]
    assert "pillar_vfe.pfn_layers.0.linear.weight" in sd and "pillar_vfe.pfn_layers.0.norm.num_batches_tracked" in sd
    nonorm = _model(True, False, False).state_dict()
    assert "pillar_vfe.pfn_layers.0.linear.bias" in nonorm and "pillar_vfe.pfn_layers.0.norm.weight" not in nonorm


@pytest.mark.parametrize("use_abs,dist,use_norm,dirty", CASES)
def test_restatement_replays_pillar_features(use_abs, dist, use_norm, dirty):
    """tests/pillar_ref.py (folded BatchNorm, relu(shift) of the masked rows in the maximum, mean over all T rows) against every
    `pillar_features` entry of the reference fixture"""
    fx = golden("gv21_point_pillar")
    args = cp.model_args(use_abs, dist, use_norm)
    sd = fill_module_(host.PointPillarFuseBEVT(copy.deepcopy(args)), cp.SEED).state_dict()
    v = cp.voxels(dirty=dirty)
    w, s = pr.fold(sd, "pillar_vfe.pfn_layers.0.", use_norm)
    got = pr.pillar_features(v["voxel_features"], v["voxel_num_points"], v["voxel_coords"], w, s,
                             pr.geom(args["voxel_size"], args["lidar_range"]), use_abs, dist)
    ref = torch.from_numpy(fx["pillar_features/" + cp.combo_name(use_abs, dist, use_norm) + ("_dirty" if dirty else "")])
    assert rel_err(got, ref) <= 1e-5


def test_restatement_replays_scatter_regroup_and_fused_map():
    fx = golden("gv21_point_pillar")
    args = cp.model_args()
    sd = fill_module_(host.PointPillarFuseBEVT(copy.deepcopy(args)), cp.SEED).state_dict()
    v = cp.voxels()
    ny, nx = cp.GRID
    w, s = pr.fold(sd, "pillar_vfe.pfn_layers.0.", True)
    rows = pr.pillar_features(v["voxel_features"], v["voxel_num_points"], v["voxel_coords"], w, s,
                              pr.geom(args["voxel_size"], args["lidar_range"]))
    spatial = pr.scatter(rows, v["voxel_coords"], cp.AGENTS, ny, nx)
    assert rel_err(spatial.permute(0, 3, 1, 2), torch.from_numpy(fx["spatial_features"])) <= 1e-5
    grouped, mask = pr.regroup(spatial, cp.RECORD_LEN, cp.MAX_CAV)
    assert rel_err(grouped.permute(0, 1, 4, 2, 3), torch.from_numpy(fx["regroup"])) <= 1e-5
    assert torch.equal(mask, torch.from_numpy(fx["regroup_mask"]).float())
    # empty cells and the padded agent slot are exactly zero in the reference as in the restatement
    assert torch.equal(grouped.permute(0, 1, 4, 2, 3) == 0, torch.from_numpy(fx["regroup"]) == 0)
    with torch.no_grad():
        fused = pr.fused_map(sd, args, v["voxel_features"], v["voxel_num_points"], v["voxel_coords"], cp.RECORD_LEN)
    assert rel_err(fused, torch.from_numpy(fx["fused_feature"])) <= 1e-5


def test_unsupported_configurations_raise():
    ok = cp.model_args()
    cases = []
    a = copy.deepcopy(ok); a["pillar_vfe"]["num_filters"] = [64, 64]; cases.append((a, "one PFN layer"))          # noqa: E702
    a = copy.deepcopy(ok); a["pillar_vfe"]["num_filters"] = [32]; cases.append((a, "64 output channels"))          # noqa: E702
    a = copy.deepcopy(ok); a["point_pillar_scatter"]["grid_size"] = [16, 16, 2]; cases.append((a, "nz = 1"))       # noqa: E702
    a = copy.deepcopy(ok); a["pillar_vfe"]["max_points_per_voxel"] = 64; cases.append((a, "T = 32"))               # noqa: E702
    a = copy.deepcopy(ok); a["max_points_per_voxel"] = 33; cases.append((a, "T = 32"))                             # noqa: E702
    a = copy.deepcopy(ok); a["fax_fusion"]["input_dim"] = 128; cases.append((a, "64 channels"))                    # noqa: E702
    for args, what in cases:
        with pytest.raises(CobevtHipError, match=what):
            host.PointPillarFuseBEVT(args)
    with pytest.raises(CobevtHipError, match="F = 4"):
        host.PillarVFE(cp.vfe_cfg(), 5, cp.VOXEL_SIZE, cp.LIDAR_RANGE)
    with pytest.raises(CobevtHipError, match="last layer"):
        host.PFNLayer(10, 64, True, last_layer=False)


def _batch():
    v = cp.voxels()
    return {"processed_lidar": v, "record_len": torch.tensor(cp.RECORD_LEN)}


def test_cpu_forward_raises_no_fallback():
    m = fill_module_(_model(), cp.SEED).eval()
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        m(_batch())
    v = cp.voxels()
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        m.pillar_vfe(dict(v))
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        m.scatter({"pillar_features": torch.zeros(v["voxel_coords"].shape[0], 64), "voxel_coords": v["voxel_coords"], "batch_size": 3})


def test_train_mode_forward_raises():
    m = fill_module_(_model(), cp.SEED).train()
    with pytest.raises(CobevtHipError, match="call .eval\\(\\) first"):
        m(_batch())
    with pytest.raises(CobevtHipError, match="call .eval\\(\\) first"):
        m.pillar_vfe(dict(cp.voxels()))
