"""The LiDAR pillar front end on the GPU: cobevt_pillar_vfe / cobevt_scatter_rows (csrc/pillar_vfe.hip) through ops, the PillarVFE /
PointPillarScatter mirrors and PointPillarFuseBEVT, against the reference fixture gv21 and the test-side restatement
(tests/pillar_ref.py, itself pinned to the reference to 1e-5).

Gates: fp32 1e-5 max-rel (a reordered fp32 sum measured 3e-7 on the CPU; ~30x that); bf16 4e-3 - the arithmetic is fp32 and the store
rounds once, unit round-off 2^-8 = 3.9e-3 (a rounded copy of the reference measured 2.0-3.4e-3)."""
import copy

import pytest
import torch

import cases_pillar as cp
import pillar_ref as pr
from cobevt_amd import host, ops
from cobevt_amd.host import pipeline
from cobevt_amd.host import runtime as rt
from cobevt_amd.synth import fill_module_
from util import BF16_FLOOR, RMS_FRACTION, assert_close, golden, rel_err, rms_rel_err

pytestmark = pytest.mark.gpu

MODES = ["bf16", "fp32", "fp32_split", "fp32_fast"]
DTYPES = [torch.bfloat16, torch.float32]
TOL = {torch.float32: 1e-5, torch.bfloat16: 4e-3}
CASES = [(a, d, True, False) for a, d in cp.COMBOS] + [(True, False, False, False), (True, False, True, True)]


def _to(vox, dev):
    return {k: v.to(dev) for k, v in vox.items()}


def _model(dev, *combo, **kw):
    return fill_module_(host.PointPillarFuseBEVT(cp.model_args(*combo, **kw)), cp.SEED).eval().to(dev)


def _folded(sd, args, dev):
    w, s = pr.fold(sd, "pillar_vfe.pfn_layers.0.", args["pillar_vfe"]["use_norm"])
    return w, s, w.to(dev), s.to(dev), pr.geom(args["voxel_size"], args["lidar_range"])


def _canvas(vox, wd, sd_, g, grid, dtype, record_len, max_cav, combo=(True, False), out=None, num_agents=None):
    rl = torch.tensor(record_len, dtype=torch.int32, device=wd.device)
    out, mask = ops.pillar_vfe_scatter(vox["voxel_features"], vox["voxel_num_points"], vox["voxel_coords"], wd, sd_, g, grid, dtype,
                                       use_absolute_xyz=combo[0], with_distance=combo[1], record_len=rl, max_cav=max_cav, out=out, num_agents=num_agents)
    torch.cuda.synchronize()
    return out, mask


# ---------------------------------------------------------------------------------------------- 1. fixture parity
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use_abs,dist,use_norm,dirty", CASES)
def test_pillar_features_match_reference(cuda, use_abs, dist, use_norm, dirty, dtype):
    """the PillarVFE mirror's dense rows against every `pillar_features` entry of gv21"""
    fx = golden("gv21_point_pillar")
    name = cp.combo_name(use_abs, dist, use_norm) + ("_dirty" if dirty else "")
    vfe = _model(cuda, use_abs, dist, use_norm).pillar_vfe
    bd = _to(cp.voxels(dirty=dirty), cuda)
    with host.compute_dtype(dtype):
        rows = vfe(bd)["pillar_features"]
    torch.cuda.synchronize()
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (300, 64)
    assert_close(rows, torch.from_numpy(fx["pillar_features/" + name]), TOL[dtype], "pillar_features " + name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_canvas_matches_reference(cuda, dtype):
    """the fused operator's canvas and mask against the reference's regroup(PointPillarScatter(PillarVFE)) output, and the
    PointPillarScatter mirror against `spatial_features`"""
    fx = golden("gv21_point_pillar")
    m = _model(cuda)
    vox = _to(cp.voxels(), cuda)
    with host.compute_dtype(dtype):
        canvas, mask = m.front_end({"processed_lidar": vox, "record_len": torch.tensor(cp.RECORD_LEN)})
        bd = dict(vox)
        bd["batch_size"] = cp.AGENTS
        spatial = m.scatter(m.pillar_vfe(bd))["spatial_features"]
        derived = m.scatter({"pillar_features": bd["pillar_features"], "voxel_coords": vox["voxel_coords"]})["spatial_features"]
    torch.cuda.synchronize()
    assert canvas.dtype == dtype and tuple(canvas.shape) == (2, 3, 16, 16, 64)
    ref = torch.from_numpy(fx["regroup"])                                   # (B, L, C, H, W)
    assert_close(canvas.permute(0, 1, 4, 2, 3), ref, TOL[dtype], "canvas")
    assert torch.equal(mask.cpu(), torch.from_numpy(fx["regroup_mask"]).float())
    assert bool((canvas.permute(0, 1, 4, 2, 3).float().cpu()[ref == 0] == 0).all())          # empty cells, the padded slot
    assert tuple(spatial.shape) == (3, 64, 16, 16) and spatial.permute(0, 2, 3, 1).is_contiguous()
    assert_close(spatial, torch.from_numpy(fx["spatial_features"]), TOL[dtype], "spatial_features")
    assert torch.equal(derived, spatial)                                    # batch size derived from the coordinates (synchronising)


# ---------------------------------------------------------------------------------------------- 2. exact properties
def test_exact_properties(cuda):
    """bf16 = the rounded fp32 result; fp32 bit-identical in all three libraries; two runs bit-identical; the fused canvas = the
    stand-alone PillarVFE -> PointPillarScatter -> ops.regroup composition, mask included"""
    m = _model(cuda)
    vox = _to(cp.voxels(), cuda)
    batch = {"processed_lidar": vox, "record_len": torch.tensor(cp.RECORD_LEN)}
    got = {}
    for mode in MODES:
        with host.compute_dtype(mode):
            got[mode] = m.front_end(batch)
            again = m.front_end(batch)
            rows = m.pillar_vfe(dict(vox))["pillar_features"]
            bd = dict(vox)
            bd["batch_size"] = cp.AGENTS
            spatial = m.scatter(m.pillar_vfe(bd))["spatial_features"]
            comp, comp_mask = ops.regroup(rt.to_nhwc(spatial), torch.tensor(cp.RECORD_LEN, dtype=torch.int32, device=cuda), cp.MAX_CAV)
        torch.cuda.synchronize()
        assert torch.equal(got[mode][0], again[0]) and torch.equal(got[mode][1], again[1]), mode
        assert torch.equal(got[mode][0], comp) and torch.equal(got[mode][1], comp_mask), mode
        got[mode + ".rows"] = rows
    assert torch.equal(got["bf16"][0], got["fp32"][0].to(torch.bfloat16))
    assert torch.equal(got["bf16.rows"], got["fp32.rows"].to(torch.bfloat16).float())
    for mode in ("fp32_split", "fp32_fast"):
        assert torch.equal(got[mode][0], got["fp32"][0]) and torch.equal(got[mode + ".rows"], got["fp32.rows"]), mode


# ---------------------------------------------------------------------------------------------- 3. shapes
# (pillars per agent, T, (ny, nx), record_len, max_cav, (use_absolute_xyz, with_distance))
SHAPES = {
    "5x7": ([13, 9, 11], 32, (5, 7), [2, 1], 3, (True, True)),
    "8x24_T5": ([70, 60, 62], 5, (8, 24), [2, 1], 3, (False, False)),
    "P0": ([0, 0, 0], 32, (5, 7), [2, 1], 3, (True, False)),
    "P1": ([1], 32, (5, 7), [1], 1, (True, False)),
    "P1000": ([400, 350, 250], 32, (24, 24), [2, 1], 3, (False, True)),
    "one_agent_T5": ([30], 5, (8, 24), [1], 1, (True, False)),
    "slot_past_max_cav": ([20, 20, 20], 32, (5, 7), [3], 2, (True, False)),
    # sample 0 holds more agents than max_cav: sample 1's agent has index 4 >= B * max_cav and must still land in slot (1, 0)
    "later_sample_past_B_max_cav": ([6, 6, 6, 6, 6], 32, (5, 7), [4, 1], 2, (True, False)),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_against_restatement(cuda, shape, dtype):
    counts, t, grid, record_len, max_cav, combo = SHAPES[shape]
    args = cp.model_args(combo[0], combo[1], grid=grid, max_cav=max_cav)
    sd = fill_module_(host.PointPillarFuseBEVT(copy.deepcopy(args)), cp.SEED).state_dict()
    w, s, wd, sd_, g = _folded(sd, args, cuda)
    vox = cp.voxels(counts=counts, t=t, grid=grid, tag="shape." + shape)
    ref, ref_mask = pr.canvas(vox["voxel_features"], vox["voxel_num_points"], vox["voxel_coords"], w, s, g, grid[0], grid[1],
                              record_len, max_cav, combo[0], combo[1])
    vd = _to(vox, cuda)
    out = torch.full((len(record_len), max_cav, grid[0], grid[1], 64), float("nan"), device=cuda, dtype=dtype)
    got, mask = _canvas(vd, wd, sd_, g, grid, dtype, record_len, max_cav, combo, out=out)
    assert got.data_ptr() == out.data_ptr() and bool(torch.isfinite(got).all())
    assert_close(got, ref, TOL[dtype], "canvas " + shape)
    assert torch.equal(mask.cpu(), ref_mask)
    occ, _ = pr.regroup(pr.scatter(torch.ones(sum(counts), 1), vox["voxel_coords"], len(counts), grid[0], grid[1]), record_len, max_cav)
    occupied = occ[..., 0] > 0
    assert int(occupied.sum()) == sum(counts[:sum(min(r, max_cav) for r in record_len)])
    assert bool((got.float().cpu()[~occupied] == 0).all()), "cells without a pillar must be exactly 0"
    # int64 index tensors are converted on the device; the dense rows of the same pillars
    got64, _ = _canvas({"voxel_features": vd["voxel_features"], "voxel_num_points": vd["voxel_num_points"].long(),
                        "voxel_coords": vd["voxel_coords"].long()}, wd, sd_, g, grid, dtype, record_len, max_cav, combo)
    assert torch.equal(got64, got)
    rows = ops.pillar_vfe_rows(vd["voxel_features"], vd["voxel_num_points"], vd["voxel_coords"], wd, sd_, g, dtype, combo[0], combo[1])
    torch.cuda.synchronize()
    assert tuple(rows.shape) == (sum(counts), 64)
    if sum(counts):
        assert_close(rows, pr.pillar_features(vox["voxel_features"], vox["voxel_num_points"], vox["voxel_coords"], w, s, g, *combo),
                     TOL[dtype], "rows " + shape)


# ---------------------------------------------------------------------------------------------- 4. skipped rows
@pytest.mark.parametrize("dtype", DTYPES)
def test_skipped_rows_are_never_written(cuda, dtype):
    """rows with n = -1, n = N, y = ny, x = nx, x = -1 and n_p = 0 change nothing, and nothing outside the canvas is touched: the
    canvas is the interior of a larger buffer whose margins hold a marker"""
    grid, record_len, max_cav = (5, 7), [2, 1], 3
    args = cp.model_args(grid=grid)
    sd = fill_module_(host.PointPillarFuseBEVT(copy.deepcopy(args)), cp.SEED).state_dict()
    _, _, wd, sd_, g = _folded(sd, args, cuda)
    vox = cp.voxels(counts=[13, 9, 11], grid=grid, tag="skip")
    clean, clean_mask = _canvas(_to(vox, cuda), wd, sd_, g, grid, dtype, record_len, max_cav)
    extra = cp.voxels(counts=[6], grid=grid, dirty=True, tag="skip.extra")
    extra["voxel_coords"] = torch.tensor([[-1, 0, 2, 3], [3, 0, 2, 3], [0, 0, 5, 3], [1, 0, 2, 7], [2, 0, 2, -1], [0, 0, 4, 6]], dtype=torch.int32)
    extra["voxel_num_points"][5] = 0
    assert not bool(((vox["voxel_coords"][:, 0] == 0) & (vox["voxel_coords"][:, 2] == 4) & (vox["voxel_coords"][:, 3] == 6)).any())
    both = {k: torch.cat([extra[k][:3], vox[k], extra[k][3:]]) for k in vox}
    numel, margin = clean.numel(), 256
    big = torch.full((numel + 2 * margin,), 7.0, device=cuda, dtype=dtype)
    out = big[margin:margin + numel].view(clean.shape)
    got, mask = _canvas(_to(both, cuda), wd, sd_, g, grid, dtype, record_len, max_cav, out=out)
    bounded, _ = _canvas(_to(both, cuda), wd, sd_, g, grid, dtype, [2, 2], max_cav, num_agents=3)     # n = 3 inside record_len, >= N
    assert torch.equal(bounded, clean)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got, clean) and torch.equal(mask, clean_mask)
    assert bool((big[:margin] == 7.0).all()) and bool((big[margin + numel:] == 7.0).all())
    # the stand-alone scatter keeps the same rules (it does not know the point counts)
    rows = torch.ones(both["voxel_coords"].shape[0], 64, device=cuda, dtype=dtype)
    sc = ops.scatter_rows(rows, both["voxel_coords"].to(cuda), 3, grid)
    torch.cuda.synchronize()
    assert int((sc.float().sum(-1) > 0).sum()) == 33 + 1            # the n_p = 0 row is a valid row for the scatter


# ---------------------------------------------------------------------------------------------- 5. the model
def _bf16_gates(fx, key):
    """max(1e-2, the reference's own bf16-autocast deviation of this output) and the rms gate derived as in tests/util.py"""
    r = fx["bf16_autocast/" + key]
    return max(BF16_FLOOR, float(r[0])), max(RMS_FRACTION[True] * BF16_FLOOR, float(r[1]))


@pytest.fixture(scope="module")
def lidar_model(cuda):
    m = _model(cuda)
    return m, {"processed_lidar": _to(cp.voxels(), cuda), "record_len": torch.tensor(cp.RECORD_LEN, dtype=torch.int32, device=cuda)}


@pytest.mark.parametrize("mode", MODES)
def test_model_matches_reference(lidar_model, mode):
    """PointPillarFuseBEVT against the reference composition's fused map (gv21): fp32 modes 1e-3; bf16 max(1e-2, the reference's own
    bf16-autocast deviation of the fusion net on this canvas); and bit-identical to fusion_net.forward_blhwc on the operator's output"""
    m, batch = lidar_model
    fx = golden("gv21_point_pillar")
    ref = torch.from_numpy(fx["fused_feature"])
    with torch.no_grad(), host.compute_dtype(mode):
        out = m(batch)["fused_feature"]
        x, cav = m.front_end(batch)
        b, l, h, w, _ = x.shape
        direct = m.fusion_net.forward_blhwc(x, cav[:, None, None, None, :].expand(b, h, w, 1, l).contiguous())
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 64, 16, 16)
    assert torch.equal(out, direct.permute(0, 3, 1, 2).float())
    if mode == "bf16":
        tol, rms_gate = _bf16_gates(fx, "PointPillarFuseBEVT")
        e, r = rel_err(out, ref), rms_rel_err(out, ref)
        assert e <= tol and r <= rms_gate, "fused map bf16: max-rel %.3e (gate %.2e) rms-rel %.3e (gate %.2e)" % (e, tol, r, rms_gate)
    else:
        assert_close(out, ref, 1e-3, "PointPillarFuseBEVT fused map " + mode)


def test_model_padded_rows_touch_only_their_sample(lidar_model):
    """the third agent (sample 1) with its rows marked n = -1: sample 0 is bit-identical, sample 1 is not"""
    m, batch = lidar_model
    lidar = dict(batch["processed_lidar"])
    coords = lidar["voxel_coords"].clone()
    coords[coords[:, 0] == 2, 0] = -1
    lidar["voxel_coords"] = coords
    with torch.no_grad(), host.compute_dtype("bf16"):
        full = m(batch)["fused_feature"]
        part = m({"processed_lidar": lidar, "record_len": batch["record_len"]})["fused_feature"]
    torch.cuda.synchronize()
    assert torch.equal(full[0], part[0]) and not torch.equal(full[1], part[1])


# ---------------------------------------------------------------------------------------------- 6. graph replay
def _padded(vox, p_fixed):
    p = vox["voxel_coords"].shape[0]
    pad = p_fixed - p
    coords = torch.cat([vox["voxel_coords"], torch.tensor([[-1, 0, 0, 0]], dtype=torch.int32).expand(pad, 4)])
    return {"voxel_features": torch.cat([vox["voxel_features"], torch.zeros(pad, *vox["voxel_features"].shape[1:])]),
            "voxel_coords": coords.contiguous(), "voxel_num_points": torch.cat([vox["voxel_num_points"], torch.zeros(pad, dtype=torch.int32)])}


def test_graph_replay_equals_eager(cuda, lidar_model):
    """pipeline.CapturedCall over the model at a fixed padded P = 320 (padding rows carry n = -1): each replay equals its eager forward"""
    m, _ = lidar_model
    sets = [_to(_padded(cp.voxels(), 320), cuda), _to(_padded(cp.voxels(counts=[90, 80, 70], seed=1, tag="replay"), 320), cuda)]
    rl = torch.tensor(cp.RECORD_LEN, dtype=torch.int32, device=cuda)

    def fn(vf, coords, npts, record_len):
        return m({"processed_lidar": {"voxel_features": vf, "voxel_coords": coords, "voxel_num_points": npts}, "record_len": record_len})
    with torch.no_grad(), host.compute_dtype("bf16"):
        eager = [fn(v["voxel_features"], v["voxel_coords"], v["voxel_num_points"], rl)["fused_feature"].clone() for v in sets]
        run = pipeline.CapturedCall(fn, sets[0]["voxel_features"], sets[0]["voxel_coords"], sets[0]["voxel_num_points"], rl)
        assert run.graph is not None
        for i in (0, 1, 0):
            v = sets[i]
            got = run.step(v["voxel_features"], v["voxel_coords"], v["voxel_num_points"], rl)["fused_feature"]
            torch.cuda.synchronize()
            assert torch.equal(got, eager[i]), i
    assert not torch.equal(eager[0], eager[1])


# ---------------------------------------------------------------------------------------------- 7. full size, once
FULL_COUNTS = [12000, 9000, 8000, 7500, 7000, 6500, 5500, 4500]          # 60 000 pillars over 8 agents, uneven
FULL_GRID = (256, 256)


@pytest.fixture(scope="module")
def full_size():
    """voxels and the restatement's canvas on the CPU, computed once for both dtypes (OpenCOOD's configuration: absolute xyz, no distance)"""
    args = cp.model_args(grid=FULL_GRID, max_cav=8)
    sd = fill_module_(host.PointPillarFuseBEVT(copy.deepcopy(args)), cp.SEED).state_dict()
    vox = cp.voxels(counts=FULL_COUNTS, grid=FULL_GRID, stride=40503, tag="full")
    w, s = pr.fold(sd, "pillar_vfe.pfn_layers.0.", True)
    g = pr.geom(args["voxel_size"], args["lidar_range"])
    rows = torch.cat([pr.pillar_features(vox["voxel_features"][i:i + 10000], vox["voxel_num_points"][i:i + 10000],
                                         vox["voxel_coords"][i:i + 10000], w, s, g) for i in range(0, sum(FULL_COUNTS), 10000)])
    ref, mask = pr.regroup(pr.scatter(rows, vox["voxel_coords"], 8, *FULL_GRID), [8], 8)
    return vox, w, s, g, ref, mask


@pytest.mark.parametrize("dtype", DTYPES)
def test_full_size_front_end(cuda, full_size, dtype):
    """8 agents x 256 x 256, T = 32, 60 000 pillars: the front end alone against the restatement (SwapFusionEncoder at this size is
    test_lidar_fusebevt_full_size's)"""
    vox, w, s, g, ref, ref_mask = full_size
    got, mask = _canvas(_to(vox, cuda), w.to(cuda), s.to(cuda), g, FULL_GRID, dtype, [8], 8)
    assert tuple(got.shape) == (1, 8, 256, 256, 64)
    assert_close(got, ref, TOL[dtype], "full-size canvas")
    assert torch.equal(mask.cpu(), ref_mask)
    assert int((got.float().abs().sum(-1) > 0).sum()) <= sum(FULL_COUNTS)
