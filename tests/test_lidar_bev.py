"""The LiDAR BEV (PIXOR) pre- and post-processor without a device: the fixture gv28_lidar_bev.npz (the reference's own run, written
by tests/golden/make_golden_bev.py) is reproduced by the float64 restatement tests/bev_ref.py within the deviations stored in it,
the case conditions hold, and the host layer validates its arguments, refuses CPU tensors and resolves the registry names."""
import ctypes

import numpy as np
import pytest
import torch

import bev_ref as br
import cases_bev as cb
from cobevt_amd import host, lib, ops, registry
from cobevt_amd.lib import CobevtHipError
from util import golden

SLACK = 1e-12          # float64 libm differences between the machine that wrote the fixture and this one


@pytest.fixture(scope="module")
def gv():
    return golden("gv28_lidar_bev")


# ---------------------------------------------------------------------------------------------- the fixture against the restatement
@pytest.mark.parametrize("name,designed,rm,em", [("pre_main", False, False, False), ("pre_main_masks", False, True, True),
                                                 ("pre_boundary_r0_e0", True, False, False), ("pre_boundary_r0_e1", True, False, True),
                                                 ("pre_boundary_r1_e0", True, True, False), ("pre_boundary_r1_e1", True, True, True)])
def test_preprocessor_fixture(gv, name, designed, rm, em):
    clouds = cb.points_boundary() if designed else cb.points_main()
    mine = br.bev_points(clouds, cb.GEOM, cb.LIDAR_RANGE, rm, em)
    ref = gv[name + "_bev"]
    assert ref.dtype == np.float32 and ref.shape == (2, 9, 96, 80)
    assert np.array_equal(ref[:, :-1], mine[:, :-1])
    d = float(np.abs(ref[:, -1].astype(np.float64) - mine[:, -1]).max())
    assert d <= float(gv[name + "_dev"]) + SLACK
    cb.pre_conditions(min(br.kept_mask(p, cb.GEOM, cb.LIDAR_RANGE, rm, em)[2] for p in clouds), designed)
    # each mask removes something, and the rule drops something
    kept = [int(br.kept_mask(p, cb.GEOM, cb.LIDAR_RANGE, rm, em)[0].sum()) for p in clouds]
    plain = [int(br.kept_mask(p, cb.GEOM, cb.LIDAR_RANGE)[0].sum()) for p in clouds]
    assert all(0 < k <= q < len(p) for k, q, p in zip(kept, plain, clouds))
    assert (kept == plain) == (not rm and not em)


def test_boundary_case_design():
    """what the designed rows are for: truncation (not floor) keeps a point just below the origin in cell 0; upper faces are out"""
    p = cb.points_boundary()[0]
    keep, idx, _ = br.kept_mask(p, cb.GEOM, cb.LIDAR_RANGE)
    g = cb.GEOM
    below_origin = (p[:, 0] < g["L1"]) & (p[:, 0] > g["L1"] - cb.RES)
    assert below_origin.sum() == 2 and keep[below_origin].all() and (idx[below_origin, 0] == 0).all()
    assert not keep[p[:, 0] == g["L2"]].any() and not keep[p[:, 0] == np.float32(g["L1"] - cb.RES)].any()
    assert not keep[~np.isfinite(p).all(axis=1)].any() and not keep[np.abs(p[:, 3]) >= 256].any()
    on_face = keep & ((p[:, 0] - g["L1"]) / cb.RES == np.round((p[:, 0] - g["L1"]) / cb.RES))
    assert on_face.sum() >= 4


@pytest.mark.parametrize("name,axis", [("label_main", False), ("label_axis", True)])
def test_label_fixture(gv, name, axis):
    gt, mask = cb.labels_axis() if axis else cb.labels_main()
    dev = float(gv[name + "_dev"])
    assert dev <= 2.0 ** -24 * 16        # the reference casts a float64 map to fp32: half an ulp of values below 16
    for b in range(gt.shape[0]):
        mine = br.generate_label(gt[b], mask[b], cb.GEOM, cb.TARGET_MEAN, cb.TARGET_STD_DEV)
        n = int(mask[b].sum())
        if n:
            cb.label_conditions(mine, axis)
        ref = gv[name + "_label_map"][b]
        assert np.array_equal(ref[0], mine["label_map"][0])
        assert float(np.abs(ref.astype(np.float64) - mine["label_map"]).max()) <= dev + SLACK
        assert np.array_equal(gv[name + "_corners"][b, :n], mine["bev_corners"]) and not gv[name + "_corners"][b, n:].any()
        assert int(gv[name + "_num_valid"][b]) == n


def test_label_case_design():
    """the overlap, the masked box and the box across the border do what they are there for"""
    gt, mask = cb.labels_main()
    assert mask[0].tolist()[:5] == [1, 1, 0, 1, 1] and not mask[1].any()
    one = lambda k: br.generate_label(gt[0], np.eye(cb.MAX_NUM)[k], cb.GEOM, cb.TARGET_MEAN, cb.TARGET_STD_DEV)["label_map"]   # noqa: E731
    a, b, masked, border = one(0), one(1), one(2), one(3)
    both = (a[0] == 1) & (b[0] == 1)
    full = br.generate_label(gt[0], mask[0], cb.GEOM, cb.TARGET_MEAN, cb.TARGET_STD_DEV)["label_map"]
    assert both.sum() >= 1 and np.array_equal(full[:, both], b[:, both]) and not np.array_equal(a[:, both], b[:, both])
    assert masked[0].sum() >= 4 and not full[0][masked[0] == 1].any()
    lx, ly, _ = cb.GEOM["label_shape"]
    corners = br.corners_f64(gt[0][3:4])[0]
    assert 0 < border[0].sum() and (corners[:, 0].max() > cb.GEOM["L2"] or corners[:, 1].min() < cb.GEOM["W1"])


@pytest.mark.parametrize("name,case,geom", [("post_two", "post_two_cavs", "GEOM"), ("post_range", "post_out_of_range", "GEOM"),
                                            ("post_cut", "post_cut", "GEOM_CUT"), ("post_none", "post_nothing", "GEOM")])
def test_post_fixture(gv, name, case, geom):
    cavs, geom = getattr(cb, case)(), getattr(cb, geom)
    out = br.post_process(cavs, geom, cb.TARGET_MEAN, cb.TARGET_STD_DEV, cb.SCORE_THRESHOLD, cb.NMS_THRESH, faithful=False)
    cb.post_conditions(out, expect_none=name == "post_none")
    assert bool(gv[name + "_none"]) == (name == "post_none")
    if name == "post_none":
        return
    assert np.array_equal(gv[name + "_index"], out["index"])
    assert (len(out["index"]) == 0) == (name == "post_range") and len(out["picked_all"]) > 0
    if name == "post_cut":
        assert len(out["candidates"]) == cb.CUT_CANDIDATES > 1000
    if len(out["index"]):
        dev_box, dev_score = [float(v) for v in gv[name + "_dev"]]
        assert float(np.abs(gv[name + "_boxes"].astype(np.float64) - out["boxes"]).max()) <= dev_box + 1e-9
        assert float(np.abs(gv[name + "_scores"].astype(np.float64) - out["scores"]).max()) <= dev_score + SLACK
        # the reference's fp32 deviation is a few ulp of the largest coordinate
        assert dev_box <= 64 * np.spacing(np.float32(gv[name + "_maxcoord"])) and dev_score <= 4 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------- host layer
def test_preprocessor_constructor():
    p = host.BevPreprocessor(cb.pre_params(True, False), train=True)
    assert p.input_shape == (96, 80, 9) and p.range_mask and not p.ego_mask and p.origin == (-12.0, -10.0, -1.25)
    bad = cb.pre_params()
    bad["geometry_param"]["input_shape"] = (96, 80, 8)
    with pytest.raises(CobevtHipError, match="disagrees with the ranges and res"):
        host.BevPreprocessor(bad, train=True)
    bad = cb.pre_params()
    del bad["geometry_param"]["H1"]
    with pytest.raises(CobevtHipError, match="geometry_param lacks H1"):
        host.BevPreprocessor(bad, train=True)
    with pytest.raises(CobevtHipError, match="a list or a dict"):
        p.collate_batch(3)


def test_postprocessor_constructor():
    p = host.LidarBevPostprocessor(cb.post_params(), train=True)
    assert p.generate_anchor_box() is None
    assert p.target_mean.tolist() == list(cb.TARGET_MEAN) and p.target_std_dev.tolist() == list(cb.TARGET_STD_DEV)
    bad = cb.post_params()
    bad["geometry_param"]["label_shape"] = (24, 20, 6)
    with pytest.raises(CobevtHipError, match=r"label_shape must be \(lx, ly, 7\)"):
        host.LidarBevPostprocessor(bad, train=True)
    hwl = host.LidarBevPostprocessor(cb.post_params(order="hwl"), train=True)
    with pytest.raises(CobevtHipError, match="only supports the 'lwh' bbx order"):
        hwl.generate_label_batch(torch.zeros(1, 4, 7), torch.zeros(1, 4))
    with pytest.raises(CobevtHipError, match=r"\(B, max_num, 7\) with mask \(B, max_num\)"):
        p.generate_label_batch(torch.zeros(1, 4, 7), torch.zeros(1, 5))
    with pytest.raises(CobevtHipError, match=r"\(max_num, 7\) with mask \(max_num,\)"):
        p.generate_label(gt_box_center=torch.zeros(1, 4, 7), mask=torch.zeros(4))


def test_no_cpu_fallback():
    pre = host.BevPreprocessor(cb.pre_params(), train=False)
    post = host.LidarBevPostprocessor(cb.post_params(), train=False)
    pts, offs = torch.zeros(8, 4), torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        pre.preprocess_batch(pts, offs)
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        ops.bev_points(pts, offs, cb.LIDAR_RANGE, (-12.0, -10.0, -1.25), 0.25, (96, 80, 9))
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        post.generate_label_batch(torch.zeros(1, 4, 7), torch.zeros(1, 4))
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        ops.bev_labels(torch.zeros(1, 4, 7), torch.zeros(1, 4), (-12.0, -10.0), 0.25, 4, (24, 20, 7))
    data = {0: {"transformation_matrix": torch.eye(4)}}
    output = {0: {"cls": torch.zeros(1, 1, 24, 20), "reg": torch.zeros(1, 6, 24, 20)}}
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        post.post_process(data, output)
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        post.post_process_device(data, output)
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        post.denormalize_reg_map(torch.zeros(24, 20, 6))
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        post.reg_map_to_bbx_corners(torch.zeros(24, 20, 6), torch.zeros(24, 20, dtype=torch.bool))


def test_ops_validation_before_any_device_use():
    with pytest.raises(CobevtHipError, match="1 .. 16 cavs"):
        ops.bev_post_process([], (-12.0, -10.0), 0.25, 4, 0.5, 0.15)
    with pytest.raises(CobevtHipError, match="res and downsample_rate must be positive"):
        ops.bev_post_process([(None, None, None)], (-12.0, -10.0), 0.0, 4, 0.5, 0.15)
    with pytest.raises(CobevtHipError, match="6 finite values each"):
        ops.bev_post_process([(None, None, None)], (-12.0, -10.0), 0.25, 4, 0.5, 0.15, target_std_dev=(1, 1, 1, 1, 1, 0))
    with pytest.raises(CobevtHipError, match=r"label_shape must be \(nx, ny, 7\)"):
        ops.bev_labels(torch.zeros(1, 4, 7), torch.zeros(1, 4), (-12.0, -10.0), 0.25, 4, (24, 20, 6))
    with pytest.raises(CobevtHipError, match="at most 128 ground-truth slots"):
        ops.bev_labels(torch.zeros(1, 129, 7), torch.zeros(1, 129), (-12.0, -10.0), 0.25, 4, (24, 20, 7))


def test_registry():
    names = {"BevPreprocessor": host.BevPreprocessor, "SpVoxelPreprocessor": host.SpVoxelPreprocessor,
             "RgbPreprocessor": host.RgbPreProcessor}
    sp = dict(core_method="SpVoxelPreprocessor", cav_lidar_range=[-12.8, -12.8, -3, 12.8, 12.8, 1],
              args=dict(voxel_size=[0.4, 0.4, 4], max_points_per_voxel=32, max_voxel_train=100, max_voxel_test=100))
    cfgs = {"BevPreprocessor": cb.pre_params(), "SpVoxelPreprocessor": sp,
            "RgbPreprocessor": dict(core_method="RgbPreprocessor", args=dict(mean=[0.5] * 3, std=[0.2] * 3))}
    for name, cls in names.items():
        obj = registry.build_preprocessor(cfgs[name], train=True)
        assert type(obj) is cls and obj.train is True and obj.params is cfgs[name]
    import cases_detect as cd
    posts = {"BevPostprocessor": (host.LidarBevPostprocessor, cb.post_params()),
             "VoxelPostprocessor": (host.VoxelPostprocessor, cd.anchor_params((2, 3), "hwl", 6.0, 4.0)),
             "CameraBevPostprocessor": (host.CameraBevPostprocessor, dict(core_method="CameraBevPostprocessor"))}
    for name, (cls, cfg) in posts.items():
        cfg = dict(cfg, core_method=name)
        obj = registry.build_postprocessor(cfg, train=False)
        assert type(obj) is cls and obj.train is False
    with pytest.raises(ValueError, match="'PixorPreprocessor' is not found"):
        registry.build_preprocessor(dict(core_method="PixorPreprocessor"), train=True)
    with pytest.raises(ValueError, match="'BasePostprocessor' is not found"):
        registry.build_postprocessor(dict(core_method="BasePostprocessor"), train=True)


# ---------------------------------------------------------------------------------------------- the C entry points without a device
def test_null_pointers_return_code_1():
    L = lib.load()
    need = ctypes.c_long(0)
    dims = (ctypes.c_long * 8)(100, 2, 96, 80, 9, 0, 0, 0)
    assert L.cobevt_bev_points_scratch(None, ctypes.byref(need)) == 1 and L.cobevt_bev_points_scratch(dims, None) == 1
    assert L.cobevt_bev_points_scratch(dims, ctypes.byref(need)) == 0 and need.value == 3 * 2 * 96 * 80
    bad = (ctypes.c_long * 8)(100, 2, 96, 80, 1, 0, 0, 0)
    assert L.cobevt_bev_points_scratch(bad, ctypes.byref(need)) == 2
    geom = (ctypes.c_double * 10)(*([0.0] * 9 + [0.25]))
    assert L.cobevt_bev_points(None, None, None, None, dims, geom, None) == 1
    assert L.cobevt_bev_points(None, None, None, None, None, None, None) == 1
    params = (ctypes.c_double * 16)(*([-12.0, -10.0, 0.25, 4.0] + list(cb.TARGET_MEAN) + list(cb.TARGET_STD_DEV)))
    ldims = (ctypes.c_int * 4)(1, 4, 24, 20)
    assert L.cobevt_bev_labels(None, None, None, None, None, ldims, params, None) == 1
    assert L.cobevt_bev_labels(None, None, None, None, None, None, None, None) == 1
    assert L.cobevt_bev_post(None, None, None, None, 1, params, 0.5, 0.15, None, None, None, None, None, None) == 1
    assert L.cobevt_bev_post(None, None, None, None, 1, None, 0.5, 0.15, None, None, None, None, None, None) == 1


def test_the_workspace_size_follows_its_key():
    """bev_points' default workspace is cached on (N, nx, ny): the point count and the channels, which the key leaves out, must not
    move the size (a key with M in it would grow one buffer per distinct cloud)"""
    assert ops.bev_points_workspace_ints(10, 2, (16, 12, 5)) == ops.bev_points_workspace_ints(99999, 2, (16, 12, 9)) == 3 * 2 * 16 * 12
