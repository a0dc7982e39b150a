"""The LiDAR BEV (PIXOR) pre- and post-processor on the GPU: csrc/bev_points.hip, csrc/bev_labels.hip and the bev mode of
csrc/detect_post.hip through ops.bev_points / bev_labels / bev_post_process, host.BevPreprocessor and host.LidarBevPostprocessor, against the reference's own run
(tests/golden/gv28_lidar_bev.npz, the cases of tests/golden/cases_bev.py) and the float64 restatement tests/bev_ref.py.

Gates.  Occupancy, the class channel, bev_corners, num_valid, the picked pixel indices and the count are compared EXACTLY: the cases
keep every decision off a rounding edge or on an exact hit (asserted on the CPU by tests/test_lidar_bev.py and by the generator).
  intensity   against the float64 mean: the kernel's stated bound 2^-33 + 2^-24 |mean| (1 + 2^-20) (csrc/bev_points.hip); against the
              fixture: that bound plus the reference's own stored deviation from the float64 mean (its fp32 running sum).
  label map   regression channels within 1 fp32 ulp of the float64 restatement (fp64 arithmetic, one cast; the device's fp64 cos /
              sin / log differ from the host's by parts of an fp64 ulp); against the fixture: 1 ulp plus the stored deviation.
  boxes       gv24's rule: 4 x the deviation the generator measured between the reference's fp32 result and the float64 restatement
              with a floor of 4 ulp of the case's largest coordinate (scores: 4 * 2^-24) - the reference and the kernel both sit
              within one such deviation of the float64 value, the factor covers exp / atan2 / sigmoid differing by a few ulp.
No element is excluded from any comparison.  Every test prints its worst |err| / gate."""
import functools

import numpy as np
import pytest
import torch

import bev_ref as br
import cases_bev as cb
from cobevt_amd import host, ops, registry
from util import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gv():
    return golden("gv28_lidar_bev")


@functools.lru_cache(maxsize=None)
def _clouds(designed):
    return cb.points_boundary() if designed else cb.points_main()


@functools.lru_cache(maxsize=None)
def _pre_ref(designed, rm, em):
    return br.bev_points(_clouds(designed), cb.GEOM, cb.LIDAR_RANGE, rm, em)


# ---------------------------------------------------------------------------------------------- preprocessor
@pytest.mark.parametrize("name,designed,rm,em", [("pre_main", False, False, False), ("pre_main_masks", False, True, True),
                                                 ("pre_boundary_r0_e0", True, False, False), ("pre_boundary_r0_e1", True, False, True),
                                                 ("pre_boundary_r1_e0", True, True, False), ("pre_boundary_r1_e1", True, True, True)])
def test_preprocessor(cuda, gv, name, designed, rm, em):
    clouds = _clouds(designed)
    pts, offs = cb.concat(clouds)
    pre = registry.build_preprocessor(cb.pre_params(rm, em), train=False)
    assert type(pre) is host.BevPreprocessor
    d_pts, d_offs = torch.from_numpy(pts).to(cuda), torch.from_numpy(offs).to(cuda)
    got = pre.preprocess_batch(d_pts, d_offs)["bev_input"]
    assert tuple(got.shape) == (2, 9, 96, 80) and got.dtype == torch.float32
    g = got.cpu().numpy()
    ref, mean = gv[name + "_bev"], _pre_ref(designed, rm, em)
    assert np.array_equal(g[:, :-1], ref[:, :-1]), "occupancy"
    bound = br.intensity_bound(mean[:, -1])
    err = np.abs(g[:, -1].astype(np.float64) - mean[:, -1])
    err_ref = np.abs(g[:, -1].astype(np.float64) - ref[:, -1].astype(np.float64))
    dev = float(gv[name + "_dev"])
    print("%s: intensity worst |err| / bound %.3f against the float64 mean, %.3f against the fixture (stored deviation %.3e)"
          % (name, float((err / bound).max()), float((err_ref / (bound + dev)).max()), dev))
    assert bool((err <= bound).all()) and bool((err_ref <= bound + dev).all())
    assert bool(((g[:, -1] != 0) <= (mean[:, -1] != 0)).all())            # a cell without points holds 0
    # bitwise identical under a permutation of the points within each agent, from run to run, and into garbage-filled buffers
    perm = np.concatenate([offs[a] + cb.permutation("gpu.%s.%d" % (name, a), len(c)) for a, c in enumerate(clouds)])
    shuffled = torch.from_numpy(np.ascontiguousarray(pts[perm])).to(cuda)
    out = torch.full((2, 9, 96, 80), 7.5, device=cuda)
    ws = torch.full((ops.bev_points_workspace_ints(len(pts), 2, (96, 80, 9)) + 16,), -1, device=cuda, dtype=torch.int32)
    again = ops.bev_points(shuffled, d_offs, cb.LIDAR_RANGE, pre.origin, pre.res, pre.input_shape, rm, em, out=out, workspace=ws[:-16])
    assert again.data_ptr() == out.data_ptr() and torch.equal(again, got) and bool((ws[-16:] == -1).all())
    assert torch.equal(pre.preprocess_batch(d_pts, d_offs)["bev_input"], got)
    # both layouts agree
    last = pre.preprocess_batch(d_pts, d_offs, channels_last=True)["bev_input"]
    assert tuple(last.shape) == (2, 96, 80, 9) and torch.equal(last.permute(0, 3, 1, 2), got)


def test_preprocessor_single_and_collate(cuda, gv):
    pre = host.BevPreprocessor(cb.pre_params(), train=False)
    clouds = _clouds(False)
    singles = [pre.preprocess(torch.from_numpy(c).to(cuda)) for c in clouds]
    assert tuple(singles[0]["bev_input"].shape) == (9, 96, 80)
    ref = torch.from_numpy(gv["pre_main_bev"])
    for batch in (singles, {"bev_input": [s["bev_input"] for s in singles]}):
        got = pre.collate_batch(batch)["bev_input"].cpu()
        assert torch.equal(got[:, :-1], ref[:, :-1])
    # int64 offsets, and rows past offsets[N] are ignored
    pts, offs = cb.concat(clouds)
    padded = torch.from_numpy(np.concatenate([pts, pts[:100]])).to(cuda)
    a = pre.preprocess_batch(padded, torch.from_numpy(offs.astype(np.int64)).to(cuda))["bev_input"]
    assert torch.equal(a, torch.stack([s["bev_input"] for s in singles]))


# ---------------------------------------------------------------------------------------------- labels
def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("name,axis", [("label_main", False), ("label_axis", True)])
def test_labels(cuda, gv, name, axis):
    gt, mask = cb.labels_axis() if axis else cb.labels_main()
    post = registry.build_postprocessor(cb.post_params(), train=True)
    assert type(post) is host.LidarBevPostprocessor
    out = post.generate_label_batch(torch.from_numpy(gt).to(cuda), torch.from_numpy(mask).to(cuda))
    label, corners, num_valid = out["label_map"].cpu().numpy(), out["bev_corners"].cpu().numpy(), out["num_valid"].cpu().numpy()
    assert label.shape == (gt.shape[0], 7, 24, 20) and label.dtype == np.float32 and num_valid.dtype == np.int32
    ref = gv[name + "_label_map"]
    assert np.array_equal(label[:, 0], ref[:, 0]), "class channel"
    assert np.array_equal(corners, gv[name + "_corners"]), "bev_corners"
    assert np.array_equal(num_valid, gv[name + "_num_valid"])
    mine = np.stack([br.generate_label(gt[b], mask[b], cb.GEOM, cb.TARGET_MEAN, cb.TARGET_STD_DEV)["label_map"] for b in range(len(gt))])
    ulp = _ulp32(mine[:, 1:])
    err = np.abs(label[:, 1:].astype(np.float64) - mine[:, 1:])
    err_ref = np.abs(label[:, 1:].astype(np.float64) - ref[:, 1:].astype(np.float64))
    dev = float(gv[name + "_dev"])
    print("%s: regression channels worst |err| %.3f ulp against the float64 restatement; %.3f of (1 ulp + stored deviation %.3e) "
          "against the fixture" % (name, float((err / ulp).max()), float((err_ref / (ulp + dev)).max()), dev))
    assert bool((err <= ulp).all()) and bool((err_ref <= ulp + dev).all())
    # the reference's per-sample signature: numpy in, numpy out
    one = post.generate_label(gt_box_center=gt[0], mask=mask[0])
    n = int(num_valid[0])
    assert np.array_equal(one["label_map"], label[0]) and np.array_equal(one["bev_corners"], corners[0, :n])
    coll = post.collate_batch([one, one])
    assert tuple(coll["label_map"].shape) == (2, 7, 24, 20) and len(coll["bev_corners"]) == 2


def test_labels_degenerate_box_and_out(cuda):
    """a box with an edge of squared norm <= 1e-6 marks no pixel (the reference asserts there); out= is written in place"""
    post = host.LidarBevPostprocessor(cb.post_params(), train=True)
    gt, mask = cb.labels_axis()
    gt = gt.copy()
    gt[0, 1, 3] = 1e-4                                           # 1e-4 m = 1e-4 label pixels: squared norm 1e-8
    outs = [torch.full((1, 7, 24, 20), 7.5, device=cuda), torch.full((1, cb.MAX_NUM, 4, 2), 7.5, device=cuda),
            torch.full((1,), 77, device=cuda, dtype=torch.int32)]
    out = post.generate_label_batch(torch.from_numpy(gt).to(cuda), torch.from_numpy(mask).to(cuda), out=outs)
    assert out["label_map"].data_ptr() == outs[0].data_ptr() and int(out["num_valid"][0]) == 2
    only_first = br.generate_label(gt[0], np.eye(cb.MAX_NUM)[0], cb.GEOM, cb.TARGET_MEAN, cb.TARGET_STD_DEV)["label_map"]
    assert np.array_equal(out["label_map"][0, 0].cpu().numpy(), only_first[0])
    assert bool(out["bev_corners"][0, 1].any()) and not bool(out["bev_corners"][0, 2:].any())


def test_normalize_roundtrip(cuda):
    post = host.LidarBevPostprocessor(cb.post_params(), train=True)
    x = torch.from_numpy(cb.uniform("gpu.norm", (24, 20, 7))).to(cuda)
    n = post.normalize_targets(x)
    assert torch.equal(n[..., 0], x[..., 0])
    back = post.denormalize_reg_map(n[..., 1:])
    assert float((back - x[..., 1:]).abs().max()) <= 1e-14


# ---------------------------------------------------------------------------------------------- post_process
def _gates(gv, name):
    dev_box, dev_score = [float(v) for v in gv[name + "_dev"]]
    floor = float(np.spacing(np.float32(abs(float(gv[name + "_maxcoord"])))))
    return max(4 * dev_box, 4 * floor), max(4 * dev_score, 4 * 2.0 ** -24)


def _dicts(cavs, dev, device_side=False):
    data, output = {}, {}
    for c, (cls, reg, m) in enumerate(cavs):
        m = torch.from_numpy(m)
        data["cav%d" % c] = {"transformation_matrix": m.to(dev) if device_side else m}
        output["cav%d" % c] = {"cls": torch.from_numpy(cls).to(dev), "reg": torch.from_numpy(reg).to(dev)}
    return data, output


def _check(got, gv, name):
    boxes, scores, index, count = [g.cpu() for g in got]
    k = int(count[0])
    ref_index = gv[name + "_index"]
    assert k == len(ref_index), "%s: %d boxes, the reference has %d" % (name, k, len(ref_index))
    assert np.array_equal(index[:k].numpy(), ref_index), name
    assert tuple(boxes.shape) == (1000, 4, 2) and tuple(scores.shape) == (1000,) and index.dtype == torch.int32
    assert not bool(boxes[k:].any()) and not bool(scores[k:].any()) and not bool(index[k:].any())
    if k:
        box_gate, score_gate = _gates(gv, name)
        d_box = float((boxes[:k].double() - torch.from_numpy(gv[name + "_boxes"]).double()).abs().max())
        d_score = float((scores[:k].double() - torch.from_numpy(gv[name + "_scores"]).double()).abs().max())
        print("%s: corners max |diff| %.3e (gate %.3e)  scores %.3e (gate %.3e)" % (name, d_box, box_gate, d_score, score_gate))
        assert d_box <= box_gate and d_score <= score_gate, (name, d_box, box_gate, d_score, score_gate)
    return k


@pytest.mark.parametrize("name,case,geom", [("post_two", "post_two_cavs", "GEOM"), ("post_cut", "post_cut", "GEOM_CUT")])
def test_post_process(cuda, gv, name, case, geom):
    cavs = getattr(cb, case)()
    post = host.LidarBevPostprocessor(cb.post_params(getattr(cb, geom)), train=False)
    data, output = _dicts(cavs, cuda)
    boxes, scores = post.post_process(data, output)
    got = post.post_process_device(data, output)
    torch.cuda.synchronize()
    k = _check(got, gv, name)
    assert k > 0 and tuple(boxes.shape) == (k, 4, 2) and torch.equal(boxes, got[0][:k]) and torch.equal(scores, got[1][:k])


def test_post_process_empty_cases(cuda, gv):
    """(None, None) when nothing passes the threshold; empty tensors when candidates exist and none is inside GT_RANGE"""
    post = host.LidarBevPostprocessor(cb.post_params(), train=False)
    data, output = _dicts(cb.post_nothing(), cuda)
    assert bool(gv["post_none_none"]) and post.post_process(data, output) == (None, None)
    dev_out = post.post_process_device(data, output)
    assert int(dev_out[3][0]) == 0 and not bool(dev_out[0].any())
    data, output = _dicts(cb.post_out_of_range(), cuda)
    assert not bool(gv["post_range_none"]) and len(gv["post_range_index"]) == 0
    boxes, scores = post.post_process(data, output)
    assert tuple(boxes.shape) == (0, 4, 2) and tuple(scores.shape) == (0,)
    assert _check(post.post_process_device(data, output), gv, "post_range") == 0


def test_post_process_graph(cuda, gv):
    """two eager runs are bit-identical; a graph replay into garbage-filled outputs and workspace equals the eager result"""
    post = host.LidarBevPostprocessor(cb.post_params(), train=False)
    cavs = cb.post_two_cavs()
    data, output = _dicts(cavs, cuda, device_side=True)
    first = [t.clone() for t in post.post_process_device(data, output)]
    outs = [torch.full((1000, 4, 2), 7.5, device=cuda), torch.full((1000,), -3.0, device=cuda),
            torch.full((1000,), 77, device=cuda, dtype=torch.int32), torch.full((1,), 77, device=cuda, dtype=torch.int32)]
    total = sum(c[0].size for c in cavs)
    ws = torch.full(((ops.detect_workspace_bytes(total) + 7) // 8 + 64,), -1, device=cuda, dtype=torch.int64)
    second = post.post_process_device(data, output, out=outs, workspace=ws[:-64])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and bool((ws[-64:] == -1).all())
    k = _check(second, gv, "post_two")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        post.post_process_device(data, output, out=outs, workspace=ws[:-64])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        post.post_process_device(data, output, out=outs, workspace=ws[:-64])
    outs[0].fill_(9.25)
    outs[1].fill_(5.0)
    outs[2].fill_(-5)
    outs[3].fill_(-5)
    ws[:-64].fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, outs))
    assert int(outs[3][0]) == k                                 # the count is read only now
    del graph
    torch.cuda.synchronize()


def test_reg_map_to_bbx_corners(cuda):
    """the corners of masked pixels, in pixel order, equal the restatement's decode with an identity matrix"""
    post = host.LidarBevPostprocessor(cb.post_params(), train=False)
    cls, reg, _ = cb.post_two_cavs()[0]
    d_reg = torch.from_numpy(reg).to(cuda)[0].permute(1, 2, 0)
    mask = torch.from_numpy(cls[0, 0] > 0).to(cuda)
    got = post.reg_map_to_bbx_corners(post.denormalize_reg_map(d_reg.double()), mask).cpu().numpy()
    _, ref = br.decode(cls, reg, np.eye(4, dtype=np.float32), cb.GEOM, cb.TARGET_MEAN, cb.TARGET_STD_DEV, faithful=False)
    ref = ref[(cls[0, 0] > 0).reshape(-1)]
    gate = 16 * float(np.spacing(np.float32(np.abs(ref).max())))       # reg is de-normalised and rounded to fp32 once more on the way
    d = float(np.abs(got - ref).max())
    print("reg_map_to_bbx_corners: %d boxes, max |diff| %.3e (gate %.3e)" % (len(ref), d, gate))
    assert got.shape == ref.shape and len(ref) == 70 and d <= gate


# ---------------------------------------------------------------------------------------------- end to end
def test_end_to_end(cuda):
    """build_preprocessor -> bev_input, build_postprocessor -> labels; the label map fed back as the network's output (logit +10 on
    positives, -10 elsewhere) recovers every ground-truth box with IoU > 0.9"""
    pre = registry.build_preprocessor(cb.pre_params(), train=False)
    post = registry.build_postprocessor(cb.post_params(), train=False)
    pts, offs = cb.concat(_clouds(False))
    bev = pre.preprocess_batch(torch.from_numpy(pts).to(cuda), torch.from_numpy(offs).to(cuda))["bev_input"]
    assert tuple(bev.shape) == (2, 9, 96, 80) and float(bev[:, :-1].sum()) > 0
    gt, mask = cb.labels_e2e()
    labels = post.generate_label_batch(torch.from_numpy(gt).to(cuda), torch.from_numpy(mask).to(cuda))
    label_map, n = labels["label_map"], int(labels["num_valid"][0])
    assert n == 4
    cls = (label_map[:, :1] * 20.0 - 10.0).contiguous()
    reg = label_map[:, 1:].contiguous()
    data = {"ego": {"transformation_matrix": torch.eye(4)}}
    boxes, scores = post.post_process(data, {"ego": {"cls": cls, "reg": reg}})
    assert boxes.shape[0] == n
    iou = ops.rotated_iou(labels["bev_corners"][0, :n], boxes).cpu().numpy()
    print("end to end: best IoU per ground-truth box %s" % np.round(iou.max(axis=1), 4).tolist())
    assert bool((iou.max(axis=1) > 0.9).all()) and sorted(iou.argmax(axis=1).tolist()) == list(range(n))
