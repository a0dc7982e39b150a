"""ops.resize_pil_bilinear / ops.decode_bev / host.nuscenes.LoadDataTransform without a device: the fixture gv_nusc_ingest.npz (the
reference's own LoadDataTransform with the real Pillow, written by tests/golden/make_golden_nusc_ingest.py) is reproduced by the
restatement tests/ingest_ref.py, the restatement equals the installed Pillow byte for byte on the shape list, ops.pil_resize_taps makes
the restatement's tables, the host layer refuses bad arguments before any launch, and one __call__ is one resize and one decode launch.

No tolerance anywhere: the arithmetic is integer plus a table lookup, every comparison is exact."""
import numpy as np
import pytest
import torch

import ingest_ref as ir
import launch_trace as lt
import launch_trace_nusc_ingest as lti
from cobevt_amd import ops
from cobevt_amd.host import nuscenes as nu
from cobevt_amd.lib import CobevtHipError
from util import golden


@pytest.fixture(scope="module")
def gv():
    return golden("gv_nusc_ingest")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_reproduces_the_fixture(gv, name):
    h, w, top = (int(v) for v in gv["image_config"])
    image = ir.resize(gv[name + "_images"], (w, h + top), top)
    assert image.dtype == np.float32 and np.array_equal(bits(image), bits(gv[name + "_out_image"]))
    bev = ir.decode_bev(gv[name + "_bev"], int(gv["num_classes"]))
    assert np.array_equal(bits(bev), bits(gv[name + "_out_bev"]))
    assert set(np.unique(bev)) == {0.0, 1.0}
    if name == "a":
        assert np.array_equal(bits(gv["a_out_center"]), bits(gv["a_aux"][..., 1][None]))
        assert np.array_equal(gv["a_out_visibility"], gv["a_visibility"])


@pytest.mark.parametrize("shape", ir.SHAPES, ids=ir.shape_id)
def test_restatement_equals_pillow(shape):
    Image = pytest.importorskip("PIL.Image")
    (hs, ws), (hr, wr), top, n = shape
    img, ref = ir.case(shape)
    assert ref.shape == (n, hr - top, wr, 3)
    for i in range(n):
        p = Image.fromarray(img[i]).resize((wr, hr), resample=Image.BILINEAR)
        p = p.crop((0, top, p.width, p.height))
        assert np.array_equal(np.asarray(p), ref[i])


def test_the_cases_reach_the_edges():
    """what the inputs are for: saturated blocks in the top third, and pixels where a wider horizontal intermediate would round
    differently (so a kernel that keeps one is caught)"""
    shape = ir.SHAPES[5]
    (hs, ws), (hr, wr), top, n = shape
    img, ref = ir.case(shape)
    assert set(np.unique(img[:, :hs // 3])) == {0, 255} and (ref == 0).any() and (ref == 255).any()
    hb, hc = ir.taps(ws, wr)
    vb, vc = ir.taps(hs, hr)
    wide = np.zeros((n, hs, wr, 3), dtype=np.int64)                     # the horizontal pass WITHOUT the rounding to a byte
    for x, (first, count) in enumerate(hb):
        for t in range(count):
            wide[:, :, x] += img[:, :, first + t].astype(np.int64) * int(hc[x, t])
    fused = np.zeros((n, hr, wr, 3), dtype=np.float64)
    for y, (first, count) in enumerate(vb):
        for t in range(count):
            fused[:, y] += wide[:, first + t] * (float(vc[y, t]) / (1 << 44))
    fused = np.clip(np.floor(fused + 0.5), 0, 255).astype(np.uint8)[:, top:]
    assert 0 < int((fused != ref).sum()) and int(np.abs(fused.astype(int) - ref).max()) == 1


def test_byte_table_is_to_tensor():
    t = torch.arange(256, dtype=torch.float32).div(255)
    assert np.array_equal(bits(t.numpy()), bits(ir.byte_table()))
    assert np.array_equal(bits(t.numpy()), bits(torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).numpy()))


# ---------------------------------------------------------------------------------------------- the tap tables
@pytest.mark.parametrize("shape", ir.SHAPES, ids=ir.shape_id)
def test_taps_equal_the_restatement(shape):
    (hs, ws), (hr, wr), _, _ = shape
    for n_in, n_out in ((hs, hr), (ws, wr)):
        b, c = ops.pil_resize_taps(n_in, n_out)
        rb, rc = ir.taps(n_in, n_out)
        assert b.dtype == np.int32 and c.dtype == np.int32 and b.shape == (n_out, 2) and c.shape == (n_out, ops.pil_ksize(n_in, n_out))
        assert np.array_equal(b, rb) and np.array_equal(c, rc)
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] >= 1).all()
        assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all()       # the kernel's band windows rely on it
        assert 255 * int(c.sum(axis=1).max()) + (1 << 21) < 2 ** 31


def test_taps_rules():
    assert ops.pil_ksize(1600, 480) == 9 and ops.pil_ksize(900, 270) == 9 and ops.pil_ksize(20, 33) == 3
    assert ops.pil_ksize(800, 100) == 17 and ops.pil_ksize(801, 100) == 19
    b, c = ops.pil_resize_taps(16, 16)               # an axis that keeps its size: the identity, exactly (and the kernel skips it)
    assert np.array_equal(b[:, 0], np.arange(16)) and np.array_equal(c[:, 0], np.full(16, 1 << 22)) and not c[:, 1:].any()
    assert ops.pil_resize_taps(16, 16)[0] is b and not b.flags.writeable
    with pytest.raises(CobevtHipError, match="positive"):
        ops.pil_resize_taps(0, 4)


# ---------------------------------------------------------------------------------------------- argument checks
def test_cpu_tensors_are_refused():
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        ops.resize_pil_bilinear(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4))
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        ops.decode_bev(torch.zeros(1, 4, 4, dtype=torch.int32), 12)
    gv = golden("gv_nusc_ingest")
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        lti.transform(gv, "cpu")(lti.sample(gv, "b"))


def test_argument_checks(monkeypatch):
    """every check in front of the two launches, with the device guard off (tests/launch_trace.py) on CPU tensors: nothing is launched"""
    rec = lt.Recorder()
    lt.install(monkeypatch.setattr, rec)
    img = torch.zeros(2, 16, 24, 3, dtype=torch.uint8)
    f = ops.resize_pil_bilinear
    for bad in (img.float(), img[0], torch.zeros(2, 16, 24, 6, dtype=torch.uint8)[..., :3], img.permute(0, 2, 1, 3)):
        with pytest.raises(CobevtHipError, match="images_u8 must be contiguous uint8"):
            f(bad, (12, 8))
    with pytest.raises(CobevtHipError, match="3 channels"):
        f(torch.zeros(2, 16, 24, 4, dtype=torch.uint8), (12, 8))
    with pytest.raises(CobevtHipError, match="images_u8 must not be empty"):
        f(torch.zeros(0, 16, 24, 3, dtype=torch.uint8), (12, 8))
    for bad in (12, (12,), (12, 8, 3), "ab"):
        with pytest.raises(CobevtHipError, match="size = "):
            f(img, bad)
    for bad in ((0, 8), (12, -1)):
        with pytest.raises(CobevtHipError, match="size = .* must be positive"):
            f(img, bad)
    for bad in (-1, 8, 9):
        with pytest.raises(CobevtHipError, match="top_crop must lie in"):
            f(img, (12, 8), bad)
    for bad in ((2, 8), (12, 1)):                            # 24 -> 2 is a down-scale of 12, 16 -> 1 of 16
        with pytest.raises(CobevtHipError, match="down-scale above 8"):
            f(img, bad)
    with pytest.raises(CobevtHipError, match="dtype must be"):
        f(img, (12, 8), dtype=torch.float16)
    for bad, dt in ((torch.zeros(2, 3, 8, 12), torch.uint8), (torch.zeros(2, 6, 12, 3, dtype=torch.uint8), torch.uint8),
                    (torch.zeros(2, 3, 6, 12), torch.float32)):
        with pytest.raises(CobevtHipError, match="out= must be"):
            f(img, (12, 8), dtype=dt, out=bad)
    lab = torch.zeros(1, 5, 7, dtype=torch.int32)
    for bad in (lab.long(), lab[0], torch.zeros(1, 5, 14, dtype=torch.int32)[..., ::2]):
        with pytest.raises(CobevtHipError, match="labels_i32 must be contiguous int32"):
            ops.decode_bev(bad, 12)
    with pytest.raises(CobevtHipError, match="must not be empty"):
        ops.decode_bev(torch.zeros(1, 0, 7, dtype=torch.int32), 12)
    for bad in (0, 17):
        with pytest.raises(CobevtHipError, match="num_classes must lie in"):
            ops.decode_bev(lab, bad)
    with pytest.raises(CobevtHipError, match="out= must be"):
        ops.decode_bev(lab, 12, out=torch.zeros(1, 11, 5, 7))
    assert rec.records == []
    # and the calls that are fine do launch: both outputs, a skipped axis, a scale of exactly 8
    assert tuple(f(img, (12, 8), 2).shape) == (2, 3, 6, 12)
    assert tuple(f(img, (24, 8), dtype=torch.uint8).shape) == (2, 8, 24, 3)
    assert tuple(f(img, (3, 2)).shape) == (2, 3, 2, 3)
    assert tuple(ops.decode_bev(lab, 16).shape) == (1, 16, 5, 7)
    assert [r[1] for r in rec.records] == ["cobevt_resize_pil_u8"] * 3 + ["cobevt_decode_bev"]
    assert rec.records[0][2][-1] == [2, 16, 24, 3, 8, 12, 2, 0] and rec.records[1][2][-1] == [2, 16, 24, 3, 8, 24, 0, 1]
    assert rec.records[1][2][2:4] == ["null", "null"] and rec.records[1][2][4:6] == ["ptr", "ptr"]      # W kept: no horizontal tables


def test_transform_argument_checks(monkeypatch, gv):
    rec = lt.Recorder()
    lt.install(monkeypatch.setattr, rec)
    for name in ("strong", "geometric"):
        with pytest.raises(CobevtHipError, match=name):
            nu.LoadDataTransform({"h": 11, "w": 24, "top_crop": 3}, 12, augment=name)
    t = lti.transform(gv, "cpu")
    s = lti.sample(gv, "a")
    s.images = s.images[:5] + [torch.zeros(30, 40, 3, dtype=torch.uint8)]
    with pytest.raises(CobevtHipError, match="one size"):
        t(s)
    s = lti.sample(gv, "a")
    s.images = [im.float() for im in s.images]
    with pytest.raises(CobevtHipError, match="uint8 frames"):
        t(s)
    s = lti.sample(gv, "a")
    s.bev = s.bev.long()
    with pytest.raises(CobevtHipError, match="bit-packed"):
        t.get_bev(s)
    assert rec.records == []


# ---------------------------------------------------------------------------------------------- LoadDataTransform on the host
def test_launch_trace(monkeypatch):
    records = lti.trace("load_data_transform", monkeypatch.setattr)
    assert records == lti.read_fixture("load_data_transform")
    assert [r[1] for r in records] == ["cobevt_resize_pil_u8", "cobevt_decode_bev"]         # six cameras, one launch
    assert records[0][2][-1] == [6, 45, 80, 3, 14, 24, 3, 0] and records[1][2][2:] == [1, 400, 12]


@pytest.mark.parametrize("name,as_list", [("a", True), ("a", False), ("b", True)])
def test_returned_dict(monkeypatch, gv, name, as_list):
    """keys, dtypes and shapes are the reference's; what is computed on the host (intrinsics, extrinsics, view, cam_idx, visibility,
    center, pose) is bit-equal to it.  (image and bev come from the device: tests/test_nusc_ingest_gpu.py.)"""
    lt.install(monkeypatch.setattr, lt.Recorder())
    out = lti.transform(gv, "cpu")(lti.sample(gv, name, as_list))
    want = {k[len(name) + 5:]: gv[k] for k in gv.files if k.startswith(name + "_out_")}
    assert list(out) == [k for k in ("cam_idx", "image", "intrinsics", "extrinsics", "bev", "view", "visibility", "center", "pose") if k in want]
    assert ("visibility" in out) == (name == "a")
    for k, ref in want.items():
        got = out[k]
        assert isinstance(got, np.ndarray) == (k in ("visibility", "pose")), k          # the reference returns these two as arrays
        got = got if isinstance(got, np.ndarray) else got.numpy()
        assert got.dtype == ref.dtype and got.shape == ref.shape, k
        if k not in ("image", "bev"):
            assert np.array_equal(bits(got), bits(ref)), k
