"""ops.resize_pil_bilinear / ops.decode_bev / host.nuscenes.LoadDataTransform on the device against the restatement tests/ingest_ref.py
(which tests/test_nusc_ingest.py pins to Pillow and to the reference's own run): byte equality for the uint8 output, bit equality for
the fp32 output, on the shape list; the golden sample through LoadDataTransform end to end; out= reuse; six frames in one launch; an
image stack at an odd byte offset; the C entry's refusals; one capture and replay in torch.cuda.graph.

No tolerance anywhere: the arithmetic is integer plus a table lookup, every comparison is exact.  (Neither Pillow nor the reference
is needed here.)"""
import ctypes

import numpy as np
import pytest
import torch

import ingest_ref as ir
import launch_trace_nusc_ingest as lti
from cobevt_amd import lib, ops
from cobevt_amd.lib import CobevtHipError
from util import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("shape", ir.SHAPES, ids=ir.shape_id)
def test_resize_equals_the_restatement(dev, shape):
    (hs, ws), (hr, wr), top, n = shape
    img, ref = ir.case(shape)
    x = torch.from_numpy(img.copy()).to(dev)
    got8 = ops.resize_pil_bilinear(x, (wr, hr), top, dtype=torch.uint8)
    got32 = ops.resize_pil_bilinear(x, (wr, hr), top)
    assert got8.dtype == torch.uint8 and tuple(got8.shape) == (n, hr - top, wr, 3)
    assert got32.dtype == torch.float32 and tuple(got32.shape) == (n, 3, hr - top, wr)
    got8, got32 = got8.cpu().numpy(), got32.cpu().numpy()
    print("%s: %d of %d bytes differ, %d of %d floats differ" % (ir.shape_id(shape), int((got8 != ref).sum()), ref.size,
                                                                 int((bits(got32) != bits(ir.to_tensor(ref))).sum()), ref.size))
    assert np.array_equal(got8, ref)
    assert np.array_equal(bits(got32), bits(ir.to_tensor(ref)))


def test_six_frames_in_one_launch_equal_six_launches(dev):
    shape = ir.SHAPES[5]
    (hs, ws), (hr, wr), top, n = shape
    assert n == 6
    img, ref = ir.case(shape)
    x = torch.from_numpy(img.copy()).to(dev)
    with ops.LaunchProfile() as prof:
        all6 = ops.resize_pil_bilinear(x, (wr, hr), top)
    assert len(prof.records) == 1
    one = torch.cat([ops.resize_pil_bilinear(x[i:i + 1], (wr, hr), top) for i in range(6)])
    assert torch.equal(all6, one) and np.array_equal(bits(all6.cpu().numpy()), bits(ir.to_tensor(ref)))


def test_unaligned_stack(dev):
    """frames that start at an odd byte offset of their buffer: a row start has no alignment the kernel could rely on"""
    shape = ir.SHAPES[0]
    (hs, ws), (hr, wr), top, n = shape
    img, ref = ir.case(shape)
    for off in (1, 7, 13):
        buf = torch.zeros(off + img.size, dtype=torch.uint8, device=dev)
        buf[off:] = torch.from_numpy(img.copy()).to(dev).flatten()
        x = buf[off:].view(n, hs, ws, 3)
        assert x.data_ptr() % 16 == off and x.is_contiguous()
        assert np.array_equal(ops.resize_pil_bilinear(x, (wr, hr), top, dtype=torch.uint8).cpu().numpy(), ref)


def test_out_reuse(dev):
    shape = ir.SHAPES[6]
    (hs, ws), (hr, wr), top, n = shape
    img, ref = ir.case(shape)
    x = torch.from_numpy(img.copy()).to(dev)
    out8 = torch.full((n, hr - top, wr, 3), 77, dtype=torch.uint8, device=dev)
    out32 = torch.full((n, 3, hr - top, wr), -5.0, device=dev)
    assert ops.resize_pil_bilinear(x, (wr, hr), top, dtype=torch.uint8, out=out8) is out8
    assert ops.resize_pil_bilinear(x, (wr, hr), top, out=out32) is out32
    assert np.array_equal(out8.cpu().numpy(), ref) and np.array_equal(bits(out32.cpu().numpy()), bits(ir.to_tensor(ref)))
    x2 = torch.flip(x, dims=[0]).contiguous()                      # the same buffers again, other frames: every element is rewritten
    ops.resize_pil_bilinear(x2, (wr, hr), top, dtype=torch.uint8, out=out8)
    ops.resize_pil_bilinear(x2, (wr, hr), top, out=out32)
    assert np.array_equal(out8.cpu().numpy(), ref[::-1]) and np.array_equal(bits(out32.cpu().numpy()), bits(ir.to_tensor(ref[::-1])))
    with pytest.raises(CobevtHipError, match="out= must be"):
        ops.resize_pil_bilinear(x, (wr, hr), top, out=out8)


def test_decode_bev(dev):
    rng = np.random.RandomState(3)
    for n, h, w, c in ((1, 20, 20, 12), (3, 7, 37, 16), (2, 200, 200, 1)):
        lab = rng.randint(0, 1 << 16, size=(n, h, w)).astype(np.int32)
        lab[0, 0, 0] = -1                                         # every bit set, the sign bit too
        ref = np.stack([ir.decode_bev(lab[i], c) for i in range(n)])
        x = torch.from_numpy(lab).to(dev)
        out = torch.full((n, c, h, w), 9.0, device=dev)
        assert ops.decode_bev(x, c, out=out) is out
        assert np.array_equal(bits(out.cpu().numpy()), bits(ref))
        assert np.array_equal(bits(ops.decode_bev(x, c).cpu().numpy()), bits(ref))


def test_c_entry_refuses_before_launch(dev):
    """status 2 from the C entry itself (the host layer refuses the same cases earlier, with the argument's name)"""
    x = torch.zeros(1, 100, 100, 3, dtype=torch.uint8, device=dev)
    out = torch.zeros(1, 50, 50, 3, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    for dims in ([1, 100, 100, 3, 12, 50, 0, 1], [1, 100, 100, 3, 50, 12, 0, 1],         # a down-scale above 8, either axis
                 [1, 100, 100, 4, 50, 50, 0, 1], [1, 100, 100, 1, 50, 50, 0, 1],         # channels
                 [0, 100, 100, 3, 50, 50, 0, 1], [1, 100, 100, 3, 0, 50, 0, 1], [1, 100, 100, 3, 50, 0, 0, 1],   # empty
                 [1, 100, 100, 3, 50, 50, 50, 1], [1, 100, 100, 3, 50, 50, -1, 1]):      # top_crop outside [0, h_resize)
        with pytest.raises(CobevtHipError, match="code 2"):
            lib.call("cobevt_resize_pil_u8", p(x), p(out), None, None, None, None, None, (ctypes.c_int * 8)(*dims), None)
    lab = torch.zeros(1, 4, 4, dtype=torch.int32, device=dev)
    for c in (0, 17):
        with pytest.raises(CobevtHipError, match="code 2"):
            lib.call("cobevt_decode_bev", p(lab), p(out), 1, 16, c, None)
    torch.cuda.synchronize()
    assert not out.any()


@pytest.mark.parametrize("name", ["a", "b"])
def test_golden_through_load_data_transform(dev, name):
    gv = golden("gv_nusc_ingest")
    t = lti.transform(gv, None)
    results = [t(lti.sample(gv, name, True))]
    s = lti.sample(gv, name, False)
    s.images = s.images.to(dev)                                   # a stack already on the device
    s.bev = s.bev.to(dev)
    results.append(t(s))
    want = {k[len(name) + 5:]: gv[k] for k in gv.files if k.startswith(name + "_out_")}
    for out in results:
        assert sorted(out) == sorted(want)
        assert out["image"].device == dev and out["bev"].device == dev
        for k, ref in want.items():
            got = out[k] if isinstance(out[k], np.ndarray) else out[k].cpu().numpy()
            assert got.dtype == ref.dtype and got.shape == ref.shape, k
            assert np.array_equal(bits(got), bits(ref)), k


def test_graph_capture_and_replay(dev):
    shape = ir.SHAPES[5]
    (hs, ws), (hr, wr), top, n = shape
    img, ref = ir.case(shape)
    x = torch.from_numpy(img.copy()).to(dev)
    lab = torch.from_numpy(np.random.RandomState(1).randint(0, 4096, size=(1, 20, 20)).astype(np.int32)).to(dev)
    eager = ops.resize_pil_bilinear(x, (wr, hr), top).clone()      # (the first call per size uploads the tables: outside the capture)
    eager_bev = ops.decode_bev(lab, 12).clone()
    out = torch.zeros_like(eager)
    out_bev = torch.zeros_like(eager_bev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.resize_pil_bilinear(x, (wr, hr), top, out=out)
        ops.decode_bev(lab, 12, out=out_bev)
    x.copy_(torch.flip(x, dims=[0]))                               # new frames in the captured buffer
    lab.copy_(lab.flip(1))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(ir.to_tensor(ref[::-1])))
    assert torch.equal(out_bev, ops.decode_bev(lab, 12)) and torch.equal(eager.flip(0), out)
    assert torch.equal(eager_bev.flip(2), out_bev)
