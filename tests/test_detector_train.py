"""Training of the PointPillar detectors without a device: the train-mode restatement tests/detector_train_ref.py against the golden
recorded from the reference's backbones in .train() mode (tests/golden/gv30_detector_train.npz), its ReLU masks in fp32 and float64 on
every module case of the GPU file, the weight tables of ops.deconv_train_weights, the chunk rule, every refusal of the new ops
functions and of the new C entry points with host pointers, the modules' refusals on CPU tensors, and the launch traces of one
forward + backward of both detectors."""
import ctypes

import pytest
import torch

import att_backbone_ref as ar
import bev_backbone_ref as br
import detector_train_ref as dr
import launch_trace as lt
import launch_trace_detector_train as ltd
from cobevt_amd import autograd as ag
from cobevt_amd import host, lib, ops
from cobevt_amd.lib import CobevtHipError


@pytest.fixture(autouse=True)
def _grad_mode():
    with torch.enable_grad():
        yield


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("tag", ["att", "base"])
def test_restatement_replays_the_reference_golden(tag):
    """output, input gradient, every parameter gradient and the running statistics after the step, at the recorded elements, to 1e-9"""
    z = dr.load_golden()
    module, cfg, x, rl = dr.module_case("golden", tag == "att")
    shape = tuple(int(v) for v in z[tag + "/output_shape"])
    got = dr.run(module.state_dict(), cfg, x, rl, torch.float64, weight=dr.loss_weight(shape))
    assert tuple(got["out"].shape) == shape

    def same(name, a, want):
        assert a.shape == want.shape, name
        assert float((a - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max())), name

    same("output", dr.sample(got["out"]), z[tag + "/output"])
    same("dx", dr.sample(got["dx"]), z[tag + "/dx"])
    keys = [k[len(tag + "/grad/"):] for k in z if k.startswith(tag + "/grad/")]
    assert sorted(keys) == sorted(k for k, _ in module.named_parameters())
    for k in keys:
        same(k, dr.sample(got["grads"][k]), z["%s/grad/%s" % (tag, k)])
    assert len(got["tape"].running) == 9
    for prefix, (rm, rv) in got["tape"].running.items():
        same(prefix + "running_mean", rm, z["%s/after/%srunning_mean" % (tag, prefix)])
        same(prefix + "running_var", rv, z["%s/after/%srunning_var" % (tag, prefix)])
        assert int(z["%s/after/%snum_batches_tracked" % (tag, prefix)]) == 1


MODULE_CASES = [(name, att) for name in sorted(dr.MODULE_SEEDS) for att in (True, False) if att or name != "compression"]


@pytest.mark.parametrize("name,att", MODULE_CASES)
def test_fp32_and_float64_restatements_cut_the_same_pre_activations(name, att):
    """the seeds of the module-level GPU cases: 0 mask disagreements of the restatement alone, and a ReLU that cuts"""
    module, cfg, x, rl = dr.module_case(name, att)
    a, b = (dr.run(module.state_dict(), cfg, x, rl, dt) for dt in (torch.float64, torch.float32))
    assert dr.mask_disagreements(a["tape"], b["tape"]) == 0
    assert 0.1 <= float((a["out"] == 0).double().mean()) <= 0.9
    forced = dr.run(module.state_dict(), cfg, x, rl, torch.float64, masks=b["tape"].free_masks())
    assert torch.equal(forced["out"], a["out"])


def test_forced_masks_and_frozen_statistics():
    module, cfg, x, rl = dr.module_case("golden", False)
    sd = module.state_dict()
    free = dr.run(sd, cfg, x, rl, torch.float64)
    masks = [~m for m in free["tape"].free_masks()]
    flipped = dr.run(sd, cfg, x, rl, torch.float64, masks=masks)
    assert not torch.equal(flipped["out"], free["out"])
    frozen = dr.run(sd, cfg, x, rl, torch.float64, frozen=["deblocks.0.1."])
    assert "deblocks.0.1." not in frozen["tape"].running and len(frozen["tape"].running) == 8


# ---------------------------------------------------------------------------------------------- weight tables, chunk rule
@pytest.mark.parametrize("case", dr.kernel_cases())
def test_deconv_train_weights_are_the_plan_and_the_igemm_rows(case):
    weight, _, _ = dr.kernel_operands(case)
    s, cin, cout = case[0], case[1], case[2]
    fwd, rows = ops.deconv_train_weights(weight)
    plan = ops.DeconvPlan(weight, None, s, torch.float32, "cpu")
    assert torch.equal(fwd, plan.wgt) and plan.kpad == fwd.shape[1]
    want, k, kpad = ag._weight_rows(weight)                  # the weight read as (out = Cin, in = Cout, s, s)
    assert k == s * s * cout and torch.equal(rows, want) and tuple(rows.shape) == (cin, kpad)
    # the rows ARE the input gradient's operand: dx = conv(dz, W as (Cin, Cout, s, s), stride s)
    _, x, dz = dr.kernel_operands(case)
    dx = torch.nn.functional.conv2d(dz.permute(0, 3, 1, 2).double(), weight.double(), stride=s).permute(0, 2, 3, 1)
    assert float((dx - dr.dgrad_f64(dz, weight)[0]).abs().max()) < 1e-12
    z = torch.nn.functional.conv_transpose2d(x.permute(0, 3, 1, 2).double(), weight.double(), stride=s).permute(0, 2, 3, 1)
    assert float((z - dr.raw_f64(x, weight)[0]).abs().max()) < 1e-12


def test_deconv_train_weights_cache_follows_the_parameter():
    w = torch.nn.Parameter((torch.rand(8, 32, 2, 2) - 0.5))
    a = ops.deconv_train_weights(w)
    assert ops.deconv_train_weights(w)[0] is a[0]
    with torch.no_grad():
        w.mul_(2.0)
    b = ops.deconv_train_weights(w)
    assert b[0] is not a[0] and torch.equal(b[0], 2.0 * a[0]) and torch.equal(b[1], 2.0 * a[1])
    key = id(w)
    del w, a, b
    assert key not in ops._DECONV_TRAIN_WEIGHTS


def test_wgrad_is_the_autograd_weight_gradient():
    case = (2, 8, 32, 2, 3, 5, 0, 32)
    weight, x, dz = dr.kernel_operands(case)
    w = weight.double().requires_grad_(True)
    z = torch.nn.functional.conv_transpose2d(x.permute(0, 3, 1, 2).double(), w, stride=2)
    (z * dz.permute(0, 3, 1, 2).double()).sum().backward()
    ref, mag = dr.wgrad_f64(x, dz, 2)
    assert float((w.grad - ref).abs().max()) < 1e-12 and bool((mag >= ref.abs() - 1e-12).all())


def test_chunk_rule():
    """a pure function of the shape: chunks of an even length of at least 64 pixels (one chunk below), at most 64 MB of partial sums,
    512 .. 4096 one-wave workgroups (two per CU at least) at the standard deblocks on a 256 x 256 canvas; minus an error code for what is not served"""
    f = lib.load("").cobevt_deconv_wgrad_chunks
    ints = lambda *v: (ctypes.c_int * len(v))(*v)          # noqa: E731
    assert f(ints(1, 37, 53, 32, 32, 1)) == 31            # 1961 pixels: 30 chunks of 64 and one of 41
    assert f(ints(3, 1, 1, 32, 32, 2)) == 1
    nums, ups = br.STANDARD_CFG["num_filters"], br.STANDARD_CFG["upsample_strides"]
    for i, (cin, s) in enumerate(zip(nums, ups)):
        hw = 128 >> i
        chunks = f(ints(1, hw, hw, cin, 128, s))
        floats = chunks * s * s * cin * 128
        groups = chunks * s * s * (cin // 32)              # 128 output channels are one group of four tiles
        assert chunks >= 1 and floats * 4 <= 64 << 20 and 512 <= groups <= 4096, (i, chunks, groups)
    assert f(None) == -1
    for bad in ((0, 4, 4, 32, 32, 2), (1, 4, 4, 32, 32, 0), (1, 4, 4, 32, 32, 9), (1, 4, 4, 30, 32, 2), (1, 4, 4, 32, 48, 2), (1, 4, 4, 0, 32, 2),
                (1, 32768, 32768, 32, 32, 2), (1, 4, 4, 4096, 4096, 8)):
        assert f(ints(*bad)) == -2, bad
    assert ops.deconv_wgrad_chunks(1, 37, 53, 32, 32, 1) == 31
    with pytest.raises(CobevtHipError, match="not served"):
        ops.deconv_wgrad_chunks(1, 4, 4, 30, 32, 2)


# ---------------------------------------------------------------------------------------------- refusals
def test_c_entries_refuse_before_any_launch():
    """null pointers: COBEVT_ERR_ARG = 1; unsupported shapes, a wrong chunk count and misaligned pointers: COBEVT_ERR_SHAPE = 2 (host
    pointers: nothing is dereferenced on this side, and nothing is launched)"""
    l = lib.load("")
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    off = ctypes.c_void_p(ptr.value + 2)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)          # noqa: E731
    f = ctypes.c_float
    good = (1, 4, 4, 32, 32, 2, 1)
    assert l.cobevt_deconv_wgrad(ptr, ptr, ptr, ptr, None, None) == 1
    for hole in range(4):
        args = [ptr] * 4
        args[hole] = None
        assert l.cobevt_deconv_wgrad(*(args + [ints(*good), None])) == 1, hole
    for hole in range(4):
        args = [ptr] * 4
        args[hole] = off
        assert l.cobevt_deconv_wgrad(*(args + [ints(*good), None])) == 2, hole
    for bad in ((1, 4, 4, 32, 32, 2, 2), (1, 4, 4, 32, 32, 2, 0), (0, 4, 4, 32, 32, 2, 1), (1, 4, 4, 30, 32, 2, 1), (1, 4, 4, 32, 16, 2, 1),
                (1, 4, 4, 32, 32, 9, 1), (1, 4, 4, 32, 32, 0, 1), (1, 32768, 32768, 32, 32, 2, 1)):
        assert l.cobevt_deconv_wgrad(ptr, ptr, ptr, ptr, ints(*bad), None) == 2, bad
    bwd = l.cobevt_att_fuse_bwd_nhwc
    for hole in range(4):
        args = [ptr] * 4
        args[hole] = None
        assert bwd(*(args + [1, 2, 6, 32, f(0.1), None])) == 1, hole
    for b, n, hw, c in ((0, 2, 6, 32), (65536, 2, 6, 32), (1, 0, 6, 32), (1, 2, 0, 32), (1, 2, 6, 24), (1, 2, 6, 4), (1, 2, 6, 1024), (1, 2, 6, 36)):
        assert bwd(ptr, ptr, ptr, ptr, b, n, hw, c, f(0.1), None) == 2, (b, n, hw, c)


def test_ops_refuse_before_any_launch(monkeypatch):
    rec = lt.Recorder()
    lt.install(monkeypatch.setattr, rec)
    x, rl, g = torch.zeros(3, 4, 5, 32), torch.tensor([2, 1], dtype=torch.int32), torch.zeros(2, 4, 5, 32)
    for bad, msg in (((x[:, :, :, :16], rl, g), "contiguous"), ((x.bfloat16(), rl, g), "fp32 storage only"), ((torch.zeros(3, 4, 5, 24), rl, g), "8 times"),
                     ((x, rl.long(), g), "int32"), ((x, rl[:0], g), "B >= 1"), ((x, rl, g[:1]), "dout must be"), ((x, rl, g.double()), "dout must be"),
                     ((x, rl, g.permute(0, 2, 1, 3)), "dout must be"), ((torch.zeros(3, 20, 32), rl, g), "contiguous non-empty")):
        with pytest.raises(CobevtHipError, match=msg):
            ops.att_fuse_bwd(*bad)
    xd, dz = torch.zeros(2, 3, 5, 8), torch.zeros(2, 6, 10, 32)
    for bad, msg in (((xd.double(), dz, 2), "fp32"), ((xd, dz, 3), "dz must be"), ((xd, torch.zeros(2, 6, 10, 16), 2), "multiple of 32"), ((torch.zeros(2, 3, 5, 6), dz, 2), "multiple of 4"),
                     ((xd, dz, 0), "stride 0"), ((xd, torch.zeros(2, 27, 45, 32), 9), "stride 9"), ((xd, dz.permute(0, 2, 1, 3), 2), "dz must be"),
                     ((xd, None, 2), "4-D")):
        with pytest.raises(CobevtHipError, match=msg):
            ops.deconv_wgrad(*bad)
    fwd, _ = ops.deconv_train_weights(torch.zeros(8, 32, 2, 2))
    for bad, msg in (((xd, fwd[:64], 32, 2), "weight table"), ((xd, fwd, 32, 1), "weight table"), ((xd.bfloat16(), fwd, 32, 2), "fp32"),
                     ((xd, fwd.double(), 32, 2), "weight table"), ((torch.zeros(2, 3, 5, 6), fwd, 32, 2), "multiple of 4")):
        with pytest.raises(CobevtHipError, match=msg):
            ops.deconv_raw(*bad)
    for bad, msg in ((torch.zeros(8, 32, 2, 3), "must be fp32"), (torch.zeros(8, 32, 2, 2).double(), "must be fp32"), (torch.zeros(8, 32, 9, 9), "stride 9"),
                     (torch.zeros(6, 32, 2, 2), "multiple of 4"), (torch.zeros(8, 16, 2, 2), "multiple of 32"), (torch.zeros(8, 32, 2), "must be fp32")):
        with pytest.raises(CobevtHipError, match=msg):
            ops.deconv_train_weights(bad)
    for conv in (torch.nn.ConvTranspose2d(8, 32, 2, stride=2), torch.nn.ConvTranspose2d(8, 32, 3, stride=2, bias=False), torch.nn.Conv2d(8, 32, 2, stride=2, bias=False),
                 torch.nn.ConvTranspose2d(8, 32, 2, stride=2, padding=1, bias=False)):
        with pytest.raises(CobevtHipError, match="training deconv"):
            ag.deconv(torch.zeros(1, 8, 3, 3), conv)
    assert rec.records == []


def test_modules_refuse_train_mode_on_cpu_tensors_with_the_inference_wording():
    for module, args in ((host.BaseBEVBackbone(dict(br.GOLDEN_CFG), 32), (torch.zeros(1, 16, 24, 32),)),
                         (host.AttBEVBackbone(dict(ar.GOLDEN_CFG), 32), (torch.zeros(2, 16, 24, 32), torch.tensor([2], dtype=torch.int32))),
                         (host.AttFusion(32), (torch.zeros(2, 4, 4, 32), torch.tensor([2], dtype=torch.int32))),
                         (host.AutoEncoder(64, 1), (torch.zeros(1, 8, 8, 64),))):
        with pytest.raises(CobevtHipError, match="fused inference path: call .eval\\(\\) first"):
            module.train().forward_nhwc(*args)


def test_level_sizes_are_checked_before_any_launch(monkeypatch):
    rec = lt.Recorder()
    lt.install(monkeypatch.setattr, rec)
    from cobevt_amd.host import training
    for cls, extra in ((host.BaseBEVBackbone, ()), (host.AttBEVBackbone, (torch.tensor([2], dtype=torch.int32),))):
        model = cls(dict(br.GOLDEN_CFG), 32).train()
        fn = training.base_bev_backbone if not extra else training.att_bev_backbone
        with pytest.raises(CobevtHipError, match="a 10 x 24 input gives 5 x 12, 6 x 12, 8 x 12"):
            fn(model, torch.zeros(2, 32, 10, 24), *extra)
    assert rec.records == []


# ---------------------------------------------------------------------------------------------- launch traces
@pytest.mark.parametrize("case", ltd.CASES)
def test_launch_trace_of_one_training_step(case, monkeypatch):
    got = ltd.trace(case, monkeypatch.setattr)
    assert lt.dumps(got) == lt.dumps(ltd.read_fixture(case))
    assert all(r[0] == "" for r in got), "a training launch left the native library"
    names = [r[1] for r in got]
    deconvs = [r[2][4] for r in got if r[1] == "cobevt_deconv_nhwc"]
    # the raw forward only: fp32, c_off 0 into a map of its own width, no activation (the shift operand is the zero vector)
    assert len(deconvs) == 3 and all(d[0] == 1 and d[8] == 0 and d[9] == d[5] and d[10] == 0 for d in deconvs)
    # one wgrad pair per transposed conv, with the chunk count the library answered
    at = [i for i, n in enumerate(names) if n == "cobevt_deconv_wgrad_chunks"]
    assert len(at) == 3 and all(names[i + 1] == "cobevt_deconv_wgrad" and got[i + 1][2][4][6] == ltd.CHUNKS for i in at)
    assert sorted(tuple(got[i][2][0]) for i in at) == sorted((d[1], d[2], d[3], d[4], d[5], d[7]) for d in deconvs)
    fwd, bwd = names.count("cobevt_att_fuse_nhwc"), names.count("cobevt_att_fuse_bwd_nhwc")
    assert (fwd, bwd) == ((3, 3) if case.startswith("point_pillar_intermediate") else (0, 0))          # exactly one backward per level
    assert names.count("cobevt_bn_batch_stats") == names.count("cobevt_bn_backward") == 9
    assert names.count("cobevt_bn_finalize") == 0
