"""The nuScenes CVT model (config/model/cvt.yaml: host.nuscenes.Encoder + Decoder + CrossViewTransformer) on the GPU, and the
camera-paired key split its first cross-view attention runs on (cobevt_window_attention_ksplit with mean_q = 2)."""
import numpy as np
import pytest
import torch

import cases_nusc_cvt as cc
from cobevt_amd import host, ops, synth
from cobevt_amd.host import nuscenes as nu
from cobevt_amd.host import pipeline
from cobevt_amd.lib import CobevtHipError
from cobevt_amd.synth import fill_module_
from util import BF16_FLOOR, RMS_FRACTION, assert_close, golden, rel_err, rms_rel_err

pytestmark = pytest.mark.gpu

MODES = ["bf16", "fp32", "fp32_split", "fp32_fast"]          # the three libraries: "" (bf16 / fp32), f32s, f32h
DENSE_TOL = {"bf16": 1e-2, "fp32": 1e-4, "fp32_split": 1e-4, "fp32_fast": 2e-3}
UNSPLIT_TOL = {"bf16": 1e-2, "fp32": 2e-5, "fp32_split": 5e-5, "fp32_fast": 1e-3}
# (cameras, BEV query side, key map h x w per camera, splits): the level-1 shape of cvt.yaml; ragged keys per camera (35: one partial tile
# per camera); 130 keys per camera (3 tiles, the last of 2 keys) so that splits start inside a camera (2, 4) and on a camera's ragged
# last tile (4: tiles [2, 4) start on camera 0's third tile; 8: one tile each)
SHAPES = {"real": (6, 25, (56, 120), (2, 3, 8, 16)),
          "ragged": (3, 6, (5, 7), (2, 3)),
          "mid_camera": (3, 6, (10, 13), (2, 3, 4, 8))}


def _dense_paired(q, k, v, B, n, Q, K, heads):
    """fp32 torch: camera c's query copy scores camera c's keys, one softmax over all cameras' keys (cvt_modules.py:142-153)"""
    qf = q.float().reshape(B, n, Q, heads, 32).permute(0, 3, 1, 2, 4)            # b m n Q dh
    kf = k.float().reshape(B, n, K, heads, 32).permute(0, 3, 1, 2, 4)            # b m n K dh
    vf = v.float().reshape(B, n * K, heads, 32).permute(0, 2, 1, 3)              # b m (n K) dh
    out = []
    for bi in range(B):
        dot = 32 ** -0.5 * torch.matmul(qf[bi], kf[bi].transpose(-1, -2))       # m n Q K
        att = dot.permute(0, 2, 1, 3).reshape(heads, Q, n * K).softmax(-1)
        out.append(torch.matmul(att, vf[bi]).permute(1, 0, 2).reshape(Q, heads * 32))
    return torch.stack(out)


def _paired(q, k, v, B, n, H, hw, heads, ksplit):
    d = heads * 32
    out = torch.empty((B, H, H, d), device=q.device, dtype=q.dtype)
    qmap, kmap, omap = ops.tokmap(0, n, H, H, H, H), ops.tokmap(0, n, hw[0], hw[1], hw[0], hw[1]), ops.tokmap(0, 1, H, H, H, H)
    with ops.LaunchProfile() as prof:
        ops.window_attention(q, k, v, out, qmap, kmap, omap, B, heads, 32 ** -0.5, d, d, d, d, mean_q=2, ksplit=ksplit)
    names = list(prof.summary(by_shape=True))
    return out, names


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("mode", MODES)
def test_camera_paired_key_split(cuda, mode, heads, shape):
    """Every split count against a dense fp32 softmax and against the single-pass launch (ksplit=None), B = 2"""
    n, H, hw, splits = SHAPES[shape]
    B, d, Q, K = 2, heads * 32, H * H, hw[0] * hw[1]
    g = torch.Generator().manual_seed(20 + heads)
    with host.compute_dtype(mode):
        dt = host.get_compute_dtype()
        q = (torch.randn(B, n, Q, d, generator=g) * 1.5).to(dt).to(cuda)
        k = (torch.randn(B * n, hw[0], hw[1], d, generator=g) * 1.5).to(dt).to(cuda)
        v = torch.randn(B * n, hw[0], hw[1], d, generator=g).to(dt).to(cuda)
        ref = _dense_paired(q, k, v, B, n, Q, K, heads).reshape(B, H, H, d)
        single, names = _paired(q, k, v, B, n, H, hw, heads, None)
        assert len(names) == 1 and "ks" not in names[0], names
        assert rel_err(single, ref) <= DENSE_TOL[mode]
        for ks in splits:
            out, names = _paired(q, k, v, B, n, H, hw, heads, ks)
            torch.cuda.synchronize()
            assert len(names) == 1 and names[0].endswith(" ks%d" % ks), names
            e_ref, e_one = rel_err(out, ref), rel_err(out, single)
            assert e_ref <= DENSE_TOL[mode], "%s ks%d vs dense: %.3e" % (mode, ks, e_ref)
            assert e_one <= UNSPLIT_TOL[mode], "%s ks%d vs single pass: %.3e" % (mode, ks, e_one)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_camera_paired_key_split_too_many_splits(cuda, dtype):
    """3 cameras x 35 keys = 3 key tiles (tiles never mix cameras): 4 splits leave one without a tile -> COBEVT_ERR_SHAPE; 17 > the cap"""
    n, H, hw = 3, 6, (5, 7)
    q = torch.zeros(1, n, H * H, 32, device=cuda, dtype=dtype)
    k = torch.zeros(n, hw[0], hw[1], 32, device=cuda, dtype=dtype)
    _paired(q, k, k, 1, n, H, hw, 1, 3)
    with pytest.raises(CobevtHipError, match="code 2"):
        _paired(q, k, k, 1, n, H, hw, 1, 4)
    with pytest.raises(CobevtHipError, match="code 1"):
        _paired(q, k, k, 1, n, H, hw, 1, 17)


# ---------------------------------------------------------------------------------------------- the model against gv20
@pytest.fixture(scope="module")
def cvt_model(cuda):
    feats, image, intr, ext = cc.inputs()
    m = fill_module_(cc.build(nu, synth.FeatureMapBackbone(feats)), cc.SEED).to(cuda)
    return m, {"image": image.to(cuda), "intrinsics": intr.to(cuda), "extrinsics": ext.to(cuda)}


def _bf16_gates(fx, key):
    """max(1e-2, the reference's own bf16-autocast deviation of this output) and the rms gate derived as in tests/util.py"""
    r = fx["bf16_autocast/nuScenes CVT." + key]
    return max(BF16_FLOOR, float(r[0])), max(RMS_FRACTION[True] * BF16_FLOOR, float(r[1]))


def _forward(m, batch, mode):
    with torch.no_grad(), host.compute_dtype(mode):
        enc = m.encoder(batch)
        out = m(batch)
    torch.cuda.synchronize()
    return {"encoder": enc, "bev": out["bev"], "center": out["center"]}


@pytest.mark.parametrize("mode", MODES)
def test_nuscenes_cvt_matches_reference(cvt_model, mode):
    """Encoder output and both heads against the reference's fp32 forward (gv20): fp32 modes within 1e-3; bf16 within the reference's
    own bf16 deviation (floor 1e-2, rms gate as tests/util.py derives it).  The bf16 encoder output is the one exception in the max
    norm: it sits at 1.05e-2 with the single-pass attention as with the key split (bf16 storage of a map whose values reach 4.5 costs
    up to 3.5e-3 in the final rounding alone), so there the key split is held to the single-pass launch's max-rel and the rms gate."""
    m, batch = cvt_model
    fx = golden("gv20_nuscenes_cvt")
    got = _forward(m, batch, mode)
    single = None
    if mode == "bf16":
        nu.CrossViewAttention.key_split = False
        try:
            single = _forward(m, batch, mode)
        finally:
            nu.CrossViewAttention.key_split = True
    for key, t in got.items():
        ref = torch.from_numpy(fx[key])
        if mode == "bf16":
            tol, rms_gate = _bf16_gates(fx, key)
            e, r = rel_err(t, ref), rms_rel_err(t, ref)
            if key == "encoder":
                tol = max(tol, rel_err(single[key], ref) + 1e-3)
            assert e <= tol and r <= rms_gate, "nuScenes CVT %s bf16: max-rel %.3e (gate %.2e) rms-rel %.3e (gate %.2e)" % (key, e, tol, r, rms_gate)
        else:
            assert_close(t, ref, 1e-3, "nuScenes CVT %s %s" % (key, mode))


def test_nuscenes_cvt_level1_runs_key_split(cvt_model):
    """LaunchProfile: the level-1 camera-paired attention (6 x 625 queries, 6 x 6720 keys) is a key-split launch; its split count is
    ops.paired_ksplit's"""
    m, batch = cvt_model
    with torch.no_grad(), host.compute_dtype(torch.bfloat16), ops.LaunchProfile() as prof:
        m(batch)
    names = [k for k in prof.summary(by_shape=True) if k.startswith("attention|")]
    lvl1 = [k for k in names if " Nq3750 Nk40320" in k]
    ks = ops.paired_ksplit(1, 4, ops.tokmap(0, 6, 25, 25, 25, 25), ops.tokmap(0, 6, 56, 120, 56, 120))
    assert ks is not None and ks >= 8
    assert lvl1 == ["attention|B1 L1 h4 Nq3750 Nk40320 ks%d" % ks], names


def test_nuscenes_cvt_graph_replay_equals_eager(cvt_model):
    """pipeline.CapturedCall (one captured HIP graph, as the probe / benchmarks run it) == the eager forward, bit for bit"""
    m, batch = cvt_model
    with torch.no_grad(), host.compute_dtype(torch.bfloat16):
        eager = m(batch)
        run = pipeline.CapturedCall(lambda im, ii, ee: m({"image": im, "intrinsics": ii, "extrinsics": ee}),
                                    batch["image"], batch["intrinsics"], batch["extrinsics"])
        got = run.step(batch["image"], batch["intrinsics"], batch["extrinsics"])
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(got[k], eager[k]), k


# ---------------------------------------------------------------------------------------------- real backbone, from images
def _from_images_model(cuda):
    backbone = nu.EfficientNetExtractor(cc.LAYER_NAMES, *cc.IMAGE)
    return fill_module_(cc.build(nu, backbone), cc.SEED).to(cuda)


def test_nuscenes_cvt_from_images_vs_oracle(cuda):
    """EfficientNet-B4 extractor mirror -> Encoder -> Decoder -> heads from images, against oracle.efficientnet + the composition
    (EfficientNet arithmetic is restated: unpinned, as in test_efficientnet.py)"""
    m = _from_images_model(cuda)
    assert [tuple(s[1:]) for s in m.encoder.backbone.output_shapes] == cc.FEATURE_SHAPES
    _, image, intr, ext = cc.inputs()
    sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref, ref_enc = cc.oracle_from_images(sd, cc.config(), image, intr, ext)
        with host.compute_dtype(torch.float32):
            batch = {"image": image.to(cuda), "intrinsics": intr.to(cuda), "extrinsics": ext.to(cuda)}
            enc = m.encoder(batch)
            out = m(batch)
    torch.cuda.synchronize()
    assert_close(enc, ref_enc, 1e-3, "nuScenes CVT from images: encoder")
    for k in ref:
        assert_close(out[k], ref[k], 1e-3, "nuScenes CVT from images: %s" % k)


# ---------------------------------------------------------------------------------------------- training
def test_nuscenes_cvt_trains_gradients_vs_oracle(cuda):
    """train() mode (training.nusc_cvt_encoder: EfficientNet graph, CVT cross-view attention, bottlenecks; extrinsics inverted) against
    torch autograd through oracle.efficientnet + the composition: logits and every parameter gradient, the max-norm gate as for SinBEVT
    (2e-2).  The rms gate is 1e-2 instead of SinBEVT's 5e-3: the last bottleneck's bn2.weight gradient - a sum over all 625 BEV cells
    of terms that largely cancel - measured 5.4e-3 in fp32"""
    from test_training_gpu import _compare, _freeze_bn, _oracle_sd
    m = _freeze_bn(_from_images_model(cuda).train())
    for group in list(m.encoder.backbone.layers)[1:]:
        group.args = [[0.0] for _ in group.args]                  # drop-connect off: the oracle is the eval-mode function
    sd = _oracle_sd(m)
    _, image, intr, ext = cc.inputs()
    with torch.enable_grad():
        ref, _ = cc.oracle_from_images(sd, cc.config(), image, intr, ext)
        out = m({"image": image.to(cuda), "intrinsics": intr.to(cuda), "extrinsics": ext.to(cuda)})
        out_ref = torch.cat([ref["bev"], ref["center"]], 1)
        _compare(m, sd, torch.cat([out["bev"], out["center"]], 1), out_ref, [], [], "nuScenes CVT", grad_tol=2e-2, rms_tol=1e-2)


def test_nuscenes_cvt_training_steps(cuda):
    """five AdamW steps of MultipleLoss(BinarySegmentationLoss + CenterLoss) in full train() mode lower the loss"""
    m = fill_module_(cc.build(nu, nu.EfficientNetExtractor(cc.LAYER_NAMES, *cc.IMAGE)), cc.SEED).train().to(cuda)
    _, image, intr, ext = cc.inputs()
    batch = {"image": image.to(cuda), "intrinsics": intr.to(cuda), "extrinsics": ext.to(cuda)}
    g = torch.Generator().manual_seed(4)
    batch["bev"] = (torch.rand(1, 12, 200, 200, generator=g) > 0.8).float().to(cuda)
    batch["center"] = torch.rand(1, 1, 200, 200, generator=g).to(cuda)
    batch["visibility"] = torch.randint(0, 5, (1, 200, 200), generator=g).to(torch.uint8).to(cuda)
    losses = nu.MultipleLoss({"bev": nu.BinarySegmentationLoss(label_indices=[[4, 5, 6, 7, 8, 10, 11]], min_visibility=2, alpha=-1.0, gamma=2.0),
                              "bev_weight": 1.0, "center": nu.CenterLoss(min_visibility=2, alpha=-1.0, gamma=2.0), "center_weight": 0.1})
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    seen = []
    with torch.enable_grad():
        for _ in range(5):
            opt.zero_grad(set_to_none=True)
            total, _ = losses(m(batch), batch)
            total.backward()
            opt.step()
            seen.append(float(total.detach()))
    assert np.isfinite(seen).all() and seen[-1] < seen[0], seen
    m.eval()
    with torch.no_grad():
        y = m(batch)
    assert torch.isfinite(y["bev"]).all() and tuple(y["bev"].shape) == (1, 1, 200, 200)

