"""The train-mode LiDAR pillar front end without a GPU: the test-side restatement (tests/pillar_train_ref.py) replayed against the
reference fixture gv22 (forward, every parameter gradient, the BatchNorm1d buffers after the step), the state_dict schema in train()
mode, and the errors the training path raises before it touches a device."""
import pytest
import torch

import cases_pillar as cp
import pillar_ref as pr
import pillar_train_ref as ptr
from cobevt_amd import host, synth
from cobevt_amd.lib import CobevtHipError
from cobevt_amd.synth import fill_module_
from util import assert_close, golden

PREFIX = "pillar_vfe.pfn_layers.0."
CASES = [(a, d, True) for a, d in cp.COMBOS] + [(True, False, False)]


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other modules of the suite switch autograd off globally; these tests differentiate"""
    with torch.enable_grad():
        yield


def _model(*combo):
    return fill_module_(host.PointPillarFuseBEVT(cp.model_args(*combo)), cp.SEED)


@pytest.mark.parametrize("use_abs,dist,use_norm", CASES)
def test_restatement_replays_the_fixture(use_abs, dist, use_norm):
    fx = golden("gv22_point_pillar_train")
    name = cp.combo_name(use_abs, dist, use_norm)
    args = cp.model_args(use_abs, dist, use_norm)
    sd = _model(use_abs, dist, use_norm).state_dict()
    vox = cp.voxels()
    p = ptr.params(sd, PREFIX, use_norm)
    rows = ptr.pillar_features(p, vox["voxel_features"], vox["voxel_num_points"], vox["voxel_coords"],
                               pr.geom(args["voxel_size"], args["lidar_range"]), use_abs, dist, use_norm)
    ref = torch.from_numpy(fx["pillar_features/" + name])
    w = synth.procedural_input("train.w.pillar_train", tuple(ref.shape), cp.SEED)
    (rows * w).sum().backward()
    assert_close(rows, ref, 1e-5, "pillar_features " + name)
    grads = [k for k in fx.files if k.startswith("grad/%s/" % name)]
    assert len(grads) == (3 if use_norm else 2)
    for k in grads:
        assert_close(p[k.split("/")[-1]].grad, torch.from_numpy(fx[k]), 1e-5, k)
    bufs = [k for k in fx.files if k.startswith("buffer/%s/" % name)]
    assert len(bufs) == (3 if use_norm else 0)
    for k in bufs:
        got, want = p[k.split("/")[-1]], torch.from_numpy(fx[k])
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(want) == 1
        else:
            assert_close(got, want, 1e-5, k)
            assert float((want - sd[PREFIX + k.split("/")[-1]]).abs().max()) > 0          # the step moved the statistics


def test_train_mode_keeps_the_state_dict_schema():
    fx = golden("gv21_point_pillar")
    m = _model().train()
    assert m.training and m.pillar_vfe.training and m.pillar_vfe.pfn_layers[0].norm.training
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in fx["keys"]]
    assert [",".join(str(int(d)) for d in t.shape) for t in sd.values()] == [str(s) for s in fx["shapes"]]
    stored = {k[len("model_grad/"):] for k in golden("gv22_point_pillar_train").files if k.startswith("model_grad/")}
    assert stored == {k for k, _ in m.named_parameters()}


def test_training_forward_refuses_what_it_cannot_do():
    m = _model().train()
    vox = cp.voxels()
    # no gradient with respect to the points
    bad = dict(vox)
    bad["voxel_features"] = vox["voxel_features"].clone().requires_grad_(True)
    with pytest.raises(CobevtHipError, match="voxel_features"):
        m.pillar_vfe(bad)
    with pytest.raises(CobevtHipError, match="voxel_features"):
        m({"processed_lidar": bad, "record_len": torch.tensor(cp.RECORD_LEN)})
    # a cumulative running average has no kernel
    m.pillar_vfe.pfn_layers[0].norm.momentum = None
    with pytest.raises(CobevtHipError, match="momentum"):
        m.pillar_vfe(dict(vox))
    with pytest.raises(CobevtHipError, match="momentum"):
        m({"processed_lidar": dict(vox), "record_len": torch.tensor(cp.RECORD_LEN)})
    # and no CPU path: on CPU tensors a train() forward is refused as before
    with pytest.raises(CobevtHipError, match="call .eval\\(\\) first"):
        _model().train().pillar_vfe(dict(vox))
    with pytest.raises(CobevtHipError, match="call .eval\\(\\) first"):
        _model().train().scatter({"pillar_features": torch.zeros(300, 64), "voxel_coords": vox["voxel_coords"], "batch_size": 3})
