"""The nuScenes CVT encoder (config/model/cvt.yaml) without a GPU: module schema and contract against the reference fixture gv20,
the test-side oracle composition against the reference's outputs, and the split-count helper of its camera-paired attention."""
import importlib
import os
import subprocess
import sys

import pytest
import torch

import cases_nusc_cvt as cc
from cobevt_amd import ops, synth
from cobevt_amd.host import nuscenes as nu
from cobevt_amd.synth import fill_module_
from util import golden, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    feats, _, _, _ = cc.inputs()
    return cc.build(nu, synth.FeatureMapBackbone(feats))


def test_state_dict_schema_matches_reference():
    fx = golden("gv20_nuscenes_cvt")
    sd = _model().state_dict()
    assert list(sd.keys()) == [str(k) for k in fx["keys"]]
    assert [",".join(str(int(d)) for d in v.shape) for v in sd.values()] == [str(s) for s in fx["shapes"]]
    assert len(sd) == 199


def test_oracle_composition_matches_reference():
    """oracle.cvt + oracle.nuscenes, composed in tests/golden/cases_nusc_cvt.py, reproduce the reference's outputs (gv20)"""
    fx = golden("gv20_nuscenes_cvt")
    feats, _, intr, ext = cc.inputs()
    sd = fill_module_(_model(), cc.SEED).state_dict()
    with torch.no_grad():
        out, enc = cc.oracle_model(sd, cc.config(), feats, intr, ext)
    assert rel_err(enc, torch.from_numpy(fx["encoder"])) <= 1e-5
    for k in ("bev", "center"):
        assert rel_err(out[k], torch.from_numpy(fx[k])) <= 1e-5, k


def test_scale_below_one_raises():
    c = cc.config()
    c["encoder"]["scale"] = 0.5
    with pytest.raises(NotImplementedError):
        cc.build(nu, synth.FeatureMapBackbone(cc.inputs()[0]), c)


def test_encoder_resolves_by_dotted_path():
    """cvt.yaml with its `_target_` lines pointed at the package"""
    for name, cls in (("Encoder", nu.Encoder), ("CrossViewAttention", nu.CrossViewAttention), ("BEVEmbedding", nu.BEVEmbedding),
                      ("CrossAttention", nu.CrossAttention)):
        mod, _, attr = ("cobevt_amd.host.nuscenes." + name).rpartition(".")
        assert getattr(importlib.import_module(mod), attr) is cls
    # the nuScenes keyword signature of CrossViewAttention (cvt.yaml's cross_view block) builds the OPV2V module's submodules
    cva = nu.CrossViewAttention(56, 120, 32, 128, **cc.config()["encoder"]["cross_view"])
    assert cva.key_split and cva.cross_attend.heads == 4 and cva.feature_proj is not None and cva.skip


def test_product_does_not_import_oracle():
    code = ("import sys; import cobevt_amd.host; from cobevt_amd.host import nuscenes; from cobevt_amd.host.nuscenes import encoder; "
            "bad = [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.')]; assert not bad, bad")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


def test_paired_ksplit_counts():
    """256 .. 512 workgroups where the keys allow it, never more splits than 64-key tiles, no split for a full grid"""
    q25 = ops.tokmap(0, 6, 25, 25, 25, 25)
    assert ops.paired_ksplit(1, 4, q25, ops.tokmap(0, 6, 56, 120, 56, 120)) == 16          # 20 workgroups -> 320
    assert ops.paired_ksplit(2, 4, q25, ops.tokmap(0, 6, 56, 120, 56, 120)) == 12          # 40 -> 480
    assert ops.paired_ksplit(1, 4, q25, ops.tokmap(0, 3, 5, 7, 5, 7)) == 3                 # one tile per camera
    assert ops.paired_ksplit(64, 4, q25, ops.tokmap(0, 6, 56, 120, 56, 120)) is None       # 1280 workgroups
