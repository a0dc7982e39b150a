"""Generate gv20_nuscenes_cvt.npz by running the REFERENCE's nuScenes CVT (config/model/cvt.yaml: encoder.py Encoder + decoder.py
Decoder + cvt.py CrossViewTransformer) on the config's shapes, in the build container like make_golden.py:

    python tests/golden/make_golden_nusc_cvt.py

Backbone: synth.FeatureMapBackbone with the EfficientNet-B4 reduction_2 / reduction_4 maps of 224 x 480 images; procedural weights
and inputs (cases_nusc_cvt.py).  Stored: encoder output, both logit maps, the state_dict schema and the reference's own
bf16-autocast deviation for this case (make_golden.gv18's method, weight sets 0..3) - the bf16 gate of the tests.  The test-side
oracle composition (cases_nusc_cvt.oracle_model) is checked against the reference on the spot."""
import sys
import types

import numpy as np
import torch

import make_golden as mg                      # (puts the repository, this directory and the stand-ins in place)
import cases_nusc_cvt as cc
from cobevt_amd.synth import FeatureMapBackbone, fill_module_

sys.path.insert(0, "/root/reference/nuscenes")
from cross_view_transformer.model.encoder import Encoder as R_Encoder  # noqa: E402
from cross_view_transformer.model.decoder import Decoder as R_Decoder  # noqa: E402
from cross_view_transformer.model.cvt import CrossViewTransformer as R_CVT  # noqa: E402

REF = types.SimpleNamespace(Encoder=R_Encoder, Decoder=R_Decoder, CrossViewTransformer=R_CVT)


def _model(feats, seed):
    model = fill_module_(cc.build(REF, FeatureMapBackbone(feats)), seed)
    inter = {}
    model.encoder.register_forward_hook(lambda mod, i, o: inter.__setitem__("enc", o))

    def run(image, intr, ext):
        r = dict(model({"image": image, "intrinsics": intr, "extrinsics": ext}))
        r["encoder"] = inter["enc"]
        return r
    return model, run


def gv20():
    c = cc.config()
    feats, image, intr, ext = cc.inputs()
    model, run = _model(feats, cc.SEED)
    ref = run(image, intr, ext)
    sd = model.state_dict()
    got, got_enc = cc.oracle_model(sd, c, feats, intr, ext)
    mg._close("nuScenes CVT Encoder", got_enc, ref["encoder"], tol=1e-5)
    for k in c["outputs"]:
        mg._close("nuScenes CVT CrossViewTransformer[%s]" % k, got[k], ref[k], tol=1e-5)
    out = {"encoder": mg._np(ref["encoder"]), "bev": mg._np(ref["bev"]), "center": mg._np(ref["center"]),
           "keys": np.array(list(sd.keys())), "shapes": np.array([",".join(str(int(d)) for d in v.shape) for v in sd.values()])}
    dev = {}

    def build(seed):
        _, run_s = _model(feats, seed)
        return lambda: run_s(image, intr, ext)
    mg._dev(dev, "nuScenes CVT", build)
    for k, v in dev.items():
        out["bf16_autocast/" + k] = v
    mg.save("gv20_nuscenes_cvt", **out)


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    gv20()
