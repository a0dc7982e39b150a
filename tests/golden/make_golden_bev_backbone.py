"""Generate gv25_base_bev_backbone.npz by running the REFERENCE's BaseBEVBackbone (opencood/models/backbones/base_bev_backbone.py) in
eval mode on the CPU, in the build container like make_golden.py:

    python tests/golden/make_golden_bev_backbone.py

Configuration tests/bev_backbone_ref.GOLDEN_CFG (three levels, layer_strides [2, 2, 2], upsample_strides [1, 2, 4]) on 32 input
channels, input (2, 32, 16, 24).  Weights, BatchNorm affine and BatchNorm running statistics are procedural (synth.fill_module_, seed 0:
running_var in [0.6, 1.4), running_mean in +-0.2, scale in [0.8, 1.2), shift in +-0.1), the input is seeded.  Stored: the state_dict
("sd/<key>"), the input and the reference's spatial_features_2d.  The test-side restatement (bev_backbone_ref.mirror) is checked
against the reference on the spot, and so is that a tenth of the outputs at least sit on either side of the ReLU.

The reference's upsample_strides < 1 branch calls np.int, which current numpy does not have: that branch is not in the fixture (the
tests pin it against the mirror instead).  Also prints the deviations d32 / d16 the module-level GPU gates are made of."""
import os
import sys

import torch

import make_golden as mg                      # first: puts the repository, this directory and the stand-ins in place
from cobevt_amd.synth import fill_module_, procedural_input

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import bev_backbone_ref as br  # noqa: E402

from opencood.models.backbones.base_bev_backbone import BaseBEVBackbone as R_BaseBEVBackbone  # noqa: E402


def gv25():
    model = fill_module_(R_BaseBEVBackbone(dict(br.GOLDEN_CFG), br.INPUT_CHANNELS), 0).eval()
    x = procedural_input("gv25.spatial_features", br.INPUT_SHAPE, 0, -1.0, 1.0)
    out = model({"spatial_features": x.clone()})["spatial_features_2d"]
    assert tuple(out.shape) == (2, 96, 8, 12) and model.num_bev_features == 96
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    mg._close("BaseBEVBackbone (mirror, fp32)", br.mirror(sd, br.GOLDEN_CFG, x, torch.float32), out, tol=1e-5)
    zero = float((out == 0).float().mean())
    print("  %.0f %% of the outputs are cut by the ReLU, max|out| %.3f" % (100 * zero, float(out.abs().max())))
    assert 0.1 <= zero <= 0.9
    mg.save("gv25_base_bev_backbone", input=mg._np(x), output=mg._np(out), **{"sd/" + k: mg._np(v) for k, v in sd.items()})
    d32, d16, scale = br.deviations(sd, br.GOLDEN_CFG, x)
    print("  golden            d32 %.3e  d16 %.3e  max|out| %.4f  -> gates %.3e / %.3e (relative)" % (d32, d16, scale, 4 * d32 / scale, 4 * d16 / scale))


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    gv25()
