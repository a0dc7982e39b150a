"""Generate gv30_detector_train.npz and gv30_att_fuse_bwd_d32.json: the REFERENCE's AttBEVBackbone and BaseBEVBackbone in .train() mode,
in double, on the CPU, in the build container like make_golden.py:

    python tests/golden/make_golden_detector_train.py

Both run att_backbone_ref.GOLDEN_CFG with procedural parameters (synth.fill_module_, seed 0) on a procedural input of
att_backbone_ref.INPUT_SHAPE / RECORD_LEN at amplitude 2 (BaseBEVBackbone takes the five maps as five samples).  Recorded per
backbone ("att/", "base/"): the output, the running statistics and num_batches_tracked after the step, every parameter's gradient and
the input's gradient of sum(out * w) for the procedural w of detector_train_ref.loss_weight.  A tensor of more than SAMPLE_CAP elements
is recorded as detector_train_ref.sample() takes it (every ceil(numel / SAMPLE_CAP)-th element): the whole tensors are compared HERE,
where the reference is, to 1e-9, and the test replays the restatement against the recorded elements.

Asserted on the spot: the restatement (detector_train_ref.backbone) agrees with the reference to 1e-9 in every recorded quantity; the
fp32 and the float64 restatement cut the same pre-activations (0 mask disagreements); between 10 % and 90 % of the outputs are cut by
the ReLU.

The json: per attention case (detector_train_ref.att_cases) the max-norm deviation of fp32 autograd from float64 autograd of
att_backbone_ref.att_fusion and max |dx|, what the kernel's gate is made of."""
import copy
import json
import os
import sys

import numpy as np
import torch

import make_golden as mg                      # first: puts the repository, this directory and the stand-ins in place
from cobevt_amd.synth import fill_module_, procedural_input

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import att_backbone_ref as ar  # noqa: E402
import detector_train_ref as dr  # noqa: E402

from opencood.models.backbones.att_bev_backbone import AttBEVBackbone as R_AttBEVBackbone  # noqa: E402
from opencood.models.backbones.base_bev_backbone import BaseBEVBackbone as R_BaseBEVBackbone  # noqa: E402


def _same(name, got, want, tol=1e-9):
    err = float((got.double() - want.double()).abs().max())
    scale = float(want.double().abs().max())
    assert err <= tol * max(1.0, scale), "%s: restatement %.3e away from the reference (scale %.3e)" % (name, err, scale)
    return err


def one(tag, cls, record_len):
    x = procedural_input("gv26.spatial_features", ar.INPUT_SHAPE, 0, -ar.AMPLITUDE, ar.AMPLITUDE)
    model = fill_module_(cls(copy.deepcopy(ar.GOLDEN_CFG), ar.INPUT_CHANNELS), 0).double().train()
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    xi = x.double().clone().requires_grad_(True)
    data = {"spatial_features": xi}
    if record_len is not None:
        data["record_len"] = torch.tensor(record_len)
    want = model(data)["spatial_features_2d"]
    w = dr.loss_weight(tuple(want.shape))
    (want * w).sum().backward()
    got = dr.run(sd0, ar.GOLDEN_CFG, x, record_len, torch.float64, weight=w)
    worst = _same(tag + " output", got["out"], want.detach())
    worst = max(worst, _same(tag + " dx", got["dx"], xi.grad))
    grads = dict(model.named_parameters())
    assert set(got["grads"]) == set(grads)
    for k, p in grads.items():
        worst = max(worst, _same(tag + " grad " + k, got["grads"][k], p.grad))
    sd1 = model.state_dict()
    for prefix, (rm, rv) in got["tape"].running.items():
        worst = max(worst, _same(tag + " " + prefix + "running_mean", rm, sd1[prefix + "running_mean"]))
        worst = max(worst, _same(tag + " " + prefix + "running_var", rv, sd1[prefix + "running_var"]))
        assert int(sd1[prefix + "num_batches_tracked"]) == 1
    r32 = dr.run(sd0, ar.GOLDEN_CFG, x, record_len, torch.float32)
    dis = dr.mask_disagreements(got["tape"], r32["tape"])
    pre = sum(int(a.numel()) for a in got["tape"].pre)
    zero = float((want == 0).double().mean())
    print("  %-5s restatement within %.2e of the reference; %d BatchNorm layers, %d pre-activations, %d fp32 / float64 mask disagreements; "
          "%.0f %% of the outputs cut by the ReLU" % (tag, worst, len(got["tape"].pre), pre, dis, 100 * zero))
    assert dis == 0 and 0.1 <= zero <= 0.9 and len(got["tape"].pre) == 9
    out = {tag + "/output": dr.sample(want).numpy(), tag + "/dx": dr.sample(xi.grad).numpy(),
           tag + "/output_shape": np.array(want.shape)}
    for k, p in grads.items():
        out["%s/grad/%s" % (tag, k)] = dr.sample(p.grad).numpy()
    for k, v in sd1.items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            out["%s/after/%s" % (tag, k)] = v.numpy()
    return out


def att_gates():
    table = {}
    for name, x, rl in dr.att_cases():
        d32, scale = dr.att_bwd_d32(x, rl, dr.att_dout(x, rl))
        table[name] = {"d32": float("%.4e" % d32), "max_dx": float("%.4e" % scale)}
        print("  att_fuse_bwd %-28s d32 %.3e  max|dx| %.3e  -> gate %.3e (relative)" % (name, d32, scale, 4 * d32 / scale))
    with open(dr.ATT_BWD_D32_FILE, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    torch.set_grad_enabled(True)            # (make_golden switches it off for its own, forward-only, cases)
    out = one("att", R_AttBEVBackbone, ar.RECORD_LEN)
    out.update(one("base", R_BaseBEVBackbone, None))
    mg.save("gv30_detector_train", **out)
    att_gates()
