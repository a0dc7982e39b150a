"""Generate gv31_hgt.npz by running the REFERENCE's base_transformer.py classes on the CPU, in the build container like make_golden.py:

    python tests/golden/make_golden_hgt.py

The file holds no weights: they are procedural (tests/hgt_ref.fill_hgt_: synth.fill_module_, then the relation matrices at unit gain per
32 x 32 block - with xavier's, or with the plain fill, the scores sit near 0 and the softmax is a mean).  Per module case of
hgt_ref.MODULE_CASES (`d64`: dim 64, 2 heads, T = 2, B = 2, L = 3, 3 x 5 pixels, mixed types, single pixels' keys masked; `d128`: dim 128,
8 heads - inner 256 - T = 3, L = 5, padded agents masked): the inputs, the float64 output of PreNorm(dim, HGTCavAttention)(x, mask,
prior_encoding) + x and of HGTCavAttention alone on x, the state-dict keys with their shapes, and the deviations of the reference's OWN
fp32 run and bf16-autocast run of the layer from its float64 run (max abs; the module gates of tests/test_hgt_gpu.py are multiples of
them) with max |out|.  RTE, RelTemporalEncoding and CavPositionalEncoding: inputs and float64 outputs."""
import json
import os
import sys

import numpy as np
import torch

import make_golden as mg                      # first: puts the repository, this directory and the stand-ins in place

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import hgt_ref as hr  # noqa: E402

from opencood.models import base_transformer as R  # noqa: E402


def _layer(c):
    torch.manual_seed(0)
    return hr.fill_hgt_(R.PreNorm(c["dim"], R.HGTCavAttention(c["dim"], c["heads"], num_types=c["T"], num_relations=c["R"], dim_head=32, dropout=0.1)), 0).eval()


def main():
    out = {}
    with torch.no_grad():
        for name, c in hr.MODULE_CASES.items():
            x, mask, prior, types = hr.module_inputs(name)
            layer = _layer(c)
            keys = {k: list(v.shape) for k, v in layer.fn.state_dict().items()}
            y32 = layer(x, mask=mask, prior_encoding=prior) + x
            with torch.autocast("cpu", dtype=torch.bfloat16):
                y16 = (layer(x, mask=mask, prior_encoding=prior) + x).float()
            layer = layer.double()
            y64 = layer(x.double(), mask=mask.double(), prior_encoding=prior.double()) + x.double()
            a64 = layer.fn(x.double(), mask.double(), prior.double())
            assert bool(torch.isfinite(y64).all())
            d32, d16, top = float((y32.double() - y64).abs().max()), float((y16.double() - y64).abs().max()), float(y64.abs().max())
            print("%-5s max|layer| %.4f  max|attention| %.4f  reference fp32 %.3e  bf16 autocast %.3e" % (name, top, float(a64.abs().max()), d32, d16))
            out.update({name + ".x": x.numpy(), name + ".mask": mask.numpy(), name + ".prior": prior.numpy(), name + ".layer64": y64.numpy(),
                        name + ".attention64": a64.numpy(), name + ".dev": np.array([d32, d16, top]),
                        name + ".keys": np.array(json.dumps(keys))})
        c = hr.RTE_CASE
        x, dts = hr.rte_inputs()
        m = hr.fill_hgt_(R.RTE(c["dim"], c["ratio"]), 0).eval().double()
        out.update({"rte.x": x.numpy(), "rte.dts": dts.numpy(), "rte.out64": m(x.double(), dts).numpy(),
                    "rte.keys": np.array(json.dumps({k: list(v.shape) for k, v in m.state_dict().items()})),
                    "rel.out64": m.emb(x[0, 1].double(), dts[0, 1]).numpy()})
        c = hr.POS_CASE
        x = hr.pos_inputs()
        m = R.CavPositionalEncoding(c["dim"], c["cav_num"]).eval()
        out.update({"pos.x": x.numpy(), "pos.out64": m.double()(x.double()).numpy(),
                    "pos.keys": np.array(json.dumps({k: list(v.shape) for k, v in m.state_dict().items()}))})
    np.savez_compressed(hr.GOLDEN_FILE, **out)
    print("%s: %d bytes" % (os.path.basename(hr.GOLDEN_FILE), os.path.getsize(hr.GOLDEN_FILE)))


if __name__ == "__main__":
    main()
