"""Generate gv27_detect_labels.npz by running the REFERENCE's VoxelPostprocessor.generate_label on the procedural cases of
cases_labels.py, in the build container like make_golden.py:

    python tests/golden/make_golden_labels.py

`bbox_overlaps` is the reference's own opencood/utils/box_overlaps.pyx, compiled here with the installed Cython into a temporary
directory outside the repository (nothing compiled is kept).  If that build fails, an fp32 numpy stand-in with the same operation
order (tests/labels_ref.bbox_overlaps) is installed instead and the README line written by this script says so.

Stored per case are only outputs: the three label arrays of every sample, the reference's fp32 anchor and gt standup boxes (what its
bbox_overlaps was called with: the kernel-level test feeds them to the kernel), and how far the fp32 restatement lies from the
reference (targets, standup boxes) or from the float64 restatement (the loss, which has no reference implementation in the tree):
the GPU tests' gates are 4 x those deviations.  Inputs are procedural and never stored.

For the sample with a non-prefix mask (c5, sample 1) the reference is run on the compacted input - the valid boxes moved to the front
- which is the documented rule; on the input as it stands the reference takes its targets from the wrong box (it indexes the
unfiltered array with the filtered index), and the generator asserts that this really differs."""
import importlib
import os
import shutil
import subprocess
import sys
import tempfile
import types
from unittest import mock

import numpy as np
import torch

import _standin_shapely

_standin_shapely.install()

import make_golden as mg                      # noqa: E402  puts the repository, this directory and the reference on the path
import cases_labels as cl                     # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import labels_ref as lr                       # noqa: E402

REF_PYX = "/root/reference/opv2v/opencood/utils/box_overlaps.pyx"
_BUILD = ("from setuptools import setup, Extension; from Cython.Build import cythonize; import numpy; "
          "setup(script_args=['build_ext', '--inplace'], ext_modules=cythonize([Extension('box_overlaps', ['box_overlaps.pyx'], "
          "include_dirs=[numpy.get_include()])], language_level=3))")


def _reference_bbox_overlaps():
    """-> (bbox_overlaps, how it was obtained, the temporary directory to remove)"""
    tmp = tempfile.mkdtemp(prefix="cobevt_box_overlaps_")
    try:
        shutil.copy(REF_PYX, tmp)
        subprocess.run([sys.executable, "-c", _BUILD], cwd=tmp, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        sys.path.insert(0, tmp)
        fn = importlib.import_module("box_overlaps").bbox_overlaps
        sys.path.remove(tmp)
        return fn, "the reference's box_overlaps.pyx compiled with Cython", tmp
    except Exception as e:                     # noqa: BLE001
        print("box_overlaps.pyx did not build (%s): fp32 numpy stand-in" % (e,))
        return (lambda a, q: lr.bbox_overlaps(a, q, np.float32)), "an fp32 numpy stand-in with the same operation order (the Cython build failed)", tmp


BBOX, BBOX_HOW, _TMP = _reference_bbox_overlaps()
CALLS = []


def _recording(a, q):
    CALLS.append((np.array(a), np.array(q)))
    return BBOX(a, q)


sys.modules["opencood.utils.box_overlaps"] = types.SimpleNamespace(bbox_overlaps=_recording)
for name in ("cv2", "timm", "timm.scheduler", "timm.scheduler.cosine_lr", "open3d", "matplotlib", "matplotlib.pyplot", "matplotlib.cm",
             "tensorboardX"):
    try:
        importlib.import_module(name)
    except Exception:
        sys.modules[name] = mock.MagicMock(name=name)
try:
    importlib.import_module("opencood.visualization.vis_utils")
except Exception:
    sys.modules["opencood.visualization.vis_utils"] = mock.MagicMock(name="vis_utils")

from opencood.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor as R_Post  # noqa: E402


def _reference(post, gt, mask, anchors):
    """the reference on one sample -> its dict and the fp32 standup boxes its bbox_overlaps saw"""
    del CALLS[:]
    out = post.generate_label(gt_box_center=gt.copy(), anchors=anchors.copy(), mask=mask.copy())
    assert len(CALLS) == 1
    return out, CALLS[0][0], CALLS[0][1]


def main():
    out, rows = {}, []
    # the compiled bbox_overlaps is C float arithmetic: the fp32 restatement reproduces its bits
    rng = np.random.RandomState(0)
    a = np.sort(rng.uniform(-30, 30, (5000, 2, 2)).astype(np.float32), axis=1).reshape(5000, 4)        # [x1, y1, x2, y2]
    q = a[:400] + rng.uniform(-1, 1, (400, 4)).astype(np.float32)
    assert np.array_equal(BBOX(np.ascontiguousarray(a), np.ascontiguousarray(q)), lr.bbox_overlaps(a, q, np.float32))
    for name in cl.HOST_CASES + ("T",):
        post = R_Post(cl.anchor_params(name), train=True)
        anchors = post.generate_anchor_box()
        gts, masks = cl.case(name, anchors)
        pos, neg, tgt = [], [], []
        dev_t, dev_s, scale_s = 0.0, 0.0, 0.0
        for b in range(len(gts)):
            gt, mask = gts[b], masks[b]
            prefix = bool(np.array_equal(mask, np.sort(mask)[::-1]))
            ref_raw, ast, gst = _reference(post, gt, mask, anchors)
            if prefix:
                ref = ref_raw
            else:
                ref, ast2, gst2 = _reference(post, *cl.compacted(gt, mask), anchors)
                assert np.array_equal(ast, ast2) and np.array_equal(gst, gst2)
                assert np.array_equal(ref["pos_equal_one"], ref_raw["pos_equal_one"]) and np.array_equal(ref["neg_equal_one"], ref_raw["neg_equal_one"])
                assert np.abs(ref["targets"] - ref_raw["targets"]).max() > 1e-3, "the non-prefix mask does not show"
            if b == 0:
                out[name + "_anchor_standup"] = ast
            else:
                assert np.array_equal(out[name + "_anchor_standup"], ast)
            out["%s_gt_standup_%d" % (name, b)] = gst
            r64 = lr.generate_label(gt, anchors, mask, cl.POS_T, cl.NEG_T, np.float64)
            # the fp32 restatement on the reference's own standup boxes decides exactly as the reference, ties included
            k32 = lr.generate_label(gt, anchors, mask, cl.POS_T, cl.NEG_T, np.float32, anchor_standup=ast, gt_standup=gst)
            for key in ("pos_equal_one", "neg_equal_one"):
                assert np.array_equal(k32[key], ref[key]), (name, b, key)
            dev_t = max(dev_t, cl.rel_dev(k32["targets"], ref["targets"], 1.0))
            s32 = np.concatenate([lr.standup(anchors.reshape(-1, 7).astype(np.float32), np.float32),
                                  lr.standup(gt[mask == 1].astype(np.float32), np.float32).reshape(-1, 4)])
            sref = np.concatenate([ast, gst.reshape(-1, 4)])
            scale_s = max(scale_s, float(np.abs(sref).max()))
            dev_s = max(dev_s, cl.rel_dev(s32, sref, float(np.abs(sref).max())))
            if name != "T":
                cl.conditions(r64)
                for key in ("pos_equal_one", "neg_equal_one"):
                    assert np.array_equal(r64[key], ref[key]), (name, b, key)
                assert np.abs(r64["targets"] - ref["targets"]).max() <= 1e-12, np.abs(r64["targets"] - ref["targets"]).max()
                if name == "c2":
                    weak, pair = cl.c2_designed(r64, anchors)
                    other = lr.generate_label(gt, anchors, mask, cl.POS_T, cl.NEG_T, np.float64, rule="max")
                    assert np.abs(other["targets"] - ref["targets"]).max() > 1e-2, "the max-IoU rule is not told apart"
            else:
                ties = int((np.sort(k32["iou"], axis=0)[-1] == np.sort(k32["iou"], axis=0)[-2]).sum())
                assert ties >= 3, "case T is meant to be tie-heavy, %d of %d gt tie" % (ties, k32["iou"].shape[1])
                print("T: %d of %d gt have an exact fp32 tie for the best anchor" % (ties, k32["iou"].shape[1]))
            pos.append(ref["pos_equal_one"])
            neg.append(ref["neg_equal_one"])
            tgt.append(ref["targets"])
            print("%-3s sample %d: %3d valid gt, %4d positives, %5d negatives of %5d; margins: threshold %.2e best-gap %.2e"
                  % (name, b, int((mask == 1).sum()), int(ref["pos_equal_one"].sum()), int(ref["neg_equal_one"].sum()),
                     ref["pos_equal_one"].size, r64["threshold_margin"], r64["best_gap"]))
        out[name + "_pos"] = np.stack(pos).astype(np.uint8)
        out[name + "_neg"] = np.stack(neg).astype(np.uint8)
        out[name + "_targets"] = np.stack(tgt)
        out[name + "_dev"] = np.array([dev_t, dev_s])
        rows.append("| `%s` targets | %.3e | %.3e (x (\\|ref\\| + 1)) |" % (name, dev_t, cl.gate(dev_t)))
        rows.append("| `%s` standup boxes | %.3e | %.3e (x (\\|ref\\| + %.1f)) |" % (name, dev_s, cl.gate(dev_s), scale_s))
    # ---- the loss: float64 restatement as the yardstick, the fp32 restatement's deviation from it as the measure
    for name in cl.LOSS_CASES:
        psm, rm, tg = cl.loss_inputs(name, out[name + "_pos"], out[name + "_targets"])
        p = out[name + "_pos"].astype(np.float32)
        l64, gp64, gr64 = lr.loss_and_grads(psm, rm, p, tg, dtype=torch.float64, **cl.LOSS_ARGS)
        l32, gp32, gr32 = lr.loss_and_grads(psm, rm, p, tg, dtype=torch.float32, **cl.LOSS_ARGS)
        assert np.isfinite(l64).all() and np.isfinite(gp64).all() and np.isfinite(gr64).all()
        dev = [cl.rel_dev(l32, l64, abs(l64[0])), cl.rel_dev(gp32, gp64, np.abs(gp64).max()), cl.rel_dev(gr32, gr64, np.abs(gr64).max())]
        out["loss_%s_ref" % name] = l64
        out["loss_%s_dev" % name] = np.array(dev)
        print("loss %s: total %.6f conf %.6f reg %.6f; fp32 restatement vs float64: loss %.3e dpsm %.3e drm %.3e"
              % (name, l64[0], l64[1], l64[2], dev[0], dev[1], dev[2]))
        for what, d, sc in (("loss", dev[0], "\\|total\\|"), ("d psm", dev[1], "max\\|d psm\\|"), ("d rm", dev[2], "max\\|d rm\\|")):
            rows.append("| loss on `%s`: %s | %.3e | %.3e (x (\\|ref\\| + %s)) |" % (name, what, d, cl.gate(d), sc))
    mg.save("gv27_detect_labels", **out)
    with open(os.path.join(mg.HERE, "README_gv27.md"), "w") as f:
        f.write(README % {"how": BBOX_HOW, "rows": "\n".join(rows)})
    shutil.rmtree(_TMP, ignore_errors=True)


README = """# gv27_detect_labels.npz

Companion to the table in `README.md` of this directory.  Written by `make_golden_labels.py`; do not edit by hand.

| Fixture | Reference code that produced it |
|---|---|
| `gv27_detect_labels` (`make_golden_labels.py`) | `VoxelPostprocessor.generate_label` (`data_utils/post_processor/voxel_postprocessor.py`) on the cases of `cases_labels.py`, with `bbox_overlaps` = %(how)s.  Per case: `<case>_pos`, `<case>_neg` (B, H, W, A) uint8, `<case>_targets` (B, H, W, 7A) float64, `<case>_anchor_standup` (H W A, 4) and `<case>_gt_standup_<b>` (valid boxes, 4) fp32 - the arguments the reference's `bbox_overlaps` was called with - and `<case>_dev`.  Sample 1 of `c5` has a non-prefix mask: the reference was run on the compacted input (see the generator's docstring).  `loss_<case>_ref`, `loss_<case>_dev`: the float64 restatement of the detection loss (`tests/labels_ref.point_pillar_loss`) on `cases_labels.loss_inputs` - NOT a reference output |

The reference tree ships no detection loss.  `tests/labels_ref.point_pillar_loss` restates upstream OpenCOOD's `PointPillarLoss` from
its published definition; its parity with upstream is unpinned.

Asserted by the generator: the compiled `bbox_overlaps` and the fp32 numpy restatement agree bit for bit on 5000 x 400 random boxes; on
every case, case `T` included, the fp32 restatement fed the reference's standup boxes reproduces the reference's `pos_equal_one` and
`neg_equal_one` exactly; on the host-level cases the float64 restatement does so from its own standup boxes, its targets lie within
1e-12 of the reference's, no IoU lies within 1e-4 of a threshold and every valid gt's best and second-best IoU are at least 1e-4
apart; the designed boxes of `c2` do what they are designed for, and matching a positive anchor to its max-IoU gt instead of the
lowest gt index above the threshold changes the targets by more than 1e-2.

## Gates (`tests/test_detect_targets_gpu.py`)

Label maps and `num_pos` are decisions: exact.  Every other quantity is gated at 4 x the worst deviation of its fp32 restatement
(numpy / torch fp32 on the fp32-rounded inputs) from the reference - for the loss, from the float64 restatement - taken relative to
`|ref|` + the quantity's scale, and never below 4 x 2^-24 (`cases_labels.gate`).  Recorded deviations and the gates they give:

| quantity | fp32 restatement's deviation | gate |
|---|---|---|
%(rows)s
"""


if __name__ == "__main__":
    main()
