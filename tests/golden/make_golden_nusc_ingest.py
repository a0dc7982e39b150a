"""Generate gv_nusc_ingest.npz by running the REFERENCE's LoadDataTransform.get_cameras / get_bev
(nuscenes/cross_view_transformer/data/transforms.py) with the real Pillow, in the build container like the other make_golden_*.py:

    python tests/golden/make_golden_nusc_ingest.py

Two samples of six cameras each, sources of 45 x 80 ("a") and 37 x 53 ("b"), resized to 14 x 24 with the top 3 rows cut, 12 classes on
a 20 x 20 BEV.  The frames are written as PNGs (lossless) into a temporary directory, the label as the reference's own bit-packed PNG,
the visibility as a PNG and the auxiliary maps as an .npz, as the reference's SaveDataTransform lays them out; sample "b" has no
visibility, aux or pose.  Stored: the inputs and, under `<sample>_out_<key>`, everything the reference returned.

ToTensor is NOT pinned by a real torchvision: torchvision is not installed, _standin_totensor.py restates it (a uint8 image becomes
`.to(float32).div(255)` in (C, H, W) order).  The resize, the crop, the intrinsics and the label unpacking are the reference's and
Pillow's own code.  The generator also asserts that the restatement tests/ingest_ref.py reproduces image and bev exactly."""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference/nuscenes"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _standin_totensor  # noqa: E402

_standin_totensor.install()

import ingest_ref as ir  # noqa: E402

IMAGE_CONFIG = {"h": 11, "w": 24, "top_crop": 3}
NUM_CLASSES = 12
CAMERAS = 6
BEV = 20
SOURCES = {"a": (45, 80), "b": (37, 53)}


def reference_transforms():
    """the reference's data/transforms.py without its package __init__ (which imports the nuScenes devkit)"""
    for name, sub in (("cross_view_transformer", ""), ("cross_view_transformer.data", "data")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REFERENCE, "cross_view_transformer", sub)]
        sys.modules[name] = pkg
    return importlib.import_module("cross_view_transformer.data.transforms")


def inputs(name):
    hs, ws = SOURCES[name]
    rng = np.random.RandomState({"a": 11, "b": 12}[name])
    d = {"images": ir.make_images(100 + ord(name), CAMERAS, hs, ws)}
    intr = np.zeros((CAMERAS, 3, 3))
    intr[:, 0, 0] = rng.uniform(700.0, 1300.0, CAMERAS)
    intr[:, 1, 1] = rng.uniform(700.0, 1300.0, CAMERAS)
    intr[:, 0, 2] = rng.uniform(0.4, 0.6, CAMERAS) * ws
    intr[:, 1, 2] = rng.uniform(0.4, 0.6, CAMERAS) * hs
    intr[:, 2, 2] = 1.0
    d["intrinsics"] = intr
    ext = np.tile(np.eye(4), (CAMERAS, 1, 1))
    ext[:, :3] = rng.standard_normal((CAMERAS, 3, 4))
    d["extrinsics"] = ext
    d["view"] = np.array([[0.0, -2.0, 100.0], [-2.0, 0.0, 100.0], [0.0, 0.0, 1.0]])
    d["cam_ids"] = np.arange(CAMERAS, dtype=np.int64)[::-1].copy()
    d["bev"] = rng.randint(0, 1 << NUM_CLASSES, size=(BEV, BEV)).astype(np.int32)
    if name == "a":
        d["visibility"] = rng.randint(0, 5, size=(BEV, BEV)).astype(np.uint8)
        d["aux"] = rng.standard_normal((BEV, BEV, 4)).astype(np.float32)
        d["pose"] = rng.standard_normal((4, 4))
    return d


def run(R, name, tmp):
    d = inputs(name)
    data_dir, labels_dir = os.path.join(tmp, "data"), os.path.join(tmp, "labels")
    scene = "scene-" + name
    os.makedirs(os.path.join(labels_dir, scene), exist_ok=True)
    os.makedirs(data_dir, exist_ok=True)
    paths = []
    for i, img in enumerate(d["images"]):
        paths.append("%s_cam%d.png" % (name, i))
        Image.fromarray(img).save(os.path.join(data_dir, paths[-1]))
        assert np.array_equal(np.asarray(Image.open(os.path.join(data_dir, paths[-1]))), img)
    extra = {"cam_ids": d["cam_ids"].tolist()}
    Image.fromarray(d["bev"]).save(os.path.join(labels_dir, scene, "bev.png"))
    if "visibility" in d:
        Image.fromarray(d["visibility"]).save(os.path.join(labels_dir, scene, "visibility.png"))
        np.savez_compressed(os.path.join(labels_dir, scene, "aux.npz"), aux=d["aux"])
        extra.update(visibility="visibility.png", aux="aux.npz", pose=d["pose"].tolist())
    sample = R.Sample(token=name, scene=scene, intrinsics=d["intrinsics"].tolist(), extrinsics=d["extrinsics"].tolist(), images=paths,
                      view=d["view"].tolist(), bev="bev.png", **extra)
    t = R.LoadDataTransform(data_dir, labels_dir, IMAGE_CONFIG, NUM_CLASSES)
    out = dict(t.get_cameras(sample, **IMAGE_CONFIG))
    out.update(t.get_bev(sample))
    again = t(sample)
    assert sorted(again) == sorted(out) and all(np.array_equal(np.asarray(again[k]), np.asarray(out[k])) for k in out)
    hr = IMAGE_CONFIG["h"] + IMAGE_CONFIG["top_crop"]
    assert np.array_equal(out["image"].numpy(), ir.resize(d["images"], (IMAGE_CONFIG["w"], hr), IMAGE_CONFIG["top_crop"])), "image"
    assert np.array_equal(out["bev"].numpy(), ir.decode_bev(d["bev"], NUM_CLASSES)), "bev"
    arrays = {"%s_%s" % (name, k): v for k, v in d.items()}
    for k, v in out.items():
        v = v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        arrays["%s_out_%s" % (name, k)] = v
        print("%s %-12s %-8s %s" % (name, k, v.dtype, v.shape))
    return arrays


def main():
    R = reference_transforms()
    arrays = {"image_config": np.array([IMAGE_CONFIG["h"], IMAGE_CONFIG["w"], IMAGE_CONFIG["top_crop"]]), "num_classes": np.array(NUM_CLASSES)}
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(SOURCES):
            arrays.update(run(R, name, tmp))
    path = os.path.join(HERE, "gv_nusc_ingest.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
