"""Stand-in for `torchvision.transforms` as far as nuscenes/cross_view_transformer/data/transforms.py uses it (ToTensor, Compose), for
make_golden_nusc_ingest.py only: torchvision is not installed in the build container.  ToTensor is written from torchvision's published
behaviour - a PIL image or an (H, W[, C]) array becomes a (C, H, W) tensor, and a uint8 one is converted with
`.to(torch.float32).div(255)` - so the fixture does NOT pin a real torchvision's ToTensor ("parity unpinned" for third-party code);
what it pins is Pillow's resize and crop and the reference's own statements around them.  Also registers empty modules for the
imports of the reference's data package that its transform never calls (cv2, pyquaternion, imgaug)."""
import sys
import types
from unittest import mock

import numpy as np
import torch


class ToTensor(object):
    def __call__(self, pic):
        if isinstance(pic, np.ndarray):
            if pic.ndim == 2:
                pic = pic[:, :, None]
            img = torch.from_numpy(pic.transpose((2, 0, 1))).contiguous()
        else:
            arr = np.array(pic, copy=True)
            if arr.ndim == 2:
                arr = arr[:, :, None]
            img = torch.from_numpy(arr).permute((2, 0, 1)).contiguous()
        if img.dtype == torch.uint8:
            return img.to(dtype=torch.float32).div(255)
        return img


class Compose(object):
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, img):
        for t in self.transforms:
            img = t(img)
        return img


def install():
    tv = sys.modules.get("torchvision")
    if tv is not None and not getattr(tv, "_cobevt_standin", False):
        return                                    # a real torchvision is present; use it
    if tv is None:
        tv = types.ModuleType("torchvision")
        tv._cobevt_standin = True
        sys.modules["torchvision"] = tv
    tr = types.ModuleType("torchvision.transforms")
    tr.ToTensor, tr.Compose = ToTensor, Compose
    tv.transforms = tr
    sys.modules["torchvision.transforms"] = tr
    for name in ("cv2", "pyquaternion", "imgaug", "imgaug.augmenters"):
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = mock.MagicMock(name=name)
