"""nuScenes data path - mirror of nuscenes/cross_view_transformer/data/transforms.py (Sample, LoadDataTransform) on decoded arrays.

The reference opens a JPEG per camera, resizes it with Pillow's antialiased BILINEAR on one host core, cuts the top rows and calls
ToTensor; here the six decoded frames go to the device as uint8 and ops.resize_pil_bilinear does all of that in one launch, bit for
bit (csrc/image_ingest.hip); the bit-packed BEV label is unpacked by ops.decode_bev.  Disk formats and JPEG decoding stay with the
caller: where the reference's Sample holds paths, this one holds arrays.

Placement: `image`, `bev` (and `center`, `visibility` when they arrive as device tensors) are on the device; `cam_idx`, `intrinsics`,
`extrinsics`, `view` and `pose` are the small host values the reference returns, for the collate function to move.
"""
import numpy as np
import torch

from ... import ops
from ...lib import CobevtHipError


class Sample(dict):
    """the reference's dict with attribute access"""

    def __init__(self, token, scene, intrinsics, extrinsics, images, view, bev, **kwargs):
        super().__init__(**kwargs)
        # identify the sample, as in the reference's save / load
        self.token = token
        self.scene = scene
        self.view = view
        self.bev = bev
        self.images = images
        self.intrinsics = intrinsics
        self.extrinsics = extrinsics

    def __getattr__(self, key):
        return super().__getitem__(key)

    def __setattr__(self, key, val):
        self[key] = val
        return super().__setattr__(key, val)


def _to_device(t, device):
    """a pinned host tensor is copied without blocking, any other host tensor the ordinary way"""
    if t.device == device:
        return t
    return t.to(device, non_blocking=t.device.type == "cpu" and t.is_pinned())


class LoadDataTransform(object):
    """LoadDataTransform(image_config={'h', 'w', 'top_crop'}, num_classes): get_cameras, get_bev and __call__ of the reference.
    sample.images: a list or a stack of (H, W, 3) uint8 tensors (or arrays) of ONE size, host or device; sample.bev: (h, w) int32
    or None; sample.visibility (h, w) uint8, sample.aux (h, w, k) float, sample.pose, sample.view as in the reference.
    device: where the images and labels are processed (default: the device the images are on, or the current ROCm device)."""

    def __init__(self, image_config, num_classes, augment="none", device=None):
        if augment != "none":
            raise CobevtHipError("LoadDataTransform: augment=%r is not supported: 'strong' and 'geometric' are imgaug pipelines "
                                 "(StrongAug, GeometricAug), only 'none' is implemented" % (augment,))
        self.image_config = dict(image_config)
        self.num_classes = int(num_classes)
        self.device = None if device is None else torch.device(device)

    def _device(self, t):
        if self.device is not None:
            return self.device
        return t.device if t.device.type != "cpu" else torch.device("cuda", torch.cuda.current_device())

    def _stack(self, images):
        if isinstance(images, (list, tuple)):
            if len(images) == 0:
                raise CobevtHipError("LoadDataTransform: sample.images is empty")
            images = [torch.as_tensor(im) for im in images]
            if any(tuple(im.shape) != tuple(images[0].shape) for im in images):
                raise CobevtHipError("LoadDataTransform: sample.images must all have one size (one launch resizes them), got %s"
                                     % sorted(set(tuple(im.shape) for im in images)))
            dev = self._device(images[0])
            return torch.stack([_to_device(im, dev) for im in images], 0)
        images = torch.as_tensor(images)
        return _to_device(images, self._device(images))

    def get_cameras(self, sample, h, w, top_crop):
        """Note: as in the reference, intrinsics and extrinsics are passed on as given (the model inverts them)."""
        stack = self._stack(sample.images)
        if stack.dim() != 4 or stack.dtype != torch.uint8 or stack.shape[-1] != 3:
            raise CobevtHipError("LoadDataTransform: sample.images must be (H, W, 3) uint8 frames, got %s %s"
                                 % (stack.dtype, tuple(stack.shape)))
        if len(sample.intrinsics) != stack.shape[0]:
            raise CobevtHipError("LoadDataTransform: %d intrinsics for %d images" % (len(sample.intrinsics), stack.shape[0]))
        height, width = int(stack.shape[1]), int(stack.shape[2])
        h_resize = h + top_crop
        w_resize = w
        image = ops.resize_pil_bilinear(stack.contiguous(), (w_resize, h_resize), top_crop)
        intrinsics = list()
        for I_original in sample.intrinsics:
            # nine numbers per camera, on the host with the reference's own NumPy statements: NumPy's scalar promotion is part of the result
            I = np.float32(I_original)
            I[0, 0] *= w_resize / width
            I[0, 2] *= w_resize / width
            I[1, 1] *= h_resize / height
            I[1, 2] *= h_resize / height
            I[1, 2] -= top_crop
            intrinsics.append(torch.tensor(I))
        return {
            "cam_idx": torch.LongTensor(sample.cam_ids),
            "image": image,
            "intrinsics": torch.stack(intrinsics, 0),
            "extrinsics": torch.tensor(np.float32(sample.extrinsics)),
        }

    def get_bev(self, sample):
        bev = None
        if sample.bev is not None:
            labels = torch.as_tensor(sample.bev)
            if labels.dim() != 2 or labels.dtype != torch.int32:
                raise CobevtHipError("LoadDataTransform: sample.bev must be the bit-packed (h, w) int32 label, got %s %s"
                                     % (labels.dtype, tuple(labels.shape)))
            labels = _to_device(labels, self._device(labels))
            bev = ops.decode_bev(labels.contiguous()[None], self.num_classes)[0]
        result = {
            "bev": bev,
            "view": torch.tensor(sample.view),
        }
        if "visibility" in sample:
            v = sample.visibility
            result["visibility"] = v.to(torch.uint8) if isinstance(v, torch.Tensor) else np.array(v, dtype=np.uint8)
        if "aux" in sample:
            aux = sample.aux
            center = aux[..., 1] if isinstance(aux, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(aux)[..., 1]))
            result["center"] = center.to(torch.float32)[None].contiguous()
        if "pose" in sample:
            result["pose"] = np.float32(sample["pose"])
        return result

    def __call__(self, batch):
        if not isinstance(batch, Sample):
            batch = Sample(**batch)
        result = dict()
        result.update(self.get_cameras(batch, **self.image_config))
        result.update(self.get_bev(batch))
        return result
