"""DataAugmentor — OpenCOOD's data_utils/augmentor/data_augmentor.py (random world flip / rotation / scaling of a LiDAR cloud and its
ground-truth boxes) on the device: the random parameters are drawn on the host with the reference's own NumPy calls, the arithmetic is
stage 3 of ops.prepare_points (csrc/cloud_prep.hip).

augment_config: the reference's list, e.g. [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']}, {'NAME': 'random_world_rotation',
'WORLD_ROT_ANGLE': [-0.785, 0.785]}, {'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]}].  forward(data_dict) reads
and replaces 'lidar_np' (M, 4) fp32, 'object_bbx_center' (G <= 128, 7) fp32 / fp64 (augmented IN PLACE, as the reference does) and
'object_bbx_mask' (G,), all device tensors; an optional 'point_offsets' (N + 1,) defaults to one agent - the default is built from
host integers with a host-to-device copy on every call, so pass the key when forward is captured in a graph (and draw the parameters
outside the capture: they are host numbers baked into the launches).  Rows with mask == 1 are the
valid boxes: the reference compacts them to the front, which is the same thing whenever the mask is a prefix, and
generate_object_center always produces one.  A plain object without parameters."""
import numpy as np
import torch

from .. import ops
from ..lib import CobevtHipError

_NAMES = ("random_world_flip", "random_world_rotation", "random_world_scaling")


class DataAugmentor(object):
    def __init__(self, augment_config, train=True):
        self.train = train
        self.data_augmentor_queue = []
        for cfg in augment_config:
            name = cfg.get("NAME")
            if name not in _NAMES:
                raise CobevtHipError("DataAugmentor: unknown augmentation %r (supported: %s)" % (name, ", ".join(_NAMES)))
            if name == "random_world_flip" and any(axis not in ("x", "y") for axis in cfg["ALONG_AXIS_LIST"]):
                raise CobevtHipError("DataAugmentor: random_world_flip's ALONG_AXIS_LIST holds 'x' / 'y', got %r" % (cfg["ALONG_AXIS_LIST"],))
            self.data_augmentor_queue.append((name, cfg))

    def draw(self, rng=np.random):
        """The random parameters of one forward, drawn with the reference's calls in queue order (so a seeded generator reproduces the
        reference's parameters): one list entry per queue entry - [(axis, enabled), ...] for a flip, the angle for a rotation, the
        scale for a scaling (None when the range is narrower than 1e-3: global_scaling draws nothing then)."""
        params = []
        for name, cfg in self.data_augmentor_queue:
            if name == "random_world_flip":
                params.append([(axis, bool(rng.choice([False, True], replace=False, p=[0.5, 0.5]))) for axis in cfg["ALONG_AXIS_LIST"]])
            elif name == "random_world_rotation":
                r = cfg["WORLD_ROT_ANGLE"]
                lo, hi = r if isinstance(r, list) else (-r, r)
                params.append(float(rng.uniform(lo, hi)))
            else:
                lo, hi = cfg["WORLD_SCALE_RANGE"]
                params.append(None if hi - lo < 1e-3 else float(rng.uniform(lo, hi)))
        return params

    def worlds(self, params):
        """The `world` dicts of the ops.prepare_points calls of one forward: ONE for a queue in the operator's own order - flip (x
        before y), rotation, scaling, each at most once -, otherwise one per queue entry (per axis for a flip that lists y before x or
        an axis twice: the two flips' heading rules do not commute bitwise), in queue order."""
        if len(params) != len(self.data_augmentor_queue):
            raise CobevtHipError("DataAugmentor: params has %d entries for a queue of %d" % (len(params), len(self.data_augmentor_queue)))
        steps = []
        for (name, _), p in zip(self.data_augmentor_queue, params):
            if name == "random_world_flip":
                axes = [axis for axis, _ in p]
                if axes in ([], ["x"], ["y"], ["x", "y"]):
                    steps.append((0, {"flip_" + axis: bool(on) for axis, on in p}))
                else:
                    steps.extend((-1, {"flip_" + axis: bool(on)}) for axis, on in p)
            elif name == "random_world_rotation":
                steps.append((1, {"rot": float(p)}))
            else:
                steps.append((2, {"scale": None if p is None else float(p)}))
        ranks = [r for r, _ in steps]
        if steps and all(r >= 0 for r in ranks) and all(a < b for a, b in zip(ranks, ranks[1:])):
            merged = {}
            for _, w in steps:
                merged.update(w)
            return [merged]
        return [w for _, w in steps]

    def forward(self, data_dict, params=None):
        if not self.train:
            return data_dict
        if params is None:
            params = self.draw()
        points, boxes, mask = data_dict["lidar_np"], data_dict["object_bbx_center"], data_dict["object_bbx_mask"]
        offsets = data_dict.get("point_offsets")
        if offsets is None:
            offsets = torch.tensor([0, points.shape[0]], dtype=torch.int32, device=points.device)
        call_mask = mask if mask.dtype == boxes.dtype else mask.to(boxes.dtype)
        for world in self.worlds(params):
            points, offsets = ops.prepare_points(points, offsets, world=world, boxes=boxes, box_mask=call_mask)
        data_dict["lidar_np"] = points
        data_dict["object_bbx_center"] = boxes
        data_dict["object_bbx_mask"] = mask
        if "point_offsets" in data_dict:
            data_dict["point_offsets"] = offsets
        return data_dict
