"""pcd_utils — the part of OpenCOOD's utils/pcd_utils.py that has a device form.  mask_ego_points, lidar_project, mask_points_by_range
and projected_lidar_stack are stages of ops.prepare_points (csrc/cloud_prep.hip); shuffle_points becomes a permutation made on the
device and handed to it as `order=`."""
import torch

from ..lib import CobevtHipError


def shuffle_order(point_offsets, num_points, generator=None):
    """A device permutation (num_points,) int32 that shuffles every agent's rows offsets[a] .. offsets[a + 1] within the agent, for
    ops.prepare_points(order=...): the stand-in for pcd_utils.shuffle_points per agent.  It does NOT reproduce NumPy's permutation.
    Rows outside every agent's range (before offsets[0], at or past offsets[N]) are shuffled among themselves.  No host read: a
    stable argsort of agent index + U[0, 1), the uniform numbers drawn in fp32 so that the fp64 sum is exact and never reaches the
    next agent's interval.  generator = a torch.Generator of point_offsets' device (default: the device's global one)."""
    if not point_offsets.is_cuda:
        raise CobevtHipError("shuffle_order: point_offsets must be on a ROCm device; there is no CPU fallback")
    if point_offsets.dim() != 1 or point_offsets.shape[0] < 2 or point_offsets.dtype not in (torch.int32, torch.int64):
        raise CobevtHipError("shuffle_order: point_offsets must be int32 / int64 (N + 1,) with N >= 1 agents, got %s %s"
                             % (point_offsets.dtype, tuple(point_offsets.shape)))
    m, dev = int(num_points), point_offsets.device
    rows = torch.arange(m, device=dev, dtype=point_offsets.dtype)
    agent = torch.bucketize(rows, point_offsets.contiguous(), right=True)
    u = torch.rand(m, device=dev, dtype=torch.float32, generator=generator)
    return torch.argsort(agent.to(torch.float64) + u.to(torch.float64), stable=True).to(torch.int32)
