"""Generate gv23_voxel.npz by running the REFERENCE's point masks (opencood/utils/pcd_utils.py mask_points_by_range and
mask_ego_points) on the procedural golden cloud of cases_voxel.py, in the build container like make_golden.py:

    python tests/golden/make_golden_voxel.py

The points are procedural and never stored; stored are only the reference's boolean keep-masks (which rows each function keeps).  The
functions return the kept points, not a mask: each row carries its index as a fifth column, which neither function reads.
pcd_utils imports open3d for reading .pcd files only; where open3d is not importable an empty stand-in module takes its place.
The cloud must put points exactly on each of the six range faces and on each of the four edges of the ego box: asserted here."""
import importlib.util
import sys
import types

import numpy as np

import make_golden as mg                      # first: puts the repository, this directory and the reference on the path
import cases_voxel as cv

if importlib.util.find_spec("open3d") is None:
    sys.modules["open3d"] = types.ModuleType("open3d")

from opencood.utils import pcd_utils  # noqa: E402


def _kept(fn, pts, *args):
    tagged = np.concatenate([pts, np.arange(len(pts), dtype=np.float32)[:, None]], axis=1)
    out = fn(tagged, *args)
    mask = np.zeros(len(pts), dtype=bool)
    mask[out[:, 4].astype(np.int64)] = True
    assert int(mask.sum()) == len(out)
    return mask


def main():
    pts = cv.golden_cloud()
    assert pts.dtype == np.float32 and len(pts) < 2 ** 24
    rng = cv.lidar_range(*cv.GOLDEN_GRID)
    for axis in range(3):
        for bound in (rng[axis], rng[3 + axis]):
            assert bool((pts[:, axis] == np.float32(bound)).any()), "no point on the range face %r of axis %d" % (bound, axis)
    x0, x1, y0, y1 = [np.float32(e) for e in cv.EGO_EDGES]
    in_y, in_x = (pts[:, 1] > y0) & (pts[:, 1] < y1), (pts[:, 0] > x0) & (pts[:, 0] < x1)
    for name, on in (("x0", (pts[:, 0] == x0) & in_y), ("x1", (pts[:, 0] == x1) & in_y), ("y0", (pts[:, 1] == y0) & in_x),
                     ("y1", (pts[:, 1] == y1) & in_x)):
        assert bool(on.any()), "no point on the ego-box edge " + name
    range_keep = _kept(pcd_utils.mask_points_by_range, pts, rng)
    ego_keep = _kept(pcd_utils.mask_ego_points, pts)
    print("golden cloud: %d points; mask_points_by_range keeps %d, mask_ego_points keeps %d"
          % (len(pts), int(range_keep.sum()), int(ego_keep.sum())))
    assert 0 < int(range_keep.sum()) < len(pts) and 0 < int(ego_keep.sum()) < len(pts)
    mg.save("gv23_voxel", range_keep=range_keep, ego_keep=ego_keep, points=np.array(len(pts)))


if __name__ == "__main__":
    main()
