"""Sequential numpy restatement of the 3-D voxeliser's specification (spconv's points_to_voxel with OpenCOOD's collate on an
(nx, ny, nz) grid), in fp32 arithmetic: the yardstick of tests/test_voxelize3d.py and tests/test_voxelize3d_gpu.py.

The rules are voxel_ref.py's - its cell_of, range_keep and ego_keep are the ones used here - with the cell now (z, y, x): per agent, in
input order, a point is dropped when a coordinate is not finite, when the optional masks remove it or when floor((p - lo) / v) is
outside [0, nx) x [0, ny) x [0, nz); the first kept point of a cell opens a voxel, voxels are numbered in order of their first point,
at most max_voxels per agent (cells that would open another are dropped with all their points; open cells keep accepting points); a
voxel keeps the first T points of its cell.  Outputs have N * max_voxels rows, agent a's from row a * max_voxels, voxel_coords
[a, z, y, x]; rows without a voxel: voxel_coords [-1, 0, 0, 0], voxel_num_points 0 (their features are zero HERE; the operator does not
write them)."""
import numpy as np

from voxel_ref import cell_of, ego_keep, grid_size, range_keep


def classify(points, lidar_range, voxel_size, range_mask=False, ego_mask=False):
    """-> keep (M,) bool, z (M,), y (M,), x (M,) int64 (0 where dropped)"""
    p = np.asarray(points, dtype=np.float32)
    nx, ny, nz = grid_size(lidar_range, voxel_size)
    keep = np.isfinite(p[:, 0]) & np.isfinite(p[:, 1]) & np.isfinite(p[:, 2])
    if range_mask:
        keep &= range_keep(p, lidar_range)
    if ego_mask:
        keep &= ego_keep(p)
    c = cell_of(p, lidar_range, voxel_size)
    with np.errstate(invalid="ignore"):
        keep &= (c[:, 0] >= 0) & (c[:, 0] < nx) & (c[:, 1] >= 0) & (c[:, 1] < ny) & (c[:, 2] >= 0) & (c[:, 2] < nz)
    x, y, z = (np.where(keep, c[:, j], 0).astype(np.int64) for j in range(3))
    return keep, z, y, x


def _empty(n, t, max_voxels):
    pcap = n * max_voxels
    coords = np.zeros((pcap, 4), dtype=np.int32)
    coords[:, 0] = -1
    return {"voxel_features": np.zeros((pcap, t, 4), dtype=np.float32), "voxel_coords": coords,
            "voxel_num_points": np.zeros(pcap, dtype=np.int32), "num_voxels": np.zeros(n, dtype=np.int32),
            # not part of the operator's output: the full point count of each voxel's cell, and per agent the cells the cap dropped
            "cell_count": np.zeros(pcap, dtype=np.int64), "dropped_cells": [set() for _ in range(n)]}


def voxelize(points, offsets, lidar_range, voxel_size, max_points, max_voxels, range_mask=False, ego_mask=False):
    """the literal per-point loop with a dict keyed on (z, y, x)"""
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(-1, 4)
    offsets = [int(o) for o in offsets]
    n, t = len(offsets) - 1, int(max_points)
    keep, zs, ys, xs = classify(p, lidar_range, voxel_size, range_mask, ego_mask)
    out = _empty(n, t, max_voxels)
    vf, coords, npts, cnt = out["voxel_features"], out["voxel_coords"], out["voxel_num_points"], out["cell_count"]
    for a in range(n):
        row_of = {}
        base = a * max_voxels
        for i in range(offsets[a], offsets[a + 1]):
            if not keep[i]:
                continue
            cell = (int(zs[i]), int(ys[i]), int(xs[i]))
            row = row_of.get(cell)
            if row is None:
                if len(row_of) >= max_voxels:
                    out["dropped_cells"][a].add(cell)
                    continue
                row = base + len(row_of)
                row_of[cell] = row
                coords[row] = (a,) + cell
            cnt[row] += 1
            if npts[row] < t:
                vf[row, npts[row]] = p[i]
                npts[row] += 1
        out["num_voxels"][a] = len(row_of)
    return out


def voxelize_fast(points, offsets, lidar_range, voxel_size, max_points, max_voxels, range_mask=False, ego_mask=False):
    """the same result, vectorised per agent with a stable argsort on the 3-D cell index (z ny + y) nx + x (pinned to `voxelize` by
    tests/test_voxelize3d.py)"""
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(-1, 4)
    offsets = [int(o) for o in offsets]
    n, t = len(offsets) - 1, int(max_points)
    nx, ny, nz = grid_size(lidar_range, voxel_size)
    keep, zs, ys, xs = classify(p, lidar_range, voxel_size, range_mask, ego_mask)
    out = _empty(n, t, max_voxels)
    for a in range(n):
        idx = np.arange(offsets[a], offsets[a + 1])[keep[offsets[a]:offsets[a + 1]]]
        if idx.size == 0:
            continue
        cell = (zs[idx] * ny + ys[idx]) * nx + xs[idx]
        order = np.argsort(cell, kind="stable")                       # groups the cells, input order inside each
        sc, si = cell[order], idx[order]
        starts = np.flatnonzero(np.r_[True, sc[1:] != sc[:-1]])
        counts = np.diff(np.r_[starts, sc.size])
        first = si[starts]                                            # the first point of every cell
        rank = np.argsort(first, kind="stable")                       # cells in order of first appearance
        kept, dropped = rank[:max_voxels], rank[max_voxels:]
        out["dropped_cells"][a] = {(int(c) // (nx * ny), int(c) // nx % ny, int(c) % nx) for c in sc[starts[dropped]]}
        rows = a * max_voxels + np.arange(kept.size)
        kc = sc[starts[kept]]
        out["num_voxels"][a] = kept.size
        out["voxel_coords"][rows, 0] = a
        out["voxel_coords"][rows, 1] = kc // (nx * ny)
        out["voxel_coords"][rows, 2] = kc // nx % ny
        out["voxel_coords"][rows, 3] = kc % nx
        out["cell_count"][rows] = counts[kept]
        n_p = np.minimum(counts[kept], t)
        out["voxel_num_points"][rows] = n_p
        for s in range(t):
            has = n_p > s
            out["voxel_features"][rows[has], s] = p[si[starts[kept][has] + s]]
    return out
