"""Sequential numpy restatement of the voxeliser's specification (spconv's points_to_voxel with OpenCOOD's collate), in fp32
arithmetic: the yardstick of tests/test_voxelize.py and tests/test_voxelize_gpu.py.

Per agent, in input order: a point is dropped when a coordinate is not finite, when the optional masks remove it (the strict
inequalities of pcd_utils.mask_points_by_range, the inclusive box of pcd_utils.mask_ego_points; fp32 against the fp32-rounded constants)
or when floor((p - lo) / v) (fp32 subtract and divide) is outside the grid.  The first kept point of a cell opens a voxel, voxels are
numbered in order of their first point, at most max_voxels per agent (cells that would open another are dropped with all their points;
open cells keep accepting points).  A voxel keeps the first T points of its cell.  Outputs have N * max_voxels rows, agent a's from
row a * max_voxels; rows without a voxel: voxel_coords [-1, 0, 0, 0], voxel_num_points 0 (their features are zero HERE; the operator
does not write them)."""
import numpy as np

EGO_BOX = (np.float32(-1.95), np.float32(2.95), np.float32(-1.1), np.float32(1.1))          # x0, x1, y0, y1 (pcd_utils.py:79-80)


def grid_size(lidar_range, voxel_size):
    r, v = np.asarray(lidar_range, dtype=np.float32), np.asarray(voxel_size, dtype=np.float32)
    return tuple(int(g) for g in np.round((r[3:] - r[:3]) / v).astype(np.int64))          # (nx, ny, nz)


def range_keep(points, lidar_range):
    """pcd_utils.mask_points_by_range's mask: strictly inside on all three axes"""
    p, r = np.asarray(points, dtype=np.float32), np.asarray(lidar_range, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (p[:, 0] > r[0]) & (p[:, 0] < r[3]) & (p[:, 1] > r[1]) & (p[:, 1] < r[4]) & (p[:, 2] > r[2]) & (p[:, 2] < r[5])


def ego_keep(points):
    """the points pcd_utils.mask_ego_points keeps: outside the inclusive box"""
    p = np.asarray(points, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return ~((p[:, 0] >= EGO_BOX[0]) & (p[:, 0] <= EGO_BOX[1]) & (p[:, 1] >= EGO_BOX[2]) & (p[:, 1] <= EGO_BOX[3]))


def cell_of(points, lidar_range, voxel_size):
    """floor((p - lo) / v) per axis as fp32 (M, 3)"""
    p, r, v = np.asarray(points, dtype=np.float32), np.asarray(lidar_range, dtype=np.float32), np.asarray(voxel_size, dtype=np.float32)
    with np.errstate(all="ignore"):
        c = np.floor((p[:, :3] - r[None, :3]) / v[None, :])
    assert c.dtype == np.float32
    return c


def classify(points, lidar_range, voxel_size, range_mask=False, ego_mask=False):
    """-> keep (M,) bool, y (M,), x (M,) int64 (0 where dropped)"""
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
    x = np.where(keep, c[:, 0], 0).astype(np.int64)
    y = np.where(keep, c[:, 1], 0).astype(np.int64)
    return keep, y, x


def _empty(n, t, max_voxels):
    pcap = n * max_voxels
    coords = np.zeros((pcap, 4), dtype=np.int32)
    coords[:, 0] = -1
    return {"voxel_features": np.zeros((pcap, t, 4), dtype=np.float32), "voxel_coords": coords,
            "voxel_num_points": np.zeros(pcap, dtype=np.int32), "num_voxels": np.zeros(n, dtype=np.int32),
            # not part of the operator's output: the full point count of each voxel's cell, and per agent the cells the cap dropped
            "cell_count": np.zeros(pcap, dtype=np.int64), "dropped_cells": [set() for _ in range(n)]}


def voxelize(points, offsets, lidar_range, voxel_size, max_points, max_voxels, range_mask=False, ego_mask=False):
    """the literal per-point loop"""
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
    offsets = [int(o) for o in offsets]
    n, t = len(offsets) - 1, int(max_points)
    nx, ny, nz = grid_size(lidar_range, voxel_size)
    assert nz == 1
    keep, ys, xs = classify(p, lidar_range, voxel_size, range_mask, ego_mask)
    out = _empty(n, t, max_voxels)
    vf, coords, npts, cnt = out["voxel_features"], out["voxel_coords"], out["voxel_num_points"], out["cell_count"]
    for a in range(n):
        row_of = {}
        base = a * max_voxels
        for i in range(offsets[a], offsets[a + 1]):
            if not keep[i]:
                continue
            cell = (int(ys[i]), int(xs[i]))
            row = row_of.get(cell)
            if row is None:
                if len(row_of) >= max_voxels:
                    out["dropped_cells"][a].add(cell)
                    continue
                row = base + len(row_of)
                row_of[cell] = row
                coords[row] = (a, 0, cell[0], cell[1])
            cnt[row] += 1
            if npts[row] < t:
                vf[row, npts[row]] = p[i]
                npts[row] += 1
        out["num_voxels"][a] = len(row_of)
    return out


def voxelize_fast(points, offsets, lidar_range, voxel_size, max_points, max_voxels, range_mask=False, ego_mask=False):
    """the same result, vectorised per agent with a stable argsort on the cell index (pinned to `voxelize` by tests/test_voxelize.py)"""
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
    offsets = [int(o) for o in offsets]
    n, t = len(offsets) - 1, int(max_points)
    nx, ny, nz = grid_size(lidar_range, voxel_size)
    assert nz == 1
    keep, ys, xs = classify(p, lidar_range, voxel_size, range_mask, ego_mask)
    out = _empty(n, t, max_voxels)
    for a in range(n):
        idx = np.arange(offsets[a], offsets[a + 1])[keep[offsets[a]:offsets[a + 1]]]
        if idx.size == 0:
            continue
        cell = ys[idx] * nx + xs[idx]
        order = np.argsort(cell, kind="stable")                       # groups the cells, input order inside each
        sc, si = cell[order], idx[order]
        starts = np.flatnonzero(np.r_[True, sc[1:] != sc[:-1]])
        counts = np.diff(np.r_[starts, sc.size])
        first = si[starts]                                            # the first point of every cell
        rank = np.argsort(first, kind="stable")                       # cells in order of first appearance
        kept, dropped = rank[:max_voxels], rank[max_voxels:]
        out["dropped_cells"][a] = {(int(c) // nx, int(c) % nx) for c in sc[starts[dropped]]}
        rows = a * max_voxels + np.arange(kept.size)
        out["num_voxels"][a] = kept.size
        out["voxel_coords"][rows, 0] = a
        out["voxel_coords"][rows, 2] = sc[starts[kept]] // nx
        out["voxel_coords"][rows, 3] = sc[starts[kept]] % nx
        out["cell_count"][rows] = counts[kept]
        n_p = np.minimum(counts[kept], t)
        out["voxel_num_points"][rows] = n_p
        for s in range(t):
            has = n_p > s
            out["voxel_features"][rows[has], s] = p[si[starts[kept][has] + s]]
    return out
