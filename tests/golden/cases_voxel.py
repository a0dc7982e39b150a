"""The voxeliser's cases shared by make_golden_voxel.py (gv23_voxel.npz), tests/test_voxelize.py, tests/test_voxelize_gpu.py and
tools/voxel_probe.py: procedural point clouds (cobevt_amd.synth; never stored) with a fixed shuffle.  All geometry uses voxel_size
0.4 - not representable in fp32 - on grids centred on the origin, z range [-3, 1] with one voxel over the height."""
import numpy as np

from cobevt_amd import synth

VOXEL_SIZE = [0.4, 0.4, 4]
GOLDEN_GRID = (32, 32)                                   # (ny, nx) of the golden cloud
EGO_EDGES = (-1.95, 2.95, -1.1, 1.1)                     # pcd_utils.mask_ego_points' box: x0, x1, y0, y1


def lidar_range(ny, nx):
    return [-0.5 * nx * VOXEL_SIZE[0], -0.5 * ny * VOXEL_SIZE[1], -3.0, 0.5 * nx * VOXEL_SIZE[0], 0.5 * ny * VOXEL_SIZE[1], 1.0]


def preprocess_params(grid, max_points=32, max_voxel_train=None, max_voxel_test=None, **extra):
    """SpVoxelPreprocessor's arguments (OpenCOOD's `preprocess` section) for an (ny, nx) grid centred on the origin"""
    ny, nx = grid
    cells = ny * nx
    args = dict(voxel_size=list(VOXEL_SIZE), max_points_per_voxel=max_points, max_voxel_train=max_voxel_train or cells,
                max_voxel_test=max_voxel_test or cells)
    return dict(core_method="SpVoxelPreprocessor", args=args, cav_lidar_range=lidar_range(ny, nx), **extra)


def uniform(tag, shape, seed=0):
    return synth.procedural_input("voxel." + tag, shape, seed, 0.0, 1.0).numpy().astype(np.float64)


def permutation(tag, n, seed=0):
    """a fixed permutation of n: the order of n procedural keys"""
    return np.argsort(uniform(tag + ".perm", (max(n, 1),), seed)[:n], kind="stable")


def points_in_cells(tag, ys, xs, grid, seed=0, margin=0.05):
    """one point inside each listed cell (ys[i], xs[i]), away from the cell's edges by `margin` of its size -> (n, 4) fp32"""
    ny, nx = grid
    rng = lidar_range(ny, nx)
    n = len(ys)
    u = uniform(tag, (max(n, 1), 4), seed)[:n]
    f = margin + (1.0 - 2.0 * margin) * u[:, :3]
    pts = np.empty((n, 4), dtype=np.float64)
    pts[:, 0] = rng[0] + (np.asarray(xs) + f[:, 0]) * VOXEL_SIZE[0]
    pts[:, 1] = rng[1] + (np.asarray(ys) + f[:, 1]) * VOXEL_SIZE[1]
    pts[:, 2] = rng[2] + f[:, 2] * VOXEL_SIZE[2]
    pts[:, 3] = u[:, 3]
    return pts.astype(np.float32)


def cloud_from_counts(tag, counts, grid, seed=0):
    """counts (ny * nx,): points per cell -> the cell's points, shuffled by a fixed permutation, (sum, 4) fp32"""
    ny, nx = grid
    cell = np.repeat(np.arange(ny * nx), np.asarray(counts, dtype=np.int64))
    pts = points_in_cells(tag, cell // nx, cell % nx, grid, seed)
    return pts[permutation(tag, len(cell), seed)]


def concat(clouds):
    """-> (points (M, 4) fp32, offsets (N + 1,) int32)"""
    offs = np.cumsum([0] + [len(c) for c in clouds]).astype(np.int32)
    pts = np.concatenate(clouds).astype(np.float32) if len(clouds) else np.zeros((0, 4), dtype=np.float32)
    return np.ascontiguousarray(pts.reshape(-1, 4)), offs


# ---- 1. counts: 5 x 7 cells, 3 agents, about 3 000 points per agent
COUNTS_GRID = (5, 7)
COUNTS_REQUIRED = [1, 31, 32, 33, 64, 65, 250]


def counts_case():
    ny, nx = COUNTS_GRID
    clouds = []
    for a in range(3):
        rest = [150 + 3 * j + a for j in range(14)] + [2 + (5 * j + 3 * a) % 29 for j in range(14)]
        per_cell = np.roll(np.array(COUNTS_REQUIRED + rest, dtype=np.int64), 11 * a)
        assert per_cell.size == ny * nx
        clouds.append(cloud_from_counts("counts.%d" % a, per_cell, COUNTS_GRID))
    return concat(clouds) + (lidar_range(ny, nx),)


# ---- 2. the voxel cap: 16 x 16 cells, max_voxels 40; agents 0 and 2 open more cells than that, agent 1 fewer
CAP_GRID = (16, 16)
CAP_MAX_VOXELS = 40


def cap_case():
    ny, nx = CAP_GRID
    clouds = []
    for a, cells in enumerate([100, 25, 60]):
        per_cell = np.zeros(ny * nx, dtype=np.int64)
        which = (np.arange(cells) * 37 + 5 * a) % (ny * nx)
        per_cell[which] = 1 + (np.arange(cells) * 7 + a) % 6
        clouds.append(cloud_from_counts("cap.%d" % a, per_cell, CAP_GRID))
    return concat(clouds) + (lidar_range(ny, nx),)


# ---- 3. scan seams: 70 000 points on 24 x 24 cells, agents of 33 333 / 0 / 36 667 points
SEAM_GRID = (24, 24)
SEAM_OFFSETS = [0, 33333, 33333, 70000]


def seam_case():
    ny, nx = SEAM_GRID
    m = SEAM_OFFSETS[-1]
    u = uniform("seam.cell", (m,))
    # a few cells hold most of the points (near the sensor), the others a few each
    cell = np.where(u < 0.5, (u * 2 * 12).astype(np.int64) * 47 % (ny * nx), (u * 7919).astype(np.int64) % (ny * nx))
    pts = points_in_cells("seam", cell // nx, cell % nx, SEAM_GRID)
    return pts, np.array(SEAM_OFFSETS, dtype=np.int32), lidar_range(ny, nx)


# ---- 4. edges: the golden cloud
def golden_cloud():
    """(M, 4) fp32: a box somewhat larger than the range filled uniformly, plus points exactly on each of the six range faces and on
    each of the four edges of the ego box, with their fp32 neighbours on either side"""
    ny, nx = GOLDEN_GRID
    rng = lidar_range(ny, nx)
    n = 1500
    u = uniform("golden", (n, 4))
    lo, hi = np.array(rng[:3]) - [1.2, 1.2, 0.7], np.array(rng[3:]) + [1.2, 1.2, 0.7]
    pts = np.empty((n, 4), dtype=np.float32)
    pts[:, :3] = (lo + (hi - lo) * u[:, :3]).astype(np.float32)
    pts[:, 3] = u[:, 3]
    # a third of them near the ego vehicle, so that the box has points inside and around it
    near = np.arange(n) % 3 == 0
    pts[near, 0] = (-3.0 + 7.0 * u[near, 0]).astype(np.float32)
    pts[near, 1] = (-2.0 + 4.0 * u[near, 1]).astype(np.float32)
    pts[near, 2] = (-2.5 + 3.0 * u[near, 2]).astype(np.float32)
    special = []
    inner = uniform("golden.inner", (64, 4))
    k = 0
    for axis in range(3):
        for bound in (rng[axis], rng[3 + axis]):
            b = np.float32(bound)
            for val in (np.nextafter(b, np.float32(-np.inf)), b, np.nextafter(b, np.float32(np.inf))):
                p = (np.array(rng[:3]) + (0.1 + 0.8 * inner[k, :3]) * (np.array(rng[3:]) - np.array(rng[:3]))).astype(np.float32)
                p[axis] = val
                special.append([p[0], p[1], p[2], np.float32(inner[k, 3])])
                k += 1
    for axis, bound, other in ((0, EGO_EDGES[0], (EGO_EDGES[2], EGO_EDGES[3])), (0, EGO_EDGES[1], (EGO_EDGES[2], EGO_EDGES[3])),
                               (1, EGO_EDGES[2], (EGO_EDGES[0], EGO_EDGES[1])), (1, EGO_EDGES[3], (EGO_EDGES[0], EGO_EDGES[1]))):
        b = np.float32(bound)
        for val in (np.nextafter(b, np.float32(-np.inf)), b, np.nextafter(b, np.float32(np.inf))):
            p = np.zeros(3, dtype=np.float32)
            p[axis] = val
            p[1 - axis] = np.float32(other[0] + (0.1 + 0.8 * inner[k, 0]) * (other[1] - other[0]))
            p[2] = np.float32(-2.0 + 2.5 * inner[k, 2])
            special.append([p[0], p[1], p[2], np.float32(inner[k, 3])])
            k += 1
    pts = np.concatenate([pts, np.array(special, dtype=np.float32)])
    return np.ascontiguousarray(pts[permutation("golden", len(pts))])


def reciprocal_sensitive(lo, v, n_cells):
    """fp32 coordinates p inside the grid for which floor(fl(fl(p - lo) / v)) and floor(fl(fl(p - lo) * fl(1 / v))) differ: a kernel
    that multiplies by a reciprocal puts these points into the neighbouring cell"""
    lo, v = np.float32(lo), np.float32(v)
    rcp = np.float32(1.0) / v
    k = np.arange(1, n_cells, dtype=np.float64)
    base = (np.float64(lo) + k * np.float64(v)).astype(np.float32)
    cands = [base]
    for _ in range(6):
        cands.append(np.nextafter(cands[-1], np.float32(np.inf)))
    down = base
    for _ in range(6):
        down = np.nextafter(down, np.float32(-np.inf))
        cands.append(down)
    p = np.unique(np.concatenate(cands))
    d = p - lo
    differ = np.floor(d / v) != np.floor(d * rcp)
    return p[differ]


def edge_case():
    """the golden cloud + NaN / inf coordinates + points on lo, on hi and on interior cell edges + reciprocal-sensitive points, as two
    agents -> (points, offsets, range, the reciprocal-sensitive x and y values present)"""
    ny, nx = GOLDEN_GRID
    rng = lidar_range(ny, nx)
    g = golden_cloud()
    extra = []
    mid = [0.3, -0.7, -1.0, 0.5]
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            p = list(mid)
            p[axis] = bad
            extra.append(p)
    extra.append([0.3, -0.7, -1.0, np.nan])                                # a NaN intensity is data, not a coordinate: kept
    for axis, n_cells in ((0, nx), (1, ny)):
        for kcell in (0, 1, n_cells // 2, n_cells - 1, n_cells):           # lo, interior edges, hi
            p = list(mid)
            p[axis] = float(np.float32(rng[axis] + kcell * VOXEL_SIZE[axis]))
            extra.append(p)
    extra.append([mid[0], mid[1], rng[2], 0.25])                           # z on lo: kept by the cell test
    extra.append([mid[0], mid[1], rng[5], 0.25])                           # z on hi: dropped
    sx = reciprocal_sensitive(rng[0], VOXEL_SIZE[0], nx)
    sy = reciprocal_sensitive(rng[1], VOXEL_SIZE[1], ny)
    for j, x in enumerate(sx):
        extra.append([float(x), -5.0 + 0.37 * (j % 27), -1.0, 0.5])
    for j, y in enumerate(sy):
        extra.append([-5.0 + 0.37 * (j % 27), float(y), -1.0, 0.5])
    extra = np.array(extra, dtype=np.float32)
    allp = np.concatenate([g, extra])
    allp = allp[permutation("edge", len(allp))]
    half = len(allp) // 2 + 3
    pts, offs = concat([allp[:half], allp[half:]])
    return pts, offs, rng, sx, sy


# ---- 7. full size: 8 agents x 65 536 points on 256 x 256 cells
FULL_GRID = (256, 256)
FULL_AGENTS = 8
FULL_POINTS = 65536
FULL_MAX_VOXELS = 32000


def full_case():
    """a LiDAR-like density: a third of each agent's points in the few hundred cells around its sensor, the rest spread out"""
    ny, nx = FULL_GRID
    m = FULL_AGENTS * FULL_POINTS
    u = uniform("full.cell", (m, 2))
    agent = np.arange(m) // FULL_POINTS
    cx, cy = 40 + 25 * agent, 200 - 20 * agent
    near = u[:, 0] < 1.0 / 3.0
    r = (u[:, 0] * 3.0) ** 2 * 12.0
    ang = 2.0 * np.pi * u[:, 1]
    x = np.where(near, np.clip(cx + r * np.cos(ang), 0, nx - 1), u[:, 0] * nx).astype(np.int64) % nx
    y = np.where(near, np.clip(cy + r * np.sin(ang), 0, ny - 1), u[:, 1] * ny).astype(np.int64) % ny
    pts = points_in_cells("full", y, x, FULL_GRID)
    offs = (np.arange(FULL_AGENTS + 1) * FULL_POINTS).astype(np.int32)
    return pts, offs, lidar_range(ny, nx)
