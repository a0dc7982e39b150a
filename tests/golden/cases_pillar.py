"""The LiDAR pillar cases shared by make_golden_pillar.py (gv21_point_pillar.npz), the tests and tools/pillar_probe.py: model
arguments and procedural voxels.  Inputs and weights are procedural (cobevt_amd.synth) and never stored.

Geometry of the fixture: voxel_size [0.4, 0.4, 4] on a 16 x 16 grid, T = 32 points per pillar, N = 3 agents as record_len [2, 1]
with max_cav 3, P = 300 pillars.  Pillar j of agent a sits in cell ((j + 7 a) * STRIDE) mod (ny nx) with STRIDE coprime to the cell
count, so coordinates are unique per agent without a random permutation; points lie inside their cell, clustered around one spot of it; n_p covers 1, T and the
values between (a fifth of the pillars at n_p = T); rows >= n_p are zero unless `dirty` (the case that pins "the mean sums all T
rows")."""
import copy

import numpy as np
import torch

from cobevt_amd import synth

SEED = 0
VOXEL_SIZE = [0.4, 0.4, 4]
LIDAR_RANGE = [-3.2, -3.2, -3.0, 3.2, 3.2, 1.0]          # 16 x 16 cells of 0.4 m
GRID = (16, 16)                                          # (ny, nx)
T = 32
AGENTS = 3
RECORD_LEN = [2, 1]
MAX_CAV = 3
COUNTS = [100, 100, 100]                                 # pillars per agent: P = 300
STRIDE = 37
# (use_absolute_xyz, with_distance)
COMBOS = [(True, False), (True, True), (False, False), (False, True)]
FUSION = dict(input_dim=64, mlp_dim=128, agent_size=3, window_size=4, dim_head=32, drop_out=0.1, depth=2, mask=True)   # cases.SWAP's shape


def combo_name(use_absolute_xyz, with_distance, use_norm=True):
    return "abs%d_dist%d%s" % (int(use_absolute_xyz), int(with_distance), "" if use_norm else "_nonorm")


def vfe_cfg(use_absolute_xyz=True, with_distance=False, use_norm=True):
    return dict(use_norm=use_norm, with_distance=with_distance, use_absolute_xyz=use_absolute_xyz, num_filters=[64])


def lidar_range(ny, nx, voxel_size=VOXEL_SIZE):
    """a range centred on the origin that gives an ny x nx grid"""
    return [-0.5 * nx * voxel_size[0], -0.5 * ny * voxel_size[1], -3.0, 0.5 * nx * voxel_size[0], 0.5 * ny * voxel_size[1], 1.0]


def model_args(use_absolute_xyz=True, with_distance=False, use_norm=True, grid=GRID, max_cav=MAX_CAV, fusion=None):
    ny, nx = grid
    return dict(voxel_size=list(VOXEL_SIZE), lidar_range=lidar_range(ny, nx), max_cav=max_cav,
                pillar_vfe=vfe_cfg(use_absolute_xyz, with_distance, use_norm),
                point_pillar_scatter=dict(num_features=64, grid_size=[nx, ny, 1]),
                fax_fusion=copy.deepcopy(FUSION if fusion is None else fusion))


def voxels(counts=COUNTS, t=T, grid=GRID, seed=SEED, dirty=False, stride=STRIDE, tag="gv21"):
    """-> {voxel_features (P, t, 4) fp32, voxel_coords (P, 4) int32 [n, z, y, x], voxel_num_points (P,) int32}, agent-major as
    OpenCOOD's collate concatenates the agents' voxels"""
    ny, nx = grid
    cells = ny * nx
    assert np.gcd(stride, cells) == 1 and max(counts) <= cells
    rng = lidar_range(ny, nx)
    p = int(sum(counts))
    agent = np.concatenate([np.full(c, a, dtype=np.int64) for a, c in enumerate(counts)]) if p else np.zeros(0, dtype=np.int64)
    j = np.concatenate([np.arange(c, dtype=np.int64) for c in counts]) if p else np.zeros(0, dtype=np.int64)
    cell = ((j + 7 * agent) * stride) % cells
    y, x = cell // nx, cell % nx
    i = np.arange(p)
    u = synth.procedural_input(tag + ".np", (max(p, 1),), seed, 0.0, 1.0).numpy()[:p]
    n_p = np.where(i % 5 == 0, t, np.where(i % 5 == 1, 1, np.minimum(t - 1, 2 + (u * max(t - 2, 1)).astype(np.int64))))
    n_p = np.clip(n_p, 1, t)
    # a pillar's points cluster around one spot of its cell (a surface hit), +-7.5 % of the cell around it: with points spread over the
    # whole cell the layer's response changes sign from row to row and the masked rows' relu(shift) rarely wins the maximum
    r = synth.procedural_input(tag + ".pts", (max(p, 1), t, 4), seed, 0.0, 1.0).numpy()[:p].astype(np.float64)
    c = synth.procedural_input(tag + ".spot", (max(p, 1), 1, 3), seed, 0.0, 1.0).numpy()[:p].astype(np.float64)
    frac = 0.1 + 0.8 * c + 0.15 * (r[..., :3] - 0.5)                      # inside (0.025, 0.975) of the cell
    pts = np.empty((p, t, 4), dtype=np.float64)
    pts[..., 0] = rng[0] + (x[:, None] + frac[..., 0]) * VOXEL_SIZE[0]
    pts[..., 1] = rng[1] + (y[:, None] + frac[..., 1]) * VOXEL_SIZE[1]
    pts[..., 2] = rng[2] + frac[..., 2] * VOXEL_SIZE[2]
    pts[..., 3] = r[..., 3]
    if not dirty:
        pts[np.arange(t)[None, :] >= n_p[:, None]] = 0.0
    coords = np.stack([agent, np.zeros_like(agent), y, x], axis=1)
    return {"voxel_features": torch.from_numpy(pts.astype(np.float32)),
            "voxel_coords": torch.from_numpy(coords.astype(np.int32)).reshape(p, 4),
            "voxel_num_points": torch.from_numpy(n_p.astype(np.int32))}


def build(modules, args):
    """modules: a namespace with PillarVFE, PointPillarScatter, SwapFusionEncoder (the reference's classes or cobevt_amd.host's) ->
    (pillar_vfe, scatter, fusion_net) in eval mode - the three children of PointPillarFuseBEVT, under its attribute names"""
    vfe = modules.PillarVFE(copy.deepcopy(args["pillar_vfe"]), 4, args["voxel_size"], args["lidar_range"]).eval()
    sc = modules.PointPillarScatter(copy.deepcopy(args["point_pillar_scatter"])).eval()
    fn = modules.SwapFusionEncoder(copy.deepcopy(args["fax_fusion"])).eval()
    return vfe, sc, fn

