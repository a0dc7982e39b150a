"""NumPy restatement of ops.prepare_points (csrc/cloud_prep.hip): stages 1 - 6 and the box rules, every floating-point operation
written out with the operator's association - the projection term by term, never as np.dot (BLAS chooses its own order and may
fuse).  NumPy's element-wise multiply and add are single IEEE operations, so the device result must equal this bit for bit."""
import numpy as np

F32, F64 = np.float32, np.float64
EGO = (F32(-1.95), F32(2.95), F32(-1.1), F32(1.1))          # mask_ego_points' limits, rounded to fp32


def ego_keep(p):
    """keep flags of pcd_utils.mask_ego_points on fp32 points, limits rounded to fp32"""
    x, y = p[:, 0], p[:, 1]
    return ~((x >= EGO[0]) & (x <= EGO[1]) & (y >= EGO[2]) & (y <= EGO[3]))


def range_keep(q, lidar_range):
    """keep flags of pcd_utils.mask_points_by_range (strict) on fp32 points, limits rounded to fp32"""
    r = np.asarray(lidar_range, dtype=F64).astype(F32)
    keep = np.ones(len(q), dtype=bool)
    for j in range(3):
        keep &= (q[:, j] > r[j]) & (q[:, j] < r[3 + j])
    return keep


def project(xyz, t):
    """rows 0 .. 2 of the 4 x 4 fp64 matrix t on fp64 (n, 3): ((t0 x + t1 y) + t2 z) + t3"""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.stack([((t[r, 0] * x + t[r, 1] * y) + t[r, 2] * z) + t[r, 3] for r in range(3)], axis=1)


def rotate(xyz, c, s):
    """the reference's fp32 rotation about z: values rounded to fp32, exact fp64 products, one add, rounded to fp32; -> fp64 (n, 3)"""
    c, s = F64(F32(c)), F64(F32(s))
    x, y, z = (xyz[:, j].astype(F32).astype(F64) for j in range(3))
    return np.stack([(x * c - y * s).astype(F32).astype(F64), (x * s + y * c).astype(F32).astype(F64), z], axis=1)


def augment(xyz, world, c=None, s=None):
    """stage 3 on fp64 (n, 3); c, s: the fp32 cosine and sine of world['rot'] (ops.rotation_cos_sin)"""
    xyz = xyz.copy()
    if world.get("flip_x"):
        xyz[:, 1] = -xyz[:, 1]
    if world.get("flip_y"):
        xyz[:, 0] = -xyz[:, 0]
    if world.get("rot") is not None:
        xyz = rotate(xyz, c, s)
    if world.get("scale") is not None:
        xyz = xyz * F64(F32(world["scale"]))
    return xyz


def stages(p, t=None, ego_mask=False, lidar_range=None, world=None, c=None, s=None):
    """stages 1 - 5 on one agent's fp32 points (n, 4): -> the fp32 output points (n, 4), keep flags, the fp64 values before stage 4"""
    keep = ego_keep(p) if ego_mask else np.ones(len(p), dtype=bool)
    xyz = p[:, :3].astype(F64)
    if t is not None:
        xyz = project(xyz, np.asarray(t, dtype=F64))
    if world:
        xyz = augment(xyz, world, c, s)
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.concatenate([xyz.astype(F32), p[:, 3:4]], axis=1)
    if lidar_range is not None:
        keep = keep & range_keep(q, lidar_range)
    return q, keep, xyz


def clamp_offsets(offsets, m):
    return np.clip(np.asarray(offsets, dtype=np.int64), 0, m)


def prepare_points(points, offsets, transforms=None, order=None, ego_mask=False, lidar_range=None, world=None, c=None, s=None):
    """-> out (K, 4) fp32, out_offsets (N + 1,) int32, per-row keep flags (M,).  Rows outside every agent's range are dropped; an
    order entry outside [0, M) drops its row."""
    points = np.asarray(points, dtype=F32)
    m = len(points)
    o = clamp_offsets(offsets, m)
    keep_all = np.zeros(m, dtype=bool)
    out_all = np.zeros((m, 4), dtype=F32)
    for a in range(len(o) - 1):
        rows = np.arange(o[a], max(o[a], o[a + 1]))                   # (offsets are non-decreasing in every case here)
        src = rows if order is None else np.asarray(order, dtype=np.int64)[rows]
        ok = (src >= 0) & (src < m)
        q, keep, _ = stages(points[np.where(ok, src, 0)], None if transforms is None else transforms[a], ego_mask, lidar_range, world, c, s)
        keep_all[rows] = keep & ok
        out_all[rows] = q
    csum = np.concatenate([[0], np.cumsum(keep_all)])
    return out_all[keep_all], csum[o].astype(np.int32), keep_all


def boxes(b, mask, world, c=None, s=None):
    """the box rules on (G, 7) fp32 / fp64 with mask (G,): rows with mask == 1 augmented in fp64 and rounded to the dtype once"""
    out = np.array(b, copy=True)
    sel = np.asarray(mask) == 1
    v = out[sel].astype(F64)
    if world.get("flip_x"):
        v[:, 1] = -v[:, 1]
        v[:, 6] = -v[:, 6]
    if world.get("flip_y"):
        v[:, 0] = -v[:, 0]
        v[:, 6] = -(v[:, 6] + np.pi)
    if world.get("rot") is not None:
        v[:, :3] = rotate(v[:, :3], c, s)
        v[:, 6] = v[:, 6] + F64(world["rot"])
    if world.get("scale") is not None:
        v[:, :6] = v[:, :6] * F64(world["scale"])
    out[sel] = v.astype(out.dtype)
    return out
