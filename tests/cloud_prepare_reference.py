"""Plain restatement of the cloud preparation, written from the contract in include/cmr_hip.h and independent of the kernels.

Voxel keys are computed in numpy float32 exactly as the header states them (one subtraction, one division, floor), so every integer of the
downsample -- keys, order, counts, inverse -- is exact and not approximate; the means are float64.  Neighbourhoods come from brute-force
chunked distances (no grid), the membership test in float32 as stated; covariance and eigen-solve are float64.  Per row the normals also
report how far the comparison can be trusted:

    gap   (l1 - l0) / l2 of the float64 eigenvalues: the normal is conditioned like 1 / gap
    near  some |norm(d) - r| <= 1e-5 r: fp32 may count that neighbour either way
    flip  |cos(n, viewpoint - p)| < 1e-3: the orientation sign is not decided in fp32
"""
import functools

import numpy as np

CELL_LIMIT = 1 << 21
SEEDS = (11, 12, 13)
VOXEL, RADIUS = 0.1, 0.6
GAP_MIN, NEAR_REL, FLIP_COS = 1e-2, 1e-5, 1e-3
U24 = 2.0 ** -24


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def scene(seed, n=5400, clump=600, far=40, scale=1.0):
    """float32 [N, 4]: a noisy ground plane, a wall, a cylinder and a clutter box on a 12 m patch (n points), a clump inside a 0.3 m cube
    (many rows per voxel), isolated far points (fewer than 3 neighbours); column 3 is a reflectance in [0, 1].  `scale` stretches the patch
    and the point count with it (the benchmark's 120 000-point scan)."""
    r = np.random.default_rng(seed)
    k = n // 4
    L = 6.0 * scale
    ground = np.stack([r.uniform(-L, L, k), r.uniform(-L, L, k), -1.7 + 0.01 * r.standard_normal(k)], 1)
    wall = np.stack([r.uniform(-L, L, k), 5.0 * scale + 0.01 * r.standard_normal(k), r.uniform(-1.7, 1.5, k)], 1)
    t, z = r.uniform(0, 2 * np.pi, k), r.uniform(-1.7, 1.0, k)
    pole = np.stack([3 + 0.8 * np.cos(t), -2 + 0.8 * np.sin(t), z], 1) + 0.01 * r.standard_normal((k, 3))
    box = r.uniform(-1, 1, (n - 3 * k, 3)) * [1.0, 1.0, 0.3] + [-3, -3, -1.0]
    clump_pts = r.uniform(0, 0.3, (clump, 3)) + [1.0, 1.0, -1.0]
    far_pts = r.uniform(-1, 1, (far, 3)) * [40, 40, 2] + [0, 0, 5]
    xyz = np.concatenate([ground, wall, pole, box, clump_pts, far_pts])
    refl = r.uniform(0, 1, (xyz.shape[0], 1))
    return np.concatenate([xyz, refl], 1).astype(np.float32)


# ---- voxel downsample -------------------------------------------------------------------------------------------------------------------
def voxel_keys(points, voxel=VOXEL, origin=None):
    """points float32 [N, 3] -> (keys int64 [N], -1 for dropped rows; origin float32 [3]; cells int64 [N, 3]).  ValueError as the op's."""
    p = np.asarray(points, dtype=np.float32)
    keep = np.isfinite(p).all(1)
    v = np.float32(voxel)
    keys = np.full(p.shape[0], -1, dtype=np.int64)
    cells = np.zeros((p.shape[0], 3), dtype=np.int64)
    if not keep.any():
        return keys, np.zeros(3, np.float32), cells
    o = np.asarray(origin, dtype=np.float32) if origin is not None else p[keep].min(0) - v * np.float32(0.5)
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.floor((p[keep] - o) / v)                                    # float32 - float32, / float32: IEEE, as the header states
    if not np.isfinite(c).all() or c.max() >= CELL_LIMIT or c.min() < 0:
        raise ValueError("cell index outside [0, 2^21)")
    c = c.astype(np.int64)
    cells[keep] = c
    keys[keep] = c[:, 2] << 42 | c[:, 1] << 21 | c[:, 0]
    return keys, o, cells


def voxel_downsample(points, attr=None, voxel=VOXEL, origin=None):
    """-> dict(points float64 [n, 3], attr float64 [n, C], count [n], inverse int64 [N], dropped, keys [n], absmax_points / absmax_attr:
    the largest |value| per voxel and column (the sequential-sum bound of the fp32 mean is count * 2^-23 * that))."""
    p = np.asarray(points, dtype=np.float32)
    a = np.zeros((p.shape[0], 0), np.float32) if attr is None else np.asarray(attr, dtype=np.float32)
    keys, o, _ = voxel_keys(p, voxel, origin)
    keep = keys >= 0
    uniq, inv_kept, count = np.unique(keys[keep], return_inverse=True, return_counts=True)
    n = uniq.size
    inverse = np.full(p.shape[0], -1, dtype=np.int64)
    inverse[keep] = inv_kept
    out = {}
    for name, src in (("points", p), ("attr", a)):
        s = np.zeros((n, src.shape[1]))
        m = np.zeros((n, src.shape[1]))
        np.add.at(s, inv_kept, src[keep].astype(np.float64))
        np.maximum.at(m, inv_kept, np.abs(src[keep]).astype(np.float64))
        out[name] = s / np.maximum(count, 1)[:, None]
        out["absmax_" + name] = m
    out.update(count=count.astype(np.int64), inverse=inverse, dropped=int((~keep).sum()), keys=uniq, origin=o)
    return out


def cell_disagreements(points, voxel=VOXEL):
    """Rows whose float64 evaluation of the cell formula lands in another cell than the float32 one."""
    p = np.asarray(points, dtype=np.float32)
    _, o, cells = voxel_keys(p, voxel)
    c64 = np.floor((p.astype(np.float64) - o.astype(np.float64)) / np.float64(np.float32(voxel))).astype(np.int64)
    return int((c64 != cells).any(1).sum())


# ---- normals ----------------------------------------------------------------------------------------------------------------------------
def point_normals(points, radius=RADIUS, viewpoint=(0.0, 0.0, 0.0), min_neighbors=3, chunk=512):
    """points float32 [n, 3] -> dict(normals float64 [n, 3], count [n], eigenvalues float64 [n, 3] ascending, zero [n] (the contract's zero
    normal), gap, near, flip [n])."""
    p = np.asarray(points, dtype=np.float32)
    n = p.shape[0]
    finite = np.isfinite(p).all(1)
    r32 = np.float32(radius)
    r2 = r32 * r32
    vp = np.asarray(viewpoint, dtype=np.float64)
    kmin = max(3, int(min_neighbors))
    out = dict(normals=np.zeros((n, 3)), count=np.zeros(n, np.int64), eigenvalues=np.zeros((n, 3)), zero=np.ones(n, bool), gap=np.zeros(n),
               near=np.zeros(n, bool), flip=np.zeros(n, bool))
    idx = np.nonzero(finite)[0]
    q = p[idx]
    q64 = q.astype(np.float64)
    for lo in range(0, idx.size, chunk):
        rows = slice(lo, min(lo + chunk, idx.size))
        d = q[None, :, :] - q[rows, None, :]                                       # float32 p_j - p_i
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]  # float32, each product and sum rounded on its own
        member = d2 <= r2
        d64 = q64[None, :, :] - q64[rows, None, :]
        dist = np.sqrt((d64 * d64).sum(-1))
        near = (np.abs(dist - float(r32)) <= NEAR_REL * float(r32)).any(1)
        for a in range(d.shape[0]):
            i = idx[lo + a]
            dj = d64[a][member[a]]
            k = dj.shape[0]
            out["count"][i], out["near"][i] = k, near[a]
            if k < kmin:
                continue
            m = dj.mean(0)
            C = dj.T @ dj / k - np.outer(m, m)
            w, v = np.linalg.eigh(C)
            nrm = v[:, 0]
            to_view = vp - q64[lo + a]
            s = float(nrm @ to_view)
            out["normals"][i] = -nrm if s < 0 else nrm
            out["eigenvalues"][i] = w
            out["zero"][i] = False
            out["gap"][i] = (w[1] - w[0]) / max(w[2], 1e-300)
            out["flip"][i] = abs(s) < FLIP_COS * max(np.linalg.norm(to_view), 1e-300)
    return out


def kept_rows(ref):
    """Rows on which a normal is compared: valid, well conditioned, no neighbour on the radius, orientation decided."""
    return ~ref["zero"] & (ref["gap"] >= GAP_MIN) & ~ref["near"] & ~ref["flip"]


def excluded_share(ref):
    valid = ~ref["zero"]
    return float((valid & ~kept_rows(ref)).sum()) / max(1, int(valid.sum()))


def angle(a, b):
    """Angle between the LINES spanned by the rows of a and b (sign free), float64, exact for small angles."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(1)))


def angle_bound(ref):
    """4 k 2^-24 / gap: the first-order perturbation of the eigenvector under the rounding of k fp32 additions, with a factor of 4."""
    return 4.0 * ref["count"] * U24 / np.maximum(ref["gap"], 1e-300)


# ---- the scenes' results, computed once and shared -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_case(seed):
    """-> dict(raw float32 [N, 4], down = voxel_downsample(raw), cloud float32 [n, 3] = its means rounded to float32, normals =
    point_normals(cloud)).  Callers must not modify it."""
    raw = scene(seed)
    down = voxel_downsample(raw[:, :3], raw[:, 3:4])
    cloud = down["points"].astype(np.float32)
    return dict(raw=raw, down=down, cloud=cloud, normals=point_normals(cloud))


# ---- a cloud whose second cluster lies beyond 2^19 cells from the grid's origin ---------------------------------------------------------------
FAR_RADIUS = 1.0


def walk_runs(points, cell, origin=None):
    """The number of runs of sorted rows that the kernels' walk (csrc/cmr_cloud_grid.h: axis_cells, Walk) searches for every row of the
    cloud on the grid of `cell` whose origin is the cloud's minimum: (cells along y) * (cells along z), in the header's fp32 arithmetic.
    A 16-lane group takes 16 runs in one pass; more need the second one."""
    p = np.asarray(points, dtype=np.float32)
    o = p.min(0) if origin is None else np.asarray(origin, dtype=np.float32)
    t = (p - o) / np.float32(cell)
    c = np.floor(t)
    tol = (t + np.float32(2.0)) * np.float32(9.5367431640625e-07)
    frac = t - c
    lo = np.maximum(c.astype(np.int64) - 1 - (frac < tol), 0)
    hi = np.minimum(c.astype(np.int64) + 1 + (frac > np.float32(1.0) - tol), CELL_LIMIT - 1)
    n = hi - lo + 1
    return n[:, 1] * n[:, 2]


@functools.lru_cache(maxsize=None)
def far_case():
    """-> dict(cloud float32 [120, 3]: 60 rows in [0, 2)^3 and 60 rows on a lattice of 1/16 at 700 000, where a cell coordinate of the
    radius-1 grid is rounded to 1/16 and axis_cells adds a cell on both sides of an axis: 16, 20 or 25 runs, the walk's second pass; normals
    = point_normals(cloud, 1.0)).  Callers must not modify it."""
    r = np.random.default_rng(5)
    first = r.uniform(0.0, 2.0, (60, 3))
    second = np.float32(700000) + r.integers(0, 33, (60, 3)) * 0.0625
    cloud = np.concatenate([first, second]).astype(np.float32)
    return dict(cloud=cloud, normals=point_normals(cloud, FAR_RADIUS))


# ---- the ops' interface on the restatement (CPU stand-ins for tests of the file layer) -----------------------------------------------------
def ops_voxel_downsample(points, attr=None, voxel=VOXEL, origin=None, want_inverse=False):
    import torch
    from cmr_agent_amd import ops
    d = voxel_downsample(points.cpu().numpy(), None if attr is None else attr.cpu().numpy(), voxel, origin)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x.astype(dt)))            # noqa: E731
    return ops.VoxelCloud(t(d["points"], np.float32), None if attr is None else t(d["attr"], np.float32), t(d["count"], np.int32),
                          t(d["inverse"], np.int64) if want_inverse else None, d["dropped"], tuple(float(v) for v in d["origin"]))


def ops_point_normals(points, radius=RADIUS, viewpoint=(0, 0, 0), min_neighbors=3, want_eigenvalues=False):
    import torch
    from cmr_agent_amd import ops
    d = point_normals(points.cpu().numpy(), radius, viewpoint, min_neighbors)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x.astype(dt)))            # noqa: E731
    return ops.PointNormals(t(d["normals"], np.float32), t(d["count"], np.int32), t(d["eigenvalues"], np.float32) if want_eigenvalues else None)


# ---- a dataset tree with raw scans only -------------------------------------------------------------------------------------------------
def write_bin(path, raw4n):
    """float32 [4, N] -> KITTI's velodyne .bin (float32 [N, 4])."""
    np.ascontiguousarray(np.asarray(raw4n).T, dtype=np.float32).tofile(path)


def write_raw_tree(root, seq=9, frames=2):
    """Calibration and images as tests/test_loader.py writes them, and <seq>/velodyne/<i>.bin instead of the prepared cloud folder.
    -> (the velodyne folder, the raw scans float32 [4, N])."""
    import os

    import cases as C
    f = C.FRAME
    fmt = lambda name, v: name + ": " + " ".join("%.12e" % x for x in v) + "\n"      # noqa: E731
    os.makedirs(os.path.join(root, "calib", "%02d" % seq), exist_ok=True)
    with open(os.path.join(root, "calib", "%02d" % seq, "calib.txt"), "w") as fh:
        fh.write("".join(fmt(k, C.FRAME_P2) for k in ("P0", "P1", "P2", "P3")) + fmt("Tr", C.FRAME_TR))
    img = os.path.join(root, "data_odometry_color_npy", "sequences", "%02d" % seq, "image_2")
    vel = os.path.join(root, "data_odometry_velodyne_NWU", "sequences", "%02d" % seq, "velodyne")
    os.makedirs(img)
    os.makedirs(vel)
    rng = np.random.RandomState(7)
    raws = []
    for i in range(frames):
        raw = scene(20 + i, n=1600, clump=100, far=10).T.copy()
        raw[0] += np.float32(8.0)                                # velodyne frame: x forward -- the patch in front of the camera
        write_bin(os.path.join(vel, "%06d.bin" % i), raw)
        np.save(os.path.join(img, "%06d.npy" % i), rng.randint(0, 256, size=(f["img_h"], f["img_w"], 3)).astype(np.uint8))
        raws.append(raw)
    return vel, raws
