"""Plain restatement of the voxel map, written from the contract in include/cmr_hip.h and independent of the kernels.

Keys and flags are numpy float32 with exactly the operations the header states -- q = R p + t operation by operation
(cloud_icp_reference.pose_apply32), then one subtraction, one division and a floor per axis (cloud_prepare_reference.voxel_keys'
arithmetic), the grid test on the float -- so every integer of an insert is EXACT: keys, counts, stamps, new, merged, removed, dropped,
outside.  The combine is float32, one operation at a time; a scan's own voxel means are float64 means rounded to float32 (exact for a
voxel with one row, which is what the bit-for-bit check uses).  Beside its float32 means every voxel carries the float64 sum of all rows
ever inserted into it, their number, the inserts that touched it and the largest |value| per column: the float64 mean and the bound

    (rows + 8 inserts) 2^-23 absmax

the float32 means are held to.  A map is a dict; nothing is changed in place.
"""
import functools

import numpy as np

import cloud_icp_reference as R
import cloud_prepare_reference as P

F32 = np.float32
CELL_MAX = P.CELL_LIMIT - 1
COUNT_MAX = (1 << 31) - 1
U23 = 2.0 ** -23
DROPPED, OUTSIDE = -1, -2


# ---- keys and flags ---------------------------------------------------------------------------------------------------------------------
def scan_rows(points, pose, origin, voxel):
    """points float32 [N, 3] -> (q float32 [N, 3], keys int64 [N]: DROPPED, OUTSIDE or the key)"""
    p = np.asarray(points, dtype=F32).reshape(-1, 3)
    q = p if pose is None else R.pose_apply32(pose, p)
    finite = np.isfinite(p).all(1) & np.isfinite(q).all(1)
    o, v = np.asarray(origin, dtype=F32), F32(voxel)
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.floor((q - o) / v)                                          # float32 - float32, / float32
        inside = ((c >= F32(0)) & (c <= F32(CELL_MAX))).all(1)              # on the float
    keys = np.full(p.shape[0], DROPPED, dtype=np.int64)
    keys[finite & ~inside] = OUTSIDE
    ok = finite & inside
    ci = c[ok].astype(np.int64)
    keys[ok] = ci[:, 2] << 42 | ci[:, 1] << 21 | ci[:, 0]
    return q, keys


# ---- the map ----------------------------------------------------------------------------------------------------------------------------
def empty(voxel, origin, channels=0):
    z = lambda *s, dt=np.float64: np.zeros(s, dtype=dt)                     # noqa: E731
    w = 3 + channels
    return dict(keys=z(0, dt=np.int64), points=z(0, 3, dt=F32), attr=z(0, channels, dt=F32), count=z(0, dt=np.int64), stamp=z(0, dt=np.int64),
                origin=tuple(float(F32(x)) for x in origin), voxel=float(voxel), sum=z(0, w), absmax=z(0, w), rows=z(0, dt=np.int64),
                inserts=z(0, dt=np.int64))


def combine(ma, mb, ca, cb):
    """float32 [h, w] means and int64 [h] counts of the two sides -> (float32 [h, w], int64 [h]), one operation at a time"""
    n = np.minimum(ca + cb, COUNT_MAX)
    w = (cb.astype(F32) / n.astype(F32)).astype(F32)
    d = (mb - ma).astype(F32)
    wd = (w[:, None] * d).astype(F32)
    return (ma + wd).astype(F32), n


def insert(m, points=None, attr=None, pose=None, stamp=0, min_stamp=None):
    """-> (the new map, dict(new, merged, removed, dropped, outside))"""
    C = m["attr"].shape[1]
    p = np.zeros((0, 3), F32) if points is None else np.asarray(points, dtype=F32).reshape(-1, 3)
    a = np.zeros((p.shape[0], C), F32) if attr is None else np.asarray(attr, dtype=F32).reshape(p.shape[0], C)
    q, keys = scan_rows(p, pose, m["origin"], m["voxel"])
    ok = keys >= 0
    sk, inv, sc = np.unique(keys[ok], return_inverse=True, return_counts=True)
    rows = np.concatenate([q, a], 1)[ok]
    ssum, smax = np.zeros((sk.size, 3 + C)), np.zeros((sk.size, 3 + C))
    np.add.at(ssum, inv, rows.astype(np.float64))
    np.maximum.at(smax, inv, np.abs(rows).astype(np.float64))
    smean = (ssum / np.maximum(sc, 1)[:, None]).astype(F32)
    sc = sc.astype(np.int64)

    allk = np.union1d(m["keys"], sk)
    ia, ib = np.searchsorted(allk, m["keys"]), np.searchsorted(allk, sk)
    hit = np.isin(sk, m["keys"])
    n = allk.size
    val, count, stamps = np.zeros((n, 3 + C), F32), np.zeros(n, np.int64), np.zeros(n, np.int64)
    tot, amax, nrows, nins = np.zeros((n, 3 + C)), np.zeros((n, 3 + C)), np.zeros(n, np.int64), np.zeros(n, np.int64)
    val[ia], count[ia], stamps[ia] = np.concatenate([m["points"], m["attr"]], 1), m["count"], m["stamp"]
    tot[ia], amax[ia], nrows[ia], nins[ia] = m["sum"], m["absmax"], m["rows"], m["inserts"]
    val[ib[~hit]], count[ib[~hit]] = smean[~hit], sc[~hit]
    val[ib[hit]], count[ib[hit]] = combine(val[ib[hit]], smean[hit], count[ib[hit]], sc[hit])
    stamps[ib] = stamp
    tot[ib] += ssum
    amax[ib] = np.maximum(amax[ib], smax)
    nrows[ib] += sc
    nins[ib] += 1
    keep = stamps >= (0 if min_stamp is None else min_stamp)
    out = dict(keys=allk[keep], points=val[keep, :3], attr=val[keep, 3:], count=count[keep], stamp=stamps[keep], origin=m["origin"],
               voxel=m["voxel"], sum=tot[keep], absmax=amax[keep], rows=nrows[keep], inserts=nins[keep])
    return out, dict(new=int((~hit).sum()), merged=int(hit.sum()), removed=int((~keep).sum()), dropped=int((keys == DROPPED).sum()),
                     outside=int((keys == OUTSIDE).sum()))


def mean64(m):
    """float64 [n, 3 + C]: the mean of all rows ever inserted into each voxel"""
    return m["sum"] / np.maximum(m["rows"], 1)[:, None]


def bound(m):
    """float64 [n, 3 + C]: (rows + 8 inserts) 2^-23 absmax"""
    return (m["rows"] + 8 * m["inserts"])[:, None] * U23 * m["absmax"]


def values(m):
    return np.concatenate([m["points"], m["attr"]], 1)


# ---- the ops' interface on the restatement (CPU stand-ins for tests of the file layer) -----------------------------------------------------
def ops_voxel_map_insert(map, points=None, attr=None, pose=None, stamp=0, min_stamp=None):
    import torch
    from cmr_agent_amd import ops
    n, C = map.keys.shape[0], map.attr.shape[1]
    m = empty(map.voxel, map.origin, C)
    m.update(keys=map.keys.numpy(), points=map.points.numpy(), attr=map.attr.numpy(), count=map.count.numpy().astype(np.int64),
             stamp=map.stamp.numpy().astype(np.int64), sum=np.zeros((n, 3 + C)), absmax=np.zeros((n, 3 + C)), rows=np.zeros(n, np.int64),
             inserts=np.zeros(n, np.int64))
    num = lambda t: None if t is None else t.cpu().numpy()                  # noqa: E731
    out, info = insert(m, num(points), num(attr), num(pose), stamp, min_stamp)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x.astype(dt)))  # noqa: E731
    new = ops.VoxelMap(t(out["keys"], np.int64), t(out["points"], F32), t(out["attr"], F32), t(out["count"], np.int32), t(out["stamp"], np.int32),
                       map.origin, map.voxel)
    return ops.MapInsert(new, info["new"], info["merged"], info["removed"], info["dropped"], info["outside"])


# ---- align --map K and accumulate on four synthetic frames ----------------------------------------------------------------------------------
MAP_K, MAP_VOXEL, MAP_EXTENT, MAP_RADIUS = 2, 0.1, 8192.0, 0.6
CHAIN_FIRST = 3


def chain_truth():
    """float64 [4, 4, 4]: frame j of the synthetic sequence in frame 0's coordinates"""
    out = [np.eye(4)]
    for rv, t in R.TRUE_POSES:
        out.append(out[-1] @ R.pose_matrix(rv, t))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def chain_frames():
    """-> the four prepared clouds float32 [7, n]: scenes 20 .. 23 at half scale, downsampled, moved by the inverse of their true pose,
    with the normals of the moved cloud.  Read only."""
    frames = []
    for j, truth in enumerate(chain_truth()):
        raw = P.scene(20 + j, n=1600, clump=100, far=10, scale=0.5)
        down = P.voxel_downsample(raw[:, :3], raw[:, 3:4])
        xyz = R.moved(down["points"].astype(F32), truth)
        nrm = P.point_normals(xyz)["normals"].astype(F32)
        frames.append(np.concatenate([xyz.T, down["attr"].astype(F32).T, nrm.T]).astype(F32))
    return tuple(frames)


def align_map(frames, first=0, k=MAP_K, voxel=MAP_VOXEL, extent=MAP_EXTENT, radius=MAP_RADIUS, max_dist=1.0, huber=0.1, iters=30):
    """The chain `align --map k` states, on the restatements: -> (poses float64 [F, 4, 4], [the icp dict of every pair])"""
    m = empty(voxel, (-extent / 2,) * 3)
    poses, rel, results = [np.eye(4)], np.eye(4), []
    m, _ = insert(m, frames[0][:3].T, pose=np.eye(4, dtype=F32), stamp=first, min_stamp=max(0, first + 1 - k))
    for j in range(1, len(frames)):
        number = first + j
        normals = P.point_normals(m["points"], radius, viewpoint=poses[-1][:3, 3])["normals"].astype(F32)
        start = (poses[-1] @ rel).astype(F32)
        res = R.icp(frames[j][:3].T, m["points"], normals, start, max_dist, huber, iters)
        T = res["pose32"].astype(np.float64)
        rel = np.linalg.inv(poses[-1]) @ T
        poses.append(T)
        results.append(res)
        m, _ = insert(m, frames[j][:3].T, pose=res["pose32"], stamp=number, min_stamp=max(0, number + 1 - k))
    return np.stack(poses), results


@functools.lru_cache(maxsize=None)
def chain_case():
    """-> dict(frames, truth, poses, results) of align --map 2 with Huber 0.1, max_dist 1.0 and 40 iterations.  Read only."""
    frames = chain_frames()
    poses, results = align_map(frames, CHAIN_FIRST, iters=R.LOOP_ITERS)
    return dict(frames=frames, truth=chain_truth(), poses=poses, results=results)


def accumulate(frames, poses, first=0, voxel=MAP_VOXEL, extent=MAP_EXTENT):
    """Every frame under its pose (float32 of the given numbers), the reflectance as the one attribute -> the map"""
    m = empty(voxel, (-extent / 2,) * 3, 1)
    for j, (f, T) in enumerate(zip(frames, poses)):
        m, _ = insert(m, f[:3].T, f[3:4].T, np.asarray(T, dtype=F32), stamp=first + j)
    return m
