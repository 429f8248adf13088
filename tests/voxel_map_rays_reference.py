"""Plain restatement of the rays cast through a voxel map, written from the contract in include/cmr_hip.h and independent
of the kernel.

Everything is numpy float32, one operation at a time, as the header states it: the moved row (cloud_icp_reference.pose_apply32), one
subtraction and one division per cell coordinate, a floor, the grid test on the float (the arithmetic of voxel_map_reference.scan_rows),
then the walk -- left_x + left_y + left_z steps, each along the axis with the least tmax, x before y before z on ties, tmax recomputed
from the integer cell and never divided on an axis that has no step left.  So every integer is EXACT: the cells of a walk, crossed, hits
and the four counts.  All rays step together, one numpy pass per step.  `slab64` is the float64 check that such a walk is a ray at all;
`carve` and `carve_frames` restate the rule of `accumulate --carve`.
"""
import math

import numpy as np

import cloud_icp_reference as R
import voxel_map_reference as V

F32 = np.float32
CELL_MAX = V.CELL_MAX
CAST, DROPPED, OUTSIDE, LONG = 0, 1, 2, 3
MAX_CELLS = 1 << 16


def pack(c):
    """int64 [n, 3] cells -> int64 [n] keys"""
    c = np.asarray(c, dtype=np.int64).reshape(-1, 3)
    return c[:, 2] << 42 | c[:, 1] << 21 | c[:, 0]


def _tmax(c, left, step, a, d):
    """float32 [n, 3]: ((float) (c + (step > 0)) - a) / d where a step is left, +inf elsewhere; no division elsewhere"""
    face = (c + (step > 0)).astype(F32)
    num = (face - a).astype(F32)
    out = np.full(c.shape, np.inf, dtype=F32)
    np.divide(num, d, out=out, where=left > 0)
    return out


def walk(points, pose, origin, voxel, max_cells=4096):
    """points float32 [N, 3] -> dict: state int [N] (CAST, DROPPED, OUTSIDE, LONG), start / end int64 [N, 3] (cells; of rows on the grid),
    a, b float32 [N, 3] (the cell coordinates of sensor and end), ray int64 [V] and cell int64 [V, 3]: every cell a cast ray visits other
    than its end's, in the order of the walk (ray by step, rays interleaved)."""
    p = np.asarray(points, dtype=F32).reshape(-1, 3)
    N = p.shape[0]
    q = p if pose is None else R.pose_apply32(pose, p)
    o = np.zeros(3, F32) if pose is None else np.asarray(pose, dtype=F32)[:3, 3]
    finite = np.isfinite(p).all(1) & np.isfinite(q).all(1)
    org, v = np.asarray(origin, dtype=F32), F32(voxel)
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.broadcast_to(((o - org).astype(F32) / v).astype(F32), (N, 3)).copy()
        b = ((q - org).astype(F32) / v).astype(F32)
        fa, fb = np.floor(a), np.floor(b)
        inside = ((fa >= F32(0)) & (fa <= F32(CELL_MAX)) & (fb >= F32(0)) & (fb <= F32(CELL_MAX))).all(1)          # on the float
        d = (b - a).astype(F32)
    ok = finite & inside
    s, e = np.zeros((N, 3), np.int64), np.zeros((N, 3), np.int64)
    s[ok], e[ok] = fa[ok].astype(np.int64), fb[ok].astype(np.int64)
    left, step = np.abs(e - s), np.sign(e - s)
    long = ok & (left.sum(1) > max_cells)
    state = np.full(N, DROPPED)
    state[finite] = OUTSIDE
    state[ok] = CAST
    state[long] = LONG

    idx = np.nonzero(state == CAST)[0]
    c, lf = s[idx].copy(), left[idx].copy()
    rays, cells = [], []
    while True:
        done = lf.sum(1) == 0
        assert np.array_equal(c[done], e[idx[done]]), "a walk did not end in the end's cell"
        idx, c, lf = idx[~done], c[~done], lf[~done]
        if idx.size == 0:
            break
        rays.append(idx)
        cells.append(c.copy())
        t = _tmax(c, lf, step[idx], a[idx], d[idx])
        assert np.isfinite(t.min(1)).all() and not np.isnan(t).any()
        axis = np.where((t[:, 0] <= t[:, 1]) & (t[:, 0] <= t[:, 2]), 0, np.where(t[:, 1] <= t[:, 2], 1, 2))
        row = np.arange(idx.size)
        assert (lf[row, axis] > 0).all()
        c[row, axis] += step[idx, axis]
        lf[row, axis] -= 1
    return dict(state=state, start=s, end=e, a=a, b=b, ray=np.concatenate(rays) if rays else np.zeros(0, np.int64),
                cell=np.concatenate(cells) if cells else np.zeros((0, 3), np.int64))


def visited(w, ray):
    """int64 [n, 3]: the cells ray `ray` of a walk visits, in order, its end's cell last"""
    assert w["state"][ray] == CAST
    return np.concatenate([w["cell"][w["ray"] == ray], w["end"][ray:ray + 1]])


def _rows_of(keys, k):
    """-> the rows of the sorted keys that hold the keys k (found ones only)"""
    keys = np.asarray(keys, dtype=np.int64)
    if keys.size == 0:
        return np.zeros(0, np.int64)
    pos = np.minimum(np.searchsorted(keys, k), keys.size - 1)
    return pos[keys[pos] == k]


def cast(keys, origin, voxel, points, pose=None, start_margin=2, end_margin=1, max_cells=4096, w=None):
    """-> dict(crossed int64 [M], hits int64 [M], cast, dropped, outside, long) of the rays of `points` through the map's keys"""
    keys = np.asarray(keys, dtype=np.int64)
    w = walk(points, pose, origin, voxel, max_cells) if w is None else w
    crossed, hits = np.zeros(keys.size, np.int64), np.zeros(keys.size, np.int64)
    ray, cell = w["ray"], w["cell"]
    sel = (np.abs(cell - w["start"][ray]).max(1) > start_margin) & (np.abs(cell - w["end"][ray]).max(1) > end_margin) if ray.size else np.zeros(0, bool)
    np.add.at(crossed, _rows_of(keys, pack(cell[sel])), 1)
    np.add.at(hits, _rows_of(keys, pack(w["end"][w["state"] == CAST])), 1)
    st = w["state"]
    return dict(crossed=crossed, hits=hits, cast=int((st == CAST).sum()), dropped=int((st == DROPPED).sum()), outside=int((st == OUTSIDE).sum()),
                long=int((st == LONG).sum()))


# ---- the float64 check: is the walk a ray? ----------------------------------------------------------------------------------------------
def _meets(A, B, lo, hi):
    """float64 segments A -> B [n, 3] against boxes [lo, hi] [n, 3]: the slab test over t in [0, 1]"""
    D = B - A
    still = D == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - A) / np.where(still, 1.0, D), (hi - A) / np.where(still, 1.0, D)
    tn, tf = np.minimum(t1, t2), np.maximum(t1, t2)
    tn = np.where(still, np.where((A >= lo) & (A <= hi), -np.inf, np.inf), tn)
    tf = np.where(still, np.where((A >= lo) & (A <= hi), np.inf, -np.inf), tf)
    return np.maximum(tn.max(1), 0.0) <= np.minimum(tf.min(1), 1.0)


def slab64(points, pose, origin, voxel, w, eps=1e-3):
    """For every (ray, cell) pair near each walk -- the walked cells and their 26 neighbours -- the float64 segment between the float64
    cell coordinates of sensor and end against the cell shrunk and grown by eps cells.  -> dict(decided = pairs whose shrunk box the
    segment meets, missed = those of them the walk lacks, extra = walked pairs whose grown box it misses, undecided = pairs in between)"""
    p = np.asarray(points, dtype=F32).reshape(-1, 3)
    q = (p if pose is None else R.pose_apply32(pose, p)).astype(np.float64)
    o = np.zeros(3) if pose is None else np.asarray(pose, dtype=F32)[:3, 3].astype(np.float64)
    org, v = np.asarray(origin, dtype=F32).astype(np.float64), float(F32(voxel))
    A_all, B_all = np.broadcast_to((o - org) / v, q.shape), (q - org) / v
    off = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    out = dict(decided=0, missed=0, extra=0, undecided=0)
    for ray in np.nonzero(w["state"] == CAST)[0]:
        own = visited(w, ray)
        near = np.unique((own[:, None, :] + off[None]).reshape(-1, 3), axis=0)
        walked = np.isin(pack(near), pack(own))
        A, B = np.broadcast_to(A_all[ray], near.shape), np.broadcast_to(B_all[ray], near.shape)
        inner, outer = _meets(A, B, near + eps, near + 1 - eps), _meets(A, B, near - eps, near + 1 + eps)
        out["decided"] += int(inner.sum())
        out["missed"] += int((inner & ~walked).sum())
        out["extra"] += int((~outer & walked).sum())
        out["undecided"] += int((outer & ~inner).sum())
    return out


# ---- the rule of accumulate --carve -------------------------------------------------------------------------------------------------------
def carve(through, seen, frames=2, ratio=1.0):
    """int [n] frames that saw through / saw each voxel -> bool [n]: the voxels to drop"""
    through, seen = np.asarray(through, dtype=np.int64), np.asarray(seen, dtype=np.int64)
    return np.array([int(t) >= frames and float(t) >= ratio * float(s) for t, s in zip(through, seen)], dtype=bool).reshape(through.shape)


def carve_frames(keys, origin, voxel, clouds, poses, rays=1, frames=2, ratio=1.0, start=2.0, end=1, max_range=120.0):
    """clouds: float32 [N, 3] per frame, poses float32 [4, 4] per frame -> (bool [M] the voxels dropped, [the cast dict of every frame with
    `through` = the voxels that frame saw through])"""
    keys = np.asarray(keys, dtype=np.int64)
    start_margin, max_cells = int(math.ceil(start / voxel)), int(min(MAX_CELLS, math.ceil(3.0 * max_range / voxel)))
    through, seen, infos = np.zeros(keys.size, np.int64), np.zeros(keys.size, np.int64), []
    for xyz, T in zip(clouds, poses):
        res = cast(keys, origin, voxel, xyz, T, start_margin, end, max_cells)
        sees_through = (res["crossed"] >= rays) & (res["hits"] == 0)
        through += sees_through
        seen += res["hits"] > 0
        infos.append(dict(res, through=int(sees_through.sum())))
    return carve(through, seen, frames, ratio), infos


def with_block(frames, poses, centre=(3.0, 0.0, 0.3), half=0.3, n=60, seed=5):
    """A moving object for a sequence of prepared clouds float32 [7, m] under poses [F, 4, 4] (frame j in frame 0's coordinates): frame 0
    gets n more rows, a block round `centre` that only it holds, and every later frame n more rows twice as far from ITS sensor along the
    beams through the block's rows -- so every later frame's rays pass through every voxel of the block.  -> (the frames, n)"""
    rng = np.random.default_rng(seed)
    block = (np.asarray(centre) + rng.uniform(-half, half, (n, 3))).astype(F32)
    extra = lambda xyz: np.concatenate([xyz.T, np.full((1, n), 0.5, F32), np.tile(F32([[-1], [0], [0]]), (1, n))]).astype(F32)      # noqa: E731
    out = [np.concatenate([frames[0], extra(block)], 1)]
    for f, T in zip(frames[1:], np.asarray(poses, dtype=np.float64)[1:]):
        beyond = T[:3, 3] + 2.0 * (block.astype(np.float64) - T[:3, 3])
        out.append(np.concatenate([f, extra(R.moved(beyond, T))], 1))
    return tuple(out), n


# ---- the op's interface on the restatement (a CPU stand-in for tests of the file layer) ----------------------------------------------------
def ops_voxel_map_rays(map, points, pose=None, start_margin=2, end_margin=1, max_cells=4096):
    import torch
    from cmr_agent_amd import ops
    res = cast(map.keys.cpu().numpy(), map.origin, map.voxel, points.cpu().numpy(), None if pose is None else pose.cpu().numpy(), start_margin,
               end_margin, max_cells)
    t = lambda x: torch.from_numpy(x.astype(np.int32))                      # noqa: E731
    return ops.MapRays(t(res["crossed"]), t(res["hits"]), res["cast"], res["dropped"], res["outside"], res["long"])
