"""Plain restatement of the cloud-against-cloud operations, written from the contract in include/cmr_hip.h and independent
of the kernels and of any grid.

The nearest row is found by brute force in numpy float32 with exactly the operations the header states -- q = R p + t operation by
operation, d = c - q, d2 = (dx dx + dy dy) + dz dz, the lowest row on equal d2 -- so idx and d2 are EXACT, not approximate.  (Queries are
taken in chunks sorted along x and a chunk looks only at the target rows whose x lies within max_dist (1 + 1e-5) of the chunk: d2 >= dx dx in
float32 too, so no row that passes the test is left out and the result is the full brute force's.)  The terms of the Gauss-Newton system
are float64 from the float32 q, c, n with the header's operation order, their sums numpy's float64 pairwise sums; Cholesky with the
header's pivot rule, Rodrigues and the pose update are float64.
"""
import functools

import numpy as np

import cloud_prepare_reference as P

F32 = np.float32
PIVOT_TOL = 1e-13
TRUE_POSES = (((0.02, -0.015, 0.05), (0.3, -0.2, 0.1)), ((0.0, 0.0, 0.10), (0.5, 0.4, -0.1)), ((0.03, 0.03, -0.08), (-0.4, 0.3, 0.15)))
MAX_DISTS = (1.0, 0.5)
HUBER_OTHER = 0.1
LOOP_ITERS = 40


# ---- nearest row ------------------------------------------------------------------------------------------------------------------------
def pose_apply32(pose, p):
    """q = R p + t in float32, every operation rounded on its own, left to right.  pose [4, 4], p float32 [M, 3] -> float32 [M, 3]."""
    T = np.asarray(pose, dtype=F32)
    p = np.asarray(p, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1).astype(F32)


def nearest(target, queries, max_dist, pose=None, chunk=256):
    """target float32 [n, 3], queries float32 [M, 3] -> (idx int64 [M], -1 for none; d2 float32 [M], NaN for none; q float32 [M, 3])."""
    c_all = np.asarray(target, dtype=F32).reshape(-1, 3)
    q = np.asarray(queries, dtype=F32).reshape(-1, 3)
    if pose is not None:
        q = pose_apply32(pose, q)
    M = q.shape[0]
    idx = np.full(M, -1, dtype=np.int64)
    d2out = np.full(M, np.nan, dtype=F32)
    rows = np.nonzero(np.isfinite(c_all).all(1))[0]
    rows = rows[np.argsort(c_all[rows, 0], kind="stable")]
    c = c_all[rows]
    cx64 = c[:, 0].astype(np.float64)
    r32 = F32(max_dist)
    r2 = r32 * r32
    reach = float(r32) * (1.0 + 1e-5) + 1e-30
    live = np.nonzero(np.isfinite(q).all(1))[0]
    live = live[np.argsort(q[live, 0], kind="stable")]
    for lo in range(0, live.size, chunk):
        qi = live[lo:lo + chunk]
        qq = q[qi]
        a = np.searchsorted(cx64, float(qq[0, 0]) - reach, "left")
        b = np.searchsorted(cx64, float(qq[-1, 0]) + reach, "right")
        if b <= a:
            continue
        cc, cr = c[a:b], rows[a:b]
        with np.errstate(over="ignore", invalid="ignore"):
            dx = cc[None, :, 0] - qq[:, None, 0]
            dy = cc[None, :, 1] - qq[:, None, 1]
            dz = cc[None, :, 2] - qq[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
        ok = d2 <= r2
        d2m = np.where(ok, d2, F32(np.inf))
        best = d2m.min(1)
        tie = np.where(ok & (d2m == best[:, None]), cr[None, :], np.iinfo(np.int64).max).min(1)
        found = ok.any(1)
        idx[qi[found]] = tie[found]
        d2out[qi[found]] = best[found]
    return idx, d2out, q


# ---- the Gauss-Newton system ------------------------------------------------------------------------------------------------------------
def pair_terms(q, c, n, huber=0.0):
    """float32 q, c, n [P, 3] -> float64 [P, 28]: every pair's contribution to H (21 upper entries, row by row), g (6) and cost, each
    operation rounded on its own in the header's order."""
    Q, C, N = (np.asarray(v, dtype=F32).astype(np.float64) for v in (q, c, n))
    r = (N[:, 0] * (Q[:, 0] - C[:, 0]) + N[:, 1] * (Q[:, 1] - C[:, 1])) + N[:, 2] * (Q[:, 2] - C[:, 2])
    J = np.stack([Q[:, 1] * N[:, 2] - Q[:, 2] * N[:, 1], Q[:, 2] * N[:, 0] - Q[:, 0] * N[:, 2], Q[:, 0] * N[:, 1] - Q[:, 1] * N[:, 0],
                  N[:, 0], N[:, 1], N[:, 2]], 1)
    w = np.ones_like(r)
    h = float(F32(huber))
    if h > 0.0:
        big = np.abs(r) > h
        w[big] = h / np.abs(r[big])
    cols = [(w * J[:, i]) * J[:, j] for i in range(6) for j in range(i, 6)]
    cols += [(w * J[:, i]) * r for i in range(6)]
    cols.append((w * r) * r)
    return np.stack(cols, 1) if r.size else np.zeros((0, 28))


def full_matrix(upper):
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = upper
    return H + np.triu(H, 1).T


def chol_solve(upper, g):
    """H x = g by Cholesky, a pivot must be > 0 and > PIVOT_TOL of its diagonal entry; None when it is not."""
    H = full_matrix(upper)
    L = np.zeros((6, 6))
    for j in range(6):
        d = H[j, j] - float(L[j, :j] @ L[j, :j])
        if not (d > 0.0 and d > PIVOT_TOL * H[j, j]):
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (H[i, j] - float(L[i, :j] @ L[j, :j])) / L[j, j]
    z = np.zeros(6)
    for i in range(6):
        z[i] = (g[i] - float(L[i, :i] @ z[:i])) / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (z[i] - float(L[i + 1:, i] @ x[i + 1:])) / L[i, i]
    return x


def expso3(w):
    w = np.asarray(w, dtype=np.float64)
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < 1e-8:
        a, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        a, c = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + a * W + c * (W @ W)


def pose_matrix(rotvec, t):
    T = np.eye(4)
    T[:3, :3] = expso3(rotvec)
    T[:3, 3] = t
    return T


def pose_error(T, truth):
    """-> (rotation angle in rad, translation distance) between two poses"""
    T, truth = np.asarray(T, np.float64), np.asarray(truth, np.float64)
    D = truth[:3, :3].T @ T[:3, :3]
    s = np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2.0
    return float(np.arctan2(s, (np.trace(D) - 1.0) / 2.0)), float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))


def step(T, xi):
    """T <- [exp(omega) | v] T, float64"""
    E = np.eye(4)
    E[:3, :3] = expso3(xi[:3])
    E[:3, 3] = xi[3:]
    return E @ T


def iteration(source, target, normals, T, max_dist, huber=0.0):
    """One iteration from the float64 pose T.  -> dict(pairs, terms [pairs, 28], sums [28], abs_sums [28], xi or None, pose (the update, or
    T), idx, d2)."""
    n32 = np.asarray(normals, dtype=F32)
    idx, d2, q = nearest(target, source, max_dist, T.astype(F32))
    use = idx >= 0
    use[use] = (n32[idx[use]] != 0).any(1)
    rows = idx[use]
    terms = pair_terms(q[use], np.asarray(target, dtype=F32)[rows], n32[rows], huber)
    sums = terms.sum(0)
    out = dict(pairs=int(use.sum()), terms=terms, sums=sums, abs_sums=np.abs(terms).sum(0), xi=None, pose=T, idx=idx, d2=d2)
    if out["pairs"] >= 6 and np.isfinite(sums).all():
        xi = chol_solve(sums[:21], -sums[21:27])
        if xi is not None and np.isfinite(step(T, xi)).all():
            out["xi"], out["pose"] = xi, step(T, xi)
    return out


def icp(source, target, normals, pose=None, max_dist=1.0, huber=0.0, iters=30, tol_rot=1e-6, tol_trans=1e-6):
    """The loop.  -> dict(pose float64 [4, 4], pose32, status, iterations, pairs, rmse, trace [iters, 4], system [iters, 28])."""
    T = np.eye(4) if pose is None else np.asarray(pose, dtype=F32).astype(np.float64)
    T[3] = [0, 0, 0, 1]
    trace, system = np.zeros((iters, 4)), np.zeros((iters, 28))
    status, done = 1, 0
    tr, tt = float(F32(tol_rot)), float(F32(tol_trans))
    for k in range(iters):
        it = iteration(source, target, normals, T, max_dist, huber)
        done = k + 1
        system[k] = it["sums"]
        trace[k, 0] = it["pairs"]
        trace[k, 1] = np.sqrt(it["sums"][27] / it["pairs"]) if it["pairs"] else 0.0
        if it["pairs"] < 6:
            status = 2
            break
        if it["xi"] is None:
            status = 3
            break
        T = it["pose"]
        trace[k, 2], trace[k, 3] = np.linalg.norm(it["xi"][:3]), np.linalg.norm(it["xi"][3:])
        if trace[k, 2] < tr and trace[k, 3] < tt:
            status = 0
            break
    last = trace[done - 1] if done else np.zeros(4)
    return dict(pose=T, pose32=T.astype(F32), status=status, iterations=done, pairs=int(last[0]), rmse=float(last[1]), trace=trace,
                system=system)


# ---- the scenes and the loop's cases, computed once and shared ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_case():
    """-> dict(target float32 [4489, 3] and normals float32 (seed 11, 42 of them zero), other float32 [4581, 3] (seed 12).  Read only."""
    a, b = P.scene_case(11), P.scene_case(12)
    return dict(target=a["cloud"], normals=a["normals"]["normals"].astype(F32), other=b["cloud"])


def moved(cloud, truth):
    """The cloud moved by the inverse of `truth` (float64) and rounded to float32: registering it back finds `truth`."""
    inv = np.linalg.inv(truth)
    return (np.asarray(cloud, np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(F32)


@functools.lru_cache(maxsize=None)
def loop_case(kind, k, max_dist):
    """kind 'same' (the target moved) or 'other' (seed 12 moved, Huber 0.1), true pose k, from the identity.  -> dict(source, truth, huber,
    ref = icp(...)).  Read only."""
    case = pair_case()
    truth = pose_matrix(*TRUE_POSES[k])
    source = moved(case["target"] if kind == "same" else case["other"], truth)
    huber = 0.0 if kind == "same" else HUBER_OTHER
    return dict(source=source, truth=truth, huber=huber,
                ref=icp(source, case["target"], case["normals"], None, max_dist, huber, LOOP_ITERS))


# ---- the ops' interface on the restatement (CPU stand-ins for tests of the file layer) -----------------------------------------------------
def ops_icp_point_to_plane(source, target, target_normals, pose=None, max_dist=1.0, huber=0.0, iters=30, tol_rot=1e-6, tol_trans=1e-6,
                           index=None, want_system=False):
    import torch
    from cmr_agent_amd import ops
    d = icp(source.cpu().numpy(), target.cpu().numpy(), target_normals.cpu().numpy(), None if pose is None else pose.cpu().numpy(), max_dist,
            huber, iters, tol_rot, tol_trans)
    return ops.IcpResult(torch.from_numpy(d["pose32"].copy()), d["pairs"], d["rmse"], d["iterations"], d["status"], torch.from_numpy(d["trace"]),
                         torch.from_numpy(d["system"]) if want_system else None)



# ---- a folder of prepared frames, as dataset/prepare.py lays it out: the one writer of the tests -----------------------------------------
def chained_frames(truths):
    """len(truths) + 1 prepared clouds float32 [7, n] from every fourth row of pair_case()'s target: frame j + 1 is frame j moved by the
    inverse of truths[j], in float64 all the way, reflectance zero."""
    case = pair_case()
    xyz, nrm = case["target"][::4].astype(np.float64), case["normals"][::4].astype(np.float64)
    frames = []
    for j in range(len(truths) + 1):
        frames.append(np.concatenate([xyz.T, np.zeros((1, xyz.shape[0])), nrm.T]).astype(F32))
        if j < len(truths):
            inv = np.linalg.inv(truths[j])
            xyz, nrm = xyz @ inv[:3, :3].T + inv[:3, 3], nrm @ inv[:3, :3].T
    return frames


def write_frames(root, frames, seq=9, first=3):
    """frames[j] -> <root>/vel/sequences/<seq>/<prepare.subdir()>/<first + j>.npy.  -> the folder"""
    import os

    from cmr_agent_amd.dataset import prepare
    folder = os.path.join(root, "vel", "sequences", "%02d" % seq, prepare.subdir())
    os.makedirs(folder)
    for j, f in enumerate(frames):
        np.save(os.path.join(folder, "%06d.npy" % (first + j)), f)
    return folder
