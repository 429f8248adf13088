"""Float64 numpy restatement of cmr_pnp_ransac_f32 (csrc/pnp.hip), step for step: the same compaction order, hash and
draws, the same Lambda Twist P3P and fourth-point choice, the same scoring rule, selection, Gauss-Newton and recount.  Differences by
design: everything here is float64 (the kernel scores in fp32 with K[R|t] rounded to fp32), and each residual is also returned so that a
test can count the correspondences whose residual lies within a small allowance of the threshold."""
import math

import numpy as np

MAX_DRAWS = 32
ORTH_TOL = 1e-5            # a P3P solution is kept only if max |R R^T - I| <= this
M32 = 0xFFFFFFFF


def mix(x):
    """lowbias32 (C. Wellons' 32-bit integer hash)."""
    x &= M32
    x ^= x >> 16
    x = (x * 0x21F0AAAD) & M32
    x ^= x >> 15
    x = (x * 0xD35A2D97) & M32
    x ^= x >> 15
    return x


def draw_hash(seed, b, h, c):
    return mix(mix(mix(mix(seed ^ 0x9E3779B9) ^ b) ^ h) ^ c)


def draws(seed, b, h, count):
    """The 4 distinct list positions of hypothesis h of sample b, or None when the counters run out or count < 4."""
    if count < 4:
        return None
    idx = []
    for c in range(MAX_DRAWS):
        if len(idx) == 4:
            break
        i = draw_hash(seed, b, h, c) % count
        if i not in idx:
            idx.append(i)
    return idx if len(idx) == 4 else None


def _cubic(c3, c2, c1, c0):
    a, b, c = c2 / c3, c1 / c3, c0 / c3
    p = b - a * a / 3.0
    q = 2.0 * a * a * a / 27.0 - a * b / 3.0 + c
    disc = q * q / 4.0 + p * p * p / 27.0
    if disc > 0.0:
        sd = math.sqrt(disc)
        r = [np.cbrt(-q / 2.0 + sd) + np.cbrt(-q / 2.0 - sd) - a / 3.0]
    else:
        m = math.sqrt(max(-p / 3.0, 0.0))
        arg = min(max(-q / (2.0 * m * m * m), -1.0), 1.0) if m > 0.0 else 0.0
        phi = math.acos(arg) / 3.0
        r = [2.0 * m * math.cos(phi - 2.0943951023931957 * k) - a / 3.0 for k in range(3)]
    out = []
    for g in r:
        for _ in range(2):
            f = ((c3 * g + c2) * g + c1) * g + c0
            d = (3.0 * c3 * g + 2.0 * c2) * g + c1
            if d != 0.0:
                g = g - f / d
        out.append(g)
    return out


def _eigvec(A, s):
    rows = A - s * np.eye(3)
    best, e = None, None
    for i, j in ((0, 1), (0, 2), (1, 2)):
        c = np.cross(rows[i], rows[j])
        n = float(c @ c)
        if best is None or n > best:
            best, e = n, c
    return e / math.sqrt(best)


def _cof(A):
    C = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            m = np.delete(np.delete(A, i, 0), j, 1)
            C[i, j] = (-1) ** (i + j) * (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0])
    return C


def p3p(x, y):
    """Lambda Twist P3P: x [3, 3] world points (rows), y [3, 3] unit bearings (rows) -> list of (R, t) with lambda_i y_i = R x_i + t."""
    d12, d13, d23 = x[0] - x[1], x[0] - x[2], x[1] - x[2]
    n123 = np.cross(d12, d13)
    a12, a13, a23 = d12 @ d12, d13 @ d13, d23 @ d23
    if not (n123 @ n123 > 1e-10 * a12 * a13):
        return []
    b12, b13, b23 = y[0] @ y[1], y[0] @ y[2], y[1] @ y[2]
    D1 = np.array([[a23, -a23 * b12, 0.0], [-a23 * b12, a23 - a12, a12 * b23], [0.0, a12 * b23, -a12]])
    D2 = np.array([[a23, 0.0, -a23 * b13], [0.0, -a13, a13 * b23], [-a23 * b13, a13 * b23, a23 - a13]])
    J1, J2 = _cof(D1).T, _cof(D2).T
    c3, c2, c1, c0 = np.linalg.det(D2), np.trace(J2 @ D1), np.trace(J1 @ D2), np.linalg.det(D1)
    if not (c3 != 0.0) or not np.isfinite(c3 + c2 + c1 + c0):
        return []
    bestq, D0, s1, s2 = 0.0, None, 0.0, 0.0
    for g in _cubic(c3, c2, c1, c0):
        A = D1 + g * D2
        tr = A[0, 0] + A[1, 1] + A[2, 2]
        m = (A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]) + (A[0, 0] * A[2, 2] - A[0, 2] * A[2, 0]) + (A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1])
        disc = tr * tr - 4.0 * m
        if not (m < 0.0) or not (disc >= 0.0):
            continue
        sq = math.sqrt(disc)
        ea, eb = 0.5 * (tr + sq), 0.5 * (tr - sq)
        q = -m / (ea * ea + eb * eb)
        if q > bestq:
            bestq, D0 = q, A
            s1, s2 = (ea, eb) if abs(ea) >= abs(eb) else (eb, ea)
    if D0 is None:
        return []
    e1, e2 = _eigvec(D0, s1), _eigvec(D0, s2)
    s = math.sqrt(-s2 / s1)
    X = np.stack([d12, d13, n123], 1)
    Xi = np.linalg.inv(X)
    sols = []
    for ss in (s, -s):
        n = e1 - ss * e2
        if not (abs(n[0]) > 1e-12 * math.sqrt(n @ n)):
            continue
        w0, w1 = -n[1] / n[0], -n[2] / n[0]
        qa = (a13 - a12) * w1 * w1 + 2.0 * a12 * b13 * w1 - a12
        qb = 2.0 * ((a13 - a12) * w0 * w1 - a13 * b12 * w1 + a12 * b13 * w0)
        qc = (a13 - a12) * w0 * w0 - 2.0 * a13 * b12 * w0 + a13
        disc = qb * qb - 4.0 * qa * qc
        if not (qa != 0.0) or not (disc >= 0.0):
            continue
        qq = -0.5 * (qb + math.copysign(math.sqrt(disc), qb))
        for tau in (qq / qa, qc / qq if qq != 0.0 else 0.0):
            if not (tau > 0.0):
                continue
            den = tau * tau - 2.0 * b23 * tau + 1.0
            if not (den > 0.0):
                continue
            l2 = math.sqrt(a23 / den)
            l3 = tau * l2
            l1 = w0 * l2 + w1 * l3
            if not (l1 > 0.0):
                continue
            r1, r2, r3 = l1 * y[0], l2 * y[1], l3 * y[2]
            yd1, yd2 = r1 - r2, r1 - r3
            Y = np.stack([yd1, yd2, np.cross(yd1, yd2)], 1)
            R = Y @ Xi
            sols.append((R, r1 - R @ x[0]))
    return sols


def hypothesis(corr, K, idx):
    """(R, t) of the hypothesis drawn at list positions idx, or None.  corr [n, 5] = X, Y, Z, u, v."""
    Ki = np.linalg.inv(K)
    P = corr[idx]
    x = P[:, 0:3]
    r = (Ki @ np.stack([P[:, 3], P[:, 4], np.ones(4)])).T
    y = r / np.linalg.norm(r, axis=1, keepdims=True)
    best, pick = 0.0, None
    with np.errstate(all="ignore"):
        for R, t in p3p(x[:3], y[:3]):
            pc = R @ x[3] + t
            p = K @ pc
            if not (pc[2] > 0.0):
                continue
            e = (p[0] / p[2] - P[3, 3]) ** 2 + (p[1] / p[2] - P[3, 4]) ** 2
            if not np.isfinite(e):
                continue
            if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))) or not (np.abs(R @ R.T - np.eye(3)).max() <= ORTH_TOL):
                continue
            if pick is None or e < best:
                best, pick = e, (R, t)
    if pick is None or not np.all(np.isfinite(K @ np.concatenate([pick[0], pick[1][:, None]], 1))):
        return None
    return pick


def residuals(corr, K, R, t):
    """Reprojection error per correspondence (inf where z <= 0)."""
    pc = corr[:, 0:3] @ R.T + t
    p = pc @ K.T
    with np.errstate(all="ignore"):
        e = np.sqrt((p[:, 0] / p[:, 2] - corr[:, 3]) ** 2 + (p[:, 1] / p[:, 2] - corr[:, 4]) ** 2)
    return np.where(pc[:, 2] > 0.0, e, np.inf)


def _expso3(w):
    th2 = float(w @ w)
    th = math.sqrt(th2)
    if th < 1e-8:
        a, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        a, c = math.sin(th) / th, (1.0 - math.cos(th)) / th2
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + a * W + c * (W @ W)


def gauss_newton(corr, K, R, t, refine_iters):
    """Gauss-Newton on the given correspondences with a left so(3) x R^3 increment; a step is kept only if the cost drops."""
    prev, cost_prev = None, 0.0
    for it in range(refine_iters + 1):
        pc = corr[:, 0:3] @ R.T + t
        p = pc @ K.T
        ok = p[:, 2] > 0.0
        pc, p, uv = pc[ok], p[ok], corr[ok, 3:5]
        iz = 1.0 / p[:, 2]
        pu, pv = p[:, 0] * iz, p[:, 1] * iz
        ru, rv = pu - uv[:, 0], pv - uv[:, 1]
        ga = (K[0][None, :] - pu[:, None] * K[2][None, :]) * iz[:, None]
        gb = (K[1][None, :] - pv[:, None] * K[2][None, :]) * iz[:, None]
        Ja = np.concatenate([np.cross(pc, ga), ga], 1)
        Jb = np.concatenate([np.cross(pc, gb), gb], 1)
        H = Ja.T @ Ja + Jb.T @ Jb
        g = Ja.T @ ru + Jb.T @ rv
        cost = float(ru @ ru + rv @ rv)
        if it > 0 and not (cost < cost_prev):
            return prev
        if it == refine_iters:
            return R, t
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            return R, t
        if not np.all(np.isfinite(L)):
            return R, t
        dx = np.linalg.solve(L.T, np.linalg.solve(L, -g))
        prev, cost_prev = (R, t), cost
        E = _expso3(dx[:3])
        R, t = E @ R, E @ t + dx[3:]
    return R, t


def compact(pts, uv, mask):
    """Selected rows of one sample in row order -> corr [n, 5] float64 (X, Y, Z, u, v)."""
    sel = np.nonzero(np.asarray(mask).reshape(-1) != 0)[0]
    return np.concatenate([np.asarray(pts, np.float64)[:, sel].T, np.asarray(uv, np.float64)[:, sel].T], 1)


def pnp_ransac(pts, uv, mask, K, n_hyp=1024, thr=1.0, seed=0, refine_iters=10, b=0, allowance=1e-3):
    """One sample (index b of its batch): pts [3, N], uv [2, N], mask [N], K [3, 3] -> dict(status, pose [4, 4], inliers, hyp_inliers
    [n_hyp] (-1 = invalid), near [n_hyp] (correspondences with |residual - thr| <= allowance), best, best_near, refined (bool),
    refine_margin (recount - hypothesis count), refine_near (near count of the refined pose), hyps [(R, t) or None])."""
    K = np.asarray(K, np.float64)
    corr = compact(pts, uv, mask)
    n = corr.shape[0]
    out = dict(status=0, pose=np.eye(4), inliers=0, hyp_inliers=np.full(n_hyp, -1, np.int64), near=np.zeros(n_hyp, np.int64),
               best=-1, best_near=0, refined=False, refine_margin=0, refine_near=0, hyps=[None] * n_hyp)
    if n < 4:
        out["status"] = 1
        return out
    res = [None] * n_hyp
    for h in range(n_hyp):
        idx = draws(seed, b, h, n)
        if idx is None:
            continue
        hyp = hypothesis(corr, K, idx)
        if hyp is None:
            continue
        out["hyps"][h] = hyp
        e = residuals(corr, K, *hyp)
        res[h] = e
        out["hyp_inliers"][h] = int((e <= thr).sum())
        out["near"][h] = int((np.abs(e - thr) <= allowance).sum())
    best = int(np.argmax(out["hyp_inliers"]))                          # argmax: the first of the maxima
    if out["hyp_inliers"][best] < 0:
        out["status"] = 2
        return out
    out["best"], out["best_near"] = best, int(out["near"][best])
    R, t = out["hyps"][best]
    hc = int(out["hyp_inliers"][best])
    inl = res[best] <= thr
    pose_R, pose_t, count = R, t, hc
    if refine_iters > 0:
        Rr, tr = gauss_newton(corr[inl], K, R, t, refine_iters)
        e = residuals(corr, K, Rr, tr)
        rc = int((e <= thr).sum())
        out["refine_margin"], out["refine_near"] = rc - hc, int((np.abs(e - thr) <= allowance).sum())
        if rc >= hc:
            pose_R, pose_t, count, out["refined"] = Rr, tr, rc, True
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = pose_R, pose_t
    out["pose"], out["inliers"] = P, count
    return out


def rotation_error_deg(Ra, Rb):
    """Angle between two rotations from the chordal distance, |Ra - Rb|_F = 2 sqrt(2) sin(angle / 2).  Unlike acos((tr(Ra Rb^T) - 1) / 2)
    it stays accurate near 0 for float32 matrices, whose rounding (~1e-7) would otherwise read as ~0.01 deg."""
    d = np.linalg.norm(np.asarray(Ra, np.float64) - np.asarray(Rb, np.float64))
    return math.degrees(2.0 * math.asin(min(1.0, d / (2.0 * math.sqrt(2.0)))))


def _rot(axis, ang):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return _expso3(axis * ang)


def planted(B, N, h, w, seed, outlier_frac=0.0, kind="6dof", noise=0.0):
    """Synthetic correspondences with known poses.  Camera-frame points whose exact projections fall inside the h x w map (depth 2-50),
    moved into the world frame by a random pose; P maps world -> camera (data['P']).  kind "6dof": any rotation, translation up to 10;
    "yaw": rotation about y in (-pi, pi) and (tx, 0, tz) in (-10, 10), the datasets' draw.  A fraction outlier_frac of the rows get a
    uniform pixel instead of their projection; noise: Gaussian pixel noise on the others.  -> dict of float64 numpy arrays pts [B,3,N],
    uv [B,2,N], K [B,3,3], P [B,4,4], inlier [B,N] bool."""
    rng = np.random.default_rng(seed)
    K = np.array([[0.6 * w, 0, w / 2.0], [0, 0.6 * w, h / 2.0], [0, 0, 1]])
    pts, uvs, Ps, inl = [], [], [], []
    for _ in range(B):
        u = rng.uniform(0, w - 1, N)
        v = rng.uniform(0, h - 1, N)
        z = rng.uniform(2, 50, N)
        cam = np.stack([(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z])
        if kind == "6dof":
            R = _rot(rng.normal(size=3), rng.uniform(-math.pi, math.pi))
            t = rng.uniform(-10, 10, 3)
        else:
            R = _rot([0, 1, 0], rng.uniform(-math.pi, math.pi))
            t = np.array([rng.uniform(-10, 10), 0.0, rng.uniform(-10, 10)])
        world = R.T @ (cam - t[:, None])                               # cam = R world + t
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = R, t
        uv = np.stack([u, v])
        if noise:
            uv = uv + rng.normal(scale=noise, size=uv.shape)
        out = rng.random(N) < outlier_frac
        uv[0, out] = rng.uniform(0, w - 1, int(out.sum()))
        uv[1, out] = rng.uniform(0, h - 1, int(out.sum()))
        pts.append(world)
        uvs.append(uv)
        Ps.append(P)
        inl.append(~out)
    return dict(pts=np.stack(pts), uv=np.stack(uvs), K=np.tile(K, (B, 1, 1)), P=np.stack(Ps), inlier=np.stack(inl))
