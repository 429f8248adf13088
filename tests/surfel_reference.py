"""Float64 restatement of oriented-disc (surfel) rendering (cmr_render_surfels_f32 / ops.render_surfels), written from the
contract in include/cmr_hip.h and independently of the kernel: brute force over every (row, pixel).  It is the yardstick of
tests/test_surfel_gpu.py and is itself checked on hand scenes by tests/test_surfel_cpu.py.

An fp32 evaluation and a float64 one may put a pixel that lies next to a disc's rim, or next to the grazing cap, on different sides, and
may round a centre next to a half-integer into different cells, which moves the window.  So the restatement returns DECIDED results, in
the manner of visibility_reference.py.  A (row, pixel) pair is MARGINAL when its rim test is within TEST_REL relative of r^2, its grazing
test within TEST_REL relative of equality, it lies where the candidate windows of an ambiguous centre (vr.EPS_PX) differ, or the row's
own drawn predicate is not decided (p2 or z_c - r next to 0); every other pair is SURE: covered or not.  A pixel is UNDECIDED when a
marginal pair's tau lies at or below the nearest sure depth plus twice the depth bar, or when its two nearest sure depths differ by no
more than twice the bar (an exact tie included: equal depths go to the lowest row, which only an exact evaluation can tell).
The depth bar of a pair is bar_c 2^-23 tau / min_cos + 8 2^-23 max_j S_j / min_cos with bar_c = 16, as derived in include/cmr_hip.h.

restate32 is the other yardstick: the per-pixel operations in numpy float32, one rounding each, started from the `surfel` output of the
op and the projected centres -- it must give the op's index_map and depth_map bit for bit."""
import math

import numpy as np
import torch

import visibility_reference as vr

TEST_REL = 1e-4
BAR_C = 16.0
DRAWN_REL = 1e-5


def _np(a):
    return np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)


def camera_ok(K):
    """The camera model the op assumes, per sample: K [3, 3]."""
    return bool(K[1, 0] == 0 and K[2, 0] == 0 and K[2, 1] == 0 and K[2, 2] == 1 and np.isfinite(K[0, 0]) and K[0, 0] > 0
                and np.isfinite(K[1, 1]) and K[1, 1] > 0)


def render(pts, normals, mask, pose, K, h, w, radius, range_slope, max_px, min_cos):
    """pts, normals [B, 3, N], mask [B, N] / [B*N] or None, pose [B, 4, 4], K [B, 3, 3] -> list over the samples of dict(status; sel [N];
    drawn_sure, drawn_maybe [N] bool; owner [h, w] int64 (-1: none) and depth [h, w] (the plain float64 answer: nearest sure-or-marginal
    covered pair by the exact tests, the lowest row on exact ties); decided [h, w] bool; owner_decided / depth_decided (valid where
    decided, from the sure pairs alone); bar [h, w] (the depth bar of the decided owner, 0 where none); undecided int; footprint [N]
    (covered pixels per row by the exact tests); full [N] bool (every map pixel of every candidate window of the row is covered with
    margin); counts_lo (selected, sure drawn rows))."""
    pts, normals = _np(pts).astype(np.float64), _np(normals).astype(np.float64)
    pose, K = _np(pose).astype(np.float64), _np(K).astype(np.float64)
    B, _, N = pts.shape
    mask = np.ones((B, N), bool) if mask is None else _np(mask).reshape(B, N) != 0
    radius, slope, mc = float(np.float32(radius)), float(np.float32(range_slope)), float(np.float32(min_cos))
    m = int(max_px)
    ys, xs = np.mgrid[0:h, 0:w]
    xs, ys = xs.ravel().astype(np.float64), ys.ravel().astype(np.float64)
    out = []
    for b in range(B):
        sel = mask[b]
        res = dict(sel=sel, status=0 if camera_ok(K[b]) else 1)
        owner, depth = np.full(h * w, -1, np.int64), np.full(h * w, math.inf)
        decided, owner_d, depth_d, bar_d = np.ones(h * w, bool), owner.copy(), depth.copy(), np.zeros(h * w)
        drawn_sure, drawn_maybe, footprint, full = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, np.int64), np.zeros(N, bool)
        if res["status"] == 0:
            fx, s, cx, fy, cy = K[b, 0, 0], K[b, 0, 1], K[b, 0, 2], K[b, 1, 1], K[b, 1, 2]
            with np.errstate(all="ignore"):
                R, t = pose[b, :3, :3], pose[b, :3, 3:4]
                X = R @ pts[b] + t
                n = R @ normals[b]
                S3 = (np.abs(R) @ np.abs(pts[b]) + np.abs(t)).max(0)
                S = vr.magnitude_sum(pts[b], pose[b], K[b])
                p = K[b] @ X
                z = p[2]
                u, v = p[0] / z, p[1] / z
                r = radius + slope * X[2]
                fin = np.isfinite(u) & np.isfinite(v) & np.isfinite(z)
                us, vs = np.where(fin, u, 0.0), np.where(fin, v, 0.0)
                cxl, cxh = np.rint(us - vr.EPS_PX), np.rint(us + vr.EPS_PX)
                cyl, cyh = np.rint(vs - vr.EPS_PX), np.rint(vs + vr.EPS_PX)
                front, behind = z > vr.P2_TOL * S, z < -vr.P2_TOL * S
                nfin = np.isfinite(normals[b]).all(0)
                gap = X[2] - r
                gap_yes, gap_no = gap > DRAWN_REL * (np.abs(X[2]) + S3), gap < -DRAWN_REL * (np.abs(X[2]) + S3)
                r_ok = np.isfinite(r) & (r > 0)
            touch = lambda ax, ay: (ax + m >= 0) & (ax - m <= w - 1) & (ay + m >= 0) & (ay - m <= h - 1)
            view_all = touch(cxl, cyl) & touch(cxl, cyh) & touch(cxh, cyl) & touch(cxh, cyh)
            view_any = touch(cxl, cyl) | touch(cxl, cyh) | touch(cxh, cyl) | touch(cxh, cyh)
            drawn_sure = sel & fin & front & view_all & nfin & r_ok & gap_yes
            drawn_maybe = sel & fin & ~behind & view_any & nfin & r_ok & ~gap_no & ~drawn_sure
            with np.errstate(all="ignore"):
                drawn_exact = sel & fin & (z > 0) & touch(np.rint(us), np.rint(vs)) & nfin & r_ok & (X[2] > r)
            rows = np.nonzero(drawn_sure | drawn_maybe)[0]
            best1, best2 = np.full(h * w, math.inf), np.full(h * w, math.inf)      # the two nearest sure depths
            marg = np.full(h * w, math.inf)                                          # the nearest marginal tau
            for i in rows:                                                           # brute force: every pixel of the map
                with np.errstate(all="ignore"):
                    dy = (ys - cy) / fy
                    dx = ((xs - cx) - s * dy) / fx
                    nx, ny, nz = n[:, i]
                    n2 = nx * nx + ny * ny + nz * nz
                    if n2 == 0:
                        tau = np.full(h * w, X[2, i])
                        oz = np.zeros(h * w)
                        ray_ok = graze_yes = graze_maybe = np.ones(h * w, bool)
                    else:
                        nd = nx * dx + ny * dy + nz
                        tau = (nx * X[0, i] + ny * X[1, i] + nz * X[2, i]) / nd
                        ray_ok = (nd != 0) & np.isfinite(tau) & (tau > 0)
                        lhs, rhs = nd * nd, mc * mc * n2 * (dx * dx + dy * dy + 1)
                        graze_yes, graze_maybe = lhs >= rhs * (1 + TEST_REL), lhs >= rhs * (1 - TEST_REL)
                        oz = tau - X[2, i]
                    ox, oy = tau * dx - X[0, i], tau * dy - X[1, i]
                    o2, r2 = ox * ox + oy * oy + oz * oz, r[i] * r[i]
                    rim_yes, rim_maybe = o2 <= r2 * (1 - TEST_REL), o2 <= r2 * (1 + TEST_REL)
                    graze_exact = graze_maybe if n2 == 0 else lhs >= rhs
                in_all = (xs >= cxh[i] - m) & (xs <= cxl[i] + m) & (ys >= cyh[i] - m) & (ys <= cyl[i] + m)
                in_any = (xs >= cxl[i] - m) & (xs <= cxh[i] + m) & (ys >= cyl[i] - m) & (ys <= cyh[i] + m)
                in_mid = (xs >= np.rint(us[i]) - m) & (xs <= np.rint(us[i]) + m) & (ys >= np.rint(vs[i]) - m) & (ys <= np.rint(vs[i]) + m)
                sure = ray_ok & graze_yes & rim_yes & in_all & bool(drawn_sure[i])
                maybe = ray_ok & graze_maybe & rim_maybe & in_any & ~sure
                exact = ray_ok & graze_exact & (o2 <= r2) & in_mid & bool(drawn_exact[i])
                footprint[i] = int(exact.sum())
                full[i] = bool((ray_ok & graze_yes & rim_yes)[in_any].all())
                take = exact & (tau < depth)                                         # rows ascend: a tie keeps the lower row
                owner[take], depth[take] = i, tau[take]
                bar = (BAR_C * tau + 8.0 * S3[i]) * 2.0 ** -23 / max(mc, 1e-30)
                ts = np.where(sure, tau, math.inf)
                first = ts < best1
                best2 = np.where(first, best1, np.minimum(best2, ts))
                owner_d = np.where(first, i, owner_d)
                bar_d = np.where(first, bar, bar_d)
                best1 = np.where(first, ts, best1)
                marg = np.minimum(marg, np.where(maybe, tau, math.inf))
            with np.errstate(all="ignore"):
                undecided = (np.isfinite(marg) & (marg <= best1 + 2 * bar_d)) | (np.isfinite(best1) & (best2 - best1 <= 2 * bar_d))
            decided = ~undecided
            depth_d = best1
            owner_d = np.where(np.isfinite(best1), owner_d, -1)
        res.update(owner=owner.reshape(h, w), depth=depth.reshape(h, w), decided=decided.reshape(h, w), owner_decided=owner_d.reshape(h, w),
                   depth_decided=depth_d.reshape(h, w), bar=bar_d.reshape(h, w), undecided=int((~decided).sum()), footprint=footprint, full=full,
                   drawn_sure=drawn_sure, drawn_maybe=drawn_maybe, counts_lo=[int(sel.sum()), int(drawn_sure.sum())])
        out.append(res)
    return out


def fma32(a, b, c):
    """fmaf on float32 arrays, exactly: the product of two float32 values is exact in float64; its sum with c is taken in float64 with
    the error of that sum (TwoSum) and rounded to odd, and a 53-bit value rounded to odd rounds to the correct 24-bit one."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        odd = (s.view(np.int64) & 1) == 1
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ~odd
        s = np.where(fix, np.nextafter(s, np.where((e > 0), np.inf, -np.inf)), s)
        return s.astype(np.float32)


def camera32(pts, normals, pose, radius, range_slope):
    """X_c, n_c and r of every row as the op computes them (cmr_project.h's chains; r = range_slope * z_c + radius, two roundings) from
    float32-representable pts, normals [B, 3, N] and pose [B, 4, 4] -> X [B, 3, N], n [B, 3, N], r [B, N] float32."""
    f = np.float32
    P, x, nr = _np(pose).astype(f), _np(pts).astype(f), _np(normals).astype(f)
    col = lambda j, k: P[:, j, k][:, None]
    with np.errstate(all="ignore"):
        X = np.stack([fma32(col(j, 0), x[:, 0], fma32(col(j, 1), x[:, 1], fma32(col(j, 2), x[:, 2], np.broadcast_to(col(j, 3), x[:, 2].shape)))) for j in range(3)], 1)
        n = np.stack([fma32(col(j, 0), nr[:, 0], fma32(col(j, 1), nr[:, 1], col(j, 2) * nr[:, 2])) for j in range(3)], 1)
        r = f(range_slope) * X[:, 2] + f(radius)
    assert X.dtype == f and n.dtype == f and r.dtype == f
    return X, n, r


def restate32(surfel, uv, K, h, w, max_px, min_cos):
    """The per-pixel operations in float32, one rounding each, from the op's `surfel` [B, 8, N] and the projected centres uv [B, 2, N]
    (ops.guided_match's proj) -> index_map int32 [B, h, w], depth_map float32 [B, h, w]."""
    f = np.float32
    surfel, uv, K = _np(surfel).astype(f), _np(uv).astype(f), _np(K).astype(f)
    B, _, N = surfel.shape
    m = int(max_px)
    mc = f(min_cos)
    index_map, depth_map = np.full((B, h, w), -1, np.int32), np.full((B, h, w), math.inf, f)
    off = np.arange(-m, m + 1)
    for b in range(B):
        rows = np.nonzero(surfel[b, 7] == 1)[0]
        if rows.size == 0:
            continue
        fx, s, cx, fy, cy = K[b, 0, 0], K[b, 0, 1], K[b, 0, 2], K[b, 1, 1], K[b, 1, 2]
        xc, yc, zc, nx, ny, nz, r = (surfel[b, k, rows][:, None, None] for k in range(7))
        ccx, ccy = np.rint(uv[b, 0, rows]).astype(np.int64), np.rint(uv[b, 1, rows]).astype(np.int64)
        x = (ccx[:, None, None] + off[None, None, :]) + 0 * off[None, :, None]
        y = (ccy[:, None, None] + off[None, :, None]) + 0 * off[None, None, :]
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        with np.errstate(all="ignore"):
            dy = (y.astype(f) - cy) / fy
            dx = ((x.astype(f) - cx) - s * dy) / fx
            n2 = (nx * nx + ny * ny) + nz * nz
            nd = (nx * dx + ny * dy) + nz
            nX = (nx * xc + ny * yc) + nz * zc
            flat = n2 == 0
            tau = np.where(flat, zc + 0 * dx, nX / nd).astype(f)
            ok = flat | ((nd != 0) & np.isfinite(tau) & (tau > 0) & (nd * nd >= ((mc * mc) * n2) * ((dx * dx + dy * dy) + f(1))))
            ox, oy = tau * dx - xc, tau * dy - yc
            oz = np.where(flat, f(0), tau - zc).astype(f)
            covered = ok & inside & ((ox * ox + oy * oy) + oz * oz <= r * r)
        assert all(a.dtype == f for a in (dy, dx, n2, nd, nX, tau, ox, oy, oz))
        key = (tau.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows[:, None, None].astype(np.uint64)
        keys = np.full(h * w, np.uint64(2 ** 64 - 1), np.uint64)
        np.minimum.at(keys, (y * w + x)[covered], key[covered])
        own = keys != np.uint64(2 ** 64 - 1)
        index_map[b].reshape(-1)[own] = (keys[own] & np.uint64(0xffffffff)).astype(np.int32)
        depth_map[b].reshape(-1)[own] = (keys[own] >> np.uint64(32)).astype(np.uint32).view(f)
    return index_map, depth_map


# ---- scenes of the GPU tier: visibility_reference.SCENES with normals ---------------------------------------------------------------------
# (scene, radius, range_slope, max_px); min_cos is MIN_COS throughout
PARAMS = {"n1025_13x19": (0.5, 0.05, 3), "n1025_40x128": (0.15, 0.03, 6), "n257_13x19_occ": (0.5, 0.05, 3), "n1_13x19": (0.5, 0.05, 3)}
MIN_COS = 0.1
_NORMALS, _REF = {}, {}


def normals_for(name):
    """Random normals for the named scene, float32-representable float64 [B, 3, N]: lengths 0.2 .. 3, about 10 % zero rows and, in clouds
    of more than 100 rows, three non-finite ones.  Built once and shared (do not modify)."""
    if name not in _NORMALS:
        sc = vr.built(name)
        B, _, N = sc["pts"].shape
        # the seed was settled on the restatement alone: under 900 two zero-normal wall discs 1e-4 apart in depth overlap, which leaves 64
        # pixels of one sample undecided by the tie rule; under 901 .. 904 no sample has more than 10
        rng = np.random.default_rng(901 + len(name) + N)
        n = rng.normal(size=(B, 3, N))
        n *= rng.uniform(0.2, 3.0, (B, 1, N)) / np.linalg.norm(n, axis=1, keepdims=True)
        n[np.broadcast_to(rng.random((B, 1, N)) < 0.1, n.shape)] = 0.0
        if N > 100:
            n[:, 0, 5], n[:, 1, 17], n[:, 2, 33] = math.nan, math.inf, -math.inf
        _NORMALS[name] = np.asarray(n, np.float32).astype(np.float64)
    return _NORMALS[name]


def reference(name):
    """render() of the named scene under PARAMS, every row selected by the scene's mask; computed once and shared."""
    if name not in _REF:
        sc = vr.built(name)
        radius, slope, m = PARAMS[name]
        _REF[name] = render(sc["pts"], normals_for(name), sc["mask"], sc["pose"], sc["K"], sc["h"], sc["w"], radius, slope, m, MIN_COS)
    return _REF[name]


def cap(pixels):
    return max(4, pixels // 100)


# The all-zero-normal comparison with ops.render_points(splat = max_px): (scene, max_px); r = ZERO_SLOPE z reaches ZERO_SLOPE f pixels
# (f = 0.6 w >= 11.4), more than (max_px + 1) sqrt(2), so the disc is the square window -- render()'s `full` confirms it with margin.
ZERO_CASES = [("n1025_13x19", 3), ("n1025_40x128", 4), ("n257_13x19_occ", 1), ("n1_13x19", 2)]
ZERO_SLOPE = 0.875

# The test of the window bound: large discs close to the camera and far off the axis, one per sample, on the hand map at max_px = 16,
# under the hand K, a K with skew and unequal focal lengths, and one four times as long (footprints of most of the map).  r = 0.625 z + 0.05: z_c - r is small beside r.
WINDOW_KS = [[[4.0, 0.0, 8.0], [0.0, 4.0, 8.0], [0.0, 0.0, 1.0]], [[4.0, 1.5, 8.0], [0.0, 3.0, 8.0], [0.0, 0.0, 1.0]],
             [[16.0, -3.0, 8.0], [0.0, 14.0, 8.0], [0.0, 0.0, 1.0]]]
WINDOW_B, WINDOW_RADIUS, WINDOW_SLOPE, WINDOW_MAX_PX = 48, 0.05, 0.625, 16


def window_scene(k):
    """-> pts, normals float32 [B, 3, 1], pose float64 [B, 4, 4] (identities), K float64 [B, 3, 3] = WINDOW_KS[k].  Of every five normals
    one is zero, two are random and two are tilted so that one side of the disc comes towards the camera: at a cosine of 0.15 .. 0.6 to
    the viewing ray.  That is where a footprint outgrows f r / z_c (tests/test_surfel_cpu.py counts the discs that do)."""
    K = WINDOW_KS[k]
    rng = np.random.default_rng(77)
    B = WINDOW_B
    z = rng.uniform(0.6, 3.0, B)
    spread = 12.0 / K[0][0]                                                         # centres up to 4 pixels outside the 17 x 17 map
    pts = np.stack([z * rng.uniform(-spread, spread, B), z * rng.uniform(-spread, spread, B), z])[None].transpose(2, 1, 0).copy()
    pts[0, :, 0] = (3.0, 1.0, 1.5)
    nrm = rng.normal(size=(B, 3, 1))
    ray = pts[:, :, 0] / np.linalg.norm(pts[:, :, 0], axis=1, keepdims=True)
    side = np.cross(ray, rng.normal(size=(B, 3)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    c = rng.uniform(0.15, 0.6, B)[:, None]
    tilted = (np.arange(B) % 5) >= 3
    nrm[tilted, :, 0] = (-c * ray + np.sqrt(1 - c * c) * side)[tilted]
    nrm[::5] = 0.0
    return np.asarray(pts, np.float32), np.asarray(nrm, np.float32), np.tile(np.eye(4), (B, 1, 1)), np.tile(np.asarray(K, np.float64), (B, 1, 1))


# ---- the hand scenes: identity pose, K = [[4, 0, 8], [0, 4, 8], [0, 0, 1]] on 17 x 17, dyadic numbers ----------------------------------------
HAND_H = HAND_W = 17
HAND_K = [[4.0, 0.0, 8.0], [0.0, 4.0, 8.0], [0.0, 0.0, 1.0]]


def hand(points, normals):
    """points, normals: lists of (x, y, z) -> pts, normals float32 [1, 3, n], pose [1, 4, 4], K [1, 3, 3] torch tensors."""
    p = torch.tensor(points, dtype=torch.float32).t()[None].contiguous()
    n = torch.tensor(normals, dtype=torch.float32).t()[None].contiguous()
    return p, n, torch.eye(4)[None].contiguous(), torch.tensor([HAND_K])
