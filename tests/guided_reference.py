"""Float64 restatement of pose-guided matching and of the pose refinement from a given pose (cmr_guided_match_f32 / cmr_pnp_refine_f32,
ops.guided_match / ops.pnp_refine), written from the contracts in include/cmr_hip.h and independently of the kernels:
explicit windows gathered with torch indexing, direct float64 distances, numpy Gauss-Newton.  It is the yardstick of
tests/test_guided_gpu.py and is itself checked, on planted scenes, by tests/test_guided_cpu.py.

guided match, per sample and selected row n: (u, v) = projection of the point under the pose; centre = rint (half to even); in view iff
p2 > 0, u and v finite and the (2r + 1)^2 window round the centre meets the map; idx = the pixel of the clipped window with the least L2
feature distance, lowest p on a tie; keep = in view and (max_dist <= 0 or dist <= max_dist); counts = (selected, in view, kept, kept and
inlier).  The window CENTRES may be handed in (`centres` = the (u, v) a device computed): a projection that lies 1e-5 from a half-integer
is then not a disagreement about which feature is nearest.  Beside the results it returns the float64 margins a decision hangs on: the
best / runner-up gap inside the window (it decides idx) and |dist - max_dist| (it decides keep); `near` = either is < TOL.

refine, per sample: working set = the selected rows within thr of their projection under pose_in (z > 0); up to `iters` Gauss-Newton
steps on it with pnp_reference.gauss_newton's accept / undo logic; recount over all selected rows; kept if the count does not drop.
status 0 refined, 1 fewer than 4 rows in the working set, 2 not kept (non-finite sums or failed FIRST factorisation -- a Cholesky pivot
<= PIVOT_TOL of its diagonal entry counts as failed -- or the recount dropped)."""
import math

import numpy as np
import torch

import match_filter_reference as mfr
import pnp_reference as pref

TOL = 1e-5           # the margin under which an fp32 decision may differ from the float64 one
CAP = 0.005          # at most this share of a sample's in-view rows may sit under TOL (a condition on the scenes, not a measurement)
PIVOT_TOL = 1e-13
ROW_CHUNK = 512      # in-view rows per gathered float64 block
ROUNDS = ((6, 4.0), (3, 2.0), (2, 1.0))
MAX_DIST = 0.6


# ---- guided match ------------------------------------------------------------------------------------------------------------------
def project(pts, pose, K):
    """pts [3, N], pose [4, 4], K [3, 3] (float64 numpy) -> u, v, p2 [N] (u, v NaN where p2 <= 0)."""
    xc = pose[:3, :3] @ pts + pose[:3, 3:4]
    p = K @ xc
    with np.errstate(all="ignore"):
        u, v = p[0] / p[2], p[1] / p[2]
    bad = ~(p[2] > 0)
    return np.where(bad, np.nan, u), np.where(bad, np.nan, v), p[2]


def guided_match(pts, pc, img, mask, pose, K, radius, max_dist=0.0, gt_xy=None, thr=3.0, centres=None):
    """pts [B, 3, N], pc [B*N, C], img [B, h, w, C], mask [B, N] / [B*N], pose [B, 4, 4], K [B, 3, 3], gt_xy [B, 2, N] or None, centres
    [B, 2, N] or None (torch tensors or numpy arrays of any float dtype) -> list over the samples of dict(sel [N] bool, view [N] bool,
    proj [2, N], idx [N] (-1 where not in view), dist [N] (NaN there), wmin [N] (the window minimum), gap [N] (runner-up - best inside the
    window, inf for a one-pixel window), keep [N] bool, inlier [N] bool, near [N] bool, counts [4] ints, dist_of: (rows, pixels) ->
    float64 distances)."""
    t64 = lambda a: torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).double()
    pts, pose, K, img, pc = t64(pts), t64(pose), t64(K), t64(img), t64(pc)
    B, h, w, C = img.shape
    N = pts.shape[2]
    mask = torch.as_tensor(np.asarray(mask.detach().cpu() if torch.is_tensor(mask) else mask)).reshape(B, N) != 0
    r = int(radius)
    off = torch.arange(-r, r + 1)
    oy, ox = torch.meshgrid(off, off, indexing="ij")                   # dy outer, dx inner: increasing p inside a window
    oy, ox = oy.reshape(-1), ox.reshape(-1)
    out = []
    for b in range(B):
        if centres is None:
            u, v, _ = project(pts[b].numpy(), pose[b].numpy(), K[b].numpy())
            u, v = torch.from_numpy(u), torch.from_numpy(v)
        else:
            u, v = t64(centres[b][0]), t64(centres[b][1])
        sel = mask[b]
        cx, cy = torch.from_numpy(np.rint(u.numpy())), torch.from_numpy(np.rint(v.numpy()))
        view = sel & torch.isfinite(u) & torch.isfinite(v) & (cx + r >= 0) & (cx - r <= w - 1) & (cy + r >= 0) & (cy - r <= h - 1)
        rows = torch.nonzero(view).flatten()
        idx = torch.full((N,), -1, dtype=torch.int64)
        dist = torch.full((N,), math.nan, dtype=torch.float64)
        wmin = torch.full((N,), math.nan, dtype=torch.float64)
        gap = torch.full((N,), math.inf, dtype=torch.float64)
        Q = img[b].reshape(h * w, C)
        F = pc[b * N:(b + 1) * N]
        for c0 in range(0, rows.numel(), ROW_CHUNK):
            rr = rows[c0:c0 + ROW_CHUNK]
            x = cx[rr].long()[:, None] + ox[None, :]
            y = cy[rr].long()[:, None] + oy[None, :]
            ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            p = y.clamp(0, h - 1) * w + x.clamp(0, w - 1)
            d = ((F[rr][:, None, :] - Q[p]) ** 2).sum(-1).sqrt()
            d = torch.where(ok, d, torch.full_like(d, math.inf))
            lo = d.min(1).values
            first = (d == lo[:, None]).to(torch.uint8).argmax(1)       # the FIRST (lowest p) pixel that attains the minimum
            idx[rr] = p[torch.arange(rr.numel()), first]
            dist[rr] = lo
            wmin[rr] = lo
            if d.shape[1] > 1:
                gap[rr] = d.topk(2, dim=1, largest=False).values[:, 1] - lo
        keep = view.clone()
        near = view & (gap < TOL)
        if max_dist > 0:
            keep &= dist <= max_dist
            near |= view & ((dist - max_dist).abs() < TOL)
        inl = torch.zeros(N, dtype=torch.bool)
        if gt_xy is not None:
            g = t64(gt_xy[b])
            px, py = (idx % w).double(), torch.div(idx, w, rounding_mode="floor").double()
            inl = view & torch.isfinite(g[0]) & torch.isfinite(g[1]) & (((px - g[0]) ** 2 + (py - g[1]) ** 2).sqrt() <= thr)

        def dist_of(rows_, pixels, F=F, Q=Q):
            return ((F[rows_] - Q[pixels]) ** 2).sum(-1).sqrt()

        out.append(dict(sel=sel, view=view, proj=torch.stack([u, v]), idx=idx, dist=dist, wmin=wmin, gap=gap, keep=keep, inlier=inl,
                        near=near, counts=[int(sel.sum()), int(view.sum()), int(keep.sum()), int((keep & inl).sum())], dist_of=dist_of))
    return out


# ---- refinement ----------------------------------------------------------------------------------------------------------------------
def _chol_ok(H):
    """Cholesky factor of H, or None when H is not positive definite or a pivot is <= PIVOT_TOL of its diagonal entry."""
    if not np.all(np.isfinite(H)):
        return None
    try:
        L = np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return None
    d = np.diag(L) ** 2
    if not np.all(np.isfinite(L)) or not np.all(d > PIVOT_TOL * np.diag(H)):
        return None
    return L


def _normal_equations(corr, K, R, t):
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
    return Ja.T @ Ja + Jb.T @ Jb, Ja.T @ ru + Jb.T @ rv, float(ru @ ru + rv @ rv)


def gauss_newton(corr, K, R, t, iters):
    """pnp_reference.gauss_newton's loop (left so(3) x R^3 increment, a step kept only if the next cost is lower) with the first
    factorisation's outcome reported: -> (R, t, ok); ok False when the sums are non-finite or the first factorisation fails."""
    prev, cost_prev = None, 0.0
    for it in range(iters + 1):
        with np.errstate(all="ignore"):
            H, g, cost = _normal_equations(corr, K, R, t)
        if it == 0 and not (np.all(np.isfinite(H)) and np.all(np.isfinite(g)) and np.isfinite(cost)):
            return R, t, False
        if it > 0 and not (cost < cost_prev):
            return prev[0], prev[1], True
        if it == iters:
            return R, t, True
        L = _chol_ok(H)
        dx = None if L is None else np.linalg.solve(L.T, np.linalg.solve(L, -g))
        if dx is not None:
            E = pref._expso3(dx[:3])
            Rn, tn = E @ R, E @ t + dx[3:]
            if not (np.all(np.isfinite(Rn)) and np.all(np.isfinite(tn))):
                dx = None
        if dx is None:
            return R, t, it > 0
        prev, cost_prev = (R, t), cost
        R, t = Rn, tn
    return R, t, True


def refine(pts, uv, mask, K, pose_in, thr=1.0, iters=10, allowance=1e-3):
    """One sample: pts [3, N], uv [2, N], mask [N], K [3, 3], pose_in [4, 4] (float64 numpy) -> dict(pose [4, 4], inliers, status, wset
    (size of the working set), near_in / near_out (selected rows whose residual under pose_in / under the refined pose lies within
    `allowance` of thr), margin (recount - wset))."""
    K, pose_in = np.asarray(K, np.float64), np.asarray(pose_in, np.float64)
    corr = pref.compact(pts, uv, mask)
    R, t = pose_in[:3, :3], pose_in[:3, 3]
    e = pref.residuals(corr, K, R, t) if corr.shape[0] else np.zeros(0)
    inl = e <= thr
    ws = int(inl.sum())
    out = dict(pose=pose_in.copy(), inliers=ws, status=0, wset=ws, near_in=int((np.abs(e - thr) <= allowance).sum()), near_out=0, margin=0)
    if ws < 4:
        out["status"] = 1
        return out
    if iters == 0:
        return out
    Rr, tr, ok = gauss_newton(corr[inl], K, R, t, iters)
    if not ok:
        out["status"] = 2
        return out
    e2 = pref.residuals(corr, K, Rr, tr)
    rc = int((e2 <= thr).sum())
    out["near_out"], out["margin"] = int((np.abs(e2 - thr) <= allowance).sum()), rc - ws
    if rc >= ws and np.all(np.isfinite(Rr)) and np.all(np.isfinite(tr)):
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = Rr, tr
        out["pose"], out["inliers"] = P, rc
    else:
        out["status"] = 2
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def blurred_map(B, h, w, g, blur=5):
    """Pixel features as match_filter_reference.planted_scene makes them: N(0, I) per pixel, blur x blur box blur, renormalised (float64)."""
    img = torch.randn(B, h, w, 64, generator=g, dtype=torch.float64)
    img = torch.nn.functional.avg_pool2d(img.permute(0, 3, 1, 2), blur, stride=1, padding=blur // 2, count_include_pad=False).permute(0, 2, 3, 1)
    return torch.nn.functional.normalize(img, dim=-1)


def perturbed(P, rng, angle_deg=1.5, sigma=0.15):
    """(dR R, dR t + sigma N(0, I)) with dR a rotation of angle_deg about a random axis."""
    out = np.array(P, np.float64)
    for b in range(out.shape[0]):
        dR = pref._rot(rng.normal(size=3), math.radians(angle_deg))
        out[b, :3, :3] = dR @ P[b, :3, :3]
        out[b, :3, 3] = dR @ P[b, :3, 3] + sigma * rng.normal(size=3)
    return out


def scene(B, N, h, w, seed, noise=0.08, outlier_frac=0.3, features="planted"):
    """Planted geometry (pnp_reference.planted, kind "yaw") carrying features.  "planted": a blurred unit feature map; point n = the
    feature at its ROUNDED TRUE pixel + noise * N(0, I), a fraction outlier_frac of the points replaced by random unit vectors,
    renormalised.  "random": unrelated random unit features on both sides (match_filter_reference.unit).  Start pose: the truth turned by
    1.5 deg about a random axis and moved by 0.15 N(0, I).  Everything the device sees is float32; the float64 fields hold the same values.
    -> dict(pts [B,3,N], K [B,3,3], P [B,4,4], start [B,4,4], uv [B,2,N] (true projections) float64 numpy; pc float32 [B*N,64], img
    float32 [B,h,w,64], mask bool [B,N], gt_xy float32 [B,2,N], planted bool [B,N])."""
    s = pref.planted(B, N, h, w, seed, kind="yaw")
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    g = torch.Generator(device="cpu").manual_seed(seed)
    rng = np.random.default_rng(seed + 7919)
    pix = torch.from_numpy((np.rint(s["uv"][:, 1]) * w + np.rint(s["uv"][:, 0])).astype(np.int64))
    if features == "planted":
        img = blurred_map(B, h, w, g)
        feat = img.reshape(B, h * w, 64).gather(1, pix[..., None].expand(B, N, 64)) + noise * torch.randn(B, N, 64, generator=g, dtype=torch.float64)
        out = torch.rand(B, N, generator=g) < outlier_frac
        feat = torch.where(out[..., None], torch.randn(B, N, 64, generator=g, dtype=torch.float64), feat)
        feat = torch.nn.functional.normalize(feat, dim=-1)
    else:
        img = mfr.unit(B, h, w, 64, seed=seed + 2).double()
        feat = mfr.unit(B, N, 64, seed=seed + 1).double()
        out = torch.ones(B, N, dtype=torch.bool)
    return dict(pts=f32(s["pts"]), K=f32(s["K"]), P=s["P"], start=f32(perturbed(s["P"], rng)), uv=s["uv"],
                pc=feat.reshape(B * N, 64).float().contiguous(), img=img.float().contiguous(), mask=torch.ones(B, N, dtype=torch.bool),
                gt_xy=torch.from_numpy(s["uv"]).float().contiguous(), planted=~out)


def refine_rounds(sc, rounds=ROUNDS, max_dist=MAX_DIST, iters=10, start=None):
    """The pipeline of MultiHeadModel.refine_pose_from_matches in float64 on a scene: for each (radius, thr): guided match under the
    current pose, correspondences = kept rows with uv = the matched pixel, refine from the current pose.
    -> (poses [B, 4, 4], per round and sample: dict(match=..., refine=...))."""
    B, _, N = sc["pts"].shape
    h, w = sc["img"].shape[1:3]
    cur = np.array(sc["start"] if start is None else start, np.float64)
    log = []
    for radius, thr in rounds:
        m = guided_match(sc["pts"], sc["pc"], sc["img"], sc["mask"], cur, sc["K"], radius, max_dist=max_dist, gt_xy=sc["gt_xy"])
        row = []
        for b in range(B):
            p = m[b]["idx"].clamp(min=0).numpy()
            uv = np.stack([p % w, p // w]).astype(np.float64)
            r = refine(sc["pts"][b], uv, m[b]["keep"].numpy(), sc["K"][b], cur[b], thr=thr, iters=iters)
            cur[b] = r["pose"]
            row.append(dict(match=m[b], refine=r))
        log.append(row)
    return cur, log


def pose_errors(pose, P):
    """-> (rotation errors in degrees, translation errors) per sample."""
    pose, P = np.asarray(pose, np.float64), np.asarray(P, np.float64)
    return ([pref.rotation_error_deg(pose[b, :3, :3], P[b, :3, :3]) for b in range(len(P))],
            [float(np.linalg.norm(pose[b, :3, 3] - P[b, :3, 3])) for b in range(len(P))])


def refine_scene(B, N, seed, outlier_frac=0.0, h=88, w=304):
    """Planted correspondences for the refine parity tests, built so that no residual sits near thr = 1 under pose_in: inliers = the true
    projection + noise of at most 0.3 px (uniform in a disc), pose_in = the truth turned by 0.01 deg and moved by 0.002 N(0, I) (a few
    tenths of a pixel), outliers = pose_in's projection moved by 3 .. 50 px in a random direction.  All values are float32-representable.
    -> dict(pts [B,3,N], uv [B,2,N], K [B,3,3], P [B,4,4], pose_in [B,4,4] float64 numpy, inlier [B,N] bool)."""
    s = pref.planted(B, N, h, w, seed)
    rng = np.random.default_rng(seed + 104729)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    pts, K = f32(s["pts"]), f32(s["K"])
    pose_in = f32(perturbed(s["P"], rng, angle_deg=0.01, sigma=0.002))
    uv = np.empty_like(s["uv"])
    inl = np.empty((B, N), bool)
    for b in range(B):
        ut, vt, _ = project(pts[b], s["P"][b], K[b])
        ui, vi, _ = project(pts[b], pose_in[b], K[b])
        rad, ang = 0.3 * np.sqrt(rng.random(N)), rng.uniform(0, 2 * math.pi, N)
        out = rng.random(N) < outlier_frac
        far, fang = rng.uniform(3.0, 50.0, N), rng.uniform(0, 2 * math.pi, N)
        uv[b, 0] = np.where(out, ui + far * np.cos(fang), ut + rad * np.cos(ang))
        uv[b, 1] = np.where(out, vi + far * np.sin(fang), vt + rad * np.sin(ang))
        inl[b] = ~out
    return dict(pts=pts, uv=f32(uv), K=K, P=s["P"], pose_in=pose_in, inlier=inl)


def collinear_case(N):
    """Every point on one line (integers: exactly collinear in float32 and float64) with exact projections under the pose handed in: the
    normal matrix has a one-dimensional null space (turning about the line), the first factorisation fails, status 2.
    -> pts [3, N], uv [2, N], K [3, 3], pose [4, 4] (float32-representable float64)."""
    k = np.arange(N, dtype=np.float64)
    pts = np.stack([k - 20.0, 2.0 * k - 30.0, 10.0 + k])
    K = np.array([[182.0, 0, 152], [0, 182.0, 44], [0, 0, 1]])
    P = np.eye(4)
    u, v, _ = project(pts, P, K)
    return pts, np.asarray(np.stack([u, v]), np.float32).astype(np.float64), K, P


# The scenes of the GPU tier's guided-match comparison: (name, kwargs of scene(), window radii, max_dist).  tests/test_guided_cpu.py
# asserts CAP on every one of them from the restatement alone.
MATCH_SCENES = [
    ("planted_201", dict(B=2, N=4096, h=40, w=128, seed=201), (0, 1, 4, 8), MAX_DIST),
    ("planted_202", dict(B=2, N=4096, h=40, w=128, seed=202), (0, 1, 4, 8), MAX_DIST),
    ("planted_203", dict(B=2, N=4096, h=40, w=128, seed=203), (0, 1, 4, 8), MAX_DIST),
    ("random_88x304", dict(B=2, N=4097, h=88, w=304, seed=211, features="random"), (0, 1, 4, 8), 1.2),
]
REFINE_SIZES = (100, 4097, 65536)
# ops.pnp_refine against cmr_pnp_ransac_f32's own refinement: pnp_reference.planted(B, N, 88, 304, seed, outlier_frac=0.3, noise=0.3),
# RANSAC seed 5, thr 1; the seeds were chosen on the CPU (tests/test_guided_cpu.py keeps the condition: at least half of the samples
# have no residual within 1e-3 px of thr under the unrefined winner)
AGREE_SHAPE = (4, 2048, 128)       # B, N, n_hyp
AGREE_SEEDS = (61, 62)
