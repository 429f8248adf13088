"""Float64 restatement of point visibility and depth rendering under a pose (cmr_visibility_f32 / ops.visibility), written
from the contract in include/cmr_hip.h and independently of the kernels.  It is the yardstick of tests/test_visibility_gpu.py and is
itself checked, on a scene small enough to do by hand, by tests/test_visibility_cpu.py.

An fp32 evaluation and a float64 one may round a projection that lies next to a half-integer into different cells, and may order two
depths that agree to a few ulp differently.  So the restatement returns DECIDED flags: what every faithful evaluation must give.
  * a coordinate within EPS_PX of a half-integer has two candidate centres (fp32 projection error is about 1e-4 px at u = 300 and
    3e-4 px at u = 1216); a row with more than one candidate centre is AMBIGUOUS;
  * Z_lo: ambiguous occluders are splatted into every candidate cell -- no evaluation's z-buffer lies below it by more than rounding;
    Z_hi: ambiguous occluders are left out -- none lies above it;
  * a queried row is decided VISIBLE if z (1 + REL) <= bound(min Z_lo over the union of the windows of its candidate centres) and decided
    OCCLUDED if z (1 - REL) > bound(min Z_hi over their intersection), REL = 1e-5; in both cases it must be in view under all of its
    candidates.  A selected row that is out of view under all of them (or clearly behind the camera) is decided not visible; an unselected
    row is decided not visible.  Every other row is UNDECIDED.
  * a depth_map cell is decided if no ambiguous occluder has it as a candidate.
bound(zmin) = zmin * opr + abs_tol with opr = (float32)(1 + rel_tol) and abs_tol as rounded to float32: the arguments as the op sees them."""
import math

import numpy as np
import torch

EPS_PX = 1e-3
REL = 1e-5
P2_TOL = 1e-5        # |p2| <= P2_TOL * S (S = the sum of magnitudes behind p2): the sign of p2 is not decided


def _np(a):
    return np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)


def opr32(rel_tol):
    """opr as the op forms it: rel_tol arrives as a float32, 1 + rel_tol is taken in float64 and rounded to float32."""
    return np.float32(1.0 + float(np.float32(rel_tol)))


def magnitude_sum(pts, pose, K):
    """S = sum_j |K_2j| (sum_k |R_jk| |x_k| + |t_j|) per row: the scale of the rounding error of z = p2.  pts [3, N] -> [N]."""
    ax = np.abs(pose[:3, :3]) @ np.abs(pts) + np.abs(pose[:3, 3:4])
    return np.abs(K[2]) @ ax


def _window_min(Z, x0, x1, y0, y1):
    """min of Z[y0..y1, x0..x1] per row (inclusive integer bounds, clipped to the map here); +inf for an empty range."""
    h, w = Z.shape
    x0, x1, y0, y1 = np.maximum(x0, 0), np.minimum(x1, w - 1), np.maximum(y0, 0), np.minimum(y1, h - 1)
    out = np.full(x0.shape, math.inf)
    if x0.size == 0:
        return out
    for dy in range(max(int((y1 - y0).max()) + 1, 0)):
        for dx in range(max(int((x1 - x0).max()) + 1, 0)):
            x, y = x0 + dx, y0 + dy
            ok = (x <= x1) & (y <= y1)
            out = np.minimum(out, np.where(ok, Z[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], math.inf))
    return out


def visibility(pts, mask, occ_mask, pose, K, h, w, radius, rel_tol, abs_tol):
    """pts [B, 3, N], mask / occ_mask [B, N] or [B*N] (occ_mask None: every row), pose [B, 4, 4], K [B, 3, 3] -> list over the samples of
    dict(sel, occ [N] bool; z [N] float64 (p2); S [N]; cand (cxl, cxh, cyl, cyh) int64 [N]; amb [N] bool (more than one candidate centre or
    an undecided sign of p2); view_all / view_any [N] bool (in view under all / any candidates); decided [N] bool; visible [N] bool (valid
    where decided); undecided int (selected rows); Z_lo, Z_hi [h, w]; cell_decided [h, w] bool; err_map [h, w] (the largest 8 2^-23 S of
    the occluders of a cell, 0 where none); counts_lo [4] (rows decided to count), occ_amb int (ambiguous occluders that may be in view))."""
    pts, pose, K = _np(pts).astype(np.float64), _np(pose).astype(np.float64), _np(K).astype(np.float64)
    B, _, N = pts.shape
    mask = _np(mask).reshape(B, N) != 0
    occ_mask = np.ones((B, N), bool) if occ_mask is None else _np(occ_mask).reshape(B, N) != 0
    opr, atol, r = float(opr32(rel_tol)), float(np.float32(abs_tol)), int(radius)
    bound = lambda zmin: zmin * opr + atol
    out = []
    for b in range(B):
        sel, occ = mask[b], occ_mask[b]
        with np.errstate(all="ignore"):
            xc = pose[b, :3, :3] @ pts[b] + pose[b, :3, 3:4]
            p = K[b] @ xc
            S = magnitude_sum(pts[b], pose[b], K[b])
            z = p[2]
            u, v = p[0] / p[2], p[1] / p[2]
            front = z > P2_TOL * S                                           # clearly in front; NaN compares false
            behind = z < -P2_TOL * S
            fin = np.isfinite(u) & np.isfinite(v) & np.isfinite(z)
            us, vs = np.where(fin, u, 0.0), np.where(fin, v, 0.0)
            cxl, cxh = np.rint(us - EPS_PX).astype(np.int64), np.rint(us + EPS_PX).astype(np.int64)
            cyl, cyh = np.rint(vs - EPS_PX).astype(np.int64), np.rint(vs + EPS_PX).astype(np.int64)
        sign_amb = fin & ~front & ~behind
        amb = fin & ((cxl != cxh) | (cyl != cyh) | sign_amb)
        inx = lambda c: (c >= 0) & (c <= w - 1)
        iny = lambda c: (c >= 0) & (c <= h - 1)
        view_all = fin & front & inx(cxl) & inx(cxh) & iny(cyl) & iny(cyh)
        view_any = fin & ~behind & (inx(cxl) | inx(cxh)) & (iny(cyl) | iny(cyh))
        # the two z-buffers
        Z_lo, Z_hi = np.full((h, w), math.inf), np.full((h, w), math.inf)
        err_map, cell_decided = np.zeros((h, w)), np.ones((h, w), bool)
        sure = occ & view_all & ~amb
        np.minimum.at(Z_hi, (cyl[sure], cxl[sure]), z[sure])
        np.minimum.at(Z_lo, (cyl[sure], cxl[sure]), z[sure])
        np.maximum.at(err_map, (cyl[sure], cxl[sure]), 8.0 * 2.0 ** -23 * S[sure])
        maybe = occ & view_any & amb
        for cx in (cxl, cxh):
            for cy in (cyl, cyh):
                m = maybe & inx(cx) & iny(cy)
                np.minimum.at(Z_lo, (cy[m], cx[m]), np.maximum(z[m], 0.0))
                cell_decided[cy[m], cx[m]] = False
        # the test
        vis_yes = np.zeros(N, bool)
        vis_no = sel & ~view_any | ~sel                                          # decided not visible without a depth test
        q = np.nonzero(sel & view_all & ~sign_amb)[0]
        lo = _window_min(Z_lo, cxl[q] - r, cxh[q] + r, cyl[q] - r, cyh[q] + r)
        hi = _window_min(Z_hi, cxh[q] - r, cxl[q] + r, cyh[q] - r, cyl[q] + r)
        vis_yes[q] = z[q] * (1.0 + REL) <= bound(lo)
        vis_no[q] = z[q] * (1.0 - REL) > bound(hi)
        decided = vis_yes | vis_no
        view_decided = ~sel | ~view_any | (view_all & ~sign_amb)
        out.append(dict(sel=sel, occ=occ, z=z, S=S, cand=(cxl, cxh, cyl, cyh), amb=amb, view_all=view_all, view_any=view_any,
                        decided=decided, visible=vis_yes, undecided=int((sel & ~decided).sum()), Z_lo=Z_lo, Z_hi=Z_hi,
                        cell_decided=cell_decided, err_map=err_map,
                        counts_lo=[int(sel.sum()), int((sel & view_all & ~sign_amb).sum()), int(vis_yes.sum()), int(sure.sum())],
                        view_undecided=int((~view_decided).sum()), occ_amb=int(maybe.sum())))
    return out


# ---- the hand-checkable scene ----------------------------------------------------------------------------------------------------------
HAND_H, HAND_W = 8, 10
# (x, y, depth) of the rows; K and the pose are identities, so the point (x z, y z, z) projects to (x, y) at depth z
HAND_ROWS = [
    (3, 2, 2.0),       # 0  near
    (3, 2, 5.0),       # 1  directly behind row 0: occluded at every radius
    (4, 2, 5.0),       # 2  one cell beside row 0: visible at r = 0, occluded at r = 1
    (7, 4, 2.0),       # 3  near
    (7, 4, 2.08),      # 4  in row 3's cell and within rel_tol = 0.05 of it (2.08 <= 2.1): visible
    (12, 3, 3.0),      # 5  outside the map: neither visible nor an occluder
    (3, 2, -1.0),      # 6  behind the camera (it would project to row 0's cell): neither
    (9, 7, 3.0),       # 7  the map's corner, its window clipped: visible at r = 0, occluded by row 8 at r = 1
    (9, 6, 1.0),       # 8  near, above the corner
    (0, 0, 6.0),       # 9  the other corner, alone: visible at every radius
]
HAND_VISIBLE = {0: [1, 0, 1, 1, 1, 0, 0, 1, 1, 1], 1: [1, 0, 0, 1, 1, 0, 0, 0, 1, 1], 16: [0, 0, 0, 0, 0, 0, 0, 0, 1, 0]}
HAND_COUNTS = {0: [10, 8, 7, 8], 1: [10, 8, 5, 8], 16: [10, 8, 1, 8]}      # radius 16 covers the whole 8 x 10 map: only the nearest point stays
HAND_REL_TOL = 0.05


def hand():
    """-> pts float32 [1, 3, 10], pose float32 [1, 4, 4], K float32 [1, 3, 3] (identities)."""
    rows = np.array(HAND_ROWS, np.float64)
    pts = np.stack([rows[:, 0] * rows[:, 2], rows[:, 1] * rows[:, 2], rows[:, 2]])[None]
    return torch.from_numpy(pts).float().contiguous(), torch.eye(4)[None].contiguous(), torch.eye(3)[None].contiguous()


def hand_depth_map():
    """The z-buffer of the hand scene with every row occluding -> float32 [1, 8, 10]."""
    Z = torch.full((1, HAND_H, HAND_W), math.inf)
    for x, y, z in HAND_ROWS:
        if z > 0 and 0 <= x < HAND_W and 0 <= y < HAND_H:
            Z[0, y, x] = min(float(Z[0, y, x]), float(np.float32(z)))
    return Z


# ---- scenes of the GPU tier ------------------------------------------------------------------------------------------------------------
def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


def _camera(B, h, w, rng):
    """A pose per sample (a turn of up to 20 degrees about a random axis, a shift of a few units) and K with the principal point at the
    map's middle and a focal length of 0.6 w -> P [B, 4, 4], K [B, 3, 3] float64, float32-representable."""
    P, K = np.tile(np.eye(4), (B, 1, 1)), np.zeros((B, 3, 3))
    for b in range(B):
        P[b, :3, :3] = _rot(rng.normal(size=3), math.radians(rng.uniform(5, 20)))
        P[b, :3, 3] = rng.normal(size=3) * 2.0
        K[b] = [[0.6 * w, 0, (w - 1) / 2], [0, 0.6 * w, (h - 1) / 2], [0, 0, 1]]
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    return f32(P), f32(K)


def _lift(u, v, z, P, K):
    """Points of the cloud whose projection under (P, K) is (u, v) at depth z -> [3, n] float64."""
    xc = np.linalg.inv(K) @ np.stack([u * z, v * z, z])
    return P[:3, :3].T @ (xc - P[:3, 3:4])


def scene(B, N, h, w, seed, selected=0.6, occluding=None):
    """Uniform projections over the map and a margin round it, depth 2 .. 50, 5 % of the rows behind the camera, plus a planted wall: a
    quarter of the rows at depth 3 .. 3.3 over the map's middle third.  mask: a random `selected` share; occ_mask: None (every row) or a
    random `occluding` share.  Everything the device sees is float32; the float64 fields hold the same values.
    -> dict(pts [B,3,N], pose [B,4,4], K [B,3,3] float64 numpy; mask bool [B,N]; occ_mask bool [B,N] or None; h, w)."""
    rng = np.random.default_rng(seed)
    P, K = _camera(B, h, w, rng)
    pts = np.empty((B, 3, N))
    for b in range(B):
        u, v = rng.uniform(-0.1 * w, 1.1 * w, N), rng.uniform(-0.1 * h, 1.1 * h, N)
        z = rng.uniform(2.0, 50.0, N)
        wall = rng.random(N) < 0.25
        u = np.where(wall, rng.uniform(w / 3, 2 * w / 3, N), u)
        z = np.where(wall, rng.uniform(3.0, 3.3, N), z)
        z = np.where(rng.random(N) < 0.05, -z, z)
        pts[b] = _lift(u, v, z, P[b], K[b])
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(B, N, generator=g) < selected
    occ = None if occluding is None else torch.rand(B, N, generator=g) < occluding
    return dict(pts=np.asarray(pts, np.float32).astype(np.float64), pose=P, K=K, mask=mask, occ_mask=occ, h=h, w=w)


# The scenes of the GPU tier's float64 comparison: (name, kwargs of scene(), radii).  tests/test_visibility_cpu.py asserts the cap on the
# undecided rows -- at most max(4, 1 %) of a sample's selected rows -- on every one of them, from the restatement alone.
REL_TOL, ABS_TOL = 0.05, 0.0
SCENES = [
    ("n1025_13x19", dict(B=3, N=1025, h=13, w=19, seed=301), (0, 1, 2, 16)),
    ("n1025_40x128", dict(B=3, N=1025, h=40, w=128, seed=302), (0, 1, 2, 16)),
    ("n257_13x19_occ", dict(B=3, N=257, h=13, w=19, seed=303, occluding=0.5), (0, 1, 2, 16)),
    ("n1_13x19", dict(B=3, N=1, h=13, w=19, seed=304, selected=1.0), (0, 1)),
]
_BUILT = {}


def built(name):
    """The named scene, built once and shared (do not modify it)."""
    if name not in _BUILT:
        _BUILT[name] = scene(**next(s for s in SCENES if s[0] == name)[1])
    return _BUILT[name]


def cap(selected):
    return max(4, selected // 100)


def planted_occlusion(h, w, seed):
    """A fronto-parallel wall of points at depth 4 on every cell centre of the map's left half (columns 0 .. w/2 - 1), a second layer at
    depth 10 on the same centres, and free points at depth 10 on the cell centres of the right half from column w/2 + 1 on -- column w/2
    stays empty, so that at radius 1 no free point has a wall cell in its window.  One sample, a true pose that is not the identity.
    -> dict(pts [1,3,N], pose, K float64 numpy (float32-representable), expect bool [N] = wall or free)."""
    rng = np.random.default_rng(seed)
    P, K = _camera(1, h, w, rng)
    ys, xs = np.mgrid[0:h, 0:w]
    left = (xs < w // 2).ravel()
    right = (xs > w // 2).ravel()
    xs, ys = xs.ravel().astype(np.float64), ys.ravel().astype(np.float64)
    u = np.concatenate([xs[left], xs[left], xs[right]])
    v = np.concatenate([ys[left], ys[left], ys[right]])
    z = np.concatenate([np.full(left.sum(), 4.0), np.full(left.sum(), 10.0), np.full(right.sum(), 10.0)])
    expect = np.concatenate([np.ones(left.sum(), bool), np.zeros(left.sum(), bool), np.ones(right.sum(), bool)])
    order = rng.permutation(len(z))
    pts = _lift(u[order], v[order], z[order], P[0], K[0])[None]
    return dict(pts=np.asarray(pts, np.float32).astype(np.float64), pose=P, K=K, expect=expect[order])
