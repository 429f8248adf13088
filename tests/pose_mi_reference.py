"""Float64 restatement of pose scoring by mutual information (cmr_pose_mi_f32 / ops.pose_mi, MultiHeadModel.score_poses_mi, DESIGN.md
4v), written from the contract in include/cmr_hip.h and independently of the kernel.  The projection is guided_reference.project.

Per sample b, pose p and selected row n: (u, v) = the projection, the centre (rint u, rint v) half to even; IN VIEW iff p2 > 0, u and v
finite and the centre a pixel of the H x W image; the grey value g = the pixel at the centre (nearest) or lerp(lerp(I00, I01, fx),
lerp(I10, I11, fx), fy) over the four pixels round (u, v) with clamped indices (bilinear); COUNTED iff in view and attr and g finite;
bin(x) = min(nb - 1, max(0, floor((x - lo) nb / (hi - lo)))); hist[ba][bg] counts the counted rows; H = ln n - (sum c ln c) / n over the
non-zero counts of the two marginals and the joint; mi = H_a + H_g - H_ag; n = 0 gives zeros.

NEAR rows, per (b, p): the selected rows on which an fp32 evaluation may decide differently from this one -- u or v within HALF_TOL px
of a half-integer (the centre may round the other way, which moves the cell and the in-view decision), or a counted row whose attribute
or grey value lies within EDGE_TOL (hi - lo) of a bin edge.  guided_reference.guided_match's own flag (the best / runner-up gap inside
the window, |dist - max_dist|) is empty at radius 0 without max_dist, which is all that is used here.  Each near row may move one count
of hist out of a cell and into another (a change of 2 in sum |hist - hist64|) and each of counts by at most one."""
import math

import numpy as np
import torch

import guided_reference as gref

HALF_TOL = 1e-4       # px from a half-integer under which the centre may round either way
EDGE_TOL = 1e-6       # share of (hi - lo) from a bin edge under which a value may fall into either bin
NEAR_CAP = 16         # near rows allowed per (sample, pose) on the scenes of the GPU tier (a condition on the scenes, not a measurement)


def _np(a, dtype=np.float64):
    return np.asarray(a.detach().cpu() if torch.is_tensor(a) else a).astype(dtype)


def bin_index(x, lo, hi, nb):
    """-> (bin int64, near-an-edge bool) of finite values x."""
    t = (x - lo) * (nb / (hi - lo))
    near = np.abs(t - np.rint(t)) * ((hi - lo) / nb) < EDGE_TOL * (hi - lo)
    near &= (np.rint(t) >= 1) & (np.rint(t) <= nb - 1)      # only an inner edge separates two bins: beyond lo and hi lie the end bins
    return np.clip(np.floor(t), 0, nb - 1).astype(np.int64), near


def sample(grey, u, v, mode):
    """grey [H, W] float64, (u, v) of rows in view -> their grey values."""
    H, W = grey.shape
    if mode == "nearest":
        return grey[np.rint(v).astype(np.int64), np.rint(u).astype(np.int64)]
    x0, y0 = np.floor(u), np.floor(v)
    fx, fy = u - x0, v - y0
    xa, xb = np.clip(x0, 0, W - 1).astype(np.int64), np.clip(x0 + 1, 0, W - 1).astype(np.int64)
    ya, yb = np.clip(y0, 0, H - 1).astype(np.int64), np.clip(y0 + 1, 0, H - 1).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        lerp = lambda a, b, t: a + t * (b - a)              # noqa: E731
        return lerp(lerp(grey[ya, xa], grey[ya, xb], fx), lerp(grey[yb, xa], grey[yb, xb], fx), fy)


def entropies(hist):
    """hist int [nb, nb] -> (H_a, H_g, H_ag, mi) in float64."""
    h = np.asarray(hist, np.int64)
    n = int(h.sum())
    if n == 0:
        return 0.0, 0.0, 0.0, 0.0

    def H(c):
        c = c[c > 0].astype(np.float64)
        return math.log(n) - float((c * np.log(c)).sum()) / n

    ha, hg, hag = H(h.sum(1)), H(h.sum(0)), H(h.reshape(-1))
    return ha, hg, hag, (ha + hg) - hag


def pose_mi(pts, attr, grey, mask, poses, K, bins=32, mode="nearest", attr_range=(0.0, 1.0), grey_range=(0.0, 1.0)):
    """pts [B, 3, N], attr [B, N], grey [B, H, W], mask [B, N] / [B*N] or None, poses [B, P, 4, 4], K [B, 3, 3] (tensors or arrays) ->
    dict(hist int64 [B, P, nb, nb], counts int64 [B, P, 2], selected int64 [B], entropy float64 [B, P, 3], mi float64 [B, P], near int64
    [B, P])."""
    pts, attr, grey, poses, K = _np(pts), _np(attr), _np(grey), _np(poses), _np(K)
    B, _, N = pts.shape
    P = poses.shape[1]
    H, W = grey.shape[1:]
    nb = int(bins)
    sel_all = np.ones((B, N), bool) if mask is None else (_np(mask, np.int64).reshape(B, N) != 0)
    (a_lo, a_hi), (g_lo, g_hi) = attr_range, grey_range
    out = dict(hist=np.zeros((B, P, nb, nb), np.int64), counts=np.zeros((B, P, 2), np.int64), selected=sel_all.sum(1).astype(np.int64),
               entropy=np.zeros((B, P, 3)), mi=np.zeros((B, P)), near=np.zeros((B, P), np.int64))
    for b in range(B):
        sel = sel_all[b]
        a_ok = np.isfinite(attr[b])
        ba, a_edge = bin_index(np.where(a_ok, attr[b], 0.0), a_lo, a_hi, nb)
        for p in range(P):
            with np.errstate(all="ignore"):
                u, v, _ = gref.project(pts[b], poses[b, p], K[b])
                fin = np.isfinite(u) & np.isfinite(v)
                cx, cy = np.rint(u), np.rint(v)
                view = sel & fin & (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
                half = sel & fin & ((np.abs(u - np.floor(u) - 0.5) < HALF_TOL) | (np.abs(v - np.floor(v) - 0.5) < HALF_TOL))
            g = np.full(N, np.nan)
            g[view] = sample(grey[b], u[view], v[view], mode)
            cnt = view & a_ok & np.isfinite(g)
            bg, g_edge = bin_index(np.where(cnt, g, 0.0), g_lo, g_hi, nb)
            np.add.at(out["hist"][b, p], (ba[cnt], bg[cnt]), 1)
            out["counts"][b, p] = int(view.sum()), int(cnt.sum())
            out["near"][b, p] = int((half | (cnt & (a_edge | g_edge))).sum())
            ha, hg, hag, mi = entropies(out["hist"][b, p])
            out["entropy"][b, p] = ha, hg, hag
            out["mi"][b, p] = mi
    return out


def best_index(mi, counts, selected, min_in_view=0.5):
    """MultiHeadModel.score_poses_mi's choice: the highest mi among the poses with counted >= min_in_view * selected (all poses when
    none is eligible), the lowest index on a tie -> int64 [B]."""
    mi, counted = np.asarray(mi), np.asarray(counts)[..., 1]
    out = []
    for b in range(mi.shape[0]):
        ok = counted[b] >= min_in_view * float(np.asarray(selected)[b])
        if not ok.any():
            ok[:] = True
        m = np.where(ok, mi[b], -np.inf)
        out.append(int(np.flatnonzero(m == m.max())[0]))
    return np.array(out, np.int64)


# ---- the ranking scene ---------------------------------------------------------------------------------------------------------------
RANK_H, RANK_W, RANK_N = 40, 128, 4096
RANK_K = np.array([[58.0, 0.0, 63.5], [0.0, 58.0, 19.5], [0.0, 0.0, 1.0]])


def _rot(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    R = np.eye(4)
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def _shift(k, d):
    T = np.eye(4)
    T[k, 3] = d
    return T


def ranking_scene(seed):
    """One sample: a 40 x 128 image of 8 x 8 blocks with uniform random levels, 4096 points with uniform true pixel positions and depths
    U(4, 20), attribute = the grey level at the true nearest pixel + 0.03 N(0, 1), clipped to [0, 1], 15 % of the rows replaced by U(0, 1);
    nine poses: the truth, then the truth turned about the camera's axes -- yaw (y) +1, -1, -2 degrees, pitch (x) 1, roll (z) 2 -- and
    moved by 0.3 / 0.3 / 1.5 along x / y / z.  Everything float32-representable.
    -> dict(pts [1, 3, N], attr [1, N], grey [1, H, W], K [1, 3, 3], poses [1, 9, 4, 4]) float32 arrays; the truth is index 0."""
    rng = np.random.default_rng(seed)
    H, W, N = RANK_H, RANK_W, RANK_N
    grey = np.kron(rng.uniform(0.0, 1.0, (H // 8, W // 8)), np.ones((8, 8))).astype(np.float32)
    u, v = rng.uniform(-0.5, W - 0.5, N), rng.uniform(-0.5, H - 0.5, N)
    z = rng.uniform(4.0, 20.0, N)
    cam = np.stack([(u - RANK_K[0, 2]) / RANK_K[0, 0] * z, (v - RANK_K[1, 2]) / RANK_K[1, 1] * z, z])
    truth = _rot("y", 7.0) @ _rot("x", -3.0) @ _shift(0, 0.4) @ _shift(2, 0.2)
    pts = (np.linalg.inv(truth) @ np.concatenate([cam, np.ones((1, N))]))[:3].astype(np.float32)
    truth = truth.astype(np.float32).astype(np.float64)
    # the attribute follows the pixel the float32 cloud lands on under the float32 truth
    uu, vv, _ = gref.project(pts.astype(np.float64), truth, RANK_K)
    cx, cy = np.clip(np.rint(uu), 0, W - 1).astype(np.int64), np.clip(np.rint(vv), 0, H - 1).astype(np.int64)
    attr = np.clip(grey[cy, cx] + 0.03 * rng.standard_normal(N), 0.0, 1.0)
    noise = rng.uniform(0.0, 1.0, N) < 0.15
    attr = np.where(noise, rng.uniform(0.0, 1.0, N), attr).astype(np.float32)
    D = [np.eye(4), _rot("y", 1.0), _rot("y", -1.0), _rot("y", -2.0), _rot("x", 1.0), _rot("z", 2.0), _shift(0, 0.3), _shift(1, 0.3),
         _shift(2, 1.5)]
    poses = np.stack([d @ truth for d in D]).astype(np.float32)
    return dict(pts=pts[None], attr=attr[None], grey=grey[None], K=RANK_K.astype(np.float32)[None], poses=poses[None])


def ranking_margin_bound(near_max, n):
    """What `near_max` rows changing cell can move the MI by: each row moves each of the three entropies by at most 2 (1 + ln n) / n."""
    return 2.0 * near_max * 6.0 * (1.0 + math.log(n)) / n


# ---- the hand-checked scene ---------------------------------------------------------------------------------------------------------
def hand_scene(kind):
    """A 2 x 3 image, 6 points at depth 1 under the identity pose and K (a point projects to (x, y) itself), one per pixel, nb = 2 on
    [0, 1] x [0, 1].  Grey: the left column and the middle pixel of the top row are dark (0.1), the rest bright (0.9):
        0.1 0.1 0.9
        0.1 0.9 0.9
    kind 'dependent': attr = grey, hist = [[3, 0], [0, 3]], H_a = H_g = H_ag = ln 2, MI = ln 2.
    kind 'independent': attr = 0.2 on two dark and two bright pixels, 0.8 on one dark and one bright pixel, hist = [[2, 2], [1, 1]] =
        the product of its marginals: H_a = ln 6 - (4 ln 4 + 2 ln 2) / 6, H_g = ln 2, H_ag = ln 6 - (4 ln 2) / 6 = H_a + H_g, MI = 0.
    -> dict(pts [1, 3, 6], attr [1, 6], grey [1, 2, 3], pose [1, 1, 4, 4], K [1, 3, 3]) float32 arrays, hist [2, 2]."""
    grey = np.array([[0.1, 0.1, 0.9], [0.1, 0.9, 0.9]], np.float32)
    xs, ys = np.array([0, 1, 2, 0, 1, 2], np.float32), np.array([0, 0, 0, 1, 1, 1], np.float32)
    pts = np.stack([xs, ys, np.ones(6, np.float32)])
    if kind == "dependent":
        attr = grey.reshape(-1).copy()
        hist = np.array([[3, 0], [0, 3]])
    else:
        #            dark dark bright dark bright bright
        attr = np.array([0.2, 0.2, 0.2, 0.8, 0.2, 0.8], np.float32)
        hist = np.array([[2, 2], [1, 1]])
    return dict(pts=pts[None], attr=attr[None], grey=grey[None], pose=np.eye(4, dtype=np.float32)[None, None], K=np.eye(3, dtype=np.float32)[None],
                hist=hist)


# ---- the scenes of the GPU tier -----------------------------------------------------------------------------------------------------
def equality_scene(B, N, H, W, seed, image="noise", P=19):
    """B samples for the comparisons of the GPU tier: true pixel positions uniform over the image and a margin of 20 % round it (rows out
    of view under every pose), depths U(2, 30), a random truth per sample.  image 'noise': grey U(-0.2, 1.2) per pixel, so values fall
    below lo = 0 and above hi = 1; 'smooth': 0.5 + 0.45 sin sin of low frequency (at most 0.03 a pixel), the image of the comparison
    with float64 -- an fp32 projection is ~1e-5 px off, which moves a bilinear value by less than EDGE_TOL there.  attr U(-0.2, 1.2) with
    one NaN, one +inf and one -inf row per sample where N >= 8, all three selected and in view under the truth.  poses: the truth, P - 3 perturbations of it (turned by up to 2 degrees
    about each axis, moved by up to 0.3), a pose that puts the cloud behind the camera and a NaN pose; mask: ~70 % of the rows.
    -> dict(pts [B, 3, N], attr [B, N], grey [B, H, W], K [B, 3, 3], poses [B, P, 4, 4] float32 arrays, mask [B, N] bool)."""
    rng = np.random.default_rng(seed)
    f = float(max(H, W))
    K = np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    out = dict(pts=[], attr=[], grey=[], K=[], poses=[], mask=[])
    for b in range(B):
        u, v = rng.uniform(-0.5 - 0.2 * W, W - 0.5 + 0.2 * W, N), rng.uniform(-0.5 - 0.2 * H, H - 0.5 + 0.2 * H, N)
        z = rng.uniform(2.0, 30.0, N)
        if N >= 8:
            u[[1, 3, 5]], v[[1, 3, 5]] = K[0, 2], K[1, 2]                 # the rows with a non-finite attribute: in view under the truth
        cam = np.stack([(u - K[0, 2]) / f * z, (v - K[1, 2]) / f * z, z, np.ones(N)])
        ang = rng.uniform(-10.0, 10.0, 3)
        truth = _rot("y", ang[0]) @ _rot("x", ang[1]) @ _rot("z", ang[2])
        truth[:3, 3] = rng.uniform(-0.5, 0.5, 3)
        pts = (np.linalg.inv(truth) @ cam)[:3]
        poses = [truth]
        for _ in range(P - 3):
            a, t = rng.uniform(-2.0, 2.0, 3), rng.uniform(-0.3, 0.3, 3)
            D = _rot("y", a[0]) @ _rot("x", a[1]) @ _rot("z", a[2])
            D[:3, 3] = t
            poses.append(D @ truth)
        behind = truth.copy()
        behind[2, 3] -= 1000.0
        poses += [behind, np.full((4, 4), math.nan)]
        if image == "noise":
            grey = rng.uniform(-0.2, 1.2, (H, W))
        else:
            yy, xx = np.mgrid[0:H, 0:W]
            grey = 0.5 + 0.45 * np.sin(0.06 * xx + rng.uniform(0, 6)) * np.sin(0.06 * yy + rng.uniform(0, 6))
        attr = rng.uniform(-0.2, 1.2, N)
        if N >= 8:
            attr[1], attr[3], attr[5] = math.nan, math.inf, -math.inf
        for k, val in (("pts", pts), ("attr", attr), ("grey", grey), ("K", K), ("poses", np.stack(poses))):
            out[k].append(val)
        out["mask"].append((rng.uniform(0, 1, N) < 0.7) | (np.isin(np.arange(N), (1, 3, 5)) & (N >= 8)))
    res = {k: np.stack(v).astype(np.float32) for k, v in out.items() if k != "mask"}
    res["mask"] = np.stack(out["mask"])
    return res


FLOAT64_SCENE = dict(B=2, N=4097, H=37, W=61, seed=411, image="smooth")      # the comparison with this restatement (tests/test_pose_mi_gpu.py)
