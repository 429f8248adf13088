"""float64 restatement of the agent environment's kernels (csrc/agent.hip, csrc/rollout.hip), numpy only, no GPU:
the observation (projection + scatter-mean), the pose update, (to|from)_disentangled, the expert action, the step reward and the
discounted return / advantage.  tests/test_env_cpu.py proves it against the fp32 oracle and the fixtures, tests/test_env_gpu.py
holds the kernels to it.

Every function takes the float32 inputs the kernels take (torch tensors or arrays), widens them to float64 and computes there, so
that what it returns is the exact answer for those inputs up to 2^-53.

Which comparisons fp32 can decide: the forward error of the projection
----------------------------------------------------------------------
project_scatter_kernel / obs_project_kernel compute, per point and in fp32,

    c_j = p_j - mu_j                                        1 rounding
    t_i = ((R_i0 c_0 + R_i1 c_1) + R_i2 c_2) + mu_i + R_i3  3 products + 2 sums, + 2 sums: 7 roundings
    n_k = (K_k0 t_0 + K_k1 t_1) + K_k2 t_2     (k = u,v,z)  3 products + 2 sums: 5 roundings
    u = n_u / n_z ,  v = n_v / n_z                          1 rounding

so 14 roundings lie between the inputs and u (13 before zc = n_z), each relative to the result it rounds, with unit roundoff
U = 2^-24.  To first order that is

    |d t_i| <= 8 U A_i ,   A_i = sum_j |R_ij| |c_j| + |mu_i| + |R_i3|       (a bound on every intermediate of t_i)
    |d n_k| <= 13 U sum_i |K_ki| A_i
    |d u|   <= (|d n_u| + |u| |d n_z|) / (|n_z| - |d n_z|) + U |u| .

The code does not use the closed form but the running analysis it summarises (`_E` below): every intermediate carries its float64
value and a bound on the distance of the kernel's fp32 value from it; a sum or product propagates the bounds of its operands and adds
U (|result| + bound) for its own rounding; the quotient uses |a'/b' - a/b| <= (|da| + |a/b| |db|) / (|b| - |db|).  The running bound
is never larger than the closed form and it is ZERO where fp32 is exact: an operation whose operands carry no error and whose exact
result is an fp32 number rounds nothing (that is how the hand scene is decided by construction: products by 0, 1 and powers of two,
sums of small multiples of 0.5).  Fused multiply-add contraction merges a product's rounding into the following sum's: it removes
roundings and never adds one, and where the analysis charges nothing (exact product, exact sum) the fused result is the same number,
so the bound holds for any contraction the compiler chooses.  The same holds for the oracle's torch statement of the chain, whose
sums may associate differently: a bound on every partial sum's magnitude bounds each association.

A factor 2 is applied on top (second-order terms, float64's own roundings, the rare sum of two fp32 numbers that float64 cannot hold).
A point is UNDECIDED when, with e = 2 x its bound (and e > 0: with e = 0 the fp32 value IS the float64 value and compares the same),
  * |zc| <= e_z                                                    (in front of or behind the camera), or, for zc certainly > 0,
  * u or v is within e of 0, w-1 / h-1 while the other axis does not already put the point certainly outside, or, for a point in view,
  * u or v is within e of a k + 0.5 rounding boundary.
A point with zc certainly <= 0, or certainly outside on one axis, is decided (outside) whatever the rest.  A CELL is undecided when an
undecided predicted-overlap point has it as a candidate: the cells of rint(u -+ e) x rint(v -+ e) clipped to the map, or every cell of the
sample when zc is undecided.  Measured shares: DESIGN.md 4x."""
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of fp32
SAFETY = 2.0


def _f64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x).astype(np.float64)


class _E:
    """float64 value + bound on |fp32 value of the kernel - value|"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else e


def _rounded(r, e):
    with np.errstate(all="ignore"):
        exact = (e == 0) & (r.astype(np.float32).astype(np.float64) == r)
        return _E(r, np.where(exact, 0.0, e + U * (np.abs(r) + e)))


def _mul(a, b):
    return _rounded(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e)


def _add(a, b):
    return _rounded(a.v + b.v, a.e + b.e)


def _sub(a, b):
    return _rounded(a.v - b.v, a.e + b.e)


def _div(a, b):
    with np.errstate(all="ignore"):
        r = a.v / b.v
        den = np.abs(b.v) - b.e
        e = np.where(den > 0, (a.e + np.abs(r) * b.e) / np.where(den > 0, den, 1.0), np.inf)
        return _rounded(r, e)


def project(pc, pose, K, mean):
    """pc [B,3,N], pose [B,4,4], K [B,3,3], mean [B,>=3] -> (u, v, zc) as _E of shape [B,N], in the kernel's order of operations."""
    pc, pose, K, mean = _f64(pc), _f64(pose), _f64(K), _f64(mean)
    B = pc.shape[0]
    col = lambda a: _E(a.reshape(B, 1))
    mu = [col(mean[:, j]) for j in range(3)]
    c = [_sub(_E(pc[:, j, :]), mu[j]) for j in range(3)]
    t = []
    for i in range(3):
        rot = _add(_add(_mul(col(pose[:, i, 0]), c[0]), _mul(col(pose[:, i, 1]), c[1])), _mul(col(pose[:, i, 2]), c[2]))
        t.append(_add(_add(rot, mu[i]), col(pose[:, i, 3])))
    n = [_add(_add(_mul(col(K[:, k, 0]), t[0]), _mul(col(K[:, k, 1]), t[1])), _mul(col(K[:, k, 2]), t[2])) for k in range(3)]
    return _div(n[0], n[2]), _div(n[1], n[2]), n[2]


def _axis(x, hi):
    """-> (inside by the float64 value, ambiguous against 0 / hi, ambiguous against a rounding boundary, e)"""
    with np.errstate(all="ignore"):
        e = np.where(np.isfinite(x.e), SAFETY * x.e, np.inf)
        inexact = e > 0
        inside = (x.v >= 0) & (x.v <= hi)
        amb = inexact & ~((np.abs(x.v) > e) & (np.abs(x.v - hi) > e))              # a NaN value with an error bound is ambiguous
        rnd = inexact & ~(np.abs(x.v - (np.floor(x.v) + 0.5)) > e)
    return inside, amb, rnd, e


def observation(pc, feat, overlap, pose, K, mean, h, w):
    """environment.py:24-126 as the kernels state it.  pc [B,3,N], feat [B,64,N], overlap [B,N] (bool / 0-1), pose [B,4,4], K [B,3,3],
    mean [B,>=3] (the centroid is an ARGUMENT: the GPU tests hand in the device's own, so that projection and colmean are judged apart).
    -> dict: map [B,h,w,64] (scatter-mean over decided, in-view, predicted-overlap points), count [B,h,w], state3d [B,N,8],
    cell [B,N] (b*h*w + y*w + x, -1 if the point scatters nowhere or is undecided), inside [B,N], decided [B,N], cell_decided [B,h,w],
    and u, v, zc with their error bounds for diagnosis."""
    pcd, ft = _f64(pc), _f64(feat)
    ov = _f64(overlap) != 0
    B, _, N = pcd.shape
    u, v, zc = project(pc, pose, K, mean)
    with np.errstate(all="ignore"):
        ez = np.where(np.isfinite(zc.e), SAFETY * zc.e, np.inf)
        z_amb = (ez > 0) & ~(np.abs(zc.v) > ez)
        front = ~z_amb & (zc.v > 0)
    in_u, amb_u, rnd_u, eu = _axis(u, w - 1)
    in_v, amb_v, rnd_v, ev = _axis(v, h - 1)
    out_sure = (~in_u & ~amb_u) | (~in_v & ~amb_v)
    edge_amb = front & ~out_sure & (amb_u | amb_v)
    inside = front & in_u & in_v & ~edge_amb
    round_amb = inside & (rnd_u | rnd_v)
    decided = ~(z_amb | edge_amb | round_amb)
    inside = inside & decided
    with np.errstate(all="ignore"):
        xi = np.where(inside, np.rint(u.v), 0).astype(np.int64)          # np.rint: half to even, like rintf and torch.round
        yi = np.where(inside, np.rint(v.v), 0).astype(np.int64)
    scat = inside & ov
    base = (np.arange(B) * h * w).reshape(B, 1)
    cell = np.where(scat, base + yi * w + xi, -1)
    acc = np.zeros((B * h * w, 64))
    cnt = np.zeros(B * h * w, dtype=np.int64)
    rows = ft.transpose(0, 2, 1).reshape(B * N, 64)
    sel = scat.reshape(-1)
    np.add.at(acc, cell.reshape(-1)[sel], rows[sel])
    np.add.at(cnt, cell.reshape(-1)[sel], 1)
    mp = acc / np.maximum(cnt, 1)[:, None]
    # cells an undecided predicted-overlap point may reach
    cd = np.ones((B, h, w), dtype=bool)
    for b, n in zip(*np.nonzero(~decided & ov)):
        if z_amb[b, n] or not (np.isfinite(eu[b, n]) and np.isfinite(ev[b, n]) and np.isfinite(u.v[b, n]) and np.isfinite(v.v[b, n])):
            cd[b] = False
            continue
        xs = {int(np.clip(np.rint(u.v[b, n] + s * eu[b, n]), 0, w - 1)) for s in (-1, 1)}
        ys = {int(np.clip(np.rint(v.v[b, n] + s * ev[b, n]), 0, h - 1)) for s in (-1, 1)}
        for y in ys:
            for x in xs:
                cd[b, y, x] = False
    st3 = np.zeros((B, N, 8))
    st3[:, :, 0:3] = pcd.transpose(0, 2, 1)
    st3[:, :, 3] = ov
    st3[:, :, 4] = inside
    return dict(map=mp.reshape(B, h, w, 64), count=cnt.reshape(B, h, w), state3d=st3, cell=cell, inside=inside, decided=decided,
                cell_decided=cd, u=u, v=v, zc=zc)


# ---- the hand scene: fp32 arithmetic is exact, the expectations are literals --------------------------------------------------------------
HAND_H, HAND_W = 4, 5
_NEXT4 = float(np.nextafter(np.float32(4.0), np.float32(np.inf)))           # the fp32 number after w - 1
# "edges": one sample, K = I, pose = I, centroid 0, u = x / z, v = y / z.           x      y     z   ov  feature base a[p]
_EDGES = [
    (0.5, 0.5, 1.0, 1, 1),        # 0  u = .5, v = .5 -> (0, 0)   half to even rounds down
    (3.0, 3.0, 2.0, 1, 2),        # 1  u = 1.5, v = 1.5 -> (2, 2)  ... and up
    (10.0, 2.0, 4.0, 1, 3),       # 2  u = 2.5, v = .5 -> (2, 0)
    (4.0, 3.0, 1.0, 1, 4),        # 3  u = w-1 and v = h-1 exactly: inside, cell (4, 3)
    (_NEXT4, 1.0, 1.0, 1, 5),     # 4  u = nextafter(w-1): outside
    (-0.0, 1.0, 1.0, 1, 6),       # 5  u = -0.0: inside, cell (0, 1)
    (-2.0 ** -20, 1.0, 1.0, 1, 7),  # 6  u = -2^-20: outside
    (0.0, 0.0, 0.0, 1, 8),        # 7  zc = 0, 0 / 0: outside
    (-2.0, -2.0, -2.0, 1, 9),     # 8  zc < 0 with u = v = 1 in range: outside
    (2.0, 1.0, 1.0, 0, 10),       # 9  in view, not predicted overlap: flag 1, nothing scattered
    (3.0, 1.0, 1.0, 1, 1),        # 10 |
    (6.0, 2.0, 2.0, 1, 3),        # 11 | four points in cell (3, 1)
    (12.0, 4.0, 4.0, 1, 5),       # 12 |
    (3.0, 1.0, 1.0, 1, 7),        # 13 |
    (1.0, 3.0, 1.0, 1, 2),        # 14 cell (1, 3)
    (3.0, 5.0, 2.0, 1, 6),        # 15 u = 1.5, v = 2.5 -> (2, 2), the second point there
    (0.0, 0.0, 1.0, 1, 5),        # 16 (0, 0), the second point there; 17 points: the last wave-group holds one
]
#                   x, y of the cell per point (None: scatters nowhere)
_EDGES_XY = [(0, 0), (2, 2), (2, 0), (4, 3), None, (0, 1), None, None, None, None, (3, 1), (3, 1), (3, 1), (3, 1), (1, 3), (2, 2), (0, 0)]
_EDGES_INSIDE = [1, 1, 1, 1, 0, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1]
#                   (y, x): (count, mean of the feature bases)
_EDGES_CELLS = {(0, 0): (2, 3.0), (2, 2): (2, 4.0), (0, 2): (1, 3.0), (3, 4): (1, 4.0), (1, 0): (1, 6.0), (1, 3): (4, 4.0), (3, 1): (1, 2.0)}
# "straddle": two samples of five points; the second has focal 2 and the principal point (1, 0.5): u = 2 x / z + 1, v = 2 y / z + 0.5.
# Points 4..7 share a wave-group across the sample boundary, 8..9 end the launch mid-group.
_STRADDLE = [
    [(1.0, 1.0, 1.0, 1, 1), (4.0, 2.0, 2.0, 1, 2), (2.0, 3.0, 1.0, 1, 3), (0.0, 0.0, 1.0, 1, 4), (3.0, 2.0, 1.0, 1, 5)],
    [(1.0, 1.0, 1.0, 1, 6), (0.5, 0.5, 1.0, 1, 7), (1.0, 0.0, 2.0, 1, 8), (3.0, 1.0, 2.0, 1, 9), (0.0, 2.0, 4.0, 1, 10)],
]
_STRADDLE_XY = [[(1, 1), (2, 1), (2, 3), (0, 0), (3, 2)], [(3, 2), (2, 2), (2, 0), (4, 2), (1, 2)]]       # v = 2.5 -> 2, 1.5 -> 2, .5 -> 0
_STRADDLE_K1 = [[2.0, 0.0, 1.0], [0.0, 2.0, 0.5], [0.0, 0.0, 1.0]]


def _hand(samples, xy, inside, Ks):
    B, N, h, w = len(samples), len(samples[0]), HAND_H, HAND_W
    pts = np.array(samples, dtype=np.float64)                                     # [B,N,5]
    a = pts[:, :, 4]
    feat = (a[:, None, :] + np.arange(64).reshape(1, 64, 1)).astype(np.float32)   # feat[b,c,n] = a[b,n] + c: small integers
    cell = np.full((B, N), -1, dtype=np.int64)
    cnt = np.zeros((B, h, w), dtype=np.int64)
    mp = np.zeros((B, h, w, 64))
    for b in range(B):
        members = {}
        for n, c in enumerate(xy[b]):
            if c is not None:
                cell[b, n] = b * h * w + c[1] * w + c[0]
                members.setdefault((c[1], c[0]), []).append(a[b, n])
        for (y, x), m in members.items():
            cnt[b, y, x] = len(m)
            mp[b, y, x] = sum(m) / len(m) + np.arange(64)
    st3 = np.zeros((B, N, 8))
    st3[:, :, 0:3] = pts[:, :, 0:3]
    st3[:, :, 3] = pts[:, :, 3]
    st3[:, :, 4] = np.array(inside)
    return dict(B=B, N=N, h=h, w=w, pc=torch.from_numpy(pts[:, :, 0:3].transpose(0, 2, 1).astype(np.float32)).contiguous(),
                feat=torch.from_numpy(feat), ov=torch.from_numpy(pts[:, :, 3] != 0), K=torch.tensor(Ks, dtype=torch.float32),
                pose=torch.eye(4).repeat(B, 1, 1), mean=torch.zeros(B, 4),
                expect=dict(cell=cell, count=cnt, map=mp, state3d=st3))


def hand_scene():
    """-> {'edges': scene, 'straddle': scene}; a scene is a dict of float32 inputs (pc [B,3,N], feat [B,64,N], ov, K, pose, mean [B,4])
    with its expectations (cell, count, map, state3d) under 'expect', written down by hand above."""
    eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    edges = _hand([_EDGES], [_EDGES_XY], [_EDGES_INSIDE], [eye])
    # the literal per-cell table must say the same as the per-point one
    for (y, x), (n, m) in _EDGES_CELLS.items():
        assert edges["expect"]["count"][0, y, x] == n and edges["expect"]["map"][0, y, x, 0] == m
    assert int(edges["expect"]["count"].sum()) == sum(n for n, _ in _EDGES_CELLS.values())
    straddle = _hand(_STRADDLE, _STRADDLE_XY, [[1] * 5, [1] * 5], [eye, _STRADDLE_K1])
    return dict(edges=edges, straddle=straddle)


# ---- random scenes -----------------------------------------------------------------------------------------------------------------------
def _yaw_pose(yaw, t):
    p = np.eye(4)
    p[0, 0], p[0, 2], p[2, 0], p[2, 2] = math.cos(yaw), math.sin(yaw), -math.sin(yaw), math.cos(yaw)
    p[0:3, 3] = t
    return p


def random_scene(B, N, h, w, seed, yaw=0.0, t=(0.0, 0.0, 0.0), overlap="random", pile=False):
    """The recipe of test_observation_and_pose (x in +-30, y in +-2, z in 1..60, focal 0.6 w, L2-normalised features, about 70 % predicted
    overlap), but K and the pose differ per sample.  overlap='none': no point is predicted overlap.  pile=True: every point is aimed within
    0.3 px of the principal point, so all of them meet in one cell."""
    r = np.random.RandomState(seed)
    z = r.uniform(1, 60, (B, N))
    K = np.zeros((B, 3, 3))
    pose = np.zeros((B, 4, 4))
    for b in range(B):
        f = 0.6 * w * (1 + 0.05 * b)
        K[b] = [[f, 0, w / 2.0 + b], [0, f, h / 2.0 - 0.5 * b], [0, 0, 1]]
        pose[b] = _yaw_pose(yaw + 0.03 * b, np.asarray(t, dtype=np.float64) + 0.1 * b * np.array([1.0, 0.0, 1.0]))
    if pile:
        x = z * r.uniform(-0.3, 0.3, (B, N)) / K[:, 0, 0].reshape(B, 1)
        y = z * r.uniform(-0.3, 0.3, (B, N)) / K[:, 1, 1].reshape(B, 1)
    else:
        x, y = r.uniform(-30, 30, (B, N)), r.uniform(-2, 2, (B, N))
    feat = r.uniform(-1, 1, (B, 64, N))
    feat = feat / np.sqrt((feat * feat).sum(1, keepdims=True))
    ov = (r.uniform(0, 1, (B, N)) > 0.3) if overlap == "random" else np.zeros((B, N), dtype=bool)
    if pile:
        ov[:] = True
    imf = r.uniform(-1, 1, (B, 64, h, w))
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.float32))
    return dict(B=B, N=N, h=h, w=w, pc=f32(np.stack([x, y, z], 1)), feat=f32(feat), ov=torch.from_numpy(ov), K=f32(K), pose=f32(pose),
                imf=f32(imf))


def planted_scene():
    """four points whose u reaches, through inexact arithmetic, a rounding boundary (2.5), the right edge (w - 1 = 9), the middle of a cell
    (4.2) and the outside (< 0): the first two are what fp32 cannot decide, the other two it can"""
    z = 7.0
    xs = torch.tensor([(2.5 - 0.1) / 3 * z, (9.0 - 0.1) / 3 * z, (4.2 - 0.1) / 3 * z, -1.0])
    pc = torch.stack([xs, torch.full((4,), (4.2 - 0.1) / 3 * z), torch.full((4,), z)]).unsqueeze(0).contiguous()
    return dict(B=1, N=4, h=10, w=10, pc=pc, feat=torch.ones(1, 64, 4), ov=torch.ones(1, 4, dtype=torch.bool),
                K=torch.tensor([[[3.0, 0, 0.1], [0, 3.0, 0.1], [0, 0, 1]]]), pose=torch.eye(4).unsqueeze(0), mean=torch.zeros(1, 4))


SCENES = {
    "tail_4001": dict(B=2, N=4001, h=24, w=40, seed=11),
    "yaw_1037": dict(B=3, N=1037, h=24, w=40, seed=12, yaw=0.4, t=(1.0, 0.0, -2.0)),
    "one_point": dict(B=1, N=1, h=8, w=8, seed=13),
    "no_overlap": dict(B=2, N=255, h=6, w=10, seed=14, overlap="none"),
    "pile_up": dict(B=1, N=4096, h=4, w=4, seed=15, pile=True),
}
MAX_UNDECIDED_POINTS = 0.005
MAX_EXCLUDED_CELLS = 0.01


def scene(name):
    return random_scene(**SCENES[name])


def shares(ref, ov):
    """-> (share of undecided points, undecided cells / occupied cells) of an observation() result"""
    occupied = int(((ref["count"] > 0) | ~ref["cell_decided"]).sum())
    return float((~ref["decided"]).mean()), float((~ref["cell_decided"]).sum()) / max(occupied, 1)


def cpu_mean(pc):
    """the fp32 centroid as the oracle takes it, [B,4]"""
    m = torch.zeros(pc.shape[0], 4)
    m[:, 0:3] = pc.float().mean(dim=2)
    return m


# ---- pose ----------------------------------------------------------------------------------------------------------------------------------
def _rot(axis, a):
    c, s, o, z = np.cos(a), np.sin(a), np.ones_like(a), np.zeros_like(a)
    flat = {"X": (o, z, z, z, c, -s, z, s, c), "Y": (c, z, s, z, o, z, -s, z, c), "Z": (c, -s, z, s, c, z, z, z, o)}[axis]
    return np.stack(flat, -1).reshape(a.shape + (3, 3))


def pose_step(pose, act_r, act_t, r_steps, t_steps, six_dof):
    """environment.py:179-207: the table entries are rounded to fp32 first, as the reference's assignment into float32 move vectors does;
    then Rx Ry Rz @ R and t + move in float64.  pose [B,4,4], act_r [B,1|3], act_t [B,2|3] -> new pose [B,4,4] float64."""
    P = _f64(pose).copy()
    ar, at = np.asarray(_f64(act_r), dtype=np.int64), np.asarray(_f64(act_t), dtype=np.int64)
    rs, ts = _f64(r_steps).astype(np.float32).astype(np.float64), _f64(t_steps).astype(np.float32).astype(np.float64)
    B = P.shape[0]
    mr, mt = np.zeros((B, 3)), np.zeros((B, 3))
    if six_dof:
        mr, mt = rs[ar], ts[at]
    else:
        mr[:, 1] = rs[ar[:, 0]]
        mt[:, 0], mt[:, 2] = ts[at[:, 0]], ts[at[:, 1]]
    E = _rot("X", mr[:, 0]) @ _rot("Y", mr[:, 1]) @ _rot("Z", mr[:, 2])
    P[:, 0:3, 0:3] = E @ P[:, 0:3, 0:3]
    P[:, 0:3, 3] += mt
    return P


def to_disentangled(pose, mean):
    """environment.py:14-21: t <- t - mu + R mu"""
    P, mu = _f64(pose).copy(), _f64(mean)[:, 0:3]
    P[:, 0:3, 3] = P[:, 0:3, 3] - mu + np.einsum("bij,bj->bi", P[:, 0:3, 0:3], mu)
    return P


def from_disentangled(pose, mean):
    """the inverse: t <- t + mu - R mu"""
    P, mu = _f64(pose).copy(), _f64(mean)[:, 0:3]
    P[:, 0:3, 3] = P[:, 0:3, 3] + mu - np.einsum("bij,bj->bi", P[:, 0:3, 0:3], mu)
    return P


# ---- expert action -------------------------------------------------------------------------------------------------------------------------
EXPERT_MARGIN = 1e-6


def _nearest(v, steps):
    """-> (first index of the nearest entry, margin to the nearest entry of ANOTHER value; inf if there is none).  Duplicated entries are at
    the same distance whatever v is, so a tie between them is no ambiguity: the first index is the answer."""
    d = np.abs(v[..., None] - steps)
    idx = d.argmin(-1)                                                    # numpy, like torch.argmin: the first index on ties
    best = np.take_along_axis(d, idx[..., None], -1)[..., 0]
    other = steps != steps[idx][..., None]
    second = np.where(other, d, np.inf).min(-1)
    return idx, second - best


def expert_action(pose_source, pose_target, r_steps, t_steps, six_dof):
    """environment.py:143-176 in float64, for step tables of any length S: extrinsic-xyz Euler angles of R_t R_s^T (R = Rz(c) Ry(b) Rx(a):
    a = atan2(R21, R22), b = atan2(-R20, |(R00, R10)|), c = atan2(R10, R00)), the fold when a > 3 (a = c = 0, b -> +-pi - b), then the nearest
    table entry with the first index on ties.  -> (action_r [B,1|3], action_t [B,2|3], decided [B]).

    decided: fp32 forms R_t R_s^T and t_t - t_s with errors of about 3 U and U |t| before the kernel widens them, i.e. below 1e-6 for the
    angles and for translations of the tables' size.  An action is decided when the margin between the nearest entry and the nearest other
    value exceeds EXPERT_MARGIN x the largest |entry| of its table, the x angle is not within 1e-6 of the fold threshold 3 or of the atan2
    cut (R21 = +-tiny with R22 < 0), and a folded y angle is not within 1e-6 of 0, where the fold jumps between +pi and -pi."""
    S, T = _f64(pose_source), _f64(pose_target)
    rs, ts = _f64(r_steps), _f64(t_steps)
    dR = np.zeros(S.shape[:1] + (3, 3))
    for i in range(3):
        for j in range(3):
            dR[:, i, j] = (T[:, i, 0] * S[:, j, 0] + T[:, i, 1] * S[:, j, 1]) + T[:, i, 2] * S[:, j, 2]
    ang = np.stack([np.arctan2(dR[:, 2, 1], dR[:, 2, 2]), np.arctan2(-dR[:, 2, 0], np.hypot(dR[:, 0, 0], dR[:, 1, 0])),
                    np.arctan2(dR[:, 1, 0], dR[:, 0, 0])], 1)
    shaky = (np.abs(ang[:, 0] - 3.0) <= 1e-6) | ((dR[:, 2, 2] < 0) & (dR[:, 2, 1] != 0) & (np.abs(dR[:, 2, 1]) <= 1e-6))
    fold = ang[:, 0] > 3.0
    shaky |= fold & (ang[:, 1] != 0) & (np.abs(ang[:, 1]) <= 1e-6)
    b = ang[:, 1]
    ang[:, 1] = np.where(fold & (b > 0), math.pi - b, np.where(fold & (b < 0), -math.pi - b, b))
    ang[fold, 0] = 0.0
    ang[fold, 2] = 0.0
    dt = T[:, 0:3, 3] - S[:, 0:3, 3]
    ar, mr = _nearest(ang, rs)
    at, mt = _nearest(dt, ts)
    okr = mr > EXPERT_MARGIN * max(float(np.abs(rs).max()), 1e-30)
    okt = mt > EXPERT_MARGIN * max(float(np.abs(ts).max()), 1e-30)
    if not six_dof:
        ar, okr = ar[:, 1:2], okr[:, 1:2]
        at, okt = at[:, [0, 2]], okt[:, [0, 2]]
    return ar, at, okr.all(1) & okt.all(1) & ~shaky


def round_trip_actions(S=11):
    """-> (3-DoF actions: every (yaw, tx, tz) of an S-entry table as act_r [S^3,1], act_t [S^3,2];
           6-DoF single-axis actions: one of the six components runs over the table, the others rest on the middle entry (0.0))"""
    g = np.stack(np.meshgrid(np.arange(S), np.arange(S), np.arange(S), indexing="ij"), -1).reshape(-1, 3)
    a6 = np.full((6 * S, 6), S // 2, dtype=np.int64)
    for k in range(6):
        a6[k * S:(k + 1) * S, k] = np.arange(S)
    return (g[:, 0:1], g[:, 1:3]), (a6[:, 0:3], a6[:, 3:6])


# ---- reward, returns -----------------------------------------------------------------------------------------------------------------------
def reward(pc, cam, mask, prev=None):
    """environment.py:263-302: mean over the masked points of |cam - (p - centroid)|^2 (NaN for an empty mask), and +0.5 / -0.5 / 0 for a
    distance below / above / equal to (or not comparable with) the previous one.  -> (reward [B], distance [B])"""
    p, c, m = _f64(pc), _f64(cam), _f64(mask) != 0
    d = c - (p - p.mean(axis=2, keepdims=True))
    sq = (d * d).sum(1)
    n = m.sum(1)
    with np.errstate(all="ignore"):
        dist = np.where(m, sq, 0.0).sum(1) / np.where(n > 0, n, np.nan)
        if prev is None:
            return np.zeros_like(dist), dist
        pv = _f64(prev).reshape(-1)
        return 0.5 * (dist < pv) - 0.5 * (dist > pv), dist


def discounted(vals, gamma):
    """buffer.py:24-33 along the last axis.  gamma is rounded to fp32 first: the kernel takes it as a float, and torch multiplies an fp32
    tensor by a Python scalar in fp32.  -> (returns, max |partial return| for the tolerance)"""
    x = _f64(vals)
    gm = float(np.float32(gamma))
    out = np.zeros_like(x)
    g = np.zeros(x.shape[:-1])
    for i in range(x.shape[-1] - 1, -1, -1):
        g = x[..., i] + gm * g
        out[..., i] = g
    return out, max(float(np.abs(out).max()), float(np.abs(x).max()))


def advantage(rewards, values, gamma, gae_lambda):
    """buffer.py:36-51: returns - values, or GAE(lambda) with a zero bootstrap value.  -> (advantage, scale): the scale also covers the values
    and the deltas, which the device forms with fp32 torch ops before / after the scan."""
    r, v = _f64(rewards), _f64(values)
    if gae_lambda == 0:
        ret, s = discounted(r, gamma)
        return ret - v, max(s, float(np.abs(v).max()), float(np.abs(ret - v).max()))
    gm = float(np.float32(gamma))
    v1 = np.concatenate([v, np.zeros(v.shape[:-1] + (1,))], -1)
    deltas = r + gm * v1[..., 1:] - v1[..., :-1]
    out, s = discounted(deltas, gamma * gae_lambda)
    return out, max(s, float(np.abs(r).max()) + 2 * float(np.abs(v).max()))


# ---- inputs shared by the CPU tier (caps) and the GPU tier (comparisons) ----------------------------------------------------------------------
def softmax_logits(rows, seed=61):
    """[rows, 2] fp32 logits in +-4, as test_small_heads draws them"""
    return torch.from_numpy(np.random.RandomState(seed + rows).uniform(-4, 4, (rows, 2)).astype(np.float32))


SOFTMAX_ROWS = (1, 257, 5000)
SOFTMAX_THRESHOLDS = ((0.5, 0.8), (0.3, 0.9))
SOFTMAX_GUARD = 1e-5
MAX_SOFTMAX_UNSAFE = 0.001


def softmax2(logits):
    x = _f64(logits)
    m = x.max(1, keepdims=True)
    e = np.exp(x - m)
    return e[:, 1] / e.sum(1)


def tiled_rollout_poses(reps=11):
    """cases.rollout_inputs() pose pairs tiled to B = 12 * reps (132: a third workgroup of the 64-thread launch)"""
    import cases as C
    inp = C.rollout_inputs()
    return inp["pose_source"].repeat(reps, 1, 1), inp["pose_target"].repeat(reps, 1, 1)


CUSTOM_TABLES = {
    "single": [0.25],
    "duplicate": [0.5, -1.0, 0.5],
    "unsorted": [0.3, -1.0, 0.0, 2.0, -0.2, 0.05, 1.0],
}
MAX_EXPERT_UNDECIDED = 0.01


def reward_case(N, kind, offset=(0.0, 0.0, 0.0), seed=3):
    """B = 3 clouds of N points in +-20 (+ offset), camera-frame points = centred cloud + 0.3 noise as cases.rollout_inputs() draws them.
    kind 'a': masks full / about 80 % / five points;  kind 'b': about 80 % / EMPTY / full."""
    r = np.random.RandomState(seed + N)
    B = 3
    pc = r.uniform(-20, 20, (B, 3, N)).astype(np.float32)
    cam = (pc - pc.mean(2, keepdims=True) + 0.3 * r.uniform(-1, 1, (B, 3, N))).astype(np.float32)
    pc = (pc + np.asarray(offset, dtype=np.float32).reshape(1, 3, 1)).astype(np.float32)
    part = (r.uniform(0, 1, N) > 0.2).astype(np.int64)
    part[0] = 1
    five = np.zeros(N, dtype=np.int64)
    five[:5] = 1
    full, empty = np.ones(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    mask = np.stack([full, part, five] if kind == "a" else [part, empty, full])
    return torch.from_numpy(pc), torch.from_numpy(cam), torch.from_numpy(mask)


REWARD_N = (1, 255, 257, 2000, 20000)
OFFSET = (1000.0, 0.0, 1000.0)


def returns_case(rows, T, seed=5):
    """rewards in {-0.5, 0, 0.5} and values in +-1, [rows, 1, T] as the buffer holds them"""
    r = np.random.RandomState(seed + rows + T)
    return (torch.from_numpy(((r.randint(0, 3, (rows, 1, T)) - 1) * 0.5).astype(np.float32)),
            torch.from_numpy(r.uniform(-1, 1, (rows, 1, T)).astype(np.float32)))
