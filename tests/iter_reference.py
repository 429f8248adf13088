"""float64 restatement of the pose cost volume's kernels (csrc/iter_model.hip), numpy only, no GPU: pose sampling, mask
selection, warp + scatter-mean + occupancy, the one-channel 3x3 stencil, the pooling head, the decision and the update of cloud and
accumulated pose.  tests/test_iter_cpu.py proves it against the fp32 oracle (O.iter_sample_poses, O.iter_model) and asserts the caps,
tests/test_iter_ops_gpu.py holds the kernels to it.

Every function takes the float32 inputs the kernels take (torch tensors or arrays), widens them to float64 and computes there.

Which cells fp32 can decide
---------------------------
iter_warp_scatter_kernel and iter_warp_band_kernel compute, per pose and point and in fp32,

    t_i = ((r_i0 x + r_i1 y) + r_i2 z) + r_i3        3 products + 3 sums
    n_k = (K_k0 t_0 + K_k1 t_1) + K_k2 t_2           3 products + 2 sums          (k = u, v, z;  zc = n_z)
    u = n_u / n_z ,  v = n_v / n_z                   1 rounding

`_project` runs that chain on env_reference's running error analysis (`_E`: every intermediate carries its float64 value and a bound on the
distance of the kernel's fp32 value from it; exact operations are charged nothing; fused multiply-add only removes roundings), and a point
is UNDECIDED under the three rules of env_reference's docstring, with e = SAFETY x its bound: |zc| <= e_z; u or v within e of 0 / w-1 /
h-1 while the other axis does not already put it outside; u or v of a point in view within e of a k + 0.5 boundary.  A CELL is undecided
when an undecided SELECTED point has it as a candidate (every cell of the pose when zc is undecided).  `rt` is an ARGUMENT: the GPU tier
hands in the device's own matrices, so the sinf / cosf error of pose sampling is judged on its own (sample_poses) and does not leak in.

One addition: a point with a non-finite coordinate.  Where float64 gives NaN for zc, u or v, fp32 gives NaN too -- NaN arises only from
0 x inf, inf - inf, 0 / 0 and inf / inf, an fp32 intermediate is infinite wherever the float64 one is, and a product with an exact zero is zero
in both -- and every comparison with NaN is false: the point is decided, outside.  Infinite results without a NaN stay undecided.

Which arg-maxes fp32 can decide
-------------------------------
`decide` reports for each of its five arg-maxes (label, ry, tx, tz, joint) the float64 gap between the best value and the best value of
an entry that is not the best one's TWIN, and a bound on the kernel's error in the difference of two such values.  Twins are entries the
kernel computes from identical inputs in identical order, so that they are equal bit for bit whatever the roundings: equal logits (joint),
equal label triples (label), identical sequences of logits (a marginal).  Among twins the kernel takes the lowest index, and so does the
reference.  An arg-max is decided when gap > bound; the joint's bound is zero (the logits are inputs)."""
import functools
import math

import numpy as np
import torch

import env_reference as er
from env_reference import SAFETY, U, _E, _add, _axis, _div, _f64, _mul

SINCOS_ERR = 4 * U      # |sinf(a) - sin(a)|, |cosf(a) - cos(a)| for |a| <= pi: 2 ulp of a value below 1 (DESIGN.md 4x uses the same; measured: 4y)
EXP_ERR = 4 * U         # relative error of expf: 2 ulp
LOG_ERR = 4 * U         # relative error of logf: 2 ulp


def _f32(x):
    return _f64(x).astype(np.float32)


# ---- pose sampling -----------------------------------------------------------------------------------------------------------------------------
def inverse_pose(a, tx, tz):
    """rows of [R_y(a) | (tx, 0, tz)]^-1 = [R^T | -R^T t] in closed form -> (M [..., 4, 4] float64, bound [..., 4, 4]).
    The kernels compute c = cosf(a), s = sinf(a) (SINCOS_ERR each), -(c tx - s tz) and -(s tx + c tz): two products and one sum of at most
    |tx| + |tz|, i.e. SINCOS_ERR (|tx| + |tz|) from the functions, U (|tx| + |tz|) from the products and U (|tx| + |tz|) from the sum."""
    a, tx, tz = np.broadcast_arrays(_f64(a), _f64(tx), _f64(tz))
    c, s, o, z = np.cos(a), np.sin(a), np.ones_like(a), np.zeros_like(a)
    M = np.stack([c, z, -s, -(c * tx - s * tz), z, o, z, z, s, z, c, -(s * tx + c * tz), z, z, z, o], -1).reshape(a.shape + (4, 4))
    et = SAFETY * (SINCOS_ERR + 2 * U) * (np.abs(tx) + np.abs(tz))
    ef = np.full_like(a, SAFETY * SINCOS_ERR)
    B = np.stack([ef, z, ef, et, z, z, z, z, ef, z, ef, et, z, z, z, z], -1).reshape(a.shape + (4, 4))
    return M, B


def sample_poses(r_amp, t_amp, n):
    """-> (delta_R [n], delta_T [n]: the fp32 statement (2 amp / (n - 1)) base as the kernel and the oracle round it, returned as float32;
    rt [n^3, 3, 4] float64: rows 0..2 of the inverse of pose (i, j, k) = (rotation delta_R[i] about y, translation (delta_T[j], 0, delta_T[k]));
    bound [n^3, 3, 4])."""
    base = np.arange(-((n - 1) // 2), (n - 1) // 2 + 1).astype(np.float32)
    step = lambda amp: (np.float32(2.0) * _f32(amp).reshape(-1)[0]) / np.float32(n - 1)
    dr, dt = (step(r_amp) * base).astype(np.float32), (step(t_amp) * base).astype(np.float32)
    i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    M, B = inverse_pose(dr[i.reshape(-1)], dt[j.reshape(-1)], dt[k.reshape(-1)])
    return dr, dt, M[:, 0:3, :], B[:, 0:3, :]


def select_mask(mask, standby):
    """IterModel.py:273-275: the mask if any byte is non-zero, else the standby mask; 0 / 1 as uint8"""
    m, s = np.asarray(_f64(mask)).reshape(-1) != 0, np.asarray(_f64(standby)).reshape(-1) != 0
    return (m if m.any() else s).astype(np.uint8)


# ---- warp, scatter-mean, occupancy ---------------------------------------------------------------------------------------------------------
def _project(pc, rt, K):
    """pc [3, N], rt [P, 3, 4], K [9] -> (u, v, zc) as _E of shape [P, N], in the kernels' order of operations"""
    P = rt.shape[0]
    col = lambda a: _E(np.asarray(a, dtype=np.float64).reshape(P, 1))
    x = [_E(pc[j].reshape(1, -1)) for j in range(3)]
    with np.errstate(all="ignore"):
        t = []
        for i in range(3):
            s = _add(_add(_mul(col(rt[:, i, 0]), x[0]), _mul(col(rt[:, i, 1]), x[1])), _mul(col(rt[:, i, 2]), x[2]))
            t.append(_add(s, col(rt[:, i, 3])))
        k = lambda r, c: _E(np.full((1, 1), K[3 * r + c]))
        n = [_add(_add(_mul(k(r, 0), t[0]), _mul(k(r, 1), t[1])), _mul(k(r, 2), t[2])) for r in range(3)]
        return _div(n[0], n[2]), _div(n[1], n[2]), n[2]


def warp(pc, feat, score, sel, rt, K, h, w, with_mean=True, margin=1.0):
    """pc [3, N], feat [N, 64] rows, score [N], sel [N] 0 / 1, rt [P, 3, 4], K [3, 3] or [9] -> dict:
    cell [P, N] (y w + x; -1: outside, unselected or undecided), inside [P, N] (in view by float64, decided), decided [P, N],
    count [P, h, w], occ [P, h, w] (sum of the scores), occ_abs [P, h, w] (sum of |score|: what the bound on occ rounds against),
    mean [P, h, w, 64] (None unless with_mean), cell_decided [P, h, w], u, v, zc (_E, for diagnosis).
    margin > 1 widens every error bound by that factor: the input generators below use it to draw clouds that stay decided when `rt`
    moves by the device's sinf / cosf error."""
    pcd, ft, sc = _f64(pc), _f64(feat), _f64(score).reshape(-1)
    selb = np.asarray(_f64(sel)).reshape(-1) != 0
    rtd, Kd = _f64(rt).reshape(-1, 3, 4), _f64(K).reshape(-1)
    P, N = rtd.shape[0], pcd.shape[1]
    u, v, zc = _project(pcd, rtd, Kd)
    if margin != 1.0:
        with np.errstate(all="ignore"):
            u, v, zc = _E(u.v, u.e * margin), _E(v.v, v.e * margin), _E(zc.v, zc.e * margin)
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
    # a non-finite coordinate that gives NaN in float64 gives NaN in fp32: every comparison is false, the point is outside for certain
    wild = ~np.isfinite(pcd).all(0).reshape(1, N)
    nan_out = wild & (np.isnan(zc.v) | np.isnan(u.v) | np.isnan(v.v))
    decided = decided | nan_out
    inside = inside & decided & ~nan_out
    with np.errstate(all="ignore"):
        xi = np.where(inside, np.rint(u.v), 0).astype(np.int64)              # np.rint: half to even, like rintf and torch.round
        yi = np.where(inside, np.rint(v.v), 0).astype(np.int64)
    scat = inside & selb.reshape(1, N)
    cell = np.where(scat, yi * w + xi, -1)
    pp, nn = np.nonzero(scat)
    key = pp * (h * w) + cell[pp, nn]
    cnt = np.bincount(key, minlength=P * h * w).reshape(P, h, w)
    occ = np.bincount(key, weights=sc[nn], minlength=P * h * w).reshape(P, h, w)
    occ_abs = np.bincount(key, weights=np.abs(sc[nn]), minlength=P * h * w).reshape(P, h, w)
    mean = None
    if with_mean:
        mean = np.zeros((P * h * w, 64))
        if key.size:
            order = np.argsort(key, kind="stable")
            ks = key[order]
            starts = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0]
            mean[ks[starts]] = np.add.reduceat(ft[nn[order]], starts, axis=0) / cnt.reshape(-1)[ks[starts]][:, None]
        mean = mean.reshape(P, h, w, 64)
    cd = np.ones((P, h, w), dtype=bool)
    for p, n in zip(*np.nonzero(~decided & selb.reshape(1, N))):
        if z_amb[p, n] or not (np.isfinite(eu[p, n]) and np.isfinite(ev[p, n]) and np.isfinite(u.v[p, n]) and np.isfinite(v.v[p, n])):
            cd[p] = False
            continue
        xs = {int(np.clip(np.rint(u.v[p, n] + s * eu[p, n]), 0, w - 1)) for s in (-1, 1)}
        ys = {int(np.clip(np.rint(v.v[p, n] + s * ev[p, n]), 0, h - 1)) for s in (-1, 1)}
        for y in ys:
            for x in xs:
                cd[p, y, x] = False
    return dict(cell=cell, inside=inside, decided=decided, count=cnt, occ=occ, occ_abs=occ_abs, mean=mean, cell_decided=cd, u=u, v=v, zc=zc,
                sel=selb)


def shares(r):
    """-> (largest share over the poses of undecided SELECTED points, largest share over the poses of undecided cells among the occupied ones)"""
    sel = r["sel"]
    pts = (~r["decided"] & sel.reshape(1, -1)).sum(1) / max(int(sel.sum()), 1)
    occupied = ((r["count"] > 0) | ~r["cell_decided"]).sum((1, 2))
    cells = (~r["cell_decided"]).sum((1, 2)) / np.maximum(occupied, 1)
    return float(pts.max()), float(cells.max())


MAX_UNDECIDED_POINTS = 0.01
MAX_UNDECIDED_CELLS = 0.01


def occ_bound(r):
    """fp32 sum of n scores in any order: every partial sum is at most sum |score|, n - 1 roundings -> (n - 1) U sum |score|, x SAFETY"""
    return SAFETY * np.maximum(r["count"] - 1, 0) * U * r["occ_abs"]


def mean_bound(r, fmax):
    """fp32 sum of n terms of at most max |feat| in any order ((n - 1) U n max |feat|, / n after the division) plus the division's own
    rounding U |mean|: ((n - 1) U max |feat| + U |mean|) x SAFETY.  The band kernel's per-chunk partial sums added to the slab row are
    n - 1 roundings as well (a sum that starts from zero rounds nothing)."""
    return SAFETY * (np.maximum(r["count"] - 1, 0)[..., None] * U * fmax + U * np.abs(r["mean"]))


def stencil(plane, w1, base):
    """res [P, h, w, 64] = base [h, w, 64] + 3x3 zero-padded convolution of plane [P, h, w] with w1 [9 taps][64]
    -> (res, mag): mag = |base| + sum |w1 plane|, the magnitude the ten fp32 products and sums round against"""
    pl, wt, bs = _f64(plane), _f64(w1), _f64(base)
    P, h, w = pl.shape
    pad = np.zeros((P, h + 2, w + 2))
    pad[:, 1:h + 1, 1:w + 1] = pl
    res = np.broadcast_to(bs.reshape(1, h, w, 64), (P, h, w, 64)).copy()
    mag = np.abs(res)
    for t in range(9):
        term = pad[:, t // 3:t // 3 + h, t % 3:t % 3 + w, None] * wt[t].reshape(1, 1, 1, 64)
        res += term
        mag += np.abs(term)
    return res, mag


def stencil_bound(mag, plane_err=None, w1=None):
    """nine products and nine sums on base: a term passes through at most one product and nine sums -> 10 U mag, x SAFETY; plus, where the
    kernel's plane may differ from the one handed to `stencil` by plane_err per cell (the band kernel's halo rows are summed by another
    workgroup than the one that writes them), sum |w1| plane_err over the taps"""
    b = SAFETY * 10 * U * mag
    if plane_err is not None:
        b = b + stencil(plane_err, np.abs(_f64(w1)), np.zeros(mag.shape[1:]))[0]
    return b


# ---- head ------------------------------------------------------------------------------------------------------------------------------------------
def head(x, w24, b24, w26, b26, slope):
    """x [P, cells, ldc >= 8] (only channels 0..7 are read) -> (logits [P], bound [P]).
    The kernel's order: lane l sums cells l, l + 64, ... (ceil(cells / 64) adds, the first onto zero), six shuffle adds, one reciprocal
    and its product: the pooled value carries (ceil(cells / 64) + 7) U mean |x|.  Hidden unit: bias + eight products and sums, a term
    passes through at most one product and eight sums: sum |w| d_pool + 9 U (|b| + sum |w pool|); the LeakyReLU is 1-Lipschitz and its
    product by the slope rounds once; output: bias + four products and sums: sum |w26| d_act + 5 U (|b26| + sum |w26 act|).  x SAFETY."""
    xd = _f64(x)[:, :, 0:8]
    cells = xd.shape[1]
    w24d, b24d, w26d, b26d = _f64(w24).reshape(4, 8), _f64(b24).reshape(4), _f64(w26).reshape(4), _f64(b26).reshape(-1)[0]
    sl = float(np.float32(slope))
    pool = xd.mean(1)                                                    # [P, 8]
    d_pool = (math.ceil(cells / 64) + 7) * U * np.abs(xd).mean(1)
    hid = pool @ w24d.T + b24d                                           # [P, 4]
    d_hid = d_pool @ np.abs(w24d).T + 9 * U * (np.abs(pool) @ np.abs(w24d).T + np.abs(b24d))
    act = np.where(hid > 0, hid, hid * sl)
    d_act = d_hid + U * np.abs(act)
    out = act @ w26d + b26d
    d_out = d_act @ np.abs(w26d) + 5 * U * (np.abs(act) @ np.abs(w26d) + abs(b26d))
    return out, SAFETY * d_out


# ---- decision --------------------------------------------------------------------------------------------------------------------------------------
def _first_with_gap(vals, twin_keys):
    """-> (lowest index of the largest value, gap to the largest value of an entry that is no twin of it; inf if all are twins)"""
    best = int(np.argmax(vals))
    other = np.array([k != twin_keys[best] for k in twin_keys])
    assert all(vals[i] == vals[best] for i in range(len(vals)) if not other[i])
    return best, (float(vals[best] - vals[other].max()) if other.any() else math.inf)


def decide(logits, n, label_r, label_tx, label_tz, delta_r, delta_t):
    """iter_decide_kernel (IterModel.py:175-193, 391-473) -> dict:
    label [n^3] and label_bound (two roundings), loss and loss_bound, marg [3, n] and marg_bound [3, n],
    idx = (label, i_ry, i_tx, i_tz, joint), gap [5], bound [5] (on the difference of two candidates), decided [5],
    step = (ry, tx, tz) = (delta_r[i_ry], delta_t[i_tx], delta_t[i_tz]), matrix_i [4, 4] and matrix_bound."""
    lg = _f64(logits).reshape(-1)
    P = n ** 3
    assert lg.size == P
    lr, lx, lz = _f64(label_r).reshape(-1), _f64(label_tx).reshape(-1), _f64(label_tz).reshape(-1)
    lab = (lr[:, None, None] * (lx[None, :, None] * lz[None, None, :])).reshape(-1)
    lab_bound = (2 * U + U * U) * np.abs(lab)
    keys = [(lr[p // (n * n)], lx[(p // n) % n], lz[p % n]) for p in range(P)]
    i_lab, g_lab = _first_with_gap(lab, keys)
    i_joint, g_joint = _first_with_gap(lg, list(lg))
    mx = lg[i_joint]
    xs = lg - mx
    term = np.exp(xs)
    denom = term.sum()
    # relative error of one fp32 term expf(l - mx): the subtraction's rounding moves the argument by U |x|, expf adds EXP_ERR
    r_term = U * np.abs(xs) + EXP_ERR
    # denominator: per-thread sums of ceil(P / 256) terms, eight tree levels
    r_den = float((term * r_term).sum() / denom) + (math.ceil(P / 256) + 8) * U
    vol = lg.reshape(n, n, n)
    rows = [vol.reshape(n, n * n), vol.transpose(1, 0, 2).reshape(n, n * n), vol.transpose(2, 0, 1).reshape(n, n * n)]      # kernel order (b, c)
    marg, mb, im, gm = np.zeros((3, n)), np.zeros((3, n)), [], []
    for m in range(3):
        t = np.exp(rows[m] - mx)
        s = np.zeros(n)
        for q in range(n * n):                                           # the same sequential order for every index: twins stay twins
            s = s + t[:, q] / denom
        marg[m] = s
        # each quotient: term error, denominator error, the division; then n^2 - 1 sums
        mb[m] = ((t / denom) * (U * np.abs(rows[m] - mx) + EXP_ERR + r_den + U)).sum(1) + (n * n - 1) * U * s
        b, g = _first_with_gap(s, [tuple(r) for r in rows[m]])
        im.append(b)
        gm.append(g)
    mb = SAFETY * mb
    logden = math.log(denom)
    loss = (logden + mx) - lg[i_lab]
    # logf(denom): the denominator's relative error, logf's own; the sum with mx; the difference with the label's logit
    loss_bound = SAFETY * (r_den + LOG_ERR * abs(logden) + U * abs(logden + mx) + U * abs(loss))
    dr, dt = _f64(delta_r).reshape(-1), _f64(delta_t).reshape(-1)
    step = (dr[im[0]], dt[im[1]], dt[im[2]])
    M, MB = inverse_pose(*step)
    idx = (i_lab, im[0], im[1], im[2], i_joint)
    gap = np.array([g_lab, gm[0], gm[1], gm[2], g_joint])
    bound = np.array([2 * SAFETY * float(lab_bound.max()), 2 * float(mb[0].max()), 2 * float(mb[1].max()), 2 * float(mb[2].max()), 0.0])
    return dict(label=lab, label_bound=lab_bound, loss=loss, loss_bound=loss_bound, marg=marg, marg_bound=mb, idx=idx, gap=gap, bound=bound,
                decided=gap > bound, step=step, matrix_i=M, matrix_bound=MB, mx=mx, denom=denom)


# ---- apply -----------------------------------------------------------------------------------------------------------------------------------------
def apply(M, pc, acc):
    """-> (pc_out [3, N] = M[0:3, 0:3] pc + M[0:3, 3], its bound, acc_out = M acc, its bound).  Point: three products and three sums, a term
    passes through at most one product and three sums: 4 U (sum |M_ij p_j| + |M_i3|).  Accumulated pose: four products, the first added
    onto zero, three sums: 4 U sum |M_ik acc_kj|.  x SAFETY."""
    Md, p, a = _f64(M).reshape(4, 4), _f64(pc), _f64(acc).reshape(4, 4)
    out = Md[0:3, 0:3] @ p + Md[0:3, 3:4]
    ob = SAFETY * 4 * U * (np.abs(Md[0:3, 0:3]) @ np.abs(p) + np.abs(Md[0:3, 3:4]))
    return out, ob, Md @ a, SAFETY * 4 * U * (np.abs(Md) @ np.abs(a))


DRAW_MARGIN = 4.0         # the input generators keep every drawn point this many bounds away from a decision (see synthetic_cloud)


# ---- hand scenes: warp -----------------------------------------------------------------------------------------------------------------------------
HAND_N, HAND_AMP, HAND_POSE = 3, 0.25, 13           # pose 13 = (1, 1, 1) of 3^3: the identity
HAND_K = [[64.0, 0.0, 0.0], [0.0, 64.0, 0.0], [0.0, 0.0, 1.0]]
EDGES_H, EDGES_W = 8, 16
_UP = 2.0 ** -18
_NAN, _INF = float("nan"), float("inf")
# "edges": x = z u / 64, y = z v / 64 with z a power of two and u, v multiples of 2^-18 below 16: every product, sum and quotient of the
# chain is exact under the identity pose.  Rows: (u, v, z, selected, score, feature base a[p]) -> cell (x, y) or None.
_EDGES = [
    # -- the u axis (w - 1 = 15)
    ((0.0, 1.0, 1.0, 1, 0.5, 1), (0, 1)),            # 0  u = 0: in
    ((-0.0, 1.0, 2.0, 1, 0.25, 3), (0, 1)),          # 1  u = -0.0: in, column 0
    ((15.0, 1.0, 1.0, 1, 0.5, 2), (15, 1)),          # 2  u = w - 1: in
    ((15.0 + _UP, 1.0, 1.0, 1, 0.5, 9), None),       # 3  u = w - 1 + 2^-18: out
    ((0.5, 2.0, 4.0, 1, 0.125, 4), (0, 2)),          # 4  u = .5 -> 0
    ((1.5, 2.0, 1.0, 1, 0.5, 1), (2, 2)),            # 5  u = 1.5 -> 2
    ((2.5, 2.0, 2.0, 1, 0.25, 5), (2, 2)),           # 6  u = 2.5 -> 2
    ((14.5, 2.0, 1.0, 1, 0.75, 6), (14, 2)),         # 7  u = w - 1.5 -> 14, the even neighbour
    # -- the v axis (h - 1 = 7)
    ((5.0, 0.0, 1.0, 1, 0.5, 2), (5, 0)),            # 8  v = 0: in
    ((5.0, -0.0, 4.0, 1, 0.5, 4), (5, 0)),           # 9  v = -0.0: in, row 0
    ((5.0, 7.0, 1.0, 1, 0.375, 7), (5, 7)),          # 10 v = h - 1: in
    ((5.0, 7.0 + _UP, 1.0, 1, 0.5, 9), None),        # 11 v = h - 1 + 2^-18: out
    ((6.0, 0.5, 2.0, 1, 0.625, 3), (6, 0)),          # 12 v = .5 -> 0
    ((6.0, 1.5, 1.0, 1, 0.5, 2), (6, 2)),            # 13 v = 1.5 -> 2
    ((6.0, 2.5, 4.0, 1, 0.25, 8), (6, 2)),           # 14 v = 2.5 -> 2
    ((6.0, 6.5, 1.0, 1, 0.875, 5), (6, 6)),          # 15 v = h - 1.5 -> 6, the even neighbour
    # -- points that scatter nowhere
    ((0.0, 0.0, 0.0, 1, 0.5, 9), None),              # 16 z = 0: 0 / 0
    ((3.0, 3.0, -2.0, 1, 0.5, 9), None),             # 17 z < 0, u = v = 3 in range
    ((_NAN, 3.0, 1.0, 1, 0.5, 9), None),             # 18 x = NaN
    ((3.0, _INF, 1.0, 1, 0.5, 9), None),             # 19 y = inf
    ((8.0, 4.0, 1.0, 0, 0.5, 9), None),              # 20 in view, not selected
    ((15.0, 7.0, 2.0, 1, 0.0, 6), (15, 7)),          # 21 the far corner, score exactly 0: counted, occupancy stays 0
    # -- crowded cells in row 4: 3, 4, 5, 8 and 9 points
    ((9.0, 4.0, 1.0, 1, 0.125, 1), (9, 4)), ((9.25, 3.75, 2.0, 1, 0.125, 2), (9, 4)), ((8.75, 4.25, 4.0, 1, 0.25, 3), (9, 4)),
    ((10.0, 4.0, 1.0, 1, 0.5, 1), (10, 4)), ((10.25, 4.0, 2.0, 1, 0.5, 3), (10, 4)), ((9.75, 4.25, 4.0, 1, 0.5, 5), (10, 4)),
    ((10.0, 3.75, 1.0, 1, 0.5, 7), (10, 4)),
    ((11.0, 4.0, 1.0, 1, 0.125, 1), (11, 4)), ((11.25, 4.0, 2.0, 1, 0.125, 2), (11, 4)), ((10.75, 4.0, 4.0, 1, 0.125, 3), (11, 4)),
    ((11.0, 4.25, 1.0, 1, 0.125, 4), (11, 4)), ((11.0, 3.75, 2.0, 1, 0.5, 5), (11, 4)),
    ((12.0, 4.0, 1.0, 1, 0.25, 1), (12, 4)), ((12.25, 4.0, 2.0, 1, 0.25, 2), (12, 4)), ((11.75, 4.0, 4.0, 1, 0.25, 3), (12, 4)),
    ((12.0, 4.25, 1.0, 1, 0.25, 4), (12, 4)), ((12.0, 3.75, 2.0, 1, 0.25, 5), (12, 4)), ((12.25, 4.25, 4.0, 1, 0.25, 6), (12, 4)),
    ((11.75, 3.75, 1.0, 1, 0.25, 7), (12, 4)), ((12.0, 4.0, 2.0, 1, 0.25, 8), (12, 4)),
    ((13.0, 4.0, 1.0, 1, 0.5, 1), (13, 4)), ((13.25, 4.0, 2.0, 1, 0.5, 2), (13, 4)), ((12.75, 4.0, 4.0, 1, 0.5, 3), (13, 4)),
    ((13.0, 4.25, 1.0, 1, 0.5, 4), (13, 4)), ((13.0, 3.75, 2.0, 1, 0.5, 5), (13, 4)), ((13.25, 4.25, 4.0, 1, 0.5, 6), (13, 4)),
    ((12.75, 3.75, 1.0, 1, 0.5, 7), (13, 4)), ((13.0, 4.0, 2.0, 1, 0.5, 8), (13, 4)), ((13.0, 4.0, 4.0, 1, 0.5, 9), (13, 4)),
]
#                (y, x): (count, occupancy, mean of the feature bases); the channel c of a cell's mean is that mean + c
_EDGES_CELLS = {
    (1, 0): (2, 0.75, 2.0), (1, 15): (1, 0.5, 2.0), (2, 0): (1, 0.125, 4.0), (2, 2): (2, 0.75, 3.0), (2, 14): (1, 0.75, 6.0),
    (0, 5): (2, 1.0, 3.0), (7, 5): (1, 0.375, 7.0), (0, 6): (1, 0.625, 3.0), (2, 6): (2, 0.75, 5.0), (6, 6): (1, 0.875, 5.0),
    (7, 15): (1, 0.0, 6.0),
    (4, 9): (3, 0.5, 2.0), (4, 10): (4, 2.0, 4.0), (4, 11): (5, 1.0, 3.0), (4, 12): (8, 2.0, 4.5), (4, 13): (9, 4.5, 5.0),
}


def _hand_inputs(rows, h, w):
    """rows of (u, v, z, selected, score, a) -> fp32 inputs in the kernels' layouts; feat[p, c] = a[p] + c"""
    t = np.array(rows, dtype=np.float64)
    z = t[:, 2]
    with np.errstate(all="ignore"):
        x, y = z * t[:, 0] / 64.0, z * t[:, 1] / 64.0
    x, y = np.where(np.isfinite(t[:, 0]), x, t[:, 0]), np.where(np.isfinite(t[:, 1]), y, t[:, 1])     # NaN / inf are the coordinate itself
    feat = (t[:, 5:6] + np.arange(64).reshape(1, 64)).astype(np.float32)
    return dict(N=len(rows), h=h, w=w, n=HAND_N, r_amp=HAND_AMP, t_amp=HAND_AMP, pose=HAND_POSE, pc=np.stack([x, y, z]).astype(np.float32),
                feat=feat, score=t[:, 4].astype(np.float32), sel=(t[:, 3] != 0).astype(np.uint8), K=np.array(HAND_K, dtype=np.float32))


def _edges():
    s = _hand_inputs([r for r, _ in _EDGES], EDGES_H, EDGES_W)
    h, w = EDGES_H, EDGES_W
    cell = np.array([-1 if c is None else c[1] * w + c[0] for _, c in _EDGES], dtype=np.int64)
    cnt, occ, mean = np.zeros((h, w), dtype=np.int64), np.zeros((h, w)), np.zeros((h, w, 64))
    for (y, x), (k, o, m) in _EDGES_CELLS.items():
        cnt[y, x], occ[y, x], mean[y, x] = k, o, m + np.arange(64)
    # the literal per-cell table must say the same as the per-point one
    for (y, x), (k, o, m) in _EDGES_CELLS.items():
        members = [r for r, c in _EDGES if c == (x, y)]
        assert len(members) == k and sum(r[4] for r in members) == o and sum(r[5] for r in members) == m * k, (y, x)
    assert int(cnt.sum()) == int((cell >= 0).sum())
    s["expect"] = dict(cell=cell, count=cnt, occ=occ, mean=mean)
    return s


CROWDED_H, CROWDED_W, CROWDED_N = 8, 128, 8193
CROWDED_CELL, CROWDED_COUNT = (1, 5), 4051                      # (y, x): 4 000 points of chunk 1, 50 of chunk 2, the one point of chunk 3


def _crowded_draw(seed):
    """8 x 128 map (bands of 3 rows).  Chunk 1 (points 0..4095): all selected, all in band 0 (rows 0..2), 4 000 of them in cell (1, 5): the
    chunk's list is full.  Chunk 2: 50 more in that cell, the rest spread over all bands, a third of them unselected.  Chunk 3: one point,
    in that cell.  u, v = cell centre + i / 16 with |i| <= 4 and z in {1, 2, 4}: exact arithmetic, every point decided by construction
    under the identity.  Under the 26 other poses the GPU tier compares decided cells: a point of chunk 2's spread that is undecided there
    (bounds widened by DRAW_MARGIN) is unselected, and a draw in which one of the others is undecided is drawn again (_crowded)."""
    r = np.random.RandomState(seed)
    N, h, w = CROWDED_N, CROWDED_H, CROWDED_W
    cx, cy = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    sel = np.ones(N, dtype=np.int64)
    cx[:4000], cy[:4000] = CROWDED_CELL[1], CROWDED_CELL[0]
    cx[4000:4096], cy[4000:4096] = r.randint(0, w, 96), r.randint(0, 3, 96)
    taken = (cx[4000:4096] == CROWDED_CELL[1]) & (cy[4000:4096] == CROWDED_CELL[0])
    cx[4000:4096][taken] += 1
    cx[4096:4146], cy[4096:4146] = CROWDED_CELL[1], CROWDED_CELL[0]
    cx[4146:8192], cy[4146:8192] = r.randint(0, w, 4046), r.randint(0, h, 4046)
    taken = (cx[4146:8192] == CROWDED_CELL[1]) & (cy[4146:8192] == CROWDED_CELL[0])
    cx[4146:8192][taken] += 1
    sel[4146:8192] = r.randint(0, 3, 4046) > 0
    cx[8192], cy[8192] = CROWDED_CELL[1], CROWDED_CELL[0]
    u = np.clip(cx + r.randint(-4, 5, N) / 16.0, 0, w - 1)
    v = np.clip(cy + r.randint(-4, 5, N) / 16.0, 0, h - 1)
    z = 2.0 ** r.randint(0, 3, N)
    s = dict(N=N, h=h, w=w, n=HAND_N, r_amp=HAND_AMP, t_amp=HAND_AMP, pose=HAND_POSE, pc=np.stack([z * u / 64.0, z * v / 64.0, z]).astype(np.float32),
             feat=r.uniform(0.5, 1.0, (N, 64)).astype(np.float32), score=r.uniform(0.0, 1.0, N).astype(np.float32), sel=sel.astype(np.uint8),
             K=np.array(HAND_K, dtype=np.float32))
    d = warp(s["pc"], s["feat"], s["score"], np.ones(N), identity_rt(), s["K"], h, w, with_mean=False, margin=DRAW_MARGIN)["decided"].all(0)
    if not (d[:4146].all() and d[8192]):
        return None
    sel[~d] = 0
    s["sel"] = sel.astype(np.uint8)
    cnt = np.zeros((h, w), dtype=np.int64)
    np.add.at(cnt, (cy[sel != 0], cx[sel != 0]), 1)
    s["expect"] = dict(cell=np.where(sel != 0, cy * w + cx, -1), count=cnt)
    return s


@functools.lru_cache(maxsize=None)
def _crowded():
    for seed in range(4051, 4051 + 100):
        s = _crowded_draw(seed)
        if s is not None:
            return s
    raise RuntimeError("crowded: no decided draw")


def hand_scenes():
    """-> {'edges': scene, 'crowded': scene}: float32 inputs in the kernels' layouts (pc [3, N], feat [N, 64], score, sel, K, n, r_amp,
    t_amp, h, w) and, under 'expect', what pose 13 (the identity) must give: cell per point, count per cell, and for 'edges' occupancy and
    mean as written down by hand above"""
    return dict(edges=_edges(), crowded=_crowded())


ROLLED_N, ROLLED_AT = 4196, 4070


def rolled_edges():
    """'edges' inside a two-chunk cloud: its points sit at ROLLED_AT.., across the chunk boundary at 4096; every other point, the last one
    (index N - 1, which the band kernel's clamped loads of the tail read again) included, is a selected filler at u = -64: out of view"""
    e = _edges()
    N, k = ROLLED_N, e["N"]
    pc = np.tile(np.array([[-1.0], [0.0], [1.0]], dtype=np.float32), (1, N))
    feat = np.tile((1.0 + np.arange(64, dtype=np.float32)).reshape(1, 64), (N, 1))
    score, sel = np.full(N, 0.5, dtype=np.float32), np.ones(N, dtype=np.uint8)
    cell = np.full(N, -1, dtype=np.int64)
    at = slice(ROLLED_AT, ROLLED_AT + k)
    pc[:, at], feat[at], score[at], sel[at], cell[at] = e["pc"], e["feat"], e["score"], e["sel"], e["expect"]["cell"]
    return dict(e, N=N, pc=pc, feat=feat, score=score, sel=sel, expect=dict(e["expect"], cell=cell))


def identity_rt(n=HAND_N):
    """rt [n^3, 3, 4] float32 as the device samples it for the hand scenes' amplitudes (float64 sin / cos rounded to fp32: the CPU tier's
    stand-in for the device's matrices; the middle pose is the identity in either)"""
    _, _, rt, _ = sample_poses(np.float32([HAND_AMP]), np.float32([HAND_AMP]), n)
    return rt.astype(np.float32)


# ---- synthetic clouds that cover a map of any shape ------------------------------------------------------------------------------------------
WARP_SHAPES = [(40, 128, 3, 1500), (8, 8, 3, 1500), (16, 24, 3, 1500), (5, 100, 3, 1500), (3, 384, 3, 1500), (2, 200, 3, 1500), (7, 37, 3, 1500),
               (1, 1, 3, 1500), (8, 8, 9, 300)]            # (h, w, n, N)
WARP_AMPS = (0.15, 1.8)


@functools.lru_cache(maxsize=None)
def synthetic_cloud(h, w, N, seed=0, n=3):
    """In the style of utils/synthetic.make_iter_batch, drawn per map shape so that the cloud covers the map: principal point at the map's
    centre, focal about w / 2, x and y wide enough to leave the view on every side, about 60 % selected (standby about 90 %), scores in
    (0, 1), unit-norm features.  fp32 cannot decide about one projection in a thousand on a map a few hundred cells wide (the bound on u is
    about 26 U w), and ONE undecided point on a map of 64 cells is more than the cap of 1 % of the occupied cells allows: a point that is
    undecided under any of the n^3 poses of WARP_AMPS, with every bound widened by DRAW_MARGIN, is drawn again.  What happens ON a boundary
    is the hand scene's subject.  On the 1 x 1 map only a point on the optical axis is in view: the first five are put there."""
    r = np.random.RandomState(1000 * h + w + 7919 * seed + N)
    f = max(w / 2.0, 1.0)
    K = np.array([[f, 0.0, (w - 1) / 2.0], [0.0, f, (h - 1) / 2.0], [0.0, 0.0, 1.0]], dtype=np.float32)

    def draw(k):
        z = r.uniform(3.0, 45.0, k)
        return np.stack([r.uniform(-1.3, 1.3, k) * z * (w / 2.0 + 1) / f, r.uniform(-1.3, 1.3, k) * z * (h / 2.0 + 1) / f, z]).astype(np.float32)
    pc = draw(N)
    if h * w == 1:
        pc[0:2, 0:5] = 0.0
    feat = r.uniform(-1, 1, (N, 64))
    feat = (feat / np.sqrt((feat * feat).sum(1, keepdims=True))).astype(np.float32)
    score = r.uniform(0, 1, N).astype(np.float32)
    mask, standby = (r.uniform(0, 1, N) < 0.6).astype(np.uint8), (r.uniform(0, 1, N) < 0.9).astype(np.uint8)
    _, _, rt, _ = sample_poses(np.float32([WARP_AMPS[0]]), np.float32([WARP_AMPS[1]]), n)
    for _ in range(50):
        d = warp(pc, feat, score, np.ones(N), rt.astype(np.float32), K, h, w, with_mean=False, margin=DRAW_MARGIN)["decided"].all(0)
        if d.all():
            break
        pc[:, ~d] = draw(int((~d).sum()))
    else:
        raise RuntimeError("synthetic_cloud: no decided cloud after 50 rounds")
    return dict(N=N, h=h, w=w, pc=pc, feat=feat, score=score, mask=mask, standby=standby, K=K)


def stencil_inputs(h, w, seed=0):
    r = np.random.RandomState(31 * h + w + seed)
    return r.uniform(-1, 1, (9, 64)).astype(np.float32), r.uniform(-1, 1, (h, w, 64)).astype(np.float32)


# ---- hand scenes: decide ---------------------------------------------------------------------------------------------------------------------------
DECIDE_N = (3, 5, 9, 15, 16)
DECIDE_SCENES = ("spike", "split", "flat", "twins", "offset", "negative")
_LN3 = float(np.float32(math.log(3.0)))


def _labels(r, n):
    out = []
    for _ in range(3):
        v = r.uniform(0.0, 1.0, n)
        out.append((v / v.sum()).astype(np.float32))
    return out


def decide_scene(name, n):
    """-> dict(logits [n^3], label_r, label_tx, label_tz, delta_r, delta_t [n], all float32, and 'expect': the indices known by construction
    (None where the scene does not fix one) in the order (label, i_ry, i_tx, i_tz, joint))"""
    r = np.random.RandomState(100 * DECIDE_SCENES.index(name) + n if name in DECIDE_SCENES else 977 + n)
    P = n ** 3
    lr, lx, lz = _labels(r, n)
    delta_r, delta_t = np.linspace(-0.3, 0.3, n).astype(np.float32), np.linspace(-2.0, 2.0, n).astype(np.float32)
    at = lambda i, j, k: (i * n + j) * n + k
    expect = [None] * 5
    if name in ("spike", "offset", "negative"):
        lg = r.uniform(-1.0, 1.0, P)
        i, j, k = n - 1, 1, n // 2
        lg[at(i, j, k)] = 50.0
        if name == "offset":
            lg = lg + 1000.0
        if name == "negative":                                           # the spike at -80, everything else in [-90, -85]
            lg = r.uniform(-90.0, -85.0, P)
            lg[at(i, j, k)] = -80.0
        expect[1:5] = [i, j, k, at(i, j, k)]
    elif name == "split":
        # spike a at (0, 0, 0); plateau b g_j h_k in slice i = n - 1 with g_1 = h_0 = 3 (log 3 on the logit), 1 otherwise; the rest 30 below.
        # S = n - 1 + 3.  R: e^b S^2 in slice n - 1 against e^a + ... in slice 0.  tx: e^b 3 S at j = 1 against e^a + e^b S at j = 0:
        # S (3 - 1) > 9 e^0.05 = 9.46 for every n >= 3.  tz: k = 0 holds both the spike and the plateau's heavy column.
        b = 0.0
        a = 2 * _LN3 + 0.05                                              # above the plateau's largest entry b + 2 log 3
        vol = np.full((n, n, n), b - 30.0)
        g = np.zeros(n)
        g[1] = _LN3
        hk = np.zeros(n)
        hk[0] = _LN3
        vol[n - 1] = b + g[:, None] + hk[None, :]
        vol[0, 0, 0] = a
        lg = vol.reshape(-1)
        expect[1:5] = [n - 1, 1, 0, 0]
    elif name == "flat":
        lg = np.full(P, 0.7)
        expect[1:5] = [0, 0, 0, 0]
    elif name == "twins":
        lg = r.uniform(-1.0, 1.0, P)
        p1, p2 = (5, P - 3) if n < 9 else (100, P - 7)
        assert (p2 - p1) % 256 != 0 and (n < 9 or p2 > 256)
        lg[p1] = lg[p2] = 5.0
        expect[4] = p1
        # the label volume's two largest products are twins too: label_tz[0] == label_tz[n - 1], on the last slice and row but one
        lr[n - 1], lx[n - 2] = 2 * lr.max(), 2 * lx.max()
        lz[0] = lz[n - 1] = 2 * lz.max()
        expect[0] = at(n - 1, n - 2, 0)
        assert (at(n - 1, n - 2, n - 1) - expect[0]) % 256 != 0 and (n < 9 or expect[0] > 256)
    elif name == "random":
        lg = r.uniform(-3.0, 3.0, P)
    else:
        raise KeyError(name)
    return dict(n=n, logits=np.asarray(lg).astype(np.float32), label_r=lr, label_tx=lx, label_tz=lz, delta_r=delta_r, delta_t=delta_t, expect=expect)


# ---- inputs shared by the CPU tier (caps, decidedness) and the GPU tier -------------------------------------------------------------------------
HEAD_CASES = [(1, 1, 8), (3, 63, 8), (4, 64, 12), (5, 65, 64), (27, 80, 64), (2, 1000, 16)]          # (P, cells, ldc)
HEAD_SLOPE = 0.01


def head_inputs(P, cells, ldc):
    """x >= 0 with channels 8.. NaN; hidden unit 0 positive, 1 negative, 2 of either sign over the poses, 3 exactly zero (weights and bias)"""
    r = np.random.RandomState(P + 10 * cells + ldc)
    x = np.full((P, cells, ldc), np.nan, dtype=np.float32)
    x[:, :, 0:8] = r.uniform(0.0, 1.0, (P, cells, 8)) * r.uniform(0.5, 1.5, (P, 1, 8))
    w24 = np.zeros((4, 8), dtype=np.float32)
    w24[0] = r.uniform(0.2, 1.0, 8)
    w24[1] = -r.uniform(0.2, 1.0, 8)
    w24[2] = r.uniform(-1.0, 1.0, 8)
    b24 = np.array([0.1, -0.1, 0.0, 0.0], dtype=np.float32)
    b24[2] = -float(x[0, :, 0:8].astype(np.float64).mean(0) @ w24[2].astype(np.float64))       # unit 2 sits near zero at pose 0: both signs over the poses
    return dict(x=x, w24=w24, b24=b24, w26=r.uniform(-1.0, 1.0, 4).astype(np.float32), b26=np.array([0.05], dtype=np.float32))


APPLY_N = (1, 255, 256, 257, 5000)


def apply_inputs(N):
    """a general rigid transform (rotations about all three axes) and a general 4 x 4"""
    r = np.random.RandomState(N)
    R = er._rot("X", np.array(0.3)) @ er._rot("Y", np.array(-1.1)) @ er._rot("Z", np.array(2.0))
    M = np.eye(4)
    M[0:3, 0:3], M[0:3, 3] = R, [1.5, -0.7, 3.0]
    pc = np.stack([r.uniform(-22, 22, N), r.uniform(-2.5, 2.5, N), r.uniform(3, 45, N)])
    return M.astype(np.float32), pc.astype(np.float32), r.uniform(-2, 2, (4, 4)).astype(np.float32)
