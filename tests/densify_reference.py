"""float64 numpy restatement of ops.densify (include/cmr_hip.h cmr_densify_f32), the scenes the tests share, and the bound
the device is held to.  Shared by tests/test_densify_cpu.py and tests/test_densify_gpu.py.

The definition.  A pixel of `depth` is a sample iff it is finite and > 0.  For pixel p and every sample q of the map with |qx - px| <= R
and |qy - py| <= R:  w = exp(-a),  a = |p - q|^2 / (2 sigma_s^2) + sum_c (G_c(p) - G_c(q))^2 / (2 sigma_r^2)  (the second term only with a
guide);  S0 = sum w,  S1 = sum w z,  A_c = sum w a_c,  n = the number of such samples.  Filled iff S0 >= min_weight: depth S1 / S0,
attribute A_c / S0; else +inf and `fill`.  keep: a pixel that is a sample returns its own depth and attributes.  sigma_s, sigma_r and
min_weight are float32 numbers by the C ABI: the restatement rounds them to float32 first and computes in float64 from there.

Decided.  A pixel is DECIDED unless n > 0 and |S0 - min_weight| <= 1e-3 min_weight: only there may fp32 and float64 disagree on "filled"
(the bound below stays under 1e-3, which the tests assert).

The bound, derived for the kernel's arithmetic with u = 2^-24 (one fp32 rounding), not measured:
  * the argument.  dx^2 + dy^2 is an exact integer.  d_c = G_c(p) - G_c(q) carries u, d_c^2 carries 2u + u for the product, and the fma
    chain over the planes adds u per plane to a sum of non-negative terms: (2 + Cg) u <= 6u at Cg = 4.  The constants log2 e / (2 sigma^2)
    are computed in double from the float32 sigma and rounded once (u), the product with them is one more rounding (u, the guide term's is
    the fma's): the guide term is off by <= 8u relative, the spatial term by <= 2u, so |a' - a| <= 8 u a.  With log2 e folded into the
    constants the exponential is exp2(-a log2 e) and its relative error from the argument is ln 2 * 8 u a log2 e = 8 u a <= 8 u a_max,
    a_max = the largest argument among the window's samples.
  * the exponential itself (v_exp_f32, 1 ulp) is off by <= 2u.
  * S0 is a sum of n non-negative terms in a fixed order: (n - 1) u.  S1 is n fmas of non-negative terms: n u.  The division: u.
  The same computed weights stand above and below the fraction, so a weight error e_i moves the mean by sum w_i e_i (z_i - z) / S0:
  |e_i| <= (8 a_i + 2) u gives at most (8 a_max + 2) u * D, D = sum w_i |z_i - z| / (S0 z) < 2, and well below 1 in effect, because
  the samples with a_i near a_max are the ones with the smallest weights (w a <= 1 / e).  The tests assert the form
      |z' - z| / z <= (2 (n + 8) + 8 a_max) u = REL
  -- the roundings of the sums ((n - 1) + n + 1) u, the exponential and D's headroom inside 2 (n + 8) u -- and the same REL for
  conf = S0.  For attributes the terms w a_c are signed and cancel, so the bound is REL * sum w |a_c| / S0 instead of REL * |value|.
  Weights below 2^-126 are flushed to 0 by the hardware exponential: an absolute n 2^-126 on S0, which the conf comparison adds; on a
  filled pixel (S0 >= 1e-24) that is below 2^-40 S0.
REL is largest at R = 16 (n <= 1089) with a_max in the hundreds: about 2 (1097 + 4 * 300) u = 2.7e-4, under 1e-3.

`count`, counts[:, 0:2], the keep pixels and the unfilled pixels are exact; counts[:, 2] is exact up to the number of undecided pixels."""
import math

import numpy as np

U = 2.0 ** -24
DECIDE_MARGIN = 1e-3
FLUSH = 2.0 ** -126
MIN_WEIGHT = 1e-3
B = 3
# (h, w, density, R, sigma_s, sigma_r): the recipe of the random scenes, numpy seed 1
SCENES = {
    "37x53_d08_r4": (37, 53, 0.08, 4, 2.0, 0.1),
    "37x53_d08_r16": (37, 53, 0.08, 16, 8.0, 0.1),
    "70x150_d05_r8": (70, 150, 0.05, 8, 4.0, 0.05),
    "37x53_d50_r4": (37, 53, 0.5, 4, 2.0, 0.1),
    "37x53_d02_r4": (37, 53, 0.02, 4, 2.0, 0.1),
}
SCENE_NAMES = tuple(SCENES)
GUIDE_PLANES = (0, 1, 3)
ATTR_PLANES = (0, 1, 4)


def f32(v):
    return float(np.float32(v))


def is_sample(depth):
    d = np.asarray(depth, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def make_guide(rng, b, h, w, planes=3):
    """Smooth sinusoids plus step edges plus sigma = 0.02 noise, float32 [b, planes, h, w] round [0, 1]."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    g = np.empty((b, planes, h, w))
    for i in range(b):
        for c in range(planes):
            fx, fy, ph = rng.uniform(0.02, 0.15), rng.uniform(0.02, 0.15), rng.uniform(0, 2 * math.pi)
            smooth = 0.5 + 0.2 * np.sin(fx * x + fy * y + ph)
            ex, ey = rng.uniform(0.2, 0.8) * w, rng.uniform(0.2, 0.8) * h
            steps = 0.25 * (x > ex) - 0.2 * (y > ey)
            g[i, c] = smooth + steps + rng.normal(0.0, 0.02, (h, w))
    return g.astype(np.float32)


def make_depth(rng, b, h, w, density):
    """Depth uniform in [2, 60] on a random `density` of the pixels, +inf elsewhere (what ops.render_points writes), float32 [b, h, w]."""
    z = rng.uniform(2.0, 60.0, (b, h, w))
    return np.where(rng.random((b, h, w)) < density, z, np.inf).astype(np.float32)


_BUILT = {}


def built(name):
    """-> dict(depth [B, h, w], guide [B, 3, h, w], attr [B, 4, h, w] (NaN off the samples: it must never be read there), R, sigma_s,
    sigma_r), built once."""
    if name not in _BUILT:
        h, w, density, R, ss, sr = SCENES[name]
        rng = np.random.default_rng([1, SCENE_NAMES.index(name)])
        depth = make_depth(rng, B, h, w, density)
        guide = make_guide(rng, B, h, w)
        attr = rng.normal(0.0, 1.0, (B, 4, h, w)).astype(np.float32)
        attr[:, 1] = np.abs(attr[:, 1])
        attr = np.where(is_sample(depth)[:, None], attr, np.float32(np.nan)).astype(np.float32)
        _BUILT[name] = dict(depth=depth, guide=guide, attr=attr, R=R, sigma_s=ss, sigma_r=sr, h=h, w=w)
    return _BUILT[name]


def densify(depth, guide=None, attr=None, radius=8, sigma_s=None, sigma_r=0.1, min_weight=MIN_WEIGHT, keep=True, fill=0.0):
    """The definition in float64 over [B, h, w] maps (a loop over the (2R + 1)^2 shifts).  -> dict: depth, attr (or None), conf, count,
    counts [B, 3], sample, filled, decided, undecided (int), rel (REL per pixel), attr_scale (sum w |a| / S0, or None), a_max, zmin / zmax
    (the least / largest sample depth in the window, +inf / -inf where n = 0)."""
    depth = np.asarray(depth)
    Bn, h, w = depth.shape
    R = int(radius)
    ss = f32(max(R, 1) / 2 if sigma_s is None else sigma_s)
    sr = f32(sigma_r)
    mw = f32(min_weight)
    valid = is_sample(depth)
    z = np.where(valid, depth.astype(np.float64), 0.0)
    G = None if guide is None else np.asarray(guide, dtype=np.float64)
    A = None if attr is None else np.where(valid[:, None], np.asarray(attr, dtype=np.float64), 0.0)
    pad = lambda a, v: np.pad(a, [(0, 0)] * (a.ndim - 2) + [(R, R), (R, R)], constant_values=v)
    vp, zp = pad(valid, False), pad(z, 0.0)
    Gp = None if G is None else pad(G, 0.0)
    Ap = None if A is None else pad(A, 0.0)
    S0, S1 = np.zeros((Bn, h, w)), np.zeros((Bn, h, w))
    n = np.zeros((Bn, h, w), dtype=np.int64)
    a_max = np.zeros((Bn, h, w))
    zmin, zmax = np.full((Bn, h, w), np.inf), np.full((Bn, h, w), -np.inf)
    SA = None if A is None else np.zeros(A.shape)
    SAabs = None if A is None else np.zeros(A.shape)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            sl = (slice(None), slice(R + dy, R + dy + h), slice(R + dx, R + dx + w))
            v = vp[sl]
            if not v.any():
                continue
            arg = np.full((Bn, h, w), (dx * dx + dy * dy) / (2.0 * ss * ss))
            if G is not None:
                arg = arg + ((G - Gp[:, :, sl[1], sl[2]]) ** 2).sum(1) / (2.0 * sr * sr)
            wt = np.where(v, np.exp(-arg), 0.0)
            S0 += wt
            S1 += wt * zp[sl]
            n += v
            a_max = np.maximum(a_max, np.where(v, arg, 0.0))
            zmin = np.minimum(zmin, np.where(v, zp[sl], np.inf))
            zmax = np.maximum(zmax, np.where(v, zp[sl], -np.inf))
            if A is not None:
                SA += wt[:, None] * Ap[:, :, sl[1], sl[2]]
                SAabs += wt[:, None] * np.abs(Ap[:, :, sl[1], sl[2]])
    filled = S0 >= mw
    decided = ~((n > 0) & (np.abs(S0 - mw) <= DECIDE_MARGIN * mw))
    safe = np.where(S0 > 0, S0, 1.0)
    out_depth = np.where(filled, S1 / safe, np.inf)
    out_attr = attr_scale = None
    if A is not None:
        out_attr = np.where(filled[:, None], SA / safe[:, None], float(fill))
        attr_scale = SAabs / safe[:, None]
    if keep:
        out_depth = np.where(valid, depth.astype(np.float64), out_depth)
        if A is not None:
            out_attr = np.where(valid[:, None], A, out_attr)
    counts = np.stack([valid.sum((1, 2)), (n > 0).sum((1, 2)), filled.sum((1, 2))], 1).astype(np.int64)
    rel = (2.0 * (n + 8) + 8.0 * a_max) * U
    return dict(depth=out_depth, attr=out_attr, conf=S0, count=n, counts=counts, sample=valid, filled=filled, decided=decided,
                undecided=int((~decided).sum()), rel=rel, attr_scale=attr_scale, a_max=a_max, zmin=zmin, zmax=zmax)


_REF = {}


def reference(name, planes):
    """The keep = True restatement of scene `name` with the first `planes` guide planes and all four attribute planes, computed once and
    not to be modified; keep = False differs at the sample pixels only (reference_nokeep)."""
    key = (name, planes, True)
    if key not in _REF:
        sc = built(name)
        for keep in (True, False):
            _REF[(name, planes, keep)] = densify(sc["depth"], sc["guide"][:, :planes] if planes else None, sc["attr"], sc["R"], sc["sigma_s"],
                                                 sc["sigma_r"], keep=keep, fill=-2.5)
    return _REF[key]


def reference_nokeep(name, planes):
    reference(name, planes)
    return _REF[(name, planes, False)]


def cap(with_samples):
    """Undecided pixels the tests tolerate: 1 % of the pixels with a sample in their window."""
    return with_samples // 100


# ---- the hand-worked scene: 3 x 5, R = 1, no guide, 1 / (2 sigma_s^2) = ln 2: the weights are 1 (the pixel itself), 1/2 (an edge
# neighbour) and 1/4 (a diagonal one) ------------------------------------------------------------------------------------------------------------
INF = math.inf
HAND_SIGMA_S = math.sqrt(1.0 / (2.0 * math.log(2.0)))
HAND_DEPTH = [[4.0, INF, INF, INF, INF],
              [INF, INF, 8.0, INF, INF],
              [INF, INF, INF, INF, 2.0]]
HAND_ATTR = [[1.0, 0.0, 0.0, 0.0, 0.0],
             [0.0, 0.0, -1.0, 0.0, 0.0],
             [0.0, 0.0, 0.0, 0.0, 3.0]]
HAND_COUNT = [[1, 2, 1, 1, 0],
              [1, 2, 1, 2, 1],
              [0, 1, 1, 2, 1]]
HAND_CONF = [[1.0, 0.75, 0.5, 0.25, 0.0],
             [0.5, 0.75, 1.0, 0.75, 0.5],
             [0.0, 0.25, 0.5, 0.75, 1.0]]
# (0, 1): (4/2 + 8/4) / .75; (1, 1): (4/4 + 8/2) / .75; (1, 3): (8/2 + 2/4) / .75; (2, 3): (8/4 + 2/2) / .75
HAND_DENSE = [[4.0, 16.0 / 3.0, 8.0, 8.0, INF],
              [4.0, 20.0 / 3.0, 8.0, 6.0, 2.0],
              [INF, 8.0, 8.0, 4.0, 2.0]]
# (0, 1): (1/2 - 1/4) / .75; (1, 1): (1/4 - 1/2) / .75; (1, 3): (-1/2 + 3/4) / .75; (2, 3): (-1/4 + 3/2) / .75
HAND_FILL = -9.0
HAND_DENSE_ATTR = [[1.0, 1.0 / 3.0, -1.0, -1.0, HAND_FILL],
                   [1.0, -1.0 / 3.0, -1.0, 1.0 / 3.0, 3.0],
                   [HAND_FILL, -1.0, -1.0, 5.0 / 3.0, 3.0]]
HAND_COUNTS = [3, 13, 13]
# min_weight = 0.3 leaves the two pixels whose only sample is a diagonal neighbour unfilled
HAND_UNFILLED_AT_03 = [(0, 3), (0, 4), (2, 0), (2, 1)]
HAND_COUNTS_AT_03 = [3, 13, 11]
HAND_TOL = 1e-6                  # sigma_s is rounded to float32: the weights are 1/2 and 1/4 to 1e-7; the device adds a few u
