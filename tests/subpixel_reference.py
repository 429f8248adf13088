"""Float64 restatement of the sub-pixel match positions (cmr_match_subpixel_f32, ops.match_subpixel), written from the
contract in include/cmr_hip.h and independently of the kernel: explicit gathers with torch indexing, direct float64 squared distances.
It is the yardstick of tests/test_subpixel_gpu.py and is itself checked, on an analytic map and on planted scenes, by
tests/test_subpixel_cpu.py.

Per sample and row n: matched iff (mask absent or non-zero) and 0 <= idx < h*w.  For a matched row p = idx, x = p % w, y = p // w,
s(q) = sum_c (a_c - b_qc)^2; along x: s0 = s(p), sm = s(p - 1), sp = s(p + 1), num = sm - sp, den = (sm - s0) + (sp - s0); the axis is
fitted iff 1 <= x <= w - 2, num and den finite and den > 0; delta = clamp(0.5 num / den, -0.5, 0.5) when fitted, else 0.  Along y the same
with p -+ w and 1 <= y <= h - 2.  uv = (x + dx, y + dy), NaN on unmatched rows.  counts = (matched, fitted on both axes, matched with the
integer pixel within thr of gt_xy, matched with the sub-pixel position within thr); a non-finite gt_xy is never an inlier.

Beside the results it returns what an fp32 decision hangs on: `den` per axis and `near` = an in-map axis has |den| < DEN_TOL (the fitted
flag and the size of delta's error both hang on den), or the row's integer or sub-pixel error lies within THR_TOL of thr."""
import math

import numpy as np
import torch

import guided_reference as gref

DEN_TOL = 1e-3       # |den| under which the fp32 fit may differ from the float64 one in its flag or by more than the derived bound
THR_TOL = 1e-4       # px: an error this close to thr may fall on either side in fp32
CAP = 0.01           # at most this share of a sample's matched rows may be `near` (a condition on the scenes, not a measurement)
EPS_S = 66 * 2.0 ** -24     # relative error bound of one fp32 squared distance: 64 non-negative terms (products + sums) and two more roundings

_t64 = lambda a: torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).double()


def match_subpixel(pc, img, idx, mask=None, gt_xy=None, thr=0.5):
    """pc [B*N, C], img [B, h, w, C], idx [B*N] / [B, N] integers, mask [B, N] / [B*N] or None, gt_xy [B, 2, N] or None (torch tensors or
    numpy arrays) -> list over the samples of dict(matched [N] bool, uv [2, N] (NaN where unmatched), delta [2, N], fitted [2, N] bool,
    in_map [2, N] bool, num / den [2, N] (NaN off the map), smax [2, N] = max(s0, sm, sp) per axis, err_int / err_sub [N] (NaN without
    gt_xy), inl_int / inl_sub [N] bool, near [N] bool, counts [4] ints); axis 0 is x, axis 1 is y."""
    pc, img = _t64(pc), _t64(img)
    B, h, w, C = img.shape
    N = pc.shape[0] // B
    idx = torch.as_tensor(np.asarray(idx.detach().cpu() if torch.is_tensor(idx) else idx)).long().reshape(B, N)
    if mask is not None:
        mask = torch.as_tensor(np.asarray(mask.detach().cpu() if torch.is_tensor(mask) else mask)).reshape(B, N) != 0
    out = []
    for b in range(B):
        sel = torch.ones(N, dtype=torch.bool) if mask is None else mask[b]
        matched = sel & (idx[b] >= 0) & (idx[b] < h * w)
        p = torch.where(matched, idx[b], torch.zeros_like(idx[b]))
        x, y = p % w, torch.div(p, w, rounding_mode="floor")
        Q, F = img[b].reshape(h * w, C), pc[b * N:(b + 1) * N]
        s = lambda q: ((F - Q[q]) ** 2).sum(-1)
        s0 = s(p)
        delta = torch.zeros(2, N, dtype=torch.float64)
        fitted = torch.zeros(2, N, dtype=torch.bool)
        in_map = torch.zeros(2, N, dtype=torch.bool)
        num = torch.full((2, N), math.nan, dtype=torch.float64)
        den = torch.full((2, N), math.nan, dtype=torch.float64)
        smax = torch.zeros(2, N, dtype=torch.float64)
        for ax, (c, size, step) in enumerate(((x, w, 1), (y, h, w))):
            ok = matched & (c >= 1) & (c <= size - 2)
            off = torch.where(ok, torch.full_like(p, step), torch.zeros_like(p))      # off the map: gather p itself, discard
            sm, sp = s(p - off), s(p + off)
            nu, de = sm - sp, (sm - s0) + (sp - s0)
            fit = ok & torch.isfinite(nu) & torch.isfinite(de) & (de > 0)
            d = torch.where(fit, (0.5 * nu / torch.where(fit, de, torch.ones_like(de))).clamp(-0.5, 0.5), torch.zeros_like(de))
            nan = torch.full_like(de, math.nan)
            delta[ax], fitted[ax], in_map[ax] = d, fit, ok
            num[ax], den[ax] = torch.where(ok, nu, nan), torch.where(ok, de, nan)
            smax[ax] = torch.maximum(torch.maximum(s0, sm), sp)
        nan = torch.full((N,), math.nan, dtype=torch.float64)
        uv = torch.stack([torch.where(matched, x.double() + delta[0], nan), torch.where(matched, y.double() + delta[1], nan)])
        near = (in_map & (den.abs() < DEN_TOL)).any(0)
        err_int, err_sub = nan.clone(), nan.clone()
        inl_int = inl_sub = torch.zeros(N, dtype=torch.bool)
        if gt_xy is not None:
            g = _t64(gt_xy[b])
            fin = matched & torch.isfinite(g[0]) & torch.isfinite(g[1])
            err_int = torch.where(fin, ((x.double() - g[0]) ** 2 + (y.double() - g[1]) ** 2).sqrt(), nan)
            err_sub = torch.where(fin, ((uv[0] - g[0]) ** 2 + (uv[1] - g[1]) ** 2).sqrt(), nan)
            inl_int, inl_sub = fin & (err_int <= thr), fin & (err_sub <= thr)
            near = near | (fin & (((err_int - thr).abs() < THR_TOL) | ((err_sub - thr).abs() < THR_TOL)))
        both = matched & fitted[0] & fitted[1]
        out.append(dict(matched=matched, uv=uv, delta=delta, fitted=fitted, in_map=in_map, num=num, den=den, smax=smax, err_int=err_int,
                        err_sub=err_sub, inl_int=inl_int, inl_sub=inl_sub, near=near & matched,
                        counts=[int(matched.sum()), int(both.sum()), int(inl_int.sum()), int(inl_sub.sum())]))
    return out


def global_match(pc, img, mask=None):
    """The nearest pixel of every selected row over the whole map in float64 (lowest p on a tie), -1 on unselected rows -> int64 [B, N]."""
    pc, img = _t64(pc), _t64(img)
    B, h, w, C = img.shape
    N = pc.shape[0] // B
    idx = torch.empty(B, N, dtype=torch.int64)
    for b in range(B):
        idx[b] = torch.cdist(pc[b * N:(b + 1) * N], img[b].reshape(h * w, C)).argmin(1)
    if mask is not None:
        idx[torch.as_tensor(np.asarray(mask)).reshape(B, N) == 0] = -1
    return idx


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def bilinear(img, u, v):
    """img [h, w, C] float64, u / v [N] float64 -> [N, C]: the bilinear sample at (u, v) clamped to the map."""
    h, w, _ = img.shape
    u, v = u.clamp(0, w - 1), v.clamp(0, h - 1)
    x0, y0 = u.floor().clamp(max=max(w - 2, 0)).long(), v.floor().clamp(max=max(h - 2, 0)).long()
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    fx, fy = (u - x0)[:, None], (v - y0)[:, None]
    return (img[y0, x0] * (1 - fx) + img[y0, x1] * fx) * (1 - fy) + (img[y1, x0] * (1 - fx) + img[y1, x1] * fx) * fy


def scene_bilinear(B, N, h, w, seed, noise=0.08, outlier_frac=0.3):
    """guided_reference.scene(features="planted") with the planted point features replaced by the bilinear sample of the (float64,
    blurred, unit) feature map at the TRUE projection, clamped to the map, instead of the feature at the rounded pixel: the same map, the
    same noise and outlier draws (the generator is advanced exactly as scene does), the same renormalisation and float32 rounding.
    -> scene's dict with `pc` replaced."""
    sc = gref.scene(B, N, h, w, seed, noise=noise, outlier_frac=outlier_frac)
    g = torch.Generator(device="cpu").manual_seed(seed)
    img = gref.blurred_map(B, h, w, g)
    assert torch.equal(img.float(), sc["img"])
    uv = torch.from_numpy(sc["uv"])
    feat = torch.stack([bilinear(img[b], uv[b, 0], uv[b, 1]) for b in range(B)]) + noise * torch.randn(B, N, 64, generator=g, dtype=torch.float64)
    out = torch.rand(B, N, generator=g) < outlier_frac
    assert torch.equal(~out, sc["planted"])
    feat = torch.where(out[..., None], torch.randn(B, N, 64, generator=g, dtype=torch.float64), feat)
    sc["pc"] = torch.nn.functional.normalize(feat, dim=-1).reshape(B * N, 64).float().contiguous()
    return sc


def window_matches(sc, radius=2, centres=None):
    """The window minimum of `radius` round the rounded TRUE projection (or round `centres` [B, 2, N]) -> int64 [B, N], -1 out of view."""
    m = gref.guided_match(sc["pts"], sc["pc"], sc["img"], sc["mask"], sc["P"], sc["K"], radius, centres=sc["uv"] if centres is None else centres)
    return torch.stack([e["idx"] for e in m])


def localisation(sc, idx, margin=2):
    """Per sample: (mean |integer pixel - true uv|, mean |sub-pixel uv - true uv|, share within 0.5 px before, after, rows) over the
    planted rows whose rounded true pixel lies at least `margin` px inside the map."""
    B, _, N = sc["pts"].shape
    h, w = sc["img"].shape[1:3]
    ref = match_subpixel(sc["pc"], sc["img"], idx, gt_xy=sc["uv"], thr=0.5)
    rows = []
    for b in range(B):
        cx, cy = np.rint(sc["uv"][b, 0]), np.rint(sc["uv"][b, 1])
        inner = torch.from_numpy((cx >= margin) & (cx <= w - 1 - margin) & (cy >= margin) & (cy <= h - 1 - margin))
        use = inner & sc["planted"][b] & ref[b]["matched"]
        ei, es = ref[b]["err_int"][use], ref[b]["err_sub"][use]
        rows.append((float(ei.mean()), float(es.mean()), float((ei <= 0.5).double().mean()), float((es <= 0.5).double().mean()), int(use.sum())))
    return rows


def refine_rounds(sc, rounds=gref.ROUNDS, max_dist=gref.MAX_DIST, iters=10, start=None, subpixel=True):
    """guided_reference.refine_rounds with every round's uv taken from match_subpixel on that round's idx under that round's keep mask
    (MultiHeadModel.refine_pose_from_matches(subpixel=True) in float64).  -> (poses [B, 4, 4], per round and sample: dict(match, sub,
    refine))."""
    B, _, N = sc["pts"].shape
    h, w = sc["img"].shape[1:3]
    cur = np.array(sc["start"] if start is None else start, np.float64)
    log = []
    for radius, thr in rounds:
        m = gref.guided_match(sc["pts"], sc["pc"], sc["img"], sc["mask"], cur, sc["K"], radius, max_dist=max_dist, gt_xy=sc["gt_xy"])
        keep = torch.stack([e["keep"] for e in m])
        sub = match_subpixel(sc["pc"], sc["img"], torch.stack([e["idx"] for e in m]), mask=keep, gt_xy=sc["gt_xy"], thr=0.5)
        row = []
        for b in range(B):
            p = m[b]["idx"].clamp(min=0).numpy()
            uv = torch.nan_to_num(sub[b]["uv"]).numpy() if subpixel else np.stack([p % w, p // w]).astype(np.float64)
            r = gref.refine(sc["pts"][b], uv, m[b]["keep"].numpy(), sc["K"][b], cur[b], thr=thr, iters=iters)
            cur[b] = r["pose"]
            row.append(dict(match=m[b], sub=sub[b], refine=r))
        log.append(row)
    return cur, log


# The scenes of the GPU tier's comparison with this restatement: (name, kwargs of scene_bilinear()).  tests/test_subpixel_cpu.py asserts
# CAP on every one of them, for global arg-min matches and for guided matches of radius 2 under the scene's start pose, from float64 alone.
GPU_SCENES = [
    ("tiny_201", dict(B=2, N=257, h=8, w=12, seed=201)),
    ("tiny_202", dict(B=3, N=257, h=8, w=12, seed=202)),
    ("planted_201", dict(B=2, N=4096, h=40, w=128, seed=201)),
]
GUIDED_RADIUS = 2

_SCENES = {}


def gpu_scene(name):
    """The scene `name` of GPU_SCENES, built once and shared (leave it unchanged)."""
    if name not in _SCENES:
        _SCENES[name] = scene_bilinear(**next(kw for n, kw in GPU_SCENES if n == name))
    return _SCENES[name]


def analytic_case(h, w, seed, off=(0, 0)):
    """The map img[y][x] = (x, y, 0, ...), one point per pixel with feature (u, v, 0, ...), (u, v) = the pixel + a fraction in
    (-0.45, 0.45)^2 (all float32-representable): s is exactly (x - u)^2 + (y - v)^2, so the fit returns (u, v).  idx = the pixel moved by
    `off` = (dx, dy) pixels (rows that would leave the map keep their pixel).
    -> (pc float32 [h*w, 64], img float32 [1, h, w, 64], idx int64 [h*w], u, v float64 [h*w], moved bool [h*w])."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    img = np.zeros((1, h, w, 64), np.float32)
    img[0, :, :, 0], img[0, :, :, 1] = xs.reshape(h, w), ys.reshape(h, w)
    u = (xs + rng.uniform(-0.45, 0.45, h * w)).astype(np.float32).astype(np.float64)
    v = (ys + rng.uniform(-0.45, 0.45, h * w)).astype(np.float32).astype(np.float64)
    pc = np.zeros((h * w, 64), np.float32)
    pc[:, 0], pc[:, 1] = u, v
    nx, ny = xs + off[0], ys + off[1]
    moved = (nx >= 0) & (nx < w) & (ny >= 0) & (ny < h)
    idx = np.where(moved, ny * w + nx, ys * w + xs)
    return torch.from_numpy(pc), torch.from_numpy(img), torch.from_numpy(idx), u, v, torch.from_numpy(moved)
