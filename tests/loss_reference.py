"""float64 restatement of the geometric heads' loss kernels, torch-CPU only, no GPU: the focal overlap loss with its metrics
(cmr_focal_metrics_f32, cmr_focal_bwd_f32), the circle loss on sampled (point, pixel) pairs (cmr_circle_loss_f32,
cmr_circle_loss_bwd_f32) and the descriptor normalisation that feeds it (cmr_l2norm64_f32, cmr_l2norm64_bwd_f32).
tests/test_loss_cpu.py proves it against the oracle (oracle/cmr_oracle.py focal_loss / circle_loss and their float64 autograd) and
asserts every condition the GPU tier relies on; tests/test_loss_gpu.py holds the kernels to it.

Every function takes the float32 inputs the kernels take, in the kernels' layouts, widens them to float64 and computes there.  Float
PARAMETERS (margins, alpha, grad_scale) are narrowed to float32 first (`f32`), as the C ABI narrows them.  The same functions run in
float32 when asked (`dtype=torch.float32`): that is the oracle's formula in fp32 on the CPU, the yardstick of the bars below.

It returns more than the kernels return -- per-row focal losses, the circle loss's pair distances, mask and [B, 2n] terms -- so that
the GPU tier can compare term by term instead of a mean in which one wrong row among B n is diluted by 1 / (2 B n).

The circle loss's gradient is in CLOSED FORM (circle_backward): with the weights pw, nw detached as the reference detaches them,

    dL / d d_ij = (pw_ij gp_ij - nw_ij gn_ij) / (B n)
    gp_ij = sig(lpr_i + lnr_i) exp(tp_ij - lpr_i) + sig(lpc_j + lnc_j) exp(tp_ij - lpc_j)        (gn likewise with tn, lnr, lnc)
    G_ij = dL / d d_ij / d_ij ,  G_ij = 0 where d_ij = 0
    d pts_i = sum_j G_ij (pts_i - pix_j) ,  d pix_j = - sum_i G_ij (pts_i - pix_j)

scattered (added) into the dense [B N, 64] and [B, h, w, 64] arrays.  sig is the derivative of F.softplus as torch defines it
(1 above the threshold 20).  Autograd cannot serve at d = 0 (sqrt's derivative is inf, times 0: NaN); the kernel clamps d at 1e-12 and
multiplies by a zero feature difference, which is the G = 0 above.  circle_forward(..., grad=True) gives autograd of the same loss with
exactly those pairs' distance detached, the CPU tier compares the two.

The mask compares |xy_float_i - xy_int_j| with dist_thres.  The case builders only use offsets that are multiples of 1/4 and
thresholds 1 and 2, so dx^2 + dy^2 is a small multiple of 1/16 and exact in fp32, its square root is correctly rounded, and the
comparison is decided the same in fp32 and float64: a pair is exactly on the threshold or at least sqrt(1 + 1/16) - 1 = 0.0307
(threshold 1) / sqrt(4 + 1/16) - 2 = 0.0155 (threshold 2) away.  circle_forward reports the gap, the CPU tier asserts it.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
F32 = torch.float32


def f32(x):
    """the value of a float argument once the C ABI narrowed it to float"""
    return float(np.float32(x))


# ---- bars ----------------------------------------------------------------------------------------------------------------------------------
# Each bar is 4 x the largest error of the ORACLE'S FORMULA EVALUATED IN FP32 ON THE CPU against the float64 reference, in the metric and
# over the inputs of the GPU test that uses the bar (tests/test_loss_cpu.py::test_fp32_oracle_stays_within_a_quarter_of_every_bar
# re-measures and asserts err <= bar / 4, so no bar can drift from its yardstick).  The device's expf / logf are 1-2 ulp against the
# host's <= 1 ulp and the kernels sum in another order (serial 64-term sums, wave butterflies): each a small constant factor, where an
# indexing, masking or branch mistake moves a term by a percent or more.  `measured` is the fp32 oracle's error the bar was taken
# from (x86-64, torch CPU); a bar is 4 x that, rounded up by at most a tenth so that another host's libm does not trip the CPU tier.
# CAPS are the bars the suite had for the same ops before (test_ops_gpu.py, test_train_geo_gpu.py): no bar may exceed its cap.
FOCAL_ROW_BAR = 6.0e-6        # per-row loss, relative to the row's own value; measured 1.35e-6 (row sweep, rows = 1 launches)
FOCAL_MEAN_BAR = 6.4e-7       # mean loss of the shape / metric cases, relative; measured 1.42e-7
FOCAL_GRAD_BAR = 1.55e-6      # per element, of alpha grad_scale / rows; measured 3.60e-7
CIRCLE_TERM_BAR = 1.15e-6     # each of the [B, 2n] terms, relative to its own value; measured 2.57e-7
CIRCLE_LOSS_BAR = 7.2e-7      # the scalar, relative; measured 1.61e-7
CIRCLE_GRAD_BAR = 6.0e-6      # d_pc / d_img incl. the pre-fill, of the gradient tensor's largest entry; measured 1.37e-6
L2NORM_FWD_BAR = 2.2e-7       # y, absolute (|y| <= 1); measured 4.93e-8
L2NORM_BWD_BAR = 1.0e-6       # dx incl. the accumulate pre-fill, per row of max|dy_row| / max(|x_row|, eps); measured 2.24e-7
CAPS = {"FOCAL_ROW_BAR": 1e-5, "FOCAL_MEAN_BAR": 1e-5, "FOCAL_GRAD_BAR": 5e-5, "CIRCLE_TERM_BAR": 2e-5, "CIRCLE_LOSS_BAR": 2e-5,
        "CIRCLE_GRAD_BAR": 2e-4, "L2NORM_FWD_BAR": 3e-5, "L2NORM_BWD_BAR": 3e-5}


def rel_err(got, ref):
    """largest |got - ref| / |ref| over the elements (float64 tensors; every ref element non-zero)"""
    got, ref = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
    return float(((got - ref).abs() / ref.abs()).max())


def scaled_err(got, ref, scale):
    """largest |got - ref| / scale; scale a number or broadcastable per-row sizes"""
    return float(((torch.as_tensor(got).double() - torch.as_tensor(ref).double()).abs() / scale).max())


# ---- focal loss (models/focal_loss.py: gamma = 2, mean, eps = 1e-6) ------------------------------------------------------------------------
@torch.enable_grad()          # other test modules switch autograd off process-wide at import
def focal(logits, label, alpha, dtype=F64):
    """logits float32 [R, 2], label int64 [R] (non-zero = class 1, as the kernels read it) -> dict:
    row [R] per-row loss, mean, counts = (tp, predicted positive, labelled positive, correct) as Python ints, pred [R],
    grad [R, 2] = d mean / d logits in closed form, grad_autograd the same by autograd."""
    z = logits.detach().to(dtype).clone().requires_grad_(True)
    lab = (label != 0).long()
    alpha = f32(alpha)
    p = F.softmax(z, dim=1)
    soft = p + 1e-6
    one_hot = torch.zeros_like(z).scatter_(1, lab.unsqueeze(1), 1.0) + 1e-6
    fl = -alpha * torch.pow(-soft + 1.0, 2.0) * torch.log(soft)
    row = torch.sum(one_hot * fl, dim=1)
    mean = torch.mean(row)
    mean.backward()
    with torch.no_grad():
        # d row / d z_k = sum_c w_c f'(s_c) p_c (delta_ck - p_k),  f'(s) = -alpha (-2 (1 - s) log s + (1 - s)^2 / s)
        fp = -alpha * (-2.0 * (1.0 - soft) * torch.log(soft) + (1.0 - soft) ** 2 / soft)
        c = one_hot * fp * p
        grad = (c - p * c.sum(1, keepdim=True)) / z.shape[0]
        pred = (logits[:, 1] > logits[:, 0]).long()                    # torch.argmax: the first maximum on ties
        counts = (int(((pred == 1) & (lab == 1)).sum()), int((pred == 1).sum()), int((lab == 1).sum()), int((pred == lab).sum()))
    return {"row": row.detach(), "mean": mean.detach(), "counts": counts, "pred": pred, "grad": grad, "grad_autograd": z.grad.detach()}


def focal_metrics(counts, rows, B):
    """(precision, recall, accuracy) as the float32 numbers the kernel must return for these integer counts: the counts are exact
    integers below 2^24, precision and recall one fp32 division each (0 / 0 = NaN), accuracy two."""
    tp, pp, lp, ok = (np.float32(v) for v in counts)
    with np.errstate(invalid="ignore", divide="ignore"):
        return tp / pp, tp / lp, (ok / np.float32(B)) / np.float32(rows // B)


FOCAL_DIFFS = (0.0, 1e-3, 0.5, 1.0, 2.0, 3.0, 5.0, 8.0, 12.0, 14.0, 16.0, 17.0, 20.0, 30.0, 50.0, 88.0, 100.0, 200.0)
FOCAL_BASES = (0.0, 37.5, -80.0)
FOCAL_ALPHAS = (0.75, 0.5)


@functools.lru_cache(maxsize=None)
def focal_sweep():
    """every logit difference x sign x label x base offset -> (logits float32 [216, 2], label int64 [216])"""
    rows, labs = [], []
    for base in FOCAL_BASES:
        for d in FOCAL_DIFFS:
            for sign in (1.0, -1.0):
                for lab in (0, 1):
                    rows.append((base, base + sign * d))
                    labs.append(lab)
    return torch.tensor(rows, dtype=F32), torch.tensor(labs, dtype=torch.int64)


FOCAL_SHAPES = ((1, 1), (255, 1), (256, 1), (257, 1), (5 * 256 + 3, 1), (3 * 4099, 3), (512 * 256 + 77, 1))      # (rows, B)
FOCAL_BWD_ROWS = (1, 257, 3 * 4099)


@functools.lru_cache(maxsize=None)
def focal_rows(rows, seed=0):
    """seeded logits in [-6, 6] (one row in eight a tie) and labels -> (float32 [rows, 2], int64 [rows])"""
    g = torch.Generator().manual_seed(7000 + rows + seed)
    z = (torch.rand(rows, 2, generator=g) * 12 - 6).to(F32)
    tie = torch.rand(rows, generator=g) < 0.125
    z[tie, 1] = z[tie, 0]
    lab = (torch.rand(rows, generator=g) < 0.4).long()
    return z, lab


FOCAL_METRIC_CASES = ("none_predicted", "none_labelled", "all_right", "ties")


@functools.lru_cache(maxsize=None)
def focal_metric_case(name):
    z, lab = focal_rows(257, seed=1)
    z, lab = z.clone(), lab.clone()
    if name == "none_predicted":
        z[:, 0] = torch.maximum(z[:, 0], z[:, 1]) + 0.5
    elif name == "none_labelled":
        lab[:] = 0
    elif name == "all_right":
        lab = (z[:, 1] > z[:, 0]).long()
    elif name == "ties":
        z[:, 1] = z[:, 0]
    else:
        raise KeyError(name)
    return z, lab


# ---- circle loss (MultiHeadModel.py:141-178 on the sampled pairs of :240-262) --------------------------------------------------------------
PRODUCT_PARAMS = dict(dist_thres=1.0, pos_margin=0.1, neg_margin=1.4, log_scale=10.0, lam=1.0)
OTHER_PARAMS = dict(dist_thres=2.0, pos_margin=0.2, neg_margin=1.0, log_scale=5.0, lam=0.5)
FEATS = ("random", "trained", "prototype")
MASKS = ("sparse", "dense")
# per-point offsets from the home pixel, all multiples of 1/4: on the threshold (+-1, 0), (0, +-1); just off it (1, 0.25); inside; outside
OFFSETS = ((1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (1.0, 0.25), (0.0, 0.0), (0.25, 0.25), (-0.5, 0.75), (0.75, -0.75), (1.25, 0.0),
           (0.5, 0.5), (-0.25, 1.0))
DENSE_PIXELS = ((2, 1), (1, 1), (1, 2))
DENSE_POINTS = ((1.25, 1.25), (1.5, 1.0), (2.0, 1.25), (3.0, 1.0), (2.0, 2.0))      # all within 1 of pixel (2, 1); (3, 1), (2, 2) exactly 1
N_POINTS = 40
TRAINED_SIGMA = 0.8           # std of the "trained" family's wave vectors: feature correlation exp(-sigma^2 |dx|^2 / 2) between pixels


def _unit(t):
    return F.normalize(t.double(), dim=-1).to(F32)


@functools.lru_cache(maxsize=None)
def circle_case(n, B, feat="random", mask="sparse", special=None):
    """One seeded case in the kernels' layouts: pc float32 [B N, 64], img float32 [B, h, w, 64], pc_idx int64 [B, n], xy_int int64
    [B, 2, n] (x row, y row), xy_float float32 [B, 2, n].  N = 40 and h x w = 3 x 5 (n <= 17) or 6 x 9, so indices repeat.

    Every point p has a home pixel and a position = home + a quarter-pixel offset; sample k names a point and, as its pixel, that point's
    home, so the pairs (k, k) include offsets exactly on the threshold.
    mask "sparse": homes keep four columns clear of the right edge; sample 0 is point 0 at pixel (0, 0), sample 1 is point N - 1 with the
    pixel (w - 1, h - 1), which no point is near (a column without a positive), sample 4 is point 1, the stray point, which sits outside the
    image at (-3, -2.25) (a row without a positive).
    mask "dense": pixels from a three-pixel cluster, positions from five places all within 1 of pixel (2, 1): sample 0 is a row and a
    column of positives only; points 0 and N - 1 are named.
    feat "random": unit vectors.  "trained": pixel features vary smoothly over the image (random Fourier features of the pixel position:
    neighbours at d ~ 0.9, far pixels at d ~ 1.4, what a trained head gives; with unrelated neighbours every positive a pixel away
    would sit at d = 1.41 and push the softplus argument past 20) and a point's feature is the feature of the pixel nearest its
    position plus 1e-2 noise, renormalised.  "prototype": +- unit basis vectors, d in {0, sqrt 2, 2}; a point carries MINUS the feature of the pixel nearest its
    position, and pixel features repeat, so positives sit at d = 2 and negatives at d = 0.
    special "repeat" (n = 130): the pixel of sample 0 again at samples 3, 70, 129; the point of sample 1 again at 2 and 100.
    special "dzero": the point of sample 3 carries, bit for bit, the feature of the pixel of sample 5: d[3, 5] = 0."""
    N = N_POINTS
    h, w = (3, 5) if n <= 17 else (6, 9)
    g = torch.Generator().manual_seed(100000 * FEATS.index(feat) + 50000 * MASKS.index(mask) + 100 * n + B + (7 if special else 0))
    ri = lambda hi, *shape: torch.randint(0, hi, shape, generator=g)
    if mask == "sparse":
        home = torch.stack([ri(w - 3, B, N), ri(h, B, N)], 1)                        # [B, 2, N] (x, y)
        home[:, :, 0] = 0
        off = torch.tensor(OFFSETS, dtype=F32)[torch.arange(N) % len(OFFSETS)].t().unsqueeze(0).expand(B, 2, N)
        pos = home.to(F32) + off
        pos[:, 0, 1], pos[:, 1, 1] = -3.0, -2.25                                     # the stray point: outside the image, near no pixel
    else:
        pix = torch.tensor(DENSE_PIXELS)[ri(len(DENSE_PIXELS), B, N)]               # [B, N, 2]
        home = pix.permute(0, 2, 1).contiguous()
        home[:, :, 0] = torch.tensor(DENSE_PIXELS[0])
        pos = torch.tensor(DENSE_POINTS, dtype=F32)[ri(len(DENSE_POINTS), B, N)].permute(0, 2, 1).contiguous()
        pos[:, :, 0] = torch.tensor(DENSE_POINTS[0])
    pc_idx = ri(N, B, n)
    pc_idx[:, 0] = 0
    if n > 1:
        pc_idx[:, 1] = N - 1
    if n > 4 and mask == "sparse":
        pc_idx[:, 4] = 1
    if special == "repeat":
        pc_idx[:, 2] = pc_idx[:, 1]
        pc_idx[:, 100] = pc_idx[:, 1]
    bi = torch.arange(B)[:, None]
    xy_int = torch.stack([home[:, 0][bi, pc_idx], home[:, 1][bi, pc_idx]], 1)       # [B, 2, n]
    xy_float = torch.stack([pos[:, 0][bi, pc_idx], pos[:, 1][bi, pc_idx]], 1).contiguous()
    if mask == "sparse":
        if n > 1:
            xy_int[:, 0, 1], xy_int[:, 1, 1] = w - 1, h - 1
    if special == "repeat":
        for k in (3, 70, 129):
            xy_int[:, :, k] = xy_int[:, :, 0]
    near = torch.stack([(pos[:, 0] + 0.5).floor(), (pos[:, 1] + 0.5).floor()], 1)      # [B, 2, N]: the pixel a point falls on (the stray: none)
    if feat == "prototype":
        axis, sign = ri(3, B, h, w), ri(2, B, h, w) * 2 - 1
        img = F.one_hot(axis, 64).to(F32) * sign.unsqueeze(-1).to(F32)
        img[:, 1, 3] = -img[:, 1, 1]                                                # dense: the points at (3, 1) are negatives of pixel (1, 1), at d = 0
        pc = -img[bi, near[:, 1].clamp(0, h - 1).long(), near[:, 0].clamp(0, w - 1).long()]      # [B, N, 64]
    elif feat == "trained":
        wave = torch.randn(B, 2, 1, 64, generator=g) * TRAINED_SIGMA
        phase = torch.rand(B, 1, 64, generator=g) * 6.283185307179586
        fourier = lambda x, y: torch.cos(x.unsqueeze(-1) * wave[:, 0] + y.unsqueeze(-1) * wave[:, 1] + phase)       # x, y [B, K] -> [B, K, 64]
        yy, xx = torch.meshgrid(torch.arange(h, dtype=F32), torch.arange(w, dtype=F32), indexing="ij")
        img = _unit(fourier(xx.reshape(1, -1).expand(B, -1), yy.reshape(1, -1).expand(B, -1))).view(B, h, w, 64)
        pc = _unit(_unit(fourier(near[:, 0], near[:, 1])) + 1e-2 * torch.randn(B, N, 64, generator=g))
    else:
        img = _unit(torch.randn(B, h, w, 64, generator=g))
        pc = _unit(torch.randn(B, N, 64, generator=g))
    pc = pc.reshape(B * N, 64).contiguous()
    if special == "dzero":
        for b in range(B):
            pc[b * N + pc_idx[b, 3]] = img[b, xy_int[b, 1, 5], xy_int[b, 0, 5]]
    return {"B": B, "N": N, "h": h, "w": w, "n": n, "feat": feat, "mask": mask, "special": special, "pc": pc, "img": img.contiguous(),
            "pc_idx": pc_idx.contiguous(), "xy_int": xy_int.contiguous(), "xy_float": xy_float}


def _cycled(shapes, full):
    """(n, B, feat, mask): the feature x mask families cycled over the shapes (each of the six meets several shapes), all six at `full`"""
    out = [(n, B, FEATS[k % 3], MASKS[k % 2]) for k, (n, B) in enumerate(shapes)]
    for n, B in full:
        out += [(n, B, f, m) for f in FEATS for m in MASKS if (n, B, f, m) not in out]
    return out


CIRCLE_FWD_CASES = _cycled([(n, B) for n in (1, 3, 15, 16, 17, 65, 257) for B in (1, 3)] + [(512, 1)], full=[(16, 1), (65, 3)])
CIRCLE_FWD_OTHER = [(17, 3, "random", "sparse"), (257, 1, "trained", "dense")]        # with OTHER_PARAMS
CIRCLE_BWD_CASES = _cycled([(n, B) for n in (1, 7, 8, 9, 64, 65, 130) for B in (1, 2)], full=[(9, 2), (65, 1)])
CIRCLE_BWD_OTHER = [(9, 2, "random", "dense"), (65, 1, "trained", "sparse")]
CIRCLE_BWD_SPECIAL = [(130, 2, "random", "sparse", "repeat"), (9, 1, "random", "sparse", "dzero"), (65, 2, "trained", "dense", "dzero")]


def bwd_grad_scale(n, B):
    """the grad_scale a backward case runs with: 1 and 0.37 both meet every loop structure"""
    return 0.37 if (n + B) % 2 else 1.0


def _softplus_grad(x):
    return torch.where(x > 20.0, torch.ones_like(x), torch.sigmoid(x))                # d F.softplus / dx as torch defines it


@torch.enable_grad()          # other test modules switch autograd off process-wide at import
def circle_forward(c, params=None, dtype=F64, grad=False, grad_scale=1.0):
    """-> dict: d [B, n, n] pair distances, mask [B, n, n] bool, on_thres (count of pairs exactly on the threshold), gap (min |dist - thres|
    over the others), terms [B, 2n] (per sample the n row terms, then the n column terms), arg [B, 2n] (the softplus arguments), loss
    = lam * sum(terms) / (B n).  grad=True adds d_pc [B N, 64], d_img [B, h, w, 64]: autograd of grad_scale * loss / lam with the distance
    of every d = 0 pair detached."""
    P = dict(PRODUCT_PARAMS if params is None else params)
    thres, pm, nm, ls, lam = (f32(P[k]) for k in ("dist_thres", "pos_margin", "neg_margin", "log_scale", "lam"))
    B, N, n = c["B"], c["N"], c["n"]
    pc = c["pc"].to(dtype).view(B, N, 64).clone().requires_grad_(grad)
    img = c["img"].to(dtype).clone().requires_grad_(grad)
    bi = torch.arange(B)[:, None]
    pts = pc[bi, c["pc_idx"]]                                                         # [B, n, 64]
    pix = img[bi, c["xy_int"][:, 1], c["xy_int"][:, 0]]
    diff = pts[:, :, None, :] - pix[:, None, :, :]
    sq = (diff * diff).sum(-1)
    zero = sq.detach() == 0
    d = torch.sqrt(torch.where(zero, torch.ones_like(sq), sq)) * (~zero)              # = sqrt(sq), with no gradient through d = 0
    fx = c["xy_float"].to(dtype)[:, :, :, None] - c["xy_int"].to(dtype)[:, :, None, :]
    dist = torch.sqrt((fx * fx).sum(1))
    m = dist <= thres
    mf = m.to(dtype)
    pos = d - 1e5 * (1 - mf)
    pw = torch.clamp_min((pos - pm).detach(), 0)
    tp = ls * (pos - pm) * pw
    neg = d + 1e5 * mf
    nw = torch.clamp_min((nm - neg).detach(), 0)
    tn = ls * (nm - neg) * nw
    lpr, lpc = torch.logsumexp(tp, -1), torch.logsumexp(tp, -2)
    lnr, lnc = torch.logsumexp(tn, -1), torch.logsumexp(tn, -2)
    arg = torch.cat([lpr + lnr, lpc + lnc], 1)
    terms = F.softplus(arg) / ls
    mean = terms.sum() / (B * n)
    off = dist != thres
    out = {"d": d.detach(), "mask": m, "on_thres": int((~off).sum()), "gap": float((dist - thres).abs()[off].min()) if off.any() else float("inf"),
           "terms": terms.detach(), "arg": arg.detach(), "loss": (lam * mean).detach(), "zero": zero,
           "parts": tuple(t.detach() for t in (diff, tp, tn, pw, nw, lpr, lpc, lnr, lnc))}
    if grad:
        (f32(grad_scale) * mean).backward()
        out["d_pc"] = pc.grad.reshape(B * N, 64)
        out["d_img"] = img.grad
    return out


def circle_backward(c, params=None, grad_scale=1.0):
    """closed-form float64 gradient of grad_scale * mean(terms) (module docstring) -> dict: d_pc [B N, 64], d_img [B, h, w, 64],
    named_pc [B N] / named_img [B, h, w] bool (rows some sample names), and the forward's dict under "fwd"."""
    fw = circle_forward(c, params, F64)
    diff, tp, tn, pw, nw, lpr, lpc, lnr, lnc = fw["parts"]
    B, N, n, h, w = c["B"], c["N"], c["n"], c["h"], c["w"]
    sr, sc = _softplus_grad(lpr + lnr), _softplus_grad(lpc + lnc)
    gp = sr[:, :, None] * torch.exp(tp - lpr[:, :, None]) + sc[:, None, :] * torch.exp(tp - lpc[:, None, :])
    gn = sr[:, :, None] * torch.exp(tn - lnr[:, :, None]) + sc[:, None, :] * torch.exp(tn - lnc[:, None, :])
    g = f32(grad_scale) * (pw * gp - nw * gn) / (B * n)
    d = fw["d"]
    G = torch.where(d > 0, g / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(d))
    dpts = (G[..., None] * diff).sum(2)
    dpix = -(G[..., None] * diff).sum(1)
    bi = torch.arange(B)[:, None]
    rows_pc = (bi * N + c["pc_idx"]).reshape(-1)
    rows_img = (bi * h * w + c["xy_int"][:, 1] * w + c["xy_int"][:, 0]).reshape(-1)
    d_pc = torch.zeros(B * N, 64, dtype=F64).index_add_(0, rows_pc, dpts.reshape(-1, 64))
    d_img = torch.zeros(B * h * w, 64, dtype=F64).index_add_(0, rows_img, dpix.reshape(-1, 64))
    named_pc = torch.zeros(B * N, dtype=torch.bool)
    named_pc[rows_pc] = True
    named_img = torch.zeros(B * h * w, dtype=torch.bool)
    named_img[rows_img] = True
    return {"d_pc": d_pc, "d_img": d_img.view(B, h, w, 64), "named_pc": named_pc, "named_img": named_img.view(B, h, w), "fwd": fw}


def prefill(shape, scale, seed):
    """what a gradient buffer holds before the circle loss adds to it: seeded, non-zero, of the gradient's own scale (the product's buffers
    hold the other heads' gradients; at a larger scale the fp32 sum's rounding would hide the addend)"""
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(shape, generator=g) + 0.25) * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return (t * float(scale)).to(F32)


def circle_prefill(c, ref):
    """(d_pc, d_img) float32 buffers as a backward case finds them, each at the scale of the gradient (ref = circle_backward's dict)
    that it is about to receive"""
    return (prefill(ref["d_pc"].shape, ref["d_pc"].abs().max(), 31 + c["n"]), prefill(ref["d_img"].shape, ref["d_img"].abs().max(), 57 + c["n"]))


def circle_grad_err(got, pre, ref):
    """the gradient metric: |got - (pre + ref)| of the gradient tensor's largest entry"""
    return scaled_err(got, pre.double() + ref, float(ref.abs().max()))


# ---- F.normalize over 64 channels ----------------------------------------------------------------------------------------------------------
L2NORM_ROWS = (1, 15, 16, 17, 1000)
L2NORM_EPS = 1e-12


@functools.lru_cache(maxsize=None)
def l2norm_case(rows):
    """x, dy float32 [rows, 64]: row norms spread log-uniformly over 1e-6 ... 1e6 (both ends present from 15 rows on), row 7 exactly
    zero where there is one"""
    g = torch.Generator().manual_seed(9000 + rows)
    e = torch.rand(rows, generator=g) * 12 - 6
    if rows > 2:
        e[1], e[2] = -6.0, 6.0
    x = (F.normalize(torch.randn(rows, 64, generator=g).double(), dim=1) * (10.0 ** e.double())[:, None]).to(F32)
    if rows > 7:
        x[7] = 0
    dy = torch.randn(rows, 64, generator=g).to(F32)
    return x, dy


@torch.enable_grad()          # other test modules switch autograd off process-wide at import
def l2norm(x, dy=None, dtype=F64):
    """-> dict: y = x / max(|x|, 1e-12); with dy also dx in closed form (a zero row: y = 0, dx = dy / 1e-12), dx_autograd, and
    scale [rows] = max|dy_row| / max(|x_row|, 1e-12), the size a row's gradient is measured against."""
    xx = x.detach().to(dtype).clone().requires_grad_(dy is not None)
    y = F.normalize(xx, dim=1, eps=L2NORM_EPS)
    out = {"y": y.detach()}
    if dy is not None:
        g = dy.to(dtype)
        y.backward(g)
        with torch.no_grad():
            nrm = xx.norm(dim=1, keepdim=True)
            dn = nrm.clamp_min(L2NORM_EPS)
            dx = g / dn - torch.where(nrm >= L2NORM_EPS, xx * (xx * g).sum(1, keepdim=True) / dn ** 3, torch.zeros_like(xx))
            out.update(dx=dx, dx_autograd=xx.grad.detach(), scale=(g.abs().max(1).values / dn[:, 0]))
    return out
