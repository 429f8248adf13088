"""Plain CPU restatements of the train-mode transformer-block and linear-attention entry points (float64 torch unless a dtype is asked
for), the comparisons the GPU tests make with them, and the inputs of those tests -- so that tests/test_block_train_cpu.py can show,
without a GPU, that every hand-written backward equals autograd of its forward, that every comparison rejects a wrong result and that
fp32 evaluation of the same formulas stays inside every bar.

Formulas: the ViT tail is ImageViT.py:81-158 (x1 = x + drop(ctx Wo^T + bo); out = x1 + drop(W2 drop(gelu(W1 LN(x1) + b1)) + b2)); the
linear-attention layer is LinearAttention.py:38-73 (state KV = K^T V / S, Ksum; message = Q KV / (Q . Ksum + eps) S; merge, LayerNorm,
MLP on cat[x, message], LayerNorm, residual); softmax attention is 8 heads x 8 dims with logits / sqrt 8.  Dropout masks restate
csrc/cmr_common.h (cmr_mix64 / cmr_keep / cmr_drop_threshold) with the element index row * width + column of the tensor the reference's
nn.Dropout sees.  No GPU import in this file."""

import numpy as np
import torch
import torch.nn.functional as F

from point_train_reference import MASK_BAND, MASK_BAND_CAP, close, rel_err, relu_mask_agrees  # noqa: F401  (one definition of each)

f32, f64 = torch.float32, torch.float64


def rnd(*shape, seed=0, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


# ------------------------------------------------------------------------------------------------------------------------------- mask
_GOLD = np.uint64(0x9E3779B97F4A7C15)


def mix64(x):
    """cmr_mix64 (murmur3 finaliser) on a numpy uint64 array; products wrap modulo 2^64 as the device's do"""
    x = np.asarray(x, dtype=np.uint64).copy()
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return x


def drop_threshold(p):
    """cmr_drop_threshold: p arrives as a float (fp32), the product is taken in double"""
    t = float(np.float32(p)) * 4294967296.0
    return 0 if t <= 0.0 else (4294967295 if t >= 4294967295.0 else int(t))


def keep_scale(p):
    """1.f / (1.f - p) as the entry points compute it, in fp32"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(seed, site, n, p):
    """cmr_keep for element indices 0 .. n-1 of dropout site `site` under `seed` -> numpy bool [n], True = kept"""
    key = mix64(np.array([seed & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64) + np.array([site], dtype=np.uint64) * _GOLD)[0]
    low = mix64(key ^ np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    return low >= np.uint64(drop_threshold(p))


class Drop:
    """the dropout of one call: seed, and per site (number, p).  mul(name, shape) -> mask * 1 / (1 - p) for a tensor of that shape whose
    elements are numbered in row-major order (1.0 without dropout)."""

    def __init__(self, seed, sites, swap=None, unscaled=None):
        self.seed, self.sites, self.swap, self.unscaled = seed, dict(sites), swap, unscaled       # swap / unscaled: planted errors

    def mul(self, name, shape, dtype=f64):
        site, p = self.sites[name]
        if self.swap and name in self.swap:
            site = self.sites[self.swap[name]][0]
        if p <= 0.0:
            return torch.ones(shape, dtype=dtype)
        keep = torch.from_numpy(keep_mask(self.seed, site, int(np.prod(shape)), p)).reshape(shape)
        return keep.to(dtype) * (1.0 if self.unscaled == name else keep_scale(p))


class NoDrop:
    seed = None

    def mul(self, name, shape, dtype=f64):
        return torch.ones(shape, dtype=dtype)


SEED = 0x5DEECE66D          # the seed of every case with dropout


# ---------------------------------------------------------------------------------------------------------------------------- helpers
def ln_fwd(x, g, b, eps):
    xc = x - x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    xh = xc * rstd
    return xh * g + b, xh, rstd


def ln_bwd(dy, xh, rstd, g):
    """-> dx, d gamma, d beta (sums over the rows)"""
    dxh = dy * g
    s1, s2 = dxh.mean(-1, keepdim=True), (dxh * xh).mean(-1, keepdim=True)
    return rstd * (dxh - s1 - xh * s2), (dy * xh).sum(0), dy.sum(0)


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752440))


def gelu_grad(v):
    return 0.5 * (1.0 + torch.erf(v * 0.70710678118654752440)) + v * 0.39894228040143267794 * torch.exp(-0.5 * v * v)


def elu1(v, exp2=False):
    """F.elu(v) + 1; exp2: the negative branch as 2^(v log2 e), as the fused kernels evaluate it"""
    neg = torch.exp2(v * 1.4426950408889634) if exp2 else torch.exp(v)
    return torch.where(v > 0, v + 1.0, neg)


def _c(d, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in d.items()}


def ln_totals(lnpart):
    """[parts, 128] partial rows of d gamma | d beta -> their float64 totals"""
    t = lnpart.detach().cpu().double().sum(0)
    return t[:64], t[64:]


def tile_partials(term_g, term_b, tile):
    """per-row LayerNorm terms [rows, 64] x 2 -> [tiles, 128] sums over tiles of `tile` rows (what a kernel's lnpart holds)"""
    rows = term_g.shape[0]
    nt = (rows + tile - 1) // tile
    out = torch.zeros(nt, 128, dtype=term_g.dtype)
    idx = torch.arange(rows) // tile
    out[:, :64].index_add_(0, idx, term_g)
    out[:, 64:].index_add_(0, idx, term_b)
    return out


# ------------------------------------------------------------------------------------------------------------------------------- bars
BAR_FWD = 2e-5              # forward outputs and saved activations (the block-level tests' bar)
BAR_GRAD = 5e-5             # data gradients
BAR_VIT_LN = 1e-4           # ViT LayerNorm parameter sums
BAR_LA_LN = 2e-4            # linear-attention LayerNorm parameter sums
FP32_MARGIN = 4.0           # fp32-on-CPU evaluation of the restatement must fit inside bar / 4


# --------------------------------------------------------------------------------------------------------------------------- ViT tail
def vit_weights(seed=300):
    return dict(wo=rnd(64, 64, seed=seed, lo=-0.3, hi=0.3), bo=rnd(64, seed=seed + 1), g2=rnd(64, seed=seed + 2, lo=0.5, hi=1.5),
                b2n=rnd(64, seed=seed + 3), w1=rnd(1024, 64, seed=seed + 4, lo=-0.3, hi=0.3), b1=rnd(1024, seed=seed + 5),
                w2=rnd(64, 1024, seed=seed + 6, lo=-0.1, hi=0.1), b2=rnd(64, seed=seed + 7), eps=1e-5)


VIT_SITES = dict(proj=(11, 0.1), act=(12, 0.3), fc2=(13, 0.3))      # p_proj != p_mlp


def vit_drop(on):
    return Drop(SEED, VIT_SITES) if on else NoDrop()


def vit_tail(w, ctx, x, drop, dtype=f64, transposed=None):
    """-> dict x1, out (what the kernel stores) and the intermediates h = LN(x1), u (fc1 pre-activation), gs (hidden after dropout).
    transposed: name of a weight used as its transpose (a planted error; square weights only)."""
    w, ctx, x = _c(w, dtype), ctx.to(dtype), x.to(dtype)
    rows = x.shape[0]
    wo = w["wo"].T if transposed == "wo" else w["wo"]
    proj = ctx @ wo.T + w["bo"]
    x1 = x + proj * drop.mul("proj", (rows, 64), dtype)
    h, _, _ = ln_fwd(x1, w["g2"], w["b2n"], w["eps"])
    u = h @ w["w1"].T + w["b1"]
    gs = gelu(u) * drop.mul("act", (rows, 1024), dtype)
    y = gs @ w["w2"].T + w["b2"]
    out = x1 + y * drop.mul("fc2", (rows, 64), dtype)
    return dict(x1=x1, out=out, h=h, u=u, gs=gs, proj=proj, y=y)


def vit_ffn_bwd(w, x1, dout, drop, dtype=f64, transposed=None):
    """backward of vit_tail from d out -> dx1, dctx, gs, du, h, dm, da, ln_g, ln_b and the per-row terms of the LayerNorm sums"""
    w, x1, dout = _c(w, dtype), x1.to(dtype), dout.to(dtype)
    rows = x1.shape[0]
    dm = dout * drop.mul("fc2", (rows, 64), dtype)
    h, xh, rstd = ln_fwd(x1, w["g2"], w["b2n"], w["eps"])
    u = h @ w["w1"].T + w["b1"]
    mact = drop.mul("act", (rows, 1024), dtype)
    gs = gelu(u) * mact
    du = (dm @ w["w2"]) * mact * gelu_grad(u)
    dh = du @ w["w1"]
    dx, ln_g, ln_b = ln_bwd(dh, xh, rstd, w["g2"])
    dx1 = dout + dx
    da = dx1 * drop.mul("proj", (rows, 64), dtype)
    wo = w["wo"].T if transposed == "wo" else w["wo"]
    return dict(dx1=dx1, dctx=da @ wo, gs=gs, du=du, h=h, dm=dm, da=da, ln_g=ln_g, ln_b=ln_b, term_g=dh * xh, term_b=dh)


# rows: one row; one full 16-row tile; one row into the second tile; 16 full tiles + 14 rows.  strided: ctx and x are column slices of
# wider buffers (ld 128 and 192)
VIT_CASES = [(rows, drop, rows in (17, 270)) for rows in (1, 16, 17, 270) for drop in (False, True)]


def vit_case(rows, drop, strided, seed=310):
    """-> (weights, ctx, x, dout, Drop)"""
    ctx = rnd(rows, 128, seed=seed)[:, 64:128] if strided else rnd(rows, 64, seed=seed)
    x = rnd(rows, 192, seed=seed + 1)[:, 64:128] if strided else rnd(rows, 64, seed=seed + 1)
    return vit_weights(), ctx, x, rnd(rows, 64, seed=seed + 2), vit_drop(drop)


VIT_FWD_BARS = dict(x1=BAR_FWD, out=BAR_FWD)
VIT_BWD_BARS = dict(dx1=BAR_GRAD, dctx=BAR_GRAD, gs=BAR_FWD, du=BAR_GRAD, h=BAR_FWD, dm=BAR_GRAD, da=BAR_GRAD, ln_g=BAR_VIT_LN, ln_b=BAR_VIT_LN)


# A gradient that is the difference of two terms of size C carries their fp32 rounding, some ulp of C, however small the difference is:
# with one key softmax attention has P = 1 and dP = D, so dq = dk = 0, and with one source row the linear-attention message does not
# depend on qf or kf but through eps.  Where a reference is below this share of its cancelling terms -- more than two of fp32's seven
# digits lost -- the error is measured against that share of C instead of max |ref|: bar x share = 5e-7 C, 8 ulp of the terms.  Nothing
# changes for a tensor that is not cancelled.
CANCEL_SHARE = 1e-2


def close_on(got, ref, rtol, name, cancel):
    """close() with the scale max(max |ref|, CANCEL_SHARE x cancel)"""
    floor = CANCEL_SHARE * cancel
    if float(ref.abs().max()) >= floor:
        return close(got, ref, rtol, name)
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    err = (got - ref.detach().cpu().double()).abs().max()
    e = float("inf") if not bool(torch.isfinite(err)) else float(err) / floor
    assert e <= rtol, "%s (cancelled): max|d| / scale = %.3e > %.1e" % (name, e, rtol)
    return e


def _check(got, ref, bars, scale=1.0, cancel=None):
    cancel = cancel or {}
    return {key: close_on(got[key], ref[key], bar * scale, key, cancel.get(key, 0.0)) for key, bar in bars.items()}


def check_vit_fwd(got, ref, scale=1.0):
    return _check(got, ref, VIT_FWD_BARS, scale)


def check_vit_ffn_bwd(got, ref, scale=1.0):
    """got: dict of the kernel's row outputs + ln_g / ln_b = ln_totals(lnpart)"""
    return _check(got, ref, VIT_BWD_BARS, scale)


# ---------------------------------------------------------------------------------------------------- LayerNorm + q / k / v backward
def lnqkv_weights(seed=330):
    """[Wq; Wk; Wv] stacked [192, 64], LayerNorm gamma / beta"""
    return dict(wcat=rnd(192, 64, seed=seed, lo=-0.3, hi=0.3), g=rnd(64, seed=seed + 1, lo=0.5, hi=1.5), b=rnd(64, seed=seed + 2), eps=1e-5)


def lnqkv_problem(wpart, d, x, res, g, b, eps, dtype=f64, transposed=False):
    """one row set: d [rows, n] gradient at the projections' outputs, wpart [n, 64] their stacked weights -> dx, xn, per-row LN terms"""
    wpart, d, x, g, b = (t.to(dtype) for t in (wpart, d, x, g, b))
    xn, xh, rstd = ln_fwd(x, g, b, eps)
    dn = d @ wpart if not transposed else d @ wpart.T
    dx, _, _ = ln_bwd(dn, xh, rstd, g)
    if res is not None:
        dx = dx + res.to(dtype)
    return dict(dx=dx, xn=xn, term_g=dn * xh, term_b=dn)


def lnqkv_bwd(w, px, py=None, dtype=f64, transposed=False):
    """px / py: dict(d, x, res | None, lo, hi) with [lo, hi) the rows of wcat this problem's projections are.  -> dx, xn, (dy, yn,) ln_g, ln_b"""
    out = {}
    tg, tb = 0.0, 0.0
    for tag, pr in (("x", px), ("y", py)):
        if pr is None:
            continue
        r = lnqkv_problem(w["wcat"][pr["lo"]:pr["hi"]], pr["d"], pr["x"], pr.get("res"), w["g"], w["b"], w["eps"], dtype, transposed and tag == "x")
        out["d" + tag], out[tag + "n"] = r["dx"], r["xn"]
        out["terms_" + tag] = (r["term_g"], r["term_b"])
        tg, tb = tg + r["term_g"].sum(0), tb + r["term_b"].sum(0)
    out["ln_g"], out["ln_b"] = tg, tb
    return out


# (rows_x, k_x, res, rows_y, k_y): every row count around the 32-row tile with both widths, with and without the residual gradient; the
# cross block's two-problem form; and 2050 + 3 tiles, past the switch to four waves per workgroup at 2048, the second problem inside it
LNQKV_CASES = [(r, k, res, 0, 0) for r in (1, 31, 32, 33, 77) for k in (64, 192) for res in (False, True)] + \
              [(77, 64, True, 50, 128), (65536 + 33, 64, True, 70, 128)]


def lnqkv_case(rows_x, k_x, res, rows_y, k_y, seed=340):
    """-> (weights, px, py).  Self block: d = [dq | dk | dv] (k_x = 192) on the rows of x; cross block: dq on x, [dk | dv] on y.  k_x = 64
    alone is the query problem.  d is a column slice of a wider buffer."""
    w = lnqkv_weights()
    px = dict(d=rnd(rows_x, k_x + 64, seed=seed)[:, 64:], x=rnd(rows_x, 128, seed=seed + 1)[:, 0:64],
              res=rnd(rows_x, 64, seed=seed + 2) if res else None, lo=0, hi=k_x)
    py = None
    if rows_y:
        py = dict(d=rnd(rows_y, k_y, seed=seed + 3), x=rnd(rows_y, 64, seed=seed + 4), res=None, lo=64, hi=64 + k_y)
    return w, px, py


def check_lnqkv_bwd(got, ref, scale=1.0):
    bars = dict(dx=BAR_GRAD, xn=BAR_FWD, ln_g=BAR_VIT_LN, ln_b=BAR_VIT_LN)
    if "dy" in ref:
        bars.update(dy=BAR_GRAD, yn=BAR_FWD)
    return _check(got, ref, bars, scale)


# ------------------------------------------------------------------------------------------------------------ linear attention, forward
LA_EPS, LA_LN_EPS = 1e-6, 1e-5


def la_weights(seed=360):
    r = lambda n, k, s: rnd(n, k, seed=seed + s, lo=-0.3, hi=0.3)
    return dict(wq=r(64, 64, 0), wk=r(64, 64, 1), wv=r(64, 64, 2), wm=r(64, 64, 3), w0=rnd(128, 128, seed=seed + 4, lo=-0.2, hi=0.2),
                w3=rnd(64, 128, seed=seed + 5, lo=-0.2, hi=0.2), g1=rnd(64, seed=seed + 6, lo=0.5, hi=1.5), b1=rnd(64, seed=seed + 7),
                g2=rnd(64, seed=seed + 8, lo=0.5, hi=1.5), b2=rnd(64, seed=seed + 9))


def la_kv_state(w, y, B, S, dtype=f64, exp2=False, ksum_scaled=False):
    """source side -> kf = elu(Wk y) + 1, v = Wv y [B S, 64], kvsum [B, 576] = KV [h][d][v] scaled by 1 / S | Ksum [h][d] unscaled"""
    y, wk, wv = y.to(dtype), w["wk"].to(dtype), w["wv"].to(dtype)
    kf, v = elu1(y @ wk.T, exp2), y @ wv.T
    K, V = kf.view(B, S, 8, 8), v.view(B, S, 8, 8)
    kv = torch.einsum("bshd,bshv->bhdv", K, V) / S
    ksum = K.sum(1)
    if ksum_scaled:
        ksum = ksum / S
    return dict(kf=kf, v=v, kvsum=torch.cat([kv.reshape(B, 512), ksum.reshape(B, 64)], 1))


# S: one row; a partial tile; one row into the second tile; several workgroups; and 8193 + 32, where a wave takes two tiles
LA_KV_CASES = [(B, S, S in (33, 257)) for B in (1, 3) for S in (1, 31, 33, 257, 8193 + 32)]


def la_kv_case(B, S, strided, seed=370):
    y = rnd(B * S, 128, seed=seed)[:, 32:96] if strided else rnd(B * S, 64, seed=seed)
    return la_weights(), y


LA_KV_BARS = dict(kf=BAR_FWD, v=BAR_FWD, kvsum=BAR_FWD)


def check_la_kv_state(got, ref, scale=1.0):
    figs = _check(got, ref, LA_KV_BARS, scale)
    # the two blocks of the state separately: Ksum is some S times larger than KV and would hide it
    figs["kv"] = close(got["kvsum"][:, :512], ref["kvsum"][:, :512], BAR_FWD * scale, "kvsum[:, :512]")
    figs["ksum"] = close(got["kvsum"][:, 512:], ref["kvsum"][:, 512:], BAR_FWD * scale, "kvsum[:, 512:]")
    return figs


LA_SITES = dict(att=(21, 0.1), hid=(22, 0.1), out=(23, 0.1))
LA_P = 0.1


def la_drop(on):
    return Drop(SEED, LA_SITES) if on else NoDrop()


def la_message(qf, kvsum, B, L, S, eps):
    Q = qf.view(B, L, 8, 8)
    KV, Ks = kvsum[:, :512].reshape(B, 8, 8, 8), kvsum[:, 512:].reshape(B, 8, 8)
    num = torch.einsum("blhd,bhdv->blhv", Q, KV)
    den = torch.einsum("blhd,bhd->blh", Q, Ks) + eps
    return (num / den[..., None] * S).reshape(B * L, 64)


def la_mlp_fwd(w, x, msg, drop, dtype=f64, transposed=None):
    """merge .. LayerNorm 2 from the message: mm, n1, d1, hid_pre, hid, o, y2 = LN2(o)"""
    rows = x.shape[0]
    wm = w["wm"].T if transposed == "wm" else w["wm"]
    mm = msg @ wm.T
    n1, _, _ = ln_fwd(mm, w["g1"], w["b1"], LA_LN_EPS)
    d1 = n1 * drop.mul("att", (rows, 64), dtype)
    hid_pre = torch.cat([x, d1], 1) @ w["w0"].T
    hid_keep = drop.mul("hid", (rows, 128), dtype)
    hid = F.relu(hid_pre) * hid_keep
    o_pre = hid @ w["w3"].T
    o = o_pre * drop.mul("out", (rows, 64), dtype)
    y2, _, _ = ln_fwd(o, w["g2"], w["b2"], LA_LN_EPS)
    return dict(mm=mm, n1=n1, d1=d1, hid_pre=hid_pre, hid_keep=hid_keep, hid=hid, o_pre=o_pre, o=o, y2=y2)


def la_query_layer(w, x, kvsum, B, L, S, drop, dtype=f64, exp2=False, transposed=None):
    """query side -> qf, msg, mm, d1, hid, o, out (what the kernel stores) and hid_pre"""
    w, x, kvsum = _c(w, dtype), x.to(dtype), kvsum.to(dtype)
    qf = elu1(x @ w["wq"].T, exp2)
    msg = la_message(qf, kvsum, B, L, S, LA_EPS)
    r = la_mlp_fwd(w, x, msg, drop, dtype, transposed)
    r.update(qf=qf, msg=msg, out=x + r["y2"])
    return r


# (B, L): one row; tiles that straddle batch elements; full tiles; the second trip of the persistent loop (256 workgroups x 8 tiles x 32
# rows) with a partly idle grid
LA_QUERY_CASES = [(B, L, drop) for (B, L) in ((1, 1), (3, 33), (2, 144), (1, 65536 + 288)) for drop in (False, True)]
LA_QUERY_S = 40


def la_query_case(B, L, seed=380):
    """-> (weights, x, kvsum, S): the state comes from the source-side restatement on S rows per batch element"""
    w = la_weights()
    kvsum = la_kv_state(w, rnd(B * LA_QUERY_S, 64, seed=seed + 1), B, LA_QUERY_S)["kvsum"].float()
    return w, rnd(B * L, 64, seed=seed), kvsum, LA_QUERY_S


LA_QUERY_BARS = dict(qf=BAR_FWD, msg=BAR_FWD, mm=BAR_FWD, d1=BAR_FWD, hid=BAR_FWD, o=BAR_FWD, out=BAR_FWD)


def check_la_query(got, ref, scale=1.0):
    figs = _check(got, ref, LA_QUERY_BARS, scale)
    pre, keep = ref["hid_pre"], ref["hid_keep"] != 0
    hid = got["hid"].detach().cpu()
    assert bool((hid[~keep] == 0).all()), "hid: a dropped entry is not zero"
    wrong, share = relu_mask_agrees(hid[keep], pre[keep], MASK_BAND * float(pre.abs().max()))
    figs["hid_band_share"] = share
    assert share <= MASK_BAND_CAP, "hid: the band holds %.2e of the entries" % share
    assert wrong == 0, "hid: %d mask entries differ outside the band" % wrong
    return figs


# ----------------------------------------------------------------------------------------------------------- linear attention, backward
def la_mlp_bwd(w, sv, dout, drop, dtype=f64, transposed=None):
    """from d out (the gradient at LN2's output) and the saved o, hid, mm -> d_o, d_hid, d_mm, d_msg, d_xa, the two LayerNorms' sums"""
    w, dout = _c(w, dtype), dout.to(dtype)
    o, hid, mm = (sv[k].to(dtype) for k in ("o", "hid", "mm"))
    rows = o.shape[0]
    _, xh2, rstd2 = ln_fwd(o, w["g2"], w["b2"], LA_LN_EPS)
    dO, g2s, b2s = ln_bwd(dout, xh2, rstd2, w["g2"])
    d_o = dO * drop.mul("out", (rows, 64), dtype)
    ks = keep_scale(drop.sites["hid"][1]) if drop.seed is not None else 1.0                   # hid > 0 iff kept and active
    d_hid = torch.where(hid > 0, (d_o @ w["w3"]) * ks, torch.zeros((), dtype=dtype))
    dc = d_hid @ w["w0"]
    d_xa = dc[:, :64]
    dn = dc[:, 64:] * drop.mul("att", (rows, 64), dtype)
    _, xh1, rstd1 = ln_fwd(mm, w["g1"], w["b1"], LA_LN_EPS)
    d_mm, g1s, b1s = ln_bwd(dn, xh1, rstd1, w["g1"])
    wm = w["wm"].T if transposed == "wm" else w["wm"]
    return dict(d_o=d_o, d_hid=d_hid, d_mm=d_mm, d_msg=d_mm @ wm, d_xa=d_xa, ln1_g=g1s, ln1_b=b1s, ln2_g=g2s, ln2_b=b2s,
                terms1=(dn * xh1, dn), terms2=(dout * xh2, dout))


# rows: one row; one tile; one row into the second tile; the second workgroup with one live wave; the second trip of the persistent loop
LA_MLP_CASES = [(rows, drop) for rows in (1, 32, 33, 8 * 32 + 1, 65536 + 288) for drop in (False, True)]


def la_mlp_case(rows, drop, seed=400):
    """-> (weights, saved dict o / hid / mm in fp32 as the forward restatement leaves them, dout, Drop)"""
    w = la_weights()
    d = la_drop(drop)
    x, msg = rnd(rows, 64, seed=seed).double(), rnd(rows, 64, seed=seed + 1).double()
    r = la_mlp_fwd(_c(w, f64), x, msg, d)
    return w, {k: r[k].float() for k in ("o", "hid", "mm")}, rnd(rows, 64, seed=seed + 2), d


LA_MLP_BARS = dict(d_o=BAR_GRAD, d_hid=BAR_GRAD, d_mm=BAR_GRAD, d_msg=BAR_GRAD, d_xa=BAR_GRAD, ln1_g=BAR_LA_LN, ln1_b=BAR_LA_LN,
                   ln2_g=BAR_LA_LN, ln2_b=BAR_LA_LN)


def check_la_mlp_bwd(got, ref, scale=1.0):
    return _check(got, ref, LA_MLP_BARS, scale)


def la_proj_problem(terms, res, dtype=f64, transposed=None):
    """terms: [(d, f | None, W [64, 64])] -> dx = sum_i e_i W_i + residual gradients, e_i = d_i (f_i > 1 ? 1 : f_i) for the saved
    f = elu + 1 (d_i itself without f); -> dict dx, e (list, None where there is no f)"""
    dx, es = 0.0, []
    for i, (d, f, wt) in enumerate(terms):
        d, wt = d.to(dtype), wt.to(dtype)
        e = d if f is None else d * torch.where(f.to(dtype) > 1, torch.ones((), dtype=dtype), f.to(dtype))
        es.append(None if f is None else e)
        dx = dx + e @ (wt.T if transposed == i else wt)
    for r in res:
        dx = dx + r.to(dtype)
    return dict(dx=dx, e=es)


# (form, rows_x, rows_y): self = one problem with q, k (saved f, e written in place) and v (neither) and both residual inputs; cross = the
# query rows (1 term, both residuals) and the source rows (2 terms, none).  The last case of each is above 2048 tiles in total.
LA_PROJ_CASES = [("self", 1, 0), ("self", 33, 0), ("self", 77, 0), ("cross", 1, 33), ("cross", 33, 77), ("cross", 77, 1),
                 ("self", 65536 + 33, 0), ("cross", 65536 - 31, 77)]


def la_saved_f(rows, seed):
    """a saved elu + 1 in (0.05, 3) with entries exactly 1.0, just below and just above"""
    f = rnd(rows, 64, seed=seed, lo=0.05, hi=3.0)
    flat = f.reshape(-1)
    flat[0::7] = 1.0
    flat[3::11] = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    flat[5::13] = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    return f


def la_proj_case(form, rows_x, rows_y, seed=420):
    """-> (weights, problems): problems = [dict(rows, terms=[(d, f | None, name of W)], res=[...])]; d of the first term is a column slice"""
    w = la_weights()
    d = lambda r, s: rnd(r, 64, seed=seed + s)
    dq = rnd(rows_x, 128, seed=seed)[:, 64:]
    if form == "self":
        return w, [dict(rows=rows_x, terms=[(dq, la_saved_f(rows_x, seed + 1), "wq"), (d(rows_x, 2), la_saved_f(rows_x, seed + 3), "wk"),
                                            (d(rows_x, 4), None, "wv")], res=[d(rows_x, 5), d(rows_x, 6)])]
    return w, [dict(rows=rows_x, terms=[(dq, la_saved_f(rows_x, seed + 1), "wq")], res=[d(rows_x, 5), d(rows_x, 6)]),
               dict(rows=rows_y, terms=[(d(rows_y, 2), la_saved_f(rows_y, seed + 3), "wk"), (d(rows_y, 4), None, "wv")], res=[])]


def la_proj_bwd(w, problems, dtype=f64, transposed=None):
    return [la_proj_problem([(d, f, w[name]) for d, f, name in pr["terms"]], pr["res"], dtype, transposed) for pr in problems]


def check_la_proj_bwd(got, ref, scale=1.0):
    """got / ref: per problem dict(dx, e=[...])"""
    figs = {}
    for i, (g, r) in enumerate(zip(got, ref)):
        figs["dx%d" % i] = close(g["dx"], r["dx"], BAR_GRAD * scale, "dx of problem %d" % i)
        for j, (ge, re_) in enumerate(zip(g["e"], r["e"])):
            if re_ is not None:
                figs["e%d%d" % (i, j)] = close(ge, re_, BAR_GRAD * scale, "e of problem %d term %d" % (i, j))
    return figs


def la_core(qf, kf, v, B, L, S, eps):
    """the attention message from qf, kf, v (the forward la_bwd differentiates)"""
    K, V = kf.view(B, S, 8, 8), v.view(B, S, 8, 8)
    kvsum = torch.cat([(torch.einsum("bshd,bshv->bhdv", K, V) / S).reshape(B, 512), K.sum(1).reshape(B, 64)], 1)
    return la_message(qf, kvsum, B, L, S, eps), kvsum


def la_bwd(qf, kf, v, kvsum, dmsg, B, L, S, eps, dtype=f64, ksum_scaled=False):
    """d msg -> dqf, dkf, dv with the state given"""
    qf, kf, v, kvsum, dmsg = (t.to(dtype) for t in (qf, kf, v, kvsum, dmsg))
    Q, K, V, G = qf.view(B, L, 8, 8), kf.view(B, S, 8, 8), v.view(B, S, 8, 8), dmsg.view(B, L, 8, 8)
    KV, Ks = kvsum[:, :512].reshape(B, 8, 8, 8), kvsum[:, 512:].reshape(B, 8, 8)
    num = torch.einsum("blhd,bhdv->blhv", Q, KV)
    den = torch.einsum("blhd,bhd->blh", Q, Ks) + eps
    dnum = S * G / den[..., None]
    dden = -(G * (S * num / den[..., None])).sum(-1) / den
    dqf = torch.einsum("blhv,bhdv->blhd", dnum, KV) + dden[..., None] * Ks[:, None]
    dKV = torch.einsum("blhd,blhv->bhdv", Q, dnum)
    dKs = torch.einsum("blh,blhd->bhd", dden, Q)
    if ksum_scaled:
        dKs = dKs / S
    dkf = torch.einsum("bhdv,bshv->bshd", dKV, V) / S + dKs[:, None]
    dv = torch.einsum("bshd,bhdv->bshv", K, dKV) / S
    cancel = dict(dqf=float((torch.einsum("blhv,bhdv->blhd", dnum.abs(), KV.abs()) + dden.abs()[..., None] * Ks.abs()[:, None]).max()),
                  dkf=float((torch.einsum("bhdv,bshv->bshd", dKV.abs(), V.abs()) / S + dKs.abs()[:, None]).max()))
    return dict(cancel=cancel, dqf=dqf.reshape(B * L, 64), dkf=dkf.reshape(B * S, 64), dv=dv.reshape(B * S, 64))


LA_BWD_CASES = [(1, 1), (15, 17), (64, 64), (65, 130)]
LA_BWD_B = 2


def la_bwd_case(L, S, seed=440):
    """-> qf, kf in (0.05, 3) as elu + 1 produces, v, d msg, and the accumulate targets' earlier contents"""
    B = LA_BWD_B
    qf, kf = rnd(B * L, 64, seed=seed, lo=0.05, hi=3.0), rnd(B * S, 64, seed=seed + 1, lo=0.05, hi=3.0)
    return dict(qf=qf, kf=kf, v=rnd(B * S, 64, seed=seed + 2), dmsg=rnd(B * L, 64, seed=seed + 3),
                old=dict(dqf=rnd(B * L, 64, seed=seed + 4), dkf=rnd(B * S, 64, seed=seed + 5), dv=rnd(B * S, 64, seed=seed + 6)))


LA_BWD_BARS = dict(dqf=BAR_GRAD, dkf=BAR_GRAD, dv=BAR_GRAD)


def check_la_bwd(got, ref, scale=1.0):
    return _check(got, ref, LA_BWD_BARS, scale, ref["cancel"])


# ------------------------------------------------------------------------------------------------------------------ softmax attention
MHA_SCALE = 0.35355339059327373
MHA_SITE, MHA_P = 31, 0.1


def mha_mask(B, Tq, Tk, on, dtype=f64):
    """M = keep / (1 - p) on the probabilities, element ((b 8 + head) Tq + query) Tk + key; None without dropout"""
    if not on:
        return None
    keep = torch.from_numpy(keep_mask(SEED, MHA_SITE, B * 8 * Tq * Tk, MHA_P)).reshape(B, 8, Tq, Tk)
    return keep.to(dtype) * keep_scale(MHA_P)


def mha_fwd(q, k, v, B, Tq, Tk, M=None):
    Q, K, V = (t.view(B, -1, 8, 8).transpose(1, 2) for t in (q, k, v))
    P = torch.softmax(Q @ K.transpose(-1, -2) * MHA_SCALE, -1)
    if M is not None:
        P = P * M
    return (P @ V).transpose(1, 2).reshape(B * Tq, 64)


def mha_bwd(q, k, v, dout, B, Tq, Tk, M=None, dtype=f64, leak=False):
    """-> o, dq, dk, dv, lse, dsum ([B Tq, 8] each of the last two).  With M the form with the mask: dV = (P o M)^T dO,
    dP = M o (dO V^T); without, M = 1.  leak: dk of batch 1 lands in batch 0 (a planted error)."""
    q, k, v, dout = (t.to(dtype) for t in (q, k, v, dout))
    Q, K, V, G = (t.view(B, -1, 8, 8).transpose(1, 2) for t in (q, k, v, dout))
    S_ = Q @ K.transpose(-1, -2) * MHA_SCALE
    lse = torch.logsumexp(S_, -1)
    P = torch.exp(S_ - lse[..., None])
    PM = P if M is None else P * M.to(dtype)
    O = PM @ V
    dV = PM.transpose(-1, -2) @ G
    dP = G @ V.transpose(-1, -2)
    if M is not None:
        dP = dP * M.to(dtype)
    D = (G * O).sum(-1)
    dS = P * (dP - D[..., None])
    dQ, dK = dS @ K * MHA_SCALE, dS.transpose(-1, -2) @ Q * MHA_SCALE
    if leak and B > 1:
        dK = dK.clone()
        dK[0] += dK[1]
        dK[1] = 0
    rows = lambda t, T: t.transpose(1, 2).reshape(B * T, 64)
    # the size of the terms whose difference dq / dk are: with one key P = 1 and dP = D, so both gradients are zero by cancellation
    mag = P * (dP.abs() + D.abs()[..., None]) * MHA_SCALE
    cancel = dict(dq=float((mag @ K.abs()).max()), dk=float((mag.transpose(-1, -2) @ Q.abs()).max()))
    return dict(cancel=cancel, o=rows(O, Tq), dq=rows(dQ, Tq), dk=rows(dK, Tk), dv=rows(dV, Tk), lse=lse.transpose(1, 2).reshape(B * Tq, 8),
                dsum=D.transpose(1, 2).reshape(B * Tq, 8))


MHA_SHAPES = [(1, 1), (3, 2), (5, 4), (63, 65), (64, 64), (65, 63), (130, 257)]
MHA_CASES = [(Tq, Tk, dist, drop) for (Tq, Tk) in MHA_SHAPES for dist in ("uniform", "peaked") for drop in (False, True)]
MHA_B = 2
MHA_PEAK = 4.7              # q and k times this: the logits reach about +-40 (std 7), and some softmax rows are one-hot to fp32


def mha_case(Tq, Tk, dist, seed=460):
    """-> q, k, v, dout and the accumulate targets' earlier contents.  q | k | v are column blocks of one [rows, 192] buffer when
    Tq = Tk, else k | v of a [rows, 128] buffer."""
    B = MHA_B
    peak = MHA_PEAK if dist == "peaked" else 1.0
    if Tq == Tk:
        buf = rnd(B * Tq, 192, seed=seed)
        buf[:, 0:128] *= peak
        q, k, v = buf[:, 0:64], buf[:, 64:128], buf[:, 128:192]
    else:
        q, buf = rnd(B * Tq, 64, seed=seed) * peak, rnd(B * Tk, 128, seed=seed + 1)
        buf[:, 0:64] *= peak
        k, v = buf[:, 0:64], buf[:, 64:128]
    return dict(q=q, k=k, v=v, dout=rnd(B * Tq, 64, seed=seed + 2),
                old=dict(dq=rnd(B * Tq, 64, seed=seed + 3), dk=rnd(B * Tk, 64, seed=seed + 4), dv=rnd(B * Tk, 64, seed=seed + 5)))


# Peaked rows: the logits reach +-40, where one fp32 rounding of a logit (2^-24 x 40 = 2.4e-6) is a relative error of that size in its
# probability.  The fp32 CPU evaluation of this restatement still fits inside a quarter of the bars of the +-1 distribution on every
# case (tests/test_block_train_cpu.py asserts it), so the peaked distribution keeps them.
MHA_BARS = dict(dq=BAR_GRAD, dk=BAR_GRAD, dv=BAR_GRAD, lse=BAR_FWD, dsum=BAR_GRAD)


def check_mha_bwd(got, ref, scale=1.0):
    return _check(got, ref, MHA_BARS, scale, ref["cancel"])


# ------------------------------------------------------------------------------------------------------------------ single-row gradients
def seam_rows(rows, tile):
    """the last row of the first tile, the first of the next, the last valid row"""
    return sorted({tile - 1, tile, rows - 1})


def one_row(dout, row):
    z = torch.zeros_like(dout)
    z[row] = dout[row]
    return z


def others_zero(t, rows_kept):
    """True when every row of t outside rows_kept is exactly 0"""
    t = t.detach().cpu()
    keep = torch.zeros(t.shape[0], dtype=torch.bool)
    keep[list(rows_kept)] = True
    return bool((t[~keep] == 0).all())
