"""CPU tier of the geometric heads' loss kernels: the float64 restatement in loss_reference.py agrees with the oracle's focal_loss /
circle_loss evaluated in float64 and with their float64 autograd, and every condition that the GPU tier (tests/test_loss_gpu.py) relies
on is asserted HERE, on the GPU tier's own inputs: which branches a case reaches, that fp32 decides every mask pair, and that each bar is
four times what the oracle's formula in fp32 loses on those inputs."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_reference as lr
from oracle import cmr_oracle as O

F64, F32 = torch.float64, torch.float32
FWD_ALL = [(c, "product") for c in lr.CIRCLE_FWD_CASES] + [(c, "other") for c in lr.CIRCLE_FWD_OTHER]
BWD_ALL = ([(c + (None,), "product") for c in lr.CIRCLE_BWD_CASES] + [(c + (None,), "other") for c in lr.CIRCLE_BWD_OTHER] +
           [(c, "product") for c in lr.CIRCLE_BWD_SPECIAL])
PARAMS = {"product": lr.PRODUCT_PARAMS, "other": lr.OTHER_PARAMS}
_id = lambda v: "-".join(str(x) for x in v[0]) + "-" + v[1]


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules switch autograd off process-wide at import (torch.set_grad_enabled(False)); the oracle's autograd needs it"""
    with torch.enable_grad():
        yield


@functools.lru_cache(maxsize=None)
def _fwd(case, pname, dtype=F64):
    r = lr.circle_forward(lr.circle_case(*case), PARAMS[pname], dtype)
    r.pop("parts")
    return r


@functools.lru_cache(maxsize=None)
def _bwd(case, pname):
    r = lr.circle_backward(lr.circle_case(*case), PARAMS[pname], lr.bwd_grad_scale(case[0], case[1]))
    r["fwd"].pop("parts")
    return r


def _oracle_circle(c, P, dtype, grad):
    """the oracle's circle_loss on the case's sampled features (dense leaves, so that autograd scatters as the kernels do)"""
    B, N = c["B"], c["N"]
    pc = c["pc"].to(dtype).view(B, N, 64).clone().requires_grad_(grad)
    img = c["img"].to(dtype).clone().requires_grad_(grad)
    bi = torch.arange(B)[:, None]
    pts = pc[bi, c["pc_idx"]].permute(0, 2, 1)                                       # [B, 64, n]
    pix = img[bi, c["xy_int"][:, 1], c["xy_int"][:, 0]].permute(0, 2, 1)
    dmap = torch.sqrt(torch.sum(torch.square(c["xy_float"].to(dtype).unsqueeze(-1) - c["xy_int"].to(dtype).unsqueeze(-2)), dim=1))
    loss = O.circle_loss(pix, pts, dmap, lr.f32(P["dist_thres"]), lr.f32(P["pos_margin"]), lr.f32(P["neg_margin"]), lr.f32(P["log_scale"]))
    if grad:
        loss.backward()
        return loss.detach(), pc.grad.reshape(B * N, 64), img.grad
    return loss.detach()


# ---- focal ---------------------------------------------------------------------------------------------------------------------------------
def _focal_inputs():
    z, lab = lr.focal_sweep()
    yield "sweep", z, lab, 1
    for rows, B in lr.FOCAL_SHAPES:
        yield "rows%d" % rows, *lr.focal_rows(rows), B
    for name in lr.FOCAL_METRIC_CASES:
        yield name, *lr.focal_metric_case(name), 1
    z, lab = lr.focal_rows(257)
    yield "rows257_all_labelled", z, torch.ones_like(lab), 1                           # what the label-rule test runs


@pytest.mark.parametrize("alpha", lr.FOCAL_ALPHAS)
def test_focal_reference_is_the_oracle_in_float64(alpha):
    for name, z, lab, _ in _focal_inputs():
        r = lr.focal(z, lab, alpha)
        zz = z.double().requires_grad_(True)
        want = O.focal_loss(zz, lab, alpha)
        want.backward()
        assert abs(float(r["mean"]) - float(want.detach())) <= 1e-14 * abs(float(want.detach())), name
        scale = alpha / z.shape[0]
        assert lr.scaled_err(r["grad_autograd"], zz.grad, scale) <= 1e-13, name
        assert lr.scaled_err(r["grad"], zz.grad, scale) <= 1e-12, name                # closed form: (1 - s)^2 / s at s = 1e-6 amplifies
    z, lab = lr.focal_sweep()
    r = lr.focal(z, lab, alpha)
    for i in range(z.shape[0]):                                                     # per row: the oracle on that row alone
        want = float(O.focal_loss(z[i:i + 1].double(), lab[i:i + 1], alpha))
        assert abs(float(r["row"][i]) - want) <= 1e-14 * abs(want)
    # the same statement in fp32 is the oracle's fp32 value (the yardstick of the bars)
    want = float(O.focal_loss(z, lab, alpha))
    assert abs(float(lr.focal(z, lab, alpha, F32)["mean"]) - want) <= 2e-7 * want


def test_focal_labels_other_than_0_and_1_read_as_class_1():
    z, lab = lr.focal_rows(257)
    one = lr.focal(z, torch.ones_like(lab), 0.75)
    for v in (2, -1):
        r = lr.focal(z, torch.full_like(lab, v), 0.75)
        assert torch.equal(r["row"], one["row"]) and torch.equal(r["grad"], one["grad"]) and r["counts"] == one["counts"]


def test_focal_sweep_reaches_what_the_gpu_tier_says_it_reaches():
    z, lab = lr.focal_sweep()
    assert z.shape == (len(lr.FOCAL_BASES) * len(lr.FOCAL_DIFFS) * 4, 2)
    p = torch.softmax(z, dim=1)                                                     # fp32
    assert (p == 0).any() and (p == 1).any(), "softmax saturates to exactly 0 and 1 in fp32"
    assert (p + 1e-6 == np.float32(1e-6)).any(), "s = 1e-6: logf(1e-6)"
    assert (z[:, 0] == z[:, 1]).any() and ((z[:, 0] == z[:, 1]) & (lab == 1)).any(), "ties, with either label"
    for alpha in lr.FOCAL_ALPHAS:
        row = lr.focal(z, lab, alpha)["row"]
        # the per-row relative comparison has something to be relative to: the +1e-6 on the one-hot keeps every row above ~4e-6 alpha
        assert float(row.min()) > 3e-6 * alpha
        # true gradients underflow on saturated rows: a per-row relative gradient comparison is not usable, alpha / rows is the scale
        g = lr.focal(z, lab, alpha)["grad"]
        assert float(g.abs().max(1).values.min()) < 1e-20
    # shift invariance: the same differences at every base give the same float64 rows to ~1 ulp of the base
    n = len(lr.FOCAL_DIFFS) * 4
    row = lr.focal(z, lab, 0.75)["row"]
    exact = (z[:, 1].double() - z[:, 0].double()).view(3, n)
    same = (exact[0] == exact[1]) & (exact[0] == exact[2])                           # 1e-3 does not survive the addition to 37.5 in fp32
    assert same.sum() >= n - 4 and torch.allclose(row.view(3, n)[1][same], row.view(3, n)[0][same], rtol=1e-9, atol=0)


def test_focal_metric_cases_are_what_their_names_say():
    got = {}
    for name in lr.FOCAL_METRIC_CASES:
        z, lab = lr.focal_metric_case(name)
        r = lr.focal(z, lab, 0.5)
        got[name] = (r["counts"], lr.focal_metrics(r["counts"], z.shape[0], 1))
    (tp, pp, lp, ok), (prec, rec, acc) = got["none_predicted"]
    assert pp == 0 and tp == 0 and lp > 0 and np.isnan(prec) and rec == 0
    (tp, pp, lp, ok), (prec, rec, acc) = got["none_labelled"]
    assert lp == 0 and pp > 0 and np.isnan(rec) and prec == 0
    (tp, pp, lp, ok), (prec, rec, acc) = got["all_right"]
    assert ok == 257 and tp == pp == lp > 0 and prec == rec == acc == 1
    (tp, pp, lp, ok), (prec, rec, acc) = got["ties"]
    assert pp == 0 and lp > 0 and ok == 257 - lp and np.isnan(prec), "a tie predicts class 0"
    for rows, B in lr.FOCAL_SHAPES:
        z, lab = lr.focal_rows(rows)
        c = lr.focal(z, lab, 0.75)["counts"]
        assert rows < 2 ** 24 and rows % B == 0 and (rows == 1 or (0 < c[0] < c[1] < rows and c[0] < c[2]))
        if rows > 8:
            assert (z[:, 0] == z[:, 1]).any()
    assert max(r for r, _ in lr.FOCAL_SHAPES) > 512 * 256, "the forward's grid-stride loop takes a second trip"


# ---- circle --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,pname", FWD_ALL, ids=map(_id, FWD_ALL))
def test_circle_forward_reference_is_the_oracle_in_float64(case, pname):
    c, r = lr.circle_case(*case), _fwd(case, pname)
    lam = lr.f32(PARAMS[pname]["lam"])
    want = float(_oracle_circle(c, PARAMS[pname], F64, False))
    assert abs(float(r["loss"]) - lam * want) <= 1e-13 * abs(want)
    assert r["terms"].shape == (c["B"], 2 * c["n"]) and float(r["terms"].min()) > 0
    # ... and in fp32 it is the oracle's fp32 value
    assert abs(float(_fwd(case, pname, F32)["loss"]) - lam * float(_oracle_circle(c, PARAMS[pname], F32, False))) <= 1e-6 * abs(want)


@pytest.mark.parametrize("case,pname", BWD_ALL, ids=map(_id, BWD_ALL))
def test_circle_closed_form_gradient_is_autograd_in_float64(case, pname):
    c, r = lr.circle_case(*case), _bwd(case, pname)
    gs = lr.f32(lr.bwd_grad_scale(case[0], case[1]))
    for k in ("d_pc", "d_img"):
        assert float(r[k].abs().max()) > 0, "a case whose gradient vanishes measures nothing"
    # autograd of the same loss with the d = 0 pairs' distance detached
    a = lr.circle_forward(c, PARAMS[pname], F64, grad=True, grad_scale=lr.bwd_grad_scale(case[0], case[1]))
    for k in ("d_pc", "d_img"):
        assert lr.scaled_err(r[k], a[k], float(a[k].abs().max())) <= 1e-12
    loss, d_pc, d_img = _oracle_circle(c, PARAMS[pname], F64, True)
    if not bool(r["fwd"]["zero"].any()):
        assert lr.scaled_err(r["d_pc"], gs * d_pc, float(r["d_pc"].abs().max())) <= 1e-12
        assert lr.scaled_err(r["d_img"], gs * d_img.view_as(r["d_img"]), float(r["d_img"].abs().max())) <= 1e-12
    else:                                                                          # why the closed form: the oracle's autograd is NaN here
        assert torch.isnan(d_pc).any() and torch.isnan(d_img).any()
        assert torch.isfinite(r["d_pc"]).all() and torch.isfinite(r["d_img"]).all()
    # rows that no sample names receive nothing
    assert (r["d_pc"][~r["named_pc"]] == 0).all() and (r["d_img"][~r["named_img"]] == 0).all()
    assert (~r["named_pc"]).any() or case[0] > 64


@pytest.mark.parametrize("case,pname", FWD_ALL + BWD_ALL, ids=map(_id, FWD_ALL + BWD_ALL))
def test_circle_cases_reach_what_the_gpu_tier_says_they_reach(case, pname):
    c = lr.circle_case(*case)
    r = _fwd(case[:4], pname) if len(case) == 4 or case[4] is None else _bwd(case, pname)["fwd"]
    n, B, feat, mask = case[:4]
    special = case[4] if len(case) > 4 else None
    h, w, N = c["h"], c["w"], c["N"]
    assert h != w and N == 40 and h * w <= 54
    # fp32 decides every mask pair: quarter-pixel offsets, so a pair is exactly on the threshold or well away from it
    assert torch.equal(c["xy_float"] * 4, (c["xy_float"] * 4).round())
    assert r["gap"] >= (0.03 if pname == "product" else 0.015)
    m = r["mask"]
    d = r["d"]
    if mask == "sparse" and n >= 2:
        x, y = c["xy_int"][:, 0], c["xy_int"][:, 1]
        assert ((x == 0) & (y == 0)).any() and ((x == w - 1) & (y == h - 1)).any()       # both corners
    if n >= 2:
        assert (c["pc_idx"] == 0).any() and (c["pc_idx"] == N - 1).any()                  # first and last point
    if n > 54:
        assert any(len(set(c["pc_idx"][b].tolist())) < n for b in range(B))               # indices repeat
    if mask == "sparse" and n >= 5:
        assert (~m.any(2)).any() and (~m.any(1)).any(), "a row and a column without a positive"
    if mask == "dense":
        assert m.all(2).any() and m.all(1).any(), "a row and a column of positives only"
        assert n < 15 or not m.all()
    if n >= 15:
        assert r["on_thres"] > 0
    if mask == "sparse" and n >= 65:
        dx = c["xy_float"][:, 0, :, None] - c["xy_int"][:, 0, None, :].float()
        dy = c["xy_float"][:, 1, :, None] - c["xy_int"][:, 1, None, :].float()
        for ox, oy, positive in ((1, 0, True), (-1, 0, True), (0, 1, True), (0, -1, True), (1, 0.25, pname == "other")):
            at = (dx == ox) & (dy == oy)
            assert at.any() and bool((m[at] == positive).all()), (ox, oy)
    if pname == "product":
        if feat == "prototype":
            assert float(r["arg"].max()) > 20, "softplus takes its x > 20 branch"
            assert set((d * d).round().reshape(-1).tolist()) <= {0.0, 2.0, 4.0} and float((d * d - (d * d).round()).abs().max()) < 1e-15
            if n >= 15:
                assert (d[m] == 2).any() and (d[~m] == 0).any(), "positives at d = 2, negatives at d = 0"
        if feat == "trained" and special != "dzero":                                 # (a copied feature makes a negative at d = 0)
            assert float(r["arg"].max()) < 20, "softplus stays on its log1p(exp) branch"
            if n >= 15:
                assert float(d[m].min()) < 0.15, "a point sits on its pixel's feature"
    if special == "repeat":
        assert n == 130
        for b in range(B):
            key = (c["xy_int"][b, 1] * w + c["xy_int"][b, 0]).tolist()
            assert all(key[k] == key[0] for k in (3, 70, 129)), "one pixel at samples 0, 3, 70, 129: > 64 apart, three ballots"
            p = c["pc_idx"][b].tolist()
            assert p[1] == p[2] == p[100], "one point across the k = 64 boundary"
    if special == "dzero":
        assert bool(r["zero"][:, 3, 5].all()) and all(
            torch.equal(c["pc"][b * N + c["pc_idx"][b, 3]], c["img"][b, c["xy_int"][b, 1, 5], c["xy_int"][b, 0, 5]]) for b in range(B))
    elif feat != "prototype":
        assert not bool(r["zero"].any())


def test_circle_case_lists_cover_the_loop_structures():
    fwd_n = {c[0] for c in lr.CIRCLE_FWD_CASES}
    assert fwd_n == {1, 3, 15, 16, 17, 65, 257, 512} and {c[1] for c in lr.CIRCLE_FWD_CASES} == {1, 3}
    assert {(c[0], c[1]) for c in lr.CIRCLE_FWD_CASES if c[0] == 512} == {(512, 1)}
    bwd_n = {c[0] for c in lr.CIRCLE_BWD_CASES}
    assert bwd_n == {1, 7, 8, 9, 64, 65, 130} and {c[1] for c in lr.CIRCLE_BWD_CASES} == {1, 2}
    for cases in (lr.CIRCLE_FWD_CASES, lr.CIRCLE_BWD_CASES):
        assert {(c[2], c[3]) for c in cases} == {(f, m) for f in lr.FEATS for m in lr.MASKS}
        assert len(set(cases)) == len(cases)
    assert {lr.bwd_grad_scale(c[0], c[1]) for c in lr.CIRCLE_BWD_CASES} == {1.0, 0.37}
    assert lr.PRODUCT_PARAMS == dict(dist_thres=1.0, pos_margin=0.1, neg_margin=1.4, log_scale=10.0, lam=1.0)
    assert all(lr.OTHER_PARAMS[k] != lr.PRODUCT_PARAMS[k] for k in lr.PRODUCT_PARAMS)


# ---- l2norm --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", lr.L2NORM_ROWS)
def test_l2norm_reference_is_normalize_in_float64(rows):
    x, dy = lr.l2norm_case(rows)
    r = lr.l2norm(x, dy)
    xx = x.double().requires_grad_(True)
    y = F.normalize(xx, dim=1, eps=1e-12)
    y.backward(dy.double())
    assert torch.equal(r["y"], y.detach()) and torch.equal(r["dx_autograd"], xx.grad)
    assert lr.scaled_err(r["dx"], xx.grad, r["scale"][:, None]) <= 1e-13
    nrm = x.double().norm(dim=1)
    if rows > 7:
        assert nrm[7] == 0 and (r["y"][7] == 0).all() and torch.equal(r["dx"][7], dy[7].double() / 1e-12) and torch.isfinite(r["dx"]).all()
        assert float(nrm[nrm > 0].min()) < 2e-6 and float(nrm.max()) > 5e5
    assert ((nrm == 0) | (nrm > 1e-7)).all(), "no row in the clamped range 0 < |x| < eps"


# ---- the bars ------------------------------------------------------------------------------------------------------------------------------
def fp32_oracle_errors():
    """the oracle's formulas in fp32 on the CPU against the float64 reference: per bar, the largest error in the GPU test's metric over
    the GPU test's inputs"""
    e = dict.fromkeys(lr.CAPS, 0.0)
    up = lambda k, v: e.__setitem__(k, max(e[k], v))
    z, lab = lr.focal_sweep()
    for alpha in lr.FOCAL_ALPHAS:
        ref = lr.focal(z, lab, alpha)
        for i in range(z.shape[0]):                                                 # rows = 1 launches: each row is its own mean
            up("FOCAL_ROW_BAR", lr.rel_err(lr.focal(z[i:i + 1], lab[i:i + 1], alpha, F32)["mean"], ref["row"][i]))
        for name, zz, ll, _ in _focal_inputs():
            r64, r32 = lr.focal(zz, ll, alpha), lr.focal(zz, ll, alpha, F32)
            if name != "sweep":                                                     # a launch of one row is held to the row bar
                up("FOCAL_ROW_BAR" if zz.shape[0] == 1 else "FOCAL_MEAN_BAR", lr.rel_err(r32["mean"], r64["mean"]))
            if name in ["sweep", "rows257_all_labelled"] + ["rows%d" % r for r in lr.FOCAL_BWD_ROWS]:
                up("FOCAL_GRAD_BAR", lr.scaled_err(r32["grad_autograd"], r64["grad"], alpha / zz.shape[0]))
    for case, pname in FWD_ALL:
        r64, r32 = _fwd(case, pname), _fwd(case, pname, F32)
        up("CIRCLE_TERM_BAR", lr.rel_err(r32["terms"], r64["terms"]))
        up("CIRCLE_LOSS_BAR", lr.rel_err(r32["loss"], r64["loss"]))
    for case, pname in BWD_ALL:
        c, ref = lr.circle_case(*case), _bwd(case, pname)
        r32 = lr.circle_forward(c, PARAMS[pname], F32, grad=True, grad_scale=lr.bwd_grad_scale(case[0], case[1]))
        pre = lr.circle_prefill(c, ref)
        up("CIRCLE_GRAD_BAR", lr.circle_grad_err(pre[0] + r32["d_pc"], pre[0], ref["d_pc"]))
        up("CIRCLE_GRAD_BAR", lr.circle_grad_err(pre[1] + r32["d_img"], pre[1], ref["d_img"]))
    for rows in lr.L2NORM_ROWS:
        x, dy = lr.l2norm_case(rows)
        r64, r32 = lr.l2norm(x, dy), lr.l2norm(x, dy, F32)
        up("L2NORM_FWD_BAR", lr.scaled_err(r32["y"], r64["y"], 1.0))
        up("L2NORM_BWD_BAR", lr.scaled_err(r32["dx_autograd"], r64["dx"], r64["scale"][:, None]))
        pre = lr.prefill((rows, 64), 1.0, 77 + rows) * r64["scale"].float()[:, None]
        up("L2NORM_BWD_BAR", lr.scaled_err(pre + r32["dx_autograd"], pre.double() + r64["dx"], r64["scale"][:, None]))
    return e


def test_fp32_oracle_stays_within_a_quarter_of_every_bar():
    e = fp32_oracle_errors()
    for k, cap in lr.CAPS.items():
        bar = getattr(lr, k)
        print("%-16s fp32 oracle %.3g   bar %.3g   cap %.3g" % (k, e[k], bar, cap))
        assert 0 < e[k] <= bar / 4, "%s: the fp32 oracle is off by %.3g, the bar is %.3g" % (k, e[k], bar)
        assert bar <= cap, k
