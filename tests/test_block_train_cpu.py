"""CPU tier of tests/test_block_train_ops_gpu.py: the float64 restatements of tests/block_train_reference.py are right (every hand-written
backward equals float64 autograd of its forward restatement), the mask restatement has the statistics of a dropout mask, fp32 evaluation
of the same formulas fits inside every bar divided by 4 on every case the GPU tier runs, and every comparison rejects a planted error."""
import copy

import numpy as np
import pytest
import torch

import block_train_reference as R

f32, f64 = torch.float32, torch.float64
AUTOGRAD_RTOL = 1e-12


@pytest.fixture(autouse=True)
def _grad_on():
    """other test modules switch autograd off process-wide at import (torch.set_grad_enabled(False)); the agreement tests need it"""
    with torch.enable_grad():
        yield


def _agree(got, want, name):
    e = R.rel_err(got, want)
    assert e <= AUTOGRAD_RTOL, "%s: %.3e" % (name, e)


def _leaf(t):
    return t.detach().double().clone().requires_grad_(True)


# ------------------------------------------------------------------------------------------------------- backward == autograd of forward
@pytest.mark.parametrize("drop", [False, True])
def test_vit_ffn_bwd_is_autograd_of_the_tail(drop):
    w, ctx, x, dout, d = R.vit_case(37, drop, True)
    wl = {k: (_leaf(v) if torch.is_tensor(v) else v) for k, v in w.items()}
    ctxl, xl = _leaf(ctx), _leaf(x)
    r = R.vit_tail(wl, ctxl, xl, d)
    for k in ("x1", "u", "proj", "y"):
        r[k].retain_grad()
    r["out"].backward(dout.double())
    b = R.vit_ffn_bwd(w, r["x1"].detach(), dout, d)
    _agree(b["dx1"], r["x1"].grad, "dx1")
    _agree(b["dx1"], xl.grad, "dx (the residual stream)")
    _agree(b["dctx"], ctxl.grad, "dctx")
    _agree(b["du"], r["u"].grad, "du")
    _agree(b["dm"], r["y"].grad, "dm")
    _agree(b["da"], r["proj"].grad, "da")
    _agree(b["gs"], r["gs"].detach(), "gs")
    _agree(b["h"], r["h"].detach(), "h")
    _agree(b["ln_g"], wl["g2"].grad, "d gamma")
    _agree(b["ln_b"], wl["b2n"].grad, "d beta")
    # the operands give the weight gradients
    _agree(b["dm"].T @ b["gs"], wl["w2"].grad, "dW2")
    _agree(b["du"].T @ b["h"], wl["w1"].grad, "dW1")
    _agree(b["da"].T @ ctx.double(), wl["wo"].grad, "dWo")
    _agree(b["term_g"].sum(0), b["ln_g"], "per-row terms")


@pytest.mark.parametrize("case", [(33, 64, False, 0, 0), (33, 192, True, 0, 0), (77, 64, True, 50, 128)])
def test_lnqkv_bwd_is_autograd(case):
    w, px, py = R.lnqkv_case(*case)
    wl = {k: (_leaf(v) if torch.is_tensor(v) else v) for k, v in w.items()}
    loss, leaves = 0.0, {}
    for tag, pr in (("x", px), ("y", py)):
        if pr is None:
            continue
        xl = _leaf(pr["x"])
        leaves[tag] = xl
        xn, _, _ = R.ln_fwd(xl, wl["g"], wl["b"], wl["eps"])
        loss = loss + ((xn @ wl["wcat"][pr["lo"]:pr["hi"]].T) * pr["d"].double()).sum()
        if pr.get("res") is not None:
            loss = loss + (xl * pr["res"].double()).sum()
    loss.backward()
    b = R.lnqkv_bwd(w, px, py)
    _agree(b["dx"], leaves["x"].grad, "dx")
    if py is not None:
        _agree(b["dy"], leaves["y"].grad, "dy")
    _agree(b["ln_g"], wl["g"].grad, "d gamma")
    _agree(b["ln_b"], wl["b"].grad, "d beta")


@pytest.mark.parametrize("drop", [False, True])
def test_la_mlp_bwd_is_autograd(drop):
    rows = 45
    w = R.la_weights()
    d = R.la_drop(drop)
    wl = {k: _leaf(v) for k, v in w.items()}
    xl, ml = _leaf(R.rnd(rows, 64, seed=1)), _leaf(R.rnd(rows, 64, seed=2))
    dout = R.rnd(rows, 64, seed=3)
    r = R.la_mlp_fwd(wl, xl, ml, d)
    for k in ("mm", "hid_pre", "o_pre"):
        r[k].retain_grad()
    r["y2"].backward(dout.double())
    b = R.la_mlp_bwd(w, {k: r[k].detach() for k in ("o", "hid", "mm")}, dout, d)
    _agree(b["d_o"], r["o_pre"].grad, "d_o")
    _agree(b["d_hid"], r["hid_pre"].grad, "d_hid")
    _agree(b["d_mm"], r["mm"].grad, "d_mm")
    _agree(b["d_msg"], ml.grad, "d_msg")
    _agree(b["d_xa"], xl.grad, "d_xa")
    for n, key in (("g1", "ln1_g"), ("b1", "ln1_b"), ("g2", "ln2_g"), ("b2", "ln2_b")):
        _agree(b[key], wl[n].grad, key)


@pytest.mark.parametrize("form", ["self", "cross"])
def test_la_proj_bwd_is_autograd(form):
    """f = elu(x W^T) + 1 recomputed from x; the derivative from the SAVED f alone: 1 where f > 1, else f (= exp z)"""
    rows_x, rows_y = 33, 21
    w = R.la_weights()
    x, y = _leaf(R.rnd(rows_x, 64, seed=5)), _leaf(R.rnd(rows_y, 64, seed=6))
    src = x if form == "self" else y
    rs = src.shape[0]
    dq, dk, dv = R.rnd(rows_x, 64, seed=7), R.rnd(rs, 64, seed=8), R.rnd(rs, 64, seed=9)
    r0, r1 = R.rnd(rows_x, 64, seed=10), R.rnd(rows_x, 64, seed=11)
    W = {k: w[k].double() for k in ("wq", "wk", "wv")}
    qf, kf, v = R.elu1(x @ W["wq"].T), R.elu1(src @ W["wk"].T), src @ W["wv"].T
    ((qf * dq).sum() + (kf * dk).sum() + (v * dv).sum() + (x * (r0 + r1).double()).sum()).backward()
    tq, tk, tv = (dq, qf.detach(), "wq"), (dk, kf.detach(), "wk"), (dv, None, "wv")
    if form == "self":
        out = R.la_proj_bwd(w, [dict(rows=rows_x, terms=[tq, tk, tv], res=[r0, r1])])
        _agree(out[0]["dx"], x.grad, "dx")
    else:
        out = R.la_proj_bwd(w, [dict(rows=rows_x, terms=[tq], res=[r0, r1]), dict(rows=rows_y, terms=[tk, tv], res=[])])
        _agree(out[0]["dx"], x.grad, "dx")
        _agree(out[1]["dx"], y.grad, "dy")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dist", ["uniform", "peaked"])
def test_mha_bwd_is_autograd(masked, dist):
    Tq, Tk, B = 13, 9, R.MHA_B
    c = R.mha_case(Tq, Tk, dist)
    M = R.mha_mask(B, Tq, Tk, masked)
    q, k, v = _leaf(c["q"]), _leaf(c["k"]), _leaf(c["v"])
    o = R.mha_fwd(q, k, v, B, Tq, Tk, M)
    o.backward(c["dout"].double())
    b = R.mha_bwd(c["q"], c["k"], c["v"], c["dout"], B, Tq, Tk, M)
    for key, want in (("o", o.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        _agree(b[key], want, key)


def test_la_bwd_is_autograd():
    L, S, B = 15, 17, R.LA_BWD_B
    c = R.la_bwd_case(L, S)
    qf, kf, v = _leaf(c["qf"]), _leaf(c["kf"]), _leaf(c["v"])
    msg, kvsum = R.la_core(qf, kf, v, B, L, S, R.LA_EPS)
    msg.backward(c["dmsg"].double())
    b = R.la_bwd(c["qf"], c["kf"], c["v"], kvsum.detach(), c["dmsg"], B, L, S, R.LA_EPS)
    for key, want in (("dqf", qf.grad), ("dkf", kf.grad), ("dv", v.grad)):
        _agree(b[key], want, key)


def test_forward_restatements_agree_with_torch_modules():
    """the hand-written LayerNorm / GELU / elu + 1 against torch.nn.functional"""
    import torch.nn.functional as F
    x, g, b = R.rnd(9, 64, seed=1).double(), R.rnd(64, seed=2).double(), R.rnd(64, seed=3).double()
    _agree(R.ln_fwd(x, g, b, 1e-5)[0], F.layer_norm(x, (64,), g, b, 1e-5), "layer norm")
    _agree(R.gelu(3 * x), F.gelu(3 * x), "gelu")
    _agree(R.elu1(3 * x), F.elu(3 * x) + 1, "elu + 1")
    assert R.rel_err(R.elu1(3 * x, exp2=True), F.elu(3 * x) + 1) < 1e-15


# ---------------------------------------------------------------------------------------------------------------------------------- mask
def test_keep_mask_properties():
    n = 20000 * 64
    for p in (0.1, 0.5):
        m = R.keep_mask(7, 3, n, p)
        assert abs(float(m.mean()) - (1 - p)) < 4e-3                                     # the bound of test_dropout_gpu.py
        assert not np.array_equal(m, R.keep_mask(7, 4, n, p))                            # other site
        assert not np.array_equal(m, R.keep_mask(8, 3, n, p))                            # other seed
        both = m & R.keep_mask(8, 3, n, p)
        assert abs(float(both.mean()) - (1 - p) ** 2) < 6e-3
        assert np.array_equal(m, R.keep_mask(7, 3, n, p))
        assert np.array_equal(m[:1000], R.keep_mask(7, 3, 1000, p))                      # a function of the element index alone
    assert R.keep_mask(7, 3, 4096, 0.0).all()                                            # p = 0 keeps everything
    assert R.drop_threshold(0.0) == 0 and R.drop_threshold(0.5) == 1 << 31
    assert R.drop_threshold(0.1) == int(float(np.float32(0.1)) * 2 ** 32)                # p is an fp32 argument
    assert R.keep_scale(0.5) == 2.0
    # negative seeds are their two's complement
    assert np.array_equal(R.keep_mask(-1, 0, 64, 0.3), R.keep_mask(2 ** 64 - 1, 0, 64, 0.3))


# ------------------------------------------------------------------------------------------------ fp32 evaluation inside bar / 4, per case
Q = 1.0 / R.FP32_MARGIN


def _f(t):
    return None if t is None else t.float()


@pytest.mark.parametrize("rows,drop,strided", R.VIT_CASES)
def test_vit_fp32_fits(rows, drop, strided):
    w, ctx, x, dout, d = R.vit_case(rows, drop, strided)
    ref = R.vit_tail(w, ctx, x, d)
    got = R.vit_tail(w, ctx, x, d, dtype=f32)
    print(R.check_vit_fwd(got, ref, Q))
    x1 = ref["x1"].float()                                 # what the forward kernel hands the backward
    print(R.check_vit_ffn_bwd(R.vit_ffn_bwd(w, x1, dout, d, dtype=f32), R.vit_ffn_bwd(w, x1, dout, d), Q))


@pytest.mark.parametrize("case", R.LNQKV_CASES)
def test_lnqkv_fp32_fits(case):
    w, px, py = R.lnqkv_case(*case)
    print(R.check_lnqkv_bwd(R.lnqkv_bwd(w, px, py, dtype=f32), R.lnqkv_bwd(w, px, py), Q))


@pytest.mark.parametrize("B,S,strided", R.LA_KV_CASES)
def test_la_kv_state_fp32_fits(B, S, strided):
    """kf through exp2(v log2 e) in fp32, as the kernel evaluates it"""
    w, y = R.la_kv_case(B, S, strided)
    print(R.check_la_kv_state(R.la_kv_state(w, y, B, S, dtype=f32, exp2=True), R.la_kv_state(w, y, B, S), Q))


@pytest.mark.parametrize("B,L,drop", R.LA_QUERY_CASES)
def test_la_query_fp32_fits_and_band_is_small(B, L, drop):
    w, x, kvsum, S = R.la_query_case(B, L)
    d = R.la_drop(drop)
    ref = R.la_query_layer(w, x, kvsum, B, L, S, d)
    print(R.check_la_query(R.la_query_layer(w, x, kvsum, B, L, S, d, dtype=f32, exp2=True), ref, Q))


@pytest.mark.parametrize("rows,drop", R.LA_MLP_CASES)
def test_la_mlp_bwd_fp32_fits(rows, drop):
    w, sv, dout, d = R.la_mlp_case(rows, drop)
    print(R.check_la_mlp_bwd(R.la_mlp_bwd(w, sv, dout, d, dtype=f32), R.la_mlp_bwd(w, sv, dout, d), Q))


@pytest.mark.parametrize("form,rows_x,rows_y", R.LA_PROJ_CASES)
def test_la_proj_bwd_fp32_fits(form, rows_x, rows_y):
    w, probs = R.la_proj_case(form, rows_x, rows_y)
    print(R.check_la_proj_bwd(R.la_proj_bwd(w, probs, dtype=f32), R.la_proj_bwd(w, probs), Q))


@pytest.mark.parametrize("Tq,Tk,dist,drop", R.MHA_CASES)
def test_mha_bwd_fp32_fits(Tq, Tk, dist, drop):
    c = R.mha_case(Tq, Tk, dist)
    M = R.mha_mask(R.MHA_B, Tq, Tk, drop)
    a = (c["q"], c["k"], c["v"], c["dout"], R.MHA_B, Tq, Tk, M)
    print(R.check_mha_bwd(R.mha_bwd(*a, dtype=f32), R.mha_bwd(*a), Q))


def test_mha_peaked_rows_are_peaked():
    """the peaked distribution does what it is for: logits near +-40, rows that are one-hot to fp32"""
    onehot, top = 0, 0.0
    for Tq, Tk in R.MHA_SHAPES:
        c = R.mha_case(Tq, Tk, "peaked")
        Qh, Kh = (t.double().view(R.MHA_B, -1, 8, 8).transpose(1, 2) for t in (c["q"], c["k"]))
        S_ = Qh @ Kh.transpose(-1, -2) * R.MHA_SCALE
        top = max(top, float(S_.abs().max()))
        if Tk > 1:
            onehot += int((torch.softmax(S_, -1).float().max(-1).values == 1.0).sum())
    print("largest logit %.1f, %d one-hot rows" % (top, onehot))
    assert 35 < top < 45 and onehot > 0


@pytest.mark.parametrize("L,S", R.LA_BWD_CASES)
def test_la_bwd_fp32_fits(L, S):
    c = R.la_bwd_case(L, S)
    _, kvsum = R.la_core(c["qf"].double(), c["kf"].double(), c["v"].double(), R.LA_BWD_B, L, S, R.LA_EPS)
    a = (c["qf"], c["kf"], c["v"], kvsum.float(), c["dmsg"], R.LA_BWD_B, L, S, R.LA_EPS)
    print(R.check_la_bwd(R.la_bwd(*a, dtype=f32), R.la_bwd(*a), Q))


# ------------------------------------------------------------------------------------------------------- single-row gradients, restated
def test_single_row_gradients_are_zero_elsewhere_in_the_restatement():
    w, ctx, x, dout, d = R.vit_case(40, True, False)
    x1 = R.vit_tail(w, ctx, x, d)["x1"]
    for row in R.seam_rows(40, 16):
        b = R.vit_ffn_bwd(w, x1, R.one_row(dout, row), d)
        for key in ("dx1", "dctx", "du", "dm", "da"):
            assert R.others_zero(b[key], [row]), key
        assert R.rel_err(b["ln_g"], b["term_g"][row]) < 1e-14
    c = R.mha_case(5, 4, "uniform")
    g = R.one_row(c["dout"], 3)                                # a query of batch element 0
    b = R.mha_bwd(c["q"], c["k"], c["v"], g, R.MHA_B, 5, 4)
    assert R.others_zero(b["dq"], [3]) and R.others_zero(b["dk"], range(4)) and R.others_zero(b["dv"], range(4))


# --------------------------------------------------------------------------------------------------------------------- planted errors
def _rejects(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def _row0_into_last(ref, keys):
    got = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ref.items()}
    for k in keys:
        got[k][-1] = got[k][0]
    return got


def test_planted_last_row_of_a_partial_tile_is_row_0():
    w, ctx, x, dout, d = R.vit_case(270, True, True)
    ref = R.vit_tail(w, ctx, x, d)
    for k in R.VIT_FWD_BARS:
        _rejects(R.check_vit_fwd, _row0_into_last(ref, [k]), ref)
    refb = R.vit_ffn_bwd(w, ref["x1"], dout, d)
    for k in ("dx1", "dctx", "gs", "du", "h", "dm", "da"):
        _rejects(R.check_vit_ffn_bwd, _row0_into_last(refb, [k]), refb)
    w, px, py = R.lnqkv_case(77, 64, True, 50, 128)
    refl = R.lnqkv_bwd(w, px, py)
    for k in ("dx", "xn", "dy", "yn"):
        _rejects(R.check_lnqkv_bwd, _row0_into_last(refl, [k]), refl)
    w, sv, dout, d = R.la_mlp_case(8 * 32 + 1, True)
    refm = R.la_mlp_bwd(w, sv, dout, d)
    for k in ("d_o", "d_hid", "d_mm", "d_msg", "d_xa"):
        _rejects(R.check_la_mlp_bwd, _row0_into_last(refm, [k]), refm)
    w, x, kvsum, S = R.la_query_case(3, 33)
    refq = R.la_query_layer(w, x, kvsum, 3, 33, S, R.la_drop(True))
    for k in R.LA_QUERY_BARS:
        _rejects(R.check_la_query, _row0_into_last(refq, [k]), refq)
    w, probs = R.la_proj_case("self", 77, 0)
    refp = R.la_proj_bwd(w, probs)
    bad = copy.deepcopy(refp)
    bad[0]["dx"][-1] = bad[0]["dx"][0]
    _rejects(R.check_la_proj_bwd, bad, refp)
    bad = copy.deepcopy(refp)
    bad[0]["e"][1][-1] = bad[0]["e"][1][0]
    _rejects(R.check_la_proj_bwd, bad, refp)
    w, y = R.la_kv_case(3, 33, True)
    refk = R.la_kv_state(w, y, 3, 33)
    for k in ("kf", "v"):
        _rejects(R.check_la_kv_state, _row0_into_last(refk, [k]), refk)


def _without_tile(terms, tile, drop_tile):
    part = R.tile_partials(terms[0], terms[1], tile)
    part[drop_tile] = 0
    return R.ln_totals(part)


def test_planted_tile_missing_from_the_layernorm_sums():
    w, ctx, x, dout, d = R.vit_case(270, False, True)
    ref = R.vit_ffn_bwd(w, R.vit_tail(w, ctx, x, d)["x1"], dout, d)
    full = R.ln_totals(R.tile_partials(ref["term_g"], ref["term_b"], 16))
    R.check_vit_ffn_bwd(dict(ref, ln_g=full[0], ln_b=full[1]), ref)                   # the partial rows do sum to the totals
    for t in (0, 16):                                                                  # the first and the last (partial) tile
        lg, lb = _without_tile((ref["term_g"], ref["term_b"]), 16, t)
        _rejects(R.check_vit_ffn_bwd, dict(ref, ln_b=lb), ref)
        _rejects(R.check_vit_ffn_bwd, dict(ref, ln_g=lg), ref)
    for case in ((77, 64, True, 50, 128), (65536 + 33, 64, True, 70, 128)):
        w, px, py = R.lnqkv_case(*case)
        ref = R.lnqkv_bwd(w, px, py)
        tg = torch.cat([R.tile_partials(*ref["terms_x"], 32), R.tile_partials(*ref["terms_y"], 32)])
        lg, lb = R.ln_totals(tg)
        R.check_lnqkv_bwd(dict(ref, ln_g=lg, ln_b=lb), ref)
        for t in (0, tg.shape[0] - 1, (case[0] + 31) // 32 - 1):                      # first, last of y, last of x
            bad = tg.clone()
            bad[t] = 0
            lg, lb = R.ln_totals(bad)
            _rejects(R.check_lnqkv_bwd, dict(ref, ln_g=lg), ref)
            _rejects(R.check_lnqkv_bwd, dict(ref, ln_b=lb), ref)
    for rows in (8 * 32 + 1, 65536 + 288):
        w, sv, dout, d = R.la_mlp_case(rows, False)
        ref = R.la_mlp_bwd(w, sv, dout, d)
        for ln in ("1", "2"):
            part = R.tile_partials(*ref["terms" + ln], 32)
            part[-1] = 0
            lg, lb = R.ln_totals(part)
            _rejects(R.check_la_mlp_bwd, dict(ref, **{"ln%s_g" % ln: lg}), ref)
            _rejects(R.check_la_mlp_bwd, dict(ref, **{"ln%s_b" % ln: lb}), ref)


def test_planted_dropout_site_swapped_or_unscaled():
    w, ctx, x, dout, d = R.vit_case(17, True, True)
    ref = R.vit_tail(w, ctx, x, d)
    refb = R.vit_ffn_bwd(w, ref["x1"], dout, d)
    for a, b in (("proj", "act"), ("act", "fc2"), ("fc2", "act")):
        bad = R.Drop(R.SEED, R.VIT_SITES, swap={a: b})
        _rejects(R.check_vit_fwd, R.vit_tail(w, ctx, x, bad), ref)
        _rejects(R.check_vit_ffn_bwd, R.vit_ffn_bwd(w, ref["x1"], dout, bad), refb)
    for site in ("proj", "act", "fc2"):
        bad = R.Drop(R.SEED, R.VIT_SITES, unscaled=site)
        _rejects(R.check_vit_fwd, R.vit_tail(w, ctx, x, bad), ref)
        _rejects(R.check_vit_ffn_bwd, R.vit_ffn_bwd(w, ref["x1"], dout, bad), refb)
    w, x, kvsum, S = R.la_query_case(3, 33)
    refq = R.la_query_layer(w, x, kvsum, 3, 33, S, R.la_drop(True))
    w2, sv, dout, d = R.la_mlp_case(33, True)
    refm = R.la_mlp_bwd(w2, sv, dout, d)
    for a, b in (("att", "hid"), ("hid", "out"), ("out", "att")):
        _rejects(R.check_la_query, R.la_query_layer(w, x, kvsum, 3, 33, S, R.Drop(R.SEED, R.LA_SITES, swap={a: b})), refq)
    for a, b in (("att", "out"), ("out", "att")):                  # (the backward reads the hidden mask from the saved activations)
        _rejects(R.check_la_mlp_bwd, R.la_mlp_bwd(w2, sv, dout, R.Drop(R.SEED, R.LA_SITES, swap={a: b})), refm)
    for site in ("att", "hid", "out"):
        _rejects(R.check_la_query, R.la_query_layer(w, x, kvsum, 3, 33, S, R.Drop(R.SEED, R.LA_SITES, unscaled=site)), refq)
    for site in ("att", "out"):
        _rejects(R.check_la_mlp_bwd, R.la_mlp_bwd(w2, sv, dout, R.Drop(R.SEED, R.LA_SITES, unscaled=site)), refm)
    # attention: the mask of the neighbouring site, and the missing scale
    c = R.mha_case(5, 4, "uniform")
    a = (c["q"], c["k"], c["v"], c["dout"], R.MHA_B, 5, 4)
    M = R.mha_mask(R.MHA_B, 5, 4, True)
    ref = R.mha_bwd(*a, M)
    other = torch.from_numpy(R.keep_mask(R.SEED, R.MHA_SITE + 1, M.numel(), R.MHA_P)).reshape(M.shape).double() * R.keep_scale(R.MHA_P)
    _rejects(R.check_mha_bwd, R.mha_bwd(*a, other), ref)
    _rejects(R.check_mha_bwd, R.mha_bwd(*a, (M != 0).double()), ref)


def test_planted_transposed_weight():
    w, ctx, x, dout, d = R.vit_case(17, False, True)
    ref = R.vit_tail(w, ctx, x, d)
    _rejects(R.check_vit_fwd, R.vit_tail(w, ctx, x, d, transposed="wo"), ref)
    _rejects(R.check_vit_ffn_bwd, R.vit_ffn_bwd(w, ref["x1"], dout, d, transposed="wo"), R.vit_ffn_bwd(w, ref["x1"], dout, d))
    w, px, py = R.lnqkv_case(33, 64, False, 0, 0)
    _rejects(R.check_lnqkv_bwd, R.lnqkv_bwd(w, px, py, transposed=True), R.lnqkv_bwd(w, px, py))
    w, x, kvsum, S = R.la_query_case(2, 144)
    _rejects(R.check_la_query, R.la_query_layer(w, x, kvsum, 2, 144, S, R.NoDrop(), transposed="wm"), R.la_query_layer(w, x, kvsum, 2, 144, S, R.NoDrop()))
    w, sv, dout, d = R.la_mlp_case(33, False)
    _rejects(R.check_la_mlp_bwd, R.la_mlp_bwd(w, sv, dout, d, transposed="wm"), R.la_mlp_bwd(w, sv, dout, d))
    w, probs = R.la_proj_case("cross", 33, 77)
    _rejects(R.check_la_proj_bwd, R.la_proj_bwd(w, probs, transposed=0), R.la_proj_bwd(w, probs))


def test_planted_ksum_scaled_by_one_over_s():
    w, y = R.la_kv_case(3, 33, True)
    _rejects(R.check_la_kv_state, R.la_kv_state(w, y, 3, 33, ksum_scaled=True), R.la_kv_state(w, y, 3, 33))
    c = R.la_bwd_case(15, 17)
    _, kvsum = R.la_core(c["qf"].double(), c["kf"].double(), c["v"].double(), R.LA_BWD_B, 15, 17, R.LA_EPS)
    a = (c["qf"], c["kf"], c["v"], kvsum, c["dmsg"], R.LA_BWD_B, 15, 17, R.LA_EPS)
    _rejects(R.check_la_bwd, R.la_bwd(*a, ksum_scaled=True), R.la_bwd(*a))


def test_planted_dk_of_batch_1_in_batch_0():
    for dist in ("uniform", "peaked"):
        c = R.mha_case(5, 4, dist)
        a = (c["q"], c["k"], c["v"], c["dout"], R.MHA_B, 5, 4)
        _rejects(R.check_mha_bwd, R.mha_bwd(*a, leak=True), R.mha_bwd(*a))
