"""GPU tier: every fused entry point the image tower trains through, called on its own through the C ABI and compared with the float64
restatements of tests/block_train_reference.py (whose own correctness, bars and rejection of wrong results tests/test_block_train_cpu.py
shows without a GPU) -- csrc/vit_train.hip (cmr_vit_out_ffn16_train_f32, cmr_vit_ffn_bwd16_f32, cmr_vit_lnqkv_bwd_f32), the train
instances of csrc/la_fused.hip (cmr_la_kv_state_train_f32, cmr_la_query_layer_train_f32), csrc/la_train.hip (cmr_la_mlp_bwd_f32,
cmr_la_proj_bwd_f32) and csrc/train_geo.hip (cmr_mha_bwd_f32 / cmr_mha_dropout_bwd_f32, cmr_la_bwd_f32).

Every output buffer starts as NaN, so an element that is never written shows; every output carries guard rows past its documented
extent (whole tiles where the kernel stores unpredicated) inside the same tensor, which must still be NaN afterwards.  Dropout masks
come from the CPU restatement, pinned bit for bit against cmr_dropout_f32 by the first test."""
import numpy as np
import pytest
import torch

import block_train_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 3
f32 = torch.float32


def raw(name, *args):
    """status of an entry point, without the wrapper's exception"""
    from cmr_agent_amd import _lib
    return getattr(_lib.load(), name)(*args)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def dv(t):
    """device copy that keeps the strides of a column slice (the base buffer travels, the view is taken again)"""
    if t is None:
        return None
    base = t._base if t._base is not None else t
    return base.to(DEV).as_strided(t.size(), t.stride(), t.storage_offset())


def p_(t):
    return None if t is None else t.data_ptr()


def nan(rows, C):
    return torch.full((rows + GUARD, C), float("nan"), dtype=f32, device=DEV)


def intact(t, rows):
    """the guard rows past `rows` are still NaN"""
    return bool(torch.isnan(t[rows:]).all())


def up(rows, tile):
    return (rows + tile - 1) // tile * tile


def seed_of(drop):
    return None if drop.seed is None else torch.full((1,), drop.seed, dtype=torch.int64, device=DEV)


def show(name, case, figs):
    print("%s %s: %s" % (name, case, "  ".join("%s %.2e" % kv for kv in figs.items())))


# ---------------------------------------------------------------------------------------------------------------------------------- mask
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_device_mask_is_the_restated_mask(p):
    """ops.dropout of ones == keep_mask / (1 - p) bit for bit; row width 30 (no multiple of 4), rebuilt through a flat call"""
    from cmr_agent_amd import ops
    seed, site = torch.full((1,), R.SEED, dtype=torch.int64, device=DEV), 5
    for rows, width in ((37, 30), (20000, 64)):
        n = rows * width
        flat = ops.dropout(torch.ones((n + 3) // 4, 4, device=DEV), p, seed, site).reshape(-1)[:n].view(rows, width).cpu()
        want = torch.from_numpy(R.keep_mask(R.SEED, site, n, p)).view(rows, width).float() * R.keep_scale(p)
        assert torch.equal(flat, want)
    neg = torch.full((1,), -3, dtype=torch.int64, device=DEV)
    got = ops.dropout(torch.ones(64, 64, device=DEV), p, neg, 2 ** 40 + 1).cpu()
    assert torch.equal(got != 0, torch.from_numpy(R.keep_mask(-3, 2 ** 40 + 1, 4096, p)).view(64, 64))


# ---------------------------------------------------------------------------------------------------------------------------- fragments
def test_pack_frags_matches_the_host_packers():
    """cmr_pack_frags_f32 against _pack.frag_pack / frag_pack16, exactly: plain and transposed blocks, and the koff form that writes
    [Wq; Wk; Wv]^T and [Wk; Wv]^T block by block -- the operands of the kernels below"""
    from cmr_agent_amd import ops
    from cmr_agent_amd.models import _pack
    mats = dict(wq=R.rnd(64, 64, seed=1), wk=R.rnd(64, 64, seed=2), wv=R.rnd(64, 64, seed=3), w1=R.rnd(1024, 64, seed=4), w2=R.rnd(64, 1024, seed=5),
                bias=R.rnd(1024, seed=6)[:190])
    src_off, off = {}, 5 * 4                                    # slots do not start at 0
    for k, m in mats.items():
        src_off[k] = off
        off += (m.numel() + 3) // 4 * 4 + 4
    src = torch.zeros(off)
    for k, m in mats.items():
        src[src_off[k]:src_off[k] + m.numel()] = m.reshape(-1)
    cat3, cat2 = torch.cat([mats["wq"], mats["wk"], mats["wv"]]), torch.cat([mats["wk"], mats["wv"]])
    # (expected fragments, the blocks (stored matrix, kind, transposed, ktot, koff) that write them)
    dests = [(_pack.frag_pack(mats["wq"]), [("wq", 0, False, None, 0)]),
             (_pack.frag_pack(mats["wq"].T.contiguous()), [("wq", 0, True, None, 0)]),
             (_pack.frag_pack(cat3.T.contiguous()), [("wq", 0, True, 192, 0), ("wk", 0, True, 192, 64), ("wv", 0, True, 192, 128)]),
             (_pack.frag_pack(cat2.T.contiguous()), [("wk", 0, True, 128, 0), ("wv", 0, True, 128, 64)])]
    for name in ("wq", "w1", "w2"):
        dests += [(_pack.frag_pack16(mats[name]), [(name, 1, False, None, 0)]),
                  (_pack.frag_pack16(mats[name].T.contiguous()), [(name, 1, True, None, 0)])]
    rows, want, dst = [], [], 0
    for expect, blocks in dests:
        for name, kind, tr, ktot, koff in blocks:
            sn, sk = mats[name].shape
            n, k = (sk, sn) if tr else (sn, sk)
            rows.append([src_off[name], n, k, sk, dst, kind, int(tr), n * k, ktot if ktot is not None else k, koff])
        want.append((dst, expect))
        dst += (expect.numel() + 63) // 64 * 64
    want.append((dst, mats["bias"]))
    rows.append([src_off["bias"], 190, 0, 0, dst, 2, 0, 192, 0, 0])
    dst += 192
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    out = torch.full((dst + 64,), float("nan"), device=DEV)
    ops.pack_frags(src.to(DEV), out, table, len(rows), max(r[7] for r in rows))
    out = out.cpu()
    for o, expect in want:
        assert torch.equal(out[o:o + expect.numel()], expect.reshape(-1)), o
    assert bool(torch.isnan(out[dst:]).all())


# --------------------------------------------------------------------------------------------------------------------------- ViT tail
def _vit_frags(w):
    from cmr_agent_amd.models import _pack
    f = {k + "_f": _pack.frag_pack16(w[k]).to(DEV) for k in ("wo", "w1", "w2")}
    f.update({k + "T_f": _pack.frag_pack16(w[k].T.contiguous()).to(DEV) for k in ("wo", "w1", "w2")})
    f.update({k: w[k].to(DEV) for k in ("bo", "g2", "b2n", "b1", "b2")})
    return f


def _vit_drop_args(d, seed):
    if d.seed is None:
        return 0.0, 0.0, None, 0, 0, 0
    s = d.sites
    return s["proj"][1], s["act"][1], seed.data_ptr(), s["proj"][0], s["act"][0], s["fc2"][0]


def run_vit_fwd(w, f, ctx, x, d):
    rows = x.shape[0]
    seed = seed_of(d)
    ctx, x = dv(ctx), dv(x)
    out, x1 = nan(rows, 64), nan(rows, 64)
    rc = raw("cmr_vit_out_ffn16_train_f32", p_(ctx), ctx.stride(0), p_(x), x.stride(0), p_(f["wo_f"]), p_(f["bo"]), p_(f["g2"]), p_(f["b2n"]),
             w["eps"], p_(f["w1_f"]), p_(f["b1"]), p_(f["w2_f"]), p_(f["b2"]), p_(out), 64, p_(x1), 64, rows, *_vit_drop_args(d, seed), _stream())
    assert rc == 0
    assert intact(out, rows) and intact(x1, rows)
    return dict(out=out[:rows], x1=x1[:rows])


def run_vit_bwd(w, f, x1, dout, d):
    rows = x1.shape[0]
    pad, tiles = up(rows, 16), (rows + 15) // 16
    seed = seed_of(d)
    x1, dout = dv(x1), dv(dout)
    o = {k: nan(pad, 1024 if k in ("gs", "du") else 64) for k in ("dx1", "dctx", "gs", "du", "h", "dm", "da")}
    lnpart = nan(tiles, 128)
    rc = raw("cmr_vit_ffn_bwd16_f32", p_(dout), dout.stride(0), p_(x1), x1.stride(0), p_(f["g2"]), p_(f["b2n"]), w["eps"], p_(f["w1_f"]), p_(f["b1"]),
             p_(f["w2T_f"]), p_(f["w1T_f"]), p_(f["woT_f"]), p_(o["dx1"]), 64, p_(o["dctx"]), 64, p_(o["gs"]), p_(o["du"]), p_(o["h"]), p_(o["dm"]),
             p_(o["da"]), p_(lnpart), rows, *_vit_drop_args(d, seed), _stream())
    assert rc == 0
    for k, t in o.items():
        assert intact(t, pad), "%s: written past its whole tiles" % k
    assert intact(lnpart, tiles)
    got = {k: t[:rows] for k, t in o.items()}
    got["ln_g"], got["ln_b"] = R.ln_totals(lnpart[:tiles])
    return got


@pytest.mark.parametrize("rows,drop,strided", R.VIT_CASES)
def test_vit_out_ffn16_train_and_ffn_bwd16(rows, drop, strided):
    w, ctx, x, dout, d = R.vit_case(rows, drop, strided)
    f = _vit_frags(w)
    ref = R.vit_tail(w, ctx, x, d)
    show("vit_out_ffn16_train", (rows, drop, strided), R.check_vit_fwd(run_vit_fwd(w, f, ctx, x, d), ref))
    x1 = ref["x1"].float()                                  # the backward is checked on its own: it gets the restated x1
    show("vit_ffn_bwd16", (rows, drop, strided), R.check_vit_ffn_bwd(run_vit_bwd(w, f, x1, dout, d), R.vit_ffn_bwd(w, x1, dout, d)))


# ---------------------------------------------------------------------------------------------------- LayerNorm + q / k / v backward
def run_lnqkv(w, px, py):
    from cmr_agent_amd.models import _pack
    g, b = w["g"].to(DEV), w["b"].to(DEV)
    args, outs, keep = [], {}, []
    tiles = 0
    for tag, pr in (("x", px), ("y", py)):
        if pr is None:
            args += [None, 0, 0, None, None, 0, None, 64, None, 64, 0]
            continue
        rows = pr["x"].shape[0]
        d, x, res = dv(pr["d"]), dv(pr["x"]), dv(pr.get("res"))
        wt = _pack.frag_pack(w["wcat"][pr["lo"]:pr["hi"]].T.contiguous()).to(DEV)
        dx, xn = nan(rows, 64), nan(rows, 64)
        keep += [d, x, res, wt]
        outs["d" + tag], outs[tag + "n"] = (dx, rows), (xn, rows)
        tiles += (rows + 31) // 32
        a = [p_(d), d.stride(0), d.shape[1], p_(wt), p_(x), x.stride(0)]
        if tag == "x":
            a += [p_(res), res.stride(0) if res is not None else 0]
        args += a + [p_(dx), 64, p_(xn), 64, rows]
    lnpart = nan(tiles, 128)
    rc = raw("cmr_vit_lnqkv_bwd_f32", *args, p_(g), p_(b), w["eps"], p_(lnpart), _stream())
    assert rc == 0
    got = {}
    for k, (t, rows) in outs.items():
        assert intact(t, rows), k
        got[k] = t[:rows]
    assert intact(lnpart, tiles)
    got["ln_g"], got["ln_b"] = R.ln_totals(lnpart[:tiles])
    return got


@pytest.mark.parametrize("case", R.LNQKV_CASES)
def test_vit_lnqkv_bwd(case):
    w, px, py = R.lnqkv_case(*case)
    show("vit_lnqkv_bwd", case, R.check_lnqkv_bwd(run_lnqkv(w, px, py), R.lnqkv_bwd(w, px, py)))


# ---------------------------------------------------------------------------------------------------------------- linear attention
def run_la_kv(w, y, B, S):
    from cmr_agent_amd import _lib
    y, wk, wv = dv(y), w["wk"].to(DEV), w["wv"].to(DEV)
    nb = _lib.load().cmr_la_kv_state_workspace_bytes(B, S)
    ws = torch.full((nb // 4 + 64,), float("nan"), device=DEV)
    kvsum, kf, v = nan(B, 576), nan(B * S, 64), nan(B * S, 64)
    rc = raw("cmr_la_kv_state_train_f32", p_(y), y.stride(0), p_(wk), p_(wv), p_(kvsum), p_(kf), p_(v), p_(ws), nb, B, S, _stream())
    assert rc == 0
    assert intact(kvsum, B) and intact(kf, B * S) and intact(v, B * S) and bool(torch.isnan(ws[nb // 4:]).all())
    return dict(kvsum=kvsum[:B], kf=kf[:B * S], v=v[:B * S])


@pytest.mark.parametrize("B,S,strided", R.LA_KV_CASES)
def test_la_kv_state_train(B, S, strided):
    w, y = R.la_kv_case(B, S, strided)
    show("la_kv_state_train", (B, S, strided), R.check_la_kv_state(run_la_kv(w, y, B, S), R.la_kv_state(w, y, B, S)))


@pytest.mark.parametrize("S", [33, 257, 8193 + 32])
def test_la_kv_state_train_does_not_depend_on_the_batch(S):
    """the same sample alone and as element 2 of 3: the same bits"""
    w, y = R.la_kv_case(3, S, False)
    three, one = run_la_kv(w, y, 3, S), run_la_kv(w, y[2 * S:].contiguous(), 1, S)
    assert torch.equal(three["kvsum"][2], one["kvsum"][0])
    assert torch.equal(three["kf"][2 * S:], one["kf"]) and torch.equal(three["v"][2 * S:], one["v"])


LA_SAVED = ("qf", "msg", "mm", "d1", "hid", "o")


def _la_drop_args(d, seed):
    if d.seed is None:
        return 0.0, None, 0, 0, 0
    s = d.sites
    return R.LA_P, seed.data_ptr(), s["att"][0], s["hid"][0], s["out"][0]


def run_la_query(w, x, kvsum, B, L, S, d, expect=0):
    rows = B * L
    pad = up(rows, 32)
    seed = seed_of(d)
    x, kvsum = dv(x), kvsum.to(DEV)
    wd = {k: w[k].to(DEV) for k in w}
    out = nan(rows, 64)
    sv = {k: nan(pad, 128 if k == "hid" else 64) for k in LA_SAVED}
    rc = raw("cmr_la_query_layer_train_f32", p_(x), x.stride(0), p_(kvsum), p_(wd["wq"]), p_(wd["wm"]), p_(wd["g1"]), p_(wd["b1"]), p_(wd["w0"]),
             p_(wd["w3"]), p_(wd["g2"]), p_(wd["b2"]), p_(out), 64, *[p_(sv[k]) for k in LA_SAVED], B, L, S, R.LA_EPS, R.LA_LN_EPS,
             *_la_drop_args(d, seed), _stream())
    assert rc == expect
    if expect != 0:
        assert bool(torch.isnan(out).all()) and all(bool(torch.isnan(t).all()) for t in sv.values())
        return None
    assert intact(out, rows)
    for k, t in sv.items():
        assert intact(t, pad), "%s: written past its whole tiles" % k
    got = {k: t[:rows] for k, t in sv.items()}
    got["out"] = out[:rows]
    return got


@pytest.mark.parametrize("B,L,drop", R.LA_QUERY_CASES)
def test_la_query_layer_train(B, L, drop):
    w, x, kvsum, S = R.la_query_case(B, L)
    d = R.la_drop(drop)
    show("la_query_layer_train", (B, L, drop), R.check_la_query(run_la_query(w, x, kvsum, B, L, S, d), R.la_query_layer(w, x, kvsum, B, L, S, d)))


def test_la_query_layer_train_refuses_twelve_states():
    """34 304 + 576 B floats of LDS <= 160 KB: B <= 11.  B = 12 is UNSUPPORTED and nothing is written."""
    from cmr_agent_amd import _lib
    w = R.la_weights()
    assert (34304 + 576 * 11) * 4 <= 160 * 1024 < (34304 + 576 * 12) * 4
    x, kvsum = R.rnd(12 * 5, 64, seed=1), R.rnd(12, 576, seed=2, lo=0.5, hi=1.5)
    run_la_query(w, x, kvsum, 12, 5, 7, R.NoDrop(), expect=_lib.UNSUPPORTED)
    x, kvsum = R.rnd(11 * 5, 64, seed=1), R.la_kv_state(w, R.rnd(11 * 7, 64, seed=3), 11, 7)["kvsum"].float()
    got = run_la_query(w, x, kvsum, 11, 5, 7, R.NoDrop())
    show("la_query_layer_train", (11, 5, False), R.check_la_query(got, R.la_query_layer(w, x, kvsum, 11, 5, 7, R.NoDrop())))


def run_la_mlp_bwd(w, sv, dout, d):
    rows = dout.shape[0]
    pad = up(rows, 32)
    nt = min(256, ((rows + 31) // 32 + 7) // 8)
    seed = seed_of(d)
    dout = dv(dout)
    svd = {k: v.to(DEV) for k, v in sv.items()}
    wd = {k: w[k].to(DEV) for k in ("wm", "w0", "w3", "g1", "g2")}
    keys = ("d_o", "d_hid", "d_mm", "d_msg", "d_xa")
    o = {k: nan(pad, 128 if k == "d_hid" else 64) for k in keys}
    ln1, ln2 = nan(nt, 128), nan(nt, 128)
    rc = raw("cmr_la_mlp_bwd_f32", p_(dout), dout.stride(0), p_(svd["o"]), p_(svd["hid"]), p_(svd["mm"]), p_(wd["wm"]), p_(wd["w0"]), p_(wd["w3"]),
             p_(wd["g1"]), p_(wd["g2"]), *[p_(o[k]) for k in keys], p_(ln1), p_(ln2), rows, R.LA_LN_EPS, *_la_drop_args(d, seed), _stream())
    assert rc == 0
    for k, t in o.items():
        assert intact(t, pad), "%s: written past its whole tiles" % k
    assert intact(ln1, nt) and intact(ln2, nt)
    got = {k: t[:rows] for k, t in o.items()}
    got["ln1_g"], got["ln1_b"] = R.ln_totals(ln1[:nt])
    got["ln2_g"], got["ln2_b"] = R.ln_totals(ln2[:nt])
    return got


@pytest.mark.parametrize("rows,drop", R.LA_MLP_CASES)
def test_la_mlp_bwd(rows, drop):
    w, sv, dout, d = R.la_mlp_case(rows, drop)
    show("la_mlp_bwd", (rows, drop), R.check_la_mlp_bwd(run_la_mlp_bwd(w, sv, dout, d), R.la_mlp_bwd(w, sv, dout, d)))


def run_la_proj(w, problems):
    """terms with a saved f write e: in place where d is contiguous (as the tape calls it), into a buffer of its own where d is a slice"""
    from cmr_agent_amd.models import _pack
    wt = {k: _pack.frag_pack(w[k].T.contiguous()).to(DEV) for k in ("wq", "wk", "wv")}
    desc, outs, keep = [], [], []
    for pr in problems:
        rows = pr["rows"]
        dx = nan(rows, 64)
        res = [dv(r) for r in pr["res"]] + [None, None]
        d = [rows, len(pr["terms"]), p_(dx), 64, p_(res[0]) or 0, res[0].stride(0) if res[0] is not None else 0, p_(res[1]) or 0,
             res[1].stride(0) if res[1] is not None else 0]
        es = []
        for dd, f, name in pr["terms"]:
            ddv, fd = dv(dd), dv(f)
            e = None
            if f is not None:
                e = ddv if ddv.stride(0) == 64 else nan(rows, 64)
            es.append(e)
            keep += [ddv, fd]
            d += [p_(ddv), ddv.stride(0), p_(fd) or 0, p_(wt[name]), p_(e) or 0]
        d += [0, 0, 0, 0, 0] * (3 - len(pr["terms"]))
        desc += d
        keep += res
        outs.append((dx, es, rows))
    arr = np.asarray(desc, dtype=np.int64)
    rc = raw("cmr_la_proj_bwd_f32", arr.ctypes.data, len(problems), _stream())
    assert rc == 0
    got = []
    for dx, es, rows in outs:
        assert intact(dx, rows)
        assert all(e is None or e.shape[0] == rows or intact(e, rows) for e in es)
        got.append(dict(dx=dx[:rows], e=[None if e is None else e[:rows] for e in es]))
    return got


@pytest.mark.parametrize("form,rows_x,rows_y", R.LA_PROJ_CASES)
def test_la_proj_bwd(form, rows_x, rows_y):
    w, probs = R.la_proj_case(form, rows_x, rows_y)
    ref = R.la_proj_bwd(w, probs)                           # before the run: e overwrites d in place
    show("la_proj_bwd", (form, rows_x, rows_y), R.check_la_proj_bwd(run_la_proj(w, probs), ref))


def run_la_bwd(c, kvsum, L, S, acc):
    from cmr_agent_amd import _lib
    B = R.LA_BWD_B
    nb = _lib.load().cmr_la_bwd_workspace_bytes(B, L)
    ws = torch.full((nb // 4 + 64,), float("nan"), device=DEV)
    qf, kf, v, dm = (dv(c[k]) for k in ("qf", "kf", "v", "dmsg"))
    kvsum = kvsum.to(DEV)
    o = dict(dqf=nan(B * L, 64), dkf=nan(B * S, 64), dv=nan(B * S, 64))
    if acc:
        for k, t in o.items():
            t[:c["old"][k].shape[0]] = c["old"][k].to(DEV)
    rc = raw("cmr_la_bwd_f32", p_(qf), 64, p_(kf), 64, p_(v), 64, p_(kvsum), p_(dm), 64, p_(o["dqf"]), 64, int(acc), p_(o["dkf"]), 64, int(acc),
             p_(o["dv"]), 64, int(acc), p_(ws), nb, B, L, S, R.LA_EPS, _stream())
    assert rc == 0
    assert intact(o["dqf"], B * L) and intact(o["dkf"], B * S) and intact(o["dv"], B * S) and bool(torch.isnan(ws[nb // 4:]).all())
    return dict(dqf=o["dqf"][:B * L], dkf=o["dkf"][:B * S], dv=o["dv"][:B * S])


@pytest.mark.parametrize("L,S", R.LA_BWD_CASES)
def test_la_bwd(L, S):
    c = R.la_bwd_case(L, S)
    _, kvsum = R.la_core(c["qf"].double(), c["kf"].double(), c["v"].double(), R.LA_BWD_B, L, S, R.LA_EPS)
    kvsum = kvsum.float()
    ref = R.la_bwd(c["qf"], c["kf"], c["v"], kvsum, c["dmsg"], R.LA_BWD_B, L, S, R.LA_EPS)
    show("la_bwd", (L, S, "written"), R.check_la_bwd(run_la_bwd(c, kvsum, L, S, False), ref))
    plus = dict(ref, **{k: ref[k] + c["old"][k].double() for k in R.LA_BWD_BARS})
    show("la_bwd", (L, S, "accumulated"), R.check_la_bwd(run_la_bwd(c, kvsum, L, S, True), plus))


# ------------------------------------------------------------------------------------------------------------------ softmax attention
def run_mha(c, o, Tq, Tk, drop, acc):
    """dq | dk | dv as column blocks of one [rows, 192] buffer when Tq = Tk, else dq alone and dk | dv of a [rows, 128] buffer"""
    B = R.MHA_B
    q, k, v, dout, o = dv(c["q"]), dv(c["k"]), dv(c["v"]), dv(c["dout"]), o.to(DEV)
    if Tq == Tk:
        buf = nan(B * Tq, 192)
        dq, dk, dvv = buf[:, 0:64], buf[:, 64:128], buf[:, 128:192]
    else:
        dq, buf = nan(B * Tq, 64), nan(B * Tk, 128)
        dk, dvv = buf[:, 0:64], buf[:, 64:128]
    outs = dict(dq=(dq, B * Tq), dk=(dk, B * Tk), dv=(dvv, B * Tk))
    if acc:
        for key, (t, rows) in outs.items():
            t[:rows] = c["old"][key].to(DEV)
    ws = torch.full((B * Tq * 16 + 64,), float("nan"), device=DEV)
    a = [p_(q), q.stride(0), p_(k), k.stride(0), p_(v), v.stride(0), p_(o), o.stride(0), p_(dout), dout.stride(0), p_(dq), dq.stride(0), int(acc),
         p_(dk), dk.stride(0), int(acc), p_(dvv), dvv.stride(0), int(acc), p_(ws), B * Tq * 16 * 4, B, Tq, Tk]
    if drop:
        seed = torch.full((1,), R.SEED, dtype=torch.int64, device=DEV)
        rc = raw("cmr_mha_dropout_bwd_f32", *a, R.MHA_P, p_(seed), R.MHA_SITE, _stream())
    else:
        rc = raw("cmr_mha_bwd_f32", *a, _stream())
    assert rc == 0
    got = {}
    for key, (t, rows) in outs.items():
        assert intact(t, rows), key
        got[key] = t[:rows]
    assert bool(torch.isnan(ws[B * Tq * 16:]).all())
    got["lse"], got["dsum"] = ws[:B * Tq * 8].view(B * Tq, 8), ws[B * Tq * 8:B * Tq * 16].view(B * Tq, 8)
    return got


@pytest.mark.parametrize("Tq,Tk,dist,drop", R.MHA_CASES)
def test_mha_bwd(Tq, Tk, dist, drop):
    c = R.mha_case(Tq, Tk, dist)
    M = R.mha_mask(R.MHA_B, Tq, Tk, drop)
    ref = R.mha_bwd(c["q"], c["k"], c["v"], c["dout"], R.MHA_B, Tq, Tk, M)
    o = ref["o"].float()
    name = "mha_dropout_bwd" if drop else "mha_bwd"
    show(name, (Tq, Tk, dist, "written"), R.check_mha_bwd(run_mha(c, o, Tq, Tk, drop, False), ref))
    plus = dict(ref, **{k: ref[k] + c["old"][k].double() for k in ("dq", "dk", "dv")})
    show(name, (Tq, Tk, dist, "accumulated"), R.check_mha_bwd(run_mha(c, o, Tq, Tk, drop, True), plus))


# ------------------------------------------------------------------------------------------------------------------ single-row gradients
def test_single_row_gradient_vit_ffn_bwd16():
    rows = 40
    w, ctx, x, dout, d = R.vit_case(rows, True, False)
    f = _vit_frags(w)
    x1 = R.vit_tail(w, ctx, x, d)["x1"].float()
    for row in R.seam_rows(rows, 16):
        g = R.one_row(dout, row)
        got, ref = run_vit_bwd(w, f, x1, g, d), R.vit_ffn_bwd(w, x1, g, d)
        for key in ("dx1", "dctx", "du", "dm", "da"):
            assert R.others_zero(got[key], [row]), (key, row)
        show("vit_ffn_bwd16 one row", row, R.check_vit_ffn_bwd(got, ref))
        R.close(got["ln_g"], ref["term_g"][row], R.BAR_VIT_LN, "d gamma = the row's term")
        R.close(got["ln_b"], ref["term_b"][row], R.BAR_VIT_LN, "d beta = the row's term")


def test_single_row_gradient_vit_lnqkv_bwd():
    w, px, py = R.lnqkv_case(77, 192, False, 0, 0)
    for row in R.seam_rows(77, 32):
        one = dict(px, d=R.one_row(px["d"], row))
        got, ref = run_lnqkv(w, one, None), R.lnqkv_bwd(w, one, None)
        assert R.others_zero(got["dx"], [row]), row
        show("vit_lnqkv_bwd one row", row, R.check_lnqkv_bwd(got, ref))
        R.close(got["ln_g"], ref["terms_x"][0][row], R.BAR_VIT_LN, "d gamma = the row's term")
        R.close(got["ln_b"], ref["terms_x"][1][row], R.BAR_VIT_LN, "d beta = the row's term")


def test_single_row_gradient_la_mlp_bwd():
    rows = 77
    w, sv, dout, d = R.la_mlp_case(rows, True)
    for row in R.seam_rows(rows, 32):
        g = R.one_row(dout, row)
        got, ref = run_la_mlp_bwd(w, sv, g, d), R.la_mlp_bwd(w, sv, g, d)
        for key in ("d_o", "d_hid", "d_mm", "d_msg", "d_xa"):
            assert R.others_zero(got[key], [row]), (key, row)
        show("la_mlp_bwd one row", row, R.check_la_mlp_bwd(got, ref))
        for ln in ("1", "2"):
            R.close(got["ln%s_g" % ln], ref["terms" + ln][0][row], R.BAR_LA_LN, "d gamma %s = the row's term" % ln)
            R.close(got["ln%s_b" % ln], ref["terms" + ln][1][row], R.BAR_LA_LN, "d beta %s = the row's term" % ln)


def test_single_row_gradient_la_proj_bwd():
    w, probs = R.la_proj_case("self", 77, 0)
    pr = probs[0]
    for row in R.seam_rows(77, 32):
        one = [dict(rows=77, terms=[(R.one_row(dd, row), f, name) for dd, f, name in pr["terms"]], res=[R.one_row(r, row) for r in pr["res"]])]
        ref = R.la_proj_bwd(w, one)
        got = run_la_proj(w, one)
        assert R.others_zero(got[0]["dx"], [row]), row
        assert all(e is None or R.others_zero(e, [row]) for e in got[0]["e"]), row
        show("la_proj_bwd one row", row, R.check_la_proj_bwd(got, ref))


def test_single_row_gradient_mha_bwd():
    """one query row's gradient: no other query's dq, and no dk / dv of the other batch element"""
    Tq, Tk, B = 130, 257, R.MHA_B
    c = R.mha_case(Tq, Tk, "uniform")
    for drop in (False, True):
        M = R.mha_mask(B, Tq, Tk, drop)
        for row in (63, 64, Tq - 1, Tq + 64):
            one = dict(c, dout=R.one_row(c["dout"], row))
            ref = R.mha_bwd(c["q"], c["k"], c["v"], one["dout"], B, Tq, Tk, M)
            got = run_mha(one, ref["o"].float(), Tq, Tk, drop, False)
            b = row // Tq
            own = range(b * Tk, (b + 1) * Tk)
            assert R.others_zero(got["dq"], [row]) and R.others_zero(got["dk"], own) and R.others_zero(got["dv"], own), (drop, row)
            show("mha_bwd one row", (row, drop), R.check_mha_bwd(got, ref))
