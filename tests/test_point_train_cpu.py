"""CPU tier: the float64 restatements of tests/point_train_reference.py and the comparisons tests/test_point_train_ops_gpu.py makes with
them have teeth.  (a) The restatements agree with torch autograd of the same formulas written another way, and the adjoint identities
hold.  (b) For every comparison of the GPU file, a deliberately wrong variant of the reference fails it.  (c) The same formulas in fp32
torch, on the GPU file's own inputs, stay inside every tolerance and cap with room (the figures are in the assertions)."""
import pytest
import torch
import torch.nn.functional as F

import point_train_reference as R

f64 = torch.float64


@pytest.fixture(autouse=True)
def _grad_enabled():
    with torch.enable_grad():
        yield


# ------------------------------------------------------------------------------------------------------------- (a) the restatements
def _front_as_the_modules_write_it(w, o, loss_w):
    """PointNN.py:151-166 / 219-225 with nn.functional layers on [1, C, rows] maps and torch.gather, as the reference modules do"""
    leaf = lambda t: t.double().clone().requires_grad_(True)
    conv = lambda x, wb: F.conv1d(x, wb[0][:, :, None], wb[1])
    P = {k: (tuple(leaf(t) for t in v) if isinstance(v, tuple) else leaf(v)) for k, v in w.items()}
    I = {k: leaf(o[k]) for k in ("feat", "q", "k", "v") if k in o}
    rows = o["ib"].numel()
    bcl = lambda t: t.T[None]                                             # [n, C] -> [1, C, n]
    take = lambda t, idx: torch.gather(bcl(t), 2, idx.long()[None, None, :].expand(1, t.shape[1], rows))
    if "feat" in o:
        x = conv(bcl(I["feat"]), P["fc1"])
        k, v = F.conv1d(x, P["wk"][:, :, None]), F.conv1d(x, P["wv"][:, :, None])
        q = take(I["q"], o["iq"])
        rel = bcl(o["pa"].double()[:, :3]) - take(o["pb"].double()[:, :3], o["ib"])
    else:
        k, v = take(I["k"], o["ikv"]), take(I["v"], o["ikv"])
        q = bcl(I["q"].repeat_interleave(16, 0))
        rel = bcl(o["pa"].double()[:, :3].repeat_interleave(16, 0)) - take(o["pb"].double()[:, :3], o["ib"])
    pos = conv(F.relu(conv(rel, P["d0"])), P["d2"])
    a = conv(F.relu(conv(q - k + pos, P["g0"])), P["g2"])
    ((a[0].T * loss_w[0].double()).sum() + ((v + pos)[0].T * loss_w[1].double()).sum()).backward()
    grads = {}
    for name, (key, i) in R.PARAM_OF.items():
        t = P[key] if i is None else P[key][i]
        grads[name] = t.grad if t.grad is not None else torch.zeros_like(t)
    grads.update({k: t.grad for k, t in I.items()})
    return grads


@pytest.mark.parametrize("mode", ["group", "knn"])
def test_front_gradients_agree_with_autograd_of_the_modules_formulation(mode):
    w, o, lw = R.tape_case(mode)
    ref, other = R.front_grads(w, o, lw), _front_as_the_modules_write_it(w, o, lw)
    assert set(ref) == set(other)
    for name in ref:
        assert R.rel_err(other[name], ref[name]) <= 1e-12 or float(ref[name].abs().max()) == 0 == float(other[name].abs().max()), name
    unused = [n for n, g in ref.items() if float(g.abs().max()) == 0]
    assert unused == ([] if mode == "group" else ["fc1.weight", "fc1.bias", "w_ks.weight", "w_vs.weight"])
    if mode == "group":
        assert float(ref["q"][6].abs().max()) == 0 and float(ref["q"][:6].abs().min(0)[0].max()) > 0     # the node without points


def _gather3_operands(name, C):
    q, c, src, dy = R.gather3_case(name, C)
    idx, wgt = R.three_nn(q, c)
    return idx, wgt, src, dy


@pytest.mark.parametrize("name", sorted(R.GATHER3_CASES))
def test_gather3_scatter3_are_adjoint_and_agree_with_autograd(name):
    idx, wgt, src, dy = _gather3_operands(name, 24)
    x = src.double().clone().requires_grad_(True)
    out = sum(wgt[:, j:j + 1] * x[idx[:, j]] for j in range(3))
    assert R.rel_err(R.weighted_gather3(src, idx, wgt), out) <= 1e-14
    out.backward(dy.double())
    sc = R.weighted_scatter3(dy, idx, wgt, src.shape[0])
    assert R.rel_err(sc, x.grad) <= 1e-13
    R.check_adjoint(R.dot64(R.weighted_gather3(src, idx, wgt), dy), R.dot64(src, sc), name)
    if name == "unreferenced":
        free = torch.ones(src.shape[0], dtype=torch.bool)
        free[idx.reshape(-1)] = False
        assert int(free.sum()) > src.shape[0] // 2 and float(sc[free].abs().max()) == 0


def test_segment_reductions_agree_with_autograd_and_the_gather_identity():
    key = R.segment_case()
    segs = R.segments_of(key, R.SEG_NSEG)
    assert {0, 1, 7, 8, 9, 1000} <= set(m.numel() for m in segs)
    assert sum(m.numel() for m in segs) == key.numel()
    x = R.rnd(R.SEG_NSEG, 20, seed=1).double().requires_grad_(True)
    dy = R.rnd(key.numel(), 20, seed=2)
    x[key.long()].backward(dy.double())                                                  # gather_rows and its backward
    ssum = R.segment_reduce(dy, segs, "sum")
    assert R.rel_err(ssum, x.grad) <= 1e-13
    R.check_adjoint(R.dot64(x[key.long()], dy), R.dot64(x, ssum), "gather / segment sum")
    ref = torch.zeros(R.SEG_NSEG, 20, dtype=f64).scatter_reduce_(0, key.long()[:, None].expand(-1, 20), dy.double(), "amax", include_self=False)
    assert torch.equal(R.segment_reduce(dy, segs, "max"), ref)
    cnt = torch.bincount(key.long(), minlength=R.SEG_NSEG).clamp_min(1).double()
    assert R.rel_err(R.segment_reduce(dy, segs, "mean"), ssum / cnt[:, None]) <= 1e-14


@pytest.mark.parametrize("kind", ["peaked", "long", "dropped"])
def test_segment_softmax_backward_agrees_with_autograd(kind):
    attn, vp, dout, key, (B, N, M), ok = R.softmax_case(kind)
    segs = R.segments_of(key, B * M)
    assert sum(m.numel() for m in segs) == int(ok.sum())
    a, v = attn.double().requires_grad_(True), vp.double().requires_grad_(True)
    R.segment_softmax(a, v, segs, R.SOFTMAX_SCALE).backward(dout.double())
    da, dv = R.segment_softmax_bwd(attn, vp, dout, segs, R.SOFTMAX_SCALE)
    assert R.rel_err(da, a.grad) <= 1e-12 and R.rel_err(dv, v.grad) <= 1e-12
    if kind == "dropped":
        assert 10 < int((~ok).sum()) < 200 and float(da[~ok].abs().max()) == 0 == float(dv[~ok].abs().max())
    if kind == "peaked":                     # one member of a segment takes nearly all the weight
        p = torch.softmax(attn.double()[segs[0]] * R.SOFTMAX_SCALE, 0)
        assert float(p.max(0)[0].median()) > 0.9


# --------------------------------------------------------------------------------------------------------------- (b) wrong variants
def _front_ref(case):
    w, o = R.front_case(*case)
    return R.front(w, **o)


def _as_kernel_outputs(ref, case):
    keys = ("a", "vp", "hd", "t", "g1") + (("x",) if case[2] == "feat" else ())
    return {k: ref[k].float() for k in keys}


WRONG_FRONT_CASE = R.FRONT_KV_CASES[2]       # 288 rows, computed k / v: all six outputs


@pytest.mark.parametrize("key", ["a", "vp", "hd", "t", "g1", "x"])
@pytest.mark.parametrize("variant", ["tail tile dropped", "row 0 in place of the last row"])
def test_front_comparison_rejects_a_wrong_output(key, variant):
    ref = _front_ref(WRONG_FRONT_CASE)
    got = _as_kernel_outputs(ref, WRONG_FRONT_CASE)
    R.check_front(got, ref)
    if variant == "tail tile dropped":
        got[key][-32:] = 0
    else:
        got[key][-1] = got[key][0]
    with pytest.raises(AssertionError):
        R.check_front(got, ref)


@pytest.mark.parametrize("key", ["hd", "g1"])
def test_mask_comparison_rejects_one_flipped_bit_and_a_band_that_swallows(key):
    ref = _front_ref(WRONG_FRONT_CASE)
    got = _as_kernel_outputs(ref, WRONG_FRONT_CASE)
    pre = ref[key + "_pre"]
    band = R.MASK_BAND * float(pre.abs().max())
    assert R.relu_mask_agrees(got[key], pre, band)[0] == 0
    # a clipped entry stored as a tiny positive number, a live one as zero, both 100 bands from zero; the value itself is taken as given
    # (the reference entry replaced by it), so that the mask comparison alone has to object
    far = (pre.abs() > 100 * band) & (pre.abs() < 200 * band)
    neg, posi = (far & (pre < 0)).nonzero()[0], (far & (pre > 0)).nonzero()[0]
    for (r, c), value in ((neg, 1e-30), (posi, 0.0)):
        bad = {k: v.clone() for k, v in got.items()}
        bad[key][r, c] = value
        assert R.relu_mask_agrees(bad[key], pre, band)[0] == 1
        with pytest.raises(AssertionError, match="mask entries differ"):
            R.check_front(bad, {**ref, key: bad[key].double()})
    wide = dict(ref)
    wide[key + "_pre"] = torch.where(pre.abs() == pre.abs().max(), pre, pre * 1e-3)      # about 1 % of the entries inside the band
    with pytest.raises(AssertionError, match="the band holds"):
        R.check_front(got, wide)


def _first_tie(q, c, idx):
    """-> (row, j, other): neighbour j of query `row` has the same distance as candidate `other` > idx[row, j], which is not among the three"""
    B, Nq, Nc = q.shape[0], q.shape[1], c.shape[1]
    d = R.sqdist3(q, c).view(B * Nq, Nc)
    base = torch.arange(B * Nq) // Nq * Nc
    for row in range(B * Nq):
        for j in range(3):
            same = (d[row] == d[row, idx[row, j] - base[row]]).nonzero().view(-1) + base[row]
            later = [int(t) for t in same if int(t) > int(idx[row, j]) and int(t) not in idx[row].tolist()]
            if later:
                return row, j, later[0]
    raise AssertionError("no tie in the case")


def test_three_nn_comparison_rejects_wrong_neighbours_and_weights():
    q, c = R.three_nn_case("lattice", 3, 257, 1025)
    idx, wgt = R.three_nn(q, c)
    R.check_three_nn(idx, wgt, q, c)
    row, j, other = _first_tie(q, c, idx)
    bad = idx.clone()
    bad[row, j] = other                                                  # a tie resolved to the larger index: same distance, same weights
    with pytest.raises(AssertionError, match="other neighbours"):
        R.check_three_nn(bad, wgt, q, c)
    bad = idx.clone()
    bad[300] -= 1025                                                      # local instead of global rows in the second batch element
    with pytest.raises(AssertionError):
        R.check_three_nn(bad, wgt, q, c)
    bad = wgt.clone()
    bad[5] = bad[5] * torch.tensor([1 + 3e-5, 1, 1])
    with pytest.raises(AssertionError, match="weights"):
        R.check_three_nn(idx, bad, q, c)


def test_three_nn_comparison_rejects_a_third_neighbour_of_two():
    q, c = R.three_nn_case("lattice", 3, 257, 2)
    idx, wgt = R.three_nn(q, c)
    R.check_three_nn(idx, wgt, q, c)
    assert float(wgt[:, 2].abs().max()) == 0 and float((wgt[:, :2].sum(1) - 1).abs().max()) < 1e-15
    assert float((wgt[0] - torch.tensor([1.0, 0, 0], dtype=f64)).abs().max()) < 1e-6       # query 0 sits on candidate 0
    bad = wgt.clone()
    bad[7, 2] = 1e-30                                                     # the third weight not zero
    with pytest.raises(AssertionError, match="missing neighbour"):
        R.check_three_nn(idx, bad, q, c)
    bad = idx.clone()
    bad[300, 2] = 0                                                       # the dummy index in another batch element
    with pytest.raises(AssertionError, match="outside"):
        R.check_three_nn(bad, wgt, q, c)
    # three neighbours' weights where two exist: the interpolation differs
    src = R.rnd(6, 8, seed=3)
    two = R.weighted_gather3(src, idx, wgt)
    even = R.weighted_gather3(src, idx, torch.full_like(wgt, 1 / 3))
    assert R.rel_err(even, two) > 1e-2


def _neg_src(C):
    return R.rnd(3000, C + 8, seed=140 + C, lo=-2.0, hi=-0.5)[:, 4:4 + C]


@pytest.mark.parametrize("mode,kwargs", [("max", dict(init=0.0)), ("mean", dict(mean_extra=1))])
def test_segment_reduce_comparison_rejects_a_wrong_reduction(mode, kwargs):
    key = R.segment_case()
    segs = R.segments_of(key, R.SEG_NSEG)
    src = _neg_src(20)[:key.numel()]
    R.check_segment_reduce(R.segment_reduce(src, segs, mode), src, segs, mode)
    with pytest.raises(AssertionError):
        R.check_segment_reduce(R.segment_reduce(src, segs, mode, **kwargs), src, segs, mode)
    if mode == "max":                     # all-negative data: 0 on the empty segments and nowhere else
        out = R.segment_reduce(src, segs, "max")
        empty = torch.tensor([m.numel() == 0 for m in segs])
        assert bool((out[empty] == 0).all()) and bool((out[~empty] < 0).all()) and int(empty.sum()) > 1


def test_softmax_and_gradient_comparisons_reject_wrong_results():
    attn, vp, dout, key, (B, N, M), ok = R.softmax_case("dropped")
    segs = R.segments_of(key, B * M)
    out = R.segment_softmax(attn, vp, segs, R.SOFTMAX_SCALE)
    da, dv = R.segment_softmax_bwd(attn, vp, dout, segs, R.SOFTMAX_SCALE)
    R.check_softmax(out, da, dv, attn, vp, dout, segs, ok)
    junk = da.clone()
    junk[(~ok).nonzero()[0]] = 1e-30                                      # what an unwritten buffer may hold
    with pytest.raises(AssertionError, match="not exactly zero"):
        R.check_softmax(out, junk, dv, attn, vp, dout, segs, ok)
    junk[(~ok).nonzero()[0]] = float("nan")
    with pytest.raises(AssertionError):
        R.check_softmax(out, junk, dv, attn, vp, dout, segs, ok)
    with pytest.raises(AssertionError):
        R.check_softmax(out, da, dv * (1 + 1e-4), attn, vp, dout, segs, ok)
    w, o, lw = R.tape_case("group")
    ref = R.front_grads(w, o, lw)
    R.check_grads(ref, ref)
    for name in ("fc_delta.0.weight", "q"):
        bad = dict(ref)
        bad[name] = ref[name].clone()
        bad[name].view(-1)[3] += 2e-4 * ref[name].abs().max()
        with pytest.raises(AssertionError):
            R.check_grads(bad, ref)
    w, o, lw = R.tape_case("knn")
    ref = R.front_grads(w, o, lw)
    bad = dict(ref)
    bad["fc1.weight"] = ref["fc1.weight"] + 2e-4 * max(float(g.abs().max()) for g in ref.values())    # a true zero gradient: absolute bar
    with pytest.raises(AssertionError):
        R.check_grads(bad, ref)


# ------------------------------------------------------------------------------------------------ (c) fp32 on the GPU file's inputs
@pytest.mark.parametrize("case", R.FRONT_KV_CASES + R.FRONT_CASES, ids=lambda c: "%d-%s-%s" % c[:3])
def test_fp32_front_sits_far_inside_the_bars(case):
    w, o = R.front_case(*case)
    ref = R.front(w, **o)
    figs = R.check_front(_as_kernel_outputs(R.front(w, dtype=torch.float32, **o), case), ref)
    for key, val in figs.items():
        if key.endswith("band_share"):
            assert val <= R.MASK_BAND_CAP / 4, (key, val)                  # at most 1.1e-4 of the entries on these inputs
        else:
            assert val <= R.FRONT_RTOL / 10, (key, val)                    # at most 4.3e-7


@pytest.mark.parametrize("mode", ["group", "knn"])
def test_fp32_front_gradients_sit_inside_the_bar(mode):
    w, o, lw = R.tape_case(mode)
    figs = R.check_grads(R.front_grads(w, o, lw, dtype=torch.float32), R.front_grads(w, o, lw))
    assert max(figs.values()) <= R.TAPE_GRAD_RTOL / 10, figs


THREE_NN_SHAPES = [(nq, nc) for nq in (1, 257, 600) for nc in (1, 2, 3, 1024, 1025, 2500)]


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("Nq,Nc", THREE_NN_SHAPES)
def test_fp32_three_nn_weights_sit_inside_the_bar(kind, Nq, Nc):
    q, c = R.three_nn_case(kind, 3, Nq, Nc)
    idx, _ = R.three_nn(q, c)
    err = R.check_three_nn(idx, R.three_nn_weights_fp32(q, c, idx), q, c)
    assert err <= R.THREE_NN_WGT_RTOL / 10, err


@pytest.mark.parametrize("name", sorted(R.GATHER3_CASES))
@pytest.mark.parametrize("C", R.GATHER3_WIDTHS)
def test_fp32_gather3_scatter3_sit_inside_the_bars(name, C):
    idx, wgt, src, dy = _gather3_operands(name, C)
    g, sc = R.gather3_scatter3_fp32(src, dy, idx, wgt)
    assert R.rel_err(g, R.weighted_gather3(src, idx, wgt.float())) <= 1e-6 / 4
    assert R.rel_err(sc, R.weighted_scatter3(dy, idx, wgt.float(), src.shape[0])) <= 2e-5 / 4
    # the adjoint identity in fp32, case by case: inside 1e-5 with room, or -- long segments of few channels, where the products cancel --
    # no more than the figure its raised bar is 4 x of
    e = R.check_adjoint(R.dot64(g, dy), R.dot64(src, sc), name, R.gather3_adjoint_rtol(name, C))
    assert e <= R.GATHER3_ADJOINT_FP32.get((name, C), 1e-5 / 4), (name, C, e)
    if (name, C) in R.GATHER3_ADJOINT_FP32:
        assert e > 1e-5, "fp32 reaches 1e-5 here: the raised bar is not needed"


def test_gather3_adjoint_bar_is_raised_for_the_two_cancelling_cases_only():
    bars = {(n, C): R.gather3_adjoint_rtol(n, C) for n in R.GATHER3_CASES for C in R.GATHER3_WIDTHS}
    assert sorted(k for k, v in bars.items() if v != 1e-5) == [("long", 4), ("long", 24)] and max(bars.values()) == 4 * 3.5e-5


@pytest.mark.parametrize("C", [3, 20, 64, 128])
def test_fp32_segment_reduce_sits_inside_the_bars(C):
    key = R.segment_case()
    segs = R.segments_of(key, R.SEG_NSEG)
    src = _neg_src(C)[:key.numel()]
    for mode in ("sum", "max", "mean"):
        assert R.check_segment_reduce(R.segment_reduce_fp32(src, segs, mode), src, segs, mode) <= 2e-5 / 4
    x = R.rnd(R.SEG_NSEG, C, seed=7)
    R.check_adjoint(R.dot64(x[key.long()], src), R.dot64(x, R.segment_reduce_fp32(src, segs, "sum")), "gather / segment sum", 1e-5 / 4)


@pytest.mark.parametrize("kind", ["peaked", "long", "dropped"])
def test_fp32_segment_softmax_sits_inside_the_bars(kind):
    attn, vp, dout, key, (B, N, M), ok = R.softmax_case(kind)
    segs = R.segments_of(key, B * M)
    f = torch.float32
    out = R.segment_softmax(attn, vp, segs, R.SOFTMAX_SCALE, dtype=f)
    da, dv = R.segment_softmax_bwd(attn, vp, dout, segs, R.SOFTMAX_SCALE, dtype=f)
    figs = R.check_softmax(out, da, dv, attn, vp, dout, segs, ok)
    assert figs["out"] <= R.SOFTMAX_FWD_RTOL / 4 and max(figs["da"], figs["dv"]) <= R.SOFTMAX_BWD_RTOL / 4, figs
