"""GPU tier, op level: the kernels behind the train-mode point path -- vecattn_front_train / vecattn_front_kv_train, vecattn_mix and
its backward, three_nn, weighted_gather3 / weighted_scatter3, segment_reduce, segment_softmax and its backward -- each against the plain
float64 restatement of tests/point_train_reference.py, at the row counts, layouts and edges where the kernels take another path.  The
inputs, the comparisons and the bars live in that module; tests/test_point_train_cpu.py shows on the CPU that each comparison rejects a
wrong result and where fp32 arithmetic sits inside each bar."""
import pytest
import torch

import point_train_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules switch autograd off process-wide at import; the float64 autograd references need it"""
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def ops():
    from cmr_agent_amd import ops as _ops
    return _ops


def dev(t):
    """to the device with the strides it has (a column slice stays a slice of a device copy of its buffer)"""
    if t is None or t._base is None:
        return None if t is None else t.to(DEV)
    return t._base.to(DEV).as_strided(t.shape, t.stride(), t.storage_offset())


def rows4(p):
    """[B, N, 3] -> contiguous [B * N, 4] device rows, 4th column zero (what planar_to_rows hands the point kernels)"""
    out = torch.zeros(p.shape[0] * p.shape[1], 4)
    out[:, :3] = p.reshape(-1, 3)
    return out.to(DEV)


# ------------------------------------------------------------------------------------------------------------------------------ front
GUARD = 64      # rows of NaN in front of, between and behind the outputs


def _guarded(n, rows):
    """n contiguous [rows, 64] outputs inside one NaN-filled buffer -> (outputs, the guard blocks around them)"""
    buf = torch.full((n * (rows + GUARD) + GUARD, 64), NAN, device=DEV)
    outs = [buf[GUARD + i * (rows + GUARD):][:rows] for i in range(n)]
    guards = [buf[i * (rows + GUARD):][:GUARD] for i in range(n + 1)]
    return outs, guards


def _call_front(ops, case, outs=None):
    rows, mode, kv, strided = case
    w, o = R.front_case(*case)
    pk = lambda wb: (wb[0].contiguous().to(DEV), wb[1].to(DEV))
    d0 = (torch.cat([w["d0"][0], torch.zeros(64, 1)], 1).to(DEV), w["d0"][1].to(DEV))            # K padded to 4 as _pack.lin does
    D = {k: dev(v) for k, v in o.items() if torch.is_tensor(v)}
    if strided:
        assert D["q"].stride(0) == 192 or kv == "rows"
        assert D["feat"].stride(0) == 128 if kv == "feat" else (D["k"].stride(0) == 192 and D["v"].stride(0) == 192)
    maps = dict(iq=D.get("iq"), divq=o.get("divq", 1), ia=None, diva=o.get("diva", 1), outs=outs)
    if kv == "feat":
        wk, between, wv = w["wk"].to(DEV), torch.empty(4096, device=DEV), w["wv"].to(DEV)           # two parameters: Wv does not follow Wk
        assert wv.data_ptr() != wk.data_ptr() + 4 * 4096
        got = ops.vecattn_front_kv_train(D["feat"], pk(w["fc1"]), wk, wv, D["q"], D["pa"], D["pb"], D["ib"], d0, pk(w["d2"]), pk(w["g0"]),
                                         pk(w["g2"]), **maps)
        names = ("a", "vp", "hd", "t", "g1", "x")
    else:
        got = ops.vecattn_front_train(D["k"], D["v"], D["q"], D["pa"], D["pb"], D["ib"], d0, pk(w["d2"]), pk(w["g0"]), pk(w["g2"]),
                                      ikv=D.get("ikv"), **maps)
        names = ("a", "vp", "hd", "t", "g1")
    return got, names, w, o


@pytest.mark.parametrize("case", R.FRONT_KV_CASES + R.FRONT_CASES, ids=lambda c: "%d-%s-%s" % c[:3])
def test_front_train_kernels_against_float64(ops, case):
    """Both train kernels of the front: every output -- a, vp, the stored hd, t, g1 and (computed k / v) x -- to 2e-5 of its own largest
    entry, the two stored ReLU maps equal to the float64 masks outside a band of 1e-5 of the largest pre-activation that holds at most
    1e-3 of the entries, and nothing written outside the [rows, 64] outputs (NaN guards around each).  Measured: the kernels are at most
    4.8e-7 off (g1 at 131 168 rows), fp32 torch on the CPU at most 4.3e-7; the band holds at most 1.1e-4 of the entries, with no mask
    entry differing outside it on either."""
    n = 6 if case[2] == "feat" else 5
    outs, guards = _guarded(n, case[0])
    got, names, w, o = _call_front(ops, case, outs)
    assert got is not False and all(g.data_ptr() == b.data_ptr() for g, b in zip(got, outs))
    torch.cuda.synchronize()
    figs = R.check_front(dict(zip(names, got)), R.front(w, **o))
    print("front %s: %s" % (case, {k: "%.2e" % v for k, v in figs.items()}))
    assert all(bool(torch.isnan(g).all()) for g in guards), "a store outside the outputs"


@pytest.mark.parametrize("kv", ["feat", "rows"])
def test_front_train_kernels_decline_rows_that_are_no_multiple_of_32(ops, kv):
    got, _, _, _ = _call_front(ops, (40, "group", kv, False))
    assert got is False


class _FrontModule(torch.nn.Module):
    """the parameters of a vector-attention front under the names the point transformers give them"""

    def __init__(self, w):
        super().__init__()
        L, S = torch.nn.Linear, torch.nn.Sequential
        self.fc1, self.w_ks, self.w_vs = L(64, 64), L(64, 64, bias=False), L(64, 64, bias=False)
        self.fc_delta = S(L(3, 64), torch.nn.ReLU(), L(64, 64))
        self.fc_gamma = S(L(64, 64), torch.nn.ReLU(), L(64, 64))
        params = dict(self.named_parameters())
        with torch.no_grad():
            for name, (key, i) in R.PARAM_OF.items():
                params[name].copy_(w[key] if i is None else w[key][i])


@pytest.mark.parametrize("mode", ["group", "knn"])
def test_front_through_the_tape_against_float64_autograd(ops, mode):
    """Tape.vecattn_front_kv (96 rows, 7 nodes, one of them without points) and Tape.vecattn_front (6 nodes x 16 neighbours, k / v tables
    through kv_idx) with the loss sum(a Wa) + sum(vp Wvp): every parameter gradient and the gradients of feat, q_src, k, v against float64
    autograd of front(), to 1e-4 of each gradient's own largest entry (a gradient that is truly zero: of the case's largest).  Measured:
    at most 5.0e-7 (the gradient of feat), the same 5.0e-7 for fp32 autograd on the CPU."""
    from cmr_agent_amd.train.flatbucket import FlatBucket
    from cmr_agent_amd.train.tape import Tape, Var
    w, o, (Wa, Wvp) = R.tape_case(mode)
    m = _FrontModule(w).to(DEV)
    bucket = FlatBucket(m)
    bucket.grads.zero_()
    t = Tape(bucket, None)
    rows, ib, pa4, pb4 = o["ib"].numel(), o["ib"].to(DEV), o["pa"].to(DEV), o["pb"].to(DEV)
    S = o["q"].shape[0]
    qn = Var(o["q"].to(DEV))
    ins = {"q": qn}
    if mode == "group":
        feat = ins["feat"] = Var(o["feat"].to(DEV))
        rel = Var(ops.rel_pos(pa4, pb4, rows, ib=ib), const=True)
        r = t.vecattn_front_kv(m.fc1, m.w_ks, m.w_vs, m.fc_delta, m.fc_gamma, feat, qn, ib, ops.csr_build(ib, 1, rows, S), rel, pa4, pb4, ib)
    else:
        k, v = ins["k"], ins["v"] = Var(o["k"].to(DEV)), Var(o["v"].to(DEV))
        rep = torch.arange(S, dtype=torch.int32).repeat_interleave(16).to(DEV)
        rel = Var(ops.rel_pos(pa4, pb4, rows, diva=16, ib=ib), const=True)
        r = t.vecattn_front(m.fc_delta, m.fc_gamma, qn, rep, ops.csr_build(rep, 1, rows, S), k, v, rel, pa4, pb4, ib, diva=16, kv_idx=ib,
                            kv_csr=ops.csr_build(ib, 1, rows, S))
    assert r is not None
    a, vp = r
    ref = R.front(w, **o)
    R.close(a.v, ref["a"], R.FRONT_RTOL, "a"), R.close(vp.v, ref["vp"], R.FRONT_RTOL, "vp")
    a.g, vp.g = Wa.to(DEV), Wvp.to(DEV)
    t.backward()
    torch.cuda.synchronize()
    got = dict(bucket.logical_grads())
    got.update({name: var.g for name, var in ins.items()})
    figs = R.check_grads(got, R.front_grads(w, o, (Wa, Wvp)))
    print("tape %s: %s" % (mode, {k: "%.2e" % v for k, v in figs.items()}))


# ------------------------------------------------------------------------------------------------------------------------------- mix
@pytest.mark.parametrize("rows", [1, 33, 3000])
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "ld192"])
def test_vecattn_mix_and_its_backward_are_exact(ops, rows, strided):
    """(q - k) + pos and v + pos in that order, dk = -da and dpos = da + dvp: the operation order Tape.vecattn_mix promises, so fp32 torch
    gives the same bits."""
    if strided:
        buf = R.rnd(rows, 192, seed=1)
        q, k, v = buf[:, 0:64], buf[:, 64:128], buf[:, 128:192]
        g = R.rnd(rows, 192, seed=3)
        da, dvp = g[:, 64:128], g[:, 128:192]
    else:
        q, k, v = (R.rnd(rows, 64, seed=s) for s in (1, 2, 3))
        da, dvp = R.rnd(rows, 64, seed=5), R.rnd(rows, 64, seed=6)
    pos = R.rnd(rows, 64, seed=4, lo=-3, hi=3)
    dq = dev(q)
    assert dq.stride(0) == (192 if strided else 64)
    a_in, vp = ops.vecattn_mix(dq, dev(k), dev(v), pos.to(DEV))
    assert torch.equal(a_in.cpu(), (q - k) + pos) and torch.equal(vp.cpu(), v + pos)
    dk, dpos = ops.vecattn_mix_bwd(dev(da), dev(dvp))
    assert torch.equal(dk.cpu(), -da) and torch.equal(dpos.cpu(), da + dvp)


# -------------------------------------------------------------------------------------------------------------------------- three_nn
@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("Nq,Nc", [(nq, nc) for nq in (1, 257, 600) for nc in (1, 2, 3, 1024, 1025, 2500)])
def test_three_nn_against_the_restatement(ops, kind, Nq, Nc):
    """Integer-lattice clouds (exact distances, ties everywhere) and random clouds in +-20; one and several query blocks with a partial
    last one, one and several candidate tiles, one, two and three candidates.  Indices (global rows b * Nc + local) equal the stable first
    three of the fp32 distances; weights to 1e-5 of each float64 weight (fp32 on the CPU: 1.8e-7); a query on a candidate gives that
    candidate all the weight; with one or two candidates the missing neighbours' weights are exactly 0 and their indices rows of the
    same batch element."""
    B = 3
    q, c = R.three_nn_case(kind, B, Nq, Nc)
    idx, wgt = ops.three_nn(rows4(q), rows4(c), B, Nq, Nc)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (B * Nq, 3) == tuple(wgt.shape)
    R.check_three_nn(idx, wgt, q, c)


@pytest.mark.parametrize("name", sorted(R.GATHER3_CASES))
@pytest.mark.parametrize("C", R.GATHER3_WIDTHS)
def test_weighted_gather3_and_scatter3_against_float64(ops, name, C):
    """The interpolation and its adjoint on the neighbours three_nn finds, CSR built as _fp_forward_train builds it, src and dy column
    slices of wider buffers: gather to 1e-6, scatter to 2e-5 of the output scale, <gather3(x), dy> = <x, scatter3(dy)> to 1e-5 of the
    inner product -- except at long / C = 24 and long / C = 4, where the products cancel and fp32 cannot reach it: fp32 torch on the CPU in
    the kernel's order is 1.25e-5 and 3.40e-5 off there (the kernel measured 1.19e-5 and 3.11e-5), and each of the two gets 4 x its own
    figure, rounded up (point_train_reference.gather3_adjoint_rtol); the other seven cases sit below 1.1e-6 in fp32 on the CPU.
    unreferenced: most source rows are nobody's neighbour and get exactly 0; long: three segments of 5000 entries per batch element;
    two: two candidates -- the result is the two-neighbour interpolation of the reference's dists[:, :, :3]."""
    B, Nq, Nc = R.GATHER3_CASES[name]
    q, c, src, dy = R.gather3_case(name, C)
    idx, wgt = ops.three_nn(rows4(q), rows4(c), B, Nq, Nc)
    R.check_three_nn(idx, wgt, q, c)
    ci, cw = idx.cpu().long(), wgt.cpu()
    ds, dd = dev(src), dev(dy)
    assert ds.stride(0) == C + 12 and dd.stride(0) == C + 8
    out = ops.weighted_gather3(ds, idx, wgt)
    figs = dict(gather=R.close(out, R.weighted_gather3(src, ci, cw), 1e-6, "gather3"))
    if name == "two":
        ri, rw = R.three_nn(q, c)
        two = rw[:, 0:1] * src.double()[ri[:, 0]] + rw[:, 1:2] * src.double()[ri[:, 1]]
        R.close(out, two, 1e-6, "two-neighbour interpolation")
    offsets, order = ops.csr_build(idx.view(-1), B, 3 * Nq, Nc)
    sc = ops.weighted_scatter3(dd, wgt, order, offsets, B * Nc)
    figs["scatter"] = R.close(sc, R.weighted_scatter3(dy, ci, cw, B * Nc), 2e-5, "scatter3")
    figs["adjoint"] = R.check_adjoint(R.dot64(out, dy), R.dot64(src, sc), "gather3 / scatter3", R.gather3_adjoint_rtol(name, C))
    print("gather3 %s C=%d: %s" % (name, C, {k: "%.2e" % v for k, v in figs.items()}))
    if name == "unreferenced":
        free = torch.ones(B * Nc, dtype=torch.bool)
        free[ci.reshape(-1)] = False
        assert int(free.sum()) > B * Nc // 2 and float(sc.cpu()[free].abs().max()) == 0
    if name == "long":
        assert int((offsets[1:] - offsets[:-1]).min()) > 4000


# -------------------------------------------------------------------------------------------------------------------- segment_reduce
@pytest.fixture(scope="module")
def seg(ops):
    key = R.segment_case()
    offsets, order = ops.csr_build(key.to(DEV), 1, key.numel(), R.SEG_NSEG)
    assert torch.equal(torch.sort(order.cpu().long())[0], torch.arange(key.numel()))         # a genuine permutation
    return key, R.segments_of(key, R.SEG_NSEG), offsets, order


@pytest.mark.parametrize("C", [3, 20, 64, 128])
def test_segment_reduce_against_float64(ops, seg, C):
    """sum / max / mean over 203 segments (not a multiple of the 4 of a workgroup) of lengths 0, 1, 7, 8, 9, 1000 and 0 .. 12, rows in a
    random order, src a column slice; fewer and more channels than the 64 lanes.  All-negative data: max is exact, 0 on the empty
    segments and nowhere else; sum / mean to 2e-5 of the output scale (fp32 on the CPU, adding in the same order: 1.4e-6);
    <gather(x), dy> = <x, segment_sum(dy)> to 1e-5."""
    key, segs, offsets, order = seg
    src = R.rnd(3000, C + 8, seed=140 + C, lo=-2.0, hi=-0.5)[:, 4:4 + C][:key.numel()]
    d = dev(src)
    assert d.stride(0) == C + 8
    figs = {mode: R.check_segment_reduce(ops.segment_reduce(d, order, offsets, R.SEG_NSEG, mode), src, segs, mode) for mode in ("sum", "max", "mean")}
    x = R.rnd(R.SEG_NSEG, C, seed=7)
    figs["adjoint"] = R.check_adjoint(R.dot64(ops.gather_rows(x.to(DEV), key.to(DEV)), src), R.dot64(x, ops.segment_reduce(d, order, offsets, R.SEG_NSEG, "sum")),
                                     "gather / segment sum")
    print("segment_reduce C=%d: %s" % (C, {k: "%.2e" % v for k, v in figs.items()}))


# ------------------------------------------------------------------------------------------------------------------- segment softmax
@pytest.mark.parametrize("kind", ["peaked", "long", "dropped"])
def test_segment_softmax_and_its_backward_against_float64(ops, kind):
    """peaked: attn in +-300 at scale 0.125, one member of a segment takes nearly all the weight; long: a segment of 5000 members;
    dropped: about 1 % of the keys point outside their batch element's segments -- csr_build drops them, no segment lists their rows, and
    their gradients are exactly zero even when the allocator hands back a block full of NaN.  Forward to 2e-5, gradients to 5e-5 of the
    output scale (measured: at most 4.0e-7, fp32 torch on the CPU 4.3e-7).  covers_all_rows=True (what the tape passes) gives the same
    bits where the segments do list every row."""
    attn, vp, dout, key, (B, N, M), ok = R.softmax_case(kind)
    segs = R.segments_of(key, B * M)
    offsets, order = ops.csr_build(key.to(DEV), B, N, M)
    ad, vd, gd = attn.to(DEV), vp.to(DEV), dout.to(DEV)
    out = ops.segment_softmax(ad, vd, B * M, R.SOFTMAX_SCALE, order=order, offsets=offsets)
    junk = [torch.full((B * N, 64), NAN, device=DEV) for _ in range(2)]                    # the blocks the two gradients are about to get
    torch.cuda.synchronize()
    del junk
    da, dv = ops.segment_softmax_bwd(ad, vd, gd, B * M, R.SOFTMAX_SCALE, order=order, offsets=offsets)
    figs = R.check_softmax(out, da, dv, attn, vp, dout, segs, ok)
    print("softmax %s: %s" % (kind, {k: "%.2e" % v for k, v in figs.items()}))
    if bool(ok.all()):
        da2, dv2 = ops.segment_softmax_bwd(ad, vd, gd, B * M, R.SOFTMAX_SCALE, order=order, offsets=offsets, covers_all_rows=True)
        assert torch.equal(da2, da) and torch.equal(dv2, dv)
