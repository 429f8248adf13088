"""GPU tier of the agent 3-D branch / tail suite: cmr_cbr_block_f32, cmr_cbr_block_bf16_f32, cmr_colmax_partials_f32, cmr_colmax_bias2_f32,
CMRAgent._embed_3d_any and the three tail entry points against the float64 restatements of tests/agent_branch_reference.py -- bit for bit on
the exact cases, within 2 x the a-priori element-wise bound on the real-valued ones (the bf16 block: the bars of test_cbr_block_bf16).
Every test prints the worst error / bound it saw.

Largest error / bound per entry point on an MI355X (2 allowed):
    cmr_cbr_block_f32            0.127  (the 8-8-64 instantiation, second pass of the tile loop; the 64- and 128-wide ones stay under 0.02)
    its column maxima            0.124  (8-8-64; under 0.02 otherwise), bit-equal to the maxima of the y of the same launch throughout
    cmr_colmax_bias2_f32         0.015  (the three launches it replaces: the same)
    cmr_agent_heads_f32 / _t     0.058  on the logits (the contracting cases, whose bound is the tight one; 0.011 on the signal-carrying
                                        ones at the product's widths, 0.001 at a feature-map mean of 1000)
    cmr_agent_heads_train_f32    0.235  on a saved intermediate (the early layers' bounds are a few roundings wide); logits as above
    cmr_cbr_block_bf16_f32       0.03 of its 2e-3 bar against the bf16-operand restatement
    the branch through CMRAgent  2.5e-7 of the output scale in fp32 (bar 1e-4), 2.3e-3 in bf16 mode (bar 2e-2)
No ratio comes near 1: the bound is a worst case over every summation order, the kernels' errors are those of one fixed order.
Every exact case is bit-equal to float64."""
import pytest
import torch

import agent_branch_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32 = R.F64, R.F32
NAN = float("nan")


def dev(t):
    """to the device; a column slice of a wider buffer stays one (same strides and offset)"""
    if t is None:
        return None
    if t._base is not None and not t.is_contiguous():
        return torch.as_strided(t._base.to(DEV), tuple(t.shape), t.stride(), t.storage_offset())
    return t.contiguous().to(DEV)


@pytest.fixture(params=["f32", "bf16"])
def mode(request):
    from cmr_agent_amd import ops
    old = ops.CONV_BF16
    ops.CONV_BF16 = request.param == "bf16"
    try:
        yield request.param
    finally:
        ops.CONV_BF16 = old


def cases(inst, name, mode):
    """the cases of one block test, from the table both tiers share"""
    for kind, kw in R.block_table(inst, name, mode == "bf16"):
        yield R.table_case(inst, kind, kw, mode == "bf16"), "%s %s %s" % (inst, kind, kw)


def make(inst, rows, mode, kind, **kw):
    return R.block_case(inst, rows, kind=kind, bf16=(mode == "bf16" and kind == "exact"), **kw)


def run_block(c, want_y=True, want_colmax=False):
    from cmr_agent_amd import ops
    return ops.cbr_block(dev(c.x1), dev(c.w1), dev(c.b1), dev(c.w2), dev(c.b2), dev(c.wsc), c.slope, x2=dev(c.x2), idx2=dev(c.idx2), div2=c.div2,
                         rows_per_batch=c.rpb, want_y=want_y, want_colmax=want_colmax)


def check_rows(c, got, mode, stat, what, ref=None, reduce=None):
    """got against the restatement of c (reduce: what to compare of y and of its bound -- per-tile or per-sample maxima)."""
    ref = R.block_ref(c) if ref is None else ref
    red = reduce or (lambda t: t)
    if c.kind == "exact":
        ok, msg = R.close_exact(got, red(ref.y), what)
        assert ok, msg
    elif mode == "f32":
        ok, worst, msg = R.close_bounded(got, red(ref.y), red(R.block_bound(c, ref)[1]), 2.0, what)
        stat.append(worst)
        assert ok, msg
    else:                                                         # the bars of test_bf16_gpu.test_cbr_block_bf16, unchanged
        scale = float(ref.y.abs().max())
        g = got.cpu().to(F64)
        e_bf = float((g - red(R.block_ref(c, bf16=True).y)).abs().max())
        e_fp = float((g - red(ref.y)).abs().max())
        stat.append(e_bf / (2e-3 * scale))
        assert e_bf <= 2e-3 * scale, (what, e_bf / scale)
        assert e_fp <= 2e-2 * scale, (what, e_fp / scale)
    return ref


def report(name, stat):
    print("  %s: worst error / bound %.3f over %d comparisons" % (name, max(stat) if stat else 0.0, len(stat)))


# ------------------------------------------------------------------------------------------------------------------ the block
@pytest.mark.parametrize("inst", R.INSTANCES, ids=lambda i: "%d-%d-%d-%s" % i)
def test_block_row_counts(inst, mode):
    """1, 31, 32, 33 and 261 rows: fewer rows than a tile, a whole tile, a partial last tile; exact and every real-valued variant."""
    stat = []
    for c, what in cases(inst, "rows", mode):
        out = run_block(c)
        assert out is not None and out[1] is None
        check_rows(c, out[0], mode, stat, what)
    report("block rows", stat)


@pytest.mark.parametrize("inst", R.INSTANCES, ids=lambda i: "%d-%d-%d-%s" % i)
def test_block_second_pass_of_the_tile_loop(inst, mode):
    """threshold + 39 rows: the persistent grid's first pass ends at 65 536 rows (256 workgroups x 8 tiles, LDS footprint over 80 KB) or at
    131 072 (512 workgroups; the bf16 launch always); the tiles behind it are the ones whose inputs were fetched a tile ahead."""
    stat = []
    for c, what in cases(inst, "second_pass", mode):
        assert c.rows == R.wrap_rows(inst, bf16=(mode == "bf16"))
        out = run_block(c)
        assert out is not None
        check_rows(c, out[0], mode, stat, what)
    report("block second pass", stat)


def test_block_third_pass_uses_the_index_fetched_two_tiles_ahead(mode):
    stat = []
    for c, what in cases(R.INSTANCES[0], "third_pass", mode):
        assert c.rows == 262183 and c.k1 == 32 and c.idx2 is not None
        out = run_block(c)
        assert out is not None
        check_rows(c, out[0], mode, stat, what)
    report("block third pass", stat)


@pytest.mark.parametrize("inst", R.INSTANCES, ids=lambda i: "%d-%d-%d-%s" % i)
def test_block_sources(inst, mode):
    """two sources with k1 on and off a half-group boundary, gather (repeats, both extreme indices) and broadcast, column slices of wider
    buffers; for the two identity instantiations the shortcut runs over the concatenated input."""
    stat = []
    for c, what in cases(inst, "sources", mode):
        check_rows(c, run_block(c)[0], mode, stat, what)
    report("block sources", stat)


@pytest.mark.parametrize("inst", R.INSTANCES, ids=lambda i: "%d-%d-%d-%s" % i)
def test_block_per_batch_biases(inst, mode):
    """tiles that straddle samples (40 rows a sample), one row a sample, a short last sample, one of the two biases per batch, bias rows as
    slices of a wider buffer; 17 samples are refused."""
    stat = []
    for c, what in cases(inst, "biases", mode):
        assert c.nb == 16
        check_rows(c, run_block(c)[0], mode, stat, what)
    for rows, rpb in ((680, 40), (17, 1), (641, 40)):
        c = make(inst, rows, mode, "exact", rpb=rpb, per_batch=(True, False))
        assert c.nb == 17 and run_block(c) is None
    report("block per-batch biases", stat)


@pytest.mark.parametrize("inst", R.INSTANCES, ids=lambda i: "%d-%d-%d-%s" % i)
def test_block_column_maxima(inst, mode):
    """one tile a sample (B = 1, 5, 16) and 513 tiles a sample (the second pass of the fold's 512-tile loop): the maxima against the
    reference's and, bit for bit, against the y of the same launch; without y the partials are the same bits."""
    from cmr_agent_amd import ops
    stat = []
    co = inst[2]
    for c, what in cases(inst, "colmax", mode):
        B, rpb = c.nb, c.rpb
        y, cm = run_block(c, want_colmax=True)
        ref = check_rows(c, y, mode, stat, what + " y")
        check_rows(c, cm, mode, stat, what + " maxima", ref=ref, reduce=lambda t: t.view(B, rpb, co).max(1)[0])
        assert torch.equal(cm, y.view(B, rpb, co).max(1)[0])
        y2, part = run_block(c, want_colmax="partials")
        none, part2 = run_block(c, want_y=False, want_colmax="partials")
        assert none is None and torch.equal(y2, y) and torch.equal(part, part2)
        assert torch.equal(part, y.view(-1, 32, co).max(1)[0])
        assert torch.equal(ops.colmax_partials(part, B, rpb // 32), cm)
    for rows, rpb in ((80, 40), (96, 64)):                        # rows_per_batch % 32 != 0, rows % rows_per_batch != 0
        c = make(inst, rows, mode, "exact", rpb=rpb, per_batch=(True, True))
        assert run_block(c, want_colmax=True) is None and run_block(c, want_colmax="partials") is None
    report("block column maxima", stat)


@pytest.mark.parametrize("inst", R.INSTANCES, ids=lambda i: "%d-%d-%d-%s" % i)
def test_block_writes_nothing_else(inst, mode):
    """through the C entry point: y a column slice of a NaN-filled buffer (ldy = CO + 8, four guard rows), the partials with a guard tile,
    a partial last tile whose maxima leave the rows past the end out."""
    from cmr_agent_amd import _lib, ops
    kx, ch, co, conv = inst
    rows = 261
    nt = (rows + 31) // 32
    p = lambda t: None if t is None else t.data_ptr()
    stat = []
    for c, what in cases(inst, "guards", mode):
        assert c.rows == rows
        kind = c.kind
        x1, x2, idx = dev(c.x1), dev(c.x2), dev(c.idx2)
        w1, b1, w2, b2, wsc = dev(c.w1), dev(c.b1), dev(c.w2), dev(c.b2), dev(c.wsc)
        ybuf = torch.full((rows + 4, co + 8), NAN, dtype=F32, device=DEV)
        pbuf = torch.full((nt + 1, co), NAN, dtype=F32, device=DEV)
        y = ybuf[:rows, 4:4 + co]
        _lib.call("cmr_cbr_block_bf16_f32" if mode == "bf16" else "cmr_cbr_block_f32", p(x1), x1.stride(0), c.k1, p(x2), x2.stride(0), p(idx), 1,
                  kx, ch, co, p(w1), p(b1), b1.stride(0), p(w2), p(b2), b2.stride(0), p(wsc), p(y), ybuf.stride(0), p(pbuf), rows, c.rpb,
                  float(c.slope), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ref = check_rows(c, y, mode, stat, "%s strided y %s" % (inst, kind))
        check_rows(c, pbuf[:nt], mode, stat, "%s partial-tile maxima %s" % (inst, kind), ref=ref, reduce=R.tile_max)
        assert torch.equal(pbuf[:nt].cpu(), R.tile_max(y.cpu()))
        guard = torch.ones_like(ybuf, dtype=torch.bool)
        guard[:rows, 4:4 + co] = False
        assert bool(torch.isnan(ybuf[guard]).all()) and not bool(torch.isnan(y).any())
        assert bool(torch.isnan(pbuf[nt]).all())
    report("block guards", stat)


# ------------------------------------------------------------------------------------------------------------------ the glue
def _glue(c, want_g=True):
    from cmr_agent_amd import ops
    return ops.colmax_bias2(dev(c.part), c.B, c.tpb, dev(c.w1), dev(c.b1), dev(c.w2), dev(c.b2), want_g=want_g)


@pytest.mark.parametrize("widths", R.GLUE_WIDTHS, ids=lambda w: "%dx%d" % w)
def test_glue_launch(widths):
    """cmr_colmax_bias2_f32 against float64 and against the three launches it replaces."""
    from cmr_agent_amd import ops
    n1, n2 = widths
    stat = []
    for B, tpb, kind, variant in R.glue_table():
        if kind == "exact":
            c = R.glue_case(B, tpb, n1, n2, variant=variant)
            y1, y2, g = _glue(c)
            want = R.glue_ref(c)
            g3 = ops.colmax_partials(dev(c.part), c.B, tpb)
            three = (g3, ops.linear(g3, dev(c.w1), dev(c.b1)), ops.linear(g3, dev(c.w2), dev(c.b2)))
            for got, w, t3, name in zip((g, y1, y2), want, three, ("g", "row 1", "row 2")):
                ok, msg = R.close_exact(got, w, "glue %s tiles %d %s" % (name, tpb, variant))
                assert ok, msg
                assert torch.equal(got, t3), (name, tpb)
            a1, a2, none = _glue(c, want_g=False)
            assert none is None and torch.equal(a1, y1) and torch.equal(a2, y2)
        else:
            c = R.glue_case(B, tpb, n1, n2, kind="real", variant=variant)
            y1, y2, g = _glue(c)
            wg, w1, w2, e1, e2 = R.glue_ref(c, g_err=torch.zeros((B, 64), dtype=F64))
            assert torch.equal(g.cpu().to(F64), wg)                # the maximum is exact
            for got, w, e in ((y1, w1, e1), (y2, w2, e2)):
                ok, worst, msg = R.close_bounded(got, w, e, 2.0, "glue tiles %d %s" % (tpb, variant))
                stat.append(worst)
                assert ok, msg
            g3 = ops.colmax_partials(dev(c.part), c.B, tpb)
            for got, w, e in ((ops.linear(g3, dev(c.w1), dev(c.b1)), w1, e1), (ops.linear(g3, dev(c.w2), dev(c.b2)), w2, e2)):
                ok, worst, msg = R.close_bounded(got, w, e, 2.0, "three launches tiles %d" % tpb)
                stat.append(worst)
                assert ok, msg
    report("glue %dx%d" % widths, stat)


def test_glue_launch_declines_what_it_does_not_serve():
    from cmr_agent_amd import _lib, ops
    c = R.glue_case(2, 3, 128, 64)
    part128 = torch.zeros((6, 128), dtype=F32, device=DEV)
    assert ops.colmax_bias2(part128, 2, 3, dev(c.w1), dev(c.b1), dev(c.w2), dev(c.b2)) is None
    w6, b6 = torch.zeros((6, 64), dtype=F32, device=DEV), torch.zeros((6,), dtype=F32, device=DEV)
    assert ops.colmax_bias2(dev(c.part), 2, 3, w6, b6, dev(c.w2), dev(c.b2)) is None
    assert ops.colmax_bias2(dev(c.part), 2, 3, dev(c.w1), dev(c.b1), w6, b6) is None
    p = lambda t: t.data_ptr()
    part, w1, b1, w2, b2 = dev(c.part), dev(c.w1), dev(c.b1), dev(c.w2), dev(c.b2)
    y1, y2 = torch.full((2, 128), NAN, dtype=F32, device=DEV), torch.full((2, 64), NAN, dtype=F32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for C, a, na, b, nb in ((128, w1, 128, w2, 64), (64, w6, 6, w2, 64), (64, w1, 128, w6, 6)):
        rc = _lib.call("cmr_colmax_bias2_f32", p(part128 if C == 128 else part), 2, 3, C, p(a), p(b1), na, p(b), p(b2), nb, None, p(y1), p(y2), s,
                       allow_unsupported=True)
        assert rc == _lib.UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(y1).all()) and bool(torch.isnan(y2).all())


# ------------------------------------------------------------------------------------------------------------------ the 3-D branch
def _agent_with(c):
    """a CMRAgent whose state_3d_embed holds the case's weights, BatchNorm at the identity (eps = 0, unit variance: the fold is exact)"""
    from cmr_agent_amd.config import KittiConfiguration
    from cmr_agent_amd.models import CMRAgent
    cfg = KittiConfiguration(cropped_img_H=96, cropped_img_W=160, num_pt=1024, device=DEV)
    torch.manual_seed(3)
    agent = CMRAgent(cfg)
    with torch.no_grad():
        for m, (w1, b1, w2, b2, sc) in zip(agent.state_3d_embed, c.blocks):
            pairs = [(m.net[0], m.net[1], w1, b1), (m.net[3], m.net[4], w2, b2)]
            if sc is not None:
                pairs.append((m.shortcut[0], m.shortcut[1], sc[0], sc[1]))
            for conv, bn, w, b in pairs:
                conv.weight.copy_(w.unsqueeze(-1))
                conv.bias.copy_(b)
                bn.weight.fill_(1.0)
                bn.bias.zero_()
                bn.running_mean.zero_()
                bn.running_var.fill_(1.0)
                bn.eps = 0.0
    return agent.to(DEV).eval()


@pytest.mark.parametrize("B,N,fused", R.CHAIN_SHAPES)
def test_branch_through_the_agent(B, N, fused, mode, monkeypatch):
    """CMRAgent._embed_3d_any on the fused chain and on the fallback chain it takes when the fused one declines (N % 32 != 0, more than 16
    samples).  The branch passes the module's slope 0.2, which is no power of two: for the exact chain the slope ARGUMENT is replaced by
    1/2 where the branch hands it to ops; the real-valued chain runs untouched."""
    from cmr_agent_amd import ops
    from cmr_agent_amd.models.PointNN import ConvBNReLURes1D

    def rows_of(c):
        x = torch.zeros((B * N, 8), dtype=F32)
        x[:, :5] = c.x.reshape(B * N, 5)
        return x.to(DEV)
    c = R.chain_case(B, N, kind="real")
    agent = _agent_with(c)
    got = agent._embed_3d_any(rows_of(c), B, N)
    assert (agent._embed_3d(rows_of(c), B, N) is not None) == fused
    want = R.chain_ref(c)
    scale = float(want.abs().max())
    err = float((got.cpu().to(F64) - want).abs().max())
    bar = 1e-4 * scale if mode == "f32" else 2e-2 * max(1.0, scale)         # test_ops_gpu.py's fp32 convention; test_bf16_gpu.py's bar
    print("  branch B %d N %d %s: error %.3g of the output scale (bar %.0e)" % (B, N, mode, err / scale, bar / scale))
    assert got.shape == (B, 128) and err <= bar
    if mode == "bf16":
        return
    c = R.chain_case(B, N, kind="exact")
    agent = _agent_with(c)
    block = ops.cbr_block
    half = lambda s: 0.5 if s == 0.2 else s
    monkeypatch.setattr(ConvBNReLURes1D, "SLOPE", 0.5)
    monkeypatch.setattr(ops, "cbr_block", lambda x1, w1, b1, w2, b2, wsc, slope, **kw: block(x1, w1, b1, w2, b2, wsc, half(slope), **kw))
    got = agent._embed_3d_any(rows_of(c), B, N)
    assert (agent._embed_3d(rows_of(c), B, N) is not None) == fused
    ok, msg = R.close_exact(got, R.chain_ref(c), "exact branch B %d N %d" % (B, N))
    assert ok, msg


# ------------------------------------------------------------------------------------------------------------------ the tail
def _pad4(w, b):
    n = w.shape[0]
    npad = (n + 3) // 4 * 4
    if npad == n:
        return w, b
    return torch.cat([w, torch.zeros((npad - n, w.shape[1]), dtype=w.dtype)]), torch.cat([b, torch.zeros((npad - n,), dtype=b.dtype)])


def _tail_args(c, transposed):
    pair = lambda wb: (dev(wb[0]), dev(wb[1]))
    tr = lambda wb: (lambda w, b: (dev(w.t().contiguous()), dev(b)))(*_pad4(*wb))       # W^T [in, out4], bias [out4]
    f = tr if transposed else pair
    return f(c.c24), f(c.c26), [[f(l) for l in head] for head in c.heads]


def _run_tail(c, kernel):
    from cmr_agent_amd import ops
    c24, c26, heads = _tail_args(c, kernel == "t")
    fn = ops.agent_heads_t if kernel == "t" else ops.agent_heads
    outs, acts = fn(dev(c.x), c.B, c.npix, c24, c26, dev(c.e3d), heads, c.slope, actions=(c.S, c.dr, c.dt))
    widths = [h[2][0].shape[0] for h in c.heads]
    return [o[:, :n] for o, n in zip(outs, widths)], acts


def _check_tail(c, ref, outs, acts, stat, what):
    for i, (o, (_, _, lg)) in enumerate(zip(outs, ref.heads)):
        if c.kind == "exact":
            ok, msg = R.close_exact(o, lg, "%s head %d" % (what, i))
            assert ok, msg
        else:
            ok, worst, msg = R.close_bounded(o, lg, ref.e_logits[i], 2.0, "%s head %d" % (what, i))
            stat.append(worst)
            assert ok, msg
    for i, d in ((0, c.dr), (1, c.dt)):
        a = acts[i].cpu()
        assert a.shape == (c.B, d) and a.dtype == torch.int64
        if c.kind == "exact":
            assert torch.equal(a, ref.acts[i]), what
        else:
            keep = R.compared_groups(ref.heads[i][2], 2.0 * ref.e_logits[i], d, c.S)
            assert float(keep.double().mean()) >= 0.95 and torch.equal(a[keep], ref.acts[i][keep]), what


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("widths", list(R.TAIL_WIDTHS))
def test_tail_kernels(widths, kind):
    """cmr_agent_heads_f32 and cmr_agent_heads_t_f32 over the pooling lengths around their unroll edges, B = 1 and 3: logits and actions
    against float64, and against each other."""
    from cmr_agent_amd import _lib
    served_t = R.TAIL_WIDTHS[widths][4]
    stat = []
    for B, npix, variant in R.tail_table(kind):
        c = R.tail_case(B, npix, widths, kind=kind, variant=variant, seed=R.REAL_SEED)
        ref = R.tail_ref(c, bounds=(kind == "real"))
        outs, acts = _run_tail(c, "rows")
        _check_tail(c, ref, outs, acts, stat, "%s B %d npix %d row-per-wave" % (widths, B, npix))
        if not served_t:
            if npix == 1:                                     # hidden widths that are no multiple of 16: refused before any launch
                with pytest.raises(_lib.CmrError):
                    _run_tail(c, "t")
            continue
        outs_t, acts_t = _run_tail(c, "t")
        _check_tail(c, ref, outs_t, acts_t, stat, "%s B %d npix %d transposed" % (widths, B, npix))
        for i, d in ((0, c.dr), (1, c.dt)):
            if kind == "exact":
                assert torch.equal(outs[i], outs_t[i]) and torch.equal(acts[i], acts_t[i])
            else:
                ok, worst, msg = R.close_bounded(outs_t[i], outs[i].cpu().to(F64), ref.e_logits[i], 2.0, "the two kernels")
                assert ok, msg
                keep = R.compared_groups(ref.heads[i][2], 2.0 * ref.e_logits[i], d, c.S)
                assert torch.equal(acts[i].cpu()[keep], acts_t[i].cpu()[keep])
    report("tail %s %s" % (widths, kind), stat)


def test_tail_planted_ties_and_a_large_mean():
    stat = []
    for kernel in ("rows", "t"):
        c = R.tail_case(3, 33, "product", variant="ties")
        ref = R.tail_ref(c)
        outs, acts = _run_tail(c, kernel)
        _check_tail(c, ref, outs, acts, stat, "ties %s" % kernel)
        assert bool((acts[0] == 1).all()) and bool((acts[1] == 1).all())          # equal maxima at 1 and S - 1: the first one wins
        c = R.tail_case(3, 33, "product", kind="real", variant="mean1000", seed=R.REAL_SEED)
        ref = R.tail_ref(c, bounds=True)
        outs, acts = _run_tail(c, kernel)
        _check_tail(c, ref, outs, acts, stat, "mean 1000 %s" % kernel)
    report("tail mean 1000", stat)


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("widths", list(R.TAIL_WIDTHS))
def test_tail_training_forward_saves(widths, kind):
    """cmr_agent_heads_train_f32: the logits and every intermediate it saves (pooled, t1, e2d, h0 / h1 of the three heads)."""
    from cmr_agent_amd import ops
    stat = []
    for B, npix, variant in R.tail_table(kind):
        c = R.tail_case(B, npix, widths, kind=kind, variant=variant, seed=R.REAL_SEED)
        ref = R.tail_ref(c, bounds=(kind == "real"))
        c24, c26, heads = _tail_args(c, False)
        r = ops.agent_heads_train(dev(c.x), B, npix, c24, c26, dev(c.e3d), heads, c.slope)
        assert r is not None
        outs, pooled, t1, e2d, hid = r
        got = [pooled, t1, e2d] + [t for pair in hid for t in pair] + list(outs)
        want = [ref.pooled, ref.t1, ref.e2d] + [t for h in ref.heads for t in h[:2]] + [h[2] for h in ref.heads]
        if kind == "exact":
            for g, w in zip(got, want):
                ok, msg = R.close_exact(g, w, "train saves %s B %d npix %d" % (widths, B, npix))
                assert ok, msg
        else:
            bounds = list(ref.e_saves[:3]) + [t for pair in ref.e_saves[3] for t in pair] + list(ref.e_logits)
            for g, w, e in zip(got, want, bounds):
                ok, worst, msg = R.close_bounded(g, w, e, 2.0, "train saves %s B %d npix %d" % (widths, B, npix))
                stat.append(worst)
                assert ok, msg
    report("tail training forward %s" % widths, stat)


@pytest.mark.parametrize("kernel", ["rows", "t"])
def test_tail_outputs_keep_their_guards(kernel):
    """logit rows with ldo > n2 (through the C entry points): the columns past n2 stay NaN."""
    from cmr_agent_amd import _lib
    c = R.tail_case(3, 33, "product")
    ref = R.tail_ref(c)
    c24, c26, heads = _tail_args(c, kernel == "t")
    p = lambda t: t.data_ptr()
    outs, args = [], []
    for (w0, b0), (w1, b1), (w2, b2) in heads:
        n0, n1, n2 = (w0.shape[1], w1.shape[1], w2.shape[1]) if kernel == "t" else (w0.shape[0], w1.shape[0], w2.shape[0])
        o = torch.full((c.B, n2 + 4), NAN, dtype=F32, device=DEV)
        outs.append((o, n2))
        args += [p(w0), p(b0), p(w1), p(b1), p(w2), p(b2), n0, n1, n2, p(o), o.stride(0)]
    ar = torch.empty((c.B, c.dr), dtype=torch.int64, device=DEV)
    at = torch.empty((c.B, c.dt), dtype=torch.int64, device=DEV)
    x, e3d = dev(c.x), dev(c.e3d)
    _lib.call("cmr_agent_heads_t_f32" if kernel == "t" else "cmr_agent_heads_f32", p(x), c.B, c.npix, p(c24[0]), p(c24[1]), p(c26[0]), p(c26[1]), p(e3d),
              *args, c.S, c.dr, c.dt, p(ar), p(at), float(c.slope), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for (o, n2), (_, _, lg) in zip(outs, ref.heads):
        ok, msg = R.close_exact(o[:, :lg.shape[1]], lg, "strided logits")
        assert ok, msg
        assert bool(torch.isnan(o[:, n2:]).all())
    assert torch.equal(ar.cpu(), ref.acts[0]) and torch.equal(at.cpu(), ref.acts[1])
