"""GPU tier of the fp32 3x3 convolution kernels (csrc/conv.hip, conv_wino.hip, conv_s2.hip, the convolution half of wgrad.hip and
wgrad_wino.hip), case by case against the float64 restatement in conv_reference.py.

On the integer cases every kernel must equal float64 EXACTLY (torch.equal, no tolerance): tests/test_conv_cpu.py shows on the same
inputs that fp32 holds every intermediate, so the summation order of a kernel cannot matter and any difference is a wrong tap, a
dropped channel group, a pixel of the neighbouring image, a stale halo or a mishandled border.  The entry points are called directly,
so the kernel of a case is the one conv_reference.expected_kernel names; every output buffer is filled with NaN first, so a pixel that
is never written shows.  One real-valued case per kernel is held to the per-element rounding bar that the CPU tier derives."""
import functools

import pytest
import torch

import conv_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
FWD = list(enumerate(R.forward_rows()))
_fid = lambda v: R.row_id(v[1])


@pytest.fixture(scope="module")
def ops():
    from cmr_agent_amd import ops as _ops
    return _ops


def _lib():
    from cmr_agent_amd import _lib as lib
    return lib


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def raw(name, *args):
    """status of an entry point, without the wrapper's exception"""
    return getattr(_lib().load(), name)(*args)


def _out_shape(c):
    B, H, W, _ = c.x.shape
    ho, wo = R.out_size(H, c.stride), R.out_size(W, c.stride)
    return (B, ho // 2, wo // 2, c.w.shape[0]) if c.pool == 2 else (B, ho, wo, c.w.shape[0])


class Operands:
    """device copies of a case and the packed weights of every entry point (host packers: _pack.winograd_u / conv_s2_frags)"""

    def __init__(self, c):
        from cmr_agent_amd.models import _pack
        self.c = c
        self.x, self.bias, self.res, self.post = dev(c.x), dev(c.bias), dev(c.res), dev(c.post)
        self.cout, self.cin = c.w.shape[0], c.w.shape[1]
        self.w9 = dev(R.w9_of(c.w))
        self.u = dev(_pack.winograd_u(c.w)) if c.stride == 1 else None
        fr = _pack.conv_s2_frags(c.w) if c.stride == 2 else None
        self.s2 = dev(fr)
        self.s2_any = dev(torch.stack([_pack.frag_pack(c.w[:, :, t // 3, t % 3].contiguous()) for t in range(9)])) if c.stride == 2 else None


def call_conv(o, slope=None):
    c = o.c
    B, H, W, _ = c.x.shape
    y = nans(*_out_shape(c))
    rc = raw("cmr_conv3x3_nhwc_f32", _p(o.x), B, H, W, o.cin, _p(o.w9), _p(o.bias), _p(o.res), _p(o.post), _p(y), o.cout, c.stride,
             float(c.slope if slope is None else slope), c.pool, _stream())
    return rc, y


def call_wino(o, budget=0, slices=1, slope=None):
    c = o.c
    B, H, W, _ = c.x.shape
    y = nans(*_out_shape(c))
    rc = raw("cmr_conv3x3_wino_nhwc_f32", _p(o.x), B, H, W, o.cin, _p(o.u), _p(o.bias), _p(o.res), _p(o.post), _p(y), o.cout,
             float(c.slope if slope is None else slope), c.pool, budget, slices, _stream())
    return rc, y


def call_s2(o, slope=None):
    c = o.c
    B, H, W, _ = c.x.shape
    y = nans(*_out_shape(c))
    rc = raw("cmr_conv3x3_s2_nhwc_f32", _p(o.x), B, H, W, o.cin, _p(o.s2_any), _p(o.bias), _p(o.res), _p(o.post), _p(y), o.cout,
             float(c.slope if slope is None else slope), _stream())
    return rc, y


CALL = {"conv": call_conv, "wino": call_wino, "s2": call_s2}


def reference(c, slope=None):
    ref = R.conv3x3_ref(c.x, c.w, c.bias, c.stride, c.slope if slope is None else slope, c.res, c.post, c.pool)
    r32 = ref.float()
    assert torch.equal(r32.double(), ref)           # the expected values are fp32 numbers
    return r32.to(DEV)


@functools.lru_cache(maxsize=None)
def _prepared(i, impulse):
    """(operands, reference on the device) of forward row i -- built once, shared by the tests that use the row, never written to"""
    c = R.row_case(i, FWD[i][1], impulse)
    return Operands(c), reference(c)


def exact(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = (got != ref) | torch.isnan(got)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d elements differ (%d NaN = never written); first at %s: got %r, want %r" % (
            what, int(bad.sum()), got.numel(), int(torch.isnan(got).sum()), idx, float(got[tuple(idx)]), float(ref[tuple(idx)])))


# ---- forward, integer cases and impulse scenes: exact -----------------------------------------------------------------------------
@pytest.mark.parametrize("impulse", [False, True], ids=["integers", "impulses"])
@pytest.mark.parametrize("ir", FWD, ids=_fid)
def test_forward_is_exact(ops, ir, impulse):
    i, r = ir
    o, ref = _prepared(i, impulse)
    B, H, W, cin, cout = r.shape
    assert R.expected_kernel(r.entry, B, H, W, cin, cout, r.stride, r.pool, o.c.slope, o.c.res is not None, o.c.post is not None) == r.kernel
    if r.kernel == R.UNSUPPORTED:
        rc, y = CALL[r.entry](o)
        assert rc == _lib().UNSUPPORTED and bool(torch.isnan(y).all()), "a refused call must not touch the output"
        if r.entry == "conv":                            # ... and ops.conv3x3 pools separately
            exact(ops.conv3x3(o.x, o.w9, o.bias, cout, 1, o.c.slope, pool=2), ref, "ops.conv3x3 after the refusal")
        else:                                            # ... and ops.conv3x3 goes to the tiled kernel
            u = o.s2_any
            u.s2 = o.s2_any                               # offered to the fragment kernel, which declines Cin = 32
            exact(ops.conv3x3(o.x, o.w9, o.bias, cout, 2, o.c.slope, res=o.res, u=u), ref, "ops.conv3x3 after the refusal")
        return
    if r.kernel != "wino_ws":
        rc, y = CALL[r.entry](o)
        assert rc == 0
        exact(y, ref, r.kernel)
        return
    for budget in R.WS_BUDGETS:
        for slices in R.WS_SLICES:
            rc, y = call_wino(o, budget, slices)
            assert rc == 0
            exact(y, ref, "wino_ws cu_budget %d slices %d" % (budget, slices))
    with ops.conv_cu_budget(8), ops.conv_slices(2):      # the launch policy as the model sets it
        exact(ops.conv3x3_wino(o.x, o.u, o.bias, cout, o.c.slope, o.res, o.post, o.c.pool), ref, "ops.conv3x3_wino under the policy")


def test_stride2_fragment_kernel_refuses_a_table(ops):
    i = next(i for i, r in FWD if r.entry == "s2" and r.shape == (2, 7, 9, 64, 64))
    o, _ = _prepared(i, False)
    B, H, W, _ = o.c.x.shape
    y = nans(*_out_shape(o.c))
    post = torch.zeros(y.shape[1:], device=DEV)
    rc = raw("cmr_conv3x3_s2_nhwc_f32", _p(o.x), B, H, W, 64, _p(o.s2), _p(o.bias), _p(o.res), _p(post), _p(y), 64, 1.0, _stream())
    assert rc == _lib().UNSUPPORTED and bool(torch.isnan(y).all())


@pytest.mark.parametrize("shape,stride,pool,have_u", R.OPS_ROUTES, ids=str)
def test_ops_conv3x3_routes_are_exact(ops, shape, stride, pool, have_u):
    """one pass through ops.conv3x3 per route, with u and u.s2 as _pack.conv9 builds them"""
    from cmr_agent_amd.models import _pack
    B, H, W, cin, cout = shape
    entry, kernel, _ = R.ops_route(ops, B, H, W, cin, cout, stride, pool, False, have_u, True)
    c = R.integer_case(sum(shape), B, H, W, cin, cout, stride, slope=0.25, bias=True, res=pool == 1, pool=pool)
    conv = torch.nn.Conv2d(cin, cout, 3, stride, 1)
    with torch.no_grad():
        conv.weight.copy_(c.w)
        conv.bias.copy_(c.bias)
    with torch.no_grad():
        w9, b, u = _pack.conv9(conv)
    assert torch.equal(w9, R.w9_of(c.w)) and (u.s2 is not None) == (stride == 2 and cin == 64)
    ud = dev(u)
    ud.s2, ud.bf16 = dev(u.s2), None
    got = ops.conv3x3(dev(c.x), dev(w9), dev(b), cout, stride, c.slope, res=dev(c.res), pool=pool, u=ud if have_u else None)
    exact(got, reference(c), "ops.conv3x3 -> %s %s" % (entry, kernel))
    if stride == 2 and cin == 64:                        # the same layer on the tiled kernel
        old = ops.STRIDE2_FRAGS
        try:
            ops.STRIDE2_FRAGS = False
            exact(ops.conv3x3(dev(c.x), dev(w9), dev(b), cout, 2, c.slope, res=dev(c.res), u=ud), reference(c), "STRIDE2_FRAGS off")
        finally:
            ops.STRIDE2_FRAGS = old


# ---- slope outside [0, 1] -----------------------------------------------------------------------------------------------------------
SLOPE_ROWS = [("conv", (2, 5, 7, 128, 128), 1), ("conv", (1, 63, 131, 32, 128), 1), ("conv", (4, 33, 400, 32, 64), 1), ("conv", (2, 7, 9, 32, 64), 2),
              ("s2", (2, 7, 9, 64, 64), 2), ("wino", (2, 7, 15, 128, 128), 1), ("wino", (2, 57, 497, 64, 64), 1), ("wino", (3, 41, 183, 64, 64), 1)]


@pytest.mark.parametrize("slope", [2.0, -0.5])
@pytest.mark.parametrize("entry,shape,stride", SLOPE_ROWS, ids=str)
def test_slope_outside_the_unit_interval_is_a_select(ops, entry, shape, stride, slope):
    """v > 0 ? v : slope v, exactly, on every entry point: the wave-specialised kernel's max(v, slope v) must not be reached"""
    B, H, W, cin, cout = shape
    k = R.expected_kernel(entry, B, H, W, cin, cout, stride, 1, slope)
    assert k != "wino_ws"
    c = R.integer_case(B + H + W, B, H, W, cin, cout, stride, slope=slope, bias=True, res=True, post=entry != "s2")
    assert R.exact_ok(c)
    o, ref = Operands(c), reference(c)
    assert bool((R.conv3x3_raw(c.x, c.w, stride) + c.bias.double() + c.res.double() < 0).any())
    rc, y = CALL[entry](o)
    assert rc == 0
    exact(y, ref, "%s at slope %g" % (k, slope))
    u = o.u if stride == 1 else o.s2_any
    if stride == 2:
        u.s2 = o.s2
    got = ops.conv3x3(o.x, o.w9, o.bias, cout, stride, slope, res=o.res, post=o.post, u=u)
    exact(got, ref, "ops.conv3x3 at slope %g" % slope)


# ---- stem --------------------------------------------------------------------------------------------------------------------------
def _stem_call(s, slope=None):
    B, _, H, W = s.x.shape
    tmp, y = nans(B, 6, H, W), nans(B, H, W, 64)
    args = [dev(s.x), dev(s.w_a), dev(s.b_a), dev(s.w3.reshape(64, 27).t()), dev(s.w1.t()), dev(s.b_b)]
    rc = raw("cmr_stem_block_f32", *[_p(a) for a in args], _p(tmp), _p(y), 0, B, H, W, float(s.slope if slope is None else slope), _stream())
    torch.cuda.synchronize()
    return rc, y, args


@pytest.mark.parametrize("impulse", [False, True], ids=["integers", "impulses"])
@pytest.mark.parametrize("i,shape", list(enumerate(R.STEM_SHAPES)), ids=str)
def test_stem_is_exact(ops, i, shape, impulse):
    s = R.stem_case(i, *shape, R.CASE_SLOPES[i % 3], impulse)
    ref = R.stem_ref(*s)
    rc, y, args = _stem_call(s)
    assert rc == 0
    exact(y, ref.float().to(DEV), "stem %s" % (shape,))
    assert torch.equal(ops.stem_block(*args, s.slope), y)


@pytest.mark.parametrize("slope", [2.0, -0.5])
def test_stem_refuses_a_slope_outside_the_unit_interval(ops, slope):
    """stem_b's max(v, slope v) is the select only for slope <= 1; the entry point admits 0 <= slope <= 1"""
    s = R.stem_case(0, 2, 5, 7, slope)
    rc, y, args = _stem_call(s)
    assert rc == -1 and bool(torch.isnan(y).all())
    with pytest.raises(_lib().CmrError):
        ops.stem_block(*args, slope)


# ---- packing -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("cout,cin", R.PACK_SHAPES)
def test_device_and_host_packers_agree(ops, cout, cin, transpose):
    from cmr_agent_amd.models import _pack
    w = torch.randint(-3, 4, (cout, cin, 3, 3), generator=torch.Generator().manual_seed(cout + cin)).float()
    wt = w.transpose(0, 1).flip(2, 3).contiguous() if transpose else w           # the data-gradient convolution's weights
    w9, u = ops.pack_conv3x3(dev(w).reshape(-1), cout, cin, transpose)
    co, ci = wt.shape[:2]
    assert torch.equal(w9.cpu(), R.w9_of(wt))
    assert torch.equal(u.cpu(), _pack.winograd_u(wt))
    assert torch.equal(R.unfragment(u.cpu(), co, ci).double(), R.winograd_u_ref(wt))
    conv = torch.nn.Conv2d(ci, co, 3, 1, 1)
    with torch.no_grad():
        conv.weight.copy_(wt)
        h9, _, hu = _pack.conv9(conv)
    assert torch.equal(h9, w9.cpu()) and torch.equal(hu, u.cpu())


# ---- statistics epilogue -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s in R.WS_SHAPES if s[4] == 64], ids=str)
def test_statistics_epilogue_counts_every_pixel_once(ops, shape):
    """With an impulse scene every non-zero output sits on a tile seam, a ragged border or an image boundary: the sums of (y - bias) and
    (y - bias)^2 over the helper waves' partials equal the reference EXACTLY, under every launch geometry -- a pixel counted twice, or
    not at all, shows as a whole number."""
    B, H, W, cin, cout = shape
    c = R.impulse_case(B, H, W, cin, cout, (8, 16), bias=True, amp=1)       # unit impulses: the sum of squares stays below 2^24
    o, ref = Operands(c), reference(c)
    want = R.stats_ref(ref.cpu(), c.bias)
    assert float(want[1].max()) < R.LIMIT and float(want[0].abs().max()) > 0
    rc, plain = call_wino(o)
    assert rc == 0
    exact(plain, ref, "wino_ws")
    for budget in R.WS_BUDGETS:
        for slices in R.WS_SLICES:
            with ops.conv_cu_budget(budget), ops.conv_slices(slices):
                y, part = ops.conv3x3_wino_stats(o.x, o.u, o.bias, cout)
            assert torch.equal(y, plain), "statistics launch: y differs from the plain entry point's (cu_budget %d slices %d)" % (budget, slices)
            got = part.double().sum(0).cpu()
            assert torch.equal(got, want), "cu_budget %d slices %d: sums off by %s" % (budget, slices, (got - want).abs().max())
    stat = ops.bn_stats_from_sums(part, B * H * W, o.bias, torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV))
    mean = ref.double().view(-1, cout).mean(0)
    assert float((stat[0].double() - mean).abs().max()) <= 1e-6 * float(mean.abs().max())


def test_statistics_epilogue_declines_small_maps(ops):
    c = R.impulse_case(1, 8, 3184, 64, 64, (8, 16), bias=True)      # 199 tiles
    o = Operands(c)
    assert ops.conv3x3_wino_stats(o.x, o.u, o.bias, 64) is None


# ---- weight gradients: exact --------------------------------------------------------------------------------------------------------
def _wgrad_call(name, x, dy, shape, ws_shape=None):
    B, H, W, cin, cout = shape
    lib = _lib().load()
    wb, wh, ww = ws_shape or (B, H, W)
    nb = int(getattr(lib, "cmr_conv3x3_wgrad_wino_workspace_bytes" if "wino" in name else "cmr_conv3x3_wgrad_workspace_bytes")(wb, wh, ww, cin, cout))
    ws = torch.empty((max(nb // 4, 1),), dtype=torch.float32, device=DEV)
    dw = nans(cout, cin, 3, 3)
    rc = raw(name, _p(x), _p(dy), B, H, W, cin, cout, _p(dw), _p(ws), nb, _stream())
    return rc, dw


def _wgrad_exact(dw, x, dy, stride, what):
    ref = R.wgrad_ref(x, dy, stride)
    r32 = ref.float()
    assert torch.equal(r32.double(), ref)
    exact(dw, r32.to(DEV), what)


@pytest.mark.parametrize("r", [r for r in R.cases() if r.entry == "wgrad"], ids=R.row_id)
def test_weight_gradient_is_exact(ops, r):
    B, H, W, cin, cout = r.shape
    wino = cin == 64 and cout == 64 and H % 2 == 0 and W % 2 == 0
    x, dy, _ = R.wgrad_case(B + H + W, B, H, W, cin, cout, winograd=wino)
    rc, dw = _wgrad_call("cmr_conv3x3_wgrad_f32", dev(x), dev(dy), r.shape)
    assert rc == 0
    _wgrad_exact(dw, x, dy, 1, r.kernel)
    for on in (True, False):                             # the dispatcher, Winograd-domain form on and off
        old = ops.WGRAD_WINO
        try:
            ops.WGRAD_WINO = on
            dw2 = nans(cout * cin * 9)
            ops.conv3x3_wgrad(dev(x), dev(dy), dw2)
        finally:
            ops.WGRAD_WINO = old
        _wgrad_exact(dw2.view(cout, cin, 3, 3), x, dy, 1, "ops.conv3x3_wgrad, WGRAD_WINO %s" % on)


@pytest.mark.parametrize("r", [r for r in R.cases() if r.entry == "wgrad_s2"], ids=R.row_id)
def test_stride2_weight_gradient_is_exact(ops, r):
    B, H, W, cin, cout = r.shape
    x, dy, _ = R.wgrad_case(B + H + W, B, H, W, cin, cout, stride=2)
    rc, dw = _wgrad_call("cmr_conv3x3_wgrad_s2_f32", dev(x), dev(dy), r.shape, (B, H // 2, W // 2))
    assert rc == 0
    _wgrad_exact(dw, x, dy, 2, r.kernel)
    dw2 = nans(cout * cin * 9)
    assert ops.conv3x3_wgrad_s2(dev(x), dev(dy), dw2)
    _wgrad_exact(dw2.view(cout, cin, 3, 3), x, dy, 2, "ops.conv3x3_wgrad_s2")


@pytest.mark.parametrize("r", [r for r in R.cases() if r.entry == "wgrad_wino"], ids=R.row_id)
def test_winograd_domain_weight_gradient_is_exact(ops, r):
    B, H, W, cin, cout = r.shape
    x, dy, _ = R.wgrad_case(B + H + W, B, H, W, cin, cout, winograd=True)
    rc, dw = _wgrad_call("cmr_conv3x3_wgrad_wino_f32", dev(x), dev(dy), r.shape)
    assert rc == 0
    _wgrad_exact(dw, x, dy, 1, r.kernel)


def test_weight_gradient_entries_refuse_what_they_do_not_serve(ops):
    x, dy = torch.ones(2, 6, 6, 64, device=DEV), torch.ones(2, 6, 6, 64, device=DEV)
    for name, shape, ws_shape, want in (("cmr_conv3x3_wgrad_f32", (2, 18, 1, 64, 64), None, -1),            # W < 2
                                        ("cmr_conv3x3_wgrad_s2_f32", (2, 6, 5, 64, 64), (2, 3, 3), -1),     # odd width
                                        ("cmr_conv3x3_wgrad_s2_f32", (2, 5, 6, 64, 64), (2, 3, 3), -1),     # odd height
                                        ("cmr_conv3x3_wgrad_wino_f32", (2, 6, 5, 64, 64), None, _lib().UNSUPPORTED),
                                        ("cmr_conv3x3_wgrad_wino_f32", (2, 5, 6, 64, 64), None, _lib().UNSUPPORTED),
                                        ("cmr_conv3x3_wgrad_wino_f32", (1, 6, 6, 32, 64), None, _lib().UNSUPPORTED)):
        rc, dw = _wgrad_call(name, x, dy, shape, ws_shape)
        assert rc == want and bool(torch.isnan(dw).all()), (name, shape, rc)
    assert not ops.conv3x3_wgrad_s2(x[:, :5].contiguous(), dy[:, :3, :3].contiguous(), nans(64 * 64 * 9))


# ---- rounding: one real-valued case per kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(R.ROUNDING_ROWS))
def test_rounding_stays_within_the_bar(ops, kernel):
    """per element |got - ref| / (sum |x||w| + |bias| + |res| + |post|) <= 4 x what fp32 F.conv2d (direct kernels) or the fp32 numpy
    Winograd (Winograd kernels) loses on the same inputs"""
    entry, shape, stride = R.ROUNDING_ROWS[kernel]
    c, ref, den, bar = R.rounding_case(kernel)
    o = Operands(c)
    if kernel == "wino_ws":
        errs = []
        for budget, slices in ((0, 1), (8, 1), (24, 3)):
            rc, y = call_wino(o, budget, slices)
            assert rc == 0
            errs.append(R.forward_error(y, ref, den))
        err = max(errs)
    else:
        rc, y = CALL[entry](o)
        assert rc == 0
        err = R.forward_error(y, ref, den)
    print("%-14s %-22s worst %.3e bar %.3e" % (kernel, shape, err, bar))
    assert err <= bar, "%s: per-element forward error %.3e above the bar %.3e" % (kernel, err, bar)
