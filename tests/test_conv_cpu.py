"""CPU tier of the fp32 3x3 convolution kernels: the premises that the GPU tier (tests/test_conv_gpu.py) relies on, asserted on the GPU
tier's own cases.  The float64 restatement in conv_reference.py agrees with float64 F.conv2d / autograd / the oracle's stem / the host
packer; every integer case is exact in fp32 BEFORE that is demanded of a kernel (fp32 F.conv2d and an fp32 numpy Winograd equal float64
bit for bit); the case table reaches every kernel instantiation on both sides of every threshold; and the rounding bars are computed
here from fp32 CPU evaluations of the same inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_reference as R
from oracle import cmr_oracle as O

F64, F32 = torch.float64, torch.float32
FWD = list(enumerate(R.forward_rows()))
WGRAD = [r for r in R.cases() if r.entry in ("wgrad", "wgrad_s2", "wgrad_wino")]
_fid = lambda v: R.row_id(v[1])


@pytest.fixture(autouse=True)
def _grad_enabled():
    """other test modules switch autograd off process-wide at import; the autograd references need it"""
    with torch.enable_grad():
        yield


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _torch_forward(c, dtype):
    """F.conv2d plus the same epilogue, in dtype."""
    y = F.conv2d(_nchw(c.x.to(dtype)), c.w.to(dtype), None, c.stride, 1).permute(0, 2, 3, 1)
    return R.epilogue(y, c.bias, c.slope, c.res, c.post, c.pool)


# ---- the reference agrees with what is already trusted ---------------------------------------------------------------------------
@pytest.mark.parametrize("ir", FWD, ids=_fid)
def test_reference_equals_float64_conv2d(ir):
    i, r = ir
    B, H, W, cin, cout = r.shape
    c = R.real_case(i, B, H, W, cin, cout, r.stride, res=r.pool == 1, post=r.pool == 1)._replace(pool=r.pool)
    ref = R.conv3x3_ref(c.x, c.w, c.bias, c.stride, c.slope, c.res, c.post, c.pool)
    want = _torch_forward(c, F64)
    assert ref.shape == want.shape
    assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("r", WGRAD, ids=R.row_id)
def test_wgrad_reference_equals_float64_autograd(r):
    B, H, W, cin, cout = r.shape
    g = torch.Generator().manual_seed(B * H * W + cin)
    x = torch.randn((B, H, W, cin), generator=g, dtype=F64)
    w = torch.zeros((cout, cin, 3, 3), dtype=F64, requires_grad=True)
    y = F.conv2d(_nchw(x), w, None, r.stride, 1)
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    (y * dy).sum().backward()
    got = (R.wgrad_s2_ref if r.stride == 2 else R.wgrad_ref)(x, dy.permute(0, 2, 3, 1))
    assert float((got - w.grad).abs().max()) <= 1e-12 * float(w.grad.abs().max())


@pytest.mark.parametrize("shape", R.STEM_SHAPES[:-1] + [(1, 19, 70)], ids=str)
@pytest.mark.parametrize("slope", [0.2, 2.0])
def test_stem_reference_equals_the_oracle(shape, slope):
    g = torch.Generator().manual_seed(sum(shape))
    rn = lambda *s: torch.randn(s, generator=g, dtype=F64)
    x, wa, ba, w3, w1, bb = rn(shape[0], 3, *shape[1:]), rn(3, 3, 3, 3), rn(3), rn(64, 3, 3, 3), rn(64, 3), rn(64)
    ident = lambda n, b: {"weight": torch.ones(n, dtype=F64), "bias": b, "running_mean": torch.zeros(n, dtype=F64),
                          "running_var": torch.full((n,), 1.0 - O.BN_EPS, dtype=F64)}
    sd = {"conv_layers.0.weight": wa, "conv_layers.3.weight": w3, "shortcut.0.weight": w1.view(64, 3, 1, 1)}
    for name, bn in (("conv_layers.1", ident(3, ba)), ("conv_layers.4", ident(64, bb)), ("shortcut.1", ident(64, torch.zeros(64, dtype=F64)))):
        sd.update({name + "." + k: v for k, v in bn.items()})
    want = O.residual_block(O.Weights(sd), x, 1, slope).permute(0, 2, 3, 1)
    got = R.stem_ref(x, wa, ba, w3, w1, bb, slope)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("co,ci", R.PACK_SHAPES)
def test_winograd_u_reference_equals_the_host_packer(co, ci):
    from cmr_agent_amd.models import _pack
    w = torch.randint(-3, 4, (co, ci, 3, 3), generator=torch.Generator().manual_seed(co + ci)).float()
    ref = R.winograd_u_ref(w)
    got = R.unfragment(_pack.winograd_u(w), co, ci)
    assert got.dtype == F32 and torch.equal(got.double(), ref)
    # the permutation is a bijection: fragmenting the reference gives the packed tensor back
    again = ref.float().reshape(16, co // 32, 32, ci // 8, 2, 4).permute(0, 1, 3, 4, 2, 5).reshape(16, co, ci)
    assert torch.equal(again, _pack.winograd_u(w))
    # frag_pack of every tap (the stride-2 kernel's operand) is the same permutation
    if ci == 64 and co % 64 == 0:
        assert torch.equal(R.unfragment(_pack.conv_s2_frags(w), co, ci), R.w9_of(w))


# ---- exactness holds before it is demanded of a kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("impulse", [False, True], ids=["integers", "impulses"])
@pytest.mark.parametrize("ir", FWD, ids=_fid)
def test_integer_cases_are_exact_in_fp32(ir, impulse):
    i, r = ir
    c = R.row_case(i, r, impulse)
    assert R.exact_ok(c)
    ref = R.conv3x3_ref(c.x, c.w, c.bias, c.stride, c.slope, c.res, c.post, c.pool)
    assert torch.equal(_torch_forward(c, F32).double(), ref), "fp32 F.conv2d is not exact: the case is wrong"
    if c.stride == 1:
        order = np.random.default_rng(i).permutation(c.x.shape[3])
        got = R.epilogue(R.wino_fp32(c.x, c.w, order), c.bias, c.slope, c.res, c.post, c.pool)
        assert got.dtype == F32 and torch.equal(got.double(), ref), "the fp32 Winograd is not exact: the case is wrong"
    if impulse:      # the scene can tell the taps and the channels apart: flipped, transposed or permuted weights change the answer
        wrongs = [c.w.roll(1, 1), c.w.roll(1, 0)]
        if min(c.x.shape[1:3]) >= 3:
            wrongs += [c.w.flip(2), c.w.flip(3), c.w.transpose(2, 3)]
        for wrong in wrongs:
            assert not torch.equal(R.conv3x3_ref(c.x, wrong, c.bias, c.stride, c.slope, c.res, c.post, c.pool), ref)


def test_every_slope_of_the_builder_is_exact():
    for seed, slope in enumerate(R.SLOPES + (-0.5,)):
        c = R.integer_case(seed, 2, 9, 13, 128, 64, slope=slope, res=True, post=True)
        assert R.exact_ok(c) and c.slope == slope
        ref = R.conv3x3_ref(c.x, c.w, c.bias, 1, c.slope, c.res, c.post)
        assert torch.equal(_torch_forward(c, F32).double(), ref)
        assert torch.equal(R.epilogue(R.wino_fp32(c.x, c.w), c.bias, c.slope, c.res, c.post).double(), ref)
    # select and max semantics differ above 1 (and agree at or below it) -- what the slope-2 cases of the GPU tier tell apart
    v = torch.tensor([-3.0, 2.0], dtype=F64)
    assert not torch.equal(R.lrelu_select(v, 2.0), torch.maximum(v, 2.0 * v))
    assert torch.equal(R.lrelu_select(v, -0.5), torch.maximum(v, -0.5 * v))
    assert torch.equal(R.lrelu_select(v, 0.25), torch.maximum(v, 0.25 * v))


def test_exact_ok_rejects_a_case_that_is_too_large():
    c = R.integer_case(0, 1, 8, 16, 128, 64, slope=0.25, pool=2)
    big = c._replace(x=c.x * 2.0 ** 14)
    assert R.exact_ok(c) and not R.exact_ok(big)


@pytest.mark.parametrize("r", WGRAD, ids=R.row_id)
def test_weight_gradient_cases_are_exact_in_fp32(r):
    B, H, W, cin, cout = r.shape
    wino = r.entry == "wgrad_wino" or (r.entry == "wgrad" and cin == 64 and cout == 64 and H % 2 == 0 and W % 2 == 0)
    x, dy, rng = R.wgrad_case(B + H + W, B, H, W, cin, cout, r.stride, winograd=wino)
    assert rng >= 1 and R.wgrad_bound(dy.numel() // cout, rng, rng, wino) < R.LIMIT
    ref = R.wgrad_ref(x, dy, r.stride)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    ho, wo, s = dy.shape[1], dy.shape[2], r.stride
    got = torch.stack([torch.stack([dy.reshape(-1, cout).t() @ xp[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s].reshape(-1, cin)
                                    for kx in range(3)], -1) for ky in range(3)], -2)
    assert got.dtype == F32 and torch.equal(got.double(), ref)


def test_the_winograd_weight_gradient_range_is_shrunk():
    """the largest map leaves less room in the Winograd domain than the builder's default range"""
    assert R.wgrad_case(0, 2, 96, 128, 64, 64, winograd=True)[2] < R.wgrad_case(0, 2, 96, 128, 64, 64, winograd=False)[2]


@pytest.mark.parametrize("impulse", [False, True])
@pytest.mark.parametrize("i,shape", list(enumerate(R.STEM_SHAPES)), ids=str)
def test_stem_cases_are_exact_in_fp32(i, shape, impulse):
    s = R.stem_case(i, *shape, R.CASE_SLOPES[i % 3], impulse)
    assert R.stem_bound(s) < R.LIMIT
    ref = R.stem_ref(*s)
    x = s.x
    t = F.leaky_relu(F.conv2d(x, s.w_a, s.b_a, 1, 1), s.slope)
    y = F.leaky_relu(F.conv2d(t, s.w3, None, 1, 1) + F.conv2d(x, s.w1.view(64, 3, 1, 1)) + s.b_b.view(1, -1, 1, 1), s.slope)
    assert y.dtype == F32 and torch.equal(y.permute(0, 2, 3, 1).double(), ref)


# ---- every kernel is covered --------------------------------------------------------------------------------------------------
def test_every_kernel_instantiation_is_reached():
    reached = {r.kernel for r in R.cases()}
    named = {"direct<1>", "direct<2>", "tiled<1,2,32>", "tiled<2,1,16>", "s2<4>", "wino<1>", "wino<2>", "wino_ws", "wgrad<1>", "wgrad<2>",
             "wgrad<4>", "wgrad_lds<2>", "wgrad_lds<4>", "wgrad_s2<1>", "wgrad_s2<2>", "wgrad_s2<4>", "wgrad_wino"}
    assert named == set(R.FORWARD_KERNELS) | set(R.WGRAD_KERNELS)
    assert named <= reached, named - reached
    assert R.UNSUPPORTED in reached and R.INVALID not in reached
    # the impulse scenes know the tile of every forward kernel
    assert set(R.TILE) == set(R.FORWARD_KERNELS)


def test_every_forward_kernel_sees_every_epilogue_operand():
    """per kernel: bias, residual, table (where the entry point takes one), a slope other than 1 next to a residual, and -- where the
    kernel pools -- the pool behind a slope other than 1 (LeakyReLU at slope 1 commutes with everything)"""
    seen = {k: set() for k in R.FORWARD_KERNELS}
    for i, r in FWD:
        if r.kernel in seen:
            c = R.row_case(i, r)
            seen[r.kernel].add((c.slope, c.bias is not None, c.res is not None, c.post is not None, c.pool))
    for k, v in seen.items():
        assert any(b for _, b, _, _, _ in v) and any(rs and s != 1.0 for s, _, rs, _, _ in v), k
        assert k == "s2<4>" or any(p and s != 1.0 for s, _, _, p, _ in v), k
        if k in ("tiled<1,2,32>", "wino<1>", "wino_ws"):
            assert any(pool == 2 and s != 1.0 for s, _, _, _, pool in v), k


def test_both_sides_of_every_threshold():
    cd = lambda a, b: (a + b - 1) // b
    conv = {r.shape: r.kernel for r in R.cases() if r.entry == "conv" and r.stride == 1 and r.pool == 1}
    tiles = lambda s: cd(s[2], 32) * cd(s[1], 8) * s[0] * (s[4] // 64)
    mt = lambda s: cd(s[0] * s[1] * s[2], 32) * (s[4] // 64)
    assert {tiles(s) for s, k in conv.items() if k == "tiled<1,2,32>"} >= {260, 585, 650}
    assert max(tiles(s) for s, k in conv.items() if k != "tiled<1,2,32>") == 255 and min(tiles(s) for s, k in conv.items() if k == "tiled<1,2,32>") == 256
    assert max(mt(s) for s, k in conv.items() if k == "direct<1>") == 508 and min(mt(s) for s, k in conv.items() if k == "direct<2>") == 512
    wino = {r.shape: r.kernel for r in R.cases() if r.entry == "wino" and r.pool == 1 and r.slope is None}
    wt = lambda s: cd(s[2], 16) * cd(s[1], 8) * s[0] * (s[4] // 64)
    assert max(wt(s) for s, k in wino.items() if k == "wino<1>" and s[3] >= 64) == 199
    assert min(wt(s) for s, k in wino.items() if k == "wino_ws") == 200
    assert max(wt(s) for s, k in wino.items() if k == "wino<1>") == 511 and min(wt(s) for s, k in wino.items() if k == "wino<2>") == 512
    # persistent walks past one lap: more tiles than the 512 workgroups of the tiled and stride-2 kernels
    assert tiles((9, 33, 400, 32, 64)) > 512 and cd(cd(385, 2), 32) * cd(cd(73, 2), 4) * 8 == 560
    # at a budget of 8 CUs a workgroup of the wave-specialised kernel walks 27 tiles of the 216-tile map
    assert wt((3, 41, 183, 64, 64)) == 216 and R.ws_tiles_per_workgroup(3, 41, 183, 64, 8, 1) == 27
    assert R.ws_tiles_per_workgroup(3, 41, 183, 64, 24, 3) == 9 and R.ws_tiles_per_workgroup(3, 41, 183, 64, 0, 64) == 1
    # weight gradients: the LDS-staged kernel from 4096 pixels, the plain one below
    assert R.expected_kernel("wgrad", 3, 37, 51, 64, 64) == "wgrad_lds<2>" and 3 * 37 * 51 >= 4096
    assert R.expected_kernel("wgrad", 1, 64, 63, 64, 64) == "wgrad<2>" and R.expected_kernel("wgrad", 1, 64, 64, 128, 64) == "wgrad_lds<4>"
    assert R.expected_kernel("wgrad", 3, 37, 51, 32, 64) == "wgrad<1>"


def test_ops_routes_read_the_thresholds_from_ops():
    from cmr_agent_amd import ops
    routes = [R.ops_route(ops, *s, st, pool, False, u, True) for s, st, pool, u in R.OPS_ROUTES]
    assert {(e, k) for e, k, _ in routes} >= {("s2", "s2<4>"), ("conv", "tiled<2,1,16>"), ("conv", "direct<1>"), ("conv", "direct<2>"),
                                             ("conv", "tiled<1,2,32>"), ("wino", "wino<1>"), ("wino", "wino_ws")}
    assert any(sep for _, _, sep in routes)
    cd = lambda a, b: (a + b - 1) // b
    wt = [cd(s[2], 16) * cd(s[1], 8) * s[0] * (s[4] // 64) for s, st, _, u in R.OPS_ROUTES if st == 1 and u]
    assert max(t for t in wt if t < ops.WINO_MIN_TILES) >= ops.WINO_MIN_TILES - 4 and min(t for t in wt if t >= ops.WINO_MIN_TILES) <= ops.WINO_MIN_TILES + 16
    old = ops.WINO_MIN_TILES
    try:
        ops.WINO_MIN_TILES = 1
        assert R.ops_route(ops, 2, 9, 13, 64, 64)[0] == "wino"
    finally:
        ops.WINO_MIN_TILES = old
    assert R.ops_route(ops, 2, 9, 13, 64, 64)[0] == "conv"


def test_impulses_sit_on_both_sides_of_every_seam():
    for kernel, (entry, shape, stride) in [("tiled<1,2,32>", ("conv", (4, 33, 400, 32, 64), 1)), ("wino_ws", ("wino", (3, 41, 183, 64, 64), 1)),
                                           ("tiled<2,1,16>", ("conv", (8, 73, 385, 32, 64), 2))]:
        B, H, W = shape[:3]
        th, tw = R.TILE[kernel]
        pos = set(R.impulse_positions(B, H, W, (th, tw)))
        ys, xs = {p[1] for p in pos}, {p[2] for p in pos}
        assert {0, H - 1, th - 1, th, (H - 1) // th * th - 1, (H - 1) // th * th} <= ys
        assert {0, W - 1, tw - 1, tw, (W - 1) // tw * tw - 1, (W - 1) // tw * tw} <= xs
        assert {(0, H - 1, W - 1), (1, 0, 0), (B - 1, H - 1, W - 1), (0, 0, 0), (0, th - 1, tw - 1), (0, th, tw)} <= pos
    pos = set(R.impulse_positions(2, 5, 7, 32))           # a 32-pixel tile that straddles the two images
    flat = {b * 35 + y * 7 + x for b, y, x in pos}
    assert {0, 31, 32, 34, 35, 63, 64, 69} <= flat
    w = R.impulse_weights(64, 32)
    assert len({float(v) for v in w[0, 0].flatten()}) == 9 and not torch.equal(w[0, 0], w[1, 0]) and not torch.equal(w[0, 0], w[0, 1])


# ---- the rounding bars ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(R.ROUNDING_ROWS))
def test_rounding_bars(kernel):
    """BAR_FACTOR x the per-element forward error of the fp32 CPU evaluation on the same inputs; printed for DESIGN.md (pytest -s)."""
    entry, shape, stride = R.ROUNDING_ROWS[kernel]
    assert R.expected_kernel(entry, *shape, stride) == kernel
    c, ref, den, bar = R.rounding_case(kernel)
    print("%-14s %-22s bar %.3e" % (kernel, shape, bar))
    assert float(c.x.mean(dim=(0, 1, 2)).abs().max()) > 0.5, "the channel means must not vanish"
    eps = 2.0 ** -24
    assert 0.25 * eps < bar < 64 * eps, "a bar outside a few units of fp32 roundoff means the metric or the case is wrong"
    assert R.forward_error(ref, ref, den) == 0.0
    # the metric does not excuse a small output next to a large one: an error of 1e-4 of the SMALLEST denominator is caught
    k = int(den.flatten().argmin())
    bad = ref.clone().flatten()
    bad[k] += 1e-4 * float(den.flatten()[k])
    assert R.forward_error(bad.view_as(ref), ref, den) > bar
