"""Float64 restatement of the fp32 3x3 convolution family (csrc/conv.hip, conv_wino.hip, conv_s2.hip and the convolution half of
wgrad.hip / wgrad_wino.hip), the integer cases on which every fp32 kernel must equal it EXACTLY, and the kernel choice of the entry
points restated in Python.  No kernels are called from this file.

Exactness.  With small-integer x, res, post, bias, w in {-1, 0, 1} and a power-of-two slope every product and every partial sum of a 3x3
convolution is an integer (a multiple of 1/4 in the F(2x2,3x3) Winograd domain: G has entries 1/2, B^T and A^T entries 0 / +-1), the
activation multiplies by a power of two and the 2x2 pool divides by 4.  As long as the largest intermediate, counted in units of the
smallest quantum that can occur, stays below 2^24, fp32 holds every one of them exactly and the summation order is irrelevant:
`exact_ok` computes that bound with the absolute-value transforms and the case builders shrink their ranges until it holds.

Layouts are the kernels': maps NHWC, weights [Cout, Cin, 3, 3] (the packers make w9 / U / fragments from it), post [Ho, Wo, Cout]."""
import collections
import functools

import numpy as np
import torch

F64 = torch.float64

# F(2x2,3x3) transforms (Lavin & Gray 2015), as cmr_agent_amd/models/_pack.py:_WINO_G and csrc/conv_wino.hip use them
WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))
WINO_BT = ((1.0, 0.0, -1.0, 0.0), (0.0, 1.0, 1.0, 0.0), (0.0, -1.0, 1.0, 0.0), (0.0, 1.0, 0.0, -1.0))
WINO_AT = ((1.0, 1.0, 1.0, 0.0), (0.0, 1.0, -1.0, -1.0))

SLOPES = (1.0, 0.5, 0.25, 0.0, 2.0)


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().to(F64)


def out_size(n, stride):
    return (n - 1) // stride + 1


def lrelu_select(v, slope):
    """The kernels' activation: v > 0 ? v : slope * v (NOT max(v, slope v): they differ for a slope outside [0, 1])."""
    return torch.where(v > 0, v, v * slope)


def conv3x3_raw(x, w, stride=1):
    """x [B,H,W,Cin], w [Cout,Cin,3,3] -> [B,Ho,Wo,Cout] float64: nine shifted matrix products over the zero-padded map."""
    x, w = _d(x), _d(w)
    B, H, W, cin = x.shape
    ho, wo = out_size(H, stride), out_size(W, stride)
    xp = torch.zeros((B, H + 2, W + 2, cin), dtype=F64)
    xp[:, 1:H + 1, 1:W + 1] = x
    y = torch.zeros((B, ho, wo, w.shape[0]), dtype=F64)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
            y += win.reshape(-1, cin).matmul(w[:, :, ky, kx].t()).view(B, ho, wo, -1)
    return y


def epilogue(y, bias=None, slope=1.0, res=None, post=None, pool=1):
    """The kernels' order: + bias, + res, select activation, + post, then the 2x2 floor average pool; in y's own precision (float64 for the
    reference, fp32 when the CPU tier checks that fp32 is exact on the integer cases)."""
    t = lambda v: torch.as_tensor(v).detach().cpu().to(y.dtype)
    if bias is not None:
        y = y + t(bias)
    if res is not None:
        y = y + t(res)
    y = lrelu_select(y, slope)
    if post is not None:
        y = y + t(post).unsqueeze(0)
    if pool == 2:
        B, ho, wo, c = y.shape
        hp, wp = ho // 2, wo // 2
        y = y[:, :2 * hp, :2 * wp].reshape(B, hp, 2, wp, 2, c).sum((2, 4)) * 0.25
    return y


def conv3x3_ref(x_nhwc, w, bias=None, stride=1, slope=1.0, res=None, post=None, pool=1):
    return epilogue(conv3x3_raw(x_nhwc, w, stride), bias, slope, res, post, pool)


def forward_denominator(x_nhwc, w, bias=None, stride=1, res=None, post=None):
    """Per element sum |x||w| + |bias| + |res| + |post|: the forward-error denominator of one output element."""
    d = conv3x3_raw(_d(x_nhwc).abs(), _d(w).abs(), stride)
    for t in (bias, res):
        if t is not None:
            d = d + _d(t).abs()
    if post is not None:
        d = d + _d(post).abs().unsqueeze(0)
    return d


def forward_error(got, ref, den):
    """max over the tensor of |got - ref| / den (elements whose denominator is 0 must be exact)."""
    got, ref = _d(got), _d(ref)
    err = (got - ref).abs()
    zero = den == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    return float((err[~zero] / den[~zero]).max()) if bool((~zero).any()) else 0.0


def stem_ref(x_nchw, w_a, b_a, w3, w1, b_b, slope):
    """ops.stem_block: t = act(conv3x3(3->3)(x) + b_a); y = act(conv3x3(3->64)(t) + conv1x1(3->64)(x) + b_b) -> NHWC [B,H,W,64].
    w_a [3,3,3,3], w3 [64,3,3,3], w1 [64,3]."""
    x = _d(x_nchw).permute(0, 2, 3, 1)
    t = lrelu_select(conv3x3_raw(x, w_a) + _d(b_a), slope)
    y = conv3x3_raw(t, w3) + x.matmul(_d(w1).t()) + _d(b_b)
    return lrelu_select(y, slope)


def wgrad_ref(x, dy, stride=1):
    """x [B,H,W,Cin], dy [B,Ho,Wo,Cout] -> dw [Cout,Cin,3,3] float64 of y = conv3x3(x, w, stride), pad 1."""
    x, dy = _d(x), _d(dy)
    B, H, W, cin = x.shape
    ho, wo, cout = dy.shape[1], dy.shape[2], dy.shape[3]
    assert (ho, wo) == (out_size(H, stride), out_size(W, stride))
    xp = torch.zeros((B, H + 2, W + 2, cin), dtype=F64)
    xp[:, 1:H + 1, 1:W + 1] = x
    dw = torch.zeros((cout, cin, 3, 3), dtype=F64)
    g = dy.reshape(-1, cout).t()
    for ky in range(3):
        for kx in range(3):
            win = xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
            dw[:, :, ky, kx] = g.matmul(win.reshape(-1, cin))
    return dw


def wgrad_s2_ref(x, dy):
    return wgrad_ref(x, dy, 2)


def stats_ref(y, bias=None):
    """[2, C]: per channel sum (y - bias) and sum (y - bias)^2 over every pixel."""
    d = _d(y)
    if bias is not None:
        d = d - _d(bias)
    d = d.reshape(-1, d.shape[-1])
    return torch.stack([d.sum(0), (d * d).sum(0)])


def winograd_u_ref(w):
    """[Cout,Cin,3,3] -> U = G g G^T, float64, [16, Cout, Cin] (position = 4 i + j), un-fragmented."""
    g = torch.tensor(WINO_G, dtype=F64)
    w = _d(w)
    return torch.einsum("ik,ockl,jl->ijoc", g, w, g).reshape(16, w.shape[0], w.shape[1])


def unfragment(t, co, ci):
    """Inverse of the MFMA A-fragment permutation of _pack.winograd_u / frag_pack: [P][co/32 tiles][ci/8 k-groups][64 lanes][4] with lane =
    32 h + l holding M[32 tile + l][8 kgroup + 4 h .. + 3]  ->  [P, co, ci]."""
    p = t.numel() // (co * ci)
    return t.reshape(p, co // 32, ci // 8, 2, 32, 4).permute(0, 1, 4, 2, 3, 5).reshape(p, co, ci)


def w9_of(w):
    """[Cout,Cin,3,3] -> [9, Cout, Cin] (tap = 3 ky + kx), the layout of cmr_conv3x3_nhwc_f32."""
    return w.permute(2, 3, 0, 1).reshape(9, w.shape[0], w.shape[1]).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------------
# fp32 F(2x2,3x3) Winograd in numpy: the yardstick of the Winograd kernels' rounding (not the code under test)
# ------------------------------------------------------------------------------------------------------------------------------------
def _wino(x, wn, g, bt, at, dt):
    """Y = A^T [ sum_c (G g G^T) (.) (B^T d B) ] A over the 2x2 output tiles of the zero-padded map, every step in dtype dt."""
    B, H, W, cin = x.shape
    cout = wn.shape[0]
    u = np.einsum("ik,ockl,jl->ijco", g, wn, g).astype(dt)                         # [4,4,cin,cout]
    ty, tx = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((B, 2 * ty + 2, 2 * tx + 2, cin), dtype=dt)
    xp[:, 1:H + 1, 1:W + 1] = x
    d = np.empty((4, 4, B, ty, tx, cin), dtype=dt)
    for i in range(4):
        for j in range(4):
            d[i, j] = xp[:, i:i + 2 * ty:2, j:j + 2 * tx:2]
    v = np.einsum("ik,kl...,jl->ij...", bt, d, bt).astype(dt)                      # additions only
    m = np.matmul(v.reshape(16, -1, cin), u.reshape(16, cin, cout)).astype(dt).reshape(4, 4, B, ty, tx, cout)
    yt = np.einsum("ai,ij...,bj->ab...", at, m, at).astype(dt)                     # [2,2,B,ty,tx,cout]
    y = yt.transpose(2, 3, 0, 4, 1, 5).reshape(B, 2 * ty, 2 * tx, cout)
    return np.ascontiguousarray(y[:, :H, :W])


def wino_fp32(x_nhwc, w, order=None):
    """fp32 throughout: U = G g G^T, V = B^T d B per 2x2 output tile, M = sum over the input channels (taken in `order`, a permutation)
    of U V, Y = A^T M A -> [B,H,W,Cout] float32 (stride 1, pad 1, no epilogue)."""
    x = np.asarray(torch.as_tensor(x_nhwc).cpu(), dtype=np.float32)
    wn = np.asarray(torch.as_tensor(w).cpu(), dtype=np.float32)
    if order is not None:
        x, wn = np.ascontiguousarray(x[..., order]), np.ascontiguousarray(wn[:, order])
    g, bt, at = (np.array(m, dtype=np.float32) for m in (WINO_G, WINO_BT, WINO_AT))
    return torch.from_numpy(_wino(x, wn, g, bt, at, np.float32))


def wino_abs(x_nhwc, w):
    """The absolute-value transforms |A^T| [ sum_c (|G||g||G|^T) (.) (|B^T||d||B|) ] |A| in float64: no intermediate of a Winograd
    evaluation of (x, w), in any summation order, exceeds the largest element of this map."""
    x = np.abs(np.asarray(torch.as_tensor(x_nhwc).cpu(), dtype=np.float64))
    wn = np.abs(np.asarray(torch.as_tensor(w).cpu(), dtype=np.float64))
    g, bt, at = (np.abs(np.array(m, dtype=np.float64)) for m in (WINO_G, WINO_BT, WINO_AT))
    return _wino(x, wn, g, bt, at, np.float64)


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernel choice of the entry points, restated
# ------------------------------------------------------------------------------------------------------------------------------------
UNSUPPORTED, INVALID = "unsupported", "invalid"
FORWARD_KERNELS = ("direct<1>", "direct<2>", "tiled<1,2,32>", "tiled<2,1,16>", "s2<4>", "wino<1>", "wino<2>", "wino_ws")
WGRAD_KERNELS = ("wgrad<1>", "wgrad<2>", "wgrad<4>", "wgrad_lds<2>", "wgrad_lds<4>", "wgrad_s2<1>", "wgrad_s2<2>", "wgrad_s2<4>", "wgrad_wino")


def _cdiv(a, b):
    return (a + b - 1) // b


def expected_kernel(entry, B, H, W, cin, cout, stride=1, pool=1, slope=1.0, res=False, post=False):
    """Which kernel an entry point launches (or UNSUPPORTED / INVALID).  entry: "conv" cmr_conv3x3_nhwc_f32 (csrc/conv.hip:662-682),
    "wino" cmr_conv3x3_wino_nhwc_f32 (csrc/conv_wino.hip:973-989), "s2" cmr_conv3x3_s2_nhwc_f32 (csrc/conv_s2.hip:210-226), "wgrad"
    cmr_conv3x3_wgrad_f32 (csrc/wgrad.hip:1579-1597 wgrad_lds_plan, :1666-1704), "wgrad_s2" cmr_conv3x3_wgrad_s2_f32 (:1707-1723),
    "wgrad_wino" cmr_conv3x3_wgrad_wino_f32 (csrc/wgrad_wino.hip:241-256)."""
    if entry == "conv":
        if cin % 32 or cin < 32 or cout % 64 or cout < 64 or stride not in (1, 2):         # conv.hip:666
            return INVALID
        if not (pool == 1 or (pool == 2 and stride == 1 and not res and not post)):         # :668
            return INVALID
        if stride == 2:
            return "tiled<2,1,16>"                                                          # :681
        tiles = _cdiv(W, 32) * _cdiv(H, 8) * B * (cout // 64)                               # :673
        if tiles < 256:                                                                     # :674
            if pool != 1:
                return UNSUPPORTED                                                          # :675
            mtiles = _cdiv(B * H * W, 32)                                                   # :676
            return "direct<1>" if mtiles * (cout // 64) < 512 else "direct<2>"              # :677
        return "tiled<1,2,32>"                                                              # :679
    if entry == "wino":
        if cin % 32 or cin < 32 or cout % 64 or cout < 64 or stride != 1:                   # conv_wino.hip:976
            return INVALID
        if not (pool == 1 or (pool == 2 and not res and not post)):                         # :979
            return INVALID
        nt64 = _cdiv(W, 16) * _cdiv(H, 8) * B * (cout // 64)                                # :980-984
        if cin >= 64 and nt64 >= 200 and 0.0 <= slope <= 1.0:                               # :986
            return "wino_ws"
        return "wino<2>" if nt64 >= 512 else "wino<1>"                                      # :987-988
    if entry == "s2":
        if cout % 64 or cout < 64:                                                          # conv_s2.hip:212
            return INVALID
        if cin != 64 or post:                                                               # :213
            return UNSUPPORTED
        return "s2<4>"                                                                      # :224
    if entry in ("wgrad", "wgrad_s2"):
        if cout not in (32, 64, 128, 256) or cin not in (32, 64, 128):                      # wgrad.hip:1669, :1710
            return INVALID
        if entry == "wgrad_s2":
            if H < 2 or W < 4 or H % 2 or W % 2:                                            # :1709
                return INVALID
            return "wgrad_s2<%d>" % (cin // 32)                                             # :1717-1719
        if W < 2:                                                                           # :1668
            return INVALID
        npx = B * H * W
        if cin in (64, 128) and 4096 <= npx <= 150000:                                      # :1586
            return "wgrad_lds<%d>" % (cin // 32)                                            # :1679-1687
        return "wgrad<%d>" % (cin // 32)                                                    # :1695-1700
    if entry == "wgrad_wino":
        if cin != 64 or cout != 64 or H % 2 or W % 2 or H < 2 or W < 2:                     # wgrad_wino.hip:244
            return UNSUPPORTED
        return "wgrad_wino"
    raise ValueError(entry)


def ws_tiles_per_workgroup(B, H, W, cout, cu_budget, slices, cus=256):
    """Tiles one workgroup of the wave-specialised kernel walks (csrc/conv_wino.hip:872-890 wino_ws_grid)."""
    nt = _cdiv(W, 16) * _cdiv(H, 8) * B * (cout // 64)
    if 0 < cu_budget < cus:
        cus = cu_budget
    cus = max(cus, 8)
    cus -= cus % 8
    want = cus
    if slices > 1:
        sl = min(slices, 64)
        while sl > 1 and nt // (cus * sl) < 8:
            sl -= 1
        want = cus * sl
    return _cdiv(nt, min(nt, want))


# ------------------------------------------------------------------------------------------------------------------------------------
# integer cases
# ------------------------------------------------------------------------------------------------------------------------------------
def _quantum(slope):
    """Smallest power of two q such that slope * integer is a multiple of q."""
    q = 1.0
    while (abs(slope) / q) % 1.0 != 0.0:
        q /= 2
    return q


LIMIT = float(2 ** 24)


def forward_bound(x, w, bmax, rmax, pmax, slope, pool, winograd, stride=1):
    """Largest intermediate of a forward kernel on (x, w), in units of the smallest quantum that occurs.  First the cheap bound (every
    input at max|x|); where that is not enough (impulse scenes: one channel per pixel, weights up to 63) the absolute-value transforms on
    the data itself."""
    wa, xmax = _d(w).abs(), float(x.abs().max())
    q = 1.0
    if winograd:
        g, bt, at = (torch.tensor(m, dtype=F64).abs() for m in (WINO_G, WINO_BT, WINO_AT))
        u = torch.einsum("ik,ockl,jl->ijo", g, wa, g)                         # summed over the input channels
        rs = bt.sum(1)
        acc = float(torch.einsum("ai,ijo,bj->abo", at, u * (rs.view(4, 1) * rs.view(1, 4) * xmax).unsqueeze(-1), at).max())
        q = 0.25
    else:
        acc = float(wa.sum((1, 2, 3)).max()) * xmax

    def total(acc):
        v = (acc + bmax + rmax) * max(1.0, abs(slope)) + pmax
        qq = q * _quantum(slope)
        return (4 * v) / (qq / 4) if pool == 2 else v / qq                     # pool: four outputs summed, then * 0.25

    if total(acc) >= LIMIT:
        acc = float(wino_abs(x, w).max()) if winograd else float(conv3x3_raw(x.abs(), wa, stride).max())
    return total(acc)


def wgrad_bound(npix, xmax, dymax, winograd):
    """Largest intermediate of a weight gradient in quanta: every pixel may contribute xmax dymax; in the Winograd domain P = A dY A^T and
    V = B^T d B sum 4 entries each over npix / 4 tiles and G^T M G (quantum 1/4) sums 4 positions of weight <= 1 per axis."""
    if winograd:
        return 4.0 * 16.0 * (npix / 4.0) * (4 * xmax) * (4 * dymax)
    return float(npix) * xmax * dymax


Case = collections.namedtuple("Case", "x w bias res post slope stride pool")


def _ints(gen, shape, r):
    if r == 0:
        return torch.zeros(shape, dtype=torch.float32)
    return torch.randint(-r, r + 1, shape, generator=gen).float()


def exact_ok(case, winograd=True):
    """True when every intermediate of every forward kernel that can serve the case (the direct ones, and Winograd for stride 1 unless
    winograd=False) is exactly representable in fp32."""
    mx = lambda t: 0.0 if t is None else float(t.abs().max())
    b = [forward_bound(case.x, case.w, mx(case.bias), mx(case.res), mx(case.post), case.slope, case.pool, False, case.stride)]
    if winograd and case.stride == 1:
        b.append(forward_bound(case.x, case.w, mx(case.bias), mx(case.res), mx(case.post), case.slope, case.pool, True))
    return max(b) < LIMIT


def integer_case(seed, B, H, W, cin, cout, stride=1, slope=None, bias=True, res=False, post=False, pool=1, xr=4):
    """x, res, post from small integers, w from {-1, 0, 1}, bias from small integers, slope (when not given) from SLOPES by the seed; the x
    range shrinks until exact_ok holds."""
    gen = torch.Generator().manual_seed(1000 + seed)
    ho, wo = out_size(H, stride), out_size(W, stride)
    slope = SLOPES[seed % len(SLOPES)] if slope is None else slope
    w = _ints(gen, (cout, cin, 3, 3), 1)
    bv = _ints(gen, (cout,), 3) if bias else None
    rv = _ints(gen, (B, ho, wo, cout), 4) if res else None
    pv = _ints(gen, (ho, wo, cout), 4) if post else None
    while True:
        x = _ints(gen, (B, H, W, cin), xr)
        c = Case(x, w, bv, rv, pv, float(slope), stride, pool)
        if exact_ok(c):
            return c
        assert xr > 1, "no integer range makes this case exact"
        xr -= 1


TAP_MOD = 7


def impulse_weights(cout, cin):
    """w[o,c,ky,kx] = 1 + kx + 3 ky + 9 ((o + 5 c) % 7): nine distinct taps, distinct across neighbouring channels."""
    o = torch.arange(cout).view(-1, 1, 1, 1)
    c = torch.arange(cin).view(1, -1, 1, 1)
    ky = torch.arange(3).view(1, 1, -1, 1)
    kx = torch.arange(3).view(1, 1, 1, -1)
    return (1 + kx + 3 * ky + 9 * ((o + 5 * c) % TAP_MOD)).float()


def _marks(n, tile):
    """Positions along one axis of n pixels: both ends and their neighbours (either parity: a stride-2 kernel sees an even pixel through
    its centre tap only), the middle, and both sides of the first, second and last tile boundary."""
    s = {0, 1, n - 2, n - 1, n // 2}
    bounds = list(range(tile, n, tile))
    for b in bounds[:2] + bounds[-1:]:
        s.update((b - 1, b))
    return sorted(p for p in s if 0 <= p < n)


def impulse_positions(B, H, W, tile):
    """(b, y, x) of the impulses for a kernel whose tile is `tile`: (th, tw) in input pixels for a 2-D tile, an int for kernels that tile
    the flattened pixel index.  Corners, edges, tile seams, and the last pixel of an image with the first of the next."""
    pos = set()
    if isinstance(tile, tuple):
        ys, xs = _marks(H, tile[0]), _marks(W, tile[1])
        for b in sorted({0, B - 1}):
            for y in ys:
                for x in xs:
                    if y in (0, H - 1, H // 2) or x in (0, W - 1, W // 2) or (y in ys[1:-1] and x in xs[1:-1]):
                        pos.add((b, y, x))
    else:
        n = B * H * W
        flat = set(_marks(n, tile))
        for b in range(B):
            flat.update((b * H * W, b * H * W + W - 1, (b + 1) * H * W - W, (b + 1) * H * W - 1))
        for p in flat:
            pos.add((p // (H * W), (p % (H * W)) // W, p % W))
    for b in range(B - 1):
        pos.update(((b, H - 1, W - 1), (b + 1, 0, 0)))
    return sorted(pos)


def impulse_case(B, H, W, cin, cout, tile, stride=1, slope=1.0, bias=False, pool=1, amp=3):
    """One pixel, one channel per impulse (value 1 .. amp, channel cycling), with impulse_weights."""
    x = torch.zeros((B, H, W, cin), dtype=torch.float32)
    for i, (b, y, xx) in enumerate(impulse_positions(B, H, W, tile)):
        x[b, y, xx, (7 * i + 3) % cin] = 1 + i % amp
    w = impulse_weights(cout, cin)
    bv = (torch.arange(cout) % 5 - 2).float() if bias else None
    c = Case(x, w, bv, None, None, float(slope), stride, pool)
    assert exact_ok(c)
    return c


def wgrad_case(seed, B, H, W, cin, cout, stride=1, winograd=False, r=3):
    """Integer x and dy whose ranges shrink until wgrad_bound stays below 2^24 -> (x, dy, range)."""
    gen = torch.Generator().manual_seed(2000 + seed)
    ho, wo = out_size(H, stride), out_size(W, stride)
    while wgrad_bound(B * ho * wo, r, r, winograd) >= LIMIT:
        assert r > 1, "no integer range makes this weight gradient exact"
        r -= 1
    return _ints(gen, (B, H, W, cin), r), _ints(gen, (B, ho, wo, cout), r), r


def real_case(seed, B, H, W, cin, cout, stride=1, res=True, post=True):
    """Real-valued data for the rounding bars: normal, with a non-zero mean per channel."""
    gen = torch.Generator().manual_seed(3000 + seed)
    ho, wo = out_size(H, stride), out_size(W, stride)
    x = torch.randn((B, H, W, cin), generator=gen) + torch.randn((cin,), generator=gen)
    w = torch.randn((cout, cin, 3, 3), generator=gen) / (3.0 * cin ** 0.5) + 0.02
    bv = torch.randn((cout,), generator=gen)
    rv = torch.randn((B, ho, wo, cout), generator=gen) + 0.5 if res else None
    pv = torch.randn((ho, wo, cout), generator=gen) if post else None
    return Case(x, w, bv, rv, pv, 0.25, stride, 1)


# ------------------------------------------------------------------------------------------------------------------------------------
# the case table: (entry, shape, expected kernel); the GPU tier cycles epilogues and slopes over it
# ------------------------------------------------------------------------------------------------------------------------------------
Row = collections.namedtuple("Row", "entry shape stride kernel pool slope note")
EPILOGUES = ("none", "bias", "bias+res", "bias+res+post")
CASE_SLOPES = (1.0, 0.25, 0.0)
TILE = {"direct<1>": 32, "direct<2>": 32, "tiled<1,2,32>": (8, 32), "tiled<2,1,16>": (8, 64), "s2<4>": (8, 64), "wino<1>": (8, 16),
        "wino<2>": (8, 16), "wino_ws": (8, 16)}          # in INPUT pixels (a stride-2 tile of 4 x 32 outputs covers 8 x 64 inputs)

_CONV_S1 = [(1, 1, 1, 32, 64), (1, 1, 2, 64, 64), (1, 2, 1, 64, 64), (1, 1, 40, 64, 64), (3, 3, 3, 64, 64), (2, 5, 7, 128, 128),
            (1, 64, 127, 32, 128),                                            # 508: last direct<1>
            (1, 64, 128, 32, 128), (1, 63, 131, 32, 128), (1, 64, 256, 32, 64),   # direct<2>: 512, a 29-pixel last tile
            (3, 33, 544, 32, 64),                                             # 255 8x32 tiles: still direct
            (8, 64, 128, 32, 64), (4, 33, 400, 32, 64), (9, 33, 400, 32, 64), (5, 33, 400, 64, 128)]    # tiled: 256, 260, 585, 650 tiles
_S2_SPATIAL = [(1, 1, 1), (1, 2, 2), (1, 3, 3), (2, 7, 9), (1, 8, 64), (1, 9, 65), (8, 73, 385)]
_S2_TILED_CIN = {(1, 3, 3): 64, (1, 9, 65): 128}
_WINO = [(1, 1, 1, 64, 64), (1, 2, 2, 64, 64), (1, 3, 3, 64, 64), (1, 8, 16, 64, 64), (1, 9, 17, 64, 64), (2, 7, 15, 128, 128),
         (3, 17, 33, 32, 64), (1, 8, 3184, 64, 64),                           # 199 tiles: last wino<1> at Cin >= 64
         (1, 50, 1160, 32, 64),                                               # 511 tiles at Cin = 32: last wino<1>
         (2, 64, 512, 32, 64), (2, 57, 497, 32, 64),                          # wino<2>: 512 tiles
         (2, 80, 160, 64, 64), (1, 8, 3200, 64, 64), (3, 41, 183, 64, 64), (2, 41, 183, 64, 128)]      # wave-specialised: 200 ...
WS_SHAPES = _WINO[-4:]
WS_BUDGETS = (0, 8, 24)
WS_SLICES = (1, 2, 3, 64)
STEM_SHAPES = [(1, 1, 1), (1, 1, 5), (2, 5, 1), (1, 3, 257), (2, 16, 35), (1, 257, 513)]

WGRAD_CHANNELS = [(32, 32), (32, 64), (32, 256), (64, 32), (64, 256), (128, 32), (128, 256)]
WGRAD_MAPS = [(1, 1, 2), (1, 2, 3), (3, 2, 3), (2, 9, 13), (3, 37, 51)]
WGRAD_S2_CHANNELS = [(32, 32), (32, 256), (64, 64), (128, 64)]
WGRAD_S2_MAPS = [(1, 2, 4), (2, 6, 10), (1, 30, 18)]
WGRAD_WINO_MAPS = [(1, 2, 2), (1, 2, 16), (3, 10, 44), (2, 96, 128)]
PACK_SHAPES = [(64, 32), (32, 64), (64, 64), (128, 64), (64, 128), (256, 128)]


@functools.lru_cache(maxsize=None)
def cases():
    """Every (entry, shape) of the two tiers with the kernel that must serve it."""
    rows = []

    def add(entry, shape, stride=1, pool=1, slope=None, note=""):
        B, H, W, cin, cout = shape
        k = expected_kernel(entry, B, H, W, cin, cout, stride, pool, 1.0 if slope is None else slope)
        rows.append(Row(entry, shape, stride, k, pool, slope, note))

    for s in _CONV_S1:
        add("conv", s)
    add("conv", (4, 33, 401, 32, 64), pool=2, note="fused pool, odd both ways")
    add("conv", (3, 33, 544, 32, 64), pool=2, note="255 tiles: the entry point leaves the pool to the caller")
    for sp in _S2_SPATIAL:
        add("conv", sp + (_S2_TILED_CIN.get(sp, 32), 64), stride=2)
        add("s2", sp + (64, 64), stride=2)
    add("s2", (4, 73, 385, 64, 128), stride=2)
    add("s2", (2, 7, 9, 32, 64), stride=2, note="Cin = 32: refused")
    for s in _WINO:
        add("wino", s)
    add("wino", (2, 9, 13, 64, 64), pool=2)
    add("wino", (2, 80, 160, 64, 64), pool=2)
    add("wino", (3, 41, 183, 64, 64), pool=2)
    add("wino", (2, 57, 497, 64, 64), slope=2.0, note="slope outside [0, 1] keeps off the wave-specialised kernel")
    for cin, cout in WGRAD_CHANNELS:
        for m in WGRAD_MAPS:
            add("wgrad", m + (cin, cout))
    add("wgrad", (3, 37, 51, 64, 64))
    add("wgrad", (3, 37, 51, 128, 128))
    add("wgrad", (2, 96, 128, 64, 64), note="ops.conv3x3_wgrad with WGRAD_WINO off")
    for cin, cout in WGRAD_S2_CHANNELS:
        for m in WGRAD_S2_MAPS:
            add("wgrad_s2", m + (cin, cout), stride=2)
    for m in WGRAD_WINO_MAPS:
        add("wgrad_wino", m + (64, 64))
    return tuple(rows)


def forward_rows(entry=None, kernel=None):
    return [r for r in cases() if r.entry in ("conv", "s2", "wino") and (entry is None or r.entry == entry)
            and (kernel is None or r.kernel == kernel)]


def row_id(r):
    return "%s-%s-s%d%s%s" % (r.entry, "x".join(map(str, r.shape)), r.stride, "-pool" if r.pool == 2 else "",
                              "" if r.slope is None else "-slope%g" % r.slope)


def row_case(i, r, impulse=False):
    """The integer (or impulse) case of forward row number i.  The epilogue and the slope cycle with the row's position j among the rows
    of ITS kernel, starting from the full epilogue at slope 0.25, so that every kernel sees every operand behind a real activation."""
    B, H, W, cin, cout = r.shape
    j = sum(1 for q in forward_rows()[:i] if q.kernel == r.kernel and q.pool == r.pool)
    slope = CASE_SLOPES[(j + 1) % 3] if r.slope is None else r.slope
    if r.pool == 2 and r.slope is None:
        slope = (0.25, 0.0)[j % 2]                       # a pool before or after an identity activation is the same thing
    if impulse:
        return impulse_case(B, H, W, cin, cout, TILE.get(r.kernel, (8, 16)), r.stride, slope, bias=not j & 1, pool=r.pool)
    e = 1 if r.pool == 2 else (3 - j) % 4
    post = e >= 3 and r.entry != "s2"
    return integer_case(i, B, H, W, cin, cout, r.stride, slope, bias=e >= 1, res=e >= 2, post=post, pool=r.pool)


def ops_route(ops, B, H, W, cin, cout, stride=1, pool=1, post=False, have_u=True, have_s2=True):
    """(entry, kernel, separate_pool) that ops.conv3x3 takes in fp32 mode (cmr_agent_amd/ops.py:375-398); the thresholds are read from
    `ops` (WINO_MIN_TILES, WINOGRAD, STRIDE2_FRAGS), not copied."""
    if ops.STRIDE2_FRAGS and stride == 2 and pool == 1 and not post and have_s2:
        k = expected_kernel("s2", B, H, W, cin, cout, 2)
        if k != UNSUPPORTED:
            return "s2", k, False
    if ops.WINOGRAD and have_u and stride == 1 and _cdiv(W, 16) * _cdiv(H, 8) * B * (cout // 64) >= ops.WINO_MIN_TILES:
        return "wino", expected_kernel("wino", B, H, W, cin, cout, 1, pool), False
    k = expected_kernel("conv", B, H, W, cin, cout, stride, pool)
    if k == UNSUPPORTED:
        return "conv", expected_kernel("conv", B, H, W, cin, cout, stride, 1), True
    return "conv", k, False


# (shape, stride, pool, have_u): one pass through ops.conv3x3 per route
OPS_ROUTES = [((2, 7, 9, 64, 64), 2, 1, True),            # stride-2 fragment kernel
              ((2, 7, 9, 32, 64), 2, 1, True),            # Cin = 32: the fragment kernel declines -> tiled stride 2
              ((2, 9, 13, 64, 64), 1, 1, True),           # 4 Winograd tiles < WINO_MIN_TILES -> direct<1>
              ((3, 17, 33, 32, 64), 1, 2, True),          # 27 tiles, pool: the direct kernel + a separate pool
              ((3, 33, 544, 32, 64), 1, 2, False),        # no U, 255 tiles, pool: direct<2> + a separate pool
              ((4, 33, 401, 32, 64), 1, 2, False),        # no U: tiled kernel with the fused pool
              ((2, 33, 65, 64, 64), 1, 1, True),          # 50 tiles -> direct<1>
              ((2, 41, 65, 64, 64), 1, 2, True),          # 60 tiles, one tile row below WINO_MIN_TILES
              ((2, 57, 65, 64, 64), 1, 2, True),          # 80 tiles -> wino<1> with the fused pool
              ((3, 41, 183, 64, 64), 1, 1, True)]         # wave-specialised Winograd


# ------------------------------------------------------------------------------------------------------------------------------------
# stem
# ------------------------------------------------------------------------------------------------------------------------------------
Stem = collections.namedtuple("Stem", "x w_a b_a w3 w1 b_b slope")


def stem_case(seed, B, H, W, slope, impulse=False):
    """Integer image [B,3,H,W] and weights for ops.stem_block; impulse: single pixels (stem_b tiles 32 flattened pixels) with distinct
    taps.  stem_bound gives the largest intermediate; the quantum is slope^2 >= 1/16."""
    gen = torch.Generator().manual_seed(4000 + seed)
    if impulse:
        x = torch.zeros((B, 3, H, W), dtype=torch.float32)
        for i, (b, y, xx) in enumerate(impulse_positions(B, H, W, 32)):
            x[b, i % 3, y, xx] = 1 + i % 3
        w_a, w3 = impulse_weights(3, 3), impulse_weights(64, 3)
        w1 = (1 + (torch.arange(64).view(-1, 1) + 3 * torch.arange(3).view(1, -1)) % 11).float()
        b_a, b_b = torch.tensor([1.0, -2.0, 0.0]), (torch.arange(64) % 5 - 2).float()
    else:
        x = _ints(gen, (B, 3, H, W), 2)
        w_a, w3, w1 = _ints(gen, (3, 3, 3, 3), 1), _ints(gen, (64, 3, 3, 3), 1), _ints(gen, (64, 3), 1)
        b_a, b_b = _ints(gen, (3,), 2), _ints(gen, (64,), 3)
    return Stem(x, w_a, b_a, w3, w1, b_b, float(slope))


def stem_bound(s):
    """Largest intermediate of the stem in quanta (slope^2: both activations may scale)."""
    x = s.x.permute(0, 2, 3, 1)
    t = conv3x3_raw(x.abs(), s.w_a.abs()) + s.b_a.abs()
    y = conv3x3_raw(t, s.w3.abs()) + _d(x).abs().matmul(_d(s.w1).abs().t()) + _d(s.b_b).abs()
    return float(y.max()) / _quantum(s.slope) ** 2


# ------------------------------------------------------------------------------------------------------------------------------------
# rounding bars: one real-valued case per forward kernel at a ragged shape
# ------------------------------------------------------------------------------------------------------------------------------------
ROUNDING_ROWS = {"direct<1>": ("conv", (2, 5, 7, 128, 128), 1), "direct<2>": ("conv", (1, 63, 131, 32, 128), 1),
                 "tiled<1,2,32>": ("conv", (4, 33, 400, 32, 64), 1), "tiled<2,1,16>": ("conv", (1, 9, 65, 128, 64), 2),
                 "s2<4>": ("s2", (1, 9, 65, 64, 64), 2), "wino<1>": ("wino", (3, 17, 33, 32, 64), 1),
                 "wino<2>": ("wino", (2, 57, 497, 32, 64), 1), "wino_ws": ("wino", (3, 41, 183, 64, 64), 1)}
BAR_FACTOR = 4.0          # the project's standing margin for a different summation order on the matrix cores


@functools.lru_cache(maxsize=None)
def rounding_case(kernel):
    """-> (case, float64 reference, denominator, bar): the bar is BAR_FACTOR x the per-element forward error of fp32 F.conv2d (direct
    kernels) or of the fp32 numpy Winograd (Winograd kernels) on the same inputs, each followed by the fp32 epilogue."""
    import torch.nn.functional as F
    entry, shape, stride = ROUNDING_ROWS[kernel]
    c = real_case(sorted(ROUNDING_ROWS).index(kernel), *shape, stride=stride, post=entry != "s2")
    ref = conv3x3_ref(c.x, c.w, c.bias, stride, c.slope, c.res, c.post)
    den = forward_denominator(c.x, c.w, c.bias, stride, c.res, c.post)
    if entry == "wino":
        raw = wino_fp32(c.x, c.w)
    else:
        raw = F.conv2d(c.x.permute(0, 3, 1, 2), c.w, None, stride, 1).permute(0, 2, 3, 1)
    cpu = forward_error(epilogue(raw.float(), c.bias, c.slope, c.res, c.post), ref, den)
    return c, ref, den, BAR_FACTOR * cpu
