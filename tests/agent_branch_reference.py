"""Float64 restatement of what every agent step runs besides the 3x3 convolutions and the observation kernels: the fused ConvBNReLURes1D
block (csrc/cbr_block.hip, csrc/cbr_block_bf16.hip), its per-tile column maxima and their fold (cmr_colmax_partials_f32), the glue launch
(cmr_colmax_bias2_f32), the whole 3-D branch (CMRAgent.py:88-101 over PointNN.py:260-282) and the one-launch tail (csrc/agent_heads.hip;
CMRAgent.py:52-56, 59-86, 101-123).  No kernel is called from this file and nothing here imports the GPU.

Two kinds of inputs.

EXACT cases.  Integer inputs, weights in {-1, 0, 1}, integer biases and slope 1/2: every product and every partial sum of every layer is
a multiple of a known power of two (1 for the first pre-activation, halved by every LeakyReLU), and as long as the sum of the ABSOLUTE
values of a layer's terms, counted in that quantum, stays below 2^24, fp32 holds every partial sum in ANY order exactly -- fused or
separate multiply-add, matrix core or scalar.  A kernel must then equal float64 bit for bit.  `*_exact_measure` returns that count.
For the bf16 block the operands of the matrix cores (x, the weights, the hidden activations) are additionally exactly representable in
bf16 (8 significant bits), so its rounding is the identity on them.

REAL-VALUED cases come with an a-priori element-wise bound (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 / 3.5): an
n-term inner product evaluated in any order, fused or not, errs by at most gamma_n sum|terms|, gamma_n = n u / (1 - n u), u = 2^-24;
LeakyReLU with a slope in [0, 1] and max are 1-Lipschitz, so an input error passes through them undiminished at worst:
    e_h = gamma_{KX+1} (|W1||x| + |b1|) + u |hid|
    e_y = |W2| e_h + gamma_{CH+KX+2} (|W2||hid| + |Wsc||x| (or |x|) + |b2|) + u |y|
and layer by layer in the same way for the glue rows and the tail (n = npix for the pool).  The GPU tier allows 2 x this bound."""
import math
import types

import torch

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24
TILE = 32                    # rows of one tile of the block kernels
MAX_BIAS_ROWS = 16           # per-batch bias rows the block kernels stage (CBR_MAXB)
# (KX, CH, CO, conv shortcut) the block kernels are instantiated for (cmr_cbr_block_f32's dispatch)
INSTANCES = ((64, 64, 64, False), (128, 128, 64, True), (64, 128, 64, True), (64, 128, 128, False), (8, 8, 64, True))
ROWS = (1, 31, 32, 33, 261)
NPIX = (1, 8, 9, 31, 33, 57, 65, 121, 129, 255, 257, 289, 6688)
TILES_PER_BATCH = (1, 2, 63, 64, 65, 512, 513)
GLUE_WIDTHS = ((128, 64), (128, 128), (4, 252), (64, 4))


# Real-valued weights are uniform in +-2 s / k: the row sums of |W| are s on average.  The any-order bound of a layer is gamma times the
# sum of |terms|, whatever the result: with s = 1/4 (block, glue) a 258-term output element carries gamma_258 * (|b| + about 0.2) against
# outputs of the size of the biases, which keeps the bound under 2e-5 of a column's maximum.  Larger weights test nothing more: a wrong
# index moves a result by the size of an operand, thousands of bounds.  (The tail's layers: _mixed.  The branch has a bar of its own.)
REAL_ROW_SUM = 0.25


TAIL_TAU = 3.0               # sum|terms| over the column's maximum, taken as a small constant (a result made of a bias and a weighted sum of like size)


def tail_tightness_ceiling(c, head, logits):
    """What the CPU tier asks of the any-order bound on the logits of head `head`, as a share of a column's maximum, derived from the
    layers' gammas and not from the bound: layer i of the five inner products (128, 128, 256, n0, n1 terms) adds gamma_{k_i + 1} times
    sum|terms|, and every later layer multiplies what it inherits by its row sum of |W|, c.row_sum; the pool adds gamma_{npix + 1}
    mean|x| in absolute terms, which passes all five.  With sum|terms| / max|result| taken as TAIL_TAU:
        TAIL_TAU * (sum_i gamma_{k_i + 1} row_sum^(4 - i)  +  gamma_{npix + 1} mean|x| row_sum^5 / median column maximum).
    For the signal-carrying cases (row_sum 1.25) this is 2e-4 to 3e-4, more where the pool is long or the map's mean is large against
    the logits.  The contracting cases (row_sum 1/8: only the last layer's gamma_257 counts, and a logit is its bias and little else)
    are held to the 2e-5 the two-layer block meets instead, at every npix."""
    n0, n1 = c.heads[head][0][0].shape[0], c.heads[head][1][0].shape[0]
    rel = sum(gamma(k + 1) * c.row_sum ** (4 - i) for i, k in enumerate((128, 128, 256, n0, n1)))
    pool = gamma(c.npix + 1) * float(c.x.to(F64).abs().mean()) * c.row_sum ** 5
    return TAIL_TAU * (rel + pool / float(logits.abs().max(0)[0].median()))


REAL_SEED = 2                # tail cases: a seed for which the float64 logits alone meet the argmax rule's 5 % condition on every case


def wrap_rows(inst, bf16=False):
    """First row count of the persistent tile loop's SECOND pass + 39: the fp32 launch caps its grid at 256 workgroups of 8 tiles
    when the LDS footprint exceeds 80 KB (one workgroup per CU) and at 512 otherwise; the bf16 launch at 512 always."""
    kx, ch, co, conv = inst
    t1 = (ch + 31) // 32
    smem = 4 * (32 * t1 * (kx + 4) + co * (ch + 4) + (co * (kx + 4) if conv else 0) + MAX_BIAS_ROWS * (32 * t1 + co))
    groups = 512 if (bf16 or smem <= 80 * 1024) else 256
    return groups * 8 * TILE + 39


def gamma(n):
    return n * U / (1.0 - n * U)


def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def bf16_round(t):
    """round to nearest even to bf16, through fp32 as the kernel's conversion does"""
    return t.to(F32).to(torch.bfloat16).to(t.dtype)


def mm(a, w, order="matmul"):
    """a [r, k] times w [n, k]^T in a's dtype; `forward` / `reversed` add one k at a time in that order."""
    if order == "matmul":
        return a.matmul(w.t())
    k = a.shape[1]
    acc = torch.zeros((a.shape[0], w.shape[0]), dtype=a.dtype)
    for j in (range(k) if order == "forward" else range(k - 1, -1, -1)):
        acc = acc + a[:, j:j + 1] * w[:, j].unsqueeze(0)
    return acc


def _gen(*key):
    s = 0
    for v in key:
        s = (s * 1000003 + (int(v) if not isinstance(v, str) else sum(ord(ch) * (i + 1) for i, ch in enumerate(v)))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F32)


def _uni(g, *shape):
    return torch.rand(shape, generator=g, dtype=F64).mul(2).sub(1).to(F32)


def _sparse_pm1(g, n, k, nnz):
    """[n, k] with nnz entries of +-1 per row on the columns (row * nnz + j) mod k: the positions rotate with the row index, so every
    column is hit by some row as soon as n * nnz >= k."""
    w = torch.zeros((n, k), dtype=F32)
    nnz = min(nnz, k)
    sign = torch.randint(0, 2, (n, nnz), generator=g).to(F32) * 2 - 1
    for r in range(n):
        for j in range(nnz):
            w[r, (r * nnz + j) % k] = sign[r, j]
    return w


def _mixed(g, n, k):
    """Real-valued weights of the tail's layers: four entries per row uniform in +-1/2 on rotating columns, which carry a signal through
    six layers (gain about 0.6 a layer), over a dense uniform background of row sum 1/4, which puts a real product on every column.
    The row sums of |W| stay near 1.25, so a layer hardly amplifies the bound it inherits; dense weights of the same gain would
    multiply it by sqrt(k) / 2 a layer and leave a bound of percents on the logits."""
    return _sparse_pm1(g, n, k, 4) * _uni(g, n, k) * 0.5 + _uni(g, n, k) * (0.5 / k)


# ------------------------------------------------------------------------------------------------------------------ the block
def block_case(inst, rows, k1=None, src="idx", div2=1, rpb=None, per_batch=(False, False), kind="exact", variant=None, seed=0,
               strided=False, bf16=False, nx2=37):
    """One input of the block kernels.  kind: 'exact' | 'real'; variant (real): None | 'neg' | 'small' | 'zero'.
    strided: x1, x2 and the per-batch bias rows are column slices of wider buffers.  bf16: exact case whose operands are bf16-exact."""
    kx, ch, co, conv = inst
    k1 = kx if k1 is None else k1
    k2 = kx - k1
    rpb = rows if rpb is None else rpb
    nb = (rows + rpb - 1) // rpb
    g = _gen(kx, ch, co, rows, k1, div2, rpb, kind, variant or "", seed, src)
    c = types.SimpleNamespace(inst=inst, kx=kx, ch=ch, co=co, conv=conv, k1=k1, rows=rows, rpb=rpb, nb=nb, kind=kind, variant=variant,
                              slope=0.5 if kind == "exact" else 0.2, x2=None, idx2=None, div2=1, bf16=bf16)
    exact = kind == "exact"
    val = (lambda *s: _ints(g, -3, 3, *s)) if exact else (lambda *s: _uni(g, *s))

    def buf(r, w):
        if not strided:
            return val(r, w)
        return val(r, w + 8)[:, 4:4 + w]                          # 16-byte aligned column slice, ld = w + 8
    c.x1 = buf(rows, k1)
    if k2:
        if src == "idx":
            idx = torch.randint(0, nx2, (rows,), generator=g)
            idx[0] = nx2 - 1                                       # both extreme indices and a repeat
            if rows > 2:
                idx[1], idx[2] = 0, nx2 - 1
            c.idx2, n2 = idx.to(torch.int32), nx2
        else:
            c.div2, n2 = int(div2), (rows + div2 - 1) // div2
        c.x2 = buf(n2, k2)
    if exact:
        c.w1 = _sparse_pm1(g, ch, kx, 4) if bf16 else _ints(g, -1, 1, ch, kx)
        c.w2 = _ints(g, -1, 1, co, ch)
        c.wsc = _ints(g, -1, 1, co, kx) if conv else None
        bias = lambda n: _ints(g, -8, 8, *n)
    else:
        c.w1, c.w2 = _uni(g, ch, kx) * (REAL_ROW_SUM * 2 / kx), _uni(g, co, ch) * (REAL_ROW_SUM * 2 / ch)
        c.wsc = _uni(g, co, kx) * (REAL_ROW_SUM * 2 / kx) if conv else None
        bias = lambda n: _uni(g, *n)

    def brow(per, n):
        if not per:
            return bias((n,))
        if strided:
            return bias((nb, n + 8))[:, 4:4 + n]
        return bias((nb, n))
    c.b1, c.b2 = brow(per_batch[0], ch), brow(per_batch[1], co)
    if variant == "neg":                                          # an all-negative output column
        c.b2 = c.b2.clone()
        c.b2[..., co // 2 + 1] = -50.0
    elif variant == "small":                                      # a small-magnitude output column: column CO - 3 (past the identity shortcut's reach only in 64-128-128; in 64-64-64
        # every output column carries x through the shortcut, so there the variant only shrinks the column's W2 row and bias)
        ch_small = co - 3
        c.w2 = c.w2.clone()
        c.w2[ch_small] *= 1e-3
        c.b2 = c.b2.clone()
        c.b2[..., ch_small] *= 1e-3
        if conv:
            c.wsc = c.wsc.clone()
            c.wsc[ch_small] *= 1e-3
    elif variant == "zero":                                       # hidden pre-activations cluster around 0
        c.w1, c.b1 = c.w1 * 1e-2, c.b1 * 1e-3
    return c


def block_input(c, plant=None):
    """x = [x1[:, :k1] | x2[map(r)]], map = idx2[r] or r // div2  (the un-materialised torch.cat / gather of the block's callers)"""
    x1 = c.x1.to(F64)
    if c.x2 is None:
        return x1
    r = torch.arange(c.rows)
    m = c.idx2.long() if c.idx2 is not None else r // c.div2
    x2 = c.x2.to(F64)
    if plant == "gather_off":
        m = (m + 1) % x2.shape[0]
    if plant == "x2_col_k1":
        k2 = x2.shape[1]
        x2 = torch.roll(x2, -(c.k1 % k2 or 4), dims=1)
    return torch.cat([x1, x2[m]], 1)


def _bias_rows(b, c, plant=None):
    b = b.to(F64)
    if b.dim() == 1:
        return b.unsqueeze(0)
    r = torch.arange(c.rows)
    batch = r // c.rpb
    if plant == "bias_neighbour":                                 # every row of a tile takes the sample of the tile's first row
        batch = (r // TILE * TILE) // c.rpb
    return b[batch]


def block_ref(c, dtype=F64, order="matmul", bf16=False, plant=None):
    """PointNN.py:281-282 with eval-mode BatchNorm folded (the kernels' header formula).  -> namespace(x, hid, y) in `dtype`.
    bf16: the matrix-core operands -- x, the three weight matrices and hid -- rounded to bf16; shortcut and epilogue unrounded."""
    r = bf16_round if bf16 else (lambda t: t)
    t = lambda v: v.to(dtype)
    x = t(block_input(c, plant))
    pos = c.slope if plant == "slope_positive" else 1.0
    act = lambda v: torch.where(v > 0, v * pos, v * c.slope)
    hid = act(mm(r(x), r(t(c.w1)), order) + t(_bias_rows(c.b1, c, plant)))
    y = mm(r(hid), r(t(c.w2)), order) + t(_bias_rows(c.b2, c, plant))
    if c.conv:
        sc = mm(r(x), r(t(c.wsc)), order)
    else:
        sc = torch.zeros_like(y)
        sc[:, :c.kx] = x                                          # identity on the first KX output channels
    if plant == "shortcut_dropped":
        sc[:, 5] = 0
    return types.SimpleNamespace(x=x, hid=hid, y=act(y + sc))


def block_bound(c, ref=None):
    """-> (e_h, e_y): the a-priori element-wise bounds of the module docstring on hid and y."""
    ref = block_ref(c) if ref is None else ref
    ax, ah = ref.x.abs(), ref.hid.abs()
    w1, w2 = c.w1.to(F64).abs(), c.w2.to(F64).abs()
    e_h = gamma(c.kx + 1) * (ax.matmul(w1.t()) + _bias_rows(c.b1, c).abs()) + U * ah
    terms = ah.matmul(w2.t()) + _bias_rows(c.b2, c).abs()
    if c.conv:
        terms = terms + ax.matmul(c.wsc.to(F64).abs().t())
    else:
        terms[:, :c.kx] += ax
    e_y = e_h.matmul(w2.t()) + gamma(c.ch + c.kx + 2) * terms + U * ref.y.abs()
    return e_h, e_y


def block_exact_measure(c, quantum=1.0):
    """Largest sum of |terms| of any element of the two layers, in units of that layer's quantum (inputs are multiples of `quantum`,
    every LeakyReLU halves it).  Below 2^24: every partial sum in any order is an fp32 number."""
    ref = block_ref(c)
    ax, ah = ref.x.abs(), ref.hid.abs()
    s1 = ax.matmul(c.w1.to(F64).abs().t()) + _bias_rows(c.b1, c).abs()
    s2 = ah.matmul(c.w2.to(F64).abs().t()) + _bias_rows(c.b2, c).abs()
    if c.conv:
        s2 = s2 + ax.matmul(c.wsc.to(F64).abs().t())
    else:
        s2[:, :c.kx] += ax
    return max(float(s1.max()) / quantum, float(s2.max()) / (quantum * c.slope), float(ref.y.abs().max()) / (quantum * c.slope ** 2))


def bf16_exact_operands(c):
    """The operands the bf16 kernel rounds, for the CPU tier's `bf16(t) == t`."""
    ref = block_ref(c)
    return [ref.x, c.w1.to(F64), c.w2.to(F64), ref.hid] + ([c.wsc.to(F64)] if c.conv else [])


def tile_max(y, plant=None):
    """Per-tile maxima [ceil(rows / 32), C]: tiles of 32 consecutive rows, rows past the end left out."""
    rows, C = y.shape
    nt = (rows + TILE - 1) // TILE
    pad = torch.full((nt * TILE - rows, C), -math.inf, dtype=y.dtype)
    if plant == "tile_max_masked" and pad.shape[0]:
        pad = y[:1].expand(pad.shape[0], C)                       # the kernel's masked lanes recompute row 0
    return torch.cat([y, pad], 0).view(nt, TILE, C).max(1)[0]


def fold(part, B, tiles_per_batch, plant=None):
    """[B * tiles_per_batch, C] -> [B, C]: maximum over each sample's consecutive tiles."""
    if plant == "fold_next":                                      # the last tile of a sample goes to the next one
        t = torch.arange(B * tiles_per_batch)
        owner = ((t + 1) // tiles_per_batch).clamp(max=B - 1)
        return torch.stack([part[owner == b].max(0)[0] for b in range(B)])
    return part.view(B, tiles_per_batch, -1).max(1)[0]


def glue_case(B, tiles_per_batch, n1, n2, kind="exact", variant=None, seed=0):
    """Input of cmr_colmax_bias2_f32: per-tile maxima [B * tiles_per_batch, 64] and the two weight / bias pairs.
    variant 'neginf': some tiles are -inf throughout (a tile of masked rows) and one column is negative in every tile."""
    g = _gen(B, tiles_per_batch, n1, n2, kind, variant or "", seed)
    c = types.SimpleNamespace(B=B, tpb=tiles_per_batch, n1=n1, n2=n2, kind=kind)
    if kind == "exact":
        c.part = _ints(g, -40, 40, B * tiles_per_batch, 64) * 0.25
        c.w1, c.w2 = _ints(g, -1, 1, n1, 64), _ints(g, -1, 1, n2, 64)
        c.b1, c.b2 = _ints(g, -8, 8, n1), _ints(g, -8, 8, n2)
    else:
        c.part = _uni(g, B * tiles_per_batch, 64) * 3
        c.w1, c.w2 = _uni(g, n1, 64) * (REAL_ROW_SUM * 2 / 64), _uni(g, n2, 64) * (REAL_ROW_SUM * 2 / 64)
        c.b1, c.b2 = _uni(g, n1), _uni(g, n2)
    if variant == "neginf":
        c.part[:, 7] = -c.part[:, 7].abs() - 1
        if tiles_per_batch > 1:
            c.part.view(B, tiles_per_batch, 64)[:, 1::2] = -math.inf      # every second tile of a sample; its tile 0 stays finite
    return c


def glue_ref(c, dtype=F64, order="matmul", g_err=None):
    """-> (g [B, 64], g W1^T + b1, g W2^T + b2) and, with g_err (the bound on g, zeros when the partials are data), their bounds."""
    g = fold(c.part.to(dtype), c.B, c.tpb)
    y1 = mm(g, c.w1.to(dtype), order) + c.b1.to(dtype)
    y2 = mm(g, c.w2.to(dtype), order) + c.b2.to(dtype)
    if g_err is None:
        return g, y1, y2
    bound = lambda w, b, y: g_err.matmul(w.to(F64).abs().t()) + gamma(64 + 1) * (g.abs().matmul(w.to(F64).abs().t()) + b.to(F64).abs()) + U * y.abs()
    return g, y1, y2, bound(c.w1, c.b1, y1), bound(c.w2, c.b2, y2)


def glue_exact_measure(c):
    g = fold(c.part.to(F64), c.B, c.tpb)
    return max(float((g.abs().matmul(w.to(F64).abs().t()) + b.to(F64).abs()).max()) for w, b in ((c.w1, c.b1), (c.w2, c.b2))) / 0.25


# ------------------------------------------------------------------------------------------------------------------ the 3-D branch
def chain_case(B, N, kind="exact", seed=0, f=64):
    """Weights of CMRAgent.state_3d_embed as its nn layers hold them (BatchNorm at identity: the test writes them into the conv layers) and
    an input [B, N, 5].  Per block: (W1 [cin, cin], b1, W2 [cout, cin], b2, (Wsc [cout, cin], bsc) or None)."""
    g = _gen(B, N, kind, seed, "chain")
    dims = ((5, f), (2 * f, f), (2 * f, f), (2 * f, 2 * f))
    c = types.SimpleNamespace(B=B, N=N, kind=kind, slope=0.5 if kind == "exact" else 0.2, blocks=[])
    exact = kind == "exact"
    c.x = _ints(g, -2, 2, B, N, 5) if exact else _uni(g, B, N, 5)
    for ci, co in dims:
        if exact:
            mk = lambda n, k: _sparse_pm1(g, n, k, 2 if k > 8 else 3)
            bb = lambda n: _ints(g, -2, 2, n)
        else:
            mk = lambda n, k: _uni(g, n, k) / k ** 0.5
            bb = lambda n: _uni(g, n)
        c.blocks.append((mk(ci, ci), bb(ci), mk(co, ci), bb(co), None if ci == co else (mk(co, ci), bb(co))))
    return c


def chain_ref(c, dtype=F64, measure=False, order="matmul"):
    """CMRAgent.py:92-101: four blocks, cat([feat, broadcast(max over the points)]) in front of blocks 1..3, final max -> [B, 2f].
    measure: -> the largest sum of |terms| in units of the layer's quantum instead (exact cases)."""
    feat = c.x.to(dtype)
    worst, q = 0.0, 1.0
    act = lambda v: torch.where(v > 0, v, v * c.slope)
    for i, (w1, b1, w2, b2, sc) in enumerate(c.blocks):
        if i > 0:
            gmax = feat.max(1, keepdim=True)[0]
            feat = torch.cat([feat, gmax.expand(-1, c.N, -1)], 2)
        t = lambda v: v.to(dtype)
        pm = lambda v, w: mm(v.reshape(-1, v.shape[2]), w, order).view(c.B, c.N, -1)
        hid = act(pm(feat, t(w1)) + t(b1))
        y = pm(hid, t(w2)) + t(b2)
        res = feat if sc is None else pm(feat, t(sc[0])) + t(sc[1])
        if measure:
            s1 = feat.abs().matmul(t(w1).abs().t()) + t(b1).abs()
            s2 = hid.abs().matmul(t(w2).abs().t()) + t(b2).abs() + (feat.abs() if sc is None else feat.abs().matmul(t(sc[0]).abs().t()) + t(sc[1]).abs())
            worst = max(worst, float(s1.max()) / q, float(s2.max()) / (q * c.slope))
            q *= c.slope ** 2
        feat = act(y + res)
    return worst if measure else feat.max(1)[0]


# ------------------------------------------------------------------------------------------------------------------ the tail
PRODUCT_HEADS = ((256, 256, 36), (256, 256, 24), (64, 64, 4))
# name -> (three (n0, n1, n2), num_steps, degree_r, degree_t, served by the transposed kernel)
TAIL_WIDTHS = {
    "product": (PRODUCT_HEADS, 12, 3, 2, True),
    "w16": (((16, 16, 1),) * 3, 1, 1, 1, True),
    "wide": (((240, 16, 255), (256, 240, 100), (16, 16, 1)), 5, 51, 20, True),
    "tiny": (((4, 12, 3),) * 3, 3, 1, 1, False),
}


def tail_case(B, npix, widths="product", kind="exact", variant=None, seed=0):
    """variant: None | 'ties' (exact: zero last layers, the logits are the biases, with two equal maxima per group) |
    'mean1000' (real: feature map 1000 +- 1) | 'contract' (real: dense weights with row sums of |W| 1/8, whose bound meets 2e-5)."""
    heads_w, S, dr, dt, _ = TAIL_WIDTHS[widths]
    g = _gen(B, npix, widths, kind, variant or "", seed, "tail")
    c = types.SimpleNamespace(B=B, npix=npix, widths=widths, kind=kind, variant=variant, S=S, dr=dr, dt=dt,
                              slope=0.5 if kind == "exact" else 0.01, heads=[])
    if kind == "exact":
        x = _ints(g, -2, 2, B, npix, 128)
        mean = _ints(g, -2, 2, B, 128)
        x[:, -1] = 0
        x[:, -1] = mean * npix - x.sum(1)                         # every channel sum is mean * npix: every pixel carries weight
        c.x = x.view(B * npix, 128)
        c.e3d = _ints(g, -4, 4, B, 128)
        lin = lambda n, k: (_sparse_pm1(g, n, k, max(3, -(-k // n))), _ints(g, -2, 2, n))
    else:
        c.x = (_uni(g, B * npix, 128) + (1000.0 if variant == "mean1000" else 0.0)).to(F32)
        c.e3d = _uni(g, B, 128)
        if variant == "contract":                                 # built as the block's real-valued cases are: dense, row sums of |W| 1/8
            c.row_sum = 0.125
            lin = lambda n, k: (_uni(g, n, k) * (2 * 0.125 / k), _uni(g, n))
        else:
            c.row_sum = 1.25                                      # _mixed: 4 x 1/4 + 1/4
            lin = lambda n, k: (_mixed(g, n, k), _uni(g, n))
    c.c24, c.c26 = lin(128, 128), lin(128, 128)
    for n0, n1, n2 in heads_w:
        l2 = lin(n2, n1)
        if variant == "contract":                                 # a logit is its bias and little else: keep every column's scale off zero
            l2 = (l2[0], torch.sign(l2[1]) * (0.5 + 0.5 * l2[1].abs()))
        if variant == "ties":
            b = _ints(g, -2, 2, n2)
            for grp in range(n2 // S):
                if S >= 3:
                    b[grp * S + 1] = b[grp * S + S - 1] = 5       # two equal maxima: the first one wins
            l2 = (torch.zeros_like(l2[0]), b)
        c.heads.append((lin(n0, 256), lin(n1, n0), l2))
    return c


def argmax_first(logits, d, S, last=False):
    """CMRAgent.py:118-123: argmax per group of S logits of the first d * S, the FIRST maximum on ties (torch.argmax's documented choice)."""
    v = logits[:, :d * S].reshape(logits.shape[0], d, S)
    if last:
        return S - 1 - torch.flip(v, (2,)).argmax(2)
    m = v.max(2, keepdim=True)[0]
    return (v == m).to(torch.int64).argmax(2)                     # first index where the maximum is met


def tail_ref(c, dtype=F64, order="matmul", plant=None, bounds=False):
    """-> namespace(pooled, t1, e2d, state, heads [(h0, h1, logits)], acts (r, t)) -- the intermediates are the ones cmr_agent_heads_train_f32
    saves; with bounds=True also .e_logits [3] and .e_saves (pooled, t1, e2d, [(h0, h1)]) by the layer-by-layer rule of the module docstring."""
    t = lambda v: v.to(dtype)
    act = lambda v: torch.where(v > 0, v, v * c.slope)
    x = t(c.x).view(c.B, c.npix, 128)
    if plant == "pool_skip":
        x = x[:, :-1] if c.npix > 1 else x * 0
    if order == "matmul":
        s = x.sum(1)
    else:
        s = torch.zeros((c.B, 128), dtype=dtype)
        for p in (range(x.shape[1]) if order == "forward" else range(x.shape[1] - 1, -1, -1)):
            s = s + x[:, p]
    pooled = s / c.npix                                           # AvgPool2d((H, W)) (CMRAgent.py:57)
    e = {}
    if bounds:
        e["pooled"] = gamma(c.npix + 1) * x.abs().sum(1) / c.npix

    def layer(v, wb, lrelu_, name, k, drop=False):
        w, b = t(wb[0]), t(wb[1])
        if drop:                                                  # one input slice of the layer (columns [5 k / 16, 6 k / 16)) dropped
            w = w.clone()
            w[:, 5 * k // 16:max(6 * k // 16, 5 * k // 16 + 1)] = 0
        y = mm(v, w, order) + b
        y = act(y) if lrelu_ else y
        if bounds:
            e[name] = e[e["_in"]].matmul(w.abs().t()) + gamma(k + 1) * (v.abs().matmul(w.abs().t()) + b.abs()) + U * y.abs()
        return y
    e["_in"] = "pooled"
    t1 = layer(pooled, c.c24, True, "t1", 128)
    e["_in"] = "t1"
    e2d = layer(t1, c.c26, False, "e2d", 128)
    e3d = t(c.e3d)
    state = torch.cat([e3d, e2d], 1) if plant == "halves_swapped" else torch.cat([e2d, e3d], 1)      # CMRAgent.py:103
    if bounds:
        e["state"] = torch.cat([e["e2d"], torch.zeros_like(e3d)], 1)
    out = types.SimpleNamespace(pooled=pooled, t1=t1, e2d=e2d, state=state, heads=[], e_logits=[], e_saves=None)
    e_hid = []
    for i, (l0, l1, l2) in enumerate(c.heads):
        e["_in"] = "state"
        h0 = layer(state, l0, True, "h0", 256, drop=(plant == "head_slice_dropped" and i == 0))
        e["_in"] = "h0"
        h1 = layer(h0, l1, True, "h1", l0[0].shape[0])
        e["_in"] = "h1"
        lg = layer(h1, l2, False, "lg", l1[0].shape[0])
        out.heads.append((h0, h1, lg))
        if bounds:
            out.e_logits.append(e["lg"])
            e_hid.append((e["h0"], e["h1"]))
    if bounds:
        out.e_saves = (e["pooled"], e["t1"], e["e2d"], e_hid)
    last = plant == "argmax_last"
    out.acts = (argmax_first(out.heads[0][2], c.dr, c.S, last), argmax_first(out.heads[1][2], c.dt, c.S, last))
    return out


def tail_exact_measure(c):
    """Largest sum of |terms| of any layer in units of its quantum (1 for the pool and the first 1x1 conv, halved by every LeakyReLU)."""
    r = tail_ref(c)
    a = lambda wb, v: float((v.abs().matmul(wb[0].to(F64).abs().t()) + wb[1].to(F64).abs()).max())
    worst = max(float(c.x.to(F64).abs().view(c.B, c.npix, 128).sum(1).max()), a(c.c24, r.pooled), a(c.c26, r.t1) / 0.5)
    for (l0, l1, l2), (h0, h1, _) in zip(c.heads, r.heads):
        worst = max(worst, a(l0, r.state) / 0.5, a(l1, h0) / 0.25, a(l2, h1) / 0.125)
    return worst


def compared_groups(logits, bound, d, S):
    """The argmax comparison rule: a group is compared only where the float64 margin between its two largest logits exceeds the sum of
    their two bounds; the caller passes its bar (2 x the a-priori bound) as `bound`.  -> bool [B, d]."""
    B = logits.shape[0]
    v = logits[:, :d * S].reshape(B, d, S)
    e = bound[:, :d * S].reshape(B, d, S)
    if S == 1:
        return torch.ones((B, d), dtype=torch.bool)
    top, pos = v.topk(2, dim=2)
    return (top[..., 0] - top[..., 1]) > e.gather(2, pos).sum(2)


# ------------------------------------------------------------------------------------------------------------------ comparisons
def close_exact(got, want, what=""):
    """Bitwise comparison of `got` (fp32) with `want` (float64 values that are fp32 numbers).  -> (ok, message); the message names the first
    differing row / column and where it sits in the block kernels' tiling (tile, row within the tile, half-wave of the column)."""
    got = got.detach().cpu()
    want = want.detach().cpu()
    if tuple(got.shape) != tuple(want.shape):
        return False, "%s: shape %s, want %s" % (what, tuple(got.shape), tuple(want.shape))
    w32 = want.to(F32)
    if not torch.equal(w32.to(F64), want.to(F64)):
        return False, "%s: the reference is not an fp32 number everywhere" % what
    same = (got.to(F32).view(torch.int32) == w32.view(torch.int32)) if got.dtype == F32 else (got == want)
    if bool(same.all()):
        return True, ""
    bad = (~same).reshape(same.shape[0], -1) if same.dim() > 1 else (~same).reshape(-1, 1)
    r, col = [int(v) for v in bad.nonzero()[0]]
    g2, w2 = got.reshape(bad.shape), want.reshape(bad.shape)
    return False, "%s: %d of %d differ, first at row %d col %d (tile %d, row %d of the tile, column group %d half %d): got %r want %r" % (
        what, int(bad.sum()), bad.numel(), r, col, r // TILE, r % TILE, col // 8, (col // 4) % 2, float(g2[r, col]), float(w2[r, col]))


def close_bounded(got, want, bound, factor=2.0, what=""):
    """|got - want| <= factor * bound element-wise (equal infinities agree).  -> (ok, worst error / bound, message)."""
    got = got.detach().cpu().to(F64)
    want, bound = want.to(F64), bound.to(F64)
    if tuple(got.shape) != tuple(want.shape):
        return False, math.inf, "%s: shape %s, want %s" % (what, tuple(got.shape), tuple(want.shape))
    err = torch.where(got == want, torch.zeros_like(want), (got - want).abs())
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst <= factor:
        return True, worst, ""
    flat = ratio.reshape(ratio.shape[0], -1)
    r, col = [int(v) for v in (flat == flat.max()).nonzero()[0]]
    return False, worst, "%s: error / bound = %.3g at row %d col %d (tile %d, row %d of the tile): got %r want %r bound %.3g" % (
        what, worst, r, col, r // TILE, r % TILE, float(got.reshape(flat.shape)[r, col]), float(want.reshape(flat.shape)[r, col]),
        float(bound.reshape(flat.shape)[r, col]))


# ------------------------------------------------------------------------------------------------------------------ planted errors
PLANTED = ("bias_neighbour", "shortcut_dropped", "slope_positive", "gather_off", "x2_col_k1", "tile_max_masked", "fold_next", "pool_skip",
           "halves_swapped", "argmax_last", "head_slice_dropped")


def planted(kind, real=False):
    """A wrong result of the named kind next to the right one: -> list of (got, want, bound or None) for the comparison that has to
    reject it (close_exact on an exact case; with real=True close_bounded on a real-valued one; actions are compared with torch.equal)."""
    k = "real" if real else "exact"
    if kind in ("bias_neighbour", "shortcut_dropped", "slope_positive", "gather_off", "x2_col_k1", "tile_max_masked"):
        inst = INSTANCES[0] if kind in ("shortcut_dropped", "gather_off", "x2_col_k1") else INSTANCES[2]
        two = kind in ("gather_off", "x2_col_k1")
        c = block_case(inst, 261 if kind == "tile_max_masked" else 200, k1=32 if two else None, rpb=40 if kind == "bias_neighbour" else None,
                       per_batch=(True, True) if kind == "bias_neighbour" else (False, False), kind=k, seed=5)
        good = block_ref(c)
        e_y = block_bound(c, good)[1] if real else None
        if kind == "tile_max_masked":
            return [(tile_max(good.y, plant=kind), tile_max(good.y), tile_max(e_y) if real else None)]
        return [(block_ref(c, plant=kind).y, good.y, e_y)]
    if kind == "fold_next":
        c = glue_case(3, 2, 128, 64, kind=k, seed=5)
        part = c.part.to(F64)
        return [(fold(part, 3, 2, plant=kind), fold(part, 3, 2), torch.zeros((3, 64), dtype=F64) + 1e-30 if real else None)]
    c = tail_case(2, 33, "product", kind=k, variant="ties" if kind == "argmax_last" else None, seed=5)
    good, bad = tail_ref(c, bounds=real), tail_ref(c, plant=kind)
    if kind == "argmax_last":
        return [(bad.acts[0], good.acts[0], None), (bad.acts[1], good.acts[1], None)]
    if kind == "pool_skip":                                       # seen where the training forward saves it: the layers behind it contract
        out = [(bad.pooled, good.pooled, good.e_saves[0] if real else None)]
        if not real:                                              # exact: every pixel carries weight, the logits of both policies move too
            out += [(bad.heads[i][2], good.heads[i][2], None) for i in (0, 1)]
        return out
    heads = (0,) if kind == "head_slice_dropped" else (0, 1, 2)
    return [(bad.heads[i][2], good.heads[i][2], good.e_logits[i] if real else None) for i in heads]


# ------------------------------------------------------------------------------------------------------------------ case tables
BLOCK_TABLES = ("rows", "second_pass", "third_pass", "sources", "biases", "colmax", "guards")
K1_SPLITS = {64: (32, 36), 8: (4,), 128: (64, 100)}


def block_table(inst, name, bf16=False):
    """The cases of one GPU test of the block, as (kind, block_case keywords): both tiers iterate these."""
    kx = inst[0]
    out = []
    if name == "rows":
        for rows in ROWS:
            out += [(k, dict(rows=rows, variant=v)) for k, v in (("exact", None), ("real", None), ("real", "neg"), ("real", "small"), ("real", "zero"))]
    elif name == "second_pass":
        out = [(k, dict(rows=wrap_rows(inst, bf16), k1=kx // 2, src="idx", nx2=1001)) for k in ("exact", "real")]
    elif name == "third_pass":
        out = [(k, dict(rows=262183, k1=32, src="idx", nx2=4099)) for k in ("exact", "real")] if inst == INSTANCES[0] else []
    elif name == "sources":
        for k1 in K1_SPLITS[kx]:
            for k in ("exact", "real"):
                out += [(k, dict(rows=261, k1=k1, src="idx", strided=st)) for st in (False, True)]
                out += [(k, dict(rows=261, k1=k1, src="div", div2=d, strided=(d == 7))) for d in (1, 7, 40, 261)]
    elif name == "biases":
        for rows, rpb, pb, st in ((640, 40, (True, True), False), (16, 1, (True, True), False), (630, 40, (True, True), True),
                                  (640, 40, (True, False), False), (640, 40, (False, True), True)):
            out += [(k, dict(rows=rows, rpb=rpb, per_batch=pb, strided=st)) for k in ("exact", "real")]
    elif name == "colmax":
        for B, rpb in ((1, 32), (5, 32), (16, 32), (2, 32 * 513)):
            out += [(k, dict(rows=B * rpb, rpb=rpb, per_batch=(True, True), variant="neg" if k == "real" else None)) for k in ("exact", "real")]
    elif name == "guards":
        out = [(k, dict(rows=261, k1=kx // 2, src="idx", rpb=40, per_batch=(True, True))) for k in ("exact", "real")]
    return out


def table_case(inst, kind, kw, bf16=False):
    kw = dict(kw)
    return block_case(inst, kw.pop("rows"), kind=kind, bf16=(bf16 and kind == "exact"), **kw)


def glue_table():
    """(B, tiles per batch, kind, variant) of the glue launch's GPU test, per (n1, n2) of GLUE_WIDTHS."""
    return [(B, tpb, kind, v) for tpb in TILES_PER_BATCH for v in (None, "neginf") for B, kind in ((3, "exact"), (5, "real"))]


CHAIN_SHAPES = ((1, 32, True), (3, 32, True), (16, 32, True), (1, 64, True), (3, 64, True), (16, 64, True), (1, 2080, True), (3, 2080, True),
                (16, 2080, True), (3, 40, False), (17, 64, False))          # (B, N, served by the fused chain)


def tail_table(kind):
    """(B, npix, variant) of the tail's GPU tests, per entry of TAIL_WIDTHS; every case is built with seed=REAL_SEED."""
    variants = (None,) if kind == "exact" else (None, "contract")
    return [(B, npix, v) for B in (1, 3) for npix in NPIX for v in variants]
