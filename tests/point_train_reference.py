"""Plain CPU restatements of the train-mode point ops (float64 torch unless a dtype is asked for), the comparisons the GPU tests make
with them, and the inputs of those tests -- so that tests/test_point_train_cpu.py can show, without a GPU, that every comparison rejects a
wrong result and that fp32 evaluation of the same formulas stays inside every tolerance.

Formulas: the vector-attention front is PointNN.py:151-170 (group transformer) / 219-226 (kNN transformer) per (point, node) /
(node, neighbour) row; the three-neighbour interpolation is pointnet_util.py:287-296; the segment reductions have torch_scatter's
semantics (an empty segment gives 0).  No GPU import in this file."""
import torch
import torch.nn.functional as F

f32, f64 = torch.float32, torch.float64


def rnd(*shape, seed=0, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def randint(n, size, seed):
    return torch.randint(0, n, (size,), generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------------------------------------ front
FRONT_KEYS = ("x", "k", "v", "hd_pre", "hd", "pos", "t", "g1_pre", "g1", "a", "vp")


def _map(n, idx, div):
    """row map of the kernel: idx[r] when an index is given, else r // div"""
    return idx.long() if idx is not None else torch.arange(n) // div


def front(w, q, pa, pb, ib, feat=None, k=None, v=None, ikv=None, iq=None, divq=1, ia=None, diva=1, dtype=f64):
    """The per-row front of a vector-attention layer.  w: dict of d0, d2, g0, g2 = (W [n, k], b [n]) and, with `feat`, fc1 = (W, b), wk, wv
    [64, 64].  k / v: computed from feat (x = fc1(feat), k = Wk x, v = Wv x) or given -- per row, or per-node tables read through ikv.
    q row = iq[r] or r // divq; pa row = ia[r] or r // diva; pb row = ib[r].  Positions may carry a 4th padding column (ignored), d0's W a
    zero 4th column.  -> dict of FRONT_KEYS (x is None when k / v are given)."""
    c = lambda t: t.to(dtype)
    lin = lambda t, wb: t @ c(wb[0]).T + c(wb[1])
    rows = ib.numel()
    if feat is not None:
        x = lin(c(feat), w["fc1"])
        kk, vv = x @ c(w["wk"]).T, x @ c(w["wv"]).T
    else:
        x = None
        rk = ikv.long() if ikv is not None else torch.arange(rows)
        kk, vv = c(k)[rk], c(v)[rk]
    rel = c(pa)[_map(rows, ia, diva), :3] - c(pb)[ib.long(), :3]
    hd_pre = rel @ c(w["d0"][0])[:, :3].T + c(w["d0"][1])
    hd = F.relu(hd_pre)
    pos = lin(hd, w["d2"])
    t = c(q)[_map(rows, iq, divq)] - kk + pos
    g1_pre = lin(t, w["g0"])
    g1 = F.relu(g1_pre)
    return dict(x=x, k=kk, v=vv, hd_pre=hd_pre, hd=hd, pos=pos, t=t, g1_pre=g1_pre, g1=g1, a=lin(g1, w["g2"]), vp=vv + pos)


def front_weights(seed=60, with_kv=True):
    """weights uniform in +-0.3, biases in +-1: the distribution of test_vector_attention_front_fused"""
    lin = lambda n, k, sd: (rnd(n, k, seed=sd, lo=-0.3, hi=0.3), rnd(n, seed=sd + 1))
    w = dict(d0=lin(64, 3, seed), d2=lin(64, 64, seed + 2), g0=lin(64, 64, seed + 4), g2=lin(64, 64, seed + 6))
    if with_kv:
        w.update(fc1=lin(64, 64, seed + 14), wk=rnd(64, 64, seed=seed + 16, lo=-0.3, hi=0.3), wv=rnd(64, 64, seed=seed + 17, lo=-0.3, hi=0.3))
    return w


# (rows, mode, k/v source, strided operands).  rows: one tile with seven idle waves; two workgroups, the second with one live wave; the
# smallest size whose second trip of the persistent loop runs with a partly idle grid: 256 workgroups x 8 tiles x 32 rows + 288 with
# computed k/v, 512 x 8 x 32 + 96 with gathered k/v.
FRONT_KV_CASES = [(32, "group", "feat", False), (288, "knn", "feat", True), (288, "group", "feat", True), (65536 + 288, "group", "feat", True)]
FRONT_CASES = [(32, "group", "rows", False), (288, "group", "rows", True), (288, "knn", "table", True), (131072 + 96, "knn", "table", True)]


def front_case(rows, mode, kv, strided, seed=70):
    """-> (weights, operands of front()) of one case.  group: q and pb are per-node tables read through iq and ib -- two independent maps, so that one read through
    the other's shows -- and pa is per row.  knn: 16 rows per node, q and pa by r // 16, pb through ib (the neighbour).  kv "feat": computed from per-row features; "rows":
    given per row; "table": per-node tables through ikv = ib.  strided: q | k | v are the column blocks of one [*, 192] buffer where they
    share their rows (else k | v of one, q contiguous), feat is a column slice of a [rows, 128] buffer."""
    w = front_weights(with_kv=kv == "feat")
    S = max(rows // 16, 2) if mode == "knn" else 37
    o = dict(ib=randint(S, rows, seed + 5).int(), pb=rnd(S, 4, seed=seed + 3, lo=-5, hi=5))
    if mode == "group":
        o.update(iq=randint(S, rows, seed + 4).int(), pa=rnd(rows, 4, seed=seed + 2, lo=-5, hi=5))
    else:
        o.update(divq=16, diva=16, pa=o["pb"])
    nq = S
    if kv == "feat":
        o["feat"] = rnd(rows, 128, seed=seed)[:, 32:96] if strided else rnd(rows, 64, seed=seed)
        o["q"] = rnd(nq, 192, seed=seed + 1)[:, 0:64] if strided else rnd(nq, 64, seed=seed + 1)
        return w, o
    nkv = S if kv == "table" else rows
    if kv == "table":
        o["ikv"] = o["ib"]
    if strided and nkv == nq:
        buf = rnd(nq, 192, seed=seed + 1)
        o.update(q=buf[:, 0:64], k=buf[:, 64:128], v=buf[:, 128:192])
    elif strided:
        buf = rnd(nkv, 192, seed=seed + 6)
        o.update(q=rnd(nq, 64, seed=seed + 1), k=buf[:, 64:128], v=buf[:, 128:192])
    else:
        o.update(q=rnd(nq, 64, seed=seed + 1), k=rnd(nkv, 64, seed=seed + 6), v=rnd(nkv, 64, seed=seed + 7))
    return w, o


FRONT_RTOL = 2e-5          # of each output's own largest entry: the bar of test_vector_attention_front_fused, same arithmetic
MASK_BAND = 1e-5           # x the largest pre-activation magnitude: inside it the sign of a pre-activation is not decided by fp32
MASK_BAND_CAP = 1e-3       # share of the entries the band may hold


def rel_err(got, ref):
    """max |got - ref| over the largest |ref| (the `close` of test_ops_gpu.py as a number)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs().max()
    return float("inf") if not bool(torch.isfinite(err)) else float(err) / max(float(ref.abs().max()), 1e-6)


def close(got, ref, rtol, name=""):
    e = rel_err(got, ref)
    assert e <= rtol, "%s: max|d| / scale = %.3e > %.1e" % (name, e, rtol)
    return e


def relu_mask_agrees(got, ref_pre, band):
    """got: a stored ReLU output; ref_pre: the float64 pre-activation.  -> (entries with (got > 0) != (ref_pre > 0) and |ref_pre| > band,
    share of the entries with |ref_pre| <= band)."""
    got, ref_pre = got.detach().cpu(), ref_pre.detach().cpu()
    assert got.shape == ref_pre.shape
    inside = ref_pre.abs() <= band
    wrong = ((got > 0) != (ref_pre > 0)) & ~inside
    return int(wrong.sum()), float(inside.double().mean())


def check_front(got, ref):
    """got: dict of the kernel's outputs (a, vp, hd, t, g1 and, where computed, x) against front()'s dict."""
    figs = {}
    for key, val in got.items():
        figs[key] = close(val, ref[key], FRONT_RTOL, key)
    for key in ("hd", "g1"):
        pre = ref[key + "_pre"]
        wrong, share = relu_mask_agrees(got[key], pre, MASK_BAND * float(pre.abs().max()))
        figs[key + "_band_share"] = share
        assert share <= MASK_BAND_CAP, "%s: the band holds %.2e of the entries" % (key, share)
        assert wrong == 0, "%s: %d mask entries differ outside the band" % (key, wrong)
    return figs


# --------------------------------------------------------------------------------------------------------------------------- three_nn
def sqdist3(q, c):
    """fp32 squared distances [B, Nq, Nc] in the kernel's order of operations, (dx dx + dy dy) + dz dz, every product rounded on its own"""
    d = q.float()[:, :, None, :3] - c.float()[:, None, :, :3]
    p = d * d
    return (p[..., 0] + p[..., 1]) + p[..., 2]


def three_nn(q, c):
    """q [B, Nq, 3+], c [B, Nc, 3+] -> (idx int64 [B * Nq, 3] GLOBAL candidate rows b * Nc + local, wgt float64 [B * Nq, 3]): the three
    nearest candidates in ascending distance, ties to the smaller index, weights 1 / (d + 1e-8) normalised.  With Nc < 3 the missing
    neighbours have weight 0 (and index b * Nc: any row of the batch element would do)."""
    B, Nq, Nc = q.shape[0], q.shape[1], c.shape[1]
    d = sqdist3(q, c)
    order = torch.sort(d, dim=2, stable=True)[1][:, :, :3]
    n = order.shape[2]
    dn = torch.gather(d, 2, order)
    r = 1.0 / (dn.double() + float(torch.tensor(1e-8, dtype=f32)))
    wgt = torch.zeros(B, Nq, 3, dtype=f64)
    wgt[:, :, :n] = r / r.sum(2, keepdim=True)
    idx = torch.zeros(B, Nq, 3, dtype=torch.int64)
    idx[:, :, :n] = order
    idx += torch.arange(B).view(B, 1, 1) * Nc
    return idx.view(-1, 3), wgt.view(-1, 3)


def three_nn_weights_fp32(q, c, idx):
    """the weights as fp32 arithmetic gives them, in the kernel's order: (r0 + r1) + r2"""
    B, Nq, Nc = q.shape[0], q.shape[1], c.shape[1]
    n = min(Nc, 3)
    local = (idx.view(B, Nq, 3) - torch.arange(B).view(B, 1, 1) * Nc)[:, :, :n]
    dn = torch.gather(sqdist3(q, c), 2, local)
    r = torch.zeros(B, Nq, 3, dtype=f32)
    r[:, :, :n] = 1.0 / (dn + torch.tensor(1e-8, dtype=f32))
    norm = (r[..., 0] + r[..., 1]) + r[..., 2]
    return (r / norm[..., None]).view(-1, 3)


def lattice_cloud(B, N, seed):
    """points with integer coordinates in {-3..3}^3 (every squared distance exact in fp32, ties everywhere); distinct points while the
    lattice has enough of them"""
    g = torch.Generator().manual_seed(seed + N)
    if N <= 343:
        cell = torch.stack([torch.randperm(343, generator=g)[:N] for _ in range(B)])
    else:
        cell = torch.randint(0, 343, (B, N), generator=g)
    return torch.stack([cell // 49, cell // 7 % 7, cell % 7], 2).float() - 3.0


def three_nn_case(kind, B, Nq, Nc, seed=90):
    """-> (q [B, Nq, 3], c [B, Nc, 3]).  Query 0 of every batch element sits on candidate 0."""
    if kind == "lattice":
        q, c = lattice_cloud(B, Nq, seed), lattice_cloud(B, Nc, seed + 1)
    else:
        q, c = rnd(B, Nq, 3, seed=seed, lo=-20, hi=20), rnd(B, Nc, 3, seed=seed + 1, lo=-20, hi=20)
    q[:, 0] = c[:, 0]
    return q, c


THREE_NN_WGT_RTOL = 1e-5   # of each float64 weight


def check_three_nn(idx, wgt, q, c):
    """idx / wgt of a three_nn implementation against the restatement: indices exact where a neighbour exists, a valid row of the same
    batch element with weight exactly 0 where none does; weights to 1e-5 of each float64 weight; a zero distance takes all the weight."""
    B, Nq, Nc = q.shape[0], q.shape[1], c.shape[1]
    n = min(Nc, 3)
    ridx, rwgt = three_nn(q, c)
    idx, wgt = idx.detach().cpu().long().view(-1, 3), wgt.detach().cpu().double().view(-1, 3)
    bad = (idx[:, :n] != ridx[:, :n]).any(1)
    assert not bool(bad.any()), "%d of %d queries with other neighbours, first at row %d" % (int(bad.sum()), B * Nq, int(bad.nonzero()[0]))
    base = (torch.arange(B * Nq) // Nq * Nc).view(-1, 1)
    assert bool(((idx >= base) & (idx < base + Nc)).all()), "an index outside the query's batch element"
    assert bool((wgt[:, n:] == 0).all()), "a missing neighbour with a non-zero weight"
    err = ((wgt - rwgt).abs() / rwgt.clamp_min(1e-300))[:, :n]
    assert float(err.max()) <= THREE_NN_WGT_RTOL, "weights: relative error %.3e" % float(err.max())
    d = torch.gather(sqdist3(q, c).view(B * Nq, Nc), 1, ridx[:, :n] - base)
    on = d[:, 0] == 0
    assert bool(on.view(B, Nq)[:, 0].all())
    share = (wgt[:, :n] * (d == 0)).sum(1)[on]
    assert float((share - 1).abs().max()) <= 1e-6, "a zero distance does not take all the weight"
    return float(err.max())


# ------------------------------------------------------------------------------------------------------- gather3 / scatter3 / segments
def weighted_gather3(src, idx, wgt):
    """out[r] = sum_j wgt[r, j] src[idx[r, j]]"""
    return (src.double()[idx.long()] * wgt.double()[:, :, None]).sum(1)


def weighted_scatter3(dy, idx, wgt, nsrc):
    """its adjoint: dsrc[t] = sum over the entries (r, j) with idx[r, j] == t of wgt[r, j] dy[r]"""
    out = torch.zeros(nsrc, dy.shape[1], dtype=f64)
    out.index_add_(0, idx.long().reshape(-1), (dy.double()[:, None, :] * wgt.double()[:, :, None]).reshape(-1, dy.shape[1]))
    return out


GATHER3_CASES = {"unreferenced": (2, 50, 400), "long": (2, 5000, 3), "two": (3, 257, 2)}     # name: (B, Nq, Nc)
GATHER3_WIDTHS = (64, 24, 4)


def gather3_case(name, C, seed=110):
    """-> (q [B, Nq, 3], c [B, Nc, 3], src [B * Nc, C], dy [B * Nq, C]); src and dy are column slices of wider buffers.  unreferenced:
    eight candidates per query, most source rows referenced by nobody; long: three candidates, so three segments of 5000 entries per
    batch element; two: two candidates, the third neighbour missing."""
    B, Nq, Nc = GATHER3_CASES[name]
    q, c = three_nn_case("random", B, Nq, Nc, seed)
    return q, c, rnd(B * Nc, C + 12, seed=seed + 2)[:, 4:4 + C], rnd(B * Nq, C + 8, seed=seed + 3)[:, 8:8 + C]


def segments_of(key, nseg, lo=0):
    """explicit member lists (ascending row) of the segments lo .. lo + nseg - 1 of a key vector; other keys belong to no segment"""
    key = key.long()
    return [torch.nonzero(key == lo + s).view(-1) for s in range(nseg)]


def segment_reduce(src, segs, mode, init=None, mean_extra=0):
    """sum | max | mean over explicit member lists -> float64 [nseg, C]; an empty segment gives 0.  (init / mean_extra exist for the
    wrong variants of the CPU tests: a max that starts from `init`, a mean divided by max(count, 1) + mean_extra.)"""
    out = torch.zeros(len(segs), src.shape[1], dtype=f64)
    for s, m in enumerate(segs):
        if m.numel() == 0:
            continue
        x = src.double()[m]
        if mode == "max":
            out[s] = x.max(0)[0] if init is None else torch.clamp_min(x.max(0)[0], init)
        elif mode == "sum":
            out[s] = x.sum(0)
        else:
            out[s] = x.sum(0) / (max(m.numel(), 1) + mean_extra)
    return out


def segment_reduce_fp32(src, segs, mode):
    """fp32, members added one after the other in list order (the kernel's order)"""
    out = torch.zeros(len(segs), src.shape[1], dtype=f32)
    for s, m in enumerate(segs):
        if m.numel() == 0:
            continue
        x = src.float()[m]
        if mode == "max":
            out[s] = x.max(0)[0]
        else:
            acc = _seq_sum(x)
            out[s] = acc if mode == "sum" else acc / torch.tensor(float(m.numel()), dtype=f32)
    return out


def _seq_sum(x):
    acc = torch.zeros(x.shape[1], dtype=f32)
    for row in x:
        acc = acc + row
    return acc


def segment_softmax(attn, vp, segs, scale, dtype=f64):
    """out[s, c] = sum_i softmax_i(attn[i, c] scale) vp[i, c] over the members of segment s; an empty segment gives 0"""
    zero = torch.zeros(attn.shape[1], dtype=dtype)
    return torch.stack([(torch.softmax(attn.to(dtype)[m] * scale, 0) * vp.to(dtype)[m]).sum(0) if m.numel() else zero for m in segs])


def segment_softmax_bwd(attn, vp, dout, segs, scale, dtype=f64):
    """-> (d attn, d vp) written out: d vp_i = p_i dout, d attn_i = scale p_i dout (vp_i - out); rows of no segment get zero"""
    da, dv = torch.zeros(attn.shape, dtype=dtype), torch.zeros(vp.shape, dtype=dtype)
    for s, m in enumerate(segs):
        if m.numel() == 0:
            continue
        p = torch.softmax(attn.to(dtype)[m] * scale, 0)
        w, g = vp.to(dtype)[m], dout.to(dtype)[s]
        dv[m] = p * g
        da[m] = scale * p * g * (w - (p * w).sum(0))
    return da, dv


SEG_LENGTHS = [0, 1, 7, 8, 9, 1000]      # empty, single, the 8-wide unroll boundary, long
SEG_NSEG = 203                            # not a multiple of the 4 segments of a workgroup


def segment_case(seed=120):
    """-> key int32 [R]: 203 segments, the lengths above first and then 0 .. 12 in turn, rows in a random order"""
    lens = SEG_LENGTHS + [(7 * s) % 13 for s in range(SEG_NSEG - len(SEG_LENGTHS))]
    key = torch.repeat_interleave(torch.arange(SEG_NSEG), torch.tensor(lens))
    return key[torch.randperm(key.numel(), generator=torch.Generator().manual_seed(seed))].int()


def check_segment_reduce(got, src, segs, mode):
    """max: exact, and (the data being negative) 0 exactly on the empty segments and nowhere else; sum / mean: 2e-5 of the output scale"""
    ref = segment_reduce(src, segs, mode)
    if mode == "max":
        assert torch.equal(got.detach().cpu().double(), ref), "max: %d entries differ" % int((got.detach().cpu().double() != ref).sum())
        return 0.0
    return close(got, ref, 2e-5, mode)


def dot64(a, b):
    return float((a.detach().cpu().double() * b.detach().cpu().double()).sum())


def gather3_scatter3_fp32(src, dy, idx, wgt):
    """fp32 in the kernels' order -> (gather3(src) = (a0 + a1) + a2 per row, scatter3(dy) with the entries of a source row added one after
    the other in ascending entry); every step is elementwise fp32 torch, so the result does not depend on a library's summation order"""
    w, C = wgt.float(), src.shape[1]
    a = [src.float()[idx[:, j]] * w[:, j:j + 1] for j in range(3)]
    g = (a[0] + a[1]) + a[2]
    terms = (dy.float()[:, None, :] * w[:, :, None]).reshape(-1, C)
    target, entry = torch.sort(idx.reshape(-1), stable=True)
    first = torch.searchsorted(target, torch.arange(src.shape[0]))
    count = torch.bincount(target, minlength=src.shape[0])
    sc = torch.zeros(src.shape[0], C, dtype=f32)
    for p in range(int(count.max())):
        live = (count > p).nonzero().view(-1)
        sc[live] = sc[live] + terms[entry[first[live] + p]]
    return g, sc


# <gather3(x), dy> = <x, scatter3(dy)> to 1e-5 of the inner product -- except where fp32 cannot reach that: with three segments of 5000
# entries per batch element ("long") and few channels the products of either sign cancel (C = 4: the inner product is 2.82, its products add
# up to 7.8e3 in magnitude), and fp32 torch on the CPU in the kernel's order (gather3_scatter3_fp32) is off by the figures below (rounded
# up; the kernel measured 1.19e-5 and 3.11e-5).  Those two cases get 4 x their own figure; fp32 sits below 1e-5 / 4 on the other seven.
GATHER3_ADJOINT_FP32 = {("long", 24): 1.3e-5, ("long", 4): 3.5e-5}


def gather3_adjoint_rtol(name, C):
    return 4 * GATHER3_ADJOINT_FP32[(name, C)] if (name, C) in GATHER3_ADJOINT_FP32 else 1e-5


def check_adjoint(lhs, rhs, name="", rtol=1e-5):
    """<A x, dy> against <x, A^T dy>, both accumulated in float64: relative to the larger of the two"""
    e = abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-30)
    assert e <= rtol, "%s: %.9e vs %.9e (%.2e)" % (name, lhs, rhs, e)
    return e


def dropped_keys(B, N, M, seed):
    """keys as test_csr_build_counting_sort makes them: about 1 % of the rows point outside their batch element's segments.
    -> (key int32 [B * N], ok bool [B * N])"""
    g = torch.Generator().manual_seed(seed + N + M)
    idx = torch.randint(0, M, (B, N), generator=g)
    key = (idx + torch.arange(B).view(B, 1) * M).reshape(-1).int()
    bad = torch.rand(B * N, generator=g) < 0.01
    key[bad] = torch.where(torch.rand(int(bad.sum()), generator=g) < 0.5, torch.tensor(-3), torch.tensor(B * M + 5)).int()
    rows = torch.arange(B * N)
    ok = (key >= (rows // N) * M) & (key < (rows // N + 1) * M)
    return key, ok


# ------------------------------------------------------------------------------------------------------- the front through the tape
TAPE_GRAD_RTOL = 1e-4      # of each gradient's own largest entry: the bar test_train_geo_gpu.py sets for its backward kernels
PARAM_OF = {"fc1.weight": ("fc1", 0), "fc1.bias": ("fc1", 1), "w_ks.weight": ("wk", None), "w_vs.weight": ("wv", None),
            "fc_delta.0.weight": ("d0", 0), "fc_delta.0.bias": ("d0", 1), "fc_delta.2.weight": ("d2", 0), "fc_delta.2.bias": ("d2", 1),
            "fc_gamma.0.weight": ("g0", 0), "fc_gamma.0.bias": ("g0", 1), "fc_gamma.2.weight": ("g2", 0), "fc_gamma.2.bias": ("g2", 1)}


def tape_case(mode, seed=150):
    """96 rows.  group: 7 nodes (the last owns no point), k / v computed from the features; knn: 6 nodes x 16 neighbours, k / v per-node
    tables read through the neighbour index.  -> (weights, operands of front(), (Wa, Wvp) of the loss sum(a Wa) + sum(vp Wvp))"""
    w = front_weights(seed)
    rows = 96
    if mode == "group":
        S = 7
        gidx = randint(S - 1, rows, seed + 1).int()
        pa, pb = rnd(rows, 4, seed=seed + 2, lo=-5, hi=5), rnd(S, 4, seed=seed + 3, lo=-5, hi=5)
        o = dict(feat=rnd(rows, 64, seed=seed + 4), q=rnd(S, 64, seed=seed + 5), pa=pa, pb=pb, ib=gidx, iq=gidx)
    else:
        S = 6
        knn = randint(S, rows, seed + 1).int()
        node = rnd(S, 4, seed=seed + 3, lo=-5, hi=5)
        o = dict(q=rnd(S, 64, seed=seed + 5), k=rnd(S, 64, seed=seed + 6), v=rnd(S, 64, seed=seed + 7), pa=node, pb=node, ib=knn, ikv=knn,
                 divq=16, diva=16)
    o["pa"][:, 3] = 0
    o["pb"][:, 3] = 0
    return w, o, (rnd(rows, 64, seed=seed + 8), rnd(rows, 64, seed=seed + 9))


def front_grads(w, o, loss_w, dtype=f64):
    """float64 (or `dtype`) autograd of sum(a Wa) + sum(vp Wvp) through front() -> {parameter name | "feat" | "q" | "k" | "v": gradient}; a
    parameter the case does not use has gradient zero"""
    leaf = lambda t: t.to(dtype).clone().requires_grad_(True)
    wl = {k: (tuple(leaf(t) for t in v) if isinstance(v, tuple) else leaf(v)) for k, v in w.items()}
    ol = {k: (leaf(v) if k in ("feat", "q", "k", "v") else v) for k, v in o.items()}
    out = front(wl, dtype=dtype, **ol)
    ((out["a"] * loss_w[0].to(dtype)).sum() + (out["vp"] * loss_w[1].to(dtype)).sum()).backward()
    grads = {}
    for name, (key, i) in PARAM_OF.items():
        t = wl[key] if i is None else wl[key][i]
        grads[name] = t.grad if t.grad is not None else torch.zeros_like(t)
    for k in ("feat", "q", "k", "v"):
        if k in ol:
            grads[k] = ol[k].grad
    return grads


def check_grads(got, ref):
    """every gradient to 1e-4 of its own largest entry; one whose true value is zero absolutely, at 1e-4 of the case's largest gradient"""
    top = max(float(g.abs().max()) for g in ref.values())
    figs = {}
    for name, r in ref.items():
        g = got[name].detach().cpu().double()
        assert g.shape == r.shape, (name, tuple(g.shape), tuple(r.shape))
        scale = float(r.abs().max())
        err = float((g - r).abs().max())
        assert err == err and err <= TAPE_GRAD_RTOL * (scale if scale > 0 else top), "%s: max|d| %.3e vs scale %.3e" % (name, err, scale)
        figs[name] = err / (scale if scale > 0 else top)
    return figs


# ---------------------------------------------------------------------------------------------------------------- segment softmax
SOFTMAX_SCALE = 0.125
SOFTMAX_FWD_RTOL, SOFTMAX_BWD_RTOL = 2e-5, 5e-5      # test_vector_attention_pieces / test_segment_softmax_backward


def softmax_case(kind, seed=130):
    """-> (attn, vp, dout, key int32, (B, N, M) of csr_build, ok bool [rows]).  peaked: attn in +-300, so that one member of a segment
    takes nearly all the weight; long: one segment of 5000 members beside a short and an empty one; dropped: about 1 % of the keys point
    outside their batch element's segments."""
    if kind == "peaked":
        B, N, M = 1, 3000, 200
        key, amp = randint(M, N, seed).int(), 300
        ok = torch.ones(N, dtype=torch.bool)
    elif kind == "long":
        B, N, M = 1, 5010, 3
        key = torch.cat([torch.ones(5000), torch.zeros(10)]).int()[torch.randperm(N, generator=torch.Generator().manual_seed(seed))]
        amp, ok = 30, torch.ones(N, dtype=torch.bool)
    else:
        B, N, M = 2, 3000, 50
        (key, ok), amp = dropped_keys(B, N, M, seed), 30
    R = B * N
    return rnd(R, 64, seed=seed + 1, lo=-amp, hi=amp), rnd(R, 64, seed=seed + 2), rnd(B * M, 64, seed=seed + 3), key, (B, N, M), ok


def check_softmax(out, da, dv, attn, vp, dout, segs, ok=None):
    """forward and both gradients against float64; the gradients of the rows of no segment exactly zero"""
    figs = dict(out=close(out, segment_softmax(attn, vp, segs, SOFTMAX_SCALE), SOFTMAX_FWD_RTOL, "segment softmax"))
    rda, rdv = segment_softmax_bwd(attn, vp, dout, segs, SOFTMAX_SCALE)
    figs["da"], figs["dv"] = close(da, rda, SOFTMAX_BWD_RTOL, "d attn"), close(dv, rdv, SOFTMAX_BWD_RTOL, "d vp")
    if ok is not None and not bool(ok.all()):
        for g in (da, dv):
            assert bool((g.detach().cpu()[~ok] == 0).all()), "a row of no segment with a gradient that is not exactly zero"
    return figs
