"""GPU tier of the dual-softmax match confidence (ops.match_conf / cmr_match_conf_f32, MultiHeadModel.pose_from_matches(min_conf=),
Test_Geo.py --min-conf).

idx must be the matcher's idx and d1 the match filter's d1, bit for bit.  Everything else is held to the float64 restatement of
match_conf_reference.py within the error bound derived there: |log conf - float64| <= 4 E + (h*w + |S_b|) 2^-24 + 1e-5 on the rows whose
float64 conf is >= 1e-30, row_lse / col_lse within E + n 2^-24 + 5e-6, keep exact off the near rows (forward gap < 1e-5 or
|log conf - log min_conf| within the bound), which are at most 1 % of a sample's selected rows (tests/test_match_conf_cpu.py asserts
that cap on the same scenes without a GPU)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_conf_reference as ref
import pnp_reference
from cmr_agent_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_NAMES = ("idx", "conf", "keep", "counts", "d1", "row_lse", "col_lse")


def _unit(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(*shape, generator=g, dtype=torch.float64), dim=-1).float().to(DEV)


def _mask(kind, B, N, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind == "all":
        m = torch.ones(B, N, dtype=torch.int64)
    elif kind == "random":
        m = (torch.rand(B, N, generator=g) < 0.3).long()
    elif kind == "one":
        m = torch.zeros(B, N, dtype=torch.int64)
        m[:, (N * 7) // 11] = 1
    else:
        m = torch.zeros(B, N, dtype=torch.int64)
    return m.to(DEV)


def _same(a, b):
    """Bit-for-bit equality of two output tuples (NaN fill values included)."""
    for x, y, name in zip(a, b, OUT_NAMES):
        assert (x is None) == (y is None), name
        if x is not None:
            bits = {1: torch.uint8, 4: torch.int32}[x.element_size()]
            assert torch.equal(x.view(bits), y.view(bits)), name


def _scene(maker, kw):
    return {k: v.to(DEV) for k, v in maker(**kw).items()}


def _check_against_float64(name, s, ckw):
    """One call with every output against the restatement; -> the largest observed share of the bound on log conf."""
    B, h, w, _ = s["img"].shape
    N = s["pc"].shape[0] // B
    hw = h * w
    idx, conf, keep, counts, d1, row_lse, col_lse = ops.match_conf(s["pc"], s["img"], s["mask"], gt_xy=s["gt_xy"], thr=3.0, want_dist=True,
                                                                   want_lse=True, **ckw)
    want = ref.restate(s["pc"], s["img"], s["mask"], gt_xy=s["gt_xy"], thr=3.0, **ckw)
    idx, conf, keep, d1, row_lse, col_lse = (idx.view(B, N), conf.view(B, N), keep.view(B, N), d1.view(B, N), row_lse.view(B, N),
                                             col_lse.view(B, hw))
    worst = 0.0
    for b, r in enumerate(want):
        sel, ns = r["sel"], r["sel"].numel()
        b_conf, b_row, b_col = ref.bound(r["E"], hw, ns)
        near = int(r["near"].sum())
        print(name, b, "selected", ns, "near", near, "counts", counts[b].tolist(), "float64", r["counts"], "bound %.3g" % b_conf)
        assert near <= ref.CAP * ns, (near, ns)
        unsel = torch.ones(N, dtype=torch.bool, device=DEV)
        unsel[sel] = False
        assert bool((idx[b][unsel] == -1).all()) and not bool(keep[b][unsel].any())
        for t in (conf, d1, row_lse):
            assert bool(torch.isnan(t[b][unsel]).all()) and not bool(torch.isnan(t[b][sel]).any())
        assert bool(((conf[b][sel] >= 0) & (conf[b][sel] <= 1)).all())
        # the sums do not hang on any decision: every selected row, every pixel
        e_row = float((row_lse[b][sel].double() - r["row_lse"][sel]).abs().max())
        e_col = float((col_lse[b].double() - r["col_lse"]).abs().max())
        print(name, b, "max |row_lse - float64| %.3g of %.3g  max |col_lse - float64| %.3g of %.3g" % (e_row, b_row, e_col, b_col))
        assert e_row <= b_row and e_col <= b_col
        rows = sel[r["fwd_gap"] >= ref.GAP_TOL]                       # idx is decided: the same pixel, so the same confidence
        assert torch.equal(idx[b][rows].long(), r["idx"][rows])
        e_d2 = float((d1[b][rows].double() ** 2 - r["d1"][rows] ** 2).abs().max())     # s = -d^2 / T carries at most E, so d^2 at most E T
        assert e_d2 <= r["E"] * ckw["temperature"] + 1e-6, (e_d2, r["E"] * ckw["temperature"])
        big = rows[r["conf"][rows] >= ref.CONF_FLOOR]
        assert big.numel() > 0.5 * ns
        e_conf = float((conf[b][big].double().log() - r["conf"][big].log()).abs().max())
        print(name, b, "max |log conf - float64| %.3g of %.3g on %d rows" % (e_conf, b_conf, big.numel()))
        assert e_conf <= b_conf
        worst = max(worst, e_conf / b_conf)
        ok = sel[~r["near"]]
        assert torch.equal(keep[b][ok], r["keep"][ok])
        c = counts[b].tolist()
        assert c[0] == r["counts"][0] and c[1] == int(keep[b].sum())
        for k in (1, 2, 3):
            assert abs(c[k] - r["counts"][k]) <= near, (b, k, c, r["counts"], near)
    return worst


CASES = [  # B, N, h, w, mask: the case list of tests/test_feat_match_gpu.py
    (1, 1000, 11, 38, "all"),
    (3, 4097, 40, 128, "random"),
    (8, 1000, 40, 128, "random"),
    (3, 4097, 88, 304, "random"),
    (1, 4097, 88, 304, "one"),
    (3, 1000, 11, 38, "one"),
    (3, 1000, 11, 38, "empty"),
    (8, 4097, 11, 38, "all"),
]


@pytest.mark.parametrize("B,N,h,w,kind", CASES)
def test_idx_is_the_matchers_idx_and_d1_the_filters(B, N, h, w, kind):
    pc, img = _unit(B * N, 64, seed=N + B), _unit(B, h, w, 64, seed=h * w + B)
    mask = _mask(kind, B, N, seed=B * N)
    g = torch.Generator(device="cpu").manual_seed(5)
    xy = (torch.rand(B, 2, N, generator=g) * torch.tensor([w, h]).view(1, 2, 1)).to(DEV)
    want_idx, _, want_counts = ops.feat_match(pc, img, mask, gt_xy=xy, thr=3.0)
    want_d1 = ops.feat_match_filter(pc, img, mask, mutual=False, want_dist=True)[3]
    idx, conf, keep, counts, d1, row_lse, col_lse = ops.match_conf(pc, img, mask, temperature=0.1, min_conf=0.02, gt_xy=xy, thr=3.0,
                                                                   want_dist=True, want_lse=True)
    assert torch.equal(idx, want_idx)
    assert torch.equal(d1.view(torch.int32), want_d1.view(torch.int32))            # the same arithmetic: the same bits, NaN fill included
    assert torch.equal(counts[:, 0], want_counts[:, 0]) and torch.equal(counts[:, 3], want_counts[:, 1])
    sel = mask.view(-1) != 0
    assert keep.dtype == torch.bool and not bool(keep[~sel].any())
    assert int(keep.sum()) == int(counts[:, 1].sum())
    assert torch.equal(keep, sel & (conf >= 0.02))
    assert bool(torch.isnan(conf[~sel]).all()) and bool(((conf[sel] > 0) & (conf[sel] <= 1)).all())
    assert bool(torch.isnan(row_lse[~sel]).all()) and bool(torch.isfinite(row_lse[sel]).all())
    if kind == "empty":
        assert bool((col_lse == -math.inf).all()) and counts.tolist() == [[0, 0, 0, 0]] * B
    else:
        assert bool(torch.isfinite(col_lse).all())
    assert torch.equal(ops.match_conf(pc, img, mask)[0], want_idx)                  # the optional outputs do not move idx


@pytest.mark.parametrize("name,maker,skw,ckw", ref.SCENES, ids=[s[0] for s in ref.SCENES])
def test_against_float64(name, maker, skw, ckw):
    worst = _check_against_float64(name, _scene(maker, skw), ckw)
    print(name, "largest observed share of the bound on log conf: %.3f" % worst)


def test_no_threshold_keeps_exactly_the_mask():
    B, N, h, w = 3, 4097, 40, 128
    s = _scene(ref.planted_scene, dict(B=B, N=N, h=h, w=w, seed=211))
    sel = s["mask"].view(-1) != 0
    idx, conf, keep, counts, d1, row_lse, col_lse = ops.match_conf(s["pc"], s["img"], s["mask"], min_conf=0.0, gt_xy=s["gt_xy"])
    assert d1 is None and row_lse is None and col_lse is None
    assert torch.equal(keep, sel)
    assert torch.equal(counts[:, 1], counts[:, 0]) and torch.equal(counts[:, 2], counts[:, 3])
    want = ops.feat_match(s["pc"], s["img"], s["mask"], gt_xy=s["gt_xy"])
    assert torch.equal(idx, want[0]) and torch.equal(counts[:, [0, 3]], want[2][:, [0, 1]])
    # min_conf = 1: conf is capped at 1, so only a row that owns its pixel entirely and vice versa could pass
    _, conf1, keep1, counts1, _, _, _ = ops.match_conf(s["pc"], s["img"], s["mask"], min_conf=1.0, gt_xy=s["gt_xy"])
    assert torch.equal(conf1.view(torch.int32), conf.view(torch.int32)) and torch.equal(keep1, sel & (conf >= 1.0))
    assert int(counts1[:, 1].sum()) == int(keep1.sum())


def test_empty_mask_and_mask_dtypes():
    B, N, h, w = 3, 1000, 11, 38
    pc, img = _unit(B * N, 64, seed=91), _unit(B, h, w, 64, seed=92)
    xy = torch.zeros(B, 2, N, device=DEV)
    idx, conf, keep, counts, d1, row_lse, col_lse = ops.match_conf(pc, img, torch.zeros(B, N, dtype=torch.int64, device=DEV), min_conf=0.1,
                                                                   gt_xy=xy, want_dist=True, want_lse=True)
    assert bool((idx == -1).all()) and not bool(keep.any()) and bool((col_lse == -math.inf).all())
    assert counts.tolist() == [[0, 0, 0, 0]] * B
    assert bool(torch.isnan(conf).all()) and bool(torch.isnan(d1).all()) and bool(torch.isnan(row_lse).all())
    # one sample empty, the others not
    mask = _mask("random", B, N, seed=93)
    mask[1] = 0
    kw = dict(temperature=0.1, min_conf=0.02, gt_xy=xy, thr=50.0, want_dist=True, want_lse=True)
    a = ops.match_conf(pc, img, mask, **kw)
    assert bool((a[6].view(B, -1)[1] == -math.inf).all()) and a[3][1].tolist() == [0, 0, 0, 0] and int(a[3][0, 1]) > 0
    assert bool(torch.isfinite(a[6].view(B, -1)[[0, 2]]).all())
    _same(a, ops.match_conf(pc, img, mask.bool(), **kw))
    _same(a, ops.match_conf(pc, img, mask.to(torch.uint8), **kw))
    _same(a, ops.match_conf(pc, img, (mask * 7).view(B * N), **kw))                 # any non-zero selects; [B*N] is accepted


def test_a_single_selected_row_owns_its_column():
    """One row selected: the column sum of its pixel is its own term, so conf = exp(s - row_lse)."""
    B, N, h, w = 2, 1000, 11, 38
    pc, img = _unit(B * N, 64, seed=95), _unit(B, h, w, 64, seed=96)
    mask = _mask("one", B, N, seed=0)
    n = (N * 7) // 11
    T = 0.1
    idx, conf, keep, counts, d1, row_lse, col_lse = ops.match_conf(pc, img, mask, temperature=T, min_conf=0.5, want_dist=True, want_lse=True)
    E = ref.eps_s(pc, img, T)
    b_conf, b_row, b_col = ref.bound(E, h * w, 1)
    for b in range(B):
        d2 = ((pc[b * N + n].double()[None, :] - img[b].reshape(h * w, 64).double()) ** 2).sum(1)
        s = -d2 / T
        p = int(d2.argmin())
        assert int(idx[b * N + n]) == p
        lse = float(torch.logsumexp(s, 0))
        assert abs(float(row_lse[b * N + n]) - lse) <= b_row
        assert float((col_lse.view(B, -1)[b].double() - s).abs().max()) <= b_col        # every column: the one row's own term
        assert abs(math.log(float(conf[b * N + n])) - (float(s[p]) - lse)) <= b_conf
        assert bool(keep[b * N + n]) == (float(conf[b * N + n]) >= 0.5)
    assert counts[:, 0].tolist() == [1] * B and int(keep.sum()) == int(counts[:, 1].sum())


def test_duplicate_points_share_the_column():
    """Two identical rows selected: each gets at most half of its pixel's column probability, and the same bits as its twin -- in one
    256-row tile, across tiles, across lane halves."""
    B, N, h, w = 2, 1000, 40, 128
    T = 0.1
    img = _unit(B, h, w, 64, seed=9)
    flat = img.view(B, h * w, 64)
    g = torch.Generator(device="cpu").manual_seed(4)
    pix = torch.randperm(h * w, generator=g)[:N].to(DEV)
    pc = torch.nn.functional.normalize(flat[:, pix] + 0.05 * torch.randn(B, N, 64, generator=g).to(DEV), dim=-1)
    dups = [(5, 700), (300, 301), (40, 72), (999, 998)]
    for a, c in dups:
        pc[:, c] = pc[:, a]
    pc = pc.reshape(B * N, 64).contiguous()
    mask = torch.ones(B, N, dtype=torch.int64, device=DEV)
    idx, conf, _, _, d1, row_lse, _ = ops.match_conf(pc, img, mask, temperature=T, want_dist=True, want_lse=True)
    idx, conf, d1, row_lse = idx.view(B, N), conf.view(B, N), d1.view(B, N), row_lse.view(B, N)
    b_conf = ref.bound(ref.eps_s(pc, img, T), h * w, N)[0]
    for a, c in dups:
        assert bool((idx[:, a] == pix[a]).all()) and bool((idx[:, c] == pix[a]).all())
        assert torch.equal(conf[:, a].view(torch.int32), conf[:, c].view(torch.int32))
        assert torch.equal(row_lse[:, a].view(torch.int32), row_lse[:, c].view(torch.int32))
        s = -(d1[:, a].double() ** 2) / T
        half = 0.5 * (s - row_lse[:, a].double()).exp()
        assert bool((conf[:, a].double() <= half * math.exp(b_conf)).all()), (conf[:, a], half)
    single = [n for n in range(N) if all(n not in d for d in dups)][:50]
    assert float(conf[:, single].median()) > 1.5 * float(conf[:, [a for a, _ in dups]].max())     # the planted rows own their pixel


def test_large_scores_do_not_overflow():
    """Features scaled by 3: |s| = 9 d^2 / T reaches past 200, so exp(s) itself underflows in fp32 everywhere off the matches; with the
    running maximum in place nothing overflows, nothing is NaN and conf stays within the bound."""
    skw = dict(B=2, N=4097, h=40, w=128, seed=221)
    s = _scene(ref.planted_scene, skw)
    s["pc"], s["img"] = (3.0 * s["pc"]).contiguous(), (3.0 * s["img"]).contiguous()
    T = 0.1
    rows = torch.nonzero(s["mask"][0]).flatten()
    d2 = torch.cdist(s["pc"][:4097][rows].double(), s["img"][0].reshape(-1, 64).double()) ** 2
    assert float(d2.max()) / T > 200.0 and float(d2.min(1).values.max()) / T > 87.0       # exp(-88) is fp32's smallest normal
    idx, conf, keep, counts, d1, row_lse, col_lse = ops.match_conf(s["pc"], s["img"], s["mask"], temperature=T, min_conf=0.05, want_lse=True)
    sel = s["mask"].view(-1) != 0
    assert bool(torch.isfinite(conf[sel]).all()) and bool(torch.isfinite(row_lse[sel]).all()) and bool(torch.isfinite(col_lse).all())
    assert float(row_lse[sel].min()) < -88.0 and float(col_lse.min()) < -88.0      # sums a plain exp would flush to 0
    _check_against_float64("scaled_by_3", s, dict(temperature=T, min_conf=0.05))


def test_two_calls_agree_and_a_sample_alone_equals_the_sample_in_a_batch():
    B, N, h, w = 3, 4097, 40, 128
    s = _scene(ref.planted_scene, dict(B=B, N=N, h=h, w=w, seed=231))
    s["mask"][1, N // 3:] = 0                                          # samples with different selected counts: different cuts
    s["mask"][2, 5:] = 0
    kw = dict(temperature=0.1, min_conf=0.05, thr=3.0, want_dist=True, want_lse=True)
    a = ops.match_conf(s["pc"], s["img"], s["mask"], gt_xy=s["gt_xy"], **kw)
    _same(a, ops.match_conf(s["pc"], s["img"], s["mask"], gt_xy=s["gt_xy"], **kw))
    for b in range(B):
        one = ops.match_conf(s["pc"][b * N:(b + 1) * N].contiguous(), s["img"][b:b + 1].contiguous(), s["mask"][b:b + 1].contiguous(),
                             gt_xy=s["gt_xy"][b:b + 1].contiguous(), **kw)
        _same([t.view(B, -1)[b].contiguous() for t in a], [t.view(-1) for t in one])
    # ... and inside another batch, at another position
    o = _scene(ref.planted_scene, dict(B=2, N=N, h=h, w=w, seed=232))
    pc2 = torch.cat([o["pc"], s["pc"][:N]]).contiguous()
    c = ops.match_conf(pc2, torch.cat([o["img"], s["img"][:1]]).contiguous(), torch.cat([o["mask"], s["mask"][:1]]).contiguous(),
                       gt_xy=torch.cat([o["gt_xy"], s["gt_xy"][:1]]).contiguous(), **kw)
    _same([t.view(B, -1)[0].contiguous() for t in a], [t.view(B, -1)[2].contiguous() for t in c])


def test_graph_replay_equals_eager():
    B, N, h, w = 3, 4097, 40, 128
    s = _scene(ref.planted_scene, dict(B=B, N=N, h=h, w=w, seed=241))
    kw = dict(temperature=0.1, min_conf=0.05, gt_xy=s["gt_xy"], want_dist=True, want_lse=True)
    eager = ops.match_conf(s["pc"], s["img"], s["mask"], **kw)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ops.match_conf(s["pc"], s["img"], s["mask"], **kw)
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ops.match_conf(s["pc"], s["img"], s["mask"], **kw)
    for t in got:
        t.view(torch.uint8).fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    _same(eager, got)


def _errors(pose, P):
    pose = pose.double().cpu().numpy()
    rre = [pnp_reference.rotation_error_deg(pose[b][:3, :3], P[b][:3, :3]) for b in range(len(P))]
    rte = [float(np.linalg.norm(pose[b][:3, 3] - P[b][:3, 3])) for b in range(len(P))]
    return rre, rte


def test_pose_from_confident_matches_end_to_end():
    """The planted geometry of tests/test_match_filter_gpu.py::test_pose_from_filtered_matches_end_to_end: pnp_reference.planted gives
    points, pose and K; point n's feature is the feature of its true rounded pixel plus noise, and half of the points carry a random
    unit feature instead.  With conf >= 0.1, 16 hypotheses recover the pose within that test's bars (rotation <= q / f rad,
    translation <= q * z_max / f, q = 0.5 * sqrt(2) px)."""
    from cmr_agent_amd.config import KittiConfiguration
    from cmr_agent_amd.models import MultiHeadModel
    from cmr_agent_amd.models.MultiHeadModel import match_features
    B, N, h, w = 2, 4096, 40, 128
    s = pnp_reference.planted(B, N, h, w, seed=131)
    K = s["K"][0]
    cam = np.einsum("bij,bjn->bin", s["P"][:, :3, :3], s["pts"]) + s["P"][:, :3, 3:4]
    pix = (np.round(s["uv"][:, 1]) * w + np.round(s["uv"][:, 0])).astype(np.int64)
    g = torch.Generator(device="cpu").manual_seed(132)
    img = torch.nn.functional.normalize(torch.randn(B, h * w, 64, generator=g, dtype=torch.float64), dim=-1)
    pcf = torch.gather(img, 1, torch.from_numpy(pix)[..., None].expand(B, N, 64)) + 0.08 * torch.randn(B, N, 64, generator=g, dtype=torch.float64)
    outlier = torch.rand(B, N, generator=g) < 0.5
    pcf = torch.where(outlier[..., None], torch.randn(B, N, 64, generator=g, dtype=torch.float64), pcf)
    pcf = torch.nn.functional.normalize(pcf, dim=-1).float()
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    data = {"pc": f(s["pts"]), "K": f(s["K"]), "P": f(s["P"]), "pc_in_cam_space": f(cam),
            "pc_geo_feat": pcf.permute(0, 2, 1).contiguous().to(DEV),
            "img_geo_feat": img.float().view(B, h, w, 64).permute(0, 3, 1, 2).contiguous().to(DEV),
            "pc_overlap_pred": torch.ones(B, N, dtype=torch.bool, device=DEV)}
    ov = torch.ones(B, h, w, dtype=torch.bool, device=DEV)
    ov[:, :, : w // 8] = False                                          # a real image-overlap mask: the left eighth is out
    model = MultiHeadModel(KittiConfiguration(num_pt=N, device=torch.device(DEV)))

    # min_conf=None: every key and value of today's call, which is bit for bit a direct match_features + ops.pnp_ransac call
    plain = dict(data)
    model.pose_from_matches(plain, img_overlap=ov, n_hyp=16)
    none = dict(data)
    model.pose_from_matches(none, img_overlap=ov, n_hyp=16, min_conf=None, temperature=0.37)
    assert set(none) == set(plain) == set(data) | {"pnp_pose", "pnp_inliers", "pnp_status"}
    idx, _, _, w_ = match_features(data, data["pc_overlap_pred"])
    p = idx.long().clamp(min=0)
    use = (idx >= 0) & torch.gather(ov.reshape(B, -1), 1, p)
    uv = torch.stack([p % w_, torch.div(p, w_, rounding_mode="floor")], 1).float().contiguous()
    pose, inl, status = ops.pnp_ransac(data["pc"], uv, use.contiguous(), data["K"], n_hyp=16, thr=1.0, seed=0, refine_iters=10)
    for d in (plain, none):
        assert torch.equal(d["pnp_pose"].view(torch.int32), pose.view(torch.int32))
        assert torch.equal(d["pnp_inliers"], inl) and torch.equal(d["pnp_status"], status)
    plain_share = inl.double() / use.sum(1).double()

    rows = data["pc_geo_feat"].permute(0, 2, 1).reshape(B * N, 64).contiguous()
    nhwc = data["img_geo_feat"].permute(0, 2, 3, 1).contiguous()
    cidx, cconf, ckeep, ccounts, _, _, _ = ops.match_conf(rows, nhwc, data["pc_overlap_pred"], temperature=0.1, min_conf=0.1)
    inside = torch.gather(ov.reshape(B, -1), 1, cidx.view(B, N).long().clamp(min=0))
    want_used = (ckeep.view(B, N) & inside).sum(1)
    q, foc = 0.5 * math.sqrt(2.0), K[0, 0]
    for sub in (False, True):
        d = dict(data)
        model.pose_from_matches(d, img_overlap=ov, n_hyp=16, min_conf=0.1, subpixel=sub)
        assert d["pnp_status"].tolist() == [0] * B
        rre, rte = _errors(d["pnp_pose"], s["P"])
        print("conf >= 0.1, subpixel", sub, ": RRE", rre, "RTE", rte, "used", d["pnp_used"].tolist(), "inliers", d["pnp_inliers"].tolist(),
              "| unfiltered inlier share", plain_share.tolist())
        assert max(rre) <= math.degrees(q / foc), (rre, math.degrees(q / foc))
        assert max(rte) <= q * cam[:, 2].max() / foc, (rte, q * cam[:, 2].max() / foc)
        # pnp_used = the kept rows whose matched pixel lies inside the image overlap, from the op's own idx and keep
        assert d["pnp_used"].shape == (B,) and torch.equal(d["pnp_used"].long(), want_used.long())
        assert torch.equal(d["pnp_conf_counts"][:, :2], ccounts[:, :2]) and d["pnp_conf_counts"].dtype == torch.int32
        assert tuple(d["pnp_conf_counts"].shape) == (B, 4)
        assert d["pnp_conf"].shape == (B, N) and torch.equal(d["pnp_conf"].view(torch.int32), cconf.view(B, N).view(torch.int32))
        assert bool((want_used < ckeep.view(B, N).sum(1)).all())          # the overlap mask did remove kept rows
        assert bool((d["pnp_used"] < use.sum(1)).all())
        assert ("pnp_subpixel_counts" in d) == sub and "pnp_filter_counts" not in d
        if sub:
            assert torch.equal(d["pnp_subpixel_counts"][:, 0].long(), want_used.long())   # the `use` mask went to ops.match_subpixel
        else:
            share = d["pnp_inliers"].double() / d["pnp_used"].double()
            assert bool((share > plain_share).all()), (share, plain_share)


def _script(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "Test_Geo.py"), "--pairs", "2", "--img", "160x512", "--num-pt", "4096", *extra]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    return res.stdout.strip().splitlines()


def test_test_geo_script_with_min_conf():
    """Two batches of one pair: per batch "IR1 IR2", the pair's "RTE RRE", then the 5-number summary and the recall block; with the flag
    one "conf kept" line per batch right after "IR1 IR2", and every line that does not hang on the pose is the same text."""
    base = _script("--pnp")
    lines = _script("--pnp", "--min-conf", "0.05")
    assert len(base) >= 6 and [len(l.split()) for l in base[:5]] == [2, 2, 2, 2, 5], base
    assert base[5].startswith("Registration Recall:")
    extra = [i for i, l in enumerate(lines) if l.startswith("conf kept ")]
    assert extra == [1, 4], lines                                         # once per batch, right after the batch's "IR1 IR2" line
    for i in extra:
        tok = lines[i].split()
        assert tok[3] == "of" and tok[5] == "IR" and tok[7] == "->" and len(tok) == 9, lines[i]
        assert 0 <= int(tok[2]) <= int(tok[4]) <= 4096
        for v in (tok[6], tok[8]):
            assert math.isnan(float(v)) or 0.0 <= float(v) <= 1.0
    rest = [l for i, l in enumerate(lines) if i not in extra]
    assert len(rest) >= 6 and rest[5].startswith("Registration Recall:")
    for i in (0, 2, 4):                                                   # the two "IR1 IR2" lines and the closing summary
        assert rest[i] == base[i], (i, rest[i], base[i])
    for i in (1, 3):
        assert len(rest[i].split()) == 2 and all(math.isfinite(float(v)) for v in rest[i].split())
