"""GPU tier of the match filter (ops.feat_match_filter / cmr_feat_match_filter_f32, MultiHeadModel.pose_from_matches(mutual=, ratio=),
Test_Geo.py --mutual / --ratio).

idx must be the matcher's idx bit for bit.  Everything else is defined against the float64 restatement of match_filter_reference.py:
the kernel rounds d^2 = |p|^2 + |q|^2 - 2 p.q in fp32, so decisions are compared only on the rows whose three float64 margins (forward
best / runner-up gap, reverse gap at the best pixel, |d1 - ratio * d2|) are all >= 1e-5, those rows being at most 0.5 % of a sample's
selected rows (tests/test_match_filter_cpu.py asserts that cap on the same scenes without a GPU)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_filter_reference as ref
import pnp_reference
from cmr_agent_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5
OUT_NAMES = ("idx", "keep", "counts", "d1", "d2", "rev")


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
def test_idx_is_the_matchers_idx(B, N, h, w, kind):
    pc, img = _unit(B * N, 64, seed=N + B), _unit(B, h, w, 64, seed=h * w + B)
    mask = _mask(kind, B, N, seed=B * N)
    g = torch.Generator(device="cpu").manual_seed(5)
    xy = (torch.rand(B, 2, N, generator=g) * torch.tensor([w, h]).view(1, 2, 1)).to(DEV)
    want_idx, want_dist, want_counts = ops.feat_match(pc, img, mask, gt_xy=xy, thr=3.0, want_dist=True)
    idx, keep, counts, d1, d2, rev = ops.feat_match_filter(pc, img, mask, mutual=True, ratio=0.9, excl_radius=2, gt_xy=xy, thr=3.0,
                                                           want_dist=True, want_rev=True)
    assert torch.equal(idx, want_idx)
    assert torch.equal(d1.view(torch.int32), want_dist.view(torch.int32))          # the same arithmetic: the same bits, NaN fill included
    assert torch.equal(counts[:, 0], want_counts[:, 0]) and torch.equal(counts[:, 3], want_counts[:, 1])
    sel = mask.view(-1) != 0
    assert keep.dtype == torch.bool and not bool(keep[~sel].any())
    assert int(keep.sum()) == int(counts[:, 1].sum())
    assert bool(torch.isnan(d2[~sel]).all()) and not bool(torch.isnan(d2[sel]).any())
    if kind == "empty":
        assert bool((rev == -1).all()) and counts.tolist() == [[0, 0, 0, 0]] * B
    else:
        assert bool(((rev >= 0) & (rev < N)).all())
        assert bool(mask.view(B, N).gather(1, rev.view(B, h * w).long()).bool().all())     # a pixel's nearest row is a selected row
    # the sweeps a call does not need are skipped: idx does not move
    for kw in (dict(mutual=False), dict(mutual=True), dict(mutual=False, ratio=0.9)):
        assert torch.equal(ops.feat_match_filter(pc, img, mask, **kw)[0], want_idx)


@pytest.mark.parametrize("name,maker,skw,fkw", ref.SCENES, ids=[s[0] for s in ref.SCENES])
def test_against_float64(name, maker, skw, fkw):
    s = _scene(maker, skw)
    B, h, w, _ = s["img"].shape
    N = s["pc"].shape[0] // B
    idx, keep, counts, d1, d2, rev = ops.feat_match_filter(s["pc"], s["img"], s["mask"], gt_xy=s["gt_xy"], thr=3.0, want_dist=True,
                                                           want_rev=True, **fkw)
    want = ref.restate(s["pc"], s["img"], s["mask"], gt_xy=s["gt_xy"], thr=3.0, **fkw)
    idx, keep, d1, d2, rev = idx.view(B, N), keep.view(B, N), d1.view(B, N), d2.view(B, N), rev.view(B, h * w)
    for b, r in enumerate(want):
        sel, ok = r["sel"], ~r["near"]
        near = int(r["near"].sum())
        print(name, b, "selected", sel.numel(), "under 1e-5:", near, "counts", counts[b].tolist(), "float64", r["counts"])
        assert near <= ref.CAP * sel.numel(), (near, sel.numel())
        unsel = torch.ones(N, dtype=torch.bool, device=DEV)
        unsel[sel] = False
        assert bool((idx[b][unsel] == -1).all()) and not bool(keep[b][unsel].any())
        assert bool(torch.isnan(d1[b][unsel]).all()) and bool(torch.isnan(d2[b][unsel]).all())
        rows = sel[ok]
        got_p = idx[b][rows].long()
        assert torch.equal(got_p, r["idx"][rows])
        assert torch.equal(keep[b][rows], r["keep"][rows])
        assert torch.equal(rev[b][got_p].long() == rows, r["rev"][got_p] == rows)
        e1 = (d1[b][rows].double() - r["d1"][rows]).abs().max()
        e2 = (d2[b][rows].double() - r["d2"][rows]).abs()
        e2 = torch.where(torch.isinf(r["d2"][rows]) & torch.isinf(d2[b][rows]), torch.zeros_like(e2), e2).max()
        print(name, b, "max |d1 - float64| %.3g  max |d2 - float64| %.3g" % (float(e1), float(e2)))
        assert float(e1) <= TOL and float(e2) <= TOL
        c = counts[b].tolist()
        assert c[0] == r["counts"][0]
        for k in (1, 2, 3):
            assert abs(c[k] - r["counts"][k]) <= near, (b, k, c, r["counts"], near)


def test_window_over_the_whole_map_and_no_window():
    B, N, h, w = 2, 1000, 11, 38
    pc, img = _unit(B * N, 64, seed=71), _unit(B, h, w, 64, seed=72)
    mask = _mask("random", B, N, seed=73)
    sel = mask.view(-1) != 0
    for radius in (max(h, w), 10 ** 6):                                # nothing lies outside the window: d2 = +inf, the ratio test passes
        _, keep, counts, _, d2, _ = ops.feat_match_filter(pc, img, mask, mutual=False, ratio=0.5, excl_radius=radius, want_dist=True)
        assert bool(torch.isinf(d2[sel]).all()) and bool((d2[sel] > 0).all())
        assert torch.equal(keep, sel) and torch.equal(counts[:, 1], counts[:, 0])
    # radius 0: the textbook second nearest
    _, _, _, d1, d2, _ = ops.feat_match_filter(pc, img, mask, mutual=False, ratio=0.5, excl_radius=0, want_dist=True)
    for b in range(B):
        rows = torch.nonzero(mask[b]).flatten()
        d = torch.cdist(pc[b * N:(b + 1) * N][rows].double(), img[b].reshape(h * w, 64).double())
        two = d.topk(2, dim=1, largest=False).values
        assert float((d1.view(B, N)[b][rows].double() - two[:, 0]).abs().max()) <= TOL
        assert float((d2.view(B, N)[b][rows].double() - two[:, 1]).abs().max()) <= TOL
    # radius 1 on a 3 x 3 map: only the centre pixel's window covers everything
    img3 = _unit(1, 3, 3, 64, seed=74)
    pc3 = img3.view(9, 64).clone()
    _, keep, _, _, d2, _ = ops.feat_match_filter(pc3, img3, torch.ones(1, 9, dtype=torch.bool, device=DEV), mutual=False, ratio=0.9,
                                                 excl_radius=1, want_dist=True)
    assert torch.isinf(d2).tolist() == [p == 4 for p in range(9)] and bool(keep.all())


def test_duplicate_points_and_duplicate_pixels():
    B, N, h, w = 2, 1000, 40, 128
    img = _unit(B, h, w, 64, seed=9)
    flat = img.view(B, h * w, 64)
    g = torch.Generator(device="cpu").manual_seed(4)
    pix = torch.randperm(h * w, generator=g)[:N].to(DEV)             # point n belongs to its own pixel pix[n]
    pc = torch.nn.functional.normalize(flat[:, pix] + 0.05 * torch.randn(B, N, 64, generator=g).to(DEV), dim=-1)
    # duplicate point features: in one 256-row tile, across tiles, across lane halves
    dups = [(5, 700), (300, 301), (40, 72), (999, 998)]
    for a, c in dups:
        pc[:, c] = pc[:, a]
    pc = pc.reshape(B * N, 64).contiguous()
    mask = torch.ones(B, N, dtype=torch.int64, device=DEV)
    idx, keep, _, _, _, rev = ops.feat_match_filter(pc, img, mask, mutual=True, want_rev=True)
    idx, keep, rev = idx.view(B, N), keep.view(B, N), rev.view(B, h * w)
    for a, c in dups:
        lo, hi = min(a, c), max(a, c)
        assert bool((idx[:, lo] == pix[a]).all()) and bool((idx[:, hi] == pix[a]).all())
        assert bool((rev[:, pix[a]] == lo).all())                      # the mutual tie goes to the lowest n
        assert bool(keep[:, lo].all()) and not bool(keep[:, hi].any())
    # with the lower twin unselected the other one wins
    mask2 = mask.clone()
    mask2[:, 5] = 0
    _, keep2, _, _, _, rev2 = ops.feat_match_filter(pc, img, mask2, mutual=True, want_rev=True)
    assert bool((rev2.view(B, h * w)[:, pix[5]] == 700).all()) and bool(keep2.view(B, N)[:, 700].all())

    # duplicate pixel features: the forward tie goes to the lowest p (different LDS tiles, sub-tiles, lane halves and registers)
    dup = [2 * w + 3, 2 * w + 40, 17 * w + 9, 30 * w + 100, h * w - 1]
    img2 = img.clone()
    img2.view(B, h * w, 64)[:, dup[1:]] = img2.view(B, h * w, 64)[:, dup[:1]]
    near = torch.nn.functional.normalize(img2.view(B, h * w, 64)[:, dup[0]][:, None, :] + 1e-3 * torch.randn(B, N, 64, generator=g).to(DEV), dim=-1)
    near = near.reshape(B * N, 64).contiguous()
    idx, keep, _, _, d2, rev = ops.feat_match_filter(near, img2, mask, mutual=True, ratio=0.9, excl_radius=0, want_dist=True, want_rev=True)
    assert bool((idx == dup[0]).all())
    assert bool((d2 < 0.05).all()) and not bool(keep.any())           # the runner-up is a twin pixel: the plain ratio test rejects all
    assert torch.equal(idx, ops.feat_match(near, img2, mask)[0])
    same = img2.view(B, h * w, 64)[:, :1].expand(B, h * w, 64).reshape(B, h, w, 64).contiguous()
    idx, _, _, _, _, rev = ops.feat_match_filter(near, same, mask, mutual=True, want_rev=True)
    assert bool((idx == 0).all())                                      # every pixel the same feature: pixel 0 wins
    assert len(set(rev.view(B, -1)[0].tolist())) == 1                  # ... and every pixel names the same nearest row


def test_filters_off_keep_the_mask_and_max_dist_alone():
    B, N, h, w = 3, 4097, 40, 128
    s = _scene(ref.planted_scene, dict(B=B, N=N, h=h, w=w, seed=81))
    sel = s["mask"].view(-1) != 0
    idx, keep, counts, d1, d2, rev = ops.feat_match_filter(s["pc"], s["img"], s["mask"], mutual=False, ratio=0.0, max_dist=0.0, gt_xy=s["gt_xy"])
    assert d1 is None and d2 is None and rev is None
    assert torch.equal(keep, sel)
    assert torch.equal(counts[:, 1], counts[:, 0]) and torch.equal(counts[:, 2], counts[:, 3])
    want = ops.feat_match(s["pc"], s["img"], s["mask"], gt_xy=s["gt_xy"])
    assert torch.equal(idx, want[0]) and torch.equal(counts[:, [0, 3]], want[2][:, [0, 1]])
    # max_dist alone: the planted points sit near 0.55 from their pixel, the replaced ones near 1
    _, _, _, d1, _, _ = ops.feat_match_filter(s["pc"], s["img"], s["mask"], mutual=False, want_dist=True)
    bound = 0.8
    idx2, keep2, counts2, _, _, _ = ops.feat_match_filter(s["pc"], s["img"], s["mask"], mutual=False, max_dist=bound, gt_xy=s["gt_xy"])
    assert torch.equal(idx2, idx)
    assert torch.equal(keep2, sel & (d1 <= bound))
    want64 = ref.restate(s["pc"], s["img"], s["mask"], mutual=False, max_dist=bound, gt_xy=s["gt_xy"])
    for b, r in enumerate(want64):
        rows = r["sel"]
        assert float((d1.view(B, N)[b][rows].double() - r["d1"][rows]).abs().max()) <= TOL
        edge = int(((r["d1"][rows] - bound).abs() < TOL).sum()) + int((r["fwd_gap"] < TOL).sum())
        assert abs(int(counts2[b, 1]) - r["counts"][1]) <= edge and abs(int(counts2[b, 2]) - r["counts"][2]) <= edge
        assert 0.3 * rows.numel() < int(counts2[b, 1]) < 0.7 * rows.numel()
        assert int(counts2[b, 2]) >= 0.95 * int(counts2[b, 1])          # what the bound keeps are the planted points


def test_empty_mask_and_mask_dtypes():
    B, N, h, w = 3, 1000, 11, 38
    pc, img = _unit(B * N, 64, seed=91), _unit(B, h, w, 64, seed=92)
    xy = torch.zeros(B, 2, N, device=DEV)
    out = ops.feat_match_filter(pc, img, torch.zeros(B, N, dtype=torch.int64, device=DEV), mutual=True, ratio=0.9, gt_xy=xy, want_dist=True,
                                want_rev=True)
    idx, keep, counts, d1, d2, rev = out
    assert bool((idx == -1).all()) and not bool(keep.any()) and bool((rev == -1).all())
    assert counts.tolist() == [[0, 0, 0, 0]] * B and bool(torch.isnan(d1).all()) and bool(torch.isnan(d2).all())
    # one sample empty, the others not
    mask = _mask("random", B, N, seed=93)
    mask[1] = 0
    kw = dict(mutual=True, ratio=0.95, excl_radius=1, gt_xy=xy, thr=50.0, want_dist=True, want_rev=True)
    a = ops.feat_match_filter(pc, img, mask, **kw)
    assert bool((a[5].view(B, -1)[1] == -1).all()) and a[2][1].tolist() == [0, 0, 0, 0] and int(a[2][0, 1]) > 0
    _same(a, ops.feat_match_filter(pc, img, mask.bool(), **kw))
    _same(a, ops.feat_match_filter(pc, img, mask.to(torch.uint8), **kw))
    _same(a, ops.feat_match_filter(pc, img, (mask * 7).view(B * N), **kw))          # any non-zero selects; [B*N] is accepted


def test_two_calls_agree_and_a_sample_depends_on_its_own_rows():
    B, N, h, w = 3, 4097, 40, 128
    s = _scene(ref.planted_scene, dict(B=B, N=N, h=h, w=w, seed=111))
    kw = dict(mutual=True, ratio=0.9, excl_radius=2, thr=3.0, want_dist=True, want_rev=True)
    a = ops.feat_match_filter(s["pc"], s["img"], s["mask"], gt_xy=s["gt_xy"], **kw)
    _same(a, ops.feat_match_filter(s["pc"], s["img"], s["mask"], gt_xy=s["gt_xy"], **kw))
    o = _scene(ref.planted_scene, dict(B=B, N=N, h=h, w=w, seed=112))
    for k in ("pc", "img", "mask", "gt_xy"):                           # sample 1 stays, samples 0 and 2 are replaced
        o[k] = o[k].clone()
    o["pc"].view(B, N, 64)[1] = s["pc"].view(B, N, 64)[1]
    o["img"][1], o["mask"][1], o["gt_xy"][1] = s["img"][1], s["mask"][1], s["gt_xy"][1]
    c = ops.feat_match_filter(o["pc"], o["img"], o["mask"], gt_xy=o["gt_xy"], **kw)
    _same([t.view(B, -1)[1].contiguous() for t in a], [t.view(B, -1)[1].contiguous() for t in c])
    assert not torch.equal(a[0].view(B, N)[0], c[0].view(B, N)[0])


def test_graph_replay_equals_eager():
    B, N, h, w = 3, 4097, 40, 128
    s = _scene(ref.planted_scene, dict(B=B, N=N, h=h, w=w, seed=121))
    kw = dict(mutual=True, ratio=0.9, excl_radius=2, gt_xy=s["gt_xy"], want_dist=True, want_rev=True)
    eager = ops.feat_match_filter(s["pc"], s["img"], s["mask"], **kw)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ops.feat_match_filter(s["pc"], s["img"], s["mask"], **kw)
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ops.feat_match_filter(s["pc"], s["img"], s["mask"], **kw)
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


def test_pose_from_filtered_matches_end_to_end():
    """pnp_reference.planted gives points, pose and K; point n's feature is the feature of its true rounded pixel plus noise, and half
    of the points carry a random unit feature instead (outlier matches).  With the filters on, 16 hypotheses recover the pose within
    the bars of tests/test_pnp_gpu.py::test_pose_from_matches_on_planted_features (matches are rounded projections, each within
    q = 0.5 * sqrt(2) px of the exact one: rotation <= q / f rad, translation <= q * z_max / f)."""
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

    # default keywords: the unfiltered path, bit for bit a direct match_features + ops.pnp_ransac call
    model.pose_from_matches(data, img_overlap=ov, n_hyp=16)
    assert "pnp_used" not in data
    idx, _, _, w_ = match_features(data, data["pc_overlap_pred"])
    p = idx.long().clamp(min=0)
    use = (idx >= 0) & torch.gather(ov.reshape(B, -1), 1, p)
    uv = torch.stack([p % w_, torch.div(p, w_, rounding_mode="floor")], 1).float().contiguous()
    pose, inl, status = ops.pnp_ransac(data["pc"], uv, use.contiguous(), data["K"], n_hyp=16, thr=1.0, seed=0, refine_iters=10)
    assert torch.equal(data["pnp_pose"].view(torch.int32), pose.view(torch.int32))
    assert torch.equal(data["pnp_inliers"], inl) and torch.equal(data["pnp_status"], status)
    plain_share = data["pnp_inliers"].double() / use.sum(1).double()

    model.pose_from_matches(data, img_overlap=ov, n_hyp=16, mutual=True, ratio=0.9)
    assert data["pnp_status"].tolist() == [0] * B
    q, foc = 0.5 * math.sqrt(2.0), K[0, 0]
    rre, rte = _errors(data["pnp_pose"], s["P"])
    print("filtered: RRE", rre, "RTE", rte, "used", data["pnp_used"].tolist(), "inliers", data["pnp_inliers"].tolist(),
          "| unfiltered inlier share", plain_share.tolist())
    assert max(rre) <= math.degrees(q / foc), (rre, math.degrees(q / foc))
    assert max(rte) <= q * cam[:, 2].max() / foc, (rte, q * cam[:, 2].max() / foc)
    share = data["pnp_inliers"].double() / data["pnp_used"].double()
    assert bool((share > plain_share).all()), (share, plain_share)
    # pnp_used = the kept rows whose matched pixel lies inside the image overlap, from the op's own idx and keep
    rows = data["pc_geo_feat"].permute(0, 2, 1).reshape(B * N, 64).contiguous()
    nhwc = data["img_geo_feat"].permute(0, 2, 3, 1).contiguous()
    fidx, fkeep, _, _, _, _ = ops.feat_match_filter(rows, nhwc, data["pc_overlap_pred"], mutual=True, ratio=0.9, excl_radius=2)
    inside = torch.gather(ov.reshape(B, -1), 1, fidx.view(B, N).long().clamp(min=0))
    want_used = (fkeep.view(B, N) & inside).sum(1)
    assert data["pnp_used"].shape == (B,) and torch.equal(data["pnp_used"].long(), want_used.long())
    assert torch.equal(data["pnp_filter_counts"][:, 1].long(), fkeep.view(B, N).sum(1))
    assert bool((want_used < fkeep.view(B, N).sum(1)).all())              # the overlap mask did remove kept rows
    assert bool((data["pnp_used"] < use.sum(1)).all())


def _script(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "Test_Geo.py"), "--pairs", "2", "--batch-size", "2", "--img", "160x512", "--num-pt", "4096",
           *extra]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    return res.stdout.strip().splitlines()


def _structure(lines):
    """The parent's line structure under --pnp: per batch "IR1 IR2", per pair "RTE RRE", the 5-number summary, the recall block."""
    rec = [i for i, l in enumerate(lines) if l.startswith("Registration Recall:")]
    assert len(rec) == 1, lines
    i = rec[0]
    assert len(lines[i - 1].split()) == 5
    two = [l for l in lines[:i - 1] if len(l.split()) == 2]
    assert len(two) == 3 and all(float(v) >= 0 or math.isnan(float(v)) for l in two for v in l.split()), lines
    recall = float(lines[i].split(":")[1])
    assert 0.0 <= recall <= 1.0
    if recall > 0:
        assert lines[i + 1].startswith("RTE Mean:") and lines[i + 2].startswith("RRE Mean:")
    else:
        assert lines[i + 1:] == []
    return [l for l in lines[:i - 1] if len(l.split()) != 2]


def test_test_geo_script_with_the_filters():
    lines = _script("--pnp", "--mutual", "--ratio", "0.9")
    extra = _structure(lines)
    assert len(extra) == 1 and extra[0].startswith("kept "), lines       # one batch, one extra line
    tok = extra[0].split()
    assert tok[2] == "of" and tok[4] == "IR" and tok[6] == "->" and len(tok) == 8, extra
    assert 0 <= int(tok[1]) <= int(tok[3]) <= 2 * 4096
    for v in (tok[5], tok[7]):
        assert math.isnan(float(v)) or 0.0 <= float(v) <= 1.0
    assert lines.index(extra[0]) == 1                                     # right after the batch's "IR1 IR2" line
    # without the new flags: the parent's structure and no extra line
    assert _structure(_script("--pnp")) == []
