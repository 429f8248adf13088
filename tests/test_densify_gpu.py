"""GPU tier of image-guided densification (ops.densify / cmr_densify_f32, MultiHeadModel.dense_depth, Test_Geo.py / Test_Agent.py
--dense-depth).

Yardsticks.  (1) The 3 x 5 scene worked by hand.  (2) The float64 restatement (densify_reference.py) on the pixels it calls decided, within
the bound derived there -- count, counts[:, 0:2], the kept samples and the unfilled pixels exactly; tests/test_densify_cpu.py caps what
it may leave out.  (3) The shapes at which a tiled stencil goes wrong.  (4) An exact chain against torch: count is a box sum of the
validity mask.  (5) Properties: a planted edge, convexity, determinism, isolation, graph replay.  (6) Composition with ops.render_points,
the model layer and the scripts."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import densify_reference as dr
import guided_reference as gref
from cmr_agent_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf
TW, TH = ops.DENSIFY_TILE_W, ops.DENSIFY_TILE_H


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same(a, b):
    """Two result tuples, bit for bit (None only against None)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y))


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check(got, r, depth, attr, keep, fill, who=""):
    """The device's tuple against the restatement `r` (computed with the same keep and fill) -> the worst shares of the bounds."""
    dd, da, conf, count, counts = (None if t is None else t.cpu().numpy() for t in got)
    Bn, h, w = depth.shape
    assert dd.dtype == np.float32 and dd.shape == (Bn, h, w) and conf.dtype == np.float32 and conf.shape == (Bn, h, w)
    assert counts.dtype == np.int32 and counts.shape == (Bn, 3)
    n, dec, sample = r["count"], r["decided"], r["sample"]
    assert float(r["rel"].max()) < 1e-3
    if count is not None:
        assert count.dtype == np.int32 and np.array_equal(count, n)
    assert np.array_equal(counts[:, :2], r["counts"][:, :2])
    und = (~dec).sum((1, 2))
    assert (np.abs(counts[:, 2].astype(np.int64) - r["counts"][:, 2]) <= und).all()
    kept = sample if keep else np.zeros_like(sample)
    # the kept samples: their own bits
    assert np.array_equal(_i32(dd)[kept], _i32(depth)[kept])
    # conf = S0 everywhere, 0 where the window is empty
    S0 = r["conf"]
    assert (conf[n == 0] == 0).all()
    cerr = np.abs(conf.astype(np.float64) - S0)
    cbound = r["rel"] * S0 + n * dr.FLUSH
    assert (cerr <= cbound).all(), (who, float((cerr / np.where(cbound > 0, cbound, 1)).max()))
    # decided and unfilled: +inf and the fill, exactly
    off = dec & ~r["filled"] & ~kept
    assert (dd[off] == INF).all()
    # decided and filled: within REL of the float64 value
    on = dec & r["filled"] & ~kept
    derr = np.abs(dd.astype(np.float64)[on] - r["depth"][on])
    dbound = r["rel"][on] * r["depth"][on]
    assert (derr <= dbound).all(), (who, float((derr / dbound).max()))
    # convexity, undecided pixels included: a filled pixel lies within its window's sample depths
    fin = np.isfinite(dd)
    assert not np.isnan(dd).any() and (dd[fin] >= r["zmin"][fin] * (1 - 1e-6)).all() and (dd[fin] <= r["zmax"][fin] * (1 + 1e-6)).all()
    assert np.array_equal(fin[dec], (r["filled"] | kept)[dec])
    share_a = 0.0
    if attr is not None:
        C = attr.shape[1]
        assert da.dtype == np.float32 and da.shape == (Bn, C, h, w)
        k4, off4, on4 = (np.broadcast_to(m[:, None], da.shape) for m in (kept, off, on))
        assert np.array_equal(_i32(da)[k4], _i32(attr)[k4])
        assert np.array_equal(_i32(da)[off4], _i32(np.full(int(off4.sum()), fill, dtype=np.float32)))
        aerr = np.abs(da.astype(np.float64)[on4] - r["attr"][:, :C][on4])
        abound = np.broadcast_to(r["rel"][:, None], da.shape)[on4] * r["attr_scale"][:, :C][on4]
        assert (aerr <= abound).all(), (who, float((aerr / np.where(abound > 0, abound, 1)).max()))
        share_a = float((aerr / np.where(abound > 0, abound, 1)).max()) if on4.any() else 0.0
        und4 = np.broadcast_to((~dec & ~kept)[:, None], da.shape)
        assert not np.isnan(da[und4]).any() or math.isnan(fill)
    else:
        assert da is None
    share_d = float((derr / dbound).max()) if on.any() else 0.0
    share_c = float((cerr / np.where(cbound > 0, cbound, 1)).max())
    return share_d, share_a, share_c


def _densify(depth, guide=None, attr=None, **kw):
    return ops.densify(T(depth), guide=T(guide), attr=T(attr), **kw)


# ---- 1. the hand scene ------------------------------------------------------------------------------------------------------------------------
def test_hand_scene():
    depth = np.asarray([dr.HAND_DEPTH], dtype=np.float32)
    attr = np.asarray([[dr.HAND_ATTR]], dtype=np.float32)
    dd, da, conf, count, counts = _densify(depth, None, attr, radius=1, sigma_s=dr.HAND_SIGMA_S, fill=dr.HAND_FILL, want_count=True)
    assert dd.dtype == torch.float32 and tuple(dd.shape) == (1, 3, 5) and tuple(da.shape) == (1, 1, 3, 5) and conf.dtype == torch.float32
    assert count.dtype == torch.int32 and counts.dtype == torch.int32 and tuple(counts.shape) == (1, 3)
    assert count[0].tolist() == dr.HAND_COUNT and counts[0].tolist() == dr.HAND_COUNTS
    want = torch.tensor(dr.HAND_DENSE)
    assert torch.equal(torch.isinf(dd[0].cpu()), torch.isinf(want))
    fin = torch.isfinite(want)
    assert torch.allclose(dd[0].cpu()[fin], want[fin], rtol=dr.HAND_TOL, atol=0)
    assert torch.allclose(da[0, 0].cpu(), torch.tensor(dr.HAND_DENSE_ATTR), rtol=dr.HAND_TOL, atol=0)
    assert torch.allclose(conf[0].cpu(), torch.tensor(dr.HAND_CONF), rtol=dr.HAND_TOL, atol=0) and conf[0, 0, 4].item() == 0.0
    for (y, x) in ((0, 0), (1, 2), (2, 4)):
        assert dd[0, y, x].item() == dr.HAND_DEPTH[y][x] and da[0, 0, y, x].item() == dr.HAND_ATTR[y][x] and conf[0, y, x].item() == 1.0
    dd, da, conf, count, counts = _densify(depth, None, attr, radius=1, sigma_s=dr.HAND_SIGMA_S, fill=dr.HAND_FILL, min_weight=0.3)
    assert count is None and counts[0].tolist() == dr.HAND_COUNTS_AT_03
    assert sorted(map(tuple, torch.nonzero(torch.isinf(dd[0])).tolist())) == dr.HAND_UNFILLED_AT_03
    assert all(da[0, 0, y, x].item() == dr.HAND_FILL for y, x in dr.HAND_UNFILLED_AT_03)
    plain = _densify(depth, None, None, radius=1, sigma_s=dr.HAND_SIGMA_S, min_weight=0.3)
    assert plain[1] is None and torch.equal(_bits(plain[0]), _bits(dd)) and torch.equal(_bits(plain[2]), _bits(conf)) and torch.equal(plain[4], counts)


# ---- 2. the random scenes against float64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", dr.GUIDE_PLANES)
@pytest.mark.parametrize("name", dr.SCENE_NAMES)
def test_random_scenes_against_float64(name, planes):
    sc = dr.built(name)
    guide = sc["guide"][:, :planes] if planes else None
    kw = dict(radius=sc["R"], sigma_s=sc["sigma_s"], sigma_r=sc["sigma_r"], min_weight=dr.MIN_WEIGHT, fill=-2.5)
    worst = [0.0, 0.0, 0.0]
    for keep in (True, False):
        r = dr.reference(name, planes) if keep else dr.reference_nokeep(name, planes)
        assert r["undecided"] <= dr.cap(int((r["count"] > 0).sum()))
        for C in dr.ATTR_PLANES:
            attr = sc["attr"][:, :C] if C else None
            for want_count in (True, False):
                got = _densify(sc["depth"], guide, attr, keep=keep, want_count=want_count, **kw)
                assert (got[3] is not None) == want_count
                shares = _check(got, r, sc["depth"], attr, keep, -2.5, who=(name, planes, keep, C))
                worst = [max(a, b) for a, b in zip(worst, shares)]
    r = dr.reference(name, planes)
    print(name, "guide planes", planes, "counts", r["counts"].tolist(), "undecided", r["undecided"], "largest REL", float(r["rel"].max()),
          "worst shares of the bound: depth %.4f attr %.4f conf %.4f" % tuple(worst))


# ---- 3. the shapes at which a tiled stencil goes wrong --------------------------------------------------------------------------------------------
def _random_case(h, w, density, seed, Bn=2, planes=3, C=2):
    rng = np.random.default_rng(seed)
    depth = dr.make_depth(rng, Bn, h, w, density)
    guide = dr.make_guide(rng, Bn, h, w, planes) if planes else None
    attr = np.where(dr.is_sample(depth)[:, None], rng.normal(0, 1, (Bn, C, h, w)), np.nan).astype(np.float32) if C else None
    return depth, guide, attr


def _against_reference(depth, guide, attr, who="", **kw):
    keep, fill = kw.get("keep", True), kw.get("fill", 0.0)
    r = dr.densify(depth, guide, attr, **{k: v for k, v in kw.items() if k != "want_count"})
    assert r["undecided"] <= dr.cap(int((r["count"] > 0).sum())), who
    got = _densify(depth, guide, attr, **kw)
    shares = _check(got, r, depth, attr, keep, fill, who=who)
    print(who, "counts", r["counts"].tolist(), "worst shares", shares)
    return got, r


@pytest.mark.parametrize("h,w", [(1, 1), (1, 40), (40, 1)])
def test_thin_maps_at_the_largest_radius(h, w):
    depth, guide, attr = _random_case(h, w, 0.3, seed=[2, h, w])
    depth[0, 0, 0], attr[0, :, 0, 0] = 7.0, 1.5
    if h * w == 1:
        depth[1], attr[1] = np.inf, np.nan                                       # a map of one empty pixel
    _against_reference(depth, guide, attr, who="%dx%d" % (h, w), radius=16, sigma_s=8.0, sigma_r=0.2, want_count=True)


@pytest.mark.parametrize("R", [3, 16])
@pytest.mark.parametrize("w", [TW - 1, TW, TW + 1])
@pytest.mark.parametrize("h", [TH - 1, TH, TH + 1])
def test_maps_round_the_tile_sides(h, w, R):
    depth, guide, attr = _random_case(h, w, 0.06, seed=[3, h, w, R], Bn=1, C=1)
    _against_reference(depth, guide, attr, who="%dx%d R%d" % (h, w, R), radius=R, sigma_s=R / 2.0, sigma_r=0.15, fill=-1.0, want_count=True)


def test_two_by_two_tiles_with_samples_in_the_corners():
    """A map of 2 x 2 tiles at R = 16: the only samples sit where the four tiles meet and in the map's corners, so whatever a tile fills
    near its inner corner comes out of its neighbours' pixels through the halo."""
    h, w = 2 * TH, 2 * TW
    depth = np.full((2, h, w), np.inf, dtype=np.float32)
    guide = dr.make_guide(np.random.default_rng(4), 2, h, w, 2)
    spots = [(TH - 1, TW - 1), (TH - 1, TW), (TH, TW - 1), (TH, TW), (0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    for i, (y, x) in enumerate(spots):
        depth[0, y, x] = 3.0 + 5.0 * i
    depth[1, TH, TW] = 8.0                                                        # one sample: three of the four tiles see it in their halo only
    attr = np.where(dr.is_sample(depth)[:, None], depth[:, None] * np.asarray([1.0, -0.5], dtype=np.float32).reshape(1, 2, 1, 1), np.nan).astype(np.float32)
    got, r = _against_reference(depth, guide, attr, who="2x2 tiles", radius=16, sigma_s=8.0, sigma_r=0.3, keep=False, want_count=True)
    assert r["counts"][1].tolist() == [1, 33 * 32, r["counts"][1][2]] and got[3][1, 0, TW - 16].item() == 1 and got[3][1, 0, TW - 17].item() == 0
    # without a guide every pixel of sample 1's window hears the lone sample: its depth exactly (w z / w)
    dd = _densify(depth, None, None, radius=16, sigma_s=8.0, min_weight=1e-24)[0]
    assert bool((dd[1][torch.isfinite(dd[1])] == 8.0).all()) and int(torch.isfinite(dd[1]).sum()) == 33 * 32


def test_radius_zero_returns_the_input():
    depth, guide, attr = _random_case(21, 70, 0.3, seed=5)
    for keep in (True, False):
        dd, da, conf, count, counts = _densify(depth, guide, attr, radius=0, keep=keep, fill=-4.0, want_count=True)
        s = torch.from_numpy(dr.is_sample(depth)).to(DEV)
        assert torch.equal(_bits(dd), _bits(torch.where(s, T(depth), torch.full_like(dd, INF))))
        assert torch.equal(_bits(da), _bits(torch.where(s[:, None], T(attr), torch.full_like(da, -4.0))))
        assert torch.equal(conf, s.float()) and torch.equal(count, s.int())
        assert torch.equal(counts.cpu(), torch.stack([s.sum((1, 2))] * 3, 1).int().cpu())


def test_an_empty_map_and_a_full_map():
    h, w = 19, 67
    empty = np.full((2, h, w), np.inf, dtype=np.float32)
    guide = dr.make_guide(np.random.default_rng(6), 2, h, w, 3)
    attr = np.full((2, 2, h, w), np.nan, dtype=np.float32)
    dd, da, conf, count, counts = _densify(empty, guide, attr, radius=8, fill=2.0, want_count=True)
    assert bool((dd == INF).all()) and bool((da == 2.0).all()) and bool((conf == 0).all()) and bool((count == 0).all()) and counts.tolist() == [[0, 0, 0]] * 2
    depth, guide, attr = _random_case(h, w, 1.1, seed=7)
    assert dr.is_sample(depth).all()
    got, r = _against_reference(depth, guide, attr, who="full", radius=4, sigma_s=2.0, sigma_r=0.1, keep=False, want_count=True)
    assert r["counts"].tolist() == [[h * w] * 3] * 2 and got[3].max().item() == 81 and got[3][0, 0, 0].item() == 25


def test_what_is_not_a_sample():
    """0, -1, NaN, +inf and -inf are empty pixels: the result is the result with +inf in their place, bit for bit."""
    depth, guide, attr = _random_case(23, 66, 0.2, seed=8)
    rng = np.random.default_rng(9)
    odd = depth.copy()
    holes = ~dr.is_sample(depth)
    odd[holes] = rng.choice(np.asarray([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, -1e-30], dtype=np.float32), int(holes.sum()))
    assert np.isnan(odd).any() and (odd == 0).any() and (odd == -np.inf).any() and (odd == -1.0).any()
    for keep in (True, False):
        kw = dict(radius=5, sigma_s=2.5, sigma_r=0.1, keep=keep, fill=1.0, want_count=True)
        _same(_densify(odd, guide, attr, **kw), _densify(depth, guide, attr, **kw))
    _against_reference(odd, guide, attr, who="odd holes", radius=5, sigma_s=2.5, sigma_r=0.1, fill=1.0)


def test_nan_fill_lands_on_the_unfilled_pixels_only():
    depth, guide, attr = _random_case(23, 66, 0.03, seed=10)
    dd, da, conf, _, counts = _densify(depth, guide, attr, radius=3, fill=math.nan)
    assert torch.equal(torch.isnan(da), torch.isinf(dd)[:, None].expand_as(da)) and bool(torch.isinf(dd).any()) and bool(torch.isfinite(dd).any())
    assert not bool(torch.isnan(dd).any()) and not bool(torch.isnan(conf).any())
    assert counts[:, 2].tolist() == torch.isfinite(dd).sum((1, 2)).tolist()
    _against_reference(depth, guide, attr, who="nan fill", radius=3, fill=math.nan)


# ---- 4. the exact chain against torch ---------------------------------------------------------------------------------------------------------------
def _box_count(depth, R):
    s = (torch.isfinite(depth) & (depth > 0)).float()[:, None]
    k = 2 * R + 1
    return (torch.nn.functional.avg_pool2d(s, k, stride=1, padding=R, count_include_pad=True)[:, 0] * (k * k)).round().int()


@pytest.mark.parametrize("name", dr.SCENE_NAMES)
def test_count_is_a_box_sum_of_the_validity_mask(name):
    sc = dr.built(name)
    depth = T(sc["depth"])
    _, _, conf, count, counts = ops.densify(depth, radius=sc["R"], want_count=True)
    box = _box_count(depth, sc["R"])
    assert torch.equal(count, box) and torch.equal(conf > 0, box > 0)
    assert counts[:, 0].tolist() == (torch.isfinite(depth) & (depth > 0)).sum((1, 2)).tolist() and counts[:, 1].tolist() == (box > 0).sum((1, 2)).tolist()
    for R in (0, 1, 7, 16):
        assert torch.equal(ops.densify(depth, guide=T(sc["guide"]), radius=R, want_count=True)[3], _box_count(depth, R))


# ---- 5. properties ----------------------------------------------------------------------------------------------------------------------------------
def test_planted_edge():
    """Two fronto-parallel planes at depths 5 and 20 meet at a column where the guide steps from 0 to 1.  With the guide (sigma_r = 0.05:
    the far side's weights are e^-200 times smaller) every filled pixel is within the bound of its own side's depth; without it the
    pixels whose window holds both sides lie strictly between the two."""
    h, w, edge, R = 40, 96, 48, 8
    rng = np.random.default_rng(11)
    side = np.broadcast_to(np.arange(w) >= edge, (2, h, w))
    plane = np.where(side, 20.0, 5.0).astype(np.float32)
    depth = np.where(rng.random((2, h, w)) < 0.1, plane, np.inf).astype(np.float32)
    guide = side[:, None].astype(np.float32)
    kw = dict(radius=R, sigma_s=4.0, sigma_r=0.05, min_weight=1e-3)
    for keep in (True, False):
        r = dr.densify(depth, guide, None, keep=keep, **kw)
        got = _densify(depth, guide, None, keep=keep, want_count=True, **kw)
        _check(got, r, depth, None, keep, 0.0, who="edge")
        dd = got[0].cpu().numpy()
        fin = np.isfinite(dd)
        assert fin.sum() > 0.9 * fin.size
        assert (np.abs(dd[fin].astype(np.float64) - plane[fin]) <= r["rel"][fin] * plane[fin]).all()
    r = dr.densify(depth, None, None, keep=False, **kw)
    dd = _densify(depth, None, None, keep=False, **kw)[0].cpu().numpy()
    both = (r["zmin"] == 5.0) & (r["zmax"] == 20.0)
    near = np.zeros_like(both)
    near[:, :, edge - R:edge + R] = True
    assert both.sum() > 0.5 * near.sum() and not (both & ~near).any()
    assert (dd[both] > 5.0).all() and (dd[both] < 20.0).all()
    one = np.isfinite(dd) & ~both
    assert (np.abs(dd[one].astype(np.float64) - r["depth"][one]) <= r["rel"][one] * r["depth"][one]).all()


def test_two_calls_agree_bit_for_bit():
    sc = dr.built("70x150_d05_r8")
    args = (T(sc["depth"]), T(sc["guide"]), T(sc["attr"]))
    run = lambda: ops.densify(args[0], guide=args[1], attr=args[2], radius=8, sigma_s=4.0, sigma_r=0.05, want_count=True)
    _same(run(), run())


def test_sample_alone_equals_sample_in_batch():
    sc = dr.built("37x53_d08_r16")
    depth, guide, attr = T(sc["depth"]), T(sc["guide"]), T(sc["attr"])
    kw = dict(radius=16, sigma_s=8.0, sigma_r=0.1, want_count=True, keep=False)
    full = ops.densify(depth, guide=guide, attr=attr, **kw)
    for k in range(depth.shape[0]):
        alone = ops.densify(depth[k:k + 1].contiguous(), guide=guide[k:k + 1].contiguous(), attr=attr[k:k + 1].contiguous(), **kw)
        _same(alone, tuple(t[k:k + 1] for t in full))
    # and on the other samples' contents: sample 1 emptied, samples 0 and 2 as they were
    d2 = depth.clone()
    d2[1] = INF
    other = ops.densify(d2, guide=guide, attr=attr, **kw)
    _same(tuple(t[[0, 2]] for t in other), tuple(t[[0, 2]] for t in full))
    assert other[4][1].tolist() == [0, 0, 0]


def test_graph_replay_equals_eager():
    sc = dr.built("37x53_d08_r16")
    depth, guide, attr = T(sc["depth"]), T(sc["guide"]), T(sc["attr"])
    for fn in (lambda: ops.densify(depth, guide=guide, attr=attr, radius=16, sigma_s=8.0, want_count=True),      # the launch above 64 KB of LDS
               lambda: ops.densify(depth, radius=4, keep=False)):
        eager = fn()
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            fn()
        torch.cuda.current_stream().wait_stream(st)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = fn()
        for t in got:
            if t is not None:
                t.fill_(1)
        graph.replay()
        torch.cuda.synchronize()
        _same(got, eager)


def test_non_contiguous_and_off_device_tensors_are_refused():
    depth, guide, attr = (T(a) for a in _random_case(8, 9, 0.3, seed=12))
    msg = "^densify: every tensor must be a contiguous tensor on the same GPU"
    for kw in (dict(depth=depth.transpose(1, 2).contiguous().transpose(1, 2)), dict(guide=guide.transpose(2, 3).contiguous().transpose(2, 3)),
               dict(attr=attr.flip(1).transpose(2, 3).contiguous().transpose(2, 3)), dict(depth=depth.cpu()), dict(guide=guide.cpu()), dict(attr=attr.cpu())):
        a = dict(depth=depth, guide=guide, attr=attr)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            ops.densify(a["depth"], guide=a["guide"], attr=a["attr"])


# ---- 6. composition, the model layer and the scripts ------------------------------------------------------------------------------------------------
_GEO = {}


def _geo():
    """One gref.scene batch and its model, built once -> (scene, model): the small model case of the other port-extension tests."""
    if not _GEO:
        from cmr_agent_amd.config import KittiConfiguration
        from cmr_agent_amd.models import MultiHeadModel
        _GEO["v"] = (gref.scene(B=2, N=1024, h=40, w=128, seed=201), MultiHeadModel(KittiConfiguration(num_pt=1024, device=torch.device(DEV))))
    return _GEO["v"]


def _data(sc):
    B, _, N = sc["pts"].shape
    g = torch.Generator().manual_seed(21)
    mask = torch.rand(B, N, generator=g) < 0.7
    return {"pc": T(sc["pts"]), "K": T(sc["K"]), "P": T(sc["P"]), "pnp_pose": T(sc["start"]), "img": torch.rand(B, 3, 160, 512, generator=g).to(DEV),
            "pc_geo_feat": sc["pc"].view(B, N, 64).permute(0, 2, 1).contiguous().to(DEV),
            "img_geo_feat": sc["img"].permute(0, 3, 1, 2).contiguous().to(DEV), "pc_overlap_pred": mask.to(DEV)}


def test_render_then_densify_equals_densify_of_the_rebuilt_maps():
    sc, _ = _geo()
    data = _data(sc)
    B, _, N = sc["pts"].shape
    attr = torch.stack([data["pc"][:, 2], data["pc_overlap_pred"].float()], 1).contiguous()
    index_map, depth_map, attr_map, rcounts = ops.render_points(data["pc"], data["pnp_pose"], data["K"], 40, 128, attr=attr, fill=0.0)
    guide = data["img"][:, :, ::4, ::4].contiguous()
    got = ops.densify(depth_map, guide=guide, attr=attr_map, radius=6, want_count=True)
    # the same maps from the owner indices in torch, NaN where render_points wrote its fill: densify reads attributes at samples only
    own = index_map.view(B, -1).clamp(min=0).long()
    owned = (index_map >= 0)
    pose_d = ops.visibility(data["pc"], data["pnp_pose"], data["K"], 40, 128, torch.ones(B, N, dtype=torch.bool, device=DEV), radius=0, want_depth=True)[4].view(B, N)
    depth2 = torch.where(owned, pose_d.gather(1, own).view(B, 40, 128), torch.full_like(depth_map, -1.0)).contiguous()      # empty as -1, not +inf
    attr2 = torch.where(owned[:, None], attr.gather(2, own[:, None].expand(B, 2, -1)).view(B, 2, 40, 128), torch.full_like(attr_map, math.nan)).contiguous()
    _same(ops.densify(depth2, guide=guide, attr=attr2, radius=6, want_count=True), got)
    assert got[4][:, 0].tolist() == rcounts[:, 2].tolist() and not bool(torch.isnan(got[1]).any())
    assert int(got[4][:, 2].sum()) > int(got[4][:, 0].sum()) > 0                  # it does densify


def test_model_dense_depth():
    sc, model = _geo()
    data = _data(sc)
    B, _, N = sc["pts"].shape
    model.dense_depth(data)
    dd, conf, cnt = data["dense_depth_map"], data["dense_conf_map"], data["dense_counts"]
    assert dd.dtype == torch.float32 and tuple(dd.shape) == (B, 160, 512) and tuple(conf.shape) == (B, 160, 512) and tuple(cnt.shape) == (B, 3)
    assert "dense_attr_map" not in data
    K4 = data["K"].clone()
    K4[:, :2] *= 4.0                                                              # 160 / 40 = 512 / 128 = 4
    _, depth_map, _, rcounts = ops.render_points(data["pc"], data["pnp_pose"], K4, 160, 512)
    direct = ops.densify(depth_map, guide=data["img"])
    assert torch.equal(_bits(dd), _bits(direct[0])) and torch.equal(_bits(conf), _bits(direct[2])) and torch.equal(cnt, direct[4])
    assert cnt[:, 0].tolist() == rcounts[:, 2].tolist() and int(cnt[:, 2].sum()) > int(cnt[:, 0].sum()) > 0
    # visible=True, an attribute, a mask and every filter parameter
    attr = data["pc_overlap_pred"].float()[:, None].contiguous()
    model.dense_depth(data, pose=T(sc["P"]), attr=attr, mask=data["pc_overlap_pred"], visible=True, splat=1, radius=5, sigma_s=2.0, sigma_r=0.2, min_weight=0.01,
                      keep=False, fill=-1.0)
    vis = ops.visibility(data["pc"], T(sc["P"]), data["K"], 40, 128, data["pc_overlap_pred"], radius=1, rel_tol=0.05)[0]
    _, depth_map, attr_map, _ = ops.render_points(data["pc"], T(sc["P"]), K4, 160, 512, attr=attr, mask=vis, splat=1, fill=-1.0)
    direct = ops.densify(depth_map, guide=data["img"], attr=attr_map, radius=5, sigma_s=2.0, sigma_r=0.2, min_weight=0.01, keep=False, fill=-1.0)
    _same((data["dense_depth_map"], data["dense_attr_map"], data["dense_conf_map"], data["dense_counts"]), (direct[0], direct[1], direct[2], direct[4]))
    am = data["dense_attr_map"]
    assert tuple(am.shape) == (B, 1, 160, 512) and bool(((am == -1.0) | ((am > 0.999) & (am < 1.001))).all())
    # size and K: the geometric map's resolution with a guide of that size
    small = torch.rand(B, 1, 40, 128, generator=torch.Generator().manual_seed(23)).to(DEV)
    model.dense_depth(data, size=(40, 128), K=data["K"], guide=small, radius=3)
    direct = ops.densify(ops.render_points(data["pc"], data["pnp_pose"], data["K"], 40, 128)[1], guide=small, radius=3)
    assert torch.equal(_bits(data["dense_depth_map"]), _bits(direct[0])) and torch.equal(data["dense_counts"], direct[4])


def _run(script, *flags):
    cmd = [sys.executable, os.path.join(ROOT, script), "--pairs", "2", "--img", "160x512", "--num-pt", "4096", *flags]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return res.stdout.strip().splitlines()


def _read_pfm(path):
    raw = open(path, "rb").read()
    magic, dims, scale, payload = raw.split(b"\n", 3)
    w, h = (int(t) for t in dims.split())
    assert magic == b"Pf" and scale == b"-1.0" and len(payload) == 4 * w * h
    return np.frombuffer(payload, "<f4").reshape(h, w)[::-1]


def _check_script(script, flags, extra, tmp_path):
    plain = _run(script, *flags)
    assert not [l for l in plain if l.startswith("dense ")]
    out = str(tmp_path / "maps")
    lines = _run(script, *flags, "--dense-depth", out, *extra)
    shown = [l.split() for l in lines if l.startswith("dense ")]
    print(script, extra, shown)
    assert shown and all(len(t) == 6 and t[2] == "of" and t[4] == "from" for t in shown), lines
    # the same seed: every other line is what the run prints without the flag, byte for byte
    assert [l for l in lines if not l.startswith("dense ")] == plain
    assert sorted(os.listdir(out)) == ["pair_0_depth.pfm", "pair_1_depth.pfm"]
    maps = [_read_pfm(os.path.join(out, "pair_%d_depth.pfm" % i)) for i in range(2)]
    assert all(m.shape == (160, 512) and np.isfinite(m).all() and (m >= 0).all() for m in maps)
    # the printed lines are dense_counts summed: filled pixels = the non-zero pixels of the files, of all the pixels, from the samples
    assert sum(int(t[1]) for t in shown) == sum(int((m > 0).sum()) for m in maps) and sum(int(t[3]) for t in shown) == 2 * 160 * 512
    assert all(0 <= int(t[5]) <= int(t[1]) <= int(t[3]) for t in shown)          # keep: every sample is a filled pixel
    return shown


def test_test_geo_script_dense_depth(tmp_path):
    shown = _check_script("Test_Geo.py", ("--pnp",), (), tmp_path)
    assert sum(int(t[5]) for t in shown) > 0 and sum(int(t[1]) for t in shown) > sum(int(t[5]) for t in shown)


def test_test_agent_script_dense_depth(tmp_path):
    _check_script("Test_Agent.py", (), ("--dense-radius", "4", "--dense-sigma-r", "0.2", "--dense-visible"), tmp_path)
