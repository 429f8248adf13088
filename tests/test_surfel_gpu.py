"""GPU tier of oriented-disc (surfel) rendering and the depth test against a brought map: ops.render_surfels and
ops.depth_test held to four yardsticks -- (1) scenes worked by hand with dyadic numbers, exact; (2) exact equalities on
visibility_reference.SCENES: the centres against ops.guided_match, the maps against the float32 restatement of the per-pixel operations
started from the op's own `surfel` output, all-zero normals against ops.render_points' square splat, the gathers, the counts, and
ops.depth_test against ops.visibility; (3) the float64 brute-force restatement in surfel_reference.py on the decided pixels; (4)
determinism -- and one planted scene of the purpose: a wall with every second point removed stops hiding what is behind it for the
one-cell z-buffer, and hides it again as surfels."""
import importlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import surfel_reference as sr
import visibility_reference as vr
from cmr_agent_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
INF = math.inf
f32 = np.float32


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == torch.bool else t.contiguous().view(torch.int32) if t.element_size() == 4 else t.contiguous()


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y))


def _uv(pts, pose, K, h, w, max_px, mask=None):
    """ops.guided_match at radius max_px on zero features -> (in view bool [B, N], proj [B, 2, N])."""
    B, _, N = pts.shape
    every = torch.ones(B, N, dtype=torch.bool, device=DEV) if mask is None else mask
    idx, _, _, _, proj = ops.guided_match(pts, torch.zeros(B * N, 64, device=DEV), torch.zeros(B, h, w, 64, device=DEV), every, pose, K, max_px,
                                          want_proj=True)
    return (idx >= 0).view(B, N), proj


# ---- 1. by hand ---------------------------------------------------------------------------------------------------------------------------------
def _hand(points, normals, **kw):
    pts, nrm, pose, K = (t.to(DEV) for t in sr.hand(points, normals))
    kw = {**dict(radius=0.5, range_slope=0.0, max_px=8, min_cos=0.1), **kw}
    K = kw.pop("K", K)
    out = ops.render_surfels(pts, nrm, pose, K, sr.HAND_H, sr.HAND_W, want_normal_map=True, want_surfel=True, **kw)
    return [None if t is None else t.cpu() for t in out]


def _covered(index_map):
    return sorted((int(x), int(y)) for y, x in np.argwhere(index_map[0].numpy() >= 0))


@pytest.mark.parametrize("normal", [(0.0, 0.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, -4.0)])
def test_hand_fronto_parallel_disc_covers_five_pixels(normal):
    idx, depth, _, counts, nmap, surfel = _hand([(0.0, 0.0, 2.0)], [normal])
    five = sorted([(8, 8), (7, 8), (9, 8), (8, 7), (8, 9)])                       # (x - 8)^2 + (y - 8)^2 <= 1: the rim is inclusive
    assert _covered(idx) == five and counts[0].tolist() == [1, 1, 5, 0]
    assert all(idx[0, y, x] == 0 and depth[0, y, x] == 2.0 for x, y in five) and int(torch.isinf(depth).sum()) == 17 * 17 - 5
    assert idx.dtype == torch.int32 and depth.dtype == torch.float32 and tuple(nmap.shape) == (1, 3, 17, 17) and tuple(surfel.shape) == (1, 8, 1)
    assert surfel[0, :, 0].tolist() == [0.0, 0.0, 2.0, normal[0], normal[1], normal[2], 0.5, 1.0]
    assert nmap[0, :, 8, 8].tolist() == [0.0, 0.0, -1.0] and nmap[0, :, 0, 0].tolist() == [0.0, 0.0, 0.0]      # faces the camera


def test_hand_tilted_disc_is_narrower_and_its_depth_varies():
    flat = _hand([(0.0, 0.0, 2.0)], [(0.0, 0.0, 1.0)], radius=1.0)
    tilt = _hand([(0.0, 0.0, 2.0)], [(1.0, 0.0, 1.0)], radius=1.0)
    row = lambda out: [x for x, y in _covered(out[0]) if y == 8]
    assert row(flat) == [6, 7, 8, 9, 10] and row(tilt) == [7, 8, 9, 10]
    # the plane x + z = 2 under the ray (dx, 0, 1): tau = 2 / (1 + dx), dx = (x - 8) / 4
    want = [f32(2.0) / f32(0.75), f32(2.0), f32(2.0) / f32(1.25), f32(2.0) / f32(1.5)]
    assert [float(tilt[1][0, 8, x]) for x in (7, 8, 9, 10)] == [float(v) for v in want]
    assert [float(flat[1][0, 8, x]) for x in (6, 7, 8, 9, 10)] == [2.0] * 5
    # in y nothing tilts: (8, 8 +- 2) is on the rim of both
    assert tilt[0][0, 6, 8] == 0 and tilt[0][0, 10, 8] == 0 and tilt[0][0, 5, 8] == -1
    s = 1.0 / math.sqrt(2.0)
    assert np.allclose(tilt[4][0, :, 8, 8].numpy(), [-s, 0.0, -s], rtol=0, atol=1e-7)


def test_hand_discs_close_the_gap_between_two_points():
    pts, nrm = [(0.0, 0.0, 2.0), (1.5, 0.0, 2.0)], [(0.0, 0.0, 1.0)] * 2           # pixels (8, 8) and (11, 8)
    idx = _hand(pts, nrm)[0]
    assert idx[0, 8, 7:13].tolist() == [0, 0, 0, 1, 1, 1]
    p, n, pose, K = (t.to(DEV) for t in sr.hand(pts, nrm))
    sparse = ops.render_points(p, pose, K, 17, 17, splat=0)[0].cpu()
    assert sparse[0, 8, 7:13].tolist() == [-1, 0, -1, -1, 1, -1]


def test_hand_near_disc_in_front_of_a_far_one():
    # r = 0.5 z: the far disc (row 0, 2 m wide at depth 4, centre at pixel 10) and the near one (row 1, 0.5 m at depth 1, pixel 8) both
    # reach two pixels; the near one owns every pixel it covers
    idx, depth, _, counts, _, _ = _hand([(2.0, 0.0, 4.0), (0.0, 0.0, 1.0)], [(0.0, 0.0, 1.0)] * 2, radius=0.0, range_slope=0.5)
    assert idx[0, 8, 6:14].tolist() == [1, 1, 1, 1, 1, 0, 0, -1] and depth[0, 8, 6:14].tolist() == [1.0] * 5 + [4.0] * 2 + [INF]
    near = {(x, y) for x in range(17) for y in range(17) if (x - 8) ** 2 + (y - 8) ** 2 <= 4}
    far = {(x, y) for x in range(17) for y in range(17) if (x - 10) ** 2 + (y - 8) ** 2 <= 4}
    assert {(x, y) for x, y in _covered(idx) if idx[0, y, x] == 1} == near and {(x, y) for x, y in _covered(idx) if idx[0, y, x] == 0} == far - near
    assert counts[0].tolist() == [2, 2, len(near | far), 0]


def test_hand_equal_depths_go_to_the_lower_row():
    idx, depth, _, counts, _, _ = _hand([(0.25, 0.0, 2.0), (0.0, 0.0, 2.0), (0.0, 0.0, 2.0), (0.25, 0.0, 2.0)], [(0.0, 0.0, 1.0)] * 4)
    # rows 1 and 2 coincide: row 1 wins; rows 0 and 3 coincide (half a pixel to the right): row 0 wins; where 0 and 1 overlap, row 0
    assert idx[0, 8, 7:10].tolist() == [1, 0, 0] and idx[0, 7, 8] == 1 and bool(((idx == 2) | (idx == 3)).sum() == 0)
    assert counts[0, :2].tolist() == [4, 4]


def test_hand_grazing_disc_is_rejected_by_min_cos():
    pts, nrm = [(0.0, 0.0, 2.0)], [(1.0, 0.0, 0.046875)]                          # the cosine to the central ray is 0.0468 < 0.1
    idx, _, _, counts, _, _ = _hand(pts, nrm)
    assert counts[0].tolist() == [1, 1, 0, 0] and bool((idx == -1).all())
    idx, depth, _, counts, _, _ = _hand(pts, nrm, min_cos=0.03125)
    assert idx[0, 8, 8] == 0 and depth[0, 8, 8] == 2.0 and counts[0, 2] >= 1


def test_hand_rows_that_are_not_drawn():
    pts = [(0.0, 0.0, 0.5), (0.0, 0.0, -2.0), (0.0, 0.0, 2.0), (0.0, 0.0, 2.0), (0.0, 0.0, 0.25)]
    nrm = [(0.0, 0.0, 1.0), (0.0, 0.0, 1.0), (math.nan, 0.0, 1.0), (0.0, math.inf, 1.0), (0.0, 0.0, 1.0)]
    idx, depth, _, counts, nmap, surfel = _hand(pts, nrm)                          # z_c = r, behind, NaN / inf normal, z_c < r
    assert counts[0].tolist() == [5, 0, 0, 0] and bool((idx == -1).all()) and bool(torch.isinf(depth).all()) and bool((nmap == 0).all())
    assert bool(torch.isnan(surfel[0, :7]).all()) and surfel[0, 7].tolist() == [0.0] * 5
    # a K outside the camera model: status 1, nothing drawn, whatever the rows
    for bad in ([[4.0, 0.0, 8.0], [0.0, 4.0, 8.0], [0.0, 0.0, 2.0]], [[4.0, 0.0, 8.0], [0.5, 4.0, 8.0], [0.0, 0.0, 1.0]],
                [[4.0, 0.0, 8.0], [0.0, 4.0, 8.0], [0.0, 0.25, 1.0]], [[-4.0, 0.0, 8.0], [0.0, 4.0, 8.0], [0.0, 0.0, 1.0]],
                [[4.0, 0.0, 8.0], [0.0, math.inf, 8.0], [0.0, 0.0, 1.0]]):
        idx, depth, _, counts, _, surfel = _hand([(0.0, 0.0, 2.0)], [(0.0, 0.0, 1.0)], K=torch.tensor([bad], device=DEV))
        assert counts[0].tolist() == [1, 0, 0, 1] and bool((idx == -1).all()) and bool(torch.isnan(surfel[0, :7]).all())
    # an unselected row is neither selected nor drawn
    p, n, pose, K = (t.to(DEV) for t in sr.hand([(0.0, 0.0, 2.0)] * 2, [(0.0, 0.0, 1.0)] * 2))
    out = ops.render_surfels(p, n, pose, K, 17, 17, radius=0.5, range_slope=0.0, mask=torch.tensor([[0, 1]], dtype=torch.uint8, device=DEV))
    assert out[3][0].tolist() == [1, 1, 5, 0] and out[0][0, 8, 8] == 1 and out[4] is None and out[5] is None


def test_hand_centre_outside_the_map():
    pts, nrm = [(-4.5, 0.0, 2.0)], [(0.0, 0.0, 1.0)]                               # u = -1: one pixel left of the map
    idx, depth, _, counts, _, _ = _hand(pts, nrm)
    assert _covered(idx) == [(0, 8)] and depth[0, 8, 0] == 2.0 and counts[0].tolist() == [1, 1, 1, 0]
    p, n, pose, K = (t.to(DEV) for t in sr.hand(pts, nrm))
    assert ops.render_points(p, pose, K, 17, 17, splat=0)[3][0].tolist() == [1, 0, 0]
    assert _hand(pts, nrm, max_px=0)[3][0].tolist() == [1, 0, 0, 0]                # the window of radius 0 does not touch the map


# large discs close to the camera and far off the axis, one per sample, at max_px = 16 (surfel_reference.window_scene): every covered pixel
# must lie inside the window the kernel walks, so the maps must equal the float32 restatement over the WHOLE (2 max_px + 1)^2 window bit
# for bit, and the float64 brute force on its decided pixels.
@pytest.mark.parametrize("k", range(len(sr.WINDOW_KS)))
def test_window_bound_holds_every_covered_pixel(k):
    pts, nrm, pose, Kb = sr.window_scene(k)
    K, B, slope = sr.WINDOW_KS[k], sr.WINDOW_B, sr.WINDOW_SLOPE
    h = w = sr.HAND_H
    idx, depth, _, counts, _, surfel = ops.render_surfels(F(pts), F(nrm), F(pose), F(Kb), h, w, radius=sr.WINDOW_RADIUS, range_slope=slope, max_px=16,
                                                          min_cos=0.1, want_surfel=True)
    view, uv = _uv(F(pts), F(pose), F(Kb), h, w, 16)
    assert torch.equal(view.view(-1), surfel[:, 7, 0] == 1) and int(counts[:, 1].sum()) >= B // 2
    ridx, rdepth = sr.restate32(surfel, uv, Kb, h, w, 16, 0.1)
    assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(depth.cpu().numpy().view(np.int32), rdepth.view(np.int32))
    ref = sr.render(pts, nrm, None, pose, Kb, h, w, sr.WINDOW_RADIUS, slope, 16, 0.1)
    owned = [int((i >= 0).sum()) for i in idx.cpu()]
    print("owned pixels per disc: largest", max(owned), "mean", sum(owned) / B, "undecided", sum(r["undecided"] for r in ref))
    # the scene does test the bound: some footprint reaches more than a pixel beyond f r / z_c of its centre
    s, own = surfel.cpu().numpy(), idx.cpu().numpy() >= 0
    reach = np.array([np.abs(np.nonzero(own[b])[1] - float(uv[b, 0, 0])).max() if own[b].any() else 0.0 for b in range(B)])
    naive = K[0][0] * s[:, 6, 0] / s[:, 2, 0]
    assert (reach > np.nan_to_num(naive, nan=1e9) + 1.0).any()
    for b, r in enumerate(ref):
        dec = r["decided"]
        assert np.array_equal(idx[b].cpu().numpy()[dec], r["owner_decided"][dec])
    assert sum(r["undecided"] for r in ref) <= B * sr.cap(h * w)


# ---- 2. exact equalities ------------------------------------------------------------------------------------------------------------------------
def _scene_call(name, mask="scene", sl=slice(None), normals=None, attr=None, **kw):
    sc = vr.built(name)
    radius, slope, m = sr.PARAMS[name]
    kw = {**dict(radius=radius, range_slope=slope, max_px=m, min_cos=sr.MIN_COS), **kw}
    mask = sc["mask"] if isinstance(mask, str) else mask
    nrm = sr.normals_for(name) if normals is None else normals
    return ops.render_surfels(F(sc["pts"][sl]), F(nrm[sl]), F(sc["pose"][sl]), F(sc["K"][sl]), sc["h"], sc["w"], attr=None if attr is None else attr[sl],
                              mask=None if mask is None else mask[sl].contiguous().to(DEV), want_normal_map=True, want_surfel=True, **kw)


@pytest.mark.parametrize("mask_dtype", [torch.bool, torch.int64])
@pytest.mark.parametrize("name", [s[0] for s in vr.SCENES])
def test_chain_of_exact_equalities(name, mask_dtype):
    sc = vr.built(name)
    B, _, N = sc["pts"].shape
    h, w = sc["h"], sc["w"]
    radius, slope, m = sr.PARAMS[name]
    mask = sc["mask"].to(mask_dtype)
    attr = torch.randn(B, 5, N, generator=torch.Generator().manual_seed(12)).to(DEV)
    idx, depth, amap, counts, nmap, surfel = _scene_call(name, mask=mask, attr=attr, fill=-7.0)
    # (a) the centres: a row is drawn iff it is in view under guided_match's predicate at radius max_px, its normal is finite, r is finite
    # and > 0 and z_c > r; X_c, n_c and r are cmr_project.h's chains (restated with an exact fma), bit for bit
    view, uv = _uv(F(sc["pts"]), F(sc["pose"]), F(sc["K"]), h, w, m, mask.to(DEV))
    s = surfel.cpu().numpy()
    drawn = s[:, 7] == 1
    Xr, nr, rr = sr.camera32(sc["pts"], sr.normals_for(name), sc["pose"], radius, slope)
    with np.errstate(all="ignore"):
        want_drawn = view.cpu().numpy() & np.isfinite(sr.normals_for(name)).all(1) & np.isfinite(rr) & (rr > 0) & (Xr[:, 2] > rr)
    assert np.array_equal(drawn, want_drawn) and set(np.unique(s[:, 7]).tolist()) <= {0.0, 1.0}
    d3 = np.broadcast_to(drawn[:, None], Xr.shape)
    assert np.array_equal(s[:, 0:3][d3].view(np.int32), Xr[d3].view(np.int32)) and np.array_equal(s[:, 3:6][d3].view(np.int32), nr[d3].view(np.int32))
    assert np.array_equal(s[:, 6][drawn].view(np.int32), rr[drawn].view(np.int32))
    assert np.isnan(s[:, :7][np.broadcast_to(~drawn[:, None], s[:, :7].shape)]).all()
    drawn = torch.from_numpy(drawn).to(DEV)
    # (b) the maps are the float32 restatement of the per-pixel operations from the op's own surfel output
    ridx, rdepth = sr.restate32(surfel, uv, sc["K"], h, w, m, sr.MIN_COS)
    print(name, "counts", counts.tolist())
    assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(depth.cpu().numpy().view(np.int32), rdepth.view(np.int32))
    # (c) the gathers
    own = idx >= 0
    o = idx.clamp(min=0).long().view(B, 1, h * w)
    want_attr = torch.where(own.view(B, 1, h * w), attr.gather(2, o.expand(B, 5, h * w)), torch.full((), -7.0, device=DEV)).view(B, 5, h, w)
    assert torch.equal(_bits(amap), _bits(want_attr))
    # the normal map from the op's own n_c and X_c in numpy float32: correctly rounded square root and divisions
    f = np.float32
    nc, xcs = s[:, 3:6], s[:, 0:3]
    with np.errstate(all="ignore"):
        n2 = (nc[:, 0] * nc[:, 0] + nc[:, 1] * nc[:, 1]) + nc[:, 2] * nc[:, 2]
        nX = (nc[:, 0] * xcs[:, 0] + nc[:, 1] * xcs[:, 1]) + nc[:, 2] * xcs[:, 2]
        unit = nc / np.sqrt(n2)[:, None]
    unit = np.where((nX > 0)[:, None], -unit, unit)
    unit = np.where((n2 == 0)[:, None], np.array([0.0, 0.0, -1.0], f).reshape(1, 3, 1), unit).astype(f)
    on = np.broadcast_to(idx.cpu().numpy().reshape(B, 1, h * w), (B, 3, h * w))
    want_n = np.where(on >= 0, np.take_along_axis(unit, np.maximum(on, 0).astype(np.int64), 2), f(0)).reshape(B, 3, h, w)
    got_n = nmap.cpu().numpy()
    assert np.array_equal(got_n == 0, want_n == 0) and np.array_equal(got_n.view(np.int32)[want_n != 0], want_n.view(np.int32)[want_n != 0])
    assert bool((np.abs((got_n * got_n).sum(1)[idx.cpu().numpy() >= 0] - 1.0) < 1e-5).all())
    # (d) the counts are the sums
    sel = mask.to(DEV).view(B, N) != 0
    want_counts = torch.stack([sel.sum(1), drawn.sum(1), own.view(B, -1).sum(1), torch.zeros(B, device=DEV, dtype=torch.long)], 1).int()
    assert torch.equal(counts, want_counts)


@pytest.mark.parametrize("name,m", sr.ZERO_CASES)
def test_zero_normals_and_a_wide_radius_equal_the_square_splat(name, m):
    sc = vr.built(name)
    zero = np.zeros_like(sc["pts"])
    # the disc is the square window: surfel_reference.ZERO_CASES; the float64 restatement confirms it here again
    kw = dict(radius=0.0, range_slope=sr.ZERO_SLOPE, max_px=m)
    idx, depth, _, counts, _, surfel = _scene_call(name, normals=zero, **kw)
    for b, r in enumerate(sr.render(sc["pts"], zero, sc["mask"], sc["pose"], sc["K"], sc["h"], sc["w"], 0.0, sr.ZERO_SLOPE, m, sr.MIN_COS)):
        rows = r["drawn_sure"] | r["drawn_maybe"]
        assert r["full"][rows].all()
    pidx, pdepth, _, pcounts = ops.render_points(F(sc["pts"]), F(sc["pose"]), F(sc["K"]), sc["h"], sc["w"], mask=sc["mask"].to(DEV), splat=m)
    view0 = _uv(F(sc["pts"]), F(sc["pose"]), F(sc["K"]), sc["h"], sc["w"], 0, sc["mask"].to(DEV))[0]
    drawn = surfel[:, 7] == 1
    # render_points draws the rows whose centre is a cell; the surfel op also those whose window merely touches the map
    extra = drawn & ~view0
    if not bool(extra.any()):
        assert torch.equal(idx, pidx) and torch.equal(_bits(depth), _bits(pdepth))
    inner = torch.zeros(sc["h"], sc["w"], dtype=torch.bool, device=DEV)
    inner[m:sc["h"] - m, m:sc["w"] - m] = True                                     # pixels no outside centre reaches
    if bool(inner.any()):
        assert torch.equal(idx[:, inner], pidx[:, inner]) and torch.equal(_bits(depth[:, inner]), _bits(pdepth[:, inner]))
    # with the rows outside the map masked out, the whole maps agree
    both = (sc["mask"].to(DEV) & view0).contiguous()
    idx2, depth2, _, counts2, _, _ = _scene_call(name, mask=both.cpu(), normals=zero, **kw)
    pidx2, pdepth2, _, pcounts2 = ops.render_points(F(sc["pts"]), F(sc["pose"]), F(sc["K"]), sc["h"], sc["w"], mask=both, splat=m)
    assert torch.equal(idx2, pidx2) and torch.equal(_bits(depth2), _bits(pdepth2)) and torch.equal(counts2[:, :3], pcounts2)


@pytest.mark.parametrize("name,radius", [(s[0], r) for s in vr.SCENES for r in (0, 1, 2, 16)])
def test_depth_test_on_visibilitys_own_map_gives_its_flags(name, radius):
    sc = vr.built(name)
    args = (F(sc["pts"]), F(sc["pose"]), F(sc["K"]))
    mask = sc["mask"].to(DEV)
    occ = None if sc["occ_mask"] is None else sc["occ_mask"].to(DEV)
    for rel_tol, abs_tol in ((vr.REL_TOL, vr.ABS_TOL), (0.0, 0.25)):
        vis, counts, dmap, _, _ = ops.visibility(*args, sc["h"], sc["w"], mask, occ_mask=occ, radius=radius, rel_tol=rel_tol, abs_tol=abs_tol,
                                                 want_depth_map=True)
        got, gcounts = ops.depth_test(*args, dmap, mask, radius=radius, rel_tol=rel_tol, abs_tol=abs_tol)
        assert got.dtype == torch.bool and tuple(got.shape) == tuple(vis.shape) and gcounts.dtype == torch.int32
        assert torch.equal(got, vis) and torch.equal(gcounts, counts[:, :3])
        got64, gcounts64 = ops.depth_test(*args, dmap, mask.long(), radius=radius, rel_tol=rel_tol, abs_tol=abs_tol)
        assert torch.equal(got64, vis) and torch.equal(gcounts64, counts[:, :3])


# include/cmr_hip.h, cmr_depth_test_f32: "a NaN cell is ignored".  Two 5 x 7 maps and eight rows each, placed by hand: K and the pose are
# identities, so the row (x z, y z, z) lands on the cell (x, y) at depth z exactly; every depth is dyadic and both tolerances are 0, so a
# row in view is visible iff z <= the least cell of its window that is not NaN.  (x, y, z, queried, the flag expected at radius (0, 2)).
_NAN_ROWS = [
    [(1, 2, 4.0, True, (True, True)),        # A: its own cell holds 4; the only other cells of its window that hold anything hold NaN
     (0, 0, 4.0, True, (True, True)),        # B: its own cell is NaN; A's 4 is in its window at radius 2, and is not nearer
     (6, 4, 4.0, True, (True, False)),       # C: the 2 at (4, 4) stands next to the NaN at (5, 4), two columns to its left
     (6, 0, 4.0, True, (False, False)),      # D: its own cell holds 2, the NaN at (5, 0) beside it changes nothing
     (1, 1, -4.0, True, (False, False)),     # behind the camera
     (9, 2, 4.0, True, (False, False)),      # beside the map
     (1, 2, 1.0, False, (False, False)),     # not queried
     (4, 4, 1.0, True, (True, True))],       # L: nearer than the 2 of its own cell
    [(3, 2, 4.0, True, (True, False)),       # E: the 2 at (5, 2) is the LAST column of its window: lane 0 of the second lane chunk
     (2, 2, 4.0, True, (True, True)),        # F: the same 2 is one column past its window: lane 1 of that chunk, cut by dx <= radius
     (1, 0, 4.0, True, (True, True)),        # G: the NaN at (3, 0) in the last column of its window
     (3, 2, 1.0, False, (False, False)),     # not queried
     (0, 4, 4.0, True, (True, True)),        # M: NaN right of it and above it, nothing else
     (5, 2, 2.0, True, (True, True)),        # P: as deep as its own cell
     (5, 2, 2.5, True, (False, False)),      # Q: behind its own cell, the NaN at (6, 2) beside it
     (2, 2, -4.0, True, (False, False))]]    # behind the camera
_NAN_CELLS = [{(1, 2): 4.0, (4, 4): 2.0, (6, 0): 2.0, (2, 2): math.nan, (2, 3): math.nan, (0, 0): math.nan, (5, 4): math.nan, (5, 0): math.nan},
              {(5, 2): 2.0, (6, 2): math.nan, (3, 0): math.nan, (1, 4): math.nan, (0, 3): math.nan}]      # (x, y): value; +inf elsewhere


@pytest.mark.parametrize("mask_dtype", [torch.bool, torch.int64])
@pytest.mark.parametrize("radius", [0, 2])
def test_depth_test_ignores_nan_cells(radius, mask_dtype):
    h, w = 5, 7
    pts = F([[[x * z for x, _, z, _, _ in rows], [y * z for _, y, z, _, _ in rows], [z for _, _, z, _, _ in rows]] for rows in _NAN_ROWS])
    mask = torch.tensor([[s for _, _, _, s, _ in rows] for rows in _NAN_ROWS]).to(DEV).to(mask_dtype)
    pose, K = torch.eye(4, device=DEV).repeat(2, 1, 1), torch.eye(3, device=DEV).repeat(2, 1, 1)
    planted = torch.full((2, h, w), INF)
    for b, cells in enumerate(_NAN_CELLS):
        for (x, y), v in cells.items():
            planted[b, y, x] = v
    assert int(torch.isnan(planted).sum()) == 9
    vis, counts = ops.depth_test(pts, pose, K, planted.to(DEV), mask, radius=radius, rel_tol=0.0, abs_tol=0.0)
    emptied, ecounts = ops.depth_test(pts, pose, K, torch.nan_to_num(planted, nan=INF, posinf=INF).to(DEV), mask, radius=radius, rel_tol=0.0,
                                      abs_tol=0.0)
    print("radius", radius, "visible", vis.view(2, -1).int().tolist(), "counts", counts.tolist())
    assert torch.equal(vis, emptied) and torch.equal(counts, ecounts)                                   # (a) NaN = empty
    want = torch.tensor([[e[radius // 2] for _, _, _, _, e in rows] for rows in _NAN_ROWS])
    assert vis.dtype == torch.bool and torch.equal(vis.cpu().view(2, -1), want)                         # (b), (c): by hand, row by row
    assert counts.cpu().tolist() == [[7, 5, int(want[0].sum())], [7, 6, int(want[1].sum())]]


# ---- 3. against float64 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in vr.SCENES])
def test_against_float64(name):
    sc = vr.built(name)
    idx, depth, counts, _, surfel = (t.cpu().numpy() for t in _scene_call(name) if t is not None)      # no attr: no attr_map
    ref = sr.reference(name)
    pixels = sc["h"] * sc["w"]
    for b, r in enumerate(ref):
        dec = r["decided"]
        fin = dec & (r["owner_decided"] >= 0)
        err = np.abs(depth[b].astype(np.float64)[fin] - r["depth_decided"][fin])
        share = float((err / r["bar"][fin]).max()) if fin.any() else 0.0
        fp = r["footprint"][r["footprint"] > 0]
        print(name, "sample", b, "counts", counts[b].tolist(), "float64 sure drawn", r["counts_lo"], "undecided", r["undecided"], "of", pixels,
              "worst share of the depth bar", share, "footprint mean", float(fp.mean()) if fp.size else 0.0, "largest", int(fp.max()) if fp.size else 0)
        assert r["undecided"] <= sr.cap(pixels) and r["status"] == 0 and counts[b, 3] == 0
        assert np.array_equal(idx[b][dec], r["owner_decided"][dec])
        assert np.array_equal(np.isinf(depth[b][dec]), r["owner_decided"][dec] < 0)
        assert (err <= r["bar"][fin]).all()
        assert counts[b, 0] == r["counts_lo"][0] and r["counts_lo"][1] <= counts[b, 1] <= r["counts_lo"][1] + int(r["drawn_maybe"].sum())
        drawn = surfel[b, 7] == 1
        assert drawn[r["drawn_sure"]].all() and not drawn[~(r["drawn_sure"] | r["drawn_maybe"])].any()


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_agree_bit_for_bit():
    _same(_scene_call("n1025_40x128"), _scene_call("n1025_40x128"))


def test_sample_alone_equals_sample_in_batch():
    name = "n257_13x19_occ"
    full = _scene_call(name)
    for k in range(3):
        _same(_scene_call(name, sl=slice(k, k + 1)), tuple(None if t is None else t[k:k + 1] for t in full))


def test_mask_dtypes_agree():
    sc = vr.built("n1025_13x19")
    base = _scene_call("n1025_13x19")
    _same(base, _scene_call("n1025_13x19", mask=sc["mask"].to(torch.uint8)))
    _same(base, _scene_call("n1025_13x19", mask=sc["mask"].long()))
    every = _scene_call("n1025_13x19", mask=None)
    _same(every, _scene_call("n1025_13x19", mask=torch.ones_like(sc["mask"])))
    assert every[3][:, 0].tolist() == [1025] * 3


def _replayed(fn):
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


def test_graph_replay_equals_eager():
    sc = vr.built("n1025_13x19")
    radius, slope, m = sr.PARAMS["n1025_13x19"]
    args = (F(sc["pts"]), F(sr.normals_for("n1025_13x19")), F(sc["pose"]), F(sc["K"]), sc["h"], sc["w"])
    attr, mask = torch.randn(3, 2, 1025, device=DEV), sc["mask"].to(DEV)
    _replayed(lambda: ops.render_surfels(*args, radius=radius, range_slope=slope, max_px=m, attr=attr, mask=mask, want_normal_map=True,
                                         want_surfel=True))
    dmap = ops.render_surfels(*args, radius=radius, range_slope=slope, max_px=m)[1]
    _replayed(lambda: ops.depth_test(args[0], args[2], args[3], dmap, mask, radius=1))


# ---- the purpose: a thinned wall hides what is behind it again --------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(13, 19), (40, 128)])
def test_planted_wall_with_every_second_point_removed(h, w):
    mhm = importlib.import_module("cmr_agent_amd.models.MultiHeadModel")
    sc = vr.planted_occlusion(h, w, seed=311)
    P, K = sc["pose"][0], sc["K"][0]
    xc = P[:3, :3] @ sc["pts"][0] + P[:3, 3:4]
    u, v = np.rint(K[0, 0] * xc[0] / xc[2] + K[0, 2]), np.rint(K[1, 1] * xc[1] / xc[2] + K[1, 2])
    wall = sc["expect"] & (xc[2] < 7.0)
    keep = ~(wall & ((u + v) % 2 == 1))                                           # a checkerboard of the wall is removed
    pts, expect = sc["pts"][:, :, keep], sc["expect"][keep]
    hidden = ~expect
    N = pts.shape[2]
    normal = P[:3, :3].T @ np.array([0.0, 0.0, -1.0])                             # the wall's own, in the cloud's frame
    data = {"pc": F(pts), "K": F(sc["K"]), "pnp_pose": F(sc["pose"]), "pc_overlap_pred": torch.ones(1, N, dtype=torch.bool, device=DEV),
            "pc_geo_feat": torch.zeros(1, 64, N, device=DEV), "img_geo_feat": torch.zeros(1, 64, h, w, device=DEV),
            "pc_normal": F(np.tile(normal[None, :, None], (1, 1, N)))}
    model = mhm.MultiHeadModel.__new__(mhm.MultiHeadModel)
    mhm.MultiHeadModel.visible_points(model, data, radius=0, occluders="all")
    through = data["visible_mask"][0].cpu().numpy()
    assert through[hidden].sum() >= hidden.sum() // 3 and through[expect].all()    # hidden points show through the gaps
    cell = 4.0 / K[0, 0]                                                          # one cell's width at the wall's depth, in metres
    mhm.MultiHeadModel.visible_points(model, data, radius=0, occluders="surfels", surfels=dict(radius=cell))
    got = data["visible_mask"][0].cpu().numpy()
    print("map", h, w, "points", N, "hidden", int(hidden.sum()), "seen through the thinned wall", int(through[hidden].sum()), "with surfels",
          int(got[hidden].sum()), "counts", data["visible_counts"].tolist())
    assert np.array_equal(got, expect) and data["visible_counts"][0].tolist() == [N, N, int(expect.sum())]


# ---- the model layer and the scripts on the device ------------------------------------------------------------------------------------------------
def test_model_layer_on_the_device():
    mhm = importlib.import_module("cmr_agent_amd.models.MultiHeadModel")
    model = mhm.MultiHeadModel.__new__(mhm.MultiHeadModel)                       # the methods under test use no weights
    sc = vr.built("n1025_40x128")
    B, _, N = sc["pts"].shape
    h, w = sc["h"], sc["w"]
    g = torch.Generator().manual_seed(3)
    data = {"pc": F(sc["pts"]), "K": F(sc["K"]), "pnp_pose": F(sc["pose"]), "pc_overlap_pred": sc["mask"].to(DEV),
            "pc_geo_feat": torch.zeros(B, 64, N, device=DEV), "img_geo_feat": torch.zeros(B, 64, h, w, device=DEV),
            "img": torch.rand(B, 3, 4 * h, 4 * w, generator=g).to(DEV)}
    mhm.MultiHeadModel.point_normals(model, data, radius=2.0)
    nrm = data["pc_normal"]
    assert nrm.dtype == torch.float32 and tuple(nrm.shape) == (B, 3, N) and nrm.is_contiguous()
    for b in range(B):
        assert torch.equal(nrm[b], ops.point_normals(data["pc"][b].t().contiguous(), radius=2.0).normals.t())
    length = nrm.norm(dim=1)
    assert bool(((length == 0) | ((length - 1).abs() < 1e-4)).all()) and bool((length > 0).any())
    mhm.MultiHeadModel.render_surfels(model, data, radius=0.15, range_slope=0.03, max_px=6)
    direct = ops.render_surfels(data["pc"], nrm, data["pnp_pose"], data["K"], h, w, radius=0.15, range_slope=0.03, max_px=6, want_normal_map=True)
    _same((data["surfel_index_map"], data["surfel_depth_map"], data["surfel_counts"], data["surfel_normal_map"]),
          (direct[0], direct[1], direct[3], direct[4]))
    assert int(data["surfel_counts"][:, 2].sum()) > 0 and "surfel_attr_map" not in data
    # dense_depth from the discs at the image's size: more samples than from one cell per point, and a denser result
    mhm.MultiHeadModel.dense_depth(model, data, radius=2)
    cells = data["dense_counts"].clone()
    mhm.MultiHeadModel.dense_depth(model, data, radius=2, surfels=dict(radius=0.15, range_slope=0.03))
    K4 = data["K"] * torch.tensor([4.0, 4.0, 1.0], device=DEV).view(1, 3, 1)
    big = ops.render_surfels(data["pc"], nrm, data["pnp_pose"], K4.contiguous(), 4 * h, 4 * w, radius=0.15, range_slope=0.03, max_px=8, min_cos=0.1)
    assert torch.equal(data["surfel_counts"], big[3]) and torch.equal(data["dense_counts"][:, 0], big[3][:, 2])
    assert bool((data["dense_counts"][:, 0] > cells[:, 0]).all()) and bool((data["dense_counts"][:, 2] >= cells[:, 2]).all())
    # visible= with surfels in paint_points: the rows ops.depth_test keeps against the surfel map of the whole cloud
    mhm.MultiHeadModel.paint_points(model, data, mask=data["pc_overlap_pred"], visible=dict(surfels=dict(radius=0.15, range_slope=0.03, max_px=6)))
    keep, kc = ops.depth_test(data["pc"], data["pnp_pose"], data["K"], direct[1], data["pc_overlap_pred"], radius=0, rel_tol=0.05)
    assert int(data["paint_counts"][:, 0].sum()) == int(keep.sum()) == int(kc[:, 2].sum()) and bool((data["point_painted"].view(-1) <= keep).all())


def _run_script(script, *flags):
    cmd = [sys.executable, os.path.join(ROOT, script), "--pairs", "1", "--img", "160x512", "--num-pt", "4096", *flags]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return res.stdout.strip().splitlines()


def _number_free(line):
    def word(t):
        try:
            float(t)
            return "#"
        except ValueError:
            return t
    return [word(t) for t in line.split()]


@pytest.mark.parametrize("script,flags", [("Test_Geo.py", ("--pnp", "--guided", "4,2")), ("Test_Agent.py", ("--refine", "4,2"))])
def test_scripts_with_the_surfel_flags(script, flags, tmp_path):
    out = str(tmp_path / "maps")
    base = (*flags, "--visible", "--dense-depth", out)
    plain = _run_script(script, *base)
    assert not [l for l in plain if l.startswith("surfels ")]
    lines = _run_script(script, *base, "--dense-surfels", "--visible-surfels", "--surfel-max-px", "4")
    sf = [l.split() for l in lines if l.startswith("surfels ")]
    assert len(sf) == 1 and len(sf[0]) == 8 and sf[0][2] == "of" and sf[0][4] == "own" and sf[0][6] == "of"
    assert 0 <= int(sf[0][1]) <= int(sf[0][3]) == 4096 and 0 <= int(sf[0][5]) <= int(sf[0][7]) == 160 * 512
    # the pose the run ends on may leave the cloud out of view (hash-filled weights), so 0 is a legal count; the map that is densified is the
    # discs': its samples are the owned pixels
    samples = [int(l.split()[-1]) for l in lines if l.startswith("dense ")]
    print(script, [l for l in lines if l.startswith(("surfels ", "dense ", "visible "))], "plain", [l for l in plain if l.startswith("dense ")])
    assert samples == [int(sf[0][5])]
    vis = [l.split() for l in lines if l.startswith("visible ")]
    assert len(vis) == 1 and 0 <= int(vis[0][1]) <= int(vis[0][3]) <= int(vis[0][5])
    # every other line keeps the format it has without the new flags (the mean / std lines appear only when a pair is recalled)
    keep = lambda ls: [_number_free(l) for l in ls if not l.startswith("surfels ") and "Mean:" not in l]
    assert keep(lines) == keep(plain)
