"""GPU tier of point painting and z-buffered attribute rendering (ops.paint_points / cmr_paint_points_f32, ops.render_points /
cmr_render_points_f32, MultiHeadModel.paint_points / render_points, Test_Geo.py / Test_Agent.py --paint).

Yardsticks.  (1) Scenes done by hand, exact.  (2) A chain of exact equalities against what exists: uv is ops.guided_match's proj, painted
and the nearest pixel are ops.visibility's cell, the bilinear value is the plain fp32 torch restatement from uv, the maps are a torch
scatter-min of int64 keys built from the op's own depth bits and row numbers -- all bit for bit.  (3) The float64 restatement
(point_image_reference.py) on the rows and cells it calls decided, within the bound derived there; tests/test_point_image_cpu.py caps
what it may leave out.  (4) The round trip: painting the rendered attribute map returns the attribute.  (5) Properties.  (6) The model
layer and the scripts."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guided_reference as gref
import point_image_reference as pir
import visibility_reference as vr
from cmr_agent_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
INF = math.inf
SPLATS = (0, 1, 4)


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == torch.bool else t.contiguous().view(torch.int32) if t.element_size() == 4 else t.contiguous()


def _same(a, b):
    """Two result tuples, bit for bit (None only against None)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y))


def _paint(sc, image, mode="bilinear", mask="scene", pose=None, sl=slice(None), want_uv=True):
    mask = sc["mask"] if isinstance(mask, str) else mask
    pose = sc["pose"] if pose is None else pose
    return ops.paint_points(F(sc["pts"][sl]), F(pose[sl]), F(sc["K"][sl]), image[sl].contiguous().to(DEV),
                            mask=None if mask is None else mask[sl].contiguous().to(DEV), mode=mode, want_uv=want_uv)


def _render(sc, attr=None, splat=0, fill=0.0, mask="scene", pose=None, sl=slice(None)):
    mask = sc["mask"] if isinstance(mask, str) else mask
    pose = sc["pose"] if pose is None else pose
    return ops.render_points(F(sc["pts"][sl]), F(pose[sl]), F(sc["K"][sl]), sc["h"], sc["w"], attr=None if attr is None else attr[sl].contiguous().to(DEV),
                             mask=None if mask is None else mask[sl].contiguous().to(DEV), splat=splat, fill=fill)


# ---- 1. the hand scenes ---------------------------------------------------------------------------------------------------------------------
def test_hand_scene_painted():
    pts, pose, K, img = (t.to(DEV) for t in pir.hand_paint())
    N = pts.shape[2]
    colors, painted, counts, uv = ops.paint_points(pts, pose, K, img, want_uv=True)
    assert colors.dtype == torch.float32 and tuple(colors.shape) == (1, 1, N) and painted.dtype == torch.bool and tuple(painted.shape) == (N,)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (1, 2) and uv.dtype == torch.float32 and tuple(uv.shape) == (1, 2, N)
    assert painted.int().tolist() == pir.HAND_PAINTED and counts[0].tolist() == [N, sum(pir.HAND_PAINTED)]
    assert colors[0, 0].tolist() == pir.HAND_BILINEAR
    want_uv = [[r[0] for r in pir.HAND_PAINT_ROWS], [r[1] for r in pir.HAND_PAINT_ROWS]]
    got = uv[0].cpu()
    assert bool(torch.isnan(got[:, 5]).all()) and [[v for i, v in enumerate(row) if i != 5] for row in got.tolist()] == [
        [v for i, v in enumerate(row) if i != 5] for row in want_uv]
    colors, painted, counts, uv = ops.paint_points(pts, pose, K, img, mode="nearest")
    assert uv is None and colors[0, 0].tolist() == pir.HAND_NEAREST and painted.int().tolist() == pir.HAND_PAINTED
    # a mask composes: unselected rows are not painted, cost nothing and count nowhere
    m = torch.tensor([[1, 0, 1, 0, 1, 1, 0, 0, 1]], dtype=torch.bool, device=DEV)
    colors, painted, counts, uv = ops.paint_points(pts, pose, K, img, mask=m, want_uv=True)
    assert painted.int().tolist() == [1, 0, 1, 0, 0, 0, 0, 0, 0] and counts[0].tolist() == [5, 2]
    assert colors[0, 0].tolist() == [28.25, 0.0, 19.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0] and bool(torch.isnan(uv[0, :, [1, 3, 5, 6, 7]]).all())


@pytest.mark.parametrize("splat", [0, 1])
def test_hand_scene_rendered(splat):
    pts, pose, K = (t.to(DEV) for t in vr.hand())
    N = pts.shape[2]
    attr = (torch.arange(N, dtype=torch.float32, device=DEV) * 10.0 + 1.0).view(1, 1, N).repeat(1, 2, 1).contiguous()
    attr[:, 1] *= -1.0
    index_map, depth_map, attr_map, counts = ops.render_points(pts, pose, K, vr.HAND_H, vr.HAND_W, attr=attr, splat=splat, fill=-7.0)
    assert index_map.dtype == torch.int32 and tuple(index_map.shape) == (1, vr.HAND_H, vr.HAND_W) and depth_map.dtype == torch.float32
    assert tuple(attr_map.shape) == (1, 2, vr.HAND_H, vr.HAND_W) and counts.dtype == torch.int32 and tuple(counts.shape) == (1, 3)
    assert index_map[0].tolist() == pir.HAND_INDEX[splat] and counts[0].tolist() == pir.HAND_RENDER_COUNTS[splat]
    assert np.array_equal(depth_map[0].cpu().numpy(), pir.hand_depth(pir.HAND_INDEX[splat]))
    idx = np.asarray(pir.HAND_INDEX[splat])
    want = np.where(idx >= 0, idx * 10.0 + 1.0, -7.0).astype(np.float32)
    assert np.array_equal(attr_map[0, 0].cpu().numpy(), want) and np.array_equal(attr_map[0, 1].cpu().numpy(), np.where(idx >= 0, -want, -7.0).astype(np.float32))
    plain = ops.render_points(pts, pose, K, vr.HAND_H, vr.HAND_W, splat=splat)
    assert plain[2] is None and torch.equal(plain[0], index_map) and torch.equal(_bits(plain[1]), _bits(depth_map)) and torch.equal(plain[3], counts)


def test_equal_depths_go_to_the_lowest_row():
    pts = torch.tensor([[[8.0, 6.0, 6.0, 6.0], [2.0, 4.0, 4.0, 4.0], [2.0, 2.0, 2.0, 2.0]]], device=DEV)      # (4, 1) once, (3, 2) three times, all at depth 2
    eye4, eye3 = torch.eye(4, device=DEV)[None].contiguous(), torch.eye(3, device=DEV)[None].contiguous()
    index_map, depth_map, _, counts = ops.render_points(pts, eye4, eye3, 8, 10)
    assert index_map[0, 2, 3].item() == 1 and index_map[0, 1, 4].item() == 0 and counts[0].tolist() == [4, 4, 2]
    index_map, _, _, _ = ops.render_points(pts, eye4, eye3, 8, 10, mask=torch.tensor([[1, 0, 1, 1]], device=DEV), splat=1)
    assert index_map[0, 2, 3].item() == 0 and index_map[0, 3, 2].item() == 2 and index_map[0, 0, 5].item() == 0


# ---- 2. exact equalities against what exists --------------------------------------------------------------------------------------------------
def _bilinear_fp32(image, uv, painted):
    """The contract in plain fp32 torch from the op's own uv: floor, subtract, three lerps a + t (b - a), clamped indices -> [B, C, N]."""
    B, C, H, W = image.shape
    N = uv.shape[2]
    u, v = torch.where(painted, uv[:, 0], torch.zeros_like(uv[:, 0])), torch.where(painted, uv[:, 1], torch.zeros_like(uv[:, 1]))
    x0, y0 = torch.floor(u), torch.floor(v)
    fx, fy = (u - x0)[:, None], (v - y0)[:, None]
    xa, xb = x0.long().clamp(0, W - 1), (x0.long() + 1).clamp(0, W - 1)
    ya, yb = y0.long().clamp(0, H - 1), (y0.long() + 1).clamp(0, H - 1)
    flat = image.reshape(B, C, H * W)
    tap = lambda y, x: flat.gather(2, (y * W + x)[:, None].expand(B, C, N))
    lerp = lambda a, b, t: a + t * (b - a)
    val = lerp(lerp(tap(ya, xa), tap(ya, xb), fx), lerp(tap(yb, xa), tap(yb, xb), fx), fy)
    return torch.where(painted[:, None], val, torch.zeros_like(val))


@pytest.mark.parametrize("C", pir.CHANNELS)
@pytest.mark.parametrize("name", pir.SCENE_NAMES)
def test_painting_chain_of_exact_equalities(name, C):
    sc = pir.built(name)
    B, _, N = sc["pts"].shape
    h, w = sc["h"], sc["w"]
    image = pir.image(name, C).to(DEV)
    mask = sc["mask"] if C in (1, 5) else sc["mask"].long() * 3                    # both mask dtypes over the cases
    colors, painted, counts, uv = _paint(sc, image, mask=mask)
    sel = sc["mask"].to(DEV)
    # (a) uv is guided_match's proj at radius 0
    zero_pc, zero_img = torch.zeros(B * N, 64, device=DEV), torch.zeros(B, h, w, 64, device=DEV)
    _, _, gcounts, _, proj = ops.guided_match(F(sc["pts"]), zero_pc, zero_img, sel, F(sc["pose"]), F(sc["K"]), 0, want_proj=True)
    assert torch.equal(_bits(uv), _bits(proj))
    # (b) painted is ops.visibility's "in view" on the selected rows
    _, vcounts, _, cell, _ = ops.visibility(F(sc["pts"]), F(sc["pose"]), F(sc["K"]), h, w, sel, occ_mask=sel, radius=0, want_cell=True)
    cell, painted2 = cell.view(B, N), painted.view(B, N)
    assert torch.equal(painted2, sel & (cell >= 0))
    assert torch.equal(counts, torch.stack([sel.sum(1), painted2.sum(1)], 1).int()) and torch.equal(counts, vcounts[:, :2]) and torch.equal(counts, gcounts[:, :2])
    print(name, "C", C, "counts", counts.tolist())
    # (c) nearest colours are the image gathered at that cell
    ncolors, npainted, ncounts, _ = _paint(sc, image, mode="nearest", mask=mask, want_uv=False)
    gathered = image.reshape(B, C, h * w).gather(2, cell.clamp(min=0).long()[:, None].expand(B, C, N))
    assert torch.equal(_bits(ncolors), _bits(torch.where(painted2[:, None], gathered, torch.zeros_like(gathered))))
    assert torch.equal(npainted, painted) and torch.equal(ncounts, counts)
    # (d) bilinear colours are the fp32 torch restatement from uv
    assert torch.equal(_bits(colors), _bits(_bilinear_fp32(image, uv, painted2)))
    assert bool((colors[~painted2[:, None].expand(B, C, N)] == 0).all())


def _keys_restated(cell, depth, sel, h, w, splat):
    """int64 keys from the op's depth bits and row numbers, scatter_reduce(amin) at the op's cell, the minimum over the shifted slices."""
    B, N = cell.shape
    empty = torch.iinfo(torch.int64).max
    view = sel & (cell >= 0)
    key = (depth.contiguous().view(torch.int32).long() << 32) | torch.arange(N, device=DEV)[None]
    key = torch.where(view, key, torch.full_like(key, empty))
    km = torch.full((B, h * w), empty, dtype=torch.int64, device=DEV).scatter_reduce(1, cell.clamp(min=0).long(), key, "amin", include_self=True)
    km = km.view(B, h, w)
    if splat:
        pad = torch.full((B, h + 2 * splat, w + 2 * splat), empty, dtype=torch.int64, device=DEV)
        pad[:, splat:splat + h, splat:splat + w] = km
        km = torch.stack([pad[:, dy:dy + h, dx:dx + w] for dy in range(2 * splat + 1) for dx in range(2 * splat + 1)]).amin(0)
    owned = km != empty
    return torch.where(owned, km & 0xffffffff, torch.full_like(km, -1)).int(), owned


@pytest.mark.parametrize("C", pir.CHANNELS)
@pytest.mark.parametrize("name", pir.SCENE_NAMES)
def test_rendering_chain_of_exact_equalities(name, C):
    sc = pir.built(name)
    B, _, N = sc["pts"].shape
    h, w = sc["h"], sc["w"]
    attr = pir.attr(name, C).to(DEV)
    mask = sc["mask"].to(torch.uint8) if C in (1, 5) else sc["mask"].long()
    sel = sc["mask"].to(DEV)
    _, vcounts, vmap, cell, depth = ops.visibility(F(sc["pts"]), F(sc["pose"]), F(sc["K"]), h, w, sel, occ_mask=sel, radius=0,
                                                   want_depth_map=True, want_cell=True, want_depth=True)
    cell, depth = cell.view(B, N), depth.view(B, N)
    for splat in SPLATS:
        index_map, depth_map, attr_map, counts = _render(sc, attr=attr, splat=splat, fill=-3.5, mask=mask)
        rindex, owned = _keys_restated(cell, depth, sel, h, w, splat)
        assert torch.equal(index_map, rindex)
        own = index_map.view(B, h * w).clamp(min=0).long()
        rdepth = torch.where(owned.view(B, -1), depth.gather(1, own), torch.full((B, h * w), INF, device=DEV)).view(B, h, w)
        assert torch.equal(_bits(depth_map), _bits(rdepth))
        if splat == 0:
            assert torch.equal(_bits(depth_map), _bits(vmap))
        rattr = torch.where(owned.view(B, 1, -1), attr.gather(2, own[:, None].expand(B, C, h * w)), torch.full((B, C, h * w), -3.5, device=DEV))
        assert torch.equal(_bits(attr_map), _bits(rattr.view(B, C, h, w)))
        rcounts = torch.stack([sel.sum(1), (sel & (cell >= 0)).sum(1), owned.view(B, -1).sum(1)], 1).int()
        assert torch.equal(counts, rcounts) and torch.equal(counts[:, :2], vcounts[:, :2])
        print(name, "C", C, "splat", splat, "counts", counts.tolist())


# ---- 3. against float64 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pir.SCENE_NAMES)
def test_painting_against_float64(name):
    """|c - c64| <= 2 G delta + 16 2^-23 M on every decided painted row (point_image_reference.py); the largest share of that bound seen on
    an MI355X is recorded in DESIGN.md 4s."""
    sc = pir.built(name)
    B, _, N = sc["pts"].shape
    C = 3
    image = pir.image(name, C)
    colors, painted, counts = (t.cpu().numpy() for t in _paint(sc, image.to(DEV), want_uv=False)[:3])
    ncolors = _paint(sc, image.to(DEV), mode="nearest", want_uv=False)[0].cpu().numpy()
    ref = pir.paint(sc["pts"], sc["mask"], sc["pose"], sc["K"], image)
    painted = painted.reshape(B, N)
    img = image.numpy()
    worst = 0.0
    for b, r in enumerate(ref):
        dec = r["decided"]
        assert r["undecided"] <= vr.cap(int(r["sel"].sum()))
        assert np.array_equal(painted[b][dec], r["painted"][dec])
        assert not painted[b][~r["sel"]].any() and not painted[b][~r["view_any"]].any()
        assert int(r["painted"].sum()) <= counts[b, 1] <= int(r["painted"].sum()) + r["undecided"] and counts[b, 0] == int(r["sel"].sum())
        on = r["painted"]                                                         # decided and painted
        err = np.abs(colors[b][:, on].astype(np.float64) - r["bilinear"][:, on])
        share = float((err / r["bound"][:, on]).max()) if on.any() else 0.0
        worst = max(worst, share)
        print(name, "sample", b, "counts", counts[b].tolist(), "undecided", r["undecided"], "worst share of the bilinear bound", share)
        assert (err <= r["bound"][:, on]).all()
        # an undecided row that the op painted is held to the same bound: the interpolant is continuous
        extra = painted[b] & ~dec
        assert (np.abs(colors[b][:, extra].astype(np.float64) - r["bilinear"][:, extra]) <= r["bound"][:, extra]).all()
        # nearest: the pixel at the row's only candidate centre, or at one of its candidates when it lies within EPS_PX of a half-integer
        uniq = on & r["unique"]
        assert np.array_equal(ncolors[b][:, uniq], r["nearest"][:, uniq].astype(np.float32))
        cxl, cxh, cyl, cyh = r["cand"]
        H, W = img.shape[2:]
        for n in np.nonzero(painted[b] & ~r["unique"])[0]:
            cands = [img[b][:, y, x] for x in (cxl[n], cxh[n]) for y in (cyl[n], cyh[n]) if 0 <= x < W and 0 <= y < H]
            assert any(np.array_equal(ncolors[b][:, n], c) for c in cands)
    print(name, "worst share of the bilinear bound", worst)


@pytest.mark.parametrize("splat", [0, 1])
@pytest.mark.parametrize("name", pir.SCENE_NAMES)
def test_rendering_against_float64(name, splat):
    sc = pir.built(name)
    index_map, depth_map, counts = (t.cpu().numpy() for t in _render(sc, splat=splat) if t is not None)
    ref = pir.render(sc["pts"], sc["mask"], sc["pose"], sc["K"], sc["h"], sc["w"], splat)
    for b, r in enumerate(ref):
        dec, Z64, Z32 = r["decided"], r["depth"], depth_map[b].astype(np.float64)
        assert np.array_equal(np.isinf(Z32[dec]), np.isinf(Z64[dec])) and np.array_equal(index_map[b][dec] < 0, np.isinf(Z64[dec]))
        fin = dec & np.isfinite(Z64)
        err = np.abs(Z32[fin] - Z64[fin])
        assert (err <= r["err"][fin]).all()                                       # 4r's bound: 8 2^-23 S
        idec = r["index_decided"]
        assert np.array_equal(index_map[b][idec], r["index"][idec])
        assert counts[b, 0] == r["selected"] and r["in_view_lo"] <= counts[b, 1] <= r["in_view_lo"] + r["view_undecided"]
        print(name, "splat", splat, "sample", b, "counts", counts[b].tolist(), "decided pixels", int(dec.sum()), "owner decided", int(idec.sum()), "of", dec.size,
              "worst share of the depth bound", float((err / r["err"][fin]).max()) if fin.any() else 0.0)


# ---- 4. the round trip ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pir.SCENE_NAMES)
def test_round_trip(name):
    """Every row that owns its cell at splat 0 gets its own attribute back when the attribute map is painted onto the cloud in nearest mode."""
    sc = pir.built(name)
    B, _, N = sc["pts"].shape
    attr = pir.attr(name, 5).to(DEV)
    index_map, _, attr_map, counts = _render(sc, attr=attr, fill=math.nan)
    colors, painted, _, _ = _paint(sc, attr_map, mode="nearest", want_uv=False)
    owner = torch.zeros(B, N, dtype=torch.bool, device=DEV)
    rows = index_map.view(B, -1)
    for b in range(B):
        owner[b, rows[b][rows[b] >= 0].long()] = True
    assert int(owner.sum()) == int(counts[:, 2].sum()) and bool((owner <= painted.view(B, N)).all())
    assert torch.equal(_bits(colors.permute(0, 2, 1)[owner]), _bits(attr.permute(0, 2, 1)[owner]))
    # a painted row that does not own its cell reads the owner's attribute, never the fill
    assert not bool(torch.isnan(colors).any())


# ---- 5. properties ------------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_agree_bit_for_bit():
    sc = pir.built("n1025_40x128")
    image, attr = pir.image("n1025_40x128", 5), pir.attr("n1025_40x128", 5)
    _same(_paint(sc, image), _paint(sc, image))
    _same(_render(sc, attr=attr, splat=2), _render(sc, attr=attr, splat=2))


def test_sample_alone_equals_sample_in_batch():
    name = "n257_13x19_occ"
    sc = pir.built(name)
    B, _, N = sc["pts"].shape
    image, attr = pir.image(name, 3), pir.attr(name, 3)
    colors, painted, counts, uv = _paint(sc, image)
    index_map, depth_map, attr_map, rcounts = _render(sc, attr=attr, splat=1)
    for k in range(B):
        rows = slice(k * N, (k + 1) * N)
        _same(_paint(sc, image, sl=slice(k, k + 1)), (colors[k:k + 1], painted[rows], counts[k:k + 1], uv[k:k + 1]))
        _same(_render(sc, attr=attr, splat=1, sl=slice(k, k + 1)), (index_map[k:k + 1], depth_map[k:k + 1], attr_map[k:k + 1], rcounts[k:k + 1]))


def test_mask_dtypes_agree_and_none_is_every_row():
    name = "n257_13x19_occ"
    sc = pir.built(name)
    image, attr = pir.image(name, 3), pir.attr(name, 3)
    casts = (lambda m: m, lambda m: m.to(torch.uint8), lambda m: m.long() * 7)
    outs = [_paint(sc, image, mask=c(sc["mask"])) for c in casts]
    routs = [_render(sc, attr=attr, splat=1, mask=c(sc["mask"])) for c in casts]
    for o, r in zip(outs[1:], routs[1:]):
        _same(o, outs[0])
        _same(r, routs[0])
    ones = torch.ones_like(sc["mask"])
    _same(_paint(sc, image, mask=None), _paint(sc, image, mask=ones))
    _same(_render(sc, attr=attr, mask=None), _render(sc, attr=attr, mask=ones))


def test_empty_sample_nan_pose_and_nan_fill():
    name = "n1025_13x19"
    sc = pir.built(name)
    B, _, N = sc["pts"].shape
    image, attr = pir.image(name, 3), pir.attr(name, 3)
    base, rbase = _paint(sc, image), _render(sc, attr=attr, splat=1, fill=math.nan)
    # fill = NaN appears in the ownerless pixels and nowhere else
    assert torch.equal(torch.isnan(rbase[2]), (rbase[0] < 0)[:, None].expand_as(rbase[2])) and bool((rbase[0] < 0).any()) and bool((rbase[0] >= 0).any())
    assert torch.equal(torch.isinf(rbase[1]), rbase[0] < 0)
    m = sc["mask"].clone()
    m[0] = False
    pose = sc["pose"].copy()
    pose[1] = math.nan
    colors, painted, counts, uv = _paint(sc, image, mask=m, pose=pose)
    index_map, depth_map, attr_map, rcounts = _render(sc, attr=attr, splat=1, fill=math.nan, mask=m, pose=pose)
    # sample 0 has no selected row, sample 1 a NaN pose: nothing painted, all-empty maps; sample 2 is as it was
    assert counts[0].tolist() == [0, 0] and counts[1].tolist() == [int(sc["mask"][1].sum()), 0] and not bool(painted[:2 * N].any())
    assert bool((colors[:2] == 0).all()) and bool(torch.isnan(uv[:2]).all())
    assert rcounts[0].tolist() == [0, 0, 0] and rcounts[1].tolist() == [int(sc["mask"][1].sum()), 0, 0]
    assert bool((index_map[:2] == -1).all()) and bool((torch.isinf(depth_map[:2]) & (depth_map[:2] > 0)).all()) and bool(torch.isnan(attr_map[:2]).all())
    _same((colors[2], painted[2 * N:], counts[2], uv[2]), (base[0][2], base[1][2 * N:], base[2][2], base[3][2]))
    _same((index_map[2], depth_map[2], attr_map[2], rcounts[2]), (rbase[0][2], rbase[1][2], rbase[2][2], rbase[3][2]))


def test_non_contiguous_and_off_device_tensors_are_refused():
    pts, pose, K, img = (t.to(DEV) for t in pir.hand_paint())
    N = pts.shape[2]
    attr = torch.zeros(1, 2, N, device=DEV)
    msg = "every tensor must be a contiguous tensor on the same GPU"
    pts_t = pts.permute(0, 2, 1).contiguous().permute(0, 2, 1)                    # [1, 3, N] over a transposed store
    img_t = img.transpose(2, 3).contiguous().transpose(2, 3)
    assert not pts_t.is_contiguous() and not img_t.is_contiguous()
    mask_t = torch.ones(N, 2, dtype=torch.bool, device=DEV)[:, :1].t()            # [1, N] with stride 2
    for kw in (dict(pts=pts_t), dict(image=img_t), dict(pose=pose.transpose(1, 2)), dict(K=K.expand(1, 3, 3).transpose(1, 2)), dict(mask=mask_t),
               dict(image=img.cpu()), dict(mask=torch.ones(1, N, dtype=torch.bool))):
        a = dict(pts=pts, pose=pose, K=K, image=img, mask=None)
        a.update(kw)
        with pytest.raises(ValueError, match="^paint_points: " + msg):
            ops.paint_points(a["pts"], a["pose"], a["K"], a["image"], mask=a["mask"])
    for kw in (dict(pts=pts_t), dict(attr=attr.permute(0, 2, 1).contiguous().permute(0, 2, 1)), dict(mask=mask_t), dict(attr=attr.cpu()), dict(pts=pts.cpu())):
        a = dict(pts=pts, attr=attr, mask=None)
        a.update(kw)
        with pytest.raises(ValueError, match="^render_points: " + msg):
            ops.render_points(a["pts"], pose, K, pir.HAND_H, pir.HAND_W, attr=a["attr"], mask=a["mask"])


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
    name = "n1025_13x19"
    sc = pir.built(name)
    pts, pose, K, mask = F(sc["pts"]), F(sc["pose"]), F(sc["K"]), sc["mask"].to(DEV)
    image, attr = pir.image(name, 5).to(DEV), pir.attr(name, 5).to(DEV)
    _replayed(lambda: ops.paint_points(pts, pose, K, image, mask=mask, want_uv=True))
    _replayed(lambda: ops.render_points(pts, pose, K, sc["h"], sc["w"], attr=attr, mask=mask, splat=2, fill=-1.0))


# ---- 6. the model layer and the scripts -------------------------------------------------------------------------------------------------------------
_GEO = {}


def _geo():
    """One gref.scene batch and its model, built once -> (scene, model)."""
    if not _GEO:
        from cmr_agent_amd.config import KittiConfiguration
        from cmr_agent_amd.models import MultiHeadModel
        _GEO["v"] = (gref.scene(B=2, N=1024, h=40, w=128, seed=201), MultiHeadModel(KittiConfiguration(num_pt=1024, device=torch.device(DEV))))
    return _GEO["v"]


def _data(sc):
    B, _, N = sc["pts"].shape
    g = torch.Generator().manual_seed(21)
    mask = torch.rand(B, N, generator=g) < 0.7
    return {"pc": F(sc["pts"]), "K": F(sc["K"]), "P": F(sc["P"]), "pnp_pose": F(sc["start"]), "img": torch.rand(B, 3, 160, 512, generator=g).to(DEV),
            "pc_geo_feat": sc["pc"].view(B, N, 64).permute(0, 2, 1).contiguous().to(DEV),
            "img_geo_feat": sc["img"].permute(0, 3, 1, 2).contiguous().to(DEV), "pc_overlap_pred": mask.to(DEV)}


def test_model_paint_points():
    sc, model = _geo()
    data = _data(sc)
    B, _, N = sc["pts"].shape
    model.paint_points(data)
    pc, pp, cnt = data["point_colors"], data["point_painted"], data["paint_counts"]
    assert pc.dtype == torch.float32 and tuple(pc.shape) == (B, 3, N) and pp.dtype == torch.bool and tuple(pp.shape) == (B, N) and tuple(cnt.shape) == (B, 2)
    K4 = data["K"].clone()
    K4[:, :2] *= 4.0                                                              # 160 / 40 = 512 / 128 = 4
    direct = ops.paint_points(data["pc"], data["pnp_pose"], K4, data["img"])
    assert torch.equal(_bits(pc), _bits(direct[0])) and torch.equal(pp.view(-1), direct[1]) and torch.equal(cnt, direct[2])
    assert cnt[:, 0].tolist() == [N] * B and 0 < int(cnt[:, 1].sum()) <= B * N
    # visible=True: ops.visibility on the geometric map with 4r's defaults, every row queried and occluding; only those are painted
    model.paint_points(data, visible=True)
    vis = ops.visibility(data["pc"], data["pnp_pose"], data["K"], 40, 128, torch.ones(B, N, dtype=torch.bool, device=DEV), radius=1, rel_tol=0.05)[0]
    direct = ops.paint_points(data["pc"], data["pnp_pose"], K4, data["img"], mask=vis)
    assert torch.equal(_bits(data["point_colors"]), _bits(direct[0])) and torch.equal(data["paint_counts"], direct[2])
    assert bool((data["point_painted"].view(-1) <= vis).all()) and int(data["paint_counts"][:, 1].sum()) <= int(cnt[:, 1].sum())
    # an explicit image and K at 1/4 scale is painting at the geometric map's resolution
    small = torch.rand(B, 5, 40, 128, generator=torch.Generator().manual_seed(22)).to(DEV)
    model.paint_points(data, pose=F(sc["P"]), image=small, K=data["K"], mask=data["pc_overlap_pred"], mode="nearest")
    direct = ops.paint_points(data["pc"], F(sc["P"]), data["K"], small, mask=data["pc_overlap_pred"], mode="nearest")
    assert tuple(data["point_colors"].shape) == (B, 5, N) and torch.equal(_bits(data["point_colors"]), _bits(direct[0]))
    assert torch.equal(data["paint_counts"], direct[2]) and data["paint_counts"][:, 0].tolist() == data["pc_overlap_pred"].sum(1).tolist()


def test_model_render_points():
    sc, model = _geo()
    data = _data(sc)
    B, _, N = sc["pts"].shape
    model.render_points(data)
    im, dm, cnt = data["index_map"], data["render_depth_map"], data["render_counts"]
    assert im.dtype == torch.int32 and tuple(im.shape) == (B, 40, 128) and tuple(dm.shape) == (B, 40, 128) and tuple(cnt.shape) == (B, 3) and "attr_map" not in data
    model.render_depth(data)                                                     # 4r's map, untouched, is the same z-buffer
    assert torch.equal(_bits(dm), _bits(data["depth_map"])) and torch.equal(im >= 0, torch.isfinite(dm))
    attr = data["pc_overlap_pred"].float()[:, None].contiguous()
    K4 = data["K"].clone()
    K4[:, :2] *= 4.0
    model.render_points(data, attr=attr, pose=F(sc["P"]), size=(160, 512), K=K4, mask=data["pc_overlap_pred"], splat=2, fill=-1.0)
    direct = ops.render_points(data["pc"], F(sc["P"]), K4, 160, 512, attr=attr, mask=data["pc_overlap_pred"], splat=2, fill=-1.0)
    _same((data["index_map"], data["render_depth_map"], data["attr_map"], data["render_counts"]), direct)
    am = data["attr_map"]
    assert tuple(am.shape) == (B, 1, 160, 512) and bool(((am == 1.0) | (am == -1.0)).all()) and torch.equal(am[:, 0] == 1.0, data["index_map"] >= 0)


def _run(script, *flags):
    cmd = [sys.executable, os.path.join(ROOT, script), "--pairs", "2", "--img", "160x512", "--num-pt", "4096", *flags]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return res.stdout.strip().splitlines()


def _check_script(script, flags, extra, tmp_path):
    plain = _run(script, *flags)
    assert not [l for l in plain if l.startswith("painted")]
    out = str(tmp_path / "clouds")
    lines = _run(script, *flags, "--paint", out, *extra)
    shown = [l.split() for l in lines if l.startswith("painted ")]
    print(script, extra, shown)
    assert len(shown) == 2 and all(len(t) == 4 and t[2] == "of" and 0 <= int(t[1]) <= int(t[3]) <= 4096 for t in shown), lines
    assert extra or all(int(t[3]) == 4096 for t in shown)                          # without --paint-visible every point is selected
    # the same seed: every other line is what the run prints without the flag, byte for byte
    assert [l for l in lines if not l.startswith("painted ")] == plain
    assert sorted(os.listdir(out)) == ["pair_0.ply", "pair_1.ply"]
    for i, t in enumerate(shown):
        raw = open(os.path.join(out, "pair_%d.ply" % i), "rb").read()
        head, payload = raw.split(b"end_header\n", 1)
        head = head.decode("ascii").split("\n")
        assert head[:2] == ["ply", "format binary_little_endian 1.0"] and head[2] == "element vertex %d" % int(t[1])
        assert [l.split()[1:] for l in head if l.startswith("property")] == [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"],
                                                                             ["uchar", "green"], ["uchar", "blue"]]
        v = np.frombuffer(payload, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
        assert len(v) == int(t[1]) and len(payload) == 15 * len(v) and np.isfinite(v["p"]).all() and (len(v) < 100 or len(np.unique(v["c"])) > 8)
        xyz, rgb = pir.read_ply(os.path.join(out, "pair_%d.ply" % i))
        assert np.array_equal(xyz, v["p"]) and np.array_equal(rgb, v["c"])


def test_test_geo_script_paint(tmp_path):
    _check_script("Test_Geo.py", ("--pnp", "--guided", "4,2", "--verify"), ("--paint-visible",), tmp_path)
    for argv in (("--paint", str(tmp_path / "x")), ("--pnp", "--paint-visible")):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "Test_Geo.py"), *argv], cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert res.returncode == 2 and "--paint" in res.stderr
    assert not os.path.exists(str(tmp_path / "x"))


def test_test_agent_script_paint(tmp_path):
    _check_script("Test_Agent.py", (), (), tmp_path)
