"""CPU tier of oriented-disc (surfel) rendering: the float64 restatement in surfel_reference.py gives the hand scenes (so the
yardstick of the GPU tests is itself checked), its float32 sibling agrees with it there, the scenes of the GPU tier keep their undecided
pixels under the cap, ops.render_surfels / ops.depth_test refuse malformed arguments before the library is touched, the C entries refuse
what is outside their contract, the model methods hand on what they should with ops stubbed -- and make the calls they made before when
the new keywords are off -- the loader's with_normals is opt-in, and the scripts reject misplaced flags."""
import argparse
import importlib
import math
import os
import random
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import cases as C
import surfel_reference as sr
import visibility_reference as vr
from cmr_agent_amd import _lib, ops
from cmr_agent_amd.utils import evalcli

mhm = importlib.import_module("cmr_agent_amd.models.MultiHeadModel")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf


# ---- the restatement on the hand scenes ------------------------------------------------------------------------------------------------------
def _hand(points, normals, radius=0.5, range_slope=0.0, max_px=8, min_cos=0.1, K=None):
    p, n, pose, Kt = (t.numpy().astype(np.float64) for t in sr.hand(points, normals))
    Kb = Kt if K is None else np.asarray([K], np.float64)
    r = sr.render(p, n, None, pose, Kb, sr.HAND_H, sr.HAND_W, radius, range_slope, max_px, min_cos)[0]
    # the float32 sibling from the chains of camera32: the same owners, and the same depths after rounding
    X, nc, rr = sr.camera32(p, n, pose, radius, range_slope)
    with np.errstate(all="ignore"):
        drawn = np.isfinite(n).all(1) & (X[:, 2] > 0) & np.isfinite(rr) & (rr > 0) & (X[:, 2] > rr) & bool(r["status"] == 0)
        uv = np.stack([Kb[:, 0, 0:1] * X[:, 0] / X[:, 2] + Kb[:, 0, 2:3], Kb[:, 1, 1:2] * X[:, 1] / X[:, 2] + Kb[:, 1, 2:3]], 1)
        drawn &= (np.rint(uv[:, 0]) + max_px >= 0) & (np.rint(uv[:, 0]) - max_px <= 16) & (np.rint(uv[:, 1]) + max_px >= 0) & (np.rint(uv[:, 1]) - max_px <= 16)
    s = np.concatenate([np.where(drawn[:, None], X, np.nan), np.where(drawn[:, None], nc, np.nan), np.where(drawn, rr, np.nan)[:, None],
                        drawn[:, None].astype(np.float32)], 1).astype(np.float32)
    idx32, depth32 = sr.restate32(s, uv, Kb, sr.HAND_H, sr.HAND_W, max_px, min_cos)
    assert np.array_equal(idx32[0], r["owner"]) and np.array_equal(depth32[0], r["depth"].astype(np.float32))
    return r


def _covered(r):
    return sorted((int(x), int(y)) for y, x in np.argwhere(r["owner"] >= 0))


def test_restatement_gives_the_hand_scenes():
    five = sorted([(8, 8), (7, 8), (9, 8), (8, 7), (8, 9)])
    for normal in ((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, -4.0)):
        r = _hand([(0.0, 0.0, 2.0)], [normal])
        assert _covered(r) == five and all(r["depth"][y, x] == 2.0 for x, y in five) and r["footprint"].tolist() == [5] and r["status"] == 0
        # the rim passes through four of the five centres: those pairs are marginal, the pixels undecided; the centre is decided
        assert r["decided"][8, 8] and r["owner_decided"][8, 8] == 0 and r["undecided"] == 4 and not r["decided"][8, 7]
    # tilted by 45 degrees about y, r = 1: narrower in x, and the depth is the plane's, 2 / (1 + dx)
    flat, tilt = _hand([(0.0, 0.0, 2.0)], [(0.0, 0.0, 1.0)], radius=1.0), _hand([(0.0, 0.0, 2.0)], [(1.0, 0.0, 1.0)], radius=1.0)
    assert np.nonzero(flat["owner"][8] >= 0)[0].tolist() == [6, 7, 8, 9, 10] and np.nonzero(tilt["owner"][8] >= 0)[0].tolist() == [7, 8, 9, 10]
    assert np.allclose(tilt["depth"][8, 7:11], [2 / 0.75, 2.0, 2 / 1.25, 2 / 1.5], rtol=1e-15) and np.nonzero(tilt["owner"][:, 8] >= 0)[0].tolist() == [6, 7, 8, 9, 10]
    # two points three cells apart: the discs meet
    assert _hand([(0.0, 0.0, 2.0), (1.5, 0.0, 2.0)], [(0.0, 0.0, 1.0)] * 2)["owner"][8, 7:13].tolist() == [0, 0, 0, 1, 1, 1]
    # a near disc (row 1) in front of a far one (row 0)
    r = _hand([(2.0, 0.0, 4.0), (0.0, 0.0, 1.0)], [(0.0, 0.0, 1.0)] * 2, radius=0.0, range_slope=0.5)
    assert r["owner"][8, 6:14].tolist() == [1, 1, 1, 1, 1, 0, 0, -1] and r["depth"][8, 6:14].tolist() == [1.0] * 5 + [4.0] * 2 + [INF]
    # equal depths go to the lower row -- and no evaluation but an exact one can tell: the pixels are undecided
    r = _hand([(0.25, 0.0, 2.0), (0.0, 0.0, 2.0), (0.0, 0.0, 2.0), (0.25, 0.0, 2.0)], [(0.0, 0.0, 1.0)] * 4)
    assert r["owner"][8, 7:10].tolist() == [1, 0, 0] and r["owner"][7, 8] == 1 and not r["decided"][8, 8]
    # the grazing cap
    assert _covered(_hand([(0.0, 0.0, 2.0)], [(1.0, 0.0, 0.046875)])) == []
    r = _hand([(0.0, 0.0, 2.0)], [(1.0, 0.0, 0.046875)], min_cos=0.03125)
    assert r["owner"][8, 8] == 0 and r["depth"][8, 8] == 2.0
    # rows that are not drawn: z_c = r, behind the camera, non-finite normals, z_c < r
    r = _hand([(0.0, 0.0, 0.5), (0.0, 0.0, -2.0), (0.0, 0.0, 2.0), (0.0, 0.0, 2.0), (0.0, 0.0, 0.25)],
              [(0.0, 0.0, 1.0), (0.0, 0.0, 1.0), (math.nan, 0.0, 1.0), (0.0, math.inf, 1.0), (0.0, 0.0, 1.0)])
    assert _covered(r) == [] and not r["drawn_sure"].any() and r["drawn_maybe"].tolist() == [True, False, False, False, False]
    # a K outside the camera model
    for bad in ([[4.0, 0.0, 8.0], [0.0, 4.0, 8.0], [0.0, 0.0, 2.0]], [[4.0, 0.0, 8.0], [0.5, 4.0, 8.0], [0.0, 0.0, 1.0]],
                [[4.0, 0.0, 8.0], [0.0, 4.0, 8.0], [0.0, 0.25, 1.0]], [[-4.0, 0.0, 8.0], [0.0, 4.0, 8.0], [0.0, 0.0, 1.0]]):
        r = _hand([(0.0, 0.0, 2.0)], [(0.0, 0.0, 1.0)], K=bad)
        assert r["status"] == 1 and _covered(r) == [] and r["undecided"] == 0
    # a centre outside the map whose disc reaches into it; at max_px = 0 its window does not touch the map
    r = _hand([(-4.5, 0.0, 2.0)], [(0.0, 0.0, 1.0)])
    assert _covered(r) == [(0, 8)] and r["depth"][8, 0] == 2.0
    assert _covered(_hand([(-4.5, 0.0, 2.0)], [(0.0, 0.0, 1.0)], max_px=0)) == []


def test_fma32_is_exact():
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=4000).astype(np.float32), rng.normal(size=4000).astype(np.float32)
    c = (-a.astype(np.float64) * b.astype(np.float64) * (1 + rng.normal(size=4000) * 1e-7)).astype(np.float32)      # heavy cancellation
    c[::7] = rng.normal(size=c[::7].size).astype(np.float32)
    got = sr.fma32(a, b, c)

    def exact(x, y, z):
        v = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.float32(float(v))                                                  # float(Fraction) rounds once to double: refine against the neighbours
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cands, key=lambda t: (abs(Fraction(float(t)) - v), int(np.float32(t).view(np.uint32)) & 1))
        return np.float32(best)

    want = np.array([exact(*t) for t in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


# ---- the cap on the scenes the GPU tier uses -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in vr.SCENES])
def test_undecided_pixels_stay_under_the_cap(name):
    sc = vr.built(name)
    pixels = sc["h"] * sc["w"]
    nrm = sr.normals_for(name)
    B, _, N = nrm.shape
    zero = (nrm == 0).all(1).mean()
    assert nrm.shape == sc["pts"].shape and (N < 100 or (0.05 < zero < 0.15 and (~np.isfinite(nrm)).any(1).sum() == 3 * B))
    for b, r in enumerate(sr.reference(name)):
        fp = r["footprint"][r["footprint"] > 0]
        print(name, "sample", b, "undecided", r["undecided"], "of", pixels, "sure drawn", r["counts_lo"], "maybe", int(r["drawn_maybe"].sum()),
              "footprint mean", float(fp.mean()) if fp.size else 0.0, "largest", int(fp.max()) if fp.size else 0, "largest bar", float(r["bar"].max()))
        assert r["undecided"] <= sr.cap(pixels) and r["status"] == 0
        assert float(r["bar"].max()) < 1e-2                                        # metres at depths of 2 .. 50: above that the derivation would be wrong


@pytest.mark.parametrize("k", range(len(sr.WINDOW_KS)))
def test_window_scenes_stay_under_the_cap_and_do_test_the_bound(k):
    pts, nrm, pose, Kb = sr.window_scene(k)
    ref = sr.render(pts, nrm, None, pose, Kb, sr.HAND_H, sr.HAND_W, sr.WINDOW_RADIUS, sr.WINDOW_SLOPE, sr.WINDOW_MAX_PX, 0.1)
    assert sum(r["undecided"] for r in ref) <= sr.WINDOW_B * sr.cap(sr.HAND_H * sr.HAND_W) and all(r["undecided"] <= sr.cap(17 * 17) for r in ref)
    # some exact footprint reaches more than a pixel beyond f r / z_c of its centre: a window of that half-extent would lose pixels
    X = pts[:, :, 0].astype(np.float64)
    r = sr.WINDOW_RADIUS + sr.WINDOW_SLOPE * X[:, 2]
    u = Kb[:, 0, 0] * X[:, 0] / X[:, 2] + Kb[:, 0, 1] * X[:, 1] / X[:, 2] + Kb[:, 0, 2]
    reach = np.array([np.abs(np.nonzero(q["owner"] >= 0)[1] - u[b]).max() if (q["owner"] >= 0).any() else 0.0 for b, q in enumerate(ref)])
    assert (reach > Kb[:, 0, 0] * r / X[:, 2] + 1.0).sum() >= (5 if k < 2 else 1)                 # under the long K the map itself cuts the reach


@pytest.mark.parametrize("name,m", sr.ZERO_CASES)
def test_zero_normal_cases_cover_their_windows_with_margin(name, m):
    sc = vr.built(name)
    for r in sr.render(sc["pts"], np.zeros_like(sc["pts"]), sc["mask"], sc["pose"], sc["K"], sc["h"], sc["w"], 0.0, sr.ZERO_SLOPE, m, sr.MIN_COS):
        assert r["full"][r["drawn_sure"] | r["drawn_maybe"]].all()


# ---- ops refuse before the library is touched --------------------------------------------------------------------------------------------------
def _touched(*a, **kw):
    raise AssertionError("the library was touched")


def test_constants_and_prototypes():
    assert ops.SURFEL_MAX_PX == 16
    src = open(os.path.join(ROOT, "cmr_agent_amd", "csrc", "surfel.hip")).read()
    for text in ("max_px <= CMR_MAX_RADIUS", "cmr_attr_ok(attr, attr_map, C)", "cmr_render_surfels_f32", "cmr_depth_test_f32", "fp contract(off)"):
        assert text in src
    csrc = os.path.join(ROOT, "cmr_agent_amd", "csrc")
    assert "constexpr int CMR_MAX_RADIUS = 16;" in open(os.path.join(csrc, "cmr_project.h")).read()      # the limits' one definition
    assert "constexpr int CMR_MAX_PLANES = 64;" in open(os.path.join(csrc, "cmr_project.h")).read()
    assert "C <= CMR_MAX_PLANES" in open(os.path.join(csrc, "cmr_zbuffer.h")).read() and ops.POINT_IMAGE_MAX_C == 64
    assert "atomicAdd(float" not in src and "atomicAdd((float" not in src
    for fn in (ops.render_surfels, ops.depth_test):
        assert "not tuned on real data" in " ".join(fn.__doc__.split())
    protos = _lib.parse_header()
    assert protos["cmr_render_surfels_f32"][2] == ["pts", "normals", "mask", "mask_bytes", "pose", "K", "attr", "C", "B", "N", "h", "w", "radius",
                                                   "range_slope", "max_px", "min_cos", "fill", "index_map", "depth_map", "normal_map", "attr_map",
                                                   "counts", "surfel", "workspace", "workspace_bytes", "stream"]
    assert protos["cmr_depth_test_f32"][2] == ["pts", "mask", "mask_bytes", "pose", "K", "Z", "B", "N", "h", "w", "radius", "rel_tol", "abs_tol",
                                               "visible", "counts", "stream"]
    assert protos["cmr_render_surfels_workspace_bytes"][2] == ["B", "h", "w"] and "cmr_depth_test_workspace_bytes" not in protos
    from cmr_agent_amd.utils import workmodel
    assert "cmr_render_surfels_f32" in open(workmodel.__file__).read() and "cmr_depth_test_f32" in open(workmodel.__file__).read()


def test_render_surfels_argument_checks(monkeypatch):
    monkeypatch.setattr(_lib, "load", _touched)
    monkeypatch.setattr(_lib, "call", _touched)
    B, N, h, w = 2, 6, 4, 5
    base = dict(pts=torch.zeros(B, 3, N), normals=torch.zeros(B, 3, N), pose=torch.eye(4).repeat(B, 1, 1), K=torch.eye(3).repeat(B, 1, 1), h=h, w=w)

    def refused(match, **kw):
        args = {**base, **kw}
        with pytest.raises(ValueError, match="^render_surfels: " + match):
            ops.render_surfels(args.pop("pts"), args.pop("normals"), args.pop("pose"), args.pop("K"), args.pop("h"), args.pop("w"), **args)

    refused("pts must be", pts=torch.zeros(B, 4, N))
    refused("pts must be", pts=None)
    refused("pts, pose and K must be float32", pts=torch.zeros(B, 3, N).double())
    refused("pose must be", pose=torch.eye(4))
    refused("K must be", K=torch.eye(3))
    refused("h and w must be integers", h=4.5)
    refused("need 1 <= B", h=4097, w=4096)
    refused("need 1 <= B", h=0)
    for normals in (None, torch.zeros(B, 3, N + 1), torch.zeros(B, 3, N).double(), torch.zeros(B, N, 3), [0.0]):
        refused("normals must be", normals=normals)
    for mask in (torch.ones(B, N), torch.ones(B, N + 1, dtype=torch.bool), "m"):
        refused("mask must be", mask=mask)
    for attr in (torch.zeros(B, N), torch.zeros(B, 2, N).half(), torch.zeros(B + 1, 2, N), torch.zeros(B, 65, N), torch.zeros(B, 0, N), "a"):
        refused("attr must be", attr=attr)
    for v in (-0.1, math.nan, math.inf, "x", None, True, 1e39):
        refused("radius must be", radius=v)
        refused("range_slope must be", range_slope=v)
        refused("min_cos must be", min_cos=v)
    refused("min_cos must be", min_cos=1.5)
    for v in (-1, 17, 1.5, math.nan, True, "2", None):
        refused("max_px must be", max_px=v)
    for v in ("x", None, [0.0]):
        refused("fill must be", fill=v)
    msg = "every tensor must be a contiguous tensor on the same GPU"
    refused(msg)
    refused(msg, attr=torch.zeros(B, 64, N), mask=torch.ones(B * N, dtype=torch.int64), radius=0, range_slope=0, max_px=16, min_cos=1, fill=math.nan,
            want_normal_map=True, want_surfel=True)


def test_depth_test_argument_checks(monkeypatch):
    monkeypatch.setattr(_lib, "load", _touched)
    monkeypatch.setattr(_lib, "call", _touched)
    B, N, h, w = 2, 6, 4, 5
    base = dict(pts=torch.zeros(B, 3, N), pose=torch.eye(4).repeat(B, 1, 1), K=torch.eye(3).repeat(B, 1, 1), depth_map=torch.ones(B, h, w),
                mask=torch.ones(B, N, dtype=torch.bool))

    def refused(match, **kw):
        args = {**base, **kw}
        with pytest.raises(ValueError, match="^depth_test: " + match):
            ops.depth_test(args.pop("pts"), args.pop("pose"), args.pop("K"), args.pop("depth_map"), args.pop("mask"), **args)

    for dm in (None, torch.ones(h, w), torch.ones(B, 1, h, w), torch.ones(B, h, w).double(), torch.ones(B + 1, h, w), [1.0]):
        refused("depth_map must be", depth_map=dm)
    refused("need 1 <= B", depth_map=torch.ones(B, 0, w))
    refused("pts must be", pts=torch.zeros(B, N, 3))
    refused("pose must be", pose=torch.eye(4).repeat(B + 1, 1, 1))
    refused("K must be", K=torch.eye(3))
    for mask in (None, torch.ones(B, N), torch.ones(B, N - 1, dtype=torch.uint8)):
        refused("mask must be", mask=mask)
    for v in (-1, 17, 0.5, math.nan, True, None):
        refused("radius must be", radius=v)
    for v in (-1e-3, math.nan, math.inf, "t", None, 1e39):
        refused("rel_tol must be", rel_tol=v)
        refused("abs_tol must be", abs_tol=v)
    refused("every tensor must be a contiguous tensor on the same GPU")
    refused("every tensor must be a contiguous tensor on the same GPU", radius=16, rel_tol=0, abs_tol=2.5, mask=torch.ones(B * N, dtype=torch.int64))


def test_c_entries_refuse_what_is_outside_the_contract():
    """CMR_EINVAL up front: every check sits ahead of the first launch, so this runs without a GPU (the pointers are never followed)."""
    lib = _lib.load()
    p = torch.zeros(64).data_ptr()
    assert p % 16 == 0
    names = _lib.parse_header()["cmr_render_surfels_f32"][2]
    base = dict(pts=p, normals=p, mask=None, mask_bytes=1, pose=p, K=p, attr=None, C=0, B=1, N=2, h=2, w=2, radius=0.1, range_slope=0.004, max_px=8,
                min_cos=0.1, fill=0.0, index_map=p, depth_map=p, normal_map=None, attr_map=None, counts=p, surfel=None, workspace=p,
                workspace_bytes=lib.cmr_render_surfels_workspace_bytes(1, 2, 2), stream=None)
    call = lambda **kw: lib.cmr_render_surfels_f32(*[{**base, **kw}[k] for k in names])
    for bad in (dict(pts=None), dict(normals=None), dict(pose=None), dict(K=None), dict(index_map=None), dict(depth_map=None), dict(counts=None),
                dict(workspace=None), dict(workspace=p + 8), dict(workspace_bytes=16), dict(B=0), dict(B=65536), dict(N=0), dict(h=0), dict(w=-1),
                dict(h=4097, w=4096), dict(mask_bytes=4), dict(mask_bytes=0), dict(max_px=-1), dict(max_px=17), dict(radius=-0.1),
                dict(radius=math.nan), dict(radius=math.inf), dict(range_slope=-1.0), dict(range_slope=math.nan), dict(range_slope=math.inf),
                dict(min_cos=-0.1), dict(min_cos=1.5), dict(min_cos=math.nan), dict(attr=p), dict(attr_map=p), dict(attr=p, attr_map=p, C=0),
                dict(attr=p, attr_map=p, C=65), dict(C=1)):
        assert call(**bad) == -1, bad
    assert lib.cmr_render_surfels_workspace_bytes(2, 3, 5) == 240 and lib.cmr_render_surfels_workspace_bytes(1, 1, 1) == 16
    for bad in ((0, 3, 5), (2, 0, 5), (2, 3, -1)):
        assert lib.cmr_render_surfels_workspace_bytes(*bad) == 0
    names = _lib.parse_header()["cmr_depth_test_f32"][2]
    base = dict(pts=p, mask=p, mask_bytes=1, pose=p, K=p, Z=p, B=1, N=2, h=2, w=2, radius=0, rel_tol=0.05, abs_tol=0.0, visible=p, counts=p, stream=None)
    call = lambda **kw: lib.cmr_depth_test_f32(*[{**base, **kw}[k] for k in names])
    for bad in (dict(pts=None), dict(mask=None), dict(pose=None), dict(K=None), dict(Z=None), dict(Z=p + 2), dict(visible=None), dict(counts=None),
                dict(B=0), dict(N=0), dict(h=0), dict(w=0), dict(h=4097, w=4096), dict(mask_bytes=2), dict(radius=-1), dict(radius=17),
                dict(rel_tol=-0.1), dict(rel_tol=math.nan), dict(rel_tol=math.inf), dict(abs_tol=-1.0), dict(abs_tol=math.nan), dict(abs_tol=math.inf)):
        assert call(**bad) == -1, bad


# ---- the model layer with ops stubbed ------------------------------------------------------------------------------------------------------------
class _FakeOps:
    """Stands in for cmr_agent_amd.ops inside MultiHeadModel: CPU tensors of the right shapes, and a log of the calls."""
    _is_int = staticmethod(ops._is_int)

    def __init__(self):
        self.log = []

    def visibility(self, pts, pose, K, h, w, mask, **kw):
        B, _, N = pts.shape
        self.log.append(("visibility", pose.clone(), K.clone(), (h, w), mask, kw))
        vis = (mask.reshape(-1) != 0) & (torch.arange(B * N) % 2 == 0)
        return vis, torch.zeros(B, 4, dtype=torch.int32), None, None, None

    def point_normals(self, points, radius=0.6, **kw):
        self.log.append(("point_normals", points.clone(), radius, kw))
        return (points * 2.0, None, None)

    def render_surfels(self, pts, normals, pose, K, h, w, **kw):
        B = pts.shape[0]
        self.log.append(("render_surfels", normals.clone(), pose.clone(), K.clone(), (h, w), kw))
        attr = kw.get("attr")
        return (torch.zeros(B, h, w, dtype=torch.int32), torch.full((B, h, w), 9.0), None if attr is None else torch.full((B, attr.shape[1], h, w), 3.0),
                torch.full((B, 4), 2, dtype=torch.int32), torch.ones(B, 3, h, w) if kw.get("want_normal_map") else None, None)

    def depth_test(self, pts, pose, K, depth_map, mask, **kw):
        B, _, N = pts.shape
        self.log.append(("depth_test", pose.clone(), K.clone(), depth_map, mask, kw))
        vis = (mask.reshape(-1) != 0) & (torch.arange(B * N) % 3 == 0)
        return vis, torch.ones(B, 3, dtype=torch.int32)

    def render_points(self, pts, pose, K, h, w, attr=None, mask=None, splat=0, fill=0.0):
        B = pts.shape[0]
        self.log.append(("render_points", pose.clone(), K.clone(), (h, w), attr, mask, splat, fill))
        return (torch.zeros(B, h, w, dtype=torch.int32), torch.full((B, h, w), 7.0), None if attr is None else torch.full((B, attr.shape[1], h, w), 3.0),
                torch.zeros(B, 3, dtype=torch.int32))

    def densify(self, depth, guide=None, attr=None, **kw):
        self.log.append(("densify", depth, guide, attr, kw))
        B, h, w = depth.shape
        return depth + 1.0, None if attr is None else attr + 1.0, torch.ones(B, h, w), None, torch.full((B, 3), 5, dtype=torch.int32)

    def guided_match(self, pts, feat, img, mask, pose, K, radius, **kw):
        B, _, N = pts.shape
        self.log.append(("guided_match", pose.clone(), radius, mask))
        return torch.zeros(B * N, dtype=torch.int32), torch.ones(B * N, dtype=torch.bool), torch.zeros(B, 4, dtype=torch.int32), None, None

    def pnp_refine(self, pts, uv, use, K, pose, thr=1.0, iters=10):
        B = pts.shape[0]
        self.log.append(("pnp_refine", pose.clone()))
        nxt = pose.clone()
        nxt[:, 0, 3] += 1.0
        return nxt, torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)

    def pose_score(self, pts, feat, img, mask, poses, K, radius=0, tau=0.8):
        B, P = poses.shape[:2]
        self.log.append(("pose_score", mask, radius))
        score = torch.ones(B, P, dtype=torch.float64)
        score[:, 1] = 0.5
        return score, torch.zeros(B, P, 2, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)

    def paint_points(self, pts, pose, K, image, mask=None, mode='bilinear', want_uv=False):
        B, _, N = pts.shape
        self.log.append(("paint_points", mask))
        return torch.zeros(B, image.shape[1], N), torch.ones(B * N, dtype=torch.bool), torch.zeros(B, 2, dtype=torch.int32), None


def _batch(B=2, N=6, h=4, w=5, planes=3):
    g = torch.Generator().manual_seed(5)
    K = torch.tensor([[50.0, 0.0, 2.0], [0.0, 60.0, 1.5], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    return {"pc": torch.randn(B, 3, N, generator=g), "K": K, "pc_geo_feat": torch.randn(B, 64, N, generator=g),
            "img_geo_feat": torch.randn(B, 64, h, w, generator=g), "pc_overlap_pred": torch.ones(B, N, dtype=torch.int64),
            "pnp_pose": torch.eye(4).repeat(B, 1, 1), "img": torch.rand(B, planes, 4 * h, 8 * w, generator=g)}


DEFAULTS = dict(radius=0.1, range_slope=0.004, max_px=8, min_cos=0.1)


def _model(monkeypatch):
    fake = _FakeOps()
    monkeypatch.setattr(mhm, "ops", fake)
    return fake, mhm.MultiHeadModel.__new__(mhm.MultiHeadModel)                   # the methods under test use no weights


def test_model_point_normals_and_render_surfels(monkeypatch):
    fake, model = _model(monkeypatch)
    assert mhm.SURFEL_DEFAULTS == DEFAULTS
    data = _batch()
    mhm.MultiHeadModel.point_normals(model, data, radius=0.4)
    assert [c[0] for c in fake.log] == ["point_normals"] * 2 and all(c[2] == 0.4 for c in fake.log)           # one call per sample
    assert all(torch.equal(c[1], data["pc"][b].t()) and c[1].is_contiguous() for b, c in enumerate(fake.log))
    assert tuple(data["pc_normal"].shape) == (2, 3, 6) and torch.equal(data["pc_normal"], data["pc"] * 2.0) and data["pc_normal"].is_contiguous()
    # render_surfels: 'pc_normal' is used when present ...
    fake.log.clear()
    data["pc_normal"] = torch.full((2, 3, 6), 5.0)
    mhm.MultiHeadModel.render_surfels(model, data)
    (ren,) = fake.log
    assert ren[0] == "render_surfels" and bool((ren[1] == 5.0).all()) and torch.equal(ren[2], data["pnp_pose"]) and torch.equal(ren[3], data["K"])
    assert ren[4] == (4, 5) and ren[5] == dict(DEFAULTS, attr=None, mask=None, fill=0.0, want_normal_map=True)
    assert tuple(data["surfel_index_map"].shape) == (2, 4, 5) and bool((data["surfel_depth_map"] == 9.0).all())
    assert tuple(data["surfel_normal_map"].shape) == (2, 3, 4, 5) and data["surfel_counts"].tolist() == [[2] * 4] * 2 and "surfel_attr_map" not in data
    # ... and computed when absent; everything explicit
    fake.log.clear()
    data = _batch()
    pose, a, m = torch.eye(4).repeat(2, 1, 1) * 2.0, torch.rand(2, 2, 6), torch.tensor([[1, 0, 1, 0, 1, 0]] * 2, dtype=torch.uint8)
    mhm.MultiHeadModel.render_surfels(model, data, attr=a, pose=pose, size=(8, 10), K=torch.eye(3) * 3.0, mask=m, radius=0.3, range_slope=0.01, max_px=4,
                                      min_cos=0.2, fill=math.nan)
    assert [c[0] for c in fake.log] == ["point_normals", "point_normals", "render_surfels"] and fake.log[0][2] == 0.6
    ren = fake.log[2]
    assert torch.equal(ren[1], data["pc"] * 2.0) and torch.equal(ren[2], pose) and torch.equal(ren[3], (torch.eye(3) * 3.0).repeat(2, 1, 1)) and ren[4] == (8, 10)
    kw = dict(ren[5])
    assert math.isnan(kw.pop("fill")) and torch.equal(kw.pop("attr"), a) and torch.equal(kw.pop("mask"), m)
    assert kw == dict(radius=0.3, range_slope=0.01, max_px=4, min_cos=0.2, want_normal_map=True)
    assert tuple(data["surfel_attr_map"].shape) == (2, 2, 8, 10) and "pc_normal" in data
    fake.log.clear()
    nrm = torch.full((2, 3, 6), 7.0)
    mhm.MultiHeadModel.render_surfels(model, _batch(), normals=nrm)               # given normals: nothing is computed
    assert [c[0] for c in fake.log] == ["render_surfels"] and torch.equal(fake.log[0][1], nrm)
    for kw in (dict(size=(8, 10)), dict(K=torch.eye(3))):
        with pytest.raises(ValueError, match="render_surfels: size and K go together"):
            mhm.MultiHeadModel.render_surfels(model, _batch(), **kw)


def test_model_dense_depth_with_surfels(monkeypatch):
    fake, model = _model(monkeypatch)
    K_full = torch.tensor([[400.0, 0.0, 16.0], [0.0, 240.0, 6.0], [0.0, 0.0, 1.0]])
    # off: the calls and their arguments are what they were
    for off in ({}, dict(surfels=None), dict(surfels=False)):
        fake.log.clear()
        data = _batch()
        mhm.MultiHeadModel.dense_depth(model, data, **off)
        ren, den = fake.log
        assert ren[0] == "render_points" and torch.equal(ren[1], data["pnp_pose"]) and torch.equal(ren[2][1], K_full) and ren[3] == (16, 40)
        assert ren[4] is None and ren[5] is None and ren[6] == 0 and ren[7] == 0.0 and den[0] == "densify" and bool((den[1] == 7.0).all())
        assert "surfel_counts" not in data and "pc_normal" not in data
    for surfels, want in ((True, DEFAULTS), (dict(radius=0.25, max_px=3), dict(DEFAULTS, radius=0.25, max_px=3))):
        fake.log.clear()
        data = _batch()
        a, m = torch.rand(2, 2, 6), torch.tensor([[1, 0, 1, 0, 1, 0]] * 2, dtype=torch.uint8)
        mhm.MultiHeadModel.dense_depth(model, data, attr=a, mask=m, fill=2.0, splat=2, surfels=surfels)
        assert [c[0] for c in fake.log] == ["point_normals", "point_normals", "render_surfels", "densify"]
        ren, den = fake.log[2], fake.log[3]
        assert torch.equal(ren[1], data["pc"] * 2.0) and torch.equal(ren[2], data["pnp_pose"]) and torch.equal(ren[3][0], K_full) and ren[4] == (16, 40)
        kw = dict(ren[5])
        assert torch.equal(kw.pop("attr"), a) and torch.equal(kw.pop("mask"), m) and kw == dict(want, fill=2.0)
        assert bool((den[1] == 9.0).all()) and bool((den[3] == 3.0).all()) and den[4]["fill"] == 2.0        # the surfel maps go to densify
        assert data["surfel_counts"].tolist() == [[2] * 4] * 2 and bool((data["dense_depth_map"] == 10.0).all())
    # with visible as well: the z-buffer first, then the discs of the visible rows
    fake.log.clear()
    mhm.MultiHeadModel.dense_depth(model, _batch(), visible=True, surfels=True)
    assert [c[0] for c in fake.log] == ["visibility", "point_normals", "point_normals", "render_surfels", "densify"]
    assert fake.log[3][5]["mask"].dtype == torch.bool
    for bad in (3, "yes", dict(tau=1.0), dict(splat=1)):
        with pytest.raises(ValueError, match="dense_depth: surfels must be"):
            mhm.MultiHeadModel.dense_depth(model, _batch(), surfels=bad)


def test_visible_keyword_with_surfels(monkeypatch):
    fake, model = _model(monkeypatch)
    # refine: per round the surfel map of the whole cloud on the geometric map under that round's pose, then the depth test of `mask`
    data = _batch()
    mhm.MultiHeadModel.refine_pose_from_matches(model, data, radii=(3, 1), thrs=(2.0, 1.0), visible=dict(surfels=True, abs_tol=0.5))
    assert [c[0] for c in fake.log] == ["point_normals", "point_normals", "render_surfels", "depth_test", "guided_match", "pnp_refine",
                                        "render_surfels", "depth_test", "guided_match", "pnp_refine"]
    for k, shift in ((2, 0.0), (6, 1.0)):
        ren, dt, gm = fake.log[k], fake.log[k + 1], fake.log[k + 2]
        assert float(ren[2][0, 0, 3]) == shift and torch.equal(ren[2], dt[1]) and torch.equal(ren[2], gm[1]) and ren[4] == (4, 5)
        assert torch.equal(ren[3], data["K"]) and ren[5] == DEFAULTS                                          # the whole cloud: no mask
        assert bool((dt[3] == 9.0).all()) and torch.equal(dt[4], data["pc_overlap_pred"]) and dt[5] == dict(radius=0, rel_tol=0.05, abs_tol=0.5)
        assert gm[3].dtype == torch.bool and gm[3].view(-1).tolist() == [i % 3 == 0 for i in range(12)]
    assert tuple(data["refine_visible_counts"].shape) == (2, 2, 3)
    # a dict of parameters and an explicit window radius
    fake.log.clear()
    mhm.MultiHeadModel.refine_pose_from_matches(model, _batch(), radii=(3,), thrs=(2.0,), visible=dict(surfels=dict(radius=0.3), radius=2))
    assert fake.log[2][5] == dict(DEFAULTS, radius=0.3) and fake.log[3][5] == dict(radius=2, rel_tol=0.05, abs_tol=0.0)
    # surfels off inside the dict: ops.visibility, as before
    for off in (dict(radius=2), dict(radius=2, surfels=None), dict(radius=2, surfels=False)):
        fake.log.clear()
        mhm.MultiHeadModel.refine_pose_from_matches(model, _batch(), radii=(3,), thrs=(2.0,), visible=off)
        assert [c[0] for c in fake.log] == ["visibility", "guided_match", "pnp_refine"] and fake.log[0][5] == dict(radius=2, rel_tol=0.05, abs_tol=0.0)
    # search_pose: once per level
    fake.log.clear()
    data = _batch()
    mhm.MultiHeadModel.search_pose(model, data, levels=((2, 1.0, 0.1, 2), (0, 0.5, 0.05, 1)), visible=dict(surfels=True))
    assert [c[0] for c in fake.log] == ["point_normals", "point_normals", "render_surfels", "depth_test", "pose_score", "pose_score", "render_surfels",
                                        "depth_test", "pose_score"]
    assert tuple(data["search_visible_counts"].shape) == (2, 2, 3) and all(c[1].dtype == torch.bool for c in fake.log if c[0] == "pose_score")
    # paint_points and dense_depth
    fake.log.clear()
    data = _batch()
    data["pc_normal"] = torch.ones(2, 3, 6)
    mhm.MultiHeadModel.paint_points(model, data, visible=dict(surfels=True))
    assert [c[0] for c in fake.log] == ["render_surfels", "depth_test", "paint_points"] and fake.log[0][4] == (4, 5) and torch.equal(fake.log[0][3], data["K"])
    assert fake.log[2][1].view(-1).tolist() == [i % 3 == 0 for i in range(12)] and bool(fake.log[1][4].all())
    fake.log.clear()
    mhm.MultiHeadModel.dense_depth(model, data, visible=dict(surfels=True))
    assert [c[0] for c in fake.log] == ["render_surfels", "depth_test", "render_points", "densify"]
    assert fake.log[0][4] == (4, 5) and fake.log[2][3] == (16, 40) and fake.log[2][5].view(-1).tolist() == [i % 3 == 0 for i in range(12)]
    # visible_points
    fake.log.clear()
    mhm.MultiHeadModel.visible_points(model, data, radius=0, occluders="surfels", surfels=dict(radius=0.35))
    assert [c[0] for c in fake.log] == ["render_surfels", "depth_test"] and fake.log[0][5] == dict(DEFAULTS, radius=0.35)
    assert fake.log[1][5] == dict(radius=0, rel_tol=0.05, abs_tol=0.0) and tuple(data["visible_mask"].shape) == (2, 6)
    assert data["visible_counts"].tolist() == [[1, 1, 1]] * 2
    fake.log.clear()
    mhm.MultiHeadModel.visible_points(model, data, occluders="surfels")
    assert fake.log[0][5] == DEFAULTS and fake.log[1][5]["radius"] == 1
    fake.log.clear()
    mhm.MultiHeadModel.visible_points(model, data)                                # the path that existed
    assert [c[0] for c in fake.log] == ["visibility"] and fake.log[0][5] == dict(occ_mask=None, radius=1, rel_tol=0.05, abs_tol=0.0)
    with pytest.raises(ValueError, match="visible_points: surfels belongs to"):
        mhm.MultiHeadModel.visible_points(model, data, surfels=True)
    with pytest.raises(ValueError, match="visible_points: occluders must be"):
        mhm.MultiHeadModel.visible_points(model, data, occluders="discs")
    for bad in (dict(surfels=3), dict(surfels=dict(tau=1.0)), dict(discs=True)):
        with pytest.raises(ValueError, match="refine_pose_from_matches: (visible|surfels) must be"):
            mhm.MultiHeadModel.refine_pose_from_matches(model, _batch(), visible=bad)


# ---- the loader keyword ----------------------------------------------------------------------------------------------------------------------------
def _write_dataset(root, rows):
    """One frame of one sequence in the reference's on-disk layout (tests/test_loader.py's helper, cut down), the cloud with `rows` rows."""
    f = C.FRAME
    fmt = lambda name, v: name + ": " + " ".join("%.12e" % x for x in v) + "\n"      # noqa: E731
    os.makedirs(os.path.join(root, "calib", "09"), exist_ok=True)
    with open(os.path.join(root, "calib", "09", "calib.txt"), "w") as fh:
        fh.write("".join(fmt(k, C.FRAME_P2) for k in ("P0", "P1", "P2", "P3")) + fmt("Tr", C.FRAME_TR))
    os.makedirs(os.path.join(root, "data_odometry_color_npy", "sequences", "09", "image_2"), exist_ok=True)
    os.makedirs(os.path.join(root, "data_odometry_velodyne_NWU", "sequences", "09", "voxel0.1-SNr0.6"), exist_ok=True)
    raw = C.frame_raw_cloud()
    rng = np.random.RandomState(3)
    nrm = rng.normal(size=(3, raw.shape[1])).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=0, keepdims=True)
    cloud = np.concatenate([raw, nrm])[:rows]
    np.save(os.path.join(root, "data_odometry_velodyne_NWU", "sequences", "09", "voxel0.1-SNr0.6", "000000.npy"), cloud)
    np.save(os.path.join(root, "data_odometry_color_npy", "sequences", "09", "image_2", "000000.npy"),
            rng.randint(0, 256, size=(f["img_h"], f["img_w"], 3)).astype(np.uint8))
    return cloud


def test_with_normals_is_opt_in(tmp_path, monkeypatch):
    """The host half only: preprocess_frame (HIP kernels) is replaced by a stand-in, so the key set and the turned normals are checked
    without a GPU."""
    from cmr_agent_amd.config import KittiConfiguration
    from cmr_agent_amd.dataset import loader
    root = str(tmp_path / "seven")
    cloud = _write_dataset(root, 7)
    f = C.FRAME
    cfg = KittiConfiguration(cropped_img_H=f["H"], cropped_img_W=f["W"], num_pt=f["num_pt"], device="cpu")
    cfg.num_node = f["num_node"]
    seen = {}

    def fake_preprocess(raw, P_Tr, K, P_random, hw4, choice=None, **kw):
        seen.update(P_Tr=np.asarray(P_Tr, np.float64), P_random=np.asarray(P_random, np.float64))
        return {"pc": raw[:3][:, choice], "in_picture_count": torch.tensor(0)}

    monkeypatch.setattr(loader, "preprocess_frame", fake_preprocess)
    keys = []
    for flag in (None, False, True):
        ds = loader.FrameDataset(root, cfg, "val", device="cpu", **({} if flag is None else dict(with_normals=flag)))
        random.seed(4)
        np.random.seed(4)
        s = ds[0]
        keys.append(set(s))
        if flag:
            n = s["pc_normal"]
            assert n.dtype == torch.float32 and tuple(n.shape) == (3, f["num_pt"]) and n.is_contiguous()
            R = seen["P_random"][:3, :3] @ seen["P_Tr"][:3, :3]
            want = R.astype(np.float32) @ cloud[4:7, ds.last_draws["choice"]]
            assert np.allclose(n.numpy(), want, rtol=0, atol=1e-6) and np.allclose(np.linalg.norm(n.numpy(), axis=0), 1.0, atol=1e-5)
            assert abs(np.linalg.det(R) - 1.0) < 1e-6                              # both factors are rigid
    assert keys[0] == keys[1] and "pc_normal" not in keys[0] and keys[2] == keys[0] | {"pc_normal"}
    # a file without the normal rows: a ValueError naming the frame -- only when asked for
    root4 = str(tmp_path / "four")
    _write_dataset(root4, 4)
    assert "pc_normal" not in loader.FrameDataset(root4, cfg, "val", device="cpu")[0]
    with pytest.raises(ValueError, match="frame 0: with_normals needs"):
        loader.FrameDataset(root4, cfg, "val", device="cpu", with_normals=True)[0]


# ---- the command-line flags --------------------------------------------------------------------------------------------------------------------------
def test_surfel_flags():
    def parse(*argv):
        ap = argparse.ArgumentParser()
        evalcli.add_visible_flags(ap, "--guided")
        evalcli.add_dense_flags(ap)
        evalcli.add_surfel_flags(ap)
        args = ap.parse_args(list(argv))
        dense = evalcli.dense_option(ap, args, ops.DENSIFY_MAX_RADIUS)
        visible = evalcli.visible_option(ap, args, "--guided", True, ops.GUIDED_MAX_RADIUS)
        return evalcli.surfel_option(ap, args, dense, visible, ops.SURFEL_MAX_PX)

    assert parse() == (None, None)
    assert parse("--dense-depth", "out", "--visible") == (("out", 8, 0.1, False), {})                       # the options as they were
    assert parse("--dense-depth", "out", "--dense-surfels") == (("out", 8, 0.1, False, True), None)
    assert parse("--visible", "--visible-surfels", "--visible-radius", "2") == (None, dict(radius=2, surfels=True))
    got = parse("--dense-depth", "out", "--dense-surfels", "--visible", "--visible-surfels", "--surfel-radius", "0.2", "--surfel-slope", "0.01",
                "--surfel-max-px", "4")
    sf = dict(radius=0.2, range_slope=0.01, max_px=4)
    assert got == (("out", 8, 0.1, False, sf), dict(surfels=sf))
    assert parse("--dense-depth", "out", "--visible", "--visible-surfels", "--surfel-max-px", "0") == (("out", 8, 0.1, False), dict(surfels=dict(max_px=0)))
    for argv in (("--dense-surfels",), ("--visible-surfels",), ("--visible", "--dense-surfels"), ("--dense-depth", "out", "--visible-surfels"),
                 ("--surfel-radius", "0.2"), ("--dense-depth", "out", "--surfel-slope", "0.01"), ("--visible", "--surfel-max-px", "4"),
                 ("--visible", "--visible-surfels", "--surfel-max-px", "17"), ("--visible", "--visible-surfels", "--surfel-max-px", "-1"),
                 ("--visible", "--visible-surfels", "--surfel-radius", "-0.1"), ("--visible", "--visible-surfels", "--surfel-radius", "nan"),
                 ("--dense-depth", "out", "--dense-surfels", "--surfel-slope", "inf")):
        with pytest.raises(SystemExit):
            parse(*argv)


def test_dense_pairs_with_surfels_prints_one_more_line(tmp_path, capsys):
    class Model:
        def dense_depth(self, data, pose=None, radius=None, sigma_r=None, visible=None, **kw):
            self.seen = (pose, radius, sigma_r, visible, kw)
            data["dense_depth_map"] = torch.ones(2, 2, 3)
            data["dense_counts"] = torch.tensor([[2, 6, 5], [3, 6, 6]], dtype=torch.int32)
            if kw:
                data["surfel_counts"] = torch.tensor([[10, 7, 4, 0], [10, 8, 5, 0]], dtype=torch.int32)

    model, data, out = Model(), {}, str(tmp_path / "maps")
    evalcli.dense_pairs(model, data, "POSE", (out, 4, 0.05, False, dict(radius=0.2)), 0)
    assert model.seen == ("POSE", 4, 0.05, None, dict(surfels=dict(radius=0.2)))
    assert capsys.readouterr().out == "dense 11 of 12 from 5\nsurfels 15 of 20 own 9 of 12\n"
    evalcli.dense_pairs(model, {}, "POSE", (out, 4, 0.05, False), 0)                 # without the flag: the call and the output as they were
    assert model.seen == ("POSE", 4, 0.05, None, {}) and capsys.readouterr().out == "dense 11 of 12 from 5\n"


@pytest.mark.parametrize("script,argv,needs", [
    ("Test_Geo.py", ("--pnp", "--dense-surfels"), "--dense-depth"),
    ("Test_Geo.py", ("--pnp", "--guided", "3", "--visible-surfels"), "--visible"),
    ("Test_Agent.py", ("--surfel-radius", "0.2"), "--dense-surfels"),
    ("Test_Agent.py", ("--refine", "3", "--visible", "--visible-surfels", "--surfel-max-px", "17"), "--surfel-max-px"),
])
def test_scripts_reject_misplaced_flags(script, argv, needs):
    res = subprocess.run([sys.executable, os.path.join(ROOT, script), *argv], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 2 and needs in res.stderr, res.stderr[-2000:]
