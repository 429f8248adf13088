"""CPU tier of point visibility: the float64 restatement in visibility_reference.py gives the hand-computed flags on a tiny
scene (so the yardstick of the GPU tests is itself checked), the scenes of the GPU tier keep their undecided rows under the cap,
ops.visibility refuses malformed arguments before the library is touched, the workspace query answers without a GPU, visible=None leaves
refine_pose_from_matches / search_pose on the path they had, and the header declares the entry points."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import visibility_reference as vr
from cmr_agent_amd import _lib, ops

mhm = importlib.import_module("cmr_agent_amd.models.MultiHeadModel")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement on the hand-checkable scene ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1, 16])
def test_restatement_on_the_hand_scene(radius):
    pts, pose, K = vr.hand()
    N = pts.shape[2]
    ones = torch.ones(1, N, dtype=torch.bool)
    r = vr.visibility(pts, ones, None, pose, K, vr.HAND_H, vr.HAND_W, radius, vr.HAND_REL_TOL, 0.0)[0]
    assert r["decided"].all() and r["undecided"] == 0 and not r["amb"].any()
    assert r["visible"].astype(int).tolist() == vr.HAND_VISIBLE[radius]
    assert r["counts_lo"] == vr.HAND_COUNTS[radius]
    assert r["cell_decided"].all() and np.array_equal(r["Z_lo"], r["Z_hi"])
    assert np.array_equal(r["Z_lo"].astype(np.float32), vr.hand_depth_map()[0].numpy())
    # the rows outside the map and behind the camera are no occluders: 8 rows in 6 cells (rows 0 / 1 and 3 / 4 share one each)
    assert int(np.isfinite(r["Z_lo"]).sum()) == 6


def test_restatement_masks_and_tolerances():
    pts, pose, K = vr.hand()
    N = pts.shape[2]
    ones = torch.ones(1, N, dtype=torch.bool)
    # without row 0 among the occluders, rows 1 and 2 are visible at radius 1; row 0, queried, does not write itself into Z
    occ = ones.clone()
    occ[0, 0] = False
    r = vr.visibility(pts, ones, occ, pose, K, vr.HAND_H, vr.HAND_W, 1, vr.HAND_REL_TOL, 0.0)[0]
    assert r["visible"].astype(int).tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 1, 1] and r["counts_lo"] == [10, 8, 7, 7]
    assert r["Z_lo"][2, 3] == 5.0
    # unselected rows are not visible but still occlude
    m = ones.clone()
    m[0, [0, 3]] = False
    r = vr.visibility(pts, m, None, pose, K, vr.HAND_H, vr.HAND_W, 0, vr.HAND_REL_TOL, 0.0)[0]
    assert r["visible"].astype(int).tolist() == [0, 0, 1, 0, 1, 0, 0, 1, 1, 1] and r["counts_lo"] == [8, 6, 5, 8]
    # a tighter relative tolerance hides row 4 (2.08 > 2 * 1.03); an absolute one brings it back
    r = vr.visibility(pts, ones, None, pose, K, vr.HAND_H, vr.HAND_W, 0, 0.03, 0.0)[0]
    assert r["visible"].astype(int).tolist() == [1, 0, 1, 1, 0, 0, 0, 1, 1, 1]
    r = vr.visibility(pts, ones, None, pose, K, vr.HAND_H, vr.HAND_W, 0, 0.03, 0.05)[0]
    assert r["visible"].astype(int).tolist() == vr.HAND_VISIBLE[0]
    # a NaN pose: nothing in view, Z all +inf, nothing visible, and all of it decided; an empty mask: zeros
    r = vr.visibility(pts, ones, None, torch.full((1, 4, 4), math.nan), K, vr.HAND_H, vr.HAND_W, 1, 0.05, 0.0)[0]
    assert r["decided"].all() and not r["visible"].any() and r["counts_lo"] == [10, 0, 0, 0] and np.isinf(r["Z_lo"]).all()
    r = vr.visibility(pts, ~ones, None, pose, K, vr.HAND_H, vr.HAND_W, 1, 0.05, 0.0)[0]
    assert r["decided"].all() and not r["visible"].any() and r["counts_lo"] == [0, 0, 0, 8]


def test_restatement_flags_a_projection_on_a_half_integer():
    """u = 3.5 exactly: the row has two candidate cells, it is ambiguous as an occluder and its cells are not decided; a row behind either
    cell and in front of everything sure is undecided, rows that a sure occluder hides or that lie in front of both stay decided."""
    pts = torch.tensor([[[3.5 * 2, 3 * 5, 4 * 5, 3 * 1], [2.0 * 2, 2 * 5, 2 * 5, 2 * 1], [2.0, 5, 5, 1]]])      # rows: (3.5, 2) z 2; (3, 2) z 5; (4, 2) z 5; (3, 2) z 1
    ones = torch.ones(1, 4, dtype=torch.bool)
    r = vr.visibility(pts, ones, None, torch.eye(4)[None], torch.eye(3)[None], 8, 10, 0, 0.05, 0.0)[0]
    assert r["amb"].tolist() == [True, False, False, False]
    assert not r["cell_decided"][2, 3] and not r["cell_decided"][2, 4] and int((~r["cell_decided"]).sum()) == 2
    assert r["decided"].tolist() == [False, True, False, True] and r["visible"].tolist() == [False, False, False, True] and r["undecided"] == 2
    assert r["Z_lo"][2, 3] == 1.0 and r["Z_lo"][2, 4] == 2.0 and r["Z_hi"][2, 3] == 1.0 and r["Z_hi"][2, 4] == 5.0


# ---- the cap on the scenes of the GPU tier -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in vr.SCENES])
def test_undecided_rows_stay_under_the_cap(name):
    """At most max(4, 1 %) of a sample's selected rows may be undecided -- a condition on the inputs, asserted from the restatement alone."""
    sc = vr.built(name)
    radii = next(s for s in vr.SCENES if s[0] == name)[2]
    for radius in radii:
        res = vr.visibility(sc["pts"], sc["mask"], sc["occ_mask"], sc["pose"], sc["K"], sc["h"], sc["w"], radius, vr.REL_TOL, vr.ABS_TOL)
        for b, r in enumerate(res):
            nsel = int(r["sel"].sum())
            print(name, "r", radius, "sample", b, "selected", nsel, "undecided", r["undecided"], "decided visible", int(r["visible"].sum()),
                  "ambiguous occluders", r["occ_amb"], "undecided cells", int((~r["cell_decided"]).sum()))
            assert r["undecided"] <= vr.cap(nsel)
            if sc["pts"].shape[2] > 1 and radius <= 2:                                      # (radius 16 covers most of a 13 x 19 map)
                assert 0 < int(r["visible"].sum()) < r["counts_lo"][1]                      # the scene has both outcomes


def test_planted_occlusion_is_decided():
    for h, w in ((13, 19), (40, 128)):
        sc = vr.planted_occlusion(h, w, seed=311)
        N = sc["pts"].shape[2]
        for radius in (0, 1):
            r = vr.visibility(sc["pts"], np.ones((1, N), bool), None, sc["pose"], sc["K"], h, w, radius, vr.REL_TOL, vr.ABS_TOL)[0]
            assert r["decided"].all() and np.array_equal(r["visible"], sc["expect"])


# ---- argument checks and the workspace query ------------------------------------------------------------------------------------------------
def _args(B=2, N=8):
    return [torch.zeros(B, 3, N), torch.eye(4).repeat(B, 1, 1), torch.eye(3).repeat(B, 1, 1), 4, 5, torch.ones(B, N, dtype=torch.bool)]


def _refused(args, match, **kw):
    with pytest.raises(ValueError, match=match):
        ops.visibility(*args, **kw)


def test_visibility_argument_checks(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(_lib, "call", touched)
    a = _args()
    _refused([a[0][0]] + a[1:], "visibility: pts must be")
    _refused([a[0][:, :2]] + a[1:], "visibility: pts must be")
    for i in (0, 1, 2):
        b = list(a)
        b[i] = b[i].double()
        _refused(b, "visibility: pts, pose and K must be float32")
    _refused([a[0], a[1][:1]] + a[2:], "visibility: pose must be")
    _refused([a[0], a[1][:, :3]] + a[2:], "visibility: pose must be")
    _refused(a[:2] + [a[2][:1]] + a[3:], "visibility: K must be")
    for h, w in ((0, 5), (4, 0), (-1, 5), (4097, 4096)):
        _refused(a[:3] + [h, w] + a[5:], "visibility: need 1 <= B")
    for h in (4.5, None, "4", True, math.nan):
        _refused(a[:3] + [h, 5] + a[5:], "visibility: h and w must be integers")
    _refused(a[:5] + [a[5].float()], "visibility: mask must be")
    _refused(a[:5] + [a[5][:1]], "visibility: mask must be")
    _refused(a, "visibility: occ_mask must be", occ_mask=a[5].float())
    _refused(a, "visibility: occ_mask must be", occ_mask=a[5][:1])
    for radius in (-1, ops.GUIDED_MAX_RADIUS + 1, 1.5, math.nan, True, "2"):
        _refused(a, "visibility: radius must be", radius=radius)
    for tol in (-0.1, math.inf, math.nan, None, "x", 1e39):
        _refused(a, "visibility: rel_tol must be", rel_tol=tol)
        _refused(a, "visibility: abs_tol must be", abs_tol=tol)
    # every check above passed on CPU tensors: the device check comes last, still ahead of the library
    _refused(a, "visibility: every tensor must be a contiguous tensor on the same GPU")
    _refused(a, "visibility: every tensor must be a contiguous tensor on the same GPU", occ_mask=a[5].long(), radius=16, rel_tol=0, abs_tol=2.5)


def test_workspace_query_and_header():
    lib = _lib.load()
    up16 = lambda v: (v + 15) // 16 * 16
    assert lib.cmr_visibility_workspace_bytes(3, 1025, 13, 19) == up16(3 * 13 * 19 * 4) + 2 * up16(3 * 1025 * 4)
    assert lib.cmr_visibility_workspace_bytes(1, 1, 1, 1) == 48
    for bad in ((0, 8, 4, 5), (2, 0, 4, 5), (2, 8, 0, 5), (2, 8, 4, -1)):
        assert lib.cmr_visibility_workspace_bytes(*bad) == 0
    text = open(os.path.join(ROOT, "include", "cmr_hip.h")).read()
    assert re.search(r"int64_t\s+cmr_visibility_workspace_bytes\s*\(\s*int B,\s*int N,\s*int h,\s*int w\s*\)", text)
    assert re.search(r"int\s+cmr_visibility_f32\s*\(", text)
    names = _lib.parse_header()["cmr_visibility_f32"][2]
    assert names == ["pts", "mask", "mask_bytes", "occ_mask", "occ_mask_bytes", "pose", "K", "B", "N", "h", "w", "radius", "rel_tol", "abs_tol",
                     "visible", "counts", "depth_map", "cell", "depth", "workspace", "workspace_bytes", "stream"]
    from cmr_agent_amd.utils import workmodel
    assert "cmr_visibility_f32" in open(workmodel.__file__).read()


# ---- visible=None is the path that existed ---------------------------------------------------------------------------------------------------
class _FakeOps:
    """Stands in for cmr_agent_amd.ops inside MultiHeadModel: CPU tensors of the right shapes, and a log of the calls."""
    _is_int = staticmethod(ops._is_int)

    def __init__(self):
        self.log = []

    def visibility(self, pts, pose, K, h, w, mask, **kw):
        B, _, N = pts.shape
        self.log.append(("visibility", pose.clone(), (h, w), mask, kw))
        vis = (mask.reshape(-1) != 0) & (torch.arange(B * N) % 2 == 0)
        counts = torch.tensor([[int(mask[b].ne(0).sum()), 0, int(vis.view(B, N)[b].sum()), N] for b in range(B)], dtype=torch.int32)
        return vis, counts, None, None, None

    def guided_match(self, pts, feat, img, mask, pose, K, radius, **kw):
        B, _, N = pts.shape
        self.log.append(("guided_match", pose.clone(), radius, mask))
        return torch.zeros(B * N, dtype=torch.int32), torch.ones(B * N, dtype=torch.bool), torch.zeros(B, 4, dtype=torch.int32), None, None

    def pnp_refine(self, pts, uv, use, K, pose, thr=1.0, iters=10):
        B = pts.shape[0]
        self.log.append(("pnp_refine", pose.clone()))
        nxt = pose.clone()
        nxt[:, 0, 3] += 1.0                                                      # every round moves the pose: the next round must see it
        return nxt, torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)

    def pose_score(self, pts, feat, img, mask, poses, K, radius=0, tau=0.8):
        B, P = poses.shape[:2]
        self.log.append(("pose_score", mask, radius))
        score = torch.ones(B, P, dtype=torch.float64)
        score[:, 1] = 0.5                                                        # candidate 1 wins every round
        return score, torch.zeros(B, P, 2, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)


def _batch(B=2, N=6, h=4, w=5):
    g = torch.Generator().manual_seed(5)
    return {"pc": torch.randn(B, 3, N, generator=g), "K": torch.eye(3).repeat(B, 1, 1), "pc_geo_feat": torch.randn(B, 64, N, generator=g),
            "img_geo_feat": torch.randn(B, 64, h, w, generator=g), "pc_overlap_pred": torch.ones(B, N, dtype=torch.int64),
            "pnp_pose": torch.eye(4).repeat(B, 1, 1)}


def test_refine_without_visible_takes_the_old_path(monkeypatch):
    fake = _FakeOps()
    monkeypatch.setattr(mhm, "ops", fake)
    model = mhm.MultiHeadModel.__new__(mhm.MultiHeadModel)                       # the methods under test use no weights
    data = _batch()
    mhm.MultiHeadModel.refine_pose_from_matches(model, data, radii=(3, 1), thrs=(2.0, 1.0), visible=None)
    assert [c[0] for c in fake.log] == ["guided_match", "pnp_refine"] * 2
    assert all(c[3].dtype == torch.int64 and torch.equal(c[3], data["pc_overlap_pred"]) for c in fake.log if c[0] == "guided_match")
    assert "refine_visible_counts" not in data and tuple(data["guided_counts"].shape) == (2, 2, 4)
    # with visible: one ops.visibility per round, ahead of the match, under that round's pose, on the geometric map, every row occluding;
    # the match sees its flags
    fake.log.clear()
    data = _batch()
    mhm.MultiHeadModel.refine_pose_from_matches(model, data, radii=(3, 1), thrs=(2.0, 1.0), visible=dict(radius=2, abs_tol=0.5))
    assert [c[0] for c in fake.log] == ["visibility", "guided_match", "pnp_refine"] * 2
    for k in (0, 3):
        vis, gm = fake.log[k], fake.log[k + 1]
        assert torch.equal(vis[1], gm[1]) and float(vis[1][0, 0, 3]) == k // 3 and vis[2] == (4, 5)
        assert vis[4] == dict(radius=2, rel_tol=0.05, abs_tol=0.5) and torch.equal(vis[3], data["pc_overlap_pred"])
        assert gm[3].dtype == torch.bool and gm[3].view(-1).tolist() == [i % 2 == 0 for i in range(12)]
    assert tuple(data["refine_visible_counts"].shape) == (2, 2, 4) and data["refine_visible_counts"].dtype == torch.int32
    fake.log.clear()
    mhm.MultiHeadModel.refine_pose_from_matches(model, _batch(), radii=(3,), thrs=(2.0,), visible=True)
    assert fake.log[0][0] == "visibility" and fake.log[0][4] == dict(radius=1, rel_tol=0.05, abs_tol=0.0)
    for bad in (3, "yes", dict(tau=1.0)):
        with pytest.raises(ValueError, match="refine_pose_from_matches: visible must be"):
            mhm.MultiHeadModel.refine_pose_from_matches(model, _batch(), visible=bad)


def test_search_without_visible_takes_the_old_path(monkeypatch):
    fake = _FakeOps()
    monkeypatch.setattr(mhm, "ops", fake)
    model = mhm.MultiHeadModel.__new__(mhm.MultiHeadModel)
    levels = ((2, 1.0, 0.1, 2), (0, 0.5, 0.05, 1))
    data = _batch()
    mhm.MultiHeadModel.search_pose(model, data, levels=levels, visible=None)
    assert [c[0] for c in fake.log] == ["pose_score"] * 3
    assert all(torch.equal(c[1], data["pc_overlap_pred"]) and c[1].dtype == torch.int64 for c in fake.log)
    assert "search_visible_counts" not in data
    want = data["searched_pose"].clone()
    fake.log.clear()
    data = _batch()
    mhm.MultiHeadModel.search_pose(model, data, levels=levels, visible=True)
    assert [c[0] for c in fake.log] == ["visibility", "pose_score", "pose_score", "visibility", "pose_score"]
    assert torch.equal(fake.log[0][1], data["pnp_pose"]) and not torch.equal(fake.log[3][1], data["pnp_pose"])      # each level under its start pose
    assert all(c[1].dtype == torch.bool for c in fake.log if c[0] == "pose_score")
    assert tuple(data["search_visible_counts"].shape) == (2, 2, 4) and torch.equal(data["searched_pose"], want)
    with pytest.raises(ValueError, match="search_pose: visible must be"):
        mhm.MultiHeadModel.search_pose(model, _batch(), levels=levels, visible=dict(tau=1.0))


def test_visible_points_and_render_depth_refuse_bad_options():
    model = mhm.MultiHeadModel.__new__(mhm.MultiHeadModel)
    with pytest.raises(ValueError, match="visible_points: occluders must be"):
        mhm.MultiHeadModel.visible_points(model, _batch(), occluders="some")
    with pytest.raises(ValueError, match="render_depth: size and K go together"):
        mhm.MultiHeadModel.render_depth(model, _batch(), size=(8, 10))
    with pytest.raises(ValueError, match="render_depth: size and K go together"):
        mhm.MultiHeadModel.render_depth(model, _batch(), K=torch.eye(3))


# ---- the command-line flags ---------------------------------------------------------------------------------------------------------------
def test_visible_flags():
    import argparse
    from cmr_agent_amd.utils import evalcli

    def parse(*argv, parent_given=True):
        ap = argparse.ArgumentParser()
        evalcli.add_visible_flags(ap, "--guided")
        return evalcli.visible_option(ap, ap.parse_args(list(argv)), "--guided", parent_given, ops.GUIDED_MAX_RADIUS)

    assert parse() is None and parse(parent_given=False) is None
    assert parse("--visible") == {}
    assert parse("--visible", "--visible-radius", "2", "--visible-rel-tol", "0.1", "--visible-abs-tol", "0.5") == dict(radius=2, rel_tol=0.1, abs_tol=0.5)
    for argv, given in ((("--visible",), False), (("--visible-radius", "2"), True), (("--visible", "--visible-radius", "17"), True),
                        (("--visible", "--visible-rel-tol", "-1"), True), (("--visible", "--visible-abs-tol", "inf"), True)):
        with pytest.raises(SystemExit):
            parse(*argv, parent_given=given)


def test_print_visible(capsys):
    from cmr_agent_amd.utils import evalcli
    evalcli.print_visible(torch.tensor([[[9, 9, 9, 9], [9, 9, 9, 9]], [[10, 8, 5, 20], [6, 4, 3, 20]]], dtype=torch.int32))
    assert capsys.readouterr().out == "visible 8 of 12 of 16\n"
