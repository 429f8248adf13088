"""CPU tier of the registration without a start pose: the restatement's hand-computed cases and its own facts on the scene
pair, every argument check of the four wrappers ahead of the library, and `align --init` with the restatement in the ops' place."""
import os

import numpy as np
import pytest
import torch

import cloud_global_reference as G
import cloud_icp_reference as I
from cmr_agent_amd import _lib, ops
from cmr_agent_amd.dataset import align


# ---- hand-computed cases ----------------------------------------------------------------------------------------------------------------
def test_two_points_with_perpendicular_normals_feature_by_feature():
    """p_i = 0, n_i = z; p_j = (3, 0, 4), n_j = y.  d = (3, 0, 4), l = 5, a1 = 4/5, a2 = 0: no swap, f3 = 0.8.  v = d x z = (0, -3, 0) ->
    (0, -1, 0); w = z x v = (1, 0, 0); f2 = v . y = -1; f1 = atan2(w . y, z . y) = atan2(0, 0) = 0.  Bins: floor(11 * 0.5) = 5,
    floor(11 * 0) = 0, floor(11 * 0.9) = 9.  Seen from j the pair SWAPS (|a1| = 0 < |a2| = 0.8) and lands on the same frame: same features."""
    p = np.array([[0, 0, 0], [3, 0, 4]], np.float32)
    n = np.array([[0, 0, 1], [0, 1, 0]], np.float32)
    f = G.pair_features(p[[0, 1]], n[[0, 1]], p[[1, 0]], n[[1, 0]])
    assert f["swap"].tolist() == [False, True] and f["used"].all()
    assert f["f1"].tolist() == [0.0, 0.0] and f["f2"].tolist() == [-1.0, -1.0] and f["f3"].tolist() == [0.8, 0.8]
    r = G.fpfh(p, n, 5.0)
    assert r["count"].tolist() == [1, 1] and r["edge"].tolist() == [0, 0] and r["pairs"][2].tolist() == [25.0, 25.0]
    want = np.zeros(33, np.int64)
    want[[5, 11 + 0, 22 + 9]] = 1
    assert np.array_equal(r["spfh"], np.stack([want, want]))
    # the neighbour's SPFH value 100 / 25, scaled to 100, plus the row's own 100
    assert np.array_equal(r["fpfh"], 200.0 * np.stack([want, want]))
    # out of reach: no neighbour, all zero
    r = G.fpfh(p, n, 4.99)
    assert not r["count"].any() and not r["spfh"].any() and not r["fpfh"].any()


def test_skipped_pairs_and_rows_that_take_no_part():
    n = np.array([[0, 0, 1], [1, 0, 0]], np.float32)
    # l = 0: the rows are neighbours (count 1), the pair is skipped and has d2 = 0
    r = G.fpfh(np.zeros((2, 3), np.float32), n, 1.0)
    assert r["count"].tolist() == [1, 1] and not r["spfh"].any() and not r["fpfh"].any()
    # d parallel to n1: from i, a1 = 0 < a2 = 1 swaps to n1 = n_j = x, d = -x: v = d x n1 = 0, skipped; from j the same
    p = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    f = G.pair_features(p[[0, 1]], n[[0, 1]], p[[1, 0]], n[[1, 0]])
    assert not f["used"].any()
    r = G.fpfh(p, n, 1.0)
    assert r["count"].tolist() == [1, 1] and not r["spfh"].any() and not r["fpfh"].any()
    # a third row makes one used pair each: the skipped pair still counts in k, so the SPFH value is 100 * 1 / 2
    p3 = np.array([[0, 0, 0], [1, 0, 0], [0, 0.5, 0.5]], np.float32)
    n3 = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float32)
    r = G.fpfh(p3, n3, 1.0)
    assert r["count"].tolist() == [2, 1, 1] and r["spfh"][0].sum() == 3 and r["value"][0].sum() == 150.0
    # zero, NaN and infinite normals, NaN rows: nobody's neighbour
    n3[2] = 0
    assert G.fpfh(p3, n3, 1.0)["count"].tolist() == [1, 1, 0]
    for bad in (np.nan, np.inf):
        n3[2] = [0, bad, 0]
        assert G.fpfh(p3, n3, 1.0)["count"].tolist() == [1, 1, 0]
    n3[2] = [0, 1, 0]
    p3[2, 0] = np.nan
    r = G.fpfh(p3, n3, 1.0)
    assert r["part"].tolist() == [True, True, False] and r["count"].tolist() == [1, 1, 0]
    # an atan2 on a bin's edge is reported: opposite normals, n1 . n2 = -1 and w . n2 = +-0 give f1 = +-pi exactly, x1 = 0 or 1
    p = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    n = np.array([[0, 0, 1], [0, 0, -1]], np.float32)
    assert G.fpfh(p, n, 1.0)["edge"].tolist() == [1, 1]


def _py_mix(x):
    x ^= x >> 16
    x = (x * 0x21f0aaad) & 0xffffffff
    x ^= x >> 15
    x = (x * 0xd35a2d97) & 0xffffffff
    x ^= x >> 15
    return x


def test_hash_and_draws():
    for seed, h, c in ((0, 0, 0), (7, 4095, 31), (2 ** 32 - 1, 123456, 5)):
        want = _py_mix(_py_mix(_py_mix(_py_mix(seed ^ 0x9e3779b9) ^ 0) ^ h) ^ c)
        assert int(G.hash32(seed, 0, np.array([h]), c)[0]) == want
    idx, got = G.draws(3, 1000, 3)
    assert (got == 3).all() and (np.sort(idx, 1) == [0, 1, 2]).all() and len({tuple(r) for r in idx}) == 6
    idx, got = G.draws(3, 1000, 1283)
    assert (got == 3).all() and (idx[:, 0] != idx[:, 1]).all() and (idx[:, 1] != idx[:, 2]).all() and (idx[:, 0] != idx[:, 2]).all()
    assert G.draws(3, 10, 2)[1].tolist() == [0] * 10


def test_three_exact_correspondences_a_collinear_triple_and_an_edge_rejection():
    a = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], np.float32)
    T = I.pose_matrix((0.0, 0.0, np.pi / 2), (1.0, 2.0, 3.0))
    b = (a.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    b[3] = 0                                                                              # row 3 is no correspondence
    corr = np.array([[0, 0], [1, 1], [2, 2]])
    r = G.ransac(a, b, corr, n_hyp=8)
    assert r["status"] == 0 and r["inliers"] == 3 and r["best"] == 0 and (r["hyp_inliers"] == 3).all() and np.abs(r["pose"] - T).max() < 1e-7
    assert abs(np.linalg.det(r["pose"][:3, :3]) - 1.0) < 1e-12
    # rows out of range and -1 are dropped first
    r2 = G.ransac(a, b, np.array([[-1, 0], [0, 0], [1, 1], [9, 1], [2, 2], [2, -1], [0, 4]]), n_hyp=8)
    assert r2["count"] == 3 and np.array_equal(r2["pose"], r["pose"])
    assert G.ransac(a, b, corr[:2], n_hyp=8)["status"] == 1
    # a mirror image has no proper rotation onto it: the fit stays a rotation
    m = b.copy()
    m[:, 2] = -m[:, 2]
    r = G.ransac(a, m, corr, n_hyp=8)
    assert abs(np.linalg.det(r["pose"][:3, :3]) - 1.0) < 1e-12
    # collinear
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
    r = G.ransac(line, line, corr, n_hyp=8)
    assert r["status"] == 2 and (r["hyp_inliers"] == -1).all() and r["inliers"] == 0 and np.array_equal(r["pose"], np.eye(4))
    # an edge 0.85 of its partner is rejected at 0.9 and passes at 0.8
    s = b.copy()
    s[2] = b[0] + 0.85 * (b[2] - b[0])
    assert G.ransac(a, s, corr, n_hyp=8)["status"] == 2
    assert G.ransac(a, s, corr, n_hyp=8, edge_ratio=0.8, thr=1.0)["status"] == 0


def test_descriptor_nearest_by_hand():
    q = np.array([[0, 0], [1, 1], [np.nan, 0], [5, 5]], np.float32)
    t = np.array([[1, 0], [0, 1], [1, 1], [1, 1]], np.float32)
    idx, d2 = G.descriptor_nearest(q, t)
    assert idx.tolist() == [0, 2, -1, 2] and d2[[0, 1, 3]].tolist() == [1.0, 0.0, 32.0] and np.isnan(d2[2])
    idx, d2 = G.descriptor_nearest(q, t, np.array([1, 1, 1, 0], bool), np.array([0, 1, 0, 1], bool))
    assert idx.tolist() == [1, 3, -1, -1]
    assert G.descriptor_nearest(q, t[:0])[0].tolist() == [-1] * 4


# ---- the restatement's own facts on the scene pair (DESIGN.md 4af records them) ---------------------------------------------------------------
def test_edge_shares():
    ft, g = G.target_features(), G.global_case("other", 3)
    for name, f in (("scene 11", ft), ("scene 12 moved", g["feat"])):
        rows, edge = int(f["part"].sum()), int((f["edge"] > 0).sum())
        print("%s: %d rows take part, %d with an edge pair, %d pairs" % (name, rows, edge, f["pairs"][0].size))
        assert edge <= 0.05 * rows
    assert ft["part"].sum() == 4447 and (~ft["part"]).sum() == 42
    print("correspondences %d, within 0.3 m under the truth %.3f" % (len(g["corr"]), g["within"]))
    assert 0.15 <= g["within"] <= 0.35 and len(g["corr"]) > 1000


@pytest.mark.parametrize("seed", G.SEEDS)
def test_ransac_lands_inside_the_basin(seed):
    g = G.global_case("other", 3)
    r = G.ransac_case("other", 3, seed)
    rot, trans = I.pose_error(r["pose"], g["truth"])
    print("seed %d: valid %d inliers %d edge %d error %.4f rad %.4f m" % (seed, (r["hyp_inliers"] >= 0).sum(), r["inliers"], r["edge"].sum(),
                                                                          rot, trans))
    assert r["status"] == 0 and rot <= G.BAR_ROT and trans <= G.BAR_TRANS
    assert r["edge"].mean() <= 0.01


@pytest.mark.parametrize("k", range(4))
def test_icp_from_the_ransac_pose_reaches_the_error_of_4ae(k):
    """4ae records 8.0 - 8.8e-4 rad and 0.9 - 1.4 mm for the other cloud from the identity, inside the basin; from the RANSAC pose the loop
    must end no more than 10 % above that.  (Measured: 8.07e-4 rad at all four poses and 1.04, 0.65, 1.32, 1.12 mm -- poses 0 and 1 end
    BELOW what 4ae's start reaches, 8.78e-4 / 1.33 mm and 8.82e-4 / 0.94 mm, which is why the bar is one-sided.)"""
    g = G.global_case("other", k)
    r = G.ransac_case("other", k, 0)
    ref = G.refined_case("other", k)
    rot0, trans0 = I.pose_error(r["pose"], g["truth"])
    rot, trans = I.pose_error(ref["pose"], g["truth"])
    print("pose %d: RANSAC %.4f rad %.4f m -> ICP status %d iterations %d: %.3g rad %.3g m" % (k, rot0, trans0, ref["status"], ref["iterations"],
                                                                                               rot, trans))
    assert rot0 <= G.BAR_ROT and trans0 <= G.BAR_TRANS and ref["status"] == 0
    assert rot <= 1.1 * 8.8e-4 and trans <= 1.1 * 1.4e-3


def test_todays_icp_alone_does_not_leave_the_identity_on_the_far_pose():
    g, case = G.global_case("other", 3), I.pair_case()
    out = I.icp(g["source"], case["target"], case["normals"], None, 1.0, 0.1, 30)
    rot, _ = I.pose_error(out["pose"], g["truth"])
    assert out["status"] == 2 or rot > 1.0


# ---- argument checks: every one raises before the library is reached --------------------------------------------------------------------
def _touched(*a, **k):
    raise AssertionError("the library was reached")


def _index(n=8, cell=1.0):
    return ops.CloudIndex(torch.zeros((n, 4)), torch.zeros((n,), dtype=torch.int64), torch.zeros((n,), dtype=torch.int64), (0.0, 0.0, 0.0), cell, n, n)


BAD_POINTS = (torch.zeros((8, 2)), torch.zeros((8,)), torch.zeros((2, 8, 3)), torch.zeros((8, 3), dtype=torch.float64), None,
              np.zeros((8, 3), np.float32))
BAD_SCALARS = (0.0, -0.1, float("inf"), float("nan"), 1e-50, 1e39)


def test_argument_checks(monkeypatch):
    monkeypatch.setattr(_lib, "load", _touched)
    monkeypatch.setattr(_lib, "call", _touched)
    p = torch.zeros((8, 3))
    # point_fpfh
    for bad in BAD_SCALARS:
        with pytest.raises(ValueError, match="radius must be a finite number > 0"):
            ops.point_fpfh(p, p, bad)
    for bad in (p, (p, p), "x"):
        with pytest.raises(ValueError, match="index must be a CloudIndex"):
            ops.point_fpfh(p, p, 1.0, bad)
    for bad in (1.5, 1.0000001):
        with pytest.raises(ValueError, match="exceeds the index's cell"):
            ops.point_fpfh(p, p, bad, _index())
    for bad in BAD_POINTS:
        with pytest.raises(ValueError, match="points must be a float32"):
            ops.point_fpfh(bad, p, 1.0)
    with pytest.raises(ValueError, match="device tensor"):
        ops.point_fpfh(p, p, 1.0)
    # descriptor_nearest
    d = torch.zeros((8, 33))
    for bad in (torch.zeros((8,)), torch.zeros((8, 0)), torch.zeros((2, 8, 33)), torch.zeros((8, 33), dtype=torch.float64), None,
                np.zeros((8, 33), np.float32)):
        with pytest.raises(ValueError, match="queries must be a float32"):
            ops.descriptor_nearest(bad, d)
        with pytest.raises(ValueError, match="targets must be a float32"):
            ops.descriptor_nearest(d, bad)
    with pytest.raises(ValueError, match="queries have 33 channels, targets 32"):
        ops.descriptor_nearest(d, torch.zeros((8, 32)))
    with pytest.raises(ValueError, match="65 channels; the kernel serves at most 64"):
        ops.descriptor_nearest(torch.zeros((8, 65)), torch.zeros((4, 65)))
    for bad in (torch.zeros(7, dtype=torch.bool), torch.zeros((8, 1), dtype=torch.bool), torch.zeros(8), torch.zeros(8, dtype=torch.int64),
                np.zeros(8, bool)):
        with pytest.raises(ValueError, match="query_mask must be None or bool / uint8 \\[8\\]"):
            ops.descriptor_nearest(d, d[:5], query_mask=bad)
        with pytest.raises(ValueError, match="target_mask must be None or bool / uint8 \\[8\\]"):
            ops.descriptor_nearest(d[:5], d, target_mask=bad)
    with pytest.raises(ValueError, match="device tensor"):
        ops.descriptor_nearest(d, d, torch.ones(8, dtype=torch.bool), torch.ones(8, dtype=torch.uint8))
    # ransac_rigid
    c = torch.zeros((5, 2), dtype=torch.int32)
    for bad in (0, -1, (1 << 20) + 1, 2.5, True, None, float("nan")):
        with pytest.raises(ValueError, match="n_hyp must be an integer"):
            ops.ransac_rigid(p, p, c, n_hyp=bad)
    for bad in BAD_SCALARS:
        with pytest.raises(ValueError, match="thr must be a finite number > 0"):
            ops.ransac_rigid(p, p, c, thr=bad)
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError, match="edge_ratio must be a number in \\[0, 1\\]"):
            ops.ransac_rigid(p, p, c, edge_ratio=bad)
    for bad in (-1, 1 << 32, 0.5, None, True):
        with pytest.raises(ValueError, match="seed must be an integer"):
            ops.ransac_rigid(p, p, c, seed=bad)
    for bad in (torch.zeros((5, 2), dtype=torch.int64), torch.zeros((5, 3), dtype=torch.int32), torch.zeros((10,), dtype=torch.int32), None,
                np.zeros((5, 2), np.int32)):
        with pytest.raises(ValueError, match="corr must be an int32 \\[L, 2\\]"):
            ops.ransac_rigid(p, p, bad)
    for bad in BAD_POINTS:
        with pytest.raises(ValueError, match="source_pts must be a float32"):
            ops.ransac_rigid(bad, p, c)
    with pytest.raises(ValueError, match="device tensor"):
        ops.ransac_rigid(p, p, c)
    # register_global
    for kw in (dict(mutual=1), dict(refine=None), dict(mutual="yes")):
        with pytest.raises(ValueError, match="mutual and refine must be True or False"):
            ops.register_global(p, p, p, p, **kw)
    with pytest.raises(ValueError, match="unknown keyword\\(s\\) index, pose"):
        ops.register_global(p, p, p, p, pose=None, index=None)
    for bad in BAD_SCALARS:
        with pytest.raises(ValueError, match="radius must be a finite number > 0"):
            ops.register_global(p, p, p, p, radius=bad)
    for bad in BAD_POINTS:
        with pytest.raises(ValueError, match="points must be a float32"):
            ops.register_global(bad, p, p, p)
    with pytest.raises(ValueError, match="device tensor"):
        ops.register_global(p, p, p, p)


def test_checks_behind_the_device_check(monkeypatch):
    """The checks that follow the first look at a tensor's device, with that look switched off."""
    monkeypatch.setattr(_lib, "load", _touched)
    monkeypatch.setattr(_lib, "call", _touched)
    real = ops._cloud_points

    def shape_only(t, name="points"):
        try:
            return real(t, name)
        except ValueError as e:
            if "device tensor" not in str(e):
                raise
            return t

    monkeypatch.setattr(ops, "_cloud_points", shape_only)
    p = torch.zeros((8, 3))
    for bad in (torch.zeros((8, 2)), torch.zeros((8, 3), dtype=torch.float64), None):
        with pytest.raises(ValueError, match="normals must be a float32"):
            ops.point_fpfh(p, bad, 1.0)
        with pytest.raises(ValueError, match="target_pts must be a float32"):
            ops.ransac_rigid(p, bad, torch.zeros((5, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="points has 8 rows, normals 7"):
        ops.point_fpfh(p, p[:7], 1.0)
    with pytest.raises(ValueError, match="points has 8 rows, normals 8, the index 9"):
        ops.point_fpfh(p, p, 1.0, _index(9))
    with pytest.raises(ValueError, match="contiguous tensor on the same GPU"):
        ops.ransac_rigid(p, p, torch.zeros((5, 2), dtype=torch.int32))
    # empty inputs: no launch, no error
    e = ops.point_fpfh(p[:0], p[:0], 1.0, want_spfh=True)
    assert e.fpfh.shape == (0, 33) and e.count.shape == (0,) and e.spfh.dtype == torch.int32
    e = ops.point_fpfh(p, p, 1.0, _index(8)._replace(kept=0))
    assert e.fpfh.shape == (8, 33) and not e.fpfh.any() and e.spfh is None and e.count.dtype == torch.int32


def test_header_and_work_model_know_the_entry_points():
    from cmr_agent_amd.utils import workmodel
    protos = _lib.parse_header()
    src = open(workmodel.__file__).read()
    for name in ("cmr_point_fpfh_f32", "cmr_point_fpfh_workspace_bytes", "cmr_descriptor_nearest_f32", "cmr_ransac_rigid_f32",
                 "cmr_ransac_rigid_workspace_bytes"):
        assert name in protos, name
        assert name.endswith("_bytes") or name in src
    assert protos["cmr_descriptor_nearest_f32"][2] == ["queries", "M", "targets", "N", "C", "query_mask", "target_mask", "idx", "d2", "stream"]
    fl, by = workmodel.WORK["cmr_descriptor_nearest_f32"](dict(M=1000, N=500, C=33))
    assert fl == 3.0 * 1000 * 500 * 33 and by > 0
    lib = _lib.load()
    assert lib.cmr_point_fpfh_workspace_bytes(0) == 0 and lib.cmr_point_fpfh_workspace_bytes(4) == 4 * 33 * 4 + 16
    assert lib.cmr_ransac_rigid_workspace_bytes(0, 16) == 0 and lib.cmr_ransac_rigid_workspace_bytes(10, 16) == 160 + 160 + 16 + 16 * 96 + 64
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "cmr_agent_amd", "csrc")
    # the hash is stated once, in the header both RANSACs include
    assert "0x21f0aaad" in open(os.path.join(csrc, "cmr_pnp.h")).read()
    for name in ("pnp.hip", "cloud_global.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "cmr_pnp.h"' in text and "pnp_hash(seed" in text and "0x21f0aaadu" not in text
    for name in ("cloud_fpfh.hip", "cloud_global.hip"):
        assert '#include "cmr_cloud_grid.h"' in open(os.path.join(csrc, name)).read()


# ---- align --init -------------------------------------------------------------------------------------------------------------------------
def test_align_init_recovers_a_broken_chain(tmp_path, monkeypatch, capsys):
    """The file layer with the restatement in the ops' place: no GPU.  Frame 5 lies 10 m from where its neighbours are."""
    used = []
    monkeypatch.setattr(ops, "icp_point_to_plane", I.ops_icp_point_to_plane)
    monkeypatch.setattr(ops, "register_global", lambda *a, **k: used.append(k) or G.ops_register_global(*a, **k))
    step = I.pose_matrix((0.0, 0.0, 0.02), (0.3, 0.02, 0.0))
    jump = I.pose_matrix((0.0, 0.0, 0.5), (0.0, 0.0, 10.0))                                   # straight up: no row within max_dist
    truths = [step, jump, np.linalg.inv(jump) @ step]
    root = str(tmp_path)
    I.write_frames(root, I.chained_frames(truths))
    base = ["--root", root, "--data-velodyne", "vel", "--sequence", "9", "--huber", "0"]
    out = str(tmp_path / "poses.txt")
    # today's behaviour: the default, and --init previous, byte for byte -- the jump ends with status 2 and poisons the pair after it
    align.main(base, device="cpu")
    plain = capsys.readouterr().out
    align.main(base + ["--init", "previous"], device="cpu")
    assert capsys.readouterr().out == plain and not used
    lines = plain.splitlines()
    assert len(lines) == 3 and " status 0 " in lines[0] and " status 2 " in lines[1] and " status 2 " in lines[2]
    # auto: the two pairs that fail are repeated from a global start, one more line each
    align.main(base + ["--init", "auto", "--out", out, "--ransac-hyp", "512", "--seed", "3", "--fpfh-radius", "1.25", "--ransac-thr", "0.25"],
               device="cpu")
    lines = capsys.readouterr().out.splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["pair 3 4", "pair 4 5", "pair 4 5", "pair 5 6", "pair 5 6"]
    assert lines[0] == plain.splitlines()[0]
    for ln in (lines[1], lines[3]):
        w = ln.split()
        assert w[3:5] == ["global", "inliers"] and w[6] == "of" and w[8:] == ["status", "0"] and 3 <= int(w[5]) <= int(w[7])
    assert all(" status 0 " in ln for ln in (lines[2], lines[4]))
    assert len(used) == 2 and used[0] == dict(radius=1.25, n_hyp=512, thr=0.25, seed=3, refine=False)
    chain = np.loadtxt(out).reshape(4, 3, 4)
    want = np.eye(4)
    for j, T in enumerate(truths):
        want = want @ T
        assert np.abs(chain[j + 1] - want[:3]).max() < 1e-4, j
    # global: every pair starts from the global registration, no extra line
    used.clear()
    align.main(base + ["--init", "global", "--ransac-hyp", "512"], device="cpu")
    lines = capsys.readouterr().out.splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["pair 3 4", "pair 4 5", "pair 5 6"] and all(" status 0 " in ln for ln in lines)
    assert len(used) == 3 and used[0]["n_hyp"] == 512 and used[0]["radius"] == 1.0


def test_align_init_flag_rules(tmp_path):
    _, args = align.parse_args(["--root", "d", "--sequence", "3"])
    assert (args.init, args.fpfh_radius, args.ransac_hyp, args.ransac_thr, args.seed) == ("previous", 1.0, 4096, 0.3, 0)
    for extra in (["--init", "icp"], ["--fpfh-radius", "0"], ["--fpfh-radius", "inf"], ["--ransac-hyp", "0"], ["--ransac-hyp", "1048577"],
                  ["--ransac-thr", "-1"], ["--ransac-thr", "nan"], ["--seed", "-1"], ["--seed", "4294967296"]):
        with pytest.raises(SystemExit):
            align.parse_args(["--root", "d", "--sequence", "3"] + extra)
