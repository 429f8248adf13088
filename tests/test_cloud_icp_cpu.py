"""CPU tier of the cloud-against-cloud operations (ops.cloud_index / ops.cloud_nearest / ops.icp_point_to_plane, dataset/align.py; DESIGN.md
4ab): the restatement on inputs computed by hand, the convergence facts on the scenes that let the GPU tier assert its bars, every argument
check ahead of the library, and the align command with the restatement in the op's place."""
import os

import numpy as np
import pytest
import torch

import cloud_icp_reference as R
from cmr_agent_amd import _lib, ops
from cmr_agent_amd.dataset import align


# ---- the restatement on hand-checked inputs ---------------------------------------------------------------------------------------------
def test_two_points_and_a_plane():
    # target rows on the plane z = 0 with normal (0, 0, 1); two source points above them
    target = np.float32([[0, 0, 0], [2, 0, 0], [0, 2, 0]])
    normals = np.float32([[0, 0, 1]] * 3)
    source = np.float32([[0.25, 0, 0.5], [2, 0.25, 0.25]])
    idx, d2, q = R.nearest(target, source, 1.0)
    assert idx.tolist() == [0, 1] and d2.tolist() == [0.3125, 0.125] and np.array_equal(q, source)
    t = R.pair_terms(source, target[idx], normals[idx])
    # r = n . (q - c) = 0.5, 0.25;  J = (q x n, n) = (qy, -qx, 0, 0, 0, 1)
    J = np.array([[0, -0.25, 0, 0, 0, 1], [0.25, -2, 0, 0, 0, 1]])
    r = np.array([0.5, 0.25])
    iu = np.triu_indices(6)
    for p in range(2):
        assert np.array_equal(t[p, :21], np.outer(J[p], J[p])[iu]) and np.array_equal(t[p, 21:27], J[p] * r[p]) and t[p, 27] == r[p] ** 2
    # Huber 0.25: the first pair (|r| = 0.5) weighs 0.25 / 0.5, the second (|r| = 0.25, not above) weighs 1
    h = R.pair_terms(source, target[idx], normals[idx], huber=0.25)
    assert np.array_equal(h[0], 0.5 * t[0]) and np.array_equal(h[1], t[1])
    # two pairs: status 2 and the start pose; the iteration still reports them
    out = R.icp(source, target, normals, None, 1.0, iters=3)
    assert out["status"] == 2 and out["iterations"] == 1 and out["pairs"] == 2 and np.array_equal(out["pose"], np.eye(4))
    assert out["rmse"] == np.sqrt((0.25 + 0.0625) / 2) and not out["trace"][1:].any()
    # a pure translation along the normal is found in one step when the plane is all there is to see: x = H^-1 (-g) on the seen subspace
    assert R.chol_solve(t.sum(0)[:21], -t.sum(0)[21:27]) is None                         # rank 3: v_x, v_y and omega_z are unseen
    assert np.allclose(R.expso3([0, 0, np.pi / 2]), [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    x = R.chol_solve(np.eye(6)[np.triu_indices(6)] * 4.0, np.arange(6.0))
    assert np.array_equal(x, np.arange(6.0) / 4.0)


def test_pose_is_applied_operation_by_operation():
    T = np.eye(4, dtype=np.float32)
    T[0, :] = [1.0, 2.0 ** -12, 0, 2.0 ** -24]
    p = np.float32([[1 + 2.0 ** -12, 1 + 2.0 ** -12, 0]])
    q = R.pose_apply32(T, p)
    prod = np.float32(np.float32(2.0 ** -12) * p[0, 1])                                   # 2^-12 + 2^-24: exact
    s = np.float32(p[0, 0] + prod)                                                       # rounds: the fused form would keep the tail
    assert q[0, 0] == np.float32(s + np.float32(2.0 ** -24)) and q[0, 1] == p[0, 1] and q[0, 2] == 0
    idx, d2, q2 = R.nearest(np.float32([[1, 1, 0]]), p, 1.0, T)
    assert idx.tolist() == [0] and np.array_equal(q2, q)
    assert d2[0] == np.float32(np.float32((q[0, 0] - 1) ** 2) + np.float32((q[0, 1] - 1) ** 2))


def test_ties_faces_and_queries_outside():
    # equal distances: the lowest row, whatever the order of the rows
    target = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, 0.5], [0, 0, -0.5]])
    idx, d2, _ = R.nearest(target, np.float32([[0, 0, 0]]), 1.0)
    assert idx.tolist() == [5] and d2.tolist() == [0.25]
    idx, _, _ = R.nearest(target[:5], np.float32([[0, 0, 0]]), 1.0)
    assert idx.tolist() == [0]
    idx, _, _ = R.nearest(target[:5][::-1], np.float32([[0, 0, 0]]), 1.0)
    assert idx.tolist() == [0]                                                           # now (0, 0, 1)
    idx, _, _ = R.nearest(np.concatenate([target[:5], target[:5]]), np.float32([[0, 0, 0]]), 1.0)
    assert idx.tolist() == [0]                                                           # duplicated rows: the first copy
    # the radius is inclusive, in float32 as stated; just beyond it there is no match
    idx, d2, _ = R.nearest(target[:1], np.float32([[0, 0, 0], [np.float32(-1e-7), 0, 0]]), 1.0)
    assert idx.tolist() == [0, -1] and d2[0] == 1.0 and np.isnan(d2[1])
    # a query on a cell face of a grid of cell 1 with the origin at the target's minimum has matches on either side at the radius
    lat = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [2, 1, 0]])
    idx, d2, _ = R.nearest(lat, np.float32([[1, 1, 0]]), 1.0)
    assert idx.tolist() == [1] and d2.tolist() == [1.0]
    idx, d2, _ = R.nearest(lat[[0, 2, 3, 4]], np.float32([[1, 1, 0]]), 1.0)
    assert idx.tolist() == [2]
    # queries outside the target's bounding box, near and far; non-finite queries; non-finite target rows
    q = np.float32([[-0.5, 0, 0], [-1.5, 0, 0], [2.75, 1, 0], [1e30, 0, 0], [-3e38, 3e38, 0], [np.nan, 0, 0], [0, np.inf, 0]])
    idx, d2, _ = R.nearest(lat, q, 1.0)
    assert idx.tolist() == [0, -1, 4, -1, -1, -1, -1] and d2[:3].tolist()[0] == 0.25 and np.isnan(d2[[1, 3, 4, 5, 6]]).all()
    holes = lat.copy()
    holes[0, 1] = np.nan
    assert R.nearest(holes, q[:1], 1.0)[0].tolist() == [-1]
    assert R.nearest(np.zeros((0, 3), np.float32), q, 1.0)[0].tolist() == [-1] * 7
    assert R.nearest(lat, np.zeros((0, 3), np.float32), 1.0)[0].shape == (0,)


def test_slab_search_is_the_full_brute_force():
    case = R.pair_case()
    q = case["other"][::9]
    pose = R.pose_matrix(*R.TRUE_POSES[2]).astype(np.float32)
    idx, d2, qq = R.nearest(case["target"], q, 0.5, pose)
    c = case["target"]
    d = c[None, :, :] - qq[:, None, :]
    full = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    ok = full <= np.float32(0.25)
    best = np.where(ok, full, np.float32(np.inf)).min(1)
    want = np.where(ok.any(1), np.where(ok & (full == best[:, None]), np.arange(c.shape[0])[None, :], c.shape[0]).min(1), -1)
    assert np.array_equal(idx, want) and np.array_equal(d2[want >= 0], best[want >= 0]) and (want >= 0).sum() > 300 and (want < 0).any()


# ---- the scenes carry what the GPU tier's bars assume -----------------------------------------------------------------------------------
def test_scene_pair():
    case = R.pair_case()
    assert case["target"].shape == (4489, 3) and case["other"].shape == (4581, 3) and case["normals"].dtype == np.float32
    assert int((~case["normals"].any(1)).sum()) == 42


@pytest.mark.parametrize("max_dist", R.MAX_DISTS)
@pytest.mark.parametrize("k", range(3))
def test_convergence_facts(k, max_dist):
    """What a float64 loop does on the twelve cases: the GPU tier's bars (1e-5 rad and m on the same cloud; 10 % of the restatement's own
    error and +-2 iterations on the other) rest on these."""
    same, other = R.loop_case("same", k, max_dist), R.loop_case("other", k, max_dist)
    rs, ro = same["ref"], other["ref"]
    es, eo = R.pose_error(rs["pose"], same["truth"]), R.pose_error(ro["pose"], other["truth"])
    conds = [np.linalg.cond(R.full_matrix(r["system"][r["iterations"] - 1][:21])) for r in (rs, ro)]
    print("pose %d max_dist %.1f: same %d iterations, %.2e rad %.2e m, cond %.0f;  other %d iterations, %.2e rad %.2e m, cond %.0f" % (
        k, max_dist, rs["iterations"], es[0], es[1], conds[0], ro["iterations"], eo[0], eo[1], conds[1]))
    assert rs["status"] == 0 and 5 <= rs["iterations"] <= 8 and es[0] <= 1e-7 and es[1] <= 1e-6 and rs["pairs"] == 4447
    assert ro["status"] == 0 and 10 <= ro["iterations"] <= 19 and 7.5e-4 <= eo[0] <= 9.5e-4 and 0.8e-3 <= eo[1] <= 1.8e-3
    assert max(conds) <= 80
    # 10 % of the other cloud's error is far above what a step below the tolerances moves the pose by
    assert 0.1 * eo[0] > 50 * 1e-6 and 0.1 * eo[1] > 50 * 1e-6


def test_without_huber_the_other_cloud_does_not_settle():
    L = R.loop_case("other", 0, 1.0)
    case = R.pair_case()
    out = R.icp(L["source"], case["target"], case["normals"], None, 1.0, 0.0, 12)
    assert out["status"] == 1 and out["iterations"] == 12 and out["trace"][-1, 2:].max() > 1e-6


# ---- argument checks: every one raises before the library is reached --------------------------------------------------------------------
def _touched(*a, **k):
    raise AssertionError("the library was reached")


def _index(n=8, cell=1.0):
    return ops.CloudIndex(torch.zeros((n, 4)), torch.zeros((n,), dtype=torch.int64), torch.zeros((n,), dtype=torch.int64), (0.0, 0.0, 0.0), cell, n, n)


def test_argument_checks(monkeypatch):
    monkeypatch.setattr(_lib, "load", _touched)
    monkeypatch.setattr(_lib, "call", _touched)
    p = torch.zeros((8, 3))
    bad_points = (torch.zeros((8, 2)), torch.zeros((8,)), torch.zeros((2, 8, 3)), torch.zeros((8, 3), dtype=torch.float64), None,
                  np.zeros((8, 3), np.float32))
    bad_scalars = (0.0, -0.1, float("inf"), float("nan"), 1e-50, 1e39)
    # cloud_index
    for bad in bad_points:
        with pytest.raises(ValueError, match="points must be a float32"):
            ops.cloud_index(bad, 1.0)
    for bad in bad_scalars:
        with pytest.raises(ValueError, match="cell must be a finite number > 0"):
            ops.cloud_index(p, bad)
    with pytest.raises(ValueError, match="device tensor"):
        ops.cloud_index(p, 1.0)
    # cloud_nearest
    for bad in (None, (p, p), p):
        with pytest.raises(ValueError, match="index must be a CloudIndex"):
            ops.cloud_nearest(bad, p)
    for bad in bad_scalars:
        with pytest.raises(ValueError, match="max_dist must be a finite number > 0"):
            ops.cloud_nearest(_index(), p, bad)
    for bad in (1.5, 1.0000001):
        with pytest.raises(ValueError, match="exceeds the index's cell"):
            ops.cloud_nearest(_index(), p, bad)
    for bad in bad_points:
        with pytest.raises(ValueError, match="queries must be a float32"):
            ops.cloud_nearest(_index(), bad)
    with pytest.raises(ValueError, match="device tensor"):
        ops.cloud_nearest(_index(), p, 0.5)
    # icp_point_to_plane
    icp = ops.icp_point_to_plane
    for bad in bad_scalars:
        with pytest.raises(ValueError, match="max_dist must be a finite number > 0"):
            icp(p, p, p, max_dist=bad)
    for name in ("huber", "tol_rot", "tol_trans"):
        for bad in (-0.1, float("inf"), float("nan"), 1e39, "x", None):
            with pytest.raises(ValueError, match=name + " must be a finite number >= 0"):
                icp(p, p, p, **{name: bad})
    for bad in (-1, 1001, 2.5, True, None, float("nan")):
        with pytest.raises(ValueError, match="iters must be an integer"):
            icp(p, p, p, iters=bad)
    with pytest.raises(ValueError, match="index must be a CloudIndex"):
        icp(p, p, p, index=(p, p))
    with pytest.raises(ValueError, match="exceeds the index's cell"):
        icp(p, p, p, max_dist=1.0, index=_index(cell=0.5))
    with pytest.raises(ValueError, match="give the target cloud or its index"):
        icp(p, None, p)
    for bad in bad_points:
        with pytest.raises(ValueError, match="source must be a float32"):
            icp(bad, p, p)
    with pytest.raises(ValueError, match="device tensor"):
        icp(p, p, p)


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
    icp = ops.icp_point_to_plane
    for bad in (torch.zeros((8, 2)), torch.zeros((8,)), torch.zeros((8, 3), dtype=torch.float64), None, np.zeros((8, 3), np.float32)):
        with pytest.raises(ValueError, match="target_normals must be a float32"):
            icp(p, p, bad)
        if bad is not None:
            with pytest.raises(ValueError, match="target must be a float32"):
                icp(p, bad, p)
    with pytest.raises(ValueError, match="the target has 8 rows, target_normals 7"):
        icp(p, p, p[:7])
    with pytest.raises(ValueError, match="target_normals 8, the index 9"):
        icp(p, None, p, index=_index(9))
    with pytest.raises(ValueError, match="the target has 7 rows"):
        icp(p, p[:7], p, index=_index(8))
    for bad in (torch.eye(3), torch.eye(4, dtype=torch.float64), np.eye(4, dtype=np.float32), torch.zeros((1, 4, 4))):
        with pytest.raises(ValueError, match="pose must be a float32 \\[4, 4\\]"):
            icp(p, p, p, pose=bad)
        with pytest.raises(ValueError, match="pose must be a float32 \\[4, 4\\]"):
            ops.cloud_nearest(_index(), p, pose=bad)
    # empty inputs: no launch, no error
    e = icp(p[:0], p, p, iters=4, want_system=True)
    assert e.status == 2 and e.iterations == 0 and e.pairs == 0 and torch.equal(e.pose, torch.eye(4)) and e.trace.shape == (4, 4)
    assert e.system.shape == (4, 28) and not e.trace.any()
    e = icp(p, p[:0], p[:0], pose=2 * torch.eye(4))
    assert e.status == 2 and torch.equal(e.pose, 2 * torch.eye(4)) and e.system is None
    n = ops.cloud_nearest(_index(0), p)
    assert n.idx.tolist() == [-1] * 8 and n.dist2.isnan().all()
    n = ops.cloud_nearest(_index(), p[:0])
    assert n.idx.shape == (0,) and n.idx.dtype == torch.int32


def test_header_and_work_model_know_the_entry_points():
    from cmr_agent_amd.utils import workmodel
    protos = _lib.parse_header()
    src = open(workmodel.__file__).read()
    for name in ("cmr_cloud_gather4_f32", "cmr_cloud_nearest_f32", "cmr_icp_point_to_plane_f32", "cmr_icp_point_to_plane_workspace_bytes"):
        assert name in protos, name
        assert name.endswith("_bytes") or name in src
    assert protos["cmr_cloud_nearest_f32"][2] == ["queries", "ld", "M", "pose", "points4", "keys_sorted", "order", "kept", "ox", "oy", "oz",
                                                  "cell", "max_dist", "idx", "d2", "stream"]
    fl, by = workmodel.WORK["cmr_icp_point_to_plane_f32"](dict(M=1000, kept=500, iters=3))
    assert fl > 0 and by == 3 * (1000 * 24 + 500 * 32)
    assert _lib.load().cmr_icp_point_to_plane_workspace_bytes(0) == 0
    a, b = (_lib.load().cmr_icp_point_to_plane_workspace_bytes(m) for m in (32, 33))
    assert b - a == 28 * 8                                                               # one more slice: its 28 sums (the counts share a 16-byte line)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prep = open(os.path.join(root, "cmr_agent_amd", "csrc", "cloud_prepare.hip")).read()
    assert '#include "cmr_cloud_grid.h"' in prep and "axis_cells(float" not in prep and "pack_key(int64_t" not in prep


# ---- align.py ---------------------------------------------------------------------------------------------------------------------------
def test_align_registers_consecutive_frames_and_chains_the_poses(tmp_path, monkeypatch, capsys):
    """The file layer with the restatement in the op's place: no GPU."""
    calls = []

    def stand_in(source, target, target_normals, pose=None, **kw):
        calls.append(None if pose is None else pose.clone())
        return R.ops_icp_point_to_plane(source, target, target_normals, pose, **kw)

    monkeypatch.setattr(ops, "icp_point_to_plane", stand_in)
    truths = [R.pose_matrix((0.0, 0.0, 0.02), (0.3, 0.02, 0.0)), R.pose_matrix((0.0, 0.005, 0.025), (0.32, 0.0, 0.01))]
    root = str(tmp_path)
    R.write_frames(root, R.chained_frames(truths))
    out = str(tmp_path / "poses.txt")
    argv = ["--root", root, "--data-velodyne", "vel", "--sequence", "9", "--huber", "0", "--out", out]
    align.main(argv, device="cpu")
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2 and lines[0].startswith("pair 3 4: pairs ") and lines[1].startswith("pair 4 5: pairs ")
    words = lines[0].split()
    assert words[3:5] == ["pairs", words[4]] and words[5] == "rmse" and words[7] == "iterations" and words[9:11] == ["status", "0"]
    assert words[11] == "t" and words[15] == "r" and len(words) == 17
    assert [float(w) for w in words[12:15]] == [0.3, 0.02, 0.0] and abs(float(words[16]) - np.degrees(0.02)) < 1e-4
    # the first pair starts from the identity (None), the second from the first pair's result
    assert calls[0] is None and R.pose_error(calls[1].numpy(), truths[0])[1] < 1e-5
    chain = np.loadtxt(out)
    assert chain.shape == (3, 12) and np.array_equal(chain[0], np.eye(4)[:3].reshape(-1))
    assert np.abs(chain[1].reshape(3, 4) - truths[0][:3]).max() < 1e-5
    assert np.abs(chain[2].reshape(3, 4) - (truths[0] @ truths[1])[:3]).max() < 1e-5
    # --frames A:B is half open; one frame is no pair
    align.main(argv[:-2] + ["--frames", "4:6"], device="cpu")
    assert [ln.split(":")[0] for ln in capsys.readouterr().out.splitlines()] == ["pair 4 5"]
    align.main(argv[:-2] + ["--frames", ":4", "--out", out], device="cpu")
    assert capsys.readouterr().out == "" and np.loadtxt(out).shape == (12,)
    kw = {}
    monkeypatch.setattr(ops, "icp_point_to_plane", lambda s, t, n, pose=None, **k: kw.update(k) or R.ops_icp_point_to_plane(s, t, n, pose, **k))
    align.main(argv[:-4] + ["--frames", "3:5", "--max-dist", "0.5", "--huber", "0.2", "--iters", "7"], device="cpu")
    assert kw == dict(max_dist=0.5, huber=0.2, iters=7)


def test_align_flag_rules(tmp_path, capsys):
    root = str(tmp_path)
    folder = R.write_frames(root, [f[:4] for f in R.chained_frames([np.eye(4)])])
    base = ["--root", root, "--data-velodyne", "vel", "--sequence", "9"]
    with pytest.raises(SystemExit):
        align.main(base, device="cpu")                                                   # [4, n] files: no normals
    err = capsys.readouterr().err
    assert "no normals" in err and "cmr_agent_amd.dataset.prepare" in err
    for extra in (["--frames", "5"], ["--frames", "6:2"], ["--frames", "a:b"], ["--max-dist", "0"], ["--max-dist", "nan"], ["--huber", "-1"],
                  ["--iters", "1001"], ["--iters", "-1"], ["--sequence", "100"]):
        with pytest.raises(SystemExit):
            align.main(base[:4] + (extra if extra[0] == "--sequence" else ["--sequence", "9"] + extra), device="cpu")
    with pytest.raises(SystemExit):
        align.main(["--root", root, "--data-velodyne", "vel"])                           # --sequence is required
    with pytest.raises(SystemExit):
        align.main(base[:4] + ["--sequence", "8"], device="cpu")                         # no such folder
    assert "prepare" in capsys.readouterr().err
    os.remove(os.path.join(folder, "000003.npy"))
    np.save(os.path.join(folder, "000005.npy"), np.zeros((7, 5), np.float32))
    np.save(os.path.join(folder, "000007.npy"), np.zeros((7, 5), np.float32))
    with pytest.raises(SystemExit):
        align.main(base + ["--frames", "5:"], device="cpu")                              # frame 6 is missing
    assert "frame 6 is missing" in capsys.readouterr().err
    _, args = align.parse_args(["--root", "d", "--sequence", "3"])
    assert (args.frames, args.max_dist, args.huber, args.iters, args.out) == ((0, None), 1.0, 0.1, 30, None)
    assert args.data_velodyne == "data_odometry_velodyne_NWU/" and args.subdir == "voxel0.1-SNr0.6"
    with pytest.raises(ValueError, match="need float32 \\[7, n\\]"):
        align.read_prepared(os.path.join(folder, "000004.npy"))
