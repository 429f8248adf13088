"""GPU tier of pose-guided matching and match-based pose refinement (ops.guided_match / cmr_guided_match_f32, ops.pnp_refine /
cmr_pnp_refine_f32, MultiHeadModel.refine_pose_from_matches, Test_Geo.py --guided, Test_Agent.py --refine).

The yardstick is the float64 restatement in guided_reference.py.  The guided match is compared with the restatement run on the window
centres the DEVICE projected (its `proj` output), so a projection that lies 1e-5 from a half-integer is not a disagreement about which
feature is nearest; the projection itself is held to a bound derived from fp32 rounding.  Rows whose float64 decision hangs on less than
1e-5 (`near`; tests/test_guided_cpu.py caps them at 0.5 % of a sample's in-view rows) may resolve either way, nothing else may."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guided_reference as gref
import pnp_reference as pref
from cmr_agent_amd import ops
from cmr_agent_amd.environment import environment as env

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 50.0                      # scene scale of pnp_reference.planted: depths up to 50
F = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _match_args(sc, pose=None, mask=None):
    return (F(sc["pts"]), sc["pc"].to(DEV), sc["img"].to(DEV), (sc["mask"] if mask is None else mask).to(DEV),
            F(sc["start"] if pose is None else pose), F(sc["K"]))


_SCENES = {}


def _scene(name):
    if name not in _SCENES:
        _, kw, radii, max_dist = next(s for s in gref.MATCH_SCENES if s[0] == name)
        _SCENES[name] = (gref.scene(**kw), max_dist)
    return _SCENES[name]


# ---- guided match ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1, 4, 8])
@pytest.mark.parametrize("name", [s[0] for s in gref.MATCH_SCENES])
def test_guided_match_against_float64(name, radius):
    sc, max_dist = _scene(name)
    B, _, N = sc["pts"].shape
    h, w = sc["img"].shape[1:3]
    idx, keep, counts, dist, proj = ops.guided_match(*_match_args(sc), radius, max_dist=max_dist, gt_xy=sc["gt_xy"].to(DEV), thr=3.0,
                                                     want_dist=True, want_proj=True)
    idx, keep, dist = idx.view(B, N).cpu().long(), keep.view(B, N).cpu(), dist.view(B, N).cpu().double()
    counts, proj = counts.cpu().tolist(), proj.cpu().double()
    ref = gref.guided_match(sc["pts"], sc["pc"], sc["img"], sc["mask"], sc["start"], sc["K"], radius, max_dist=max_dist, gt_xy=sc["gt_xy"],
                            centres=proj)
    for b in range(B):
        # the projection: 64 * 2^-24 * (f (|x| + |t|) / z + w) px per row -- about a dozen fp32 roundings, each relative to the largest
        # intermediate
        u, v, z = gref.project(sc["pts"][b], sc["start"][b], sc["K"][b])
        front = z > 0
        bound = 64 * 2.0 ** -24 * (sc["K"][b][0, 0] * (np.linalg.norm(sc["pts"][b], axis=0) + np.linalg.norm(sc["start"][b][:3, 3])) / np.abs(z) + w)
        du, dv = np.abs(proj[b, 0].numpy() - u)[front], np.abs(proj[b, 1].numpy() - v)[front]
        print(name, "r", radius, "sample", b, "proj max deviation", du.max(), dv.max(), "of bound (max ratio)", (np.maximum(du, dv) / bound[front]).max())
        assert (du <= bound[front]).all() and (dv <= bound[front]).all()
        assert np.isnan(proj[b, 0].numpy()[~front]).all()
        e = ref[b]
        near, view = e["near"], e["view"]
        n_near = int(near.sum())
        rows = torch.nonzero(view).flatten()
        chosen = e["dist_of"](rows, idx[b][rows].clamp(min=0))
        print("   counts", counts[b], "restatement", e["counts"], "near", n_near, "idx differ", int((idx[b] != e["idx"]).sum()),
              "max |dist - float64|", float((dist[b][rows] - chosen).abs().max()) if rows.numel() else 0.0,
              "max chosen - window min", float((chosen - e["wmin"][rows]).max()) if rows.numel() else 0.0)
        assert n_near <= gref.CAP * e["counts"][1]                                       # the excluded set stays under the cap on the device's centres too
        assert torch.equal(idx[b] >= 0, view)                                            # in view: decided on the same floats, exactly
        assert torch.isnan(dist[b][~view]).all() and not bool(keep[b][~view].any())
        assert torch.equal(idx[b][~near], e["idx"][~near])
        assert float((dist[b][rows] - chosen).abs().max()) <= 1e-5
        assert float((chosen - e["wmin"][rows]).abs().max()) <= 1e-5                     # every row: as good as the float64 minimum
        assert torch.equal(keep[b][~near], e["keep"][~near])
        assert counts[b][0] == e["counts"][0] and counts[b][1] == e["counts"][1]
        assert abs(counts[b][2] - e["counts"][2]) <= n_near and abs(counts[b][3] - e["counts"][3]) <= n_near
        assert counts[b][2] == int(keep[b].sum())


def test_radius_zero_returns_the_rounded_projection():
    sc, _ = _scene("random_88x304")
    B, _, N = sc["pts"].shape
    h, w = sc["img"].shape[1:3]
    idx, keep, counts, _, proj = ops.guided_match(*_match_args(sc), 0, want_proj=True)
    idx, proj = idx.view(B, N).cpu().long(), proj.cpu().double()
    cx, cy = torch.from_numpy(np.rint(proj[:, 0].numpy())), torch.from_numpy(np.rint(proj[:, 1].numpy()))
    inside = (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
    assert int(inside.sum()) > N and torch.equal(idx >= 0, inside)
    assert torch.equal(idx[inside], (cy * w + cx)[inside].long())
    assert counts[:, 1].cpu().tolist() == inside.sum(1).tolist() == keep.view(B, N).sum(1).cpu().tolist()


def _tiny():
    h, w = 8, 10
    img = torch.nn.functional.normalize(torch.arange(h * w * 64, dtype=torch.float64).reshape(1, h, w, 64).sin(), dim=-1).float()
    # depth 1, K = identity: the points project to (x, y) themselves.  Centres (3, 4), (0, 0) (the window straddles two edges), (11, 4)
    # (two columns outside, the best pixel on the border), (13, 4) (farther than r = 2 outside), behind the camera, a NaN coordinate
    pts = torch.tensor([[[3.2, 0.4, 11.0, 13.0, 3.0, math.nan], [3.7, -0.3, 4.0, 4.0, 4.0, 1.0], [1.0, 1.0, 1.0, 1.0, -1.0, 1.0]]])
    N = pts.shape[2]
    pc = img[0, 4, 3][None].repeat(N, 1)
    pc[1] = img[0, 0, 0]
    pc[2] = img[0, 4, 9]
    return pts.to(DEV), pc.contiguous().to(DEV), img.to(DEV), torch.eye(4, device=DEV)[None].contiguous(), torch.eye(3, device=DEV)[None].contiguous(), w


def test_window_edges_and_rows_out_of_view():
    pts, pc, img, pose, K, w = _tiny()
    N = pts.shape[2]
    m = torch.ones(1, N, dtype=torch.bool, device=DEV)
    idx, keep, counts, dist, proj = ops.guided_match(pts, pc, img, m, pose, K, 2, want_dist=True, want_proj=True)
    assert idx.tolist() == [4 * w + 3, 0, 4 * w + 9, -1, -1, -1]
    assert keep.tolist() == [True, True, True, False, False, False]
    assert counts.tolist() == [[6, 3, 3, 0]]
    assert torch.isnan(dist[3:]).all() and float(dist[:3].max()) <= 1e-6
    assert proj[0, :, 3].tolist() == [13.0, 4.0] and torch.isnan(proj[0, :, 4:]).all()       # in front but out of view: the numbers; behind / NaN: NaN
    idx0 = ops.guided_match(pts, pc, img, m, pose, K, 0)[0]
    assert idx0.tolist() == [4 * w + 3, 0, -1, -1, -1, -1]                                   # 3.7 rounds to 4, -0.3 to 0, 11 is outside at r = 0
    # duplicate pixel features inside a window resolve to the lowest p
    img2 = img.clone()
    img2[0, 3, 2] = img2[0, 4, 3]
    assert int(ops.guided_match(pts, pc, img2, m, pose, K, 2)[0][0]) == 3 * w + 2
    # the distance bound drops the match from keep, not from idx
    idx, keep, counts, _, _ = ops.guided_match(pts, (pc + 0.5).contiguous(), img, m, pose, K, 2, max_dist=0.1)
    assert counts.tolist() == [[6, 3, 0, 0]] and not bool(keep.any()) and bool((idx[:3] >= 0).all())
    # gt_xy: the inlier count
    gt = torch.tensor([[[3.0, 5.0, math.nan, 0, 0, 0], [4.0, 5.0, 4.0, 0, 0, 0]]], device=DEV)
    assert ops.guided_match(pts, pc, img, m, pose, K, 2, gt_xy=gt, thr=3.0)[2].tolist() == [[6, 3, 3, 1]]


def test_empty_selection_and_mask_dtypes():
    sc, max_dist = _scene("random_88x304")
    B, _, N = sc["pts"].shape
    a = _match_args(sc)
    idx, keep, counts, dist, proj = ops.guided_match(*a[:3], torch.zeros(B, N, dtype=torch.bool, device=DEV), *a[4:], 4, want_dist=True,
                                                     want_proj=True)
    assert bool((idx == -1).all()) and not bool(keep.any()) and counts.tolist() == [[0, 0, 0, 0]] * B
    assert torch.isnan(dist).all() and torch.isnan(proj).all()
    mb = torch.rand(B, N, generator=torch.Generator().manual_seed(4)) < 0.4
    outs = [ops.guided_match(*a[:3], m.to(DEV), *a[4:], 4, max_dist=max_dist, want_dist=True, want_proj=True)
            for m in (mb, mb.to(torch.uint8), mb.long() * 7)]
    for o in outs[1:]:
        for x, y in zip(o, outs[0]):
            assert torch.equal(_bits(x), _bits(y))
    assert outs[0][2][:, 0].tolist() == mb.sum(1).tolist()
    assert bool((outs[0][0].view(B, N).cpu()[~mb] == -1).all())


# ---- refinement ------------------------------------------------------------------------------------------------------------------------
def _refine_args(s, mask=None):
    B, _, N = s["pts"].shape
    m = torch.ones(B, N, dtype=torch.bool, device=DEV) if mask is None else mask
    return F(s["pts"]), F(s["uv"]), m, F(s["K"]), F(s["pose_in"])


def _close(pose, want, tol=1e-4):
    pose, want = np.asarray(pose, np.float64), np.asarray(want, np.float64)
    return pref.rotation_error_deg(pose[:3, :3], want[:3, :3]), float(np.linalg.norm(pose[:3, 3] - want[:3, 3]))


@pytest.mark.parametrize("frac", [0.0, 0.3])
@pytest.mark.parametrize("N", gref.REFINE_SIZES)
def test_refine_against_float64(N, frac):
    B = 2
    s = gref.refine_scene(B, N, seed=300 + N % 1000 + int(10 * frac), outlier_frac=frac)
    pose, inl, status = ops.pnp_refine(*_refine_args(s), thr=1.0, iters=10)
    assert bool(torch.isfinite(pose).all())
    pose, inl, status = pose.double().cpu().numpy(), inl.tolist(), status.tolist()
    for b in range(B):
        r = gref.refine(s["pts"][b], s["uv"][b], np.ones(N), s["K"][b], s["pose_in"][b], thr=1.0, iters=10)
        er, et = _close(pose[b], r["pose"])
        print("N", N, "outliers", frac, "sample", b, "status", status[b], r["status"], "inliers", inl[b], r["inliers"], "pose deviation", er, "deg", et)
        assert status[b] == r["status"] == 0 and inl[b] == r["inliers"]
        assert er < 1e-4 and et < 1e-4 * SCALE
        assert np.array_equal(pose[b, 3], [0, 0, 0, 1])


def test_refine_status_codes_and_zero_iterations():
    N = 64
    s = gref.refine_scene(2, N, seed=42)
    m = torch.zeros(2, N, dtype=torch.uint8, device=DEV)
    m[1, [3, 17, 40]] = 1                                              # sample 0: none, sample 1: three rows
    a = _refine_args(s, m)
    pose, inl, status = ops.pnp_refine(*a)
    assert status.tolist() == [1, 1] and inl.tolist() == [0, 3] and torch.equal(pose, a[4])
    pose, inl, status = ops.pnp_refine(*_refine_args(s), iters=0)
    assert status.tolist() == [0, 0] and inl.tolist() == [N, N] and torch.equal(pose, a[4])
    # every row on one line: the normal matrix is singular, the first factorisation fails
    pts, uv, K, P = gref.collinear_case(N)
    pose, inl, status = ops.pnp_refine(F(pts[None]), F(uv[None]), torch.ones(1, N, dtype=torch.bool, device=DEV), F(K[None]), F(P[None]))
    assert status.tolist() == [2] and inl.tolist() == [N] and torch.equal(pose, F(P[None]))
    # non-finite correspondences: never a NaN in the pose
    bad = F(s["uv"]).clone()
    bad[0, 0, 5] = math.nan
    bad[1, 1, 7] = math.inf
    pose, inl, status = ops.pnp_refine(a[0], bad, torch.ones(2, N, dtype=torch.bool, device=DEV), a[3], a[4])
    assert bool(torch.isfinite(pose).all()) and status.tolist() == [0, 0] and inl.tolist() == [N - 1, N - 1]


def test_refining_the_optimum_changes_nothing():
    N = 4097
    s = gref.refine_scene(2, N, seed=43, outlier_frac=0.3)
    a = _refine_args(s)
    first, _, st1 = ops.pnp_refine(*a, thr=1.0, iters=10)
    second, _, st2 = ops.pnp_refine(*a[:4], first, thr=1.0, iters=10)
    assert st1.tolist() == [0, 0] and st2.tolist() == [0, 0]
    for b in range(2):
        er, et = _close(second[b].double().cpu().numpy(), first[b].double().cpu().numpy())
        print("second call moved the pose by", er, "deg", et)
        assert er < 1e-4 and et < 1e-4 * SCALE


@pytest.mark.parametrize("seed", gref.AGREE_SEEDS)
def test_refine_agrees_with_pnp_ransac_refinement(seed):
    """Started from the unrefined RANSAC winner with the same thr, ops.pnp_refine takes cmr_pnp_ransac_f32's own refinement steps: the
    same working set wherever the winner has no residual within 1e-3 px of thr (the fp32 starts differ by rounding only)."""
    B, N, n_hyp = gref.AGREE_SHAPE
    s = pref.planted(B, N, 88, 304, seed=seed, outlier_frac=0.3, noise=0.3)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    pts, uv, K = F(s["pts"]), F(s["uv"]), F(s["K"])
    m = torch.ones(B, N, dtype=torch.bool, device=DEV)
    p0, _, st0 = ops.pnp_ransac(pts, uv, m, K, n_hyp=n_hyp, thr=1.0, seed=5, refine_iters=0)
    p10, i10, st10 = ops.pnp_ransac(pts, uv, m, K, n_hyp=n_hyp, thr=1.0, seed=5, refine_iters=10)
    mine, imine, stm = ops.pnp_refine(pts, uv, m, K, p0, thr=1.0, iters=10)
    compared = 0
    for b in range(B):
        r = pref.pnp_ransac(f32(s["pts"][b]), f32(s["uv"][b]), np.ones(N), f32(s["K"][b]), n_hyp=n_hyp, thr=1.0, seed=5, refine_iters=0, b=b)
        same = r["status"] == 0 and max(_close(p0[b].double().cpu().numpy(), r["pose"])) < 1e-4
        if not (same and r["best_near"] == 0):
            continue
        er, et = _close(mine[b].double().cpu().numpy(), p10[b].double().cpu().numpy())
        print("seed", seed, "sample", b, "pnp_refine vs pnp_ransac(refine_iters=10):", er, "deg", et, "inliers", int(imine[b]), int(i10[b]))
        assert int(stm[b]) == 0 and int(st10[b]) == 0
        assert er < 2e-4 and et < 2e-4 * SCALE
        compared += 1
    assert 2 * compared >= B


# ---- determinism, batch independence, graph replay ---------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.uint8) if t.dtype == torch.bool else t.contiguous().view(torch.int32)


def _both_calls(B=3, N=4096, seed=221):
    sc = gref.scene(B, N, 40, 128, seed)
    ma = _match_args(sc, mask=torch.rand(B, N, generator=torch.Generator().manual_seed(6)) < 0.7)
    gt = sc["gt_xy"].to(DEV)
    gm = lambda a: ops.guided_match(*a, 4, max_dist=gref.MAX_DIST, gt_xy=gt, want_dist=True, want_proj=True)
    s = gref.refine_scene(B, N, seed=seed + 1, outlier_frac=0.3)
    ra = _refine_args(s, (torch.rand(B, N, generator=torch.Generator().manual_seed(7)) < 0.8).to(DEV))
    rf = lambda a: ops.pnp_refine(*a, thr=1.0, iters=10)
    return (gm, ma), (rf, ra)


def test_two_calls_agree_bit_for_bit():
    for fn, args in _both_calls():
        for x, y in zip(fn(args), fn(args)):
            assert torch.equal(_bits(x), _bits(y))


def test_pnp_refine_sample_alone_equals_sample_in_batch():
    (_, _), (rf, args) = _both_calls()
    full = rf(args)
    assert full[2].tolist() == [0, 0, 0]
    for k in range(3):
        alone = rf(tuple(t[k:k + 1].contiguous() for t in args))
        for x, y in zip(alone, full):
            assert torch.equal(_bits(x[0]), _bits(y[k]))


def test_guided_match_sample_alone_equals_sample_in_batch():
    B, N = 3, 4096
    sc = gref.scene(B, N, 40, 128, 223)
    mask = torch.rand(B, N, generator=torch.Generator().manual_seed(8)) < 0.7
    a = _match_args(sc, mask=mask)
    gt = sc["gt_xy"].to(DEV)
    kw = dict(max_dist=gref.MAX_DIST, want_dist=True, want_proj=True)
    idx, keep, counts, dist, proj = ops.guided_match(*a, 4, gt_xy=gt, **kw)
    for k in range(B):
        one = (a[0][k:k + 1].contiguous(), a[1][k * N:(k + 1) * N].contiguous(), a[2][k:k + 1].contiguous(), a[3][k:k + 1].contiguous(),
               a[4][k:k + 1].contiguous(), a[5][k:k + 1].contiguous())
        i1, k1, c1, d1, p1 = ops.guided_match(*one, 4, gt_xy=gt[k:k + 1].contiguous(), **kw)
        assert torch.equal(i1, idx.view(B, N)[k]) and torch.equal(k1, keep.view(B, N)[k]) and torch.equal(c1[0], counts[k])
        assert torch.equal(_bits(d1), _bits(dist.view(B, N)[k])) and torch.equal(_bits(p1[0]), _bits(proj[k]))


def test_graph_replay_equals_eager():
    for fn, args in _both_calls(B=2, N=8192, seed=225):
        eager = fn(args)
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            fn(args)
        torch.cuda.current_stream().wait_stream(st)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = fn(args)
        for t in got:
            t.fill_(1) if t.dtype == torch.bool else t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(eager, got):
            assert torch.equal(_bits(x), _bits(y))


# ---- from_disentangled ---------------------------------------------------------------------------------------------------------------------
def test_from_disentangled_inverts_to_disentangled():
    """To 1e-5 on a cloud and poses of a few units (fp32: half an ulp at 8 .. 16 is 5e-7, a handful of roundings each way)."""
    g = torch.Generator().manual_seed(9)
    B, N = 3, 2048
    pcd = (torch.randn(B, 3, N, generator=g) * 3 + 1).to(DEV)
    P = torch.eye(4).repeat(B, 1, 1)
    for b in range(B):
        P[b, :3, :3] = torch.from_numpy(pref._rot(np.array([0.3, 1.0, -0.2]), 0.4 + b)).float()
        P[b, :3, 3] = torch.randn(3, generator=g) * 2
    P = P.to(DEV)
    D = env.to_disentangled(P.clone(), pcd)
    assert float((D - P).abs().max()) > 0.1
    back = env.from_disentangled(D.clone(), pcd)
    print("round trip max deviation", float((back - P).abs().max()))
    assert float((back - P).abs().max()) <= 1e-5
    data = {"pc": pcd}
    D = env.to_disentangled(P.clone(), pcd, data=data)
    assert float((env.from_disentangled(D, pcd, data=data) - P).abs().max()) <= 1e-5


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def _model(N):
    from cmr_agent_amd.models import MultiHeadModel
    from cmr_agent_amd.config import KittiConfiguration
    return MultiHeadModel(KittiConfiguration(num_pt=N, device=torch.device(DEV)))


def _data(pts, K, P, pc_rows, img_nhwc):
    B, _, N = pts.shape
    cam = np.einsum("bij,bjn->bin", P[:, :3, :3], pts) + P[:, :3, 3:4]
    h, w = img_nhwc.shape[1:3]
    return {"pc": F(pts), "K": F(K), "P": F(P), "pc_in_cam_space": F(cam),
            "pc_geo_feat": pc_rows.view(B, N, 64).permute(0, 2, 1).contiguous().to(DEV),
            "img_geo_feat": img_nhwc.permute(0, 3, 1, 2).contiguous().to(DEV), "pc_overlap_pred": torch.ones(B, N, dtype=torch.bool, device=DEV)}, cam


@pytest.mark.parametrize("seed", [201, 202, 203])
def test_refine_pose_from_matches_follows_the_restatement(seed):
    B, N, h, w = 2, 4096, 40, 128
    sc = gref.scene(B, N, h, w, seed)
    want, _ = gref.refine_rounds(sc)
    wr, wt = gref.pose_errors(want, sc["P"])
    data, _ = _data(sc["pts"], sc["K"], sc["P"], sc["pc"], sc["img"])
    _model(N).refine_pose_from_matches(data, pose=F(sc["start"]), radii=[r for r, _ in gref.ROUNDS], thrs=[t for _, t in gref.ROUNDS],
                                       max_dist=gref.MAX_DIST)
    assert data["refined_status"].tolist() == [0] * B and data["refined_pose"].shape == (B, 4, 4)
    assert data["guided_counts"].shape == (len(gref.ROUNDS), B, 4) and data["guided_counts"].dtype == torch.int32
    gr, gt = gref.pose_errors(data["refined_pose"].double().cpu().numpy(), sc["P"])
    r0, t0 = gref.pose_errors(sc["start"], sc["P"])
    print("seed", seed, "start", r0, t0, "device", gr, gt, "restatement", wr, wt, "inliers", data["refined_inliers"].tolist(),
          "counts", data["guided_counts"].tolist())
    for b in range(B):
        assert gr[b] <= 2 * wr[b] + 1e-3 and gt[b] <= 2 * wt[b] + 1e-3


def test_refine_pose_from_matches_after_pnp():
    """The scene of test_pnp_gpu.py::test_pose_from_matches_on_planted_features (point n carries the pixel feature of its true rounded
    pixel): the refined pose meets the quantisation bounds that test derives for the PnP pose -- rotation <= q / f, translation <= q z_max /
    f, mean reprojection deviation <= q, q = 0.5 sqrt(2) px."""
    B, N, h, w = 2, 4096, 40, 128
    s = pref.planted(B, N, h, w, seed=51)
    K = s["K"][0]
    pix = (np.round(s["uv"][:, 1]) * w + np.round(s["uv"][:, 0])).astype(np.int64)
    g = torch.Generator(device="cpu").manual_seed(52)
    img = torch.nn.functional.normalize(torch.randn(B, h * w, 64, generator=g, dtype=torch.float64), dim=-1).float()
    pcf = torch.gather(img, 1, torch.from_numpy(pix)[..., None].expand(B, N, 64))
    data, cam = _data(s["pts"], s["K"], s["P"], pcf.reshape(B * N, 64), img.view(B, h, w, 64))
    model = _model(N)
    ov = torch.ones(B, h, w, dtype=torch.bool, device=DEV)
    model.pose_from_matches(data, img_overlap=ov, n_hyp=64, thr=1.0)
    assert data["pnp_status"].tolist() == [0] * B
    model.refine_pose_from_matches(data, img_overlap=ov)
    assert data["refined_status"].tolist() == [0] * B
    q, foc = 0.5 * math.sqrt(2.0), K[0, 0]
    P = data["refined_pose"].double().cpu().numpy()
    rre, rte = gref.pose_errors(P, s["P"])
    print("pnp", gref.pose_errors(data["pnp_pose"].double().cpu().numpy(), s["P"]), "refined", rre, rte, "inliers", data["pnp_inliers"].tolist(),
          data["refined_inliers"].tolist())
    assert max(rre) <= math.degrees(q / foc) and max(rte) <= q * cam[:, 2].max() / foc
    for b in range(B):
        pr = K @ (P[b, :3, :3] @ s["pts"][b] + P[b, :3, 3:4])
        assert np.hypot(pr[0] / pr[2] - s["uv"][b, 0], pr[1] / pr[2] - s["uv"][b, 1]).mean() <= q


# ---- the scripts ---------------------------------------------------------------------------------------------------------------------------------
def _run(script, *flags):
    cmd = [sys.executable, os.path.join(ROOT, script), "--pairs", "2", "--img", "160x512", "--num-pt", "4096", *flags]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    return res.stdout.strip().splitlines()


def _check_refined_lines(lines, pair_width):
    """`refined <RTE> <RRE>` right after each pair's `RTE RRE` line; the closing block again with the prefix `Refined `."""
    ref = [i for i, l in enumerate(lines) if l.startswith("refined ")]
    assert len(ref) == 2, lines
    for i in ref:
        assert len(lines[i].split()) == 3 and all(float(v) >= 0 for v in lines[i].split()[1:])
        assert len(lines[i - 1].split()) == pair_width and all(float(v) >= 0 for v in lines[i - 1].split())
    rec = [i for i, l in enumerate(lines) if l.startswith("Registration Recall:")]
    rrec = [i for i, l in enumerate(lines) if l.startswith("Refined Registration Recall:")]
    assert len(rec) == 1 and len(rrec) == 1 and rrec[0] > rec[0] > max(ref)
    assert all(not l.startswith("Refined") for l in lines[:rrec[0]])
    recall = float(lines[rrec[0]].split(":")[1])
    tail = lines[rrec[0] + 1:]
    if recall > 0:
        assert tail[0].startswith("Refined RTE Mean:") and "RTE Std:" in tail[0]
        assert tail[1].startswith("Refined RRE Mean:") and "RRE Std:" in tail[1] and len(tail) == 2
    else:
        assert tail == []


def test_test_geo_script_guided():
    lines = _run("Test_Geo.py", "--batch-size", "2", "--pnp", "--guided", "4,2")
    _check_refined_lines(lines, 2)
    plain = _run("Test_Geo.py", "--batch-size", "2", "--pnp")
    assert not any(l.startswith("refined") or l.startswith("Refined") for l in plain)


def test_test_agent_script_refine():
    lines = _run("Test_Agent.py", "--refine", "4,2")
    _check_refined_lines(lines, 2)
    plain = _run("Test_Agent.py")
    assert not any(l.startswith("refined") or l.startswith("Refined") for l in plain)
