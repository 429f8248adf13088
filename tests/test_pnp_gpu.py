"""GPU tier of PnP-RANSAC (ops.pnp_ransac / cmr_pnp_ransac_f32, MultiHeadModel.pose_from_matches, Test_Geo.py --pnp).

The kernel scores in fp32 with K[R|t] rounded to fp32, the restatement in pnp_reference.py in float64, so a per-hypothesis inlier count
may differ from the restatement's by the correspondences whose float64 residual lies within ALLOW px of the threshold, and nothing more."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pnp_reference as ref
from cmr_agent_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALLOW = 1e-3
SCALE = 50.0                      # scene scale of pnp_reference.planted: depths up to 50


def _dev(s, mask=None):
    B, _, N = s["pts"].shape
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    m = torch.ones(B, N, dtype=torch.bool, device=DEV) if mask is None else mask
    return f(s["pts"]), f(s["uv"]), m, f(s["K"])


def _errors(pose, P):
    pose = pose.double().cpu().numpy()
    return ([ref.rotation_error_deg(pose[b, :3, :3], P[b, :3, :3]) for b in range(len(P))],
            [float(np.linalg.norm(pose[b, :3, 3] - P[b, :3, 3])) for b in range(len(P))])


@pytest.mark.parametrize("N", [1024, 65536])
@pytest.mark.parametrize("kind", ["6dof", "yaw"])
@pytest.mark.parametrize("frac", [0.0, 0.3, 0.6, 0.8])
def test_planted_poses(N, kind, frac):
    B = 8
    s = ref.planted(B, N, 88, 304, seed=100 + N + int(10 * frac) + (kind == "yaw"), outlier_frac=frac, kind=kind)
    n_hyp = 8192 if frac >= 0.8 else 1024          # P(no all-inlier draw) = (1 - 0.2^4)^8192 ~ 2e-6 at 80 % outliers
    pose, inl, status = ops.pnp_ransac(*_dev(s), n_hyp=n_hyp, thr=1.0, seed=3)
    assert status.tolist() == [0] * B
    rre, rte = _errors(pose, s["P"])
    assert max(rre) < 0.01, rre
    assert max(rte) < 1e-3 * SCALE, rte
    assert bool(torch.isfinite(pose).all())
    assert (inl.cpu().numpy() >= s["inlier"].sum(1)).all()


def test_parity_with_the_float64_restatement():
    B, N, n_hyp, thr = 3, 2048, 256, 1.0
    s = ref.planted(B, N, 88, 304, seed=7, outlier_frac=0.4, noise=0.3)
    s["pts"], s["uv"], s["K"] = (s[k].astype(np.float32).astype(np.float64) for k in ("pts", "uv", "K"))
    g = np.random.default_rng(8)
    mask = g.random((B, N)) < 0.7
    pose, inl, status, hyp = ops.pnp_ransac(*_dev(s, torch.from_numpy(mask).to(DEV)), n_hyp=n_hyp, thr=thr, seed=11, refine_iters=10,
                                            want_hyp_inliers=True)
    pose, inl, status, hyp = pose.double().cpu().numpy(), inl.cpu().numpy(), status.cpu().numpy(), hyp.cpu().numpy()
    compared = 0
    for b in range(B):
        r = ref.pnp_ransac(s["pts"][b], s["uv"][b], mask[b], s["K"][b], n_hyp=n_hyp, thr=thr, seed=11, refine_iters=10, b=b,
                           allowance=ALLOW)
        assert status[b] == r["status"] == 0
        valid = r["hyp_inliers"] >= 0
        assert np.array_equal(hyp[b] >= 0, valid)
        diff = np.abs(hyp[b] - r["hyp_inliers"])
        assert (diff[valid] <= r["near"][valid]).all(), np.nonzero(diff > r["near"])
        # the selected hypothesis: the same whenever the restatement's margin exceeds the allowance
        order = np.argsort(-r["hyp_inliers"], kind="stable")
        best, second = order[0], order[1]
        gbest = int(np.argmax(hyp[b]))
        margin = r["hyp_inliers"][best] - r["hyp_inliers"][second]
        if margin > r["near"][best] + r["near"][second]:
            assert gbest == best == r["best"]
        # the output pose: within 1e-4 deg / 1e-4 x scale of the restatement's when the inlier set and the keep decision are unambiguous
        if gbest == r["best"] and r["best_near"] == 0 and r["refine_near"] == 0 and r["refine_margin"] != 0:
            assert ref.rotation_error_deg(pose[b, :3, :3], r["pose"][:3, :3]) < 1e-4
            assert np.linalg.norm(pose[b, :3, 3] - r["pose"][:3, 3]) < 1e-4 * SCALE
            assert inl[b] == r["inliers"]
            compared += 1
        assert inl[b] >= hyp[b][gbest]                                 # the refined pose is kept only with at least as many inliers
    assert compared >= 1


def test_too_few_correspondences_give_status_1():
    s = ref.planted(2, 64, 88, 304, seed=21)
    m = torch.zeros(2, 64, dtype=torch.uint8, device=DEV)
    m[1, [3, 17, 40]] = 1                                              # sample 0: none, sample 1: three
    pose, inl, status, hyp = ops.pnp_ransac(*_dev(s, m), n_hyp=64, want_hyp_inliers=True)
    assert status.tolist() == [1, 1] and inl.tolist() == [0, 0]
    assert torch.equal(pose, torch.eye(4, device=DEV).expand(2, 4, 4))
    assert bool((hyp == -1).all())


def test_degenerate_correspondences_give_status_2_and_no_nan():
    N = 256
    s = ref.planted(2, N, 88, 304, seed=22)
    pts = np.empty((2, 3, N))
    pts[0] = np.array([[1.5], [-2.0], [20.0]])                         # every point the same
    k = np.arange(N, dtype=np.float64)
    pts[1] = np.stack([k - 100, 2 * k - 50, 10 + k])                   # integers: exactly collinear in float32 and float64
    s["pts"] = pts
    pose, inl, status, hyp = ops.pnp_ransac(*_dev(s), n_hyp=512, want_hyp_inliers=True)
    assert status.tolist() == [2, 2] and inl.tolist() == [0, 0]
    assert torch.equal(pose, torch.eye(4, device=DEV).expand(2, 4, 4))
    assert bool((hyp == -1).all())


def test_deterministic_and_independent_of_the_batch():
    B, N = 8, 4096
    s = ref.planted(B, N, 88, 304, seed=31, outlier_frac=0.5, noise=0.2)
    args = _dev(s, (torch.rand(B, N, generator=torch.Generator().manual_seed(2)) < 0.6).to(DEV))
    kw = dict(n_hyp=512, thr=1.0, seed=9, want_hyp_inliers=True)
    a = ops.pnp_ransac(*args, **kw)
    b = ops.pnp_ransac(*args, **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # sample 0 alone == sample 0 of the batch
    alone = ops.pnp_ransac(*(t[:1].contiguous() for t in args), **kw)
    for x, y in zip(alone, a):
        assert torch.equal(x[0].view(torch.int32), y[0].view(torch.int32))
    # sample 5 with every other sample replaced: bit for bit the same
    s2 = ref.planted(B, N, 88, 304, seed=32, outlier_frac=0.2)
    other = list(_dev(s2, (torch.rand(B, N, generator=torch.Generator().manual_seed(3)) < 0.3).to(DEV)))
    for t, o in zip(args, other):
        o[5] = t[5]
    c = ops.pnp_ransac(*other, **kw)
    for x, y in zip(c, a):
        assert torch.equal(x[5].view(torch.int32), y[5].view(torch.int32))
    assert a[2].tolist() == [0] * B


def test_graph_replay_equals_eager():
    B, N = 4, 8192
    s = ref.planted(B, N, 88, 304, seed=41, outlier_frac=0.5)
    args = _dev(s)
    kw = dict(n_hyp=1024, thr=1.0, seed=1, want_hyp_inliers=True)
    eager = ops.pnp_ransac(*args, **kw)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ops.pnp_ransac(*args, **kw)
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ops.pnp_ransac(*args, **kw)
    for t in got:
        t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, got):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_pose_from_matches_on_planted_features():
    """Point n's geometric feature is the pixel feature at its true rounded pixel, so the matches are the rounded projections: each is
    within q = 0.5 * sqrt(2) px of the exact one.  A pose whose reprojections all stay within q of the exact ones can be rotated by at
    most q / f rad (f = focal length in px) and, for a point at depth z, moved by at most q z / f; that is the bound checked (with the
    scene's largest depth), together with the mean reprojection deviation itself."""
    from cmr_agent_amd.models import MultiHeadModel
    from cmr_agent_amd.config import KittiConfiguration
    B, N, h, w = 2, 4096, 40, 128
    s = ref.planted(B, N, h, w, seed=51)
    K = s["K"][0]
    cam = np.einsum("bij,bjn->bin", s["P"][:, :3, :3], s["pts"]) + s["P"][:, :3, 3:4]
    pix = (np.round(s["uv"][:, 1]) * w + np.round(s["uv"][:, 0])).astype(np.int64)
    g = torch.Generator(device="cpu").manual_seed(52)
    img = torch.nn.functional.normalize(torch.randn(B, h * w, 64, generator=g, dtype=torch.float64), dim=-1).float()
    pcf = torch.gather(img, 1, torch.from_numpy(pix)[..., None].expand(B, N, 64))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    data = {"pc": f(s["pts"]), "K": f(s["K"]), "P": f(s["P"]), "pc_in_cam_space": f(cam),
            "pc_geo_feat": pcf.permute(0, 2, 1).contiguous().to(DEV), "img_geo_feat": img.view(B, h, w, 64).permute(0, 3, 1, 2).contiguous().to(DEV),
            "pc_overlap_pred": torch.ones(B, N, dtype=torch.bool, device=DEV)}
    model = MultiHeadModel(KittiConfiguration(num_pt=N, device=torch.device(DEV)))
    model.pose_from_matches(data, img_overlap=torch.ones(B, h, w, dtype=torch.bool, device=DEV), thr=1.0)
    assert data["pnp_status"].tolist() == [0] * B
    assert data["pnp_pose"].shape == (B, 4, 4) and data["pnp_inliers"].shape == (B,)
    q, foc = 0.5 * math.sqrt(2.0), K[0, 0]
    rre, rte = _errors(data["pnp_pose"], s["P"])
    assert max(rre) <= math.degrees(q / foc), (rre, math.degrees(q / foc))
    assert max(rte) <= q * cam[:, 2].max() / foc, (rte, q * cam[:, 2].max() / foc)
    P = data["pnp_pose"].double().cpu().numpy()
    for b in range(B):
        pc = P[b, :3, :3] @ s["pts"][b] + P[b, :3, 3:4]
        pr = K @ pc
        dev = np.hypot(pr[0] / pr[2] - s["uv"][b, 0], pr[1] / pr[2] - s["uv"][b, 1])
        assert dev.mean() <= q, dev.mean()
    # an image overlap that excludes every matched pixel leaves no correspondence
    model.pose_from_matches(data, img_overlap=torch.zeros(B, h, w, dtype=torch.bool, device=DEV))
    assert data["pnp_status"].tolist() == [1] * B


def test_test_geo_script_pnp():
    cmd = [sys.executable, os.path.join(ROOT, "Test_Geo.py"), "--pairs", "2", "--batch-size", "2", "--img", "160x512", "--num-pt", "4096",
           "--pnp"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = res.stdout.strip().splitlines()
    rec = [i for i, l in enumerate(lines) if l.startswith("Registration Recall:")]
    assert len(rec) == 1, res.stdout[-2000:]
    i = rec[0]
    assert len(lines[i - 1].split()) == 5                               # the unchanged summary line comes first
    pairs = [l.split() for l in lines[:i - 1] if len(l.split()) == 2]
    pairs = pairs[1:]                                                   # the first 2-number line is the batch's "IR1 IR2"
    assert len(pairs) == 2 and all(float(v) >= 0 for p in pairs for v in p), res.stdout[-2000:]
    recall = float(lines[i].split(":")[1])
    assert 0.0 <= recall <= 1.0
    tail = lines[i + 1:]
    if recall > 0:
        assert tail[0].startswith("RTE Mean:") and "RTE Std:" in tail[0]
        assert tail[1].startswith("RRE Mean:") and "RRE Std:" in tail[1]
    else:
        assert tail == []
