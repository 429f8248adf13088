"""GPU tier of pose scoring (ops.pose_score / cmr_pose_score_f32, MultiHeadModel.score_poses / search_pose, Test_Agent.py --verify /
--search, Test_Geo.py --verify).

The defining test holds ops.pose_score to the path that existed before it: one ops.guided_match(want_dist=True) per pose, reduced in
torch float64 as the contract says.  Both sides run the same fp32 arithmetic, so counts are equal exactly and the scores differ by the
float64 summation order only.  The float64 restatement (pose_score_reference.py) is the second yardstick: there the rows on which an
fp32 evaluation may decide differently (`near`; tests/test_pose_score_cpu.py caps them at 16 per (sample, pose)) may each move the score
by tau^2."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guided_reference as gref
import pose_score_reference as psr
from cmr_agent_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
NAMES = ("planted_201", "random_88x304")
SLICE, CHUNK = 256, 32            # csrc/pose_score.hip PS_SLICE / PS_CHUNK

_SCENES, _DIST = {}, {}


def _scene(name):
    """-> (scene, its 19 poses float64 [B, 19, 4, 4]), built once."""
    if name not in _SCENES:
        _, kw, _, _ = next(s for s in gref.MATCH_SCENES if s[0] == name)
        sc = gref.scene(**kw)
        _SCENES[name] = (sc, psr.equality_poses(sc, kw["seed"]))
    return _SCENES[name]


def _mask(sc, kind):
    B, _, N = sc["pts"].shape
    if kind == "all":
        return sc["mask"]
    m = torch.rand(B, N, generator=torch.Generator().manual_seed(12)) < 0.4
    if kind == "empty0":
        m[0] = False
    return m


def _args(sc, mask, poses):
    return F(sc["pts"]), sc["pc"].to(DEV), sc["img"].to(DEV), mask.to(DEV), F(poses), F(sc["K"])


def _guided(a, radius):
    """One ops.guided_match per pose -> (view bool [B, P, N], dist float32 [B, P, N])."""
    pts, pc, img, mask, poses, K = a
    B, _, N = pts.shape
    view, dist = [], []
    for p in range(poses.shape[1]):
        idx, _, _, d, _ = ops.guided_match(pts, pc, img, mask, poses[:, p].contiguous(), K, radius, want_dist=True)
        view.append(idx.view(B, N) >= 0)
        dist.append(d.view(B, N))
    return torch.stack(view, 1), torch.stack(dist, 1)


def _reduce(a, view, dist, tau):
    """The contract's reduction of guided_match's per-row outputs, in torch: d = min(dist, tau) in fp32 where in view, else tau; the sum
    of (double)d^2 over the selected rows -> (score float64 [B, P], counts int32 [B, P, 2], selected int32 [B])."""
    mask = a[3]
    B, P, N = view.shape
    sel = (mask.view(B, N) != 0)[:, None, :]
    t = torch.tensor(tau, dtype=torch.float32, device=DEV)
    d = torch.where(view, torch.minimum(torch.where(view, dist, t), t), t).double()
    score = torch.where(sel, d * d, torch.zeros_like(d)).sum(2)
    counts = torch.stack([(view & sel).sum(2), (view & sel & (dist <= t)).sum(2)], 2).int()
    return score, counts, sel.sum(2)[:, 0].int()


def _same(got, want):
    """counts and selected exactly; the scores to the float64 summation order."""
    (s, c, n), (rs, rc, rn) = got, want
    assert s.dtype == torch.float64 and c.dtype == torch.int32 and n.dtype == torch.int32
    assert torch.equal(c, rc) and torch.equal(n, rn)
    err = ((s - rs).abs() / rs.clamp(min=1.0)).max()
    print("   max |score - reduction| / max(1, score)", float(err))
    assert float(err) <= 1e-10


# ---- 1. equality with the existing path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["all", "sparse", "empty0"])
@pytest.mark.parametrize("radius", [0, 1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_equals_guided_match_reduced(name, radius, kind):
    sc, poses = _scene(name)
    assert poses.shape[1] == 19
    a = _args(sc, _mask(sc, kind), poses)
    view, dist = _guided(a, radius)
    for tau in (0.6, 0.8):
        got = ops.pose_score(*a, radius=radius, tau=tau)
        want = _reduce(a, view, dist, tau)
        print(name, "r", radius, kind, "tau", tau, "scores", got[0][:, :3].tolist(), "selected", got[2].tolist())
        _same(got, want)
        assert float(got[0][:, 18].sub(got[2].double() * float(np.float32(tau)) ** 2).abs().max()) <= 1e-9    # the NaN pose: tau^2 a row
        assert got[1][:, 17:].abs().max().item() == 0                                                              # behind / NaN: nothing in view
    if kind == "empty0":
        assert got[0][0].abs().max().item() == 0 and got[1][0].abs().max().item() == 0 and got[2].tolist()[0] == 0


# ---- 2. against float64 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_against_float64(name, radius):
    sc, poses = _scene(name)
    tau = 0.8
    score, counts, selected = ops.pose_score(*_args(sc, sc["mask"], poses), radius=radius, tau=tau)
    ref = psr.pose_score(sc["pts"], sc["pc"], sc["img"], sc["mask"], poses, sc["K"], radius, tau)
    score, counts = score.cpu().numpy(), counts.cpu().numpy().astype(np.int64)
    assert selected.cpu().tolist() == ref["selected"].tolist()
    bound = ref["near"] * tau * tau + 1e-5 * ref["selected"][:, None]
    err = np.abs(score - ref["score"])
    print(name, "r", radius, "max |score - float64|", err.max(), "max near", int(ref["near"].max()), "worst share of the bound", (err / bound).max(),
          "max count deviation", np.abs(counts - ref["counts"]).max())
    assert (err <= bound).all()
    assert (np.abs(counts - ref["counts"]) <= ref["near"][..., None]).all()


# ---- 3. ranking ---------------------------------------------------------------------------------------------------------------------------
def _model(N):
    from cmr_agent_amd.models import MultiHeadModel
    from cmr_agent_amd.config import KittiConfiguration
    return MultiHeadModel(KittiConfiguration(num_pt=N, device=torch.device(DEV)))


def _data(sc):
    B, _, N = sc["pts"].shape
    return {"pc": F(sc["pts"]), "K": F(sc["K"]), "P": F(sc["P"]),
            "pc_geo_feat": sc["pc"].view(B, N, 64).permute(0, 2, 1).contiguous().to(DEV),
            "img_geo_feat": sc["img"].permute(0, 3, 1, 2).contiguous().to(DEV), "pc_overlap_pred": sc["mask"].to(DEV)}


@pytest.mark.parametrize("seed", [201, 202, 203])
def test_score_poses_picks_the_truth(seed):
    sc = gref.scene(B=2, N=4096, h=40, w=128, seed=seed)
    cand = psr.candidates(sc, seed)
    data = _data(sc)
    _model(4096).score_poses(data, F(cand), radius=0, tau=0.8)
    s, q = data["pose_scores"], data["pose_quality"]
    print("seed", seed, "truth", s[:, 0].tolist(), "runner-up", s[:, 1:].min(1).values.tolist(), "quality of the truth", q[:, 0].tolist())
    assert data["pose_best"].dtype == torch.int64 and data["pose_best"].tolist() == [0, 0]
    assert s.dtype == torch.float64 and tuple(s.shape) == (2, 17) and tuple(data["pose_score_counts"].shape) == (2, 17, 2)
    tau2 = float(np.float32(0.8)) ** 2
    want = (1.0 - s / (4096 * tau2)).clamp(min=0.0)                      # to a few ulp: a division by a scalar may be a multiplication by its reciprocal
    assert q.dtype == torch.float64 and float((q - want).abs().max()) <= 1e-15 and bool(((q >= 0) & (q <= 1)).all())
    # a tie keeps the lowest index; no selected row gives quality 0
    twice = F(np.concatenate([cand[:, 3:4], cand[:, 0:1], cand[:, 0:1]], 1))
    _model(4096).score_poses(data, twice, mask=torch.zeros(2, 4096, dtype=torch.bool))
    assert data["pose_best"].tolist() == [0, 0] and data["pose_quality"].abs().max().item() == 0
    _model(4096).score_poses(data, twice)
    assert data["pose_best"].tolist() == [1, 1]


# ---- 4. slice and chunk edges ---------------------------------------------------------------------------------------------------------------
_EDGE = {}


def _edge_scene():
    if not _EDGE:
        sc = gref.scene(B=3, N=4 * SLICE + 1, h=40, w=128, seed=231)
        poses = np.concatenate([psr.equality_poses(sc, 231), psr.candidates(sc, 232)], 1)                 # 36 >= CHUNK + 1
        _EDGE["v"] = (sc, poses)
    return _EDGE["v"]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("P", [1, 2, CHUNK + 1])
@pytest.mark.parametrize("N", [1, 15, SLICE + 1, 4 * SLICE + 1])
def test_slice_and_chunk_edges(N, P, B):
    sc, poses = _edge_scene()
    N0 = sc["pts"].shape[2]
    mask = (torch.rand(3, N0, generator=torch.Generator().manual_seed(13)) < 0.7)[:B, :N].contiguous()
    a = (F(sc["pts"][:B, :, :N]), sc["pc"].view(3, N0, 64)[:B, :N].reshape(B * N, 64).contiguous().to(DEV), sc["img"][:B].contiguous().to(DEV),
         mask.to(DEV), F(poses[:B, :P]), F(sc["K"][:B]))
    view, dist = _guided(a, 1)
    _same(ops.pose_score(*a, radius=1, tau=0.8), _reduce(a, view, dist, 0.8))


# ---- 5. independence and determinism -------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def _det_args():
    sc, poses = _edge_scene()
    mask = torch.rand(3, sc["pts"].shape[2], generator=torch.Generator().manual_seed(14)) < 0.7
    return _args(sc, mask, poses)


def test_two_calls_agree_bit_for_bit():
    a = _det_args()
    for x, y in zip(ops.pose_score(*a, radius=1), ops.pose_score(*a, radius=1)):
        assert torch.equal(_bits(x), _bits(y))


def test_pose_alone_equals_pose_in_batch():
    a = _det_args()
    score, counts, selected = ops.pose_score(*a, radius=1)
    for p in range(a[4].shape[1]):
        s1, c1, n1 = ops.pose_score(*a[:4], a[4][:, p:p + 1].contiguous(), a[5], radius=1)
        assert torch.equal(_bits(s1[:, 0]), _bits(score[:, p])) and torch.equal(c1[:, 0], counts[:, p]) and torch.equal(n1, selected)


def test_sample_alone_equals_sample_in_batch():
    a = _det_args()
    B, _, N = a[0].shape
    score, counts, selected = ops.pose_score(*a, radius=1)
    for k in range(B):
        one = (a[0][k:k + 1].contiguous(), a[1][k * N:(k + 1) * N].contiguous(), a[2][k:k + 1].contiguous(), a[3][k:k + 1].contiguous(),
               a[4][k:k + 1].contiguous(), a[5][k:k + 1].contiguous())
        s1, c1, n1 = ops.pose_score(*one, radius=1)
        assert torch.equal(_bits(s1[0]), _bits(score[k])) and torch.equal(c1[0], counts[k]) and torch.equal(n1[0], selected[k])


def test_graph_replay_equals_eager():
    a = _det_args()
    fn = lambda: ops.pose_score(*a, radius=1)
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
        t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, got):
        assert torch.equal(_bits(x), _bits(y))


def test_tiny_scene_and_mask_dtypes():
    pts, pc, img, pose, K = (t.to(DEV) for t in psr.tiny())
    N = pts.shape[2]
    ones = torch.ones(1, N, dtype=torch.bool, device=DEV)
    both = torch.stack([torch.full((1, 4, 4), math.nan, device=DEV), pose], 1).contiguous()
    score, counts, selected = ops.pose_score(pts, pc, img, ones, both, K, radius=0, tau=0.8)
    tau2 = float(np.float32(0.8)) ** 2
    assert abs(float(score[0, 1]) - (0.25 + 5 * tau2)) <= 1e-6 and counts[0, 1].tolist() == psr.TINY_COUNTS and selected.tolist() == [psr.TINY_SELECTED]
    assert abs(float(score[0, 0]) - N * tau2) <= 1e-12 and counts[0, 0].tolist() == [0, 0]
    assert counts[0, 1, 0].item() == 2 and ops.pose_score(pts, pc, img, ones, both, K, radius=2)[1][0, 1, 0].item() == 3
    z = ops.pose_score(pts, pc, img, torch.zeros(1, N, dtype=torch.bool, device=DEV), both, K)
    assert z[0].tolist() == [[0.0, 0.0]] and z[1].tolist() == [[[0, 0], [0, 0]]] and z[2].tolist() == [0]
    m = torch.tensor([[True, False, True, False, True, True]], device=DEV)
    outs = [ops.pose_score(pts, pc, img, mm, both, K, radius=2) for mm in (m, m.to(torch.uint8), m.long() * 7)]
    assert outs[0][2].tolist() == [4] and outs[0][1][0, 1].tolist() == [2, 2]
    for o in outs[1:]:
        for x, y in zip(o, outs[0]):
            assert torch.equal(_bits(x), _bits(y))


# ---- 6. search ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [201, 202])
def test_search_pose_reaches_the_truth(seed):
    """Bars: twice the worst end of the float64 restatement of the same search (pose_score_reference.search, run on the CPU, about
    90 s a seed, so not a committed test; its figures are in DESIGN.md 4q).  The device may break a near-tie the other way and take a
    different but equally good path."""
    sc = gref.scene(B=2, N=1024, h=40, w=128, seed=seed)
    data = _data(sc)
    model = _model(1024)
    start = F(sc["start"])
    model.search_pose(data, pose=start, tau=0.8)
    pose, score = data["searched_pose"], data["searched_score"]
    assert tuple(pose.shape) == (2, 4, 4) and pose.dtype == torch.float32 and score.dtype == torch.float64 and tuple(score.shape) == (2,)
    er, et = gref.pose_errors(pose.double().cpu().numpy(), sc["P"])
    s0 = ops.pose_score(*_args(sc, sc["mask"], np.asarray(sc["start"])[:, None]), radius=0, tau=0.8)[0][:, 0]
    print("seed", seed, "start", gref.pose_errors(sc["start"], sc["P"]), "searched", er, et, "score", s0.tolist(), "->", score.tolist())
    assert max(er) <= 0.1 and max(et) <= 0.05
    assert bool((score <= s0).all())
    model.search_pose(data, pose=start, tau=0.8)
    assert torch.equal(_bits(data["searched_pose"]), _bits(pose)) and torch.equal(_bits(data["searched_score"]), _bits(score))


# ---- 7. the scripts ---------------------------------------------------------------------------------------------------------------------------
def _run(script, *flags):
    cmd = [sys.executable, os.path.join(ROOT, script), "--pairs", "1", "--img", "160x512", "--num-pt", "4096", *flags]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return res.stdout.strip().splitlines()


def _in_order(plain, lines):
    it = iter(lines)
    assert all(any(l == x for x in it) for l in plain), (plain, lines)


def _check_verified(lines, names, extra_blocks):
    ver = [l for l in lines if l.startswith("verified ")]
    assert len(ver) == 1
    tok = ver[0].split()
    assert [t.split("=")[0] for t in tok[1:-2]] == names and tok[-2] == "->" and tok[-1] in names
    assert all(0.0 <= float(t.split("=")[1]) <= 1.0 for t in tok[1:-2])
    heads = [l.split(":")[0] for l in lines if "Registration Recall:" in l]
    assert heads == ["Registration Recall"] + [p + " Registration Recall" for p in extra_blocks]


def test_test_agent_script_search_and_verify():
    lines = _run("Test_Agent.py", "--refine", "4,2", "--search", "--verify")
    _in_order(_run("Test_Agent.py", "--refine", "4,2"), lines)
    sea = [i for i, l in enumerate(lines) if l.startswith("searched ")]
    assert len(sea) == 1 and len(lines[sea[0]].split()) == 3 and all(float(v) >= 0 for v in lines[sea[0]].split()[1:])
    assert lines[sea[0] - 1].startswith("refined ") and lines[sea[0] + 1].startswith("verified ")
    _check_verified(lines, ["agent", "refined", "searched"], ["Refined", "Searched", "Verified"])


def test_test_geo_script_verify():
    lines = _run("Test_Geo.py", "--pnp", "--guided", "4,2", "--verify")
    _in_order(_run("Test_Geo.py", "--pnp", "--guided", "4,2"), lines)
    _check_verified(lines, ["pnp", "refined"], ["Refined", "Verified"])
    res = subprocess.run([sys.executable, os.path.join(ROOT, "Test_Geo.py"), "--verify"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "--verify" in res.stderr
