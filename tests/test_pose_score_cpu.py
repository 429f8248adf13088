"""CPU tier of pose scoring: the float64 restatement in pose_score_reference.py gives the hand-computed values on a tiny
scene (so the yardstick of the GPU tests is itself checked), the scenes of the GPU tier meet the conditions its ranking and float64
comparisons rely on (the truth scores lowest; at most NEAR_CAP rows per (sample, pose) may resolve either way in fp32), ops.pose_score
refuses malformed arguments before any launch, search_pose's candidate table is what the contract says, and the header declares the entry
points."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import guided_reference as gref
import pose_score_reference as psr
from cmr_agent_amd import ops

mhm = importlib.import_module("cmr_agent_amd.models.MultiHeadModel")     # the module: the package exports the class under this name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 0.8


# ---- the restatement on the hand-checkable scene ------------------------------------------------------------------------------------------
def test_restatement_on_the_tiny_scene():
    pts, pc, img, pose, K = psr.tiny()
    N = pts.shape[2]
    ones = torch.ones(1, N, dtype=torch.bool)
    r = psr.pose_score(pts, pc, img, ones, pose[:, None], K, 0, TAU)
    assert abs(r["score"][0, 0] - psr.TINY_SCORE) <= 1e-6                  # 0.5^2 + 5 tau^2: the features are float32, 0.5 is exact to 1e-7
    assert r["counts"][0, 0].tolist() == psr.TINY_COUNTS and r["selected"].tolist() == [psr.TINY_SELECTED]
    # radius 2: row 2 (centre two columns outside) comes into view and meets its own pixel feature on the border; row 0's window holds
    # nothing nearer than 0.5 that could be known by hand, so only the bounds and the counts are asserted
    r2 = psr.pose_score(pts, pc, img, ones, pose[:, None], K, 2, TAU)
    assert r2["counts"][0, 0].tolist()[0] == 3 and 3 * TAU * TAU <= r2["score"][0, 0] <= 0.25 + 4 * TAU * TAU + 1e-6
    # only rows 0 and 2 selected, radius 2: row 2 costs 0
    m = torch.tensor([[True, False, True, False, False, False]])
    r3 = psr.pose_score(pts, pc, img, m, pose[:, None], K, 2, TAU)
    assert r3["selected"].tolist() == [2] and r3["counts"][0, 0].tolist() == [2, 2] and r3["score"][0, 0] <= 0.25 + 1e-6
    # a NaN pose: every row costs tau^2; two poses at once keep their places
    both = torch.stack([torch.full((1, 4, 4), math.nan), pose], 1)
    r4 = psr.pose_score(pts, pc, img, ones, both, K, 0, TAU)
    assert abs(r4["score"][0, 0] - N * TAU * TAU) <= 1e-12 and r4["counts"][0, 0].tolist() == [0, 0]
    assert abs(r4["score"][0, 1] - psr.TINY_SCORE) <= 1e-6 and psr.best_index(r4["score"]).tolist() == [1]
    # an empty mask: zeros
    r5 = psr.pose_score(pts, pc, img, torch.zeros(1, N, dtype=torch.bool), pose[:, None], K, 0, TAU)
    assert r5["score"].tolist() == [[0.0]] and r5["counts"].tolist() == [[[0, 0]]] and r5["selected"].tolist() == [0]


# ---- conditions on the scenes of the GPU tier ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [201, 202, 203])
def test_truth_scores_lowest_and_near_rows_stay_under_the_cap(seed):
    """(a) the truth (index 0) has the lowest score on every sample, by a margin far above NEAR_CAP tau^2; (b) at most NEAR_CAP near rows
    per (sample, pose) -- conditions on the scenes, asserted from the restatement alone."""
    sc = gref.scene(B=2, N=4096, h=40, w=128, seed=seed)
    cand = psr.candidates(sc, seed)
    assert cand.shape == (2, 17, 4, 4)
    r = psr.pose_score(sc["pts"], sc["pc"], sc["img"], sc["mask"], cand, sc["K"], 0, TAU)
    for b in range(2):
        order = np.sort(r["score"][b])
        print("seed", seed, "sample", b, "truth", r["score"][b, 0], "runner-up", order[1], "max near", int(r["near"][b].max()))
        assert psr.best_index(r["score"])[b] == 0
        assert order[1] - r["score"][b, 0] > 4 * psr.NEAR_CAP * TAU * TAU
    assert int(r["near"].max()) <= psr.NEAR_CAP


# ---- argument checks --------------------------------------------------------------------------------------------------------------------
def _args(B=2, N=8, P=3, h=4, w=5):
    return [torch.zeros(B, 3, N), torch.zeros(B * N, 64), torch.zeros(B, h, w, 64), torch.ones(B, N, dtype=torch.bool),
            torch.eye(4).repeat(B, P, 1, 1), torch.eye(3).repeat(B, 1, 1)]


def _refused(args, match, **kw):
    with pytest.raises(ValueError, match=match):
        ops.pose_score(*args, **kw)


def test_pose_score_argument_checks():
    a = _args()
    _refused([a[0][0]] + a[1:], "pose_score: pts must be")
    _refused([a[0][:, :2]] + a[1:], "pose_score: pts must be")
    _refused([a[0], a[1][None]] + a[2:], "pose_score: point rows must be 2-D")
    _refused(a[:2] + [a[2][0]] + a[3:], "pose_score: point rows must be 2-D")
    _refused([a[0], torch.zeros(16, 32)] + a[2:], "pose_score: feature width must be 64")
    _refused(a[:2] + [torch.zeros(2, 4, 5, 32)] + a[3:], "pose_score: feature width must be 64")
    _refused([a[0], torch.zeros(17, 64)] + a[2:], "do not agree on B and N")
    _refused(a[:2] + [torch.zeros(3, 4, 5, 64)] + a[3:], "do not agree on B and N")
    for i in (0, 1, 2, 4, 5):
        b = list(a)
        b[i] = b[i].double()
        _refused(b, "pose_score: pts, features, poses and K must be float32")
    _refused(a[:4] + [a[4][:, 0]] + a[5:], "pose_score: poses must be")
    _refused(a[:4] + [a[4][:1]] + a[5:], "pose_score: poses must be")
    _refused(a[:4] + [a[4][..., :3]] + a[5:], "pose_score: poses must be")
    _refused(a[:4] + [a[4][:, :0]] + a[5:], "pose_score: need 1 <= P <= 4096")
    _refused(a[:4] + [torch.eye(4).repeat(2, 4097, 1, 1)] + a[5:], "pose_score: need 1 <= P <= 4096")
    _refused(a[:5] + [a[5][:1]], "pose_score: K must be")
    _refused(a[:3] + [a[3].float()] + a[4:], "pose_score: mask must be")
    _refused(a[:3] + [a[3][:1]] + a[4:], "pose_score: mask must be")
    for radius in (-1, ops.GUIDED_MAX_RADIUS + 1, 1.5, math.nan, True, "2"):
        _refused(a, "pose_score: radius must be", radius=radius)
    for tau in (0.0, -0.5, math.inf, math.nan, None):
        _refused(a, "pose_score: tau must be", tau=tau)
    assert ops.POSE_SCORE_MAX_POSES == 4096
    # every check above passed on CPU tensors: the device check comes last
    _refused(a, "pose_score: every tensor must be a contiguous tensor on the same GPU")


# ---- the candidate table of search_pose ---------------------------------------------------------------------------------------------------
def test_search_table():
    o = mhm.pose_search_offsets()
    assert o.shape == (729, 6) and o[0].tolist() == [0] * 6 and len({tuple(r) for r in o.tolist()}) == 729
    assert set(np.unique(o).tolist()) == {-1, 0, 1}
    key = [(int(np.abs(r).sum()), tuple(r)) for r in o.tolist()]
    assert key == sorted(key)
    assert o[1].tolist() == [-1, 0, 0, 0, 0, 0] and o[12].tolist() == [1, 0, 0, 0, 0, 0] and o[-1].tolist() == [1] * 6
    assert np.array_equal(o, psr.search_offsets())
    D = mhm.pose_search_table(0.5, 0.05)
    assert D.dtype == torch.float64 and tuple(D.shape) == (729, 4, 4) and torch.equal(D[0], torch.eye(4, dtype=torch.float64))
    D = D.numpy()
    R, t = D[:, :3, :3], D[:, :3, 3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-15 and np.abs(np.linalg.det(R) - 1).max() <= 1e-15
    assert np.array_equal(D[:, 3], np.tile([0.0, 0, 0, 1], (729, 1)))
    assert np.allclose(t, 0.05 * o[:, 3:], rtol=0, atol=0)
    ang = np.degrees(np.arccos(np.clip((np.trace(R, axis1=1, axis2=2) - 1) / 2, -1, 1)))
    assert np.abs(ang - 0.5 * np.linalg.norm(o[:, :3], axis=1)).max() <= 1e-6      # arccos near 1 loses half the digits
    assert np.abs(D - psr.search_table(0.5, 0.05)).max() <= 1e-15
    # every level of the default schedule is well-formed
    assert mhm.SEARCH_LEVELS == psr.DEFAULT_LEVELS
    for radius, rot, trans, rounds in mhm.SEARCH_LEVELS:
        assert 0 <= radius <= ops.GUIDED_MAX_RADIUS and rot > 0 and trans > 0 and rounds >= 1


def test_first_min_takes_the_lowest_index():
    s = torch.tensor([[3.0, 1.0, 1.0, 2.0], [0.5, 0.5, 0.5, 0.5], [2.0, 3.0, 4.0, 1.0]], dtype=torch.float64)
    assert mhm._first_min(s).tolist() == [1, 0, 3]


# ---- the header ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_pose_score():
    text = open(os.path.join(ROOT, "include", "cmr_hip.h")).read()
    assert re.search(r"int64_t\s+cmr_pose_score_workspace_bytes\s*\(\s*int B,\s*int N,\s*int P\s*\)", text)
    assert re.search(r"int\s+cmr_pose_score_f32\s*\(", text)
