"""Float64 restatement of pose scoring and of the lattice pose search built on it (cmr_pose_score_f32 / ops.pose_score,
MultiHeadModel.score_poses / search_pose), written from the contract in include/cmr_hip.h and independently of the kernel.
The per-row quantities -- in view, the window minimum -- are guided_reference.guided_match's `view` / `wmin`.

score, per sample b and pose p: over the selected rows, d = min(wmin, tau) if the row is in view under pose p, else tau; score = sum d^2;
counts = (in view, in view and wmin <= tau); selected = the selected rows.  A window without a finite distance has wmin = +inf -> tau.

NEAR rows, per (b, p): the selected rows on which an fp32 evaluation may decide differently from this one -- u or v within HALF_TOL px
of a half-integer (the centre may round the other way, which also moves the in-view decision), |wmin - tau| < TOL, or guided_match's own
`near` flag.  Each may move the score by at most tau^2 and each count by at most one.

search: MultiHeadModel.search_pose's rounds, scored here: per round the 729 poses D_i cur, rounded to float32 as the device scores
float32 poses; lowest score wins, lowest index on a tie."""
import itertools
import math

import numpy as np
import torch

import guided_reference as gref
import pnp_reference as pref

TOL = gref.TOL        # |wmin - tau| under which `close` / the clamp may resolve either way
HALF_TOL = 1e-4       # px from a half-integer under which the centre may round either way
NEAR_CAP = 16         # near rows allowed per (sample, pose) on the scenes of the GPU tier (a condition on the scenes, not a measurement)
DEFAULT_LEVELS = ((4, 1.0, 0.1, 3), (2, 0.5, 0.05, 3), (1, 0.25, 0.025, 3), (0, 0.1, 0.01, 6), (0, 0.03, 0.003, 6))


def pose_score(pts, pc, img, mask, poses, K, radius=0, tau=0.8):
    """pts [B, 3, N], pc [B*N, C], img [B, h, w, C], mask [B, N] / [B*N], poses [B, P, 4, 4], K [B, 3, 3] (tensors or arrays of any float
    dtype) -> dict(score float64 [B, P], counts int64 [B, P, 2], selected int64 [B], near int64 [B, P])."""
    poses = np.asarray(poses.detach().cpu() if torch.is_tensor(poses) else poses, np.float64)
    B, P = poses.shape[:2]
    score, counts = np.zeros((B, P)), np.zeros((B, P, 2), np.int64)
    selected, near = np.zeros(B, np.int64), np.zeros((B, P), np.int64)
    for p in range(P):
        with np.errstate(all="ignore"):
            m = gref.guided_match(pts, pc, img, mask, poses[:, p], K, radius)
        for b in range(B):
            e = m[b]
            sel, view, wmin = e["sel"].numpy(), e["view"].numpy(), e["wmin"].numpy()
            with np.errstate(invalid="ignore"):
                d = np.where(view, np.minimum(np.where(np.isnan(wmin), math.inf, wmin), tau), tau)
                close = view & (wmin <= tau)
                u, v = e["proj"][0].numpy(), e["proj"][1].numpy()
                half = (np.abs(u - np.floor(u) - 0.5) < HALF_TOL) | (np.abs(v - np.floor(v) - 0.5) < HALF_TOL)
                edge = view & (np.abs(wmin - tau) < TOL)
            score[b, p] = float((d[sel] ** 2).sum())
            counts[b, p] = int(view.sum()), int(close.sum())
            selected[b] = int(sel.sum())
            near[b, p] = int((sel & (half | edge | e["near"].numpy())).sum())
    return dict(score=score, counts=counts, selected=selected, near=near)


def best_index(score):
    """Lowest score, lowest index on a tie -> int64 [B]."""
    score = np.asarray(score)
    return np.array([int(np.flatnonzero(score[b] == score[b].min())[0]) for b in range(score.shape[0])], np.int64)


# ---- candidate sets ------------------------------------------------------------------------------------------------------------------
MAGNITUDES = ((0.1, 0.01), (0.25, 0.03), (0.5, 0.05), (3.0, 0.3), (10.0, 1.0))


def candidates(sc, seed, draws=3):
    """The candidate set of the ranking tests on a guided_reference.scene: truth, `start`, then `draws` draws of
    guided_reference.perturbed(P, rng, a, sigma) per magnitude, rng = default_rng(seed + 1) -> float64 [B, 2 + 5 draws, 4, 4], all
    float32-representable; the truth is index 0."""
    rng = np.random.default_rng(seed + 1)
    out = [np.asarray(sc["P"], np.float64), np.asarray(sc["start"], np.float64)]
    for a, sigma in MAGNITUDES:
        for _ in range(draws):
            out.append(gref.perturbed(sc["P"], rng, a, sigma))
    return np.stack(out, 1).astype(np.float32).astype(np.float64)


def equality_poses(sc, seed):
    """The 19 poses of the GPU tier's comparison with ops.guided_match: candidates() (17: truth, `start`, three draws per magnitude), a
    pose that puts the cloud behind the camera and a NaN pose -> float64 [B, 19, 4, 4], float32-representable."""
    base = candidates(sc, seed)
    B = base.shape[0]
    behind = np.array(sc["P"], np.float64)
    behind[:, 2, 3] -= 1000.0
    nan = np.full((B, 4, 4), math.nan)
    return np.concatenate([base, behind[:, None], nan[:, None]], 1).astype(np.float32).astype(np.float64)


# ---- the search ----------------------------------------------------------------------------------------------------------------------
def search_offsets():
    """{-1, 0, 1}^6 ordered by (sum |o_j|, o lexicographic) -> int64 [729, 6]; entry 0 is "stay"."""
    return np.array(sorted(itertools.product((-1, 0, 1), repeat=6), key=lambda o: (sum(abs(x) for x in o), o)), np.int64)


def search_table(rot_step_deg, trans_step):
    """D_i = [[Exp(w_i), v_i], [0, 1]], w_i = radians(rot_step_deg) o[:3], v_i = trans_step o[3:] -> float64 [729, 4, 4]."""
    o = search_offsets().astype(np.float64)
    D = np.tile(np.eye(4), (len(o), 1, 1))
    for i in range(len(o)):
        D[i, :3, :3] = pref._expso3(math.radians(rot_step_deg) * o[i, :3])
        D[i, :3, 3] = trans_step * o[i, 3:]
    return D


def search(sc, start, levels=DEFAULT_LEVELS, tau=0.8):
    """-> (poses float64 [B, 4, 4] (float32-representable), last round's best scores [B])."""
    cur = np.asarray(start, np.float64).astype(np.float32).astype(np.float64)
    best = None
    for radius, rot, trans, rounds in levels:
        D = search_table(rot, trans)
        for _ in range(rounds):
            cand = np.einsum("pij,bjk->bpik", D, cur).astype(np.float32).astype(np.float64)
            r = pose_score(sc["pts"], sc["pc"], sc["img"], sc["mask"], cand, sc["K"], radius, tau)
            k = best_index(r["score"])
            cur = np.stack([cand[b, k[b]] for b in range(len(k))])
            best = np.array([r["score"][b, k[b]] for b in range(len(k))])
    return cur, best


# ---- the hand-checkable scene -------------------------------------------------------------------------------------------------------
def tiny():
    """The 8 x 10 scene of tests/test_guided_gpu.py:_tiny (identity K and pose, depth 1: a point projects to (x, y) itself) with known
    distances.  Rows: 0 centre (3, 4), its feature = that pixel's with channel 0 moved by 0.5 (dist 0.5); 1 centre (0, 0), channel 0
    moved by 1 (dist 1 > tau); 2 centre (11, 4): outside the map by 2 columns; 3 centre (13, 4); 4 behind the camera; 5 a NaN coordinate.
    At radius 0 and tau 0.8: rows 0 and 1 in view, row 0 close: score = 0.25 + 5 * 0.64 = 3.45, counts (2, 1), selected 6.
    -> pts [1, 3, 6], pc [6, 64], img [1, 8, 10, 64] (float32 tensors), pose [1, 4, 4], K [1, 3, 3]."""
    h, w = 8, 10
    img = torch.nn.functional.normalize(torch.arange(h * w * 64, dtype=torch.float64).reshape(1, h, w, 64).sin(), dim=-1).float()
    pts = torch.tensor([[[3.2, 0.4, 11.0, 13.0, 3.0, math.nan], [3.7, -0.3, 4.0, 4.0, 4.0, 1.0], [1.0, 1.0, 1.0, 1.0, -1.0, 1.0]]])
    N = pts.shape[2]
    pc = img[0, 4, 3][None].repeat(N, 1)
    pc[0, 0] += 0.5
    pc[1] = img[0, 0, 0]
    pc[1, 0] += 1.0
    pc[2] = img[0, 4, 9]
    return pts, pc.contiguous(), img, torch.eye(4)[None].contiguous(), torch.eye(3)[None].contiguous()


TINY_SCORE, TINY_COUNTS, TINY_SELECTED = 0.25 + 5 * 0.64, [2, 1], 6
