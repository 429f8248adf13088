"""GPU tier of the agent environment's kernels (csrc/agent.hip, csrc/rollout.hip): every kernel case by case against the
float64 restatement in env_reference.py, whose agreement with the oracle and whose caps tests/test_env_cpu.py asserts.  Index- and
flag-valued results must be identical wherever fp32 can decide them (env_reference's docstring says where that is); values carry
tolerances derived from the roundings of the kernel, stated next to each constant."""
import math

import numpy as np
import pytest
import torch

import env_reference as er
from oracle import cmr_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = er.U


@pytest.fixture(scope="module")
def ops():
    from cmr_agent_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def env():
    from cmr_agent_amd.environment import environment as _env
    return _env


def _np(t):
    return t.detach().cpu().double().numpy()


# ---- observation ---------------------------------------------------------------------------------------------------------------------------
class _Scene:
    """device-side inputs of one scene in the kernels' layouts"""

    def __init__(self, ops, s, mean=None):
        self.s, self.B, self.N, self.h, self.w = s, s["B"], s["N"], s["h"], s["w"]
        self.pc4 = ops.planar_to_rows4(s["pc"].contiguous().to(DEV))
        self.feat = s["feat"].permute(0, 2, 1).reshape(-1, 64).contiguous().to(DEV)
        self.ov = s["ov"].to(torch.uint8).reshape(-1).to(DEV)
        self.K = s["K"].contiguous().to(DEV)
        self.mean4 = ops.colmean(self.pc4, self.B, self.N) if mean is None else mean.contiguous().to(DEV)
        self.imf = s["imf"].permute(0, 2, 3, 1).contiguous().to(DEV) if "imf" in s else torch.zeros(self.B, self.h, self.w, 64, device=DEV)
        self.fmax = float(s["feat"].abs().max())

    def ref(self, pose):
        s = self.s
        return er.observation(s["pc"], s["feat"], s["ov"], pose, s["K"], self.mean4.cpu(), self.h, self.w)

    def scatter(self, ops, pose, zero_first=True, acc=None, cnt=None, clear=False):
        B, N, h, w = self.B, self.N, self.h, self.w
        acc = torch.full((B * h * w, 64), 7.0, device=DEV) if acc is None else acc        # zero_first=True has to clear them
        cnt = torch.full((B * h * w,), 7.0, device=DEV) if cnt is None else cnt
        st3 = torch.full((B * N, 8), -1.0, device=DEV)
        ops.project_scatter(self.pc4, self.feat, self.ov, pose.contiguous().to(DEV), self.K, self.mean4, B, N, h, w, acc, cnt, st3,
                            zero_first=zero_first)
        counts = cnt.clone()
        st2 = torch.empty(B, h, w, 128, device=DEV)
        proj = torch.empty(B, h, w, 64, device=DEV)
        ops.observation_finalize(self.imf, acc, cnt, st2, proj, B, h, w, True, clear=clear)
        assert torch.equal(st2[..., 64:], proj) and torch.equal(st2[..., :64], self.imf)
        return proj, counts, st3, acc, cnt

    def direct_state(self):
        B, N, h, w = self.B, self.N, self.h, self.w
        return (torch.zeros(B, h, w, 64, device=DEV), torch.zeros(B * h * w, device=DEV), torch.full((B * N,), -1, dtype=torch.int32, device=DEV))

    def direct(self, ops, pose, state):
        B, N, h, w = self.B, self.N, self.h, self.w
        st3 = torch.full((B * N, 8), -1.0, device=DEV)
        ops.observation_proj(self.pc4, self.feat, self.ov, pose.contiguous().to(DEV), self.K, self.mean4, B, N, h, w, state[0], state[1], state[2], st3)
        return st3


def _check_state3d(st3, r):
    got = _np(st3).reshape(r["state3d"].shape)
    assert np.array_equal(got[:, :, 0:4], r["state3d"][:, :, 0:4])          # the cloud and the overlap flag: bit exact for all points
    assert np.array_equal(got[:, :, 5:8], np.zeros_like(got[:, :, 5:8]))
    d = r["decided"]
    assert np.array_equal(got[:, :, 4][d], r["state3d"][:, :, 4][d])        # in view: exact wherever fp32 can decide


def _check_map(proj, counts, r, fmax):
    """on decided cells: occupancy and count exact, values within (n + 1) 2^-23 max|feat| -- the fp32 sum of n terms of at most max|feat|
    ((n - 1) U n max|feat| / n after the division) plus the division's rounding; the direct path's n divisions and n - 1 sums come to the same"""
    got, cnt = _np(proj), _np(counts).reshape(r["count"].shape)
    cd = r["cell_decided"]
    assert np.array_equal(cnt[cd], r["count"][cd].astype(np.float64))
    assert np.array_equal((np.abs(got).max(-1) > 0)[cd], (r["count"] > 0)[cd])
    tol = (r["count"] + 1) * 2.0 ** -23 * fmax
    err = np.abs(got - r["map"]).max(-1)
    assert (err[cd] <= tol[cd]).all(), (float(err[cd].max()), float(tol[cd].min()))


@pytest.mark.parametrize("name", ["edges", "straddle"])
def test_hand_scene_bit_for_bit_on_both_paths(ops, name):
    s = er.hand_scene()[name]
    sc = _Scene(ops, s, mean=s["mean"])
    e = s["expect"]
    proj, counts, st3, acc, cnt = sc.scatter(ops, s["pose"], clear=True)
    assert np.array_equal(_np(proj), e["map"]) and np.array_equal(_np(counts).reshape(e["count"].shape), e["count"].astype(np.float64))
    assert np.array_equal(_np(st3).reshape(e["state3d"].shape), e["state3d"])                   # columns 5..7 are zero in the literal
    assert float(acc.abs().max()) == 0 and float(cnt.abs().max()) == 0                          # finalize(clear=True) left them zeroed
    # ... so the next scatter needs no memset and gives the same picture
    proj2, _, st3b, acc, cnt = sc.scatter(ops, s["pose"], zero_first=False, acc=acc, cnt=cnt, clear=True)
    assert torch.equal(proj2, proj) and torch.equal(st3b, st3) and float(acc.abs().max()) == 0 and float(cnt.abs().max()) == 0
    state = sc.direct_state()
    for _ in range(2):                                                                          # the second call clears and rebuilds
        st3d = sc.direct(ops, s["pose"], state)
        assert np.array_equal(_np(state[0]), e["map"]) and np.array_equal(_np(state[1]).reshape(e["count"].shape), e["count"].astype(np.float64))
        assert np.array_equal(state[2].cpu().numpy().reshape(e["cell"].shape), e["cell"])
        assert np.array_equal(_np(st3d).reshape(e["state3d"].shape), e["state3d"])


def test_points_fp32_cannot_decide_are_left_out_and_the_rest_is_held(ops):
    s = er.planted_scene()
    sc = _Scene(ops, s, mean=s["mean"])
    r = sc.ref(s["pose"])
    assert r["decided"][0].tolist() == [False, False, True, True] and int(r["cell_decided"].sum()) == 100 - 3
    proj, counts, st3, _, _ = sc.scatter(ops, s["pose"])
    _check_state3d(st3, r)
    _check_map(proj, counts, r, sc.fmax)
    assert float(counts.sum()) in (1.0, 2.0, 3.0) and float(counts[4 * 10 + 4]) == 1      # the undecided two land in their candidate cells or nowhere
    assert set(torch.nonzero(counts).reshape(-1).tolist()) <= {42, 43, 44, 49}
    state = sc.direct_state()
    _check_state3d(sc.direct(ops, s["pose"], state), r)
    _check_map(state[0], state[1], r, sc.fmax)
    assert torch.equal(state[1], counts)


@pytest.fixture(scope="module")
def scenes(ops):
    """name -> (_Scene, float64 reference at the scene's own pose), computed once"""
    out = {}
    for name in er.SCENES:
        sc = _Scene(ops, er.scene(name))
        out[name] = (sc, sc.ref(sc.s["pose"]))
    return out


@pytest.mark.parametrize("name", sorted(er.SCENES))
def test_random_scenes_scatter_and_finalize(ops, scenes, name):
    sc, r = scenes[name]
    und, exc = er.shares(r, sc.s["ov"])
    print("%s (device centroid): undecided points %.5f, excluded cells %.5f" % (name, und, exc))
    assert und <= er.MAX_UNDECIDED_POINTS and exc <= er.MAX_EXCLUDED_CELLS
    proj, counts, st3, acc, cnt = sc.scatter(ops, sc.s["pose"], clear=True)
    _check_state3d(st3, r)
    _check_map(proj, counts, r, sc.fmax)
    assert float(acc.abs().max()) == 0 and float(cnt.abs().max()) == 0
    _special(name, sc, r, proj, counts, st3)


@pytest.mark.parametrize("name", sorted(er.SCENES))
def test_random_scenes_direct_path(ops, scenes, name):
    sc, r = scenes[name]
    state = sc.direct_state()
    st3 = sc.direct(ops, sc.s["pose"], state)
    _check_state3d(st3, r)
    _check_map(state[0], state[1], r, sc.fmax)
    d = r["decided"].reshape(-1)
    assert np.array_equal(state[2].cpu().numpy()[d], r["cell"].reshape(-1)[d])
    _special(name, sc, r, state[0], state[1], st3)


def _special(name, sc, r, proj, counts, st3):
    if name == "pile_up":                                                   # one cell with 4096 contributions, everything else exactly zero
        assert r["decided"].all() and int((r["count"] > 0).sum()) == 1 and int(r["count"].max()) == sc.N
        assert int((counts != 0).sum()) == 1 and float(counts.max()) == sc.N
        assert int((proj.abs().amax(-1) != 0).sum()) == 1
    if name == "no_overlap":                                                # nothing scattered, the flags still written
        assert float(proj.abs().max()) == 0 and float(counts.abs().max()) == 0
        assert float(st3[:, 4].sum()) > 0 and float(st3[:, 3].abs().max()) == 0


def test_direct_path_over_a_sequence_of_poses(ops, scenes):
    sc, _ = scenes["yaw_1037"]
    start = sc.s["pose"]
    shift = start.clone()
    shift[:, 0, 3] += 3.0
    away = start.clone()
    away[:, 2, 3] -= 1000.0                                                 # everything behind the camera
    state = sc.direct_state()
    refs = {}
    prev_occ = np.zeros((sc.B, sc.h, sc.w), dtype=bool)
    for tag, pose in (("start", start), ("shift", shift), ("start", start), ("away", away), ("start", start), ("start", start)):
        if tag not in refs:
            refs[tag] = sc.ref(pose)
        r = refs[tag]
        st3 = sc.direct(ops, pose, state)
        _check_state3d(st3, r)
        _check_map(state[0], state[1], r, sc.fmax)
        d = r["decided"].reshape(-1)
        assert np.array_equal(state[2].cpu().numpy()[d], r["cell"].reshape(-1)[d])
        # cells the previous pose filled and this one does not: exactly zero in both buffers
        vacated = prev_occ & (r["count"] == 0) & r["cell_decided"]
        assert float(np.abs(_np(state[0])[vacated]).sum()) == 0 and float(np.abs(_np(state[1]).reshape(prev_occ.shape)[vacated]).sum()) == 0
        if tag == "away":
            assert r["decided"].all() and float(state[0].abs().max()) == 0 and float(state[1].abs().max()) == 0 and int(state[2].max()) == -1
        else:
            assert vacated.any() or tag == "start"
        prev_occ = (r["count"] > 0) | ~r["cell_decided"]
    assert refs["shift"]["count"].sum() > 0 and (refs["shift"]["count"] > 0).sum() != (refs["start"]["count"] > 0).sum()


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), er.OFFSET], ids=["origin", "offset"])
def test_colmean_against_float64(ops, offset):
    """tolerance N 2^-24 max|p|: every partial sum of N terms is at most N max|p| and the adds of any summation tree contribute at most
    U x that each along a path of depth <= N; for the offset cloud max|p| grows with the offset and the tolerance with it"""
    for name in sorted(er.SCENES):
        s = er.scene(name)
        pc = (s["pc"] + torch.tensor(offset).view(1, 3, 1)).contiguous()
        got = _np(ops.colmean(ops.planar_to_rows4(pc.to(DEV)), s["B"], s["N"]))
        ref = pc.double().mean(dim=2).numpy()
        tol = s["N"] * 2.0 ** -24 * float(pc.abs().max())
        assert np.abs(got[:, 0:3] - ref).max() <= tol, (name, float(np.abs(got[:, 0:3] - ref).max()), tol)


def test_environment_level_observation(ops, env):
    """env.observation_from_a_pose with plain tensors in the batch dict and no model, materialised and direct, against the same reference"""
    s = er.scene("yaw_1037")
    data = dict(K=s["K"].to(DEV), pc=s["pc"].to(DEV), pc_overlap_pred=s["ov"].to(DEV), pc_geo_feat=s["feat"].to(DEV), img_geo_feat=s["imf"].to(DEV))
    pose = s["pose"].to(DEV)
    s2, s3 = env.observation_from_a_pose(data, pose)
    ctx = data["_cmr_obs"]
    assert not ctx.dirty and ctx.acc is not None
    r = er.observation(s["pc"], s["feat"], s["ov"], s["pose"], s["K"], ctx.mean4.cpu(), s["h"], s["w"])
    cd = r["cell_decided"]
    tol = (r["count"] + 1) * 2.0 ** -23 * float(s["feat"].abs().max())

    def check(half, st3):
        assert st3.shape == (s["B"], 5, s["N"])
        got3 = _np(st3).transpose(0, 2, 1)
        assert np.array_equal(got3[:, :, :4], r["state3d"][:, :, :4])
        assert np.array_equal(got3[:, :, 4][r["decided"]], r["state3d"][:, :, 4][r["decided"]])
        got = _np(half)
        assert np.array_equal((np.abs(got).max(-1) > 0)[cd], (r["count"] > 0)[cd])
        assert (np.abs(got - r["map"]).max(-1)[cd] <= tol[cd]).all()

    assert s2.shape == (s["B"], 128, s["h"], s["w"]) and torch.equal(s2[:, :64], data["img_geo_feat"])       # the image half: bit for bit
    check(s2[:, 64:].permute(0, 2, 3, 1), s3)
    first = s2.clone()
    # the second call on the same dict finds the accumulators zeroed by the first (zero_first=False) and must give the same picture
    assert float(ctx.acc.abs().max()) == 0 and float(ctx.cnt.abs().max()) == 0
    s2b, s3b = env.observation_from_a_pose(data, pose)
    assert data["_cmr_obs"] is ctx and s2b.data_ptr() != s2.data_ptr()
    check(s2b[:, 64:].permute(0, 2, 3, 1), s3b)
    assert float((s2b - first).abs().max()) <= 2 * float(tol.max())
    # the direct path: a shape-only state_2d carrying its halves
    m2, m3 = env.observation_from_a_pose(data, pose, materialize_state_2d=False)
    img, proj, _ = m2._cmr_split
    assert m2.device.type == "meta" and m2.shape == s2.shape
    assert torch.equal(img.permute(0, 3, 1, 2), data["img_geo_feat"])
    check(proj, m3)
    d = r["decided"].reshape(-1)
    assert np.array_equal(ctx.proj_cell.cpu().numpy()[d], r["cell"].reshape(-1)[d])


# ---- pose ------------------------------------------------------------------------------------------------------------------------------------
# One pose_step against float64, per entry of the rotation.  cosf / sinf are within 2 ulp of a value of at most 1, i.e. 4 U.  For
# C = A B with |a|, |b| <= 1, rows of A and columns of B of unit norm: |dC| <= sqrt(3) (dA + dB) + 3 U (three products and two sums whose
# partial sums are at most 1, at most 3 U together with contraction or without).  Rx, Ry, Rz: 4 U each; T = Rx Ry: sqrt(3) 8 U + 3 U < 17 U;
# E = T Rz: sqrt(3) 21 U + 3 U < 40 U; E R with R exact: sqrt(3) 40 U + 3 U < 73 U.
POSE_STEP_TOL = 73 * U


def _cfg(six):
    from cmr_agent_amd.config import KittiConfiguration
    cfg = KittiConfiguration(device=DEV)
    cfg.is_6_DoF = six
    return cfg


def _actions(B, S, six, seed=0):
    r = np.random.RandomState(seed)
    nr, nt = (3, 3) if six else (1, 2)
    ar, at = r.randint(0, S, (B, nr)), r.randint(0, S, (B, nt))
    ar[:S, 0], at[:S, 0], at[S:2 * S, -1] = np.arange(S), np.arange(S), np.arange(S)
    ar[-S:, -1] = np.arange(S)                                              # every index in the last workgroup too
    return torch.from_numpy(ar), torch.from_numpy(at)


def _poses(B, seed=1, t=5.0):
    r = np.random.RandomState(seed)
    q, _ = np.linalg.qr(r.normal(size=(B, 3, 3)))
    q = q * np.sign(np.linalg.det(q)).reshape(B, 1, 1)
    P = np.tile(np.eye(4), (B, 1, 1))
    P[:, :3, :3], P[:, :3, 3] = q, r.uniform(-t, t, (B, 3))
    return torch.from_numpy(P.astype(np.float32))


@pytest.mark.parametrize("six", [False, True], ids=["3dof", "6dof"])
def test_pose_step_at_130_samples(ops, six):
    cfg = _cfg(six)
    B = 130
    P = _poses(B)
    ar, at = _actions(B, 11, six)
    assert set(ar[:, 0].tolist()) == set(range(11)) and set(at[:, 0].tolist()) == set(range(11))
    ref = er.pose_step(P, ar, at, cfg.r_steps, cfg.t_steps, six)
    g = P.clone().to(DEV)
    ops.pose_step(g, ar.to(DEV), at.to(DEV), cfg.r_steps, cfg.t_steps, six)
    got = _np(g)
    assert np.abs(got[:, :3, :3] - ref[:, :3, :3]).max() <= POSE_STEP_TOL
    assert (np.abs(got[:, :3, 3] - ref[:, :3, 3]) <= U * np.abs(ref[:, :3, 3])).all()           # one fp32 sum
    assert np.array_equal(got[:, 3], np.tile([0.0, 0, 0, 1], (B, 1)))
    if not six:                                                            # a yaw step never touches the y row of a pose that has none
        eye = torch.eye(4).repeat(B, 1, 1)
        eye[:, 1, 3] = torch.linspace(-3, 3, B)
        g = eye.clone().to(DEV)
        ops.pose_step(g, ar.to(DEV), at.to(DEV), cfg.r_steps, cfg.t_steps, False)
        assert torch.equal(g[:, 1].cpu(), eye[:, 1])


def test_twenty_6dof_steps_in_sequence(ops):
    cfg = _cfg(True)
    B = 130
    P = _poses(B, seed=4)
    ref = P.double().numpy()
    g = P.clone().to(DEV)
    tmax = float(np.abs(ref[:, :3, 3]).max())
    for k in range(20):
        ar, at = _actions(B, 11, True, seed=10 + k)
        ref = er.pose_step(ref, ar, at, cfg.r_steps, cfg.t_steps, True)
        tmax = max(tmax, float(np.abs(ref[:, :3, 3]).max()))
        ops.pose_step(g, ar.to(DEV), at.to(DEV), cfg.r_steps, cfg.t_steps, True)
    got = _np(g)
    assert np.abs(got[:, :3, :3] - ref[:, :3, :3]).max() <= 20 * POSE_STEP_TOL
    R = got[:, :3, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 20 * POSE_STEP_TOL
    assert np.abs(got[:, :3, 3] - ref[:, :3, 3]).max() <= 20 * U * tmax            # twenty fp32 sums


def test_to_disentangled_and_back(ops, env):
    B, N = 130, 64
    P = _poses(B, seed=2)
    pc = torch.from_numpy(np.random.RandomState(3).uniform(-30, 30, (B, 3, N)).astype(np.float32) + np.float32(7.0))
    pc4 = ops.planar_to_rows4(pc.to(DEV))
    mean4 = ops.colmean(pc4, B, N)
    g = P.clone().to(DEV)
    ops.to_disentangled(g, mean4)
    ref = er.to_disentangled(P, mean4.cpu())
    got = _np(g)
    # t_i - mu_i + (R_i0 mu_0 + R_i1 mu_1 + R_i2 mu_2): 7 roundings, every intermediate at most A_i = |t_i| + |mu_i| + sum_j |R_ij mu_j|
    mu = _np(mean4)[:, :3]
    A = np.abs(_np(P)[:, :3, 3]) + np.abs(mu) + np.einsum("bij,bj->bi", np.abs(_np(P)[:, :3, :3]), np.abs(mu))
    assert (np.abs(got[:, :3, 3] - ref[:, :3, 3]) <= 7 * U * A).all()
    assert np.array_equal(got[:, :3, :3], _np(P)[:, :3, :3]) and np.array_equal(got[:, 3], _np(P)[:, 3])
    # the environment's pair, on the device: back to P within 4 x 2^-23 (|t| + |mu|)
    pcd = pc.to(DEV)
    back = env.from_disentangled(env.to_disentangled(P.clone().to(DEV), pcd), pcd)
    bound = 4 * 2.0 ** -23 * (np.linalg.norm(_np(P)[:, :3, 3], axis=1) + np.linalg.norm(mu, axis=1))
    assert (np.abs(_np(back) - _np(P)).reshape(B, -1).max(1) <= bound).all()


# ---- action heads ----------------------------------------------------------------------------------------------------------------------------
def test_argmax_rows_ties_infinities_and_strides(ops):
    r = np.random.RandomState(63)
    lg = torch.from_numpy(r.uniform(-1, 1, (130, 11)).astype(np.float32))
    lg[5, [2, 7, 9]] = 3.0                                                  # exact duplicates of the maximum: the first index
    lg[64, [10, 0]] = 2.0
    lg[129, [4, 5]] = 1.5
    lg[77] = -math.inf                                                      # nothing is greater than the first element
    lg[78, 1:] = -math.inf
    ref = lg.argmax(1)
    assert ref[5] == 2 and ref[64] == 0 and ref[129] == 4 and ref[77] == 0 and ref[78] == 0
    assert torch.equal(ops.argmax_rows(lg.to(DEV).view(10, 13, 11)).cpu(), ref.view(10, 13))
    assert torch.equal(ops.argmax_rows(lg.to(DEV).view(130, 1, 11)).cpu(), ref.view(130, 1))
    assert torch.equal(ops.argmax_rows(lg.to(DEV).view(1, 130, 11)).cpu(), ref.view(1, 130))
    pad = torch.zeros(8, 24, device=DEV)                                    # the strided view of test_small_heads
    pad[:, :22] = lg[:16].reshape(8, 22).to(DEV)
    assert torch.equal(ops.argmax_rows(pad[:, :22].view(8, 2, 11)).cpu(), ref[:16].view(8, 2))


@pytest.mark.parametrize("rows", er.SOFTMAX_ROWS)
def test_softmax2_rows_thresholds_and_leading_dimension(ops, rows):
    logits = er.softmax_logits(rows)
    ref = er.softmax2(logits)
    wide = torch.full((rows, 4), 50.0, device=DEV)
    wide[:, :2] = logits.to(DEV)
    for src in (logits.to(DEV), wide[:, :2]):                               # ld = 2 and an ld = 4 view
        for lo_t, hi_t in er.SOFTMAX_THRESHOLDS:
            prob, lo, hi = ops.softmax2(src, lo_t, hi_t)
            assert np.abs(_np(prob) - ref).max() <= 1e-6
            for pred, thr in ((lo, lo_t), (hi, hi_t)):
                safe = np.abs(ref - thr) > er.SOFTMAX_GUARD
                assert np.array_equal(pred.cpu().numpy().astype(bool)[safe], (ref > thr)[safe])


def test_softmax2_extreme_logits(ops):
    lg = torch.tensor([[100.0, -100.0], [-100.0, 100.0], [100.0, 99.0], [-100.0, -99.0], [0.0, 30.0], [30.0, 0.0], [100.0, 100.0],
                       [-100.0, -100.0], [0.0, -100.0], [88.0, -88.0]])
    ref = er.softmax2(lg)
    prob = _np(ops.softmax2(lg.to(DEV))[0])
    assert np.isfinite(prob).all()
    as32 = ref.astype(np.float32).astype(np.float64)
    sat = (as32 == 0) | (as32 == 1)
    assert sat.sum() >= 4 and np.array_equal(prob[sat], as32[sat])          # exactly 0 or 1 where float64 rounds to that in fp32
    assert np.abs(prob - ref).max() <= 1e-6


@pytest.mark.parametrize("rows", [1, 17, 3001])
def test_l2norm64_rows_zero_row_and_out_slice(ops, rows):
    """|y| <= 1.  The squared norm: a product and six levels of sums of positive terms, 7 U relative; sqrtf halves that and adds U, the
    division adds U: 5.5 U.  Twice that for the second-order terms: 11 U."""
    x = torch.from_numpy(np.random.RandomState(62 + rows).uniform(-1, 1, (rows, 64)).astype(np.float32))
    x[rows // 2] = 0.0                                                      # an all-zero row gives exactly zeros (0 / 1e-12)
    xd = x.double()
    ref = (xd / xd.norm(dim=1, keepdim=True).clamp_min(1e-12)).numpy()
    got = ops.l2norm64(x.to(DEV))
    assert np.abs(_np(got) - ref).max() <= 11 * U
    assert float(got[rows // 2].abs().max()) == 0
    buf = torch.full((rows, 192), 9.0, device=DEV)
    out = ops.l2norm64(x.to(DEV), out=buf[:, 64:128])
    assert torch.equal(buf[:, 64:128], got) and out.data_ptr() == buf[:, 64:128].data_ptr()
    assert float((buf[:, :64] - 9.0).abs().max()) == 0 and float((buf[:, 128:] - 9.0).abs().max()) == 0


# ---- rollout ---------------------------------------------------------------------------------------------------------------------------------
def test_expert_round_trips_on_the_device(ops):
    """the round trips of the CPU tier: ops.pose_step from the identity, then ops.expert_action, returns the action (3-DoF: every
    (yaw, tx, tz); 6-DoF: single-axis actions only, pose_step composes Rx Ry Rz and the expert decomposes Rz Ry Rx)"""
    (r3, t3), (r6, t6) = er.round_trip_actions(11)
    for six, ar, at in ((False, r3, t3), (True, r6, t6)):
        cfg = _cfg(six)
        B = ar.shape[0]
        eye = torch.eye(4, device=DEV).repeat(B, 1, 1)
        tgt = eye.clone()
        ar_d, at_d = torch.from_numpy(ar).contiguous().to(DEV), torch.from_numpy(at).contiguous().to(DEV)
        ops.pose_step(tgt, ar_d, at_d, cfg.r_steps, cfg.t_steps, six)
        gr, gt = ops.expert_action(eye, tgt, cfg.r_steps, cfg.t_steps, six)
        assert torch.equal(gr, ar_d) and torch.equal(gt, at_d)


@pytest.mark.parametrize("six", [False, True], ids=["3dof", "6dof"])
def test_expert_action_at_132_pairs_and_custom_tables(ops, six):
    src, tgt = er.tiled_rollout_poses()
    cfg = _cfg(six)
    tables = dict(config=(cfg.r_steps.cpu(), cfg.t_steps.cpu()))
    for name, tab in er.CUSTOM_TABLES.items():
        t = torch.tensor(tab, dtype=torch.float64)
        tables[name] = (t, t * 4)
    for name, (rs, ts) in tables.items():
        ar, at, dec = er.expert_action(src, tgt, rs, ts, six)
        gr, gt = ops.expert_action(src.to(DEV), tgt.to(DEV), rs.to(DEV), ts.to(DEV), six)
        assert gr.shape == ar.shape and gt.shape == at.shape
        assert np.array_equal(gr.cpu().numpy()[dec], ar[dec]) and np.array_equal(gt.cpu().numpy()[dec], at[dec]), name
        if name == "duplicate":
            assert int(gr.max()) < 2 and int(gt.max()) < 2                  # ties between twins give the first
        if name == "single":
            assert int(gr.abs().max()) == 0 and int(gt.abs().max()) == 0


@pytest.mark.parametrize("kind", ["a", "b"])
@pytest.mark.parametrize("N", er.REWARD_N)
def test_reward_masks_sizes_and_previous_distance(ops, N, kind):
    pc, cam, mask = er.reward_case(N, kind)
    _, ref = er.reward(pc, cam, mask)
    pcd, camd, md = pc.to(DEV), cam.to(DEV), mask.to(DEV)
    r0, d0 = ops.reward(pcd, camd, md)
    got = _np(d0)
    empty = mask.sum(1).numpy() == 0
    print("N=%d %s: rel err %s" % (N, kind, np.abs(got - ref)[~empty] / ref[~empty]))
    assert np.array_equal(np.isnan(got), empty) and float(r0.abs().max()) == 0
    assert (np.abs(got - ref)[~empty] <= 1e-5 * ref[~empty]).all()
    same, _ = ops.reward(pcd, camd, md, d0)                                  # the device's own distance as prev: exactly 0
    assert float(same.abs().max()) == 0
    # a distance below the previous one earns +0.5, one above costs 0.5 (environment.py:297-300); an empty mask earns 0 either way
    up, _ = ops.reward(pcd, camd, md, d0 + 0.5)
    down, _ = ops.reward(pcd, camd, md, d0 - 0.5)
    want = torch.from_numpy(np.where(empty, 0.0, 0.5)).float()
    assert torch.equal(up.cpu(), want) and torch.equal(down.cpu(), -want)
    ru, _ = er.reward(pc, cam, mask, _np(d0) + 0.5)
    assert np.array_equal(_np(up), ru)


def test_reward_on_a_cloud_far_from_the_origin(ops):
    """the bar is the fp32 torch restatement on the same input: the kernel may be at most 4 times as far from float64 as O.env_reward is
    (the summation orders differ).  Measured errors: DESIGN.md 4x."""
    pc, cam, mask = er.reward_case(2000, "a", offset=er.OFFSET)
    _, ref = er.reward(pc, cam, mask)
    _, d32 = O.env_reward(dict(pc=pc, pc_in_cam_space=cam, pc_mask=mask))
    _, d0 = ops.reward(pc.to(DEV), cam.to(DEV), mask.to(DEV))
    e_kernel = np.abs(_np(d0) - ref) / ref
    e_torch = np.abs(_np(d32.reshape(-1)) - ref) / ref
    print("offset cloud: kernel rel err %s, fp32 torch rel err %s" % (e_kernel, e_torch))
    assert e_kernel.max() <= 4 * e_torch.max()


@pytest.mark.parametrize("T", [1, 10])
@pytest.mark.parametrize("rows", [1, 65, 1000])
def test_discounted_and_advantage(rows, T):
    from cmr_agent_amd.environment import buffer as buf
    rew, val = er.returns_case(rows, T)
    rd, vd = rew.to(DEV), val.to(DEV)
    for gamma in (0.0, 1.0, 0.99):
        ref, scale = er.discounted(rew, gamma)
        got = buf.discounted(rd, gamma)
        assert got.shape == rew.shape and np.abs(_np(got) - ref).max() <= T * 2.0 ** -23 * scale, (gamma,)
        for lam in (0, 0.95):
            ref, scale = er.advantage(rew, val, gamma, lam)
            got = buf.advantage(rd, vd, gamma, lam)
            assert np.abs(_np(got) - ref).max() <= T * 2.0 ** -23 * scale, (gamma, lam)
