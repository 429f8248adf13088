"""CPU tier of the pose-graph solve: the contract's restatement (tests/pose_graph_reference.py) against central differences and
against an independent dense solver, the wrappers' and the command's argument checks, the incidence CSR, the command end to end on the
restatement as a stand-in for the device, and the work model's entries.  No kernel runs here."""
import math
import os

import numpy as np
import pytest
import torch

import pose_graph_reference as ref
from cmr_agent_amd import ops
from cmr_agent_amd.dataset import align, posegraph

EPS = 2.0 ** -52


def _random_pose(rng, spread=3.0):
    return ref.make_pose(ref.exp_so3(rng.normal(size=3)), rng.normal(size=3) * spread)


@pytest.mark.parametrize("theta", [0.0, 1e-10, 1e-4, 0.5, 2.5])
def test_jacobian_against_central_differences(theta):
    """The hand-derived J against (r(xi = +h e_q) - r(-h e_q)) / 2h of the restated residual, at both ends of the edge.  The bar is the
    quotient's own error: truncation h^2 |r'''| / 6 and rounding eps |r| / h; r's derivatives grow with the lever arms, so both carry
    (1 + |t_i| + |t_j|)^2, and a factor 10 stands for the constants."""
    rng = np.random.default_rng(int(theta * 1e6) % 1000 + 3)
    Xi, Xj = _random_pose(rng), _random_pose(rng)
    axis = rng.normal(size=3)
    D = ref.make_pose(ref.exp_so3(axis / np.linalg.norm(axis) * theta), rng.normal(size=3))
    Z = ref.inv_pose(Xj) @ Xi @ ref.inv_pose(D)                      # so that the residual's rotation is theta
    r, th = ref.residual(Xi, Xj, Z)
    assert abs(th - theta) <= 1e-12
    J = ref.jacobian(Xi, Xj, Z)
    h = 1e-5
    bar = 10.0 * (h * h + EPS / h) * (1.0 + np.linalg.norm(Xi[:3, 3]) + np.linalg.norm(Xj[:3, 3])) ** 2
    for q in range(6):
        d = np.zeros(6)
        d[q] = h
        at_i = (ref.residual(ref.left_update(Xi, d), Xj, Z)[0] - ref.residual(ref.left_update(Xi, -d), Xj, Z)[0]) / (2 * h)
        at_j = (ref.residual(Xi, ref.left_update(Xj, d), Z)[0] - ref.residual(Xi, ref.left_update(Xj, -d), Z)[0]) / (2 * h)
        assert np.abs(J[:, q] - at_i).max() <= bar, (q, np.abs(J[:, q] - at_i).max(), bar)
        assert np.abs(-J[:, q] - at_j).max() <= bar, (q, np.abs(J[:, q] + at_j).max(), bar)


@pytest.mark.parametrize("theta", [0.0, 1e-10, 1e-9, 1e-4, 0.5, 2.5, 3.0])
def test_log_of_exp_round_trip(theta):
    """Log(Exp(phi)) = phi.  atan2(s, c) is well conditioned everywhere; the direction a / s loses digits as s = sin theta falls, so the bar
    is 16 eps max(1, theta / sin theta) -- 16 for the few dozen operations of Exp and Log."""
    rng = np.random.default_rng(5)
    axis = rng.normal(size=3)
    phi = axis / np.linalg.norm(axis) * theta
    back, th = ref.log_so3(ref.exp_so3(phi))
    bar = 16.0 * EPS * max(1.0, theta / math.sin(theta) if theta > 0 else 1.0)
    assert np.abs(back - phi).max() <= bar and abs(th - theta) <= bar


def test_wide_edge_is_counted():
    Xi, Xj = np.eye(4), np.eye(4)
    Z = ref.make_pose(ref.exp_so3([0.0, 0.0, 3.1]), [0.0, 0.0, 0.0])
    t = ref.edge_terms(np.stack([Xi, Xj]), np.array([[0, 1]], np.int32), Z[None], np.ones((1, 2)))
    assert t.wide == 1 and abs(t.theta[0] - 3.1) < 1e-12


def test_huber_terms():
    g = ref.drifted(40, 6)
    plain = ref.edge_terms(g.poses, g.edges, g.meas, g.weights)
    k = float(np.median(plain.chi[plain.chi > 0]))
    hub = ref.edge_terms(g.poses, g.edges, g.meas, g.weights, k)
    out = plain.chi > k
    assert out.any() and (~out).any()
    assert np.array_equal(hub.scale[~out], np.ones((~out).sum())) and np.allclose(hub.scale[out], k / plain.chi[out], rtol=1e-15)
    assert np.allclose(hub.costs[out], k * plain.chi[out] - 0.5 * k * k, rtol=1e-15) and np.array_equal(hub.costs[~out], plain.costs[~out])
    assert np.allclose(hub.A, plain.A * hub.scale[:, None], rtol=1e-14) and np.allclose(hub.b, plain.b * hub.scale[:, None], rtol=1e-14)


@pytest.mark.parametrize("maker,F,loops", [(ref.drifted, 40, 6), (ref.drifted, 65, 3)])
def test_stated_order_pcg_against_the_dense_solve(maker, F, loops):
    """The Laplacian-form PCG of the contract against np.linalg.solve on the system assembled from the Jacobians: |x - delta| <= 4 cond_2(H)
    cg_tol |delta|, the first-order bound of a solve stopped at a relative preconditioned residual of cg_tol."""
    g = maker(F, loops)
    fixed = ref.default_fixed(F)
    delta, cond = ref.dense_step(g.poses, g.edges, g.meas, g.weights, fixed)
    assert cond < 1e10
    t = ref.edge_terms(g.poses, g.edges, g.meas, g.weights)
    s = ref.pcg(t.A, t.b, g.edges, F, fixed, 0.0, 6 * F, 1e-12)
    assert not s.singular and s.used < 6 * F and s.rel <= 1e-12
    assert np.linalg.norm(s.x - delta) <= 4.0 * cond * 1e-12 * np.linalg.norm(delta)
    assert np.array_equal(s.x[0], np.zeros(6))


def test_restatement_converges_to_the_dense_solvers_poses():
    g = ref.drifted(40, 6)
    fixed = ref.default_fixed(40)
    res = ref.optimize(g.poses, g.edges, g.meas, g.weights)
    assert res.status == 0 and res.cost < ref.edge_terms(g.poses, g.edges, g.meas, g.weights).cost
    conv = ref.dense_gauss_newton(g.poses, g.edges, g.meas, g.weights, fixed)
    d = np.array([ref.left_delta(a, b) for a, b in zip(res.poses, conv)])
    assert np.abs(d).max() <= 1e-9                                    # the outer tolerances


def test_restatement_statuses():
    g = ref.ring(8, 1)
    lonely = np.concatenate([g.poses, np.eye(4)[None]])               # a ninth pose without edges
    assert ref.optimize(lonely, g.edges, g.meas, g.weights).status == 2
    assert ref.optimize(lonely, g.edges, g.meas, g.weights, damping=1e-6).status == 0
    meas = g.meas.copy()
    meas[-1] = meas[-1] @ ref.make_pose(ref.exp_so3([0.0, 0.0, 3.1]), [0.0, 0.0, 0.0])
    res = ref.optimize(g.poses, g.edges, meas, g.weights)
    assert res.status == 3 and np.array_equal(res.poses, g.poses)
    d = ref.drifted(40, 6)
    assert ref.optimize(d.poses, d.edges, d.meas, d.weights, iters=1).status == 1


def test_incidence_by_hand():
    """Four nodes, five edges, edge 3 a duplicate of edge 0:  0: (1, 0)  1: (2, 1)  2: (3, 0)  3: (1, 0)  4: (0, 2)"""
    edges = np.array([[1, 0], [2, 1], [3, 0], [1, 0], [0, 2]], np.int32)
    offsets, numbers, signs = [0, 4, 7, 9, 10], [0, 2, 3, 4, 0, 1, 3, 1, 4, 2], [-1, -1, -1, 1, 1, -1, 1, 1, -1, 1]
    for got in (ref.incidence(edges, 4), [t.numpy() for t in ops.pose_graph_incidence(torch.from_numpy(edges), 4)]):
        assert [a.tolist() for a in got] == [offsets, numbers, signs]
        assert all(a.dtype == np.int32 for a in got)
    o, n, s = ops.pose_graph_incidence(torch.zeros((0, 2), dtype=torch.int32), 3)
    assert o.tolist() == [0, 0, 0, 0] and n.numel() == 0 and s.numel() == 0


def test_chain_edges_have_zero_residuals_at_the_chain():
    g = ref.drifted(40, 6)
    edges, meas, weights = posegraph.chain_edges(g.poses, 0.002, 0.05)
    assert edges.dtype == np.int32 and edges.tolist() == [[n + 1, n] for n in range(39)]
    assert np.allclose(weights, [[250000.0, 400.0]] * 39, rtol=1e-12)
    t = ref.edge_terms(g.poses, edges, meas, weights)
    assert np.abs(t.r).max() <= 64 * EPS * 10.0 and t.cost <= 1e-18   # lever arms of 10 m


def test_project_rotations():
    rng = np.random.default_rng(2)
    P = np.stack([_random_pose(rng) for _ in range(5)])
    Q = P.copy()
    Q[:, :3, :3] = Q[:, :3, :3].astype(np.float32)
    R = posegraph.project_rotations(Q)
    assert np.abs(R[:, :3, :3] @ R[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() <= 8 * EPS
    assert np.allclose(np.linalg.det(R[:, :3, :3]), 1.0) and np.abs(R - P).max() <= 1e-6 and np.array_equal(R[:, :3, 3], Q[:, :3, 3])


# ---- argument checks --------------------------------------------------------------------------------------------------------------------------
def _graph_tensors(F=5):
    g = ref.ring(F, 1)
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in (g.poses, g.edges, g.meas, g.weights)]


def _bad_graphs():
    P, E, Z, W = _graph_tensors()
    yield "poses dtype", (P.float(), E, Z, W)
    yield "poses shape", (P[:, :3], E, Z, W)
    yield "poses type", (P.numpy(), E, Z, W)
    yield "edges dtype", (P, E.long(), Z, W)
    yield "edges shape", (P, E.reshape(-1), Z, W)
    yield "meas dtype", (P, E, Z.float(), W)
    yield "meas shape", (P, E, Z[:-1], W)
    yield "weights dtype", (P, E, Z, W.float())
    yield "weights shape", (P, E, Z, W[:, :1])
    yield "no pose", (P[:0], E[:0], Z[:0], W[:0])
    same = E.clone()
    same[1, 0] = same[1, 1]
    yield "i == j", (P, same, Z, W)
    for v in (-1, 5):
        out = E.clone()
        out[2, 1] = v
        yield "index %d" % v, (P, out, Z, W)
    for v in (-1.0, math.nan, math.inf):
        w = W.clone()
        w[0, 1] = v
        yield "weight %r" % v, (P, E, Z, w)
    p = P.clone()
    p[1, 0, 3] = math.inf
    yield "poses finite", (p, E, Z, W)
    z = Z.clone()
    z[0, 1, 1] = math.nan
    yield "meas finite", (P, E, z, W)
    yield "mixed devices", (P.to("meta"), E, Z, W)


@pytest.mark.parametrize("what,graph", list(_bad_graphs()), ids=[w for w, _ in _bad_graphs()])
def test_wrappers_refuse_a_bad_graph(what, graph):
    with pytest.raises(ValueError, match="pose_graph_linearize"):
        ops.pose_graph_linearize(*graph)
    with pytest.raises(ValueError, match="pose_graph_optimize"):
        ops.pose_graph_optimize(*graph)


@pytest.mark.parametrize("kw", [dict(huber=-1.0), dict(huber=math.nan), dict(huber=math.inf), dict(huber="3"[:0]), dict(huber=True),
                                dict(iters=-1), dict(iters=ops.PG_MAX_ITERS + 1), dict(iters=1.5), dict(iters=True),
                                dict(cg_iters=-1), dict(cg_iters=ops.PG_MAX_CG_ITERS + 1), dict(cg_tol=-1e-9), dict(cg_tol=math.nan),
                                dict(damping=-1.0), dict(damping=math.inf), dict(tol_rot=-1.0), dict(tol_rot=math.nan), dict(tol_trans=-1.0),
                                dict(tol_trans=math.inf)])
def test_optimize_refuses_a_bad_scalar(kw):
    with pytest.raises(ValueError, match="pose_graph_optimize"):
        ops.pose_graph_optimize(*_graph_tensors(), **kw)
    if "huber" in kw:
        with pytest.raises(ValueError, match="pose_graph_linearize"):
            ops.pose_graph_linearize(*_graph_tensors(), **kw)


def test_optimize_refuses_bad_fixed_and_a_cpu_graph():
    P, E, Z, W = _graph_tensors()
    for fixed in (torch.ones(5, dtype=torch.bool), torch.zeros(4, dtype=torch.bool), torch.zeros(5, dtype=torch.uint8), [True] + [False] * 4,
                  torch.zeros(5, dtype=torch.bool, device="meta")):
        with pytest.raises(ValueError, match="pose_graph_optimize"):
            ops.pose_graph_optimize(P, E, Z, W, fixed)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.pose_graph_optimize(P, E, Z, W)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.pose_graph_linearize(P, E, Z, W)
    with pytest.raises(ValueError, match="pose_graph_incidence"):
        ops.pose_graph_incidence(E.long(), 5)
    with pytest.raises(ValueError, match="pose_graph_incidence"):
        ops.pose_graph_incidence(E, 4)
    with pytest.raises(ValueError, match="pose_graph_incidence"):
        ops.pose_graph_incidence(E, 0)


def test_sizes_at_or_beyond_2_to_31_are_refused():
    E = (1 << 31) // 28 + 1
    big = [torch.empty((2, 4, 4), dtype=torch.float64, device="meta"), torch.empty((E, 2), dtype=torch.int32, device="meta"),
           torch.empty((E, 4, 4), dtype=torch.float64, device="meta"), torch.empty((E, 2), dtype=torch.float64, device="meta")]
    with pytest.raises(ValueError, match="2\\^31"):
        ops.pose_graph_optimize(*big)
    F = (1 << 31) // 6 + 1
    big = [torch.empty((F, 4, 4), dtype=torch.float64, device="meta"), torch.empty((1, 2), dtype=torch.int32, device="meta"),
           torch.empty((1, 4, 4), dtype=torch.float64, device="meta"), torch.empty((1, 2), dtype=torch.float64, device="meta")]
    with pytest.raises(ValueError, match="2\\^31"):
        ops.pose_graph_linearize(*big)


def test_empty_graphs_launch_nothing():
    """E = 0 and F = 1 return before the library is touched: they pass on CPU tensors, where any launch would be refused"""
    P, E, Z, W = _graph_tensors()
    res = ops.pose_graph_optimize(P, E[:0], Z[:0], W[:0], iters=3)
    assert res.status == 0 and res.iterations == 0 and res.cost == 0.0 and torch.equal(res.poses, P) and res.poses is not P
    assert res.trace.shape == (3, 5) and not res.trace.any()
    res = ops.pose_graph_optimize(P[:1], E[:0], Z[:0], W[:0])
    assert res.status == 0 and torch.equal(res.poses, P[:1])
    t = ops.pose_graph_linearize(P, E[:0], Z[:0], W[:0])
    assert t.cost == 0.0 and t.wide == 0 and t.A.shape == (0, 21) and t.r.shape == (0, 6) and t.chi.shape == (0,)
    assert ops.PG_STATUS[0] == "converged" and len(ops.PG_STATUS) == 4 and ops.PG_MAX_ITERS >= 20 and ops.PG_MAX_CG_ITERS >= 200


# ---- the command ------------------------------------------------------------------------------------------------------------------------------
def _stand_ins(monkeypatch):
    """ops.pose_graph_linearize / optimize restated by tests/pose_graph_reference.py on CPU tensors"""
    def linearize(poses, edges, meas, weights, huber=0.0):
        t = ref.edge_terms(poses.numpy(), edges.numpy(), meas.numpy(), weights.numpy(), huber)
        return ops.PoseGraphTerms(*(torch.from_numpy(a) for a in (t.r, t.chi, t.scale, t.A, t.b)), t.cost, t.wide)

    def optimize(poses, edges, meas, weights, fixed=None, *a):
        r = ref.optimize(poses.numpy(), edges.numpy(), meas.numpy(), weights.numpy(), fixed, *a)
        return ops.PoseGraphResult(torch.from_numpy(r.poses), r.cost, r.iterations, r.status, torch.from_numpy(r.trace))
    monkeypatch.setattr(ops, "pose_graph_linearize", linearize)
    monkeypatch.setattr(ops, "pose_graph_optimize", optimize)


def test_command_end_to_end_on_stand_ins(tmp_path, monkeypatch, capsys):
    _stand_ins(monkeypatch)
    g = ref.drifted(40, 6)
    poses, edges = ref.write_graph_files(tmp_path, g, first=100)
    out = str(tmp_path / "out.txt")
    posegraph.main(["--poses", poses, "--edges", edges, "--out", out, "--first", "100"], device=torch.device("cpu"))
    lines = capsys.readouterr().out.splitlines()
    assert sum(l.startswith("edge ") for l in lines) == 6 and lines[0].startswith("edge 139 100: chi ")
    assert lines[-1].startswith("posegraph: cost ") and " status 0 moved " in lines[-1]
    assert sum(l.startswith("iter ") for l in lines) == int(lines[-1].split(" iterations ")[1].split()[0])
    # what the command solved: the poses as the file holds them, projected, the chain from them, the loop edges from their file
    P = posegraph.project_rotations(align.read_poses(poses))
    E, Z, W = posegraph.build_graph(P, align.read_edges(edges), 100)
    assert len(E) == 45 and E[39:].tolist() == g.edges[39:].tolist()
    want = ref.optimize(P, E, Z, W, None, 3.0)
    got = align.read_poses(out)                                       # accumulate --poses reads the file through this
    assert got.shape == (40, 4, 4)
    assert np.abs(got - want.poses).max() <= 1e-9 * max(1.0, np.abs(want.poses).max())     # the %.9e round trip
    before = np.mean([np.linalg.norm(ref.left_delta(a, b)) for a, b in zip(P, g.truth)])
    after = np.mean([np.linalg.norm(ref.left_delta(a, b)) for a, b in zip(got, g.truth)])
    assert after < before


@pytest.mark.parametrize("extra", [["--first", "1"], ["--first", "-1"], ["--odom-sigma-t", "0"], ["--loop-sigma-r", "nan"], ["--huber", "-1"],
                                   ["--iters", "101"], ["--cg-iters", "-1"], ["--cg-tol", "inf"], ["--damping", "-1"], ["--tol-rot", "-1"],
                                   ["--tol-trans", "nan"]])
def test_command_refuses_bad_arguments(tmp_path, monkeypatch, extra):
    _stand_ins(monkeypatch)
    poses, edges = ref.write_graph_files(tmp_path, ref.drifted(10, 2))
    with pytest.raises(SystemExit):                                   # --first 1: the closing edge (9, 0) lies outside frames [1, 11)
        posegraph.main(["--poses", poses, "--edges", edges, "--out", str(tmp_path / "o.txt")] + extra, device=torch.device("cpu"))
    assert not os.path.exists(str(tmp_path / "o.txt"))


def test_command_refuses_bad_files(tmp_path, monkeypatch):
    _stand_ins(monkeypatch)
    poses, edges = ref.write_graph_files(tmp_path, ref.drifted(10, 2))
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("1 2 3\n")
    for argv in (["--poses", bad, "--edges", edges], ["--poses", poses, "--edges", bad], ["--poses", poses], ["--edges", edges]):
        with pytest.raises(SystemExit):
            posegraph.main(argv + ["--out", str(tmp_path / "o.txt")], device=torch.device("cpu"))
    with pytest.raises(ValueError, match="two different frames"):
        posegraph.build_graph(np.tile(np.eye(4), (3, 1, 1)), [(1, 1, np.eye(4), 0.0, 0.0, 1)])


def test_documents_point_to_the_command():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from cmr_agent_amd.dataset import loops
    assert "dataset.posegraph" in loops.__doc__ and "is not here" not in loops.__doc__
    for name in ("README.md", "DESIGN.md", os.path.join("tools", "README.md")):
        assert "pose_graph" in open(os.path.join(root, name)).read() or "posegraph" in open(os.path.join(root, name)).read(), name
    assert "tuned on real data" in posegraph.__doc__ and "SO(3)" in posegraph.__doc__


def test_workmodel_prices_the_entry_points():
    from cmr_agent_amd import _lib
    from cmr_agent_amd.utils import workmodel
    protos = _lib.parse_header()
    for name in ("cmr_pose_graph_linearize_f64", "cmr_pose_graph_optimize_f64"):
        assert name in protos and name in workmodel.WORK, name
    assert workmodel.WORK["cmr_pose_graph_linearize_f64"](dict(E=100)) == (60000.0, 100 * 680)
    fl, by = workmodel.WORK["cmr_pose_graph_optimize_f64"](dict(F=10, E=20, iters=2, cg_iters=3))
    assert fl == 3 * 600.0 * 20 + 2 * (7000.0 + 3 * (168.0 * 20 + 1000.0)) and by > 0
    assert protos["cmr_pose_graph_optimize_f64"][2][:6] == ["poses_in", "F", "edges", "meas", "weights", "E"]
