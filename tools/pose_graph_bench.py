#!/usr/bin/env python3
"""ops.pose_graph_optimize (csrc/pose_graph.hip) at the size of a KITTI-length sequence: a chain of `--frames` poses on a
closed synthetic path -- a planted yaw and translation bias per odometry edge, so the chained poses drift -- with `--loops` exact loop edges.

  * the whole call at the defaults (iters 20, cg_iters 200), with its launches counted: how many a call issues, how many of them did work
    (from the trace: the executed steps and the CG iterations each used) and how many were early returns;
  * the launch floor: the same call on the same graph with one loop edge turned by 3.1 rad, which is wide, so the call stops at its first
    judgement (status 3) and every later launch is an early return -- what the launches cost when they do nothing;
  * one outer step (iters 1) beside a torch restatement of the same PCG on the device -- block-Jacobi preconditioner by torch.linalg.inv,
    H p by gathers and index_add_, whose sums are in no stated order, run for the CG iterations the kernel used, with no stop test and so
    no host read -- plus the two ops.pose_graph_linearize calls that stand for the step's linearisations.  The two steps are compared.

HIP events round each call, the median over `--repeats` after `--warmup`, the jobs alternating.
python tools/pose_graph_bench.py [--frames 4541] [--loops 200] [--repeats 5] [--warmup 1] [--out profiles/pose_graph_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cmr_agent_amd import ops  # noqa: E402
from cmr_agent_amd.dataset import posegraph  # noqa: E402


def _times_ms(fns, repeats, warmup):
    """the median of each of `fns`, the calls alternating"""
    ms = [[] for _ in fns]
    for it in range(warmup + repeats):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[k].append(e0.elapsed_time(e1))
    return [statistics.median(m) for m in ms]


def _rot(axis, angle):
    K = np.zeros((3, 3))
    K[[2, 0, 1], [1, 2, 0]] = axis
    K[[1, 2, 0], [2, 0, 1]] = -np.asarray(axis)
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def synthetic_lap(F, nloops, seed=0, radius=300.0, yaw_bias=2e-5, trans_bias=2e-4):
    """-> (drifted poses, edges, meas, weights): truth on a closed path of `radius` metres with pitch and roll wobble; the odometry edges
    carry the bias, the loop edges -- the closing pair and drawn pairs at least F / 4 apart -- are exact"""
    truth = np.tile(np.eye(4), (F, 1, 1))
    for n in range(F):
        a = 2.0 * np.pi * n / F
        truth[n, :3, :3] = _rot([0, 0, 1], a + np.pi / 2) @ _rot([0, 1, 0], 0.05 * np.sin(3 * a)) @ _rot([1, 0, 0], 0.05 * np.cos(2 * a))
        truth[n, :3, 3] = radius * np.cos(a), radius * np.sin(a), 2.0 * np.sin(2 * a)
    truth = np.stack([posegraph.inverse(truth[0]) @ x for x in truth])
    edges, meas, weights = posegraph.chain_edges(truth)
    bias = np.eye(4)
    bias[:3, :3], bias[0, 3] = _rot([0, 0, 1], yaw_bias), trans_bias
    meas = meas @ bias
    poses = [np.eye(4)]
    for n in range(F - 1):
        poses.append(poses[n] @ meas[n])
    rng = np.random.default_rng(seed)
    pairs = [(F - 1, 0)]
    while len(pairs) < nloops:
        j = int(rng.integers(0, F - F // 4))
        pairs.append((int(rng.integers(j + F // 4, F)), j))
    loop_edges = [(i, j, posegraph.inverse(truth[j]) @ truth[i], 0.0, 0.0, 1) for i, j in pairs[:nloops]]
    poses = np.stack(poses)
    return (poses,) + posegraph.build_graph(poses, loop_edges)


def torch_pcg(A21, b, edges, F, cg_iters):
    """One outer step's PCG in torch: -> x [F, 6] after exactly cg_iters iterations from x = 0, node 0 fixed"""
    dev = A21.device
    iu = torch.triu_indices(6, 6, device=dev)
    A = torch.zeros((A21.shape[0], 6, 6), dtype=torch.float64, device=dev)
    A[:, iu[0], iu[1]] = A21
    A[:, iu[1], iu[0]] = A21
    i, j = edges[:, 0].long(), edges[:, 1].long()
    free = torch.ones((F, 1), dtype=torch.float64, device=dev)
    free[0] = 0.0
    M = torch.zeros((F, 6, 6), dtype=torch.float64, device=dev).index_add_(0, i, A).index_add_(0, j, A)
    M[0] = torch.eye(6, dtype=torch.float64, device=dev)
    Minv = torch.linalg.inv(M) * free[:, :, None]
    g = torch.zeros((F, 6), dtype=torch.float64, device=dev).index_add_(0, i, b).index_add_(0, j, -b) * free

    def apply(p):
        t = torch.einsum("eab,eb->ea", A, p[i] - p[j])
        return torch.zeros_like(p).index_add_(0, i, t).index_add_(0, j, -t) * free

    x = torch.zeros_like(g)
    r = -g
    z = torch.einsum("nab,nb->na", Minv, r)
    p = z.clone()
    rz = (r * z).sum()
    for _ in range(cg_iters):
        q = apply(p)
        alpha = rz / (p * q).sum()
        x = x + alpha * p
        r = r - alpha * q
        z = torch.einsum("nab,nb->na", Minv, r)
        rz_new = (r * z).sum()
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4541)
    ap.add_argument("--loops", type=int, default=200)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cg-iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    F, iters, cg = args.frames, args.iters, args.cg_iters
    graph = synthetic_lap(F, args.loops)
    P, E, Z, W = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in graph)
    wide = graph[2].copy()
    wide[-1, :3, :3] = wide[-1, :3, :3] @ _rot([0, 0, 1], 3.1)
    Zw = torch.from_numpy(wide).to(dev)
    nE = E.shape[0]

    full = ops.pose_graph_optimize(P, E, Z, W, iters=iters, cg_iters=cg)
    floor = ops.pose_graph_optimize(P, E, Zw, W, iters=iters, cg_iters=cg)
    one = ops.pose_graph_optimize(P, E, Z, W, iters=1, cg_iters=cg)
    assert floor.status == 3 and floor.iterations == 0
    used = [int(v) for v in full.trace[:full.iterations, 1]]
    launches = 2 * (iters + 1) + iters * (2 + 2 * cg) + 2
    # the launches that did work: init and final, a linearisation and a judgement per executed step and one more pair after the last, the
    # node blocks and the step, and per CG iteration two -- plus the apply that saw CG converge, when it stopped short of cg_iters
    live = 2 + 2 * (full.iterations + 1) + sum(2 + 2 * u + (1 if u < cg else 0) for u in used)
    live = min(live, launches)
    used1 = int(one.trace[0, 1])

    def torch_step():
        a = ops.pose_graph_linearize(P, E, Z, W)
        x = torch_pcg(a.A, a.b, E, F, used1)
        ops.pose_graph_linearize(P, E, Z, W)
        return x

    x = torch_step()
    # the step's translation part from the pose change: X' = [Exp(w) | v] X gives v = t' - R' R^T t
    dv = one.poses[:, :3, 3] - torch.einsum("nab,nb->na", one.poses[:, :3, :3] @ P[:, :3, :3].transpose(1, 2), P[:, :3, 3])
    diff = float((dv - x[:, 3:]).norm() / x[:, 3:].norm())
    full_ms, floor_ms, one_ms, torch_ms = _times_ms([lambda: ops.pose_graph_optimize(P, E, Z, W, iters=iters, cg_iters=cg),
                                                     lambda: ops.pose_graph_optimize(P, E, Zw, W, iters=iters, cg_iters=cg),
                                                     lambda: ops.pose_graph_optimize(P, E, Z, W, iters=1, cg_iters=cg), torch_step],
                                                    args.repeats, args.warmup)
    lines = ["%d poses on a closed path, %d odometry + %d loop edges, iters %d, cg_iters %d: ops.pose_graph_optimize whole call %.3f ms; cost %.4e -> "
             "%.4e, %d steps, status %d, CG iterations per step %s" % (F, F - 1, nE - F + 1, iters, cg, full_ms, float(full.trace[0, 0]) if full.iterations else full.cost,
                                                                        full.cost, full.iterations, full.status, used),
             "    launches per call %d, of which %d did work and %d (%.1f %%) were early returns" % (launches, live, launches - live,
                                                                                                    100.0 * (launches - live) / launches),
             "    the launch floor -- the same call stopped at its first judgement by a wide edge (status 3), every later launch an early return: "
             "%.3f ms = %.2f us per launch" % (floor_ms, 1e3 * floor_ms / launches),
             "    so of the whole call %.3f ms is the floor of its %d launches and %.3f ms is left for the %d that work = %.2f us each on top" % (
                 floor_ms, launches, full_ms - floor_ms, live, 1e3 * (full_ms - floor_ms) / max(live, 1)),
             "one outer step (iters 1, %d CG iterations used): ops.pose_graph_optimize %.3f ms;  torch on the device -- two ops.pose_graph_linearize, "
             "torch.linalg.inv blocks, index_add_ products, %d CG iterations, no stop test: %.3f ms;  x %.2f" % (used1, one_ms, used1, torch_ms, torch_ms / one_ms),
             "    the two steps' translations differ by %.3e of their norm (index_add_ sums in no stated order)" % diff]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
