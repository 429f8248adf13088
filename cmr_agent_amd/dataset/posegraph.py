"""Chained poses and loop edges -> the poses of a pose-graph solve over both.

    --poses FILE      the poses `align --out` writes: line n maps frame A + n into frame A                                  (read)
    --edges FILE      the loop edges `loops --out` writes: i j, the pose that maps frame i into frame j, dist rmse pairs    (read)
    --out FILE        the corrected poses, as `accumulate --poses` reads them                                              (written)

The graph's nodes are the poses; its edges are one odometry edge per consecutive pair -- the file's own inv(P_n) P_{n+1}, so the chain
itself has zero residual -- at the weights 1 / sigma^2 of --odom-sigma-r (rad) and --odom-sigma-t (m), and the loop edges at those of
--loop-sigma-r and --loop-sigma-t.  The files hold float32 digits, so each rotation read is first projected onto SO(3) (U V^T of its
SVD, in numpy).  The loop edges' i and j are frame numbers; --first is the frame number of the first pose line.  The first pose is held
fixed.  `ops.pose_graph_optimize` (HIP, csrc/pose_graph.hip) solves: Gauss-Newton with a Huber weight on every edge's chi (--huber, 0 =
off), the linear system by preconditioned conjugate gradients, all on the device.  One line per loop edge, with its chi before and after
the solve and its final Huber factor -- a loop that stays far out is a wrong loop --

    edge <i> <j>: chi <before> -> <after> scale <s>

one per outer iteration,

    iter <k>: cost <c> cg <iterations> rel <residual> step <rad> <m>

and the closing line, `moved` being the largest change of any pose:

    posegraph: cost <a> -> <b> iterations <k> status <s> moved <metres> <degrees>

No default of this command is tuned on real data.

    python -m cmr_agent_amd.dataset.posegraph --poses FILE --edges FILE --out FILE [--first A --odom-sigma-t 0.05 --odom-sigma-r 0.002
                                              --loop-sigma-t 0.1 --loop-sigma-r 0.005 --huber 3.0 --iters 20 --cg-iters 200 --cg-tol 1e-8
                                              --damping 0 --tol-rot 1e-9 --tol-trans 1e-9]
"""
import argparse
import math

import numpy as np
import torch

from .. import ops
from . import align, loops


# ---- the rules: plain functions ---------------------------------------------------------------------------------------------------------------
def project_rotations(poses):
    """float64 [F, 4, 4] -> the same with every rotation replaced by the nearest one (U V^T of its SVD, the sign fixed to det +1)"""
    out = np.array(poses, np.float64)
    U, _, Vt = np.linalg.svd(out[:, :3, :3])
    U[:, :, 2] *= np.sign(np.linalg.det(U @ Vt))[:, None]
    out[:, :3, :3] = U @ Vt
    return out


def inverse(P):
    T = np.eye(4)
    T[:3, :3] = P[:3, :3].T
    T[:3, 3] = -P[:3, :3].T @ P[:3, 3]
    return T


def chain_edges(poses, sigma_r=0.002, sigma_t=0.05):
    """-> (edges int32 [F - 1, 2], meas float64 [F - 1, 4, 4], weights float64 [F - 1, 2]): one edge (n + 1, n, inv(P_n) P_{n+1}) per
    consecutive pair at the odometry weights 1 / sigma^2"""
    F = len(poses)
    edges = np.stack([np.arange(1, F), np.arange(0, F - 1)], 1).astype(np.int32)
    meas = np.stack([inverse(poses[n]) @ poses[n + 1] for n in range(F - 1)]) if F > 1 else np.zeros((0, 4, 4))
    return edges, meas, np.tile([1.0 / sigma_r ** 2, 1.0 / sigma_t ** 2], (F - 1, 1))


def build_graph(poses, loop_edges, first=0, odom_sigma_r=0.002, odom_sigma_t=0.05, loop_sigma_r=0.005, loop_sigma_t=0.1):
    """poses float64 [F, 4, 4] and the list align.read_edges gives -> (edges, meas, weights) of the chain followed by the loop edges, their
    frame numbers turned into positions by `first`, their rotations projected.  ValueError for an edge outside the poses or onto itself."""
    F = len(poses)
    edges, meas, weights = chain_edges(poses, odom_sigma_r, odom_sigma_t)
    for i, j, _, _, _, _ in loop_edges:
        if not (first <= i < first + F and first <= j < first + F) or i == j:
            raise ValueError("edge %d %d: need two different frames in [%d, %d)" % (i, j, first, first + F))
    if loop_edges:
        edges = np.concatenate([edges, np.array([(i - first, j - first) for i, j, *_ in loop_edges], np.int32)])
        meas = np.concatenate([meas, project_rotations(np.stack([T for _, _, T, *_ in loop_edges]))])
        weights = np.concatenate([weights, np.tile([1.0 / loop_sigma_r ** 2, 1.0 / loop_sigma_t ** 2], (len(loop_edges), 1))])
    return edges, meas, weights


def moved(before, after):
    """-> (metres, degrees): the largest change of any pose"""
    m = d = 0.0
    for a, b in zip(before, after):
        dm, dd = loops.drift([a, b], 0, 1, np.eye(4))
        m, d = max(m, dm), max(d, dd)
    return m, d


def solve(poses, edges, meas, weights, huber=3.0, iters=20, cg_iters=200, cg_tol=1e-8, damping=0.0, tol_rot=1e-9, tol_trans=1e-9, loops_from=None,
          first=0, device=None, report=print):
    """The graph on the device -> (corrected poses float64 [F, 4, 4] numpy, ops.PoseGraphResult); reports the lines of the docstring, the
    edge lines for the edges from position `loops_from` on."""
    device = align.on_device(device)
    P, Ed, Z, W = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (poses, edges, meas, weights))
    before = ops.pose_graph_linearize(P, Ed, Z, W, huber)
    res = ops.pose_graph_optimize(P, Ed, Z, W, None, huber, iters, cg_iters, cg_tol, damping, tol_rot, tol_trans)
    after = ops.pose_graph_linearize(res.poses, Ed, Z, W, huber)
    chi0, chi1, scale = before.chi.cpu().numpy(), after.chi.cpu().numpy(), after.scale.cpu().numpy()
    for e in range(len(edges) if loops_from is None else loops_from, len(edges)):
        report("edge %d %d: chi %.4f -> %.4f scale %.4f" % (edges[e][0] + first, edges[e][1] + first, chi0[e], chi1[e], scale[e]))
    for k in range(res.iterations):
        c, used, rel, dw, dv = res.trace[k].tolist()
        report("iter %d: cost %.6e cg %d rel %.3e step %.3e %.3e" % (k, c, int(used), rel, dw, dv))
    out = res.poses.cpu().numpy()
    report("posegraph: cost %.6e -> %.6e iterations %d status %d moved %.4f %.4f" % ((before.cost, res.cost, res.iterations, res.status) + moved(poses, out)))
    return out, res


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cmr_agent_amd.dataset.posegraph", description=__doc__.split("\n\n")[0],
                                 epilog="No default of this command is tuned on real data.")
    ap.add_argument("--poses", required=True, help="the chained poses, 12 numbers per line (align --out)")
    ap.add_argument("--edges", required=True, help="the loop edges: i j, 12 numbers of the pose of i in j, dist rmse pairs (loops --out)")
    ap.add_argument("--out", required=True, help="write the corrected poses here, 12 numbers per line (accumulate --poses reads them)")
    ap.add_argument("--first", type=int, default=0, help="the frame number of the first pose line (default 0)")
    ap.add_argument("--odom-sigma-t", type=float, default=0.05, help="metres of an odometry edge (default 0.05, not tuned on real data)")
    ap.add_argument("--odom-sigma-r", type=float, default=0.002, help="radians of an odometry edge (default 0.002, not tuned on real data)")
    ap.add_argument("--loop-sigma-t", type=float, default=0.1, help="metres of a loop edge (default 0.1, not tuned on real data)")
    ap.add_argument("--loop-sigma-r", type=float, default=0.005, help="radians of a loop edge (default 0.005, not tuned on real data)")
    ap.add_argument("--huber", type=float, default=3.0, help="edges with chi above this are down-weighted; 0 = off (default 3.0, not tuned on real data)")
    ap.add_argument("--iters", type=int, default=20, help="most Gauss-Newton steps (default 20)")
    ap.add_argument("--cg-iters", type=int, default=200, help="most conjugate-gradient iterations per step (default 200)")
    ap.add_argument("--cg-tol", type=float, default=1e-8, help="relative residual at which conjugate gradients stop (default 1e-8)")
    ap.add_argument("--damping", type=float, default=0.0, help="added to the system's diagonal (default 0)")
    ap.add_argument("--tol-rot", type=float, default=1e-9, help="stop when no pose turns by more than this many radians (default 1e-9)")
    ap.add_argument("--tol-trans", type=float, default=1e-9, help="and none moves by more than this many metres (default 1e-9)")
    args = ap.parse_args(argv)
    for name in ("odom_sigma_t", "odom_sigma_r", "loop_sigma_t", "loop_sigma_r"):
        v = getattr(args, name)
        if not (0.0 < v < math.inf):
            ap.error("--%s must be finite and > 0, got %r" % (name.replace("_", "-"), v))
    for name in ("huber", "cg_tol", "damping", "tol_rot", "tol_trans"):
        v = getattr(args, name)
        if not (0.0 <= v < math.inf):
            ap.error("--%s must be finite and >= 0, got %r" % (name.replace("_", "-"), v))
    if args.first < 0:
        ap.error("--first must be >= 0")
    if not 0 <= args.iters <= ops.PG_MAX_ITERS:
        ap.error("--iters must lie in [0, %d]" % ops.PG_MAX_ITERS)
    if not 0 <= args.cg_iters <= ops.PG_MAX_CG_ITERS:
        ap.error("--cg-iters must lie in [0, %d]" % ops.PG_MAX_CG_ITERS)
    return ap, args


def main(argv=None, device=None):
    ap, args = parse_args(argv)
    try:
        poses = project_rotations(align.read_poses(args.poses))
        loop_edges = align.read_edges(args.edges)
        edges, meas, weights = build_graph(poses, loop_edges, args.first, args.odom_sigma_r, args.odom_sigma_t, args.loop_sigma_r, args.loop_sigma_t)
    except ValueError as e:
        ap.error(str(e))
    try:
        out, _ = solve(poses, edges, meas, weights, args.huber, args.iters, args.cg_iters, args.cg_tol, args.damping, args.tol_rot, args.tol_trans,
                       loops_from=len(poses) - 1, first=args.first, device=device)
    except ValueError as e:
        ap.error(str(e))
    align.write_poses(args.out, out)


if __name__ == "__main__":
    main()
