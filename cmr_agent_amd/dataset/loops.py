"""Prepared clouds of a sequence -> the loop edges between frames taken at the same place long apart.

    <root>/<data_velodyne>/sequences/<seq>/voxel0.1-SNr0.6/<i>.npy        float32 [7, n]: x, y, z, reflectance, nx, ny, nz   (read)

Every frame gets a ring-and-sector descriptor of its rows 0-2 (`ops.scan_descriptor`, HIP, csrc/scan_descriptor.hip: Scan Context, Kim &
Kim, IROS 2018); one `ops.scan_match` compares every frame with every frame at least --gap positions before it, at every ring shift, so a
place is recognised whatever the heading; per frame the --top earlier frames of least distance at or below --max-desc-dist are its
candidates (equal distances go to the lower frame), selected on the device.  Each candidate pair (i the later frame, j the earlier) is
then registered, source i onto target j, by `ops.icp_point_to_plane` as `align` registers consecutive frames.  --init says where the
start pose comes from: `shift` turns frame i about z by the heading the best ring shift stands for (`ops.scan_shift_yaw`), with no
translation; `global` is `align --init global`'s FPFH and RANSAC start; `auto` (the default) tries the first and, when its result is
not accepted, the second.  A pair is accepted when ICP ends with status 0 or 1, with at least --min-overlap x the source's rows paired
and an rmse of at most --max-rmse.  One line per candidate:

    loop <i> <j>: dist <d> shift <k> yaw <degrees> pairs <n> rmse <m> iterations <it> status <s> start <shift|global> -> accepted|rejected

With --poses FILE (line n maps frame A + n into frame A, as `align --out` writes them) an accepted line ends `drift <metres> <degrees>`:
how far the file's inv(P_j) P_i lies from the measured pose.  The closing line is

    loops: <a> accepted of <c> candidates of <F> frames

--out FILE writes one line per accepted edge (`align.write_edges`): i j, the 12 numbers of the pose that maps frame i into frame j, then
dist rmse pairs.  No default of this command is tuned on real data.  The pose-graph solve over the chain and these edges is
`python -m cmr_agent_amd.dataset.posegraph`, which reads this file.

    python -m cmr_agent_amd.dataset.loops --root DIR --sequence S [--frames A:B --rings 20 --sectors 60 --max-range 80 --min-range 0
                                          --height 2.0 --gap 50 --top 1 --max-desc-dist 0.3 --min-cols S/4]
                                          [--init shift|global|auto --max-dist 1.0 --huber 0.1 --iters 30 --max-rmse 0.2 --min-overlap 0.3]
                                          [--fpfh-radius 1.0 --ransac-hyp 4096 --ransac-thr 0.3 --seed 0 --poses FILE --out FILE]
"""
import argparse
import math

import numpy as np
import torch

from .. import ops
from . import align, prepare


# ---- the rules: plain functions ---------------------------------------------------------------------------------------------------------------
def gap_limits(frames, gap):
    """limit of ops.scan_match for a list of `frames` frames: the frame at position i meets the positions [0, max(0, i - gap + 1))"""
    return np.maximum(0, np.arange(frames, dtype=np.int64) - gap + 1).astype(np.int32)


def select_candidates(dist, top, max_desc_dist):
    """dist [Q, N] (torch, any device; NaN = not compared) -> (query, candidate, distance) as three tensors on that device: per query the
    `top` candidates of least distance at or below max_desc_dist, nearest first, equal distances to the lower candidate; by query."""
    d = torch.where(torch.isnan(dist), torch.full_like(dist, math.inf), dist)
    val, idx = torch.sort(d, dim=1, stable=True)
    val, idx = val[:, :top], idx[:, :top]
    q, r = torch.nonzero(val <= max_desc_dist, as_tuple=True)          # row-major: by query, then by rank
    return q, idx[q, r], val[q, r]


def accepted(res, rows, max_rmse, min_overlap):
    """the acceptance rule on an ops.IcpResult of a source of `rows` rows"""
    return res.status in (0, 1) and res.pairs >= min_overlap * rows and res.rmse <= max_rmse


def shift_start(shift, sectors):
    """The start pose of source i (the query) onto target j (the candidate) that a ring shift stands for: Rz(-scan_shift_yaw), float64"""
    a = -ops.scan_shift_yaw(int(shift), sectors)
    T = np.eye(4)
    T[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    return T


def drift(poses, pi, pj, measured):
    """-> (metres, degrees) between inv(P_j) P_i of the poses and the measured pose of frame i in frame j"""
    D = np.linalg.inv(measured) @ np.linalg.inv(poses[pj]) @ poses[pi]
    sine = np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2.0       # acos of the trace loses half the digits near 0
    return float(np.linalg.norm(D[:3, 3])), math.degrees(math.atan2(sine, (np.trace(D[:3, :3]) - 1.0) / 2.0))


# ---- the search -------------------------------------------------------------------------------------------------------------------------------
def describe_sequence(files, rings=20, sectors=60, max_range=80.0, min_range=0.0, height=2.0, device=None):
    """-> the frames' descriptors float32 [F, rings, sectors] on the device, one call each"""
    return torch.stack([ops.scan_descriptor(align.device_rows(align.read_prepared(path)[0:3], device), rings, sectors, max_range, min_range,
                                            height).desc for _, path in files])


def find_candidates(descs, gap=50, top=1, max_desc_dist=0.3, min_cols=None):
    """-> [(position i, position j, distance, shift)] with j <= i - gap, by i and then by distance: one match of all against all earlier"""
    F = descs.shape[0]
    limit = torch.from_numpy(gap_limits(F, gap)).to(descs.device)
    m = ops.scan_match(descs, descs, limit, min_cols)
    q, c, d = select_candidates(m.dist, top, max_desc_dist)
    return list(zip(q.tolist(), c.tolist(), d.tolist(), m.shift[q, c].tolist()))


def close_loops(files, candidates, sectors, init="auto", max_dist=1.0, huber=0.1, iters=30, max_rmse=0.2, min_overlap=0.3, fpfh_radius=1.0,
                ransac_hyp=4096, ransac_thr=0.3, seed=0, poses=None, device=None, report=print):
    """Registers every candidate (positions in `files`), reports one line each -> the accepted edges as align.write_edges takes them."""
    edges = []
    for pi, pj, d, k in candidates:
        (i, path_i), (j, path_j) = files[pi], files[pj]
        source, target = align.read_prepared(path_i), align.read_prepared(path_j)
        for start in {"shift": ("shift",), "global": ("global",), "auto": ("shift", "global")}[init]:
            if start == "shift":
                pose = align.device_pose(shift_start(k, sectors), device)
            else:
                pose = align.global_start(target, source, fpfh_radius, ransac_hyp, ransac_thr, seed, device).pose
            res = align.register_pair(target, source, pose, max_dist, huber, iters, device)
            ok = accepted(res, source.shape[1], max_rmse, min_overlap)
            if ok:
                break
        T = res.pose.cpu().numpy().astype(np.float64)
        line = "loop %d %d: dist %.4f shift %d yaw %.2f pairs %d rmse %.4f iterations %d status %d start %s -> %s" % (
            i, j, d, k, math.degrees(ops.scan_shift_yaw(k, sectors)), res.pairs, res.rmse, res.iterations, res.status, start,
            "accepted" if ok else "rejected")
        if ok and poses is not None:
            line += " drift %.4f %.4f" % drift(poses, pi, pj, T)
        report(line)
        if ok:
            edges.append((i, j, T, d, res.rmse, res.pairs))
    return edges


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cmr_agent_amd.dataset.loops", description=__doc__.split("\n\n")[0],
                                 epilog="No default of this command is tuned on real data.")
    align.sequence_flags(ap)
    ap.add_argument("--rings", type=int, default=20, help="rings of the descriptor (default 20)")
    ap.add_argument("--sectors", type=int, default=60, help="sectors of the descriptor, a multiple of 4 (default 60)")
    ap.add_argument("--max-range", type=float, default=80.0, help="the descriptor's outer radius in metres (default 80)")
    ap.add_argument("--min-range", type=float, default=0.0, help="the descriptor's inner radius in metres (default 0)")
    ap.add_argument("--height", type=float, default=2.0, help="the sensor's height above the ground in metres, added to z (default 2.0)")
    ap.add_argument("--gap", type=int, default=50, help="a frame is compared with frames at least this many positions before it (default 50)")
    ap.add_argument("--top", type=int, default=1, help="candidates per frame at most (default 1)")
    ap.add_argument("--max-desc-dist", type=float, default=0.3, help="largest descriptor distance of a candidate (default 0.3, not tuned on real data)")
    ap.add_argument("--min-cols", type=int, default=None, help="a ring shift counts when this many column pairs are non-empty (default sectors / 4)")
    ap.add_argument("--init", default="auto", choices=("shift", "global", "auto"),
                    help="a candidate's start pose: the heading of its ring shift, a global registration from FPFH descriptors and RANSAC, or "
                         "the first and, when the result is not accepted, the second (default)")
    ap.add_argument("--max-dist", type=float, default=1.0, help="largest distance of a pair in metres, and the grid's cell (default 1.0)")
    ap.add_argument("--huber", type=float, default=0.1, help="residuals above this many metres are down-weighted; 0 = off (default 0.1)")
    ap.add_argument("--iters", type=int, default=30, help="most iterations per pair (default 30)")
    ap.add_argument("--max-rmse", type=float, default=0.2, help="an accepted pair's rmse in metres at most (default 0.2, not tuned on real data)")
    ap.add_argument("--min-overlap", type=float, default=0.3, help="an accepted pair pairs at least this share of the source's rows (default 0.3, "
                    "not tuned on real data)")
    ap.add_argument("--fpfh-radius", type=float, default=1.0, help="radius of the FPFH descriptors in metres (default 1.0)")
    ap.add_argument("--ransac-hyp", type=int, default=4096, help="RANSAC hypotheses of a global registration (default 4096)")
    ap.add_argument("--ransac-thr", type=float, default=0.3, help="RANSAC inlier distance in metres (default 0.3)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the RANSAC draws (default 0)")
    ap.add_argument("--poses", default=None, help="the poses of the frames, 12 numbers per line: accepted lines then end with the drift")
    ap.add_argument("--out", default=None, help="write the accepted edges here: i j, 12 numbers of the pose of i in j, dist rmse pairs")
    args = ap.parse_args(argv)
    align.check_sequence_flags(ap, args)
    prepare.check_positive(ap, args, "max_range", "max_dist", "max_rmse", "fpfh_radius", "ransac_thr")
    try:
        ops._scan_shape("loops", args.rings, args.sectors)
    except ValueError as e:
        ap.error(str(e))
    if not 0.0 <= args.min_range < args.max_range:
        ap.error("--min-range must lie in [0, --max-range)")
    if not math.isfinite(args.height):
        ap.error("--height must be finite")
    if not 1 <= args.gap < 1 << 31:
        ap.error("--gap must lie in [1, 2^31)")
    if not 1 <= args.top < 1 << 31:
        ap.error("--top must lie in [1, 2^31)")
    if not 0.0 <= args.max_desc_dist < float("inf"):
        ap.error("--max-desc-dist must be finite and >= 0, got %r" % (args.max_desc_dist,))
    if args.min_cols is not None and not 1 <= args.min_cols <= args.sectors:
        ap.error("--min-cols must lie in [1, --sectors]")
    if not (0.0 <= args.huber < float("inf")):
        ap.error("--huber must be finite and >= 0, got %r" % (args.huber,))
    if not 0 <= args.iters <= ops.ICP_MAX_ITERS:
        ap.error("--iters must lie in [0, %d]" % ops.ICP_MAX_ITERS)
    if not 0.0 <= args.min_overlap <= 1.0:
        ap.error("--min-overlap must lie in [0, 1]")
    if not 1 <= args.ransac_hyp <= ops.RANSAC_MAX_HYP:
        ap.error("--ransac-hyp must lie in [1, %d]" % ops.RANSAC_MAX_HYP)
    if not 0 <= args.seed < 1 << 32:
        ap.error("--seed must lie in [0, 2^32)")
    return ap, args


def main(argv=None, device=None):
    ap, args = parse_args(argv)
    files = align.sequence_files(ap, args)
    poses = None
    if args.poses is not None:
        try:
            poses = align.read_poses(args.poses)
        except ValueError as e:
            ap.error(str(e))
        if poses.shape[0] != len(files):
            ap.error("%s holds %d poses, --frames names %d frames" % (args.poses, poses.shape[0], len(files)))
    edges, candidates = [], []
    try:
        if files:
            descs = describe_sequence(files, args.rings, args.sectors, args.max_range, args.min_range, args.height, device)
            candidates = find_candidates(descs, args.gap, args.top, args.max_desc_dist, args.min_cols)
            edges = close_loops(files, candidates, args.sectors, args.init, args.max_dist, args.huber, args.iters, args.max_rmse, args.min_overlap,
                                args.fpfh_radius, args.ransac_hyp, args.ransac_thr, args.seed, poses, device)
    except ValueError as e:
        ap.error(str(e))
    print("loops: %d accepted of %d candidates of %d frames" % (len(edges), len(candidates), len(files)))
    if args.out is not None:
        align.write_edges(args.out, edges)


if __name__ == "__main__":
    main()
