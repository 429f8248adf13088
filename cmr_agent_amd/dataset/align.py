"""Prepared clouds of a sequence -> the motion between consecutive scans, by point-to-plane ICP.

    <root>/<data_velodyne>/sequences/<seq>/voxel0.1-SNr0.6/<i>.npy        float32 [7, n]: x, y, z, reflectance, nx, ny, nz   (read)

Frame i + 1 (the source) is registered onto frame i (the target, with the normals `prepare` wrote into rows 4-6) by
`ops.icp_point_to_plane` (HIP, csrc/cloud_icp.hip); the start pose of a pair is the previous pair's result -- a vehicle moves much like it
did a scan ago -- and the identity for the first pair.  One line per pair:

    pair <i> <i+1>: pairs <n> rmse <m> iterations <k> status <s> t <x y z> r <degrees>

pairs and rmse are those of the last iteration (at the pose it started from), status is the op's (0 converged, 1 iterations exhausted,
2 fewer than 6 pairs, 3 singular system), t and r are the translation in metres and the rotation angle of the pair's pose.  --out FILE
writes the chained poses (`write_poses`): line j maps frame A + j into frame A, the first line is the identity, all in the velodyne frame.

--init says where a pair's start pose comes from.  `previous` (the default) is the rule above.  `global` starts every pair
from `ops.register_global(refine=False)`: FPFH descriptors of both clouds (the source's normals are rows 4-6 of its own file), mutual
nearest descriptors, RANSAC -- no start pose needed, so a gap, a dropped frame or a revisit does not matter.  `auto` tries `previous` and
repeats the pair from `global` when ICP ends with status 2 or 3; one more line is then printed ahead of the pair's, with RANSAC's inliers,
the correspondences it was given and its status (`register_from`).

--map K (0, the default, is all of the above unchanged) registers frame j against the voxel map of the last K registered
frames, kept in frame A's coordinates by `ops.voxel_map_insert` (HIP, csrc/voxel_map.hip), instead of against frame i alone: the map's
normals are `ops.point_normals` of its points seen from frame i's position, the start pose is frame i's pose times the previous relative
motion, and ICP's result is frame j's pose in frame A directly.  t and r of the pair's line stay those of the relative pose; a `global` or
`auto` fallback registers against frame i as above and is moved into frame A.  The map's grid starts at -extent / 2 on each axis; when c
of frame j's n rows fall off it, one more line follows the pair's:

    pair <i> <i+1>: outside <c> of <n>

    python -m cmr_agent_amd.dataset.align --root DIR --sequence S [--frames A:B --max-dist 1.0 --huber 0.1 --iters 30 --out FILE]
                                          [--init previous|global|auto --fpfh-radius 1.0 --ransac-hyp 4096 --ransac-thr 0.3 --seed 0]
                                          [--map K --map-voxel 0.1 --map-extent 8192 --map-normal-radius 0.6]
"""
import argparse
import math
import os

import numpy as np
import torch

from .. import ops
from . import prepare


def read_prepared(path):
    """<i>.npy of a prepared folder -> float32 [7, n]; ValueError for anything else (a [4, n] file has no normals)."""
    cloud = np.load(path)
    if cloud.dtype != np.float32 or cloud.ndim != 2 or cloud.shape[0] != 7:
        raise ValueError("%s: need float32 [7, n] (x, y, z, reflectance, nx, ny, nz), got %s %s" % (path, cloud.dtype, cloud.shape))
    return cloud


def read_poses(path):
    """A poses file (write_poses; KITTI's layout) -> float64 [F, 4, 4]; ValueError for anything else."""
    try:
        rows = np.loadtxt(path, dtype=np.float64, ndmin=2)
    except (OSError, ValueError) as e:
        raise ValueError("%s: %s" % (path, e))
    if rows.shape[1:] != (12,) or not np.isfinite(rows).all():
        raise ValueError("%s: need 12 finite numbers per line (the upper 3 x 4 of a pose, row-major)" % path)
    poses = np.tile(np.eye(4), (rows.shape[0], 1, 1))
    poses[:, :3, :] = rows.reshape(-1, 3, 4)
    return poses


def write_poses(path, poses):
    """float64 [F, 4, 4] -> the file read_poses reads: the upper 3 x 4 of each, row-major, 12 numbers per line; %.9e carries a float32 exactly."""
    np.savetxt(path, np.asarray(poses)[:, :3].reshape(-1, 12), fmt="%.9e")


def write_edges(path, edges):
    """Loop edges (dataset/loops.py) as (i, j, pose [4, 4], dist, rmse, pairs) -> one line each: i j, the upper 3 x 4 of the pose that maps
    frame i into frame j (row-major, %.9e as write_poses), then dist rmse pairs."""
    with open(path, "w") as fh:
        for i, j, pose, dist, rmse, pairs in edges:
            fh.write("%d %d %s %.9e %.9e %d\n" % (i, j, " ".join("%.9e" % v for v in np.asarray(pose, np.float64)[:3].reshape(-1)), dist, rmse, pairs))


def read_edges(path):
    """The file write_edges writes -> a list of (i, j, pose float64 [4, 4], dist, rmse, pairs); ValueError for anything else."""
    edges = []
    with open(path) as fh:
        for n, line in enumerate(fh):
            words = line.split()
            try:
                if len(words) != 17:
                    raise ValueError
                i, j, pairs = int(words[0]), int(words[1]), int(words[16])
                nums = np.array([float(w) for w in words[2:16]])
                if not np.isfinite(nums).all() or min(i, j, pairs) < 0:
                    raise ValueError
            except ValueError:
                raise ValueError("%s line %d: need `i j`, 12 numbers of a pose, `dist rmse pairs`" % (path, n + 1))
            pose = np.eye(4)
            pose[:3] = nums[:12].reshape(3, 4)
            edges.append((i, j, pose, float(nums[12]), float(nums[13]), pairs))
    return edges


def on_device(device):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else device


def device_rows(a, device=None):
    """rows of a prepared cloud, numpy float32 [c, n] -> the device tensor [n, c] the ops read"""
    return torch.from_numpy(np.ascontiguousarray(a.T)).to(on_device(device))


def device_pose(T, device=None):
    return torch.from_numpy(T.astype(np.float32)).to(on_device(device))                # float64 [4, 4] -> the float32 the ops read


def register_pair(target7, source7, pose=None, max_dist=1.0, huber=0.1, iters=30, device=None):
    """Two prepared clouds float32 [7, n] (numpy) -> ops.IcpResult of the source onto the target."""
    return ops.icp_point_to_plane(device_rows(source7[0:3], device), device_rows(target7[0:3], device), device_rows(target7[4:7], device),
                                  pose=pose, max_dist=max_dist, huber=huber, iters=iters)


def global_start(target7, source7, radius=1.0, n_hyp=4096, thr=0.3, seed=0, device=None):
    """Two prepared clouds float32 [7, n] (numpy) -> ops.GlobalResult of the source onto the target without a start pose, not polished."""
    return ops.register_global(device_rows(source7[0:3], device), device_rows(source7[4:7], device), device_rows(target7[0:3], device),
                               device_rows(target7[4:7], device), radius=radius, n_hyp=n_hyp, thr=thr, seed=seed, refine=False)


def rotation_degrees(pose):
    c = (float(pose[0, 0]) + float(pose[1, 1]) + float(pose[2, 2]) - 1.0) / 2.0
    return math.degrees(math.acos(min(1.0, max(-1.0, c))))


def register_from(init, i, j, report, icp, previous, from_global):
    """--init for pair (i, j): icp(start) -> ops.IcpResult, `previous` = the start `previous` means, from_global() -> ops.GlobalResult with the
    start as its pose.  `auto` repeats a pair that ends with status 2 or 3 from the global start, after one more line.  -> ops.IcpResult."""
    if init != "global":
        res = icp(previous)
    if init == "global" or (init == "auto" and res.status in (2, 3)):
        g = from_global()
        if init == "auto":
            report("pair %d %d: global inliers %d of %d status %d" % (i, j, g.inliers, g.correspondences, g.status))
        res = icp(g.pose)
    return res


def report_pair(report, i, j, res, rel):
    report("pair %d %d: pairs %d rmse %.4f iterations %d status %d t %.4f %.4f %.4f r %.4f" % (
        i, j, res.pairs, res.rmse, res.iterations, res.status, rel[0, 3], rel[1, 3], rel[2, 3], rotation_degrees(rel)))


def align_sequence(files, max_dist=1.0, huber=0.1, iters=30, device=None, report=print, init="previous", fpfh_radius=1.0, ransac_hyp=4096,
                   ransac_thr=0.3, seed=0):
    """files: the prepared clouds of consecutive frames as (frame number, path).  -> float64 [len(files), 4, 4]: frame j in frame 0's
    coordinates.  `report` receives one line per pair (two for a pair that `auto` repeats from a global start)."""
    chain = [np.eye(4)]
    pose = None
    target = read_prepared(files[0][1]) if files else None
    for (i, _), (j, path) in zip(files[:-1], files[1:]):
        source = read_prepared(path)
        res = register_from(init, i, j, report, lambda start: register_pair(target, source, start, max_dist, huber, iters, device), pose,
                            lambda: global_start(target, source, fpfh_radius, ransac_hyp, ransac_thr, seed, device))
        pose = res.pose
        T = pose.cpu().numpy().astype(np.float64)
        report_pair(report, i, j, res, T)
        chain.append(chain[-1] @ T)
        target = source
    return np.stack(chain[:len(files)]) if files else np.zeros((0, 4, 4))


def align_to_map(files, k, max_dist=1.0, huber=0.1, iters=30, device=None, report=print, init="previous", fpfh_radius=1.0, ransac_hyp=4096,
                 ransac_thr=0.3, seed=0, map_voxel=0.1, map_extent=8192.0, map_normal_radius=0.6):
    """align_sequence against a map: the target of pair (i, j) is the voxel map of the last k registered frames in the first
    frame's coordinates (ops.voxel_map_insert with stamp = the frame number and min_stamp = j - k), its normals ops.point_normals of the
    map's points seen from frame i's position, and ICP's result is frame j's pose in the first frame directly.  Same lines as
    align_sequence, t and r those of the pose relative to frame i; `pair <i> <j>: outside <c> of <n>` follows when c of frame j's n rows
    fell off the map's grid."""
    chain, rel = [np.eye(4)], np.eye(4)
    vmap = ops.voxel_map(map_voxel, (-map_extent / 2,) * 3, device=device)
    target = None
    for n, (j, path) in enumerate(files):
        source = read_prepared(path)
        xyz = device_rows(source[0:3], device)
        if n:
            normals = ops.point_normals(vmap.points, radius=map_normal_radius, viewpoint=tuple(chain[-1][:3, 3])).normals
            icp = lambda start: ops.icp_point_to_plane(xyz, vmap.points, normals, pose=device_pose(start, device), max_dist=max_dist,  # noqa: E731
                                                       huber=huber, iters=iters)

            def from_global():                               # frame j against frame i from the files, moved into the first frame
                g = global_start(target, source, fpfh_radius, ransac_hyp, ransac_thr, seed, device)
                return g._replace(pose=chain[-1] @ g.pose.cpu().numpy().astype(np.float64))

            res = register_from(init, j - 1, j, report, icp, chain[-1] @ rel, from_global)
            T = res.pose.cpu().numpy().astype(np.float64)
            rel = np.linalg.inv(chain[-1]) @ T
            report_pair(report, j - 1, j, res, rel)
            chain.append(T)
        ins = ops.voxel_map_insert(vmap, xyz, pose=device_pose(chain[-1], device), stamp=j, min_stamp=max(0, j + 1 - k))
        if n and ins.outside:
            report("pair %d %d: outside %d of %d" % (j - 1, j, ins.outside, xyz.shape[0]))
        vmap, target = ins.map, source
    return np.stack(chain) if files else np.zeros((0, 4, 4))


def sequence_files(ap, args):
    """The prepared files of the frames --frames names as (frame number, path), consecutive; anything else is an argparse error."""
    folder = os.path.join(args.root, args.data_velodyne, "sequences", "%02d" % args.sequence, args.subdir)
    if not os.path.isdir(folder):
        ap.error("%s is not a directory; python -m cmr_agent_amd.dataset.prepare writes it" % folder)
    a, b = args.frames
    files = []
    for name in sorted(os.listdir(folder)):
        stem, ext = os.path.splitext(name)
        if ext == ".npy" and stem.isdigit() and a <= int(stem) and (b is None or int(stem) < b):
            files.append((int(stem), os.path.join(folder, name)))
    files.sort()
    for (i, _), (j, _) in zip(files[:-1], files[1:]):
        if j != i + 1:
            ap.error("frame %d is missing between %d and %d in %s" % (i + 1, i, j, folder))
    for _, path in files:                                # the headers only: a wrong layout ends the run before any work
        shape = np.load(path, mmap_mode="r").shape
        if len(shape) == 2 and shape[0] == 4:
            ap.error("%s holds [4, n] rows and no normals; write [7, n] files with python -m cmr_agent_amd.dataset.prepare "
                     "(without --no-normals)" % path)
    return files


def sequence_flags(ap):
    """the flags that name the prepared files of a sequence"""
    ap.add_argument("--root", required=True, help="dataset root: <root>/<data_velodyne>/sequences/<seq>/<subdir>/*.npy is read")
    ap.add_argument("--sequence", required=True, type=int, help="the sequence number")
    ap.add_argument("--frames", default=":", help="A:B, the frames A <= i < B of the sequence (default: all of them)")
    ap.add_argument("--data-velodyne", default=None, help="the velodyne folder under --root (default: the KITTI configuration's data_velodyne)")
    ap.add_argument("--subdir", default=prepare.subdir(), help="the prepared folder of the sequence (default %s)" % prepare.subdir())


def check_sequence_flags(ap, args):
    if not 0 <= args.sequence <= 99:
        ap.error("--sequence must lie in [0, 99]")
    try:
        a, b = args.frames.split(":")
        args.frames = (int(a) if a else 0, int(b) if b else None)
        if args.frames[0] < 0 or (args.frames[1] is not None and args.frames[1] < args.frames[0]):
            raise ValueError
    except ValueError:
        ap.error("--frames must be A:B with integers 0 <= A <= B (either may be left out)")
    if args.data_velodyne is None:
        from ..config.KittiConfig import KittiConfiguration
        args.data_velodyne = KittiConfiguration(None).data_velodyne


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cmr_agent_amd.dataset.align", description=__doc__.split("\n\n")[0])
    sequence_flags(ap)
    ap.add_argument("--max-dist", type=float, default=1.0, help="largest distance of a pair in metres, and the grid's cell (default 1.0)")
    ap.add_argument("--huber", type=float, default=0.1, help="residuals above this many metres are down-weighted; 0 = off (default 0.1)")
    ap.add_argument("--iters", type=int, default=30, help="most iterations per pair (default 30)")
    ap.add_argument("--out", default=None, help="write the chained poses here, 12 numbers per line")
    ap.add_argument("--init", default="previous", choices=("previous", "global", "auto"),
                    help="a pair's start pose: the previous pair's result (default), a global registration from FPFH descriptors and RANSAC, "
                         "or the first and, when ICP ends with status 2 or 3, the second")
    ap.add_argument("--fpfh-radius", type=float, default=1.0, help="radius of the FPFH descriptors in metres (default 1.0)")
    ap.add_argument("--ransac-hyp", type=int, default=4096, help="RANSAC hypotheses of a global registration (default 4096)")
    ap.add_argument("--ransac-thr", type=float, default=0.3, help="RANSAC inlier distance in metres (default 0.3)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the RANSAC draws (default 0)")
    ap.add_argument("--map", type=int, default=0, metavar="K",
                    help="register every frame against the voxel map of the last K registered frames instead of the frame before it (default 0: off)")
    ap.add_argument("--map-voxel", type=float, default=0.1, help="the map's voxel in metres (default 0.1)")
    ap.add_argument("--map-extent", type=float, default=8192.0, help="the map's grid starts at -extent / 2 on each axis, in metres (default 8192)")
    ap.add_argument("--map-normal-radius", type=float, default=0.6, help="radius of the map's normals in metres (default 0.6)")
    args = ap.parse_args(argv)
    check_sequence_flags(ap, args)
    prepare.check_positive(ap, args, "max_dist", "fpfh_radius", "ransac_thr", "map_voxel", "map_extent", "map_normal_radius")
    if not (0.0 <= args.huber < float("inf")):
        ap.error("--huber must be finite and >= 0, got %r" % (args.huber,))
    if not 0 <= args.iters <= ops.ICP_MAX_ITERS:
        ap.error("--iters must lie in [0, %d]" % ops.ICP_MAX_ITERS)
    if not 1 <= args.ransac_hyp <= ops.RANSAC_MAX_HYP:
        ap.error("--ransac-hyp must lie in [1, %d]" % ops.RANSAC_MAX_HYP)
    if not 0 <= args.seed < 1 << 32:
        ap.error("--seed must lie in [0, 2^32)")
    if not 0 <= args.map < 1 << 31:
        ap.error("--map must lie in [0, 2^31)")
    return ap, args


def main(argv=None, device=None):
    ap, args = parse_args(argv)
    files = sequence_files(ap, args)
    kw = dict(init=args.init, fpfh_radius=args.fpfh_radius, ransac_hyp=args.ransac_hyp, ransac_thr=args.ransac_thr, seed=args.seed)
    try:
        if args.map:
            chain = align_to_map(files, args.map, args.max_dist, args.huber, args.iters, device, map_voxel=args.map_voxel,
                                 map_extent=args.map_extent, map_normal_radius=args.map_normal_radius, **kw)
        else:
            chain = align_sequence(files, args.max_dist, args.huber, args.iters, device, **kw)
    except ValueError as e:
        ap.error(str(e))
    if args.out is not None:
        write_poses(args.out, chain)


if __name__ == "__main__":
    main()
