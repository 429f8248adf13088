"""Prepared clouds of a sequence and their poses -> one map of the sequence in the prepared layout.

    <root>/<data_velodyne>/sequences/<seq>/voxel0.1-SNr0.6/<i>.npy        float32 [7, n]: x, y, z, reflectance, nx, ny, nz   (read)
    --poses FILE                                                          12 numbers per line, as `align --out` writes them  (read)
    --out FILE                                                            float32 [7, n], the same layout                    (written)

Line j of the poses file maps frame A + j into frame A.  Every frame is inserted under its pose into one voxel map
(`ops.voxel_map_insert`, HIP, csrc/voxel_map.hip) with the reflectance as the one attribute; a voxel's row is the mean of all rows that
fell into it, whichever frame they came from.  The map's grid starts at -extent / 2 on each axis (metres, in frame A); rows off it are
counted and left out.  Voxels with fewer than --min-count rows are dropped, normals are `ops.point_normals` of what is left, seen from
frame A's origin, and the result is written as one more prepared cloud: whatever reads those reads the map.  One line per frame and one
at the end:

    frame <i>: rows <n> new <a> merged <b> outside <c>
    map: <n> voxels from <rows> rows of <frames> frames

--carve removes what the frames saw THROUGH: a map that only grows keeps the trail of every moving object, every stray
return and the ghosts of frames whose pose was off.  After all frames are inserted, and before --min-count and the normals, every row of
every frame is cast as a ray from the sensor to the row through the final map (`ops.voxel_map_rays`, HIP, csrc/voxel_map_rays.hip), within
ceil(carve-start / voxel) cells of the sensor and --carve-end cells of the row nothing is counted, and rays of more than
min(65 536, ceil(3 carve-max-range / voxel)) cells are not cast.  A frame sees THROUGH a voxel that at least --carve-rays of its rays
cross and none ends in, and SEES a voxel one of its rays ends in; a voxel is dropped when at least --carve-frames frames see through it and
at least --carve-ratio times as many as see it (`carve_rule`).  The defaults are not tuned on real data.  One more line per frame, and one
ahead of the map's:

    carve <i>: cast <n> long <l> outside <c> through <k>
    carved: <d> of <n> voxels

    python -m cmr_agent_amd.dataset.accumulate --root DIR --sequence S --poses FILE [--frames A:B --voxel 0.1 --extent 8192]
                                               [--normal-radius 0.6 --min-count 1 --out FILE]
                                               [--carve [--carve-rays 1 --carve-frames 2 --carve-ratio 1.0 --carve-start 2.0 --carve-end 1
                                                         --carve-max-range 120.0]]
"""
import argparse
import math

import numpy as np
import torch

from .. import ops
from . import align, prepare
from .align import device_pose, device_rows, read_poses            # read_poses stays a name of this module: its callers read it here


def accumulate_sequence(files, poses, voxel=0.1, extent=8192.0, device=None, report=print):
    """files: the prepared clouds as (frame number, path); poses float64 [len(files), 4, 4].  -> (ops.VoxelMap with one attribute, the
    rows read).  `report` receives one line per frame."""
    vmap = ops.voxel_map(voxel, (-extent / 2,) * 3, channels=1, device=device)
    total = 0
    for (i, path), T in zip(files, poses):
        cloud = align.read_prepared(path)
        ins = ops.voxel_map_insert(vmap, device_rows(cloud[0:3], device), device_rows(cloud[3:4], device), pose=device_pose(T, device), stamp=i)
        report("frame %d: rows %d new %d merged %d outside %d" % (i, cloud.shape[1], ins.new, ins.merged, ins.outside))
        total += cloud.shape[1]
        vmap = ins.map
    return vmap, total


def carve_rule(through, seen, frames=2, ratio=1.0):
    """through, seen: per voxel, the frames that saw through it and the frames that saw it (integer tensors or arrays of one shape)
    -> the bool mask of the voxels to drop: through >= frames and through >= ratio * seen."""
    return (through >= frames) & (through >= ratio * seen)


def carve_margins(voxel, start=2.0, max_range=120.0):
    """-> (start_margin, max_cells) of ops.voxel_map_rays for lengths in metres: ceil(start / voxel), min(65 536, ceil(3 max_range / voxel))"""
    return int(math.ceil(start / voxel)), int(min(ops.MAP_RAYS_MAX_CELLS, math.ceil(3.0 * max_range / voxel)))


def carve_sequence(vmap, files, poses, rays=1, frames=2, ratio=1.0, start=2.0, end=1, max_range=120.0, device=None, report=print):
    """Every frame cast through the map under its pose -> the bool [n] mask of the voxels `carve_rule` drops.  `report` receives one
    line per frame."""
    start_margin, max_cells = carve_margins(vmap.voxel, start, max_range)
    through = torch.zeros((vmap.keys.shape[0],), dtype=torch.int64, device=vmap.keys.device)
    seen = torch.zeros_like(through)
    for (i, path), T in zip(files, poses):
        cloud = align.read_prepared(path)
        res = ops.voxel_map_rays(vmap, device_rows(cloud[0:3], device), pose=device_pose(T, device), start_margin=start_margin, end_margin=end,
                                 max_cells=max_cells)
        sees_through = (res.crossed >= rays) & (res.hits == 0)
        through += sees_through
        seen += res.hits > 0
        report("carve %d: cast %d long %d outside %d through %d" % (i, res.cast, res.long, res.outside, int(sees_through.sum())))
    return carve_rule(through, seen.double(), frames, ratio)


def map_cloud(vmap, min_count=1, normal_radius=0.6):
    """The voxels with at least min_count rows as a prepared cloud, float32 [7, n] (numpy)"""
    keep = vmap.count >= min_count
    points, refl = vmap.points[keep].contiguous(), vmap.attr[keep]
    normals = ops.point_normals(points, radius=normal_radius).normals
    return torch.cat([points, refl, normals], 1).T.contiguous().cpu().numpy()


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cmr_agent_amd.dataset.accumulate", description=__doc__.split("\n\n")[0])
    align.sequence_flags(ap)
    ap.add_argument("--poses", required=True, help="the poses of the frames, 12 numbers per line: line j maps frame A + j into frame A")
    ap.add_argument("--voxel", type=float, default=0.1, help="the map's voxel in metres (default 0.1)")
    ap.add_argument("--extent", type=float, default=8192.0, help="the map's grid starts at -extent / 2 on each axis, in metres (default 8192)")
    ap.add_argument("--normal-radius", type=float, default=0.6, help="radius of the map's normals in metres (default 0.6)")
    ap.add_argument("--min-count", type=int, default=1, help="drop voxels with fewer rows than this (default 1)")
    ap.add_argument("--out", default=None, help="write the map here, float32 [7, n]")
    ap.add_argument("--carve", action="store_true", help="drop the voxels the frames saw through: every frame's rows are cast as rays from "
                    "its sensor through the final map, before --min-count and the normals.  The defaults of the --carve-* flags are not "
                    "tuned on real data")
    ap.add_argument("--carve-rays", type=int, default=1, help="a frame sees through a voxel that at least this many of its rays cross and none "
                    "ends in (default 1)")
    ap.add_argument("--carve-frames", type=int, default=2, help="drop a voxel at least this many frames see through (default 2) ...")
    ap.add_argument("--carve-ratio", type=float, default=1.0, help="... and at least this many times as many as see it (default 1.0)")
    ap.add_argument("--carve-start", type=float, default=2.0, help="count nothing within this many metres of the sensor, rounded up to whole "
                    "voxels: the vehicle itself (default 2.0)")
    ap.add_argument("--carve-end", type=int, default=1, help="count nothing within this many voxels of a ray's end: surfaces seen at a grazing "
                    "angle (default 1)")
    ap.add_argument("--carve-max-range", type=float, default=120.0, help="rays of more than min(65536, ceil(3 x this / voxel)) cells are not "
                    "cast, in metres (default 120.0)")
    args = ap.parse_args(argv)
    align.check_sequence_flags(ap, args)
    prepare.check_positive(ap, args, "voxel", "extent", "normal_radius", "carve_max_range")
    if not 1 <= args.min_count < 1 << 31:
        ap.error("--min-count must lie in [1, 2^31)")
    for name in ("carve_rays", "carve_frames"):
        if not 1 <= getattr(args, name) < 1 << 31:
            ap.error("--%s must lie in [1, 2^31)" % name.replace("_", "-"))
    if not 0.0 <= args.carve_ratio < float("inf"):
        ap.error("--carve-ratio must be finite and >= 0, got %r" % args.carve_ratio)
    if not (0.0 <= args.carve_start < float("inf")) or math.ceil(args.carve_start / args.voxel) >= ops.CLOUD_CELL_LIMIT:
        ap.error("--carve-start must be >= 0 and below 2^21 voxels, got %r" % args.carve_start)
    if not 0 <= args.carve_end < ops.CLOUD_CELL_LIMIT:
        ap.error("--carve-end must lie in [0, 2^21)")
    return ap, args


def main(argv=None, device=None):
    ap, args = parse_args(argv)
    files = align.sequence_files(ap, args)
    try:
        poses = read_poses(args.poses)
    except ValueError as e:
        ap.error(str(e))
    if poses.shape[0] != len(files):
        ap.error("%s holds %d poses, --frames names %d frames" % (args.poses, poses.shape[0], len(files)))
    try:
        vmap, total = accumulate_sequence(files, poses, args.voxel, args.extent, device)
        if args.carve:
            drop = carve_sequence(vmap, files, poses, args.carve_rays, args.carve_frames, args.carve_ratio, args.carve_start, args.carve_end,
                                  args.carve_max_range, device)
            print("carved: %d of %d voxels" % (int(drop.sum()), drop.shape[0]))
            vmap = ops.voxel_map_keep(vmap, ~drop)
        cloud = map_cloud(vmap, args.min_count, args.normal_radius)
    except ValueError as e:
        ap.error(str(e))
    print("map: %d voxels from %d rows of %d frames" % (cloud.shape[1], total, len(files)))
    if args.out is not None:
        with open(args.out, "wb") as fh:                  # an open file: np.save adds no suffix to the name
            np.save(fh, cloud)


if __name__ == "__main__":
    main()
