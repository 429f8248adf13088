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

    python -m cmr_agent_amd.dataset.accumulate --root DIR --sequence S --poses FILE [--frames A:B --voxel 0.1 --extent 8192]
                                               [--normal-radius 0.6 --min-count 1 --out FILE]
"""
import argparse

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
    args = ap.parse_args(argv)
    align.check_sequence_flags(ap, args)
    prepare.check_positive(ap, args, "voxel", "extent", "normal_radius")
    if not 1 <= args.min_count < 1 << 31:
        ap.error("--min-count must lie in [1, 2^31)")
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
        cloud = map_cloud(vmap, args.min_count, args.normal_radius)
    except ValueError as e:
        ap.error(str(e))
    print("map: %d voxels from %d rows of %d frames" % (cloud.shape[1], total, len(files)))
    if args.out is not None:
        with open(args.out, "wb") as fh:                  # an open file: np.save adds no suffix to the name
            np.save(fh, cloud)


if __name__ == "__main__":
    main()
