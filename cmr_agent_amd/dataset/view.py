"""A map of a sequence and the frames' poses -> per frame what a spinning LiDAR standing there would see of the map.

    --map FILE                                                            float32 [7, n] in frame A, as `accumulate --out` writes it    (read)
    --poses FILE                                                          12 numbers per line, as `align --out` / `posegraph --out`    (read)
    <root>/<data_velodyne>/sequences/<seq>/<scan-subdir>/<i>.npy          the prepared frames: their names say which frames there are   (listed)
    <root>/<data_velodyne>/sequences/<seq>/<subdir>/<i>.npy               float32 [7, k]: x, y, z, reflectance, nx, ny, nz in frame i   (written)

A map holds every wall of the block, the wall behind the wall included; a scan carries its own occlusion, and the image-to-cloud models
were built for scans.  Line j of the poses file maps frame A + j into frame A.  It is inverted in float64 (R^T, -R^T t) and rounded to
float32, the map is moved by it (in fp32, as every cloud kernel moves a row) and `ops.virtual_scan` (HIP, csrc/range_image.hip) keeps
per cell of a rows x cols range image the nearest row, and of those the rows that pass the windowed occlusion test.  The file holds those
rows in frame A + j: the moved coordinates, the reflectance, the map's normals turned by the same rotation in fp32.  It is one more
prepared cloud, and `FrameDataset(..., pc_subdir=<subdir>)` / `--pc-subdir <subdir>` of Test_Geo.py and Test_Agent.py read it in place of
the frame's own scan.  Existing files are kept unless --overwrite.  One line per frame and one at the end:

    view <i>: rows <k> of <binned> binned outside <o>
    views: <frames> frames, <total> rows

Angles are in degrees.  The defaults (a 64-beam sensor's field, a 3 x 3 window, 5 % in range) are not tuned on real data.

    python -m cmr_agent_amd.dataset.view --root DIR --sequence S --map FILE --poses FILE [--frames A:B --rows 64 --cols 1024 --elev-lo -25
                                         --elev-hi 3 --min-range 1 --max-range 80 --radius-rows 1 --radius-cols 1 --rel-tol 0.05
                                         --subdir map-view --scan-subdir voxel0.1-SNr0.6 --overwrite]
"""
import argparse
import math
import os

import numpy as np
import torch

from .. import ops
from . import align, prepare
from .align import device_pose, device_rows, read_poses


def inverse_pose(T):
    """float64 [4, 4] (R, t) -> (R^T, -R^T t), formed in float64: what maps frame A into the frame whose pose T is"""
    T = np.asarray(T, dtype=np.float64)
    inv = np.eye(4)
    inv[:3, :3] = T[:3, :3].T
    inv[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return inv


def moved_rows(rows, pose, shift=True):
    """rows float32 [k, 3] under pose float32 [4, 4], one rounded fp32 operation at a time in the order of the kernels' pose step (every
    torch operation below is one product or one sum): the bits `ops.range_image` binned.  shift=False turns without the translation."""
    x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
    out = []
    for r in range(3):
        v = (pose[r, 0] * x + pose[r, 1] * y) + pose[r, 2] * z
        out.append(v + pose[r, 3] if shift else v)
    return torch.stack(out, 1)


def map_view(xyz, refl, normals, pose, device=None, **kw):
    """The map's rows float32 [n, 3] / [n, 1] / [n, 3] (device tensors) seen from the float64 [4, 4] pose of a frame in the map's frame
    -> (float32 [7, k] numpy: the prepared cloud of the view in that frame, the ops.VirtualScan).  kw: ops.virtual_scan's."""
    inv = device_pose(inverse_pose(pose), device)
    scan = ops.virtual_scan(xyz, inv, **kw)
    keep = scan.rows
    cloud = torch.cat([moved_rows(xyz[keep], inv), refl[keep], moved_rows(normals[keep], inv, shift=False)], 1)
    return cloud.T.contiguous().cpu().numpy(), scan


def view_sequence(frames, poses, cloud, out_dir, overwrite=False, device=None, report=print, **kw):
    """frames: the frame numbers; poses float64 [len(frames), 4, 4]; cloud: the map float32 [7, n] (numpy).  Writes <out_dir>/<i>.npy per
    frame (kept when it exists, unless `overwrite`) -> (frames written, rows written).  `report` receives one line per written frame."""
    os.makedirs(out_dir, exist_ok=True)
    xyz, refl, normals = device_rows(cloud[0:3], device), device_rows(cloud[3:4], device), device_rows(cloud[4:7], device)
    written = total = 0
    for i, T in zip(frames, poses):
        out = os.path.join(out_dir, "%06d.npy" % i)
        if os.path.exists(out) and not overwrite:
            continue
        view, scan = map_view(xyz, refl, normals, T, device, **kw)
        np.save(out, view)
        report("view %d: rows %d of %d binned outside %d" % (i, view.shape[1], scan.image.binned, scan.image.outside))
        written, total = written + 1, total + view.shape[1]
    return written, total


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cmr_agent_amd.dataset.view", description=__doc__.split("\n\n")[0])
    align.sequence_flags(ap)
    for action in ap._actions:                                # --subdir names what is WRITTEN here; the frames are listed from --scan-subdir
        if action.dest == "subdir":
            action.default, action.help = "map-view", "the folder of the sequence the views are written to (default map-view)"
    ap.add_argument("--scan-subdir", default=prepare.subdir(), help="the prepared folder of the sequence whose file names say which frames "
                    "there are (default %s)" % prepare.subdir())
    ap.add_argument("--map", required=True, help="the map, float32 [7, n] in frame A: what `accumulate --out` wrote")
    ap.add_argument("--poses", required=True, help="the poses of the frames, 12 numbers per line: line j maps frame A + j into frame A")
    ap.add_argument("--rows", type=int, default=64, help="elevation rows of the range image (default 64)")
    ap.add_argument("--cols", type=int, default=1024, help="azimuth columns of the range image, a multiple of 4 (default 1024)")
    ap.add_argument("--elev-lo", type=float, default=-25.0, help="the lowest elevation in degrees (default -25)")
    ap.add_argument("--elev-hi", type=float, default=3.0, help="the highest elevation in degrees (default 3)")
    ap.add_argument("--min-range", type=float, default=1.0, help="rows nearer than this many metres are left out (default 1)")
    ap.add_argument("--max-range", type=float, default=80.0, help="rows at or beyond this many metres are left out (default 80)")
    ap.add_argument("--radius-rows", type=int, default=1, help="the occlusion window reaches this many image rows up and down (default 1)")
    ap.add_argument("--radius-cols", type=int, default=1, help="... and this many columns to either side, wrapping (default 1)")
    ap.add_argument("--rel-tol", type=float, default=0.05, help="a cell is kept when its range is within this share of the nearest one in "
                    "its window (default 0.05).  None of the defaults is tuned on real data")
    ap.add_argument("--overwrite", action="store_true", help="write files that exist again (default: keep them)")
    args = ap.parse_args(argv)
    align.check_sequence_flags(ap, args)
    prepare.check_positive(ap, args, "min_range", "max_range")
    if not 1 <= args.rows <= ops.RANGE_MAX_ROWS:
        ap.error("--rows must lie in [1, %d]" % ops.RANGE_MAX_ROWS)
    if not 4 <= args.cols <= ops.RANGE_MAX_COLS or args.cols % 4 or args.rows * args.cols > ops.RANGE_MAX_CELLS:
        ap.error("--cols must be a multiple of 4 in [4, %d] with rows x cols at most %d" % (ops.RANGE_MAX_COLS, ops.RANGE_MAX_CELLS))
    if not -90.0 < args.elev_lo < args.elev_hi < 90.0:
        ap.error("need -90 < --elev-lo < --elev-hi < 90 degrees, got %r and %r" % (args.elev_lo, args.elev_hi))
    if not args.min_range < args.max_range:
        ap.error("--min-range must be below --max-range, got %r and %r" % (args.min_range, args.max_range))
    for name in ("radius_rows", "radius_cols"):
        if not 0 <= getattr(args, name) < 1 << 30:
            ap.error("--%s must lie in [0, 2^30)" % name.replace("_", "-"))
    if min(2 * args.radius_rows + 1, args.rows) * min(2 * args.radius_cols + 1, args.cols) > ops.RANGE_MAX_WINDOW:
        ap.error("the window of --radius-rows and --radius-cols must hold at most %d cells of the image" % ops.RANGE_MAX_WINDOW)
    if not 0.0 <= args.rel_tol < float("inf"):
        ap.error("--rel-tol must be finite and >= 0, got %r" % args.rel_tol)
    if not args.subdir or os.path.basename(args.subdir) != args.subdir or args.subdir in (".", "..", args.scan_subdir, "velodyne"):
        ap.error("--subdir must be a folder name other than --scan-subdir and velodyne, got %r" % args.subdir)
    return ap, args


def read_map(path):
    """The map as accumulate writes it -> float32 [7, n]; ValueError for anything else."""
    try:
        return align.read_prepared(path)
    except (OSError, EOFError) as e:
        raise ValueError("%s: %s" % (path, e))


def main(argv=None, device=None):
    ap, args = parse_args(argv)
    listed = argparse.Namespace(**dict(vars(args), subdir=args.scan_subdir))
    files = align.sequence_files(ap, listed)
    try:
        poses = read_poses(args.poses)
        cloud = read_map(args.map)
    except ValueError as e:
        ap.error(str(e))
    if poses.shape[0] != len(files):
        ap.error("%s holds %d poses, --frames names %d frames" % (args.poses, poses.shape[0], len(files)))
    out_dir = os.path.join(args.root, args.data_velodyne, "sequences", "%02d" % args.sequence, args.subdir)
    try:
        written, total = view_sequence([i for i, _ in files], poses, cloud, out_dir, args.overwrite, device, rows=args.rows, cols=args.cols,
                                       elev_lo=math.radians(args.elev_lo), elev_hi=math.radians(args.elev_hi), min_range=args.min_range,
                                       max_range=args.max_range, radius=(args.radius_rows, args.radius_cols), rel_tol=args.rel_tol)
    except ValueError as e:
        ap.error(str(e))
    print("views: %d frames, %d rows" % (written, total))


if __name__ == "__main__":
    main()
