"""Command-line helpers shared by Test_Geo.py and Test_Agent.py: the round lists of --guided / --refine, the --visible flags, the --paint flags
with the per-pair PLY output, the --dense-depth flags with the per-pair PFM output, the surfel flags that extend --dense-depth and --visible,
the --verify-mi flags, the --from-raw flag, and the closing recall block."""
import os

import numpy as np


def guided_rounds(ap, radii, thrs, max_radius):
    """'R[,R...]' and the optional 'T[,T...]' of --guided / --refine -> (radii, thrs), one pair per round; ap.error on a malformed list."""
    try:
        radii = tuple(int(v) for v in radii.split(","))
        thrs = tuple(float(v) for v in thrs.split(",")) if thrs is not None else tuple(max(1.0, r / 1.5) for r in radii)
    except ValueError:
        ap.error("window radii must be integers and thresholds numbers, comma separated")
    if len(radii) != len(thrs) or not all(0 <= r <= max_radius for r in radii) or not all(0.0 < t < float("inf") for t in thrs):
        ap.error("need one threshold > 0 per window radius, radii in [0, %d]" % max_radius)
    return radii, thrs


def add_visible_flags(ap, parent):
    """--visible and its three optional values; `parent` is the flag whose rounds it acts on (--guided / --refine)."""
    ap.add_argument('--visible', action='store_true', help="with %s: every round matches only the points a z-buffer of the cloud under the "
                    "round's pose leaves visible" % parent)
    ap.add_argument('--visible-radius', type=int, default=None, help="with --visible: the z-buffer is searched in the (2R + 1)^2 cells round the point's own (default 1)")
    ap.add_argument('--visible-rel-tol', type=float, default=None, help="with --visible: visible when depth <= nearest * (1 + T) + A (default T = 0.05)")
    ap.add_argument('--visible-abs-tol', type=float, default=None, help="with --visible: the A of the line above (default 0)")


def visible_option(ap, args, parent, parent_given, max_radius):
    """-> None without --visible, else the dict refine_pose_from_matches(visible=) takes; ap.error on a misplaced or malformed value."""
    given = {"radius": args.visible_radius, "rel_tol": args.visible_rel_tol, "abs_tol": args.visible_abs_tol}
    given = {k: v for k, v in given.items() if v is not None}
    if not args.visible:
        if given:
            ap.error("--visible-radius / --visible-rel-tol / --visible-abs-tol belong to --visible")
        return None
    if not parent_given:
        ap.error("--visible acts on the rounds of %s: give %s as well" % (parent, parent))
    if not 0 <= given.get("radius", 1) <= max_radius:
        ap.error("--visible-radius must lie in [0, %d]" % max_radius)
    if not all(0.0 <= given.get(k, 0.0) < float("inf") for k in ("rel_tol", "abs_tol")):
        ap.error("--visible-rel-tol and --visible-abs-tol must be finite and >= 0")
    return given


def print_visible(counts):
    """One line per batch from refine_pose_from_matches' 'refine_visible_counts' [rounds, B, 4]: the last round's, summed over the batch."""
    c = counts[-1].sum(0).cpu().tolist()
    print("visible", int(c[2]), "of", int(c[1]), "of", int(c[0]))


def add_paint_flags(ap, parent=None):
    """--paint DIR and --paint-visible; `parent` is the flag --paint needs beside it (None: free-standing)."""
    ap.add_argument('--paint', type=str, default=None, metavar="DIR", help="%spaint every pair's cloud with the image under the last pose the run "
                    "produced and write DIR/pair_<index>.ply (binary PLY: x y z float, red green blue uchar)" % ("with %s: " % parent if parent else ""))
    ap.add_argument('--paint-visible', action='store_true', help="with --paint: paint only the points a z-buffer of the cloud under that pose leaves visible")


def paint_option(ap, args, parent=None, parent_given=True):
    """-> None without --paint, else (DIR, visible); ap.error on a misplaced flag."""
    if args.paint is None:
        if args.paint_visible:
            ap.error("--paint-visible belongs to --paint")
        return None
    if parent is not None and not parent_given:
        ap.error("--paint paints under the pose %s produces: give %s as well" % (parent, parent))
    return args.paint, bool(args.paint_visible)


def paint_pairs(model, data, pose, option, first_index):
    """Paint the batch's clouds under `pose` (MultiHeadModel.paint_points, bilinear, every point or the visible ones), write one PLY per
    pair -- DIR/pair_<first_index + b>.ply with the painted points in the cloud's own frame; the first three planes are red, green, blue, a
    single plane is grey -- and print the batch's line."""
    import os

    from .ply import write_ply
    out_dir, visible = option
    os.makedirs(out_dir, exist_ok=True)
    model.paint_points(data, pose=pose, visible=True if visible else None)
    colors, painted = data['point_colors'].cpu(), data['point_painted'].cpu()
    if colors.shape[1] == 1:
        colors = colors.expand(-1, 3, -1)                                # a grey image: the one plane is red, green and blue
    elif colors.shape[1] < 3:
        raise ValueError("--paint writes red, green, blue: the image must have 1 plane (grey) or at least 3, got %d" % colors.shape[1])
    pc = data['pc'].float().cpu()
    for b in range(pc.shape[0]):
        m = painted[b]
        write_ply(os.path.join(out_dir, "pair_%d.ply" % (first_index + b)), pc[b][:, m].t(), colors[b][:3, m].t())
    c = data['paint_counts'].sum(0).cpu().tolist()
    print("painted", int(c[1]), "of", int(c[0]))


def add_dense_flags(ap, parent=None):
    """--dense-depth DIR, --dense-radius, --dense-sigma-r and --dense-visible; `parent` is the flag --dense-depth needs beside it (None:
    free-standing)."""
    ap.add_argument('--dense-depth', type=str, default=None, metavar="DIR", help="%srender every pair's cloud under the last pose the run produced, "
                    "fill the sparse depth in under the image's guidance and write DIR/pair_<index>_depth.pfm" % ("with %s: " % parent if parent else ""))
    ap.add_argument('--dense-radius', type=int, default=None, metavar="R", help="with --dense-depth: window radius of the filter in pixels (default 8)")
    ap.add_argument('--dense-sigma-r', type=float, default=None, metavar="S", help="with --dense-depth: range sigma on the image's values (default 0.1)")
    ap.add_argument('--dense-visible', action='store_true', help="with --dense-depth: render only the points a z-buffer of the cloud under that pose leaves visible")


def dense_option(ap, args, max_radius, parent=None, parent_given=True):
    """-> None without --dense-depth, else (DIR, radius, sigma_r, visible); ap.error on a misplaced or malformed flag."""
    if args.dense_depth is None:
        for name, given in (("--dense-radius", args.dense_radius is not None), ("--dense-sigma-r", args.dense_sigma_r is not None),
                            ("--dense-visible", args.dense_visible)):
            if given:
                ap.error("%s belongs to --dense-depth" % name)
        return None
    if parent is not None and not parent_given:
        ap.error("--dense-depth renders under the pose %s produces: give %s as well" % (parent, parent))
    radius = 8 if args.dense_radius is None else args.dense_radius
    sigma_r = 0.1 if args.dense_sigma_r is None else args.dense_sigma_r
    if not 0 <= radius <= max_radius:
        ap.error("--dense-radius must be in [0, %d] (--dense-depth), got %d" % (max_radius, radius))
    if not 0.0 < sigma_r < float("inf"):
        ap.error("--dense-sigma-r must be finite and > 0 (--dense-depth), got %r" % (sigma_r,))
    return args.dense_depth, radius, sigma_r, bool(args.dense_visible)


def dense_pairs(model, data, pose, option, first_index):
    """Densify the batch's rendered depth under `pose` (MultiHeadModel.dense_depth at the image's size, guided by the image), write one
    PFM per pair -- DIR/pair_<first_index + b>_depth.pfm, unfilled pixels as 0 -- and print the batch's line.  An option that
    surfel_option extended by a fifth entry (--dense-surfels) renders the cloud as surfels and prints one more line."""
    import os

    from .pfm import write_pfm
    out_dir, radius, sigma_r, visible = option[:4]
    kw = dict(surfels=option[4]) if len(option) > 4 else {}
    os.makedirs(out_dir, exist_ok=True)
    model.dense_depth(data, pose=pose, radius=radius, sigma_r=sigma_r, visible=True if visible else None, **kw)
    dense = data['dense_depth_map'].cpu()
    for b in range(dense.shape[0]):
        write_pfm(os.path.join(out_dir, "pair_%d_depth.pfm" % (first_index + b)), dense[b])
    c = data['dense_counts'].sum(0).cpu().tolist()
    print("dense", int(c[2]), "of", dense.shape[0] * dense.shape[1] * dense.shape[2], "from", int(c[0]))
    if kw:
        s = data['surfel_counts'].sum(0).cpu().tolist()
        print("surfels", int(s[1]), "of", int(s[0]), "own", int(s[2]), "of", dense.shape[0] * dense.shape[1] * dense.shape[2])


def add_surfel_flags(ap):
    """--dense-surfels (with --dense-depth), --visible-surfels (with --visible) and the three values both share."""
    ap.add_argument('--dense-surfels', action='store_true', help="with --dense-depth: render the cloud as oriented discs from its normals "
                    "instead of one cell per point")
    ap.add_argument('--visible-surfels', action='store_true', help="with --visible: the z-buffer is the surfel depth map of the whole cloud")
    ap.add_argument('--surfel-radius', type=float, default=None, metavar="R", help="with --dense-surfels / --visible-surfels: disc radius in "
                    "metres at range 0 (default 0.1)")
    ap.add_argument('--surfel-slope', type=float, default=None, metavar="S", help="with --dense-surfels / --visible-surfels: metres of radius "
                    "per metre of range (default 0.004)")
    ap.add_argument('--surfel-max-px', type=int, default=None, metavar="M", help="with --dense-surfels / --visible-surfels: a disc is cut to "
                    "the (2M + 1)^2 pixels round its centre (default 8)")


def surfel_option(ap, args, dense, visible, max_px):
    """dense_option's and visible_option's results with the surfel flags worked in -> (dense, visible): --dense-surfels appends the
    dict dense_depth(surfels=) takes to the dense option, --visible-surfels puts it under the key 'surfels' of the visible dict.
    Neither flag: both come back as they are.  ap.error on a misplaced or malformed flag."""
    given = {"radius": args.surfel_radius, "range_slope": args.surfel_slope, "max_px": args.surfel_max_px}
    given = {k: v for k, v in given.items() if v is not None}
    if args.dense_surfels and dense is None:
        ap.error("--dense-surfels belongs to --dense-depth")
    if args.visible_surfels and visible is None:
        ap.error("--visible-surfels belongs to --visible")
    if not (args.dense_surfels or args.visible_surfels):
        if given:
            ap.error("--surfel-radius / --surfel-slope / --surfel-max-px belong to --dense-surfels or --visible-surfels")
        return dense, visible
    if not all(0.0 <= given.get(k, 0.0) < float("inf") for k in ("radius", "range_slope")):
        ap.error("--surfel-radius and --surfel-slope must be finite and >= 0")
    if not 0 <= given.get("max_px", 0) <= max_px:
        ap.error("--surfel-max-px must lie in [0, %d]" % max_px)
    if args.dense_surfels:
        dense = tuple(dense) + (given or True,)
    if args.visible_surfels:
        visible = dict(visible, surfels=given or True)
    return dense, visible


def add_mi_flags(ap, parent=None):
    """--verify-mi and --mi-bins; `parent` is the flag --verify-mi needs beside it (None: free-standing)."""
    ap.add_argument('--verify-mi', action='store_true', help="%swith --data-root: score the pair's candidate poses by the mutual information of the "
                    "LiDAR reflectance and the image's grey values (no ground truth, no learned features) and report the best" % (
                        "with %s, " % parent if parent else ""))
    ap.add_argument('--mi-bins', type=int, default=None, metavar="NB", help="with --verify-mi: bins per axis of the joint histogram (default 32)")


def mi_option(ap, args, max_bins, parent=None, parent_given=True):
    """-> None without --verify-mi, else the bin count; ap.error on a misplaced or malformed flag."""
    if not args.verify_mi:
        if args.mi_bins is not None:
            ap.error("--mi-bins belongs to --verify-mi")
        return None
    if parent is not None and not parent_given:
        ap.error("--verify-mi scores the poses %s produces: give %s as well" % (parent, parent))
    if not args.data_root:
        ap.error("--verify-mi reads the reflectance of real frames: give --data-root as well (synthetic pairs have a noise image and no reflectance)")
    bins = 32 if args.mi_bins is None else args.mi_bins
    if not 2 <= bins <= max_bins:
        ap.error("--mi-bins must be in [2, %d] (--verify-mi), got %d" % (max_bins, bins))
    return bins


def add_raw_flag(ap):
    """--from-raw: the loader prepares raw scans on the fly (FrameDataset(..., from_raw=True))."""
    ap.add_argument('--from-raw', action='store_true', help="with --data-root: a sequence without the prepared cloud folder is read from its raw "
                    "scans (<seq>/velodyne/*.bin), voxel-downsampled on the device as it is loaded")


def raw_option(ap, args):
    """-> the keyword arguments --from-raw adds to FrameDataset; ap.error on a misplaced flag."""
    if not args.from_raw:
        return {}
    if not args.data_root:
        ap.error("--from-raw reads raw scans of real frames: give --data-root as well (synthetic pairs have no files)")
    return dict(from_raw=True)


def add_pc_subdir_flag(ap):
    """--pc-subdir: the loader reads another cloud folder of every sequence (FrameDataset(..., pc_subdir=NAME))."""
    ap.add_argument('--pc-subdir', default=None, metavar='NAME', help="with --data-root: read the clouds from <seq>/NAME instead of the prepared "
                    "folder, e.g. the views of a map that python -m cmr_agent_amd.dataset.view wrote")


def pc_subdir_option(ap, args):
    """-> the keyword arguments --pc-subdir adds to FrameDataset; ap.error on a misplaced flag."""
    if args.pc_subdir is None:
        return {}
    if not args.data_root:
        ap.error("--pc-subdir names a cloud folder of real frames: give --data-root as well (synthetic pairs have no files)")
    if not args.pc_subdir or os.path.basename(args.pc_subdir) != args.pc_subdir or args.pc_subdir in (".", ".."):
        ap.error("--pc-subdir must be a folder name, got %r" % args.pc_subdir)
    return dict(pc_subdir=args.pc_subdir)


def print_mi(names, values, chosen):
    """The per-pair line of --verify-mi: mi <name>=<value> ... -> <chosen name>."""
    print("mi", " ".join("%s=%.4f" % (n, v) for n, v in zip(names, values)), "->", names[chosen])


def print_recall(rte, rre, prefix=""):
    """Test_Agent.py's closing lines (registration recall: RTE < 5 and RRE < 10; mean / std of the recalled pairs), each with `prefix`."""
    rte, rre = np.array(rte), np.array(rre)
    mask = (rte < 5) & (rre < 10)
    print(prefix + "Registration Recall:", mask.sum() / mask.shape[0])
    if mask.any():
        print(prefix + 'RTE Mean:', rte[mask].mean(), 'RTE Std:', rte[mask].std())
        print(prefix + 'RRE Mean:', rre[mask].mean(), 'RRE Std:', rre[mask].std())
