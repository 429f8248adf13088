"""Command-line helpers shared by Test_Geo.py and Test_Agent.py: the round lists of --guided / --refine, the --visible flags, the --paint flags
with the per-pair PLY output, and the closing recall block."""
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


def print_recall(rte, rre, prefix=""):
    """Test_Agent.py's closing lines (registration recall: RTE < 5 and RRE < 10; mean / std of the recalled pairs), each with `prefix`."""
    rte, rre = np.array(rte), np.array(rre)
    mask = (rte < 5) & (rre < 10)
    print(prefix + "Registration Recall:", mask.sum() / mask.shape[0])
    if mask.any():
        print(prefix + 'RTE Mean:', rte[mask].mean(), 'RTE Std:', rte[mask].std())
        print(prefix + 'RRE Mean:', rre[mask].mean(), 'RRE Std:', rre[mask].std())
