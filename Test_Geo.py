#!/usr/bin/env python3
"""Evaluation of the geometric model with the reference's structure and output (Test_Geo.py:29-132: `python Test_Geo.py --dataset
kitti|nuscenes`), running the HIP path.

Per pair: the overlap head's precision / recall against pc_mask (computed by forward when the batch carries labels), the inlier ratio of
the nearest-feature matches of the ground-truth overlap points (IR, cal_match_accuracy), of the predicted overlap points (IR1) and of
those predicted points whose matched pixel is predicted to overlap too (IR2); a match is an inlier within 3 px of the projected point at
1/4 scale.  All three come from one cmr_feat_match_f32 launch per batch and ratio (per sample, then averaged over the pairs as the
reference's lists are).  The last line is the reference's: pc_overlap_precision pc_overlap_recall IR IR1 IR2.

Left out: the reference's IterModel call (:56-62, 79).  No number printed depends on it, and it needs label keys (R_amplitude,
label_R, ...) that no loader emits.

--pnp (port extension): also the camera pose from those IR2 matches alone, PnP inside RANSAC
(MultiHeadModel.pose_from_matches), scored per pair like Test_Agent.py (both poses through env.to_disentangled, get_P_diff; one line
"RTE RRE" per pair), then Test_Agent.py's closing lines: registration recall (RTE < 5 and RRE < 10) and the RTE / RRE mean and std of the
recalled pairs.  Without the flag the output is unchanged.

--mutual / --ratio R / --excl-radius K (with --pnp): the matches are filtered before PnP -- mutual nearest neighbours and
/ or Lowe's ratio test d1 <= R * d2 with d2 taken outside the (2K + 1)^2 window of the best pixel (cmr_feat_match_filter_f32) -- and each
batch prints one extra line "kept <kept> of <selected> IR <unfiltered> -> <kept>": the predicted-overlap matches that pass and their
inlier ratio beside the unfiltered one.  Without these flags the output is unchanged.

--guided R[,R...] (with --pnp; optional --guided-thr T[,T...], --guided-max-dist D): the PnP pose is refined by rounds of
(guided match inside the (2R + 1)^2 window round every point's projection -> Gauss-Newton on the kept matches with inlier threshold T;
MultiHeadModel.refine_pose_from_matches).  Per pair one extra line "refined <RTE> <RRE>" after the pair's "RTE RRE" line, and after the
closing block the same three lines again with the prefix "Refined ".  Without the flag the output is unchanged.

--subpixel (with --pnp): the correspondences handed to PnP, and to every --guided round, carry sub-pixel positions from a
parabola fit on the feature distances round the matched pixel (cmr_match_subpixel_f32) instead of the integer pixel, and each batch prints
one extra line "subpixel fitted <fitted> of <matched> IR@0.5 <integer> -> <sub-pixel>": the PnP correspondences fitted on both axes and
their share within 0.5 px (at 1/4 scale) of the projected point before and after the fit.  Without the flag the output is unchanged.

--min-conf C [--temperature T] (with --pnp, instead of --mutual / --ratio): only the matches whose dual-softmax confidence
(cmr_match_conf_f32: softmax over the point's row times softmax over the pixel's column of -d^2 / T, default T = 0.1) reaches C go into
PnP, and each batch prints one extra line "conf kept <kept> of <selected> IR <unfiltered> -> <kept>".  Without the flag the output is
unchanged.

--verify (with --pnp): the pair's candidate poses -- the PnP pose and, with --guided, the refined pose -- are scored
against the geometric features with no ground truth (MultiHeadModel.score_poses, window radius 0); per pair one extra line "verified
<name>=<quality> ... -> <chosen name>", quality = 1 - score / (selected tau^2) in [0, 1], and after the closing block(s) the same three
lines again for the chosen poses with the prefix "Verified ".  Without the flag the output is unchanged.

--verify-mi [--mi-bins NB] (with --pnp and --data-root): the same candidate poses are scored by the mutual information of
the LiDAR reflectance (the loader keeps it: FrameDataset(..., with_intensity=True)) and the image's grey values under each pose
(MultiHeadModel.score_poses_mi, NB x NB joint histogram, NB default 32) -- a score that reads the sensors, not the learned features;
per pair one extra line "mi <name>=<MI in nats> ... -> <chosen name>" and after the closing block(s) the same three lines for the chosen
poses with the prefix "MI-verified ".  Synthetic pairs have a noise image and no reflectance: without --data-root the flag is refused.
Without the flag the output is unchanged.

--visible (with --guided; optional --visible-radius R, --visible-rel-tol T, --visible-abs-tol A): every --guided round first
takes a z-buffer of the whole cloud under the round's pose (cmr_visibility_f32) and matches only the predicted-overlap points it leaves
visible: depth <= nearest depth in the (2R + 1)^2 cells round the point's own * (1 + T) + A, defaults 1 / 0.05 / 0.  Each batch prints
one extra line "visible <visible> of <in view> of <selected>" for the last round.  Without the flag the output is unchanged.

--paint DIR [--paint-visible] (with --pnp): every pair's cloud is painted with the image under the last pose the run produced
-- the verified choice with --verify, else the refined pose with --guided, else the PnP pose (cmr_paint_points_f32, bilinear) -- and
DIR/pair_<index>.ply holds the painted points (binary little-endian PLY: x y z float32 in the cloud's own frame, red green blue uchar =
clamp(rint(255 c), 0, 255)); --paint-visible paints only the points a z-buffer of the cloud under that pose leaves visible.  Each batch
prints one extra line "painted <painted> of <selected>".  Without the flag the output is unchanged.

--dense-depth DIR [--dense-radius R] [--dense-sigma-r S] [--dense-visible] (with --pnp): every pair's cloud is rendered at the
image's size under the same pose --paint uses (cmr_render_points_f32), the sparse depth is filled in by the joint bilateral filter guided
by the image (cmr_densify_f32; window radius R, default 8; range sigma S, default 0.1) and DIR/pair_<index>_depth.pfm holds the dense map
(PFM "Pf", little-endian, scale -1.0, rows bottom to top, unfilled pixels 0); --dense-visible renders only the points a z-buffer of the
cloud under that pose leaves visible.  Each batch prints one extra line "dense <filled> of <pixels> from <samples>".  Without the flag the
output is unchanged.

--dense-surfels (with --dense-depth) and --visible-surfels (with --visible) [--surfel-radius R] [--surfel-slope S] [--surfel-max-px M]
(DESIGN.md 4z): the cloud is drawn as oriented discs from its normals (cmr_render_surfels_f32; r = R + S z metres, defaults 0.1 and 0.004,
cut to the (2M + 1)^2 pixels round the centre, default 8; the normals are the batch's 'pc_normal' or are computed on the device).  With
--dense-surfels the map that is densified comes from the discs and each batch prints one more line "surfels <drawn> of <selected> own
<owned> of <pixels>"; with --visible-surfels every round's z-buffer is the surfel depth map of the whole cloud (cmr_depth_test_f32).
Without these flags the output is unchanged.

--from-raw (with --data-root): a sequence whose prepared cloud folder is missing is read from its raw scans
(<seq>/velodyne/*.bin) and voxel-downsampled on the device as it is loaded (FrameDataset(..., from_raw=True));
`python -m cmr_agent_amd.dataset.prepare --root DIR` writes the folder once instead.  Without the flag nothing changes.

--pc-subdir NAME (with --data-root): the clouds are read from <seq>/NAME instead of the prepared folder
(FrameDataset(..., pc_subdir=NAME)) -- the views of a map that `python -m cmr_agent_amd.dataset.view` wrote, so that the images are
registered against the map as a sensor at the frame's pose would see it.  Without the flag nothing changes.

Pairs come from the synthetic generator (cmr_agent_amd.utils.synthetic) unless --data-root names a dataset in the reference's layout
(its 'test' split), and the weights are the deterministic hash fill unless --geo-ckpt points at a reference-format state_dict."""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cmr_agent_amd import ops  # noqa: E402
from cmr_agent_amd.config import KittiConfiguration, NuScenesConfiguration  # noqa: E402
from cmr_agent_amd.dataset.sampling import hip_fps, hip_nearest  # noqa: E402
from cmr_agent_amd.environment import environment as env  # noqa: E402
from cmr_agent_amd.models import MultiHeadModel  # noqa: E402
from cmr_agent_amd.models.MultiHeadModel import match_features  # noqa: E402
from cmr_agent_amd.utils import hashfill, synthetic  # noqa: E402
from cmr_agent_amd.utils.checkpoint import load_checked  # noqa: E402
from cmr_agent_amd.utils.evalcli import (add_dense_flags, add_mi_flags, add_paint_flags, add_pc_subdir_flag, add_raw_flag, add_surfel_flags,  # noqa: E402
                                         add_visible_flags, dense_option, dense_pairs, guided_rounds, mi_option, paint_option, paint_pairs,
                                         pc_subdir_option, print_mi, print_recall, print_visible, raw_option, surfel_option, visible_option)


def _ratios(counts):
    c = counts.double().cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        return c[:, 1] / c[:, 0], c[:, 3] / c[:, 2]              # IR1, IR2 per sample (0 / 0 = NaN, as torch)


def get_P_diff(P_pred, P_gt):
    """Test_Agent.py:99-105 (scipy Euler 'XYZ' in degrees, summed absolute angles)."""
    from scipy.spatial.transform import Rotation
    r = Rotation.from_matrix(np.dot(P_pred[0:3, 0:3], P_gt[0:3, 0:3].T)).as_euler('XYZ', degrees=True)
    return np.linalg.norm(P_pred[0:3, 3] - P_gt[0:3, 3]), np.sum(np.abs(r))


def main():
    ap = argparse.ArgumentParser(description='Image to point Registration: geometric model matching (MI355X HIP path)')
    ap.add_argument('--dataset', type=str, default='kitti', help=" 'kitti' or 'nuscenes' ")
    ap.add_argument('--pairs', type=int, default=4, help="number of (image, cloud) pairs")
    ap.add_argument('--batch-size', type=int, default=1)
    ap.add_argument('--num-pt', type=int, default=None)
    ap.add_argument('--img', type=str, default=None, help="HxW network input size (multiples of 32), default from the config")
    ap.add_argument('--geo-ckpt', default=None)
    ap.add_argument('--data-root', default=None, help="dataset root in the reference's on-disk layout (cmr_agent_amd/dataset/loader.py): the 'test' split; "
                    "default: the synthetic generator")
    ap.add_argument('--pnp', action='store_true', help="also register each pair from the IR2 matches alone (PnP-RANSAC) and print "
                    "Test_Agent.py's RTE / RRE and registration recall")
    ap.add_argument('--mutual', action='store_true', help="with --pnp: keep only mutual nearest-neighbour matches")
    ap.add_argument('--ratio', type=float, default=None, help="with --pnp: Lowe's ratio test, keep a match when d1 <= RATIO * d2 (0 < RATIO <= 1)")
    ap.add_argument('--excl-radius', type=int, default=2, help="with --ratio: d2 is the best distance outside the (2K + 1)^2 window of the best pixel")
    ap.add_argument('--guided', type=str, default=None, help="with --pnp: refine the PnP pose by guided matching, one round per window radius R[,R...]")
    ap.add_argument('--guided-thr', type=str, default=None, help="with --guided: inlier threshold in pixels per round T[,T...] (default: R / 1.5 per round, at least 1)")
    ap.add_argument('--guided-max-dist', type=float, default=None, help="with --guided: keep a guided match only when its feature distance is <= D")
    ap.add_argument('--subpixel', action='store_true', help="with --pnp: sub-pixel match positions (parabola fit on the feature distances) for PnP and the --guided rounds")
    ap.add_argument('--min-conf', type=float, default=None, help="with --pnp: keep a match when its dual-softmax confidence is >= C (0 < C <= 1)")
    ap.add_argument('--temperature', type=float, default=None, help="with --min-conf: temperature T of the softmax over -d^2 / T (default 0.1)")
    ap.add_argument('--verify', action='store_true', help="with --pnp: score the pair's candidate poses against the geometric features (no ground truth) and report the best")
    add_visible_flags(ap, "--guided")
    add_paint_flags(ap, "--pnp")
    add_dense_flags(ap, "--pnp")
    add_mi_flags(ap, "--pnp")
    add_raw_flag(ap)
    add_pc_subdir_flag(ap)
    add_surfel_flags(ap)
    args = ap.parse_args()
    paint = paint_option(ap, args, "--pnp", args.pnp)
    dense = dense_option(ap, args, ops.DENSIFY_MAX_RADIUS, "--pnp", args.pnp)
    mi_bins = mi_option(ap, args, ops.POSE_MI_MAX_BINS, "--pnp", args.pnp)
    raw_kw = raw_option(ap, args)
    raw_kw.update(pc_subdir_option(ap, args))
    if args.verify and not args.pnp:
        ap.error("--verify scores the PnP pose (and the --guided one): give --pnp as well")
    filtered = args.mutual or args.ratio is not None
    if filtered and not args.pnp:
        ap.error("--mutual / --ratio filter the matches that go into PnP: give --pnp as well")
    if args.ratio is not None and not 0.0 < args.ratio <= 1.0:
        ap.error("--ratio must lie in (0, 1]")
    if args.excl_radius < 0:
        ap.error("--excl-radius must be >= 0")
    if args.subpixel and not args.pnp:
        ap.error("--subpixel refines the matches that go into PnP: give --pnp as well")
    if args.min_conf is not None:
        if not args.pnp:
            ap.error("--min-conf filters the matches that go into PnP: give --pnp as well")
        if filtered:
            ap.error("--min-conf and --mutual / --ratio are alternative filters: give one or the other")
        if not 0.0 < args.min_conf <= 1.0:
            ap.error("--min-conf must lie in (0, 1]")
    elif args.temperature is not None:
        ap.error("--temperature belongs to --min-conf")
    if args.temperature is not None and not 0.0 < args.temperature < float("inf"):
        ap.error("--temperature must be > 0")
    conf_kw = {} if args.min_conf is None else dict(min_conf=args.min_conf, temperature=0.1 if args.temperature is None else args.temperature)
    radii = thrs = None
    if args.guided is not None:
        if not args.pnp:
            ap.error("--guided refines the PnP pose: give --pnp as well")
        radii, thrs = guided_rounds(ap, args.guided, args.guided_thr, ops.GUIDED_MAX_RADIUS)
    elif args.guided_thr is not None or args.guided_max_dist is not None:
        ap.error("--guided-thr / --guided-max-dist belong to --guided")
    visible = visible_option(ap, args, "--guided", radii is not None, ops.GUIDED_MAX_RADIUS)
    dense, visible = surfel_option(ap, args, dense, visible, ops.SURFEL_MAX_PX)
    vis_kw = {} if visible is None else dict(visible=visible or True)
    dev = torch.device("cuda")
    Cfg = {"kitti": KittiConfiguration, "nuscenes": NuScenesConfiguration}[args.dataset]
    kw = {}
    if args.img:
        kw["cropped_img_H"], kw["cropped_img_W"] = (int(v) for v in args.img.lower().split("x"))
    config = Cfg(num_pt=args.num_pt, device=dev, data_root=args.data_root, **kw)
    spec = json.load(open(os.path.join(ROOT, "tests", "golden", "specs.json")))
    geo_model = MultiHeadModel(config)
    load_checked(geo_model, torch.load(args.geo_ckpt) if args.geo_ckpt else hashfill.make_state_dict(spec["geo"], "geo4/"))
    geo_model = geo_model.to(dev).eval()

    bs, nbatch = args.batch_size, (args.pairs + args.batch_size - 1) // args.batch_size
    prec, rec, ir, ir1, ir2 = [], [], [], [], []
    rte, rre, rte_ref, rre_ref, rte_ver, rre_ver = [], [], [], [], [], []
    rte_mi, rre_mi = [], []
    done = 0
    with torch.no_grad():
        if args.data_root:
            from cmr_agent_amd.dataset import FrameDataset, FrameLoader
            batches = itertools.islice(iter(FrameLoader(FrameDataset(args.data_root, config, 'test', device=dev, **({} if mi_bins is None else dict(with_intensity=True)), **raw_kw), bs, shuffle=False)), nbatch)
        else:
            batches = (synthetic.make_batch(bs, config.num_pt, config.cropped_img_H, config.cropped_img_W, config.num_node, hip_fps(dev),
                                            hip_nearest(dev), seed=config.seed + i, n_circle=16, device=dev) for i in range(nbatch))
        for data in batches:
            geo_model(data)
            if 'pc_overlap_precision' in data:
                prec.append(float(data['pc_overlap_precision']))
                rec.append(float(data['pc_overlap_recall']))
            geo_model.geo_head.cal_match_accuracy(data)
            ir.extend(data['matching_ir_per_sample'].double().cpu().numpy().tolist())
            img_overlap = ops.softmax2(data['_cmr']["img_overlap_logits"])[1]           # img_overlap_logits.argmax(0), Test_Geo.py:88
            _, _, counts, _ = match_features(data, data['pc_overlap_pred'], img_overlap=img_overlap)
            r1, r2 = _ratios(counts)
            ir1.extend(r1.tolist())
            ir2.extend(r2.tolist())
            print(np.mean(r1), np.mean(r2))
            if args.pnp:
                geo_model.pose_from_matches(data, img_overlap=img_overlap, mutual=args.mutual, ratio=args.ratio,
                                            excl_radius=args.excl_radius, subpixel=args.subpixel, **conf_kw)
                if conf_kw:
                    cc = data['pnp_conf_counts'].double().cpu().numpy().sum(0)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        print("conf kept", int(cc[1]), "of", int(cc[0]), "IR", cc[3] / cc[0], "->", cc[2] / cc[1])
                if filtered:
                    fc = data['pnp_filter_counts'].double().cpu().numpy().sum(0)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        print("kept", int(fc[1]), "of", int(fc[0]), "IR", fc[3] / fc[0], "->", fc[2] / fc[1])
                if args.subpixel:
                    sc = data['pnp_subpixel_counts'].double().cpu().numpy().sum(0)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        print("subpixel fitted", int(sc[1]), "of", int(sc[0]), "IR@0.5", sc[2] / sc[0], "->", sc[3] / sc[0])
                pred = env.to_disentangled(data['pnp_pose'].clone(), data['pc'])
                gt = env.to_disentangled(data['P'].to(dev).float().clone(), data['pc'])
                if radii is not None:
                    geo_model.refine_pose_from_matches(data, radii=radii, thrs=thrs, max_dist=args.guided_max_dist, img_overlap=img_overlap,
                                                       subpixel=args.subpixel, **vis_kw)
                    if vis_kw:
                        print_visible(data['refine_visible_counts'])
                    ref = env.to_disentangled(data['refined_pose'].clone(), data['pc'])
                names = ["pnp"] + (["refined"] if radii is not None else [])
                if args.verify:
                    geo_model.score_poses(data, torch.stack([data['pnp_pose']] + ([data['refined_pose']] if radii is not None else []), 1), radius=0)
                    chosen, quality = data['pose_best'].cpu().tolist(), data['pose_quality'].cpu().tolist()
                if mi_bins is not None:
                    geo_model.score_poses_mi(data, torch.stack([data['pnp_pose']] + ([data['refined_pose']] if radii is not None else []), 1), bins=mi_bins)
                    mi_chosen, mi_values = data['pose_mi_best'].cpu().tolist(), data['pose_mi'].cpu().tolist()
                for b in range(pred.shape[0]):
                    t_diff, r_diff = get_P_diff(pred[b].cpu().numpy(), gt[b].cpu().numpy())
                    print(t_diff, r_diff)
                    rte.append(t_diff)
                    rre.append(r_diff)
                    errs = [(t_diff, r_diff)]
                    if radii is not None:
                        t_diff, r_diff = get_P_diff(ref[b].cpu().numpy(), gt[b].cpu().numpy())
                        print("refined", t_diff, r_diff)
                        rte_ref.append(t_diff)
                        rre_ref.append(r_diff)
                        errs.append((t_diff, r_diff))
                    if args.verify:
                        print("verified", " ".join("%s=%.4f" % (n, q) for n, q in zip(names, quality[b])), "->", names[chosen[b]])
                        rte_ver.append(errs[chosen[b]][0])
                        rre_ver.append(errs[chosen[b]][1])
                    if mi_bins is not None:
                        print_mi(names, mi_values[b], mi_chosen[b])
                        rte_mi.append(errs[mi_chosen[b]][0])
                        rre_mi.append(errs[mi_chosen[b]][1])
                if paint is not None or dense is not None:
                    last = data['refined_pose'] if radii is not None else data['pnp_pose']
                    if args.verify:
                        last = torch.stack([data['pnp_pose']] + ([data['refined_pose']] if radii is not None else []), 1)[
                            torch.arange(pred.shape[0], device=dev), data['pose_best']]
                    if paint is not None:
                        paint_pairs(geo_model, data, last, paint, done)
                    if dense is not None:
                        dense_pairs(geo_model, data, last, dense, done)
            done += data['pc'].shape[0]

    mean = lambda v: float(np.mean(v)) if v else float("nan")
    print(mean(prec), mean(rec), mean(ir), mean(ir1), mean(ir2))
    if args.pnp:
        print_recall(rte, rre)
        if radii is not None:
            print_recall(rte_ref, rre_ref, "Refined ")
        if args.verify:
            print_recall(rte_ver, rre_ver, "Verified ")
        if mi_bins is not None:
            print_recall(rte_mi, rre_mi, "MI-verified ")


if __name__ == '__main__':
    main()
