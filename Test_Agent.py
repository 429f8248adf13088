#!/usr/bin/env python3
"""Evaluation entry point with the reference's structure and flag (Test_Agent.py:108-206:
`python Test_Agent.py --dataset kitti|nuscenes`), running the HIP path.

There are no KITTI / nuScenes files and no checkpoints in this environment, so the loader is the
synthetic generator (cmr_agent_amd.utils.synthetic) and the weights are the deterministic hash
fill unless --geo-ckpt / --agent-ckpt point at reference-format state_dicts.  Metrics are the
reference's: RTE / RRE per pair and registration recall (RTE < 5 m and RRE < 10 deg, :198).

--refine R[,R...] (port extension; optional --guided-thr T[,T...], --guided-max-dist D): the agent's final pose, which sits on
the lattice of its step tables, is polished against the geometric features -- a clone of it through env.from_disentangled, rounds of
(guided match inside the (2R + 1)^2 window -> Gauss-Newton with inlier threshold T; MultiHeadModel.refine_pose_from_matches), back
through env.to_disentangled.  Per pair one extra line "refined <RTE> <RRE>", and after the closing block the same three lines again with
the prefix "Refined ".  Without the flag the output is unchanged.

--subpixel (with --refine): every round's correspondences carry sub-pixel positions from a parabola fit on the feature
distances round the matched pixel (cmr_match_subpixel_f32) instead of the integer pixel.  The lines printed are the same.

--visible (with --refine; optional --visible-radius R, --visible-rel-tol T, --visible-abs-tol A): every --refine round first
takes a z-buffer of the whole cloud under the round's pose (cmr_visibility_f32) and matches only the predicted-overlap points it leaves
visible: depth <= nearest depth in the (2R + 1)^2 cells round the point's own * (1 + T) + A, defaults 1 / 0.05 / 0.  Each pair prints
one extra line "visible <visible> of <in view> of <selected>" for the last round, before its "refined" line.

--search (port extension): the agent's final pose (through env.from_disentangled) is the start of the derivative-free
coarse-to-fine lattice search MultiHeadModel.search_pose (729 poses per round under cmr_pose_score_f32).  Per pair one extra line
"searched <RTE> <RRE>", and after the closing block(s) the same three lines again with the prefix "Searched ".

--verify: the candidate poses of the pair -- the agent's final pose, the refined pose (--refine), the searched pose
(--search) -- are scored against the geometric features with no ground truth (MultiHeadModel.score_poses, window radius 0) and the pair
prints "verified <name>=<quality> ... -> <chosen name>", quality = 1 - score / (selected tau^2) in [0, 1]; the chosen pose's RTE / RRE
are collected and the closing lines printed once more with the prefix "Verified ".  Without these flags the output is unchanged.

--verify-mi [--mi-bins NB] (with --data-root): the same candidate poses are scored by the mutual information of the LiDAR
reflectance (the loader keeps it: FrameDataset(..., with_intensity=True)) and the image's grey values under each pose
(MultiHeadModel.score_poses_mi, NB x NB joint histogram, NB default 32); the pair prints "mi <name>=<MI in nats> ... -> <chosen name>"
and the closing lines are printed once more for the chosen poses with the prefix "MI-verified ".  Synthetic pairs have a noise image and
no reflectance: without --data-root the flag is refused.  Without the flag the output is unchanged.

--paint DIR [--paint-visible]: every pair's cloud is painted with the image under the last pose the run produced -- the
refined pose with --refine, else the agent's final pose through env.from_disentangled (cmr_paint_points_f32, bilinear) -- and
DIR/pair_<index>.ply holds the painted points (binary little-endian PLY: x y z float32 in the cloud's own frame, red green blue uchar =
clamp(rint(255 c), 0, 255)); --paint-visible paints only the points a z-buffer of the cloud under that pose leaves visible.  Each pair
prints one extra line "painted <painted> of <selected>".  Without the flag the output is unchanged.

--dense-depth DIR [--dense-radius R] [--dense-sigma-r S] [--dense-visible]: every pair's cloud is rendered at the image's size
under the same pose --paint uses (cmr_render_points_f32), the sparse depth is filled in by the joint bilateral filter guided by the image
(cmr_densify_f32; window radius R, default 8; range sigma S, default 0.1) and DIR/pair_<index>_depth.pfm holds the dense map (PFM "Pf",
little-endian, scale -1.0, rows bottom to top, unfilled pixels 0); --dense-visible renders only the points a z-buffer of the cloud under
that pose leaves visible.  Each pair prints one extra line "dense <filled> of <pixels> from <samples>".  Without the flag the output is
unchanged.

--dense-surfels (with --dense-depth) and --visible-surfels (with --visible) [--surfel-radius R] [--surfel-slope S] [--surfel-max-px M]
(DESIGN.md 4z): the cloud is drawn as oriented discs from its normals (cmr_render_surfels_f32; r = R + S z metres, defaults 0.1 and 0.004,
cut to the (2M + 1)^2 pixels round the centre, default 8; the normals are the batch's 'pc_normal' or are computed on the device).  With
--dense-surfels the map that is densified comes from the discs and each pair prints one more line "surfels <drawn> of <selected> own
<owned> of <pixels>"; with --visible-surfels every round's z-buffer is the surfel depth map of the whole cloud (cmr_depth_test_f32).
Without these flags the output is unchanged.

--from-raw (with --data-root): a sequence whose prepared cloud folder is missing is read from its raw scans
(<seq>/velodyne/*.bin) and voxel-downsampled on the device as it is loaded (FrameDataset(..., from_raw=True));
`python -m cmr_agent_amd.dataset.prepare --root DIR` writes the folder once instead.  Without the flag nothing changes.

--pc-subdir NAME (with --data-root): the clouds are read from <seq>/NAME instead of the prepared folder
(FrameDataset(..., pc_subdir=NAME)) -- the views of a map that `python -m cmr_agent_amd.dataset.view` wrote, so that the images are
registered against the map as a sensor at the frame's pose would see it.  Without the flag nothing changes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC (RCCL on this host driver): read at HSA init, so set before any GPU call
os.environ.setdefault("ROC_CPU_WAIT_FOR_SIGNAL", "1")        # HIP runtime: cross-queue waits resolved on the host; replayed registration / agent update - 2 to - 3 % (bench.py, profiles/r06_ab_cpuwait.txt)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cmr_agent_amd import ops  # noqa: E402
from cmr_agent_amd.dataset.sampling import hip_fps, hip_nearest  # noqa: E402
from cmr_agent_amd.config import KittiConfiguration, NuScenesConfiguration  # noqa: E402
from cmr_agent_amd.environment import environment as env  # noqa: E402
from cmr_agent_amd.models import CMRAgent, MultiHeadModel  # noqa: E402
from cmr_agent_amd.utils import hashfill, synthetic  # noqa: E402
from cmr_agent_amd.utils.checkpoint import load_checked  # noqa: E402
from cmr_agent_amd.utils.evalcli import (add_dense_flags, add_mi_flags, add_paint_flags, add_pc_subdir_flag, add_raw_flag, add_surfel_flags,  # noqa: E402
                                         add_visible_flags, dense_option, dense_pairs, guided_rounds, mi_option, paint_option, paint_pairs,
                                         pc_subdir_option, print_mi, print_recall, print_visible, raw_option, surfel_option, visible_option)


def get_P_diff(P_pred, P_gt):
    """Test_Agent.py:99-105 (scipy Euler 'XYZ' in degrees, summed absolute angles)."""
    from scipy.spatial.transform import Rotation
    r = Rotation.from_matrix(np.dot(P_pred[0:3, 0:3], P_gt[0:3, 0:3].T)).as_euler('XYZ', degrees=True)
    return np.linalg.norm(P_pred[0:3, 3] - P_gt[0:3, 3]), np.sum(np.abs(r))


def main():
    ap = argparse.ArgumentParser(description='Image to point Registration (MI355X HIP path)')
    ap.add_argument('--dataset', type=str, default='kitti', help=" 'kitti' or 'nuscenes' ")
    ap.add_argument('--pairs', type=int, default=4, help="number of synthetic (image, cloud) pairs")
    ap.add_argument('--num-pt', type=int, default=None)
    ap.add_argument('--img', type=str, default=None, help="HxW network input size (multiples of 32), default from the config")
    ap.add_argument('--geo-ckpt', default=None)
    ap.add_argument('--agent-ckpt', default=None)
    ap.add_argument('--data-root', default=None, help="dataset root in the reference's on-disk layout (cmr_agent_amd/dataset/loader.py): the 'test' split; "
                    "default: the synthetic generator")
    ap.add_argument('--refine', type=str, default=None, help="refine the agent's final pose by guided matching, one round per window radius R[,R...]")
    ap.add_argument('--guided-thr', type=str, default=None, help="with --refine: inlier threshold in pixels per round T[,T...] (default: R / 1.5 per round, at least 1)")
    ap.add_argument('--guided-max-dist', type=float, default=None, help="with --refine: keep a guided match only when its feature distance is <= D")
    ap.add_argument('--subpixel', action='store_true', help="with --refine: sub-pixel match positions (parabola fit on the feature distances) in every round")
    ap.add_argument('--search', action='store_true', help="search round the agent's final pose on a coarse-to-fine pose lattice scored against the geometric features")
    ap.add_argument('--verify', action='store_true', help="score the pair's candidate poses against the geometric features (no ground truth) and report the best")
    add_visible_flags(ap, "--refine")
    add_paint_flags(ap)
    add_dense_flags(ap)
    add_mi_flags(ap)
    add_raw_flag(ap)
    add_pc_subdir_flag(ap)
    add_surfel_flags(ap)
    args = ap.parse_args()
    paint = paint_option(ap, args)
    dense = dense_option(ap, args, ops.DENSIFY_MAX_RADIUS)
    mi_bins = mi_option(ap, args, ops.POSE_MI_MAX_BINS)
    raw_kw = raw_option(ap, args)
    raw_kw.update(pc_subdir_option(ap, args))
    if args.subpixel and args.refine is None:
        ap.error("--subpixel belongs to --refine")
    radii = thrs = None
    if args.refine is not None:
        radii, thrs = guided_rounds(ap, args.refine, args.guided_thr, ops.GUIDED_MAX_RADIUS)
    elif args.guided_thr is not None or args.guided_max_dist is not None:
        ap.error("--guided-thr / --guided-max-dist belong to --refine")
    visible = visible_option(ap, args, "--refine", radii is not None, ops.GUIDED_MAX_RADIUS)
    dense, visible = surfel_option(ap, args, dense, visible, ops.SURFEL_MAX_PX)
    vis_kw = {} if visible is None else dict(visible=visible or True)
    dev = torch.device("cuda")
    Cfg = {"kitti": KittiConfiguration, "nuscenes": NuScenesConfiguration}[args.dataset]
    kw = {}
    if args.img:
        kw["cropped_img_H"], kw["cropped_img_W"] = (int(v) for v in args.img.lower().split("x"))
    config = Cfg(num_pt=args.num_pt, device=dev, data_root=args.data_root, **kw)
    spec = json.load(open(os.path.join(ROOT, "tests", "golden", "specs.json")))
    geo_model, agent = MultiHeadModel(config), CMRAgent(config)
    load_checked(geo_model, torch.load(args.geo_ckpt) if args.geo_ckpt else hashfill.make_state_dict(spec["geo"], "geo4/"))
    load_checked(agent, torch.load(args.agent_ckpt) if args.agent_ckpt else hashfill.make_state_dict(spec["agent"], "agent/"))
    geo_model, agent = geo_model.to(dev).eval(), agent.to(dev).eval()

    rte, rre, rte_ref, rre_ref = [], [], [], []
    rte_sea, rre_sea, rte_ver, rre_ver = [], [], [], []
    rte_mi, rre_mi = [], []
    with torch.no_grad():
        if args.data_root:
            from cmr_agent_amd.dataset import FrameDataset, FrameLoader
            import itertools
            frames = itertools.islice(iter(FrameLoader(FrameDataset(args.data_root, config, 'test', device=dev, **({} if mi_bins is None else dict(with_intensity=True)), **raw_kw), 1, shuffle=False)), args.pairs)
        else:
            frames = (synthetic.make_batch(1, config.num_pt, config.cropped_img_H, config.cropped_img_W, config.num_node,
                                           hip_fps(dev), hip_nearest(dev), seed=config.seed + i, n_circle=16, device=dev) for i in range(args.pairs))
        for index, data in enumerate(frames):                        # batch_size = 1 like the reference loader (:125)
            geo_model(data)
            pose_source, pose_target = env.init(data)
            pose_target = env.to_disentangled(pose_target, data['pc'], data=data)
            for _ in range(config.action_num):
                s2, s3 = env.observation_from_a_pose(data, pose_source, materialize_state_2d=False)
                r_logits, t_logits, _ = agent(s2, s3)
                action_r, action_t = agent.action_from_logits(r_logits, t_logits, deterministic=True)
                pose_source = env.step(action_r, action_t, pose_source, config)
            t_diff, r_diff = get_P_diff(pose_source[0].cpu().numpy(), pose_target[0].cpu().numpy())
            print(t_diff, r_diff)
            rte.append(t_diff)
            rre.append(r_diff)
            cands = [("agent", None, (t_diff, r_diff))]                 # (name, pose mapping 'pc' into the camera frame, (RTE, RRE))
            if args.search or args.verify or mi_bins is not None:
                final = env.from_disentangled(pose_source.clone(), data['pc'], data=data)
                cands[0] = ("agent", final, (t_diff, r_diff))
            if radii is not None:
                start = env.from_disentangled(pose_source.clone(), data['pc'], data=data)
                geo_model.refine_pose_from_matches(data, pose=start, radii=radii, thrs=thrs, max_dist=args.guided_max_dist,
                                                   subpixel=args.subpixel, **vis_kw)
                if vis_kw:
                    print_visible(data['refine_visible_counts'])
                ref = env.to_disentangled(data['refined_pose'].clone(), data['pc'], data=data)
                t_diff, r_diff = get_P_diff(ref[0].cpu().numpy(), pose_target[0].cpu().numpy())
                print("refined", t_diff, r_diff)
                rte_ref.append(t_diff)
                rre_ref.append(r_diff)
                cands.append(("refined", data['refined_pose'], (t_diff, r_diff)))
            if args.search:
                geo_model.search_pose(data, pose=final)
                sea = env.to_disentangled(data['searched_pose'].clone(), data['pc'], data=data)
                t_diff, r_diff = get_P_diff(sea[0].cpu().numpy(), pose_target[0].cpu().numpy())
                print("searched", t_diff, r_diff)
                rte_sea.append(t_diff)
                rre_sea.append(r_diff)
                cands.append(("searched", data['searched_pose'], (t_diff, r_diff)))
            if args.verify:
                geo_model.score_poses(data, torch.stack([c[1].float() for c in cands], 1), radius=0)
                k = int(data['pose_best'][0])
                quality = data['pose_quality'][0].cpu().tolist()
                print("verified", " ".join("%s=%.4f" % (c[0], q) for c, q in zip(cands, quality)), "->", cands[k][0])
                rte_ver.append(cands[k][2][0])
                rre_ver.append(cands[k][2][1])
            if mi_bins is not None:
                geo_model.score_poses_mi(data, torch.stack([c[1].float() for c in cands], 1), bins=mi_bins)
                k = int(data['pose_mi_best'][0])
                print_mi([c[0] for c in cands], data['pose_mi'][0].cpu().tolist(), k)
                rte_mi.append(cands[k][2][0])
                rre_mi.append(cands[k][2][1])
            if paint is not None or dense is not None:
                last = data['refined_pose'] if radii is not None else env.from_disentangled(pose_source.clone(), data['pc'], data=data)
                if paint is not None:
                    paint_pairs(geo_model, data, last, paint, index)
                if dense is not None:
                    dense_pairs(geo_model, data, last, dense, index)
    print_recall(rte, rre)
    if radii is not None:
        print_recall(rte_ref, rre_ref, "Refined ")
    if args.search:
        print_recall(rte_sea, rre_sea, "Searched ")
    if args.verify:
        print_recall(rte_ver, rre_ver, "Verified ")
    if mi_bins is not None:
        print_recall(rte_mi, rre_mi, "MI-verified ")


if __name__ == '__main__':
    main()
