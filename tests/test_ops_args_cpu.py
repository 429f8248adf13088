"""The wording of the matching and pose wrappers' argument checks, recorded (tests/golden/ops_arg_messages.json): one table of
(wrapper, argument, what is wrong with it, the keywords that differ from a good call), every case on CPU tensors at B = 2, N = 16, a 4 x 6
map, so none reaches the library -- the case with nothing wrong but the device is refused by the last check of its wrapper.  The strings
were recorded by running this table against the wrappers as they stood before their checks were stated once (`PYTHONPATH=. python
tests/test_ops_args_cpu.py --record` writes the file from the ops module it imports); a case is in the table only if the wrapper then
raised a ValueError of its own wording.

The eleven cloud wrappers follow in the same table on CPU tensors of 8 rows, with the faults their own CPU
tiers list; their strings were recorded against the wrappers as they stood before their prologues were stated once.  The
cases marked `behind` run with the device sentence of `ops._cloud_points` switched off, as those tiers do, to reach the checks after it.  The
three command-line drivers' `ap.error` texts are recorded the same way from stderr, the usage lines and the temporary folder's name cut."""
import functools
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import cloud_icp_reference
from cmr_agent_amd import _lib, ops
from cmr_agent_amd.dataset import accumulate, align, prepare

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_arg_messages.json")
B, N, H, W = 2, 16, 4, 6
INF, NAN = math.inf, math.nan
z = torch.zeros
PTS, UV, ROWS, IMG = z(B, 3, N), z(B, 2, N), z(B * N, 64), z(B, H, W, 64)
MASK, POSE, POSES, K = torch.ones(B, N, dtype=torch.bool), torch.eye(4).repeat(B, 1, 1), torch.eye(4).repeat(B, 3, 1, 1), torch.eye(3).repeat(B, 1, 1)
PAIR = dict(pc_feat_rows=ROWS, img_feat_nhwc=IMG, mask=MASK)
CLOUD = dict(pts=PTS, pose=POSE, K=K)

GOOD = {
    "feat_match": PAIR,
    "feat_match_filter": PAIR,
    "match_conf": PAIR,
    "pnp_ransac": dict(pts=PTS, uv=UV, mask=MASK, K=K),
    "guided_match": dict(PAIR, pts=PTS, pose=POSE, K=K, radius=2),
    "pose_score": dict(PAIR, pts=PTS, poses=POSES, K=K),
    "visibility": dict(CLOUD, h=H, w=W, mask=MASK),
    "paint_points": dict(CLOUD, image=z(B, 3, H, W)),
    "render_points": dict(CLOUD, h=H, w=W),
    "render_surfels": dict(CLOUD, normals=PTS, h=H, w=W),
    "depth_test": dict(CLOUD, depth_map=z(B, H, W), mask=MASK),
    "pose_mi": dict(pts=PTS, attr=z(B, N), grey=z(B, H, W), mask=MASK, poses=POSES, K=K),
    "densify": dict(depth=z(B, H, W)),
    "pnp_refine": dict(pts=PTS, uv=UV, mask=MASK, K=K, pose=POSE),
    "match_subpixel": dict(pc_feat_rows=ROWS, img_feat_nhwc=IMG, idx=z(B * N, dtype=torch.int32)),
}

# the cloud wrappers: 8 rows
P8, A8, D8, C5 = z(8, 3), z(8, 1), z(8, 33), z(5, 2, dtype=torch.int32)


def cloud_idx(n=8, cell=1.0):
    return ops.CloudIndex(z(n, 4), z(n, dtype=torch.int64), z(n, dtype=torch.int64), (0.0, 0.0, 0.0), cell, n, n)


def vmap(n=4, channels=1, **over):
    parts = dict(keys=torch.arange(n, dtype=torch.int64), points=z(n, 3), attr=z(n, channels), count=torch.ones(n, dtype=torch.int32),
                 stamp=z(n, dtype=torch.int32), origin=(0.0, 0.0, 0.0), voxel=0.5)
    parts.update(over)
    return ops.VoxelMap(**parts)


CLOUD_GOOD = {
    "voxel_downsample": dict(points=P8),
    "point_normals": dict(points=P8),
    "cloud_index": dict(points=P8, cell=1.0),
    "cloud_nearest": dict(index=cloud_idx(), queries=P8),
    "icp_point_to_plane": dict(source=P8, target=P8, target_normals=P8),
    "point_fpfh": dict(points=P8, normals=P8, radius=1.0),
    "descriptor_nearest": dict(queries=D8, targets=D8),
    "ransac_rigid": dict(source_pts=P8, target_pts=P8, corr=C5),
    "register_global": dict(source=P8, source_normals=P8, target=P8, target_normals=P8),
    "voxel_map": dict(voxel=0.1, origin=(0, 0, 0), device="cpu"),              # no tensor comes in: the one wrapper without a device case
    "voxel_map_insert": dict(map=vmap(), points=P8, attr=A8),
}
GOOD.update(CLOUD_GOOD)
BEHIND = set()                                                                  # ids that run with _cloud_points' device sentence switched off


# ---- the families of cases that recur ----------------------------------------------------------------------------------------------------
def tensor(who, arg, **bad):
    """one case per keyword: what is wrong = the keyword, the value = the tensor that is wrong in that way"""
    return [(who, arg, what.replace("_", " "), {arg: t}) for what, t in bad.items()]


def scalar(who, arg, *values):
    return [(who, arg, repr(v), {arg: v}) for v in values]


def pair(who):
    return (tensor(who, "pc_feat_rows", rank_3=z(B, N, 64), width_32=z(B * N, 32), float64=ROWS.double(), one_row_more=z(B * N + 1, 64))
            + tensor(who, "img_feat_nhwc", rank_3=z(B, H * W, 64), width_32=z(B, H, W, 32), float64=IMG.double()))


def cloud(who, *more):
    """pts and the [B, ...] float32 tensors that go with it, by name"""
    good = dict(pose=POSE, poses=POSES, K=K, uv=UV)
    return (tensor(who, "pts", rank_2=z(3, N), four_rows=z(B, 4, N), float64=PTS.double())
            + [c for a in more for c in tensor(who, a, one_sample=good[a][0], one_sample_more=torch.cat([good[a], good[a][:1]]), float64=good[a].double())])


def mask(who, arg="mask"):
    return tensor(who, arg, float32=z(B, N), one_element_more=torch.ones(B, N + 1, dtype=torch.bool))


def gt_xy(who):
    return tensor(who, "gt_xy", float64=UV.double(), pairs_last=z(B, N, 2))


def size(who):
    return (scalar(who, "h", 0, -1, 4.5, INF, NAN, True, "4") + scalar(who, "w", 0, 4.5, None)
            + [(who, "h", "over 2^24 pixels", dict(h=4097, w=4096))])


def attr(who):
    return tensor(who, "attr", rank_2=z(B, N), float16=z(B, 2, N).half(), one_sample_more=z(B + 1, 2, N), one_point_more=z(B, 2, N + 1),
                  no_plane=z(B, 0, N), planes_65=z(B, 65, N))


def empty(who, **kw):
    return [(who, "pts", "no points", dict(pts=z(B, 3, 0), mask=z(B, 0, dtype=torch.bool), **kw))]


def behind(cases):
    BEHIND.update("%s:%s:%s" % c[:3] for c in cases)
    return cases


def points(who, arg, more=False, none=True):
    """the malformed clouds the cloud tiers share"""
    bad = dict(width_2=z(8, 2), rank_1=z(8), rank_3=z(2, 8, 3), float64=P8.double(), numpy=np.zeros((8, 3), np.float32))
    if none:
        bad["none"] = None
    if more:
        bad.update(width_4=z(8, 4), int64=z(8, 3, dtype=torch.int64))
    return tensor(who, arg, **bad)


def poses(who):
    return tensor(who, "pose", three_by_three=torch.eye(3), float64=torch.eye(4).double(), numpy=np.eye(4, dtype=np.float32), a_batch=z(1, 4, 4))


BAD_SCALARS = (0.0, -0.1, INF, NAN, 1e-50, 1e39)
BAD_TRIPLES = ((0, 0), (0, 0, 0, 0), 1.0, (0, NAN, 0), (0, 0, INF))
NOT_INDEX = dict(none=None, a_pair=(P8, P8), a_tensor=P8)
MALFORMED = dict(
    keys_int32=dict(keys=z(4, dtype=torch.int32)), keys_rank_2=dict(keys=z(4, 1, dtype=torch.int64)), points_width_4=dict(points=z(4, 4)),
    points_3_rows=dict(points=z(3, 3)), points_float64=dict(points=z(4, 3).double()), attr_5_rows=dict(attr=z(5, 1)), attr_rank_1=dict(attr=z(4)),
    attr_none=dict(attr=None), count_int64=dict(count=torch.ones(4, dtype=torch.int64)), count_3_rows=dict(count=torch.ones(3, dtype=torch.int32)),
    stamp_float32=dict(stamp=z(4)), stamp_5_rows=dict(stamp=z(5, dtype=torch.int32)), voxel_0=dict(voxel=0.0), voxel_nan=dict(voxel=NAN),
    voxel_x=dict(voxel="x"), origin_pair=dict(origin=(0.0, 0.0)), origin_inf=dict(origin=(0.0, INF, 0.0)), origin_float64=dict(origin=(0.1, 0.0, 0.0)),
    origin_none=dict(origin=None), keys_numpy=dict(keys=np.zeros(4, np.int64)), points_on_meta=dict(points=z(4, 3, device="meta")))
BAD_STAMPS = (-1, 2 ** 31, 1.5, True, NAN, "3")

CLOUD_CASES = [
    *points("voxel_downsample", "points", more=True), *scalar("voxel_downsample", "voxel", *BAD_SCALARS),
    *tensor("voxel_downsample", "attr", seven_rows=z(7, 1), nine_rows_no_channel=z(9, 0), rank_1=z(8), float64=A8.double(), numpy=np.zeros((8, 1), np.float32)),
    *scalar("voxel_downsample", "origin", *BAD_TRIPLES),

    *points("point_normals", "points", more=True), *scalar("point_normals", "radius", *BAD_SCALARS), *scalar("point_normals", "viewpoint", *BAD_TRIPLES),

    *points("cloud_index", "points"), *scalar("cloud_index", "cell", *BAD_SCALARS),

    *tensor("cloud_nearest", "index", **NOT_INDEX), *scalar("cloud_nearest", "max_dist", *BAD_SCALARS, 1.5, 1.0000001), *points("cloud_nearest", "queries"),
    *behind(poses("cloud_nearest")),

    *scalar("icp_point_to_plane", "max_dist", *BAD_SCALARS),
    *[c for a in ("huber", "tol_rot", "tol_trans") for c in scalar("icp_point_to_plane", a, -0.1, INF, NAN, 1e39, "x", None)],
    *scalar("icp_point_to_plane", "iters", -1, 1001, 2.5, True, None, NAN),
    *tensor("icp_point_to_plane", "index", a_pair=(P8, P8)),
    *[("icp_point_to_plane", "index", "a cell of 0.5", dict(max_dist=1.0, index=cloud_idx(cell=0.5))),
      ("icp_point_to_plane", "target", "none and no index", dict(target=None))],
    *points("icp_point_to_plane", "source"),
    *behind(points("icp_point_to_plane", "target_normals")), *behind(points("icp_point_to_plane", "target", none=False)),
    *behind([("icp_point_to_plane", "target_normals", "seven rows", dict(target_normals=P8[:7])),
             ("icp_point_to_plane", "index", "nine rows", dict(target=None, index=cloud_idx(9))),
             ("icp_point_to_plane", "target", "seven rows and an index", dict(target=P8[:7], index=cloud_idx(8)))]),
    *behind(poses("icp_point_to_plane")),

    *scalar("point_fpfh", "radius", *BAD_SCALARS), *tensor("point_fpfh", "index", a_tensor=P8, a_pair=(P8, P8), a_string="x"),
    *[("point_fpfh", "radius", "%r with an index" % r, dict(radius=r, index=cloud_idx())) for r in (1.5, 1.0000001)],
    *points("point_fpfh", "points"),
    *behind(tensor("point_fpfh", "normals", width_2=z(8, 2), float64=P8.double(), none=None, seven_rows=P8[:7])),
    *behind([("point_fpfh", "index", "nine rows", dict(index=cloud_idx(9)))]),

    *[c for a in ("queries", "targets") for c in tensor("descriptor_nearest", a, rank_1=z(8), no_channel=z(8, 0), rank_3=z(2, 8, 33), float64=D8.double(),
                                                        none=None, numpy=np.zeros((8, 33), np.float32))],
    *tensor("descriptor_nearest", "targets", channels_32=z(8, 32)),
    *[("descriptor_nearest", "queries", "65 channels", dict(queries=z(8, 65), targets=z(4, 65)))],
    *[("descriptor_nearest", a, what, {a: m, b: D8[:5]}) for a, b in (("query_mask", "targets"), ("target_mask", "queries"))
      for what, m in dict(seven=z(7, dtype=torch.bool), rank_2=z(8, 1, dtype=torch.bool), float32=z(8), int64=z(8, dtype=torch.int64),
                          numpy=np.zeros(8, bool)).items()],
    *[("descriptor_nearest", "device", "with both masks", dict(query_mask=torch.ones(8, dtype=torch.bool), target_mask=torch.ones(8, dtype=torch.uint8)))],

    *scalar("ransac_rigid", "n_hyp", 0, -1, (1 << 20) + 1, 2.5, True, None, NAN), *scalar("ransac_rigid", "thr", *BAD_SCALARS),
    *scalar("ransac_rigid", "edge_ratio", -0.1, 1.5, NAN, INF, "x", None, True), *scalar("ransac_rigid", "seed", -1, 1 << 32, 0.5, None, True),
    *tensor("ransac_rigid", "corr", int64=z(5, 2, dtype=torch.int64), width_3=z(5, 3, dtype=torch.int32), rank_1=z(10, dtype=torch.int32), none=None,
            numpy=np.zeros((5, 2), np.int32)),
    *points("ransac_rigid", "source_pts"),
    *behind(tensor("ransac_rigid", "target_pts", width_2=z(8, 2), float64=P8.double(), none=None)),
    *behind([("ransac_rigid", "device", "behind the device look", {})]),

    *[("register_global", "mutual", "1", dict(mutual=1)), ("register_global", "refine", "None", dict(refine=None)),
      ("register_global", "mutual", "'yes'", dict(mutual="yes")), ("register_global", "icp", "pose and index", dict(pose=None, index=None))],
    *scalar("register_global", "radius", *BAD_SCALARS), *points("register_global", "source"),

    *scalar("voxel_map", "voxel", *BAD_SCALARS), *scalar("voxel_map", "origin", (0, 0), (0, 0, 0, 0), (0, NAN, 0), (0, 0, 1e39), 5, None),
    *scalar("voxel_map", "channels", -1, 1.5, None, True),

    *tensor("voxel_map_insert", "map", none=None, a_pair=(P8, P8), a_tensor=P8, a_plain_tuple=tuple(vmap())),
    *[("voxel_map_insert", "map", what.replace("_", " "), dict(map=vmap(**over))) for what, over in MALFORMED.items()],
    *scalar("voxel_map_insert", "stamp", *BAD_STAMPS, None), *scalar("voxel_map_insert", "min_stamp", *BAD_STAMPS),
    *[("voxel_map_insert", "attr", "without points", dict(points=None)), ("voxel_map_insert", "attr", "none for one channel", dict(attr=None)),
      ("voxel_map_insert", "attr", "one channel for none", dict(map=vmap(channels=0)))],
    *tensor("voxel_map_insert", "attr", rank_1=z(8), float64=A8.double(), numpy=np.zeros((8, 1), np.float32), two_channels=z(8, 2), seven_rows=A8[:7]),
    *poses("voxel_map_insert"),
    *[("voxel_map_insert", "points", c[2], dict(map=vmap(channels=0), attr=None, **c[3])) for c in points("voxel_map_insert", "points", none=False)],
    *[("voxel_map_insert", "map", "on the host, a pure prune", dict(points=None, attr=None, min_stamp=3))],

    *[(who, "device", "everything right but the device", {}) for who in CLOUD_GOOD if who != "voxel_map"],
]

NOT_INT = (1.5, INF, NAN, True, "2", None)
NOT_NUM = (INF, NAN, "x", None)

CASES = [
    *pair("feat_match"), *mask("feat_match"), *gt_xy("feat_match"),
    *tensor("feat_match", "img_feat_nhwc", no_sample=z(0, H, W, 64)),
    *tensor("feat_match", "img_overlap", int64=z(B, H, W, dtype=torch.int64), one_element_more=z(B * H * W + 1, dtype=torch.bool)),

    *pair("feat_match_filter"), *mask("feat_match_filter"), *gt_xy("feat_match_filter"),
    *tensor("feat_match_filter", "img_feat_nhwc", no_sample=z(0, H, W, 64), no_pixel=z(B, 0, W, 64)),
    *tensor("feat_match_filter", "pc_feat_rows", no_row=z(0, 64)),
    *scalar("feat_match_filter", "ratio", -0.1, 1.1, INF, NAN),
    *scalar("feat_match_filter", "excl_radius", -1, 1 << 31, 1.5, True, "2"),
    *scalar("feat_match_filter", "max_dist", -0.1, INF, NAN),

    *pair("match_conf"), *mask("match_conf"), *gt_xy("match_conf"),
    *tensor("match_conf", "img_feat_nhwc", no_sample=z(0, H, W, 64), no_pixel=z(B, 0, W, 64)),
    *tensor("match_conf", "pc_feat_rows", no_row=z(0, 64)),
    *scalar("match_conf", "temperature", 0.0, -1.0, INF, NAN),
    *scalar("match_conf", "min_conf", -0.1, 1.1, INF, NAN),

    *cloud("pnp_ransac", "uv", "K"), *mask("pnp_ransac"),
    *empty("pnp_ransac", uv=z(B, 2, 0)),
    *scalar("pnp_ransac", "n_hyp", 0, (1 << 20) + 1, 1.5, "8"),
    *scalar("pnp_ransac", "thr", 0.0, -1.0, INF, NAN),
    *scalar("pnp_ransac", "seed", -1, 1 << 32, 1.5, "8"),
    *scalar("pnp_ransac", "refine_iters", -1, 1.5, "8"),

    *cloud("guided_match", "pose", "K"), *pair("guided_match"), *mask("guided_match"), *gt_xy("guided_match"),
    *tensor("guided_match", "img_feat_nhwc", one_sample_more=z(B + 1, H, W, 64)),
    *empty("guided_match", pc_feat_rows=z(0, 64)),
    *[("guided_match", "img_feat_nhwc", "no pixel", dict(img_feat_nhwc=z(B, 0, W, 64)))],
    *scalar("guided_match", "radius", -1, ops.GUIDED_MAX_RADIUS + 1, *NOT_INT),
    *scalar("guided_match", "max_dist", -0.1, INF, NAN),

    *cloud("pose_score", "poses", "K"), *pair("pose_score"), *mask("pose_score"),
    *tensor("pose_score", "poses", rank_3=POSE, no_pose=z(B, 0, 4, 4), poses_4097=z(B, ops.POSE_SCORE_MAX_POSES + 1, 4, 4), three_by_four=z(B, 3, 3, 4)),
    *tensor("pose_score", "img_feat_nhwc", one_sample_more=z(B + 1, H, W, 64)),
    *empty("pose_score", pc_feat_rows=z(0, 64)),
    *scalar("pose_score", "radius", -1, ops.GUIDED_MAX_RADIUS + 1, *NOT_INT),
    *scalar("pose_score", "tau", 0.0, -1.0, *NOT_NUM),

    *cloud("visibility", "pose", "K"), *size("visibility"), *mask("visibility"), *mask("visibility", "occ_mask"), *empty("visibility"),
    *scalar("visibility", "radius", -1, ops.GUIDED_MAX_RADIUS + 1, *NOT_INT),
    *scalar("visibility", "rel_tol", -1e-3, 1e39, *NOT_NUM),
    *scalar("visibility", "abs_tol", -1e-3, 1e39, *NOT_NUM),

    *cloud("paint_points", "pose", "K"), *mask("paint_points"), *empty("paint_points"),
    *scalar("paint_points", "pts", None), *scalar("paint_points", "pose", None), *scalar("paint_points", "K", None), *scalar("paint_points", "mask", "m"),
    *tensor("paint_points", "image", rank_3=z(B, H, W), float64=z(B, 3, H, W).double(), one_sample_more=z(B + 1, 3, H, W), no_plane=z(B, 0, H, W),
            planes_65=z(B, 65, H, W), no_pixel=z(B, 3, 0, W)),
    *scalar("paint_points", "image", None),
    *scalar("paint_points", "mode", "cubic", 1, None),

    *cloud("render_points", "pose", "K"), *size("render_points"), *mask("render_points"), *attr("render_points"), *empty("render_points"),
    *scalar("render_points", "pts", None), *scalar("render_points", "attr", "a"), *scalar("render_points", "mask", "m"),
    *scalar("render_points", "splat", -1, ops.RENDER_MAX_SPLAT + 1, *NOT_INT),
    *scalar("render_points", "fill", "x", None, [0.0]),

    *cloud("render_surfels", "pose", "K"), *size("render_surfels"), *mask("render_surfels"), *attr("render_surfels"), *empty("render_surfels", normals=z(B, 3, 0)),
    *tensor("render_surfels", "normals", one_point_more=z(B, 3, N + 1), float64=PTS.double(), points_first=z(B, N, 3)),
    *scalar("render_surfels", "normals", None, [0.0]), *scalar("render_surfels", "pts", None), *scalar("render_surfels", "mask", "m"),
    *scalar("render_surfels", "radius", -0.1, 1e39, True, *NOT_NUM),
    *scalar("render_surfels", "range_slope", -0.1, 1e39, True, *NOT_NUM),
    *scalar("render_surfels", "min_cos", -0.1, 1.5, True, *NOT_NUM),
    *scalar("render_surfels", "max_px", -1, ops.SURFEL_MAX_PX + 1, *NOT_INT),
    *scalar("render_surfels", "fill", "x", None, [0.0]),

    *cloud("depth_test", "pose", "K"), *mask("depth_test"), *scalar("depth_test", "mask", None),
    *tensor("depth_test", "depth_map", rank_2=z(H, W), rank_4=z(B, 1, H, W), float64=z(B, H, W).double(), one_sample_more=z(B + 1, H, W), no_pixel=z(B, 0, W)),
    *scalar("depth_test", "depth_map", None, [1.0]),
    *scalar("depth_test", "radius", -1, ops.GUIDED_MAX_RADIUS + 1, *NOT_INT),
    *scalar("depth_test", "rel_tol", -1e-3, 1e39, *NOT_NUM),
    *scalar("depth_test", "abs_tol", -1e-3, 1e39, *NOT_NUM),

    *cloud("pose_mi", "poses", "K"), *mask("pose_mi"), *scalar("pose_mi", "pts", None), *scalar("pose_mi", "attr", None), *scalar("pose_mi", "mask", "m"),
    *empty("pose_mi", attr=z(B, 0)),
    *tensor("pose_mi", "attr", rank_3=z(B, 1, N), one_point_more=z(B, N + 1), float64=z(B, N).double()),
    *tensor("pose_mi", "grey", rank_4=z(B, 1, H, W), one_sample_more=z(B + 1, H, W), float64=z(B, H, W).double(), no_pixel=z(B, 0, W)),
    *tensor("pose_mi", "poses", rank_3=POSE, no_pose=z(B, 0, 4, 4), poses_4097=z(B, ops.POSE_SCORE_MAX_POSES + 1, 4, 4)),
    *scalar("pose_mi", "bins", 1, ops.POSE_MI_MAX_BINS + 1, *NOT_INT),
    *scalar("pose_mi", "mode", "cubic", 1, None),
    *scalar("pose_mi", "attr_range", (1.0, 1.0), (1.0, 0.0), (0.0, INF), (NAN, 1.0), (0.0, 1e-40), (0.0,), 1.0, "ab", None),
    *scalar("pose_mi", "grey_range", (1.0, 1.0), (0.0, INF), (0.0, 1.0, 2.0), None),

    *tensor("densify", "depth", rank_2=z(H, W), float64=z(B, H, W).double(), no_sample=z(0, H, W), no_pixel=z(B, H, 0)),
    *scalar("densify", "depth", None),
    *tensor("densify", "guide", rank_3=z(B, H, W), float64=z(B, 3, H, W).double(), one_sample_more=z(B + 1, 3, H, W), one_row_more=z(B, 3, H + 1, W),
            no_plane=z(B, 0, H, W), planes_5=z(B, ops.DENSIFY_MAX_C + 1, H, W)),
    *tensor("densify", "attr", rank_3=z(B, H, W), float64=z(B, 3, H, W).double(), one_sample_more=z(B + 1, 3, H, W), one_column_more=z(B, 3, H, W + 1),
            no_plane=z(B, 0, H, W), planes_5=z(B, ops.DENSIFY_MAX_C + 1, H, W)),
    *scalar("densify", "guide", "g"), *scalar("densify", "attr", "a"),
    *scalar("densify", "radius", -1, ops.DENSIFY_MAX_RADIUS + 1, *NOT_INT),
    *scalar("densify", "sigma_s", 0.0, -1.0, 1e-50, 1e39, 1e-20, INF, NAN, "x"),
    *scalar("densify", "sigma_r", 0.0, -1.0, 1e-50, 1e39, *NOT_NUM),
    *[("densify", "sigma_r", "1e-20 with a guide", dict(sigma_r=1e-20, guide=z(B, 1, H, W)))],
    *scalar("densify", "min_weight", 0.0, ops.DENSIFY_MIN_WEIGHT / 2, 1e39, *NOT_NUM),
    *scalar("densify", "keep", 2, 1.0, "yes", None),
    *scalar("densify", "fill", "x", None, [0.0]),

    *cloud("pnp_refine", "uv", "K", "pose"), *mask("pnp_refine"), *empty("pnp_refine", uv=z(B, 2, 0)),
    *scalar("pnp_refine", "thr", 0.0, -1.0, INF, NAN),
    *scalar("pnp_refine", "iters", -1, 1001, *NOT_INT),

    *pair("match_subpixel"), *mask("match_subpixel"), *gt_xy("match_subpixel"),
    *tensor("match_subpixel", "img_feat_nhwc", no_sample=z(0, H, W, 64), no_pixel=z(B, 0, W, 64)),
    *tensor("match_subpixel", "pc_feat_rows", no_row=z(0, 64)),
    *tensor("match_subpixel", "idx", int64=z(B * N, dtype=torch.int64), one_element_more=z(B * N + 1, dtype=torch.int32)),
    *scalar("match_subpixel", "thr", 0.0, -1.0, INF, NAN),

    *[(who, "device", "everything right but the device", {}) for who in GOOD if who not in CLOUD_GOOD],
    *CLOUD_CASES,
]
IDS = ["%s:%s:%s" % c[:3] for c in CASES]


def _shape_only(t, name="points", real=ops._cloud_points):
    """ops._cloud_points without its device sentence"""
    try:
        return real(t, name)
    except ValueError as e:
        if "device tensor" not in str(e):
            raise
        return t


def _message(who, bad, behind=False):
    """what the wrapper says to the good call with `bad` laid over it: (type of the exception or None, its text)"""
    real = ops._cloud_points
    if behind:
        ops._cloud_points = _shape_only
    try:
        getattr(ops, who)(**{**GOOD[who], **bad})
    except Exception as e:                                                          # noqa: BLE001 -- the recorder reports what is no ValueError
        return type(e), str(e)
    finally:
        ops._cloud_points = real
    return None, ""


@functools.lru_cache(None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_is_whole():
    assert len(set(IDS)) == len(IDS) and set(IDS) == set(_golden()) and {c[0] for c in CASES} == set(GOOD)
    for who in GOOD:                                                                # 10 or more cases per wrapper, the device case among them
        assert sum(c[0] == who for c in CASES) >= 10 and ((who, "device") in {c[:2] for c in CASES} or who == "voxel_map")
    assert BEHIND <= set(IDS) and all(i.split(":")[0] in CLOUD_GOOD for i in BEHIND)


@pytest.mark.parametrize("who,arg,what,bad", CASES, ids=IDS)
def test_message(who, arg, what, bad, monkeypatch):
    def touched(*a, **kw):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(_lib, "call", touched)
    kind, text = _message(who, bad, "%s:%s:%s" % (who, arg, what) in BEHIND)
    assert kind is ValueError and text == _golden()["%s:%s:%s" % (who, arg, what)]


# ---- the drivers' ap.error texts ---------------------------------------------------------------------------------------------------------
DRIVER_GOLDEN = os.path.join(os.path.dirname(GOLDEN), "cloud_driver_messages.json")
SEQ = ["--data-velodyne", "vel", "--sequence"]
DRIVER_CASES = [
    *[("prepare", " ".join(a), ["--root", "d"] + a) for a in (["--voxel", "0"], ["--voxel", "nan"], ["--sn-radius", "-1"], ["--sn-radius", "inf"],
                                                               ["--sequences", "9,x"], ["--sequences", "100"])],
    ("prepare", "no such root", ["--root", "<root>/missing"]),
    ("prepare", "no such sequence", ["--root", "<root>", "--data-velodyne", "vel", "--sequences", "12"]),
    *[("align", " ".join(a), ["--root", "<root>"] + SEQ + ["9"] + a) for a in (
        ["--frames", "5"], ["--frames", "6:2"], ["--frames", "a:b"], ["--max-dist", "0"], ["--max-dist", "nan"], ["--huber", "-1"], ["--iters", "1001"],
        ["--iters", "-1"], ["--fpfh-radius", "0"], ["--fpfh-radius", "inf"], ["--ransac-hyp", "0"], ["--ransac-hyp", "1048577"], ["--ransac-thr", "-1"],
        ["--ransac-thr", "nan"], ["--seed", "-1"], ["--seed", "4294967296"], ["--map", "-1"], ["--map-voxel", "0"], ["--map-extent", "inf"],
        ["--map-normal-radius", "nan"])],
    ("align", "--sequence 100", ["--root", "<root>"] + SEQ + ["100"]),
    ("align", "no such folder", ["--root", "<root>"] + SEQ + ["8"]),
    ("align", "[4, n] files", ["--root", "<root>"] + SEQ + ["10"]),
    ("align", "a frame is missing", ["--root", "<root>"] + SEQ + ["11"]),
    ("align", "a frame is missing, --map", ["--root", "<root>"] + SEQ + ["11", "--map", "2"]),
    *[("accumulate", " ".join(a), ["--root", "<root>"] + SEQ + ["9", "--poses", "<root>/two.txt"] + a) for a in (
        ["--voxel", "0"], ["--extent", "nan"], ["--normal-radius", "-1"], ["--min-count", "0"], ["--frames", "a:b"])],
    ("accumulate", "--sequence 100", ["--root", "<root>"] + SEQ + ["100", "--poses", "<root>/two.txt"]),
    ("accumulate", "no such folder", ["--root", "<root>"] + SEQ + ["8", "--poses", "<root>/two.txt"]),
    ("accumulate", "[4, n] files", ["--root", "<root>"] + SEQ + ["10", "--poses", "<root>/two.txt"]),
    ("accumulate", "three poses for two frames", ["--root", "<root>"] + SEQ + ["9", "--poses", "<root>/three.txt"]),
    ("accumulate", "eleven numbers per line", ["--root", "<root>"] + SEQ + ["9", "--poses", "<root>/eleven.txt"]),
]
DRIVER_IDS = ["%s:%s" % c[:2] for c in DRIVER_CASES]


def _driver_tree(root):
    """sequence 9: frames 3 and 4; 10: [4, n] files; 11: frames 3 and 5; the poses files"""
    frame = np.zeros((7, 5), np.float32)
    cloud_icp_reference.write_frames(root, [frame, frame], seq=9)
    cloud_icp_reference.write_frames(root, [frame[:4], frame[:4]], seq=10)
    folder = cloud_icp_reference.write_frames(root, [frame, frame, frame], seq=11)
    os.remove(os.path.join(folder, "000004.npy"))
    line = "1 0 0 0 0 1 0 0 0 0 1 0\n"
    for name, text in (("two.txt", line * 2), ("three.txt", line * 3), ("eleven.txt", line[2:] * 2)):
        with open(os.path.join(root, name), "w") as fh:
            fh.write(text)


def _driver_message(root, driver, argv, capsys):
    """-> what the driver's parser says after `error: ` when it ends the run, the folder's name replaced; None when it does not end it"""
    capsys.readouterr()
    try:
        {"prepare": prepare, "align": align, "accumulate": accumulate}[driver].main([a.replace("<root>", root) for a in argv], device="cpu")
    except SystemExit:
        err = capsys.readouterr().err
        return err[err.index(": error: ") + 9:].replace(root, "<root>")
    return None


@functools.lru_cache(None)
def _driver_golden():
    with open(DRIVER_GOLDEN) as f:
        return json.load(f)


def test_driver_messages(tmp_path, capsys, monkeypatch):
    def touched(*a, **kw):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(_lib, "call", touched)
    root = str(tmp_path)
    _driver_tree(root)
    assert len(set(DRIVER_IDS)) == len(DRIVER_IDS) and set(DRIVER_IDS) == set(_driver_golden())
    for i, (driver, _, argv) in zip(DRIVER_IDS, DRIVER_CASES):
        assert _driver_message(root, driver, argv, capsys) == _driver_golden()[i], i


class _Capsys:
    """pytest's capsys for the recorder: stderr into a buffer"""

    def readouterr(self):
        import collections
        import io
        err = sys.stderr.getvalue() if isinstance(sys.stderr, io.StringIO) else ""
        sys.stderr = io.StringIO()
        return collections.namedtuple("Captured", "out err")("", err)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_ops_args_cpu.py --record")
    _lib.load = _lib.call = None                                                    # no case may get that far
    got = {i: _message(c[0], c[3], i in BEHIND) for i, c in zip(IDS, CASES)}
    # the cloud wrappers name the argument first and the wrapper only where two share a check: any ValueError of theirs is their wording
    other = {i: g for i, g in got.items()
             if g[0] is not ValueError or not (i.split(":")[0] in CLOUD_GOOD or g[1].startswith(i.split(":")[0] + ": "))}
    for i, (kind, text) in other.items():
        print("not recorded: %s -> %s %s" % (i, getattr(kind, "__name__", kind), text))
    json.dump({i: g[1] for i, g in got.items() if i not in other}, open(GOLDEN, "w"), indent=0, sort_keys=True)
    print("%d cases recorded, %d not" % (len(got) - len(other), len(other)))
    import tempfile
    stderr = sys.stderr
    with tempfile.TemporaryDirectory() as root:
        _driver_tree(root)
        said = {i: _driver_message(root, c[0], c[2], _Capsys()) for i, c in zip(DRIVER_IDS, DRIVER_CASES)}
    sys.stderr = stderr
    for i in said:
        if said[i] is None:
            print("not recorded: %s ended without an error" % i)
    json.dump({i: t for i, t in said.items() if t is not None}, open(DRIVER_GOLDEN, "w"), indent=0, sort_keys=True)
    print("%d driver messages recorded" % sum(t is not None for t in said.values()))
