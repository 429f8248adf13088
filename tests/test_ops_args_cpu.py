"""The wording of the matching and pose wrappers' argument checks, recorded (tests/golden/ops_arg_messages.json): one table of
(wrapper, argument, what is wrong with it, the keywords that differ from a good call), every case on CPU tensors at B = 2, N = 16, a 4 x 6
map, so none reaches the library -- the case with nothing wrong but the device is refused by the last check of its wrapper.  The strings
were recorded by running this table against the wrappers as they stood before their checks were stated once (`PYTHONPATH=. python
tests/test_ops_args_cpu.py --record` writes the file from the ops module it imports); a case is in the table only if the wrapper then
raised a ValueError of its own wording."""
import functools
import json
import math
import os
import sys

import pytest
import torch

from cmr_agent_amd import _lib, ops

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

    *[(who, "device", "everything right but the device", {}) for who in GOOD],
]
IDS = ["%s:%s:%s" % c[:3] for c in CASES]


def _message(who, bad):
    """what the wrapper says to the good call with `bad` laid over it: (type of the exception or None, its text)"""
    try:
        getattr(ops, who)(**{**GOOD[who], **bad})
    except Exception as e:                                                          # noqa: BLE001 -- the recorder reports what is no ValueError
        return type(e), str(e)
    return None, ""


@functools.lru_cache(None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_is_whole():
    assert len(set(IDS)) == len(IDS) and set(IDS) == set(_golden()) and {c[0] for c in CASES} == set(GOOD)
    for who in GOOD:                                                                # 10 or more cases per wrapper, the device case among them
        assert sum(c[0] == who for c in CASES) >= 10 and (who, "device") in {c[:2] for c in CASES}


@pytest.mark.parametrize("who,arg,what,bad", CASES, ids=IDS)
def test_message(who, arg, what, bad, monkeypatch):
    def touched(*a, **kw):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(_lib, "call", touched)
    kind, text = _message(who, bad)
    assert kind is ValueError and text == _golden()["%s:%s:%s" % (who, arg, what)]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_ops_args_cpu.py --record")
    _lib.load = _lib.call = None                                                    # no case may get that far
    got = {i: _message(c[0], c[3]) for i, c in zip(IDS, CASES)}
    other = {i: g for i, g in got.items() if g[0] is not ValueError or not g[1].startswith(i.split(":")[0] + ": ")}
    for i, (kind, text) in other.items():
        print("not recorded: %s -> %s %s" % (i, getattr(kind, "__name__", kind), text))
    json.dump({i: g[1] for i, g in got.items() if i not in other}, open(GOLDEN, "w"), indent=0, sort_keys=True)
    print("%d cases recorded, %d not" % (len(got) - len(other), len(other)))
