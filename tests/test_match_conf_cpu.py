"""CPU tier of the dual-softmax match confidence: the float64 restatement in match_conf_reference.py is right on a scene
worked out by hand and does on planted scenes what the confidence is for (so the yardstick of the GPU tests is itself checked), the
scenes of the GPU tier keep the share of near rows under the cap, ops.match_conf refuses malformed arguments before any launch, and the
header declares the entry points."""
import inspect
import math
import os
import re

import pytest
import torch

import match_conf_reference as ref
import match_filter_reference as fref
from cmr_agent_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_on_a_hand_made_scene():
    """2 x 2 map, e_k = k-th unit vector of R^64, pixel p has feature e_p, T = 1.  Points: 0 = e_1, 1 = e_1 (its duplicate), 2 = e_3
    unselected, 3 = e_2.  Squared distances are 0 (same vector) or 2, so with a = exp(-2):
      every selected row:  row sum = 1 + 3 a;
      column 1 (rows 0, 1 at distance 0, row 3 at 2): 2 + a;  column 2 (row 3 at 0, rows 0, 1 at 2): 1 + 2 a;  columns 0 and 3: 3 a;
      conf[0] = conf[1] = 1 / ((1 + 3 a)(2 + a)),  conf[3] = 1 / ((1 + 3 a)(1 + 2 a))."""
    e = torch.eye(64)
    img = e[:4].reshape(1, 2, 2, 64).contiguous()
    pc = torch.stack([e[1], e[1], e[3], e[2]])
    mask = torch.tensor([[1, 1, 0, 1]])
    xy = torch.tensor([[[1.0, math.nan, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0]]])       # row 0 on its pixel, row 1 not finite, row 3 one pixel off
    a = math.exp(-2.0)
    c01, c3 = 1.0 / ((1 + 3 * a) * (2 + a)), 1.0 / ((1 + 3 * a) * (1 + 2 * a))
    assert c01 < 0.4 < c3
    r = ref.restate(pc, img, mask, temperature=1.0, min_conf=0.4, gt_xy=xy, thr=0.5)[0]
    assert r["idx"].tolist() == [1, 1, -1, 2]
    assert torch.allclose(r["conf"][[0, 1, 3]], torch.tensor([c01, c01, c3], dtype=torch.float64), rtol=1e-12)
    assert torch.allclose(r["row_lse"][[0, 1, 3]], torch.full((3,), math.log(1 + 3 * a), dtype=torch.float64), rtol=1e-12)
    assert torch.allclose(r["col_lse"], torch.tensor([3 * a, 2 + a, 1 + 2 * a, 3 * a], dtype=torch.float64).log(), rtol=1e-12)
    assert torch.allclose(r["d1"][[0, 1, 3]], torch.zeros(3, dtype=torch.float64))
    assert torch.isnan(r["conf"][2]) and torch.isnan(r["row_lse"][2]) and torch.isnan(r["d1"][2])
    assert r["keep"].tolist() == [False, False, False, True]
    assert r["counts"] == [3, 1, 0, 1]                                 # only row 0 is an inlier, and it is not kept
    assert torch.allclose(r["fwd_gap"], torch.full((3,), math.sqrt(2.0), dtype=torch.float64))
    assert torch.allclose(r["conf_gap"], torch.tensor([math.log(0.4 / c01)] * 2 + [math.log(c3 / 0.4)], dtype=torch.float64), rtol=1e-12)
    assert r["near"].tolist() == [False, False, False]
    # no threshold: the mask is kept; nothing selected: fill values
    r0 = ref.restate(pc, img, mask, temperature=1.0, min_conf=0.0, gt_xy=xy, thr=0.5)[0]
    assert r0["keep"].tolist() == [True, True, False, True] and r0["counts"] == [3, 3, 1, 1]
    empty = ref.restate(pc, img, torch.zeros(1, 4, dtype=torch.int64), temperature=1.0, min_conf=0.4, gt_xy=xy)[0]
    assert empty["counts"] == [0, 0, 0, 0] and bool(torch.isnan(empty["conf"]).all()) and bool(torch.isinf(empty["col_lse"]).all())
    assert bool((empty["col_lse"] < 0).all()) and bool((empty["idx"] == -1).all())
    # a single selected row: its column sum is its own term, conf = exp(s - row_lse)
    one = ref.restate(pc, img, torch.tensor([[0, 0, 0, 1]]), temperature=1.0)[0]
    assert math.isclose(float(one["conf"][3]), 1.0 / (1 + 3 * a), rel_tol=1e-12)


@pytest.mark.parametrize("N", [4097, 16384])
def test_confidence_threshold_on_planted_scenes(N):
    """match_filter_reference.planted_scene(1, N, 40, 128, seed=N), T = 0.1, conf >= 0.1, against the hard filters of DESIGN.md 4m as
    their own float64 restatement computes them.  Measured (kept / kept inliers / kept inlier ratio):
                              N = 4 097              N = 16 384
      none                    1 632 / 827 / 0.507    6 607 / 3 363 / 0.509
      mutual + ratio 0.9 r2     767 / 764 / 0.996    2 424 / 2 424 / 1.000
      ratio 0.9 r2              838 / 824 / 0.983    3 404 / 3 346 / 0.983
      conf >= 0.1               824 / 820 / 0.995    3 251 / 3 251 / 1.000"""
    s = fref.planted_scene(1, N, 40, 128, seed=N)
    c = ref.restate(s["pc"], s["img"], s["mask"], temperature=0.1, min_conf=0.1, gt_xy=s["gt_xy"])[0]["counts"]
    both = fref.restate(s["pc"], s["img"], s["mask"], mutual=True, ratio=0.9, excl_radius=2, gt_xy=s["gt_xy"])[0]["counts"]
    ratio = fref.restate(s["pc"], s["img"], s["mask"], mutual=False, ratio=0.9, excl_radius=2, gt_xy=s["gt_xy"])[0]["counts"]
    print(N, "conf", c, "mutual + ratio", both, "ratio", ratio)
    assert c[0] == both[0] == ratio[0] and c[3] == both[3]
    assert c[2] >= both[2]
    assert c[2] / c[1] >= ratio[2] / ratio[1]
    assert c[2] / c[1] >= 0.99


@pytest.mark.parametrize("name,maker,skw,ckw", ref.SCENES, ids=[s[0] for s in ref.SCENES])
def test_gpu_scenes_keep_the_near_row_cap(name, maker, skw, ckw):
    """The scenes of tests/test_match_conf_gpu.py::test_against_float64: per sample, the rows whose forward gap is under 1e-5 or whose
    |log conf - log min_conf| is within the bound on log conf are at most 1 % of the selected rows -- asserted here on the restatement
    alone, so the GPU comparison cannot hide behind its exclusions."""
    s = maker(**skw)
    hw = s["img"].shape[1] * s["img"].shape[2]
    for b, r in enumerate(ref.restate(s["pc"], s["img"], s["mask"], gt_xy=s["gt_xy"], **ckw)):
        near, n = int(r["near"].sum()), r["counts"][0]
        print(name, b, "selected", n, "kept", r["counts"][1], "near", near, "bound %.3g" % ref.bound(r["E"], hw, n)[0])
        assert n > 0 and near <= ref.CAP * n, (name, b, near, n)
        assert 0 < r["counts"][1] < n                                   # the threshold decides something on every scene


def _args(B=2, N=100, h=4, w=6):
    return torch.zeros(B * N, 64), torch.zeros(B, h, w, 64), torch.ones(B, N, dtype=torch.bool)


@pytest.mark.parametrize("bad,match", [
    (lambda p, i, m: (p.view(2, 100, 64), i, m), "2-D"),
    (lambda p, i, m: (p, i[0], m), "4-D"),
    (lambda p, i, m: (p[:, :32], i, m), "width must be 64"),
    (lambda p, i, m: (p, i[..., :32], m), "width must be 64"),
    (lambda p, i, m: (p.double(), i, m), "float32"),
    (lambda p, i, m: (p, i.half(), m), "float32"),
    (lambda p, i, m: (p[:-1], i, m), "do not split"),
    (lambda p, i, m: (p, i, m.float()), "mask"),
    (lambda p, i, m: (p, i, m[:, :-1]), "mask"),
])
def test_argument_checks(bad, match):
    with pytest.raises(ValueError, match=match) as e:
        ops.match_conf(*bad(*_args()))
    assert str(e.value).startswith("match_conf:")


@pytest.mark.parametrize("kw,match", [
    (dict(temperature=0.0), "temperature"), (dict(temperature=-0.1), "temperature"), (dict(temperature=float("inf")), "temperature"),
    (dict(temperature=float("nan")), "temperature"), (dict(min_conf=-0.1), "min_conf"), (dict(min_conf=1.5), "min_conf"),
    (dict(min_conf=float("nan")), "min_conf"), (dict(gt_xy=torch.zeros(2, 2, 99)), "gt_xy"), (dict(gt_xy=torch.zeros(2, 2, 100).double()), "gt_xy"),
])
def test_scalar_argument_checks(kw, match):
    with pytest.raises(ValueError, match=match) as e:
        ops.match_conf(*_args(), **kw)
    assert str(e.value).startswith("match_conf:")


def test_map_over_the_limit_is_refused():
    big = torch.zeros(1).expand(1, 4097, 4096, 64)                    # 2^24 + 4096 pixels, no memory behind it
    with pytest.raises(ValueError, match="2\\^24"):
        ops.match_conf(torch.zeros(4, 64), big, torch.ones(1, 4, dtype=torch.bool))


def test_cpu_tensors_are_refused_before_any_launch():
    with pytest.raises(ValueError, match="GPU"):                       # everything right but the device
        ops.match_conf(*_args())
    with pytest.raises(ValueError, match="GPU"):
        ops.match_conf(*_args(), temperature=0.05, min_conf=0.2, gt_xy=torch.zeros(2, 2, 100), want_dist=True, want_lse=True)


def test_signatures_and_model_keywords():
    sig = inspect.signature(ops.match_conf)
    want = dict(temperature=0.1, min_conf=0.0, gt_xy=None, thr=3.0, want_dist=False, want_lse=False)
    assert list(sig.parameters) == ["pc_feat_rows", "img_feat_nhwc", "mask"] + list(want)
    assert {k: v.default for k, v in sig.parameters.items() if k in want} == want
    from cmr_agent_amd.models import MultiHeadModel
    from cmr_agent_amd.models.MultiHeadModel import match_features_conf
    sig = inspect.signature(match_features_conf)
    assert list(sig.parameters) == ["data_batch", "mask", "temperature", "min_conf"]
    assert sig.parameters["temperature"].default == 0.1 and sig.parameters["min_conf"].default == 0.0
    sig = inspect.signature(MultiHeadModel.pose_from_matches)
    want = dict(mutual=False, ratio=None, excl_radius=2, max_dist=None, subpixel=False, min_conf=None, temperature=0.1)
    assert {k: v.default for k, v in sig.parameters.items() if k in want} == want


@pytest.mark.parametrize("other", [dict(mutual=True), dict(ratio=0.9), dict(max_dist=0.8)])
def test_pose_from_matches_takes_one_filter_or_the_other(other):
    from cmr_agent_amd.models import MultiHeadModel
    with pytest.raises(ValueError, match="min_conf"):                  # refused before the batch is looked at
        MultiHeadModel.pose_from_matches(None, {}, min_conf=0.1, **other)


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "cmr_hip.h")).read()
    assert re.search(r"\bint\s+cmr_match_conf_f32\s*\(", text)
    assert re.search(r"\bint64_t\s+cmr_match_conf_workspace_bytes\s*\(", text)
    from cmr_agent_amd import _lib
    from cmr_agent_amd.utils import workmodel
    protos = _lib.parse_header()
    assert protos["cmr_match_conf_f32"][2] == ["pc_feat", "img_feat", "C", "B", "N", "h", "w", "mask", "mask_bytes", "temperature",
                                               "min_conf", "gt_xy", "thr", "idx", "conf", "keep", "counts", "d1", "row_lse", "col_lse",
                                               "workspace", "workspace_bytes", "stream"]
    assert len(protos["cmr_match_conf_workspace_bytes"][1]) == 4
    assert len(protos["cmr_feat_match_filter_f32"][1]) == 24 and len(protos["cmr_feat_match_f32"][1]) == 18     # untouched
    assert "cmr_match_conf_f32" in open(workmodel.__file__).read()


def test_entry_point_refuses_bad_arguments():
    """The argument checks come before the first HIP call, so one wrong argument at a time is refused without a GPU (CMR_EINVAL = -1;
    a feature width other than 64 is CMR_EUNSUPPORTED = -3); the pointers are host addresses that are never dereferenced."""
    import ctypes
    from cmr_agent_amd import _lib
    lib = _lib.load()
    B, N, h, w = 2, 100, 4, 6
    need = lib.cmr_match_conf_workspace_bytes(B, N, h, w)
    assert need > 0 and need % 16 == 0
    assert lib.cmr_match_conf_workspace_bytes(0, N, h, w) == 0
    assert lib.cmr_match_conf_workspace_bytes(B, N, h, 2 * w) > need and lib.cmr_match_conf_workspace_bytes(B, 2 * N, h, w) > need
    raw = ctypes.create_string_buffer(4096 + 16)
    a = (ctypes.addressof(raw) + 15) & ~15                              # a 16-byte aligned address
    good = dict(pc=a, img=a, C=64, B=B, N=N, h=h, w=w, mask=a, mask_bytes=1, T=0.1, min_conf=0.1, gt=None, thr=3.0, idx=a, conf=a, keep=a,
                counts=a, d1=None, row_lse=None, col_lse=None, ws=a, ws_bytes=need, stream=None)
    for change in (dict(C=32), dict(C=128)):
        assert lib.cmr_match_conf_f32(*dict(good, **change).values()) == -3, change
    for change in (dict(T=0.0), dict(T=-0.1), dict(T=float("inf")), dict(T=float("nan")), dict(min_conf=1.5), dict(min_conf=-0.1),
                   dict(min_conf=float("nan")), dict(mask_bytes=4), dict(mask_bytes=0), dict(pc=a + 4), dict(img=a + 8), dict(ws=a + 4),
                   dict(ws_bytes=need - 1), dict(ws=None), dict(idx=None), dict(conf=None), dict(keep=None), dict(counts=None),
                   dict(mask=None), dict(B=0), dict(N=0), dict(h=0), dict(B=65536), dict(h=4097, w=4097)):
        assert lib.cmr_match_conf_f32(*dict(good, **change).values()) == -1, change
