"""CPU tier of the match filter: the float64 restatement in match_filter_reference.py does on planted scenes what the
filters are for (so the yardstick of the GPU tests is itself checked), the scenes of the GPU tier keep the share of ambiguous rows under
the cap, ops.feat_match_filter refuses malformed arguments before any launch, and the header declares the entry points."""
import inspect
import math
import os
import re

import pytest
import torch

import match_filter_reference as ref
from cmr_agent_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FILTERS = {"none": dict(mutual=False), "mutual": dict(mutual=True), "ratio": dict(mutual=False, ratio=0.9, excl_radius=2),
           "both": dict(mutual=True, ratio=0.9, excl_radius=2)}


def _run(scene, **kw):
    return ref.restate(scene["pc"], scene["img"], scene["mask"], gt_xy=scene["gt_xy"], **kw)


@pytest.mark.parametrize("N,seed", [(4097, 4097), (16384, 16384)])
def test_filters_lift_the_inlier_ratio_on_planted_scenes(N, seed):
    """40 x 128 map, 50 % of the points replaced by random unit vectors, ~40 % selected.  Measured with this generator and these seeds
    (kept of selected, kept inlier ratio):
                       N = 4 097 (1 632 selected)      N = 16 384 (6 607 selected)
      none             1 632   0.507                   6 607   0.509
      mutual             817   0.935   (50 %)          2 426   0.999   (37 %)
      ratio 0.9, r 2     838   0.983   (51 %)          3 404   0.983   (52 %)
      both               767   0.996   (47 %)          2 424   1.000   (37 %)
    The bars (each filter alone >= 0.9, both together keep >= 25 % of the selected rows) sit well inside these."""
    s = ref.planted_scene(1, N, 40, 128, seed=seed)
    got = {}
    for name, kw in FILTERS.items():
        c = _run(s, **kw)[0]["counts"]
        got[name] = (c[1], c[2] / c[1], c[1] / c[0])
        print(N, name, c, "inlier ratio %.4f kept share %.3f" % got[name][1:])
    assert 0.4 <= got["none"][1] <= 0.6 and got["none"][2] == 1.0
    assert got["mutual"][1] >= 0.9 and got["ratio"][1] >= 0.9 and got["both"][1] >= 0.9
    assert got["both"][2] >= 0.25
    assert got["both"][0] <= min(got["mutual"][0], got["ratio"][0])


def test_restatement_on_a_hand_made_scene():
    """2 x 3 map, 4 points, everything checkable by eye: e_k = k-th unit vector of R^64, pixel p has feature e_p; point 0 = e_4, point 1 and
    point 3 = e_1 (duplicates), point 2 unselected."""
    e = torch.eye(64)
    img = e[:6].reshape(1, 2, 3, 64).contiguous()
    pc = torch.stack([e[4], e[1], e[0], e[1]])
    mask = torch.tensor([[1, 1, 0, 1]])
    xy = torch.tensor([[[1.0, 1.0, 0.0, math.nan], [1.0, 0.0, 0.0, 0.0]]])
    r = ref.restate(pc, img, mask, mutual=True, ratio=0.5, excl_radius=0, gt_xy=xy, thr=0.5)[0]
    assert r["idx"].tolist() == [4, 1, -1, 1]
    assert r["rev"].tolist() == [0, 1, 0, 0, 0, 0]                   # pixel 1: rows 1 and 3 tie at 0, the lower wins; pixel 4: row 0;
    #                                                                  every other pixel is sqrt(2) from all three rows: row 0
    assert r["keep"].tolist() == [True, True, False, False]           # row 3 loses pixel 1 to its duplicate, row 1
    assert r["counts"] == [3, 2, 2, 2]                                # row 3's ground truth is not finite
    assert torch.allclose(r["fwd_gap"], torch.full((3,), math.sqrt(2.0), dtype=torch.float64))
    assert torch.allclose(r["rev_gap"], torch.tensor([math.sqrt(2.0), 0.0, 0.0], dtype=torch.float64))
    assert r["near"].tolist() == [False, True, True]
    assert torch.allclose(r["d1"][[0, 1, 3]], torch.zeros(3, dtype=torch.float64))
    assert torch.allclose(r["d2"][[0, 1, 3]], torch.full((3,), math.sqrt(2.0), dtype=torch.float64))
    assert torch.isnan(r["d1"][2]) and torch.isnan(r["d2"][2])


def test_window_covers_the_map_and_plain_second_nearest():
    s = ref.random_scene(1, 50, 5, 7, seed=3, select=1.0)
    r = ref.restate(s["pc"], s["img"], s["mask"], mutual=False, ratio=0.9, excl_radius=7)[0]
    assert bool(torch.isinf(r["d2"]).all()) and bool(r["keep"].all()) and bool(torch.isinf(r["ratio_gap"]).all())
    r = ref.restate(s["pc"], s["img"], s["mask"], mutual=False, ratio=0.9, excl_radius=0)[0]
    d = torch.cdist(s["pc"].double(), s["img"].reshape(35, 64).double())
    two = d.topk(2, dim=1, largest=False).values
    assert torch.allclose(r["d1"], two[:, 0], atol=1e-9) and torch.allclose(r["d2"], two[:, 1], atol=1e-9)
    assert torch.allclose(r["fwd_gap"], two[:, 1] - two[:, 0], atol=1e-9)
    dr = d.topk(2, dim=0, largest=False).values
    assert torch.allclose(r["rev_gap"], (dr[1] - dr[0])[r["idx"]], atol=1e-9)
    assert torch.equal(r["rev"], d.argmin(0))
    empty = ref.restate(s["pc"], s["img"], torch.zeros(1, 50, dtype=torch.int64), gt_xy=s["gt_xy"])[0]
    assert empty["counts"] == [0, 0, 0, 0] and bool((empty["rev"] == -1).all()) and bool((empty["idx"] == -1).all())


@pytest.mark.parametrize("name,maker,skw,fkw", ref.SCENES, ids=[s[0] for s in ref.SCENES])
def test_gpu_scenes_keep_the_ambiguity_cap(name, maker, skw, fkw):
    """The scenes of tests/test_match_filter_gpu.py::test_against_float64: per sample, the rows with a float64 margin under 1e-5 are at
    most 0.5 % of the selected rows -- asserted here on the restatement alone, so the GPU comparison cannot hide behind its exclusions."""
    s = maker(**skw)
    for b, r in enumerate(_run(s, **fkw)):
        near, n = int(r["near"].sum()), r["counts"][0]
        print(name, b, "selected", n, "kept", r["counts"][1], "under 1e-5:", near)
        assert n > 0 and near <= ref.CAP * n, (name, b, near, n)
        assert 0 < r["counts"][1] < n                                   # the filter decides something on every scene


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
    with pytest.raises(ValueError, match=match):
        ops.feat_match_filter(*bad(*_args()))


@pytest.mark.parametrize("kw,match", [
    (dict(excl_radius=-1), "excl_radius"), (dict(excl_radius=1.5), "excl_radius"), (dict(ratio=-0.1), "ratio"), (dict(ratio=1.5), "ratio"),
    (dict(ratio=float("nan")), "ratio"), (dict(max_dist=-1.0), "max_dist"), (dict(max_dist=float("inf")), "max_dist"),
    (dict(max_dist=float("nan")), "max_dist"), (dict(gt_xy=torch.zeros(2, 2, 99)), "gt_xy"), (dict(gt_xy=torch.zeros(2, 2, 100).double()), "gt_xy"),
])
def test_scalar_argument_checks(kw, match):
    with pytest.raises(ValueError, match=match):
        ops.feat_match_filter(*_args(), **kw)


def test_cpu_tensors_are_refused_before_any_launch():
    with pytest.raises(ValueError, match="GPU"):                   # everything right but the device
        ops.feat_match_filter(*_args())


def test_signature_and_model_keywords():
    sig = inspect.signature(ops.feat_match_filter)
    want = dict(mutual=True, ratio=0.0, excl_radius=2, max_dist=0.0, gt_xy=None, thr=3.0, want_dist=False, want_rev=False)
    assert list(sig.parameters)[:3] == ["pc_feat_rows", "img_feat_nhwc", "mask"]
    assert {k: v.default for k, v in sig.parameters.items() if k in want} == want
    from cmr_agent_amd.models import MultiHeadModel
    sig = inspect.signature(MultiHeadModel.pose_from_matches)
    want = dict(mutual=False, ratio=None, excl_radius=2, max_dist=None)
    assert {k: v.default for k, v in sig.parameters.items() if k in want} == want


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "cmr_hip.h")).read()
    assert re.search(r"\bint\s+cmr_feat_match_filter_f32\s*\(", text)
    assert re.search(r"\bint64_t\s+cmr_feat_match_filter_workspace_bytes\s*\(", text)
    from cmr_agent_amd import _lib
    protos = _lib.parse_header()
    assert len(protos["cmr_feat_match_filter_f32"][1]) == 24
    assert len(protos["cmr_feat_match_filter_workspace_bytes"][1]) == 4
    assert len(protos["cmr_feat_match_f32"][1]) == 18              # the matcher's entry point is untouched


def test_entry_point_refuses_bad_arguments():
    """CMR_REQUIRE comes before the first HIP call, so one wrong argument at a time is refused (CMR_EINVAL = -1) without a GPU; the
    pointers are host addresses that are never dereferenced."""
    import ctypes
    from cmr_agent_amd import _lib
    lib = _lib.load()
    B, N, h, w = 2, 100, 4, 6
    need = lib.cmr_feat_match_filter_workspace_bytes(B, N, h, w)
    assert need > 0 and need % 16 == 0
    assert lib.cmr_feat_match_filter_workspace_bytes(0, N, h, w) == 0
    assert lib.cmr_feat_match_filter_workspace_bytes(B, N, h, 2 * w) > need      # the reverse direction's buffers grow with the map
    raw = ctypes.create_string_buffer(4096 + 16)
    a = (ctypes.addressof(raw) + 15) & ~15                              # a 16-byte aligned address
    good = dict(pc=a, img=a, C=64, B=B, N=N, h=h, w=w, mask=a, mask_bytes=1, mutual=1, ratio=0.9, excl=2, max_dist=0.0, gt=None, thr=3.0,
                idx=a, keep=a, counts=a, d1=None, d2=None, rev=None, ws=a, ws_bytes=need, stream=None)
    for change in (dict(C=32), dict(mask_bytes=4), dict(mask_bytes=0), dict(excl=-1), dict(pc=a + 4), dict(img=a + 8), dict(ws=a + 4),
                   dict(ws_bytes=need - 1), dict(ws=None), dict(idx=None), dict(keep=None), dict(counts=None), dict(mask=None), dict(B=0),
                   dict(N=0), dict(h=0), dict(B=65536), dict(ratio=float("nan")), dict(max_dist=float("nan"))):
        args = dict(good, **change)
        assert lib.cmr_feat_match_filter_f32(*args.values()) == -1, change
