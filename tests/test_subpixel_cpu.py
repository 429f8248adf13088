"""CPU tier of the sub-pixel match positions: the float64 restatement in subpixel_reference.py returns the analytic truth
on a map whose distances are exact parabolas and keeps every rule of the contract (borders, den <= 0, NaN neighbours, bad indices,
masks, counts); on planted scenes with bilinearly sampled point features it cuts the localisation error of a match by at least 1.5 x;
the scenes of the GPU tier keep the cap on the rows its comparison leaves out; the guided rounds still converge in float64 with sub-pixel
correspondences; ops.match_subpixel refuses malformed arguments before any launch; the header declares the entry point."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import guided_reference as gref
import subpixel_reference as sref
from cmr_agent_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- analytic truth --------------------------------------------------------------------------------------------------------------------
def test_restatement_returns_the_analytic_vertex():
    """img[y][x] = (x, y, 0, ...), point feature (u, v, 0, ...): s = (x - u)^2 + (y - v)^2 exactly, num = 4 (u - x), den = 2."""
    h, w = 7, 9
    pc, img, idx, u, v, _ = sref.analytic_case(h, w, seed=1)
    r = sref.match_subpixel(pc, img, idx)[0]
    both = r["fitted"][0] & r["fitted"][1]
    x, y = idx % w, idx // w
    assert torch.equal(both, (x >= 1) & (x <= w - 2) & (y >= 1) & (y <= h - 2)) and int(both.sum()) == (h - 2) * (w - 2)
    assert float((r["uv"][0][both] - torch.from_numpy(u)[both]).abs().max()) <= 1e-12
    assert float((r["uv"][1][both] - torch.from_numpy(v)[both]).abs().max()) <= 1e-12
    assert float((r["den"][0][r["in_map"][0]] - 2).abs().max()) <= 1e-12 and r["counts"][:2] == [h * w, (h - 2) * (w - 2)]
    # on a border the other axis is still fitted and exact
    only_x = r["fitted"][0] & ~r["fitted"][1]
    assert int(only_x.sum()) == 2 * (w - 2) and float((r["uv"][0][only_x] - torch.from_numpy(u)[only_x]).abs().max()) <= 1e-12
    assert torch.equal(r["uv"][1][only_x], y[only_x].double())


@pytest.mark.parametrize("off", [(1, 0), (-1, 0), (0, 1), (0, -1)])
def test_an_index_one_pixel_off_clamps_to_half_a_pixel(off):
    """The true vertex lies 0.55 .. 1.45 px from the handed pixel, towards the true one: that axis clamps to -+0.5 exactly."""
    h, w = 7, 9
    pc, img, idx, u, v, moved = sref.analytic_case(h, w, seed=2, off=off)
    r = sref.match_subpixel(pc, img, idx)[0]
    ax = 0 if off[0] else 1
    rows = moved & r["fitted"][ax]
    assert int(rows.sum()) > 20
    assert torch.equal(r["delta"][ax][rows], torch.full((int(rows.sum()),), -0.5 * (off[0] + off[1]), dtype=torch.float64))
    other = moved & r["fitted"][1 - ax]
    want = torch.from_numpy(v if ax == 0 else u)
    assert float((r["uv"][1 - ax][other] - want[other]).abs().max()) <= 1e-12


# ---- rules -----------------------------------------------------------------------------------------------------------------------------
def _unit_map(h, w, seed=3, N=None):
    g = torch.Generator().manual_seed(seed)
    img = torch.nn.functional.normalize(torch.randn(1, h, w, 64, generator=g, dtype=torch.float64), dim=-1)
    pc = torch.nn.functional.normalize(torch.randn(h * w if N is None else N, 64, generator=g, dtype=torch.float64), dim=-1)
    return pc, img


@pytest.mark.parametrize("h,w", [(5, 6), (1, 6), (5, 1), (1, 1), (2, 2), (3, 3)])
def test_border_pixels_are_left_unfitted_on_that_axis(h, w):
    pc, img = _unit_map(h, w)
    idx = torch.arange(h * w)
    r = sref.match_subpixel(pc, img, idx)[0]
    x, y = idx % w, idx // w
    assert torch.equal(r["in_map"][0], (x >= 1) & (x <= w - 2)) and torch.equal(r["in_map"][1], (y >= 1) & (y <= h - 2))
    assert not bool((r["fitted"] & ~r["in_map"]).any())
    assert torch.equal(r["delta"][0][~r["in_map"][0]], torch.zeros(int((~r["in_map"][0]).sum()), dtype=torch.float64))
    assert torch.equal(r["uv"][0][~r["in_map"][0]], x[~r["in_map"][0]].double())
    assert torch.equal(r["uv"][1][~r["in_map"][1]], y[~r["in_map"][1]].double())
    assert bool(r["matched"].all()) and float(r["delta"].abs().max()) <= 0.5
    if h < 3 or w < 3:
        assert r["counts"][1] == 0


def test_flat_and_non_finite_neighbours_give_no_shift():
    h, w = 5, 6
    pc, img = _unit_map(h, w)
    p = 2 * w + 3
    flat = img.clone()
    flat[0, 2, 2] = flat[0, 2, 4] = flat[0, 2, 3]                             # equal neighbours and centre along x: den = 0
    r = sref.match_subpixel(pc[:1], flat, torch.tensor([p]))[0]
    assert float(r["den"][0][0]) == 0.0 and not bool(r["fitted"][0][0]) and float(r["delta"][0][0]) == 0.0 and bool(r["near"][0])
    assert float(r["uv"][0][0]) == 3.0 and bool(r["in_map"][0][0])
    peak = img.clone()
    peak[0, 2, 2] = peak[0, 2, 4] = pc[0]                                       # both neighbours nearer than the centre: den < 0
    r = sref.match_subpixel(pc[:1], peak, torch.tensor([p]))[0]
    assert float(r["den"][0][0]) < 0 and not bool(r["fitted"][0][0]) and float(r["delta"][0][0]) == 0.0
    bad = img.clone()
    bad[0, 1, 3, 7] = math.nan                                                  # the upper neighbour: y is left alone, x is fitted
    r = sref.match_subpixel(pc[:1], bad, torch.tensor([p]))[0]
    assert not bool(r["fitted"][1][0]) and float(r["delta"][1][0]) == 0.0 and float(r["uv"][1][0]) == 2.0
    assert bool(torch.isfinite(r["uv"]).all())
    bad[0, 2, 3, 0] = math.inf                                                  # the centre: neither axis
    r = sref.match_subpixel(pc[:1], bad, torch.tensor([p]))[0]
    assert not bool(r["fitted"].any()) and r["uv"][:, 0].tolist() == [3.0, 2.0]


def test_unmatched_rows_and_counts():
    h, w = 6, 7
    pc, img = _unit_map(h, w, N=6)
    idx = torch.tensor([2 * w + 3, -1, h * w, h * w + 5, 3 * w + 2, 1 * w + 1])
    gt = torch.tensor([[3.2, 0.0, 0.0, 0.0, 2.0, math.nan], [2.1, 0.0, 0.0, 0.0, 9.0, 1.0]])[None].double()
    r = sref.match_subpixel(pc, img, idx, gt_xy=gt, thr=0.5)[0]
    assert r["matched"].tolist() == [True, False, False, False, True, True]
    assert torch.isnan(r["uv"][:, 1:4]).all() and torch.isfinite(r["uv"][:, [0, 4, 5]]).all()
    both = r["matched"] & r["fitted"][0] & r["fitted"][1]
    assert r["counts"] == [3, int(both.sum()), int(r["inl_int"].sum()), int(r["inl_sub"].sum())]
    assert bool(r["inl_int"][0]) and not bool(r["inl_int"][4]) and not bool(r["inl_int"][5]) and not bool(r["inl_sub"][5])   # 0.22 px; 6 px; NaN
    # a masked-off row is unmatched whatever its index; an int64 mask with values other than 1 selects
    m = torch.tensor([0, 1, 1, 1, 7, 1])
    r = sref.match_subpixel(pc, img, idx, mask=m, gt_xy=gt)[0]
    assert r["matched"].tolist() == [False, False, False, False, True, True] and torch.isnan(r["uv"][:, 0]).all() and r["counts"][0] == 2
    # without gt_xy both inlier counts are 0
    r = sref.match_subpixel(pc, img, idx)[0]
    assert r["counts"][0] == 3 and r["counts"][2:] == [0, 0] and torch.isnan(r["err_int"]).all()
    r = sref.match_subpixel(pc, img, idx, mask=torch.zeros(6))[0]
    assert r["counts"] == [0, 0, 0, 0] and torch.isnan(r["uv"]).all()


# ---- gain ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [201, 202])
def test_parabola_fit_cuts_the_localisation_error(seed):
    """Planted 40 x 128 scene, point features sampled bilinearly at the true projection, match = the window minimum of radius 2 round the
    rounded true pixel: over the planted rows at least 2 px inside the map the mean error falls by at least 1.5 x (measured: 1.82 x on
    both seeds, 0.417 -> 0.229 and 0.420 -> 0.231 px) and the share within 0.5 px rises."""
    sc = sref.scene_bilinear(2, 4096, 40, 128, seed)
    for b, (ei, es, si, ss, n) in enumerate(sref.localisation(sc, sref.window_matches(sc, 2))):
        print("seed", seed, "sample", b, "rows", n, "mean error", ei, "->", es, "x", ei / es, "within 0.5 px", si, "->", ss)
        assert n > 2000
        assert es * 1.5 <= ei
        assert ss > si


# ---- cap -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in sref.GPU_SCENES])
def test_gpu_scenes_keep_the_cap_on_near_rows(name):
    """Every scene and idx source of tests/test_subpixel_gpu.py's comparison, in float64 (the device's idx differs on near-ties of the
    matcher only): rows whose fit hangs on |den| < 1e-3 or whose error lies within 1e-4 px of thr are at most 1 % of the matched rows."""
    sc = sref.gpu_scene(name)
    guided = gref.guided_match(sc["pts"], sc["pc"], sc["img"], sc["mask"], sc["start"], sc["K"], sref.GUIDED_RADIUS, gt_xy=sc["gt_xy"])
    sources = {"global": sref.global_match(sc["pc"], sc["img"]), "guided": torch.stack([e["idx"] for e in guided])}
    for src, idx in sources.items():
        for b, r in enumerate(sref.match_subpixel(sc["pc"], sc["img"], idx, gt_xy=sc["gt_xy"], thr=0.5)):
            print(name, src, "sample", b, "counts", r["counts"], "near", int(r["near"].sum()))
            assert r["counts"][0] > 0.5 * idx.shape[1]
            assert int(r["near"].sum()) <= sref.CAP * r["counts"][0]


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [201, 202])
def test_guided_rounds_converge_with_subpixel_correspondences(seed):
    """test_guided_cpu.py::test_guided_rounds_converge_on_planted_scenes' bar -- 20 x closer in rotation and translation, every round's
    refinement accepted -- on scene_bilinear with every round's uv from the parabola fit.  (Not asserted: that it beats the integer path
    at pose level; integer rounding averages out over thousands of matches)"""
    sc = sref.scene_bilinear(2, 4096, 40, 128, seed)
    r0, t0 = gref.pose_errors(sc["start"], sc["P"])
    poses, log = sref.refine_rounds(sc)
    r1, t1 = gref.pose_errors(poses, sc["P"])
    print("seed", seed, "rotation", r0, "->", r1, "translation", t0, "->", t1)
    for b in range(2):
        assert r1[b] * 20 <= r0[b], (r0, r1)
        assert t1[b] * 20 <= t0[b], (t0, t1)
    for row in log:
        for e in row:
            assert e["refine"]["status"] == 0
            assert e["sub"]["counts"][0] == e["match"]["counts"][2] >= e["refine"]["wset"] >= 4       # the fit follows the kept matches


# ---- argument checks -------------------------------------------------------------------------------------------------------------------
def _args(B=2, N=16, h=4, w=6):
    return [torch.zeros(B * N, 64), torch.zeros(B, h, w, 64), torch.zeros(B * N, dtype=torch.int32)]


@pytest.mark.parametrize("pos,bad,match", [
    (0, lambda t: t[0], "2-D"), (1, lambda t: t[0], "4-D"), (0, lambda t: t[:-1], "agree"), (0, lambda t: t[:, :32], "64"),
    (1, lambda t: t[..., :32], "64"), (0, lambda t: t.double(), "float32"), (1, lambda t: t.half(), "float32"),
    (2, lambda t: t.long(), "idx"), (2, lambda t: t[:-1], "idx"), (2, lambda t: t.float(), "idx"),
])
def test_match_subpixel_argument_checks(pos, bad, match):
    a = _args()
    a[pos] = bad(a[pos])
    with pytest.raises(ValueError, match=match) as e:
        ops.match_subpixel(*a)
    assert str(e.value).startswith("match_subpixel:")


@pytest.mark.parametrize("kw,match", [
    (dict(mask=torch.ones(2, 16)), "mask"), (dict(mask=torch.ones(2, 15, dtype=torch.bool)), "mask"),
    (dict(mask=torch.ones(2, 16, dtype=torch.int32)), "mask"), (dict(gt_xy=torch.zeros(2, 2, 15)), "gt_xy"),
    (dict(gt_xy=torch.zeros(2, 2, 16).double()), "gt_xy"), (dict(gt_xy=torch.zeros(2, 16, 2)), "gt_xy"), (dict(thr=0.0), "thr"),
    (dict(thr=-1.0), "thr"), (dict(thr=float("nan")), "thr"), (dict(thr=float("inf")), "thr"),
])
def test_match_subpixel_optional_and_scalar_checks(kw, match):
    with pytest.raises(ValueError, match=match) as e:
        ops.match_subpixel(*_args(), **kw)
    assert str(e.value).startswith("match_subpixel:")


def test_match_subpixel_limits_on_the_map():
    big = torch.zeros(1).expand(1, 4097, 4096, 64)                             # 2^24 + 4096 pixels, no memory behind it
    with pytest.raises(ValueError, match="2\\^24") as e:
        ops.match_subpixel(torch.zeros(4, 64), big, torch.zeros(4, dtype=torch.int32))
    assert str(e.value).startswith("match_subpixel:")


def test_match_subpixel_refuses_cpu_tensors_last():
    for kw in (dict(), dict(mask=torch.ones(2, 16, dtype=torch.bool), gt_xy=torch.zeros(2, 2, 16), thr=0.5)):
        with pytest.raises(ValueError, match="GPU") as e:                       # everything right but the device: refused before the launch
            ops.match_subpixel(*_args(), **kw)
        assert str(e.value).startswith("match_subpixel:")


def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "cmr_hip.h")).read()
    assert re.search(r"\bint\s+cmr_match_subpixel_f32\s*\(", text)
    from cmr_agent_amd import _lib
    protos = _lib.parse_header()
    assert len(protos["cmr_match_subpixel_f32"][1]) == 15
    assert protos["cmr_match_subpixel_f32"][2] == ["pc_feat", "img_feat", "C", "B", "N", "h", "w", "idx", "mask", "mask_bytes", "gt_xy", "thr",
                                                  "uv", "counts", "stream"]
    from cmr_agent_amd.utils import workmodel
    assert "cmr_match_subpixel_f32" in open(workmodel.__file__).read()
    import inspect
    from cmr_agent_amd.models import MultiHeadModel
    for fn in (MultiHeadModel.pose_from_matches, MultiHeadModel.refine_pose_from_matches):
        assert inspect.signature(fn).parameters["subpixel"].default is False


@pytest.mark.parametrize("script,needs", [("Test_Geo.py", "--pnp"), ("Test_Agent.py", "--refine")])
def test_scripts_refuse_subpixel_without_the_flag_it_depends_on(script, needs):
    res = subprocess.run([sys.executable, os.path.join(ROOT, script), "--subpixel"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and needs in res.stderr
    text = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120).stdout
    assert "--subpixel" in text
