"""GPU tier of the sub-pixel match positions (ops.match_subpixel / cmr_match_subpixel_f32, MultiHeadModel.pose_from_matches and
refine_pose_from_matches with subpixel=True, Test_Geo.py / Test_Agent.py --subpixel).

The yardstick is the float64 restatement in subpixel_reference.py, handed the DEVICE's idx, so a near-tie in the matcher is not a
disagreement here.  The bound on delta is derived: every squared distance is a sum of 64 non-negative fp32 terms, so its absolute error is
at most E = 66 * 2^-24 * max(s0, sm, sp); num combines two of them (error <= 2 E), den four (<= 4 E) and |delta| <= 0.5, so
|delta_device - delta_float64| <= 0.5 * 2 E / den + 0.5 * 4 E / den = 3 E / |den|.  (delta_device is read back as uv - x, which adds the
rounding of that one fp32 addition, <= 2^-18 px for x < 128; the sums' own error is far under its worst case, so the bound is kept as
derived.)  Rows whose float64 fit hangs on |den| < 1e-3 or whose error lies within 1e-4 px of thr (`near`; tests/test_subpixel_cpu.py caps
them at 1 % of a sample's matched rows) may resolve either way, nothing else may."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guided_reference as gref
import pnp_reference as pref
import subpixel_reference as sref
from cmr_agent_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- analytic map ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(8, 12), (40, 128)])
def test_analytic_map_returns_the_planted_position(h, w):
    """img[y][x] = (x, y, 0, ...), point feature (u, v, 0, ...): uv = (u, v) within 3 E / den, E = 66 * 2^-24 * max(s0, sm, sp), den = 2
    (about 3e-5 px); on a border axis uv is the integer coordinate."""
    pc, img, idx, u, v, _ = sref.analytic_case(h, w, seed=5)
    uv, counts = ops.match_subpixel(pc.to(DEV), img.to(DEV), idx.int().to(DEV))
    uv = uv[0].double().cpu()
    x, y = (idx % w).double(), (idx // w).double()
    worst = 0.0
    for ax, (c, size, t) in enumerate(((x, w, u), (y, h, v))):
        t = torch.from_numpy(t)
        inner = (c >= 1) & (c <= size - 2)
        smax = (c - t).abs() + 1.0                                             # the farther neighbour lies |c - t| + 1 away on this axis
        other = (y - torch.from_numpy(v)) if ax == 0 else (x - torch.from_numpy(u))
        bound = 3 * sref.EPS_S * (smax ** 2 + other ** 2) / 2.0
        err = (uv[ax] - t).abs()
        worst = max(worst, float((err[inner] / bound[inner]).max()))
        assert bool((err[inner] <= bound[inner]).all()), float(err[inner].max())
        assert torch.equal(uv[ax][~inner], c[~inner])
    print("analytic", h, w, "max error / bound", worst)
    assert counts.tolist() == [[h * w, (h - 2) * (w - 2), 0, 0]]


@pytest.mark.parametrize("off", [(1, 0), (-1, 0), (0, 1), (0, -1)])
def test_an_index_one_pixel_off_clamps_to_half_a_pixel(off):
    h, w = 8, 12
    pc, img, idx, u, v, moved = sref.analytic_case(h, w, seed=6, off=off)
    uv, _ = ops.match_subpixel(pc.to(DEV), img.to(DEV), idx.int().to(DEV))
    ref = sref.match_subpixel(pc, img, idx)[0]
    ax = 0 if off[0] else 1
    rows = moved & ref["fitted"][ax]
    assert int(rows.sum()) > 20
    assert torch.equal(uv[0, ax].cpu().double()[rows], ref["uv"][ax][rows])                  # x -+ 0.5 exactly


# ---- against the restatement ---------------------------------------------------------------------------------------------------------------
def _device_idx(sc, source):
    pc, img = sc["pc"].to(DEV), sc["img"].to(DEV)
    if source == "global":
        return ops.feat_match(pc, img, sc["mask"].to(DEV))[0]
    return ops.guided_match(F(sc["pts"]), pc, img, sc["mask"].to(DEV), F(sc["start"]), F(sc["K"]), sref.GUIDED_RADIUS)[0]


def _compare(pc, img, idx, uv, counts, mask=None, gt_xy=None, thr=0.5):
    """Device uv / counts against the restatement on the same idx -> the restatement's per-sample dicts."""
    B, h, w, _ = img.shape
    N = pc.shape[0] // B
    ref = sref.match_subpixel(pc, img, idx, mask=mask, gt_xy=gt_xy, thr=thr)
    uv, counts, idx = uv.double().cpu(), counts.cpu().tolist(), idx.view(B, N).cpu().long()
    for b in range(B):
        e = ref[b]
        near, m = e["near"], e["matched"]
        n_near = int(near.sum())
        assert n_near <= sref.CAP * e["counts"][0]                                       # the excluded set stays under the cap on the device's idx too
        assert torch.equal(torch.isnan(uv[b, 0]), ~m) and torch.equal(torch.isnan(uv[b, 1]), ~m)        # the NaN pattern, every row
        p = idx[b].clamp(min=0)
        cell = torch.stack([p % w, torch.div(p, w, rounding_mode="floor")]).double()
        worst = worst_abs = 0.0
        for ax in range(2):
            d = uv[b, ax] - cell[ax]                                                     # delta as the device added it
            assert bool((d[m].abs() <= 0.5).all())
            assert not bool((d[m & ~e["in_map"][ax]] != 0).any())                        # off the map: the integer coordinate, near or not
            rows = m & ~near & e["in_map"][ax]
            assert not bool((d[rows & ~e["fitted"][ax]] != 0).any())                     # the fitted flag: unfitted in float64 = no shift here ...
            bound = 3 * sref.EPS_S * e["smax"][ax] / e["den"][ax].abs()
            err = (d - e["delta"][ax]).abs()
            if bool(rows.any()):                                                         # ... and fitted in float64 = the float64 shift within the bound
                worst, worst_abs = max(worst, float((err[rows] / bound[rows]).max())), max(worst_abs, float(err[rows].max()))
                assert bool((err[rows] <= bound[rows]).all()), (float(err[rows].max()), float((err[rows] / bound[rows]).max()))
        print("   sample", b, "counts", counts[b], "restatement", e["counts"], "near", n_near, "max |delta - float64|", worst_abs,
              "px, of its bound", worst)
        assert counts[b][0] == e["counts"][0]
        for k in (1, 2, 3):
            assert abs(counts[b][k] - e["counts"][k]) <= n_near, (k, counts[b], e["counts"])
    return ref


@pytest.mark.parametrize("source", ["global", "guided"])
@pytest.mark.parametrize("name", [n for n, _ in sref.GPU_SCENES])
def test_match_subpixel_against_float64(name, source):
    sc = sref.gpu_scene(name)
    idx = _device_idx(sc, source)
    uv, counts = ops.match_subpixel(sc["pc"].to(DEV), sc["img"].to(DEV), idx, gt_xy=sc["gt_xy"].to(DEV), thr=0.5)
    print(name, source)
    _compare(sc["pc"], sc["img"], idx, uv, counts, gt_xy=sc["gt_xy"])


def test_masked_rows_and_absent_ground_truth_against_float64():
    sc = sref.gpu_scene("tiny_202")
    B, _, N = sc["pts"].shape
    idx = _device_idx(sc, "guided")
    mask = torch.rand(B, N, generator=torch.Generator().manual_seed(3)) < 0.6
    mask[1] = False                                                                      # an all-unmatched sample
    uv, counts = ops.match_subpixel(sc["pc"].to(DEV), sc["img"].to(DEV), idx, mask=mask.to(DEV))
    _compare(sc["pc"], sc["img"], idx, uv, counts, mask=mask)
    assert counts[1].tolist() == [0, 0, 0, 0] and bool(torch.isnan(uv[1]).all()) and counts[:, 2:].tolist() == [[0, 0]] * B


# ---- borders and degenerate maps -----------------------------------------------------------------------------------------------------------
def _unit(shape, seed):
    return torch.nn.functional.normalize(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)), dim=-1)


@pytest.mark.parametrize("h,w", [(8, 12), (1, 12), (8, 1), (1, 1), (2, 2)])
def test_every_pixel_as_the_match_including_edges_and_corners(h, w):
    """One row per pixel of the map (every edge and corner among them; 1 x w, h x 1 and 1 x 1 maps have no inner pixel on an axis), plus
    rows with idx -1, h*w and 2^31 - 1, for B = 2."""
    B, extra = 2, 3
    N = h * w + extra
    img, pc = _unit((B, h, w, 64), 11), _unit((B * N, 64), 12)
    idx = torch.cat([torch.arange(h * w), torch.tensor([-1, h * w, 2 ** 31 - 1])]).repeat(B).int()
    gt = torch.rand(B, 2, N, generator=torch.Generator().manual_seed(13)) * torch.tensor([w, h]).view(1, 2, 1)
    uv, counts = ops.match_subpixel(pc.to(DEV), img.to(DEV), idx.to(DEV), gt_xy=gt.to(DEV), thr=0.5)
    ref = _compare(pc, img, idx.to(DEV), uv, counts, gt_xy=gt)
    uv = uv.cpu()
    for b in range(B):
        assert bool(torch.isnan(uv[b, :, h * w:]).all()) and bool(torch.isfinite(uv[b, :, :h * w]).all())
        assert counts[b, 0].item() == h * w
        if h < 3 or w < 3:
            assert counts[b, 1].item() == 0
        if h < 3:
            assert torch.equal(uv[b, 1, :h * w], (torch.arange(h * w) // w).float())
        if w < 3:
            assert torch.equal(uv[b, 0, :h * w], (torch.arange(h * w) % w).float())
        if h >= 3 and w >= 3:
            assert ref[b]["counts"][1] > 0 and counts[b, 1].item() > 0


def test_flat_and_non_finite_neighbours_give_no_shift():
    h, w = 5, 6
    img, pc = _unit((1, h, w, 64), 21), _unit((4, 64), 22)
    p = 2 * w + 3
    img[0, 2, 2] = img[0, 2, 4] = img[0, 2, 3]                                 # row 0: den = 0 along x (exactly: the same bits three times)
    idx = torch.tensor([p, p, 3 * w + 1, 1 * w + 4]).int()
    uv, counts = ops.match_subpixel(pc.to(DEV), img.to(DEV), idx.to(DEV))
    assert uv[0, 0, :2].tolist() == [3.0, 3.0] and counts.tolist()[0][0] == 4
    bad = img.clone()
    bad[0, 2, 1, 9] = math.nan                                                  # left neighbour of (1, 3)... and lower neighbour of (1, 1)
    bad[0, 1, 4, 0] = math.inf                                                  # the centre of row 3
    uv, counts = ops.match_subpixel(pc.to(DEV), bad.to(DEV), torch.tensor([3 * w + 1, 1 * w + 1, p, 1 * w + 4]).int().to(DEV))
    uv = uv[0].cpu()
    assert bool(torch.isfinite(uv).all())
    assert uv[1, 0].item() == 3.0 and uv[1, 1].item() == 1.0 and uv[:, 3].tolist() == [4.0, 1.0]


# ---- determinism and interfaces --------------------------------------------------------------------------------------------------------------
def _call_args(B=3, N=4096, seed=231):
    sc = gref.scene(B, N, 40, 128, seed)
    idx = _device_idx(sc, "guided")
    mask = (torch.rand(B, N, generator=torch.Generator().manual_seed(6)) < 0.7).to(DEV)
    return sc["pc"].to(DEV), sc["img"].to(DEV), idx, mask, sc["gt_xy"].to(DEV)


def test_two_calls_agree_bit_for_bit_and_mask_dtypes_agree():
    pc, img, idx, mask, gt = _call_args()
    first = ops.match_subpixel(pc, img, idx, mask=mask, gt_xy=gt)
    for m in (mask, mask.to(torch.uint8), mask.long() * 7):
        for x, y in zip(ops.match_subpixel(pc, img, idx, mask=m, gt_xy=gt), first):
            assert torch.equal(_bits(x), _bits(y))
    # an absent mask = a mask of ones
    for x, y in zip(ops.match_subpixel(pc, img, idx, gt_xy=gt), ops.match_subpixel(pc, img, idx, mask=torch.ones_like(mask), gt_xy=gt)):
        assert torch.equal(_bits(x), _bits(y))
    assert first[1][:, 0].tolist() == (mask.view(3, -1) & (idx.view(3, -1) >= 0)).sum(1).tolist()


def test_sample_alone_equals_sample_in_batch():
    pc, img, idx, mask, gt = _call_args()
    B, N = mask.shape
    uv, counts = ops.match_subpixel(pc, img, idx, mask=mask, gt_xy=gt)
    for k in range(B):
        u1, c1 = ops.match_subpixel(pc[k * N:(k + 1) * N].contiguous(), img[k:k + 1].contiguous(), idx[k * N:(k + 1) * N].contiguous(),
                                    mask=mask[k:k + 1].contiguous(), gt_xy=gt[k:k + 1].contiguous())
        assert torch.equal(_bits(u1[0]), _bits(uv[k])) and torch.equal(c1[0], counts[k])


def test_graph_replay_equals_eager():
    pc, img, idx, mask, gt = _call_args(B=2, N=8192, seed=233)
    fn = lambda: ops.match_subpixel(pc, img, idx, mask=mask, gt_xy=gt)
    eager = fn()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        fn()
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = fn()
    for t in got:
        t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, got):
        assert torch.equal(_bits(x), _bits(y))


# ---- model -----------------------------------------------------------------------------------------------------------------------------------
def _model(N):
    from cmr_agent_amd.models import MultiHeadModel
    from cmr_agent_amd.config import KittiConfiguration
    return MultiHeadModel(KittiConfiguration(num_pt=N, device=torch.device(DEV)))


def _data(pts, K, P, pc_rows, img_nhwc):
    B, _, N = pts.shape
    cam = np.einsum("bij,bjn->bin", P[:, :3, :3], pts) + P[:, :3, 3:4]
    return {"pc": F(pts), "K": F(K), "P": F(P), "pc_in_cam_space": F(cam),
            "pc_geo_feat": pc_rows.view(B, N, 64).permute(0, 2, 1).contiguous().to(DEV),
            "img_geo_feat": img_nhwc.permute(0, 3, 1, 2).contiguous().to(DEV), "pc_overlap_pred": torch.ones(B, N, dtype=torch.bool, device=DEV)}, cam


@pytest.mark.parametrize("seed", [201, 202])
def test_refine_pose_from_matches_subpixel_follows_the_restatement(seed):
    """The tolerances of test_guided_gpu.py::test_refine_pose_from_matches_follows_the_restatement (error against the truth at most twice
    the float64 rounds' + 1e-3), on scene_bilinear with sub-pixel correspondences on both sides."""
    B, N, h, w = 2, 4096, 40, 128
    sc = sref.scene_bilinear(B, N, h, w, seed)
    want, _ = sref.refine_rounds(sc)
    wr, wt = gref.pose_errors(want, sc["P"])
    data, _ = _data(sc["pts"], sc["K"], sc["P"], sc["pc"], sc["img"])
    _model(N).refine_pose_from_matches(data, pose=F(sc["start"]), radii=[r for r, _ in gref.ROUNDS], thrs=[t for _, t in gref.ROUNDS],
                                       max_dist=gref.MAX_DIST, subpixel=True)
    assert data["refined_status"].tolist() == [0] * B and data["refined_pose"].shape == (B, 4, 4)
    sc4 = data["guided_subpixel_counts"]
    assert sc4.shape == (len(gref.ROUNDS), B, 4) and sc4.dtype == torch.int32
    assert torch.equal(sc4[:, :, 0], data["guided_counts"][:, :, 2])                       # matched = that round's kept rows
    assert bool((sc4[:, :, 1] <= sc4[:, :, 0]).all()) and bool((sc4[:, :, 3] > sc4[:, :, 2]).all())
    gr, gt = gref.pose_errors(data["refined_pose"].double().cpu().numpy(), sc["P"])
    print("seed", seed, "device", gr, gt, "restatement", wr, wt, "sub-pixel counts", sc4.tolist())
    for b in range(B):
        assert gr[b] <= 2 * wr[b] + 1e-3 and gt[b] <= 2 * wt[b] + 1e-3


def _filter_scene():
    """The scene of test_match_filter_gpu.py::test_pose_from_filtered_matches_end_to_end."""
    B, N, h, w = 2, 4096, 40, 128
    s = pref.planted(B, N, h, w, seed=131)
    pix = (np.round(s["uv"][:, 1]) * w + np.round(s["uv"][:, 0])).astype(np.int64)
    g = torch.Generator(device="cpu").manual_seed(132)
    img = torch.nn.functional.normalize(torch.randn(B, h * w, 64, generator=g, dtype=torch.float64), dim=-1)
    pcf = torch.gather(img, 1, torch.from_numpy(pix)[..., None].expand(B, N, 64)) + 0.08 * torch.randn(B, N, 64, generator=g, dtype=torch.float64)
    outlier = torch.rand(B, N, generator=g) < 0.5
    pcf = torch.where(outlier[..., None], torch.randn(B, N, 64, generator=g, dtype=torch.float64), pcf)
    pcf = torch.nn.functional.normalize(pcf, dim=-1).float()
    data, cam = _data(s["pts"], s["K"], s["P"], pcf.reshape(B * N, 64), img.float().view(B, h, w, 64))
    ov = torch.ones(B, h, w, dtype=torch.bool, device=DEV)
    ov[:, :, : w // 8] = False
    return s, data, cam, ov


def test_pose_from_matches_subpixel_sets_its_keys_and_recovers_the_pose():
    """That test's bars (rotation <= q / f, translation <= q z_max / f, q = 0.5 sqrt(2) px) with the filters on and sub-pixel uv."""
    s, data, cam, ov = _filter_scene()
    B, N = 2, 4096
    model = _model(N)
    model.pose_from_matches(data, img_overlap=ov, n_hyp=16, mutual=True, ratio=0.9, subpixel=True)
    assert data["pnp_status"].tolist() == [0] * B
    c = data["pnp_subpixel_counts"]
    assert c.shape == (B, 4) and c.dtype == torch.int32 and torch.equal(c[:, 0].long(), data["pnp_used"].long())
    assert bool((c[:, 1] <= c[:, 0]).all()) and bool((c[:, 1] > 0).all())
    q, foc = 0.5 * math.sqrt(2.0), s["K"][0][0, 0]
    rre, rte = gref.pose_errors(data["pnp_pose"].double().cpu().numpy(), s["P"])
    print("sub-pixel: RRE", rre, "RTE", rte, "counts", c.tolist())
    assert max(rre) <= math.degrees(q / foc) and max(rte) <= q * cam[:, 2].max() / foc


def test_subpixel_false_is_the_call_without_the_argument():
    s, data, cam, ov = _filter_scene()
    model = _model(4096)
    keys = ("pnp_pose", "pnp_inliers", "pnp_status", "refined_pose", "refined_inliers", "refined_status", "guided_counts")
    outs = []
    for kw in (dict(), dict(subpixel=False)):
        d = dict(data)
        model.pose_from_matches(d, img_overlap=ov, n_hyp=16, **kw)
        model.refine_pose_from_matches(d, img_overlap=ov, **kw)
        assert "pnp_subpixel_counts" not in d and "guided_subpixel_counts" not in d
        outs.append((d, set(d)))
    assert outs[0][1] == outs[1][1]
    for k in keys:
        assert torch.equal(_bits(outs[0][0][k]), _bits(outs[1][0][k])), k
    d = dict(data)
    model.pose_from_matches(d, img_overlap=ov, n_hyp=16, subpixel=True)
    model.refine_pose_from_matches(d, img_overlap=ov, subpixel=True)
    assert set(d) == outs[0][1] | {"pnp_subpixel_counts", "guided_subpixel_counts"}
    assert not torch.equal(_bits(d["refined_pose"]), _bits(outs[0][0]["refined_pose"]))


# ---- the scripts -------------------------------------------------------------------------------------------------------------------------------
def _run(script, *flags):
    cmd = [sys.executable, os.path.join(ROOT, script), "--pairs", "1", "--num-pt", "1024", "--img", "96x160", *flags]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return res.stdout.strip().splitlines()


def _shape(line):
    """A line with its numbers blanked: the words and the number of fields."""
    out = []
    for tok in line.split():
        try:
            float(tok)
            out.append("#")
        except ValueError:
            out.append(tok)
    return " ".join(out)


def test_test_geo_script_subpixel():
    lines = _run("Test_Geo.py", "--pnp", "--subpixel")
    plain = _run("Test_Geo.py", "--pnp")
    sub = [i for i, l in enumerate(lines) if l.startswith("subpixel fitted ")]
    assert len(sub) == 1 and not any(l.startswith("subpixel") for l in plain)
    tok = lines[sub[0]].split()
    assert len(tok) == 9 and tok[3] == "of" and tok[5] == "IR@0.5" and tok[7] == "->" and 0 <= int(tok[2]) <= int(tok[4])
    rest = lines[:sub[0]] + lines[sub[0] + 1:]
    assert rest[:sub[0]] == plain[:sub[0]]                                      # everything printed before the pose: the same numbers
    summary = next(i for i, l in enumerate(plain) if len(l.split()) == 5 and _shape(l) == "# # # # #")
    assert rest[summary] == plain[summary]
    assert len(rest) >= sub[0] + 2 and [_shape(l) for l in rest[:summary + 2]] == [_shape(l) for l in plain[:summary + 2]]


def test_test_agent_script_subpixel():
    lines = _run("Test_Agent.py", "--refine", "2", "--subpixel")
    plain = _run("Test_Agent.py", "--refine", "2")
    assert not any(l.startswith("subpixel") for l in lines + plain)
    assert lines[0] == plain[0] and lines[1].startswith("refined ") and plain[1].startswith("refined ")
    rec = [i for i, l in enumerate(plain) if "Registration Recall:" in l]
    assert [_shape(l) for l in lines[:rec[0] + 1]] == [_shape(l) for l in plain[:rec[0] + 1]]
    assert [i for i, l in enumerate(lines) if "Registration Recall:" in l] and lines[rec[0]] == plain[rec[0]]
