"""GPU tier of point visibility and depth rendering (ops.visibility / cmr_visibility_f32, MultiHeadModel.visible_points / render_depth,
refine_pose_from_matches / search_pose with visible=, Test_Geo.py / Test_Agent.py --visible).

Three yardsticks.  (1) A scene done by hand, exact.  (2) A chain of exact equalities against what exists: the op's cells are
ops.guided_match's at radius 0, its depth map is a torch scatter-min of its own depths at its own cells, its flags are the fp32 torch
restatement (max_pool2d, one multiply, one add, one compare) from that map -- all bit for bit.  (3) The float64 restatement
(visibility_reference.py) on the rows and cells it calls decided; tests/test_visibility_cpu.py caps the undecided rows."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guided_reference as gref
import visibility_reference as vr
from cmr_agent_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
INF = math.inf


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == torch.bool else t.contiguous().view(torch.int32) if t.element_size() == 4 else t.contiguous()


def _same(a, b):
    """Two result tuples of ops.visibility, bit for bit (None only against None)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y))


def _call(sc, radius, rel_tol=vr.REL_TOL, abs_tol=vr.ABS_TOL, mask=None, occ_mask="scene", pose=None, sl=slice(None)):
    mask = sc["mask"] if mask is None else mask
    occ = sc.get("occ_mask") if isinstance(occ_mask, str) else occ_mask
    pose = sc["pose"] if pose is None else pose
    return ops.visibility(F(sc["pts"][sl]), F(pose[sl]), F(sc["K"][sl]), sc["h"], sc["w"], mask[sl].contiguous().to(DEV),
                          occ_mask=None if occ is None else occ[sl].contiguous().to(DEV), radius=radius, rel_tol=rel_tol, abs_tol=abs_tol,
                          want_depth_map=True, want_cell=True, want_depth=True)


# ---- 1. the hand scene ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1, 16])
def test_hand_scene(radius):
    pts, pose, K = (t.to(DEV) for t in vr.hand())
    N = pts.shape[2]
    ones = torch.ones(1, N, dtype=torch.bool, device=DEV)
    vis, counts, dmap, cell, depth = ops.visibility(pts, pose, K, vr.HAND_H, vr.HAND_W, ones, radius=radius, rel_tol=vr.HAND_REL_TOL,
                                                    want_depth_map=True, want_cell=True, want_depth=True)
    assert vis.dtype == torch.bool and tuple(vis.shape) == (N,) and counts.dtype == torch.int32 and tuple(counts.shape) == (1, 4)
    assert dmap.dtype == torch.float32 and tuple(dmap.shape) == (1, vr.HAND_H, vr.HAND_W) and cell.dtype == torch.int32 and depth.dtype == torch.float32
    assert vis.int().tolist() == vr.HAND_VISIBLE[radius] and counts[0].tolist() == vr.HAND_COUNTS[radius]
    assert torch.equal(dmap.cpu(), vr.hand_depth_map())
    want_cell = [y * vr.HAND_W + x if (z > 0 and x < vr.HAND_W) else -1 for x, y, z in vr.HAND_ROWS]
    assert cell.tolist() == want_cell
    d = depth.cpu()
    assert math.isnan(d[6]) and [float(v) for i, v in enumerate(d) if i != 6] == [float(np.float32(z)) for i, (_, _, z) in enumerate(vr.HAND_ROWS) if i != 6]
    # the optional outputs are optional, and leaving them out changes nothing
    plain = ops.visibility(pts, pose, K, vr.HAND_H, vr.HAND_W, ones, radius=radius, rel_tol=vr.HAND_REL_TOL)
    assert plain[2] is None and plain[3] is None and plain[4] is None and torch.equal(plain[0], vis) and torch.equal(plain[1], counts)


# ---- 2. exact equalities against what exists --------------------------------------------------------------------------------------------------
def _restated(sc, out, radius, rel_tol, abs_tol):
    """The contract in fp32 torch from the op's own cell / depth: -> (depth map, visible, counts)."""
    _, _, _, cell, depth = out
    B, _, N = sc["pts"].shape
    h, w = sc["h"], sc["w"]
    sel = sc["mask"].to(DEV).view(B, N)
    occ = torch.ones_like(sel) if sc.get("occ_mask") is None else sc["occ_mask"].to(DEV).view(B, N)
    cell, depth = cell.view(B, N), depth.view(B, N)
    view = cell >= 0
    inf = torch.full_like(depth, INF)
    Z = torch.full((B, h * w), INF, device=DEV).scatter_reduce(1, cell.clamp(min=0).long(), torch.where(occ & view, depth, inf), "amin", include_self=True)
    zmin = -torch.nn.functional.max_pool2d(-Z.view(B, 1, h, w), 2 * radius + 1, stride=1, padding=radius).view(B, h * w)
    bound = zmin * torch.tensor(vr.opr32(rel_tol), device=DEV)
    bound = bound + torch.tensor(np.float32(abs_tol), device=DEV)
    vis = sel & view & (torch.where(view, depth, inf) <= bound.gather(1, cell.clamp(min=0).long()))
    counts = torch.stack([sel.sum(1), (sel & view).sum(1), vis.sum(1), (occ & view).sum(1)], 1).int()
    return Z.view(B, h, w), vis.view(-1), counts


@pytest.mark.parametrize("name,radius", [(s[0], r) for s in vr.SCENES for r in s[2]])
def test_chain_of_exact_equalities(name, radius):
    sc = vr.built(name)
    B, _, N = sc["pts"].shape
    out = _call(sc, radius)
    vis, counts, dmap, cell, depth = out
    # (a) cell and "in view" are guided_match's at radius 0 on the rows of mask | occ_mask
    union = torch.ones_like(sc["mask"]) if sc["occ_mask"] is None else sc["mask"] | sc["occ_mask"]
    zero_pc, zero_img = torch.zeros(B * N, 64, device=DEV), torch.zeros(B, sc["h"], sc["w"], 64, device=DEV)
    idx, _, gcounts, _, _ = ops.guided_match(F(sc["pts"]), zero_pc, zero_img, union.to(DEV), F(sc["pose"]), F(sc["K"]), 0)
    assert torch.equal(cell, idx) and torch.equal((cell >= 0).view(B, N).sum(1).int(), gcounts[:, 1])
    assert bool((torch.isnan(depth) | (depth > 0)).all()) and bool((depth[cell >= 0] > 0).all())
    # (b), (c) the map, the flags and the counts from the op's own cell / depth
    rZ, rvis, rcounts = _restated(sc, out, radius, vr.REL_TOL, vr.ABS_TOL)
    print(name, "r", radius, "counts", counts.tolist())
    assert torch.equal(_bits(dmap), _bits(rZ))
    assert torch.equal(vis, rvis)
    assert torch.equal(counts, rcounts)
    # another tolerance pair, the same chain
    out2 = _call(sc, radius, rel_tol=0.0, abs_tol=0.25)
    rZ2, rvis2, rcounts2 = _restated(sc, out2, radius, 0.0, 0.25)
    assert torch.equal(_bits(out2[2]), _bits(rZ2)) and torch.equal(out2[0], rvis2) and torch.equal(out2[1], rcounts2)


# ---- 3. against float64 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,radius", [(s[0], r) for s in vr.SCENES for r in s[2]])
def test_against_float64(name, radius):
    sc = vr.built(name)
    B, _, N = sc["pts"].shape
    vis, counts, dmap, cell, depth = (t.cpu().numpy() for t in _call(sc, radius))
    ref = vr.visibility(sc["pts"], sc["mask"], sc["occ_mask"], sc["pose"], sc["K"], sc["h"], sc["w"], radius, vr.REL_TOL, vr.ABS_TOL)
    vis, depth = vis.reshape(B, N), depth.reshape(B, N).astype(np.float64)
    for b, r in enumerate(ref):
        und = r["undecided"]
        print(name, "r", radius, "sample", b, "counts", counts[b].tolist(), "float64, decided", r["counts_lo"], "undecided", und,
              "ambiguous occluders", r["occ_amb"])
        assert np.array_equal(vis[b][r["decided"]], r["visible"][r["decided"]])
        assert counts[b, 0] == r["counts_lo"][0]
        for k in (1, 2):
            assert r["counts_lo"][k] <= counts[b, k] <= r["counts_lo"][k] + und
        assert r["counts_lo"][3] <= counts[b, 3] <= r["counts_lo"][3] + r["occ_amb"]
        # the map on the decided cells: +inf where float64 has +inf, else within the rounding bound of the cell's occluders
        dec, Z64, Z32 = r["cell_decided"], r["Z_lo"], dmap[b].astype(np.float64)
        assert np.array_equal(np.isinf(Z32[dec]), np.isinf(Z64[dec]))
        fin = dec & np.isfinite(Z64)
        err = np.abs(Z32[fin] - Z64[fin])
        print("   decided cells", int(dec.sum()), "of", dec.size, "finite", int(fin.sum()), "worst share of the rounding bound",
              float((err / r["err_map"][fin]).max()) if fin.any() else 0.0)
        assert (err <= r["err_map"][fin]).all()
        # the per-row depth: 8 2^-23 S
        union = r["sel"] | r["occ"]
        front = union & (r["z"] > vr.P2_TOL * r["S"])
        assert (np.abs(depth[b][front] - r["z"][front]) <= 8.0 * 2.0 ** -23 * r["S"][front]).all()
        assert np.isnan(depth[b][~union]).all() and np.isnan(depth[b][union & (r["z"] < -vr.P2_TOL * r["S"])]).all()


# ---- 4. planted occlusion -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1])
@pytest.mark.parametrize("h,w", [(13, 19), (40, 128)])
def test_planted_occlusion(h, w, radius):
    sc = vr.planted_occlusion(h, w, seed=311)
    N = sc["pts"].shape[2]
    ones = torch.ones(1, N, dtype=torch.bool, device=DEV)
    vis, counts, dmap, _, _ = ops.visibility(F(sc["pts"]), F(sc["pose"]), F(sc["K"]), h, w, ones, radius=radius, rel_tol=vr.REL_TOL, want_depth_map=True)
    assert np.array_equal(vis.cpu().numpy(), sc["expect"])
    assert counts[0].tolist() == [N, N, int(sc["expect"].sum()), N]
    assert bool(torch.isinf(dmap[0, :, w // 2]).all()) and bool(((dmap[0, :, :w // 2] - 4).abs() < 1e-3).all()) and bool(((dmap[0, :, w // 2 + 1:] - 10).abs() < 1e-3).all())


# ---- 5. edges -------------------------------------------------------------------------------------------------------------------------------------
def test_empty_sample_and_nan_pose():
    sc = vr.built("n1025_13x19")
    base = _call(sc, 1)
    N = sc["pts"].shape[2]
    m = sc["mask"].clone()
    m[0] = False
    vis, counts, dmap, cell, depth = _call(sc, 1, mask=m)
    assert not bool(vis[:N].any()) and counts[0, :3].tolist() == [0, 0, 0] and counts[0, 3] == base[1][0, 3]
    assert torch.equal(vis[N:], base[0][N:]) and torch.equal(counts[1:], base[1][1:]) and torch.equal(_bits(dmap), _bits(base[2]))
    # sample 0 with no row at all in either mask: zeros, a map of +inf, cell -1, depth NaN
    vis, counts, dmap, cell, depth = _call(sc, 1, mask=m, occ_mask=m)
    assert counts[0].tolist() == [0, 0, 0, 0] and bool(torch.isinf(dmap[0]).all()) and bool((cell[:N] == -1).all()) and bool(torch.isnan(depth[:N]).all())
    # a NaN pose in sample 1 leaves the others as they were
    pose = sc["pose"].copy()
    pose[1] = math.nan
    vis, counts, dmap, cell, depth = _call(sc, 1, pose=pose)
    assert counts[1].tolist() == [int(sc["mask"][1].sum()), 0, 0, 0] and not bool(vis[N:2 * N].any())
    assert bool(torch.isinf(dmap[1]).all()) and bool((dmap[1] > 0).all()) and bool((cell[N:2 * N] == -1).all()) and bool(torch.isnan(depth[N:2 * N]).all())
    for k in (0, 2):
        assert torch.equal(vis[k * N:(k + 1) * N], base[0][k * N:(k + 1) * N]) and torch.equal(counts[k], base[1][k])
        assert torch.equal(_bits(dmap[k]), _bits(base[2][k])) and torch.equal(cell[k * N:(k + 1) * N], base[3][k * N:(k + 1) * N])


def test_a_queried_row_that_does_not_occlude_stays_out_of_the_map():
    pts, pose, K = (t.to(DEV) for t in vr.hand())
    N = pts.shape[2]
    ones = torch.ones(1, N, dtype=torch.bool, device=DEV)
    occ = ones.clone()
    occ[0, 0] = False                     # row 0 (depth 2) would hide rows 1 and 2 (depth 5) if it wrote itself into Z
    vis, counts, dmap, cell, depth = ops.visibility(pts, pose, K, vr.HAND_H, vr.HAND_W, ones, occ_mask=occ, radius=1, rel_tol=vr.HAND_REL_TOL,
                                                    want_depth_map=True, want_cell=True, want_depth=True)
    assert vis.int().tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 1, 1] and counts[0].tolist() == [10, 8, 7, 7]
    assert float(dmap[0, 2, 3]) == 5.0 and cell[0].item() == 2 * vr.HAND_W + 3 and float(depth[0]) == 2.0
    # an occluder that is not queried: not visible, but in the map
    q = ones.clone()
    q[0, [0, 3]] = False
    vis, counts, dmap, _, _ = ops.visibility(pts, pose, K, vr.HAND_H, vr.HAND_W, q, radius=0, rel_tol=vr.HAND_REL_TOL, want_depth_map=True)
    assert vis.int().tolist() == [0, 0, 1, 0, 1, 0, 0, 1, 1, 1] and counts[0].tolist() == [8, 6, 5, 8] and torch.equal(dmap.cpu(), vr.hand_depth_map())


def test_mask_dtypes_agree():
    sc = vr.built("n257_13x19_occ")
    outs = [_call(sc, 2, mask=cast(sc["mask"]), occ_mask=cast(sc["occ_mask"])) for cast in
            (lambda m: m, lambda m: m.to(torch.uint8), lambda m: m.long() * 7)]
    mixed = _call(sc, 2, mask=sc["mask"].long(), occ_mask=sc["occ_mask"])
    for o in outs[1:] + [mixed]:
        _same(o, outs[0])


def test_equal_depths_at_zero_tolerance_are_both_visible():
    pts = torch.tensor([[[3.0 * 2, 3 * 2, 3 * 2.5], [2.0 * 2, 2 * 2, 2 * 2.5], [2.0, 2.0, 2.5]]], device=DEV)      # (3, 2) twice at depth 2, once at 2.5
    ones = torch.ones(1, 3, dtype=torch.bool, device=DEV)
    eye4, eye3 = torch.eye(4, device=DEV)[None].contiguous(), torch.eye(3, device=DEV)[None].contiguous()
    for radius in (0, 1):
        vis, counts, _, _, _ = ops.visibility(pts, eye4, eye3, 8, 10, ones, radius=radius, rel_tol=0.0, abs_tol=0.0)
        assert vis.tolist() == [True, True, False] and counts[0].tolist() == [3, 3, 2, 3]
    vis, _, _, _, _ = ops.visibility(pts, eye4, eye3, 8, 10, ones, radius=0, rel_tol=0.0, abs_tol=0.5)
    assert vis.tolist() == [True, True, True]


def test_bound_is_rounded_twice():
    """bound = zmin * opr + abs_tol is a rounded product and then a rounded sum, never one fma.  With both tolerances
    positive the two differ for about a third of the depths, so rows are planted ON the bound: 96 occluder / query pairs, each alone in
    its cell of a 12 x 16 map under the identity pose and intrinsics (depth = Z exactly).  Pairs 0 .. 31: the fused bound is lower, the
    query sits on the two-rounding bound and is visible.  Pairs 32 .. 63: the fused bound is higher, the query sits one float above the
    two-rounding bound and is not.  Pairs 64 .. 95: the bounds agree; half on the bound, half one float above."""
    h, w, rel_tol, abs_tol, per = 12, 16, 0.05, 0.1, 32
    opr, tol = vr.opr32(rel_tol), np.float32(abs_tol)
    z0 = np.random.default_rng(20261018).uniform(1.0, 50.0, 4096).astype(np.float32)
    unfused = (z0 * opr).astype(np.float32) + tol                                                     # fp32 product, then fp32 sum
    fused = (z0.astype(np.float64) * np.float64(opr) + np.float64(tol)).astype(np.float32)            # exact in float64: rounded once
    assert unfused.dtype == np.float32
    above = np.nextafter(unfused, np.float32(np.inf))
    groups = [np.flatnonzero(fused < unfused)[:per], np.flatnonzero(fused > unfused)[:per], np.flatnonzero(fused == unfused)[:per]]
    assert [len(g) for g in groups] == [per, per, per]
    pick = np.concatenate(groups)
    on_bound = np.r_[np.ones(per, bool), np.zeros(per, bool), np.arange(per) < per // 2]              # the planted expectation
    zo, zq = z0[pick], np.where(on_bound, unfused[pick], above[pick]).astype(np.float32)
    assert bool(((zq <= unfused[pick]) == on_bound).all())
    assert bool((zq[:per] > fused[pick[:per]]).all()) and bool((zq[per:2 * per] <= fused[pick[per:2 * per]]).all())
    assert bool(((zq[2 * per:] <= fused[pick[2 * per:]]) == on_bound[2 * per:]).all())
    npair = 3 * per
    N = 2 * npair
    cells = np.random.default_rng(7).permutation(h * w)[:npair]
    z = np.stack([zo, zq], 1).reshape(N)                                                              # row 2i occludes, row 2i + 1 is queried
    cx, cy = np.repeat(cells % w, 2).astype(np.float32), np.repeat(cells // w, 2).astype(np.float32)
    query = torch.arange(N) % 2 == 1
    sc = {"pts": np.stack([cx * z, cy * z, z])[None], "pose": np.eye(4, dtype=np.float32)[None], "K": np.eye(3, dtype=np.float32)[None],
          "h": h, "w": w, "mask": query[None].clone(), "occ_mask": ~query[None]}
    out = _call(sc, 0, rel_tol=rel_tol, abs_tol=abs_tol)
    vis, counts, dmap, cell, depth = out
    assert torch.equal(_bits(depth), _bits(F(z)))                                                     # depth is Z, bit for bit
    assert cell.tolist() == np.repeat(cells, 2).tolist()                                              # each pair alone in its cell
    want = torch.zeros(N, dtype=torch.bool)
    want[1::2] = torch.from_numpy(on_bound)
    wrong = (vis.cpu() != want)[1::2].view(3, per).sum(1).tolist()
    print("pairs classified against the two-rounding bound, per group (fused lower, fused higher, equal):", wrong)
    assert torch.equal(vis.cpu(), want)
    _, rvis, rcounts = _restated(sc, out, 0, rel_tol, abs_tol)
    assert torch.equal(vis, rvis)
    assert torch.equal(counts, rcounts) and counts[0].tolist() == [npair, npair, int(on_bound.sum()), npair]


# ---- 6. determinism ------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_agree_bit_for_bit():
    sc = vr.built("n1025_40x128")
    _same(_call(sc, 2), _call(sc, 2))


def test_sample_alone_equals_sample_in_batch():
    sc = vr.built("n257_13x19_occ")
    B, _, N = sc["pts"].shape
    vis, counts, dmap, cell, depth = _call(sc, 1)
    for k in range(B):
        one = _call(sc, 1, sl=slice(k, k + 1))
        rows = slice(k * N, (k + 1) * N)
        _same(one, (vis[rows], counts[k:k + 1], dmap[k:k + 1], cell[rows], depth[rows]))


def test_graph_replay_equals_eager():
    sc = vr.built("n1025_13x19")
    args = (F(sc["pts"]), F(sc["pose"]), F(sc["K"]), sc["h"], sc["w"], sc["mask"].to(DEV))
    fn = lambda: ops.visibility(*args, radius=2, want_depth_map=True, want_cell=True, want_depth=True)
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
        t.fill_(1)
    graph.replay()
    torch.cuda.synchronize()
    _same(got, eager)


# ---- 7. the model layer and the scripts -------------------------------------------------------------------------------------------------------------
def _model(N):
    from cmr_agent_amd.models import MultiHeadModel
    from cmr_agent_amd.config import KittiConfiguration
    return MultiHeadModel(KittiConfiguration(num_pt=N, device=torch.device(DEV)))


_GEO = {}


def _geo():
    """One gref.scene batch and its model, built once -> (scene, model)."""
    if not _GEO:
        _GEO["v"] = (gref.scene(B=2, N=1024, h=40, w=128, seed=201), _model(1024))
    return _GEO["v"]


def _data(sc):
    B, _, N = sc["pts"].shape
    mask = torch.rand(B, N, generator=torch.Generator().manual_seed(21)) < 0.7
    return {"pc": F(sc["pts"]), "K": F(sc["K"]), "P": F(sc["P"]), "pnp_pose": F(sc["start"]),
            "pc_geo_feat": sc["pc"].view(B, N, 64).permute(0, 2, 1).contiguous().to(DEV),
            "img_geo_feat": sc["img"].permute(0, 3, 1, 2).contiguous().to(DEV), "pc_overlap_pred": mask.to(DEV)}


def test_visible_points_and_render_depth():
    sc, model = _geo()
    data = _data(sc)
    B, _, N = sc["pts"].shape
    model.visible_points(data)
    vm, vc = data["visible_mask"], data["visible_counts"]
    assert vm.dtype == torch.bool and tuple(vm.shape) == (B, N) and vc.dtype == torch.int32 and tuple(vc.shape) == (B, 4)
    direct = ops.visibility(data["pc"], data["pnp_pose"], data["K"], 40, 128, data["pc_overlap_pred"], radius=1, rel_tol=0.05)
    assert torch.equal(vm.view(-1), direct[0]) and torch.equal(vc, direct[1])
    assert vc[:, 0].tolist() == data["pc_overlap_pred"].sum(1).tolist() and bool((vm <= data["pc_overlap_pred"]).all())
    model.visible_points(data, pose=F(sc["P"]), radius=0, rel_tol=0.1, abs_tol=0.2, mask=torch.ones(B, N, dtype=torch.bool), occluders="mask")
    assert data["visible_counts"][:, 0].tolist() == [N] * B and torch.equal(data["visible_counts"][:, 1], data["visible_counts"][:, 3])
    model.render_depth(data)
    dm = data["depth_map"]
    assert dm.dtype == torch.float32 and tuple(dm.shape) == (B, 40, 128) and bool((dm > 0).all()) and bool(torch.isinf(dm).any()) and bool(torch.isfinite(dm).any())
    every = torch.ones(B, N, dtype=torch.bool, device=DEV)
    assert torch.equal(_bits(dm), _bits(ops.visibility(data["pc"], data["pnp_pose"], data["K"], 40, 128, every, radius=0, want_depth_map=True)[2]))
    K4 = F(sc["K"]).clone()
    K4[:, :2] *= 4.0
    model.render_depth(data, pose=F(sc["P"]), size=(160, 512), K=K4)
    assert tuple(data["depth_map"].shape) == (B, 160, 512) and bool(torch.isfinite(data["depth_map"]).any())
    # no more cells are filled than points are in view, and the nearest depth of the cloud is in the map
    assert int(torch.isfinite(data["depth_map"]).sum()) <= B * N


def test_refine_with_visible():
    sc, model = _geo()
    data = _data(sc)
    radii, thrs = (4, 2), (3.0, 1.5)
    model.refine_pose_from_matches(data, radii=radii, thrs=thrs, visible=True)
    rv, gc = data["refine_visible_counts"], data["guided_counts"]
    assert rv.dtype == torch.int32 and tuple(rv.shape) == (2, 2, 4) and tuple(gc.shape) == (2, 2, 4)
    assert torch.equal(gc[:, :, 0], rv[:, :, 2])                                      # the rows handed to the match are the visible ones
    print("refine_visible_counts", rv.tolist())
    # round 0 runs under the start pose, round 1 under the pose round 0 returned (every op is deterministic, so a one-round run gives it)
    direct0 = ops.visibility(data["pc"], data["pnp_pose"], data["K"], 40, 128, data["pc_overlap_pred"], radius=1, rel_tol=0.05)
    assert torch.equal(rv[0], direct0[1])
    one = _data(sc)
    model.refine_pose_from_matches(one, radii=radii[:1], thrs=thrs[:1], visible=True)
    direct1 = ops.visibility(data["pc"], one["refined_pose"], data["K"], 40, 128, data["pc_overlap_pred"], radius=1, rel_tol=0.05)
    assert torch.equal(rv[1], direct1[1])
    # a dict changes the test, None is the old path and sets no key
    two = _data(sc)
    model.refine_pose_from_matches(two, radii=radii, thrs=thrs, visible=dict(radius=0, rel_tol=0.5))
    assert bool((two["refine_visible_counts"][0, :, 2] >= rv[0, :, 2]).all())
    plain = _data(sc)
    model.refine_pose_from_matches(plain, radii=radii, thrs=thrs)
    assert "refine_visible_counts" not in plain and torch.equal(plain["guided_counts"][:, :, 0], rv[:, :, 0])


def test_search_with_visible():
    sc, model = _geo()
    data = _data(sc)
    levels = ((1, 0.5, 0.05, 1), (0, 0.25, 0.025, 1))
    model.search_pose(data, levels=levels, visible=True)
    sv = data["search_visible_counts"]
    assert sv.dtype == torch.int32 and tuple(sv.shape) == (2, 2, 4) and tuple(data["searched_pose"].shape) == (2, 4, 4)
    direct0 = ops.visibility(data["pc"], data["pnp_pose"], data["K"], 40, 128, data["pc_overlap_pred"], radius=1, rel_tol=0.05)
    assert torch.equal(sv[0], direct0[1])


def _run(script, *flags):
    cmd = [sys.executable, os.path.join(ROOT, script), "--pairs", "1", "--img", "160x512", "--num-pt", "4096", *flags]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return res.stdout.strip().splitlines()


def _shape(line):
    """A line's format: its words, every number replaced by '#'."""
    def word(t):
        try:
            float(t)
            return "#"
        except ValueError:
            return t
    return [word(t) for t in line.split()]


def _check_script(script, flags):
    plain = _run(script, *flags)
    assert not [l for l in plain if l.startswith("visible")]
    lines = _run(script, *flags, "--visible", "--visible-radius", "1", "--visible-rel-tol", "0.05")
    vis = [l for l in lines if l.startswith("visible ")]
    assert len(vis) == 1, lines                                                        # one batch
    tok = vis[0].split()
    assert len(tok) == 6 and tok[2] == "of" and tok[4] == "of" and 0 <= int(tok[1]) <= int(tok[3]) <= int(tok[5])
    # every other line keeps the format it has without the flag (the mean / std lines appear only when a pair is recalled: left out)
    keep = lambda ls: [_shape(l) for l in ls if not l.startswith("visible ") and "Mean:" not in l]
    assert keep(lines) == keep(plain)


def test_test_geo_script_visible():
    _check_script("Test_Geo.py", ("--pnp", "--guided", "4,2"))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "Test_Geo.py"), "--pnp", "--visible"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "--visible" in res.stderr


def test_test_agent_script_visible():
    _check_script("Test_Agent.py", ("--refine", "4,2"))
