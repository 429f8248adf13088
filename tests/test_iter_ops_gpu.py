"""GPU tier of the pose cost volume's kernels (csrc/iter_model.hip): every kernel case by case against the float64 restatement in
iter_reference.py, whose agreement with the oracle and whose caps tests/test_iter_cpu.py asserts.  Cells, counts and indices must be
identical wherever fp32 can decide them (iter_reference's docstring says where that is); values carry tolerances derived from the
roundings of the kernel, stated next to each bound in iter_reference.  Each check prints its largest error / bound ratio."""
import math

import numpy as np
import pytest
import torch

import iter_reference as ir

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = ir.U


@pytest.fixture(scope="module")
def ops():
    from cmr_agent_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib():
    from cmr_agent_amd import _lib
    return _lib


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().double().numpy()


def _ratio(err, bound):
    """largest err / bound; an error where the bound is zero must be zero (ratio inf otherwise)"""
    err, bound = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    with np.errstate(all="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(q.max()) if q.size else 0.0


def _poses(ops, r_amp, t_amp, n):
    return ops.iter_sample_poses(_d(np.float32([r_amp])), _d(np.float32([t_amp])), n)


# ---- iter_sample_poses ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 5, 7, 9, 11, 13, 15])
@pytest.mark.parametrize("amps", [(0.1, 1.5), (math.pi, 40.0), (0.0, 0.0)])
def test_sample_poses_tables_bit_for_bit_and_matrices_within_the_bound(ops, n, amps):
    dr, dt, rt = _poses(ops, amps[0], amps[1], n)
    wr, wt, wrt, bound = ir.sample_poses(np.float32([amps[0]]), np.float32([amps[1]]), n)
    assert np.array_equal(dr.cpu().numpy(), wr) and np.array_equal(dt.cpu().numpy(), wt)
    got = _np(rt)
    assert got.shape == (n ** 3, 3, 4)
    assert np.array_equal(got[:, 1], np.broadcast_to(np.array([0.0, 1.0, 0.0, 0.0]), (n ** 3, 4)))
    err = np.abs(got - wrt)
    sincos = max(float(err[:, 0, 0].max()), float(err[:, 0, 2].max()), float(err[:, 2, 0].max()), float(err[:, 2, 2].max()))
    print("sample_poses n=%d amps=%s: sinf / cosf off by at most %.2f U (stated %.0f U); err / bound %.3f"
          % (n, amps, sincos / U, ir.SINCOS_ERR / U, _ratio(err, bound)))
    assert sincos <= ir.SINCOS_ERR
    assert (err <= bound).all()


@pytest.mark.parametrize("n", [1, 2, 4, 17])
def test_sample_poses_refuses_what_it_cannot_sample(ops, lib, n):
    with pytest.raises(lib.CmrError):
        _poses(ops, 0.1, 1.5, n)


# ---- warp: both paths against the reference -----------------------------------------------------------------------------------------------
class _Warp:
    """one scene on the device: both paths run once, the float64 reference computed once from the device's own matrices"""

    def __init__(self, ops, s, rt, mask, standby, want_sel=None):
        self.s, self.h, self.w, self.N = s, s["h"], s["w"], s["pc"].shape[1]
        h, w = self.h, self.w
        self.w1, self.base = ir.stencil_inputs(h, w)
        pc, feat, score, K = _d(s["pc"]), _d(s["feat"]), _d(s["score"]), _d(s["K"]).view(-1)
        mask, standby, w1, base = _d(mask), _d(standby), _d(self.w1), _d(self.base)
        acc, cnt, occ, sel = ops.iter_warp_scatter(pc, feat, score, mask, standby, rt, K, h, w)
        res = ops.iter_finalize(acc, cnt, occ, w1, base)                       # acc becomes the scatter mean in place
        self.atomic = dict(mean=acc, cnt=cnt, occ=occ, res=res, sel=sel)
        warped, res2, occ2, sel2 = ops.iter_warp_bin(pc, feat, score, mask, standby, rt, K, w1, base, h, w)
        self.band = dict(mean=warped, cnt=None, occ=occ2, res=res2, sel=sel2)
        self.sel = ir.select_mask(_np(mask), _np(standby)) if want_sel is None else want_sel
        self.r = ir.warp(s["pc"], s["feat"], s["score"], self.sel, _np(rt), s["K"], h, w)
        self.fmax = float(np.abs(s["feat"]).max())

    def check(self, tag):
        r, h, w = self.r, self.h, self.w
        pts, cells = ir.shares(r)
        assert pts <= ir.MAX_UNDECIDED_POINTS and cells <= ir.MAX_UNDECIDED_CELLS, (pts, cells)      # with the device's matrices too
        cd = r["cell_decided"]
        ob, mb = ir.occ_bound(r), ir.mean_bound(r, self.fmax)
        # what the occupancy plane of an undecided cell may be off by, for the stencil of its neighbours: one point more, one score (< 1) more
        plane_err = np.where(cd, ob, ir.SAFETY * r["count"] * U * (r["occ_abs"] + 1.0))
        for path, g in (("atomic", self.atomic), ("band", self.band)):
            assert np.array_equal(g["sel"].cpu().numpy(), self.sel), path
            occ, mean = _np(g["occ"]), _np(g["mean"])
            if g["cnt"] is not None:
                assert np.array_equal(_np(g["cnt"])[cd], r["count"][cd].astype(np.float64)), path
            assert np.array_equal((occ != 0)[cd], (r["occ"] != 0)[cd]), path
            e_occ, e_mean = np.abs(occ - r["occ"]), np.abs(mean - r["mean"])
            want, mag = ir.stencil(occ, self.w1, self.base)                     # the path's own occupancy plane goes in
            rb = ir.stencil_bound(mag, plane_err if path == "band" else None, self.w1)
            e_res = np.abs(_np(g["res"]) - want)
            print("%s %s: occupancy err / bound %.3f, mean %.3f, res %.3f; %d cells left out of %d" %
                  (tag, path, _ratio(e_occ[cd], ob[cd]), _ratio(e_mean[cd], mb[cd]), _ratio(e_res, rb), int((~cd).sum()), cd.size))
            assert (e_occ[cd] <= ob[cd]).all(), path
            assert (e_mean[cd] <= mb[cd]).all(), path
            assert (e_res <= rb).all(), path


def _hand(ops, name, rolled=False):
    s = ir.hand_scenes()[name] if not rolled else ir.rolled_edges()
    _, _, rt = _poses(ops, s["r_amp"], s["t_amp"], s["n"])
    assert np.array_equal(np.abs(_np(rt)[s["pose"]]), np.eye(4)[0:3])             # cosf(0) = 1, sinf(0) = 0: the identity, exactly
    return s, _Warp(ops, s, rt, s["sel"], np.zeros_like(s["sel"]), want_sel=s["sel"])


@pytest.mark.parametrize("rolled", [False, True])
def test_edges_bit_for_bit_on_both_paths(ops, rolled):
    """every boundary of the in-view test and of the rounding, with N as given and with the scene rolled across the chunk boundary at 4096"""
    s, wp = _hand(ops, "edges", rolled)
    p, e, r = s["pose"], s["expect"], wp.r
    assert r["decided"][p].all() and r["cell_decided"][p].all() and np.array_equal(r["cell"][p], e["cell"])       # nothing is left out
    for path, g in (("atomic", wp.atomic), ("band", wp.band)):
        if g["cnt"] is not None:
            assert np.array_equal(_np(g["cnt"])[p], e["count"].astype(np.float64)), path
        assert np.array_equal(_np(g["occ"])[p], e["occ"]), path
        assert np.array_equal(_np(g["mean"])[p], e["mean"]), path
    wp.check("edges rolled" if rolled else "edges")


def test_crowded_cell_fed_from_three_chunks(ops):
    s, wp = _hand(ops, "crowded")
    p, e, r = s["pose"], s["expect"], wp.r
    y, x = ir.CROWDED_CELL
    assert r["decided"][p].all() and r["cell_decided"][p].all() and np.array_equal(r["count"][p], e["count"])
    assert float(wp.atomic["cnt"][p, y, x]) == ir.CROWDED_COUNT == e["count"][y, x]
    assert np.array_equal(_np(wp.atomic["cnt"])[p], e["count"].astype(np.float64))
    for path, g in (("atomic", wp.atomic), ("band", wp.band)):
        err = np.abs(_np(g["mean"])[p, y, x] - r["mean"][p, y, x])
        bound = ir.mean_bound(r, wp.fmax)[p, y, x]
        print("crowded %s: the cell of %d points: mean err %.3e against the bound %.3e" % (path, ir.CROWDED_COUNT, float(err.max()), float(bound.min())))
        assert (np.abs(_np(g["mean"])[p]).max(-1) > 0).sum() == (e["count"] > 0).sum()
    wp.check("crowded")


@pytest.mark.parametrize("h,w,n,N", ir.WARP_SHAPES)
def test_warp_on_maps_of_every_band_layout(ops, h, w, n, N):
    s = ir.synthetic_cloud(h, w, N, n=n)
    _, _, rt = _poses(ops, ir.WARP_AMPS[0], ir.WARP_AMPS[1], n)
    wp = _Warp(ops, s, rt, s["mask"], s["standby"])
    assert wp.r["count"].sum() > 0
    wp.check("%dx%d n=%d" % (h, w, n))


# ---- mask selection ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 5000])
def test_mask_selection_through_both_entry_points(ops, N):
    s = ir.synthetic_cloud(8, 8, N, seed=1)
    _, _, rt = _poses(ops, ir.WARP_AMPS[0], ir.WARP_AMPS[1], 3)
    standby = (np.arange(N) % 3 != 1).astype(np.uint8)
    last = np.zeros(N, dtype=np.uint8)
    last[N - 1] = 1
    odd = np.zeros(N, dtype=np.uint8)
    odd[::2], odd[N - 1] = 2, 255
    zero = np.zeros(N, dtype=np.uint8)
    for tag, mask, sb, want in (("last", last, standby, last), ("2/255", odd, standby, (odd != 0).astype(np.uint8)), ("standby", zero, standby, standby),
                                ("none", zero, zero, zero)):
        wp = _Warp(ops, s, rt, mask, sb)
        assert np.array_equal(wp.sel, want) and wp.sel.max() <= 1
        wp.check("mask %s N=%d" % (tag, N))
        if tag == "none":
            for g in (wp.atomic, wp.band):
                assert float(g["mean"].abs().max()) == 0 and float(g["occ"].abs().max()) == 0
                assert torch.equal(g["res"].cpu(), torch.from_numpy(wp.base).expand(27, -1, -1, -1))
            assert float(wp.atomic["cnt"].abs().max()) == 0


# ---- refusals: no launch happens -------------------------------------------------------------------------------------------------------------
def test_warp_refuses_a_map_wider_than_a_band_and_an_empty_cloud(ops, lib):
    from cmr_agent_amd.ops import _p, _stream
    h, w, N, P = 1, 385, 8, 27
    s = ir.synthetic_cloud(8, 8, N, seed=2)
    _, _, rt = _poses(ops, 0.1, 1.5, 3)
    pc, feat, score, K = _d(s["pc"]), _d(s["feat"]), _d(s["score"]), _d(s["K"]).view(-1)
    m = torch.ones(N, dtype=torch.uint8, device=DEV)
    w1, base = (_d(a) for a in ir.stencil_inputs(h, w))
    with pytest.raises(ValueError):
        ops.iter_warp_bin(pc, feat, score, m, m, rt, K, w1, base, h, w)
    warped, res, occ = torch.zeros(P, h, w, 64, device=DEV), torch.zeros(P, h, w, 64, device=DEV), torch.zeros(P, h, w, device=DEV)
    sel = torch.zeros(N, dtype=torch.uint8, device=DEV)
    with pytest.raises(lib.CmrError):
        lib.call("cmr_iter_warp_bin_f32", _p(pc), _p(feat), _p(score), _p(m), _p(m), _p(sel), _p(rt), _p(K), _p(w1), _p(base), _p(warped), _p(res),
                 _p(occ), N, P, h, w, _stream())
    assert float(warped.abs().max()) == 0 and float(res.abs().max()) == 0 and float(sel.max()) == 0
    # the same call is accepted one column narrower: it was the width that was refused
    w1n, basen = (_d(a) for a in ir.stencil_inputs(h, 384))
    ops.iter_warp_bin(pc, feat, score, m, m, rt, K, w1n, basen, h, 384)
    # N = 0: pointers to one element, so that it is the count that is refused
    for name, extra in (("cmr_iter_warp_bin_f32", (_p(w1n), _p(basen), _p(warped), _p(res), _p(occ))), ("cmr_iter_warp_scatter_f32", (_p(warped), _p(res), _p(occ)))):
        with pytest.raises(lib.CmrError):
            lib.call(name, _p(pc), _p(feat), _p(score), _p(m), _p(m), _p(sel), _p(rt), _p(K), *extra, 0, P, h, 384, _stream())
    e3, e64, e0 = torch.zeros(3, 0, device=DEV), torch.zeros(0, 64, device=DEV), torch.zeros(0, device=DEV)
    m0 = torch.zeros(0, dtype=torch.uint8, device=DEV)
    with pytest.raises(lib.CmrError):
        ops.iter_warp_scatter(e3, e64, e0, m0, m0, rt, K, 8, 8)
    with pytest.raises(lib.CmrError):
        ops.iter_warp_bin(e3, e64, e0, m0, m0, rt, K, w1n, basen, h, 384)


# ---- iter_finalize without accumulators: the model's overlap-plane call ---------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (9, 1), (16, 24)])
def test_finalize_without_accumulators_is_the_stencil(ops, h, w, P):
    r = np.random.RandomState(17 * h + w + P)
    plane = (r.uniform(0, 1, (P, h, w)) < 0.7).astype(np.float32) * r.uniform(0.5, 1.5, (P, h, w)).astype(np.float32)
    w1, base = ir.stencil_inputs(h, w, seed=P)
    got = ops.iter_finalize(None, None, _d(plane), _d(w1), _d(base))
    want, mag = ir.stencil(plane, w1, base)
    err, bound = np.abs(_np(got) - want), ir.stencil_bound(mag)
    print("finalize %dx%d P=%d: err / bound %.3f" % (h, w, P, _ratio(err, bound)))
    assert got.shape == (P, h, w, 64) and (err <= bound).all()


# ---- iter_head -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,cells,ldc", ir.HEAD_CASES)
def test_head_reads_eight_channels_and_pools_over_any_cell_count(ops, P, cells, ldc):
    a = ir.head_inputs(P, cells, ldc)
    got = ops.iter_head(_d(a["x"]).view(P, cells, 1, ldc), _d(a["w24"]), _d(a["b24"]), _d(a["w26"]), _d(a["b26"]), ir.HEAD_SLOPE)
    want, bound = ir.head(a["x"], a["w24"], a["b24"], a["w26"], a["b26"], ir.HEAD_SLOPE)
    g = _np(got)
    assert np.isfinite(g).all()                                                  # channels 8.. are NaN and must not be read
    err = np.abs(g - want)
    print("head P=%d cells=%d ldc=%d: err / bound %.3f (largest err %.2e)" % (P, cells, ldc, _ratio(err, bound), float(err.max())))
    assert (err <= bound).all()


# ---- iter_decide -----------------------------------------------------------------------------------------------------------------------------
def _decide(ops, s):
    n = s["n"]
    label, out_f, out_i, m = ops.iter_decide(_d(s["logits"]), n, _d(s["label_r"]), _d(s["label_tx"]), _d(s["label_tz"]), _d(s["delta_r"]),
                                             _d(s["delta_t"]))
    d = ir.decide(s["logits"], n, s["label_r"], s["label_tx"], s["label_tz"], s["delta_r"], s["delta_t"])
    idx, f = out_i.cpu().numpy().tolist(), out_f.cpu().numpy()
    assert (np.abs(_np(label) - d["label"]) <= d["label_bound"]).all()                      # two roundings of the float64 product
    assert all(0 <= i < n for i in idx[1:4]) and 0 <= idx[0] < n ** 3 and 0 <= idx[4] < n ** 3
    # the step is the table entry of the kernel's own index, bit for bit
    assert f[1] == s["delta_r"][idx[1]] and f[2] == s["delta_t"][idx[2]] and f[3] == s["delta_t"][idx[3]]
    M, MB = ir.inverse_pose(f[1], f[2], f[3])
    e_m = np.abs(_np(m) - M)
    assert (e_m <= MB).all(), (e_m, MB)
    return d, idx, float(f[0]), _ratio(e_m, MB)


@pytest.mark.parametrize("n", ir.DECIDE_N)
@pytest.mark.parametrize("name", ir.DECIDE_SCENES)
def test_decide_scenes_every_index_exact(ops, name, n):
    s = ir.decide_scene(name, n)
    d, idx, loss, rm = _decide(ops, s)
    assert d["decided"].all()                                                    # by construction; asserted on the CPU tier as well
    assert tuple(idx) == tuple(d["idx"]), (idx, d["idx"])
    for want, got in zip(s["expect"], idx):
        assert want is None or want == got
    err = abs(loss - d["loss"])
    print("decide %s n=%d: loss %.6f err %.2e bound %.2e; matrix err / bound %.3f" % (name, n, d["loss"], err, d["loss_bound"], rm))
    assert err <= d["loss_bound"]


@pytest.mark.parametrize("n", ir.DECIDE_N)
def test_decide_on_random_logits_where_fp32_can_decide(ops, n):
    s = ir.decide_scene("random", n)
    d, idx, loss, _ = _decide(ops, s)
    for k in range(5):
        if d["decided"][k]:
            assert idx[k] == d["idx"][k], (k, idx, d["idx"])
    if d["decided"][0]:
        assert abs(loss - d["loss"]) <= d["loss_bound"]


@pytest.mark.parametrize("n", [2, 17])
def test_decide_refuses_what_it_has_no_room_for(ops, lib, n):
    z = lambda k: torch.zeros(k, device=DEV)
    with pytest.raises(lib.CmrError):
        ops.iter_decide(z(n ** 3), n, z(n), z(n), z(n), z(n), z(n))


# ---- iter_apply ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ir.APPLY_N)
def test_apply_moves_the_cloud_and_the_accumulated_pose(ops, N):
    M, pc, acc = ir.apply_inputs(N)
    got_pc, got_acc = ops.iter_apply(_d(M), _d(pc), _d(acc))
    want_pc, pb, want_acc, ab = ir.apply(M, pc, acc)
    e_pc, e_acc = np.abs(_np(got_pc) - want_pc), np.abs(_np(got_acc) - want_acc)
    print("apply N=%d: cloud err / bound %.3f, accumulated pose %.3f" % (N, _ratio(e_pc, pb), _ratio(e_acc, ab)))
    assert (e_pc <= pb).all() and (e_acc <= ab).all()
