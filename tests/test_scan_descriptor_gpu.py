"""GPU tier of place recognition between scans (ops.scan_descriptor / ops.scan_match, csrc/scan_descriptor.hip, dataset/loops.py;
DESIGN.md 4ak), against the restatement of scan_descriptor_reference.py.

Every comparison with the kernels is EXACT: descriptors and distances bit for bit, counts and shifts as integers -- the header states
every fp32 operation behind them.  Every case is run twice: the two calls agree bit for bit, and the inputs are what they were."""
import numpy as np
import pytest
import torch

import scan_descriptor_reference as D
from cmr_agent_amd import _lib, ops
from cmr_agent_amd.dataset import align, loops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
F = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)      # noqa: E731
ROWS = (1, 63, 64, 65, 255, 256, 257, 1025)                           # round the wave (64), a pass (256) and a workgroup's rows (1 024)
RS = ((1, 4), (3, 4), (2, 8), (8, 24), (20, 60), (64, 64), (16, 256))


def same_bits(t, ref):
    return np.array_equal(D.bits(t.cpu().numpy()), D.bits(ref))


def describe(pts, R, S, min_range=0.0, max_range=25.0, height=2.0):
    """One descriptor on both sides, compared.  -> the op's result"""
    p = F(pts)
    before = p.clone()
    got = ops.scan_descriptor(p, R, S, max_range, min_range, height)
    again = ops.scan_descriptor(p, R, S, max_range, min_range, height)
    ref, counts = D.describe(pts, R, S, min_range, max_range, height)
    assert got.desc.dtype == torch.float32 and tuple(got.desc.shape) == (R, S)
    assert tuple(got[1:]) == counts and sum(counts) == pts.shape[0], (tuple(got[1:]), counts)
    assert same_bits(got.desc, ref), np.argwhere(got.desc.cpu().numpy() != ref)[:8]
    assert torch.equal(got.desc, again.desc) and got[1:] == again[1:]
    assert torch.equal(p.view(torch.int32), before.view(torch.int32)), "the input was changed"
    return got


def scene(N, seed=1):
    """N rows within 30 m of the sensor (the descriptors reach 25), one of them no number from 16 rows on"""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.uniform(-30, 30, (1025, 2)), rng.uniform(-3, 6, (1025, 1))], 1).astype(F32)[:N]
    if N >= 16:
        pts[7, 1] = np.nan
    return pts


# ---- scan_descriptor -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ROWS)
def test_descriptor_sizes(N):
    pts = scene(N)
    for R, S in RS:
        got = describe(pts, R, S)
        assert got.dropped == (1 if N >= 16 else 0) and (N < 64 or (got.outside > 0 and got.binned > 0))
    describe(pts, 8, 24, min_range=3.0, max_range=22.5, height=0.25)


@pytest.mark.parametrize("last", (1023, 1024, 1025))
@pytest.mark.parametrize("R,S", ((1, 4), (2, 8), (3, 12), (16, 256)))
def test_descriptor_sector_where_it_is_decided(R, S, last):
    """The kernel bisects the sector; the restatement compared with it COUNTS, as the header states it.  The rows are D.planted(S) -- every
    table direction at three scales and one ulp round it, the axes, the origin, subnormal and 1e19 coordinates, in all four quadrants --
    standing above random filler, each with a z of its own that rises along the planted order, so that a planted row in a wrong sector
    shows wherever it is the largest of the cell it left or of the cell it reached.  The shapes: no table, one entry, an odd
    quarter, the largest quarter.  N = 1 023, 1 024 and 1 025 (for 256 sectors, whose planted rows alone are 3 824, 3 072 more): the last
    workgroup one row short of full, full, and one row past."""
    xy = D.planted(S)
    N = -(-len(xy) // 1024) * 1024 - 1024 + last
    rng = np.random.default_rng(S)
    fill = rng.uniform(-1, 1, (N - len(xy), 2)) * 2.0 ** rng.integers(-20, 21, (N - len(xy), 1))
    rising = 1.0 + 3.0 * np.arange(1, len(xy) + 1) / (len(xy) + 1)        # every planted row its own z: no two of them tie in a cell
    pts = np.concatenate([np.concatenate([xy, fill]), np.concatenate([rising, rng.uniform(-3, 1, len(fill))])[:, None]], 1)
    pts = pts.astype(F32)[rng.permutation(N)]
    got = describe(pts, R, S, max_range=2.0 ** 21)
    assert got.dropped == 0 and got.outside == 20 and got.desc[0].count_nonzero() == S      # outside: the five rows at 1e19 of each quadrant


def test_descriptor_rows_on_the_axes_the_origin_and_the_edges():
    pts = F32([[1, 0, 0], [0, 1, 1], [-1, 0, 2], [0, -1, 3], [0, 0, 5]])
    got = describe(pts, 3, 4, 0.0, 10.0, 0.5)
    assert got.desc[0].tolist() == [5.5, 1.5, 2.5, 3.5] and not got.desc[1:].any() and got[1:] == (5, 0, 0)
    for R, S in RS:                                                      # the axes, the diagonals, the origin with either zero
        rim = F32([[3, 0, 1], [0, 3, 1.5], [-3, 0, 2], [0, -3, 2.5], [2, 2, 3], [-2, 2, 3.5], [-2, -2, 4], [2, -2, 4.5], [0, 0, 5], [-0.0, 0, 6], [0, -0.0, 7],
                   [-0.0, -0.0, 8], [3, -0.0, 9], [-0.0, 3, 9.5]])
        describe(rim, R, S)
        # rows exactly on the sector edges of the first quadrant and their turns, as far as fp32 holds them
        k = np.arange(0, S)
        ang = k * 2 * np.pi / S
        describe(np.stack([7 * np.cos(ang), 7 * np.sin(ang), 1 + k / 256.0], 1).astype(F32), R, S)
    # rows exactly on ring edges: range 10 in 2 and 4 rings, radii 2.5, 5, 7.5 and 10 on an axis and as 3-4-5 triangles
    on = F32([[2.5, 0, 1], [0, 5, 1], [3, 4, 2], [-4, 3, 3], [7.5, 0, 1], [-4.5, -6, 2], [10, 0, 1], [6, 8, 1], [0, -10, 1], [np.nextafter(F32(10), F32(0)), 0, 4]])
    for R in (1, 2, 4):
        got = describe(on, R, 4, 0.0, 10.0)
        assert got.outside == 3 and got.binned == 7
    got = describe(on, 2, 8, 5.0, 10.0)                                 # an inner radius: its edge belongs to the first ring
    assert got.outside == 4 and got.binned == 6


def test_descriptor_rows_that_are_no_numbers_outside_and_below_the_ground():
    inf, nan = np.inf, np.nan
    bad = F32([[nan, 0, 0], [0, inf, 0], [0, 0, -inf], [nan, nan, nan], [1, 1, 1], [-inf, 1, 1], [2e19, 2e19, 1], [3e38, 0, 1], [1, 1, 3e38]])
    got = describe(bad, 8, 24, height=3e38)                             # z + height overflows: the cell holds +inf, as the restatement's
    assert got[1:] == (2, 5, 2) and torch.isinf(got.desc).sum() == 1
    far = scene(300) * F32([10, 10, 1]) + F32([400, 0, 0])
    got = describe(far, 8, 24)
    assert got.binned == 0 and got.outside == 299 and not got.desc.any()
    low = scene(300)
    low[:, 2] = -np.abs(low[:, 2]) - 2.0                                # z + height <= 0 everywhere: binned rows, an all-zero image
    got = describe(low, 8, 24)
    assert got.binned > 100 and not got.desc.any() and (got.desc.view(torch.int32) == 0).all()
    assert describe(F32([[1, 1, -2.0]]), 3, 4).desc.view(torch.int32).any().item() is False         # z + height = 0 exactly: +0


def test_descriptor_row_strides_and_shapes_not_served():
    pts = np.concatenate([scene(700), np.full((700, 1), 9e9, F32)], 1)                    # a fourth column that must not be read
    want = describe(pts[:, :3], 8, 24)
    p4 = F(pts)
    edge2, dirs = (torch.from_numpy(t).to(DEV) for t in ops.scan_tables(8, 24, 0.0, 25.0))
    desc, counts = torch.full((8, 24), -1.0, device=DEV), torch.full((3,), -1, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.call("cmr_scan_descriptor_f32", p4.data_ptr(), 4, 700, 8, 24, edge2.data_ptr(), dirs.data_ptr(), 2.0, desc.data_ptr(), counts.data_ptr(), stream)
    assert torch.equal(desc, want.desc) and tuple(counts.tolist()) == tuple(want[1:])
    for R, S in ((8, 22), (65, 4), (17, 256), (8, 2)):                   # no launch: the outputs are untouched
        rc = _lib.call("cmr_scan_descriptor_f32", p4.data_ptr(), 4, 700, R, S, edge2.data_ptr(), dirs.data_ptr(), 2.0, desc.data_ptr(),
                       counts.data_ptr(), stream, allow_unsupported=True)
        assert rc == _lib.UNSUPPORTED
    assert torch.equal(desc, want.desc)
    empty = ops.scan_descriptor(torch.zeros((0, 3), device=DEV), 3, 4)
    assert empty[1:] == (0, 0, 0) and not empty.desc.any()


# ---- scan_match ----------------------------------------------------------------------------------------------------------------------------------
def batch(n, R, S, seed, empty=0.2, sparse=0.3):
    """n descriptors: values in [0, 6), a share of their cells 0, a share of their columns empty"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0, 6, (n, R, S)) * (rng.uniform(size=(n, R, S)) >= sparse) * (rng.uniform(size=(n, 1, S)) >= empty)
    return d.astype(F32)


def match(q, c, limit=None, min_cols=None):
    """One match on both sides, compared.  -> the op's result"""
    tq, tc = F(q), F(c)
    tl = None if limit is None else torch.tensor(list(limit), dtype=torch.int32, device=DEV)
    before = (tq.clone(), tc.clone())
    got = ops.scan_match(tq, tc, tl, min_cols)
    again = ops.scan_match(tq, tc, tl, min_cols)
    dist, shift = D.match(q, c, limit, min_cols)
    assert got.dist.dtype == torch.float32 and got.shift.dtype == torch.int32 and tuple(got.dist.shape) == tuple(got.shift.shape) == (q.shape[0], c.shape[0])
    assert np.array_equal(got.shift.cpu().numpy(), shift), np.argwhere(got.shift.cpu().numpy() != shift)[:8]
    assert same_bits(got.dist, dist), np.argwhere(D.bits(got.dist.cpu().numpy()) != D.bits(dist))[:8]
    assert torch.equal(got.dist.view(torch.int32), again.dist.view(torch.int32)) and torch.equal(got.shift, again.shift)
    assert torch.equal(tq, before[0]) and torch.equal(tc, before[1]), "the inputs were changed"
    return got


@pytest.mark.parametrize("Q,N,R,S", [(q, n, r, s) for r, s in ((3, 4), (8, 24)) for q, n in ((1, 1), (3, 17), (17, 3), (65, 65))] +
                         [(5, 9, 20, 60), (5, 9, 64, 64), (2, 3, 16, 256), (3, 40, 1, 4), (9, 5, 2, 8)])
def test_match_sizes(Q, N, R, S):
    q, c = batch(Q, R, S, 10 + Q), batch(N, R, S, 20 + N)
    c[N // 2] = np.roll(q[Q // 2], 3 % S, 1)                            # one pair that is a roll of the other: distance ~ 0 at shift 3
    got = match(q, c)
    assert q[Q // 2].any(0).sum() < max(1, S // 4) or abs(got.dist[Q // 2, N // 2].item()) <= 2.0 ** -20
    match(q, c, limit=[(3 * i) % (N + 1) for i in range(Q)], min_cols=1)
    if Q == N:                                                          # the loop search's case: a batch against itself, earlier frames only
        got = match(q, q, limit=[max(0, i - 2) for i in range(Q)])
        assert torch.isnan(got.dist[:3]).all() and (got.shift[:3] == -1).all()


def test_match_empty_columns_and_min_cols():
    R, S = 3, 12
    q, c = batch(4, R, S, 1, 0.0, 0.0), batch(6, R, S, 2, 0.0, 0.0)
    c[:, :, 7:] = 0                                                     # candidate columns 0-6 only
    q[1, :, :8] = 0                                                     # query 1: columns 8-11 only
    q[2] = 0                                                            # query 2: nothing
    c[5] = 0                                                            # candidate 5: nothing
    for m in (1, 2, 3, 4, 5, 6, 7, 8, 12):                                # query 1 pairs at most 4 columns, the others 7
        got = match(q, c, min_cols=m)
        assert torch.isnan(got.dist[2]).all() and torch.isnan(got.dist[:, 5]).all() and (got.shift[2] == -1).all() and (got.shift[:, 5] == -1).all()
        assert bool(torch.isnan(got.dist[1, :5]).all()) == (m > 4) and bool(torch.isnan(got.dist[0, :5]).all()) == (m > 7)
    z = np.zeros((3, R, S), F32)
    got = match(z, z, min_cols=1)
    assert torch.isnan(got.dist).all() and (got.shift == -1).all()
    # equal distances go to the lowest shift: columns all the same, and a pattern of period 4 in 12 columns
    same = np.tile(batch(1, R, 1, 3, 0.0, 0.0), (1, 1, S))
    period = np.tile(batch(1, R, 4, 4, 0.0, 0.0), (1, 1, 3))
    assert match(same, same).shift.item() == 0
    assert match(period, np.roll(period, 1, 2)).shift.item() == 1


def test_match_limits_and_the_split_of_the_queries(monkeypatch):
    R, S, Q, N = 8, 24, 21, 19
    q, c = batch(Q, R, S, 5), batch(N, R, S, 6)
    free = match(q, c)
    for limit in ([0] * Q, [N] * Q, [i % (N + 1) for i in range(Q)], [N if i % 2 else 0 for i in range(Q)]):
        got = match(q, c, limit=limit)
        for i, lim in enumerate(limit):
            assert torch.isnan(got.dist[i, lim:]).all() and (got.shift[i, lim:] == -1).all()
            assert torch.equal(got.dist[i, :lim].view(torch.int32), free.dist[i, :lim].view(torch.int32)) and torch.equal(got.shift[i, :lim], free.shift[i, :lim])
    # one call's outputs under the budget: 8 N bytes per query, so 5 queries a call here, the last call a single one
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: calls.append(a[1]) or real(name, *a, **k))
    monkeypatch.setattr(ops, "SCAN_MATCH_CALL_BYTES", 8 * N * 5)
    limit = [i % (N + 1) for i in range(Q)]
    split = match(q, c, limit=limit)
    assert calls == [5, 5, 5, 5, 1] * 2
    monkeypatch.undo()
    whole = match(q, c, limit=limit)
    assert torch.equal(split.dist.view(torch.int32), whole.dist.view(torch.int32)) and torch.equal(split.shift, whole.shift)


# ---- the command -----------------------------------------------------------------------------------------------------------------------------------
def test_loops_command_finds_the_planted_revisits(tmp_path, capsys):
    """python -m cmr_agent_amd.dataset.loops on the synthetic drive: exactly the planted revisits, from the shift's heading and with auto.
    The descriptors and the match are the restatement's bit for bit, so the lines' distances and shifts are; the turned frames start within
    half a sector of the true heading (checked on the restatement by the CPU tier, and the shifts are the same).  The tolerance on the
    accepted poses is twice ICP's own error on the same pairs started from the truth (align.register_pair): measured 2026-10, see DESIGN.md 4ak."""
    d = D.drive(D.DRIVE_SEED)
    got = torch.stack([ops.scan_descriptor(F(f[:3].T), D.DRIVE["rings"], D.DRIVE["sectors"], D.DRIVE["max_range"], 0.0, D.DRIVE["height"]).desc
                       for f in d["frames"]])
    assert same_bits(got, D.drive_descriptors(D.DRIVE_SEED))
    rot, trans = D.drive_icp_error(lambda t, s, start: align.register_pair(t, s, align.device_pose(start)).pose.cpu().numpy().astype(np.float64))
    with capsys.disabled():
        print("ICP from the truth: rotation %.3e rad, translation %.3e m" % (rot, trans))
    root, out = str(tmp_path), str(tmp_path / "edges.txt")
    for init in ("shift", "auto"):
        loops.main(D.drive_argv(root, "--init", init, "--out", out))
        worst = D.check_drive_run(capsys.readouterr().out.splitlines(), ["shift"] * 4, 2 * rot, 2 * trans, out)
        with capsys.disabled():
            print("loop edges, --init %s: rotation %.3e rad, translation %.3e m" % ((init,) + worst))
