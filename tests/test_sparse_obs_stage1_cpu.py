"""CPU tier of the sparse observation's second stage (CMRAgent.SPARSE_OBS_STAGES = 2): the reach of a cell on the half-resolution tile
grid, which tiles of a stage's first convolution its second one reads, the three-part list, and -- in the fp32 Winograd arithmetic of
conv_reference.wino_fp32 -- that a skipped tile of either stage equals the tile of the run on an empty projection, bit for bit, through
all four convolutions and both pools.  tests/test_sparse_obs_cpu.py shows why one convolution can be skipped exactly."""
import numpy as np
import pytest

import conv_reference as R
import sparse_obs_reference as S
import sparse_obs_stage1_reference as S1


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _mark_by_clamped_shifts(y, x, h, w):
    """the rule as the observation kernel evaluates it: four stores at the clamped corners of the r-neighbourhood, tile = cell >> (4, 5)"""
    ty, tx = S1.stage1_grid(h, w)
    out = [np.zeros((ty, tx), dtype=np.uint8) for _ in S1.R1]
    for r, m in zip(S1.R1, out):
        ya, yb = max(y - r, 0) >> 4, min((y + r) >> 4, ty - 1)
        xa, xb = max(x - r, 0) >> 5, min((x + r) >> 5, tx - 1)
        for j in (ya, yb):
            for i in (xa, xb):
                m[j, i] = 1
    return out


@pytest.mark.parametrize("h,w", [(80, 320), (88, 304), (16, 32), (18, 34)])
def test_stage1_reach_rule_every_cell(h, w):
    """footprint dilated by 4 / 6 = the dependence of the two half-resolution convolutions' output tiles on the cell (mark, dilate,
    dilate, 2 x 2 any-pool, dilate, dilate, reduce to tiles) = the four corner stores, for every cell of the map on its own"""
    ty, tx = S1.stage1_grid(h, w)
    ys = np.arange(ty)[:, None, None, None] * 16
    xs = np.arange(tx)[None, :, None, None] * 32
    near = lambda p, n: p < 8 or p >= n - 8
    fy, fx = [S1.axis_flow(y, h, 8) for y in range(h)], [S1.axis_flow(x, w, 16) for x in range(w)]
    for y in range(h):
        for x in range(w):
            flow_a, flow_b = S1.reach_by_dilation_separable(fy[y], fx[x])
            if h * w <= 1024 or (near(y, h) or y % 9 == 0) and (near(x, w) or x % 17 == 0):
                # the 2-D flow itself: every cell of the small maps, the border bands and a lattice of the large ones
                full_a, full_b = S1.reach_by_dilation(y, x, h, w)
                assert np.array_equal(full_a, flow_a) and np.array_equal(full_b, flow_b), (y, x)
            rule = [((ys - r <= y) & (y <= ys + 15 + r) & (xs - r <= x) & (x <= xs + 31 + r))[:, :, 0, 0].astype(np.uint8) for r in S1.R1]
            got = _mark_by_clamped_shifts(y, x, h, w)
            assert np.array_equal(rule[0], flow_a) and np.array_equal(rule[1], flow_b), (y, x)
            assert np.array_equal(got[0], flow_a) and np.array_equal(got[1], flow_b), (y, x)


def test_stage1_reach_rule_as_stated_matches_the_helper():
    g = np.random.default_rng(5)
    for h, w in ((80, 320), (88, 304)):
        cells = [(int(g.integers(2)), int(g.integers(h)), int(g.integers(w))) for _ in range(12)]
        a, b = S1.reach_maps_stage1(cells, 2, h, w)
        wa, wb = np.zeros_like(a), np.zeros_like(b)
        for bb, y, x in cells:
            fa, fb = S1.reach_by_dilation(y, x, h, w)
            wa[bb] |= fa
            wb[bb] |= fb
        assert np.array_equal(a, wa) and np.array_equal(b, wb) and 0 < a.sum() <= b.sum() < b.size


@pytest.mark.parametrize("B,H,W", [(2, 40, 160), (2, 44, 152), (1, 9, 17), (3, 88, 304)])
def test_every_pixel_a_live_second_tile_reads_is_written_by_the_first(B, H, W):
    """the need rule: the 10 x 18 input window of every live tile of the second convolution lies in live or copy tiles of the first"""
    g = np.random.default_rng(9)
    ty, tx = S.tile_grid(H, W)
    for p in (0.0, 0.05, 0.3, 1.0):
        rb = (g.random((B, ty, tx)) < p).astype(np.uint8)
        ra = rb & (g.random((B, ty, tx)) < 0.5)                       # the first convolution's marks: a subset, as the smaller dilation gives
        cls = S1.copy_class(ra, rb)
        written = S1.tile_pixels(cls != 0, H, W)
        for b, j, i in np.argwhere(rb != 0):
            y0, y1 = max(8 * j - 1, 0), min(8 * j + 9, H)
            x0, x1 = max(16 * i - 1, 0), min(16 * i + 17, W)
            assert written[b, y0:y1, x0:x1].all(), (b, j, i)
        # ... and no more than that: a copy tile touches a live tile of the second convolution
        for b, j, i in np.argwhere(cls == 2):
            assert rb[b, max(j - 1, 0):j + 2, max(i - 1, 0):i + 2].any() and not ra[b, j, i]
        if p == 0.0:
            assert not cls.any()


def test_three_part_list_order_and_counts():
    g = np.random.default_rng(3)
    for nco in (1, 2, 4):
        for p in (0.0, 0.1, 0.4, 1.0):
            rb = (g.random((3, 6, 10)) < p).astype(np.uint8)
            ra = rb & (g.random((3, 6, 10)) < 0.6)
            order, nlive, nend = S1.three_part_list(ra, rb, nco)
            cls = S1.copy_class(ra, rb).reshape(-1)
            n = cls.size * nco
            assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(n))        # a permutation of every virtual tile
            assert nlive == int(ra.sum()) * nco and nend - nlive == int((cls == 2).sum()) * nco and nlive <= nend <= n
            parts = order[:nlive], order[nlive:nend], order[nend:]
            for part, c in zip(parts, (1, 2, 0)):
                assert np.all(np.diff(part) > 0) and np.all(cls[part // nco] == c)
            # the live part is the two-part list's (sparse_obs_reference.tile_lists); the second convolution's list is that list
            two, nl2 = S.tile_lists(ra, nco)
            assert nl2 == nlive and np.array_equal(two[:nlive], order[:nlive])
            if p == 1.0:
                assert nend == n
            if p == 0.0:
                assert nlive == 0 and nend == 0


def test_a_skipped_tile_of_either_stage_equals_the_tile_of_the_empty_run_through_four_convolutions():
    """conv 0 (+ residual), conv 1 (+ bias, pool), conv 2 (+ bias), conv 3 (+ bias, pool), LeakyReLU after each: every tile outside its
    convolution's map equals the tile of the run on an empty projection."""
    g = np.random.default_rng(7)
    B, h, w, c = 1, 48, 96, 8
    res = g.standard_normal((B, h, w, c)).astype(np.float32)
    ws = [g.standard_normal((c, c, 3, 3)).astype(np.float32) for _ in range(4)]
    bs = [g.standard_normal(c).astype(np.float32) for _ in range(4)]
    x = np.zeros((B, h, w, c), dtype=np.float32)
    pts = [(0, 0, 0), (0, 8, 26), (0, 16 + 19, 32 + 35), (0, 47, 5)]          # (35, 67): 4 below and 4 right of tile (1, 1)'s footprint; (8, 26): 6 left of (0, 1)'s
    for b, yy, xx in pts:
        x[b, yy, xx] = g.standard_normal(c).astype(np.float32)
    lrelu = lambda v: np.maximum(v, v * np.float32(0.01))
    pool = lambda a: a.reshape(a.shape[0], a.shape[1] // 2, 2, a.shape[2] // 2, 2, c).sum(axis=(2, 4)) * np.float32(0.25)

    def run(xin):
        a1 = lrelu(R.wino_fp32(xin, ws[0]).numpy() + res)
        a2 = pool(lrelu(R.wino_fp32(a1, ws[1]).numpy() + bs[1]))
        a3 = lrelu(R.wino_fp32(a2, ws[2]).numpy() + bs[2])
        a4 = pool(lrelu(R.wino_fp32(a3, ws[3]).numpy() + bs[3]))
        return a1, a2, a3, a4

    f, e = run(x), run(np.zeros_like(x))
    r1, r2 = S.reach_maps(pts, B, h, w)
    r3, r4 = S1.reach_maps_stage1(pts, B, h, w)
    assert 0 < r3.sum() < r4.sum() < r4.size and r3[0, 1, 1] and r4[0, 1, 1] and (r3[0, 0, 1], r4[0, 0, 1]) == (0, 1)
    for k, (m, th, tw) in enumerate(((r1, 8, 16), (r2, 4, 8), (r3, 8, 16), (r4, 4, 8))):
        for j in range(m.shape[1]):
            for i in range(m.shape[2]):
                t = (0, slice(th * j, th * j + th), slice(tw * i, tw * i + tw))
                assert m[0, j, i] or np.array_equal(_bits(f[k][t]), _bits(e[k][t])), (k, j, i)
    # the marks are no wider than needed on this scene: every marked tile of stage 1's first convolution differs from the empty run's
    for j in range(r3.shape[1]):
        for i in range(r3.shape[2]):
            t = (0, slice(8 * j, 8 * j + 8), slice(16 * i, 16 * i + 16))
            assert not r3[0, j, i] or not np.array_equal(f[2][t], e[2][t]), (j, i)
