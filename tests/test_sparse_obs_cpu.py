"""CPU tier of the sparse observation (CMRAgent.SPARSE_OBS): why skipping a convolution tile is exact, and the tile rules restated.

The F(2x2,3x3) evaluation of conv_reference.wino_fp32 is fp32 step for step as the kernels of csrc/conv_wino.hip are (input transform by
additions, products summed over the channels, output transform by additions).  In it an output pixel is a function of its own 3 x 3 input
support only, BIT FOR BIT: the rows and columns of B^T outside the support enter the sums as exact zeros.  So
  * where the support is empty the product is exactly 0, and
  * two inputs that agree on a pixel's support give that pixel the same bits whatever lies outside,
which is what lets cmr_conv3x3_wino_list_nhwc_f32 copy a tile from the result on an empty input.  Finite operands are the precondition
(0 x Inf is not 0); the last test shows that this is the only one."""
import numpy as np
import pytest
import torch

import conv_reference as R
import sparse_obs_reference as S


def _case(seed, B=1, H=20, W=36, cin=8, cout=8):
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, H, W, cin)).astype(np.float32)
    w = g.standard_normal((cout, cin, 3, 3)).astype(np.float32)
    return x, w


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_outputs_with_an_empty_support_are_exactly_zero(seed):
    x, w = _case(seed)
    y0, y1, x0, x1 = 5, 15, 9, 30                     # planted empty region (odd and even borders: both halves of a 2 x 2 output tile)
    x[:, y0:y1, x0:x1] = 0.0
    y = R.wino_fp32(x, w).numpy()
    inner = y[:, y0 + 1:y1 - 1, x0 + 1:x1 - 1]        # pixels whose 3 x 3 support lies in the region
    assert inner.size and not inner.any()
    # ... and it is tight: the ring of pixels whose support touches an occupied cell is not zero
    ring = y[:, y0:y1, x0:x1].copy()
    ring[:, 1:-1, 1:-1] = 1.0
    assert np.all(ring != 0)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_outputs_with_equal_supports_are_bitwise_equal(seed):
    x, w = _case(seed)
    g = np.random.default_rng(100 + seed)
    keep = np.zeros(x.shape[1:3], dtype=bool)
    keep[3:14, 7:27] = True                           # the two inputs agree here and differ everywhere else, by orders of magnitude
    other = (g.standard_normal(x.shape) * 1.0e3).astype(np.float32)
    x2 = np.where(keep[None, :, :, None], x, other)
    a, b = R.wino_fp32(x, w).numpy(), R.wino_fp32(x2, w).numpy()
    same = (slice(None), slice(4, 13), slice(8, 26))   # supports inside the common region
    assert np.array_equal(_bits(a[same]), _bits(b[same]))
    assert not np.array_equal(a[:, 3:14, 7:27], b[:, 3:14, 7:27])          # the border pixels of the region see the difference
    # the map on an EMPTY common region is what the list kernel copies from: same statement with zeros
    x3, x4 = x.copy(), x2.copy()
    x3[:, 3:14, 7:27] = 0.0
    x4[:, 3:14, 7:27] = 0.0
    a, b = R.wino_fp32(x3, w).numpy(), R.wino_fp32(x4, w).numpy()
    assert np.array_equal(_bits(a[same]), _bits(b[same])) and not a[same].any()


def test_a_skipped_tile_equals_the_tile_of_the_empty_run_through_two_convolutions():
    """conv 0 (+ residual, LeakyReLU) then conv 1 (+ bias, LeakyReLU, 2 x 2 pool): a conv-1 tile with no point within 2 pixels equals the
    tile of the run on an empty projection; conv-0 tiles with no point within 1 pixel likewise."""
    g = np.random.default_rng(7)
    B, h, w, c = 1, 24, 48, 8
    res = g.standard_normal((B, h, w, c)).astype(np.float32)
    w0 = g.standard_normal((c, c, 3, 3)).astype(np.float32)
    w1 = g.standard_normal((c, c, 3, 3)).astype(np.float32)
    b1 = g.standard_normal(c).astype(np.float32)
    x = np.zeros((B, h, w, c), dtype=np.float32)
    pts = [(0, 0, 0), (0, 9, 17), (0, 23, 47), (0, 13, 30)]         # (13, 30): 2 px under tile row 1's ... see the marks below
    for b, yy, xx in pts:
        x[b, yy, xx] = g.standard_normal(c).astype(np.float32)
    lrelu = lambda v: np.maximum(v, v * np.float32(0.01))

    def run(xin):
        a1 = lrelu(R.wino_fp32(xin, w0).numpy() + res)
        a2 = lrelu(R.wino_fp32(a1, w1).numpy() + b1)
        return a1, a2.reshape(B, h // 2, 2, w // 2, 2, c).sum(axis=(2, 4)) * np.float32(0.25)

    (f1, f2), (e1, e2) = run(x), run(np.zeros_like(x))
    r1, r2 = S.reach_maps(pts, B, h, w)
    assert 0 < r1.sum() < r2.sum() < r2.size
    for j in range(r1.shape[1]):
        for i in range(r1.shape[2]):
            t1 = (0, slice(8 * j, 8 * j + 8), slice(16 * i, 16 * i + 16))
            t2 = (0, slice(4 * j, 4 * j + 4), slice(8 * i, 8 * i + 8))
            assert r1[0, j, i] or np.array_equal(_bits(f1[t1]), _bits(e1[t1])), (j, i)
            assert r2[0, j, i] or np.array_equal(_bits(f2[t2]), _bits(e2[t2])), (j, i)
            assert not r1[0, j, i] or not np.array_equal(f1[t1], e1[t1])          # the marks are no wider than needed on this scene
    assert r1.sum() < r1.size


def _mark_by_clamped_shifts(cells, B, h, w):
    """the rule as the observation kernel evaluates it: four stores at the clamped corners of the r-neighbourhood"""
    ty, tx = S.tile_grid(h, w)
    out = [np.zeros((B, ty, tx), dtype=np.uint8) for _ in (1, 2)]
    for b, y, x in cells:
        for r, m in zip((1, 2), out):
            ya, yb = max(y - r, 0) >> 3, min((y + r) >> 3, ty - 1)
            xa, xb = max(x - r, 0) >> 4, min((x + r) >> 4, tx - 1)
            for j in (ya, yb):
                for i in (xa, xb):
                    m[b, j, i] = 1
    return out


@pytest.mark.parametrize("h,w", [(40, 160), (44, 152), (8, 16), (9, 17)])
def test_reach_rule_every_cell(h, w):
    """four corner stores = the definition (tile dilated by r holds the cell), for every cell of the map on its own"""
    for y in range(h):
        for x in range(w):
            want = S.reach_maps([(0, y, x)], 1, h, w)
            got = _mark_by_clamped_shifts([(0, y, x)], 1, h, w)
            assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]), (y, x)


def test_reach_rule_one_two_and_three_pixels_outside_a_tile_edge():
    h, w = 40, 160
    for axis in (0, 1):
        for side in (-1, 1):
            for d, (in1, in2) in {1: (1, 1), 2: (0, 1), 3: (0, 0)}.items():
                # target tile (2, 4): rows 16..23, columns 64..79
                y, x = 20, 70
                if axis == 0:
                    y = 16 - d if side < 0 else 23 + d
                else:
                    x = 64 - d if side < 0 else 79 + d
                r1, r2 = S.reach_maps([(0, y, x)], 1, h, w)
                assert (r1[0, 2, 4], r2[0, 2, 4]) == (in1, in2), (axis, side, d)


def test_list_order():
    g = np.random.default_rng(3)
    for nco in (1, 2, 4):
        for p in (0.0, 0.3, 1.0):
            reach = (g.random((3, 5, 10)) < p).astype(np.uint8)
            order, nlive = S.tile_lists(reach, nco)
            n = reach.size * nco
            assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(n))        # a permutation of every virtual tile
            assert nlive == int(reach.sum()) * nco
            live, rest = order[:nlive], order[nlive:]
            assert np.all(np.diff(live) > 0) and np.all(np.diff(rest) > 0)                     # ascending, both parts
            assert np.all(reach.reshape(-1)[live // nco] == 1) and np.all(reach.reshape(-1)[rest // nco] == 0)


def test_finite_weights_are_the_precondition():
    x, w = _case(4)
    x[:, 5:15, 9:30] = 0.0
    w[0, 0, 1, 1] = np.inf
    with np.errstate(invalid="ignore"):
        y = R.wino_fp32(x, w).numpy()
    assert np.isnan(y[0, 8, 16, 0]) and not y[0, 8, 16, 1:].any()          # 0 x Inf: the skipped value would differ, in that channel only
