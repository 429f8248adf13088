"""Restatement of the rules of the sparse observation's SECOND stage (CMRAgent.SPARSE_OBS_STAGES = 2; csrc/agent.hip obs_mark_reach on the
half-resolution tile grid, csrc/conv_wino.hip wino_tile_lists_staged_kernel and the `nend` bound of the list launch), in numpy, from their
DEFINITIONS -- not the code under test.  sparse_obs_reference.py holds the first stage's.

Stage 1 convolves the 2 x 2 pooled output of stage 0 (h / 2 x w / 2) twice; its 8 x 16 tiles cover a 16 x 32 footprint of observation cells.
Tile (j, i) of its first / second convolution is marked when the footprint dilated by 4 / 6 cells holds an occupied cell.  The first
convolution of a stage writes only what the second one reads: its list is live | copy | rest, where "copy" are the unmarked tiles with a
tile marked for the SECOND convolution among the 3 x 3 tiles around them in the same sample."""
import numpy as np

TH, TW = 8, 16
R1 = (4, 6)                 # dilation of a stage-1 tile's footprint, first / second convolution, in observation cells


def stage1_grid(h, w):
    """tile grid of the pooled map (h // 2) x (w // 2)"""
    return (h // 2 + TH - 1) // TH, (w // 2 + TW - 1) // TW


def reach_maps_stage1(cells, B, h, w):
    """cells (b, y, x) -> (map a, map b) uint8 [B, ty, tx] by the rule as stated: 16 j - r <= y <= 16 j + 15 + r and
    32 i - r <= x <= 32 i + 31 + r with r = 4 / 6 (every tile is tested)."""
    ty, tx = stage1_grid(h, w)
    out = [np.zeros((B, ty, tx), dtype=np.uint8) for _ in R1]
    for b, y, x in cells:
        for r, m in zip(R1, out):
            for j in range(ty):
                for i in range(tx):
                    if 2 * TH * j - r <= y <= 2 * TH * j + 2 * TH - 1 + r and 2 * TW * i - r <= x <= 2 * TW * i + 2 * TW - 1 + r:
                        m[b, j, i] = 1
    return out


def dilate(m):
    """boolean [H, W] -> every pixel with a set pixel among its 3 x 3 neighbours (the support of a 3x3 convolution, clipped to the map)"""
    p = np.zeros((m.shape[0] + 2, m.shape[1] + 2), dtype=bool)
    p[1:-1, 1:-1] = m
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


def to_tiles(m):
    """boolean [H, W] -> uint8 [ceil(H / 8), ceil(W / 16)]: tiles that hold a set pixel"""
    H, W = m.shape
    ty, tx = (H + TH - 1) // TH, (W + TW - 1) // TW
    p = np.zeros((ty * TH, tx * TW), dtype=bool)
    p[:H, :W] = m
    return p.reshape(ty, TH, tx, TW).any(axis=(1, 3)).astype(np.uint8)


def reach_by_dilation(y, x, h, w):
    """the data flow itself, for one occupied cell: conv, conv, 2 x 2 pool, conv (map a), conv (map b) as boolean dependence, then the
    tiles that hold a dependent output pixel"""
    m = np.zeros((h, w), dtype=bool)
    m[y, x] = True
    m = dilate(dilate(m))
    q = m[:2 * (h // 2), :2 * (w // 2)].reshape(h // 2, 2, w // 2, 2).any(axis=(1, 3))
    a = dilate(q)
    return to_tiles(a), to_tiles(dilate(a))


def axis_flow(p, n, tile):
    """reach_by_dilation along one axis of n cells on its own -> (tiles of map a, of map b), boolean [ceil(n / 2 / tile)]"""
    m = np.zeros((1, n), dtype=bool)
    m[0, p] = True
    m = dilate(dilate(m))
    q = m[:, :2 * (n // 2)].reshape(1, n // 2, 2).any(axis=2)
    a = dilate(q)
    red = lambda v: np.pad(v[0], (0, -v.shape[1] % tile)).reshape(-1, tile).any(axis=1)
    return red(a), red(dilate(a))


def reach_by_dilation_separable(fy, fx):
    """fy, fx = axis_flow of the cell's row and column: every step of the flow (3-wide dilation, pairwise any-pool, reduction to tiles of
    8 / 16) turns a rectangle into a rectangle, so the 2-D result is the outer product of the two 1-D flows (checked against the 2-D flow
    where both are run).  An 88 x 304 map costs a few hundred array operations per cell in 2-D; this is what lets EVERY cell be tested."""
    return np.outer(fy[0], fx[0]).astype(np.uint8), np.outer(fy[1], fx[1]).astype(np.uint8)


def copy_class(ra, rb):
    """uint8 [B, ty, tx] maps of a stage's first / second convolution -> class of every tile of the FIRST: 1 live, 2 copy, 0 rest"""
    ra, rb = np.asarray(ra) != 0, np.asarray(rb) != 0
    B, ty, tx = rb.shape
    p = np.zeros((B, ty + 2, tx + 2), dtype=bool)
    p[:, 1:-1, 1:-1] = rb
    near = np.zeros_like(rb)
    for dy in range(3):
        for dx in range(3):
            near |= p[:, dy:dy + ty, dx:dx + tx]
    return np.where(ra, 1, np.where(near, 2, 0)).astype(np.uint8)


def three_part_list(ra, rb, nco):
    """-> (order int32 [ntile * nco], nlive, nend) of a stage's first convolution: live, copy, rest, each ascending, expanded to the
    nco virtual tiles of a tile (id = tile * nco + cout group); nlive / nend in virtual tiles"""
    cls = copy_class(ra, rb).reshape(-1)
    ids = np.arange(cls.size)
    tiles = np.concatenate([ids[cls == 1], ids[cls == 2], ids[cls == 0]])
    order = (tiles[:, None] * nco + np.arange(nco)[None, :]).reshape(-1).astype(np.int32)
    nlive = int((cls == 1).sum()) * nco
    return order, nlive, nlive + int((cls == 2).sum()) * nco


def tile_pixels(tile_map, H, W):
    """[B, ty, tx] -> [B, H, W]: every pixel gets its 8 x 16 tile's value"""
    return np.repeat(np.repeat(np.asarray(tile_map), TH, axis=1), TW, axis=2)[:, :H, :W]
