"""Restatement of the sparse-observation rules (csrc/agent.hip obs_mark_reach, csrc/conv_wino.hip wino_tile_lists_kernel and the LIST
instantiation of the wave-specialised Winograd kernel), in numpy, from their DEFINITIONS -- not the code under test.

Tiles are the convolutions' 8 x 16 output tiles of an h x w map (ceil at the borders).  reach_r marks every tile whose area dilated by r
pixels holds an occupied cell; a convolution's list is the marked tiles in ascending order, then the others in ascending order, each
expanded to its cout / 64 virtual tiles (id = tile * nco + cout group)."""
import numpy as np

TH, TW = 8, 16


def tile_grid(h, w):
    return (h + TH - 1) // TH, (w + TW - 1) // TW


def reach_maps(cells, B, h, w):
    """cells: iterable of (b, y, x) occupied cells -> (reach1, reach2) uint8 [B, tiles_y, tiles_x], by the definition: tile (ty, tx) is
    marked in reach_r when its pixel rectangle grown by r on every side contains the cell (every tile is tested)."""
    ty, tx = tile_grid(h, w)
    out = [np.zeros((B, ty, tx), dtype=np.uint8) for _ in (1, 2)]
    for b, y, x in cells:
        for r, m in zip((1, 2), out):
            for j in range(ty):
                for i in range(tx):
                    if TH * j - r <= y < TH * j + TH + r and TW * i - r <= x < TW * i + TW + r:
                        m[b, j, i] = 1
    return out


def tile_lists(reach, nco):
    """reach uint8 [...] (any shape, flattened in C order = tile id) -> (order int32 [ntile * nco], nlive)."""
    flat = np.asarray(reach).reshape(-1) != 0
    ids = np.arange(flat.size)
    tiles = np.concatenate([ids[flat], ids[~flat]])
    order = (tiles[:, None] * nco + np.arange(nco)[None, :]).reshape(-1).astype(np.int32)
    return order, int(flat.sum()) * nco


def occupied(x_nhwc):
    """cells (b, y, x) of a map [B, h, w, C] that hold a non-zero value"""
    nz = np.asarray(x_nhwc != 0).any(axis=-1)
    return [tuple(int(v) for v in c) for c in np.argwhere(nz)]
