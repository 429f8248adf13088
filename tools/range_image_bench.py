#!/usr/bin/env python3
"""ops.virtual_scan and ops.range_image (csrc/range_image.hip) at the sizes of a mapped block.

  * the whole ops.virtual_scan (tables, three launches of the image, one host read, the visible launch, the sort of the kept rows) of the
    synthetic map tools/voxel_map_bench.py builds -- ten scans of the 120 000-point scene at 0.1 m on a 4 x 3 lattice of patches, about
    457 000 voxels -- seen from the middle of the second row of patches under a turned pose, at 64 x 1024 and at 32 x 512;
  * ops.range_image alone on one raw scan of `--points` rows, no pose.

Beside each the same result in torch on the device: the pose as a matrix product, atan2 binning, scatter_reduce(amin) on the packed
(bits of d2) << 32 | row keys, and for the virtual scan a min-pool over the wrapped window and the same sort.  The torch job bins by
atan2, so rows on a cell edge may fall into the neighbouring cell: the share of cells with the same winner is printed, not asserted.

HIP events round each call, the median over `--repeats` after `--warmup`, the two jobs alternating.
python tools/range_image_bench.py [--points 120000] [--repeats 5] [--warmup 1] [--out profiles/range_image_bench.txt]"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cloud_prepare_reference as R  # noqa: E402
from cmr_agent_amd import ops  # noqa: E402

FIELD = dict(elev_lo=-0.4363, elev_hi=0.0524, min_range=1.0, max_range=80.0)
EMPTY = (1 << 63) - 1


def _times_ms(fns, repeats, warmup):
    """the median of each of `fns`, the calls alternating"""
    ms = [[] for _ in fns]
    for it in range(warmup + repeats):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[k].append(e0.elapsed_time(e1))
    return [statistics.median(m) for m in ms]


def torch_image(pts, pose, rows, cols, elev_lo, elev_hi, min_range, max_range):
    """-> (index int64 [rows, cols], -1 where empty; dist2 float32, +inf where empty) by atan2 binning and scatter_reduce(amin)"""
    p = pts if pose is None else pts @ pose[:3, :3].T + pose[:3, 3]
    x, y, z = p.unbind(1)
    r2 = x * x + y * y
    d2 = r2 + z * z
    row = torch.floor((torch.atan2(z, r2.sqrt()) - elev_lo) / (elev_hi - elev_lo) * rows)
    col = torch.floor(torch.remainder(torch.atan2(y, x), 2 * math.pi) / (2 * math.pi / cols)).clamp_(max=cols - 1)
    ok = torch.isfinite(p).all(1) & (d2 >= min_range * min_range) & (d2 < max_range * max_range) & (row >= 0) & (row < rows)
    key = (d2.view(torch.int32).to(torch.int64) << 32) | torch.arange(pts.shape[0], device=pts.device)
    cell = (row * cols + col).to(torch.int64)[ok]
    img = torch.full((rows * cols,), EMPTY, dtype=torch.int64, device=pts.device).scatter_reduce_(0, cell, key[ok], "amin")
    empty = img == EMPTY
    dist2 = torch.where(empty, torch.full((), float("inf"), device=pts.device), (img >> 32).to(torch.int32).view(torch.float32))
    return torch.where(empty, -1, img & 0xffffffff).reshape(rows, cols), dist2.reshape(rows, cols)


def torch_virtual_scan(pts, pose, rows, cols, radius=(1, 1), rel_tol=0.05, **field):
    index, dist2 = torch_image(pts, pose, rows, cols, **field)
    rr, rc = radius
    wide = torch.cat([dist2[:, cols - rc:], dist2, dist2[:, :rc]], 1) if rc else dist2
    wide = torch.nn.functional.pad(wide, (0, 0, rr, rr), value=float("inf"))
    m2 = -torch.nn.functional.max_pool2d(-wide[None, None], (2 * rr + 1, 2 * rc + 1), stride=1)[0, 0]
    visible = (index >= 0) & (dist2 <= m2 * float(np.float32((1.0 + rel_tol) ** 2)))
    return torch.sort(index[visible]).values, index, visible


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--extent", type=float, default=8192.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    scale = (args.points / 5400.0) ** 0.5
    step = 14.0 * scale

    def raw_of(seed):
        return torch.from_numpy(R.scene(seed, n=args.points - 640, scale=scale).copy()).to(dev)

    # ---- the map of tools/voxel_map_bench.py ----
    vmap = ops.voxel_map(R.VOXEL, (-args.extent / 2,) * 3, 1, dev)
    for k in range(10):
        raw = raw_of(11 if k == 0 else 12 + k)
        down = ops.voxel_downsample(raw[:, :3].contiguous(), raw[:, 3:4].contiguous(), voxel=R.VOXEL)
        vmap = ops.voxel_map_insert(vmap, down.points + torch.tensor([step * (k % 4), step * (k // 4), 0.0], device=dev), down.attr, stamp=k).map
    cloud = vmap.points.contiguous()
    yaw = 0.3                                                          # the sensor stands in the middle of patch 5, turned by 0.3 rad
    T = np.eye(4)
    T[:2, :2] = [[math.cos(yaw), -math.sin(yaw)], [math.sin(yaw), math.cos(yaw)]]
    T[:3, 3] = [step, step, 0.0]
    inv = np.eye(4)
    inv[:3, :3], inv[:3, 3] = T[:3, :3].T, -T[:3, :3].T @ T[:3, 3]
    pose = torch.from_numpy(inv.astype(np.float32)).to(dev)
    lines = ["a map of %d voxels (ten scans of %d raw points at %.2f m) seen from the middle of it, field %.1f to %.1f degrees, %g to %g m, "
             "window (1, 1), 5 %%" % (cloud.shape[0], args.points, R.VOXEL, math.degrees(FIELD["elev_lo"]), math.degrees(FIELD["elev_hi"]),
                                     FIELD["min_range"], FIELD["max_range"])]
    for rows, cols in ((64, 1024), (32, 512)):
        got = ops.virtual_scan(cloud, pose, rows, cols, **FIELD)
        ref_rows, ref_index, _ = torch_virtual_scan(cloud, pose, rows, cols, **FIELD)
        same = float((got.image.index.to(torch.int64) == ref_index).float().mean())
        both = np.intersect1d(got.rows.cpu().numpy(), ref_rows.cpu().numpy()).size
        hip_ms, torch_ms = _times_ms([lambda: ops.virtual_scan(cloud, pose, rows, cols, **FIELD),
                                      lambda: torch_virtual_scan(cloud, pose, rows, cols, **FIELD)], args.repeats, args.warmup)
        lines += ["%3d x %4d: ops.virtual_scan whole call %8.3f ms (binned %d, outside %d, kept %d rows);  the same in torch %8.3f ms:  x %.2f" % (
                      rows, cols, hip_ms, got.image.binned, got.image.outside, got.rows.shape[0], torch_ms, torch_ms / hip_ms),
                  "    kernel against torch: the same winner in %.4f of the cells, %d of %d kept rows in common (torch keeps %d)" % (
                      same, both, got.rows.shape[0], ref_rows.shape[0])]

    # ---- one raw scan ----
    scan = raw_of(12)[:, :3].contiguous()
    for rows, cols in ((64, 1024),):
        got = ops.range_image(scan, None, rows, cols, **FIELD)
        ref_index, _ = torch_image(scan, None, rows, cols, **FIELD)
        same = float((got.index.to(torch.int64) == ref_index).float().mean())
        hip_ms, torch_ms = _times_ms([lambda: ops.range_image(scan, None, rows, cols, **FIELD), lambda: torch_image(scan, None, rows, cols, **FIELD)],
                                     4 * args.repeats, args.warmup)
        lines += ["one scan of %d rows at %d x %d, no pose (binned %d, outside %d): ops.range_image whole call %.3f ms;  the same in torch %.3f ms:  "
                  "x %.2f;  the same winner in %.4f of the cells" % (scan.shape[0], rows, cols, got.binned, got.outside, hip_ms, torch_ms,
                                                                      torch_ms / hip_ms, same)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
