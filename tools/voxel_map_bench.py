#!/usr/bin/env python3
"""ops.voxel_map_insert (csrc/voxel_map.hip): one scan -- the source of tools/cloud_icp_bench.py, the 120 000-point scene of
seed 12 downsampled at 0.1 m -- inserted into maps of 0, about 50 000 and about 500 000 voxels.  The maps are built by inserts of the same
scene under other seeds, the later ones shifted along x and y so that they cover new ground; the timed scan overlaps the first of them.

HIP events round each call (its host reads are inside), the median over `--repeats` after `--warmup`; below each whole call the entry
points of one insert, timed one by one (utils/workmodel.CallTimer; the torch.sort of the keys is what is left).  Beside it the only other
route to the same keys: ops.voxel_downsample over the concatenated rows of every scan inserted so far and the new one, on the map's grid.
python tools/voxel_map_bench.py [--points 120000] [--repeats 9] [--warmup 2] [--out profiles/voxel_map_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import cloud_prepare_reference as R  # noqa: E402
from cmr_agent_amd import ops  # noqa: E402
from cmr_agent_amd.utils import workmodel  # noqa: E402


def _median_ms(fn, repeats, warmup):
    ms = []
    for it in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--extent", type=float, default=8192.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    scale = (args.points / 5400.0) ** 0.5
    origin = (-args.extent / 2,) * 3

    def scan_of(seed, dx=0.0, dy=0.0):
        raw = torch.from_numpy(R.scene(seed, n=args.points - 640, scale=scale).copy()).to(dev)
        down = ops.voxel_downsample(raw[:, :3].contiguous(), raw[:, 3:4].contiguous(), voxel=R.VOXEL)
        return down.points + torch.tensor([dx, dy, 0.0], device=dev), down.attr

    scan, refl = scan_of(12)
    step = 14.0 * scale                                               # the patch is 12 m x scale wide: shifted scans do not overlap
    lines = ["one scan of %d rows (voxels of %.2f m of %d raw points, one attribute) into a map on the grid of %.2f m from %.0f m" % (
        scan.shape[0], R.VOXEL, args.points, R.VOXEL, origin[0])]
    vmap = ops.voxel_map(R.VOXEL, origin, 1, dev)
    inserted = []
    for scans in (0, 1, 10):
        while len(inserted) < scans:
            k = len(inserted)
            pts, att = scan_of(11 if k == 0 else 12 + k, step * (k % 4), step * (k // 4))
            vmap = ops.voxel_map_insert(vmap, pts, att, stamp=k).map
            inserted.append(pts)
        one = ops.voxel_map_insert(vmap, scan, refl, stamp=99)
        insert_ms = _median_ms(lambda: ops.voxel_map_insert(vmap, scan, refl, stamp=99), args.repeats, args.warmup)
        with workmodel.CallTimer() as timer:
            ops.voxel_map_insert(vmap, scan, refl, stamp=99)
        torch.cuda.synchronize()
        parts = ", ".join("%s %.3f" % (d["name"].replace("cmr_", ""), d["ms"]) for d in timer.table())
        rows = torch.cat(inserted + [scan])
        down = ops.voxel_downsample(rows, voxel=R.VOXEL, origin=origin)
        assert down.points.shape[0] == one.map.keys.shape[0] and torch.equal(down.count, one.map.count)
        down_ms = _median_ms(lambda: ops.voxel_downsample(rows, voxel=R.VOXEL, origin=origin), args.repeats, args.warmup)
        lines += ["map of %7d voxels: ops.voxel_map_insert whole call %8.3f ms (new %d, merged %d -> %d voxels);  ops.voxel_downsample of the "
                  "%d concatenated rows %8.3f ms (no attribute, no counts kept, no stamps):  insert x %.2f" % (
                      vmap.keys.shape[0], insert_ms, one.new, one.merged, one.map.keys.shape[0], rows.shape[0], down_ms, down_ms / insert_ms),
                  "    entry points of one insert, ms: " + parts]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
