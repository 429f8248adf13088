#!/usr/bin/env python3
"""ops.voxel_map_rays (csrc/voxel_map_rays.hip): the scan of tools/voxel_map_bench.py -- the 120 000-point scene of seed 12
downsampled at 0.1 m, the sensor at the origin of its frame -- cast through the maps of that tool, about 50 000 and about 500 000 voxels
built by inserts of the same scene under other seeds (the first of them overlaps the scan, the later ones lie beside it).

HIP events round each call (its host read is inside), the median over `--repeats` after `--warmup`; beside it ops.voxel_map_insert of the
same scan into the same map, as the scale of the subsystem.  Below, the entry point alone (its two memsets, the walk, the count; no host
read) under either lookup of the A/B library, the two alternating: every key searched in the whole list, and the run of a (y, z) pair
found once and searched alone.  The steps and lookups of the scan are counted on the host from the result of a map that holds nothing.
python tools/voxel_map_rays_bench.py [--points 120000] [--repeats 9] [--warmup 2] [--out profiles/voxel_map_rays_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import cloud_prepare_reference as R  # noqa: E402
from cmr_agent_amd import _lib, ops  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--extent", type=float, default=8192.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.use_ab()
    dev = torch.device("cuda")
    scale = (args.points / 5400.0) ** 0.5
    origin = (-args.extent / 2,) * 3

    def scan_of(seed, dx=0.0, dy=0.0):
        raw = torch.from_numpy(R.scene(seed, n=args.points - 640, scale=scale).copy()).to(dev)
        down = ops.voxel_downsample(raw[:, :3].contiguous(), raw[:, 3:4].contiguous(), voxel=R.VOXEL)
        return down.points + torch.tensor([dx, dy, 0.0], device=dev), down.attr

    scan, refl = scan_of(12)
    N = scan.shape[0]
    step = 14.0 * scale
    cells = torch.floor((scan - torch.tensor(origin, device=dev)) / R.VOXEL) - torch.floor(-torch.tensor(origin, device=dev) / R.VOXEL)
    steps = cells.abs().sum(1)
    lines = ["one scan of %d rows (voxels of %.2f m of %d raw points) cast from the origin of its frame through a map on the grid of %.2f m from "
             "%.0f m; start_margin 2, end_margin 1, max_cells 4096; about %.0f steps a ray (median %.0f, longest %.0f), %.1f million in all" % (
                 N, R.VOXEL, args.points, R.VOXEL, origin[0], float(steps.mean()), float(steps.median()), float(steps.max()), float(steps.sum()) / 1e6)]
    vmap = ops.voxel_map(R.VOXEL, origin, 1, dev)
    inserted = 0
    for scans in (1, 10):
        while inserted < scans:
            k = inserted
            pts, att = scan_of(11 if k == 0 else 12 + k, step * (k % 4), step * (k // 4))
            vmap = ops.voxel_map_insert(vmap, pts, att, stamp=k).map
            inserted += 1
        M = vmap.keys.shape[0]
        one = ops.voxel_map_rays(vmap, scan)
        rays_ms, insert_ms = _times_ms([lambda: ops.voxel_map_rays(vmap, scan), lambda: ops.voxel_map_insert(vmap, scan, refl, stamp=99)],
                                       args.repeats, args.warmup)
        # the entry point alone, under either lookup
        out = [[torch.empty((M,), dtype=torch.int32, device=dev) for _ in range(2)] for _ in range(2)]
        counts = torch.empty((4,), dtype=torch.int64, device=dev)
        nb = lib.cmr_voxel_map_rays_workspace_bytes(N)
        ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def entry(runs):
            lib.cmr_set_voxel_map_rays_variant(runs)
            _lib.call("cmr_voxel_map_rays_f32", vmap.keys.data_ptr(), M, origin[0], origin[1], origin[2], R.VOXEL, scan.data_ptr(), 3, N, None, 2, 1,
                      4096, out[runs][0].data_ptr(), out[runs][1].data_ptr(), counts.data_ptr(), ws.data_ptr(), nb, stream)

        full_ms, runs_ms = _times_ms([lambda: entry(0), lambda: entry(1)], args.repeats, args.warmup)
        lib.cmr_set_voxel_map_rays_variant(0)                      # the library's own choice
        assert all(torch.equal(out[0][j], out[1][j]) and torch.equal(out[0][j], one[j]) for j in range(2))
        lines += ["map of %7d voxels: ops.voxel_map_rays whole call %8.3f ms (cast %d, long %d, outside %d; %d voxels crossed, %d crossings, %d "
                  "voxels hit);  ops.voxel_map_insert of the same scan %8.3f ms" % (
                      M, rays_ms, one.cast, one.long, one.outside, int((one.crossed > 0).sum()), int(one.crossed.sum()), int((one.hits > 0).sum()),
                      insert_ms),
                  "    cmr_voxel_map_rays_f32 alone, ms: every key in the whole list %.3f, the run of a (y, z) pair searched alone %.3f:  x %.2f" % (
                      full_ms, runs_ms, full_ms / runs_ms)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
