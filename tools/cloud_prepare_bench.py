#!/usr/bin/env python3
"""ops.voxel_downsample and ops.point_normals (csrc/cloud_prepare.hip) on a synthetic 120 000-point scan: the scene of
tests/cloud_prepare_reference.py stretched to a 56 m patch (ground, wall, pole, clutter, clump, far points), voxel 0.1 m, radius 0.6 m.

Per op the median over `--repeats` of a HIP-event time round the whole call (host read-backs included), and per C-ABI entry point the
median event time of the call alone (utils/workmodel.CallTimer) plus torch.sort's.  For the normals: the neighbour pairs accepted (sum of
count) and the candidate rows the search reads (the rows of the 27 cells round every query, counted on the host), as rates; the candidate
rate x 16 B is the bandwidth the kernel draws from L2 (the gathered float4 rows; 8 TB/s-class HBM holds the whole cloud many times over,
so the compulsory HBM traffic -- every array once -- is reported beside it).  The host baseline is scipy's cKDTree on the same cloud: build
+ query_ball_point, one thread, the SEARCH ONLY (no covariance, no eigen-solve).
python tools/cloud_prepare_bench.py [--points 120000] [--repeats 9] [--warmup 2] [--out profiles/cloud_prepare_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cloud_prepare_reference as R  # noqa: E402
from cmr_agent_amd import ops  # noqa: E402
from cmr_agent_amd.utils.workmodel import CallTimer  # noqa: E402

HBM_PEAK, L2_PEAK = 8.0e12, 17.0e12          # B/s: HBM3E peak; rows that every workgroup shares gather from the XCDs' L2 at 16.8 - 18.8 TB/s chip-wide


def _timed(fn, repeats, warmup):
    """-> (median ms of the whole call, {entry point: median ms})"""
    whole, per = [], {}
    for it in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with CallTimer() as t:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            whole.append(e0.elapsed_time(e1))
            for row in t.table():
                per.setdefault(row["name"], []).append(row["ms"])
    return statistics.median(whole), {k: statistics.median(v) for k, v in per.items()}


def _sort_ms(n, repeats, warmup, dev):
    keys = torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device=dev)
    ms = []
    for it in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.sort(keys, stable=True)
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def _candidates(cloud, radius):
    """Rows in the 27 cells round every row's own, summed over the rows (what a query of the grid search reads)."""
    keys, _, cells = R.voxel_keys(cloud, radius, origin=cloud.min(0))
    uniq, cnt = np.unique(keys, return_counts=True)
    total = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                c = cells + [dx, dy, dz]
                ok = (c >= 0).all(1)
                k = c[:, 2] << 42 | c[:, 1] << 21 | c[:, 0]
                pos = np.searchsorted(uniq, k)
                hit = ok & (pos < uniq.size) & (uniq[np.minimum(pos, uniq.size - 1)] == k)
                total += int(cnt[np.minimum(pos, uniq.size - 1)][hit].sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    scale = (args.points / 5400.0) ** 0.5
    raw = R.scene(11, n=args.points - 640, scale=scale)
    N = raw.shape[0]
    pts, refl = torch.from_numpy(raw[:, :3].copy()).to(dev), torch.from_numpy(raw[:, 3:4].copy()).to(dev)
    down = ops.voxel_downsample(pts, refl, voxel=R.VOXEL)
    cloud = down.points
    n = cloud.shape[0]
    nrm = ops.point_normals(cloud, radius=R.RADIUS)
    pairs = int(nrm.count.sum().item())
    cand = _candidates(cloud.cpu().numpy(), R.RADIUS)

    d_ms, d_per = _timed(lambda: ops.voxel_downsample(pts, refl, voxel=R.VOXEL), args.repeats, args.warmup)
    n_ms, n_per = _timed(lambda: ops.point_normals(cloud, radius=R.RADIUS), args.repeats, args.warmup)
    sort_N, sort_n = _sort_ms(N, args.repeats, args.warmup, dev), _sort_ms(n, args.repeats, args.warmup, dev)

    from scipy.spatial import cKDTree
    q = cloud.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    lists = cKDTree(q).query_ball_point(q, R.RADIUS, workers=1)
    host_s = time.perf_counter() - t0
    host_pairs = int(sum(len(l) for l in lists))

    k_ms = n_per["cmr_point_normals_f32"]
    hbm_bytes = n * (12 + 16 + 16 + 8 + 8 + 12 + 4)          # rows in, float4 out and in again, key, order, normal, count
    lines = ["synthetic scan: %d raw points -> %d voxels of %.2f m (%.1f %%), %d dropped; normals at radius %.2f m: %d neighbour pairs "
             "(%.1f per row, most %d), %d candidate rows read (%.1f per row)" % (
                 N, n, R.VOXEL, 100.0 * n / N, down.dropped, R.RADIUS, pairs, pairs / n, int(nrm.count.max().item()), cand, cand / n),
             "ops.voxel_downsample  whole call %8.3f ms   (bounds %.3f, keys %.3f, torch.sort ~%.3f, heads %.3f, means %.3f)" % (
                 d_ms, d_per["cmr_cloud_bounds_f32"], d_per["cmr_voxel_keys_f32"], sort_N, d_per["cmr_segment_heads_i64"],
                 d_per["cmr_segment_reduce_f32"]),
             "ops.point_normals     whole call %8.3f ms   (bounds %.3f, keys %.3f, torch.sort ~%.3f, gather + normals %.3f)" % (
                 n_ms, n_per["cmr_cloud_bounds_f32"], n_per["cmr_voxel_keys_f32"], sort_n, k_ms),
             "cmr_point_normals_f32: %.2f G accepted pairs/s, %.2f G candidate rows/s = %.3f TB/s of 16-byte rows from L2 (%.1f %% of a "
             "%.0f TB/s L2), compulsory HBM traffic %.2f MB = %.2f GB/s (%.3f %% of %.0f TB/s)" % (
                 pairs / k_ms * 1e-6, cand / k_ms * 1e-6, cand * 16.0 / k_ms * 1e-9, 100.0 * cand * 16.0 / (k_ms * 1e-3) / L2_PEAK,
                 L2_PEAK * 1e-12, hbm_bytes * 1e-6, hbm_bytes / k_ms * 1e-6, 100.0 * hbm_bytes / (k_ms * 1e-3) / HBM_PEAK, HBM_PEAK * 1e-12),
             "host baseline: scipy cKDTree build + query_ball_point (one thread, search only) %.1f ms, %d pairs; device normals whole call "
             "x %.0f faster" % (host_s * 1e3, host_pairs, host_s * 1e3 / n_ms)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
