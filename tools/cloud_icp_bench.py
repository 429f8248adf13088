#!/usr/bin/env python3
"""ops.cloud_index, ops.cloud_nearest and ops.icp_point_to_plane (csrc/cloud_icp.hip) on two synthetic 120 000-point scans:
the scene of tests/cloud_prepare_reference.py stretched as in tools/cloud_prepare_bench.py, seeds 11 (target) and 12 (source), each
downsampled at 0.1 m; the target's normals at 0.6 m; the source moved by the inverse of the first true pose of tests/cloud_icp_reference.py.

HIP events round each call, the median over `--repeats` after `--warmup`.  ICP is timed three ways: with tolerances of 0 at 10 and at 30
iterations on a prebuilt index -- the difference / 20 is the time of one iteration, matching and sums and step, free of the call's fixed
cost -- and as the default call (index built inside, Huber 0.1, stops when converged; the host read of status and trace is inside the
events).  The host baseline, the only one available, is scipy's cKDTree on the same rows: build + query(k=1, distance_upper_bound), one
thread, the SEARCH of one iteration only (no sums, no solve).
python tools/cloud_icp_bench.py [--points 120000] [--repeats 9] [--warmup 2] [--out profiles/cloud_icp_bench.txt]"""
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

import cloud_icp_reference as RI  # noqa: E402
import cloud_prepare_reference as R  # noqa: E402
from cmr_agent_amd import ops  # noqa: E402


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
    ap.add_argument("--max-dist", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    scale = (args.points / 5400.0) ** 0.5
    clouds = []
    for seed in (11, 12):
        raw = torch.from_numpy(R.scene(seed, n=args.points - 640, scale=scale)[:, :3].copy()).to(dev)
        clouds.append(ops.voxel_downsample(raw, voxel=R.VOXEL).points)
    target = clouds[0]
    normals = ops.point_normals(target, radius=R.RADIUS).normals
    truth = RI.pose_matrix(*RI.TRUE_POSES[0])
    source = torch.from_numpy(RI.moved(clouds[1].cpu().numpy(), truth)).to(dev)
    md = args.max_dist
    index = ops.cloud_index(target, md)
    near = ops.cloud_nearest(index, source, md)
    matched = int((near.idx >= 0).sum().item())
    res = ops.icp_point_to_plane(source, target, normals, max_dist=md, huber=0.1)
    rot, trans = RI.pose_error(res.pose.cpu().numpy(), truth)

    t = lambda fn: _median_ms(fn, args.repeats, args.warmup)      # noqa: E731
    index_ms = t(lambda: ops.cloud_index(target, md))
    near_ms = t(lambda: ops.cloud_nearest(index, source, md))
    fixed = {k: t(lambda: ops.icp_point_to_plane(source, None, normals, max_dist=md, huber=0.1, iters=k, tol_rot=0.0, tol_trans=0.0, index=index))
             for k in (10, 30)}
    call_ms = t(lambda: ops.icp_point_to_plane(source, target, normals, max_dist=md, huber=0.1))
    iter_ms = (fixed[30] - fixed[10]) / 20.0

    from scipy.spatial import cKDTree
    c64, q64 = target.cpu().numpy().astype(np.float64), source.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    dist, _ = cKDTree(c64).query(q64, k=1, distance_upper_bound=md, workers=1)
    host_ms = (time.perf_counter() - t0) * 1e3
    host_matched = int(np.isfinite(dist).sum())

    lines = ["synthetic scans: target %d rows, source %d rows (voxels of %.2f m of %d raw points each), max_dist = cell = %.2f m: %d source "
             "rows have a target row within it before registration (host, float64: %d)" % (
                 target.shape[0], source.shape[0], R.VOXEL, args.points, md, matched, host_matched),
             "ops.cloud_index        whole call %8.3f ms   (bounds and their host read, keys, torch.sort, gather)" % index_ms,
             "ops.cloud_nearest      whole call %8.3f ms   = %.2f G queries/s" % (near_ms, source.shape[0] / near_ms * 1e-6),
             "ops.icp_point_to_plane %8.3f ms per iteration (match + float64 sums + step; (30 iterations %.3f ms - 10 iterations %.3f ms) / 20, "
             "tolerances 0, prebuilt index)" % (iter_ms, fixed[30], fixed[10]),
             "ops.icp_point_to_plane whole call %8.3f ms   (index built inside, Huber 0.1, from the identity: %d iterations, status %d, %d pairs, "
             "rmse %.4f m, %.2e rad and %.2e m from the true pose)" % (call_ms, res.iterations, res.status, res.pairs, res.rmse, rot, trans),
             "host baseline: scipy cKDTree build + query(k=1, distance_upper_bound) (one thread, the search of ONE iteration only) %.1f ms; "
             "device search x %.0f faster, a whole device iteration x %.0f faster than the host's search" % (
                 host_ms, host_ms / near_ms, host_ms / iter_ms)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
