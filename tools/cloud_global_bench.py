#!/usr/bin/env python3
"""ops.point_fpfh, ops.descriptor_nearest, ops.ransac_rigid and ops.register_global (csrc/cloud_fpfh.hip, csrc/cloud_global.hip, DESIGN.md
4af) on the two synthetic 120 000-point scans of tools/cloud_icp_bench.py: seeds 11 (target) and 12 (source), each downsampled at 0.1 m, the
normals of both at 0.6 m; the source moved by the inverse of the far pose of tests/cloud_global_reference.py, which no ICP recovers.

HIP events round each call, the median over `--repeats` after `--warmup`; ransac_rigid and register_global include their host read.  The
host baseline, one thread: the same steps with scipy's cKDTree for the two searches (neighbour pairs within the radius; the nearest
descriptor in 33 dimensions, one way) and the restatement of tests/cloud_global_reference.py for the pair features, the second stage and
RANSAC.
python tools/cloud_global_bench.py [--points 120000] [--repeats 9] [--warmup 2] [--out profiles/cloud_global_bench.txt]"""
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

import cloud_global_reference as G  # noqa: E402
import cloud_icp_reference as RI  # noqa: E402
import cloud_prepare_reference as R  # noqa: E402
from cmr_agent_amd import ops  # noqa: E402

FP32_VECTOR_PEAK = 157.3e12          # FLOP/s, MI355X vector fp32 with every operation an fma; an unfused operation counts one


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


def host_fpfh(points, normals, radius):
    """The restatement's two stages on scipy's neighbour pairs (float64 distances: a pair on the radius may differ from the kernel's)"""
    from scipy.spatial import cKDTree
    p, n = points.astype(np.float32), normals.astype(np.float32)
    part = G.takes_part(p, n)
    rows = np.nonzero(part)[0]
    und = cKDTree(p[rows].astype(np.float64)).query_pairs(radius, output_type="ndarray")
    i = rows[np.concatenate([und[:, 0], und[:, 1]])]
    j = rows[np.concatenate([und[:, 1], und[:, 0]])]
    N = p.shape[0]
    hist = np.zeros((N, G.DIM), dtype=np.int64)
    d2 = np.zeros(i.size, np.float32)
    for lo in range(0, i.size, 1 << 20):
        a, b = i[lo:lo + (1 << 20)], j[lo:lo + (1 << 20)]
        f = G.pair_features(p[a], n[a], p[b], n[b])
        u = f["used"]
        for g, x in enumerate((f["x1"], (f["f2"] + 1.0) / 2.0, (f["f3"] + 1.0) / 2.0)):
            np.add.at(hist, (a[u], g * G.BINS + G.bins_of(x[u])), 1)
        d = p[b] - p[a]
        d2[lo:lo + (1 << 20)] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    count = np.bincount(i, minlength=N)
    return G.fpfh_stage(hist, count, (i, j, d2), N)["fpfh32"], count, i.size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--radius", type=float, default=G.RADIUS)
    ap.add_argument("--hyp", type=int, default=4096)
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline (minutes)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    scale = (args.points / 5400.0) ** 0.5
    clouds = []
    for seed in (11, 12):
        raw = torch.from_numpy(R.scene(seed, n=args.points - 640, scale=scale)[:, :3].copy()).to(dev)
        clouds.append(ops.voxel_downsample(raw, voxel=R.VOXEL).points)
    target = clouds[0]
    tn = ops.point_normals(target, radius=R.RADIUS).normals
    truth = RI.pose_matrix(*G.FAR_POSE)
    sn0 = ops.point_normals(clouds[1], radius=R.RADIUS).normals
    source = torch.from_numpy(RI.moved(clouds[1].cpu().numpy(), truth)).to(dev)
    sn = torch.from_numpy(G.moved_normals(sn0.cpu().numpy(), truth)).to(dev)
    rad = args.radius

    fs, ft = ops.point_fpfh(source, sn, rad), ops.point_fpfh(target, tn, rad)
    sm, tm = fs.count > 0, ft.count > 0
    fwd = ops.descriptor_nearest(fs.fpfh, ft.fpfh, sm, tm)
    back = ops.descriptor_nearest(ft.fpfh, fs.fpfh, tm, sm)
    keep = (fwd.idx >= 0) & (back.idx[fwd.idx.clamp(min=0).long()] == torch.arange(source.shape[0], dtype=torch.int32, device=dev))
    rows = torch.nonzero(keep).reshape(-1)
    corr = torch.stack([rows.to(torch.int32), fwd.idx[rows]], 1).contiguous()
    rr = ops.ransac_rigid(source, target, corr, n_hyp=args.hyp)
    rot0, trans0 = RI.pose_error(rr.pose.cpu().numpy(), truth)
    res = ops.register_global(source, sn, target, tn, radius=rad, n_hyp=args.hyp)
    rot, trans = RI.pose_error(res.pose.cpu().numpy(), truth)
    alone = ops.icp_point_to_plane(source, target, tn, max_dist=1.0, huber=0.1)
    rot_a, trans_a = RI.pose_error(alone.pose.cpu().numpy(), truth)
    pairs_s, pairs_t = int(fs.count.sum().item()), int(ft.count.sum().item())

    t = lambda fn: _median_ms(fn, args.repeats, args.warmup)      # noqa: E731
    index_t = ops.cloud_index(target, rad)
    fpfh_s = t(lambda: ops.point_fpfh(source, sn, rad))
    fpfh_t = t(lambda: ops.point_fpfh(target, tn, rad))
    fpfh_k = t(lambda: ops.point_fpfh(target, tn, rad, index_t))
    near_f = t(lambda: ops.descriptor_nearest(fs.fpfh, ft.fpfh, sm, tm))
    near_b = t(lambda: ops.descriptor_nearest(ft.fpfh, fs.fpfh, tm, sm))
    ransac = t(lambda: ops.ransac_rigid(source, target, corr, n_hyp=args.hyp))
    whole = t(lambda: ops.register_global(source, sn, target, tn, radius=rad, n_hyp=args.hyp))
    coarse = t(lambda: ops.register_global(source, sn, target, tn, radius=rad, n_hyp=args.hyp, refine=False))
    M, N = int(sm.sum().item()), int(tm.sum().item())
    sweep_flop = 3.0 * M * N * 33

    lines = ["synthetic scans: target %d rows, source %d rows (voxels of %.2f m of %d raw points each), FPFH radius %.2f m: %d and %d "
             "neighbour pairs; %d mutual correspondences; source moved by the inverse of the far pose" % (
                 target.shape[0], source.shape[0], R.VOXEL, args.points, rad, pairs_t, pairs_s, corr.shape[0]),
             "ops.icp_point_to_plane alone, from the identity: status %d, %.3f rad and %.3f m from the true pose" % (alone.status, rot_a, trans_a),
             "ops.point_fpfh         target %8.3f ms  (index built inside; %.3f ms on a prebuilt index = %.2f G pairs/s over both launches)   "
             "source %8.3f ms" % (fpfh_t, fpfh_k, 2 * pairs_t / fpfh_k * 1e-6, fpfh_s),
             "ops.descriptor_nearest source -> target %8.3f ms   target -> source %8.3f ms   (%d x %d selected rows x 33 channels: %.2f "
             "TFLOP/s of unfused fp32 operations = %.3f of the vector fp32 peak counted in fma FLOP)" % (
                 near_f, near_b, M, N, sweep_flop / near_f * 1e-9, sweep_flop / (near_f * 1e-3) / FP32_VECTOR_PEAK),
             "ops.ransac_rigid       %8.3f ms  (%d hypotheses x %d correspondences, host read included): %d inliers, status %d, %.4f rad "
             "and %.4f m from the true pose" % (ransac, args.hyp, corr.shape[0], rr.inliers, rr.status, rot0, trans0),
             "ops.register_global    %8.3f ms without the polish, %8.3f ms whole (ICP: %d iterations, status %d): %.2e rad and %.2e m from "
             "the true pose" % (coarse, whole, res.icp.iterations if res.icp else 0, res.icp.status if res.icp else -1, rot, trans),
             "share of the whole call: point_fpfh %.2f, descriptor_nearest %.2f, ransac_rigid %.2f" % (
                 (fpfh_s + fpfh_t) / whole, (near_f + near_b) / whole, ransac / whole)]
    if not args.no_host:
        from scipy.spatial import cKDTree
        t0 = time.perf_counter()
        host_ft, _, host_pairs = host_fpfh(target.cpu().numpy(), tn.cpu().numpy(), rad)
        h_fpfh = (time.perf_counter() - t0) * 1e3
        q, c = fs.fpfh.cpu().numpy()[sm.cpu().numpy()].astype(np.float64), host_ft[tm.cpu().numpy()].astype(np.float64)
        t0 = time.perf_counter()
        cKDTree(c).query(q, k=1, workers=1)
        h_near = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        h = G.ransac(source.cpu().numpy(), target.cpu().numpy(), corr.cpu().numpy(), args.hyp)
        h_ransac = (time.perf_counter() - t0) * 1e3
        lines.append("host baseline, one thread: FPFH of the target (scipy query_pairs, %d pairs, + the restatement's two stages) %.0f ms = x %.0f "
                     "the device's; nearest descriptor one way (scipy cKDTree in 33-D) %.0f ms = x %.0f; RANSAC (the restatement, numpy SVD, "
                     "%d inliers) %.0f ms = x %.0f" % (host_pairs, h_fpfh, h_fpfh / fpfh_t, h_near, h_near / near_f, h["inliers"], h_ransac,
                                                      h_ransac / ransac))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
