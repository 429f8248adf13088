#!/usr/bin/env python3
"""ops.render_surfels beside the nearest call that existed before it, ops.render_points(splat=4): HIP events after
warm-up, the two timed alternately in the same process, `--repeats` times `--iters` calls: medians, and the largest |repeat - median| /
median over both sides as the spread.  A record, not a bar: the surfel op intersects a ray with a plane for every pixel of every
footprint, the square splat does not, and no ratio is required.  ops.depth_test is timed beside ops.visibility(radius=1) the same way.

Shapes: B = 8, N = 16384, ~40 % of the rows selected, maps 88 x 304 and 352 x 1216 (scenes: visibility_reference.scene), default
parameters (radius 0.1, range_slope 0.004, max_px 8, min_cos 0.1), random normals with ~10 % zero rows.  Beside the times: drawn rows,
owned pixels, and the nominal footprint radius f r / z_c in pixels (mean and largest over the drawn rows, from the op's `surfel` output).
python tools/surfel_bench.py [--iters 200] [--warmup 3] [--repeats 5] [--out profiles/surfel_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import visibility_reference as vr  # noqa: E402
from cmr_agent_amd import ops  # noqa: E402

SHAPES = [(8, 16384, 88, 304), (8, 16384, 352, 1216)]


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters                                  # us


def _alternate(calls, warmup, repeats, iters):
    """calls: [(name, fn)] -> ({name: median us}, spread)."""
    for _, fn in calls:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name, _ in calls}
    for _ in range(repeats):
        for name, fn in calls:
            t[name].append(_time(fn, iters))
    med = {k: statistics.median(v) for k, v in t.items()}
    return med, max(abs(x - med[k]) / med[k] for k, v in t.items() for x in v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    lines = ["%-24s | %10s %12s %7s | %10s %12s %7s | %6s | %s" % ("shape B x N, h x w", "surfels us", "splat=4 us", "ratio", "depth_test", "visibility",
                                                                   "ratio", "spread", "selected, drawn, owned pixels (splat=4: owned); f r / z_c mean, largest")]
    for B, N, h, w in SHAPES:
        sc = vr.scene(B, N, h, w, seed=41, selected=0.4)
        pts, pose, K, mask = f(sc["pts"]), f(sc["pose"]), f(sc["K"]), sc["mask"].to(dev)
        rng = np.random.default_rng(43)
        nrm = rng.normal(size=(B, 3, N))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        nrm[np.broadcast_to(rng.random((B, 1, N)) < 0.1, nrm.shape)] = 0.0
        nrm = f(nrm)
        surfels = lambda: ops.render_surfels(pts, nrm, pose, K, h, w, mask=mask)
        splat = lambda: ops.render_points(pts, pose, K, h, w, mask=mask, splat=4)
        _, dmap, _, counts, _, s = ops.render_surfels(pts, nrm, pose, K, h, w, mask=mask, want_surfel=True)
        test = lambda: ops.depth_test(pts, pose, K, dmap, mask, radius=0)
        vis = lambda: ops.visibility(pts, pose, K, h, w, mask, radius=1)
        med, spread = _alternate([("surfels", surfels), ("splat", splat), ("test", test), ("vis", vis)], args.warmup, args.repeats, args.iters)
        drawn = s[:, 7] == 1
        px = (K[:, 0, 0:1] * s[:, 6] / s[:, 2])[drawn]
        c = counts.sum(0).tolist()
        lines.append("%-24s | %10.1f %12.1f %7.2f | %10.1f %12.1f %7.2f | %5.1f%% | %d, %d, %d (%d); %.2f, %.2f" % (
            "%d x %d, %d x %d" % (B, N, h, w), med["surfels"], med["splat"], med["surfels"] / med["splat"], med["test"], med["vis"],
            med["test"] / med["vis"], 100.0 * spread, c[0], c[1], c[2], int(splat()[3][:, 2].sum()), float(px.mean()), float(px.max())))
    lines.append("surfels = one ops.render_surfels call at the default parameters; splat=4 = one ops.render_points(splat=4) call on the same rows; "
                 "depth_test = ops.depth_test(radius=0) against the surfel map; visibility = ops.visibility(radius=1); ratio = new / old; spread = "
                 "largest |repeat - median| / median over the four; wall times of whole calls (three or two launches and the allocation of the "
                 "outputs), not per-kernel device times: those and the counters were not measured")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
