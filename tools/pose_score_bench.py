#!/usr/bin/env python3
"""The call of DESIGN.md 4q against what stood in its place: HIP events after warm-up, the two sides timed alternately in the same process,
`--repeats` times: medians, and the largest |repeat - median| / median over both sides as the spread.

single: one ops.pose_score (cmr_pose_score_f32) call scoring P poses per sample.
loop:   P x (ops.guided_match(radius, want_dist=True) + the contract's reduction in torch float64) -- what the parent commit offers for the
        same numbers: 3 launches and a [B*N] dist vector per pose, the N x 64 point features read again for every pose.
Shapes: 88 x 304 and 40 x 128 maps, B = 8, N = 16384 with ~40 % of the rows selected, P in {1, 27, 729}, radius in {0, 1, 4}.  Geometry:
pnp_reference.planted; features: random unit vectors (the time does not depend on their values); poses: the truth turned by 0.5 deg
about a random axis and moved by 0.05 N(0, I), a fresh draw per pose.  "gather TB/s" counts (2r + 1)^2 pixel rows of 256 B per in-view
(row, pose) of the single call, shared or not.
python tools/pose_score_bench.py [--iters 10] [--warmup 2] [--repeats 5] [--out profiles/pose_score_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import guided_reference as gref  # noqa: E402
import pnp_reference as pref  # noqa: E402
from cmr_agent_amd import ops  # noqa: E402

SHAPES = [(8, 16384, 88, 304), (8, 16384, 40, 128)]
POSES = (1, 27, 729)
RADII = (0, 1, 4)
TAU = 0.8


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters                                  # us


def _alternate(calls, warmup, repeats):
    """calls: [(name, fn, iters)] -> ({name: median us}, spread)."""
    for _, fn, _ in calls:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name, _, _ in calls}
    for _ in range(repeats):
        for name, fn, iters in calls:
            t[name].append(_time(fn, iters))
    med = {k: statistics.median(v) for k, v in t.items()}
    return med, max(abs(x - med[k]) / med[k] for k, v in t.items() for x in v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    g = torch.Generator(device="cpu").manual_seed(7)
    lines = ["%-22s %4s %2s | %10s %12s %8s | %11s | %6s | %s" % ("shape B x N, h x w", "P", "r", "single us", "loop us", "loop / 1", "gather TB/s",
                                                               "spread", "selected, in view per pose")]
    for B, N, h, w in SHAPES:
        s = pref.planted(B, N, h, w, seed=31, kind="yaw")
        pts, K = f(s["pts"]), f(s["K"])
        pc = torch.nn.functional.normalize(torch.randn(B * N, 64, generator=g), dim=1).to(dev)
        img = torch.nn.functional.normalize(torch.randn(B, h, w, 64, generator=g), dim=3).to(dev)
        mask = (torch.rand(B, N, generator=g) < 0.4).to(dev)
        rng = np.random.default_rng(5)
        allp = f(np.stack([gref.perturbed(s["P"], rng, 0.5, 0.05) for _ in range(max(POSES))], 1))
        t32 = torch.tensor(TAU, dtype=torch.float32, device=dev)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        for P in POSES:
            poses = allp[:, :P].contiguous()
            each = [poses[:, p].contiguous() for p in range(P)]
            for r in RADII:
                def loop():
                    out = []
                    for p in range(P):
                        idx, _, _, d, _ = ops.guided_match(pts, pc, img, mask, each[p], K, r, want_dist=True)
                        dd = torch.where(idx.view(B, N) >= 0, torch.minimum(d.view(B, N), t32), t32).double()
                        out.append(torch.where(mask, dd * dd, zero).sum(1))
                    return torch.stack(out, 1)

                single = lambda: ops.pose_score(pts, pc, img, mask, poses, K, radius=r, tau=TAU)
                score, counts, selected = single()
                dev_err = float(((score - loop()).abs() / score.clamp(min=1.0)).max())
                assert dev_err <= 1e-10, dev_err                              # the two sides compute the same numbers
                med, spread = _alternate([("single", single, args.iters), ("loop", loop, max(1, args.iters // P))], args.warmup, args.repeats)
                nview = int(counts[..., 0].sum())
                lines.append("%-22s %4d %2d | %10.1f %12.1f %8.2f | %11.3f | %5.1f%% | %d, %d" % (
                    "%d x %d, %d x %d" % (B, N, h, w), P, r, med["single"], med["loop"], med["loop"] / med["single"],
                    nview * (2 * r + 1) ** 2 * 256.0 / med["single"] * 1e-6, 100.0 * spread, int(selected.sum()), nview // P))
    lines.append("single = one ops.pose_score call; loop = P x (ops.guided_match(want_dist=True) + torch float64 reduction); loop / 1 = their "
                 "ratio; gather TB/s = in-view (row, pose) x (2r + 1)^2 x 256 B / single time; spread = largest |repeat - median| / median")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
