#!/usr/bin/env python3
"""The call of DESIGN.md 4t against the composition a user writes without it: HIP events after warm-up, the two sides timed alternately
in the same process, `--repeats` times: medians, and the largest |repeat - median| / median over both sides as the spread.

single:  one ops.densify (cmr_densify_f32) call: dense depth, confidence and counts.
compose: the joint bilateral filter in eager torch with the same formula: the maps padded by R, then a loop over the (2R + 1)^2 shifted
         slices, each a handful of elementwise launches over B x h x w (the guide's squared difference, exp, the validity mask, two
         accumulations), and the normalisation at the end.  unfold is not used: its (2R + 1)^2-fold copy of the maps does not fit.
The sparse maps are rendered first: ops.render_points of visibility_reference.scene's cloud, every row selected; the guide is
densify_reference.make_guide's 3 planes.  Before timing the two sides are held to the same composition run in float64 on the device:
"filled" equal on every pixel that run calls decided, values within the bound of tests/densify_reference.py of its value.
Shapes: B = 8, N = 16384, maps 88 x 304 and 352 x 1216, R in {4, 8}, with and without the guide.
python tools/densify_bench.py [--iters 200] [--compose-iters 3] [--warmup 3] [--repeats 5] [--out profiles/densify_bench.txt]"""
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

import densify_reference as dr  # noqa: E402
import visibility_reference as vr  # noqa: E402
from cmr_agent_amd import ops  # noqa: E402

SHAPES = [(8, 16384, 88, 304), (8, 16384, 352, 1216)]
RADII = (4, 8)
SIGMA_R = 0.1
MIN_WEIGHT = 1e-3


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


def compose(depth, guide, R, sigma_s, sigma_r, min_weight, dtype=torch.float32, extras=False):
    """The definition as a loop over shifted slices -> (dense_depth, conf[, n, a_max]); keep = True."""
    B, h, w = depth.shape
    ks, kr = 1.0 / (2.0 * dr.f32(sigma_s) ** 2), 1.0 / (2.0 * dr.f32(sigma_r) ** 2)
    valid = torch.isfinite(depth) & (depth > 0)
    z = torch.where(valid, depth, torch.zeros_like(depth)).to(dtype)
    pad = lambda a: torch.nn.functional.pad(a, (R, R, R, R))
    zp, vp = pad(z), pad(valid.to(dtype))
    g = None if guide is None else guide.to(dtype)
    gp = None if g is None else pad(g)
    S0, S1 = torch.zeros_like(z), torch.zeros_like(z)
    if extras:
        n, a_max = torch.zeros_like(z), torch.zeros_like(z)
    for dy in range(2 * R + 1):
        for dx in range(2 * R + 1):
            v = vp[:, dy:dy + h, dx:dx + w]
            a = ((dx - R) ** 2 + (dy - R) ** 2) * ks
            if g is None:
                wt = v * math.exp(-a)
            else:
                d = g - gp[:, :, dy:dy + h, dx:dx + w]
                arg = (d * d).sum(1) * kr + a
                wt = torch.exp(-arg) * v
            S0 += wt
            S1 += wt * zp[:, dy:dy + h, dx:dx + w]
            if extras:
                n += v
                a_max = torch.maximum(a_max, v * (a if g is None else arg))
    filled = S0 >= dr.f32(min_weight)
    dense = torch.where(valid, z, torch.where(filled, S1 / S0, torch.full_like(z, math.inf)))
    return (dense, S0, n, a_max) if extras else (dense, S0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--compose-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    lines = ["%-24s %-10s | %10s %11s %11s | %6s | %s" % ("shape B x N, h x w", "R, guide", "single us", "compose us", "compose / 1", "spread", "counts; worst share of the bound")]
    ok = True
    for B, N, h, w in SHAPES:
        sc = vr.scene(B, N, h, w, seed=41, selected=0.4)
        depth = ops.render_points(f(sc["pts"]), f(sc["pose"]), f(sc["K"]), h, w)[1]
        guide3 = f(dr.make_guide(np.random.default_rng(7), B, h, w, 3))
        for R in RADII:
            for guide in (None, guide3):
                ss = max(R, 1) / 2
                single = lambda: ops.densify(depth, guide=guide, radius=R, sigma_r=SIGMA_R, min_weight=MIN_WEIGHT)
                eager = lambda: compose(depth, guide, R, ss, SIGMA_R, MIN_WEIGHT)
                dd, _, conf, _, counts = single()
                od, oconf = eager()
                d64, S64, n, a_max = compose(depth, guide, R, ss, SIGMA_R, MIN_WEIGHT, dtype=torch.float64, extras=True)
                decided = ~((n > 0) & ((S64 - dr.f32(MIN_WEIGHT)).abs() <= dr.DECIDE_MARGIN * dr.f32(MIN_WEIGHT)))
                rel = (2.0 * (n + 8.0) + 8.0 * a_max) * dr.U
                fin = torch.isfinite(d64)
                shares = []
                for name, got in (("the op", dd), ("the composition", od)):
                    assert not bool(((torch.isfinite(got) != fin) & decided).any()), name + " disagrees with float64 on a decided pixel"
                    on = fin & decided
                    share = ((got.double() - d64).abs()[on] / (rel * d64)[on]).max().item()
                    assert share <= 1.0, name + " misses the float64 bound: share %.3f" % share
                    shares.append(share)
                med, spread = _alternate([("single", single, args.iters), ("compose", eager, args.compose_iters)], args.warmup, args.repeats)
                faster = med["single"] * (1.0 + spread) < med["compose"] * (1.0 - spread)
                ok = ok and faster
                c = counts.sum(0).tolist()
                lines.append("%-24s %-10s | %10.1f %11.1f %11.1f | %5.1f%% | samples %d, filled %d of %d; undecided %d; op %.3f, composition %.3f%s" % (
                    "%d x %d, %d x %d" % (B, N, h, w), "%d, %s" % (R, "none" if guide is None else "3 planes"), med["single"], med["compose"],
                    med["compose"] / med["single"], 100.0 * spread, c[0], c[2], B * h * w, int((~decided).sum()), shares[0], shares[1],
                    "" if faster else "   <- not faster by more than the spread"))
    lines.append("single = one ops.densify call (keep, sigma_s = R / 2, sigma_r = %g, min_weight = %g); compose = the eager torch loop over the "
                 "(2R + 1)^2 shifted slices with the same formula; compose / 1 = their ratio; spread = largest |repeat - median| / median over both "
                 "sides; share = largest error against the float64 run of the composition as a share of the bound of tests/densify_reference.py" % (
                     SIGMA_R, MIN_WEIGHT))
    lines.append("requirement (single faster than compose by more than the spread at every shape): %s" % ("met" if ok else "NOT met"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
