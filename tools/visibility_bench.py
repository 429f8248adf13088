#!/usr/bin/env python3
"""The call of DESIGN.md 4r against the composition a user writes without it: HIP events after warm-up, the two sides timed alternately in
the same process, `--repeats` times: medians, and the largest |repeat - median| / median over both sides as the spread.

single:  one ops.visibility (cmr_visibility_f32) call: visible flags and counts.
compose: torch.matmul projection, rounding and the in-view test, scatter_reduce(amin) into a map of +inf, max_pool2d of the negated map,
         gather and compare -- the same flags from eager torch (about twenty launches and half a dozen [B, N] / [B, h w] temporaries).
Before timing, the two sides' flags must agree except on the rows the float64 restatement (tests/visibility_reference.py) calls undecided.
Shapes: B = 8, N = 16384, ~40 % of the rows queried, every row occluding, maps 88 x 304 and 352 x 1216, radius in {0, 1, 4}; scenes:
visibility_reference.scene.  Last line: refine_pose_from_matches on a guided_reference.scene batch (8 x 16384, 88 x 304, rounds 6 / 3 / 2)
with visible=True against visible=None, the difference per round.
python tools/visibility_bench.py [--iters 200] [--warmup 3] [--repeats 5] [--out profiles/visibility_bench.txt]"""
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

import guided_reference as gref  # noqa: E402
import visibility_reference as vr  # noqa: E402
from cmr_agent_amd import ops  # noqa: E402

SHAPES = [(8, 16384, 88, 304), (8, 16384, 352, 1216)]
RADII = (0, 1, 4)
REL_TOL, ABS_TOL = 0.05, 0.0
ROUNDS = ((6, 4.0), (3, 2.0), (2, 1.0))


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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    lines = ["%-24s %2s | %10s %11s %11s | %6s | %s" % ("shape B x N, h x w", "r", "single us", "compose us", "compose / 1", "spread",
                                                       "queried, in view, visible; undecided rows, rows that differ")]
    ok = True
    for B, N, h, w in SHAPES:
        sc = vr.scene(B, N, h, w, seed=41, selected=0.4)
        pts, pose, K, mask = f(sc["pts"]), f(sc["pose"]), f(sc["K"]), sc["mask"].to(dev)
        R, t = pose[:, :3, :3].contiguous(), pose[:, :3, 3:4].contiguous()
        opr, atol = torch.tensor(vr.opr32(REL_TOL), device=dev), torch.tensor(np.float32(ABS_TOL), device=dev)
        inf = torch.full((B, N), math.inf, device=dev)
        for r in RADII:
            def compose():
                p = torch.matmul(K, torch.matmul(R, pts) + t)
                z = p[:, 2]
                u, v = p[:, 0] / z, p[:, 1] / z
                cx, cy = torch.round(u), torch.round(v)
                view = (z > 0) & torch.isfinite(u) & torch.isfinite(v) & (cx >= 0) & (cx <= w - 1) & (cy >= 0) & (cy <= h - 1)
                cell = torch.where(view, cy * w + cx, torch.zeros_like(cx)).long()
                Z = torch.full((B, h * w), math.inf, device=dev).scatter_reduce(1, cell, torch.where(view, z, inf), "amin", include_self=True)
                zmin = -torch.nn.functional.max_pool2d(-Z.view(B, 1, h, w), 2 * r + 1, stride=1, padding=r).view(B, h * w)
                return mask & view & (z <= (zmin * opr + atol).gather(1, cell))

            single = lambda: ops.visibility(pts, pose, K, h, w, mask, radius=r, rel_tol=REL_TOL, abs_tol=ABS_TOL)
            vis, counts, _, _, _ = single()
            other = compose()
            ref = vr.visibility(sc["pts"], sc["mask"], None, sc["pose"], sc["K"], h, w, r, REL_TOL, ABS_TOL)
            decided = torch.from_numpy(np.stack([x["decided"] for x in ref])).to(dev)
            want = torch.from_numpy(np.stack([x["visible"] for x in ref])).to(dev)
            differ = vis.view(B, N) != other
            assert not bool((differ & decided).any()), "the two sides disagree on a decided row"
            assert not bool(((vis.view(B, N) != want) & decided).any()), "the op disagrees with float64 on a decided row"
            med, spread = _alternate([("single", single, args.iters), ("compose", compose, args.iters)], args.warmup, args.repeats)
            c = counts.sum(0).tolist()
            faster = med["single"] * (1.0 + spread) < med["compose"] * (1.0 - spread)
            ok = ok and faster
            lines.append("%-24s %2d | %10.1f %11.1f %11.2f | %5.1f%% | %d, %d, %d; %d, %d%s" % (
                "%d x %d, %d x %d" % (B, N, h, w), r, med["single"], med["compose"], med["compose"] / med["single"], 100.0 * spread, c[0], c[1], c[2],
                sum(x["undecided"] for x in ref), int(differ.sum()), "" if faster else "   <- not faster by more than the spread"))
    lines.append("single = one ops.visibility call; compose = matmul projection + scatter_reduce(amin) + max_pool2d + gather and compare in eager "
                 "torch; compose / 1 = their ratio; spread = largest |repeat - median| / median over both sides")
    # the extra time per round of refine_pose_from_matches(visible=True)
    from cmr_agent_amd.config import KittiConfiguration
    from cmr_agent_amd.models import MultiHeadModel
    B, N, h, w = SHAPES[0]
    gs = gref.scene(B=B, N=N, h=h, w=w, seed=201)
    model = MultiHeadModel(KittiConfiguration(num_pt=N, device=dev))
    data = {"pc": f(gs["pts"]), "K": f(gs["K"]), "pnp_pose": f(gs["start"]), "pc_overlap_pred": (torch.rand(B, N) < 0.4).to(dev),
            "pc_geo_feat": gs["pc"].view(B, N, 64).permute(0, 2, 1).contiguous().to(dev), "img_geo_feat": gs["img"].permute(0, 3, 1, 2).contiguous().to(dev)}
    radii, thrs = tuple(x[0] for x in ROUNDS), tuple(x[1] for x in ROUNDS)
    plain = lambda: model.refine_pose_from_matches(data, radii=radii, thrs=thrs)
    withv = lambda: model.refine_pose_from_matches(data, radii=radii, thrs=thrs, visible=True)
    iters = max(1, args.iters // 4)
    med, spread = _alternate([("plain", plain, iters), ("visible", withv, iters)], args.warmup, args.repeats)
    lines.append("refine_pose_from_matches %d x %d, %d x %d, rounds %s: visible=None %.1f us, visible=True %.1f us, %+.1f us per round (spread %.1f%%)" % (
        B, N, h, w, "/".join(str(x) for x in radii), med["plain"], med["visible"], (med["visible"] - med["plain"]) / len(radii), 100.0 * spread))
    lines.append("requirement (single faster than compose by more than the spread at every shape): %s" % ("met" if ok else "NOT met"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
