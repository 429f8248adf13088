#!/usr/bin/env python3
"""The two calls of DESIGN.md 4n against what they stand beside, HIP events after warm-up, each pair timed alternately in the same
process, `--repeats` times: medians, and the largest |repeat - median| / median as the spread.

match:  ops.guided_match (cmr_guided_match_f32) at the three shapes of tools/match_bench.py -- the same random unit features and the same
        selection (the synthetic loader's pc_mask), pose = the loader's true pose turned by 1.5 deg about a random axis and moved by
        0.15 N(0, I) -- for r in {2, 4, 8}, against ops.feat_match (the global sweep) on the same selection.  "gather TB/s" counts
        (2r + 1)^2 pixel rows of 256 B per in-view point, shared or not (windows clipped by the map edge count in full).
refine: ops.pnp_refine (cmr_pnp_refine_f32, iters = 10) on the scenes of tools/pnp_bench.py, started from the unrefined winner of
        ops.pnp_ransac(refine_iters=0), eager and replayed from a captured graph, beside the whole ops.pnp_ransac(refine_iters=10) call
        (whose pnp_select_kernel holds the single-workgroup refinement; kernel times: a rocprofv3 --kernel-trace --stats run of
        `--part refine`, profiles/guided_kernel_stats.txt).
python tools/guided_bench.py [--part match|refine|both] [--iters 20] [--warmup 3] [--repeats 5] [--out profiles/guided_bench.txt]"""
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

import pnp_reference as ref  # noqa: E402
from cmr_agent_amd import ops  # noqa: E402
from cmr_agent_amd.utils import synthetic  # noqa: E402

MATCH_SHAPES = [(8, 16384, 40, 128), (8, 65536, 88, 304), (4, 32768, 224, 400)]
REFINE_SHAPES = [(8, 16384, 1024), (8, 65536, 1024), (4, 32768, 1024)]
RADII = (2, 4, 8)


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters                                  # us


def _alternate(calls, iters, warmup, repeats):
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


def _perturbed(P, seed):
    rng = np.random.default_rng(seed)
    out = np.array(P, np.float64)
    for b in range(out.shape[0]):
        dR = ref._rot(rng.normal(size=3), math.radians(1.5))
        out[b, :3, :3] = dR @ P[b, :3, :3]
        out[b, :3, 3] = dR @ P[b, :3, 3] + 0.15 * rng.normal(size=3)
    return out


def bench_match(args, dev, lines):
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    g = torch.Generator(device="cpu").manual_seed(7)
    lines.append("%-24s %8s %8s | %10s | %s | %6s" % ("shape B x N, h x w", "selected", "in view", "global us", " | ".join(
        "r=%d us %6s %11s" % (r, "x", "gather TB/s") for r in RADII), "spread"))
    for B, N, h, w in MATCH_SHAPES:
        raw = synthetic.make_raw(B, N, 4 * h, 4 * w, seed=11, n_circle=1)
        mask = torch.from_numpy(raw["pc_mask"]).to(dev).contiguous()                 # int64 [B, N]
        pc = torch.nn.functional.normalize(torch.randn(B * N, 64, generator=g), dim=1).to(dev)
        img = torch.nn.functional.normalize(torch.randn(B, h, w, 64, generator=g), dim=3).to(dev)
        pts, K, pose = f(raw["pc"]), f(raw["K"]), f(_perturbed(raw["P"], 5))
        calls = [("global", lambda: ops.feat_match(pc, img, mask))]
        for r in RADII:
            calls.append(("r%d" % r, lambda r=r: ops.guided_match(pts, pc, img, mask, pose, K, r)))
        med, spread = _alternate(calls, args.iters, args.warmup, args.repeats)
        counts = ops.guided_match(pts, pc, img, mask, pose, K, 4)[2].sum(0).tolist()
        cols = []
        for r in RADII:
            nview = int(ops.guided_match(pts, pc, img, mask, pose, K, r)[2][:, 1].sum())
            t = med["r%d" % r]
            cols.append("%7.1f %6.2f %11.2f" % (t, med["global"] / t, nview * (2 * r + 1) ** 2 * 256.0 / t * 1e-6))
        lines.append("%-24s %8d %8d | %10.1f | %s | %5.1f%%" % ("%d x %d, %d x %d" % (B, N, h, w), counts[0], counts[1], med["global"],
                                                               " | ".join(cols), 100.0 * spread))
    lines.append("x = global sweep / guided call; in view at r = 4; gather TB/s = in-view points x (2r + 1)^2 x 256 B / time")


def bench_refine(args, dev, lines):
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    lines.append("%-22s %8s | %12s %12s %12s | %14s | %6s %s" % ("B x N, n_hyp", "sel/smp", "refine us", "replayed us", "launches",
                                                               "pnp_ransac us", "spread", "status"))
    for B, N, n_hyp in REFINE_SHAPES:
        s = ref.planted(B, N, 88, 304, seed=N + n_hyp, outlier_frac=0.3, noise=0.3)
        mask = (torch.rand(B, N, generator=torch.Generator().manual_seed(1)) < 0.4).to(dev)
        a = (f(s["pts"]), f(s["uv"]), mask, f(s["K"]))
        start = ops.pnp_ransac(*a, n_hyp=n_hyp, thr=1.0, seed=0, refine_iters=0)[0]
        eager = lambda: ops.pnp_refine(*a, start, thr=1.0, iters=10)
        eager()
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            eager()
        torch.cuda.current_stream().wait_stream(st)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = eager()
        calls = [("refine", eager), ("replay", graph.replay),
                 ("ransac", lambda: ops.pnp_ransac(*a, n_hyp=n_hyp, thr=1.0, seed=0, refine_iters=10))]
        med, spread = _alternate(calls, args.iters, args.warmup, args.repeats)
        graph.replay()
        torch.cuda.synchronize()
        lines.append("%-22s %8d | %12.1f %12.1f %12d | %14.1f | %5.1f%% %s" % (
            "%d x %d, %d" % (B, N, n_hyp), float(mask.sum()) / B, med["refine"], med["replay"], 3 + 2 * 11, med["ransac"], 100.0 * spread,
            "".join(map(str, out[2].tolist()))))
    lines.append("refine = ops.pnp_refine(iters=10) from the unrefined RANSAC winner, eager; replayed = the same call from a captured graph; "
                 "pnp_ransac = the whole ops.pnp_ransac(refine_iters=10) call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("match", "refine", "both"), default="both")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    lines = []
    if args.part in ("match", "both"):
        bench_match(args, dev, lines)
    if args.part in ("refine", "both"):
        if lines:
            lines.append("")
        bench_refine(args, dev, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
