#!/usr/bin/env python3
"""ops.pnp_ransac (cmr_pnp_ransac_f32): time per call (HIP events after warm-up, eager launches) and the share of each of
its kernels (torch.profiler device times over the same calls), on planted scenes with ~40 % of the points selected and 30 % of those
outliers, at B = 8 x {16 384, 65 536} points x n_hyp {512, 1024, 4096} and at the nuScenes shape B = 4 x 32 768 points.
VALU bound of the scoring kernel: its inner loop issues SCORE_VALU_PER_PAIR vector instructions per (hypothesis, correspondence) pair
(110 per unrolled step of 8 pairs, gfx950 ISA of csrc/pnp.hip, v_pk_fma_f32 counted once); the chip issues 256 CU x 4 SIMD x 32 lanes
per clock at 2.4 GHz = 78.6e12 lane-instructions / s (the 157.3 TFLOP/s fp32 vector peak of the MI355X datasheet, packed FMA), so the
bound is pairs x SCORE_VALU_PER_PAIR / 78.6e12.
python tools/pnp_bench.py [--iters 20] [--warmup 3] [--out profiles/pnp_bench.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pnp_reference as ref  # noqa: E402
from cmr_agent_amd import ops  # noqa: E402

SHAPES = [(8, 16384, 512), (8, 16384, 1024), (8, 16384, 4096), (8, 65536, 512), (8, 65536, 1024), (8, 65536, 4096), (4, 32768, 1024)]
SCORE_VALU_PER_PAIR = 110 / 8
LANE_RATE = 256 * 4 * 32 * 2.4e9


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters                                  # us


def _kernel_us(fn, iters):
    """Device time per call of every pnp_* kernel (torch.profiler); {} when the profiler records no device events."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        if "pnp_" in e.key:
            name = e.key.split("pnp_")[1].split("(")[0].split("_kernel")[0]
            t = getattr(e, "device_time_total", None)
            if t is None:
                t = getattr(e, "cuda_time_total", 0.0)
            out[name] = out.get(name, 0.0) + t / iters
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    lines = ["%-24s %8s %10s %9s %10s %9s %11s %12s %s" % ("B x N, n_hyp", "sel/smp", "call us", "score us", "score %", "hyp us",
                                                         "select us", "score/VALU", "status")]
    for B, N, n_hyp in SHAPES:
        s = ref.planted(B, N, 88, 304, seed=N + n_hyp, outlier_frac=0.3, noise=0.3)
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        mask = (torch.rand(B, N, generator=torch.Generator().manual_seed(1)) < 0.4).to(dev)
        args_ = (f(s["pts"]), f(s["uv"]), mask, f(s["K"]))
        fn = lambda: ops.pnp_ransac(*args_, n_hyp=n_hyp, thr=1.0, seed=0, refine_iters=10)
        t = _time(fn, args.iters, args.warmup)
        k = _kernel_us(fn, max(3, args.iters // 4))
        nsel = float(mask.sum()) / B
        bound = B * n_hyp * nsel * SCORE_VALU_PER_PAIR / LANE_RATE * 1e6
        st = fn()[2].tolist()
        sc = k.get("score")
        fmt = lambda v: "%9.1f" % v if v is not None else "unmeasd"
        lines.append("%-24s %8d %10.1f %9s %9s%% %9s %11s %11s %s" % (
            "%d x %d, %d" % (B, N, n_hyp), nsel, t, fmt(sc), ("%.1f" % (100.0 * sc / t)) if sc else "unmeasd", fmt(k.get("hyp")),
            fmt(k.get("select")), ("%.0f%%" % (100.0 * bound / sc)) if sc else "unmeasured", "".join(map(str, st))))
    lines.append("score/VALU = the scoring kernel's time at the VALU issue bound (%.2f instructions per pair) / its measured time" %
                 SCORE_VALU_PER_PAIR)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
