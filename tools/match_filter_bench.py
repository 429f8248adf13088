#!/usr/bin/env python3
"""ops.feat_match_filter (cmr_feat_match_filter_f32: nearest pixel + mutual check / windowed ratio test) against
ops.feat_match (cmr_feat_match_f32) on the same inputs, HIP events after warm-up, at the three map sizes of tools/match_bench.py: random
unit features, the selection is the synthetic loader's pc_mask.  The matcher is one distance sweep, "mutual" and "ratio" are two, "both"
is three; the matcher and the three filter calls are timed alternately, `--repeats` times, and the median of each is printed with its
ratio to the matcher's median (spread: the largest |repeat - median| / median over the four).  TFLOP/s counts 2 * 64 FLOP per (selected
point, pixel) pair and sweep; the fraction is of the measured fp32 MFMA peak, 155 TFLOP/s (profiles/r04_mfma_peak.txt).
python tools/match_filter_bench.py [--iters 20] [--warmup 3] [--repeats 5]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cmr_agent_amd import ops  # noqa: E402
from cmr_agent_amd.utils import synthetic  # noqa: E402

SHAPES = [(8, 16384, 40, 128), (8, 65536, 88, 304), (4, 32768, 224, 400)]
PEAK_TF = 155.0


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters                                  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(7)
    print("%-22s %8s %6s | %10s %6s | %10s %5s %6s | %10s %5s %6s | %10s %5s %6s | %6s" % (
        "shape B x N, h x w", "selected", "kept", "match us", "peak", "mutual us", "x", "peak", "ratio us", "x", "peak", "both us", "x",
        "peak", "spread"))
    for B, N, h, w in SHAPES:
        raw = synthetic.make_raw(B, N, 4 * h, 4 * w, seed=11, n_circle=1)
        mask = torch.from_numpy(raw["pc_mask"]).to(dev).contiguous()                 # int64 [B, N]
        pc = torch.nn.functional.normalize(torch.randn(B * N, 64, generator=g), dim=1).to(dev)
        img = torch.nn.functional.normalize(torch.randn(B, h, w, 64, generator=g), dim=3).to(dev)
        nsel = int(mask.sum())
        flop = 2.0 * 64 * h * w * nsel                                               # one sweep
        calls = [("match", 1, lambda: ops.feat_match(pc, img, mask)),
                 ("mutual", 2, lambda: ops.feat_match_filter(pc, img, mask, mutual=True)),
                 ("ratio", 2, lambda: ops.feat_match_filter(pc, img, mask, mutual=False, ratio=0.9, excl_radius=2)),
                 ("both", 3, lambda: ops.feat_match_filter(pc, img, mask, mutual=True, ratio=0.9, excl_radius=2))]
        for _, _, fn in calls:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name, _, _ in calls}
        for _ in range(args.repeats):
            for name, _, fn in calls:
                t[name].append(_time(fn, args.iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = max(abs(x - med[k]) / med[k] for k, v in t.items() for x in v)
        idx, keep, counts, _, _, _ = calls[3][2]()
        assert torch.equal(idx, ops.feat_match(pc, img, mask)[0])                    # the same matches as the matcher, at the timed size
        peak = lambda name, sweeps: 100.0 * sweeps * flop / med[name] * 1e-6 / PEAK_TF
        print("%-22s %8d %6d | %10.1f %5.1f%% | %10.1f %5.2f %5.1f%% | %10.1f %5.2f %5.1f%% | %10.1f %5.2f %5.1f%% | %5.1f%%" % (
            "%d x %d, %d x %d" % (B, N, h, w), nsel, int(keep.sum()), med["match"], peak("match", 1),
            med["mutual"], med["mutual"] / med["match"], peak("mutual", 2), med["ratio"], med["ratio"] / med["match"], peak("ratio", 2),
            med["both"], med["both"] / med["match"], peak("both", 3), 100.0 * spread))


if __name__ == "__main__":
    main()
