#!/usr/bin/env python3
"""ops.match_conf (cmr_match_conf_f32: nearest pixel + dual-softmax confidence) against ops.feat_match_filter
(cmr_feat_match_filter_f32, DESIGN.md 4m, unchanged) on the same inputs, HIP events after warm-up, at the three shapes, features and
masks of tools/match_filter_bench.py: random unit features, the selection is the synthetic loader's pc_mask.  "mutual" is the filter's
two-sweep call (forward + reverse: the same MFMA work and traffic as match_conf, without the exponentials), "both" its three-sweep call
(mutual + windowed ratio test), the filter that reaches the precision of conf >= 0.1 on the planted scenes.  The three calls are timed
alternately, `--repeats` times, and the median of each is printed (spread: the largest |repeat - median| / median over the three).
TFLOP/s counts 2 * 64 FLOP per (selected point, pixel) pair and sweep; the fraction is of the measured fp32 MFMA peak, 155 TFLOP/s
(profiles/r04_mfma_peak.txt).  The requirement of 4p: conf / both < 1 at every shape; conf / mutual is reported.
python tools/match_conf_bench.py [--iters 20] [--warmup 3] [--repeats 5] [--once SHAPE_INDEX]"""
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


def _inputs(B, N, h, w, g, dev):
    raw = synthetic.make_raw(B, N, 4 * h, 4 * w, seed=11, n_circle=1)
    mask = torch.from_numpy(raw["pc_mask"]).to(dev).contiguous()                     # int64 [B, N]
    pc = torch.nn.functional.normalize(torch.randn(B * N, 64, generator=g), dim=1).to(dev)
    img = torch.nn.functional.normalize(torch.randn(B, h, w, 64, generator=g), dim=3).to(dev)
    return pc, img, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--once", type=int, default=None, help="one ops.match_conf call at SHAPES[i] and nothing else (for a kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(7)
    if args.once is not None:
        pc, img, mask = _inputs(*SHAPES[args.once], g, dev)
        ops.match_conf(pc, img, mask, temperature=0.1, min_conf=0.1)
        torch.cuda.synchronize()
        return
    print("%-22s %8s %6s | %10s %6s | %10s %6s | %10s %6s | %11s %13s | %6s" % (
        "shape B x N, h x w", "selected", "kept", "conf us", "peak", "mutual us", "peak", "both us", "peak", "conf / both", "conf / mutual",
        "spread"))
    for B, N, h, w in SHAPES:
        pc, img, mask = _inputs(B, N, h, w, g, dev)
        nsel = int(mask.sum())
        flop = 2.0 * 64 * h * w * nsel                                               # one sweep
        calls = [("conf", 2, lambda: ops.match_conf(pc, img, mask, temperature=0.1, min_conf=0.1)),
                 ("mutual", 2, lambda: ops.feat_match_filter(pc, img, mask, mutual=True)),
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
        idx, _, keep, _, _, _, _ = calls[0][2]()
        assert torch.equal(idx, ops.feat_match(pc, img, mask)[0])                    # the same matches as the matcher, at the timed size
        peak = lambda name, sweeps: 100.0 * sweeps * flop / med[name] * 1e-6 / PEAK_TF
        print("%-22s %8d %6d | %10.1f %5.1f%% | %10.1f %5.1f%% | %10.1f %5.1f%% | %11.3f %13.3f | %5.1f%%" % (
            "%d x %d, %d x %d" % (B, N, h, w), nsel, int(keep.sum()), med["conf"], peak("conf", 2), med["mutual"], peak("mutual", 2),
            med["both"], peak("both", 3), med["conf"] / med["both"], med["conf"] / med["mutual"], 100.0 * spread))


if __name__ == "__main__":
    main()
