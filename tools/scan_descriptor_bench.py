#!/usr/bin/env python3
"""ops.scan_descriptor and ops.scan_match (csrc/scan_descriptor.hip) at the sizes of a KITTI-length sequence.

  * one descriptor of a scan of `--points` rows (uniform over +-90 m, so a fifth of them lie outside the 80 m the descriptor reaches) at
    `--rings` x `--sectors`: the whole op (its tables, its launch, its one host read) and the entry point alone;
  * one match of `--frames` descriptors against themselves with the triangular limit of the loop search (`--gap`): the whole op, and beside it
    the same job in torch on the device -- unit columns, then per shift ONE matrix product of the flattened unit columns with the rolled
    candidates' and one of the empty flags, a division and a running minimum.  The torch job has no limit to honour (it computes all
    F x F pairs, twice the kernel's) and sums in the matrix product's order, so its distances agree with the kernel's to rounding, not bit
    for bit; the largest difference is printed.

HIP events round each call, the median over `--repeats` after `--warmup`, the two match jobs alternating.
python tools/scan_descriptor_bench.py [--points 120000] [--frames 4541] [--repeats 5] [--warmup 1] [--out profiles/scan_descriptor_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cmr_agent_amd import _lib, ops  # noqa: E402
from cmr_agent_amd.dataset import loops  # noqa: E402
from cmr_agent_amd.utils import workmodel  # noqa: E402


def _times_ms(fns, repeats, warmup):
    """the median of each of `fns`, the calls alternating"""
    ms = [[] for _ in fns]
    for it in range(warmup + repeats):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[k].append(e0.elapsed_time(e1))
    return [statistics.median(m) for m in ms]


def torch_match(desc, min_cols):
    """-> (dist, shift) of desc [F, R, S] against itself, every pair, by one matrix product per shift"""
    F, R, S = desc.shape
    n2 = (desc * desc).sum(1)
    full = (n2 != 0).to(desc.dtype)
    unit = torch.where(n2[:, None, :] != 0, desc / n2.sqrt()[:, None, :], torch.zeros_like(desc))
    q = unit.reshape(F, R * S)
    best = torch.full((F, F), float("inf"), device=desc.device)
    shift = torch.full((F, F), -1, dtype=torch.int32, device=desc.device)
    for k in range(S):
        total = q @ torch.roll(unit, -k, 2).reshape(F, R * S).T
        cnt = full @ torch.roll(full, -k, 1).T
        d = torch.where(cnt >= min_cols, 1.0 - total / cnt, torch.full_like(total, float("inf")))
        better = d < best
        best, shift = torch.where(better, d, best), torch.where(better, torch.full_like(shift, k), shift)
    return torch.where(shift < 0, torch.full_like(best, float("nan")), best), shift


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--frames", type=int, default=4541)
    ap.add_argument("--rings", type=int, default=20)
    ap.add_argument("--sectors", type=int, default=60)
    ap.add_argument("--gap", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    R, S, F = args.rings, args.sectors, args.frames
    gen = torch.Generator(device=dev).manual_seed(0)
    stream = torch.cuda.current_stream().cuda_stream

    # ---- one descriptor ----
    pts = torch.cat([torch.rand((args.points, 2), device=dev, generator=gen) * 180 - 90, torch.rand((args.points, 1), device=dev, generator=gen) * 12 - 1.7], 1)
    one = ops.scan_descriptor(pts, R, S)
    edge2, dirs = (torch.from_numpy(t).to(dev) for t in ops.scan_tables(R, S, 0.0, 80.0))
    desc, counts = torch.empty((R, S), device=dev), torch.empty((3,), dtype=torch.int64, device=dev)

    def entry():
        _lib.call("cmr_scan_descriptor_f32", pts.data_ptr(), 3, args.points, R, S, edge2.data_ptr(), dirs.data_ptr(), 2.0, desc.data_ptr(),
                  counts.data_ptr(), stream)

    op_ms, entry_ms = _times_ms([lambda: ops.scan_descriptor(pts, R, S), entry], 4 * args.repeats, args.warmup)
    assert torch.equal(desc, one.desc) and tuple(counts.tolist()) == tuple(one[1:])
    lines = ["one scan of %d rows at %d x %d, 80 m (binned %d, outside %d): ops.scan_descriptor whole call %.3f ms, cmr_scan_descriptor_f32 alone "
             "%.3f ms" % (args.points, R, S, one.binned, one.outside, op_ms, entry_ms)]

    # ---- one match of a sequence against itself ----
    batch = torch.rand((F, R, S), device=dev, generator=gen) * 6
    batch = batch * (torch.rand((F, R, S), device=dev, generator=gen) >= 0.3) * (torch.rand((F, 1, S), device=dev, generator=gen) >= 0.1)
    limit = torch.from_numpy(loops.gap_limits(F, args.gap)).to(dev)
    pairs = int(limit.sum())
    got = ops.scan_match(batch, batch, limit)
    ref = torch_match(batch, S // 4)
    seen = ~torch.isnan(got.dist)
    diff = float((got.dist[seen] - ref[0][seen]).abs().max()) if pairs else 0.0
    agree = float((got.shift[seen] == ref[1][seen]).float().mean()) if pairs else 1.0
    hip_ms, torch_ms = _times_ms([lambda: ops.scan_match(batch, batch, limit), lambda: torch_match(batch, S // 4)], args.repeats, args.warmup)
    flops = workmodel.WORK["cmr_scan_match_f32"](dict(Q=1, N=1, R=R, S=S))[0] * pairs
    lines += ["%d descriptors of %d x %d against themselves, limit i - %d + 1 (%d of %d pairs compared): ops.scan_match whole call %.3f ms = "
              "%.2f T unfused fp32 operations/s over the compared pairs" % (F, R, S, args.gap, pairs, F * F, hip_ms, flops / hip_ms / 1e9),
              "    the same job in torch (one matrix product per shift, all %d pairs, no limit): %.3f ms;  x %.2f" % (F * F, torch_ms, torch_ms / hip_ms),
              "    kernel against torch over the compared pairs: largest |distance difference| %.3e, same shift in %.4f of them" % (diff, agree)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
