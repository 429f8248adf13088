#!/usr/bin/env python3
"""ops.match_subpixel (cmr_match_subpixel_f32) beside ops.guided_match(radius=1) on the same rows, HIP events after
warm-up, the two timed alternately in the same process, `--repeats` times: medians, and the largest |repeat - median| / median as the
spread.

The three shapes, random unit features and selection (the synthetic loader's pc_mask) of tools/match_bench.py, the perturbed pose of
tools/guided_bench.py; idx = ops.guided_match(radius=2)'s, mask = its keep (the in-view rows).  guided_match(radius=1) reads 9 pixel rows
per in-view point and also projects and compacts; match_subpixel reads 5.  "gather TB/s" counts 5 rows of 256 B per matched row.
The requirement of 4o: at every shape match_subpixel takes no longer than guided_match(radius=1) plus the run's spread.
python tools/subpixel_bench.py [--iters 20] [--warmup 3] [--repeats 5] [--out profiles/subpixel_bench.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cmr_agent_amd import ops  # noqa: E402
from cmr_agent_amd.utils import synthetic  # noqa: E402
from guided_bench import _alternate, _perturbed  # noqa: E402
from match_bench import SHAPES  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    g = torch.Generator(device="cpu").manual_seed(7)
    lines = ["%-24s %8s %8s | %12s %11s | %14s | %6s | %s" % ("shape B x N, h x w", "matched", "fitted", "subpixel us", "gather TB/s",
                                                             "guided r=1 us", "spread", "requirement")]
    met = True
    for B, N, h, w in SHAPES:
        raw = synthetic.make_raw(B, N, 4 * h, 4 * w, seed=11, n_circle=1)
        mask = torch.from_numpy(raw["pc_mask"]).to(dev).contiguous()                 # int64 [B, N]
        pc = torch.nn.functional.normalize(torch.randn(B * N, 64, generator=g), dim=1).to(dev)
        img = torch.nn.functional.normalize(torch.randn(B, h, w, 64, generator=g), dim=3).to(dev)
        pts, K, pose = f(raw["pc"]), f(raw["K"]), f(_perturbed(raw["P"], 5))
        idx, keep, _, _, _ = ops.guided_match(pts, pc, img, mask, pose, K, 2)
        keep = keep.contiguous()
        calls = [("subpixel", lambda: ops.match_subpixel(pc, img, idx, mask=keep)),
                 ("guided1", lambda: ops.guided_match(pts, pc, img, mask, pose, K, 1))]
        med, spread = _alternate(calls, args.iters, args.warmup, args.repeats)
        counts = ops.match_subpixel(pc, img, idx, mask=keep)[1].sum(0).tolist()
        ok = med["subpixel"] <= med["guided1"] * (1.0 + spread)
        met = met and ok
        lines.append("%-24s %8d %8d | %12.1f %11.2f | %14.1f | %5.1f%% | %s" % (
            "%d x %d, %d x %d" % (B, N, h, w), counts[0], counts[1], med["subpixel"], counts[0] * 5 * 256.0 / med["subpixel"] * 1e-6,
            med["guided1"], 100.0 * spread, "met" if ok else "MISSED"))
    lines.append("subpixel = ops.match_subpixel on guided_match(radius=2)'s idx under its keep mask; guided r=1 = ops.guided_match(radius=1) "
                 "on the same selection; gather TB/s = matched rows x 5 x 256 B / time; requirement: subpixel <= guided r=1 x (1 + spread): "
                 + ("met at every shape" if met else "MISSED"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
