#!/usr/bin/env python3
"""The call of DESIGN.md 4v against what stood in its place: HIP events after warm-up, the two sides timed alternately in the same process,
`--repeats` times: medians, and the largest |repeat - median| / median over both sides as the spread.

single: one ops.pose_mi (cmr_pose_mi_f32) call scoring P poses per sample.
comp:   P x (ops.paint_points at C = 1 in the same mode + the bins in fp32 torch + torch.bincount) and the entropies in torch float64 --
        what the parent commit offers for the same numbers: per pose 2 launches of paint, a [B, N] colour vector written and read back,
        and a dozen elementwise launches.
Shapes: B = 8, N = 16384, images 88 x 304 and 352 x 1216, nb in {16, 32, 64}, both modes, P in {1, 27, 729}.  Geometry:
pose_mi_reference.equality_scene (a noise image, ~70 % of the rows selected, about half of those in view).  The histograms of the two
sides are asserted equal before anything is timed, and at P = 27 and P = 729 the run asserts single (1 + spread) < comp (1 - spread).
python tools/pose_mi_bench.py [--iters 10] [--warmup 2] [--repeats 5] [--out profiles/pose_mi_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pose_mi_reference as pmr  # noqa: E402
from cmr_agent_amd import ops  # noqa: E402

SHAPES = [(8, 16384, 88, 304), (8, 16384, 352, 1216)]
POSES = (1, 27, 729)
BINS = (16, 32, 64)
MODES = ("nearest", "bilinear")


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


def _clogc(c):
    c = c.double()
    return torch.where(c > 0, c * torch.log(c.clamp(min=1.0)), torch.zeros_like(c))


def composition(pts, attr, grey4, mask, each, K, nb, mode):
    """-> (hist int64 [B, P, nb, nb], mi float64 [B, P]) the parent's way; unit ranges."""
    B, _, N = pts.shape
    scale = float(np.float32(nb))
    base = torch.arange(B, device=pts.device)[:, None] * (nb * nb)
    hist = []
    for pose in each:
        colors, painted, _, _ = ops.paint_points(pts, pose, K, grey4, mask=mask, mode=mode)
        g = colors[:, 0]
        ok = painted.view(B, N) & torch.isfinite(attr) & torch.isfinite(g)
        zero = torch.zeros_like(g)
        ba = (torch.where(ok, attr, zero) * scale).floor().clamp(0, nb - 1)      # lo = 0: x - lo is x
        bg = (torch.where(ok, g, zero) * scale).floor().clamp(0, nb - 1)
        cell = torch.where(ok, base + (ba * nb + bg).long(), torch.full_like(base, B * nb * nb).expand(B, N))
        hist.append(torch.bincount(cell.reshape(-1), minlength=B * nb * nb + 1)[:-1].view(B, nb, nb))      # no boolean index: no host sync
    h = torch.stack(hist, 1)
    n = h.sum((2, 3)).double()
    ln = torch.log(n.clamp(min=1.0))
    den = n.clamp(min=1.0)
    ha = ln - _clogc(h.sum(3)).sum(2) / den
    hg = ln - _clogc(h.sum(2)).sum(2) / den
    hag = ln - _clogc(h).sum((2, 3)) / den
    return h, (ha + hg) - hag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)      # noqa: E731
    lines = ["%-24s %2s %-8s %4s | %10s %12s %8s | %6s | %s" % ("shape B x N, H x W", "nb", "mode", "P", "single us", "comp us", "comp / 1", "spread",
                                                               "selected, counted per pose")]
    failed = []
    for B, N, H, W in SHAPES:
        s = pmr.equality_scene(B, N, H, W, seed=51, P=3)
        pts, attr, grey, K, mask = f(s["pts"]), f(s["attr"]).clamp(-0.2, 1.2).nan_to_num(0.5), f(s["grey"]), f(s["K"]), torch.from_numpy(s["mask"]).to(dev)
        grey4 = grey[:, None].contiguous()
        rng = np.random.default_rng(5)
        truth = s["poses"][:, 0].astype(np.float64)
        allp = []
        for _ in range(max(POSES)):                                         # the truth turned by up to 1 degree about each axis, moved by up to 0.1
            a, t = rng.uniform(-1.0, 1.0, 3), rng.uniform(-0.1, 0.1, 3)
            D = pmr._rot("y", a[0]) @ pmr._rot("x", a[1]) @ pmr._rot("z", a[2])
            D[:3, 3] = t
            allp.append(D @ truth)
        allp = f(np.stack(allp, 1))
        for nb in BINS:
            for mode in MODES:
                for P in POSES:
                    poses = allp[:, :P].contiguous()
                    each = [poses[:, p].contiguous() for p in range(P)]
                    single = lambda: ops.pose_mi(pts, attr, grey, mask, poses, K, bins=nb, mode=mode, want_hist=True)      # noqa: E731
                    comp = lambda: composition(pts, attr, grey4, mask, each, K, nb, mode)                               # noqa: E731
                    mi, _, counts, selected, hist = single()
                    h0, mi0 = comp()
                    assert torch.equal(hist.long(), h0), "the two sides disagree on the histogram"
                    assert float((mi - mi0).abs().max()) <= 1e-10
                    med, spread = _alternate([("single", single, args.iters), ("comp", comp, max(1, args.iters // P))], args.warmup, args.repeats)
                    ok = P == 1 or med["single"] * (1 + spread) < med["comp"] * (1 - spread)
                    if not ok:
                        failed.append((B, N, H, W, nb, mode, P))
                    lines.append("%-24s %2d %-8s %4d | %10.1f %12.1f %8.2f | %5.1f%% | %d, %d%s" % (
                        "%d x %d, %d x %d" % (B, N, H, W), nb, mode, P, med["single"], med["comp"], med["comp"] / med["single"], 100.0 * spread,
                        int(selected.sum()), int(counts[..., 1].sum()) // P, "" if ok else "   <-- single is not faster"))
                    print(lines[-1], flush=True)
    lines.append("single = one ops.pose_mi call; comp = P x (ops.paint_points at C = 1 + bins + torch.bincount) + the entropies in torch float64; "
                 "comp / 1 = their ratio; spread = largest |repeat - median| / median")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    assert not failed, failed


if __name__ == "__main__":
    main()
