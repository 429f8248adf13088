#!/usr/bin/env python3
"""The two calls of DESIGN.md 4s against the compositions a user writes without them: HIP events after warm-up, the two sides timed
alternately in the same process, `--repeats` times: medians, and the largest |repeat - median| / median over both sides as the spread.

paint    single:  one ops.paint_points (cmr_paint_points_f32) call, bilinear: colours, painted flags and counts.
         compose: torch.matmul projection, rounding and the in-view test, grid_sample(bilinear, align_corners=True, padding_mode='border')
                  at the normalised projections, a masked fill -- the same colours from eager torch.
render   single:  one ops.render_points (cmr_render_points_f32) call: index, depth and attribute maps and counts.
         compose: projection, int64 keys (depth bits << 32 | row), scatter_reduce(amin) into a map of "empty", the minimum over the
                  (2 splat + 1)^2 shifted slices, the gathers of depth and attributes.
Before timing the two sides must agree on the rows and pixels the float64 restatement (tests/point_image_reference.py) calls decided:
painted flags and owners equal, colours within the restatement's bound of each other's float64 value.
Shapes: B = 8, N = 16384, ~40 % of the rows selected, maps 88 x 304 and 352 x 1216, C = 3, splat in {0, 2}; scenes: visibility_reference.scene.
python tools/point_image_bench.py [--iters 200] [--warmup 3] [--repeats 5] [--out profiles/point_image_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import point_image_reference as pir  # noqa: E402
import visibility_reference as vr  # noqa: E402
from cmr_agent_amd import ops  # noqa: E402

SHAPES = [(8, 16384, 88, 304), (8, 16384, 352, 1216)]
SPLATS = (0, 2)
C = 3


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
    lines = ["%-24s %-9s | %10s %11s %11s | %6s | %s" % ("shape B x N, h x w", "op", "single us", "compose us", "compose / 1", "spread", "counts; differing")]
    ok = True

    def row(shape, op, med, spread, note):
        faster = med["single"] * (1.0 + spread) < med["compose"] * (1.0 - spread)
        lines.append("%-24s %-9s | %10.1f %11.1f %11.2f | %5.1f%% | %s%s" % (
            "%d x %d, %d x %d" % shape, op, med["single"], med["compose"], med["compose"] / med["single"], 100.0 * spread, note,
            "" if faster else "   <- not faster by more than the spread"))
        return faster

    for B, N, h, w in SHAPES:
        sc = vr.scene(B, N, h, w, seed=41, selected=0.4)
        pts, pose, K, mask = f(sc["pts"]), f(sc["pose"]), f(sc["K"]), sc["mask"].to(dev)
        R, t = pose[:, :3, :3].contiguous(), pose[:, :3, 3:4].contiguous()
        g = torch.Generator().manual_seed(7)
        image = torch.rand(B, C, h, w, generator=g).to(dev)
        attr = torch.rand(B, C, N, generator=g).to(dev)
        rows = torch.arange(N, device=dev)[None]
        empty = torch.iinfo(torch.int64).max

        def project():
            p = torch.matmul(K, torch.matmul(R, pts) + t)
            z = p[:, 2]
            u, v = p[:, 0] / z, p[:, 1] / z
            cx, cy = torch.round(u), torch.round(v)
            view = mask & (z > 0) & torch.isfinite(u) & torch.isfinite(v) & (cx >= 0) & (cx <= w - 1) & (cy >= 0) & (cy <= h - 1)
            return u, v, z, cx, cy, view

        # ---- painting ----
        def compose_paint():
            u, v, z, cx, cy, view = project()
            grid = torch.stack([u * (2.0 / max(w - 1, 1)) - 1.0, v * (2.0 / max(h - 1, 1)) - 1.0], -1)
            grid = torch.where(view[..., None], grid, torch.zeros_like(grid))[:, None]                  # [B, 1, N, 2]
            val = torch.nn.functional.grid_sample(image, grid, mode="bilinear", padding_mode="border", align_corners=True)[:, :, 0]
            return torch.where(view[:, None], val, torch.zeros_like(val)), view

        single_paint = lambda: ops.paint_points(pts, pose, K, image, mask=mask)
        colors, painted, counts, _ = single_paint()
        other, oview = compose_paint()
        ref = pir.paint(sc["pts"], sc["mask"], sc["pose"], sc["K"], image.cpu())
        decided = torch.from_numpy(np.stack([x["decided"] for x in ref])).to(dev)
        want = torch.from_numpy(np.stack([x["painted"] for x in ref])).to(dev)
        assert not bool(((painted.view(B, N) != want) & decided).any()), "the op disagrees with float64 on a decided row"
        assert not bool(((oview != want) & decided).any()), "the composition disagrees with float64 on a decided row"
        c64 = torch.from_numpy(np.stack([x["bilinear"] for x in ref])).to(dev)
        bound = torch.from_numpy(np.stack([x["bound"] for x in ref])).to(dev)
        on = want[:, None].expand_as(c64)
        assert bool(((colors.double() - c64).abs() <= bound)[on].all()), "the op misses the float64 bound on a decided row"
        # grid_sample forms its own coordinates (u -> normalised -> back): allow it the same bound once more plus 2 G 4 ulp(w) of that detour
        assert bool(((other.double() - c64).abs() <= 2.0 * bound + 1e-4)[on].all()), "the composition is not the same interpolation"
        med, spread = _alternate([("single", single_paint, args.iters), ("compose", compose_paint, args.iters)], args.warmup, args.repeats)
        c = counts.sum(0).tolist()
        ok = row((B, N, h, w), "paint", med, spread, "selected %d, painted %d; undecided rows %d, painted flags that differ %d" % (
            c[0], c[1], sum(x["undecided"] for x in ref), int((painted.view(B, N) != oview).sum()))) and ok

        # ---- rendering ----
        for s in SPLATS:
            def compose_render():
                u, v, z, cx, cy, view = project()
                cell = torch.where(view, cy * w + cx, torch.zeros_like(cx)).long()
                key = (z.contiguous().view(torch.int32).long() << 32) | rows
                key = torch.where(view, key, torch.full_like(key, empty))
                km = torch.full((B, h * w), empty, dtype=torch.int64, device=dev).scatter_reduce(1, cell, key, "amin", include_self=True).view(B, h, w)
                if s:
                    pad = torch.full((B, h + 2 * s, w + 2 * s), empty, dtype=torch.int64, device=dev)
                    pad[:, s:s + h, s:s + w] = km
                    km = pad[:, 0:h, 0:w]
                    for dy in range(2 * s + 1):
                        for dx in range(2 * s + 1):
                            if dy or dx:
                                km = torch.minimum(km, pad[:, dy:dy + h, dx:dx + w])
                owned = (km != empty).view(B, h * w)
                own = torch.where(owned, km.view(B, h * w) & 0xffffffff, torch.zeros_like(owned, dtype=torch.int64))
                index = torch.where(owned, own, torch.full_like(own, -1)).int().view(B, h, w)
                depth = torch.where(owned, z.gather(1, own), torch.full_like(z[:, :1], float("inf")).expand(B, h * w)).view(B, h, w)
                amap = torch.where(owned[:, None], attr.gather(2, own[:, None].expand(B, C, h * w)), torch.zeros((), device=dev)).view(B, C, h, w)
                return index, depth, amap

            single_render = lambda: ops.render_points(pts, pose, K, h, w, attr=attr, mask=mask, splat=s)
            index_map, depth_map, attr_map, rcounts = single_render()
            oindex, odepth, oattr = compose_render()
            rref = pir.render(sc["pts"], sc["mask"], sc["pose"], sc["K"], h, w, s)
            idec = torch.from_numpy(np.stack([x["index_decided"] for x in rref])).to(dev)
            iwant = torch.from_numpy(np.stack([x["index"] for x in rref])).to(dev).int()
            assert not bool(((index_map != iwant) & idec).any()), "the op disagrees with float64 on a decided pixel"
            assert not bool(((oindex != iwant) & idec).any()), "the composition disagrees with float64 on a decided pixel"
            same = index_map == oindex
            assert bool((attr_map == oattr)[same[:, None].expand_as(oattr)].all()) and bool((same | ~idec).all())
            med, spread = _alternate([("single", single_render, args.iters), ("compose", compose_render, args.iters)], args.warmup, args.repeats)
            c = rcounts.sum(0).tolist()
            ok = row((B, N, h, w), "render s=%d" % s, med, spread, "selected %d, in view %d, owned pixels %d; owners that differ %d" % (
                c[0], c[1], c[2], int((~same).sum()))) and ok
    lines.append("single = one ops.paint_points / ops.render_points call; compose = the eager torch composition (matmul projection + grid_sample, or "
                 "int64 keys + scatter_reduce(amin) + shifted minima + gathers); compose / 1 = their ratio; spread = largest |repeat - median| / "
                 "median over both sides")
    lines.append("requirement (single faster than compose by more than the spread at every shape): %s" % ("met" if ok else "NOT met"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
