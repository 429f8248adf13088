#!/usr/bin/env python3
"""ops.feat_match (cmr_feat_match_f32: nearest pixel feature of every selected point + inlier counts) against torch's best formulation
on the same GPU (torch.cdist + argmin per sample, chunked so the distance block stays under 2 GiB), HIP events after warm-up, at the
three map sizes of the match evaluation.  Features are random unit vectors, the selection is the synthetic loader's pc_mask (points
that project into the image).  TFLOP/s counts 2 * 64 FLOP per (selected point, pixel) pair; the fraction is of the measured fp32 MFMA
peak, 155 TFLOP/s (profiles/r04_mfma_peak.txt).  "all rows us": the same call with every row selected (what the
selection saves: the kernel compacts the selected rows first, so its time follows the selected count).
python tools/match_bench.py [--iters 20] [--warmup 3]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cmr_agent_amd import ops  # noqa: E402
from cmr_agent_amd.utils import synthetic  # noqa: E402

SHAPES = [(8, 16384, 40, 128), (8, 65536, 88, 304), (4, 32768, 224, 400)]
PEAK_TF = 155.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(7)
    print("%-26s %9s %11s %11s %8s %11s %8s %8s %9s %13s" % ("shape B x N, h x w", "selected", "fused us", "TFLOP/s", "of peak", "cdist us",
                                                              "TFLOP/s", "speedup", "idx agree", "all rows us"))
    for B, N, h, w in SHAPES:
        raw = synthetic.make_raw(B, N, 4 * h, 4 * w, seed=11, n_circle=1)
        mask = torch.from_numpy(raw["pc_mask"]).to(dev).contiguous()                 # int64 [B, N]
        pc = torch.nn.functional.normalize(torch.randn(B * N, 64, generator=g), dim=1).to(dev)
        img = torch.nn.functional.normalize(torch.randn(B, h, w, 64, generator=g), dim=3).to(dev)
        nsel = int(mask.sum())
        flop = 2.0 * 64 * h * w * nsel
        fused = lambda: ops.feat_match(pc, img, mask)
        chunk = max(1, (1 << 29) // (h * w))

        def ref():
            out = []
            for b in range(B):
                p = pc[b * N:(b + 1) * N][mask[b].bool()]
                q = img[b].view(h * w, 64)
                out.append(torch.cat([torch.cdist(p[i:i + chunk], q).argmin(1) for i in range(0, p.shape[0], chunk)]))
            return out

        t_f = _time(fused, args.iters, args.warmup)
        t_r = _time(ref, max(2, args.iters // 4), 1)
        every = torch.ones_like(mask)
        t_all = _time(lambda: ops.feat_match(pc, img, every), args.iters, args.warmup)      # the same call with every row selected
        idx = fused()[0].view(B, N)
        want = ref()
        agree = sum(int((idx[b][mask[b].bool()].long() == want[b]).sum()) for b in range(B)) / max(nsel, 1)
        print("%-26s %9d %11.1f %11.1f %7.1f%% %11.1f %8.1f %7.2fx %9.6f %13.1f" % (
            "%d x %d, %d x %d" % (B, N, h, w), nsel, t_f, flop / t_f * 1e-6, 100.0 * flop / t_f * 1e-6 / PEAK_TF, t_r,
            flop / t_r * 1e-6, t_r / t_f, agree, t_all))


if __name__ == "__main__":
    main()
