"""Float64 restatement of the dual-softmax match confidence (cmr_match_conf_f32 / ops.match_conf), written from the
contract in include/cmr_hip.h and independently of the kernel: explicit float64 distance blocks and torch.logsumexp, no matrix core
layout, no online maximum, no compaction.  It is the yardstick of tests/test_match_conf_gpu.py and is itself checked by
tests/test_match_conf_cpu.py.  The scenes come from match_filter_reference (planted_scene / random_scene).

Per sample b: S = rows with mask != 0, d2(n, p) = squared L2 distance of point feature n and pixel feature p, s(n, p) = -d2(n, p) / T;
  idx[n]     = argmin_p d(n, p), lowest p on a tie (-1 outside S);       d1[n] = that minimum distance (NaN outside S);
  row_lse[n] = log sum over all h*w pixels p of exp s(n, p) (NaN outside S);
  col_lse[p] = log sum over n in S of exp s(n, p) (-inf when S is empty);
  conf[n]    = min(1, exp(2 s(n, idx[n]) - row_lse[n] - col_lse[idx[n]])) (NaN outside S);
  keep[n]    = n in S and (min_conf <= 0 or conf[n] >= min_conf);
  counts     = (|S|, kept, kept and inlier, selected and inlier); inlier: gt_xy finite and the best pixel within thr of it.
Beside the results it returns, per selected row, the two float64 margins a decision hangs on: the forward best / runner-up gap (on
distances, as match_filter_reference: it decides idx) and |log conf - log min_conf| (it decides keep).

The bound the GPU tier holds the kernel to (bound()): each s carries at most E = 68 * 2^-24 * (max|x| + max|q|)^2 / T of fp32 rounding
(the expanded form over 64 channels); a log-sum-exp of perturbed terms moves by at most the largest perturbation; any summation order of
n non-negative terms has relative error <= n * 2^-24.  Hence |log conf_device - log conf_float64| <= 4 E + (h*w + |S_b|) * 2^-24 + 1e-5
(the last term: exp2 / log2 and the final exp), and row_lse / col_lse stay within E + n * 2^-24 + 5e-6."""
import math

import torch

from match_filter_reference import planted_scene, random_scene  # noqa: F401  (re-exported: the scenes' makers)

GAP_TOL = 1e-5       # forward gap under which the fp32 argmin may differ from the float64 one (match_filter_reference.TOL)
CAP = 0.01           # at most this share of a sample's selected rows may be "near" (a condition on the scenes, not a measurement)
CONF_FLOOR = 1e-30   # log conf is compared on the rows whose float64 conf is at least this
ROW_CHUNK = 1024     # selected rows per float64 distance block
U = 2.0 ** -24


def eps_s(pc, img, T):
    """E: the fp32 rounding one s may carry, from the largest feature norms of the call."""
    return 68.0 * U * (float(pc.double().norm(dim=-1).max()) + float(img.double().norm(dim=-1).max())) ** 2 / T


def bound(E, hw, ns):
    """-> (bound on |log conf - float64|, on |row_lse - float64|, on |col_lse - float64|) for a sample with ns selected rows."""
    return 4.0 * E + (hw + ns) * U + 1e-5, E + hw * U + 5e-6, E + ns * U + 5e-6


def restate(pc, img, mask, temperature=0.1, min_conf=0.0, gt_xy=None, thr=3.0):
    """pc [B*N, C], img [B, h, w, C], mask [B, N] / [B*N], gt_xy [B, 2, N] or None (any float dtype / device) -> list over the samples
    of dict(sel [n_sel] rows, idx [N], d1 [N], row_lse [N], col_lse [h*w], conf [N], log_conf [N] (before the min with 1), keep [N] bool,
    counts [4] ints, inlier [n_sel] bool, the margins fwd_gap, conf_gap [n_sel], and near [n_sel] bool = fwd_gap < GAP_TOL or conf_gap
    within the sample's bound on log conf)."""
    B, h, w, C = img.shape
    N = pc.shape[0] // B
    dev = pc.device
    hw = h * w
    T = float(temperature)
    E = eps_s(pc, img, T)
    px = (torch.arange(hw, device=dev) % w)
    py = torch.div(torch.arange(hw, device=dev), w, rounding_mode="floor")
    out = []
    for b in range(B):
        sel = torch.nonzero(mask.reshape(B, N)[b] != 0).flatten()
        ns = sel.numel()
        Q = img[b].reshape(hw, C).double()
        nan = lambda n: torch.full((n,), math.nan, dtype=torch.float64, device=dev)
        idx = torch.full((N,), -1, dtype=torch.int64, device=dev)
        d1, row_lse, conf, log_conf = nan(N), nan(N), nan(N), nan(N)
        keep = torch.zeros(N, dtype=torch.bool, device=dev)
        col_lse = torch.full((hw,), -math.inf, dtype=torch.float64, device=dev)
        best_s = torch.zeros(ns, dtype=torch.int64, device=dev)
        s_best = torch.zeros(ns, dtype=torch.float64, device=dev)
        d1_s, rl_s = torch.zeros_like(s_best), torch.zeros_like(s_best)
        fwd_gap = torch.full((ns,), math.inf, dtype=torch.float64, device=dev)
        for c0 in range(0, ns, ROW_CHUNK):
            rows = sel[c0:c0 + ROW_CHUNK]
            P = pc[b * N:(b + 1) * N][rows].double()
            d2 = ((P[:, None, :] - Q[None, :, :]) ** 2).sum(2) if hw * rows.numel() <= 1 << 16 else \
                ((P * P).sum(1)[:, None] + (Q * Q).sum(1)[None, :] - 2.0 * (P @ Q.T)).clamp(min=0.0)
            s = -d2 / T                                               # [c, hw]
            lo = d2.min(1).values
            best = (d2 == lo[:, None]).to(torch.uint8).argmax(1)      # the FIRST pixel that attains the minimum
            if hw > 1:
                two = d2.sqrt().topk(2, dim=1, largest=False).values
                fwd_gap[c0:c0 + rows.numel()] = two[:, 1] - two[:, 0]
            k = slice(c0, c0 + rows.numel())
            best_s[k], d1_s[k], s_best[k], rl_s[k] = best, lo.sqrt(), -lo / T, torch.logsumexp(s, 1)
            col_lse = torch.logaddexp(col_lse, torch.logsumexp(s, 0))
        lc = 2.0 * s_best - rl_s - (col_lse[best_s] if ns else s_best)
        c = lc.exp().clamp(max=1.0)
        kp = torch.ones(ns, dtype=torch.bool, device=dev) if min_conf <= 0 else c >= min_conf
        idx[sel], d1[sel], row_lse[sel], conf[sel], log_conf[sel], keep[sel] = best_s, d1_s, rl_s, c, lc, kp
        inl = torch.zeros(ns, dtype=torch.bool, device=dev)
        if gt_xy is not None and ns:
            gx, gy = gt_xy[b, 0, sel].double(), gt_xy[b, 1, sel].double()
            inl = torch.isfinite(gx) & torch.isfinite(gy) & (((px[best_s].double() - gx) ** 2 + (py[best_s].double() - gy) ** 2).sqrt() <= thr)
        if min_conf > 0:
            conf_gap = (lc - math.log(min_conf)).abs()
        else:
            conf_gap = torch.full((ns,), math.inf, dtype=torch.float64, device=dev)
        near = (fwd_gap < GAP_TOL) | (conf_gap <= bound(E, hw, ns)[0])
        out.append(dict(sel=sel, idx=idx, d1=d1, row_lse=row_lse, col_lse=col_lse, conf=conf, log_conf=log_conf, keep=keep, inlier=inl,
                        counts=[ns, int(kp.sum()), int((kp & inl).sum()), int(inl.sum())], fwd_gap=fwd_gap, conf_gap=conf_gap,
                        near=near, E=E))
    return out


# The scenes of the GPU tier's float64 comparison: (name, maker, kwargs of the maker, kwargs of the call).  tests/test_match_conf_cpu.py
# asserts CAP on every one of them from the restatement alone.  The last three are the smallest at which the kernel can go wrong: 418 and
# 96 pixels are no multiple of the 64-pixel tile, 300 and 1000 rows straddle the 256-query workgroup, B is odd in one; 88 x 304
# exercises the splits.
SCENES = [
    ("planted_4097", planted_scene, dict(B=2, N=4097, h=40, w=128, seed=201), dict(temperature=0.1, min_conf=0.05)),
    ("planted_16384", planted_scene, dict(B=1, N=16384, h=40, w=128, seed=202), dict(temperature=0.1, min_conf=0.05)),
    ("planted_sharp", planted_scene, dict(B=2, N=4097, h=40, w=128, seed=203), dict(temperature=0.05, min_conf=0.2)),
    ("random_88x304", random_scene, dict(B=2, N=4097, h=88, w=304, seed=205), dict(temperature=0.1, min_conf=0.01)),
    ("random_11x38", random_scene, dict(B=3, N=1000, h=11, w=38, seed=206, select=1.0), dict(temperature=0.1, min_conf=0.01)),
    ("random_8x12", random_scene, dict(B=2, N=300, h=8, w=12, seed=207, select=1.0), dict(temperature=0.2, min_conf=0.003)),
]
