"""Float64 restatement of the match filter (cmr_feat_match_filter_f32 / ops.feat_match_filter), written from the
contract in include/cmr_hip.h and independently of the kernel: direct argmin / masked min over explicit float64 distance blocks, no
matrix core layout, no compaction.  It is the yardstick of tests/test_match_filter_gpu.py and is itself checked, on planted scenes, by
tests/test_match_filter_cpu.py.

Per sample b: S = rows with mask != 0, d(n, p) = L2 distance of point feature n and pixel feature p (p = y * w + x);
  idx[n]  = argmin_p d(n, p), lowest p on a tie (-1 outside S);              d1[n] = that minimum (NaN outside S);
  d2[n]   = min of d(n, p) over the pixels with max(|x_p - x_best|, |y_p - y_best|) > excl_radius, +inf when there is none;
  rev[p]  = argmin over n in S of d(n, p) as a row number, lowest n on a tie; -1 when S is empty;
  keep[n] = n in S and (not mutual or rev[idx[n]] == n) and (ratio <= 0 or d1 <= ratio * d2) and (max_dist <= 0 or d1 <= max_dist);
  counts  = (|S|, kept, kept and inlier, selected and inlier); inlier: gt_xy finite and the best pixel within thr of it.
Beside the results it returns, per selected row, the three float64 margins a decision hangs on: the forward best / runner-up gap (plain
runner-up: it decides idx), the reverse gap at the row's best pixel (it decides rev[idx[n]]) and |d1 - ratio * d2| (it decides the ratio
test).  A kernel that rounds d^2 = |p|^2 + |q|^2 - 2 p.q in fp32 is compared only where all three are >= 1e-5."""
import math

import torch

TOL = 1e-5           # the margin under which an fp32 decision may differ from the float64 one (tests/test_feat_match_gpu.py's bar)
CAP = 0.005          # at most this share of a sample's selected rows may sit under TOL (a condition on the scenes, not a measurement)
ROW_CHUNK = 1024     # selected rows per float64 distance block


def _dist(P, Q):
    """[n, C] x [m, C] float64 -> [n, m] L2 distances.  Float64 throughout: the expanded form's rounding (~1e-15 on d^2, ~3e-8 on d at
    d = 0) is far below the 1e-5 bars."""
    return ((P * P).sum(1)[:, None] + (Q * Q).sum(1)[None, :] - 2.0 * (P @ Q.T)).clamp(min=0.0).sqrt()


def restate(pc, img, mask, mutual=True, ratio=0.0, excl_radius=2, max_dist=0.0, gt_xy=None, thr=3.0):
    """pc [B*N, C], img [B, h, w, C], mask [B, N] / [B*N], gt_xy [B, 2, N] or None (any float dtype / device) -> list over the samples
    of dict(sel [n_sel] rows, idx [N], d1 [N], d2 [N], rev [h*w], keep [N] bool, counts [4] ints, inlier [n_sel] bool, and the margins
    fwd_gap, rev_gap, ratio_gap [n_sel], near [n_sel] bool = any margin < TOL)."""
    B, h, w, C = img.shape
    N = pc.shape[0] // B
    dev = pc.device
    hw = h * w
    px = (torch.arange(hw, device=dev) % w)
    py = torch.div(torch.arange(hw, device=dev), w, rounding_mode="floor")
    out = []
    for b in range(B):
        sel = torch.nonzero(mask.reshape(B, N)[b] != 0).flatten()
        ns = sel.numel()
        Q = img[b].reshape(hw, C).double()
        idx = torch.full((N,), -1, dtype=torch.int64, device=dev)
        d1 = torch.full((N,), math.nan, dtype=torch.float64, device=dev)
        d2 = torch.full((N,), math.nan, dtype=torch.float64, device=dev)
        keep = torch.zeros(N, dtype=torch.bool, device=dev)
        rev = torch.full((hw,), -1, dtype=torch.int64, device=dev)
        inf = torch.full((hw,), math.inf, dtype=torch.float64, device=dev)
        rb, rs = inf.clone(), inf.clone()                             # per pixel: best and second-best distance over the selected rows
        fwd_gap = torch.full((ns,), math.inf, dtype=torch.float64, device=dev)
        best_s = torch.zeros(ns, dtype=torch.int64, device=dev)
        d1_s = torch.zeros(ns, dtype=torch.float64, device=dev)
        d2_s = torch.zeros(ns, dtype=torch.float64, device=dev)
        for c0 in range(0, ns, ROW_CHUNK):
            rows = sel[c0:c0 + ROW_CHUNK]
            d = _dist(pc[b * N:(b + 1) * N][rows].double(), Q)        # [c, hw]
            lo = d.min(1).values
            best = (d == lo[:, None]).to(torch.uint8).argmax(1)       # the FIRST pixel that attains the minimum
            if hw > 1:
                two = d.topk(2, dim=1, largest=False).values
                fwd_gap[c0:c0 + rows.numel()] = two[:, 1] - two[:, 0]
            inside = ((px[None, :] - px[best][:, None]).abs() <= excl_radius) & ((py[None, :] - py[best][:, None]).abs() <= excl_radius)
            second = d.masked_fill(inside, math.inf).min(1).values
            best_s[c0:c0 + rows.numel()], d1_s[c0:c0 + rows.numel()], d2_s[c0:c0 + rows.numel()] = best, lo, second
            # reverse direction: fold this block of rows into the per-pixel (best, second, argbest); an earlier block wins a tie
            clo = d.min(0).values
            carg = rows[(d == clo[None, :]).to(torch.uint8).argmax(0)]          # the lowest row of the block that attains it
            csec = d.topk(2, dim=0, largest=False).values[1] if rows.numel() > 1 else inf
            rs = torch.minimum(torch.minimum(torch.maximum(rb, clo), rs), csec)
            take = clo < rb
            rev = torch.where(take, carg, rev)
            rb = torch.minimum(rb, clo)
        idx[sel], d1[sel], d2[sel] = best_s, d1_s, d2_s
        rev_gap = (rs - rb)[best_s] if ns else fwd_gap
        rev_gap = torch.where(torch.isnan(rev_gap), torch.full_like(rev_gap, math.inf), rev_gap)
        if ratio > 0:
            ratio_gap = (d1_s - ratio * d2_s).abs()                   # inf where d2 is inf: the test passes with room
        else:
            ratio_gap = torch.full((ns,), math.inf, dtype=torch.float64, device=dev)
        k = torch.ones(ns, dtype=torch.bool, device=dev)
        if mutual:
            k &= rev[best_s] == sel
        if ratio > 0:
            k &= d1_s <= ratio * d2_s
        if max_dist > 0:
            k &= d1_s <= max_dist
        keep[sel] = k
        inl = torch.zeros(ns, dtype=torch.bool, device=dev)
        if gt_xy is not None and ns:
            gx, gy = gt_xy[b, 0, sel].double(), gt_xy[b, 1, sel].double()
            inl = torch.isfinite(gx) & torch.isfinite(gy) & (((px[best_s].double() - gx) ** 2 + (py[best_s].double() - gy) ** 2).sqrt() <= thr)
        near = (fwd_gap < TOL) | (rev_gap < TOL) | (ratio_gap < TOL)
        out.append(dict(sel=sel, idx=idx, d1=d1, d2=d2, rev=rev, keep=keep, inlier=inl,
                        counts=[ns, int(k.sum()), int((k & inl).sum()), int(inl.sum())],
                        fwd_gap=fwd_gap, rev_gap=rev_gap, ratio_gap=ratio_gap, near=near))
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def unit(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(*shape, generator=g, dtype=torch.float64), dim=-1).float()


def planted_scene(B, N, h, w, seed, noise=0.08, outlier_frac=0.5, select=0.4, blur=5):
    """A feature map whose neighbours resemble each other, and points that mostly belong to a pixel of it: unit pixel features, box-blurred
    blur x blur and renormalised; point n = the feature of a uniformly drawn pixel + noise * N(0, I), renormalised; a fraction outlier_frac
    of the points replaced by random unit vectors; about `select` of the rows selected.  gt_xy is the drawn pixel (also for the replaced
    points, whose match then lands within 3 px of it only by chance).
    -> dict(pc float32 [B*N, 64], img float32 [B, h, w, 64], mask int64 [B, N], gt_xy float32 [B, 2, N], planted bool [B, N])."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    img = torch.randn(B, h, w, 64, generator=g, dtype=torch.float64)
    if blur > 1:
        img = torch.nn.functional.avg_pool2d(img.permute(0, 3, 1, 2), blur, stride=1, padding=blur // 2, count_include_pad=False).permute(0, 2, 3, 1)
    img = torch.nn.functional.normalize(img, dim=-1)
    pix = torch.randint(0, h * w, (B, N), generator=g)
    feat = img.reshape(B, h * w, 64).gather(1, pix[..., None].expand(B, N, 64)) + noise * torch.randn(B, N, 64, generator=g, dtype=torch.float64)
    out = torch.rand(B, N, generator=g) < outlier_frac
    feat = torch.where(out[..., None], torch.randn(B, N, 64, generator=g, dtype=torch.float64), feat)
    feat = torch.nn.functional.normalize(feat, dim=-1)
    mask = (torch.rand(B, N, generator=g) < select).long()
    xy = torch.stack([pix % w, torch.div(pix, w, rounding_mode="floor")], 1).float()
    return dict(pc=feat.reshape(B * N, 64).float().contiguous(), img=img.float().contiguous(), mask=mask, gt_xy=xy.contiguous(), planted=~out)


def random_scene(B, N, h, w, seed, select=0.3):
    """Unrelated random unit features (the matcher's own kind of test scene), about `select` of the rows selected, uniform gt_xy."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    mask = (torch.rand(B, N, generator=g) < select).long()
    xy = (torch.rand(B, 2, N, generator=g) * torch.tensor([w, h]).view(1, 2, 1)).float()
    return dict(pc=unit(B * N, 64, seed=seed + 1), img=unit(B, h, w, 64, seed=seed + 2), mask=mask, gt_xy=xy.contiguous())


# The scenes of the GPU tier's float64 comparison, with the filter settings each is run under: (name, maker, kwargs of the maker,
# kwargs of the filter).  tests/test_match_filter_cpu.py asserts CAP on every one of them from the restatement alone.
SCENES = [
    ("planted_4097", planted_scene, dict(B=2, N=4097, h=40, w=128, seed=101), dict(mutual=True, ratio=0.9, excl_radius=2)),
    ("planted_16384", planted_scene, dict(B=1, N=16384, h=40, w=128, seed=102), dict(mutual=True, ratio=0.9, excl_radius=2)),
    ("planted_ratio_only", planted_scene, dict(B=2, N=4097, h=40, w=128, seed=103), dict(mutual=False, ratio=0.8, excl_radius=0)),
    ("planted_mutual_only", planted_scene, dict(B=2, N=4097, h=40, w=128, seed=104), dict(mutual=True, ratio=0.0, excl_radius=2)),
    ("random_88x304", random_scene, dict(B=2, N=4097, h=88, w=304, seed=105), dict(mutual=True, ratio=0.95, excl_radius=3)),
    ("random_11x38", random_scene, dict(B=3, N=1000, h=11, w=38, seed=106, select=1.0), dict(mutual=True, ratio=0.97, excl_radius=1)),
]
