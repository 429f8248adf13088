"""Tensor-level wrappers over the C ABI (include/cmr_hip.h).  PyTorch is used for device
memory and the current HIP stream only; every computation is a HIP kernel.  Arguments are
2-D row views ([rows, C], unit inner stride, arbitrary row stride) unless stated otherwise."""
import collections
import math
import os

import numpy as np
import torch

from . import _lib

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_GELU, ACT_ELU1 = 0, 1, 2, 3, 4
f32 = torch.float32
GRID_Y_MAX = 65535          # groups / samples that ride in gridDim.y: entry points refuse more (CMR_EINVAL), callers chunk


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _rows(t, name="tensor"):
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype != f32 or not t.is_cuda:
        raise ValueError("%s must be a 2-D float32 device tensor with unit inner stride, got %s %s %s" % (
            name, tuple(t.shape), t.stride(), t.dtype))
    return t


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _i32(t):
    if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
        raise ValueError("row-id tensors must be contiguous int32")
    return t


LINEAR_BF16 = os.environ.get("CMR_LINEAR_BF16", "1") != "0"            # with CONV_BF16: contiguous row maps of at least LINEAR_BF16_MIN_ROWS rows through cmr_linear_rows_bf16_f32
LINEAR_BF16_MIN_ROWS = 16384
# with CONV_BF16: the train-mode [linear + BatchNorm] layers on the big row maps (cmr_linear_bn_fwd_f32 / cmr_bn_linear_bwd_f32) CAN take their
# products on the bf16 matrix cores too (cmr_linear_bn_fwd_bf16_f32 / cmr_bn_linear_bwd_bf16_f32; fp32 maps, statistics and accumulation;
# independent of fp32_linears(), which keeps the plain row GEMMs of the training updates in fp32).  Both are OFF in the product, by measurement
# (round 6):
#   forward  -- not faster than the fp32 kernel (both stream at ~2.5 TB/s alone, profiles/r06_bn_linear_bf16_bench.txt) and its logit shift
#               moves the 2-D tower's weakest gradient cosine from 0.976 to 0.969, under the 0.97 bar of tests/test_train_gpu.py;
#   backward -- 1.2 - 1.6 x faster alone (65 / 43 us against 102 / 52 us), -0.1 ms of the 3.4 ms update, gradients at cosine 0.99999 with
#               the fp32 ones (profiles/r06_bnl_grad_cosines.txt) -- but the 40-update trajectory test ends at a total loss of 0.216 against
#               the fp32 run's 0.192 (bar: 5 %; fp32-equivalent summation orders spread that final loss by +- 2 %): the bar decides.
BN_LINEAR_BF16_FWD = os.environ.get("CMR_BN_LINEAR_BF16_FWD", "0") != "0"
BN_LINEAR_BF16_BWD = os.environ.get("CMR_BN_LINEAR_BF16_BWD", "0") != "0"


class fp32_linears:
    """with fp32_linears(): row GEMMs stay on cmr_linear_f32 whatever the mode -- the training updates (bf16 mode there means the
    convolutions: forward, data and weight gradients; the 1x1 stacks and their gradients are fp32)."""

    def __enter__(self):
        global LINEAR_BF16
        self.old, LINEAR_BF16 = LINEAR_BF16, False

    def __exit__(self, *a):
        global LINEAR_BF16
        LINEAR_BF16 = self.old


def linear(x1, w, bias=None, x2=None, idx2=None, div2=1, res=None, res_mod=0, act=ACT_NONE, act_param=0.0, out=None):
    _rows(x1, "x1")
    rows, k1 = x1.shape
    n_out, kw = w.shape
    k2 = 0
    if x2 is not None:
        _rows(x2, "x2")
        k2 = x2.shape[1]
    if kw != k1 + k2 or w.stride(1) != 1 or w.stride(0) < kw:
        raise ValueError("weight shape %s / strides %s do not match k1+k2=%d" % (tuple(w.shape), w.stride(), k1 + k2))
    ldw = w.stride(0) if n_out > 1 else kw                     # a column block of a wider matrix (W[:, lo:hi]) is read in place
    if out is None:
        out = torch.empty((rows, n_out), dtype=f32, device=x1.device)
    _rows(out, "out")
    if res is not None:
        _rows(res, "res")
    if CONV_BF16 and LINEAR_BF16 and x2 is None and ldw == kw and rows >= LINEAR_BF16_MIN_ROWS and k1 in (32, 64, 128) and n_out <= 128 and n_out % 4 == 0:
        # bf16 mode: the big row maps stream through the bf16 cores (the fp32 kernel is bound by its MFMA chain at these shapes)
        rc = _lib.call("cmr_linear_rows_bf16_f32", _p(x1), _ld(x1), k1, _p(w), kw, _p(bias), _p(res), _ld(res) if res is not None else 0,
                       int(res_mod), _p(out), _ld(out), rows, n_out, act, float(act_param), _stream(), allow_unsupported=True)
        if rc != _lib.UNSUPPORTED:
            return out
    _lib.call("cmr_linear_f32", _p(x1), _ld(x1), k1, _p(x2), _ld(x2) if x2 is not None else 0, k2, _p(_i32(idx2)),
              int(div2), _p(w), ldw, _p(bias), _p(res), _ld(res) if res is not None else 0, int(res_mod), _p(out),
              _ld(out), rows, n_out, act, float(act_param), _stream())
    return out


def cbr_block(x1, w1, b1, w2, b2, wsc, slope, x2=None, idx2=None, div2=1, rows_per_batch=None, want_y=True,
              want_colmax=False):
    """Fused ConvBNReLURes1D block.  b1 / b2: [C] shared or [B, C] per batch.  Returns (y or None,
    colmax [B, co] or None), or None when the shape is not instantiated (caller composes linears)."""
    _rows(x1, "x1")
    rows, k1 = x1.shape
    kx = k1 + (x2.shape[1] if x2 is not None else 0)
    ch, co = w1.shape[0], w2.shape[0]
    if w1.shape[1] != kx or w2.shape[1] != ch or (wsc is not None and tuple(wsc.shape) != (co, kx)):
        raise ValueError("cbr_block: inconsistent weight shapes")
    rpb = rows if rows_per_batch is None else rows_per_batch
    B = rows // rpb
    if want_colmax and (rpb % 32 or rows % rpb):
        return None
    y = torch.empty((rows, co), dtype=f32, device=x1.device) if want_y else None
    ntiles = (rows + 31) // 32
    part = torch.empty((ntiles, co), dtype=f32, device=x1.device) if want_colmax else None
    s1 = b1.stride(0) if b1.dim() == 2 else 0
    s2 = b2.stride(0) if b2.dim() == 2 else 0
    rc = _lib.call("cmr_cbr_block_bf16_f32" if CONV_BF16 else "cmr_cbr_block_f32", _p(x1), _ld(x1), k1, _p(x2), _ld(x2) if x2 is not None else 0, _p(_i32(idx2)),
                   int(div2), kx, ch, co, _p(w1), _p(b1), s1, _p(w2), _p(b2), s2, _p(wsc), _p(y), co, _p(part), rows, rpb,
                   float(slope), _stream(), allow_unsupported=True)
    if rc == _lib.UNSUPPORTED:
        return None
    cm = None
    if want_colmax == "partials":                # the per-tile maxima themselves: colmax_bias2 / colmax_partials finish them
        return y, part
    if want_colmax:
        cm = colmax_partials(part, B, rpb // 32)
    return y, cm


def colmax_partials(part, B, tiles_per_batch):
    """part [B * tiles_per_batch, C] per-tile maxima of a block kernel -> [B, C]."""
    co = part.shape[1]
    cm = torch.empty((B, co), dtype=f32, device=part.device)
    _lib.call("cmr_colmax_partials_f32", _p(part), _p(cm), B, int(tiles_per_batch), co, _stream())
    return cm


# fp32 mode only, by measurement (profiles/r06_ab_glue.txt, same box, alternating): headline 19.54 -> 19.43 ms per registration with the glue
# launch, but the bf16-mode lines LOSE 1.5 % (c3 12.42 -> 12.60 ms, c1 in bf16 mode 8.93 -> 9.06 ms): under the bf16 convolutions the three
# small launches (25 + 2 x 9 us in the graph) find room next to the persistent workgroups sooner than one 1024-thread workgroup per sample does.
# CMR_COLMAX_BIAS2=0 / 1 forces it off / on in both modes.
COLMAX_BIAS2 = os.environ.get("CMR_COLMAX_BIAS2", "fp32")


def colmax_bias2(part, B, tiles_per_batch, w1, b1, w2, b2, want_g=False):
    """The glue between two blocks of the agent's 3-D branch in one launch: column maxima g [B, 64] of the per-tile maxima `part`, and the
    per-sample bias rows g w1^T + b1 [B, n1], g w2^T + b2 [B, n2] of the next block.  -> (y1, y2, g or None), or None when not served."""
    C = part.shape[1]
    n1, n2 = w1.shape[0], w2.shape[0]
    if COLMAX_BIAS2 == "0" or (COLMAX_BIAS2 == "fp32" and CONV_BF16) or C != 64 or n1 % 4 or n2 % 4 or not (w1.is_contiguous() and w2.is_contiguous()) or w1.shape[1] != C or w2.shape[1] != C:
        return None
    y1 = torch.empty((B, n1), dtype=f32, device=part.device)
    y2 = torch.empty((B, n2), dtype=f32, device=part.device)
    g = torch.empty((B, C), dtype=f32, device=part.device) if want_g else None
    rc = _lib.call("cmr_colmax_bias2_f32", _p(part), B, int(tiles_per_batch), C, _p(w1), _p(b1), n1, _p(w2), _p(b2), n2, _p(g), _p(y1), _p(y2), _stream(),
                   allow_unsupported=True)
    return None if rc == _lib.UNSUPPORTED else (y1, y2, g)


def layernorm64(x, gamma, beta, eps, res=None, out=None):
    _rows(x, "x")
    if out is None:
        out = torch.empty((x.shape[0], 64), dtype=f32, device=x.device)
    _lib.call("cmr_layernorm64_f32", _p(x), _ld(x), _p(gamma), _p(beta), float(eps), _p(res),
              _ld(res) if res is not None else 0, _p(out), _ld(out), x.shape[0], _stream())
    return out


CONV_BF16 = False        # True: bf16 mode -- 3x3 convolutions (cmr_conv3x3_bf16_nhwc_f32), ConvBNReLURes1D blocks (cmr_cbr_block_bf16_f32)
                         # and the query side of the linear-attention layers (cmr_la_query_layer_bf16_f32) run on the bf16 matrix cores
                         # where served; storage and everything else stay fp32
BF16_CHAINS = True       # bf16 mode: a convolution whose output only feeds another bf16 convolution stores it as bf16 (bit-identical, half the bytes)
BF16_STORE = True        # bf16 mode: the full- and half-resolution maps of the image tower (read only by bf16 convolutions, as input and as the
                         # residual of their own block) are STORED as bf16; not bit-neutral (the residual enters the epilogue rounded to bf16)
STRIDE2_FRAGS = True     # stride-2 convolutions (Cin = 64) on the fragment-weight kernel cmr_conv3x3_s2_nhwc_f32; False = the tiled kernel (A/B, tests)
WINOGRAD = True          # stride-1 convolutions on maps with enough 8x16 tiles go through Winograd F(2x2,3x3)
WINO_MIN_TILES = 64      # below that (11x38 at B < 6 ...) the per-wave direct kernel has more parallelism


TOWER_CU_BUDGET = 160    # bf16 mode: CUs of the image tower's persistent convolution kernels while the point tower runs beside it (0 = all)
TOWER_CU_BUDGET_F32 = 0  # the same for the fp32 Winograd kernels: matrix-bound, within noise at 240 / 224 / 208 (two boxes) -- left alone


TOWER_SLICES_F32 = int(os.environ.get("CMR_TOWER_SLICES", "1"))     # fp32: workgroups per CU of the image tower's Winograd launches while the point tower runs beside it


# Launch policy of the persistent convolution kernels: ARGUMENTS of every call (the library keeps no state); the host side keeps the current
# values per thread, set for the extent of a `with` block by the code that forks a concurrent branch.
import threading

_policy = threading.local()


def _cu_budget():
    return getattr(_policy, "cu_budget", 0)


def _slices():
    return getattr(_policy, "slices", 1)


class conv_slices:
    """with conv_slices(n): the persistent Winograd launches inside are split into n workgroups per CU (`slices` argument of
    cmr_conv3x3_wino_nhwc_f32)."""

    def __init__(self, n):
        self.n = max(1, int(n))

    def __enter__(self):
        self.old, _policy.slices = _slices(), self.n

    def __exit__(self, *a):
        _policy.slices = self.old


class conv_cu_budget:
    """with conv_cu_budget(n): the persistent convolution kernels launched inside occupy at most n CUs (`cu_budget` argument of the
    convolution entry points; 0 = all)."""

    def __init__(self, cus):
        self.cus = max(0, int(cus))

    def __enter__(self):
        self.old, _policy.cu_budget = _cu_budget(), self.cus

    def __exit__(self, *a):
        _policy.cu_budget = self.old


def conv3x3_wino(x, u, bias, cout, slope=1.0, res=None, post=None, pool=1):
    """Stride-1 3x3 convolution through the fused Winograd F(2x2,3x3) kernel; u [16,Cout,Cin] = G g G^T."""
    B, H, W, cin = x.shape
    if pool == 2 and (res is not None or post is not None):
        raise ValueError("conv3x3: pool=2 cannot be combined with res / post")
    if not x.is_contiguous() or tuple(u.shape) != (16, cout, cin):
        raise ValueError("conv3x3_wino: bad operand layout")
    hp, wp = (H // 2, W // 2) if pool == 2 else (H, W)
    y = torch.empty((B, hp, wp, cout), dtype=f32, device=x.device)
    _lib.call("cmr_conv3x3_wino_nhwc_f32", _p(x), B, H, W, cin, _p(u), _p(bias), _p(res), _p(post), _p(y), cout,
              float(slope), pool, _cu_budget(), _slices(), _stream())
    return y


def wino_list_served(B, H, W, cin, cout):
    """Shapes cmr_conv3x3_wino_list_nhwc_f32 serves: those the dense call runs on the persistent Winograd kernel."""
    return WINOGRAD and cin >= 64 and cin % 32 == 0 and cout % 64 == 0 and ((W + 15) // 16) * ((H + 7) // 8) * B * (cout // 64) >= max(200, WINO_MIN_TILES)


def conv3x3_wino_list(x, u, bias, cout, slope, order, nlive, y0, res=None, pool=1, nend=None):
    """conv3x3_wino on the virtual tiles order[:nlive] (device tensors, see wino_tile_lists); the other tiles are copied from y0, the result
    on an all-zero x -- or, with y0 None (pool 1), computed as act(bias + res), which IS that result.  nend (device int32 [1], see
    wino_tile_lists_staged): only order[nlive:nend] are copied; the tiles behind are left as torch.empty made them."""
    B, H, W, cin = x.shape
    hp, wp = (H // 2, W // 2) if pool == 2 else (H, W)
    ntiles = ((W + 15) // 16) * ((H + 7) // 8) * B * (cout // 64)
    if not x.is_contiguous() or x.dtype != f32 or tuple(u.shape) != (16, cout, cin):
        raise ValueError("conv3x3_wino_list: bad operand layout")
    if order.dtype != torch.int32 or nlive.dtype != torch.int32 or order.numel() != ntiles or nlive.numel() != 1 or not order.is_contiguous():
        raise ValueError("conv3x3_wino_list: order must be int32 [%d] and nlive int32 [1]" % ntiles)
    if nend is not None and (nend.dtype != torch.int32 or nend.numel() != 1):
        raise ValueError("conv3x3_wino_list: nend must be int32 [1]")
    if (y0 is not None and (tuple(y0.shape) != (B, hp, wp, cout) or not y0.is_contiguous() or y0.dtype != f32)) or (
            res is not None and (tuple(res.shape) != (B, H, W, cout) or not res.is_contiguous() or res.dtype != f32)):
        raise ValueError("conv3x3_wino_list: y0 / res of the wrong shape")
    y = torch.empty((B, hp, wp, cout), dtype=f32, device=x.device)
    if nend is not None:
        _lib.call("cmr_conv3x3_wino_list_nend_nhwc_f32", _p(x), B, H, W, cin, _p(u), _p(bias), _p(res), _p(y), cout, float(slope), pool,
                  _p(order), _p(nlive), _p(nend), _p(y0), _cu_budget(), _slices(), _stream())
        return y
    _lib.call("cmr_conv3x3_wino_list_nhwc_f32", _p(x), B, H, W, cin, _p(u), _p(bias), _p(res), _p(y), cout, float(slope), pool, _p(order),
              _p(nlive), _p(y0), _cu_budget(), _slices(), _stream())
    return y


def wino_tile_lists(reach, B, H, W, cout1, cout2):
    """reach uint8 [2, B, ceil(H/8), ceil(W/16)] (observation_proj marks it; cleared here) -> ((order1, nlive1), (order2, nlive2)) for two
    chained list convolutions of cout1 / cout2 channels: live virtual tiles first, ascending, then the others."""
    nt = B * ((H + 7) // 8) * ((W + 15) // 16)
    if reach.dtype != torch.uint8 or reach.numel() != 2 * nt or not reach.is_contiguous():
        raise ValueError("wino_tile_lists: reach must be uint8 [2, %d]" % nt)
    n1, n2 = nt * (cout1 // 64), nt * (cout2 // 64)
    buf = torch.empty((n1 + n2 + 8,), dtype=torch.int32, device=reach.device)
    o1, o2, l1, l2 = buf[:n1], buf[n1:n1 + n2], buf[n1 + n2:n1 + n2 + 1], buf[n1 + n2 + 4:n1 + n2 + 5]
    _lib.call("cmr_wino_tile_lists", _p(reach), reach.data_ptr() + nt, B, H, W, cout1, cout2, _p(o1), _p(l1), _p(o2), _p(l2), _stream())
    return (o1, l1), (o2, l2)


def wino_tile_lists_staged(reach, B, H, W, cout0, cout1):
    """reach: the four maps observation_proj marks, flat uint8 (2 full-resolution maps, then 2 of the half-resolution stage; cleared here)
    -> ((order, nlive, nend) of stage 0's first convolution, (order, nlive) of its second, the same two of stage 1).  A first list is
    live | copy | rest (see cmr_wino_tile_lists_staged): nend = live + copy ends what its convolution has to write."""
    nt, nt1 = reach_tiles(B, H, W)
    if reach.dtype != torch.uint8 or reach.numel() != 2 * nt + 2 * nt1 or not reach.is_contiguous() or H % 2 or W % 2:
        raise ValueError("wino_tile_lists_staged: reach must be uint8 [2 * %d + 2 * %d] and H, W even" % (nt, nt1))
    n0, n1 = nt * (cout0 // 64), nt1 * (cout1 // 64)
    buf = torch.empty((2 * n0 + 2 * n1 + 8,), dtype=torch.int32, device=reach.device)
    o = [buf[:n0], buf[n0:2 * n0], buf[2 * n0:2 * n0 + n1], buf[2 * n0 + n1:2 * n0 + 2 * n1]]
    c = buf[2 * n0 + 2 * n1:]
    a = reach.data_ptr()
    _lib.call("cmr_wino_tile_lists_staged", a, a + nt, a + 2 * nt, a + 2 * nt + nt1, B, H, W, cout0, cout1, _p(o[0]), _p(o[1]), _p(o[2]),
              _p(o[3]), _p(c), _stream())
    return (o[0], c[0:1], c[1:2]), (o[1], c[2:3]), (o[2], c[3:4], c[4:5]), (o[3], c[5:6])


def conv3x3_wino_stats(x, u, bias, cout):
    """conv3x3 (stride 1, + bias, nothing else) through the wave-specialised Winograd kernel WITH the BatchNorm sums of its output from the
    kernel's own epilogue -> (y [B,H,W,Cout], part [parts, 2, Cout]) for bn_stats_from_sums (pivot = bias), or None where not served."""
    B, H, W, cin = x.shape
    if not (WINOGRAD and u is not None and x.dtype == f32 and x.is_contiguous() and tuple(u.shape) == (16, cout, cin)):
        return None
    parts = int(_lib.load().cmr_conv3x3_wino_stats_parts(B, H, W, cin, cout, _cu_budget(), _slices()))
    if parts <= 0:
        return None
    y = torch.empty((B, H, W, cout), dtype=f32, device=x.device)
    part = torch.empty((parts, 2, cout), dtype=f32, device=x.device)
    _lib.call("cmr_conv3x3_wino_stats_nhwc_f32", _p(x), B, H, W, cin, _p(u), _p(bias), _p(y), cout, _cu_budget(), _slices(), _p(part), parts, _stream())
    return y, part


def conv3x3_wino_bnbwd(dy, u, cout, bn_x, stat, slope):
    """Data gradient conv3x3(dy; u) of a convolution whose input was lrelu_slope(BatchNorm(bn_x)) (stat = that layer's [4, cout]) WITH the two
    sums of the BatchNorm's backward reduction from the kernel's epilogue -> (dx [B,H,W,cout], part [parts, 2, cout]) for bn_bwd_from_sums,
    or None where not served."""
    B, H, W, cin = dy.shape
    if not (WINOGRAD and u is not None and dy.is_contiguous() and bn_x.is_contiguous() and tuple(u.shape) == (16, cout, cin)
            and tuple(bn_x.shape) == (B, H, W, cout) and tuple(stat.shape) == (4, cout) and 0.0 <= slope <= 1.0):
        return None
    parts = int(_lib.load().cmr_conv3x3_wino_stats_parts(B, H, W, cin, cout, _cu_budget(), _slices()))
    if parts <= 0:
        return None
    dx = torch.empty((B, H, W, cout), dtype=f32, device=dy.device)
    part = torch.empty((parts, 2, cout), dtype=f32, device=dy.device)
    rc = _lib.call("cmr_conv3x3_wino_bnbwd_nhwc_f32", _p(dy), B, H, W, cin, _p(u), _p(dx), cout, _p(bn_x), _p(stat), float(slope), _cu_budget(),
                   _slices(), _p(part), parts, _stream(), allow_unsupported=True)
    return None if rc == _lib.UNSUPPORTED else (dx, part)          # (the library is built without this form by default: CMR_WS_BNBWD)


def bn_bwd_from_sums(dz, slope, x, stat, part, dgamma=None, dbeta=None):
    """bn_bwd(dz, None, slope, x, stat) with the reduction's partial sums given (conv3x3_wino_bnbwd) -> dx [rows, C]."""
    _rows(dz), _rows(x)
    rows, C = x.shape
    out = torch.empty((rows, C), dtype=f32, device=x.device)
    ws = _ws(8 * C, x.device)
    _lib.call("cmr_bn_bwd_from_sums_f32", _p(dz), _ld(dz), float(slope), _p(x), _ld(x), _p(stat), _p(part), part.shape[0], _p(out), _ld(out),
              _p(dgamma), _p(dbeta), rows, C, _p(ws), 8 * C, _stream())
    return out


def bn_stats_from_sums(part, rows, pivot, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1):
    """-> stat [4, C] (mean, rstd, scale, shift) from a producer's partial sums [parts, 2, C] of (x - pivot), (x - pivot)^2 (conv3x3_wino_stats);
    running statistics updated as bn_stats does."""
    parts, _, C = part.shape
    stat = torch.empty((4, C), dtype=f32, device=part.device)
    _lib.call("cmr_bn_stats_from_sums_f32", _p(part), parts, int(rows), C, _p(pivot), float(eps), float(momentum), _p(gamma), _p(beta),
              _p(running_mean), _p(running_var), _p(stat), _stream())
    return stat


def conv3x3_bf16(x, frags, bias, cout, slope=1.0, res=None, post=None, pool=1, stride=1, out_bf16=False):
    """3x3 convolution (stride 1 | 2) on the bf16 matrix cores; frags = (bf16 fragment tensor, nt) from _pack.conv_bf16_frags.  x is fp32 or
    bf16 NHWC (a bf16 x is the output of another bf16 convolution); out_bf16: store the result as bf16 (for a following bf16 convolution:
    that one would round fp32 to the same values).  Returns None when the library does not serve the shape (the caller falls back to the
    fp32 kernels -- impossible once x is bf16, which raises instead)."""
    B, H, W, cin = x.shape
    wf, nt = frags
    xb = x.dtype == torch.bfloat16
    if not x.is_contiguous() or wf.dtype != torch.bfloat16 or wf.numel() != 9 * cin * cout or x.dtype not in (f32, torch.bfloat16):
        raise ValueError("conv3x3_bf16: bad operand layout")
    if pool == 2 and (res is not None or post is not None):
        raise ValueError("conv3x3: pool=2 cannot be combined with res / post")
    rb = res is not None and res.dtype == torch.bfloat16          # bf16-stored towers: the block input is the residual, as bf16
    unserved = (pool == 2 and (H % 2 or W % 2)) or (stride == 2 and (pool != 1 or cin != 64)) or ((xb or out_bf16) and post is not None)
    if not unserved:
        hp, wp = (H // 2, W // 2) if pool == 2 else ((H - 1) // stride + 1, (W - 1) // stride + 1)
        y = torch.empty((B, hp, wp, cout), dtype=torch.bfloat16 if out_bf16 else f32, device=x.device)
        if xb or out_bf16 or rb:
            rc = _lib.call("cmr_conv3x3_bf16io_nhwc", _p(x), int(xb), B, H, W, cin, _p(wf), nt, _p(bias), _p(res), int(rb), _p(post), _p(y),
                           int(out_bf16), cout, int(stride), float(slope), pool, _cu_budget(), _stream(), allow_unsupported=True)
        else:
            rc = _lib.call("cmr_conv3x3_bf16_nhwc_f32", _p(x), B, H, W, cin, _p(wf), nt, _p(bias), _p(res), _p(post), _p(y), cout, int(stride),
                           float(slope), pool, _cu_budget(), _stream(), allow_unsupported=True)
        if rc != _lib.UNSUPPORTED:
            return y
    if xb or rb:
        raise ValueError("conv3x3_bf16: bf16 operands of shape %s (stride %d, pool %d, bf16 residual %s) are not served" % (tuple(x.shape), stride, pool, rb))
    return None


def conv3x3_bn_pro(x, in_scale, in_shift, in_slope, bias, cout, slope, u):
    """conv3x3(lrelu_{in_slope}(x * in_scale + in_shift)) + bias, LeakyReLU(slope), with the affine + activation applied in the convolution's
    staging pass (bf16 mode, matrix-class kernel): bit-identical to affine_act + conv3x3.  None where not served."""
    B, H, W, cin = x.shape
    fr = getattr(u, "bf16", None)
    if not (CONV_BF16 and fr is not None and x.dtype == f32 and x.is_contiguous() and cin == 128 and in_scale.numel() == cin and in_shift.numel() == cin):
        return None
    wf, nt = fr
    y = torch.empty((B, H, W, cout), dtype=f32, device=x.device)
    rc = _lib.call("cmr_conv3x3_bf16_pro_nhwc_f32", _p(x), _p(in_scale), _p(in_shift), float(in_slope), B, H, W, cin, _p(wf), nt, _p(bias), _p(y),
                   cout, float(slope), _cu_budget(), _stream(), allow_unsupported=True)
    return None if rc == _lib.UNSUPPORTED else y


def conv3x3(x, w9, bias, cout, stride=1, slope=1.0, res=None, post=None, out=None, pool=1, u=None, out_bf16=False):
    """x [B,H,W,Cin] contiguous NHWC; w9 [9,Cout,Cin]; returns [B,Ho,Wo,Cout] (or the 2x2 average-pooled
    map when pool=2: fused into the conv epilogue where the tiled kernel runs, a second kernel otherwise).
    u [16,Cout,Cin] (= G g G^T) enables the Winograd kernel for stride 1."""
    B, H, W, cin = x.shape
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if not x.is_contiguous() or tuple(w9.shape) != (9, cout, cin):
        raise ValueError("conv3x3: bad operand layout")
    if x.dtype == torch.bfloat16:                           # the output of a bf16 convolution: only a bf16 convolution reads it
        if getattr(u, "bf16", None) is None or out is not None:
            raise ValueError("conv3x3: bf16 activations need the bf16 operands of the layer (u.bf16)")
        return conv3x3_bf16(x, u.bf16, bias, cout, slope, res, post, pool, stride, out_bf16)
    if CONV_BF16 and out is None and getattr(u, "bf16", None) is not None:
        # out_bf16 is a REQUEST: honoured when the bf16 kernel serves the layer (the result's dtype tells), ignored on the fp32 kernels
        y = conv3x3_bf16(x, u.bf16, bias, cout, slope, res, post, pool, stride, out_bf16 and BF16_CHAINS)
        if y is not None:
            return y
    if (STRIDE2_FRAGS and stride == 2 and out is None and pool == 1 and post is None and getattr(u, "s2", None) is not None):
        y = torch.empty((B, ho, wo, cout), dtype=f32, device=x.device)
        rc = _lib.call("cmr_conv3x3_s2_nhwc_f32", _p(x), B, H, W, cin, _p(u.s2), _p(bias), _p(res), None, _p(y), cout, float(slope), _stream(),
                       allow_unsupported=True)
        if rc != _lib.UNSUPPORTED:
            return y
    if (WINOGRAD and u is not None and stride == 1 and out is None
            and ((W + 15) // 16) * ((H + 7) // 8) * B * (cout // 64) >= WINO_MIN_TILES):
        return conv3x3_wino(x, u, bias, cout, slope, res, post, pool)
    if pool == 2:
        if res is not None or post is not None or out is not None:
            raise ValueError("conv3x3: pool=2 cannot be combined with res / post / out (the fused-pool epilogue has none; "
                             "the Winograd entry point rejects the same combination)")
        y = torch.empty((B, ho // 2, wo // 2, cout), dtype=f32, device=x.device)
        rc = _lib.call("cmr_conv3x3_nhwc_f32", _p(x), B, H, W, cin, _p(w9), _p(bias), None, None, _p(y), cout, stride,
                       float(slope), 2, _stream(), allow_unsupported=True)
        if rc == _lib.UNSUPPORTED:
            return avgpool(conv3x3(x, w9, bias, cout, stride, slope), 2, 2)
        return y
    if out is None:
        out = torch.empty((B, ho, wo, cout), dtype=f32, device=x.device)
    _lib.call("cmr_conv3x3_nhwc_f32", _p(x), B, H, W, cin, _p(w9), _p(bias), _p(res), _p(post), _p(out), cout, stride,
              float(slope), 1, _stream())
    return out


def stem_block(img_nchw, w_a, b_a, w3, w1, b_b, slope, out_bf16=False):
    B, c, H, W = img_nchw.shape
    if c != 3 or not img_nchw.is_contiguous():
        raise ValueError("stem expects a contiguous [B,3,H,W] image")
    tmp = torch.empty((B, 6, H, W), dtype=f32, device=img_nchw.device)      # conv-a output | a copy of the image (stem_b's single operand base)
    out = torch.empty((B, H, W, 64), dtype=torch.bfloat16 if out_bf16 else f32, device=img_nchw.device)
    _lib.call("cmr_stem_block_f32", _p(img_nchw), _p(w_a), _p(b_a), _p(w3), _p(w1), _p(b_b), _p(tmp), _p(out), int(out_bf16), B, H, W,
              float(slope), _stream())
    return out


def avgpool(x, kh, kw):
    B, H, W, C = x.shape
    out = torch.empty((B, H // kh, W // kw, C), dtype=f32, device=x.device)
    _lib.call("cmr_avgpool_nhwc_f32", _p(x), _p(out), B, H, W, C, kh, kw, _stream())
    return out


def upsample_concat(f, proxy_rows, scale):
    B, H, W, c1 = f.shape
    c2 = proxy_rows.shape[1]
    out = torch.empty((B, H, W, c1 + c2), dtype=f32, device=f.device)
    _lib.call("cmr_upsample_concat_f32", _p(f), _p(proxy_rows), _p(out), B, H, W, c1, c2, scale, _stream())
    return out


def patchify(x, P):
    B, H, W, C = x.shape
    out = torch.empty((B * (H // P) * (W // P), P * P * C), dtype=f32, device=x.device)
    _lib.call("cmr_patchify_nhwc_f32", _p(x), _p(out), B, H, W, C, P, _stream())
    return out


def patch_embed(x, P, w, bias, res=None, res_mod=0):
    """Conv2d(kernel = stride = P) on an NHWC map as one GEMM over the patches read in place: [B,H,W,C] -> [B*(H/P)*(W/P), n_out];
    w [n_out, P*P*C] in (ky, kx, c) order.  Falls back to patchify + linear where the kernel does not serve the shape."""
    B, H, W, C = x.shape
    n_out, K = w.shape
    rows = B * (H // P) * (W // P)
    if K % 64 == 0 and K >= 512 and (P * C) % 8 == 0 and rows <= 65536 and n_out % 4 == 0 and x.is_contiguous() and x.dtype == f32:
        out = torch.empty((rows, n_out), dtype=f32, device=x.device)
        _lib.call("cmr_patch_embed_f32", _p(x), B, H, W, C, P, _p(w), w.stride(0), _p(bias), _p(res), _ld(res) if res is not None else 0,
                  int(res_mod), _p(out), n_out, n_out, _stream())
        return out
    return linear(patchify(x, P), w, bias, res=res, res_mod=res_mod)


def transpose(x):
    """[batch, R, C] contiguous -> [batch, C, R] contiguous."""
    b, r, c = x.shape
    if not x.is_contiguous():
        raise ValueError("transpose expects a contiguous tensor")
    out = torch.empty((b, c, r), dtype=f32, device=x.device)
    _lib.call("cmr_transpose_f32", _p(x), _p(out), b, r, c, _stream())
    return out


def mha(q, k, v, B, Tq, Tk, out=None, libm_exp=False):
    """softmax(Q K^T / sqrt(8)) V per head; libm_exp: exponentials through expf (the training tape's forward, see cmr_mha_expf_f32)."""
    if out is None:
        out = torch.empty((B * Tq, 64), dtype=f32, device=q.device)
    _lib.call("cmr_mha_expf_f32" if libm_exp else "cmr_mha_f32", _p(_rows(q)), _ld(q), _p(_rows(k)), _ld(k), _p(_rows(v)), _ld(v), _p(out), _ld(out), B, Tq,
              Tk, _stream())
    return out


def mha_ln(x, y, ln, eps, frags, B, Tq, Tk, out=None):
    """LayerNorm + Q / K / V projections + softmax attention in one launch (cmr_mha_ln_f32); frags = _pack.mha_ln_frags(...)."""
    wq_f, wkv_f, bq, bk, bv = frags
    if out is None:
        out = torch.empty((B * Tq, 64), dtype=f32, device=x.device)
    y = x if y is None else y
    _lib.call("cmr_mha_ln_f32", _p(_rows(x)), _ld(x), _p(_rows(y)), _ld(y), _p(ln[0]), _p(ln[1]), float(eps), _p(wq_f), _p(wkv_f), _p(bq), _p(bk),
              _p(bv), _p(out), _ld(out), B, Tq, Tk, _stream())
    return out


def la_reduce(kf, v, B, S):
    ws_bytes = _lib.load().cmr_la_reduce_workspace_bytes(B, S)
    ws = torch.empty((ws_bytes // 4,), dtype=f32, device=kf.device)
    kvsum = torch.empty((B, 576), dtype=f32, device=kf.device)
    _lib.call("cmr_la_reduce_f32", _p(_rows(kf)), _ld(kf), _p(_rows(v)), _ld(v), _p(kvsum), _p(ws), ws_bytes, B, S,
              _stream())
    return kvsum


def la_apply(qf, kvsum, B, L, S, eps, out=None):
    if out is None:
        out = torch.empty((B * L, 64), dtype=f32, device=qf.device)
    _lib.call("cmr_la_apply_f32", _p(_rows(qf)), _ld(qf), _p(kvsum), _p(out), _ld(out), B, L, S, float(eps), _stream())
    return out


def agent_heads(x, B, npix, c24, c26, e3d, heads, slope, actions=None):
    """x [B*npix,128] (last 2-D feature map) -> global mean -> two 1x1 convs -> cat with e3d [B,128] -> the three
    MLP heads.  c24 / c26 / heads[i][j] are (W [out,in], bias) pairs; returns the three logit tensors [B, n2_i].
    actions = (num_steps, degree_r, degree_t): the same launch also emits the deterministic actions (argmax per group of
    num_steps logits) -> returns (outs, (action_r [B,degree_r], action_t [B,degree_t]))."""
    outs, args = [], []
    for (w0, b0), (w1, b1), (w2, b2) in heads:
        o = torch.empty((B, w2.shape[0]), dtype=f32, device=x.device)
        outs.append(o)
        args += [_p(w0), _p(b0), _p(w1), _p(b1), _p(w2), _p(b2), w0.shape[0], w1.shape[0], w2.shape[0], _p(o), o.stride(0)]
    if actions is None:
        _lib.call("cmr_agent_heads_f32", _p(_rows(x)), B, npix, _p(c24[0]), _p(c24[1]), _p(c26[0]), _p(c26[1]), _p(e3d), *args,
                  0, 0, 0, None, None, float(slope), _stream())
        return outs
    S, dr, dt = actions
    ar = torch.empty((B, dr), dtype=torch.int64, device=x.device)
    at = torch.empty((B, dt), dtype=torch.int64, device=x.device)
    _lib.call("cmr_agent_heads_f32", _p(_rows(x)), B, npix, _p(c24[0]), _p(c24[1]), _p(c26[0]), _p(c26[1]), _p(e3d), *args,
              int(S), int(dr), int(dt), _p(ar), _p(at), float(slope), _stream())
    return outs, (ar, at)


def agent_heads_train(x, B, npix, c24, c26, e3d, heads, slope):
    """Training forward of the agent's tail in one launch (cmr_agent_heads_train_f32): x [B*npix,128] (activated output of the last 3x3
    conv), c24 / c26 / heads[i][j] = (W [out4,in4], bias [out4]) as stored in the flat bucket, e3d [B,128] ->
    (outs [3 x [B,n2]], pooled, t1, e2d, [(h0, h1) per head]); the intermediates are views of ONE buffer.  None when the widths are not
    the ones the kernel is built for (128 channels, hidden widths multiples of 4 up to 256)."""
    if x.shape[1] != 128 or e3d.shape != (B, 128) or not e3d.is_contiguous() or c24[0].shape != (128, 128) or c26[0].shape != (128, 128):
        return None
    outs, args, widths = [], [], []
    for (w0, b0), (w1, b1), (w2, b2) in heads:
        n0, n1 = w0.shape[0], w1.shape[0]
        if w0.shape[1] != 256 or w1.shape[1] != n0 or w2.shape[1] != n1 or n0 % 4 or n1 % 4 or n0 > 256 or n1 > 256:
            return None
        o = torch.empty((B, w2.shape[0]), dtype=f32, device=x.device)
        outs.append(o)
        widths.append((n0, n1))
        args += [_p(w0), _p(b0), _p(w1), _p(b1), _p(w2), _p(b2), n0, n1, w2.shape[0], _p(o), o.stride(0)]
    total = B * (3 * 128 + sum(a + b for a, b in widths))
    saves = torch.empty((total,), dtype=f32, device=x.device)
    _lib.call("cmr_agent_heads_train_f32", _p(_rows(x)), B, npix, _p(c24[0]), _p(c24[1]), _p(c26[0]), _p(c26[1]), _p(e3d), *args,
              _p(saves), total, float(slope), _stream())
    pooled, t1, e2d = (saves[i * B * 128:(i + 1) * B * 128].view(B, 128) for i in range(3))
    off, hid = 3 * B * 128, []
    for n0, n1 in widths:
        hid.append((saves[off:off + B * n0].view(B, n0), saves[off + B * n0:off + B * (n0 + n1)].view(B, n1)))
        off += B * (n0 + n1)
    return outs, pooled, t1, e2d, hid


def agent_heads_t(x, B, npix, c24t, c26t, e3d, heads_t, slope, actions=None):
    """agent_heads with every weight TRANSPOSED at plan time: c24t / c26t / heads_t[i][j] are (W^T [in, out4], bias [out4]) pairs
    (models/CMRAgent.py:_build_plan); one memory round trip per layer instead of per batch of weight rows + cross-lane reductions."""
    outs, args = [], []
    for (w0, b0), (w1, b1), (w2, b2) in heads_t:
        o = torch.empty((B, w2.shape[1]), dtype=f32, device=x.device)
        outs.append(o)
        args += [_p(w0), _p(b0), _p(w1), _p(b1), _p(w2), _p(b2), w0.shape[1], w1.shape[1], w2.shape[1], _p(o), o.stride(0)]
    if actions is None:
        _lib.call("cmr_agent_heads_t_f32", _p(_rows(x)), B, npix, _p(c24t[0]), _p(c24t[1]), _p(c26t[0]), _p(c26t[1]), _p(e3d), *args,
                  0, 0, 0, None, None, float(slope), _stream())
        return outs
    S, dr, dt = actions
    ar = torch.empty((B, dr), dtype=torch.int64, device=x.device)
    at = torch.empty((B, dt), dtype=torch.int64, device=x.device)
    _lib.call("cmr_agent_heads_t_f32", _p(_rows(x)), B, npix, _p(c24t[0]), _p(c24t[1]), _p(c26t[0]), _p(c26t[1]), _p(e3d), *args,
              int(S), int(dr), int(dt), _p(ar), _p(at), float(slope), _stream())
    return outs, (ar, at)


def ln64_linear(x, wf_x, bias_x, gamma, beta, eps, y=None, wf_y=None, bias_y=None):
    """LayerNorm(64) + projection of x rows (and, with the same norm, of y rows) in one launch; weights are
    fragment-packed (_pack.frag_pack).  Returns out_x [rows_x, n_x] (and out_y [rows_y, n_y])."""
    nx = bias_x.numel()
    ox = torch.empty((x.shape[0], nx), dtype=f32, device=x.device)
    name = "cmr_ln64_linear_bf16_f32" if wf_x.dtype == torch.bfloat16 else "cmr_ln64_linear_f32"       # by the fragments' dtype
    if y is None:
        _lib.call(name, _p(_rows(x)), _ld(x), x.shape[0], _p(wf_x), _p(bias_x), nx, _p(ox), _ld(ox), None, 0, 0,
                  None, None, 0, None, 0, _p(gamma), _p(beta), float(eps), _stream())
        return ox
    ny = bias_y.numel()
    oy = torch.empty((y.shape[0], ny), dtype=f32, device=y.device)
    _lib.call(name, _p(_rows(x)), _ld(x), x.shape[0], _p(wf_x), _p(bias_x), nx, _p(ox), _ld(ox), _p(_rows(y)),
              _ld(y), y.shape[0], _p(wf_y), _p(bias_y), ny, _p(oy), _ld(oy), _p(gamma), _p(beta), float(eps), _stream())
    return ox, oy


def vit_out_ffn(ctx, x, wo_f, bo, ln, eps, w1_f, b1, w2_f, b2, rows16=False):
    """attention out-projection + residual, then the pre-LN MLP (64 -> 1024 -> 64, erf GELU) + residual.  rows16: the fp32 kernel on
    16-row tiles; the weights are then _pack.frag_pack16 fragments."""
    if b1.numel() != 1024 or bo.numel() != 64:
        raise ValueError("vit_out_ffn is instantiated for embed_dim 64 / mlp_dim 1024")
    out = torch.empty((x.shape[0], 64), dtype=f32, device=x.device)
    _lib.call("cmr_vit_out_ffn_bf16_f32" if w1_f.dtype == torch.bfloat16 else ("cmr_vit_out_ffn16_f32" if rows16 else "cmr_vit_out_ffn_f32"), _p(_rows(ctx)), _ld(ctx), _p(_rows(x)), _ld(x), _p(wo_f), _p(bo), _p(ln[0]), _p(ln[1]),
              float(eps), _p(w1_f), _p(b1), _p(w2_f), _p(b2), _p(out), _ld(out), x.shape[0], _stream())
    return out


LA_STATE_BF16 = True      # with CONV_BF16: the K / V projections of the state kernel on the bf16 cores as well (False: round 2's fp32 state kernel)


def la_kv_state(y, wk, wv, B, S):
    """Fused k/v projections + per-(batch, head) state of one linear-attention layer: y [B*S,64] -> [B,576]."""
    ws_bytes = _lib.load().cmr_la_kv_state_workspace_bytes(B, S)
    ws = torch.empty((ws_bytes // 4,), dtype=f32, device=y.device)
    kvsum = torch.empty((B, 576), dtype=f32, device=y.device)
    _lib.call("cmr_la_kv_state_bf16_f32" if (CONV_BF16 and LA_STATE_BF16) else "cmr_la_kv_state_f32", _p(_rows(y)), _ld(y), _p(wk), _p(wv), _p(kvsum), _p(ws), ws_bytes, B, S,
              _stream())
    return kvsum


def la_query_layer(x, kvsum, wq, wmerge, ln1, w0, w3, ln2, B, L, S, eps, ln_eps, out=None):
    """Fused query side of a linear-attention layer (q projection .. residual).  Returns None when the library
    does not serve the shape (too many batch states for LDS) so that the caller can take the unfused path."""
    if out is None:
        out = torch.empty((B * L, 64), dtype=f32, device=x.device)
    rc = _lib.call("cmr_la_query_layer_bf16_f32" if CONV_BF16 else "cmr_la_query_layer_f32", _p(_rows(x)), _ld(x), _p(kvsum), _p(wq), _p(wmerge), _p(ln1[0]), _p(ln1[1]),
                   _p(w0), _p(w3), _p(ln2[0]), _p(ln2[1]), _p(out), _ld(out), B, L, S, float(eps), float(ln_eps),
                   _stream(), allow_unsupported=True)
    return None if rc == _lib.UNSUPPORTED else out


def planar_to_rows(x, cpad=4):
    """contiguous [B,C,N] -> [B*N,cpad] (zero padded), cpad in {4, 8}."""
    B, C, N = x.shape
    if not x.is_contiguous() or x.dtype != f32:
        raise ValueError("planar_to_rows expects a contiguous float32 [B,C,N] tensor")
    out = torch.empty((B * N, cpad), dtype=f32, device=x.device)
    _lib.call("cmr_planar_to_rows_f32", _p(x), _p(out), B, C, N, cpad, _stream())
    return out


def planar_to_rows4(x):
    return planar_to_rows(x, 4)


def concat_rows(x1, x2, idx2=None, div2=1):
    _rows(x1), _rows(x2)
    rows = x1.shape[0]
    out = torch.empty((rows, x1.shape[1] + x2.shape[1]), dtype=f32, device=x1.device)
    _lib.call("cmr_concat_rows_f32", _p(x1), _ld(x1), x1.shape[1], _p(x2), _ld(x2), x2.shape[1], _p(_i32(idx2)),
              int(div2), _p(out), rows, _stream())
    return out


def index_to_global(idx, M):
    """int64 [B,N] per-batch ids in [0,M) -> int32 [B*N] global row ids."""
    B, N = idx.shape
    if idx.dtype != torch.int64 or not idx.is_contiguous():
        raise ValueError("index tensor must be contiguous int64")
    out = torch.empty((B * N,), dtype=torch.int32, device=idx.device)
    _lib.call("cmr_index_to_global_i32", _p(idx), _p(out), B, N, M, _stream())
    return out


def csr_build(key, B, n_per_batch, seg_per_batch):
    total = B * seg_per_batch
    count = torch.empty((total,), dtype=torch.int32, device=key.device)
    offsets = torch.empty((total + 1,), dtype=torch.int32, device=key.device)
    order = torch.empty((B * n_per_batch,), dtype=torch.int32, device=key.device)
    _lib.call("cmr_csr_build_i32", _p(_i32(key)), _p(count), _p(offsets), _p(order), B, n_per_batch, seg_per_batch,
              _stream())
    return offsets, order


def knn16(xyz4, B, M):
    out = torch.empty((B * M, 16), dtype=torch.int32, device=xyz4.device)
    _lib.call("cmr_knn16_f32", _p(xyz4), _p(out), B, M, _stream())
    return out


def knn(q4, c4, B, S, N, K):
    """-> int64 [B, S, K]: the K nearest candidates of every query, ascending distance, ties in ascending index."""
    if not 1 <= K <= 64:
        raise ValueError("knn: K = %d (the kernel keeps up to 64 neighbours)" % K)
    out = torch.empty((B, S, K), dtype=torch.int64, device=q4.device)
    _lib.call("cmr_knn_f32", _p(q4), _p(c4), _p(out), B, S, N, K, _stream())
    return out


def nearest(q4, c4, B, Nq, Nc, want_local=True, want_global=True):
    og = torch.empty((B * Nq,), dtype=torch.int32, device=q4.device) if want_global else None
    ol = torch.empty((B, Nq), dtype=torch.int64, device=q4.device) if want_local else None
    _lib.call("cmr_nearest_f32", _p(q4), _p(c4), _p(og), _p(ol), B, Nq, Nc, _stream())
    return og, ol


def rel_pos(a, b, rows, ia=None, diva=1, ib=None, divb=1):
    out = torch.empty((rows, 4), dtype=f32, device=a.device)
    _lib.call("cmr_rel_pos_f32", _p(a), _p(_i32(ia)), int(diva), _p(b), _p(_i32(ib)), int(divb), _p(out), rows, _stream())
    return out


def vecattn_prep(q, k, v, pos, rows, iq=None, divq=1, ik=None):
    t = torch.empty((rows, 64), dtype=f32, device=q.device)
    vp = torch.empty((rows, 64), dtype=f32, device=q.device)
    _lib.call("cmr_vecattn_prep_f32", _p(_rows(q)), _ld(q), _p(_i32(iq)), int(divq), _p(_rows(k)), _ld(k), _p(_rows(v)),
              _ld(v), _p(_i32(ik)), _p(pos), _p(t), _p(vp), rows, _stream())
    return t, vp


def vecattn_front(q, pa4, pb4, ib, d0, d2, g0, g2, rows, iq=None, divq=1, ia=None, diva=1, feat=None, fc1=None, wkv=None,
                  kv=None, ik=None):
    """Per-row front of the vector attention (see cmr_vecattn_front_f32): returns (a, vp), both [rows, 64].
    Either feat + fc1 (W, b) + wkv ([128, 64]) or a precomputed kv table [*, >=128] (+ ik) supplies k / v."""
    a = torch.empty((rows, 64), dtype=f32, device=q.device)
    vp = torch.empty((rows, 64), dtype=f32, device=q.device)
    if feat is not None:
        src = (_p(_rows(feat)), _ld(feat), _p(fc1[0]), _p(fc1[1]), _p(wkv), None, 0, None)
    else:
        src = (None, 0, None, None, None, _p(_rows(kv)), _ld(kv), _p(_i32(ik)))
    _lib.call("cmr_vecattn_front_f32", *src, _p(_rows(q)), _ld(q), _p(_i32(iq)), int(divq), _p(pa4), _p(_i32(ia)), int(diva),
              _p(pb4), _p(_i32(ib)), _p(d0[0]), _p(d0[1]), _p(d2[0]), _p(d2[1]), _p(g0[0]), _p(g0[1]), _p(g2[0]), _p(g2[1]),
              _p(a), _p(vp), rows, _stream())
    return a, vp


def _front_outs(outs, n, rows, device):
    if outs is None:
        return [torch.empty((rows, 64), dtype=f32, device=device) for _ in range(n)]
    if len(outs) != n or any(o.dtype != f32 or tuple(o.shape) != (rows, 64) or not o.is_contiguous() or o.device != device for o in outs):
        raise ValueError("vecattn_front_*_train: outs must be %d contiguous float32 [%d, 64] tensors on %s" % (n, rows, device))
    return list(outs)


def vecattn_front_train(k, v, q, pa4, pb4, ib, d0, d2, g0, g2, iq=None, divq=1, ia=None, diva=1, ikv=None, outs=None):
    """Training forward of the vector-attention front in one launch -> (a, vp, hd, t, g1), all [rows, 64] (see cmr_vecattn_front_train_f32),
    or False when rows is not a multiple of 32.  ikv: k and v are per-node tables, row ikv[r] of both is the pair's.  outs: five contiguous
    [rows, 64] buffers to write instead of fresh ones."""
    _rows(k), _rows(v), _rows(q)
    rows = ib.numel()                                       # one row per (point, node) / (node, neighbour) pair
    if rows % 32 or k.shape[1] != 64 or v.shape[1] != 64 or q.shape[1] != 64 or (ikv is None and (k.shape[0] != rows or v.shape[0] != rows)):
        return False
    outs = _front_outs(outs, 5, rows, k.device)
    _lib.call("cmr_vecattn_front_train_f32", _p(k), _ld(k), _p(v), _ld(v), _p(_i32(ikv)), _p(q), _ld(q), _p(_i32(iq)), int(divq), _p(pa4), _p(_i32(ia)),
              int(diva), _p(pb4), _p(_i32(ib)), _p(d0[0]), _p(d0[1]), _p(d2[0]), _p(d2[1]), _p(g0[0]), _p(g0[1]), _p(g2[0]), _p(g2[1]),
              *[_p(o) for o in outs], rows, _stream())
    return tuple(outs)


def vecattn_front_kv_train(feat, fc1, wk, wv, q, pa4, pb4, ib, d0, d2, g0, g2, iq=None, divq=1, ia=None, diva=1, outs=None):
    """... with x = fc1(feat), k = Wk x, v = Wv x computed inside -> (a, vp, hd, t, g1, x), or False when rows is not a multiple of 32.
    outs: six contiguous [rows, 64] buffers to write instead of fresh ones."""
    _rows(feat), _rows(q)
    rows = feat.shape[0]
    if rows % 32 or feat.shape[1] != 64 or q.shape[1] != 64 or tuple(wk.shape) != (64, 64) or tuple(wv.shape) != (64, 64) or not (wk.is_contiguous() and wv.is_contiguous()):
        return False
    outs = _front_outs(outs, 6, rows, feat.device)
    _lib.call("cmr_vecattn_front_kv_train_f32", _p(feat), _ld(feat), _p(fc1[0]), _p(fc1[1]), _p(wk), _p(wv), _p(q), _ld(q), _p(_i32(iq)), int(divq),
              _p(pa4), _p(_i32(ia)), int(diva), _p(pb4), _p(_i32(ib)), _p(d0[0]), _p(d0[1]), _p(d2[0]), _p(d2[1]), _p(g0[0]), _p(g0[1]),
              _p(g2[0]), _p(g2[1]), *[_p(o) for o in outs], rows, _stream())
    return tuple(outs)


def segment_softmax(attn, vp, nseg, scale, order=None, offsets=None, fixed_len=0):
    out = torch.empty((nseg, 64), dtype=f32, device=attn.device)
    _lib.call("cmr_segment_softmax_f32", _p(attn), _p(vp), _p(_i32(order)), _p(_i32(offsets)), fixed_len, float(scale),
              _p(out), nseg, _stream(), work_extra={"_rows": attn.shape[0]})
    return out


def segment_reduce(src, order, offsets, nseg, mode):
    """mode 'sum' | 'max' | 'mean' over the CSR segments (offsets, order) of the rows of src [R, C] -> [nseg, C]."""
    _rows(src)
    C = src.shape[1]
    out = torch.empty((nseg, C), dtype=f32, device=src.device)
    _lib.call("cmr_segment_reduce_f32", _p(src), _ld(src), _p(_i32(order)), _p(_i32(offsets)), _p(out), C, nseg, C,
              {"sum": 0, "max": 1, "mean": 2}[mode], _stream(), work_extra={"_rows": src.shape[0]})
    return out


def gather_rows(src, idx, C=None, out=None):
    _rows(src)
    C = src.shape[1] if C is None else C
    rows = idx.numel()
    if out is None:
        out = torch.empty((rows, C), dtype=f32, device=src.device)
    _lib.call("cmr_gather_rows_f32", _p(src), _ld(src), _p(_i32(idx)), _p(out), _ld(out), rows, C, _stream())
    return out


def three_nn(q4, c4, B, Nq, Nc):
    idx = torch.empty((B * Nq, 3), dtype=torch.int32, device=q4.device)
    wgt = torch.empty((B * Nq, 3), dtype=f32, device=q4.device)
    _lib.call("cmr_three_nn_f32", _p(q4), _p(c4), _p(idx), _p(wgt), B, Nq, Nc, _stream())
    return idx, wgt


def weighted_gather3(src, idx, wgt):
    _rows(src)
    rows, C = idx.shape[0], src.shape[1]
    out = torch.empty((rows, C), dtype=f32, device=src.device)
    _lib.call("cmr_weighted_gather3_f32", _p(src), _ld(src), _p(idx), _p(wgt), _p(out), C, rows, C, _stream())
    return out


def weighted_scatter3(dy, wgt, order, offsets, nseg):
    """backward of weighted_gather3 w.r.t. its source rows -> [nseg, C]"""
    _rows(dy)
    C = dy.shape[1]
    out = torch.empty((nseg, C), dtype=f32, device=dy.device)
    _lib.call("cmr_weighted_scatter3_f32", _p(dy), _ld(dy), _p(wgt), _p(_i32(order)), _p(_i32(offsets)), _p(out), C, nseg, C, _stream())
    return out


FPS_COOP_MIN_N = 16385      # clouds above this take the multi-workgroup kernel (one workgroup keeps <= 16 384 points in registers)


def fps(xyz4, start, B, N, npoint, coop=None, spin_limit=None, status=None):
    """Farthest point sampling -> int64 [B, npoint] local indices.  coop: None = by size, True / False = force the multi- /
    single-workgroup kernel (identical results).  The multi-workgroup kernel needs the workgroups of a cloud co-resident; a cloud
    that could not get them within the spin bound is recomputed by one workgroup inside the same call (never -1 in the result).
    spin_limit: polls per round before giving a cloud up (None = the library's bound, 0 = give up at once: tests).  status: a list
    that receives the int32 [B] device view of the per-cloud status words (0 cooperative, 2 repaired)."""
    out = torch.empty((B, npoint), dtype=torch.int64, device=xyz4.device)
    use = (N >= FPS_COOP_MIN_N and B <= 64) if coop is None else coop
    if use:
        nb = _lib.load().cmr_fps_workspace_bytes(B, N, npoint)
        ws = torch.empty((nb // 8 + 1,), dtype=torch.int64, device=xyz4.device)
        if spin_limit is None:
            _lib.call("cmr_fps_ws_f32", _p(xyz4), _p(start), _p(out), B, N, npoint, _p(ws), nb, _stream())
        else:
            _lib.call("cmr_fps_ws_spin_f32", _p(xyz4), _p(start), _p(out), B, N, npoint, _p(ws), nb, int(spin_limit), _stream())
        if status is not None:
            words = 2 * B * npoint * 16                     # int32 words of the [B][npoint][16] 64-bit round slots (csrc/points.hip: FPS_GMAX)
            status.append(ws.view(torch.int32)[words + B:words + 2 * B])
    else:
        _lib.call("cmr_fps_f32", _p(xyz4), _p(start), _p(out), B, N, npoint, _stream())
    return out


def ball_query(xyz4, new4, B, N, S, nsample, radius):
    out = torch.empty((B, S, nsample), dtype=torch.int64, device=xyz4.device)
    r2 = torch.tensor(float(radius) ** 2, dtype=f32).item()      # the scalar the reference compares against
    _lib.call("cmr_ball_query_f32", _p(xyz4), _p(new4), _p(out), B, N, S, nsample, r2, _stream())
    return out


def square_distance(a4, b4, B, N, M):
    out = torch.empty((B, N, M), dtype=f32, device=a4.device)
    _lib.call("cmr_square_distance_f32", _p(a4), _p(b4), _p(out), B, N, M, _stream())
    return out


def _colreduce(name, x, B, N):
    _rows(x)
    C = x.shape[1]
    ws_bytes = _lib.load().cmr_colreduce_workspace_bytes(B, N, C)
    ws = torch.empty((max(ws_bytes // 4, 1),), dtype=f32, device=x.device)
    out = torch.empty((B, C), dtype=f32, device=x.device)
    _lib.call(name, _p(x), _ld(x), _p(out), _p(ws), ws_bytes, B, N, C, _stream())
    return out


def colmax(x, B, N):
    return _colreduce("cmr_colmax_f32", x, B, N)


def colmean(x, B, N):
    return _colreduce("cmr_colmean_f32", x, B, N)


def project_scatter(pc4, feat, overlap_u8, pose, K, mean4, B, N, h, w, acc, cnt, state3d, zero_first=True):
    """acc / cnt must be zero on entry; zero_first=False when the previous observation_finalize(clear=True) left them so."""
    _lib.call("cmr_project_scatter_f32", _p(pc4), _p(feat), _p(overlap_u8), _p(pose), _p(K), _p(mean4), _p(acc), _p(cnt),
              _p(state3d), B, N, h, w, int(zero_first), _stream())


def observation_finalize(img_feat, acc, cnt, state2d, proj, B, h, w, write_img, clear=False):
    _lib.call("cmr_observation_finalize_f32", _p(img_feat), _p(acc), _p(cnt), _p(state2d), _p(proj), B, h, w,
              int(write_img), int(clear), _stream())


def reach_tiles(B, h, w):
    """(tiles of the full-resolution stage, tiles of the half-resolution stage) of the observation's reach maps"""
    return B * ((h + 7) // 8) * ((w + 15) // 16), B * ((h // 2 + 7) // 8) * ((w // 2 + 15) // 16)


def observation_proj(pc4, feat, overlap_u8, pose, K, mean4, B, N, h, w, proj, cnt, cell, state3d, reach=None):
    """The projected half of the observation maintained in place (see cmr_observation_proj_f32): proj / cnt / cell are the caller's state.
    reach (uint8 [2, B, ceil(h/8), ceil(w/16)], zero before the first call): the tiles within 1 / 2 pixels of a cell hit now are marked in
    reach[0] / reach[1], for wino_tile_lists.  With 2 B ceil(h/16) ceil(w/32) more bytes behind them (flat; h, w multiples of 4): the two
    maps of the half-resolution stage too (footprints dilated by 4 / 6 cells), for wino_tile_lists_staged."""
    if cell.dtype != torch.int32 or cell.numel() != B * N or proj.numel() != B * h * w * 64 or cnt.numel() != B * h * w:
        raise ValueError("observation_proj: state buffers of the wrong shape / dtype")
    if reach is not None:
        nt, nt1 = reach_tiles(B, h, w)
        staged = reach.numel() == 2 * nt + 2 * nt1 and h % 4 == 0 and w % 4 == 0
        if reach.dtype != torch.uint8 or not (reach.numel() == 2 * nt or staged) or not reach.is_contiguous():
            raise ValueError("observation_proj: reach must be uint8 [2, %d] (+ [2, %d])" % (nt, nt1))
        if staged:
            a = reach.data_ptr()
            _lib.call("cmr_observation_proj_reach_staged_f32", _p(pc4), _p(feat), _p(overlap_u8), _p(pose), _p(K), _p(mean4), _p(proj), _p(cnt),
                      _p(cell), _p(state3d), B, N, h, w, a, a + nt, a + 2 * nt, a + 2 * nt + nt1, _stream())
            return
        _lib.call("cmr_observation_proj_reach_f32", _p(pc4), _p(feat), _p(overlap_u8), _p(pose), _p(K), _p(mean4), _p(proj), _p(cnt), _p(cell),
                  _p(state3d), B, N, h, w, _p(reach), reach.data_ptr() + nt, _stream())
        return
    _lib.call("cmr_observation_proj_f32", _p(pc4), _p(feat), _p(overlap_u8), _p(pose), _p(K), _p(mean4), _p(proj), _p(cnt), _p(cell), _p(state3d),
              B, N, h, w, _stream())


def pose_step(pose, act_r, act_t, r_steps, t_steps, six_dof):
    _lib.call("cmr_pose_step_f32", _p(pose), _p(act_r), _p(act_t), _p(r_steps), _p(t_steps), pose.shape[0], int(six_dof),
              _stream())


def to_disentangled(pose, mean4):
    _lib.call("cmr_to_disentangled_f32", _p(pose), _p(mean4), pose.shape[0], _stream())


def focal_metrics(logits_rows, label_i64, alpha, B):
    """2-class logits rows [R, >=2] + int64 labels [R] -> float32 [4] = (focal loss, precision, recall, accuracy)."""
    R = logits_rows.shape[0]
    ws_bytes = _lib.load().cmr_focal_metrics_workspace_bytes(R)
    ws = torch.empty((max(ws_bytes // 4, 1),), dtype=f32, device=logits_rows.device)
    out = torch.empty((4,), dtype=f32, device=logits_rows.device)
    _lib.call("cmr_focal_metrics_f32", _p(logits_rows), logits_rows.stride(0), _p(label_i64), float(alpha), R, B, _p(out), _p(ws),
              ws_bytes, _stream())
    return out


def circle_loss(pc_feat_rows, img_feat_nhwc, pc_idx, xy_int, xy_float, B, N, dist_thres, pos_margin, neg_margin, log_scale, lam, terms=None):
    """Circle loss over the sampled (point, pixel) pairs: pc_feat rows [B*N,64], img_feat [B,h,w,64], pc_idx int64 [B,n],
    xy_int int64 [B,2,n], xy_float [B,2,n] -> float32 [1].  terms: a list that receives the float32 [B, 2n] device view of the
    softplus terms the loss is the mean of (per sample: the n rows, then the n columns; csrc/losses.hip circle_terms_kernel)."""
    _, h, w, _ = img_feat_nhwc.shape
    n = pc_idx.shape[1]
    ws_bytes = _lib.load().cmr_circle_loss_workspace_bytes(B, n)
    ws = torch.empty((ws_bytes // 4,), dtype=f32, device=pc_feat_rows.device)
    out = torch.empty((1,), dtype=f32, device=pc_feat_rows.device)
    _lib.call("cmr_circle_loss_f32", _p(_rows(pc_feat_rows)), _p(img_feat_nhwc), _p(pc_idx), _p(xy_int), _p(xy_float), B, N, h, w, n,
              float(dist_thres), float(pos_margin), float(neg_margin), float(log_scale), float(lam), _p(out), _p(ws), ws_bytes,
              _stream())
    if terms is not None:
        first = 2 * B * n * n + B                           # float words of EP, EN [B][n][n] and the [B] partial sums ahead of the terms
        terms.append(ws[first:first + 2 * B * n].view(B, 2 * n))
    return out


# ---- the argument checks of the matching and pose wrappers below, each stated once.  `who` is the wrapper's name; every failure is a
# ValueError "<who>: ...".  Nothing here looks at a tensor's device or storage but _on_one_gpu, which every wrapper calls last.
def _is_int(v):
    """An integer-valued number that is not a bool; inf, NaN and non-numbers are simply not one (no OverflowError / TypeError)."""
    try:
        return not isinstance(v, bool) and math.isfinite(v) and int(v) == v
    except (TypeError, ValueError, OverflowError):
        return False


def _int_arg(who, name, v, lo, hi):
    if not _is_int(v) or not lo <= v <= hi:
        raise ValueError("%s: %s must be an integer in [%d, %d], got %r" % (who, name, lo, hi, v))
    return int(v)


def _f32_arg(who, name, v, must, lo=0.0, hi=math.inf, lo_open=False, as_f32=True, bools=True):
    """float(v) of a number in [lo, hi] -- (lo, hi] with lo_open, and below +inf whatever hi is -- that is still finite, and with lo_open
    still above lo, as the float32 the kernel takes (as_f32=False: the kernel takes what float32 makes of it).  lo=None: any float, NaN
    included.  bools=False refuses True and False.  Else the ValueError '<who>: <name> must <must>, got <v>'."""
    try:
        x = float(v)
        y = float(torch.tensor(x, dtype=f32)) if as_f32 else x
        ok = (bools or not isinstance(v, bool)) and (
            lo is None or ((lo < x and lo < y if lo_open else lo <= x) and x <= hi and abs(y) < math.inf))
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("%s: %s must %s, got %r" % (who, name, must, v))
    return x


def _got(t):
    """(dtype, shape) of a tensor for a message; the type's name and nothing of anything else"""
    return (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else (type(t).__name__, "")


def _shaped(who, name, t, *shape):
    """t.shape of a tensor of that shape; an entry that is a str ("B", "N", "P") stands for any size"""
    if not torch.is_tensor(t) or t.dim() != len(shape) or any(not isinstance(s, str) and s != d for s, d in zip(shape, t.shape)):
        raise ValueError("%s: %s must be [%s], got %s" % (who, name, ", ".join(map(str, shape)), tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    return t.shape


def _float32(who, names, *ts, what="float32"):
    if not all(torch.is_tensor(t) and t.dtype == f32 for t in ts):
        raise ValueError("%s: %s must be %s, got %s" % (who, names, what, " / ".join(str(_got(t)[0]) for t in ts)))


def _poses_arg(who, poses, B):
    P = _shaped(who, "poses", poses, B, "P", 4, 4)[1]
    if P < 1 or P > POSE_SCORE_MAX_POSES:
        raise ValueError("%s: need 1 <= P <= %d poses per sample, got %d" % (who, POSE_SCORE_MAX_POSES, P))
    return P


def _cloud_range(who, B, N, n_cap, h=None, w=None, noun="map"):
    """1 <= B <= GRID_Y_MAX, 1 <= N <= GRID_Y_MAX * n_cap (the kernel's rows per workgroup) and, given h and w, 1 .. 2^24 pixels"""
    ok = 1 <= B <= GRID_Y_MAX and 1 <= N <= GRID_Y_MAX * n_cap
    if h is None and not ok:
        raise ValueError("%s: need 1 <= B <= %d and 1 <= N <= %d, got B=%d N=%d" % (who, GRID_Y_MAX, GRID_Y_MAX * n_cap, B, N))
    if h is not None and (not ok or h < 1 or w < 1 or h * w > 1 << 24):
        raise ValueError("%s: need 1 <= B <= %d, 1 <= N <= %d and %s of 1 .. 2^24 pixels, got B=%d N=%d %s %d x %d" % (
            who, GRID_Y_MAX, GRID_Y_MAX * n_cap, "an image" if noun == "image" else "a " + noun, B, N, noun, h, w))


def _camera_args(who, pts, pose, K, h, w, noun="image", what="float32 tensors"):
    """The cloud under one pose on an h x w `noun`: pts [B, 3, N], pose [B, 4, 4], K [B, 3, 3], integers h and w -> (B, N, h, w)"""
    B, _, N = _shaped(who, "pts", pts, "B", 3, "N")
    _float32(who, "pts, pose and K", pts, pose, K, what=what)
    _shaped(who, "pose", pose, B, 4, 4)
    _shaped(who, "K", K, B, 3, 3)
    if not _is_int(h) or not _is_int(w):
        raise ValueError("%s: h and w must be integers, got %r x %r" % (who, h, w))
    h, w = int(h), int(w)
    _cloud_range(who, B, N, 256, h, w, noun)
    return B, N, h, w


def _feature_pair(who, pc_feat_rows, img_feat_nhwc, pts=None):
    """Point rows [B*N, 64] and pixel features NHWC [B, h, w, 64] -> (B, h, w, 64); given pts [B, 3, N], they agree with it on B and N"""
    if not torch.is_tensor(pc_feat_rows) or not torch.is_tensor(img_feat_nhwc) or pc_feat_rows.dim() != 2 or img_feat_nhwc.dim() != 4:
        raise ValueError("%s: point rows must be 2-D [B*N, C] and pixel features 4-D [B, h, w, C], got %s / %s" % (
            who, _got(pc_feat_rows)[1], _got(img_feat_nhwc)[1]))
    B, h, w, C = img_feat_nhwc.shape
    if C != 64 or pc_feat_rows.shape[1] != 64:
        raise ValueError("%s: feature width must be 64, got %d / %d" % (who, pc_feat_rows.shape[1], C))
    if pts is not None and (B != pts.shape[0] or pc_feat_rows.shape[0] != B * pts.shape[2]):
        raise ValueError("%s: pts %s, point rows %s and pixel features %s do not agree on B and N" % (
            who, tuple(pts.shape), tuple(pc_feat_rows.shape), tuple(img_feat_nhwc.shape)))
    return B, h, w, C


def _rows_per_sample(who, pc_feat_rows, B, h, w, px_log2):
    """N of B*N point rows, within the ranges of the kernels that sweep every pixel of the map for every row"""
    if B < 1 or B > GRID_Y_MAX or pc_feat_rows.shape[0] % B or h < 1 or w < 1 or h * w > 1 << px_log2:
        raise ValueError("%s: %d point rows do not split into %d samples (1 <= B <= %d) or the map %d x %d is empty / over 2^%d pixels" % (
            who, pc_feat_rows.shape[0], B, GRID_Y_MAX, h, w, px_log2))
    N = pc_feat_rows.shape[0] // B
    if N < 1 or N > GRID_Y_MAX * 256:
        raise ValueError("%s: need 1 <= N <= %d rows per sample, got %d" % (who, GRID_Y_MAX * 256, N))
    return N


def _row_mask(who, name, m, n, or_none=False):
    """A row mask of n elements as the kernels take it: bool viewed as uint8.  or_none: None passes (and the message says so)."""
    if m is None and or_none:
        return None
    if not torch.is_tensor(m) or m.dtype not in (torch.bool, torch.uint8, torch.int64) or m.numel() != n:
        text = "%s: %s must be None or bool / uint8 / int64 with %d elements, got %s %s" if or_none else \
               "%s: %s must be bool / uint8 / int64 with %d elements, got %s %s"
        raise ValueError(text % ((who, name, n) + _got(m)))
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _depth_test_args(who, radius, rel_tol, abs_tol):
    """The window and the two tolerances of the depth test (visibility, depth_test), as the entry takes them"""
    _int_arg(who, "radius", radius, 0, GUIDED_MAX_RADIUS)
    _f32_arg(who, "rel_tol", rel_tol, "be finite and >= 0")
    _f32_arg(who, "abs_tol", abs_tol, "be finite and >= 0")
    return int(radius), float(rel_tol), float(abs_tol)


def _render_maps(B, C, h, w, dev, workspace_bytes):
    """render_points' and render_surfels' index_map, depth_map, attr_map (None at C = 0) and key-map workspace with its size, by that export"""
    index_map = torch.empty((B, h, w), dtype=torch.int32, device=dev)
    depth_map = torch.empty((B, h, w), dtype=f32, device=dev)
    attr_map = torch.empty((B, C, h, w), dtype=f32, device=dev) if C else None
    nb = getattr(_lib.load(), workspace_bytes)(B, h, w)
    return index_map, depth_map, attr_map, _ws(nb, dev), nb


def _gt_xy_arg(who, gt_xy, B, N):
    if gt_xy is not None and (not torch.is_tensor(gt_xy) or gt_xy.dtype != f32 or tuple(gt_xy.shape) != (B, 2, N)):
        raise ValueError("%s: gt_xy must be float32 [%d, 2, %d], got %s %s" % ((who, B, N) + _got(gt_xy)))


def _on_one_gpu(who, *ts, aligned=()):
    """The last check of a wrapper, over the tensors that are not None; `aligned`: the feature rows the kernels load 16 bytes at a time"""
    ts = [t for t in ts if t is not None]
    if not all(t.is_cuda and t.is_contiguous() and t.device == ts[0].device for t in ts):
        raise ValueError("%s: every tensor must be a contiguous tensor on the same GPU" % who)
    if any(t.data_ptr() % 16 for t in aligned):
        raise ValueError("%s: feature rows must be 16-byte aligned" % who)


def feat_match(pc_feat_rows, img_feat_nhwc, mask, gt_xy=None, thr=3.0, img_overlap=None, want_dist=False):
    """Nearest pixel feature of every selected point (include/cmr_hip.h cmr_feat_match_f32): pc_feat rows [B*N, 64], img_feat NHWC
    [B, h, w, 64] (both contiguous float32), mask [B, N] / [B*N] of bool / uint8 / int64 (non-zero = selected); optional gt_xy float32
    [B, 2, N] with threshold thr, optional img_overlap bool / uint8 [B, h, w] / [B*h*w].
    -> (idx int32 [B*N]: pixel p = y * w + x or -1, dist float32 [B*N] or None, counts int32 [B, 4] = (selected, inliers, selected whose
    pixel is in img_overlap, both))."""
    B, h, w, C = _feature_pair("feat_match", pc_feat_rows, img_feat_nhwc)
    _float32("feat_match", "features", pc_feat_rows, img_feat_nhwc)
    if B < 1 or B > GRID_Y_MAX or pc_feat_rows.shape[0] % B:
        raise ValueError("feat_match: %d point rows do not split into %d samples (1 <= B <= %d)" % (pc_feat_rows.shape[0], B, GRID_Y_MAX))
    N = pc_feat_rows.shape[0] // B
    mask = _row_mask("feat_match", "mask", mask, B * N)
    _gt_xy_arg("feat_match", gt_xy, B, N)
    if img_overlap is not None and (img_overlap.dtype not in (torch.bool, torch.uint8) or img_overlap.numel() != B * h * w):    # no int64 here
        raise ValueError("feat_match: img_overlap must be bool / uint8 with %d elements, got %s %s" % (
            B * h * w, img_overlap.dtype, tuple(img_overlap.shape)))
    _on_one_gpu("feat_match", pc_feat_rows, img_feat_nhwc, mask, gt_xy, img_overlap, aligned=(pc_feat_rows, img_feat_nhwc))
    if img_overlap is not None and img_overlap.dtype == torch.bool:
        img_overlap = img_overlap.view(torch.uint8)
    dev = pc_feat_rows.device
    idx = torch.empty((B * N,), dtype=torch.int32, device=dev)
    dist = torch.empty((B * N,), dtype=f32, device=dev) if want_dist else None
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    nb = _lib.load().cmr_feat_match_workspace_bytes(B, N)
    ws = _ws(nb, dev)
    _lib.call("cmr_feat_match_f32", _p(pc_feat_rows), _p(img_feat_nhwc), C, B, N, h, w, _p(mask), mask.element_size(), _p(gt_xy),
              float(thr), _p(img_overlap), _p(idx), _p(dist), _p(counts), _p(ws), nb, _stream())
    return idx, dist, counts


def feat_match_filter(pc_feat_rows, img_feat_nhwc, mask, mutual=True, ratio=0.0, excl_radius=2, max_dist=0.0, gt_xy=None, thr=3.0,
                      want_dist=False, want_rev=False):
    """Nearest pixel feature of every selected point plus the filters that go ahead of PnP-RANSAC (include/cmr_hip.h
    cmr_feat_match_filter_f32); tensors as feat_match.  mutual: keep a row only when its pixel's nearest selected point is
    that row; ratio in [0, 1] (0 = off): keep when d1 <= ratio * d2, d2 = the best distance outside the (2 excl_radius + 1)^2 window of
    the best pixel; max_dist >= 0 (0 = off): keep when d1 <= max_dist.
    -> (idx int32 [B*N] as feat_match, keep bool [B*N], counts int32 [B, 4] = (selected, kept, kept inliers, selected inliers),
    d1 / d2 float32 [B*N] or None (want_dist), rev int32 [B*h*w]: the nearest selected row of every pixel, or None (want_rev))."""
    who = "feat_match_filter"
    B, h, w, C = _feature_pair(who, pc_feat_rows, img_feat_nhwc)
    _float32(who, "features", pc_feat_rows, img_feat_nhwc)
    N = _rows_per_sample(who, pc_feat_rows, B, h, w, 30)
    mask = _row_mask(who, "mask", mask, B * N)
    _gt_xy_arg(who, gt_xy, B, N)
    if not _is_int(excl_radius) or not 0 <= excl_radius < 1 << 31:
        raise ValueError("feat_match_filter: excl_radius must be a non-negative integer, got %r" % (excl_radius,))
    _f32_arg(who, "ratio", ratio, "lie in [0, 1] (0 = no ratio test)", hi=1.0)
    _f32_arg(who, "max_dist", max_dist, "be finite and >= 0 (0 = no bound)", as_f32=False)      # the kernel takes +inf for no bound as well
    _on_one_gpu(who, pc_feat_rows, img_feat_nhwc, mask, gt_xy, aligned=(pc_feat_rows, img_feat_nhwc))
    dev = pc_feat_rows.device
    idx = torch.empty((B * N,), dtype=torch.int32, device=dev)
    keep = torch.empty((B * N,), dtype=torch.uint8, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    d1 = torch.empty((B * N,), dtype=f32, device=dev) if want_dist else None
    d2 = torch.empty((B * N,), dtype=f32, device=dev) if want_dist else None
    rev = torch.empty((B * h * w,), dtype=torch.int32, device=dev) if want_rev else None
    nb = _lib.load().cmr_feat_match_filter_workspace_bytes(B, N, h, w)
    ws = _ws(nb, dev)
    _lib.call("cmr_feat_match_filter_f32", _p(pc_feat_rows), _p(img_feat_nhwc), C, B, N, h, w, _p(mask), mask.element_size(),
              1 if mutual else 0, float(ratio), int(excl_radius), float(max_dist), _p(gt_xy), float(thr), _p(idx), _p(keep), _p(counts),
              _p(d1), _p(d2), _p(rev), _p(ws), nb, _stream())
    return idx, keep.view(torch.bool), counts, d1, d2, rev


def match_conf(pc_feat_rows, img_feat_nhwc, mask, temperature=0.1, min_conf=0.0, gt_xy=None, thr=3.0, want_dist=False, want_lse=False):
    """Nearest pixel feature of every selected point with its dual-softmax confidence (include/cmr_hip.h cmr_match_conf_f32, DESIGN.md
    4p); tensors as feat_match.  With s(n, p) = -|point n - pixel p|^2 / temperature over the selected points x the sample's pixels,
    conf = softmax over the row times softmax over the column at the match, in (0, 1]; min_conf in [0, 1] (0 = off): keep a row when
    conf >= min_conf.
    -> (idx int32 [B*N] as feat_match, conf float32 [B*N] (NaN on unselected rows), keep bool [B*N], counts int32 [B, 4] = (selected,
    kept, kept inliers, selected inliers), d1 float32 [B*N] or None (want_dist), row_lse float32 [B*N] / col_lse float32 [B*h*w]: the
    log-sum-exp of s over a point's pixels / over a pixel's selected points, or None (want_lse))."""
    who = "match_conf"
    B, h, w, C = _feature_pair(who, pc_feat_rows, img_feat_nhwc)
    _float32(who, "features", pc_feat_rows, img_feat_nhwc)
    N = _rows_per_sample(who, pc_feat_rows, B, h, w, 24)
    mask = _row_mask(who, "mask", mask, B * N)
    _gt_xy_arg(who, gt_xy, B, N)
    _f32_arg(who, "temperature", temperature, "be finite and > 0", lo_open=True)
    _f32_arg(who, "min_conf", min_conf, "lie in [0, 1] (0 = no threshold)", hi=1.0)
    _on_one_gpu(who, pc_feat_rows, img_feat_nhwc, mask, gt_xy, aligned=(pc_feat_rows, img_feat_nhwc))
    dev = pc_feat_rows.device
    idx = torch.empty((B * N,), dtype=torch.int32, device=dev)
    conf = torch.empty((B * N,), dtype=f32, device=dev)
    keep = torch.empty((B * N,), dtype=torch.uint8, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    d1 = torch.empty((B * N,), dtype=f32, device=dev) if want_dist else None
    row_lse = torch.empty((B * N,), dtype=f32, device=dev) if want_lse else None
    col_lse = torch.empty((B * h * w,), dtype=f32, device=dev) if want_lse else None
    nb = _lib.load().cmr_match_conf_workspace_bytes(B, N, h, w)
    ws = _ws(nb, dev)
    _lib.call("cmr_match_conf_f32", _p(pc_feat_rows), _p(img_feat_nhwc), C, B, N, h, w, _p(mask), mask.element_size(), float(temperature),
              float(min_conf), _p(gt_xy), float(thr), _p(idx), _p(conf), _p(keep), _p(counts), _p(d1), _p(row_lse), _p(col_lse), _p(ws), nb,
              _stream())
    return idx, conf, keep.view(torch.bool), counts, d1, row_lse, col_lse


def pnp_ransac(pts, uv, mask, K, n_hyp=1024, thr=1.0, seed=0, refine_iters=10, want_hyp_inliers=False):
    """Camera pose from 2-D/3-D correspondences, PnP inside RANSAC (include/cmr_hip.h cmr_pnp_ransac_f32): pts float32 [B, 3, N]
    (data['pc'] layout), uv float32 [B, 2, N] pixel coordinates on the map K refers to, mask [B, N] / [B*N] of bool / uint8 / int64
    (non-zero = use), K float32 [B, 3, 3]; n_hyp hypotheses, inlier threshold thr pixels, hash seed, up to refine_iters Gauss-Newton steps.
    -> (pose float32 [B, 4, 4] mapping pts into the camera frame, inliers int32 [B], status int32 [B] (0 ok, 1 fewer than 4
    correspondences, 2 no valid hypothesis)[, hyp_inliers int32 [B, n_hyp], -1 = invalid hypothesis])."""
    who = "pnp_ransac"
    B, _, N = _shaped(who, "pts", pts, "B", 3, "N")
    _shaped(who, "uv", uv, B, 2, N)
    _shaped(who, "K", K, B, 3, 3)
    _float32(who, "pts, uv and K", pts, uv, K)
    mask = _row_mask(who, "mask", mask, B * N)
    _cloud_range(who, B, N, 512)
    # n_hyp, refine_iters and seed take True for 1, which _is_int refuses: their own test
    if int(n_hyp) != n_hyp or not 1 <= n_hyp <= 1 << 20:
        raise ValueError("pnp_ransac: n_hyp must be an integer in [1, 2^20], got %r" % (n_hyp,))
    _f32_arg(who, "thr", thr, "be a finite positive number", lo_open=True)
    if int(refine_iters) != refine_iters or refine_iters < 0:
        raise ValueError("pnp_ransac: refine_iters must be a non-negative integer, got %r" % (refine_iters,))
    if int(seed) != seed or not 0 <= seed < 1 << 32:
        raise ValueError("pnp_ransac: seed must be an unsigned 32-bit integer, got %r" % (seed,))
    _on_one_gpu(who, pts, uv, mask, K)
    dev = pts.device
    n_hyp, refine_iters, seed = int(n_hyp), int(refine_iters), int(seed)
    pose = torch.empty((B, 4, 4), dtype=f32, device=dev)
    inliers = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    hyp = torch.empty((B, n_hyp), dtype=torch.int32, device=dev) if want_hyp_inliers else None
    nb = _lib.load().cmr_pnp_ransac_workspace_bytes(B, N, n_hyp)
    ws = _ws(nb, dev)
    _lib.call("cmr_pnp_ransac_f32", _p(pts), _p(uv), _p(mask), mask.element_size(), _p(K), B, N, n_hyp, float(thr), seed, refine_iters,
              _p(pose), _p(inliers), _p(status), _p(hyp), _p(ws), nb, _stream())
    return (pose, inliers, status, hyp) if want_hyp_inliers else (pose, inliers, status)


GUIDED_MAX_RADIUS = 16      # csrc/cmr_project.h CMR_MAX_RADIUS: every window radius below


def guided_match(pts, pc_feat_rows, img_feat_nhwc, mask, pose, K, radius, max_dist=0.0, gt_xy=None, thr=3.0, want_dist=False,
                 want_proj=False):
    """Nearest pixel feature of every selected point inside the (2 radius + 1)^2 window round its projection under `pose`
    (include/cmr_hip.h cmr_guided_match_f32): pts float32 [B, 3, N] (data['pc']), pc_feat rows [B*N, 64], img_feat NHWC
    [B, h, w, 64], mask [B, N] / [B*N] of bool / uint8 / int64, pose float32 [B, 4, 4] mapping pts into the camera frame, K float32
    [B, 3, 3] for the h x w map, 0 <= radius <= GUIDED_MAX_RADIUS, max_dist >= 0 (0 = off), optional gt_xy float32 [B, 2, N] with thr.
    -> (idx int32 [B*N]: pixel p = y * w + x or -1 (unselected / out of view), keep bool [B*N], counts int32 [B, 4] = (selected, in view,
    kept, kept inliers), dist float32 [B*N] or None (want_dist), proj float32 [B, 2, N] = (u, v) as the kernel computed them or None)."""
    who = "guided_match"
    B, _, N = _shaped(who, "pts", pts, "B", 3, "N")
    _, h, w, C = _feature_pair(who, pc_feat_rows, img_feat_nhwc, pts)
    _float32(who, "pts, features, pose and K", pts, pc_feat_rows, img_feat_nhwc, pose, K)
    _shaped(who, "pose", pose, B, 4, 4)
    _shaped(who, "K", K, B, 3, 3)
    _cloud_range(who, B, N, 256, h, w)
    mask = _row_mask(who, "mask", mask, B * N)
    _gt_xy_arg(who, gt_xy, B, N)
    _int_arg(who, "radius", radius, 0, GUIDED_MAX_RADIUS)
    _f32_arg(who, "max_dist", max_dist, "be finite and >= 0 (0 = no bound)")
    _on_one_gpu(who, pts, pc_feat_rows, img_feat_nhwc, mask, pose, K, gt_xy, aligned=(pc_feat_rows, img_feat_nhwc))
    dev = pts.device
    idx = torch.empty((B * N,), dtype=torch.int32, device=dev)
    keep = torch.empty((B * N,), dtype=torch.uint8, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    dist = torch.empty((B * N,), dtype=f32, device=dev) if want_dist else None
    proj = torch.empty((B, 2, N), dtype=f32, device=dev) if want_proj else None
    nb = _lib.load().cmr_guided_match_workspace_bytes(B, N)
    ws = _ws(nb, dev)
    _lib.call("cmr_guided_match_f32", _p(pts), _p(pc_feat_rows), _p(img_feat_nhwc), C, B, N, h, w, _p(mask), mask.element_size(), _p(pose),
              _p(K), int(radius), float(max_dist), _p(gt_xy), float(thr), _p(idx), _p(keep), _p(counts), _p(dist), _p(proj), _p(ws), nb,
              _stream())
    return idx, keep.view(torch.bool), counts, dist, proj


POSE_SCORE_MAX_POSES = 4096  # csrc/cmr_project.h CMR_MAX_POSES


def pose_score(pts, pc_feat_rows, img_feat_nhwc, mask, poses, K, radius=0, tau=0.8):
    """Truncated feature-metric cost of P candidate poses per sample in one sweep, with no ground truth (include/cmr_hip.h
    cmr_pose_score_f32): pts float32 [B, 3, N] (data['pc']), pc_feat rows [B*N, 64], img_feat NHWC [B, h, w, 64], mask
    [B, N] / [B*N] of bool / uint8 / int64, poses float32 [B, P, 4, 4] each mapping pts into the camera frame, 1 <= P <=
    POSE_SCORE_MAX_POSES, K float32 [B, 3, 3] for the h x w map, 0 <= radius <= GUIDED_MAX_RADIUS, tau finite and > 0.  Per pose and
    selected row: d = min(guided_match's dist under that pose, tau) if the row is in view, else tau; the row costs d^2 in float64.
    tau = 0.8 is a default for unit-norm features (two unrelated ones lie about sqrt(2) apart); it is not tuned on real data.
    -> (score float64 [B, P] = the sum over the selected rows, lower is better; counts int32 [B, P, 2] = (in view, in view and dist <=
    tau); selected int32 [B])."""
    who = "pose_score"
    B, _, N = _shaped(who, "pts", pts, "B", 3, "N")
    _, h, w, C = _feature_pair(who, pc_feat_rows, img_feat_nhwc, pts)
    _float32(who, "pts, features, poses and K", pts, pc_feat_rows, img_feat_nhwc, poses, K)
    P = _poses_arg(who, poses, B)
    _shaped(who, "K", K, B, 3, 3)
    _cloud_range(who, B, N, 256, h, w)
    mask = _row_mask(who, "mask", mask, B * N)
    _int_arg(who, "radius", radius, 0, GUIDED_MAX_RADIUS)
    _f32_arg(who, "tau", tau, "be a finite positive number", lo_open=True)
    nslices = (N + 255) // 256
    if nslices * ((P + 31) // 32) * B > 0x7fffffff:
        raise ValueError("pose_score: B=%d N=%d P=%d need more than 2^31 - 1 workgroups, score the poses or the samples in parts" % (B, N, P))
    _on_one_gpu(who, pts, pc_feat_rows, img_feat_nhwc, mask, poses, K, aligned=(pc_feat_rows, img_feat_nhwc))
    dev = pts.device
    score = torch.empty((B, P), dtype=torch.float64, device=dev)
    counts = torch.empty((B, P, 2), dtype=torch.int32, device=dev)
    selected = torch.empty((B,), dtype=torch.int32, device=dev)
    nb = _lib.load().cmr_pose_score_workspace_bytes(B, N, P)
    ws = _ws(nb, dev)
    _lib.call("cmr_pose_score_f32", _p(pts), _p(pc_feat_rows), _p(img_feat_nhwc), C, B, N, h, w, _p(mask), mask.element_size(), _p(poses),
              P, _p(K), int(radius), float(tau), _p(score), _p(counts), _p(selected), _p(ws), nb, _stream())
    return score, counts, selected


def visibility(pts, pose, K, h, w, mask, occ_mask=None, radius=1, rel_tol=0.05, abs_tol=0.0, want_depth_map=False, want_cell=False,
               want_depth=False):
    """Z-buffer visibility of the queried points and the rendered depth of the cloud under `pose` (include/cmr_hip.h cmr_visibility_f32,
    DESIGN.md 4r): pts float32 [B, 3, N] (data['pc']), pose float32 [B, 4, 4] mapping pts into the camera frame, K float32 [B, 3, 3] for
    the h x w map (1 <= h w <= 2^24; no features are read, so the 1/4-scale feature map and the full image both work), mask [B, N] /
    [B*N] of bool / uint8 / int64 = the rows that are queried, occ_mask the same = the rows that occlude (None: every row), 0 <= radius
    <= GUIDED_MAX_RADIUS, rel_tol and abs_tol finite and >= 0.  Z[b, y, x] = the least depth p2 of the occluder rows whose rounded
    projection is (x, y), +inf where there is none; a queried row in view (guided_match's predicate at radius 0) is visible iff its own
    depth z <= zmin * (1 + rel_tol) + abs_tol, zmin = the least Z over the (2 radius + 1)^2 window round its own cell.  radius = 1 and
    rel_tol = 0.05 are defaults for the 1/4-scale map; they are not tuned on real data.
    -> (visible bool [B*N], counts int32 [B, 4] = (selected, selected and in view, visible, occluder rows in view), depth_map float32
    [B, h, w] or None, cell int32 [B*N] = y * w + x of the rows of mask | occ_mask in view, else -1, or None, depth float32 [B*N] = p2 of
    those rows where p2 > 0, else NaN, or None)."""
    who = "visibility"
    B, N, h, w = _camera_args(who, pts, pose, K, h, w, "map", "float32")
    mask = _row_mask(who, "mask", mask, B * N)
    occ_mask = None if occ_mask is None else _row_mask(who, "occ_mask", occ_mask, B * N)
    radius, rel_tol, abs_tol = _depth_test_args(who, radius, rel_tol, abs_tol)
    _on_one_gpu(who, pts, pose, K, mask, occ_mask)
    dev = pts.device
    visible = torch.empty((B * N,), dtype=torch.uint8, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    depth_map = torch.empty((B, h, w), dtype=f32, device=dev) if want_depth_map else None
    cell = torch.empty((B * N,), dtype=torch.int32, device=dev) if want_cell else None
    depth = torch.empty((B * N,), dtype=f32, device=dev) if want_depth else None
    nb = _lib.load().cmr_visibility_workspace_bytes(B, N, h, w)
    ws = _ws(nb, dev)
    _lib.call("cmr_visibility_f32", _p(pts), _p(mask), mask.element_size(), _p(occ_mask), 1 if occ_mask is None else occ_mask.element_size(),
              _p(pose), _p(K), B, N, h, w, radius, rel_tol, abs_tol, _p(visible), _p(counts), _p(depth_map), _p(cell),
              _p(depth), _p(ws), nb, _stream())
    return visible.view(torch.bool), counts, depth_map, cell, depth


POINT_IMAGE_MAX_C = 64      # csrc/cmr_project.h CMR_MAX_PLANES
RENDER_MAX_SPLAT = 4        # csrc/point_image.hip PI_MAX_SPLAT
_PAINT_MODES = {"nearest": 0, "bilinear": 1}


def _point_attr(who, attr, B, N):
    """render_points' and render_surfels' attr float32 [B, C, N] or None -> C (0 without)"""
    if attr is None:
        return 0
    if not torch.is_tensor(attr) or attr.dtype != f32 or attr.dim() != 3 or attr.shape[0] != B or attr.shape[2] != N or not (
            1 <= attr.shape[1] <= POINT_IMAGE_MAX_C):
        raise ValueError("%s: attr must be float32 [%d, C, %d] with 1 <= C <= %d, got %s %s" % ((who, B, N, POINT_IMAGE_MAX_C) + _got(attr)))
    return attr.shape[1]


def paint_points(pts, pose, K, image, mask=None, mode='bilinear', want_uv=False):
    """The image laid over the cloud: every selected point that projects into `image` under `pose` takes the value of the pixel it lands
    on (include/cmr_hip.h cmr_paint_points_f32).  pts float32 [B, 3, N] (data['pc']), pose float32 [B, 4, 4] mapping pts
    into the camera frame, K float32 [B, 3, 3] for the H x W image, image float32 planar [B, C, H, W] with 1 <= C <= POINT_IMAGE_MAX_C
    and 1 <= H W <= 2^24, mask [B, N] / [B*N] of bool / uint8 / int64 (None: every row; pass ops.visibility's flags to paint only what
    the camera sees).  In view is ops.visibility's predicate (guided_match's at radius 0).  mode 'nearest': the pixel at the rounded
    projection, the cell ops.visibility reports; 'bilinear': the four pixels round (u, v), pixel centres on the integers, border
    replicate, each lerp a + t (b - a) rounded operation by operation.
    -> (colors float32 [B, C, N], 0 on the rows that are not painted; painted bool [B*N]; counts int32 [B, 2] = (selected, painted); uv
    float32 [B, 2, N] = (u, v) as computed, NaN for unselected rows and behind the camera (guided_match's proj), or None)."""
    if not torch.is_tensor(image) or image.dim() != 4:
        raise ValueError("paint_points: image must be planar [B, C, H, W], got %s" % (
            tuple(image.shape) if torch.is_tensor(image) else type(image).__name__,))
    Bi, C, H, W = image.shape
    B, N, H, W = _camera_args("paint_points", pts, pose, K, H, W)
    mask = _row_mask("paint_points", "mask", mask, B * N, or_none=True)
    if image.dtype != f32:
        raise ValueError("paint_points: image must be float32, got %s" % (image.dtype,))
    if Bi != B or C < 1 or C > POINT_IMAGE_MAX_C:
        raise ValueError("paint_points: image must be [%d, C, H, W] with 1 <= C <= %d, got %s" % (B, POINT_IMAGE_MAX_C, tuple(image.shape)))
    if not isinstance(mode, str) or mode not in _PAINT_MODES:
        raise ValueError("paint_points: mode must be 'nearest' or 'bilinear', got %r" % (mode,))
    _on_one_gpu("paint_points", pts, pose, K, image, mask)
    dev = pts.device
    colors = torch.empty((B, C, N), dtype=f32, device=dev)
    painted = torch.empty((B * N,), dtype=torch.uint8, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    uv = torch.empty((B, 2, N), dtype=f32, device=dev) if want_uv else None
    _lib.call("cmr_paint_points_f32", _p(pts), _p(mask), 1 if mask is None else mask.element_size(), _p(pose), _p(K), _p(image), B, N, C, H, W,
              _PAINT_MODES[mode], _p(colors), _p(painted), _p(counts), _p(uv), _stream())
    return colors, painted.view(torch.bool), counts, uv


def render_points(pts, pose, K, h, w, attr=None, mask=None, splat=0, fill=0.0):
    """The cloud laid over the image: a z-buffer that remembers its owner (include/cmr_hip.h cmr_render_points_f32).  pts
    float32 [B, 3, N], pose float32 [B, 4, 4], K float32 [B, 3, 3] for the h x w map (1 <= h w <= 2^24), attr float32 [B, C, N] with
    1 <= C <= POINT_IMAGE_MAX_C or None, mask [B, N] / [B*N] of bool / uint8 / int64 (None: every row), 0 <= splat <= RENDER_MAX_SPLAT,
    fill any float (NaN included).  Every selected row in view (ops.visibility's predicate and cell) competes for its cell with the key
    (bits of depth) << 32 | n; the least key owns the cell -- the nearest row, the lowest n on equal depths -- and a pixel is owned by the
    least key within `splat` cells of it in both axes.
    -> (index_map int32 [B, h, w], -1 where no row owns the pixel; depth_map float32 [B, h, w], +inf there; attr_map float32 [B, C, h, w]
    = attr[b, :, owner], `fill` there, or None without attr; counts int32 [B, 3] = (selected, selected and in view, pixels with an
    owner))."""
    who = "render_points"
    B, N, h, w = _camera_args(who, pts, pose, K, h, w)
    mask = _row_mask(who, "mask", mask, B * N, or_none=True)
    C = _point_attr(who, attr, B, N)
    _int_arg(who, "splat", splat, 0, RENDER_MAX_SPLAT)
    fill = _f32_arg(who, "fill", fill, "be a number", lo=None)
    _on_one_gpu(who, pts, pose, K, attr, mask)
    index_map, depth_map, attr_map, ws, nb = _render_maps(B, C, h, w, pts.device, "cmr_render_points_workspace_bytes")
    counts = torch.empty((B, 3), dtype=torch.int32, device=pts.device)
    _lib.call("cmr_render_points_f32", _p(pts), _p(mask), 1 if mask is None else mask.element_size(), _p(pose), _p(K), _p(attr), C, B, N, h, w,
              int(splat), fill, _p(index_map), _p(depth_map), _p(attr_map), _p(counts), _p(ws), nb, _stream())
    return index_map, depth_map, attr_map, counts


SURFEL_MAX_PX = 16          # csrc/cmr_project.h CMR_MAX_RADIUS


def render_surfels(pts, normals, pose, K, h, w, radius=0.1, range_slope=0.004, max_px=8, min_cos=0.1, attr=None, mask=None, fill=0.0,
                   want_normal_map=False, want_surfel=False):
    """The cloud drawn as oriented discs (surfels): every selected point is a disc in space, centred on it, perpendicular to its normal,
    r = radius + range_slope z_c metres wide, and every pixel intersects its own ray with that disc (include/cmr_hip.h
    cmr_render_surfels_f32).  pts and normals float32 [B, 3, N] (normals in the cloud's frame, any length; a zero row is
    drawn fronto-parallel, a non-finite one is not drawn), pose float32 [B, 4, 4], K float32 [B, 3, 3] for the h x w map (1 <= h w <=
    2^24) of the form [[fx, s, cx], [0, fy, cy], [0, 0, 1]] (checked on the device: a sample whose K is not draws nothing and has status
    1), radius and range_slope finite and >= 0, 0 <= max_px <= SURFEL_MAX_PX (a disc is cut to the (2 max_px + 1)^2 pixels round its
    centre), 0 <= min_cos <= 1 (a pixel whose ray meets the plane at a cosine below it is not covered), attr float32 [B, C, N] with
    1 <= C <= POINT_IMAGE_MAX_C or None, mask [B, N] / [B*N] of bool / uint8 / int64 (None: every row), fill any float.  The nearest disc
    owns a pixel, the lowest row on equal depths.  radius = 0.1 is one voxel of the prepared clouds and range_slope = 0.004 about half
    of KITTI's ring spacing per metre of range; these defaults, max_px and min_cos are not tuned on real data.
    -> (index_map int32 [B, h, w], -1 where no disc covers the pixel; depth_map float32 [B, h, w], the depth of the owner's plane there,
    +inf where none; attr_map float32 [B, C, h, w] or None; counts int32 [B, 4] = (selected, drawn, pixels with an owner, status);
    normal_map float32 [B, 3, h, w] (unit, facing the camera, 0 where no owner) or None; surfel float32 [B, 8, N] = (x_c, y_c, z_c, n_cx,
    n_cy, n_cz, r, drawn) as computed, NaN in the first seven planes of undrawn rows, or None)."""
    who = "render_surfels"
    B, N, h, w = _camera_args(who, pts, pose, K, h, w)
    mask = _row_mask(who, "mask", mask, B * N, or_none=True)
    if not torch.is_tensor(normals) or normals.dtype != f32 or tuple(normals.shape) != (B, 3, N):
        raise ValueError("render_surfels: normals must be float32 [%d, 3, %d], got %s %s" % ((B, N) + _got(normals)))
    C = _point_attr(who, attr, B, N)
    # the second closing bracket is the wording these three have had, and callers may match on it
    radius = _f32_arg(who, "radius", radius, "be a finite number in [0, inf)]", bools=False)
    range_slope = _f32_arg(who, "range_slope", range_slope, "be a finite number in [0, inf)]", bools=False)
    min_cos = _f32_arg(who, "min_cos", min_cos, "be a finite number in [0, 1]]", hi=1.0, bools=False)
    _int_arg(who, "max_px", max_px, 0, SURFEL_MAX_PX)
    fill = _f32_arg(who, "fill", fill, "be a number", lo=None)
    _on_one_gpu(who, pts, normals, pose, K, attr, mask)
    dev = pts.device
    index_map, depth_map, attr_map, ws, nb = _render_maps(B, C, h, w, dev, "cmr_render_surfels_workspace_bytes")
    normal_map = torch.empty((B, 3, h, w), dtype=f32, device=dev) if want_normal_map else None
    surfel = torch.empty((B, 8, N), dtype=f32, device=dev) if want_surfel else None
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    _lib.call("cmr_render_surfels_f32", _p(pts), _p(normals), _p(mask), 1 if mask is None else mask.element_size(), _p(pose), _p(K), _p(attr),
              C, B, N, h, w, radius, range_slope, int(max_px), min_cos, fill, _p(index_map), _p(depth_map), _p(normal_map), _p(attr_map),
              _p(counts), _p(surfel), _p(ws), nb, _stream())
    return index_map, depth_map, attr_map, counts, normal_map, surfel


def depth_test(pts, pose, K, depth_map, mask, radius=0, rel_tol=0.05, abs_tol=0.0):
    """ops.visibility's depth test against a z-buffer the caller brings (include/cmr_hip.h cmr_depth_test_f32): depth_map
    float32 [B, h, w], +inf where empty -- ops.render_surfels' for a hole-free occluder, or ops.visibility's own, which gives that op's
    flags back bit for bit.  pts float32 [B, 3, N], pose float32 [B, 4, 4], K float32 [B, 3, 3] for the h x w map, mask [B, N] / [B*N] of
    bool / uint8 / int64 = the rows that are queried, 0 <= radius <= GUIDED_MAX_RADIUS, rel_tol and abs_tol finite and >= 0.  A queried
    row in view (the predicate at radius 0) is visible iff its depth z <= zmin * (1 + rel_tol) + abs_tol, zmin = the least depth_map
    value over the (2 radius + 1)^2 window round its own cell.  A surfel map is continuous, so radius defaults to 0 here; like rel_tol
    = 0.05 it is not tuned on real data.
    -> (visible bool [B*N], counts int32 [B, 3] = (selected, selected and in view, visible))."""
    if not torch.is_tensor(depth_map) or depth_map.dim() != 3 or depth_map.dtype != f32:
        raise ValueError("depth_test: depth_map must be float32 [B, h, w], got %s %s" % _got(depth_map))
    Bd, h, w = depth_map.shape
    if mask is None:
        raise ValueError("depth_test: mask must be bool / uint8 / int64 (the rows that are queried), got None")
    B, N, h, w = _camera_args("depth_test", pts, pose, K, h, w)
    mask = _row_mask("depth_test", "mask", mask, B * N, or_none=True)
    if Bd != B:
        raise ValueError("depth_test: depth_map must be float32 [%d, h, w], got %s" % (B, tuple(depth_map.shape)))
    radius, rel_tol, abs_tol = _depth_test_args("depth_test", radius, rel_tol, abs_tol)
    _on_one_gpu("depth_test", pts, pose, K, depth_map, mask)
    dev = pts.device
    visible = torch.empty((B * N,), dtype=torch.uint8, device=dev)
    counts = torch.empty((B, 3), dtype=torch.int32, device=dev)
    _lib.call("cmr_depth_test_f32", _p(pts), _p(mask), mask.element_size(), _p(pose), _p(K), _p(depth_map), B, N, h, w, radius, rel_tol,
              abs_tol, _p(visible), _p(counts), _stream())
    return visible.view(torch.bool), counts


POSE_MI_MAX_BINS = 64       # csrc/pose_mi.hip PMI_MAX_BINS
POSE_MI_SLICE = 4096        # csrc/pose_mi.hip PMI_SLICE: rows per workgroup


def pose_mi_chunk(bins):
    """Poses per workgroup of cmr_pose_mi_f32 (csrc/pose_mi.hip pmi_chunk): the chunk's histograms take at most 32 KB of LDS."""
    return min(8, (32 * 1024) // (bins * bins * 4))


def _pose_mi_range(name, r, bins):
    """(lo, hi) as the fp32 values the kernel takes, or a ValueError: both finite, lo < hi and bins / (hi - lo) finite in fp32."""
    try:
        lo, hi = (float(torch.tensor(float(v), dtype=f32)) for v in r)
        ok = abs(lo) < float("inf") and abs(hi) < float("inf") and lo < hi and float(torch.tensor(bins / (hi - lo), dtype=f32)) < float("inf")
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("pose_mi: %s must be (lo, hi), finite in float32 with lo < hi and bins / (hi - lo) finite, got %r" % (name, r))
    return lo, hi


def pose_mi(pts, attr, grey, mask, poses, K, bins=32, mode='nearest', attr_range=(0.0, 1.0), grey_range=(0.0, 1.0), want_hist=False):
    """Mutual information of a per-point attribute and the image's grey values under P candidate poses per sample, in one sweep
    (include/cmr_hip.h cmr_pose_mi_f32): a pose score that reads the sensors alone.  pts float32 [B, 3, N] (data['pc']),
    attr float32 [B, N] (the LiDAR reflectance, data['pc_intensity']), grey float32 [B, H, W] (one plane, 1 <= H W <= 2^24), mask
    [B, N] / [B*N] of bool / uint8 / int64 (None: every row), poses float32 [B, P, 4, 4] each mapping pts into the camera frame,
    1 <= P <= POSE_SCORE_MAX_POSES, K float32 [B, 3, 3] for the H x W image, 2 <= bins <= POSE_MI_MAX_BINS, mode 'nearest' or
    'bilinear' (ops.paint_points' sampling), attr_range / grey_range = (lo, hi) of the histogram's axes (values outside go to the end
    bins).  Per pose a selected row is counted iff it is in view (ops.paint_points' predicate) and its attribute and grey value -- the
    value ops.paint_points gives it at C = 1 -- are finite; bin = min(bins - 1, max(0, floor((x - lo) * scale))), scale = bins /
    (hi - lo) rounded once to float32.
    -> (mi float64 [B, P] = H_a + H_g - H_ag in nats, higher is better; entropy float64 [B, P, 3] = (H_a, H_g, H_ag); counts int32
    [B, P, 2] = (in view, counted); selected int32 [B]; hist int32 [B, P, bins, bins] (attribute bin, grey bin) or None)."""
    who = "pose_mi"
    B, _, N = _shaped(who, "pts", pts, "B", 3, "N")
    if not all(torch.is_tensor(t) for t in (attr, grey, poses, K)):
        raise ValueError("pose_mi: attr, grey, poses and K must be tensors")
    _float32(who, "pts, attr, grey, poses and K", pts, attr, grey, poses, K)
    _shaped(who, "attr", attr, B, N)
    if grey.dim() != 3 or grey.shape[0] != B:
        raise ValueError("pose_mi: grey must be one plane per sample [%d, H, W], got %s" % (B, tuple(grey.shape)))
    H, W = grey.shape[1:]
    P = _poses_arg(who, poses, B)
    _shaped(who, "K", K, B, 3, 3)
    _cloud_range(who, B, N, 256, H, W, "image")
    mask = _row_mask(who, "mask", mask, B * N, or_none=True)
    bins = _int_arg(who, "bins", bins, 2, POSE_MI_MAX_BINS)
    if not isinstance(mode, str) or mode not in _PAINT_MODES:
        raise ValueError("pose_mi: mode must be 'nearest' or 'bilinear', got %r" % (mode,))
    a_lo, a_hi = _pose_mi_range("attr_range", attr_range, bins)
    g_lo, g_hi = _pose_mi_range("grey_range", grey_range, bins)
    chunk = pose_mi_chunk(bins)
    if ((N + POSE_MI_SLICE - 1) // POSE_MI_SLICE) * ((P + chunk - 1) // chunk) * B > 0x7fffffff:
        raise ValueError("pose_mi: B=%d N=%d P=%d need more than 2^31 - 1 workgroups, score the poses or the samples in parts" % (B, N, P))
    _on_one_gpu(who, pts, attr, grey, mask, poses, K)
    dev = pts.device
    hist = torch.empty((B, P, bins, bins), dtype=torch.int32, device=dev)
    counts = torch.empty((B, P, 2), dtype=torch.int32, device=dev)
    selected = torch.empty((B,), dtype=torch.int32, device=dev)
    entropy = torch.empty((B, P, 3), dtype=torch.float64, device=dev)
    mi = torch.empty((B, P), dtype=torch.float64, device=dev)
    _lib.call("cmr_pose_mi_f32", _p(pts), _p(attr), _p(mask), 1 if mask is None else mask.element_size(), _p(poses), P, _p(K), _p(grey), B, N,
              H, W, _PAINT_MODES[mode], bins, a_lo, a_hi, g_lo, g_hi, _p(hist), _p(counts), _p(selected), _p(entropy), _p(mi), _stream())
    return mi, entropy, counts, selected, hist if want_hist else None


DENSIFY_MAX_RADIUS = 16     # csrc/cmr_project.h CMR_MAX_RADIUS
DENSIFY_MAX_C = 4           # csrc/densify.hip DN_MAX_C: attribute planes, and guide planes
DENSIFY_TILE_W = 64         # csrc/densify.hip DN_TW x DN_TH: the pixels of one workgroup (tests put their shapes round these)
DENSIFY_TILE_H = 16
DENSIFY_MIN_WEIGHT = 1e-24


def densify(depth, guide=None, attr=None, radius=8, sigma_s=None, sigma_r=0.1, min_weight=1e-3, keep=True, fill=0.0, want_count=False):
    """Image-guided densification of a sparse depth map and of attribute planes that ride on it: the joint bilateral filter as a
    normalised convolution (include/cmr_hip.h cmr_densify_f32).  depth float32 [B, h, w] with 1 <= h w <= 2^24: a pixel is
    a sample iff its depth is finite and > 0 (ops.render_points and ops.visibility write +inf where nothing landed; 0, negatives and NaN
    are empty too).  guide float32 [B, Cg, h, w] with 1 <= Cg <= DENSIFY_MAX_C or None; it must be finite, which is NOT checked.  attr
    float32 [B, C, h, w] with 1 <= C <= DENSIFY_MAX_C or None, read at samples only (render_points' fill is never read).  0 <= radius <=
    DENSIFY_MAX_RADIUS; sigma_s > 0 (None: max(radius, 1) / 2); sigma_r > 0, ignored without a guide; min_weight finite and >=
    DENSIFY_MIN_WEIGHT; fill any float (NaN included).  sigma_s, sigma_r and min_weight act as their float32 values.  Every pixel p sums
    over the samples q within `radius` of it in both axes: w = exp(-(|p - q|^2 / (2 sigma_s^2) + sum_c (G_c(p) - G_c(q))^2 /
    (2 sigma_r^2))), S0 = sum w, and is filled iff S0 >= min_weight; with keep a pixel that is a sample keeps its own depth and
    attributes bit for bit.  The defaults (radius 8, sigma_r 0.1 for a guide in [0, 1], min_weight 1e-3) are not tuned on real data.
    -> (dense_depth float32 [B, h, w] = sum w z / S0, +inf where not filled; dense_attr float32 [B, C, h, w] = sum w a / S0, `fill`
    where not filled, or None without attr; conf float32 [B, h, w] = S0; count int32 [B, h, w] = the samples in the window, or None;
    counts int32 [B, 3] = (samples in the map, pixels with a sample in their window, filled pixels))."""
    if not torch.is_tensor(depth) or depth.dim() != 3:
        raise ValueError("densify: depth must be [B, h, w], got %s" % (tuple(depth.shape) if torch.is_tensor(depth) else type(depth).__name__,))
    B, h, w = depth.shape
    if depth.dtype != f32:
        raise ValueError("densify: depth must be float32, got %s" % (depth.dtype,))
    if B < 1 or B > GRID_Y_MAX or h < 1 or w < 1 or h * w > 1 << 24:
        raise ValueError("densify: need 1 <= B <= %d and a map of 1 .. 2^24 pixels, got B=%d map %d x %d" % (GRID_Y_MAX, B, h, w))
    C = Cg = 0
    if guide is not None:
        if not torch.is_tensor(guide) or guide.dtype != f32 or guide.dim() != 4 or guide.shape[0] != B or tuple(guide.shape[2:]) != (h, w) \
                or not 1 <= guide.shape[1] <= DENSIFY_MAX_C:
            raise ValueError("densify: guide must be float32 [%d, Cg, %d, %d] with 1 <= Cg <= %d, got %s %s" % ((B, h, w, DENSIFY_MAX_C) + _got(guide)))
        Cg = guide.shape[1]
    if attr is not None:
        if not torch.is_tensor(attr) or attr.dtype != f32 or attr.dim() != 4 or attr.shape[0] != B or tuple(attr.shape[2:]) != (h, w) \
                or not 1 <= attr.shape[1] <= DENSIFY_MAX_C:
            raise ValueError("densify: attr must be float32 [%d, C, %d, %d] with 1 <= C <= %d, got %s %s" % ((B, h, w, DENSIFY_MAX_C) + _got(attr)))
        C = attr.shape[1]
    _int_arg("densify", "radius", radius, 0, DENSIFY_MAX_RADIUS)
    if sigma_s is None:
        sigma_s = max(int(radius), 1) / 2
    _f32_arg("densify", "sigma_s", sigma_s, "be finite and > 0", lo_open=True)
    _f32_arg("densify", "sigma_r", sigma_r, "be finite and > 0", lo_open=True)
    _f32_arg("densify", "min_weight", min_weight, "be finite and >= %g" % DENSIFY_MIN_WEIGHT, lo=DENSIFY_MIN_WEIGHT)
    coefs = [math.log2(math.e) / (2.0 * float(s) ** 2) for s in ((sigma_s, sigma_r) if Cg else (sigma_s,))]      # the kernel's exponents' factors
    if not all(0.0 < float(torch.tensor(c, dtype=f32)) < math.inf for c in coefs):
        raise ValueError("densify: 1 / (2 sigma^2) must be a float32 > 0, got sigma_s=%r sigma_r=%r" % (sigma_s, sigma_r))
    if not isinstance(keep, (bool, int)) or keep not in (0, 1):
        raise ValueError("densify: keep must be True or False, got %r" % (keep,))
    fill = _f32_arg("densify", "fill", fill, "be a number", lo=None)
    _on_one_gpu("densify", depth, guide, attr)
    dev = depth.device
    dense_depth = torch.empty((B, h, w), dtype=f32, device=dev)
    dense_attr = torch.empty((B, C, h, w), dtype=f32, device=dev) if attr is not None else None
    conf = torch.empty((B, h, w), dtype=f32, device=dev)
    count = torch.empty((B, h, w), dtype=torch.int32, device=dev) if want_count else None
    counts = torch.empty((B, 3), dtype=torch.int32, device=dev)
    _lib.call("cmr_densify_f32", _p(depth), _p(attr), C, _p(guide), Cg, B, h, w, int(radius), float(sigma_s), float(sigma_r),
              float(min_weight), int(bool(keep)), fill, _p(dense_depth), _p(dense_attr), _p(conf), _p(count), _p(counts), _stream())
    return dense_depth, dense_attr, conf, count, counts


def pnp_refine(pts, uv, mask, K, pose, thr=1.0, iters=10):
    """Gauss-Newton refinement of a given pose on 2-D/3-D correspondences (include/cmr_hip.h cmr_pnp_refine_f32): pts
    float32 [B, 3, N], uv float32 [B, 2, N], mask [B, N] / [B*N] of bool / uint8 / int64, K float32 [B, 3, 3], pose float32 [B, 4, 4]
    (finite; maps pts into the camera frame); the rows that are inliers of `pose` within thr pixels are the working set, up to iters steps.
    -> (pose float32 [B, 4, 4], inliers int32 [B], status int32 [B]: 0 refined, 1 fewer than 4 rows in the working set, 2 refinement
    not kept; 1 and 2 return the input pose)."""
    who = "pnp_refine"
    B, _, N = _shaped(who, "pts", pts, "B", 3, "N")
    _shaped(who, "uv", uv, B, 2, N)
    _shaped(who, "K", K, B, 3, 3)
    _shaped(who, "pose", pose, B, 4, 4)
    _float32(who, "pts, uv, K and pose", pts, uv, K, pose)
    mask = _row_mask(who, "mask", mask, B * N)
    _cloud_range(who, B, N, 1024)
    _f32_arg(who, "thr", thr, "be a finite positive number", lo_open=True)
    _int_arg(who, "iters", iters, 0, 1000)
    _on_one_gpu(who, pts, uv, mask, K, pose)
    dev = pts.device
    out = torch.empty((B, 4, 4), dtype=f32, device=dev)
    inliers = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    nb = _lib.load().cmr_pnp_refine_workspace_bytes(B, N)
    ws = _ws(nb, dev)
    _lib.call("cmr_pnp_refine_f32", _p(pts), _p(uv), _p(mask), mask.element_size(), _p(K), _p(pose), B, N, float(thr), int(iters), _p(out),
              _p(inliers), _p(status), _p(ws), nb, _stream())
    return out, inliers, status


def match_subpixel(pc_feat_rows, img_feat_nhwc, idx, mask=None, gt_xy=None, thr=0.5):
    """Sub-pixel positions of given matches by a parabola fit on the squared feature distances of the matched pixel and its two
    neighbours per axis (include/cmr_hip.h cmr_match_subpixel_f32): pc_feat rows [B*N, 64], img_feat NHWC [B, h, w, 64],
    idx int32 with B*N elements (the idx of feat_match / feat_match_filter / guided_match), optional mask [B, N] / [B*N] of bool / uint8 /
    int64 (non-zero = use the row), optional gt_xy float32 [B, 2, N] with threshold thr in pixels.  A row is matched when its mask is
    non-zero and 0 <= idx < h * w.
    -> (uv float32 [B, 2, N] = (x + dx, y + dy) with |dx|, |dy| <= 0.5, NaN on unmatched rows, counts int32 [B, 4] = (matched, fitted on
    both axes, matched whose integer pixel is within thr of gt_xy, matched whose sub-pixel position is))."""
    who = "match_subpixel"
    B, h, w, C = _feature_pair(who, pc_feat_rows, img_feat_nhwc)
    if B < 1 or pc_feat_rows.shape[0] % B:
        raise ValueError("match_subpixel: point rows %s and pixel features %s do not agree on B and N" % (
            tuple(pc_feat_rows.shape), tuple(img_feat_nhwc.shape)))
    N = pc_feat_rows.shape[0] // B
    _float32(who, "features", pc_feat_rows, img_feat_nhwc)
    if idx.dtype != torch.int32 or idx.numel() != B * N:
        raise ValueError("match_subpixel: idx must be int32 with %d elements, got %s %s" % (B * N, idx.dtype, tuple(idx.shape)))
    mask = None if mask is None else _row_mask(who, "mask", mask, B * N)
    _gt_xy_arg(who, gt_xy, B, N)
    _f32_arg(who, "thr", thr, "be a finite positive number", lo_open=True, as_f32=False)    # the kernel compares with whatever float32 makes of it
    _cloud_range(who, B, N, 256, h, w)
    _on_one_gpu(who, pc_feat_rows, img_feat_nhwc, idx, mask, gt_xy, aligned=(pc_feat_rows, img_feat_nhwc))
    dev = pc_feat_rows.device
    uv = torch.empty((B, 2, N), dtype=f32, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    _lib.call("cmr_match_subpixel_f32", _p(pc_feat_rows), _p(img_feat_nhwc), C, B, N, h, w, _p(idx), _p(mask),
              mask.element_size() if mask is not None else 0, _p(gt_xy), float(thr), _p(uv), _p(counts), _stream())
    return uv, counts


def expert_action(pose_source, pose_target, r_steps, t_steps, six_dof):
    """-> (action_r int64 [B, 1|3], action_t int64 [B, 2|3]); the step tables are float64 device tensors."""
    B = pose_source.shape[0]
    ar = torch.empty((B, 3 if six_dof else 1), dtype=torch.int64, device=pose_source.device)
    at = torch.empty((B, 3 if six_dof else 2), dtype=torch.int64, device=pose_source.device)
    _lib.call("cmr_expert_action_f32", _p(pose_source), _p(pose_target), _p(r_steps), _p(t_steps), r_steps.numel(), int(six_dof),
              _p(ar), _p(at), B, _stream())
    return ar, at


def reward(pc, pc_in_cam, mask_i64, prev_distance=None):
    """planar clouds [B,3,N], mask int64 [B,N] -> (reward [B], distance [B])."""
    B, _, N = pc.shape
    dist = torch.empty((B,), dtype=f32, device=pc.device)
    rew = torch.empty((B,), dtype=f32, device=pc.device)
    _lib.call("cmr_reward_f32", _p(pc), _p(pc_in_cam), _p(mask_i64), _p(prev_distance), _p(dist), _p(rew), B, N, _stream())
    return rew, dist


def discounted(vals, gamma):
    """Reverse discounted cumulative sum along the last axis of a contiguous float32 tensor."""
    if not vals.is_contiguous() or vals.dtype != f32:
        raise ValueError("discounted expects a contiguous float32 tensor")
    out = torch.empty_like(vals)
    T = vals.shape[-1]
    _lib.call("cmr_discounted_f32", _p(vals), _p(out), float(gamma), vals.numel() // T, T, _stream())
    return out


def argmax_rows(x):
    """x [outer, inner, n] (unit stride on the last dim) -> int64 [outer, inner]."""
    outer, inner, n = x.shape
    if x.stride(2) != 1:
        raise ValueError("argmax_rows needs unit stride on the last dim")
    out = torch.empty((outer, inner), dtype=torch.int64, device=x.device)
    _lib.call("cmr_argmax_rows_f32", _p(x), _p(out), outer, inner, n, x.stride(0), x.stride(1), _stream())
    return out


def softmax2(logits, thr_lo=0.5, thr_hi=0.8):
    _rows(logits)
    rows = logits.shape[0]
    prob = torch.empty((rows,), dtype=f32, device=logits.device)
    lo = torch.empty((rows,), dtype=torch.uint8, device=logits.device)
    hi = torch.empty((rows,), dtype=torch.uint8, device=logits.device)
    _lib.call("cmr_softmax2_f32", _p(logits), _ld(logits), _p(prob), _p(lo), _p(hi), thr_lo, thr_hi, rows, _stream())
    return prob, lo, hi


def l2norm64(x, out=None):
    _rows(x)
    if out is None:
        out = torch.empty((x.shape[0], 64), dtype=f32, device=x.device)
    _lib.call("cmr_l2norm64_f32", _p(x), _ld(x), _p(out), _ld(out), x.shape[0], _stream())
    return out


# ----------------------------------------------------------------------------------------------------------------------
# agent update: training-mode BatchNorm, backward pieces, loss, optimizer -- see include/cmr_hip.h
# ----------------------------------------------------------------------------------------------------------------------
def _ws(nbytes, dev):
    return torch.empty((max(int(nbytes) // 4, 1),), dtype=f32, device=dev)


def bn_stats(x, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1):
    """x [rows, C] -> stat [4, C] = (mean, rstd, scale, shift); updates the running statistics in place when given."""
    _rows(x)
    rows, C = x.shape
    stat = torch.empty((4, C), dtype=f32, device=x.device)
    nb = _lib.load().cmr_bn_workspace_bytes(rows, C)
    ws = _ws(nb, x.device)
    _lib.call("cmr_bn_stats_f32", _p(x), _ld(x), rows, C, float(eps), float(momentum), _p(gamma), _p(beta), _p(running_mean),
              _p(running_var), _p(stat), _p(ws), nb, _stream())
    return stat


def affine_act(x, scale=None, shift=None, res=None, rscale=None, rshift=None, slope=1.0, out=None):
    _rows(x)
    rows, C = x.shape
    if out is None:
        out = torch.empty((rows, C), dtype=f32, device=x.device)
    _lib.call("cmr_affine_act_f32", _p(x), _ld(x), _p(scale), _p(shift), _p(res), _ld(res) if res is not None else 0, _p(rscale),
              _p(rshift), _p(out), _ld(out), rows, C, float(slope), _stream())
    return out


def bn_bwd(dz, z, slope, x, stat, dgamma=None, dbeta=None, add=None, out=None, want_masked=False):
    """Backward of [BatchNorm(train) -> LeakyReLU(slope)] -> dx [rows, C].  z None: slope 1 = no activation, any other slope = the mask is
    recomputed from x and stat (the activation sat directly on the BatchNorm output); want_masked: -> (dx, dz * act'(z)), the second one
    being the gradient a residual branch added in front of the activation receives."""
    _rows(dz), _rows(x)
    rows, C = x.shape
    if out is None:
        out = torch.empty((rows, C), dtype=f32, device=x.device)
    dzm = torch.empty((rows, C), dtype=f32, device=x.device) if want_masked else None
    nb = _lib.load().cmr_bn_bwd_workspace_bytes(rows, C)
    ws = _ws(nb, x.device)
    _lib.call("cmr_bn_bwd_f32", _p(dz), _ld(dz), _p(z), _ld(z) if z is not None else 0, float(slope), _p(x), _ld(x), _p(stat), _p(add),
              _ld(add) if add is not None else 0, _p(out), _ld(out), _p(dzm), C if want_masked else 0, _p(dgamma), _p(dbeta), rows, C, _p(ws), nb,
              _stream())
    return (out, dzm) if want_masked else out


def linear_bn_fwd_ok(rows, n, k):
    return n in (64, 128) and k in (64, 128) and rows >= 32 and rows % 32 == 0


def linear_bn_fwd(x, w, bias, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1, pro=None, pro_slope=1.0, bias_seg_rows=0):
    """-> (h [rows, n] = x' W^T + bias, stat [4, n] = bn_stats(h)) in one pass; pro = the previous layer's stat [4, k]: x' =
    lrelu_{pro_slope}(x * pro[2] + pro[3]) (x is then that layer's BatchNorm input).  bias_seg_rows: bias is [rows / bias_seg_rows, n], one
    row per segment (sample).  False when the shape is not served."""
    _rows(x)
    rows, k = x.shape
    n = gamma.numel()
    if not linear_bn_fwd_ok(rows, n, k) or w.shape[0] < n or w.shape[1] != k or w.stride(1) != 1:
        return False
    if bias_seg_rows and (bias_seg_rows < 128 or bias_seg_rows % 32 or rows % bias_seg_rows):
        return False
    if bias_seg_rows and (bias is None or tuple(bias.shape) != (rows // bias_seg_rows, n) or bias.stride(1) != 1):
        raise ValueError("linear_bn_fwd: per-segment bias must be [%d, %d]" % (rows // bias_seg_rows, n))
    if pro is not None and tuple(pro.shape) != (4, k):
        raise ValueError("linear_bn_fwd: prologue statistics %s for an input of width %d" % (tuple(pro.shape), k))
    h = torch.empty((rows, n), dtype=f32, device=x.device)
    stat = torch.empty((4, n), dtype=f32, device=x.device)
    bf = bool(CONV_BF16 and BN_LINEAR_BF16_FWD and w.stride(0) % 4 == 0 and w.data_ptr() % 16 == 0)
    nb = getattr(_lib.load(), "cmr_linear_bn_fwd_bf16_workspace_bytes" if bf else "cmr_linear_bn_fwd_workspace_bytes")(rows, n, k)
    ws = _ws(nb, x.device)
    _lib.call("cmr_linear_bn_fwd_bf16_f32" if bf else "cmr_linear_bn_fwd_f32", _p(x), _ld(x), k, _p(pro), float(pro_slope), _p(w), w.stride(0), _p(bias), int(bias_seg_rows),
              bias.stride(0) if bias_seg_rows else 0, _p(h), n, rows, n, float(eps), float(momentum), _p(gamma), _p(beta), _p(running_mean),
              _p(running_var), _p(stat), _p(ws), nb, _stream())
    return h, stat


def bn_bwd_coef(dz, z, slope, x, stat, dgamma=None, dbeta=None):
    """The reduction half of bn_bwd alone -> coef [2, C] = (mean(dy), mean(dy xhat)) (and dgamma / dbeta): the apply half rides in
    bn_linear_bwd's prologue."""
    _rows(dz), _rows(x)
    rows, C = x.shape
    coef = torch.empty((2, C), dtype=f32, device=x.device)
    nb = _lib.load().cmr_bn_bwd_workspace_bytes(rows, C)
    ws = _ws(nb, x.device)
    _lib.call("cmr_bn_bwd_coef_f32", _p(dz), _ld(dz), _p(z), _ld(z) if z is not None else 0, float(slope), _p(x), _ld(x), _p(stat), _p(coef),
              _p(dgamma), _p(dbeta), rows, C, _p(ws), nb, _stream())
    return coef


def bn_linear_bwd_ok(rows, n, k):
    """shapes cmr_bn_linear_bwd_f32 serves"""
    return n in (64, 128) and k in (64, 128) and rows >= 32 and rows % 32 == 0


def bn_linear_bwd(dz, z, slope, h, stat, coef, x, w, dw, accumulate_dw=False, res=None, dx=None, want_dx=True, want_masked=False,
                  mask_from_h=False, xstat=None, xslope=1.0, xdgamma=None, xdbeta=None, db=None, accumulate_db=False, seg_rows=0):
    """Backward of [h = x' W^T + b -> BatchNorm(train) -> (+ residual) -> LeakyReLU(slope) = z] in one pass over the row maps: with
    (stat, coef) from bn_stats / bn_bwd_coef, dw (+)= dh^T x' and dx = dh W (+ res; dx may be res itself) where
    dh = scale (d - c1 - xhat c2), d = dz * act'(z).  stat = coef = None: no BatchNorm (dh = d); db (+)= column sums of dh.
    mask_from_h: z was never stored (z ignored): act' from the sign of h * stat[2] + stat[3].
    xstat [4, k]: x is the previous layer's BatchNorm input, x' = lrelu_{xslope}(x * xstat[2] + xstat[3]); dx is then the gradient at x'
    and the third result is the previous layer's coef [2, k] (its dgamma / dbeta written into xdgamma / xdbeta).
    seg_rows: the map is seg_rows-row segments (samples); third result = the column sums of dh per segment [rows / seg_rows, n].
    -> (dx or None, d or None: the masked gradient a residual branch receives[, xcoef | segment sums]), or False when the shape is not served."""
    _rows(dz), _rows(x)
    rows, n = dz.shape
    k = x.shape[1]
    if not bn_linear_bwd_ok(rows, n, k) or x.shape[0] != rows or w.shape[0] < n or w.shape[1] != k or w.stride(1) != 1 or dw.stride(1) != 1:
        return False
    if xstat is not None and n != 64:
        return False
    if stat is not None and (h is None or tuple(h.shape) != (rows, n)):
        raise ValueError("bn_linear_bwd: BatchNorm input %s vs gradient %s" % (None if h is None else tuple(h.shape), (rows, n)))
    if xstat is not None and (tuple(xstat.shape) != (4, k) or not want_dx or stat is None):
        raise ValueError("bn_linear_bwd: a lazy operand needs its statistics [4, %d], a BatchNorm layer and the data gradient" % k)
    if want_dx and dx is None:
        dx = torch.empty((rows, k), dtype=f32, device=x.device)
    dzm = torch.empty((rows, n), dtype=f32, device=x.device) if want_masked else None
    xcoef = torch.empty((2, k), dtype=f32, device=x.device) if xstat is not None else None
    if seg_rows and (seg_rows < 128 or seg_rows % 32 or rows % seg_rows):
        return False
    seg_db = torch.empty((rows // seg_rows, n), dtype=f32, device=x.device) if seg_rows else None
    bf = bool(CONV_BF16 and BN_LINEAR_BF16_BWD)
    nb = getattr(_lib.load(), "cmr_bn_linear_bwd_bf16_workspace_bytes" if bf else "cmr_bn_linear_bwd_workspace_bytes")(rows, n, k)
    ws = _ws(nb, x.device)
    zz = None if mask_from_h else z
    _lib.call("cmr_bn_linear_bwd_bf16_f32" if bf else "cmr_bn_linear_bwd_f32", _p(dz), _ld(dz), _p(zz), _ld(zz) if zz is not None else 0, float(slope), _p(h), _ld(h) if h is not None else 0,
              _p(stat), _p(coef), int(bool(mask_from_h)), _p(dzm), n if want_masked else 0, _p(x), _ld(x), _p(xstat), float(xslope), _p(xcoef),
              _p(xdgamma), _p(xdbeta), _p(w), w.stride(0), _p(res), _ld(res) if res is not None else 0,
              _p(dx) if want_dx else None, _ld(dx) if want_dx else 0, rows, n, k, _p(dw), dw.stride(0), int(accumulate_dw), _p(db),
              int(accumulate_db), int(seg_rows), _p(seg_db), _p(ws), nb, _stream())
    if xstat is not None:
        return dx, dzm, xcoef
    if seg_rows:
        return (dx if want_dx else None), dzm, seg_db
    return (dx if want_dx else None), dzm


def vecattn_mix(q, k, v, pos):
    """-> (q - k + pos, v + pos) in one pass (the elementwise glue of a vector-attention layer)."""
    for t in (q, k, v, pos):
        _rows(t)
    rows, C = q.shape
    a_in = torch.empty((rows, C), dtype=f32, device=q.device)
    vp = torch.empty((rows, C), dtype=f32, device=q.device)
    _lib.call("cmr_vecattn_mix_f32", _p(q), _ld(q), _p(k), _ld(k), _p(v), _ld(v), _p(pos), _ld(pos), _p(a_in), _p(vp), rows, C, _stream())
    return a_in, vp


def vecattn_mix_bwd(da, dvp):
    """-> (dk = -da, dpos = da + dvp)."""
    _rows(da), _rows(dvp)
    rows, C = da.shape
    dk = torch.empty((rows, C), dtype=f32, device=da.device)
    dpos = torch.empty((rows, C), dtype=f32, device=da.device)
    _lib.call("cmr_vecattn_mix_bwd_f32", _p(da), _ld(da), _p(dvp), _ld(dvp), _p(dk), _p(dpos), rows, C, _stream())
    return dk, dpos


def act_bwd(dz, z, slope, add=None, out=None):
    _rows(dz), _rows(z)
    rows, C = z.shape
    if out is None:
        out = torch.empty((rows, C), dtype=f32, device=z.device)
    _lib.call("cmr_act_bwd_f32", _p(dz), _ld(dz), _p(z), _ld(z), float(slope), _p(add), _ld(add) if add is not None else 0, _p(out),
              _ld(out), rows, C, _stream())
    return out


def pool_act_bwd(g, d, ph, pw, slope):
    """g [B,H/ph,W/pw,C] (contiguous), d [B,H,W,C] activation output -> gradient w.r.t. the pre-activation [B,H,W,C]."""
    B, H, W, C = d.shape
    if not (g.is_contiguous() and d.is_contiguous()) or g.numel() != B * (H // ph) * (W // pw) * C:
        raise ValueError("pool_act_bwd: bad operand layout")
    out = torch.empty_like(d)
    _lib.call("cmr_pool_act_bwd_f32", _p(g), _p(d), _p(out), B, H, W, C, ph, pw, float(slope), _stream())
    return out


def colsum(x, B, N, out=None):
    _rows(x)
    C = x.shape[1]
    nb = _lib.load().cmr_colarg_workspace_bytes(B, N, C)
    ws = _ws(nb, x.device)
    if out is None:
        out = torch.empty((B, C), dtype=f32, device=x.device)
    _lib.call("cmr_colsum_f32", _p(x), _ld(x), _p(out), _p(ws), nb, B, N, C, _stream())
    return out


def colmax_arg(x, B, N):
    """max and arg-max row over the N consecutive rows of each of the B groups of x [B N, C] -> ([B, C] f32, [B, C] i32 row within the
    group).  The groups ride in gridDim.y (<= 65535): more groups (a train-mode set abstraction with B * npoint >= 65536 centroids,
    pointnet_util.py:190) go in chunks."""
    _rows(x)
    C = x.shape[1]
    out = torch.empty((B, C), dtype=f32, device=x.device)
    arg = torch.empty((B, C), dtype=torch.int32, device=x.device)
    for b0 in range(0, B, GRID_Y_MAX):
        b = min(GRID_Y_MAX, B - b0)
        nb = _lib.load().cmr_colarg_workspace_bytes(b, N, C)
        ws = _ws(nb, x.device)
        xs = x[b0 * N:(b0 + b) * N]
        _lib.call("cmr_colmax_arg_f32", _p(xs), _ld(xs), _p(out[b0:b0 + b]), _p(arg[b0:b0 + b]), _p(ws), nb, b, N, C, _stream())
    return out, arg


def add_at_arg(dx, arg, g, B, N):
    _rows(dx)
    C = g.shape[1]
    _lib.call("cmr_add_at_arg_f32", _p(dx), _ld(dx), _p(_i32(arg)), _p(g), g.stride(0), B, N, C, _stream())
    return dx


def linear_bwd_small(x1, dy, w, ldw, n, y=None, slope=1.0, x2=None, dw=None, lddw=0, db=None, dx1=None, dx2=None, acc_dx=False):
    """Backward of a Linear on <= 1024 rows; w / dw are raw views (pointer + row stride) into the flat buckets."""
    rows, k1 = x1.shape
    k2 = x2.shape[1] if x2 is not None else 0
    _lib.call("cmr_linear_bwd_small_f32", _p(x1), x1.stride(0), k1, _p(x2), x2.stride(0) if x2 is not None else 0, k2, _p(y),
              y.stride(0) if y is not None else 0, float(slope), _p(dy), dy.stride(0), _p(w), int(ldw), _p(dw), int(lddw), _p(db), _p(dx1),
              dx1.stride(0) if dx1 is not None else 0, _p(dx2), dx2.stride(0) if dx2 is not None else 0, int(acc_dx), rows, int(n),
              _stream())


def agent_loss(r_logits, t_logits, value, expert_r, expert_t, act_r, act_t, old_logprob, returns, adv, dr, dt, S, alpha, clip_eps,
               w_value, w_entropy, grad_scale=1.0):
    """-> (losses float32 [8], d_r_logits, d_t_logits, d_value) with the gradient buffers shaped like the (padded) inputs."""
    B = r_logits.shape[0]
    # the padding columns of the gradient buffers must be zero (the kernel writes the logical ones): ONE zeroed allocation for the three
    # (three fills were three nodes on the serial chain of every replayed update)
    if r_logits.is_contiguous() and t_logits.is_contiguous() and value.is_contiguous():
        nr, nt, nv = r_logits.numel(), t_logits.numel(), value.numel()
        z = torch.zeros((nr + nt + nv,), dtype=f32, device=r_logits.device)
        d_r, d_t, d_v = z[:nr].view_as(r_logits), z[nr:nr + nt].view_as(t_logits), z[nr + nt:].view_as(value)
    else:
        d_r, d_t, d_v = torch.zeros_like(r_logits), torch.zeros_like(t_logits), torch.zeros_like(value)
    out = torch.empty((8,), dtype=f32, device=r_logits.device)
    for t in (expert_r, expert_t, act_r, act_t):
        if t.dtype != torch.int64 or not t.is_contiguous():
            raise ValueError("agent_loss: actions must be contiguous int64")
    _lib.call("cmr_agent_loss_f32", _p(r_logits), r_logits.stride(0), _p(t_logits), t_logits.stride(0), _p(value), value.stride(0),
              _p(expert_r), _p(expert_t), _p(act_r), _p(act_t), _p(old_logprob), _p(returns), _p(adv), _p(d_r), d_r.stride(0), _p(d_t),
              d_t.stride(0), _p(d_v), d_v.stride(0), _p(out), B, dr, dt, S, float(alpha), float(clip_eps), float(w_value),
              float(w_entropy), float(grad_scale), _stream())
    return out, d_r, d_t, d_v


def adam(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, grad_clip=0.0):
    _lib.call("cmr_adam_f32", _p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
              float(weight_decay), 1.0 - beta1 ** step, 1.0 - beta2 ** step, float(grad_scale), float(grad_clip), _stream())


def sgd(p, g, buf, lr, momentum, weight_decay, step, grad_scale=1.0, grad_clip=0.0):
    """torch.optim.SGD(momentum, weight_decay) over the flat bucket; step counts from 1."""
    _lib.call("cmr_sgd_f32", _p(p), _p(g), _p(buf), p.numel(), float(lr), float(momentum), float(weight_decay), float(grad_scale),
              float(grad_clip), int(step == 1), _stream())


def transpose_slots(src, dst, table, nslots, total_tiles):
    """dst <- per-slot transposes of the matrix parameters in the flat buffer src (table: FlatBucket.transpose_table)."""
    _lib.call("cmr_transpose_slots_f32", _p(src), _p(dst), _p(table), int(nslots), int(total_tiles), _stream())
    return dst


WGRAD_WINO = os.environ.get("CMR_WGRAD_WINO", "1") != "0"     # fp32 64 -> 64 stride-1 weight gradients in the Winograd domain (cmr_conv3x3_wgrad_wino_f32)
WGRAD_WINO_MIN_PIXELS = 16384                                 # below: too few stages per workgroup to fill the two-buffer pipeline
WGRAD_BF16 = True        # with CONV_BF16: 3x3 weight gradients on the bf16 cores as well (False: fp32 weight gradients, round 2's behaviour)


def conv3x3_wgrad(x, dy, dw, db=None, xpro=None):
    """x [B,H,W,Cin], dy [B,H,W,Cout] (contiguous NHWC) -> dw (flat view of [Cout,Cin,3,3] in the gradient bucket); db [Cout] (optional):
    the bias gradient, from the same launch on the bf16 path, by a column sum over dy otherwise.
    xpro = (scale, shift, slope): x is a BatchNorm input and the operand is lrelu_slope(x * scale + shift) (conv3x3_bn_pro's forward); returns
    False when that form is not served (the caller materialises the activation)."""
    B, H, W, cin = x.shape
    cout = dy.shape[3]
    if not (x.is_contiguous() and dy.is_contiguous()) or dw.numel() != cout * cin * 9:
        raise ValueError("conv3x3_wgrad: bad operand layout")
    nb = _lib.load().cmr_conv3x3_wgrad_workspace_bytes(B, H, W, cin, cout)
    ws = _ws(nb, x.device)
    if xpro is not None:
        if not (CONV_BF16 and WGRAD_BF16 and cin == 128):
            return False
        sc, sh, sl = xpro
        rc = _lib.call("cmr_conv3x3_wgrad_bias_bf16_pro_f32", _p(x), _p(sc), _p(sh), float(sl), _p(dy), B, H, W, cin, cout, _p(dw), _p(db), _p(ws), nb,
                       _stream(), allow_unsupported=True)
        return rc != _lib.UNSUPPORTED
    # bf16 training mode: the weight gradient on the bf16 matrix cores too (operands rounded to bf16, fp32 accumulate), like the forward
    # and data-gradient convolutions
    if CONV_BF16 and WGRAD_BF16 and cin in (64, 128):
        if db is not None and (db.numel() != cout or not db.is_contiguous()):
            raise ValueError("conv3x3_wgrad: db must be a contiguous [Cout] view")
        _lib.call("cmr_conv3x3_wgrad_bias_bf16_f32", _p(x), _p(dy), B, H, W, cin, cout, _p(dw), _p(db), _p(ws), nb, _stream())
        return
    rc = _lib.UNSUPPORTED
    if WGRAD_WINO and cin == 64 and cout == 64 and H % 2 == 0 and W % 2 == 0 and B * H * W >= WGRAD_WINO_MIN_PIXELS:
        # fp32, 64 -> 64: the weight gradient in the Winograd domain (16/36 of the direct sum's multiplies, like the forward)
        nbw = _lib.load().cmr_conv3x3_wgrad_wino_workspace_bytes(B, H, W, cin, cout)
        rc = _lib.call("cmr_conv3x3_wgrad_wino_f32", _p(x), _p(dy), B, H, W, cin, cout, _p(dw), _p(_ws(nbw, x.device)), nbw, _stream(),
                       allow_unsupported=True)
    if rc == _lib.UNSUPPORTED:
        _lib.call("cmr_conv3x3_wgrad_f32", _p(x), _p(dy), B, H, W, cin, cout, _p(dw), _p(ws), nb, _stream())
    if db is not None:
        colsum(dy.view(-1, cout), 1, B * H * W, out=db.view(1, cout))


def conv3x3_wgrad_s2(x, dy, dw):
    """Weight gradient of a stride-2 3x3 convolution: x [B,H,W,Cin], dy [B,H/2,W/2,Cout] (contiguous NHWC) -> dw (flat [Cout,Cin,3,3] view).
    Returns False when the shape is not served (odd sizes; bf16 mode keeps its own path): the caller zero-inserts and uses conv3x3_wgrad."""
    B, H, W, cin = x.shape
    cout = dy.shape[3]
    if H % 2 or W % 2 or W < 4 or tuple(dy.shape[:3]) != (B, H // 2, W // 2) or cin not in (32, 64, 128) or cout not in (32, 64, 128, 256):
        return False
    if (CONV_BF16 and WGRAD_BF16) or not (x.is_contiguous() and dy.is_contiguous()) or dw.numel() != cout * cin * 9:
        return False
    nb = _lib.load().cmr_conv3x3_wgrad_workspace_bytes(B, H // 2, W // 2, cin, cout)
    ws = _ws(nb, x.device)
    _lib.call("cmr_conv3x3_wgrad_s2_f32", _p(x), _p(dy), B, H, W, cin, cout, _p(dw), _p(ws), nb, _stream())
    return True


def linear_wgrad(dy, x, dw, lddw, n=None, k=None, accumulate=False, db=None, accumulate_db=False):
    """dw[n][k] (+)= dy^T x over the rows, db[n] (+)= column sums of dy (optional); dw is a raw view (pointer + row stride)."""
    _rows(dy), _rows(x)
    rows = dy.shape[0]
    n = dy.shape[1] if n is None else n
    k = x.shape[1] if k is None else k
    nb = _lib.load().cmr_linear_wgrad_workspace_bytes(rows, n, k)
    ws = _ws(nb, x.device)
    _lib.call("cmr_linear_wgrad_f32", _p(dy), _ld(dy), n, _p(x), _ld(x), k, rows, _p(dw), int(lddw), int(accumulate), _p(db),
              int(accumulate_db), _p(ws), nb, _stream())


def pack_conv3x3(w, cout, cin, transpose=False, want_u=True):
    """nn.Conv2d weight (flat [Cout,Cin,3,3]) -> (w9 [9,Co',Ci'], U fragments [16,Co',Ci'] or None) for the forward kernels."""
    co, ci = (cin, cout) if transpose else (cout, cin)
    w9 = torch.empty((9, co, ci), dtype=f32, device=w.device)
    u = torch.empty((16, co, ci), dtype=f32, device=w.device) if want_u and co % 32 == 0 and ci % 32 == 0 else None
    bf, nt = None, 1
    if CONV_BF16 and u is not None and ci in (64, 128):          # operands of the bf16 variant, same attribute as _pack.conv9 sets
        nt = 2 if (ci == 64 and co % 64 == 0) else 1
        bf = torch.empty((9 * co * ci,), dtype=torch.bfloat16, device=w.device)
    _lib.call("cmr_pack_conv3x3_f32", _p(w), cout, cin, int(transpose), _p(w9), _p(u), _p(bf), nt, _stream())
    if bf is not None:
        u.bf16 = (bf, nt)
    return w9, u


# ----------------------------------------------------------------------------------------------------------------------
# geometric-model update (Train_Geo.py:166-174): backward pieces -- see include/cmr_hip.h
# ----------------------------------------------------------------------------------------------------------------------
def axpy(y, x, alpha=1.0):
    """y += alpha * x on row maps."""
    _rows(y), _rows(x)
    _lib.call("cmr_axpy_f32", _p(y), _ld(y), _p(x), _ld(x), float(alpha), y.shape[0], y.shape[1], _stream())
    return y


def act(x, kind, param=0.0, out=None):
    _rows(x)
    if out is None:
        out = torch.empty((x.shape[0], x.shape[1]), dtype=f32, device=x.device)
    _lib.call("cmr_act_f32", _p(x), _ld(x), _p(out), _ld(out), x.shape[0], x.shape[1], int(kind), float(param), _stream())
    return out


def act_bwd_x(dy, x, kind, param=0.0, out=None, accumulate=False):
    _rows(dy), _rows(x)
    if out is None:
        out = torch.empty((x.shape[0], x.shape[1]), dtype=f32, device=x.device)
        accumulate = False
    _lib.call("cmr_act_bwd_x_f32", _p(dy), _ld(dy), _p(x), _ld(x), _p(out), _ld(out), x.shape[0], x.shape[1], int(kind), float(param),
              int(accumulate), _stream())
    return out


def layernorm64_bwd(dy, x, gamma, eps, dgamma, dbeta, acc_params, out=None, accumulate=False):
    _rows(dy), _rows(x)
    rows = x.shape[0]
    if out is None:
        out = torch.empty((rows, 64), dtype=f32, device=x.device)
        accumulate = False
    nb = _lib.load().cmr_layernorm64_bwd_workspace_bytes(rows)
    ws = _ws(nb, x.device)
    _lib.call("cmr_layernorm64_bwd_f32", _p(dy), _ld(dy), _p(x), _ld(x), _p(gamma), float(eps), _p(out), _ld(out), int(accumulate),
              _p(dgamma), _p(dbeta), int(acc_params), rows, _p(ws), nb, _stream())
    return out


def l2norm64_bwd(dy, x, out=None, accumulate=False):
    _rows(dy), _rows(x)
    if out is None:
        out = torch.empty((x.shape[0], 64), dtype=f32, device=x.device)
        accumulate = False
    _lib.call("cmr_l2norm64_bwd_f32", _p(dy), _ld(dy), _p(x), _ld(x), _p(out), _ld(out), int(accumulate), x.shape[0], _stream())
    return out


def zero_insert2(g, H, W):
    B, Ho, Wo, C = g.shape
    out = torch.empty((B, H, W, C), dtype=f32, device=g.device)
    _lib.call("cmr_zero_insert2_f32", _p(g), _p(out), B, Ho, Wo, H, W, C, _stream())
    return out


def patchify_bwd(dpatches, B, H, W, C, P, out=None, accumulate=False):
    if out is None:
        out = torch.empty((B, H, W, C), dtype=f32, device=dpatches.device)
        accumulate = False
    _lib.call("cmr_patchify_bwd_f32", _p(dpatches), _p(out), B, H, W, C, P, int(accumulate), _stream())
    return out


def upsample_bwd(dcat, coff, B, H, W, C2, scale, out=None, accumulate=False):
    """dcat: NHWC [B,H,W,Ctot] contiguous; -> d proxy rows [B * (H/s) * (W/s), C2]."""
    ldc = dcat.shape[3]
    if out is None:
        out = torch.empty((B * (H // scale) * (W // scale), C2), dtype=f32, device=dcat.device)
        accumulate = False
    _lib.call("cmr_upsample_bwd_f32", _p(dcat), ldc, coff, _p(out), B, H, W, C2, scale, int(accumulate), _stream())
    return out


def im2col3(x4):
    B, H, W, c = x4.shape
    if c != 4 or not x4.is_contiguous():
        raise ValueError("im2col3 expects a contiguous NHWC tensor with 4 channels (xyz0-style padding)")
    cols = torch.empty((B * H * W, 36), dtype=f32, device=x4.device)
    _lib.call("cmr_im2col3_f32", _p(x4), _p(cols), B, H, W, _stream())
    return cols


def col2im3(dcols, B, H, W, out=None, accumulate=False):
    if out is None:
        out = torch.empty((B, H, W, 4), dtype=f32, device=dcols.device)
        accumulate = False
    _lib.call("cmr_col2im3_f32", _p(dcols), _p(out), B, H, W, int(accumulate), _stream())
    return out


def mha_bwd(q, k, v, o, dout, B, Tq, Tk, dq=None, dk=None, dv=None, acc=(False, False, False)):
    mk = lambda t, r: (torch.empty((r, 64), dtype=f32, device=q.device), False) if t is None else (t, True)
    (dq, aq), (dk, ak), (dv, av) = mk(dq, B * Tq), mk(dk, B * Tk), mk(dv, B * Tk)
    ws = torch.empty((B * Tq * 16,), dtype=f32, device=q.device)
    _lib.call("cmr_mha_bwd_f32", _p(_rows(q)), _ld(q), _p(_rows(k)), _ld(k), _p(_rows(v)), _ld(v), _p(_rows(o)), _ld(o), _p(_rows(dout)),
              _ld(dout), _p(dq), _ld(dq), int(aq and acc[0]), _p(dk), _ld(dk), int(ak and acc[1]), _p(dv), _ld(dv), int(av and acc[2]),
              _p(ws), ws.numel() * 4, B, Tq, Tk, _stream())
    return dq, dk, dv


def la_bwd(qf, kf, v, kvsum, dmsg, B, L, S, eps, dqf=None, dkf=None, dv=None, acc=(False, False, False)):
    mk = lambda t, r: (torch.empty((r, 64), dtype=f32, device=qf.device), False) if t is None else (t, True)
    (dqf, aq), (dkf, ak), (dv, av) = mk(dqf, B * L), mk(dkf, B * S), mk(dv, B * S)
    nb = _lib.load().cmr_la_bwd_workspace_bytes(B, L)
    ws = _ws(nb, qf.device)
    _lib.call("cmr_la_bwd_f32", _p(_rows(qf)), _ld(qf), _p(_rows(kf)), _ld(kf), _p(_rows(v)), _ld(v), _p(kvsum), _p(_rows(dmsg)), _ld(dmsg),
              _p(dqf), _ld(dqf), int(aq and acc[0]), _p(dkf), _ld(dkf), int(ak and acc[1]), _p(dv), _ld(dv), int(av and acc[2]), _p(ws), nb, B,
              L, S, float(eps), _stream())
    return dqf, dkf, dv


def segment_softmax_bwd(attn, vp, dout, nseg, scale, order=None, offsets=None, fixed_len=0, covers_all_rows=False):
    """Backward of segment_softmax -> (d attn, d vp), both [rows, 64].  The kernel writes the rows the segments list; a row listed in no
    segment (csr_build drops keys that point outside their batch element's segments) receives zero gradient.  covers_all_rows: the caller
    vouches that the segments list every row, and the two buffers are not zero-filled first."""
    alloc = torch.empty_like if covers_all_rows else torch.zeros_like
    dattn, dvp = alloc(attn), alloc(vp)
    _lib.call("cmr_segment_softmax_bwd_f32", _p(attn), _p(vp), _p(_i32(order)), _p(_i32(offsets)), fixed_len, float(scale), _p(dout), _p(dattn),
              _p(dvp), nseg, _stream(), work_extra={"_rows": attn.shape[0]})
    return dattn, dvp


def focal_bwd(logits_rows, label_i64, alpha, grad_scale=1.0):
    R = logits_rows.shape[0]
    out = torch.zeros((R, 4), dtype=f32, device=logits_rows.device)
    _lib.call("cmr_focal_bwd_f32", _p(logits_rows), logits_rows.stride(0), _p(label_i64), float(alpha), R, float(grad_scale), _p(out), 4,
              _stream())
    return out


def circle_loss_bwd(pc_feat_rows, img_feat_nhwc, pc_idx, xy_int, xy_float, B, N, d_pc, d_img, dist_thres, pos_margin, neg_margin, log_scale,
                    grad_scale=1.0):
    _, h, w, _ = img_feat_nhwc.shape
    n = pc_idx.shape[1]
    nb = _lib.load().cmr_circle_bwd_workspace_bytes(B, n)
    ws = _ws(nb, pc_feat_rows.device)
    _lib.call("cmr_circle_loss_bwd_f32", _p(_rows(pc_feat_rows)), _p(img_feat_nhwc), _p(pc_idx), _p(xy_int), _p(xy_float), B, N, h, w, n,
              float(dist_thres), float(pos_margin), float(neg_margin), float(log_scale), float(grad_scale), _p(d_pc), _p(d_img), _p(ws), nb,
              _stream())


LINEAR_BWD_ROWS = os.environ.get("CMR_LINEAR_BWD_ROWS", "1") != "0"     # A/B: the one-launch backward of small row-map linears


def linear_bwd_rows(dy, y, slope, x, w, dw, accumulate_dw=False, db=None, accumulate_db=False, res=None, out=None, want_dx=True):
    """One-launch backward of y = act(x W^T + b) on a small row map: dw (+)= dYe^T x, db (+)= colsum(dYe), returns dx = dYe W (+ res)
    (None with want_dx False) -- or False when the shape is not served (caller composes act_bwd / linear_wgrad / linear)."""
    if not LINEAR_BWD_ROWS:
        return False
    _rows(dy), _rows(x)
    rows, n = dy.shape
    k = x.shape[1]
    if tuple(dw.shape) != (n, k) or tuple(w.shape) != (n, k) or x.shape[0] != rows or rows > 4096 or n % 32 or n > 128 or k not in (32, 64, 128):
        return False
    if (y is not None and tuple(y.shape) != (rows, n)) or (res is not None and tuple(res.shape) != (rows, k)) or w.stride(1) != 1 or dw.stride(1) != 1:
        return False
    if want_dx and out is None:
        out = torch.empty((rows, k), dtype=f32, device=x.device)
    rc = _lib.call("cmr_linear_bwd_rows_f32", _p(dy), _ld(dy), _p(y), _ld(y) if y is not None else 0, float(slope), _p(x), _ld(x), _p(w),
                   w.stride(0), rows, n, k, _p(dw), dw.stride(0), int(accumulate_dw), _p(db), int(accumulate_db), _p(res),
                   _ld(res) if res is not None else 0, _p(out) if want_dx else None, _ld(out) if want_dx else 0, _stream(),
                   allow_unsupported=True)
    if rc == _lib.UNSUPPORTED:
        return False
    return out if want_dx else None


def linear_wgrad_any(dy, x, dw, accumulate=False, db=None, accumulate_db=False):
    """dw [n, k] (+)= dy^T x (and db) for any n, k (the MLP of the transformer blocks has n or k = 1024, the patch embedding
    k = 4096): one launch."""
    n, k = dw.shape
    if dy.shape[1] < n or x.shape[1] < k:
        raise ValueError("linear_wgrad_any: operand widths %d / %d vs gradient %s" % (dy.shape[1], x.shape[1], tuple(dw.shape)))
    linear_wgrad(dy, x, dw, dw.stride(0), n=n, k=k, accumulate=accumulate, db=db, accumulate_db=accumulate_db)


# ---- IterModel (models/IterModel.py): the stages around the cost volume's convolutions ----------------------------------------

def iter_sample_poses(r_amp, t_amp, nlabel):
    """-> (delta_r [nlabel], delta_t [nlabel], rt [nlabel^3, 3, 4]: rows 0..2 of the inverse sampled poses)."""
    dev = r_amp.device
    dr, dt = torch.empty(nlabel, dtype=f32, device=dev), torch.empty(nlabel, dtype=f32, device=dev)
    rt = torch.empty((nlabel ** 3, 3, 4), dtype=f32, device=dev)
    _lib.call("cmr_iter_sample_poses_f32", _p(r_amp), _p(t_amp), int(nlabel), _p(dr), _p(dt), _p(rt), _stream())
    return dr, dt, rt


def iter_warp_scatter(pc_3n, feat_rows, score, mask_u8, standby_u8, rt, K, h, w):
    """-> (acc [P, h, w, 64] feature sums, cnt [P, h, w], occ [P, h, w], sel [N] the point mask in use)."""
    N, P = pc_3n.shape[1], rt.shape[0]
    if tuple(pc_3n.shape) != (3, N) or tuple(feat_rows.shape) != (N, 64) or not (pc_3n.is_contiguous() and feat_rows.is_contiguous()):
        raise ValueError("iter_warp_scatter: pc [3, N] planar and feat [N, 64] rows, contiguous")
    if score.numel() != N or mask_u8.numel() != N or standby_u8.numel() != N or mask_u8.dtype != torch.uint8 or standby_u8.dtype != torch.uint8:
        raise ValueError("iter_warp_scatter: score [N] float32, masks [N] uint8")
    dev = pc_3n.device
    acc = torch.empty((P, h, w, 64), dtype=f32, device=dev)
    cnt, occ = torch.empty((P, h, w), dtype=f32, device=dev), torch.empty((P, h, w), dtype=f32, device=dev)
    sel = torch.empty(N, dtype=torch.uint8, device=dev)
    _lib.call("cmr_iter_warp_scatter_f32", _p(pc_3n), _p(feat_rows), _p(score), _p(mask_u8), _p(standby_u8), _p(sel), _p(rt), _p(K),
              _p(acc), _p(cnt), _p(occ), N, P, h, w, _stream())
    return acc, cnt, occ, sel


ITER_BAND_CELLS = 384      # IB_CELLS of csrc/iter_model.hip: the band kernel holds whole map rows of at most this many cells


def iter_warp_bin(pc_3n, feat_rows, score, mask_u8, standby_u8, rt, K, w_occ, base, h, w):
    """-> (warped [P, h, w, 64] scatter mean, res [P, h, w, 64] = base + 3x3 stencil of the occupancy plane, occ [P, h, w], sel [N])."""
    N, P = pc_3n.shape[1], rt.shape[0]
    if tuple(pc_3n.shape) != (3, N) or tuple(feat_rows.shape) != (N, 64) or not (pc_3n.is_contiguous() and feat_rows.is_contiguous()):
        raise ValueError("iter_warp_bin: pc [3, N] planar and feat [N, 64] rows, contiguous")
    if score.numel() != N or mask_u8.numel() != N or standby_u8.numel() != N or mask_u8.dtype != torch.uint8 or standby_u8.dtype != torch.uint8:
        raise ValueError("iter_warp_bin: score [N] float32, masks [N] uint8")
    if tuple(base.shape) != (h, w, 64) or tuple(w_occ.shape) != (9, 64) or w > ITER_BAND_CELLS:
        raise ValueError("iter_warp_bin: base [h, w, 64], w_occ [9, 64], w <= 384")
    dev = pc_3n.device
    warped = torch.empty((P, h, w, 64), dtype=f32, device=dev)
    res = torch.empty((P, h, w, 64), dtype=f32, device=dev)
    occ = torch.empty((P, h, w), dtype=f32, device=dev)
    sel = torch.empty(N, dtype=torch.uint8, device=dev)
    _lib.call("cmr_iter_warp_bin_f32", _p(pc_3n), _p(feat_rows), _p(score), _p(mask_u8), _p(standby_u8), _p(sel), _p(rt), _p(K), _p(w_occ),
              _p(base), _p(warped), _p(res), _p(occ), N, P, h, w, _stream())
    return warped, res, occ, sel


def iter_finalize(acc, cnt, plane, w1, base):
    """res [P, h, w, 64] = base [h, w, 64] + conv3x3(plane [P, h, w], w1 [9, 64]); acc (if given) becomes the scatter mean in place."""
    P, h, w = plane.shape
    res = torch.empty((P, h, w, 64), dtype=f32, device=plane.device)
    _lib.call("cmr_iter_finalize_f32", _p(acc), _p(cnt), _p(plane), _p(w1), _p(base), _p(res), P, h, w, _stream())
    return res


def iter_head(x, w24, b24, w26, b26, slope):
    """x [P, hh, ww, C >= 8] -> logits [P]: global average of channels 0..7, 8 -> 4, LeakyReLU, 4 -> 1."""
    P, hh, ww, C = x.shape
    logits = torch.empty(P, dtype=f32, device=x.device)
    _lib.call("cmr_iter_head_f32", _p(x), C, hh * ww, _p(w24), _p(b24), _p(w26), _p(b26), float(slope), _p(logits), P, _stream())
    return logits


def iter_decide(logits, nlabel, label_r, label_tx, label_tz, delta_r, delta_t):
    """-> (label [P], out_f [4] = (loss, ry, tx, tz), out_i [5] = (label, i_ry, i_tx, i_tz, i_joint), matrix_i [4, 4])."""
    dev = logits.device
    label = torch.empty(nlabel ** 3, dtype=f32, device=dev)
    out_f, out_i = torch.empty(4, dtype=f32, device=dev), torch.empty(5, dtype=torch.int64, device=dev)
    m = torch.empty((4, 4), dtype=f32, device=dev)
    _lib.call("cmr_iter_decide_f32", _p(logits), int(nlabel), _p(label_r), _p(label_tx), _p(label_tz), _p(delta_r), _p(delta_t), _p(label),
              _p(out_f), _p(out_i), _p(m), _stream())
    return label, out_f, out_i, m


def iter_apply(matrix_i, pc_3n, matrix_acc):
    """-> (matrix_i[0:3, 0:3] pc + matrix_i[0:3, 3] as [3, N], matrix_i @ matrix_acc)."""
    N = pc_3n.shape[1]
    pc_out, acc_out = torch.empty_like(pc_3n), torch.empty((4, 4), dtype=f32, device=pc_3n.device)
    _lib.call("cmr_iter_apply_f32", _p(matrix_i), _p(pc_3n), _p(pc_out), N, _p(matrix_acc), _p(acc_out), _stream())
    return pc_out, acc_out


# ---- dropout (train mode; include/cmr_hip.h) ---------------------------------------------------------------------------------------

def dropout(x, p, seed, site, out=None):
    """y = x * keep / (1 - p) with the counter-based mask of (seed[0], site); seed: int64 device tensor [1].  The backward pass is the same
    call on the gradient.  out may be x (in place)."""
    _rows(x)
    if seed.dtype != torch.int64 or not seed.is_cuda:
        raise ValueError("dropout: seed must be an int64 device tensor")
    if out is None:
        out = torch.empty((x.shape[0], x.shape[1]), dtype=f32, device=x.device)
    _lib.call("cmr_dropout_f32", _p(x), _ld(x), _p(_rows(out)), _ld(out), x.shape[0], x.shape[1], float(p), _p(seed), int(site), _stream())
    return out


def mha_dropout(q, k, v, B, Tq, Tk, p, seed, site):
    """softmax attention with dropout on the probabilities (train mode)."""
    out = torch.empty((B * Tq, 64), dtype=f32, device=q.device)
    _lib.call("cmr_mha_dropout_f32", _p(_rows(q)), _ld(q), _p(_rows(k)), _ld(k), _p(_rows(v)), _ld(v), _p(out), _ld(out), B, Tq, Tk, float(p),
              _p(seed), int(site), _stream())
    return out


def mha_dropout_bwd(q, k, v, o, dout, B, Tq, Tk, p, seed, site, dq=None, dk=None, dv=None):
    """dq / dk / dv: optional row views to write into (e.g. the column blocks of one [rows, 192] buffer)."""
    mk = lambda t, r: torch.empty((r, 64), dtype=f32, device=q.device) if t is None else _rows(t)
    dq, dk, dv = mk(dq, B * Tq), mk(dk, B * Tk), mk(dv, B * Tk)
    ws = torch.empty((B * Tq * 16,), dtype=f32, device=q.device)
    _lib.call("cmr_mha_dropout_bwd_f32", _p(_rows(q)), _ld(q), _p(_rows(k)), _ld(k), _p(_rows(v)), _ld(v), _p(_rows(o)), _ld(o), _p(_rows(dout)),
              _ld(dout), _p(dq), _ld(dq), 0, _p(dk), _ld(dk), 0, _p(dv), _ld(dv), 0, _p(ws), ws.numel() * 4, B, Tq, Tk, float(p), _p(seed),
              int(site), _stream())
    return dq, dk, dv


# ---- train-mode transformer block in fused launches (csrc/vit_train.hip, csrc/wgrad_group.hip; include/cmr_hip.h) --------------------

def pack_frags(src, dst, table, nslots, max_elements):
    """dst <- MFMA-fragment-ordered copies of matrix slots of the flat parameter buffer src (table: train/fragpack.py)."""
    _lib.call("cmr_pack_frags_f32", _p(src), _p(dst), _p(table), int(nslots), int(max_elements), _stream(), work_extra={"_elems": dst.numel()})
    return dst


def _drop_args(p_proj, p_mlp, seed, sites):
    if seed is None:
        return 0.0, 0.0, None, 0, 0, 0
    if seed.dtype != torch.int64 or not seed.is_cuda:
        raise ValueError("dropout seed must be an int64 device tensor")
    return float(p_proj), float(p_mlp), seed.data_ptr(), int(sites[0]), int(sites[1]), int(sites[2])


def vit_out_ffn16_train(ctx, x, wo_f16, bo, ln, eps, w1_f16, b1, w2_f16, b2, p_proj=0.0, p_mlp=0.0, seed=None, sites=(0, 0, 0)):
    """Train-mode tail of a transformer block -> (out, x1); sites = dropout site numbers (proj, act, fc2)."""
    rows = x.shape[0]
    out = torch.empty((rows, 64), dtype=f32, device=x.device)
    x1 = torch.empty((rows, 64), dtype=f32, device=x.device)
    pp, pm, sp, s0, s1, s2 = _drop_args(p_proj, p_mlp, seed, sites)
    _lib.call("cmr_vit_out_ffn16_train_f32", _p(_rows(ctx)), _ld(ctx), _p(_rows(x)), _ld(x), _p(wo_f16), _p(bo), _p(ln[0]), _p(ln[1]), float(eps),
              _p(w1_f16), _p(b1), _p(w2_f16), _p(b2), _p(out), _ld(out), _p(x1), _ld(x1), rows, pp, pm, sp, s0, s1, s2, _stream())
    return out, x1


def vit_ffn_bwd16(dout, x1, ln, eps, w1_f16, b1, w2t_f16, w1t_f16, wot_f16, p_proj=0.0, p_mlp=0.0, seed=None, sites=(0, 0, 0)):
    """Backward of vit_out_ffn16_train from d out -> dict(dx1, dctx, gs, du, h, dm, da, lnpart)."""
    rows, dev = x1.shape[0], x1.device
    mk = lambda c: torch.empty(((rows + 15) // 16 * 16, c), dtype=f32, device=dev)[:rows]      # whole 16-row tiles: the kernel stores unpredicated
    r = dict(dx1=mk(64), dctx=mk(64), gs=mk(1024), du=mk(1024), h=mk(64), dm=mk(64), da=mk(64),
             lnpart=torch.empty(((rows + 15) // 16, 128), dtype=f32, device=dev))
    pp, pm, sp, s0, s1, s2 = _drop_args(p_proj, p_mlp, seed, sites)
    _lib.call("cmr_vit_ffn_bwd16_f32", _p(_rows(dout)), _ld(dout), _p(_rows(x1)), _ld(x1), _p(ln[0]), _p(ln[1]), float(eps), _p(w1_f16), _p(b1),
              _p(w2t_f16), _p(w1t_f16), _p(wot_f16), _p(r["dx1"]), 64, _p(r["dctx"]), 64, _p(r["gs"]), _p(r["du"]), _p(r["h"]), _p(r["dm"]),
              _p(r["da"]), _p(r["lnpart"]), rows, pp, pm, sp, s0, s1, s2, _stream())
    return r


def vit_lnqkv_bwd(d_x, wt_f_x, x, res, gamma, beta, eps, d_y=None, wt_f_y=None, y=None):
    """Backward of LayerNorm + q / k / v projections -> (dx, xn, dy, yn, lnpart); d_x [rows_x, 64 | 192], d_y [rows_y, 128] (cross block)."""
    dev = x.device
    rx = x.shape[0]
    dx, xn = torch.empty((rx, 64), dtype=f32, device=dev), torch.empty((rx, 64), dtype=f32, device=dev)
    tiles = (rx + 31) // 32
    dy = yn = None
    ry = 0
    if d_y is not None:
        ry = y.shape[0]
        dy, yn = torch.empty((ry, 64), dtype=f32, device=dev), torch.empty((ry, 64), dtype=f32, device=dev)
        tiles += (ry + 31) // 32
    lnpart = torch.empty((tiles, 128), dtype=f32, device=dev)
    _lib.call("cmr_vit_lnqkv_bwd_f32", _p(_rows(d_x)), _ld(d_x), d_x.shape[1], _p(wt_f_x), _p(_rows(x)), _ld(x), _p(res), _ld(res) if res is not None else 0,
              _p(dx), 64, _p(xn), 64, rx, _p(d_y), _ld(d_y) if d_y is not None else 0, d_y.shape[1] if d_y is not None else 0, _p(wt_f_y),
              _p(y), _ld(y) if y is not None else 0, _p(dy), 64, _p(yn), 64, ry, _p(gamma), _p(beta), float(eps), _p(lnpart), _stream())
    return dx, xn, dy, yn, lnpart


def wgrad_group(problems, vectors=()):
    """problems: [(dy, x, dw, accumulate, db | None, accumulate_db)] with dy [rows, n], x [rows, k] row views and dw [n, k] / db [n] views of
    the gradient bucket; vectors: [(part [nparts, 2 len], out_a [len], out_b [len], accumulate)].  One call, two kernels."""
    import numpy as np
    if not 0 < len(problems) + len(vectors) or len(problems) > 8 or len(vectors) > 4:
        raise ValueError("wgrad_group: at most 8 problems and 4 vector jobs per call")
    desc = []
    for dy, x, dw, acc, db, accb in problems:
        _rows(dy), _rows(x)
        n, k = dw.shape
        if dy.shape[0] != x.shape[0] or dy.shape[1] < n or x.shape[1] < k or dw.stride(1) != 1:
            raise ValueError("wgrad_group: operand shapes %s / %s vs gradient %s" % (tuple(dy.shape), tuple(x.shape), tuple(dw.shape)))
        desc += [dy.data_ptr(), _ld(dy), n, x.data_ptr(), _ld(x), k, dy.shape[0], dw.data_ptr(), dw.stride(0), int(bool(acc)),
                 db.data_ptr() if db is not None else 0, int(bool(accb))]
    for part, oa, ob, acc in vectors:
        if part.dim() != 2 or not part.is_contiguous() or part.shape[1] != 2 * oa.numel() or ob.numel() != oa.numel():
            raise ValueError("wgrad_group: vector job wants part [nparts, 2 len]")
        desc += [part.data_ptr(), part.shape[0], oa.numel(), oa.data_ptr(), ob.data_ptr(), int(bool(acc))]
    d = np.asarray(desc, dtype=np.int64)
    nb = _lib.load().cmr_wgrad_group_workspace_bytes(d.ctypes.data, len(problems), len(vectors))
    if nb < 0:
        raise ValueError("wgrad_group: bad descriptor")
    dev = (problems[0][0] if problems else vectors[0][0]).device
    ws = _ws(nb, dev)
    _lib.call("cmr_wgrad_group_f32", d.ctypes.data, len(problems), len(vectors), _p(ws), nb, _stream(),
              work_extra={"_group": [(dy.shape[0], dw.shape[0], dw.shape[1]) for dy, _, dw, _, _, _ in problems]})


# ---- train-mode linear-attention layer in fused launches (csrc/la_fused.hip train instances, csrc/la_train.hip) -------------------------

def _tile_rows(rows, C, dev):
    """[rows, C] view of a buffer that holds whole 32-row tiles (the row kernels store unpredicated)."""
    return torch.empty(((rows + 31) // 32 * 32, C), dtype=f32, device=dev)[:rows]


def la_kv_state_train(y, wk, wv, B, S):
    """k / v projections + per-(batch, head) state, keeping kf = elu(Wk y) + 1 and v = Wv y -> (kvsum [B, 576], kf, v [B*S, 64])."""
    ws_bytes = _lib.load().cmr_la_kv_state_workspace_bytes(B, S)
    ws = torch.empty((ws_bytes // 4,), dtype=f32, device=y.device)
    kvsum = torch.empty((B, 576), dtype=f32, device=y.device)
    kf, v = torch.empty((B * S, 64), dtype=f32, device=y.device), torch.empty((B * S, 64), dtype=f32, device=y.device)
    _lib.call("cmr_la_kv_state_train_f32", _p(_rows(y)), _ld(y), _p(wk), _p(wv), _p(kvsum), _p(kf), _p(v), _p(ws), ws_bytes, B, S, _stream())
    return kvsum, kf, v


def la_query_layer_train(x, kvsum, wq, wmerge, ln1, w0, w3, ln2, B, L, S, eps, ln_eps, p=0.0, seed=None, sites=(0, 0, 0)):
    """Train-mode query side of a linear-attention layer -> (out, saved dict qf / msg / mm / d1 / hid / o), or None when not served."""
    rows, dev = B * L, x.device
    out = torch.empty((rows, 64), dtype=f32, device=dev)
    sv = {k: _tile_rows(rows, 128 if k == "hid" else 64, dev) for k in ("qf", "msg", "mm", "d1", "hid", "o")}
    sp = seed.data_ptr() if (seed is not None and p > 0.0) else None
    rc = _lib.call("cmr_la_query_layer_train_f32", _p(_rows(x)), _ld(x), _p(kvsum), _p(wq), _p(wmerge), _p(ln1[0]), _p(ln1[1]), _p(w0), _p(w3),
                   _p(ln2[0]), _p(ln2[1]), _p(out), _ld(out), _p(sv["qf"]), _p(sv["msg"]), _p(sv["mm"]), _p(sv["d1"]), _p(sv["hid"]), _p(sv["o"]),
                   B, L, S, float(eps), float(ln_eps), float(p), sp, int(sites[0]), int(sites[1]), int(sites[2]), _stream(), allow_unsupported=True)
    return None if rc == _lib.UNSUPPORTED else (out, sv)


def la_mlp_bwd(dout, sv, wmerge, w0, w3, g1, g2, ln_eps, p=0.0, seed=None, sites=(0, 0, 0)):
    """Backward of the MLP half of the query side -> dict d_o, d_hid, d_mm, d_msg, d_xa, lnpart1, lnpart2."""
    rows, dev = sv["o"].shape[0], dout.device
    r = {k: _tile_rows(rows, 128 if k == "d_hid" else 64, dev) for k in ("d_o", "d_hid", "d_mm", "d_msg", "d_xa")}
    nt = min(256, ((rows + 31) // 32 + 7) // 8)                  # one partial row per workgroup of the kernel's grid
    r["lnpart1"], r["lnpart2"] = torch.empty((nt, 128), dtype=f32, device=dev), torch.empty((nt, 128), dtype=f32, device=dev)
    sp = seed.data_ptr() if (seed is not None and p > 0.0) else None
    _lib.call("cmr_la_mlp_bwd_f32", _p(_rows(dout)), _ld(dout), _p(sv["o"]), _p(sv["hid"]), _p(sv["mm"]), _p(wmerge), _p(w0), _p(w3), _p(g1), _p(g2),
              _p(r["d_o"]), _p(r["d_hid"]), _p(r["d_mm"]), _p(r["d_msg"]), _p(r["d_xa"]), _p(r["lnpart1"]), _p(r["lnpart2"]), rows, float(ln_eps),
              float(p), sp, int(sites[0]), int(sites[1]), int(sites[2]), _stream())
    return r


def la_proj_bwd(problems):
    """problems: 1 or 2 of dict(rows, dx, terms=[(d, f | None, wt_f, e_out | None)], res=[row maps]) -- see cmr_la_proj_bwd_f32."""
    import numpy as np
    desc = []
    for pr in problems:
        res = list(pr.get("res", ())) + [None, None]
        dx = pr["dx"]
        d = [pr["rows"], len(pr["terms"]), dx.data_ptr(), _ld(dx), _p(res[0]) or 0, _ld(res[0]) if res[0] is not None else 0, _p(res[1]) or 0,
             _ld(res[1]) if res[1] is not None else 0]
        for dd, f, wt, eo in list(pr["terms"]) + [(None, None, None, None)] * (3 - len(pr["terms"])):
            d += [0, 0, 0, 0, 0] if dd is None else [_rows(dd).data_ptr(), _ld(dd), _p(f) or 0, wt.data_ptr(), _p(eo) or 0]
        desc += d
    arr = np.asarray(desc, dtype=np.int64)
    _lib.call("cmr_la_proj_bwd_f32", arr.ctypes.data, len(problems), _stream(), work_extra={"_rows": sum(pr["rows"] * len(pr["terms"]) for pr in problems)})


# ---- raw scan -> prepared cloud (csrc/cloud_prepare.hip) ----------------------------------------------------------------------
CLOUD_CELL_LIMIT = 1 << 21          # cells per axis a grid key holds (cz << 42 | cy << 21 | cx)
CLOUD_MAX_ROWS = (1 << 31) - 1      # the CSR of cmr_segment_reduce_f32 is int32


class VoxelCloud(collections.namedtuple("VoxelCloud", "points attr count inverse dropped origin")):
    """voxel_downsample's result: points [n, 3], attr [n, C] (None without attr), count int32 [n], inverse int64 [N] (None unless asked
    for), dropped = the number of input rows with a non-finite coordinate, origin = the grid's origin as three python floats (fp32 values)."""


class PointNormals(collections.namedtuple("PointNormals", "normals count eigenvalues")):
    """point_normals' result: normals [n, 3], count int32 [n] (neighbours within the radius, the row itself included), eigenvalues [n, 3]
    ascending (None unless asked for)."""


def _cloud_scalar(value, name):
    value = float(value)
    with np.errstate(over="ignore", under="ignore"):
        v32 = float(np.float32(value))
    if not (0.0 < value < float("inf")) or not (0.0 < v32 < float("inf")):
        raise ValueError("%s must be a finite number > 0 (in float32 too), got %r" % (name, value))
    return value


def _cloud_points(points, name="points"):
    if not isinstance(points, torch.Tensor) or points.dtype != f32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("%s must be a float32 [N, 3] tensor, got %s %s" % (name, getattr(points, "dtype", type(points)), tuple(getattr(points, "shape", ()))))
    if points.shape[0] > CLOUD_MAX_ROWS:
        raise ValueError("%s holds %d rows; at most 2^31 - 1 (int32 row ids)" % (name, points.shape[0]))
    if not points.is_cuda:
        raise ValueError("%s must be a device tensor (there is no CPU path)" % name)
    return points.contiguous()


def _cloud_triple(value, name):
    try:
        value = [float(v) for v in value]
    except TypeError:
        raise ValueError("%s must be three numbers" % name)
    with np.errstate(over="ignore"):
        finite = [math.isfinite(float(np.float32(v))) for v in value]
    if len(value) != 3 or not all(finite):
        raise ValueError("%s must be three finite numbers, got %r" % (name, value))
    return value


def _cloud_bounds(points):
    """-> (float32 minimum [3], float32 maximum [3], kept) of the rows with finite coordinates: one host read."""
    N, dev = points.shape[0], points.device
    out = torch.empty((8,), dtype=f32, device=dev)            # six floats and, in the last two words, the int64 count: one read-back
    nb = _lib.load().cmr_cloud_bounds_workspace_bytes(N)
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
    _lib.call("cmr_cloud_bounds_f32", _p(points), 3, N, _p(out), _p(out) + 24, _p(ws), nb, _stream())
    b = out.cpu().numpy()
    return b[0:3].copy(), b[3:6].copy(), int(b[6:8].view(np.int64)[0])


def _cloud_grid(points, cell, who, origin=lambda lo: lo):
    """The prologue of every grid over one cloud: the bounds of its rows with finite coordinates (one host read; none without rows), the grid's
    origin = origin(their float32 minimum), the check that the keys fit, the keys and their stable sort.  -> (origin, kept, keys int64 [N]
    sorted, order int64 [N]); (None, 0, None, None) and no further launch without a finite row."""
    N = points.shape[0]
    lo, hi, kept = _cloud_bounds(points) if N else (None, None, 0)
    if kept == 0:
        return None, 0, None, None
    org = origin(lo)
    with np.errstate(over="ignore", invalid="ignore"):        # the largest cell index per axis in the kernel's fp32 arithmetic: monotone in x
        top = np.floor((hi.astype(np.float32) - org) / np.float32(cell))
    if not np.all(np.isfinite(top)) or top.max() >= CLOUD_CELL_LIMIT:
        raise ValueError("%s: the cloud spans %s cells of %g on some axis; a grid key holds at most 2^21 = %d per axis"
                         % (who, "%.0f" % np.nanmax(top + 1) if np.any(np.isfinite(top)) else "too many", cell, CLOUD_CELL_LIMIT))
    keys = torch.empty((N,), dtype=torch.int64, device=points.device)
    _lib.call("cmr_voxel_keys_f32", _p(points), 3, N, float(org[0]), float(org[1]), float(org[2]), float(cell), _p(keys), _stream())
    return (org, kept) + tuple(torch.sort(keys, stable=True))       # the one torch computation of this path: plumbing, like the allocator


def _voxel_means(keys, order, n, kept, points, attr, want_inverse=False):
    """The last `kept` of n sorted keys -> (runs S: one host read, offsets, means of points, of attr or None, count [kept], inverse or None)."""
    dev = keys.device
    order32 = torch.empty((kept,), dtype=torch.int32, device=dev)
    offsets = torch.empty((kept + 1,), dtype=torch.int32, device=dev)
    count = torch.empty((kept,), dtype=torch.int32, device=dev)
    inverse = torch.empty((n,), dtype=torch.int64, device=dev) if want_inverse else None
    nseg = torch.empty((1,), dtype=torch.int64, device=dev)
    nb = _lib.load().cmr_segment_heads_workspace_bytes(n)
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
    _lib.call("cmr_segment_heads_i64", _p(keys), _p(order), n, kept, _p(order32), _p(offsets), _p(count), _p(inverse), _p(nseg), _p(ws), nb, _stream())
    S = int(nseg.item())
    offsets = offsets[:S + 1]
    means = segment_reduce(points, order32, offsets, S, "mean")
    return S, offsets, means, segment_reduce(attr, order32, offsets, S, "mean") if attr is not None and attr.shape[1] else None, count, inverse


def voxel_downsample(points, attr=None, voxel=0.1, origin=None, want_inverse=False):
    """Voxel-grid downsample of one cloud (_cloud_grid's keys, _voxel_means' heads and cmr_segment_reduce_f32; the contract is the
    header's): one output row per occupied voxel in ascending key order, the fp32 mean of the voxel's rows summed in ascending input index.
    points float32 [N, 3], attr float32 [N, C] (C >= 0) or None -> VoxelCloud.  Rows with a non-finite coordinate are dropped.  The number
    of voxels is read back by the host: not capturable in a graph."""
    voxel = _cloud_scalar(voxel, "voxel")
    if origin is not None:
        origin = _cloud_triple(origin, "origin")
    if attr is not None:
        if not isinstance(attr, torch.Tensor) or attr.dtype != f32 or attr.dim() != 2:
            raise ValueError("attr must be a float32 [N, C] tensor or None")
        if isinstance(points, torch.Tensor) and points.dim() == 2 and attr.shape[0] != points.shape[0]:
            raise ValueError("attr has %d rows, points %d" % (attr.shape[0], points.shape[0]))
    points = _cloud_points(points)
    if attr is not None:
        if attr.device != points.device:
            raise ValueError("attr must be on the device of points")
        attr = attr.contiguous()
    N, dev = points.shape[0], points.device
    C = 0 if attr is None else attr.shape[1]

    def result(n, pts, att, cnt, inv, dropped, org):
        return VoxelCloud(pts, att if attr is not None else None, cnt, inv if want_inverse else None, dropped, tuple(float(v) for v in org))

    def grid_origin(lo):
        v32 = np.float32(voxel)
        org = np.asarray(origin, dtype=np.float32) if origin is not None else lo - v32 * np.float32(0.5)
        if not np.all(np.isfinite(org)):
            raise ValueError("voxel_downsample: the grid origin %r is not finite in float32" % (org,))
        if np.any(np.floor((lo - org) / v32) < 0):
            raise ValueError("voxel_downsample: origin %r lies above the cloud's minimum %r on some axis (cell indices start at 0)" % (org, lo))
        return org

    org, kept, keys, order = _cloud_grid(points, voxel, "voxel_downsample", grid_origin)
    if kept == 0:
        return result(0, torch.empty((0, 3), dtype=f32, device=dev), torch.empty((0, C), dtype=f32, device=dev),
                      torch.empty((0,), dtype=torch.int32, device=dev), torch.full((N,), -1, dtype=torch.int64, device=dev), N,
                      origin if origin is not None else (0.0, 0.0, 0.0))
    n, _, out, att, count, inverse = _voxel_means(keys, order, N, kept, points, attr, want_inverse)
    return result(n, out, att if C else torch.empty((n, C), dtype=f32, device=dev), count[:n], inverse, N - kept, org)


def point_normals(points, radius=0.6, viewpoint=(0, 0, 0), min_neighbors=3, want_eigenvalues=False):
    """Surface normals of one cloud from the neighbours within `radius` (cmr_point_normals_f32; the contract is the header's): the
    eigenvector of the smallest eigenvalue of the neighbourhood's covariance, turned towards `viewpoint`; the zero vector where a row has
    fewer than max(3, min_neighbors) neighbours (itself included) or a non-finite coordinate.  points float32 [n, 3] in any order ->
    PointNormals, in the input's order.  No cap on the number of neighbours (Open3D's hybrid search has max_nn)."""
    radius = _cloud_scalar(radius, "radius")
    viewpoint = _cloud_triple(viewpoint, "viewpoint")
    min_neighbors = int(min_neighbors)
    points = _cloud_points(points)
    N, dev = points.shape[0], points.device
    normals = torch.zeros((N, 3), dtype=f32, device=dev)
    count = torch.zeros((N,), dtype=torch.int32, device=dev)
    eig = torch.zeros((N, 3), dtype=f32, device=dev) if want_eigenvalues else None
    lo, kept, keys, order = _cloud_grid(points, radius, "point_normals")
    if kept == 0:
        return PointNormals(normals, count, eig)
    pts4 = torch.empty((N, 4), dtype=f32, device=dev)
    _lib.call("cmr_point_normals_f32", _p(points), 3, _p(keys), _p(order), N, kept, float(lo[0]), float(lo[1]), float(lo[2]), radius,
              viewpoint[0], viewpoint[1], viewpoint[2], min(max(min_neighbors, 3), CLOUD_MAX_ROWS), _p(pts4), _p(normals), _p(count), _p(eig),
              _stream())
    return PointNormals(normals, count, eig)


# ---- cloud against cloud: nearest row and point-to-plane ICP on a grid index (csrc/cloud_icp.hip) ---------------------------
ICP_MAX_ITERS = 1000
ICP_STATUS = ("converged", "iterations exhausted", "fewer than 6 pairs", "singular or non-finite system")


class CloudIndex(collections.namedtuple("CloudIndex", "pts4 keys order origin cell kept n")):
    """cloud_index's result, the grid index of one cloud: pts4 float32 [kept, 4] = the rows with finite coordinates in key order, keys int64
    [n] sorted, order int64 [n] = the row each key came from, origin = the grid's origin (three python floats holding fp32 values), cell,
    kept, n = the cloud's rows.  Built once, read by every cloud_nearest / icp_point_to_plane call on that cloud."""


class CloudNearest(collections.namedtuple("CloudNearest", "idx dist2")):
    """cloud_nearest's result: idx int32 [M] = the nearest target row in the target's own order (-1: none within max_dist), dist2 float32
    [M] = its squared distance (NaN where idx is -1)."""


class IcpResult(collections.namedtuple("IcpResult", "pose pairs rmse iterations status trace system")):
    """icp_point_to_plane's result: pose float32 [4, 4] on the device; pairs and rmse of the last executed iteration (those of the pose it
    started from); iterations executed; status 0 .. 3 (ICP_STATUS); trace float64 [iters, 4] = pairs, rmse, |omega|, |v| per iteration (host);
    system float64 [iters, 28] = H upper, g, cost per iteration (host; None unless asked for)."""


def _cloud_index_arg(index, reach, who, name="max_dist", why="a match must lie in the query's cell or one next to it"):
    if not isinstance(index, CloudIndex):
        raise ValueError("%s: index must be a CloudIndex (ops.cloud_index), got %s" % (who, type(index).__name__))
    if reach is None:
        return index.cell
    reach = _cloud_scalar(reach, name)
    if np.float32(reach) > np.float32(index.cell):
        raise ValueError("%s: %s %g exceeds the index's cell %g (%s)" % (who, name, reach, index.cell, why))
    return reach


def _cloud_family(who, dev, index, one_device, rows=None):
    """rows = (words, first or None, name, second): one row each per row of the index's cloud -> that number; all of them on dev.  Else ValueError."""
    words, first, name, second = rows or ("", None, "", None)
    n = index.n if index is not None else first.shape[0]
    if rows and (second.shape[0] != n or (first is not None and first.shape[0] != n)):
        raise ValueError("%s: %s %d rows, %s %d%s" % (who, words, first.shape[0] if first is not None else n, name, second.shape[0],
                                                    "" if index is None else ", the index %d" % n))
    if any(t is not None and t.device != dev for t in (first, second)) or (index is not None and index.pts4.device != dev):
        raise ValueError("%s: %s" % (who, one_device))
    return n


def _none_found(M, dev):
    return torch.full((M,), -1, dtype=torch.int32, device=dev), torch.full((M,), float("nan"), dtype=f32, device=dev)


def _cloud_pose(pose, dev, who):
    if pose is None:
        return None
    if not isinstance(pose, torch.Tensor) or pose.dtype != f32 or tuple(pose.shape) != (4, 4):
        raise ValueError("%s: pose must be a float32 [4, 4] tensor or None, got %s %s" % ((who,) + _got(pose)))
    return pose.to(dev).contiguous()


def cloud_index(points, cell):
    """The sorted-key grid index of one cloud, the prologue of point_normals on its own: bounds (one host read), keys on the grid of `cell`
    with the origin at the cloud's minimum, a stable sort, the kept rows gathered into key order (cmr_cloud_gather4_f32).  points float32
    [n, 3] -> CloudIndex.  A cloud without a finite row gives an empty index (kept = 0) and no launch."""
    cell = _cloud_scalar(cell, "cell")
    points = _cloud_points(points)
    n, dev = points.shape[0], points.device
    lo, kept, keys, order = _cloud_grid(points, cell, "cloud_index")
    if kept == 0:
        return CloudIndex(torch.empty((0, 4), dtype=f32, device=dev), torch.empty((0,), dtype=torch.int64, device=dev),
                          torch.empty((0,), dtype=torch.int64, device=dev), (0.0, 0.0, 0.0), cell, 0, n)
    pts4 = torch.empty((kept, 4), dtype=f32, device=dev)
    _lib.call("cmr_cloud_gather4_f32", _p(points), 3, _p(order), kept, _p(pts4), _stream())
    return CloudIndex(pts4, keys, order, tuple(float(v) for v in lo), cell, kept, n)


def cloud_nearest(index, queries, max_dist=None, pose=None):
    """The nearest row of an indexed cloud for every query row (cmr_cloud_nearest_f32; the contract is the header's): exact, the lowest
    row on equal distances.  index: ops.cloud_index of the target; queries float32 [M, 3]; max_dist <= index.cell (default: the cell); pose
    float32 [4, 4] or None: the queries are moved by it first, in fp32.  -> CloudNearest(idx int32 [M], dist2 float32 [M])."""
    who = "cloud_nearest"
    max_dist = _cloud_index_arg(index, max_dist, who)
    queries = _cloud_points(queries, "queries")
    M, dev = queries.shape[0], queries.device
    pose = _cloud_pose(pose, dev, who)
    _cloud_family(who, dev, index, "queries must be on the device of the index")
    if M == 0 or index.kept == 0:
        return CloudNearest(*_none_found(M, dev))
    idx = torch.empty((M,), dtype=torch.int32, device=dev)
    dist2 = torch.empty((M,), dtype=f32, device=dev)
    o = index.origin
    _lib.call("cmr_cloud_nearest_f32", _p(queries), 3, M, _p(pose), _p(index.pts4), _p(index.keys), _p(index.order), index.kept, o[0], o[1], o[2],
              index.cell, max_dist, _p(idx), _p(dist2), _stream())
    return CloudNearest(idx, dist2)


def icp_point_to_plane(source, target, target_normals, pose=None, max_dist=1.0, huber=0.0, iters=30, tol_rot=1e-6, tol_trans=1e-6, index=None,
                       want_system=False):
    """Point-to-plane ICP of one cloud onto another (cmr_icp_point_to_plane_f32; the contract is the header's): the pose that maps the
    source rows onto the planes through their nearest target rows, Gauss-Newton from `pose` (identity by default), every iteration on the
    device and one host read at the end.  source float32 [M, 3]; target float32 [n, 3] (may be None when `index` is given);
    target_normals float32 [n, 3] in the target's row order, zero rows take no part; index: ops.cloud_index(target, cell >= max_dist),
    built here with cell = max_dist when None -- pass one to register several sources, or several start poses, against one target.
    huber: residuals above it are down-weighted by huber / |r| (0: off).  -> IcpResult.  An empty source or target returns the start pose
    with status 2 and no launch."""
    who = "icp_point_to_plane"
    max_dist = _cloud_scalar(max_dist, "max_dist")
    huber = _f32_arg(who, "huber", huber, "be a finite number >= 0")
    tol_rot = _f32_arg(who, "tol_rot", tol_rot, "be a finite number >= 0")
    tol_trans = _f32_arg(who, "tol_trans", tol_trans, "be a finite number >= 0")
    iters = _int_arg(who, "iters", iters, 0, ICP_MAX_ITERS)
    if index is not None:
        _cloud_index_arg(index, max_dist, who)
    elif target is None:
        raise ValueError("%s: give the target cloud or its index" % who)
    source = _cloud_points(source, "source")
    dev = source.device
    target_normals = _cloud_points(target_normals, "target_normals")
    if target is not None:
        target = _cloud_points(target, "target")
    n = _cloud_family(who, dev, index, "source, target, target_normals and the index must be on one device",
                      ("the target has", target, "target_normals", target_normals))
    pose = _cloud_pose(pose, dev, who)
    if pose is None:
        pose = torch.eye(4, dtype=f32, device=dev)
    M = source.shape[0]
    if index is None and M and n:
        index = cloud_index(target, max_dist)
    trace = torch.zeros((iters, 4), dtype=torch.float64, device=dev)
    system = torch.zeros((iters, 28), dtype=torch.float64, device=dev) if want_system else None
    if M == 0 or n == 0 or index.kept == 0:
        return IcpResult(pose.clone(), 0, 0.0, 0, 2, trace.cpu(), None if system is None else system.cpu())
    out = torch.empty((4, 4), dtype=f32, device=dev)
    status = torch.empty((2,), dtype=torch.int32, device=dev)
    nb = _lib.load().cmr_icp_point_to_plane_workspace_bytes(M)
    ws = _ws(nb, dev)
    o = index.origin
    _lib.call("cmr_icp_point_to_plane_f32", _p(source), 3, M, _p(index.pts4), _p(index.keys), _p(index.order), index.kept, o[0], o[1], o[2],
              index.cell, _p(target_normals), _p(pose), max_dist, huber, iters, tol_rot, tol_trans, _p(out), _p(trace), _p(system), _p(status),
              _p(ws), nb, _stream())
    code, executed = (int(v) for v in status.cpu())                    # the one host read (trace and system ride behind it)
    trace = trace.cpu()
    last = trace[executed - 1] if executed else torch.zeros(4, dtype=torch.float64)
    return IcpResult(out, int(last[0]), float(last[1]), executed, code, trace, None if system is None else system.cpu())


# ---- registration without a start pose: FPFH, nearest descriptors, RANSAC (csrc/cloud_fpfh.hip, csrc/cloud_global.hip) -------
FPFH_DIM = 33
DESCRIPTOR_MAX_WIDTH = 64
RANSAC_MAX_HYP = 1 << 20
RANSAC_MAX_CORR = 1 << 24
RANSAC_STATUS = ("ok", "fewer than 3 correspondences", "no valid hypothesis")


class PointFpfh(collections.namedtuple("PointFpfh", "fpfh count spfh")):
    """point_fpfh's result: fpfh float32 [N, 33], count int32 [N] = the neighbours that take part (the row itself not counted), spfh int32
    [N, 33] = the row's own three histograms as integer counts (None unless asked for).  All in the input's row order."""


class DescriptorNearest(collections.namedtuple("DescriptorNearest", "idx dist2")):
    """descriptor_nearest's result: idx int32 [M] = the nearest selected target row (-1: none), dist2 float32 [M] (NaN where idx is -1)."""


class RansacRigid(collections.namedtuple("RansacRigid", "pose inliers status best hyp_inliers")):
    """ransac_rigid's result: pose float32 [4, 4] on the device (source -> target); inliers; status 0 .. 2 (RANSAC_STATUS); best = the
    winning hypothesis (-1 without one); hyp_inliers int32 [n_hyp] on the device, -1 for an invalid hypothesis (None unless asked for)."""


class GlobalResult(collections.namedtuple("GlobalResult", "pose inliers correspondences status icp")):
    """register_global's result: pose float32 [4, 4] on the device; inliers and status of the RANSAC stage; correspondences = the number
    handed to it; icp = the IcpResult of the polish (None with refine=False or when RANSAC found nothing)."""


def point_fpfh(points, normals, radius, index=None, want_spfh=False):
    """FPFH descriptors of one cloud from its normals (cmr_point_fpfh_f32; the contract is the header's): Open3D's ComputeFPFHFeature with a
    pure radius search.  points, normals float32 [N, 3]; a row takes part when it is finite and its normal is finite and not zero, any
    other row gets zeros and is nobody's neighbour.  index: ops.cloud_index(points, cell >= radius), built here with cell = radius when
    None.  -> PointFpfh.  Two launches; no host read beyond cloud_index's."""
    who = "point_fpfh"
    radius = _cloud_scalar(radius, "radius")
    if index is not None:
        _cloud_index_arg(index, radius, who, "radius", "a neighbour must lie in the row's cell or one next to it")
    points = _cloud_points(points)
    normals = _cloud_points(normals, "normals")
    N, dev = points.shape[0], points.device
    _cloud_family(who, dev, index, "points, normals and the index must be on one device", ("points has", points, "normals", normals))
    if index is None and N:
        index = cloud_index(points, radius)
    if N == 0 or index.kept == 0:
        return PointFpfh(torch.zeros((N, FPFH_DIM), dtype=f32, device=dev), torch.zeros((N,), dtype=torch.int32, device=dev),
                         torch.zeros((N, FPFH_DIM), dtype=torch.int32, device=dev) if want_spfh else None)
    fpfh = torch.empty((N, FPFH_DIM), dtype=f32, device=dev)
    count = torch.empty((N,), dtype=torch.int32, device=dev)
    spfh = torch.empty((N, FPFH_DIM), dtype=torch.int32, device=dev) if want_spfh else None
    nb = _lib.load().cmr_point_fpfh_workspace_bytes(index.kept)
    ws = _ws(nb, dev)
    o = index.origin
    _lib.call("cmr_point_fpfh_f32", _p(index.pts4), _p(index.keys), _p(index.order), N, index.kept, o[0], o[1], o[2], index.cell, _p(normals),
              radius, _p(fpfh), _p(count), _p(spfh), _p(ws), nb, _stream())
    return PointFpfh(fpfh, count, spfh)


def _descriptor_rows(who, name, t):
    if not isinstance(t, torch.Tensor) or t.dtype != f32 or t.dim() != 2 or t.shape[1] < 1:
        raise ValueError("%s: %s must be a float32 [rows, C >= 1] tensor, got %s %s" % ((who, name) + _got(t)))
    if t.shape[0] > CLOUD_MAX_ROWS:
        raise ValueError("%s: %s holds %d rows; at most 2^31 - 1 (int32 row ids)" % (who, name, t.shape[0]))
    return t


def _byte_mask(who, name, m, n):
    if m is None:
        return None
    if not isinstance(m, torch.Tensor) or m.dtype not in (torch.bool, torch.uint8) or tuple(m.shape) != (n,):
        raise ValueError("%s: %s must be None or bool / uint8 [%d], got %s %s" % ((who, name, n) + _got(m)))
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def descriptor_nearest(queries, targets, query_mask=None, target_mask=None):
    """The nearest target descriptor of every query descriptor by brute force (cmr_descriptor_nearest_f32; the contract is the header's):
    the plain fp32 sum of squared differences in channel order, the lowest row on equal distances -- exact against float32 numpy.  queries
    float32 [M, C], targets float32 [N, C], C <= 64; masks bool / uint8 [M] / [N] or None = every row.  -> DescriptorNearest; -1 / NaN for an
    unselected query, a query with a non-finite entry and when no target is selected."""
    who = "descriptor_nearest"
    queries = _descriptor_rows(who, "queries", queries)
    targets = _descriptor_rows(who, "targets", targets)
    M, C = queries.shape
    N = targets.shape[0]
    if targets.shape[1] != C:
        raise ValueError("%s: queries have %d channels, targets %d" % (who, C, targets.shape[1]))
    if C > DESCRIPTOR_MAX_WIDTH:
        raise ValueError("%s: %d channels; the kernel serves at most %d (the entry point answers CMR_EUNSUPPORTED)" % (who, C, DESCRIPTOR_MAX_WIDTH))
    query_mask = _byte_mask(who, "query_mask", query_mask, M)
    target_mask = _byte_mask(who, "target_mask", target_mask, N)
    if not queries.is_cuda:
        raise ValueError("%s: queries must be a device tensor (there is no CPU path)" % who)
    queries, targets = queries.contiguous(), targets.contiguous()
    query_mask = None if query_mask is None else query_mask.contiguous()
    target_mask = None if target_mask is None else target_mask.contiguous()
    _on_one_gpu(who, queries, targets, query_mask, target_mask)
    dev = queries.device
    if M == 0 or N == 0:
        return DescriptorNearest(*_none_found(M, dev))
    idx = torch.empty((M,), dtype=torch.int32, device=dev)
    dist2 = torch.empty((M,), dtype=f32, device=dev)
    _lib.call("cmr_descriptor_nearest_f32", _p(queries), M, _p(targets), N, C, _p(query_mask), _p(target_mask), _p(idx), _p(dist2), _stream())
    return DescriptorNearest(idx, dist2)


def ransac_rigid(source_pts, target_pts, corr, n_hyp=4096, thr=0.3, edge_ratio=0.9, seed=0, want_hyp_inliers=False):
    """The rigid transform that most correspondences agree on, by RANSAC over 3-point hypotheses (cmr_ransac_rigid_f32; the contract is the
    header's).  source_pts float32 [M, 3], target_pts float32 [N, 3], corr int32 [L, 2] = (source row, target row); rows of corr with an
    index out of range (-1 included) are dropped on the device.  -> RansacRigid.  Everything is enqueued on the stream; the one host read is
    status / inliers / best."""
    who = "ransac_rigid"
    n_hyp = _int_arg(who, "n_hyp", n_hyp, 1, RANSAC_MAX_HYP)
    thr = _cloud_scalar(thr, "thr")
    edge_ratio = _f32_arg(who, "edge_ratio", edge_ratio, "be a number in [0, 1]", 0.0, 1.0, bools=False)
    seed = _int_arg(who, "seed", seed, 0, (1 << 32) - 1)
    if not isinstance(corr, torch.Tensor) or corr.dtype != torch.int32 or corr.dim() != 2 or corr.shape[1] != 2:
        raise ValueError("%s: corr must be an int32 [L, 2] tensor, got %s %s" % ((who,) + _got(corr)))
    L = corr.shape[0]
    if L > RANSAC_MAX_CORR:
        raise ValueError("%s: corr holds %d rows; at most 2^24" % (who, L))
    source_pts = _cloud_points(source_pts, "source_pts")
    target_pts = _cloud_points(target_pts, "target_pts")
    corr = corr.contiguous()
    _on_one_gpu(who, source_pts, target_pts, corr)
    dev = source_pts.device
    hyp = torch.full((n_hyp,), -1, dtype=torch.int32, device=dev) if want_hyp_inliers else None
    if L == 0 or source_pts.shape[0] == 0 or target_pts.shape[0] == 0:
        return RansacRigid(torch.eye(4, dtype=f32, device=dev), 0, 1, -1, hyp)
    pose = torch.empty((4, 4), dtype=f32, device=dev)
    result = torch.empty((3,), dtype=torch.int32, device=dev)
    nb = _lib.load().cmr_ransac_rigid_workspace_bytes(L, n_hyp)
    ws = _ws(nb, dev)
    _lib.call("cmr_ransac_rigid_f32", _p(source_pts), source_pts.shape[0], _p(target_pts), target_pts.shape[0], _p(corr), L, n_hyp, thr,
              edge_ratio, seed, _p(pose), _p(result), _p(hyp), _p(ws), nb, _stream())
    inliers, status, best = (int(v) for v in result.cpu())             # the one host read
    return RansacRigid(pose, inliers, status, best, hyp)


def register_global(source, source_normals, target, target_normals, radius=1.0, mutual=True, n_hyp=4096, thr=0.3, edge_ratio=0.9, seed=0,
                    refine=True, **icp):
    """One cloud onto another without a start pose: point_fpfh on both, descriptor_nearest source -> target (with `mutual` also target ->
    source, a correspondence is kept when the two agree; rows without a neighbour are masked out), ransac_rigid on the kept
    correspondences and, with `refine`, icp_point_to_plane from the RANSAC pose (keywords `icp`, defaults max_dist=1.0, huber=0.1).  ->
    GlobalResult; pose is the polish's when its status is 0 or 1, RANSAC's otherwise."""
    who = "register_global"
    if not isinstance(mutual, bool) or not isinstance(refine, bool):
        raise ValueError("%s: mutual and refine must be True or False, got %r / %r" % (who, mutual, refine))
    unknown = set(icp) - {"max_dist", "huber", "iters", "tol_rot", "tol_trans"}
    if unknown:
        raise ValueError("%s: unknown keyword(s) %s" % (who, ", ".join(sorted(unknown))))
    fs = point_fpfh(source, source_normals, radius)
    ft = point_fpfh(target, target_normals, radius)
    sm, tm = fs.count > 0, ft.count > 0
    fwd = descriptor_nearest(fs.fpfh, ft.fpfh, sm, tm)
    keep = fwd.idx >= 0
    if mutual and ft.fpfh.shape[0]:
        back = descriptor_nearest(ft.fpfh, fs.fpfh, tm, sm)
        rows = torch.arange(fs.fpfh.shape[0], dtype=torch.int32, device=fs.fpfh.device)
        keep = keep & (back.idx[fwd.idx.clamp(min=0).long()] == rows)
    src_rows = torch.nonzero(keep).reshape(-1)                          # the compaction: torch plumbing, in row order
    corr = torch.stack([src_rows.to(torch.int32), fwd.idx[src_rows]], 1).contiguous()
    rr = ransac_rigid(source, target, corr, n_hyp, thr, edge_ratio, seed)
    if not refine or rr.status != 0:
        return GlobalResult(rr.pose, rr.inliers, corr.shape[0], rr.status, None)
    kw = dict(max_dist=1.0, huber=0.1)
    kw.update(icp)
    res = icp_point_to_plane(source, target, target_normals, pose=rr.pose, **kw)
    return GlobalResult(res.pose if res.status in (0, 1) else rr.pose, rr.inliers, corr.shape[0], rr.status, res)


# ---- a voxel map of registered scans: insert, merge, forget (csrc/voxel_map.hip) --------------------------------------------
VOXEL_MAP_MAX_STAMP = (1 << 31) - 1


class VoxelMap(collections.namedtuple("VoxelMap", "keys points attr count stamp origin voxel")):
    """A voxel map: keys int64 [n] ascending and unique, points float32 [n, 3] and attr float32 [n, C] = the running means of the rows that
    fell into each voxel, count int32 [n] = their number, stamp int32 [n] = the stamp of the last insert that touched the voxel; origin =
    the grid's origin (three python floats holding fp32 values, fixed for the map's life), voxel = its cell.  ops.voxel_map makes the empty
    one, ops.voxel_map_insert a new one from an old one; nothing changes a map in place."""


class MapInsert(collections.namedtuple("MapInsert", "map new merged removed dropped outside")):
    """voxel_map_insert's result: the new map; new = voxels the scan added, merged = voxels of the map the scan touched, removed = rows
    forgotten (stamp below min_stamp after the insert); dropped = input rows with a non-finite coordinate before or after the pose, outside
    = finite input rows off the grid on some axis."""


def voxel_map(voxel, origin, channels=0, device=None):
    """The empty map on the grid (origin, voxel) with `channels` attribute columns.  origin: three finite fp32 values, required -- a map
    that grows cannot take its origin from the first scan's corner, and every later key depends on it."""
    who = "voxel_map"
    voxel = _cloud_scalar(voxel, "voxel")
    origin = tuple(float(np.float32(v)) for v in _cloud_triple(origin, "origin"))
    channels = _int_arg(who, "channels", channels, 0, 1 << 16)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return VoxelMap(torch.empty((0,), dtype=torch.int64, device=dev), torch.empty((0, 3), dtype=f32, device=dev),
                    torch.empty((0, channels), dtype=f32, device=dev), torch.empty((0,), dtype=torch.int32, device=dev),
                    torch.empty((0,), dtype=torch.int32, device=dev), origin, voxel)


def _voxel_map_arg(map, who):
    """-> (rows, channels, device) of a well-formed VoxelMap; ValueError for anything else.  That the keys ascend is the map's contract and is
    not read back."""
    if not isinstance(map, VoxelMap):
        raise ValueError("%s: map must be a VoxelMap (ops.voxel_map), got %s" % (who, type(map).__name__))
    want = (("keys", torch.int64, 1), ("points", f32, 2), ("attr", f32, 2), ("count", torch.int32, 1), ("stamp", torch.int32, 1))
    for name, dtype, dim in want:
        t = getattr(map, name)
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != dim:
            raise ValueError("%s: malformed VoxelMap: %s must be a %s tensor of %d dimension(s), got %s %s" % ((who, name, dtype, dim) + _got(t)))
    n = map.keys.shape[0]
    if tuple(map.points.shape) != (n, 3) or map.attr.shape[0] != n or map.count.shape[0] != n or map.stamp.shape[0] != n:
        raise ValueError("%s: malformed VoxelMap: %d keys, points %s, attr %s, count %s, stamp %s" % (
            who, n, tuple(map.points.shape), tuple(map.attr.shape), tuple(map.count.shape), tuple(map.stamp.shape)))
    if n > CLOUD_MAX_ROWS:
        raise ValueError("%s: malformed VoxelMap: %d rows; at most 2^31 - 1" % (who, n))
    if any(getattr(map, name).device != map.keys.device for name, _, _ in want):
        raise ValueError("%s: malformed VoxelMap: its tensors are on different devices" % who)
    try:
        _cloud_scalar(map.voxel, "voxel")
        if tuple(float(np.float32(v)) for v in _cloud_triple(map.origin, "origin")) != tuple(map.origin):
            raise ValueError("origin must hold float32 values, got %r" % (map.origin,))
    except (TypeError, ValueError) as e:
        raise ValueError("%s: malformed VoxelMap: %s" % (who, e))
    return n, map.attr.shape[1], map.keys.device


def voxel_map_insert(map, points=None, attr=None, pose=None, stamp=0, min_stamp=None):
    """One scan into a voxel map (cmr_voxel_map_keys_f32 / _voxel_means' heads and cmr_segment_reduce_f32 / cmr_voxel_map_plan_i64 /
    cmr_voxel_map_write_f32; the contract is the header's) -> MapInsert with a NEW map; `map` is not changed.  points float32 [N, 3] in
    the scan's frame, attr float32 [N, C] with the map's C channels (None when C = 0), pose float32 [4, 4] or None: the scan's pose in the
    map's frame, applied in fp32.  Rows with a non-finite coordinate are dropped and rows off the grid counted as outside; neither is an
    error.  Touched and new voxels get `stamp`; with min_stamp, voxels whose stamp is then below it are forgotten.  points=None (or an empty
    scan) with min_stamp is a pure prune.  The host reads back sizes only, three times: the dropped and outside counts, the scan's voxel
    count, the new map's sizes (a scan without a kept row: two; without rows: one) -- not capturable in a graph."""
    who = "voxel_map_insert"
    M, C, dev = _voxel_map_arg(map, who)
    stamp = _int_arg(who, "stamp", stamp, 0, VOXEL_MAP_MAX_STAMP)
    if min_stamp is not None:
        min_stamp = _int_arg(who, "min_stamp", min_stamp, 0, VOXEL_MAP_MAX_STAMP)
    if points is None:
        if attr is not None:
            raise ValueError("%s: attr without points" % who)
    else:
        if attr is None and C:
            raise ValueError("%s: the map has %d attribute channel(s), attr is None" % (who, C))
        if attr is not None:
            if not isinstance(attr, torch.Tensor) or attr.dtype != f32 or attr.dim() != 2:
                raise ValueError("%s: attr must be a float32 [N, C] tensor or None, got %s %s" % ((who,) + _got(attr)))
            if attr.shape[1] != C:
                raise ValueError("%s: attr has %d channel(s), the map %d" % (who, attr.shape[1], C))
            if isinstance(points, torch.Tensor) and points.dim() == 2 and attr.shape[0] != points.shape[0]:
                raise ValueError("%s: attr has %d rows, points %d" % (who, attr.shape[0], points.shape[0]))
    pose = _cloud_pose(pose, dev, who)
    if points is not None:
        points = _cloud_points(points)
        if points.device != dev or (attr is not None and attr.device != dev):
            raise ValueError("%s: points and attr must be on the map's device" % who)
        if attr is not None:
            attr = attr.contiguous().view(-1).view(attr.shape)      # row strides as the kernels take them, whatever an [N, 1] tensor came with
    if not map.keys.is_cuda:
        raise ValueError("%s: the map must hold device tensors (there is no CPU path)" % who)
    N = 0 if points is None else points.shape[0]
    if M + N > CLOUD_MAX_ROWS:
        raise ValueError("%s: the map's %d rows and the scan's %d exceed 2^31 - 1 together" % (who, M, N))
    lib = _lib.load()
    o = map.origin
    i32, i64 = torch.int32, torch.int64
    dropped = outside = S = 0
    keys = offsets = scan_points = scan_attr = scan_count = None
    if N:
        keys = torch.empty((N,), dtype=i64, device=dev)
        moved = torch.empty((N, 3), dtype=f32, device=dev)
        counts = torch.empty((2,), dtype=i64, device=dev)
        nb = lib.cmr_voxel_map_keys_workspace_bytes(N)
        ws = _ws(nb, dev)
        _lib.call("cmr_voxel_map_keys_f32", _p(points), 3, N, _p(pose), o[0], o[1], o[2], map.voxel, _p(keys), _p(moved), _p(counts), _p(ws), nb,
                  _stream())
        keys, order = torch.sort(keys, stable=True)               # plumbing, as in voxel_downsample
        dropped, outside = (int(v) for v in counts.cpu())       # host read 1
        kept = N - dropped - outside
        keys, order = keys[N - kept:], order[N - kept:]           # both marks sort in front of every cell
        if kept:
            S, offsets, scan_points, scan_attr, scan_count, _ = _voxel_means(keys, order, kept, kept, moved, attr)      # host read 2
    if M + S == 0:
        return MapInsert(VoxelMap(*(t.clone() for t in map[:5]), map.origin, map.voxel), 0, 0, 0, dropped, outside)
    low = 0 if min_stamp is None else min_stamp
    sizes = torch.empty((4,), dtype=i64, device=dev)
    nb = lib.cmr_voxel_map_plan_workspace_bytes(M, S)
    ws = _ws(nb, dev)
    _lib.call("cmr_voxel_map_plan_i64", _p(map.keys), _p(map.stamp), M, _p(keys), _p(offsets), S, stamp, low, _p(sizes), _p(ws), nb, _stream())
    rows, new, merged, removed = (int(v) for v in sizes.cpu())  # host read 3
    out = VoxelMap(torch.empty((rows,), dtype=i64, device=dev), torch.empty((rows, 3), dtype=f32, device=dev),
                   torch.empty((rows, C), dtype=f32, device=dev), torch.empty((rows,), dtype=i32, device=dev),
                   torch.empty((rows,), dtype=i32, device=dev), map.origin, map.voxel)
    _lib.call("cmr_voxel_map_write_f32", _p(map.keys), _p(map.points.contiguous()), _p(map.attr.contiguous()), _p(map.count), _p(map.stamp), M,
              _p(scan_points), _p(scan_attr), _p(scan_count), S, C, stamp, low, _p(ws), nb, rows, _p(out.keys), _p(out.points), _p(out.attr),
              _p(out.count), _p(out.stamp), _stream())
    return MapInsert(out, new, merged, removed, dropped, outside)


# ---- free space in a voxel map: the rays of a scan cast through it (csrc/voxel_map_rays.hip) -----------------------------------
MAP_RAYS_MAX_CELLS = 1 << 16        # the longest walk a ray may be asked for


class MapRays(collections.namedtuple("MapRays", "crossed hits cast dropped outside long")):
    """voxel_map_rays' result: crossed int32 [n] = the rays that passed through each of the map's voxels, hits int32 [n] = the rays that
    ended in it, both aligned with the map's rows; cast = rays walked, dropped = rows with a non-finite coordinate before or after the
    pose, outside = finite rows whose sensor or end lies off the grid, long = rays of more than max_cells steps, which are not walked."""


def voxel_map_rays(map, points, pose=None, start_margin=2, end_margin=1, max_cells=4096):
    """The rays of one scan cast through a voxel map (cmr_voxel_map_rays_f32; the contract is the header's) -> MapRays; `map` is not
    changed.  points float32 [N, 3] in the scan's frame: row i is a beam from the sensor -- the pose's translation, the origin without a
    pose -- to the row moved by the pose, in fp32 as ops.voxel_map_insert moves it.  A voxel within start_margin cells of the ray's first
    cell or within end_margin cells of its last (Chebyshev distances, on any axis) is not counted as crossed.  One host read: the four
    counts."""
    who = "voxel_map_rays"
    M, _, dev = _voxel_map_arg(map, who)
    start_margin = _int_arg(who, "start_margin", start_margin, 0, CLOUD_CELL_LIMIT - 1)
    end_margin = _int_arg(who, "end_margin", end_margin, 0, CLOUD_CELL_LIMIT - 1)
    max_cells = _int_arg(who, "max_cells", max_cells, 1, MAP_RAYS_MAX_CELLS)
    pose = _cloud_pose(pose, dev, who)
    points = _cloud_points(points)
    if points.device != dev:
        raise ValueError("%s: points must be on the map's device" % who)
    if not map.keys.is_cuda:
        raise ValueError("%s: the map must hold device tensors (there is no CPU path)" % who)
    N = points.shape[0]
    crossed = torch.empty((M,), dtype=torch.int32, device=dev)
    hits = torch.empty((M,), dtype=torch.int32, device=dev)
    if N == 0:
        return MapRays(crossed.zero_(), hits.zero_(), 0, 0, 0, 0)
    counts = torch.empty((4,), dtype=torch.int64, device=dev)
    nb = _lib.load().cmr_voxel_map_rays_workspace_bytes(N)
    ws = _ws(nb, dev)
    o = map.origin
    _lib.call("cmr_voxel_map_rays_f32", _p(map.keys) if M else None, M, o[0], o[1], o[2], map.voxel, _p(points), 3, N, _p(pose), start_margin,
              end_margin, max_cells, _p(crossed) if M else None, _p(hits) if M else None, _p(counts), _p(ws), nb, _stream())
    return MapRays(crossed, hits, *(int(v) for v in counts.cpu()))


def voxel_map_keep(map, mask):
    """The rows of a voxel map where mask (bool [n], on the map's device) is true, as a NEW map on the same grid: torch indexing."""
    who = "voxel_map_keep"
    M, _, dev = _voxel_map_arg(map, who)
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or tuple(mask.shape) != (M,) or mask.device != dev:
        raise ValueError("%s: mask must be a bool [%d] tensor on the map's device, got %s %s%s" % (
            (who, M) + _got(mask) + (" on %s" % mask.device if torch.is_tensor(mask) else "",)))
    return VoxelMap(*(t[mask] for t in map[:5]), map.origin, map.voxel)


# ---- place recognition between scans: ring-and-sector descriptors and their ring-shift match (csrc/scan_descriptor.hip) -----
SCAN_MAX_RINGS = 64
SCAN_MAX_SECTORS = 256
SCAN_MAX_CELLS = 4096               # rings x sectors: the image a workgroup keeps in LDS is 16 KiB at most
SCAN_MATCH_CALL_BYTES = 1 << 28     # dist and shift of ONE cmr_scan_match_f32 call stay under this; scan_match splits its queries to keep it


class ScanDescriptor(collections.namedtuple("ScanDescriptor", "desc binned dropped outside")):
    """scan_descriptor's result: desc float32 [rings, sectors] = per cell the largest z + height over its rows, 0 when none is above 0;
    binned = rows that fell into a cell, dropped = rows with a non-finite coordinate, outside = finite rows nearer than min_range or at
    or beyond max_range.  The three sum to the cloud's rows."""


class ScanMatch(collections.namedtuple("ScanMatch", "dist shift")):
    """scan_match's result: dist float32 [Q, N] = the least column-cosine distance over the ring shifts that count, shift int32 [Q, N] = the
    lowest shift that reaches it; NaN and -1 where no shift counts and for every candidate at or beyond the query's limit."""


def _azimuth_shape(who, names, shape, most):
    """The shape of an image whose second axis goes round the circle in quarters (a scan descriptor, a range image): names = what the
    caller calls the two axes, most = (the first axis', the second's, the cells') upper bounds -> the two as ints"""
    a = _int_arg(who, names[0], shape[0], 1, most[0])
    b = _int_arg(who, names[1], shape[1], 4, most[1])
    if b % 4 or a * b > most[2]:
        raise ValueError("%s: %s must be a multiple of 4 and %s x %s at most %d, got %d x %d" % (who, names[1], names[0], names[1], most[2], a, b))
    return a, b


def _azimuth_dirs(bins):
    """float32 [bins / 4 - 1, 2] = (cos, sin) of the edges inside the first quadrant of a circle cut into `bins`, computed in float64 and
    rounded: the table csrc/cmr_scan_rows.h bisects"""
    k = np.arange(1, bins // 4, dtype=np.float64) * (2.0 * np.pi / bins)
    return np.stack([np.cos(k), np.sin(k)], 1).astype(np.float32)


def _scan_shape(who, rings, sectors):
    return _azimuth_shape(who, ("rings", "sectors"), (rings, sectors), (SCAN_MAX_RINGS, SCAN_MAX_SECTORS, SCAN_MAX_CELLS))


def scan_tables(rings, sectors, min_range, max_range):
    """The two tables cmr_scan_descriptor_f32 reads, computed in float64 and rounded to float32 (numpy): ring_edge2 [rings + 1] = the squared
    ring edges, sector_dir [sectors / 4 - 1, 2] = (cos, sin) of the sector edges inside the first quadrant."""
    j = np.arange(rings + 1, dtype=np.float64)
    return ((min_range + (max_range - min_range) * j / rings) ** 2).astype(np.float32), _azimuth_dirs(sectors)


def scan_descriptor(points, rings=20, sectors=60, max_range=80.0, min_range=0.0, height=2.0):
    """The ring-and-sector descriptor of one scan (cmr_scan_descriptor_f32; the contract is the header's): the cloud seen from above, cut
    into `rings` rings between min_range and max_range and `sectors` sectors from the x axis towards y, each cell holding the largest
    z + height of its rows.  points float32 [N, 3] in the sensor's frame -> ScanDescriptor.  One host read: the three counts."""
    who = "scan_descriptor"
    rings, sectors = _scan_shape(who, rings, sectors)
    max_range = _cloud_scalar(max_range, "max_range")
    min_range = _f32_arg(who, "min_range", min_range, "be a number in [0, max_range)", 0.0)
    if not np.float32(min_range) < np.float32(max_range):
        raise ValueError("%s: min_range must be a number in [0, max_range), got %r with max_range %r" % (who, min_range, max_range))
    height = _f32_arg(who, "height", height, "be a finite number", -math.inf)
    points = _cloud_points(points)
    N, dev = points.shape[0], points.device
    desc = torch.empty((rings, sectors), dtype=f32, device=dev)
    if N == 0:
        return ScanDescriptor(desc.zero_(), 0, 0, 0)
    edge2, dirs = (torch.from_numpy(t).to(dev) for t in scan_tables(rings, sectors, min_range, max_range))
    counts = torch.empty((3,), dtype=torch.int64, device=dev)
    _lib.call("cmr_scan_descriptor_f32", _p(points), 3, N, rings, sectors, _p(edge2), _p(dirs) if sectors > 4 else None, height, _p(desc),
              _p(counts), _stream())
    return ScanDescriptor(desc, *(int(v) for v in counts.cpu()))


def _scan_batch(who, name, t):
    if not isinstance(t, torch.Tensor) or t.dtype != f32 or t.dim() != 3:
        raise ValueError("%s: %s must be a float32 [n, rings, sectors] tensor, got %s %s" % ((who, name) + _got(t)))
    if not 0 < t.shape[0] <= CLOUD_MAX_ROWS:
        raise ValueError("%s: %s holds %d descriptors; need 1 to 2^31 - 1" % (who, name, t.shape[0]))
    if not t.is_cuda:
        raise ValueError("%s: %s must be a device tensor (there is no CPU path)" % (who, name))
    return t.contiguous()


def scan_match(queries, cands, limit=None, min_cols=None):
    """Every query descriptor against every candidate at every ring shift (cmr_scan_match_f32; the contract is the header's) -> ScanMatch.
    queries float32 [Q, R, S], cands float32 [N, R, S]; limit int32 [Q] or None: query q meets the candidates [0, limit[q]) only (a loop
    search passes the earlier frames); min_cols: a shift counts when that many column pairs are non-empty on both sides (default S // 4).
    The queries are split so that one call's outputs stay under SCAN_MATCH_CALL_BYTES; the result does not depend on the split."""
    who = "scan_match"
    queries, cands = _scan_batch(who, "queries", queries), _scan_batch(who, "cands", cands)
    if queries.shape[1:] != cands.shape[1:]:
        raise ValueError("%s: queries are %d x %d, cands %d x %d" % ((who,) + tuple(queries.shape[1:]) + tuple(cands.shape[1:])))
    R, S = _scan_shape(who, queries.shape[1], queries.shape[2])
    min_cols = _int_arg(who, "min_cols", S // 4 if min_cols is None else min_cols, 1, S)
    Q, N, dev = queries.shape[0], cands.shape[0], queries.device
    if cands.device != dev:
        raise ValueError("%s: queries and cands must be on one device" % who)
    if limit is not None:
        if not isinstance(limit, torch.Tensor) or limit.dtype != torch.int32 or limit.dim() != 1:
            raise ValueError("%s: limit must be an int32 [Q] tensor or None, got %s %s" % ((who,) + _got(limit)))
        _cloud_family(who, dev, None, "limit must be on the device of queries", ("queries hold", queries, "limit", limit))
        limit = limit.contiguous()
        if Q and (int(limit.min()) < 0 or int(limit.max()) > N):
            raise ValueError("%s: limit must lie in [0, %d] (the candidates), got [%d, %d]" % (who, N, int(limit.min()), int(limit.max())))
    dist = torch.empty((Q, N), dtype=f32, device=dev)
    shift = torch.empty((Q, N), dtype=torch.int32, device=dev)
    step = max(1, SCAN_MATCH_CALL_BYTES // (8 * N))
    lib = _lib.load()
    for a in range(0, Q, step):
        b = min(Q, a + step)
        nb = lib.cmr_scan_match_workspace_bytes(b - a, N, R, S)
        ws = _ws(nb, dev)
        _lib.call("cmr_scan_match_f32", _p(queries[a:b]), b - a, _p(cands), N, R, S, _p(limit[a:b]) if limit is not None else None, min_cols,
                  _p(dist[a:b]), _p(shift[a:b]), _p(ws), nb, _stream())
    return ScanMatch(dist, shift)


def scan_shift_yaw(shift, sectors):
    """The heading a ring shift stands for: -shift 2 pi / sectors wrapped into (-pi, pi] (python float, or numpy float64 for an array of
    shifts).  Turning the candidate's points by it about z brings them onto the query's: p_query ~ Rz(yaw) p_candidate."""
    sectors = _int_arg("scan_shift_yaw", "sectors", sectors, 1, 1 << 30)
    k = np.mod(-np.asarray(shift, dtype=np.int64), sectors)
    yaw = np.where(2 * k > sectors, k - sectors, k) * (2.0 * np.pi / sectors)
    return float(yaw) if yaw.ndim == 0 else yaw


# ---- a pose-graph solve over a chain of poses and its loop edges (csrc/pose_graph.hip) ------------------------------------------
PG_MAX_ITERS = 100
PG_MAX_CG_ITERS = 4096
PG_STATUS = ("converged", "iterations exhausted", "singular block or non-finite value", "wide edges at the start")


class PoseGraphTerms(collections.namedtuple("PoseGraphTerms", "r chi scale A b cost wide")):
    """pose_graph_linearize's result, float64 on the device: r [E, 6] = (phi, rho), chi [E], scale [E] = the Huber factor s_e, A [E, 21] =
    s_e J^T W J (upper triangle, row by row), b [E, 6] = s_e J^T W r; cost (python float) and wide (int, edges turned by more than 3 rad)."""


class PoseGraphResult(collections.namedtuple("PoseGraphResult", "poses cost iterations status trace")):
    """pose_graph_optimize's result: poses float64 [F, 4, 4] on the device; cost at them; iterations = steps executed (an undone one
    counts); status 0 .. 3 (PG_STATUS); trace float64 [iters, 5] = cost the step started from, CG iterations used, sqrt(r.z / r0.z0) at
    the end of CG, max |dw|, max |dv| per executed step (host)."""


def _pg_edges(who, edges):
    if not isinstance(edges, torch.Tensor) or edges.dtype != torch.int32 or edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError("%s: edges must be an int32 [E, 2] tensor, got %s %s" % ((who,) + _got(edges)))
    return edges.contiguous()


def _pg_f64(who, name, t, *shape):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
        raise ValueError("%s: %s must be a float64 tensor, got %s %s" % ((who, name) + _got(t)))
    _shaped(who, name, t, *shape)
    return t.contiguous()


def _pg_graph(who, poses, edges, meas, weights, fixed=None):
    """The tensors of a graph, checked: types, shapes, one device, sizes, and -- in ONE host read -- indices, weights and finiteness.
    -> poses, edges, meas, weights, fixed (uint8 [F]; None in, None out), F, E."""
    poses = _pg_f64(who, "poses", poses, "F", 4, 4)
    edges = _pg_edges(who, edges)
    F, E = poses.shape[0], edges.shape[0]
    meas = _pg_f64(who, "meas", meas, E, 4, 4)
    weights = _pg_f64(who, "weights", weights, E, 2)
    if F < 1:
        raise ValueError("%s: need at least one pose" % who)
    if 6 * F >= 1 << 31 or 28 * E >= 1 << 31:
        raise ValueError("%s: %d poses and %d edges: 6 F and 28 E must stay below 2^31" % (who, F, E))
    ts = [poses, edges, meas, weights]
    if fixed is not None:
        if not isinstance(fixed, torch.Tensor) or fixed.dtype != torch.bool or tuple(fixed.shape) != (F,):
            raise ValueError("%s: fixed must be a bool [%d] tensor or None, got %s %s" % ((who, F) + _got(fixed)))
        ts.append(fixed)
    if any(t.device != poses.device for t in ts):
        raise ValueError("%s: poses, edges, meas, weights and fixed must be on one device" % who)
    flags = [(edges[:, 0] == edges[:, 1]).any(), ((edges < 0) | (edges >= F)).any(), (~torch.isfinite(weights) | (weights < 0)).any(),
             (~torch.isfinite(poses)).any(), (~torch.isfinite(meas)).any(),
             fixed.all() if fixed is not None else torch.zeros((), dtype=torch.bool, device=poses.device)]
    same, outside, weight, pose, measured, none_free = torch.stack(flags).cpu().tolist()                  # the one host read
    if same:
        raise ValueError("%s: an edge joins a pose to itself" % who)
    if outside:
        raise ValueError("%s: an edge names a pose outside [0, %d)" % (who, F))
    if weight:
        raise ValueError("%s: weights must be finite and >= 0" % who)
    if pose or measured:
        raise ValueError("%s: %s must be finite" % (who, "poses" if pose else "meas"))
    if none_free:
        raise ValueError("%s: every pose is fixed: there is nothing to solve" % who)
    return poses, edges, meas, weights, (fixed.to(torch.uint8).contiguous() if fixed is not None else None), F, E


def _pg_on_gpu(who, t):
    if not t.is_cuda:
        raise ValueError("%s: the tensors must be on a GPU (there is no CPU path)" % who)


def pose_graph_incidence(edges, F):
    """The incidence of a graph's F nodes as a CSR, on edges' device (pure torch; runs on the CPU too): offsets int32 [F + 1], edge numbers
    int32 [2 E] -- a node's edges ascending, by a STABLE sort, a duplicate edge once per copy -- and signs int32 [2 E]: +1 where the node
    is the edge's i, -1 where it is its j.  edges int32 [E, 2] with every index in [0, F) (pose_graph_optimize checks that; here an index
    outside raises from torch or is a ValueError)."""
    who = "pose_graph_incidence"
    edges = _pg_edges(who, edges)
    F = _int_arg(who, "F", F, 1, (1 << 31) // 6)
    nodes = edges.reshape(-1).to(torch.int64)                          # entry 2 e is edge e's i, 2 e + 1 its j
    if nodes.numel() and (int(nodes.min()) < 0 or int(nodes.max()) >= F):
        raise ValueError("%s: an edge names a pose outside [0, %d)" % (who, F))
    order = torch.sort(nodes, stable=True).indices
    counts = torch.bincount(nodes, minlength=F)
    offsets = torch.zeros((F + 1,), dtype=torch.int64, device=edges.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets.to(torch.int32), (order // 2).to(torch.int32), (1 - 2 * (order % 2)).to(torch.int32)


def pose_graph_linearize(poses, edges, meas, weights, huber=0.0):
    """Every edge's residual, weight and Gauss-Newton terms at the given poses (cmr_pose_graph_linearize_f64; the contract is the
    header's).  poses float64 [F, 4, 4] (X_n maps frame n into the first frame), edges int32 [E, 2] = (i, j), meas float64 [E, 4, 4] (Z_e
    maps frame i into frame j), weights float64 [E, 2] = (w_rot, w_trans).  -> PoseGraphTerms.  chi before and after a solve is how a wrong
    loop shows.  E = 0 gives empty terms and no launch."""
    who = "pose_graph_linearize"
    huber = _f32_arg(who, "huber", huber, "be a finite number >= 0", as_f32=False, bools=False)
    poses, edges, meas, weights, _, F, E = _pg_graph(who, poses, edges, meas, weights)
    dev = poses.device
    r, chi, scale, A, b = (torch.empty((E,) + s, dtype=torch.float64, device=dev) for s in ((6,), (), (), (21,), (6,)))
    if E == 0:
        return PoseGraphTerms(r, chi, scale, A, b, 0.0, 0)
    _pg_on_gpu(who, poses)
    cost = torch.empty((1,), dtype=torch.float64, device=dev)
    wide = torch.empty((1,), dtype=torch.int32, device=dev)
    nb = _lib.load().cmr_pose_graph_linearize_workspace_bytes(E)
    ws = _ws(nb, dev)
    _lib.call("cmr_pose_graph_linearize_f64", _p(poses), F, _p(edges), _p(meas), _p(weights), E, huber, _p(r), _p(chi), _p(scale), _p(A), _p(b),
              _p(cost), _p(wide), _p(ws), nb, _stream())
    return PoseGraphTerms(r, chi, scale, A, b, float(cost.cpu()[0]), int(wide.cpu()[0]))


def pose_graph_optimize(poses, edges, meas, weights, fixed=None, huber=0.0, iters=20, cg_iters=200, cg_tol=1e-8, damping=0.0, tol_rot=1e-9,
                        tol_trans=1e-9):
    """Gauss-Newton over a pose graph, the linear system by matrix-free preconditioned conjugate gradients, the whole loop on the device
    (cmr_pose_graph_optimize_f64; the contract is the header's).  Tensors as pose_graph_linearize's; fixed bool [F]: the poses that do not
    move (default: pose 0 alone).  huber: edges with chi above it are down-weighted by huber / chi (0: off); damping is added to H's
    diagonal.  The launch count depends on (iters, cg_iters) alone; the result is read once at the end.  -> PoseGraphResult.  E = 0 or
    F = 1 returns the poses unchanged with status 0 and no launch."""
    who = "pose_graph_optimize"
    huber = _f32_arg(who, "huber", huber, "be a finite number >= 0", as_f32=False, bools=False)
    iters = _int_arg(who, "iters", iters, 0, PG_MAX_ITERS)
    cg_iters = _int_arg(who, "cg_iters", cg_iters, 0, PG_MAX_CG_ITERS)
    cg_tol = _f32_arg(who, "cg_tol", cg_tol, "be a finite number >= 0", as_f32=False, bools=False)
    damping = _f32_arg(who, "damping", damping, "be a finite number >= 0", as_f32=False, bools=False)
    tol_rot = _f32_arg(who, "tol_rot", tol_rot, "be a finite number >= 0", as_f32=False, bools=False)
    tol_trans = _f32_arg(who, "tol_trans", tol_trans, "be a finite number >= 0", as_f32=False, bools=False)
    if fixed is None and torch.is_tensor(poses) and poses.dim() == 3 and poses.shape[0] > 1:
        fixed = torch.zeros((poses.shape[0],), dtype=torch.bool, device=poses.device)
        fixed[0] = True
    poses, edges, meas, weights, fixed, F, E = _pg_graph(who, poses, edges, meas, weights, fixed)
    dev = poses.device
    if E == 0 or F == 1:
        return PoseGraphResult(poses.clone(), 0.0, 0, 0, torch.zeros((iters, 5), dtype=torch.float64))
    _pg_on_gpu(who, poses)
    offsets, numbers, _ = pose_graph_incidence(edges, F)
    out = torch.empty((F, 4, 4), dtype=torch.float64, device=dev)
    cost = torch.empty((1,), dtype=torch.float64, device=dev)
    trace = torch.empty((iters, 5), dtype=torch.float64, device=dev)
    status = torch.empty((3,), dtype=torch.int32, device=dev)
    nb = _lib.load().cmr_pose_graph_optimize_workspace_bytes(F, E)
    ws = _ws(nb, dev)
    _lib.call("cmr_pose_graph_optimize_f64", _p(poses), F, _p(edges), _p(meas), _p(weights), E, _p(offsets), _p(numbers), _p(fixed), huber, iters,
              cg_iters, cg_tol, damping, tol_rot, tol_trans, _p(out), _p(cost), _p(trace), _p(status), _p(ws), nb, _stream())
    code, executed, _ = (int(v) for v in status.cpu())                  # the one host read (cost and trace ride behind it)
    return PoseGraphResult(out, float(cost.cpu()[0]), executed, code, trace.cpu())


# ---- range images and virtual scans of a cloud from a sensor pose (csrc/range_image.hip) --------------------------------------
RANGE_MAX_ROWS = 128
RANGE_MAX_COLS = 4096
RANGE_MAX_CELLS = 1 << 19           # rows x cols of a range image
RANGE_MAX_WINDOW = 1024             # cells range_visible reads round one cell, after clipping to the image


class RangeImage(collections.namedtuple("RangeImage", "index dist2 binned dropped outside")):
    """range_image's result: index int32 [rows, cols] = per cell the input row nearest to the sensor, -1 where the cell is empty; dist2
    float32 [rows, cols] = its squared distance, NaN where empty; binned = rows that fell into a cell, dropped = rows with a non-finite
    coordinate before or after the pose, outside = finite rows out of range or out of the field of elevation.  The three sum to the
    cloud's rows.  Image row 0 is the lowest elevation; column 0 starts at the x axis and the columns turn towards y."""


class VirtualScan(collections.namedtuple("VirtualScan", "rows image visible")):
    """virtual_scan's result: rows int64 [k] = the input row numbers of the visible winners, ascending; image = the RangeImage;
    visible bool [rows, cols] = range_visible of it."""


def _range_shape(who, rows, cols):
    return _azimuth_shape(who, ("rows", "cols"), (rows, cols), (RANGE_MAX_ROWS, RANGE_MAX_COLS, RANGE_MAX_CELLS))


def range_tables(rows, cols, elev_lo, elev_hi):
    """The two tables cmr_range_image_f32 reads, computed in float64 and rounded to float32 (numpy): elev [rows + 1, 2] = (sign(tan e_j),
    tan^2 e_j) of the edge angles e_j = elev_lo + (elev_hi - elev_lo) j / rows, col_dir [cols / 4 - 1, 2] = (cos, sin) of the column edges
    inside the first quadrant (scan_tables' sector_dir).  Angles in radians, -pi/2 < elev_lo < elev_hi < pi/2."""
    who = "range_tables"
    rows, cols = _range_shape(who, rows, cols)
    try:
        lo, hi = float(elev_lo), float(elev_hi)
        ok = not isinstance(elev_lo, bool) and not isinstance(elev_hi, bool) and -math.pi / 2 < lo < hi < math.pi / 2
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s: need -pi/2 < elev_lo < elev_hi < pi/2 in radians, got %r and %r" % (who, elev_lo, elev_hi))
    t = np.tan(lo + (hi - lo) * np.arange(rows + 1, dtype=np.float64) / rows)
    with np.errstate(over="ignore"):
        elev = np.stack([np.sign(t), t * t], 1).astype(np.float32)
    if not np.isfinite(elev).all():
        raise ValueError("%s: tan^2 of an edge angle is not finite in float32; keep elev_lo and elev_hi away from +-pi/2, got %r and %r" % (who, elev_lo, elev_hi))
    return elev, _azimuth_dirs(cols)


def _range_ranges(who, min_range, max_range):
    """-> (min_range2, max_range2): the squares formed in float64, with 0 < min_range2 < max_range2 < inf as float32"""
    max_range = _cloud_scalar(max_range, "max_range")
    min_range = _f32_arg(who, "min_range", min_range, "be a number in (0, max_range)", 0.0, lo_open=True, bools=False)
    with np.errstate(over="ignore", under="ignore"):
        lo2, hi2 = np.float32(min_range * min_range), np.float32(max_range * max_range)
    if not np.isfinite(hi2):
        raise ValueError("max_range must be a finite number > 0 whose square is finite in float32, got %r" % max_range)
    if not 0.0 < lo2 < hi2:
        raise ValueError("%s: min_range must be a number in (0, max_range), got %r with max_range %r" % (who, min_range, max_range))
    return float(lo2), float(hi2)


def range_image(points, pose=None, rows=64, cols=1024, elev_lo=-0.4363, elev_hi=0.0524, min_range=1.0, max_range=80.0):
    """The range image of a cloud seen from a sensor (cmr_range_image_f32; the contract is the header's): a spherical z-buffer of `rows`
    elevation rows between elev_lo and elev_hi (radians) and `cols` azimuth columns, each cell keeping the row nearest to the sensor among
    those between min_range and max_range.  points float32 [N, 3]; pose float32 [4, 4] or None: the rows are moved by it first, in fp32 --
    it maps the cloud's frame into the sensor's, whose origin is where the sensor stands.  -> RangeImage.  One host read: the three
    counts.  N = 0 gives the empty image and no launch.  The defaults (a 64-beam sensor's field, 1 m to 80 m) are not tuned on real data."""
    who = "range_image"
    rows, cols = _range_shape(who, rows, cols)
    elev, dirs = range_tables(rows, cols, elev_lo, elev_hi)
    min2, max2 = _range_ranges(who, min_range, max_range)
    points = _cloud_points(points)
    N, dev = points.shape[0], points.device
    pose = _cloud_pose(pose, dev, who)
    index = torch.empty((rows, cols), dtype=torch.int32, device=dev)
    dist2 = torch.empty((rows, cols), dtype=f32, device=dev)
    if N == 0:
        return RangeImage(index.fill_(-1), dist2.fill_(float("nan")), 0, 0, 0)
    elev, dirs = torch.from_numpy(elev).to(dev), torch.from_numpy(dirs).to(dev)
    counts = torch.empty((3,), dtype=torch.int64, device=dev)
    nb = _lib.load().cmr_range_image_workspace_bytes(rows, cols)
    ws = _ws(nb, dev)
    _lib.call("cmr_range_image_f32", _p(points), 3, N, _p(pose), rows, cols, _p(elev), _p(dirs) if cols > 4 else None, min2, max2, _p(index),
              _p(dist2), _p(counts), _p(ws), nb, _stream())
    return RangeImage(index, dist2, *(int(v) for v in counts.cpu()))


def _range_window(who, radius, rel_tol, rows, cols):
    """-> (radius_rows, radius_cols, factor): the window's reach, clipped to the image, and fp32((1 + rel_tol)^2) formed in float64"""
    try:
        rr, rc = radius
    except (TypeError, ValueError):
        raise ValueError("%s: radius must be two integers (rows, cols), got %r" % (who, radius))
    rr = min(_int_arg(who, "radius[0]", rr, 0, 1 << 30), rows)
    rc = min(_int_arg(who, "radius[1]", rc, 0, 1 << 30), cols)
    if min(2 * rr + 1, rows) * min(2 * rc + 1, cols) > RANGE_MAX_WINDOW:
        raise ValueError("%s: the window of radius %r holds more than %d cells of a %d x %d image" % (who, tuple(radius), RANGE_MAX_WINDOW, rows, cols))
    rel_tol = _f32_arg(who, "rel_tol", rel_tol, "be a finite number >= 0", as_f32=False, bools=False)
    with np.errstate(over="ignore"):
        factor = float(np.float32((1.0 + rel_tol) ** 2)) if rel_tol < 1e150 else math.inf
    if not factor < math.inf:
        raise ValueError("%s: rel_tol must be a finite number >= 0 with (1 + rel_tol)^2 finite in float32, got %r" % (who, rel_tol))
    return rr, rc, factor


def range_visible(dist2, radius=(1, 1), rel_tol=0.05):
    """Which cells of a range image a sensor sees (cmr_range_visible_f32; the contract is the header's): a cell with a winner is visible
    when its squared distance is at most (1 + rel_tol)^2 times the least one in the window of `radius` = (rows, cols) cells round it --
    image rows clipped at the border, columns wrapped -- which stops far surfaces leaking through the gaps between near rows.  dist2
    float32 [rows, cols] as range_image gives it (NaN = empty) -> bool [rows, cols].  radius (0, 0) keeps every winner.  The defaults are
    not tuned on real data."""
    who = "range_visible"
    if not isinstance(dist2, torch.Tensor) or dist2.dtype != f32 or dist2.dim() != 2:
        raise ValueError("%s: dist2 must be a float32 [rows, cols] tensor, got %s %s" % ((who,) + _got(dist2)))
    rows, cols = _range_shape(who, dist2.shape[0], dist2.shape[1])
    rr, rc, factor = _range_window(who, radius, rel_tol, rows, cols)
    if not dist2.is_cuda:
        raise ValueError("%s: dist2 must be a device tensor (there is no CPU path)" % who)
    dist2 = dist2.contiguous()
    visible = torch.empty((rows, cols), dtype=torch.uint8, device=dist2.device)
    _lib.call("cmr_range_visible_f32", _p(dist2), rows, cols, rr, rc, factor, _p(visible), _stream())
    return visible.view(torch.bool)


def virtual_scan(points, pose=None, rows=64, cols=1024, elev_lo=-0.4363, elev_hi=0.0524, min_range=1.0, max_range=80.0, radius=(1, 1),
                 rel_tol=0.05):
    """What a spinning LiDAR standing at `pose` would see of a cloud: range_image, then range_visible of it, then the visible winners'
    row numbers in ascending order (torch glue over the two ops) -> VirtualScan.  It depends on where the sensor stands, not on its heading,
    save for which rows sit on a cell edge.  Arguments as the two ops'; every default is untuned on real data."""
    who = "virtual_scan"
    rows, cols = _range_shape(who, rows, cols)
    _range_window(who, radius, rel_tol, rows, cols)                     # ahead of the first launch
    image = range_image(points, pose, rows, cols, elev_lo, elev_hi, min_range, max_range)
    if image.binned == 0:                                               # an empty image: nothing is visible, and no second launch
        return VirtualScan(torch.empty((0,), dtype=torch.int64, device=image.index.device), image, torch.zeros_like(image.index, dtype=torch.bool))
    visible = range_visible(image.dist2, radius, rel_tol)
    return VirtualScan(torch.sort(image.index[visible].to(torch.int64)).values, image, visible)
