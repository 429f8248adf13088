"""GPU tier of the geometric heads' loss kernels (csrc/losses.hip, csrc/train_geo.hip, csrc/agent.hip): the focal overlap loss with its
metrics and its backward, the circle loss forward (every row and column term, then the scalar) and backward (into live gradient buffers),
and the descriptor normalisation, case by case against the float64 restatement in loss_reference.py.  tests/test_loss_cpu.py proves that
restatement against the oracle, asserts what each case reaches, and pins every bar used here to four times the fp32 oracle's own error.
Each test prints its figure before it asserts."""
import functools

import numpy as np
import pytest
import torch

import loss_reference as lr

pytestmark = pytest.mark.gpu
DEV = "cuda"
PARAMS = {"product": lr.PRODUCT_PARAMS, "other": lr.OTHER_PARAMS}
FWD_ALL = [(c, "product") for c in lr.CIRCLE_FWD_CASES] + [(c, "other") for c in lr.CIRCLE_FWD_OTHER]
BWD_ALL = ([(c + (None,), "product") for c in lr.CIRCLE_BWD_CASES] + [(c + (None,), "other") for c in lr.CIRCLE_BWD_OTHER] +
           [(c, "product") for c in lr.CIRCLE_BWD_SPECIAL])
_id = lambda v: "-".join(str(x) for x in v[0]) + "-" + v[1]


@pytest.fixture(scope="module")
def ops():
    from cmr_agent_amd import ops as _ops
    return _ops


def within(name, err, bar):
    print("%s: error %.3g, bar %.3g" % (name, err, bar))
    assert err <= bar, "%s: error %.3g above the bar %.3g" % (name, err, bar)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.array_equal(a, b, equal_nan=True)


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def check_metrics(got, counts, rows, B):
    """got: the kernel's (precision, recall, accuracy); counts: the reference's integers"""
    prec, rec, acc = lr.focal_metrics(counts, rows, B)
    assert same_bits(got[0], prec) and same_bits(got[1], rec), (got, prec, rec, counts)
    assert ulps(got[2], acc) <= 2, (got[2], acc)


def padded(z, ld):
    """the [rows, 2] logits as the kernels see them: contiguous (ld = 2) or the first two columns of the product's 4-wide rows"""
    if ld == 2:
        return z.to(DEV)
    buf = torch.full((z.shape[0], ld), 9.0, device=DEV)
    buf[:, :2] = z.to(DEV)
    return buf[:, :2]


@functools.lru_cache(maxsize=None)
def focal_ref(rows, alpha):
    z, lab = lr.focal_sweep() if rows == "sweep" else lr.focal_rows(rows)
    return lr.focal(z, lab, alpha)


# ---- focal forward and metrics -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", lr.FOCAL_ALPHAS)
def test_focal_row_sweep_one_launch_per_row(ops, alpha):
    """every logit difference from a tie to softmax = exactly 0 / 1 in fp32, both signs, both labels, three base offsets: nothing diluted"""
    z, lab = lr.focal_sweep()
    ref = focal_ref("sweep", alpha)
    zd, ld_ = z.to(DEV), lab.to(DEV)
    got = torch.stack([ops.focal_metrics(zd[i:i + 1], ld_[i:i + 1], alpha, 1) for i in range(z.shape[0])]).cpu()
    assert torch.isfinite(got[:, 0]).all()
    pred, one = ref["pred"], (lab != 0).long()
    for i in range(z.shape[0]):
        p, l = int(pred[i]), int(one[i])
        check_metrics(got[i, 1:].numpy(), (p & l, p, l, int(p == l)), 1, 1)
    worst = int(((got[:, 0].double() - ref["row"]).abs() / ref["row"]).argmax())
    print("worst row: logits %s label %d" % (z[worst].tolist(), int(lab[worst])))
    within("focal per-row loss, alpha %g" % alpha, lr.rel_err(got[:, 0], ref["row"]), lr.FOCAL_ROW_BAR)


@pytest.mark.parametrize("ld", [2, 4])
@pytest.mark.parametrize("rows,B", lr.FOCAL_SHAPES)
def test_focal_forward_shapes(ops, rows, B, ld):
    """one row, either side of one workgroup, several workgroups with a ragged tail, B > 1, and the grid-stride loop's second trip"""
    z, lab = lr.focal_rows(rows)
    ref = focal_ref(rows, 0.75)
    got = ops.focal_metrics(padded(z, ld), lab.to(DEV), 0.75, B).cpu().numpy()
    check_metrics(got[1:], ref["counts"], rows, B)
    within("focal mean, rows %d" % rows, lr.rel_err(got[0], ref["mean"]), lr.FOCAL_ROW_BAR if rows == 1 else lr.FOCAL_MEAN_BAR)


@pytest.mark.parametrize("name", lr.FOCAL_METRIC_CASES)
def test_focal_metrics_edge_cases(ops, name):
    """0 / 0 precision and recall are NaN as in the reference, a tie predicts class 0"""
    z, lab = lr.focal_metric_case(name)
    ref = lr.focal(z, lab, 0.5)
    got = ops.focal_metrics(z.to(DEV), lab.to(DEV), 0.5, 1).cpu().numpy()
    check_metrics(got[1:], ref["counts"], z.shape[0], 1)
    within("focal mean, %s" % name, lr.rel_err(got[0], ref["mean"]), lr.FOCAL_MEAN_BAR)


# ---- focal backward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad_scale", [1.0, 0.37])
@pytest.mark.parametrize("rows", ["sweep"] + list(lr.FOCAL_BWD_ROWS))
@pytest.mark.parametrize("alpha", lr.FOCAL_ALPHAS)
def test_focal_backward(ops, alpha, rows, grad_scale):
    z, lab = lr.focal_sweep() if rows == "sweep" else lr.focal_rows(rows)
    ref = focal_ref(rows, alpha)
    got = ops.focal_bwd(padded(z, 4), lab.to(DEV), alpha, grad_scale).cpu()
    assert got.shape == (z.shape[0], 4) and (got[:, 2:] == 0).all()
    gs = lr.f32(grad_scale)
    within("focal gradient, rows %s" % rows, lr.scaled_err(got[:, :2], gs * ref["grad"], alpha * gs / z.shape[0]), lr.FOCAL_GRAD_BAR)


@pytest.mark.parametrize("value", [2, -1])
def test_focal_reads_any_non_zero_label_as_class_1_forward_and_backward(ops, value):
    z, lab = lr.focal_rows(257)
    zd = z.to(DEV)
    ones, odd = torch.ones_like(lab).to(DEV), torch.full_like(lab, value).to(DEV)
    ref = lr.focal(z, torch.ones_like(lab), 0.75)
    f1, fv = ops.focal_metrics(zd, ones, 0.75, 1).cpu(), ops.focal_metrics(zd, odd, 0.75, 1).cpu()
    b1, bv = ops.focal_bwd(zd, ones, 0.75).cpu(), ops.focal_bwd(zd, odd, 0.75).cpu()
    assert torch.equal(f1, fv) and torch.equal(b1, bv), "label %d is label 1 to both kernels" % value
    within("focal mean, label %d" % value, lr.rel_err(fv[0], ref["mean"]), lr.FOCAL_MEAN_BAR)
    within("focal gradient, label %d" % value, lr.scaled_err(bv[:, :2], ref["grad"], 0.75 / 257), lr.FOCAL_GRAD_BAR)
    # mixed labels: each row follows its own label's rule
    mixed = lab.clone()
    mixed[lab != 0] = value
    want = lr.focal(z, lab, 0.75)
    within("focal gradient, labels {0, %d}" % value, lr.scaled_err(ops.focal_bwd(zd, mixed.to(DEV), 0.75).cpu()[:, :2], want["grad"], 0.75 / 257),
           lr.FOCAL_GRAD_BAR)


# ---- circle forward ------------------------------------------------------------------------------------------------------------------------
def _dev(c):
    return [c[k].to(DEV) for k in ("pc", "img", "pc_idx", "xy_int", "xy_float")]


def _args(pname):
    P = PARAMS[pname]
    return [P[k] for k in ("dist_thres", "pos_margin", "neg_margin", "log_scale")]


@pytest.mark.parametrize("case,pname", FWD_ALL, ids=map(_id, FWD_ALL))
def test_circle_forward_every_term_then_the_scalar(ops, case, pname):
    c = lr.circle_case(*case)
    ref = lr.circle_forward(c, PARAMS[pname])
    terms = []
    got = ops.circle_loss(*_dev(c), c["B"], c["N"], *_args(pname), PARAMS[pname]["lam"], terms=terms)
    assert len(terms) == 1 and terms[0].shape == (c["B"], 2 * c["n"])
    t = terms[0].cpu()
    assert torch.isfinite(t).all()
    within("circle terms", lr.rel_err(t, ref["terms"]), lr.CIRCLE_TERM_BAR)
    within("circle loss", lr.rel_err(got.cpu(), ref["loss"]), lr.CIRCLE_LOSS_BAR)


# ---- circle backward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,pname", BWD_ALL, ids=map(_id, BWD_ALL))
def test_circle_backward_adds_the_closed_form_gradient_to_live_buffers(ops, case, pname):
    """d_pc / d_img arrive holding other gradients: the result is that pre-fill plus the reference gradient, rows no sample names keep
    their bits, a d = 0 pair gives a finite (zero) contribution, and a second call from the same pre-fill gives the same bits."""
    c = lr.circle_case(*case)
    gs = lr.bwd_grad_scale(case[0], case[1])
    ref = lr.circle_backward(c, PARAMS[pname], gs)
    pre = lr.circle_prefill(c, ref)
    dev = _dev(c)
    runs = []
    for _ in range(2):
        d_pc, d_img = pre[0].to(DEV), pre[1].to(DEV)
        ops.circle_loss_bwd(*dev, c["B"], c["N"], d_pc, d_img, *_args(pname), gs)
        runs.append((d_pc.cpu(), d_img.cpu()))
    (d_pc, d_img), again = runs
    assert torch.isfinite(d_pc).all() and torch.isfinite(d_img).all()
    assert torch.equal(d_pc[~ref["named_pc"]], pre[0][~ref["named_pc"]]) and torch.equal(d_img[~ref["named_img"]], pre[1][~ref["named_img"]])
    assert not torch.equal(d_pc, pre[0]) and not torch.equal(d_img, pre[1])
    within("circle d_pc", lr.circle_grad_err(d_pc, pre[0], ref["d_pc"]), lr.CIRCLE_GRAD_BAR)
    within("circle d_img", lr.circle_grad_err(d_img, pre[1], ref["d_img"]), lr.CIRCLE_GRAD_BAR)
    assert torch.equal(d_pc, again[0]) and torch.equal(d_img, again[1]), "a fixed summation order"


# ---- l2norm --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("rows", lr.L2NORM_ROWS)
def test_l2norm_forward_and_backward(ops, rows, strided):
    """row norms over 1e-6 ... 1e6 and an exactly-zero row (y = 0, dx = dy / 1e-12, both finite); strided: 64-column views of 128-column
    buffers for every operand; the backward's accumulate flag into a non-zero buffer"""
    x, dy = lr.l2norm_case(rows)
    ref = lr.l2norm(x, dy)
    scale = ref["scale"][:, None]

    def buf(t):
        if not strided:
            return t.to(DEV).clone()
        b = torch.full((rows, 128), 7.0, device=DEV)
        b[:, :64] = t.to(DEV)
        return b[:, :64]

    xd, dyd = buf(x), buf(dy)
    y = buf(torch.full((rows, 64), 5.0))
    assert ops.l2norm64(xd, out=y) is y
    within("l2norm y", lr.scaled_err(y.cpu(), ref["y"], 1.0), lr.L2NORM_FWD_BAR)
    dx = buf(torch.full((rows, 64), 5.0))
    ops.l2norm64_bwd(dyd, xd, out=dx, accumulate=False)
    assert torch.isfinite(dx).all()
    within("l2norm dx", lr.scaled_err(dx.cpu(), ref["dx"], scale), lr.L2NORM_BWD_BAR)
    pre = lr.prefill((rows, 64), 1.0, 77 + rows) * ref["scale"].float()[:, None]
    acc = buf(pre)
    ops.l2norm64_bwd(dyd, xd, out=acc, accumulate=True)
    within("l2norm dx, accumulated", lr.scaled_err(acc.cpu(), pre.double() + ref["dx"], scale), lr.L2NORM_BWD_BAR)
    if rows > 7:
        assert (y[7] == 0).all() and float(dx[7].abs().max()) > 1e10
    if strided:
        for t in (y, dx, acc, xd, dyd):
            assert (t._base[:, 64:] == 7.0).all(), "nothing written past the 64 columns"
    fresh = ops.l2norm64(xd)
    assert fresh.is_contiguous() and torch.equal(fresh, y)
