"""GPU tier of pose scoring by mutual information (ops.pose_mi / cmr_pose_mi_f32, MultiHeadModel.score_poses_mi, Test_Geo.py /
Test_Agent.py --verify-mi).

The defining test holds ops.pose_mi to the path that existed before it: per pose ops.paint_points at C = 1 in the same mode, the bin
formula in fp32 torch and torch.bincount.  Both sides run the same fp32 arithmetic and every sum is an integer, so hist, counts and
selected are equal EXACTLY.  entropy and mi are held to numpy float64 computed from the device's own hist: a float64 sum in a different
order, |difference| <= 1e-10 on values <= ln 4096 (4q's bar).  The float64 restatement (pose_mi_reference.py) is the second yardstick:
there the rows on which an fp32 evaluation may decide differently (`near`; capped at 16 per (sample, pose) on the scenes used) may each
move one count from a cell to another."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pose_mi_reference as pmr
from cmr_agent_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)      # noqa: E731
SLICE = ops.POSE_MI_SLICE
RANGES = dict(attr_range=(0.0, 1.0), grey_range=(0.0, 1.0))

_SCENES = {}


def _scene(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _SCENES:
        _SCENES[key] = pmr.equality_scene(**kw)
    return _SCENES[key]


def _args(sc, empty=None, P=None):
    """-> (pts, attr, grey, mask, poses, K) on the device; `empty`: the sample whose mask selects nothing."""
    mask = torch.from_numpy(sc["mask"].copy())
    if empty is not None:
        mask[empty] = False
    poses = sc["poses"]
    if P is not None:                                                    # P >= 3 keeps the pose behind the camera and the NaN pose
        poses = poses[:, :P] if P < 3 else np.concatenate([poses[:, :P - 2], poses[:, -2:]], 1)
    return F(sc["pts"]), F(sc["attr"]), F(sc["grey"]), mask.to(DEV), F(poses), F(sc["K"])


def _composition(a, nb, mode, attr_range=(0.0, 1.0), grey_range=(0.0, 1.0)):
    """What the tree offered before: P x (ops.paint_points at C = 1, the bins in fp32 torch, torch.bincount) -> (hist, counts, selected)."""
    pts, attr, grey, mask, poses, K = a
    B, _, N = pts.shape
    f32 = lambda v: float(np.float32(v))                                  # noqa: E731
    a_lo, g_lo = f32(attr_range[0]), f32(grey_range[0])
    a_scale = f32(nb / (f32(attr_range[1]) - a_lo))                       # in double, rounded once
    g_scale = f32(nb / (f32(grey_range[1]) - g_lo))
    binf = lambda x, lo, scale: ((x - lo) * scale).floor().clamp(0, nb - 1)      # noqa: E731  two rounded fp32 operations, then the clamp
    base = torch.arange(B, device=DEV)[:, None] * (nb * nb)
    hist, counts = [], []
    for p in range(poses.shape[1]):
        colors, painted, cnt, _ = ops.paint_points(pts, poses[:, p].contiguous(), K, grey[:, None].contiguous(), mask=mask, mode=mode)
        g, view = colors[:, 0], painted.view(B, N)
        ok = view & torch.isfinite(attr) & torch.isfinite(g)
        zero = torch.zeros_like(g)
        cell = base + (binf(torch.where(ok, attr, zero), a_lo, a_scale) * nb + binf(torch.where(ok, g, zero), g_lo, g_scale)).long()
        hist.append(torch.bincount(cell[ok], minlength=B * nb * nb).view(B, nb, nb))
        counts.append(torch.stack([cnt[:, 1].long(), ok.sum(1)], 1))
        selected = cnt[:, 0]
    return torch.stack(hist, 1).int(), torch.stack(counts, 1).int(), selected


def _entropy64(hist):
    h = hist.cpu().numpy()
    ent, mi = np.zeros(h.shape[:2] + (3,)), np.zeros(h.shape[:2])
    for b in range(h.shape[0]):
        for p in range(h.shape[1]):
            ent[b, p, 0], ent[b, p, 1], ent[b, p, 2], mi[b, p] = pmr.entropies(h[b, p])
    return ent, mi


def _check_against_composition(a, nb, mode, ranges=RANGES):
    mi, ent, counts, selected, hist = ops.pose_mi(*a, bins=nb, mode=mode, want_hist=True, **ranges)
    h0, c0, s0 = _composition(a, nb, mode, **ranges)
    assert hist.dtype == torch.int32 and tuple(hist.shape) == tuple(h0.shape) and counts.dtype == torch.int32 and selected.dtype == torch.int32
    assert torch.equal(hist, h0), int((hist != h0).sum())
    assert torch.equal(counts, c0) and torch.equal(selected, s0)
    assert torch.equal(hist.sum((2, 3)), counts[..., 1])
    e64, m64 = _entropy64(hist)
    de, dm = np.abs(ent.cpu().numpy() - e64).max(), np.abs(mi.cpu().numpy() - m64).max()
    print("nb", nb, mode, "B N P", a[0].shape[0], a[0].shape[2], a[4].shape[1], "image", tuple(a[2].shape[1:]), "counted", int(counts[..., 1].sum()),
          "max |entropy - float64|", de, "max |mi - float64|", dm)
    assert mi.dtype == torch.float64 and ent.dtype == torch.float64 and de <= 1e-10 and dm <= 1e-10
    return mi, ent, counts, selected, hist


# ---- 1. against the existing path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("nb", [2, 16, 64])
def test_equals_paint_points_binned(nb, mode):
    """B = 3 with the mask of sample 1 empty, P = 19 with a pose behind the camera and a NaN pose, NaN and +-inf attributes, values
    below lo and above hi, N = PMI_SLICE + 1: two row slices, so the global atomics run."""
    a = _args(_scene(B=3, N=SLICE + 1, H=37, W=61, seed=401), empty=1)
    mi, ent, counts, selected, hist = _check_against_composition(a, nb, mode)
    assert selected[1].item() == 0 and counts[1].abs().sum().item() == 0 and hist[1].abs().sum().item() == 0
    assert mi[1].abs().sum().item() == 0 and ent[1].abs().sum().item() == 0
    assert counts[:, -2:].abs().sum().item() == 0 and mi[:, -2:].abs().sum().item() == 0      # behind the camera, NaN
    assert counts[0, 0, 0].item() - 3 == counts[0, 0, 1].item() > 1000                    # in view, not counted: the three non-finite attributes
    assert hist[0, 0, 0].sum().item() > 0 and hist[0, 0, -1].sum().item() > 0 and hist[0, 0, :, 0].sum().item() > 0      # the end bins are used


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("hw", [(1, 1), (1, 40), (40, 1)])
def test_degenerate_maps(hw, mode):
    a = _args(_scene(B=2, N=300, H=hw[0], W=hw[1], seed=402))
    _check_against_composition(a, 16, mode)


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("nb,P", [(32, 9), (64, 3), (33, 8), (5, 1)])
def test_chunk_edges_one_slice_and_other_ranges(nb, P, mode):
    """P = a chunk + 1 at nb = 32 (8 + 1) and nb = 64 (2 + 1); an odd nb whose chunk is 7 and whose hist is no multiple of 16 bytes per
    pose; N <= PMI_SLICE: one slice, the plain stores.  Ranges other than the unit one, an int64 mask."""
    sc = _scene(B=2, N=1000, H=37, W=61, seed=403)
    a = list(_args(sc, P=P))
    assert ops.pose_mi_chunk(32) == 8 and ops.pose_mi_chunk(64) == 2 and ops.pose_mi_chunk(33) == 7
    _check_against_composition(a, nb, mode)
    a[3] = a[3].long() * 5
    _check_against_composition(a, nb, mode, dict(attr_range=(-0.25, 1.5), grey_range=(0.1, 0.7)))
    a[3] = None
    h_all = ops.pose_mi(*a, bins=nb, mode=mode, want_hist=True)
    a[3] = torch.ones(2, 1000, dtype=torch.uint8, device=DEV)
    h_one = ops.pose_mi(*a, bins=nb, mode=mode, want_hist=True)
    assert all(torch.equal(x, y) for x, y in zip(h_all, h_one)) and ops.pose_mi(*a, bins=nb, mode=mode)[4] is None


def test_hand_checked_scene():
    for kind in ("dependent", "independent"):
        s = pmr.hand_scene(kind)
        mi, ent, counts, selected, hist = ops.pose_mi(F(s["pts"]), F(s["attr"]), F(s["grey"]), None, F(s["pose"]), F(s["K"]), bins=2, want_hist=True)
        assert hist[0, 0].tolist() == s["hist"].tolist() and counts.tolist() == [[[6, 6]]] and selected.tolist() == [6]
        want = math.log(2.0) if kind == "dependent" else 0.0
        assert abs(mi.item() - want) <= 1e-12


# ---- 2. against the float64 restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("nb", [16, 64])
def test_against_float64(nb, mode):
    sc = _scene(**pmr.FLOAT64_SCENE)
    ref = pmr.pose_mi(sc["pts"], sc["attr"], sc["grey"], sc["mask"], sc["poses"], sc["K"], bins=nb, mode=mode)
    mi, ent, counts, selected, hist = ops.pose_mi(*_args(sc), bins=nb, mode=mode, want_hist=True)
    dh = np.abs(hist.cpu().numpy().astype(np.int64) - ref["hist"]).sum((2, 3))
    dc = np.abs(counts.cpu().numpy().astype(np.int64) - ref["counts"])
    print("nb", nb, mode, "max near", int(ref["near"].max()), "max sum |hist - hist64|", int(dh.max()), "max count deviation", int(dc.max()),
          "max |mi - mi64|", np.abs(mi.cpu().numpy() - ref["mi"]).max())
    assert int(ref["near"].max()) <= pmr.NEAR_CAP
    assert selected.cpu().tolist() == ref["selected"].tolist()
    assert (dh <= 2 * ref["near"]).all() and (dc <= ref["near"][..., None]).all()


# ---- 3. ranking -------------------------------------------------------------------------------------------------------------------------
def _model():
    from cmr_agent_amd.models import MultiHeadModel
    return MultiHeadModel.__new__(MultiHeadModel)                         # score_poses_mi uses no weights


_RANK = {}


def _rank():
    if not _RANK:
        sc = [pmr.ranking_scene(s) for s in (301, 302, 303)]
        _RANK["v"] = {k: np.concatenate([s[k] for s in sc]) for k in sc[0]}
    return _RANK["v"]


@pytest.mark.parametrize("nb", [16, 32])
def test_truth_ranks_first(nb):
    """tests/test_pose_mi_cpu.py asserts on these scenes that the truth leads by more than the near rows can move the MI."""
    s = _rank()
    mi = ops.pose_mi(F(s["pts"]), F(s["attr"]), F(s["grey"]), None, F(s["poses"]), F(s["K"]), bins=nb)[0]
    print("nb", nb, "truth", mi[:, 0].tolist(), "runner-up", mi[:, 1:].max(1).values.tolist())
    assert mi.argmax(1).tolist() == [0, 0, 0]
    data = {"pc": F(s["pts"]), "pc_intensity": F(s["attr"]), "img": F(s["grey"])[:, None].contiguous()}
    _model().score_poses_mi(data, F(s["poses"]), K=F(s["K"]), bins=nb, attr_range=(0.0, 1.0))
    assert data["pose_mi_best"].dtype == torch.int64 and data["pose_mi_best"].tolist() == [0, 0, 0]
    assert torch.equal(data["pose_mi"], mi) and tuple(data["pose_mi_entropy"].shape) == (3, 9, 3) and tuple(data["pose_mi_counts"].shape) == (3, 9, 2)
    ent = data["pose_mi_entropy"]
    assert torch.equal(data["pose_nmi"], (ent[..., 0] + ent[..., 1]) / ent[..., 2])
    # the default attribute range (the batch's own extremes, taken on the device) ranks the same
    _model().score_poses_mi(data, F(s["poses"]), K=F(s["K"]), bins=nb)
    assert data["pose_mi_best"].tolist() == [0, 0, 0]


def test_min_in_view_turns_a_planted_pose_down():
    """Three extra points 100 m to the side, one per grey block with the attribute of its block, and a pose that looks at them alone:
    3 rows in view, each in a cell of its own, MI = ln 3 -- more than the two wrong poses it competes with, and it must lose."""
    s = pmr.ranking_scene(301)
    Kd, grey = s["K"][0].astype(np.float64), s["grey"][0]
    px = np.array([[4.0, 4.0], [60.0, 20.0], [100.0, 36.0]])
    lv = np.array([0.1, 0.5, 0.9], np.float32)
    grey = grey.copy()
    for (x, y), v in zip(px, lv):
        grey[int(y) // 8 * 8:int(y) // 8 * 8 + 8, int(x) // 8 * 8:int(x) // 8 * 8 + 8] = v
    z = 10.0
    cam = np.stack([(px[:, 0] - Kd[0, 2]) / Kd[0, 0] * z, (px[:, 1] - Kd[1, 2]) / Kd[1, 1] * z, np.full(3, z)])
    planted = np.eye(4)
    planted[0, 3] = -1000.0                                              # camera frame = cloud frame moved 1000 m along x
    extra = cam + np.array([[1000.0], [0.0], [0.0]])
    pts = np.concatenate([s["pts"][0], extra.astype(np.float32)], 1)[None]
    attr = np.concatenate([s["attr"][0], lv])[None]
    poses = np.stack([s["poses"][0, 3], s["poses"][0, 8], planted.astype(np.float32)])[None]      # yaw -2 degrees, z + 1.5, the planted one
    a = (F(pts), F(attr), F(grey[None]), None, F(poses), F(s["K"]))
    mi, _, counts, selected, _ = ops.pose_mi(*a, bins=16)
    print("mi", mi.tolist(), "counts", counts.tolist(), "selected", selected.tolist())
    assert counts[0, 2].tolist() == [3, 3] and abs(mi[0, 2].item() - math.log(3.0)) <= 1e-12 and mi[0, 2] > mi[0, :2].max()
    data = {"pc": a[0], "pc_intensity": a[1], "img": a[2][:, None].contiguous()}
    _model().score_poses_mi(data, a[4], K=a[5], bins=16, attr_range=(0.0, 1.0))
    assert data["pose_mi_best"].tolist() == [0]
    _model().score_poses_mi(data, a[4], K=a[5], bins=16, attr_range=(0.0, 1.0), min_in_view=0.0)
    assert data["pose_mi_best"].tolist() == [2]


# ---- 4. determinism ---------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(x, y):
    return all(torch.equal(_bits(u), _bits(v)) for u, v in zip(x, y))


def _det_args():
    return _args(_scene(B=3, N=SLICE + 1, H=37, W=61, seed=401))


def _call(a, **kw):
    return ops.pose_mi(*a, bins=32, mode="bilinear", want_hist=True, **kw)


def test_two_calls_agree_bit_for_bit():
    a = _det_args()
    assert _same(_call(a), _call(a))


def test_pose_alone_equals_pose_in_batch():
    a = _det_args()
    mi, ent, counts, selected, hist = _call(a)
    for p in (0, 7, 8, 16, 18):                                           # chunk starts, chunk ends and the last pose
        o = _call(a[:4] + (a[4][:, p:p + 1].contiguous(), a[5]))
        assert _same((o[0][:, 0], o[1][:, 0], o[2][:, 0], o[3], o[4][:, 0]), (mi[:, p], ent[:, p], counts[:, p], selected, hist[:, p]))


def test_sample_alone_equals_sample_in_batch():
    a = _det_args()
    full = _call(a)
    for k in range(a[0].shape[0]):
        o = _call(tuple(t[k:k + 1].contiguous() for t in a))
        assert _same(tuple(t[0] for t in o), tuple(t[k] for t in full))


def test_graph_replay_equals_eager():
    a = _det_args()
    fn = lambda: _call(a)                                                 # noqa: E731
    eager = fn()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        fn()
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = fn()
    for t in got:
        t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(eager, got)


# ---- 5. the scripts ---------------------------------------------------------------------------------------------------------------------
def _write_dataset(root):
    """Two frames of sequence 09 in the reference's on-disk layout (tests/test_loader.py's helper): 200 x 340 images, whose half size
    holds the 96 x 160 crop, the smallest image the scripts' tests feed the geometric model, and [4, n] clouds with reflectance."""
    from test_pose_mi_cpu import _write_dataset as write
    write(root, seqs=(9,), frames=2, with_image_3=False, n_raw=6000, img_hw=(200, 340))


def _run(script, root, *flags, code=0):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    cmd = [sys.executable, os.path.join(ROOT, script), "--pairs", "2", "--img", "96x160", "--num-pt", "10240", *flags]
    res = subprocess.run(cmd + (["--data-root", root] if root else []), cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == code, res.stderr[-3000:]
    return res.stdout.strip().splitlines() if code == 0 else res.stderr


_NUM = re.compile(r"[-+]?(?:\d+\.?\d*(?:[eE][-+]?\d+)?|nan|inf)")


def _shape(lines):
    """The format of an output: every number replaced by '#' (the loader's draws are not seeded, so two runs differ in the figures)."""
    return [_NUM.sub("#", l) for l in lines]


def _check_mi(lines, plain, names, blocks):
    mi = [l for l in lines if l.startswith("mi ")]
    assert len(mi) == 2                                                   # one line per pair
    for l in mi:
        tok = l.split()
        assert [t.split("=")[0] for t in tok[1:-2]] == names and tok[-2] == "->" and tok[-1] in names
        assert all(math.isfinite(float(t.split("=")[1])) and float(t.split("=")[1]) >= -1e-9 for t in tok[1:-2])
    heads = [l.split(":")[0] for l in lines if "Registration Recall:" in l]
    assert heads == ["Registration Recall"] + [p + " Registration Recall" for p in blocks]
    # without the flag: the format the parent prints, line for line
    rest = [l for l in lines if not l.startswith("mi ") and not l.startswith("MI-verified ")]
    assert _shape(rest) == _shape(plain)
    assert not any(l.startswith("mi ") or "MI-verified" in l for l in plain)


def test_test_geo_script_verify_mi(tmp_path):
    root = str(tmp_path)
    _write_dataset(root)
    lines = _run("Test_Geo.py", root, "--pnp", "--guided", "4,2", "--verify-mi", "--mi-bins", "16")
    plain = _run("Test_Geo.py", root, "--pnp", "--guided", "4,2")
    _check_mi(lines, plain, ["pnp", "refined"], ["Refined", "MI-verified"])
    assert "--verify-mi" in _run("Test_Geo.py", None, "--pnp", "--verify-mi", code=2)              # synthetic pairs: refused
    assert "--verify-mi" in _run("Test_Geo.py", root, "--verify-mi", code=2)                       # without --pnp


def test_test_agent_script_verify_mi(tmp_path):
    root = str(tmp_path)
    _write_dataset(root)
    lines = _run("Test_Agent.py", root, "--refine", "4,2", "--verify-mi")
    plain = _run("Test_Agent.py", root, "--refine", "4,2")
    _check_mi(lines, plain, ["agent", "refined"], ["Refined", "MI-verified"])
