"""CPU tier of image-guided densification: the float64 restatement in densify_reference.py gives the values worked by hand
on a 3 x 5 scene (so the yardstick of the GPU tests is itself checked), the scenes of the GPU tier keep their undecided pixels under the
cap and their bound under 1e-3, ops.densify refuses malformed arguments before the library is touched, the C entry refuses what is
outside its contract, the PFM writer round-trips, MultiHeadModel.dense_depth hands on what it should and the scripts reject misplaced
flags."""
import importlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import densify_reference as dr
from cmr_agent_amd import _lib, ops
from cmr_agent_amd.utils import evalcli, pfm

mhm = importlib.import_module("cmr_agent_amd.models.MultiHeadModel")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement on the hand scene -------------------------------------------------------------------------------------------------------
def test_restatement_gives_the_hand_scene():
    depth = np.asarray([dr.HAND_DEPTH], dtype=np.float32)
    attr = np.asarray([[dr.HAND_ATTR]], dtype=np.float32)
    r = dr.densify(depth, None, attr, radius=1, sigma_s=dr.HAND_SIGMA_S, min_weight=1e-3, keep=True, fill=dr.HAND_FILL)
    assert r["count"][0].tolist() == dr.HAND_COUNT and r["counts"][0].tolist() == dr.HAND_COUNTS and r["undecided"] == 0
    assert np.allclose(r["conf"][0], dr.HAND_CONF, rtol=dr.HAND_TOL, atol=0)
    want = np.asarray(dr.HAND_DENSE)
    assert np.array_equal(np.isinf(r["depth"][0]), np.isinf(want))
    fin = np.isfinite(want)
    assert np.allclose(r["depth"][0][fin], want[fin], rtol=dr.HAND_TOL, atol=0)
    assert np.allclose(r["attr"][0, 0], dr.HAND_DENSE_ATTR, rtol=dr.HAND_TOL, atol=0)
    # the samples keep their own values exactly, with and without keep here (a lone weight of 1)
    for (y, x) in ((0, 0), (1, 2), (2, 4)):
        assert r["depth"][0, y, x] == dr.HAND_DEPTH[y][x] and r["attr"][0, 0, y, x] == dr.HAND_ATTR[y][x]
    # the window's extremes and the largest argument: (1, 1) sees 4 (diagonal: 2 ln 2) and 8 (edge: ln 2)
    assert r["zmin"][0, 1, 1] == 4.0 and r["zmax"][0, 1, 1] == 8.0 and abs(r["a_max"][0, 1, 1] - 2 * math.log(2)) < 1e-6
    assert math.isinf(r["zmin"][0, 0, 4]) and r["conf"][0, 0, 4] == 0.0
    # min_weight = 0.3: the pixels whose only sample is a diagonal neighbour (S0 = 1/4) are not filled
    r = dr.densify(depth, None, attr, radius=1, sigma_s=dr.HAND_SIGMA_S, min_weight=0.3, fill=dr.HAND_FILL)
    assert sorted(map(tuple, np.argwhere(~r["filled"][0]).tolist())) == dr.HAND_UNFILLED_AT_03 and r["counts"][0].tolist() == dr.HAND_COUNTS_AT_03
    assert all(math.isinf(r["depth"][0, y, x]) and r["attr"][0, 0, y, x] == dr.HAND_FILL for y, x in dr.HAND_UNFILLED_AT_03)


def test_restatement_without_keep_and_with_a_guide():
    depth = np.full((1, 1, 3), np.inf, dtype=np.float32)
    depth[0, 0, 0], depth[0, 0, 2] = 10.0, 20.0
    guide = np.asarray([[[[0.0, 0.0, 1.0]]]], dtype=np.float32)
    # no guide, keep off: pixel 0 hears pixel 2 at distance 2 (weight 1/16 with ln 2): (10 + 20 / 16) / (1 + 1 / 16)
    r = dr.densify(depth, None, None, radius=2, sigma_s=dr.HAND_SIGMA_S, keep=False)
    assert abs(r["depth"][0, 0, 0] - (10 + 20 / 16) / (1 + 1 / 16)) < 1e-5 and abs(r["depth"][0, 0, 1] - 15.0) < 1e-6
    r = dr.densify(depth, None, None, radius=2, sigma_s=dr.HAND_SIGMA_S, keep=True)
    assert r["depth"][0, 0, 0] == 10.0 and r["depth"][0, 0, 2] == 20.0
    # the guide steps between pixels 1 and 2: with sigma_r = 0.1 the far side's weight is e^-50 times smaller, pixel 1 belongs to pixel 0
    r = dr.densify(depth, guide, None, radius=2, sigma_s=dr.HAND_SIGMA_S, sigma_r=0.1, keep=False)
    assert abs(r["depth"][0, 0, 1] - 10.0) < 1e-15 * 1e6 and abs(r["depth"][0, 0, 0] - 10.0) < 1e-9
    assert abs(r["a_max"][0, 0, 1] - (math.log(2) + 1.0 / (2 * dr.f32(0.1) ** 2))) < 1e-6
    # 0, negatives, NaN and both infinities are not samples
    bad = np.asarray([[[0.0, -1.0, np.nan, np.inf, -np.inf, 3.0]]], dtype=np.float32)
    assert dr.is_sample(bad)[0, 0].tolist() == [False] * 5 + [True]


# ---- the cap and the size of the bound on the scenes the GPU tier uses -----------------------------------------------------------------------
@pytest.mark.parametrize("planes", dr.GUIDE_PLANES)
@pytest.mark.parametrize("name", dr.SCENE_NAMES)
def test_undecided_pixels_stay_under_the_cap(name, planes):
    r = dr.reference(name, planes)
    with_samples = int((r["count"] > 0).sum())
    print(name, "guide planes", planes, "pixels with samples", with_samples, "undecided", r["undecided"], "largest REL", float(r["rel"].max()),
          "largest argument", float(r["a_max"].max()), "filled", int(r["filled"].sum()), "of", r["filled"].size)
    assert with_samples > 0 and r["undecided"] <= dr.cap(with_samples)
    assert float(r["rel"].max()) < 1e-3                                           # above that the derivation would be wrong
    assert dr.reference_nokeep(name, planes)["undecided"] == r["undecided"]
    sc = dr.built(name)
    density = dr.is_sample(sc["depth"]).mean()
    assert 0.5 * dr.SCENES[name][2] < density < 1.5 * dr.SCENES[name][2] and sc["depth"].dtype == np.float32
    z = sc["depth"][dr.is_sample(sc["depth"])]
    assert 2.0 <= z.min() and z.max() <= 60.0 and np.isnan(sc["attr"][~np.broadcast_to(dr.is_sample(sc["depth"])[:, None], sc["attr"].shape)]).all()


# ---- ops.densify refuses before the library is touched --------------------------------------------------------------------------------------
def _touched(*a, **kw):
    raise AssertionError("the library was touched")


def test_constants():
    assert ops.DENSIFY_MAX_RADIUS == 16 and ops.DENSIFY_MAX_C == 4 and ops.DENSIFY_TILE_W == 64 and ops.DENSIFY_TILE_H == 16
    src = open(os.path.join(ROOT, "cmr_agent_amd", "csrc", "densify.hip")).read()
    for text in ("radius <= CMR_MAX_RADIUS", "DN_MAX_C = 4", "DN_TW = 64", "DN_TH = 16", "cmr_densify_f32"):
        assert text in src
    assert "constexpr int CMR_MAX_RADIUS = 16;" in open(os.path.join(ROOT, "cmr_agent_amd", "csrc", "cmr_project.h")).read()
    assert "not tuned on real data" in " ".join(ops.densify.__doc__.split()) and "NOT checked" in ops.densify.__doc__
    protos = _lib.parse_header()
    assert protos["cmr_densify_f32"][2] == ["depth", "attr", "C", "guide", "Cg", "B", "h", "w", "radius", "sigma_s", "sigma_r", "min_weight", "keep",
                                            "fill", "dense_depth", "dense_attr", "conf", "count", "counts", "stream"]
    assert "cmr_densify_workspace_bytes" not in protos                          # no workspace
    from cmr_agent_amd.utils import workmodel
    assert "cmr_densify_f32" in open(workmodel.__file__).read()


def test_densify_argument_checks(monkeypatch):
    monkeypatch.setattr(_lib, "load", _touched)
    monkeypatch.setattr(_lib, "call", _touched)
    depth = torch.ones(2, 4, 5)

    def refused(match, depth=depth, **kw):
        with pytest.raises(ValueError, match="^densify: " + match):
            ops.densify(depth, **kw)

    refused("depth must be", depth=depth[0])
    refused("depth must be", depth=None)
    refused("depth must be", depth=torch.ones(2, 1, 4, 5))
    refused("depth must be float32", depth=depth.double())
    refused("need 1 <= B", depth=torch.ones(2, 0, 5))
    refused("need 1 <= B", depth=torch.ones(0, 4, 5))
    refused("need 1 <= B", depth=torch.zeros(1).expand(1, 4097, 4096))            # shape only: 4 bytes of storage
    refused("need 1 <= B", depth=torch.zeros(1).expand(65536, 1, 1))
    for guide in (torch.ones(2, 4, 5), torch.ones(2, 3, 4, 5).double(), torch.ones(1, 3, 4, 5), torch.ones(2, 3, 5, 4), torch.ones(2, 5, 4, 5),
                  torch.ones(2, 0, 4, 5), [1.0]):
        refused("guide must be", guide=guide)
    for attr in (torch.ones(2, 4, 5), torch.ones(2, 1, 4, 5).half(), torch.ones(3, 1, 4, 5), torch.ones(2, 1, 4, 6), torch.ones(2, 5, 4, 5),
                 torch.ones(2, 0, 4, 5), "a"):
        refused("attr must be", attr=attr)
    for radius in (-1, 17, 1.5, math.nan, True, "2", None):
        refused("radius must be", radius=radius)
    for s in (0.0, -1.0, math.nan, math.inf, "x", 1e39):
        refused("sigma_s must be", sigma_s=s)
        refused("sigma_r must be", sigma_r=s)
    refused("sigma_r must be", sigma_r=None)
    for mw in (0.0, -1e-3, 1e-25, math.nan, math.inf, None, "w"):
        refused("min_weight must be", min_weight=mw)
    for s in (1e-20, 1e-30):
        refused(r"1 / \(2 sigma\^2\) must be", sigma_s=s)
    refused(r"1 / \(2 sigma\^2\) must be", sigma_r=1e-20, guide=torch.ones(2, 1, 4, 5))
    for keep in (2, -1, None, "yes", 0.5):
        refused("keep must be", keep=keep)
    for fill in ("x", None, [0.0]):
        refused("fill must be", fill=fill)
    # every check above passed on CPU tensors: the device check comes last, still ahead of the library
    msg = "every tensor must be a contiguous tensor on the same GPU"
    refused(msg)
    refused(msg, guide=torch.ones(2, 4, 4, 5), attr=torch.ones(2, 4, 4, 5), radius=16, sigma_s=0.5, sigma_r=10.0, min_weight=1e-24, keep=0,
            fill=math.nan, want_count=True)
    refused(msg, radius=0, sigma_r=1e-20)                                         # sigma_r is ignored without a guide


def test_c_entry_refuses_what_is_outside_the_contract():
    """CMR_EINVAL up front: every check sits ahead of the first launch, so this runs without a GPU (the pointers are never followed)."""
    lib = _lib.load()
    buf = torch.zeros(64)
    p = buf.data_ptr()
    names = _lib.parse_header()["cmr_densify_f32"][2]
    base = dict(depth=p, attr=None, C=0, guide=None, Cg=0, B=1, h=2, w=2, radius=1, sigma_s=1.0, sigma_r=0.1, min_weight=1e-3, keep=1, fill=0.0,
                dense_depth=p, dense_attr=None, conf=p, count=None, counts=p, stream=None)
    call = lambda **kw: lib.cmr_densify_f32(*[{**base, **kw}[k] for k in names])
    for bad in (dict(depth=None), dict(dense_depth=None), dict(conf=None), dict(counts=None), dict(B=0), dict(B=65536), dict(h=0), dict(w=-1),
                dict(h=4097, w=4096), dict(radius=-1), dict(radius=17), dict(sigma_s=0.0), dict(sigma_s=-1.0), dict(sigma_s=math.nan),
                dict(sigma_s=math.inf), dict(sigma_s=1e-30), dict(min_weight=0.0), dict(min_weight=1e-25), dict(min_weight=math.nan),
                dict(min_weight=math.inf), dict(keep=2), dict(keep=-1), dict(attr=p), dict(dense_attr=p), dict(attr=p, dense_attr=p, C=0),
                dict(attr=p, dense_attr=p, C=5), dict(C=1), dict(guide=p, Cg=0), dict(guide=p, Cg=5), dict(Cg=1),
                dict(guide=p, Cg=1, sigma_r=0.0), dict(guide=p, Cg=1, sigma_r=math.nan), dict(guide=p, Cg=1, sigma_r=1e-30)):
        assert call(**bad) == -1, bad


# ---- the PFM writer -------------------------------------------------------------------------------------------------------------------------
def _read_pfm(path):
    """A reader written for this test: -> (float32 [h, w] with row 0 at the top, scale)."""
    raw = open(path, "rb").read()
    magic, dims, scale, payload = raw.split(b"\n", 3)
    assert magic == b"Pf"
    w, h = (int(t) for t in dims.split())
    scale = float(scale)
    data = np.frombuffer(payload, "<f4" if scale < 0 else ">f4")
    assert data.size == w * h
    return data.reshape(h, w)[::-1], scale


def test_pfm_round_trip(tmp_path):
    g = torch.Generator().manual_seed(4)
    img = torch.rand(5, 7, generator=g) * 50.0
    img[0, 0], img[4, 6], img[2, 3] = math.inf, math.nan, -math.inf
    path = str(tmp_path / "d.pfm")
    assert pfm.write_pfm(path, img) == (5, 7)
    raw = open(path, "rb").read()
    assert raw.startswith(b"Pf\n7 5\n-1.0\n") and len(raw) == len(b"Pf\n7 5\n-1.0\n") + 4 * 35
    got, scale = _read_pfm(path)
    want = torch.where(torch.isfinite(img), img, torch.zeros(())).numpy()
    assert scale == -1.0 and np.array_equal(got, want) and got[0, 0] == 0.0 and got[4, 6] == 0.0
    # the first float of the payload is the BOTTOM row's first pixel
    assert np.frombuffer(raw[-4 * 35:][:4], "<f4")[0] == want[4, 0]
    pfm.write_pfm(path, np.arange(6.0).reshape(2, 3), empty=-1.0)
    assert _read_pfm(path)[0].tolist() == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]
    for bad in (np.zeros(4), np.zeros((2, 3, 1)), np.zeros((0, 3))):
        with pytest.raises(ValueError, match="write_pfm: image must be"):
            pfm.write_pfm(path, bad)


# ---- the model layer with ops stubbed ---------------------------------------------------------------------------------------------------------
class _FakeOps:
    """Stands in for cmr_agent_amd.ops inside MultiHeadModel: CPU tensors of the right shapes, and a log of the calls."""
    _is_int = staticmethod(ops._is_int)

    def __init__(self):
        self.log = []

    def visibility(self, pts, pose, K, h, w, mask, **kw):
        B, _, N = pts.shape
        self.log.append(("visibility", pose.clone(), K.clone(), (h, w), mask, kw))
        vis = (mask.reshape(-1) != 0) & (torch.arange(B * N) % 2 == 0)
        return vis, torch.zeros(B, 4, dtype=torch.int32), None, None, None

    def render_points(self, pts, pose, K, h, w, attr=None, mask=None, splat=0, fill=0.0):
        B = pts.shape[0]
        self.log.append(("render_points", pose.clone(), K.clone(), (h, w), attr, mask, splat, fill))
        return (torch.zeros(B, h, w, dtype=torch.int32), torch.full((B, h, w), 7.0), None if attr is None else torch.full((B, attr.shape[1], h, w), 3.0),
                torch.zeros(B, 3, dtype=torch.int32))

    def densify(self, depth, guide=None, attr=None, **kw):
        self.log.append(("densify", depth, guide, attr, kw))
        B, h, w = depth.shape
        return depth + 1.0, None if attr is None else attr + 1.0, torch.ones(B, h, w), None, torch.full((B, 3), 5, dtype=torch.int32)


def _batch(B=2, N=6, h=4, w=5, planes=3):
    g = torch.Generator().manual_seed(5)
    K = torch.tensor([[50.0, 0.0, 2.0], [0.0, 60.0, 1.5], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    return {"pc": torch.randn(B, 3, N, generator=g), "K": K, "pc_geo_feat": torch.randn(B, 64, N, generator=g),
            "img_geo_feat": torch.randn(B, 64, h, w, generator=g), "pc_overlap_pred": torch.ones(B, N, dtype=torch.int64),
            "pnp_pose": torch.eye(4).repeat(B, 1, 1), "img": torch.rand(B, planes, 4 * h, 8 * w, generator=g)}


def test_model_dense_depth_hands_on_the_right_arguments(monkeypatch):
    fake = _FakeOps()
    monkeypatch.setattr(mhm, "ops", fake)
    model = mhm.MultiHeadModel.__new__(mhm.MultiHeadModel)                       # the method under test uses no weights
    data = _batch()
    mhm.MultiHeadModel.dense_depth(model, data)
    ren, den = fake.log
    K_full = torch.tensor([[400.0, 0.0, 16.0], [0.0, 240.0, 6.0], [0.0, 0.0, 1.0]])  # row 0 by 40 / 5, row 1 by 16 / 4, as paint_points
    assert ren[0] == "render_points" and torch.equal(ren[1], data["pnp_pose"]) and torch.equal(ren[2][1], K_full) and ren[3] == (16, 40)
    assert ren[4] is None and ren[5] is None and ren[6] == 0 and ren[7] == 0.0
    assert den[0] == "densify" and bool((den[1] == 7.0).all()) and den[2].data_ptr() == data["img"].data_ptr() and den[3] is None
    assert den[4] == dict(radius=8, sigma_s=None, sigma_r=0.1, min_weight=1e-3, keep=True, fill=0.0)
    assert tuple(data["dense_depth_map"].shape) == (2, 16, 40) and bool((data["dense_depth_map"] == 8.0).all())
    assert tuple(data["dense_conf_map"].shape) == (2, 16, 40) and data["dense_counts"].tolist() == [[5, 5, 5]] * 2 and "dense_attr_map" not in data
    # an image of more than 4 planes guides with its first 3; 4 planes are used as they are
    for planes, used in ((6, 3), (4, 4), (1, 1)):
        fake.log.clear()
        d = _batch(planes=planes)
        mhm.MultiHeadModel.dense_depth(model, d)
        assert tuple(fake.log[1][2].shape) == (2, used, 16, 40) and torch.equal(fake.log[1][2], d["img"][:, :used]) and fake.log[1][2].is_contiguous()
    # everything explicit: size and K together, a [3, 3] K is broadcast, the guide at that size, attr / mask / splat go to render_points
    fake.log.clear()
    pose, a, m = torch.eye(4).repeat(2, 1, 1) * 2.0, torch.rand(2, 2, 6), torch.tensor([[1, 0, 1, 0, 1, 0]] * 2, dtype=torch.uint8)
    gd = torch.rand(2, 1, 8, 10)
    mhm.MultiHeadModel.dense_depth(model, data, pose=pose, size=(8, 10), K=torch.eye(3) * 3.0, guide=gd, attr=a, mask=m, splat=2, radius=4, sigma_s=1.5,
                                   sigma_r=0.2, min_weight=0.5, keep=False, fill=math.nan)
    ren, den = fake.log
    assert torch.equal(ren[1], pose) and torch.equal(ren[2], (torch.eye(3) * 3.0).repeat(2, 1, 1)) and ren[3] == (8, 10) and torch.equal(ren[4], a)
    assert torch.equal(ren[5], m) and ren[6] == 2 and math.isnan(ren[7])
    assert torch.equal(den[2], gd) and bool((den[3] == 3.0).all()) and tuple(den[3].shape) == (2, 2, 8, 10)
    kw = dict(den[4])
    assert math.isnan(kw.pop("fill")) and kw == dict(radius=4, sigma_s=1.5, sigma_r=0.2, min_weight=0.5, keep=False)
    assert tuple(data["dense_attr_map"].shape) == (2, 2, 8, 10) and bool((data["dense_attr_map"] == 4.0).all())
    # guide=False: a plain normalised convolution
    fake.log.clear()
    mhm.MultiHeadModel.dense_depth(model, data, guide=False)
    assert fake.log[1][2] is None and fake.log[0][3] == (16, 40)
    # visible: ops.visibility first, on the geometric map with the batch's own K under the same pose, the whole cloud occluding
    for visible, want in ((True, dict(radius=1, rel_tol=0.05, abs_tol=0.0)), (dict(radius=2, abs_tol=0.5), dict(radius=2, rel_tol=0.05, abs_tol=0.5))):
        fake.log.clear()
        mhm.MultiHeadModel.dense_depth(model, data, pose=pose, mask=m, visible=visible)
        assert [c[0] for c in fake.log] == ["visibility", "render_points", "densify"]
        vis, ren, _ = fake.log
        assert torch.equal(vis[1], pose) and torch.equal(vis[2], data["K"]) and vis[3] == (4, 5) and torch.equal(vis[4], m) and vis[5] == want
        assert ren[5].dtype == torch.bool and ren[5].view(-1).tolist() == [bool(m.view(-1)[i]) and i % 2 == 0 for i in range(12)]
        assert torch.equal(ren[2][0], K_full)
    fake.log.clear()
    mhm.MultiHeadModel.dense_depth(model, data, visible=True)                    # no mask: every row is queried
    assert fake.log[0][4].dtype == torch.bool and bool(fake.log[0][4].all()) and tuple(fake.log[0][4].shape) == (2, 6)
    for kw in (dict(size=(8, 10)), dict(K=torch.eye(3))):
        with pytest.raises(ValueError, match="dense_depth: size and K go together"):
            mhm.MultiHeadModel.dense_depth(model, _batch(), **kw)
    for bad in (3, "yes", dict(tau=1.0)):
        with pytest.raises(ValueError, match="dense_depth: visible must be"):
            mhm.MultiHeadModel.dense_depth(model, _batch(), visible=bad)


# ---- the command-line flags ---------------------------------------------------------------------------------------------------------------
def test_dense_flags():
    import argparse

    def parse(*argv, parent="--pnp", parent_given=True):
        ap = argparse.ArgumentParser()
        evalcli.add_dense_flags(ap, parent)
        return evalcli.dense_option(ap, ap.parse_args(list(argv)), ops.DENSIFY_MAX_RADIUS, parent, parent_given)

    assert parse() is None and parse(parent_given=False) is None
    assert parse("--dense-depth", "out") == ("out", 8, 0.1, False)
    assert parse("--dense-depth", "out", "--dense-radius", "4", "--dense-sigma-r", "0.05", "--dense-visible") == ("out", 4, 0.05, True)
    assert parse("--dense-depth", "out", "--dense-radius", "0", parent=None, parent_given=False) == ("out", 0, 0.1, False)   # free-standing
    for argv, given in ((("--dense-visible",), True), (("--dense-radius", "4"), True), (("--dense-sigma-r", "0.1"), True), (("--dense-depth", "out"), False),
                        (("--dense-depth", "out", "--dense-radius", "17"), True), (("--dense-depth", "out", "--dense-radius", "-1"), True),
                        (("--dense-depth", "out", "--dense-sigma-r", "0"), True), (("--dense-depth", "out", "--dense-sigma-r", "nan"), True)):
        with pytest.raises(SystemExit):
            parse(*argv, parent_given=given)


def test_dense_pairs_writes_one_file_per_pair(tmp_path, capsys):
    class Model:
        def dense_depth(self, data, pose=None, radius=None, sigma_r=None, visible=None):
            self.seen = (pose, radius, sigma_r, visible)
            d = torch.arange(12.0).view(2, 2, 3) + 1.0
            d[0, 0, 1] = math.inf
            data["dense_depth_map"] = d
            data["dense_counts"] = torch.tensor([[2, 6, 5], [3, 6, 6]], dtype=torch.int32)

    model, data = Model(), {}
    out = str(tmp_path / "maps")
    evalcli.dense_pairs(model, data, "POSE", (out, 4, 0.05, True), 4)
    assert model.seen == ("POSE", 4, 0.05, True) and capsys.readouterr().out == "dense 11 of 12 from 5\n"
    assert sorted(os.listdir(out)) == ["pair_4_depth.pfm", "pair_5_depth.pfm"]
    assert _read_pfm(os.path.join(out, "pair_4_depth.pfm"))[0].tolist() == [[1.0, 0.0, 3.0], [4.0, 5.0, 6.0]]
    assert _read_pfm(os.path.join(out, "pair_5_depth.pfm"))[0].tolist() == [[7.0, 8.0, 9.0], [10.0, 11.0, 12.0]]
    evalcli.dense_pairs(model, data, "POSE", (out, 8, 0.1, False), 0)
    assert model.seen == ("POSE", 8, 0.1, None)


@pytest.mark.parametrize("script,argv", [
    ("Test_Geo.py", ("--dense-depth", "x")),                                      # needs --pnp
    ("Test_Geo.py", ("--pnp", "--dense-visible")),
    ("Test_Geo.py", ("--pnp", "--dense-radius", "4")),
    ("Test_Agent.py", ("--dense-sigma-r", "0.2")),
    ("Test_Agent.py", ("--dense-depth", "x", "--dense-radius", "17")),
])
def test_scripts_reject_misplaced_flags(script, argv, tmp_path):
    argv = tuple(str(tmp_path / a) if a == "x" else a for a in argv)
    res = subprocess.run([sys.executable, os.path.join(ROOT, script), *argv], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 2 and "--dense-depth" in res.stderr, res.stderr[-2000:]
    assert not os.path.exists(str(tmp_path / "x"))
