"""CPU tier of point painting and attribute rendering: the float64 restatement in point_image_reference.py gives the
hand-computed values on scenes small enough to check by eye (so the yardstick of the GPU tests is itself checked), the scenes of the GPU
tier keep their undecided rows under the cap, ops.paint_points / ops.render_points refuse malformed arguments before the library is
touched, the workspace query answers without a GPU, the PLY writer round-trips, and the two model methods hand on what they should."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import point_image_reference as pir
import visibility_reference as vr
from cmr_agent_amd import _lib, ops
from cmr_agent_amd.utils import evalcli, ply

mhm = importlib.import_module("cmr_agent_amd.models.MultiHeadModel")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement on the hand scenes -----------------------------------------------------------------------------------------------------
def test_restatement_paints_the_hand_scene():
    pts, pose, K, img = pir.hand_paint()
    r = pir.paint(pts, None, pose, K, img)[0]
    # rows 0, 3, 6, 7 and 8 sit on half-integers by construction: two candidate centres each, the rest one
    assert r["unique"].tolist() == [False, True, True, False, True, True, False, False, False]
    assert r["decided"].tolist() == [True] * 8 + [False] and r["undecided"] == 1          # row 8: rint may give column 9 or 10
    assert r["painted"][:8].astype(int).tolist() == pir.HAND_PAINTED[:8]
    on = np.array(pir.HAND_PAINTED, bool)
    assert r["bilinear"][0][on].tolist() == [v for v, p in zip(pir.HAND_BILINEAR, pir.HAND_PAINTED) if p]
    uniq = on & r["unique"]
    assert r["nearest"][0][uniq].tolist() == [v for v, p, q in zip(pir.HAND_NEAREST, pir.HAND_PAINTED, r["unique"]) if p and q]
    # every hand-written nearest value is the pixel at one of the row's candidate centres
    cxl, cxh, cyl, cyh = r["cand"]
    ramp = img[0, 0].numpy()
    for n in np.nonzero(on)[0]:
        cands = {float(ramp[y, x]) for x in (cxl[n], cxh[n]) for y in (cyl[n], cyh[n]) if 0 <= x < pir.HAND_W and 0 <= y < pir.HAND_H}
        assert pir.HAND_NEAREST[n] in cands
    # a mask composes; a NaN pose paints nothing and all of it is decided
    m = torch.tensor([[1, 0, 1, 0, 1, 1, 0, 0, 0]])
    r = pir.paint(pts, m, pose, K, img)[0]
    assert r["painted"].astype(int).tolist() == [1, 0, 1, 0, 0, 0, 0, 0, 0] and r["undecided"] == 0
    r = pir.paint(pts, None, torch.full((1, 4, 4), math.nan), K, img)[0]
    assert r["decided"].all() and not r["painted"].any()


def test_bound_is_tight_on_a_ramp_and_grows_with_the_slope():
    pts, pose, K, img = pir.hand_paint()
    r = pir.paint(pts, None, pose, K, img)[0]
    # on the ramp the largest difference between neighbours is 10 (one row down), the largest tap of row 0 is I[3, 4] = 34
    assert r["bound"][0, 0] == pytest.approx(2 * 10 * 64 * 2.0 ** -24 * (1.0 * np.linalg.norm([6.5, 5.0, 2.0]) / 2.0 + 10) + 16 * 2.0 ** -23 * 34)
    steep = pir.paint(pts, None, pose, K, img * 3.0)[0]
    assert steep["bound"][0, 0] == pytest.approx(3.0 * r["bound"][0, 0])


@pytest.mark.parametrize("splat", [0, 1])
def test_restatement_renders_the_hand_scene(splat):
    pts, pose, K = vr.hand()
    r = pir.render(pts, None, pose, K, vr.HAND_H, vr.HAND_W, splat)[0]
    assert r["decided"].all() and r["index_decided"].all()
    assert r["index"].tolist() == pir.HAND_INDEX[splat]
    assert np.array_equal(r["depth"].astype(np.float32), pir.hand_depth(pir.HAND_INDEX[splat]))
    assert [r["selected"], r["in_view_lo"], int((r["index"] >= 0).sum())] == pir.HAND_RENDER_COUNTS[splat]
    if splat == 0:
        assert np.array_equal(pir.hand_depth(pir.HAND_INDEX[0]), vr.hand_depth_map()[0].numpy())


def test_restatement_flags_what_fp32_may_decide_differently():
    # (3.5, 2) at depth 2 has two candidate cells: both undecided; two rows in one cell whose depths agree to 1e-9 leave the depth
    # decided and the owner open; equal depths go to the lower row
    pts = torch.tensor([[[3.5 * 2, 6.0, 6.0 * (1 + 1e-9), 8.0, 8.0], [2.0 * 2, 5.0, 5.0 * (1 + 1e-9), 1.0, 1.0], [2.0, 1.0, 1 + 1e-9, 1.0, 1.0]]],
                       dtype=torch.float64)
    r = pir.render(pts, None, torch.eye(4)[None], torch.eye(3)[None], 8, 10, 0)[0]
    assert not r["decided"][2, 3] and not r["decided"][2, 4] and int((~r["decided"]).sum()) == 2
    assert r["decided"][5, 6] and not r["index_decided"][5, 6] and r["index"][5, 6] == 1
    assert r["decided"][1, 8] and not r["index_decided"][1, 8] and r["index"][1, 8] == 3
    r1 = pir.render(pts, None, torch.eye(4)[None], torch.eye(3)[None], 8, 10, 1)[0]
    assert not r1["decided"][1:4, 2:6].any() and r1["decided"][0, 0] and r1["index"][0, 7] == 3


# ---- the cap on the scenes of the GPU tier -------------------------------------------------------------------------------------------------
def _scenes():
    return [(name, pir.built(name)) for name in pir.SCENE_NAMES]


def test_undecided_rows_stay_under_the_cap():
    """At most max(4, 1 %) of a sample's selected rows may have an undecided in-view decision -- a condition on the inputs, asserted from
    the restatement alone; and the scenes have rows inside and outside the image."""
    for name, sc in _scenes():
        B, _, N = sc["pts"].shape
        img = np.zeros((B, 1, sc["h"], sc["w"]))
        for b, r in enumerate(pir.paint(sc["pts"], sc["mask"], sc["pose"], sc["K"], img)):
            nsel = int(r["sel"].sum())
            print(name, "sample", b, "selected", nsel, "undecided", r["undecided"], "decided painted", int(r["painted"].sum()))
            assert r["undecided"] <= vr.cap(nsel)
            if N > 1:
                assert 0 < int(r["painted"].sum()) < nsel
        for splat in (0, 1, 4):
            for b, r in enumerate(pir.render(sc["pts"], sc["mask"], sc["pose"], sc["K"], sc["h"], sc["w"], splat)):
                und, open_owner = int((~r["decided"]).sum()), int((r["decided"] & ~r["index_decided"]).sum())
                print(name, "splat", splat, "sample", b, "ambiguous rows", r["ambiguous"], "undecided pixels", und, "of", r["decided"].size,
                      "decided pixels with an open owner", open_owner)
                assert r["view_undecided"] <= vr.cap(r["selected"]) and r["ambiguous"] <= vr.cap(r["selected"])
                # what the float64 comparison may leave out, at every footprint the GPU tier compares (0 and 1) and at the largest: an
                # ambiguous row has at most 2 x 2 candidate cells, each inside the window of (2 splat + 1)^2 pixels -- together a square of
                # at most (2 splat + 2)^2 pixels; and an owner is open only where two depths in one window agree to 2 * 8 2^-23 S, about
                # 2e-6 of the depth, which uniform depths (2 .. 50, the wall 3 .. 3.3) do for well under 1 % of the windows
                assert und <= r["ambiguous"] * (2 * splat + 2) ** 2
                assert open_owner <= max(1, r["decided"].size // 100)
                if N > 1 and sc["h"] * sc["w"] > 1 and splat <= 1:
                    assert r["decided"].mean() > 0.9


# ---- argument checks and the workspace query ------------------------------------------------------------------------------------------------
def _touched(*a, **k):
    raise AssertionError("the library was touched before the arguments were checked")


def _args(B=2, N=8, C=3, H=4, W=5):
    return dict(pts=torch.zeros(B, 3, N), pose=torch.eye(4).repeat(B, 1, 1), K=torch.eye(3).repeat(B, 1, 1), image=torch.zeros(B, C, H, W))


def test_paint_points_argument_checks(monkeypatch):
    monkeypatch.setattr(_lib, "load", _touched)
    monkeypatch.setattr(_lib, "call", _touched)

    def refused(match, **kw):
        a = _args()
        opt = {k: kw.pop(k) for k in ("mask", "mode", "want_uv") if k in kw}
        a.update(kw)
        with pytest.raises(ValueError, match="^paint_points: " + match):
            ops.paint_points(a["pts"], a["pose"], a["K"], a["image"], **opt)

    a = _args()
    refused("pts must be", pts=a["pts"][0])
    refused("pts must be", pts=a["pts"][:, :2])
    for k in ("pts", "pose", "K"):
        refused("pts, pose and K must be float32", **{k: a[k].double()})
    refused("pose must be", pose=a["pose"][:1])
    refused("pose must be", pose=a["pose"][:, :3])
    refused("K must be", K=a["K"][:, :2])
    refused("image must be planar", image=a["image"][0])
    refused("image must be planar", image=None)
    refused("image must be float32", image=a["image"].double())
    refused("image must be float32", image=(a["image"] * 255).to(torch.uint8))
    refused("image must be", image=a["image"][:1])
    refused("image must be", image=torch.zeros(2, 65, 4, 5))
    refused("image must be", image=torch.zeros(2, 0, 4, 5))
    refused("need 1 <= B", image=torch.zeros(2, 1, 0, 5))
    refused("need 1 <= B", image=torch.zeros(1).expand(2, 1, 4097, 4096))      # shape only: 4 bytes of storage
    refused("mask must be", mask=torch.ones(2, 8))
    refused("mask must be", mask=torch.ones(2, 7, dtype=torch.bool))
    for mode in ("bicubic", 1, None, "Nearest"):
        refused("mode must be", mode=mode)
    # every check above passed on CPU tensors: the device check comes last, still ahead of the library
    refused("every tensor must be a contiguous tensor on the same GPU")
    refused("every tensor must be a contiguous tensor on the same GPU", mask=torch.ones(16, dtype=torch.int64), mode="nearest", want_uv=True)


def test_render_points_argument_checks(monkeypatch):
    monkeypatch.setattr(_lib, "load", _touched)
    monkeypatch.setattr(_lib, "call", _touched)

    def refused(match, h=4, w=5, **kw):
        a = _args()
        opt = {k: kw.pop(k) for k in ("attr", "mask", "splat", "fill") if k in kw}
        a.update(kw)
        with pytest.raises(ValueError, match="^render_points: " + match):
            ops.render_points(a["pts"], a["pose"], a["K"], h, w, **opt)

    a = _args()
    refused("pts must be", pts=a["pts"][:, :, 0])
    for k in ("pts", "pose", "K"):
        refused("pts, pose and K must be float32", **{k: a[k].half()})
    refused("pose must be", pose=a["pose"][:1])
    refused("K must be", K=a["K"][:1])
    for h, w in ((0, 5), (4, 0), (-1, 5), (4097, 4096)):
        refused("need 1 <= B", h=h, w=w)
    for h in (4.5, None, "4", True, math.nan):
        refused("h and w must be integers", h=h)
    refused("mask must be", mask=torch.ones(2, 8, dtype=torch.int32))
    for attr in (torch.zeros(2, 3, 8).double(), torch.zeros(2, 3, 7), torch.zeros(1, 3, 8), torch.zeros(2, 65, 8), torch.zeros(2, 0, 8), torch.zeros(2, 8), [1.0]):
        refused("attr must be", attr=attr)
    for splat in (-1, 5, 1.5, math.nan, True, "2", None):
        refused("splat must be", splat=splat)
    for fill in ("x", None, [0.0]):
        refused("fill must be", fill=fill)
    refused("every tensor must be a contiguous tensor on the same GPU")
    refused("every tensor must be a contiguous tensor on the same GPU", attr=torch.zeros(2, 64, 8), mask=torch.ones(2, 8, dtype=torch.uint8), splat=4,
            fill=math.nan)


def test_workspace_query_and_header():
    lib = _lib.load()
    assert lib.cmr_render_points_workspace_bytes(3, 13, 19) == 3 * 13 * 19 * 8 + 8       # rounded up to 16
    assert lib.cmr_render_points_workspace_bytes(1, 1, 1) == 16
    for bad in ((0, 4, 5), (2, 0, 5), (2, 4, -1)):
        assert lib.cmr_render_points_workspace_bytes(*bad) == 0
    text = open(os.path.join(ROOT, "include", "cmr_hip.h")).read()
    assert re.search(r"int64_t\s+cmr_render_points_workspace_bytes\s*\(\s*int B,\s*int h,\s*int w\s*\)", text)
    protos = _lib.parse_header()
    assert protos["cmr_paint_points_f32"][2] == ["pts", "mask", "mask_bytes", "pose", "K", "image", "B", "N", "C", "H", "W", "mode", "colors",
                                                 "painted", "counts", "uv", "stream"]
    assert protos["cmr_render_points_f32"][2] == ["pts", "mask", "mask_bytes", "pose", "K", "attr", "C", "B", "N", "h", "w", "splat", "fill",
                                                  "index_map", "depth_map", "attr_map", "counts", "workspace", "workspace_bytes", "stream"]
    src = os.path.join(ROOT, "cmr_agent_amd", "csrc", "point_image.hip")
    assert os.path.exists(src) and "cmr_paint_points_f32" in open(src).read() and "cmr_render_points_f32" in open(src).read()
    from cmr_agent_amd.utils import workmodel
    assert "cmr_paint_points_f32" in open(workmodel.__file__).read() and "cmr_render_points_f32" in open(workmodel.__file__).read()


def test_c_entries_refuse_what_is_outside_the_contract():
    """CMR_EINVAL up front: every check sits ahead of the first launch, so this runs without a GPU (the pointers are never followed)."""
    lib = _lib.load()
    buf = torch.zeros(64)
    p = buf.data_ptr()
    paint = lambda **kw: lib.cmr_paint_points_f32(*[{**dict(pts=p, mask=p, mask_bytes=1, pose=p, K=p, image=p, B=1, N=4, C=3, H=2, W=2, mode=1, colors=p,
                                                            painted=p, counts=p, uv=None, stream=None), **kw}[k] for k in _lib.parse_header()["cmr_paint_points_f32"][2]])
    for bad in (dict(pts=None), dict(image=None), dict(colors=None), dict(painted=None), dict(counts=None), dict(B=0), dict(B=65536), dict(N=0),
                dict(C=0), dict(C=65), dict(H=0), dict(W=-1), dict(H=4097, W=4096), dict(mode=2), dict(mode=-1), dict(mask_bytes=4),
                dict(mask=None, mask_bytes=0)):
        assert paint(**bad) == -1, bad
    render = lambda **kw: lib.cmr_render_points_f32(*[{**dict(pts=p, mask=p, mask_bytes=1, pose=p, K=p, attr=None, C=0, B=1, N=4, h=2, w=2, splat=0,
                                                              fill=0.0, index_map=p, depth_map=p, attr_map=None, counts=p, workspace=p, workspace_bytes=32,
                                                              stream=None), **kw}[k] for k in _lib.parse_header()["cmr_render_points_f32"][2]])
    for bad in (dict(pts=None), dict(index_map=None), dict(depth_map=None), dict(counts=None), dict(workspace=None), dict(workspace_bytes=31),
                dict(workspace=p + 4), dict(B=0), dict(N=0), dict(h=0), dict(h=4097, w=4096, workspace_bytes=1 << 40), dict(splat=-1), dict(splat=5),
                dict(mask_bytes=2), dict(attr=p), dict(attr_map=p), dict(attr=p, attr_map=p, C=0), dict(attr=p, attr_map=p, C=65), dict(C=3)):
        assert render(**bad) == -1, bad


# ---- the PLY writer --------------------------------------------------------------------------------------------------------------------------
def test_ply_round_trip(tmp_path):
    g = torch.Generator().manual_seed(3)
    xyz = torch.randn(37, 3, generator=g)
    rgb = torch.tensor([[0.0, 1.0, 0.5], [-0.2, 1.7, 0.25], [0.002, 0.998, 0.01]] + [[0.1, 0.2, 0.3]] * 34)
    path = str(tmp_path / "cloud.ply")
    assert ply.write_ply(path, xyz, rgb) == 37
    raw = open(path, "rb").read()
    head, payload = raw.split(b"end_header\n", 1)
    assert head.decode("ascii").split("\n")[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 37"]
    assert [l.split()[1:] for l in head.decode("ascii").split("\n") if l.startswith("property")] == [
        ["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
    assert len(payload) == 37 * 15
    v = np.frombuffer(payload, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    assert np.array_equal(v["p"], xyz.numpy())
    assert v["c"][:3].tolist() == [[0, 255, 128], [0, 255, 64], [1, 254, 3]]               # clamp(rint(255 c), 0, 255), half to even
    back_xyz, back_rgb = pir.read_ply(path)
    assert np.array_equal(back_xyz, xyz.numpy()) and np.array_equal(back_rgb, v["c"])
    assert ply.write_ply(path, np.zeros((0, 3)), np.zeros((0, 3))) == 0 and pir.read_ply(path)[0].shape == (0, 3)
    with pytest.raises(ValueError, match="write_ply: xyz and rgb"):
        ply.write_ply(path, np.zeros((4, 3)), np.zeros((3, 3)))


# ---- the model layer with ops stubbed -----------------------------------------------------------------------------------------------------------
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

    def paint_points(self, pts, pose, K, image, mask=None, mode='bilinear', want_uv=False):
        B, _, N = pts.shape
        self.log.append(("paint_points", pose.clone(), K.clone(), image, mask, mode))
        return torch.ones(B, image.shape[1], N), torch.ones(B * N, dtype=torch.bool), torch.full((B, 2), N, dtype=torch.int32), None

    def render_points(self, pts, pose, K, h, w, attr=None, mask=None, splat=0, fill=0.0):
        B = pts.shape[0]
        self.log.append(("render_points", pose.clone(), K.clone(), (h, w), attr, mask, splat, fill))
        return (torch.zeros(B, h, w, dtype=torch.int32), torch.zeros(B, h, w), None if attr is None else torch.zeros(B, attr.shape[1], h, w),
                torch.zeros(B, 3, dtype=torch.int32))


def _batch(B=2, N=6, h=4, w=5):
    g = torch.Generator().manual_seed(5)
    K = torch.tensor([[50.0, 0.0, 2.0], [0.0, 60.0, 1.5], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    return {"pc": torch.randn(B, 3, N, generator=g), "K": K, "pc_geo_feat": torch.randn(B, 64, N, generator=g),
            "img_geo_feat": torch.randn(B, 64, h, w, generator=g), "pc_overlap_pred": torch.ones(B, N, dtype=torch.int64),
            "pnp_pose": torch.eye(4).repeat(B, 1, 1), "img": torch.rand(B, 3, 4 * h, 8 * w, generator=g)}


def test_model_paint_points_hands_on_the_right_arguments(monkeypatch):
    fake = _FakeOps()
    monkeypatch.setattr(mhm, "ops", fake)
    model = mhm.MultiHeadModel.__new__(mhm.MultiHeadModel)                       # the methods under test use no weights
    data = _batch()
    mhm.MultiHeadModel.paint_points(model, data)
    (name, pose, K, image, mask, mode), = fake.log
    # defaults: 'pnp_pose', 'img', every row, bilinear, and 'K' scaled from the 4 x 5 map to the 16 x 40 image: row 0 by 8, row 1 by 4
    assert name == "paint_points" and torch.equal(pose, data["pnp_pose"]) and image.data_ptr() == data["img"].data_ptr() and mask is None
    assert mode == "bilinear" and K.is_contiguous()
    assert torch.equal(K[1], torch.tensor([[400.0, 0.0, 16.0], [0.0, 240.0, 6.0], [0.0, 0.0, 1.0]]))
    assert tuple(data["point_colors"].shape) == (2, 3, 6) and data["point_painted"].dtype == torch.bool and tuple(data["point_painted"].shape) == (2, 6)
    assert tuple(data["paint_counts"].shape) == (2, 2)
    # everything explicit: a [3, 3] K is broadcast, the mask is handed on as it is, no visibility call
    fake.log.clear()
    pose, img5, m = torch.eye(4).repeat(2, 1, 1) * 2.0, torch.rand(2, 5, 7, 9), torch.tensor([[1, 0, 1, 0, 1, 0]] * 2, dtype=torch.uint8)
    mhm.MultiHeadModel.paint_points(model, data, pose=pose, image=img5, K=torch.eye(3) * 3.0, mask=m, mode="nearest")
    (name, gpose, K, image, mask, mode), = fake.log
    assert torch.equal(gpose, pose) and torch.equal(K, (torch.eye(3) * 3.0).repeat(2, 1, 1)) and torch.equal(image, img5)
    assert mask.dtype == torch.uint8 and torch.equal(mask, m) and mode == "nearest"
    # visible: ops.visibility first, on the geometric map with the batch's own K under the same pose, 4r's defaults, every row occluding;
    # what it leaves visible is the mask that is painted
    for visible, want in ((True, dict(radius=1, rel_tol=0.05, abs_tol=0.0)), (dict(radius=2, abs_tol=0.5), dict(radius=2, rel_tol=0.05, abs_tol=0.5))):
        fake.log.clear()
        mhm.MultiHeadModel.paint_points(model, data, pose=pose, mask=m, visible=visible)
        assert [c[0] for c in fake.log] == ["visibility", "paint_points"]
        vis, pnt = fake.log
        assert torch.equal(vis[1], pose) and torch.equal(vis[2], data["K"]) and vis[3] == (4, 5) and torch.equal(vis[4], m) and vis[5] == want
        assert pnt[4].dtype == torch.bool and pnt[4].view(-1).tolist() == [bool(m.view(-1)[i]) and i % 2 == 0 for i in range(12)]
        assert torch.equal(pnt[2][0], torch.tensor([[400.0, 0.0, 16.0], [0.0, 240.0, 6.0], [0.0, 0.0, 1.0]]))
    fake.log.clear()
    mhm.MultiHeadModel.paint_points(model, data, visible=True)                    # no mask: every row is queried
    assert fake.log[0][4].dtype == torch.bool and bool(fake.log[0][4].all()) and tuple(fake.log[0][4].shape) == (2, 6)
    for bad in (3, "yes", dict(tau=1.0)):
        with pytest.raises(ValueError, match="paint_points: visible must be"):
            mhm.MultiHeadModel.paint_points(model, _batch(), visible=bad)


def test_model_render_points_hands_on_the_right_arguments(monkeypatch):
    fake = _FakeOps()
    monkeypatch.setattr(mhm, "ops", fake)
    model = mhm.MultiHeadModel.__new__(mhm.MultiHeadModel)
    data = _batch()
    mhm.MultiHeadModel.render_points(model, data)
    (name, pose, K, size, attr, mask, splat, fill), = fake.log
    assert name == "render_points" and torch.equal(pose, data["pnp_pose"]) and torch.equal(K, data["K"]) and size == (4, 5)
    assert attr is None and mask is None and splat == 0 and fill == 0.0
    assert data["index_map"].dtype == torch.int32 and tuple(data["index_map"].shape) == (2, 4, 5) and tuple(data["render_depth_map"].shape) == (2, 4, 5)
    assert tuple(data["render_counts"].shape) == (2, 3) and "attr_map" not in data and "depth_map" not in data
    fake.log.clear()
    a, m, pose = torch.rand(2, 5, 6), torch.ones(2, 6, dtype=torch.bool), torch.eye(4).repeat(2, 1, 1) * 2.0
    mhm.MultiHeadModel.render_points(model, data, attr=a, pose=pose, size=(16, 40), K=torch.eye(3), mask=m, splat=2, fill=math.nan)
    (name, gpose, K, size, attr, mask, splat, fill), = fake.log
    assert torch.equal(gpose, pose) and torch.equal(K, torch.eye(3).repeat(2, 1, 1)) and size == (16, 40) and torch.equal(attr, a)
    assert torch.equal(mask, m) and splat == 2 and math.isnan(fill) and tuple(data["attr_map"].shape) == (2, 5, 16, 40)
    for kw in (dict(size=(8, 10)), dict(K=torch.eye(3))):
        with pytest.raises(ValueError, match="render_points: size and K go together"):
            mhm.MultiHeadModel.render_points(model, _batch(), **kw)


# ---- the command-line flags ---------------------------------------------------------------------------------------------------------------
def test_paint_flags():
    import argparse

    def parse(*argv, parent="--pnp", parent_given=True):
        ap = argparse.ArgumentParser()
        evalcli.add_paint_flags(ap, parent)
        return evalcli.paint_option(ap, ap.parse_args(list(argv)), parent, parent_given)

    assert parse() is None and parse(parent_given=False) is None
    assert parse("--paint", "out") == ("out", False) and parse("--paint", "out", "--paint-visible") == ("out", True)
    assert parse("--paint", "out", parent=None, parent_given=False) == ("out", False)          # free-standing
    for argv, given in ((("--paint-visible",), True), (("--paint", "out"), False)):
        with pytest.raises(SystemExit):
            parse(*argv, parent_given=given)


def test_paint_pairs_writes_one_file_per_pair(tmp_path, capsys):
    class Model:
        def paint_points(self, data, pose=None, visible=None):
            self.seen = (pose, visible)
            data["point_colors"] = torch.tensor([[[0.0, 1.0, 0.5], [0.2, 0.4, 0.6], [1.0, 0.0, 0.0]]] * 2)
            data["point_painted"] = torch.tensor([[True, False, True], [False, False, True]])
            data["paint_counts"] = torch.tensor([[3, 2], [3, 1]], dtype=torch.int32)

    data = {"pc": torch.arange(18.0).view(2, 3, 3)}
    model = Model()
    out = str(tmp_path / "clouds")
    evalcli.paint_pairs(model, data, "POSE", (out, True), 4)
    assert model.seen == ("POSE", True) and capsys.readouterr().out == "painted 3 of 6\n"
    assert sorted(os.listdir(out)) == ["pair_4.ply", "pair_5.ply"]
    xyz, rgb = pir.read_ply(os.path.join(out, "pair_4.ply"))
    assert xyz.tolist() == [[0.0, 3.0, 6.0], [2.0, 5.0, 8.0]] and rgb.tolist() == [[0, 51, 255], [128, 153, 0]]
    xyz, rgb = pir.read_ply(os.path.join(out, "pair_5.ply"))
    assert xyz.tolist() == [[11.0, 14.0, 17.0]] and rgb.tolist() == [[128, 153, 0]]
    evalcli.paint_pairs(model, data, "POSE", (out, False), 0)
    assert model.seen == ("POSE", None)


def test_paint_pairs_with_other_plane_counts(tmp_path, capsys):
    class Model:
        def __init__(self, C):
            self.C = C

        def paint_points(self, data, pose=None, visible=None):
            data["point_colors"] = torch.tensor([0.2, 0.4]).view(1, 1, 2).repeat(1, self.C, 1) + torch.arange(self.C).view(1, self.C, 1) * 0.125
            data["point_painted"] = torch.tensor([[True, True]])
            data["paint_counts"] = torch.tensor([[2, 2]], dtype=torch.int32)

    data = {"pc": torch.arange(6.0).view(1, 3, 2)}
    out = str(tmp_path / "c")
    evalcli.paint_pairs(Model(1), data, None, (out, False), 0)               # one plane: grey
    assert pir.read_ply(os.path.join(out, "pair_0.ply"))[1].tolist() == [[51, 51, 51], [102, 102, 102]]
    evalcli.paint_pairs(Model(5), data, None, (out, False), 0)               # five planes: the first three
    assert pir.read_ply(os.path.join(out, "pair_0.ply"))[1].tolist() == [[51, 83, 115], [102, 134, 166]]
    with pytest.raises(ValueError, match="--paint writes red, green, blue"):
        evalcli.paint_pairs(Model(2), data, None, (out, False), 0)
