"""GPU tier of range images and virtual scans (ops.range_image / ops.range_visible / ops.virtual_scan, csrc/range_image.hip,
dataset/view.py), against the restatement of range_image_reference.py.

Every comparison with the kernels is EXACT: index, counts and visible as integers, dist2 bit for bit -- the header states every fp32
operation behind them.  Every case is run twice: the two calls agree bit for bit, and the inputs are what they were."""
import os

import numpy as np
import pytest
import torch

import range_image_reference as G
from cmr_agent_amd import _lib, ops
from cmr_agent_amd.dataset import view

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
F = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)      # noqa: E731
ROWS = (1, 63, 64, 65, 255, 256, 257, 1025)                           # round the wave (64), a pass (256) and a workgroup's rows (1 024)
SHAPES = ((1, 4), (3, 8), (16, 64), (64, 1024), (128, 4096))
FIELD = dict(elev_lo=-0.5, elev_hi=0.3, min_range=1.0, max_range=80.0)


def same_bits(t, ref):
    return np.array_equal(G.bits(t.cpu().numpy()), G.bits(ref))


def image(pts, R, C, pose=None, **field):
    """One range image on both sides, compared.  -> the op's result"""
    field = field or FIELD
    p, T = F(pts), None if pose is None else F(pose)
    before = p.clone()
    got = ops.range_image(p, T, R, C, **field)
    again = ops.range_image(p, T, R, C, **field)
    index, dist2, counts = G.image(pts, R, C, pose, **field)
    assert got.index.dtype == torch.int32 and got.dist2.dtype == torch.float32 and tuple(got.index.shape) == tuple(got.dist2.shape) == (R, C)
    assert tuple(got[2:]) == counts and sum(counts) == pts.shape[0], (tuple(got[2:]), counts)
    assert np.array_equal(got.index.cpu().numpy(), index), np.argwhere(got.index.cpu().numpy() != index)[:8]
    assert same_bits(got.dist2, dist2), np.argwhere(G.bits(got.dist2.cpu().numpy()) != G.bits(dist2))[:8]
    assert torch.equal(got.index, again.index) and torch.equal(got.dist2.view(torch.int32), again.dist2.view(torch.int32)) and got[2:] == again[2:]
    assert torch.equal(p.view(torch.int32), before.view(torch.int32)), "the input was changed"
    return got


def visible(dist2, radius=(1, 1), rel_tol=0.05):
    """One visibility mask on both sides, compared.  -> the op's result"""
    d = F(dist2)
    before = d.clone()
    got = ops.range_visible(d, radius, rel_tol)
    again = ops.range_visible(d, radius, rel_tol)
    want = G.visible(dist2, radius, rel_tol)
    assert got.dtype == torch.bool and tuple(got.shape) == dist2.shape
    assert np.array_equal(got.cpu().numpy(), want), np.argwhere(got.cpu().numpy() != want)[:8]
    assert torch.equal(got, again) and torch.equal(d.view(torch.int32), before.view(torch.int32))
    return got


# ---- range_image ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ROWS)
def test_image_sizes(N):
    pts = G.scene(N)
    for R, C in SHAPES:
        for pose in (None, G.a_pose()):
            got = image(pts, R, C, pose)
            assert got.dropped == (1 if N >= 16 else 0) and (N < 255 or (got.outside > 0 and got.binned > 0))
    image(pts, 64, 1024, None, **{k: G.DEFAULTS[k] for k in FIELD})   # the wrapper's defaults


@pytest.mark.parametrize("R,C", SHAPES)
def test_image_rows_on_the_borders(R, C):
    lo, hi = FIELD["elev_lo"], FIELD["elev_hi"]
    # the axes, the diagonals, the origin of (x, y) with either zero, the z axis (r2 = 0: a positive z is outside through above(R))
    rim = F32([[3, 0, -1], [0, 3, -1.5], [-3, 0, -0.5], [0, -3, -0.25], [2, 2, -1], [-2, 2, -0.5], [-2, -2, -1.5], [2, -2, -0.75], [0, 0, -5], [-0.0, 0, -6],
               [0, -0.0, -7], [-0.0, -0.0, 8], [0, 0, 5], [3, -0.0, -0.9], [-0.0, 3, -0.95], [3, 0, 0.0], [3, 0, -0.0], [-3, -0.0, 0.0]])
    got = image(rim, R, C)
    assert got.outside == 5 and got.binned == 13
    # rows on the column edges and on the elevation edges, as far as fp32 holds them, and one step of fp32 to either side
    ang = np.arange(C) * 2 * np.pi / C
    cols = np.stack([9 * np.cos(ang), 9 * np.sin(ang), np.full(C, -0.7)], 1).astype(F32)
    e = lo + (hi - lo) * np.arange(R + 1) / R
    rows = np.concatenate([np.stack([7 * np.cos(e) * np.cos(a), 7 * np.cos(e) * np.sin(a), 7 * np.sin(e)], 1) for a in (0.3, 2.0, -2.5)]).astype(F32)
    pts = np.concatenate([cols, rows])
    got = image(np.concatenate([pts, np.nextafter(pts, F32(np.inf)), np.nextafter(pts, F32(-np.inf))]), R, C)
    assert got.binned > 3 * C and got.dropped == 0
    image(np.concatenate([pts, np.nextafter(pts, F32(np.inf)), np.nextafter(pts, F32(-np.inf))]), R, C, G.a_pose(3, (0.5, 0.25, -0.125)))
    # min_range and max_range exactly (3-4-5 triangles and an axis), the floats next to them, and squares that overflow
    on = F32([[1, 0, 0], [0.6, 0.8, 0], [0, -0.6, -0.8], [np.nextafter(F32(1), F32(0)), 0, 0], [np.nextafter(F32(1), F32(2)), 0, 0], [80, 0, 0], [48, 64, 0],
              [-64, 0, -48], [np.nextafter(F32(80), F32(0)), 0, 0], [np.nextafter(F32(80), F32(90)), 0, 0], [3e19, 3e19, 1], [2e38, 0, 0], [1, 1, -3e38],
              [np.nan, 1, 1], [1, -np.inf, 1], [1, 1, np.inf]])
    wide = dict(elev_lo=-1.2, elev_hi=1.2, min_range=1.0, max_range=80.0)
    got = image(on, R, C, None, **wide)
    assert got.dropped == 3 and got.binned == sum(G.rows(on, R, C, None, **wide)["state"] == G.BINNED) and 4 <= got.binned <= 6
    still = np.eye(4, dtype=F32)
    still[0, 3] = np.inf                                                # finite rows, a pose that makes them infinite: dropped
    assert image(on[:10], R, C, still, **wide).dropped == 10


def test_image_ties_and_contention():
    R, C = 16, 64
    rng = np.random.default_rng(5)
    pts = (F32([10, 1.5, -1.3]) + rng.uniform(-0.05, 0.05, (1025, 3))).astype(F32)                # well inside one cell of 16 x 64
    pts[800] = F32([9, 1.35, -1.17])                                    # the nearest row of the cell, three times: the lowest index wins
    pts[300] = pts[900] = pts[800]
    pts[512], pts[100] = pts[20], pts[1000]                             # more duplicates that lose
    w = G.rows(pts, R, C, **FIELD)
    assert len(set(zip(w["row"], w["col"]))) == 1 and (w["state"] == G.BINNED).all()
    got = image(pts, R, C)
    assert got.binned == 1025 and (got.index >= 0).sum() == 1 and got.index.max() == 300
    # duplicated rows: the first copy wins everywhere
    twice = np.concatenate([G.scene(1025)[8:], G.scene(1025)[8:]])
    got = image(twice, 64, 1024)
    assert got.index.max() < 1017 and (got.index >= 0).sum() > 300
    # every row loses to row 0: one cell, the nearest row first
    pts = (F32([10, 1, -1]) * rng.uniform(1.0, 3.0, (1025, 1))).astype(F32)
    pts[0] = F32([5, 0.5, -0.5])
    got = image(pts, 1, 4)
    assert got.index.flatten().tolist() == [0, -1, -1, -1] and got.binned == 1025
    got = image(pts[::-1].copy(), 1, 4)                                 # and last
    assert got.index.flatten().tolist() == [1024, -1, -1, -1]


def test_image_row_strides_shapes_not_served_and_no_launch(monkeypatch):
    pts = np.concatenate([G.scene(700), np.full((700, 1), 9e9, F32)], 1)                  # a fourth column that must not be read
    want = image(pts[:, :3], 16, 64)
    p4 = F(pts)
    elev, dirs = (torch.from_numpy(t).to(DEV) for t in ops.range_tables(16, 64, FIELD["elev_lo"], FIELD["elev_hi"]))
    index, dist2 = torch.full((16, 64), -7, dtype=torch.int32, device=DEV), torch.full((16, 64), -1.0, device=DEV)
    counts = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    nb = _lib.load().cmr_range_image_workspace_bytes(16, 64)
    ws = torch.empty((nb // 4,), dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    args = (elev.data_ptr(), dirs.data_ptr(), 1.0, 6400.0, index.data_ptr(), dist2.data_ptr(), counts.data_ptr(), ws.data_ptr(), nb, stream)
    _lib.call("cmr_range_image_f32", p4.data_ptr(), 4, 700, None, 16, 64, *args)
    assert torch.equal(index, want.index) and torch.equal(dist2.view(torch.int32), want.dist2.view(torch.int32)) and tuple(counts.tolist()) == tuple(want[2:])
    vis = torch.full((16, 64), 7, dtype=torch.uint8, device=DEV)
    for R, C in ((16, 62), (129, 4), (16, 2), (3, 4100)):                # no launch: the outputs are untouched
        assert _lib.call("cmr_range_image_f32", p4.data_ptr(), 4, 700, None, R, C, *args, allow_unsupported=True) == _lib.UNSUPPORTED
        assert _lib.call("cmr_range_visible_f32", dist2.data_ptr(), R, C, 1, 1, 1.0, vis.data_ptr(), stream, allow_unsupported=True) == _lib.UNSUPPORTED
    assert torch.equal(index, want.index) and (vis == 7).all()
    big, seen = torch.zeros((32, 64), device=DEV), torch.full((32, 64), 7, dtype=torch.uint8, device=DEV)
    for radius, factor in (((8, 32), 1.0), ((1, 1), 0.5), ((-1, 1), 1.0), ((1, 1), float("inf"))):      # a window of 17 x 64 > 1 024 cells, a factor below 1
        with pytest.raises(_lib.CmrError, match="invalid argument"):
            _lib.call("cmr_range_visible_f32", big.data_ptr(), 32, 64, radius[0], radius[1], factor, seen.data_ptr(), stream)
    assert (seen == 7).all()

    def touched(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", touched)
    empty = ops.range_image(torch.zeros((0, 3), device=DEV), None, 3, 8)
    assert empty[2:] == (0, 0, 0) and (empty.index == -1).all() and torch.isnan(empty.dist2).all() and empty.index.is_cuda
    scan = ops.virtual_scan(torch.zeros((0, 3), device=DEV), torch.eye(4, device=DEV), 3, 8)
    assert scan.rows.numel() == 0 and not scan.visible.any() and scan.visible.is_cuda


# ---- range_visible -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C", ((1, 4), (3, 8), (32, 512)))
def test_visible_on_hand_made_images(R, C):
    rng = np.random.default_rng(R)
    d = (rng.uniform(3, 80, (R, C)) ** 2).astype(F32)
    d[rng.uniform(size=(R, C)) < 0.3] = np.nan
    d[0, 0], d[0, C - 1] = 4, 100                                       # the column seam in the top row: 100 sits next to 4 across it
    if R > 1:
        d[R - 1, 0], d[R - 1, C - 1] = 101, 4.1                         # and in the bottom row, the other way round
    for radius in ((0, 0), (1, 1), (0, 1), (1, 0), (R + 5, 1), (2, 3), (0, C), (1000, 0)):
        got = visible(d, radius)
        if radius == (0, 0):
            assert torch.equal(got.cpu(), torch.from_numpy(~np.isnan(d)))                  # every winner is visible
        if radius[1] >= 1:
            assert got[0, 0] and not got[0, C - 1] and (R == 1 or (not got[R - 1, 0] and got[R - 1, C - 1]))
    visible(d, (1, 1), 0.0)
    visible(d, (1, 1), 3.0)
    assert not visible(np.full((R, C), np.nan, F32)).any()
    one = np.full((R, C), np.nan, F32)
    one[R // 2, C // 2] = 25
    assert visible(one, (R, 1)).sum() == 1
    # a value exactly m2 f is visible, the next float is not
    f = G.factor(0.05)
    for m2 in F32([4, 9.5, 6399.5, 1.0000001]):
        edge = m2 * f
        d = np.full((R, C), np.nan, F32)
        d[0, 0], d[0, 1], d[R - 1, C - 1] = m2, edge, np.nextafter(edge, F32(np.inf))
        d[0, C - 2] = np.nextafter(edge, F32(np.inf)) if C > 4 else np.nan                 # two columns from the nearest cell: out of its window
        got = visible(d, (R, 1))
        assert got[0, 0] and got[0, 1] and not got[R - 1, C - 1] and (C == 4 or got[0, C - 2])


def test_occlusion_scene():
    """A far wall behind a near one: without the window the far wall leaks through the gaps between the near wall's rows, with the 3 x 3
    window it does not, and the near wall's winners are all kept either way (the restatement's counts: 324 / 0 leaked, 1 669 kept)."""
    pts, near, hidden = G.occlusion_scene()
    kw = {k: v for k, v in G.OCCLUSION.items() if k not in ("rows", "cols")}
    p = F(pts)
    kept = {}
    for radius in ((0, 0), (1, 1)):
        got = ops.virtual_scan(p, None, G.OCCLUSION["rows"], G.OCCLUSION["cols"], radius=radius, rel_tol=0.05, **kw)
        again = ops.virtual_scan(p, None, G.OCCLUSION["rows"], G.OCCLUSION["cols"], radius=radius, rel_tol=0.05, **kw)
        rows, index, dist2, counts, vis = G.virtual_scan(pts, G.OCCLUSION["rows"], G.OCCLUSION["cols"], None, radius, 0.05, **kw)
        assert got.rows.dtype == torch.int64 and np.array_equal(got.rows.cpu().numpy(), rows) and (np.diff(rows) > 0).all()
        assert np.array_equal(got.image.index.cpu().numpy(), index) and same_bits(got.image.dist2, dist2) and tuple(got.image[2:]) == counts
        assert np.array_equal(got.visible.cpu().numpy(), vis) and torch.equal(got.rows, again.rows) and torch.equal(got.visible, again.visible)
        kept[radius] = got.rows.cpu().numpy()
        winners = index[index >= 0]
        assert near[kept[radius]].sum() == near[winners].sum() > 1000    # every near winner is kept
    print("hidden far rows kept: %d at radius (0, 0), %d at (1, 1); near winners kept %d" % (
        hidden[kept[(0, 0)]].sum(), hidden[kept[(1, 1)]].sum(), near[kept[(1, 1)]].sum()))
    assert hidden[kept[(0, 0)]].sum() > 0 and hidden[kept[(1, 1)]].sum() == 0


# ---- virtual_scan and the command ------------------------------------------------------------------------------------------------------------------
def test_virtual_scan_under_a_pose():
    pts = np.concatenate([G.scene(1025), G.room()[:3].T])
    pose = G.a_pose(2, (1.0, -0.5, 0.3))
    for R, C, radius in ((16, 64, (1, 1)), (64, 1024, (1, 1)), (64, 1024, (2, 3)), (3, 8, (0, 0))):
        got = ops.virtual_scan(F(pts), F(pose), R, C, radius=radius, rel_tol=0.1, **FIELD)
        rows, index, dist2, counts, vis = G.virtual_scan(pts, R, C, pose, radius, 0.1, **FIELD)
        assert np.array_equal(got.rows.cpu().numpy(), rows) and (np.diff(rows) > 0).all() and len(rows) > 3
        assert np.array_equal(got.visible.cpu().numpy(), vis) and np.array_equal(got.image.index.cpu().numpy(), index) and tuple(got.image[2:]) == counts


def test_view_command_through_the_files(tmp_path, capsys, monkeypatch):
    """python -m cmr_agent_amd.dataset.view on a three-frame synthetic sequence: x, y, z and reflectance of every file are the bits of
    ops.virtual_scan of the same inputs (and of the restatement), the normals are within 2^-21 of the float64 rotation (three products of
    unit-bounded terms, each rounded to 2^-24 of at most 1, and two sums), the loader reads the files, and they are kept without --overwrite."""
    root = str(tmp_path)
    view.main(G.view_argv(root))
    lines = capsys.readouterr().out.splitlines()
    ks = G.check_view_files(root)
    counts = [G.expected_view(j)[2] for j in range(3)]
    assert lines == ["view %d: rows %d of %d binned outside %d" % (G.VIEW["first"] + j, ks[j], counts[j][0], counts[j][2]) for j in range(3)] + \
        ["views: 3 frames, %d rows" % sum(ks)]
    cloud = G.room()
    folder = os.path.join(root, "vel", "sequences", "09", "map-view")
    field = dict(elev_lo=np.radians(G.VIEW["elev_lo_deg"]), elev_hi=np.radians(G.VIEW["elev_hi_deg"]), min_range=G.VIEW["min_range"], max_range=G.VIEW["max_range"])
    for j in range(3):
        inv = G.inverse_pose(G.room_poses()[j])
        scan = ops.virtual_scan(F(cloud[:3].T), F(inv), G.VIEW["rows"], G.VIEW["cols"], **field)
        keep = scan.rows.cpu().numpy()
        got = np.load(os.path.join(folder, "%06d.npy" % (G.VIEW["first"] + j)))
        assert np.array_equal(G.bits(got[:3]), G.bits(G.pose_apply(cloud[:3].T[keep], inv).T)) and np.array_equal(G.bits(got[3]), G.bits(cloud[3, keep]))
    # kept without --overwrite, written again with it
    path = os.path.join(folder, "%06d.npy" % (G.VIEW["first"] + 1))
    np.save(path, np.zeros((7, 1), F32))
    view.main(G.view_argv(root))
    assert capsys.readouterr().out.splitlines() == ["views: 0 frames, 0 rows"] and np.load(path).shape == (7, 1)
    view.main(G.view_argv(root, "--overwrite"))
    assert capsys.readouterr().out.splitlines()[-1] == "views: 3 frames, %d rows" % sum(ks) and G.check_view_files(root) == ks
    # the loader reads them: FrameDataset(..., pc_subdir=...)
    from cmr_agent_amd.config.KittiConfig import KittiConfiguration
    from cmr_agent_amd.dataset import loader
    cfg = KittiConfiguration(None)
    cfg.data_velodyne, cfg.data_color = "vel", "col"
    img = os.path.join(root, cfg.data_color, "sequences", "09", "image_2")
    os.makedirs(img)
    for i in range(G.VIEW["first"] + 3):
        np.save(os.path.join(img, "%06d.npy" % i), np.zeros((2 * cfg.cropped_img_H, 2 * cfg.cropped_img_W, 3), np.uint8) if i == G.VIEW["first"] + 2 else np.zeros(1))
    K = np.array([[700.0, 0, 600.0], [0, 700.0, 180.0], [0, 0, 1.0]], F32)
    monkeypatch.setattr(loader, "read_calib", lambda r: {9: {"P2": np.eye(4), "P2_K": K, "Tr": np.eye(4)}})
    ds = loader.FrameDataset(root, cfg, "test", pc_subdir="map-view")
    assert len(ds) == G.VIEW["first"] + 3
    raw = ds.read_frame(G.VIEW["first"] + 2)["raw"]
    assert raw.shape == (7, ks[2]) and np.array_equal(G.bits(raw[:4]), G.bits(G.expected_view(2)[0]))
