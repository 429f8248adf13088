"""CPU tier of the cloud preparation (ops.voxel_downsample / ops.point_normals, cmr_agent_amd/dataset/prepare.py, FrameDataset's from_raw,
--from-raw): the restatement on inputs computed by hand, the conditions on the scenes that let the GPU tier assert its bars,
every argument check of the two ops ahead of the library, the file layer with the restatement in the ops' place, and the flag rules."""
import argparse
import os
import random

import numpy as np
import pytest
import torch

import cases as C
import cloud_prepare_reference as R
from cmr_agent_amd import _lib, ops
from cmr_agent_amd.dataset import prepare
from cmr_agent_amd.utils import evalcli


# ---- the restatement on hand-checked inputs ---------------------------------------------------------------------------------------------
def test_five_points_in_two_voxels():
    # voxel 1, origin = minimum - 0.5 = (-0.5, -0.5, -0.5): x in [-0.5, 0.5) is cell 0, [0.5, 1.5) is cell 1
    p = np.array([[0.0, 0.0, 0.0], [1.0, 0.25, 0.0], [0.25, 0.25, 0.25], [0.75, 0.0, 0.25], [0.25, 0.0, 0.0]], np.float32)
    a = np.array([[1.0], [2.0], [3.0], [4.0], [5.0]], np.float32)
    d = R.voxel_downsample(p, a, voxel=1.0)
    assert d["keys"].tolist() == [0, 1] and d["count"].tolist() == [3, 2] and d["inverse"].tolist() == [0, 1, 0, 1, 0] and d["dropped"] == 0
    assert np.array_equal(d["points"], [[0.5 / 3, 0.25 / 3, 0.25 / 3], [0.875, 0.125, 0.125]])
    assert np.array_equal(d["attr"], [[3.0], [3.0]])
    assert np.array_equal(d["origin"], np.float32([-0.5, -0.5, -0.5]))
    # a dropped row keeps its place in `inverse`; the origin comes from the kept rows
    q = np.concatenate([p[:2], [[np.nan, 0, 0]], p[2:], [[0, np.inf, 0]]]).astype(np.float32)
    e = R.voxel_downsample(q, None, voxel=1.0)
    assert e["inverse"].tolist() == [0, 1, -1, 0, 1, 0, -1] and e["dropped"] == 2 and np.array_equal(e["points"], d["points"])
    # the key packs z above y above x
    k, _, cells = R.voxel_keys(np.float32([[0, 0, 0], [1, 2, 3]]), voxel=1.0)
    assert cells.tolist() == [[0, 0, 0], [1, 2, 3]] and k.tolist() == [0, 3 << 42 | 2 << 21 | 1]


def test_points_on_cell_faces_pin_the_floor_convention():
    # voxel 0.125 and coordinates that are multiples of it: fp32 is exact.  With the origin at a multiple of the voxel a point ON a face
    # belongs to the cell above it (floor), and the default origin (minimum - voxel / 2) puts every such point mid-cell.
    v = 0.125
    p = np.float32([[0, 0, 0], [v, 0, 0], [2 * v, 0, 0], [-v, -v, -v], [v, v, v]])
    k, o, cells = R.voxel_keys(p, voxel=v, origin=(-v, -v, -v))
    assert cells.tolist() == [[1, 1, 1], [2, 1, 1], [3, 1, 1], [0, 0, 0], [2, 2, 2]]
    k2, o2, cells2 = R.voxel_keys(p, voxel=v)
    assert np.array_equal(o2, np.float32([-1.5 * v] * 3)) and cells2.tolist() == cells.tolist()
    with pytest.raises(ValueError):
        R.voxel_keys(p, voxel=v, origin=(0, 0, 0))                         # a kept row below the origin
    with pytest.raises(ValueError):
        R.voxel_keys(np.float32([[0, 0, 0], [1e7, 0, 0]]), voxel=1.0)      # 10^7 cells > 2^21


def test_planar_patch_three_points_and_two_points():
    g = np.arange(5, dtype=np.float32) * 0.1
    patch = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    patch = np.concatenate([patch, np.full((25, 1), 2.0, np.float32)], 1).astype(np.float32)
    up = R.point_normals(patch, radius=0.6, viewpoint=(0, 0, 10))
    down = R.point_normals(patch, radius=0.6, viewpoint=(0, 0, -10))
    assert np.array_equal(up["count"], np.full(25, 25)) and not up["zero"].any()
    assert np.allclose(up["normals"], [0, 0, 1], atol=1e-12) and np.allclose(down["normals"], [0, 0, -1], atol=1e-12)
    assert np.abs(up["eigenvalues"][:, 0]).max() < 1e-15 and np.allclose(up["eigenvalues"][:, 1:], 0.02, atol=1e-9)   # var of {0, .1, .., .4}
    three = R.point_normals(np.float32([[0, 0, 1], [0.1, 0, 1], [0, 0.1, 1]]), radius=0.6)
    assert three["count"].tolist() == [3, 3, 3] and not three["zero"].any() and np.allclose(three["normals"], [0, 0, -1], atol=1e-7)
    two = R.point_normals(np.float32([[0, 0, 1], [0.1, 0, 1]]), radius=0.6)
    assert two["count"].tolist() == [2, 2] and two["zero"].all() and not two["normals"].any()
    assert R.point_normals(np.float32([[0, 0, 1], [0.1, 0, 1], [0, 0.1, 1]]), radius=0.6, min_neighbors=4)["zero"].all()
    # the radius is inclusive, in float32 as stated: 0.5 is exact
    edge = R.point_normals(np.float32([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.75]]), radius=0.5)
    assert edge["count"].tolist() == [3, 2, 2, 1] and edge["near"].tolist() == [True, True, True, False]
    # a non-finite row is nobody's neighbour and gets the zero normal
    nf = R.point_normals(np.float32([[0, 0, 1], [0.1, 0, 1], [0, 0.1, 1], [np.nan, 0, 0]]), radius=0.6)
    assert nf["count"].tolist() == [3, 3, 3, 0] and nf["zero"].tolist() == [False, False, False, True]


def test_brute_force_neighbourhoods_agree_with_a_kd_tree():
    from scipy.spatial import cKDTree
    case = R.scene_case(R.SEEDS[0])
    q, ref = case["cloud"].astype(np.float64), case["normals"]
    cnt = np.array([len(l) for l in cKDTree(q).query_ball_point(q, float(np.float32(R.RADIUS)))])
    differ = cnt != ref["count"]
    assert not (differ & ~ref["near"]).any()                               # float64 against float32 membership: only on the radius


# ---- the scenes carry what the GPU tier's bars assume -----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.SEEDS)
def test_scene_conditions(seed):
    case = R.scene_case(seed)
    down, ref = case["down"], case["normals"]
    share = R.excluded_share(ref)
    print("seed %d: raw %d voxels %d most rows per voxel %d neighbours <= %d rows with < 3 neighbours %d excluded share %.4f" % (
        seed, case["raw"].shape[0], down["count"].size, down["count"].max(), ref["count"].max(), (ref["count"] < 3).sum(), share))
    assert share <= 0.02
    assert down["count"].max() >= 16
    assert (ref["count"] < 3).sum() >= 1
    assert ref["count"].max() >= 256
    assert R.cell_disagreements(case["raw"][:, :3]) == 0
    assert 3000 <= down["count"].size < case["raw"].shape[0]


def test_far_case_reaches_the_walks_second_pass():
    """What the GPU tier's far-cloud cases assume: the rows of the second cluster search more than 16 runs (a 16-lane group's second pass,
    csrc/cmr_cloud_grid.h walk16) or exactly 16, and every row is compared -- none near the radius, none without a normal."""
    case = R.far_case()
    cloud, ref = case["cloud"], case["normals"]
    runs = R.walk_runs(cloud, R.FAR_RADIUS)
    assert cloud.shape == (120, 3) and set(runs[60:].tolist()) == {16, 20, 25} and (runs[60:] > 16).sum() >= 30 and runs[:60].max() <= 9
    assert not ref["near"].any() and not ref["zero"].any() and R.excluded_share(ref) == 0 and R.kept_rows(ref).all()
    assert R.walk_runs(R.scene_case(R.SEEDS[0])["cloud"], R.RADIUS).max() <= 16                    # no row of a scene gets there


def test_fp32_sums_sit_inside_the_angle_bar():
    """The bar the GPU tier asserts (4 k 2^-24 / gap) against an emulation of what a kernel may do: covariance sums in float32,
    accumulated row by row, the solve in float64."""
    case = R.scene_case(R.SEEDS[0])
    q, ref = case["cloud"], case["normals"]
    keep = np.nonzero(R.kept_rows(ref))[0][::7]
    r32 = np.float32(R.RADIUS)
    worst = 0.0
    for i in keep:
        d = q - q[i]
        d = d[(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r32 * r32]
        k = d.shape[0]
        s1 = np.cumsum(d, 0, dtype=np.float32)[-1].astype(np.float64)
        s2 = np.cumsum(d[:, :, None] * d[:, None, :], 0, dtype=np.float32)[-1].astype(np.float64)
        m = s1 / k
        w, v = np.linalg.eigh(s2 / k - np.outer(m, m))
        worst = max(worst, float(R.angle(v[:, 0][None], ref["normals"][i][None])[0] / R.angle_bound(ref)[i]))
    print("fp32 sums: worst angle / bar = %.3f over %d rows" % (worst, keep.size))
    assert worst <= 0.25


# ---- argument checks: every one raises before the library is reached --------------------------------------------------------------------
def _touched(*a, **k):
    raise AssertionError("the library was reached")


def test_argument_checks(monkeypatch):
    monkeypatch.setattr(_lib, "load", _touched)
    monkeypatch.setattr(_lib, "call", _touched)
    p = torch.zeros((8, 3))
    for bad in (torch.zeros((8, 2)), torch.zeros((8, 4)), torch.zeros((8,)), torch.zeros((2, 8, 3)), torch.zeros((8, 3), dtype=torch.float64),
                torch.zeros((8, 3), dtype=torch.int64), None, np.zeros((8, 3), np.float32)):
        with pytest.raises(ValueError, match="points must be a float32"):
            ops.voxel_downsample(bad)
        with pytest.raises(ValueError, match="points must be a float32"):
            ops.point_normals(bad)
    with pytest.raises(ValueError, match="device tensor"):                 # a well-formed CPU tensor: there is no CPU path
        ops.voxel_downsample(p)
    with pytest.raises(ValueError, match="device tensor"):
        ops.point_normals(p)
    for bad in (0.0, -0.1, float("inf"), float("nan"), 1e-50, 1e39):
        with pytest.raises(ValueError, match="voxel must be a finite number > 0"):
            ops.voxel_downsample(p, voxel=bad)
        with pytest.raises(ValueError, match="radius must be a finite number > 0"):
            ops.point_normals(p, radius=bad)
    for bad in (torch.zeros((7, 1)), torch.zeros((9, 0))):
        with pytest.raises(ValueError, match="attr has"):
            ops.voxel_downsample(p, bad)
    for bad in (torch.zeros((8,)), torch.zeros((8, 1), dtype=torch.float64), np.zeros((8, 1), np.float32)):
        with pytest.raises(ValueError, match="attr must be a float32"):
            ops.voxel_downsample(p, bad)
    for bad in ((0, 0), (0, 0, 0, 0), 1.0, (0, float("nan"), 0), (0, 0, float("inf"))):
        with pytest.raises(ValueError, match="viewpoint must be three"):
            ops.point_normals(p, viewpoint=bad)
        with pytest.raises(ValueError, match="origin must be three"):
            ops.voxel_downsample(p, origin=bad)


def test_header_declares_the_entry_points():
    protos = _lib.parse_header()
    for name in ("cmr_cloud_bounds_f32", "cmr_voxel_keys_f32", "cmr_segment_heads_i64", "cmr_point_normals_f32"):
        assert name in protos, name
    assert protos["cmr_voxel_keys_f32"][2] == ["points", "ld", "N", "ox", "oy", "oz", "cell", "keys", "stream"]


# ---- prepare.py -------------------------------------------------------------------------------------------------------------------------
def test_bin_round_trip_and_subdir(tmp_path):
    from cmr_agent_amd.dataset import FrameDataset
    raw = R.scene(5)[:100].T.copy()
    path = str(tmp_path / "000003.bin")
    R.write_bin(path, raw)
    back = prepare.read_velodyne_bin(path)
    assert back.dtype == np.float32 and back.shape == (4, 100) and np.array_equal(back, raw) and back.flags["C_CONTIGUOUS"]
    with open(path, "ab") as fh:
        fh.write(b"\0" * 4)
    with pytest.raises(ValueError, match="not rows of"):
        prepare.read_velodyne_bin(path)
    assert prepare.subdir() == prepare.subdir(0.1, 0.6) == "voxel0.1-SNr0.6" == FrameDataset.PC_SUBDIR
    assert prepare.subdir(0.25, 1) == "voxel0.25-SNr1"


def test_prepare_sequence_writes_what_the_loader_reads(tmp_path, monkeypatch, capsys):
    """The file layer with the restatement in the ops' place: no GPU."""
    from cmr_agent_amd.config import KittiConfiguration
    from cmr_agent_amd.dataset import loader
    monkeypatch.setattr(ops, "voxel_downsample", R.ops_voxel_downsample)
    monkeypatch.setattr(ops, "point_normals", R.ops_point_normals)
    root = str(tmp_path)
    vel, raws = R.write_raw_tree(root)
    f = C.FRAME
    cfg = KittiConfiguration(cropped_img_H=f["H"], cropped_img_W=f["W"], num_pt=f["num_pt"], device="cpu")
    assert len(loader.FrameDataset(root, cfg, "val", device="cpu")) == 0                    # raw scans alone are not listed ...
    listed = loader.FrameDataset(root, cfg, "val", device="cpu", from_raw=True)             # ... unless asked for
    assert len(listed) == 2 and os.path.basename(listed.frames[0][1]) == "velodyne"

    out = os.path.join(os.path.dirname(vel), prepare.subdir())
    assert prepare.prepare_sequence(vel, out, device="cpu")[0] == 2
    assert sorted(os.listdir(out)) == ["000000.npy", "000001.npy"]
    assert prepare.prepare_sequence(vel, out, device="cpu")[0] == 0                          # kept unless overwrite
    frames, n_raw, n_kept = prepare.prepare_sequence(vel, out, device="cpu", overwrite=True)
    assert (frames, n_raw) == (2, sum(r.shape[1] for r in raws))
    clouds = [np.load(os.path.join(out, "%06d.npy" % i)) for i in range(2)]
    assert n_kept == sum(c.shape[1] for c in clouds)
    for raw, cloud in zip(raws, clouds):
        d = R.voxel_downsample(raw[:3].T, raw[3:4].T)
        assert cloud.dtype == np.float32 and cloud.shape == (7, d["count"].size)
        assert np.array_equal(cloud[:3], d["points"].astype(np.float32).T) and np.array_equal(cloud[3], d["attr"][:, 0].astype(np.float32))
        nrm = np.linalg.norm(cloud[4:7].astype(np.float64), axis=0)
        assert np.all((np.abs(nrm - 1) < 1e-6) | (nrm == 0)) and (nrm > 0).mean() > 0.9
        assert np.all((cloud[4:7] * -cloud[:3]).sum(0) >= -1e-6)                             # turned towards the sensor origin
    four = prepare.prepare_cloud(raws[0], normals=False, device="cpu")
    assert four.shape == (4, clouds[0].shape[1]) and np.array_equal(four.numpy(), clouds[0][:4])

    # the loader lists and reads the written folder, and prefers it to the raw scans
    for kw in ({}, dict(from_raw=True)):
        ds = loader.FrameDataset(root, cfg, "val", device="cpu", **kw)
        assert len(ds) == 2 and os.path.basename(ds.frames[0][1]) == prepare.subdir()
        random.seed(3)
        np.random.seed(3)
        fr = ds.read_frame(1)
        assert np.array_equal(fr["raw"], clouds[1]) and fr["choice"].shape == (f["num_pt"],) and fr["choice"].max() < clouds[1].shape[1]
    # from_raw prepares the same rows 0-3 on the fly
    random.seed(3)
    np.random.seed(3)
    fr_raw = listed.read_frame(1)
    assert np.array_equal(fr_raw["raw"], clouds[1][:4]) and np.array_equal(fr_raw["choice"], fr["choice"])

    # the command line: one line per sequence
    capsys.readouterr()
    prepare.main(["--root", root, "--sequences", "9", "--overwrite"], device="cpu")
    assert capsys.readouterr().out == "sequence 09: prepared 2 frames, %d -> %d points\n" % (n_raw, n_kept)
    prepare.main(["--root", root], device="cpu")                                                           # every sequence found; nothing to do
    assert capsys.readouterr().out == "sequence 09: prepared 0 frames, 0 -> 0 points\n"
    prepare.main(["--root", root, "--no-normals", "--voxel", "0.2", "--sn-radius", "1"], device="cpu")
    assert np.load(os.path.join(os.path.dirname(vel), "voxel0.2-SNr1", "000000.npy")).shape[0] == 4
    with pytest.raises(SystemExit):
        prepare.main(["--root", root, "--sequences", "10"])                                  # no such sequence on disk


def test_prepare_flag_rules(tmp_path):
    for argv in (["--root", "d", "--voxel", "0"], ["--root", "d", "--voxel", "nan"], ["--root", "d", "--sn-radius", "-1"],
                 ["--root", "d", "--sn-radius", "inf"], ["--root", "d", "--sequences", "9,x"], ["--root", "d", "--sequences", "100"],
                 ["--voxel", "0.1"], ["--root", str(tmp_path / "missing")]):
        with pytest.raises(SystemExit):
            prepare.main(argv)
    _, args = prepare.parse_args(["--root", "d", "--sequences", "9,10"])
    assert args.sequences == (9, 10) and args.voxel == 0.1 and args.sn_radius == 0.6 and not args.no_normals and not args.overwrite
    assert args.data_velodyne == "data_odometry_velodyne_NWU/"


def test_from_raw_flag_placement():
    def parse(*argv):
        ap = argparse.ArgumentParser()
        ap.add_argument("--data-root", default=None)
        evalcli.add_raw_flag(ap)
        return evalcli.raw_option(ap, ap.parse_args(list(argv)))

    assert parse() == {} and parse("--data-root", "d") == {}
    assert parse("--from-raw", "--data-root", "d") == dict(from_raw=True)
    with pytest.raises(SystemExit):
        parse("--from-raw")                                                                  # synthetic pairs have no files
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for script in ("Test_Geo.py", "Test_Agent.py"):
        src = open(os.path.join(root, script)).read()
        assert "add_raw_flag(ap)" in src and "raw_option(ap, args)" in src and "**raw_kw" in src, script
