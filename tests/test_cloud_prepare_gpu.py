"""GPU tier of the cloud preparation (ops.voxel_downsample / ops.point_normals, csrc/cloud_prepare.hip, dataset/prepare.py, FrameDataset's
from_raw), against the restatement of cloud_prepare_reference.py.

Downsample: every integer -- the number of voxels, their order, count, inverse, dropped -- is EXACT (the keys are stated in fp32 operation by
operation); a mean is within count * 2^-23 * max|value in the voxel| of the float64 mean (a sequential fp32 sum of `count` terms and one
division).  Normals, on the rows the restatement keeps (gap >= 1e-2, no neighbour on the radius, orientation decided; at most 2 % are
excluded, asserted): angle <= 4 k 2^-24 / gap, unit length to 1e-5, the exact orientation sign, eigenvalues within 4 k 2^-24 l2; the count
is exact on every row without a neighbour on the radius, and the zero normal sits exactly where the restatement puts it."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases as C
import cloud_prepare_reference as R
from cmr_agent_amd import ops
from cmr_agent_amd.dataset import prepare

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)      # noqa: E731


# ---- downsample -------------------------------------------------------------------------------------------------------------------------
def _check_downsample(points, attr=None, voxel=R.VOXEL, origin=None, ref=None):
    ref = R.voxel_downsample(points, attr, voxel, origin) if ref is None else ref
    got = ops.voxel_downsample(F(points).view(-1, 3), None if attr is None else F(attr).view(len(points), attr.shape[1]), voxel=voxel, origin=origin,
                               want_inverse=True)
    n = ref["count"].size
    assert got.points.shape == (n, 3) and got.points.dtype == torch.float32 and got.count.dtype == torch.int32
    assert got.dropped == ref["dropped"]
    assert np.array_equal(got.count.cpu().numpy(), ref["count"])
    assert got.inverse.dtype == torch.int64 and np.array_equal(got.inverse.cpu().numpy(), ref["inverse"])
    if n:
        assert np.array_equal(np.float32(got.origin), ref["origin"])
    worst = 0.0
    pairs = [(got.points, "points")] + ([] if attr is None else [(got.attr, "attr")])
    for out, name in pairs:
        assert out.shape == ref[name].shape
        err = np.abs(out.cpu().numpy().astype(np.float64) - ref[name])
        bound = ref["count"][:, None] * 2.0 ** -23 * ref["absmax_" + name]
        assert np.all(err <= bound), (name, float((err - bound).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0)
    if attr is None:
        assert got.attr is None
    return got, ref, worst


@pytest.mark.parametrize("seed", R.SEEDS)
def test_downsample_scenes(seed):
    case = R.scene_case(seed)
    raw = case["raw"]
    got, ref, worst = _check_downsample(raw[:, :3], raw[:, 3:4], ref=case["down"])
    print("seed %d: %d -> %d voxels, worst mean error / bound %.3f" % (seed, raw.shape[0], got.points.shape[0], worst))
    assert ops.voxel_downsample(F(raw[:, :3])).inverse is None


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1023, 1024, 1025])
@pytest.mark.parametrize("Cn", [0, 1, 4])
def test_downsample_small_sizes(N, Cn):
    r = np.random.default_rng(100 + N)
    p = r.uniform(-0.4, 0.4, (N, 3)).astype(np.float32)
    a = r.uniform(-2, 2, (N, Cn)).astype(np.float32)
    got, ref, _ = _check_downsample(p, a)
    assert got.attr.shape == (ref["count"].size, Cn)


def test_downsample_layouts():
    r = np.random.default_rng(5)
    # all points in one voxel; every point its own voxel
    one = r.uniform(0.0, 0.05, (200, 3)).astype(np.float32)
    got, ref, _ = _check_downsample(one, None, voxel=1.0)
    assert got.count.tolist() == [200]
    g = np.arange(7, dtype=np.float32) * 0.25
    own = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[r.permutation(343)]
    got, ref, _ = _check_downsample(own, own[:, :1].copy())
    assert got.points.shape[0] == 343 and torch.equal(got.points, F(own)[torch.argsort(got.inverse)])
    # negative coordinates only, and a caller's origin
    neg = (r.uniform(-3, -1, (500, 3))).astype(np.float32)
    _check_downsample(neg, neg[:, :2].copy())
    _check_downsample(neg, None, voxel=0.25, origin=(-3.5, -4.0, -3.25))
    # points exactly on cell faces: voxel 0.125, coordinates that are multiples of it (fp32 exact), origin on the lattice
    v = 0.125
    face = (r.integers(-8, 9, (400, 3)) * v).astype(np.float32)
    got, ref, _ = _check_downsample(face, None, voxel=v, origin=(-1.0, -1.0, -1.0))
    assert got.points.shape[0] == len(np.unique(face, axis=0))
    _check_downsample(face, None, voxel=v)
    # NaN and inf rows are dropped, wherever they are
    bad = R.scene(3, n=800, clump=50, far=5)
    for row, col, val in ((0, 0, np.nan), (17, 1, np.inf), (18, 2, -np.inf), (400, 0, np.nan), (len(bad) - 1, 2, np.nan)):
        bad[row, col] = val
    got, ref, _ = _check_downsample(bad[:, :3], bad[:, 3:4])
    assert got.dropped == 5 and (got.inverse == -1).sum().item() == 5
    # nothing kept
    for pts in (np.zeros((0, 3), np.float32), np.full((5, 3), np.nan, np.float32)):
        got = ops.voxel_downsample(F(pts).view(-1, 3), F(np.zeros((len(pts), 2))).view(-1, 2), want_inverse=True)
        assert got.points.shape == (0, 3) and got.attr.shape == (0, 2) and got.count.shape == (0,) and got.dropped == len(pts)
        assert got.inverse.tolist() == [-1] * len(pts)


def test_downsample_many_tiles():
    """More than 256 scan tiles of 1024 rows and more rows than the bounds kernel's grid covers in one stride."""
    r = np.random.default_rng(9)
    p = r.uniform(-1.5, 1.5, (300001, 3)).astype(np.float32)
    got, ref, _ = _check_downsample(p, p[:, :1].copy())
    assert got.points.shape[0] > 20000


def test_key_range_errors():
    far = F(np.float32([[0, 0, 0], [1e7, 0, 0]]))
    with pytest.raises(ValueError, match="2\\^21"):
        ops.voxel_downsample(far, voxel=1.0)
    with pytest.raises(ValueError, match="2\\^21"):
        ops.point_normals(far, radius=1.0)
    with pytest.raises(ValueError, match="origin"):
        ops.voxel_downsample(far, voxel=1e3, origin=(1.0, 0.0, 0.0))
    assert ops.voxel_downsample(far, voxel=8.0).points.shape[0] == 2               # 1 250 000 cells fit


# ---- normals ----------------------------------------------------------------------------------------------------------------------------
def _check_normals(points, ref, got, what="", max_excluded=None):
    nrm = got.normals.cpu().numpy().astype(np.float64)
    cnt = got.count.cpu().numpy()
    eig = got.eigenvalues.cpu().numpy().astype(np.float64)
    assert np.array_equal(cnt[~ref["near"]], ref["count"][~ref["near"]])
    sure = ~ref["near"]                                                     # a neighbour on the radius may move a row across min_neighbors
    assert not nrm[ref["zero"] & sure].any() and not eig[ref["zero"] & sure].any()
    assert np.all(np.linalg.norm(nrm[~ref["zero"] & sure], axis=1) > 0.5)
    keep = R.kept_rows(ref)
    share = R.excluded_share(ref)
    assert max_excluded is None or share <= max_excluded
    ang, bound = R.angle(nrm[keep], ref["normals"][keep]), R.angle_bound(ref)[keep]
    assert np.all(ang <= bound), float((ang / bound).max())
    assert np.abs(np.linalg.norm(nrm[keep], axis=1) - 1.0).max() <= 1e-5
    assert np.all((nrm[keep] * ref["normals"][keep]).sum(1) > 0)            # the orientation sign
    ebound = 4.0 * ref["count"][keep, None] * R.U24 * ref["eigenvalues"][keep, 2:3]
    eerr = np.abs(eig[keep] - ref["eigenvalues"][keep])
    assert np.all(eerr <= ebound), float((eerr / ebound).max())
    assert np.all(np.diff(eig, axis=1) >= 0)
    print("%s: %d rows, %d compared (excluded share %.4f), worst angle / bound %.4f (%.2e rad), worst eigenvalue error / bound %.4f" % (
        what, len(points), keep.sum(), share, float((ang / bound).max()), float(ang.max()), float((eerr / ebound).max())))
    return nrm, cnt


@pytest.mark.parametrize("seed", R.SEEDS)
def test_normals_scenes(seed):
    case = R.scene_case(seed)
    got = ops.point_normals(F(case["cloud"]), want_eigenvalues=True)
    assert got.normals.shape == (len(case["cloud"]), 3) and got.count.dtype == torch.int32
    _check_normals(case["cloud"], case["normals"], got, "seed %d" % seed, max_excluded=0.02)
    again = ops.point_normals(F(case["cloud"]), want_eigenvalues=True)
    assert torch.equal(got.normals, again.normals) and torch.equal(got.count, again.count) and torch.equal(got.eigenvalues, again.eigenvalues)
    assert ops.point_normals(F(case["cloud"])).eigenvalues is None


def test_normals_far_from_the_origin_take_the_walks_second_pass():
    """Rows beyond 2^19 cells from the grid's origin search 20 or 25 runs, more than the 16 lanes of a group take in one pass
    (tests/test_cloud_prepare_cpu.py asserts that of the case).  Every row is compared."""
    case = R.far_case()
    got = ops.point_normals(F(case["cloud"]), radius=R.FAR_RADIUS, want_eigenvalues=True)
    _check_normals(case["cloud"], case["normals"], got, "far cloud", max_excluded=0)


def test_normals_of_a_permuted_cloud():
    case = R.scene_case(R.SEEDS[0])
    cloud, ref = case["cloud"], case["normals"]
    perm = np.random.default_rng(1).permutation(len(cloud))
    got = ops.point_normals(F(cloud[perm]), want_eigenvalues=True)
    base = ops.point_normals(F(cloud))
    inv = np.argsort(perm)
    assert torch.equal(got.count[torch.from_numpy(inv).to(DEV)], base.count)           # membership does not depend on the order
    back = ops.PointNormals(got.normals[torch.from_numpy(inv).to(DEV)], got.count[torch.from_numpy(inv).to(DEV)],
                            got.eigenvalues[torch.from_numpy(inv).to(DEV)])
    _check_normals(cloud, ref, back, "permuted", max_excluded=0.02)


def test_normals_other_arguments():
    """Another radius, viewpoint and min_neighbors; non-finite rows; queries in cell 0 of every axis; a cloud inside one cell."""
    r = np.random.default_rng(21)
    pts = np.concatenate([np.zeros((1, 3)), r.uniform(0, 2, (400, 3)) * [1, 1, 0.05], r.uniform(0, 0.3, (60, 3)) + [3, 3, 3],
                          r.uniform(0, 0.2, (5, 3)) + [10, 10, 10]]).astype(np.float32)        # five neighbours: fewer than min_neighbors
    pts[50] = np.nan
    pts[51, 1] = np.inf
    ref = R.point_normals(pts, radius=0.35, viewpoint=(1.0, 1.0, 4.0), min_neighbors=6)
    got = ops.point_normals(F(pts), radius=0.35, viewpoint=(1.0, 1.0, 4.0), min_neighbors=6, want_eigenvalues=True)
    nrm, cnt = _check_normals(pts, ref, got, "radius 0.35")
    assert cnt[50] == 0 and cnt[51] == 0 and not nrm[50:52].any() and np.isfinite(nrm).all()
    assert ((ref["count"] >= 3) & (ref["count"] < 6)).any() and ref["zero"][ref["count"] < 6].all()
    one_cell = r.uniform(0, 0.1, (40, 3)).astype(np.float32) + np.float32([5, -5, 1])
    ref = R.point_normals(one_cell)
    got = ops.point_normals(F(one_cell), want_eigenvalues=True)
    assert got.count.tolist() == [40] * 40
    _check_normals(one_cell, ref, got, "one cell")


def test_normals_on_a_lattice_of_the_radius():
    """Coordinates that are multiples of the radius 0.5 (fp32 exact): every query sits on a cell face and its six lattice neighbours are at
    exactly the radius, which is inclusive.  The count is exact here although every row is `near`."""
    g = np.arange(5, dtype=np.float32) * 0.5
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) - np.float32(1.0)
    ref = R.point_normals(pts, radius=0.5)
    got = ops.point_normals(F(pts), radius=0.5, want_eigenvalues=True)
    assert ref["near"].all() and ref["count"].max() == 7 and ref["count"].min() == 4
    assert np.array_equal(got.count.cpu().numpy(), ref["count"])
    assert torch.isfinite(got.normals).all()


def test_normals_edge_cases():
    for n in (1, 2, 3):
        pts = np.float32([[0, 0, 1], [0.1, 0, 1], [0, 0.1, 1]])[:n]
        got = ops.point_normals(F(pts).view(-1, 3), want_eigenvalues=True)
        assert got.count.tolist() == [n] * n
        if n < 3:
            assert not got.normals.any() and not got.eigenvalues.any()
        else:
            assert torch.allclose(got.normals, F([[0, 0, -1]] * 3), atol=1e-6)
    got = ops.point_normals(F(np.zeros((0, 3))).view(-1, 3), want_eigenvalues=True)
    assert got.normals.shape == (0, 3) and got.count.shape == (0,) and got.eigenvalues.shape == (0, 3)
    got = ops.point_normals(F(np.full((4, 3), np.nan)))
    assert not got.normals.any() and not got.count.any()
    # all points coincident: a degenerate covariance gives a finite unit vector (or zero)
    got = ops.point_normals(F(np.tile(np.float32([[1.5, -2.0, 0.25]]), (10, 1))), want_eigenvalues=True)
    length = got.normals.double().norm(dim=1)
    assert got.count.tolist() == [10] * 10 and torch.isfinite(got.normals).all() and bool((((length - 1).abs() < 1e-5) | (length == 0)).all())
    assert not got.eigenvalues.any()
    # a planar patch: (0, 0, +-1), the sign set by the viewpoint
    g = np.arange(5, dtype=np.float32) * 0.1
    patch = np.concatenate([np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2), np.full((25, 1), 2.0)], 1).astype(np.float32)
    for z, sign in ((10.0, 1.0), (-10.0, -1.0)):
        got = ops.point_normals(F(patch), viewpoint=(0, 0, z))
        assert torch.allclose(got.normals, F([[0, 0, sign]] * 25), atol=1e-6) and got.count.tolist() == [25] * 25


def test_downsample_is_repeatable():
    raw = R.scene_case(R.SEEDS[1])["raw"]
    a = ops.voxel_downsample(F(raw[:, :3]), F(raw[:, 3:4]), want_inverse=True)
    b = ops.voxel_downsample(F(raw[:, :3]), F(raw[:, 3:4]), want_inverse=True)
    assert all(torch.equal(x, y) for x, y in ((a.points, b.points), (a.attr, b.attr), (a.count, b.count), (a.inverse, b.inverse)))


# ---- the file layer ---------------------------------------------------------------------------------------------------------------------
def test_prepare_cloud_is_the_composition_of_the_two_ops():
    raw = R.scene_case(R.SEEDS[2])["raw"]
    cloud = prepare.prepare_cloud(raw.T.copy())
    down = ops.voxel_downsample(F(raw[:, :3]), F(raw[:, 3:4]), voxel=0.1)
    nrm = ops.point_normals(down.points, radius=0.6, viewpoint=(0, 0, 0)).normals
    assert cloud.is_cuda and cloud.shape == (7, down.points.shape[0]) and cloud.is_contiguous()
    assert torch.equal(cloud[0:3], down.points.t()) and torch.equal(cloud[3], down.attr[:, 0]) and torch.equal(cloud[4:7], nrm.t())
    assert torch.equal(prepare.prepare_cloud(torch.from_numpy(raw.T.copy()), normals=False), cloud[0:4])


def test_from_raw_equals_the_prepared_files(tmp_path):
    """FrameDataset(from_raw=True) on two raw scans against FrameDataset on the files the command line wrote from them: the same samples,
    key for key, under the same seeds.  The command line runs as a child process under its own time limit; its line is checked."""
    from cmr_agent_amd.config import KittiConfiguration
    from cmr_agent_amd.dataset import FrameDataset
    root = str(tmp_path)
    vel, raws = R.write_raw_tree(root)
    f = C.FRAME
    cfg = KittiConfiguration(cropped_img_H=f["H"], cropped_img_W=f["W"], num_pt=f["num_pt"], device=DEV)
    cfg.num_node = f["num_node"]

    def samples(ds):
        out = []
        for i in range(len(ds)):
            random.seed(40 + i)
            np.random.seed(40 + i)
            torch.manual_seed(40 + i)
            out.append(ds[i])
        return out

    on_the_fly = FrameDataset(root, cfg, "val", device=DEV, from_raw=True)
    assert len(on_the_fly) == 2 and len(FrameDataset(root, cfg, "val", device=DEV)) == 0
    a = samples(on_the_fly)
    res = subprocess.run([sys.executable, "-m", "cmr_agent_amd.dataset.prepare", "--root", root, "--sequences", "9"], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    kept = [prepare.prepare_cloud(r).shape[1] for r in raws]
    assert res.stdout == "sequence 09: prepared 2 frames, %d -> %d points\n" % (sum(r.shape[1] for r in raws), sum(kept))
    out = os.path.join(os.path.dirname(vel), prepare.subdir())
    for i, r in enumerate(raws):
        assert np.array_equal(np.load(os.path.join(out, "%06d.npy" % i)), prepare.prepare_cloud(r).cpu().numpy())
    from_files = FrameDataset(root, cfg, "val", device=DEV)
    assert len(from_files) == 2 and os.path.basename(from_files.frames[0][1]) == prepare.subdir()
    b = samples(from_files)
    for sa, sb in zip(a, b):
        assert set(sa) == set(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
