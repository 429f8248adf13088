"""GPU tier of the rays cast through a voxel map (ops.voxel_map_rays / ops.voxel_map_keep, csrc/voxel_map_rays.hip, accumulate --carve;
DESIGN.md 4aj), against the restatement of voxel_map_rays_reference.py.

Every check is EXACT: crossed, hits and the four counts are integers, and the header states every fp32 operation behind a cell.  Every
case is cast twice by the product library and once more by the A/B library with the other lookup (the run of a (y, z) pair searched
alone): all three agree count by count, and the map's tensors are what they were."""
import numpy as np
import pytest
import torch

import cloud_icp_reference as R
import cloud_prepare_reference as P
import voxel_map_reference as V
import voxel_map_rays_reference as Y
from cmr_agent_amd import _lib, ops
from cmr_agent_amd.dataset import accumulate

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
F = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)      # noqa: E731
UNIT = ((0.0, 0.0, 0.0), 1.0)
ORIGIN, VOXEL = (-64.0, -64.0, -64.0), 0.5
ROWS = (1, 63, 64, 65, 255, 256, 257, 1025)                           # round the wave (64) and the workgroup (256)
VOXELS = (0, 1, 2, 255, 256, 257, 1025)


def sensor(x, y, z):
    T = np.eye(4, dtype=F32)
    T[:3, 3] = (x, y, z)
    return T


def gmap(keys, origin, voxel):
    """the map with these keys (sorted here), every other tensor of the right shape"""
    keys = torch.from_numpy(np.sort(np.asarray(keys, dtype=np.int64))).to(DEV)
    n = keys.shape[0]
    return ops.VoxelMap(keys, torch.zeros((n, 3), device=DEV), torch.zeros((n, 0), device=DEV), torch.ones((n,), dtype=torch.int32, device=DEV),
                        torch.zeros((n,), dtype=torch.int32, device=DEV), tuple(float(F32(v)) for v in origin), float(voxel))


def counts(res):
    return tuple(res[2:]) if isinstance(res, ops.MapRays) else (res["cast"], res["dropped"], res["outside"], res["long"])


def cast(keys, origin, voxel, pts, pose=None, w=None, **kw):
    """One cast on both sides, compared.  -> (the op's result, the restatement's)"""
    m = gmap(keys, origin, voxel)
    before = [t.clone() for t in m[:5]]
    got = ops.voxel_map_rays(m, F(pts), F(pose), **kw)
    again = ops.voxel_map_rays(m, F(pts), F(pose), **kw)
    with _lib.ab() as lib:                                       # the A/B library: same sources + the variant switches
        old = lib.cmr_set_voxel_map_rays_variant(1)
        try:
            other = ops.voxel_map_rays(m, F(pts), F(pose), **kw)
        finally:
            lib.cmr_set_voxel_map_rays_variant(old)
    ref = Y.cast(np.sort(np.asarray(keys, dtype=np.int64)), origin, voxel, pts, pose, w=w, **kw)
    assert got.crossed.dtype == got.hits.dtype == torch.int32 and got.crossed.shape == got.hits.shape == m.keys.shape
    assert counts(got) == counts(ref), (counts(got), counts(ref))
    for name in ("crossed", "hits"):
        have = getattr(got, name).cpu().numpy()
        assert np.array_equal(have, ref[name]), (name, np.nonzero(have != ref[name])[0][:8], have.sum(), ref[name].sum())
    for res in (again, other):
        assert torch.equal(res.crossed, got.crossed) and torch.equal(res.hits, got.hits) and counts(res) == counts(got)
    assert old == 0 and all(torch.equal(a, b) for a, b in zip(before, m[:5])), "the input map was changed"
    return got, ref


def all_cells(w):
    """the keys of every cell the walks visit, the ends' included"""
    return np.unique(np.concatenate([Y.pack(w["cell"]), Y.pack(w["end"][w["state"] == Y.CAST])]))


# ---- sizes --------------------------------------------------------------------------------------------------------------------------------
POSE = R.pose_matrix((0.02, -0.015, 0.4), (0.33, -0.27, 0.14)).astype(F32)


def size_rays():
    """1 025 rays of 2 to 12 m in all directions from a sensor off every face, the first one long enough for the default margins"""
    rng = np.random.default_rng(3)
    dirs = rng.normal(size=(1025, 3))
    pts = dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * rng.uniform(2, 12, (1025, 1))
    pts[0] = (6.0, 2.5, 1.0)
    return pts.astype(F32)


@pytest.mark.parametrize("N", ROWS)
def test_sizes(N):
    """N rays through maps of M voxels, half of them cells the walks visit and count, half strangers: found and not-found lookups in every
    case (no voxel can be found in a map of none)."""
    rng = np.random.default_rng(N)
    pts = size_rays()[:N]
    w = Y.walk(pts, POSE, ORIGIN, VOXEL)
    assert (w["state"] == Y.CAST).all()
    ray, cell = w["ray"], w["cell"]
    counted = (np.abs(cell - w["start"][ray]).max(1) > 2) & (np.abs(cell - w["end"][ray]).max(1) > 1)
    first = Y.pack(cell[counted & (ray == 0)])[:1]                # a voxel the first ray counts as crossed: the one key of M = 1
    walked = np.setdiff1d(np.unique(np.concatenate([Y.pack(cell[counted]), Y.pack(w["end"])])), first)
    strangers = np.setdiff1d(Y.pack(rng.integers(100, 156, (4000, 3))), all_cells(w))
    assert first.size == 1 and strangers.size > 1100
    for M in VOXELS:
        own = min((M + 1) // 2, 1 + walked.size)
        keys = np.concatenate([first, rng.permutation(walked)[:max(own - 1, 0)], rng.permutation(strangers)[:M - own]])[:M]
        assert keys.size == M and np.unique(keys).size == M
        got, ref = cast(keys, ORIGIN, VOXEL, pts, POSE, w=w)
        assert counts(ref) == (N, 0, 0, 0) and (M == 0 or ref["crossed"].sum() > 0) and w["ray"].size + N > ref["crossed"].sum() + ref["hits"].sum()


# ---- rays -----------------------------------------------------------------------------------------------------------------------------------
def test_rays_walked_by_hand():
    """the rays of the CPU tier, on the unit grid, the map holding every cell they visit and a stranger"""
    cases = [((0.5, 0.5, 0.5), (4, 0, 0), [[x, 0, 0] for x in range(5)]),
             ((0.5, 4.5, 0.5), (0, -3, 0), [[0, 4, 0], [0, 3, 0], [0, 2, 0], [0, 1, 0]]),
             ((3.5, 2.5, 1.5), (0, 0, 0), [[3, 2, 1]]),
             ((3.0, 0.5, 0.5), (-2, 0, 0), [[3, 0, 0], [2, 0, 0], [1, 0, 0]]),
             ((3.0, 0.5, 0.5), (2.5, 0, 0), [[3, 0, 0], [4, 0, 0], [5, 0, 0]]),
             ((3.0, 2.0, 1.0), (-1, -1, -1), [[3, 2, 1], [2, 2, 1], [2, 1, 1], [2, 1, 0]]),
             ((0.5, 0.5, 0.5), (2, 2, 0), [[0, 0, 0], [1, 0, 0], [1, 1, 0], [2, 1, 0], [2, 2, 0]]),
             ((0.5, 0.5, 0.5), (2, 2, 2), [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1], [2, 1, 1], [2, 2, 1], [2, 2, 2]]),
             ((2.5, 2.5, 0.5), (-2, -2, 0), [[2, 2, 0], [1, 2, 0], [1, 1, 0], [0, 1, 0], [0, 0, 0]]),
             ((0.5, 0.75, 0.5), (1, 1, 0), [[0, 0, 0], [0, 1, 0], [1, 1, 0]])]
    for at, point, cells in cases:
        keys = np.unique(np.concatenate([Y.pack(cells), Y.pack([[9, 9, 9]])]))
        got, ref = cast(keys, *UNIT, F32([point]), sensor(*at), start_margin=0, end_margin=0)
        want_crossed, want_hits = np.zeros(keys.size, np.int64), np.zeros(keys.size, np.int64)
        want_crossed[np.searchsorted(keys, Y.pack(cells[1:-1]))] = 1                      # neither the start's cell nor the end's
        want_hits[np.searchsorted(keys, Y.pack(cells[-1:]))] = 1
        assert got.crossed.cpu().tolist() == want_crossed.tolist() and got.hits.cpu().tolist() == want_hits.tolist() and counts(got) == (1, 0, 0, 0)
    # without a pose the sensor is the origin of the frame
    keys = Y.pack([[0, 0, 0], [1, 0, 0], [2, 0, 0]])
    got, _ = cast(keys, *UNIT, F32([[2.5, 0.5, 0.5]]), None, start_margin=0, end_margin=0)
    assert got.crossed.cpu().tolist() == [0, 1, 0] and got.hits.cpu().tolist() == [0, 0, 1]


@pytest.mark.parametrize("at", [(8.5, 8.5, 8.5), (8.0, 8.0, 8.0), (8.25, 8.0, 8.75)])
def test_octants_and_axes(at):
    """rays into all eight octants and along every axis in both directions, from inside a cell and from its faces; the map holds every
    visited cell, so with margins 0 every cell but a ray's first and last is a crossing"""
    signs = np.stack(np.meshgrid([-1, 1], [-1, 1], [-1, 1], indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([signs * [3.3, 2.2, 1.1], signs * [1.7, 4.9, 2.6], signs * [3.0, 3.0, 3.0], np.eye(3) * 5, np.eye(3) * -5,
                          np.eye(3) * 2.0, np.eye(3) * -2.0]).astype(F32)
    w = Y.walk(pts, sensor(*at), *UNIT)
    got, ref = cast(all_cells(w), *UNIT, pts, sensor(*at), w=w, start_margin=0, end_margin=0)
    steps = np.abs(w["end"] - w["start"]).sum(1)
    assert counts(got) == (pts.shape[0], 0, 0, 0) and int(got.hits.sum()) == pts.shape[0] and int(got.crossed.sum()) == np.maximum(steps - 1, 0).sum()
    assert len(set(map(tuple, np.sign(w["end"] - w["start"]).tolist()))) == 14                  # 8 octants and 6 axis directions


def test_pose_none_is_the_identity():
    pts = size_rays()[:300] + F32([40.0, 40.0, 40.0])                                     # no sensor at the origin of the frame sees this grid's middle
    w = Y.walk(pts, None, (0.0, 0.0, 0.0), VOXEL)
    m = gmap(all_cells(w)[::2], (0.0, 0.0, 0.0), VOXEL)
    a = ops.voxel_map_rays(m, F(pts), None, max_cells=65536)
    b = ops.voxel_map_rays(m, F(pts), torch.eye(4, device=DEV), max_cells=65536)
    assert torch.equal(a.crossed, b.crossed) and torch.equal(a.hits, b.hits) and counts(a) == counts(b) == (300, 0, 0, 0)
    ref = Y.cast(m.keys.cpu().numpy(), (0.0, 0.0, 0.0), VOXEL, pts, None, max_cells=65536)
    assert np.array_equal(a.crossed.cpu().numpy(), ref["crossed"]) and np.array_equal(a.hits.cpu().numpy(), ref["hits"]) and ref["crossed"].sum() > 3000


def test_the_end_of_a_ray_is_the_key_of_the_row():
    """a pose with a rotation, voxel 0.1: the map is the keys cmr_voxel_map_keys_f32 gives the rows, so every ray ends in a voxel of the
    map and hits counts the rows of every key"""
    rng = np.random.default_rng(8)
    pts = np.concatenate([rng.uniform(-6, 6, (900, 3)), np.round(rng.uniform(-6, 6, (100, 3)) * 10) / 10]).astype(F32)
    pts = np.concatenate([pts, pts[:24]])                                                   # and 24 rows twice
    pose = R.pose_matrix((0.3, -0.2, 0.5), (0.33, -0.27, 0.14)).astype(F32)
    N = pts.shape[0]
    keys = torch.empty((N,), dtype=torch.int64, device=DEV)
    moved = torch.empty((N, 3), device=DEV)
    two = torch.empty((2,), dtype=torch.int64, device=DEV)
    nb = _lib.load().cmr_voxel_map_keys_workspace_bytes(N)
    ws = torch.empty((nb,), dtype=torch.uint8, device=DEV)
    dp, dpose = F(pts), F(pose)
    _lib.call("cmr_voxel_map_keys_f32", dp.data_ptr(), 3, N, dpose.data_ptr(), ORIGIN[0], ORIGIN[1], ORIGIN[2], 0.1, keys.data_ptr(), moved.data_ptr(),
              two.data_ptr(), ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
    keys = keys.cpu().numpy()
    uniq, rows = np.unique(keys, return_counts=True)
    assert two.cpu().tolist() == [0, 0] and np.array_equal(keys, V.scan_rows(pts, pose, ORIGIN, 0.1)[1]) and 900 < uniq.size < N
    got, ref = cast(uniq, ORIGIN, 0.1, pts, pose, max_cells=65536)
    assert np.array_equal(got.hits.cpu().numpy(), rows) and counts(got) == (N, 0, 0, 0)


# ---- the edges of the grid, rows off it, rows that are no numbers ----------------------------------------------------------------------------
def test_edges_of_the_grid_outside_and_non_finite_rows():
    top, cm = 2.0 ** 21, (1 << 21) - 1
    # ends in cell 0 of each axis, from a sensor two cells in
    keys = Y.pack([[0, 2, 2], [1, 2, 2], [2, 2, 2], [2, 0, 2], [2, 1, 2], [2, 2, 0], [2, 2, 1]])
    got, _ = cast(keys, *UNIT, F32([[-2, 0, 0], [0, -2, 0], [0, 0, -2]]), sensor(2.5, 2.5, 2.5), start_margin=0, end_margin=0)
    order = np.argsort(keys)
    assert got.crossed.cpu().numpy()[np.argsort(order)].tolist() == [0, 1, 0, 0, 1, 0, 1] and got.hits.cpu().numpy()[np.argsort(order)].tolist() == [1, 0, 0, 1, 0, 1, 0]
    # ends in cell 2^21 - 1 of each axis
    for axis in range(3):
        at, point = [2.5, 2.5, 2.5], [0.0, 0.0, 0.0]
        at[axis], point[axis] = top - 2.5, 2.0
        cells = np.full((3, 3), 2, np.int64)
        cells[:, axis] = [cm - 2, cm - 1, cm]
        keys = Y.pack(cells)
        got, _ = cast(keys, *UNIT, F32([point, [0, 0, 0]]), sensor(*at), start_margin=0, end_margin=0)
        assert got.crossed.cpu().tolist() == [0, 1, 0] and got.hits.cpu().tolist() == [1, 0, 1] and counts(got) == (2, 0, 0, 0)
        assert int(keys[2]) == cm << (21 * axis) | sum(2 << (21 * a) for a in range(3) if a != axis)
    # ends off the grid, rows that are no numbers; the four counts by hand
    rows = F32([[1, 0, 0], [-3, 0, 0], [0, -2.75, 0], [0, 0, -1e30], [3e38, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3,
                [0, 0, 0], [9, 9, 9]])
    got, _ = cast(Y.pack([[3, 2, 2], [2, 2, 2]]), *UNIT, rows, sensor(2.5, 2.5, 2.5), start_margin=0, end_margin=0, max_cells=26)
    assert counts(got) == (2, 4, 4, 1) and got.hits.cpu().tolist() == [1, 1] and got.crossed.cpu().tolist() == [0, 0]
    # the sensor off the grid: every finite row is outside, whatever its end
    for at in ((-0.5, 2.5, 2.5), (2.5, top + 0.5, 2.5), (2.5, 2.5, -3e38)):
        got, _ = cast(Y.pack([[3, 2, 2], [2, 2, 2]]), *UNIT, rows, sensor(*at))
        assert counts(got) == (0, 4, 7, 0) and int(got.hits.sum()) == 0 and int(got.crossed.sum()) == 0
    # a row the pose makes non-finite: 3e38 + 3e38
    got, _ = cast(Y.pack([[3, 2, 2]]), *UNIT, F32([[3e38, 0, 0], [1, 0, 0], [-3e38, 0, 0]]), sensor(3e38, 2.5, 2.5))
    assert counts(got) == (0, 1, 2, 0)
    spin = F32([[2, 2, 2, 2.5], [0, 1, 0, 2.5], [0, 0, 1, 2.5], [0, 0, 0, 1]])            # (2 + 2) 1e38 overflows on the way
    got, _ = cast(Y.pack([[3, 2, 2]]), *UNIT, F32([[1e38, 1e38, 1e38], [0, 0, 0]]), spin)
    assert counts(got) == (1, 1, 0, 0)
    # an empty scan and an empty map
    m = gmap(Y.pack([[3, 2, 2]]), *UNIT)
    res = ops.voxel_map_rays(m, torch.zeros((0, 3), device=DEV))
    assert counts(res) == (0, 0, 0, 0) and res.crossed.tolist() == [0] and res.hits.tolist() == [0]
    res = ops.voxel_map_rays(ops.voxel_map(1.0, (0, 0, 0), 0, DEV), F(rows), F(sensor(2.5, 2.5, 2.5)), max_cells=26)
    assert counts(res) == (2, 4, 4, 1) and res.crossed.shape == res.hits.shape == (0,) and res.crossed.dtype == torch.int32


# ---- many rays, one voxel ---------------------------------------------------------------------------------------------------------------------
def test_contention():
    """4 096 rays from one sensor through one voxel three cells out: with start_margin 2 every one of them counts, with 3 none"""
    rng = np.random.default_rng(4)
    pts = np.stack([rng.uniform(6.0, 7.0, 4096), rng.uniform(-0.4, 0.4, 4096), rng.uniform(-0.4, 0.4, 4096)], 1).astype(F32)
    keys = Y.pack([[11, 8, 8]])
    got, _ = cast(keys, *UNIT, pts, sensor(8.5, 8.5, 8.5), start_margin=2, end_margin=1)
    assert got.crossed.cpu().tolist() == [4096] and got.hits.cpu().tolist() == [0] and counts(got) == (4096, 0, 0, 0)
    got, _ = cast(keys, *UNIT, pts, sensor(8.5, 8.5, 8.5), start_margin=3, end_margin=1)
    assert got.crossed.cpu().tolist() == [0] and got.hits.cpu().tolist() == [0]
    got, _ = cast(keys, *UNIT, F32([[2.5, 0, 0]] * 4096), sensor(8.5, 8.5, 8.5), start_margin=0, end_margin=0)      # and all of them ending in it
    assert got.crossed.cpu().tolist() == [0] and got.hits.cpu().tolist() == [4096]


# ---- margins and the cap ------------------------------------------------------------------------------------------------------------------------
def test_margins_and_the_cap():
    pts, at = F32([[5.3, 3.1, -2.2], [-4.0, 0, 0]]), sensor(8.5, 8.5, 8.5)
    w = Y.walk(pts, at, *UNIT)
    keys = all_cells(w)
    steps = np.abs(w["end"] - w["start"]).sum(1)
    assert steps.tolist() == [10, 4]
    for sm in (0, 1, 99):
        for em in (0, 1, 99):
            got, ref = cast(keys, *UNIT, pts, at, w=w, start_margin=sm, end_margin=em)
            d0, d1 = np.abs(w["cell"] - w["start"][w["ray"]]).max(1), np.abs(w["cell"] - w["end"][w["ray"]]).max(1)
            assert int(got.crossed.sum()) == ((d0 > sm) & (d1 > em)).sum() and int(got.hits.sum()) == 2 and counts(got) == (2, 0, 0, 0)
            assert (sm < 99 and em < 99) == (int(got.crossed.sum()) > 0)
    got, _ = cast(keys, *UNIT, pts, at, start_margin=0, end_margin=0, max_cells=10)
    assert counts(got) == (2, 0, 0, 0) and int(got.crossed.sum()) == 9 + 3 and int(got.hits.sum()) == 2
    got, _ = cast(keys, *UNIT, pts, at, start_margin=0, end_margin=0, max_cells=9)            # one below the first ray's steps: long, nothing else moves
    assert counts(got) == (1, 0, 0, 1) and int(got.crossed.sum()) == 3 and int(got.hits.sum()) == 1
    got, _ = cast(keys, *UNIT, pts, at, start_margin=0, end_margin=0, max_cells=3)
    assert counts(got) == (0, 0, 0, 2) and int(got.crossed.sum()) == 0 and int(got.hits.sum()) == 0


# ---- one scene ----------------------------------------------------------------------------------------------------------------------------------
def test_accumulate_carve_drops_a_block_only_one_scan_saw(tmp_path, capsys):
    """Two of the synthetic scans of the voxel map's tier at voxel 0.5, the first with a block of rows that the second one's rays pass through:
    accumulate --carve drops exactly the voxels the restatement drops, the block among them and none of the ground."""
    raws = [P.scene(30 + j, n=1600, clump=200, far=10, scale=0.5) for j in range(2)]
    poses = np.stack([np.eye(4), R.pose_matrix(*R.TRUE_POSES[1])])
    frames, nblock = Y.with_block(tuple(np.concatenate([r.T, np.zeros((3, r.shape[0]), F32)]).astype(F32) for r in raws), poses,
                                  centre=(2.8, 0.6, -0.6), half=0.25)
    R.write_frames(str(tmp_path), frames)
    pfile, out = str(tmp_path / "poses.txt"), str(tmp_path / "map.npy")
    accumulate.align.write_poses(pfile, poses)
    poses = accumulate.read_poses(pfile)
    rule = dict(frames=1, ratio=1.0, start=1.0, end=2, max_range=60.0)
    accumulate.main(["--root", str(tmp_path), "--data-velodyne", "vel", "--sequence", "9", "--poses", pfile, "--voxel", "0.5", "--extent", "128",
                     "--out", out, "--carve", "--carve-frames", "1", "--carve-start", "1.0", "--carve-end", "2", "--carve-max-range", "60"])
    lines = capsys.readouterr().out.splitlines()
    ref = V.accumulate(frames, poses, V.CHAIN_FIRST, voxel=0.5, extent=128.0)
    clouds, poses32 = [f[:3].T for f in frames], [T.astype(F32) for T in poses]
    drop, infos = Y.carve_frames(ref["keys"], ref["origin"], 0.5, clouds, poses32, **rule)
    n = ref["keys"].size
    for j, info in enumerate(infos):
        assert lines[2 + j] == "carve %d: cast %d long %d outside %d through %d" % (3 + j, info["cast"], info["long"], info["outside"], info["through"])
        assert info["cast"] == frames[j].shape[1] - info["long"] and info["long"] <= 10 and info["through"] > 0
    assert lines[4] == "carved: %d of %d voxels" % (drop.sum(), n) and lines[5].startswith("map: %d voxels from " % (n - drop.sum())) and len(lines) == 6
    # which voxels: the mask itself, on the map of the same files; the file's rows are the kept voxels' means, within the map's bound
    files = accumulate.align.sequence_files(*accumulate.parse_args(["--root", str(tmp_path), "--data-velodyne", "vel", "--sequence", "9", "--poses", pfile]))
    quiet = lambda ln: None                                                                          # noqa: E731
    vmap, _ = accumulate.accumulate_sequence(files, poses, 0.5, 128.0, report=quiet)
    mask = accumulate.carve_sequence(vmap, files, poses, report=quiet, **rule)
    assert np.array_equal(vmap.keys.cpu().numpy(), ref["keys"]) and mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), drop)
    kept = ops.voxel_map_keep(vmap, ~mask)
    assert np.array_equal(kept.keys.cpu().numpy(), ref["keys"][~drop]) and kept.origin == vmap.origin and kept.voxel == vmap.voxel
    cloud = np.load(out)
    assert cloud.shape == (7, n - drop.sum()) and np.array_equal(cloud[:3].T, kept.points.cpu().numpy()) and np.array_equal(cloud[3:4].T, kept.attr.cpu().numpy())
    assert (np.abs(cloud[:4].T.astype(np.float64) - V.mean64(ref)[~drop]) <= V.bound(ref)[~drop]).all()
    # the block is among the dropped voxels, the ground is not
    scan_keys = lambda rows, j: V.scan_rows(rows, poses32[j], ref["origin"], 0.5)[1]                 # noqa: E731
    rest = np.concatenate([scan_keys(clouds[0][:-nblock], 0), scan_keys(clouds[1], 1)])
    own = np.setdiff1d(scan_keys(clouds[0][-nblock:], 0), rest)
    ground = np.unique(np.concatenate([scan_keys(clouds[j][:400], j) for j in range(2)]))
    assert own.size >= 4 and drop[np.searchsorted(ref["keys"], own)].all() and ground.size > 100 and not drop[np.searchsorted(ref["keys"], ground)].any()
    assert own.size <= drop.sum() < n // 4
