"""CPU tier of the rays cast through a voxel map (ops.voxel_map_rays / ops.voxel_map_keep, accumulate --carve): the
restatement on rays walked by hand, the float64 check that its walks are rays, every argument check ahead of the library, the carve rule on
hand-written counts, and the command with the restatements in the ops' places."""
import os

import numpy as np
import pytest
import torch

import cloud_icp_reference as R
import cloud_prepare_reference as P
import voxel_map_reference as V
import voxel_map_rays_reference as Y
from cmr_agent_amd import _lib, ops
from cmr_agent_amd.dataset import accumulate, align

F32 = np.float32
UNIT = ((0.0, 0.0, 0.0), 1.0)                                             # the grid of the rays walked by hand: origin, voxel


def sensor(x, y, z):
    T = np.eye(4, dtype=F32)
    T[:3, 3] = (x, y, z)
    return T


def cells_of(sensor_at, point, **kw):
    w = Y.walk(F32([point]), sensor(*sensor_at), *UNIT, **kw)
    return Y.visited(w, 0).tolist() if w["state"][0] == Y.CAST else int(w["state"][0])


# ---- the restatement on rays walked by hand -----------------------------------------------------------------------------------------------
def test_axis_rays_by_hand():
    # along +x through five cells; the map holds all five and a stranger: the start's cell is no crossing (distance 0), the end's a hit
    assert cells_of((0.5, 0.5, 0.5), (4, 0, 0)) == [[x, 0, 0] for x in range(5)]
    keys = np.sort(Y.pack([[x, 0, 0] for x in range(5)] + [[2, 1, 0]]))
    res = Y.cast(keys, *UNIT, F32([[4, 0, 0]]), sensor(0.5, 0.5, 0.5), start_margin=0, end_margin=0)
    assert res["crossed"].tolist() == [0, 1, 1, 1, 0, 0] and res["hits"].tolist() == [0, 0, 0, 0, 1, 0]
    assert (res["cast"], res["dropped"], res["outside"], res["long"]) == (1, 0, 0, 0)
    res = Y.cast(keys, *UNIT, F32([[4, 0, 0]]), sensor(0.5, 0.5, 0.5), start_margin=1, end_margin=1)
    assert res["crossed"].tolist() == [0, 0, 1, 0, 0, 0] and res["hits"].tolist() == [0, 0, 0, 0, 1, 0]
    # along -y
    assert cells_of((0.5, 4.5, 0.5), (0, -3, 0)) == [[0, 4, 0], [0, 3, 0], [0, 2, 0], [0, 1, 0]]
    assert cells_of((0.5, 0.5, 2.25), (0, 0, -2)) == [[0, 0, 2], [0, 0, 1], [0, 0, 0]]
    # without a pose the sensor is the origin of the frame
    assert Y.visited(Y.walk(F32([[2.5, 0.5, 0.5]]), None, *UNIT), 0).tolist() == [[0, 0, 0], [1, 0, 0], [2, 0, 0]]


def test_a_ray_of_length_zero_crosses_nothing_and_hits_once():
    assert cells_of((3.5, 2.5, 1.5), (0, 0, 0)) == [[3, 2, 1]]
    keys = Y.pack([[3, 2, 1]])
    res = Y.cast(keys, *UNIT, F32([[0, 0, 0]]), sensor(3.5, 2.5, 1.5), start_margin=0, end_margin=0)
    assert res["crossed"].tolist() == [0] and res["hits"].tolist() == [1] and res["cast"] == 1
    # an axis without a step is never divided on: d = 0 on all three here, and on two of three for an axis ray
    w = Y.walk(F32([[0, 0, 0], [2, 0, 0]]), sensor(3.5, 2.5, 1.5), *UNIT)
    assert (w["b"][0] - w["a"][0] == 0).all() and w["ray"].tolist() == [1, 1]


def test_a_start_on_a_cell_face():
    # the face x = 3 belongs to cell 3; towards -x the ray leaves that cell at t = 0, towards +x after a whole cell
    assert cells_of((3.0, 0.5, 0.5), (-2, 0, 0)) == [[3, 0, 0], [2, 0, 0], [1, 0, 0]]
    assert cells_of((3.0, 0.5, 0.5), (2.5, 0, 0)) == [[3, 0, 0], [4, 0, 0], [5, 0, 0]]
    assert cells_of((3.0, 2.0, 1.0), (-1, -1, -1)) == [[3, 2, 1], [2, 2, 1], [2, 1, 1], [2, 1, 0]]      # all three at t = 0: x, y, z
    # an end on a face lies in the cell above it
    assert cells_of((0.5, 0.5, 0.5), (1.5, 0, 0)) == [[0, 0, 0], [1, 0, 0], [2, 0, 0]]


def test_ties_go_to_x_before_y_before_z():
    assert cells_of((0.5, 0.5, 0.5), (2, 2, 0)) == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [2, 1, 0], [2, 2, 0]]
    assert cells_of((0.5, 0.5, 0.5), (2, 2, 2)) == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1], [2, 1, 1], [2, 2, 1], [2, 2, 2]]
    assert cells_of((0.5, 0.5, 0.5), (0, 1, 1)) == [[0, 0, 0], [0, 1, 0], [0, 1, 1]]
    assert cells_of((2.5, 2.5, 0.5), (-2, -2, 0)) == [[2, 2, 0], [1, 2, 0], [1, 1, 0], [0, 1, 0], [0, 0, 0]]
    # no tie: the nearer face first
    assert cells_of((0.5, 0.75, 0.5), (1, 1, 0)) == [[0, 0, 0], [0, 1, 0], [1, 1, 0]]


def test_margins_that_swallow_the_ray_and_the_cap():
    keys = np.sort(Y.pack([[x, 0, 0] for x in range(5)]))
    at, row = sensor(0.5, 0.5, 0.5), F32([[4, 0, 0]])
    for kw in (dict(start_margin=4, end_margin=0), dict(start_margin=0, end_margin=4), dict(start_margin=3, end_margin=3), dict(start_margin=99, end_margin=99)):
        res = Y.cast(keys, *UNIT, row, at, **kw)
        assert res["crossed"].tolist() == [0] * 5 and res["hits"].tolist() == [0, 0, 0, 0, 1] and res["cast"] == 1
    assert Y.cast(keys, *UNIT, row, at, start_margin=2, end_margin=0)["crossed"].tolist() == [0, 0, 0, 1, 0]
    assert Y.cast(keys, *UNIT, row, at, start_margin=0, end_margin=2)["crossed"].tolist() == [0, 1, 0, 0, 0]
    # four steps: max_cells 4 casts the ray, 3 counts it long and nothing else moves
    res = Y.cast(keys, *UNIT, row, at, start_margin=0, end_margin=0, max_cells=4)
    assert (res["cast"], res["long"]) == (1, 0) and res["crossed"].sum() == 3 and res["hits"].sum() == 1
    res = Y.cast(keys, *UNIT, row, at, start_margin=0, end_margin=0, max_cells=3)
    assert (res["cast"], res["long"], res["dropped"], res["outside"]) == (0, 1, 0, 0) and res["crossed"].sum() == 0 and res["hits"].sum() == 0
    assert cells_of((0.5, 0.5, 0.5), (1, 2, 1), max_cells=4) != Y.LONG and cells_of((0.5, 0.5, 0.5), (1, 2, 1), max_cells=3) == Y.LONG


def test_flags_by_hand():
    top = 2.0 ** 21
    rows = F32([[1, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [-1, 0, 0], [top, 0, 0], [3e38, 0, 0], [0, 0, 0]])
    w = Y.walk(rows, sensor(0.5, 0.5, 0.5), *UNIT)
    assert w["state"].tolist() == [Y.CAST, Y.DROPPED, Y.DROPPED, Y.OUTSIDE, Y.OUTSIDE, Y.OUTSIDE, Y.CAST]
    # the sensor off the grid: every finite row is outside, whatever its end
    assert Y.walk(rows, sensor(-0.5, 0.5, 0.5), *UNIT)["state"].tolist() == [Y.OUTSIDE, Y.DROPPED, Y.DROPPED] + [Y.OUTSIDE] * 4
    # a pose that makes a row non-finite
    assert Y.walk(F32([[3e38, 0, 0], [1, 0, 0]]), sensor(3e38, 0.5, 0.5), *UNIT)["state"].tolist() == [Y.DROPPED, Y.OUTSIDE]
    # the end's key is the key the map gives the row
    pose = R.pose_matrix((0.3, -0.2, 0.5), (7.0, 9.0, 4.0)).astype(F32)
    pts = np.random.default_rng(0).uniform(-3, 3, (50, 3)).astype(F32)
    w = Y.walk(pts, pose, (-1.0, -2.0, -3.0), 0.25)
    assert (w["state"] == Y.CAST).all() and np.array_equal(Y.pack(w["end"]), V.scan_rows(pts, pose, (-1.0, -2.0, -3.0), 0.25)[1])


# ---- the restatement against float64 ------------------------------------------------------------------------------------------------------
def slab_rays(rng):
    """300 rays of 1 to 20 m in all directions, and axis-aligned, diagonal and zero-length ones"""
    dirs = rng.normal(size=(300, 3))
    rays = dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * rng.uniform(1, 20, (300, 1))
    special = [[7, 0, 0], [-7, 0, 0], [0, 5.5, 0], [0, -5.5, 0], [0, 0, 3.25], [0, 0, -3.25], [4, 4, 0], [-4, 4, 4], [3, -3, 3], [-2, -2, -2], [0, 0, 0]]
    return np.concatenate([rays, special]).astype(F32)


@pytest.mark.parametrize("voxel", [0.5, 0.1])
def test_the_walk_is_a_ray_in_float64(voxel):
    """Every cell whose box, shrunk by 10^-3 cells, the float64 segment meets is walked; no walked cell's box, grown by as much, is missed
    by it; what lies in between is at most 1 % of the decided crossings (measured: DESIGN.md 4aj)."""
    origin = (-64.0, -64.0, -64.0)
    pts = slab_rays(np.random.default_rng(11))
    pose = R.pose_matrix((0.02, -0.015, 0.4), (0.33, -0.27, 0.14)).astype(F32)         # a sensor on no face of either grid
    w = Y.walk(pts, pose, origin, voxel, max_cells=65536)
    assert (w["state"] == Y.CAST).all()
    got = Y.slab64(pts, pose, origin, voxel, w)
    share = got["undecided"] / got["decided"]
    print("voxel %.1f: %d decided crossings, %d missed, %d extra, %d undecided (%.2f %%)" % (
        voxel, got["decided"], got["missed"], got["extra"], got["undecided"], 100 * share))
    assert got["decided"] > 5000 and got["missed"] == 0 and got["extra"] == 0 and share <= 0.01


# ---- argument checks: every one raises before the library is reached ----------------------------------------------------------------------
def _touched(*a, **k):
    raise AssertionError("the library was reached")


def _map(n=4, channels=1, device="cpu", **over):
    parts = dict(keys=torch.arange(n, dtype=torch.int64, device=device), points=torch.zeros((n, 3), device=device),
                 attr=torch.zeros((n, channels), device=device), count=torch.ones((n,), dtype=torch.int32, device=device),
                 stamp=torch.zeros((n,), dtype=torch.int32, device=device), origin=(0.0, 0.0, 0.0), voxel=0.5)
    parts.update(over)
    return ops.VoxelMap(**parts)


def test_argument_checks(monkeypatch):
    monkeypatch.setattr(_lib, "load", _touched)
    monkeypatch.setattr(_lib, "call", _touched)
    rays, p = ops.voxel_map_rays, torch.zeros((8, 3))
    for bad in (None, (p, p), p, tuple(_map())):
        with pytest.raises(ValueError, match="voxel_map_rays: map must be a VoxelMap"):
            rays(bad, p)
    for over in (dict(keys=torch.zeros((4,), dtype=torch.int32)), dict(points=torch.zeros((4, 4))), dict(count=torch.ones((3,), dtype=torch.int32)),
                 dict(voxel=0.0), dict(origin=(0.1, 0.0, 0.0)), dict(points=torch.zeros((4, 3), device="meta"))):
        with pytest.raises(ValueError, match="malformed VoxelMap"):
            rays(_map(**over), p)
    for name, lo, hi in (("start_margin", 0, 2 ** 21 - 1), ("end_margin", 0, 2 ** 21 - 1), ("max_cells", 1, 65536)):
        for bad in (lo - 1, hi + 1, 1.5, True, None, "3", float("nan")):
            with pytest.raises(ValueError, match="voxel_map_rays: %s must be an integer in \\[%d, %d\\]" % (name, lo, hi)):
                rays(_map(), p, **{name: bad})
    for bad in (torch.eye(3), torch.eye(4, dtype=torch.float64), np.eye(4, dtype=np.float32), torch.zeros((1, 4, 4))):
        with pytest.raises(ValueError, match="voxel_map_rays: pose must be a float32 \\[4, 4\\]"):
            rays(_map(), p, pose=bad)
    for bad in (torch.zeros((8, 2)), torch.zeros((8,)), torch.zeros((2, 8, 3)), torch.zeros((8, 3), dtype=torch.float64), np.zeros((8, 3), np.float32), None):
        with pytest.raises(ValueError, match="points must be a float32"):
            rays(_map(), bad)
    with pytest.raises(ValueError, match="device tensor"):
        rays(_map(), p)
    # behind the check of the points' device, which no tensor of this tier passes
    monkeypatch.setattr(ops, "_cloud_points", lambda points, name="points": points)
    with pytest.raises(ValueError, match="voxel_map_rays: points must be on the map's device"):
        rays(_map(device="meta"), p)
    with pytest.raises(ValueError, match="voxel_map_rays: the map must hold device tensors"):
        rays(_map(), p)
    with pytest.raises(ValueError, match="voxel_map_rays: the map must hold device tensors"):
        rays(_map(n=0), p)


def test_voxel_map_keep():
    m = _map(n=5, channels=2, points=torch.arange(15, dtype=torch.float32).reshape(5, 3), origin=(-4096.0, 0.0, 0.5), voxel=0.25)
    mask = torch.tensor([True, False, True, True, False])
    out = ops.voxel_map_keep(m, mask)
    assert isinstance(out, ops.VoxelMap) and out.origin == m.origin and out.voxel == m.voxel
    assert out.keys.tolist() == [0, 2, 3] and out.points.tolist() == [[0, 1, 2], [6, 7, 8], [9, 10, 11]] and out.attr.shape == (3, 2)
    assert out.count.dtype == out.stamp.dtype == torch.int32 and out.count.shape == out.stamp.shape == (3,) and m.keys.shape == (5,)
    assert ops.voxel_map_keep(m, torch.zeros(5, dtype=torch.bool)).keys.shape == (0,)
    assert ops.voxel_map_keep(_map(n=0), torch.zeros(0, dtype=torch.bool)).points.shape == (0, 3)
    for bad in (mask[:4], mask[None], mask.to(torch.uint8), mask.numpy(), None, mask.to("meta")):
        with pytest.raises(ValueError, match="voxel_map_keep: mask must be a bool \\[5\\] tensor on the map's device"):
            ops.voxel_map_keep(m, bad)
    with pytest.raises(ValueError, match="voxel_map_keep: map must be a VoxelMap"):
        ops.voxel_map_keep(tuple(m), mask)


def test_header_and_work_model_know_the_entry_point():
    from cmr_agent_amd.utils import workmodel
    protos = _lib.parse_header()
    name = "cmr_voxel_map_rays_f32"
    assert name in protos and name in workmodel.WORK
    assert protos[name][2] == ["keys", "M", "ox", "oy", "oz", "voxel", "points", "ld", "N", "pose", "start_margin", "end_margin", "max_cells",
                               "crossed", "hits", "counts", "workspace", "workspace_bytes", "stream"]
    assert workmodel.WORK[name](dict(N=1000, M=100)) == (0, 12000 + 1600)
    lib = _lib.load()
    assert lib.cmr_voxel_map_rays_workspace_bytes(0) == 0 and lib.cmr_voxel_map_rays_workspace_bytes(2 ** 31) == 0
    assert lib.cmr_voxel_map_rays_workspace_bytes(256) == 4 and lib.cmr_voxel_map_rays_workspace_bytes(257) == 8
    assert "cmr_set_voxel_map_rays_variant" in _lib.parse_header(_lib.AB_HEADER_PATH) and not hasattr(lib, "cmr_set_voxel_map_rays_variant")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "cmr_agent_amd", "csrc", "voxel_map_rays.hip")).read()
    assert '#include "cmr_cloud_grid.h"' in src and "key_bound(" in src and "max_cells" in src


# ---- the carve rule on counts written by hand -----------------------------------------------------------------------------------------------
def test_the_carve_rule():
    through, seen = np.int64([0, 1, 2, 2, 2, 3, 5, 2]), np.int64([0, 0, 0, 2, 3, 3, 9, 1])
    want = [False, False, True, True, False, True, False, True]                 # two frames at least, and as many as saw it
    assert accumulate.carve_rule(through, seen).tolist() == want == Y.carve(through, seen).tolist()
    assert accumulate.carve_rule(torch.from_numpy(through), torch.from_numpy(seen)).tolist() == want
    assert accumulate.carve_rule(through, seen, frames=1, ratio=0.0).tolist() == [False] + [True] * 7
    assert accumulate.carve_rule(through, seen, frames=3, ratio=0.5).tolist() == [False] * 5 + [True, True, False]
    assert accumulate.carve_rule(through, seen, frames=1, ratio=2.0).tolist() == [False, True, True, False, False, False, False, True]
    for kw in (dict(frames=1, ratio=0.0), dict(frames=3, ratio=0.5), dict(frames=1, ratio=2.0)):
        assert accumulate.carve_rule(through, seen, **kw).tolist() == Y.carve(through, seen, **kw).tolist()
    assert accumulate.carve_margins(0.1) == (20, 3600) and accumulate.carve_margins(0.5, 2.0, 120.0) == (4, 720)
    assert accumulate.carve_margins(0.3, 1.0, 10.0) == (4, 100) and accumulate.carve_margins(0.001, 0.0, 120.0) == (0, 65536)


# ---- the command, with the restatements in the ops' places ----------------------------------------------------------------------------------
@pytest.fixture
def stand_ins(monkeypatch):
    """-> the arguments of every ops.voxel_map_rays call"""
    calls = []

    def rays(map, points, pose=None, **kw):
        calls.append(dict(kw, rows=points.shape[0], voxels=map.keys.shape[0]))
        return Y.ops_voxel_map_rays(map, points, pose, **kw)

    monkeypatch.setattr(ops, "point_normals", P.ops_point_normals)
    monkeypatch.setattr(ops, "voxel_map_insert", V.ops_voxel_map_insert)
    monkeypatch.setattr(ops, "voxel_map_rays", rays)
    return calls


def test_accumulate_carve(tmp_path, stand_ins, capsys):
    truth = V.chain_truth()
    frames, nblock = Y.with_block(tuple(np.ascontiguousarray(f[:, ::3]) for f in V.chain_frames()), truth)
    R.write_frames(str(tmp_path), frames)
    pfile, plain, carved = str(tmp_path / "poses.txt"), str(tmp_path / "plain.npy"), str(tmp_path / "carved.npy")
    align.write_poses(pfile, truth)
    poses = accumulate.read_poses(pfile)
    base = ["--root", str(tmp_path), "--data-velodyne", "vel", "--sequence", "9", "--poses", pfile, "--voxel", "0.4"]
    # without --carve: the lines and the file as before, and no ray is cast
    accumulate.main(base + ["--out", plain], device="cpu")
    lines = capsys.readouterr().out.splitlines()
    ref = V.accumulate(frames, poses, V.CHAIN_FIRST, voxel=0.4)
    n, rows = ref["keys"].size, sum(f.shape[1] for f in frames)
    assert not stand_ins and [ln.split(":")[0] for ln in lines] == ["frame 3", "frame 4", "frame 5", "frame 6", "map"]
    assert lines[4] == "map: %d voxels from %d rows of 4 frames" % (n, rows)
    cloud = np.load(plain)
    assert np.array_equal(cloud[:3].T, ref["points"]) and np.array_equal(cloud[4:7].T, P.point_normals(ref["points"], 0.6)["normals"].astype(F32))
    # with it
    flags = ["--carve", "--carve-start", "1.0", "--carve-max-range", "30"]
    accumulate.main(base + flags + ["--out", carved], device="cpu")
    out = capsys.readouterr().out.splitlines()
    drop, infos = Y.carve_frames(ref["keys"], ref["origin"], 0.4, [f[:3].T for f in frames], [T.astype(F32) for T in poses], start=1.0, max_range=30.0)
    assert out[:4] == lines[:4] and len(out) == 10
    for j, info in enumerate(infos):
        assert out[4 + j] == "carve %d: cast %d long %d outside %d through %d" % (3 + j, info["cast"], info["long"], info["outside"], info["through"])
        assert info["cast"] + info["long"] == frames[j].shape[1] and info["through"] > 0
    assert out[8] == "carved: %d of %d voxels" % (drop.sum(), n) and out[9] == "map: %d voxels from %d rows of 4 frames" % (n - drop.sum(), rows)
    assert [c["rows"] for c in stand_ins] == [f.shape[1] for f in frames] and all(c["voxels"] == n for c in stand_ins)
    assert all((c["start_margin"], c["end_margin"], c["max_cells"]) == (3, 1, 225) for c in stand_ins)
    cloud = np.load(carved)
    assert np.array_equal(cloud[:3].T, ref["points"][~drop]) and np.array_equal(cloud[3:4].T, ref["attr"][~drop])
    assert np.array_equal(cloud[4:7].T, P.point_normals(ref["points"][~drop], 0.6)["normals"].astype(F32))
    # the block is gone: every voxel that only its rows fill
    _, block_keys = V.scan_rows(frames[0][:3, -nblock:].T, poses[0].astype(F32), ref["origin"], 0.4)
    rest = np.concatenate([V.scan_rows(f[:3, :(-nblock if j == 0 else None)].T, T.astype(F32), ref["origin"], 0.4)[1] for j, (f, T) in enumerate(zip(frames, poses))])
    own = np.setdiff1d(block_keys, rest)
    assert own.size >= 4 and drop[np.searchsorted(ref["keys"], own)].all() and 0 < drop.sum() < n // 4
    # --min-count comes after the carve; the rule's flags reach it
    accumulate.main(base + flags + ["--min-count", "2", "--carve-frames", "3", "--carve-ratio", "0.5", "--carve-rays", "2", "--carve-end", "0"], device="cpu")
    out = capsys.readouterr().out.splitlines()
    drop3, _ = Y.carve_frames(ref["keys"], ref["origin"], 0.4, [f[:3].T for f in frames], [T.astype(F32) for T in poses], rays=2, frames=3, ratio=0.5,
                              start=1.0, end=0, max_range=30.0)
    assert out[8] == "carved: %d of %d voxels" % (drop3.sum(), n) and out[9].startswith("map: %d voxels " % (~drop3 & (ref["count"] >= 2)).sum())
    assert all(c["end_margin"] == 0 for c in stand_ins[8:])


def test_carve_flag_rules(capsys):
    base = ["--root", "d", "--sequence", "3", "--poses", "p"]
    _, args = accumulate.parse_args(base)
    assert (args.carve, args.carve_rays, args.carve_frames, args.carve_ratio, args.carve_start, args.carve_end, args.carve_max_range) == (
        False, 1, 2, 1.0, 2.0, 1, 120.0)
    assert accumulate.parse_args(base + ["--carve"])[1].carve is True
    for extra in (["--carve-rays", "0"], ["--carve-frames", "0"], ["--carve-frames", "1.5"], ["--carve-ratio", "-1"], ["--carve-ratio", "nan"],
                  ["--carve-start", "-0.1"], ["--carve-start", "inf"], ["--carve-start", "1e9"], ["--carve-end", "-1"], ["--carve-end", str(2 ** 21)],
                  ["--carve-max-range", "0"], ["--carve-max-range", "inf"]):
        with pytest.raises(SystemExit):
            accumulate.parse_args(base + extra)
    assert "--carve-max-range must be finite and > 0" in capsys.readouterr().err
    assert "not tuned on real data" in " ".join(accumulate.parse_args(base)[0].format_help().split())
