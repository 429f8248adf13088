"""What the cloud wrappers of ops.py launch, recorded (tests/golden/cloud_launches.json): for every case of one table, the entry points that
reached `_lib.call` in order, every argument of each that is no pointer, whether each pointer is null, and how often the call read the device
back through `Tensor.cpu` / `Tensor.item`.  The wrappers hold no arithmetic of their own, so two versions of them that launch the same
entry points with the same sizes and scalars on the same inputs compute the same; `python tests/test_cloud_launches_gpu.py --record` on
the MI355X writes the file from the ops module it imports, and was run against the wrappers as they stood before their prologues were stated
once.  The clouds are seeded and no larger than the host code's branches need: 0, 1, 17 and 257 rows, one with a NaN row,
one of NaN rows only."""
import ctypes
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from cmr_agent_amd import _lib, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cloud_launches.json")
ROWS = (0, 1, 17, 257)
NAN = float("nan")


# ---- the seeded inputs -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _host_cloud(n, seed=0):
    return np.random.default_rng(1000 * seed + n).uniform(0.0, 4.0, (n, 3)).astype(np.float32)


def cloud(n, seed=0, nan=()):
    """n rows in [0, 4)^3; the rows `nan` (or all of them: nan=True) without a finite coordinate"""
    c = _host_cloud(n, seed).copy()
    if nan is True:
        c[:] = NAN
    else:
        for r in nan:
            c[r, r % 3] = NAN
    return torch.from_numpy(c).cuda()


def attr(n, c=2):
    return torch.from_numpy(np.random.default_rng(7 + n).uniform(0.0, 1.0, (n, c)).astype(np.float32)).cuda()


def pose(shift=0.05):
    c, s = np.cos(0.02), np.sin(0.02)
    return torch.tensor([[c, -s, 0, shift], [s, c, 0, -shift], [0, 0, 1, shift / 2], [0, 0, 0, 1]], dtype=torch.float32).cuda()


def moved(points, T):
    return (points @ T[:3, :3].T + T[:3, 3]).contiguous()


def normals(points):
    return ops.point_normals(points, radius=1.0).normals


def descriptors(n, seed=0):
    return torch.from_numpy(np.random.default_rng(50 + seed).uniform(0.0, 1.0, (n, 33)).astype(np.float32)).cuda()


def corr(n):
    return torch.stack([torch.arange(n, dtype=torch.int32), torch.arange(n, dtype=torch.int32)], 1).cuda()


def filled(n=257, channels=1, origin=(-8.0, -8.0, -8.0)):
    """a map that holds cloud(n) under stamp 1"""
    m = ops.voxel_map(0.5, origin, channels)
    return ops.voxel_map_insert(m, cloud(n), attr(n, channels) if channels else None, stamp=1).map


# ---- the table: name -> the call, its inputs built ahead of the recording by `given` --------------------------------------------------------
CASES = {}


def case(name, given, call):
    assert name not in CASES, name
    CASES[name] = (given, call)


for n in ROWS:
    case("voxel_downsample:%d rows" % n, lambda n=n: cloud(n), lambda p: ops.voxel_downsample(p, voxel=0.5))
    case("point_normals:%d rows" % n, lambda n=n: cloud(n), lambda p: ops.point_normals(p, radius=1.0))
    case("cloud_index:%d rows" % n, lambda n=n: cloud(n), lambda p: ops.cloud_index(p, 1.0))
    case("point_fpfh:%d rows" % n, lambda n=n: (cloud(n), normals(cloud(n))), lambda a: ops.point_fpfh(a[0], a[1], 1.0))
case("voxel_downsample:attr and inverse", lambda: (cloud(257), attr(257)), lambda a: ops.voxel_downsample(a[0], a[1], voxel=0.5, want_inverse=True))
case("voxel_downsample:attr without channels", lambda: (cloud(17), attr(17, 0)), lambda a: ops.voxel_downsample(a[0], a[1], voxel=0.5))
case("voxel_downsample:origin", lambda: cloud(257), lambda p: ops.voxel_downsample(p, voxel=0.5, origin=(-1.0, -1.0, -1.0)))
case("voxel_downsample:a NaN row", lambda: (cloud(17, nan=(5,)), attr(17)), lambda a: ops.voxel_downsample(a[0], a[1], voxel=0.5, want_inverse=True))
case("voxel_downsample:NaN rows only", lambda: cloud(17, nan=True), lambda p: ops.voxel_downsample(p, voxel=0.5, want_inverse=True))
case("point_normals:eigenvalues", lambda: cloud(257), lambda p: ops.point_normals(p, radius=1.0, viewpoint=(1, 2, 3), min_neighbors=5, want_eigenvalues=True))
case("point_normals:a NaN row", lambda: cloud(17, nan=(5,)), lambda p: ops.point_normals(p, radius=1.0))
case("point_normals:NaN rows only", lambda: cloud(17, nan=True), lambda p: ops.point_normals(p, radius=1.0))
case("cloud_index:a NaN row", lambda: cloud(17, nan=(5,)), lambda p: ops.cloud_index(p, 1.0))
case("cloud_index:NaN rows only", lambda: cloud(17, nan=True), lambda p: ops.cloud_index(p, 1.0))

case("cloud_nearest:plain", lambda: (ops.cloud_index(cloud(257), 1.0), cloud(17)), lambda a: ops.cloud_nearest(*a))
case("cloud_nearest:max_dist and pose", lambda: (ops.cloud_index(cloud(257), 1.0), cloud(17), 0.5, pose()), lambda a: ops.cloud_nearest(*a))
case("cloud_nearest:no query", lambda: (ops.cloud_index(cloud(257), 1.0), cloud(0)), lambda a: ops.cloud_nearest(*a))
case("cloud_nearest:an empty index", lambda: (ops.cloud_index(cloud(17, nan=True), 1.0), cloud(17)), lambda a: ops.cloud_nearest(*a))


def _pair(n=257, nan=()):
    t = cloud(n, nan=nan)
    return moved(cloud(n), pose()), t, normals(t)


case("icp_point_to_plane:plain", _pair, lambda a: ops.icp_point_to_plane(*a, iters=3))
case("icp_point_to_plane:index, pose and system", lambda: _pair() + (ops.cloud_index(cloud(257), 2.0),),
     lambda a: ops.icp_point_to_plane(a[0], None, a[2], pose=pose(0.01), max_dist=1.5, huber=0.1, iters=2, index=a[3], want_system=True))
case("icp_point_to_plane:target and index", lambda: _pair(17) + (ops.cloud_index(cloud(17), 1.0),),
     lambda a: ops.icp_point_to_plane(a[0], a[1], a[2], iters=2, index=a[3]))
case("icp_point_to_plane:no source row", lambda: (cloud(0),) + _pair(17)[1:], lambda a: ops.icp_point_to_plane(*a, iters=2, want_system=True))
case("icp_point_to_plane:no target row", lambda: (cloud(17), cloud(0), cloud(0)), lambda a: ops.icp_point_to_plane(*a, iters=2))
case("icp_point_to_plane:a target of NaN rows", lambda: (cloud(17), cloud(17, nan=True), cloud(17, 1)), lambda a: ops.icp_point_to_plane(*a, iters=2))

case("point_fpfh:index and spfh", lambda: (cloud(257), normals(cloud(257)), 1.0, ops.cloud_index(cloud(257), 1.5), True), lambda a: ops.point_fpfh(*a))
case("point_fpfh:a NaN row", lambda: (cloud(17, nan=(5,)), normals(cloud(17))), lambda a: ops.point_fpfh(a[0], a[1], 1.0))
case("point_fpfh:NaN rows only", lambda: (cloud(17, nan=True), cloud(17, 1)), lambda a: ops.point_fpfh(a[0], a[1], 1.0, want_spfh=True))

case("descriptor_nearest:plain", lambda: (descriptors(17), descriptors(257, 1)), lambda a: ops.descriptor_nearest(*a))
case("descriptor_nearest:masks", lambda: (descriptors(17), descriptors(257, 1), torch.arange(17).cuda() % 3 > 0, (torch.arange(257).cuda() % 2).to(torch.uint8)),
     lambda a: ops.descriptor_nearest(*a))
case("descriptor_nearest:no query", lambda: (descriptors(0), descriptors(17)), lambda a: ops.descriptor_nearest(*a))
case("descriptor_nearest:no target", lambda: (descriptors(17), descriptors(0)), lambda a: ops.descriptor_nearest(*a))

case("ransac_rigid:plain", lambda: (moved(cloud(17), pose()), cloud(17), corr(17)), lambda a: ops.ransac_rigid(*a, n_hyp=64, seed=3))
case("ransac_rigid:hypothesis counts", lambda: (moved(cloud(257), pose()), cloud(257), corr(257)),
     lambda a: ops.ransac_rigid(*a, n_hyp=33, thr=0.2, edge_ratio=0.8, want_hyp_inliers=True))
case("ransac_rigid:no correspondence", lambda: (cloud(17), cloud(17), corr(0)), lambda a: ops.ransac_rigid(*a, n_hyp=8, want_hyp_inliers=True))
case("ransac_rigid:no target row", lambda: (cloud(17), cloud(0), corr(17)), lambda a: ops.ransac_rigid(*a, n_hyp=8))


def _both(n=257):
    s, t = moved(cloud(n), pose()), cloud(n)
    return s, normals(s), t, normals(t)


for mutual in (True, False):
    for refine in (True, False):
        case("register_global:mutual %s refine %s" % (mutual, refine), _both,
             lambda a, m=mutual, r=refine: ops.register_global(*a, radius=1.0, mutual=m, n_hyp=64, seed=1, refine=r, iters=2))
case("register_global:no target row", lambda: _both(17)[:2] + (cloud(0), cloud(0)), lambda a: ops.register_global(*a, n_hyp=8))
case("register_global:one row each", lambda: _both(1), lambda a: ops.register_global(*a, n_hyp=8, max_dist=0.5))

case("voxel_map:empty", lambda: None, lambda a: ops.voxel_map(0.5, (-8.0, -8.0, -8.0), 2, device="cuda"))
for n in ROWS:
    case("voxel_map_insert:%d rows into an empty map" % n, lambda n=n: (ops.voxel_map(0.5, (-8.0, -8.0, -8.0), 1), cloud(n), attr(n, 1)),
         lambda a: ops.voxel_map_insert(*a, stamp=1))
case("voxel_map_insert:onto an overlapping map", lambda: (filled(), cloud(17), attr(17, 1), pose()), lambda a: ops.voxel_map_insert(*a, stamp=2))
case("voxel_map_insert:no channel, forgetting", lambda: (filled(channels=0), cloud(257, 1)), lambda a: ops.voxel_map_insert(*a, stamp=2, min_stamp=2))
case("voxel_map_insert:a NaN row", lambda: (filled(17), cloud(17, nan=(5,)), attr(17, 1)), lambda a: ops.voxel_map_insert(*a, stamp=2))
case("voxel_map_insert:NaN rows only", lambda: (filled(17), cloud(17, nan=True), attr(17, 1)), lambda a: ops.voxel_map_insert(*a, stamp=2))
case("voxel_map_insert:NaN rows only into an empty map", lambda: (ops.voxel_map(0.5, (-8.0, -8.0, -8.0), 1), cloud(17, nan=True), attr(17, 1)),
     lambda a: ops.voxel_map_insert(*a, stamp=2))
case("voxel_map_insert:every row outside", lambda: (filled(17, origin=(0.0, 0.0, 0.0)), moved(cloud(17), pose(-9.0)), attr(17, 1)),
     lambda a: ops.voxel_map_insert(*a, stamp=2))
case("voxel_map_insert:no row", lambda: (filled(17), cloud(0), attr(0, 1)), lambda a: ops.voxel_map_insert(*a, stamp=2))
case("voxel_map_insert:a pure prune", lambda: (filled(17),), lambda a: ops.voxel_map_insert(a[0], min_stamp=2))
case("voxel_map_insert:a pure prune of an empty map", lambda: (ops.voxel_map(0.5, (-8.0, -8.0, -8.0), 1),), lambda a: ops.voxel_map_insert(a[0], min_stamp=2))

# the host reads voxel_map_insert's docstring promises: with a kept row, without one, without rows
HOST_READS = {"voxel_map_insert:onto an overlapping map": 3, "voxel_map_insert:a NaN row": 3, "voxel_map_insert:NaN rows only": 2,
              "voxel_map_insert:every row outside": 2, "voxel_map_insert:no row": 1, "voxel_map_insert:a pure prune": 1,
              "voxel_downsample:257 rows": 2, "voxel_downsample:NaN rows only": 1, "cloud_index:257 rows": 1, "cloud_index:0 rows": 0}


# ---- the recorder ------------------------------------------------------------------------------------------------------------------------
def run(name):
    """-> dict(calls = [[entry point, {argument: its value, or "null" / "set" for a pointer}], ...], cpu, item) of one case"""
    given, call = CASES[name]
    args = given()
    torch.cuda.synchronize()
    protos = _lib.prototypes()
    log, reads = [], dict(cpu=0, item=0)
    real_call, real_cpu, real_item = _lib.call, torch.Tensor.cpu, torch.Tensor.item

    def logged(entry, *a, **kw):
        _, types, names = protos[entry]
        assert len(a) == len(names), entry
        seen = {}
        for value, kind, arg in zip(a, types, names):
            if arg == "stream":
                continue
            if kind is ctypes.c_void_p:
                seen[arg] = "null" if not value else "set"
            else:
                seen[arg] = float(value) if kind is ctypes.c_float else int(value)
        log.append([entry, seen])
        return real_call(entry, *a, **kw)

    def cpu(t, *a, **kw):
        reads["cpu"] += 1
        return real_cpu(t, *a, **kw)

    def item(t):
        reads["item"] += 1
        return real_item(t)

    _lib.call, torch.Tensor.cpu, torch.Tensor.item = logged, cpu, item
    try:
        call(args)
    finally:
        _lib.call, torch.Tensor.cpu, torch.Tensor.item = real_call, real_cpu, real_item
    torch.cuda.synchronize()
    return dict(calls=log, **reads)


@functools.lru_cache(None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_is_whole():
    assert set(CASES) == set(_golden()) and set(HOST_READS) <= set(CASES)
    wrappers = {name.split(":")[0] for name in CASES}
    assert wrappers == {"voxel_downsample", "point_normals", "cloud_index", "cloud_nearest", "icp_point_to_plane", "point_fpfh", "descriptor_nearest",
                        "ransac_rigid", "register_global", "voxel_map", "voxel_map_insert"}
    entries = {c[0] for got in _golden().values() for c in got["calls"]}                # every entry point of the four sources is launched
    assert entries >= {"cmr_cloud_bounds_f32", "cmr_voxel_keys_f32", "cmr_segment_heads_i64", "cmr_segment_reduce_f32", "cmr_point_normals_f32",
                       "cmr_cloud_gather4_f32", "cmr_cloud_nearest_f32", "cmr_icp_point_to_plane_f32", "cmr_point_fpfh_f32",
                       "cmr_descriptor_nearest_f32", "cmr_ransac_rigid_f32", "cmr_voxel_map_keys_f32", "cmr_voxel_map_plan_i64", "cmr_voxel_map_write_f32"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_launches(name):
    got = json.loads(json.dumps(run(name)))
    if name in HOST_READS:
        assert got["cpu"] + got["item"] == HOST_READS[name]
    assert got == _golden()[name]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_cloud_launches_gpu.py --record")
    got = {name: run(name) for name in CASES}
    for name, n in HOST_READS.items():
        assert got[name]["cpu"] + got[name]["item"] == n, (name, got[name]["cpu"], got[name]["item"])
    with open(GOLDEN, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
    print("%d cases recorded, %d launches" % (len(got), sum(len(g["calls"]) for g in got.values())))
