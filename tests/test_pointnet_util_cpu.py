"""CPU tier: the host-side / view-only members of models/pointnet_util.py that the package exports by the reference's names
(pc_normalize :12-17, sample_and_group_all :136-153) -- against their definitions and against the reference's own outputs on the same
inputs (tests/golden/pointnet_util_host.npz, tests/golden/make_golden_pointnet_util_host.py)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cmr_agent_amd.models import pointnet_util as PU  # noqa: E402


def _inputs():
    g = torch.Generator().manual_seed(9)
    return torch.randn(2, 37, 3, generator=g) * 3.0 + 1.5, torch.randn(2, 37, 5, generator=g)


def test_pc_normalize_and_sample_and_group_all_by_definition():
    xyz, pts = _inputs()
    pc = xyz[0].numpy()
    out = PU.pc_normalize(pc)
    assert isinstance(out, np.ndarray) and out.shape == pc.shape
    assert np.abs(out.mean(axis=0)).max() <= 1e-6 and abs(np.sqrt((out ** 2).sum(axis=1)).max() - 1.0) <= 1e-6
    assert np.abs(PU.pc_normalize(xyz[0]).numpy() - out).max() <= 1e-6            # tensor in, tensor out, same values
    new_xyz, new_points = PU.sample_and_group_all(xyz, pts)
    assert tuple(new_xyz.shape) == (2, 1, 3) and float(new_xyz.abs().max()) == 0.0
    assert tuple(new_points.shape) == (2, 1, 37, 8)
    assert torch.equal(new_points[:, 0, :, :3], xyz) and torch.equal(new_points[:, 0, :, 3:], pts)
    assert torch.equal(PU.sample_and_group_all(xyz, None)[1], xyz.view(2, 1, 37, 3))
    for name in ("timeit", "pc_normalize", "square_distance", "index_points", "farthest_point_sample", "query_ball_point", "knn_point",
                 "sample_and_group", "sample_and_group_all", "PointNetSetAbstraction", "PointNetSetAbstractionMsg",
                 "PointNetFeaturePropagation"):
        assert hasattr(PU, name), name                                               # every public name of the reference's module


def test_against_the_imported_reference():
    """The reference's own pc_normalize / sample_and_group_all on the same inputs, as tests/golden/make_golden_pointnet_util_host.py
    recorded them (pointnet_util_host.npz): bit for bit."""
    import golden_util as G
    fx = G.load_case("pointnet_util_host")
    xyz, pts = _inputs()
    got = {"pc_normalize": PU.pc_normalize(xyz[1].numpy())}
    for tag, p in (("pts", pts), ("none", None)):
        got["sample_and_group_all_%s_xyz" % tag], got["sample_and_group_all_%s_points" % tag] = PU.sample_and_group_all(xyz, p)
    assert sorted(got) == sorted(fx)
    for name, a in got.items():
        a = a.numpy() if torch.is_tensor(a) else np.asarray(a)
        assert tuple(fx[name]["shape"]) == a.shape and fx[name]["stride"] == 1, name
        assert fx[name]["sample"].dtype == a.dtype and np.array_equal(fx[name]["sample"], a.reshape(-1)), name
