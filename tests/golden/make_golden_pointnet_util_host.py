#!/usr/bin/env python3
"""Generates tests/golden/pointnet_util_host.npz by running the REFERENCE's models/pointnet_util.py (pc_normalize :12-17,
sample_and_group_all :136-153) on tests/test_pointnet_util_cpu.py's inputs, imported on CPU through ref_harness.

Run in the authoring container only:   python tests/golden/make_golden_pointnet_util_host.py
"""
import importlib.util
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_harness  # noqa: E402
import golden_util as G  # noqa: E402
from test_pointnet_util_cpu import _inputs  # noqa: E402


def main():
    if not ref_harness.reference_available():
        raise SystemExit("reference tree not present; the committed fixture is used instead")
    ref_harness.load_reference()                  # stubs for the reference's unused top-level imports
    sys.path.insert(0, ref_harness.REF_ROOT)
    try:
        spec = importlib.util.spec_from_file_location("_ref_pointnet_util", os.path.join(ref_harness.REF_ROOT, "models", "pointnet_util.py"))
        R = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(R)
    finally:
        sys.path.remove(ref_harness.REF_ROOT)
    xyz, pts = _inputs()
    out = {"pc_normalize": torch.from_numpy(R.pc_normalize(xyz[1].numpy()))}
    for tag, p in (("pts", pts), ("none", None)):
        new_xyz, new_points = R.sample_and_group_all(xyz, p)
        out["sample_and_group_all_%s_xyz" % tag], out["sample_and_group_all_%s_points" % tag] = new_xyz, new_points
    G.save_case("pointnet_util_host", out)
    print("pointnet_util_host.npz:", ", ".join(sorted(out)))


if __name__ == "__main__":
    main()
