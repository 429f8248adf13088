"""A small host-side writer of coloured point clouds as binary little-endian PLY:
x, y, z float32 and red, green, blue uchar per vertex (Test_Geo.py / Test_Agent.py --paint)."""
import numpy as np

_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def _np(a):
    return np.asarray(a.detach().cpu() if hasattr(a, "detach") else a)


def colors_to_u8(colors):
    """clamp(rint(255 c), 0, 255) -> uint8; a NaN becomes 0."""
    c = np.rint(255.0 * np.nan_to_num(_np(colors).astype(np.float64), nan=0.0, posinf=1.0, neginf=0.0))
    return np.clip(c, 0, 255).astype(np.uint8)


def write_ply(path, xyz, rgb):
    """xyz [n, 3] floats, rgb [n, 3] uint8 (or floats in [0, 1], converted by colors_to_u8) -> the file at `path`; returns n."""
    xyz, rgb = _np(xyz), _np(rgb)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape:
        raise ValueError("write_ply: xyz and rgb must both be [n, 3], got %s / %s" % (xyz.shape, rgb.shape))
    if rgb.dtype != np.uint8:
        rgb = colors_to_u8(rgb)
    v = np.empty(xyz.shape[0], _VERTEX)
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(v)
    header += "".join("property float %s\n" % n for n in "xyz") + "".join("property uchar %s\n" % n for n in ("red", "green", "blue"))
    with open(path, "wb") as fh:
        fh.write((header + "end_header\n").encode("ascii"))
        fh.write(v.tobytes())
    return len(v)
