"""A small host-side writer of single-channel float maps as PFM (Test_Geo.py / Test_Agent.py --dense-depth): the header
"Pf\\n<width> <height>\\n-1.0\\n" -- a negative scale means little-endian -- then height x width float32, rows from the BOTTOM one up."""
import numpy as np


def write_pfm(path, image, empty=0.0):
    """image [h, w] floats -> the file at `path`; every value that is not finite (the +inf of an unfilled pixel, a NaN) is written as
    `empty`.  Returns (h, w)."""
    a = np.asarray(image.detach().cpu() if hasattr(image, "detach") else image)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_pfm: image must be [h, w], got %s" % (a.shape,))
    a = a.astype("<f4")
    a = np.where(np.isfinite(a), a, np.float32(empty)).astype("<f4")
    h, w = a.shape
    with open(path, "wb") as fh:
        fh.write(("Pf\n%d %d\n-1.0\n" % (w, h)).encode("ascii"))
        fh.write(np.ascontiguousarray(a[::-1]).tobytes())
    return h, w
