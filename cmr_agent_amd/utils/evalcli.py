"""Command-line helpers shared by Test_Geo.py and Test_Agent.py: the round lists of --guided / --refine and the closing recall block."""
import numpy as np


def guided_rounds(ap, radii, thrs, max_radius):
    """'R[,R...]' and the optional 'T[,T...]' of --guided / --refine -> (radii, thrs), one pair per round; ap.error on a malformed list."""
    try:
        radii = tuple(int(v) for v in radii.split(","))
        thrs = tuple(float(v) for v in thrs.split(",")) if thrs is not None else tuple(max(1.0, r / 1.5) for r in radii)
    except ValueError:
        ap.error("window radii must be integers and thresholds numbers, comma separated")
    if len(radii) != len(thrs) or not all(0 <= r <= max_radius for r in radii) or not all(0.0 < t < float("inf") for t in thrs):
        ap.error("need one threshold > 0 per window radius, radii in [0, %d]" % max_radius)
    return radii, thrs


def print_recall(rte, rre, prefix=""):
    """Test_Agent.py's closing lines (registration recall: RTE < 5 and RRE < 10; mean / std of the recalled pairs), each with `prefix`."""
    rte, rre = np.array(rte), np.array(rre)
    mask = (rte < 5) & (rre < 10)
    print(prefix + "Registration Recall:", mask.sum() / mask.shape[0])
    if mask.any():
        print(prefix + 'RTE Mean:', rte[mask].mean(), 'RTE Std:', rte[mask].std())
        print(prefix + 'RRE Mean:', rre[mask].mean(), 'RRE Std:', rre[mask].std())
