"""numpy restatement of the scan descriptor and its ring-shift match (csrc/scan_descriptor.hip), written from
include/cmr_hip.h: every operation on float32 arrays, so every product, sum, square root and quotient is rounded on its own, in the order
the header states.  The kernels are compared with it EXACTLY: descriptors, counts, distances as bits, shifts.

Also here: an independent float64 statement of the bins (hypot, arctan2, floor) with the rows near a bin edge flagged, the ops' interface
on the restatement (CPU stand-ins for tests of the file layer), and the synthetic drive the loop search is tested on."""
import functools

import numpy as np

F32 = np.float32
BINNED, DROPPED, OUTSIDE = 0, 1, 2
QUIET = dict(invalid="ignore", over="ignore", divide="ignore", under="ignore")


def directions(bins):
    """-> float32 [bins / 4 - 1, 2] = (cos, sin) of the edges inside the first quadrant of a circle cut into `bins`, float64 rounded once"""
    ang = np.array([k * 2.0 * np.pi / bins for k in range(1, bins // 4)], dtype=np.float64)
    return np.stack([np.cos(ang), np.sin(ang)], 1).astype(F32).reshape(-1, 2)


def quadrant(x, y):
    """-> (q, u, v): the quadrant of (x, y) and the direction turned into the first one, by exact swaps and negations"""
    q = np.zeros(x.shape, np.int64)
    u, v = np.zeros_like(x), np.zeros_like(y)                          # x = y = 0 keeps q = 0, (0, 0)
    for k, mask, uu, vv in ((0, (x > 0) & (y >= 0), x, y), (1, (x <= 0) & (y > 0), y, -x), (2, (x < 0) & (y <= 0), -x, -y),
                            (3, (x >= 0) & (y < 0), -y, x)):
        q[mask], u[mask], v[mask] = k, uu[mask], vv[mask]
    return q, u, v


def column(x, y, dirs, search=False):
    """The azimuth bin of every (x, y) on the table `dirs` of 4 (len(dirs) + 1) bins: q quarter + m, m the COUNT of table entries with
    fp32(v c_k) >= fp32(u s_k) as the header states it, or with search=True the lower end of the kernels' bisection (csrc/cmr_scan_rows.h)."""
    quarter = len(dirs) + 1
    q, u, v = quadrant(x, y)
    with np.errstate(**QUIET):
        if search:
            m, end = np.zeros(x.shape, np.int64), np.full(x.shape, quarter - 1, np.int64)
            while (m < end).any():
                go = m < end
                mid = np.minimum((m + end) >> 1, quarter - 2)          # a row that is done may point past the table
                holds = v * dirs[mid, 0] >= u * dirs[mid, 1]
                m, end = np.where(go & holds, mid + 1, m), np.where(go & ~holds, mid, end)
        else:
            m = (v[:, None] * dirs[None, :, 0] >= u[:, None] * dirs[None, :, 1]).sum(1)
    return q * quarter + m


def tables(R, S, min_range, max_range):
    """-> (ring_edge2 float32 [R + 1], sector_dir float32 [S / 4 - 1, 2]), computed in float64 and rounded"""
    edge = np.array([(min_range + (max_range - min_range) * j / R) ** 2 for j in range(R + 1)], dtype=np.float64)
    return edge.astype(F32), directions(S)


def rows(points, R, S, min_range=0.0, max_range=80.0, height=2.0, search=False):
    """Per row of points [N, >= 3]: -> dict(state, ring, sector, value); ring and sector mean something where state is BINNED.
    search=True finds the sector by the kernel's bisection instead of the count."""
    p = np.asarray(points, dtype=F32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    e2, dirs = tables(R, S, min_range, max_range)
    with np.errstate(**QUIET):
        dropped = ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z))
        r2 = x * x + y * y                                             # float32 arrays: three roundings
        outside = ~dropped & ((r2 < e2[0]) | (r2 >= e2[R]))
        ring = (r2[:, None] >= e2[None, 1:R]).sum(1)
        value = z + F32(height)
    state = np.where(dropped, DROPPED, np.where(outside, OUTSIDE, BINNED))
    return dict(state=state, ring=ring, sector=column(x, y, dirs, search), value=value)


@functools.lru_cache(maxsize=None)
def planted(bins):
    """Directions (x, y) float32 [n, 2] on which a bin of a circle cut into `bins` is decided: in every quadrant, every table direction
    (c_k, s_k) scaled by 2^-20, 1 and 2^20, each also one ulp to either side in either coordinate; the four axes and the origin (with
    zeros of both signs); rows with a subnormal coordinate; rows at 1e19, whose squares overflow.  Read only."""
    first = []
    for scale in (2.0 ** -20, 1.0, 2.0 ** 20):
        d = directions(bins) * F32(scale)                              # a power of two: exact
        c, s = d[:, 0], d[:, 1]
        for cc, ss in ((c, s), (np.nextafter(c, F32(np.inf)), s), (np.nextafter(c, F32(0)), s), (c, np.nextafter(s, F32(np.inf))),
                       (c, np.nextafter(s, F32(0)))):
            first.append(np.stack([cc, ss], 1))
    tiny, huge = F32(1e-45), F32(1e19)
    first.append(np.array([(1, 0), (0, 0), (tiny, 1), (1, tiny), (tiny, tiny), (tiny, 0), (huge, huge), (huge, 1), (1, huge), (huge, tiny), (huge, 0)], F32))
    uv = np.concatenate(first).astype(F32)
    u, v = uv[:, 0], uv[:, 1]
    out = np.concatenate([np.stack([u, v], 1), np.stack([-v, u], 1), np.stack([-u, -v], 1), np.stack([v, -u], 1)]).astype(F32)
    out.setflags(write=False)
    return out


def describe(points, R, S, min_range=0.0, max_range=80.0, height=2.0):
    """-> (desc float32 [R, S], (binned, dropped, outside))"""
    w = rows(points, R, S, min_range, max_range, height)
    desc = np.zeros((R, S), F32)
    sel = (w["state"] == BINNED) & (w["value"] > 0)
    np.maximum.at(desc, (w["ring"][sel], w["sector"][sel]), w["value"][sel])
    return desc, tuple(int((w["state"] == s).sum()) for s in (BINNED, DROPPED, OUTSIDE))


def rows64(points, R, S, min_range=0.0, max_range=80.0, tol=1e-6):
    """The bins stated independently in float64: ring = floor of the radius' share of the range, sector = floor of arctan2's share of the
    circle.  near = rows whose radius lies within tol (relative) of a ring edge or whose direction lies within tol radians of a sector
    edge, and the rows at the origin, whose direction is undefined: there the two statements may differ.  Finite rows only."""
    p = np.asarray(points, dtype=F32).astype(np.float64)
    r = np.hypot(p[:, 0], p[:, 1])
    edges = min_range + (max_range - min_range) * np.arange(R + 1) / R
    outside = (r < min_range) | (r >= max_range)
    ring = np.floor((r - min_range) / (max_range - min_range) * R).astype(np.int64)
    width = 2.0 * np.pi / S
    turn = np.mod(np.arctan2(p[:, 1], p[:, 0]), 2.0 * np.pi) / width
    sector = np.floor(turn).astype(np.int64) % S
    near = (np.abs(r[:, None] - edges[None]).min(1) <= tol * r) | (np.abs(turn - np.round(turn)) * width <= tol) | (r == 0)
    return dict(state=np.where(outside, OUTSIDE, BINNED), ring=ring, sector=sector, near=near)


def unit(desc):
    """desc [D, R, S] -> (unit columns float32 [D, R, S], zero in empty columns; full bool [D, S])"""
    d = np.asarray(desc, dtype=F32)
    n2 = np.zeros((d.shape[0], d.shape[2]), F32)
    with np.errstate(**QUIET):
        for r in range(d.shape[1]):
            n2 = n2 + d[:, r] * d[:, r]
        full = n2 != 0                                                 # n2 == 0 is empty; a NaN sum is not
        e = np.where(full[:, None, :], d / np.sqrt(n2)[:, None, :], F32(0))
    return e.astype(F32), full


def match(queries, cands, limit=None, min_cols=None, all_shifts=False):
    """queries [Q, R, S] against cands [N, R, S] -> (dist float32 [Q, N], shift int32 [Q, N]); with all_shifts also the distance of every
    shift [S, Q, N] (NaN where the shift does not count)."""
    eq, fq = unit(queries)
    ec, fc = unit(cands)
    (Q, R, S), N = eq.shape, ec.shape[0]
    min_cols = S // 4 if min_cols is None else min_cols
    best, shift, every = np.full((Q, N), np.nan, F32), np.full((Q, N), -1, np.int32), []
    with np.errstate(**QUIET):
        for k in range(S):
            c, f = np.roll(ec, -k, axis=2), np.roll(fc, -k, axis=1)    # column j of c is candidate column (j + k) mod S
            dot = np.zeros((Q, N, S), F32)
            for r in range(R):
                dot = dot + eq[:, None, r, :] * c[None, :, r, :]
            both = fq[:, None, :] & f[None, :, :]
            total, cnt = np.zeros((Q, N), F32), np.zeros((Q, N), np.int64)
            for j in range(S):
                total = np.where(both[:, :, j], total + dot[:, :, j], total)
                cnt += both[:, :, j]
            d = np.where(cnt >= min_cols, F32(1) - total / cnt.astype(F32), F32(np.nan)).astype(F32)
            every.append(d)
            better = ~np.isnan(d) & ((shift < 0) | (d < best))
            best, shift = np.where(better, d, best), np.where(better, k, shift).astype(np.int32)
    if limit is not None:
        off = np.arange(N)[None, :] >= np.asarray(limit)[:, None]
        best, shift = np.where(off, F32(np.nan), best), np.where(off, -1, shift).astype(np.int32)
        every = [np.where(off, F32(np.nan), d) for d in every]
    return (best, shift, np.stack(every)) if all_shifts else (best, shift)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


# ---- the ops' interface on the restatement (CPU stand-ins for tests of the file layer) -------------------------------------------------------
def ops_scan_descriptor(points, rings=20, sectors=60, max_range=80.0, min_range=0.0, height=2.0):
    import torch
    from cmr_agent_amd import ops
    desc, counts = describe(points.cpu().numpy(), rings, sectors, min_range, max_range, height)
    return ops.ScanDescriptor(torch.from_numpy(desc), *counts)


def ops_scan_match(queries, cands, limit=None, min_cols=None):
    import torch
    from cmr_agent_amd import ops
    dist, shift = match(queries.cpu().numpy(), cands.cpu().numpy(), None if limit is None else limit.cpu().numpy(), min_cols)
    return ops.ScanMatch(torch.from_numpy(dist), torch.from_numpy(shift))


# ---- a synthetic drive: a town seen from a circle driven 1.25 times ----------------------------------------------------------------------------
DRIVE = dict(rings=8, sectors=24, max_range=25.0, height=2.0, gap=6)
SENSOR = 1.73                                                           # the sensor's height above the ground
LAP, FRAMES, RADIUS, SIDE, TURNED, TURN = 16, 20, 18.0, 0.6, (17, 19), np.radians(140.0)


def rz(a):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    return T


def town(seed, ground=5000, boxes=40, per_box=120, extent=46.0):
    """-> (points float64 [n, 3], unit normals float64 [n, 3]): the ground at z = -SENSOR and the walls of boxes standing on it"""
    rng = np.random.default_rng(seed)
    rad, ang = extent * np.sqrt(rng.uniform(size=ground)), rng.uniform(0, 2 * np.pi, ground)
    pts = [np.stack([rad * np.cos(ang), rad * np.sin(ang), np.full(ground, -SENSOR)], 1)]
    nrm = [np.tile([0.0, 0.0, 1.0], (ground, 1))]
    for _ in range(boxes):
        c, half, tall = rng.uniform(-extent, extent, 2), rng.uniform(1.5, 5.0, 2), rng.uniform(2.0, 8.0)
        wall, t, z = rng.integers(0, 4, per_box), rng.uniform(-1, 1, per_box), rng.uniform(-SENSOR, tall - SENSOR, per_box)
        along_x = wall < 2                                              # walls 0 and 1 face +-y, walls 2 and 3 face +-x
        sign = np.where(wall % 2 == 0, 1.0, -1.0)
        x = np.where(along_x, t * half[0], sign * half[0])
        y = np.where(along_x, sign * half[1], t * half[1])
        pts.append(np.stack([c[0] + x, c[1] + y, z], 1))
        nrm.append(np.stack([np.where(along_x, 0.0, sign), np.where(along_x, sign, 0.0), np.zeros(per_box)], 1))
    return np.concatenate(pts), np.concatenate(nrm)


def scan(world, normals, pose, max_range):
    """The rows of the world within max_range of the sensor (seen from above), in the sensor's frame -> prepared cloud float32 [7, n]"""
    inv = np.linalg.inv(pose)
    p = world @ inv[:3, :3].T + inv[:3, 3]
    keep = np.hypot(p[:, 0], p[:, 1]) < max_range
    return np.concatenate([p[keep].T, np.zeros((1, keep.sum())), (normals[keep] @ inv[:3, :3].T).T]).astype(F32)


@functools.lru_cache(maxsize=None)
def drive(seed):
    """-> dict(frames: FRAMES prepared clouds float32 [7, n]; poses float64 [FRAMES, 4, 4]: frame n in the world; revisits: the planted
    (later, earlier) positions).  The last FRAMES - LAP frames revisit the first ones SIDE metres to the side, those of TURNED turned by TURN.
    Read only."""
    world, normals = town(seed)
    poses = []
    for n in range(FRAMES):
        a = 2.0 * np.pi * (n % LAP) / LAP
        T = rz(a + np.pi / 2 + (TURN if n in TURNED else 0.0))
        T[:2, 3] = (RADIUS + (SIDE if n >= LAP else 0.0)) * np.array([np.cos(a), np.sin(a)])
        poses.append(T)
    frames = tuple(scan(world, normals, T, DRIVE["max_range"]) for T in poses)
    return dict(frames=frames, poses=np.stack(poses), revisits=tuple((n, n - LAP) for n in range(LAP, FRAMES)))


def drive_descriptors(seed):
    d = drive(seed)
    return np.stack([describe(f[:3].T, DRIVE["rings"], DRIVE["sectors"], 0.0, DRIVE["max_range"], DRIVE["height"])[0] for f in d["frames"]])


@functools.lru_cache(maxsize=None)
def drive_match(seed):
    """-> (dist, shift) of the drive's frames against the frames at least `gap` positions earlier, by the restatement.  Read only."""
    desc = drive_descriptors(seed)
    limit = np.maximum(0, np.arange(FRAMES) - DRIVE["gap"] + 1)
    return match(desc, desc, limit)


def drive_margin(seed):
    """-> (largest distance of a planted revisit, smallest distance of any other compared pair)"""
    dist, _ = drive_match(seed)
    d = drive(seed)
    planted = np.zeros(dist.shape, bool)
    for i, j in d["revisits"]:
        planted[i, j] = True
    return float(dist[planted].max()), float(dist[~planted & ~np.isnan(dist)].min())


# ---- the loop search on the drive: what the CPU tier (stand-ins) and the GPU tier (the command) both check ---------------------------------------
DRIVE_SEED = 3                                                          # test_scan_descriptor_cpu.py checks the margin of this seed


def drive_argv(root, *extra):
    """Writes the drive's frames (frame numbers 3 ..) and its true poses under root once -> the command's arguments for it, with
    --max-desc-dist at the midpoint between the planted revisits and every other pair."""
    import os

    import cloud_icp_reference as I
    from cmr_agent_amd.dataset import align
    d = drive(DRIVE_SEED)
    if not os.path.isdir(os.path.join(root, "vel")):
        I.write_frames(root, d["frames"])
        align.write_poses(os.path.join(root, "poses.txt"), np.stack([np.linalg.inv(d["poses"][0]) @ T for T in d["poses"]]))
    hi, lo = drive_margin(DRIVE_SEED)
    return ["--root", root, "--data-velodyne", "vel", "--sequence", "9", "--rings", str(DRIVE["rings"]), "--sectors", str(DRIVE["sectors"]),
            "--max-range", str(DRIVE["max_range"]), "--height", str(DRIVE["height"]), "--gap", str(DRIVE["gap"]),
            "--max-desc-dist", "%.6f" % (0.5 * (hi + lo)), "--poses", os.path.join(root, "poses.txt")] + list(extra)


def drive_truth(i, j):
    """the pose that maps frame i of the drive into frame j"""
    d = drive(DRIVE_SEED)
    return np.linalg.inv(d["poses"][j]) @ d["poses"][i]


def drive_icp_error(register):
    """ICP's own error on the planted pairs: register(target [7, n], source [7, m], start float64 [4, 4]) -> pose [4, 4], started from
    the truth.  -> (largest rotation error in rad, largest translation error) over the pairs."""
    import cloud_icp_reference as I
    d = drive(DRIVE_SEED)
    errs = [I.pose_error(register(d["frames"][j], d["frames"][i], drive_truth(i, j)), drive_truth(i, j)) for i, j in d["revisits"]]
    return max(e[0] for e in errs), max(e[1] for e in errs)


def check_drive_run(lines, starts, tol_rot, tol_trans, edges_file, first=3):
    """The lines and the edges of a run on drive_argv's files: exactly the planted revisits, each accepted from starts[n], each measured
    pose within (tol_rot, tol_trans) of the truth, and no drift against the poses file, which is the truth.  -> the errors' maxima"""
    import cloud_icp_reference as I
    from cmr_agent_amd import ops
    from cmr_agent_amd.dataset import align
    d = drive(DRIVE_SEED)
    dist, shift = drive_match(DRIVE_SEED)
    S = DRIVE["sectors"]
    assert len(lines) == 5 and lines[4] == "loops: 4 accepted of 4 candidates of %d frames" % FRAMES, lines
    edges = align.read_edges(edges_file)
    assert [(e[0] - first, e[1] - first) for e in edges] == list(d["revisits"])
    worst = [0.0, 0.0]
    for (i, j), line, start, e in zip(d["revisits"], lines, starts, edges):
        w = line.split()
        assert w[:3] == ["loop", str(first + i), "%d:" % (first + j)], line
        assert w[3:19:2] == ["dist", "shift", "yaw", "pairs", "rmse", "iterations", "status", "start"] and len(w) == 24, line
        assert w[4] == "%.4f" % dist[i, j] and int(w[6]) == shift[i, j] and w[8] == "%.2f" % np.degrees(ops.scan_shift_yaw(int(shift[i, j]), S)), line
        assert w[18] == start and w[19:22] == ["->", "accepted", "drift"] and w[16] in ("0", "1"), line
        assert int(w[10]) >= 0.9 * d["frames"][i].shape[1] and int(w[10]) == e[5] and float(w[12]) < 0.05, line
        rot, trans = I.pose_error(e[2], drive_truth(i, j))
        worst = [max(worst[0], rot), max(worst[1], trans)]
        assert rot <= tol_rot and trans <= tol_trans, (i, j, rot, trans, tol_rot, tol_trans)
        assert float(w[22]) <= trans + 1e-4 and float(w[23]) <= np.degrees(rot) + 1e-4, line      # printed to four places
        assert bits(e[3]) == bits(dist[i, j])                                                     # %.9e carries the float32 exactly
    return tuple(worst)
