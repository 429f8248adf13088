"""GPU tier of the sparse observation's second stage (CMRAgent.SPARSE_OBS_STAGES = 2): the four maps of
cmr_observation_proj_reach_staged_f32, the four lists of cmr_wino_tile_lists_staged and the list launch with its `nend` bound
(cmr_conv3x3_wino_list_nend_nhwc_f32), through the agent's four-convolution chain against the DENSE entry point on the same inputs, bit for
bit, on NaN-filled outputs: the maps the next stage reads densely (x2, x4) must equal the dense ones everywhere; the maps whose only
reader is the next list launch (x1, x3) must equal them on the live and copy tiles and still hold NaN on the rest -- which also shows that
no live tile of their reader took a NaN in.  Shapes: the smallest whose half-resolution stage the persistent kernel serves -- B = 2 at
80 x 320 (stage 1: 40 x 160, 200 virtual tiles, one lap) and at 88 x 304 (44 x 152, 240 tiles, partial last tile row and column).
tests/test_sparse_obs_stage1_cpu.py shows why the comparison can be exact."""
import functools

import numpy as np
import pytest
import torch

import sparse_obs_reference as S
import sparse_obs_stage1_reference as S1

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOPE = 0.01
GEOMS = {"b2_80x320": (2, 80, 320), "b2_88x304": (2, 88, 304)}
# single points d cells outside the left edge of stage-1 tile (2, i)'s footprint in sample 0, and outside the top edge of tile (2, i)'s in
# the last sample -> (map a, map b) of that tile
EDGE_TILES = {4: (1, (1, 1)), 5: (3, (0, 1)), 6: (5, (0, 1)), 7: (7, (0, 0))}


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _raw(name, *args):
    from cmr_agent_amd import _lib
    rc = getattr(_lib.load(), name)(*args)
    assert rc == 0, (name, rc)


def nans(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def scene(name, B, h, w):
    """-> occupied cells (b, y, x) of the h x w observation"""
    ty, tx = S1.stage1_grid(h, w)
    if name == "none":
        return []
    if name == "all":                                   # one point in every full-resolution tile: every tile of all four maps
        ty, tx = S.tile_grid(h, w)
        return [(b, min(8 * j + 3, h - 1), min(16 * i + 5, w - 1)) for b in range(B) for j in range(ty) for i in range(tx)]
    if name == "corners":
        return [(0, 0, 0), (0, 0, w - 1), (0, h - 1, 0), (0, h - 1, w - 1)]
    if name == "edges":
        return [(0, 40, 32 * i - d) for d, (i, _) in EDGE_TILES.items()] + [(B - 1, 32 - d, 32 * i + 16) for d, (i, _) in EDGE_TILES.items()]
    if name == "random":
        g = np.random.default_rng(11)
        return [(int(g.integers(B)), int(g.integers(h)), int(g.integers(w))) for _ in range(12)]
    raise KeyError(name)


SCENES = ("none", "all", "corners", "edges", "random")


@functools.lru_cache(maxsize=None)
def layers():
    """the chain's weights (64 -> 128 with a residual, then three 128 -> 128 with a bias; pools after the second and the fourth),
    real-valued, packed once"""
    from cmr_agent_amd.models import _pack
    g = torch.Generator().manual_seed(5)
    ws = [torch.randn(128, 64, 3, 3, generator=g) * 0.05] + [torch.randn(128, 128, 3, 3, generator=g) * 0.04 for _ in range(3)]
    bs = [None] + [(torch.randn(128, generator=g) * 0.1).to(DEV) for _ in range(3)]
    return [_pack.winograd_u(w).to(DEV).contiguous() for w in ws], bs


def _shapes(B, h, w):
    return (B, h, w, 128), (B, h // 2, w // 2, 128), (B, h // 2, w // 2, 128), (B, h // 4, w // 4, 128)


def dense(x, res):
    us, bs = layers()
    B, h, w, _ = x.shape
    ys = [nans(*s) for s in _shapes(B, h, w)]
    src = x
    for k in range(4):
        hh, ww = (h, w) if k < 2 else (h // 2, w // 2)
        _raw("cmr_conv3x3_wino_nhwc_f32", _p(src), B, hh, ww, 64 if k == 0 else 128, _p(us[k]), _p(bs[k]), _p(res) if k == 0 else None, None,
             _p(ys[k]), 128, SLOPE, 2 if k & 1 else 1, 0, 1, _stream())
        src = ys[k]
    return ys


@functools.lru_cache(maxsize=None)
def dense_empty(geom):
    """(res, the four maps of the empty projection) by the DENSE entry point -- shared by the scenes of a geometry, never written to"""
    B, h, w = GEOMS[geom]
    res = torch.randn(B, h, w, 128, generator=torch.Generator().manual_seed(17)).to(DEV)
    return res, dense(torch.zeros(B, h, w, 64, device=DEV), res)


def listed(x, res, lists, empty):
    us, bs = layers()
    B, h, w, _ = x.shape
    ys = [nans(*s) for s in _shapes(B, h, w)]
    src = x
    for k in range(4):
        hh, ww = (h, w) if k < 2 else (h // 2, w // 2)
        order, nlive = lists[k][0], lists[k][1]
        nend = lists[k][2] if len(lists[k]) == 3 else None
        _raw("cmr_conv3x3_wino_list_nend_nhwc_f32", _p(src), B, hh, ww, 64 if k == 0 else 128, _p(us[k]), _p(bs[k]), _p(res) if k == 0 else None,
             _p(ys[k]), 128, SLOPE, 2 if k & 1 else 1, _p(order), _p(nlive), _p(nend), _p(empty[k]), 0, 1, _stream())
        src = ys[k]
    return ys


def exact(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        raise AssertionError("%s: %d of %d elements differ (%d NaN = never written), first at %s" % (
            what, int(bad.sum()), got.numel(), int(torch.isnan(got).sum()), bad.nonzero()[0].tolist()))


def exact_where_written(got, want, cls, what):
    """cls [B, ty, tx] of the map's own tile grid: live and copy tiles equal the dense map, the rest still holds the NaN fill"""
    B, H, W, _ = got.shape
    written = torch.from_numpy(S1.tile_pixels(cls != 0, H, W)).to(DEV)
    exact(got[written], want[written], what + ", live and copy tiles")
    rest = got[~written]
    assert bool(torch.isnan(rest).all()), "%s: %d elements of rest tiles were written" % (what, int((~torch.isnan(rest)).sum()))


def numpy_maps(cells, B, h, w):
    return S.reach_maps(cells, B, h, w) + S1.reach_maps_stage1(cells, B, h, w)


def flat_reach(maps):
    return torch.from_numpy(np.concatenate([np.asarray(m).reshape(-1) for m in maps])).to(DEV)


def check_lists(lists, maps, nco=2):
    for s in (0, 1):
        ra, rb = maps[2 * s], maps[2 * s + 1]
        wo, wl, we = S1.three_part_list(ra, rb, nco)
        o, nl, ne = lists[2 * s]
        assert (int(nl), int(ne)) == (wl, we) and np.array_equal(o.cpu().numpy(), wo), (s, "first list")
        wo, wl = S.tile_lists(rb, nco)
        o, nl = lists[2 * s + 1]
        assert int(nl) == wl and np.array_equal(o.cpu().numpy(), wo), (s, "second list")


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_four_list_convolutions_equal_the_dense_chain(geom, name):
    from cmr_agent_amd import ops
    B, h, w = GEOMS[geom]
    cells = scene(name, B, h, w)
    res, empty = dense_empty(geom)
    g = torch.Generator().manual_seed(23)
    x = torch.zeros(B, h, w, 64)
    for b, yy, xx in cells:
        x[b, yy, xx] = torch.randn(64, generator=g) + 0.1
    x = x.to(DEV)
    want = dense(x, res)
    maps = numpy_maps(cells, B, h, w)
    reach = flat_reach(maps)
    lists = ops.wino_tile_lists_staged(reach, B, h, w, 128, 128)
    assert not reach.any()                                                    # consumed: cleared for the next observation
    check_lists(lists, maps)
    counts = [int(l[1]) for l in lists]
    totals = [maps[0].size * 2] * 2 + [maps[2].size * 2] * 2
    if name == "none":
        assert counts == [0, 0, 0, 0] and int(lists[0][2]) == 0 and int(lists[2][2]) == 0
    elif name == "all":
        assert counts == totals and int(lists[0][2]) == totals[0] and int(lists[2][2]) == totals[2]
    elif name == "edges":
        for d, (i, marks) in EDGE_TILES.items():
            assert (int(maps[2][0, 2, i]), int(maps[3][0, 2, i])) == marks, d
            assert (int(maps[2][B - 1, 2, i]), int(maps[3][B - 1, 2, i])) == marks, d
    if name != "all":
        assert int(lists[0][2]) < totals[0] and int(lists[2][2]) < totals[2]          # some tiles of x1 and x3 are left unwritten
    got = listed(x, res, lists, empty)
    cls0, cls1 = S1.copy_class(maps[0], maps[1]), S1.copy_class(maps[2], maps[3])
    exact(got[1], want[1], "x2: stage 0, second convolution + pool (%d of %d tiles live)" % (counts[1], totals[1]))
    exact(got[3], want[3], "x4: stage 1, second convolution + pool (%d of %d tiles live)" % (counts[3], totals[3]))
    exact_where_written(got[0], want[0], cls0, "x1: stage 0, first convolution (%d live)" % counts[0])
    exact_where_written(got[2], want[2], cls1, "x3: stage 1, first convolution (%d live)" % counts[2])


@pytest.mark.parametrize("geom", list(GEOMS))
def test_observation_marks_four_maps(geom):
    """cmr_observation_proj_reach_staged_f32 against the numpy rules applied to the cells the kernel itself reports; points that round onto
    the last row and column, points 4 .. 7 cells off a stage-1 footprint, points out of view or outside the predicted overlap."""
    from cmr_agent_amd import ops
    B, h, w = GEOMS[geom]
    pix = [(0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0), (w - 1.4, 20.0), (50.0, h - 1.4), (w - 1.5, h - 1.5),
           (32.0 - 4, 40.0), (96.0 - 5, 40.0), (160.0 - 6, 40.3), (224.0 - 7, 39.6), (48.0, 32.0 - 4), (112.0, 32.0 - 5), (176.4, 32.0 - 6),
           (240.0, 32.0 - 7), (15.5, 7.5), (16.5, 8.5), (-0.4, 3.0), (w - 0.6, 3.0), (50.0, h - 0.6), (60.0, -0.2)]
    N = 32
    pc = torch.zeros(B, N, 4)
    pc[:, :, 2] = 1.0
    ov = torch.zeros(B, N, dtype=torch.uint8)
    for b in range(B):
        for k, (u, v) in enumerate(pix):
            if (k + b) % 2 and 7 <= k < 15:
                continue                                                 # the two samples see different subsets
            z = 1.0 + 0.5 * ((k + b) % 3)
            pc[b, k] = torch.tensor([u * z, v * z, z, 0.0])
            ov[b, k] = 1
        pc[b, 30] = torch.tensor([70.0, 30.0, 1.0, 0.0])            # in view, not in the predicted overlap
        pc[b, 31] = torch.tensor([70.0, 30.0, -1.0, 0.0])           # behind the camera
        ov[b, 31] = 1
    feat = torch.randn(B * N, 64, generator=torch.Generator().manual_seed(2))
    dev = lambda t: t.to(DEV).contiguous()
    proj = torch.zeros(B, h, w, 64, device=DEV)
    cnt = torch.zeros(B * h * w, device=DEV)
    cell = torch.full((B * N,), -1, dtype=torch.int32, device=DEV)
    st = torch.empty(B * N, 8, device=DEV)
    nt, nt1 = ops.reach_tiles(B, h, w)
    assert (nt, nt1) == (B * np.prod(S.tile_grid(h, w)), B * np.prod(S1.stage1_grid(h, w)))
    reach = torch.zeros(2 * nt + 2 * nt1, dtype=torch.uint8, device=DEV)
    args = (dev(pc.view(-1, 4)), dev(feat), dev(ov.view(-1)), dev(torch.eye(4).repeat(B, 1, 1)), dev(torch.eye(3).repeat(B, 1, 1)),
            torch.zeros(B, 4, device=DEV), B, N, h, w, proj, cnt, cell, st)
    ops.observation_proj(*args, reach=reach)
    cells = [(int(v) // (h * w), (int(v) % (h * w)) // w, int(v) % w) for v in cell.cpu().numpy() if v >= 0]
    assert set(cells) == set(S.occupied(proj.cpu().numpy())) and any(y == h - 1 for _, y, _ in cells) and any(x == w - 1 for _, _, x in cells)
    maps = numpy_maps(cells, B, h, w)
    got = reach.cpu().numpy()
    off = 0
    for m in maps:
        assert np.array_equal(got[off:off + m.size].reshape(m.shape), m), off
        off += m.size
    assert 0 < maps[2].sum() < maps[3].sum() < maps[3].size
    # the two-map call marks the first two maps alone, and the same ones
    two = torch.zeros(2 * nt, dtype=torch.uint8, device=DEV)
    ops.observation_proj(*args, reach=two)
    assert np.array_equal(two.cpu().numpy(), got[:2 * nt])


@pytest.mark.parametrize("geom", list(GEOMS))
def test_staged_lists_against_numpy(geom):
    """cmr_wino_tile_lists_staged on random maps (not only those a projection can make): orders, counts, maps cleared."""
    from cmr_agent_amd import ops
    B, h, w = GEOMS[geom]
    g = np.random.default_rng(31)
    shapes = [(B,) + S.tile_grid(h, w)] * 2 + [(B,) + S1.stage1_grid(h, w)] * 2
    for p in (0.0, 0.04, 0.3, 1.0):
        maps = [(g.random(s) < p).astype(np.uint8) for s in shapes]
        maps[0] &= (g.random(shapes[0]) < 0.7).astype(np.uint8)
        reach = flat_reach(maps)
        lists = ops.wino_tile_lists_staged(reach, B, h, w, 128, 128)
        check_lists(lists, maps)
        assert not reach.any()


def _env_data(B, h, w, N, seed):
    """an observation context without the geometric model: a cloud that projects into the middle of the map (about a tenth of its width
    and height around the centre at the nearest depth), so that both stages keep tiles of all three kinds"""
    g = torch.Generator().manual_seed(seed)
    pc = torch.stack([(torch.rand(B, N, generator=g) - 0.5) * 1.2, (torch.rand(B, N, generator=g) - 0.5) * 0.5, 8 + 12 * torch.rand(B, N, generator=g)], 1)
    img = (torch.rand(1, 64, 1, 1, generator=g) - 0.5) * 2 + 0.3 * (torch.rand(B, 64, h, w, generator=g) - 0.5)
    return dict(pc=pc, K=torch.tensor([[0.6 * w, 0, w / 2], [0, 0.6 * w, h / 2], [0, 0, 1.0]]).repeat(B, 1, 1),
                pc_overlap_pred=torch.rand(B, N, generator=g) > 0.4,
                pc_geo_feat=torch.nn.functional.normalize(torch.rand(B, 64, N, generator=g) - 0.5, dim=1),
                img_geo_feat=torch.nn.functional.normalize(img, dim=1))


def _registration(agent, cfg, data, steps, both):
    """`steps` agent steps from the identity pose.  both: every observation goes through the agent twice -- with SPARSE_OBS_STAGES as it is
    and with 1 -- so that the two forwards see the SAME projected map (two observations of one pose differ in the last bit: the
    scatter-mean adds with float atomics)."""
    from cmr_agent_amd.environment import environment as env
    from cmr_agent_amd.models import CMRAgent
    out = []
    data = dict(data)
    pose, _ = env.init(dict(data, P=torch.eye(4, device=data['pc'].device).repeat(data['pc'].shape[0], 1, 1)))
    for _ in range(steps):
        s2, s3 = env.observation_from_a_pose(data, pose, materialize_state_2d=False)
        r, t, v = agent(s2, s3)
        out += [r, t, v]
        if both:
            was, CMRAgent.SPARSE_OBS_STAGES = CMRAgent.SPARSE_OBS_STAGES, 1
            try:
                out += list(agent(s2, s3))
            finally:
                CMRAgent.SPARSE_OBS_STAGES = was
        ar, at = agent.action_from_logits(r, t, deterministic=True)
        pose = env.step(ar, at, pose, cfg)
    return out + [pose], data['_cmr_obs'].agent_cache


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_two_step_registration_with_one_and_two_stages(mode, monkeypatch):
    """Poses, logits and values of a two-step registration with SPARSE_OBS_STAGES 2 and 1 on an 80 x 320 agent map, B = 2: the smallest whose
    stage 1 is served (asserted).  The comparisons are those of tests/test_sparse_obs_gpu.py's switch test."""
    import parity_e2e
    from cmr_agent_amd.config import KittiConfiguration
    from cmr_agent_amd.models import CMRAgent
    cfg = KittiConfiguration(cropped_img_H=320, cropped_img_W=1280, num_pt=1024, device="cpu", action_num=2)
    assert (cfg.image_H, cfg.image_W) == (80, 320)
    _, agent, _, _ = parity_e2e.build_models(cfg)
    data = {k: v.cuda() for k, v in _env_data(2, 80, 320, 1024, 3).items()}
    cfg.r_steps, cfg.t_steps = cfg.r_steps.cuda(), cfg.t_steps.cuda()
    assert CMRAgent.SPARSE_OBS_STAGES == 2 and CMRAgent.sparse_obs()
    fresh = lambda: {k: v for k, v in data.items() if k != '_cmr_obs'}       # every run is a registration of its own (new context)

    def run(both):
        with torch.no_grad():
            if mode == "eager":
                return _registration(agent, cfg, fresh(), 2, both)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                _registration(agent, cfg, fresh(), 2, both)                 # plans and kernel attributes outside the capture
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out, cache = _registration(agent, cfg, fresh(), 2, both)
            graph.replay()
            graph.replay()                                                   # the second replay starts from what the first one left
            torch.cuda.synchronize()
            return [o.clone() for o in out], cache

    out, cache = run(both=True)
    assert "x3_0" in cache and "x4_0" in cache and cache["lists_staged"] is not None
    l4 = cache["lists_staged"]
    n1, n2, n3, n4 = (int(l[1]) for l in l4)
    e1, e3 = int(l4[0][2]), int(l4[2][2])
    t0, t1 = l4[0][0].numel(), l4[2][0].numel()
    assert (t0, t1) == (800, 200)
    assert 0 < n1 <= n2 < t0 and 0 < n3 <= n4 < t1, (n1, n2, n3, n4)          # some tiles multiplied, some not, in both stages
    assert n1 <= e1 < t0 and n3 <= e3 < t1, (e1, e3)                          # ... and some neither multiplied nor copied
    for k in range(2):
        two, one = out[6 * k:6 * k + 3], out[6 * k + 3:6 * k + 6]
        for a, b, what in zip(two, one, ("rotation logits", "translation logits", "value")):
            assert torch.equal(a, b), (k, what, float((a - b).abs().max()))
    # ... and a registration of its own with one stage from the start: the same poses to the bit (logits to the atomics' rounding)
    monkeypatch.setattr(CMRAgent, "SPARSE_OBS_STAGES", 1)
    ref, cache = run(both=False)
    assert "x3_0" not in cache and cache["lists_staged"] is None and "x1_0" in cache
    assert torch.equal(out[-1], ref[-1])
    for k in range(2):
        for a, b in zip(out[6 * k:6 * k + 3], ref[3 * k:3 * k + 3]):
            assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max()))
