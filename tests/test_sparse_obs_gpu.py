"""GPU tier of the sparse observation (CMRAgent.SPARSE_OBS): the tile marks of cmr_observation_proj_reach_f32, the lists of
cmr_wino_tile_lists and the list-driven Winograd launch cmr_conv3x3_wino_list_nhwc_f32 against the DENSE entry point on the same inputs,
bit for bit (torch.equal on NaN-filled outputs: a tile that is neither multiplied nor copied shows), and against the numpy restatement of
the rules (sparse_obs_reference.py).  Shapes: the smallest the wave-specialised kernel accepts -- 200 virtual tiles (B = 2, 40 x 160, 128
couts: one lap of the persistent grid), 300 (B = 3: a second lap, and fewer live tiles than workgroups), and a 44 x 152 map whose last
tile row and column are partial.  tests/test_sparse_obs_cpu.py shows why the comparison can be exact."""
import functools

import numpy as np
import pytest
import torch

import sparse_obs_reference as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOPE = 0.01
GEOMS = {"b2_40x160": (2, 40, 160), "b3_40x160": (3, 40, 160), "b2_44x152": (2, 44, 152)}


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
    """-> occupied cells (b, y, x)"""
    ty, tx = S.tile_grid(h, w)
    if name == "none":
        return []
    if name == "all":                                   # one point in every tile
        return [(b, min(8 * j + 3, h - 1), min(16 * i + 5, w - 1)) for b in range(B) for j in range(ty) for i in range(tx)]
    if name == "corners":                               # a single point in each corner of the map (sample 0; the others stay empty)
        return [(0, 0, 0), (0, 0, w - 1), (0, h - 1, 0), (0, h - 1, w - 1)]
    if name == "edges":
        # 1, 2 and 3 pixels outside the left edge of tiles (2, 2), (2, 5), (2, 8) of sample 0, and outside the top edge of tiles
        # (3, 2), (3, 5), (3, 8) of the last sample
        return [(0, 20, 32 - 1), (0, 20, 80 - 2), (0, 20, 128 - 3), (B - 1, 24 - 1, 40), (B - 1, 24 - 2, 88), (B - 1, 24 - 3, 136)]
    if name == "random":
        g = np.random.default_rng(11)
        return [(int(g.integers(B)), int(g.integers(h)), int(g.integers(w))) for _ in range(25)]
    raise KeyError(name)


SCENES = ("none", "all", "corners", "edges", "random")


@functools.lru_cache(maxsize=None)
def layers():
    """weights of the two convolutions (64 -> 128 with a residual; 128 -> 128 with bias and pool), real-valued, packed once"""
    from cmr_agent_amd.models import _pack
    g = torch.Generator().manual_seed(5)
    w0 = torch.randn(128, 64, 3, 3, generator=g) * 0.05
    w1 = torch.randn(128, 128, 3, 3, generator=g) * 0.04
    b1 = torch.randn(128, generator=g) * 0.1
    return _pack.winograd_u(w0).to(DEV).contiguous(), _pack.winograd_u(w1).to(DEV).contiguous(), b1.to(DEV)


@functools.lru_cache(maxsize=None)
def dense_empty(geom):
    """(res, x1 of the empty projection, x2 of it) by the DENSE entry point -- shared by the scenes of a geometry, never written to"""
    B, h, w = GEOMS[geom]
    g = torch.Generator().manual_seed(17)
    res = torch.randn(B, h, w, 128, generator=g).to(DEV)
    x1, x2 = dense(torch.zeros(B, h, w, 64, device=DEV), res)
    return res, x1, x2


def dense(x, res):
    u0, u1, b1 = layers()
    B, h, w, _ = x.shape
    y1, y2 = nans(B, h, w, 128), nans(B, h // 2, w // 2, 128)
    _raw("cmr_conv3x3_wino_nhwc_f32", _p(x), B, h, w, 64, _p(u0), None, _p(res), None, _p(y1), 128, SLOPE, 1, 0, 1, _stream())
    _raw("cmr_conv3x3_wino_nhwc_f32", _p(y1), B, h, w, 128, _p(u1), _p(b1), None, None, _p(y2), 128, SLOPE, 2, 0, 1, _stream())
    return y1, y2


def listed(x, res, lists, y10, y20):
    u0, u1, b1 = layers()
    B, h, w, _ = x.shape
    (o1, n1), (o2, n2) = lists
    y1, y2 = nans(B, h, w, 128), nans(B, h // 2, w // 2, 128)
    _raw("cmr_conv3x3_wino_list_nhwc_f32", _p(x), B, h, w, 64, _p(u0), None, _p(res), _p(y1), 128, SLOPE, 1, _p(o1), _p(n1), _p(y10), 0, 1, _stream())
    _raw("cmr_conv3x3_wino_list_nhwc_f32", _p(y1), B, h, w, 128, _p(u1), _p(b1), None, _p(y2), 128, SLOPE, 2, _p(o2), _p(n2), _p(y20), 0, 1, _stream())
    return y1, y2


def exact(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        raise AssertionError("%s: %d of %d elements differ (%d NaN = never written), first at %s" % (
            what, int(bad.sum()), got.numel(), int(torch.isnan(got).sum()), bad.nonzero()[0].tolist()))


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_list_convolutions_equal_the_dense_ones(geom, name):
    from cmr_agent_amd import ops
    B, h, w = GEOMS[geom]
    cells = scene(name, B, h, w)
    res, e1, e2 = dense_empty(geom)
    g = torch.Generator().manual_seed(23)
    x = torch.zeros(B, h, w, 64)
    for b, yy, xx in cells:
        x[b, yy, xx] = torch.randn(64, generator=g) + 0.1
    x = x.to(DEV)
    want1, want2 = dense(x, res)
    r1, r2 = S.reach_maps(cells, B, h, w)
    reach = torch.from_numpy(np.stack([r1, r2])).to(DEV)
    lists = ops.wino_tile_lists(reach, B, h, w, 128, 128)
    assert not reach.any()                                                    # consumed: cleared for the next observation
    for (o, n), r in zip(lists, (r1, r2)):
        wo, wn = S.tile_lists(r, 2)
        assert int(n) == wn and np.array_equal(o.cpu().numpy(), wo)
    n1, n2 = int(lists[0][1]), int(lists[1][1])
    ntiles = r1.size * 2
    if name == "none":
        assert n1 == 0 and n2 == 0
    elif name == "all":
        assert n1 == ntiles and n2 == ntiles
    elif name == "edges":
        t = lambda m, b, j, i: int(m[b, j, i])
        assert (t(r1, 0, 2, 2), t(r2, 0, 2, 2)) == (1, 1) and (t(r1, 0, 2, 5), t(r2, 0, 2, 5)) == (0, 1) and (t(r1, 0, 2, 8), t(r2, 0, 2, 8)) == (0, 0)
        assert (t(r1, B - 1, 3, 2), t(r2, B - 1, 3, 2)) == (1, 1) and (t(r1, B - 1, 3, 5), t(r2, B - 1, 3, 5)) == (0, 1) and (t(r1, B - 1, 3, 8), t(r2, B - 1, 3, 8)) == (0, 0)
    if name in ("corners", "edges"):
        assert 0 < n1 <= n2 < 256                                              # fewer live tiles than workgroups
    got1, got2 = listed(x, res, lists, e1, e2)
    exact(got1, want1, "conv 0 (%d of %d tiles live)" % (n1, ntiles))
    exact(got2, want2, "conv 1 + pool (%d of %d tiles live)" % (n2, ntiles))
    if name in ("none", "random"):
        # without a map to copy from, conv 0 evaluates its epilogue on a zero product: the same bits
        got1, _ = listed(x, res, lists, None, e2)
        exact(got1, want1, "conv 0, y0 path computed")


@pytest.mark.parametrize("geom", ["b2_40x160", "b2_44x152"])
def test_observation_marks_the_tiles_its_points_reach(geom):
    """cmr_observation_proj_reach_f32: marks from the same predicate and the same rounded cell as the scatter (compared with the
    restatement applied to the cells the kernel itself reports), points out of view or outside the predicted overlap mark nothing, and
    the maps accumulate until the list kernel clears them."""
    from cmr_agent_amd import ops
    B, h, w = GEOMS[geom]
    pix = [(0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0), (31.0, 20.0), (78.0, 20.0), (125.0, 20.0), (40.0, 23.0), (88.4, 21.6),
           (136.5, 20.5), (15.5, 7.5), (16.5, 8.5), (-0.4, 3.0), (w - 0.6, 3.0), (50.0, h - 0.6), (60.0, -0.2)]
    N = 32
    pc = torch.zeros(B, N, 4)
    pc[:, :, 2] = 1.0
    ov = torch.zeros(B, N, dtype=torch.uint8)
    for b in range(B):
        for k, (u, v) in enumerate(pix):
            z = 1.0 + 0.5 * ((k + b) % 3)
            pc[b, k] = torch.tensor([u * z, v * z, z, 0.0])
            ov[b, k] = 1
        pc[b, 20] = torch.tensor([70.0, 30.0, 1.0, 0.0])            # in view, not in the predicted overlap
        pc[b, 21] = torch.tensor([70.0, 30.0, -1.0, 0.0])           # behind the camera
        ov[b, 21] = 1
    feat = torch.randn(B * N, 64, generator=torch.Generator().manual_seed(2))
    K = torch.eye(3).repeat(B, 1, 1)
    pose = torch.eye(4).repeat(B, 1, 1)
    dev = lambda t: t.to(DEV).contiguous()
    proj = torch.zeros(B, h, w, 64, device=DEV)
    cnt = torch.zeros(B * h * w, device=DEV)
    cell = torch.full((B * N,), -1, dtype=torch.int32, device=DEV)
    st = torch.empty(B * N, 8, device=DEV)
    ty, tx = S.tile_grid(h, w)
    reach = torch.zeros(2, B, ty, tx, dtype=torch.uint8, device=DEV)
    args = (dev(pc.view(-1, 4)), dev(feat), dev(ov.view(-1)), dev(pose), dev(K), torch.zeros(B, 4, device=DEV), B, N, h, w, proj, cnt, cell, st)
    ops.observation_proj(*args, reach=reach)
    c = cell.cpu().numpy()
    cells = [(int(v) // (h * w), (int(v) % (h * w)) // w, int(v) % w) for v in c if v >= 0]
    assert len(cells) == B * (len(pix) - 4)                        # u = -0.4 rounds into the map but is not inside; v = -0.2 ... likewise
    assert set(cells) == set(S.occupied(proj.cpu().numpy()))       # the cells the scatter wrote
    r1, r2 = S.reach_maps(cells, B, h, w)
    assert np.array_equal(reach[0].cpu().numpy(), r1) and np.array_equal(reach[1].cpu().numpy(), r2)
    assert 0 < r1.sum() < r2.sum() < r2.size
    # a second observation from a shifted pose before anybody consumed the marks: the union
    pose2 = pose.clone()
    pose2[:, 0, 3] = 40.0
    ops.observation_proj(*(args[:3] + (dev(pose2),) + args[4:]), reach=reach)
    c2 = cell.cpu().numpy()
    cells2 = [(int(v) // (h * w), (int(v) % (h * w)) // w, int(v) % w) for v in c2 if v >= 0]
    q1, q2 = S.reach_maps(cells2, B, h, w)
    assert np.array_equal(reach[0].cpu().numpy(), r1 | q1) and np.array_equal(reach[1].cpu().numpy(), r2 | q2)
    # without maps the call is the one it was
    ops.observation_proj(*args)


def _env_data(B, h, w, N, seed):
    """an observation context without the geometric model: a cloud that projects into the middle third of the map"""
    g = torch.Generator().manual_seed(seed)
    pc = torch.stack([(torch.rand(B, N, generator=g) - 0.5) * 4, (torch.rand(B, N, generator=g) - 0.5) * 2, 8 + 12 * torch.rand(B, N, generator=g)], 1)
    img = (torch.rand(1, 64, 1, 1, generator=g) - 0.5) * 2 + 0.3 * (torch.rand(B, 64, h, w, generator=g) - 0.5)
    return dict(pc=pc, K=torch.tensor([[0.6 * w, 0, w / 2], [0, 0.6 * w, h / 2], [0, 0, 1.0]]).repeat(B, 1, 1),
                pc_overlap_pred=torch.rand(B, N, generator=g) > 0.4,
                pc_geo_feat=torch.nn.functional.normalize(torch.rand(B, 64, N, generator=g) - 0.5, dim=1),
                img_geo_feat=torch.nn.functional.normalize(img, dim=1))


def _registration(agent, cfg, data, steps, both):
    """`steps` agent steps from the identity pose.  both: every observation goes through the agent twice -- with the switch as it is and
    with it off -- so that the two forwards see the SAME projected map (two observations of one pose differ in the last bit: the
    scatter-mean adds with float atomics, see tests/test_e2e_gpu.py)."""
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
            was, CMRAgent.SPARSE_OBS = CMRAgent.SPARSE_OBS, False
            try:
                out += list(agent(s2, s3))
            finally:
                CMRAgent.SPARSE_OBS = was
        ar, at = agent.action_from_logits(r, t, deterministic=True)
        pose = env.step(ar, at, pose, cfg)
    return out + [pose], data['_cmr_obs'].agent_cache


@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("case", ["e2e_small", "map_40x160"])
def test_two_step_registration_with_the_switch_on_and_off(case, mode, monkeypatch):
    """Poses, logits and values of a two-step registration with SPARSE_OBS on and off: torch.equal.  e2e_small is the smallest
    configuration of the end-to-end tests (24 x 40 maps: below the persistent kernel's 200 tiles, so stage 0 runs dense either way --
    the switch must change nothing there); map_40x160 is the smallest on which the lists are used (asserted)."""
    import cases as C
    import parity_e2e
    from cmr_agent_amd.config import KittiConfiguration
    from cmr_agent_amd.models import CMRAgent
    if case == "e2e_small":
        cfg = C.e2e_config(case)
        geo, agent, _, _ = parity_e2e.build_models(cfg)
        data = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in C.e2e_batch(case).items()}
        with torch.no_grad():
            geo(data)
    else:
        cfg = KittiConfiguration(cropped_img_H=160, cropped_img_W=640, num_pt=1024, device="cpu", action_num=2)
        assert (cfg.image_H, cfg.image_W) == (40, 160)
        _, agent, _, _ = parity_e2e.build_models(cfg)
        data = {k: v.cuda() for k, v in _env_data(2, 40, 160, 1024, 3).items()}
    cfg.r_steps, cfg.t_steps = cfg.r_steps.cuda(), cfg.t_steps.cuda()
    assert CMRAgent.SPARSE_OBS and CMRAgent.sparse_obs()
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
    assert ("x1_0" in cache) == (case == "map_40x160")
    if case == "map_40x160":
        n1, n2 = (int(l[1]) for l in cache["lists"][1])
        assert 0 < n1 <= n2 < 200, (n1, n2)                                 # some tiles multiplied, some copied
    for k in range(2):
        on, off = out[6 * k:6 * k + 3], out[6 * k + 3:6 * k + 6]
        for a, b, what in zip(on, off, ("rotation logits", "translation logits", "value")):
            assert torch.equal(a, b), (k, what, float((a - b).abs().max()))
    # ... and a registration of its own with the switch off from the start: the same poses to the bit (logits to the atomics' rounding)
    monkeypatch.setattr(CMRAgent, "SPARSE_OBS", False)
    ref, cache = run(both=False)
    assert "x1_0" not in cache and cache.get("reach") is None
    assert torch.equal(out[-1], ref[-1])
    for k in range(2):
        for a, b in zip(out[6 * k:6 * k + 3], ref[3 * k:3 * k + 3]):
            assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max()))
