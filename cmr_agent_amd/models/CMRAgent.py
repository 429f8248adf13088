"""Stage-2 actor-critic policy.  API / state_dict mirror of the reference's models/CMRAgent.py
(:17-144).  2-D branch: 8 x conv3x3(128->128) (+BN on the odd ones) with LeakyReLU(0.01), three
2x2 average pools and a global pool, two 1x1 convs; 3-D branch: 4 x ConvBNReLURes1D with a global
max-pool whose result is broadcast-concatenated to every point (never materialised: it enters the
next layer as the second GEMM source); heads: three small MLPs on the 256-d state."""
import torch
import torch.nn as nn

from .. import ops
from ..utils.streams import fork_join
from . import _pack
from ._pack import Planned
from .ImageResNet import to_nhwc
from .PointNN import ConvBNReLURes1D

SLOPE = 0.01          # nn.LeakyReLU default (CMRAgent.py:36)


def _mlp(sizes):
    layers = []
    for i in range(len(sizes) - 1):
        layers.append(nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            layers.append(nn.LeakyReLU(inplace=True))
    return nn.Sequential(*layers)


class CMRAgent(Planned):
    def __init__(self, config):
        super().__init__()
        self.config = config
        f = config.embed_dim
        self.state_3d_embed = nn.ModuleList([ConvBNReLURes1D(5, f), ConvBNReLURes1D(2 * f, f),
                                             ConvBNReLURes1D(2 * f, f), ConvBNReLURes1D(2 * f, 2 * f)])
        H, W = config.image_H // 8, config.image_W // 8
        c = 2 * f
        conv = lambda: nn.Conv2d(c, c, kernel_size=(3, 3), padding=(1, 1), stride=1)
        seq = []
        for stage in range(4):
            seq += [conv(), nn.BatchNorm2d(c), nn.LeakyReLU(inplace=True), conv(), nn.LeakyReLU(inplace=True),
                    nn.AvgPool2d((2, 2), stride=(2, 2)) if stage < 3 else nn.AvgPool2d((H, W), stride=1)]
        seq += [nn.Conv2d(c, c, kernel_size=(1, 1), padding=(0, 0), stride=1), nn.LeakyReLU(inplace=True),
                nn.Conv2d(c, c, kernel_size=(1, 1), padding=(0, 0), stride=1)]
        self.state_2d_embed = nn.Sequential(*seq)
        self.degree_r, self.degree_t = (3, 3) if config.is_6_DoF else (1, 2)
        self.policy_r = _mlp([4 * f, 4 * f, 4 * f, self.degree_r * config.num_steps])
        self.policy_t = _mlp([4 * f, 4 * f, 4 * f, self.degree_t * config.num_steps])
        self.value = _mlp([4 * f, f, f, 1])

    def _build_plan(self):
        e = self.state_2d_embed
        p = {"convs": []}
        for stage in range(4):
            b = stage * 6
            p["convs"].append((_pack.conv9(e[b], e[b + 1]), _pack.conv9(e[b + 3])))
        # conv(W, [img | proj]) = conv(W[:, :f], img) + conv(W[:, f:], proj): the image half of the observation
        # does not change over the action_num steps of one registration
        f = self.config.embed_dim
        p["conv0_img"] = _pack.conv9(e[0], e[1], cin_slice=slice(0, f))
        p["conv0_proj"] = _pack.conv9(e[0], e[1], cin_slice=slice(f, 2 * f))
        p["c24"], p["c26"] = _pack.lin(e[24]), _pack.lin(e[26])
        tr = lambda wb: (wb[0].t().contiguous(), wb[1])          # W^T [in, out4]: operand of cmr_agent_heads_t_f32
        p["c24t"], p["c26t"] = tr(p["c24"]), tr(p["c26"])
        for name in ("policy_r", "policy_t", "value"):
            m = getattr(self, name)
            p[name] = [_pack.lin(m[0]), _pack.lin(m[2]), _pack.lin(m[4])]
            p[name + "_t"] = [tr(x) for x in p[name]]
        # the transposed-weight tail serves hidden widths that are multiples of 16 up to 256 and a 128-wide 2-D embedding (embed_dim 64)
        p["tail_t"] = 2 * self.config.embed_dim == 128 and all(p[n][0][0].shape[0] % 16 == 0 and p[n][1][0].shape[0] % 16 == 0 and p[n][0][0].shape[0] <= 256
                                       and p[n][1][0].shape[0] <= 256 and p[n][0][0].shape[1] == 256 for n in ("policy_r", "policy_t", "value"))
        # 3-D branch, layers 1..3: the input is cat([feat, broadcast(global max)]) (CMRAgent.py:95-99).  Split every
        # weight that multiplies it into the streamed half (feat) and the per-sample half (max), which becomes a
        # per-batch bias computed by a skinny GEMM each step.
        f = self.config.embed_dim
        p["s3d"] = []
        for i in (1, 2, 3):
            q = self.state_3d_embed[i].plan()
            w1, b1 = q["l1"]
            ent = dict(w1a=w1[:, :f].contiguous(), w1b=w1[:, f:].contiguous(), b1=b1, w2=q["l2"][0])
            if q["sc"] is not None:
                ent.update(wsca=q["sc"][0][:, :f].contiguous(), wscb=q["sc"][0][:, f:].contiguous(), b2=q["b2f"])
            else:   # identity shortcut: the max half of the residual is per-sample too -> selection matrix [0; I]
                e = torch.zeros((2 * f, f), dtype=w1.dtype, device=w1.device)
                e[f:, :] = torch.eye(f, dtype=w1.dtype, device=w1.device)
                ent.update(wsca=None, wscb=e, b2=q["b2f"])
            p["s3d"].append(ent)
        return p

    def _embed_3d(self, state3d_rows, B, N):
        """-> [B, 2f] global max of the last block, one fused kernel per ConvBNReLURes1D block."""
        p = self.plan()
        layers = self.state_3d_embed
        q0 = layers[0].plan()
        r = ops.cbr_block(state3d_rows, q0["l1"][0], q0["l1"][1], q0["l2"][0], q0["b2f"], q0["sc"][0], 0.2,
                          rows_per_batch=N, want_colmax="partials")
        if r is None:
            return None
        feat, part = r
        for i, ent in enumerate(p["s3d"]):
            # the block kernel leaves per-tile maxima; ONE launch finishes the max over the points and folds the broadcast half of the next
            # block's input into its per-sample biases (three launches -- column max + two skinny GEMMs -- on the serial chain before round 6)
            glue = ops.colmax_bias2(part, B, N // 32, ent["w1b"], ent["b1"], ent["wscb"], ent["b2"])
            if glue is not None:
                b1b, b2b = glue[0], glue[1]
            else:
                g = ops.colmax_partials(part, B, N // 32)
                b1b = ops.linear(g, ent["w1b"], ent["b1"])               # [B, 2f] per-sample hidden bias
                b2b = ops.linear(g, ent["wscb"], ent["b2"])              # [B, co] per-sample output bias
            last = i == 2
            r = ops.cbr_block(feat, ent["w1a"], b1b, ent["w2"], b2b, ent["wsca"], 0.2, rows_per_batch=N,
                              want_y=not last, want_colmax="partials")
            if r is None:
                return None
            feat, part = r
        return ops.colmax_partials(part, B, N // 32)

    FUSED_TAIL = True
    TAIL_T = True           # ... on the transposed-weight kernel (cmr_agent_heads_t_f32); False: the row-per-wave kernel

    # Stage 0 of the 2-D branch multiplies only the 8x16 tiles that a projected point can reach (1 pixel for conv 0, 2 for conv 1, marked
    # by the observation kernel); every other tile is, bit for bit, that of the same two convolutions on an empty projection, computed once
    # per registration next to the image half of conv 0 ("Sparse observation").  fp32 evaluation only: the bf16 chain and
    # the training engine run the dense calls.  False: every call is the dense one.
    SPARSE_OBS = True
    # 2: stage 1 (the two convolutions on the pooled map) runs on lists too, where it has the tiles for it: a tile of its first / second
    # convolution no point comes within 4 / 6 cells of is that of the empty projection as well, and the first convolution of either stage
    # stops copying the tiles its successor does not read (ops.wino_tile_lists_staged).  1: stage 0 only, every skipped tile copied.
    SPARSE_OBS_STAGES = 2

    @classmethod
    def sparse_obs(cls):
        return cls.SPARSE_OBS and ops.WINOGRAD and not ops.CONV_BF16

    def _tile_lists(self, cache, proj, c, u0, u1):
        """-> ((order, nlive) of conv 0, of conv 1) of stage 0 for the observation `proj` belongs to, or None where stage 0 runs dense.
        cache["lists_staged"]: the four lists of ops.wino_tile_lists_staged where stage 1 is served too, else None."""
        mark = cache.get("reach")
        if mark is None or not self.sparse_obs() or self.training or mark[1] is not proj or u0 is None or u1 is None:
            return None
        B, h, w, cin = proj.shape
        if h % 2 or w % 2 or not (ops.wino_list_served(B, h, w, cin, c) and ops.wino_list_served(B, h, w, c, c)):
            return None
        if cache.get("lists_of") != mark[2]:                  # once per observation: the list kernel clears the marks
            nt, nt1 = ops.reach_tiles(B, h, w)
            staged = (self.SPARSE_OBS_STAGES >= 2 and mark[0].numel() == 2 * nt + 2 * nt1 and h % 4 == 0 and w % 4 == 0
                      and ops.wino_list_served(B, h // 2, w // 2, c, c))
            if staged:
                l4 = ops.wino_tile_lists_staged(mark[0], B, h, w, c, c)
                cache["lists"] = (c, (l4[0][:2], l4[1]))
                cache["lists_staged"] = l4
            else:
                cache["lists"] = (c, ops.wino_tile_lists(mark[0].view(-1)[:2 * nt], B, h, w, c, c))
                cache["lists_staged"] = None
            cache["lists_of"] = mark[2]
        width, lists = cache["lists"]
        return lists if width == c else None

    def _embed_2d(self, state2d, B, split):
        p = self.plan()
        c = 2 * self.config.embed_dim
        x = state2d
        staged = None                                        # stage 1 on lists: its two lists, from stage 0
        for stage, ((wa, ba, ua), (wb, bb, ub)) in enumerate(p["convs"]):
            if stage == 0 and split is not None:
                # split = (image half, projected half, per-registration cache): the cache dict belongs to the
                # observation context of ONE registration (environment._ObsContext), so the image half of conv 0
                # (+ bias) is computed on the first step of that registration and can never be confused with
                # another batch whose buffer happens to land at the same address
                img_src, proj, cache = split
                tag = (id(self), id(p))
                if cache.get("tag") != tag:
                    wi, bi, ui = p["conv0_img"]
                    cache["val"] = ops.conv3x3(img_src, wi, bi, c, 1, 1.0, u=ui)
                    cache["tag"] = tag
                wp, _, up = p["conv0_proj"]
                lists = self._tile_lists(cache, proj, c, up, ub)
                if lists is not None:
                    # stage 0 on the tiles the projected points can reach; the others are those of the image-only maps
                    if cache.get("tag0") != tag:
                        none = torch.zeros((1,), dtype=torch.int32, device=proj.device)         # no live tile: every tile from the y0 path
                        cache["x1_0"] = ops.conv3x3_wino_list(proj, up, None, c, SLOPE, lists[0][0], none, None, res=cache["val"])
                        cache["x2_0"] = ops.conv3x3(cache["x1_0"], wb, bb, c, 1, SLOPE, pool=2, u=ub)
                        cache["tag0"] = tag
                    (o1, n1), (o2, n2) = lists
                    l4 = cache.get("lists_staged") if self.SPARSE_OBS_STAGES >= 2 else None
                    if l4 is not None and p["convs"][1][0][2] is not None and p["convs"][1][1][2] is not None:
                        if cache.get("tag1") != tag:           # the image-only maps of stage 1, next to those of stage 0
                            (w2, b2, u2), (w3, b3, u3) = p["convs"][1]
                            cache["x3_0"] = ops.conv3x3(cache["x2_0"], w2, b2, c, 1, SLOPE, u=u2)
                            cache["x4_0"] = ops.conv3x3(cache["x3_0"], w3, b3, c, 1, SLOPE, pool=2, u=u3)
                            cache["tag1"] = tag
                        staged = (l4[2], l4[3], cache["x3_0"], cache["x4_0"])
                    # x1 is read by the next launch alone, on its live tiles and their halo: with the staged lists the rest is not written
                    x = ops.conv3x3_wino_list(proj, up, None, c, SLOPE, o1, n1, cache["x1_0"], res=cache["val"],
                                              nend=l4[0][2] if l4 is not None else None)
                    x = ops.conv3x3_wino_list(x, ub, bb, c, SLOPE, o2, n2, cache["x2_0"], pool=2)
                    continue
                x = ops.conv3x3(proj, wp, None, c, 1, SLOPE, res=cache["val"], u=up, out_bf16=True)
            elif stage == 1 and staged is not None:
                (o3, n3, e3), (o4, n4), x3_0, x4_0 = staged
                x = ops.conv3x3_wino_list(x, ua, ba, c, SLOPE, o3, n3, x3_0, nend=e3)
                x = ops.conv3x3_wino_list(x, ub, bb, c, SLOPE, o4, n4, x4_0, pool=2)
                continue
            else:
                x = ops.conv3x3(x, wa, ba, c, 1, SLOPE, u=ua, out_bf16=True)
            # every map of the chain only feeds the next convolution (bf16 mode: stored as bf16); the last one goes to the heads in fp32
            x = ops.conv3x3(x, wb, bb, c, 1, SLOPE, pool=2 if stage < 3 else 1, u=ub, out_bf16=stage < 3)     # AvgPool2d(2,2) in the epilogue
            if stage == 3:
                kh, kw = self.config.image_H // 8, self.config.image_W // 8
                if (x.shape[1], x.shape[2]) != (kh, kw):
                    raise ValueError("state_2d is %dx%d at the global pool, config says %dx%d" % (x.shape[1], x.shape[2], kh, kw))
        return x                                             # [B, kh, kw, c]: global pool + 1x1 convs live in _tail

    def _embed_3d_any(self, state3d_rows, B, N):
        e3d = self._embed_3d(state3d_rows, B, N)
        if e3d is None:                                      # shapes the fused block kernel is not built for
            layers = self.state_3d_embed
            feat = layers[0].rows(state3d_rows)
            for i in (1, 2, 3):
                g = ops.colmax(feat, B, N)                   # torch.max over points, broadcast back (:95-99)
                feat = layers[i].rows(feat, x2=g, div2=N)
            e3d = ops.colmax(feat, B, N)
        return e3d

    # ------------------------------------------------------------------------------------------
    def forward_cl(self, state2d, state3d_rows, B, N, split=None):
        """state2d NHWC [B,h,w,128]; state3d rows [B*N,8] = (x,y,z,overlap,in_cam,0,0,0).
        split = (img_geo_feat NHWC [B,h,w,64], projected half NHWC [B,h,w,64], cache dict of this registration) when
        the observation comes from cmr_agent_amd.environment: the two halves of state2d as separate tensors."""
        self._require_eval()
        # the 3-D branch (4 fused blocks on B*N points) runs on a side stream underneath the 2-D convolutions
        e3d, e2d = fork_join(lambda: self._embed_3d_any(state3d_rows, B, N), lambda: self._embed_2d(state2d, B, split), tag="agent")
        p = self.plan()
        _, kh, kw, c = e2d.shape
        xr = e2d.view(B * kh * kw, c)
        heads = [p[name] for name in ("policy_r", "policy_t", "value")]
        if self.FUSED_TAIL and e3d.is_contiguous():
            # AvgPool2d((H, W)) + the two 1x1 convs + the three heads: one launch (13 otherwise)
            # ... and the deterministic actions (argmax per group of num_steps logits): attached to the logits, picked up by
            # action_from_logits(deterministic=True) instead of two more launches per step
            if self.TAIL_T and p["tail_t"]:
                out, acts = ops.agent_heads_t(xr, B, kh * kw, p["c24t"], p["c26t"], e3d, [p[name + "_t"] for name in ("policy_r", "policy_t", "value")],
                                              SLOPE, actions=(self.config.num_steps, self.degree_r, self.degree_t))
            else:
                out, acts = ops.agent_heads(xr, B, kh * kw, p["c24"], p["c26"], e3d, heads, SLOPE,
                                            actions=(self.config.num_steps, self.degree_r, self.degree_t))
        else:
            acts = None
            x = ops.colmean(xr, B, kh * kw)                  # AvgPool2d((H, W)) = per-sample channel mean
            e2 = ops.linear(ops.linear(x.view(B, c), *p["c24"], act=ops.ACT_LRELU, act_param=SLOPE), *p["c26"])
            out = []
            for l0, l1, l2 in heads:
                hcur = ops.linear(e2, *l0, x2=e3d, act=ops.ACT_LRELU, act_param=SLOPE)   # cat([embed_2d, embed_3d])
                hcur = ops.linear(hcur, *l1, act=ops.ACT_LRELU, act_param=SLOPE)
                out.append(ops.linear(hcur, *l2))
        S = self.config.num_steps          # head widths are padded to a multiple of 4: slice, then split
        r = out[0][:, :self.degree_r * S].view(B, self.degree_r, S)
        t = out[1][:, :self.degree_t * S].view(B, self.degree_t, S)
        if acts is not None:
            r._cmr_argmax, t._cmr_argmax = (acts[0], r._version), (acts[1], t._version)
        return r, t, out[2][:, :1].view(B, 1, 1)

    def forward(self, state_2d, state_3d):
        """state_2d [B,128,h,w], state_3d [B,5,N] (reference layout; the views produced by
        cmr_agent_amd.environment are consumed without a copy)."""
        B, _, N = state_3d.shape
        split = getattr(state_2d, "_cmr_split", None)
        if state_2d.device.type == "meta":                  # environment.observation_from_a_pose(materialize_state_2d=False)
            if split is None:
                raise ValueError("CMRAgent.forward: a shape-only state_2d must carry its two halves (_cmr_split)")
            s2 = None
        else:
            s2 = to_nhwc(state_2d)
        if state_3d.stride(1) == 1 and state_3d.stride(2) == 8 and state_3d.stride(0) == 8 * N:
            s3 = torch.as_strided(state_3d, (B * N, 8), (8, 1))            # view of the env's [B*N,8] rows
        else:
            s3 = ops.planar_to_rows(state_3d.contiguous(), 8)
        if self.training:
            return self._forward_train(s2, s3, B, N, split)
        return self.forward_cl(s2, s3, B, N, split)

    # ---- train mode (Train_Agent.py:256-305): the network is ONE autograd node over the HIP kernels (train/bridge.py); the caller composes
    # the loss from the returned logits / value in torch and steps a torch optimizer
    def hip_engine(self):
        br = getattr(self, "_hip_bridge", None)
        if br is not None:
            try:
                br.bucket.check_attached()
            except RuntimeError:                                 # the module was moved (.to / .cuda) since: rebuild on the new storage
                br = self._hip_bridge = None
        if br is None:
            from ..train.bridge import AgentBridge
            self._hip_bridge = None
            br = AgentBridge(self, self.config)
            self._hip_bridge = br
        return br

    def _forward_train(self, s2, s3, B, N, split):
        if s2 is None:                                       # shape-only state_2d: its two halves, concatenated once (training keeps the input)
            s2 = torch.cat([split[0], split[1]], dim=3)
        return self.hip_engine().forward(self, s2, s3, B, N)

    @staticmethod
    def action_from_logits(r_logits, t_logits, deterministic=False):
        """CMRAgent.py:118-127.  deterministic: argmax (of the Categorical probs = of the logits)."""
        if deterministic:
            # logits that come straight from forward() carry their argmax (same launch); anything else (modified in place,
            # sliced, user-made) goes through the argmax kernel
            def pick(x):
                a = getattr(x, "_cmr_argmax", None)
                return a[0] if a is not None and a[1] == x._version else ops.argmax_rows(x)
            return pick(r_logits), pick(t_logits)
        from torch.distributions import Categorical
        return Categorical(logits=r_logits).sample(), Categorical(logits=t_logits).sample()

    @staticmethod
    def action_logprob_and_entropy(r_logits, t_logits, action_r, action_t):
        """CMRAgent.py:129-144 (training-side bookkeeping; plain torch)."""
        from torch.distributions import Categorical
        dr, dt = Categorical(logits=r_logits), Categorical(logits=t_logits)
        return (torch.cat([dr.log_prob(action_r), dt.log_prob(action_t)], dim=1),
                torch.cat([dr.entropy(), dt.entropy()], dim=1))
