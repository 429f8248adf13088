"""Sparse observation (CMRAgent.SPARSE_OBS), outside the timed path of bench.py, on the benchmark's own batch (configs[1], fp32):

  live     one eager registration as bench.py runs it; after every agent step the live share of the two stage-0 convolutions is read
           from the device (nlive / tiles), per step and per sample, and -- with CMRAgent.SPARSE_OBS_STAGES = 2 where stage 1 is served --
           the live / copy / rest shares of all four lists ("lists": conv0 .. conv3; copy = skipped tiles that are copied from the
           image-only map, rest = tiles that are not written at all: only the first convolution of a stage has any)
  worst    a registration started at the ground-truth pose with the overlap mask all ones and held there in all action_num steps (the
           actions are applied to a scratch pose), as a captured agent loop (observation + agent + pose step) replayed with the switch
           off, with it on, and with it on and every tile MARKED after each observation (one fill launch per step more: every tile
           live whatever the cloud covers), the last two with one and with two stages on lists, alternating: the cost of the lists when
           they save little and when they save nothing (the image-only maps once + list launches that multiply everything)

    python tools/sparse_obs_probe.py [--reps 20]          -> one JSON line"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from cmr_agent_amd.dataset.sampling import hip_fps, hip_nearest  # noqa: E402
from cmr_agent_amd.config import KittiConfiguration  # noqa: E402
from cmr_agent_amd.environment import environment as env  # noqa: E402
from cmr_agent_amd.models import CMRAgent  # noqa: E402
from cmr_agent_amd.utils import synthetic  # noqa: E402


def live_shares(geo, agent, cfg, batch):
    data = dict(batch)
    geo(data)
    pose, target = env.init(data)
    env.to_disentangled(target, data['pc'], data=data)
    B = data['pc'].shape[0]
    steps = []
    for _ in range(cfg.action_num):
        s2, s3 = env.observation_from_a_pose(data, pose, materialize_state_2d=False)
        r, t, v = agent(s2, s3)
        width, lists = data['_cmr_obs'].agent_cache["lists"]
        row = {}
        for name, (order, nlive) in zip(("conv0", "conv1"), lists):
            n, nco = int(nlive), width // 64
            per = order.numel() // B
            row[name] = round(n / order.numel(), 4)
            row[name + "_per_sample"] = [round(float(((order[:n] // per) == b).sum()) / per, 3) for b in range(B)]
        row["lists"] = list_shares(data['_cmr_obs'].agent_cache.get("lists_staged"))
        steps.append(row)
        ar, at = agent.action_from_logits(r, t, deterministic=True)
        pose = env.step(ar, at, pose, cfg)
    return steps


def list_shares(l4):
    """the four lists of ops.wino_tile_lists_staged -> [live, copy, rest] share of each (None where stage 1 is not on lists)"""
    if l4 is None:
        return None
    out = {}
    for k, l in enumerate(l4):
        n, live = l[0].numel(), int(l[1])
        end = int(l[2]) if len(l) == 3 else n
        out["conv%d" % k] = [round(live / n, 4), round((end - live) / n, 4), round((n - end) / n, 4)]
    return out


def agent_loop_graph(agent, cfg, data, start, hold, mark_all=False):
    """the action_num agent steps from pose `start` as one hipGraph (a registration of its own: new observation context); hold: every
    step observes `start` (the pose update runs on a copy); mark_all: every tile is marked live after each observation"""
    def loop():
        d = {k: v for k, v in data.items() if k != '_cmr_obs'}
        pose = start.clone()
        for _ in range(cfg.action_num):
            s2, s3 = env.observation_from_a_pose(d, pose, materialize_state_2d=False)
            if mark_all and d['_cmr_obs'].reach is not None:
                d['_cmr_obs'].reach.fill_(1)
            r, t, v = agent(s2, s3)
            ar, at = agent.action_from_logits(r, t, deterministic=True)
            moved = env.step(ar, at, pose.clone() if hold else pose, cfg)
            pose = pose if hold else moved
        return moved, d
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loop()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pose, d = loop()
    return g, pose, d


def timed(g, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS["c1"]
    cfg = KittiConfiguration(cropped_img_H=w["H"], cropped_img_W=w["W"], num_pt=w["N"], device=dev, action_num=w["steps"])
    geo, agent, _ = bench.load_models(cfg, dev)
    batch = synthetic.make_batch(w["B"], w["N"], w["H"], w["W"], w["M"], hip_fps(dev), hip_nearest(dev), seed=cfg.seed, n_circle=16, device=dev)
    out = {}
    truth = batch['P'].clone()          # (to_disentangled rewrites the pose it is given in place)
    with torch.no_grad():
        CMRAgent.SPARSE_OBS = True
        out["stages"] = CMRAgent.SPARSE_OBS_STAGES
        out["live_share_per_agent_step"] = live_shares(geo, agent, cfg, batch)
        # worst case: ground-truth start, every point selected
        data = dict(batch, P=truth)
        geo(data)
        _, target = env.init(data)
        env.to_disentangled(target, data['pc'], data=data)
        data['pc_overlap_pred'] = torch.ones_like(data['pc_overlap_pred'])
        graphs = {}
        for name, on, stages, mark_all in (("dense", False, 1, False), ("lists_at_truth", True, 1, False), ("lists_all_live", True, 1, True),
                                           ("lists2_at_truth", True, 2, False), ("lists2_all_live", True, 2, True)):
            CMRAgent.SPARSE_OBS, CMRAgent.SPARSE_OBS_STAGES = on, stages
            graphs[name] = agent_loop_graph(agent, cfg, data, target, hold=True, mark_all=mark_all)
        ms = {name: [] for name in graphs}
        for _ in range(3):
            for name in graphs:
                ms[name].append(round(timed(graphs[name][0], args.reps), 4))
        out["worst_case_agent_loop_ms"] = ms
        for name in ("lists_at_truth", "lists_all_live", "lists2_at_truth", "lists2_all_live"):
            assert torch.equal(graphs["dense"][1], graphs[name][1])          # the pose after the last step's actions, from the replays
            cache = graphs[name][2]['_cmr_obs'].agent_cache
            out[name + "_live_share"] = [round(int(n) / o.numel(), 4) for o, n in cache["lists"][1]]
            if cache.get("lists_staged") is not None:
                out[name + "_lists"] = list_shares(cache["lists_staged"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
