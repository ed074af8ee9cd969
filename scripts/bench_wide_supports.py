"""Full search loop with the reference's default supports [-300, 300] (601 elements): ms per
environment step of the default loop, of `fused_transforms=True` (such supports keep torch's softmax,
multiply and sum; only _inv_h is fused) and of `fused_transforms=True, wide_supports=True` (the whole
chain in one mz_inverse_transform_wide launch).  SMAC 3m, 3 agents x 256 roots x 50 simulations,
K = 1, MuZeroShapedNet under autocast, the graph-replayed loop as in bench_search.py.  The legs are
interleaved, --runs times each, in one process; one JSON line (profiles/wide_supports/full_loop.json)
with every run, and whether one environment step's actions and visit counts are equal in all legs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mazero_amd  # noqa: E402,F401
import torch  # noqa: E402

from mazero_amd.mcts_sampled import SampledMCTS  # noqa: E402
from mazero_amd.nets import MuZeroShapedNet, SearchConfig, make_root_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--roots", type=int, default=256)
ap.add_argument("--sims", type=int, default=50)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

N, A, K, SUPPORT = 3, 9, 1, (-300, 300)
B, S = args.roots, args.sims
dev = torch.device("cuda", 0)
cfg = SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=K, value_support=SUPPORT,
                   reward_support=SUPPORT)
torch.manual_seed(0)
net = MuZeroShapedNet(N, 64, A, support=SUPPORT).to(dev).eval()
roots = [make_root_batch(net, B, 64, seed=10 + i, device=dev, legal_zero_frac=0.2) for i in range(3)]
LEGS = {"device": {}, "device_fused_transforms": {"fused_transforms": True},
        "device_wide_supports": {"fused_transforms": True, "wide_supports": True}}


def env_step(mcts, i):
    out, legal = roots[i % len(roots)]
    acts = np.zeros((B, N), np.int32)
    res = []
    for agent in range(N):  # selfplay_worker.py:196-211
        factor = acts[:, :agent].copy() if agent else None
        r = mcts.batch_search(net, out, agent, factor, N, legal, device=dev, add_noise=True)
        acts[:, agent] = [int(a[np.argmax(v), 0]) if len(a) else 0
                          for a, v in zip(r.sampled_actions, r.sampled_visit_count)]
        res.append(r)
    return res


def timed(mcts, steps, warm):
    for i in range(warm):
        env_step(mcts, i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        env_step(mcts, i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


drivers = {k: SampledMCTS(cfg, np.random.RandomState(0), use_graph=True, **kw) for k, kw in LEGS.items()}
ms = {k: [] for k in LEGS}
for run in range(args.runs):
    for k, drv in drivers.items():
        ms[k].append(round(timed(drv, args.steps, 2) * 1e3, 3))

steps = {k: env_step(SampledMCTS(cfg, np.random.RandomState(5), use_graph=True, **kw), 0) for k, kw in LEGS.items()}


def same(a, b):
    return all(np.array_equal(x, y) for ra, rb in zip(a, b)
               for fa, fb in ((ra.sampled_actions, rb.sampled_actions), (ra.sampled_visit_count, rb.sampled_visit_count))
               for x, y in zip(fa, fb))


line = {"metric": f"ms per environment step, SMAC 3m ({N} agents x {B} roots x {S} sims, K={K}), supports {list(SUPPORT)}",
        "steps": args.steps, "runs": args.runs}
for k in LEGS:
    line[k] = {"ms_per_step": ms[k], "mean": round(sum(ms[k]) / len(ms[k]), 3),
               "spread": round(max(ms[k]) - min(ms[k]), 3)}
line["actions_equal_all_legs"] = bool(same(steps["device"], steps["device_fused_transforms"]) and
                                      same(steps["device"], steps["device_wide_supports"]))
print(json.dumps(line), flush=True)
