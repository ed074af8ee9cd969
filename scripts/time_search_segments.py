"""Times merged searches (SampledMCTS.batch_search_many: several searches on one recorded loop, per-segment
tree seeds) against the separate searches they replace, at the BASELINE reanalyze batch: SMAC 3m (3 agents,
9 actions), 256 trajectories x (5 + 1) unroll steps = 1,536 rows, 50 simulations, K = 1, MuZeroShapedNet
under autocast.

reanalyze   consume.reanalyze_value_targets followed by consume.reanalyze_policy_targets (today's two
            calls: N + 1 searches) against consume.reanalyze_batch_targets (the value search and the
            agent-0 policy search as one search of 3,072 roots: N searches);
agent k     agent k's searches of two batches, two batch_search_device calls against one
            batch_search_many_device with the draws made beforehand (draw_search), for every k.

All legs run in one process, interleaved round by round, after warm-up calls that run eagerly, record the
graphs and replay them once.  Every call ends with a device synchronisation; per leg the median and the
range of the rounds' medians of the wall-clock time.  Prints one JSON line.

    python scripts/time_search_segments.py [--rounds 5] [--reps 5] [--no-fused]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mazero_amd import consume  # noqa: E402
from mazero_amd.mcts_sampled import _LOOPS, SampledMCTS  # noqa: E402
from mazero_amd.nets import SearchConfig, make_net, make_root_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trajectories", type=int, default=256)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--no-fused", action="store_true", help="the model's own inverse transforms")
    a = ap.parse_args()
    N, A, U, TD, disc = 3, 9, 5, 5, 0.997
    G = a.trajectories
    B = G * (U + 1)
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=a.sims, sampled_action_times=1)
    net = make_net(N, A, seed=0, device=dev)
    batches = [make_root_batch(net, B, 64, seed=10 + i, device=dev, legal_zero_frac=0.2) for i in range(2)]
    rng = np.random.default_rng(0)
    tl = rng.integers(20, 120, size=G)
    tv = dict(rewards=[rng.standard_normal(t) for t in tl], pos=np.array([rng.integers(0, t) for t in tl]),
              traj_len=tl, td_steps=rng.integers(1, TD + 1, size=G), discount=disc, num_unroll_steps=U, td_max=TD)
    mask = rng.integers(0, 2, size=B)
    kw = dict(fused_transforms=not a.no_fused)
    drv = {name: SampledMCTS(cfg, np.random.RandomState(0), **kw) for name in ("two_calls", "batch", "separate", "merged")}
    (vout, vlegal), (pout, plegal) = batches

    def two_calls():
        consume.reanalyze_value_targets(drv["two_calls"], net, vout, vlegal, device=dev, **tv)
        consume.reanalyze_policy_targets(drv["two_calls"], net, pout, plegal, mask, dev)

    def batch():
        consume.reanalyze_batch_targets(drv["batch"], net, vout, vlegal, pout, plegal, mask, device=dev, **tv)

    factors = [np.random.RandomState(3 + i).randint(0, A, (B, N)).astype(np.int32) for i in range(2)]

    def separate(k):
        for (out, legal), f in zip(batches, factors):
            drv["separate"].batch_search_device(net, out, k, f if k else None, N, legal, dev, add_noise=True)

    def merged(k):
        d = drv["merged"]
        draws = [d.draw_search(B) for _ in batches]
        d.batch_search_many_device(net, [b[0] for b in batches], k, factors if k else None, N, [b[1] for b in batches],
                                   dev, add_noise=True, draws=draws)

    legs = {"reanalyze_two_calls": two_calls, "reanalyze_batch_targets": batch}
    for k in range(N):
        legs[f"agent{k}_separate"] = lambda k=k: separate(k)
        legs[f"agent{k}_merged"] = lambda k=k: merged(k)
    for fn in legs.values():  # eager, recorded, replayed
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    med = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, fn in legs.items():
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            med[name].append(float(np.median(ts)))
    res = dict(rows=B, agents=N, actions=A, sims=a.sims, rounds=a.rounds, reps=a.reps, fused_transforms=not a.no_fused,
               device=torch.cuda.get_device_name(0),
               graph_nodes=sorted({(k[8][0], k[4], v.graph_nodes[0]) for k, v in _LOOPS.items() if v.graph_nodes}),
               ms={name: dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3),
                              rounds=[round(x, 3) for x in v]) for name, v in med.items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
