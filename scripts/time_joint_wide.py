"""Cost of the wide joint search (SampledMCTS(..., wide_joint=True).batch_search_joint): ms per
environment step, bench_search.py's `device_joint` leg at shapes past the narrow joint bounds.

    python scripts/time_joint_wide.py [--roots 256] [--sims 50] [--steps 5]

One JSON line per shape (N, A, K): (3, 100, 5), wide action spaces, and (3, 9, 100), more than 64 sampled
joint actions; and, for scale, the narrow joint search (3, 9, 5) of the same process.  A cost, not an A/B:
the shapes are different searches."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=256)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()

    import torch

    from mazero_amd.mcts_sampled import _LOOPS, SampledMCTS, release
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch

    B, S = args.roots, args.sims
    dev = torch.device("cuda", 0)
    for N, A, K, wide in ((3, 9, 5, False), (3, 100, 5, True), (3, 9, 100, True)):
        cfg = SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=K)
        net = make_net(N, A, seed=0, device=dev)
        roots = [make_root_batch(net, B, 64, seed=10 + i, device=dev, legal_zero_frac=0.2) for i in range(3)]
        mcts = SampledMCTS(cfg, np.random.RandomState(0), use_graph=True, wide_joint=wide)

        def step(i):
            out, legal = roots[i % len(roots)]
            return mcts.batch_search_joint(net, out, legal, dev, True, 1.0)

        for i in range(2):  # the eager run and the capture
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            res = step(i)
        torch.cuda.synchronize()
        t = (time.perf_counter() - t0) / args.steps
        loop = [v for v in _LOOPS.values() if v.joint_mode and v.model_ref() is net][-1]
        print(json.dumps({"agents": N, "actions": A, "sampled_times": K, "roots": B, "sims": S, "wide_joint": wide,
                          "ms_per_step": round(t * 1e3, 3), "simulations_per_s": round(B * S / t, 1),
                          "fused_kernel": loop.tb.fused_kernel(), "prepare_kernel": loop.tb.prepare_kernel(),
                          "max_root_degree": max(len(v) for v in res.sampled_visit_count),
                          "graph_nodes": loop.graph_nodes[0] if loop.graph_nodes else None, "steps": args.steps}),
              flush=True)
        release()


if __name__ == "__main__":
    main()
