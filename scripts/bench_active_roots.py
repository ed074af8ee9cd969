"""What a shrinking batch costs the search loop, without and with `root_capacity`.

The reference's self-play loop searches only the environments still running
(selfplay_worker.py:171-211), so the root count falls step by step as episodes end.  A plain
`SampledMCTS` meets a new geometry at every new count: a new tree handle, new per-agent loops and an
eager search, and a loop replays its recorded graph only from its third search on.
`SampledMCTS(root_capacity=256)` serves every count on the 256-root handle and its recorded loops.

Schedule, on SMAC 3m shapes (3 agents, 9 actions) with `MuZeroShapedNet` under autocast,
`fused_transforms` on, 50 simulations, K = 1: 5 environment steps at 256 roots, then 60 steps in which
the active count falls 255, 254, ..., 196.  Both legs run it from the same seeds.  Printed per leg: ms
per step for every step, how many tree handles and loops the leg created, and how many of its agent
searches were graph replays; then one JSON summary line per leg.

    python scripts/bench_active_roots.py [--repeats R] [--out FILE]

One GPU process at a time: this launcher never touches the GPU; each leg is a fresh child process
under its own time limit, one after the other (R rounds of plain, capacity), and the first leg that
fails, is killed by a signal or runs into its limit ends the run with nothing started after it.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, A, ROOTS, SIMS, OBS = 3, 9, 256, 50, 64
SCHEDULE = [ROOTS] * 5 + list(range(ROOTS - 1, ROOTS - 61, -1))
LEG_TIMEOUT = 240  # seconds; a leg takes well under a minute


def leg(name: str) -> None:
    sys.path.insert(0, ROOT)
    import mazero_amd  # noqa: F401  (HIP runtime settings, before anything initialises HIP)
    import numpy as np
    import torch

    from mazero_amd import mcts_sampled as ms
    from mazero_amd.nets import NetworkOutput, SearchConfig, make_net, make_root_batch

    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=SIMS, sampled_action_times=1)
    net = make_net(N, A, seed=0, device=dev)
    batches = [make_root_batch(net, ROOTS, OBS, seed=10 + i, device=dev, legal_zero_frac=0.2) for i in range(3)]
    mcts = ms.SampledMCTS(cfg, np.random.RandomState(0), fused_transforms=True,
                          root_capacity=ROOTS if name == "capacity" else None)

    # what the leg creates and replays
    made = {"handles": 0, "loops": 0, "replays": 0}

    class CountedTree(ms.Tree_batch):
        def __init__(self, *a, **k):
            made["handles"] += 1
            super().__init__(*a, **k)

    class CountedLoop(ms._SearchLoop):
        def __init__(self, *a, **k):
            made["loops"] += 1
            super().__init__(*a, **k)

    ms.Tree_batch, ms._SearchLoop = CountedTree, CountedLoop
    graph_replay = torch.cuda.CUDAGraph.replay

    def counted_replay(self):
        made["replays"] += 1
        return graph_replay(self)

    torch.cuda.CUDAGraph.replay = counted_replay

    def env_step(i, B):  # selfplay_worker.py:171-211 on the first B environments
        out, legal = batches[i % len(batches)]
        out = NetworkOutput(out.hidden_state[:B], out.reward[:B], out.value[:B], out.policy_logits[:B])
        acts = np.zeros((B, N), np.int32)
        for agent in range(N):
            factor = acts[:, :agent].copy() if agent else None
            res = mcts.batch_search(net, out, agent, factor, N, legal[:B], device=dev, add_noise=True)
            assert res.value.shape == (B,) and len(res.sampled_actions) == B
            acts[:, agent] = [int(a[np.argmax(v), 0]) if len(a) else 0
                              for a, v in zip(res.sampled_actions, res.sampled_visit_count)]
        return acts

    ms_per_step, replayed = [], []
    for i, B in enumerate(SCHEDULE):
        before = made["replays"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env_step(i, B)
        torch.cuda.synchronize()
        ms_per_step.append((time.perf_counter() - t0) * 1e3)
        replayed.append(made["replays"] - before)
        print(f"{name} step {i:2d} roots {B:3d} {ms_per_step[-1]:9.3f} ms  replayed {replayed[-1]}/{N} searches",
              flush=True)
    full, shrink = ms_per_step[2:5], ms_per_step[5:]  # (steps 0 and 1 at 256 roots: eager, then recording)
    print(json.dumps({
        "leg": name, "schedule": "5 x 256 roots, then 255 .. 196", "searches": N * len(SCHEDULE),
        "handles_created": made["handles"], "loops_created": made["loops"], "graph_replays": made["replays"],
        "ms_step_256_replayed_median": round(float(np.median(full)), 3),
        "ms_step_256_replayed": [round(x, 3) for x in full],
        "ms_step_shrinking_median": round(float(np.median(shrink)), 3),
        "ms_step_shrinking_mean": round(float(np.mean(shrink)), 3),
        "ms_step_shrinking_min_max": [round(min(shrink), 3), round(max(shrink), 3)],
        "ms_total": round(float(np.sum(ms_per_step)), 1)}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["plain", "capacity"], help="run one leg in this process (the launcher's child)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", help="also write the legs' output to this file")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg)
        return 0
    sink = open(args.out, "w") if args.out else None
    for r in range(args.repeats):
        for name in ("plain", "capacity"):
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name], timeout=LEG_TIMEOUT,
                                   stdout=subprocess.PIPE, text=True)  # (stderr passes through)
                text, rc = p.stdout, p.returncode
            except subprocess.TimeoutExpired as e:  # (the child was killed)
                text = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
                rc = 124
            block = f"# round {r + 1}, leg {name}\n{text}"
            print(block, end="", flush=True)
            if sink:
                sink.write(block)
                sink.flush()
            if rc != 0:  # nothing more runs on the GPU after a failure
                print(f"leg {name} ended with status {rc}: stopping", flush=True)
                return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
