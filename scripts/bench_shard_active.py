"""What a falling active count costs two sharded ranks, without and with `shard_active`'s search.

Two ranks of 128 environments each are emulated on one GPU, one after the other in every environment
step (one process: the ranks share nothing but the device).  Schedule, on SMAC 3m shapes (3 agents,
9 actions) with `MuZeroShapedNet` under autocast, `fused_transforms` on, 50 simulations, K = 1: 5 steps
with all 256 environments running, then 60 steps in which one more environment has finished at every
step, alternately the last one still running on rank 0 and on rank 1, so the active count falls 255,
254, ..., 196 as in scripts/bench_active_roots.py and rank 1's position in the active list moves at
every other step.

Each rank searches its own rows of the active list as the root shard (p_lo, p_hi, n) of
shard.active_shard:
  plain         SampledMCTS(root_shard=...): the tree handle is keyed by the shard's size and its offset,
                so a step after an environment finished meets a new handle, new loops and eager searches;
  shard_active  SampledMCTS(root_capacity=128, root_shard=..., device_root_offset=True), what
                SelfPlayShard(shard_active=True) builds: one 128-root handle per rank geometry whose root
                offset is device state, its recorded loops replayed at every size and position.
Both legs run from the same seeds.  Printed per leg: ms per step (both ranks, one after the other) for
every step, the handles and loops created, the graph replays; then one JSON summary line.

    python scripts/bench_shard_active.py [--repeats R] [--out FILE]

One GPU process at a time: this launcher never touches the GPU; each leg is a fresh child process
under its own time limit, one after the other (R rounds of plain, shard_active), and the first leg that
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
N, A, TOTAL, WORLD, SIMS, OBS = 3, 9, 256, 2, 50, 64
FULL_STEPS, SHRINK_STEPS = 5, 60
LEG_TIMEOUT = 300  # seconds; a leg takes well under a minute


def schedule():
    """The sorted active lists of the run: everyone for FULL_STEPS steps, then one environment fewer at
    every step, the last one still running on rank 0 and on rank 1 in turn."""
    running = [list(range(r * TOTAL // WORLD, (r + 1) * TOTAL // WORLD)) for r in range(WORLD)]
    out = [sorted(sum(running, [])) for _ in range(FULL_STEPS)]
    for i in range(SHRINK_STEPS):
        running[i % WORLD].pop()
        out.append(sorted(sum(running, [])))
    return out


def leg(name: str) -> None:
    sys.path.insert(0, ROOT)
    import mazero_amd  # noqa: F401  (HIP runtime settings, before anything initialises HIP)
    import numpy as np
    import torch

    from mazero_amd import mcts_sampled as ms
    from mazero_amd.nets import NetworkOutput, SearchConfig, make_net, make_root_batch
    from mazero_amd.shard import active_shard, shard_bounds

    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=SIMS, sampled_action_times=1)
    nets = [make_net(N, A, seed=0, device=dev) for _ in range(WORLD)]  # a loop's key carries the model: one per rank
    batches = [make_root_batch(nets[0], TOTAL, OBS, seed=10 + i, device=dev, legal_zero_frac=0.2) for i in range(3)]
    rs = [np.random.RandomState(0) for _ in range(WORLD)]
    cap = TOTAL // WORLD

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

    def rank_step(i, r, active):  # selfplay_worker.py:171-211 on the rank's part of the active list
        p_lo, p_hi, n = active_shard(active, *shard_bounds(TOTAL, WORLD, r))
        kw = dict(root_capacity=cap, device_root_offset=True) if name == "shard_active" else {}
        mcts = ms.SampledMCTS(cfg, rs[r], fused_transforms=True, root_shard=(p_lo, p_hi, n), **kw)
        out, legal = batches[i % len(batches)]
        rows = torch.as_tensor(active[p_lo:p_hi], device=dev)
        host = np.asarray(active[p_lo:p_hi])
        out = NetworkOutput(out.hidden_state[rows], out.reward[host], out.value[host], out.policy_logits[host])
        B = p_hi - p_lo
        acts = np.zeros((B, N), np.int32)
        for agent in range(N):
            factor = acts[:, :agent].copy() if agent else None
            res = mcts.batch_search(nets[r], out, agent, factor, N, legal[host], device=dev, add_noise=True)
            assert res.value.shape == (B,) and len(res.sampled_actions) == B
            acts[:, agent] = [int(a[np.argmax(v), 0]) if len(a) else 0
                              for a, v in zip(res.sampled_actions, res.sampled_visit_count)]

    ms_per_step, ms_per_rank, replayed = [], [], []
    for i, active in enumerate(schedule()):
        before = made["replays"]
        per_rank = []
        for r in range(WORLD):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rank_step(i, r, active)
            torch.cuda.synchronize()
            per_rank.append((time.perf_counter() - t0) * 1e3)
        ms_per_rank.append(per_rank)
        ms_per_step.append(sum(per_rank))
        replayed.append(made["replays"] - before)
        print(f"{name} step {i:2d} active {len(active):3d} {ms_per_step[-1]:9.3f} ms "
              f"(ranks {' '.join(f'{x:8.3f}' for x in per_rank)})  replayed {replayed[-1]}/{WORLD * N} searches",
              flush=True)
    full, shrink = ms_per_step[2:FULL_STEPS], ms_per_step[FULL_STEPS:]  # (steps 0 and 1: eager, then recording)
    slow = [max(x) for x in ms_per_rank[FULL_STEPS:]]  # the slower rank of a step: what two GPUs would wait for
    print(json.dumps({
        "leg": name, "schedule": f"{FULL_STEPS} x {TOTAL} active, then {TOTAL - 1} .. {TOTAL - SHRINK_STEPS}, "
                                 f"{WORLD} ranks emulated in sequence",
        "searches": WORLD * N * (FULL_STEPS + SHRINK_STEPS),
        "handles_created": made["handles"], "loops_created": made["loops"], "graph_replays": made["replays"],
        "ms_step_all_active_replayed_median": round(float(np.median(full)), 3),
        "ms_step_shrinking_median": round(float(np.median(shrink)), 3),
        "ms_step_shrinking_mean": round(float(np.mean(shrink)), 3),
        "ms_step_shrinking_min_max": [round(min(shrink), 3), round(max(shrink), 3)],
        "ms_slower_rank_shrinking_median": round(float(np.median(slow)), 3),
        "ms_total": round(float(np.sum(ms_per_step)), 1)}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["plain", "shard_active"], help="run one leg in this process (the launcher's child)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", help="also write the legs' output to this file")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg)
        return 0
    sink = open(args.out, "w") if args.out else None
    for r in range(args.repeats):
        for name in ("plain", "shard_active"):
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
