"""Times the agent wavefront over reanalyze batches (consume.reanalyze_policy_targets_many on a
SampledMCTS(mixed_agents=True): G + N - 1 merged searches whose rows are of different agents, the agent a
per-row device table) against the G consecutive consume.reanalyze_policy_targets calls it replaces (G * N
per-agent searches on a driver without the flag: the code path of the parent commit), at the BASELINE
reanalyze batch: SMAC 3m (3 agents, 9 actions), G = 4 batches of 256 trajectories x (5 + 1) unroll steps =
1,536 rows, 50 simulations, K = 1, MuZeroShapedNet under autocast, fused_transforms and later_action_cache
on.

wavefront      both legs in one process, interleaved run by run, after warm-up calls that run eagerly,
               record the graphs and replay them once; every call ends with a device synchronisation.
ticks          the wavefront once more with a synchronisation around every tick's merged search.
glue launches  200 launches of mz_policy_glue / mz_policy_glue_rows and of mz_policy_glue_later /
               mz_policy_glue_later_rows on 4,608 rows in a recorded graph each, replayed: the time of a graph
               node with and without the table's dependent load.

Both legs start every run from the same generator state and their outputs are compared field by field.
MuZeroShapedNet's matrix products need not give row i the same bits at another row count, so inequality
here is the model's, not the search's (tests/test_mixed_agents.py compares on a model of elementwise
operations).  Prints one JSON line.

    python scripts/time_mixed_agents.py [--runs 3] [--reps 3] [--batches 4]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mazero_amd import consume  # noqa: E402
from mazero_amd._capi import MZ_DT_F16, check  # noqa: E402
from mazero_amd.cytree import Tree_batch  # noqa: E402
from mazero_amd.mcts_sampled import _LOOPS, SampledMCTS, ensure_half_exp  # noqa: E402
from mazero_amd.nets import SearchConfig, make_net, make_root_batch  # noqa: E402


def glue_launch_times(B, N, A, launches=200, replays=20):
    """us per graph node of the policy glue with the agent as a launch constant and as a table entry."""
    dev = torch.device("cuda", 0)
    tb = Tree_batch(B, 1, A, 1, 4, 0.01, 0, 0.75, 0.8)
    lib, h = tb._lib, tb._h
    ensure_half_exp(lib, 0)
    x = torch.randn(B, N * A, device=dev).half()
    probs, beta = torch.empty(B, A, device=dev), torch.empty(B, A, device=dev)
    later = torch.zeros(B, N, dtype=torch.int32, device=dev)
    table = torch.from_numpy(np.arange(B, dtype=np.int32) % N).to(dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    calls = {
        "mz_policy_glue": lambda: lib.mz_policy_glue(h, p(x), MZ_DT_F16, N * A, A, 1.0, p(probs), p(beta)),
        "mz_policy_glue_rows": lambda: lib.mz_policy_glue_rows(h, p(x), MZ_DT_F16, N * A, N, p(table), 1.0, p(probs),
                                                               p(beta)),
        "mz_policy_glue_later": lambda: lib.mz_policy_glue_later(h, p(x), MZ_DT_F16, N * A, N, 0, 1.0, p(probs),
                                                                 p(beta), p(later)),
        "mz_policy_glue_later_rows": lambda: lib.mz_policy_glue_later_rows(h, p(x), MZ_DT_F16, N * A, N, p(table), 1.0,
                                                                           p(probs), p(beta), p(later)),
    }
    graphs = {}
    for name, fn in calls.items():
        tb._sync_stream()
        check(lib, fn(), name)  # (once eagerly)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            tb._sync_stream()  # the handle launches on the capturing stream
            for _ in range(launches):
                check(lib, fn(), name)
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    tb._sync_stream()
    us = {name: [] for name in calls}
    for _ in range(replays):  # interleaved
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / launches)
    return {name: dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3))
            for name, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--trajectories", type=int, default=256)
    ap.add_argument("--sims", type=int, default=50)
    a = ap.parse_args()
    N, A, U = 3, 9, 5
    G, B = a.batches, a.trajectories * (U + 1)
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=a.sims, sampled_action_times=1)
    net = make_net(N, A, seed=0, device=dev)
    batches = [make_root_batch(net, B, 64, seed=10 + g, device=dev, legal_zero_frac=0.2) for g in range(G)]
    outs, legals = [o for o, _ in batches], [la for _, la in batches]
    masks = [np.random.default_rng(g).integers(0, 2, size=B) for g in range(G)]
    kw = dict(fused_transforms=True, later_action_cache=True)
    rs = {"consecutive": np.random.RandomState(0), "wavefront": np.random.RandomState(0)}
    drv = {"consecutive": SampledMCTS(cfg, rs["consecutive"], **kw),
           "wavefront": SampledMCTS(cfg, rs["wavefront"], mixed_agents=True, **kw)}

    def consecutive():
        return [consume.reanalyze_policy_targets(drv["consecutive"], net, outs[g], legals[g], masks[g], dev)
                for g in range(G)]

    def wavefront():
        return consume.reanalyze_policy_targets_many(drv["wavefront"], net, outs, legals, masks, dev)

    legs = {"consecutive": consecutive, "wavefront": wavefront}
    for fn in legs.values():  # eager, recorded, replayed
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    equal, states_equal = [], []
    for run in range(a.runs):
        res = {}
        for name, fn in legs.items():
            rs[name].seed(100 + run)  # both legs from the same generator state
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[name] = fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            ms[name].append(float(np.median(ts)))
        fields = res["consecutive"][0]._fields
        equal.append({f: all(torch.equal(getattr(x, f), getattr(y, f))
                             for x, y in zip(res["consecutive"], res["wavefront"])) for f in fields})
        sa, sb = rs["consecutive"].get_state(), rs["wavefront"].get_state()
        states_equal.append(bool(sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]))

    # the ticks: a synchronisation around every merged search of one more wavefront
    d = drv["wavefront"]
    inner, ticks = d.batch_search_many_device, []

    def timed(*args, **kwargs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = inner(*args, **kwargs)
        torch.cuda.synchronize()
        ticks[-1].append(round((time.perf_counter() - t0) * 1e3, 3))
        return r

    d.batch_search_many_device = timed
    for _ in range(a.reps):
        ticks.append([])
        wavefront()
    del d.batch_search_many_device
    plan = consume.agent_wavefront(G, N)
    loops = sorted({(k[8][0], str(k[4]), v.graph_nodes[0]) for k, v in _LOOPS.items() if v.graph_nodes})
    res = dict(rows=B, batches=G, agents=N, actions=A, sims=a.sims, runs=a.runs, reps=a.reps, **kw,
               device=torch.cuda.get_device_name(0),
               ms={name: dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3),
                              runs=[round(x, 3) for x in v]) for name, v in ms.items()},
               outputs_equal=equal, np_random_equal=states_equal,
               ticks=[dict(entries=t, rows=B * len(t), ms=[rep[i] for rep in ticks]) for i, t in enumerate(plan)],
               graph_nodes=[dict(rows=r, agent=c, nodes=n) for r, c, n in loops],
               glue_launch_us=glue_launch_times(B * min(G, N), N, A))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
