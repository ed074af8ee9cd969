"""Per-launch time of the driver glue's entry points (include/mzdriver.h) on cuda:0: policy, root and
joint-action glue through the narrow, wide, joint and later-action entry points, at the workload's own
action counts (9, 64) and past one tile (65, 128, 255).  A record, not a gate:
profiles/wide_glue/README.md and profiles/glue_unify/README.md hold the numbers.

Each configuration is a window of `--launches` back-to-back launches on the handle's stream between
two device events, after a warm-up window; the windows of all configurations alternate `--repeats`
times, and the per-launch time is window / launches (median, minimum and maximum over the repeats).
Two windows per configuration: "eager" enqueues the launches from Python, so the host's enqueue rate
bounds it from below; "graph" replays a captured graph of the same launches, which is how a search
runs them (mazero_amd.mcts_sampled).
B = 256 roots, N = 3 agents, float32 and float16 logits, sampled_tau = 1; the root glue with a legal
mask (about 30 % zeros) and noise_eps = 0.25; mz_policy_glue_later as the first agent's (two argmax
roles); the joint entry points over all 3 agents.

    python scripts/wide_glue_timing.py [--launches 2000] [--repeats 7] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, N = 256, 3
CONFIGS = [  # (entry point, A)
    ("mz_policy_glue", 9),
    ("mz_policy_glue", 64),
    ("mz_root_glue", 9),
    ("mz_root_glue", 64),
    ("mz_policy_glue_joint", 9),
    ("mz_root_glue_joint", 9),
    ("mz_policy_glue_later", 9),
    ("mz_policy_glue_later", 255),
    ("mz_joint_action", 9),
    ("mz_policy_glue_wide", 64),
    ("mz_policy_glue_wide", 65),
    ("mz_policy_glue_wide", 128),
    ("mz_policy_glue_wide", 255),
    ("mz_joint_action_wide", 255),
]


def make_launch(fn_name, A, dtype, handles):
    import torch

    from mazero_amd._capi import MZ_DT_F16, MZ_DT_F32, check
    from mazero_amd.cytree import Tree_batch
    from mazero_amd.mcts_sampled import ensure_half_exp

    dev = torch.device("cuda", 0)
    if A not in handles:
        handles[A] = Tree_batch(B, 1, A, 1, 4, 0.01, 0, 0.75, 0.8)
        ensure_half_exp(handles[A]._lib, 0)
    tb = handles[A]
    lib, h = tb._lib, tb._h
    code = MZ_DT_F16 if dtype == "float16" else MZ_DT_F32
    rng = np.random.default_rng(A)
    logits = torch.from_numpy(rng.standard_normal((B, N, A)).astype(dtype)).to(dev)
    fn = getattr(lib, fn_name)
    rows = N if fn_name.endswith("_joint") else 1  # agents per launch
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    if fn_name.startswith("mz_root_glue"):
        noise = torch.from_numpy(rng.dirichlet([0.3] * A, (B, rows)).astype(np.float32)).to(dev)
        legal = (rng.random((B, rows, A)) >= 0.3).astype(np.int32)
        legal[..., 0] = np.where(legal.sum(-1) == 0, 1, legal[..., 0])
        legal = torch.from_numpy(legal).to(dev)
        outs = [torch.empty(B, rows, A, device=dev) for _ in range(3)]
        where = (N * A, N) if rows > 1 else (N * A, A)  # (row stride, agents) / (row stride, col_offset)
        args = (h, p(logits), code, *where, p(legal), rows * A, p(noise), 0.25, 1.0, *[p(o) for o in outs])
        keep = (logits, noise, legal, outs)
    elif fn_name == "mz_policy_glue_later":
        probs, beta = torch.empty(B, A, device=dev), torch.empty(B, A, device=dev)
        later = torch.empty(B, N, dtype=torch.int32, device=dev)
        args = (h, p(logits), code, N * A, N, 0, 1.0, p(probs), p(beta), p(later))
        keep = (logits, probs, beta, later)
    elif fn_name.startswith("mz_policy_glue"):
        probs, beta = torch.empty(B, rows, A, device=dev), torch.empty(B, rows, A, device=dev)
        where = (N * A, N) if rows > 1 else (N * A, A)
        args = (h, p(logits), code, *where, 1.0, p(probs), p(beta))
        keep = (logits, probs, beta)
    else:  # mz_joint_action(_wide), current agent 0: the argmax of the two later agents' rows
        act = torch.zeros(B, dtype=torch.int32, device=dev)
        fac = torch.zeros(B, 1, dtype=torch.int32, device=dev)
        joint = torch.empty(B, N, dtype=torch.int64, device=dev)
        args = (h, C.c_void_p(logits.data_ptr()), code, N, 0, C.c_void_p(fac.data_ptr()), 1,
                C.c_void_p(act.data_ptr()), C.c_void_p(joint.data_ptr()))
        keep = (logits, act, fac, joint)

    def launch(n):
        tb._sync_stream()
        for _ in range(n):
            rc = fn(*args)
        check(lib, rc, fn_name)

    return launch, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "needs cuda:0"
    torch.cuda.set_device(0)
    handles, runs = {}, []
    for dtype in ("float32", "float16"):
        for fn_name, A in CONFIGS:
            launch, keep = make_launch(fn_name, A, dtype, handles)
            runs.append(dict(entry=fn_name, A=A, dtype=dtype, launch=launch, keep=keep, eager=[], graph=[]))
    for r in runs:  # warm-up: code objects loaded, every shape launched; then the graph recorded
        r["launch"](a.launches)
        torch.cuda.synchronize()
        r["g"] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(r["g"]):
            r["launch"](a.launches)
        r["g"].replay()
    torch.cuda.synchronize()

    def window(work):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        work()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / a.launches

    for _ in range(a.repeats):
        for r in runs:
            r["eager"].append(window(lambda: r["launch"](a.launches)))
            r["graph"].append(window(r["g"].replay))
    rows = [dict(entry=r["entry"], A=r["A"], dtype=r["dtype"], mode=mode, B=B, launches=a.launches,
                 repeats=a.repeats, us_per_launch_median=round(statistics.median(r[mode]), 3),
                 us_per_launch_min=round(min(r[mode]), 3), us_per_launch_max=round(max(r[mode]), 3))
            for r in runs for mode in ("eager", "graph")]
    for row in rows:
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
