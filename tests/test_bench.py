"""bench.py contract pieces that run without a GPU: argument defaults (N = 1, the headline
configuration) and the CPU baseline leg (the oracle library timed on host cores, one core plus the
multi-core leg), on a small sample."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_defaults_are_the_headline_config():
    import bench

    a = bench.parse([])
    assert (a.map, a.roots, a.sims, a.sampled_times) == ("3m", 256, 50, 1)
    assert not a.strong and not a.no_graph and a.broadcast_every == 0
    # a plain run measures the headline figure only; nothing is written unless asked for
    assert not a.full and a.dump_outputs is None
    assert bench.parse(["--full", "--dump-outputs", "d"]).full


def _run_main(monkeypatch, capsys, argv):
    """bench.main() in this process with `argv`; the JSON line it printed."""
    import json

    import bench

    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    capsys.readouterr()
    bench.main()
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load_dump(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _expected_searches(port_lib, seed, B, A, S, N, K=1):
    """The port's outputs for the inputs bench.py generates at --seed (rank 0 of a one-rank job)."""
    from mazero_amd.cytree import Tree_batch
    from mazero_amd.synthetic import DEFAULTS, make_search_inputs, run_search

    d = DEFAULTS
    rng = np.random.default_rng(seed * 1000)
    out = []
    for inp in [make_search_inputs(rng, B, A, S) for _ in range(N)]:
        tb = Tree_batch(B, 1, A, K, S, d["delta_lb"], inp.seed, d["rho"], d["lam"], lib=port_lib)
        out.append(run_search(tb, inp, K, per_sim=False))
    return out


def test_dump_outputs_files(tmp_path, monkeypatch):
    """--dump-outputs writes float arrays; past the size limit, the same seeded sample every time."""
    import bench

    arrays = dict(a=np.arange(12, dtype=np.int32).reshape(3, 4), b=np.linspace(0, 1, 5000, dtype=np.float32),
                  c=np.ones(3, np.float64))
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    got = _load_dump(str(tmp_path / "all"))
    assert sorted(got) == ["a", "b", "c"]
    assert got["a"].dtype == np.float32 and got["a"].shape == (3, 4) and np.array_equal(got["a"], arrays["a"])
    assert got["b"].dtype == np.float32 and np.array_equal(got["b"], arrays["b"]) and got["c"].dtype == np.float64
    monkeypatch.setattr(bench, "DUMP_LIMIT", 3000)
    bench.dump_outputs(str(tmp_path / "s1"), arrays)
    bench.dump_outputs(str(tmp_path / "s2"), arrays, prefix="rank1_")
    s1, s2 = _load_dump(str(tmp_path / "s1")), _load_dump(str(tmp_path / "s2"))
    assert sorted(s2) == ["rank1_a", "rank1_b", "rank1_c"]
    assert sum(v.nbytes for v in s1.values()) <= 3000
    assert s1["b"].shape == (250,) and np.isin(s1["b"], arrays["b"]).all() and len(set(s1["b"])) == 250
    assert np.array_equal(s1["b"], s2["rank1_b"]) and np.array_equal(s1["a"], arrays["a"])


def test_plain_run_dumps_its_outputs(port_lib, tmp_path, monkeypatch, capsys):
    """A plain run (here on the CPU port) times exactly --steps steps, measures nothing else, and
    --dump-outputs writes the last step's search outputs: the same in two runs, and the port's own."""
    B, S, N, A = 8, 6, 3, 9
    argv = ["--gpus", "1", "--backend", "port", "--roots", str(B), "--sims", str(S), "--steps", "3", "--warmup", "1",
            "--seed", "2"]
    line = _run_main(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "a")])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    # value = simulations of one step / ms_per_step (both rounded: 0.1 sims/s, 1e-4 ms)
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / (B * S * N) - 1) <= 1e-4 / line["ms_per_step"] + 1e-3
    assert line["roofline"] is None and line["cpu_baseline"] is None
    _run_main(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "b")])
    a, b = _load_dump(str(tmp_path / "a")), _load_dump(str(tmp_path / "b"))
    assert sorted(a) == [f"search{i}_values" for i in range(N)] and sorted(b) == sorted(a)
    exp = _expected_searches(port_lib, 2, B, A, S, N)
    for i in range(N):
        v = a[f"search{i}_values"]
        assert v.dtype == np.float32 and v.shape == (B,)
        assert np.array_equal(v.view(np.uint32), b[f"search{i}_values"].view(np.uint32))
        assert np.array_equal(v.view(np.uint32), np.asarray(exp[i]["root_values"], np.float32).view(np.uint32))


@pytest.mark.gpu
def test_gpu_run_dumps_its_outputs(port_lib, tmp_path, monkeypatch, capsys):
    """The timed HIP path at a small size (16 roots x 8 sims, graph replay): a plain run carries no
    roofline or CPU leg, --dump-outputs writes the last timed step's outputs -- bit for bit the CPU
    port's values, visit counts and last selection -- and a second run writes the same files, the
    gathered hidden states included.  --full --no-cpu adds the roofline."""
    B, S, N, A = 16, 8, 3, 9
    argv = ["--gpus", "1", "--roots", str(B), "--sims", str(S), "--steps", "2", "--warmup", "1", "--seed", "3"]
    line = _run_main(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "a")])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["config"]["graph"]
    assert line["roofline"] is None and line["cpu_baseline"] is None
    _run_main(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "b")])
    a, b = _load_dump(str(tmp_path / "a")), _load_dump(str(tmp_path / "b"))
    names = ("values", "marginal_visit_count", "sel_idx", "sel_idy", "sel_act", "leaf")
    assert sorted(a) == sorted(f"search{i}_{n}" for i in range(N) for n in names) and sorted(b) == sorted(a)
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    exp = _expected_searches(port_lib, 3, B, A, S, N)
    for i, e in enumerate(exp):
        assert np.array_equal(a[f"search{i}_values"].view(np.uint32),
                              np.asarray(e["root_values"], np.float32).view(np.uint32))
        assert np.array_equal(a[f"search{i}_marginal_visit_count"], np.asarray(e["marginal_visit_count"]))
        assert np.array_equal(a[f"search{i}_sel_idx"], e["sel_idx"][S - 1])
        assert np.array_equal(a[f"search{i}_sel_act"][:, 0], e["sel_act"][S - 1])
        assert np.array_equal(a[f"search{i}_sel_idy"], np.arange(B))
        assert a[f"search{i}_leaf"].shape == (B, N * 128) and np.isfinite(a[f"search{i}_leaf"]).all()
    full = _run_main(monkeypatch, capsys, argv + ["--full", "--no-cpu"])
    assert full["roofline"]["achieved"] > 0 and full["cpu_baseline"] is None


def test_cpu_baseline_fields(port_lib):
    import bench
    from mazero_amd.synthetic import make_search_inputs

    rng = np.random.default_rng(0)
    B, A, K, S, N = 16, 9, 1, 10, 3
    inputs = [make_search_inputs(rng, B, A, S) for _ in range(N)]
    r = bench.cpu_baseline(inputs, B, A, K, S, N, 0.4, procs=2)
    assert r is not None
    assert r["unit"] == "simulations/s" and r["cores"] == 1 and r["kind"] in ("reference", "port")
    assert r["value"] > 0 and "sims" in r["sample"]
    mc = r["multi_core"]
    assert mc["value"] > 0 and mc["processes"] == 2 and mc["cores"] == 2


def test_gpus_flag_spawns_ranks(port_lib):
    """`bench.py --gpus 2` without torchrun starts two ranks itself (torch.distributed.run), each
    rank reports the job's world size, and rank 0 prints one JSON line.  `value` is the weak leg:
    every rank searches its own --roots roots (one shard of the node's self-play per GPU, the
    "whole node" of the metric); the strong leg (--roots roots split over the ranks) rides beside
    it.  --backend port keeps it on the CPU (gloo): the plumbing, not a measurement."""
    import json
    import subprocess

    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "port", "--roots", "8",
            "--sims", "6", "--steps", "2", "--warmup", "1", "--no-cpu"]
    r = subprocess.run(base, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak"
    assert line["config"]["roots_total"] == 16 and line["config"]["roots_per_gpu"] == 8
    assert "8 roots" in line["metric"] and "per GPU" in line["metric"]
    st = line["strong_scaling"]
    assert st["roots_total"] == 8 and st["roots_per_gpu"] == 4 and st["value"] > 0
    assert line["value"] > 0
    # the line verifies itself: the collective's world size, every rank's device and own step time
    # in both legs; the headline ms_per_step is the max over ranks
    rk = line["ranks"]
    assert rk["world_size"] == 2 and rk["backend"] == "gloo"
    assert [r["rank"] for r in rk["per_rank"]] == [0, 1]
    assert [r["local_rank"] for r in rk["per_rank"]] == [0, 1]
    for r in rk["per_rank"]:
        assert set(r["ms_per_step"]) == {"strong", "weak"} and min(r["ms_per_step"].values()) > 0
        assert r["device"] == "cpu"
    assert abs(max(r["ms_per_step"]["weak"] for r in rk["per_rank"]) - line["ms_per_step"]) < 1e-3
    assert abs(max(r["ms_per_step"]["strong"] for r in rk["per_rank"]) - st["ms_per_step"]) < 1e-3
    # --strong: the strong leg is the headline (the 8 roots split over the two ranks)
    r = subprocess.run(base + ["--strong"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][0])
    assert line["scaling"] == "strong" and line["config"]["roots_total"] == 8
    assert "8 roots" in line["metric"] and "per GPU" not in line["metric"]
    assert line["weak_scaling"]["roots_total"] == 16


def test_gpus_flag_eight_ranks(port_lib):
    """The driver's widest job, rehearsed on the CPU: `bench.py --gpus 8` over gloo with the port
    backend, 256 roots on every rank (the strong leg beside it: 32 per rank); rank 0 prints one line
    naming 8 ranks.  With
    --broadcast-every 1 (BASELINE config #5's weight broadcast in the timed loop) the line carries
    every rank's sync count, checkpoint and own time per sync."""
    import json
    import subprocess

    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--backend", "port", "--sims", "4",
           "--steps", "2", "--warmup", "1", "--no-cpu", "--broadcast-every", "1"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 8 and line["scaling"] == "weak"
    assert line["config"]["roots_total"] == 2048 and line["config"]["roots_per_gpu"] == 256
    assert line["metric"].endswith("SMAC 3m, 256 roots×4 sims per GPU")
    assert line["strong_scaling"]["roots_total"] == 256 and line["strong_scaling"]["roots_per_gpu"] == 32
    rk = line["ranks"]
    assert rk["world_size"] == 8 and [x["rank"] for x in rk["per_rank"]] == list(range(8))
    assert abs(max(x["ms_per_step"]["weak"] for x in rk["per_rank"]) - line["ms_per_step"]) < 1e-3
    # config #5's weight broadcast inside the timed loop (--broadcast-every 1): one sync per env step
    # on every rank, each moving the 27m network's weights from rank 0 (warm-up sync + 2 timed)
    wb = line["weight_broadcast"]
    assert wb["every_steps"] == 1 and wb["syncs"] == 2 and wb["src_rank"] == 0 and wb["bytes"] > 1_000_000
    assert wb["checkpoint"] == 3 and wb["transfers"] == 3 and "27m_vs_30m" in wb["network"]
    assert len(wb["per_rank_ms_per_sync"]) == 8 and min(wb["per_rank_ms_per_sync"]) > 0
    for x in rk["per_rank"]:
        for kind in ("weak", "strong"):
            assert x["weight_broadcast"][kind]["syncs"] == 2 and x["weight_broadcast"][kind]["checkpoint"] == 3


def test_strong_leg_is_the_global_batch(port_lib):
    """The strong leg's ranks search slices of ONE global batch: rank r's inputs are rows [lo, hi)
    of the inputs an unsharded run generates (so N > 1 measures the metric's own job)."""
    import bench
    from mazero_amd.shard import shard_bounds, slice_inputs
    from mazero_amd.synthetic import make_search_inputs

    rng = np.random.default_rng(0)
    full = [make_search_inputs(rng, 10, 9, 4) for _ in range(3)]
    lo, hi = shard_bounds(10, 4, 1)
    part = [slice_inputs(x, lo, hi) for x in full]
    assert part[0].B == hi - lo and np.array_equal(part[2].policy, full[2].policy[:, lo:hi])
    assert bench.parse(["--gpus", "4"]).roots == 256


def test_world_size_mismatch_fails(port_lib):
    """Under a launcher whose world size differs from --gpus, bench.py refuses to report."""
    import subprocess

    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "port", "--roots", "4",
           "--sims", "4", "--steps", "1", "--no-cpu"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--gpus 2" in (r.stderr + r.stdout)


def test_matrix_config_ptree_leg(port_lib):
    """BASELINE config #1 (matrix, N = 2, A = 3, 8 roots x 25 sims): bench.py knows the map and
    its CPU baseline carries the pure-Python ptree timing beside the ctree's."""
    import bench
    from mazero_amd.synthetic import make_search_inputs

    assert bench.CONFIGS["matrix"] == (2, 3)
    rng = np.random.default_rng(1)
    B, A, K, S, N = 8, 3, 1, 25, 2
    inputs = [make_search_inputs(rng, B, A, S) for _ in range(N)]
    r = bench.cpu_baseline(inputs, B, A, K, S, N, 0.4, procs=2, ptree=True)
    pt = r["ptree"]
    assert pt["value"] > 0 and pt["cores"] == 1 and "ptree" in pt["sample"]
