"""k_prepare1, the role-specialised prepare kernel of K = 1 searches (needs an MI355X: `pytest -m gpu`).

Handles with agent_num = 1, sampled_times = 1 and at most 64 actions launch k_prepare1 for
mz_prepare and mz_prepare_select: five waves, the root wave and four twist waves, the first of which
seeds the engine.  The root wave issues the root's loads, takes the seeding barrier with them in
flight, computes the engine words the draw and the header need itself, builds the distribution,
draws and stores the records and the header; it takes every barrier of the twist (one per 624-word
block after the first) at a point of its own work that depends on the action count.  It must leave
byte for byte what k_prepare leaves.

Every case runs searches through the fused device loop against the CPU port, bit for bit: per launch
idx, idy, act and the gathered row; at the end every readback and the error word; the event counters
against the same search on a handle that keeps k_prepare (MZ_PREPARE_GENERAL, read at mz_create),
which is compared with the port as well.  Every case asserts through `prepare_kernel` which kernel
its handle launches.  The shapes are the smallest that take each path: each class of the
distribution, one, two, three and five twist blocks (the chain consumes engine words past 624 and
1,248 at S = 50), each seeding path, one workgroup and more workgroups than CUs.

An error the first selection itself would report (kErrRoot: a selection on a root without children)
cannot arise at K = 1 -- the root's expansion always creates one child, and the pool holds S + 2 >= 2
nodes -- so no case constructs it.
"""
from __future__ import annotations

import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

if __name__ != "__main__":
    import test_chain3_round1 as round1
    import test_chain3_tail as tail
    from conftest import assert_same
    from test_gpu_parity import gpu_lib, make_tb, to_device  # noqa: F401  (gpu_lib: fixture)

    torch = pytest.importorskip("torch")

K = 1
NEW, GENERAL = "k_prepare1", "k_prepare"
COUNTERS = ("selects", "path_edges", "scored", "expands", "new_children", "backup_nodes", "minmax_nodes")
# the searches the two kernels run against each other in child processes: (B, A, S, H, seed)
CHILD_CASES = [(3, 9, 20, 384, 9200), (5, 36, 6, 4, 9201), (2, 1, 6, 0, 9202), (4, 9, 50, 4, 9203)]


def _inputs(B, A, S, seed, **kw):
    from mazero_amd.synthetic import make_search_inputs

    return make_search_inputs(np.random.default_rng(seed), B, A, S, **kw)


def _general(gpu_lib, inp, monkeypatch, **kw):  # noqa: F811
    monkeypatch.setenv("MZ_PREPARE_GENERAL", "1")  # (read at mz_create)
    tb = make_tb(gpu_lib, inp, K, {}, **kw)
    monkeypatch.delenv("MZ_PREPARE_GENERAL")
    assert tb.prepare_kernel() == GENERAL
    return tb


class _HostPrepare:
    """The handle, with prepare taking its inputs from host memory (the staged path)."""

    def __init__(self, tb):
        self._tb = tb

    def __getattr__(self, name):
        return getattr(self._tb, name)

    def prepare(self, r, v, p, b, k, eps, n):
        h = lambda x: x.cpu().numpy()  # noqa: E731
        return self._tb.prepare(h(r), h(v), h(p), h(b), k, eps, h(n))


def _check(gpu_lib, port_lib, inp, monkeypatch, first="prepare_select", H=4, kernel=NEW, **kw):  # noqa: F811
    """One search against the port, then the same on a handle that keeps k_prepare; returns the handle."""
    where = f"B={inp.B} A={inp.A} S={inp.S} first={first}: "
    exp = round1._port(port_lib, inp)
    tb = make_tb(gpu_lib, inp, K, {}, **kw)
    assert tb.prepare_kernel() == kernel, where
    pool = round1._pool(inp, H) if H else None
    modes = ["fused"] * inp.S
    drive = lambda h: round1._drive(_HostPrepare(h) if first == "prepare_host" else h, inp, modes,  # noqa: E731
                                    first="prepare_select" if first == "prepare_select" else "prepare", pool=pool)
    out, gathered = drive(tb)
    assert_same(out, exp, where)
    if pool is not None:
        round1._rows_ok(pool, out, gathered, where)
    tb.synchronize()  # (raises on a non-zero error word)
    if kernel == NEW:
        tb2 = _general(gpu_lib, inp, monkeypatch, **kw)
        out2, _ = drive(tb2)
        assert_same(out2, exp, where + "k_prepare ")
        round1._same_counters(tb, tb2, where)
        assert tb.stats()["selects"] == inp.B * inp.S and tb.stats()["expands"] == inp.B * (inp.S + 1)
    return tb


# ---- action counts: no draw, both ends of every cdf_short class, the LDS form ----
@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 2, 4, 5, 9, 12, 13, 16, 17, 36, 64])
def test_action_counts(gpu_lib, port_lib, A, monkeypatch):  # noqa: F811
    _check(gpu_lib, port_lib, _inputs(5, A, 6, 100 + A), monkeypatch)


@pytest.mark.gpu
def test_more_actions_than_lanes_keeps_the_general_kernel(gpu_lib, port_lib, monkeypatch):  # noqa: F811
    _check(gpu_lib, port_lib, _inputs(3, 65, 6, 165), monkeypatch, kernel=GENERAL)


# ---- twist blocks: one, two, three (engine words past 624 and 1,248 consumed), five; the root wave
# takes one barrier for each, at other points of its work for no draw, up to 16 and past 16 actions ----
@pytest.mark.gpu
@pytest.mark.parametrize("S", [6, 30, 50, 70])
def test_twist_blocks(gpu_lib, port_lib, S, monkeypatch):  # noqa: F811
    _check(gpu_lib, port_lib, _inputs(4, 9, S, 200 + S), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [30, 50])
@pytest.mark.parametrize("A", [1, 17, 36])
def test_twist_blocks_other_action_counts(gpu_lib, port_lib, A, S, monkeypatch):  # noqa: F811
    _check(gpu_lib, port_lib, _inputs(3, A, S, 250 + S + A), monkeypatch)


# ---- seeding: the checkpoint table, no table, a seed value beyond the table ----
@pytest.mark.gpu
@pytest.mark.parametrize("seeding", ["table", "chain", "beyond_table"])
def test_seeding_paths(gpu_lib, port_lib, seeding, monkeypatch):  # noqa: F811
    inp = _inputs(4, 9, 50, 300)
    if seeding == "beyond_table":
        inp = replace(inp, seed=100000)
    if seeding == "chain":
        monkeypatch.setenv("MZ_NO_SEED_TABLE", "1")  # (read at mz_create: both handles of _check)
    _check(gpu_lib, port_lib, inp, monkeypatch)


# ---- a shard's handle against the matching rows of the unsharded search ----
@pytest.mark.gpu
def test_root_offset(gpu_lib, port_lib):  # noqa: F811
    B, lo = 5, 2
    inp = _inputs(B, 9, 6, 400)
    full = round1._port(port_lib, inp)
    sub = replace(inp, B=B - lo, root_reward=inp.root_reward[lo:], root_value=inp.root_value[lo:],
                  root_policy=inp.root_policy[lo:], root_beta=inp.root_beta[lo:], root_noise=inp.root_noise[lo:],
                  reward=inp.reward[:, lo:], value=inp.value[:, lo:], policy=inp.policy[:, lo:], beta=inp.beta[:, lo:])
    tb = make_tb(gpu_lib, sub, K, {}, root_offset=lo)
    assert tb.prepare_kernel() == NEW
    out, _ = round1._drive(tb, sub, ["fused"] * sub.S, first="prepare_select")
    tb.synchronize()
    for k, v in full.items():
        want = v[:, lo:] if k in ("sel_idx", "sel_act") else v[lo:]
        got = np.asarray(out[k])
        if want.ndim == 2 and k.startswith("sampled_"):  # (padded to each search's own largest degree)
            w = max(want.shape[1], got.shape[1])
            want = np.pad(want, ((0, 0), (0, w - want.shape[1])))
            got = np.pad(got, ((0, 0), (0, w - got.shape[1])))
        assert got.shape == want.shape and np.array_equal(got.view(np.uint8), want.astype(got.dtype).view(np.uint8)), k


# ---- one workgroup; more workgroups than CUs ----
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 300])
def test_grid_sizes(gpu_lib, port_lib, B, monkeypatch):  # noqa: F811
    _check(gpu_lib, port_lib, _inputs(B, 9, 6, 500 + B), monkeypatch)


# ---- root noise off and on ----
@pytest.mark.gpu
@pytest.mark.parametrize("eps", [0.0, 0.25])
def test_root_noise(gpu_lib, port_lib, eps, monkeypatch):  # noqa: F811
    inp = _inputs(4, 9, 6, 600, noise_eps=eps)
    assert inp.noise_eps == eps
    _check(gpu_lib, port_lib, inp, monkeypatch)


# ---- masked rows: zero beta entries, the last action among them ----
@pytest.mark.gpu
def test_masked_rows(gpu_lib, port_lib, monkeypatch):  # noqa: F811
    inp = _inputs(5, 13, 6, 700, legal_zero_frac=0.4)
    p, b = inp.root_policy.copy(), inp.root_beta.copy()
    p[..., -1] = 0
    b[..., -1] = 0
    inp = replace(inp, root_policy=p, root_beta=b)
    assert (inp.root_beta[..., 0] == 0).all() and (inp.root_beta[..., -1] == 0).all() and (inp.root_beta[..., 1] > 0).all()
    _check(gpu_lib, port_lib, inp, monkeypatch)


def _concentrated(b, j):
    out = np.full(b.shape, 1e-6 / (b.shape[-1] - 1), np.float32)
    out[..., j] = np.float32(1.0 - 1e-6)
    return out


def _tiny_tail(b):
    out = b.copy()
    out[..., -3:] = out[..., :-3].sum(axis=-1, keepdims=True) * np.float32(1e-30)
    return out


# ---- distribution edge rows at the root: the forced cp = 1.0 of the last action ----
@pytest.mark.gpu
@pytest.mark.parametrize("row", ["concentrated", "tiny_tail"])
def test_distribution_edge_rows(gpu_lib, port_lib, row, monkeypatch):  # noqa: F811
    A = 9
    inp = _inputs(5, A, 6, 800)
    f = (lambda b: _concentrated(b, A - 1)) if row == "concentrated" else _tiny_tail
    inp = replace(inp, root_beta=f(inp.root_beta), beta=f(inp.beta))
    _check(gpu_lib, port_lib, inp, monkeypatch)
    if row == "concentrated":
        assert (round1._port(port_lib, inp)["sel_act"][0] == A - 1).all()  # (the root draws what the row is named for)


# ---- not tame: the header's tame = 0, the first fused launch takes the exact selection ----
@pytest.mark.gpu
@pytest.mark.parametrize("wild", ["prior", "value"])
@pytest.mark.parametrize("first", ["prepare", "prepare_select"])
def test_not_tame(gpu_lib, port_lib, wild, first, monkeypatch):  # noqa: F811
    inp = _inputs(3, 9, 6, 900)
    if wild == "prior":  # policy 1 over beta * 1e-31: the root child's prior is above 1e30
        inp = replace(inp, root_policy=np.ones_like(inp.root_policy), root_beta=inp.root_beta * np.float32(1e-31))
    else:
        v = inp.root_value.copy()
        v[1] = 1e31
        inp = replace(inp, root_value=v)
    _check(gpu_lib, port_lib, inp, monkeypatch, first=first)


# ---- entry points: mz_prepare on device and on host inputs (then batch_selection_device), mz_prepare_select ----
@pytest.mark.gpu
@pytest.mark.parametrize("first", ["prepare", "prepare_host", "prepare_select"])
@pytest.mark.parametrize("A", [1, 9])
def test_entry_points(gpu_lib, port_lib, first, A, monkeypatch):  # noqa: F811
    _check(gpu_lib, port_lib, _inputs(3, A, 6, 1000 + A), monkeypatch, first=first)


# ---- two searches on one handle; a second prepare after a search that ended in error ----
@pytest.mark.gpu
@pytest.mark.parametrize("first", ["prepare", "prepare_select"])
def test_two_searches_on_one_handle(gpu_lib, port_lib, first):  # noqa: F811
    B, A, S = 3, 9, 6
    inp1 = _inputs(B, A, S, 1100)
    inp2 = replace(_inputs(B, A, S, 1101), seed=inp1.seed + 12345)
    tb = make_tb(gpu_lib, inp1, K, {})
    assert tb.prepare_kernel() == NEW
    out, _ = round1._drive(tb, inp1, ["fused"] * 4, first=first, select_last=True)
    exp = round1._port(port_lib, inp1, n_sims=4, select_last=True)
    assert_same(out, {k: exp[k] for k in ("sel_idx", "sel_act")}, "first search: ")
    tb.reseed(inp2.seed)
    out, _ = round1._drive(tb, inp2, ["fused"] * S, first=first)
    assert_same(out, round1._port(port_lib, inp2), "second search: ")
    tb.synchronize()


@pytest.mark.gpu
def test_prepare_after_a_search_that_ended_in_error(gpu_lib, port_lib):  # noqa: F811
    B, A, S = 3, 9, 6
    inp = _inputs(B, A, S, 1200)
    n = S + 4  # (the pool is sized for simulation_num: a launch soon after overflows)
    long_inp = replace(inp, reward=np.resize(inp.reward, (n,) + inp.reward.shape[1:]),
                       value=np.resize(inp.value, (n,) + inp.value.shape[1:]),
                       policy=np.resize(inp.policy, (n,) + inp.policy.shape[1:]),
                       beta=np.resize(inp.beta, (n,) + inp.beta.shape[1:]))
    tb = make_tb(gpu_lib, inp, K, {})
    assert tb.prepare_kernel() == NEW
    round1._drive(tb, long_inp, ["fused"] * n, first="prepare_select", select_last=True)
    word, msg = round1._error_word(tb)
    assert word & 1 and "node pool exhausted" in msg, msg
    # the next prepare clears the error word and every header: a whole search equal to the port's
    inp2 = replace(_inputs(B, A, S, 1201), seed=inp.seed + 777)
    tb.reseed(inp2.seed)
    out, _ = round1._drive(tb, inp2, ["fused"] * S, first="prepare_select")
    assert_same(out, round1._port(port_lib, inp2), "after the error: ")
    tb.synchronize()


# ---- a search driven past simulation_num still raises ----
@pytest.mark.gpu
def test_past_simulation_num(gpu_lib, port_lib):  # noqa: F811
    from mazero_amd.cytree import Tree_batch

    probe = make_tb(gpu_lib, _inputs(3, 9, 6, 7000), K, {})
    assert probe.prepare_kernel() == NEW  # (the handles below are alike)
    tail.test_past_the_pool(gpu_lib, port_lib)
    B, A, S = 4, 3, 2
    tb = Tree_batch(B, 1, A, K, S, 0.01, 5, 0.75, 0.8, lib=gpu_lib)
    assert tb.prepare_kernel() == NEW
    p = np.full((B, 1, A), 1.0 / A, np.float32)
    z = np.zeros(B, np.float32)
    tb.prepare(z, z, p, p, K, 0.0, p)
    with pytest.raises(RuntimeError):
        for s in range(10):
            tb.batch_selection(19652.0, 1.25, 0.997)
            tb.batch_expansion_and_backup(s + 1, 0.997, K, z, z, p, p)


# ---- a captured graph of prepare_select and three fused launches, replayed twice ----
@pytest.mark.gpu
def test_graph_replayed_twice(gpu_lib, port_lib):  # noqa: F811
    B, A, S, n = 3, 9, 6, 3
    inp = _inputs(B, A, S, 1300)
    c2, c1, g = round1._consts()
    exp = round1._port(port_lib, inp, n_sims=n, select_last=True)
    d = to_device(inp)
    tb = make_tb(gpu_lib, inp, K, {})
    assert tb.prepare_kernel() == NEW
    dev = torch.device("cuda")
    idx = torch.zeros(n + 1, B, dtype=torch.int32, device=dev)
    idy = torch.zeros(n + 1, B, dtype=torch.int32, device=dev)
    act = torch.zeros(n + 1, B, 1, dtype=torch.int32, device=dev)

    def sequence():
        tb.prepare_selection_device(d.root_reward, d.root_value, d.root_policy, d.root_beta, K, d.noise_eps, d.root_noise,
                                    c2, c1, g, out=(idx[0], idy[0], act[0]))
        for s in range(n):
            tb.expansion_backup_selection_device(s + 1, g, K, d.reward[s], d.value[s], d.policy[s], d.beta[s], c2, c1,
                                                 out=(idx[s + 1], idy[s + 1], act[s + 1]))

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        sequence()  # (eager once: the handle's tables are in place before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        sequence()
    for rep in range(2):
        for o in (idx, idy, act):
            o.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert (idy.cpu().numpy() == np.arange(B, dtype=np.int32)[None]).all(), rep
        assert np.array_equal(idx.cpu().numpy(), exp["sel_idx"]), rep
        assert np.array_equal(act.cpu().numpy()[:, :, 0], exp["sel_act"]), rep
    tb.synchronize()


# ---- the two kernels against each other, in child processes (MZ_PREPARE_GENERAL is read at mz_create):
# the first fused launch behind either takes the header's hot copy (hot_tag == tot), seen through
# identical outputs of every launch ----
def _child(path):
    import conftest  # noqa: F401  (the import path, the HIP runtime settings)
    import torch as th
    from mazero_amd._lib import load
    from test_gpu_parity import make_tb as mk, run_fused, to_device as dev_of

    lib = load()
    res = {}
    for n, (B, A, S_, H, seed) in enumerate(CHILD_CASES):
        inp = _inputs(B, A, S_, seed)
        tb = mk(lib, inp, K, {})
        gen = th.Generator(device="cuda")
        gen.manual_seed(n)
        pool = th.randn(S_ + 1, B, H, device="cuda", generator=gen) if H else None
        out, gathered = run_fused(tb, dev_of(inp), K, {}, pool=pool)
        tb.synchronize()
        res[f"c{n}_prepare"] = np.frombuffer(tb.prepare_kernel().encode(), np.uint8)
        st = tb.stats()
        res[f"c{n}_counters"] = np.asarray([st[k] for k in COUNTERS], np.int64)
        for k, v in out.items():
            res[f"c{n}_{k}"] = np.asarray(v)
        if gathered is not None:
            res[f"c{n}_gathered"] = gathered.cpu().numpy().view(np.int32)
    np.savez(path, **res)


@pytest.mark.gpu
def test_both_prepare_kernels_agree(tmp_path):
    outs = []
    for name, general in (("new", None), ("general", "1")):
        env = {k: v for k, v in os.environ.items() if k != "MZ_PREPARE_GENERAL"}
        if general:
            env["MZ_PREPARE_GENERAL"] = general
        path = str(tmp_path / f"{name}.npz")
        r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), path], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(dict(np.load(path)))
    new, general = outs
    assert set(new) == set(general)
    for n in range(len(CHILD_CASES)):
        assert new[f"c{n}_prepare"].tobytes().decode() == NEW and general[f"c{n}_prepare"].tobytes().decode() == GENERAL
    for k in new:
        if k.endswith("_prepare"):
            continue
        assert new[k].shape == general[k].shape and new[k].dtype == general[k].dtype, k
        assert np.array_equal(new[k].view(np.uint8), general[k].view(np.uint8)), k


if __name__ == "__main__":
    _child(sys.argv[1])
