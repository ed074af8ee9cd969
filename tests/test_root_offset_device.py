"""The root offset of a tree handle as device state (needs an MI355X: `pytest -m gpu`).

Tree i of a handle is seeded with random_seed * 2333 + root_offset + i.  The offset is a device word
beside the seed word, read by both prepare kernels with the seed in one 8-byte load, and moved by
mz_set_root_offset (include/mzdriver.h), so one handle -- and the graphs recorded on it -- serves a shard
whose position in the batch changes from search to search:

- kernel level: one 4-tree handle searches rows [0:4], [4:8] and [2:6] of an 8-root batch and gives the
  CPU port's rows of the unsharded search, for each prepare kernel and each seeding path;
- the argument checks of the two entry points;
- driver level: SampledMCTS(root_capacity=4, root_shard=..., device_root_offset=True) for three emulated
  ranks over a shrinking and growing active set, on one handle and one recorded loop per agent, against
  the plain search over the active rows;
- worker level: SelfPlayShard(shard_active=True) with the device consumers against the single rank.

Everything compared bit for bit at driver and worker level runs on `RowwiseNet`
(tests/test_root_capacity.py): row i of its outputs does not depend on the batch's row count.
"""
from __future__ import annotations

import ctypes as C
import warnings
from dataclasses import replace

import numpy as np
import pytest

import test_chain3_round1 as round1
from test_gpu_parity import gpu_lib, make_tb, run_fused, to_device  # noqa: F401  (gpu_lib: fixture)
from test_root_capacity import HID, RowwiseNet, _loops_of, _same, _trees_of, rowwise_batch, rowwise_config
from test_shard_active import ACTIVES, FIELDS, TOTAL, WORLD

torch = pytest.importorskip("torch")

B, C4, A, S = 8, 4, 9, 6
NEW, GENERAL = "k_prepare1", "k_prepare"
KERNELS = {"prepare1_k1": (1, None, NEW), "general_k1": (1, "MZ_PREPARE_GENERAL", GENERAL), "general_k5": (5, None, GENERAL)}
_PORT = {}


def _inputs(seeding):
    from mazero_amd.synthetic import make_search_inputs

    inp = make_search_inputs(np.random.default_rng(4100), B, A, S)
    return replace(inp, seed=100000) if seeding == "beyond_table" else inp


def _port(port_lib, inp, K, **kw):
    """The CPU port's search of `inp` (computed once per input seed and K, never modified)."""
    from mazero_amd.synthetic import run_search

    key = (inp.seed, K, inp.B, tuple(sorted(kw.items())))
    if key not in _PORT:
        _PORT[key] = run_search(make_tb(port_lib, inp, K, {}, **kw), inp, K, per_sim=False)
    return _PORT[key]


def _rows_equal(out, full, lo, hi, where):
    for k, v in full.items():
        want = v[:, lo:hi] if k in ("sel_idx", "sel_act") else v[lo:hi]
        got = np.asarray(out[k])
        if want.ndim == 2 and k.startswith("sampled_"):  # (padded to each search's own largest degree)
            w = max(want.shape[1], got.shape[1])
            want = np.pad(want, ((0, 0), (0, w - want.shape[1])))
            got = np.pad(got, ((0, 0), (0, w - got.shape[1])))
        assert got.shape == want.shape and np.array_equal(got.view(np.uint8), want.astype(got.dtype).view(np.uint8)), \
            f"{where}: {k}"


def _search(tb, sub, K, first):
    if K == 1 and first == "prepare_select":
        out, _ = round1._drive(tb, sub, ["fused"] * sub.S, first="prepare_select")
    else:
        out, _ = run_fused(tb, to_device(sub), K, {})
    tb.synchronize()  # (raises on a non-zero error word)
    return out


# ---- kernel level: one handle, three shard positions ----
@pytest.mark.gpu
@pytest.mark.parametrize("seeding", ["table", "chain", "beyond_table"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_one_handle_follows_the_shard(gpu_lib, port_lib, kernel, seeding, monkeypatch):  # noqa: F811
    from mazero_amd.shard import slice_inputs

    K, env, name = KERNELS[kernel]
    inp = _inputs(seeding)
    full = _port(port_lib, inp, K)
    if seeding == "chain":
        monkeypatch.setenv("MZ_NO_SEED_TABLE", "1")  # (read at mz_create)
    if env:
        monkeypatch.setenv(env, "1")  # (read at mz_create)
    tb = make_tb(gpu_lib, slice_inputs(inp, 0, C4), K, {})
    tb3 = make_tb(gpu_lib, slice_inputs(inp, 0, C4), K, {}, root_offset=3)
    if env:
        monkeypatch.delenv(env)
    assert tb.prepare_kernel() == name and tb3.prepare_kernel() == name
    assert tb.root_offset == 0 and tb3.root_offset == 3
    for n, lo in enumerate((0, 4, 2)):
        if n:
            tb.set_root_offset(lo)
        assert tb.root_offset == lo
        tb.reseed(inp.seed)
        out = _search(tb, slice_inputs(inp, lo, lo + C4), K, "prepare" if n == 0 else "prepare_select")
        _rows_equal(out, full, lo, lo + C4, f"rows [{lo}:{lo + C4}]")
    # a handle created at another offset, moved to 0: the offset-0 handle
    out = _search(tb3, slice_inputs(inp, 3, 3 + C4), K, "prepare")
    _rows_equal(out, full, 3, 3 + C4, "created at 3")
    tb3.set_root_offset(0)
    assert tb3.root_offset == 0
    tb3.reseed(inp.seed)
    out = _search(tb3, slice_inputs(inp, 0, C4), K, "prepare_select")
    _rows_equal(out, full, 0, C4, "created at 3, moved to 0")


# ---- an offset that takes only some of a handle's trees past the seeding table: the check is per tree ----
@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 5])
def test_offset_across_the_end_of_the_table(gpu_lib, port_lib, K):  # noqa: F811
    from mazero_amd.synthetic import make_search_inputs

    # the table holds at least 256 * 2333 + 4096 seed values (it may have grown: then every tree reads it);
    # at random_seed 255 trees 0 and 1 are its last two rows and trees 2 and 3 lie past it
    lo = 2333 + 4096 - 2
    inp = replace(make_search_inputs(np.random.default_rng(4200), C4, A, S), seed=255)
    exp = _port(port_lib, inp, K, root_offset=lo)
    tb = make_tb(gpu_lib, inp, K, {})
    assert tb.prepare_kernel() == (NEW if K == 1 else GENERAL)
    tb.set_root_offset(lo)
    out = _search(tb, inp, K, "prepare_select")
    _rows_equal(out, exp, 0, C4, f"offset {lo}")


# ---- the entry points' argument checks; what the call leaves alone ----
@pytest.mark.gpu
def test_root_offset_arguments(gpu_lib, port_lib):  # noqa: F811
    from mazero_amd._capi import MZ_ERR_ARG
    from mazero_amd.shard import slice_inputs

    inp = slice_inputs(_inputs("table"), 0, C4)
    tb = make_tb(gpu_lib, inp, 5, {})
    lib, h = tb._lib, tb._h
    _search(tb, inp, 5, "prepare")
    values = tb.get_roots_values()
    tb.set_active_roots(3)
    int_max = (1 << 31) - 1
    got = C.c_int(-5)
    for bad in (-1, -int_max - 1, int_max, int_max - C4 + 1):
        assert lib.mz_set_root_offset(h, bad) == MZ_ERR_ARG, bad
        assert lib.mz_get_root_offset(h, C.byref(got)) == 0 and got.value == 0
    with pytest.raises(ValueError):
        tb.set_root_offset(-1)
    assert lib.mz_set_root_offset(None, 0) == MZ_ERR_ARG and lib.mz_get_root_offset(h, None) == MZ_ERR_ARG
    assert lib.mz_get_root_offset(None, C.byref(got)) == MZ_ERR_ARG
    for ok in (int_max - C4, 7, 0, 2):  # (root_offset + root_num == INT32_MAX is the last one taken)
        assert lib.mz_set_root_offset(h, ok) == 0
        assert lib.mz_get_root_offset(h, C.byref(got)) == 0 and got.value == ok and tb.root_offset == ok
    # the active-root count and the finished search's readback are untouched
    assert tb.active_roots == 3 and _same(tb.get_roots_values(), values[:3])
    tb.set_active_roots(C4)
    assert _same(tb.get_roots_values(), values)
    # ... and so is the seed: the next search is the one at offset 2
    full = _port(port_lib, _inputs("table"), 5)
    out = _search(tb, slice_inputs(_inputs("table"), 2, 2 + C4), 5, "prepare")
    _rows_equal(out, full, 2, 2 + C4, "after the argument checks")


# ---- driver level: three emulated ranks on one capacity handle ----
SN, SA, SS = 3, 9, 8


def _shards(active):
    from mazero_amd.shard import active_shard, shard_bounds

    return [active_shard(active, *shard_bounds(TOTAL, WORLD, r)) for r in range(WORLD)]


def _slice_out(out, lo, hi):
    from mazero_amd.nets import NetworkOutput

    return NetworkOutput(out.hidden_state[lo:hi], out.reward[lo:hi], out.value[lo:hi], out.policy_logits[lo:hi])


@pytest.mark.gpu
@pytest.mark.parametrize("cur", [0, 1])
@pytest.mark.parametrize("K", [1, 5])
def test_sharded_capacity_search_is_the_plain_search(K, cur):
    from mazero_amd.mcts_sampled import SampledMCTS

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, K)
    net_sh, net_pl = (RowwiseNet(SN, SA, seed=3).to(dev).eval() for _ in range(2))
    rs_pl = np.random.RandomState(11)
    rs_sh = [np.random.RandomState(11) for _ in range(WORLD)]
    counts, offsets = [], set()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for step, active in enumerate(ACTIVES + ACTIVES):  # twice: each loop searches 20 times
            n = len(active)
            factor = np.random.RandomState(50 + step).randint(0, SA, (n, SN)).astype(np.int32) if cur else None
            out, legal = rowwise_batch(net_pl, n, 900 + step, dev)
            plain = SampledMCTS(cfg, rs_pl).batch_search(net_pl, out, cur, factor, SN, legal, device=dev, add_noise=True)
            for r, (p_lo, p_hi, _) in enumerate(_shards(active)):
                drv = SampledMCTS(cfg, rs_sh[r], root_capacity=C4, root_shard=(p_lo, p_hi, n), device_root_offset=True)
                if p_lo == p_hi:
                    drv.skip_search()
                else:
                    got = drv.batch_search(net_sh, _slice_out(out, p_lo, p_hi), cur,
                                           None if factor is None else factor[p_lo:p_hi], SN, legal[p_lo:p_hi],
                                           device=dev, add_noise=True)
                    for name in got._fields:
                        assert _same(getattr(got, name), getattr(plain, name)[p_lo:p_hi]), \
                            f"step {step} rank {r} rows [{p_lo}:{p_hi}) of {n}: {name}"
                    offsets.add(p_lo)
                assert rs_sh[r].get_state()[2] == rs_pl.get_state()[2], (step, r)
                assert np.array_equal(rs_sh[r].get_state()[1], rs_pl.get_state()[1]), (step, r)
            loops = _loops_of(net_sh)
            counts.append((len(loops), len(_trees_of(loops)), loops[0].runs, bool(loops[0].graph)))
    # one handle and one loop from the first search on, every shard position; recorded once, then replayed
    assert all(c[:2] == (1, 1) for c in counts), counts
    assert [c[2] for c in counts] == [3, 6, 7, 10, 13, 16, 17, 20]
    assert all(c[3] for c in counts), counts
    lp = _loops_of(net_sh)[0]
    assert lp.B == C4 and lp.tb.root_num == C4 and isinstance(lp.graph, torch.cuda.CUDAGraph)
    assert offsets == {0, 3, 5, 4, 8}


@pytest.mark.gpu
def test_an_empty_shard_is_refused_by_the_search():
    from mazero_amd.mcts_sampled import SampledMCTS

    dev = torch.device("cuda", 0)
    net = RowwiseNet(SN, SA, seed=3).to(dev).eval()
    out, legal = rowwise_batch(net, 2, 1, dev)
    drv = SampledMCTS(rowwise_config(SA, SS, 1), np.random.RandomState(1), root_capacity=C4, root_shard=(1, 1, 2),
                      device_root_offset=True)
    with pytest.raises(ValueError, match="skip_search"):
        drv.batch_search(net, _slice_out(out, 1, 1), 0, None, SN, legal[1:1], device=dev, add_noise=True)
    assert not _loops_of(net)


# ---- worker level: SelfPlayShard(shard_active=True), the device consumers ----
@pytest.mark.gpu
def test_selfplay_shards_follow_the_active_set():
    from mazero_amd.shard import shard_bounds
    from mazero_amd.workers import SelfPlayShard

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, 3)

    def rows(t):
        rng = np.random.default_rng(600 + t)
        obs = rng.standard_normal((TOTAL, SN, HID)).astype(np.float32)
        legal = (rng.random((TOTAL, SN, SA)) > 0.2).astype(np.int64)
        legal[..., 1] = 1
        return obs, legal

    def eps(t, n):
        rng = np.random.default_rng(700 + t)
        return rng.random((SN, n)).astype(np.float32), rng.random((SN, n))

    class Counting(RowwiseNet):
        calls = 0

        def initial_inference(self, obs):
            self.calls += 1
            return super().initial_inference(obs)

    net_solo = RowwiseNet(SN, SA, seed=8).to(dev).eval()
    net = Counting(SN, SA, seed=8).to(dev).eval()
    solo = SelfPlayShard(net_solo, cfg, TOTAL, SN, seed=23, rank=0, world=1, device=dev)
    ranks = [SelfPlayShard(net, cfg, TOTAL, SN, seed=23, rank=r, world=WORLD, shard_active=True, device=dev)
             for r in range(WORLD)]
    idle = 0
    for t, active in enumerate(ACTIVES):
        obs, legal = rows(t)
        u = eps(t, len(active))
        a = np.asarray(active)
        ref = solo.step(t, torch.from_numpy(obs[a]).to(dev), legal[a], greedy_epsilon=0.25, eps_uniforms=u, active=active)
        recs = []
        for sp in ranks:
            lo, hi = shard_bounds(TOTAL, WORLD, sp.rank)
            mine = np.asarray([e for e in active if lo <= e < hi], dtype=np.int64)
            loops = _loops_of(net)
            before = (net.calls, [lp.runs for lp in loops], [lp.tb.root_offset for lp in loops])
            recs.append(sp.step(t, torch.from_numpy(obs[mine]).to(dev), legal[mine], greedy_epsilon=0.25,
                                eps_uniforms=u, active=active))
            assert recs[-1].actions.shape == (len(mine), SN)
            if not len(mine):  # nothing ran: no model call, no search, the handle as it was
                loops = _loops_of(net)
                assert before == (net.calls, [lp.runs for lp in loops], [lp.tb.root_offset for lp in loops])
                idle += 1
        for f in FIELDS:
            cat = np.concatenate([getattr(r, f) for r in recs])
            assert _same(cat, getattr(ref, f)), f"step {t} field {f}"
        for sp in ranks:
            assert np.array_equal(sp.np_random.get_state()[1], solo.np_random.get_state()[1]), (t, sp.rank)
            assert sp.np_random.get_state()[2] == solo.np_random.get_state()[2], (t, sp.rank)
    assert idle == 2
    loops = _loops_of(net)
    assert len(_trees_of(loops)) == 1 and len(loops) == SN  # one handle, one loop per agent, for all three ranks
    assert all(lp.B == C4 for lp in loops)
