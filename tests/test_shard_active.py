"""Sharded ranks following a varying active set, on the CPU: shard.active_shard, workers.gather_active,
SelfPlayShard(shard_active=True).step(active=...) on explicit ranks with the oracle driver over the CPU
port and the restated host consumers injected (as tests/test_workers.py injects them), the opt-ins
(SampledMCTS device_root_offset, _Shard shard_active) with what stays refused without them, and the
ctypes signatures of mz_set_root_offset / mz_get_root_offset against the header.

The worker harness runs on `RowwiseNet` (tests/test_root_capacity.py): row i of its outputs does not
depend on how many rows the batch has, so a rank's two rows and the single rank's seven are computed
alike and the records can be compared bit for bit.
"""
from __future__ import annotations

import ctypes as C
import itertools
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT
from test_root_capacity import HID, RowwiseNet, rowwise_config

DRIVER_HEADER = os.path.join(ROOT, "include", "mzdriver.h")

TOTAL, WORLD, N, A, S = 12, 3, 3, 9, 6
ACTIVES = [list(range(TOTAL)), [0, 1, 2, 5, 6, 10, 11], [5], list(range(TOTAL))]
FIELDS = ("actions", "prob_action", "root_value", "count_entropy", "visit_entropy")


# ------------------------------------------------------------------------------------ active_shard
def test_active_shard_exhaustive():
    from mazero_amd.shard import active_shard, shard_bounds

    for total in range(1, 9):
        for world in range(1, min(4, total) + 1):
            bounds = [shard_bounds(total, world, r) for r in range(world)]
            for mask in range(1 << total):
                active = [i for i in range(total) if mask >> i & 1]
                at = 0
                for lo, hi in bounds:
                    p_lo, p_hi, n = active_shard(active, lo, hi)
                    assert n == len(active)
                    assert p_lo == at  # the positions tile [0, n) in rank order
                    assert p_lo == sum(1 for e in active if e < lo)  # the active environments on lower ranks
                    assert active[p_lo:p_hi] == [e for e in active if lo <= e < hi]  # exactly the rank's own
                    if not any(lo <= e < hi for e in active):
                        assert p_lo == p_hi
                    at = p_hi
                assert at == len(active)


def test_active_shard_takes_arrays_and_refuses_unsorted_lists():
    from mazero_amd.shard import active_shard

    assert active_shard(np.asarray([0, 1, 2, 5, 6, 10, 11]), 4, 8) == (3, 5, 7)
    assert active_shard([5], 0, 4) == (0, 0, 1) and active_shard([5], 8, 12) == (1, 1, 1)
    for bad in ([3, 2], [1, 1]):
        with pytest.raises(ValueError, match="sorted"):
            active_shard(bad, 0, 4)


# ------------------------------------------------------------------------------------ the opt-ins
def test_flags_default_off_and_read_from_config():
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig
    from mazero_amd.workers import SelfPlayShard

    cfg = SearchConfig(action_space_size=A)
    assert SampledMCTS(cfg, np.random.RandomState(0)).device_root_offset is False
    assert SelfPlayShard(None, cfg, 8, 2, seed=0, rank=1, world=2).shard_active is False
    cfg.device_root_offset = True
    cfg.shard_active = True
    assert SampledMCTS(cfg, np.random.RandomState(0)).device_root_offset is True
    assert SampledMCTS(cfg, np.random.RandomState(0), device_root_offset=False).device_root_offset is False
    assert SelfPlayShard(None, cfg, 8, 2, seed=0, rank=1, world=2).shard_active is True
    assert SelfPlayShard(None, cfg, 8, 2, seed=0, rank=1, world=2, shard_active=False).shard_active is False


@pytest.mark.parametrize("flag", [False, None])
def test_refusals_stay_with_the_flags_off(flag):
    """What tests/test_root_capacity.py pins, with the new keywords spelled False or left None."""
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig
    from mazero_amd.workers import SelfPlayShard

    cfg = SearchConfig(action_space_size=A)
    with pytest.raises(ValueError, match="root_shard"):
        SampledMCTS(cfg, np.random.RandomState(0), root_capacity=8, root_shard=(0, 4, 8), device_root_offset=flag)
    with pytest.raises(ValueError, match="bad root shard"):  # an empty shard
        SampledMCTS(cfg, np.random.RandomState(0), root_shard=(4, 4, 8), device_root_offset=flag)
    sp = SelfPlayShard(None, cfg, 8, 2, seed=0, rank=1, world=2, shard_active=flag)
    with pytest.raises(NotImplementedError, match="root offset"):
        sp.step(0, None, None, active=[4, 5])
    sharded = SelfPlayShard(None, cfg, 8, 2, seed=0, rank=1, world=2, root_capacity=8, shard_active=flag)
    with pytest.raises(ValueError, match="root_shard"):
        sharded.make_mcts(sharded.config, sharded.np_random, sharded._search_shard())


def test_device_root_offset_accepts_capacity_with_a_shard():
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=A)
    m = SampledMCTS(cfg, np.random.RandomState(0), root_capacity=4, root_shard=(3, 5, 7), device_root_offset=True)
    assert m.root_capacity == 4 and m.root_shard == (3, 5, 7)
    m = SampledMCTS(cfg, np.random.RandomState(0), root_capacity=4, root_shard=(3, 7, 7), device_root_offset=True)
    assert m.root_shard == (3, 7, 7)  # hi - lo == C
    with pytest.raises(ValueError, match="root_capacity"):  # a shard wider than the capacity
        SampledMCTS(cfg, np.random.RandomState(0), root_capacity=4, root_shard=(0, 5, 8), device_root_offset=True)
    for bad in ((5, 4, 8), (-1, 2, 8), (0, 9, 8)):
        with pytest.raises(ValueError, match="bad root shard"):
            SampledMCTS(cfg, np.random.RandomState(0), root_shard=bad, device_root_offset=True)


def test_device_root_offset_needs_the_entry_point(port_lib):
    from mazero_amd.cytree import Tree_batch
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=A)
    with pytest.raises(RuntimeError, match="mz_set_root_offset"):
        SampledMCTS(cfg, np.random.RandomState(0), lib=port_lib, device_root_offset=True)
    assert SampledMCTS(cfg, np.random.RandomState(0), lib=port_lib).device_root_offset is False
    tb = Tree_batch(4, 1, 3, 1, 2, 0.01, 0, 0.75, 0.8, root_offset=3, lib=port_lib)
    assert tb.root_offset == 3  # (the constructor's, on a library without the getter)
    with pytest.raises(RuntimeError, match="mz_set_root_offset"):
        tb.set_root_offset(0)


def test_skip_search_consumes_one_search_and_an_empty_shard_draws_for_the_whole_batch():
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=A)
    rs, ref = np.random.RandomState(3), np.random.RandomState(3)
    m = SampledMCTS(cfg, rs, root_shard=(2, 2, 7), device_root_offset=True)
    m.skip_search()
    ref.dirichlet([cfg.root_dirichlet_alpha] * A, 7)
    ref.choice(256)
    assert m.draw_root_uniforms(0).shape == (0,)
    ref.random(7)
    assert rs.randint(1 << 30) == ref.randint(1 << 30)
    with pytest.raises(ValueError, match="not empty"):
        SampledMCTS(cfg, rs, root_shard=(2, 3, 7), device_root_offset=True).skip_search()


def test_ctypes_signatures_match_header():
    from mazero_amd import _capi

    txt = open(DRIVER_HEADER).read()
    ctype = {"mz_batch *": C.c_void_p, "int": C.c_int, "int *": C.POINTER(C.c_int)}
    want = {"mz_set_root_offset": ["mz_batch *", "int"], "mz_get_root_offset": ["mz_batch *", "int *"]}
    for name, types in want.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", txt, re.M)
        assert m, f"{name} is not declared"
        declared = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            declared.append(re.match(r"(.*?)(\w+)$", arg).group(1).strip())
        assert declared == types, name
        res, args = _capi.DRIVER_SIGNATURES[name]
        assert res is C.c_int and args == [ctype[t] for t in declared], name
        assert name in _capi.DRIVER_EXPORTS


# ------------------------------------------------------------------------------------ the worker harness
def _rows(t):
    rng = np.random.default_rng(1000 + t)
    obs = rng.standard_normal((TOTAL, N, HID)).astype(np.float32)
    legal = (rng.random((TOTAL, N, A)) > 0.3).astype(np.int64)
    legal[..., 1] = 1
    return obs, legal


def _eps(t, n):
    rng = np.random.default_rng(2000 + t)
    return rng.random((N, n)).astype(np.float32), rng.random((N, n))


@pytest.mark.parametrize("K", [1, 5])
def test_sharded_active_steps_are_the_single_rank_steps(port_lib, K):
    """Three explicit ranks of 12 environments against the single rank's step(active=...), over a step
    sequence in which the active set shrinks, leaves two ranks empty, and grows back: the ranks' records,
    concatenated, equal the single rank's field by field, bit for bit, and all four generators are in the
    same state after every step."""
    import consume as oracle_consume
    import driver as oracle_driver
    from mazero_amd.shard import shard_bounds
    from mazero_amd.workers import SelfPlayShard

    torch.set_num_threads(1)
    cfg = rowwise_config(A, S, K)
    net = RowwiseNet(N, A, seed=4).eval()

    def make_mcts(config, rs, shard):
        return oracle_driver.OracleSampledMCTS(config, rs, port_lib, root_shard=shard)

    def decide(mcts, model, net_out, n, legal, *, temperature, sampled_tau, greedy_epsilon, eps_uniforms, device):
        u_eps, u_cat = eps_uniforms
        return oracle_consume.selfplay_step(mcts, model, net_out, n, legal, temperature, sampled_tau, greedy_epsilon,
                                            mcts.np_random, u_eps, u_cat, device, root_shard=mcts.root_shard)

    kw = dict(seed=11, make_mcts=make_mcts, decide=decide)
    solo = SelfPlayShard(net, cfg, TOTAL, N, rank=0, world=1, **kw)
    ranks = [SelfPlayShard(net, cfg, TOTAL, N, rank=r, world=WORLD, shard_active=True, **kw) for r in range(WORLD)]
    assert [(sp.lo, sp.hi) for sp in ranks] == [shard_bounds(TOTAL, WORLD, r) for r in range(WORLD)]
    empty_steps = 0
    for t, active in enumerate(ACTIVES):
        obs, legal = _rows(t)
        u = _eps(t, len(active))
        a = np.asarray(active)
        ref = solo.step(t, torch.from_numpy(obs[a]), legal[a], greedy_epsilon=0.25, eps_uniforms=u, active=active)
        recs = []
        for sp in ranks:
            mine = np.asarray([e for e in active if sp.lo <= e < sp.hi], dtype=np.int64)
            rec = sp.step(t, torch.from_numpy(obs[mine]), legal[mine], greedy_epsilon=0.25, eps_uniforms=u,
                          active=active)
            assert rec.actions.shape == (len(mine), N) and rec.lo == sp.lo
            assert np.array_equal(rec.active, a)
            empty_steps += len(mine) == 0
            recs.append(rec)
        for f in FIELDS:
            cat = np.concatenate([getattr(r, f) for r in recs])
            exp = getattr(ref, f)
            assert cat.shape == exp.shape and cat.dtype == exp.dtype, (t, f)
            assert cat.tobytes() == exp.tobytes(), f"step {t} field {f}: sharded != single rank"
        want = solo.np_random.get_state()
        for sp in ranks:
            got = sp.np_random.get_state()
            assert np.array_equal(got[1], want[1]) and got[2:] == want[2:], f"step {t}: rank {sp.rank}'s generator"
    assert empty_steps == 2  # ranks 0 and 2 at active = [5]


# ------------------------------------------------------------------------------------ gather_active
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, q):
    import sys

    sys.path[:0] = [ROOT]
    import torch.distributed as dist

    from mazero_amd.workers import gather_active

    torch.set_num_threads(1)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    local = [[5, 0, 2], [11, 6]][rank]  # each rank's running environments, in no particular order
    got = [gather_active(local).tolist(), gather_active([] if rank == 0 else [7]).tolist()]
    q.put((rank, got))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_active_over_two_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    world = 2
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0] == res[1] == [[0, 2, 5, 6, 11], [7]]


def test_gather_active_without_a_process_group():
    from mazero_amd.workers import gather_active

    got = gather_active([4, 1, 3])
    assert got.dtype == np.int64 and got.tolist() == [1, 3, 4]
