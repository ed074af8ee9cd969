"""Entries of different agents in one recorded loop: the _rows glue entry points (include/mzdriver.h:
mz_policy_glue_rows, mz_joint_action_rows, mz_policy_glue_later_rows, mz_joint_action_cached_rows),
SampledMCTS(..., mixed_agents=True) and consume.reanalyze_policy_targets_many (GPU tests need an MI355X:
`pytest -m gpu`).

Every comparison is for equality of bytes.  The kernels are compared with the scalar-agent entry points
they generalise, row by row; the searches with the consecutive `batch_search` calls on a second driver
from the same generator seed, on `RowwiseNet` (tests/test_root_capacity.py), whose row i does not depend
on the batch's row count.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
import warnings

import numpy as np
import pytest

from test_root_capacity import SA, SN, SS, RowwiseNet, _loops_of, _same, _trees_of, rowwise_batch, rowwise_config

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [5, 1, 9]
AGENTS = [[0, 1, 2], [2, 0, 1], [1, 1, 0]]  # per call: the entries' agents


@pytest.fixture(scope="module", autouse=True)
def _driver_caches_as_found():
    """The driver's loop and handle caches are process-wide and LRU-bounded, and this module makes more
    handles than the bound (every tick of the wavefront is a geometry).  The entries found are kept alive
    while the module runs and put back in their order afterwards, and this module's own go: the modules
    that follow meet the caches, and so the device buffers the cached loops hold, as if this one had not
    run."""
    from mazero_amd import mcts_sampled as ms

    with ms._LOCK:
        found = [list(ms._LOOPS.items()), list(ms._TREES.items())]
    yield
    with ms._LOCK:
        for cache, items in zip((ms._LOOPS, ms._TREES), found):
            cache.clear()
            cache.update(items)
    _handle.cache_clear()


def _state_equal(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("G,N", [(1, 1), (1, 3), (4, 3), (2, 5), (5, 2)])
def test_agent_wavefront(G, N):
    from mazero_amd.consume import agent_wavefront

    ticks = agent_wavefront(G, N)
    assert len(ticks) == G + N - 1
    when = {}
    for t, tick in enumerate(ticks):
        assert tick and [g for g, _ in tick] == sorted({g for g, _ in tick})  # ascending, no batch twice
        for g, k in tick:
            assert (g, k) not in when and k == t - g
            when[(g, k)] = t
    assert set(when) == {(g, k) for g in range(G) for k in range(N)}
    assert all(when[(g, k - 1)] < when[(g, k)] for g in range(G) for k in range(1, N))


def test_agent_wavefront_refuses_an_empty_grid():
    from mazero_amd.consume import agent_wavefront

    for G, N in ((0, 3), (2, 0)):
        with pytest.raises(ValueError, match="agent_wavefront"):
            agent_wavefront(G, N)


def test_flag_from_the_argument_and_the_config():
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=9)
    assert SampledMCTS(cfg, np.random.RandomState(0)).mixed_agents is False  # off by default
    assert SampledMCTS(cfg, np.random.RandomState(0), mixed_agents=True).mixed_agents is True
    cfg.mixed_agents = True
    assert SampledMCTS(cfg, np.random.RandomState(0)).mixed_agents is True
    assert SampledMCTS(cfg, np.random.RandomState(0), mixed_agents=False).mixed_agents is False  # the argument wins


def test_ctypes_signatures_match_header():
    from mazero_amd import _capi

    txt = open(os.path.join(ROOT, "include", "mzdriver.h")).read()
    ctype = {"mz_batch *": C.c_void_p, "const void *": C.c_void_p, "const int32_t *": C.c_void_p,
             "int32_t *": C.c_void_p, "int64_t *": C.c_void_p, "float *": C.c_void_p, "int": C.c_int,
             "int64_t": C.c_int64, "double": C.c_double}
    want = {
        "mz_policy_glue_rows": ["mz_batch *", "const void *", "int", "int64_t", "int", "const int32_t *", "double",
                                "float *", "float *"],
        "mz_joint_action_rows": ["mz_batch *", "const void *", "int", "int", "const int32_t *", "const int32_t *",
                                 "int", "const int32_t *", "int64_t *"],
        "mz_policy_glue_later_rows": ["mz_batch *", "const void *", "int", "int64_t", "int", "const int32_t *",
                                      "double", "float *", "float *", "int32_t *"],
        "mz_joint_action_cached_rows": ["mz_batch *", "const int32_t *", "int", "const int32_t *", "int",
                                        "const int32_t *", "const int32_t *", "int", "const int32_t *", "int64_t *"],
    }
    for name, types in want.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", txt, re.M)
        assert m, f"{name} is not declared"
        declared = [re.match(r"(.*?)(\w+)$", " ".join(arg.split())).group(1).strip() for arg in m.group(1).split(",")]
        assert declared == types, name
        res, args = _capi.DRIVER_SIGNATURES[name]
        assert res is C.c_int and args == [ctype[t] for t in declared], name
        assert name in _capi.DRIVER_EXPORTS


def test_mixed_agents_needs_the_rows_glue(port_lib):
    """A tree library without the _rows entry points (the oracle libraries) is refused at construction."""
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=9)
    with pytest.raises(ValueError, match="mz_policy_glue_rows"):
        SampledMCTS(cfg, np.random.RandomState(0), lib=port_lib, mixed_agents=True)
    assert SampledMCTS(cfg, np.random.RandomState(0), lib=port_lib).mixed_agents is False


def test_wavefront_targets_need_the_flag():
    from mazero_amd.consume import reanalyze_policy_targets_many
    from mazero_amd.mcts_sampled import SampledMCTS

    rs = np.random.RandomState(0)
    state = rs.get_state()[1].copy()
    with pytest.raises(ValueError, match="mixed_agents"):
        reanalyze_policy_targets_many(SampledMCTS(rowwise_config(SA, SS, 1), rs), None, [None], [None], [None])
    with pytest.raises(ValueError, match="root_shard"):
        reanalyze_policy_targets_many(SampledMCTS(rowwise_config(SA, SS, 1), rs, mixed_agents=True,
                                                  root_shard=(0, 4, 8)), None, [None], [None], [None])
    assert np.array_equal(rs.get_state()[1], state)


# ------------------------------------------------------------------------------------------ GPU: kernels
KB = 7  # rows
SENT_F, SENT_I = -7.0, -9


@functools.lru_cache(maxsize=None)
def _handle(B, A):
    from mazero_amd.cytree import Tree_batch
    from mazero_amd.mcts_sampled import ensure_half_exp

    tb = Tree_batch(B, 1, A, 1, 4, 0.01, 0, 0.75, 0.8)
    ensure_half_exp(tb._lib, torch.cuda.current_device())  # (as the search loop does)
    tb._sync_stream()
    return tb


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _tables(rng, N):
    """Agent tables [KB]: a random one that holds 0 and N - 1, and the all-equal ones of both ends."""
    if N == 1:
        return [np.zeros(KB, np.int32)]
    t = rng.integers(0, N, size=KB).astype(np.int32)
    t[rng.permutation(KB)[:2]] = (0, N - 1)
    return [t, np.zeros(KB, np.int32), np.full(KB, N - 1, np.int32)]


class _KernelCase:
    """One (N, A, dtype) case on the device: logits [KB, N, A] in rows of N * A + 3 elements (row 2 holds a
    NaN and row 4 a +inf in every agent), factor rows one column wider than needed, selection actions, a
    later pool and hidden-state indices of which two lie outside the pool."""

    def __init__(self, rng, N, A, dtype):
        from mazero_amd._capi import MZ_DT_F16, MZ_DT_F32

        dev = torch.device("cuda", 0)
        self.N, self.A, self.dt = N, A, MZ_DT_F16 if dtype == np.float16 else MZ_DT_F32
        self.tb = _handle(KB, A)
        self.wide = "_wide" if A > 64 else ""
        x = (rng.standard_normal((KB, N, A)) * 2).astype(dtype)
        x[2, :, A // 2] = np.nan
        x[4, :, A - 1] = np.inf
        self.stride = N * A + 3
        rows = np.full((KB, self.stride), 3.0, dtype)
        rows[:, : N * A] = x.reshape(KB, N * A)
        self.strided = torch.from_numpy(rows).to(dev)
        self.pred = torch.from_numpy(x).to(dev)  # contiguous [KB, N, A]
        self.fcols = max(1, N - 1) + 1
        self.factor = torch.from_numpy(rng.integers(0, A, size=(KB, self.fcols)).astype(np.int32)).to(dev)
        self.actions = torch.from_numpy(rng.integers(0, A, size=KB).astype(np.int32)).to(dev)
        self.slots = 3
        self.pool = torch.from_numpy(rng.integers(0, A, size=(self.slots, KB, N)).astype(np.int32)).to(dev)
        idx = rng.integers(0, self.slots, size=KB).astype(np.int32)
        idx[1], idx[5] = -1, self.slots
        self.idx_x = torch.from_numpy(idx).to(dev)
        self.dev = dev

    def _outs(self):
        """probs, beta [KB, A] and, between guard rows, later int32 and joint int64 [KB + 2, N]."""
        return (torch.full((KB, self.A), SENT_F, device=self.dev), torch.full((KB, self.A), SENT_F, device=self.dev),
                torch.full((KB + 2, self.N), SENT_I, dtype=torch.int32, device=self.dev),
                torch.full((KB + 2, self.N), SENT_I, dtype=torch.int64, device=self.dev))

    def run(self, agent, tau):
        """The four computations for `agent`: a table (int32 [KB] tensor: the _rows entry points) or one
        agent index (the entry points they generalise).  Returns the outputs as byte arrays per name;
        "later" / "later_only" / "joint*" with their guard rows."""
        from mazero_amd._capi import check

        lib, h, N = self.tb._lib, self.tb._h, self.N
        rows = isinstance(agent, torch.Tensor)
        a = _p(agent) if rows else int(agent)
        res = {}
        # policy glue
        probs, beta, later, joint = self._outs()
        if rows:
            check(lib, lib.mz_policy_glue_rows(h, _p(self.strided), self.dt, self.stride, N, a, tau, _p(probs),
                                               _p(beta)), "policy_glue_rows")
        else:
            check(lib, getattr(lib, "mz_policy_glue" + self.wide)(h, _p(self.strided), self.dt, self.stride,
                                                                  agent * self.A, tau, _p(probs), _p(beta)),
                  "policy_glue")
        res["probs"], res["beta"] = probs, beta
        # joint action from the leaf logits
        fn = lib.mz_joint_action_rows if rows else getattr(lib, "mz_joint_action" + self.wide)
        check(lib, fn(h, _p(self.pred), self.dt, N, a, _p(self.factor), self.fcols, _p(self.actions), _p(joint[1:])),
              "joint_action")
        res["joint"] = joint
        # policy glue with the later agents' argmax, and the argmax alone
        fn = lib.mz_policy_glue_later_rows if rows else lib.mz_policy_glue_later
        probs, beta, later, joint = self._outs()
        check(lib, fn(h, _p(self.strided), self.dt, self.stride, N, a, tau, _p(probs), _p(beta), _p(later[1:])),
              "policy_glue_later")
        res["later_probs"], res["later_beta"], res["later"] = probs, beta, later
        later_only = self._outs()[2]
        if N > 1 and (rows or agent + 1 < N):  # (the scalar call has no output to give for the last agent)
            check(lib, fn(h, _p(self.strided), self.dt, self.stride, N, a, tau, None, None, _p(later_only[1:])),
                  "policy_glue_later")
        res["later_only"] = later_only
        # joint action from the pool
        fn = lib.mz_joint_action_cached_rows if rows else lib.mz_joint_action_cached
        check(lib, fn(h, _p(self.pool), self.slots, _p(self.idx_x), N, a, _p(self.factor), self.fcols,
                      _p(self.actions), _p(joint[1:])), "joint_action_cached")
        res["joint_cached"] = joint
        return {k: v.cpu().numpy() for k, v in res.items()}


GUARDED = ("later", "later_only", "joint", "joint_cached")


def _assert_rows_equal(got, want, sel, where):
    """Rows `sel` (a bool mask over the KB rows) of every output of `got` hold the bytes of `want`'s."""
    for name in want:
        g, w = got[name], want[name]
        if name in GUARDED:
            g, w = g[1:-1], w[1:-1]
        g, w = (np.ascontiguousarray(x[sel]).view(np.uint8) for x in (g, w))
        assert np.array_equal(g, w), f"{where}: {name}"


def _assert_guards(out, where):
    for name in GUARDED:
        assert (out[name][0] == SENT_I).all() and (out[name][-1] == SENT_I).all(), f"{where}: {name} guard rows"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("A", [1, 3, 9, 64, 65, 130, 255])
def test_rows_kernels_are_the_scalar_agent_kernels(A, dtype):
    rng = np.random.default_rng(1000 * A + np.dtype(dtype).itemsize)
    dev = torch.device("cuda", 0)
    for N in (1, 2, 4):
        case = _KernelCase(rng, N, A, dtype)
        for tau in (1.0, 0.5):
            scalar = {k: case.run(k, tau) for k in range(N)}
            for table in _tables(rng, N):
                where = f"N={N} tau={tau} table={table.tolist()}"
                got = case.run(torch.from_numpy(table).to(dev), tau)
                _assert_guards(got, where)
                for k in sorted(set(table.tolist())):
                    _assert_rows_equal(got, scalar[k], table == k, f"{where} agent {k}")
                # the later columns <= the row's agent keep the sentinel (the scalar outputs above hold it there
                # too; stated on its own)
                for name in ("later", "later_only"):
                    cols = np.arange(N)[None, :] <= table[:, None]
                    assert (got[name][1:-1][cols] == SENT_I).all(), f"{where}: {name} columns <= agent"
            # a table holding -1 and N: the kernels clamp to agents 0 and N - 1 and write nothing else
            bad = _tables(rng, N)[0].copy()
            bad[0], bad[KB - 1] = -1, N
            got = case.run(torch.from_numpy(bad).to(dev), tau)
            _assert_guards(got, f"N={N} clamped")
            clamped = np.clip(bad, 0, N - 1)
            for k in sorted(set(clamped.tolist())):
                _assert_rows_equal(got, scalar[k], clamped == k, f"N={N} tau={tau} clamped table agent {k}")


@pytest.mark.gpu
def test_rows_argument_errors():
    from mazero_amd._capi import MZ_DT_F32, MZ_ERR_ARG

    N, A = 3, 9
    tb = _handle(KB, A)
    lib, h = tb._lib, tb._h
    dev = torch.device("cuda", 0)
    x = torch.zeros(KB, N * A, device=dev)
    o1, o2 = torch.zeros(KB, A, device=dev), torch.zeros(KB, A, device=dev)
    tab = torch.zeros(KB, dtype=torch.int32, device=dev)
    fac = torch.zeros(KB, N - 1, dtype=torch.int32, device=dev)
    act = torch.zeros(KB, dtype=torch.int32, device=dev)
    later = torch.zeros(KB, N, dtype=torch.int32, device=dev)
    joint = torch.zeros(KB, N, dtype=torch.int64, device=dev)
    pool = torch.zeros(2, KB, N, dtype=torch.int32, device=dev)

    def refused(rc, msg):
        assert rc == MZ_ERR_ARG and msg in lib.mz_last_error().decode(), lib.mz_last_error().decode()

    refused(lib.mz_policy_glue_rows(h, _p(x), MZ_DT_F32, N * A, N, None, 1.0, _p(o1), _p(o2)), "null row_agent")
    refused(lib.mz_policy_glue_rows(h, _p(x), MZ_DT_F32, N * A - 1, N, _p(tab), 1.0, _p(o1), _p(o2)), "every agent")
    refused(lib.mz_policy_glue_rows(h, _p(x), MZ_DT_F32, N * A, 0, _p(tab), 1.0, _p(o1), _p(o2)), "bad agent count")
    refused(lib.mz_joint_action_rows(h, _p(x), MZ_DT_F32, N, _p(tab), _p(fac), N - 2, _p(act), _p(joint)),
            "factor_cols")
    refused(lib.mz_joint_action_rows(h, _p(x), MZ_DT_F32, N, _p(tab), None, N - 1, _p(act), _p(joint)), "factor")
    refused(lib.mz_joint_action_rows(h, None, MZ_DT_F32, N, _p(tab), _p(fac), N - 1, _p(act), _p(joint)),
            "leaf policy logits")
    refused(lib.mz_policy_glue_later_rows(h, _p(x), MZ_DT_F32, N * A, N, _p(tab), 1.0, _p(o1), None, _p(later)),
            "go together")
    refused(lib.mz_policy_glue_later_rows(h, _p(x), MZ_DT_F32, N * A, N, _p(tab), 1.0, _p(o1), _p(o2), None),
            "later_out")
    refused(lib.mz_policy_glue_later_rows(h, _p(x), MZ_DT_F32, N * A, 1, _p(tab), 1.0, None, None, None),
            "no output")
    refused(lib.mz_joint_action_cached_rows(h, _p(pool), 0, _p(act), N, _p(tab), _p(fac), N - 1, _p(act), _p(joint)),
            "later-action pool")
    refused(lib.mz_joint_action_cached_rows(h, _p(pool), 2, _p(act), N, None, _p(fac), N - 1, _p(act), _p(joint)),
            "null row_agent")


# ------------------------------------------------------------------------------------------ GPU: searches
class HalfPolicyNet(RowwiseNet):
    """RowwiseNet with float16 policy logits (what a net gives under autocast)."""

    def prediction(self, h):
        policy, value = super().prediction(h)
        return policy.half(), value


class WideRowwiseNet(torch.nn.Module):
    """RowwiseNet's surface for action spaces past its hidden size: a hidden state of WH values per agent,
    row-wise arithmetic only."""

    WH = 128

    def __init__(self, num_agents: int, action_space_size: int, seed: int = 0):
        super().__init__()
        assert action_space_size <= self.WH
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.nn.Parameter(torch.randn(*s, generator=g))  # noqa: E731
        self.num_agents, self.action_space_size = num_agents, action_space_size
        self.rep_w, self.rep_b, self.dyn_w = r(self.WH), r(self.WH), r(self.WH)
        self.emb = r(action_space_size, self.WH)
        self.pol_w = r(action_space_size)

    def prediction(self, h):
        hs = h.reshape(h.shape[0], self.num_agents, self.WH)
        policy = 3.0 * hs[:, :, : self.action_space_size] * self.pol_w
        value = 2.0 * hs[:, 0, 0:1] * hs[:, self.num_agents - 1, 1:2] + hs[:, 0, 2:3]
        return policy.float(), value.float()

    def dynamics(self, h, action):
        hs = h.reshape(h.shape[0], self.num_agents, self.WH)
        nxt = torch.tanh(hs * self.dyn_w + self.emb[action.long()])
        return nxt.reshape(h.shape[0], -1), (0.5 * nxt[:, 0, 3:4] * nxt[:, self.num_agents - 1, 4:5]).float()

    def inverse_value_transform(self, x):
        return x[:, :1]

    def inverse_reward_transform(self, x):
        return x[:, :1]


def _batch(net, n, seed, dev):
    """An initial inference of n roots and their legal mask, for either net class."""
    if isinstance(net, RowwiseNet):
        return rowwise_batch(net, n, seed, dev)
    from mazero_amd.nets import NetworkOutput

    rng = np.random.default_rng(seed)
    N, A = net.num_agents, net.action_space_size
    obs = torch.from_numpy(rng.standard_normal((n, N, net.WH)).astype(np.float32)).to(dev)
    with torch.no_grad():
        h = torch.tanh(obs * net.rep_w + net.rep_b).reshape(n, -1)
        policy, value = net.prediction(h)
    legal = (rng.random((n, N, A)) >= 0.2).astype(np.int64)
    legal[..., 0] = np.where(legal.sum(-1) == 0, 1, legal[..., 0])
    return NetworkOutput(h, np.zeros((n, 1), np.float32), value.cpu().numpy(), policy.cpu().numpy()), legal


def _entries(net, step, dev, sizes=SIZES):
    outs, legals, factors = [], [], []
    for g, n in enumerate(sizes):
        out, legal = _batch(net, n, 2000 + 10 * step + g, dev)
        outs.append(out)
        legals.append(legal)
        factors.append(np.random.RandomState(70 + 10 * step + g).randint(0, net.action_space_size,
                                                                         (n, net.num_agents)).astype(np.int32))
    return outs, legals, factors


def _mixed_and_separate(K, make_net=None, A=SA, calls=AGENTS, **kw):
    """One batch_search_many call per element of `calls` (the entries' agents) on a mixed_agents driver,
    against the consecutive batch_search calls on a plain driver from the same generator seed, each with
    its own copy of the net.  Any warning is an error.  Returns the merged driver's net."""
    from mazero_amd.mcts_sampled import SampledMCTS

    make_net = make_net or (lambda: RowwiseNet(SN, A, seed=3))
    dev = torch.device("cuda", 0)
    cfg = rowwise_config(A, SS, K)
    nets = [make_net().to(dev).eval() for _ in range(2)]
    rs = [np.random.RandomState(13), np.random.RandomState(13)]
    many = SampledMCTS(cfg, rs[0], mixed_agents=True, **kw)
    plain = SampledMCTS(cfg, rs[1], **{k: v for k, v in kw.items() if k != "root_capacity"})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for step, agents in enumerate(calls):
            outs, legals, factors = _entries(nets[0], step, dev)
            fs = [f if c else None for f, c in zip(factors, agents)]
            got = many.batch_search_many(nets[0], outs, agents, fs, SN, legals, device=dev, add_noise=True,
                                         sampled_tau=1.0)
            assert len(got) == len(SIZES)
            outs, legals, factors = _entries(nets[1], step, dev)
            for g, (n, c) in enumerate(zip(SIZES, agents)):
                want = plain.batch_search(nets[1], outs[g], c, factors[g] if c else None, SN, legals[g], device=dev,
                                          add_noise=True, sampled_tau=1.0)
                assert got[g].value.shape == (n,) and len(got[g].sampled_actions) == n
                for name in want._fields:
                    assert _same(getattr(got[g], name), getattr(want, name)), f"call {step} entry {g} agent {c}: {name}"
            assert _state_equal(rs[0], rs[1]), f"call {step}: np_random"
    return nets[0]


def _the_mixed_loop(net, B=sum(SIZES)):
    """Exactly one loop and one tree handle; three searches, the second recorded and the third a replay of
    the same graph under another agent table; no memset node."""
    from mazero_amd.mcts_sampled import _LOOPS, _MIXED_AGENTS

    loops = _loops_of(net)
    assert len(loops) == 1 and len(_trees_of(loops)) == 1
    lp = loops[0]
    assert lp.mixed and lp.B == B and lp.runs == 3 and isinstance(lp.graph, torch.cuda.CUDAGraph)
    assert lp.graph_nodes[0] > 0 and lp.graph_nodes[1] == 0
    assert lp.row_agent.shape == (B,) and lp.row_agent.dtype == torch.int32 and lp.fac.shape == (B, SN - 1)
    key = [k for k, v in _LOOPS.items() if v is lp][0]
    assert key[4] == _MIXED_AGENTS
    return lp


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
def test_mixed_search_is_the_consecutive_searches(K):
    lp = _the_mixed_loop(_mixed_and_separate(K))
    # the table of the last call, [1, 1, 0] over 5 + 1 + 9 rows, and each row's factor columns with zeros behind
    agents = np.repeat(AGENTS[-1], SIZES)
    assert np.array_equal(lp.row_agent.cpu().numpy(), agents)
    fac = lp.fac.cpu().numpy()
    assert (fac[np.arange(SN - 1)[None, :] >= agents[:, None]] == 0).all()
    assert lp.later is None and lp.tb.seed_segments[0] == [0, 5, 6]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
def test_mixed_search_with_fused_transforms_and_later_action_cache(K):
    lp = _the_mixed_loop(_mixed_and_separate(K, fused_transforms=True, later_action_cache=True))
    assert lp.fused == "identity" and lp.later is not None and lp.later.shape == (SS + 1, sum(SIZES), SN)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
def test_mixed_search_on_a_capacity_loop(K):
    lp = _the_mixed_loop(_mixed_and_separate(K, root_capacity=32), B=32)
    assert lp.tb.root_num == 32 and lp.tb.active_roots == sum(SIZES)
    # rows [n, B) carry row 0's agent along with row 0's inputs
    assert (lp.row_agent[sum(SIZES):] == lp.row_agent[0]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
def test_mixed_search_through_the_wide_tiles(K):
    _the_mixed_loop(_mixed_and_separate(K, make_net=lambda: WideRowwiseNet(SN, 100, seed=3), A=100,
                                        wide_actions=True))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
def test_mixed_search_with_half_policy_logits(K):
    from mazero_amd._capi import MZ_DT_F16

    lp = _the_mixed_loop(_mixed_and_separate(K, make_net=lambda: HalfPolicyNet(SN, SA, seed=3)))
    assert lp.root_mode[0] == MZ_DT_F16


@pytest.mark.gpu
def test_mixed_search_matches_oracle_driver(port_lib):
    """One oracle search (numpy + the CPU port) per entry, each of its own agent."""
    from driver import OracleSampledMCTS
    from mazero_amd.mcts_sampled import SampledMCTS
    from test_driver import _compare_outputs

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, 3)
    net = RowwiseNet(SN, SA, seed=5).to(dev).eval()
    rs_o, rs_d = np.random.RandomState(5), np.random.RandomState(5)
    oracle = OracleSampledMCTS(cfg, rs_o, port_lib)
    drv = SampledMCTS(cfg, rs_d, mixed_agents=True)
    outs, legals, factors = _entries(net, 0, dev)
    agents = [1, 2, 0]
    factors = [f if c else None for f, c in zip(factors, agents)]
    got = drv.batch_search_many(net, outs, agents, factors, SN, legals, device=dev, add_noise=True)
    for g, c in enumerate(agents):
        exp = oracle.batch_search(net, outs[g], c, factors[g], SN, legals[g], device=dev, add_noise=True)
        _compare_outputs(got[g], exp)
    assert rs_o.randint(1 << 30) == rs_d.randint(1 << 30)
    assert _loops_of(net)[0].mixed


@pytest.mark.gpu
def test_one_agent_on_a_mixed_driver_takes_the_per_agent_loop():
    from mazero_amd.mcts_sampled import _LOOPS, _MIXED_AGENTS

    net = _mixed_and_separate(1, calls=[[1, 1, 1]])
    loops = _loops_of(net)
    assert len(loops) == 1 and not loops[0].mixed and loops[0].cur == 1 and loops[0].fac.shape == (sum(SIZES), 1)
    key = [k for k, v in _LOOPS.items() if v is loops[0]][0]
    assert key[4] == 1 and _MIXED_AGENTS not in key
    assert loops[0].joint_action.__name__ == "mz_joint_action"


@pytest.mark.gpu
def test_mixed_refusals():
    from mazero_amd.mcts_sampled import SampledMCTS

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, 1)
    net = RowwiseNet(SN, SA, seed=3).to(dev).eval()
    rs = np.random.RandomState(1)
    state = rs.get_state()[1].copy()
    outs, legals, factors = _entries(net, 0, dev)

    def refused(drv, match, *a, **k):
        with pytest.raises(ValueError, match=match):
            drv.batch_search_many(net, *a, device=dev, add_noise=True, **k)
        assert np.array_equal(rs.get_state()[1], state) and not _loops_of(net)  # before anything ran

    drv = SampledMCTS(cfg, rs, mixed_agents=True)
    refused(drv, "current_agent_idx", outs, [0, -1, 1], factors, SN, legals)
    refused(drv, "current_agent_idx", outs, [0, SN, 1], factors, SN, legals)
    refused(drv, "factor", outs, [0, 1, 2], [None, None, factors[2]], SN, legals)
    refused(drv, "factor", outs, [0, 1, 2], [None, factors[1], factors[2][:, :1]], SN, legals)
    refused(SampledMCTS(cfg, rs, mixed_agents=True, root_shard=(0, 15, 15)), "root_shard", outs, [0, 1, 2], factors,
            SN, legals)
    # without the flag the entries' agents still have to agree
    refused(SampledMCTS(cfg, rs), "current_agent_idx", outs, [0, 1, 2], factors, SN, legals)


@pytest.mark.gpu
def test_mixed_agents_on_an_oracle_library_is_refused(port_lib):
    from mazero_amd.mcts_sampled import SampledMCTS

    rs = np.random.RandomState(1)
    state = rs.get_state()[1].copy()
    with pytest.raises(ValueError, match="mz_policy_glue_rows"):
        SampledMCTS(rowwise_config(SA, SS, 1), rs, lib=port_lib, mixed_agents=True)
    assert np.array_equal(rs.get_state()[1], state)


# ------------------------------------------------------------------------------------------ GPU: the wavefront
@pytest.mark.gpu
@pytest.mark.parametrize("N,sizes", [(3, [6, 1, 4, 5]), (1, [3, 2])], ids=["4x3", "2x1"])
def test_wavefront_targets_are_the_consecutive_calls(N, sizes):
    """All seven fields of every batch and the generator state, against G consecutive
    reanalyze_policy_targets calls; twice, so that every tick's loop also replays."""
    from mazero_amd.consume import agent_wavefront, reanalyze_policy_targets, reanalyze_policy_targets_many
    from mazero_amd.mcts_sampled import SampledMCTS

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, 3)
    nets = [RowwiseNet(N, SA, seed=3).to(dev).eval() for _ in range(2)]
    rs = [np.random.RandomState(23), np.random.RandomState(23)]
    merged, plain = SampledMCTS(cfg, rs[0], mixed_agents=True), SampledMCTS(cfg, rs[1])
    rng = np.random.default_rng(6)
    masks = [[rng.integers(0, 2, size=b) for b in sizes] for _ in range(2)]
    got, states = [], []
    # (the wavefront's calls first: its ticks and the plain calls together hold more tree handles than the
    # driver's cache keeps, and an evicted handle takes its recorded loops with it)
    for step in range(2):
        batches = [rowwise_batch(nets[0], b, 700 + 10 * step + g, dev) for g, b in enumerate(sizes)]
        got.append(reanalyze_policy_targets_many(merged, nets[0], [o for o, _ in batches], [la for _, la in batches],
                                                 masks[step], dev))
        states.append(rs[0].get_state())
    loops = _loops_of(nets[0])
    ticks = agent_wavefront(len(sizes), N)
    assert len(loops) == len({sum(sizes[g] for g, _ in t) for t in ticks} if N > 1 else set(sizes))
    assert all(lp.runs >= 2 and isinstance(lp.graph, torch.cuda.CUDAGraph) for lp in loops)
    assert sum(lp.mixed for lp in loops) == sum(len(t) > 1 for t in ticks)
    for step in range(2):
        batches = [rowwise_batch(nets[1], b, 700 + 10 * step + g, dev) for g, b in enumerate(sizes)]
        for g, (out, legal) in enumerate(batches):
            want = reanalyze_policy_targets(plain, nets[1], out, legal, masks[step][g], dev)
            assert len(want) == 7
            for name, a, b in zip(want._fields, got[step][g], want):
                a, b = (torch.as_tensor(x).cpu().numpy() for x in (a, b))
                assert a.shape == b.shape and _same(a, b), f"call {step} batch {g}: {name}"
        st = rs[1].get_state()
        assert st[0] == states[step][0] and np.array_equal(st[1], states[step][1]) and st[2:] == states[step][2:], \
            f"call {step}: np_random"


@pytest.mark.gpu
def test_wavefront_needs_a_capacity_for_its_largest_tick():
    from mazero_amd.consume import reanalyze_policy_targets_many
    from mazero_amd.mcts_sampled import SampledMCTS

    dev = torch.device("cuda", 0)
    net = RowwiseNet(SN, SA, seed=3).to(dev).eval()
    rs = np.random.RandomState(2)
    state = rs.get_state()[1].copy()
    sizes = [6, 1, 4, 5]  # the largest tick: 6 + 1 + 4
    batches = [rowwise_batch(net, b, 900 + g, dev) for g, b in enumerate(sizes)]
    drv = SampledMCTS(rowwise_config(SA, SS, 1), rs, mixed_agents=True, root_capacity=10)
    with pytest.raises(ValueError, match=r"11.*10"):
        reanalyze_policy_targets_many(drv, net, [o for o, _ in batches], [la for _, la in batches],
                                      [np.ones(b) for b in sizes], dev)
    assert np.array_equal(rs.get_state()[1], state) and not _loops_of(net)
