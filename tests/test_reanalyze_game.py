"""consume.reanalyze_game / consume.write_game: the full-game reanalysis of
ReanalyzeWorker.make_renalyze_update after its initial inference (reanalyze_worker.py:507-607).

The reference here is a numpy restatement of :533-596, written below in the project's own words and
driven by the oracle driver (oracle/driver.py on the CPU port) from the same RandomState.  The searches
run on `RowwiseNet` (tests/test_root_capacity.py), whose outputs do not depend on the batch's row count, so
a game of T steps searched on a driver with root_capacity = 32 must give the oracle's T-root results.

The host fallback (a root whose visits all lie on illegal actions, :568-570) is tested without a GPU, on
a stub search.
"""
from __future__ import annotations

import types

import numpy as np
import pytest
import torch

from test_root_capacity import RowwiseNet, _loops_of, _same, _trees_of, rowwise_batch, rowwise_config

N, A, S, K, CAP = 3, 9, 8, 5, 32


def numpy_game_reanalysis(search, np_random, legal, T, num_agents):
    """What make_renalyze_update computes after its initial inference (reanalyze_worker.py:533-596), for
    searches of at least one simulation (every root then has visits).  `search(agent, factor)` ->
    (value [T], marginal visits [T, 1, A]) is the agent turn's batch_search.  Per agent turn: the first
    argmax of visits * legal; a root with no visit on a legal action draws a legal action from np_random
    instead (root order; 0 when none is legal); the joint probability is the float64 product, in agent
    order, of each agent's visit share at its action.  Returns (actions int32 [T, N], probs float32
    [T, 1], root values float32 [T, 1])."""
    chosen = np.zeros((T, num_agents), dtype=np.int32)
    joint = np.ones(T, dtype=np.float64)
    root_values = None
    rows = np.arange(T)
    for k in range(num_agents):
        value, marginal = search(k, chosen[:, :k].copy() if k else None)
        if k == 0:
            root_values = np.asarray(value, dtype=np.float32).reshape(T, 1)
        visits = marginal[:, 0, :].astype(np.int64)
        assert (visits.sum(axis=1) > 0).all()
        masked = visits * legal[:, k, :]
        pick = masked.argmax(axis=1)
        for i in np.flatnonzero(masked.sum(axis=1) <= 0):
            options = np.flatnonzero(legal[i, k, :] == 1)
            pick[i] = np_random.choice(options) if options.size else 0
        chosen[:, k] = pick
        joint = joint * (visits[rows, pick] / visits.sum(axis=1))
    return chosen, joint.astype(np.float32).reshape(T, 1), root_values


# ------------------------------------------------------------------------------------------ CPU
class _StubSearch:
    """batch_search_device of a driver whose every search puts all visits on action 0; records the
    generator's position at each search."""

    def __init__(self, np_random, T, action_space):
        self.config = types.SimpleNamespace(num_simulations=4, action_space_size=action_space)
        self.np_random, self.T, self.A = np_random, T, action_space
        self.calls = []  # (agent, factor rows seen, a probe of the generator state)

    def batch_search_device(self, model, network_output, agent, factor, num_agents, legal, device, add_noise,
                            sampled_tau):
        assert add_noise is True and sampled_tau == 1.0
        self.calls.append((agent, None if factor is None else factor.clone().numpy(),
                           self.np_random.get_state()[2]))
        mv = torch.zeros(self.T, 1, self.A, dtype=torch.int32)
        mv[:, 0, 0] = 4
        return types.SimpleNamespace(value=torch.arange(self.T, dtype=torch.float32) + agent,
                                     marginal_visit_count=mv, tree=None)


def _host_marginal_policy(out, mode, action, prob, legal=None, entropy=None):
    """include/mzconsume.h mz_marginal_policy, modes 0 and 2, on host tensors."""
    from mazero_amd._capi import MZ_MARGINAL_ARGMAX_LEGAL, MZ_MARGINAL_GIVEN

    m = out.marginal_visit_count[:, 0, :].to(torch.int64)
    if mode == MZ_MARGINAL_ARGMAX_LEGAL:
        assert prob is None and entropy is None
        masked = m * legal.to(torch.int64)
        action.copy_(torch.where(masked.sum(1) > 0, masked.argmax(1), torch.tensor(-1)).to(torch.int32))
    else:
        assert mode == MZ_MARGINAL_GIVEN
        prob *= m[torch.arange(m.shape[0]), action.long()].double() / m.sum(1).double()


def test_host_fallback_draws_in_root_order_before_the_next_search(monkeypatch):
    from mazero_amd import consume

    T, A_ = 6, 5
    legal = np.ones((T, 2, A_), np.int64)
    legal[:, :, 0] = 0  # every visit (action 0) is illegal for both agents ...
    legal[1, 0, :] = 0  # ... and root 1 has no legal action for agent 0: action 0, no draw
    legal[4, 0, 0] = 1  # root 4 keeps its argmax for agent 0: no draw
    legal[2, 0, 3] = 0
    rs, rs_ref = np.random.RandomState(7), np.random.RandomState(7)
    stub = _StubSearch(rs, T, A_)
    monkeypatch.setattr(consume, "marginal_policy", _host_marginal_policy)
    out = types.SimpleNamespace(hidden_state=torch.zeros(T, 4), value=np.arange(T, dtype=np.float32).reshape(T, 1))
    res = consume.reanalyze_game(stub, None, out, legal)

    expected = np.zeros((T, 2), np.int32)
    positions = []
    for k in range(2):
        positions.append(rs_ref.get_state()[2])
        for i in range(T):  # root order
            if legal[i, k, 0]:
                continue
            idx = np.where(legal[i, k, :] == 1)[0]
            expected[i, k] = rs_ref.choice(idx) if idx.size else 0
    np.testing.assert_array_equal(res.actions.numpy(), expected)
    assert rs.randint(1 << 30) == rs_ref.randint(1 << 30)
    # agent 1's search ran after agent 0's draws and saw the resolved actions as its factor
    assert [c[0] for c in stub.calls] == [0, 1]
    assert [c[2] for c in stub.calls] == positions and positions[1] != positions[0]
    assert stub.calls[0][1] is None
    np.testing.assert_array_equal(stub.calls[1][1][:, 0], expected[:, 0])
    # the chosen actions carry no visits: probability 0, except root 4's kept argmax for agent 0 times
    # agent 1's unvisited draw
    assert res.policy_probs.dtype == torch.float32 and res.policy_probs.shape == (T, 1)
    assert (res.policy_probs.numpy() == 0).all()
    assert _same(res.root_values.numpy(), np.arange(T, dtype=np.float32).reshape(T, 1))
    assert res.pred_values.shape == (T, 1)


def test_reanalyze_game_needs_a_simulation():
    from mazero_amd import consume

    stub = types.SimpleNamespace(config=types.SimpleNamespace(num_simulations=0))
    with pytest.raises(ValueError, match="num_simulations"):
        consume.reanalyze_game(stub, None, None, None)


def test_write_game_fills_the_lists():
    """reanalyze_worker.py:598-607 on a plain object."""
    from mazero_amd.consume import GameReanalysis, write_game

    T = 4
    actions = np.arange(T * N, dtype=np.int32).reshape(T, N)
    probs = np.linspace(0.1, 0.4, T, dtype=np.float32).reshape(T, 1)
    values = np.linspace(-1, 1, T, dtype=np.float32).reshape(T, 1)
    pred = np.linspace(2, 3, T, dtype=np.float32)
    for pv in (pred.reshape(T, 1), pred):
        res = GameReanalysis(*(torch.from_numpy(x) for x in (actions, probs, values, pv)))
        game = write_game(types.SimpleNamespace(), res, model_index=12)
        assert np.array_equal(game.model_indices, np.array([12] * T))
        assert len(game.sampled_actions) == T and all(a.shape == (1, N) for a in game.sampled_actions)
        assert _same(np.concatenate(game.sampled_actions), actions)
        assert all(p.shape == (1,) for p in game.sampled_policies) and _same(np.stack(game.sampled_policies), probs)
        assert all(m.dtype == np.bool_ and m.shape == (1,) and m[0] for m in game.sampled_padding_masks)
        assert len(game.sampled_padding_masks) == T
        assert all(q.shape == (1,) for q in game.sampled_qvalues) and _same(np.stack(game.sampled_qvalues), values)
        assert game.root_values == [v[0] for v in values]
        assert game.pred_values == (pred.tolist() if pv.ndim == 1 else [v for v in pred])
    kept = types.SimpleNamespace(pred_values="kept")
    write_game(kept, GameReanalysis(*(torch.from_numpy(x) for x in (actions, probs, values)), None), 0)
    assert kept.pred_values == "kept"  # (another value shape: the reference leaves them, :608-609)


# ------------------------------------------------------------------------------------------ GPU
def _visits_onto_an_illegal_action(marginal, legal_rows):
    """A copy of the marginal visits [T, 1, A] in which every third root that has an illegal action carries
    all its visits on its first illegal one, and the roots so changed: what forces the np_random fallback
    (the search itself never visits an illegal action)."""
    m = np.array(marginal, copy=True)
    forced = [i for i in range(0, m.shape[0], 3) if (legal_rows[i] == 0).any()]
    for i in forced:
        total = m[i, 0].sum()
        m[i, 0] = 0
        m[i, 0, np.flatnonzero(legal_rows[i] == 0)[0]] = total
    return m, forced


@pytest.mark.gpu
def test_reanalyze_game_matches_the_numpy_restatement(port_lib):
    """T = 1, 7, 32 on one driver with root_capacity = 32: actions, float32 probabilities, root values
    and the final generator state equal the restatement's over the oracle driver; one set of loops
    serves all three lengths.  Both sides see the same doctored visits (every third root's moved onto an
    illegal action), so the device path's fallback runs: -1 from the kernel, the host draws in root
    order, the resolved column back on the device as the next agent's factor."""
    from driver import OracleSampledMCTS
    from mazero_amd.consume import reanalyze_game
    from mazero_amd.mcts_sampled import SampledMCTS

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(A, S, K)
    net = RowwiseNet(N, A, seed=6).to(dev).eval()
    rs_o, rs_d = np.random.RandomState(31), np.random.RandomState(31)
    oracle = OracleSampledMCTS(cfg, rs_o, port_lib)
    state = {"legal": None, "forced": 0}

    class Doctored(SampledMCTS):
        def batch_search_device(self, model, network_output, agent, *a, **kw):
            out = super().batch_search_device(model, network_output, agent, *a, **kw)
            m, forced = _visits_onto_an_illegal_action(out.marginal_visit_count.cpu().numpy(),
                                                       state["legal"][:, agent, :])
            out.marginal_visit_count.copy_(torch.from_numpy(m).to(dev))
            state["forced"] += len(forced)
            return out

    drv = Doctored(cfg, rs_d, root_capacity=CAP)
    for T in (1, 7, 32):
        out, legal = rowwise_batch(net, T, 500 + T, dev, legal_zero_frac=0.45)
        state["legal"] = legal

        def search(k, factor):
            o = oracle.batch_search(net, out, k, factor, N, legal, device=dev, add_noise=True, sampled_tau=1.0)
            return o["value"], _visits_onto_an_illegal_action(o["marginal_visit_count"], legal[:, k, :])[0]

        before = rs_o.get_state()[2]
        exp_a, exp_p, exp_v = numpy_game_reanalysis(search, rs_o, legal, T, N)
        got = reanalyze_game(drv, net, out, legal, device=dev)
        assert got.actions.dtype == torch.int32 and got.policy_probs.dtype == torch.float32
        np.testing.assert_array_equal(got.actions.cpu().numpy(), exp_a)
        assert _same(got.policy_probs.cpu().numpy(), exp_p)
        assert _same(got.root_values.cpu().numpy(), exp_v)
        assert _same(got.pred_values.cpu().numpy(), np.asarray(out.value))
        if T > 1:  # forced roots took the fallback: a legal action without visits, probability 0
            assert (exp_p == 0).any() and before != rs_o.get_state()[2]
    assert state["forced"] >= 10  # the fallback ran on the device path, many times
    assert rs_o.randint(1 << 30) == rs_d.randint(1 << 30)
    loops = _loops_of(net)
    assert len(loops) == N and len(_trees_of(loops)) == 1  # one loop per agent turn, one handle
    assert all(lp.B == CAP and lp.runs == 3 for lp in loops)
