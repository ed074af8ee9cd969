"""The expansion's distribution in registers (cdf_row), and wave 1 of k_chain3 beside it (needs an
MI355X: `pytest -m gpu`).

For up to 16 actions k_chain3's draw wave builds std::discrete_distribution's table from DPP row
broadcasts instead of LDS broadcasts, and so does wave 0's own draw when the hand-over runs out of
polls (formerly v_readlane; the whole file also passed on a build with no polls at all, where every
hand-over takes it).  17 actions and more keep the LDS form.  Wave 0 of the three-wave variant,
expand_node (k_prepare, k_tree, k_step, k_hbm), expand_joint's per-agent tables and k_chain were
routed through the same table while this was built and went back to their LDS / v_readlane forms:
the lanes were active everywhere, but the three-wave kernel and k_tree measured slower (they hide
other work behind the LDS waits, profiles/cdf_row/README.md).  Their cases stay here: they passed
on both routings and hold the table's classes for whoever routes them again.

The wave-1 cases pin what any reordering of wave 1's round 1 must keep (staging the chain's rewards
under the wait for this launch's reward and value was measured with this change and left out, see
profiles/cdf_row/README.md): chains past the 16- and 32-level reads of the recurrence, chains of
one and two nodes, the 128-node class on three and four waves, a replay out of sequence (the
reload) and a value that takes the exact selection.

Every case is bit-exact against the CPU port: per launch idx, idy, act and the gathered row; at the
end every readback and the error word.  Every handle goes through k_prepare, so the root expansion
is covered by all of them.  The shapes are the smallest that take each class of the table (4, 8,
12, 16 terms), both sides of the row limit, and each length class of wave 1's recurrence.
"""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import pytest

import test_chain3_tail as tail
from conftest import assert_same
from edge_inputs import masked as _masked
from test_gpu_parity import _joint_run, gpu_lib, make_tb, run_fused, to_device  # noqa: F401  (gpu_lib: fixture)

torch = pytest.importorskip("torch")


def _inputs(B, A, S, seed, **kw):
    from mazero_amd.synthetic import make_search_inputs

    return make_search_inputs(np.random.default_rng(seed), B, A, S, **kw)


def _check_k(gpu_lib, port_lib, inp, K, kernel, H=4):  # noqa: F811
    """One search with K draws per expansion through the fused device loop against the port."""
    from mazero_amd.synthetic import run_search

    exp = run_search(make_tb(port_lib, inp, K, {}), inp, K, {})
    exp = {k: v for k, v in exp.items() if k not in tail.PER_SIM}
    tb = make_tb(gpu_lib, inp, K, {})
    assert tb.fused_kernel().startswith(kernel), tb.fused_kernel()
    pool = tail._pool(inp, H)
    out, gathered = run_fused(tb, to_device(inp), K, {}, pool=pool)
    where = f"K={K} B={inp.B} A={inp.A} S={inp.S}: "
    assert_same(out, exp, where)
    rows = torch.arange(inp.B, device="cuda")
    for s in range(inp.S):
        want = pool[torch.from_numpy(out["sel_idx"][s]).cuda().long(), rows]
        assert torch.equal(gathered[s].view(torch.int32), want.view(torch.int32)), f"{where}gathered row, launch {s}"
    tb.synchronize()  # (raises on a non-zero error word)
    return exp


# ---- three-wave k_chain3: wave 0's own distribution, with its callbacks ----
@pytest.mark.gpu
@pytest.mark.parametrize("A", [2, 4, 5, 9, 12, 13, 16, 17])
def test_three_waves_action_counts(gpu_lib, port_lib, A, monkeypatch):  # noqa: F811
    monkeypatch.setenv("MZ_CHAIN3_W3", "1")
    tb = tail._check(gpu_lib, port_lib, _inputs(5, A, 20, 1100 + A))
    assert tb.fused_waves() == 3


@pytest.mark.gpu
def test_three_waves_masked(gpu_lib, port_lib, monkeypatch):  # noqa: F811
    monkeypatch.setenv("MZ_CHAIN3_W3", "1")
    tb = tail._check(gpu_lib, port_lib, _masked(5, 13, 20, 1200))
    assert tb.fused_waves() == 3


# ---- four-wave k_chain3: both sides of the row limit ----
@pytest.mark.gpu
@pytest.mark.parametrize("A", [15, 16, 17])
def test_four_waves_row_limit(gpu_lib, port_lib, A):  # noqa: F811
    tb = tail._check(gpu_lib, port_lib, _inputs(5, A, 20, 1300 + A))
    assert tb.fused_waves() == 4


# ---- no draw, no engine word ----
@pytest.mark.gpu
def test_single_action(gpu_lib, port_lib):  # noqa: F811
    tail._check(gpu_lib, port_lib, _inputs(3, 1, 6, 1400))


# ---- k_tree, K = 5 ----
@pytest.mark.gpu
@pytest.mark.parametrize("A", [2, 9, 15, 16, 17])
def test_tree_action_counts(gpu_lib, port_lib, A):  # noqa: F811
    _check_k(gpu_lib, port_lib, _inputs(4, A, 12, 1500 + A), 5, "k_tree<")


@pytest.mark.gpu
def test_tree_masked(gpu_lib, port_lib):  # noqa: F811
    _check_k(gpu_lib, port_lib, _masked(4, 13, 12, 1600), 5, "k_tree<")


@pytest.mark.gpu
def test_tree_concentrated_on_the_last_action(gpu_lib, port_lib):  # noqa: F811
    A = 9
    inp = tail._concentrated(_inputs(4, A, 12, 1700), A - 1)
    inp = replace(inp, root_beta=inp.beta[0].copy())  # (the root's row too: every node's K draws)
    exp = _check_k(gpu_lib, port_lib, inp, 5, "k_tree<")
    # (all but 1e-6 of the weight on the last action: the K draws land there, on the lane whose
    # cumulative probability is forced to 1.0, so every node has that one child)
    assert (exp["sel_act"] == A - 1).all() and (exp["degree"] == 1).all()


# ---- k_step: the per-agent tables of a joint tree; more draws than lanes ----
@pytest.mark.gpu
def test_step_joint_tree(gpu_lib, port_lib):  # noqa: F811
    from mazero_amd.cytree import Tree_batch

    B, N, A, K, S = 3, 2, 9, 5, 8
    assert Tree_batch(B, N, A, K, S, 0.01, 17, 0.75, 0.8, lib=gpu_lib).fused_kernel().startswith("k_step<")
    rec_g, out_g = _joint_run(gpu_lib, B, N, A, K, S, 1800)
    rec_c, out_c = _joint_run(port_lib, B, N, A, K, S, 1800)
    for s, ((ig, ag), (ic, ac)) in enumerate(zip(rec_g, rec_c)):
        np.testing.assert_array_equal(ig, ic, err_msg=f"idx sim {s}")
        np.testing.assert_array_equal(ag, ac, err_msg=f"actions sim {s}")
    for k in ("values", "mv", "mp"):
        g, c = out_g[k], out_c[k]
        assert g.shape == c.shape and g.dtype == c.dtype, k
        np.testing.assert_array_equal(g.view(np.int32), c.view(np.int32), err_msg=k)
    for k in ("q", "acts", "vc", "pr", "bh"):
        for i, (g, c) in enumerate(zip(out_g[k], out_c[k])):
            assert g.shape == c.shape, (k, i)
            np.testing.assert_array_equal(g.view(np.int32), c.view(np.int32), err_msg=f"{k}[{i}]")


@pytest.mark.gpu
def test_step_more_draws_than_lanes(gpu_lib, port_lib):  # noqa: F811
    _check_k(gpu_lib, port_lib, _inputs(2, 9, 6, 1900), 65, "k_step<")


# ---- wave 1 of k_chain3: the recurrence's length classes, the node classes, the reload ----
@pytest.mark.gpu
@pytest.mark.parametrize("S", [40, 2])
def test_wave1_chain_lengths(gpu_lib, port_lib, S, monkeypatch):  # noqa: F811
    # S = 40: past the 16- and 32-level reads, the leaf's reward patched into the first batch;
    # S = 2: chains of one and two nodes
    tb = tail._check(gpu_lib, port_lib, _inputs(2, 9, S, 2000 + S), monkeypatch=monkeypatch)
    assert tb.fused_waves() == 4


@pytest.mark.gpu
@pytest.mark.parametrize("w4", [True, False], ids=["four_waves", "three_waves"])
def test_wave1_128_node_class(gpu_lib, port_lib, w4, monkeypatch):  # noqa: F811
    if w4:
        monkeypatch.setenv("MZ_CHAIN3_W4", "1")
    tb = tail._check(gpu_lib, port_lib, _inputs(2, 9, 70, 2100), kernel="k_chain3<128>")
    assert tb.fused_waves() == (4 if w4 else 3)


@pytest.mark.gpu
def test_wave1_replay_out_of_sequence(gpu_lib, port_lib):  # noqa: F811
    tail.test_graph_of_one_launch_replayed_out_of_sequence(gpu_lib, port_lib)


@pytest.mark.gpu
def test_wave1_not_tame_value(gpu_lib, port_lib, monkeypatch):  # noqa: F811
    tail._check(gpu_lib, port_lib, tail._wild_value(_inputs(2, 9, 20, 2200)), monkeypatch=monkeypatch)
