"""The ends of k_chain3's two arms (needs an MI355X: `pytest -m gpu`).

Wave 1 ends on the value normaliser: the minimum and maximum of the chain's q values, reduced by
one fused DPP butterfly (`wave_minmax_to63`) whose results lane 63 stores to LDS and to the header.
The draw ends on the cumulative table of `cdf_row<N>`, whose last prefix term feeds the lane that
is forced to 1.0.

A wrong normaliser is invisible in a K = 1 search: every node has one child, so no score changes a
selection.  The first group therefore reads the header's normaliser after every fused launch
(`mz_debug_minmax`) and compares it, bit for bit, with the multiset of the pure-Python tree
(oracle/ptree.py: `mm.se[0]`, `mm.se[-1]`, `len(mm.se)`).  One simulation's reward is +-50, so the
unique maximum or minimum sits at a chosen node j = a chosen lane of the butterfly: the cases are
the DPP row and chunk boundaries of every node class.  The second group runs whole searches
against the CPU port, bit for bit (every launch's idx, idy and act, every readback), over every
action count and with the draw concentrated on the first bin, on the last prefix term's bin and on
its neighbour (the cases an exact term count per action count has to get right).
"""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import pytest

from test_chain3_tail import K, _check, _concentrated, _inputs
from test_gpu_parity import gpu_lib, make_tb, to_device  # noqa: F401  (gpu_lib: fixture)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def _spike(inp, j, sign):
    """Node j's reward (simulation j - 1 expands node j) is sign * 50 on every tree: its q is the
    unique maximum (minimum) of the chain from that launch on."""
    r = inp.reward.copy()
    r[j - 1] = np.float32(sign * 50.0)
    return replace(inp, reward=r)


def _minmax_search(lib, inp, kernel, fused_rb=False, waves=None):
    """One K = 1 search through the fused device loop, the pure-Python tree stepped beside it: after
    every fused launch the header's normaliser against the tree's multiset.  Returns the largest
    |value| seen (what the wild case reports)."""
    import ptree

    from mazero_amd.synthetic import DEFAULTS as d

    c2, c1, g = d["pb_c_base"], d["pb_c_init"], d["discount"]
    B, S = inp.B, inp.S
    pt = ptree.Tree_batch(B, 1, inp.A, K, S, d["delta_lb"], inp.seed, d["rho"], d["lam"])
    pt.prepare(inp.root_reward, inp.root_value, inp.root_policy, inp.root_beta, K, inp.noise_eps, inp.root_noise)
    tb = make_tb(lib, inp, K, {})
    assert tb.fused_kernel() == kernel
    if waves is not None:
        assert tb.fused_waves() == waves
    di = to_device(inp)
    tb.prepare(di.root_reward, di.root_value, di.root_policy, di.root_beta, K, di.noise_eps, di.root_noise)
    sel = tb.batch_selection_device(c2, c1, g)
    seen = 0.0
    with np.errstate(over="ignore"):
        for s in range(S):
            pt.batch_selection(c2, c1, g)
            pt.batch_expansion_and_backup(s + 1, g, K, inp.reward[s], inp.value[s], inp.policy[s], inp.beta[s])
            if s + 1 < S:
                tb.expansion_backup_selection_device(s + 1, g, K, di.reward[s], di.value[s], di.policy[s], di.beta[s],
                                                     c2, c1, out=sel)
            elif fused_rb:
                tb.expansion_backup_readback_device(s + 1, g, K, di.reward[s], di.value[s], di.policy[s], di.beta[s],
                                                    readback_discount=g, out=None)
            else:
                tb.batch_expansion_and_backup(s + 1, g, K, di.reward[s], di.value[s], di.policy[s], di.beta[s])
            mn, mx, cnt = tb.debug_minmax()
            want_mn = np.array([t.mm.se[0] for t in pt.trees], np.float32)
            want_mx = np.array([t.mm.se[-1] for t in pt.trees], np.float32)
            want_cnt = np.array([len(t.mm.se) for t in pt.trees], np.int32)
            where = f"B={B} S={S} launch {s}: "
            assert not np.isnan(want_mn).any() and not np.isnan(want_mx).any(), where + "the multiset orders no NaN"
            assert (cnt == want_cnt).all(), (where, cnt, want_cnt)
            assert (_bits(mn) == _bits(want_mn)).all(), (where, mn, want_mn)
            assert (_bits(mx) == _bits(want_mx)).all(), (where, mx, want_mx)
            seen = max(seen, float(np.abs(want_mn).max()), float(np.abs(want_mx).max()))
    tb.synchronize()  # (raises on a non-zero error word)
    return seen


def _spiked(lib, B, S, j, sign, kernel):
    inp = _spike(_inputs(B, 9, S, 21000 + 13 * S + j), j, sign)
    seen = _minmax_search(lib, inp, kernel)
    assert 40.0 < seen < 60.0  # (the spike is the extreme it was meant to be)


# ---- the extreme at a chosen lane: the DPP rows' and the chunks' boundaries ----
@pytest.mark.parametrize("sign", [1, -1], ids=["max", "min"])
@pytest.mark.parametrize("j", [1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 47, 48, 49, 50])
def test_extreme_at_node_64(gpu_lib, j, sign):  # noqa: F811
    _spiked(gpu_lib, 4, 50, j, sign, "k_chain3<64>")


@pytest.mark.parametrize("j", [63, 64, 65, 69])
def test_extreme_at_node_128(gpu_lib, j):  # noqa: F811
    for sign in (1, -1):
        _spiked(gpu_lib, 4, 70, j, sign, "k_chain3<128>")


@pytest.mark.parametrize("j", [127, 128, 129, 191, 192, 199])
def test_extreme_at_node_256(gpu_lib, j):  # noqa: F811
    _spiked(gpu_lib, 2, 200, j, 1 if j % 2 else -1, "k_chain3<256>")


# ---- the three-wave handle: more trees than compute units ----
def test_three_wave_handle(gpu_lib):  # noqa: F811
    B = torch.cuda.get_device_properties(0).multi_processor_count + 1
    _minmax_search(gpu_lib, _spike(_inputs(B, 9, 6, 22000), 3, -1), "k_chain3<64>", waves=3)


# ---- the last launch fused with the readback (SEL = false) ----
def test_last_launch_fused_readback(gpu_lib):  # noqa: F811
    _minmax_search(gpu_lib, _spike(_inputs(4, 9, 6, 22100), 6, 1), "k_chain3<64>", fused_rb=True)


# ---- a wild value: the launch is not tame, wave 0 reads the pair lane 63 left in LDS ----
def test_wild_value(gpu_lib):  # noqa: F811
    inp = _inputs(4, 9, 8, 22200)
    v = inp.value.copy()
    v[2] = np.float32(1e35)
    seen = _minmax_search(gpu_lib, replace(inp, value=v), "k_chain3<64>")
    print("largest |q| in the multiset:", seen)
    assert seen > 1e30


# ---- whole searches against the CPU port: every action count ----
@pytest.mark.parametrize("A", list(range(1, 18)))
def test_every_action_count(gpu_lib, port_lib, A):  # noqa: F811
    _check(gpu_lib, port_lib, _inputs(4, A, 6, 23000 + A))


# ---- the draw concentrated on the first bin, on the last prefix term's bin and its neighbour ----
@pytest.mark.parametrize("A", [2, 3, 9, 11, 16])
def test_drawn_bin(gpu_lib, port_lib, A):  # noqa: F811
    from test_chain3_tail import _expected

    for j in sorted({0, A - 2, A - 1}):
        inp = _concentrated(_inputs(4, A, 6, 24000 + 17 * A + j), j)
        _check(gpu_lib, port_lib, inp)
        assert (_expected(port_lib, inp)["sel_act"][1:] == j).all()  # (the case draws what it is named for)


# ---- wave 0's own draw: a wild prior on one action of one tree (the draw wave stores nothing) ----
@pytest.mark.parametrize("A", [3, 9, 11, 16])
def test_wave0_draws(gpu_lib, port_lib, A):  # noqa: F811
    inp = _inputs(4, A, 6, 25000 + A)
    b = inp.beta.copy()
    k = A - 2
    b[2:, 1, 0, k] = np.float32(1e-38)  # policy / beta is past 1e30 there: tree 1 is not tame from simulation 2 on
    inp = replace(inp, beta=b)
    assert (inp.policy[2:, 1, 0, k] / b[2:, 1, 0, k] > 1e30).all()
    tb = _check(gpu_lib, port_lib, inp)
    assert tb.fused_waves() == 4
