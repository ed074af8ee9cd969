"""k_chain3: the draw wave stores what it draws (needs an MI355X: `pytest -m gpu`).

In the four-wave kernel's launches with a selection, wave 0 and the draw wave load the same header
line, rows and arguments and evaluate one predicate: no error, the chain in sequence, select_walk's
fast case whatever the draw.  When it holds the draw wave stores the five words the drawn action
feeds (the child's prior and action records, act[t], the header's leaf_y, the root child's D record)
and wave 0 writes the rest without reading an action; when it does not, the draw wave stores nothing
and wave 0 draws itself.  No wave waits for another.

Every case is a K = 1 search of B = 4 trees and S = 6 simulations through the fused device loop
against the CPU port, bit for bit: every launch's idx, idy and act, and at the end the root values,
the visit counts and every other readback.  A test cannot see which wave stored: the same file also
passes on a build with -DMZ_CHAIN3_DRAW_STORES=0, where the predicate is false everywhere.
"""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import pytest

import test_chain3_tail as tail
from test_gpu_parity import gpu_lib, make_tb, to_device  # noqa: F401  (gpu_lib: fixture)

torch = pytest.importorskip("torch")

K = 1
B = 4
S = 6


def _inputs(A, seed, B_=B):
    from mazero_amd.synthetic import make_search_inputs

    return make_search_inputs(np.random.default_rng(seed), B_, A, S)


def _check4(gpu_lib, port_lib, inp, **kw):  # noqa: F811
    tb = tail._check(gpu_lib, port_lib, inp, **kw)
    assert tb.fused_waves() == 4, "the handle did not take the four-wave kernel"
    return tb


# ---- every cdf_short class (4, 8, 12 and 16 terms) and the long form ----
@pytest.mark.gpu
@pytest.mark.parametrize("A", [2, 5, 9, 12, 16, 17])
def test_action_counts(gpu_lib, port_lib, A):  # noqa: F811
    _check4(gpu_lib, port_lib, _inputs(A, 11000 + A))


# ---- no draw: the draw wave still stores the child's records and act ----
@pytest.mark.gpu
def test_one_action(gpu_lib, port_lib):  # noqa: F811
    _check4(gpu_lib, port_lib, _inputs(1, 11100))


# ---- a wild prior: the predicate's false branch, on one tree of the launch ----
@pytest.mark.gpu
def test_wild_prior_on_one_action(gpu_lib, port_lib):  # noqa: F811
    inp = _inputs(9, 11200)
    b = inp.beta.copy()
    b[2:, 1, 0, 3] = np.float32(1e-38)  # policy / beta is past 1e30 there: tree 1 is not tame from simulation 2 on
    inp = replace(inp, beta=b)
    assert (inp.policy[2:, 1, 0, 3] / b[2:, 1, 0, 3] > 1e30).all()
    _check4(gpu_lib, port_lib, inp)


def _drive(tb, inp, hsx_of, n_sims, dev):
    """prepare, select, then n_sims fused launches with hidden-state index hsx_of(s): every launch's
    (idx, idy, act)."""
    from mazero_amd.synthetic import DEFAULTS

    c2, c1, g = DEFAULTS["pb_c_base"], DEFAULTS["pb_c_init"], DEFAULTS["discount"]
    tb.prepare(inp.root_reward, inp.root_value, inp.root_policy, inp.root_beta, K, inp.noise_eps, inp.root_noise)
    got = []
    if dev:
        out = tb.batch_selection_device(c2, c1, g)

        def rec():
            torch.cuda.synchronize()
            got.append((out[0].cpu().tolist(), out[1].cpu().tolist(), out[2].cpu().reshape(inp.B).tolist()))

        rec()
        for s in range(n_sims):
            tb.expansion_backup_selection_device(hsx_of(s), g, K, inp.reward[s % S], inp.value[s % S],
                                                 inp.policy[s % S], inp.beta[s % S], c2, c1, out=out)
            rec()
    else:
        for s in range(n_sims + 1):
            ix, iy, act = tb.batch_selection(c2, c1, g)
            got.append((list(ix), list(iy), np.asarray(act).reshape(inp.B).tolist()))
            if s < n_sims:
                tb.batch_expansion_and_backup(hsx_of(s), g, K, inp.reward[s % S], inp.value[s % S], inp.policy[s % S],
                                              inp.beta[s % S])
    return got


# ---- the error path: a pool one node too small for the launch ----
@pytest.mark.gpu
def test_pool_one_node_too_small(gpu_lib, port_lib):  # noqa: F811
    from mazero_amd.synthetic import DEFAULTS

    inp = _inputs(9, 11300)
    c2, c1, g = DEFAULTS["pb_c_base"], DEFAULTS["pb_c_init"], DEFAULTS["discount"]
    # the port: simulations past simulation_num until one finds the pool a node short
    ref = make_tb(port_lib, inp, K, {})
    ref.prepare(inp.root_reward, inp.root_value, inp.root_policy, inp.root_beta, K, inp.noise_eps, inp.root_noise)
    ref_sel, ok = [], 0
    for s in range(S + 4):
        try:
            ix, iy, act = ref.batch_selection(c2, c1, g)
            ref.batch_expansion_and_backup(s + 1, g, K, inp.reward[s % S], inp.value[s % S], inp.policy[s % S],
                                           inp.beta[s % S])
        except RuntimeError:
            break
        ref_sel.append((list(ix), list(iy), np.asarray(act).reshape(B).tolist()))
        ok += 1
    assert S <= ok < S + 4, ok
    tb = make_tb(gpu_lib, inp, K, {})
    assert tb.fused_kernel() == "k_chain3<64>" and tb.fused_waves() == 4
    # launches 0 .. ok - 1 fit (the selection after the last one is not the port's to give); launch ok
    # is the one the port refuses: the outputs zero, the error word the pool's
    got = _drive(tb, to_device(inp), lambda s: s + 1, ok + 1, dev=True)
    assert got[:ok] == ref_sel
    assert got[ok + 1] == ([0] * B, list(range(B)), [0] * B)
    word, msg = tail._error_word(tb)
    assert word & 1 and "node pool exhausted" in msg, msg


# ---- one launch out of sequence: the header's chain wins over the launch's hidden-state index ----
@pytest.mark.gpu
def test_one_launch_out_of_sequence(gpu_lib, port_lib):  # noqa: F811
    from mazero_amd.synthetic import DEFAULTS, readbacks

    inp = _inputs(9, 11400)
    hsx_of = lambda s: 3 if s == 3 else s + 1  # noqa: E731  (launch 3 names launch 2's leaf slot)
    ref = make_tb(port_lib, inp, K, {})
    want = _drive(ref, inp, hsx_of, S, dev=False)
    tb = make_tb(gpu_lib, inp, K, {})
    assert tb.fused_kernel() == "k_chain3<64>" and tb.fused_waves() == 4
    got = _drive(tb, to_device(inp), hsx_of, S, dev=True)
    assert got == want
    tb.synchronize()
    g = DEFAULTS["discount"]
    a, b = readbacks(tb, g), readbacks(ref, g)
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


# ---- the last launch fused with the readback (SEL = false: the hand-over stays) ----
@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 9])
def test_fused_readback_last_launch(gpu_lib, port_lib, A):  # noqa: F811
    _check4(gpu_lib, port_lib, _inputs(A, 11500 + A), fused_rb="packed")


# ---- more workgroups than CUs: the handle still launches three waves ----
@pytest.mark.gpu
def test_more_workgroups_than_cus_keeps_three_waves(gpu_lib, port_lib):  # noqa: F811
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tb = tail._check(gpu_lib, port_lib, _inputs(9, 11600, B_=cus + 1), H=4)
    assert tb.fused_waves() == 3
