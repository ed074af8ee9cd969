"""Every kernel family on adversarial network outputs (needs an MI355X: `pytest -m gpu`).

The searches of the rest of the suite are fed by `mazero_amd.synthetic.make_search_inputs`, whose
outputs are benign: beta equals policy at every non-root node, no row has an exact zero, a
subnormal or nearly all its weight on one action, values and rewards are of order one, and all
trees of a batch are alike.  k_chain3 has hand-written cases for each of these edges; every other
family carries its own copy of the expansion and draw, the tame bookkeeping, the min/max normaliser
and (K = 1) the fast and exact selections, and none had been run on such inputs.

Each row here is the smallest shape that `mz_create`'s own rules (and its test flags, read at
create) send to one kernel; the row first asserts the kernel's name.  It then runs every input
class of tests/edge_inputs.py, on every tree and on tree 1 alone (a wild tree beside tame ones in
one launch), through the fused device loop against the CPU port, bit for bit: every selection,
every readback, and the error word.  tests/test_oracle.py pins the port against the reference
ctree on the same classes.  The three long chains (one launch per simulation for hundreds of
simulations) run six classes on tree 1 alone.

K = 1 rows whose kernel has a fast selection also run the wild classes on a second handle of
another K = 1 family and compare the event counters of the two.

NaN inputs are out of scope: the reference ctree throws on them (tests/edge_inputs.py).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import pytest

from conftest import assert_same
from edge_inputs import EDGE_CLASSES, WILD
from test_chain3_tail import COUNTERS, PER_SIM
from test_gpu_parity import gpu_lib, make_tb, run_fused, to_device  # noqa: F401  (gpu_lib: fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALL = tuple(EDGE_CLASSES)
# the long chains run these
LONG = ("beta_tau2", "beta_rolled", "peaked", "wild_value", "wild_prior", "small_spread")
BOTH = (None, [1])
ONE = ([1],)

# id, kernel, K, A, S, B, flags set at create, classes, trees, flags of the second K = 1 handle
Row = namedtuple("Row", "id kernel K A S B env classes trees other")
ROWS = [
    # ---- K = 1: P = S + 2 nodes ----
    Row("k1_chain3_64", "k_chain3<64>", 1, 9, 6, 3, (), ALL, BOTH, ("MZ_CHAIN_V2",)),
    # (the k_chain3 tests run the 256-node class on benign inputs and reward spikes only: every class)
    Row("k1_chain3_256", "k_chain3<256>", 1, 9, 200, 3, (), ALL, BOTH, ("MZ_CHAIN_V2",)),
    Row("k1_chain_64", "k_chain<64>", 1, 9, 6, 3, ("MZ_CHAIN_V2",), ALL, BOTH, ("MZ_NO_CHAIN",)),
    Row("k1_chain_512", "k_chain<512>", 1, 9, 300, 3, (), LONG, ONE, ("MZ_NO_CHAIN",)),
    Row("k1_chain_1024", "k_chain<1024>", 1, 9, 600, 3, (), LONG, ONE, ("MZ_NO_CHAIN",)),
    Row("k1_chain_general", "k_chain<0>", 1, 9, 1030, 2, (), LONG, ONE, ("MZ_NO_CHAIN",)),
    Row("k1_step_64", "k_step<64>", 1, 9, 6, 3, ("MZ_NO_CHAIN",), ALL, BOTH, ("MZ_CHAIN_V2",)),
    Row("k1_hbm", "k_hbm", 1, 9, 6, 3, ("MZ_HBM",), ALL, BOTH, None),  # (k_hbm has the exact selection only)
    # ---- K > 1: P = 1 + min(K, A) * (S + 1) nodes ----
    Row("k2_tree_64", "k_tree<64>", 2, 9, 6, 3, (), ALL, BOTH, None),
    Row("k5_tree_64", "k_tree<64>", 5, 9, 10, 3, (), ALL, BOTH, None),
    Row("k5_tree_128", "k_tree<128>", 5, 9, 20, 3, (), ALL, BOTH, None),
    Row("k5_tree_256", "k_tree<256>", 5, 9, 45, 3, (), ALL, BOTH, None),
    Row("k5_tree_384", "k_tree<384>", 5, 9, 70, 3, (), ALL, BOTH, None),
    Row("k5_tree_512", "k_tree<512>", 5, 9, 100, 3, (), ALL, BOTH, None),
    Row("k10_tree_1024_s128", "k_tree<1024,s128>", 10, 15, 80, 3, (), ALL, BOTH, None),
    Row("k5_tree_1024", "k_tree<1024>", 5, 9, 200, 3, (), ALL, BOTH, None),
    Row("k5_step_64", "k_step<64>", 5, 9, 10, 3, ("MZ_NO_TREE",), ALL, BOTH, None),
    Row("k5_step_256", "k_step<256>", 5, 9, 45, 3, ("MZ_NO_TREE",), ALL, BOTH, None),
    # more draws than actions (every node can hold all nine children, beta_hat counts above 1).  Up to
    # 64 draws k_tree serves a pool of this size at any S a test can afford (k_step takes over past
    # 340 value entries), so K = 33 runs on both: k_tree as created, k_step under MZ_NO_TREE; with
    # more draws than lanes (K = 65) k_step is what mz_create chooses by itself
    Row("k33_tree_128", "k_tree<128>", 33, 9, 10, 3, (), ALL, BOTH, None),
    Row("k33_step_128", "k_step<128>", 33, 9, 10, 3, ("MZ_NO_TREE",), ALL, BOTH, None),
    Row("k65_step_128", "k_step<128>", 65, 9, 10, 3, (), ALL, BOTH, None),
    Row("k5_hbm", "k_hbm", 5, 9, 10, 3, ("MZ_HBM",), ALL, BOTH, None),
    Row("k10_hbm_wide", "k_hbm", 10, 100, 10, 3, (), ALL, BOTH, None),  # (past one lane per action)
]


def _create(monkeypatch, lib, inp, K, knobs, env):
    """A handle created under mz_create's test flags `env` (read at create, cleared after)."""
    for e in env:
        monkeypatch.setenv(e, "1")
    try:
        return make_tb(lib, inp, K, knobs)
    finally:
        for e in env:
            monkeypatch.delenv(e)


def _expected(port_lib, inp, K, knobs):
    from mazero_amd.synthetic import run_search

    with np.errstate(all="ignore"):
        exp = run_search(make_tb(port_lib, inp, K, knobs), inp, K, knobs, per_sim=False)
    return {k: v for k, v in exp.items() if k not in PER_SIM}


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_kernel_row(gpu_lib, port_lib, row, monkeypatch):  # noqa: F811
    from mazero_amd.synthetic import make_search_inputs

    K = row.K
    base = make_search_inputs(np.random.default_rng(31000 + sum(map(ord, row.id))), row.B, row.A, row.S)
    ran = 0
    for name in row.classes:
        for trees in row.trees:
            inp = EDGE_CLASSES[name](base, trees)
            where = f"{row.id} {name} trees={trees}: "
            tb = _create(monkeypatch, gpu_lib, inp, K, {}, row.env)
            assert tb.fused_kernel() == row.kernel, where + tb.fused_kernel()
            out, _ = run_fused(tb, to_device(inp), K, {})
            assert_same(out, _expected(port_lib, inp, K, {}), where)
            tb.synchronize()  # (raises on a non-zero error word)
            ran += 1
            if row.other is not None and name in WILD:
                # the same search on another K = 1 family: what the two counted
                tb2 = _create(monkeypatch, gpu_lib, inp, K, {}, row.other)
                assert tb2.fused_kernel() != row.kernel and not tb2.fused_kernel().startswith("k_hbm"), where
                run_fused(tb2, to_device(inp), K, {})
                tb2.synchronize()
                a, b = tb.stats(), tb2.stats()
                assert {k: a[k] for k in COUNTERS} == {k: b[k] for k in COUNTERS}, where + tb2.fused_kernel()
                assert a["selects"] == inp.B * inp.S
    assert ran == len(row.classes) * len(row.trees)


def test_rows_cover_every_class_and_family():
    """The table itself: every class runs on every short row, every kernel family has a row."""
    assert set(ALL) == set(EDGE_CLASSES) and set(LONG) <= set(ALL) and set(WILD) <= set(ALL)
    for r in ROWS:
        assert r.classes is ALL or (r.K == 1 and r.S >= 300 and r.classes is LONG and r.trees is ONE), r.id
    want = {"k_chain3<64>", "k_chain3<256>", "k_chain<64>", "k_chain<512>", "k_chain<1024>", "k_chain<0>",
            "k_step<64>", "k_step<128>", "k_step<256>", "k_hbm", "k_tree<64>", "k_tree<128>", "k_tree<256>",
            "k_tree<384>", "k_tree<512>", "k_tree<1024,s128>", "k_tree<1024>"}
    assert {r.kernel for r in ROWS} == want
    assert {(r.kernel, r.K == 1) for r in ROWS} >= {("k_step<64>", True), ("k_step<64>", False), ("k_hbm", True),
                                                    ("k_hbm", False)}


@pytest.mark.parametrize("chunk", range(4))
def test_edge_fuzz_vs_port(gpu_lib, port_lib, chunk, monkeypatch):  # noqa: F811
    """Forty seeded random small configurations (tests/fuzz_configs.py::fuzz_edge_configs: B 1-8,
    A 2-100, K 1-70, S 4-60, every search knob, one or two input classes on all trees or a subset),
    every third one forced onto k_hbm: the fused device loop against the CPU port."""
    from fuzz_configs import edge_inputs_of, fuzz_edge_configs

    for i, cfg in enumerate(fuzz_edge_configs(4321 + chunk, 10)):
        B, A, K, S, knobs, lz, ties, eps, s, classes, trees = cfg
        inp = edge_inputs_of(cfg)
        where = f"B={B} A={A} K={K} S={S} knobs={knobs} lz={lz} ties={ties} eps={eps} {classes} trees={trees}: "
        tb = _create(monkeypatch, gpu_lib, inp, K, knobs, ("MZ_HBM",) if i % 3 == 1 else ())
        assert tb.fused_kernel() == "k_hbm" or (i % 3 != 1 and A <= 64), where + tb.fused_kernel()
        out, _ = run_fused(tb, to_device(inp), K, knobs)
        assert_same(out, _expected(port_lib, inp, K, knobs), "gpu fused " + where)
        tb.synchronize()
