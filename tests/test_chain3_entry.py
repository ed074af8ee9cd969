"""k_chain3's entry and the node arrays' closed-form layout (needs an MI355X: `pytest -m gpu`).

The node arrays' spans are multiples of one unit c, the span of a 4-byte array (the 16-byte arrays
take 4 c), so every node array is at o_A plus a constant multiple of c.  k_chain3 gets o_A and c in
one preloaded argument dword, tests the wave index in its first instructions and addresses every
record as the arena base plus a 32-bit byte offset; the discount rides in wave 0's argument line.
Every other kernel family gets the same layout through arena_nodes(), and mz_create checks its plan
against arena_hot() for every handle.

Every search case is a search against the CPU port, bit for bit; the K = 1 ones per launch (idx,
idy, act and the gathered row), at the end every readback, the event counters against the same
search on k_chain (MZ_CHAIN_V2=1) and the error word.  The shapes are the smallest that take each
path.  A handle whose o_A or c does not fit 16 bits keeps k_chain, the route MZ_CHAIN_V2 forces at
any size.
"""
from __future__ import annotations

import gc

import numpy as np
import pytest

from conftest import assert_same
from test_chain3_round1 import K, _check, _inputs
from test_gpu_parity import _joint_run, gpu_lib, make_tb, run_fused, to_device  # noqa: F401  (gpu_lib: fixture)

torch = pytest.importorskip("torch")

# B x S with P = S + 2: B * P on and off multiples of 16 and 64 (the units of the 16- and 4-byte
# arrays' 256-byte blocks); two action counts per pair, every count six times
_AS = [1, 2, 9, 17, 36]
LAYOUT = [(B, S, _AS[(2 * n + j) % len(_AS)])
          for n, (B, S) in enumerate((B, S) for B in (1, 3, 63, 64, 65) for S in (2, 6, 62)) for j in (0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,A", LAYOUT)
def test_layout_closed_form(gpu_lib, port_lib, B, S, A, monkeypatch):  # noqa: F811
    _check(gpu_lib, port_lib, _inputs(B, A, S, 10000 + 1000 * B + 10 * S + A), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("S,kernel", [(70, "k_chain3<128>"), (200, "k_chain3<256>")])
def test_node_classes(gpu_lib, port_lib, S, kernel, monkeypatch):  # noqa: F811
    _check(gpu_lib, port_lib, _inputs(3, 9, S, 20000 + S), monkeypatch, kernel=kernel)


# The 16 KiB row class (a row past 4 KiB) keeps the earlier entry -- offsets by arena_nodes() on the
# new layout, the discount in the 14th argument dword: B * P on and off multiples of 16 and 64, both
# wave variants, and the 128-node class.
@pytest.mark.gpu
@pytest.mark.parametrize("B,S,A,flag,kernel", [(3, 6, 9, "MZ_CHAIN3_W4", "k_chain3<64>"), (65, 62, 36, "MZ_CHAIN3_W4", "k_chain3<64>"),
                                               (64, 6, 17, "MZ_CHAIN3_W3", "k_chain3<64>"), (3, 70, 9, "MZ_CHAIN3_W3", "k_chain3<128>")])
def test_row_class2_entry(gpu_lib, port_lib, B, S, A, flag, kernel, monkeypatch):  # noqa: F811
    import test_chain3_tail as tail
    from mazero_amd.synthetic import make_search_inputs

    monkeypatch.setenv(flag, "1")  # (read at mz_create)
    inp = make_search_inputs(np.random.default_rng(24000 + 100 * B + S), B, A, S)
    tb = tail._check(gpu_lib, port_lib, inp, kernel=kernel, H=1028)  # 4,112-byte rows
    assert tb.fused_waves() == (4 if flag == "MZ_CHAIN3_W4" else 3)


@pytest.mark.gpu
@pytest.mark.parametrize("flag,waves", [("MZ_CHAIN3_W3", 3), ("MZ_CHAIN3_W4", 4)])
def test_wave_variants(gpu_lib, port_lib, flag, waves, monkeypatch):  # noqa: F811
    monkeypatch.setenv(flag, "1")  # (read at mz_create)
    tb = _check(gpu_lib, port_lib, _inputs(3, 9, 6, 21000 + waves), monkeypatch)
    assert tb.fused_waves() == waves


@pytest.mark.gpu
def test_forced_out_of_range_route(gpu_lib, port_lib, monkeypatch):  # noqa: F811
    # a handle whose packed offsets do not fit keeps k_chain; MZ_CHAIN_V2 forces that route at any size
    monkeypatch.setenv("MZ_CHAIN_V2", "1")
    _check(gpu_lib, port_lib, _inputs(3, 9, 6, 22000), monkeypatch, kernel="k_chain<64>")


# ---- the other kernel families on the new arena ----
FAMILIES = [("k_tree", 5, None, "k_tree<64>"), ("k_step", 1, "MZ_NO_CHAIN", "k_step<64>"), ("k_hbm", 1, "MZ_HBM", "k_hbm"),
            ("k_hbm_k5", 5, "MZ_HBM", "k_hbm"), ("prepare_general", 1, "MZ_PREPARE_GENERAL", "k_chain3<64>"),
            ("k_chain", 1, "MZ_CHAIN_V2", "k_chain<64>")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,flag,kernel", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_other_kernel_families(gpu_lib, port_lib, name, k, flag, kernel, monkeypatch):  # noqa: F811
    from mazero_amd.synthetic import run_search

    inp = _inputs(3, 9, 6, 23000 + k)
    exp = run_search(make_tb(port_lib, inp, k, {}), inp, k, {})
    if flag:
        monkeypatch.setenv(flag, "1")  # (read at mz_create)
    tb = make_tb(gpu_lib, inp, k, {})
    assert tb.fused_kernel() == kernel
    out, _ = run_fused(tb, to_device(inp), k, {})
    exp = {key: v for key, v in exp.items() if key not in ("root_values_per_sim", "marginal_per_sim")}
    assert_same(out, exp, f"{name}: ")
    tb.synchronize()  # (raises on a non-zero error word)


@pytest.mark.gpu
def test_joint_tree(gpu_lib, port_lib):  # noqa: F811
    rec_g, out_g = _joint_run(gpu_lib, 3, 2, 9, 4, 6, 5)
    rec_c, out_c = _joint_run(port_lib, 3, 2, 9, 4, 6, 5)
    for s, ((ig, ag), (ic, ac)) in enumerate(zip(rec_g, rec_c)):
        np.testing.assert_array_equal(ig, ic, err_msg=f"idx sim {s}")
        np.testing.assert_array_equal(ag, ac, err_msg=f"actions sim {s}")
    for key in ("values", "mv", "mp"):
        np.testing.assert_array_equal(out_g[key].view(np.int32), out_c[key].view(np.int32), err_msg=key)
    for key in ("q", "acts", "vc", "pr", "bh"):
        for i, (g, c) in enumerate(zip(out_g[key], out_c[key])):
            assert g.shape == c.shape, (key, i)
            np.testing.assert_array_equal(g.view(np.int32), c.view(np.int32), err_msg=f"{key}[{i}]")


# ---- mz_create's plan check: every geometry's arena agrees with arena_hot() ----
SWEEP = [(B, _AS[1 + (i + j + n) % 4], Kk, S)
         for i, B in enumerate((1, 7, 256, 1024)) for j, Kk in enumerate((1, 5, 64)) for n, S in enumerate((4, 50, 200))]
SWEEP += [(1, 1, 1, 4), (7, 1, 5, 50), (256, 36, 5, 4), (1024, 2, 64, 200)]


@pytest.mark.gpu
def test_create_destroy_sweep(gpu_lib):  # noqa: F811
    from mazero_amd._lib import trim_caches
    from mazero_amd.cytree import Tree_batch

    assert len(SWEEP) == 40
    for B, A, Kk, S in SWEEP:
        tb = Tree_batch(B, 1, A, Kk, S, 0.01, 17, 0.75, 0.8, lib=gpu_lib)  # (raises if the plan check fails)
        assert tb.fused_kernel()
        if Kk == 1 and S + 2 <= 256:
            assert tb.fused_kernel().startswith("k_chain3<"), (B, A, Kk, S, tb.fused_kernel())
        del tb
        gc.collect()
    torch.cuda.synchronize()
    trim_caches()
