"""k_chain3's wave 0 after the expansion's draw (needs an MI355X: `pytest -m gpu`).

Wave 0 computes everything the draw does not feed before the draw -- the record and output
addresses, the errors, the leaf's new structure record, every lane's prior and its tame test, the
draw's u -- stores what carries no drawn word ahead of the distribution (one lane per record) and
leaves a readlane, two selects and the remaining stores for after it.  Every case here runs K = 1
searches through the fused device loop against the CPU port, bit for bit: per launch idx, idy, act
and the gathered row; at the end the root values, visit counts, every other readback, the event
counters (against the same search on the round-2 kernel k_chain, whose wave 0 is untouched) and
the error word.  The shapes are the smallest at which the reordered code takes another path.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import assert_same
from edge_inputs import concentrated as _concentrated  # noqa: F401  (the builders moved; the old names stay)
from edge_inputs import wild_prior as _wild_prior, wild_reward as _wild_reward, wild_value as _wild_value
from test_gpu_parity import gpu_lib, make_tb, run_fused, to_device  # noqa: F401  (gpu_lib: fixture)

torch = pytest.importorskip("torch")

K = 1
COUNTERS = ("selects", "path_edges", "scored", "expands", "new_children", "backup_nodes", "minmax_nodes")
PER_SIM = ("root_values_per_sim", "marginal_per_sim")


def _inputs(B, A, S, seed):
    from mazero_amd.synthetic import make_search_inputs

    return make_search_inputs(np.random.default_rng(seed), B, A, S)


def _expected(port_lib, inp):
    from mazero_amd.synthetic import run_search

    exp = run_search(make_tb(port_lib, inp, K, {}), inp, K, {})
    return {k: v for k, v in exp.items() if k not in PER_SIM}


def _pool(inp, H, seed=0):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return torch.randn(inp.S + 1, inp.B, H, device="cuda", generator=gen)


def _check(gpu_lib, port_lib, inp, kernel="k_chain3<64>", H=384, fused_rb=None, monkeypatch=None):
    """One search on k_chain3 against the port; returns the handle (kept alive by the caller)."""
    exp = _expected(port_lib, inp)
    tb = make_tb(gpu_lib, inp, K, {})
    assert tb.fused_kernel() == kernel
    pool = _pool(inp, H) if H else None
    out, gathered = run_fused(tb, to_device(inp), K, {}, pool=pool, fused_rb=fused_rb)
    where = f"B={inp.B} A={inp.A} S={inp.S} H={H}: "
    assert_same(out, exp, where)
    if pool is not None:
        rows = torch.arange(inp.B, device="cuda")
        for s in range(inp.S):
            want = pool[torch.from_numpy(out["sel_idx"][s]).cuda().long(), rows]
            assert torch.equal(gathered[s].view(torch.int32), want.view(torch.int32)), f"{where}gathered row, launch {s}"
    tb.synchronize()  # (raises on a non-zero error word)
    if monkeypatch is not None:
        # the event counters: the same search on k_chain (MZ_CHAIN_V2 is read at mz_create)
        monkeypatch.setenv("MZ_CHAIN_V2", "1")
        tb2 = make_tb(gpu_lib, inp, K, {})
        monkeypatch.delenv("MZ_CHAIN_V2")
        assert tb2.fused_kernel().startswith("k_chain<")
        run_fused(tb2, to_device(inp), K, {}, pool=pool, fused_rb=fused_rb)
        a, b = tb.stats(), tb2.stats()
        print(where, {k: a[k] for k in COUNTERS})
        assert {k: a[k] for k in COUNTERS} == {k: b[k] for k in COUNTERS}, where
        assert a["selects"] == inp.B * inp.S and a["new_children"] >= inp.B * inp.S
    return tb


def _largest_chain3_A(gpu_lib):
    from mazero_amd.cytree import Tree_batch

    for A in range(64, 36, -1):
        if Tree_batch(1, 1, A, K, 6, 0.01, 1, 0.75, 0.8, lib=gpu_lib).fused_kernel().startswith("k_chain3"):
            return A
    return 36


# ---- action-count classes of the distribution (4, 8, 12, 16, long) and the no-draw path A = 1 ----
@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 2, 4, 5, 8, 9, 12, 13, 16, 17, 36, "largest"])
def test_action_classes(gpu_lib, port_lib, A, monkeypatch):
    if A == "largest":
        A = _largest_chain3_A(gpu_lib)
        print("largest A on k_chain3:", A)
        assert A >= 36
    for B in (1, 3):
        _check(gpu_lib, port_lib, _inputs(B, A, 6, 1000 + 7 * A + B), monkeypatch=monkeypatch)


# ---- which lane is drawn: the drawn lane's own words, the forced last cp = 1.0 ----
@pytest.mark.gpu
@pytest.mark.parametrize("j", [0, 4, 8])
def test_drawn_lane(gpu_lib, port_lib, j, monkeypatch):
    for B in (1, 3):
        inp = _concentrated(_inputs(B, 9, 6, 2000 + B), j)
        _check(gpu_lib, port_lib, inp, monkeypatch=monkeypatch)
        exp = _expected(port_lib, inp)
        assert (exp["sel_act"][1:] == j).all()  # (the cases draw what they are named for)


# ---- not tame: the exact selection with the barrier ----
@pytest.mark.gpu
@pytest.mark.parametrize("wild", [_wild_prior, _wild_value, _wild_reward], ids=["prior", "value", "reward"])
def test_not_tame(gpu_lib, port_lib, wild, monkeypatch):
    for B in (1, 3):
        _check(gpu_lib, port_lib, wild(_inputs(B, 9, 6, 3000 + B)), monkeypatch=monkeypatch)


# ---- row classes of the leaf-row gather, and no pool at all ----
@pytest.mark.gpu
@pytest.mark.parametrize("H", [4, 384, 1024, 1028, 5, 0], ids=["16B", "1536B", "4096B", "4112B", "20B", "no_pool"])
def test_row_classes(gpu_lib, port_lib, H):
    for B in (1, 3):
        _check(gpu_lib, port_lib, _inputs(B, 9, 6, 4000 + B), H=H)


# ---- the last expansion (SEL = false) with the fused readback ----
@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 9])
def test_last_expansion_fused_readback(gpu_lib, port_lib, A, monkeypatch):
    for B in (1, 3):
        _check(gpu_lib, port_lib, _inputs(B, A, 6, 5000 + A + B), fused_rb="packed", monkeypatch=monkeypatch)
    # S = 1: the last expansion's leaf is the root's child (the D record of a root child)
    _check(gpu_lib, port_lib, _inputs(3, A, 1, 5100 + A), fused_rb="packed")


# ---- the other node classes ----
@pytest.mark.gpu
@pytest.mark.parametrize("S,kernel", [(70, "k_chain3<128>"), (200, "k_chain3<256>")])
def test_node_classes(gpu_lib, port_lib, S, kernel, monkeypatch):
    _check(gpu_lib, port_lib, _inputs(2, 9, S, 6000 + S), kernel=kernel, monkeypatch=monkeypatch)


def _error_word(tb):
    from mazero_amd._capi import MZError

    with pytest.raises(MZError) as e:
        tb.synchronize()
    msg = str(e.value)
    return int(msg.split("device error word 0x")[1].split(")")[0], 16), msg


# ---- error paths: launches past the pool ----
@pytest.mark.gpu
def test_past_the_pool(gpu_lib, port_lib):
    from mazero_amd.synthetic import DEFAULTS

    B, A, S = 3, 9, 6
    inp = _inputs(B, A, S, 7000)
    c2, c1, g = DEFAULTS["pb_c_base"], DEFAULTS["pb_c_init"], DEFAULTS["discount"]
    # the port: simulations past simulation_num until it refuses one
    ref = make_tb(port_lib, inp, K, {})
    ref.prepare(inp.root_reward, inp.root_value, inp.root_policy, inp.root_beta, K, inp.noise_eps, inp.root_noise)
    ref_sel, ok = [], 0
    for s in range(S + 4):
        try:
            ix, _, act = ref.batch_selection(c2, c1, g)
            ref.batch_expansion_and_backup(s + 1, g, K, inp.reward[s % S], inp.value[s % S], inp.policy[s % S],
                                           inp.beta[s % S])
        except RuntimeError:
            break
        ref_sel.append((list(ix), np.asarray(act).reshape(B).tolist()))
        ok += 1
    assert S <= ok < S + 4, ok  # (the pool is sized for simulation_num: a launch soon after overflows)
    d = to_device(inp)
    tb = make_tb(gpu_lib, inp, K, {})
    assert tb.fused_kernel() == "k_chain3<64>"
    tb.prepare(d.root_reward, d.root_value, d.root_policy, d.root_beta, K, d.noise_eps, d.root_noise)
    out = tb.batch_selection_device(c2, c1, g)
    got = []

    def launch(s):
        tb.expansion_backup_selection_device(s + 1, g, K, d.reward[s % S], d.value[s % S], d.policy[s % S],
                                             d.beta[s % S], c2, c1, out=out)
        torch.cuda.synchronize()
        return out[0].cpu().tolist(), out[1].cpu().tolist(), out[2].cpu().reshape(B).tolist()

    got.append((out[0].cpu().tolist(), out[2].cpu().reshape(B).tolist()))
    for s in range(ok - 1):  # every launch the port accepts: the selection that follows it
        ix, iy, act = launch(s)
        got.append((ix, act))
    assert got == ref_sel[:ok]
    # launch ok - 1 expands the last node the port accepts; launch ok is the expansion the port
    # refuses: the same error (the pool), the outputs zero
    launch(ok - 1)
    ix, iy, act = launch(ok)
    assert ix == [0] * B and act == [0] * B and iy == list(range(B))
    word, msg = _error_word(tb)
    print("error word past the pool:", hex(word))
    assert word & 1 and "node pool exhausted" in msg, msg  # kErrPool, as the port's "node pool overflow"
    # a dead tree stays dead and re-reports
    ix, iy, act = launch(ok + 1)
    assert ix == [0] * B and act == [0] * B and iy == list(range(B))
    word2, _ = _error_word(tb)
    assert word2 == word


# ---- out of sequence: one captured launch replayed at later simulations ----
@pytest.mark.gpu
def test_graph_of_one_launch_replayed_out_of_sequence(gpu_lib, port_lib):
    from mazero_amd.synthetic import DEFAULTS, readbacks

    B, A, S = 2, 9, 8
    inp = _inputs(B, A, S, 8000)
    c2, c1, g = DEFAULTS["pb_c_base"], DEFAULTS["pb_c_init"], DEFAULTS["discount"]
    hsx_of = lambda s: min(s + 1, 3)  # noqa: E731  (the graph holds simulation 3's launch)
    n_sims = 6  # simulations 1, 2 launched, 3 captured and replayed in sequence, then at 4, 5, 6
    ref = make_tb(port_lib, inp, K, {})
    ref.prepare(inp.root_reward, inp.root_value, inp.root_policy, inp.root_beta, K, inp.noise_eps, inp.root_noise)
    ref_sel = []
    sel = ref.batch_selection(c2, c1, g)
    ref_sel.append((list(sel[0]), np.asarray(sel[2]).reshape(B).tolist()))
    for s in range(n_sims):
        ref.batch_expansion_and_backup(hsx_of(s), g, K, inp.reward[s], inp.value[s], inp.policy[s], inp.beta[s])
        sel = ref.batch_selection(c2, c1, g)
        ref_sel.append((list(sel[0]), np.asarray(sel[2]).reshape(B).tolist()))
    d = to_device(inp)
    tb = make_tb(gpu_lib, inp, K, {})
    assert tb.fused_kernel() == "k_chain3<64>"
    dev = torch.device("cuda")
    out = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
           torch.empty(B, 1, dtype=torch.int32, device=dev))
    stat = [torch.empty_like(d.reward[0]), torch.empty_like(d.value[0]), torch.empty_like(d.policy[0]),
            torch.empty_like(d.beta[0])]
    got = []

    def record():
        torch.cuda.synchronize()
        assert out[1].cpu().tolist() == list(range(B))
        got.append((out[0].cpu().tolist(), out[2].cpu().reshape(B).tolist()))

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        tb.prepare(d.root_reward, d.root_value, d.root_policy, d.root_beta, K, d.noise_eps, d.root_noise)
        tb.batch_selection_device(c2, c1, g, out=out)
        record()
        for s in range(2):
            tb.expansion_backup_selection_device(s + 1, g, K, d.reward[s], d.value[s], d.policy[s], d.beta[s], c2, c1,
                                                 out=out)
            record()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        tb.expansion_backup_selection_device(3, g, K, *stat, c2, c1, out=out)
    for s in range(2, n_sims):  # (capture does not execute)
        for st_, src in zip(stat, (d.reward[s], d.value[s], d.policy[s], d.beta[s])):
            st_.copy_(src)
        torch.cuda.synchronize()
        graph.replay()
        record()
    assert got == ref_sel
    tb.synchronize()
    a, b = readbacks(tb, g), readbacks(ref, g)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


# ---- the comparison partner, pinned: the port against the compiled reference on these inputs ----
def _port_vs_ref_inputs():
    yield "A1", _inputs(3, 1, 6, 1000 + 7 * 1 + 3)
    yield "A9", _inputs(3, 9, 6, 1000 + 7 * 9 + 3)
    yield "A17", _inputs(3, 17, 6, 1000 + 7 * 17 + 3)
    yield "A36", _inputs(3, 36, 6, 1000 + 7 * 36 + 3)
    yield "A64", _inputs(3, 64, 6, 1000 + 7 * 64 + 3)
    for j in (0, 4, 8):
        yield f"lane{j}", _concentrated(_inputs(3, 9, 6, 2003), j)
    for w in (_wild_prior, _wild_value, _wild_reward):
        yield w.__name__, w(_inputs(3, 9, 6, 3003))
    yield "S70", _inputs(2, 9, 70, 6070)
    yield "S200", _inputs(2, 9, 200, 6200)


def test_port_matches_reference_on_these_inputs(ref_lib, port_lib):
    from mazero_amd.synthetic import run_search

    for name, inp in _port_vs_ref_inputs():
        outs = [run_search(make_tb(lib, inp, K, {}), inp, K, {}) for lib in (ref_lib, port_lib)]
        assert_same(outs[1], outs[0], f"port vs ref {name}: ")
