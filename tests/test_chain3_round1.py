"""k_chain3's round 1 (needs an MI355X: `pytest -m gpu`).

Every address a wave loads in round 1 follows from the preloaded launch arguments: the tree headers
are 256-byte blocks right after Params, the lambda-power table and the node arrays follow at
offsets computed from B, PS and B * P.  The header's first 64-byte line carries a copy of the root's
visit count and the leaf's Bn.y, tagged with the tot it was written at; k_prepare and k_chain3
maintain it, every other header writer invalidates it, and a launch that finds no valid copy loads
the two records instead.  The handle constants the roles read arrive as launch arguments.

Every case runs K = 1 searches against the CPU port, bit for bit: per launch idx, idy, act and the
gathered row; at the end every readback, the event counters against the same search on k_chain
(MZ_CHAIN_V2=1) and the error word.  The shapes are the smallest that take each path.
"""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import pytest

from conftest import assert_same
from test_gpu_parity import gpu_lib, make_tb, run_fused, to_device  # noqa: F401  (gpu_lib: fixture)

torch = pytest.importorskip("torch")

K = 1
COUNTERS = ("selects", "path_edges", "scored", "expands", "new_children", "backup_nodes", "minmax_nodes")


def _inputs(B, A, S, seed):
    from mazero_amd.synthetic import make_search_inputs

    return make_search_inputs(np.random.default_rng(seed), B, A, S)


def _consts():
    from mazero_amd.synthetic import DEFAULTS

    return DEFAULTS["pb_c_base"], DEFAULTS["pb_c_init"], DEFAULTS["discount"]


def _pool(inp, H=384, seed=0):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return torch.randn(inp.S + 1, inp.B, H, device="cuda", generator=gen)


def _port(port_lib, inp, n_sims=None, hsx_of=None, select_last=False):
    """The CPU port through the reference's call sequence: the selections [n_sims (+1), B] and the readbacks."""
    from mazero_amd.synthetic import readbacks

    c2, c1, g = _consts()
    n = inp.S if n_sims is None else n_sims
    hsx_of = hsx_of or (lambda s: s + 1)
    ref = make_tb(port_lib, inp, K, {})
    ref.prepare(inp.root_reward, inp.root_value, inp.root_policy, inp.root_beta, K, inp.noise_eps, inp.root_noise)
    idx, act = [], []
    for s in range(n + (1 if select_last else 0)):
        ix, iy, a = ref.batch_selection(c2, c1, g)
        assert list(iy) == list(range(inp.B))
        idx.append(np.asarray(ix, np.int32))
        act.append(np.asarray(a, np.int32).reshape(inp.B))
        if s < n:
            ref.batch_expansion_and_backup(hsx_of(s), g, K, inp.reward[s], inp.value[s], inp.policy[s], inp.beta[s])
    out = dict(sel_idx=np.stack(idx), sel_act=np.stack(act))
    out.update(readbacks(ref, g))
    return out


def _drive(tb, inp, modes, first="prepare", pool=None, hsx_of=None, last="plain", select_last=False):
    """One search on the product.  modes[s] says how simulation s's expansion and the selection after
    it are issued: "fused" (one k_chain3 launch), "device" (mz_expand_backup then mz_select on device
    tensors) or "host" (the numpy path).  first: "prepare" (+ a selection) or "prepare_select" (one
    launch).  last: the last expansion "plain" or "packed" (fused with the readback); select_last:
    the last simulation is followed by a selection like the others."""
    from mazero_amd.synthetic import readbacks

    c2, c1, g = _consts()
    d = to_device(inp)
    n, B = len(modes), inp.B
    hsx_of = hsx_of or (lambda s: s + 1)
    dev = torch.device("cuda")
    rows = n + (1 if select_last else 0)
    idx = torch.zeros(rows, B, dtype=torch.int32, device=dev)
    idy = torch.zeros(rows, B, dtype=torch.int32, device=dev)
    act = torch.zeros(rows, B, 1, dtype=torch.int32, device=dev)
    gathered = None if pool is None else torch.zeros((rows,) + tuple(pool.shape[1:]), dtype=pool.dtype, device=dev)
    if first == "prepare_select":
        tb.prepare_selection_device(d.root_reward, d.root_value, d.root_policy, d.root_beta, K, d.noise_eps, d.root_noise,
                                    c2, c1, g, out=(idx[0], idy[0], act[0]))
    else:
        tb.prepare(d.root_reward, d.root_value, d.root_policy, d.root_beta, K, d.noise_eps, d.root_noise)
        tb.batch_selection_device(c2, c1, g, out=(idx[0], idy[0], act[0]))
    if pool is not None:
        tb.gather_rows(pool, idx[0], gathered[0])
    for s, m in enumerate(modes):
        hsx = hsx_of(s)
        if s + 1 == n and not select_last:
            if last == "packed":
                tb.expansion_backup_readback_device(hsx, g, K, d.reward[s], d.value[s], d.policy[s], d.beta[s],
                                                    readback_discount=g, out=None)
            else:
                tb.batch_expansion_and_backup(hsx, g, K, d.reward[s], d.value[s], d.policy[s], d.beta[s])
            break
        o = (idx[s + 1], idy[s + 1], act[s + 1])
        if m == "fused":
            tb.expansion_backup_selection_device(hsx, g, K, d.reward[s], d.value[s], d.policy[s], d.beta[s], c2, c1, out=o,
                                                 pool=pool, gather_out=None if pool is None else gathered[s + 1])
            continue
        if m == "device":
            tb.batch_expansion_and_backup(hsx, g, K, d.reward[s], d.value[s], d.policy[s], d.beta[s])
            tb.batch_selection_device(c2, c1, g, out=o)
        else:
            tb.batch_expansion_and_backup(hsx, g, K, inp.reward[s], inp.value[s], inp.policy[s], inp.beta[s])
            ix, iy, a = tb.batch_selection(c2, c1, g)
            idx[s + 1].copy_(torch.tensor(ix, dtype=torch.int32))
            idy[s + 1].copy_(torch.tensor(iy, dtype=torch.int32))
            act[s + 1].copy_(torch.from_numpy(np.asarray(a, np.int32).reshape(B, 1)))
        if pool is not None:
            tb.gather_rows(pool, idx[s + 1], gathered[s + 1])
    torch.cuda.synchronize()
    assert (idy.cpu().numpy() == np.arange(B, dtype=np.int32)[None]).all()
    out = dict(sel_idx=idx.cpu().numpy(), sel_act=act.cpu().numpy()[:, :, 0])
    if not select_last:
        out.update(readbacks(tb, g))
    return out, gathered


def _rows_ok(pool, out, gathered, where):
    rows = torch.arange(pool.shape[1], device="cuda")
    for s in range(out["sel_idx"].shape[0]):
        want = pool[torch.from_numpy(out["sel_idx"][s]).cuda().long(), rows]
        assert torch.equal(gathered[s].view(torch.int32), want.view(torch.int32)), f"{where}gathered row, launch {s}"


def _chain_v2(gpu_lib, inp, monkeypatch):
    monkeypatch.setenv("MZ_CHAIN_V2", "1")  # (read at mz_create)
    tb = make_tb(gpu_lib, inp, K, {})
    monkeypatch.delenv("MZ_CHAIN_V2")
    assert tb.fused_kernel().startswith("k_chain<")
    return tb


def _same_counters(tb, tb2, where):
    a, b = tb.stats(), tb2.stats()
    print(where, {k: a[k] for k in COUNTERS})
    assert {k: a[k] for k in COUNTERS} == {k: b[k] for k in COUNTERS}, where


def _check(gpu_lib, port_lib, inp, monkeypatch, kernel="k_chain3<64>", first="prepare_select", last="plain", modes=None,
           H=384):
    modes = modes or ["fused"] * inp.S
    where = f"B={inp.B} A={inp.A} S={inp.S} first={first} last={last}: "
    exp = _port(port_lib, inp)
    tb = make_tb(gpu_lib, inp, K, {})
    assert tb.fused_kernel() == kernel
    pool = _pool(inp, H)
    out, gathered = _drive(tb, inp, modes, first=first, pool=pool, last=last)
    assert_same(out, exp, where)
    _rows_ok(pool, out, gathered, where)
    tb.synchronize()  # (raises on a non-zero error word)
    tb2 = _chain_v2(gpu_lib, inp, monkeypatch)
    out2, _ = _drive(tb2, inp, modes, first=first, pool=pool, last=last)
    assert_same(out2, exp, where + "k_chain ")
    _same_counters(tb, tb2, where)
    return tb


# ---- the arena layout: B * P off every 16- and 64-record boundary, every action-count class ----
@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 2, 9, 36])
@pytest.mark.parametrize("B", [1, 3, 5, 65])
def test_layout_rounding(gpu_lib, port_lib, B, A, monkeypatch):
    _check(gpu_lib, port_lib, _inputs(B, A, 6, 100 * B + A), monkeypatch)


# ---- node classes 128 and 256 ----
@pytest.mark.gpu
@pytest.mark.parametrize("S,kernel", [(70, "k_chain3<128>"), (200, "k_chain3<256>")])
def test_node_classes(gpu_lib, port_lib, S, kernel, monkeypatch):
    _check(gpu_lib, port_lib, _inputs(3, 9, S, 600 + S), monkeypatch, kernel=kernel)


# ---- the hot copy invalidated by a step on another kernel, then valid again ----
@pytest.mark.gpu
@pytest.mark.parametrize("first", ["prepare", "prepare_select"])
@pytest.mark.parametrize("other", ["host", "device"])
def test_hot_copy_invalidated(gpu_lib, port_lib, other, first, monkeypatch):
    # fused launches, one (then two) steps through the other path, fused launches again: the first
    # fused launch after them finds no valid copy and loads the records, the following ones find one
    modes = ["fused", "fused", other, "fused", "fused", other, other, "fused", "fused", "fused"]
    for B in (1, 3):
        _check(gpu_lib, port_lib, _inputs(B, 9, len(modes), 700 + B), monkeypatch, first=first, modes=modes)


# ---- a launch whose slot argument disagrees with the header's leaf ----
@pytest.mark.gpu
@pytest.mark.parametrize("hsx_of", [lambda s: min(s + 1, 2), lambda s: 1000 + s], ids=["behind", "beyond_the_pool"])
def test_launch_out_of_sequence(gpu_lib, port_lib, hsx_of):
    inp = _inputs(3, 9, 6, 800)
    exp = _port(port_lib, inp, hsx_of=hsx_of)
    tb = make_tb(gpu_lib, inp, K, {})
    assert tb.fused_kernel() == "k_chain3<64>"
    out, _ = _drive(tb, inp, ["fused"] * inp.S, first="prepare_select", hsx_of=hsx_of)
    assert_same(out, exp, "out of sequence: ")
    tb.synchronize()


# ---- two searches on one handle: k_prepare resets the hot copy ----
@pytest.mark.gpu
@pytest.mark.parametrize("first", ["prepare", "prepare_select"])
def test_two_searches_on_one_handle(gpu_lib, port_lib, first):
    B, A, S = 3, 9, 6
    inp1 = _inputs(B, A, S, 900)
    inp2 = replace(_inputs(B, A, S, 901), seed=inp1.seed + 12345)
    tb = make_tb(gpu_lib, inp1, K, {})
    assert tb.fused_kernel() == "k_chain3<64>"
    # the first search stops after four fused launches: a valid copy of a deeper chain is left behind
    out, _ = _drive(tb, inp1, ["fused"] * 4, first=first, select_last=True)
    exp = _port(port_lib, inp1, n_sims=4, select_last=True)
    assert_same(out, {k: exp[k] for k in ("sel_idx", "sel_act")}, "first search: ")
    tb.reseed(inp2.seed)
    out, _ = _drive(tb, inp2, ["fused"] * S, first=first)
    assert_same(out, _port(port_lib, inp2), "second search: ")
    tb.synchronize()


def _error_word(tb):
    from mazero_amd._capi import MZError

    with pytest.raises(MZError) as e:
        tb.synchronize()
    msg = str(e.value)
    return int(msg.split("device error word 0x")[1].split(")")[0], 16), msg


# ---- handled errors: one launch more than the pool allows, then a tree already dead ----
@pytest.mark.gpu
def test_handled_errors(gpu_lib, monkeypatch):
    B, A, S = 3, 9, 6
    inp = _inputs(B, A, S, 1000)
    n = S + 6  # (the pool is sized for simulation_num: a launch soon after overflows; the rest hit dead trees)
    long_inp = replace(inp, reward=np.resize(inp.reward, (n,) + inp.reward.shape[1:]),
                       value=np.resize(inp.value, (n,) + inp.value.shape[1:]),
                       policy=np.resize(inp.policy, (n,) + inp.policy.shape[1:]),
                       beta=np.resize(inp.beta, (n,) + inp.beta.shape[1:]))
    tb = make_tb(gpu_lib, inp, K, {})
    assert tb.fused_kernel() == "k_chain3<64>"
    tb2 = _chain_v2(gpu_lib, inp, monkeypatch)
    outs, words = [], []
    for h in (tb, tb2):
        out, _ = _drive(h, long_inp, ["fused"] * n, first="prepare_select", select_last=True)
        outs.append(out)
        words.append(_error_word(h))
    assert_same(outs[0], outs[1], "past the pool: ")
    print("error word past the pool:", hex(words[0][0]))
    assert words[0][0] == words[1][0] and words[0][0] & 1 and "node pool exhausted" in words[0][1], words
    # the refused launch and the dead trees after it: the outputs zero
    assert (outs[0]["sel_idx"][-3:] == 0).all() and (outs[0]["sel_act"][-3:] == 0).all()
    assert (outs[0]["sel_idx"][:S] == np.arange(S, dtype=np.int32)[:, None]).all()


# ---- the last launch, with and without the fused readback ----
@pytest.mark.gpu
@pytest.mark.parametrize("last", ["plain", "packed"])
@pytest.mark.parametrize("first", ["prepare", "prepare_select"])
def test_last_launch(gpu_lib, port_lib, first, last, monkeypatch):
    for B in (1, 3):
        _check(gpu_lib, port_lib, _inputs(B, 9, 6, 1100 + B), monkeypatch, first=first, last=last)
    # S = 1: the only expansion's leaf is the root's child, straight after k_prepare
    _check(gpu_lib, port_lib, _inputs(3, 9, 1, 1110), monkeypatch, first=first, last=last)
