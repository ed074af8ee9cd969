"""k_chain3's draw wave (needs an MI355X: `pytest -m gpu`).

In the 64-node class, with one workgroup per CU at most, k_chain3 runs four waves (the larger
node classes only under MZ_CHAIN3_W4, which their cases here set): wave 3 builds the expansion's
distribution and draws the action from launch start, beside wave 0's round 1, and hands the action
to wave 0 through one LDS dword that wave 0 cleared ahead of a start barrier all four waves take.
Wave 0 polls the dword a bounded number of times and draws itself if the bound runs out.

Every case runs K = 1 searches through the fused device loop against the CPU port, bit for bit:
per launch idx, idy, act and the gathered row; at the end every readback and the error word.  Each
asserts that the handle launches the four-wave kernel (`fused_waves`).  The shapes are the smallest
that take each path of the distribution (4, 8, 12, 16 terms and the long form), each node and row
class, the exact selection with wave 0's later barrier, the fused readback, a replay out of
sequence and the error paths.

The last-action case: the issue asks for a row whose last entries are tiny "so that the draw lands
on the last action through the cp = 1.0 rule".  The draw's u comes from the tree's engine words and
cannot be steered, so two rows cover the rule: one with all but 1e-6 of the weight on the last
action (the draw lands there, on the lane whose cumulative probability is forced to 1.0), and one
whose last three weights are 1e-30 of the rest (the prefix sums before the forced 1.0 sit within
rounding of it).  Both are compared with the port like every other case.
"""
from __future__ import annotations

import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

if __name__ != "__main__":
    import test_chain3_round1 as round1
    import test_chain3_tail as tail
    from edge_inputs import tiny_tail as _tiny_tail
    from test_gpu_parity import gpu_lib, make_tb, to_device  # noqa: F401  (gpu_lib: fixture)

    torch = pytest.importorskip("torch")

K = 1
S = 20
# the searches the two builds run against each other in child processes: (B, A, S, H, seed)
CHILD_CASES = [(3, 9, 20, 384, 9100), (5, 36, 20, 1028, 9101), (2, 1, 6, 0, 9102), (300, 9, 6, 4, 9103)]


def _inputs(B, A, S_, seed, **kw):
    from mazero_amd.synthetic import make_search_inputs

    return make_search_inputs(np.random.default_rng(seed), B, A, S_, **kw)


def _check4(gpu_lib, port_lib, inp, **kw):  # noqa: F811
    tb = tail._check(gpu_lib, port_lib, inp, **kw)
    assert tb.fused_waves() == 4, "the handle did not take the four-wave kernel"
    return tb


# ---- action counts: no draw, both ends of every cdf_terms class, cdf_long ----
@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 2, 4, 5, 9, 12, 13, 16, 17, 36, 64])
def test_action_counts(gpu_lib, port_lib, A, monkeypatch):  # noqa: F811
    _check4(gpu_lib, port_lib, _inputs(5, A, S, 100 + A), monkeypatch=monkeypatch)


# ---- legal-action masks: zero beta entries ----
@pytest.mark.gpu
def test_masked_actions(gpu_lib, port_lib):  # noqa: F811
    inp = _inputs(5, 13, S, 200, legal_zero_frac=0.4)  # (masks the root's row)
    # the same kind of mask on every simulation's row: action 0 illegal, action 1 legal, 40 % of the rest
    legal = np.random.default_rng(201).random(inp.beta.shape) >= 0.4
    legal[..., 0] = False
    legal[..., 1] = True
    inp = replace(inp, policy=np.where(legal, inp.policy, np.float32(0)), beta=np.where(legal, inp.beta, np.float32(0)))
    assert (inp.beta == 0).any() and (inp.beta[..., -1] == 0).any()
    _check4(gpu_lib, port_lib, inp)


# ---- the last action: the forced cp = 1.0 (see the module docstring) ----
@pytest.mark.gpu
@pytest.mark.parametrize("row", ["concentrated", "tiny_tail"])
def test_last_action(gpu_lib, port_lib, row):  # noqa: F811
    A = 9
    inp = _inputs(5, A, S, 300)
    inp = tail._concentrated(inp, A - 1) if row == "concentrated" else _tiny_tail(inp)
    _check4(gpu_lib, port_lib, inp)
    if row == "concentrated":
        assert (tail._expected(port_lib, inp)["sel_act"][1:] == A - 1).all()  # (it draws what it is named for)


# ---- node classes 128 and 256 ----
@pytest.mark.gpu
@pytest.mark.parametrize("S_,kernel", [(70, "k_chain3<128>"), (200, "k_chain3<256>")])
def test_node_classes(gpu_lib, port_lib, S_, kernel, monkeypatch):  # noqa: F811
    # these classes keep the three-wave kernel by default (wave 1 ends last in their longer chains);
    # MZ_CHAIN3_W4 (read at mz_create) takes the four-wave instantiations
    inp = _inputs(2, 9, S_, 400 + S_)
    assert make_tb(gpu_lib, inp, K, {}).fused_waves() == 3
    monkeypatch.setenv("MZ_CHAIN3_W4", "1")
    _check4(gpu_lib, port_lib, inp, kernel=kernel)


# ---- row classes 0 (unaligned pool), 1, 2 (a row past 4 KiB), 3 (no pool) ----
@pytest.mark.gpu
@pytest.mark.parametrize("H", [5, 384, 1028, 0], ids=["class0_20B", "class1_1536B", "class2_4112B", "class3_no_pool"])
def test_row_classes(gpu_lib, port_lib, H):  # noqa: F811
    _check4(gpu_lib, port_lib, _inputs(3, 9, S, 500 + H), H=H)


# ---- not tame: the exact selection, wave 0's later barrier ----
@pytest.mark.gpu
@pytest.mark.parametrize("wild", ["prior", "value"])
def test_not_tame(gpu_lib, port_lib, wild, monkeypatch):  # noqa: F811
    f = tail._wild_prior if wild == "prior" else tail._wild_value
    _check4(gpu_lib, port_lib, f(_inputs(3, 9, S, 600)), monkeypatch=monkeypatch)


# ---- the last expansion fused with the readback (SEL = false) ----
@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 9])
def test_fused_readback(gpu_lib, port_lib, A):  # noqa: F811
    _check4(gpu_lib, port_lib, _inputs(3, A, S, 700 + A), fused_rb="packed")


# ---- one captured launch replayed out of sequence, a host-path step in between (no valid hot copy) ----
@pytest.mark.gpu
def test_graph_replayed_out_of_sequence_after_a_host_step(gpu_lib, port_lib):  # noqa: F811
    from mazero_amd.synthetic import DEFAULTS, readbacks

    B, A = 3, 9
    inp = _inputs(B, A, 8, 800)
    c2, c1, g = DEFAULTS["pb_c_base"], DEFAULTS["pb_c_init"], DEFAULTS["discount"]
    host_step = 4  # simulations 0, 1 launched; 2, 3 replayed; 4 on the host path; 5, 6 replayed
    n_sims = 7
    hsx_of = lambda s: s + 1 if s < 2 or s == host_step else 3  # noqa: E731  (the graph holds slot 3's launch)
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
    assert tb.fused_kernel() == "k_chain3<64>" and tb.fused_waves() == 4
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
        if s == host_step:
            with torch.cuda.stream(stream):
                tb.batch_expansion_and_backup(s + 1, g, K, inp.reward[s], inp.value[s], inp.policy[s], inp.beta[s])
                ix, iy, a = tb.batch_selection(c2, c1, g)
            torch.cuda.synchronize()
            got.append((list(ix), np.asarray(a).reshape(B).tolist()))
            continue
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


# ---- error paths: a pool exhausted mid-search, a dead tree re-reporting ----
@pytest.mark.gpu
def test_pool_exhausted_and_dead_tree(gpu_lib, port_lib, monkeypatch):  # noqa: F811
    probe = make_tb(gpu_lib, _inputs(3, 9, 6, 7000), K, {})
    assert probe.fused_kernel() == "k_chain3<64>" and probe.fused_waves() == 4  # (the handles below are alike)
    # launches up to and past the pool against the port: the error word set, the outputs zero, later
    # launches returning cleanly with the same word
    tail.test_past_the_pool(gpu_lib, port_lib)
    # six launches past the pool against k_chain: the searches end, the same outputs and word
    round1.test_handled_errors(gpu_lib, monkeypatch)


# ---- above the CU count the handle keeps the three-wave kernel ----
@pytest.mark.gpu
def test_more_workgroups_than_cus_keeps_three_waves(gpu_lib, port_lib):  # noqa: F811
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    inp = _inputs(cus + 1, 9, 6, 900)
    tb = tail._check(gpu_lib, port_lib, inp, H=4)
    assert tb.fused_waves() == 3
    assert make_tb(gpu_lib, _inputs(cus, 9, 6, 901), K, {}).fused_waves() == 4


# ---- the two builds against each other, in child processes (MZ_CHAIN3_W3 is read at mz_create) ----
def _child(path):
    import conftest  # noqa: F401  (the import path, the HIP runtime settings)
    import torch as th
    from mazero_amd._lib import load
    from test_gpu_parity import make_tb as mk, run_fused, to_device as dev_of

    lib = load()
    res = {}
    for n, (B, A, S_, H, seed) in enumerate(CHILD_CASES):
        inp = _inputs(B, A, S_, seed)
        tb = mk(lib, inp, K, {})
        gen = th.Generator(device="cuda")
        gen.manual_seed(n)
        pool = th.randn(S_ + 1, B, H, device="cuda", generator=gen) if H else None
        out, gathered = run_fused(tb, dev_of(inp), K, {}, pool=pool)
        tb.synchronize()
        res[f"c{n}_waves"] = np.int32(tb.fused_waves())
        res[f"c{n}_kernel"] = np.frombuffer(tb.fused_kernel().encode(), np.uint8)
        for k, v in out.items():
            res[f"c{n}_{k}"] = np.asarray(v)
        if gathered is not None:
            res[f"c{n}_gathered"] = gathered.cpu().numpy().view(np.int32)
    np.savez(path, **res)


@pytest.mark.gpu
def test_three_and_four_wave_builds_agree(tmp_path):
    outs = []
    for name, w3 in (("w4", None), ("w3", "1")):
        env = {k: v for k, v in os.environ.items() if k not in ("MZ_CHAIN3_W3", "MZ_CHAIN3_W4")}
        if w3:
            env["MZ_CHAIN3_W3"] = w3
        path = str(tmp_path / f"{name}.npz")
        r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), path], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(dict(np.load(path)))
    w4, w3 = outs
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for n, (B, *_rest) in enumerate(CHILD_CASES):
        assert int(w3[f"c{n}_waves"]) == 3
        assert int(w4[f"c{n}_waves"]) == (4 if B <= cus else 3), (n, B)
    assert set(w3) == set(w4)
    for k in w4:
        if k.endswith("_waves"):
            continue
        assert w3[k].shape == w4[k].shape and w3[k].dtype == w4[k].dtype, k
        assert np.array_equal(w3[k].view(np.uint8), w4[k].view(np.uint8)), k


if __name__ == "__main__":
    _child(sys.argv[1])
