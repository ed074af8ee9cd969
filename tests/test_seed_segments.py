"""Per-segment tree seeds of a handle (include/mzdriver.h: mz_set_seed_segments, mz_get_seed_segments;
Tree_batch.set_seed_segments / seed_segments).  GPU tests need an MI355X: `pytest -m gpu`.

Tree t of segment g is the tree of a fresh Tree_batch(..., seeds[g], root_offset=root_offsets[g]) at row
t - first_tree[g].  The product handle of 7 trees in segments of 3, 1 and 3 (seeds 5, 200 and 5, offsets
0, 0 and 3: the last segment continues the first one's batch) is compared with one CPU-port handle per
segment, every selection and every getter, bit for bit, for each prepare kernel and layout that reads the
seed: k_prepare1 (K = 1), k_prepare (K = 5; the same with MZ_HBM=1; N = 2 joint trees; A = 100) and a
segment whose offset puts its seed values past the seeding checkpoints (the sequential chain).  Then: one
segment (seed, 0) is the unsegmented handle; n = 0 returns the handle to its seed words; a recorded
one-search graph follows the segments between replays; argument errors change nothing.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import gpu_lib  # noqa: F401  (fixture)

torch = pytest.importorskip("torch")

B, S = 7, 8
FIRST, SEEDS, OFFS = [0, 3, 4], [5, 200, 5], [0, 0, 3]
C2, C1, DISC = 19652.0, 1.25, 0.997
LISTS = ("actions", "visit_count", "pred_probs", "beta", "beta_hat", "priors", "imp_ratio", "pred_values",
         "mcts_values", "rewards")
# name: (N, A, K, environment switch read at mz_create, the prepare kernel, the segments' root offsets)
CONFIGS = {
    "prepare1_k1": (1, 9, 1, None, "k_prepare1", OFFS),
    "general_k5": (1, 9, 5, None, "k_prepare", OFFS),
    "hbm_k5": (1, 9, 5, "MZ_HBM", "k_prepare", OFFS),
    "joint_n2": (2, 9, 3, None, "k_prepare", OFFS),
    "wide_a100": (1, 100, 5, None, "k_prepare", OFFS),
    # seed values of 200 * 2333 + 50,000,000 + i: far past any seeding table (160 bytes a row)
    "chain_k1": (1, 9, 1, None, "k_prepare1", [0, 50_000_000, 3]),
    "chain_k5": (1, 9, 5, None, "k_prepare", [0, 50_000_000, 3]),
}
_PORT = {}


def _inputs(N, A, seed=77):
    """Fixed synthetic inputs of one search of B roots: [B, N, A] policies, [B] rewards and values."""
    rng = np.random.default_rng(seed)
    pol = lambda: rng.dirichlet([1.0] * A, (B, N)).astype(np.float32)  # noqa: E731
    sc = lambda s: (s * rng.standard_normal(B)).astype(np.float32)  # noqa: E731
    return dict(root=(sc(0.1), sc(1.0), pol(), pol(), rng.dirichlet([0.3] * A, (B, N)).astype(np.float32)),
                sims=[(sc(0.1), sc(1.0), pol(), pol()) for _ in range(S)])


def _rows(inp, lo, hi):
    return dict(root=tuple(a[lo:hi] for a in inp["root"]), sims=[tuple(a[lo:hi] for a in s) for s in inp["sims"]])


def _readbacks(tb):
    out = dict(values=tb.get_roots_values(), mv=tb.get_roots_marginal_visit_count(),
               mp=tb.get_roots_marginal_priors(), qvalues=tb.get_roots_sampled_qvalues(DISC))
    for f in LISTS:
        out[f] = getattr(tb, "get_roots_sampled_" + f)()
    return out


def _search(tb, inp, K):
    """One search through the host surface (the reference driver's calls): every selection, every getter."""
    tb.prepare(*inp["root"][:4], K, 0.25, inp["root"][4])
    sel = []
    for s in range(S):
        ix, iy, act = tb.batch_selection(C2, C1, DISC)
        assert list(iy) == list(range(len(ix)))
        sel.append((np.asarray(ix, np.int32), np.asarray(act, np.int32).copy()))
        tb.batch_expansion_and_backup(s + 1, DISC, K, *inp["sims"][s])
    out = _readbacks(tb)
    out["sel_idx"] = np.stack([s[0] for s in sel], 1)  # [rows, S]
    out["sel_act"] = np.stack([s[1] for s in sel], 1)  # [rows, S, N]
    return out


def _port_segment(port_lib, cfg, inp_seed, g, segs):
    """The CPU port's search of segment g: its own handle (B_g, seed_g, root_offset_g).  Computed once."""
    from mazero_amd.cytree import Tree_batch

    first, seeds, offs = segs
    N, A, K = CONFIGS[cfg][:3]
    lo, hi = first[g], (first[g + 1] if g + 1 < len(first) else B)
    key = (N, A, K, inp_seed, lo, hi, seeds[g], offs[g])
    if key not in _PORT:
        tb = Tree_batch(hi - lo, N, A, K, S, 0.01, seeds[g], 0.75, 0.8, root_offset=offs[g], lib=port_lib)
        _PORT[key] = _search(tb, _rows(_inputs(N, A, inp_seed), lo, hi), K)
    return lo, hi, _PORT[key]


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_rows(got, want, lo, hi, where):
    for k, w in want.items():
        g = got[k][lo:hi]
        if isinstance(w, list):
            assert len(g) == len(w) and all(_bits(x, y) for x, y in zip(g, w)), f"{where}: {k}"
        else:
            assert _bits(g, w), f"{where}: {k}"


def _assert_segments(port_lib, cfg, inp_seed, got, segs, where=""):
    for g in range(len(segs[0])):
        lo, hi, want = _port_segment(port_lib, cfg, inp_seed, g, segs)
        _assert_rows(got, want, lo, hi, f"{where}{cfg} segment {g} rows [{lo}:{hi})")


def _handle(gpu_lib, cfg, seed, monkeypatch):  # noqa: F811
    from mazero_amd.cytree import Tree_batch

    N, A, K, env, name, _ = CONFIGS[cfg]
    if env:
        monkeypatch.setenv(env, "1")
    tb = Tree_batch(B, N, A, K, S, 0.01, seed, 0.75, 0.8, lib=gpu_lib)
    if env:
        monkeypatch.delenv(env)
    assert tb.prepare_kernel() == name
    return tb


# ------------------------------------------------------------------------------------------ CPU
def test_oracle_libraries_lack_the_calls(port_lib):
    """The oracle libraries do not export the entry points: the wrapper says so, and reports no segments."""
    from mazero_amd.cytree import Tree_batch

    assert not hasattr(port_lib, "mz_set_seed_segments") and not hasattr(port_lib, "mz_get_seed_segments")
    tb = Tree_batch(4, 1, 3, 1, 2, 0.01, 0, 0.75, 0.8, lib=port_lib)
    assert tb.seed_segments == ([], [], [])
    with pytest.raises(RuntimeError, match="mz_set_seed_segments"):
        tb.set_seed_segments([0, 2], [1, 2])


def test_bindings_declared():
    from mazero_amd import _capi

    for name in ("mz_set_seed_segments", "mz_get_seed_segments"):
        assert name in _capi.DRIVER_EXPORTS and _capi.DRIVER_SIGNATURES[name][0] is C.c_int


# ------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_segments_are_the_ports_handles(gpu_lib, port_lib, cfg, monkeypatch):  # noqa: F811
    N, A, K, _, name, offs = CONFIGS[cfg]
    segs = (FIRST, SEEDS, offs)
    tb = _handle(gpu_lib, cfg, 91, monkeypatch)  # (the handle's own seed is not any segment's)
    assert tb.seed_segments == ([], [], [])
    tb.set_seed_segments(*segs)
    assert tb.seed_segments == tuple(list(x) for x in segs) and tb.prepare_kernel() == name
    for rep, inp_seed in enumerate((77, 78)):  # a second search on the same handle and segments
        got = _search(tb, _inputs(N, A, inp_seed), K)
        tb.synchronize()  # (raises on a non-zero error word)
        _assert_segments(port_lib, cfg, inp_seed, got, segs, f"search {rep}: ")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["prepare1_k1", "general_k5"])
def test_one_segment_is_the_unsegmented_handle(gpu_lib, cfg, monkeypatch):  # noqa: F811
    N, A, K = CONFIGS[cfg][:3]
    inp = _inputs(N, A)
    plain = _search(_handle(gpu_lib, cfg, 200, monkeypatch), inp, K)
    tb = _handle(gpu_lib, cfg, 3, monkeypatch)
    tb.set_seed_segments([0], [200], [0])
    got = _search(tb, inp, K)
    _assert_rows(got, plain, 0, B, f"{cfg}: one segment (200, 0)")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["prepare1_k1", "general_k5"])
def test_no_segments_is_a_plain_reseed(gpu_lib, port_lib, cfg, monkeypatch):  # noqa: F811
    """mz_reseed and mz_set_root_offset keep writing the handle's words under segments; n = 0 returns to
    them."""
    N, A, K = CONFIGS[cfg][:3]
    tb = _handle(gpu_lib, cfg, 91, monkeypatch)
    tb.set_seed_segments(FIRST, SEEDS, OFFS)
    _assert_segments(port_lib, cfg, 77, _search(tb, _inputs(N, A), K), (FIRST, SEEDS, OFFS))
    tb.reseed(200)
    tb.set_root_offset(2)
    assert tb.seed_segments[0] == FIRST and tb.root_offset == 2
    _assert_segments(port_lib, cfg, 77, _search(tb, _inputs(N, A), K), (FIRST, SEEDS, OFFS), "after reseed: ")
    tb.set_seed_segments([], [])
    assert tb.seed_segments == ([], [], [])
    got = _search(tb, _inputs(N, A), K)
    _assert_segments(port_lib, cfg, 77, got, ([0], [200], [2]), "n = 0: ")


@pytest.mark.gpu
def test_replayed_graph_reads_the_table(gpu_lib, port_lib, monkeypatch):  # noqa: F811
    """A one-search graph recorded under segments, replayed after the segments changed."""
    cfg = "prepare1_k1"
    N, A, K = CONFIGS[cfg][:3]
    inp = _inputs(N, A)
    dev = torch.device("cuda")
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    root = [f(a) for a in inp["root"]]
    sims = [[f(a) for a in s] for s in inp["sims"]]
    idx = torch.zeros(S, B, dtype=torch.int32, device=dev)
    idy = torch.zeros(S, B, dtype=torch.int32, device=dev)
    act = torch.zeros(S, B, 1, dtype=torch.int32, device=dev)
    tb = _handle(gpu_lib, cfg, 91, monkeypatch)
    first = (FIRST, SEEDS, OFFS)
    second = ([0, 2, 6], [17, 5, 200], [4, 1, 0])
    tb.set_seed_segments(*first)

    def sequence():
        tb.prepare_selection_device(root[0], root[1], root[2], root[3], K, 0.25, root[4], C2, C1, DISC,
                                    out=(idx[0], idy[0], act[0]))
        for s in range(S):
            if s + 1 < S:
                tb.expansion_backup_selection_device(s + 1, DISC, K, *sims[s], C2, C1,
                                                     out=(idx[s + 1], idy[s + 1], act[s + 1]))
            else:
                tb.batch_expansion_and_backup(s + 1, DISC, K, *sims[s])

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        sequence()  # (eager once: the handle's tables are in place before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        sequence()
    for segs in (first, second, first):
        with torch.cuda.stream(stream):
            tb.set_seed_segments(*segs)
            graph.replay()
            tb.state_changed()
            got = _readbacks(tb)
        torch.cuda.synchronize()
        got["sel_idx"] = idx.cpu().numpy().T.copy()
        got["sel_act"] = act.cpu().numpy().transpose(1, 0, 2).copy()
        _assert_segments(port_lib, cfg, 77, got, segs, f"replay under {segs}: ")
    tb.synchronize()


@pytest.mark.gpu
def test_argument_errors_change_nothing(gpu_lib, port_lib, monkeypatch):  # noqa: F811
    from mazero_amd._capi import MZ_ERR_ARG

    cfg = "general_k5"
    N, A, K = CONFIGS[cfg][:3]
    tb = _handle(gpu_lib, cfg, 91, monkeypatch)
    tb.set_seed_segments(FIRST, SEEDS, OFFS)
    done = _search(tb, _inputs(N, A), K)
    lib, h = tb._lib, tb._h
    i32 = lambda xs: (C.c_int32 * len(xs))(*xs)  # noqa: E731
    u32 = lambda xs: (C.c_uint32 * len(xs))(*xs)  # noqa: E731
    int_max = (1 << 31) - 1
    bad = [
        (2, [1, 4], [1, 2], [0, 0]),                # first_tree[0] != 0
        (3, [0, 4, 4], [1, 2, 3], [0, 0, 0]),       # not strictly increasing
        (3, [0, 5, 3], [1, 2, 3], [0, 0, 0]),
        (2, [0, B], [1, 2], [0, 0]),                # a segment that starts past the last tree
        (2, [0, 3], [1, 2], [0, -1]),               # a negative offset
        (2, [0, 3], [1, 2], [0, int_max - 3]),      # offset + the segment's 4 trees > INT32_MAX
        (-1, [0], [1], [0]),
    ]
    for n, first, seeds, offs in bad:
        assert lib.mz_set_seed_segments(h, n, i32(first), u32(seeds), i32(offs)) == MZ_ERR_ARG, (n, first, offs)
    assert lib.mz_set_seed_segments(h, B + 1, i32(list(range(B + 1))), u32([0] * (B + 1)), i32([0] * (B + 1))) == MZ_ERR_ARG
    assert lib.mz_set_seed_segments(None, 0, None, None, None) == MZ_ERR_ARG
    assert lib.mz_set_seed_segments(h, 1, None, u32([1]), i32([0])) == MZ_ERR_ARG
    n = C.c_int(-1)
    assert lib.mz_get_seed_segments(h, 0, None, None, None, None) == MZ_ERR_ARG
    assert lib.mz_get_seed_segments(None, 0, C.byref(n), None, None, None) == MZ_ERR_ARG
    assert lib.mz_get_seed_segments(h, 3, C.byref(n), None, None, None) == MZ_ERR_ARG
    with pytest.raises(ValueError):
        tb.set_seed_segments([0, 9], [1, 2])
    with pytest.raises(ValueError):
        tb.set_seed_segments([0, 1], [1, 2], [0])
    # the segments and the finished search are as they were
    assert lib.mz_get_seed_segments(h, 0, C.byref(n), None, None, None) == 0 and n.value == 3
    assert tb.seed_segments == (FIRST, SEEDS, OFFS)
    _assert_rows(_readbacks(tb), {k: v for k, v in done.items() if not k.startswith("sel_")}, 0, B, "after the errors")
    # the largest offset taken: offset + the segment's trees == INT32_MAX; the next search is theirs
    tb.set_seed_segments([0, 3], [5, 200], [0, int_max - 4])
    assert tb.seed_segments == ([0, 3], [5, 200], [0, int_max - 4])
    tb.set_seed_segments(FIRST, SEEDS, OFFS)
    _assert_segments(port_lib, cfg, 77, _search(tb, _inputs(N, A), K), (FIRST, SEEDS, OFFS), "after the errors: ")
