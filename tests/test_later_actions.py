"""The later agents' greedy actions from a per-node cache (include/mzdriver.h: mz_policy_glue_later,
mz_joint_action_cached) and SampledMCTS(..., later_action_cache=True).

CPU tests pin the opt-in (constructor, config object, worker shards) and the ctypes signatures against
the header.  GPU tests compare the two kernels with the numpy expressions of the reference driver
(mcts_sampled.py:116-147,156-161), whole searches with and without the flag bit for bit and against
the oracle driver on the CPU port, count the `prediction` calls and the recorded graph's nodes, and
check the guard against a model whose `prediction` is not a function of the state.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_HEADER = os.path.join(ROOT, "include", "mzdriver.h")


# ------------------------------------------------------------------------------------------ CPU
def test_constructor_accepts_the_flag():
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=9)
    assert SampledMCTS(cfg, np.random.RandomState(0), later_action_cache=True).later_action_cache is True
    assert SampledMCTS(cfg, np.random.RandomState(0), later_action_cache=False).later_action_cache is False
    assert SampledMCTS(cfg, np.random.RandomState(0)).later_action_cache is False  # off by default


def test_flag_read_from_config():
    """A reference-style call SampledMCTS(config, np_random) opts in through its config object; an
    explicit argument wins."""
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=9)
    cfg.later_action_cache = True
    assert SampledMCTS(cfg, np.random.RandomState(0)).later_action_cache is True
    assert SampledMCTS(cfg, np.random.RandomState(0), later_action_cache=False).later_action_cache is False


def test_worker_shard_passes_the_flag():
    from mazero_amd.nets import SearchConfig
    from mazero_amd.workers import ReanalyzeShard, SelfPlayShard

    cfg = SearchConfig(action_space_size=9)
    sp = SelfPlayShard(None, cfg, 8, 2, seed=0, rank=1, world=2, later_action_cache=True)
    m = sp.make_mcts(sp.config, sp.np_random, sp.root_shard)
    assert m.later_action_cache and m.root_shard == (4, 8, 8)
    ra = ReanalyzeShard(None, cfg, 8, seed=0, rank=0, world=1)
    assert not ra.make_mcts(ra.config, ra.np_random, ra.root_shard).later_action_cache
    cfg.later_action_cache = True
    ra = ReanalyzeShard(None, cfg, 8, seed=0, rank=0, world=1)
    assert ra.make_mcts(ra.config, ra.np_random, ra.root_shard).later_action_cache


def test_ctypes_signatures_match_header():
    """The binding table's entries for the two entry points, argument by argument, against their
    declarations in include/mzdriver.h."""
    from mazero_amd import _capi

    txt = open(DRIVER_HEADER).read()
    ctype = {"mz_batch *": C.c_void_p, "const void *": C.c_void_p, "float *": C.c_void_p, "int32_t *": C.c_void_p,
             "const int32_t *": C.c_void_p, "int64_t *": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64,
             "double": C.c_double}
    want = {
        "mz_policy_glue_later": ["mz_batch *", "const void *", "int", "int64_t", "int", "int", "double", "float *",
                                 "float *", "int32_t *"],
        "mz_joint_action_cached": ["mz_batch *", "const int32_t *", "int", "const int32_t *", "int", "int",
                                   "const int32_t *", "int", "const int32_t *", "int64_t *"],
    }
    for name, types in want.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", txt, re.M)
        assert m, f"{name} is not declared"
        declared = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            declared.append(re.match(r"(.*?)(\w+)$", arg).group(1).strip())
        assert declared == types, name
        res, args = _capi.DRIVER_SIGNATURES[name]
        assert res is C.c_int and args == [ctype[t] for t in declared], name
        assert name in _capi.DRIVER_EXPORTS


# ------------------------------------------------------------------------------------------ GPU
def _u32(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _code(dtype):
    from mazero_amd._capi import MZ_DT_F16, MZ_DT_F32

    return MZ_DT_F16 if np.dtype(dtype) == np.float16 else MZ_DT_F32


def _numpy_policy_glue(logits, tau=1.0):
    """mcts_sampled.py:158-161 + astype(np.float32) (:169-170), in the logits' dtype."""
    p = np.exp(logits - np.max(logits, axis=-1, keepdims=True))
    p = p / np.sum(p, axis=-1, keepdims=True)
    b = p ** (1 / tau)
    b = b / np.sum(b, axis=-1, keepdims=True)
    return p.astype(np.float32), b.astype(np.float32)


def _half_exp_exceptions() -> np.ndarray:
    """Non-positive float16 values d where this host's np.exp(d) differs from np.exp in float32
    rounded to half (numpy's SIMD half loop; the softmax evaluates exp(x - max) <= 1): what
    ensure_half_exp hands the kernels a table for.  Empty on hosts without that loop."""
    x = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    x = x[np.isfinite(x) & (x <= 0)]
    with np.errstate(all="ignore"):
        diff = np.exp(x).view(np.uint16) != np.exp(x.astype(np.float32)).astype(np.float16).view(np.uint16)
    return x[diff]


@functools.lru_cache(maxsize=None)
def _handle(B, A):
    import torch

    from mazero_amd.cytree import Tree_batch
    from mazero_amd.mcts_sampled import ensure_half_exp

    tb = Tree_batch(B, 1, A, 1, 4, 0.01, 0, 0.75, 0.8)
    ensure_half_exp(tb._lib, torch.cuda.current_device())  # (as the search loop does)
    tb._sync_stream()
    return tb


def _later_case(rng, B, N, A, cur, dtype):
    """Logits [B, N, A].  The current agent's rows (the policy glue): random rows of several scales,
    rows with -inf entries, constant rows, a dominant logit and, in float16, rows whose x - max are the
    values where numpy's half exp is not float32 exp rounded.  Every other agent's rows (the argmax;
    agents before the current one are not read) cycle through: random, small integers (exact ties),
    all -inf, a NaN that is not in the first position behind a larger maximum, constant, the maximum
    twice with a NaN-free row; root 0 holds NaNs in its last two agents."""
    scale = np.array([1, 1, 0.1, 4, 30])[np.arange(B) % 5].reshape(B, 1, 1)
    x = (rng.standard_normal((B, N, A)) * scale).astype(dtype)
    exc = _half_exp_exceptions() if np.dtype(dtype) == np.float16 else np.zeros(0)
    for i in range(B):
        for k in range(N):
            kind = (i + k) % 6
            row = x[i, k]
            if k == cur:
                if kind == 1 and A > 1:
                    row[rng.choice(A, size=max(A // 3, 1), replace=False)] = -np.inf
                    row[rng.integers(A)] = 0.5  # (at least one finite logit)
                elif kind == 2:
                    row[:] = row[0]
                elif kind == 3:
                    row[rng.integers(A)] = 60.0
                elif kind == 4 and exc.size and A > 1:
                    row[:] = rng.choice(exc, size=A)
                    row[rng.integers(A)] = 0.0
                continue
            if kind == 1:
                row[:] = rng.integers(-3, 3, size=A)
            elif kind == 2:
                row[:] = -np.inf
            elif kind == 3:
                row[0] = 50.0
                row[min(1 + int(rng.integers(max(A - 1, 1))), A - 1)] = np.nan
            elif kind == 4:
                row[:] = row[0]
            elif kind == 5:
                row[rng.integers(A)] = 40.0
                row[rng.integers(A)] = 40.0
    for k in (N - 1, N - 2):
        if k != cur:
            x[0, k, A - 1] = np.nan
            x[0, k, A // 2] = np.nan
    return x


def _run_later(tb, logits, cur, tau, pad, glue=True, want_later=True):
    """mz_policy_glue_later on `logits` stored with a row stride of N * A + pad elements.  Returns
    (probs, beta, later); the outputs are prefilled with sentinels (-7.0, -9)."""
    import torch

    from mazero_amd._capi import check

    Bn, N, A = logits.shape
    dev = torch.device("cuda", 0)
    rows = np.full((Bn, N * A + pad), 3.0, logits.dtype)
    rows[:, : N * A] = logits.reshape(Bn, N * A)
    x = torch.from_numpy(rows).to(dev)
    probs, beta = torch.full((Bn, A), -7.0, device=dev), torch.full((Bn, A), -7.0, device=dev)
    later = torch.full((Bn, N), -9, dtype=torch.int32, device=dev)
    check(tb._lib, tb._lib.mz_policy_glue_later(
        tb._h, C.c_void_p(x.data_ptr()), _code(logits.dtype), N * A + pad, N, cur, tau,
        C.c_void_p(probs.data_ptr()) if glue else None, C.c_void_p(beta.data_ptr()) if glue else None,
        C.c_void_p(later.data_ptr()) if want_later else None), "policy_glue_later")
    return probs.cpu().numpy(), beta.cpu().numpy(), later.cpu().numpy()


def _expected_later(logits, cur):
    Bn, N, _ = logits.shape
    exp = np.full((Bn, N), -9, np.int32)  # columns <= cur keep the sentinel
    for k in range(cur + 1, N):
        exp[:, k] = np.argmax(logits[:, k, :], axis=-1)
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("A", [1, 2, 9, 63, 64, 65, 128, 129, 255])
def test_policy_glue_later_matches_numpy(A, dtype):
    """probs / beta against the numpy softmax and power of the current agent's row, byte for byte, and
    against mz_policy_glue(_wide) on the same buffer; later[:, k > cur] against np.argmax; every B, N,
    current agent and sampled_tau, contiguous and padded rows; the later-only mode (the root's slot)
    and the last agent without a later_out."""
    import torch

    from mazero_amd._capi import check

    rng = np.random.default_rng(17 * A + (np.dtype(dtype) == np.float16))
    for Bn in (1, 3, 65):
        tb = _handle(Bn, A)
        for N in (2, 3, 5, 27):
            for ci, cur in enumerate(sorted({0, 1, N - 2, N - 1})):
                logits = _later_case(rng, Bn, N, A, cur, dtype)
                want_later = _expected_later(logits, cur)
                for ti, tau in enumerate((1.0, 0.5)):
                    pad = 5 * ((ci + ti) % 2)  # contiguous and padded rows at either tau
                    where = f"B={Bn} N={N} cur={cur} A={A} {dtype} tau={tau} pad={pad}"
                    gp, gb, gl = _run_later(tb, logits, cur, tau, pad)
                    with np.errstate(all="ignore"):
                        ep, eb = _numpy_policy_glue(logits[:, cur:cur + 1, :], tau)
                    np.testing.assert_array_equal(_u32(gp), _u32(ep.reshape(Bn, A)), err_msg="probs " + where)
                    np.testing.assert_array_equal(_u32(gb), _u32(eb.reshape(Bn, A)), err_msg="beta " + where)
                    np.testing.assert_array_equal(gl, want_later, err_msg="later " + where)
                # the bytes of mz_policy_glue / mz_policy_glue_wide (tau = 0.5, the last of the loop)
                dev = torch.device("cuda", 0)
                x = torch.from_numpy(np.ascontiguousarray(logits)).to(dev)
                p0, b0 = torch.full((Bn, A), -7.0, device=dev), torch.full((Bn, A), -7.0, device=dev)
                fn = tb._lib.mz_policy_glue_wide if A > 64 else tb._lib.mz_policy_glue
                check(tb._lib, fn(tb._h, C.c_void_p(x.data_ptr()), _code(dtype), N * A, cur * A, 0.5,
                                  C.c_void_p(p0.data_ptr()), C.c_void_p(b0.data_ptr())), "policy_glue")
                gp, gb, _ = _run_later(tb, logits, cur, 0.5, 0)
                np.testing.assert_array_equal(_u32(gp), _u32(p0.cpu().numpy()))
                np.testing.assert_array_equal(_u32(gb), _u32(b0.cpu().numpy()))
                if cur + 1 < N:  # only the later agents: probs / beta keep their sentinel
                    gp, gb, gl = _run_later(tb, logits, cur, 1.0, 3, glue=False)
                    assert (gp == -7.0).all() and (gb == -7.0).all()
                    np.testing.assert_array_equal(gl, want_later)
                else:  # the last agent needs no later_out: mz_policy_glue
                    gp2, gb2, gl = _run_later(tb, logits, cur, 0.5, 0, want_later=False)
                    np.testing.assert_array_equal(_u32(gp2), _u32(gp))
                    np.testing.assert_array_equal(_u32(gb2), _u32(gb))
                    assert (gl == -9).all()


@pytest.mark.gpu
def test_policy_glue_later_argument_errors():
    import torch

    from mazero_amd._capi import MZ_DT_F32, MZ_ERR_ARG

    Bn, N, A = 3, 3, 9
    tb = _handle(Bn, A)
    lib, h = tb._lib, tb._h
    dev = torch.device("cuda", 0)
    x = torch.zeros(Bn, N, A, device=dev)
    o1, o2 = torch.full((Bn, A), -7.0, device=dev), torch.full((Bn, A), -7.0, device=dev)
    later = torch.full((Bn, N), -9, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    fn = lib.mz_policy_glue_later

    def refused(rc, text):
        assert rc == MZ_ERR_ARG and text in lib.mz_last_error().decode(), (rc, lib.mz_last_error())

    refused(fn(h, p(x), MZ_DT_F32, N * A, N, 0, 1.0, p(o1), None, p(later)), "probs_out and beta_out go together")
    refused(fn(h, p(x), MZ_DT_F32, N * A, N, 0, 1.0, None, p(o2), p(later)), "probs_out and beta_out go together")
    refused(fn(h, p(x), 7, N * A, N, 0, 1.0, p(o1), p(o2), p(later)), "mz_policy_glue_later: bad dtype")
    refused(fn(h, p(x), MZ_DT_F32, N * A - 1, N, 0, 1.0, p(o1), p(o2), p(later)), "logits row does not hold")
    refused(fn(h, p(x), MZ_DT_F32, N * A, N, N, 1.0, p(o1), p(o2), p(later)), "bad agent index / count")
    refused(fn(h, p(x), MZ_DT_F32, N * A, N, -1, 1.0, p(o1), p(o2), p(later)), "bad agent index / count")
    refused(fn(h, p(x), MZ_DT_F32, N * A, 0, 0, 1.0, p(o1), p(o2), p(later)), "bad agent index / count")
    refused(fn(h, None, MZ_DT_F32, N * A, N, 0, 1.0, p(o1), p(o2), p(later)), "mz_policy_glue_later: null buffer")
    refused(fn(h, p(x), MZ_DT_F32, N * A, N, 0, 1.0, p(o1), p(o2), None), "later_out required")
    refused(fn(h, p(x), MZ_DT_F32, N * A, N, N - 1, 1.0, None, None, None), "no output asked for")
    refused(fn(h, p(x), MZ_DT_F32, N * A, N, 0, 0.0, p(o1), p(o2), p(later)), "sampled_tau must be > 0")
    torch.cuda.synchronize()
    assert (o1 == -7.0).all() and (o2 == -7.0).all() and (later == -9).all()  # nothing was launched
    assert fn(h, p(x), MZ_DT_F32, N * A, N, 0, 1.0, p(o1), p(o2), p(later)) == 0  # (the valid call goes through)
    np.testing.assert_array_equal(o1.cpu().numpy(), np.full((Bn, A), np.float32(1) / np.float32(A)))
    np.testing.assert_array_equal(later.cpu().numpy(), np.array([[-9, 0, 0]] * Bn, np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("cur", [0, 2, 4])
@pytest.mark.parametrize("slots", [1, 9])
def test_joint_action_cached_matches_numpy(slots, cur):
    """joint[:, :cur] = factor, joint[:, cur] = actions, joint[:, k > cur] = pool[idx_x[i]][i][k], an
    idx_x outside [0, slots) reading slot 0; 65 roots x 5 agents is more than one workgroup."""
    import torch

    from mazero_amd._capi import MZ_ERR_ARG, check

    Bn, N, A = 65, 5, 9
    rng = np.random.default_rng(100 * slots + cur)
    tb = _handle(Bn, A)
    lib, h = tb._lib, tb._h
    pool = rng.integers(0, A, size=(slots, Bn, N)).astype(np.int32)
    idx = rng.integers(0, slots, size=Bn).astype(np.int32)  # differs per root
    idx[:6] = [0, slots - 1, -1, slots, np.iinfo(np.int32).max, np.iinfo(np.int32).min]
    factor = rng.integers(0, A, size=(Bn, max(cur, 1) + 1)).astype(np.int32)  # (factor_cols above cur)
    act = rng.integers(0, A, size=Bn).astype(np.int32)
    dev = torch.device("cuda", 0)
    tp, ti, tf, ta = (torch.from_numpy(v).to(dev) for v in (pool, idx, factor, act))
    joint = torch.full((Bn, N), -7, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    check(lib, lib.mz_joint_action_cached(h, p(tp), slots, p(ti), N, cur, p(tf), factor.shape[1], p(ta), p(joint)),
          "joint_action_cached")
    clipped = np.where((idx >= 0) & (idx < slots), idx, 0)
    exp = np.zeros((Bn, N), np.int64)
    exp[:, :cur] = factor[:, :cur]
    exp[:, cur] = act
    exp[:, cur + 1:] = pool[clipped, np.arange(Bn), cur + 1:]
    np.testing.assert_array_equal(joint.cpu().numpy(), exp)

    def refused(rc, text):
        assert rc == MZ_ERR_ARG and text in lib.mz_last_error().decode(), (rc, lib.mz_last_error())

    if cur > 0:
        refused(lib.mz_joint_action_cached(h, p(tp), slots, p(ti), N, cur, None, 0, p(ta), p(joint)),
                "factor must hold")
        refused(lib.mz_joint_action_cached(h, p(tp), slots, p(ti), N, cur, p(tf), cur - 1, p(ta), p(joint)),
                "factor must hold")
    if cur + 1 < N:
        refused(lib.mz_joint_action_cached(h, None, slots, p(ti), N, cur, p(tf), factor.shape[1], p(ta), p(joint)),
                "pool and idx_x required")
        refused(lib.mz_joint_action_cached(h, p(tp), 0, p(ti), N, cur, p(tf), factor.shape[1], p(ta), p(joint)),
                "pool and idx_x required")
    refused(lib.mz_joint_action_cached(h, p(tp), slots, p(ti), N, N, p(tf), factor.shape[1], p(ta), p(joint)),
            "bad agent index / count")
    refused(lib.mz_joint_action_cached(h, p(tp), slots, p(ti), N, cur, p(tf), factor.shape[1], None, p(joint)),
            "mz_joint_action_cached: null buffer")


# ------------------------------------------------------------------------------------ whole searches
N3M, A3M, B3M, S3M = 3, 9, 32, 8  # the 3m shape


def _same(a, b):
    if isinstance(a, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_same_outputs(a, b, where):
    for name in a._fields:
        assert _same(getattr(a, name), getattr(b, name)), f"{where}: {name} differs"


def _loops_of(net):
    """{later_action_cache flag: loop} of the loops recorded for `net` (the flag ends a loop's key)."""
    from mazero_amd.mcts_sampled import _LOOPS

    return {k[-1]: v for k, v in _LOOPS.items() if v.model_ref() is net}


@functools.lru_cache(maxsize=None)
def _searches(K, cur, fused, A=A3M):
    """Four searches (eager; recorded and replayed; replayed; replayed again), each on new roots, by the
    default driver and by the driver with the cache, from the same generator state.  Any warning is an
    error: the guard must stay silent.  Returns the outputs and the two recorded loops."""
    import torch

    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import MuZeroShapedNet, SearchConfig, make_root_batch

    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=S3M, sampled_action_times=K)
    torch.manual_seed(3)
    net = MuZeroShapedNet(N3M, 64, A).to(dev).eval()
    factor = np.random.RandomState(5).randint(0, A, (B3M, N3M)).astype(np.int32) if cur else None
    outs = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for flag in (False, True):
            drv = SampledMCTS(cfg, np.random.RandomState(11), fused_transforms=fused, wide_actions=A > 64,
                              later_action_cache=flag)
            outs[flag] = []
            for step in range(4):
                out, legal = make_root_batch(net, B3M, 64, seed=700 + step, device=dev, legal_zero_frac=0.2)
                outs[flag].append(drv.batch_search(net, out, cur, factor, N3M, legal, device=dev, add_noise=True))
    return outs, _loops_of(net), net


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["torch_transforms", "fused_transforms"])
@pytest.mark.parametrize("cur", [0, 1, 2])
@pytest.mark.parametrize("K", [1, 5])
def test_cached_search_is_the_same_search(K, cur, fused):
    """Every SearchOutput field with the cache equals the default driver's, bit for bit, on the eager
    (checked) first search, the recorded search and two more replays.  Agent 2 is the last: the flag
    has no effect there."""
    import torch

    outs, loops, _ = _searches(K, cur, fused)
    assert set(loops) == {False, True}
    for lp in loops.values():  # both loops were recorded and replayed
        assert isinstance(lp.graph, torch.cuda.CUDAGraph) and lp.runs == 4
    assert loops[False].later is None
    assert (loops[True].later is not None) == (cur + 1 < N3M)  # the cache is on (no mismatch) where it applies
    for step, (a, b) in enumerate(zip(outs[False], outs[True])):
        _assert_same_outputs(a, b, f"search {step}")


@pytest.mark.gpu
def test_cached_search_wide_actions():
    """A = 100 under wide_actions: the tile bodies of both kernels inside a search."""
    outs, loops, _ = _searches(5, 0, False, 100)
    assert loops[True].later is not None and loops[True].graph
    for step, (a, b) in enumerate(zip(outs[False], outs[True])):
        _assert_same_outputs(a, b, f"search {step}")


@pytest.mark.gpu
def test_cached_search_root_shard():
    """Roots [8, 24) of 32 searched by a shard with the cache against the rows of the unsharded
    default search (three searches: eager, recorded, replayed)."""
    import torch

    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import MuZeroShapedNet, NetworkOutput, SearchConfig, make_root_batch

    K, cur, lo, hi = 5, 1, 8, 24
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A3M, num_simulations=S3M, sampled_action_times=K)
    torch.manual_seed(4)
    net = MuZeroShapedNet(N3M, 64, A3M).to(dev).eval()
    factor = np.random.RandomState(6).randint(0, A3M, (B3M, N3M)).astype(np.int32)
    whole = SampledMCTS(cfg, np.random.RandomState(12))
    shard = SampledMCTS(cfg, np.random.RandomState(12), root_shard=(lo, hi, B3M), later_action_cache=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for step in range(3):
            out, legal = make_root_batch(net, B3M, 64, seed=800 + step, device=dev, legal_zero_frac=0.2)
            a = whole.batch_search(net, out, cur, factor, N3M, legal, device=dev, add_noise=True)
            part = NetworkOutput(out.hidden_state[lo:hi], out.reward[lo:hi], out.value[lo:hi],
                                 out.policy_logits[lo:hi])
            b = shard.batch_search(net, part, cur, factor[lo:hi], N3M, legal[lo:hi], device=dev, add_noise=True)
            for name in a._fields:
                assert _same(getattr(a, name)[lo:hi], getattr(b, name)), f"search {step}: {name} differs"
    assert _loops_of(net)[True].later is not None


@pytest.mark.gpu
def test_cached_search_matches_oracle_driver(port_lib):
    """Against the oracle driver (numpy + the CPU port), which calls `prediction` on the gathered leaves
    itself: three searches (eager, recorded, replayed) at K = 5, agent 0, then the generator state."""
    import torch

    from driver import OracleSampledMCTS
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch
    from test_driver import _compare_outputs

    K, cur = 5, 0
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A3M, num_simulations=S3M, sampled_action_times=K)
    net = make_net(N3M, A3M, seed=12, device=dev)
    rs_o, rs_d = np.random.RandomState(5), np.random.RandomState(5)
    oracle = OracleSampledMCTS(cfg, rs_o, port_lib)
    drv = SampledMCTS(cfg, rs_d, later_action_cache=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for step in range(3):
            out, legal = make_root_batch(net, B3M, 64, seed=100 + step, device=dev, legal_zero_frac=0.3)
            exp = oracle.batch_search(net, out, cur, None, N3M, legal, device=dev, add_noise=True)
            got = drv.batch_search(net, out, cur, None, N3M, legal, device=dev, add_noise=True)
            _compare_outputs(got, exp)
    assert rs_o.randint(1 << 30) == rs_d.randint(1 << 30)
    assert _loops_of(net)[True].later is not None


@pytest.mark.gpu
@pytest.mark.parametrize("cur", [0, 1])
def test_prediction_call_count(cur):
    """Eager searches (use_graph=False) of S simulations: the default loop calls `prediction` 2 S times
    (the leaves, then the recurrent inference); with the cache the first search, which is checked
    against the default path, calls it 2 S times too and every later search S + 1 times (the root,
    then the recurrent inference)."""
    import torch

    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import MuZeroShapedNet, SearchConfig, make_root_batch

    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A3M, num_simulations=S3M, sampled_action_times=5)
    factor = np.random.RandomState(5).randint(0, A3M, (B3M, N3M)).astype(np.int32) if cur else None
    for flag, want in ((True, [2 * S3M, S3M + 1, S3M + 1]), (False, [2 * S3M] * 3)):
        torch.manual_seed(3)
        net = MuZeroShapedNet(N3M, 64, A3M).to(dev).eval()
        calls, inner = [0], net.prediction

        def counted(h, calls=calls, inner=inner):
            calls[0] += 1
            return inner(h)

        net.prediction = counted
        drv = SampledMCTS(cfg, np.random.RandomState(11), use_graph=False, later_action_cache=flag)
        got = []
        for step in range(3):
            out, legal = make_root_batch(net, B3M, 64, seed=700 + step, device=dev, legal_zero_frac=0.2)
            calls[0] = 0
            drv.batch_search(net, out, cur, factor, N3M, legal, device=dev, add_noise=True)
            got.append(calls[0])
        assert got == want, (flag, got)


@pytest.mark.gpu
def test_graph_census():
    """The recorded graph of agent 0 has strictly fewer nodes with the cache (S - 1 prediction passes
    go, one launch for the root's slot comes); the last agent's loops are node for node the same."""
    _, loops, _ = _searches(1, 0, False)
    default_nodes, cached_nodes = loops[False].graph_nodes[0], loops[True].graph_nodes[0]
    print(f"graph nodes, agent 0: default loop {default_nodes}, cached loop {cached_nodes}, {S3M} simulations")
    assert cached_nodes < default_nodes
    _, loops, _ = _searches(1, 2, False)
    assert loops[False].graph_nodes == loops[True].graph_nodes


@pytest.mark.gpu
def test_guard_drops_the_cache():
    """A model whose `prediction` moves the later agents' best action with every call is not a function
    of the state: the loop's first search warns once, naming the model class, and returns the default
    path's results; the loop then is the default loop, recorded graph included."""
    import torch

    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import MuZeroShapedNet, SearchConfig, make_root_batch

    class CountingNet(MuZeroShapedNet):
        calls = 0

        def prediction(self, h):
            policy, value = super().prediction(h)
            self.calls += 1
            bump = torch.zeros_like(policy)
            bump[:, 1:, self.calls % self.action_space_size] = 100.0
            return policy + bump, value

    K, cur = 5, 0
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A3M, num_simulations=S3M, sampled_action_times=K)
    outs, nets = {}, {}
    for flag in (False, True):
        torch.manual_seed(3)
        net = nets[flag] = CountingNet(N3M, 64, A3M).to(dev).eval()
        drv = SampledMCTS(cfg, np.random.RandomState(11), later_action_cache=flag)
        outs[flag] = []
        for step in range(3):
            out, legal = make_root_batch(net, B3M, 64, seed=700 + step, device=dev, legal_zero_frac=0.2)
            net.calls = 100 * step  # (the same call numbers in both drivers' searches)
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                outs[flag].append(drv.batch_search(net, out, cur, None, N3M, legal, device=dev, add_noise=True))
            mine = [w for w in caught if "later_action_cache" in str(w.message)]
            if flag and step == 0:
                assert len(mine) == 1 and issubclass(mine[0].category, RuntimeWarning)
                assert "CountingNet" in str(mine[0].message)
            else:
                assert not mine
    cached, default = _loops_of(nets[True])[True], _loops_of(nets[False])[False]
    assert cached.later is None  # the cache is off for good
    assert cached.graph_nodes is not None and cached.graph_nodes == default.graph_nodes
    _assert_same_outputs(outs[False][0], outs[True][0], "the checked search")
