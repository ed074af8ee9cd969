"""The driver glue for action spaces of 65..255 (include/mzdriver.h: mz_policy_glue_wide,
mz_root_glue_wide, mz_joint_action_wide) and SampledMCTS(..., wide_actions=True).

CPU tests pin what the glue kernels rely on at every width: the block plan of a row sum (one function
for host and device, mz_wide_sum_plan on the host) reproduces numpy's pairwise np.sum for every row
length up to 255, and the constructor's opt-in.
GPU tests compare the kernels with the numpy expressions of the reference driver
(mcts_sampled.py:64-100,116-147,156-161) bit for bit, the _wide entry points with the narrow ones at
A <= 64, and whole searches with the oracle driver on the CPU port.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from test_driver import _compare_outputs, _numpy_policy_glue

WIDE_A = (65, 128, 129, 136, 200, 248, 249, 255)
B = 6


def _u32(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


# ------------------------------------------------------------------------------------------------
# CPU: the block plan
# ------------------------------------------------------------------------------------------------
def _plan(lib, n):
    starts, lens, k = (C.c_int * 3)(), (C.c_int * 3)(), C.c_int(0)
    assert lib.mz_wide_sum_plan(n, starts, lens, C.byref(k)) == 0, n
    return [(starts[i], lens[i]) for i in range(k.value)]


def _block_sum(X):
    """numpy's pairwise-sum base case (n <= 128) of every row of the float32 array X [R, n]: what one
    group of 8 lanes and its first lane compute in np_row_sum (mzdriver.hip), at every tile count;
    n < 8 (only a row of A < 8 is such a block) is the sequential sum its first lane's tail loop takes."""
    n = X.shape[1]
    if n < 8:
        r = np.zeros(X.shape[0], np.float32)
        for i in range(n):
            r = r + X[:, i]
        return r
    acc = [X[:, j] for j in range(8)]
    n8 = n - n % 8
    for i in range(8, n8, 8):
        for j in range(8):
            acc[j] = acc[j] + X[:, i + j]
    r = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))
    for i in range(n8, n):
        r = r + X[:, i]
    return r


def _planned_sum(X, plan):
    """The row sums of the float32 array X as the glue kernels take them: base-case blocks, joined
    from the right."""
    assert X.dtype == np.float32
    sums = [_block_sum(X[:, s:s + ln]) for s, ln in plan]
    r = sums[-1]
    for s in reversed(sums[:-1]):
        r = s + r
    assert r.dtype == np.float32
    return r


@pytest.fixture(scope="module")
def product_lib():
    from mazero_amd._lib import load

    return load()  # (loads without a GPU; mz_wide_sum_plan makes no device call)


def test_sum_plan_shape(product_lib):
    """The plan tiles the row with blocks of at most 128 elements that start at multiples of 8; the
    split points are numpy's (n2 = n / 2, n2 -= n2 % 8), a third block appears from n = 249."""
    for n in range(1, 256):
        plan = _plan(product_lib, n)
        assert sum(ln for _, ln in plan) == n and plan[0][0] == 0
        for (s, ln), (s2, _) in zip(plan, plan[1:]):
            assert s + ln == s2
        assert all(s % 8 == 0 and 1 <= ln <= 128 for s, ln in plan)
        assert len(plan) == (1 if n <= 128 else 2 if n <= 248 else 3), n
        if n > 64:  # past one tile no block takes numpy's n < 8 path: only a row of A < 8 does
            assert all(ln >= 64 for _, ln in plan), n
    assert _plan(product_lib, 129) == [(0, 64), (64, 65)]
    assert _plan(product_lib, 200) == [(0, 96), (96, 104)]
    assert _plan(product_lib, 248) == [(0, 120), (120, 128)]
    assert _plan(product_lib, 249) == [(0, 120), (120, 64), (184, 65)]
    assert _plan(product_lib, 255) == [(0, 120), (120, 64), (184, 71)]
    k = C.c_int(0)
    for bad in (0, 256, -3):
        assert product_lib.mz_wide_sum_plan(bad, (C.c_int * 3)(), (C.c_int * 3)(), C.byref(k)) != 0


def test_sum_plan_matches_numpy_float32(product_lib):
    """np.sum(X, axis=-1, keepdims=True) of float32 rows with mixed magnitudes, every n in 1..255,
    contiguous rows and the strided view logits[:, k:k+1, :] the driver sums."""
    rng = np.random.default_rng(1)
    for n in range(1, 256):
        X = (rng.random((40, 3, n)) * rng.choice([1e-3, 1.0, 1e3], size=(40, 3, n))).astype(np.float32)
        plan = _plan(product_lib, n)
        flat = np.ascontiguousarray(X[:, 0, :])
        np.testing.assert_array_equal(_u32(_planned_sum(flat, plan)),
                                      _u32(np.sum(flat, axis=-1, keepdims=True)[:, 0]), err_msg=f"n={n}")
        view = X[:, 1:2, :]
        np.testing.assert_array_equal(_u32(_planned_sum(np.ascontiguousarray(view[:, 0, :]), plan)),
                                      _u32(np.sum(view, axis=-1, keepdims=True)[:, 0, 0]), err_msg=f"view n={n}")


def test_sum_plan_matches_numpy_float16(product_lib):
    """float16 rows: the same plan accumulated in float32 and rounded to half once."""
    rng = np.random.default_rng(2)
    for n in range(1, 256):
        X = (rng.random((40, 2, n)) * rng.choice([1e-2, 1.0, 8.0], size=(40, 2, n))).astype(np.float16)
        plan = _plan(product_lib, n)
        view = X[:, 1:2, :]
        got = _planned_sum(np.ascontiguousarray(view[:, 0, :]).astype(np.float32), plan).astype(np.float16)
        exp = np.sum(view, axis=-1, keepdims=True)[:, 0, 0]
        np.testing.assert_array_equal(got.view(np.uint16), exp.view(np.uint16), err_msg=f"n={n}")


# ------------------------------------------------------------------------------------------------
# CPU: the opt-in
# ------------------------------------------------------------------------------------------------
def test_wide_actions_constructs_without_a_device():
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    m = SampledMCTS(SearchConfig(action_space_size=100), wide_actions=True)
    assert m.wide_actions
    assert SampledMCTS(SearchConfig(action_space_size=255), np.random.RandomState(0), wide_actions=True).wide_actions
    assert not SampledMCTS(SearchConfig(action_space_size=9)).wide_actions


def test_wide_actions_read_from_config():
    """A reference-style call SampledMCTS(config, np_random) opts in through its config object."""
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=100)
    cfg.wide_actions = True
    assert SampledMCTS(cfg, np.random.RandomState(0)).wide_actions
    # an explicit argument wins over the config
    with pytest.raises(RuntimeError, match="action_space_size 100 > 64"):
        SampledMCTS(cfg, np.random.RandomState(0), wide_actions=False)


def test_wide_actions_stop_at_255():
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    with pytest.raises(RuntimeError, match="255"):
        SampledMCTS(SearchConfig(action_space_size=256), wide_actions=True)


def test_narrow_default_still_refuses_65():
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    with pytest.raises(RuntimeError, match="action_space_size 65 > 64"):
        SampledMCTS(SearchConfig(action_space_size=65))
    cfg = SearchConfig(action_space_size=65)
    cfg.wide_actions = False
    with pytest.raises(RuntimeError, match="action_space_size 65 > 64"):
        SampledMCTS(cfg)


def test_worker_shard_passes_wide_actions():
    """mazero_amd.workers: the flag reaches the shard's default search, as an argument and through
    the config object; without either the default search still refuses A > 64."""
    from mazero_amd.nets import SearchConfig
    from mazero_amd.workers import ReanalyzeShard, SelfPlayShard

    cfg = SearchConfig(action_space_size=100)
    sp = SelfPlayShard(None, cfg, 8, 2, seed=0, rank=1, world=2, wide_actions=True)
    m = sp.make_mcts(sp.config, sp.np_random, sp.root_shard)
    assert m.wide_actions and m.root_shard == (4, 8, 8)
    with pytest.raises(RuntimeError, match="action_space_size 100 > 64"):
        ReanalyzeShard(None, cfg, 8, seed=0, rank=0, world=1).make_mcts(cfg, None, (0, 8, 8))
    cfg.wide_actions = True
    ra = ReanalyzeShard(None, cfg, 8, seed=0, rank=0, world=1)
    assert ra.make_mcts(ra.config, ra.np_random, ra.root_shard).wide_actions


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
def _handle(A):
    import torch

    from mazero_amd.cytree import Tree_batch
    from mazero_amd.mcts_sampled import ensure_half_exp

    tb = Tree_batch(B, 1, A, 1, 4, 0.01, 0, 0.75, 0.8)
    ensure_half_exp(tb._lib, torch.cuda.current_device())  # (as the search loop does)
    tb._sync_stream()
    return tb


def _code(dtype):
    from mazero_amd._capi import MZ_DT_F16, MZ_DT_F32

    return MZ_DT_F16 if np.dtype(dtype) == np.float16 else MZ_DT_F32


def _policy_logits(rng, N, A, cur, dtype):
    """B = 6 rows of the current agent: a NaN in the last tile, -inf entries, constant logits, three
    random rows of different scales, one of them with a +inf (its softmax is inf - inf: numpy's NaN
    for a row without a NaN of its own)."""
    logits = (rng.standard_normal((B, N, A)) * np.array([1, 1, 1, 0.1, 4, 30]).reshape(B, 1, 1)).astype(dtype)
    logits[0, cur, A - 1] = np.nan
    logits[1, cur, rng.choice(A, size=A // 3, replace=False)] = -np.inf
    logits[2, cur, :] = logits[2, cur, 0]
    logits[4, cur, A // 2] = np.inf
    return logits


def _run_policy_glue(fn, tb, logits, cur, tau):
    import torch

    from mazero_amd._capi import check

    _, N, A = logits.shape
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(logits).to(dev)
    probs, beta = torch.full((B, A), -7.0, device=dev), torch.full((B, A), -7.0, device=dev)
    check(tb._lib, fn(tb._h, C.c_void_p(x.data_ptr()), _code(logits.dtype), N * A, cur * A, tau,
                      C.c_void_p(probs.data_ptr()), C.c_void_p(beta.data_ptr())), "policy_glue")
    return probs.cpu().numpy(), beta.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tau", [("float32", 1.0), ("float16", 1.0), ("float16", 0.5)])
@pytest.mark.parametrize("A", WIDE_A)
def test_policy_glue_wide_matches_numpy(A, dtype, tau):
    N, cur = 3, 1
    logits = _policy_logits(np.random.default_rng(A), N, A, cur, dtype)
    tb = _handle(A)
    gp, gb = _run_policy_glue(tb._lib.mz_policy_glue_wide, tb, logits, cur, tau)
    with np.errstate(all="ignore"):
        ep, eb = _numpy_policy_glue(logits[:, cur:cur + 1, :], tau)
    print(f"A={A} {dtype} tau={tau}: probs mismatches {(_u32(gp) != _u32(ep.reshape(B, A))).sum()}, "
          f"beta mismatches {(_u32(gb) != _u32(eb.reshape(B, A))).sum()}")
    np.testing.assert_array_equal(_u32(gp), _u32(ep.reshape(B, A)))
    np.testing.assert_array_equal(_u32(gb), _u32(eb.reshape(B, A)))


def _run_root_glue(fn, tb, arrays, mode, eps, A, tau=1.0):
    import torch

    from mazero_amd._capi import check

    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in arrays.items()}
    probs, beta, nz = (torch.full((B, A), -7.0, device=dev) for _ in range(3))
    lg = t.get("legal")
    check(tb._lib, fn(tb._h, C.c_void_p(t["logits"].data_ptr()), mode[0], A, 0,
                      None if lg is None else C.c_void_p(lg.data_ptr()), A, C.c_void_p(t["noise"].data_ptr()),
                      float(eps), tau, C.c_void_p(probs.data_ptr()), C.c_void_p(beta.data_ptr()),
                      C.c_void_p(nz.data_ptr())), "root_glue")
    return probs.cpu().numpy(), beta.cpu().numpy(), nz.cpu().numpy()


def _root_case(rng, A, dtype, legal_kind, N=3, cur=1):
    import torch

    from mazero_amd.nets import NetworkOutput

    logits = (rng.standard_normal((B, N, A)) * np.array([0.1, 1, 1, 4, 4, 30]).reshape(B, 1, 1)).astype(dtype)
    logits[0, cur, 1] = 60.0  # one dominant logit
    legal = None
    if legal_kind == "int64":
        legal = (rng.random((B, N, A)) >= 0.3).astype(np.int64)
        legal[..., 0] = np.where(legal.sum(-1) == 0, 1, legal[..., 0])
    out = NetworkOutput(torch.zeros(B, 4, device="cuda"), rng.standard_normal((B, 1)).astype(np.float32),
                        rng.standard_normal((B, 1)).astype(np.float32), logits)
    return out, legal


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("A", WIDE_A)
def test_root_glue_wide_matches_host_root_inputs(A, dtype):
    """mz_root_glue_wide against SampledMCTS.root_inputs (numpy on the host, as the reference computes
    the root): int64 masks with ~30 % zeros and no mask, noise on and off."""
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cur = 1
    rng = np.random.default_rng(1000 + A)
    tb = _handle(A)
    cfg = SearchConfig(action_space_size=A)
    for legal_kind in ("none", "int64"):
        for noise in (True, False):
            out, legal = _root_case(rng, A, dtype, legal_kind, cur=cur)
            seed = int(rng.integers(1 << 30))
            m_host = SampledMCTS(cfg, np.random.RandomState(seed), wide_actions=True)
            m_dev = SampledMCTS(cfg, np.random.RandomState(seed), wide_actions=True)
            (rr, rv, rp, rb, eps, rn), seed_h = m_host.root_inputs(out, cur, legal, noise, 1.0)
            arrays, mode, eps_d, seed_d = m_dev.root_raw(out, cur, legal, noise)
            assert seed_d == seed_h and eps_d == eps and mode == (_code(dtype), legal is not None)
            got = _run_root_glue(tb._lib.mz_root_glue_wide, tb, arrays, mode, eps_d, A)
            where = f"{dtype} A={A} legal={legal_kind} noise={noise}"
            for g, e, name in zip(got, (rp, rb, rn), ("probs", "beta", "noises")):
                print(f"{name} {where}: mismatches {(_u32(g) != _u32(e.reshape(B, A))).sum()}")
            for g, e, name in zip(got, (rp, rb, rn), ("probs", "beta", "noises")):
                np.testing.assert_array_equal(_u32(g), _u32(e.reshape(B, A)), err_msg=f"{name} {where}")


def _joint_case(rng, N, A, dtype):
    """Integer-valued leaf logits (many ties), B = 6 rows of every agent; per agent k:
    row 0: the maximum in tile 0 at a high lane and again in tile 1 at a low lane (action order is
           not lane order);
    row 1: the maximum only in the later tiles, twice;
    row 2: a NaN in the last tile (tile 2 where the row has one) and the maximum in tile 0;
    row 3: NaNs in two tiles, the later tile's at the lower lane;
    row 4: all equal."""
    pred = rng.integers(-3, 3, size=(B, N, A)).astype(dtype)
    last = ((A - 1) // 64) * 64  # first action of the last tile
    pred[0, :, 40] = 5
    pred[0, :, 64] = 5
    pred[1, :, A - 1] = 7
    pred[1, :, 64] = 7
    pred[2, :, 3] = 9
    pred[2, :, min(last + 1, A - 1)] = np.nan
    pred[3, :, 50] = np.nan
    pred[3, :, min(64 + 9, A - 1)] = np.nan
    pred[3, :, 10] = 11
    pred[4, :, :] = pred[4, :, :1]
    return pred


def _run_joint_action(fn, tb, pred, cur, factor, act):
    import torch

    from mazero_amd._capi import check

    _, N, A = pred.shape
    dev = torch.device("cuda", 0)
    joint = torch.full((B, N), -7, dtype=torch.int64, device=dev)
    p, f, a = (torch.from_numpy(v).to(dev) for v in (pred, factor, act))
    check(tb._lib, fn(tb._h, C.c_void_p(p.data_ptr()), _code(pred.dtype), N, cur, C.c_void_p(f.data_ptr()),
                      factor.shape[1], C.c_void_p(a.data_ptr()), C.c_void_p(joint.data_ptr())), "joint_action")
    return joint.cpu().numpy()


def _numpy_joint(pred, cur, factor, act):
    _, N, _ = pred.shape
    exp = np.zeros((B, N), np.int64)  # mcts_sampled.py:116-145
    exp[:, :cur] = factor[:, :cur]
    exp[:, cur] = act
    for k in range(cur + 1, N):
        exp[:, k] = np.argmax(pred[:, k, :], axis=-1)
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("A", [65, 130, 255])
def test_joint_action_wide_matches_numpy(A, dtype):
    N = 4
    rng = np.random.default_rng(A)
    pred = _joint_case(rng, N, A, dtype)
    tb = _handle(A)
    for cur in range(N):
        factor = rng.integers(0, A, size=(B, max(cur, 1))).astype(np.int32)
        act = rng.integers(0, A, size=B).astype(np.int32)
        got = _run_joint_action(tb._lib.mz_joint_action_wide, tb, pred, cur, factor, act)
        np.testing.assert_array_equal(got, _numpy_joint(pred, cur, factor, act), err_msg=f"cur={cur}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("A", [7, 9, 64])
def test_wide_entry_points_equal_narrow_up_to_64(A, dtype):
    """A <= 64: the _wide entry points launch the kernels of the narrow ones (the T = 1 instantiations);
    same bytes on the same inputs.  A = 7: numpy's sequential row sum."""
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    N, cur = 3, 1
    rng = np.random.default_rng(64 + A)
    tb = _handle(A)
    lib = tb._lib
    logits = (rng.standard_normal((B, N, A)) * np.array([1, 1, 1, 0.1, 4, 30]).reshape(B, 1, 1)).astype(dtype)
    logits[0, cur, A - 1] = np.nan
    logits[1, cur, :3] = -np.inf
    for tau in (1.0, 0.5, 1.5):
        n = _run_policy_glue(lib.mz_policy_glue, tb, logits, cur, tau)
        w = _run_policy_glue(lib.mz_policy_glue_wide, tb, logits, cur, tau)
        for a, b in zip(n, w):
            np.testing.assert_array_equal(_u32(a), _u32(b))
    cfg = SearchConfig(action_space_size=A)
    for legal_kind in ("none", "int64"):
        out, legal = _root_case(rng, A, dtype, legal_kind, cur=cur)
        arrays, mode, eps, _ = SampledMCTS(cfg, np.random.RandomState(A)).root_raw(out, cur, legal, True)
        n = _run_root_glue(lib.mz_root_glue, tb, arrays, mode, eps, A)
        w = _run_root_glue(lib.mz_root_glue_wide, tb, arrays, mode, eps, A)
        for a, b in zip(n, w):
            np.testing.assert_array_equal(_u32(a), _u32(b))
    pred = rng.integers(-3, 3, size=(B, N, A)).astype(dtype)
    pred[0, 2, A - 2] = np.nan
    pred[1, :, :] = pred[1, :, :1]
    for c in range(N):
        factor = rng.integers(0, A, size=(B, max(c, 1))).astype(np.int32)
        act = rng.integers(0, A, size=B).astype(np.int32)
        n = _run_joint_action(lib.mz_joint_action, tb, pred, c, factor, act)
        w = _run_joint_action(lib.mz_joint_action_wide, tb, pred, c, factor, act)
        np.testing.assert_array_equal(n, w)
        np.testing.assert_array_equal(w, _numpy_joint(pred, c, factor, act))


@pytest.mark.gpu
def test_wide_launchers_keep_the_argument_checks():
    """The _wide launchers refuse what the narrow ones refuse (nothing is launched), under their own
    names; the narrow ones still refuse A = 100."""
    import torch

    from mazero_amd._capi import MZ_DT_F32, MZ_ERR_ARG, MZ_ERR_UNSUPPORTED

    A, N = 100, 2
    tb = _handle(A)
    lib, h = tb._lib, tb._h
    dev = torch.device("cuda", 0)
    x = torch.zeros(B, N, A, device=dev)
    o1, o2, o3 = (torch.zeros(B, A, device=dev) for _ in range(3))
    legal = torch.ones(B, A, dtype=torch.int32, device=dev)
    act = torch.zeros(B, dtype=torch.int32, device=dev)
    joint = torch.zeros(B, N, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def refused(rc, code, text):
        assert rc == code and text in lib.mz_last_error().decode(), (rc, lib.mz_last_error())

    refused(lib.mz_policy_glue(h, p(x), MZ_DT_F32, N * A, 0, 1.0, p(o1), p(o2)), MZ_ERR_UNSUPPORTED,
            "mz_policy_glue: action_space_size > 64")
    refused(lib.mz_root_glue(h, p(x), MZ_DT_F32, N * A, 0, None, A, p(o3), 0.25, 1.0, p(o1), p(o2), p(o3)),
            MZ_ERR_UNSUPPORTED, "mz_root_glue: action_space_size > 64")
    refused(lib.mz_joint_action(h, p(x), MZ_DT_F32, N, 0, None, 0, p(act), p(joint)), MZ_ERR_UNSUPPORTED,
            "mz_joint_action: action_space_size > 64")

    pg = lib.mz_policy_glue_wide
    refused(pg(h, None, MZ_DT_F32, N * A, 0, 1.0, p(o1), p(o2)), MZ_ERR_ARG, "mz_policy_glue_wide: null buffer")
    refused(pg(h, p(x), 7, N * A, 0, 1.0, p(o1), p(o2)), MZ_ERR_ARG, "mz_policy_glue_wide: bad dtype")
    refused(pg(h, p(x), MZ_DT_F32, A - 1, 0, 1.0, p(o1), p(o2)), MZ_ERR_ARG, "logits row does not hold")
    refused(pg(h, p(x), MZ_DT_F32, N * A, (N - 1) * A + 1, 1.0, p(o1), p(o2)), MZ_ERR_ARG, "logits row does not hold")
    refused(pg(h, p(x), MZ_DT_F32, N * A, 0, 0.0, p(o1), p(o2)), MZ_ERR_ARG, "sampled_tau must be > 0")
    rg = lib.mz_root_glue_wide
    refused(rg(h, p(x), MZ_DT_F32, N * A, 0, p(legal), A - 1, p(o3), 0.25, 1.0, p(o1), p(o2), p(o3)), MZ_ERR_ARG,
            "mz_root_glue_wide: legal rows hold fewer than A")
    refused(rg(h, p(x), MZ_DT_F32, N * A, 0, None, A, None, 0.25, 1.0, p(o1), p(o2), p(o3)), MZ_ERR_ARG,
            "mz_root_glue_wide: null buffer")
    refused(rg(h, p(x), MZ_DT_F32, N * A, 0, None, A, p(o3), 0.25, -1.0, p(o1), p(o2), p(o3)), MZ_ERR_ARG,
            "sampled_tau must be > 0")
    ja = lib.mz_joint_action_wide
    refused(ja(h, p(x), MZ_DT_F32, N, N, None, 0, p(act), p(joint)), MZ_ERR_ARG, "bad agent index / count")
    refused(ja(h, None, MZ_DT_F32, N, 0, None, 0, p(act), p(joint)), MZ_ERR_ARG, "leaf policy logits required")
    refused(ja(h, p(x), MZ_DT_F32, N, 1, None, 0, p(act), p(joint)), MZ_ERR_ARG, "factor must hold")
    refused(ja(h, p(x), MZ_DT_F32, N, 0, None, 0, None, p(joint)), MZ_ERR_ARG, "mz_joint_action_wide: null buffer")
    assert pg(h, p(x), MZ_DT_F32, N * A, A, 1.0, p(o1), p(o2)) == 0  # (and the valid call goes through)
    np.testing.assert_array_equal(o1.cpu().numpy(), np.full((B, A), np.float32(1) / np.float32(A)))


WIDE_DRIVER_CASES = [
    # (N, A, B, S, K, agent, legal_zero_frac, add_noise)
    (2, 100, 8, 12, 5, 0, 0.3, True),
    (3, 200, 6, 10, 1, 1, 0.0, True),   # a later agent: the wide argmax
    (2, 255, 4, 8, 10, 1, 0.2, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("fpol", [False, True], ids=["half_policy", "float_policy"])
@pytest.mark.parametrize("case", WIDE_DRIVER_CASES, ids=lambda c: f"N{c[0]}A{c[1]}B{c[2]}S{c[3]}K{c[4]}ag{c[5]}")
def test_wide_driver_matches_oracle_driver(case, fpol, port_lib):
    """Whole searches through the wide glue against the oracle driver (numpy + the CPU port), with the
    arguments of test_driver.test_driver_matches_oracle_driver."""
    import torch

    from driver import OracleSampledMCTS
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch

    N, A, Bn, S, K, cur, zf, noise = case
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=K)
    net = make_net(N, A, seed=3, device=dev, float_policy=fpol)
    out, legal = make_root_batch(net, Bn, 64, seed=4, device=dev, legal_zero_frac=zf)
    factor = np.random.default_rng(5).integers(0, A, size=(Bn, max(cur, 1))).astype(np.int32)[:, :cur] if cur else None
    exp = OracleSampledMCTS(cfg, np.random.RandomState(11), port_lib).batch_search(
        net, out, cur, factor, N, legal, device=dev, add_noise=noise)
    got = SampledMCTS(cfg, np.random.RandomState(11), wide_actions=True).batch_search(
        net, out, cur, factor, N, legal, device=dev, add_noise=noise)
    _compare_outputs(got, exp)


@pytest.mark.gpu
def test_wide_driver_graph_replay_matches_oracle(port_lib):
    """One wide configuration searched three times in a row (eager, capture + replay, replay), each
    with new roots: every SearchOutput field, then the generator state."""
    import torch

    from driver import OracleSampledMCTS
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch

    N, A, Bn, S, K, cur = 2, 100, 8, 12, 5, 0
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=K)
    net = make_net(N, A, seed=12, device=dev)
    rs_o, rs_d = np.random.RandomState(5), np.random.RandomState(5)
    oracle = OracleSampledMCTS(cfg, rs_o, port_lib)
    drv = SampledMCTS(cfg, rs_d, use_graph=True, wide_actions=True)
    for step in range(3):
        out, legal = make_root_batch(net, Bn, 64, seed=100 + step, device=dev, legal_zero_frac=0.3)
        exp = oracle.batch_search(net, out, cur, None, N, legal, device=dev, add_noise=True)
        got = drv.batch_search(net, out, cur, None, N, legal, device=dev, add_noise=True)
        _compare_outputs(got, exp)
    assert rs_o.randint(1 << 30) == rs_d.randint(1 << 30)


@pytest.mark.gpu
def test_wide_selfplay_decisions_match_oracle(port_lib):
    """One self-play step at A = 100 through the device consumers (one lane per root, loops over A:
    unchanged) against the restated consumers, as tests/test_consume.py does at small A."""
    import torch

    from consume import selfplay_step
    from driver import OracleSampledMCTS
    from mazero_amd.consume import selfplay_decisions
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch

    N, A, Bn, S, K, temperature, eps = 2, 100, 8, 12, 5, 0.5, 0.3
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=K)
    net = make_net(N, A, seed=21, device=dev)
    out, legal = make_root_batch(net, Bn, 64, seed=22, device=dev, legal_zero_frac=0.3)
    ur = np.random.default_rng(23)
    u_eps = ur.random((N, Bn)).astype(np.float32)
    u_cat = ur.random((N, Bn))
    rs_o = np.random.Generator(np.random.PCG64(31))
    rs_d = np.random.Generator(np.random.PCG64(31))
    exp = selfplay_step(OracleSampledMCTS(cfg, rs_o, port_lib), net, out, N, legal, temperature, 1.0, eps, rs_o,
                        u_eps, u_cat, device=dev)
    got = selfplay_decisions(SampledMCTS(cfg, rs_d, wide_actions=True), net, out, N, legal, temperature=temperature,
                             greedy_epsilon=eps, eps_uniforms=(u_eps, u_cat), device=dev)
    np.testing.assert_array_equal(got.actions.cpu().numpy(), exp["actions"])
    np.testing.assert_array_equal(got.prob_action.cpu().numpy(), exp["prob_action"])
    np.testing.assert_array_equal(got.root_value.cpu().numpy().view(np.uint32), exp["root_value"].view(np.uint32))
    np.testing.assert_allclose(got.count_entropy.cpu().numpy(), exp["count_entropy"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got.visit_entropy.cpu().numpy(), exp["visit_entropy"], rtol=1e-12, atol=1e-15)
    assert rs_o.random() == rs_d.random()  # np_random consumed identically
