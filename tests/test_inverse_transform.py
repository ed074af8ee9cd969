"""mz_inverse_transform (include/mzdriver.h) and SampledMCTS(fused_transforms=True).

The target of every device comparison is the torch chain on the same device under autocast,
`mazero_amd.nets.inverse_support_transform` (softmax -> support_expectation -> inverse_h; the later
stages are compared with its later parts), as int32 bit patterns: the fused launch replaces those
torch kernels inside the search loop, so it has to compute the same floats.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from mazero_amd import _capi

DRIVER_HEADER = os.path.join(ROOT, "include", "mzdriver.h")
SUPPORT_SIZES = [1, 2, 3, 11, 16, 17, 33, 64]
ROW_COUNTS = [1, 2, 3, 257, 1536]


# ------------------------------------------------------------------------------------------ CPU
def test_ctypes_signature_matches_header():
    """The binding table's entry for mz_inverse_transform, argument by argument, against the
    declaration in include/mzdriver.h; the stage constants against enum mz_inv_stage."""
    txt = open(DRIVER_HEADER).read()
    m = re.search(r"^int\s+mz_inverse_transform\s*\(([^;]*)\)\s*;", txt, re.M)
    assert m, "mz_inverse_transform is not declared"
    ctype = {"mz_batch *": C.c_void_p, "void *": C.c_void_p, "const void *": C.c_void_p, "float *": C.c_void_p,
             "int": C.c_int, "int64_t": C.c_int64}
    declared = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        ty = re.match(r"(.*?)(\w+)$", arg).group(1).strip()
        declared.append(ctype[ty])
    res, args = _capi.DRIVER_SIGNATURES["mz_inverse_transform"]
    assert res is C.c_int
    assert args == declared
    enum = re.search(r"enum\s+mz_inv_stage\s*\{([^}]*)\}", txt).group(1)
    values = {k: int(v) for k, v in re.findall(r"(MZ_INV_[A-Z]+)\s*=\s*(\d+)", enum)}
    assert values == {"MZ_INV_LOGITS": _capi.MZ_INV_LOGITS, "MZ_INV_PROBS": _capi.MZ_INV_PROBS,
                      "MZ_INV_EXPECTATION": _capi.MZ_INV_EXPECTATION}


def test_search_config_defaults_and_flag_default():
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=9)
    assert cfg.value_support == (-5, 5) and cfg.reward_support == (-5, 5) and cfg.use_vectorization is True
    assert SampledMCTS(cfg, np.random.RandomState(0)).fused_transforms is None  # off by default

    class Support:
        min, max = -300, 300

    cfg.value_support = Support()
    assert SampledMCTS(cfg, np.random.RandomState(0), fused_transforms=True).fused_transforms == ((-300, 300), (-5, 5))
    cfg.use_vectorization = False
    assert SampledMCTS(cfg, np.random.RandomState(0), fused_transforms=True).fused_transforms == "identity"


# ------------------------------------------------------------------------------------------ GPU
def _lib():
    from mazero_amd._lib import load

    return load()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _launch(stage, n, value=None, vsup=(0, 0), reward=None, rsup=(0, 0), want_rc=0):
    """One mz_inverse_transform launch on the current stream; returns (value_out, reward_out)."""
    import torch

    lib = _lib()
    outs = []
    args = [None, C.c_void_p(torch.cuda.current_stream().cuda_stream), stage, n]
    for t, (lo, hi) in ((value, vsup), (reward, rsup)):
        if t is None:
            args += [None, 0, 0, lo, hi]
            outs.append(None)
        else:
            code = {torch.float32: _capi.MZ_DT_F32, torch.float16: _capi.MZ_DT_F16}.get(t.dtype, 7)
            args += [_ptr(t), code, t.stride(0), lo, hi]
            outs.append(torch.full((max(n, 1),), 7.0, dtype=torch.float32, device=t.device))
    rc = lib.mz_inverse_transform(*args, _ptr(outs[0]), _ptr(outs[1]))
    assert rc == want_rc, (rc, lib.mz_last_error())
    return outs


def _rows(n, S, seed, dtype, pad):
    """[n, S] logits (a view of [n, S + pad]): rows cycle through normal logits x 3, a constant row, a
    spread of +-60 (exponentials underflow to 0), -inf but one entry, a row holding a NaN, all -inf."""
    import torch

    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, S, generator=g) * 3
    kind = torch.arange(n) % 8
    x[kind == 3] = 1.25
    x[kind == 4] = (torch.rand(n, S, generator=g) * 120 - 60)[kind == 4]
    one = torch.randint(0, S, (n,), generator=g)
    keep = torch.zeros(n, S, dtype=torch.bool)
    keep[torch.arange(n), one] = True
    x[(kind == 5)[:, None] & ~keep] = float("-inf")
    x[(kind == 6)[:, None] & keep] = float("nan")
    x[kind == 7] = float("-inf")
    buf = torch.full((n, S + pad), 1000.0, dtype=dtype, device="cuda")  # (a read past the row would show)
    buf[:, :S] = x.to(dtype).cuda()
    return buf[:, :S]


def _bits(t):
    import torch

    return t.reshape(-1).contiguous().view(torch.int32)


def _assert_bits(got, want, what):
    import torch

    g, w = _bits(got), _bits(want)
    bad = torch.nonzero(g != w).reshape(-1)
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {g.numel()} differ; first at {int(bad[0])}: "
                              f"got {int(g[bad[0]]):#010x}, torch {int(w[bad[0]]):#010x}")


@pytest.mark.gpu
def test_expectation_stage_is_exact():
    """_inv_h alone over 2^20 floats: IEEE arithmetic on one float, no exception allowed."""
    import torch

    from mazero_amd.nets import inverse_h

    n = 1 << 20
    g = torch.Generator().manual_seed(1)
    x = torch.rand(n, generator=g) * 12 - 6
    q = n // 4
    x[q:2 * q] = torch.randint(-(1 << 31), (1 << 31) - 1, (q,), generator=g, dtype=torch.int64).to(torch.int32).view(
        torch.float32)
    x[2 * q:3 * q] = torch.rand(q, generator=g) * 600 - 300
    edge = torch.linspace(0.0004, 0.0006, q // 2)  # results on both sides of 0.001
    x[3 * q:3 * q + q // 2] = edge
    x[3 * q + q // 2:] = -edge
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-45, -1e-45, 1e-39, -1e-39,
                            1.1754942e-38, 300.0, -300.0])
    x[: special.numel()] = special
    x = x.cuda()
    with torch.autocast("cuda"):
        want = inverse_h(x.reshape(n, 1))
    v, r = _launch(_capi.MZ_INV_EXPECTATION, n, value=x, vsup=(-300, 300), reward=x, rsup=(-5, 5))
    _assert_bits(v, want, "value head")
    _assert_bits(r, want, "reward head")
    assert int((want != 0).sum()) > n // 2 and int((want == 0).sum()) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("S", SUPPORT_SIZES)
@pytest.mark.parametrize("stage", ["logits", "probs"])
def test_rows_match_torch(stage, S, dtype):
    """LOGITS and PROBS against the torch chain, for every row count (torch's launch shapes depend
    on it; the arithmetic must not), two heads with different supports and data per launch, and a
    row stride larger than S for two of the row counts."""
    import torch

    from mazero_amd.nets import inverse_h, inverse_support_transform, support_expectation

    dt = getattr(torch, dtype)
    lo = -(S // 2)
    vsup, rsup = (lo, lo + S - 1), (lo + 1, lo + S)
    for n in ROW_COUNTS:
        pad = 3 if n in (3, 257) else 0
        xv, xr = _rows(n, S, 100 + n, dt, pad), _rows(n, S, 200 + n, dt, pad)
        with torch.autocast("cuda"):
            if stage == "logits":
                want_v = inverse_support_transform(xv, *vsup)
                want_r = inverse_support_transform(xr, *rsup)
                v, r = _launch(_capi.MZ_INV_LOGITS, n, xv, vsup, xr, rsup)
            else:
                pv, pr = torch.softmax(xv, dim=-1), torch.softmax(xr, dim=-1)
                assert pv.dtype == torch.float32
                want_v = inverse_h(support_expectation(pv, *vsup))
                want_r = inverse_h(support_expectation(pr, *rsup))
                if pad:  # the probabilities in rows of S + pad elements
                    wide = torch.full((n, S + pad), 1000.0, dtype=torch.float32, device="cuda")
                    wide[:, :S] = pv
                    pv = wide[:, :S]
                v, r = _launch(_capi.MZ_INV_PROBS, n, pv, vsup, pr, rsup)
        _assert_bits(v, want_v, f"value head, n={n}")
        _assert_bits(r, want_r, f"reward head, n={n}")


@pytest.mark.gpu
def test_two_heads_and_one_head():
    """The value head on (-5, 5) and the reward head on (-2, 2) in one launch; either head alone."""
    import torch

    from mazero_amd.nets import inverse_support_transform

    n = 257
    xv, xr = _rows(n, 11, 5, torch.float16, 0), _rows(n, 5, 6, torch.float32, 2)
    with torch.autocast("cuda"):
        want_v, want_r = inverse_support_transform(xv, -5, 5), inverse_support_transform(xr, -2, 2)
    v, r = _launch(_capi.MZ_INV_LOGITS, n, xv, (-5, 5), xr, (-2, 2))
    _assert_bits(v, want_v, "value head")
    _assert_bits(r, want_r, "reward head")
    v, r = _launch(_capi.MZ_INV_LOGITS, n, xv, (-5, 5))
    assert r is None
    _assert_bits(v, want_v, "value head alone")
    v, r = _launch(_capi.MZ_INV_LOGITS, n, None, (0, 0), xr, (-2, 2))
    assert v is None
    _assert_bits(r, want_r, "reward head alone")


@pytest.mark.gpu
def test_argument_errors():
    import torch

    lib = _lib()
    x = torch.zeros(4, 65, device="cuda")
    _launch(_capi.MZ_INV_LOGITS, 4, x, (-32, 32), want_rc=_capi.MZ_ERR_UNSUPPORTED)
    assert b"support size > 64" in lib.mz_last_error()
    _launch(_capi.MZ_INV_PROBS, 4, x, (-32, 32), want_rc=_capi.MZ_ERR_UNSUPPORTED)
    _launch(_capi.MZ_INV_LOGITS, 4, x.double(), (-5, 5), want_rc=_capi.MZ_ERR_ARG)
    assert b"bad dtype" in lib.mz_last_error()
    _launch(_capi.MZ_INV_PROBS, 4, x.half(), (-5, 5), want_rc=_capi.MZ_ERR_ARG)  # probabilities are float32
    assert b"bad dtype" in lib.mz_last_error()
    _launch(_capi.MZ_INV_LOGITS, 4, x, (5, 4), want_rc=_capi.MZ_ERR_ARG)
    assert b"hi < lo" in lib.mz_last_error()
    _launch(_capi.MZ_INV_LOGITS, -1, x, (-5, 5), want_rc=_capi.MZ_ERR_ARG)
    assert b"n must be" in lib.mz_last_error()
    _launch(7, 4, x, (-5, 5), want_rc=_capi.MZ_ERR_ARG)
    assert b"bad stage" in lib.mz_last_error()
    v, _ = _launch(_capi.MZ_INV_EXPECTATION, 4, x[:, 0], (-32, 32))  # any support size, stride 65
    assert torch.count_nonzero(v).item() == 0


def _same(a, b):
    if isinstance(a, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _searches(K, cur, support):
    """Three searches (eager, recorded + replayed, replayed) by the default and by the fused driver
    from the same generator state; returns their outputs and the two recorded loops."""
    import torch

    from mazero_amd.mcts_sampled import _LOOPS, SampledMCTS
    from mazero_amd.nets import MuZeroShapedNet, SearchConfig, make_root_batch

    N, A, B, S = 3, 9, 32, 8
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=K, value_support=support,
                       reward_support=support)
    torch.manual_seed(3)
    net = MuZeroShapedNet(N, 64, A, support=support).to(dev).eval()
    factor = np.random.RandomState(5).randint(0, A, (B, N)).astype(np.int32) if cur else None
    outs = {}
    for fused in (False, True):
        drv = SampledMCTS(cfg, np.random.RandomState(11), fused_transforms=fused)
        outs[fused] = []
        for step in range(3):
            out, legal = make_root_batch(net, B, 64, seed=700 + step, device=dev, legal_zero_frac=0.2)
            outs[fused].append(drv.batch_search(net, out, cur, factor, N, legal, device=dev, add_noise=True))
    loops = {(v.fused is not None): v for v in _LOOPS.values() if v.model_ref() is net}
    return outs, loops, S, net


@pytest.mark.gpu
@pytest.mark.parametrize("K,cur,support", [(1, 0, (-5, 5)), (1, 1, (-5, 5)), (5, 0, (-5, 5)), (5, 1, (-5, 5)),
                                           (1, 0, (-300, 300))])
def test_fused_search_is_the_same_search(K, cur, support):
    """Every SearchOutput field of the fused driver equals the default driver's, bit for bit, on the
    eager first search and on the graph replays; supports (-300, 300) take the driver's route for
    more than 64 support elements."""
    import torch

    outs, loops, _, _ = _searches(K, cur, support)
    assert set(loops) == {False, True}
    for lp in loops.values():  # both loops were recorded and replayed
        assert isinstance(lp.graph, torch.cuda.CUDAGraph) and lp.runs == 3
    for step, (a, b) in enumerate(zip(outs[False], outs[True])):
        for name in a._fields:
            assert _same(getattr(a, name), getattr(b, name)), f"search {step}: {name} differs"


@pytest.mark.gpu
def test_launch_census():
    """The fused loop's recorded graph has at least 30 nodes per simulation fewer than the default
    loop's (_inv_h alone is 15 elementwise torch kernels per head)."""
    _, loops, S, _ = _searches(1, 0, (-5, 5))
    default_nodes, fused_nodes = loops[False].graph_nodes[0], loops[True].graph_nodes[0]
    print(f"graph nodes: default loop {default_nodes}, fused loop {fused_nodes}, {S} simulations")
    assert default_nodes - fused_nodes >= 30 * S
