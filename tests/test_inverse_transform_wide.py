"""mz_inverse_transform_wide, mz_inverse_sum_plan (include/mzdriver.h) and
SampledMCTS(fused_transforms=True, wide_supports=True): supports of 65 to 1,024 elements.

As in test_inverse_transform.py the target of every device comparison is the torch chain on the
same device under autocast (`mazero_amd.nets.inverse_support_transform`), as int32 bit patterns.
For these supports torch's sum reads the rows of its [n, S] input as aligned vectors and chooses
its block width from S and n, so the result of a row depends on the row's index and on the row
count: every comparison is against torch on the same n rows.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_inverse_transform import _assert_bits, _rows, _same  # the row recipe and the bit comparison

from mazero_amd import _capi

DRIVER_HEADER = os.path.join(ROOT, "include", "mzdriver.h")
# every softmax elements-per-lane count (2, 4, 8, 16), every regime of the sum (not vectorised below
# 128; block widths 32, 64, 128, 256) and every S mod 4
SUPPORT_SIZES = [65, 100, 127, 128, 130, 131, 255, 256, 257, 511, 512, 513, 601, 603, 1023, 1024]
# both sides of every block-width switch (n = 4, 8), and n >= 5 so that all four row alignments occur
ROW_COUNTS = [1, 2, 3, 4, 5, 7, 8, 9, 257]
PLAN_ROW_COUNTS = [1, 2, 3, 4, 7, 8, 9, 256, 511, 512, 1536]


# ------------------------------------------------------------------------------------------ CPU
def _declared(txt, name):
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", txt, re.M)
    assert m, f"{name} is not declared"
    ctype = {"mz_batch *": C.c_void_p, "void *": C.c_void_p, "const void *": C.c_void_p, "float *": C.c_void_p,
             "int": C.c_int, "int64_t": C.c_int64, "int *": C.POINTER(C.c_int)}
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        out.append(ctype[re.match(r"(.*?)(\w+)$", arg).group(1).strip()])
    return out


def test_ctypes_signatures_match_header():
    """The binding table's entries for the two new functions, argument by argument, against their
    declarations in include/mzdriver.h; the wide entry point has mz_inverse_transform's signature."""
    txt = open(DRIVER_HEADER).read()
    for name in ("mz_inverse_transform_wide", "mz_inverse_sum_plan"):
        res, args = _capi.DRIVER_SIGNATURES[name]
        assert res is C.c_int
        assert args == _declared(txt, name), name
    assert _capi.DRIVER_SIGNATURES["mz_inverse_transform_wide"] == _capi.DRIVER_SIGNATURES["mz_inverse_transform"]
    assert _declared(txt, "mz_inverse_transform_wide") == _declared(txt, "mz_inverse_transform")


def _last_pow2(n):
    n |= n >> 1
    n |= n >> 2
    n |= n >> 4
    n |= n >> 8
    n |= n >> 16
    return max(1, n - (n >> 1))


def _torch_plan(S, n):
    """ATen Reduce.cuh for a sum over the last dimension of a contiguous float32 [n, S] tensor:
    setReduceConfig's vectorisation rule and ReduceConfig::set_block_dimension (MAX_NUM_THREADS 512,
    input_vec_size 4, warp size 64)."""
    dim0, dim1, max_threads, warp = S, n, 512, 64
    vec = dim0 >= 128
    if vec:
        dim0 //= 4
    dim0_pow2 = _last_pow2(dim0) if dim0 < max_threads else max_threads
    dim1_pow2 = _last_pow2(dim1) if dim1 < max_threads else max_threads
    block_width = min(dim0_pow2, warp)
    block_height = min(dim1_pow2, max_threads // block_width)
    block_width = min(dim0_pow2, max_threads // block_height)
    return int(vec), block_width


def test_sum_plan_matches_set_block_dimension():
    from mazero_amd._lib import load

    lib = load()
    vec, bw = C.c_int(-1), C.c_int(-1)

    def plan(S, n):
        assert lib.mz_inverse_sum_plan(S, n, C.byref(vec), C.byref(bw)) == 0, lib.mz_last_error()
        return vec.value, bw.value

    for S in range(65, 1025):
        for n in PLAN_ROW_COUNTS:
            assert plan(S, n) == _torch_plan(S, n), (S, n)
    assert plan(601, 1) == (1, 128) and plan(601, 8) == (1, 64)
    assert plan(1024, 3) == (1, 256) and plan(1024, 4) == (1, 128)
    for n in PLAN_ROW_COUNTS:
        assert plan(200, n) == (1, 32)
        assert plan(100, n) == (0, 64)
    assert lib.mz_inverse_sum_plan(1025, 1, C.byref(vec), C.byref(bw)) == _capi.MZ_ERR_UNSUPPORTED
    assert lib.mz_inverse_sum_plan(601, 0, C.byref(vec), C.byref(bw)) == _capi.MZ_ERR_ARG
    assert lib.mz_inverse_sum_plan(601, 1, None, C.byref(bw)) == _capi.MZ_ERR_ARG


def test_wide_supports_flag():
    """The keyword and config.wide_supports, without a device; off by default; alone it changes nothing."""
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=9, value_support=(-300, 300), reward_support=(-300, 300))
    rng = np.random.RandomState(0)
    m = SampledMCTS(cfg, rng, fused_transforms=True, wide_supports=True)
    assert m.wide_supports is True and m.fused_transforms == ((-300, 300), (-300, 300))
    assert SampledMCTS(cfg, rng, fused_transforms=True).wide_supports is False
    assert SampledMCTS(cfg, rng).wide_supports is False
    alone = SampledMCTS(cfg, rng, wide_supports=True)
    assert alone.wide_supports is True and alone.fused_transforms is None
    cfg.wide_supports = True
    assert SampledMCTS(cfg, rng, fused_transforms=True).wide_supports is True
    assert SampledMCTS(cfg, rng, fused_transforms=True, wide_supports=False).wide_supports is False


# ------------------------------------------------------------------------------------------ GPU
def _lib():
    from mazero_amd._lib import load

    return load()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _launch(stage, n, value=None, vsup=(0, 0), reward=None, rsup=(0, 0), want_rc=0, fn="mz_inverse_transform_wide"):
    """One launch of `fn` on the current stream; returns (value_out, reward_out)."""
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
    rc = getattr(lib, fn)(*args, _ptr(outs[0]), _ptr(outs[1]))
    assert rc == want_rc, (rc, lib.mz_last_error())
    return outs


def _padded(p, pad):
    """`p` in rows of S + pad elements."""
    import torch

    n, S = p.shape
    wide = torch.full((n, S + pad), 1000.0, dtype=p.dtype, device=p.device)
    wide[:, :S] = p
    return wide[:, :S]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("S", SUPPORT_SIZES)
@pytest.mark.parametrize("stage", ["logits", "probs"])
def test_rows_match_torch(stage, S, dtype):
    """LOGITS and PROBS against the torch chain on the same n rows, for every row count, two heads
    with different supports and data per launch, and a row stride larger than S for two of the row
    counts.  No tolerance."""
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
                if pad:
                    pv = _padded(pv, pad)
                v, r = _launch(_capi.MZ_INV_PROBS, n, pv, vsup, pr, rsup)
        _assert_bits(v, want_v, f"value head, n={n}")
        _assert_bits(r, want_r, f"reward head, n={n}")
        # (the rows are not all zeros or NaN -> 0: the comparison sees the sums)
        assert int((want_v != 0).sum()) >= min(n, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("Sv,Sr", [(100, 1024), (601, 130), (601, 11), (16, 257)])
def test_heads_of_different_sizes(Sv, Sr):
    """Two heads whose supports differ in size in one launch (different elements per lane; a head of
    at most 64 elements beside a long one), and either head alone."""
    import torch

    from mazero_amd.nets import inverse_support_transform

    for n in (5, 8):
        xv, xr = _rows(n, Sv, 5, torch.float16, 0), _rows(n, Sr, 6, torch.float32, 2)
        vsup, rsup = (-(Sv // 2), -(Sv // 2) + Sv - 1), (-3, Sr - 4)
        with torch.autocast("cuda"):
            want_v, want_r = inverse_support_transform(xv, *vsup), inverse_support_transform(xr, *rsup)
        v, r = _launch(_capi.MZ_INV_LOGITS, n, xv, vsup, xr, rsup)
        _assert_bits(v, want_v, f"value head, n={n}")
        _assert_bits(r, want_r, f"reward head, n={n}")
        v, r = _launch(_capi.MZ_INV_LOGITS, n, xv, vsup)
        assert r is None
        _assert_bits(v, want_v, f"value head alone, n={n}")
        v, r = _launch(_capi.MZ_INV_LOGITS, n, None, (0, 0), xr, rsup)
        assert v is None
        _assert_bits(r, want_r, f"reward head alone, n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("stage", ["logits", "probs"])
def test_small_supports_give_the_narrow_bytes(stage):
    """S <= 64 through the wide entry point: the bytes of mz_inverse_transform."""
    import torch

    for S in (1, 2, 3, 11, 16, 17, 33, 64):
        for n in (1, 3, 257):
            xv, xr = _rows(n, S, 300 + n, torch.float16, 0), _rows(n, S, 400 + n, torch.float32, 3)
            code = _capi.MZ_INV_LOGITS
            if stage == "probs":
                xv, xr = torch.softmax(xv.float(), dim=-1), _padded(torch.softmax(xr, dim=-1), 3)
                code = _capi.MZ_INV_PROBS
            vsup, rsup = (-(S // 2), -(S // 2) + S - 1), (0, S - 1)
            wide = _launch(code, n, xv, vsup, xr, rsup)
            narrow = _launch(code, n, xv, vsup, xr, rsup, fn="mz_inverse_transform")
            _assert_bits(wide[0], narrow[0], f"value head, S={S}, n={n}")
            _assert_bits(wide[1], narrow[1], f"reward head, S={S}, n={n}")


@pytest.mark.gpu
def test_argument_errors():
    import torch

    lib = _lib()
    x = torch.zeros(4, 1025, device="cuda")
    _launch(_capi.MZ_INV_LOGITS, 4, x, (-512, 512), want_rc=_capi.MZ_ERR_UNSUPPORTED)
    assert b"mz_inverse_transform_wide" in lib.mz_last_error() and b"support size > 1024" in lib.mz_last_error()
    _launch(_capi.MZ_INV_PROBS, 4, x, (-512, 512), want_rc=_capi.MZ_ERR_UNSUPPORTED)
    v, _ = _launch(_capi.MZ_INV_EXPECTATION, 4, x[:, 0], (-512, 512))  # any support size, stride 1025
    assert torch.count_nonzero(v).item() == 0
    _launch(_capi.MZ_INV_LOGITS, 4, x.double(), (-300, 300), want_rc=_capi.MZ_ERR_ARG)
    assert b"bad dtype" in lib.mz_last_error()
    _launch(_capi.MZ_INV_PROBS, 4, x.half(), (-300, 300), want_rc=_capi.MZ_ERR_ARG)  # probabilities are float32
    _launch(_capi.MZ_INV_LOGITS, 4, x[:, :100].contiguous(), (-300, 300), want_rc=_capi.MZ_ERR_ARG)
    assert b"row stride below" in lib.mz_last_error()
    _launch(_capi.MZ_INV_LOGITS, 4, x, (5, 4), want_rc=_capi.MZ_ERR_ARG)
    assert b"hi < lo" in lib.mz_last_error()
    _launch(_capi.MZ_INV_LOGITS, -1, x, (-300, 300), want_rc=_capi.MZ_ERR_ARG)
    assert b"n must be" in lib.mz_last_error()
    _launch(7, 4, x, (-300, 300), want_rc=_capi.MZ_ERR_ARG)
    assert b"bad stage" in lib.mz_last_error()
    # the narrow entry point keeps its limit
    _launch(_capi.MZ_INV_LOGITS, 4, x[:, :65], (-32, 32), want_rc=_capi.MZ_ERR_UNSUPPORTED, fn="mz_inverse_transform")
    assert b"support size > 64" in lib.mz_last_error()


@functools.lru_cache(maxsize=None)
def _searches(K, cur, B):
    """Three searches (eager, recorded + replayed, replayed) with supports (-300, 300) by the fused
    driver without and with wide_supports, from the same generator state; returns their outputs and
    the two recorded loops."""
    import torch

    from mazero_amd.mcts_sampled import _LOOPS, SampledMCTS
    from mazero_amd.nets import MuZeroShapedNet, SearchConfig, make_root_batch

    N, A, S, support = 3, 9, 8, (-300, 300)
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=K, value_support=support,
                       reward_support=support)
    torch.manual_seed(3)
    net = MuZeroShapedNet(N, 64, A, support=support).to(dev).eval()
    factor = np.random.RandomState(5).randint(0, A, (B, N)).astype(np.int32) if cur else None
    outs = {}
    for wide in (False, True):
        drv = SampledMCTS(cfg, np.random.RandomState(11), fused_transforms=True, wide_supports=wide)
        outs[wide] = []
        for step in range(3):
            out, legal = make_root_batch(net, B, 64, seed=700 + step, device=dev, legal_zero_frac=0.2)
            outs[wide].append(drv.batch_search(net, out, cur, factor, N, legal, device=dev, add_noise=True))
    loops = {v.wide_supports: v for v in _LOOPS.values() if v.model_ref() is net}
    return outs, loops, S


@pytest.mark.gpu
@pytest.mark.parametrize("K,cur,B", [(1, 0, 32), (1, 1, 32), (5, 0, 32), (5, 1, 32), (1, 1, 4), (5, 0, 4)])
def test_wide_search_is_the_same_search(K, cur, B):
    """Every SearchOutput field with wide_supports equals the field without it (the EXPECTATION route
    behind torch's softmax, multiply and sum), bit for bit, on the eager first search and on the
    graph replays; B = 4 is below the row count at which torch's sum changes its block width."""
    import torch

    outs, loops, _ = _searches(K, cur, B)
    assert set(loops) == {False, True}
    for lp in loops.values():  # both loops were recorded and replayed
        assert lp.fused == ((-300, 300), (-300, 300))
        assert isinstance(lp.graph, torch.cuda.CUDAGraph) and lp.runs == 3
    for step, (a, b) in enumerate(zip(outs[False], outs[True])):
        for name in a._fields:
            assert _same(getattr(a, name), getattr(b, name)), f"search {step}: {name} differs"


@pytest.mark.gpu
def test_launch_census():
    """The wide loop's recorded graph has at least 5 nodes per simulation fewer than the EXPECTATION
    loop's: the two heads' softmax, multiply and sum are six torch launches."""
    _, loops, S = _searches(1, 0, 32)
    narrow_nodes, wide_nodes = loops[False].graph_nodes[0], loops[True].graph_nodes[0]
    print(f"graph nodes: EXPECTATION loop {narrow_nodes}, wide loop {wide_nodes}, {S} simulations")
    assert narrow_nodes - wide_nodes >= 5 * S
