"""Joint-action trees past 64 actions per agent and 64 sampled joint actions: mz_create_wide_joint
(`Tree_batch(..., wide_joint=True)`), the _joint_wide glue, `SampledMCTS(..., wide_joint=True)` and
`consume.select_joint_actions` on their wider outputs.

References: the CPU port (oracle/_build/libmzport.so) run with the same inputs, and the committed
fixtures tests/golden/joint_wide_<shape>.npz, which scripts/gen_joint_wide_golden.py records from the
reference's own ctree (libmzref).  Inputs are those of tests/test_gpu_parity.py's `_joint_run`: generator
seed 3, tree seed 17, eps = 0.25, Dirichlet rows.  Every comparison is bitwise: integers equal, floats
through their bit patterns."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GEN_SEED, TREE_SEED, EPS = 3, 17, 0.25
C2, C1, DISC = 19652.0, 1.25, 0.997

# (B, N, A, K, S) and the property the shape is there for: "deg" a root of more than 64 children, "act" an
# action >= 64, "idx" a selection past the root's children -- with the port's measured figures in the
# comments.  A shape that silently stops exercising the wide path fails its property.
SHAPES = [
    ((4, 2, 100, 5, 8), ("act", "idx")),       # wide A, narrow K; idx_x reaches 7
    ((3, 3, 255, 10, 6), ("act",)),            # A = 255
    ((2, 16, 255, 5, 4), ("act",)),            # N * A = 4080
    ((3, 2, 200, 200, 4), ("deg", "act")),     # root degrees 196-200: the readback past 64 children, wide A
    ((4, 3, 9, 100, 130), ("deg", "idx")),     # degrees 71-82, S past the forced round: > 64 children scored
    ((3, 2, 200, 70, 90), ("deg", "act", "idx")),  # both widths, degrees 69-70
    ((4, 5, 11, 128, 140), ("deg", "idx")),    # the int64 key wraps (N = 5) with K > 64, degrees 127-128
]
FIXTURE_SHAPES = [(4, 2, 100, 5, 8), (3, 2, 200, 70, 90), (4, 5, 11, 128, 140)]
LISTS = ("q", "acts", "vc", "pr", "bh")


def _sid(shape):
    return "B{}N{}A{}K{}S{}".format(*shape)


def fixture_path(shape):
    return os.path.join(GOLDEN, "joint_wide_b{}_n{}_a{}_k{}_s{}.npz".format(*shape))


def joint_run(lib, shape, wide_joint=False):
    """`_joint_run`'s recipe on `lib`: ([(idx_x [B], actions [B, N])] per simulation, readbacks)."""
    from mazero_amd.cytree import Tree_batch

    B, N, A, K, S = shape
    rng = np.random.default_rng(GEN_SEED)
    pol = lambda: rng.dirichlet([1.0] * A, (B, N)).astype(np.float32)  # noqa: E731
    p0, b0 = pol(), pol()
    noise = rng.dirichlet([0.3] * A, (B, N)).astype(np.float32)
    r0 = (0.1 * rng.standard_normal(B)).astype(np.float32)
    v0 = rng.standard_normal(B).astype(np.float32)
    tb = Tree_batch(B, N, A, K, S, 0.01, TREE_SEED, 0.75, 0.8, lib=lib, wide_joint=wide_joint)
    tb.prepare(r0, v0, p0, b0, K, EPS, noise)
    rec = []
    for s in range(S):
        ix, _, act = tb.batch_selection(C2, C1, DISC)
        rec.append((np.asarray(ix, np.int32).copy(), np.asarray(act, np.int32).reshape(B, N).copy()))
        r = (0.1 * rng.standard_normal(B)).astype(np.float32)
        v = rng.standard_normal(B).astype(np.float32)
        p, b = pol(), pol()
        tb.batch_expansion_and_backup(s + 1, DISC, K, r, v, p, b)
    out = dict(values=tb.get_roots_values(), mv=tb.get_roots_marginal_visit_count(),
               mp=tb.get_roots_marginal_priors(), q=tb.get_roots_sampled_qvalues(DISC),
               acts=tb.get_roots_sampled_actions(), vc=tb.get_roots_sampled_visit_count(),
               pr=tb.get_roots_sampled_priors(), bh=tb.get_roots_sampled_beta_hat())
    return rec, out, tb


def pack(shape, rec, out):
    """The arrays of a fixture file: the seed recipe, every simulation's idx_x and [B, N] actions, and the
    readbacks (the per-root lists concatenated in root order, with the roots' degrees)."""
    z = dict(cfg=np.array(shape, np.int32), seeds=np.array([GEN_SEED, TREE_SEED], np.int32),
             knobs=np.array([C2, C1, DISC, 0.01, 0.75, 0.8, EPS], np.float64),
             idx_x=np.stack([r[0] for r in rec]).astype(np.int32), actions=np.stack([r[1] for r in rec]).astype(np.int32),
             values=np.asarray(out["values"]), mv=np.asarray(out["mv"]), mp=np.asarray(out["mp"]),
             deg=np.array([len(v) for v in out["vc"]], np.int32))
    for k in LISTS:
        z[k] = np.concatenate([np.asarray(v) for v in out[k]])
    return z


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype.kind == "f" else a


def _same(got, exp, where):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (where, got.dtype, exp.dtype, got.shape, exp.shape)
    np.testing.assert_array_equal(_bits(got), _bits(exp), err_msg=where)


def _same_run(got, exp, where=""):
    (rec_g, out_g), (rec_e, out_e) = got, exp
    assert len(rec_g) == len(rec_e)
    for s, ((ig, ag), (ie, ae)) in enumerate(zip(rec_g, rec_e)):
        _same(ig, ie, f"{where}idx_x of simulation {s}")
        _same(ag, ae, f"{where}actions of simulation {s}")
    for k in ("values", "mv", "mp"):
        _same(out_g[k], out_e[k], where + k)
    for k in LISTS:
        assert len(out_g[k]) == len(out_e[k]), (where, k)
        for i, (g, e) in enumerate(zip(out_g[k], out_e[k])):
            _same(g, e, f"{where}{k}[{i}]")


def _same_fixture(shape, rec, out, where):
    z = np.load(fixture_path(shape))
    assert tuple(int(x) for x in z["cfg"]) == tuple(shape)
    assert [int(x) for x in z["seeds"]] == [GEN_SEED, TREE_SEED]
    got = pack(shape, rec, out)
    for k in z.files:
        _same(got[k], z[k], f"{where} fixture {k}")


def _check_properties(shape, props, rec, out):
    B, N, A, K, S = shape
    assert (np.asarray(out["mv"]).sum(axis=2) == S).all()  # every agent's marginal sums to the simulations
    max_deg = max(len(v) for v in out["vc"])
    max_act = max(int(a.max()) for _, a in rec)
    max_idx = max(int(i.max()) for i, _ in rec)
    print(f"{_sid(shape)}: max root degree {max_deg}, max action {max_act}, max idx_x {max_idx}")
    if "deg" in props:
        assert max_deg > 64
    if "act" in props:
        assert max_act >= 64
    if "idx" in props:
        assert max_idx > 0
    assert all(a.shape == (len(v), N) for a, v in zip(out["acts"], out["vc"]))


@pytest.fixture(scope="module")
def port_runs(port_lib):
    """The port's run of each shape, computed once and shared (never modified)."""
    cache = {}

    def get(shape):
        if shape not in cache:
            rec, out, _ = joint_run(port_lib, shape)
            cache[shape] = (rec, out)
        return cache[shape]

    return get


@pytest.fixture(scope="module")
def gpu_lib():
    from mazero_amd._lib import load

    return load()


# ------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FIXTURE_SHAPES, ids=_sid)
def test_port_reproduces_fixture(shape, port_runs):
    rec, out = port_runs(shape)
    _same_fixture(shape, rec, out, "port")
    _check_properties(shape, dict(SHAPES)[shape], rec, out)


@pytest.mark.parametrize("shape", FIXTURE_SHAPES, ids=_sid)
def test_reference_reproduces_fixture(shape, ref_lib):
    rec, out, _ = joint_run(ref_lib, shape)
    _same_fixture(shape, rec, out, "reference")


def test_wide_joint_constructor():
    """wide_joint=True accepts A <= 255, as wide_actions does; 256 raises; config.wide_joint is read."""
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=200)
    assert SampledMCTS(cfg, wide_joint=True).wide_joint is True
    assert SampledMCTS(SearchConfig(action_space_size=9)).wide_joint is False
    with pytest.raises(RuntimeError, match="action_space_size 200"):
        SampledMCTS(cfg)
    with pytest.raises(RuntimeError, match="action_space_size 256"):
        SampledMCTS(SearchConfig(action_space_size=256), wide_joint=True)

    class Cfg:
        def __init__(self, base, **extra):
            self.__dict__.update(base.__dict__)
            self.__dict__.update(extra)

    assert SampledMCTS(Cfg(cfg, wide_joint=True)).wide_joint is True
    with pytest.raises(RuntimeError, match="action_space_size 200"):  # the argument wins over the config
        SampledMCTS(Cfg(cfg, wide_joint=True), wide_joint=False)
    with pytest.raises(RuntimeError, match="action_space_size 200"):
        SampledMCTS(Cfg(cfg, wide_joint=False))


def test_driver_exports_list_the_wide_joint_entry_points():
    from mazero_amd import _capi

    for name in ("mz_create_wide_joint", "mz_policy_glue_joint_wide", "mz_root_glue_joint_wide"):
        assert name in _capi.DRIVER_EXPORTS and name not in _capi.EXPORTS
    assert _capi.DRIVER_SIGNATURES["mz_create_wide_joint"][1][:5] == [C.c_int] * 5


# ------------------------------------------------------------------------------------------------
# GPU: tree level
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,props", SHAPES, ids=[_sid(s) for s, _ in SHAPES])
def test_wide_joint_trees_vs_port(shape, props, gpu_lib, port_runs):
    rec, out, tb = joint_run(gpu_lib, shape, wide_joint=True)
    assert tb.fused_kernel() == "k_hbm<joint>"
    _same_run((rec, out), port_runs(shape), _sid(shape) + ": ")
    if shape in FIXTURE_SHAPES:
        _same_fixture(shape, rec, out, "GPU")
    _check_properties(shape, props, rec, out)
    B, N, A, K, S = shape
    assert tb.max_children() == min(K, A ** N)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(32, 3, 9, 5, 30), (16, 5, 11, 10, 20)], ids=["3m_n3_k5", "n5_k10_keywrap"])
def test_wide_joint_handle_inside_narrow_bounds_is_mz_create(shape, gpu_lib):
    """Inside mz_create's joint bounds mz_create_wide_joint builds mz_create's handle: the same
    mz_fused_kernel and prepare kernel names, identical outputs."""
    rec_w, out_w, tb_w = joint_run(gpu_lib, shape, wide_joint=True)
    rec_n, out_n, tb_n = joint_run(gpu_lib, shape, wide_joint=False)
    assert tb_w.fused_kernel() == tb_n.fused_kernel() == "k_step<0,joint>"
    assert tb_w.prepare_kernel() == tb_n.prepare_kernel()
    assert tb_w.max_children() == tb_n.max_children()
    _same_run((rec_w, out_w), (rec_n, out_n))


@pytest.mark.gpu
def test_wide_joint_one_agent_is_mz_create(gpu_lib):
    """N = 1 through mz_create_wide_joint: the one-agent handle (A = 100: k_hbm, as without the flag)."""
    from mazero_amd.cytree import Tree_batch

    a = Tree_batch(4, 1, 100, 5, 10, 0.01, 1, 0.75, 0.8, lib=gpu_lib, wide_joint=True)
    b = Tree_batch(4, 1, 100, 5, 10, 0.01, 1, 0.75, 0.8, lib=gpu_lib)
    assert a.fused_kernel() == b.fused_kernel() == "k_hbm"


# ------------------------------------------------------------------------------------------------
# GPU: refusals of the new entry point
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,A,K,bound", [(2, 256, 5, "action_space_size > 255"), (2, 9, 256, "sampled_times <= 255"),
                                         (65, 9, 5, "agent_num <= 64"),
                                         (17, 255, 5, r"agent_num \* action_space_size <= 4096")],
                         ids=["A256", "K256", "N65", "N17A255"])
def test_wide_joint_refusals(N, A, K, bound, gpu_lib):
    from mazero_amd._capi import MZ_ERR_UNSUPPORTED, MZError
    from mazero_amd.cytree import Tree_batch

    h = C.c_void_p()
    rc = gpu_lib.mz_create_wide_joint(4, N, A, K, 8, 0.01, 1, 0.75, 0.8, 0, C.byref(h))
    assert rc == MZ_ERR_UNSUPPORTED and not h.value
    with pytest.raises(MZError, match=bound):
        Tree_batch(4, N, A, K, 8, 0.01, 1, 0.75, 0.8, lib=gpu_lib, wide_joint=True)


# ------------------------------------------------------------------------------------------------
# GPU: glue
# ------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("A", [65, 100, 255])
def test_joint_wide_glue_is_the_wide_kernel_per_agent(A, dtype, gpu_lib):
    """Slice k of the _joint_wide outputs holds the bytes of the per-agent _wide call with
    col_offset = k * A: N in {1, 2, 3}, legal masks with zeros and none, noise on and off, B = 5, row
    stride N * A + 3."""
    import torch

    from mazero_amd._capi import MZ_DT_F16, MZ_DT_F32, check
    from mazero_amd.cytree import Tree_batch
    from mazero_amd.mcts_sampled import ensure_half_exp

    B, dev = 5, torch.device("cuda", 0)
    code = MZ_DT_F16 if dtype == "float16" else MZ_DT_F32
    tb = Tree_batch(B, 1, A, 1, 4, 0.01, 0, 0.75, 0.8, lib=gpu_lib)
    ensure_half_exp(gpu_lib, torch.cuda.current_device())
    tb._sync_stream()
    lib, h = gpu_lib, tb._h
    for N in (1, 2, 3):
        rng = np.random.default_rng(1000 * A + N)
        v = (rng.standard_normal((B, N, A)) * np.array([1, 1, 0.1, 4, 30]).reshape(B, 1, 1)).astype(dtype)
        v[1, N - 1, 0] = -np.inf
        v[3, 0, :] = v[3, 0, 0]
        full = rng.standard_normal((B, N * A + 3)).astype(dtype)
        full[:, :N * A] = v.reshape(B, N * A)
        x = torch.from_numpy(full).to(dev)
        stride = full.shape[1]
        noise = rng.dirichlet([0.3] * A, (B, N)).astype(np.float32)
        legal = (rng.random((B, N, A)) >= 0.3).astype(np.int32)
        legal[..., 0] = np.where(legal.sum(-1) == 0, 1, legal[..., 0])
        nz, lgl = torch.from_numpy(noise).to(dev), torch.from_numpy(legal).to(dev)
        for tau in (1.0, 0.5):
            probs, beta = (torch.full((B, N, A), -7.0, device=dev) for _ in range(2))
            check(lib, lib.mz_policy_glue_joint_wide(h, _p(x), code, stride, N, tau, _p(probs), _p(beta)), "glue")
            for k in range(N):
                p1, b1 = (torch.full((B, A), -7.0, device=dev) for _ in range(2))
                check(lib, lib.mz_policy_glue_wide(h, _p(x), code, stride, k * A, tau, _p(p1), _p(b1)), "glue")
                _same(probs[:, k, :].cpu().numpy(), p1.cpu().numpy(), f"policy probs N={N} agent {k} tau={tau}")
                _same(beta[:, k, :].cpu().numpy(), b1.cpu().numpy(), f"policy beta N={N} agent {k} tau={tau}")
            for has_legal in (False, True):
                for eps in (0.0, 0.25):
                    outs = [torch.full((B, N, A), -7.0, device=dev) for _ in range(3)]
                    check(lib, lib.mz_root_glue_joint_wide(h, _p(x), code, stride, N, _p(lgl) if has_legal else None,
                                                           N * A, _p(nz), eps, tau, *[_p(o) for o in outs]), "glue")
                    for k in range(N):
                        nk = nz[:, k, :].contiguous()
                        lk = lgl[:, k, :].contiguous() if has_legal else None
                        one = [torch.full((B, A), -7.0, device=dev) for _ in range(3)]
                        check(lib, lib.mz_root_glue_wide(h, _p(x), code, stride, k * A, _p(lk), A, _p(nk), eps, tau,
                                                         *[_p(o) for o in one]), "glue")
                        for name, g, o in zip(("probs", "beta", "noise"), outs, one):
                            _same(g[:, k, :].cpu().numpy(), o.cpu().numpy(),
                                  f"root {name} N={N} agent {k} legal={has_legal} eps={eps} tau={tau}")


# ------------------------------------------------------------------------------------------------
# GPU: consumer
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_select_joint_actions_on_wide_output(gpu_lib):
    """consume.select_joint_actions, deterministic and sampled, on the (3, 2, 200, 200, 4) search's output
    (roots of 196-200 children, actions up to 199) against oracle/consume.py's select_action and the row
    gather of core/test.py:107: positions and action rows exact."""
    import torch

    from consume import select_action
    from mazero_amd.consume import select_joint_actions
    from mazero_amd.mcts_sampled import DeviceSearchOutput

    shape = (3, 2, 200, 200, 4)
    B, N, A, K, S = shape
    rec, out, tb = joint_run(gpu_lib, shape, wide_joint=True)
    dev = torch.device("cuda", 0)
    W = tb.max_children()
    assert W == 200
    deg = torch.empty(B, dtype=torch.int32, device=dev)
    vis = torch.empty(B, W, dtype=torch.int32, device=dev)
    act = torch.empty(B, W * N, dtype=torch.int32, device=dev)
    tb.get_roots_device(DISC, degrees=deg, sampled={"visit_count": vis, "actions": act})
    torch.cuda.synchronize()
    assert int(deg.max()) > 64
    for i in range(B):  # the device readback is the host readback
        d = int(deg[i])
        _same(vis[i, :d].cpu().numpy(), out["vc"][i], f"visits of root {i}")
        _same(act[i].cpu().numpy().reshape(W, N)[:d], out["acts"][i], f"actions of root {i}")
    dout = DeviceSearchOutput(None, torch.zeros(B, N, A, dtype=torch.int32, device=dev), None, deg,
                              {"visit_count": vis, "actions": act}, tb)
    u = np.random.RandomState(5).random(B)
    for temperature, deterministic in ((1.0, True), (1.0, False), (0.5, False)):
        rs = np.random.RandomState(5)  # (one double per root, in root order)
        ga, gp, _ = select_joint_actions(dout, temperature, deterministic,
                                         None if deterministic else torch.from_numpy(u).to(dev))
        for i in range(B):
            p, _ = select_action(out["vc"][i], temperature=temperature, deterministic=deterministic, np_random=rs)
            assert int(gp[i]) == p, (temperature, deterministic, i)
            np.testing.assert_array_equal(ga[i].cpu().numpy(), out["acts"][i][p])


# ------------------------------------------------------------------------------------------------
# GPU: whole searches against the restated joint driver on the port
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 100, 5, 8, 4), (2, 9, 100, 12, 4)], ids=["N2A100K5S8B4", "N2A9K100S12B4"])
def test_wide_joint_search_matches_restated_driver(shape, port_lib):
    """Three consecutive batch_search_joint calls on one wide_joint driver (eager, capture, replay)
    against tests/joint_driver_fixture.py on the port: every SearchOutput field and np_random."""
    from mazero_amd.mcts_sampled import release
    from test_joint_search import _three_searches

    release()
    try:
        loop = _three_searches(shape, port_lib, wide_joint=True)
        assert loop.tb.wide_joint and loop.tb.fused_kernel() == "k_hbm<joint>"
        assert loop.tb.agent_num == shape[0]
    finally:
        release()
