"""The joint search: `SampledMCTS.batch_search_joint` (one search over joint-action trees, the call of
the reference's evaluation loop, core/test.py:84), its device glue (mz_policy_glue_joint,
mz_root_glue_joint, include/mzdriver.h) and its consumer (mz_select_actions_joint,
`consume.select_joint_actions`).

The checker is tests/joint_driver_fixture.py: the reference driver restated for num_agents = N.  On the
CPU that restatement runs on the reference's own ctree and on the CPU port and must agree with itself;
on the GPU the device driver must agree with it on the port, field by field.  Every comparison is
bitwise: integers equal, floats through their bit patterns."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

# (N, A, K, S, B): K = 5 samples of 9^3 joint actions; a small action space where children collide;
# K = 1 chains; eight agents, past the four whose actions fit the int64 child key without wrapping
SHAPES = [(3, 9, 5, 20, 8), (2, 3, 5, 12, 4), (3, 9, 1, 20, 8), (8, 6, 8, 24, 4)]
SHAPE_IDS = [f"N{n}A{a}K{k}S{s}B{b}" for n, a, k, s, b in SHAPES]
FIELDS = ("value", "marginal_visit_count", "marginal_priors", "sampled_actions", "sampled_visit_count",
          "sampled_pred_probs", "sampled_beta", "sampled_beta_hat", "sampled_priors", "sampled_imp_ratio",
          "sampled_pred_values", "sampled_mcts_values", "sampled_rewards", "sampled_qvalues")


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        return a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return a


def _same(got, exp, where):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (where, got.dtype, exp.dtype, got.shape, exp.shape)
    np.testing.assert_array_equal(_bits(got), _bits(exp), err_msg=where)


def _compare(got, exp, where=""):
    """Every SearchOutput field of `got` (a SearchOutput or a dict) against the dict `exp`."""
    for name in FIELDS:
        g = got[name] if isinstance(got, dict) else getattr(got, name)
        e = exp[name]
        if isinstance(e, list):
            assert len(g) == len(e), (where, name)
            for i, (gi, ei) in enumerate(zip(g, e)):
                _same(gi, ei, f"{where}{name}[{i}]")
        else:
            _same(g, e, f"{where}{name}")


def _rng_state_equal(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


# ------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_restated_joint_driver_ref_equals_port(shape, ref_lib, port_lib):
    """The restated joint driver on the reference's own ctree equals itself on the CPU port: every
    simulation's selection (idx_x, idy, the [B, N] actions), every SearchOutput field and the generator
    state afterwards."""
    import torch

    from joint_driver_fixture import JointOracleSampledMCTS
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch

    N, A, K, S, B = shape
    cfg = SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=K)
    net = make_net(N, A, seed=3)
    out, legal = make_root_batch(net, B, 64, seed=4, device=torch.device("cpu"), legal_zero_frac=0.3)
    rs_r, rs_p = np.random.RandomState(11), np.random.RandomState(11)
    ref, port = JointOracleSampledMCTS(cfg, rs_r, ref_lib), JointOracleSampledMCTS(cfg, rs_p, port_lib)
    exp = ref.batch_search_joint(net, out, legal, None, True, 1.0)
    got = port.batch_search_joint(net, out, legal, None, True, 1.0)
    assert len(ref.trace) == len(port.trace) == S
    for s, (r, p) in enumerate(zip(ref.trace, port.trace)):
        for what, a, b in zip(("idx_x", "idy", "actions"), r, p):
            np.testing.assert_array_equal(b, a, err_msg=f"simulation {s} {what}")
    _compare(got, exp)
    assert exp["marginal_visit_count"].shape == (B, N, A)
    assert all(a.shape[1] == N for a in exp["sampled_actions"])
    assert _rng_state_equal(rs_r, rs_p)
    if S > K:  # (the searches leave the roots' children: the deepest hidden_state_index_x is past 0)
        assert max(int(t[0].max()) for t in port.trace) > 0


def test_joint_search_draws(port_lib):
    """What a joint search consumes from np_random -- (B, N) Dirichlet rows, then the tree seed -- is
    what skip_search_draws(..., num_agents=N) and SampledMCTS's root preprocessing consume; (B, 1) rows
    are the B rows of a one-agent search."""
    import torch

    from joint_driver_fixture import JointOracleSampledMCTS
    from mazero_amd.mcts_sampled import SampledMCTS, skip_search_draws
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch

    N, A, K, S, B = 3, 9, 5, 6, 8
    cfg = SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=K)
    net = make_net(N, A, seed=3)
    out, legal = make_root_batch(net, B, 64, seed=4, device=torch.device("cpu"), legal_zero_frac=0.3)
    rs = [np.random.RandomState(5) for _ in range(4)]
    JointOracleSampledMCTS(cfg, rs[0], port_lib).batch_search_joint(net, out, legal, None, True, 1.0)
    skip_search_draws(cfg, rs[1], B, N)
    (_, _, probs, beta, _, noises), _ = SampledMCTS(cfg, rs[2]).root_inputs(out, None, legal, True, 1.0)
    arrays, mode, _, _ = SampledMCTS(cfg, rs[3]).root_raw(out, None, legal, True)
    assert probs.shape == beta.shape == noises.shape == (B, N, A)
    assert arrays["noise"].shape == (B, N, A) and arrays["legal"].shape == (B, N, A) and mode[1]
    for r in rs[1:]:
        assert _rng_state_equal(rs[0], r)
    # an empty root shard skips what the other ranks' joint search draws: (total, N) rows, then the seed
    a, b = np.random.RandomState(6), np.random.RandomState(6)
    SampledMCTS(cfg, a, root_shard=(2, 2, 7), device_root_offset=True).skip_search(N)
    skip_search_draws(cfg, b, 7, N)
    assert _rng_state_equal(a, b)
    a, b = np.random.RandomState(6), np.random.RandomState(6)
    skip_search_draws(cfg, a, B, 1)
    skip_search_draws(cfg, b, B)
    assert _rng_state_equal(a, b)
    np.testing.assert_array_equal(np.random.RandomState(7).dirichlet([0.3] * A, (B, N)).reshape(B * N, A),
                                  np.random.RandomState(7).dirichlet([0.3] * A, B * N))


@pytest.mark.parametrize("temperature", [1.0, 0.5, 0.25])
def test_select_joint_actions_host_is_select_action(temperature):
    """The host restatement of select_joint_actions agrees with select_action as oracle/consume.py
    restates core/utils.py:289-316, plus the row gather of core/test.py:107 -- deterministic, and
    sampled with the doubles np_random.choice draws."""
    from consume import select_action
    from joint_driver_fixture import select_joint_actions_host

    rng = np.random.default_rng(int(temperature * 100))
    B, N = 40, 3
    visits = [rng.integers(0, 9, size=rng.integers(1, 7)).astype(np.int32) for _ in range(B)]
    for v in visits:
        v[rng.integers(len(v))] += 1  # (select_action asserts a visit)
    visits[0][:] = visits[0][0]  # ties: the first maximum
    actions = [rng.integers(0, 9, size=(len(v), N)).astype(np.int32) for v in visits]
    acts, pos, ent = select_joint_actions_host(actions, visits, temperature, True)
    for i in range(B):
        p, h = select_action(visits[i], temperature=temperature, deterministic=True)
        assert pos[i] == p and np.array_equal(acts[i], actions[i][p])
        assert _bits(np.float64(ent[i])) == _bits(np.float64(h))
    rs = np.random.RandomState(3)
    u = np.random.RandomState(3).random(B)  # one double per root, in root order
    acts, pos, ent = select_joint_actions_host(actions, visits, temperature, False, u)
    for i in range(B):
        p, h = select_action(visits[i], temperature=temperature, deterministic=False, np_random=rs)
        assert pos[i] == p and np.array_equal(acts[i], actions[i][p])
        assert _bits(np.float64(ent[i])) == _bits(np.float64(h))
    # a root without children, and one without visits
    acts, pos, ent = select_joint_actions_host(
        [np.zeros((0, N), np.int32), np.ones((2, N), np.int32)], [np.zeros(0, np.int32), np.zeros(2, np.int32)])
    assert (acts == -1).all() and (pos == -1).all() and np.isnan(ent).all()


# ------------------------------------------------------------------------------------------------
# GPU: the glue against the existing kernels
# ------------------------------------------------------------------------------------------------
def _handle(B, A, N=1):
    import torch

    from mazero_amd.cytree import Tree_batch
    from mazero_amd.mcts_sampled import ensure_half_exp

    tb = Tree_batch(B, N, A, 1, 4, 0.01, 0, 0.75, 0.8)
    ensure_half_exp(tb._lib, torch.cuda.current_device())  # (as the search loop does)
    tb._sync_stream()
    return tb


def _code(dtype):
    from mazero_amd._capi import MZ_DT_F16, MZ_DT_F32

    return MZ_DT_F16 if np.dtype(dtype) == np.float16 else MZ_DT_F32


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


GLUE_B = 5


def _glue_logits(rng, N, A, dtype, pad=3):
    """[B, N * A + pad] rows (row stride N * A + 3): random logits of several scales; agent 0 of root 0
    holds a NaN, agent 1 of root 1 a -inf, agent 0 of root 2 a +inf, agent 1 of root 3 equal logits."""
    B = GLUE_B
    v = (rng.standard_normal((B, N, A)) * np.array([1, 1, 0.1, 4, 30]).reshape(B, 1, 1)).astype(dtype)
    v[0, 0, A - 1] = np.nan
    v[1, 1, 0] = -np.inf
    v[2, 0, A // 2] = np.inf
    v[3, 1, :] = v[3, 1, 0]
    full = rng.standard_normal((B, N * A + pad)).astype(dtype)  # (the pad columns are never read)
    full[:, :N * A] = v.reshape(B, N * A)
    return full, v


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("A", [1, 3, 9, 11, 64])
def test_policy_glue_joint_is_the_narrow_kernel_per_agent(A, dtype):
    """mz_policy_glue_joint, one launch (mz_policy_glue's kernel with an agent per grid row), against N
    launches of mz_policy_glue stacked and against the numpy expression (mcts_sampled.py:158-161), for
    N in {2, 3, 8}, B = 5, row stride N * A + 3, with rows holding a NaN, -inf, +inf and all-equal
    logits; tau 1 and 0.5."""
    import torch

    from mazero_amd._capi import check

    B, dev = GLUE_B, torch.device("cuda", 0)
    tb = _handle(B, A)
    lib = tb._lib
    for N in (2, 3, 8):
        full, view = _glue_logits(np.random.default_rng(100 * A + N), N, A, dtype)
        x = torch.from_numpy(full).to(dev)
        stride = full.shape[1]
        for tau in (1.0, 0.5):
            probs, beta = (torch.full((B, N, A), -7.0, device=dev) for _ in range(2))
            check(lib, lib.mz_policy_glue_joint(tb._h, _p(x), _code(dtype), stride, N, tau, _p(probs), _p(beta)),
                  "policy_glue_joint")
            gp, gb = probs.cpu().numpy(), beta.cpu().numpy()
            for k in range(N):
                p1, b1 = (torch.full((B, A), -7.0, device=dev) for _ in range(2))
                check(lib, lib.mz_policy_glue(tb._h, _p(x), _code(dtype), stride, k * A, tau, _p(p1), _p(b1)),
                      "policy_glue")
                _same(gp[:, k, :], p1.cpu().numpy(), f"probs N={N} agent {k} tau={tau} vs mz_policy_glue")
                _same(gb[:, k, :], b1.cpu().numpy(), f"beta N={N} agent {k} tau={tau} vs mz_policy_glue")
            with np.errstate(all="ignore"):  # numpy: the exponents 1, and 2 (np.square) in the logits' dtype
                p = np.exp(view - np.max(view, axis=-1, keepdims=True))
                p = p / np.sum(p, axis=-1, keepdims=True)
                b = p ** (1 / tau)
                b = b / np.sum(b, axis=-1, keepdims=True)
            print(f"A={A} {dtype} N={N} tau={tau}: probs mismatches vs numpy "
                  f"{(_bits(gp) != _bits(p.astype(np.float32))).sum()}, beta "
                  f"{(_bits(gb) != _bits(b.astype(np.float32))).sum()}")
            _same(gp, p.astype(np.float32), f"probs N={N} tau={tau} vs numpy")
            _same(gb, b.astype(np.float32), f"beta N={N} tau={tau} vs numpy")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("A", [1, 3, 9, 11, 64])
def test_root_glue_joint_is_the_narrow_kernel_per_agent(A, dtype):
    """mz_root_glue_joint (mz_root_glue's kernel with an agent per grid row) against N launches of
    mz_root_glue on the agent's own logits, legal and noise columns: with and without `legal` (at least
    one legal action per (root, agent)), eps in {0, 0.25}, tau in {1, 0.5}, N in {2, 3, 8}, B = 5, row
    stride N * A + 3."""
    import torch

    from mazero_amd._capi import check

    B, dev = GLUE_B, torch.device("cuda", 0)
    tb = _handle(B, A)
    lib = tb._lib
    for N in (2, 3, 8):
        rng = np.random.default_rng(1000 * A + N)
        full, _ = _glue_logits(rng, N, A, dtype)
        x = torch.from_numpy(full).to(dev)
        stride = full.shape[1]
        noise = rng.dirichlet([0.3] * A, (B, N)).astype(np.float32)
        legal = (rng.random((B, N, A)) >= 0.3).astype(np.int32)
        legal[..., 0] = np.where(legal.sum(-1) == 0, 1, legal[..., 0])
        nz, lgl = torch.from_numpy(noise).to(dev), torch.from_numpy(legal).to(dev)
        for has_legal in (False, True):
            for eps in (0.0, 0.25):
                for tau in (1.0, 0.5):
                    outs = [torch.full((B, N, A), -7.0, device=dev) for _ in range(3)]
                    check(lib, lib.mz_root_glue_joint(tb._h, _p(x), _code(dtype), stride, N,
                                                      _p(lgl) if has_legal else None, N * A, _p(nz), eps, tau,
                                                      *[_p(o) for o in outs]), "root_glue_joint")
                    got = [o.cpu().numpy() for o in outs]
                    for k in range(N):
                        nk = nz[:, k, :].contiguous()
                        lk = lgl[:, k, :].contiguous() if has_legal else None
                        one = [torch.full((B, A), -7.0, device=dev) for _ in range(3)]
                        check(lib, lib.mz_root_glue(tb._h, _p(x), _code(dtype), stride, k * A, _p(lk), A, _p(nk),
                                                    eps, tau, *[_p(o) for o in one]), "root_glue")
                        for name, g, o in zip(("probs", "beta", "noise"), got, one):
                            _same(g[:, k, :], o.cpu().numpy(),
                                  f"{name} N={N} agent {k} legal={has_legal} eps={eps} tau={tau}")


@pytest.mark.gpu
def test_joint_glue_refuses_wide_action_spaces():
    """A > 64: MZ_ERR_UNSUPPORTED with the bound in the message; too short rows: ValueError."""
    import torch

    from mazero_amd._capi import MZ_DT_F32, MZError, check

    B, A, N, dev = 3, 65, 1, torch.device("cuda", 0)
    tb = _handle(B, A)
    lib = tb._lib
    x = torch.zeros(B, N * A, device=dev)
    o = [torch.zeros(B, N, A, device=dev) for _ in range(3)]
    with pytest.raises(MZError, match="action_space_size > 64"):
        check(lib, lib.mz_policy_glue_joint(tb._h, _p(x), MZ_DT_F32, N * A, N, 1.0, _p(o[0]), _p(o[1])), "glue")
    with pytest.raises(MZError, match="action_space_size > 64"):
        check(lib, lib.mz_root_glue_joint(tb._h, _p(x), MZ_DT_F32, N * A, N, None, 0, _p(x), 0.0, 1.0,
                                          *[_p(t) for t in o]), "glue")
    tb = _handle(B, 9)
    with pytest.raises(ValueError, match="every agent"):
        check(lib, lib.mz_policy_glue_joint(tb._h, _p(x), MZ_DT_F32, 17, 2, 1.0, _p(o[0]), _p(o[1])), "glue")


# ------------------------------------------------------------------------------------------------
# GPU: whole searches against the restated driver on the port
# ------------------------------------------------------------------------------------------------
def _three_searches(shape, port_lib, monkeypatch=None, hbm=False, **flags):
    """Three searches in a row on one driver (the eager run, the capture, a replay), each against the
    restated driver on the CPU port with the same GPU model; legal masks with about 30 % zeros,
    add_noise=True, make_net under autocast.  Returns the loop."""
    import torch

    from joint_driver_fixture import JointOracleSampledMCTS
    from mazero_amd.mcts_sampled import _LOOPS, SampledMCTS
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch

    N, A, K, S, B = shape
    if hbm:
        monkeypatch.setenv("MZ_HBM", "1")
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=K)
    net = make_net(N, A, seed=3, device=dev)
    rs_o, rs_d = np.random.RandomState(11), np.random.RandomState(11)
    oracle, drv = JointOracleSampledMCTS(cfg, rs_o, port_lib), SampledMCTS(cfg, rs_d, **flags)
    tree = None
    for step in range(3):
        out, legal = make_root_batch(net, B, 64, seed=4 + step, device=dev, legal_zero_frac=0.3)
        exp = oracle.batch_search_joint(net, out, legal, dev, True, 1.0)
        if step == 1:  # the device-output form once, through to_host
            dout = drv.batch_search_joint_device(net, out, legal, dev, True, 1.0)
            got, tree = dout.to_host(), dout.tree
            assert dout.marginal_visit_count.shape == (B, N, A)
        else:
            got = drv.batch_search_joint(net, out, legal, dev, True, 1.0)
        _compare(got, exp, f"search {step}: ")
        assert _rng_state_equal(rs_o, rs_d), f"np_random after search {step}"
    loops = [v for k, v in _LOOPS.items() if v.model_ref() is net and v.joint_mode]
    assert len(loops) == 1 and loops[0].runs == 3 and loops[0].tb is tree
    # recorded and replayed; mz_graph_census found no memset node
    assert loops[0].graph not in (None, False) and loops[0].graph_nodes[0] > 0 and loops[0].graph_nodes[1] == 0
    assert tree.agent_num == N
    return loops[0]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_joint_search_matches_restated_driver(shape, port_lib):
    loop = _three_searches(shape, port_lib)
    N, K = shape[0], shape[2]
    assert loop.tb.fused_kernel().startswith("k_step<0,joint>" if N > 1 else "k_")
    assert (loop.pool is None) == (K == 1)  # K = 1: the chain shortcut, no pool and no gather


@pytest.mark.gpu
def test_joint_search_matches_restated_driver_hbm(port_lib, monkeypatch):
    """The first shape once more with the trees in the arena (MZ_HBM=1: k_hbm<joint>)."""
    from mazero_amd.mcts_sampled import release

    release()  # (a cached handle of this geometry was created without the flag)
    try:
        loop = _three_searches(SHAPES[0], port_lib, monkeypatch, hbm=True)
        assert loop.tb.fused_kernel() == "k_hbm<joint>"
    finally:
        release()


@pytest.mark.gpu
def test_joint_search_fused_transforms(port_lib):
    """fused_transforms=True gives the same joint search as the default (and so does wide_supports,
    which only changes supports past 64 elements)."""
    _three_searches(SHAPES[0], port_lib, fused_transforms=True, wide_supports=True)


@pytest.mark.gpu
def test_joint_search_host_root_path(port_lib):
    """device_root=False: the root preprocessing in numpy on the host (root_inputs with every agent's
    rows) feeds the same loop; the same search."""
    loop = _three_searches(SHAPES[1], port_lib, device_root=False)
    assert loop.root_mode is None


@pytest.mark.gpu
def test_joint_search_root_shard(port_lib):
    """root_shard composes: a rank that searches roots [3, 8) of 11 draws the whole batch's (11, N)
    Dirichlet rows and keeps its own, seeds tree i as root 3 + i, and so equals the restated driver
    with the same shard on the port; its generator ends where the unsharded search's does."""
    import torch

    from joint_driver_fixture import JointOracleSampledMCTS
    from mazero_amd.mcts_sampled import SampledMCTS, skip_search_draws
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch

    N, A, K, S, B = 3, 9, 5, 12, 5
    shard = (3, 8, 11)
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=K)
    net = make_net(N, A, seed=3, device=dev)
    rs_o, rs_d, rs_w = (np.random.RandomState(13) for _ in range(3))
    oracle = JointOracleSampledMCTS(cfg, rs_o, port_lib, root_shard=shard)
    drv = SampledMCTS(cfg, rs_d, root_shard=shard)
    for step in range(2):
        out, legal = make_root_batch(net, B, 64, seed=40 + step, device=dev, legal_zero_frac=0.3)
        exp = oracle.batch_search_joint(net, out, legal, dev, True, 1.0)
        got = drv.batch_search_joint(net, out, legal, dev, True, 1.0)
        _compare(got, exp, f"search {step}: ")
        skip_search_draws(cfg, rs_w, shard[2], N)  # what the whole batch's search draws
        assert _rng_state_equal(rs_o, rs_d) and _rng_state_equal(rs_w, rs_d)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 5])
def test_joint_search_of_one_agent_is_batch_search(K):
    """N = 1: batch_search_joint equals batch_search(model, out, 0, None, 1, ...) on the same inputs,
    bitwise, np_random included; it runs the one-agent trees' kernels on a loop of its own."""
    import torch

    from mazero_amd.mcts_sampled import _LOOPS, SampledMCTS
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch

    A, S, B = 9, 20, 8
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=K)
    net = make_net(1, A, seed=5, device=dev)
    rs_a, rs_j = np.random.RandomState(2), np.random.RandomState(2)
    agent, joint = SampledMCTS(cfg, rs_a), SampledMCTS(cfg, rs_j)
    for step in range(3):
        out, legal = make_root_batch(net, B, 64, seed=20 + step, device=dev, legal_zero_frac=0.3)
        exp = agent.batch_search(net, out, 0, None, 1, legal, dev, True, 1.0)
        got = joint.batch_search_joint(net, out, legal, dev, True, 1.0)
        _compare(got, exp._asdict(), f"search {step}: ")
        assert _rng_state_equal(rs_a, rs_j)
    loops = [v for v in _LOOPS.values() if v.model_ref() is net]
    assert sorted(v.joint_mode for v in loops) == [False, True]
    tb = [v for v in loops if v.joint_mode][0].tb
    assert tb.agent_num == 1 and tb.prepare_kernel() == ("k_prepare1" if K == 1 else "k_prepare")
    assert "joint" not in tb.fused_kernel() and (K > 1 or tb.fused_kernel().startswith("k_chain"))


def _host_lists(out):
    h = out.to_host()
    return h.sampled_actions, h.sampled_visit_count


@pytest.mark.gpu
def test_select_joint_actions(port_lib):
    """consume.select_joint_actions on a real DeviceSearchOutput and on a hand-made batch with a root
    of zero visits and a root without children, deterministic and with given uniforms, against the host
    restatement: actions and positions equal.  The entropy is mz_select_actions' own, bit for bit (that
    kernel's device log is pinned to scipy's within 1e-12 by tests/test_consume.py; this issue sets no
    tolerance, so the comparison here is with the kernel whose arithmetic the joint consumer shares)."""
    import torch

    from joint_driver_fixture import select_joint_actions_host
    from mazero_amd.consume import select_actions, select_joint_actions
    from mazero_amd.cytree import Tree_batch
    from mazero_amd.mcts_sampled import DeviceSearchOutput, SampledMCTS
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch

    N, A, K, S, B = SHAPES[0]
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=K)
    net = make_net(N, A, seed=3, device=dev)
    out, legal = make_root_batch(net, B, 64, seed=4, device=dev, legal_zero_frac=0.3)
    real = SampledMCTS(cfg, np.random.RandomState(1)).batch_search_joint_device(net, out, legal, dev, True, 1.0)

    W = 4  # hand-made: root 1 has no visits, root 3 no children, root 0 a tie, root 4 a full row
    deg = np.array([3, 2, 1, 0, 4], np.int32)
    vis = np.array([[2, 5, 5, 9], [0, 0, 7, 7], [4, 1, 1, 1], [3, 3, 3, 3], [1, 2, 3, 4]], np.int32)
    act = np.random.default_rng(0).integers(0, A, size=(5, W * N)).astype(np.int32)
    tb = Tree_batch(5, N, A, K, S, 0.01, 0, 0.75, 0.8)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    made = DeviceSearchOutput(None, torch.zeros(5, N, A, dtype=torch.int32, device=dev), None, t(deg),
                              {"visit_count": t(vis), "actions": t(act)}, tb)

    for what, dout in (("search", real), ("hand-made", made)):
        sa, sv = _host_lists(dout) if dout is real else (
            [act[i].reshape(W, N)[:deg[i]] for i in range(5)], [vis[i, :deg[i]] for i in range(5)])
        n = len(sa)
        u = np.random.default_rng(9).random(n)
        for temperature, deterministic in ((1.0, True), (1.0, False), (0.5, False), (0.25, False)):
            ea, ep, _ = select_joint_actions_host(sa, sv, temperature, deterministic, None if deterministic else u)
            ga, gp, ge = select_joint_actions(dout, temperature, deterministic, None if deterministic else t(u))
            where = f"{what} T={temperature} deterministic={deterministic}"
            assert ga.shape == (n, N) and ga.dtype == torch.int32
            _same(gp.cpu().numpy(), ep, where + " pos")
            _same(ga.cpu().numpy(), ea, where + " actions")
            p1, a1, e1 = select_actions(dout, None if deterministic else t(u), temperature, deterministic)
            _same(gp.cpu().numpy(), p1.cpu().numpy(), where + " pos vs select_actions")
            _same(ga.cpu().numpy()[:, 0], a1.cpu().numpy(), where + " agent 0 vs select_actions")
            _same(ge.cpu().numpy(), e1.cpu().numpy(), where + " entropy vs select_actions")
    ga, gp, ge = select_joint_actions(made)
    assert (ga.cpu().numpy()[[1, 3]] == -1).all() and (gp.cpu().numpy()[[1, 3]] == -1).all()
    assert np.isnan(ge.cpu().numpy()[[1, 3]]).all()


# ------------------------------------------------------------------------------------------------
# GPU: refusals
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("flag", ["root_capacity", "later_action_cache", "wide_actions"])
def test_joint_search_refuses_flag(flag):
    import torch

    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch

    N, A, B = 2, 3, 4
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=4, sampled_action_times=2)
    net = make_net(N, A, seed=1, device=dev)
    out, legal = make_root_batch(net, B, 64, seed=2, device=dev)
    rs = np.random.RandomState(0)
    before = rs.get_state()[1].copy()
    drv = SampledMCTS(cfg, rs, **{flag: 8 if flag == "root_capacity" else True})
    for call in (drv.batch_search_joint, drv.batch_search_joint_device):
        with pytest.raises(ValueError, match=flag):
            call(net, out, legal, dev, True, 1.0)
    assert np.array_equal(rs.get_state()[1], before)  # refused before anything is drawn
    with pytest.raises(NotImplementedError):
        SampledMCTS(cfg, rs).batch_search_joint(net, out, legal, dev, False, 1.0, (None, None))


@pytest.mark.gpu
def test_joint_trees_refused_at_construction():
    """What the handle refuses for N > 1 raises when the tree batch is made, before anything launches:
    A = 65 with N = 2 from Tree_batch (and from SampledMCTS's own constructor), K = 65 from the search."""
    import torch

    from mazero_amd._capi import MZError
    from mazero_amd.cytree import Tree_batch
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch

    with pytest.raises(MZError, match="joint-action trees"):
        Tree_batch(4, 2, 65, 5, 8, 0.01, 0, 0.75, 0.8)
    with pytest.raises(RuntimeError, match="action_space_size 65"):
        SampledMCTS(SearchConfig(action_space_size=65))
    N, A, B = 2, 3, 4
    dev = torch.device("cuda", 0)
    net = make_net(N, A, seed=1, device=dev)
    out, legal = make_root_batch(net, B, 64, seed=2, device=dev)
    cfg = SearchConfig(action_space_size=A, num_simulations=4, sampled_action_times=65)
    with pytest.raises(MZError, match="joint-action trees"):
        SampledMCTS(cfg, np.random.RandomState(0)).batch_search_joint(net, out, legal, dev, True, 1.0)
