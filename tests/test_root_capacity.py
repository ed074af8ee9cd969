"""Active roots of a tree handle (include/mzdriver.h: mz_set_active_roots, mz_get_active_roots),
MZ_MARGINAL_ARGMAX_LEGAL (include/mzconsume.h) and SampledMCTS(..., root_capacity=C): every search of
B <= C roots on the tree handle and the recorded loops of the C-root geometry.

CPU tests pin the opt-in (constructor, config object, worker shards, what is refused) and the ctypes
signatures against the header.  GPU tests check the handle's getters and consumers on n-row buffers
with guard rows, mode 2 against the numpy expression of reanalyze_worker.py:563-570, and whole
searches of varying root counts on one capacity driver against a plain driver, bit for bit.

Everything compared bit for bit runs on `RowwiseNet`, a model that is row-count-invariant by
construction: no matrix product and no reduction, only elementwise arithmetic, indexing of a small
embedding by the action, and slices.  Row i of its outputs therefore does not depend on how many rows
the batch has, which is the condition under which a padded search equals the plain one.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_HEADER = os.path.join(ROOT, "include", "mzdriver.h")
CONSUME_HEADER = os.path.join(ROOT, "include", "mzconsume.h")

HID = 16  # hidden size per agent


class RowwiseNet(torch.nn.Module):
    """The core/model.py surface with row-wise arithmetic only (see the module docstring).  The value and
    reward heads are scalars and the inverse transforms slices, so `fused_transforms` applies to it as
    "identity" (use_vectorization = False)."""

    def __init__(self, num_agents: int, action_space_size: int, seed: int = 0):
        super().__init__()
        assert action_space_size <= HID
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.nn.Parameter(torch.randn(*s, generator=g))  # noqa: E731
        self.num_agents, self.action_space_size = num_agents, action_space_size
        self.rep_w, self.rep_b = r(HID), r(HID)
        self.emb = r(action_space_size, HID)  # indexed by the action
        self.dyn_w = r(HID)
        self.pol_w, self.pol_v = r(action_space_size), r(action_space_size)

    def representation(self, obs):
        return torch.tanh(obs[:, :, :HID] * self.rep_w + self.rep_b).reshape(obs.shape[0], -1)

    def prediction(self, h):
        hs = h.reshape(h.shape[0], self.num_agents, HID)
        A = self.action_space_size
        policy = 3.0 * (hs[:, :, :A] * self.pol_w + hs[:, :, HID - A:] * self.pol_v)
        value = 2.0 * hs[:, 0, 0:1] * hs[:, self.num_agents - 1, 1:2] + hs[:, 0, 2:3]
        return policy.float(), value.float()

    def dynamics(self, h, action):
        hs = h.reshape(h.shape[0], self.num_agents, HID)
        nxt = torch.tanh(hs * self.dyn_w + self.emb[action.long()])
        reward = 0.5 * nxt[:, 0, 3:4] * nxt[:, self.num_agents - 1, 4:5]
        return nxt.reshape(h.shape[0], -1), reward.float()

    def inverse_value_transform(self, x):
        return x[:, :1]

    def inverse_reward_transform(self, x):
        return x[:, :1]

    def initial_inference(self, obs):
        from mazero_amd.nets import NetworkOutput

        h = self.representation(obs)
        policy, value = self.prediction(h)
        return NetworkOutput(h, np.zeros((obs.shape[0], 1), np.float32), value.detach().cpu().numpy(),
                             policy.detach().cpu().numpy())

    def recurrent_inference(self, h, action):
        from mazero_amd.nets import NetworkOutput

        nxt, reward = self.dynamics(h, action)
        policy, value = self.prediction(nxt)
        return NetworkOutput(nxt, self.inverse_reward_transform(reward).detach().cpu().numpy(),
                             self.inverse_value_transform(value).detach().cpu().numpy(),
                             policy.detach().cpu().numpy())


def rowwise_batch(net, B, seed, device, legal_zero_frac=0.2):
    """Synthetic observations -> initial_inference, and a legal mask [B, N, A] with about
    `legal_zero_frac` zeros (at least one legal action per row)."""
    rng = np.random.default_rng(seed)
    obs = torch.from_numpy(rng.standard_normal((B, net.num_agents, HID)).astype(np.float32)).to(device)
    with torch.no_grad():
        out = net.initial_inference(obs)
    legal = (rng.random((B, net.num_agents, net.action_space_size)) >= legal_zero_frac).astype(np.int64)
    legal[..., 0] = np.where(legal.sum(-1) == 0, 1, legal[..., 0])
    return out, legal


def rowwise_config(A, S, K):
    from mazero_amd.nets import SearchConfig

    return SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=K, use_vectorization=False)


# ------------------------------------------------------------------------------------------ CPU
def test_constructor_takes_root_capacity():
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=9)
    assert SampledMCTS(cfg, np.random.RandomState(0), root_capacity=32).root_capacity == 32
    assert SampledMCTS(cfg, np.random.RandomState(0)).root_capacity is None  # off by default


def test_root_capacity_read_from_config():
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=9)
    cfg.root_capacity = 16
    assert SampledMCTS(cfg, np.random.RandomState(0)).root_capacity == 16
    assert SampledMCTS(cfg, np.random.RandomState(0), root_capacity=8).root_capacity == 8  # the argument wins


def test_root_capacity_refusals():
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=9)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="root_capacity"):
            SampledMCTS(cfg, np.random.RandomState(0), root_capacity=bad)
    with pytest.raises(ValueError, match="root_shard"):
        SampledMCTS(cfg, np.random.RandomState(0), root_capacity=8, root_shard=(0, 4, 8))


def test_worker_shards_pass_root_capacity():
    from mazero_amd.nets import SearchConfig
    from mazero_amd.workers import ReanalyzeShard, SelfPlayShard

    cfg = SearchConfig(action_space_size=9)
    sp = SelfPlayShard(None, cfg, 8, 2, seed=0, rank=0, world=1, root_capacity=8)
    m = sp.make_mcts(sp.config, sp.np_random, sp._search_shard())
    assert m.root_capacity == 8 and m.root_shard is None
    ra = ReanalyzeShard(None, cfg, 8, seed=0, rank=0, world=1, root_capacity=12)
    assert ra.make_mcts(ra.config, ra.np_random, ra._search_shard()).root_capacity == 12
    plain = SelfPlayShard(None, cfg, 8, 2, seed=0, rank=1, world=2)
    m = plain.make_mcts(plain.config, plain.np_random, plain._search_shard())
    assert m.root_capacity is None and m.root_shard == (4, 8, 8)  # as before
    sharded = SelfPlayShard(None, cfg, 8, 2, seed=0, rank=1, world=2, root_capacity=8)
    with pytest.raises(ValueError, match="root_shard"):  # refused by the search, with the reason
        sharded.make_mcts(sharded.config, sharded.np_random, sharded._search_shard())


def test_active_refused_on_sharded_ranks():
    from mazero_amd.nets import SearchConfig
    from mazero_amd.workers import SelfPlayShard

    sp = SelfPlayShard(None, SearchConfig(action_space_size=9), 8, 2, seed=0, rank=1, world=2)
    with pytest.raises(NotImplementedError, match="root offset"):
        sp.step(0, None, None, active=[4, 5])


def test_ctypes_signatures_match_header():
    from mazero_amd import _capi

    txt = open(DRIVER_HEADER).read()
    ctype = {"mz_batch *": C.c_void_p, "int": C.c_int, "int *": C.POINTER(C.c_int)}
    want = {"mz_set_active_roots": ["mz_batch *", "int"], "mz_get_active_roots": ["mz_batch *", "int *"]}
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


def test_marginal_mode_constant_matches_header():
    from mazero_amd import _capi

    m = re.search(r"MZ_MARGINAL_ARGMAX_LEGAL\s*=\s*(\d+)", open(CONSUME_HEADER).read())
    assert m and int(m.group(1)) == 2 and _capi.MZ_MARGINAL_ARGMAX_LEGAL == 2
    assert (_capi.MZ_MARGINAL_GIVEN, _capi.MZ_MARGINAL_ARGMAX) == (0, 1)


def test_root_capacity_needs_the_active_root_calls(port_lib):
    """A tree library without mz_set_active_roots is refused at construction, before any search runs."""
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig

    cfg = SearchConfig(action_space_size=9)
    with pytest.raises(RuntimeError, match="mz_set_active_roots"):
        SampledMCTS(cfg, np.random.RandomState(0), lib=port_lib, root_capacity=8)
    assert SampledMCTS(cfg, np.random.RandomState(0), lib=port_lib).root_capacity is None


def test_set_active_roots_needs_the_symbol(port_lib):
    """A library without mz_set_active_roots (the oracle libraries): RuntimeError, active_roots stays
    root_num."""
    from mazero_amd.cytree import Tree_batch

    tb = Tree_batch(4, 1, 3, 1, 2, 0.01, 0, 0.75, 0.8, lib=port_lib)
    assert tb.active_roots == 4
    with pytest.raises(RuntimeError, match="mz_set_active_roots"):
        tb.set_active_roots(2)


# ---------------------------------------------------------------------------------- GPU, the handle
HC, HA, HK, HS = 80, 9, 5, 8  # 80 roots cross the consumers' 64-lane block
ACTIVE_COUNTS = [1, 63, 64, 65, 80]
GUARD_I, GUARD_F = -77, -77.5


@functools.lru_cache(maxsize=None)
def _searched_handle():
    """One synthetic search on an 80-root handle and its full readback (every getter at 80 active roots)."""
    from mazero_amd.cytree import Tree_batch
    from mazero_amd.synthetic import DEFAULTS, make_search_inputs, run_search

    torch.cuda.set_device(0)
    d = DEFAULTS
    inp = make_search_inputs(np.random.default_rng(3), HC, HA, HS, legal_zero_frac=0.2)
    tb = Tree_batch(HC, 1, HA, HK, HS, d["delta_lb"], inp.seed, d["rho"], d["lam"])
    run_search(tb, inp, HK, record=False, per_sim=False)
    return tb, _host_getters(tb, d["discount"])


def _host_getters(tb, disc):
    out = dict(values=tb.get_roots_values(), mv=tb.get_roots_marginal_visit_count(),
               mp=tb.get_roots_marginal_priors())
    from mazero_amd._capi import FIELDS

    for f in FIELDS:
        out[f] = tb._sampled_lists(f, disc)
        out["padded_" + f] = tb.get_roots_sampled_padded(f, disc)
    return out


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", ACTIVE_COUNTS)
def test_getters_return_the_active_rows(n):
    from mazero_amd.synthetic import DEFAULTS

    tb, full = _searched_handle()
    try:
        tb.set_active_roots(n)
        assert tb.active_roots == n
        got = _host_getters(tb, DEFAULTS["discount"])
        for k, v in full.items():
            want = tuple(x[:n] for x in v) if isinstance(v, tuple) else v[:n]
            assert _same(got[k], want), k
            assert len(got[k][0] if isinstance(v, tuple) else got[k]) == n, k
        # per-root calls: tree_id < n
        lib, deg = tb._lib, C.c_int32()
        assert lib.mz_get_num_children_of_root(tb._h, n - 1, C.byref(deg)) == 0
        assert deg.value == len(full["visit_count"][n - 1])
        buf = np.zeros(tb.max_children(), np.int32)
        assert lib.mz_get_root_sampled(tb._h, 1, n - 1, 0.0, buf.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(buf[: deg.value], full["visit_count"][n - 1])
        if n < HC:
            from mazero_amd._capi import MZ_ERR_ARG

            assert lib.mz_get_num_children_of_root(tb._h, n, C.byref(deg)) == MZ_ERR_ARG
            assert lib.mz_get_root_sampled(tb._h, 1, n, 0.0, buf.ctypes.data_as(C.c_void_p)) == MZ_ERR_ARG
    finally:
        tb.set_active_roots(HC)


def _device_readback(tb, rows, disc):
    """mz_get_roots_device (and the per-field device getters) into tensors of rows + 1 rows, the last a
    guard."""
    from mazero_amd._capi import FIELDS, INT_FIELDS

    dev = torch.device("cuda", 0)
    W = tb.max_children()

    def buf(width, integer):
        return torch.full((rows + 1, width), GUARD_I if integer else GUARD_F,
                          dtype=torch.int32 if integer else torch.float32, device=dev)

    o = dict(values=buf(1, False), mv=buf(HA, True), mp=buf(HA, False), deg=buf(1, True))
    sampled = {f: buf(W, f in INT_FIELDS) for f in FIELDS}
    tb.get_roots_device(disc, values=o["values"], marginal_visit_count=o["mv"], marginal_priors=o["mp"],
                        degrees=o["deg"], sampled=sampled)
    single = dict(values=buf(1, False), mv=buf(HA, True), mp=buf(HA, False))
    tb.get_roots_values_device(single["values"])
    tb.get_roots_marginal_device(single["mv"], single["mp"])
    torch.cuda.synchronize()
    o.update({"s_" + f: t for f, t in sampled.items()})
    o.update({"single_" + k: t for k, t in single.items()})
    return {k: t.cpu().numpy() for k, t in o.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("n", ACTIVE_COUNTS)
def test_device_readback_leaves_the_guard_rows(n):
    from mazero_amd.synthetic import DEFAULTS

    tb, _ = _searched_handle()
    disc = DEFAULTS["discount"]
    full = _device_readback(tb, HC, disc)
    try:
        tb.set_active_roots(n)
        got = _device_readback(tb, n, disc)
    finally:
        tb.set_active_roots(HC)
    for k, v in got.items():
        assert _same(v[:n], full[k][:n]), k
        guard = GUARD_I if v.dtype == np.int32 else GUARD_F
        assert (v[n] == guard).all(), f"{k}: guard row written"


@pytest.mark.gpu
def test_active_roots_argument_errors_and_readback_stays_valid():
    from mazero_amd._capi import MZ_ERR_ARG

    tb, full = _searched_handle()
    lib = tb._lib
    for bad in (0, HC + 1, -1):
        assert lib.mz_set_active_roots(tb._h, bad) == MZ_ERR_ARG
        assert tb.active_roots == HC
    with pytest.raises(ValueError):
        tb.set_active_roots(HC + 1)
    assert lib.mz_get_active_roots(tb._h, None) == MZ_ERR_ARG
    tb.set_active_roots(7)
    tb.set_active_roots(HC)
    assert _same(tb.get_roots_values(), full["values"])
    # the Python getters read the count from the library: a raw C call is seen too
    try:
        assert lib.mz_set_active_roots(tb._h, 9) == 0
        assert tb.active_roots == 9 and _same(tb.get_roots_values(), full["values"][:9])
        assert len(tb.get_roots_sampled_visit_count()) == 9
    finally:
        tb.set_active_roots(HC)


@pytest.mark.gpu
def test_expand_backup_readback_keeps_asking_for_every_row():
    """mz_expand_backup_readback with caller buffers writes all root_num rows whatever the active count
    (include/mzdriver.h): with fewer active roots the wrapper must still refuse buffers of only that many
    rows, before anything is launched, while get_roots_device takes them."""
    tb, _ = _searched_handle()
    dev = torch.device("cuda", 0)
    n = 5
    small = dict(values=torch.empty(n, device=dev), degrees=torch.empty(n, dtype=torch.int32, device=dev),
                 marginal_visit_count=torch.empty(n, 1, HA, dtype=torch.int32, device=dev))
    z = torch.zeros(HC, device=dev)
    p = torch.full((HC, HA), 1.0 / HA, device=dev)
    try:
        tb.set_active_roots(n)
        tb.get_roots_device(0.997, **small)  # n rows are what this launch writes
        for key in small:
            with pytest.raises(ValueError, match="the readback writes"):
                tb.expansion_backup_readback_device(HS, 0.997, HK, z, z, p, p, readback_discount=0.997,
                                                    out={key: small[key]})
    finally:
        tb.set_active_roots(HC)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_consumers_refuse_an_output_of_an_earlier_root_count():
    """On a capacity handle a DeviceSearchOutput of a 5-root search must not be consumed after a 9-root
    search: the consumers launch one lane per active root.  Refused with ValueError, nothing launched."""
    from mazero_amd.consume import marginal_policy, select_actions
    from mazero_amd.mcts_sampled import SampledMCTS

    dev = torch.device("cuda", 0)
    net = RowwiseNet(SN, SA, seed=3).to(dev).eval()
    drv = SampledMCTS(rowwise_config(SA, SS, 5), np.random.RandomState(1), root_capacity=32)
    outs = {}
    for B in (5, 9):
        out, legal = rowwise_batch(net, B, 70 + B, dev)
        outs[B] = drv.batch_search_device(net, out, 0, None, SN, legal, device=dev, add_noise=True)
    assert outs[5].tree is outs[9].tree and outs[9].tree.active_roots == 9
    with pytest.raises(ValueError, match="5 roots.*9 active"):
        select_actions(outs[5], torch.zeros(5, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="5 roots.*9 active"):
        marginal_policy(outs[5], 0, torch.zeros(5, dtype=torch.int32, device=dev),
                        torch.ones(5, dtype=torch.float64, device=dev))
    pos, _, _ = select_actions(outs[9], torch.zeros(9, dtype=torch.float64, device=dev))  # the current one works
    assert pos.shape == (9,)


@pytest.mark.gpu
def test_reseed_keeps_active_roots():
    from mazero_amd.cytree import Tree_batch

    torch.cuda.set_device(0)
    tb = Tree_batch(8, 1, 3, 1, 2, 0.01, 0, 0.75, 0.8)
    assert tb.active_roots == 8
    tb.set_active_roots(3)
    tb.reseed(5)
    assert tb.active_roots == 3


def _consumer_inputs():
    tb, full = _searched_handle()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9)
    vis, deg = full["padded_visit_count"]
    act, _ = full["padded_actions"]
    legal = (rng.random((HC, HA)) > 0.3).astype(np.int32)
    legal[:, 1] = 1
    return dict(tb=tb, dev=dev, deg=deg, vis=vis, act=act, mv=np.ascontiguousarray(full["mv"][:, 0, :]), legal=legal,
                u=rng.random(HC), u_eps=rng.random(HC).astype(np.float32), u_cat=rng.random(HC),
                given=rng.integers(0, HA, HC).astype(np.int32))


def _run_consumers(ci, n):
    """The three consumers on n-row inputs and (n + 1)-row outputs (the last row a guard)."""
    from mazero_amd._capi import MZ_MARGINAL_ARGMAX, MZ_MARGINAL_ARGMAX_LEGAL, MZ_MARGINAL_GIVEN, check

    tb, dev = ci["tb"], ci["dev"]
    lib, h = tb._lib, tb._h
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[:n])).to(dev)  # noqa: E731
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    gi = lambda: torch.full((n + 1,), GUARD_I, dtype=torch.int32, device=dev)  # noqa: E731
    gd = lambda v=GUARD_F: torch.full((n + 1,), v, dtype=torch.float64, device=dev)  # noqa: E731
    deg, vis, act, mv, legal = t(ci["deg"]), t(ci["vis"]), t(ci["act"]), t(ci["mv"]), t(ci["legal"])
    tb._sync_stream()
    out = {}
    pos, a, ent = gi(), gi(), gd()
    check(lib, lib.mz_select_actions(h, p(deg), p(vis), p(act), vis.shape[1], 1.0, 0, p(t(ci["u"])), p(pos), p(a),
                                     p(ent)), "select_actions")
    out.update(sel_pos=pos, sel_act=a, sel_ent=ent)
    eg = gi()
    eg[:n] = t(ci["given"])
    check(lib, lib.mz_eps_greedy(h, p(legal), HA, 0.5, p(t(ci["u_eps"])), p(t(ci["u_cat"])), p(eg)), "eps_greedy")
    out["eps"] = eg
    for mode, name in ((MZ_MARGINAL_GIVEN, "given"), (MZ_MARGINAL_ARGMAX, "argmax"),
                       (MZ_MARGINAL_ARGMAX_LEGAL, "legal")):
        a, prob, ent = gi(), gd(1.0), gd()
        if mode == MZ_MARGINAL_GIVEN:
            a[:n] = t(ci["given"])
        prob[n] = GUARD_F
        check(lib, lib.mz_marginal_policy(h, p(mv), HA, p(legal), HA, mode, p(a), p(prob), p(ent)), "marginal_policy")
        out.update({name + "_act": a, name + "_prob": prob, name + "_ent": ent})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("n", ACTIVE_COUNTS)
def test_consumers_work_on_the_active_rows(n):
    ci = _consumer_inputs()
    tb = ci["tb"]
    full = _run_consumers(ci, HC)
    try:
        tb.set_active_roots(n)
        got = _run_consumers(ci, n)
    finally:
        tb.set_active_roots(HC)
    for k, v in got.items():
        assert _same(v[:n], full[k][:n]), k
        assert v[n] == (GUARD_I if v.dtype == np.int32 else GUARD_F), f"{k}: guard row written"
    # mode 2 leaves prob and entropy alone on every row
    assert (got["legal_prob"][:n] == 1.0).all() and (got["legal_ent"][:n] == GUARD_F).all()


@pytest.mark.gpu
def test_eps_greedy_takes_strided_uniform_rows():
    """consume.eps_greedy with rows of column-major [N, B] uniforms (what numpy's u[:, idx] yields, as
    SelfPlayShard.run slices them to the active environments): the contiguous copies it makes must both
    live until the launch.  Same actions as with contiguous rows."""
    from mazero_amd.consume import eps_greedy
    from mazero_amd.mcts_sampled import DeviceSearchOutput

    ci = _consumer_inputs()
    dev = ci["dev"]
    out = DeviceSearchOutput(None, None, None, None, {}, ci["tb"])
    legal = torch.from_numpy(ci["legal"]).to(dev)
    rng = np.random.default_rng(2)
    ue, uc = rng.random((3, HC)).astype(np.float32), rng.random((3, HC))
    got = []
    for a, b in ((ue, uc), (ue[:, np.arange(HC)], uc[:, np.arange(HC)])):
        assert a.flags["C_CONTIGUOUS"] == (a is ue)
        te, tc = torch.as_tensor(a).to(dev), torch.as_tensor(b).to(dev)
        act = torch.from_numpy(ci["given"]).to(dev)
        eps_greedy(out, act, legal, 0.5, te[1], tc[1])
        got.append(act.cpu().numpy())
    assert (got[0] != ci["given"]).any() and np.array_equal(got[0], got[1])


# ---------------------------------------------------------------------------------- GPU, mode 2
def _mode2_arrays():
    rng = np.random.default_rng(21)
    B, A = HC, HA
    marginal = rng.integers(0, 6, (B, A)).astype(np.int32)
    legal = (rng.random((B, A)) > 0.3).astype(np.int32)
    marginal[0:8] = 0  # visits on illegal actions only
    marginal[0:8, 2] = 5
    legal[0:8, 2] = 0
    legal[0:8, 3] = 1
    legal[8:12] = 0  # no legal action
    marginal[12:20] = 0  # ties: the first maximum wins
    marginal[12:20, [1, 4, 7]] = 3
    legal[12:20] = 1
    legal[16:20, 1] = 0
    marginal[20:24] = 0  # no visits at all
    legal[24, :] = 2  # weights other than 0 / 1 scale the products
    return marginal, legal


def _mode2_numpy(marginal, legal):
    """reanalyze_worker.py:563-570 without the np_random draw: -1 where the reference draws."""
    out = np.empty(marginal.shape[0], np.int32)
    for i in range(marginal.shape[0]):
        masked_visits = marginal[i].astype(np.int64) * legal[i]
        out[i] = np.argmax(masked_visits) if np.sum(masked_visits) > 0 else -1
    return out


@pytest.mark.gpu
def test_marginal_argmax_legal_matches_numpy():
    from mazero_amd._capi import MZ_ERR_ARG, MZ_MARGINAL_ARGMAX, MZ_MARGINAL_ARGMAX_LEGAL, MZ_MARGINAL_GIVEN

    tb, _ = _searched_handle()
    dev = torch.device("cuda", 0)
    lib, h = tb._lib, tb._h
    marginal, legal = _mode2_arrays()
    want = _mode2_numpy(marginal, legal)
    assert (want[:12] == -1).all() and (want[12:16] == 1).all() and (want[16:20] == 4).all() and (want >= 0).any()
    tm, tl = torch.from_numpy(marginal).to(dev), torch.from_numpy(legal).to(dev)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    tb._sync_stream()
    a = torch.full((HC,), GUARD_I, dtype=torch.int32, device=dev)
    assert lib.mz_marginal_policy(h, p(tm), HA, p(tl), HA, MZ_MARGINAL_ARGMAX_LEGAL, p(a), None, None) == 0  # NULL prob
    np.testing.assert_array_equal(a.cpu().numpy(), want)
    assert lib.mz_marginal_policy(h, p(tm), HA, None, HA, MZ_MARGINAL_ARGMAX_LEGAL, p(a), None, None) == MZ_ERR_ARG
    assert lib.mz_marginal_policy(h, p(tm), HA, p(tl), HA, 3, p(a), None, None) == MZ_ERR_ARG
    # modes 0 and 1 on the same arrays: what the header says of them
    msum = marginal.sum(1).astype(np.int64)
    given = np.random.default_rng(4).integers(0, HA, HC).astype(np.int32)
    ta = torch.from_numpy(given).to(dev)
    prob = torch.ones(HC, dtype=torch.float64, device=dev)
    ent = torch.full((HC,), GUARD_F, dtype=torch.float64, device=dev)
    assert lib.mz_marginal_policy(h, p(tm), HA, None, 0, MZ_MARGINAL_GIVEN, p(ta), p(prob), p(ent)) == 0
    exp_prob = np.where(msum > 0, marginal[np.arange(HC), given] / np.maximum(msum, 1).astype(np.float64), 1.0 / HA)
    assert _same(prob.cpu().numpy(), exp_prob)
    assert np.array_equal(ta.cpu().numpy(), given)
    dist = marginal / np.maximum(msum, 1)[:, None].astype(np.float64)
    exp_ent = np.where(msum > 0, -np.sum(dist * np.log(dist + 1e-9), axis=1), 0.0)
    np.testing.assert_allclose(ent.cpu().numpy(), exp_ent, rtol=1e-12, atol=1e-15)
    a1 = torch.full((HC,), GUARD_I, dtype=torch.int32, device=dev)
    prob1 = torch.ones(HC, dtype=torch.float64, device=dev)
    assert lib.mz_marginal_policy(h, p(tm), HA, p(tl), HA, MZ_MARGINAL_ARGMAX, p(a1), p(prob1), None) == 0
    exp_a1 = np.where(msum > 0, np.argmax(marginal.astype(np.int64) * legal, axis=1), -1)
    np.testing.assert_array_equal(a1.cpu().numpy(), exp_a1)
    exp_p1 = np.where(msum > 0, marginal[np.arange(HC), np.maximum(exp_a1, 0)] / np.maximum(msum, 1).astype(np.float64),
                      1.0)
    assert _same(prob1.cpu().numpy(), exp_p1)
    assert lib.mz_marginal_policy(h, p(tm), HA, p(tl), HA, MZ_MARGINAL_ARGMAX, p(a1), None, None) == MZ_ERR_ARG


# ---------------------------------------------------------------------------------- GPU, searches
SN, SA, SS = 3, 9, 8
COUNTS = [32, 5, 31, 1, 5, 32]


def _loops_of(net):
    from mazero_amd.mcts_sampled import _LOOPS

    return [v for v in _LOOPS.values() if v.model_ref() is net]


def _trees_of(loops):
    return {id(lp.tb) for lp in loops}


def _assert_same_outputs(a, b, where):
    for name in a._fields:
        assert _same(getattr(a, name), getattr(b, name)), f"{where}: {name} differs"


def _capacity_and_plain(K, cur, cache, capacity, counts, seed=11, fused=None):
    """The root counts `counts`, in that order, on one capacity driver and on a plain driver from the same
    generator seed, each with its own copy of the net (a loop's key carries the model).  Any warning is an
    error.  Returns (outputs, the capacity net's loops, the graph after each search, the generators)."""
    from mazero_amd.mcts_sampled import SampledMCTS

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, K)
    nets = [RowwiseNet(SN, SA, seed=3).to(dev).eval() for _ in range(2)]
    rs = [np.random.RandomState(seed), np.random.RandomState(seed)]
    kw = dict(later_action_cache=cache, fused_transforms=fused)
    drv = [SampledMCTS(cfg, rs[0], root_capacity=capacity, **kw), SampledMCTS(cfg, rs[1], **kw)]
    outs, graphs = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for step, B in enumerate(counts):
            factor = np.random.RandomState(50 + step).randint(0, SA, (B, SN)).astype(np.int32) if cur else None
            pair = []
            for net, d in zip(nets, drv):
                out, legal = rowwise_batch(net, B, 900 + step, dev)
                pair.append(d.batch_search(net, out, cur, factor, SN, legal, device=dev, add_noise=True))
            outs.append(pair)
            graphs.append([lp.graph for lp in _loops_of(nets[0])])
    return outs, _loops_of(nets[0]), graphs, rs, nets


@pytest.mark.gpu
@pytest.mark.parametrize("cache", [False, True], ids=["default", "later_action_cache"])
@pytest.mark.parametrize("cur", [0, 1])
@pytest.mark.parametrize("K", [1, 5])
def test_capacity_search_is_the_plain_search(K, cur, cache):
    outs, loops, graphs, rs, _ = _capacity_and_plain(K, cur, cache, 32, COUNTS)
    for step, (a, b) in enumerate(outs):
        assert a.value.shape == (COUNTS[step],) and len(a.sampled_actions) == COUNTS[step]
        _assert_same_outputs(a, b, f"search {step} ({COUNTS[step]} roots)")
    assert rs[0].randint(1 << 30) == rs[1].randint(1 << 30)  # the generators end in the same state
    assert len(loops) == 1 and len(_trees_of(loops)) == 1
    lp = loops[0]
    assert lp.B == 32 and lp.tb.root_num == 32 and lp.runs == 6
    assert isinstance(lp.graph, torch.cuda.CUDAGraph)
    assert graphs[0] == [None] and all(g == [lp.graph] for g in graphs[1:])  # recorded once, at the second search


@pytest.mark.gpu
def test_capacity_search_across_a_consumer_block():
    """C = 80, B = 65 (eager, recorded, replayed) with the fused identity transforms."""
    outs, loops, _, rs, _ = _capacity_and_plain(5, 1, False, 80, [65, 80, 65], fused=True)
    for step, (a, b) in enumerate(outs):
        _assert_same_outputs(a, b, f"search {step}")
    assert len(loops) == 1 and loops[0].B == 80 and loops[0].runs == 3 and loops[0].fused == "identity"
    assert rs[0].randint(1 << 30) == rs[1].randint(1 << 30)


@pytest.mark.gpu
def test_capacity_refuses_a_larger_batch():
    from mazero_amd.mcts_sampled import SampledMCTS

    dev = torch.device("cuda", 0)
    net = RowwiseNet(SN, SA, seed=3).to(dev).eval()
    rs = np.random.RandomState(1)
    state = rs.get_state()[1].copy()
    drv = SampledMCTS(rowwise_config(SA, SS, 1), rs, root_capacity=32)
    out, legal = rowwise_batch(net, 33, 1, dev)
    with pytest.raises(ValueError, match=r"33.*32"):
        drv.batch_search(net, out, 0, None, SN, legal, device=dev, add_noise=True)
    assert np.array_equal(rs.get_state()[1], state) and not _loops_of(net)  # refused before anything ran


@pytest.mark.gpu
def test_capacity_selfplay_decisions():
    """batch_search_device + selfplay_decisions with given eps_uniforms: the consumers see B rows."""
    from mazero_amd.consume import selfplay_decisions
    from mazero_amd.mcts_sampled import SampledMCTS

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, 5)
    res = []
    for capacity in (32, None):
        net = RowwiseNet(SN, SA, seed=3).to(dev).eval()
        rs = np.random.RandomState(17)
        drv = SampledMCTS(cfg, rs, root_capacity=capacity)
        steps = []
        for step, B in enumerate([32, 5, 31]):
            out, legal = rowwise_batch(net, B, 300 + step, dev)
            rng = np.random.default_rng(40 + step)
            eps = (rng.random((SN, B)).astype(np.float32), rng.random((SN, B)))
            d = selfplay_decisions(drv, net, out, SN, legal, temperature=1.0, greedy_epsilon=0.25, eps_uniforms=eps,
                                   device=dev)
            steps.append([t.cpu().numpy() for t in (d.actions, d.count_entropy, d.prob_action, d.visit_entropy,
                                                    d.root_value)])
            assert d.actions.shape == (B, SN) and d.outputs[0].degrees.shape == (B,)
        res.append((steps, rs.randint(1 << 30)))
    assert res[0][1] == res[1][1]
    for step, (a, b) in enumerate(zip(res[0][0], res[1][0])):
        assert _same(a, b), f"step {step}"


@pytest.mark.gpu
def test_capacity_search_matches_oracle_driver(port_lib):
    """B = 5 on C = 32 against the oracle driver (numpy + the CPU port) on the 5-root batch."""
    from driver import OracleSampledMCTS
    from mazero_amd.mcts_sampled import SampledMCTS
    from test_driver import _compare_outputs

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, 5)
    net = RowwiseNet(SN, SA, seed=5).to(dev).eval()
    rs_o, rs_d = np.random.RandomState(5), np.random.RandomState(5)
    oracle = OracleSampledMCTS(cfg, rs_o, port_lib)
    drv = SampledMCTS(cfg, rs_d, root_capacity=32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for step in range(3):  # eager, recorded, replayed
            out, legal = rowwise_batch(net, 5, 100 + step, dev)
            exp = oracle.batch_search(net, out, 0, None, SN, legal, device=dev, add_noise=True)
            got = drv.batch_search(net, out, 0, None, SN, legal, device=dev, add_noise=True)
            _compare_outputs(got, exp)
    assert rs_o.randint(1 << 30) == rs_d.randint(1 << 30)


@pytest.mark.gpu
def test_capacity_search_structure_with_a_real_net():
    """MuZeroShapedNet under autocast with fused_transforms, B = 5 on C = 32: its matrix products need
    not be row-count-invariant, so no bit comparison: shapes, visit sums, one loop recorded and replayed."""
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch

    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=SA, num_simulations=SS, sampled_action_times=5)
    net = make_net(SN, SA, seed=2, device=dev)
    drv = SampledMCTS(cfg, np.random.RandomState(2), root_capacity=32, fused_transforms=True)
    for step in range(3):
        out, legal = make_root_batch(net, 5, 64, seed=step, device=dev, legal_zero_frac=0.2)
        o = drv.batch_search(net, out, 0, None, SN, legal, device=dev, add_noise=True)
        assert o.value.shape == (5,) and o.marginal_visit_count.shape == (5, 1, SA)
        assert o.marginal_priors.shape == (5, 1, SA) and np.isfinite(o.value).all()
        assert all(len(getattr(o, f)) == 5 for f in o._fields[3:])
        assert (o.marginal_visit_count.sum(axis=(1, 2)) == SS).all()
        assert all(v.sum() == SS for v in o.sampled_visit_count)
    loops = _loops_of(net)
    assert len(loops) == 1 and loops[0].B == 32 and loops[0].runs == 3
    assert isinstance(loops[0].graph, torch.cuda.CUDAGraph)


# ---------------------------------------------------------------------------------- GPU, the worker
@pytest.mark.gpu
def test_selfplay_shard_with_a_shrinking_active_set():
    """SelfPlayShard(world=1, root_capacity=8).run over an environment whose active set shrinks 8 -> 3:
    each record equals the plain per-step selfplay_decisions on the active rows."""
    from mazero_amd.consume import selfplay_decisions
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.workers import SelfPlayShard

    dev = torch.device("cuda", 0)
    total, steps = 8, 6
    cfg = rowwise_config(SA, SS, 3)
    actives = [np.arange(total)[: total - t] if t % 2 else np.arange(total)[t:] for t in range(steps)]  # 8 .. 3 rows

    def whole_eps(t):
        rng = np.random.default_rng(700 + t)
        return rng.random((SN, total)).astype(np.float32), rng.random((SN, total))

    def rows(t):
        rng = np.random.default_rng(600 + t)
        obs = rng.standard_normal((total, SN, HID)).astype(np.float32)
        legal = (rng.random((total, SN, SA)) > 0.2).astype(np.int64)
        legal[..., 1] = 1
        a = actives[t]
        return torch.from_numpy(obs[a]).to(dev), legal[a], tuple(u[:, a] for u in whole_eps(t))

    def env(t, lo, hi):  # the environment says who is still running
        assert (lo, hi) == (0, total)
        obs, legal, _ = rows(t)
        return obs, legal, (None if len(actives[t]) == total else actives[t])

    net = RowwiseNet(SN, SA, seed=8).to(dev).eval()
    sp = SelfPlayShard(net, cfg, total, SN, seed=23, rank=0, world=1, root_capacity=total, device=dev)
    recs = sp.run(env, steps, eps_uniforms=whole_eps, greedy_epsilon=0.25)

    net2 = RowwiseNet(SN, SA, seed=8).to(dev).eval()
    rs = np.random.RandomState(23)
    for t, rec in enumerate(recs):
        obs, legal, eps = rows(t)
        with torch.no_grad(), torch.autocast("cuda"):  # as _Shard._initial_inference
            out = net2.initial_inference(obs)
        d = selfplay_decisions(SampledMCTS(cfg, rs), net2, out, SN, legal, temperature=1.0, greedy_epsilon=0.25,
                               eps_uniforms=eps, device=dev)
        assert rec.actions.shape == (len(actives[t]), SN)
        assert _same(rec.actions, d.actions.cpu().numpy()) and _same(rec.prob_action, d.prob_action.cpu().numpy())
        assert _same(rec.root_value, d.root_value.cpu().numpy().reshape(-1))
        assert _same(rec.count_entropy, d.count_entropy.cpu().numpy())
        assert _same(rec.visit_entropy, d.visit_entropy.cpu().numpy())
        if len(actives[t]) == total:
            assert rec.active is None
        else:
            assert np.array_equal(rec.active, actives[t])
    loops = _loops_of(net)
    assert len(_trees_of(loops)) == 1 and len(loops) == SN  # one handle, one loop per agent
