"""SampledMCTS.batch_search_many: several independent searches of one agent as one search over the
concatenated roots, on one tree handle with per-segment seeds and one recorded loop (GPU tests need an
MI355X: `pytest -m gpu`).

Entry g of the result must equal, field by field and bit by bit, what the g-th of the consecutive
`batch_search` calls returns, and `np_random` must end in the state those calls leave.  Entries of 5, 1
and 9 roots, three calls (eager, recorded, replayed), K in {1, 3}, agent 0 and agent 1 with factors; the
same under root_capacity=32, under fused_transforms with later_action_cache, and with `draws=` from
`draw_search`; once against the oracle driver on the CPU port; every refusal; and
consume.reanalyze_batch_targets against reanalyze_value_targets followed by reanalyze_policy_targets.

Everything compared bit for bit runs on `RowwiseNet` (tests/test_root_capacity.py): row i of its outputs
does not depend on the batch's row count, the condition under which a merged search equals the separate
ones.
"""
from __future__ import annotations

import warnings

import numpy as np
import pytest

from test_root_capacity import SA, SN, SS, RowwiseNet, _loops_of, _same, _trees_of, rowwise_batch, rowwise_config

torch = pytest.importorskip("torch")

SIZES = [5, 1, 9]


def _state_equal(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


# ------------------------------------------------------------------------------------------ CPU
def test_draw_search_consumes_np_random_as_root_raw():
    """draw_search(B) is the (noise, seed) that root_raw draws for a B-root batch, and leaves the generator
    where root_raw leaves it; root_raw and root_inputs given the pair draw nothing."""
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import NetworkOutput

    cfg = rowwise_config(SA, SS, 1)
    rng = np.random.default_rng(2)
    for B in (1, 5, 9):
        out = NetworkOutput(np.zeros((B, 4), np.float32), np.zeros((B, 1), np.float32),
                            rng.standard_normal((B, 1)).astype(np.float32),
                            rng.standard_normal((B, SN, SA)).astype(np.float32))
        legal = (rng.random((B, SN, SA)) > 0.2).astype(np.int64)
        legal[..., 0] = 1
        rs = [np.random.RandomState(7 + B) for _ in range(3)]
        arrays, mode, eps, seed = SampledMCTS(cfg, rs[0]).root_raw(out, 1, legal, True)
        drv = SampledMCTS(cfg, rs[1])
        noise, seed_d = drv.draw_search(B)
        assert _state_equal(rs[0], rs[1])
        assert seed == seed_d and _same(arrays["noise"], noise.astype(np.float32))
        before = rs[1].get_state()[1].copy()
        arrays_d, mode_d, eps_d, seed_r = drv.root_raw(out, 1, legal, True, draw=(noise, seed_d))
        assert seed_r == seed and mode_d == mode and eps_d == eps
        assert all(_same(arrays[k], arrays_d[k]) for k in arrays)
        host, seed_h = drv.root_inputs(out, 1, legal, True, 1.0, draw=(noise, seed_d))
        want, seed_w = SampledMCTS(cfg, rs[2]).root_inputs(out, 1, legal, True, 1.0)
        assert seed_h == seed_w == seed and all(_same(a, b) for a, b in zip(host, want))
        assert np.array_equal(rs[1].get_state()[1], before)  # nothing drawn
        assert _state_equal(rs[1], rs[2])


def test_many_refuses_a_root_shard():
    from mazero_amd.mcts_sampled import SampledMCTS

    drv = SampledMCTS(rowwise_config(SA, SS, 1), np.random.RandomState(0), root_shard=(0, 4, 8))
    with pytest.raises(ValueError, match="root_shard"):
        drv.batch_search_many(None, [None], 0, [None], SN, [None])


# ------------------------------------------------------------------------------------------ GPU
def _entries(net, step, dev, cur, sizes=SIZES):
    outs, legals, factors = [], [], []
    for g, n in enumerate(sizes):
        out, legal = rowwise_batch(net, n, 1000 + 10 * step + g, dev)
        outs.append(out)
        legals.append(legal)
        factors.append(np.random.RandomState(60 + 10 * step + g).randint(0, SA, (n, SN)).astype(np.int32) if cur else None)
    return outs, legals, factors


def _many_and_separate(K, cur, steps=3, use_draws=False, **kw):
    """`steps` calls of batch_search_many on one driver against the consecutive batch_search calls on
    another, from the same generator seed, each with its own copy of the net.  Any warning is an error."""
    from mazero_amd.mcts_sampled import SampledMCTS

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, K)
    nets = [RowwiseNet(SN, SA, seed=3).to(dev).eval() for _ in range(2)]
    rs = [np.random.RandomState(11), np.random.RandomState(11)]
    many = SampledMCTS(cfg, rs[0], **kw)
    plain = SampledMCTS(cfg, rs[1], **{k: v for k, v in kw.items() if k != "root_capacity"})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for step in range(steps):
            outs, legals, factors = _entries(nets[0], step, dev, cur)
            draws = [many.draw_search(n) for n in SIZES] if use_draws else None
            got = many.batch_search_many(nets[0], outs, cur, factors, SN, legals, device=dev, add_noise=True,
                                         sampled_tau=1.0, draws=draws)
            assert len(got) == len(SIZES)
            outs, legals, factors = _entries(nets[1], step, dev, cur)
            for g, n in enumerate(SIZES):
                want = plain.batch_search(nets[1], outs[g], cur, factors[g], SN, legals[g], device=dev, add_noise=True,
                                          sampled_tau=1.0)
                assert got[g].value.shape == (n,) and len(got[g].sampled_actions) == n
                for name in want._fields:
                    assert _same(getattr(got[g], name), getattr(want, name)), f"call {step} entry {g}: {name}"
            assert _state_equal(rs[0], rs[1]), f"call {step}: np_random"
    return nets[0]


@pytest.mark.gpu
@pytest.mark.parametrize("cur", [0, 1])
@pytest.mark.parametrize("K", [1, 3])
def test_many_is_the_consecutive_searches(K, cur):
    net = _many_and_separate(K, cur)
    loops = _loops_of(net)
    assert len(loops) == 1 and len(_trees_of(loops)) == 1
    lp = loops[0]
    assert lp.B == sum(SIZES) and lp.runs == 3 and isinstance(lp.graph, torch.cuda.CUDAGraph)
    assert lp.tb.seed_segments[0] == [0, 5, 6] and lp.tb.seed_segments[2] == [0, 0, 0]
    assert lp.tb.prepare_kernel() == ("k_prepare1" if K == 1 else "k_prepare")


@pytest.mark.gpu
@pytest.mark.parametrize("cur", [0, 1])
@pytest.mark.parametrize("K", [1, 3])
def test_many_on_a_capacity_loop(K, cur):
    net = _many_and_separate(K, cur, root_capacity=32)
    loops = _loops_of(net)
    assert len(loops) == 1 and loops[0].B == 32 and loops[0].tb.root_num == 32 and loops[0].runs == 3
    assert loops[0].tb.active_roots == sum(SIZES)


@pytest.mark.gpu
@pytest.mark.parametrize("cur", [0, 1])
@pytest.mark.parametrize("K", [1, 3])
def test_many_with_fused_transforms_and_later_action_cache(K, cur):
    net = _many_and_separate(K, cur, fused_transforms=True, later_action_cache=True)
    lp = _loops_of(net)[0]
    assert lp.fused == "identity" and (lp.later is not None) == (cur + 1 < SN)


@pytest.mark.gpu
def test_many_through_the_wide_glue():
    net = _many_and_separate(3, 1, wide_actions=True, root_capacity=16)
    lp = _loops_of(net)[0]
    assert lp.B == 16 and lp.policy_glue.__name__ == "mz_policy_glue_wide"


@pytest.mark.gpu
@pytest.mark.parametrize("cur", [0, 1])
@pytest.mark.parametrize("K", [1, 3])
def test_many_with_given_draws(K, cur):
    _many_and_separate(K, cur, use_draws=True)


@pytest.mark.gpu
def test_given_draws_in_another_grouping():
    """Agent 1 of two batches, merged, with the draws made in the reference's order: batch 0's agent 0 and
    agent 1, then batch 1's agent 0 and agent 1."""
    from mazero_amd.mcts_sampled import SampledMCTS

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, 3)
    nets = [RowwiseNet(SN, SA, seed=3).to(dev).eval() for _ in range(2)]
    rs = [np.random.RandomState(4), np.random.RandomState(4)]
    many, plain = SampledMCTS(cfg, rs[0]), SampledMCTS(cfg, rs[1])
    sizes = [5, 9]
    outs, legals, factors = _entries(nets[0], 0, dev, 1, sizes)
    draws0 = [many.draw_search(n) for n in sizes for _ in range(2)]  # [b0 a0, b0 a1, b1 a0, b1 a1]
    got0 = many.batch_search_many(nets[0], outs, 0, None, SN, legals, device=dev, add_noise=True, draws=draws0[0::2])
    got1 = many.batch_search_many(nets[0], outs, 1, factors, SN, legals, device=dev, add_noise=True, draws=draws0[1::2])
    outs, legals, factors = _entries(nets[1], 0, dev, 1, sizes)
    for g in range(2):
        w0 = plain.batch_search(nets[1], outs[g], 0, None, SN, legals[g], device=dev, add_noise=True)
        w1 = plain.batch_search(nets[1], outs[g], 1, factors[g], SN, legals[g], device=dev, add_noise=True)
        for name in w0._fields:
            assert _same(getattr(got0[g], name), getattr(w0, name)), f"agent 0 batch {g}: {name}"
            assert _same(getattr(got1[g], name), getattr(w1, name)), f"agent 1 batch {g}: {name}"
    assert _state_equal(rs[0], rs[1])


@pytest.mark.gpu
def test_many_matches_oracle_driver(port_lib):
    """One oracle search (numpy + the CPU port) per entry."""
    from driver import OracleSampledMCTS
    from mazero_amd.mcts_sampled import SampledMCTS
    from test_driver import _compare_outputs

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, 3)
    net = RowwiseNet(SN, SA, seed=5).to(dev).eval()
    rs_o, rs_d = np.random.RandomState(5), np.random.RandomState(5)
    oracle = OracleSampledMCTS(cfg, rs_o, port_lib)
    drv = SampledMCTS(cfg, rs_d)
    outs, legals, factors = _entries(net, 0, dev, 1)
    got = drv.batch_search_many(net, outs, 1, factors, SN, legals, device=dev, add_noise=True)
    for g in range(len(SIZES)):
        exp = oracle.batch_search(net, outs[g], 1, factors[g], SN, legals[g], device=dev, add_noise=True)
        _compare_outputs(got[g], exp)
    assert rs_o.randint(1 << 30) == rs_d.randint(1 << 30)


@pytest.mark.gpu
def test_plain_search_after_a_merged_one_on_the_same_handle():
    """A 15-root batch_search shares the handle of the merged 5 + 1 + 9: the segments go, its loop is its
    own, and the device slices of the merged output are the entries."""
    from mazero_amd.mcts_sampled import SampledMCTS, slice_search_output

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, 1)
    nets = [RowwiseNet(SN, SA, seed=3).to(dev).eval() for _ in range(2)]
    rs = [np.random.RandomState(9), np.random.RandomState(9)]
    drv, plain = SampledMCTS(cfg, rs[0]), SampledMCTS(cfg, rs[1])
    outs, legals, _ = _entries(nets[0], 0, dev, 0)
    whole, bounds = drv.batch_search_many_device(nets[0], outs, 0, None, SN, legals, device=dev, add_noise=True)
    assert bounds == [0, 5, 6, 15] and whole.value.shape == (15,)
    parts = [slice_search_output(whole, lo, hi).to_host() for lo, hi in zip(bounds[:-1], bounds[1:])]
    tb = _loops_of(nets[0])[0].tb
    assert tb.seed_segments[0] == [0, 5, 6]
    big, legal = rowwise_batch(nets[0], 15, 77, dev)
    got = drv.batch_search(nets[0], big, 0, None, SN, legal, device=dev, add_noise=True)
    assert tb.seed_segments == ([], [], []) and len(_loops_of(nets[0])) == 2 and len(_trees_of(_loops_of(nets[0]))) == 1
    outs, legals, _ = _entries(nets[1], 0, dev, 0)
    for g in range(3):
        want = plain.batch_search(nets[1], outs[g], 0, None, SN, legals[g], device=dev, add_noise=True)
        for name in want._fields:
            assert _same(getattr(parts[g], name), getattr(want, name)), f"entry {g}: {name}"
    big, legal = rowwise_batch(nets[1], 15, 77, dev)
    want = plain.batch_search(nets[1], big, 0, None, SN, legal, device=dev, add_noise=True)
    for name in want._fields:
        assert _same(getattr(got, name), getattr(want, name)), name


@pytest.mark.gpu
def test_many_refusals():
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import NetworkOutput

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, 1)
    net = RowwiseNet(SN, SA, seed=3).to(dev).eval()
    rs = np.random.RandomState(1)
    state = rs.get_state()[1].copy()
    outs, legals, factors = _entries(net, 0, dev, 1)
    kw = dict(device=dev)

    def refused(drv, match, *a, **k):
        with pytest.raises(ValueError, match=match):
            drv.batch_search_many(net, *a, **kw, **k)
        assert np.array_equal(rs.get_state()[1], state) and not _loops_of(net)  # before anything ran

    drv = SampledMCTS(cfg, rs)
    refused(drv, "current_agent_idx", outs, [0, 1, 0], factors, SN, legals, add_noise=True)
    refused(drv, "add_noise", outs, 0, None, SN, legals, add_noise=[True, False, True])
    refused(drv, "sampled_tau", outs, 0, None, SN, legals, add_noise=True, sampled_tau=[1.0, 1.0, 0.5])
    half = NetworkOutput(outs[1].hidden_state, outs[1].reward, outs[1].value, outs[1].policy_logits.astype(np.float16))
    refused(drv, "dtype", [outs[0], half, outs[2]], 0, None, SN, legals, add_noise=True)
    joint = NetworkOutput(outs[1].hidden_state, outs[1].reward, outs[1].value, outs[1].policy_logits[:, 0, :])
    refused(drv, "joint", [outs[0], joint, outs[2]], 0, None, SN, legals, add_noise=True)
    refused(SampledMCTS(cfg, rs, root_shard=(0, 15, 15)), "root_shard", outs, 0, None, SN, legals, add_noise=True)
    refused(SampledMCTS(cfg, rs, root_capacity=14), r"15.*14", outs, 0, None, SN, legals, add_noise=True)
    refused(drv, "factor", outs, 1, [factors[0], None, factors[2]], SN, legals, add_noise=True)


@pytest.mark.gpu
def test_shard_batch_targets_are_the_two_calls():
    """ReanalyzeShard.batch_targets on a single rank against value_targets followed by targets; a sharded
    rank is refused before anything runs."""
    from mazero_amd.workers import ReanalyzeShard

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, 3)
    G, U, TD = 2, 2, 5
    Bv = Bp = G * (U + 1)  # (a shard's two calls share its total_roots)
    nets = [RowwiseNet(SN, SA, seed=3).to(dev).eval() for _ in range(2)]
    shards = [ReanalyzeShard(net, cfg, Bv, seed=31, rank=0, world=1, device=dev) for net in nets]
    rng = np.random.default_rng(9)
    tl = rng.integers(2, 9, size=G)
    tv = dict(rewards=[rng.standard_normal(n + 1) for n in tl], pos=np.array([rng.integers(0, t) for t in tl]),
              traj_len=tl, td_steps=rng.integers(1, TD + 1, size=G), num_unroll_steps=U, td_max=TD)
    for step in range(2):
        vobs = torch.from_numpy(rng.standard_normal((Bv, SN, 16)).astype(np.float32)).to(dev)
        pobs = torch.from_numpy(rng.standard_normal((Bp, SN, 16)).astype(np.float32)).to(dev)
        vlegal, plegal = (np.ones((n, SN, SA), np.int64) for n in (Bv, Bp))
        plegal[:, :, 2] = 0
        mask = rng.integers(0, 2, size=Bp)
        got = shards[0].batch_targets(vobs, vlegal, pobs, plegal, mask, **tv)
        want = shards[1].value_targets(vobs, vlegal, **tv)
        want.update(shards[1].targets(pobs, plegal, mask))
        assert set(got) == set(want)
        for k in want:
            assert _same(got[k], want[k]), f"call {step}: {k}"
        assert _state_equal(shards[0].np_random, shards[1].np_random), f"call {step}"
    sharded = ReanalyzeShard(nets[0], cfg, Bv, seed=31, rank=1, world=2, device=dev)
    with pytest.raises(ValueError, match="root shards"):
        sharded.batch_targets(vobs, vlegal, pobs, plegal, mask, **tv)


@pytest.mark.gpu
def test_reanalyze_batch_targets_are_the_two_calls():
    """All nine outputs and the generator state, against reanalyze_value_targets then
    reanalyze_policy_targets; twice, so that the merged loop also replays."""
    from mazero_amd.consume import reanalyze_batch_targets, reanalyze_policy_targets, reanalyze_value_targets
    from mazero_amd.mcts_sampled import SampledMCTS

    dev = torch.device("cuda", 0)
    cfg = rowwise_config(SA, SS, 3)
    G, U, TD, disc = 2, 2, 5, 0.997
    Bv, Bp = G * (U + 1), 5
    nets = [RowwiseNet(SN, SA, seed=3).to(dev).eval() for _ in range(2)]
    rs = [np.random.RandomState(21), np.random.RandomState(21)]
    merged, plain = SampledMCTS(cfg, rs[0]), SampledMCTS(cfg, rs[1])
    rng = np.random.default_rng(8)
    tl = rng.integers(2, 9, size=G)
    tv = dict(rewards=[rng.standard_normal(n + 1) for n in tl], pos=np.array([rng.integers(0, t) for t in tl]),
              traj_len=tl, td_steps=rng.integers(1, TD + 1, size=G), discount=disc, num_unroll_steps=U, td_max=TD)
    mask = rng.integers(0, 2, size=Bp)
    for step in range(3):
        res = []
        for net, drv in zip(nets, (merged, plain)):
            vout, vlegal = rowwise_batch(net, Bv, 500 + step, dev)
            pout, plegal = rowwise_batch(net, Bp, 600 + step, dev)
            if drv is merged:
                r, v, pol = reanalyze_batch_targets(drv, net, vout, vlegal, pout, plegal, mask, device=dev, **tv)
            else:
                r, v = reanalyze_value_targets(drv, net, vout, vlegal, device=dev, **tv)
                pol = reanalyze_policy_targets(drv, net, pout, plegal, mask, dev)
            res.append([r, v, *pol])
        assert len(res[0]) == 9
        for i, (a, b) in enumerate(zip(*res)):
            a, b = (torch.as_tensor(x).cpu().numpy() for x in (a, b))
            assert _same(a, b), f"call {step}: output {i}"
        assert _state_equal(rs[0], rs[1]), f"call {step}"
