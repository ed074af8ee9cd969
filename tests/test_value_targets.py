"""The reanalyze batch's value, reward and advantage targets on the device (mazero_amd.consume:
reanalyze_value_targets, value_targets_non_re, normalize_advantage; include/mzconsume.h) against
core/reanalyze_worker.py:51-210 (`_prepare_reward_value_re`, `_prepare_reward_value_non_re`) and
:466-473 (step (6) of `make_batch`).

CPU tests pin what the kernels rely on:
- the pairwise-sum plan (mz_pairwise_plan), evaluated in numpy float64, is `np.sum` bit for bit;
- the advantage restatement by that plan is numpy's own nanmean / nanstd arithmetic;
- the per-row restatement of the value targets, on numpy scalars (numpy decides every dtype),
  reproduces tests/golden/reanalyze_values.npz, which scripts/gen_reanalyze_golden.py recorded
  from the reference's own two methods.
GPU tests compare the kernels bit for bit with the restatements and the fixture.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN

PLAN_SIZES = list(range(1, 1101)) + [1536, 1537, 4096, 65536]
ADV_SIZES = [1, 7, 8, 9, 128, 129, 136, 1536, 1537]
DTYPES = {"64": np.float64, "32": np.float32}


@pytest.fixture(scope="module")
def product_lib():
    from mazero_amd._lib import load

    return load()  # (loads without a GPU; mz_pairwise_plan makes no device call)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "reanalyze_values.npz")))


# ------------------------------------------------------------------------------------------------
# restatements
# ------------------------------------------------------------------------------------------------
def plan_sum(starts, ops, a):
    """The plan's arithmetic in numpy float64 scalars (what k_normalize_advantage evaluates)."""
    a = np.asarray(a, np.float64)
    leaves = []
    for s, e in zip(starts[:-1], starts[1:]):
        x = a[s:e]
        n = e - s
        if n < 8:
            res = np.float64(0.0)
            for v in x:
                res = res + v
        else:
            body = n - n % 8
            r = x[:8].copy()
            for k in range(8, body, 8):
                r = r + x[k:k + 8]  # eight independent accumulators
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
            for v in x[body:]:
                res = res + v
        leaves.append(res)
    stack, nb = [], 0
    for o in ops:
        if o == 0:
            stack.append(leaves[nb])
            nb += 1
        else:
            hi = stack.pop()
            stack[-1] = stack[-1] + hi
    assert len(stack) == 1 and nb == len(leaves)
    return np.float64(0.0) + stack[0]


def advantage_restated(q, pred, mask, plan):
    """Step (6) of make_batch as the kernel evaluates it (include/mzconsume.h)."""
    starts, ops = plan
    adv = q.astype(np.float64) - pred.astype(np.float64)
    valid = mask.astype(bool) & ~np.isnan(adv)
    cnt = np.float64(valid.sum())
    with np.errstate(all="ignore"):
        mean = plan_sum(starts, ops, np.where(valid, adv, 0.0)) / cnt
        d = np.where(valid, adv - mean, 0.0)
        std = np.sqrt(plan_sum(starts, ops, d * d) / cnt)
        out = np.where(mask.astype(bool), (adv - mean) / (std + 1e-5), 0.0)
    return out, mean, std


def advantage_numpy(q, pred, mask):
    """reanalyze_worker.py:466-473 with the arrays' shapes and dtypes of make_batch ([n, C = 1];
    the float32 targets are concatenated onto float64 empties, :432-459)."""
    qv = np.concatenate([np.empty((0, 1)), q.reshape(-1, 1)])
    pv = np.concatenate([np.empty((0, 1)), pred.reshape(-1, 1)])
    masks = np.concatenate([np.empty((0, 1), dtype=np.bool_), mask.reshape(-1, 1).astype(np.bool_)])
    adv = qv - pv
    adv_copy = np.array(adv)
    adv_copy[~masks] = np.nan
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        adv_mean = np.nanmean(adv_copy)
        adv_std = np.nanstd(adv_copy)
        adv = (adv - adv_mean) / (adv_std + 1e-5)
    adv[~masks] = 0.
    return adv.reshape(-1), adv_mean, adv_std


def adv_case(n, seed, kind="random"):
    rng = np.random.default_rng(seed)
    q = (3.0 * rng.standard_normal(n)).astype(np.float32)
    pred = (3.0 * rng.standard_normal(n)).astype(np.float32)
    mask = rng.random(n) < 0.8
    if kind == "all_masked":
        mask[:] = False
    elif kind == "single":
        mask[:] = False
        mask[n // 2] = True
    elif kind == "nan_masked":
        mask[n // 3] = False
        q[n // 3] = np.nan
    return q, pred, mask


def rows_re(value, td_pow, td, pos, traj_len, rewards, U, discount):
    """reanalyze_worker.py:137-157 row by row on numpy scalars taken from the arrays."""
    out_r, out_v = [], []
    j = 0
    for g in range(len(pos)):
        for current in range(pos[g], pos[g] + U + 1):
            boot = current + int(td[g])
            v = value[j] * td_pow[j]               # np.float32 * np.float64
            v = v * np.int64(boot < traj_len[g])   # the value mask, a list of Python ints
            for i, reward in enumerate(rewards[g][current:boot]):
                v += reward * discount ** i
            inside = current < traj_len[g]
            out_v.append(v if inside else 0.0)
            out_r.append(rewards[g][current] if inside else 0.0)
            j += 1
    return np.asarray(out_r).reshape(len(pos), U + 1), np.asarray(out_v).reshape(len(pos), U + 1)


def rows_non_re(stored, td, pos, traj_len, rewards, U, discount):
    """reanalyze_worker.py:186-204 row by row on numpy scalars taken from the arrays."""
    out_r, out_v = [], []
    for g in range(len(pos)):
        for current in range(pos[g], pos[g] + U + 1):
            if current < traj_len[g]:
                boot = current + td
                v = stored[g][boot] if boot < traj_len[g] else 0
                for i, reward in enumerate(rewards[g][current:boot]):
                    v += reward * discount ** i
                out_v.append(v)
                out_r.append(rewards[g][current])
            else:
                out_v.append(0.)
                out_r.append(0.)
    return np.asarray(out_r).reshape(len(pos), U + 1), np.asarray(out_v).reshape(len(pos), U + 1)


def golden_games(z, rdt, sdt):
    rewards = [z["rewards"][g, : z["reward_len"][g]].astype(rdt) for g in range(len(z["pos"]))]
    stored = [z["stored"][g, : z["traj_len"][g]].astype(sdt) for g in range(len(z["pos"]))]
    return rewards, stored


def golden_td_pow(z):
    U = int(z["cfg"][1])
    td_steps_lst = [np.intc(t) for t in np.repeat(z["td_steps"], U + 1)]
    return np.power(float(z["discount"]), td_steps_lst)


def same_bits(got, exp, what=""):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype == np.float64, what
    bad = np.argwhere(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, f"{what}: {len(bad)} differ, first {bad[:3].tolist()}: {got[tuple(bad[0])]!r} != {exp[tuple(bad[0])]!r}"


def same_stats(got, exp, what=""):
    """Mean and std bit for bit; a NaN (nothing valid) equals any NaN: its sign is the host's 0/0."""
    for g, e in zip(np.asarray(got, np.float64).reshape(-1), np.asarray(exp, np.float64).reshape(-1)):
        assert (np.isnan(g) and np.isnan(e)) or g.tobytes() == e.tobytes(), (what, got, exp)


# ------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------
def test_pairwise_plan_is_numpy_sum(product_lib):
    from mazero_amd.consume import pairwise_plan

    rng = np.random.default_rng(0)
    for n in PLAN_SIZES:
        starts, ops = pairwise_plan(n, product_lib)
        lens = np.diff(starts)
        assert starts[0] == 0 and starts[-1] == n and (lens >= 1).all() and (lens <= 128).all(), n
        assert (starts[:-1] % 8 == 0).all(), n
        a = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, size=n)
        want = np.sum(a.reshape(n, 1))
        got = plan_sum(starts, ops, a)
        assert got.tobytes() == np.float64(want).tobytes(), (n, got, want)


def test_pairwise_plan_refuses_sizes_outside_the_range(product_lib):
    from mazero_amd._capi import MZ_ERR_ARG, MZ_ERR_UNSUPPORTED

    k = C.c_int32()
    s, o = (C.c_int32 * 1025)(), (C.c_int32 * 2048)()
    for bad in (0, -3, 65537):
        assert product_lib.mz_pairwise_plan(bad, s, o, 1024, C.byref(k), C.byref(k)) == MZ_ERR_UNSUPPORTED
    assert product_lib.mz_pairwise_plan(4096, s, o, 8, C.byref(k), C.byref(k)) == MZ_ERR_ARG  # 32 leaves
    assert product_lib.mz_pairwise_plan(4096, None, o, 1024, C.byref(k), C.byref(k)) == MZ_ERR_ARG


@pytest.mark.parametrize("kind", ["random", "all_masked", "single", "nan_masked"])
def test_advantage_restatement_is_numpy(kind, product_lib):
    from mazero_amd.consume import pairwise_plan

    for n in ADV_SIZES + [600, 3000, 4096, 20000]:  # (above 8192 numpy sums chunk after chunk)
        if kind == "nan_masked" and n < 3:
            continue
        q, pred, mask = adv_case(n, 100 + n, kind)
        got, gm, gs = advantage_restated(q, pred, mask, pairwise_plan(n, product_lib))
        want, wm, ws = advantage_numpy(q, pred, mask)
        same_bits(got, want, f"{kind} n={n}")
        same_stats([gm, gs], [wm, ws], f"{kind} n={n}")
        if kind == "all_masked":
            assert np.isnan(gm) and np.isnan(gs) and not got.any()
        if kind == "single":
            assert gs == 0.0 and not got.any()


def test_row_restatement_reproduces_the_reference_fixture(golden):
    z = golden
    G, U, TD = (int(x) for x in z["cfg"][:3])
    disc = float(z["discount"])
    assert z["td_steps"].tolist() == [1, 3, 5, 5] and (G, U, TD) == (4, 5, 5)
    td_pow = golden_td_pow(z)
    for rk, rdt in DTYPES.items():
        rewards, _ = golden_games(z, rdt, np.float64)
        for which in ("root", "pred"):
            value = z["search_value"] if which == "root" else z["pred_value"]
            r, v = rows_re(value, td_pow, z["td_steps"], z["pos"], z["traj_len"], rewards, U, disc)
            same_bits(r, z[f"re_{which}_r{rk}_rewards"], f"re {which} r{rk} rewards")
            same_bits(v, z[f"re_{which}_r{rk}_values"], f"re {which} r{rk} values")
        for sk, sdt in DTYPES.items():
            rewards, stored = golden_games(z, rdt, sdt)
            r, v = rows_non_re(stored, TD, z["pos"], z["traj_len"], rewards, U, disc)
            same_bits(r, z[f"nonre_r{rk}_s{sk}_rewards"], f"non-re r{rk} s{sk} rewards")
            same_bits(v, z[f"nonre_r{rk}_s{sk}_values"], f"non-re r{rk} s{sk} values")
    # the float32 rewards change the targets: the dtype rules are exercised, not vacuous
    assert not np.array_equal(z["re_root_r32_values"], z["re_root_r64_values"])
    assert not np.array_equal(z["nonre_r32_s32_values"], z["nonre_r32_s64_values"])


def test_fixture_covers_the_trajectory_cases(golden):
    z = golden
    U = int(z["cfg"][1])
    pos, tl, rl, td = z["pos"], z["traj_len"], z["reward_len"], z["td_steps"]
    assert pos[0] + U + td[0] < tl[0]                          # entirely inside
    assert pos[1] < tl[1] <= pos[1] + U                        # ends inside the unroll window
    assert pos[2] + U < tl[2] <= pos[2] + U + td[2] and rl[2] > tl[2]  # mask 0, slice clipped by reward_len
    assert pos[3] == 0 and tl[3] == 1
    assert (z["re_root_r64_values"][1, tl[1] - pos[1]:] == 0).all()


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
class _Out:
    """A network output holding only predicted values (use_pred_value runs no search)."""

    def __init__(self, value, dev):
        self.value = torch.from_numpy(value.reshape(-1, 1)).to(dev)
        self.hidden_state = self.value


@pytest.mark.gpu
@pytest.mark.parametrize("rk", ["64", "32"])
def test_value_targets_re_kernel(rk, golden):
    """Mode RE on the fixture's trajectories, fed the recorded search / predicted values."""
    from mazero_amd.consume import reanalyze_value_targets

    z = golden
    dev = torch.device("cuda", 0)
    U, disc = int(z["cfg"][1]), float(z["discount"])
    rewards, _ = golden_games(z, DTYPES[rk], np.float64)
    for which in ("root", "pred"):
        value = z["search_value"] if which == "root" else z["pred_value"]
        r, v = reanalyze_value_targets(None, None, _Out(value, dev), None, rewards=rewards, pos=z["pos"],
                                       traj_len=z["traj_len"], td_steps=z["td_steps"], discount=disc,
                                       num_unroll_steps=U, td_max=5, use_root_value=False, use_pred_value=True)
        same_bits(r.cpu().numpy(), z[f"re_{which}_r{rk}_rewards"], f"re {which} r{rk} rewards")
        same_bits(v.cpu().numpy(), z[f"re_{which}_r{rk}_values"], f"re {which} r{rk} values")
        er, ev = rows_re(value, golden_td_pow(z), z["td_steps"], z["pos"], z["traj_len"], rewards, U, disc)
        same_bits(v.cpu().numpy(), ev, "restatement")
        same_bits(r.cpu().numpy(), er, "restatement")


@pytest.mark.gpu
@pytest.mark.parametrize("rk", ["64", "32"])
@pytest.mark.parametrize("sk", ["64", "32"])
def test_value_targets_non_re_kernel(rk, sk, golden):
    from mazero_amd.consume import value_targets_non_re

    z = golden
    dev = torch.device("cuda", 0)
    U, TD, disc = int(z["cfg"][1]), int(z["cfg"][2]), float(z["discount"])
    rewards, stored = golden_games(z, DTYPES[rk], DTYPES[sk])
    r, v = value_targets_non_re(rewards, stored, z["pos"], z["traj_len"], td_steps=TD, discount=disc,
                                num_unroll_steps=U, device=dev)
    same_bits(r.cpu().numpy(), z[f"nonre_r{rk}_s{sk}_rewards"], "rewards")
    same_bits(v.cpu().numpy(), z[f"nonre_r{rk}_s{sk}_values"], "values")
    er, ev = rows_non_re(stored, TD, z["pos"], z["traj_len"], rewards, U, disc)
    same_bits(v.cpu().numpy(), ev, "restatement")
    same_bits(r.cpu().numpy(), er, "restatement")


@pytest.mark.gpu
def test_value_targets_many_rows_against_restatement():
    """More than one block of rows (G = 40, U = 5: 240 rows), random trajectories, td 1..5."""
    from mazero_amd.consume import reanalyze_value_targets, value_targets_non_re

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    G, U, TD, disc = 40, 5, 5, 0.997
    tl = rng.integers(1, 16, size=G)
    rl = tl + rng.integers(0, 3, size=G)
    pos = np.array([rng.integers(0, t) for t in tl])
    td = rng.integers(1, TD + 1, size=G)
    value = (3.0 * rng.standard_normal(G * (U + 1))).astype(np.float32)
    td_pow = np.power(disc, [np.intc(t) for t in np.repeat(td, U + 1)])
    for rdt in (np.float64, np.float32):
        rewards = [rng.standard_normal(n).astype(rdt) for n in rl]
        r, v = reanalyze_value_targets(None, None, _Out(value, dev), None, rewards=rewards, pos=pos, traj_len=tl,
                                       td_steps=td, discount=disc, num_unroll_steps=U, td_max=TD,
                                       use_root_value=False, use_pred_value=True)
        er, ev = rows_re(value, td_pow, td, pos, tl, rewards, U, disc)
        same_bits(v.cpu().numpy(), ev, "re values")
        same_bits(r.cpu().numpy(), er, "re rewards")
        # a rank's share that starts and ends inside a trajectory: rows [7, 100)
        rp, vp = reanalyze_value_targets(None, None, _Out(value[7:100], dev), None, rewards=rewards, pos=pos,
                                         traj_len=tl, td_steps=td, discount=disc, num_unroll_steps=U, td_max=TD,
                                         use_root_value=False, use_pred_value=True, rows=(7, 100))
        same_bits(vp.cpu().numpy(), ev.reshape(-1)[7:100], "re values, rows [7, 100)")
        same_bits(rp.cpu().numpy(), er.reshape(-1)[7:100], "re rewards, rows [7, 100)")
        for sdt in (np.float64, np.float32):
            stored = [(3.0 * rng.standard_normal(n)).astype(sdt) for n in tl]
            r, v = value_targets_non_re(rewards, stored, pos, tl, td_steps=TD, discount=disc, num_unroll_steps=U,
                                        device=dev)
            er, ev = rows_non_re(stored, TD, pos, tl, rewards, U, disc)
            same_bits(v.cpu().numpy(), ev, "non-re values")
            same_bits(r.cpu().numpy(), er, "non-re rewards")


def _run_adv(q, pred, mask, dev):
    from mazero_amd.consume import normalize_advantage

    adv, stats = normalize_advantage(torch.from_numpy(q).to(dev), torch.from_numpy(pred).to(dev),
                                     torch.from_numpy(mask).to(dev))
    return adv.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", ADV_SIZES)
def test_normalize_advantage_kernel(n, product_lib):
    from mazero_amd.consume import pairwise_plan

    dev = torch.device("cuda", 0)
    q, pred, mask = adv_case(n, 100 + n)
    adv, stats = _run_adv(q, pred, mask, dev)
    want, wm, ws = advantage_numpy(q, pred, mask)
    print(f"n={n}: mean {stats[0]!r} (numpy {wm!r}), std {stats[1]!r} (numpy {ws!r})")
    same_bits(adv, want, f"n={n}")
    same_stats(stats, [wm, ws], f"n={n} statistics")
    got, gm, gs = advantage_restated(q, pred, mask, pairwise_plan(n, product_lib))
    same_bits(adv, got, "restatement")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["all_masked", "single", "nan_masked"])
def test_normalize_advantage_edge_cases(kind):
    dev = torch.device("cuda", 0)
    for n in (9, 1537):
        q, pred, mask = adv_case(n, 7 + n, kind)
        adv, stats = _run_adv(q, pred, mask, dev)
        want, wm, ws = advantage_numpy(q, pred, mask)
        same_bits(adv, want, f"{kind} n={n}")
        same_stats(stats, [wm, ws], f"{kind} n={n} statistics")
        if kind == "all_masked":
            assert np.isnan(stats).all() and not adv.any()
        elif kind == "single":
            assert stats[1] == 0.0 and not adv.any()
        else:
            assert np.isfinite(stats).all() and np.isfinite(adv).all()  # the NaN stayed out of the sums


def _trajectories(rng, G, U):
    tl = np.array([14, 4][:G] + [int(x) for x in rng.integers(1, 12, size=max(0, G - 2))])
    pos = np.array([2, 1][:G] + [0] * max(0, G - 2))
    td = np.array([3, 5][:G] + [int(x) for x in rng.integers(1, 6, size=max(0, G - 2))])
    rewards = [rng.standard_normal(n + 1) for n in tl]
    return rewards, pos, tl, td


@pytest.mark.gpu
def test_reanalyze_value_targets_match_oracle(port_lib):
    """use_root_value end to end: the agent-0 search on the device feeds the kernel; the oracle
    driver on the CPU port feeds the restatement.  12 roots (2 x 6), the 3m shape."""
    from driver import OracleSampledMCTS
    from mazero_amd.consume import reanalyze_value_targets
    from mazero_amd.mcts_sampled import SampledMCTS
    from mazero_amd.nets import SearchConfig, make_net, make_root_batch

    N, A, G, U, S = 3, 9, 2, 5, 8
    dev = torch.device("cuda", 0)
    cfg = SearchConfig(action_space_size=A, num_simulations=S, sampled_action_times=1)
    net = make_net(N, A, seed=51, device=dev)
    out, legal = make_root_batch(net, G * (U + 1), 64, seed=52, device=dev, legal_zero_frac=0.25)
    rewards, pos, tl, td = _trajectories(np.random.default_rng(53), G, U)
    rs_o = np.random.Generator(np.random.PCG64(54))
    rs_d = np.random.Generator(np.random.PCG64(54))
    so = OracleSampledMCTS(cfg, rs_o, port_lib).batch_search(net, out, 0, None, N, legal, device=dev, add_noise=True,
                                                             sampled_tau=1.0)
    value = np.asarray(so["value"], np.float32).reshape(-1)
    td_pow = np.power(cfg.discount, [np.intc(t) for t in np.repeat(td, U + 1)])
    er, ev = rows_re(value, td_pow, td, pos, tl, rewards, U, cfg.discount)
    r, v = reanalyze_value_targets(SampledMCTS(cfg, rs_d), net, out, legal, rewards=rewards, pos=pos, traj_len=tl,
                                   td_steps=td, discount=cfg.discount, num_unroll_steps=U, td_max=5, device=dev)
    assert r.shape == (G, U + 1) and v.dtype == torch.float64 and v.is_cuda
    same_bits(v.cpu().numpy(), ev, "values")
    same_bits(r.cpu().numpy(), er, "rewards")
    assert np.array_equal(rs_o.random(4), rs_d.random(4))  # np_random consumed identically


@pytest.mark.gpu
def test_sharded_value_targets_match_unsharded():
    from mazero_amd.nets import SearchConfig, make_net
    from mazero_amd.workers import ReanalyzeShard

    # 64 rows in shards of 32, the shapes tests/test_workers.py pins the harness at: the network's
    # half-precision matrix products give a row the same bits in both batch sizes there (they do
    # not for every pair of sizes, e.g. 18 and 9; that is the network's arithmetic, not the targets')
    N, A, G, U, OBS = 3, 9, 16, 3, 64
    total = G * (U + 1)
    dev = torch.device("cuda", 0)
    net = make_net(N, A, obs_size=OBS, seed=61, device=dev)
    cfg = SearchConfig(action_space_size=A, num_simulations=12, sampled_action_times=2)
    rng = np.random.default_rng(62)
    obs = rng.standard_normal((total, N, OBS)).astype(np.float32)
    legal = (rng.random((total, N, A)) > 0.3).astype(np.int64)
    legal[..., 1] = 1
    rewards, pos, tl, td = _trajectories(rng, G, U)

    def run(rank, world, root):
        sh = ReanalyzeShard(net, cfg, total, seed=63, rank=rank, world=world, device=dev)
        return sh.value_targets(torch.from_numpy(obs[sh.lo:sh.hi]).to(dev), legal[sh.lo:sh.hi], rewards=rewards,
                                pos=pos, traj_len=tl, td_steps=td, num_unroll_steps=U, td_max=5, use_root_value=root)

    for root in (True, False):
        ref = run(0, 1, root)
        parts = [run(r, 2, root) for r in range(2)]
        assert [p["lo"] for p in parts] == [0, total // 2]
        for f in ("batch_values", "batch_rewards"):
            same_bits(np.concatenate([p[f] for p in parts]), ref[f].reshape(-1), f"{f} root={root}")
        assert ref["batch_values"].any()


@pytest.mark.gpu
def test_argument_checks(product_lib):
    from mazero_amd._capi import MZ_ERR_ARG, MZ_ERR_UNSUPPORTED, MZ_VALUE_NON_RE, MZ_VALUE_RE
    from mazero_amd.consume import normalize_advantage, reanalyze_value_targets, value_targets_non_re

    dev = torch.device("cuda", 0)
    lib = product_lib
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    i32 = torch.ones(2, dtype=torch.int32, device=dev)
    f64 = torch.zeros(16, dtype=torch.float64, device=dev)
    f32 = torch.zeros(16, dtype=torch.float32, device=dev)
    u8 = torch.ones(16, dtype=torch.uint8, device=dev)

    def vt(mode=MZ_VALUE_RE, row0=0, n=4, value=p(f32), out=p(f64), stored=None):
        return lib.mz_value_targets(None, None, mode, row0, n, 2, 1, value, p(f64), p(i32), p(i32), p(i32), p(i32),
                                    p(f64), 0, stored, 0, 8, p(f64), p(f32), 5, out, p(f64))

    assert vt() == 0
    assert vt(value=None) == MZ_ERR_ARG and b"null" in lib.mz_last_error()
    assert vt(out=None) == MZ_ERR_ARG
    assert vt(mode=MZ_VALUE_NON_RE) == MZ_ERR_ARG  # no stored values
    assert vt(mode=7) == MZ_ERR_ARG
    assert vt(row0=2, n=3) == MZ_ERR_ARG and b"rows" in lib.mz_last_error()
    assert lib.mz_normalize_advantage(None, None, p(f32), p(f32), p(u8), 16, p(f64), p(f64)) == 0
    assert lib.mz_normalize_advantage(None, None, None, p(f32), p(u8), 16, p(f64), p(f64)) == MZ_ERR_ARG
    assert lib.mz_normalize_advantage(None, None, p(f32), p(f32), p(u8), 0, p(f64), p(f64)) == MZ_ERR_ARG
    assert lib.mz_normalize_advantage(None, None, p(f32), p(f32), p(u8), 65537, p(f64), p(f64)) == MZ_ERR_UNSUPPORTED
    assert b"65536" in lib.mz_last_error()
    torch.cuda.synchronize()
    big = torch.zeros(65537, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError):
        normalize_advantage(big, big, torch.ones(65537, dtype=torch.bool, device=dev))
    kw = dict(pos=[0], traj_len=[4], discount=0.997, num_unroll_steps=2)
    with pytest.raises(ValueError, match="reward_len < traj_len"):
        value_targets_non_re([np.zeros(3)], [np.zeros(4)], td_steps=2, device=dev, **kw)
    with pytest.raises(ValueError, match="reward_len < traj_len"):
        reanalyze_value_targets(None, None, _Out(np.zeros(3, np.float32), dev), None, rewards=[np.zeros(3)],
                                td_steps=[2], use_root_value=False, use_pred_value=True, **kw)
    with pytest.raises(ValueError, match="td_max"):
        reanalyze_value_targets(None, None, _Out(np.zeros(3, np.float32), dev), None, rewards=[np.zeros(4)],
                                td_steps=[6], td_max=5, use_root_value=False, use_pred_value=True, **kw)
