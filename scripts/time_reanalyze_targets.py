"""Times the reanalyze batch's value / reward / advantage targets at the BASELINE batch: 256
trajectories x (5 + 1) unroll steps = 1,536 rows, td_steps = 5 (core/reanalyze_worker.py:137-164 and
:466-473), once the search's root values are on the device.

host    what a caller of the search had to do before: copy `DeviceSearchOutput.value` to the host,
        run the reference-shaped Python loop over the rows, normalise the advantages with numpy;
device  mazero_amd.consume.reanalyze_value_targets (use_pred_value: the values are already a device
        tensor, as after the search) + normalize_advantage, ending with a device synchronisation --
        `wrappers` includes their host preparation (padding, np.power, uploads), `kernels` is the
        two launches alone on prepared inputs.

Each path: warm-up, then `--reps` repetitions, the median and the 10th / 90th percentiles of the
wall-clock time.  Prints one JSON line.

    python scripts/time_reanalyze_targets.py [--reps 200] [--warmup 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mazero_amd import consume  # noqa: E402
from mazero_amd._capi import MZ_VALUE_RE  # noqa: E402


def host_targets(value_dev, td_steps, pos, traj_len, rewards, U, discount, q_dev, pred_dev, mask):
    value_lst = value_dev.cpu().numpy().flatten()  # the device-to-host copy
    td_steps_lst = [np.intc(t) for t in np.repeat(td_steps, U + 1)]
    value_mask = [int(pos[g] + k + td_steps[g] < traj_len[g]) for g in range(len(pos)) for k in range(U + 1)]
    value_lst = value_lst * np.power(discount, td_steps_lst)
    value_lst = value_lst * value_mask
    batch_values, batch_rewards = [], []
    j = 0
    for g in range(len(pos)):
        tv, tr = [], []
        for current in range(pos[g], pos[g] + U + 1):
            boot = current + td_steps_lst[j]
            for i, reward in enumerate(rewards[g][current:boot]):
                value_lst[j] += reward * discount ** i
            if current < traj_len[g]:
                tv.append(value_lst[j])
                tr.append(rewards[g][current])
            else:
                tv.append(0.0)
                tr.append(0.0)
            j += 1
        batch_values.append(tv)
        batch_rewards.append(tr)
    batch_values, batch_rewards = np.asarray(batch_values), np.asarray(batch_rewards)
    adv = q_dev.cpu().numpy().astype(np.float64) - pred_dev.cpu().numpy().astype(np.float64)
    adv_copy = np.array(adv)
    adv_copy[~mask] = np.nan
    adv = (adv - np.nanmean(adv_copy)) / (np.nanstd(adv_copy) + 1e-5)
    adv[~mask] = 0.
    return batch_rewards, batch_values, adv


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(np.percentile(ts, 10)), 4),
                p90_ms=round(float(np.percentile(ts, 90)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trajectories", type=int, default=256)
    a = ap.parse_args()
    G, U, TD, disc = a.trajectories, 5, 5, 0.997
    n = G * (U + 1)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    tl = rng.integers(20, 120, size=G)
    pos = np.array([rng.integers(0, t) for t in tl])
    td = rng.integers(1, TD + 1, size=G)
    rewards = [rng.standard_normal(t) for t in tl]
    value = torch.from_numpy((3 * rng.standard_normal(n)).astype(np.float32)).to(dev)
    pred = torch.from_numpy((3 * rng.standard_normal(n)).astype(np.float32)).to(dev)
    mask = rng.random(n) < 0.8
    mask_dev = torch.from_numpy(mask).to(dev)

    Out = types.SimpleNamespace(hidden_state=value, value=value)  # (only the values are read)

    def device_wrappers():
        r, v = consume.reanalyze_value_targets(None, None, Out, None, rewards=rewards, pos=pos, traj_len=tl,
                                               td_steps=td, discount=disc, num_unroll_steps=U, td_max=TD,
                                               use_root_value=False, use_pred_value=True)
        adv, stats = consume.normalize_advantage(value, pred, mask_dev)
        return r, v, adv

    ti = consume._target_inputs(rewards, pos, tl, td, disc, U, TD, dev)
    td_pow = torch.from_numpy(np.power(disc, [np.intc(t) for t in np.repeat(td, U + 1)])).to(dev)
    mask_u8 = mask_dev.to(torch.uint8)

    def device_kernels():
        consume._launch_value_targets(None, dev, MZ_VALUE_RE, ti, 0, n, value, td_pow, None, False)
        consume.normalize_advantage(value, pred, mask_u8)

    hr, hv, hadv = host_targets(value, td, pos, tl, rewards, U, disc, value, pred, mask)
    dr, dv, dadv = device_wrappers()
    same = all(np.array_equal(x.cpu().numpy().reshape(-1).view(np.uint64), np.asarray(y).reshape(-1).view(np.uint64))
               for x, y in ((dr, hr), (dv, hv), (dadv, hadv)))
    res = dict(rows=n, unroll_steps=U, td_steps=TD, reps=a.reps, warmup=a.warmup, bit_identical=bool(same),
               device=torch.cuda.get_device_name(0),
               host=timed(lambda: host_targets(value, td, pos, tl, rewards, U, disc, value, pred, mask),
                          max(2, a.warmup // 4), max(10, a.reps // 4)),
               device_wrappers=timed(device_wrappers, a.warmup, a.reps),
               device_kernels=timed(device_kernels, a.warmup, a.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
