"""Records tests/golden/reanalyze_values.npz: the value and reward targets computed by the REFERENCE's
own `ReanalyzeWorker._prepare_reward_value_re` and `_prepare_reward_value_non_re`
(core/reanalyze_worker.py:51-210), imported from the reference checkout (MZ_REFERENCE, default
/root/reference).  Build container only: the tests read the .npz, never the reference.

How the reference methods are run without their environment (as oracle/gen_driver_golden.py):
- `ray`, `cv2`, `gymnasium` and the Cython tree are absent: empty stand-in modules are registered
  for the import of core.reanalyze_worker alone; no bytecode is written under the reference;
- the two methods are called unbound on a SimpleNamespace `self` (config, zero_obs, device, model,
  np_random) with duck-typed games (`__len__`, rewards, root_values, pred_values, legal_actions, obs);
- the module's `SampledMCTS` is replaced by a stub whose `batch_search` returns recorded root
  values, and the model's `initial_inference` returns recorded predicted values: the search and the
  network are inputs of the methods under record, not part of them.

Recorded: the trajectories (padded rewards and stored values, lengths, positions, replay indices),
the configuration numbers, the per-row search / predicted values (float32), and both outputs of
- RE with use_root_value and with use_pred_value, rewards float64 and float32;
- NON_RE for rewards x stored values in {float64, float32}^2.

Usage:  python scripts/gen_reanalyze_golden.py
"""
from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True  # nothing may be written under the reference checkout

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = os.environ.get("MZ_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "reanalyze_values.npz")

G, U, TD, AUTO_TD, DISCOUNT, TC = 4, 5, 5, 10, 0.997, 100
# (len(game), len(game.rewards), state_index, replay index): td steps 1, 3, 5, 5 after the clip
#   0: every row and every bootstrap index inside the trajectory
#   1: the trajectory ends inside the unroll window (rows past it give 0; the others bootstrap outside)
#   2: current < len(game) <= current + td for the later rows; one reward more than steps
#   3: state_index 0 of a single-step trajectory
GAMES = [(20, 20, 3, TC - 4 * AUTO_TD), (9, 9, 6, TC - 2 * AUTO_TD), (12, 13, 4, TC), (1, 1, 0, TC - 5)]


def _import_reference():
    for name in ("ray", "cv2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["ray"].remote = lambda cls: cls  # the decorator of RemoteReanalyzeWorker (:614)
    gym = types.ModuleType("gymnasium")

    class Wrapper:
        def __init__(self, env=None):
            self.env = env

    gym.Wrapper = gym.ObservationWrapper = Wrapper
    gym.spaces = types.SimpleNamespace(Box=None)
    gym.utils = types.ModuleType("gymnasium.utils")
    gym.utils.seeding = types.SimpleNamespace(np_random=None)
    sys.modules.setdefault("gymnasium", gym)
    sys.modules.setdefault("gymnasium.utils", gym.utils)
    cy = types.ModuleType("core.mcts.ctree.ctree_sampled.cytree")
    cy.Tree_batch = object
    sys.modules["core.mcts.ctree.ctree_sampled.cytree"] = cy
    if REFERENCE not in sys.path:
        sys.path.insert(0, REFERENCE)
    from core import reanalyze_worker

    assert os.path.realpath(reanalyze_worker.__file__).startswith(os.path.realpath(REFERENCE))
    return reanalyze_worker


class Game:
    """The GameHistory attributes the two methods read."""

    def __init__(self, n, rewards, root_values, pred_values):
        self.n, self.rewards, self.root_values, self.pred_values = n, rewards, root_values, pred_values
        self.legal_actions = [np.ones((1, 3), np.int64) for _ in range(n)]

    def __len__(self):
        return self.n

    def obs(self, i, extra_len=0, padding=False):
        return np.zeros((extra_len + 2, 1, 2), np.float32)  # sliced to (stacked_observations, N, d)


def main():
    rw = _import_reference()
    g = np.random.default_rng(20)
    L = max(r for _, r, _, _ in GAMES)
    rewards = np.zeros((G, L))
    stored = np.zeros((G, L))
    for i, (n, rl, _, _) in enumerate(GAMES):
        rewards[i, :rl] = g.standard_normal(rl)
        stored[i, :n] = 3.0 * g.standard_normal(n)
    n_rows = G * (U + 1)
    search_value = (3.0 * g.standard_normal(n_rows)).astype(np.float32)
    pred_value = (3.0 * g.standard_normal(n_rows)).astype(np.float32)

    class StubMCTS:  # stands in for core.mcts.SampledMCTS: the search's values are an input here
        def __init__(self, config, np_random):
            pass

        def batch_search(self, **kw):
            assert kw["current_agent_idx"] == 0 and kw["factor"] is None and kw["add_noise"] and kw["sampled_tau"] == 1.0
            assert kw["legal_actions_lst"].shape == (n_rows, 1, 3)
            return types.SimpleNamespace(value=search_value.copy())

    rw.SampledMCTS = StubMCTS
    model = types.SimpleNamespace(
        initial_inference=lambda obs: types.SimpleNamespace(value=pred_value.copy().reshape(n_rows, 1)))

    def worker(**cfg):
        config = types.SimpleNamespace(auto_td_steps=AUTO_TD, td_steps=TD, num_unroll_steps=U, stacked_observations=1,
                                       image_based=False, discount=DISCOUNT, num_agents=1, batch_size=G, **cfg)
        return types.SimpleNamespace(config=config, zero_obs=np.zeros((1, 1, 2), np.float32), device="cpu", model=model,
                                     np_random=None)

    def games(rdt, sdt):
        return [Game(n, rewards[i, :rl].astype(rdt), stored[i, :n].astype(sdt), stored[i, :n].astype(sdt))
                for i, (n, rl, _, _) in enumerate(GAMES)]

    pos = [p for _, _, p, _ in GAMES]
    indices = [ix for _, _, _, ix in GAMES]
    z = dict(cfg=np.array([G, U, TD, AUTO_TD, TC], np.int64), discount=np.float64(DISCOUNT),
             traj_len=np.array([n for n, _, _, _ in GAMES], np.int32),
             reward_len=np.array([r for _, r, _, _ in GAMES], np.int32), pos=np.array(pos, np.int32),
             indices=np.array(indices, np.int64), rewards=rewards, stored=stored, search_value=search_value,
             pred_value=pred_value)
    td = [int(np.clip(TD - (TC - ix) // AUTO_TD, 1, TD)) for ix in indices]
    assert td == [1, 3, 5, 5], td
    z["td_steps"] = np.array(td, np.int32)
    dts = {"64": np.float64, "32": np.float32}
    for rk, rdt in dts.items():
        for which, cfg in (("root", dict(use_root_value=True, use_pred_value=False)),
                           ("pred", dict(use_root_value=False, use_pred_value=True))):
            br, bv = rw.ReanalyzeWorker._prepare_reward_value_re(worker(**cfg), indices, games(rdt, np.float64), pos, TC)
            z[f"re_{which}_r{rk}_rewards"], z[f"re_{which}_r{rk}_values"] = br, bv
            assert br.dtype == np.float64 and bv.dtype == np.float64 and bv.shape == (G, U + 1)
        for sk, sdt in dts.items():
            br, bv = rw.ReanalyzeWorker._prepare_reward_value_non_re(
                worker(use_root_value=True, use_pred_value=False), games(rdt, sdt), pos)
            z[f"nonre_r{rk}_s{sk}_rewards"], z[f"nonre_r{rk}_s{sk}_values"] = br, bv
            assert br.dtype == np.float64 and bv.dtype == np.float64 and bv.shape == (G, U + 1)
    np.savez_compressed(OUT, **z)
    print(f"{OUT}: {os.path.getsize(OUT)} B")


if __name__ == "__main__":
    main()
