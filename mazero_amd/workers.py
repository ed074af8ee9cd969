"""Process-per-GPU self-play and reanalyze.

The reference runs its workers as Ray actors (`RemoteDataWorker`, core/selfplay_worker.py:344-407;
`RemoteReanalyzeWorker`, core/reanalyze_worker.py:614-722).  Each one pulls fresh weights from the
`SharedStorage` actor through the object store (core/storage.py:68-80) when the learner's trained-steps
counter has crossed into a new checkpoint interval (`_update_model_before_step`,
selfplay_worker.py:371-375; reanalyze: `target_model_interval`, reanalyze_worker.py:663-669).

Here there is one process per GPU and one rank per process:
- the environments (self-play) or the batch's roots (reanalyze) are sharded over the ranks,
  contiguously (`shard.shard_bounds`);
- every rank holds the same `np_random` state and its search is `SampledMCTS(..., root_shard=...)`:
  the per-root random draws are made for the whole batch and sliced, and tree i is seeded with its
  global index, so rank r's decisions are rows [lo, hi) of the unsharded step, bit for bit;
- the weights travel by one collective from the learner's rank (`weights.WeightBroadcaster`, RCCL
  over xGMI on MI355X; gloo on the CPU), with the reference's checkpoint-interval rule;
- nothing crosses ranks during a search;
- with `shard_active`, self-play ranks search only the environments still running: each rank takes
  its part of the sorted global active list (`shard.active_shard`, `gather_active`) as the root shard
  of the search over that list, on one tree handle whose root offset follows the shard on the device
  (`SampledMCTS(..., device_root_offset=True)`).

The environment, the replay buffer and the learner stay out of scope: `env` is a
callable that yields a shard's observations and legal-action masks, and `learner` is an optional
callable run on the source rank after each step, returning the trained-steps counter it publishes.
`make_mcts` and `decide` default to the MI355X search and the on-device consumers
(mazero_amd.consume); tests inject the oracle driver and the restated host consumers to run the
same harness on the CPU.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np
import torch
import torch.distributed as dist

from .shard import active_shard, shard_bounds


def _rank_world(group=None):
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def _to_np(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _device_selfplay_decide(mcts, model, network_output, N, legal, *, temperature, sampled_tau, greedy_epsilon,
                            eps_uniforms, device):
    from .consume import selfplay_decisions

    d = selfplay_decisions(mcts, model, network_output, N, legal, temperature=temperature, sampled_tau=sampled_tau,
                           greedy_epsilon=greedy_epsilon, eps_uniforms=eps_uniforms, device=device)
    return dict(actions=d.actions, count_entropy=d.count_entropy, prob_action=d.prob_action,
                visit_entropy=d.visit_entropy, root_value=d.root_value)


def _device_reanalyze_decide(mcts, model, network_output, legal, policy_mask, device):
    from .consume import reanalyze_policy_targets

    return reanalyze_policy_targets(mcts, model, network_output, legal, policy_mask, device)._asdict()


def _default_mcts(config, np_random, root_shard, wide_actions=None, later_action_cache=None, root_capacity=None,
                  device_root_offset=None):
    from .mcts_sampled import SampledMCTS

    return SampledMCTS(config, np_random, root_shard=root_shard, wide_actions=wide_actions,
                       later_action_cache=later_action_cache, root_capacity=root_capacity,
                       device_root_offset=device_root_offset)


def gather_active(local_active, group=None) -> np.ndarray:
    """The sorted global list of the environments still running, from each rank's own: an
    all_gather_object of the ranks' running global indices, so that every rank holds the same `active`
    for SelfPlayShard.step without a collective of the caller's.  Without a process group the local
    list is the global one."""
    local = [int(i) for i in np.asarray(local_active, dtype=np.int64).reshape(-1)]
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return np.asarray(sorted(local), dtype=np.int64)
    parts = [None] * dist.get_world_size(group)
    dist.all_gather_object(parts, local, group=group)
    return np.asarray(sorted(i for part in parts for i in part), dtype=np.int64)


@dataclass
class StepRecord:
    """What one rank decided in one environment step (selfplay_worker.py:189-293)."""

    step: int
    model_index: int          # the checkpoint the rank searched with
    lo: int                   # the rank's first global environment
    actions: np.ndarray       # int32 [hi - lo, N]
    prob_action: np.ndarray   # float64 [hi - lo]
    root_value: np.ndarray    # float32 [hi - lo]
    count_entropy: np.ndarray  # float64 [hi - lo, N]
    visit_entropy: np.ndarray  # float64 [hi - lo, N]
    # SelfPlayShard.step(active=...): the environments that ran this step (sorted indices; the rows
    # above are theirs, in this order); None when all ran
    active: Optional[np.ndarray] = None


class _Shard:
    def __init__(self, model, config, total: int, *, seed: int, broadcaster=None, group=None, src: int = 0,
                 make_mcts: Optional[Callable] = None, device=None, rank: Optional[int] = None,
                 world: Optional[int] = None, wide_actions: Optional[bool] = None,
                 later_action_cache: Optional[bool] = None, root_capacity: Optional[int] = None,
                 shard_active: Optional[bool] = None):
        """`root_capacity` goes to the default search (SampledMCTS: every search of up to that many
        roots on one tree handle and one set of recorded loops; None reads `config.root_capacity`).
        Without `shard_active` it needs world == 1, where the shard builds its search without a root
        shard (the whole batch is the shard): SampledMCTS refuses it together with a root shard.
        `shard_active`: SelfPlayShard.step(active=...) on any rank.  The rank searches the active
        environments it owns as the root shard shard.active_shard(active, lo, hi) of the search over the
        whole active list, on one tree handle of `root_capacity` roots (default: the rank's own hi - lo)
        whose root offset follows the shard on the device (SampledMCTS device_root_offset).  None reads
        `config.shard_active` (False when the config has none: the refusal of step(active=...) with
        world > 1 is pinned by the test suite).
        `wide_actions` goes to the default search (SampledMCTS: action spaces up to 255 instead of
        64; None reads `config.wide_actions`), and so does `later_action_cache` (the later agents'
        greedy actions from a per-node cache; None reads `config.later_action_cache`); a `make_mcts` of
        the caller's decides for itself."""
        self.model, self.config, self.total = model, config, int(total)
        self.rank, self.world = _rank_world(group)
        if rank is not None or world is not None:  # a shard without a process group (single-GPU tests)
            if broadcaster is not None:
                raise ValueError("an explicit rank / world needs broadcaster=None")
            self.rank, self.world = int(rank or 0), int(world or 1)
        self.lo, self.hi = shard_bounds(self.total, self.world, self.rank)
        if self.hi <= self.lo:
            raise ValueError(f"rank {self.rank} of {self.world} owns no roots of {self.total}")
        # the same generator state on every rank: sharded draws are sliced from whole-batch draws
        self.np_random = np.random.RandomState(seed)
        self.broadcaster, self.src, self.group = broadcaster, src, group
        if shard_active is None:
            shard_active = getattr(config, "shard_active", False)
        self.shard_active = bool(shard_active)
        self.make_mcts = make_mcts or (lambda c, r, s: _default_mcts(c, r, s, wide_actions, later_action_cache,
                                                                     root_capacity))
        if root_capacity is None:
            root_capacity = getattr(config, "root_capacity", None)
        self.root_capacity = root_capacity
        # step(active=...) under shard_active: the search of the rank's active environments
        cap = (self.hi - self.lo) if root_capacity is None else int(root_capacity)
        self.make_active_mcts = make_mcts or (lambda c, r, s: _default_mcts(c, r, s, wide_actions, later_action_cache,
                                                                            cap, device_root_offset=True))
        self.device = device
        self.model_index = -1
        if broadcaster is not None and self.rank == src and broadcaster.model_index < 0:
            # the source's weights are checkpoint 0, pulled by every rank before its first step
            # (last_model_index starts at -1: -1 // interval < 0 // interval)
            broadcaster.publish(0)

    @property
    def root_shard(self):
        return (self.lo, self.hi, self.total)

    def _search_shard(self):
        """The root shard the search is built with: None for a capacity search on a single rank (the
        whole batch is the shard, so the draws and the tree seeds are those of (0, total, total))."""
        if self.root_capacity is not None and self.world == 1:
            return None
        return self.root_shard

    def _sync(self) -> int:
        if self.broadcaster is not None:
            self.model_index = self.broadcaster.sync()
        return self.model_index

    def _publish(self, learner, t) -> None:
        """The learner's hook on the source rank: learner(model, t) -> trained-steps counter, or
        (counter, state_dict) with the learner's new weights, or None."""
        if learner is None or self.rank != self.src:
            return
        r = learner(self.model, t)
        if r is None or self.broadcaster is None:
            return
        trained, sd = (r if isinstance(r, tuple) else (r, None))
        self.broadcaster.publish(int(trained), sd)

    def _initial_inference(self, obs):
        with torch.no_grad(), torch.autocast("cuda", enabled=isinstance(obs, torch.Tensor) and obs.is_cuda):
            return self.model.initial_inference(obs)  # selfplay_worker.py:181-185


class SelfPlayShard(_Shard):
    """One rank of process-per-GPU self-play over `total_envs` environments: the rank-local
    replacement of DataWorker.run + RemoteDataWorker._update_model_before_step."""

    def __init__(self, model, config, total_envs: int, num_agents: int, *, decide: Optional[Callable] = None,
                 **kw):
        super().__init__(model, config, total_envs, **kw)
        self.num_agents = int(num_agents)
        self.decide = decide or _device_selfplay_decide

    def step(self, t: int, obs, legal, *, temperature: float = 1.0, sampled_tau: float = 1.0,
             greedy_epsilon: float = 0.0, eps_uniforms=None, active=None) -> StepRecord:
        """One environment step of this rank's environments.  `obs` / `legal` are the shard's rows;
        `eps_uniforms` (u_eps [N, total], u_cat [N, total]) are whole-batch draws, sliced here.

        `active`: the sorted indices of the environments still running (selfplay_worker.py:171); `obs`,
        `legal` and `eps_uniforms` then hold those rows only and the step searches len(active) roots, as
        the reference does (:180-211).  The search is built without a root shard, so the per-root draws
        are made for the active rows.  Single rank only, unless the shard was built with `shard_active`.

        With `shard_active`, on any rank: `active` is the global list (the same on every rank;
        gather_active), `obs` / `legal` hold the rows of this rank's active environments only, and
        `eps_uniforms` are whole-active-batch [N, len(active)] arrays, sliced here.  The rank's search is
        the root shard shard.active_shard(active, lo, hi) of the search over the active list, so the
        ranks' records, concatenated, are the single rank's record bit for bit.  A rank none of whose
        environments runs calls neither the model nor the search: it draws from `np_random` what the
        other ranks draw and returns a record of zero rows."""
        if active is not None:
            if self.world > 1 and not self.shard_active:
                raise NotImplementedError(
                    "SelfPlayShard.step(active=...) with world > 1: tree i is seeded with its position in the "
                    "whole active list, so the rank's root offset would change per step, and that offset is a "
                    "launch argument of the prepare kernels baked into the recorded graph")
            active = np.asarray(active, dtype=np.int64).reshape(-1)
            if active.size < 1 or (np.diff(active) <= 0).any() or active[0] < 0 or active[-1] >= self.total:
                raise ValueError(f"active must be sorted, distinct indices in [0, {self.total})")
        idx = self._sync()  # _update_model_before_step, selfplay_worker.py:176-177
        if active is not None and self.shard_active:
            if isinstance(eps_uniforms, str):  # ("torch": torch's global stream, consumed root by root)
                raise NotImplementedError(f"eps_uniforms={eps_uniforms!r} with shard_active: pass the whole "
                                          "active batch's uniforms as arrays")
            p_lo, p_hi, n = active_shard(active, self.lo, self.hi)
            if p_lo == p_hi:
                return self._idle_step(t, idx, n, active)
            if eps_uniforms is not None:
                eps_uniforms = tuple(np.asarray(u)[:, p_lo:p_hi] for u in eps_uniforms)
        net_out = self._initial_inference(obs)
        if active is not None and self.shard_active:
            mcts = self.make_active_mcts(self.config, self.np_random, (p_lo, p_hi, n))
        elif active is not None:
            mcts = self.make_mcts(self.config, self.np_random, None)
        else:
            mcts = self.make_mcts(self.config, self.np_random, self._search_shard())  # :187
            if eps_uniforms is not None:
                eps_uniforms = tuple(np.asarray(u)[:, self.lo:self.hi] for u in eps_uniforms)
        d = self.decide(mcts, self.model, net_out, self.num_agents, legal, temperature=temperature,
                        sampled_tau=sampled_tau, greedy_epsilon=greedy_epsilon, eps_uniforms=eps_uniforms,
                        device=self.device)
        return StepRecord(t, idx, self.lo, _to_np(d["actions"]).astype(np.int32), _to_np(d["prob_action"]),
                          _to_np(d["root_value"]).reshape(-1), _to_np(d["count_entropy"]),
                          _to_np(d["visit_entropy"]), active)

    def _idle_step(self, t: int, idx: int, n: int, active) -> StepRecord:
        """A step in which none of this rank's environments runs: nothing is launched; `np_random`
        moves as on every other rank -- per agent one search's draws (mcts_sampled.skip_search_draws),
        then select_action's uniforms of the n active roots (draw_root_uniforms)."""
        from .mcts_sampled import skip_search_draws

        N = self.num_agents
        for _ in range(N):
            skip_search_draws(self.config, self.np_random, n)
            self.np_random.random(n)
        return StepRecord(t, idx, self.lo, np.zeros((0, N), np.int32), np.zeros(0, np.float64),
                          np.zeros(0, np.float32), np.zeros((0, N), np.float64), np.zeros((0, N), np.float64), active)

    def run(self, env: Callable, steps: int, *, learner: Optional[Callable] = None, eps_uniforms: Callable = None,
            **step_kw) -> List[StepRecord]:
        """`steps` environment steps.  env(t, lo, hi) -> (obs, legal) for environments [lo, hi), or
        (obs, legal, active) with the rows of the environments `active` still running (see step; None:
        all of them; with `shard_active` the global list, with the rows of this rank's part of it);
        learner(model, t) on the source rank after step t -> the trained-steps counter to
        publish (or None); eps_uniforms(t) -> whole-batch (u_eps, u_cat) or None, sliced to the active
        environments here."""
        out = []
        for t in range(steps):
            obs, legal, *rest = env(t, self.lo, self.hi)
            active = rest[0] if rest else None
            u = None if eps_uniforms is None else eps_uniforms(t)
            if u is not None and active is not None:
                u = tuple(np.asarray(x)[:, np.asarray(active, dtype=np.int64)] for x in u)
            out.append(self.step(t, obs, legal, eps_uniforms=u, active=active, **step_kw))
            self._publish(learner, t)
        return out


class ReanalyzeShard(_Shard):
    """One rank of process-per-GPU reanalysis: the policy targets of `_prepare_policy_re`
    (reanalyze_worker.py:212-366) and the value / reward targets of `_prepare_reward_value_re`
    (:51-164) for this rank's share of a batch's B·(K+1) roots, with the target
    weights refreshed by the target-model-interval rule (reanalyze_worker.py:663-669; build the
    broadcaster with checkpoint_interval = config.target_model_interval)."""

    def __init__(self, model, config, total_roots: int, *, decide: Optional[Callable] = None, **kw):
        super().__init__(model, config, total_roots, **kw)
        self.decide = decide or _device_reanalyze_decide

    def targets(self, obs, legal, policy_mask) -> dict:
        """obs / legal / policy_mask: this rank's rows [lo, hi) of the batch."""
        idx = self._sync()
        net_out = self._initial_inference(obs)
        mcts = self.make_mcts(self.config, self.np_random, self._search_shard())
        out = self.decide(mcts, self.model, net_out, legal, policy_mask, self.device)
        out = {k: _to_np(v) for k, v in out.items()}
        out["model_index"] = idx
        out["lo"] = self.lo
        return out

    def value_targets(self, obs, legal, *, rewards, pos, traj_len, td_steps, num_unroll_steps: int,
                      discount: Optional[float] = None, td_max: Optional[int] = None, use_root_value: bool = True
                      ) -> dict:
        """The value and reward targets of `_prepare_reward_value_re` (reanalyze_worker.py:51-164)
        for this rank's rows [lo, hi) of the batch's G·(U+1) rows (`total_roots`).  obs / legal: the
        rank's rows of the bootstrap observations and legal actions (:86-103); rewards, pos,
        traj_len, td_steps: the whole batch's G trajectories (a few numbers each: every rank holds
        them).  Rows are independent, so the result equals rows [lo, hi) of the unsharded call.
        `use_root_value=False` is the reference's use_pred_value.  The advantage normalisation of
        make_batch's step (6) needs the whole batch: gather the ranks' rows, then call
        `consume.normalize_advantage` once."""
        if len(pos) * (int(num_unroll_steps) + 1) != self.total:
            raise ValueError(f"{len(pos)} trajectories x {int(num_unroll_steps) + 1} rows != {self.total} roots")
        idx = self._sync()
        net_out = self._initial_inference(obs)
        mcts = self.make_mcts(self.config, self.np_random, self._search_shard())
        from .consume import reanalyze_value_targets

        r, v = reanalyze_value_targets(
            mcts, self.model, net_out, legal, rewards=rewards, pos=pos, traj_len=traj_len, td_steps=td_steps,
            discount=self.config.discount if discount is None else discount, num_unroll_steps=num_unroll_steps,
            td_max=td_max, use_root_value=use_root_value, use_pred_value=not use_root_value,
            rows=(self.lo, self.hi), device=self.device)
        return dict(batch_rewards=_to_np(r), batch_values=_to_np(v), model_index=idx, lo=self.lo)

    def batch_targets(self, value_obs, value_legal, policy_obs, policy_legal, policy_mask, *, rewards, pos, traj_len,
                      td_steps, num_unroll_steps: int, discount: Optional[float] = None, td_max: Optional[int] = None
                      ) -> dict:
        """`value_targets(value_obs, value_legal, ...)` followed by `targets(policy_obs, policy_legal,
        policy_mask)` with one search fewer: the value search and the agent-0 policy search run as one
        merged search (consume.reanalyze_batch_targets, SampledMCTS.batch_search_many).  The result holds
        both calls' entries, and `np_random` ends where the two calls leave it.  One weight sync and one
        model index serve both.  A merged search draws each entry's own rows, so the rank must own the
        whole batch (world == 1); across root shards it raises ValueError, and the two calls remain."""
        if self.world != 1:
            raise ValueError(f"batch_targets on rank {self.rank} of {self.world}: merged searches do not cross "
                             "root shards (value_targets and targets do)")
        if len(pos) * (int(num_unroll_steps) + 1) != self.total:
            raise ValueError(f"{len(pos)} trajectories x {int(num_unroll_steps) + 1} rows != {self.total} roots")
        idx = self._sync()
        value_out = self._initial_inference(value_obs)
        policy_out = self._initial_inference(policy_obs)
        mcts = self.make_mcts(self.config, self.np_random, None)
        from .consume import reanalyze_batch_targets

        r, v, pol = reanalyze_batch_targets(
            mcts, self.model, value_out, value_legal, policy_out, policy_legal, policy_mask, rewards=rewards, pos=pos,
            traj_len=traj_len, td_steps=td_steps, discount=self.config.discount if discount is None else discount,
            num_unroll_steps=num_unroll_steps, td_max=td_max, rows=(self.lo, self.hi), device=self.device)
        out = {k: _to_np(x) for k, x in pol._asdict().items()}
        out.update(batch_rewards=_to_np(r), batch_values=_to_np(v), model_index=idx, lo=self.lo)
        return out
