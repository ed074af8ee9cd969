"""On-device consumers of the search output (C-ABI include/mzconsume.h).

After every agent's search the reference workers copy each root's result lists to the host and
decide per root in Python:
- self-play (core/selfplay_worker.py:189-293): `select_action` over the root children's visit
  counts with `np_random` (core/utils.py:289-316), `eps_greedy_action` with torch's generator
  (core/utils.py:319-334), then the stored policy probability and visit entropy;
- reanalyze (core/reanalyze_worker.py:275-366, `_prepare_policy_re`): the action
  argmax(marginal visits * legal), and the product of the agents' marginal visit distributions;
- full-game reanalysis (core/reanalyze_worker.py:491-611, `make_renalyze_update`): the same per agent
  turn over the len(game) steps of one game, with the reference's np_random fallback for a root whose
  visits all lie on illegal actions (`reanalyze_game`, `write_game`).

Here the same decisions are made on the device from `DeviceSearchOutput`, in the tree handle's
stream; the next agent's search takes the actions as a device tensor, so an environment step
needs no device-to-host copy of the search lists.

Random draws keep the reference's host generator and order where it has one: each root's
`np_random.choice(n, p=probs)` draws one double (`np_random.random()`), so one
`np_random.random(B)` per agent, in root order, reproduces them (tests/test_consume.py checks this
against numpy's own `choice`).  The epsilon-greedy draws come from torch's global generator in the
reference, one root at a time on the CPU; here they are device uniforms (the same distribution,
not the same stream), or caller-supplied ones.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from ._capi import (MZ_MARGINAL_ARGMAX, MZ_MARGINAL_ARGMAX_LEGAL, MZ_MARGINAL_GIVEN, MZ_VALUE_NON_RE, MZ_VALUE_RE,
                    check)
from .mcts_sampled import DeviceSearchOutput


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev_i32(x, dev) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=torch.int32).contiguous()
    a = np.asarray(x)
    if a.dtype.kind == "f" and not np.array_equal(a, np.round(a)):
        raise ValueError("legal-action masks must hold integer weights")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _root_uniforms(mcts, B: int) -> np.ndarray:
    """select_action's np_random.choice doubles for B roots (a sharded driver draws the whole
    batch's and keeps its own, mcts_sampled.SampledMCTS.draw_root_uniforms)."""
    fn = getattr(mcts, "draw_root_uniforms", None)
    if fn is not None:
        return fn(B)
    return np.asarray(mcts.np_random.random(B), dtype=np.float64)


def _tree(out: DeviceSearchOutput):
    if out.tree is None:
        raise ValueError("DeviceSearchOutput without its tree handle (use SampledMCTS.batch_search_device)")
    tb = out.tree
    # the consumers launch one lane per active root of the handle: `out` must be the handle's current
    # search (on a root_capacity driver a later search of another root count changes the active count)
    ref = out.degrees if out.degrees is not None else out.marginal_visit_count
    if ref is not None and ref.shape[0] != tb.active_roots:
        raise ValueError(f"this search output holds {ref.shape[0]} roots but its tree handle now has "
                         f"{tb.active_roots} active roots: consume an output before a search of another root "
                         "count runs on the same handle")
    tb._sync_stream()
    return tb


def select_actions(out: DeviceSearchOutput, uniforms: Optional[torch.Tensor], temperature: float = 1.0,
                   deterministic: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """select_action (core/utils.py:289-316) at every root -> (pos, agent-0 action, count
    entropy), int32 / int32 / float64 [B] device tensors.  `uniforms`: float64 [B], the doubles
    `np_random.choice` would draw, in root order (unused when deterministic).  A root the kernel cannot
    answer exactly (no children or visits, or a count past what its powers cover: include/mzconsume.h)
    gets -1 and a NaN entropy.  Outside 1/temperature = 1, 2, 3 the first call for a temperature uploads
    a table and must be made outside any graph capture."""
    tb = _tree(out)
    visits = out.sampled["visit_count"].contiguous()
    actions = out.sampled["actions"].contiguous()
    B, width = visits.shape
    dev = visits.device
    if not deterministic:
        uniforms = torch.as_tensor(uniforms, dtype=torch.float64).to(dev).contiguous()
        if uniforms.shape != (B,):
            raise ValueError(f"uniforms must have shape ({B},)")
    pos = torch.empty(B, dtype=torch.int32, device=dev)
    act = torch.empty(B, dtype=torch.int32, device=dev)
    ent = torch.empty(B, dtype=torch.float64, device=dev)
    lib = tb._lib
    with torch.cuda.device(dev):  # (a power table is uploaded to the current device)
        check(lib, lib.mz_select_actions(tb._h, _p(out.degrees), _p(visits), _p(actions), int(width),
                                         float(temperature), int(bool(deterministic)),
                                         None if deterministic else _p(uniforms), _p(pos), _p(act), _p(ent)),
              "select_actions")
    return pos, act, ent


def select_joint_actions(out: DeviceSearchOutput, temperature: float = 1.0, deterministic: bool = True,
                         uniforms: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """select_action at every root of a joint search (SampledMCTS.batch_search_joint_device) and the
    chosen child's whole joint action, `roots_sampled_actions[i][action_pos]` -> (actions int32 [B, N],
    pos int32 [B], count entropy float64 [B]) device tensors.  With the default `deterministic=True`
    this is the reference's evaluation step (core/test.py:101-107); otherwise `uniforms` holds the
    doubles `np_random.choice` would draw, float64 [B] in root order.  A root without children or visits
    gets -1 in `pos` and in every column of its action row."""
    tb = _tree(out)
    visits = out.sampled["visit_count"].contiguous()
    actions = out.sampled["actions"].contiguous()
    B, width = visits.shape
    N = tb.agent_num
    if actions.shape != (B, width * N):
        raise ValueError(f"sampled actions of shape {tuple(actions.shape)} for {B} roots, {width} children and "
                         f"{N} agents")
    dev = visits.device
    if not deterministic:
        uniforms = torch.as_tensor(uniforms, dtype=torch.float64).to(dev).contiguous()
        if uniforms.shape != (B,):
            raise ValueError(f"uniforms must have shape ({B},)")
    pos = torch.empty(B, dtype=torch.int32, device=dev)
    act = torch.empty(B, N, dtype=torch.int32, device=dev)
    ent = torch.empty(B, dtype=torch.float64, device=dev)
    lib = tb._lib
    with torch.cuda.device(dev):
        check(lib, lib.mz_select_actions_joint(tb._h, _p(out.degrees), _p(visits), _p(actions), int(width),
                                               float(temperature), int(bool(deterministic)),
                                               None if deterministic else _p(uniforms), _p(pos), _p(act), _p(ent)),
              "select_joint_actions")
    return act, pos, ent


def eps_greedy(out: DeviceSearchOutput, action: torch.Tensor, legal: torch.Tensor, eps: float,
               u_eps: torch.Tensor, u_cat: torch.Tensor) -> torch.Tensor:
    """eps_greedy_action (core/utils.py:319-334) at every root, in place on `action` (int32 [B]).
    legal: int32 [B, A] (a view with unit column stride); u_eps float32 [B]; u_cat float64 [B]."""
    tb = _tree(out)
    if legal.stride(-1) != 1:
        legal = legal.contiguous()
    lib = tb._lib
    # (named, so that a contiguous copy of a strided row lives until the launch is enqueued: as unnamed
    # temporaries the two copies were freed at once and could share one block of torch's allocator)
    u_eps, u_cat = u_eps.contiguous(), u_cat.contiguous()
    check(lib, lib.mz_eps_greedy(tb._h, _p(legal), int(legal.stride(0)), float(eps), _p(u_eps), _p(u_cat),
                                 _p(action)), "eps_greedy")
    return action


def marginal_policy(out: DeviceSearchOutput, mode: int, action: torch.Tensor, prob: torch.Tensor,
                    legal: Optional[torch.Tensor] = None, entropy: Optional[torch.Tensor] = None):
    """One agent's marginal visit distribution at each root (include/mzconsume.h
    mz_marginal_policy): ARGMAX picks `action`, both modes multiply `prob` (float64 [B]) by the
    distribution at the action and write the visit entropy.  ARGMAX_LEGAL writes `action` only (-1
    where no visit lies on a legal action); `prob` and `entropy` may be None."""
    tb = _tree(out)
    marginal = out.marginal_visit_count[:, 0, :]
    if marginal.stride(-1) != 1:
        marginal = marginal.contiguous()
    if legal is not None and legal.stride(-1) != 1:
        legal = legal.contiguous()
    lib = tb._lib
    check(lib, lib.mz_marginal_policy(tb._h, _p(marginal), int(marginal.stride(0)), _p(legal),
                                      int(legal.stride(0)) if legal is not None else 0, int(mode), _p(action),
                                      _p(prob), _p(entropy)), "marginal_policy")


class SelfPlayDecisions(NamedTuple):
    """One environment step's decisions for every active env (selfplay_worker.py:189-293)."""

    actions: torch.Tensor          # int32 [B, N]: agent_actions
    count_entropy: torch.Tensor    # float64 [B, N]: select_action's entropy (temp_entropies)
    prob_action: torch.Tensor      # float64 [B]: sampled_policy, prod_k marginal_k[action_k]
    visit_entropy: torch.Tensor    # float64 [B, N]: agent_entropies
    root_value: torch.Tensor       # float32 [B]: agent 0's search value
    outputs: List[DeviceSearchOutput]


def torch_eps_uniforms(legal_rows) -> Tuple[np.ndarray, np.ndarray]:
    """The epsilon-greedy draws of eps_greedy_action (core/utils.py:319-334) from torch's global CPU
    generator, exactly as the reference's worker loop makes them: root after root, one
    `torch.rand_like` (float32) then one `Categorical(mask).sample()`.  Returned as the uniforms the
    device kernel (mz_eps_greedy) takes: u_eps is the float32 draw itself; u_cat is the lower edge of
    the sampled action's interval of the mask's cumulative weights, c[a-1] / total in float64, which
    the kernel's inverse cdf maps back to exactly that action (a positive-weight action: the sample's
    own).  legal_rows: [B, A] (the agent's rows, the reference's array dtype).  A host loop over the
    roots, as the reference's: for replaying the reference's torch stream bit for bit."""
    rows = np.asarray(legal_rows)
    B = rows.shape[0]
    u_eps = np.empty(B, np.float32)
    u_cat = np.empty(B, np.float64)
    for i in range(B):
        mask = torch.from_numpy(np.ascontiguousarray(rows[i]))
        u_eps[i] = float(torch.rand_like(mask[..., 0].float()))
        a = int(torch.distributions.Categorical(mask).sample())
        c = np.cumsum(rows[i].astype(np.int64))
        u_cat[i] = 0.0 if a == 0 else float(c[a - 1]) / float(c[-1])
    return u_eps, u_cat


def selfplay_decisions(mcts, model, network_output, true_num_agents: int, legal_actions_lst, *,
                       temperature: float, sampled_tau: float = 1.0, greedy_epsilon: float = 0.0,
                       eps_uniforms: Optional[Tuple] = None, device=None) -> SelfPlayDecisions:
    """The self-play agent loop of selfplay_worker.py:189-293 on the device: one search per
    agent (`mcts.batch_search_device`, later agents conditioned on the earlier agents' device
    actions), select_action + epsilon-greedy per root, then the recorded policy probability.

    `mcts.np_random` is consumed exactly as the reference consumes `self.np_random`.
    eps_uniforms: optional (u_eps float32 [N, B], u_cat float64 [N, B]); drawn with torch.rand on
    the device when omitted (same distribution, not the reference's stream); "torch": drawn per agent
    from torch's global CPU generator as the reference draws them (torch_eps_uniforms), so the
    actions replay the reference's bit for bit (a host loop over the roots)."""
    N = int(true_num_agents)
    hidden = network_output.hidden_state
    dev = hidden.device
    B = hidden.shape[0]
    legal = _dev_i32(legal_actions_lst, dev) if legal_actions_lst is not None else \
        torch.ones(B, N, mcts.config.action_space_size, dtype=torch.int32, device=dev)
    torch_stream = isinstance(eps_uniforms, str)
    if torch_stream:
        if eps_uniforms != "torch":
            raise ValueError(f"eps_uniforms: {eps_uniforms!r} (a tuple of arrays or 'torch')")
        legal_host = np.ones((B, N, mcts.config.action_space_size), np.int64) if legal_actions_lst is None \
            else (legal_actions_lst.cpu().numpy() if isinstance(legal_actions_lst, torch.Tensor)
                  else np.asarray(legal_actions_lst))
        u_eps = torch.empty(N, B, dtype=torch.float32, device=dev)
        u_cat = torch.empty(N, B, dtype=torch.float64, device=dev)
    elif eps_uniforms is None:
        u_eps = torch.rand(N, B, dtype=torch.float32, device=dev)
        u_cat = torch.rand(N, B, dtype=torch.float64, device=dev)
    else:
        u_eps = torch.as_tensor(eps_uniforms[0], dtype=torch.float32).to(dev)
        u_cat = torch.as_tensor(eps_uniforms[1], dtype=torch.float64).to(dev)
    actions = torch.full((B, N), -1, dtype=torch.int32, device=dev)
    count_ent = torch.zeros(B, N, dtype=torch.float64, device=dev)
    outs = []
    for k in range(N):
        factor = actions[:, :k] if k > 0 else None
        out = mcts.batch_search_device(model, network_output, k, factor, N, legal_actions_lst, device,
                                       add_noise=True, sampled_tau=sampled_tau)
        outs.append(out)
        # select_action's np_random.choice: one double per root, in root order (:240-247)
        u = torch.from_numpy(_root_uniforms(mcts, B)).to(dev)
        if torch_stream:  # the agent's torch draws, root by root (:250-254)
            ue, uc = torch_eps_uniforms(legal_host[:, k, :])
            u_eps[k].copy_(torch.from_numpy(ue))
            u_cat[k].copy_(torch.from_numpy(uc))
        with torch.cuda.device(dev):
            _, act, ent = select_actions(out, u, temperature, deterministic=False)
            eps_greedy(out, act, legal[:, k, :], greedy_epsilon, u_eps[k], u_cat[k])  # :250-254
        actions[:, k] = act
        count_ent[:, k] = ent
    prob = torch.ones(B, dtype=torch.float64, device=dev)
    vent = torch.zeros(B, N, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        for k in range(N):  # :278-290
            a = actions[:, k].contiguous()
            e = torch.empty(B, dtype=torch.float64, device=dev)
            marginal_policy(outs[k], MZ_MARGINAL_GIVEN, a, prob, entropy=e)
            vent[:, k] = e
    return SelfPlayDecisions(actions, count_ent, prob, vent, outs[0].value, outs)


class ReanalyzePolicy(NamedTuple):
    """The targets of reanalyze_worker.py:345-366 (device tensors)."""

    sampled_actions: torch.Tensor   # int32 [B', 1, N]
    sampled_policies: torch.Tensor  # float32 [B', 1]
    sampled_imp_ratio: torch.Tensor  # float32 [B', 1] (ones)
    sampled_masks: torch.Tensor     # bool [B', 1]
    sampled_qvalues: torch.Tensor   # float32 [B', 1]: agent 0's root value
    root_mcts_values: torch.Tensor  # float32 [B', 1]
    root_pred_values: torch.Tensor  # network_output.value as [B', 1]


def reanalyze_policy_targets(mcts, model, network_output, legal_actions_lst, policy_mask, device=None,
                             _first=None) -> ReanalyzePolicy:
    """`_prepare_policy_re` after the initial inference (reanalyze_worker.py:266-366): per agent
    a search (add_noise=True, sampled_tau=1.0) conditioned on the earlier agents' chosen actions,
    action = argmax(marginal visits * legal), and the product of the agents' marginal
    distributions at the chosen actions.  Requires num_simulations >= 1: with no visits the
    reference draws the action from np_random instead.
    (`_first` = (out, lo, hi, legal): agent 0's search already ran as rows [lo, hi) of the merged search
    `out`, whose rows have the agent-0 legal actions `legal`: reanalyze_batch_targets.)"""
    if mcts.config.num_simulations < 1:
        raise ValueError("reanalyze_policy_targets needs num_simulations >= 1")
    hidden = network_output.hidden_state
    dev = hidden.device
    B = hidden.shape[0]
    legal_np = np.asarray(legal_actions_lst)
    N = legal_np.shape[1]
    legal = _dev_i32(legal_np, dev)
    current = torch.zeros(B, N, dtype=torch.int32, device=dev)
    prob = torch.ones(B, dtype=torch.float64, device=dev)
    value0 = None
    for k in range(N):
        factor = current[:, :k] if k > 0 else None
        if k == 0 and _first is not None:
            # the kernel runs over the merged handle's rows; this search's are sliced out (rows are
            # independent: its own rows get what a launch over them alone writes)
            whole, lo, hi, legal_whole = _first
            value0 = whole.value[lo:hi].reshape(B, 1)
            rows = whole.value.shape[0]
            a_whole = torch.empty(rows, dtype=torch.int32, device=dev)
            prob_whole = torch.ones(rows, dtype=torch.float64, device=dev)
            with torch.cuda.device(dev):
                marginal_policy(whole, MZ_MARGINAL_ARGMAX, a_whole, prob_whole, legal=legal_whole)
            current[:, 0] = a_whole[lo:hi]
            prob = prob_whole[lo:hi].clone()
            continue
        out = mcts.batch_search_device(model, network_output, k, factor, N, legal_np, device, add_noise=True,
                                       sampled_tau=1.0)
        if k == 0:
            value0 = out.value.reshape(B, 1)
        a = torch.empty(B, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            marginal_policy(out, MZ_MARGINAL_ARGMAX, a, prob, legal=legal[:, k, :])
        current[:, k] = a
    masks = torch.as_tensor(np.asarray(policy_mask).reshape(B, 1).astype(np.bool_)).to(dev)
    pv = network_output.value
    pv = torch.as_tensor(pv).to(dev)
    if pv.ndim == 1:
        pv = pv.reshape(B, 1)
    return ReanalyzePolicy(current.reshape(B, 1, N), prob.to(torch.float32).reshape(B, 1),
                           torch.ones(B, 1, dtype=torch.float32, device=dev), masks, value0, value0, pv)


def agent_wavefront(G: int, N: int) -> List[List[Tuple[int, int]]]:
    """The order in which the N dependent agent searches of G independent batches can run merged: tick t
    holds every (batch g, agent k) with k = t - g and 0 <= k < N, in ascending g.  Agent k of a batch needs
    the actions of that batch's agents before k (reanalyze_worker.py:278-317) and nothing of another
    batch, so the N x G grid has dependencies along one axis only: (g, k - 1) lies one tick before (g, k),
    no tick holds a batch twice, and G + N - 1 ticks replace G * N searches."""
    G, N = int(G), int(N)
    if G < 1 or N < 1:
        raise ValueError(f"agent_wavefront: {G} batches of {N} agents")
    return [[(g, t - g) for g in range(G) if 0 <= t - g < N] for t in range(G + N - 1)]


def reanalyze_policy_targets_many(mcts, model, network_outputs: list, legal_actions_lsts: list, policy_masks: list,
                                  device=None) -> List[ReanalyzePolicy]:
    """`reanalyze_policy_targets` of G batches, their agent searches run as a wavefront (agent_wavefront):
    one merged search per tick over entries of different agents (SampledMCTS.batch_search_many_device on a
    `mixed_agents` driver) and one mz_marginal_policy launch over its rows.  Entry g equals, all seven
    fields and bit for bit, the g-th of the consecutive calls `reanalyze_policy_targets(mcts, model,
    network_outputs[g], legal_actions_lsts[g], policy_masks[g], device)` under batch_search_many's
    condition, and `np_random` ends in the state those calls leave: every search's draws are made first,
    in the reference's order (batch 0's agents 0 .. N - 1, then batch 1's), and handed to the ticks.
    Requires `mixed_agents=True` and num_simulations >= 1; a `root_shard` driver is refused; a
    `root_capacity` must hold the largest tick.  All refusals come before anything is drawn."""
    if mcts.config.num_simulations < 1:
        raise ValueError("reanalyze_policy_targets_many needs num_simulations >= 1")
    if not getattr(mcts, "mixed_agents", False):
        raise ValueError("reanalyze_policy_targets_many needs a SampledMCTS with mixed_agents=True (a tick "
                         "merges searches of different agents)")
    if mcts.root_shard is not None:
        raise ValueError(f"reanalyze_policy_targets_many with root_shard={mcts.root_shard}: merged searches across "
                         "root shards are not supported")
    G = len(network_outputs)
    if G < 1 or len(legal_actions_lsts) != G or len(policy_masks) != G:
        raise ValueError(f"reanalyze_policy_targets_many: {G} batches, {len(legal_actions_lsts)} legal-action "
                         f"arrays and {len(policy_masks)} masks")
    legal_np = [np.asarray(la) for la in legal_actions_lsts]
    N = legal_np[0].shape[1]
    sizes = [int(o.hidden_state.shape[0]) for o in network_outputs]
    if any(la.ndim != 3 or la.shape[:2] != (b, N) for la, b in zip(legal_np, sizes)):
        raise ValueError(f"reanalyze_policy_targets_many: legal actions of shapes {[la.shape for la in legal_np]} "
                         f"for batches of {sizes} roots and {N} agents")
    ticks = agent_wavefront(G, N)
    largest = max(sum(sizes[g] for g, _ in tick) for tick in ticks)
    if mcts.root_capacity is not None and largest > mcts.root_capacity:
        raise ValueError(f"the largest tick holds {largest} roots, more than root_capacity={mcts.root_capacity}")
    dev = network_outputs[0].hidden_state.device
    draws = [[mcts.draw_search(b) for _ in range(N)] for b in sizes]  # the reference's order
    legal = [_dev_i32(la, dev) for la in legal_np]
    current = [torch.zeros(b, N, dtype=torch.int32, device=dev) for b in sizes]
    prob = [torch.ones(b, dtype=torch.float64, device=dev) for b in sizes]
    value0 = [None] * G
    for tick in ticks:
        whole, bounds = mcts.batch_search_many_device(
            model, [network_outputs[g] for g, _ in tick], [k for _, k in tick],
            [current[g][:, :k] if k > 0 else None for g, k in tick], N, [legal_np[g] for g, _ in tick], device,
            add_noise=True, sampled_tau=1.0, draws=[draws[g][k] for g, k in tick])
        # one launch over the merged rows: each row's legal actions are its own agent's, its running
        # product its batch's (rows are independent: an entry's rows get what a launch over them alone writes)
        legal_rows = torch.cat([legal[g][:, k, :] for g, k in tick], 0)
        prob_rows = torch.cat([prob[g] for g, _ in tick], 0)
        a = torch.empty(bounds[-1], dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            marginal_policy(whole, MZ_MARGINAL_ARGMAX, a, prob_rows, legal=legal_rows)
        for (g, k), lo, hi in zip(tick, bounds[:-1], bounds[1:]):
            current[g][:, k] = a[lo:hi]
            prob[g] = prob_rows[lo:hi]
            if k == 0:
                value0[g] = whole.value[lo:hi].reshape(sizes[g], 1)
    res = []
    for g, b in enumerate(sizes):
        masks = torch.as_tensor(np.asarray(policy_masks[g]).reshape(b, 1).astype(np.bool_)).to(dev)
        pv = torch.as_tensor(network_outputs[g].value).to(dev)
        if pv.ndim == 1:
            pv = pv.reshape(b, 1)
        res.append(ReanalyzePolicy(current[g].reshape(b, 1, N), prob[g].to(torch.float32).reshape(b, 1),
                                   torch.ones(b, 1, dtype=torch.float32, device=dev), masks, value0[g], value0[g], pv))
    return res


class GameReanalysis(NamedTuple):
    """What make_renalyze_update computes for the T = len(game) steps of one game
    (reanalyze_worker.py:515-596, :604-607), as device tensors."""

    actions: torch.Tensor       # int32 [T, N]: the chosen joint actions
    policy_probs: torch.Tensor  # float32 [T, 1]: the probability of the chosen joint action
    root_values: torch.Tensor   # float32 [T, 1]: agent 0's search value
    pred_values: Optional[torch.Tensor]  # network_output.value, [T, 1] or [T] as given (None: another shape)


def _device_ctx(dev):
    return torch.cuda.device(dev) if torch.device(dev).type == "cuda" else contextlib.nullcontext()


def reanalyze_game(mcts, model, network_output, legal_actions_lst, device=None) -> GameReanalysis:
    """`make_renalyze_update` after its initial inference (reanalyze_worker.py:507-596) for the T steps
    of one game: per agent turn a search of the T roots (add_noise=True, sampled_tau=1.0) conditioned on
    the earlier agents' chosen actions on the device, then the action argmax(marginal visits * legal)
    (MZ_MARGINAL_ARGMAX_LEGAL).  A root whose visits all lie on illegal actions comes back -1 and is
    resolved on the host as the reference does (:568-570), in root order and before the next agent's
    search: `np_random.choice(np.where(legal_row == 1)[0])`, or 0 when no action is legal; this is the
    one small device-to-host read of the action column per agent.  After the last agent the probability
    of the chosen joint action is the running float64 product of the agents' marginal visit
    distributions at their actions (:587-596), stored as float32.  Requires num_simulations >= 1.

    On a `SampledMCTS(root_capacity >= max_moves)` games of every length share one set of recorded
    loops."""
    if mcts.config.num_simulations < 1:
        raise ValueError("reanalyze_game needs num_simulations >= 1")
    hidden = network_output.hidden_state
    dev = hidden.device
    T = hidden.shape[0]
    legal_np = legal_actions_lst.cpu().numpy() if isinstance(legal_actions_lst, torch.Tensor) \
        else np.asarray(legal_actions_lst)
    N = legal_np.shape[1]
    legal = _dev_i32(legal_np, dev)
    current = torch.zeros(T, N, dtype=torch.int32, device=dev)
    outs, value0 = [], None
    for k in range(N):
        factor = current[:, :k] if k > 0 else None
        out = mcts.batch_search_device(model, network_output, k, factor, N, legal_np, device, add_noise=True,
                                       sampled_tau=1.0)
        outs.append(out)
        if k == 0:
            value0 = out.value.reshape(T, 1)
        a = torch.empty(T, dtype=torch.int32, device=dev)
        with _device_ctx(dev):
            marginal_policy(out, MZ_MARGINAL_ARGMAX_LEGAL, a, None, legal=legal[:, k, :])
        a_host = a.cpu().numpy()
        missing = np.flatnonzero(a_host < 0)
        if missing.size:  # :568-570, in root order
            a_host = a_host.copy()
            for i in missing:
                options = np.flatnonzero(legal_np[i, k, :] == 1)
                a_host[i] = mcts.np_random.choice(options) if options.size else 0
            a.copy_(torch.from_numpy(a_host))
        current[:, k] = a
    prob = torch.ones(T, dtype=torch.float64, device=dev)
    with _device_ctx(dev):
        for k in range(N):  # :587-596, agent order
            marginal_policy(outs[k], MZ_MARGINAL_GIVEN, current[:, k].contiguous(), prob)
    pv = torch.as_tensor(network_output.value).to(dev)
    if not ((pv.ndim == 2 and pv.shape[1] == 1) or pv.ndim == 1):
        pv = None  # (the reference leaves game.pred_values as they are, :608-609)
    return GameReanalysis(current, prob.to(torch.float32).reshape(T, 1), value0, pv)


def write_game(game, result: GameReanalysis, model_index: int):
    """Store a `reanalyze_game` result on `game` (any object with these attributes) in the per-step list
    form the reference's replay code reads (reanalyze_worker.py:598-607): one entry per step, each a view
    of the result's row.  Returns `game`."""
    actions = result.actions.cpu().numpy()
    T, N = actions.shape
    probs = result.policy_probs.cpu().numpy().reshape(T, 1)
    values = result.root_values.cpu().numpy().reshape(T, 1)
    game.model_indices = np.full(T, model_index)
    game.sampled_actions = list(actions.reshape(T, 1, N))       # [1, N] each
    game.sampled_policies = list(probs)                         # [1] each
    game.sampled_padding_masks = list(np.ones((T, 1), np.bool_))
    game.sampled_qvalues = list(values)
    game.root_values = list(values[:, 0])                       # scalars
    if result.pred_values is not None:
        pred = result.pred_values.cpu().numpy()
        game.pred_values = list(pred[:, 0]) if pred.ndim == 2 else pred.tolist()
    return game


# ------------------------------------------------------------------------------------------------
# reanalyze batch targets: value, reward, advantage (core/reanalyze_worker.py:376-489, make_batch)
# ------------------------------------------------------------------------------------------------
def _stream_args(tb, dev):
    """(library, handle, stream) of a launch: the tree handle's stream, or torch's current one."""
    if tb is not None:
        return tb._lib, tb._h, None
    from ._lib import load
    from .cytree import _raw_stream_of

    return load(), None, C.c_void_p(_raw_stream_of(dev.index if dev.index is not None else torch.cuda.current_device()))


def _padded_rows(rows, what: str) -> Tuple[np.ndarray, np.ndarray]:
    """Per-trajectory sequences -> ([G, L] array of their common float dtype, lengths int32 [G]).
    float32 stays float32 (numpy's scalar promotion depends on it); everything else is float64."""
    arrs = [np.asarray(r).reshape(-1) for r in rows]
    kinds = {a.dtype for a in arrs if a.size}
    dtype = np.float32 if kinds == {np.dtype(np.float32)} else np.float64
    if dtype is np.float64 and np.dtype(np.float32) in kinds:
        raise ValueError(f"{what}: float32 and other dtypes mixed across trajectories")
    lens = np.array([a.shape[0] for a in arrs], np.int32)
    out = np.zeros((len(arrs), max(1, int(lens.max(initial=0)))), dtype)
    for g, a in enumerate(arrs):
        out[g, : lens[g]] = a
    return out, lens


class _TargetInputs(NamedTuple):
    G: int
    U: int
    td: np.ndarray
    td_max: int
    dev_args: tuple  # td, pos, traj_len, reward_len, rewards, dpow, dpow32 (device tensors)
    rewards_f32: bool
    L: int


def _target_inputs(rewards, pos, traj_len, td_steps, discount, num_unroll_steps, td_max, dev) -> _TargetInputs:
    rew, rlen = _padded_rows(rewards, "rewards")
    G, L = rew.shape
    pos = np.asarray(pos, np.int64).reshape(-1)
    tl = np.asarray(traj_len, np.int64).reshape(-1)
    td = np.asarray(td_steps, np.int64).reshape(-1)
    if td.shape[0] == 1 and G > 1:
        td = np.repeat(td, G)
    if not (pos.shape[0] == tl.shape[0] == td.shape[0] == G):
        raise ValueError(f"rewards, pos, traj_len, td_steps must describe the same {G} trajectories")
    if (rlen < tl).any():
        raise ValueError("reward_len < traj_len: a trajectory holds fewer rewards than steps")
    if (pos < 0).any() or (tl < 0).any() or (td < 0).any():
        raise ValueError("pos, traj_len and td_steps must be >= 0")
    td_max = int(td.max()) if td_max is None else int(td_max)
    td_max = max(td_max, 1)
    if (td > td_max).any():
        raise ValueError(f"td_steps above td_max = {td_max}")
    dpow = np.array([float(discount) ** i for i in range(td_max)], np.float64)  # Python's own power
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    dev_args = (t(td.astype(np.int32)), t(pos.astype(np.int32)), t(tl.astype(np.int32)), t(rlen), t(rew), t(dpow),
                t(dpow.astype(np.float32)))
    return _TargetInputs(G, int(num_unroll_steps), td, td_max, dev_args, rew.dtype == np.float32, L)


def _launch_value_targets(tb, dev, mode, ti: _TargetInputs, lo, hi, value, td_pow, stored, stored_f32):
    n = hi - lo
    out_v = torch.empty(n, dtype=torch.float64, device=dev)
    out_r = torch.empty(n, dtype=torch.float64, device=dev)
    td, pos, tl, rlen, rew, dpow, dpow32 = ti.dev_args
    lib, h, stream = _stream_args(tb, dev)
    with torch.cuda.device(dev):
        check(lib, lib.mz_value_targets(h, stream, int(mode), int(lo), int(n), ti.G, ti.U, _p(value), _p(td_pow),
                                        _p(td), _p(pos), _p(tl), _p(rlen), _p(rew), int(ti.rewards_f32), _p(stored),
                                        int(stored_f32), ti.L, _p(dpow), _p(dpow32), ti.td_max, _p(out_v), _p(out_r)),
              "value_targets")
    return out_r, out_v


def _rows_of(rows, total):
    lo, hi = (0, total) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= lo < hi <= total:
        raise ValueError(f"rows {rows} outside the batch's {total} rows")
    return lo, hi


def reanalyze_value_targets(mcts, model, network_output, legal_actions_lst, *, rewards, pos, traj_len, td_steps,
                            discount: float, num_unroll_steps: int, td_max: Optional[int] = None,
                            use_root_value: bool = True, use_pred_value: bool = False, rows=None, device=None,
                            _search=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`_prepare_reward_value_re` after the initial inference (reanalyze_worker.py:116-164) ->
    (batch_rewards, batch_values), float64 [G, U+1] device tensors.

    `network_output` is the inference on the bootstrap observations of the G * (U+1) rows (row
    j = g * (U+1) + k, :90-103) and `legal_actions_lst` their legal actions.  With `use_root_value`
    the agent-0 search of :121-129 runs here (add_noise=True, sampled_tau=1.0, factor=None;
    `mcts.np_random` is consumed as the reference consumes `self.np_random`) and its
    `DeviceSearchOutput.value` feeds the kernel in the search's stream, without a host copy; with
    `use_pred_value` the kernel takes `network_output.value` (mcts, model, legal_actions_lst unused).

    rewards: per trajectory, `game.rewards` (all float64 / Python floats, or all float32: the
    reference's arithmetic depends on it, include/mzconsume.h); pos, traj_len: `game_pos_lst`,
    `len(game)`; td_steps: per trajectory, after the clip of :82-84 (`td_max` defaults to their
    maximum; pass config.td_steps to keep one table size).

    rows = (lo, hi): `network_output` holds rows [lo, hi) only (a rank's share, with `mcts` built
    for that root shard); the result is then flat, float64 [hi - lo] each.
    (`_search` = (out, lo, hi): the agent-0 search already ran as rows [lo, hi) of the merged search `out`:
    reanalyze_batch_targets.)"""
    U = int(num_unroll_steps)
    hidden = network_output.hidden_state
    dev = hidden.device if isinstance(hidden, torch.Tensor) and hidden.is_cuda else torch.device(device or "cuda")
    ti = _target_inputs(rewards, pos, traj_len, td_steps, discount, U, td_max, dev)
    total = ti.G * (U + 1)
    lo, hi = _rows_of(rows, total)
    n = hi - lo
    # :138 on the whole batch's list, exactly the reference's expression (numpy's array power)
    td_steps_lst = [np.intc(x) for x in np.repeat(ti.td, U + 1)]
    td_pow = torch.from_numpy(np.ascontiguousarray(np.power(discount, td_steps_lst)[lo:hi], dtype=np.float64)).to(dev)
    tb = None
    if use_root_value and _search is not None:
        tb = _tree(_search[0])
        value = _search[0].value[_search[1]:_search[2]].reshape(-1)  # (a contiguous row range: no copy)
    elif use_root_value:
        legal_np = np.asarray(legal_actions_lst)
        out = mcts.batch_search_device(model, network_output, 0, None, legal_np.shape[1], legal_np, device,
                                       add_noise=True, sampled_tau=1.0)
        tb = _tree(out)
        value = out.value.reshape(-1)
    elif use_pred_value:
        value = torch.as_tensor(network_output.value).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    else:
        raise NotImplementedError  # as the reference, :134-135
    if value.shape[0] != n:
        raise ValueError(f"{value.shape[0]} values for {n} rows")
    r, v = _launch_value_targets(tb, dev, MZ_VALUE_RE, ti, lo, hi, value, td_pow, None, False)
    return (r, v) if rows is not None else (r.reshape(ti.G, U + 1), v.reshape(ti.G, U + 1))


def reanalyze_batch_targets(mcts, model, value_output, value_legal, policy_output, policy_legal, policy_mask, *,
                            rewards, pos, traj_len, td_steps, discount: float, num_unroll_steps: int,
                            td_max: Optional[int] = None, rows=None, device=None
                            ) -> Tuple[torch.Tensor, torch.Tensor, ReanalyzePolicy]:
    """A reanalyze batch's targets, make_batch of core/reanalyze_worker.py: `reanalyze_value_targets(mcts,
    model, value_output, value_legal, ...)` followed by `reanalyze_policy_targets(mcts, model,
    policy_output, policy_legal, policy_mask)` -> (batch_rewards, batch_values, ReanalyzePolicy), with the
    value search (:121-129) and the first policy search (:284-294) -- both agent 0, factor None,
    add_noise=True, sampled_tau=1.0, on other observations -- run as one
    `mcts.batch_search_many_device`: one search latency less per batch.  The outputs and the state of
    `mcts.np_random` equal those of the two calls made one after the other, on the guarantee of
    SampledMCTS.batch_search_many.  mz_value_targets reads the value segment's rows of the merged output;
    mz_marginal_policy runs over the handle's rows and the policy segment is sliced out; the later
    agents' searches are those of reanalyze_policy_targets."""
    if mcts.config.num_simulations < 1:
        raise ValueError("reanalyze_batch_targets needs num_simulations >= 1")
    vl, pl = np.asarray(value_legal), np.asarray(policy_legal)
    N = pl.shape[1]
    whole, bounds = mcts.batch_search_many_device(model, [value_output, policy_output], 0, [None, None], N,
                                                  [vl, pl], device, add_noise=True, sampled_tau=1.0)
    dev = whole.value.device
    r, v = reanalyze_value_targets(mcts, model, value_output, vl, rewards=rewards, pos=pos, traj_len=traj_len,
                                   td_steps=td_steps, discount=discount, num_unroll_steps=num_unroll_steps,
                                   td_max=td_max, use_root_value=True, rows=rows, device=device,
                                   _search=(whole, bounds[0], bounds[1]))
    legal_whole = torch.cat([_dev_i32(vl[:, 0, :], dev), _dev_i32(pl[:, 0, :], dev)], 0)
    pol = reanalyze_policy_targets(mcts, model, policy_output, pl, policy_mask, device,
                                   _first=(whole, bounds[1], bounds[2], legal_whole))
    return r, v, pol


def value_targets_non_re(rewards, stored, pos, traj_len, *, td_steps: int, discount: float, num_unroll_steps: int,
                         rows=None, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`_prepare_reward_value_non_re` (reanalyze_worker.py:166-210) -> (batch_rewards,
    batch_values), float64 [G, U+1] device tensors, in torch's current stream.  stored: per
    trajectory, `game.root_values` (use_root_value) or `game.pred_values` (use_pred_value), all
    float32 or all float64 like `rewards`; td_steps: config.td_steps."""
    dev = torch.device(device or "cuda")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    U = int(num_unroll_steps)
    ti = _target_inputs(rewards, pos, traj_len, [int(td_steps)], discount, U, int(td_steps), dev)
    st, slen = _padded_rows(stored, "stored")
    if st.shape[0] != ti.G or (slen < np.asarray(traj_len).reshape(-1)).any():
        raise ValueError("stored values must cover every step of every trajectory")
    st_full = np.zeros((ti.G, ti.L), st.dtype)  # the rewards' row stride
    w = min(ti.L, st.shape[1])
    st_full[:, :w] = st[:, :w]
    lo, hi = _rows_of(rows, ti.G * (U + 1))
    r, v = _launch_value_targets(None, dev, MZ_VALUE_NON_RE, ti, lo, hi, None, None,
                                 torch.from_numpy(st_full).to(dev), st.dtype == np.float32)
    return (r, v) if rows is not None else (r.reshape(ti.G, U + 1), v.reshape(ti.G, U + 1))


def pairwise_plan(n: int, lib=None) -> Tuple[np.ndarray, np.ndarray]:
    """numpy's float64 pairwise sum of n elements as (leaf starts [leaves + 1], postfix ops), the
    plan mz_normalize_advantage sums by (include/mzconsume.h mz_pairwise_plan; no device call)."""
    if lib is None:
        from ._lib import load

        lib = load()
    cap = 1024
    starts = (C.c_int32 * (cap + 1))()
    ops = (C.c_int32 * (2 * cap))()
    nl, nops = C.c_int32(), C.c_int32()
    check(lib, lib.mz_pairwise_plan(int(n), starts, ops, cap, C.byref(nl), C.byref(nops)), "pairwise_plan")
    return np.array(starts[: nl.value + 1], np.int32), np.array(ops[: nops.value], np.int32)


def normalize_advantage(q: torch.Tensor, pred: torch.Tensor, mask: torch.Tensor, out: DeviceSearchOutput = None
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Step (6) of make_batch (reanalyze_worker.py:466-473) on the gathered batch: q =
    batch_sampled_qvalues, pred = batch_root_pred_values (float32), mask = batch_sampled_masks ->
    (batch_sampled_adv float64, q's shape; float64 [2] = adv_mean, adv_std), numpy's nanmean /
    nanstd bit for bit.  The statistics span the whole batch: gather the ranks' rows first (this
    call is not sharded).  Runs in torch's current stream, or in `out`'s tree's when given.  At
    most 65,536 entries; the first call for a size must be outside any graph capture."""
    dev = q.device
    qf = q.to(torch.float32).reshape(-1).contiguous()
    pf = torch.as_tensor(pred).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    mf = torch.as_tensor(mask).to(device=dev).reshape(-1).ne(0).to(torch.uint8).contiguous()
    n = qf.shape[0]
    if pf.shape[0] != n or mf.shape[0] != n:
        raise ValueError("q, pred and mask must have the same number of entries")
    adv = torch.empty(n, dtype=torch.float64, device=dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    lib, h, stream = _stream_args(_tree(out) if out is not None else None, dev)
    with torch.cuda.device(dev):
        check(lib, lib.mz_normalize_advantage(h, stream, _p(qf), _p(pf), _p(mf), int(n), _p(adv), _p(stats)),
              "normalize_advantage")
    return adv.reshape(q.shape), stats
