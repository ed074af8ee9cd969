"""Host restatement of the joint search (test infrastructure only): the checker of
`mazero_amd.mcts_sampled.SampledMCTS.batch_search_joint` and of `mazero_amd.consume.select_joint_actions`.

`JointOracleSampledMCTS.batch_search_joint` is the reference driver
(core/mcts/tree_search/mcts_sampled.py:34-200) as oracle/driver.py restates it -- numpy glue on the
host, a Python-list hidden-state pool with `torch.vstack` gathers, the model's eval-mode
`recurrent_inference`, three tree calls per simulation on an oracle tree library through the
`Tree_batch` shim -- with exactly these changes, the call of core/test.py:84:

    :53      num_agents = N = network_output.policy_logits.shape[1]
    :60-62   the policy logits are the whole [B, N, A] array, no current-agent slice
    :68      noises = np_random.dirichlet([alpha] * A, (B, N)), drawn before the tree seed (:89)
    :74      the legal mask is the whole legal_actions_lst [B, N, A]
    :89      Tree_batch(B, N, A, K, ...)
    :116-121, :136-147 are gone (no factor, no prediction pass for later agents)
    :123-124 batch_selection returns batch_actions [B, N], and :151 hands them to recurrent_inference
    :156     all agents' logits, [B, N, A]

Everything else is line for line, the order in which `np_random` is consumed included.
`select_joint_actions_host` is core/test.py:101-107 over such a result (select_action as
oracle/consume.py restates it, then the row gather)."""
from __future__ import annotations

import numpy as np
import torch


def _np(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


class JointOracleSampledMCTS:
    def __init__(self, config, np_random, tree_lib, root_shard=None):
        self.config = config
        self.np_random = np_random
        self.lib = tree_lib
        self.trace = []  # per simulation: (idx_x, idy, actions [B, N]) of the selection
        self.root_shard = root_shard  # (lo, hi, total), as oracle/driver.py (CPU port only)

    def _rows(self, draw, B):
        if self.root_shard is None:
            return draw(B)
        lo, hi, total = self.root_shard
        assert hi - lo == B
        return draw(total)[lo:hi]

    def batch_search_joint(self, model, network_output, legal_actions_lst=None, device=None, add_noise=False,
                           sampled_tau=1.0):
        from mazero_amd.cytree import Tree_batch

        cfg = self.config
        c2, c1, disc = cfg.pb_c_base, cfg.pb_c_init, cfg.discount
        rho, lam = cfg.mcts_rho, cfg.mcts_lambda
        alpha, eps = cfg.root_dirichlet_alpha, cfg.root_exploration_fraction
        A, K = cfg.action_space_size, cfg.sampled_action_times
        B = network_output.hidden_state.shape[0]
        N = network_output.policy_logits.shape[1]

        # mcts_sampled.py:57-83
        hs0 = network_output.hidden_state
        rewards = _np(network_output.reward)
        values = _np(network_output.value)
        logits = _np(network_output.policy_logits)
        assert logits.shape == (B, N, A)
        probs = np.exp(logits - np.max(logits, axis=-1, keepdims=True))
        probs = probs / np.sum(probs, axis=-1, keepdims=True)
        noises = self._rows(lambda n: self.np_random.dirichlet([alpha] * A, (n, N)), B).astype(np.float32)
        if not add_noise:
            eps = 0.0
        if legal_actions_lst is not None:
            legal = legal_actions_lst
            probs *= legal
            probs += legal * 1e-4
            probs = probs / np.sum(probs, axis=-1, keepdims=True)
            noises *= legal
            noises += legal * 1e-4
            noises = noises / np.sum(noises, axis=-1, keepdims=True)

        # mcts_sampled.py:86-106
        pool = [hs0]
        trees = Tree_batch(B, N, A, K, cfg.num_simulations, cfg.tree_value_stat_delta_lb,
                           self.np_random.choice(256), rho, lam, lib=self.lib,
                           root_offset=0 if self.root_shard is None else self.root_shard[0])
        beta = probs * (1 - eps) + noises * eps
        beta = beta ** (1 / sampled_tau)
        if legal_actions_lst is not None:
            beta *= legal
        beta = beta / np.sum(beta, axis=-1, keepdims=True)
        trees.prepare(rewards.reshape(B).astype(np.float32), values.reshape(B).astype(np.float32),
                      probs.astype(np.float32), beta.astype(np.float32), K, eps, noises)

        # mcts_sampled.py:111-172
        self.trace = []
        with torch.no_grad():
            model.eval()
            for s in range(cfg.num_simulations):
                ix, iy, acts = trees.batch_selection(c2, c1, disc)
                self.trace.append((np.asarray(ix, np.int32), np.asarray(iy, np.int32),
                                   np.asarray(acts, np.int32).reshape(B, N).copy()))
                leaf = torch.vstack([pool[x][y] for x, y in zip(ix, iy)])
                joint_t = torch.from_numpy(np.asarray(acts).reshape(B, N)).to(leaf.device)
                with torch.autocast("cuda", enabled=leaf.is_cuda):
                    out = model.recurrent_inference(leaf, joint_t)
                lg = out.policy_logits
                p = np.exp(lg - np.max(lg, axis=-1, keepdims=True))
                p = p / np.sum(p, axis=-1, keepdims=True)
                bt = p ** (1 / sampled_tau)
                bt = bt / np.sum(bt, axis=-1, keepdims=True)
                pool.append(out.hidden_state)
                r = out.reward.reshape(B).astype(np.float32)
                v = out.value.reshape(B).astype(np.float32)
                trees.batch_expansion_and_backup(s + 1, disc, K, r, v, p.astype(np.float32), bt.astype(np.float32))

        # mcts_sampled.py:176-200
        return dict(
            value=trees.get_roots_values(),
            marginal_visit_count=trees.get_roots_marginal_visit_count(),
            marginal_priors=trees.get_roots_marginal_priors(),
            sampled_actions=trees.get_roots_sampled_actions(),
            sampled_visit_count=trees.get_roots_sampled_visit_count(),
            sampled_pred_probs=trees.get_roots_sampled_pred_probs(),
            sampled_beta=trees.get_roots_sampled_beta(),
            sampled_beta_hat=trees.get_roots_sampled_beta_hat(),
            sampled_priors=trees.get_roots_sampled_priors(),
            sampled_imp_ratio=trees.get_roots_sampled_imp_ratio(),
            sampled_pred_values=trees.get_roots_sampled_pred_values(),
            sampled_mcts_values=trees.get_roots_sampled_mcts_values(),
            sampled_rewards=trees.get_roots_sampled_rewards(),
            sampled_qvalues=trees.get_roots_sampled_qvalues(disc),
        )


def select_position_host(visit_counts, temperature=1.0, deterministic=True, uniform=None):
    """select_action (core/utils.py:289-316) on one root's visit counts, its np_random.choice draw
    given as the double `uniform` -> (action_pos, count entropy in bits).  The sums are Python's
    left-to-right sums; the draw is what numpy's choice(n, p=probs) does with its one double: cumsum,
    / cdf[-1], searchsorted(side='right')."""
    from scipy.stats import entropy

    assert sum(visit_counts) > 0
    action_probs = [v ** (1 / temperature) for v in visit_counts]
    total = sum(action_probs)
    action_probs = np.array([x / total for x in action_probs])
    if deterministic:
        pos = int(np.argmax([v for v in visit_counts]))
    else:
        cdf = action_probs.cumsum()
        cdf /= cdf[-1]
        pos = int(cdf.searchsorted(uniform, side="right"))
    return pos, float(entropy(action_probs, base=2))


def select_joint_actions_host(sampled_actions, sampled_visit_count, temperature=1.0, deterministic=True,
                              uniforms=None):
    """core/test.py:101-107 at every root: (actions int32 [B, N], pos int32 [B], entropy float64 [B]);
    a root without children or visits gets -1 (and a NaN entropy), as the device consumer reports it."""
    B = len(sampled_actions)
    N = sampled_actions[0].shape[1]
    acts = np.full((B, N), -1, np.int32)
    pos = np.full(B, -1, np.int32)
    ent = np.full(B, np.nan)
    for i in range(B):
        v = sampled_visit_count[i]
        if len(v) == 0 or int(np.sum(v)) <= 0:
            continue
        pos[i], ent[i] = select_position_host(v, temperature, deterministic,
                                              None if uniforms is None else float(uniforms[i]))
        acts[i] = sampled_actions[i][pos[i]]
    return acts, pos, ent
