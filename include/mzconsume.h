/*
 * mzconsume.h — C-ABI of the on-device consumers of the search output.
 *
 * After each agent's search the reference workers pull every root's result to the host and make
 * their decisions per root in Python:
 *   - self-play: select_action over the root children's visit counts (core/utils.py:289-316),
 *     then eps_greedy_action (core/utils.py:319-334), then the stored policy probability and the
 *     visit entropy from the marginal visit counts (core/selfplay_worker.py:228-293);
 *   - reanalyze: the action argmax(marginal visits * legal mask) and the product of the agents'
 *     marginal visit distributions at the chosen actions (core/reanalyze_worker.py:296-332).
 * These entry points make the same decisions on the device, one lane per root, reading the padded
 * device results of mz_get_roots_sampled_padded / mz_get_roots_marginal_visit_count, in the
 * stream of a tree handle (mzmcts.h).  Random draws are inputs: the caller draws them on the host
 * from the same generator, in the same order as the reference (see each function).
 *
 * Integer and index results are exact; the float64 probabilities are the reference's own
 * operation sequence (Python sum, numpy cumsum, IEEE division), so they are bit-identical too.
 * The entropies use the device log and are within 1e-12 (relative) of scipy / numpy.
 * The reanalyze batch's value / reward targets and normalised advantages (the last section) follow
 * the same rule and are bit-identical to the reference's numpy arithmetic.
 *
 * Exported only by the product library (mazero_amd/_build/libmzmcts.so); device memory only.
 *
 * Active roots: in mz_select_actions, mz_eps_greedy and mz_marginal_policy, B below is the handle's
 * active-root count (mz_set_active_roots, include/mzdriver.h; root_num unless it was set): every
 * buffer holds B rows, lanes past B write nothing.
 */
#ifndef MZCONSUME_H
#define MZCONSUME_H

#include <stdint.h>

#include "mzmcts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* select_action(sampled_visit_count[i], temperature, deterministic, np_random)
 * (core/utils.py:289-316) for every root i, as the self-play worker calls it
 * (core/selfplay_worker.py:240-247), then agent_action = sampled_actions[pos, 0].
 *   degrees   int32 [B]              children of each root (mz_get_roots_sampled_padded)
 *   visits    int32 [B, width]       per-child visit counts, row i valid up to degrees[i]
 *   actions   int32 [B, width * N]   per-child joint actions (N = agent_num of the handle)
 *   uniforms  float64 [B]            np_random.random(B): the double each root's
 *                                    np_random.choice(len, p=probs) draws, in root order
 *                                    (ignored when deterministic)
 *   pos_out   int32 [B]   chosen child; action_out int32 [B] its action for agent 0;
 *   entropy_out float64 [B] scipy.stats.entropy(action_probs, base=2) (may be NULL).
 * probs = v ** (1 / temperature) / sum(...), where v ** e is Python's float power of an int, the
 * host libm's pow (mz_select_pow_plan below says which of the two ways a count takes):
 *   - e an integer in 1..8 and v ** e <= 2**53 (e = 1: every v; 2: v <= 94,906,265; 3: 208,063;
 *     4: 9,741; 5: 1,552; 6: 456; 7: 190; 8: 98): the repeated product in the kernel, whose every
 *     partial product is an integer below 2**53, hence exact and equal to pow.  The reference's
 *     schedule (1/temperature = 1, 2, 4; config.py:392-401) with counts in that range runs as it
 *     always did: no table, no upload.
 *   - every other count up to MZ_SELECT_POW_TABLE_MAX, for every other temperature and for e = 4..8
 *     past the bound: a table of pow((double)v, e) computed by the host's libm, uploaded on first use
 *     of an e on a device and kept (16 per process): make the first call for a temperature outside any
 *     stream capture (MZ_ERR_RUNTIME inside one).  The device pow is not used: it is not libm's, and
 *     with it the kernel chose another child than numpy at 18 to 447 of about 2,600 boundary draws in
 *     every class tried (1/temperature = 10; temperatures 0.3, 0.7, 1.5, 2.0; the table is in
 *     tests/test_consume_edges.py).
 * A root without children or without visits gets -1 (the reference asserts / draws from the
 * legal actions instead; neither happens after num_simulations >= 1).  So does a root of a degree
 * past `width`, a root holding a count that neither way covers (past the product's bound with e = 1..3,
 * past MZ_SELECT_POW_TABLE_MAX otherwise, or negative outside the product), and a root whose powers
 * sum to infinity: -1 in pos_out and action_out and a NaN entropy, never an inexact answer.
 * tests/test_consume_edges.py checks pos and action at every cdf entry and its two float64 neighbours
 * (1/temperature = 1..8 and 10, temperatures 0.3, 0.7, 1.5, 2.0, counts up to 3,000, and up to 20,000
 * at 0.25; rows of 1 to 255 children) against numpy's cumsum / searchsorted.
 * B = the handle's active roots (mz_set_active_roots): every buffer holds B rows. */
int mz_select_actions(mz_batch *b, const int32_t *degrees, const int32_t *visits, const int32_t *actions,
                      int width, double temperature, int deterministic, const double *uniforms, int32_t *pos_out,
                      int32_t *action_out, double *entropy_out);

/* mz_select_actions for a joint search (a handle of agent_num = N > 1, one search for all agents): the
 * same arguments, checks and arithmetic, and action_out is int32 [B, N], the chosen child's whole joint
 * action actions[i, pos * N .. pos * N + N) -- `roots_sampled_actions[i][action_pos]` of the reference's
 * evaluation loop (core/test.py:101-107, which calls select_action with deterministic=True).  A root
 * without children or visits gets -1 in pos_out and in every column of its action row.  With N = 1 the
 * results are those of mz_select_actions.  `width` is any row width >= 1 (one thread walks a root's
 * row): the 255 children per root of a wide joint handle (mz_create_wide_joint) included. */
int mz_select_actions_joint(mz_batch *b, const int32_t *degrees, const int32_t *visits, const int32_t *actions,
                            int width, double temperature, int deterministic, const double *uniforms,
                            int32_t *pos_out, int32_t *action_out, double *entropy_out);

/* The largest visit count of the host-made power table of mz_select_actions. */
#define MZ_SELECT_POW_TABLE_MAX 65535

/* How mz_select_actions computes v ** (1 / temperature) (host only: no device call):
 *   *ipow        the exponent of the in-kernel repeated product, 1..8, or 0 when 1/temperature is no
 *                integer in that range;
 *   *exact_max   the largest v the product is used for: the largest int32 v with v ** ipow <= 2**53,
 *                found in integer arithmetic from the exponent alone (-1 when *ipow == 0);
 *   *uses_table  1 when some count in 0..MZ_SELECT_POW_TABLE_MAX lies past exact_max, i.e. the call
 *                uploads the table; 0 otherwise (1/temperature = 1, 2, 3);
 *   table        (may be NULL) table_len <= MZ_SELECT_POW_TABLE_MAX + 1 doubles: table[v] = the
 *                uploaded table's entry, pow((double)v, 1 / temperature) by the host's libm. */
int mz_select_pow_plan(double temperature, int32_t *ipow, int32_t *exact_max, int32_t *uses_table, double *table,
                       int table_len);

/* eps_greedy_action(greedy, legal_mask, eps) (core/utils.py:319-334) for every root:
 *   action_io = (u_eps[i] < (float)eps) ? categorical(legal[i, :]; u_cat[i]) : action_io[i]
 * legal: int32 [B, A] (row stride legal_stride elements), the agent's legal-action weights;
 * categorical(w; u) = the first a with cumsum(w)[a] / sum(w) > u (float64), i.e. a draw from
 * torch.distributions.Categorical(w).  u_eps float32 [B], u_cat float64 [B] in [0, 1): the
 * reference draws them from torch's global generator per root; the caller supplies them (the same
 * distribution, not the same stream).  A root with no legal action keeps its greedy action.
 * B = the handle's active roots (mz_set_active_roots): every buffer holds B rows. */
int mz_eps_greedy(mz_batch *b, const int32_t *legal, int64_t legal_stride, float eps, const float *u_eps,
                  const double *u_cat, int32_t *action_io);

enum mz_marginal_mode {
    MZ_MARGINAL_GIVEN = 0,  /* self-play record: action given (core/selfplay_worker.py:278-290) */
    MZ_MARGINAL_ARGMAX = 1, /* reanalyze: action = argmax(marginal * legal) (reanalyze_worker.py:303-319) */
    MZ_MARGINAL_ARGMAX_LEGAL = 2, /* full-game reanalysis: the action alone (reanalyze_worker.py:563-570) */
};

/* One agent's marginal visit distribution dist = marginal / sum(marginal) (float64) at each root:
 *   MZ_MARGINAL_ARGMAX: action_io[i] = first argmax_a marginal[i, a] * legal[i, a] (int64 products);
 *   prob_io[i] *= dist[action_io[i]]  (the running product over agents; start it at 1.0);
 *   entropy_out[i] = -sum_a dist[a] * log(dist[a] + 1e-9)  (may be NULL).
 * When sum(marginal) == 0 (only with num_simulations == 0): GIVEN multiplies by 1/A and reports
 * entropy 0 (as the self-play worker); ARGMAX writes action -1 and leaves prob_io and entropy_out
 * unchanged -- the reference draws that root's action from np_random -- for the caller to resolve.
 * marginal: int32 [B, A] (row stride marginal_stride); legal: int32 [B, A] (row stride
 * legal_stride), required for ARGMAX, ignored by GIVEN.
 *   MZ_MARGINAL_ARGMAX_LEGAL (make_renalyze_update, reanalyze_worker.py:563-570): when the int64 sum
 *   over a of marginal[i, a] * legal[i, a] is > 0, action_io[i] = the first argmax of those products;
 *   otherwise action_io[i] = -1 (no visit on a legal action: the reference draws the action from
 *   np_random, the caller resolves it).  Neither prob_io nor entropy_out is touched; both may be NULL.
 *   legal is required.
 * B = the handle's active roots (mz_set_active_roots): every buffer holds B rows. */
int mz_marginal_policy(mz_batch *b, const int32_t *marginal, int64_t marginal_stride, const int32_t *legal,
                       int64_t legal_stride, int mode, int32_t *action_io, double *prob_io, double *entropy_out);

/* ---- reanalyze batch targets (core/reanalyze_worker.py:376-489, make_batch) ------------------
 *
 * The two entry points below take a tree handle OR a stream: with b != NULL the launch goes to the
 * handle's stream (ordered after its search, like the consumers above; `stream` is ignored); with
 * b == NULL it goes to `stream` (a hipStream_t, NULL = the default stream) on the current device --
 * the paths that run no search (NON_RE, use_pred_value) have no handle. */

enum mz_value_mode {
    MZ_VALUE_RE = 0,     /* _prepare_reward_value_re, reanalyze_worker.py:137-157 */
    MZ_VALUE_NON_RE = 1, /* _prepare_reward_value_non_re, reanalyze_worker.py:186-204 */
};

/* The n-step value targets and the reward targets, one lane per row.  Row j = g * (U + 1) + k is
 * unroll step k of trajectory g, current = pos[g] + k; the call covers rows [row0, row0 + n) of the
 * G * (U + 1) rows (a rank's share), and value / td_pow / out_* are indexed by j - row0.
 *   value      float32 [n]   RE: the agent-0 search's root values (reanalyze_worker.py:121-130) or
 *                            the network's predicted values (:132-133); unused by NON_RE (may be NULL)
 *   td_pow     float64 [n]   RE: np.power(discount, td_steps_lst) (:138), computed on the host by
 *                            exactly that expression (numpy's array power is not libm's pow on
 *                            every host, so the device does not recompute it); unused by NON_RE
 *   td         int32 [G]     td steps of each trajectory (after the clip of :82-84; NON_RE: all equal)
 *   pos, traj_len, reward_len  int32 [G]  state_index, len(game), len(game.rewards) >= traj_len
 *   rewards    [G, L]        game.rewards, rows padded to L; float32 when rewards_f32 else float64
 *   stored     [G, L]        NON_RE: game.root_values or game.pred_values (:191-194), padded;
 *                            float32 when stored_f32 else float64; unused by RE (may be NULL)
 *   dpow float64 [td_max], dpow32 float32 [td_max]   discount ** i as Python computes it, and that
 *                            cast to float32; td[g] <= td_max
 * RE:      v = (double)value[j] * td_pow[j];  v = v * (double)(current + td[g] < traj_len[g]);
 * NON_RE:  v = stored[g][current + td[g]] if current + td[g] < traj_len[g], else Python's int 0;
 * both:    for i in 0 .. min(current + td[g], reward_len[g]) - current - 1:  v += term(i), in order.
 * term(i) = reward * discount ** i under numpy 2 scalar promotion: a float64 reward gives the
 * float64 product with dpow[i], a float32 reward the float32 product with dpow32[i].  RE accumulates
 * in float64; NON_RE accumulates in float32 while rewards are float32 and the start is a float32
 * stored value or the int 0, in float64 otherwise.
 *   out_value[j - row0]  = v                    if current < traj_len[g] else 0   (float64 [n])
 *   out_reward[j - row0] = rewards[g][current]  if current < traj_len[g] else 0   (float64 [n])
 * Every index read from td / pos / traj_len / reward_len is clamped to the buffers' extents. */
int mz_value_targets(mz_batch *b, void *stream, int mode, int64_t row0, int n, int G, int U, const float *value,
                     const double *td_pow, const int32_t *td, const int32_t *pos, const int32_t *traj_len,
                     const int32_t *reward_len, const void *rewards, int rewards_f32, const void *stored,
                     int stored_f32, int64_t L, const double *dpow, const float *dpow32, int td_max,
                     double *out_value, double *out_reward);

/* numpy's float64 sum (np.add.reduce) of n contiguous elements as a plan (host only: no device
 * call).  numpy sums chunks of 8192 elements (its default buffer size) one after the other, in
 * order, each chunk by its pairwise recursion (above 128 elements: split at n2 = n / 2,
 * n2 -= n2 % 8, sum(left) + sum(right)).  Chunks and recursion are walked once: leaf l covers [starts[l], starts[l + 1]) (starts[num_leaves] = n; at most 128
 * elements, each start a multiple of 8), and ops is the recursion in postfix order: 0 pushes the
 * next leaf's sum, 1 replaces the two topmost sums by their sum.  A leaf of fewer than 8 elements
 * is a serial sum from 0.0; otherwise eight accumulators r[i] over the elements i mod 8 of the
 * whole groups of 8, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the n % 8 tail in order.
 * starts holds cap + 1 entries, ops 2 * cap; 1 <= n <= 65536 needs cap <= 1024. */
int mz_pairwise_plan(int n, int32_t *starts, int32_t *ops, int cap, int32_t *num_leaves, int32_t *num_ops);

/* Step (6) of make_batch (reanalyze_worker.py:466-473) over the whole batch, one workgroup:
 *   adv = (double)q - (double)pred;  mean = np.nanmean, std = np.nanstd over the entries with
 *   mask != 0 (and adv not NaN);  adv_out = (adv - mean) / (std + 1e-5), 0 where mask == 0.
 * numpy's own evaluation, bit for bit: mean = pairwise_sum(where(valid, adv, 0)) / cnt,
 * d = where(valid, adv - mean, 0), std = sqrt(pairwise_sum(d * d) / cnt), the pairwise sums by the
 * plan above.  cnt == 0 gives adv_out all zero and NaN statistics.
 *   q, pred float32 [n]; mask uint8 [n]; adv_out float64 [n]; stats_out float64 [2] = mean, std.
 * 1 <= n <= 65536 (MZ_ERR_UNSUPPORTED above).  The plan of each n is built and uploaded on first
 * use and kept: make the first call for an n outside any stream capture. */
int mz_normalize_advantage(mz_batch *b, void *stream, const float *q, const float *pred, const uint8_t *mask, int n,
                           double *adv_out, double *stats_out);

#ifdef __cplusplus
}
#endif

#endif /* MZCONSUME_H */
