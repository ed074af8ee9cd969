"""Device-resident `SampledMCTS.batch_search` — drop-in for the reference driver
core/mcts/tree_search/mcts_sampled.py:29-200.

Same constructor, same `batch_search` signature, same `SearchOutput` (numpy arrays and per-root
lists).  What changes is where the loop runs.  The reference moves every simulation's network
outputs to the host, prepares the next tree inputs with numpy and calls the CPU tree three times
per simulation.  Here the tree (mazero_amd.cytree on the MI355X library), the hidden-state pool
and the per-simulation glue stay on the device:

    select(s+1) + gather leaf rows          one kernel (fused with expand/backup of s)
    model.prediction(leaf)                  the model's own kernels (only when later agents exist)
    joint action                            mz_joint_action (numpy argmax semantics)
    model.dynamics + model.prediction       the model's own kernels, inverse transforms included
    policy softmax + beta                   mz_policy_glue (numpy float32/float16 arithmetic)

(with `wide_actions`: mz_root_glue_wide, mz_joint_action_wide, mz_policy_glue_wide, for action spaces
of 65..255; with `fused_transforms`: the inverse transforms of the value and reward heads are one
mz_inverse_transform launch, torch's arithmetic on this device restated bit for bit, instead of the
model's ~46 torch kernels; with `wide_supports` as well, mz_inverse_transform_wide does the same for
supports of 65..1024 elements; with `later_action_cache`: the `model.prediction(leaf)` pass goes, the
later agents' argmax is taken once per node by mz_policy_glue_later, which also does the policy glue,
and the joint action reads it back through mz_joint_action_cached; with `mixed_agents`: a merged
search whose entries are of different agents takes the current agent from a per-row device table,
through mz_policy_glue_rows, mz_joint_action_rows, mz_policy_glue_later_rows, mz_joint_action_cached_rows)

(`batch_search_joint` is the one search over joint-action trees that the reference's evaluation loop
calls, core/test.py:84: trees of agent_num = N, [B, N, A] tree inputs from mz_root_glue_joint and
mz_policy_glue_joint, the selection's [B, N] actions straight into the model, no joint-action estimate)

so a search has no host synchronisation between `prepare` and the final readback.  The root
preprocessing (mcts_sampled.py:51-106) is split: the host draws from `np_random` (the Dirichlet
noise, then the tree seed, in the reference's order) and packs the raw root inputs into one pinned
upload; the softmax, the legal masks and beta run on the device (mz_root_glue, numpy's dtype rules
restated) inside the recorded loop.  Inputs the kernel does not cover (float legal masks, other
logits dtypes) take the host path, `root_inputs`, numpy exactly as the reference computes it.

Model interface (core/model.py:45-79): `prediction(h) -> (policy_logits [B,N,A], value_logits)`,
`dynamics(h, joint_action [B,N]) -> (next_h, reward_logits)`, `inverse_value_transform`,
`inverse_reward_transform`; this is what MAMuZeroNet.recurrent_inference does in eval mode
(config/smac/model.py:562-572) minus the host copies.  A model may instead provide
`recurrent_inference_device(h, action) -> (next_h, reward [B,1], value [B,1], policy_logits)`.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import warnings
import weakref
from collections import OrderedDict
from typing import List, NamedTuple, Tuple

import numpy as np
import torch

from ._capi import INT_FIELDS, MZ_DT_F16, MZ_DT_F32, MZ_INV_EXPECTATION, MZ_INV_LOGITS, MZ_INV_PROBS, check
from .cytree import Tree_batch


class SearchOutput(NamedTuple):
    """mcts_sampled.py:12-26."""

    value: np.ndarray
    marginal_visit_count: np.ndarray
    marginal_priors: np.ndarray
    sampled_actions: List[np.ndarray]
    sampled_visit_count: List[np.ndarray]
    sampled_pred_probs: List[np.ndarray]
    sampled_beta: List[np.ndarray]
    sampled_beta_hat: List[np.ndarray]
    sampled_priors: List[np.ndarray]
    sampled_imp_ratio: List[np.ndarray]
    sampled_pred_values: List[np.ndarray]
    sampled_mcts_values: List[np.ndarray]
    sampled_rewards: List[np.ndarray]
    sampled_qvalues: List[np.ndarray]


_SAMPLED_FIELDS = ("actions", "visit_count", "pred_probs", "beta", "beta_hat", "priors", "imp_ratio",
                   "pred_values", "mcts_values", "rewards", "qvalues")


class DeviceSearchOutput(NamedTuple):
    """The search results as device tensors: per-root lists padded to the widest root degree
    (`degrees[i]` valid entries in row i).  `to_host()` gives the reference's SearchOutput."""

    value: torch.Tensor                  # f32 [B]
    marginal_visit_count: torch.Tensor   # i32 [B, 1, A] ([B, N, A] from a joint search)
    marginal_priors: torch.Tensor        # f32 [B, 1, A] ([B, N, A] from a joint search)
    degrees: torch.Tensor                # i32 [B]
    sampled: dict                        # field -> [B, maxdeg] (i32 for actions / visit_count; actions of a
    #                                      joint search: [B, maxdeg * N])
    tree: object = None                  # the Tree_batch that ran the search (its stream; consumers)

    def to_host(self) -> SearchOutput:
        deg = self.degrees.cpu().numpy()
        host = {k: v.cpu().numpy() for k, v in self.sampled.items()}
        B = deg.shape[0]
        N = self.marginal_visit_count.shape[1]  # the trees' agent_num (a joint search: all agents)

        def lists(name):
            a = host[name]
            if name == "actions":
                return [np.ascontiguousarray(a[i, : deg[i] * N]).reshape(deg[i], N) for i in range(B)]
            return [np.ascontiguousarray(a[i, : deg[i]]) for i in range(B)]

        return SearchOutput(self.value.cpu().numpy(), self.marginal_visit_count.cpu().numpy(),
                            self.marginal_priors.cpu().numpy(), *[lists(f) for f in _SAMPLED_FIELDS])


def slice_search_output(out: DeviceSearchOutput, lo: int, hi: int) -> DeviceSearchOutput:
    """Rows [lo, hi) of a DeviceSearchOutput as views: one entry of SampledMCTS.batch_search_many_device
    (its row bounds).  The per-root lists stay padded to the whole output's widest root; `to_host()` gives
    the entry's SearchOutput.  The slice keeps no tree: the consumers that size their launches by the
    handle's active roots take the whole output."""
    return DeviceSearchOutput(out.value[lo:hi], out.marginal_visit_count[lo:hi], out.marginal_priors[lo:hi],
                              out.degrees[lo:hi], {k: v[lo:hi] for k, v in out.sampled.items()}, None)


def _np(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return MZ_DT_F32
    if t.dtype == torch.float16:
        return MZ_DT_F16
    raise TypeError(f"policy logits must be float32 or float16, got {t.dtype}")


class _SearchLoop:
    """Static device buffers of one search configuration and, after the first (eager) search, a
    HIP graph of the whole simulation loop (prepare, S x [network, glue, fused tree kernel]).
    Every input is copied into the static buffers before a run, and the tree seed lives in device
    memory (mz_reseed), so replaying the graph is a new search."""

    def __init__(self, tb, B, A, N, cur, hidden, dev, model, root_mode=None, wide=False, fused=None,
                 wide_supports=False, later_slots=0, joint=False, mixed=False, wide_joint=False):
        self.tb, self.B, self.A, self.N, self.cur, self.dev = tb, B, A, N, cur, dev
        # mixed: the rows' searches are of different agents (SampledMCTS's mixed_agents).  The current agent
        # is device state, the static table row_agent [B] that the _rows glue reads at every launch (cur = 0
        # is unused), so one recorded graph serves every assignment of agents to rows; fac holds N - 1
        # columns, of which row i's first row_agent[i] are read.  The loop always runs the later-agents pass:
        # a row of the last agent takes nothing from it.
        self.mixed = bool(mixed)
        # joint: one search over the joint-action trees of all N agents (SampledMCTS.batch_search_joint;
        # the handle has agent_num = N).  The tree inputs are [B, N, A], the selection returns every agent's
        # action, so there is no current agent (cur = 0 is unused), no factor and no estimate of the later
        # agents' actions; the glue is the _joint entry points, every agent's row in one launch.
        self.joint_mode = bool(joint)
        # wide_joint (SampledMCTS's): the _joint_wide glue, which takes any A the handle has (A <= 255)
        jsfx = "_joint_wide" if wide_joint else "_joint"
        if joint:
            self.root_glue_joint = getattr(tb._lib, "mz_root_glue" + jsfx)
            self.policy_glue_joint = getattr(tb._lib, "mz_policy_glue" + jsfx)
        R = N if joint else 1  # rows of A actions per root in the tree's policy / beta / noise inputs
        # later_slots = S + 1 (SampledMCTS's later_action_cache; 0: off): the later agents' greedy actions
        # of every node, slot hidden_state_index_x, filled by mz_policy_glue_later when the node's state
        # is produced and read by mz_joint_action_cached instead of a prediction pass on the leaf.  The
        # last agent has no later agents: its loop is the default one.
        self.later = None
        if later_slots and (mixed or cur + 1 < N):
            # (zeros: an action read before its slot was written would still index the model's embedding)
            self.later = torch.zeros(later_slots, B, N, dtype=torch.int32, device=dev)
            # the first search also takes the default path and compares the two joint actions
            self.joint_cached = torch.empty(B, N, dtype=torch.int64, device=dev)
            self.mismatch = torch.zeros((), dtype=torch.bool, device=dev)
        # supports of 65 .. 1024 elements take LOGITS through mz_inverse_transform_wide (SampledMCTS's
        # wide_supports) instead of EXPECTATION behind torch's softmax, multiply and sum
        self.wide_supports = bool(wide_supports)
        # fused = (value (lo, hi), reward (lo, hi)) or the string "identity": the inverse transforms of
        # the two heads run as one mz_inverse_transform launch into inv_v / inv_r, which the tree call
        # reads (SampledMCTS's fused_transforms); None: the model's own transforms
        self.fused = fused
        if fused is not None and fused != "identity":
            self.inv_v = torch.empty(B, dtype=torch.float32, device=dev)
            self.inv_r = torch.empty(B, dtype=torch.float32, device=dev)
            # float32 supports of the EXPECTATION route (supports past 64 elements)
            self.inv_support = [torch.arange(lo, hi + 1, dtype=torch.float32, device=dev) for lo, hi in fused]
        # the glue entry points this loop records: the _wide ones take A <= 255 (SampledMCTS's
        # wide_actions), the narrow ones refuse A > 64
        sfx = "_wide" if wide else ""
        lib = tb._lib
        self.root_glue, self.joint_action, self.policy_glue = (
            getattr(lib, "mz_root_glue" + sfx), getattr(lib, "mz_joint_action" + sfx),
            getattr(lib, "mz_policy_glue" + sfx))
        if mixed:
            if not hasattr(lib, "mz_policy_glue_rows"):
                raise RuntimeError("mixed_agents needs a tree library with mz_policy_glue_rows (include/mzdriver.h, "
                                   "product library only)")
            self.row_agent = torch.zeros(B, dtype=torch.int32, device=dev)
        ensure_half_exp(tb._lib, dev.index if dev.index is not None else torch.cuda.current_device())
        self.model_ref = weakref.ref(model)  # the captured graph reads this model's parameters
        # [B, cols] like the caller's hidden state; B is the loop's root count, the driver's root_capacity
        # when it has one (the search's own hidden state may then hold fewer rows)
        self.root = hidden.new_empty((B, hidden[0].numel()))
        RA = R * A
        self.rin = [torch.empty(n, dtype=torch.float32, device=dev) for n in (B, B, B * RA, B * RA, B * RA)]
        # root_mode = (logits dtype code, has legal): the root preprocessing runs on the device
        # (mz_root_glue) from one packed upload of the raw root inputs; None: the host computes the
        # prepare arguments (SampledMCTS.root_inputs)
        self.root_mode = root_mode
        if root_mode is not None:
            dt_code, has_legal = root_mode
            ld = np.float16 if dt_code == MZ_DT_F16 else np.float32
            secs = [("rewards", np.float32, B), ("values", np.float32, B), ("noise", np.float32, B * RA)]
            if has_legal:
                secs.append(("legal", np.int32, B * RA))
            secs.append(("logits", ld, B * RA))
            off, self.sec = 0, {}
            for name, dt, n in secs:
                self.sec[name] = (off, dt, n)
                off += (np.dtype(dt).itemsize * n + 15) & ~15
            self.raw_host = torch.empty(off, dtype=torch.uint8, pin_memory=True)
            self.raw = torch.empty(off, dtype=torch.uint8, device=dev)
            self.raw_ev = None
            hv = self.raw_host.numpy()
            self.host_view = {k: hv[o:o + np.dtype(dt).itemsize * n].view(dt) for k, (o, dt, n) in self.sec.items()}
            tdt = {np.float32: torch.float32, np.float16: torch.float16, np.int32: torch.int32}
            self.dev_view = {k: self.raw[o:o + np.dtype(dt).itemsize * n].view(tdt[dt]) for k, (o, dt, n) in self.sec.items()}
        self.sel = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                    torch.empty(B, R, dtype=torch.int32, device=dev))
        self.joint = torch.empty(B, N, dtype=torch.int64, device=dev)
        self.probs = torch.empty(B, RA, dtype=torch.float32, device=dev)
        self.beta = torch.empty(B, RA, dtype=torch.float32, device=dev)
        self.fac = torch.zeros(B, max(N - 1 if mixed else cur, 1), dtype=torch.int32, device=dev)
        self.pool = None
        self.leaf = None
        self.pool_ref = None  # the shared _Pool the two above belong to (K > 1)
        self.graph = None  # None: not recorded yet; False: not replayable (capture found memset nodes)
        self.graph_nodes = None  # (nodes, memset nodes) of the recorded graph
        self.runs = 0
        self.storage = None  # _storage_signature(model) when the loop was made
        self.fused_rb = hasattr(tb._lib, "mz_expand_backup_readback")

    def load(self, hidden, root_arrays, factor):
        if hidden.shape[0] != self.B:
            return self._load_padded(hidden, root_arrays, factor)
        self.root.copy_(hidden.reshape(self.B, -1))
        if self.root_mode is None:
            for t, a in zip(self.rin, root_arrays):
                t.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        else:  # the raw root inputs: packed in pinned memory, one host->device copy
            if self.raw_ev is not None:
                self.raw_ev.synchronize()  # (the previous search's copy has read the pinned buffer)
            dev_logits = None
            for k, a in root_arrays.items():
                if isinstance(a, torch.Tensor):  # device logits: copied on the device below
                    dev_logits = a
                    continue
                np.copyto(self.host_view[k], np.asarray(a).reshape(-1), casting="no")
            self.raw.copy_(self.raw_host, non_blocking=True)
            self.raw_ev = torch.cuda.Event()
            self.raw_ev.record()
            if dev_logits is not None:
                self.dev_view["logits"].copy_(dev_logits.reshape(-1))
        if self.mixed:  # factor: (the rows' agents, their factor columns with zeros behind), on the device
            self.row_agent.copy_(factor[0])
            self.fac.copy_(factor[1])
        elif self.cur > 0:
            if isinstance(factor, torch.Tensor):  # previous agents' actions, already on the device
                self.fac.copy_(factor[:, : self.cur])
            else:
                self.fac.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(factor)[:, : self.cur], dtype=np.int32)))

    def _load_padded(self, hidden, root_arrays, factor):
        """load() for a search of n < B roots on this loop of B = root_capacity trees: the n real rows go
        into rows [0, n) of every static buffer and rows [n, B) get a copy of row 0, so the spare trees are
        replicas of tree 0 under other seeds: every input is finite and legal, and they raise no error
        that tree 0 could not."""
        n, B = hidden.shape[0], self.B

        def fill(t, src):  # t: a static buffer viewed [B, per]; src: its n real rows, on the device
            t[:n].copy_(src)
            t[n:] = t[0]

        fill(self.root, hidden.reshape(n, -1))
        if self.root_mode is None:
            for t, a in zip(self.rin, root_arrays):
                fill(t.view(B, -1), torch.from_numpy(np.ascontiguousarray(a).reshape(n, -1)))
        else:  # padded in the pinned buffer, then the one host->device copy
            if self.raw_ev is not None:
                self.raw_ev.synchronize()
            dev_logits = None
            for k, a in root_arrays.items():
                if isinstance(a, torch.Tensor):
                    dev_logits = a
                    continue
                hv = self.host_view[k].reshape(B, -1)
                np.copyto(hv[:n], np.asarray(a).reshape(n, -1), casting="no")
                hv[n:] = hv[0]
            self.raw.copy_(self.raw_host, non_blocking=True)
            self.raw_ev = torch.cuda.Event()
            self.raw_ev.record()
            if dev_logits is not None:
                fill(self.dev_view["logits"].view(B, -1), dev_logits.reshape(n, -1))
        if self.mixed:  # (the spare rows are row 0's searches: its agent with its inputs)
            fill(self.row_agent.view(B, 1), factor[0].view(n, 1))
            fill(self.fac, factor[1])
        elif self.cur > 0:
            if not isinstance(factor, torch.Tensor):
                factor = torch.from_numpy(np.ascontiguousarray(np.asarray(factor)[:, : self.cur], dtype=np.int32))
            fill(self.fac, factor[:, : self.cur])

    def run(self, model, cfg, eps, tau):
        """One search, mcts_sampled.py:106-172, all on the current stream."""
        tb, B, A, N, cur = self.tb, self.B, self.A, self.N, self.cur
        lib, h = tb._lib, tb._h
        c2, c1, disc = cfg.pb_c_base, cfg.pb_c_init, cfg.discount
        K, S = cfg.sampled_action_times, cfg.num_simulations
        r = self.rin
        model.eval()
        # bind the handle to the current stream first: the direct mz_* launches below (root glue,
        # joint action, policy glue) run on the handle's stream, which under a capture must be the
        # capturing one, or the launch runs at record time and is missing from the graph
        tb._sync_stream()
        if self.root_mode is not None:  # root preprocessing on the device, mcts_sampled.py:64-100
            dv = self.dev_view
            lg = dv.get("legal")
            if self.joint_mode:  # every agent's row: [B, N, A] in, [B, N, A] out
                check(lib, self.root_glue_joint(h, C.c_void_p(dv["logits"].data_ptr()), self.root_mode[0], N * A,
                                                N, None if lg is None else C.c_void_p(lg.data_ptr()), N * A,
                                                C.c_void_p(dv["noise"].data_ptr()), float(eps), float(tau),
                                                C.c_void_p(r[2].data_ptr()), C.c_void_p(r[3].data_ptr()),
                                                C.c_void_p(r[4].data_ptr())), "root_glue_joint")
            else:
                check(lib, self.root_glue(h, C.c_void_p(dv["logits"].data_ptr()), self.root_mode[0], A, 0,
                                          None if lg is None else C.c_void_p(lg.data_ptr()), A,
                                          C.c_void_p(dv["noise"].data_ptr()), float(eps), float(tau),
                                          C.c_void_p(r[2].data_ptr()), C.c_void_p(r[3].data_ptr()),
                                          C.c_void_p(r[4].data_ptr())), "root_glue")
            r = [dv["rewards"], dv["values"], r[2], r[3], r[4]]
        # prepare + the first selection (the root's forced first child) in one launch
        tb.prepare_selection_device(r[0], r[1], r[2], r[3], K, eps, r[4], c2, c1, disc, out=self.sel)
        act = self.sel[2]
        leaf = self.root  # simulation 0 selects a child of every root: its parent is the root (slot 0)
        # the later-action cache is checked on the loop's first search, which is always eager
        checked = self.later is not None and self.runs == 0
        if checked:
            self.mismatch.zero_()
        # One autocast context around the whole loop, its cast cache on: each fp32 weight is cast to
        # float16 once per search instead of once per simulation (the reference enters autocast per
        # simulation, mcts_sampled.py:150, so it casts every weight S times; the casts are identical).
        # The context opens and closes inside a capture, so the cached casts live in the graph's pool.
        # Inside a caller's own autocast context the cache would outlive this loop (it is cleared
        # when the outermost context exits), so there the casts stay per simulation.
        with torch.autocast("cuda", cache_enabled=not torch.is_autocast_enabled("cuda")):
            self._simulations(model, lib, h, leaf, act, B, A, N, cur, K, S, c2, c1, disc, tau, checked)
        if checked and bool(self.mismatch.item()):  # (the one host synchronisation, on a warm-up search)
            warnings.warn(f"later_action_cache: the cached later agents' actions differ from those of "
                          f"{type(model).__name__}.prediction on the selected leaves (prediction is not a "
                          "deterministic row-wise function of the state); this search loop takes the default "
                          "path", RuntimeWarning)
            self.later = None  # for good: this search already ran on the default joint actions

    def _later_glue(self, lib, h, logits, tau, slot, glue=True):
        """mz_policy_glue_later on `logits` [B, N, A]: the later agents' argmax into later[slot], with the
        policy glue of the current agent into probs / beta unless `glue` is False (the root's slot)."""
        logits = logits.contiguous()
        call, agent = lib.mz_policy_glue_later, self.cur
        if self.mixed:
            call, agent = lib.mz_policy_glue_later_rows, C.c_void_p(self.row_agent.data_ptr())
        check(lib, call(h, C.c_void_p(logits.data_ptr()), _dtype_code(logits), logits.shape[1] * logits.shape[2],
                        self.N, agent, float(tau), C.c_void_p(self.probs.data_ptr()) if glue else None,
                        C.c_void_p(self.beta.data_ptr()) if glue else None,
                        C.c_void_p(self.later[slot].data_ptr())), "policy_glue_later")

    def _simulations(self, model, lib, h, leaf, act, B, A, N, cur, K, S, c2, c1, disc, tau, checked=False):
        tb = self.tb
        cached = self.later is not None
        # the current agent as the glue takes it: the launch constant, or the table of a mixed loop
        joint_action, joint_action_cached, agent = self.joint_action, lib.mz_joint_action_cached, cur
        if self.mixed:
            joint_action, joint_action_cached = lib.mz_joint_action_rows, lib.mz_joint_action_cached_rows
            agent = C.c_void_p(self.row_agent.data_ptr())
        for s in range(S):
            # later agents' actions from the leaf policy, :136-145: a prediction pass on the leaves, or
            # (later_action_cache) the selected nodes' cached actions; the checked search runs both
            ptr, dt = None, MZ_DT_F32
            if self.joint_mode:
                # the selection's [B, N] actions are the whole joint action (:123-124 on joint trees):
                # widened into the static int64 buffer the model reads; no later agents to estimate
                self.joint.copy_(act)
            elif (self.mixed or cur + 1 < N) and (checked or not cached or s == 0):
                pred_logits, _ = model.prediction(leaf)  # (s == 0: the leaf batch is the root batch)
                pred_logits = pred_logits.contiguous()
                ptr, dt = C.c_void_p(pred_logits.data_ptr()), _dtype_code(pred_logits)
                if cached and s == 0:
                    self._later_glue(lib, h, pred_logits, tau, 0, glue=False)
            if cached:
                check(lib, joint_action_cached(
                    h, C.c_void_p(self.later.data_ptr()), self.later.shape[0], C.c_void_p(self.sel[0].data_ptr()),
                    N, agent, C.c_void_p(self.fac.data_ptr()), self.fac.shape[1], C.c_void_p(act.data_ptr()),
                    C.c_void_p((self.joint_cached if checked else self.joint).data_ptr())), "joint_action_cached")
            if (checked or not cached) and not self.joint_mode:
                check(lib, joint_action(h, ptr, dt, N, agent, C.c_void_p(self.fac.data_ptr()), self.fac.shape[1],
                                        C.c_void_p(act.data_ptr()), C.c_void_p(self.joint.data_ptr())),
                      "joint_action")
            if checked:  # dynamics takes the default joint action below: a mismatch costs nothing but the cache
                self.mismatch |= (self.joint != self.joint_cached).any()
            r32 = v32 = None
            if self.fused is not None and getattr(model, "recurrent_inference_device", None) is None:
                next_h, reward_logits = model.dynamics(leaf, self.joint)
                logits, value_logits = model.prediction(next_h)
                if self.fused == "identity":  # use_vectorization off: the heads' scalars, core/config.py:487-499
                    reward, value = reward_logits, value_logits
                elif self._inverse_transform(lib, h, value_logits, reward_logits):
                    r32, v32 = self.inv_r, self.inv_v
                else:
                    reward = model.inverse_reward_transform(reward_logits)
                    value = model.inverse_value_transform(value_logits)
            else:
                next_h, reward, value, logits = SampledMCTS._recurrent(model, leaf, self.joint)  # :150-156
            nh = next_h.reshape(B, -1)
            chain = K == 1
            if chain:
                # K = 1: every tree is a chain, so every selection of simulation s + 1 ends at the
                # child created by simulation s, whose parent holds hidden_state_index_x = s + 1 for
                # every root: the reference's gather pool[s + 1][i] (mcts_sampled.py:130-134) is row i
                # of this network output.  No pool and no gather: the output is the next leaf batch.
                pass
            else:
                if self.pool is None:
                    # one pool per (thread, device, S, B, row, dtype), shared by the agent loops of a
                    # geometry: searches on one thread run one after the other, and every search
                    # writes slot 0 and slots 1..S before it reads them
                    pdt = torch.promote_types(self.root.dtype, nh.dtype)
                    self.pool_ref = _shared_pool(self.dev, S, B, nh.shape[1], pdt)
                    self.pool, self.leaf = self.pool_ref.pool, self.pool_ref.leaf
                if s == 0:
                    self.pool[0].copy_(self.root)
                self.pool[s + 1].copy_(nh)  # :164
            if cached:  # the policy glue, and the new node's later actions into its slot
                self._later_glue(lib, h, logits, tau, s + 1)
            elif self.joint_mode:  # all agents' logits, :156 on joint trees
                if logits.dim() != 3 or logits.shape[1] != N or logits.shape[2] != A:
                    raise ValueError(f"joint search: policy logits of shape {tuple(logits.shape)} for {N} agents "
                                     f"and {A} actions")
                logits = logits.contiguous()
                check(lib, self.policy_glue_joint(h, C.c_void_p(logits.data_ptr()), _dtype_code(logits),
                                                  logits.shape[1] * logits.shape[2], N, float(tau),
                                                  C.c_void_p(self.probs.data_ptr()),
                                                  C.c_void_p(self.beta.data_ptr())), "policy_glue_joint")
            elif self.mixed:  # every row's own agent's logits
                logits = logits.contiguous()
                check(lib, lib.mz_policy_glue_rows(h, C.c_void_p(logits.data_ptr()), _dtype_code(logits),
                                                   logits.shape[1] * logits.shape[2], N, agent, float(tau),
                                                   C.c_void_p(self.probs.data_ptr()),
                                                   C.c_void_p(self.beta.data_ptr())), "policy_glue_rows")
            else:
                logits = logits.contiguous()
                check(lib, self.policy_glue(h, C.c_void_p(logits.data_ptr()), _dtype_code(logits),
                                            logits.shape[1] * logits.shape[2], cur * A, float(tau),
                                            C.c_void_p(self.probs.data_ptr()), C.c_void_p(self.beta.data_ptr())),
                      "policy_glue")
            if r32 is None:
                r32 = reward.reshape(B).float()
                v32 = value.reshape(B).float()
            if s + 1 < S:
                tb.expansion_backup_selection_device(s + 1, disc, K, r32, v32, self.probs, self.beta, c2, c1,
                                                     out=self.sel, pool=None if chain else self.pool,
                                                     gather_out=None if chain else self.leaf)
                leaf = nh if chain else self.leaf
            elif self.fused_rb:
                # the last expansion also writes the packed readback (mz_expand_backup_readback): the
                # SearchOutput getters then only copy it to the host
                tb.expansion_backup_readback_device(s + 1, disc, K, r32, v32, self.probs, self.beta,
                                                    readback_discount=disc)
            else:
                tb.batch_expansion_and_backup(s + 1, disc, K, r32, v32, self.probs, self.beta)

    def _inverse_transform(self, lib, h, value_logits, reward_logits) -> bool:
        """inverse_value_transform / inverse_reward_transform of the two heads' logits (core/config.py:
        487-499) as one mz_inverse_transform launch into inv_v / inv_r.  False: these logits are not
        covered (the caller applies the model's own transforms): a dtype other than float32 / float16,
        or half logits outside autocast, where torch rounds the softmax to half."""
        B = self.B
        heads = []
        for t, (lo, hi) in zip((value_logits, reward_logits), self.fused):
            if t.dtype not in (torch.float32, torch.float16):
                return False
            if t.dtype == torch.float16 and not torch.is_autocast_enabled("cuda"):
                return False
            if t.dim() != 2 or t.shape[0] != B or t.shape[1] != hi - lo + 1:
                raise ValueError(f"fused_transforms: head logits of shape {tuple(t.shape)} for the support "
                                 f"[{lo}, {hi}] of the config and {B} roots")
            heads.append(t)
        stage, call = FUSED_STAGE, lib.mz_inverse_transform
        longest = max(hi - lo + 1 for lo, hi in self.fused)
        if longest > MAX_FUSED_SUPPORT:  # a support past one wave, the reference's default [-300, 300]
            if self.wide_supports and longest <= MAX_WIDE_SUPPORT:
                call = lib.mz_inverse_transform_wide
            else:
                stage = MZ_INV_EXPECTATION
        if stage == MZ_INV_LOGITS:
            heads = [t if t.stride(1) == 1 else t.contiguous() for t in heads]
        elif stage == MZ_INV_PROBS:
            heads = [torch.softmax(t, dim=-1) for t in heads]
        else:  # torch's softmax, multiply and sum; the kernel is _inv_h
            heads = [torch.sum(sup * torch.softmax(t, dim=-1), dim=-1, keepdim=True)
                     for t, sup in zip(heads, self.inv_support)]
        (v, r), ((vlo, vhi), (rlo, rhi)) = heads, self.fused
        check(lib, call(h, None, stage, B,
                        C.c_void_p(v.data_ptr()), _dtype_code(v), v.stride(0), vlo, vhi,
                        C.c_void_p(r.data_ptr()), _dtype_code(r), r.stride(0), rlo, rhi,
                        C.c_void_p(self.inv_v.data_ptr()), C.c_void_p(self.inv_r.data_ptr())),
              "inverse_transform")
        return True

    def capture(self, model, cfg, eps, tau) -> bool:
        """Record the loop.  The recorded graph is checked before it is instantiated: under the HIP
        runtime's default graph packet capture a replayed memset node can write a stale fill
        pattern.  No mz_* call records one, but the model's ops might (a BLAS
        workspace clear, an output zeroing); then this loop stays eager (graph = False) and the
        caller runs it eagerly.  Returns whether a graph is ready to replay."""
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g):
            self.run(model, cfg, eps, tau)
        lib = self.tb._lib
        total, memsets = C.c_int(0), C.c_int(0)
        check(lib, lib.mz_graph_census(C.c_void_p(g.raw_cuda_graph()), C.byref(total), C.byref(memsets)),
              "graph_census")
        self.graph_nodes = (total.value, memsets.value)
        if memsets.value:
            warnings.warn(f"the captured search loop holds {memsets.value} memset node(s) of {total.value} "
                          "(recorded by the model's ops): a replayed memset node can write a stale value under "
                          "the HIP runtime's graph packet capture, so this search loop runs eagerly", RuntimeWarning)
            self.graph = False
            return False
        g.instantiate()
        self.graph = g
        return True


# Search-loop caches.  The reference builds a new Tree_batch and a new hidden-state pool per search
# (mcts_sampled.py:86,89) and frees both when the search returns; here a search geometry keeps its
# device arena (_TREES), each agent loop its captured graph (_LOOPS), and the loops of one geometry
# share one hidden-state pool (_POOLS), so that a 27-agent self-play step holds one [S+1, B, N*H]
# pool, not 27.  Every key carries the calling thread: two threads never share a handle (a handle is
# single-threaded, include/mzmcts.h) or a pool; a pool's key also carries the stream its first loop
# ran on.  Both caches are LRU-bounded (MZ_MAX_TREES,
# MZ_MAX_LOOPS); release() empties them.
_LOCK = threading.RLock()
_LOOPS: "OrderedDict" = OrderedDict()
_TREES: "OrderedDict" = OrderedDict()
_POOLS: "weakref.WeakValueDictionary" = weakref.WeakValueDictionary()
_MAX_LOOPS = int(os.environ.get("MZ_MAX_LOOPS", "64"))  # >= the agents of one self-play step
_MAX_TREES = int(os.environ.get("MZ_MAX_TREES", "8"))
_HALF_EXP: set = set()  # (library, device index) pairs holding the host's float16 exp table


class _Pool:
    """A hidden-state pool [S+1, B, cols] and its leaf-row buffer [B, cols]; freed when the last loop
    holding it goes."""

    __slots__ = ("pool", "leaf", "__weakref__")

    def __init__(self, pool, leaf):
        self.pool, self.leaf = pool, leaf


def _shared_pool(dev, S: int, B: int, cols: int, dtype) -> _Pool:
    # (the current stream too: loops that a thread runs on different streams may overlap on the
    # device, so they must not share a pool -- ADVICE round 5; loops on one stream run in order)
    stream = torch.cuda.current_stream(dev).cuda_stream if torch.device(dev).type == "cuda" else 0
    key = (threading.get_ident(), stream, str(dev), S + 1, B, int(cols), dtype)
    with _LOCK:
        p = _POOLS.get(key)
        if p is None:
            p = _Pool(torch.empty((S + 1, B, cols), dtype=dtype, device=dev), torch.empty((B, cols), dtype=dtype, device=dev))
            _POOLS[key] = p
        return p


def _evict_loops_of(tb) -> None:
    for k in [k for k, v in _LOOPS.items() if v.tb is tb]:
        del _LOOPS[k]


def release() -> int:
    """Drop every cached tree handle, search loop (its graph) and hidden-state pool, of every thread
    (what the reference frees after each search, mcts_sampled.py:86,89), then free the device arenas
    the destroyed handles returned to the library's cache (mz_trim_caches).  The next search of a
    geometry allocates and records again.  Returns the bytes the library released."""
    with _LOCK:
        _LOOPS.clear()
        _TREES.clear()
        _POOLS.clear()
    from ._lib import trim_caches

    return trim_caches()


def half_exp_table() -> np.ndarray:
    """np.exp of every float16 bit pattern as this host's numpy evaluates it (uint16 bits).  numpy's
    float16 exp is not always float32 exp rounded to half (its AVX512_SKX half loop differs in a
    few inputs), and the reference computes the root / leaf softmax with it under autocast."""
    with np.errstate(all="ignore"):
        return np.exp(np.arange(1 << 16, dtype=np.uint16).view(np.float16)).view(np.uint16).copy()


def ensure_half_exp(lib, device_index: int) -> None:
    """Give `lib`'s float16 glue kernels on device `device_index` the host's exp table (once)."""
    key = (id(lib), int(device_index))
    if key in _HALF_EXP or not hasattr(lib, "mz_set_half_exp_table"):
        return
    t = half_exp_table()
    with torch.cuda.device(int(device_index)):
        check(lib, lib.mz_set_half_exp_table(t.ctypes.data_as(C.c_void_p)), "set_half_exp_table")
    _HALF_EXP.add(key)


def _storage_signature(model) -> tuple:
    """Device addresses of the model's parameters and buffers (what a recorded graph reads)."""
    return tuple(t.data_ptr() for t in model.parameters()) + tuple(t.data_ptr() for t in model.buffers())


# One device arena per search geometry and thread, kept across searches and across SampledMCTS
# instances (the self-play worker makes a new SampledMCTS every environment step,
# selfplay_worker.py:187); a search reseeds it instead of allocating a new tree batch as the
# reference does (:89).


MAX_GLUE_ACTIONS = 64  # include/mzdriver.h: the glue kernels hold one action per lane
MAX_WIDE_ACTIONS = 255  # the _wide glue entry points: every action space the tree itself takes
MAX_FUSED_SUPPORT = 64  # mz_inverse_transform's LOGITS / PROBS stages: one lane per support element
# how much of softmax -> _inv_phi -> _inv_h the fused launch computes for supports of up to 64
# elements; longer supports take MZ_INV_EXPECTATION behind torch's softmax and sum
FUSED_STAGE = MZ_INV_LOGITS
MAX_WIDE_SUPPORT = 1024  # mz_inverse_transform_wide's LOGITS / PROBS stages (torch's softmax_warp_forward)


def _support_bounds(support) -> Tuple[int, int]:
    """(lo, hi) of a DiscreteSupport-like object (`.min` / `.max`, core/config.py:247-255) or a pair."""
    lo, hi = getattr(support, "min", None), getattr(support, "max", None)
    if lo is None or hi is None or callable(lo) or callable(hi):  # (an array's min / max are methods)
        lo, hi = support
    lo, hi = int(lo), int(hi)
    if hi < lo:
        raise ValueError(f"support [{lo}, {hi}] is empty")
    return lo, hi


# the place of the root offset in the key of a handle whose offset is device state (device_root_offset)
_DEVICE_OFFSET = "device_root_offset"
# the place of the current agent in the key of a joint search's loop (no agent index is negative)
_JOINT_AGENT = -1
# the place of the current agent in the key of a mixed loop (mixed_agents: the agent is per-row device state)
_MIXED_AGENTS = "row_agent"
# the last element of the key of a merged search's loop (batch_search_many: per-segment tree seeds)
_SEGMENTED = "seed_segments"


def skip_search_draws(config, np_random, total: int, num_agents: int = 1) -> None:
    """What one search of `total` roots draws from `np_random` before it launches anything: the
    Dirichlet rows, then the tree seed (mcts_sampled.py:68,89).  `num_agents`: a joint search
    (batch_search_joint) draws one row per (root, agent)."""
    size = int(total) if int(num_agents) == 1 else (int(total), int(num_agents))
    np_random.dirichlet([config.root_dirichlet_alpha] * config.action_space_size, size)
    np_random.choice(256)


class SampledMCTS:
    """mcts_sampled.py:29-32.  `lib` selects the tree library (default: the MI355X product)."""

    def __init__(self, config, np_random: np.random.RandomState = None, *, lib=None, use_graph: bool = True,
                 root_shard: Tuple[int, int, int] = None, device_root: bool = True, wide_actions: bool = None,
                 fused_transforms: bool = None, wide_supports: bool = None, later_action_cache: bool = None,
                 root_capacity: int = None, device_root_offset: bool = None, mixed_agents: bool = None,
                 wide_joint: bool = None):
        """`wide_joint`: batch_search_joint builds its trees with mz_create_wide_joint and runs the
        _joint_wide glue (include/mzdriver.h): joint-action trees of up to 255 actions per agent and 255
        sampled joint actions (agent_num <= 64, agent_num * action_space_size <= 4096), instead of 64 and
        64.  Inside the narrow bounds the handle and its kernels are those of the search without the flag.
        The constructor then accepts action_space_size <= 255, as with `wide_actions`.  None reads
        `config.wide_joint` (False when the config has none).  Off by default: the refusals of the joint
        search are pinned by the test suite.  The per-agent searches are unchanged by it.

        `mixed_agents`: batch_search_many takes entries of different agents (`current_agent_idx` a
        sequence with differing values) and runs them on one loop whose current agent is per-row device
        state: a static int32 table that the _rows glue entry points read (include/mzdriver.h), so one
        recorded graph serves every assignment of agents to rows of a geometry.  Entry g equals
        `batch_search(model, outs[g], cur_g, factors[g], N, legals[g], ...)` bit for bit, under
        batch_search_many's condition.  The mixed loop always runs the later-agents pass (rows of the last
        agent take nothing from it).  A call whose entries all name one agent takes the per-agent loop,
        with the key, the launches and the bytes it has without the flag.  None reads
        `config.mixed_agents` (False when the config has none).  Off by default: the refusal of entries
        of different agents is pinned by the test suite.  consume.reanalyze_policy_targets_many runs the
        agent searches of several reanalyze batches as a wavefront on such loops.

        `root_capacity` = C: every search of B <= C roots runs on the tree handle and the per-agent
        loops (static buffers, recorded graph) of the C-root geometry, so a batch that shrinks and grows
        (self-play searches only the environments still running, selfplay_worker.py:171-211; full-game
        reanalysis searches len(game) roots, reanalyze_worker.py:491-611) keeps replaying one recorded
        loop per agent instead of meeting a new geometry at every size.  The B real rows are loaded into
        rows [0, B) of the loop's buffers and rows [B, C) are copies of row 0; the handle then reports B
        active roots (Tree_batch.set_active_roots), so the outputs hold exactly B rows.  `np_random` is
        consumed as by a B-root search.  Trees are independent and tree i is seeded by its index: the
        results are rows [0, B) of the reference search over the padded C-row batch, and they equal the
        plain B-root search bit for bit whenever row i of the model's outputs and of the transforms does
        not depend on how many rows the batch has.  B > C raises ValueError.  None reads
        `config.root_capacity` (off when the config has none).  Together with `root_shard` only under
        `device_root_offset`.

        `device_root_offset`: the tree handle's root offset follows the shard from search to search.  A
        sharded rank's tree i is seeded with its position lo + i in the whole batch; that offset is a
        device word beside the seed (Tree_batch.set_root_offset, include/mzdriver.h mz_set_root_offset),
        which the prepare kernels read, so a recorded graph follows it.  With the flag the handle is keyed
        without the offset: one handle and its recorded loops serve every shard position, the offset is
        set next to the reseed whenever it differs from the handle's, `root_capacity=C` is accepted with
        `root_shard=(lo, hi, total)` when hi - lo <= C, and an empty shard (lo == hi: a rank none of whose
        environments still runs) is legal -- it searches nothing, and `skip_search` consumes what one
        search draws from `np_random`, so every rank's generator stays in the same state.  None reads
        `config.device_root_offset` (False when the config has none).  Off by default: the refusal of
        `root_capacity` with `root_shard` is pinned by the test suite.

        `later_action_cache`: take the later agents' greedy actions of every simulation
        (mcts_sampled.py:136-147) from a per-node cache instead of a `model.prediction` pass on the
        selected leaves' parent states.  Such a state is row i of the `next_h` an earlier simulation
        produced, and `prediction` already ran on it there; mz_policy_glue_later keeps the later agents'
        argmax of those logits per node, and mz_joint_action_cached looks them up by the selection's
        hidden_state_index_x.  This assumes that `prediction` is a deterministic, row-wise function of the
        state (every net of the reference in eval mode is).  The assumption is checked on each loop's
        first search, which also runs the default path and compares the joint actions on the device: on
        a mismatch that search returns the default path's results, a RuntimeWarning names the model
        class and the loop takes the default path from then on.  None reads
        `config.later_action_cache` (False when the config has none).  The search of the last agent
        has no later agents and is unchanged.

        `fused_transforms`: compute the inverse value / reward transforms of every simulation
        (core/config.py:487-499) with one mz_inverse_transform launch instead of the model's
        `inverse_value_transform` / `inverse_reward_transform`; the search calls `model.dynamics` and
        `model.prediction` itself.  The supports are `config.value_support` / `config.reward_support`
        (objects with `.min` / `.max`, or (lo, hi) pairs); with `config.use_vectorization` False the
        heads' scalars pass through.  None reads `config.fused_transforms` (False when the config has
        none).  The results are those of the torch chain on the same device, bit for bit.  A model with
        `recurrent_inference_device`, or head logits that are not float32 / autocast float16, keep the
        model's own transforms.

        `wide_supports`: with `fused_transforms`, supports of 65 to 1,024 elements (the reference's
        default DiscreteSupport(-300, 300)) also get the whole chain in that one launch, through
        mz_inverse_transform_wide; without it they keep torch's softmax, multiply and sum and only
        _inv_h is fused.  None reads `config.wide_supports` (False when the config has none).  Longer
        supports keep that route either way, and the flag alone, without `fused_transforms`, has no
        effect.

        `wide_actions`: run the driver glue through the _wide entry points (include/mzdriver.h), which
        take action spaces up to 255 instead of 64.  None reads `config.wide_actions` (False when the
        config has none), so a reference-style `SampledMCTS(config, np_random)` opts in through its
        config object.  Off by default: the refusal of A > 64 below is pinned by the test suite.

        `root_shard` = (lo, hi, total): this instance searches roots [lo, hi) of a batch of `total`
        roots sharded over ranks (mazero_amd.workers).  Every rank holds the same `np_random` state;
        the per-root draws (Dirichlet noise here, select_action's uniforms in consume) are drawn for
        the whole batch and sliced, and tree i is seeded with its global index, so a rank's results
        equal rows [lo, hi) of the unsharded search."""
        self.config = config
        if wide_actions is None:
            wide_actions = getattr(config, "wide_actions", False)
        self.wide_actions = bool(wide_actions)
        if wide_joint is None:
            wide_joint = getattr(config, "wide_joint", False)
        self.wide_joint = bool(wide_joint)
        if self.wide_actions or self.wide_joint:
            if int(config.action_space_size) > MAX_WIDE_ACTIONS:
                raise RuntimeError(f"SampledMCTS: action_space_size {config.action_space_size} > {MAX_WIDE_ACTIONS} "
                                   "(a tree node packs its action in 8 bits; the wide driver glue and "
                                   "mazero_amd.cytree.Tree_batch take up to 255)")
        elif int(config.action_space_size) > MAX_GLUE_ACTIONS:
            # the device driver glue (mz_policy_glue, mz_root_glue, mz_joint_action: one lane per
            # action) refuses wider action spaces; refused here, before any search launches (the
            # drop-in Tree_batch surface itself takes A <= 255)
            raise RuntimeError(f"SampledMCTS: action_space_size {config.action_space_size} > {MAX_GLUE_ACTIONS} "
                               "(the device driver glue takes one lane per action; mazero_amd.cytree.Tree_batch "
                               "takes up to 255)")
        if fused_transforms is None:
            fused_transforms = getattr(config, "fused_transforms", False)
        # None, "identity" (use_vectorization off) or the two heads' (lo, hi); part of the loop's key
        self.fused_transforms = None
        if fused_transforms:
            if not getattr(config, "use_vectorization", True):
                self.fused_transforms = "identity"
            else:
                self.fused_transforms = (_support_bounds(config.value_support),
                                         _support_bounds(config.reward_support))
        if wide_supports is None:
            wide_supports = getattr(config, "wide_supports", False)
        self.wide_supports = bool(wide_supports)
        if later_action_cache is None:
            later_action_cache = getattr(config, "later_action_cache", False)
        self.later_action_cache = bool(later_action_cache)
        self.np_random = np.random if np_random is None else np_random
        self._lib = lib
        if device_root_offset is None:
            device_root_offset = getattr(config, "device_root_offset", False)
        self.device_root_offset = bool(device_root_offset)
        if self.device_root_offset and lib is not None and not hasattr(lib, "mz_set_root_offset"):
            raise RuntimeError("device_root_offset needs a tree library with mz_set_root_offset "
                               "(include/mzdriver.h, product library only)")
        if root_shard is not None:
            lo, hi, total = (int(x) for x in root_shard)
            # (an empty shard only where the handle follows the shard: skip_search)
            if not (0 <= lo <= hi <= total and (lo < hi or self.device_root_offset)):
                raise ValueError(f"bad root shard {root_shard}")
            root_shard = (lo, hi, total)
        self.root_shard = root_shard
        if root_capacity is None:
            root_capacity = getattr(config, "root_capacity", None)
        if root_capacity is not None:
            root_capacity = int(root_capacity)
            if root_capacity < 1:
                raise ValueError(f"root_capacity must be >= 1, got {root_capacity}")
            if root_shard is not None and not self.device_root_offset:
                raise ValueError(f"root_capacity={root_capacity} with root_shard={root_shard}: a rank's trees "
                                 "are seeded from its root offset, a launch argument of the prepare kernels in "
                                 "the recorded graph, which cannot follow a varying root count")
            if root_shard is not None and root_shard[1] - root_shard[0] > root_capacity:
                raise ValueError(f"root_shard={root_shard} holds {root_shard[1] - root_shard[0]} roots, more than "
                                 f"root_capacity={root_capacity}")
            if lib is not None and not hasattr(lib, "mz_set_active_roots"):
                raise RuntimeError("root_capacity needs a tree library with mz_set_active_roots "
                                   "(include/mzdriver.h, product library only)")
        self.root_capacity = root_capacity
        if mixed_agents is None:
            mixed_agents = getattr(config, "mixed_agents", False)
        self.mixed_agents = bool(mixed_agents)
        if self.mixed_agents and lib is not None and not hasattr(lib, "mz_policy_glue_rows"):
            raise ValueError("mixed_agents needs a tree library with mz_policy_glue_rows (include/mzdriver.h, "
                             "product library only)")
        self.use_graph = use_graph
        # root preprocessing (softmax, masks, beta) on the device (mz_root_glue); False: in numpy on
        # the host (root_inputs), as the reference computes it
        self.device_root = device_root

    # ---------------------------------------------------------------------------------------
    def root_inputs(self, network_output, current_agent_idx, legal_actions_lst, add_noise, sampled_tau, draw=None):
        """Root preprocessing, mcts_sampled.py:51-106, in numpy on the host (it draws from
        np_random).  Returns the prepare() arguments and the tree seed.  `current_agent_idx` None: the
        joint search's (batch_search_joint), every agent's row, [B, N, A] arrays.  `draw`: the (noise,
        seed) pair of an earlier draw_search(B) instead of fresh draws."""
        cfg = self.config
        alpha, eps = cfg.root_dirichlet_alpha, cfg.root_exploration_fraction
        A = cfg.action_space_size
        B = network_output.hidden_state.shape[0]
        joint = current_agent_idx is None
        logits = _np(network_output.policy_logits)
        R = logits.shape[1] if joint else 1
        logits = logits.reshape(B, R, A) if joint else logits[:, current_agent_idx, :].reshape(B, 1, A)
        # softmax in the logits' own dtype (float16 under autocast), :64-65
        probs = np.exp(logits - np.max(logits, axis=-1, keepdims=True))
        probs = probs / np.sum(probs, axis=-1, keepdims=True)
        # Dirichlet noise is always drawn, then disabled for evaluation, :68-70
        noises = self.draw_rows(lambda n: self.np_random.dirichlet([alpha] * A, (n, R) if joint else n), B) \
            if draw is None else np.asarray(draw[0])
        noises = noises.astype(np.float32).reshape(B, R, A)
        if not add_noise:
            eps = 0.0
        mask = None
        if legal_actions_lst is not None:  # :73-83
            mask = (legal_actions_lst if joint else legal_actions_lst[:, current_agent_idx, :]).reshape(B, R, A)
            probs *= mask
            probs += mask * 1e-4
            probs = probs / np.sum(probs, axis=-1, keepdims=True)
            noises *= mask
            noises += mask * 1e-4
            noises = noises / np.sum(noises, axis=-1, keepdims=True)
        seed = self.np_random.choice(256) if draw is None else draw[1]  # drawn after the noise, :89
        beta = probs * (1 - eps) + noises * eps  # :93-100
        beta = beta ** (1 / sampled_tau)
        if mask is not None:
            beta *= mask
        beta = beta / np.sum(beta, axis=-1, keepdims=True)
        rewards = _np(network_output.reward).reshape(B).astype(np.float32)
        values = _np(network_output.value).reshape(B).astype(np.float32)
        return (rewards, values, probs.astype(np.float32), beta.astype(np.float32), eps,
                noises.astype(np.float32, copy=False)), seed

    def root_raw(self, network_output, current_agent_idx, legal_actions_lst, add_noise, draw=None):
        """The raw root inputs of the device root preprocessing (mz_root_glue): the Dirichlet draws
        (np_random, then the tree seed, in the reference's order, mcts_sampled.py:68,89) and the
        arrays to upload, or None when the device path does not cover the inputs' dtypes (the host
        path, root_inputs, takes them).  Returns (arrays, (logits dtype code, has legal), eps, seed).
        `current_agent_idx` None: the joint search's (batch_search_joint), every agent's columns and one
        Dirichlet row per (root, agent), for mz_root_glue_joint.  `draw`: the (noise, seed) pair of an
        earlier draw_search(B) instead of fresh draws."""
        cfg = self.config
        A = cfg.action_space_size
        B = network_output.hidden_state.shape[0]
        joint = current_agent_idx is None
        lg = network_output.policy_logits
        if isinstance(lg, torch.Tensor):
            if not lg.is_cuda or lg.dtype not in (torch.float32, torch.float16):
                return None
            logits = lg if joint else lg[:, current_agent_idx, :]
            code = _dtype_code(lg)
        else:
            lg = np.asarray(lg)
            if lg.dtype not in (np.float32, np.float16):
                return None
            logits = lg if joint else lg[:, current_agent_idx, :]
            code = MZ_DT_F16 if lg.dtype == np.float16 else MZ_DT_F32
        R = lg.shape[1] if joint else 1
        legal = None
        if legal_actions_lst is not None:
            la = _np(legal_actions_lst)
            if la.dtype.kind not in "iub":
                return None  # (float masks: numpy's float arithmetic differs; the host path)
            legal = la if joint else la[:, current_agent_idx, :]
            if legal.dtype.kind != "b" and legal.size and (legal.min() < -(1 << 31) or legal.max() >= (1 << 31)):
                return None
            legal = legal.astype(np.int32)
        alpha, eps = cfg.root_dirichlet_alpha, cfg.root_exploration_fraction
        noise = self.draw_rows(lambda n: self.np_random.dirichlet([alpha] * A, (n, R) if joint else n), B) \
            if draw is None else np.asarray(draw[0])
        if noise.shape[0] != B:
            raise ValueError(f"draws for {noise.shape[0]} roots, batch of {B}")
        noise = noise.astype(np.float32)
        if not add_noise:
            eps = 0.0
        seed = self.np_random.choice(256) if draw is None else draw[1]  # drawn after the noise, :89
        arrays = dict(rewards=_np(network_output.reward).reshape(B).astype(np.float32),
                      values=_np(network_output.value).reshape(B).astype(np.float32), noise=noise, logits=logits)
        if legal is not None:
            arrays["legal"] = legal
        return arrays, (code, legal is not None), eps, seed

    def draw_rows(self, draw, B: int) -> np.ndarray:
        """`draw(n)` -> n per-root rows from np_random; with a root shard the whole batch's rows are
        drawn (same generator consumption on every rank) and this shard's rows returned."""
        if self.root_shard is None:
            return draw(B)
        lo, hi, total = self.root_shard
        if hi - lo != B:
            raise ValueError(f"batch of {B} roots but the root shard is [{lo}, {hi})")
        return draw(total)[lo:hi]

    def draw_search(self, B: int):
        """What one per-agent search of B roots draws from `np_random` before it launches anything --
        the Dirichlet rows, then the tree seed (mcts_sampled.py:68,89) -- as a (noise, seed) pair for
        batch_search_many's `draws=`: a caller draws in the reference's order for searches it runs later,
        in another grouping."""
        cfg = self.config
        noise = self.draw_rows(lambda n: self.np_random.dirichlet([cfg.root_dirichlet_alpha] * cfg.action_space_size,
                                                                  n), int(B))
        return noise, self.np_random.choice(256)

    def skip_search(self, num_agents: int = 1) -> None:
        """Consume from `np_random` exactly what one search consumes -- the Dirichlet rows of the whole
        batch, then the tree seed (mcts_sampled.py:68,89) -- and launch nothing: the search of an empty
        root shard (`device_root_offset`), which keeps this rank's generator in step with the others'.
        `num_agents`: the model's agent count where the other ranks run batch_search_joint."""
        if self.root_shard is None or self.root_shard[0] != self.root_shard[1]:
            raise ValueError(f"skip_search: root shard {self.root_shard} is not empty")
        skip_search_draws(self.config, self.np_random, self.root_shard[2], num_agents)

    def draw_root_uniforms(self, B: int) -> np.ndarray:
        """One double per root in root order, as B np_random.choice(n, p) calls draw them."""
        return np.asarray(self.draw_rows(lambda n: self.np_random.random(n), B), dtype=np.float64)

    def _tree(self, B, seed, device, agent_num: int = 1, segments=None, wide_joint: bool = False):
        """The cached handle of this geometry, reseeded.  `agent_num` > 1: joint-action trees
        (batch_search_joint); what the handle refuses (A > 64, K > 64, N * A > 4096; with `wide_joint`,
        Tree_batch's, A > 255, K > 255, N * A > 4096) raises here.
        `segments` = (first_tree, seeds, root_offsets): the trees of several searches
        (Tree_batch.set_seed_segments)."""
        cfg = self.config
        # (pb_c_base, pb_c_init) select the handle's pUCT tables, which a graph replay does not
        # rewrite: a handle serves one pair only
        key = (threading.get_ident(), B, cfg.action_space_size, cfg.sampled_action_times, cfg.num_simulations,
               float(cfg.tree_value_stat_delta_lb), float(cfg.mcts_rho), float(cfg.mcts_lambda),
               float(cfg.pb_c_base), float(cfg.pb_c_init), str(device), id(self._lib),
               _DEVICE_OFFSET if self.device_root_offset else self._root_offset(), int(agent_num),
               bool(wide_joint))
        with _LOCK:
            tb = _TREES.get(key)
            if tb is None:
                tb = Tree_batch(B, int(agent_num), cfg.action_space_size, cfg.sampled_action_times,
                                cfg.num_simulations,
                                cfg.tree_value_stat_delta_lb, int(seed), cfg.mcts_rho, cfg.mcts_lambda,
                                root_offset=0 if self.device_root_offset else self._root_offset(),
                                lib=self._lib, wide_joint=bool(wide_joint))
                _TREES[key] = tb
                while len(_TREES) > max(_MAX_TREES, 1):  # least recently used first, with its loops
                    _, old = _TREES.popitem(last=False)
                    _evict_loops_of(old)
            else:
                _TREES.move_to_end(key)
                tb.reseed(int(seed))
            # (in the stream order of the reseed: the next prepare, eager or replayed, reads both words)
            if self.device_root_offset and tb.root_offset != self._root_offset():
                tb.set_root_offset(self._root_offset())
            # per-segment seeds (batch_search_many), in the same stream order; a plain search on a handle
            # that a merged search used last returns it to its (seed, root_offset) words
            if segments is not None:
                tb.set_seed_segments(*segments)
            elif tb._segmented:
                tb.set_seed_segments([], [])
            return tb

    def _root_offset(self) -> int:
        return 0 if self.root_shard is None else self.root_shard[0]

    # ---------------------------------------------------------------------------------------
    def batch_search(self, model, network_output, current_agent_idx: int, factor: np.ndarray,
                     true_num_agents: int, legal_actions_lst: np.ndarray = None, device: torch.device = None,
                     add_noise: bool = False, sampled_tau: float = 1.0,
                     sampled_actions_res: Tuple[np.ndarray, np.ndarray] = None) -> SearchOutput:
        """mcts_sampled.py:34-200; results identical to the reference driver given the same model."""
        out = self.batch_search_device(model, network_output, current_agent_idx, factor, true_num_agents,
                                       legal_actions_lst, device, add_noise, sampled_tau, sampled_actions_res,
                                       _host_readback=True)
        return out

    def batch_search_device(self, model, network_output, current_agent_idx: int, factor, true_num_agents: int,
                            legal_actions_lst=None, device=None, add_noise: bool = False, sampled_tau: float = 1.0,
                            sampled_actions_res=None, _host_readback: bool = False, _joint: bool = False):
        """The search with device-resident outputs (DeviceSearchOutput), for on-device consumers."""
        if sampled_actions_res is not None:
            raise NotImplementedError  # as the reference, mcts_sampled.py:108-109
        N, cur = int(true_num_agents), int(current_agent_idx)
        # a joint search (batch_search_joint_device): no current agent; None selects every agent's root
        # inputs, and _JOINT_AGENT stands in the loop's key where a per-agent loop has its agent
        root_agent, cur = (None, 0) if _joint else (cur, cur)
        hidden = network_output.hidden_state
        if not (isinstance(hidden, torch.Tensor) and hidden.is_cuda):
            raise ValueError("network_output.hidden_state must be a GPU tensor")
        dev = hidden.device
        B = hidden.shape[0]
        # Bc: the root count of the tree handle and the loop (root_capacity, else the batch's own)
        Bc = B if self.root_capacity is None else self.root_capacity
        if B > Bc:
            raise ValueError(f"batch of {B} roots exceeds root_capacity={Bc}")
        if B < 1:
            raise ValueError("batch of 0 roots: an empty root shard searches nothing (skip_search)")

        raw = self.root_raw(network_output, root_agent, legal_actions_lst, add_noise) if self.device_root else None
        if raw is not None:
            root_arrays, root_mode, eps, seed = raw
        else:
            (rr, rv, rp, rb, eps, rn), seed = self.root_inputs(network_output, root_agent, legal_actions_lst,
                                                               add_noise, sampled_tau)
            root_arrays, root_mode = (rr, rv, rp, rb, rn), None
        return self._search(model, hidden, root_arrays, root_mode, eps, seed, factor, N, cur, sampled_tau, Bc,
                            _joint, _host_readback)

    def _search(self, model, hidden, root_arrays, root_mode, eps, seed, factor, N, cur, sampled_tau, Bc,
                _joint=False, _host_readback=False, segments=None, mixed=False):
        """The search behind the root draws: the handle and the loop of Bc roots, the load, the run or the
        replay, the readback.  `segments`: a merged search's (batch_search_many_device), which returns the
        whole handle's rows.  `mixed`: its rows are of different agents; `factor` is then the pair (the rows'
        agents, their factor columns) on the device and `cur` is unused."""
        cfg = self.config
        disc = cfg.discount
        A, S = cfg.action_space_size, cfg.num_simulations
        dev = hidden.device
        B = hidden.shape[0]
        with torch.cuda.device(dev):
            wide_joint = bool(_joint and self.wide_joint)
            tb = self._tree(Bc, seed, dev, N if _joint else 1, segments, wide_joint)
            # the discount is a kernel argument of the recorded launches; a segmented loop records the
            # prepare kernel that reads the per-tree seed table
            key = (threading.get_ident(), id(tb), id(model), N,
                   _JOINT_AGENT if _joint else _MIXED_AGENTS if mixed else cur, float(eps),
                   float(sampled_tau), float(disc),
                   (Bc,) + tuple(hidden.shape[1:]), hidden.dtype, root_mode, wide_joint, self.wide_actions,
                   self.fused_transforms, self.wide_supports, self.later_action_cache) + (() if segments is None else (_SEGMENTED,))
            with _LOCK:
                for k in [k for k, v in _LOOPS.items() if v.model_ref() is None]:
                    del _LOOPS[k]  # loops (graph, pool) of models that no longer exist
                st = _LOOPS.get(key)
                sig = _storage_signature(model)
                # ids are reused once an object is freed; a recorded graph reads the parameters at the
                # addresses it was recorded with (re-homed weights, weights.FlatWeights, need a new one)
                if st is None or st.model_ref() is not model or st.storage != sig or st.tb is not tb:
                    st = _LOOPS[key] = _SearchLoop(tb, Bc, A, N, cur, hidden, dev, model, root_mode,
                                                   wide=self.wide_actions, fused=self.fused_transforms,
                                                   wide_supports=self.wide_supports,
                                                   later_slots=S + 1 if self.later_action_cache else 0,
                                                   joint=_joint, mixed=mixed, wide_joint=wide_joint)
                    st.storage = sig
                _LOOPS.move_to_end(key)
                while len(_LOOPS) > max(_MAX_LOOPS, 1):  # least recently used first
                    _LOOPS.popitem(last=False)
            st.load(hidden, root_arrays, factor)
            with torch.no_grad():
                if self.use_graph and st.runs > 0 and st.graph is None:
                    st.capture(model, cfg, eps, sampled_tau)  # (records only: nothing runs)
                if self.use_graph and st.runs > 0 and st.graph:
                    st.graph.replay()
                    if st.fused_rb:  # (its last launch left the packed readback)
                        tb.readback_ready(disc)
                    else:
                        tb.state_changed()
                else:
                    st.run(model, cfg, eps, sampled_tau)  # eager (the first search also warms up)
                st.runs += 1
            # the handle may serve searches of other root counts (root_capacity): the getters and the
            # consumers see this search's B rows
            if tb.active_roots != B:
                tb.set_active_roots(B)

            if _host_readback:  # :176-191 (one packed device->host copy)
                return SearchOutput(
                    tb.get_roots_values(), tb.get_roots_marginal_visit_count(), tb.get_roots_marginal_priors(),
                    tb.get_roots_sampled_actions(), tb.get_roots_sampled_visit_count(),
                    tb.get_roots_sampled_pred_probs(), tb.get_roots_sampled_beta(), tb.get_roots_sampled_beta_hat(),
                    tb.get_roots_sampled_priors(), tb.get_roots_sampled_imp_ratio(),
                    tb.get_roots_sampled_pred_values(), tb.get_roots_sampled_mcts_values(),
                    tb.get_roots_sampled_rewards(), tb.get_roots_sampled_qvalues(disc))
            # every output in one readback launch (mz_get_roots_device)
            W, Nt = tb.max_children(), tb.agent_num  # (the trees' agent_num, mcts_sampled.py:89)
            value = torch.empty(B, dtype=torch.float32, device=dev)
            mv = torch.empty(B, Nt, A, dtype=torch.int32, device=dev)
            mp = torch.empty(B, Nt, A, dtype=torch.float32, device=dev)
            deg = torch.empty(B, dtype=torch.int32, device=dev)
            sampled = {f: torch.empty(B, W * Nt if f == "actions" else W,
                                      dtype=torch.int32 if f in INT_FIELDS else torch.float32, device=dev)
                       for f in _SAMPLED_FIELDS}
            tb.get_roots_device(disc, values=value, marginal_visit_count=mv, marginal_priors=mp, degrees=deg,
                                sampled=sampled)
            return DeviceSearchOutput(value, mv, mp, deg, sampled, tb)

    # ---------------------------------------------------------------------------------------
    def batch_search_many(self, model, network_outputs: list, current_agent_idx, factors: list,
                          true_num_agents: int, legal_actions_lsts: list = None, device: torch.device = None,
                          add_noise=False, sampled_tau=1.0, draws: list = None) -> List[SearchOutput]:
        """Several independent searches of one agent as one search over the concatenated roots: entry g
        of the result equals, field by field and bit by bit, what the g-th of the consecutive calls
        `batch_search(model, network_outputs[g], current_agent_idx, factors[g], true_num_agents,
        legal_actions_lsts[g], device, add_noise, sampled_tau)` returns, and `np_random` ends in the
        state those calls leave: per entry and in order, dirichlet(B_g) then choice(256)
        (mcts_sampled.py:68,89).  `draws`: per entry the (noise, seed) pair of an earlier
        `draw_search(B_g)`, for searches whose draws the caller made in the reference's order before
        grouping them otherwise; nothing is drawn here then.

        One tree handle and one recorded loop of sum(B_g) roots -- or of `root_capacity` C >= sum(B_g),
        padded as batch_search pads -- whose trees are seeded per segment (Tree_batch.set_seed_segments:
        entry g's tree i is tree i of a fresh Tree_batch under entry g's seed).  The guarantee is
        `root_capacity`'s: exact whenever row i of the model's outputs and of the transforms does not
        depend on how many rows the batch has.  `fused_transforms`, `wide_supports`,
        `later_action_cache`, `wide_actions` and `root_capacity` compose.  `current_agent_idx`,
        `add_noise` and `sampled_tau` may be per-entry sequences; entries that differ in them or in their
        dtypes, a `root_shard`, and sum(B_g) over the capacity raise ValueError before anything launches
        (the joint search has no merged form: batch_search_joint).  On a `mixed_agents` driver the entries'
        agents may differ: entry g is then the search of agent current_agent_idx[g], on one loop whose
        agent is a per-row device table; an agent outside [0, true_num_agents), or an entry of agent
        cur_g > 0 without a factor of at least cur_g columns, raises ValueError before anything is drawn."""
        whole, bounds = self.batch_search_many_device(model, network_outputs, current_agent_idx, factors,
                                                      true_num_agents, legal_actions_lsts, device, add_noise,
                                                      sampled_tau, draws, _host_readback=True)
        return [SearchOutput(*[np.ascontiguousarray(f[lo:hi]) if isinstance(f, np.ndarray) else list(f[lo:hi])
                               for f in whole]) for lo, hi in zip(bounds[:-1], bounds[1:])]

    def batch_search_many_device(self, model, network_outputs: list, current_agent_idx, factors: list,
                                 true_num_agents: int, legal_actions_lsts: list = None, device=None,
                                 add_noise=False, sampled_tau=1.0, draws: list = None,
                                 _host_readback: bool = False):
        """batch_search_many with device-resident outputs: (the whole handle's DeviceSearchOutput, the row
        bounds [0, B_0, B_0 + B_1, ...]); entry g's rows are [bounds[g], bounds[g + 1]) of every tensor
        (`slice_search_output`).  The consumers that take their row count from the handle
        (mazero_amd.consume) run over the whole output."""
        G = len(network_outputs)
        if G < 1:
            raise ValueError("batch_search_many: no entries")

        def same(x, what):  # a scalar for every entry, or one per entry, all equal
            if isinstance(x, (list, tuple, np.ndarray)):
                vals = list(x)
                if len(vals) != G:
                    raise ValueError(f"batch_search_many: {len(vals)} {what} values for {G} entries")
                if any(v != vals[0] for v in vals[1:]):
                    raise ValueError(f"batch_search_many: the entries differ in {what} ({vals}); searches of "
                                     "different agents, noise settings or temperatures do not merge")
                return vals[0]
            return x

        N = int(true_num_agents)
        # entries of different agents: one loop with the agent per row (mixed_agents); a sequence naming one
        # agent is that agent's merged search
        curs = None
        if self.mixed_agents and isinstance(current_agent_idx, (list, tuple, np.ndarray)):
            curs = [int(c) for c in current_agent_idx]
            if len(curs) != G:
                raise ValueError(f"batch_search_many: {len(curs)} current_agent_idx values for {G} entries")
            if all(c == curs[0] for c in curs[1:]):
                curs = None
        mixed = curs is not None
        cur = 0 if mixed else int(same(current_agent_idx, "current_agent_idx"))
        add_noise = bool(same(add_noise, "add_noise"))
        sampled_tau = float(same(sampled_tau, "sampled_tau"))
        if self.root_shard is not None:
            raise ValueError(f"batch_search_many with root_shard={self.root_shard}: a rank's draws are sliced from "
                             "the whole batch's; merged searches across root shards are not supported")
        factors = [None] * G if factors is None else list(factors)
        legal_actions_lsts = [None] * G if legal_actions_lsts is None else list(legal_actions_lsts)
        if len(factors) != G or len(legal_actions_lsts) != G or (draws is not None and len(draws) != G):
            raise ValueError(f"batch_search_many: factors, legal_actions_lsts and draws must hold {G} entries")
        hiddens = [o.hidden_state for o in network_outputs]
        for hd in hiddens:
            if not (isinstance(hd, torch.Tensor) and hd.is_cuda):
                raise ValueError("network_output.hidden_state must be a GPU tensor")
            if hd.shape[0] < 1:
                raise ValueError("batch_search_many: an entry of 0 roots")
        sizes = [int(hd.shape[0]) for hd in hiddens]
        total = sum(sizes)
        Bc = total if self.root_capacity is None else self.root_capacity
        if total > Bc:
            raise ValueError(f"entries of {sizes} roots, {total} together, exceed root_capacity={Bc}")

        def kind(o, legal):  # what has to agree for the entries' rows to share the loop's buffers
            lg = o.policy_logits
            if getattr(lg, "ndim", 0) != 3:
                raise ValueError("batch_search_many takes per-agent searches ([B, num_agents, A] logits); the joint "
                                 "search has no merged form")
            return (str(lg.dtype).replace("torch.", ""), isinstance(lg, torch.Tensor), str(o.hidden_state.dtype),
                    tuple(o.hidden_state.shape[1:]), o.hidden_state.device, legal is not None,
                    None if legal is None else _np(legal).dtype.kind in "iub")

        kinds = [kind(o, la) for o, la in zip(network_outputs, legal_actions_lsts)]
        if any(k != kinds[0] for k in kinds[1:]):
            raise ValueError(f"batch_search_many: the entries differ in dtype, device or legal-action form: {kinds}")
        if cur > 0 and any(f is None for f in factors):
            raise ValueError(f"batch_search_many: agent {cur} needs every entry's factor")
        if mixed:  # (the glue kernels clamp what the table holds; the driver refuses it here)
            for g, c in enumerate(curs):
                if not 0 <= c < N:
                    raise ValueError(f"batch_search_many: entry {g} names agent {c} of {N} (current_agent_idx)")
                if c > 0 and (factors[g] is None or getattr(factors[g], "ndim", 0) != 2 or factors[g].shape[1] < c):
                    raise ValueError(f"batch_search_many: entry {g} of agent {c} needs a factor of at least {c} "
                                     "columns, the previous agents' actions")

        # the draws, entry after entry in the reference's order, then each entry's root inputs
        parts, seeds, modes, epss = [], [], [], []
        for g in range(G):
            d = None if draws is None else draws[g]
            cur_g = curs[g] if mixed else cur
            raw = self.root_raw(network_outputs[g], cur_g, legal_actions_lsts[g], add_noise, draw=d) \
                if self.device_root else None
            if raw is not None:
                arrays, mode, eps, seed = raw
            else:
                (rr, rv, rp, rb, eps, rn), seed = self.root_inputs(network_outputs[g], cur_g, legal_actions_lsts[g],
                                                                   add_noise, sampled_tau, draw=d)
                arrays, mode = (rr, rv, rp, rb, rn), None
            parts.append(arrays)
            seeds.append(int(seed))
            modes.append(mode)
            epss.append(eps)
        if any(m != modes[0] for m in modes[1:]):
            raise ValueError(f"batch_search_many: the entries take different root paths: {modes}")
        root_mode, eps = modes[0], epss[0]

        def cat(xs):
            if all(isinstance(x, torch.Tensor) for x in xs):
                return torch.cat([x.reshape(x.shape[0], -1) for x in xs], 0)
            return np.concatenate([np.asarray(x).reshape(np.asarray(x).shape[0], -1) for x in xs], 0)

        if root_mode is not None:
            root_arrays = {k: cat([p[k] for p in parts]) for k in parts[0]}
        else:
            root_arrays = tuple(cat([p[i] for p in parts]) for i in range(5))
        hidden = torch.cat(hiddens, 0)
        dev = hidden.device
        factor = None
        if cur > 0:
            factor = torch.cat([torch.as_tensor(np.ascontiguousarray(_np(f)[:, :cur]) if not isinstance(f, torch.Tensor)
                                                else f[:, :cur]).to(device=dev, dtype=torch.int32) for f in factors], 0)
        if mixed:  # the table, and each row's first cur_g factor columns with zeros behind them
            fac = torch.zeros(total, max(N - 1, 1), dtype=torch.int32, device=dev)
            lo = 0
            for c, b, f in zip(curs, sizes, factors):
                if c > 0:
                    fac[lo:lo + b, :c] = torch.as_tensor(f[:, :c] if isinstance(f, torch.Tensor) else
                                                         np.ascontiguousarray(_np(f)[:, :c])).to(dev, torch.int32)
                lo += b
            factor = (torch.from_numpy(np.repeat(np.asarray(curs, np.int32), sizes)).to(dev), fac)
        bounds = [0]
        for b in sizes:
            bounds.append(bounds[-1] + b)
        # (the last segment runs to the handle's root count: under root_capacity the padding trees
        # continue the last entry's batch, and nobody reads them)
        segments = (bounds[:-1], seeds, [0] * G)
        out = self._search(model, hidden, root_arrays, root_mode, eps, seeds[0], factor, N, cur, sampled_tau, Bc,
                           False, _host_readback, segments=segments, mixed=mixed)
        return out, bounds

    # ---------------------------------------------------------------------------------------
    def batch_search_joint(self, model, network_output, legal_actions_lst: np.ndarray = None,
                           device: torch.device = None, add_noise: bool = False, sampled_tau: float = 1.0,
                           sampled_actions_res: Tuple[np.ndarray, np.ndarray] = None) -> SearchOutput:
        """One search over the joint-action trees of all agents: the call of the reference's evaluation
        loop, `SampledMCTS(config, np_random).batch_search(model, network_output, legal_actions_lst,
        device, False, 1.0)` (core/test.py:84), whose `roots_sampled_actions[i][action_pos]` is the whole
        joint action (:101-107).

        It is mcts_sampled.py:34-200 with num_agents = N, the model's agent count
        (`network_output.policy_logits.shape[1]`), in place of 1 (:53,89): the root policy, the Dirichlet
        noise ((B, N) rows, drawn before the tree seed as :68,89), the legal mask and beta are [B, N, A];
        every node samples K joint actions; the selection returns all N agents' actions (:123-124), so
        there is no factor, no prediction pass for later agents (:116-121, :136-147 go) and
        `recurrent_inference(leaf, batch_actions)` takes them as they are; the policy glue of every
        simulation covers all agents' logits (:156).  In the result `marginal_*` are [B, N, A] and
        `sampled_actions[i]` is (K_i, N).  With N = 1 the trees, the kernels and the results are those of
        `batch_search(model, network_output, 0, None, 1, ...)`.

        On the device: one packed upload of the raw root inputs, mz_root_glue_joint, then per simulation
        the selection's [B, N] actions widened into the model's int64 action buffer, the model, and
        mz_policy_glue_joint, around the fused tree kernel; the first search is eager, later ones replay
        one recorded graph.  `fused_transforms`, `wide_supports` and `root_shard` compose;
        `root_capacity`, `later_action_cache` and `wide_actions` raise ValueError.  What the tree handle
        refuses for N > 1 (A > 64, K > 64, N * A > 4096) raises from Tree_batch before anything launches.
        With the constructor's `wide_joint` the handle is mz_create_wide_joint's and the glue the
        _joint_wide entry points: A <= 255 and K <= 255 (N <= 64, N * A <= 4096)."""
        return self.batch_search_joint_device(model, network_output, legal_actions_lst, device, add_noise,
                                              sampled_tau, sampled_actions_res, _host_readback=True)

    def batch_search_joint_device(self, model, network_output, legal_actions_lst=None, device=None,
                                  add_noise: bool = False, sampled_tau: float = 1.0, sampled_actions_res=None,
                                  _host_readback: bool = False):
        """batch_search_joint with device-resident outputs (DeviceSearchOutput; consume.select_joint_actions
        takes the joint actions from it)."""
        for flag, on in (("root_capacity", self.root_capacity is not None),
                         ("later_action_cache", self.later_action_cache), ("wide_actions", self.wide_actions)):
            if on:
                raise ValueError(f"batch_search_joint does not take {flag}: " + {
                    "root_capacity": "the padded loop is the per-agent one",
                    "later_action_cache": "a joint search estimates no later agents' actions",
                    "wide_actions": "joint-action trees take at most 64 actions per agent "
                                    "(wide_joint: up to 255)"}[flag])
        logits = network_output.policy_logits
        if getattr(logits, "ndim", 0) != 3:
            raise ValueError("network_output.policy_logits must be [B, num_agents, A]")
        return self.batch_search_device(model, network_output, 0, None, int(logits.shape[1]), legal_actions_lst,
                                        device, add_noise, sampled_tau, sampled_actions_res,
                                        _host_readback=_host_readback, _joint=True)

    @staticmethod
    def _recurrent(model, hidden, action):
        """(next_h, reward [B,1], value [B,1], policy_logits [B,N,A]) on the device, as
        MAMuZeroNet.recurrent_inference computes them in eval mode (config/smac/model.py:562-572)."""
        fn = getattr(model, "recurrent_inference_device", None)
        if fn is not None:
            return fn(hidden, action)
        next_h, reward_logits = model.dynamics(hidden, action)
        policy_logits, value_logits = model.prediction(next_h)
        reward = model.inverse_reward_transform(reward_logits)
        value = model.inverse_value_transform(value_logits)
        return next_h, reward, value, policy_logits
