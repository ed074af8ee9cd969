"""Adversarial network outputs for whole searches: the input classes of the edge tests, in one place.

`mazero_amd.synthetic.make_search_inputs` is benign: beta equals policy at every non-root node,
policies are softmax(N(0,1)) (no zeros, no subnormals, no near-one-hot rows), values and rewards
are of order one, and every tree of a batch is alike.  Each function here takes a `SearchInputs`
and returns one with a single such property broken, in float32 the way a caller would produce it:

    f(inp, trees=None) -> SearchInputs

`trees=None` alters every tree; a list of tree indices alters those and leaves every array of the
other trees byte-identical, so one launch holds trees whose state diverges.  `EDGE_CLASSES` is the
registry the tests loop over (tests/test_oracle.py: the CPU port against the reference ctree;
tests/test_edge_inputs.py: every kernel family against the port).

The builders the k_chain3 tests were written with (`concentrated`, `wild_prior`, `wild_value`,
`wild_reward`, `masked`, `tiny_tail`) live here too and are imported back into those tests under
their old names; with `trees=None` they return what they always returned.

Out of the reference's domain, so not a class: NaN.  A NaN value makes the reference ctree throw
(`CMinMaxStats::remove: value not found`: its multiset cannot find a NaN again), so there is
nothing to compare a kernel with.
"""
from __future__ import annotations

from dataclasses import replace

import numpy as np

F32_MIN_NORMAL = np.float32(np.finfo(np.float32).tiny)  # 2^-126: below it a float32 is subnormal

_ROOT = ("root_reward", "root_value", "root_policy", "root_beta", "root_noise")  # [B, ...]
_SIM = ("reward", "value", "policy", "beta")  # [S, B, ...]


def _only(inp, new, trees):
    """`new` on the trees listed, `inp` (byte for byte) on the others."""
    if trees is None:
        return new
    trees = np.asarray(sorted(set(int(t) for t in trees)), np.int64)
    assert trees.size and 0 <= trees[0] and trees[-1] < inp.B, (trees, inp.B)
    kw = {}
    for name in _ROOT + _SIM:
        a, b = getattr(inp, name), getattr(new, name)
        if a is b:
            continue
        assert a.shape == b.shape and a.dtype == b.dtype == np.float32, name
        c = a.copy()
        if name in _ROOT:
            c[trees] = b[trees]
        else:
            c[:, trees] = b[:, trees]
        kw[name] = c
    return replace(inp, **kw)


def _rng(inp, tag):
    """A generator of the class's own, fixed by the inputs it alters."""
    return np.random.default_rng([int(inp.seed), inp.B, inp.A, inp.S, tag])


def _renorm(x):
    return (x / x.sum(axis=-1, keepdims=True, dtype=np.float32)).astype(np.float32)


def _softmax32(x):
    """softmax in float64, rounded to float32 once: what underflows becomes subnormal, then zero."""
    e = np.exp(x - np.max(x, axis=-1, keepdims=True))
    return (e / np.sum(e, axis=-1, keepdims=True)).astype(np.float32)


def is_subnormal(a):
    return (a > 0) & (a < F32_MIN_NORMAL)


# ---- beta != policy: a sampling temperature ----
def _beta_tau(inp, tau, trees):
    beta = _renorm(inp.policy ** np.float32(1.0 / tau))
    return _only(inp, replace(inp, beta=beta), trees)


def beta_tau2(inp, trees=None):
    """Non-root beta = renorm(policy ** (1 / 2)); policy unchanged."""
    return _beta_tau(inp, 2.0, trees)


def beta_tau05(inp, trees=None):
    """Non-root beta = renorm(policy ** 2); policy unchanged."""
    return _beta_tau(inp, 0.5, trees)


def beta_rolled(inp, trees=None):
    """Non-root beta = the policy of the next action (the row rolled by one): the same weights in
    another order, so the two rows rank the actions differently (a temperature keeps the ranking, and
    with many draws a prior computed from the wrong row then selects the same children)."""
    return _only(inp, replace(inp, beta=np.roll(inp.policy, -1, axis=-1)), trees)


# ---- exact zeros ----
def _mask(inp, legal):
    return replace(inp, policy=np.where(legal, inp.policy, np.float32(0)), beta=np.where(legal, inp.beta, np.float32(0)))


def masked(B, A, S, seed):
    """40 % zero beta entries on the root's row and on every simulation's (action 1 stays legal)."""
    from mazero_amd.synthetic import make_search_inputs

    inp = make_search_inputs(np.random.default_rng(seed), B, A, S, legal_zero_frac=0.4)
    legal = np.random.default_rng(seed + 1).random(inp.beta.shape) >= 0.4
    legal[..., 0] = False
    legal[..., 1] = True
    inp = _mask(inp, legal)
    assert (inp.beta == 0).any() and (inp.beta[..., -1] == 0).any()
    return inp


def zero_entries(inp, trees=None):
    """40 % of the entries of every simulation's row zero in policy and beta alike; action 1 stays
    legal (with two actions the last one is action 1: elsewhere the last action is zero somewhere)."""
    legal = _rng(inp, 1).random(inp.beta.shape) >= 0.4
    legal[..., 1 % inp.A] = True
    altered = _sel(trees, 1)
    if inp.A > 2 and altered(legal)[..., -1].all():  # (a short search of one tree can miss it by chance)
        legal[0, 0 if trees is None else int(min(trees)), ..., -1] = False
    new = _mask(inp, legal)
    assert inp.A <= 2 or (altered(new.beta)[..., -1] == 0).any()
    return _only(inp, new, trees)


def tiny_tail(inp, trees=None):
    """The last three beta weights 1e-30 of the rest: the prefix sums before the forced 1.0 sit
    within rounding of it."""
    b = inp.beta.copy()
    b[..., -3:] = b[..., :-3].sum(axis=-1, keepdims=True) * np.float32(1e-30)
    return _only(inp, replace(inp, beta=b), trees)


# ---- near-one-hot rows: exact zeros and subnormals out of a softmax ----
def _peaked_rows(inp, shape, tag, rows):
    """softmax(90 * N(0,1)) rows.  At nine actions about 59 % of the entries are exactly zero and
    about 6 % subnormal; of up to 32 seeded draws the first whose rows `rows` hold both kinds is
    taken.  With 256 entries or more a draw without both has a probability below 1e-6, so there it
    is asserted; a few short rows (a root's, a search of four simulations) cannot always hold both."""
    first = None
    for attempt in range(32):
        p = _softmax32(90.0 * _rng(inp, [tag, attempt]).standard_normal(shape))
        if first is None:
            first = p
        q = rows(p)
        if (q == 0).any() and is_subnormal(q).any():
            return p
    assert rows(first).size < 256, "peaked rows without an exact zero and a subnormal"
    return first


def _sel(trees, axis):
    if trees is None:
        return lambda p: p
    t = sorted(set(int(x) for x in trees))
    return (lambda p: p[t]) if axis == 0 else (lambda p: p[:, t])


def peaked(inp, trees=None):
    """policy = beta = softmax(90 * N(0,1)) on every simulation's row."""
    p = _peaked_rows(inp, inp.policy.shape, 2, _sel(trees, 1))
    return _only(inp, replace(inp, policy=p, beta=p.copy()), trees)


def concentrated(inp, j, trees=None):
    """beta of every simulation with weight 1 - 1e-6 on action j."""
    A = inp.A
    b = np.full(inp.beta.shape, 1e-6 / (A - 1), np.float32)
    b[..., j] = np.float32(1.0 - 1e-6)
    return _only(inp, replace(inp, beta=b), trees)


def concentrated_first(inp, trees=None):
    return concentrated(inp, 0, trees)


def concentrated_last(inp, trees=None):
    return concentrated(inp, inp.A - 1, trees)


# ---- not tame: a prior above 1e30, a value or a reward outside +-1e30 ----
def wild_prior(inp, trees=None):
    """policy 1 and beta * 1e-31 from simulation 2 on: every prior (policy / beta) is above 1e30."""
    p, b = inp.policy.copy(), inp.beta.copy()
    p[2:] = 1.0
    b[2:] *= np.float32(1e-31)
    return _only(inp, replace(inp, policy=p, beta=b), trees)


def wild_value(inp, trees=None):
    v = inp.value.copy()
    v[2] = 1e31
    return _only(inp, replace(inp, value=v), trees)


def wild_reward(inp, trees=None):
    r = inp.reward.copy()
    r[2] = 1e31
    return _only(inp, replace(inp, reward=r), trees)


def inf_value(inp, trees=None):
    v = inp.value.copy()
    v[2] = np.inf
    return _only(inp, replace(inp, value=v), trees)


# ---- the min/max normaliser ----
def small_spread(inp, trees=None):
    """value, reward and root_value * 1e-3: max - min stays under delta_lb = 0.01 all search long."""
    k = np.float32(1e-3)
    return _only(inp, replace(inp, value=inp.value * k, reward=inp.reward * k, root_value=inp.root_value * k), trees)


def large_scale(inp, trees=None):
    """value and root_value * 300, reward * 200: what the heads' supports of +-300 can produce."""
    return _only(inp, replace(inp, value=inp.value * np.float32(300), reward=inp.reward * np.float32(200),
                              root_value=inp.root_value * np.float32(300)), trees)


def constant_value(inp, trees=None):
    """Every value 0.5, every reward 0: max == min at a non-zero q (ties=True has them at zero)."""
    return _only(inp, replace(inp, value=np.full_like(inp.value, 0.5), reward=np.zeros_like(inp.reward)), trees)


# ---- the same edges on the root's row (k_prepare, k_prepare1) ----
def root_wild_value(inp, trees=None):
    return _only(inp, replace(inp, root_value=np.full_like(inp.root_value, 1e31)), trees)


def root_wild_prior(inp, trees=None):
    """root_policy 1 and root_beta * 1e-31: every root child's prior is above 1e30."""
    return _only(inp, replace(inp, root_policy=np.ones_like(inp.root_policy),
                              root_beta=inp.root_beta * np.float32(1e-31)), trees)


def root_peaked(inp, trees=None):
    """root_policy = root_beta = softmax(90 * N(0,1))."""
    p = _peaked_rows(inp, inp.root_policy.shape, 3, _sel(trees, 0))
    return _only(inp, replace(inp, root_policy=p, root_beta=p.copy()), trees)


EDGE_CLASSES = {
    "beta_tau2": beta_tau2,
    "beta_tau05": beta_tau05,
    "beta_rolled": beta_rolled,
    "zero_entries": zero_entries,
    "peaked": peaked,
    "concentrated_first": concentrated_first,
    "concentrated_last": concentrated_last,
    "wild_prior": wild_prior,
    "wild_value": wild_value,
    "wild_reward": wild_reward,
    "inf_value": inf_value,
    "small_spread": small_spread,
    "large_scale": large_scale,
    "constant_value": constant_value,
    "root_wild_value": root_wild_value,
    "root_wild_prior": root_wild_prior,
    "root_peaked": root_peaked,
}
# the classes that clear a tree's tame flag (the exact selection of the K = 1 kernels)
WILD = ("wild_prior", "wild_value", "wild_reward", "inf_value", "root_wild_value", "root_wild_prior")


def apply(inp, names, trees=None):
    """The classes `names` one after another (a later one overwrites what it shares with an earlier)."""
    for n in names:
        inp = EDGE_CLASSES[n](inp, trees)
    return inp
