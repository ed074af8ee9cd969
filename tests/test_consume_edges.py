"""The per-root consumers (include/mzconsume.h) at the draws where one bit decides the answer.

`select_action` (core/utils.py:289-316) picks `cdf.searchsorted(u, side='right')` of numpy's `choice`: a
random uniform lies within an ulp of a cdf entry about once in 1e16 draws, so random draws never see
whether a `v ** e` term, a partial sum or the `>` is off by a bit.  Here every uniform is a cdf entry of
the reference or one of its two float64 neighbours (`boundary_draws`), for every way the kernel computes
`v ** (1 / temperature)`: the in-kernel repeated product (1/T = 1..8 while v ** e <= 2**53), and the
host-made table of libm's pow for everything else (mz_select_pow_plan).

CPU tests pin the restatement of `choice` against numpy's own generators, the kernel's arithmetic
(test_consume.kernel_cdf) against that restatement at every boundary draw, the domain of the repeated
product, and the library's table against Python's float power.  GPU tests run the kernels on the same
draws, one lane per root (root = (base row, draw)), and mz_eps_greedy / mz_marginal_policy at their own
boundaries and widest sizes.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest
import torch

from consume import eps_greedy_given, select_action
from test_consume import POW_TABLE_MAX, kernel_cdf, kernel_pow_plan, kernel_select

INTEGER_T = [1.0, 0.5, 1 / 3, 0.25, 0.2, 1 / 6, 1 / 7, 0.125]  # 1/T = 1..8
OTHER_T = [0.1, 0.3, 0.7, 1.5, 2.0]  # 1/T = 10.0 (an integer above the product's window), then non-integers
# (temperature, largest visit count)
CLASSES = [(t, vmax) for t in INTEGER_T + OTHER_T for vmax in (60, 300, 3000)] + [(0.25, 20000)]
WIDTHS = (1, 2, 7, 8, 9, 64, 255)
GARBAGE = 2 ** 31 - 1  # what the padding past a row's degree holds: never read


def class_id(c):
    return f"T{c[0]:.4g}-v{c[1]}"


def class_rows(temperature, vmax):
    """The 28 base rows of a class: two random rows of every width in WIDTHS, six of a random width up
    to 20, rows with leading, inner and trailing zero counts, rows of all-equal counts, rows with one
    nonzero count.  Counts are uniform in 0..vmax."""
    rng = np.random.default_rng(int(round(1000 / temperature)) * 100003 + vmax)
    draw = lambda n: rng.integers(0, vmax + 1, size=n)  # noqa: E731
    rows = [draw(w) for w in WIDTHS for _ in range(2)]
    rows += [draw(int(rng.integers(3, 21))) for _ in range(6)]
    lead, inner, trail = draw(9), draw(12), draw(9)
    lead[:3] = 0
    inner[[2, 3, 7]] = 0
    trail[-3:] = 0
    rows += [lead, inner, trail, np.full(9, vmax), np.full(64, max(1, vmax // 7))]
    for at in (0, 4, 8):
        one = np.zeros(9, np.int64)
        one[at] = int(rng.integers(1, vmax + 1))
        rows.append(one)
    for r in rows:
        if r.sum() == 0:
            r[len(r) // 2] = max(1, vmax // 2)
    return [r.astype(np.int32) for r in rows]


def reference_cdf(row, temperature):
    """The cdf numpy's `choice(n, p=probs)` searches, from select_action's own expressions
    (core/utils.py:302-306, then `cdf = p.cumsum(); cdf /= cdf[-1]`)."""
    p = [int(v) ** (1 / temperature) for v in row]
    total = sum(p)
    cdf = np.array([x / total for x in p]).cumsum()
    cdf /= cdf[-1]
    return cdf


def boundary_draws(row, temperature):
    """(uniforms, expected child): every entry of cdf[:-1] with its two float64 neighbours (values >= 1.0
    skipped: `random()` never returns them), then 0.0 and the largest double below 1."""
    cdf = reference_cdf(row, temperature)
    us = []
    for c in cdf[:-1]:
        us += [u for u in (np.nextafter(c, 0.0), c, np.nextafter(c, 1.0)) if u < 1.0]
    us += [0.0, np.nextafter(1.0, 0.0)]
    u = np.array(us, np.float64)
    return u, cdf.searchsorted(u, side="right")


_DRAWS = {}


def class_draws(cls):
    """[(row, uniforms, expected)] of a class, computed once and shared (read-only)."""
    if cls not in _DRAWS:
        out = []
        for r in class_rows(*cls):
            u, exp = boundary_draws(r, cls[0])
            u.setflags(write=False)
            exp.setflags(write=False)
            out.append((r, u, exp))
        _DRAWS[cls] = out
    return _DRAWS[cls]


def kernel_positions(row, temperature, u):
    """kernel_select at every uniform of u at once: the first j with c_j / last > u, else the last child."""
    cdf = kernel_cdf(row, temperature)
    if cdf is None:
        return np.full(len(u), -1)
    gt = np.asarray(cdf)[None, :] > np.asarray(u)[:, None]
    return np.where(gt.any(axis=1), gt.argmax(axis=1), len(row) - 1)


# ------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------
def test_the_integer_temperatures_give_the_integer_exponents():
    assert [1 / t for t in INTEGER_T] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    assert 1 / 0.1 == 10.0
    assert all(1 / t != math.floor(1 / t) for t in OTHER_T[1:])


@pytest.mark.parametrize("gen", ["generator", "randomstate"])
@pytest.mark.parametrize("cls", [(1.0, 3000), (0.125, 300), (0.25, 20000), (0.1, 300), (0.3, 3000), (1.5, 60)],
                         ids=class_id)
def test_reference_cdf_is_numpy_choice(gen, cls):
    """`reference_cdf(row, T).searchsorted(u, 'right')` with u = one `random()` is what select_action's
    `np_random.choice(n, p=probs)` returns, for Generator and RandomState, on this file's rows (1 to 255
    children, counts up to 20,000): the boundary tests below stand on numpy's own choice."""
    temperature = cls[0]
    rows = class_rows(*cls) * 4
    make = (lambda: np.random.Generator(np.random.PCG64(11))) if gen == "generator" else \
        (lambda: np.random.RandomState(11))
    ra, rb = make(), make()
    exp = [int(select_action([int(v) for v in r], temperature=temperature, deterministic=False, np_random=ra)[0])
           for r in rows]
    u = rb.random(len(rows))
    got = [int(reference_cdf(r, temperature).searchsorted(u[i], side="right")) for i, r in enumerate(rows)]
    assert got == exp
    assert ra.random() == rb.random()


@pytest.mark.parametrize("cls", CLASSES, ids=class_id)
def test_kernel_arithmetic_at_boundary_draws(cls):
    """The kernel's arithmetic (test_consume.kernel_cdf: product or host pow, left-to-right sums, IEEE
    divisions, c / last > u) picks numpy's child at every boundary draw of the class.

    The arithmetic of the commit before this file (the repeated product for every 1/T in 1..8, whatever
    the count) picks another child at T = 0.125 with counts <= 300 on 241 of these 2,630 draws (6 of the 28
    rows); the other classes it fails are in the table of test_select_actions_at_boundary_draws."""
    temperature = cls[0]
    draws = class_draws(cls)
    # the cap on skipped draws: at least two boundary draws a row on average survive the `>= 1.0` skip
    assert sum(len(u) for _, u, _ in draws) >= 2 * len(draws)
    bad = rows_bad = 0
    for row, u, exp in draws:
        got = kernel_positions(row, temperature, u)
        n = int((got != exp).sum())
        bad += n
        rows_bad += n > 0
    assert bad == 0, f"{bad} of {sum(len(u) for _, u, _ in draws)} draws ({rows_bad} rows) pick another child"


def test_kernel_positions_is_kernel_select():
    """The vectorised pick above is kernel_select's loop."""
    for cls in [(0.125, 300), (0.3, 3000), (1.0, 60)]:
        for row, u, _ in class_draws(cls)[::3]:
            got = kernel_positions(row, cls[0], u[:40])
            assert [kernel_select(list(row), cls[0], False, x) for x in u[:40]] == got.tolist()


def test_boundary_draws_cover_every_edge():
    """The generator itself: three draws around every cdf entry below 1, both ends, all inside [0, 1)."""
    row = np.array([0, 3, 0, 5, 2, 0], np.int32)
    u, exp = boundary_draws(row, 1.0)
    # cdf = [0, .3, .3, .8, 1, 1]: three draws at each of the first four entries, one below the 1.0, two ends
    assert len(u) == 3 * 4 + 1 + 2 and (u >= 0).all() and (u < 1).all()
    assert set(exp.tolist()) == {1, 3, 4}  # never a child without visits
    assert exp[-2] == 1 and exp[-1] == 4  # u = 0 skips the leading zero; u -> 1 stays off the trailing one
    u1, exp1 = boundary_draws(np.array([7], np.int32), 0.3)
    assert u1.tolist() == [0.0, np.nextafter(1.0, 0.0)] and exp1.tolist() == [0, 0]


@pytest.fixture(scope="module")
def product_lib():
    from mazero_amd._lib import load

    return load()  # (loads without a GPU; mz_select_pow_plan makes no device call)


def _pow_plan(lib, temperature, table_len=0):
    ipow, exact_max, uses = C.c_int32(), C.c_int32(), C.c_int32()
    table = (C.c_double * table_len)() if table_len else None
    rc = lib.mz_select_pow_plan(float(temperature), C.byref(ipow), C.byref(exact_max), C.byref(uses), table,
                                table_len)
    assert rc == 0
    return ipow.value, exact_max.value, bool(uses.value), np.array(table[:], np.float64) if table_len else None


def test_product_domain_is_where_it_is_exact(product_lib):
    """For e in 1..8 and v in 0..20000 the in-kernel product is used only where every partial product is
    <= 2**53 (Python's integers), and there it is `float(v) ** e`; the library's plan is the restated one."""
    for e in range(1, 9):
        temperature = INTEGER_T[e - 1]
        ipow, exact_max, uses_table, _ = _pow_plan(product_lib, temperature)
        assert (1 / temperature, ipow, exact_max) == kernel_pow_plan(temperature)
        assert ipow == e and exact_max ** e <= 2 ** 53
        assert (exact_max + 1) ** e > 2 ** 53 or exact_max == 2 ** 31 - 1  # (e = 1: every int32 count)
        assert uses_table == (exact_max < POW_TABLE_MAX)
        for v in range(0, 20001):
            exact = all(v ** k <= 2 ** 53 for k in range(1, e + 1))
            assert (v <= exact_max) == exact, (e, v)
            if exact:
                r = float(v)
                for _ in range(e - 1):
                    r *= float(v)
                assert r == float(v) ** e == float(v ** e), (e, v)
    assert [kernel_pow_plan(t)[2] for t in INTEGER_T] == [2 ** 31 - 1, 94906265, 208063, 9741, 1552, 456, 190, 98]
    for t in OTHER_T + [1 / 9, 3.0, 1e-3]:
        assert _pow_plan(product_lib, t)[:3] == (0, -1, True) and kernel_pow_plan(t)[1:] == (0, -1)


def test_pow_table_is_pythons_float_power(product_lib):
    """The table mz_select_actions uploads (the host libm's pow) is `float(v) ** (1 / T)`, bit for bit, for
    every count it covers and every temperature of this file."""
    for t in INTEGER_T[3:] + OTHER_T:
        table = _pow_plan(product_lib, t, POW_TABLE_MAX + 1)[3]
        e = 1 / t
        want = np.array([float(v) ** e for v in range(POW_TABLE_MAX + 1)], np.float64)
        assert table.tobytes() == want.tobytes(), t


def test_pow_plan_refuses_bad_arguments(product_lib):
    from mazero_amd._capi import MZ_ERR_ARG

    k = C.c_int32()
    buf = (C.c_double * 4)()
    for bad in (0.0, -1.0, float("nan")):
        assert product_lib.mz_select_pow_plan(bad, C.byref(k), C.byref(k), C.byref(k), None, 0) == MZ_ERR_ARG
    assert product_lib.mz_select_pow_plan(1.0, None, C.byref(k), C.byref(k), None, 0) == MZ_ERR_ARG
    assert product_lib.mz_select_pow_plan(1.0, C.byref(k), C.byref(k), C.byref(k), buf, POW_TABLE_MAX + 2) == MZ_ERR_ARG


def test_restatement_refuses_what_no_path_covers():
    assert kernel_select([5, POW_TABLE_MAX + 1], 0.3, False, 0.5) == -1  # past the table
    assert kernel_select([5, POW_TABLE_MAX + 1], 0.25, False, 0.5) == -1  # past the product and the table
    assert kernel_select([5, 208064], 1 / 3, False, 0.5) == -1  # past the product: 1/T = 3 has no table
    assert kernel_select([5, 208063], 1 / 3, False, 0.0) == 0
    assert kernel_select([5, 2 ** 31 - 1], 1.0, False, 0.5) == 1
    assert kernel_select([3, POW_TABLE_MAX], 0.01, False, 0.5) == -1  # the powers overflow


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
def _output(B, A, dev, N=1, degrees=None, visits=None, actions=None, marginal=None):
    """A DeviceSearchOutput over given per-root lists, bound to a fresh handle: the consumers take the
    handle's stream, active-root count, agent_num and action_space_size; the row width is the tensor's."""
    from mazero_amd.cytree import Tree_batch
    from mazero_amd.mcts_sampled import DeviceSearchOutput

    tb = Tree_batch(B, N, A, 1, 1, 0.01, 0, 0.75, 0.8)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    sampled = None if visits is None else {"visit_count": t(visits), "actions": t(actions)}
    return DeviceSearchOutput(torch.zeros(B, dtype=torch.float32, device=dev), t(marginal), None, t(degrees),
                              sampled, tb)


class Layout:
    """Boundary draws laid out as roots: root = (base row, draw), the base row repeated, padded to `width`
    with GARBAGE; B kept off the multiples of 64 (the last root once more)."""

    def __init__(self, draws, temperature, N=1, width=None, seed=0):
        rows = [d for d in draws if width is None or len(d[0]) <= width]
        self.rows = rows
        self.width = W = width or max(len(r) for r, _, _ in rows)
        base = np.concatenate([np.full(len(u), k) for k, (_, u, _) in enumerate(rows)])
        u = np.concatenate([u for _, u, _ in rows])
        exp = np.concatenate([e for _, _, e in rows])
        if len(base) % 64 == 0:
            base, u, exp = np.append(base, base[-1]), np.append(u, u[-1]), np.append(exp, exp[-1])
        self.base, self.u, self.exp = base, u, exp.astype(np.int32)
        self.B = B = len(base)
        self.N = N
        self.deg = np.array([len(rows[k][0]) for k in base], np.int32)
        self.visits = np.full((B, W), GARBAGE, np.int32)
        for i, k in enumerate(base):
            self.visits[i, : self.deg[i]] = rows[k][0]
        self.actions = np.random.default_rng(seed).integers(0, 200, size=(B, W * N)).astype(np.int32)
        # scipy's entropy of the reference's probabilities, once per base row
        ent = [select_action([int(v) for v in r], temperature=temperature, deterministic=True)[1] for r, _, _ in rows]
        self.ent = np.array(ent)[base]

    def output(self, dev, A=4):
        return _output(self.B, A, dev, self.N, self.deg, self.visits, self.actions)


def _select(out, u, temperature, deterministic=False):
    from mazero_amd.consume import select_actions

    ud = None if u is None else torch.from_numpy(np.ascontiguousarray(u)).to(out.degrees.device)
    pos, act, ent = select_actions(out, ud, temperature, deterministic)
    return pos.cpu().numpy(), act.cpu().numpy(), ent.cpu().numpy()


def _select_joint(out, u, temperature, deterministic=False):
    from mazero_amd.consume import select_joint_actions

    ud = None if u is None else torch.from_numpy(np.ascontiguousarray(u)).to(out.degrees.device)
    act, pos, ent = select_joint_actions(out, temperature, deterministic, ud)
    return pos.cpu().numpy(), act.cpu().numpy(), ent.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES, ids=class_id)
def test_select_actions_at_boundary_draws(cls):
    """mz_select_actions at every boundary draw of the class: pos and action are numpy's (`cdf.searchsorted
    (u, 'right')` of the reference's cdf), the entropy scipy's to 1e-12 relative.

    Boundary draws at which the kernels of the commit before this file chose another child than numpy,
    measured on an MI355X with this file's rows (draws differing of draws; rows affected of the 28 rows):
      the in-kernel product past 2**53 (1/T = 4..8; the Python restatement of that product gives the same
      counts on the CPU; every integer class not listed: 0)
        T = 0.25   counts <= 20000:    1 of 2,633;  1     T = 0.2    counts <= 3000:    3 of 2,498;  2
        T = 1/6    counts <= 3000:    62 of 2,558;  9     T = 1/7    counts <= 300:     2 of 2,673;  1
        T = 1/7    counts <= 3000:   217 of 2,597; 11     T = 0.125  counts <= 300:   241 of 2,630;  6
        T = 0.125  counts <= 3000:   365 of 2,629; 16
      the device pow, by counts <= 60 / <= 300 / <= 3000
        T = 0.1 (1/T = 10):    82 of 2,618;  7     18 of 2,684;  6    236 of 2,615; 10
        T = 0.3:              246 of 2,606; 15    309 of 2,642; 12    123 of 2,625; 12
        T = 0.7:              416 of 2,646; 14    215 of 2,660; 10     42 of 2,612; 12
        T = 1.5:              173 of 2,628; 13    217 of 2,636; 10    447 of 2,570; 13
        T = 2.0:              107 of 2,654; 16    261 of 2,594; 15     79 of 2,618; 13
    So the device pow is not libm's at any temperature tried, and every power outside the exact product now
    comes from the host's table.  The entropies of those kernels were within 2e-13 (relative) of scipy's."""
    temperature = cls[0]
    dev = torch.device("cuda", 0)
    lay = Layout(class_draws(cls), temperature)
    assert lay.B % 64 and lay.B >= 2 * len(lay.rows)
    pos, act, ent = _select(lay.output(dev), lay.u, temperature)
    bad = np.flatnonzero(pos != lay.exp)
    assert bad.size == 0, (f"{bad.size} of {lay.B} draws ({len(set(lay.base[bad]))} of {len(lay.rows)} rows) pick "
                           f"another child; first: root {bad[0]}, got {pos[bad[0]]}, numpy {lay.exp[bad[0]]}")
    np.testing.assert_array_equal(act, lay.actions[np.arange(lay.B), lay.exp])
    np.testing.assert_allclose(ent, lay.ent, rtol=1e-12, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", [(1.0, 60), (0.125, 300), (0.3, 3000)], ids=class_id)
@pytest.mark.parametrize("width", [20, 255, 1])
def test_select_actions_joint_at_boundary_draws(cls, width):
    """mz_select_actions_joint with N = 3 on the rows of the class that fit the width: the whole joint
    action row is the chosen child's, pos is numpy's, and pos and the entropy have the bits of
    mz_select_actions on the same inputs."""
    temperature, N = cls[0], 3
    dev = torch.device("cuda", 0)
    lay = Layout(class_draws(cls), temperature, N=N, width=width, seed=width)
    assert lay.B % 64 and (max(lay.deg) == width or (width == 20 and max(lay.deg) > 9))
    out = lay.output(dev)
    pos, act, ent = _select_joint(out, lay.u, temperature)
    np.testing.assert_array_equal(pos, lay.exp)
    assert act.shape == (lay.B, N)
    np.testing.assert_array_equal(act, lay.actions.reshape(lay.B, lay.width, N)[np.arange(lay.B), lay.exp])
    pos1, act1, ent1 = _select(out, lay.u, temperature)
    np.testing.assert_array_equal(pos1, pos)
    np.testing.assert_array_equal(act1, act[:, 0])
    np.testing.assert_array_equal(_bits(ent1), _bits(ent))
    np.testing.assert_allclose(ent, lay.ent, rtol=1e-12, atol=0)


def _tie_rows():
    rng = np.random.default_rng(77)
    rows = []
    for w in (2, 9, 64, 255):
        r = rng.integers(0, 50, size=w)
        first_last = r.copy()
        first_last[0] = first_last[-1] = 60  # a tie in the first and last positions
        last_two = r.copy()
        last_two[-2:] = 60
        inner = r.copy()
        inner[[w // 3, w // 2]] = 60
        rows += [first_last, last_two, inner, np.full(w, 7)]  # ... and every position tied
    rows.append(np.array([5]))
    return [r.astype(np.int32) for r in rows]


@pytest.mark.gpu
@pytest.mark.parametrize("temperature", [1.0, 0.125, 0.3])
def test_deterministic_mode_takes_the_first_maximum(temperature):
    """deterministic=True on rows with ties at the maximum (first and last positions, width 255): np.argmax's
    first maximum, for mz_select_actions and mz_select_actions_joint; no uniforms are read."""
    dev = torch.device("cuda", 0)
    rows = _tie_rows()
    draws = [(r, np.zeros(1), np.array([int(np.argmax([v for v in r]))])) for r in rows]
    assert draws[0][2][0] == 0 and draws[-2][2][0] == 0  # (the first of the tied maxima)
    for N in (1, 3):
        lay = Layout(draws, temperature, N=N)
        out = lay.output(dev)
        pos, act, ent = (_select if N == 1 else _select_joint)(out, None, temperature, True)
        for i, (r, _, _) in enumerate(lay.rows):
            assert pos[i] == int(select_action(r, temperature=temperature, deterministic=True)[0]) == lay.exp[i]
        got = act if N == 1 else act[:, 0]
        np.testing.assert_array_equal(got, lay.actions[np.arange(lay.B), lay.exp * N])
        np.testing.assert_allclose(ent, lay.ent, rtol=1e-12, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("temperature", [1.0, 0.125, 0.3])
@pytest.mark.parametrize("joint", [False, True])
def test_degenerate_rows_leave_their_neighbours_alone(temperature, joint):
    """Degree 0, degree > width, all counts zero, a count no path covers: -1 and a NaN entropy.  Degree 1 and
    a degree covering part of a row padded with large garbage counts: the row's own answer.  Every healthy
    neighbour in the batch keeps its result, bit for bit, of a batch without the degenerate rows."""
    dev = torch.device("cuda", 0)
    N = 3 if joint else 1
    run = _select_joint if joint else _select
    lay = Layout(class_draws((temperature, 300)), temperature, N=N, width=20, seed=5)
    W, B0 = lay.width, lay.B
    pos0, act0, ent0 = run(lay.output(dev), lay.u, temperature)
    np.testing.assert_array_equal(pos0, lay.exp)

    # every 9th root is replaced by a degenerate one, the kinds in turn
    at = np.arange(4, B0, 9)
    kind = np.arange(len(at)) % 6
    deg, visits = lay.deg.copy(), lay.visits.copy()
    exp_pos = lay.exp.copy()
    partial = np.array([4, 0, 9, 2, 1], np.int32)
    part_u, part_exp = boundary_draws(partial, temperature)
    u = lay.u.copy()
    for n, (i, k) in enumerate(zip(at, kind)):
        visits[i] = GARBAGE
        if k == 0:
            deg[i], exp_pos[i] = 0, -1
        elif k == 1:
            deg[i], exp_pos[i] = W + 1 + n % 3 * 1000, -1
        elif k == 2:
            deg[i], exp_pos[i] = 5, -1
            visits[i, :5] = 0
        elif k == 3:  # a count past the table (and, at 1/T = 1, a row the product covers whatever it holds)
            deg[i] = 3
            visits[i, :3] = [2, POW_TABLE_MAX + 1, 1]
            exp_pos[i] = -1 if temperature != 1.0 else int(
                reference_cdf(visits[i, :3], 1.0).searchsorted(u[i], side="right"))
        elif k == 4:
            deg[i], exp_pos[i] = 1, 0
            visits[i, 0] = 1 + n
        else:  # part of a row; the padding holds GARBAGE
            deg[i] = len(partial)
            visits[i, : len(partial)] = partial
            u[i], exp_pos[i] = part_u[n % len(part_u)], part_exp[n % len(part_u)]
    assert len(at) >= 12 and B0 % 64
    out = _output(B0, 4, dev, N, deg, visits, lay.actions)
    pos, act, ent = run(out, u, temperature)
    np.testing.assert_array_equal(pos, exp_pos)
    refused = exp_pos < 0
    assert refused[at].sum() >= len(at) // 2 - 2 and np.isnan(ent[refused]).all() and not np.isnan(ent[~refused]).any()
    act2 = act.reshape(B0, N)
    assert (act2[refused] == -1).all()
    ok = np.flatnonzero(~refused)
    chosen = lay.actions.reshape(B0, W, N)[ok, exp_pos[ok]]
    np.testing.assert_array_equal(act2[ok], chosen if joint else chosen[:, :1])
    healthy = np.setdiff1d(np.arange(B0), at)
    np.testing.assert_array_equal(pos[healthy], pos0[healthy])
    np.testing.assert_array_equal(act2[healthy], act0.reshape(B0, N)[healthy])
    np.testing.assert_array_equal(_bits(ent[healthy]), _bits(ent0[healthy]))


# -- mz_eps_greedy -------------------------------------------------------------------------------
def _eps_cases(A, eps):
    """(weights [A], greedy, u_eps, u_cat) per root: u_cat at every cumsum / total entry and its two
    neighbours under a draw that picks (u_eps just below float32(eps)); u_eps at float32(eps) and its two
    float32 neighbours, and at 0."""
    rng = np.random.default_rng(100 + A)
    rows = [rng.integers(0, 6, size=A) for _ in range(5)]           # weights above 1, and zeros
    rows += [np.ones(A, np.int64), rng.integers(0, 2, size=A) * 50000, np.zeros(A, np.int64)]
    rows[1][0] = 0
    rows[2][-1] = 0
    e32 = np.float32(eps)
    below, above = np.nextafter(e32, np.float32(0)), np.nextafter(e32, np.float32(1))
    cases = []
    for w in rows:
        w = w.astype(np.int64)
        tot = int(w.sum())
        us = [0.0, np.nextafter(1.0, 0.0)]
        if tot > 0:
            for c in np.cumsum(w)[:-1]:
                x = float(c) / float(tot)
                us += [v for v in (np.nextafter(x, 0.0), x, np.nextafter(x, 1.0)) if v < 1.0]
        cases += [(w, below, v) for v in us]
        cases += [(w, ue, us[len(us) // 2]) for ue in (below, e32, above, np.float32(0))]
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 2, 255])
def test_eps_greedy_at_boundary_draws(A):
    """mz_eps_greedy at A = 1, 2, 255 with legal weights above 1, a row stride above A (garbage between
    the rows), u_cat at every cumsum / total boundary and u_eps around float32(eps): the action of
    eps_greedy_given (oracle/consume.py: core/utils.py:319-334 with its two draws passed in)."""
    from mazero_amd.consume import eps_greedy

    dev = torch.device("cuda", 0)
    eps = 0.3
    cases = _eps_cases(A, eps)
    B = len(cases) + (len(cases) % 64 == 0)
    cases = cases + cases[:B - len(cases)]
    rng = np.random.default_rng(A)
    greedy = rng.integers(0, A, size=B).astype(np.int32)
    stride = A + 5
    legal = np.full((B, stride), GARBAGE, np.int32)
    for i, (w, _, _) in enumerate(cases):
        legal[i, :A] = w
    u_eps = np.array([c[1] for c in cases], np.float32)
    u_cat = np.array([c[2] for c in cases], np.float64)
    exp = [eps_greedy_given(greedy[i], cases[i][0], eps, u_eps[i], u_cat[i]) for i in range(B)]
    assert A == 1 or len(set(np.asarray(exp) != greedy)) == 2  # both branches are taken
    out = _output(B, A, dev)
    act = torch.from_numpy(greedy.copy()).to(dev)
    legal_d = torch.from_numpy(legal).to(dev)
    eps_greedy(out, act, legal_d[:, :A], eps, torch.from_numpy(u_eps).to(dev), torch.from_numpy(u_cat).to(dev))
    np.testing.assert_array_equal(act.cpu().numpy(), np.asarray(exp, np.int32))


# -- mz_marginal_policy --------------------------------------------------------------------------
def _marginal_rows(A):
    """(marginal [B, A], legal [B, A]) int32: counts near 2**31 / A (the row sums pass 2**31 and the
    products with the legal weights pass it too: only int64 sums and products are right), ties in the
    argmax of the products, legal weights above 1, rows without visits, rows with no visit on a legal action."""
    rng = np.random.default_rng(200 + A)
    big = (2 ** 31 - 1) // A
    B = 67
    lo = big if A > 1 else big - big // 8  # (A = 1: one count cannot pass 2**31, its product can)
    m = rng.integers(lo, lo + big // 8 + 1, size=(B, A)).astype(np.int64)
    legal = rng.integers(0, 4, size=(B, A)).astype(np.int64)
    m[10:20] = rng.integers(0, 40, size=(10, A))
    legal[40:50] = rng.integers(0, max(4, 2 * (2 ** 31 // big)), size=(10, A))  # products past 2**31 at every A
    m[20] = lo + 1                                # every count the same
    legal[20] = 3                                 # ... and every product ties
    if A > 1:
        m[21, [3, 200]], legal[21, [3, 200]] = [6, 4], [2, 3]   # equal products of different factors
        m[21, [0, A - 1]], legal[21, [0, A - 1]] = 0, 9
        m[22, [0, A - 1]], legal[22, [0, A - 1]] = big, 3       # a tie in the first and last positions
        legal[23] = (m[23] == m[23].max()) * 2                  # one legal action
        legal[24] = 0                                           # no legal action
        m[25, 1:] = 0
        legal[25, 0] = 0                                        # the only visits lie on an illegal action
    m[30:33] = 0                                  # roots without visits
    assert (A == 1 or (m.sum(axis=1) > 2 ** 31).any()) and ((m * legal).max(axis=1) > 2 ** 31).any()
    assert m.max() < 2 ** 31
    return m.astype(np.int32), legal.astype(np.int32)


def _check_marginal(mode, m, legal, action, prob0, act, prob, ent):
    """The results of one mz_marginal_policy call (prob started at prob0, ent at -5, act at `action` or 99)
    against the reference's lines, root by root."""
    B, A = m.shape
    for i in range(B):
        mi = m[i]
        masked = mi.astype(np.int64) * legal[i].astype(np.int64)
        if mode == "argmax_legal":  # reanalyze_worker.py:563-570
            assert act[i] == (np.argmax(masked) if np.sum(masked) > 0 else -1), i
            assert prob[i] == prob0[i] and ent[i] == -5.0
            continue
        if mode == "argmax":  # reanalyze_worker.py:303-319
            if np.sum(mi) == 0:
                assert act[i] == -1 and prob[i] == prob0[i] and ent[i] == -5.0
                continue
            assert act[i] == np.argmax(masked), i
        else:
            assert act[i] == action[i]
        a = act[i]
        if np.sum(mi) > 0:  # selfplay_worker.py:284-286
            d = mi / np.sum(mi)
            if 0 <= a < A:
                assert prob[i] == prob0[i] * d[a], i  # bit-exact float64
            else:
                assert np.isnan(prob[i]), i
            np.testing.assert_allclose(ent[i], -np.sum(d * np.log(d + 1e-9)), rtol=1e-12, atol=1e-15)
        else:  # :287-288
            assert prob[i] == prob0[i] * (1.0 / A) and ent[i] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 255])
@pytest.mark.parametrize("mode", ["given", "argmax", "argmax_legal"])
def test_marginal_policy_wide_and_large_counts(mode, A):
    """mz_marginal_policy in its three modes at A = 1 and 255 (selfplay_worker.py:278-290,
    reanalyze_worker.py:303-343 and :563-570 restated): first argmax of the int64 products, float64
    `marginal / sum` bit for bit, entropy to 1e-12; GIVEN with an action outside 0..A-1 gives a NaN
    probability."""
    from mazero_amd._capi import MZ_MARGINAL_ARGMAX, MZ_MARGINAL_ARGMAX_LEGAL, MZ_MARGINAL_GIVEN
    from mazero_amd.consume import marginal_policy

    dev = torch.device("cuda", 0)
    m, legal = _marginal_rows(A)
    B = m.shape[0]
    rng = np.random.default_rng(A)
    out = _output(B, A, dev, marginal=m.reshape(B, 1, A))
    prob0 = rng.random(B) + 0.5
    prob = torch.from_numpy(prob0.copy()).to(dev)
    ent = torch.full((B,), -5.0, dtype=torch.float64, device=dev)
    legal_d = torch.from_numpy(legal).to(dev)
    if mode == "given":
        action = rng.integers(0, A, size=B).astype(np.int32)
        action[[1, 2, 3, 31]] = [-1, A, A + 5, -3]  # outside the row
        act = torch.from_numpy(action.copy()).to(dev)
        marginal_policy(out, MZ_MARGINAL_GIVEN, act, prob, entropy=ent)
    elif mode == "argmax":
        act = torch.full((B,), 99, dtype=torch.int32, device=dev)
        marginal_policy(out, MZ_MARGINAL_ARGMAX, act, prob, legal=legal_d, entropy=ent)
    else:
        act = torch.full((B,), 99, dtype=torch.int32, device=dev)
        marginal_policy(out, MZ_MARGINAL_ARGMAX_LEGAL, act, None, legal=legal_d)
    _check_marginal(mode, m, legal, action if mode == "given" else None, prob0, act.cpu().numpy(),
                    prob.cpu().numpy(), ent.cpu().numpy())
