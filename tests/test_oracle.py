"""The oracle itself, pinned before it is trusted (CPU only).

* libstdc++ known answers (tests/golden/kat_libstdcxx.json, made by oracle/kat_libstdcxx.cpp):
  the restated std::mt19937 and std::discrete_distribution of oracle/ptree.py
* the golden traces (tests/golden/trace_*.npz, recorded from the compiled reference ctree by
  oracle/gen_golden.py) replayed through the pure-Python ptree and the C++ CPU port
* the reference oracle itself, when it is built here, reproduces the committed traces
"""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, assert_same, full_fixtures, golden_traces, load_full, load_trace

import ptree
from mazero_amd.cytree import Tree_batch
from mazero_amd.synthetic import make_search_inputs, run_search


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(GOLDEN, "kat_libstdcxx.json")) as f:
        return json.load(f)


def test_mt19937_known_answers(kat):
    for seed, words in kat["mt"]:
        g = ptree.MT19937(seed)
        assert [g() for _ in range(len(words))] == words, f"seed {seed}"
    g = ptree.MT19937(5489)
    for _ in range(9999):
        g()
    assert g() == kat["mt10000_5489"] == 4123659995  # C++ standard [rand.predef]/3


def test_discrete_distribution_known_answers(kat):
    for seed, weights, draws, consumed in kat["dd"]:
        w = np.asarray(weights, np.float32)
        g = ptree.MT19937(seed)
        d = ptree.Discrete(w)
        got = [d(g) for _ in range(len(draws))]
        assert got == draws, f"seed {seed} weights {weights}"
        assert consumed == (0 if len(w) < 2 else 2 * len(draws))


def test_pbc_table_known_answers(kat):
    """glibc logf as ucb_score evaluates it (cnode.cpp:313)."""
    libm = C.CDLL("libm.so.6")
    libm.logf.restype = C.c_float
    libm.logf.argtypes = [C.c_float]
    f32 = np.float32
    for c2, c1, n, bits in kat["pbc_logf_bits"]:
        x = f32(f32(f32(n) + f32(c2)) + f32(1.0))
        v = f32(f32(libm.logf(float(f32(x / f32(c2))))) + f32(c1))
        assert int(v.view(np.uint32)) == bits


@pytest.mark.parametrize("path", golden_traces(), ids=lambda p: os.path.basename(p)[6:-4])
def test_port_matches_golden(path, port_lib):
    inp, knobs, K, expected = load_trace(path)
    tb = Tree_batch(inp.B, 1, inp.A, K, inp.S, knobs["delta_lb"], inp.seed, knobs["rho"], knobs["lam"], lib=port_lib)
    assert_same(run_search(tb, inp, K, knobs), expected, "port ")


SMALL = [p for p in golden_traces() if not any(s in p for s in ("deep", "27m_k5"))]


@pytest.mark.parametrize("path", SMALL, ids=lambda p: os.path.basename(p)[6:-4])
def test_ptree_matches_golden(path):
    inp, knobs, K, expected = load_trace(path)
    tb = ptree.Tree_batch(inp.B, 1, inp.A, K, inp.S, knobs["delta_lb"], inp.seed, knobs["rho"], knobs["lam"])
    assert_same(run_search(tb, inp, K, knobs), expected, "ptree ")


@pytest.mark.parametrize("path", golden_traces()[:4], ids=lambda p: os.path.basename(p)[6:-4])
def test_reference_reproduces_golden(path, ref_lib):
    inp, knobs, K, expected = load_trace(path)
    tb = Tree_batch(inp.B, 1, inp.A, K, inp.S, knobs["delta_lb"], inp.seed, knobs["rho"], knobs["lam"], lib=ref_lib)
    assert_same(run_search(tb, inp, K, knobs), expected, "ref ")


@pytest.mark.parametrize("K,A,ties,lz", [(1, 9, False, 0.0), (5, 9, False, 0.3), (10, 15, True, 0.0)])
def test_port_matches_reference_fresh(ref_lib, port_lib, K, A, ties, lz):
    """Beyond the committed traces: fresh random searches, reference vs port, bit-exact."""
    rng = np.random.default_rng(K * 100 + A)
    inp = make_search_inputs(rng, 32, A, 50, legal_zero_frac=lz, ties=ties)
    outs = []
    for lib in (ref_lib, port_lib):
        tb = Tree_batch(inp.B, 1, A, K, inp.S, 0.01, inp.seed, 0.75, 0.8, lib=lib)
        outs.append(run_search(tb, inp, K))
    assert_same(outs[1], outs[0], "port vs ref ")


@pytest.mark.parametrize("chunk", range(int(os.environ.get("MZ_FUZZ_CHUNKS", "4"))))  # (as the GPU fuzz)
def test_port_matches_reference_fuzz(ref_lib, port_lib, chunk):
    """The GPU fuzz configurations (tests/fuzz_configs.py: A 1-64, K 1-70, S 1-60, B 1-48, every
    search knob, masks, ties, noise), the CPU port against the reference ctree, bit for bit: the
    GPU's comparison partner is pinned on the same cases."""
    from dataclasses import replace

    from fuzz_configs import fuzz_configs

    for B, A, K, S, knobs, lz, ties, eps, s in fuzz_configs(1234 + chunk, 10):
        rng = np.random.default_rng(s)
        inp = replace(make_search_inputs(rng, B, A, S, legal_zero_frac=lz, ties=ties), noise_eps=eps)
        outs = []
        for lib in (ref_lib, port_lib):
            tb = Tree_batch(inp.B, 1, A, K, inp.S, knobs["delta_lb"], inp.seed, knobs["rho"], knobs["lam"], lib=lib)
            outs.append(run_search(tb, inp, K, knobs))
        assert_same(outs[1], outs[0], f"port vs ref B={B} A={A} K={K} S={S} knobs={knobs}: ")

# ---- adversarial network outputs (tests/edge_inputs.py): the port pinned where the kernels are checked ----
EDGE_SHAPES = [(1, 9), (5, 9), (10, 100)]  # (K, A)


def _edge_base(K, A, B=3, S=40):
    return make_search_inputs(np.random.default_rng(5000 + 100 * K + A), B, A, S)


def _search(lib, inp, K, knobs=None):
    k = knobs or {}
    tb = Tree_batch(inp.B, 1, inp.A, K, inp.S, k.get("delta_lb", 0.01), inp.seed, k.get("rho", 0.75),
                    k.get("lam", 0.8), lib=lib)
    return run_search(tb, inp, K, knobs)


@pytest.mark.parametrize("K,A", EDGE_SHAPES)
def test_port_matches_reference_edges(ref_lib, port_lib, K, A):
    """Every input class of tests/edge_inputs.py, on every tree and on tree 1 alone: the reference
    ctree and the CPU port, bit for bit (the GPU edge tests compare the kernels with the port)."""
    from edge_inputs import EDGE_CLASSES

    base = _edge_base(K, A)
    for name, f in EDGE_CLASSES.items():
        for trees in (None, [1]):
            inp = f(base, trees)
            with np.errstate(all="ignore"):
                outs = [_search(lib, inp, K) for lib in (ref_lib, port_lib)]
            assert_same(outs[1], outs[0], f"port vs ref {name} trees={trees} K={K} A={A}: ")


@pytest.mark.parametrize("chunk", range(int(os.environ.get("MZ_FUZZ_CHUNKS", "4"))))
def test_port_matches_reference_edge_fuzz(ref_lib, port_lib, chunk):
    """The GPU edge fuzz configurations (tests/fuzz_configs.py::fuzz_edge_configs), the CPU port
    against the reference ctree, bit for bit."""
    from fuzz_configs import edge_inputs_of, fuzz_edge_configs

    for cfg in fuzz_edge_configs(4321 + chunk, 10):
        B, A, K, S, knobs, lz, ties, eps, s, classes, trees = cfg
        inp = edge_inputs_of(cfg)
        with np.errstate(all="ignore"):
            outs = [_search(lib, inp, K, knobs) for lib in (ref_lib, port_lib)]
        assert_same(outs[1], outs[0], f"port vs ref B={B} A={A} K={K} S={S} knobs={knobs} lz={lz} ties={ties} "
                                      f"eps={eps} classes={classes} trees={trees}: ")


_INPUT_ARRAYS = ("root_reward", "root_value", "root_policy", "root_beta", "root_noise", "reward", "value", "policy",
                 "beta")


def test_edge_classes_are_what_they_are_named(port_lib):
    """Each class of tests/edge_inputs.py has the property it is named for, and `trees=[1]` leaves
    trees 0 and 2 byte-identical to the unmodified inputs."""
    import edge_inputs as E

    base = _edge_base(1, 9)
    B, A, S = base.B, base.A, base.S
    assert np.array_equal(base.beta, base.policy)  # (what the benign generator gives)
    alt = {name: f(base) for name, f in E.EDGE_CLASSES.items()}
    for name, f in E.EDGE_CLASSES.items():
        one = f(base, [1])
        changed = False
        for k in _INPUT_ARRAYS:
            a, b, c = getattr(base, k), getattr(one, k), getattr(alt[name], k)
            ax = 0 if k.startswith("root_") else 1
            assert b.dtype == np.float32 and b.shape == a.shape, (name, k)
            for t in (0, 2):
                assert np.take(a, t, ax).tobytes() == np.take(b, t, ax).tobytes(), (name, k, t)
            changed |= np.take(a, 1, ax).tobytes() != np.take(b, 1, ax).tobytes()
            if name not in ("peaked", "root_peaked"):  # (those draw per call: the same kind, other rows)
                assert np.take(c, 1, ax).tobytes() == np.take(b, 1, ax).tobytes(), (name, k)
        assert changed, name
        assert (one.B, one.A, one.S, one.seed, one.noise_eps) == (B, A, S, base.seed, base.noise_eps)
    # beta differs from policy, both still distributions, policy untouched
    for name, tau in (("beta_tau2", 2.0), ("beta_tau05", 0.5)):
        x = alt[name]
        assert np.array_equal(x.policy, base.policy) and not np.array_equal(x.beta, x.policy)
        want = base.policy.astype(np.float64) ** (1 / tau)
        want /= want.sum(-1, keepdims=True)
        assert np.allclose(x.beta, want, rtol=1e-5, atol=0) and np.allclose(x.beta.sum(-1), 1, atol=1e-6)
        assert np.array_equal(np.argsort(x.beta, -1), np.argsort(x.policy, -1))
    x = alt["beta_rolled"]
    assert np.array_equal(x.policy, base.policy) and np.array_equal(x.beta[..., :-1], base.policy[..., 1:])
    assert np.array_equal(x.beta[..., -1], base.policy[..., 0])
    assert (np.argmax(x.beta, -1) != np.argmax(x.policy, -1)).all()
    flat, sharp = alt["beta_tau2"].beta.max(-1), alt["beta_tau05"].beta.max(-1)
    assert (flat < base.policy.max(-1)).all() and (sharp > base.policy.max(-1)).all()
    # exact zeros; subnormals
    z = alt["zero_entries"]
    assert np.array_equal(z.beta == 0, z.policy == 0) and (z.beta[..., 1] > 0).all() and (z.beta[..., -1] == 0).any()
    assert 0.3 < (z.beta == 0).mean() < 0.5
    for x, rows in ((alt["peaked"], "policy"), (alt["root_peaked"], "root_policy")):
        p = getattr(x, rows)
        assert np.array_equal(p, getattr(x, rows.replace("policy", "beta")))
        assert (p == 0).any() and np.allclose(p.sum(-1), 1, atol=1e-6) and (p.max(-1) > 0.5).mean() > 0.9
    p = alt["peaked"].policy
    assert 0.5 < (p == 0).mean() < 0.7 and 0.02 < E.is_subnormal(p).mean() < 0.12
    for name, j in (("concentrated_first", 0), ("concentrated_last", A - 1)):
        b = alt[name].beta
        assert (b[..., j] > 0.99999).all() and (np.delete(b, j, -1) < 1e-6).all() and (b > 0).all()
        assert (_search(port_lib, alt[name], 1)["sel_act"][1:] == j).all()  # (K = 1: it draws what it is named for)
    # wild: a prior above 1e30, a value or a reward outside +-1e30, where stated
    with np.errstate(all="ignore"):
        w = alt["wild_prior"]
        assert (w.policy[2:] / w.beta[2:] > 1e30).all() and np.array_equal(w.policy[:2], base.policy[:2])
        assert (w.beta[2:] > 0).all() and np.isfinite(w.policy[2:] / w.beta[2:]).any()
        assert (alt["wild_value"].value[2] > 1e30).all() and np.isfinite(alt["wild_value"].value).all()
        assert (np.delete(alt["wild_value"].value, 2, 0) == np.delete(base.value, 2, 0)).all()
        assert (alt["wild_reward"].reward[2] > 1e30).all() and np.isfinite(alt["wild_reward"].reward).all()
        assert np.isposinf(alt["inf_value"].value[2]).all() and np.isfinite(np.delete(alt["inf_value"].value, 2, 0)).all()
        assert (alt["root_wild_value"].root_value > 1e30).all()
        r = alt["root_wild_prior"]
        assert (r.root_policy / r.root_beta > 1e30).all() and (r.root_beta > 0).all()
        # (all but the non-root priors reach the root's read-backs: some q or prior past the tame range)
        for name in (n for n in E.WILD if n != "wild_prior"):
            out = _search(port_lib, alt[name], 1)
            far = [np.abs(out[k]).max() for k in ("sampled_qvalues", "sampled_priors", "root_values")]
            assert max(far) > 1e30 or np.isnan(far).any(), (name, far)
    for name in E.EDGE_CLASSES:
        assert not any(np.isnan(getattr(alt[name], k)).any() for k in _INPUT_ARRAYS), name  # (NaN: out of scope)
    # the normaliser: a spread under delta_lb all search long; magnitudes of the real heads; max == min
    delta_lb = 0.01
    for K in (1, 5):
        out = _search(port_lib, alt["small_spread"], K)
        for t in range(B):
            q = np.concatenate([out["sampled_qvalues"][t, : out["degree"][t]], out["root_values"][t : t + 1],
                                out["root_values_per_sim"][:, t]])
            assert q.max() - q.min() < delta_lb, (K, t, q.min(), q.max())
    lg = alt["large_scale"]
    assert np.abs(lg.value).max() > 300 and np.abs(lg.reward).max() > 20
    c = alt["constant_value"]
    assert (c.value == 0.5).all() and (c.reward == 0).all()


def test_ptree_joint_action_matches_reference(ref_lib):
    """agent_num = 2 joint-action trees (upstream MAZero semantics)."""
    rng = np.random.default_rng(7)
    B, N, A, K, S = 4, 2, 3, 5, 20
    pol = rng.dirichlet([1.0] * A, (B, N)).astype(np.float32)
    noise = rng.dirichlet([0.3] * A, (B, N)).astype(np.float32)
    r = np.zeros(B, np.float32)
    v = rng.standard_normal(B).astype(np.float32)
    trees = [Tree_batch(B, N, A, K, S, 0.01, 11, 0.75, 0.8, lib=ref_lib),
             ptree.Tree_batch(B, N, A, K, S, 0.01, 11, 0.75, 0.8)]
    res = [[], []]
    for k, tb in enumerate(trees):
        tb.prepare(r, v, pol, pol, K, 0.25, noise)
        for s in range(S):
            ix, _, act = tb.batch_selection(19652.0, 1.25, 0.997)
            res[k].append((list(ix), np.asarray(act).tolist()))
            p = rng.dirichlet([1.0] * A, (B, N)).astype(np.float32) if k == 0 else saved[s][0]
            if k == 0:
                saved.append((p,))
            tb.batch_expansion_and_backup(s + 1, 0.997, K, r, v, p, p)
        res[k].append(tb.get_roots_marginal_visit_count().tolist())
        res[k].append(tb.get_roots_values().tolist())
    assert res[0] == res[1]


saved = []


def test_port_joint_action_trees_match_reference(ref_lib, port_lib):
    """agent_num > 1 on the CPU port vs the reference ctree: the checker of the GPU joint-action
    kernels (tests/test_gpu_parity.py::test_joint_action_trees_vs_port), incl. int64 key wrap."""
    import test_gpu_parity as T

    for name, B, N, A, K, S in T.JOINT:
        rr, orf = T._joint_run(ref_lib, B, N, A, K, S, 3)
        rp, op = T._joint_run(port_lib, B, N, A, K, S, 3)
        for (ia, aa), (ib, ab) in zip(rr, rp):
            assert np.array_equal(ia, ib) and np.array_equal(aa, ab), name
        for k in ("values", "mv", "mp"):
            assert np.array_equal(orf[k].view(np.int32), op[k].view(np.int32)), (name, k)
        for k in ("q", "acts", "vc", "pr", "bh"):
            assert all(np.array_equal(g.view(np.int32), c.view(np.int32)) for g, c in zip(orf[k], op[k])), (name, k)


FULL = full_fixtures()


@pytest.mark.parametrize("path", FULL, ids=[os.path.basename(p)[5:-4] for p in FULL])
def test_port_matches_reference_at_baseline_sizes(port_lib, path):
    """The CPU port against the reference ctree's own outputs at the BASELINE sizes (3m 256 x 50,
    2s3z 1024 x 50, 3s5z 512 x 100, 27m 256 x 200; ties; 30 % masked actions), recorded by
    oracle/gen_golden.py --full; the regenerated inputs are checked against the recorded digest."""
    inp, K, expected = load_full(path)
    tb = Tree_batch(inp.B, 1, inp.A, K, inp.S, 0.01, inp.seed, 0.75, 0.8, lib=port_lib)
    assert_same(run_search(tb, inp, K, per_sim=False), expected, "port ")



def test_port_under_sanitizers():
    """the CPU restatement built with AddressSanitizer + UBSan (make -C oracle asan)
    replays every golden trace and three BASELINE-size fixtures bit-exactly with no report (the
    sanitizer runtime aborts the child process on the first error)."""
    import subprocess
    import sys

    root = os.path.dirname(GOLDEN.rstrip("/"))
    root = os.path.dirname(root)
    subprocess.run(["make", "-C", os.path.join(root, "oracle"), "asan"], check=True, stdout=subprocess.DEVNULL)
    asan = subprocess.check_output(["g++", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan):
        pytest.skip("libasan not available")
    env = dict(os.environ)
    env["LD_PRELOAD"] = ":".join(x for x in (asan, os.environ.get("LD_PRELOAD", "")) if x)
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    code = f"""
import ctypes as C, os, sys
sys.path[:0] = [{root!r}, {os.path.join(root, "tests")!r}, {os.path.join(root, "oracle")!r}]
from conftest import assert_same, full_fixtures, golden_traces, load_full, load_trace
from mazero_amd import _capi
from mazero_amd.cytree import Tree_batch
from mazero_amd.synthetic import run_search
lib = _capi.bind(C.CDLL(os.path.join({root!r}, "oracle", "_build", "libmzport_asan.so")))
n = 0
for p in golden_traces():
    inp, knobs, K, exp = load_trace(p)
    tb = Tree_batch(inp.B, 1, inp.A, K, inp.S, knobs["delta_lb"], inp.seed, knobs["rho"], knobs["lam"], lib=lib)
    assert_same(run_search(tb, inp, K, knobs), exp, os.path.basename(p)); n += 1
for p in [f for f in full_fixtures() if any(k in f for k in ("3m_k5_ties", "3m_k10", "27m_k1"))]:
    inp, K, exp = load_full(p)
    tb = Tree_batch(inp.B, 1, inp.A, K, inp.S, 0.01, inp.seed, 0.75, 0.8, lib=lib)
    assert_same(run_search(tb, inp, K, per_sim=False), exp, os.path.basename(p)); n += 1
print("sanitized replays", n)
"""
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert f"sanitized replays {len(golden_traces()) + 3}" in r.stdout
