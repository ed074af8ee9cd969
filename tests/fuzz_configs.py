"""Seeded random small search configurations shared by the fuzz parity tests: the GPU against
the CPU port (tests/test_gpu_parity.py) and the port against the reference ctree
(tests/test_oracle.py), so the two comparisons cover the same cases."""
from __future__ import annotations

import numpy as np


def fuzz_configs(seed: int, n: int):
    """Seeded random small configurations across the kernels' classes and the search knobs (A up to
    255: past 64 actions the wide expansion and k_hbm)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        A = int(rng.choice([1, 2, 3, 5, 9, 11, 15, 16, 17, 36, 63, 64, 65, 130, 255]))
        K = int(rng.choice([1, 1, 2, 3, 5, 8, 10, 33, 64, 70]))
        S = int(rng.integers(1, 61))
        B = int(rng.integers(1, 49))
        knobs = dict(discount=float(rng.choice([0.997, 0.9, 1.0])), rho=float(rng.choice([0.75, 0.5, 0.0])),
                     lam=float(rng.choice([0.8, 1.0, 0.5])), delta_lb=float(rng.choice([0.01, 0.1])),
                     pb_c_init=float(rng.choice([1.25, 2.5])), pb_c_base=float(rng.choice([19652.0, 500.0])))
        lz = float(rng.choice([0.0, 0.3])) if A >= 2 else 0.0
        ties = bool(rng.random() < 0.15)
        eps = float(rng.choice([0.0, 0.25]))
        out.append((B, A, K, S, knobs, lz, ties, eps, int(rng.integers(1 << 30))))
    return out


def fuzz_configs_large(seed: int, n: int):
    """Seeded random configurations at SMAC-like sizes (S 60-300, B 64-512): the larger layout
    classes of the chain and tree kernels and the general kernel."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        A = int(rng.choice([5, 9, 11, 14, 17, 36, 64, 100]))
        K = int(rng.choice([1, 1, 2, 3, 5, 8, 10, 16]))
        S = int(rng.integers(60, 301))
        B = int(rng.integers(64, 513))
        knobs = dict(discount=float(rng.choice([0.997, 0.99])), rho=float(rng.choice([0.75, 0.5])),
                     lam=float(rng.choice([0.8, 1.0])), delta_lb=0.01, pb_c_init=1.25, pb_c_base=19652.0)
        lz = float(rng.choice([0.0, 0.3]))
        eps = float(rng.choice([0.0, 0.25]))
        out.append((B, A, K, S, knobs, lz, False, eps, int(rng.integers(1 << 30))))
    return out


def fuzz_edge_configs(seed: int, n: int):
    """Seeded random small configurations with adversarial network outputs (tests/edge_inputs.py):
    the knob choices of `fuzz_configs`, one or two input classes applied in the order drawn, to every
    tree or to a random subset of the trees.  A stream of its own: `fuzz_configs` draws as before."""
    from edge_inputs import EDGE_CLASSES

    rng = np.random.default_rng(seed)
    names = sorted(EDGE_CLASSES)
    out = []
    for _ in range(n):
        B = int(rng.integers(1, 9))
        A = int(rng.choice([2, 9, 17, 64, 100]))
        K = int(rng.choice([1, 2, 5, 10, 33, 70]))
        S = int(rng.integers(4, 61))
        knobs = dict(discount=float(rng.choice([0.997, 0.9, 1.0])), rho=float(rng.choice([0.75, 0.5, 0.0])),
                     lam=float(rng.choice([0.8, 1.0, 0.5])), delta_lb=float(rng.choice([0.01, 0.1])),
                     pb_c_init=float(rng.choice([1.25, 2.5])), pb_c_base=float(rng.choice([19652.0, 500.0])))
        lz = float(rng.choice([0.0, 0.3]))
        ties = bool(rng.random() < 0.15)
        eps = float(rng.choice([0.0, 0.25]))
        classes = [str(c) for c in rng.choice(names, size=int(rng.integers(1, 3)), replace=False)]
        trees = None
        if rng.random() < 0.5:
            trees = sorted(int(t) for t in rng.choice(B, size=int(rng.integers(1, B + 1)), replace=False))
        out.append((B, A, K, S, knobs, lz, ties, eps, int(rng.integers(1 << 30)), classes, trees))
    return out


def edge_inputs_of(cfg):
    """The search inputs of one `fuzz_edge_configs` entry."""
    from dataclasses import replace

    from edge_inputs import apply
    from mazero_amd.synthetic import make_search_inputs

    B, A, K, S, knobs, lz, ties, eps, s, classes, trees = cfg
    inp = replace(make_search_inputs(np.random.default_rng(s), B, A, S, legal_zero_frac=lz, ties=ties), noise_eps=eps)
    return apply(inp, classes, trees)
