"""Record the wide joint-tree fixtures tests/golden/joint_wide_<shape>.npz from the reference's own
ctree (oracle/_ref/libmzref.so, built by `make -C oracle` where the reference sources exist).

    python scripts/gen_joint_wide_golden.py [--check]

Each file holds the seed recipe (cfg = B, N, A, K, S; seeds = generator seed, tree seed; knobs), every
simulation's idx_x [S, B] and actions [S, B, N], and the readbacks: values, the [B, N, A] marginals, the
roots' degrees and the per-child fields concatenated in root order.  The inputs are regenerated from the
seeds by tests/test_joint_wide.py's `joint_run`, which is also what the tests run on the CPU port and on
the GPU.  --check compares the files on disk with a fresh recording instead of writing them."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libmzref.so")


def main() -> int:
    from mazero_amd import _capi
    from test_joint_wide import FIXTURE_SHAPES, fixture_path, joint_run, pack

    if not os.path.exists(REF_LIB):
        print(f"{REF_LIB} is not built (it needs the reference sources): nothing recorded", file=sys.stderr)
        return 1
    ref = _capi.bind(C.CDLL(REF_LIB))
    check = "--check" in sys.argv[1:]
    bad = 0
    for shape in FIXTURE_SHAPES:
        rec, out, _ = joint_run(ref, shape)
        z = pack(shape, rec, out)
        path = fixture_path(shape)
        if check:
            old = np.load(path)
            same = sorted(old.files) == sorted(z) and all(
                old[k].dtype == z[k].dtype and old[k].shape == z[k].shape and old[k].tobytes() == z[k].tobytes()
                for k in z)
            print(f"{os.path.basename(path)}: {'same' if same else 'DIFFERS'}")
            bad += not same
            continue
        np.savez_compressed(path, **z)
        print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, max root degree {int(z['deg'].max())}, "
              f"max action {int(z['actions'].max())}, max idx_x {int(z['idx_x'].max())}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
