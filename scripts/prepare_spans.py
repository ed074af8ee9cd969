"""Where a prepare launch's time goes, per wave role: the scripts/time_prepare.py loop on a spans
build (scripts/build_variant.sh spans -DMZ_SPANS=1, loaded with MZ_LIB_OVERRIDE), read from slot 0
of the launch spans (mz_debug_spans), which k_prepare and k_prepare1 record in such builds only.

    MZ_LIB_OVERRIDE=mazero_amd/_build/variant_spans.so python scripts/prepare_spans.py [B A K S]
    MZ_PREPARE_GENERAL=1 ... the same handle on the general k_prepare

Prints, as means over the workgroups of the last launch and in ns after each workgroup's own start
(100 MHz clock: 10 ns steps): the seeding barrier left, the last twist round's end, the root wave's
end; the launch's body (earliest start to latest end) and the HIP-event period of back-to-back
launches beside it."""
import ctypes as C
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
from mazero_amd._lib import load  # noqa: E402
from mazero_amd.cytree import Tree_batch  # noqa: E402
from mazero_amd.synthetic import DEFAULTS, make_search_inputs  # noqa: E402


def main():
    B, A, K, S = (int(x) for x in (sys.argv[1:5] if len(sys.argv) > 4 else (256, 9, 1, 50)))
    lib = load()
    spans = getattr(lib, "mz_debug_spans", None)
    if spans is None:
        raise SystemExit("not a spans build: build with -DMZ_SPANS=1 and set MZ_LIB_OVERRIDE")
    spans.argtypes, spans.restype = [C.c_void_p, C.c_int, C.c_int, C.c_int], C.c_int
    inp = make_search_inputs(np.random.default_rng(0), B, A, S)
    d = DEFAULTS
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rr, rv, rp, rb, rn = (t(x) for x in (inp.root_reward, inp.root_value, inp.root_policy, inp.root_beta, inp.root_noise))
    tb = Tree_batch(B, 1, A, K, S, d["delta_lb"], inp.seed, d["rho"], d["lam"])
    out = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
           torch.empty(B, 1, dtype=torch.int32, device=dev))
    c2, c1, g = d["pb_c_base"], d["pb_c_init"], d["discount"]
    for _ in range(20):
        tb.prepare_selection_device(rr, rv, rp, rb, K, inp.noise_eps, rn, c2, c1, g, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(50):
            tb.prepare_selection_device(rr, rv, rp, rb, K, inp.noise_eps, rn, c2, c1, g, out=out)
    trees = min(B, 1024)
    buf = (C.c_ulonglong * (4 * trees))()
    rows, period = [], []
    for _ in range(5):
        torch.cuda.synchronize()
        spans(None, 0, 0, 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        period.append(e0.elapsed_time(e1) * 1e3 / 50)
        spans(C.cast(buf, C.c_void_p), 1, trees, 0)  # slot 0: the replay's last launch
        raw = np.array(buf[:], dtype=np.float64).reshape(trees, 4) * 10.0  # ns: start, root end, seeded, twisted
        start = raw[:, 0]
        rel = raw[:, 1:] - start[:, None]
        rows.append([rel[:, 1].mean(), rel[:, 2].mean(), rel[:, 0].mean(), raw[:, 1:].max() - start.min()])
    seeded, twisted, root, body = np.median(np.array(rows), axis=0)
    print(f"prepare spans {tb.prepare_kernel()} B={B} A={A} K={K} S={S}: seeding barrier left {seeded:.0f} ns, "
          f"last twist round ends {twisted:.0f} ns, root wave ends {root:.0f} ns after the workgroup's start; "
          f"body {body:.0f} ns; period {np.median(period):.2f} us per launch")


if __name__ == "__main__":
    main()
