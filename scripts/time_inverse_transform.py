"""Per-launch time of mz_inverse_transform (include/mzdriver.h) by device events over a replayed
graph of back-to-back launches, beside the torch chain it replaces in the search loop
(mazero_amd.nets.inverse_support_transform for both heads).  Prints one JSON line
(profiles/fused_transforms/per_launch.json)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mazero_amd  # noqa
import torch

from mazero_amd import _capi
from mazero_amd._lib import load
from mazero_amd.nets import inverse_support_transform

lib = load()
B, S, REP = 256, 11, 500
dev = torch.device("cuda", 0)
torch.manual_seed(0)
xv = (torch.randn(B, S, device=dev) * 3).half()
xr = (torch.randn(B, S, device=dev) * 3).half()
ov = torch.empty(B, device=dev)
orr = torch.empty(B, device=dev)
p = lambda t: C.c_void_p(t.data_ptr())


def fused():
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.mz_inverse_transform(None, st, _capi.MZ_INV_LOGITS, B, p(xv), _capi.MZ_DT_F16, S, -5, 5,
                                  p(xr), _capi.MZ_DT_F16, S, -5, 5, p(ov), p(orr))
    assert rc == 0, lib.mz_last_error()


def chain():
    with torch.autocast("cuda"):
        inverse_support_transform(xr, -5, 5)
        inverse_support_transform(xv, -5, 5)


def graph_time(fn, rep):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(rep):
                fn()
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / rep)
    times.sort()
    return {"us_per_call_median": round(times[len(times) // 2], 3), "min": round(times[0], 3), "max": round(times[-1], 3)}


with torch.no_grad():
    out = {"shape": f"B={B}, S={S}, both heads, f16 logits, {REP} calls per replayed graph, 20 replays",
           "mz_inverse_transform": graph_time(fused, REP),
           "torch_chain_both_heads": graph_time(chain, 100)}
print(json.dumps(out), flush=True)
