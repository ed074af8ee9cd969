"""Per-launch time of mz_inverse_transform_wide (include/mzdriver.h) at the reference's default
support [-300, 300] (601 elements), by device events over a replayed graph of back-to-back calls,
beside the two routes it replaces in the search loop: torch's softmax, multiply and sum for both
heads in front of mz_inverse_transform at stage EXPECTATION (what `fused_transforms` alone records
for such supports), and the full torch chain (mazero_amd.nets.inverse_support_transform for both
heads).  Prints one JSON line (profiles/wide_supports/per_launch.json)."""
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
B, LO, HI, REP = 256, -300, 300, 200
S = HI - LO + 1
dev = torch.device("cuda", 0)
torch.manual_seed(0)
xv = (torch.randn(B, S, device=dev) * 3).half()
xr = (torch.randn(B, S, device=dev) * 3).half()
ov = torch.empty(B, device=dev)
orr = torch.empty(B, device=dev)
sup = torch.arange(LO, HI + 1, dtype=torch.float32, device=dev)
p = lambda t: C.c_void_p(t.data_ptr())


def wide():
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.mz_inverse_transform_wide(None, st, _capi.MZ_INV_LOGITS, B, p(xv), _capi.MZ_DT_F16, S, LO, HI,
                                       p(xr), _capi.MZ_DT_F16, S, LO, HI, p(ov), p(orr))
    assert rc == 0, lib.mz_last_error()


def expectation():  # mcts_sampled._SearchLoop._inverse_transform's route for supports past 64 elements
    with torch.autocast("cuda"):
        ev, er = [torch.sum(sup * torch.softmax(t, dim=-1), dim=-1, keepdim=True) for t in (xv, xr)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.mz_inverse_transform(None, st, _capi.MZ_INV_EXPECTATION, B, p(ev), _capi.MZ_DT_F32, 1, LO, HI,
                                  p(er), _capi.MZ_DT_F32, 1, LO, HI, p(ov), p(orr))
    assert rc == 0, lib.mz_last_error()


def chain():
    with torch.autocast("cuda"):
        inverse_support_transform(xr, LO, HI)
        inverse_support_transform(xv, LO, HI)


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
    wide()
    a = (ov.clone(), orr.clone())
    expectation()
    torch.cuda.synchronize()
    same = bool(torch.equal(a[0].view(torch.int32), ov.view(torch.int32)) and
                torch.equal(a[1].view(torch.int32), orr.view(torch.int32)))
    out = {"shape": f"B={B}, S={S}, both heads, f16 logits, 20 replays of a recorded graph of back-to-back calls",
           "mz_inverse_transform_wide_logits": graph_time(wide, REP),
           "torch_softmax_mul_sum_then_expectation": graph_time(expectation, 100),
           "torch_chain_both_heads": graph_time(chain, 100),
           "wide_equals_expectation_route_bits": same}
print(json.dumps(out), flush=True)
