"""Sliced contraction: one engine against one engine per slice.

Arm (a) is the host-driven method (bench.py's distributed path on one rank):
one ContractionEngine per slice_network(tn, assignment), each contracted in
turn, the results copied device-to-device into a torch tensor and added.
Arm (b) is one engine with slice_edges and contract_sliced(): leaves
uploaded once, one arena, the sum taken by the executor.

The arms are interleaved (a b a b ...) after warm-up so drift hits both, and
each repetition is a host wall time around a full contraction with a device
synchronisation at its end. Prints one JSON line.

    python scripts/sliced_single_engine.py --fixture rqc36 --edges 1
    python scripts/sliced_single_engine.py --fixture rqc24 --edges 2
"""

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pool_bytes(eng):
    from tnc_amd import hiplib

    used, cached = ctypes.c_uint64(), ctypes.c_uint64()
    hiplib.check(hiplib.lib().tn_net_pool_bytes(
        eng.net, ctypes.byref(used), ctypes.byref(cached)), "pool_bytes")
    return used.value, cached.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default="rqc36")
    ap.add_argument("--edges", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import numpy as np
    import torch

    from tnc_amd import hiplib
    from tnc_amd.contraction_path import ContractionPath
    from tnc_amd.executor import ContractionEngine
    from tnc_amd.fixtures import load_fixture
    from tnc_amd.slicing import (find_slice_edges, iter_assignments,
                                 slice_network)

    torch.cuda.set_device(0)
    tn, frozen, meta = load_fixture(args.fixture)
    dtype = meta.get("dtype", "c128")
    replace = ContractionPath.simple(frozen)
    edges, _ = find_slice_edges(tn, frozen, 0, max_edges=args.edges)
    assignments = list(iter_assignments(tn, edges))
    L = hiplib.lib()
    esize = 16 if dtype == "c128" else 8
    view = torch.float64 if dtype == "c128" else torch.float32

    torch.cuda.synchronize()
    free0, total = torch.cuda.mem_get_info()
    engines = [ContractionEngine(slice_network(tn, a), replace, dtype=dtype)
               for a in assignments]
    free_a, _ = torch.cuda.mem_get_info()
    one = ContractionEngine(tn, replace, dtype=dtype, slice_edges=edges)
    free_b, _ = torch.cuda.mem_get_info()

    elems = 1
    for d in (engines[0].infos[-1].out_dims if engines[0].infos else []):
        elems *= int(d)
    local = torch.zeros((elems, 2), dtype=view, device="cuda:0")
    tmp = torch.empty((elems, 2), dtype=view, device="cuda:0")

    peak_a = [0] * len(engines)
    peak_b = 0

    def arm_a():
        local.zero_()
        for x, eng in enumerate(engines):
            eng.contract()
            hiplib.check(L.tn_memcpy_dtod(tmp.data_ptr(), eng.result_dev(),
                                          elems * esize), "tn_memcpy_dtod")
            local.add_(tmp)
            peak_a[x] = max(peak_a[x], pool_bytes(eng)[0])
        torch.cuda.synchronize()

    dev_ms_b = []

    def arm_b():
        nonlocal peak_b
        dev_ms_b.append(one.contract_sliced())
        peak_b = max(peak_b, pool_bytes(one)[0])

    ta, tb = [], []
    for it in range(args.warmup + args.reps):
        for arm, sink in ((arm_a, ta), (arm_b, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arm()
            dt = (time.perf_counter() - t0) * 1e3
            if it >= args.warmup:
                sink.append(dt)
    dev_ms_b = dev_ms_b[args.warmup:]

    npc = np.complex128 if dtype == "c128" else np.complex64
    got_a = local.cpu().numpy().view(npc).reshape(-1)
    got_b = one.result()[1].reshape(-1)
    out = {
        "fixture": args.fixture, "dtype": dtype, "edges": edges,
        "assignments": len(assignments), "steps": len(one.steps),
        "reps": args.reps,
        "a_ms": ta, "b_ms": tb, "b_device_ms": dev_ms_b,
        "a_median_ms": statistics.median(ta),
        "b_median_ms": statistics.median(tb),
        "a_spread_ms": max(ta) - min(ta),
        "b_spread_ms": max(tb) - min(tb),
        "b_device_ms_per_assignment":
            statistics.median(dev_ms_b) / len(assignments),
        "a_pool_in_use_peak": sum(peak_a),
        "a_pool_reserved": sum(pool_bytes(e)[1] for e in engines),
        "b_pool_in_use_peak": peak_b,
        "b_pool_reserved": pool_bytes(one)[1],
        "mem_free_before": free0, "mem_total": total,
        "a_setup_bytes": free0 - free_a,
        "b_setup_bytes": free_a - free_b,
        "same_bits": bool(np.array_equal(got_a, got_b)),
    }
    print(json.dumps(out))
    for e in engines:
        e.close()
    one.close()


if __name__ == "__main__":
    main()
