#!/usr/bin/env python
"""Measure sampling on the device (DESIGN.md "Sampling the final tensor")
against what it replaces: eng.result() to the host, then numpy cumsum and
searchsorted.

The tensor is the final tensor of an engine: the outer product of two random
leaves, n = 2^30 elements for c128 and 2^31 for c64 (16 GB each). Shots: 10^3
and 10^6.

Device side, by device events around tn_sample_*_dev on the engine's result
pointer (uniforms, indices and workspace already on the device): the call
with no shots (k_prob_chunk_sums + k_prob_scan) and the whole call; the draw
is the difference. ContractionEngine.sample_flat is timed by the host clock
(upload of u, the three launches, download of idx, synchronous). Baseline,
host clock: result() and |.|^2 and cumsum once per repetition, then
searchsorted per shot count. All of it interleaved in one loop after WARMUP
untimed rounds; the table gives the median and [min, max] in ms.

The split of the first two kernels comes from a kernel trace, a run of its
own with the profiler on:

  python scripts/sample_device.py --out profiles/sample_device.md
  rocprofv3 --kernel-trace --stats --output-format csv -d trace -- \\
      python scripts/sample_device.py --kernels
  python scripts/sample_device.py --trace trace >> profiles/sample_device.md

Needs an MI355X (except --trace, which only reads the trace).
"""

import argparse
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPS, BASE_REPS = 2, 10, 2
SIZES = {"c128": 30, "c64": 31}
SHOTS = (10 ** 3, 10 ** 6)
HBM_ACHIEVABLE = 6.3e12  # bytes/s, the achievable figure for this part
ESIZE = {"c128": 16, "c64": 8}


def spread(ms):
    return (f"{statistics.median(ms):.3f} [{min(ms):.3f}, {max(ms):.3f}]"
            if ms else "not measured")


def outer_product_engine(dtype, log2n):
    """An engine whose final tensor has 2^log2n elements: two random leaves
    with no leg in common."""
    from tnc_amd.contraction_path import ContractionPath
    from tnc_amd.executor import ContractionEngine
    from tnc_amd.tensor import CompositeTensor, LeafTensor, TensorData

    rng = np.random.default_rng(log2n)
    ra = log2n // 2
    leaves = []
    for legs in (list(range(ra)), list(range(ra, log2n))):
        dims = [2] * len(legs)
        leaf = LeafTensor(legs, dims)
        leaf.set_tensor_data(TensorData(
            TensorData.MATRIX,
            matrix=rng.standard_normal(dims) + 1j * rng.standard_normal(dims)))
        leaves.append(leaf)
    eng = ContractionEngine(CompositeTensor(leaves),
                            ContractionPath.simple([(0, 1)]), dtype=dtype)
    eng.contract()
    return eng


class DeviceCall:
    """tn_sample_<dtype>_dev on the engine's final tensor, everything else in
    torch-held device memory, timed by device events."""

    def __init__(self, torch, eng, dtype, n, u):
        from tnc_amd import hiplib as H

        self.torch, self.n, self.H = torch, n, H
        self.data = eng.result_dev()
        self.fn = getattr(H.lib(), "tn_sample_%s_dev" % dtype)
        self.u = torch.from_numpy(u).to("cuda:0")
        self.idx = torch.zeros(u.size, dtype=torch.int64, device="cuda:0")
        self.norm2 = torch.zeros(1, dtype=torch.float64, device="cuda:0")
        self.ws_bytes = H.plan_sample(n, u.size, dtype).ws_bytes
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8,
                              device="cuda:0")

    def run(self, nshots):
        torch = self.torch
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        self.H.check(self.fn(
            self.data, self.n, self.u.data_ptr(), nshots, self.idx.data_ptr(),
            self.norm2.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
            torch.cuda.current_stream().cuda_stream), "tn_sample_dev")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)


def baseline(eng, us):
    """(fetch + cumsum ms, {nshots: searchsorted ms}, {nshots: idx})."""
    t0 = time.perf_counter()
    _, data = eng.result()
    flat = data.reshape(-1)
    p = np.square(flat.real, dtype=np.float64)
    p += np.square(flat.imag, dtype=np.float64)
    del data, flat
    np.cumsum(p, out=p)
    t1 = time.perf_counter()
    search, idx = {}, {}
    for u in us:
        t2 = time.perf_counter()
        idx[u.size] = np.searchsorted(p, u * p[-1], side="right")
        search[u.size] = (time.perf_counter() - t2) * 1e3
    return (t1 - t0) * 1e3, search, idx


def measure(dtype, kernels_only, lines):
    import torch

    log2n = SIZES[dtype]
    n = 1 << log2n
    eng = outer_product_engine(dtype, log2n)
    # the device call draws its first nshots uniforms: one array, prefixes
    big = np.random.default_rng(7).random(max(SHOTS))
    us = [big[:s] for s in SHOTS]
    try:
        call = DeviceCall(torch, eng, dtype, n, us[-1])
        if kernels_only:
            for _ in range(3):
                for u in us:
                    call.run(u.size)
            return
        t = {"norm": [], "fetch": []}
        for s in SHOTS:
            t["full", s], t["host", s], t["search", s] = [], [], []
        agree = {}
        for r in range(WARMUP + REPS):
            print(f"{dtype} round {r}", file=sys.stderr, flush=True)
            keep = r >= WARMUP
            ms = call.run(0)
            if keep:
                t["norm"].append(ms)
            for u in us:
                ms = call.run(u.size)
                dev_idx = call.idx[:u.size].cpu().numpy()
                t0 = time.perf_counter()
                host_idx = eng.sample_flat(u)
                host_ms = (time.perf_counter() - t0) * 1e3
                assert np.array_equal(host_idx.astype(np.int64), dev_idx)
                if keep:
                    t["full", u.size].append(ms)
                    t["host", u.size].append(host_ms)
            if r < 1 + BASE_REPS:  # one untimed, then BASE_REPS timed
                try:
                    fetch, search, idx = baseline(eng, us)
                except MemoryError:
                    continue
                for u in us:
                    agree[u.size] = int(np.sum(
                        idx[u.size] == eng.sample_flat(u).astype(np.int64)))
                if r >= 1:
                    t["fetch"].append(fetch)
                    for s in SHOTS:
                        t["search", s].append(search[s])
    finally:
        eng.close()
    gb = n * ESIZE[dtype] / 1e9
    norm = statistics.median(t["norm"])
    lines.append(f"\n### {dtype}, n = 2^{log2n} ({gb:.1f} GB)\n")
    lines.append(f"- chunk sums + scan (no shots), device events: "
                 f"{spread(t['norm'])} ms; {gb / (norm * 1e-3):.0f} GB/s "
                 "over both kernels = "
                 f"{gb * 1e9 / (norm * 1e-3) / HBM_ACHIEVABLE:.0%} "
                 "of the 6.3 TB/s achievable HBM figure")
    lines.append(f"- baseline result() + |.|^2 + cumsum, host clock: "
                 f"{spread(t['fetch'])} ms")
    lines.append("")
    lines.append("| shots | whole device call | draw (call - no shots) | "
                 "sample_flat, host clock | baseline searchsorted | "
                 "baseline total | same index as baseline |")
    lines.append("|---|---|---|---|---|---|---|")
    for s in SHOTS:
        full = t["full", s]
        draw = statistics.median(full) - norm
        base = ([a + b for a, b in zip(t["fetch"], t["search", s])])
        lines.append(
            f"| {s} | {spread(full)} | {draw:.3f} | {spread(t['host', s])} | "
            f"{spread(t['search', s])} | {spread(base)} | "
            f"{agree.get(s, 'not measured')} of {s} |")


def from_trace(directory):
    """Per-kernel times of the three sampling kernels out of rocprofv3's
    kernel stats."""
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"),
                          recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                if not any(k in name for k in ("k_prob_chunk_sums",
                                               "k_prob_scan",
                                               "k_sample_draw")):
                    continue
                dtype = ("c128" if "double, 2" in name
                         else "c64" if "float, 2" in name else "both")
                rows[name.split("(")[0].replace("void ", ""), dtype] = row
    if not rows:
        raise SystemExit(f"no kernel stats under {directory}")
    lines = ["\n### Per kernel (rocprofv3 --kernel-trace --stats, a run of "
             "its own)\n",
             "k_sample_draw rows mix the 10^3- and 10^6-shot launches: "
             "MinNs is the former, MaxNs the latter. k_prob_scan runs on "
             "2^18 entries for c128 and 2^19 for c64.\n",
             "| kernel | dtype | calls | avg ms | min ms | max ms | "
             "pass-1 rate |", "|---|---|---|---|---|---|---|"]
    for (name, dtype), row in sorted(rows.items()):
        avg = float(row["AverageNs"]) * 1e-6
        rate = ""
        if "chunk_sums" in name and dtype in SIZES:
            bytes_ = (1 << SIZES[dtype]) * ESIZE[dtype]
            bps = bytes_ / (avg * 1e-3)
            rate = (f"{bps / 1e9:.0f} GB/s = {bps / HBM_ACHIEVABLE:.0%} of "
                    "6.3 TB/s")
        lines.append(f"| {name} | {dtype} | {row['Calls']} | {avg:.3f} | "
                     f"{float(row['MinNs']) * 1e-6:.3f} | "
                     f"{float(row['MaxNs']) * 1e-6:.3f} | {rate} |")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="write the tables here as well")
    ap.add_argument("--kernels", action="store_true",
                    help="device calls only, a few: for a kernel trace")
    ap.add_argument("--trace", help="directory of a kernel trace to tabulate")
    ap.add_argument("--dtypes", default="c128,c64")
    args = ap.parse_args()
    if args.trace:
        print("\n".join(from_trace(args.trace)))
        return
    lines = ["## Measured: device sampling against result() + numpy",
             "",
             f"{WARMUP} untimed rounds, then {REPS} timed (baseline: 1 "
             f"untimed, {BASE_REPS} timed), interleaved in one process; "
             "median [min, max] in ms."]
    for dtype in args.dtypes.split(","):
        measure(dtype, args.kernels, lines)
        if args.out and not args.kernels:  # what is measured so far
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    if not args.kernels:
        print("\n".join(lines))


if __name__ == "__main__":
    main()
