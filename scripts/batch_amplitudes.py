#!/usr/bin/env python
"""Measure what batch labels buy (DESIGN.md "Batch labels").

Part 1: B amplitudes of one Sycamore-style circuit. One batched walk
(Circuit.into_amplitudes_network + contract_batched) against the mechanism
without batch labels: B ordinary engines, one per bitstring, each contract()
replayed as a hipGraph. Both the walk time and the end-to-end time (engine
construction, upload and the first contraction included) are reported, per
amplitude.

Part 2: the batched MFMA kernel (TN_BATCH_GEMM class) against the element
step looped over the batch (TN_BATCH_LOOP). The switch TN_BATCH_GEMM is read
once per process, so each side runs in child processes, alternated
(GEMM, LOOP, GEMM, LOOP); a one-step batched walk on a reserved arena is
timed, so neither side pays an allocation.

Protocol: every timed call ends in a device synchronise; WARMUP untimed
calls, then REPS timed ones; the table gives the median and [min, max] of
the host clock around the call (ms). Needs an MI355X.

  python scripts/batch_amplitudes.py --out profiles/batch_amplitudes.md
"""

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPS = 3, 20
QUBITS, DEPTH, SEED = 16, 8, 11
SHAPES = [(mn, k, b) for mn in (16, 64, 256) for k in (128, 1024)
          for b in (8, 64)]


def timed(fn, warmup=WARMUP, reps=REPS):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def spread(ms, per=1):
    ms = [x / per for x in ms]
    return (f"{statistics.median(ms):.4f} "
            f"[{min(ms):.4f}, {max(ms):.4f}]")


# ---- part 1 ----------------------------------------------------------------

def part1():
    from tnc_amd import Greedy
    from tnc_amd.builders import sycamore_circuit
    from tnc_amd.executor import ContractionEngine

    rng = np.random.default_rng(SEED)
    rows = []
    single, _ = sycamore_circuit(QUBITS, DEPTH, SEED).into_amplitude_network(
        "0" * QUBITS)
    replace = Greedy().find_path(single).replace_path()
    for nb in (1, 8, 64):
        strings = ["".join(rng.choice(["0", "1"], QUBITS)) for _ in range(nb)]
        # one batched walk
        t0 = time.perf_counter()
        tn, _, beta = sycamore_circuit(
            QUBITS, DEPTH, SEED).into_amplitudes_network(strings)
        # B == 1: no bra varies, no leaf carries beta, nothing is batched
        carried = any(beta in t.legs for t in tn.tensors)
        eng = ContractionEngine(tn, replace,
                                batch_edges=[beta] if carried else [])
        eng.contract_batched()
        legs, got = eng.result()
        e2e_batched = (time.perf_counter() - t0) * 1e3
        got = np.array(got, copy=True).reshape(-1)
        if not legs:  # B == 1 or all strings equal: no varying bra
            got = np.repeat(got, nb)
        walk_batched = timed(eng.contract_batched)
        classes = list(eng.batch_classes)
        eng.close()
        # the same amplitudes without batch labels: one engine per string
        t0 = time.perf_counter()
        engines, ref = [], []
        for s in strings:
            net, _ = sycamore_circuit(
                QUBITS, DEPTH, SEED).into_amplitude_network(s)
            e = ContractionEngine(net, replace)
            e.contract()
            ref.append(complex(e.result()[1]))
            engines.append(e)
        e2e_single = (time.perf_counter() - t0) * 1e3

        def replay_all():
            for e in engines:
                e.contract()

        walk_single = timed(replay_all)
        for e in engines:
            e.close()
        err = float(np.max(np.abs(got - np.array(ref))))
        rows.append(dict(B=nb, steps=len(classes),
                         classes=[classes.count(c) for c in range(4)],
                         walk_batched=spread(walk_batched, nb),
                         walk_single=spread(walk_single, nb),
                         e2e_batched=f"{e2e_batched / nb:.3f}",
                         e2e_single=f"{e2e_single / nb:.3f}",
                         max_abs_diff=f"{err:.2e}"))
        print("PART1", json.dumps(rows[-1]), flush=True)
    return rows


# ---- part 2 ----------------------------------------------------------------

def part2_child():
    """Times every shape under this process's TN_BATCH_GEMM setting."""
    from tnc_amd import hiplib
    from tnc_amd.contraction_path import ContractionPath
    from tnc_amd.executor import ContractionEngine
    from tnc_amd.tensor import CompositeTensor, LeafTensor, TensorData

    beta, i, j, k = 50, 1, 2, 3
    rng = np.random.default_rng(5)
    for mn, kk, nb in SHAPES:
        leaves = []
        for legs, dims in (([beta, i, k], [nb, mn, kk]),
                           ([beta, k, j], [nb, kk, mn])):
            data = (rng.standard_normal(dims)
                    + 1j * rng.standard_normal(dims))
            leaf = LeafTensor(legs, dims)
            leaf.set_tensor_data(TensorData(TensorData.MATRIX, matrix=data))
            leaves.append(leaf)
        eng = ContractionEngine(CompositeTensor(leaves),
                                ContractionPath.simple([(0, 1)]),
                                batch_edges=[beta])
        # an arena for every shape: no per-call hipMalloc on either side
        hiplib.check(hiplib.lib().tn_net_reserve(eng.net, 1 << 29),
                     "tn_net_reserve")
        ms = timed(eng.contract_batched)
        dev = [eng.contract_batched() for _ in range(REPS)]
        print("PART2", json.dumps(dict(
            mn=mn, k=kk, B=nb, cls=eng.batch_classes[0], wall=ms,
            dev=statistics.median(dev))), flush=True)
        eng.close()


def part2():
    runs = {"gemm": [], "loop": []}
    for _ in range(2):
        for side in ("gemm", "loop"):
            env = {k: v for k, v in os.environ.items() if k != "TN_BATCH_GEMM"}
            if side == "loop":
                env["TN_BATCH_GEMM"] = "0"
            proc = subprocess.run(
                [sys.executable, os.path.abspath(__file__), "--child"],
                cwd=ROOT, env=env, capture_output=True, text=True,
                timeout=600)
            if proc.returncode != 0:
                raise RuntimeError(f"{side} child failed: {proc.stderr[-2000:]}")
            runs[side].append([json.loads(l[6:])
                               for l in proc.stdout.splitlines()
                               if l.startswith("PART2 ")])
    rows = []
    for x, (mn, kk, nb) in enumerate(SHAPES):
        g = [r[x] for r in runs["gemm"]]
        l = [r[x] for r in runs["loop"]]
        gw = [t for r in g for t in r["wall"]]
        lw = [t for r in l for t in r["wall"]]
        rows.append(dict(
            mn=mn, k=kk, B=nb, cls=g[0]["cls"],
            gemm=spread(gw), loop=spread(lw),
            gemm_rounds=[round(statistics.median(r["wall"]), 4) for r in g],
            loop_rounds=[round(statistics.median(r["wall"]), 4) for r in l],
            gemm_dev=round(statistics.median(r["dev"] for r in g), 4),
            loop_dev=round(statistics.median(r["dev"] for r in l), 4),
            speedup=round(statistics.median(lw) / statistics.median(gw), 2)))
        print("PART2ROW", json.dumps(rows[-1]), flush=True)
    return rows


CLASS = ["NONE", "GATHER", "GEMM", "LOOP"]


def report(p1, p2):
    out = ["# Batch labels: measured on an MI355X", "",
           "Written by `scripts/batch_amplitudes.py`; the protocol is in its "
           "docstring.", "",
           f"Every timed call ends in a device synchronise. {WARMUP} warm-up "
           f"calls, then {REPS} timed; cells are median [min, max] of the "
           "host clock, ms.", "",
           "## 1. B amplitudes: one batched walk vs one engine per bitstring",
           "",
           f"Circuit: `sycamore_circuit({QUBITS}, {DEPTH}, {SEED})`, path: "
           "Greedy on the single-bitstring network, random bitstrings. "
           "\"walk\" is the steady-state contraction (batched: a plain walk, "
           "no hipGraph; per-bitstring engines: hipGraph replay, all B "
           "engines in turn), per amplitude. \"end to end\" adds network "
           "construction, planning, upload and the first contraction, per "
           "amplitude, one sample; the first row's batched sample also holds "
           "the process's first device initialisation and code-object load.",
           "",
           "| B | steps (NONE/GATHER/GEMM/LOOP) | batched walk, ms/amp | "
           "per-engine replay, ms/amp | batched end to end, ms/amp | "
           "per-engine end to end, ms/amp | max abs diff |",
           "|---|---|---|---|---|---|---|"]
    for r in p1:
        out.append(f"| {r['B']} | {r['steps']} ({'/'.join(map(str, r['classes']))})"
                   f" | {r['walk_batched']} | {r['walk_single']} | "
                   f"{r['e2e_batched']} | {r['e2e_single']} | "
                   f"{r['max_abs_diff']} |")
    out += ["", "## 2. Batched MFMA kernel vs the element step looped", "",
            "One-step batched walk `A[B,M,K] B[B,K,N] -> [B,M,N]`, c128, "
            "M = N, arena reserved. GEMM side: default; LOOP side: "
            "`TN_BATCH_GEMM=0`. Two child processes per side, alternated; "
            "\"rounds\" are the per-process medians. \"class\" is what the "
            "default planner chooses: where it says LOOP (the element plans "
            "split-K) both sides run the same code and the row measures "
            "noise. \"dev\" is the median device-event time of the walk.", "",
            "| M=N | K | B | class | default, ms | TN_BATCH_GEMM=0, ms | "
            "rounds default | rounds =0 | dev default | dev =0 | "
            "LOOP/default |",
            "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in p2:
        out.append(f"| {r['mn']} | {r['k']} | {r['B']} | {CLASS[r['cls']]} | "
                   f"{r['gemm']} | {r['loop']} | {r['gemm_rounds']} | "
                   f"{r['loop_rounds']} | {r['gemm_dev']} | {r['loop_dev']} | "
                   f"{r['speedup']} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "batch_amplitudes.md"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--part", type=int, default=0, help="1 or 2; 0 = both")
    args = ap.parse_args()
    from tnc_amd import hiplib

    if hiplib.device_count() == 0:
        raise SystemExit("no AMD GPU present: nothing can be measured here")
    if args.child:
        return part2_child()
    p1 = part1() if args.part in (0, 1) else []
    p2 = part2() if args.part in (0, 2) else []
    text = report(p1, p2)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
