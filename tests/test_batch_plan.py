"""Batch labels, planner side (tn_plan_step_batched, tn_plan_batch_walk):
classes, dispatch counts, workspaces, refusals and the walk's stored orders.
Needs the built library, no GPU. All operands contiguous unless a case says
otherwise."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BETA, GAMMA, I_, J_, K_ = 50, 51, 1, 2, 3


def plan(out, a, b, batch, dtype="c128", **kw):
    """out / a / b: [(label, dim), ...]."""
    from tnc_amd import hiplib

    return hiplib.plan_step_batched(
        [l for l, _ in out], [d for _, d in out],
        [l for l, _ in a], [d for _, d in a],
        [l for l, _ in b], [d for _, d in b], batch, dtype=dtype, **kw)


def mm(m, n, k, beta=3):
    """A[beta, i:m, k] B[beta, k, j:n] -> [beta, i, j]"""
    return ([(BETA, beta), (I_, m), (J_, n)],
            [(BETA, beta), (I_, m), (K_, k)],
            [(BETA, beta), (K_, k), (J_, n)])


def fields(p):
    return {f: getattr(p, f) for f, _ in p._fields_}


# ---- classes and dispatch counts ------------------------------------------

def test_gather_class():
    from tnc_amd import hiplib as H

    p = plan(*mm(2, 2, 2), [BETA])
    assert (p.cls, p.dispatches, p.batch) == (H.BATCH_GATHER, 1, 3)
    assert p.elem.route == H.ROUTE_GATHER
    assert (p.elem.m, p.elem.n, p.elem.k) == (2, 2, 2)
    assert p.ws_pack_a == 0 and p.ws_pack_b == 0
    # the batch axis of 3 leads the launch's out map: div/mod, whatever the
    # pow2 element alone would take
    assert p.gather_kernel == H.GK_SMALLK
    assert p.elem.gather_kernel == H.GK_SMALLK_P2


def test_gather_class_kernel():
    """The batch-level gather kernel counts the batch axes in; the other
    classes report none."""
    from tnc_amd import hiplib as H

    p = plan(*mm(2, 2, 2, beta=4), [BETA])
    assert (p.cls, p.batch) == (H.BATCH_GATHER, 4)
    assert p.gather_kernel == p.elem.gather_kernel == H.GK_SMALLK_P2
    # K past the LDS table, skinny element
    p = plan(*mm(2, 2, 128, beta=4), [BETA])
    assert (p.cls, p.gather_kernel) == (H.BATCH_GATHER, H.GK_ANYK_P2)
    p = plan(*mm(2, 2, 128, beta=3), [BETA])
    assert (p.gather_kernel, p.elem.gather_kernel) == (H.GK_ANYK,
                                                       H.GK_ANYK_P2)
    # no batch label, GEMM and LOOP classes: no batch-level launch
    p = plan([(I_, 2), (J_, 2)], [(I_, 2), (K_, 2)], [(K_, 2), (J_, 2)],
             [BETA])
    assert (p.cls, p.gather_kernel) == (H.BATCH_NONE, H.GK_NONE)
    assert p.elem.gather_kernel == H.GK_SMALLK_P2
    p = plan(*mm(40, 40, 72), [BETA])
    assert (p.cls, p.gather_kernel) == (H.BATCH_GEMM, H.GK_NONE)
    p = plan([(BETA, 3)], [(BETA, 3), (K_, 128)], [(BETA, 3), (K_, 128)],
             [BETA])
    assert (p.cls, p.gather_kernel) == (H.BATCH_LOOP, H.GK_NONE)


@pytest.mark.parametrize("dtype,esize", [("c128", 16), ("c64", 8)])
def test_gemm_class_and_packs(dtype, esize):
    from tnc_amd import hiplib as H

    out, a, b = mm(17, 65, 67)
    p = plan(out, a, b, [BETA], dtype=dtype)
    assert (p.cls, p.dispatches, p.batch) == (H.BATCH_GEMM, 1, 3)
    assert p.elem.route == H.ROUTE_TTGT and p.elem.splitk == 1
    assert p.ws_pack_a == 0 and p.ws_pack_b == 0
    # A given as [M][beta][K]: one batched pack of A, none of B
    a_mbk = [a[1], a[0], a[2]]
    p = plan(out, a_mbk, b, [BETA], dtype=dtype)
    assert p.cls == H.BATCH_GEMM
    assert p.ws_pack_a == 3 * 17 * 67 * esize and p.ws_pack_b == 0
    # the same layout handed over as a strided view of a [beta][M][K] buffer
    # is ready again
    p = plan(out, a_mbk, b, [BETA], dtype=dtype,
             a_strides=[67, 17 * 67, 1])
    assert p.cls == H.BATCH_GEMM and p.ws_pack_a == 0


def test_loop_class_splitk():
    from tnc_amd import hiplib as H

    p = plan(*mm(32, 32, 256), [BETA])
    assert (p.cls, p.dispatches) == (H.BATCH_LOOP, 3)
    assert p.elem.splitk == 4


def test_loop_class_dot():
    from tnc_amd import hiplib as H

    p = plan(*mm(1, 1, 100), [BETA])
    assert (p.cls, p.dispatches) == (H.BATCH_LOOP, 3)
    assert p.elem.route == H.ROUTE_DOT


def test_loop_class_full_grid():
    from tnc_amd import hiplib as H

    p = plan(*mm(2048, 1024, 128, beta=2), [BETA])
    assert (p.cls, p.dispatches) == (H.BATCH_LOOP, 2)
    assert p.elem.row_tiles * p.elem.col_tiles == 256
    # one row tile fewer and the element shares a launch
    p = plan(*mm(2048 - 128, 1024, 128, beta=2), [BETA])
    assert p.cls == H.BATCH_GEMM


def test_two_batch_labels():
    from tnc_amd import hiplib as H

    out = [(GAMMA, 3), (BETA, 2), (I_, 16), (J_, 16)]
    a = [(BETA, 2), (GAMMA, 3), (I_, 16), (K_, 68)]
    b = [(BETA, 2), (GAMMA, 3), (K_, 68), (J_, 16)]
    p = plan(out, a, b, [BETA, GAMMA])
    assert p.batch == 6 and p.cls == H.BATCH_GEMM
    # out leads with [gamma, beta]; A and B store [beta, gamma]: both packed
    assert p.ws_pack_a == 6 * 16 * 68 * 16 and p.ws_pack_b == 6 * 68 * 16 * 16
    out = [(BETA, 2), (GAMMA, 3), (I_, 16), (J_, 16)]
    p = plan(out, a, b, [GAMMA, BETA])
    assert p.batch == 6 and p.ws_pack_a == 0 and p.ws_pack_b == 0


@pytest.mark.parametrize("batch", [[BETA], []])
def test_none_class_equals_plan_step(batch):
    """beta carried by A only (a free label), or no batch label listed."""
    from tnc_amd import hiplib as H

    out = [(BETA, 3), (I_, 32), (J_, 48)]
    a = [(BETA, 3), (I_, 32), (K_, 96)]
    b = [(K_, 96), (J_, 48)]
    p = plan(out, a, b, batch, has_stream2=True)
    ref = H.plan_step([l for l, _ in out], [d for _, d in out],
                      [l for l, _ in a], [d for _, d in a],
                      [l for l, _ in b], [d for _, d in b], has_stream2=True)
    assert (p.cls, p.batch, p.dispatches) == (H.BATCH_NONE, 1, 1)
    assert p.ws_pack_a == 0 and p.ws_pack_b == 0
    assert fields(p.elem) == fields(ref)
    assert p.elem.m == 96 and p.elem.n == 48


# ---- refusals --------------------------------------------------------------

def refused(out, a, b, batch):
    from tnc_amd import hiplib

    with pytest.raises(RuntimeError, match="rc=1"):
        plan(out, a, b, batch)
    return hiplib.last_error()


def test_refusals():
    out, a, b = mm(4, 4, 4)
    assert (refused([out[1], out[0], out[2]], a, b, [BETA])
            == "batch labels must lead out")
    assert (refused(out[1:], a, b, [BETA])
            == f"batch label {BETA} missing from out")
    assert (refused(out, a, [(BETA, 2)] + b[1:], [BETA])
            == f"batch dim mismatch on label {BETA}")
    assert (refused([(BETA, 2)] + out[1:], a, b, [BETA])
            == f"batch dim mismatch on label {BETA}")
    # in A, B and out but not listed: today's text
    assert (refused(out, a, b, [])
            == f"out label {BETA} present in both inputs")
    assert (refused(out, a, b, [GAMMA])
            == f"out label {BETA} present in both inputs")


# ---- environment switch (read once: a child process) -----------------------

CHILD = r"""
import json, sys
from tnc_amd import hiplib
case = json.loads(sys.argv[1])
p = hiplib.plan_step_batched(*case["args"])
print("PLAN " + json.dumps({"cls": p.cls, "dispatches": p.dispatches}))
"""


def test_env_batch_gemm_off():
    from tnc_amd import hiplib as H

    out, a, b = mm(17, 65, 67)
    args = [[l for l, _ in out], [d for _, d in out],
            [l for l, _ in a], [d for _, d in a],
            [l for l, _ in b], [d for _, d in b], [BETA]]
    got = {}
    for value in ("0", None):
        env = {k: v for k, v in os.environ.items() if k != "TN_BATCH_GEMM"}
        if value is not None:
            env["TN_BATCH_GEMM"] = value
        proc = subprocess.run(
            [sys.executable, "-c", CHILD, json.dumps({"args": args})],
            cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert proc.returncode == 0, (proc.stdout, proc.stderr)
        line = [l for l in proc.stdout.splitlines()
                if l.startswith("PLAN ")][-1]
        got[value] = json.loads(line[5:])
    assert got["0"] == {"cls": H.BATCH_LOOP, "dispatches": 3}
    assert got[None] == {"cls": H.BATCH_GEMM, "dispatches": 1}


# ---- plan_batch_walk -------------------------------------------------------

# V[e4,k96] X[beta3,a32,e4] Y[beta3,k96,c48] Z[beta3,c48,a32]
E_, KK, A_, C_ = 10, 11, 12, 13
FOUR_LEAVES = [([E_, KK], [4, 96]), ([BETA, A_, E_], [3, 32, 4]),
               ([BETA, KK, C_], [3, 96, 48]), ([BETA, C_, A_], [3, 48, 32])]
FOUR_STEPS = [(1, 0), (1, 2), (1, 3)]


def test_walk_four_leaves():
    from tnc_amd import hiplib as H

    cls, labels, ws = H.plan_batch_walk(FOUR_LEAVES, FOUR_STEPS, [BETA])
    assert cls == [H.BATCH_NONE, H.BATCH_GEMM, H.BATCH_LOOP]
    assert labels == [[BETA, A_, KK], [BETA, A_, C_], [BETA]]
    # [beta][a][k] and [beta][k][c] are GEMM-ready; the dot asks for its
    # partials
    assert ws[1] == 0 and ws[2] > 0
    # no batch label listed: beta is contracted at the last step
    cls, labels, _ = H.plan_batch_walk(FOUR_LEAVES, FOUR_STEPS, [])
    assert cls == [H.BATCH_NONE] * 3
    assert labels == [[BETA, A_, KK], [A_, C_], [BETA]]


def circuit_network():
    from tnc_amd import Greedy
    from tnc_amd.builders import sycamore_circuit
    from tnc_amd.contraction_path import flatten_network

    strings = ["010110100", "111000111", "000000000", "010110100", "101010101"]
    tn, _, beta = sycamore_circuit(9, 4, 7).into_amplitudes_network(strings)
    single, _ = sycamore_circuit(9, 4, 7).into_amplitude_network(strings[0])
    replace = Greedy().find_path(single).replace_path()
    leaves, steps, _ = flatten_network(tn, replace)
    return [(t.legs, t.bond_dims) for t in leaves], steps, beta


def test_walk_circuit():
    from tnc_amd import hiplib as H

    leaves, steps, beta = circuit_network()
    assert len(leaves) == 74 and len(steps) == 73
    cls, labels, ws = H.plan_batch_walk(leaves, steps, [beta])
    assert labels[-1] == [beta]
    assert H.BATCH_GATHER in cls
    # the part of the circuit upstream of every bra runs once
    assert cls[0] == H.BATCH_NONE and beta not in labels[0]


def test_walk_refusals():
    from tnc_amd import hiplib as H

    def refused(leaves, steps, batch):
        with pytest.raises(RuntimeError, match="rc=1"):
            H.plan_batch_walk(leaves, steps, batch)
        return H.last_error()

    assert (refused(FOUR_LEAVES, FOUR_STEPS, [BETA, BETA])
            == f"batch label {BETA} is listed twice")
    assert (refused(FOUR_LEAVES, FOUR_STEPS, [GAMMA])
            == f"batch label {GAMMA} is in no leaf")
    bad = list(FOUR_LEAVES)
    bad[3] = ([BETA, C_, A_], [2, 48, 32])
    assert (refused(bad, FOUR_STEPS, [BETA])
            == f"batch label {BETA} has differing dims across leaves")
    assert (refused(FOUR_LEAVES, [(1, 0), (1, 0)], [BETA])
            == "invalid contraction path step")
    wide = [(list(range(100, 141)), [1] * 41), ([7], [2])]
    assert refused(wide, [(0, 1)], []) == "tensor rank exceeds 40"
