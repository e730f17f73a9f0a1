"""The look-ahead pack of the walk, on a network small enough for a quick test.

Four leaves, three steps, all TTGT (legs of dim 2):

    M11 = 100..110  N10 = 200..209  K5 = 300..304  X6 = 400..405  Y7 = 500..506
    K1 = M11[5:] + N10[6:]          K2 = X6 + N10[:5]
    leaves: 0 = M11+K5   1 = K5+N10   2 = X6+K1   3 = K2+Y7
    path:   (0,1) (0,2) (3,0)

2048x1024x32 (the smallest shape the 3M gate admits), 2048x64x1024 and
128x64x2048 (both split-K). Leaf 2 is step 1's B and leaf 3 is step 2's A,
neither in GEMM order, so the walk packs both one step early on the second
stream, defers the frees of what the packs replace, joins the streams, and
captures that fork into its graph. The engine reserves an arena for this
network by itself (the prepack needs one). tests/native/layout_plan_check.cpp
checks the plan of this same network without a GPU.

The switches are read once per process: each setting (default,
TN_NO_PREPACK=1, TN_EPI_SCATTER=0) runs once in a child over the same saved
inputs. A child contracts three times (normal walk, capture + replay,
replay), then once profiled, and saves the result of each. With
TN_EPI_SCATTER=0 step 1 packs its A inline as well, its split-K buffer then
does not fit the arena, and the capture is given up for normal walks: that
child covers the way back out of a capture that spills.
"""

import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M11 = [100 + x for x in range(11)]
N10 = [200 + x for x in range(10)]
K5 = [300 + x for x in range(5)]
X6 = [400 + x for x in range(6)]
Y7 = [500 + x for x in range(7)]
K1 = M11[5:] + N10[6:]
K2 = X6 + N10[:5]
LEAVES = [M11 + K5, K5 + N10, X6 + K1, K2 + Y7]
STEPS = [(0, 1), (0, 2), (3, 0)]
FINAL = Y7 + M11[:5] + N10[5:6]

SETTINGS = {"default": {}, "no_prepack": {"TN_NO_PREPACK": "1"},
            "scatter_off": {"TN_EPI_SCATTER": "0"}}

# max|got - ref| / max|ref| against the step-by-step oracle. Measured with
# this file's children on the library before the walk plan, on an MI355X:
# 8.0912e-16 in each of the three settings (they agree bit for bit). Four
# times that, only so the check does not sit on the last bit; a wrong axis
# order is off by the size of the values.
REL_BOUND = 4 * 8.0912e-16

CHILD = r"""
import ctypes, hashlib, json, sys
import numpy as np
from tnc_amd import hiplib
from tnc_amd.contraction_path import ContractionPath
from tnc_amd.executor import ContractionEngine
from tnc_amd.tensor import CompositeTensor, LeafTensor, TensorData

d, dst = sys.argv[1], sys.argv[2]
spec = json.load(open(d + "/spec.json"))
inp = np.load(d + "/inputs.npz")
leaves = []
for x, legs in enumerate(spec["leaves"]):
    t = LeafTensor(legs, [2] * len(legs))
    t.set_tensor_data(TensorData(TensorData.MATRIX, matrix=inp["l%d" % x]))
    leaves.append(t)
steps = [tuple(p) for p in spec["steps"]]
eng = ContractionEngine(CompositeTensor(leaves), ContractionPath.simple(steps))
arrs, res = {}, {}
try:
    cached = ctypes.c_uint64()
    hiplib.check(hiplib.lib().tn_net_pool_bytes(eng.net, None,
                                                ctypes.byref(cached)),
                 "tn_net_pool_bytes")
    res["arena"] = int(cached.value)
    for name in ("walk", "capture", "replay"):
        eng.contract()
        res["legs"], arrs[name] = eng.result()
    _, _, _, kind = eng.contract_profiled()
    legs, arrs["profiled"] = eng.result()
    assert legs == res["legs"]
finally:
    eng.close()
res["legs"] = [int(l) for l in res["legs"]]
res["kind"] = [int(k) for k in kind]
res["sha256"] = hashlib.sha256(arrs["walk"].tobytes()).hexdigest()
np.savez(dst + ".npz", **arrs)
json.dump(res, open(dst + ".json", "w"))
print("PREPACK_CHILD_OK sha256", res["sha256"])
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("prepack"))
    rng = np.random.default_rng(808)
    arrs = {}
    for x, legs in enumerate(LEAVES):
        dims = [2] * len(legs)
        arrs["l%d" % x] = (rng.standard_normal(dims)
                           + 1j * rng.standard_normal(dims))
    with open(os.path.join(d, "spec.json"), "w") as f:
        json.dump({"leaves": LEAVES, "steps": STEPS}, f)
    np.savez(os.path.join(d, "inputs.npz"), **arrs)
    # the oracle, step by step, once
    mid0 = oracle.contract_ndarrays(M11 + N10, LEAVES[0], arrs["l0"],
                                    LEAVES[1], arrs["l1"])
    mid1_legs = M11[:5] + N10[:6] + X6
    mid1 = oracle.contract_ndarrays(mid1_legs, M11 + N10, mid0, LEAVES[2],
                                    arrs["l2"])
    ref = oracle.contract_ndarrays(FINAL, LEAVES[3], arrs["l3"], mid1_legs,
                                   mid1)
    ref.setflags(write=False)
    outs = {}
    for mode, extra in SETTINGS.items():
        env = {k: v for k, v in os.environ.items()
               if k not in ("TN_NO_PREPACK", "TN_EPI_SCATTER")}
        env.update(extra)
        dst = os.path.join(d, "out_" + mode)
        proc = subprocess.run([sys.executable, "-c", CHILD, d, dst], cwd=ROOT,
                              env=env, capture_output=True, text=True,
                              timeout=120)
        print(f"--- child {mode} ---\n{proc.stdout[-2000:]}\n"
              f"{proc.stderr[-4000:]}")
        assert proc.returncode == 0, mode
        assert "PREPACK_CHILD_OK" in proc.stdout, mode
        outs[mode] = (dict(np.load(dst + ".npz")),
                      json.load(open(dst + ".json")))
    return ref, outs


@pytest.mark.parametrize("mode", list(SETTINGS))
def test_every_walk_of_a_child_agrees(runs, mode):
    """Normal walk, captured graph, replay and profiled walk: same bits."""
    _, outs = runs
    arrs, res = outs[mode]
    assert res["arena"] > 0  # no arena, no prepack: the test would be idle
    assert res["kind"] == [2, 2, 2]
    assert res["legs"] == FINAL
    for name in ("capture", "replay", "profiled"):
        assert np.array_equal(arrs["walk"], arrs[name]), name
    assert res["sha256"] == hashlib.sha256(arrs["walk"].tobytes()).hexdigest()
    print(f"sha256 {mode}: {res['sha256']}")


def test_prepack_changes_no_bit(runs):
    """Same kernels, same operands; only the stream and the moment of the
    packs differ."""
    _, outs = runs
    assert np.array_equal(outs["default"][0]["walk"],
                          outs["no_prepack"][0]["walk"])
    assert outs["default"][1]["sha256"] == outs["no_prepack"][1]["sha256"]


def test_a_path_without_a_plan_is_refused_and_leaves_nothing():
    """A dead operand, or a path that stops early, has no walk plan: the
    walk says so, the arena is empty afterwards and the net still works."""
    import ctypes

    from tnc_amd import hiplib
    from tnc_amd.contraction_path import ContractionPath
    from tnc_amd.executor import ContractionEngine
    from tnc_amd.tensor import CompositeTensor, LeafTensor, TensorData

    rng = np.random.default_rng(9)
    leaves = []
    for legs in ([1, 2], [2, 3], [3, 4]):
        t = LeafTensor(legs, [2, 2])
        t.set_tensor_data(TensorData(
            TensorData.MATRIX, matrix=rng.standard_normal((2, 2)) + 0j))
        leaves.append(t)
    eng = ContractionEngine(CompositeTensor(leaves),
                            ContractionPath.simple([(0, 1), (0, 2)]))
    L = hiplib.lib()
    try:
        hiplib.check(L.tn_net_reserve(eng.net, 1 << 20), "tn_net_reserve")
        eng.contract()
        legs, good = eng.result()
        for pairs, why in (([0, 1, 1, 2], "invalid contraction path step"),
                           ([0, 1], "path did not fully contract")):
            rc = L.tn_net_contract(eng.net, hiplib._u64arr(pairs),
                                   len(pairs) // 2, None)
            assert rc == 1 and why in hiplib.last_error(), hiplib.last_error()
            used = ctypes.c_uint64(1)
            hiplib.check(L.tn_net_pool_bytes(eng.net, ctypes.byref(used),
                                             None), "tn_net_pool_bytes")
            assert used.value == 0
        eng.contract()
        assert eng.result()[0] == legs
        assert np.array_equal(eng.result()[1], good)
    finally:
        eng.close()


@pytest.mark.parametrize("mode", list(SETTINGS))
def test_agrees_with_the_oracle(runs, mode):
    ref, outs = runs
    got = outs[mode][0]["walk"]
    rel = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    print(f"max|got - ref| / max|ref| ({mode}): {rel:.3e}")
    assert rel <= REL_BOUND
