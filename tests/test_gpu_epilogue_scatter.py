"""Scatter epilogue of the c128 3M GEMM and the layout pre-pass that feeds it.

A step whose out order interleaves M and N legs is stored by the GEMM itself
when the planner admits it (tests/test_layout_plan.py has the gate); with
TN_EPI_SCATTER=0 the same binary writes a temporary C and permutes it. The
arithmetic is the same either way, only the addresses differ, so the two
must agree bit for bit.

TN_EPI_SCATTER is read once per process: each setting runs once in a child
over the same saved inputs, and the tests share what the children wrote.

Shapes: M = 2^11, N = 2^10, K = 2^5 in legs of dim 2 is the smallest shape
the 3M gate admits (256 tiles), so every case has several row and column
tiles. The "high" case has N = 2^17 and puts the seven tile-local row bits on
destination bits 21-27: byte offsets reach 2^32, which a 32-bit offset
anywhere in the epilogue would wrap. It is checked on the device, against
torch's matmul, to keep the 4 GiB result off the host.
"""

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
N17 = [200 + x for x in range(17)]
K5 = [300 + x for x in range(5)]
X6 = [400 + x for x in range(6)]
# M and N legs interleaved, the three lowest N legs lowest (run of 8 columns)
INTERLEAVED = M11[:6] + N10[:4] + M11[6:10] + N10[4:7] + [M11[10]] + N10[7:]
# low seven row bits (M11[4:]) on top of everything, three N legs lowest
HIGH = M11[4:] + N17[:14] + M11[:4] + N17[14:]
# chain: step 1 contracts six legs of M_0 and four of N_0 with leaf 2
K1 = M11[5:] + N10[6:]

CHILD = r"""
import ctypes, json, sys
import numpy as np
import torch
from tnc_amd import hiplib
from tnc_amd.contraction_path import ContractionPath
from tnc_amd.executor import ContractionEngine
from tnc_amd.tensor import CompositeTensor, LeafTensor, TensorData

d, dst = sys.argv[1], sys.argv[2]
spec = json.load(open(d + "/spec.json"))
inp = np.load(d + "/inputs.npz")
L = hiplib.lib()
dev = torch.device("cuda:0")


def einsum_dev(out_legs, a_legs, a, b_legs, b):
    # a, b: contiguous device tensors, all legs of dim 2
    out = torch.empty([2] * len(out_legs), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize()
    u = hiplib._u64arr
    hiplib.check(L.tn_einsum_c128_dev(
        u(out_legs), u([2] * len(out_legs)), len(out_legs),
        u(a_legs), u([2] * len(a_legs)), None, a.data_ptr(), len(a_legs),
        u(b_legs), u([2] * len(b_legs)), None, b.data_ptr(), len(b_legs),
        out.data_ptr(), None), "tn_einsum_c128_dev")
    torch.cuda.synchronize()
    return out


res, arrs = {}, {}
# small: the gated shape, twice
c = spec["small"]
a = torch.from_numpy(inp["small_a"]).to(dev)
b = torch.from_numpy(inp["small_b"]).to(dev)
arrs["small"] = einsum_dev(c["out"], c["a"], a, c["b"], b).cpu().numpy()
arrs["small_again"] = einsum_dev(c["out"], c["a"], a, c["b"], b).cpu().numpy()

# high: checked on the device
c = spec["high"]
a = torch.from_numpy(inp["high_a"]).to(dev)
b = torch.from_numpy(inp["high_b"]).to(dev)
got = einsum_dev(c["out"], c["a"], a, c["b"], b)
nm, nn, nk = c["nm"], c["nn"], c["nk"]
ref = (a.reshape(2 ** nm, 2 ** nk) @ b.reshape(2 ** nk, 2 ** nn)).reshape(
    [2] * (nm + nn))
mn = c["a"][:nm] + c["b"][nk:]
ref = ref.permute([mn.index(l) for l in c["out"]])
err = (got - ref).abs()
res["high_max_abs_err"] = float(err.max())
res["high_allclose"] = bool(torch.all(err <= 1e-12 * ref.abs() + 1e-10))
del err
res["high_max_abs_ref"] = float(ref.abs().max())
# order-sensitive digest, to compare the two settings bit for bit
w = torch.arange(got.numel() * 2, dtype=torch.int64, device=dev) | 1
res["high_digest"] = int((torch.view_as_real(got).reshape(-1)
                          .view(torch.int64) * w).sum())
del got, ref, w

# chain: three leaves, two steps
leaves = []
for name, legs in (("c0", spec["chain"]["l0"]), ("c1", spec["chain"]["l1"]),
                   ("c2", spec["chain"]["l2"])):
    t = LeafTensor(legs, [2] * len(legs))
    t.set_tensor_data(TensorData(TensorData.MATRIX, matrix=inp[name]))
    leaves.append(t)
steps = [(0, 1), (0, 2)]
eng = ContractionEngine(CompositeTensor(leaves), ContractionPath.simple(steps))
try:
    _, _, _, kind = eng.contract_profiled()
    legs, data = eng.result()
    _, _, _, kind2 = eng.contract_profiled()
    legs2, data2 = eng.result()
finally:
    eng.close()
res["chain_kind"] = list(kind)
res["chain_legs"] = [int(l) for l in legs]
assert legs2 == legs and list(kind2) == list(kind)
arrs["chain"], arrs["chain_again"] = data, data2
scatter, inline = hiplib.plan_layouts(
    [(t.legs, t.bond_dims) for t in leaves], steps)
res["chain_scatter"], res["chain_inline"] = scatter, inline
np.savez(dst + ".npz", **arrs)
json.dump(res, open(dst + ".json", "w"))
print("SCATTER_CHILD_OK")
"""


def _cplx(rng, nlegs):
    dims = [2] * nlegs
    return rng.standard_normal(dims) + 1j * rng.standard_normal(dims)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("scatter"))
    rng = np.random.default_rng(55)
    spec = {
        "small": dict(out=INTERLEAVED, a=M11 + K5, b=K5 + N10),
        "high": dict(out=HIGH, a=M11 + K5, b=K5 + N17, nm=11, nn=17, nk=5),
        "chain": dict(l0=M11 + K5, l1=K5 + N10, l2=K1 + X6),
    }
    arrs = {
        "small_a": _cplx(rng, 16), "small_b": _cplx(rng, 15),
        "high_a": _cplx(rng, 16), "high_b": _cplx(rng, 22),
        "c0": _cplx(rng, 16), "c1": _cplx(rng, 15), "c2": _cplx(rng, 16),
    }
    with open(os.path.join(d, "spec.json"), "w") as f:
        json.dump(spec, f)
    np.savez(os.path.join(d, "inputs.npz"), **arrs)
    outs = {}
    for mode in ("on", "off"):
        env = dict(os.environ)
        env.pop("TN_EPI_SCATTER", None)
        if mode == "off":
            env["TN_EPI_SCATTER"] = "0"
        dst = os.path.join(d, "out_" + mode)
        proc = subprocess.run([sys.executable, "-c", CHILD, d, dst], cwd=ROOT,
                              env=env, capture_output=True, text=True,
                              timeout=240)
        print(f"--- child, scatter {mode} ---\n{proc.stdout[-2000:]}\n"
              f"{proc.stderr[-4000:]}")
        assert proc.returncode == 0, mode
        assert "SCATTER_CHILD_OK" in proc.stdout, mode
        outs[mode] = (dict(np.load(dst + ".npz")),
                      json.load(open(dst + ".json")))
    return spec, arrs, outs


def test_planner_admits_the_cases():
    """The cases above run the scatter epilogue, not the unpack permute."""
    from tnc_amd import hiplib as H

    for out, a, b in ((INTERLEAVED, M11 + K5, K5 + N10),
                      (HIGH, M11 + K5, K5 + N17)):
        p = H.plan_step(out, [2] * len(out), a, [2] * len(a), b, [2] * len(b))
        assert p.kernel == H.GEMM_C128_3M and not p.direct
        assert (p.scatter_out, p.kind, p.ws_tmp_c) == (1, 2, 0)


def test_scatter_equals_unpack_bit_for_bit(runs):
    spec, arrs, outs = runs
    on, off = outs["on"][0]["small"], outs["off"][0]["small"]
    assert np.array_equal(on, off)
    c = spec["small"]
    ref = oracle.contract_ndarrays(c["out"], c["a"], arrs["small_a"], c["b"],
                                   arrs["small_b"])
    print("small: max|got - ref| =", float(np.max(np.abs(on - ref))))
    np.testing.assert_allclose(on, ref, rtol=1e-12, atol=1e-10)
    # np.einsum takes sublist labels below 52
    small = {l: x for x, l in enumerate(M11 + N10 + K5)}
    sub = lambda legs: [small[l] for l in legs]  # noqa: E731
    np.testing.assert_allclose(
        on, np.einsum(arrs["small_a"], sub(c["a"]), arrs["small_b"],
                      sub(c["b"]), sub(c["out"])), rtol=1e-12, atol=1e-10)


def test_offsets_past_32_bits(runs):
    _, _, outs = runs
    on, off = outs["on"][1], outs["off"][1]
    print("high: max|got - ref| =", on["high_max_abs_err"], "max|ref| =",
          on["high_max_abs_ref"])
    # elementwise |got - ref| <= 1e-12 |ref| + 1e-10, evaluated on the device
    assert on["high_allclose"]
    assert on["high_digest"] == off["high_digest"]


def test_chain_consumer_finds_operand_ready(runs):
    spec, arrs, outs = runs
    (a_on, r_on), (a_off, r_off) = outs["on"], outs["off"]
    assert r_on["chain_kind"] == [2, 2]
    assert r_on["chain_scatter"] == [1, 0]
    assert r_on["chain_inline"][1] == 0
    # switched off: step 0 is direct, step 1 packs step 0's output inline
    assert r_off["chain_kind"] == [2, 2]
    assert r_off["chain_scatter"] == [0, 0]
    assert r_off["chain_inline"][1] == 2 ** 21 * 16
    c = spec["chain"]
    mid_legs = M11 + N10
    mid = oracle.contract_ndarrays(mid_legs, c["l0"], arrs["c0"], c["l1"],
                                   arrs["c1"])
    legs = r_on["chain_legs"]
    assert legs == r_off["chain_legs"] == M11[:5] + N10[:6] + X6
    ref = oracle.contract_ndarrays(legs, mid_legs, mid, c["l2"], arrs["c2"])
    print("chain: max|on - ref| =", float(np.max(np.abs(a_on["chain"] - ref))),
          "max|on - off| =",
          float(np.max(np.abs(a_on["chain"] - a_off["chain"]))))
    np.testing.assert_allclose(a_on["chain"], ref, rtol=1e-12, atol=1e-10)
    np.testing.assert_allclose(a_on["chain"], a_off["chain"], rtol=1e-12,
                               atol=1e-10)


def test_deterministic(runs):
    _, _, outs = runs
    arrs = outs["on"][0]
    assert np.array_equal(arrs["small"], arrs["small_again"])
    assert np.array_equal(arrs["chain"], arrs["chain_again"])
