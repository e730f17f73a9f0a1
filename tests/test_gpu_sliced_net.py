"""Sliced contraction inside one executor (tn_net_contract_sliced): the
leaves uploaded once, sliced on the device per assignment, one walk per
assignment over the reduced plan, the sum taken on the device.

The yardstick is the host-driven path (slicing.contract_sliced_gpu: one
fresh engine per slice_network(tn, assignment), summed on the host in
order). The on-device path runs the same kernels on the same inputs and
adds in the same order, so the comparison is bit for bit."""

import ctypes
import math

import numpy as np
import pytest

from oracle import contract_network
from oracle.adapters import network_to_otensors

pytestmark = pytest.mark.gpu

TN_ERR_INVALID = 1


def _per_slice(tn, replace, edges, dtype="c128"):
    """One fresh engine per assignment, in iter_assignments order."""
    from tnc_amd.executor import ContractionEngine
    from tnc_amd.slicing import iter_assignments, slice_network

    parts, legs = [], None
    for assignment in iter_assignments(tn, edges):
        eng = ContractionEngine(slice_network(tn, assignment), replace,
                                dtype=dtype)
        try:
            eng.contract()
            legs, data = eng.result()
        finally:
            eng.close()
        parts.append(np.array(data, copy=True))
    return legs, parts


def _host_sum(parts, which):
    total = np.array(parts[which[0]], copy=True)
    for t in which[1:]:
        total += parts[t]
    return total


@pytest.fixture(scope="module")
def eagle():
    """The 295-step network of test_sliced_contraction_gpu with its two
    sliced edges, the per-slice results and the direct contraction."""
    from tnc_amd import Greedy
    from tnc_amd.builders import random_circuit
    from tnc_amd.connectivity import ConnectivityLayout
    from tnc_amd.executor import contract_tensor_network_gpu
    from tnc_amd.slicing import _walk_sizes, find_slice_edges

    tn = random_circuit(16, 14, 0.5, 0.8, 3, ConnectivityLayout.EAGLE)
    replace = Greedy().find_path(tn).replace_path()
    peak, _, _ = _walk_sizes(tn, replace.toplevel)
    edges, _ = find_slice_edges(tn, replace.toplevel, peak / 4, max_edges=4)
    assert edges == [365, 362] and len(replace.toplevel) == 295
    legs, parts = _per_slice(tn, replace, edges)
    assert len(parts) == 4
    legs_d, direct = contract_tensor_network_gpu(tn, replace)
    return dict(tn=tn, replace=replace, edges=edges, legs=legs, parts=parts,
                legs_direct=legs_d, direct=np.array(direct, copy=True))


def test_same_bits_as_host_driven_path(eagle):
    from tnc_amd import contract_sliced_device
    from tnc_amd.slicing import contract_sliced_gpu

    tn, replace, edges = eagle["tn"], eagle["replace"], eagle["edges"]
    legs, got = contract_sliced_device(tn, replace, edges)
    legs_h, host = contract_sliced_gpu(tn, replace, edges)
    ref = contract_network(network_to_otensors(tn), replace)
    assert legs == legs_h == eagle["legs_direct"] == ref.legs
    print("device", complex(got), "host", complex(host),
          "direct", complex(eagle["direct"]), "oracle", complex(ref.data))
    assert np.array_equal(got, host)
    assert np.array_equal(host, _host_sum(eagle["parts"], [0, 1, 2, 3]))
    np.testing.assert_allclose(got, eagle["direct"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(got, ref.data, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("which", [[1, 3], [3, 1]])
def test_a_ranks_share(eagle, which):
    from tnc_amd import contract_sliced_device

    legs, got = contract_sliced_device(eagle["tn"], eagle["replace"],
                                       eagle["edges"], which=which)
    assert legs == eagle["legs"]
    assert np.array_equal(got, _host_sum(eagle["parts"], which))


def _three_leaf_network():
    """A[i:3, s:3, k:5] B[k:5, t:2, j:7] C[s:3, t:2, l:5], random complex."""
    from tnc_amd.tensor import CompositeTensor, LeafTensor, TensorData

    i, s, k, t, j, l = 1, 2, 3, 4, 5, 6
    rng = np.random.default_rng(20)
    leaves, arrays = [], []
    for legs, dims in (([i, s, k], [3, 3, 5]), ([k, t, j], [5, 2, 7]),
                       ([s, t, l], [3, 2, 5])):
        data = rng.standard_normal(dims) + 1j * rng.standard_normal(dims)
        leaf = LeafTensor(legs, dims)
        leaf.set_tensor_data(TensorData(TensorData.MATRIX, matrix=data))
        leaves.append(leaf)
        arrays.append(data)
    ref = np.einsum("isk,ktj,stl->ijl", *arrays)
    return CompositeTensor(leaves), [s, t], [i, j, l], ref


@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_nonpow2_radices_tensor_result_odd_count(dtype):
    from tnc_amd import contract_sliced_device
    from tnc_amd.contraction_path import ContractionPath

    tn, edges, final_legs, ref = _three_leaf_network()
    replace = ContractionPath.simple([(0, 1), (0, 2)])
    legs, got = contract_sliced_device(tn, replace, edges, dtype=dtype)
    assert legs == final_legs and got.shape == (3, 7, 5) and got.size == 105
    err = np.max(np.abs(got - ref) / np.abs(ref))
    print(dtype, "max relative error vs einsum", err)
    if dtype == "c128":
        assert got.dtype == np.complex128
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-13)
    else:
        assert got.dtype == np.complex64
        np.testing.assert_allclose(got, ref, rtol=2e-3)
    legs_p, parts = _per_slice(tn, replace, edges, dtype=dtype)
    assert legs_p == legs and len(parts) == 6
    assert parts[0].dtype == got.dtype
    assert np.array_equal(got, _host_sum(parts, list(range(6))))
    # a share in another order, through the non-pow2 digit decode
    _, share = contract_sliced_device(tn, replace, edges, dtype=dtype,
                                      which=[5, 2, 3])
    assert np.array_equal(share, _host_sum(parts, [5, 2, 3]))


def test_statevector():
    from tnc_amd import Circuit, Greedy, TensorData, contract_sliced_device
    from tnc_amd.executor import contract_tensor_network_gpu
    from tnc_amd.slicing import find_slice_edges

    c = Circuit()
    qr = c.allocate_register(6)
    qubits = list(qr.qubits())
    # T = diag(1, e^{i pi/4}) = u(0, 0, pi/4)
    t_gate = lambda: TensorData.from_gate("u", (0.0, 0.0, math.pi / 4))
    for q in qubits:
        c.append_gate(TensorData.from_gate("h"), [q])
    for _ in range(3):
        for a, b in zip(qubits, qubits[1:]):
            c.append_gate(TensorData.from_gate("cx"), [a, b])
        for q in qubits:
            c.append_gate(t_gate(), [q])
        for q in qubits:
            c.append_gate(TensorData.from_gate("h"), [q])
    tn, _ = c.into_statevector_network()
    replace = Greedy().find_path(tn).replace_path()
    edges, _ = find_slice_edges(tn, replace.toplevel, 0, max_edges=2)
    assert len(tn.tensors) == 63 and len(edges) == 2
    legs, got = contract_sliced_device(tn, replace, edges)
    legs_d, direct = contract_tensor_network_gpu(tn, replace)
    assert got.size == 64
    assert legs == legs_d
    np.testing.assert_allclose(got, direct, rtol=1e-12, atol=1e-13)
    ref = contract_network(network_to_otensors(tn), replace)
    np.testing.assert_allclose(got, ref.data, rtol=1e-10, atol=1e-12)


def _in_use(eng):
    from tnc_amd import hiplib

    used, cached = ctypes.c_uint64(), ctypes.c_uint64()
    hiplib.check(hiplib.lib().tn_net_pool_bytes(
        eng.net, ctypes.byref(used), ctypes.byref(cached)), "pool_bytes")
    assert cached.value >= 256 * 1024 * 1024  # the floor: replay can engage
    return used.value


def test_replay(eagle):
    from tnc_amd.executor import ContractionEngine

    want = _host_sum(eagle["parts"], [0, 1, 2, 3])
    eng = ContractionEngine(eagle["tn"], eagle["replace"],
                            slice_edges=eagle["edges"])
    try:
        assert eng.num_slices == 4
        sliced, in_use = [], []
        for _ in range(3):
            ms = eng.contract_sliced()
            assert ms > 0
            sliced.append(np.array(eng.result()[1], copy=True))
            in_use.append(_in_use(eng))
        assert np.array_equal(sliced[0], want)
        assert np.array_equal(sliced[1], sliced[0])
        assert np.array_equal(sliced[2], sliced[0])
        assert in_use[1] == in_use[2]
        eng.contract()
        plain = np.array(eng.result()[1], copy=True)
        np.testing.assert_allclose(plain, eagle["direct"], rtol=1e-12,
                                   atol=1e-13)
        eng.contract_sliced()
        assert np.array_equal(eng.result()[1], sliced[0])
        eng.contract()
        assert np.array_equal(eng.result()[1], plain)
        # a share after the full sum, and the full sum after a share
        eng.contract_sliced([2, 0])
        assert np.array_equal(eng.result()[1],
                              _host_sum(eagle["parts"], [2, 0]))
        eng.contract_sliced()
        assert np.array_equal(eng.result()[1], sliced[0])
    finally:
        eng.close()


def test_degenerate_no_labels(eagle):
    from tnc_amd.executor import ContractionEngine

    eng = ContractionEngine(eagle["tn"], eagle["replace"], slice_edges=[])
    try:
        assert eng.num_slices == 1
        eng.contract()
        legs, plain = eng.result()
        plain = np.array(plain, copy=True)
        eng.contract_sliced(which=[0])
        legs_s, got = eng.result()
        assert legs_s == legs
        assert np.array_equal(got, plain)
    finally:
        eng.close()


def test_refusals_on_a_live_net():
    from tnc_amd import hiplib
    from tnc_amd.contraction_path import ContractionPath
    from tnc_amd.executor import ContractionEngine

    tn, edges, final_legs, ref = _three_leaf_network()
    replace = ContractionPath.simple([(0, 1), (0, 2)])
    eng = ContractionEngine(tn, replace, slice_edges=edges)
    L = hiplib.lib()

    def call(labels, which):
        ms = ctypes.c_double()
        return L.tn_net_contract_sliced(
            eng.net, eng._pairs, len(eng.steps), hiplib._u64arr(labels),
            len(labels), hiplib._u64arr(which), len(which), ctypes.byref(ms))

    try:
        assert call(edges, [0, 6]) == TN_ERR_INVALID  # 6 assignments: 0..5
        assert "out of range" in hiplib.last_error()
        assert call([final_legs[1]], [0]) == TN_ERR_INVALID  # open leg j
        assert "final tensor" in hiplib.last_error()
        assert call(edges, []) == TN_ERR_INVALID
        assert hiplib.last_error()
        assert not L.tn_net_result_dev(eng.net)  # no result from a refusal
        with pytest.raises(RuntimeError, match="tn_net_contract_sliced"):
            eng.contract_sliced([7])
        eng.contract()
        legs, got = eng.result()
        assert legs == final_legs
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-13)
        eng.contract_sliced()
        np.testing.assert_allclose(eng.result()[1], ref, rtol=1e-12,
                                   atol=1e-13)
    finally:
        eng.close()
