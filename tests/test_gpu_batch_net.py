"""Batched network contraction (tn_net_contract_batched): many bitstrings'
amplitudes in one walk. The reference for a network is the oracle on
slicing.slice_network(tn, {beta: r}), row by row."""

import ctypes

import numpy as np
import pytest

from oracle import contract_network
from oracle.adapters import network_to_otensors

pytestmark = pytest.mark.gpu

TOL = {"c128": dict(rtol=1e-10, atol=1e-12), "c64": dict(rtol=2e-3, atol=1e-4)}
STRINGS = ["010110100", "111000111", "000000000", "010110100", "101010101"]


def _circuit():
    from tnc_amd.builders import sycamore_circuit

    return sycamore_circuit(9, 4, 7)


def _path(bitstring):
    """Greedy on the single-bitstring network of a fresh circuit."""
    from tnc_amd import Greedy

    single, _ = _circuit().into_amplitude_network(bitstring)
    return Greedy().find_path(single).replace_path()


def _oracle_rows(tn, replace, beta, nrows, legs):
    """Row r = the oracle's contraction of bitstring r's own network, its
    axes put in the order `legs`."""
    from tnc_amd.slicing import slice_network

    rows = []
    for r in range(nrows):
        ref = contract_network(
            network_to_otensors(slice_network(tn, {beta: r})), replace)
        assert sorted(ref.legs) == sorted(legs)
        data = np.asarray(ref.data).reshape([2] * len(ref.legs))
        rows.append(np.transpose(data, [ref.legs.index(l) for l in legs]))
    return np.stack(rows)


@pytest.fixture(scope="module")
def amplitudes():
    tn, _, beta = _circuit().into_amplitudes_network(STRINGS)
    replace = _path(STRINGS[0])
    assert len(tn.tensors) == 74 and len(replace.toplevel) == 73
    ref = _oracle_rows(tn, replace, beta, len(STRINGS), [])
    assert ref.shape == (5,)
    # amplitudes of order 2^-4.5, none near zero: rtol is what decides
    assert 5e-3 < np.min(np.abs(ref)) and np.max(np.abs(ref)) < 1e-1
    return dict(tn=tn, replace=replace, beta=beta, ref=ref)


@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_circuit_amplitudes(amplitudes, dtype):
    from tnc_amd import hiplib as H
    from tnc_amd.executor import ContractionEngine, amplitudes_gpu

    tn, replace, beta = (amplitudes[k] for k in ("tn", "replace", "beta"))
    legs, got = amplitudes_gpu(tn, replace, beta, dtype=dtype)
    assert legs == [beta] and got.shape == (5,)
    print(dtype, "max rel err vs oracle",
          np.max(np.abs(got - amplitudes["ref"]) / np.abs(amplitudes["ref"])))
    np.testing.assert_allclose(got, amplitudes["ref"], **TOL[dtype])
    assert got[0] == got[3]  # the same bitstring twice
    eng = ContractionEngine(tn, replace, dtype=dtype, batch_edges=[beta])
    try:
        assert H.BATCH_GATHER in eng.batch_classes
        assert eng.total_flops > 0
        assert eng.contract_batched() > 0
        first = np.array(eng.result()[1], copy=True)
        eng.contract_batched()
        legs2, second = eng.result()
        assert legs2 == [beta]
        assert np.array_equal(first, got) and np.array_equal(second, got)
        with pytest.raises(RuntimeError, match="batch_edges"):
            eng.contract()
        with pytest.raises(RuntimeError, match="batch_edges"):
            eng.contract_profiled()
        with pytest.raises(RuntimeError, match="batch_edges"):
            eng.contract_sliced()
    finally:
        eng.close()


def test_open_legs():
    from tnc_amd.executor import amplitudes_gpu

    strings = ["01*1101*0", "11*0001*1", "00*0000*0", "10*0101*1"]
    tn, permutor, beta = _circuit().into_amplitudes_network(strings)
    replace = _path(strings[0])
    legs, got = amplitudes_gpu(tn, replace, beta)
    assert legs[0] == beta and got.shape == (4, 2, 2)
    assert sorted(legs[1:]) == sorted(permutor.target_leg_order)
    ref = _oracle_rows(tn, replace, beta, 4, legs[1:])
    np.testing.assert_allclose(got, ref, **TOL["c128"])


def _four_leaf_network(dtype):
    """V[e4,k96] X[beta3,a32,e4] Y[beta3,k96,c48] Z[beta3,c48,a32]."""
    from tnc_amd.tensor import CompositeTensor, LeafTensor, TensorData

    beta, e, k, a, c = 50, 10, 11, 12, 13
    rng = np.random.default_rng(33)
    leaves, arrays = [], []
    for legs, dims in (([e, k], [4, 96]), ([beta, a, e], [3, 32, 4]),
                       ([beta, k, c], [3, 96, 48]), ([beta, c, a], [3, 48, 32])):
        data = rng.standard_normal(dims) + 1j * rng.standard_normal(dims)
        if dtype == "c64":
            data = data.astype(np.complex64).astype(np.complex128)
        leaf = LeafTensor(legs, dims)
        leaf.set_tensor_data(TensorData(TensorData.MATRIX, matrix=data))
        leaves.append(leaf)
        arrays.append(data)
    ref = np.einsum("ek,bae,bkc,bca->b", *arrays)
    return CompositeTensor(leaves), beta, ref


@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_four_leaves_none_gemm_loop(dtype):
    from tnc_amd import hiplib as H
    from tnc_amd.contraction_path import ContractionPath
    from tnc_amd.executor import ContractionEngine

    tn, beta, ref = _four_leaf_network(dtype)
    replace = ContractionPath.simple([(1, 0), (1, 2), (1, 3)])
    eng = ContractionEngine(tn, replace, dtype=dtype, batch_edges=[beta])
    try:
        assert eng.batch_classes == [H.BATCH_NONE, H.BATCH_GEMM, H.BATCH_LOOP]
        assert [(s.m, s.n, s.k) for s in eng.infos[1:]] == [(32, 48, 96),
                                                            (1, 1, 1536)]
        eng.contract_batched()
        legs, got = eng.result()
    finally:
        eng.close()
    assert legs == [beta] and got.shape == (3,)
    print(dtype, "max rel err", np.max(np.abs(got - ref) / np.abs(ref)))
    # |ref| ~ sqrt(4*96*32*48) * 2^2 ~ 3e3: the relative bound decides
    if dtype == "c128":
        np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12)
    else:
        np.testing.assert_allclose(got, ref, rtol=2e-3, atol=1e-4)


def test_alternating_with_plain_contract():
    """tn_net_contract (normal run, then captured and replayed) and
    tn_net_contract_batched with no batch label alternate on one net and
    agree bit for bit, the replayed graph included."""
    from tnc_amd import hiplib as H
    from tnc_amd.executor import ContractionEngine
    from tnc_amd.fixtures import load_fixture
    from tnc_amd.contraction_path import ContractionPath

    tn, replace_toplevel, _ = load_fixture("rqc24")
    eng = ContractionEngine(tn, ContractionPath.simple(replace_toplevel))
    L = H.lib()

    def batched():
        ms = ctypes.c_double()
        H.check(L.tn_net_contract_batched(
            eng.net, eng._pairs, len(eng.steps), H._u64arr([]), 0,
            ctypes.byref(ms)), "tn_net_contract_batched")
        legs, data = eng.result()
        return legs, np.array(data, copy=True)

    def plain():
        eng.contract()
        legs, data = eng.result()
        return legs, np.array(data, copy=True)

    try:
        # plain, batched, plain (captures), plain (replays), batched (the
        # graph's final block set aside), plain (replays), batched, batched
        order = [plain, batched, plain, plain, batched, plain, batched,
                 batched, plain]
        results = [f() for f in order]
    finally:
        eng.close()
    legs0, data0 = results[0]
    assert np.abs(data0) > 0
    for legs, data in results[1:]:
        assert legs == legs0
        assert np.array_equal(data, data0)


def test_python_refusals():
    from tnc_amd.contraction_path import ContractionPath
    from tnc_amd.executor import ContractionEngine

    tn, beta, _ = _four_leaf_network("c128")
    replace = ContractionPath.simple([(1, 0), (1, 2), (1, 3)])
    with pytest.raises(ValueError, match="slice_edges"):
        ContractionEngine(tn, replace, batch_edges=[beta], slice_edges=[11])
    with pytest.raises(ValueError, match="one character per qubit"):
        _circuit().into_amplitudes_network(["010110100", "0101"])
    with pytest.raises(ValueError, match="same positions"):
        _circuit().into_amplitudes_network(["01011010*", "0101101*0"])
    eng = ContractionEngine(tn, replace)
    try:
        with pytest.raises(RuntimeError, match="without batch_edges"):
            eng.contract_batched()
    finally:
        eng.close()
