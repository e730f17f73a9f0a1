"""Sampling on the device (tn_sample_*_dev, tn_net_sample,
ContractionEngine.sample, sample_bitstrings_gpu): indices drawn with
probability |amplitude|^2 from uniforms the test supplies.

The kernel-level tests hand torch device tensors to tn_sample_*_dev. Where
every partial sum is an integer below 2^53 the order of the adds cannot
matter and the drawn index must EQUAL numpy's searchsorted over the
cumulative sum; on Gaussian tensors every drawn index must bracket u * total
within a tolerance derived below."""

import ctypes
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CH = 4096
NPDT = {"c128": np.complex128, "c64": np.complex64}
EXACT_SIZES = [1, 63, 4096, 4097, 3 * 4096 + 5, (1 << 20) + 3, (1 << 23) + 5]
TOL_SIZES = EXACT_SIZES[:-1]
NSHOTS = 4096


@pytest.fixture(scope="module")
def torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def dev_sample(torch, amps, u, dtype):
    """tn_sample_<dtype>_dev on torch-held device memory. amps: complex host
    array of NPDT[dtype]. Returns (idx uint64[nshots], norm2)."""
    from tnc_amd import hiplib as H

    n = amps.size
    real = np.float64 if dtype == "c128" else np.float32
    # (copies: the cached cases are read-only)
    host = np.array(amps).view(real).reshape(n, 2)
    data = torch.from_numpy(host).to("cuda:0")
    u_dev = torch.from_numpy(np.array(u, dtype=np.float64)).to("cuda:0")
    nshots = u_dev.numel()
    idx = torch.full((max(nshots, 1),), -1, dtype=torch.int64, device="cuda:0")
    norm2 = torch.full((1,), -1.0, dtype=torch.float64, device="cuda:0")
    plan = H.plan_sample(n, nshots, dtype)
    assert plan.nchunks == (n + CH - 1) // CH
    ws = torch.empty(plan.ws_bytes, dtype=torch.uint8, device="cuda:0")
    fn = getattr(H.lib(), "tn_sample_%s_dev" % dtype)
    H.check(fn(data.data_ptr(), n, u_dev.data_ptr(), nshots, idx.data_ptr(),
               norm2.data_ptr(), ws.data_ptr(), plan.ws_bytes,
               torch.cuda.current_stream().cuda_stream),
            "tn_sample_%s_dev" % dtype)
    torch.cuda.synchronize()
    return (idx[:nshots].cpu().numpy().astype(np.uint64),
            float(norm2.cpu()[0]))


# ---- exact: integer masses, any summation order ---------------------------

_exact_cache = {}


def exact_case(n):
    """Integer amplitudes in 0..7, about a third of the elements zero; the
    uniforms; the reference indices. Computed once per size, never changed."""
    if n in _exact_cache:
        return _exact_cache[n]
    rng = np.random.default_rng(1000 + n)
    parts = rng.integers(0, 8, size=(n, 2))
    parts[rng.random(n) < 1 / 3] = 0
    if not parts.any():
        parts[0] = (1, 2)
    p = (parts[:, 0] ** 2 + parts[:, 1] ** 2).astype(np.int64)
    cum = np.cumsum(p)
    total = int(cum[-1])
    assert 0 < total < 2 ** 53
    cumf = cum.astype(np.float64)
    u = rng.random(NSHOTS)
    u[0] = 0.0
    u[1] = 1.0 - 2.0 ** -53
    # elements i whose cumulative sum some u reproduces exactly: the draw
    # must land strictly after i
    hits = []
    inner = np.flatnonzero(cum < total)
    for i in (rng.choice(inner, size=min(64, inner.size), replace=False)
              if inner.size else []):
        cand = cumf[i] / float(total)
        for v in (cand, np.nextafter(cand, 0.0), np.nextafter(cand, 1.0)):
            if 0.0 <= v < 1.0 and v * float(total) == cumf[i]:
                u[2 + len(hits)] = v
                hits.append(int(i))
                break
    t = u * float(total)
    ref = np.searchsorted(cumf, t, side="right")
    # u * total rounding up to total: the clamp, the last element with mass
    ref[ref == n] = np.flatnonzero(p)[-1]
    case = dict(amps=parts[:, 0] + 1j * parts[:, 1], p=p, cum=cum,
                total=total, u=u, ref=ref.astype(np.uint64), hits=hits)
    for a in (case["amps"], p, cum, u, case["ref"]):
        a.setflags(write=False)
    _exact_cache[n] = case
    return case


@pytest.mark.parametrize("dtype", ["c128", "c64"])
@pytest.mark.parametrize("n", EXACT_SIZES)
def test_exact_integer_masses(torch, n, dtype):
    case = exact_case(n)
    if n >= 4096:
        assert len(case["hits"]) >= 8
    idx, norm2 = dev_sample(torch, case["amps"].astype(NPDT[dtype]),
                            case["u"], dtype)
    assert norm2 == float(case["total"])
    wrong = np.flatnonzero(idx != case["ref"])
    print(dtype, n, "shots", idx.size, "boundary hits", len(case["hits"]),
          "mismatches", wrong.size)
    assert wrong.size == 0, (wrong[:5], idx[wrong[:5]], case["ref"][wrong[:5]])
    assert np.all(case["p"][idx.astype(np.int64)] > 0)
    for k, i in enumerate(case["hits"]):
        assert idx[2 + k] > i
    # u = 0 skips the leading zeros; u next to 1 ends on the last mass
    assert idx[0] == np.flatnonzero(case["p"])[0]
    assert idx[1] == np.flatnonzero(case["p"])[-1]


# ---- tolerance: Gaussian amplitudes ----------------------------------------

def check_brackets(amps, idx, u, norm2):
    """Every drawn i has p[i] > 0 and cdf[i-1] - tol <= u * total <= cdf[i]
    + tol, cdf in long double. tol = (n + 4) * 2^-52 * total: at most 3
    roundings per p[i] and n - 1 per sum of non-negative terms at unit
    roundoff 2^-53, doubled to cover the product u * total and the
    reference's own rounding."""
    amps = np.asarray(amps).ravel()
    n = amps.size
    assert idx.shape == u.shape  # no shot left out
    p = amps.real.astype(np.float64) ** 2 + amps.imag.astype(np.float64) ** 2
    cdf = np.cumsum(p.astype(np.longdouble))
    total = cdf[-1]
    tol = (n + 4) * np.longdouble(2.0) ** -52 * total
    assert abs(np.longdouble(norm2) - total) <= tol
    i = idx.astype(np.int64)
    assert np.all((0 <= i) & (i < n))
    assert np.all(p[i] > 0)
    t = u.astype(np.longdouble) * total
    below = np.where(i > 0, cdf[np.maximum(i - 1, 0)], np.longdouble(0))
    slack = np.maximum(below - t, t - cdf[i])
    print("n", n, "shots", idx.size, "worst excess / tol",
          float(slack.max() / tol))
    assert np.all(below - tol <= t)
    assert np.all(t <= cdf[i] + tol)


_gauss_cache = {}


def gauss_case(n, dtype):
    if (n, dtype) not in _gauss_cache:
        rng = np.random.default_rng(2000 + n)
        amps = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(
            NPDT[dtype])
        u = rng.random(NSHOTS)
        u[0] = 0.0
        u[1] = 1.0 - 2.0 ** -53
        amps.setflags(write=False)
        u.setflags(write=False)
        _gauss_cache[(n, dtype)] = (amps, u)
    return _gauss_cache[(n, dtype)]


@pytest.mark.parametrize("dtype", ["c128", "c64"])
@pytest.mark.parametrize("n", TOL_SIZES)
def test_gaussian_brackets(torch, n, dtype):
    amps, u = gauss_case(n, dtype)
    idx, norm2 = dev_sample(torch, amps, u, dtype)
    check_brackets(amps, idx, u, norm2)


@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_reproducible(torch, dtype):
    amps, u = gauss_case((1 << 20) + 3, dtype)
    first = dev_sample(torch, amps, u, dtype)
    second = dev_sample(torch, amps, u, dtype)
    assert np.array_equal(first[0], second[0])
    assert first[1] == second[1]


# ---- support: four elements carry all the mass -----------------------------

@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_support_exact_counts(torch, dtype):
    n = 2 * CH + 7
    amps = np.zeros(n, dtype=NPDT[dtype])
    support = [0, CH - 1, CH, n - 1]
    amps[support] = [0.5, 0.5, 0.25 + 0.25j, 0.25 + 0.25j]
    mass = [Fraction(1, 4), Fraction(1, 4), Fraction(1, 8), Fraction(1, 8)]
    total = sum(mass)
    shots = 1024
    u = (np.arange(shots) + 0.5) / shots
    want = {s: 0 for s in support}
    for k in range(shots):
        t = Fraction(2 * k + 1, 2 * shots) * total
        run = Fraction(0)
        for s, m in zip(support, mass):
            run += m
            if run > t:
                want[s] += 1
                break
    assert sum(want.values()) == shots
    idx, norm2 = dev_sample(torch, amps, u, dtype)
    assert norm2 == float(total)
    got = {s: int(np.sum(idx == s)) for s in support}
    print(dtype, "counts", got)
    assert got == want
    assert set(idx.tolist()) <= set(support)


def test_dev_refusals(torch):
    from tnc_amd import hiplib as H

    L = H.lib()
    data = torch.zeros((CH + 1, 2), dtype=torch.float64, device="cuda:0")
    out = torch.zeros(4, dtype=torch.float64, device="cuda:0")
    # two chunks need 16 bytes of workspace
    rc = L.tn_sample_c128_dev(data.data_ptr(), CH + 1, None, 0, None,
                              out.data_ptr(), out.data_ptr() + 8, 8, None)
    assert rc == 1 and "workspace of 8 bytes, 16 needed" in H.last_error()
    rc = L.tn_sample_c128_dev(data.data_ptr() + 8, CH, None, 0, None,
                              out.data_ptr(), out.data_ptr() + 8, 16, None)
    assert rc == 1 and "16-byte aligned" in H.last_error()
    rc = L.tn_sample_c64_dev(data.data_ptr(), 0, None, 0, None,
                             out.data_ptr(), out.data_ptr() + 8, 16, None)
    assert rc == 1 and H.last_error() == "tensor has no elements"
    # nshots == 0: the norm only
    idx, norm2 = dev_sample(torch, np.full(CH + 1, 2 + 1j), np.zeros(0),
                            "c128")
    assert idx.size == 0 and norm2 == 5.0 * (CH + 1)


# ---- engine level ----------------------------------------------------------

def ghz():
    from tnc_amd import Circuit, TensorData

    c = Circuit()
    q = list(c.allocate_register(3).qubits())
    c.append_gate(TensorData.from_gate("h"), [q[0]])
    c.append_gate(TensorData.from_gate("cx"), [q[0], q[1]])
    c.append_gate(TensorData.from_gate("cx"), [q[1], q[2]])
    return c


def greedy(tn):
    from tnc_amd import Greedy

    return Greedy().find_path(tn).replace_path()


def test_ghz_statevector():
    from tnc_amd.executor import ContractionEngine, decode_bitstrings

    tn, permutor = ghz().into_statevector_network()
    eng = ContractionEngine(tn, greedy(tn))
    try:
        with pytest.raises(RuntimeError, match="no final tensor"):
            eng.sample([0.5])
        assert eng.sample_norm2 is None
        eng.contract()
        u = np.concatenate([[0.25, 0.75, 0.0, 1.0 - 2.0 ** -53],
                            np.random.default_rng(5).random(252)])
        legs, digits = eng.sample(u)
        assert sorted(legs) == sorted(permutor.target_leg_order)
        assert digits.shape == (256, 3)
        assert abs(eng.sample_norm2 - 1.0) < 1e-14
        strings = decode_bitstrings(legs, digits, permutor.target_leg_order)
        assert strings[:4] == ["000", "111", "000", "111"]
        assert set(strings) == {"000", "111"}
        assert strings == ["000" if x < 0.5 else "111" for x in u]
        # refusals leave the engine usable
        for bad in (1.0, -1e-300, float("nan")):
            with pytest.raises(RuntimeError, match=r"u\[1\] = .* outside"):
                eng.sample([0.5, bad])
        # no shots: the norm only
        eng.sample_norm2 = None
        legs0, digits0 = eng.sample([])
        assert legs0 == legs and digits0.shape == (0, 3)
        assert abs(eng.sample_norm2 - 1.0) < 1e-14
    finally:
        eng.close()


def test_zero_tensor_refused():
    from tnc_amd.executor import ContractionEngine

    # GHZ has no amplitude on 0*1
    tn, _ = ghz().into_amplitude_network("0*1")
    eng = ContractionEngine(tn, greedy(tn))
    try:
        eng.contract()
        assert not np.any(eng.result()[1])
        with pytest.raises(RuntimeError, match="final tensor has zero norm"):
            eng.sample([0.5])
        with pytest.raises(RuntimeError, match="final tensor has zero norm"):
            eng.sample([])
    finally:
        eng.close()


def test_ghz_bitstrings_from_seed():
    from tnc_amd.executor import sample_bitstrings_gpu

    tn, permutor = ghz().into_statevector_network()
    shots = sample_bitstrings_gpu(tn, greedy(tn), permutor, 64, seed=3)
    u = np.random.default_rng(3).random(64)
    assert shots == ["000" if x < 0.5 else "111" for x in u]
    # the README's example
    assert (sample_bitstrings_gpu(tn, greedy(tn), permutor, shots=4, seed=0)
            == ["111", "000", "000", "000"])
    # one qubit closed on 1: only 111 is left, the template fills the rest
    tn, permutor = ghz().into_amplitude_network("*1*")
    shots = sample_bitstrings_gpu(tn, greedy(tn), permutor, 8,
                                  bitstrings=["*1*"])
    assert shots == ["111"] * 8


STRINGS = ["01*11*1*0", "11*00*1*1", "00*00*0*0", "01*11*1*0", "10*01*0*1"]


def sycamore():
    from tnc_amd.builders import sycamore_circuit

    return sycamore_circuit(9, 4, 7)


@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_sycamore_statevector(dtype):
    from tnc_amd.executor import ContractionEngine

    tn, _ = sycamore().into_statevector_network()
    eng = ContractionEngine(tn, greedy(tn), dtype=dtype)
    try:
        eng.contract()
        u = np.random.default_rng(11).random(512)
        idx = eng.sample_flat(u)
        legs, amps = eng.result()
        assert amps.size == 512
        check_brackets(amps, idx, u, eng.sample_norm2)
        legs2, digits = eng.sample(u)
        assert legs2 == legs
        assert np.array_equal(np.ravel_multi_index(tuple(digits.T), amps.shape),
                              idx.astype(np.int64))
    finally:
        eng.close()


def test_sycamore_amplitudes_block():
    from tnc_amd.executor import (ContractionEngine, decode_bitstrings,
                                  sample_bitstrings_gpu)

    tn, permutor, beta = sycamore().into_amplitudes_network(STRINGS)
    single, _ = sycamore().into_amplitude_network(STRINGS[0])
    replace = greedy(single)
    seed, shots = 17, 400
    u = np.random.default_rng(seed).random(shots)
    eng = ContractionEngine(tn, replace, batch_edges=[beta])
    try:
        eng.contract_batched()
        idx = eng.sample_flat(u)
        legs, amps = eng.result()
        assert amps.size == 5 * 8 and beta in legs
        check_brackets(amps, idx, u, eng.sample_norm2)
        legs, digits = eng.sample(u)
    finally:
        eng.close()
    rows = digits[:, legs.index(beta)]
    assert len(set(rows.tolist())) > 1
    want = decode_bitstrings(legs, digits, permutor.target_leg_order, beta,
                             STRINGS)
    tn, permutor, beta = sycamore().into_amplitudes_network(STRINGS)
    got = sample_bitstrings_gpu(tn, replace, permutor, shots, seed=seed,
                                batch_edge=beta, bitstrings=STRINGS)
    assert got == want
    for s, r in zip(got, rows):
        assert len(s) == 9 and set(s) <= {"0", "1"}
        # closed positions: the drawn row of STRINGS
        assert all(c == "*" or c == b for b, c in zip(s, STRINGS[r]))


def test_sliced_result_mixed_radix():
    """contract_sliced()'s final tensor samples like any other; dims 3, 7, 5
    go through the mixed-radix decode."""
    from tnc_amd.contraction_path import ContractionPath
    from tnc_amd.executor import ContractionEngine
    from tnc_amd.tensor import CompositeTensor, LeafTensor, TensorData

    i, s, k, t, j, l = 1, 2, 3, 4, 5, 6
    rng = np.random.default_rng(20)
    leaves = []
    for legs, dims in (([i, s, k], [3, 3, 5]), ([k, t, j], [5, 2, 7]),
                       ([s, t, l], [3, 2, 5])):
        leaf = LeafTensor(legs, dims)
        leaf.set_tensor_data(TensorData(
            TensorData.MATRIX,
            matrix=rng.standard_normal(dims) + 1j * rng.standard_normal(dims)))
        leaves.append(leaf)
    eng = ContractionEngine(CompositeTensor(leaves),
                            ContractionPath.simple([(0, 1), (0, 2)]),
                            slice_edges=[s, t])
    try:
        eng.contract_sliced()
        u = np.random.default_rng(21).random(300)
        legs, digits = eng.sample(u)
        _, amps = eng.result()
        assert legs == [i, j, l] and amps.shape == (3, 7, 5)
        assert np.all(digits.max(axis=0) == [2, 6, 4])
        idx = np.ravel_multi_index(tuple(digits.T), amps.shape)
        check_brackets(amps, idx.astype(np.uint64), u, eng.sample_norm2)
    finally:
        eng.close()


def test_alongside_graph_replay():
    """contract x3 (normal, captured, replayed), sample, contract, sample on
    the rqc24 engine: the sampling workspace comes from the arena and goes
    back, so the replayed graph and its result are untouched."""
    from tnc_amd import hiplib as H
    from tnc_amd.contraction_path import ContractionPath
    from tnc_amd.executor import ContractionEngine
    from tnc_amd.fixtures import load_fixture

    tn, replace_toplevel, _ = load_fixture("rqc24")
    eng = ContractionEngine(tn, ContractionPath.simple(replace_toplevel))

    def in_use():
        used, cached = ctypes.c_uint64(), ctypes.c_uint64()
        H.check(H.lib().tn_net_pool_bytes(
            eng.net, ctypes.byref(used), ctypes.byref(cached)), "pool_bytes")
        assert cached.value >= 256 * 1024 * 1024  # an arena: replay engages
        return used.value

    def contract():
        eng.contract()
        return np.array(eng.result()[1], copy=True)

    u = np.random.default_rng(9).random(1000)
    try:
        results = [contract(), contract(), contract()]
        before = in_use()
        first = eng.sample_flat(u)
        norm_first = eng.sample_norm2
        assert in_use() == before
        results.append(contract())
        assert in_use() == before
        second = eng.sample_flat(u)
        assert in_use() == before
        results.append(contract())
    finally:
        eng.close()
    assert np.abs(results[0]) > 0
    for r in results[1:]:
        assert np.array_equal(r, results[0])
    # one amplitude: every shot draws it
    assert first.shape == (1000,) and not first.any()
    assert np.array_equal(first, second)
    assert norm_first == eng.sample_norm2
    amp = complex(results[0])
    assert norm_first == amp.real * amp.real + amp.imag * amp.imag
