"""Sampling, the parts that need no GPU: the exported plan (tn_plan_sample)
against the numbers tests/native/sample_plan_check.cpp checks in C++, and the
pure-numpy decode of drawn indices into digits and bitstrings."""

import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tnc_amd", "libtnc_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB),
                               reason="library not built")


@needs_lib
@pytest.mark.parametrize("dtype", ["c128", "c64"])
@pytest.mark.parametrize("n,nchunks", [(1, 1), (4095, 1), (4096, 1),
                                       (4097, 2), (1 << 34, 1 << 22)])
def test_plan_sample(n, nchunks, dtype):
    from tnc_amd import hiplib as H

    for nshots in (0, 1, 1000, 10 ** 6):
        p = H.plan_sample(n, nshots, dtype)
        assert p.chunk == 4096
        assert p.nchunks == nchunks
        assert (p.grid_sums, p.grid_scan, p.grid_draw) == (nchunks, 1, nshots)
        # C, the uniforms, the indices, total
        assert p.ws_bytes == 8 * nchunks + 8 * nshots + 8 * nshots + 8


@needs_lib
def test_plan_sample_refusals():
    from tnc_amd import hiplib as H

    def refused(*args):
        with pytest.raises(RuntimeError, match="rc=1"):
            H.plan_sample(*args)
        return H.last_error()

    assert refused(0, 5) == "tensor has no elements"
    assert (refused(4096, 1 << 31)
            == "more chunks or shots than one grid holds")
    assert (refused((1 << 31) * 4096, 1, "c64")
            == "more chunks or shots than one grid holds")


def test_decode_digits():
    from tnc_amd.executor import decode_digits

    dims = [3, 2, 5]
    idx = np.array([0, 1, 4, 5, 29, 17], dtype=np.uint64)
    digits = decode_digits(idx, dims)
    assert digits.shape == (6, 3) and digits.dtype == np.int64
    assert digits.tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 4], [0, 1, 0],
                               [2, 1, 4], [1, 1, 2]]
    assert np.array_equal(
        digits, np.stack(np.unravel_index(idx.astype(np.int64), dims), 1))
    # a scalar has no digits; no shots, no rows
    assert decode_digits(np.zeros(4, np.uint64), []).shape == (4, 0)
    assert decode_digits(np.zeros(0, np.uint64), dims).shape == (0, 3)
    with pytest.raises(ValueError, match="beyond"):
        decode_digits([30], dims)
    # a flat index beyond 2^32
    big = decode_digits([(1 << 33) + 5], [1 << 20, 1 << 14])
    assert big.tolist() == [[1 << 19, 5]]


def test_decode_statevector():
    from tnc_amd.executor import decode_bitstrings, decode_digits

    # stored legs [7, 3, 5]; qubits 0, 1, 2 end on edges 3, 5, 7
    legs, target = [7, 3, 5], [3, 5, 7]
    digits = decode_digits([0b100, 0b011, 0b110], [2, 2, 2])
    # digit on leg 7 is qubit 2's bit
    assert decode_bitstrings(legs, digits, target) == ["001", "110", "101"]
    assert (decode_bitstrings(legs, digits, target, bitstrings=["***"])
            == ["001", "110", "101"])
    assert decode_bitstrings([], np.zeros((2, 0), np.int64), []) == ["", ""]


def test_decode_batched_block():
    """A [B, 2, 2] result of into_amplitudes_network: the row picks the
    closed bits, the open digits fill the '*' positions in qubit order."""
    from tnc_amd.executor import decode_bitstrings, decode_digits

    beta = 40
    strings = ["0*1*0", "1*1*1", "0*0*1"]
    # qubit 1 ends on edge 21, qubit 3 on edge 17; stored order [beta, 17, 21]
    legs, target = [beta, 17, 21], [21, 17]
    idx = [0b000, 0b001, 0b110, 0b1011, 0b1001]  # rows 0, 0, 1, 2, 2
    digits = decode_digits(idx, [3, 2, 2])
    got = decode_bitstrings(legs, digits, target, beta, strings)
    #   row 0, leg17=0, leg21=0 -> q1=0, q3=0
    #   row 0, leg17=0, leg21=1 -> q1=1, q3=0
    #   row 1, leg17=1, leg21=0 -> q1=0, q3=1
    #   row 2, leg17=1, leg21=1 ; row 2, leg17=0, leg21=1
    assert got == ["00100", "01100", "10111", "01011", "01001"]
    # the batch edge stored last
    order = [1, 2, 0]
    got = decode_bitstrings([legs[x] for x in order], digits[:, order],
                            target, beta, strings)
    assert got == ["00100", "01100", "10111", "01011", "01001"]
    # without the strings: the open qubits only
    assert (decode_bitstrings(legs, digits, target, beta)
            == ["00", "10", "01", "11", "10"])
    # every string alike on the closed qubits: no batch leg, row 0
    assert (decode_bitstrings([17, 21], digits[:, 1:], target, beta,
                              ["0*1*0", "0*1*0"])
            == ["00100", "01100", "00110", "01110", "01100"])


def test_decode_refusals():
    from tnc_amd.executor import decode_bitstrings

    digits = np.zeros((1, 2), np.int64)
    with pytest.raises(ValueError, match="neither"):
        decode_bitstrings([1, 2], digits, [1])
    with pytest.raises(ValueError, match="no leg"):
        decode_bitstrings([1, 2], digits, [1, 2, 3])
    with pytest.raises(ValueError, match="one '\\*' per open edge"):
        decode_bitstrings([1, 2], digits, [1, 2], bitstrings=["0*"])
    with pytest.raises(ValueError, match="nshots"):
        decode_bitstrings([1, 2], np.zeros((1, 3), np.int64), [1, 2])
    with pytest.raises(ValueError, match="row beyond"):
        decode_bitstrings([9, 1], np.array([[2, 0]]), [1], 9, ["*0", "*1"])
