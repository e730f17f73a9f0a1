"""Gauss three-multiply (3M) c128 GEMM: parity, error against the 4M path,
exact-zero imaginary part on real inputs, gate liveness, determinism.

TN_GEMM3M is read once at library load, so each mode ("force", "0",
unset) runs once in a subprocess over the same saved inputs; the tests
share those outputs and the host references.

Shapes are the smallest at which the kernel can go wrong: its tile is
128x64 with 16-deep K-tiles, so one tile / one K-tile, one tile / many
K-tiles, and 2x2 tiles with both packs and the unpack permute.
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
TM = 128  # row tile of k_zgemm_c128_glds_3m

CHILD = r"""
import json, sys
import numpy as np
from tnc_amd import hiplib
d = sys.argv[1]
spec = json.load(open(d + "/spec.json"))
inp = np.load(d + "/inputs.npz")
out = {}
for name, c in spec.items():
    a, b = inp[name + "_a"], inp[name + "_b"]
    out[name] = hiplib.einsum_c128(c["out"], c["a"], a, c["b"], b)
    if c.get("twice"):
        out[name + "_again"] = hiplib.einsum_c128(c["out"], c["a"], a,
                                                  c["b"], b)
np.savez(sys.argv[2], **out)
print("GEMM3M_CHILD_OK")
"""


def _cplx(rng, dims):
    return rng.standard_normal(dims) + 1j * rng.standard_normal(dims)


def _cases():
    rng = np.random.default_rng(33)
    cases = {}

    def add(name, out, a_legs, a, b_legs, b, **kw):
        cases[name] = dict(out=out, a=a_legs, b=b_legs, A=a, B=b, **kw)

    def plain(name, m, n, k, a=None, b=None, **kw):
        a = _cplx(rng, [m, k]) if a is None else a
        b = _cplx(rng, [k, n]) if b is None else b
        add(name, [1, 20], [1, 10], a, [10, 20], b, **kw)

    # one tile, one K-tile / many K-tiles
    plain("p_one", TM, 64, 16)
    plain("p_manyk", TM, 64, 512)
    # 2x2 tiles, K = 64: A's K legs interleaved, B N-first (both packs);
    # the out order interleaves M and N legs (unpack permute)
    a_legs, a_dims = [10, 1, 11, 2, 12], [4, 16, 4, 16, 4]
    b_legs, b_dims = [20, 21, 10, 11, 12], [8, 16, 4, 4, 4]
    add("p_2x2", [20, 1, 21, 2], a_legs, _cplx(rng, a_dims), b_legs,
        _cplx(rng, b_dims), twice=True)
    # qubit legs: all dims 2, same M = 256, N = 128, K = 64
    m_l, n_l, k_l = list(range(1, 9)), list(range(20, 27)), list(range(10, 16))
    qa = [int(x) for x in rng.permutation(m_l + k_l)]
    qb = [int(x) for x in rng.permutation(n_l + k_l)]
    qo = [int(x) for x in rng.permutation(m_l + n_l)]
    add("p_qubit", qo, qa, _cplx(rng, [2] * len(qa)), qb,
        _cplx(rng, [2] * len(qb)))
    # error against 4M: N(0,1), and one operand's imaginary part x1e3
    plain("e_n01", TM, 64, 512)
    a = _cplx(rng, [TM, 512])
    a = a.real + 1e3j * a.imag
    plain("e_skew", TM, 64, 512, a=a)
    # real-only inputs, one tile with split K and 2x2 tiles
    plain("r_one", TM, 64, 512, a=rng.standard_normal([TM, 512]) + 0j,
          b=rng.standard_normal([512, 64]) + 0j)
    plain("r_2x2", 2 * TM, 128, 64, a=rng.standard_normal([2 * TM, 64]) + 0j,
          b=rng.standard_normal([64, 128]) + 0j)
    # gate: 32 x 8 = 256 tiles, unsplit -> admitted; 2 tiles -> not
    plain("g_big", 4096, 512, 512)
    plain("g_small", 256, 64, 64)
    return cases


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gemm3m"))
    cases = _cases()
    spec = {n: {k: v for k, v in c.items() if k not in ("A", "B")}
            for n, c in cases.items()}
    with open(os.path.join(d, "spec.json"), "w") as f:
        json.dump(spec, f)
    arrs = {}
    for n, c in cases.items():
        arrs[n + "_a"], arrs[n + "_b"] = c["A"], c["B"]
    np.savez(os.path.join(d, "inputs.npz"), **arrs)
    outs = {}
    for mode in ("force", "0", None):
        env = dict(os.environ)
        env.pop("TN_GEMM3M", None)
        if mode is not None:
            env["TN_GEMM3M"] = mode
        dst = os.path.join(d, f"out_{mode}.npz")
        proc = subprocess.run([sys.executable, "-c", CHILD, d, dst], cwd=ROOT,
                              env=env, capture_output=True, text=True,
                              timeout=240)
        assert proc.returncode == 0, (proc.stdout, proc.stderr)
        assert "GEMM3M_CHILD_OK" in proc.stdout, (proc.stdout, proc.stderr)
        outs[mode] = dict(np.load(dst))
    return cases, outs


def _oracle(c):
    return oracle.contract_ndarrays(c["out"], c["a"], c["A"], c["b"], c["B"])


@pytest.mark.parametrize("name", ["p_one", "p_manyk", "p_2x2", "p_qubit"])
def test_forced_3m_parity(runs, name):
    """TN_GEMM3M=force reproduces the oracle at the suite's bars."""
    cases, outs = runs
    np.testing.assert_allclose(outs["force"][name], _oracle(cases[name]),
                               rtol=1e-11, atol=1e-10)


@pytest.mark.parametrize("name", ["e_n01", "e_skew"])
def test_3m_error_vs_4m(runs, name):
    """max|err_3M| <= 4 x max|err_4M| against a longdouble host reference
    (M = 128, N = 64, K = 512): Gauss's form measured 1.1-2.2x the 4M error
    in float64 emulation; the factor 4 leaves 2x for MFMA summation order."""
    cases, outs = runs
    c = cases[name]
    al, bl = c["A"].astype(np.clongdouble), c["B"].astype(np.clongdouble)
    ref = al @ bl
    e3 = float(np.max(np.abs(outs["force"][name] - ref)))
    e4 = float(np.max(np.abs(outs["0"][name] - ref)))
    print(f"{name}: max|err_3M| = {e3:.3e}  max|err_4M| = {e4:.3e}  "
          f"ratio = {e3 / e4:.2f}")
    assert e3 <= 4 * e4, (e3, e4)


@pytest.mark.parametrize("name", ["r_one", "r_2x2"])
def test_3m_real_inputs_exact_zero_imag(runs, name):
    """Real operands: P3 and P1 accumulate identically and P2 is 0, so the
    imaginary part is exactly 0.0."""
    cases, outs = runs
    got = outs["force"][name]
    assert np.all(got.imag == 0.0)
    np.testing.assert_allclose(got, _oracle(cases[name]), rtol=1e-11,
                               atol=1e-10)


def test_gate_is_live(runs):
    """A shape past the natural gate runs 3M by default (within the bar, not
    bit-equal to TN_GEMM3M=0, bit-equal to force); one below it keeps the 4M
    kernel bit for bit."""
    cases, outs = runs
    ref = _oracle(cases["g_big"])
    for mode in (None, "0"):
        np.testing.assert_allclose(outs[mode]["g_big"], ref, rtol=1e-11,
                                   atol=1e-10)
    assert not np.array_equal(outs[None]["g_big"], outs["0"]["g_big"])
    assert np.array_equal(outs[None]["g_big"], outs["force"]["g_big"])
    assert np.array_equal(outs[None]["g_small"], outs["0"]["g_small"])
    np.testing.assert_allclose(outs[None]["g_small"],
                               _oracle(cases["g_small"]), rtol=1e-11,
                               atol=1e-10)


def test_forced_3m_deterministic(runs):
    """Two runs under force are bit-identical."""
    _, outs = runs
    assert np.array_equal(outs["force"]["p_2x2"], outs["force"]["p_2x2_again"])
