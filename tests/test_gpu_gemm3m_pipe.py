"""Pipelined main loop of the c128 3M GEMM against its serial loop.

The pipelined loop (default) stages the next 8-deep K-slab into one half of
the LDS array while the MFMAs of the other half run; TN_GEMM3M_PIPE=0 selects
the serial loop from the same binary. Both add the same products in the same
order per accumulator, so every output must agree bit for bit.

The switches are read once per process: each setting runs once in a child
over the same saved inputs, and the tests share what the children wrote.

Shapes are the smallest at which the loop can go wrong (tile 128x64, K-tile
16 = two slabs): K = 16 (the prologue's slab pair is also the last), K = 32
and 48 (even / odd number of tiles after the first), 256x128x64 (tile origin),
one forced split-K case whose slices are an odd number of K-tiles, a 2x2-tile
case through the scatter epilogue (its tables are written over the staging
array: no DMA may still be in flight), and the smallest gated shape.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TM, TN, KT = 128, 64, 16

CHILD = r"""
import json, sys
import numpy as np
from tnc_amd import hiplib
d = sys.argv[1]
spec = json.load(open(d + "/spec.json"))
inp = np.load(d + "/inputs.npz")
out, plans = {}, {}
for name, c in spec.items():
    a, b = inp[name + "_a"], inp[name + "_b"]
    p = hiplib.plan_step(c["out"], c["out_shape"], c["a"], list(a.shape),
                         c["b"], list(b.shape))
    plans[name] = {f: getattr(p, f) for f, _ in p._fields_}
    if len(sys.argv) > 3 and name not in sys.argv[3].split(","):
        continue
    out[name] = hiplib.einsum_c128(c["out"], c["a"], a, c["b"], b)
np.savez(sys.argv[2] + ".npz", **out)
json.dump(plans, open(sys.argv[2] + ".json", "w"))
print("PIPE_CHILD_OK")
"""

# 2x2 tiles, M = 2^8, N = 2^7, K = 2^5 in legs of dim 2; the out order
# interleaves M and N legs and keeps the three lowest N legs lowest, as the
# "small" case of tests/test_gpu_epilogue_scatter.py does
M8 = list(range(1, 9))
K5 = list(range(10, 15))
N7 = list(range(20, 27))
SCATTER_OUT = M8[:5] + N7[:4] + M8[5:] + N7[4:]

MODES = {
    "pipe": {"TN_GEMM3M": "force"},
    "serial": {"TN_GEMM3M": "force", "TN_GEMM3M_PIPE": "0"},
    "unpack": {"TN_GEMM3M": "force", "TN_EPI_SCATTER": "0"},
    "default": {},
}


def _cplx(rng, dims):
    return rng.standard_normal(dims) + 1j * rng.standard_normal(dims)


def _cases():
    rng = np.random.default_rng(66)
    cases = {}

    def plain(name, m, n, k):
        cases[name] = dict(out=[1, 20], out_shape=[m, n], a=[1, 10],
                           b=[10, 20], A=_cplx(rng, [m, k]),
                           B=_cplx(rng, [k, n]))

    plain("k16", TM, TN, 16)
    plain("k32", TM, TN, 32)
    plain("k48", TM, TN, 48)
    plain("origin", 2 * TM, 2 * TN, 64)
    plain("splitk", TM, TN, 272)
    plain("gated", 4096, 512, 512)
    cases["scatter"] = dict(out=SCATTER_OUT, out_shape=[2] * len(SCATTER_OUT),
                            a=M8 + K5, b=K5 + N7, A=_cplx(rng, [2] * 13),
                            B=_cplx(rng, [2] * 12))
    return cases


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gemm3m_pipe"))
    cases = _cases()
    spec = {n: {k: v for k, v in c.items() if k not in ("A", "B")}
            for n, c in cases.items()}
    with open(os.path.join(d, "spec.json"), "w") as f:
        json.dump(spec, f)
    arrs = {}
    for n, c in cases.items():
        arrs[n + "_a"], arrs[n + "_b"] = c["A"], c["B"]
    np.savez(os.path.join(d, "inputs.npz"), **arrs)
    outs, plans = {}, {}
    for mode, extra in MODES.items():
        env = dict(os.environ)
        for k in ("TN_GEMM3M", "TN_GEMM3M_PIPE", "TN_EPI_SCATTER"):
            env.pop(k, None)
        env.update(extra)
        dst = os.path.join(d, "out_" + mode)
        args = [sys.executable, "-c", CHILD, d, dst]
        if mode == "unpack":
            args.append("scatter")
        elif mode == "default":
            args.append("gated")
        proc = subprocess.run(args, cwd=ROOT, env=env, capture_output=True,
                              text=True, timeout=240)
        assert proc.returncode == 0, (mode, proc.stdout, proc.stderr)
        assert "PIPE_CHILD_OK" in proc.stdout, (mode, proc.stdout, proc.stderr)
        outs[mode] = dict(np.load(dst + ".npz"))
        plans[mode] = json.load(open(dst + ".json"))
    return cases, outs, plans


def _numpy_ref(c):
    labels = {l: x for x, l in enumerate(sorted(set(c["a"] + c["b"])))}
    sub = lambda legs: [labels[l] for l in legs]  # noqa: E731
    return np.einsum(c["A"], sub(c["a"]), c["B"], sub(c["b"]), sub(c["out"]))


@pytest.fixture(scope="module")
def refs(runs):
    cases, _, _ = runs
    return {n: _numpy_ref(c) for n, c in cases.items()}


@pytest.mark.parametrize("name", ["k16", "k32", "k48", "origin", "splitk",
                                  "scatter", "gated"])
def test_pipe_equals_serial_bit_for_bit(runs, refs, name):
    from tnc_amd import hiplib as H

    _, outs, plans = runs
    for mode, pipe in (("pipe", 1), ("serial", 0)):
        p = plans[mode][name]
        assert p["kernel"] == H.GEMM_C128_3M, (mode, p)
        assert p["gemm_pipe"] == pipe, (mode, p)
    got, serial = outs["pipe"][name], outs["serial"][name]
    print(f"{name}: max|pipe - serial| = "
          f"{float(np.max(np.abs(got - serial))):.3e}  max|pipe - numpy| = "
          f"{float(np.max(np.abs(got - refs[name]))):.3e}")
    assert np.array_equal(got, serial)
    np.testing.assert_allclose(got, refs[name], rtol=1e-11, atol=1e-10)


def test_splitk_case_is_split_with_odd_tile_count(runs):
    _, _, plans = runs
    for mode in ("pipe", "serial"):
        p = plans[mode]["splitk"]
        assert p["splitk"] > 1, p
        assert p["kchunk"] % KT == 0 and (p["kchunk"] // KT) % 2 == 1, p


def test_scatter_case_takes_the_scatter_epilogue(runs):
    """The pipelined loop's closing barrier has drained every DMA before the
    scatter tables go over the staging array: same bits as the serial loop
    (above) and as the unpack permute of TN_EPI_SCATTER=0."""
    _, outs, plans = runs
    for mode in ("pipe", "serial"):
        p = plans[mode]["scatter"]
        assert (p["scatter_out"], p["kind"], p["direct"]) == (1, 2, 0), p
        assert (p["row_tiles"], p["col_tiles"]) == (2, 2), p
    p = plans["unpack"]["scatter"]
    assert (p["scatter_out"], p["kind"], p["gemm_pipe"]) == (0, 3, 1), p
    assert np.array_equal(outs["pipe"]["scatter"], outs["unpack"]["scatter"])


def test_pipelined_loop_is_the_default(runs):
    """With no switch set a shape past the 3M gate runs the pipelined loop,
    and gives the bits of the forced run; below the gate nothing changes."""
    from tnc_amd import hiplib as H

    _, outs, plans = runs
    p = plans["default"]["gated"]
    assert p["kernel"] == H.GEMM_C128_3M and p["gemm_pipe"] == 1, p
    assert np.array_equal(outs["default"]["gated"], outs["pipe"]["gated"])
    p = plans["default"]["k16"]
    assert p["kernel"] != H.GEMM_C128_3M and p["gemm_pipe"] == 0, p
