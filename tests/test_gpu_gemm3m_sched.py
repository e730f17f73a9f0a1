"""The 3M GEMM's scheduled main loop with every CU holding two blocks.

The pipelined loop issues the DMAs of the next slab one by one among the
MFMAs of a half-step's first k-quad, behind that quad's fragment reads. What
moved DMAs (or a moved barrier, which the harness arms of
scripts/zgemm_tune.hip try) can newly get wrong is a matter of timing
between the blocks and waves of one CU:
a half overwritten while a slow wave still reads it, or read before it has
landed. The small cases of tests/test_gpu_gemm3m_pipe.py never fill a CU, so
these run 512 tiles (two blocks on each of 256 CUs) with full-entropy
operands, five launches of the same inputs per setting, each setting in a
child process (the switches are read once per process):

- 4096 x 1024 x 256: 16 K-tiles;
- 4096 x 1024 x 16: one K-tile, i.e. the prologue, the restaged last slab and
  the closing barrier with nothing in between;
- 2048 x 2048 x 48 through the scatter epilogue, whose tables are written
  over the staging array right after the loop, also against TN_EPI_SCATTER=0;
- split-K: plan_step splits only below 192 tiles and doubles the slice count
  until the grid reaches 256 blocks, so 127 tiles (16256 x 64) x 4 slices =
  508 blocks is the fullest split grid it plans; K = 272 gives slices of
  5, 5, 5 and 2 K-tiles, as the split case of the small tests does.

The loops add the same products in the same order per accumulator, so every
launch of the default must equal TN_GEMM3M_PIPE=0 bit for bit; one comparison
against numpy at the tolerances of the small tests guards both.
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
LAUNCHES = 5

CHILD = r"""
import json, sys
import numpy as np
from tnc_amd import hiplib
d, dst, names = sys.argv[1], sys.argv[2], sys.argv[3].split(",")
spec = json.load(open(d + "/spec.json"))
info = {}
for name in names:
    c = spec[name]
    a, b = np.load(d + "/" + name + "_a.npy"), np.load(d + "/" + name + "_b.npy")
    p = hiplib.plan_step(c["out"], c["out_shape"], c["a"], list(a.shape),
                         c["b"], list(b.shape))
    first, same = None, []
    for _ in range(int(sys.argv[4])):
        got = hiplib.einsum_c128(c["out"], c["a"], a, c["b"], b)
        if first is None:
            first = got
        else:
            same.append(bool(np.array_equal(got, first)))
    np.save(dst + "_" + name + ".npy", first)
    info[name] = {"plan": {f: getattr(p, f) for f, _ in p._fields_},
                  "same": same}
json.dump(info, open(dst + ".json", "w"))
print("SCHED_CHILD_OK")
"""

# 2048 x 2048 x 48 in legs: M and N are 11 legs of dim 2, K is 3 x 2^4; the
# out order interleaves M and N legs and keeps the three lowest N legs lowest
# (the run the scatter epilogue asks for)
M11 = list(range(1, 12))
K5 = list(range(20, 25))
N11 = list(range(30, 41))
SCATTER_OUT = M11[:6] + N11[:5] + M11[6:] + N11[5:]

MODES = {
    "serial": ({"TN_GEMM3M": "force", "TN_GEMM3M_PIPE": "0"},
               ["big", "k16", "scatter", "splitk"]),
    "pipe": ({"TN_GEMM3M": "force"}, ["big", "k16", "scatter", "splitk"]),
    "unpack": ({"TN_GEMM3M": "force", "TN_EPI_SCATTER": "0"}, ["scatter"]),
}


def _cplx(rng, dims):
    return rng.standard_normal(dims) + 1j * rng.standard_normal(dims)


def _cases():
    rng = np.random.default_rng(77)
    cases = {}

    def plain(name, m, n, k):
        cases[name] = dict(out=[1, 30], out_shape=[m, n], a=[1, 20],
                           b=[20, 30], A=_cplx(rng, [m, k]),
                           B=_cplx(rng, [k, n]), mnk=(m, n, k))

    plain("big", 4096, 1024, 256)
    plain("k16", 4096, 1024, 16)
    plain("splitk", 127 * TM, TN, 272)
    cases["scatter"] = dict(out=SCATTER_OUT, out_shape=[2] * 22,
                            a=M11 + K5, b=K5 + N11,
                            A=_cplx(rng, [2] * 11 + [3, 2, 2, 2, 2]),
                            B=_cplx(rng, [3, 2, 2, 2, 2] + [2] * 11),
                            mnk=(2048, 2048, 48))
    return cases


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gemm3m_sched"))
    cases = _cases()
    spec = {n: {k: c[k] for k in ("out", "out_shape", "a", "b")}
            for n, c in cases.items()}
    with open(os.path.join(d, "spec.json"), "w") as f:
        json.dump(spec, f)
    for n, c in cases.items():
        np.save(os.path.join(d, n + "_a.npy"), c["A"])
        np.save(os.path.join(d, n + "_b.npy"), c["B"])
    outs, info = {}, {}
    for mode, (extra, names) in MODES.items():
        env = dict(os.environ)
        for k in ("TN_GEMM3M", "TN_GEMM3M_PIPE", "TN_EPI_SCATTER"):
            env.pop(k, None)
        env.update(extra)
        dst = os.path.join(d, "out_" + mode)
        proc = subprocess.run(
            [sys.executable, "-c", CHILD, d, dst, ",".join(names),
             str(LAUNCHES)],
            cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
        assert proc.returncode == 0, (mode, proc.stdout, proc.stderr)
        assert "SCHED_CHILD_OK" in proc.stdout, (mode, proc.stdout,
                                                 proc.stderr)
        outs[mode] = {n: np.load(dst + "_" + n + ".npy") for n in names}
        info[mode] = json.load(open(dst + ".json"))
    return cases, outs, info


@pytest.fixture(scope="module")
def refs(runs):
    """numpy, as a matrix product: the legs of A and B are already in
    [M][K] / [K][N] order, only the output is permuted."""
    cases, _, _ = runs
    out = {}
    for n, c in cases.items():
        m, nn, k = c["mnk"]
        r = c["A"].reshape(m, k) @ c["B"].reshape(k, nn)
        if n == "scatter":
            mn = M11 + N11
            r = r.reshape([2] * 22).transpose([mn.index(l) for l in c["out"]])
        out[n] = r
    return out


@pytest.mark.parametrize("name", ["big", "k16", "scatter", "splitk"])
def test_every_launch_equals_the_serial_loop(runs, refs, name):
    from tnc_amd import hiplib as H

    cases, outs, info = runs
    m, n, _ = cases[name]["mnk"]
    for mode, pipe in (("pipe", 1), ("serial", 0)):
        p = info[mode][name]["plan"]
        assert p["kernel"] == H.GEMM_C128_3M, (mode, p)
        assert p["gemm_pipe"] == pipe, (mode, p)
        assert (p["row_tiles"], p["col_tiles"]) == (m // TM, n // TN), p
        # launches 2..5 of this setting gave the bits of its first
        assert info[mode][name]["same"] == [True] * (LAUNCHES - 1), mode
    got, serial = outs["pipe"][name], outs["serial"][name]
    print(f"{name}: max|pipe - serial| = "
          f"{float(np.max(np.abs(got - serial))):.3e}  max|pipe - numpy| = "
          f"{float(np.max(np.abs(got - refs[name]))):.3e}")
    assert np.array_equal(got, serial)
    np.testing.assert_allclose(got, refs[name], rtol=1e-11, atol=1e-10)


def test_grids_fill_every_cu_twice(runs):
    _, _, info = runs
    for mode in ("pipe", "serial"):
        for name in ("big", "k16", "scatter"):
            p = info[mode][name]["plan"]
            assert p["row_tiles"] * p["col_tiles"] == 512 and p["splitk"] == 1, p
        p = info[mode]["splitk"]["plan"]
        assert p["row_tiles"] * p["col_tiles"] == 127 and p["splitk"] == 4, p
        assert p["kchunk"] == 5 * KT, p


def test_scatter_tables_go_over_a_drained_staging_array(runs):
    """The scatter case takes the scatter epilogue in both loops and gives
    the bits of the unpack permute of TN_EPI_SCATTER=0."""
    _, outs, info = runs
    for mode in ("pipe", "serial"):
        p = info[mode]["scatter"]["plan"]
        assert (p["scatter_out"], p["kind"], p["direct"]) == (1, 2, 0), p
    p = info["unpack"]["scatter"]["plan"]
    assert (p["scatter_out"], p["kind"], p["gemm_pipe"]) == (0, 3, 1), p
    assert info["unpack"]["scatter"]["same"] == [True] * (LAUNCHES - 1)
    assert np.array_equal(outs["pipe"]["scatter"], outs["unpack"]["scatter"])
