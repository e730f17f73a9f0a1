"""The layout pre-pass (tn_plan_layouts) and the scatter-epilogue gate of
tn_plan_step, checked without a GPU.

The pre-pass decides the order every step of a path stores its output in. On
the rqc36 fixture the inline packs it is there to remove are the ones of
steps 436-439, each packing the output of the step before it. The byte
figures below are those operands' sizes, M x K x 16 B, from the fixture's
shapes:

    436: 2^21 x 2^10    437: 2^14 x 2^15    438: 2^15 x 2^11    439: 2^17 x 2^11

and 50.6 GB for all inline packs of the contraction together.

TN_EPI_SCATTER is read once per process, so every setting runs in a child.
"""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tnc_amd", "libtnc_hip.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB),
                                reason="library not built")

CHAIN = (436, 437, 438, 439)
CHAIN_BYTES = {436: 2 ** 31 * 16, 437: 2 ** 29 * 16, 438: 2 ** 26 * 16,
               439: 2 ** 28 * 16}

LAYOUT_CHILD = r"""
import json, sys
from tnc_amd import hiplib
from tnc_amd.contraction_path import ContractionPath, flatten_network
from tnc_amd.fixtures import load_fixture
fixture, dtype = sys.argv[1:3] if len(sys.argv) > 2 else ("rqc36", "c128")
tn, replace_toplevel, _ = load_fixture(fixture)
leaves, steps, _ = flatten_network(tn, ContractionPath.simple(replace_toplevel))
scatter, inline = hiplib.plan_layouts(
    [(t.legs, t.bond_dims) for t in leaves], steps, dtype=dtype)
print("LAYOUT " + json.dumps({"scatter": scatter, "inline": inline}))
"""

# sum(inline_pack_bytes) of the frozen paths, as planned before the look-ahead
# rule moved into the pre-pass: (fixture, dtype, TN_EPI_SCATTER) -> bytes
INLINE_PINS = [
    ("rqc36", "c128", None, 1_480_720_384),
    ("rqc36", "c128", "0", 50_604_408_832),
    ("syc49", "c64", None, 103_079_215_104),
    ("rqc24", "c128", None, 0),
]

PLAN_CHILD = r"""
import json, sys
from tnc_amd import hiplib
out = []
for args in json.loads(sys.argv[1]):
    p = hiplib.plan_step(*args, has_stream2=True)
    out.append({f: getattr(p, f) for f, _ in p._fields_})
print("PLANS " + json.dumps(out))
"""


def run_child(code, tag, env_extra, *argv):
    env = {k: v for k, v in os.environ.items()
           if k not in ("TN_NO_PIPELINE", "TN_PIPELINE_FORCE",
                        "TN_GATHER_GEMM", "TN_GEMM3M", "TN_EPI_SCATTER")}
    env.update(env_extra)
    proc = subprocess.run([sys.executable, "-c", code, *argv], cwd=ROOT,
                          env=env, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, (proc.stdout, proc.stderr)
    line = [l for l in proc.stdout.splitlines() if l.startswith(tag + " ")][-1]
    return json.loads(line[len(tag) + 1:])


@pytest.fixture(scope="module")
def layout_off():
    return run_child(LAYOUT_CHILD, "LAYOUT", {"TN_EPI_SCATTER": "0"})


@pytest.fixture(scope="module")
def layout_on():
    return run_child(LAYOUT_CHILD, "LAYOUT", {})


def test_switched_off_packs_match_the_trace(layout_off):
    inline, scatter = layout_off["inline"], layout_off["scatter"]
    assert len(inline) == 720 and not any(scatter)
    for s in CHAIN:
        assert inline[s] == CHAIN_BYTES[s], (s, inline[s])
    total = sum(inline)
    print("inline pack bytes, switched off:", total)
    # 50.6 GB of operands = 101.2 GB of pack traffic, to the table's digit
    assert abs(total - 50.6e9) < 0.05e9


def test_chain_packs_nothing_inline(layout_on):
    inline, scatter = layout_on["inline"], layout_on["scatter"]
    for s in CHAIN:
        assert inline[s] == 0, (s, inline[s])
        assert scatter[s - 1] == 1, s - 1


def test_inline_packs_fall_below_five_percent(layout_on, layout_off):
    on, off = sum(layout_on["inline"]), sum(layout_off["inline"])
    print("inline pack bytes: on", on, "off", off)
    assert on < 0.05 * off


@pytest.mark.parametrize("fixture,dtype,scatter_env,total", INLINE_PINS)
def test_inline_pack_totals_are_pinned(fixture, dtype, scatter_env, total):
    env = {} if scatter_env is None else {"TN_EPI_SCATTER": scatter_env}
    got = run_child(LAYOUT_CHILD, "LAYOUT", env, fixture, dtype)
    assert sum(got["inline"]) == total


# ---- plan_step route table: the scatter gate ------------------------------
# base shape M = 2^11, N = 2^10, K = 2^5, all legs of dim 2: 256 tiles, the
# smallest gated 3M shape. Labels: M legs 100.., N legs 200.., K legs 300..

def legs(base, count):
    return [base + x for x in range(count)]


def case(out, m_legs, n_legs, k_legs, dims=None):
    dims = dims or {}
    d = lambda ls: [dims.get(l, 2) for l in ls]  # noqa: E731
    a, b = m_legs + k_legs, k_legs + n_legs
    return [out, d(out), a, d(a), b, d(b)]


M11, N10, K5 = legs(100, 11), legs(200, 10), legs(300, 5)
# M and N legs interleaved, the three lowest N legs lowest
INTERLEAVED = M11[:6] + N10[:4] + M11[6:10] + N10[4:7] + [M11[10]] + N10[7:]
# only the two lowest N legs stay lowest: an M leg sits above them
RUN2 = M11[:6] + N10[:4] + M11[6:10] + N10[4:8] + [M11[10]] + N10[8:]
M_LOWEST = N10[:5] + M11[:10] + N10[5:] + [M11[10]]
# N legs 208, 209 merged into one dim-4 leg (label 208); same for a dim-3
MERGED_N = N10[:9]
MERGED_OUT = M11[:6] + N10[:4] + M11[6:] + N10[4:9]

ROUTE_CASES = {
    "interleaved": case(INTERLEAVED, M11, N10, K5),
    "run2": case(RUN2, M11, N10, K5),
    "m_lowest": case(M_LOWEST, M11, N10, K5),
    "dim4": case(MERGED_OUT, M11, MERGED_N, K5, {208: 4}),
    "dim3": case(MERGED_OUT, M11, MERGED_N, K5, {208: 3}),
    "k16": case(INTERLEAVED, M11, N10, K5[:4]),
    "tiles128": case([l for l in INTERLEAVED if l != M11[0]], M11[1:], N10,
                     K5),
}


@pytest.fixture(scope="module")
def routes_on():
    names = list(ROUTE_CASES)
    plans = run_child(PLAN_CHILD, "PLANS", {},
                      json.dumps([ROUTE_CASES[n] for n in names]))
    return dict(zip(names, plans))


@pytest.mark.parametrize("name", ["interleaved", "dim4"])
def test_scatter_chosen(routes_on, name):
    from tnc_amd import hiplib as H

    p = routes_on[name]
    assert p["kernel"] == H.GEMM_C128_3M and not p["direct"]
    assert (p["scatter_out"], p["ws_tmp_c"], p["kind"]) == (1, 0, 2)
    assert (p["m"], p["n"], p["k"]) == (2048, 1024, 32)


@pytest.mark.parametrize("name", ["run2", "m_lowest", "dim3", "k16",
                                  "tiles128"])
def test_scatter_refused(routes_on, name):
    p = routes_on[name]
    assert not p["direct"]
    assert (p["scatter_out"], p["kind"]) == (0, 3)
    assert p["ws_tmp_c"] == p["m"] * p["n"] * 16


def test_env_scatter_off():
    from tnc_amd import hiplib as H

    p, = run_child(PLAN_CHILD, "PLANS", {"TN_EPI_SCATTER": "0"},
                   json.dumps([ROUTE_CASES["interleaved"]]))
    assert p["kernel"] == H.GEMM_C128_3M
    assert (p["scatter_out"], p["kind"]) == (0, 3)
    assert p["ws_tmp_c"] == 2048 * 1024 * 16
