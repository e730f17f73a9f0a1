"""The CPU half of the kernel-reach table (tests/kernel_reach_cases.py):
every case must plan as the table says, so that the GPU half
(test_gpu_kernel_reach.py) runs the kernel each case is named for. Needs no
GPU.

Checked per case and dtype: route, kernel, splitk, kchunk, kind, pack_a/b,
perm_*, pipe_p / pipe_kc / pipe_perm_*, dot_form, gather_kernel and
gather_blocks where the case names them; that the kernel is not the
3M GEMM (which has test files of its own); and for a split-K case the length
of the last slice. The environment switches are read once per process, so
cases that depend on them plan in a child with the environment set.
"""

import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_reach_cases as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tnc_amd", "libtnc_hip.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB),
                                reason="library not built")

ENV_SWITCHES = ("TN_NO_PIPELINE", "TN_PIPELINE_FORCE", "TN_GATHER_GEMM",
                "TN_GEMM3M", "TN_GEMM3M_PIPE", "TN_NO_PREPACK",
                "TN_EPI_SCATTER")

PLAN_CHILD = r"""
import json, sys
from tnc_amd import hiplib
args, kwargs, dtype, stream2 = json.loads(sys.argv[1])
p = hiplib.plan_step(*args, dtype=dtype, has_stream2=stream2, **kwargs)
print("PLAN " + json.dumps({f: getattr(p, f) for f, _ in p._fields_}))
"""


def plan_case(case, dtype):
    """The case's plan as a dict, planned under the case's environment."""
    env = {k: v for k, v in os.environ.items() if k not in ENV_SWITCHES}
    env.update(case["env"])
    proc = subprocess.run(
        [sys.executable, "-c", PLAN_CHILD,
         json.dumps([T.plan_args(case), T.plan_kwargs(case), dtype,
                     case["engine"]])],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, (proc.stdout, proc.stderr)
    line = [l for l in proc.stdout.splitlines() if l.startswith("PLAN ")][-1]
    return json.loads(line[5:])


@pytest.mark.parametrize("case,dtype", T.PAIRS, ids=T.PAIR_IDS)
def test_case_plans_as_tabled(case, dtype):
    from tnc_amd import hiplib

    if case["env"]:
        got = plan_case(case, dtype)
    else:
        # default switches: the parent process must not carry any either
        assert not [k for k in ENV_SWITCHES if os.environ.get(k)]
        p = hiplib.plan_step(*T.plan_args(case), dtype=dtype,
                             has_stream2=case["engine"],
                             **T.plan_kwargs(case))
        got = {f: getattr(p, f) for f, _ in p._fields_}
    assert T.plan_mismatches(case, dtype, got, hiplib) == []
    assert got["kernel"] != hiplib.GEMM_C128_3M


def test_table_covers_what_it_claims():
    """The table as a whole reaches every kernel the GPU half is there for."""
    from tnc_amd import hiplib

    kernels = {(d, T.expected_plan(c, d).get("kernel"))
               for c, d in T.PAIRS if c["group"] != "dot"}
    for d, k in [("c128", "GEMM_V1"), ("c64", "GEMM_V1"),
                 ("c128", "GEMM_C128_GLDS"), ("c64", "GEMM_MFMA"),
                 ("c128", "GEMM_C128_PURE"), ("c64", "GEMM_C64_PURE")]:
        assert (d, k) in kernels and hasattr(hiplib, k)
    for field in ("perm_a", "perm_b", "perm_out", "pipe_perm_a"):
        for d in ("c128", "c64"):
            assert any(T.expected_plan(c, d).get(field) == hiplib.PERM_TILE
                       for c, dt in T.PAIRS if dt == d), (field, d)
    assert {c["plan"]["dot_form"] for c in T.DOT_CASES} == {
        "DOT_LINEAR", "DOT_GATHER", "DOT_TILED"}
    # every gather kernel, in both dtypes
    gks = ("GK_SMALLK", "GK_SMALLK_P2", "GK_SMALLK_TBL", "GK_ANYK",
           "GK_ANYK_P2")
    assert sorted(getattr(hiplib, g) for g in gks) == [1, 2, 3, 4, 5]
    assert hiplib.GK_NONE == 0
    for d in ("c128", "c64"):
        assert {c["plan"]["gather_kernel"] for c in T.GATHER_CASES
                if d in c["dtypes"]} == set(gks), d
    # a second pass of the grid-stride loops: grid_for caps the grid at
    # 64 * 2048 blocks of 256 threads = 2^25 threads
    assert any(T.nout_of(c) > 1 << 25 for c in T.GATHER_CASES)
    assert any(T.nout_of(c) > 1 << 25 for c in T.CASES
               if c["plan"].get("perm_out") == hiplib.PERM_CT)
    for c in T.CASES:
        assert bool(c.get("big")) == (T.nout_of(c) > 1 << 25), c["name"]
    # the ready-B window branch of the pipeline
    p = T.P_SUBBOX["plan"]
    assert p["pipe_p"] and not p["pack_b"] and p["pipe_perm_b"] == 0
    # every split case names its last slice; the ragged ones are short
    split = {c["name"] for c in T.CASES if c["plan"].get("splitk", 1) > 1}
    assert split == set(T.LAST_SLICE)
    for name in ("v1_split", "rag_split", "pure_split"):
        assert T.LAST_SLICE[name] < T.by_name(name)["plan"]["kchunk"]


def test_pipe_perm_fields_zero_without_pipeline():
    """pipe_perm_* are 0 when pipe_p == 0, whatever the serial packs are."""
    from tnc_amd import hiplib

    p = hiplib.plan_step(*T.plan_args(T.by_name("T1_interleave")),
                         has_stream2=True)
    assert p.pipe_p == 0 and (p.pipe_perm_a, p.pipe_perm_b) == (0, 0)
    assert p.perm_a == hiplib.PERM_TILE


def test_scalar_k65_is_a_dot():
    """G_scalar64 is the last scalar-output step on the gather route: one
    more K element plans ROUTE_DOT (D_linear65), and gather_kernel is 0."""
    from tnc_amd import hiplib

    for dtype in ("c128", "c64"):
        p = hiplib.plan_step([], [], [101], [64], [101], [64], dtype=dtype)
        assert (p.route, p.gather_kernel) == (hiplib.ROUTE_GATHER,
                                              hiplib.GK_SMALLK_P2)
        p = hiplib.plan_step([], [], [101], [65], [101], [65], dtype=dtype)
        assert p.route == hiplib.ROUTE_DOT
        assert (p.gather_kernel, p.gather_blocks) == (hiplib.GK_NONE, 0)
