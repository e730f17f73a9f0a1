"""The step planner (tn_plan_step), checked without a GPU.

The planner is the one place a contraction step's dispatch is decided; the
C++ executor, the prepack look-ahead and the Python arena model all read it.
Route expectations below were derived by reading the dispatch as it stood
before the planner existed (einsum_dev_impl at commit 303c7bf); the fixture
pins are the values that commit's Python model produced.
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

# labels
M_, N_, K_, K2_ = 1, 2, 3, 4


def plan(out, a, b, **kw):
    """out/a/b are [(label, dim), ...] lists."""
    from tnc_amd import hiplib

    return hiplib.plan_step(
        [l for l, _ in out], [d for _, d in out],
        [l for l, _ in a], [d for _, d in a],
        [l for l, _ in b], [d for _, d in b], **kw)


def mm(m, k, n, **kw):
    """A[m,k] . B[k,n] -> [m,n], all contiguous."""
    return plan([(M_, m), (N_, n)], [(M_, m), (K_, k)], [(K_, k), (N_, n)],
                **kw)


# ---- pins against the parent commit --------------------------------------

PINS = [
    # fixture, dtype, esize, steps, packa, packb, pipelined {step: P}, arena
    ("rqc24", "c128", 16, 262, 191, 176, {}, 1070067),
    ("rqc36", "c128", 16, 720, 595, 582, {}, 104351557222),
    ("syc49", "c64", 8, 968, 743, 640, {966: 8}, 175343088435),
]


@pytest.mark.parametrize("name,dtype,esize,nsteps,npacka,npackb,pipe,arena",
                         PINS, ids=[p[0] for p in PINS])
def test_fixture_pins(name, dtype, esize, nsteps, npacka, npackb, pipe, arena):
    from tnc_amd.contraction_path import ContractionPath, flatten_network
    from tnc_amd.executor import arena_bytes, plan_steps
    from tnc_amd.fixtures import load_fixture

    tn, replace_toplevel, _ = load_fixture(name)
    leaves, steps, _ = flatten_network(tn,
                                       ContractionPath.simple(replace_toplevel))
    infos = plan_steps(leaves, steps, dtype)
    assert len(infos) == nsteps
    assert sum(bool(i.packa) for i in infos) == npacka
    assert sum(bool(i.packb) for i in infos) == npackb
    assert {s: i.pipe_p for s, i in enumerate(infos) if i.pipe_p} == pipe
    assert arena_bytes(leaves, steps, infos, esize) == arena


# ---- route table ----------------------------------------------------------

def test_dot_linear():
    from tnc_amd import hiplib as H

    p = plan([], [(K_, 128)], [(K_, 128)])
    assert (p.route, p.dot_form, p.kind) == (H.ROUTE_DOT, H.DOT_LINEAR, 5)
    assert (p.m, p.n, p.k) == (1, 1, 128)


def test_dot_gather_form():
    from tnc_amd import hiplib as H

    p = plan([], [(K_, 8), (K2_, 16)], [(K2_, 16), (K_, 8)])
    assert (p.route, p.dot_form, p.kind) == (H.ROUTE_DOT, H.DOT_GATHER, 1)


def test_dot_tiled():
    from tnc_amd import hiplib as H

    p = plan([], [(K_, 1024), (K2_, 1024)], [(K2_, 1024), (K_, 1024)])
    assert (p.route, p.dot_form, p.kind) == (H.ROUTE_DOT, H.DOT_TILED, 6)
    assert p.tbits == 8 and p.dot_blocks == 256
    assert p.ws_dot == 256 * 16


@pytest.mark.parametrize("m,k,n", [(8, 4, 8), (4, 128, 64)],
                         ids=["smallk", "skinny"])
def test_gather_route(m, k, n):
    from tnc_amd import hiplib as H

    p = mm(m, k, n)
    assert (p.route, p.kind) == (H.ROUTE_GATHER, 0)
    assert p.ws_pack_a == p.ws_pack_b == p.ws_tmp_c == p.ws_split == 0
    assert p.gather_kernel == (H.GK_SMALLK_P2 if k <= 64 else H.GK_ANYK_P2)
    assert p.gather_blocks == 1


def test_gather_kernel_only_where_run_gather_can_run():
    """gather_kernel / gather_blocks are set on the gather route and on TTGT
    steps with gather_ok (the out-of-memory fallback), 0 elsewhere."""
    from tnc_amd import hiplib as H

    # dot route
    p = plan([], [(K_, 128)], [(K_, 128)])
    assert p.route == H.ROUTE_DOT
    assert (p.gather_kernel, p.gather_blocks) == (H.GK_NONE, 0)
    # TTGT, K > 64 and not skinny: no fallback
    p = mm(16, 128, 16)
    assert p.route == H.ROUTE_TTGT and not p.gather_ok
    assert (p.gather_kernel, p.gather_blocks) == (H.GK_NONE, 0)
    # TTGT with gather_ok: K <= 64 ...
    p = mm(128, 16, 64)
    assert p.route == H.ROUTE_TTGT and p.gather_ok
    assert (p.gather_kernel, p.gather_blocks) == (H.GK_SMALLK_P2, 32)
    p = mm(129, 64, 65)
    assert p.route == H.ROUTE_TTGT and p.gather_ok
    assert (p.gather_kernel, p.gather_blocks) == (H.GK_SMALLK, 33)
    # ... the grid is capped at 64 * 2048 blocks
    p = mm(1 << 14, 16, 1 << 12)
    assert p.route == H.ROUTE_TTGT and p.gather_ok
    assert (p.gather_kernel, p.gather_blocks) == (H.GK_SMALLK_P2, 1 << 17)


def test_ttgt_v1():
    from tnc_amd import hiplib as H

    p = mm(16, 128, 16)
    assert (p.route, p.kind) == (H.ROUTE_TTGT, 2)
    assert not p.pack_a and not p.pack_b
    assert p.kernel == H.GEMM_V1
    assert p.row_tiles * p.col_tiles == 1 and p.splitk == 1


def test_ttgt_pure():
    from tnc_amd import hiplib as H

    p = mm(128, 16, 64)
    assert p.route == H.ROUTE_TTGT and not p.pack_a and not p.pack_b
    assert p.splitk == 1 and p.kernel == H.GEMM_C128_PURE
    assert mm(128, 16, 64, dtype="c64").kernel == H.GEMM_C64_PURE


def test_ttgt_ragged():
    from tnc_amd import hiplib as H

    p = mm(40, 72, 40)
    assert p.route == H.ROUTE_TTGT and p.kernel == H.GEMM_C128_GLDS
    assert mm(40, 72, 40, dtype="c64").kernel == H.GEMM_MFMA


def test_ttgt_splitk():
    from tnc_amd import hiplib as H

    p = mm(128, 4096, 64)
    assert (p.splitk, p.kchunk) == (64, 64)
    assert p.kernel == H.GEMM_C128_PURE
    assert p.ws_split == 64 * 128 * 64 * 16


def test_ttgt_3m():
    from tnc_amd import hiplib as H

    p = mm(2048, 32, 1024)
    assert p.row_tiles * p.col_tiles == 256 and p.splitk == 1
    assert p.kernel == H.GEMM_C128_3M
    assert mm(2048, 32, 1024, dtype="c64").kernel == H.GEMM_C64_PURE


def test_ttgt_pack_a():
    from tnc_amd import hiplib as H

    p = plan([(M_, 128), (N_, 64)], [(K_, 16), (M_, 128)],
             [(K_, 16), (N_, 64)])
    assert p.route == H.ROUTE_TTGT
    assert p.pack_a and not p.pack_b
    assert p.ws_pack_a == 128 * 16 * 16 and p.ws_pack_b == 0
    # a 2^11-element pack goes through the gather permute
    assert (p.perm_a, p.perm_b, p.perm_out) == (H.PERM_CT, 0, 0)
    assert (p.pipe_perm_a, p.pipe_perm_b) == (0, 0)


def test_ttgt_out_permute():
    from tnc_amd import hiplib as H

    p = plan([(N_, 64), (M_, 128)], [(M_, 128), (K_, 16)],
             [(K_, 16), (N_, 64)])
    assert p.route == H.ROUTE_TTGT
    assert not p.direct and p.kind == 3
    assert p.ws_tmp_c == 128 * 64 * 16
    assert (p.perm_a, p.perm_b, p.perm_out) == (0, 0, H.PERM_CT)


def test_invalid_operands():
    from tnc_amd import hiplib

    with pytest.raises(RuntimeError, match="rc=1.*out label 1 present in both"):
        plan([(M_, 4)], [(M_, 4), (K_, 4)], [(K_, 4), (M_, 4)])
    assert hiplib.last_error() == "out label 1 present in both inputs"
    with pytest.raises(RuntimeError,
                       match="rc=1.*label 9 of A neither contracted nor in"):
        plan([(M_, 4), (N_, 4)], [(M_, 4), (9, 2), (K_, 4)],
             [(K_, 4), (N_, 4)])
    assert (hiplib.last_error()
            == "label 9 of A neither contracted nor in out")


# ---- env switches (read once: one child process each) ---------------------

CHILD = r"""
import json, sys
from tnc_amd import hiplib
case = json.loads(sys.argv[1])
p = hiplib.plan_step(*case["args"], has_stream2=True)
print("PLAN " + json.dumps({f: getattr(p, f) for f, _ in p._fields_}))
"""

# operand shapes of PIPELINE_CASE / GATHER_CASE in test_gpu_altpaths.py
PIPELINE_ARGS = [[1, 2, 3, 20, 21], [8, 16, 16, 16, 64],
                 [10, 1, 11, 2, 12, 3, 13], [4, 8, 4, 16, 4, 16, 4],
                 [10, 20, 11, 12, 13, 21], [4, 16, 4, 4, 4, 64]]
GATHER_ARGS = [[1, 2, 20], [16, 16, 64],
               [10, 1, 11, 2, 12], [4, 16, 4, 16, 4],
               [12, 20, 10, 11], [4, 64, 4, 4]]


def mm_args(m, k, n):
    return [[M_, N_], [m, n], [M_, K_], [m, k], [K_, N_], [k, n]]


def plan_in_child(args, env_extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("TN_NO_PIPELINE", "TN_PIPELINE_FORCE",
                        "TN_GATHER_GEMM", "TN_GEMM3M")}
    env.update(env_extra)
    proc = subprocess.run(
        [sys.executable, "-c", CHILD, json.dumps({"args": args})],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, (proc.stdout, proc.stderr)
    line = [l for l in proc.stdout.splitlines() if l.startswith("PLAN ")][-1]
    return json.loads(line[5:])


def test_env_pipeline_force():
    p = plan_in_child(PIPELINE_ARGS, {"TN_PIPELINE_FORCE": "1"})
    assert (p["pipe_p"], p["pipe_kc"], p["pipe_npre"]) == (16, 16, 2)
    assert p["ws_slices"] == 16 * 2048 * 1024 * 16
    assert plan_in_child(PIPELINE_ARGS, {})["pipe_p"] == 0


def test_env_gemm3m_off():
    from tnc_amd import hiplib as H

    p = plan_in_child(mm_args(2048, 32, 1024), {"TN_GEMM3M": "0"})
    assert p["kernel"] == H.GEMM_C128_PURE


def test_env_gemm3m_force():
    from tnc_amd import hiplib as H

    p = plan_in_child(mm_args(128, 4096, 64), {"TN_GEMM3M": "force"})
    assert p["kernel"] == H.GEMM_C128_3M and p["splitk"] == 64


def test_env_gather_gemm():
    from tnc_amd import hiplib as H

    p = plan_in_child(GATHER_ARGS, {"TN_GATHER_GEMM": "1"})
    assert p["kernel"] == H.GEMM_C128_GATHER and p["gather_gemm"]
    assert p["ws_pack_a"] == p["ws_pack_b"] == 0
