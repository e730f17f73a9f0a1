"""The GPU half of the kernel-reach table (tests/kernel_reach_cases.py).

Every case first re-asserts its plan (route, kernel, split-K, permute
kernels, pipeline windows, dot form: the same check test_kernel_reach_plan.py
makes on the CPU), then runs. A planner change therefore fails the case
instead of silently moving it to another kernel. What the table reaches:

  k_zgemm_v1              M / N / K guards, 65 column tiles, split-K   c128 c64
  k_zgemm_c128_glds       edge tiles, K-tail, ragged split-K           c128
  k_zgemm_mfma<float2>    the same shapes (f32 D-fragment row map)     c64
  k_zgemm_c128_glds_pure  1 tile, 3x3 tiles, ragged-K split            c128
  k_zgemm_c64_glds_pure   the same                                     c64
  k_permute_ct<false>     both packs and the unpack (R_packs)          c128 c64
  k_permute_tile          pack of A, pack of B, unpack, pipeline
                          window with a source gap                     c128 c64
  pack pipeline           ready-B window branch (P_subbox)             c128 c64
  k_dot_partial<*>        gather form, pow2 and not                    c128 c64
  k_dot_tile              tiled form                                   c128 c64

Comparison. The tiled-permute cases contract a random operand with a 0/1
selection matrix: the einsum is a permutation composed with a column (row)
selection, the 4M kernels and the split-K reduce add only exact zeros, and
the result must equal numpy indexing plus transpose bit for bit. Every other
case is held to the worst-case bound of a length-K complex inner product in
any summation order, with a factor of slack,

    |got - ref| <= 4 (K + 8) u S        u = 2^-53 (c128), 2^-24 (c64)

elementwise, where ref is the oracle in c128 on the inputs as given (c64
inputs rounded first, then widened) and S the oracle contraction of |A| and
|B|. The c64 dot kernels accumulate in double and round once:
4 (K + 8) 2^-53 S + 2^-23 |ref|. With N(0,1) operands one dropped or
misplaced product is of order 1; the bound at the largest non-exact K is
about 1e-2 in c64 (rag_split, K 271) and 1e-9 in c128 (P_subbox, K 512).

Guard bands. The GEMM-edge cases and R_packs run through
tn_einsum_c128_dev / tn_einsum_c64_dev over torch buffers laid out as
[256 guard | out | 256 guard] elements, the guards (and out) pre-filled with
a fixed NaN bit pattern, A and B each followed by 256 NaN elements. After
the call the guards must be bit-identical and the result free of NaN: a
store past either end of out, a read past the end of an operand that reaches
the result, or an element never stored all fail. With correct kernels every
access stays inside the operands.
"""

import ctypes
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_reach_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_SWITCHES = ("TN_NO_PIPELINE", "TN_PIPELINE_FORCE", "TN_GATHER_GEMM",
                "TN_GEMM3M", "TN_GEMM3M_PIPE", "TN_NO_PREPACK",
                "TN_EPI_SCATTER")
U = {"c128": 2.0 ** -53, "c64": 2.0 ** -24}
NPDT = {"c128": np.complex128, "c64": np.complex64}
GUARD = 256
# NaN as one f64 and as two f32
PATTERN = 0x7FF8DEAD7FC0BEEF


def labels(axes):
    return [l for l, _ in axes]


def dims(axes):
    return [d for _, d in axes]


def rand(shape, rng, dtype):
    x = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return x.astype(NPDT[dtype])


def rng_of(case, dtype):
    return np.random.default_rng(zlib.crc32(
        ("%s-%s" % (case["name"], dtype)).encode()))


def assert_plan(case, dtype):
    """In-process: the plan the run below will get (default switches)."""
    from tnc_amd import hiplib

    assert not case["env"]
    assert not [k for k in ENV_SWITCHES if os.environ.get(k)]
    p = hiplib.plan_step(*T.plan_args(case), dtype=dtype,
                         has_stream2=case["engine"])
    assert T.plan_mismatches(case, dtype, p, hiplib) == []
    assert p.kernel != hiplib.GEMM_C128_3M


def error_ratio(case, dtype, got, a, b):
    """max over elements of |got - ref| / bound; the bound comes from the
    oracle alone (module docstring)."""
    a128, b128 = a.astype(np.complex128), b.astype(np.complex128)
    al, bl = labels(case["a"]), labels(case["b"])
    ref = oracle.contract_ndarrays(case["out"], al, a128, bl, b128)
    S = oracle.contract_ndarrays(case["out"], al, np.abs(a128), bl,
                                 np.abs(b128))
    K = T.expected_plan(case, dtype)["k"]
    if case["group"] == "dot" and dtype == "c64":
        bound = 4 * (K + 8) * 2.0 ** -53 * S + 2.0 ** -23 * np.abs(ref)
    else:
        bound = 4 * (K + 8) * U[dtype] * S
    got = np.asarray(got)
    assert got.shape == np.shape(ref) and got.dtype == NPDT[dtype]
    assert np.all(bound > 0)
    return float(np.max(np.abs(got.astype(np.complex128) - ref) / bound))


def report(case, dtype, what):
    p = T.expected_plan(case, dtype)
    print("REACH %s %s %s %s" % (case["name"], dtype,
                                 p.get("kernel", p["dot_form"]), what))


# ---- runners ---------------------------------------------------------------

def run_host(case, dtype, a, b):
    from tnc_amd import hiplib

    fn = hiplib.einsum_c128 if dtype == "c128" else hiplib.einsum_c64
    return fn(case["out"], labels(case["a"]), a, labels(case["b"]), b)


def run_dev_guarded(case, dtype, a, b):
    """The device entry over torch buffers with guard bands (module
    docstring). Returns the result; asserts the guards and NaN-freeness."""
    import torch

    from tnc_amd import hiplib

    L = hiplib.lib()
    esize = 16 if dtype == "c128" else 8
    words = esize // 8  # int64 words per element
    real = np.float64 if dtype == "c128" else np.float32
    shape_of = dict(case["a"] + case["b"])
    out_shape = [shape_of[l] for l in case["out"]]
    nout = int(np.prod(out_shape))

    def operand(x):
        tail = np.full(GUARD, np.nan + 1j * np.nan, dtype=x.dtype)
        flat = np.concatenate([np.ascontiguousarray(x).reshape(-1), tail])
        return torch.from_numpy(flat.view(real)).cuda()

    a_dev, b_dev = operand(a), operand(b)
    buf = torch.full(((GUARD + nout + GUARD) * words,), PATTERN,
                     dtype=torch.int64, device="cuda")
    u64, vp = hiplib._u64arr, ctypes.c_void_p
    fn = L.tn_einsum_c128_dev if dtype == "c128" else L.tn_einsum_c64_dev
    torch.cuda.synchronize()
    rc = fn(u64(case["out"]), u64(out_shape), len(out_shape),
            u64(labels(case["a"])), u64(dims(case["a"])), None,
            vp(a_dev.data_ptr()), len(case["a"]),
            u64(labels(case["b"])), u64(dims(case["b"])), None,
            vp(b_dev.data_ptr()), len(case["b"]),
            vp(buf.data_ptr() + GUARD * esize), None)
    hiplib.check(rc, "tn_einsum_%s_dev" % dtype)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    lo, hi = host[:GUARD * words], host[-GUARD * words:]
    assert np.all(lo == PATTERN), "store below out"
    assert np.all(hi == PATTERN), "store past the end of out"
    got = host[GUARD * words:-GUARD * words].view(NPDT[dtype]).reshape(
        out_shape)
    assert not np.isnan(got).any(), "NaN in the result"
    return got


# ---- GEMM edges and R_packs: device entry, guard bands, derived bound ------
# torch brings a HIP runtime of its own, and of two runtimes in one process
# only the first to initialise finds the device. Loaded before the library,
# torch's runtime is the one the library binds to (same soname), so the
# guarded cases run in one child that imports torch first. The child runs
# every case and prints one record each; the tests below assert on them.

BOUNDED = [(c, d) for c, d in T.PAIRS if c["group"] in ("gemm", "packs")]

GUARD_CHILD = r"""
import json, sys
import torch
assert torch.cuda.is_available(), "torch sees no GPU"
torch.cuda.init()
tests_dir = sys.argv[1]
sys.path.insert(0, tests_dir)
import kernel_reach_cases as T
import test_gpu_kernel_reach as R

for cid in sys.argv[2:]:
    name, dtype = cid.rsplit("-", 1)
    case = T.by_name(name)
    rec = {"id": cid}
    try:
        R.assert_plan(case, dtype)
        rng = R.rng_of(case, dtype)
        a = R.rand(R.dims(case["a"]), rng, dtype)
        b = R.rand(R.dims(case["b"]), rng, dtype)
        got = R.run_dev_guarded(case, dtype, a, b)
        rec["ratio"] = R.error_ratio(case, dtype, got, a, b)
    except AssertionError as e:
        rec["error"] = "AssertionError: %s" % e
    except Exception as e:
        # a failed call or a device error: nothing more runs on the GPU
        rec["error"] = "%s: %s" % (type(e).__name__, e)
        print("CASE " + json.dumps(rec), flush=True)
        break
    print("CASE " + json.dumps(rec), flush=True)
"""


@pytest.fixture(scope="module")
def guarded_records():
    env = {k: v for k, v in os.environ.items() if k not in ENV_SWITCHES}
    proc = subprocess.run(
        [sys.executable, "-c", GUARD_CHILD, os.path.join(ROOT, "tests")]
        + ["%s-%s" % (c["name"], d) for c, d in BOUNDED],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    recs = {}
    for line in proc.stdout.splitlines():
        if line.startswith("CASE "):
            rec = json.loads(line[5:])
            recs[rec["id"]] = rec
    return proc, recs


@pytest.mark.parametrize("case,dtype", BOUNDED,
                         ids=["%s-%s" % (c["name"], d) for c, d in BOUNDED])
def test_gemm_edges_guarded(case, dtype, guarded_records):
    assert_plan(case, dtype)
    proc, recs = guarded_records
    rec = recs.get("%s-%s" % (case["name"], dtype))
    assert rec is not None, ("case did not run", proc.returncode,
                             proc.stdout[-2000:], proc.stderr[-2000:])
    assert "error" not in rec, rec["error"]
    report(case, dtype, "worst |err|/bound = %.3g" % rec["ratio"])
    assert rec["ratio"] <= 1.0


# ---- tiled permute: exact ---------------------------------------------------

def selection_case(case, dtype, rng):
    """(a, b, expect): one operand random, the other a 0/1 selection matrix;
    expect is the einsum by numpy indexing and transpose alone."""
    al, bl, out = labels(case["a"]), labels(case["b"]), case["out"]
    ad, bd = dict(case["a"]), dict(case["b"])
    m_legs = [l for l in out if l in ad]   # out order
    n_legs = [l for l in out if l in bd]
    M = int(np.prod([ad[l] for l in m_legs]))
    N = int(np.prod([bd[l] for l in n_legs]))
    one = NPDT[dtype](1)
    if case["select"] == "b":
        # B = [K legs][N legs] stored; one 1 per output column
        k_legs = [l for l in bl if l in ad]
        assert bl == k_legs + [l for l in bl if l not in ad]
        K = int(np.prod([ad[l] for l in k_legs]))
        a = rand(dims(case["a"]), rng, dtype)
        ksel = rng.integers(0, K, size=N)
        sel = np.zeros((K, N), dtype=NPDT[dtype])
        sel[ksel, np.arange(N)] = one
        b = sel.reshape(dims(case["b"]))
        a2 = np.transpose(a, [al.index(l) for l in m_legs + k_legs])
        c = a2.reshape(M, K)[:, ksel]
        n_stored = [l for l in bl if l not in ad]  # columns of sel
        c_legs = m_legs + n_stored
    else:
        # A = [M legs][K legs] stored; one 1 per output row
        k_legs = [l for l in al if l in bd]
        assert al == [l for l in al if l not in bd] + k_legs
        K = int(np.prod([ad[l] for l in k_legs]))
        b = rand(dims(case["b"]), rng, dtype)
        ksel = rng.integers(0, K, size=M)
        sel = np.zeros((M, K), dtype=NPDT[dtype])
        sel[np.arange(M), ksel] = one
        a = sel.reshape(dims(case["a"]))
        b2 = np.transpose(b, [bl.index(l) for l in k_legs + n_legs])
        c = b2.reshape(K, N)[ksel, :]
        m_stored = [l for l in al if l not in bd]  # rows of sel
        c_legs = m_stored + n_legs
    alld = dict(case["a"] + case["b"])
    c = c.reshape([alld[l] for l in c_legs])
    expect = np.transpose(c, [c_legs.index(l) for l in out])
    return a, b, np.ascontiguousarray(expect)


TPERM = [(c, d) for c, d in T.PAIRS if c["group"] == "tperm"]


@pytest.mark.parametrize("case,dtype", TPERM,
                         ids=["%s-%s" % (c["name"], d) for c, d in TPERM])
def test_tiled_permute_exact(case, dtype):
    assert_plan(case, dtype)
    a, b, expect = selection_case(case, dtype, rng_of(case, dtype))
    got = run_host(case, dtype, a, b)
    report(case, dtype, "exact")
    assert got.dtype == NPDT[dtype]
    np.testing.assert_array_equal(got, expect)


# ---- dots -------------------------------------------------------------------

DOTS = [(c, d) for c, d in T.PAIRS if c["group"] == "dot"]


@pytest.mark.parametrize("case,dtype", DOTS,
                         ids=["%s-%s" % (c["name"], d) for c, d in DOTS])
def test_dot_forms(case, dtype):
    assert_plan(case, dtype)
    rng = rng_of(case, dtype)
    a = rand(dims(case["a"]), rng, dtype)
    b = rand(dims(case["b"]), rng, dtype)
    got = run_host(case, dtype, a, b)
    ratio = error_ratio(case, dtype, got, a, b)
    report(case, dtype, "worst |err|/bound = %.3g" % ratio)
    assert ratio <= 1.0


# ---- pipeline window (environment-dependent: runs in a child) ---------------

PIPE_CHILD = r"""
import json, sys
tests_dir, name, dtype = sys.argv[1:4]
sys.path.insert(0, tests_dir)
import numpy as np
import kernel_reach_cases as T
import test_gpu_kernel_reach as R
from tnc_amd import hiplib
from tnc_amd.contraction_path import ContractionPath
from tnc_amd.executor import ContractionEngine
from tnc_amd.tensor import CompositeTensor, LeafTensor, TensorData

case = T.by_name(name)
p = hiplib.plan_step(*T.plan_args(case), dtype=dtype, has_stream2=True)
bad = T.plan_mismatches(case, dtype, p, hiplib)
assert bad == [] and p.kernel != hiplib.GEMM_C128_3M, bad
rng = R.rng_of(case, dtype)
a = R.rand(R.dims(case["a"]), rng, dtype)
b = R.rand(R.dims(case["b"]), rng, dtype)
leaves = []
for axes, data in ((case["a"], a), (case["b"], b)):
    t = LeafTensor(R.labels(axes), R.dims(axes))
    t.set_tensor_data(TensorData(TensorData.MATRIX, matrix=data))
    leaves.append(t)
eng = ContractionEngine(CompositeTensor(leaves),
                        ContractionPath.simple([(0, 1)]), dtype=dtype)
try:
    # the pipeline's window buffers come from the arena
    hiplib.check(hiplib.lib().tn_net_reserve(eng.net, 1 << 30), "reserve")
    eng.contract()
    legs, got = eng.result()
finally:
    eng.close()
assert list(legs) == case["out"], legs
ratio = R.error_ratio(case, dtype, got, a, b)
print("RATIO " + json.dumps(ratio))
"""

PIPE = [(c, d) for c, d in T.PAIRS if c["group"] == "pipe"]


@pytest.mark.parametrize("case,dtype", PIPE,
                         ids=["%s-%s" % (c["name"], d) for c, d in PIPE])
def test_pipeline_window_subbox(case, dtype):
    """Forced pack pipeline through the engine: each window of A is a
    2^20-element tiled permute whose source has a gap, B is ready so the
    window GEMMs read it in place."""
    env = {k: v for k, v in os.environ.items() if k not in ENV_SWITCHES}
    env.update(case["env"])
    proc = subprocess.run(
        [sys.executable, "-c", PIPE_CHILD, os.path.join(ROOT, "tests"),
         case["name"], dtype],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, (proc.stdout, proc.stderr)
    line = [l for l in proc.stdout.splitlines() if l.startswith("RATIO ")][-1]
    ratio = json.loads(line[6:])
    report(case, dtype, "worst |err|/bound = %.3g" % ratio)
    assert ratio <= 1.0


def test_every_case_runs():
    """No case of the table is left without a test above."""
    ran = BOUNDED + TPERM + DOTS + PIPE
    assert sorted(T.PAIR_IDS) == sorted("%s-%s" % (c["name"], d)
                                        for c, d in ran)
