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
  k_permute_ct<false>     second grid-stride pass (R_unpack_pass2)     c64
  k_dot_partial<*>        gather form, pow2 and not                    c128 c64
  k_dot_tile              tiled form                                   c128 c64
  k_dot_partial_linear    one block of 65; 2048 blocks, second pass    c128 c64
  k_einsum_smallk<false>  div/mod maps, K = 64, K = 1, rank-1 A,
                          strided A                                    c128 c64
                          second grid-stride pass (G_pass2_np2)        c64
  k_einsum_smallk<true>   gate apply, folded out permute, nout = 1     c128 c64
                          second grid-stride pass (G_pass2_p2)         c64
  k_einsum_smallk_tbl     2^26 elements, 8 passes (G_tbl)              c128 c64
  k_einsum_anyk<*>        K = 65, two K axes, pow2                     c128 c64

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

The gather cases run twice. Once with integer operands, real and imaginary
parts drawn from -4..4: every product and partial sum is an integer of
magnitude at most 32 K <= 2^15 (K <= 1024), far below 2^24, so the result is
exact in c64 and c128 in any summation order, with or without fma, and must
equal the oracle contraction of the same integers (computed in c128, cast)
bit for bit: a dropped, duplicated or misaddressed element cannot hide in a
tolerance. And once with N(0,1) operands against the bound above, which
integers alone would not hold an accumulator of the wrong width to. The big
cases (more than 2^25 output elements, T.big) run the integer way only,
through the host entry, against np.multiply.outer (K = 1) or np.tensordot
plus transpose.

Guard bands. The GEMM-edge cases, R_packs and the gather cases that are not
big run through
tn_einsum_c128_dev / tn_einsum_c64_dev over torch buffers laid out as
[256 guard | out | 256 guard] elements, the guards (and out) pre-filled with
a fixed NaN bit pattern, A and B each followed by 256 NaN elements. After
the call the guards must be bit-identical and the result free of NaN: a
store past either end of out, a read past the end of an operand that reaches
the result, or an element never stored all fail. With correct kernels every
access stays inside the operands. G_strided hands the device entry its
strides and a pointer one element into its [6, 4] base buffer; the guard
follows the whole base.
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


def ints(shape, rng, dtype):
    """Integer-valued complex: real and imaginary parts from -4..4, drawn as
    int8 (a 2^26-element operand is not generated through float64)."""
    x = np.empty(shape, dtype=NPDT[dtype])
    x.real = rng.integers(-4, 5, size=shape, dtype=np.int8)
    x.imag = rng.integers(-4, 5, size=shape, dtype=np.int8)
    return x


def rng_of(case, dtype):
    return np.random.default_rng(zlib.crc32(
        ("%s-%s" % (case["name"], dtype)).encode()))


def operands(case, dtype, draw):
    """(a, b, a_base) drawn by rand or ints from the case's seed. a_base is
    None, or for a strided case the flat buffer that `a` is a view into."""
    rng = rng_of(case, dtype)
    if "a_strides" in case:
        a_base = draw([case["a_base"]], rng, dtype)
        esize = a_base.itemsize
        a = np.lib.stride_tricks.as_strided(
            a_base[case["a_offset"]:], shape=dims(case["a"]),
            strides=[s * esize for s in case["a_strides"]], writeable=False)
    else:
        a_base, a = None, draw(dims(case["a"]), rng, dtype)
    return a, draw(dims(case["b"]), rng, dtype), a_base


def assert_plan(case, dtype):
    """In-process: the plan the run below will get (default switches)."""
    from tnc_amd import hiplib

    assert not case["env"]
    assert not [k for k in ENV_SWITCHES if os.environ.get(k)]
    p = hiplib.plan_step(*T.plan_args(case), dtype=dtype,
                         has_stream2=case["engine"], **T.plan_kwargs(case))
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


def exact_mismatches(case, dtype, got, a, b):
    """Number of elements that differ from the oracle contraction of the
    (integer-valued) operands, computed in c128 and cast."""
    ref = oracle.contract_ndarrays(
        case["out"], labels(case["a"]), a.astype(np.complex128),
        labels(case["b"]), b.astype(np.complex128)).astype(NPDT[dtype])
    got = np.asarray(got)
    assert got.shape == np.shape(ref) and got.dtype == NPDT[dtype]
    return int(np.count_nonzero(got != ref))


def report(case, dtype, what):
    p = T.expected_plan(case, dtype)
    kernel = (p["gather_kernel"] if case["group"] == "gather"
              else p.get("kernel") or p["dot_form"])
    print("REACH %s %s %s %s" % (case["name"], dtype, kernel, what))


# ---- runners ---------------------------------------------------------------

def run_host(case, dtype, a, b):
    from tnc_amd import hiplib

    fn = hiplib.einsum_c128 if dtype == "c128" else hiplib.einsum_c64
    return fn(case["out"], labels(case["a"]), a, labels(case["b"]), b)


def run_dev_guarded(case, dtype, a, b, a_base=None):
    """The device entry over torch buffers with guard bands (module
    docstring). Returns the result; asserts the guards and NaN-freeness.
    a_base: the flat buffer a strided `a` views (operands)."""
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

    a_dev, b_dev = operand(a if a_base is None else a_base), operand(b)
    a_ptr, a_strides = a_dev.data_ptr(), None
    if a_base is not None:
        a_ptr += case["a_offset"] * esize
        a_strides = hiplib._i64arr(case["a_strides"])
    buf = torch.full(((GUARD + nout + GUARD) * words,), PATTERN,
                     dtype=torch.int64, device="cuda")
    u64, vp = hiplib._u64arr, ctypes.c_void_p
    fn = L.tn_einsum_c128_dev if dtype == "c128" else L.tn_einsum_c64_dev
    torch.cuda.synchronize()
    rc = fn(u64(case["out"]), u64(out_shape), len(out_shape),
            u64(labels(case["a"])), u64(dims(case["a"])), a_strides,
            vp(a_ptr), len(case["a"]),
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

BOUNDED = [(c, d) for c, d in T.PAIRS
           if c["group"] in ("gemm", "packs", "gather") and not c.get("big")]
GEMM_EDGES = [(c, d) for c, d in BOUNDED if c["group"] != "gather"]
GATHER = [(c, d) for c, d in BOUNDED if c["group"] == "gather"]

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
        if case["group"] == "gather":
            a, b, a_base = R.operands(case, dtype, R.ints)
            got = R.run_dev_guarded(case, dtype, a, b, a_base)
            rec["mismatches"] = R.exact_mismatches(case, dtype, got, a, b)
        a, b, a_base = R.operands(case, dtype, R.rand)
        got = R.run_dev_guarded(case, dtype, a, b, a_base)
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


@pytest.mark.parametrize("case,dtype", GEMM_EDGES,
                         ids=["%s-%s" % (c["name"], d) for c, d in GEMM_EDGES])
def test_gemm_edges_guarded(case, dtype, guarded_records):
    assert_plan(case, dtype)
    proc, recs = guarded_records
    rec = recs.get("%s-%s" % (case["name"], dtype))
    assert rec is not None, ("case did not run", proc.returncode,
                             proc.stdout[-2000:], proc.stderr[-2000:])
    assert "error" not in rec, rec["error"]
    report(case, dtype, "worst |err|/bound = %.3g" % rec["ratio"])
    assert rec["ratio"] <= 1.0


# ---- gather route: guard bands, exact on integers, derived bound -----------

@pytest.mark.parametrize("case,dtype", GATHER,
                         ids=["%s-%s" % (c["name"], d) for c, d in GATHER])
def test_gather_guarded(case, dtype, guarded_records):
    assert_plan(case, dtype)
    proc, recs = guarded_records
    rec = recs.get("%s-%s" % (case["name"], dtype))
    assert rec is not None, ("case did not run", proc.returncode,
                             proc.stdout[-2000:], proc.stderr[-2000:])
    assert "error" not in rec, rec["error"]
    report(case, dtype, "integer mismatches = %d, worst |err|/bound = %.3g"
           % (rec["mismatches"], rec["ratio"]))
    assert rec["mismatches"] == 0
    assert rec["ratio"] <= 1.0


BIG = [(c, d) for c, d in T.PAIRS if c.get("big")]


def big_reference(case, a, b):
    """The contraction by numpy alone, in the operands' own dtype (exact on
    these integers): outer product when nothing is contracted, else
    tensordot; then the out order by transpose."""
    al, bl = labels(case["a"]), labels(case["b"])
    shared = [l for l in al if l in bl]
    if shared:
        c = np.tensordot(a, b, axes=([al.index(l) for l in shared],
                                     [bl.index(l) for l in shared]))
    else:
        c = np.multiply.outer(a, b)
    c_legs = ([l for l in al if l not in shared]
              + [l for l in bl if l not in shared])
    return np.transpose(c, [c_legs.index(l) for l in case["out"]])


@pytest.mark.parametrize("case,dtype", BIG,
                         ids=["%s-%s" % (c["name"], d) for c, d in BIG])
def test_second_pass_exact(case, dtype):
    """More than 2^25 output elements: the grid-stride loop of the case's
    kernel takes a second pass (G_tbl: eight). Integer operands, host entry,
    bit for bit."""
    assert_plan(case, dtype)
    assert T.nout_of(case) > 1 << 25
    a, b, _ = operands(case, dtype, ints)
    got = run_host(case, dtype, a, b)
    ref = big_reference(case, a, b)
    assert got.dtype == NPDT[dtype] and got.shape == ref.shape
    bad = int(np.count_nonzero(got != ref))
    report(case, dtype, "integer mismatches = %d of %d" % (bad, got.size))
    assert bad == 0


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
    a, b, _ = operands(case, dtype, rand)
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
    ran = GEMM_EDGES + GATHER + BIG + TPERM + DOTS + PIPE
    assert len(ran) == len(T.PAIRS)
    assert sorted(T.PAIR_IDS) == sorted("%s-%s" % (c["name"], d)
                                        for c, d in ran)
