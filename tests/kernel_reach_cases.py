"""The kernel-reach case table: named einsum cases and the plan each must get.

Data only. tests/test_kernel_reach_plan.py plans every case on the CPU and
checks the plan; tests/test_gpu_kernel_reach.py re-asserts the plan and then
runs the case on the GPU, so a case cannot drift to another kernel unnoticed.

A case is a dict:
  name            case id
  group           "gemm" | "packs" | "tperm" | "pipe" | "dot" | "gather"
  a, b            [(label, dim), ...] in stored (row-major) order
  a_strides       optional: element strides of A, a view into a larger buffer
                  of a_base elements starting at element a_offset
  big             optional flag: more than 2^25 output elements. Runs once,
                  through the host entry, with integer operands, compared
                  bit for bit
  out             out labels
  dtypes          the dtypes the case runs in
  env             environment the plan depends on ({} = default switches)
  engine          True: runs through ContractionEngine (has_stream2 = True);
                  False: through the einsum entry points (has_stream2 = False)
  plan            expected tn_step_plan fields; a (c128, c64) tuple where the
                  dtypes differ. route / kernel / dot_form are names of the
                  hiplib constants (ROUTE_*, GEMM_*, DOT_*, GK_*).
  select          tperm only: which operand is the 0/1 selection matrix
                  ("a" or "b"); the other one is random

Labels: M legs 1.., K legs 101.., N legs 200 / 201...

Grid-stride second passes. grid_for caps a grid at 64 * 2048 blocks of 256
threads = 2^25 threads (the table kernel at 32768 blocks = 2^23), so a loop
`for (p = ...; p < nout; p += gridDim.x * blockDim.x)` takes a second pass
only past 2^25 elements. The big cases do that for k_einsum_smallk<false>
(G_pass2_np2), k_einsum_smallk<true> (G_pass2_p2), k_einsum_smallk_tbl
(G_tbl, 8 passes) and k_permute_ct<false> (R_unpack_pass2). Two loops of the
same shape stay on their first pass in this suite: k_einsum_anyk, because a
K > 64 operand at that nout is several GB, and k_splitk_reduce, because
split-K needs fewer than 192 tiles and nout then stays below 2^21. No test
of this table takes those two further.
"""

M0, K0, N0 = 1, 101, 201
N_WIDE = 200


def _legs(base, count, dim=2):
    return [(base + i, dim) for i in range(count)]


def _interleave(x, y):
    """x1 y1 x2 y2 ... then the rest of the longer list."""
    out = []
    for i in range(max(len(x), len(y))):
        if i < len(x):
            out.append(x[i])
        if i < len(y):
            out.append(y[i])
    return out


NO_PERM = dict(perm_a=0, perm_b=0, perm_out=0, pipe_p=0, pipe_kc=0,
               pipe_perm_a=0, pipe_perm_b=0)

# ---- GEMM edges: 2-D contiguous operands, out = [M, N], no packs ----------

V1 = ("GEMM_V1", "GEMM_V1")
RAGGED = ("GEMM_C128_GLDS", "GEMM_MFMA")
PURE = ("GEMM_C128_PURE", "GEMM_C64_PURE")


def _gemm(name, m, k, n, kernel, splitk, kchunk):
    return dict(
        name=name, group="gemm", dtypes=("c128", "c64"), env={}, engine=False,
        a=[(M0, m), (K0, k)], b=[(K0, k), (N_WIDE, n)], out=[M0, N_WIDE],
        plan=dict(NO_PERM, route="ROUTE_TTGT", kind=2, kernel=kernel,
                  m=m, k=k, n=n, splitk=splitk, kchunk=kchunk,
                  pack_a=0, pack_b=0, dot_form="DOT_LINEAR"))


GEMM_CASES = [
    # one tile, M and N edges, K-tail of 1
    _gemm("v1_edge", 17, 65, 31, V1, 1, 80),
    # transposed raggedness
    _gemm("v1_edge_t", 31, 129, 17, V1, 1, 144),
    # 65 column tiles, the last 1 wide
    _gemm("v1_manycol", 16, 65, 4097, V1, 1, 80),
    # split-K, last slice 31
    _gemm("v1_split", 31, 271, 17, V1, 4, 80),
    # one edge tile, guarded staging throughout
    _gemm("rag_1tile", 33, 65, 33, RAGGED, 1, 80),
    # interior tile takes LDS-DMA slabs plus a guarded K-tail; three edge
    # tiles with edges of 1
    _gemm("rag_2x2", 129, 79, 65, RAGGED, 1, 80),
    # split-K, last slice 31 with a tail of 15
    _gemm("rag_split", 255, 271, 65, RAGGED, 4, 80),
    # one tile, one slab
    _gemm("pure_1", 128, 16, 64, PURE, 1, 16),
    # tile-index strides, 3 slabs
    _gemm("pure_3x3", 384, 48, 192, PURE, 1, 48),
    # split-K, last slice 32
    _gemm("pure_split", 128, 272, 64, PURE, 4, 80),
]

# both packs and the unpack through k_permute_ct<false>, ragged kernel
R_PACKS = dict(
    name="R_packs", group="packs", dtypes=("c128", "c64"), env={},
    engine=False,
    a=[(101, 5), (1, 7), (102, 13), (2, 5)],
    b=[(201, 3), (102, 13), (202, 11), (101, 5)],
    out=[201, 1, 202, 2],
    plan=dict(NO_PERM, route="ROUTE_TTGT", kind=3, kernel=RAGGED,
              m=35, k=65, n=33, splitk=1, kchunk=80, pack_a=1, pack_b=1,
              perm_a=1, perm_b=1, perm_out=1, dot_form="DOT_LINEAR"))

# ---- tiled permute: exact cases (one operand a 0/1 selection matrix) ------

_M12, _K8 = _legs(M0, 12), _legs(K0, 8)
_T1_B = _K8 + [(N_WIDE, 64)]
_T1_OUT = [l for l, _ in _M12] + [N_WIDE]
_T1_PLAN = dict(NO_PERM, route="ROUTE_TTGT", kind=2, kernel=PURE,
                m=4096, k=256, n=64, splitk=4, kchunk=64, pack_a=1, pack_b=0,
                perm_a=2, dot_form="DOT_LINEAR")


def _tperm(name, a, b, out, plan, select):
    return dict(name=name, group="tperm", dtypes=("c128", "c64"), env={},
                engine=False, a=a, b=b, out=out, plan=plan, select=select)


_N12 = _legs(N0, 12)
_M10, _N10 = _legs(M0, 10), _legs(N0, 10)

TPERM_CASES = [
    # A stored m1 k1 m2 k2 ... m8 k8 m9..m12
    _tperm("T1_interleave", _interleave(_M12, _K8), _T1_B, _T1_OUT, _T1_PLAN,
           "b"),
    # A stored [K legs reversed][M legs], out M legs reversed; B's K legs are
    # then out of A's order: a small (2^14) pack of B through k_permute_ct
    _tperm("T1_reverse", _K8[::-1] + _M12, _T1_B, _T1_OUT[-2::-1] + [N_WIDE],
           dict(_T1_PLAN, pack_b=1, perm_b=1), "b"),
    # A stored [m1..m6][k1..k8][m7..m12]
    _tperm("T1_block", _M12[:6] + _K8 + _M12[6:], _T1_B, _T1_OUT, _T1_PLAN,
           "b"),
    # A stored [m1..m6][k1 k2][m7..m12][k3..k8]: the six lowest source bits
    # stay the six lowest destination bits of the pack
    _tperm("T1_lowfixed", _M12[:6] + _K8[:2] + _M12[6:] + _K8[2:], _T1_B,
           _T1_OUT, _T1_PLAN, "b"),
    # mixed pow2 dims 16 / 64 / 4
    _tperm("T1_mixed",
           [(101, 16), (1, 64), (102, 4), (2, 16), (103, 4), (3, 4)],
           [(101, 16), (102, 4), (103, 4), (N_WIDE, 64)], [3, 1, 2, N_WIDE],
           _T1_PLAN, "b"),
    # B stored n1 k1 n2 k2 ... n8 k8 n9..n12; A ready
    _tperm("T2_packB", [(M0, 128)] + _K8, _interleave(_N12, _K8),
           [M0] + [l for l, _ in _N12],
           dict(NO_PERM, route="ROUTE_TTGT", kind=2, kernel=PURE,
                m=128, k=256, n=4096, splitk=4, kchunk=64, pack_a=0,
                pack_b=1, perm_b=2, dot_form="DOT_LINEAR"), "a"),
    # out order n1 m1 n2 m2 ...: the unpack is the tiled permute
    _tperm("T3_unpack", _M10 + [(K0, 16)], [(K0, 16)] + _N10,
           [l for l, _ in _interleave(_N10, _M10)],
           dict(NO_PERM, route="ROUTE_TTGT", kind=3, kernel=PURE,
                m=1024, k=16, n=1024, splitk=1, kchunk=16, pack_a=0,
                pack_b=0, perm_out=2, dot_form="DOT_LINEAR"), "b"),
]

# ---- pipeline window: sub-box tiled permute, ready-B window branch --------
# The engine stores a step's output in symmetric-difference order: A-only
# legs in A order, then B-only legs.
P_SUBBOX = dict(
    name="P_subbox", group="pipe", dtypes=("c128", "c64"),
    env={"TN_PIPELINE_FORCE": "1", "TN_GEMM3M": "0"}, engine=True,
    a=[(2, 64), (100, 2), (1, 64), (101, 256)],
    b=[(100, 2), (101, 256), (N_WIDE, 512)],
    out=[2, 1, N_WIDE],
    plan=dict(route="ROUTE_TTGT", kind=2, kernel=PURE, m=4096, k=512, n=512,
              splitk=1, kchunk=512, pack_a=1, pack_b=0, perm_a=2, perm_b=0,
              perm_out=0, pipe_p=2, pipe_kc=256, pipe_perm_a=2, pipe_perm_b=0,
              dot_form="DOT_LINEAR"))

# ---- dots -----------------------------------------------------------------


def _dot(name, a, plan, dtypes=("c128", "c64")):
    return dict(name=name, group="dot", dtypes=dtypes, env={}, engine=False,
                a=a, b=a[::-1], out=[],
                plan=dict(NO_PERM, route="ROUTE_DOT", m=1, n=1, **plan))


DOT_CASES = [
    # gather form, non-pow2 dims: k_dot_partial<false>
    _dot("D_np2", [(101, 3), (102, 5), (103, 7), (104, 11)],
         dict(k=1155, kind=1, dot_form="DOT_GATHER", tbits=0, dot_blocks=5)),
    # gather form, pow2 dims, K = 4096 < 2^20: k_dot_partial<true>
    _dot("D_p2", _legs(K0, 12),
         dict(k=4096, kind=1, dot_form="DOT_GATHER", tbits=0, dot_blocks=16)),
    # tiled form
    _dot("D_tiled", _legs(K0, 20),
         dict(k=1 << 20, kind=6, dot_form="DOT_TILED", tbits=8,
              dot_blocks=256)),
    # linear form, the first K past the gather route: one block, 65 of its
    # 256 threads live
    _dot("D_linear65", [(K0, 65)],
         dict(k=65, kind=5, dot_form="DOT_LINEAR", tbits=0, dot_blocks=1)),
    # linear form at the block cap: every block takes a second pass, the
    # tail of 77 is partial
    _dot("D_linear_stride", [(K0, 256 * 2048 + 77)],
         dict(k=256 * 2048 + 77, kind=5, dot_form="DOT_LINEAR", tbits=0,
              dot_blocks=2048)),
]

# ---- gather route: k_einsum_smallk<*>, k_einsum_smallk_tbl, k_einsum_anyk<*>
# gather_kernel is what run_gather launches; gather_blocks its grid.


def _gather(name, a, b, out, m, n, k, kernel, blocks, dtypes=("c128", "c64"),
            **extra):
    return dict(name=name, group="gather", dtypes=dtypes, env={},
                engine=False, a=a, b=b, out=out,
                plan=dict(NO_PERM, route="ROUTE_GATHER", kind=0, m=m, n=n,
                          k=k, gather_kernel=kernel, gather_blocks=blocks),
                **extra)


# a rank-8 qubit state with the gate's two qubits at positions 3 and 5
_Q8 = _legs(M0, 3) + [(K0, 2)] + [(M0 + 3, 2)] + [(K0 + 1, 2)] + _legs(5, 2)
_GATE = [(N0, 2), (N0 + 1, 2), (K0, 2), (K0 + 1, 2)]
# 26 qubits, the gate's at positions 3 and 17
_Q26 = (_legs(M0, 3) + [(K0, 2)] + _legs(4, 13) + [(K0 + 1, 2)]
        + _legs(17, 8))
# the 26 out legs, shuffled once (numpy default_rng(26).permutation)
_Q26_OUT = [15, 21, 2, 4, 6, 10, 7, 202, 8, 11, 22, 16, 13, 19, 24, 9, 1, 201,
            3, 14, 17, 20, 23, 12, 18, 5]

GATHER_CASES = [
    # div/mod decode
    _gather("G_np2", [(1, 3), (2, 5), (101, 7)], [(101, 7), (201, 4)],
            [1, 2, 201], 15, 4, 7, "GK_SMALLK", 1),
    # the rqc36 workhorse: a two-qubit gate applied in place. The out map
    # has 8 axes, but nout is far below the table kernel's 2^26
    _gather("G_gate", _Q8, _GATE, [1, 2, 3, 201, 4, 202, 5, 6], 64, 4, 4,
            "GK_SMALLK_P2", 1),
    # the same, an out permute folded into the map (default_rng(8))
    _gather("G_gate_outorder", _Q8, _GATE, [4, 202, 1, 6, 201, 2, 3, 5],
            64, 4, 4, "GK_SMALLK_P2", 1),
    # K = TN_SMALLK: all 64 LDS offset slots
    _gather("G_k64", [(1, 8), (101, 64)], [(101, 64), (201, 300)], [1, 201],
            8, 300, 64, "GK_SMALLK", 10),
    # neither skinny nor GEMM-worthy
    _gather("G_k64_mid", [(1, 100), (101, 64)], [(101, 64), (201, 50)],
            [1, 201], 100, 50, 64, "GK_SMALLK", 20),
    # the first K past the LDS table
    _gather("G_k65", [(1, 8), (101, 65)], [(101, 65), (201, 300)], [1, 201],
            8, 300, 65, "GK_ANYK", 10),
    # two K axes, B's in the other order
    _gather("G_k65_np2", [(1, 3), (101, 5), (102, 13)],
            [(102, 13), (101, 5), (201, 301)], [1, 201], 3, 301, 65,
            "GK_ANYK", 4),
    _gather("G_anyk_p2", [(1, 4), (101, 1024)], [(101, 1024), (201, 4096)],
            [1, 201], 4, 4096, 1024, "GK_ANYK_P2", 64),
    # rank-1 A: no A-only out axis
    _gather("G_m1", [(101, 64)], [(101, 64), (201, 1000)], [201],
            1, 1000, 64, "GK_SMALLK", 4),
    # nout = 1, empty out map. One more K element and the step is a dot:
    # D_linear65
    _gather("G_scalar64", [(101, 64)], [(101, 64)], [], 1, 1, 64,
            "GK_SMALLK_P2", 1),
    # K = 1, empty K map
    _gather("G_outer", [(1, 5)], [(201, 6)], [1, 201], 5, 6, 1, "GK_SMALLK",
            1),
    # A = rows 0, 2, 4 and columns 1..2 of a [6, 4] buffer: source strides
    # that are not suffix products
    _gather("G_strided", [(1, 3), (101, 2)], [(101, 2), (201, 5)], [1, 201],
            3, 5, 2, "GK_SMALLK", 1, a_strides=(8, 1), a_offset=1,
            a_base=24),
    # the table kernel: 2^26 output elements over 26 axes, 8 passes of its
    # capped grid, bits 24-25 of the index go to table 3
    _gather("G_tbl", _Q26, _GATE, _Q26_OUT, 1 << 24, 4, 4, "GK_SMALLK_TBL",
            32768, big=True),
    # nout = 33 648 691 > 2^25: second pass of the div/mod variant
    _gather("G_pass2_np2", [(1, 8209)], [(201, 4099)], [1, 201], 8209, 4099,
            1, "GK_SMALLK", 131072, dtypes=("c64",), big=True),
    # nout = 2^26 but only 2 axes: second pass of the shift/mask variant,
    # not the table
    _gather("G_pass2_p2", [(1, 8192)], [(201, 8192)], [1, 201], 8192, 8192,
            1, "GK_SMALLK_P2", 131072, dtypes=("c64",), big=True),
]

# the unpack of a 33.6 M element GEMM result through k_permute_ct<false>:
# second pass of its grid-stride loop
R_UNPACK_PASS2 = dict(
    name="R_unpack_pass2", group="packs", dtypes=("c64",), env={},
    engine=False, big=True,
    a=[(1, 8209), (101, 16)], b=[(101, 16), (201, 4099)], out=[201, 1],
    plan=dict(NO_PERM, route="ROUTE_TTGT", kind=3, kernel="GEMM_MFMA",
              m=8209, k=16, n=4099, splitk=1, kchunk=16, pack_a=0, pack_b=0,
              perm_out=1, gather_kernel="GK_SMALLK", gather_blocks=131072,
              dot_form="DOT_LINEAR"))

CASES = (GEMM_CASES + [R_PACKS, R_UNPACK_PASS2] + TPERM_CASES + [P_SUBBOX]
         + DOT_CASES + GATHER_CASES)

# every (case, dtype) pair, for pytest.mark.parametrize
PAIRS = [(c, d) for c in CASES for d in c["dtypes"]]
PAIR_IDS = ["%s-%s" % (c["name"], d) for c, d in PAIRS]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def plan_args(case):
    """Positional arguments of hiplib.plan_step for the case."""
    dims = dict(case["a"] + case["b"])
    return [list(case["out"]), [dims[l] for l in case["out"]],
            [l for l, _ in case["a"]], [d for _, d in case["a"]],
            [l for l, _ in case["b"]], [d for _, d in case["b"]]]


def plan_kwargs(case):
    """Keyword arguments of hiplib.plan_step the case adds (its strides)."""
    if "a_strides" in case:
        return {"a_strides": list(case["a_strides"])}
    return {}


def nout_of(case):
    dims = dict(case["a"] + case["b"])
    n = 1
    for l in case["out"]:
        n *= dims[l]
    return n


def expected_plan(case, dtype):
    """The expected plan of one dtype: tuples resolved, names kept."""
    x = 0 if dtype == "c128" else 1
    return {f: (v[x] if isinstance(v, tuple) else v)
            for f, v in case["plan"].items()}


def plan_mismatches(case, dtype, got, consts):
    """Differences between a planned step and the table. `got` maps field ->
    value (a dict, or anything with the fields as attributes); `consts` is
    the namespace holding ROUTE_* / GEMM_* / DOT_* (tnc_amd.hiplib)."""
    get = got.get if isinstance(got, dict) else lambda f: getattr(got, f)
    bad = []
    for f, want in expected_plan(case, dtype).items():
        if isinstance(want, str):
            want = getattr(consts, want)
        if get(f) != want:
            bad.append("%s: %s = %r, expected %r" % (case["name"], f, get(f),
                                                     want))
    if get("kernel") == consts.GEMM_C128_3M:
        bad.append("%s: plans as the 3M kernel" % case["name"])
    if case["plan"].get("splitk", 1) > 1:
        last = get("k") - (get("splitk") - 1) * get("kchunk")
        if last != LAST_SLICE[case["name"]]:
            bad.append("%s: last split-K slice %d, expected %d"
                       % (case["name"], last, LAST_SLICE[case["name"]]))
    return bad


# length of the last split-K slice, k - (splitk - 1) * kchunk, of every split
# case: short (and, for the guarded kernels, with a K-tail inside it) where
# the shape was chosen for that, full for the exact cases
LAST_SLICE = {"v1_split": 31, "rag_split": 31, "pure_split": 32,
              "T1_interleave": 64, "T1_reverse": 64, "T1_block": 64,
              "T1_lowfixed": 64, "T1_mixed": 64, "T2_packB": 64}
