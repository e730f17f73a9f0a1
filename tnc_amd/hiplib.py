"""ctypes binding of the tnc_hip C ABI (include/tnc_hip.h).

The product path fails loudly: importing this module without the built
library, or calling compute without a GPU, raises — there is no CPU
fallback anywhere in tnc_amd.
"""

from __future__ import annotations

import ctypes
import os

import numpy as np

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libtnc_hip.so")

_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"tnc_hip library not built: {_LIB_PATH} missing. "
                "Run `python -c 'import __graft_entry__; __graft_entry__.build()'`."
            )
        L = ctypes.CDLL(_LIB_PATH)
        u64p = ctypes.POINTER(ctypes.c_uint64)
        i64p = ctypes.POINTER(ctypes.c_int64)
        L.tn_last_error.restype = ctypes.c_char_p
        L.tn_device_count.restype = ctypes.c_int
        L.tn_set_device.argtypes = [ctypes.c_int]
        L.tn_einsum_c128.restype = ctypes.c_int
        L.tn_einsum_c128.argtypes = [
            u64p, u64p, ctypes.c_size_t,
            u64p, u64p, i64p, ctypes.c_void_p, ctypes.c_size_t,
            u64p, u64p, i64p, ctypes.c_void_p, ctypes.c_size_t,
            ctypes.c_void_p,
        ]
        L.tn_einsum_c128_dev.restype = ctypes.c_int
        L.tn_einsum_c128_dev.argtypes = [
            u64p, u64p, ctypes.c_size_t,
            u64p, u64p, i64p, ctypes.c_void_p, ctypes.c_size_t,
            u64p, u64p, i64p, ctypes.c_void_p, ctypes.c_size_t,
            ctypes.c_void_p, ctypes.c_void_p,
        ]
        L.tn_einsum_c64.restype = ctypes.c_int
        L.tn_einsum_c64.argtypes = L.tn_einsum_c128.argtypes
        L.tn_einsum_c64_dev.restype = ctypes.c_int
        L.tn_einsum_c64_dev.argtypes = L.tn_einsum_c128_dev.argtypes
        L.tn_net_create2.restype = ctypes.c_void_p
        L.tn_net_create2.argtypes = [ctypes.c_int, ctypes.c_int]
        L.tn_net_create.restype = ctypes.c_void_p
        L.tn_net_create.argtypes = [ctypes.c_int]
        L.tn_net_reserve.restype = ctypes.c_int
        L.tn_net_reserve.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        L.tn_net_add_leaf.restype = ctypes.c_int64
        L.tn_net_add_leaf.argtypes = [
            ctypes.c_void_p, u64p, u64p, ctypes.c_size_t, ctypes.c_void_p,
        ]
        L.tn_net_add_leaf_dev.restype = ctypes.c_int64
        L.tn_net_add_leaf_dev.argtypes = [
            ctypes.c_void_p, u64p, u64p, ctypes.c_size_t, ctypes.c_void_p,
        ]
        L.tn_net_contract.restype = ctypes.c_int
        L.tn_net_contract.argtypes = [
            ctypes.c_void_p, u64p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double),
        ]
        L.tn_net_contract_profiled.restype = ctypes.c_int
        L.tn_net_contract_profiled.argtypes = [
            ctypes.c_void_p, u64p, ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
            ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double),
        ]
        L.tn_memcpy_dtod.restype = ctypes.c_int
        L.tn_memcpy_dtod.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
        ]
        L.tn_memcpy_dtoh.restype = ctypes.c_int
        L.tn_memcpy_dtoh.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
        ]
        L.tn_net_result_meta.restype = ctypes.c_int
        L.tn_net_result_meta.argtypes = [
            ctypes.c_void_p, u64p, u64p, ctypes.POINTER(ctypes.c_size_t),
        ]
        L.tn_net_result_data.restype = ctypes.c_int
        L.tn_net_result_data.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.tn_net_result_dev.restype = ctypes.c_void_p
        L.tn_net_result_dev.argtypes = [ctypes.c_void_p]
        L.tn_net_pool_bytes.restype = ctypes.c_int
        L.tn_net_pool_bytes.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
            ctypes.POINTER(ctypes.c_uint64),
        ]
        L.tn_net_replay_state.restype = ctypes.c_int
        L.tn_net_replay_state.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32),
            ctypes.POINTER(ctypes.c_int32),
        ]
        L.tn_net_destroy.argtypes = [ctypes.c_void_p]
        L.tn_plan_step.restype = ctypes.c_int
        L.tn_plan_step.argtypes = [
            ctypes.c_int, u64p, u64p, ctypes.c_size_t,
            u64p, u64p, i64p, ctypes.c_size_t,
            u64p, u64p, i64p, ctypes.c_size_t,
            ctypes.c_int, ctypes.POINTER(StepPlan),
        ]
        L.tn_plan_layouts.restype = ctypes.c_int
        L.tn_plan_layouts.argtypes = [
            ctypes.c_int, u64p, u64p, u64p, ctypes.c_size_t,
            u64p, ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_int32), u64p,
        ]
        L.tn_plan_slices.restype = ctypes.c_int
        L.tn_plan_slices.argtypes = [
            ctypes.c_int, u64p, u64p, u64p, ctypes.c_size_t,
            u64p, ctypes.c_size_t, u64p, ctypes.c_size_t,
            u64p, u64p, u64p,
        ]
        L.tn_net_contract_sliced.restype = ctypes.c_int
        L.tn_net_contract_sliced.argtypes = [
            ctypes.c_void_p, u64p, ctypes.c_size_t, u64p, ctypes.c_size_t,
            u64p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double),
        ]
        L.tn_plan_step_batched.restype = ctypes.c_int
        L.tn_plan_step_batched.argtypes = [
            ctypes.c_int, u64p, u64p, ctypes.c_size_t,
            u64p, u64p, i64p, ctypes.c_size_t,
            u64p, u64p, i64p, ctypes.c_size_t,
            u64p, ctypes.c_size_t,
            ctypes.c_int, ctypes.POINTER(BatchPlan),
        ]
        L.tn_plan_batch_walk.restype = ctypes.c_int
        L.tn_plan_batch_walk.argtypes = [
            ctypes.c_int, u64p, u64p, u64p, ctypes.c_size_t,
            u64p, ctypes.c_size_t, u64p, ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_int32), u64p, u64p, u64p,
        ]
        for name in ("tn_einsum_c128_batched", "tn_einsum_c64_batched"):
            fn = getattr(L, name)
            fn.restype = ctypes.c_int
            fn.argtypes = (L.tn_einsum_c128.argtypes[:-1]
                           + [u64p, ctypes.c_size_t, ctypes.c_void_p])
        for name in ("tn_einsum_c128_batched_dev",
                     "tn_einsum_c64_batched_dev"):
            fn = getattr(L, name)
            fn.restype = ctypes.c_int
            fn.argtypes = (L.tn_einsum_c128_dev.argtypes[:-2]
                           + [u64p, ctypes.c_size_t, ctypes.c_void_p,
                              ctypes.c_void_p])
        L.tn_net_contract_batched.restype = ctypes.c_int
        L.tn_net_contract_batched.argtypes = [
            ctypes.c_void_p, u64p, ctypes.c_size_t, u64p, ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_double),
        ]
        L.tn_plan_sample.restype = ctypes.c_int
        L.tn_plan_sample.argtypes = [
            ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
            ctypes.POINTER(SamplePlan),
        ]
        for name in ("tn_sample_c128_dev", "tn_sample_c64_dev"):
            fn = getattr(L, name)
            fn.restype = ctypes.c_int
            fn.argtypes = [
                ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
            ]
        L.tn_net_sample.restype = ctypes.c_int
        L.tn_net_sample.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_uint64,
            u64p, ctypes.POINTER(ctypes.c_double),
        ]
        _lib = L
    return _lib


class SamplePlan(ctypes.Structure):
    """tn_sample_plan (include/tnc_hip.h): the three launches of a sampling
    call and the workspace tn_net_sample takes."""

    _fields_ = [
        ("chunk", ctypes.c_uint64), ("nchunks", ctypes.c_uint64),
        ("grid_sums", ctypes.c_uint64), ("grid_scan", ctypes.c_uint64),
        ("grid_draw", ctypes.c_uint64), ("ws_bytes", ctypes.c_uint64),
    ]


def plan_sample(n, nshots, dtype="c128") -> SamplePlan:
    """The plan of sampling nshots indices from a tensor of n elements
    (tn_plan_sample). Raises on a refused plan. Needs no GPU."""
    plan = SamplePlan()
    rc = lib().tn_plan_sample(int(n), int(nshots),
                              {"c128": 0, "c64": 1}[dtype],
                              ctypes.byref(plan))
    check(rc, "tn_plan_sample")
    return plan


class StepPlan(ctypes.Structure):
    """tn_step_plan (include/tnc_hip.h): how one einsum step is dispatched."""

    _fields_ = [
        ("m", ctypes.c_uint64), ("n", ctypes.c_uint64), ("k", ctypes.c_uint64),
        ("route", ctypes.c_int32), ("kind", ctypes.c_int32),
        ("dot_form", ctypes.c_int32), ("tbits", ctypes.c_int32),
        ("dot_blocks", ctypes.c_uint64),
        ("gather_ok", ctypes.c_int32),
        ("pack_a", ctypes.c_int32), ("pack_b", ctypes.c_int32),
        ("direct", ctypes.c_int32), ("gather_gemm", ctypes.c_int32),
        ("pipe_p", ctypes.c_int32), ("pipe_npre", ctypes.c_int32),
        ("pipe_kc", ctypes.c_uint64),
        ("row_tiles", ctypes.c_uint64), ("col_tiles", ctypes.c_uint64),
        ("splitk", ctypes.c_uint64), ("kchunk", ctypes.c_uint64),
        ("kernel", ctypes.c_int32),
        ("ws_pack_a", ctypes.c_uint64), ("ws_pack_b", ctypes.c_uint64),
        ("ws_tmp_c", ctypes.c_uint64), ("ws_slices", ctypes.c_uint64),
        ("ws_split", ctypes.c_uint64), ("ws_dot", ctypes.c_uint64),
        ("scatter_out", ctypes.c_int32),
        ("gemm_pipe", ctypes.c_int32),
        ("perm_a", ctypes.c_int32), ("perm_b", ctypes.c_int32),
        ("perm_out", ctypes.c_int32),
        ("pipe_perm_a", ctypes.c_int32), ("pipe_perm_b", ctypes.c_int32),
        ("gather_kernel", ctypes.c_int32), ("gather_blocks", ctypes.c_int32),
    ]


ROUTE_DOT, ROUTE_GATHER, ROUTE_TTGT = 0, 1, 2
DOT_LINEAR, DOT_TILED, DOT_GATHER = 0, 1, 2
(GEMM_V1, GEMM_MFMA, GEMM_C128_GLDS, GEMM_C128_PURE, GEMM_C128_3M,
 GEMM_C128_GATHER, GEMM_C64_PURE) = range(7)
PERM_NONE, PERM_CT, PERM_TILE = 0, 1, 2  # perm_* / pipe_perm_* fields
# gather_kernel: k_einsum_smallk<false> / <true> / _tbl, k_einsum_anyk<false>
# / <true>
(GK_NONE, GK_SMALLK, GK_SMALLK_P2, GK_SMALLK_TBL, GK_ANYK,
 GK_ANYK_P2) = range(6)


def plan_step(out_labels, out_shape, a_labels, a_shape, b_labels, b_shape,
              dtype="c128", has_stream2=False, a_strides=None,
              b_strides=None) -> StepPlan:
    """The dispatch plan of one einsum step (tn_plan_step). Strides are in
    elements; None = contiguous row-major. Needs no GPU."""
    plan = StepPlan()
    rc = lib().tn_plan_step(
        {"c128": 0, "c64": 1}[dtype],
        _u64arr(out_labels), _u64arr(out_shape), len(out_labels),
        _u64arr(a_labels), _u64arr(a_shape),
        None if a_strides is None else _i64arr(a_strides), len(a_labels),
        _u64arr(b_labels), _u64arr(b_shape),
        None if b_strides is None else _i64arr(b_strides), len(b_labels),
        int(has_stream2), ctypes.byref(plan),
    )
    check(rc, "tn_plan_step")
    return plan


class BatchPlan(ctypes.Structure):
    """tn_batch_plan (include/tnc_hip.h): how one batched step is run."""

    _fields_ = [
        ("batch", ctypes.c_uint64), ("cls", ctypes.c_int32),
        ("dispatches", ctypes.c_uint64),
        ("ws_pack_a", ctypes.c_uint64), ("ws_pack_b", ctypes.c_uint64),
        ("elem", StepPlan),
        ("gather_kernel", ctypes.c_int32),
    ]


BATCH_NONE, BATCH_GATHER, BATCH_GEMM, BATCH_LOOP = range(4)


def plan_step_batched(out_labels, out_shape, a_labels, a_shape, b_labels,
                      b_shape, batch_labels, dtype="c128", has_stream2=False,
                      a_strides=None, b_strides=None) -> BatchPlan:
    """The plan of one batched einsum step (tn_plan_step_batched): plan_step
    plus the labels that are kept, not summed, when both operands carry
    them. Needs no GPU."""
    plan = BatchPlan()
    rc = lib().tn_plan_step_batched(
        {"c128": 0, "c64": 1}[dtype],
        _u64arr(out_labels), _u64arr(out_shape), len(out_labels),
        _u64arr(a_labels), _u64arr(a_shape),
        None if a_strides is None else _i64arr(a_strides), len(a_labels),
        _u64arr(b_labels), _u64arr(b_shape),
        None if b_strides is None else _i64arr(b_strides), len(b_labels),
        _u64arr(batch_labels), len(batch_labels),
        int(has_stream2), ctypes.byref(plan),
    )
    check(rc, "tn_plan_step_batched")
    return plan


def plan_batch_walk(leaves, steps, batch_labels, dtype="c128"):
    """The walk plan of tn_net_contract_batched (tn_plan_batch_walk). leaves
    and steps as for plan_layouts. Returns (cls[], out_labels[], ws_bytes[]),
    one entry per step: the TN_BATCH_* class, the labels of the step's output
    in stored order, and the workspace the step asks for beyond its output.
    Raises on a refused plan. Needs no GPU."""
    n = len(steps)
    cls = (ctypes.c_int32 * n)()
    nd = (ctypes.c_uint64 * n)()
    labels = (ctypes.c_uint64 * max(64 * n, 1))()
    ws = (ctypes.c_uint64 * n)()
    rc = lib().tn_plan_batch_walk(
        {"c128": 0, "c64": 1}[dtype],
        _u64arr([l for labs, _ in leaves for l in labs]),
        _u64arr([d for _, dims in leaves for d in dims]),
        _u64arr([len(labs) for labs, _ in leaves]), len(leaves),
        _u64arr([x for p in steps for x in p]), n,
        _u64arr(batch_labels), len(batch_labels), cls, nd, labels, ws,
    )
    check(rc, "tn_plan_batch_walk")
    return (list(cls),
            [[labels[64 * s + x] for x in range(nd[s])] for s in range(n)],
            list(ws))


def plan_layouts(leaves, steps, dtype="c128"):
    """The executor's layout pre-pass (tn_plan_layouts) over a flat
    replace-left path. leaves = [(labels, dims), ...], steps = [(i, j), ...].
    Returns (scatter_out[], inline_pack_bytes[]), one entry per step: whether
    the step stores its output through the scatter epilogue, and the bytes
    it still packs inline on the main stream. Needs no GPU."""
    n = len(steps)
    scatter = (ctypes.c_int32 * n)()
    inline = (ctypes.c_uint64 * n)()
    rc = lib().tn_plan_layouts(
        {"c128": 0, "c64": 1}[dtype],
        _u64arr([l for labels, _ in leaves for l in labels]),
        _u64arr([d for _, dims in leaves for d in dims]),
        _u64arr([len(labels) for labels, _ in leaves]), len(leaves),
        _u64arr([x for p in steps for x in p]), n, scatter, inline,
    )
    check(rc, "tn_plan_layouts")
    return list(scatter), list(inline)


def plan_slices(leaves, steps, slice_labels, dtype="c128"):
    """The slice plan of tn_net_contract_sliced (tn_plan_slices). leaves and
    steps as for plan_layouts. Returns (nassign, reduced_nd[], strides):
    the number of assignments, each leaf's rank without the slice labels,
    and strides[leaf][label], the element stride of each slice label in the
    stored leaf (0 where absent). Assignment t decodes with the first label
    most significant. Raises on a refused plan. Needs no GPU."""
    nl, ns = len(leaves), len(slice_labels)
    nassign = ctypes.c_uint64()
    reduced = (ctypes.c_uint64 * nl)()
    strides = (ctypes.c_uint64 * max(nl * ns, 1))()
    rc = lib().tn_plan_slices(
        {"c128": 0, "c64": 1}[dtype],
        _u64arr([l for labels, _ in leaves for l in labels]),
        _u64arr([d for _, dims in leaves for d in dims]),
        _u64arr([len(labels) for labels, _ in leaves]), nl,
        _u64arr([x for p in steps for x in p]), len(steps),
        _u64arr(slice_labels), ns,
        ctypes.byref(nassign), reduced, strides,
    )
    check(rc, "tn_plan_slices")
    return (nassign.value, list(reduced),
            [[strides[x * ns + y] for y in range(ns)] for x in range(nl)])


def last_error() -> str:
    return lib().tn_last_error().decode()


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {last_error()}")


def device_count() -> int:
    return lib().tn_device_count()


def _u64arr(vals):
    return (ctypes.c_uint64 * len(vals))(*[int(v) for v in vals])


def _i64arr(vals):
    return (ctypes.c_int64 * len(vals))(*[int(v) for v in vals])


def _einsum_host(out_labels, a_labels, a, b_labels, b, out_shape, npdtype,
                 esize, fn_name, batch_labels=None):
    """batch_labels None: the plain entry point; a list (possibly empty): the
    *_batched one, which takes the labels ahead of the out buffer."""
    a = np.asarray(a, dtype=npdtype)
    b = np.asarray(b, dtype=npdtype)
    if out_shape is None:
        dimmap = {}
        for lab, d in zip(a_labels, a.shape):
            dimmap[lab] = d
        for lab, d in zip(b_labels, b.shape):
            dimmap[lab] = d
        out_shape = [dimmap[l] for l in out_labels]
    out = np.empty(tuple(out_shape), dtype=npdtype)
    a_str = [s // esize for s in a.strides]
    b_str = [s // esize for s in b.strides]
    batch = ([] if batch_labels is None
             else [_u64arr(batch_labels), len(batch_labels)])
    rc = getattr(lib(), fn_name)(
        _u64arr(out_labels), _u64arr(out_shape), len(out_labels),
        _u64arr(a_labels), _u64arr(a.shape), _i64arr(a_str),
        a.ctypes.data_as(ctypes.c_void_p), a.ndim,
        _u64arr(b_labels), _u64arr(b.shape), _i64arr(b_str),
        b.ctypes.data_as(ctypes.c_void_p), b.ndim,
        *batch, out.ctypes.data_as(ctypes.c_void_p),
    )
    check(rc, fn_name)
    return out


def einsum_batched_c128(out_labels, a_labels, a: np.ndarray, b_labels,
                        b: np.ndarray, batch_labels,
                        out_shape=None) -> np.ndarray:
    """einsum_c128 with batch labels (tn_einsum_c128_batched): a label of
    batch_labels carried by both operands is kept in out, not summed, and
    those labels lead out_labels. Accepts non-contiguous views."""
    return _einsum_host(out_labels, a_labels, a, b_labels, b, out_shape,
                        np.complex128, 16, "tn_einsum_c128_batched",
                        list(batch_labels))


def einsum_batched_c64(out_labels, a_labels, a: np.ndarray, b_labels,
                       b: np.ndarray, batch_labels,
                       out_shape=None) -> np.ndarray:
    """complex64 batched einsum (tn_einsum_c64_batched)."""
    return _einsum_host(out_labels, a_labels, a, b_labels, b, out_shape,
                        np.complex64, 8, "tn_einsum_c64_batched",
                        list(batch_labels))


def einsum_c128(out_labels, a_labels, a: np.ndarray, b_labels, b: np.ndarray,
                out_shape=None) -> np.ndarray:
    """Host-buffer einsum via the GPU (tn_einsum_c128): the direct
    tblis::tensor_mult parity entry point. Accepts non-contiguous views
    (strides forwarded in elements)."""
    return _einsum_host(out_labels, a_labels, a, b_labels, b, out_shape,
                        np.complex128, 16, "tn_einsum_c128")


def einsum_c64(out_labels, a_labels, a: np.ndarray, b_labels, b: np.ndarray,
               out_shape=None) -> np.ndarray:
    """complex64 einsum via the GPU (tn_einsum_c64, f32 MFMA path)."""
    return _einsum_host(out_labels, a_labels, a, b_labels, b, out_shape,
                        np.complex64, 8, "tn_einsum_c64")
