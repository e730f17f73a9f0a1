"""Batched einsum on the GPU (tn_einsum_*_batched): every class of
tn_plan_step_batched, each case asserting through the planner that it reaches
the class it means to, then checking values against np.einsum in complex128.
The shapes are the smallest at which each path can go wrong."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BETA, GAMMA = 50, 51
TOL = {"c128": dict(rtol=1e-12, atol=1e-10), "c64": dict(rtol=2e-3, atol=1e-4)}
NPDT = {"c128": np.complex128, "c64": np.complex64}


def rand(shape, seed, dtype):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return x.astype(NPDT[dtype])


def ref_einsum(out_labels, a_labels, a, b_labels, b):
    """np.einsum in complex128; labels remapped (numpy refuses integer
    subscripts >= 52). Labels in out are kept, the rest summed."""
    ids = {}
    for l in list(a_labels) + list(b_labels):
        ids.setdefault(l, len(ids))
    return np.einsum(a.astype(np.complex128), [ids[l] for l in a_labels],
                     b.astype(np.complex128), [ids[l] for l in b_labels],
                     [ids[l] for l in out_labels])


def gpu_einsum(dtype, batched):
    from tnc_amd import hiplib as H

    if batched:
        return H.einsum_batched_c128 if dtype == "c128" else H.einsum_batched_c64
    return H.einsum_c128 if dtype == "c128" else H.einsum_c64


def planned(dtype, out_labels, a_labels, a, b_labels, b, batch):
    from tnc_amd import hiplib as H

    dims = dict(zip(a_labels, a.shape))
    dims.update(zip(b_labels, b.shape))
    return H.plan_step_batched(
        out_labels, [dims[l] for l in out_labels], a_labels, a.shape,
        b_labels, b.shape, batch, dtype=dtype,
        a_strides=[s // a.itemsize for s in a.strides],
        b_strides=[s // b.itemsize for s in b.strides])


def run_case(dtype, want_cls, out_labels, a_labels, a, b_labels, b, batch):
    p = planned(dtype, out_labels, a_labels, a, b_labels, b, batch)
    assert p.cls == want_cls, (p.cls, want_cls)
    got = gpu_einsum(dtype, True)(out_labels, a_labels, a, b_labels, b, batch)
    ref = ref_einsum(out_labels, a_labels, a, b_labels, b)
    assert got.dtype == NPDT[dtype] and got.shape == ref.shape
    print(dtype, "class", p.cls, "batch", p.batch, "max abs err",
          np.max(np.abs(got - ref)))
    np.testing.assert_allclose(got, ref, **TOL[dtype])
    return p, got


def rows_unbatched(dtype, out_labels, a_labels, a, b_labels, b, nbeta):
    """The unbatched einsum of every row of beta (leading in a, b and out)."""
    fn = gpu_einsum(dtype, False)
    return np.stack([
        fn(out_labels[1:], a_labels[1:], np.ascontiguousarray(a[r]),
           b_labels[1:], np.ascontiguousarray(b[r])) for r in range(nbeta)])


# ---- gather class ----------------------------------------------------------

@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_gather_gate_apply(dtype):
    from tnc_amd import hiplib as H

    a, b = rand((3, 2, 2), 1, dtype), rand((3, 2, 2), 2, dtype)
    p, _ = run_case(dtype, H.BATCH_GATHER, [BETA, 1, 2], [BETA, 1, 3], a,
                    [BETA, 3, 2], b, [BETA])
    assert p.dispatches == 1
    # batch 3 leads the out map: the one launch is the div/mod kernel, though
    # an element alone would take the shift/mask one
    assert p.gather_kernel == H.GK_SMALLK
    assert p.elem.gather_kernel == H.GK_SMALLK_P2


@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_gather_gate_apply_batch4(dtype):
    """A pow2 batch keeps the launch on the shift/mask kernel."""
    from tnc_amd import hiplib as H

    a, b = rand((4, 2, 2), 9, dtype), rand((4, 2, 2), 10, dtype)
    p, _ = run_case(dtype, H.BATCH_GATHER, [BETA, 1, 2], [BETA, 1, 3], a,
                    [BETA, 3, 2], b, [BETA])
    assert p.dispatches == 1 and p.batch == 4
    assert p.gather_kernel == H.GK_SMALLK_P2
    assert p.elem.gather_kernel == H.GK_SMALLK_P2


@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_gather_outer_product(dtype):
    from tnc_amd import hiplib as H

    a, b = rand((3, 4), 3, dtype), rand((3, 5), 4, dtype)
    p, _ = run_case(dtype, H.BATCH_GATHER, [BETA, 1, 2], [BETA, 1], a,
                    [BETA, 2], b, [BETA])
    assert p.elem.k == 1
    assert p.gather_kernel == H.GK_SMALLK


@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_gather_nonpow2_and_out_order(dtype):
    from tnc_amd import hiplib as H

    a, b = rand((3, 3, 5), 5, dtype), rand((5, 3, 6), 6, dtype)
    # beta in the middle of B; out keeps the N leg ahead of the M leg
    p, _ = run_case(dtype, H.BATCH_GATHER, [BETA, 2, 1], [BETA, 1, 3], a,
                    [3, BETA, 2], b, [BETA])
    assert p.gather_kernel == H.GK_SMALLK


@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_gather_strided_view(dtype):
    from tnc_amd import hiplib as H

    base = rand((3, 6, 4), 7, dtype)
    a = base[:, ::2, 1:3]  # [3, 3, 2], element strides (24, 8, 1)
    assert not a.flags["C_CONTIGUOUS"]
    b = rand((3, 2, 5), 8, dtype)
    p, _ = run_case(dtype, H.BATCH_GATHER, [BETA, 1, 2], [BETA, 1, 3], a,
                    [BETA, 3, 2], b, [BETA])
    assert p.gather_kernel == H.GK_SMALLK


# ---- GEMM class ------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_gemm_ragged_and_no_cross_talk(dtype):
    """One past a fragment (M=17), one past a tile (N=65), K no multiple of
    4; each row also against the unbatched einsum of that row."""
    from tnc_amd import hiplib as H

    a, b = rand((3, 17, 67), 10, dtype), rand((3, 67, 65), 11, dtype)
    labels = ([BETA, 1, 2], [BETA, 1, 3], [BETA, 3, 2])
    p, got = run_case(dtype, H.BATCH_GEMM, labels[0], labels[1], a, labels[2],
                      b, [BETA])
    assert p.dispatches == 1 and p.ws_pack_a == 0 and p.ws_pack_b == 0
    rows = rows_unbatched(dtype, labels[0], labels[1], a, labels[2], b, 3)
    np.testing.assert_allclose(got, rows, **TOL[dtype])


@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_gemm_min_fragment_two_batch_labels(dtype):
    from tnc_amd import hiplib as H

    a = rand((2, 3, 16, 68), 12, dtype)
    b = rand((2, 3, 68, 16), 13, dtype)
    p, _ = run_case(dtype, H.BATCH_GEMM, [BETA, GAMMA, 1, 2],
                    [BETA, GAMMA, 1, 3], a, [BETA, GAMMA, 3, 2], b,
                    [GAMMA, BETA])
    assert p.batch == 6 and p.ws_pack_a == 0 and p.ws_pack_b == 0


@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_gemm_exact_tile(dtype):
    from tnc_amd import hiplib as H

    a, b = rand((5, 64, 80), 14, dtype), rand((5, 80, 64), 15, dtype)
    p, _ = run_case(dtype, H.BATCH_GEMM, [BETA, 1, 2], [BETA, 1, 3], a,
                    [BETA, 3, 2], b, [BETA])
    assert p.batch == 5


@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_gemm_both_packs_and_out_permute(dtype):
    """A stored [M][beta][K], B stored [N legs][K][beta], out asked for as
    [beta][N legs][M]: two batched packs and the out permute."""
    from tnc_amd import hiplib as H

    esize = 16 if dtype == "c128" else 8
    a = rand((17, 3, 67), 16, dtype)
    b = rand((5, 13, 67, 3), 17, dtype)
    p, _ = run_case(dtype, H.BATCH_GEMM, [BETA, 20, 21, 1], [1, BETA, 3], a,
                    [20, 21, 3, BETA], b, [BETA])
    assert p.ws_pack_a == 3 * 17 * 67 * esize
    assert p.ws_pack_b == 3 * 67 * 65 * esize
    assert not p.elem.direct


# ---- LOOP class ------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["c128", "c64"])
@pytest.mark.parametrize("m,k", [(32, 256), (1, 100)])
def test_loop_rows_bit_equal(dtype, m, k):
    """The element step on offset views: the same kernel on the same data as
    the unbatched einsum of each row, so the rows agree bit for bit."""
    from tnc_amd import hiplib as H

    a, b = rand((3, m, k), 18, dtype), rand((3, k, m), 19, dtype)
    labels = ([BETA, 1, 2], [BETA, 1, 3], [BETA, 3, 2])
    p, got = run_case(dtype, H.BATCH_LOOP, labels[0], labels[1], a, labels[2],
                      b, [BETA])
    assert p.dispatches == 3
    assert (p.elem.splitk == 4) if m == 32 else (p.elem.route == H.ROUTE_DOT)
    rows = rows_unbatched(dtype, labels[0], labels[1], a, labels[2], b, 3)
    assert np.array_equal(got, rows)


# ---- the unbatched boundary is where it was --------------------------------

def test_none_class_matches_einsum():
    from tnc_amd import hiplib as H

    a, b = rand((3, 8, 20), 20, "c128"), rand((20, 7), 21, "c128")
    labels = ([BETA, 1, 2], [BETA, 1, 3], [3, 2])
    _, got = run_case("c128", H.BATCH_NONE, labels[0], labels[1], a, labels[2],
                      b, [BETA])
    plain = H.einsum_c128(labels[0], labels[1], a, labels[2], b)
    assert np.array_equal(got, plain)
    with pytest.raises(RuntimeError, match="batch labels must lead out"):
        H.einsum_batched_c128([1, BETA, 2], [BETA, 1, 3], a,
                              [BETA, 3, 2], rand((3, 20, 7), 22, "c128"),
                              [BETA])
