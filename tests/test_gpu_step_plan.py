"""The executor takes the route the planner reports.

Each route-table case of tests/test_step_plan.py that a two-leaf network can
reach is contracted on the GPU: the `kind` a profiled run returns must be
the planner's, and the result must match the oracle at the c128 bar of
tests/test_gpu_einsum.py (rtol 1e-12, atol 1e-10).
"""

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

M_, N_, K_, K2_ = 1, 2, 3, 4

CASES = {
    # name: (A legs, A dims, B legs, B dims)
    "dot_linear": ([K_], [128], [K_], [128]),
    "dot_gather": ([K_, K2_], [8, 16], [K2_, K_], [16, 8]),
    "dot_tiled": ([K_, K2_], [1024, 1024], [K2_, K_], [1024, 1024]),
    "gather_smallk": ([M_, K_], [8, 4], [K_, N_], [4, 8]),
    "gather_skinny": ([M_, K_], [4, 128], [K_, N_], [128, 64]),
    "v1": ([M_, K_], [16, 128], [K_, N_], [128, 16]),
    "c128_pure": ([M_, K_], [128, 16], [K_, N_], [16, 64]),
    "c128_glds": ([M_, K_], [40, 72], [K_, N_], [72, 40]),
    "splitk": ([M_, K_], [128, 4096], [K_, N_], [4096, 64]),
    "c128_3m": ([M_, K_], [2048, 32], [K_, N_], [32, 1024]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kind_matches_plan(name):
    from tnc_amd import hiplib
    from tnc_amd.contraction_path import ContractionPath
    from tnc_amd.executor import ContractionEngine
    from tnc_amd.tensor import CompositeTensor, LeafTensor, TensorData

    a_legs, a_dims, b_legs, b_dims = CASES[name]
    rng = np.random.default_rng(list(CASES).index(name))
    a = rng.standard_normal(a_dims) + 1j * rng.standard_normal(a_dims)
    b = rng.standard_normal(b_dims) + 1j * rng.standard_normal(b_dims)
    ta = LeafTensor(a_legs, a_dims)
    ta.set_tensor_data(TensorData(TensorData.MATRIX, matrix=a))
    tb = LeafTensor(b_legs, b_dims)
    tb.set_tensor_data(TensorData(TensorData.MATRIX, matrix=b))
    eng = ContractionEngine(CompositeTensor([ta, tb]),
                            ContractionPath.simple([(0, 1)]))
    try:
        _, _, _, kind = eng.contract_profiled()
        legs, data = eng.result()
        info = eng.infos[0]
    finally:
        eng.close()
    plan = hiplib.plan_step(info.out_legs, info.out_dims, a_legs, a_dims,
                            b_legs, b_dims, has_stream2=True)
    print(name, "kind", kind, "plan kind", plan.kind, "kernel", plan.kernel)
    assert kind == [plan.kind]
    ref = oracle.contract_ndarrays(legs, a_legs, a, b_legs, b)
    np.testing.assert_allclose(data, ref, rtol=1e-12, atol=1e-10)
