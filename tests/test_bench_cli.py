"""bench.py command line: a plain run emits only the headline line,
--steps sets the timed step count, and --dump-outputs writes the final
tensor of the timed path (deterministic, capped by a fixed seeded sample).
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_bench(monkeypatch):
    import importlib.util

    # bench.py defaults the BLAS thread caps at import; keep that out of
    # the rest of the session's environment
    for k in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS"):
        monkeypatch.setenv(k, os.environ.get(k, "1"))

    spec = importlib.util.spec_from_file_location(
        "tnc_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_roundtrip_and_dtype(tmp_path, monkeypatch):
    bench = _load_bench(monkeypatch)
    rng = np.random.default_rng(3)
    z = rng.standard_normal((3, 5)) + 1j * rng.standard_normal((3, 5))
    bench.dump_outputs(str(tmp_path / "c128"), z)
    got = np.load(tmp_path / "c128" / "result.npy")
    assert got.dtype == np.float64 and got.shape == (3, 5, 2)
    np.testing.assert_array_equal(got[..., 0] + 1j * got[..., 1], z)
    bench.dump_outputs(str(tmp_path / "c64"), z.astype(np.complex64))
    got = np.load(tmp_path / "c64" / "result.npy")
    assert got.dtype == np.float32 and got.shape == (3, 5, 2)


def test_dump_outputs_sample_is_capped_and_fixed(tmp_path, monkeypatch):
    bench = _load_bench(monkeypatch)
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 1024)
    z = (np.arange(4096) + 1j * np.arange(4096)).reshape(64, 64)
    bench.dump_outputs(str(tmp_path / "a"), z)
    bench.dump_outputs(str(tmp_path / "b"), z)
    a = np.load(tmp_path / "a" / "result.npy")
    b = np.load(tmp_path / "b" / "result.npy")
    assert a.nbytes <= 1024 and a.shape == (64, 2)
    np.testing.assert_array_equal(a, b)
    # sampled rows are genuine elements of the output
    np.testing.assert_array_equal(a[:, 0], a[:, 1])


@pytest.mark.gpu
def test_plain_run_headline_only_and_dump_matches_oracle(tmp_path):
    from oracle import contract_network
    from oracle.adapters import network_to_otensors
    from tnc_amd.fixtures import load_fixture

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
           "--steps", "2", "--warmup", "1", "--fixture", "rqc24",
           "--dump-outputs", str(tmp_path)]
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True,
                          timeout=240)
    assert proc.returncode == 0, (proc.stdout[-2000:], proc.stderr[-2000:])
    lines = [json.loads(l) for l in proc.stdout.splitlines()
             if l.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]
    d = lines[0]
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0 and d["value"] > 0
    assert d["dtype"] == "c128" and d["higher_is_better"] is True
    # the legs that take runs of their own are --full only
    assert d["roofline"] is None and d["cpu_baseline"] is None
    assert "secondary" not in d

    got = np.load(tmp_path / "result.npy")
    assert got.dtype == np.float64 and got.shape[-1] == 2
    tn, rp, _ = load_fixture("rqc24")
    ref = np.atleast_1d(contract_network(network_to_otensors(tn), rp).data)
    np.testing.assert_allclose(
        (got[..., 0] + 1j * got[..., 1]).reshape(-1), ref.reshape(-1),
        rtol=1e-10)
