"""TN_GEMM3M_PIPE in the step planner (no GPU): gemm_pipe follows the 3M
route and the switch. The switch is read once: one child process per setting.
"""

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys
from tnc_amd import hiplib
out = {}
for name, (m, k, n) in json.loads(sys.argv[1]).items():
    p = hiplib.plan_step([1, 20], [m, n], [1, 10], [m, k], [10, 20], [k, n])
    out[name] = {f: getattr(p, f) for f, _ in p._fields_}
print("PLAN " + json.dumps(out))
"""

SHAPES = {
    "gated": (2048, 32, 1024),   # 256 tiles, K = 32: the smallest admitted
    "below": (2048, 32, 512),    # 128 tiles: stays on the 4M kernel
    "ragged": (2048, 40, 1024),  # K % 16 != 0: never 3M
}


def plans(env_extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("TN_GEMM3M", "TN_GEMM3M_PIPE", "TN_GATHER_GEMM")}
    env.update(env_extra)
    proc = subprocess.run([sys.executable, "-c", CHILD, json.dumps(SHAPES)],
                          cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=120)
    assert proc.returncode == 0, (proc.stdout, proc.stderr)
    line = [l for l in proc.stdout.splitlines() if l.startswith("PLAN ")][-1]
    return json.loads(line[5:])


def test_pipe_is_the_default_on_the_3m_route_only():
    from tnc_amd import hiplib as H

    p = plans({})
    assert p["gated"]["kernel"] == H.GEMM_C128_3M
    assert p["gated"]["gemm_pipe"] == 1
    for name in ("below", "ragged"):
        assert p[name]["kernel"] != H.GEMM_C128_3M
        assert p[name]["gemm_pipe"] == 0


def test_pipe_switch_off_keeps_the_route():
    from tnc_amd import hiplib as H

    on, off = plans({}), plans({"TN_GEMM3M_PIPE": "0"})
    assert off["gated"]["kernel"] == H.GEMM_C128_3M
    assert off["gated"]["gemm_pipe"] == 0
    for name in SHAPES:
        a, b = dict(on[name]), dict(off[name])
        a.pop("gemm_pipe"), b.pop("gemm_pipe")
        assert a == b


def test_pipe_follows_forced_3m_and_gemm3m_off():
    from tnc_amd import hiplib as H

    p = plans({"TN_GEMM3M": "force"})
    assert p["below"]["kernel"] == H.GEMM_C128_3M
    assert p["below"]["gemm_pipe"] == 1
    assert p["ragged"]["gemm_pipe"] == 0
    p = plans({"TN_GEMM3M": "0"})
    assert all(v["gemm_pipe"] == 0 for v in p.values())
