"""The stand-alone host checks under tests/native, built with the host
sanitizers and run (no GPU, nothing loaded into Python):

  layout_plan_check  scatter-epilogue gate and addressing, walk plan
                     (also with TN_EPI_SCATTER=0)
  slice_plan_check   slice plan
  tile_perm_check    address replay of k_permute_tile and k_dot_tile, with
                     self-tests that fail when a plan entry is perturbed
  gather_map_check   both encodings of the gather maps against a mixed-radix
                     loop, the four offset tables of k_einsum_smallk_tbl,
                     plan_gather_kernel at its thresholds, with self-tests
                     that fail when a shift, mask or table entry is perturbed

Each is one translation unit with its own main that includes only
step_plan.hpp. Where the sanitizer runtime cannot be linked the same file is
built without it, so the checks themselves always run.
"""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
BASE = ["-std=c++17", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None,
                                reason="no g++")


def build(name, tmp_path):
    """Sanitized build; the plain one where that does not compile and link."""
    src = os.path.join(NATIVE, name + ".cpp")
    exe = str(tmp_path / name)
    errs = []
    for flags in (BASE + SANITIZE, BASE):
        proc = subprocess.run(["g++", *flags, src, "-o", exe],
                              capture_output=True, text=True, timeout=600)
        if proc.returncode == 0:
            return exe
        errs.append(proc.stderr)
    raise AssertionError("g++ failed on %s:\n%s" % (name, "\n".join(errs)))


def run(exe, env_extra=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TN_")}
    env.update(env_extra or {})
    return subprocess.run([exe], env=env, capture_output=True, text=True,
                          timeout=600)


@pytest.mark.parametrize("name,env,ok_line", [
    ("layout_plan_check", {}, "layout_plan_check OK (scatter on)"),
    ("layout_plan_check", {"TN_EPI_SCATTER": "0"},
     "layout_plan_check OK (scatter off)"),
    ("slice_plan_check", {}, "slice_plan_check OK"),
    ("tile_perm_check", {}, "tile_perm_check OK"),
    ("gather_map_check", {}, "gather_map_check OK"),
], ids=["layout", "layout_scatter_off", "slice", "tile_perm", "gather_map"])
def test_native_check(name, env, ok_line, tmp_path):
    proc = run(build(name, tmp_path), env)
    assert proc.returncode == 0, (proc.stdout, proc.stderr)
    assert ok_line in proc.stdout, (proc.stdout, proc.stderr)
