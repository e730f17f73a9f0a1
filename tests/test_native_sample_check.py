"""The stand-alone host check of the sampling plan and pick rules
(tests/native/sample_plan_check.cpp), built with the host sanitizers and run
the way test_native_checks.py builds and runs its programs: one translation
unit with its own main that includes only step_plan.hpp, no GPU, nothing
loaded into Python. Where the sanitizer runtime cannot be linked the same
file is built without it, so the check itself always runs.
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


def test_sample_plan_check(tmp_path):
    exe = build("sample_plan_check", tmp_path)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TN_")}
    proc = subprocess.run([exe], env=env, capture_output=True, text=True,
                          timeout=600)
    assert proc.returncode == 0, (proc.stdout, proc.stderr)
    assert "sample_plan_check OK" in proc.stdout, (proc.stdout, proc.stderr)
