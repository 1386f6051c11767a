"""The step plan (csrc/step_plan.h) keeps the step invariant: no GPU, no HIP.

cpu/step_plan_check.cpp enumerates every StepFacts combination, checks on each
accepted plan that the draw counter advances once, the update is applied once,
the bookkeeping happens once and the next draw follows the advance, and pins
the plans of the regimes the GPU tests run against a literal table.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "distributed-deep-q_amd", "cpu", "step_plan_check.cpp")


def test_step_plan_invariant(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "step_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "step plan ok" in r.stdout


def test_step_plan_header_is_plain_cxx():
    """The header compiles alone: nothing of HIP in it."""
    hdr = os.path.join(ROOT, "distributed-deep-q_amd", "csrc", "step_plan.h")
    assert "#include" not in open(hdr).read()
