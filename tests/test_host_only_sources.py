"""Every .cpp of the library is host-only: a host compiler takes it with no ROCm directory on the include path.

The planners, the tier choice and the layouts (csrc/*_plan.cpp, qp_tier*.cpp, qp_debug.cpp, sqp_*.cpp, qp_polish_plan.cpp) are
kept out of the kernel files so that they can be read, tested and swept under a sanitizer (scripts/sanitize/) without a GPU
or a HIP header.  One include of sco_internal.h -- which pulls in <hip/hip_runtime.h> -- would undo that without anything
else failing; this test fails instead.  Strict warnings: these files are the index arithmetic the kernels follow blindly."""
import os
import shutil
import subprocess

import pytest

from sco_py_amd import _build

CPPS = [s for s in _build.SOURCES if s.endswith(".cpp")]


def test_the_planners_are_among_them():
    for name in ("qp_plan.cpp", "qp_tier.cpp", "qp_tier_choice.cpp", "qp_debug.cpp", "rl_plan.cpp", "wv_plan.cpp", "big_plan.cpp",
                 "reg_fast_plan.cpp", "sqp_sched.cpp", "sqp_layout.cpp"):
        assert name in CPPS


@pytest.mark.parametrize("src", CPPS)
def test_compiles_without_hip(src):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", src], cwd=_build.CSRC,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_kernel_file_holds_a_planner():
    """No .hip file defines a function that takes a QpPlan and fills a host plan, and none but the two launch-time reads
    (SCO_QP_BT_TRIPLE in big_launch, SCO_WV_ABLATE in wv_fill_args) touches the environment."""
    reads = {}
    for s in _build.SOURCES:
        if not s.endswith(".hip"):
            continue
        with open(os.path.join(_build.CSRC, s)) as f:
            text = f.read()
        assert "const QpPlan &pl," not in text, s
        n = text.count("getenv(")
        if n:
            reads[s] = n
    assert reads == {"sco_qp_big.hip": 1, "sco_admm_wv.hip": 1}
    for s in ("rl_plan.cpp", "wv_plan.cpp", "big_plan.cpp", "reg_fast_plan.cpp", "qp_tier_choice.cpp", "qp_debug.cpp", "qp_plan.cpp"):
        with open(os.path.join(_build.CSRC, s)) as f:
            assert "getenv" not in f.read(), s
