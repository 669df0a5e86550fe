"""Syntax / layout hygiene of the reference-side binding, adapters/opencv/loop_closing.cpp.

The adapter defines the members that the reference's own header declares (include/loop_closing.hpp:31-66) on top of the
C ABI.  OpenCV is not in this image, so it cannot be BUILT here; this test runs `g++ -fsyntax-only` on it against the
reference's real header and tests/stubs/opencv2/*.hpp (declarations of the few cv:: names involved).  That catches
typos, signature drift against the header and lcm.h, and the static_asserts on cv::DMatch / LoopCandidate layout.
It pins NO behaviour: nothing is linked or run, and the stubs are not OpenCV.
The reference's header is not part of this repository: build() precompiles it into oracle/_ref/include/ (oracle/Makefile,
target `ref`), and GCC reads that precompiled header where the adapter includes "loop_closing.hpp"."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_INC = os.path.join(ROOT, "oracle", "_ref", "include")


def _compiler():
    r = subprocess.run(["g++", "--version"], capture_output=True, text=True)
    return r.stdout.splitlines()[0].strip() if r.returncode == 0 and r.stdout else None


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_adapter_is_valid_cxx_against_the_reference_header():
    if not os.path.exists(os.path.join(REF_INC, "loop_closing.hpp.gch")):
        pytest.skip("build() found no reference checkout: oracle/_ref/include/loop_closing.hpp.gch was not built")
    built_by = open(os.path.join(REF_INC, "compiler.txt")).read().strip()
    if built_by != _compiler():
        pytest.skip(f"the reference header was precompiled by another compiler ({built_by})")
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Winvalid-pch",
           "-I", os.path.join(ROOT, "tests", "stubs"), "-I", REF_INC, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "adapters", "opencv", "loop_closing.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]


def test_adapter_defines_every_hot_path_member_of_the_header():
    src = open(os.path.join(ROOT, "adapters", "opencv", "loop_closing.cpp")).read()
    for member in ("LoopClosingSystem::LoopClosingSystem(", "LoopClosingSystem::processFrame(", "LoopClosingSystem::detectFeatures(",
                   "LoopClosingSystem::matchFeatures(", "LoopClosingSystem::detectLoops(", "LoopClosingSystem::saveResults("):
        assert member in src, member
