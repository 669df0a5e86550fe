"""The geometry stages' shared header (csrc/lcm_geom_device.h) and the sliced launcher (csrc/lcm_kernels.h) without a device: each
shared function and record defined once, there and nowhere else under csrc, with its own fp contract pragma; what they replaced
gone from csrc; the launcher defined once and the only reader of the grid limit in the kernel files; and the header's arithmetic
as a stand-alone program under ASan + UBSan.  Nothing loaded into Python runs under a sanitizer."""
import os
import re
import subprocess

import pytest

import geomsrc as G

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
HIP_INCLUDE = "/opt/rocm/include"          # lcm_geom_device.h includes hip_runtime.h: as plain C++ its markers expand to nothing
# kernel file -> launches through the sliced launcher
SLICED = {"lcm_kernels.hip": 1, "lcm_knn.hip": 1, "lcm_l2.hip": 1, "lcm_l2_emit.hip": 2, "lcm_epi.hip": 3, "lcm_lo.hip": 2, "lcm_pose.hip": 1}


def test_every_shared_function_and_record_exists_once():
    G.assert_defined_once_in_geom(G.SHARED)
    src = G.sources()
    for record in G.RECORDS:
        for f, text in src.items():
            assert text.count(record) == (1 if f == G.GEOM else 0), (record, f)
    for f, text in src.items():
        for old in G.GONE:
            assert not re.search(rf"\b{old}\b", text), (old, f)
    make = src["Makefile"]
    hdrs = re.search(r"^HDRS = (.*)$", make, flags=re.M).group(1).split()
    assert sorted(h for h in hdrs if "/" not in h) == sorted(f for f in src if f.endswith((".h", ".hpp")))      # every header is listed


def test_every_shared_function_states_its_own_rules():
    geom = G.sources()[G.GEOM]
    code = G.strip(geom)
    bodies = re.split(r"\n(?=__host__ __device__ )", code.replace("template <int N>\n", ""))[1:]
    assert len(bodies) == len(G.SHARED)
    for body in bodies:
        head = body[: body.index("{")]
        if "constexpr" in head:                                         # an index: integers only
            assert "double" not in body, head
            continue
        assert "__forceinline__" in head, head
        assert body.count("#pragma clang fp contract(off)") == 1, head  # lexical: a callee does not take it from its caller
        assert not re.search(r"\bfma\b|__fma_rn|float\b", body), head
    assert "namespace lcm {" in code and "atomic" not in code and "asm" not in re.findall(r"\b\w+\b", code)
    # the essential-matrix rotation stays its own, and the header says why
    assert re.search(r"^// lcm_epi_device\.h's rotation stays its own:.*\n__host__ __device__ __forceinline__ bool jacobi_angle\(", geom, flags=re.M)
    epi = G.strip(G.sources()["lcm_epi_device.h"])
    project = epi[epi.index("bool epi_project("):epi.index("bool epi_solve8(")]
    assert "lcm_geom_device.h" not in epi and "jacobi_angle" not in epi and "fp contract" not in project and "zeta * zeta" in project
    pose = G.sources()["lcm_pose_device.h"]
    assert "lcm_geom_device.h" not in pose
    # the feature headers take it from there, the bundle adjustment no longer through the pose graph's
    for f in ("lcm_pgo_device.h", "lcm_ba_device.h", "lcm_map_device.h", "lcm_lo_device.h"):
        assert '#include "lcm_geom_device.h"' in G.sources()[f], f
    assert "lcm_pgo" not in G.sources()["lcm_ba_device.h"]
    # the records' layouts against include/lcm.h are stated once per record, in the .cpp that owns it
    owners = {"lcm::Pose": "lcm_pgo.cpp", "lcm::Point3": "lcm_ba.cpp", "lcm::Observation": "lcm_ba.cpp"}
    for f, text in G.sources().items():
        if f.endswith(".cpp"):
            for record, owner in owners.items():
                assert (f"sizeof({record})" in text) == (f == owner), (record, f)


def test_the_sliced_launcher_exists_once_and_every_sliced_launch_goes_through_it():
    src = G.sources()
    for f, text in src.items():
        assert text.count("hipError_t launch_y_sliced(") == (1 if f == "lcm_kernels.h" else 0), f
        assert "launch_sliced(" not in text, f                          # the file-local copies are gone
        if f.endswith(".hip"):
            code = G.strip(text)
            assert code.count("launch_y_sliced(") == SLICED.get(f, 0), f
            assert text.count("grid_y_limit(") == (1 if f == "lcm_kernels.hip" else 0), f           # its own definition
            assert not re.search(r"\.(?:pair|job)_base\s*\+?=[^=]", code), f                       # no kernel file steps a base itself
    body = src["lcm_kernels.h"]
    body = body[body.index("hipError_t launch_y_sliced("):]
    body = body[: body.index("\n}\n")]
    assert "if (n == 0) return hipSuccess;" in body and "grid_y_limit(&lim)" in body and "std::min(lim, n - s.*base)" in body
    assert "if (n - s.*base <= lim) break;" in body                     # before the base can wrap
    assert body.index("hipGetLastError()") < body.index("if (n - s.*base <= lim) break;")
    for f in ("lcm_pgo.cpp", "lcm_ba.cpp"):
        assert "up16(size_t" not in src[f] and "up16(" in src[f], f
    assert src["lcm_internal.h"].count("size_t up16(size_t v)") == 1


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs clang++")
def test_the_shared_arithmetic_runs_clean_under_sanitizers(tmp_path):
    """tests/cpp/geom_host_check.cpp is the stand-alone program of csrc/lcm_geom_device.h.  Built as plain C++ (no HIP runtime is
    linked) with ASan + UBSan (no recovery) and run on the CPU: exit status 0 and no report."""
    exe = tmp_path / "geom_host_check"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", HIP_INCLUDE, "-I", G.CSRC,
                           os.path.join(G.ROOT, "tests", "cpp", "geom_host_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "all held" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr)
