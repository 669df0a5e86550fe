"""Code-object metadata of the map building (lcm_map.hip; hipcc cross-compiles gfx950 without a GPU): exactly the kernels the file's
header names, without scratch memory or spills, each within the VGPR and LDS budget the header states; and from the source text: the
arithmetic defined once in lcm_map_device.h and called from the kernels, the camera point, the projection, the packed index and
the Jacobi rotation's angle taken from lcm_geom_device.h and stated nowhere else, every index of the 4 x 4 problem a compile-time
constant, integer atomics only.  Metadata fields and source structure only."""
import os
import re
import subprocess

import pytest

import geomsrc as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")
# kernel -> (VGPRs, LDS bytes), the file header's budget.  128 VGPRs leave the triangulation four waves per SIMD
BUDGET = {"k_map_triangulate": (128, 0), "k_map_median": (64, 1040), "k_map_merge_count": (64, 32), "k_map_merge_emit": (64, 32)}


def kernels_of(src):
    return re.findall(r"__global__[^\n]*\bvoid\s+(\w+)\s*\(", src)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_kernels_use_no_scratch_and_fit_their_budgets(tmp_path):
    out = tmp_path / "lcm_map.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip",
                           os.path.join(CSRC, "lcm_map.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    ks = {}
    for block in re.split(r"\n  - \.a", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        short = re.search(r"\d+(k_map_[a-z_]+?)E", name).group(1)
        ks[short] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in FIELDS}
    assert sorted(ks) == sorted(BUDGET)
    for name, m in sorted(ks.items()):
        print(name, m)
        vgprs, lds = BUDGET[name]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= vgprs and m["group_segment_fixed_size"] <= lds, (name, m)
        assert (m["group_segment_fixed_size"] > 0) == (lds > 0), (name, m)


def test_the_header_names_every_kernel_and_states_the_budget():
    src = open(os.path.join(CSRC, "lcm_map.hip")).read()
    head = src[: src.index("#include")]
    assert sorted(kernels_of(src)) == sorted(BUDGET)
    for name in BUDGET:
        assert re.search(rf"^// {name}\s", head, flags=re.M), name
    flat = re.sub(r"\s+", " ", head.replace("\n//", " "))
    budget = flat[flat.index("Budget"):]
    assert "no scratch, no spills" in budget
    for names, (vgprs, lds) in ((("k_map_triangulate",), (128, 0)), (("k_map_median",), (64, 1040)), (("k_map_merge_count", "k_map_merge_emit"), (64, 32))):
        what = f"at most {vgprs} VGPRs and " + (f"{lds} bytes of LDS" if lds else "no LDS")
        assert re.search(rf"{' and '.join(names)} {re.escape(what)}", budget), (names, what)
        assert all(BUDGET[n] == (vgprs, lds) for n in names)
    assert "in list order by construction" in flat and "the same call gives the same bytes" in flat and "radix select" in flat
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert all(f in make for f in ("lcm_map.hip", "lcm_map.cpp", "lcm_map_device.h", "lcm_map_host.h", G.GEOM))


def test_the_arithmetic_exists_once_and_is_called_from_the_kernels():
    src = open(os.path.join(CSRC, "lcm_map.hip")).read()
    dev = open(os.path.join(CSRC, "lcm_map_device.h")).read()
    host = open(os.path.join(CSRC, "lcm_map_host.h")).read()
    cpp = open(os.path.join(CSRC, "lcm_map.cpp")).read()
    strip = lambda t: re.sub(r"//[^\n]*", "", t)                               # noqa: E731
    code, dev_code, host_code, cpp_code = strip(src), strip(dev), strip(host), strip(cpp)
    geom_code = strip(open(os.path.join(CSRC, G.GEOM)).read())
    for fn in ("double map_displacement(", "void map_system(", "void map_rotate_row(", "void map_rotate(", "void map_jacobi4(",
               "double map_parallax_cos(", "double map_reproj_error(", "int map_record("):
        assert dev.count(fn) == 1 and fn not in src and fn not in host and fn not in cpp and fn not in geom_code, fn
    # the shared functions are used, not restated: defined once in the shared header, in no other file of csrc
    G.assert_defined_once_in_geom(("rigid_apply", "pinhole_project", "sym_index", "jacobi_angle"))
    assert re.findall(r'#include "([^"]+)"', src) == ["lcm_map_device.h"] and '#include "lcm_geom_device.h"' in dev
    assert dev_code.count("rigid_apply(") == 2 and dev_code.count("pinhole_project(") == 1 and dev_code.count("jacobi_angle(") == 1
    # the kernels call it: the record's arithmetic once, the displacement once
    assert code.count("map_record(") == 1 and code.count("map_displacement(") == 1
    # the Jacobi rotation's angle is stated in the shared header alone: its formula appears nowhere else under csrc, the
    # RANSAC's 3 x 3 (compiled with contraction, so kept apart) aside
    for f in sorted(os.listdir(CSRC)):
        text = strip(open(os.path.join(CSRC, f)).read())
        if f not in (G.GEOM, "lcm_epi_device.h"):
            assert "zeta" not in text, f
        if f != "lcm_map_device.h":
            assert "map_rotate" not in text and "map_jacobi4(" not in text and "map_system(" not in text, f
    assert geom_code.count("zeta * zeta") == 1 and dev_code.count("map_jacobi4(") == 2 and dev_code.count("map_system(") == 2
    # every index into M and the product is a compile-time constant: template arguments and literals, no subscript by a loop
    # variable inside the rotation, the six pairs unrolled, one loop over the sweeps
    rot = dev_code[dev_code.index("void map_rotate_row("):dev_code.index("double map_parallax_cos(")]
    assert set(re.findall(r"\bsym_index<4>\(([^()]*)\)", rot)) <= {"K, P", "K, Q", "P, P", "Q, Q", "P, Q", "0, 0", "1, 1", "2, 2", "3, 3"}
    assert set(re.findall(r"\bsym_index<(\w+)>", dev_code)) == {"4"} and len(re.findall(r"\ba\[([^\]]*)\]", rot)) == len(re.findall(r"\ba\[sym_index<4>\(", rot))
    assert "constexpr int sym_index(int i, int j)" in geom_code           # so that each of these is a constant
    assert set(re.findall(r"\bv\[([^\]]*)\]", rot)) <= {"4 * K + P", "4 * K + Q", "16"} | {str(i) for i in range(16)}
    assert [tuple(map(int, m)) for m in re.findall(r"map_rotate<(\d), (\d)>\(m, v\)", rot)] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert rot.count("for (") == 1 and "sweep < MAP_JACOBI_SWEEPS" in rot and "unroll(disable)" in rot
    # no floating-point atomics: the atomics are the histogram's, the counts' and the winner's, all on integers
    atomics = re.findall(r"atomic\w+\(&([\w\.]+\[)", code)
    assert sorted(atomics) == ["a.counts[", "a.winner[", "hist["] and len(re.findall(r"atomic", code)) == 3
    assert re.search(r"__shared__ uint32_t hist\[256\]", code) and re.search(r"uint32_t\* counts;", dev_code) and re.search(r"int32_t\* winner;", dev_code)
    assert "atomic" not in dev_code.replace("integer atomic", "") and "asm" not in set(re.findall(r"\b\w+\b", code))
    assert "#pragma clang fp contract(off)" in dev and "fp contract(off)" in src and "fp contract(off)" in host
    words = set(re.findall(r"\b\w+\b", code + dev_code))
    assert not words & {"acos", "cos", "sin", "atan2", "fma", "__fma_rn"}
    # the host runs none of the record arithmetic; the plan and the gates live in lcm_map_host.h and are called from lcm_map.cpp
    for fn in ("map_record(", "map_jacobi4(", "map_parallax_cos(", "map_reproj_error("):
        assert fn not in cpp_code and fn not in host_code, fn
    for fn in ("map_plan_pair(", "map_offsets_problem(", "map_merge_problem(", "map_motion_verdict(", "map_pose_verdict(", "map_new_pose(", "map_params_problem("):
        assert host_code.count(f" {fn}") == 1 and fn in cpp_code, fn
    assert "hip" not in host_code.replace("../../include/lcm.h", "").replace("lcm_map_device.h", "").lower().replace("ship", "")


def test_kernel_names_are_the_files_own():
    every = []
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hip"):
            ks = kernels_of(open(os.path.join(CSRC, f)).read())
            every += ks
            assert all(k.startswith("k_map_") == (f == "lcm_map.hip") for k in ks), f
    assert len(every) == len(set(every))
