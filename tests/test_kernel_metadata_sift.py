"""Code-object metadata of the SIFT keypoint detector (lcm_sift.hip; hipcc cross-compiles gfx950 without a GPU): exactly the kernels
the file's header names, without scratch memory or spills, each within the VGPR and LDS budget the header states, the blur's dynamic
LDS within a CU's 160 KiB at the largest radius; and from the source text: the arithmetic defined once in lcm_sift_device.h and
called from the kernels, no contraction in the blur, correctly rounded divisions, no atomic at all, every blur load through the
fold, one-dimensional grids.  Metadata fields and source structure only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")
# kernel -> (VGPRs, static LDS bytes), the file header's budget
BUDGET = {"k_sift_base": (32, 0), "k_sift_blur": (48, 0), "k_sift_half": (32, 0), "k_sift_extrema": (32, 16), "k_sift_refine": (80, 256),
          "k_sift_compact": (32, 16)}
CU_LDS = 160 * 1024


def kernels_of(src):
    return re.findall(r"__global__[^\n]*\bvoid\s+(\w+)\s*\(", src)


def strip(text):
    return re.sub(r"//[^\n]*", "", text)


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    out = tmp_path_factory.mktemp("sift") / "lcm_sift.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip",
                           os.path.join(CSRC, "lcm_sift.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    return out.read_text()


def test_kernels_use_no_scratch_and_fit_their_budgets(assembly):
    meta = assembly[assembly.index("amdhsa.kernels:"):]
    ks = {}
    for block in re.split(r"\n  - \.a", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        short = re.search(r"\d+(k_sift_[a-z_]+?)E", name).group(1)
        ks[short] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in FIELDS}
    assert sorted(ks) == sorted(BUDGET)
    for name, m in sorted(ks.items()):
        print(name, m)
        vgprs, lds = BUDGET[name]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= vgprs and m["group_segment_fixed_size"] <= lds, (name, m)
        assert (m["group_segment_fixed_size"] > 0) == (lds > 0), (name, m)
    assert not re.search(r"^\s+(scratch_|buffer_(load|store)\S* .*offen)", assembly, flags=re.M)


def test_the_blur_is_not_contracted_and_divisions_are_correctly_rounded(assembly):
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^_ZN3lcm\d+(k_sift_[a-z]+)E\w+:[^\n]*\n(.*?)\n\.Lfunc_end\d+:", assembly, flags=re.M | re.S)}
    assert sorted(bodies) == sorted(BUDGET)
    fused = re.compile(r"^\s+v_(?:pk_)?(?:fma|fmac|mad|mac)\w*_f(?:16|32|64)", flags=re.M)
    for name in ("k_sift_base", "k_sift_blur", "k_sift_half", "k_sift_extrema", "k_sift_compact"):
        assert not fused.search(bodies[name]), name          # every product and every sum is rounded on its own
    refine = bodies["k_sift_refine"]
    # the only fused operations are those inside the seven IEEE division sequences (six of the solve, one of the size)
    assert len(re.findall(r"^\s+v_div_fixup_f32", refine, flags=re.M)) == 7 and len(re.findall(r"^\s+v_div_fmas_f32", refine, flags=re.M)) == 7
    assert len(fused.findall(refine)) == 5 * 7
    assert not re.search(r"^\s+v_(exp|log|sin|cos|sqrt|rsq)_f32", assembly, flags=re.M)


def test_the_header_names_every_kernel_and_states_the_budget():
    src = open(os.path.join(CSRC, "lcm_sift.hip")).read()
    head = src[: src.index("#include")]
    assert sorted(kernels_of(src)) == sorted(BUDGET)
    for name in BUDGET:
        assert re.search(rf"^// {name}\s", head, flags=re.M), name
    flat = re.sub(r"\s+", " ", head.replace("\n//", " "))
    budget = flat[flat.index("Budget"):]
    assert "no scratch, no spills" in budget
    for names, (vgprs, lds) in ((("k_sift_refine",), (80, 256)), (("k_sift_blur",), (48, 0)), (("k_sift_extrema", "k_sift_compact"), (32, 16)),
                                (("k_sift_base", "k_sift_half"), (32, 0))):
        what = f"at most {vgprs} VGPRs and " + (f"{lds} bytes of LDS" if lds else "no (static )?LDS")
        assert re.search(rf"{' and '.join(names)} {what}", budget), (names, what)
        assert all(BUDGET[n] == (vgprs, lds) for n in names)
    assert "the same call gives the same bytes" in flat and "goes through sift_fold" in flat and "one-dimensional" in flat
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert all(f in make for f in ("lcm_sift.hip", "lcm_sift.cpp", "lcm_sift_device.h", "lcm_sift_host.h"))


def test_the_blur_tile_fits_a_cu():
    host = open(os.path.join(CSRC, "lcm_sift_host.h")).read()
    dev = open(os.path.join(CSRC, "lcm_sift_device.h")).read()
    tile = int(re.search(r"constexpr int SIFT_TILE = (\d+);", dev).group(1))
    r_max = int(re.search(r"constexpr int SIFT_MAX_RADIUS = (\d+);", dev).group(1))
    assert "(SIFT_TILE + 2 * r) * (size_t)(SIFT_TILE + 2 * r) + (size_t)(SIFT_TILE + 2 * r) * (size_t)SIFT_TILE) * sizeof(float)" in host
    lds = lambda r: ((tile + 2 * r) ** 2 + (tile + 2 * r) * tile) * 4            # noqa: E731
    assert (tile, r_max) == (32, 48) and lds(r_max) == 81920 <= CU_LDS // 2 and lds(13) == 20880 and CU_LDS // lds(13) == 7
    assert "static_assert(sift_blur_lds_bytes(SIFT_MAX_RADIUS) <= SIFT_LDS_BYTES / 2" in host
    src = strip(open(os.path.join(CSRC, "lcm_sift.hip")).read())
    assert "extern __shared__ float lds[];" in src and "hipFuncAttributeMaxDynamicSharedMemorySize" in src
    assert src.count("sift_blur_lds_bytes") == 0 and open(os.path.join(CSRC, "lcm_sift.cpp")).read().count("lcm::sift_blur_lds_bytes(") == 2


def test_the_arithmetic_exists_once_and_is_called_from_the_kernels():
    src = open(os.path.join(CSRC, "lcm_sift.hip")).read()
    dev = open(os.path.join(CSRC, "lcm_sift_device.h")).read()
    host = open(os.path.join(CSRC, "lcm_sift_host.h")).read()
    cpp = open(os.path.join(CSRC, "lcm_sift.cpp")).read()
    code, dev_code, host_code, cpp_code = strip(src), strip(dev), strip(host), strip(cpp)
    for fn in ("int sift_fold(", "float sift_upsampled(", "bool sift_is_extremum(", "bool sift_solve3(", "float sift_pow2(", "int sift_refine("):
        assert dev.count(fn) == 1 and fn not in src and fn not in host and fn not in cpp, fn
    assert re.findall(r'#include "([^"]+)"', src) == ["lcm_sift_device.h"]
    calls = lambda fn: len(re.findall(rf"(?<![\w]){fn}\(", code))               # noqa: E731
    assert calls("sift_refine") == 1 and calls("sift_is_extremum") == 1 and calls("sift_upsampled") == 1
    # every load of the blur's source goes through the fold, both coordinates
    blur = code[code.index("void k_sift_blur("):code.index("void k_sift_half(")]
    assert len(re.findall(r"a\.src\b", blur)) == 1 and blur.count("sift_fold(") == 2 and "fp contract(off)" in blur
    assert "const float* row = a.src + (size_t)sift_fold(ty0 + ly - r, a.h) * (size_t)a.w;" in blur
    assert len(re.findall(r"\brow\[", blur)) == 1 and "= row[sift_fold(tx0 + lx - r, a.w)];" in blur
    assert "x < a.w && y < a.h" in blur                      # nothing is stored beyond the image
    # the host runs none of the per-pixel arithmetic; the plan and the checks live in lcm_sift_host.h and are called from lcm_sift.cpp
    for fn in ("sift_refine", "sift_is_extremum", "sift_solve3"):
        assert not re.search(rf"(?<![\w]){fn}\(", cpp_code + host_code), fn
    for fn in ("sift_plan(", "sift_params_problem(", "sift_taps(", "sift_levels(", "sift_threshold(", "sift_refine_consts(", "sift_gauss_offset(",
               "sift_dog_offset("):
        assert re.search(rf"inline [\w: \*]+ {re.escape(fn)}", host_code), fn
    for fn in ("sift_plan(", "sift_taps(", "sift_levels(", "sift_threshold(", "sift_refine_consts(", "sift_gauss_offset(", "sift_dog_offset("):
        assert f"lcm::{fn}" in cpp_code, fn
    assert "hip" not in host_code.replace("../../include/lcm.h", "").lower().replace("ship", "")
    # no atomic of any kind, no inline assembly, no transcendental: the lists are ordered compactions
    words = set(re.findall(r"\b\w+\b", code + dev_code))
    assert not [w for w in words if w.lower().startswith("atomic")] and "asm" not in words
    assert not words & {"expf", "exp2f", "powf", "logf", "sqrtf", "atan2f", "fmaf", "__fmaf_rn", "exp", "pow"}
    assert code.count("__ballot(") == 2 and code.count("__syncthreads_count(") == 1 and "launch_block_scan" in cpp_code
    assert dev_code.count("#pragma clang fp contract(off)") == 4 and "fp contract(off)" in host
    # every grid is one-dimensional: nothing to slice
    assert "blockIdx.y" not in code and "launch_y_sliced" not in code and not re.search(r"dim3\([^)]*,[^)]*\), dim3\(256\)", code)


def test_kernel_names_are_the_files_own():
    every = []
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hip"):
            ks = kernels_of(open(os.path.join(CSRC, f)).read())
            every += ks
            assert all(k.startswith("k_sift_") == (f == "lcm_sift.hip") for k in ks), f
    assert len(every) == len(set(every))
