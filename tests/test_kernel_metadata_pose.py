"""Code-object metadata of the relative-pose recovery (lcm_pose.hip; hipcc cross-compiles gfx950 without a GPU): exactly
the one kernel the file's header names, without scratch memory or spills, within the VGPR and LDS budget the header states,
and the depth test defined once in lcm_pose_device.h and called, not restated, by both passes of the kernel."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")
# The compiler gives 90 VGPRs: 96 is the most at which five waves share a SIMD's 512 registers, the next
# occupancy step above that.  LDS: 4 waves x 5 words.
VGPRS, LDS = 96, 80


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_pose_kernel_uses_no_scratch_and_fits_its_budget(tmp_path):
    out = tmp_path / "lcm_pose.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip",
                           os.path.join(CSRC, "lcm_pose.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    ks = {}
    for block in re.split(r"\n  - \.a", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        ks[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in FIELDS}
    assert len(ks) == 1 and "14k_pose_recoverE" in next(iter(ks)), sorted(ks)
    m = next(iter(ks.values()))
    print("k_pose_recover:", m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["vgpr_count"] <= VGPRS, m
    assert 0 < m["group_segment_fixed_size"] <= LDS, m


def test_the_header_names_the_kernel_and_states_the_budget():
    src = open(os.path.join(CSRC, "lcm_pose.hip")).read()
    head = src[: src.index("#include")]
    assert re.findall(r"__global__[^\n]*\bvoid\s+(\w+)\s*\(", src) == ["k_pose_recover"]
    assert re.search(r"^// k_pose_recover\s", head, flags=re.M)
    budget = re.sub(r"\s+", " ", head[head.index("// Budget"):].replace("\n//", " "))
    m = re.search(r"k_pose_recover at most (\d+) VGPRs and (\d+) bytes of LDS", budget)
    assert m and (int(m.group(1)), int(m.group(2))) == (VGPRS, LDS), budget
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"k_pose_recover[^\n]*\b90 VGPRs", design) and re.search(r"\b96\b[^\n]*five waves", design)
    assert "lcm_pose.hip" in open(os.path.join(CSRC, "Makefile")).read() and "lcm_pose.cpp" in open(os.path.join(CSRC, "Makefile")).read()


def test_the_depth_test_exists_once_and_is_called_from_both_passes():
    src = open(os.path.join(CSRC, "lcm_pose.hip")).read()
    dev = open(os.path.join(CSRC, "lcm_pose_device.h")).read()
    assert dev.count("bool pose_in_front(") == 1 and dev.count("uu * vv - uv * uv") == 1 and dev.count("max_depth * D") == 1
    assert dev.count("bool pose_decompose(") == 1
    code = re.sub(r"//[^\n]*", "", src)                     # the kernel's text without its comments
    kernel = code[code.index("__global__"): code.index("hipError_t launch_pose_recover")]
    one, two = kernel.split("__syncthreads();")             # pass 1 | the reduction's second half and pass 2
    assert one.count("pose_in_front(") == 4 and two.count("pose_in_front(") == 1
    assert kernel.count("pose_decompose(") == 1 and kernel.count("epi_norm(") == 8
    # no verdict of the kernel file's own: none of the depth test's quantities outside the header
    words = set(re.findall(r"\b\w+\b", code))
    assert not words & {"uu", "vv", "uv", "ut", "vt", "D", "n1", "n2", "far"}
    assert not re.search(r"max_depth\s*\*|\*\s*[\w.]*max_depth\b", code)
    host = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "lcm_pose.cpp")).read())
    assert "pose_in_front(" not in host and "pose_decompose(" not in host      # the host never restates or runs them
    # the existing RANSAC kernels' file is untouched by the feature: it still holds its three kernels and no pose code
    epi = open(os.path.join(CSRC, "lcm_epi.hip")).read()
    assert "pose" not in epi
