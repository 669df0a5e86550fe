"""Code-object metadata of the essential-matrix RANSAC (lcm_epi.hip; hipcc cross-compiles gfx950 without a GPU): exactly
the three kernels the file's header names, none with scratch memory or spills, each within the VGPR and LDS budget the
header states, and the inlier rule defined once in lcm_epi_device.h and called, not restated, by the kernels."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")
# mangled name fragment -> (VGPRs, LDS bytes): the header's budget
BUDGET = {"11k_epi_solveE": (192, 36864), "11k_epi_scoreE": (64, 16400), "10k_epi_maskE": (64, 0)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_epi_kernels_use_no_scratch_and_fit_their_budget(tmp_path):
    out = tmp_path / "lcm_epi.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip",
                           os.path.join(CSRC, "lcm_epi.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    ks = {}
    for block in re.split(r"\n  - \.a", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        ks[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in FIELDS}
    for want in BUDGET:
        assert sum(want in n for n in ks) == 1, (want, sorted(ks))
    assert len(ks) == len(BUDGET), sorted(ks)
    for name, m in ks.items():
        vgprs, lds = next(v for k, v in BUDGET.items() if k in name)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= vgprs, (name, m)
        assert m["group_segment_fixed_size"] <= lds, (name, m)


def test_the_header_names_the_kernels_and_states_the_budget():
    src = open(os.path.join(CSRC, "lcm_epi.hip")).read()
    head = src[: src.index("#include")]
    defined = re.findall(r"__global__[^\n]*\bvoid\s+(\w+)\s*\(", src)
    assert sorted(defined) == ["k_epi_mask", "k_epi_score", "k_epi_solve"]
    for k in defined:
        assert re.search(rf"^// {k}\s", head, flags=re.M), k
    budget = re.sub(r"\s+", " ", head[head.index("// Budget"):].replace("\n//", " "))
    for frag, (vgprs, lds) in BUDGET.items():
        k = re.search(r"k_epi_\w+?(?=E$)", frag).group(0)
        m = re.search(rf"{k} at most (\d+) VGPRs and ([\d ]+) bytes|{k} at most (\d+) VGPRs and no LDS", budget)
        assert m, k
        assert int(m.group(1) or m.group(3)) == vgprs and int((m.group(2) or "0").replace(" ", "")) == lds, (k, m.groups())


def test_the_inlier_rule_exists_once_and_is_called():
    src = open(os.path.join(CSRC, "lcm_epi.hip")).read()
    dev = open(os.path.join(CSRC, "lcm_epi_device.h")).read()
    assert dev.count("bool epi_inlier(") == 1 and dev.count("num * num") == 1 and dev.count("t2 * den") == 1
    code = re.sub(r"//[^\n]*", "", src)                     # the kernels' text without its comments
    assert code.count("epi_inlier(") == 2                   # k_epi_score and k_epi_mask, nowhere else
    # no verdict of the kernel file's own: no numerator, denominator or comparison against t2 outside the header
    assert "num" not in re.findall(r"\b\w+\b", code) and "den" not in re.findall(r"\b\w+\b", code)
    assert not re.search(r"\bt2\s*\*|\*\s*[\w.]*t2\b", code)
    host = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "lcm_epi.cpp")).read())
    assert "epi_inlier(" not in host                       # the host never restates or runs it either
