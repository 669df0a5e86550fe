"""Code-object metadata of the RANSAC's local optimisation (lcm_lo.hip; hipcc cross-compiles gfx950 without a GPU): exactly
the two kernels the file's header names, none with scratch memory or spills, each within the VGPR and LDS budget the header
states, the inlier rule, the projection and the constraint row called from lcm_epi_device.h, the packed index and the rotation's
angle from lcm_geom_device.h, not restated."""
import os
import re
import subprocess

import pytest

import geomsrc as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")
# mangled name fragment -> (VGPRs, LDS bytes): the header's budget.  k_lo_refine: 126 doubles x 64 lanes of LDS let two
# workgroups share a CU's 160 KiB, and 256 VGPRs let two waves share a SIMD: the register file is not the limit.
BUDGET = {"11k_lo_selectE": (64, 1292), "11k_lo_refineE": (256, 64512)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_lo_kernels_use_no_scratch_and_fit_their_budget(tmp_path):
    out = tmp_path / "lcm_lo.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip",
                           os.path.join(CSRC, "lcm_lo.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
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
    src = open(os.path.join(CSRC, "lcm_lo.hip")).read()
    head = src[: src.index("#include")]
    defined = re.findall(r"__global__[^\n]*\bvoid\s+(\w+)\s*\(", src)
    assert sorted(defined) == ["k_lo_refine", "k_lo_select"]
    for k in defined:
        assert re.search(rf"^// {k}\s", head, flags=re.M), k
    budget = re.sub(r"\s+", " ", head[head.index("// Budget"):].replace("\n//", " "))
    assert "no scratch, no spills" in budget
    for frag, (vgprs, lds) in BUDGET.items():
        k = re.search(r"k_lo_\w+?(?=E$)", frag).group(0)
        m = re.search(rf"{k} at most (\d+) VGPRs and ([\d ]+) bytes", budget)
        assert m, k
        assert int(m.group(1)) == vgprs and int(m.group(2).replace(" ", "")) == lds, (k, m.groups())


def test_the_shared_rules_are_called_not_restated():
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "lcm_lo.hip")).read())
    dev = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "lcm_lo_device.h")).read())
    epi = open(os.path.join(CSRC, "lcm_epi_device.h")).read()
    assert epi.count("bool epi_inlier(") == 1 and epi.count("bool epi_project(") == 1      # still defined once, there
    for text in (src, dev):
        assert "bool epi_inlier(" not in text and "epi_project(double" not in text and "epi_put_row(double" not in text
        words = re.findall(r"\b\w+\b", text)
        assert "num" not in words and "den" not in words                 # no verdict of the files' own
    assert src.count("epi_inlier(") == 6 and src.count("epi_project(") == 1 and src.count("epi_norm(") >= 4
    assert dev.count("epi_put_row<1>(") == 1
    host = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "lcm_lo.cpp")).read())
    assert "epi_inlier(" not in host and "lo_eig9" not in host          # the host never restates or runs the model
    # the eigenvector's packed index and the rotation's gate and angle are the shared header's; lo_eig9 keeps its LDS stride, its
    # loops that are not unrolled and its loads before the gate
    G.assert_defined_once_in_geom(("sym_index", "jacobi_angle"))
    assert '#include "lcm_geom_device.h"' in dev and "zeta" not in dev and "1e-36" not in dev
    eig = dev[dev.index("void lo_eig9("):dev.index("void lo_denormalise(")]
    assert eig.count("jacobi_angle(") == 1 and set(re.findall(r"sym_index<(\w+)>", dev)) == {"9"} and "template <int STRIDE>" in dev
    assert eig.count("#pragma clang loop unroll(disable)") == 3 and eig.count("* STRIDE]") == 18
    assert eig.index("vq[k] = V[(9 * k + q) * STRIDE];") < eig.index("jacobi_angle(") < eig.index("W[sym_index<9>(k, p) * STRIDE] = cs * ap[k] - sn * aq[k];")
    assert "atomicAdd(" in src and not re.search(r"atomic\w*\([^)]*(double|float)", src)  # integer atomics only
