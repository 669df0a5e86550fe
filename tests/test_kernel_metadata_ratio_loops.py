"""Code-object metadata of the ratio loop-test kernels (lcm_ratio.hip; hipcc cross-compiles gfx950 without a GPU):
k_ratio_loop_count and k_ratio_loop_emit exist, use no scratch memory and spill nothing; k_ratio_rowlane's four shapes keep
the figures tests/test_kernel_metadata_ratio.py pins (the score kernel is untouched by the loop test)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    out = tmp_path_factory.mktemp("meta") / "lcm_ratio.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-x", "hip",
                           os.path.join(CSRC, "lcm_ratio.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    ks = {}
    for block in re.split(r"\n  - \.a", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        ks[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in FIELDS}
    return ks


def test_loop_test_kernels_exist_without_scratch_or_spills(kernels):
    for want in ("k_ratio_loop_count", "k_ratio_loop_emit"):
        found = [n for n in kernels if want in n]
        assert len(found) == 1, (want, sorted(kernels))
        m = kernels[found[0]]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (want, m)
        assert m["vgpr_count"] <= 64, (want, m)                 # 256-thread blocks, memory-bound: full occupancy
        # per-wave counts (emit) / the block-wide count's exchange words (count); the file-wide bound of
        # test_kernel_metadata_ratio.py applies to every kernel of lcm_ratio.hip
        assert m["group_segment_fixed_size"] <= 1024, (want, m)


def test_score_kernel_keeps_its_figures(kernels):
    shapes = [n for n in kernels if "k_ratio_rowlane" in n]
    assert len(shapes) == 4, sorted(kernels)
    for name in shapes:
        m = kernels[name]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 96, (name, m)
        assert m["group_segment_fixed_size"] <= 1024, (name, m)
