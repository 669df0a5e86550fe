"""The SIFT matcher's planning without a device (csrc/lcm_l2_host.h): the tile space, the chunk rule and its two environment
pins, the items and jobs of a list run, the count items, a loop search's tables and runs and the candidates walked from its
records, as a stand-alone program under ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-loop-closing_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_planners_run_clean_under_sanitizers(tmp_path):
    """tests/cpp/l2_host_check.cpp compares whole plans with literals: rows of 1, 32, 33, 128, 129, 256, 257, 512 and 513 on
    either side, one matrix as both sides, an empty matrix, a matrix that no pair names (tiles in the list plan, none in the
    count plan), 1023 and 1024 items-at-256 with the pin unset / 128 / 256 / illegal, and a store with a skipped slot, slots
    below and at min_rows, an empty admitted slot, last_past of -1, 0 and beyond the last slot, a curr without a run and several
    currs in one search.  Ragged tall calls (frames of 65535, 0, 1, 257, 32768 and 65535 rows; live and empty-sided pairs
    interleaved, empty pairs first and last, all empty, none, 300 pairs of 256 blocks; both chunk pins): every job's `reserved`
    and `out_row0`, `n_blocks`, `max_nq` and l2_pair_block for every p <= n_pairs against sums taken from the row counts alone.
    Built as plain C++ (HIP's headers for lcm_kernels.h's types only, no runtime is linked) with ASan +
    UBSan (no recovery) and run on the CPU: exit status 0 and no report."""
    exe = tmp_path / "l2_host_check"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem",
                           "/opt/rocm/include", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "l2_host_check.cpp"), "-o", str(exe)])
    env = {k: v for k, v in os.environ.items() if not k.startswith("LCM_TUNE_L2")}
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "all held" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr)
