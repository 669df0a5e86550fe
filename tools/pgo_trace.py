"""Per-kernel time of lcm_pgo_optimize from a kernel trace of tools/pgo_time.py, which itself sees kernel_ms per call only:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o pgo -- python tools/pgo_time.py --calls 5 --warmup 1 --out /dev/null
    python tools/pgo_trace.py DIR/pgo_kernel_trace.csv >> profiles/pgo_time.txt

A run starts at k_pgo_params; its size is k_pgo_assemble's grid (one workgroup of 64 threads per pose); the runs of 102 launches
are lcm_pgo_optimize's with 20 iterations (lcm_pgo_step makes 7).  The first run of every size is left out as warm-up."""
import collections
import csv
import re
import sys

NAMES = ("k_pgo_params", "k_pgo_linearise", "k_pgo_assemble", "k_pgo_sweep", "k_pgo_schur", "k_pgo_finish", "k_pgo_writeback")


def main(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    runs, cur = [], None
    for r in rows:
        m = re.search(r"k_pgo_[a-z]+", r["Kernel_Name"])
        if not m:
            continue
        if m.group(0) == "k_pgo_params":
            cur = {"n": None, "ms": collections.defaultdict(float), "launches": 0}
            runs.append(cur)
        if m.group(0) == "k_pgo_assemble" and cur["n"] is None:
            cur["n"] = int(r["Grid_Size_X"]) // 64
        cur["ms"][m.group(0)] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        cur["launches"] += 1
    by = collections.defaultdict(list)
    for r in runs:
        if r["launches"] == 102:
            by[r["n"]].append(r["ms"])
    print("per kernel, ms per call of lcm_pgo_optimize (20 iterations), mean over the traced calls but the first (rocprofv3 --kernel-trace, a run of its own; at 64 poses the chain's lcm_pgo_close_loop calls are among them):")
    for n in sorted(by):
        ks = by[n][1:]
        total = sum(sum(k.values()) for k in ks) / len(ks)
        print(f"trace {n:5d} poses ({len(ks)} calls): " + " | ".join(f"{nm[6:]} {sum(k[nm] for k in ks) / len(ks):.3f}" for nm in NAMES) + f" | sum {total:.3f}")


if __name__ == "__main__":
    main(sys.argv[1])
