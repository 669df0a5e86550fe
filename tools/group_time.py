"""Host wall time of two group calls whose cost is mostly host work: lcm_group_all_vs_all_loops and
lcm_group_query_scores_batch (8 queries) on a loopback group of --shards shards holding --frames frames of --rows rows,
min_gap 30.  --warmup calls, then the median, minimum and maximum over --calls calls, in ms.  One line per call kind.
LCM_LIB_PATH selects the library, so two builds can be compared in alternating fresh processes.

    python tools/group_time.py [--shards 8] [--frames 300] [--rows 500] [--calls 20]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402


def timed(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--rows", type=int, default=500)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    pkg = entry.load_package()
    fs = pkg.synth.make_frames(a.frames, a.rows, seed=11, dup_frac=0.2)
    p = pkg.default_params()
    p.min_gap = 30
    with pkg.Group(p, n_devices=a.shards, loopback_device=0) as g:
        g.reserve(a.frames, a.rows)
        for f in range(fs.n_frames):
            g.append(int(fs.ids[f]), fs.frame(f))
        pairs = pkg.synth.n_pairs_all_vs_all(a.frames, 30)
        out = np.zeros(pairs + 1, pkg.capi.CANDIDATE_DTYPE)
        found = []
        loops = timed(lambda: found.append(len(g.all_vs_all_loops(out=out)[0])), a.warmup, a.calls)
        queries = [fs.frame(f) for f in range(8)]
        qids = [int(fs.ids[-1]) + 31 + k for k in range(8)]
        records = []
        batch = timed(lambda: records.append(len(g.query_scores_batch(queries, qids)[0])), a.warmup, a.calls)
    print(f"lcm_group_all_vs_all_loops    {a.shards} shards {a.frames} x {a.rows}: wall_ms median {loops[0]:8.3f} min {loops[1]:8.3f} max {loops[2]:8.3f} | "
          f"{pairs} pairs, {found[-1]} candidates")
    print(f"lcm_group_query_scores_batch  {a.shards} shards, 8 queries   : wall_ms median {batch[0]:8.3f} min {batch[1]:8.3f} max {batch[2]:8.3f} | "
          f"{records[-1]} records")


if __name__ == "__main__":
    main()
