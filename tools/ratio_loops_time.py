"""Times the ratio-scored loop search with its verdict fused on the device against the two calls it is made of, on the same
stored frames (synth.make_frames, --frames x --rows, min_gap 30, LCM_TUNE_PACKED = 0), in one process and one run:

  (a) lcm_all_vs_all_ratio(--ratio)             kernel_ms                  k_ratio_rowlane alone
  (b) lcm_all_vs_all_loops_ratio(rp)            kernel_ms, aux_kernel_ms   the same search + k_ratio_loop_count, k_block_scan,
                                                                           k_ratio_loop_emit
  (c) lcm_all_vs_all_loops                      aux_kernel_ms              the existing loop-test kernels on the same pair count

Per call: --warmup calls, then the median, minimum and maximum over --calls calls of the device times lcm_last_launch_info
reports.  The statements checked (printed as `holds: True / False`, nothing is asserted):
  1. (b)'s kernel_ms is within the run's own spread of (a): |median_b - median_a| <= max(spread_a, spread_b), spread = max - min;
  2. (b)'s aux_kernel_ms is within max(relative spread, 10 %) of (c)'s: both read 8 bytes per pair and write 24 per candidate,
     (b) reads one more cached row count per pair.

    python tools/ratio_loops_time.py --out profiles/ratio_loops_time.txt
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402


def stats(xs):
    return statistics.median(xs), min(xs), max(xs)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--ratio", type=float, default=0.7)
    ap.add_argument("--min-rows", type=int, default=100)
    ap.add_argument("--min-matches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default="", help="also write the report to this file")
    args = ap.parse_args()

    pkg = entry.load_package()
    capi = pkg.capi
    fs = pkg.synth.make_frames(args.frames, args.rows, seed=pkg.synth.BASE_SEED)
    with pkg.Matcher() as m:
        m.reserve(fs.n_frames, args.rows)
        for f in range(fs.n_frames):
            m.append(int(fs.ids[f]), fs.frame(f))
        m.set_tuning(capi.TUNE_PACKED, 0)
        n, _ = m.all_vs_all_ratio_plan(args.ratio)
        d = m.dev_alloc(max(n, 1) * 8)
        out = np.zeros(max(n, 1), capi.CANDIDATE_DTYPE)
        found = {}

        def call_a():
            m.all_vs_all_ratio(args.ratio, d, n)
            m.sync()
            return m.launch_info()

        def call_b():
            c, _ = m.all_vs_all_loops_ratio(args.ratio, args.min_rows, args.min_matches, out=out)
            found["b"] = len(c)
            return m.launch_info()

        def call_c():
            c, _ = m.all_vs_all_loops(out=out)
            found["c"] = len(c)
            return m.launch_info()

        res = {}
        for name, call in (("a", call_a), ("b", call_b), ("c", call_c)):
            for _ in range(args.warmup):
                call()
            infos = [call() for _ in range(args.calls)]
            res[name] = {"kernel": stats([i.kernel_ms for i in infos]), "aux": stats([i.aux_kernel_ms for i in infos]),
                         "pairs": infos[-1].pairs}
        m.dev_free(d)

    (ka, ka0, ka1), (kb, kb0, kb1) = res["a"]["kernel"], res["b"]["kernel"]
    (xb, xb0, xb1), (xc, xc0, xc1) = res["b"]["aux"], res["c"]["aux"]
    holds1 = abs(kb - ka) <= max(ka1 - ka0, kb1 - kb0)
    rel = max((xb1 - xb0) / xb if xb > 0 else 0.0, (xc1 - xc0) / xc if xc > 0 else 0.0, 0.10)
    holds2 = xc > 0 and abs(xb - xc) <= rel * xc
    p = capi.default_params()
    lines = [
        f"ratio_loops_time: {args.frames} frames x {args.rows} rows, min_gap {p.min_gap}, pairs {res['a']['pairs']}, "
        f"{args.calls} calls after {args.warmup} warm-ups, ms as median [min .. max]",
        f"(a) lcm_all_vs_all_ratio({args.ratio})            kernel_ms     {ka:.3f} [{ka0:.3f} .. {ka1:.3f}]",
        f"(b) lcm_all_vs_all_loops_ratio({args.ratio}, {args.min_rows}, {args.min_matches}) kernel_ms     {kb:.3f} [{kb0:.3f} .. {kb1:.3f}]",
        f"                                               aux_kernel_ms {xb:.4f} [{xb0:.4f} .. {xb1:.4f}]   candidates {found['b']}",
        f"(c) lcm_all_vs_all_loops (min_matches {p.min_matches}, sim > {p.sim_threshold}) aux_kernel_ms {xc:.4f} [{xc0:.4f} .. {xc1:.4f}]   "
        f"candidates {found['c']}   pairs {res['c']['pairs']}",
        f"1. |(b) - (a)| kernel_ms = {abs(kb - ka):.3f} <= spread {max(ka1 - ka0, kb1 - kb0):.3f}: holds: {holds1}",
        f"2. |(b) - (c)| aux_kernel_ms = {abs(xb - xc):.4f} <= {rel * 100:.1f} % of (c) = {rel * xc:.4f}: holds: {holds2}",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
