"""Times the ratio-test scored bulk search against the plain bulk search it is modelled on, on the same stored frames
(synth.make_frames, --frames x --rows, min_gap 30: the plain route, one workgroup per (query frame, run of stored frames)).

  --mode ratio   lcm_all_vs_all_ratio(--ratio): k_ratio_rowlane, two running distances per query row + count on the device
  --mode plain   lcm_all_vs_all with LCM_TUNE_PACKED = 0: k_score_rowlane, distance only (works with a library built from
                 the PARENT commit: only the entry points it exports are bound)
  --mode lists   the same score through the pair mode: lcm_match_stored_batch_ratio over the first --pairs pairs, match
                 lists downloaded and counted on the host (what a user of the reference's loop search had before)

Per mode: --warmup calls, then the median, minimum and maximum of lcm_last_launch_info().kernel_ms (device events around
the score kernel) and of the call's wall time (call + lcm_sync) over --calls calls; one JSON line.  The surcharge of the
second running distance is (ratio, this commit) / (plain, parent commit's library selected with LCM_LIB_PATH); run the two
alternately in one session on an otherwise idle card:

    LCM_LIB_PATH=/path/to/parent/liblcm_hip.so python tools/ratio_time.py --mode plain
    python tools/ratio_time.py --mode ratio
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("ratio", "plain", "lists"), required=True)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--ratio", type=float, default=0.7)
    ap.add_argument("--pairs", type=int, default=512, help="--mode lists: pairs per call")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    pkg = entry.load_package()
    capi = pkg.capi
    exported = ctypes.CDLL(capi.LIB_PATH)        # a library built from the parent commit lacks the new entry points
    for name in [n for n in capi._SIGNATURES if not hasattr(exported, n)]:
        del capi._SIGNATURES[name]
    fs = pkg.synth.make_frames(args.frames, args.rows, seed=pkg.synth.BASE_SEED)
    with pkg.Matcher() as m:
        m.reserve(fs.n_frames, args.rows)
        for f in range(fs.n_frames):
            m.append(int(fs.ids[f]), fs.frame(f))
        m.set_tuning(capi.TUNE_PACKED, 0)
        n, offs = m.all_vs_all_plan()
        extra = {}
        if args.mode == "lists":
            gap = m.params.min_gap
            pairs = [(int(fs.ids[c]), int(fs.ids[s])) for c in range(fs.n_frames) for s in range(max(c - gap + 1, 0))][: args.pairs]
            cap = args.rows * len(pairs)
            counts = []

            def call():
                lists, o = m.match_stored_batch_ratio(pairs, args.ratio, cap=cap)
                counts[:] = [len(x) for x in lists]
            n = len(pairs)
            # device -> host: two 4-byte keys per query row; the lists are then built on the host (16-byte records)
            extra = {"download_bytes_per_pair": 8 * args.rows}
        else:
            d = m.dev_alloc(n * 8)
            if args.mode == "ratio":
                call = lambda: (m.all_vs_all_ratio(args.ratio, d, n), m.sync())  # noqa: E731
            else:
                call = lambda: (m.all_vs_all(d, n), m.sync())  # noqa: E731
            extra = {"download_bytes_per_pair": 8}
        for _ in range(args.warmup):
            call()
        kernel, wall = [], []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            kernel.append(m.launch_info().kernel_ms)
        info = m.launch_info()
        if args.mode == "lists":
            extra["matches_per_pair_mean"] = sum(counts) / max(len(counts), 1)
        else:
            import numpy as np
            got = np.zeros(n, capi.SCORE_DTYPE)
            m.dev_download(d, got)
            m.dev_free(d)
            extra["good_count_sum"] = int(got["good_count"].astype(np.int64).sum())
        km, wm = statistics.median(kernel), statistics.median(wall)
        out = {"mode": args.mode, "label": args.label, "library": capi.LIB_PATH, "frames": args.frames, "rows": args.rows,
               "ratio": args.ratio, "pairs": n, "distances": info.distances, "workgroups": info.workgroups,
               "launches": info.launches, "route": info.route, "calls": args.calls, "warmup": args.warmup,
               "kernel_ms_median": km, "kernel_ms_min": min(kernel), "kernel_ms_max": max(kernel),
               "wall_ms_median": wm, "wall_ms_min": min(wall),
               "distances_per_s_kernel": info.distances / (km * 1e-3) if km > 0 else None,
               "pairs_per_s_wall": n / (wm * 1e-3)}
        out.update(extra)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
