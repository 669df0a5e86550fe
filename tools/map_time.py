"""Times the map building's triangulation on the device (lcm_map_triangulate_pairs; lcm_map.hip), in one process and one run.

Scenes: per pair two neighbouring cameras of a ring of 24 (radius 4, numpy default_rng(53)) looking at a cloud of --records points
in [-1, 1]^3, pixels with 0.5 px of noise rounded to float, every tenth record with a zero mask byte.  Two shapes: one pair (the
per-keyframe call) and --pairs pairs (re-triangulating a whole trajectory in one launch).

  triangulate  lcm_map_triangulate_pairs per shape: kernel_ms (the one launch between the call's two events) and wall time (the
               host's per-pair plans, the upload of 17 bytes a record and the download of 65 included); the records per status.
  median       lcm_map_median_displacement on the same lists: kernel_ms and wall time.
  numpy        tests/mapref.py's triangulate on the same inputs: the whole of the one-pair shape, the first --ref-pairs pairs of
               the large one (said so in the line), once; the statuses compared with the device's.

Warm-up calls, then --calls timed calls; median (min - max).

    python tools/map_time.py          # writes profiles/map_time.txt and prints it
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as entry  # noqa: E402
from epi_time import mmm  # noqa: E402

K = (1000.0, 1000.0, 640.0, 360.0)


def scene(np, rng, n_pairs, n_records):
    """(R1, t1, R2, t2 per pair, pts float32 [n_pairs * n_records, 4], mask)."""
    a = 2 * np.pi * (rng.integers(0, 24, n_pairs)[:, None] + np.arange(2)[None, :] + 0.3 * rng.random((n_pairs, 2))) / 24
    C = np.stack([4 * np.cos(a), 4 * np.sin(a), 0.4 * rng.standard_normal((n_pairs, 2))], 2)          # [pair, view, 3]
    z = -C / np.linalg.norm(C, axis=2, keepdims=True)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x, axis=2, keepdims=True)
    R = np.stack([x, np.cross(z, x), z], 2)                                                             # [pair, view, 3, 3]
    t = -np.einsum("pvij,pvj->pvi", R, C)
    pts = np.empty((n_pairs, n_records, 4), np.float32)
    for p in range(n_pairs):
        X = rng.uniform(-1.0, 1.0, (n_records, 3))
        for v in range(2):
            Xc = X @ R[p, v].T + t[p, v]
            pts[p, :, 2 * v] = K[0] * Xc[:, 0] / Xc[:, 2] + K[2] + rng.uniform(-0.5, 0.5, n_records)
            pts[p, :, 2 * v + 1] = K[1] * Xc[:, 1] / Xc[:, 2] + K[3] + rng.uniform(-0.5, 0.5, n_records)
    mask = np.ones(n_pairs * n_records, np.uint8)
    mask[::10] = 0
    return R[:, 0], t[:, 0], R[:, 1], t[:, 1], pts.reshape(-1, 4), mask


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--records", type=int, default=4000)
    ap.add_argument("--ref-pairs", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_time.txt"))
    args = ap.parse_args()

    import numpy as np
    import mapref as M
    pkg = entry.load_package()
    c = pkg.capi
    rng = np.random.default_rng(53)
    mp = c.default_map_params(fx=K[0], fy=K[1], cx=K[2], cy=K[3])
    lines = [f"map_time: two neighbouring ring cameras a pair, {args.records} records a pair, 0.5 px of noise, every tenth record masked out, "
             f"{args.calls} timed calls after {args.warmup} warm-up calls"]
    with pkg.Matcher() as m:
        for n_pairs in (1, args.pairs):
            R1, t1, R2, t2, pts, mask = scene(np, rng, n_pairs, args.records)
            offs = (np.arange(n_pairs + 1) * args.records).astype(np.uintp)
            p1, p2 = c.pgo_poses(R1, t1), c.pgo_poses(R2, t2)
            kernel, wall, mk, mw = [], [], [], []
            for k in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                tri, status, info = m.map_triangulate_pairs(pts, offs, p1, p2, mp, mask)
                w = (time.perf_counter() - t0) * 1e3
                i = m.launch_info()
                t0 = time.perf_counter()
                med = m.map_median_displacement(pts, offs)
                w2 = (time.perf_counter() - t0) * 1e3
                if k >= args.warmup:
                    kernel.append(i.kernel_ms), wall.append(w), mk.append(m.launch_info().kernel_ms), mw.append(w2)
            assert i.launches == 1 and i.pairs == len(pts)
            counts = info["counts"].sum(0).tolist()
            lines.append(f"triangulate {n_pairs:5d} pairs x {args.records} records = {len(pts):9d}: kernel_ms {mmm(kernel)} | wall_ms {mmm(wall)} | "
                         f"{len(pts) / (np.median(kernel) * 1e-3):.3g} records/s in the kernel | records per status {counts[:6]}")
            lines.append(f"median      {n_pairs:5d} pairs x {args.records} records = {len(pts):9d}: kernel_ms {mmm(mk)} | wall_ms {mmm(mw)} | "
                         f"medians {float(med.min()):.2f} .. {float(med.max()):.2f} px")
            ref = min(n_pairs, args.ref_pairs)
            t0 = time.perf_counter()
            same = True
            for p in range(ref):
                lo, hi = p * args.records, (p + 1) * args.records
                want = M.triangulate(M.Plan(K, R1[p], t1[p], R2[p], t2[p], float(info[p]["cos_min"])), pts[lo:hi], mask[lo:hi])
                same = same and bool(np.array_equal(want.status, status[lo:hi])) and want.tri().tobytes() == tri[lo:hi].tobytes()
            ms = (time.perf_counter() - t0) * 1e3
            whole = "" if ref == n_pairs else f" (the first {ref} of the {n_pairs} pairs; x {n_pairs // ref} for all of them)"
            lines.append(f"numpy       {ref:5d} pairs x {args.records} records: tests/mapref.py triangulate, once: {ms:.0f} ms of wall time{whole} | "
                         f"statuses and records identical to the device's: {same}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
