"""Deterministic frames whose Hamming distances are CHOSEN, not random: inputs for the good-match filter
`d <= max(ratio * min_d, dist_floor)` at its boundaries.

Random descriptors put every best distance near 90..110, where `2 * min_d` keeps every row and the `<=` boundary is
never reached.  The frames here plant, for a given (ratio, dist_floor), query rows whose best distance is exactly
`thr - 1`, `thr` and `thr + 1` (thr = max(ratio * min_d, dist_floor)), and put the first minimum of a row (with an
equal-distance decoy after it) on the kernels' structural seams: train rows 0 / last, the 8-row group of the group-key
argmin, the 32-row tile of the matrix-core kernels; query rows 511 / 512 and 2047 / 2048 (the query chunk seams).

* near pairs: train row = query row XOR a mask of exactly k bits (spread over all 8 dwords and both 16-bit halves of
  each dword), every other train row ~128 away: best distances 0..80 as planted;
* far pairs: query rows = b ^ (small mask on bits A), train rows = ~b ^ (small mask on bits B), A and B disjoint:
  every distance is 256 - |mask_q| - |mask_t|, i.e. 240..256, min_d > 128, and 256 (the exact complement) occurs in
  the `tied` form (every train row == ~b).

Every generator computes the distances it produced (numpy, popcount table) and asserts that the planted rows are
there: the best distance and first-minimum index of each planted row, and the presence of the rows at thr - 1 / thr /
thr + 1 wherever the distance range allows them.  A test built on these cannot silently degrade to "every row good".
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

NEAR_LIMIT = 80          # planted near distances stay <= this; unrelated random rows are >= ~95 (asserted)
GRID = [(2, 0), (1, 0), (0, 0), (3, 0), (0, 64), (2, 64), (1, 255), (0, 256), (65536, 0), (0, 65536)]
QUERY_SEAMS = (0, 511, 512, 2047, 2048)
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
# 16-bit halves of the 8 dwords, as bit positions of the 256-bit row (little-endian bytes, like the kernels' loads)
_HALVES = [list(range(16 * h, 16 * h + 16)) for h in range(16)]
_FAR_A = [b for b in range(256) if b % 16 < 8]      # query-side mask bits (every half holds 8 of them)
_FAR_B = [b for b in range(256) if b % 16 >= 8]     # train-side mask bits


def threshold(ratio: int, floor: int, min_d: int) -> int:
    return max(ratio * min_d, floor)


def dist_matrix(q, t) -> np.ndarray:
    """Exact Hamming distances (nq, nt), int32, in row chunks (a 2500 x 2500 pair stays small)."""
    q = np.asarray(q, np.uint8)
    t = np.asarray(t, np.uint8)
    out = np.zeros((len(q), len(t)), np.int32)
    for r0 in range(0, len(q), 128):
        out[r0: r0 + 128] = _POP[q[r0: r0 + 128, None, :] ^ t[None, :, :]].sum(axis=2)
    return out


def _bits_to_row(bits) -> np.ndarray:
    row = np.zeros(256, np.uint8)
    row[list(bits)] = 1
    return np.packbits(row, bitorder="little")


def spread_mask(rng, k: int) -> np.ndarray:
    """32-byte mask of exactly k bits, dealt round-robin over the 16 half-dwords (every dword, both halves)."""
    order = rng.permutation(16)
    pools = [list(rng.permutation(_HALVES[h])) for h in range(16)]
    bits = [pools[order[i % 16]].pop() for i in range(k)]
    return _bits_to_row(bits)


def _mask_from(rng, pool, k: int) -> np.ndarray:
    """k bits of `pool` (already interleaved over the 16 halves), round-robin from a random start."""
    pool = list(pool)
    by_half = [[b for b in pool if b // 16 == h] for h in range(16)]
    for lst in by_half:
        rng.shuffle(lst)
    order = rng.permutation(16)
    bits = [by_half[order[i % 16]][i // 16] for i in range(k)]
    return _bits_to_row(bits)


@dataclass
class Pair:
    q: np.ndarray                 # (nq, 32) uint8
    t: np.ndarray                 # (nt, 32) uint8
    ratio: int
    floor: int
    min_d: int                    # min over the query rows' best distances (as planted and verified)
    thr: int
    kind: str
    boundary: dict = field(default_factory=dict)    # distance -> number of rows with that best distance (thr - 1 .. + 1)


def _wanted(thr: int, lo: int, hi: int):
    return [d for d in (thr, thr + 1, thr - 1) if lo <= d <= hi]


def _check(pair: Pair, planted: dict, first: dict, hi: int, need_boundary: bool):
    d = dist_matrix(pair.q, pair.t)
    best = d.min(axis=1)
    arg = d.argmin(axis=1)
    for r, k in planted.items():
        assert best[r] == k, (pair.kind, r, int(best[r]), k)
        assert arg[r] == first[r], (pair.kind, r, int(arg[r]), first[r])
    assert int(best.min()) == pair.min_d, (pair.kind, int(best.min()), pair.min_d)
    if pair.kind == "near":         # the rows without a partner are far above every planted distance
        free = [r for r in range(len(pair.q)) if r not in planted]
        assert all(best[r] > NEAR_LIMIT for r in free), pair.kind
    pair.boundary = {w: int((best == w).sum()) for w in (pair.thr - 1, pair.thr, pair.thr + 1)}
    if need_boundary:
        for w in _wanted(pair.thr, pair.min_d, hi):
            assert pair.boundary[w] > 0, (pair.kind, pair.ratio, pair.floor, pair.thr, w)
        if pair.thr + 1 <= hi:      # at least one row fails the filter
            assert int((best > pair.thr).sum()) > 0


def _near_min(ratio: int, floor: int, seed: int) -> int:
    """A planted min_d for which thr + 1 still fits under NEAR_LIMIT when the ratio decides it."""
    choices = [0, 1, 20, 36, 5]
    m = choices[seed % len(choices)]
    while m > 0 and ratio * m + 1 > NEAR_LIMIT:
        m //= 2
    return m


def near_pair(nq: int, nt: int, ratio: int, floor: int, seed: int, min_d: int | None = None) -> Pair:
    """Query rows at random; train rows = partners (query row ^ k-bit mask) on the seams, decoys after them, the rest
    partners of further query rows (or random filler rows)."""
    rng = np.random.default_rng([seed, nq, nt, ratio % 65537, floor % 65537, 1])
    m = _near_min(ratio, floor, seed) if min_d is None else min_d
    thr = threshold(ratio, floor, m)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    # query rows that get a partner: the query seams and the last row first, then the others in random order
    prio = [r for r in list(QUERY_SEAMS) + [nq - 1, 1, 7, 8] if r < nq]
    prio = list(dict.fromkeys(prio)) + [r for r in rng.permutation(nq).tolist() if r not in prio]
    # train positions: (first, decoy) on the seams, the last row alone (padding rows copy it when nt % 4 != 0)
    seams = [(7, 8), (31, 32), (0, nt - 1), (63, 64), (nt - 1, None), (127, 128)]
    used, slots = set(), []
    for a, b in seams:
        if a < nt and a not in used and (b is None or (b < nt and b not in used and b != a)):
            slots.append((a, b)); used.add(a)
            if b is not None:
                used.add(b)
    slots += [(p, None) for p in rng.permutation(nt).tolist() if p not in used]
    ks = [k for k in [m] + _wanted(thr, m, NEAR_LIMIT)]
    ks = list(dict.fromkeys(ks))
    planted, first = {}, {}
    for i, (r, (a, b)) in enumerate(zip(prio, slots)):
        k = ks[i] if i < len(ks) else int(rng.integers(m, NEAR_LIMIT + 1))
        t[a] = q[r] ^ spread_mask(rng, k)
        if b is not None:
            t[b] = q[r] ^ spread_mask(rng, k)          # equal distance, later index: must lose the tie
        planted[r], first[r] = k, a
    pair = Pair(q, t, ratio, floor, m if planted else -1, thr, "near")
    if not planted:                                     # an empty side: nothing to plant
        return pair
    _check(pair, planted, first, NEAR_LIMIT, need_boundary=len(planted) >= 4)
    return pair


def far_pair(nq: int, nt: int, ratio: int, floor: int, seed: int, tied: bool = False, seam: int = 0,
             wmax: int = 12) -> Pair:
    """Every distance in 240..256.  tied: every train row is ~b (best = 256 - |mask_q|, 256 present, first minimum at
    row 0 for all).  Otherwise train masks have weight 1, and weight 2 at the seam's (first, decoy) rows: every query
    row's best is 254 - |mask_q| with its first minimum on that seam."""
    rng = np.random.default_rng([seed, nq, nt, ratio % 65537, floor % 65537, 2 + int(tied)])
    b = rng.integers(0, 256, 32, dtype=np.uint8)
    top = 256 if tied else 254
    m = top - wmax
    thr = threshold(ratio, floor, m)
    if tied:
        t = np.repeat((~b)[None, :], nt, axis=0)
        f = 0
    else:
        t = np.stack([~b ^ _mask_from(rng, _FAR_B, 1) for _ in range(nt)]) if nt else np.zeros((0, 32), np.uint8)
        f, dec = [(0, nt - 1), (7, 8), (31, 32), (nt - 1, None)][seam % 4]
        if f >= nt or (dec is not None and (dec >= nt or dec == f)):
            f, dec = nt - 1, None
        t[f] = ~b ^ _mask_from(rng, _FAR_B, 2)
        if dec is not None:
            t[dec] = ~b ^ _mask_from(rng, _FAR_B, 2)
    ws = [wmax] + [top - d for d in _wanted(thr, m, top)]
    ws = list(dict.fromkeys(ws))
    prio = [r for r in list(QUERY_SEAMS) + [nq - 1] if r < nq]
    prio = list(dict.fromkeys(prio)) + [r for r in range(nq) if r not in prio]
    q = np.zeros((nq, 32), np.uint8)
    planted, first = {}, {}
    for i, r in enumerate(prio):
        w = ws[i] if i < len(ws) else int(rng.integers(0, wmax + 1))
        q[r] = b ^ _mask_from(rng, _FAR_A, w)
        planted[r], first[r] = top - w, f
    pair = Pair(q, t, ratio, floor, m if nq and nt else -1, thr, "far")
    if nq and nt:
        _check(pair, planted, first, top, need_boundary=nq >= 4)
    return pair


@dataclass
class Frames:
    """Stored-frame layout of the oracle / the GPU tests: rows (n, stride, 32), counts, strictly increasing ids."""
    rows: np.ndarray
    counts: np.ndarray
    ids: np.ndarray
    pairs: list            # (query frame, train frame, Pair) of the planted pairs

    @property
    def n_frames(self) -> int:
        return int(self.rows.shape[0])

    def frame(self, f: int) -> np.ndarray:
        return self.rows[f, : int(self.counts[f])]


def frames(specs, ratio: int, floor: int, seed: int, empty: bool = True, duplicate: bool = True) -> Frames:
    """A database of planted pairs: for each spec (kind, nq, nt[, option]) the train frame, then its query frame (so
    that with min_gap 1 the query frame sees its train frame, and every earlier frame, as stored frames).  `empty`
    adds an empty frame after the first pair, `duplicate` an exact copy of the first pair's train frame at the end."""
    fr, pairs = [], []
    for i, spec in enumerate(specs):
        kind, nq, nt = spec[:3]
        opt = spec[3] if len(spec) > 3 else None
        if kind == "near":
            p = near_pair(nq, nt, ratio, floor, seed + i, min_d=opt)
        else:
            p = far_pair(nq, nt, ratio, floor, seed + i, tied=bool(opt == "tied"), seam=i)
        pairs.append((len(fr) + 1, len(fr), p))
        fr += [p.t, p.q]
        if i == 0 and empty:
            fr.append(np.zeros((0, 32), np.uint8))
    if duplicate and pairs:
        fr.append(fr[pairs[0][1]].copy())
    stride = max(max(len(f) for f in fr), 1)
    rows = np.zeros((len(fr), stride, 32), np.uint8)
    for i, f in enumerate(fr):
        rows[i, : len(f)] = f
    counts = np.array([len(f) for f in fr], np.int32)
    ids = np.arange(len(fr), dtype=np.int32) * 2
    return Frames(rows, counts, ids, pairs)
