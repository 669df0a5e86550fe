"""Reference for the ratio-scored loop test (helper module, not a test file): the reference's own loop rule
(src/main.cpp:1379-1388) in numpy on top of ratioref.ratio_counts, and the frame sets the GPU tests use.

A pair (current frame c, stored frame s, id_c - id_s >= max(gap, 1)) is a loop candidate iff
    rows_c >= min_rows and rows_s >= min_rows and good_count(c, s, ratio) >= min_matches
and its record is (id_c, id_s, good_count, float64(good_count) / float64(min(rows_c, rows_s))) — 0.0 when that minimum
is 0 (possible only with min_rows = 0).  Order: (current, matched) ascending.

Planting: every frame of a set holds `flip(B[j], 5)` for j < k of one shared pool B of random rows, plus random rows of
its own.  Two frames' copies of B[j] are at most 10 bits apart, every other row is ~128 +- 8 bits away, so at ratio 0.7
exactly the planted rows survive: good_count(c, s) = min(k_c, k_s) when the stored frame has two rows or more.  `expected`
never assumes that — it computes the count — and `planted_count` is what the tests compare it with."""
import numpy as np

import knnref
import ratioref

DEFAULTS = (0.7, 100, 300)            # src/main.cpp:1386, :1382, :1388


def rnd(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flip(rng, row, k):
    """`row` with exactly k of its 256 bits flipped."""
    m = np.zeros(256, np.uint8)
    m[rng.choice(256, int(k), replace=False)] = 1
    return row ^ np.packbits(m, bitorder="little")


def similarity(good, rows_c, rows_s):
    den = min(int(rows_c), int(rows_s))
    return np.float64(good) / np.float64(den) if den > 0 else np.float64(0.0)


def verdict(good, rows_c, rows_s, min_rows, min_matches):
    """(rows_c ok, rows_s ok, count ok): a candidate iff all three."""
    return rows_c >= min_rows, rows_s >= min_rows, good >= min_matches


class Ref:
    """good_count of every eligible pair of `frames` (list of (id, rows), the database) and `queries` (default: the
    frames themselves), computed once per (pair, ratio) and shared by everything that asks."""

    def __init__(self, frames, queries=None):
        self.frames = frames
        self.queries = frames if queries is None else queries
        self.knn, self.cnt = {}, {}

    def count(self, c, s, ratio):
        if (c, s, ratio) not in self.cnt:
            q, t = self.queries[c][1], self.frames[s][1]
            if len(q) and len(t) and (c, s) not in self.knn:
                self.knn[(c, s)] = knnref.knn2(q, t)
            self.cnt[(c, s, ratio)] = ratioref.ratio_counts(q, t, ratio, self.knn.get((c, s)))[0]
        return self.cnt[(c, s, ratio)]

    def pairs(self, gap):
        """eligible (c, s) in (query ascending, stored ascending) order"""
        return [(c, s) for c, (qid, _) in enumerate(self.queries) for s, (fid, _) in enumerate(self.frames)
                if qid - fid >= max(gap, 1)]

    def expected(self, gap, ratio, min_rows, min_matches, only_query=None):
        """the candidate list [(current id, matched id, good_count, similarity)], in order"""
        out = []
        for c, s in self.pairs(gap):
            if only_query is not None and c != only_query:
                continue
            rc, rs = len(self.queries[c][1]), len(self.frames[s][1])
            good = self.count(c, s, ratio)
            if all(verdict(good, rc, rs, min_rows, min_matches)):
                out.append((int(self.queries[c][0]), int(self.frames[s][0]), int(good), similarity(good, rc, rs)))
        return out

    def classes(self, gap, ratio, min_rows, min_matches):
        """per eligible pair: ((rows_c ok, rows_s ok, count ok), good_count)"""
        return [(verdict(self.count(c, s, ratio), len(self.queries[c][1]), len(self.frames[s][1]), min_rows, min_matches),
                 self.count(c, s, ratio)) for c, s in self.pairs(gap)]


def planted_frames(seed, spec, ids=None):
    """spec: list of (rows, k planted) -> list of (id, rows) with frame f holding flip(B[j], 5), j < k_f, at random places
    among random rows."""
    rng = np.random.default_rng(seed)
    pool = rnd(rng, max([k for _, k in spec] + [1]))
    frames = []
    for f, (n, k) in enumerate(spec):
        assert k <= n
        rows = rnd(rng, n)
        where = rng.permutation(n)[:k]
        for j, r in enumerate(where):
            rows[r] = flip(rng, pool[j], 5)
        frames.append((f if ids is None else int(ids[f]), rows))
    return frames


def planted_count(spec, c, s):
    """what the planting makes good_count(c, s) at ratio 0.7 (stored frame of two rows or more)"""
    return min(spec[c][1], spec[s][1]) if spec[s][0] >= 2 and spec[c][0] >= 1 else 0


# ---- the frame sets of the GPU tests ----------------------------------------------------------------------------------

# boundaries: 39 / 40 / 41 rows on either side, planted counts 11 / 12 / 13, under min_rows = 40, min_matches = 12
BOUNDARY_RP = (0.7, 40, 12)
BOUNDARY_SPEC = [(39, 13), (40, 12), (41, 13), (40, 11), (41, 13), (39, 13), (40, 13), (160, 13), (20, 13), (57, 0), (41, 12)]

# the reference's own values: two frames of 330 rows with 300 planted, one with 299, a 99-row frame that a later frame
# matches 300 times (several query rows per stored row), the rest random
DEFAULT_SPEC = [(330, 300), (330, 300), (330, 299), (120, 0), (330, 300), (101, 0)]


def default_frames():
    frames = planted_frames(901, DEFAULT_SPEC)
    rng = np.random.default_rng(902)
    short = rnd(rng, 99)                                          # id 6: 99 rows
    many = rnd(rng, 330)                                          # id 7: 300 of its rows are near copies of `short`'s
    for r in range(300):
        many[r] = flip(rng, short[r % 99], 5)
    return frames + [(6, short), (7, many[rng.permutation(330)])]


# a group's database: 11 frames of 0..160 rows, one of them empty (uneven shards for W = 2, 3, 4)
GROUP_RP = (0.7, 40, 12)
GROUP_SPEC = [(39, 13), (160, 14), (40, 12), (0, 0), (41, 13), (40, 11), (96, 13), (20, 13), (41, 12), (64, 0), (57, 13)]
GROUP_EXTRA_SPEC = GROUP_SPEC + [(48, 13), (40, 12)]            # ... and the two frames appended later


def tiny_set(seed, n_query, n_stored):
    """Compaction sets: frames of 1..4 rows.  Returns (stored frames, query frames with ids 1000 + c): every query frame
    sees every stored frame, n_query * n_stored pairs.  At ratio 1.0 a query row survives iff its two nearest stored rows
    differ in distance: a stored frame of one row, or of copies of one row, gives good_count = 0."""
    rng = np.random.default_rng(seed)
    stored = []
    for s in range(n_stored):
        n = int(rng.integers(1, 5))
        rows = rnd(rng, n)
        if rng.random() < 0.4:
            rows[:] = rows[0]                                     # dead: second == best for every query row
        stored.append((s, rows))
    queries = [(1000 + c, rnd(rng, int(rng.integers(1, 5)))) for c in range(n_query)]
    return stored, queries


TINY_SHAPES = {255: (15, 17), 256: (16, 16), 257: (1, 257), 1025: (25, 41)}     # n_pairs -> (query frames, stored frames)
TINY_RPS = ((1.0, 0, 0), (1.0, 0, 1), (1.0, 3, 1))              # every pair; a subset by count; ... and by rows on either side
