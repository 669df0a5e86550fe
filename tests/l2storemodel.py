"""A plain-Python model of the SIFT keyframe store and a seeded stream of API calls over it (helper module, not a test file;
no device): tests/test_l2_store_model_host.py dry-runs the streams, tests/test_gpu_l2_store_sequences.py replays them on a
long-lived handle and compares every answer.

The model mirrors what lcm_l2_db.cpp keeps: the stored frames (rows, keypoints or None), the tiles they use, and the
capacities that lcm_l2_db_info reports - the arenas' (first exactly what is needed, then doubling until the request fits, a
staged host query included), the frame table's (64 entries, doubling) and whether the points arena exists.  Expected results
come from what the suite already trusts: l2ref.knn2 + ratio_filter over l2cases.distances_sq for counts, candidates and match
lists, a numpy gather compared on the bits for point pairs, src/main.cpp:1375-1388 restated as in l2countcases.loop_search_ref.
The verification's results are checked by verifychecks (closure on the device's own hypotheses, poseref bit for bit).

ops(seed, n_steps) depends on the seed and on the model alone, never on a device answer: the same stream can be dry-run
without a device and replayed on a second handle."""
from collections import namedtuple

import numpy as np

import epicases
import epiref
import l2cases as L
import l2countcases as K
import l2ref

TILE, SEG = K.TILE, K.SEG
ROW_CHOICES = (0, 1, 31, 32, 33, 64, 65, 100, 129, 256, 257, 300)
HOST_ROW_CHOICES = ROW_CHOICES + 2 * (256, 257, 300, 300)        # a host query is more often tall: the free tail is too small for it
MAX_FRAMES = 24
LIFT_FRAMES, LIFT_ROWS, LIFT_STEP = 70, (0, 1, 2, 3), 60      # the stretch that doubles the frame table under stored frames
TABLE_FIRST = 64
TILE_BYTES, PTS_TILE_BYTES, ENTRY_BYTES = 2 * 4096 + 128, 256, 8
AUTO_LARGE_ITEMS = 1024                                       # csrc/lcm_l2_host.h: l2_chunk_rows
RATIOS = (0.7, 0.75, 1.0, 1e30)
MIN_ROWS = (0, 1, 33)
MIN_MATCHES = (0, 8, 30)
ITERS = (128, 1024)
BIG_MATRIX = 700
SCENES = ((200, 60), (230, 70), (20, 10))                     # a family's (inliers, outliers): 260, 300 and 30 records
SPECIAL_EVERY, SPECIAL_FIRST = 40, 2                          # which generated frames carry NaN, -0.0 and all-ones keypoint bits

# The sequences the GPU file replays and the dry run pins (tests/test_l2_store_model_host.py): chosen so that every seed meets
# Coverage.check and the main seeds together reach every (verification call, edge) combination.
SEEDS, LIFT_SEED, STEPS = (4000, 4001, 4005, 4006, 4007, 4009), 4009, 250
TWIN_SEEDS, TWIN_STEPS = ((4013, 4017),), 120

DMATCH_DTYPE = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("img_idx", "<i4"), ("distance", "<f4")])
SCORE_DTYPE = K.SCORE_DTYPE

KINDS = ("append_kp", "append", "truncate", "clear", "read", "score_pairs", "match_pairs", "match_points", "match_points_plain",
         "loop_search", "detect_stored", "detect_host", "points_host", "points_stored", "epi_db", "pose_db", "lo_db", "lo_detect_host",
         "host_matrix", "hamming", "chunk", "cap_refusal", "replay")
WEIGHTS = {"append_kp": 5.0, "clear": 0.5}
RESULT_KINDS = ("score_pairs", "match_pairs", "match_points", "match_points_plain", "loop_search", "detect_stored", "detect_host",
                "points_host", "points_stored", "epi_db", "pose_db", "lo_db", "lo_detect_host")
VERIFY_KINDS = ("epi_db", "pose_db", "lo_db")
EDGES = ("few", "empty", "blocks")                            # a pair of < 8 records, an empty-side pair, > 256 records

Step = namedtuple("Step", "kind args frames info fallback")


def tiles(n):
    return -(-n // TILE)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Frame:
    """Rows uint8[n, 128], keypoints float32[n, 2] or None, and an identity for the reference cache."""
    __slots__ = ("rows", "pts", "uid")

    def __init__(self, rows, pts, uid):
        self.rows, self.pts, self.uid = rows, pts, uid
        rows.setflags(write=False)
        if pts is not None:
            pts.setflags(write=False)

    def __len__(self):
        return len(self.rows)

    def plain(self):
        return Frame(self.rows, None, self.uid)


# ---- the store ----------------------------------------------------------------------------------------------------------------
class Store:
    """What lcm_l2_db_info must report after every call."""

    def __init__(self):
        self.frames = []
        self.reserved = 0             # tiles_reserved
        self.table = 0                # entries of the device frame table
        self.points = False           # the points arena exists

    @property
    def used(self):
        return sum(tiles(len(f)) for f in self.frames)

    def reserve(self, need):
        """store_reserve: True when the arenas moved."""
        need = max(need, 1)
        if need <= self.reserved:
            return False
        cap = self.reserved or need
        while cap < need:
            cap *= 2
        self.reserved = cap
        return True

    def append(self, frame):
        grew = self.reserve(self.used + tiles(len(frame)))
        if len(self.frames) + 1 > self.table:
            self.table = max(2 * self.table, TABLE_FIRST)
        self.points |= frame.pts is not None
        self.frames.append(frame)
        return grew

    def stage(self, n_rows, with_points):
        """A host query of n_rows in the free tail: nothing is stored, the capacities may move."""
        grew = self.reserve(self.used + tiles(n_rows))
        self.points |= with_points
        return grew

    def truncate(self, n):
        assert 0 <= n <= len(self.frames)
        del self.frames[n:]

    def info(self):
        return dict(frames=len(self.frames), tiles_used=self.used, tiles_reserved=self.reserved,
                    device_bytes=self.reserved * (TILE_BYTES + (PTS_TILE_BYTES if self.points else 0)) + self.table * ENTRY_BYTES)


def reserved_sequence(row_counts):
    """tiles_reserved after each append of frames with these rows to a fresh store."""
    s, out = Store(), []
    for n in row_counts:
        s.append(Frame(np.zeros((n, 128), np.uint8), None, -1))
        out.append(s.reserved)
    return out


# ---- references ---------------------------------------------------------------------------------------------------------------
class Refs:
    """(l2ref.knn2, minimum squared distance) per (frame identity, frame identity), computed once."""

    def __init__(self):
        self.cache = {}

    def pair(self, q, t):
        key = (q.uid, t.uid)
        if key not in self.cache:
            D = L.distances_sq(q.rows, t.rows)
            self.cache[key] = (l2ref.knn2(q.rows, t.rows, D), int(D.min()))
        return self.cache[key]

    def score(self, q, t, ratio):
        """(good_count, min_dist_sq): l2countcases.ref_score."""
        if len(q) == 0 or len(t) == 0:
            return 0, K.NONE
        return K.ref_score(q.rows, t.rows, ratio, self.pair(q, t))

    def records(self, q, t, ratio):
        """DMATCH_DTYPE[n] of one pair: knn2 + ratio_filter, query order."""
        if len(q) == 0 or len(t) == 0:
            return np.zeros(0, DMATCH_DTYPE)
        (idx, dist, _), _ = self.pair(q, t)
        rows, train, d = l2ref.ratio_filter(idx, dist, ratio)
        out = np.zeros(len(rows), DMATCH_DTYPE)
        out["query_idx"], out["train_idx"], out["distance"] = rows, train, d
        return out


def want_scores(refs, sides, ratio):
    """SCORE_DTYPE[n] for [(query frame, train frame)]."""
    out = np.zeros(len(sides), SCORE_DTYPE)
    for k, (q, t) in enumerate(sides):
        out[k] = refs.score(q, t, ratio)
    return out


def want_lists(refs, sides, ratio, points):
    """(DMATCH_DTYPE[total], uint32[total, 4] point bits or None, offsets int64[n + 1]) for [(query frame, train frame)]."""
    recs = [refs.records(q, t, ratio) for q, t in sides]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    out = np.concatenate(recs) if recs else np.zeros(0, DMATCH_DTYPE)
    pts = None
    if points:
        parts = [np.concatenate([bits(q.pts)[r["query_idx"]], bits(t.pts)[r["train_idx"]]], axis=1) for (q, t), r in zip(sides, recs) if len(r)]
        pts = np.concatenate(parts) if parts else np.zeros((0, 4), np.uint32)
    return out, pts, offs


def want_search(refs, frames, gap, skip, ratio, min_rows, min_matches, currs=None, query=None):
    """src/main.cpp:1375-1388 over the stored frames: ([(curr, past, good, similarity)], pairs scored, the scored (query frame,
    train frame) sides).  currs: the outer loop's values (default: every stored one from gap on); query: a host frame that stands
    for the one `curr` given.  The caller has decided about :1377 for the currs it names."""
    S = len(frames)
    skip = [0] * S if skip is None else skip
    out, sides = [], []
    every = currs is None
    for curr in (range(gap, S) if every else currs):
        q = query if query is not None else frames[curr]
        if every and skip[curr]:
            continue
        for past in range(0, min(curr - gap, S - 1) + 1):
            if skip[past]:
                continue
            if len(q) < min_rows or len(frames[past]) < min_rows:
                continue
            sides.append((q, frames[past]))
            good = refs.score(q, frames[past], ratio)[0]
            if good < min_matches:
                continue
            den = min(len(q), len(frames[past]))
            out.append((curr, past, good, float(np.float64(good) / np.float64(den)) if den else 0.0))
    return out, len(sides), sides


def sides_of(frames, pairs):
    return [(frames[a], frames[b]) for a, b in pairs]


def want_detect(refs, frames, a, query=None):
    """One keyframe's search for the arguments a of a detect-form op: (candidates, pairs scored, scored sides, the candidates'
    (query frame, train frame) sides, whose lists the call makes)."""
    cands, scored, sides = want_search(refs, frames, a["gap"], a["skip"], a["ratio"], a["min_rows"], a["min_matches"], currs=[a["curr"]], query=query)
    q = query if query is not None else frames[a["curr"]]
    return cands, scored, sides, [(q, frames[c[1]]) for c in cands]


def verify_sides(refs, step):
    """The (query frame, train frame) sides whose records a verification step (VERIFY_KINDS) hands to the RANSAC."""
    a = step.args
    return sides_of(step.frames, a["pairs"]) if "pairs" in a else want_detect(refs, step.frames, a)[3]


def launch_of(sides, pin, form):
    """(pairs, distances, workgroups) of the launch record after a call over these sides; form: 'count' (searches and score
    calls: one item per query chunk) or 'list' (an item per query chunk and 512-row train segment).  None when nothing is live."""
    live = [(len(q), len(t)) for q, t in sides if len(q) and len(t)]
    if not live:
        return None
    per = (lambda nq, nt, ch: K.items(nq, ch)) if form == "count" else (lambda nq, nt, ch: K.items(nq, ch) * K.items(nt, SEG))
    ch = pin or (128 if sum(per(nq, nt, 256) for nq, nt in live) < AUTO_LARGE_ITEMS else 256)
    return len(live), sum(nq * nt for nq, nt in live), sum(per(nq, nt, ch) for nq, nt in live)


# ---- the comparisons: each raises AssertionError on a wrong answer --------------------------------------------------------------
def check_scores(got, want):
    assert len(got) == len(want), (len(got), len(want))
    np.testing.assert_array_equal(got["good_count"], want["good_count"])
    np.testing.assert_array_equal(got["min_dist_sq"], want["min_dist_sq"])


def check_candidates(got, n_pairs, want, want_pairs):
    assert n_pairs == want_pairs, (n_pairs, want_pairs)
    triples = [(int(c["current_frame_id"]), int(c["matched_frame_id"]), int(c["num_matches"])) for c in got]
    assert triples == [w[:3] for w in want], (triples, want)
    np.testing.assert_array_equal(np.asarray(got["similarity_score"]).view(np.uint64), np.array([w[3] for w in want], np.float64).view(np.uint64))


def check_lists(out, pts, offs, want):
    """Offsets, records and point bits of a list call, byte for byte."""
    w_out, w_pts, w_offs = want
    np.testing.assert_array_equal(np.asarray(offs).astype(np.int64), w_offs)
    assert len(out) == len(w_out)
    for name in DMATCH_DTYPE.names:
        np.testing.assert_array_equal(out[name].view(np.uint32), w_out[name].view(np.uint32), err_msg=name)
    if w_pts is None:
        assert pts is None
    else:
        assert pts is not None
        np.testing.assert_array_equal(bits(pts).reshape(-1, 4), w_pts)


def check_info(got, want):
    got = {k: int(getattr(got, k)) if not isinstance(got, dict) else int(got[k]) for k in want}
    assert got == want, (got, want)


def check_launch(got, want):
    """pairs, distances, workgroups and the route of the launch record (want: launch_of's triple)."""
    if want is not None:
        record = (int(got.pairs), int(got.distances), int(got.workgroups), int(got.route))
        assert record == (*want, 0), (record, want)


def edges_of(sides, offs):
    """Which of EDGES a verification call's pairs reach, from the offsets it returned."""
    n = np.diff(np.asarray(offs).astype(np.int64))
    out = set()
    for (q, t), k in zip(sides, n):
        if len(q) == 0 or len(t) == 0:
            out.add("empty")
        elif k < 8:
            out.add("few")
        if k > 256:
            out.add("blocks")
    return out


# ---- frames -------------------------------------------------------------------------------------------------------------------
class Family:
    """One two-view scene and a descriptor row per scene record."""

    def __init__(self, rng, n_in, n_out, seed):
        self.pts, _ = epiref.make_scene(n_in, n_out, seed)
        self.pool = rng.integers(0, 256, (len(self.pts), l2ref.SIFT_BYTES), dtype=np.uint8)


class Frames:
    """The frame generator of one seed: frames of two or three families, and every SPECIAL_EVERY-th one with hostile bits."""

    def __init__(self, rng, seed):
        self.rng = rng
        self.families = [Family(rng, *SCENES[k], 1000 * seed + k) for k in range(2 + seed % 2)] + [Family(rng, *SCENES[2], 1000 * seed + 7)]
        self.made = 0

    def make(self, n, uid):
        rng = self.rng
        special = self.made % SPECIAL_EVERY == SPECIAL_FIRST
        self.made += 1
        rows = K.mixed(rng, n)
        pts = np.stack([rng.uniform(0.0, 640.0, n), rng.uniform(0.0, 480.0, n)], axis=1).astype(np.float32)
        if special:
            b = pts.view(np.uint32)
            b[0::4, 0] = 0x7FC12345                   # quiet NaN with a payload
            b[1::4, 1] = 0x80000000                   # -0.0
            b[2::4, 0] = 0x7F800001                   # signalling NaN
            b[3::4, 1] = 0xFFFFFFFF
        elif n and rng.random() < 0.85:
            fam = self.families[int(rng.integers(len(self.families)))]
            view = int(rng.integers(2))
            k = min(n, len(fam.pts), max(1, int(n * rng.choice((0.1, 0.5, 0.9, 1.0)))))
            rec = rng.choice(len(fam.pts), k, replace=False)
            at = rng.choice(n, k, replace=False)
            for r, i in zip(rec, at):
                rows[i] = L.near_copy(rng, fam.pool[r], int(rng.integers(1, 5)))
            pts[at] = fam.pts[rec, 2 * view: 2 * view + 2]
        return Frame(rows, pts, uid)


# ---- the op stream ------------------------------------------------------------------------------------------------------------
class Stream:
    """ops(): Steps of (kind, arguments, the stored frames after the step, the predicted lcm_l2_db_info, whether the drawn op fell
    back to append_kp).  Arguments name slots and carry host frames; expectations are computed by whoever runs the stream."""

    def __init__(self, seed, n_steps, lift=False):
        self.seed, self.n_steps, self.lift = seed, n_steps, lift
        self.rng = np.random.default_rng(seed)
        self.store = Store()
        self.gen = Frames(self.rng, seed)
        self.uid = 0
        self.recent = []                              # result-bearing calls whose slots are still stored
        self.lifting = self.lift_searched = False
        self.grew = False                             # the last step moved the arenas

    # -- helpers --
    def new_uid(self):
        self.uid += 1
        return self.uid

    def frame(self, choices=ROW_CHOICES):
        return self.gen.make(int(self.rng.choice(choices)), self.new_uid())

    def pointed(self):
        """Slots a call that wants points may name: stored with points, or empty."""
        return [k for k, f in enumerate(self.store.frames) if f.pts is not None or len(f) == 0]

    def with_points(self):
        return [k for k, f in enumerate(self.store.frames) if f.pts is not None and len(f)]

    def pairs(self, slots, verify=False):
        """1 ... 12 (query, train) pairs over `slots`: self pairs, repeats, and an empty side where there is one."""
        rng = self.rng
        n = int(rng.integers(1, 13))
        out = [(int(rng.choice(slots)), int(rng.choice(slots))) for _ in range(n)]
        if n > 1 and rng.random() < 0.4:
            out[int(rng.integers(n))] = out[0]                                  # a repeat
        if rng.random() < 0.4:
            k = int(rng.choice(slots))
            out[int(rng.integers(n))] = (k, k)                                  # a self pair
        empty = [k for k in slots if len(self.store.frames[k]) == 0]
        if empty and rng.random() < (0.8 if verify else 0.4):
            k, other = int(rng.choice(empty)), int(rng.choice(slots))
            out[int(rng.integers(n))] = (k, other) if rng.random() < 0.5 else (other, k)
        return out

    def search_args(self, pointed_only=False):
        """pointed_only: the search skips every slot a call that wants points may not name."""
        rng = self.rng
        S = len(self.store.frames)
        skip = None
        if pointed_only or rng.random() < 0.5:
            skip = [int(rng.random() < 0.2) for _ in range(S)]
            if pointed_only:
                ok = set(self.pointed())
                skip = [1 if k not in ok else s for k, s in enumerate(skip)]
        return dict(gap=int(rng.integers(1, 5)), skip=skip, ratio=float(rng.choice(RATIOS)), min_rows=int(rng.choice(MIN_ROWS)),
                    min_matches=int(rng.choice(MIN_MATCHES)))

    def epi(self):
        rng = self.rng
        return dict(iters=int(rng.choice(ITERS)), seed=int(rng.choice(epicases.SEEDS)))

    def lo(self):
        return None if self.rng.random() < 0.5 else (1.0,)

    def floor(self):
        return -1 if self.rng.random() < 0.5 else int(self.rng.integers(0, 200))

    # -- the draw --
    def possible(self, kind):
        S, wp = len(self.store.frames), len(self.with_points())
        if kind in ("truncate", "clear", "read", "score_pairs", "match_pairs", "match_points_plain", "detect_host"):
            return S >= 1
        if kind in ("loop_search", "detect_stored"):
            return S >= 2
        if kind in ("match_points", "points_stored", "epi_db", "pose_db", "lo_db", "points_host"):
            return wp >= 2
        if kind == "lo_detect_host":
            return wp >= 1
        if kind == "cap_refusal":
            return any(len(self.store.frames[a]) >= 1 and len(self.store.frames[b]) >= 2 for a in self.with_points() for b in self.with_points())
        if kind == "replay":
            return len(self.recent) >= 1
        return True

    def draw(self):
        w = np.array([WEIGHTS.get(k, 1.0) for k in KINDS])
        return KINDS[int(self.rng.choice(len(KINDS), p=w / w.sum()))]

    def build(self, kind):
        """The arguments of one op; the store is moved for the ops that store, truncate or stage."""
        rng, st = self.rng, self.store
        S = len(st.frames)
        self.grew = False
        if kind in ("append_kp", "append"):
            f = self.frame(LIFT_ROWS if self.lifting else ROW_CHOICES)
            limit = LIFT_FRAMES if self.lifting else MAX_FRAMES
            if S >= limit:                                                      # an append above the limit becomes a truncate
                kind = "truncate"
            else:
                f = f if kind == "append_kp" else f.plain()
                self.grew = st.append(f)
                self.recent = [(k, a) for k, a in self.recent if a.get("skip") is None]      # a skip vector is one flag per stored slot
                return kind, dict(frame=f)
        if kind == "truncate":
            n = int(rng.integers(0, min(S, 20) if self.lifting else S))
            st.truncate(n)
            self.recent = []
            return kind, dict(n=n)
        if kind == "clear":
            st.truncate(0)
            self.recent = []
            return kind, {}
        if kind == "read":
            return kind, dict(slot=int(rng.integers(S)))
        if kind in ("score_pairs", "match_pairs", "match_points_plain"):
            return kind, dict(pairs=self.pairs(list(range(S))), ratio=float(rng.choice(RATIOS)))
        if kind == "match_points":
            return kind, dict(pairs=self.pairs(self.pointed()), ratio=float(rng.choice(RATIOS)))
        if kind == "loop_search":
            return kind, self.search_args()
        if kind == "detect_stored":
            return kind, dict(curr=int(rng.integers(1, S)), **self.search_args())
        if kind == "points_stored":
            return kind, dict(curr=int(rng.choice(self.with_points())), points=bool(rng.random() < 0.7), **self.search_args(pointed_only=True))
        if kind in ("detect_host", "points_host", "lo_detect_host"):
            q = self.frame(HOST_ROW_CHOICES)
            a = dict(curr=S, query=q, **self.search_args(pointed_only=kind != "detect_host"))
            if kind == "points_host":
                a["points"] = True
            if kind == "lo_detect_host":
                a.update(ep=self.epi(), lp=self.lo(), floor=self.floor())
            self.grew = st.stage(len(q), kind != "detect_host")
            return kind, a
        if kind in VERIFY_KINDS:
            a = dict(ep=self.epi(), ratio=float(rng.choice(RATIOS)))
            if kind != "lo_db" and rng.random() < 0.5:                          # the detect_loops form, on a stored slot
                a.update(curr=int(rng.choice(self.with_points())), **self.search_args(pointed_only=True))
                if kind == "pose_db":
                    a["floor"] = self.floor()
            else:
                a["pairs"] = self.pairs(self.pointed(), verify=True)
                if kind == "lo_db":
                    a["lp"] = self.lo()
            return kind, a
        if kind == "host_matrix":
            call = str(rng.choice(("score_pairs_ratio_l2", "match_pairs_ratio_l2", "knn2_pair_l2", "epi_verify_pairs", "lo_verify_pairs")))
            big = bool(rng.random() < 1 / 3)
            if call in ("epi_verify_pairs", "lo_verify_pairs"):
                n = BIG_MATRIX if big else int(rng.choice((7, 40, 260)))
                pts, _ = epiref.make_scene(n - n // 4, n // 4, int(rng.integers(1 << 20)))
                return kind, dict(call=call, pts=pts, ep=self.epi())
            mats = [Frame(K.mixed(rng, BIG_MATRIX if big else int(rng.choice(ROW_CHOICES))), None, self.new_uid()) for _ in range(2)]
            return kind, dict(call=call, mats=mats, ratio=float(rng.choice(RATIOS)))
        if kind == "hamming":
            return kind, dict(q=rng.integers(0, 256, (int(rng.integers(1, 90)), 32), dtype=np.uint8),
                              t=rng.integers(0, 256, (int(rng.integers(2, 90)), 32), dtype=np.uint8), ratio=float(rng.choice((0.7, 0.9))))
        if kind == "chunk":
            pick = lambda: (None, 128, 256)[int(rng.integers(3))]
            return kind, dict(list=pick(), count=pick())
        if kind == "cap_refusal":
            wp = self.with_points()
            ok = [(a, b) for a in wp for b in wp if len(st.frames[b]) >= 2]
            a, b = ok[int(rng.integers(len(ok)))]
            plain = [k for k, f in enumerate(st.frames) if f.pts is None and len(f)]
            forms = ("match_points", "epi_db") + (("cand_cap",) if len(wp) >= 2 else ()) + (("no_points",) if plain else ())
            form = str(rng.choice(forms))
            out = dict(form=form, pair=(a, b), ep=self.epi())
            if form == "no_points":
                out["plain"] = int(rng.choice(plain))
            return kind, out
        if kind == "replay":
            calls = list(self.recent[-3:])
            for k, a in calls:                                                  # a host query is staged again
                if "query" in a:
                    self.grew |= st.stage(len(a["query"]), k != "detect_host")
            return kind, dict(calls=calls)
        raise AssertionError(kind)

    def ops(self):
        for step in range(self.n_steps):
            fallback = False
            if self.lift and step == LIFT_STEP:
                self.lifting = True
            if self.lifting and len(self.store.frames) >= LIFT_FRAMES:      # the table has doubled: one search, then back
                kind, args = self.build("truncate" if self.lift_searched else "loop_search")
                self.lifting, self.lift_searched = not self.lift_searched, True
            else:
                kind = self.draw()
                if self.lifting and kind in ("truncate", "clear"):
                    kind = "append"
                elif self.lifting and self.rng.random() < 0.7:
                    kind = "append_kp" if self.rng.random() < 0.5 else "append"
                if not self.possible(kind):
                    kind, fallback = "append_kp", True
                kind, args = self.build(kind)
            yield self.emit(kind, args, fallback)

    def emit(self, kind, args, fallback):
        if kind in RESULT_KINDS:
            self.recent.append((kind, args))
        return Step(kind, args, tuple(self.store.frames), dict(self.store.info(), grew=self.grew), fallback)


def ops(seed, n_steps, lift=False):
    return Stream(seed, n_steps, lift).ops()


# ---- what a run reached ---------------------------------------------------------------------------------------------------------
class Coverage:
    """Counts what a run of a stream reached, from the executed steps and the lcm_l2_db_info values the runner saw (the model's
    in the dry run, the device's on the GPU)."""

    def __init__(self):
        self.kinds, self.fallbacks, self.steps = {}, 0, 0
        self.growths_with_points = self.growths_staged = 0
        self.reused = self.plain_over_points = 0
        self.table_doubled = self.points = False
        self.edges = set()                            # (verification kind, edge)
        self.slots = []                               # (first tile, tiles, has points) per stored frame
        self.freed = 0                                # tiles below this held a frame that was truncated or cleared ...
        self.freed_points = 0                         # ... and below this one with points, since the arenas last moved

    def step(self, s, before, after):
        """s: the Step; before / after: dicts with tiles_used, tiles_reserved, device_bytes, frames as the runner read them."""
        self.steps += 1
        self.kinds[s.kind] = self.kinds.get(s.kind, 0) + 1
        self.fallbacks += bool(s.fallback)
        grew = after["tiles_reserved"] != before["tiles_reserved"]
        stored_points = any(p for _, _, p in self.slots)
        if grew and before["tiles_reserved"]:
            self.growths_with_points += stored_points
            self.growths_staged += s.kind in ("detect_host", "points_host", "lo_detect_host")
        if grew:                                      # the new arenas hold the used tiles only
            self.freed = self.freed_points = 0
        if s.kind in ("append_kp", "append"):
            first, n = before["tiles_used"], after["tiles_used"] - before["tiles_used"]
            if n and first < self.freed:
                self.reused += 1
                self.plain_over_points += s.kind == "append" and first < self.freed_points
            self.slots.append((first, n, s.kind == "append_kp"))
        elif s.kind in ("truncate", "clear"):
            keep = after["frames"]
            for first, n, p in self.slots[keep:]:
                self.freed = max(self.freed, first + n)
                if p:
                    self.freed_points = max(self.freed_points, first + n)
            del self.slots[keep:]
        brings_points = ("append_kp", "points_host", "lo_detect_host")
        self.points |= s.kind in brings_points or (s.kind == "replay" and any(k in brings_points for k, _ in s.args["calls"]))
        table = (after["device_bytes"] - after["tiles_reserved"] * (TILE_BYTES + (PTS_TILE_BYTES if self.points else 0))) // ENTRY_BYTES
        self.table_doubled |= table > TABLE_FIRST and after["frames"] > TABLE_FIRST

    def verified(self, kind, sides, offs):
        self.edges |= {(kind, e) for e in edges_of(sides, offs)}

    def summary(self):
        return dict(fallbacks=self.fallbacks, growths_with_points=self.growths_with_points, growths_staged=self.growths_staged,
                    reused=self.reused, plain_over_points=self.plain_over_points, table_doubled=self.table_doubled)

    def check(self, lift):
        """The per-seed conditions the sequences are there for."""
        missing = [k for k in KINDS if not self.kinds.get(k)]
        assert not missing, missing
        assert self.fallbacks * 10 <= self.steps, (self.fallbacks, self.steps)
        assert self.growths_with_points >= 2 and self.growths_staged >= 1, self.summary()
        assert self.reused >= 10 and self.plain_over_points >= 1, self.summary()
        assert self.table_doubled == lift, self.summary()


def describe(step):
    """A step's arguments without its arrays, for a failure message."""
    def short(v):
        if isinstance(v, (Frame, np.ndarray)):
            return f"<{len(v)} rows>"
        return [short(x) for x in v] if isinstance(v, list) and v and isinstance(v[0], Frame) else v

    return {k: (short(v) if k != "calls" else [c[0] for c in v]) for k, v in step.args.items()}


def dry_run(seed, n_steps, lift=False, refs=None):
    """The stream without a device: the Coverage it must reach, from the model's own lcm_l2_db_info and the references' record
    counts.  Asserts what the GPU file relies on beyond that: a refusal's call has at least one record or candidate to refuse."""
    refs = Refs() if refs is None else refs
    cov, before = Coverage(), Store().info()
    for s in ops(seed, n_steps, lift):
        after = {k: v for k, v in s.info.items() if k != "grew"}
        assert (after["tiles_reserved"] != before["tiles_reserved"]) == s.info["grew"] and after["tiles_used"] <= after["tiles_reserved"]
        cov.step(s, before, after)
        before = after
        if s.kind in VERIFY_KINDS:
            sides = verify_sides(refs, s)
            cov.verified(s.kind, sides, want_lists(refs, sides, s.args["ratio"], False)[2])
        if s.kind == "cap_refusal" and s.args["form"] in ("match_points", "epi_db"):
            a, b = s.args["pair"]
            assert len(refs.records(s.frames[a], s.frames[b], 1e30)) >= 1
    return cov
