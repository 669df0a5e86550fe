"""A plain-Python model of the 32-byte ORB database and a seeded stream of API calls over its two-neighbour and ratio-scored
routes (helper module, not a test file; no device): tests/test_ratio_model_host.py dry-runs the streams,
tests/test_gpu_ratio_sequences.py replays them on a long-lived handle and compares every answer.

The model is ids, frames, min_gap and cross_check; a stored frame s is eligible for a query id q iff q - id_s >= max(gap, 1).
Expectations come from knnref (knn2, ratio_filter), ratioref (ratio_counts) and ratioloopref's rule alone: expected(step, refs)
gives a step's outputs as a list of (tag, value), the runner on the device returns the same list, check_outputs compares them.
Coverage counts what a run reached from the steps and the outputs it is given - the model's in the dry run, the device's on the
GPU - so both must arrive at the same figures.

ops(seed, n_steps) depends on the seed and on the model alone, never on a device answer."""
from collections import namedtuple

import numpy as np

import knnref
import ratioloopref as R
import ratioref

MAX_ROWS = 140
ROW_CHOICES = (0, 1, 2, 3, 17, 64, 65, 100, MAX_ROWS)
MAX_FRAMES = 32
EXT_MAX = 6                                                  # frames of the external query set's device buffer
POOL = 40
RATIOS = (0.0, 0.5, 0.7, 0.75, 1.0, 1.5, 1e30)
EMPTY_MIN = ratioref.EMPTY_MIN

# The sequences the GPU file replays and the dry run pins (tests/test_ratio_model_host.py)
SEEDS, STEPS = (5107, 5113, 5117, 5126, 5140, 5145), 250
TWIN_SEEDS, TWIN_STEPS = ((5150, 5162),), 120
GROUP_RUNS, GROUP_STEPS = ((2, 5204), (3, 5205), (8, 5207)), 120

SCORE_DTYPE = np.dtype([("good_count", "<u4"), ("min_dist", "<u2"), ("n_train", "<u2")])
DMATCH_DTYPE = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("img_idx", "<i4"), ("distance", "<f4")])
CANDIDATE_DTYPE = np.dtype([("current_frame_id", "<i4"), ("matched_frame_id", "<i4"), ("num_matches", "<i4"), ("_pad", "<i4"),
                            ("similarity_score", "<f8")])

KINDS = ("append", "append_dev", "truncate", "clear", "snapshot", "params", "variant", "tuning",
         "bulk_self", "bulk_ext", "loops_self", "loops_ext", "loops_cap", "rewind", "classic", "classic_loops",
         "query_host", "detect_host", "detect_stored", "tickets",
         "stored_ratio", "stored_batch_ratio", "query_batch_ratio", "knn2_pair", "features_ratio", "classic_pair", "replay")
WEIGHTS = {"append": 4.0, "clear": 0.4, "snapshot": 0.6, "variant": 0.6, "bulk_self": 1.5, "loops_self": 1.5, "classic_loops": 1.5,
           "rewind": 0.6, "tickets": 0.8}
# the C entry point a ratio kind calls: under cross_check != 0 the step is that call's refusal
ENTRY = {"bulk_self": "lcm_all_vs_all_ratio", "bulk_ext": "lcm_all_vs_all_ratio", "loops_self": "lcm_all_vs_all_loops_ratio",
         "loops_ext": "lcm_all_vs_all_loops_ratio", "loops_cap": "lcm_all_vs_all_loops_ratio", "query_host": "lcm_query_scores_ratio",
         "detect_host": "lcm_detect_loops_ratio", "detect_stored": "lcm_detect_loops_ratio", "stored_ratio": "lcm_match_stored_ratio",
         "stored_batch_ratio": "lcm_match_stored_batch_ratio", "query_batch_ratio": "lcm_match_query_batch_ratio",
         "knn2_pair": "lcm_knn2_pair", "features_ratio": "lcm_match_features_ratio"}
ENTRY_POINTS = tuple(sorted(set(ENTRY.values())))
NOT_UNDER_CROSS = ("rewind", "tickets", "replay")                  # composite steps: drawn only while cross_check = 0
REPLAYED = ("bulk_self", "loops_self", "query_host", "detect_host", "detect_stored", "stored_ratio", "stored_batch_ratio",
            "query_batch_ratio")

Step = namedtuple("Step", "kind args ids frames gap cross slots fallback")
ExtSet = namedtuple("ExtSet", "ids frames bases rewrite")          # rewrite: 'new' (rows, counts, ids), 'counts' / 'ids' (only those), 'keep'


class Frame:
    """Rows uint8[n, 32] and an identity for the reference cache."""
    __slots__ = ("rows", "uid")

    def __init__(self, rows, uid):
        self.rows, self.uid = np.ascontiguousarray(rows, np.uint8).reshape(-1, 32), uid
        self.rows.setflags(write=False)

    def __len__(self):
        return len(self.rows)


# ---- references ---------------------------------------------------------------------------------------------------------------
class Refs:
    """knnref.knn2 per (frame identity, frame identity), computed once, and what each pair is an example of."""

    def __init__(self):
        self.knn, self.cnt, self.flags = {}, {}, {}
        self.watch = None                                        # a Coverage that wants to know which pairs were asked for

    def pair(self, q, t):
        key = (q.uid, t.uid)
        if key not in self.knn:
            idx, dist = knnref.knn2(q.rows, t.rows)
            self.knn[key] = (idx, dist)
            f = set()
            if len(idx):
                if (idx[:, 1] == knnref.NO_IDX).any():
                    f.add("no_second")
                else:
                    f |= {name for name, d in (("d2_zero", 0), ("d2_256", 256)) if (dist[:, 1] == d).any()}
            self.flags[key] = f
        if self.watch is not None:
            self.watch.seen |= self.flags[key]
        return self.knn[key]

    def record(self, q, t, ratio):
        """(good_count, min_dist, n_train): ratioref.ratio_counts; an empty side's record as tests/test_gpu_ratio_scores.py has it."""
        if len(q) == 0 or len(t) == 0:
            return 0, EMPTY_MIN, len(t)
        key = (q.uid, t.uid, ratio)
        if key not in self.cnt:
            self.cnt[key] = ratioref.ratio_counts(q.rows, t.rows, ratio, self.pair(q, t))
        elif self.watch is not None:
            self.watch.seen |= self.flags[key[:2]]
        return (*self.cnt[key], len(t))

    def matches(self, q, t, ratio):
        """DMATCH_DTYPE[n] of one pair: knn2 + ratio_filter, query order."""
        if len(q) == 0 or len(t) == 0:
            return np.zeros(0, DMATCH_DTYPE)
        rows, train, d = knnref.ratio_filter(*self.pair(q, t), ratio)
        out = np.zeros(len(rows), DMATCH_DTYPE)
        out["query_idx"], out["train_idx"], out["distance"] = rows, train, d
        return out


def elig(ids, qid, gap):
    return [s for s, sid in enumerate(ids) if qid - sid >= max(gap, 1)]


def want_records(refs, ids, frames, gap, ratio, q_ids=None, q_frames=None):
    """(SCORE_DTYPE[n], offsets[n_q + 1], [(query position, stored slot)]) in (query ascending, stored ascending) order."""
    q_ids, q_frames = (ids, frames) if q_ids is None else (q_ids, q_frames)
    recs, offs, pairs = [], [0], []
    for c, qid in enumerate(q_ids):
        for s in elig(ids, qid, gap):
            recs.append(refs.record(q_frames[c], frames[s], ratio))
            pairs.append((c, s))
        offs.append(len(recs))
    out = np.zeros(len(recs), SCORE_DTYPE)
    for k, r in enumerate(recs):
        out[k] = r
    return out, offs, pairs


def want_cands(recs, pairs, ids, frames, rp, q_ids=None, q_frames=None):
    """CANDIDATE_DTYPE[n] by ratioloopref's rule and order; rp: (ratio, min_rows, min_matches) or None (the defaults)."""
    q_ids, q_frames = (ids, frames) if q_ids is None else (q_ids, q_frames)
    _, min_rows, min_matches = R.DEFAULTS if rp is None else rp
    keep = []
    for (c, s), r in zip(pairs, recs):
        rc, rs, good = len(q_frames[c]), len(frames[s]), int(r["good_count"])
        if all(R.verdict(good, rc, rs, min_rows, min_matches)):
            keep.append((int(q_ids[c]), int(ids[s]), good, 0, R.similarity(good, rc, rs)))
    out = np.zeros(len(keep), CANDIDATE_DTYPE)
    for k, c in enumerate(keep):
        out[k] = c
    return out


def want_lists(refs, sides, ratio):
    """(DMATCH_DTYPE[total], offsets[n + 1]) for [(query frame, train frame)]."""
    recs = [refs.matches(q, t, ratio) for q, t in sides]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    return (np.concatenate(recs) if recs else np.zeros(0, DMATCH_DTYPE)), offs


def launch_bulk(ids, frames, gap, slots, q_ids=None, q_frames=None):
    """(pairs, distances, workgroups) of the launch record after a bulk ratio search, None when it has no pair.  An item holds
    `slots` stored frames of one query frame (the pinned ITEM_SLOTS, else one: every search here is below 4096 pairs)."""
    q_ids, q_frames = (ids, frames) if q_ids is None else (q_ids, q_frames)
    chunk = slots if slots >= 1 else 1
    pairs = dist = wgs = 0
    for c, qid in enumerate(q_ids):
        e = elig(ids, qid, gap)
        pairs += len(e)
        dist += len(q_frames[c]) * sum(len(frames[s]) for s in e)
        wgs += -(-len(e) // chunk)
    return (pairs, dist, wgs) if pairs else None


def launch_online(ids, frames, gap, qid, nq):
    """... after the online ratio query: one workgroup per eligible frame (the library puts 2 or 4 frames into one from 4096 /
    8192 eligible frames on, which a database of MAX_FRAMES never has)."""
    e = elig(ids, qid, gap)
    return (len(e), nq * sum(len(frames[s]) for s in e), len(e)) if e else None


# ---- the comparisons: each raises AssertionError on a wrong answer --------------------------------------------------------------
def check_records(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in SCORE_DTYPE.names:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)


def check_cands(got, want):
    """Every field of every candidate, the similarity on its bits and the padding word included."""
    got = np.ascontiguousarray(got)
    assert got.dtype == CANDIDATE_DTYPE and len(got) == len(want), (len(got), len(want))
    for f in ("current_frame_id", "matched_frame_id", "num_matches", "_pad"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    np.testing.assert_array_equal(got["similarity_score"].view(np.uint64), want["similarity_score"].view(np.uint64), err_msg="similarity")


def check_lists(got, want):
    (out, offs), (w_out, w_offs) = got, want
    np.testing.assert_array_equal(np.asarray(offs).astype(np.int64), w_offs)
    assert len(out) == len(w_out), (len(out), len(w_out))
    for name in DMATCH_DTYPE.names:
        np.testing.assert_array_equal(out[name].view(np.uint32), w_out[name].view(np.uint32), err_msg=name)


def check_knn2(got, want):
    for g, w, name in zip(got, want, ("train_idx", "dist")):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=name)


def check_launch(got, want):
    """pairs, distances, workgroups and the plain route; None on both sides: the call launched nothing."""
    assert (got is None) == (want is None), (got, want)
    if want is None:
        return
    if not isinstance(got, tuple):
        got = (int(got.pairs), int(got.distances), int(got.workgroups), int(got.route))
    pairs, dist, wgs = want
    assert got[:3] == (pairs, dist, wgs) and got[3] == 0, (got, want)


def check_equal(got, want):
    assert np.array_equal(np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)), (got, want)


CHECKS = {"records": check_records, "bulk": check_records, "cands": check_cands, "list": check_lists, "knn2": check_knn2,
          "launch": check_launch, "offsets": check_equal, "ids": check_equal, "n": check_equal, "refused": check_equal}


def check_outputs(got, want):
    assert [t for t, _ in got] == [t for t, _ in want], ([t for t, _ in got], [t for t, _ in want])
    for k, ((tag, g), (_, w)) in enumerate(zip(got, want)):
        try:
            CHECKS[tag](g, w)
        except AssertionError as e:
            raise AssertionError(f"output {k} ({tag})") from e


# ---- frames -------------------------------------------------------------------------------------------------------------------
class Frames:
    """The frame generator of one seed.  A frame's rows: pool rows with 0 ... 12 flipped bits (0 most often, so that other frames
    hold the very row), exact duplicates of a row it already has (as a train frame: best == second, d2 == 0 for an equal query
    row), a pool row and its complement (a 2-row frame of them: the second neighbour at 256), random rows."""

    def __init__(self, rng):
        self.rng = rng
        self.pool = R.rnd(rng, POOL)

    def near(self):
        rng = self.rng
        k = 0 if rng.random() < 0.35 else int(rng.integers(1, 13))
        return R.flip(rng, self.pool[int(rng.integers(POOL))], k)

    def make(self, n, uid):
        rng, rows = self.rng, []
        if n == 2 and rng.random() < 0.6:
            x = self.pool[int(rng.integers(POOL))]
            rows = [x, ~x]
        while len(rows) < n:
            u = rng.random()
            if u < 0.5:
                rows.append(self.near())
            elif u < 0.6 and rows:
                rows.append(rows[int(rng.integers(len(rows)))].copy())
            elif u < 0.66 and len(rows) + 2 <= n:
                x = self.pool[int(rng.integers(POOL))]
                rows += [x, ~x]
            else:
                rows.append(R.rnd(rng, 1)[0])
        rows = np.stack(rows)[rng.permutation(n)] if n else np.zeros((0, 32), np.uint8)
        return Frame(rows, uid)


# ---- the op stream ------------------------------------------------------------------------------------------------------------
class Stream:
    """ops(): Steps of (kind, arguments, the stored ids and frames after the step, min_gap, cross_check and the ITEM_SLOTS pin
    after it, whether the drawn op fell back to append).  Arguments name slots and carry host frames."""

    def __init__(self, seed, n_steps, refs=None):
        self.seed, self.n_steps = seed, n_steps
        self.rng = np.random.default_rng(seed)
        self.refs = Refs() if refs is None else refs
        self.gen = Frames(self.rng)
        self.ids, self.frames = [], []
        self.gap, self.cross, self.slots = 2, 0, 0
        self.cross_left = 0
        self.next_id = self.uid = 0
        self.ext = None                                          # the external query set as the device buffer holds it
        self.recent = []                                         # result-bearing calls that still describe the database

    # -- helpers --
    def new_uid(self):
        self.uid += 1
        return (self.seed, self.uid)

    def frame(self, choices=ROW_CHOICES):
        return self.gen.make(int(self.rng.choice(choices)), self.new_uid())

    def store(self, f):
        self.next_id += int(self.rng.integers(1, 4))
        self.ids.append(self.next_id)
        self.frames.append(f)
        self.recent = []
        return self.next_id

    def drop(self, keep):
        del self.ids[keep:], self.frames[keep:]
        self.next_id = max(self.next_id, self.ids[-1] if self.ids else 0)
        self.recent = []

    def n_pairs(self):
        return sum(len(elig(self.ids, q, self.gap)) for q in self.ids)

    def ratio(self):
        return float(self.rng.choice(RATIOS))

    def query_id(self):
        return self.next_id + int(self.rng.integers(-3, 6))

    def rp(self, q_ids=None, q_frames=None):
        """Loop parameters drawn from the model's own counts: min_matches is a pair's good_count that another pair stays below (or
        one above it when another pair reaches that), min_rows a frame's row count (or one above), so both sides of both
        comparisons occur in the very call.  None: rp = NULL."""
        rng = self.rng
        if rng.random() < 0.12:
            return None
        ratio = self.ratio()
        recs, _, _ = want_records(self.refs, self.ids, self.frames, self.gap, ratio, q_ids, q_frames)
        goods = [int(g) for g in recs["good_count"]]
        m = 0
        above = sorted(set(goods))[1:]                                           # the counts that have a smaller one beside them
        if above and rng.random() < 0.75:
            m = above[int(rng.integers(len(above)))]
            if rng.random() < 0.3 and max(goods) > m:
                m += 1
        rows = [len(f) for f in self.frames] + [len(f) for f in (q_frames or [])]
        r = 0
        if rows and rng.random() < 0.6:
            r = rows[int(rng.integers(len(rows)))] + int(rng.random() < 0.3)
        return (ratio, r, m)

    def slot_pairs(self):
        """1 ... 12 (query slot, train slot) pairs: self pairs, repeats, and an empty side where there is one."""
        rng, S = self.rng, len(self.frames)
        n = int(rng.integers(1, 13))
        out = [(int(rng.integers(S)), int(rng.integers(S))) for _ in range(n)]
        if n > 1 and rng.random() < 0.4:
            out[int(rng.integers(n))] = out[0]
        if rng.random() < 0.4:
            k = int(rng.integers(S))
            out[int(rng.integers(n))] = (k, k)
        empty = [k for k, f in enumerate(self.frames) if len(f) == 0]
        if empty and rng.random() < 0.5:
            k, other = int(rng.choice(empty)), int(rng.integers(S))
            out[int(rng.integers(n))] = (k, other) if rng.random() < 0.5 else (other, k)
        return out

    def rewrite_ext(self, mode):
        """The external set after one in-place rewrite of the device buffer."""
        rng = self.rng
        if mode == "new" or self.ext is None:
            n = int(rng.integers(1, EXT_MAX + 1))
            ids = sorted(int(x) for x in rng.integers(0, self.next_id + 6, n))
            bases = [self.gen.make(MAX_ROWS, None).rows for _ in range(n)]
            counts = [int(rng.choice(ROW_CHOICES)) for _ in range(n)]
            mode = "new"
        else:
            ids, bases = list(self.ext.ids), self.ext.bases
            counts = [len(f) for f in self.ext.frames]
            if mode == "ids":                                                    # the rows and counts stay: other eligible prefixes
                k = int(rng.integers(len(ids)))
                ids[k] = int(rng.choice([x for x in range(self.next_id + 6) if x != ids[k]]))
                ids = sorted(ids)
            if mode == "counts":
                k = int(rng.integers(len(counts)))
                counts[k] = int(rng.choice([c for c in ROW_CHOICES if c != counts[k]]))
                for j in range(len(counts)):
                    if j != k and rng.random() < 0.3:
                        counts[j] = int(rng.choice(ROW_CHOICES))
        if mode in ("keep", "ids"):
            frames = self.ext.frames
        else:
            frames = tuple(Frame(b[:c], self.new_uid()) for b, c in zip(bases, counts))
        self.ext = ExtSet(tuple(ids), tuple(frames), tuple(bases), mode)
        return self.ext

    def ext_sets(self):
        """The sets an external-set step runs, in order: 'counts' runs the set as it stands, then again with only its counts
        rewritten - the same ids, the same database, two plans; 'ids' likewise with only one id changed."""
        mode = str(self.rng.choice(("new", "counts", "ids", "keep")))
        if self.ext is None:
            mode = "new"
        if mode in ("counts", "ids"):
            return [self.ext._replace(rewrite="keep"), self.rewrite_ext(mode)]
        return [self.rewrite_ext(mode)]

    # -- the draw --
    def possible(self, kind):
        S = len(self.frames)
        if kind in ("truncate", "classic_pair"):
            return S >= 2
        if kind in ("clear", "snapshot", "bulk_ext", "loops_ext", "detect_stored", "stored_ratio", "stored_batch_ratio", "query_batch_ratio"):
            return S >= 1
        if kind in ("bulk_self", "loops_self", "classic", "classic_loops", "loops_cap"):
            return self.n_pairs() >= 1
        if kind == "rewind":
            return S >= 4 and self.n_pairs() >= 1
        if kind == "replay":
            return len(self.recent) >= 1
        return True

    def draw(self):
        kinds = [k for k in KINDS if not (self.cross and k in NOT_UNDER_CROSS)]
        w = np.array([WEIGHTS.get(k, 1.0) * (3.0 if self.cross and k in ENTRY else 1.0) for k in kinds])
        return kinds[int(self.rng.choice(len(kinds), p=w / w.sum()))]

    def build(self, kind):
        rng = self.rng
        S = len(self.frames)
        if kind in ("append", "append_dev"):
            if S >= MAX_FRAMES:                                                  # an append above the limit becomes a truncate
                kind = "truncate"
            else:
                f = self.frame()
                return kind, dict(frame=f, id=self.store(f))
        if kind == "truncate":
            keep = int(rng.integers(1, S))
            self.drop(keep)
            return kind, dict(keep=keep)
        if kind == "clear":
            self.drop(0)
            return kind, {}
        if kind == "snapshot":
            return kind, dict(clear=bool(rng.random() < 0.5))
        if kind == "params":
            self.gap = int(rng.integers(0, 5))
            self.cross = int(rng.choice([0, 0, 0, 1, 2]))
            self.cross_left = int(rng.integers(4, 9)) if self.cross else 0
            self.recent = []
            return kind, dict(gap=self.gap, cross=self.cross)
        if kind == "variant":
            return kind, dict(variant=int(rng.choice([0, 0, 1, 4, 5])))
        if kind == "tuning":
            self.slots = int(rng.choice([0, 1, 2, 5]))
            return kind, dict(item_slots=self.slots, packed=int(rng.choice([-1, 0, 1, 2])), scratch_mb=int(rng.choice([1, 2, 1024])),
                              upload_kernel=int(rng.choice([0, 1])), host_fold=int(rng.choice([0, 1])), online_streams=int(rng.choice([0, 1])))
        if kind == "bulk_self":
            return kind, dict(ratio=self.ratio())
        if kind == "bulk_ext":
            return kind, dict(sets=self.ext_sets(), ratio=self.ratio())
        if kind == "loops_self":
            return kind, dict(rp=self.rp())
        if kind == "loops_ext":
            sets = self.ext_sets()
            return kind, dict(sets=sets, rp=self.rp(sets[-1].ids, sets[-1].frames))
        if kind == "loops_cap":
            return kind, dict(rp=(self.ratio(), 0, 0))                           # every pair is a candidate: at least one
        if kind == "rewind":
            k = int(rng.integers(1, 4))
            before = (tuple(self.ids), tuple(self.frames))
            self.drop(S - k)
            new = []
            for _ in range(k):
                f = self.frame()
                new.append((self.store(f), f))
            return kind, dict(before=before, keep=S - k, new=new, ratio=self.ratio(), rp=self.rp())
        if kind in ("classic", "classic_loops"):
            return kind, {}
        if kind == "query_host":
            return kind, dict(query=self.frame(), qid=self.query_id(), ratio=self.ratio())
        if kind == "detect_host":
            q, qid = self.frame(), self.query_id()
            return kind, dict(query=q, qid=qid, rp=self.rp([qid], [q]))
        if kind == "detect_stored":
            slot = int(rng.integers(S))
            return kind, dict(slot=slot, rp=self.rp([self.ids[slot]], [self.frames[slot]]))
        if kind == "tickets":
            subs = []
            for _ in range(int(rng.integers(1, 4))):
                k = 1 if rng.random() < 0.5 else int(rng.integers(1, 5))
                qs = [self.frame() for _ in range(k)]
                qids = [self.next_id + 1 + j for j in range(k)]
                form = "one" if k == 1 and rng.random() < 0.7 else "batch"
                n_stored = len(self.frames)
                add = None
                if rng.random() < 0.6 and len(self.frames) < MAX_FRAMES:
                    f = self.frame()
                    add = (self.store(f), f)
                subs.append(dict(form=form, qs=qs, qids=qids, n_stored=n_stored, add=add))
            calls = []
            for _ in range(int(rng.integers(1, 4))):
                sub = str(rng.choice(("query_host", "detect_host") + (("detect_stored",) if self.frames else ())))
                calls.append(self.build(sub))
            return kind, dict(subs=subs, calls=calls)
        if kind == "stored_ratio":
            return kind, dict(pair=self.slot_pairs()[0], ratio=self.ratio())
        if kind == "stored_batch_ratio":
            return kind, dict(pairs=self.slot_pairs(), ratio=self.ratio())
        if kind == "query_batch_ratio":
            return kind, dict(query=self.frame(), trains=[t for _, t in self.slot_pairs()], ratio=self.ratio())
        if kind in ("knn2_pair", "features_ratio"):
            q = self.frame()
            t = q if rng.random() < 0.15 else self.frame()
            return kind, dict(query=q, train=t, ratio=self.ratio())
        if kind == "classic_pair":
            a, b = (int(x) for x in rng.integers(0, S, 2))
            return kind, dict(pair=(a, b), query=self.frame(), train=self.frame())
        if kind == "replay":
            return kind, dict(calls=list(self.recent[-3:]))
        raise AssertionError(kind)

    def ops(self):
        for _ in range(self.n_steps):
            fallback = False
            if self.cross and self.cross_left == 0:                              # cross_check has been on for a while: back to 0
                self.gap, self.cross = int(self.rng.integers(0, 5)), 0
                kind, args = "params", dict(gap=self.gap, cross=0)
            else:
                kind = self.draw()
                if not self.possible(kind):
                    kind, fallback = "append", True
                self.cross_left -= bool(self.cross and kind != "params")
                cross_before = self.cross
                kind, args = self.build(kind)
                if kind in REPLAYED and not cross_before:
                    self.recent.append((kind, args))
            yield Step(kind, args, tuple(self.ids), tuple(self.frames), self.gap, self.cross, self.slots, fallback)


def ops(seed, n_steps, refs=None):
    return Stream(seed, n_steps, refs).ops()


# ---- what a step must return ----------------------------------------------------------------------------------------------------
def expected_call(kind, a, ids, frames, gap, slots, refs):
    """The outputs of one ratio call on the database (ids, frames) as [(tag, value)]; the runner returns the same list."""
    if kind == "bulk_self":
        recs, offs, _ = want_records(refs, ids, frames, gap, a["ratio"])
        return [("offsets", offs), ("n", len(recs)), ("records", recs), ("launch", launch_bulk(ids, frames, gap, slots))]
    if kind in ("loops_self", "loops_cap"):
        ratio = R.DEFAULTS[0] if a["rp"] is None else a["rp"][0]
        recs, _, pairs = want_records(refs, ids, frames, gap, ratio)
        cands = want_cands(recs, pairs, ids, frames, a["rp"])
        launch = ("launch", launch_bulk(ids, frames, gap, slots))                # the fused call's record is its ratio search's
        if kind == "loops_cap":
            return [("n", len(recs)), ("n", len(cands)), ("bulk", recs), launch]
        return [("n", len(recs)), ("cands", cands), ("bulk", recs), launch]
    if kind in ("bulk_ext", "loops_ext"):
        out = []
        for e in a["sets"]:
            if kind == "bulk_ext":
                recs, offs, _ = want_records(refs, ids, frames, gap, a["ratio"], e.ids, e.frames)
                out += [("offsets", offs), ("n", len(recs)), ("records", recs), ("launch", launch_bulk(ids, frames, gap, slots, e.ids, e.frames))]
            else:
                ratio = R.DEFAULTS[0] if a["rp"] is None else a["rp"][0]
                recs, _, pairs = want_records(refs, ids, frames, gap, ratio, e.ids, e.frames)
                out += [("n", len(recs)), ("cands", want_cands(recs, pairs, ids, frames, a["rp"], e.ids, e.frames)), ("bulk", recs),
                        ("launch", launch_bulk(ids, frames, gap, slots, e.ids, e.frames))]
        return out
    if kind == "query_host":
        q, qid = a["query"], a["qid"]
        recs, _, pairs = want_records(refs, ids, frames, gap, a["ratio"], [qid], [q])
        return [("records", recs), ("ids", [ids[s] for _, s in pairs]), ("launch", launch_online(ids, frames, gap, qid, len(q)))]
    if kind in ("detect_host", "detect_stored"):
        q, qid = (a["query"], a["qid"]) if kind == "detect_host" else (frames[a["slot"]], ids[a["slot"]])
        ratio = R.DEFAULTS[0] if a["rp"] is None else a["rp"][0]
        recs, _, pairs = want_records(refs, ids, frames, gap, ratio, [qid], [q])
        return [("cands", want_cands(recs, pairs, ids, frames, a["rp"], [qid], [q])), ("records", recs),
                ("launch", launch_online(ids, frames, gap, qid, len(q)))]
    if kind == "stored_ratio":
        q, t = a["pair"]
        return [("list", want_lists(refs, [(frames[q], frames[t])], a["ratio"]))]
    if kind == "stored_batch_ratio":
        return [("list", want_lists(refs, [(frames[q], frames[t]) for q, t in a["pairs"]], a["ratio"]))]
    if kind == "query_batch_ratio":
        return [("list", want_lists(refs, [(a["query"], frames[t]) for t in a["trains"]], a["ratio"]))]
    if kind == "knn2_pair":
        return [("knn2", refs.pair(a["query"], a["train"]))]
    if kind == "features_ratio":
        return [("list", want_lists(refs, [(a["query"], a["train"])], a["ratio"]))]
    raise AssertionError(kind)


def expected(step, refs, cross=None):
    """A whole step's outputs.  Under cross_check != 0 a ratio kind's only output is its refusal."""
    kind, a = step.kind, step.args
    cross = step.cross if cross is None else cross
    db = (step.ids, step.frames, step.gap, step.slots, refs)
    if kind in ENTRY:
        if cross:
            return [("refused", list(ENTRY_POINTS).index(ENTRY[kind]))]
        return expected_call(kind, a, *db)
    if kind == "rewind":
        ids0, frames0 = a["before"]
        return (expected_call("bulk_self", a, ids0, frames0, step.gap, step.slots, refs) + expected_call("bulk_self", a, *db) +
                expected_call("loops_self", a, *db))
    if kind in ("tickets", "replay"):
        return [o for k, args in a["calls"] for o in expected_call(k, args, *db)]
    return []


# ---- what a run reached ---------------------------------------------------------------------------------------------------------
class Coverage:
    """Counts what a run reached: from the steps, the outputs the runner hands in (see the module text) and - through Refs.watch -
    the pairs whose references those outputs were compared with."""

    def __init__(self):
        self.kinds, self.fallbacks, self.steps = {}, 0, 0
        self.rewinds = self.ext_counts = self.ext_ids = self.with_tickets = 0
        self.fused_order = set()                                  # ('ratio', 'classic'), ('classic', 'ratio'): fused calls back to back
        self.last_fused = None
        self.found = self.not_found = 0
        self.below, self.at_least = set(), set()                  # drawn min_matches with a count below it / at or above it
        self.drawn = set()
        self.seen = set()                                         # no_second, d2_zero, d2_256
        self.refused = set()

    def fused(self, which):
        if self.last_fused is not None and self.last_fused != which:
            self.fused_order.add((self.last_fused, which))
        self.last_fused = which

    def judged(self, rp, recs, cands):
        """One loop decision over these records."""
        if len(cands):
            self.found += 1
        else:
            self.not_found += 1
        m = R.DEFAULTS[2] if rp is None else rp[2]
        if rp is not None and m > 0 and len(recs):
            self.drawn.add(m)
            if (recs["good_count"] < m).any():
                self.below.add(m)
            if (recs["good_count"] >= m).any():
                self.at_least.add(m)

    def call(self, kind, a, outs):
        """outs: one call's (tag, value) list, as expected_call orders it."""
        if kind in ("loops_self", "loops_ext"):
            for k in range(0, len(outs), 4):
                self.fused("ratio")
                self.judged(a["rp"], outs[k + 2][1], outs[k + 1][1])
        elif kind == "loops_cap":
            self.fused("ratio")
        elif kind in ("detect_host", "detect_stored"):
            self.judged(a["rp"], outs[1][1], outs[0][1])

    def step(self, s, outs):
        self.steps += 1
        self.kinds[s.kind] = self.kinds.get(s.kind, 0) + 1
        self.fallbacks += bool(s.fallback)
        kind, a = s.kind, s.args
        if outs and outs[0][0] == "refused":
            self.refused.add(ENTRY[kind])
            return
        if kind == "classic_loops":
            self.fused("classic")
        elif kind == "rewind":
            self.rewinds += 1                                     # truncate, append back to the frame count of the search before
            self.call("loops_self", a, outs[8:])
        elif kind in ("tickets", "replay"):
            self.with_tickets += kind == "tickets"
            at = 0
            for k, args in a["calls"]:
                if kind == "tickets":                             # (a replay repeats calls that were counted when they ran)
                    self.call(k, args, outs[at:at + TAGS[k]])
                at += TAGS[k]
        elif kind in ENTRY:
            if kind in ("bulk_ext", "loops_ext") and len(a["sets"]) == 2:
                self.ext_counts += a["sets"][1].rewrite == "counts"
                self.ext_ids += a["sets"][1].rewrite == "ids"
            self.call(kind, a, outs)

    def summary(self):
        return dict(fallbacks=self.fallbacks, rewinds=self.rewinds, ext_counts=self.ext_counts, ext_ids=self.ext_ids, with_tickets=self.with_tickets,
                    fused_order=sorted(self.fused_order), found=self.found, not_found=self.not_found, drawn=len(self.drawn),
                    seen=sorted(self.seen), refused=sorted(self.refused))

    def check(self):
        """The per-seed conditions the sequences are there for."""
        missing = [k for k in KINDS if not self.kinds.get(k)]
        assert not missing, missing
        assert self.fallbacks * 10 <= self.steps, (self.fallbacks, self.steps)
        assert self.rewinds >= 2 and self.ext_counts >= 1 and self.ext_ids >= 1 and self.with_tickets >= 1, self.summary()
        assert self.fused_order == {("ratio", "classic"), ("classic", "ratio")}, self.summary()
        assert self.found >= 1 and self.not_found >= 1, self.summary()
        assert self.drawn and self.drawn == self.below == self.at_least, (sorted(self.drawn), sorted(self.below), sorted(self.at_least))
        assert self.seen == {"no_second", "d2_zero", "d2_256"}, self.summary()
        assert self.refused, self.summary()


# outputs of one call of a kind (the external-set kinds: per set)
TAGS = {"bulk_self": 4, "loops_self": 4, "loops_cap": 4, "query_host": 3, "detect_host": 3, "detect_stored": 3, "stored_ratio": 1,
        "stored_batch_ratio": 1, "query_batch_ratio": 1, "knn2_pair": 1, "features_ratio": 1}


def describe(step):
    """A step's arguments without its arrays, for a failure message."""
    def short(v):
        if isinstance(v, (Frame, np.ndarray)):
            return f"<{len(v)} rows>"
        if isinstance(v, ExtSet):
            return f"<ext {v.rewrite} ids {list(v.ids)} rows {[len(f) for f in v.frames]}>"
        if isinstance(v, (list, tuple)):
            return [short(x) for x in v]
        if isinstance(v, dict):
            return {k: short(x) for k, x in v.items()}
        return v

    return dict(args={k: (short(v) if k != "calls" else [c[0] for c in v]) for k, v in step.args.items() if k != "before"},
                ids=list(step.ids), rows=[len(f) for f in step.frames], gap=step.gap, cross=step.cross, slots=step.slots)


def dry_run(seed, n_steps, refs=None):
    """The stream without a device: the Coverage it must reach, from the model's own outputs."""
    refs = Refs() if refs is None else refs
    cov = Coverage()
    refs.watch = cov
    try:
        for s in ops(seed, n_steps, refs):
            cov.step(s, expected(s, refs))
    finally:
        refs.watch = None
    return cov


# ---- the group's stream ---------------------------------------------------------------------------------------------------------
GROUP_KINDS = ("append", "truncate", "clear", "params", "g_ratio", "g_loops", "g_loops_cap", "g_classic", "g_classic_loops", "g_refusals",
               "g_trim")
GROUP_WEIGHTS = {"append": 4.0, "clear": 0.4, "g_ratio": 2.0, "g_loops": 2.0, "g_refusals": 0.5}
GStep = namedtuple("GStep", "kind args ids frames gap changed fallback")


def group_ops(seed, n_steps, world, refs=None):
    """The loopback group's stream: GSteps of (kind, arguments, ids and frames after the step, min_gap, whether frames changed since
    the last search that exchanged the shard arenas - judged BEFORE this step's own search - and the fallback flag).  g_trim drops
    the last frame where that leaves every shard's slot count as it was (so that nothing but the database's own stamp asks for a
    new exchange) and searches at once."""
    st = Stream(seed, n_steps, refs)
    rng = st.rng
    changed = True
    for _ in range(n_steps):
        w = np.array([GROUP_WEIGHTS.get(k, 1.0) for k in GROUP_KINDS])
        kind = GROUP_KINDS[int(rng.choice(len(GROUP_KINDS), p=w / w.sum()))]
        fallback = False
        S = len(st.frames)
        searches = kind.startswith("g_") and kind != "g_refusals"
        ok = S >= 2 if kind == "truncate" else S >= 1 if kind == "clear" else st.n_pairs() >= 1 if searches else True
        if kind == "g_trim":
            ok = S >= 3 and (S - 1) % world != 0 and sum(len(elig(st.ids[:-1], q, st.gap)) for q in st.ids[:-1]) >= 1
        if not ok:
            kind, fallback = "append", True
        was = changed
        if kind in ("append", "truncate", "clear"):
            kind, args = st.build(kind)
            changed = True
        elif kind == "params":
            st.gap = int(rng.integers(0, 5))
            args = dict(gap=st.gap)
        elif kind == "g_trim":
            st.drop(S - 1)
            args, was = dict(keep=S - 1, ratio=st.ratio()), True
        elif kind == "g_ratio":
            args = dict(ratio=st.ratio())
        elif kind == "g_loops":
            args = dict(rp=st.rp())
        elif kind == "g_loops_cap":
            args = dict(rp=(st.ratio(), 0, 0))
        elif kind == "g_refusals":
            args = dict(cross=int(rng.choice([1, 2])), ratio=st.ratio())
        else:
            args = {}
        if searches and not fallback:
            changed = False                                       # every search with a pair exchanges what changed
        yield GStep(kind, args, tuple(st.ids), tuple(st.frames), st.gap, was, fallback)


def group_expected(s, refs):
    kind, a = s.kind, s.args
    if kind in ("g_ratio", "g_trim"):
        recs, offs, _ = want_records(refs, s.ids, s.frames, s.gap, a["ratio"])
        return [("records", recs), ("offsets", offs)]
    if kind in ("g_loops", "g_loops_cap"):
        ratio = R.DEFAULTS[0] if a["rp"] is None else a["rp"][0]
        recs, _, pairs = want_records(refs, s.ids, s.frames, s.gap, ratio)
        cands = want_cands(recs, pairs, s.ids, s.frames, a["rp"])
        return [("n", len(recs)), ("cands", cands)] if kind == "g_loops" else [("n", len(recs)), ("n", len(cands))]
    return []


def group_dry_run(seed, n_steps, world, refs=None):
    """(kinds, fallbacks, searches that exchanged arenas, searches that skipped the exchange, loop searches with / without a
    candidate) of a group stream."""
    refs = Refs() if refs is None else refs
    kinds, fallbacks, gathered, skipped, found, none = {}, 0, 0, 0, 0, 0
    for s in group_ops(seed, n_steps, world, refs):
        kinds[s.kind] = kinds.get(s.kind, 0) + 1
        fallbacks += s.fallback
        if s.kind.startswith("g_") and s.kind != "g_refusals":
            gathered += s.changed
            skipped += not s.changed
        if s.kind == "g_loops":
            n = len(group_expected(s, refs)[1][1])
            found += n > 0
            none += n == 0
    return dict(kinds=kinds, fallbacks=fallbacks, gathered=gathered, skipped=skipped, found=found, none=none)


def group_check(fig, n_steps):
    missing = [k for k in GROUP_KINDS if not fig["kinds"].get(k)]
    assert not missing, missing
    assert fig["fallbacks"] * 10 <= n_steps and fig["gathered"] >= 5 and fig["skipped"] >= 5 and fig["found"] >= 1 and fig["none"] >= 1, fig
