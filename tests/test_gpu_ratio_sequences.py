"""The two-neighbour and ratio-scored routes of the 32-byte ORB database under random call sequences (lcm_all_vs_all_ratio,
lcm_all_vs_all_loops_ratio, lcm_query_scores_ratio, lcm_detect_loops_ratio, the k = 2 pair calls, the two group forms: lcm_ratio.cpp,
lcm_knn.cpp, lcm_group_search.cpp) against tests/ratiomodel.py.  Needs a real MI355X.

One long-lived handle per seed replays ratiomodel.ops(seed): appends from the host and from the device, truncates, clears, snapshot
round trips, parameter / kernel-variant / tuning changes, the ratio searches on the stored frames and on an external query set whose
device buffer is rewritten in place, the fused ratio search between the classic fused one, online ratio calls beside tickets in
flight, the k = 2 pair calls between the k = 1 ones.  After every step every returned field is compared with the model (knnref,
ratioref, ratioloopref's rule), lcm_last_bulk_scores with the records of the fused call that left them, the launch record with the
model's arithmetic; the classic calls in between are compared with the C oracle as tests/test_gpu_state_machine.py does.  Under
cross_check != 0 every ratio call must refuse with its pre-filled buffers untouched.  `replay` repeats the last calls here and on a
fresh handle holding the same frames: every output byte must be equal.  It hunts state that outlives its validity - the cached
ratio plan first of all, which nothing but its signature comparison protects.

The file imports no torch and drives the C ABI through capi.py (raw ctypes where a refusal needs the caller's own buffer)."""
import ctypes as C

import numpy as np
import pytest

import ratiomodel as M

pytestmark = pytest.mark.gpu

FILL = 0xA7


def filled(dtype, n, *tail):
    """A caller's buffer of n records (n, *tail) with every byte FILL."""
    dt = np.dtype(dtype)
    width = int(np.prod(tail, dtype=np.int64)) * dt.itemsize
    return np.full((max(n, 1), width), FILL, np.uint8).view(dt).reshape(max(n, 1), *tail)


def untouched(*arrays):
    return all((np.ascontiguousarray(a).view(np.uint8) == FILL).all() for a in arrays)


def vp(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)


def as_bytes(tag, v):
    if tag == "list":
        return v[0].tobytes() + np.asarray(v[1]).astype(np.int64).tobytes()
    if tag == "knn2":
        return v[0].tobytes() + v[1].tobytes()
    return np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else np.asarray(v).astype(np.int64).tobytes()


def arrays(frames, extra=()):
    fr = list(frames) + list(extra)
    rows = np.zeros((max(len(fr), 1), M.MAX_ROWS, 32), np.uint8)
    counts = np.zeros(max(len(fr), 1), np.int32)
    for i, f in enumerate(fr):
        rows[i, : len(f)] = f.rows
        counts[i] = len(f)
    return rows, counts


def loop_params(pkg, rp):
    return None if rp is None else pkg.capi.RatioLoopParams(*rp)


def launch(m):
    i = m.launch_info()
    return int(i.pairs), int(i.distances), int(i.workgroups), int(i.route)


class Runner:
    """One handle and the stream it replays."""

    def __init__(self, pkg, oracle, tmp_path, seed, refs=None):
        self.pkg, self.oracle, self.path = pkg, oracle, str(tmp_path / f"ratio_db_{seed}.bin")
        self.refs = M.Refs() if refs is None else refs
        self.cov = M.Coverage()
        self.refs.watch = self.cov                            # as in the dry run: the coverage sees every pair a reference is asked for
        self.m = m = pkg.Matcher()
        m.set_params(min_gap=2, min_matches=1, sim_threshold=0.0)
        self.d_frame = m.dev_alloc(M.MAX_ROWS * 32)
        self.d_ext_rows = m.dev_alloc(M.EXT_MAX * M.MAX_ROWS * 32)
        self.d_ext_counts = m.dev_alloc(M.EXT_MAX * 4)

    def close(self):
        for d in (self.d_frame, self.d_ext_rows, self.d_ext_counts):
            self.m.dev_free(d)
        self.m.close()

    def params(self, s, cross=None):
        return self.oracle.default_params(min_gap=s.gap, min_matches=1, sim_threshold=0.0, cross_check=s.cross if cross is None else cross)

    # -- one step of the stream, every check included --
    def step(self, s):
        outs = self.run(s)
        M.check_outputs(outs, M.expected(s, self.refs))
        self.cov.step(s, outs)
        assert len(self.m) == len(s.frames)

    def run(self, s):
        m, kind, a, cap = self.m, s.kind, s.args, self.pkg.capi
        if kind in ("append", "append_dev"):
            f = a["frame"]
            if kind == "append_dev" and len(f):
                m.dev_upload(self.d_frame, f.rows)
                m.append_device(a["id"], self.d_frame, len(f))
                m.sync()                                      # d_frame is reused by the next device append
            else:
                m.append(a["id"], f.rows)
        elif kind == "truncate":
            m.truncate(a["keep"])
        elif kind == "clear":
            m.clear()
        elif kind == "snapshot":
            m.save(self.path)
            if a["clear"]:
                m.clear()
            m.load(self.path)
        elif kind == "params":
            m.set_params(min_gap=a["gap"], cross_check=a["cross"])
        elif kind == "variant":
            m.set_kernel_variant(a["variant"])
        elif kind == "tuning":
            for knob, key in ((cap.TUNE_ITEM_SLOTS, "item_slots"), (cap.TUNE_PACKED, "packed"), (cap.TUNE_PACKED_SCRATCH_MB, "scratch_mb"),
                              (cap.TUNE_PAIR_UPLOAD_KERNEL, "upload_kernel"), (cap.TUNE_PAIR_HOST_FOLD, "host_fold"),
                              (cap.TUNE_ONLINE_STREAMS, "online_streams")):
                m.set_tuning(knob, a[key])
        elif kind in M.ENTRY:
            if s.cross:
                for e in a.get("sets", ()):                   # the device buffer follows the model whatever the call answers
                    self.upload_ext(m, e)
                self.refuse(m, kind, a, s)
                return [("refused", M.ENTRY_POINTS.index(M.ENTRY[kind]))]
            return self.call(m, kind, a, s.ids, s.frames, s)
        elif kind in ("classic", "classic_loops"):
            self.classic(s)
        elif kind == "classic_pair":
            self.classic_pair(s)
        elif kind == "rewind":
            ids0, frames0 = a["before"]
            outs = self.call(m, "bulk_self", a, ids0, frames0, s)
            m.truncate(a["keep"])
            for fid, f in a["new"]:
                m.append(fid, f.rows)
            return outs + self.call(m, "bulk_self", a, s.ids, s.frames, s) + self.call(m, "loops_self", a, s.ids, s.frames, s)
        elif kind == "tickets":
            return self.tickets(s)
        elif kind == "replay":
            return self.replay(s)
        else:
            raise AssertionError(kind)
        return []

    # -- the ratio calls --
    def upload_ext(self, m, e):
        counts = np.zeros(M.EXT_MAX, np.int32)
        counts[: len(e.frames)] = [len(f) for f in e.frames]
        if e.rewrite == "new":
            rows = np.zeros((M.EXT_MAX, M.MAX_ROWS, 32), np.uint8)
            for k, b in enumerate(e.bases):
                rows[k] = b
            m.dev_upload(self.d_ext_rows, rows)
        if e.rewrite in ("new", "counts"):                    # ('ids' rewrites nothing on the device: the ids are the call's argument)
            m.dev_upload(self.d_ext_counts, counts)

    def ext_kw(self, e):
        return dict(d_query_rows=self.d_ext_rows, d_query_counts=self.d_ext_counts, q_ids=list(e.ids), q_stride_rows=M.MAX_ROWS)

    def bulk(self, m, ratio, **kw):
        n, offs = m.all_vs_all_ratio_plan(ratio, **kw)
        got, info = np.zeros(n, M.SCORE_DTYPE), None
        if n:
            d = m.dev_alloc(n * 8 + 64)
            try:
                m.dev_upload(d, np.full(n * 8 + 64, FILL, np.uint8))
                assert m.all_vs_all_ratio(ratio, d, n, **kw) == n
                info = launch(m)
                m.sync()
                back = np.zeros(n * 8 + 64, np.uint8)
                m.dev_download(d, back)
                assert untouched(back[n * 8:])
                got = back[: n * 8].view(M.SCORE_DTYPE).copy()
            finally:
                m.dev_free(d)
        return [("offsets", offs), ("n", n), ("records", got), ("launch", info)]

    def fused_raw(self, m, rp, buf, room, e=None):
        """lcm_all_vs_all_loops_ratio with the caller's buffer and a room of its own choice: (rc, n_out, n_pairs)."""
        n, npairs = C.c_size_t(0), C.c_size_t(0)
        p = loop_params(self.pkg, rp)
        ids = None if e is None else np.ascontiguousarray(e.ids, np.int32)
        rc = m._lib.lcm_all_vs_all_loops_ratio(m._h, C.c_void_p(self.d_ext_rows) if e else None, C.c_void_p(self.d_ext_counts) if e else None,
                                               None if e is None else ids.ctypes.data_as(C.c_void_p), 0 if e is None else len(ids),
                                               M.MAX_ROWS if e else 0, None if p is None else C.byref(p), buf.ctypes.data_as(C.c_void_p), room,
                                               C.byref(n), C.byref(npairs))
        return rc, n.value, npairs.value

    def fused(self, m, rp, count, e=None):
        """The fused ratio search with room for exactly `count` candidates (the model's count: one more is a refusal)."""
        buf = filled(M.CANDIDATE_DTYPE, count + 2)
        rc, n, npairs = self.fused_raw(m, rp, buf, count, e)
        assert rc == 0 and n == count, (rc, n, count, m._lib.lcm_last_error())
        assert untouched(buf[count:])
        info = launch(m) if npairs else None
        return [("n", npairs), ("cands", buf[:count].copy()), ("bulk", m.last_bulk_scores()), ("launch", info)]

    def call(self, m, kind, a, ids, frames, s):
        """One ratio call on handle m, its outputs in ratiomodel.expected_call's order."""
        want = M.expected_call(kind, a, ids, frames, s.gap, s.slots, self.refs)      # (only for the room of the fused calls)
        if kind == "bulk_self":
            return self.bulk(m, a["ratio"])
        if kind == "bulk_ext":
            outs = []
            for e in a["sets"]:
                self.upload_ext(m, e)
                outs += self.bulk(m, a["ratio"], **self.ext_kw(e))
            return outs
        if kind == "loops_self":
            return self.fused(m, a["rp"], len(want[1][1]))
        if kind == "loops_ext":
            outs = []
            for k, e in enumerate(a["sets"]):
                self.upload_ext(m, e)
                outs += self.fused(m, a["rp"], len(want[4 * k + 1][1]), e)
            return outs
        if kind == "loops_cap":
            count = int(want[1][1])
            buf = filled(M.CANDIDATE_DTYPE, count)
            rc, n, npairs = self.fused_raw(m, a["rp"], buf, count - 1)
            assert rc == self.pkg.capi.ERR_CAPACITY and untouched(buf), (rc, n, count)
            return [("n", npairs), ("n", n), ("bulk", m.last_bulk_scores()), ("launch", launch(m))]
        if kind == "query_host":
            sc, got_ids = m.query_scores_ratio(a["query"].rows, a["qid"], a["ratio"])
            return [("records", sc), ("ids", got_ids), ("launch", launch(m) if len(sc) else None)]
        if kind in ("detect_host", "detect_stored"):
            q, qid = (a["query"], a["qid"]) if kind == "detect_host" else (frames[a["slot"]], ids[a["slot"]])
            rp = a["rp"] or (None, None, None)
            cands = m.detect_loops_ratio(qid, q.rows if kind == "detect_host" else None, *rp)
            info = launch(m)
            sc, _ = m.query_scores_ratio(q.rows, qid, M.R.DEFAULTS[0] if a["rp"] is None else a["rp"][0])    # the records it judged
            return [("cands", cands), ("records", sc), ("launch", info if len(sc) else None)]
        if kind == "stored_ratio":
            q, t = a["pair"]
            out = m.match_stored_ratio(ids[q], ids[t], a["ratio"])
            return [("list", (out, [0, len(out)]))]
        if kind == "stored_batch_ratio":
            lists, offs = m.match_stored_batch_ratio([(ids[q], ids[t]) for q, t in a["pairs"]], a["ratio"])
            return [("list", (np.concatenate(lists), offs))]
        if kind == "query_batch_ratio":
            lists, offs = m.match_query_batch_ratio(a["query"].rows, [ids[t] for t in a["trains"]], a["ratio"])
            return [("list", (np.concatenate(lists), offs))]
        if kind == "knn2_pair":
            return [("knn2", m.knn2_pair(a["query"].rows, a["train"].rows))]
        if kind == "features_ratio":
            out = m.match_features_ratio(a["query"].rows, a["train"].rows, a["ratio"])
            return [("list", (out, [0, len(out)]))]
        raise AssertionError(kind)

    def refuse(self, m, kind, a, s):
        """The call under cross_check != 0: LCM_ERR_INVALID_ARG and not a byte of the caller's buffers written."""
        lib, h, bad = m._lib, m._h, self.pkg.capi.ERR_INVALID_ARG
        ids, frames = s.ids, s.frames
        n32, nsz, npairs = C.c_int32(0), C.c_size_t(0), C.c_size_t(0)
        entry = M.ENTRY[kind]
        e = a["sets"][-1] if "sets" in a else None
        ext = (None, None, None, 0, 0)
        if e is not None:
            eids = np.ascontiguousarray(e.ids, np.int32)
            ext = (C.c_void_p(self.d_ext_rows), C.c_void_p(self.d_ext_counts), eids.ctypes.data_as(C.c_void_p), len(eids), M.MAX_ROWS)
        rp = loop_params(self.pkg, a.get("rp"))
        rp = None if rp is None else C.byref(rp)
        q = a["query"].rows if "query" in a else None
        out, offs = filled(M.DMATCH_DTYPE, 2048), filled(np.uintp, 16)
        cands, scores, sids = filled(M.CANDIDATE_DTYPE, 64), filled(M.SCORE_DTYPE, 64), filled(np.int32, 64)
        if entry == "lcm_all_vs_all_ratio":
            d = m.dev_alloc(1024)
            try:
                m.dev_upload(d, np.full(1024, FILL, np.uint8))
                rc = lib.lcm_all_vs_all_ratio(h, *ext, a["ratio"], C.c_void_p(d), 128, C.byref(nsz), None)
                back = np.zeros(1024, np.uint8)
                m.sync()
                m.dev_download(d, back)
                assert untouched(back)
            finally:
                m.dev_free(d)
        elif entry == "lcm_all_vs_all_loops_ratio":
            rc = lib.lcm_all_vs_all_loops_ratio(h, *ext, rp, vp(cands), 64, C.byref(nsz), C.byref(npairs))
        elif entry == "lcm_query_scores_ratio":
            rc = lib.lcm_query_scores_ratio(h, vp(q), len(q), a["qid"], a["ratio"], vp(scores), vp(sids), C.byref(n32))
        elif entry == "lcm_detect_loops_ratio":
            if kind == "detect_host":
                rc = lib.lcm_detect_loops_ratio(h, a["qid"], vp(q) if len(q) else vp(np.zeros((1, 32), np.uint8)), len(q), rp, vp(cands), 64, C.byref(n32))
            else:
                rc = lib.lcm_detect_loops_ratio(h, ids[a["slot"]], None, 0, rp, vp(cands), 64, C.byref(n32))
        elif entry == "lcm_match_stored_ratio":
            rc = lib.lcm_match_stored_ratio(h, ids[a["pair"][0]], ids[a["pair"][1]], a["ratio"], vp(out), 2048, C.byref(n32))
        elif entry == "lcm_match_stored_batch_ratio":
            pr = np.ascontiguousarray([(ids[x], ids[y]) for x, y in a["pairs"]], np.int32)
            rc = lib.lcm_match_stored_batch_ratio(h, vp(pr), len(pr), a["ratio"], vp(out), 2048, vp(offs))
        elif entry == "lcm_match_query_batch_ratio":
            tr = np.ascontiguousarray([ids[t] for t in a["trains"]], np.int32)
            rc = lib.lcm_match_query_batch_ratio(h, vp(q), len(q), vp(tr), len(tr), a["ratio"], vp(out), 2048, vp(offs))
        else:
            t = a["train"].rows
            idx, dist = filled(np.int32, len(q), 2), filled(np.uint16, len(q), 2)
            if entry == "lcm_knn2_pair":
                rc = lib.lcm_knn2_pair(h, vp(q), len(q), vp(t), len(t), vp(idx), vp(dist), C.byref(n32))
            else:
                rc = lib.lcm_match_features_ratio(h, vp(q), len(q), vp(t), len(t), a["ratio"], vp(out), C.byref(n32))
            assert untouched(idx, dist)
        assert rc == bad, (entry, rc)
        # a known deviation from "nothing written" (DESIGN 9o): the two batch calls zero offsets[0] before they look at
        # cross_check, as every call zeroes *n_out; no other byte of any buffer may change
        batch = entry in ("lcm_match_stored_batch_ratio", "lcm_match_query_batch_ratio")
        assert untouched(out, offs[1:], cands, scores, sids) and (int(offs[0]) == 0 if batch else untouched(offs[:1])), entry

    # -- the classic calls in between, against the C oracle --
    def classic_want(self, s):
        rows, counts = arrays(s.frames)
        pq, pt, offs = [], [], [0]
        for c, cid in enumerate(s.ids):
            for i in M.elig(s.ids, cid, s.gap):
                pq.append(c); pt.append(i)
            offs.append(len(pq))
        want, wsums = self.oracle.fast_score_pairs_idx(rows, counts, pq, pt, self.params(s), n_threads=2)
        return want, wsums, pq, pt, offs, counts

    def classic(self, s):
        m = self.m
        want, wsums, pq, pt, offs, counts = self.classic_want(s)
        n, goffs = m.all_vs_all_plan()
        assert n == len(pq) and goffs.astype(np.int64).tolist() == offs
        if s.kind == "classic":
            d, ds = m.dev_alloc(n * 8), m.dev_alloc(n * 4)
            try:
                got, sums = np.zeros(n, want.dtype), np.zeros(n, np.uint32)
                m.all_vs_all(d, n); m.sync(); m.dev_download(d, got)
                np.testing.assert_array_equal(got, want)
                m.all_vs_all_argmin(d, n, ds); m.sync(); m.dev_download(d, got); m.dev_download(ds, sums)
                np.testing.assert_array_equal(got, want)
                np.testing.assert_array_equal(sums, wsums)
            finally:
                m.dev_free(d); m.dev_free(ds)
        else:
            cands, npairs = m.all_vs_all_loops(cap=n)
            p = self.params(s)
            keep = [(s.ids[pq[k]], s.ids[pt[k]], int(want[k]["good_count"])) for k in range(n)
                    if self.oracle.loop_test(int(want[k]["good_count"]), int(counts[pq[k]]), int(counts[pt[k]]), p)[0]]
            assert npairs == n
            assert [(int(r["current_frame_id"]), int(r["matched_frame_id"]), int(r["num_matches"])) for r in cands] == keep
            np.testing.assert_array_equal(m.last_bulk_scores(), want)       # the records of THIS fused call, not the ratio one's

    def classic_pair(self, s):
        m, a = self.m, s.args
        x, y = a["pair"]
        got, md = m.match_stored(s.ids[x], s.ids[y])
        om, omd = self.oracle.match_features(s.frames[x].rows, s.frames[y].rows, self.params(s))
        assert md == omd or len(om) == 0
        np.testing.assert_array_equal(got, om.astype(got.dtype))
        q, t = a["query"].rows, a["train"].rows
        if not s.cross and len(q) and len(t):
            idx, dist = m.match_pair(q, t)
            D = M.knnref.distances(q, t).astype(np.int64)
            np.testing.assert_array_equal(idx, D.argmin(axis=1))
            np.testing.assert_array_equal(dist, D.min(axis=1))

    def tickets(self, s):
        """Classic tickets in flight, appends between them, ratio calls beside them; then every ticket is collected and checked."""
        m, a = self.m, s.args
        pending = []
        for sub in a["subs"]:
            if sub["form"] == "one":
                t = m.query_submit(sub["qs"][0].rows, sub["qids"][0])
            else:
                t = m.query_submit_batch([q.rows for q in sub["qs"]], sub["qids"])
            pending.append((t, sub))
            if sub["add"]:
                m.append(sub["add"][0], sub["add"][1].rows)
        outs = [o for k, args in a["calls"] for o in self.call(m, k, args, s.ids, s.frames, s)]

        def want_query(q, qid, n_stored):
            rows, counts = arrays(s.frames, [q])
            el = [i for i in M.elig(s.ids, qid, s.gap) if i < n_stored]
            return self.oracle.fast_score_pairs_idx(rows, counts, [len(s.frames)] * len(el), el, self.params(s), n_threads=2)[0], el

        for t, sub in reversed(pending):
            if sub["form"] == "one":
                sc, got_ids = m.query_collect(t)
                want, el = want_query(sub["qs"][0], sub["qids"][0], sub["n_stored"])
                np.testing.assert_array_equal(sc, want)
                assert got_ids.tolist() == [s.ids[i] for i in el]
            else:
                sc, offs = m.query_collect_batch(t)
                for k, (q, qid) in enumerate(zip(sub["qs"], sub["qids"])):
                    np.testing.assert_array_equal(sc[int(offs[k]): int(offs[k + 1])], want_query(q, qid, sub["n_stored"])[0])
        return outs

    def replay(self, s):
        """The recent calls again here, then on a fresh handle with the same frames: the same bytes, the launch record aside (the
        fresh handle has no ITEM_SLOTS pin)."""
        calls = s.args["calls"]
        mine = [self.call(self.m, k, args, s.ids, s.frames, s) for k, args in calls]
        fresh = self.pkg.Matcher()
        try:
            fresh.set_params(min_gap=s.gap, min_matches=1, sim_threshold=0.0)
            for fid, f in zip(s.ids, s.frames):
                fresh.append(fid, f.rows)
            theirs = [self.call(fresh, k, args, s.ids, s.frames, s) for k, args in calls]
        finally:
            fresh.close()
        for (k, _), x, y in zip(calls, mine, theirs):
            assert [t for t, _ in x] == [t for t, _ in y]
            for j, ((tag, u), (_, v)) in enumerate(zip(x, y)):
                assert tag == "launch" or as_bytes(tag, u) == as_bytes(tag, v), (k, j, tag)
        return [o for x in mine for o in x]

    def finish(self, seed, n_steps, check=True):
        """What the sequence reached, recomputed from what ran: the dry run's conditions and its very figures."""
        if check:
            self.cov.check()
        dry = M.dry_run(seed, n_steps)
        assert self.cov.summary() == dry.summary() and self.cov.kinds == dry.kinds, (self.cov.summary(), dry.summary())


def play(runner, seed, n, s):
    try:
        runner.step(s)
    except Exception as e:
        raise AssertionError(f"seed {seed} step {n} {s.kind} {M.describe(s)}") from e


@pytest.mark.parametrize("seed", M.SEEDS)
def test_random_ratio_sequences_equal_model(pkg, oracle, tmp_path, seed):
    r = Runner(pkg, oracle, tmp_path, seed)
    try:
        for n, s in enumerate(M.ops(seed, M.STEPS, r.refs)):
            play(r, seed, n, s)
        r.finish(seed, M.STEPS)
    finally:
        r.close()


@pytest.mark.parametrize("seeds", M.TWIN_SEEDS, ids=lambda t: f"{t[0]}-{t[1]}")
def test_two_handles_interleaved(pkg, oracle, tmp_path, seeds):
    """Two handles in one process, their streams in alternating steps: nothing process-wide leaks between them."""
    runners = [Runner(pkg, oracle, tmp_path, seed) for seed in seeds]
    try:
        streams = [M.ops(seed, M.TWIN_STEPS, r.refs) for seed, r in zip(seeds, runners)]
        for n in range(M.TWIN_STEPS):
            for seed, r, stream in zip(seeds, runners, streams):
                play(r, seed, n, next(stream))
        for seed, r in zip(seeds, runners):
            r.finish(seed, M.TWIN_STEPS, check=False)
    finally:
        for r in runners:
            r.close()


# ---- the group forms --------------------------------------------------------------------------------------------------------------
def group_params(pkg, gap, cross=0):
    p = pkg.default_params()
    p.min_gap, p.min_matches, p.sim_threshold, p.cross_check = gap, 1, 0.0, cross
    return p


def group_loops_raw(g, pkg, rp, buf, room):
    n, npairs = C.c_size_t(0), C.c_size_t(0)
    p = loop_params(pkg, rp)
    rc = g._lib.lcm_group_all_vs_all_loops_ratio(g._g, None if p is None else C.byref(p), buf.ctypes.data_as(C.c_void_p), room, C.byref(n), C.byref(npairs))
    return rc, n.value, npairs.value


@pytest.mark.parametrize("world,seed", M.GROUP_RUNS)
def test_random_group_ratio_sequences(pkg, oracle, world, seed):
    """A loopback group of W shards under append / truncate / clear / set_params and the two ratio searches, the classic group
    searches in between: every answer against the model itself, and lcm_group_last_info reports the arena exchange as skipped
    exactly when no frame changed since the last search."""
    refs = M.Refs()
    kinds, fallbacks, gathered, skipped, found, none = {}, 0, 0, 0, 0, 0
    with pkg.Group(group_params(pkg, 2), n_devices=world, loopback_device=0) as g:
        for n, s in enumerate(M.group_ops(seed, M.GROUP_STEPS, world, refs)):
            kind, a = s.kind, s.args
            kinds[kind] = kinds.get(kind, 0) + 1
            fallbacks += s.fallback
            want = M.group_expected(s, refs)
            try:
                if kind == "append":
                    g.append(a["id"], a["frame"].rows)
                elif kind == "truncate":
                    g.truncate(a["keep"])
                elif kind == "clear":
                    g.clear()
                elif kind == "params":
                    g.set_params(group_params(pkg, a["gap"]))
                elif kind == "g_refusals":
                    g.set_params(group_params(pkg, s.gap, a["cross"]))
                    buf, recs = filled(M.CANDIDATE_DTYPE, 64), filled(M.SCORE_DTYPE, 2048)
                    nsz = C.c_size_t(0)
                    assert group_loops_raw(g, pkg, (a["ratio"], 0, 0), buf, 64)[0] == pkg.capi.ERR_INVALID_ARG
                    assert g._lib.lcm_group_all_vs_all_ratio(g._g, a["ratio"], recs.ctypes.data_as(C.c_void_p), 2048, C.byref(nsz), None) == pkg.capi.ERR_INVALID_ARG
                    assert untouched(buf, recs)
                    g.set_params(group_params(pkg, s.gap))
                elif kind in ("g_ratio", "g_trim"):
                    if kind == "g_trim":
                        g.truncate(a["keep"])
                    got, offs = g.all_vs_all_ratio(a["ratio"])
                    M.check_outputs([("records", got), ("offsets", offs)], want)
                elif kind == "g_loops":
                    count = len(want[1][1])
                    buf = filled(M.CANDIDATE_DTYPE, count + 2)
                    rc, k, npairs = group_loops_raw(g, pkg, a["rp"], buf, count)
                    assert rc == 0 and k == count and untouched(buf[count:]), (rc, k, count)
                    M.check_outputs([("n", npairs), ("cands", buf[:count].copy())], want)
                    found += count > 0
                    none += count == 0
                elif kind == "g_loops_cap":
                    count = int(want[1][1])
                    buf = filled(M.CANDIDATE_DTYPE, count)
                    rc, k, npairs = group_loops_raw(g, pkg, a["rp"], buf, count - 1)
                    assert rc == pkg.capi.ERR_CAPACITY and untouched(buf), (rc, k, count)
                    M.check_outputs([("n", npairs), ("n", k)], want)
                else:
                    rows, counts = arrays(s.frames)
                    pq, pt, woffs = [], [], [0]
                    for c, cid in enumerate(s.ids):
                        for i in M.elig(s.ids, cid, s.gap):
                            pq.append(c); pt.append(i)
                        woffs.append(len(pq))
                    p = oracle.default_params(min_gap=s.gap, min_matches=1, sim_threshold=0.0)
                    wrecs, wsums = oracle.fast_score_pairs_idx(rows, counts, pq, pt, p, n_threads=2)
                    if kind == "g_classic":
                        merged, offs = g.all_vs_all()
                        assert g.info().arena_gather_skipped == (0 if s.changed else 1)
                        assert np.asarray(offs).astype(np.int64).tolist() == woffs
                        np.testing.assert_array_equal(merged, wrecs)
                        gs, gi, _ = g.all_vs_all_argmin()                  # a second search in this step: nothing to exchange
                        np.testing.assert_array_equal(gs, wrecs)
                        np.testing.assert_array_equal(gi, wsums)
                    else:
                        cands, npairs = g.all_vs_all_loops(cap=len(pq))
                        keep = [(s.ids[pq[k]], s.ids[pt[k]], int(wrecs[k]["good_count"])) for k in range(len(pq))
                                if oracle.loop_test(int(wrecs[k]["good_count"]), int(counts[pq[k]]), int(counts[pt[k]]), p)[0]]
                        assert npairs == len(pq)
                        assert [(int(r["current_frame_id"]), int(r["matched_frame_id"]), int(r["num_matches"])) for r in cands] == keep
                if kind.startswith("g_") and kind != "g_refusals":
                    gi = g.info()
                    assert gi.arena_gather_skipped == (0 if s.changed and kind != "g_classic" else 1), (gi.arena_gather_skipped, s.changed)
                    assert gi.n_devices == world and gi.pairs == sum(len(M.elig(s.ids, q, s.gap)) for q in s.ids)
                    gathered += s.changed
                    skipped += not s.changed
                assert len(g) == len(s.frames)
            except Exception as e:
                raise AssertionError(f"world {world} seed {seed} step {n} {kind} ids {list(s.ids)} rows {[len(f) for f in s.frames]} gap {s.gap}") from e
    fig = dict(kinds=kinds, fallbacks=fallbacks, gathered=gathered, skipped=skipped, found=found, none=none)
    M.group_check(fig, M.GROUP_STEPS)
    assert fig == M.group_dry_run(seed, M.GROUP_STEPS, world)
