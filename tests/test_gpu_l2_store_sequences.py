"""The SIFT keyframe store and the loop verification behind it under random call sequences (lcm_l2_db_*, lcm_epi_db_*,
lcm_lo_db_*, lcm_pose_db_*: lcm_l2_db.cpp, lcm_l2.cpp, lcm_verify.cpp) against tests/l2storemodel.py.  Needs a real MI355X.

One long-lived handle per seed replays l2storemodel.ops(seed): appends with and without keypoints, truncates, searches, list
calls, verification calls, host-matrix calls that re-allocate the shared scratch between two store calls, Hamming calls, chunk
pins, refusals.  After every step every returned field is compared with the model (l2ref for counts, candidates and lists, a
gather on the bits for points, the closure on the device's own hypotheses, poseref bit for bit, the host-list calls for the local
optimisation), lcm_l2_db_info with the model's prediction, and the launch record with the planners' arithmetic.  `replay` repeats
the last calls on a second, fresh handle holding the same frames: every output byte must be equal, whatever the long-lived
handle's scratch, arenas, tables and events went through before.  It hunts state that outlives its validity."""
import numpy as np
import pytest

import epiref as E_
import l2storemodel as M
import poseref as P
import ratioref
from verifychecks import as_bytes, check_against_reference, check_closure

pytestmark = pytest.mark.gpu

SEEDS = M.SEEDS
TWINS = M.TWIN_SEEDS
FILL = 0xA7
ENV = {"list": "LCM_TUNE_L2_CHUNK", "count": "LCM_TUNE_L2_COUNT_CHUNK"}
ORB_ROWS, ORB_QUERY_ID = (40, 70, 33), 1000


def epi_params(pkg, ep):
    return pkg.capi.default_epi_params(E_.FX, E_.FY, E_.CX, E_.CY, iters=ep["iters"], seed=ep["seed"])


def lo_params(pkg, lp):
    return None if lp is None else pkg.capi.default_lo_params(mult=lp)


def info_dict(m):
    i = m.l2_db_info()
    return dict(frames=int(i.frames), tiles_used=int(i.tiles_used), tiles_reserved=int(i.tiles_reserved), device_bytes=int(i.device_bytes))


def filled(dtype, n, *tail):
    """A caller's buffer of n records (n, *tail) with every byte FILL."""
    dt = np.dtype(dtype)
    width = int(np.prod(tail, dtype=np.int64)) * dt.itemsize
    return np.full((max(n, 1), width), FILL, np.uint8).view(dt).reshape(max(n, 1), *tail)


def untouched(*arrays):
    return all((a.view(np.uint8) == FILL).all() for a in arrays)


def refused(pkg, code, fn, *a, **kw):
    with pytest.raises(pkg.LcmError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, code)


def hamming(q, t):
    return np.bitwise_count(q[:, None, :] ^ t[None, :, :]).sum(axis=2).astype(np.int64)


class Runner:
    """One handle and the stream it replays; `pins` (the two chunk variables) is the process's and may be shared."""

    def __init__(self, pkg, monkeypatch, pins, refs=None):
        self.pkg, self.mp, self.pins = pkg, monkeypatch, pins
        self.m = pkg.Matcher()
        self.refs = M.Refs() if refs is None else refs
        self.cov = M.Coverage()
        self.last = info_dict(self.m)
        self.orb = None
        assert self.last == M.Store().info()

    def close(self):
        self.m.close()

    # -- one step of the stream, every check included --
    def step(self, s):
        outs = self.run(self.m, s.kind, s.args, s.frames, True)
        after = info_dict(self.m)
        M.check_info(after, {k: v for k, v in s.info.items() if k != "grew"})
        assert self.m.l2_db_size() == len(s.frames)
        self.cov.step(s, self.last, after)
        if after["tiles_reserved"] != self.last["tiles_reserved"]:          # the arenas moved: every slot reads back bit for bit
            for k in range(len(s.frames)):
                self.read(self.m, k, s.frames)
        self.last = after
        return outs

    def read(self, m, slot, frames):
        f = frames[slot]
        assert m.l2_db_rows(slot) == len(f)
        assert m.l2_db_read(slot).tobytes() == f.rows.tobytes(), slot
        if f.pts is not None:
            assert M.bits(m.l2_db_read_kp(slot)).tobytes() == M.bits(f.pts).tobytes(), slot
        else:
            refused(self.pkg, self.pkg.capi.ERR_INVALID_ARG, m.l2_db_read_kp, slot)

    # -- the calls --
    def lists(self, m, sides, ratio, points, out, pts, offs):
        M.check_lists(out, pts if points else None, offs, M.want_lists(self.refs, sides, ratio, points))
        assert (out["img_idx"] == 0).all()
        M.check_launch(m.launch_info(), M.launch_of(sides, self.pins["list"], "list"))

    def closure(self, m, ep, res, mask, pts, offs):
        n = len(offs) - 1
        hyps = [m.epi_hypotheses(pts[int(offs[p]):int(offs[p + 1])], p, ep) for p in range(n)]
        with np.errstate(all="ignore"):
            check_closure(res, mask, pts, offs, hyps, range(n), ep.threshold)

    def pose(self, res, pres, mask, pmask, pts, offs):
        with np.errstate(all="ignore"):
            check_against_reference(pres, pmask, pts, offs, res["E"], mask, P.MAX_DEPTH)

    def composed(self, m, ep, lp, res, info, pres, mask, pmask, pts, offs):
        """The local optimisation's records as the host-list calls make them from the returned points."""
        if len(pts) == 0:
            assert not res["n_points"].any() and not mask.size
            return
        w_res, w_info, w_mask = m.lo_verify_pairs(pts, offs, ep, lp)
        assert as_bytes(res) == as_bytes(w_res) and as_bytes(info) == as_bytes(w_info) and as_bytes(mask) == as_bytes(w_mask)
        w_pose, w_pmask = m.pose_recover_pairs(pts, offs, res["E"], ep, None, mask)
        assert as_bytes(pres) == as_bytes(w_pose) and as_bytes(pmask) == as_bytes(w_pmask)
        self.pose(res, pres, mask, pmask, pts, offs)

    def search_kw(self, a):
        return dict(skip=a["skip"], ratio=a["ratio"], min_rows=a["min_rows"], min_matches=a["min_matches"])

    def run(self, m, kind, a, frames, own):
        """Runs one op on handle m and checks it against the model; returns the outputs (for `replay`).  own: m is the
        stream's long-lived handle (the ops that change or describe it run there only)."""
        pkg, refs, C = self.pkg, self.refs, self.pkg.capi
        if kind in ("append_kp", "append"):
            f = a["frame"]
            slot = m.l2_db_append_kp(f.rows, f.pts) if kind == "append_kp" else m.l2_db_append(f.rows)
            assert slot == len(frames) - 1
            return []
        if kind == "truncate":
            m.l2_db_truncate(a["n"])
            return []
        if kind == "clear":
            m.l2_db_clear()
            return []
        if kind == "read":
            self.read(m, a["slot"], frames)
            return []
        if kind == "chunk":
            for which, name in ENV.items():
                self.pins[which] = a[which]
                if a[which] is None:
                    self.mp.delenv(name, raising=False)
                else:
                    self.mp.setenv(name, str(a[which]))
            return []
        if kind == "score_pairs":
            sides = M.sides_of(frames, a["pairs"])
            got = m.l2_db_score_pairs(a["pairs"], a["ratio"])
            M.check_scores(got, M.want_scores(refs, sides, a["ratio"]))
            M.check_launch(m.launch_info(), M.launch_of(sides, self.pins["count"], "count"))
            return [got]
        if kind == "match_pairs":
            sides = M.sides_of(frames, a["pairs"])
            lists, offs = m.l2_db_match_pairs_ratio(a["pairs"], a["ratio"])
            out = np.concatenate(lists)
            self.lists(m, sides, a["ratio"], False, out, None, offs)
            return [out, offs]
        if kind in ("match_points", "match_points_plain"):
            sides, points = M.sides_of(frames, a["pairs"]), kind == "match_points"
            out, pts, offs = m.l2_db_match_points(a["pairs"], a["ratio"], points=points)
            self.lists(m, sides, a["ratio"], points, out, pts, offs)
            if not points:
                assert pts is None
                lists, offs2 = m.l2_db_match_pairs_ratio(a["pairs"], a["ratio"])
                assert as_bytes(np.concatenate(lists)) == as_bytes(out) and as_bytes(offs2) == as_bytes(offs)
            return [out, pts, offs]
        if kind == "loop_search":
            cands, scored, sides = M.want_search(refs, frames, a["gap"], a["skip"], a["ratio"], a["min_rows"], a["min_matches"])
            got, n_pairs = m.l2_db_loop_search(a["gap"], **self.search_kw(a))
            M.check_candidates(got, n_pairs, cands, scored)
            M.check_launch(m.launch_info(), M.launch_of(sides, self.pins["count"], "count"))
            return [got, n_pairs]
        query = a.get("query")
        q_rows = None if query is None else query.rows
        if kind in ("detect_stored", "detect_host"):
            cands, scored, sides, _ = M.want_detect(refs, frames, a, query)
            got, n_pairs = m.l2_db_detect_loops(a["curr"], a["gap"], query=q_rows, **self.search_kw(a))
            M.check_candidates(got, n_pairs, cands, scored)
            M.check_launch(m.launch_info(), M.launch_of(sides, self.pins["count"], "count"))
            return [got, n_pairs]
        if kind in ("points_stored", "points_host", "lo_detect_host") or (kind in M.VERIFY_KINDS and "curr" in a):
            cands, scored, sides, cand_sides = M.want_detect(refs, frames, a, query)
            kw = dict(query=q_rows, query_pts=None if query is None else query.pts, **self.search_kw(a))
            ep = epi_params(pkg, a["ep"]) if "ep" in a else None
            floor = a.get("floor", -1)
            if kind in ("points_stored", "points_host"):
                got = m.l2_db_detect_loops_points(a["curr"], a["gap"], points=a["points"], **kw)
            elif kind == "epi_db":
                got = m.epi_db_detect_loops(a["curr"], a["gap"], ep, **kw)
            elif kind == "pose_db":
                got = m.pose_db_detect_loops(a["curr"], a["gap"], ep, None, floor, **kw)
            else:
                got = m.lo_db_detect_loops(a["curr"], a["gap"], ep, lo_params(pkg, a["lp"]), None, floor, **kw)
            launch = m.launch_info()
            M.check_candidates(got[0], got[1], cands, scored)
            points = a.get("points", True)
            if kind in ("points_stored", "points_host"):
                out, pts, offs = got[2:5]
            elif kind == "epi_db":
                res, out, pts, mask, offs = got[2:7]
            elif kind == "pose_db":
                res, pres, out, pts, mask, pmask, offs, best = got[2:10]
            else:
                res, info, pres, out, pts, mask, pmask, offs, best = got[2:11]
            M.check_lists(out, pts if points else None, offs, M.want_lists(refs, cand_sides, a["ratio"], points))
            live = M.launch_of(cand_sides, self.pins["list"], "list")
            M.check_launch(launch, live if live else M.launch_of(sides, self.pins["count"], "count"))
            if kind == "epi_db":
                self.closure(m, ep, res, mask, pts, offs)
            elif kind == "pose_db":
                self.closure(m, ep, res, mask, pts, offs)
                self.pose(res, pres, mask, pmask, pts, offs)
            elif kind == "lo_detect_host":
                self.composed(m, ep, lo_params(pkg, a["lp"]), res, info, pres, mask, pmask, pts, offs)
            if kind in ("pose_db", "lo_detect_host"):
                assert best == C.pose_best(res, pres, ep, None, floor), (best, floor)
            if own and kind in M.VERIFY_KINDS:
                self.cov.verified(kind, cand_sides, offs)
            return list(got)
        if kind in M.VERIFY_KINDS:
            sides = M.sides_of(frames, a["pairs"])
            ep = epi_params(pkg, a["ep"])
            if kind == "epi_db":
                got = res, out, pts, mask, offs = m.epi_db_verify_pairs(a["pairs"], a["ratio"], ep)
            elif kind == "pose_db":
                got = res, pres, out, pts, mask, pmask, offs = m.pose_db_verify_pairs(a["pairs"], a["ratio"], ep)
            else:
                got = res, info, pres, out, pts, mask, pmask, offs = m.lo_db_verify_pairs(a["pairs"], a["ratio"], ep, lo_params(pkg, a["lp"]))
            self.lists(m, sides, a["ratio"], True, out, pts, offs)
            if kind == "lo_db":
                self.composed(m, ep, lo_params(pkg, a["lp"]), res, info, pres, mask, pmask, pts, offs)
            else:
                self.closure(m, ep, res, mask, pts, offs)
                if kind == "pose_db":
                    self.pose(res, pres, mask, pmask, pts, offs)
            if own:
                self.cov.verified(kind, sides, offs)
            return list(got)
        if kind == "host_matrix":
            return self.host_matrix(m, a)
        if kind == "hamming":
            return self.hamming(m, a)
        if kind == "cap_refusal":
            return self.cap_refusal(m, a, frames)
        if kind == "replay":
            return self.replay(a, frames)
        raise AssertionError(kind)

    def host_matrix(self, m, a):
        pkg, refs = self.pkg, self.refs
        if a["call"] in ("epi_verify_pairs", "lo_verify_pairs"):
            pts, ep = a["pts"], epi_params(pkg, a["ep"])
            offs = np.array([0, len(pts)], np.uintp)
            res, mask = m.epi_verify_pairs(pts, offs, ep)
            self.closure(m, ep, res, mask, pts, offs)
            if a["call"] == "lo_verify_pairs":
                res1, info1, mask1 = m.lo_verify_pairs(pts, offs, ep)
                assert info1[0]["n_inliers_ransac"] == res[0]["n_inliers"] <= res1[0]["n_inliers"] == int(mask1.sum())
            return []
        A, B = a["mats"]
        pairs = [(0, 1), (1, 0), (0, 0)]
        sides = M.sides_of((A, B), pairs)
        mats = [A.rows, B.rows]
        if a["call"] == "score_pairs_ratio_l2":
            M.check_scores(m.score_pairs_ratio_l2(mats, pairs, a["ratio"]), M.want_scores(refs, sides, a["ratio"]))
            M.check_launch(m.launch_info(), M.launch_of(sides, self.pins["count"], "count"))
        elif a["call"] == "match_pairs_ratio_l2":
            lists, offs = m.match_pairs_ratio_l2(mats, pairs, a["ratio"])
            self.lists(m, sides, a["ratio"], False, np.concatenate(lists), None, offs)
        else:
            idx, dist, dsq = m.knn2_pair_l2(A.rows, B.rows)
            if len(A) and len(B):
                (w_idx, w_dist, w_dsq), _ = refs.pair(A, B)
                assert as_bytes(idx) == as_bytes(w_idx) and as_bytes(dist) == as_bytes(w_dist) and as_bytes(dsq) == as_bytes(w_dsq)
            else:
                assert len(idx) == 0
        return []

    def hamming(self, m, a):
        if self.orb is None:
            rng = np.random.default_rng(3)
            self.orb = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in ORB_ROWS]
            for k, f in enumerate(self.orb):
                m.append(k, f)
        q, t = a["q"], a["t"]
        idx, dist = m.match_pair(q, t)
        D = hamming(q, t)
        np.testing.assert_array_equal(idx, D.argmin(axis=1))
        np.testing.assert_array_equal(dist, D.min(axis=1))
        scores, ids = m.query_scores_ratio(q, ORB_QUERY_ID, a["ratio"])
        assert ids.tolist() == list(range(len(self.orb)))
        for k, f in enumerate(self.orb):
            assert (int(scores[k]["good_count"]), int(scores[k]["min_dist"])) == ratioref.ratio_counts(q, f, a["ratio"]), k
            assert scores[k]["n_train"] == len(f)
        return []

    def cap_refusal(self, m, a, frames):
        pkg, refs, C = self.pkg, self.refs, self.pkg.capi
        x, y = a["pair"]
        if a["form"] == "no_points":
            refused(pkg, C.ERR_INVALID_ARG, m.l2_db_match_points, [(x, y), (a["plain"], y)], 0.7)
            refused(pkg, C.ERR_INVALID_ARG, m.l2_db_match_points, [(y, a["plain"])], 0.7)
            return []
        if a["form"] == "cand_cap":
            curr = max(k for k, f in enumerate(frames) if f.pts is not None and len(f))
            ok = [f.pts is not None or len(f) == 0 for f in frames]
            args = dict(curr=curr, gap=1, skip=[0 if o else 1 for o in ok], ratio=0.7, min_rows=0, min_matches=0)
            want, _, _, _ = M.want_detect(refs, frames, args)
            assert len(want) >= 1
            cands = filled(C.CANDIDATE_DTYPE, len(want))
            refused(pkg, C.ERR_CAPACITY, m.l2_db_detect_loops_points, curr, 1, cands=cands, cand_cap=len(want) - 1, cap=1 << 16,
                    **self.search_kw(args))
            assert m.last_n_cands.value == len(want) and untouched(cands) and int(m.last_offsets[0]) == 0
            return []
        sides = [(frames[x], frames[y])]
        _, _, w_offs = want = M.want_lists(refs, sides, 1e30, True)
        total = int(w_offs[-1])
        assert total >= 1
        out, pts = filled(C.DMATCH_DTYPE, total), filled(np.float32, total, 4)
        if a["form"] == "match_points":
            refused(pkg, C.ERR_CAPACITY, m.l2_db_match_points, [(x, y)], 1e30, cap=total - 1, out=out, pts=pts)
            assert untouched(out, pts)
        else:
            res, mask = filled(C.EPI_RESULT_DTYPE, 1), filled(np.uint8, total)
            refused(pkg, C.ERR_CAPACITY, m.epi_db_verify_pairs, [(x, y)], 1e30, epi_params(pkg, a["ep"]), cap=total - 1, out=out, pts=pts,
                    results=res, mask=mask)
            assert untouched(out, pts, res, mask)
        assert int(m.last_offsets[1]) == total
        launch = m.launch_info()                      # the refused call's own record: both event pairs were recorded
        M.check_launch(launch, M.launch_of(sides, self.pins["list"], "list"))
        assert launch.kernel_ms > 0 and launch.aux_kernel_ms > 0, (launch.kernel_ms, launch.aux_kernel_ms)
        return []

    def replay(self, a, frames):
        """The calls again here, then on a fresh handle with the same frames: the same bytes."""
        mine = [self.run(self.m, k, args, frames, False) for k, args in a["calls"]]
        fresh = self.pkg.Matcher()
        try:
            for k, f in enumerate(frames):
                assert (fresh.l2_db_append(f.rows) if f.pts is None else fresh.l2_db_append_kp(f.rows, f.pts)) == k
            theirs = [self.run(fresh, k, args, frames, False) for k, args in a["calls"]]
        finally:
            fresh.close()
        for (k, _), x, y in zip(a["calls"], mine, theirs):
            assert len(x) == len(y)
            for j, (u, v) in enumerate(zip(x, y)):
                assert (u is None) == (v is None) and (u is None or as_bytes(np.asarray(u)) == as_bytes(np.asarray(v))), (k, j)
        return []

    def finish(self, seed, n_steps, lift):
        """What the sequence reached, from what ran and what lcm_l2_db_info said: the dry run's conditions and its very figures."""
        self.cov.check(lift)
        dry = M.dry_run(seed, n_steps, lift, self.refs)
        assert self.cov.summary() == dry.summary() and self.cov.edges == dry.edges and self.cov.kinds == dry.kinds


def fresh_pins(monkeypatch):
    for name in ENV.values():
        monkeypatch.delenv(name, raising=False)
    return {"list": None, "count": None}


@pytest.mark.parametrize("seed", SEEDS)
def test_random_store_sequences_equal_model(pkg, monkeypatch, seed):
    r = Runner(pkg, monkeypatch, fresh_pins(monkeypatch))
    lift = seed == M.LIFT_SEED
    try:
        for n, s in enumerate(M.ops(seed, M.STEPS, lift)):
            try:
                r.step(s)
            except Exception as e:
                raise AssertionError(f"seed {seed} step {n} {s.kind} {M.describe(s)}") from e
        r.finish(seed, M.STEPS, lift)
    finally:
        r.close()


@pytest.mark.parametrize("seeds", TWINS, ids=lambda t: f"{t[0]}-{t[1]}")
def test_two_handles_interleaved(pkg, monkeypatch, seeds):
    """Two handles in one process, their streams in alternating steps: nothing process-wide leaks between them - the scratch
    of one, or the chunk pins, which either stream sets and both read per call."""
    pins = fresh_pins(monkeypatch)
    runners = [Runner(pkg, monkeypatch, pins) for _ in seeds]
    try:
        streams = [M.ops(seed, M.TWIN_STEPS) for seed in seeds]
        for n in range(M.TWIN_STEPS):
            for seed, r, stream in zip(seeds, runners, streams):
                s = next(stream)
                try:
                    r.step(s)
                except Exception as e:
                    raise AssertionError(f"seed {seed} step {n} {s.kind} {M.describe(s)}") from e
        for seed, r in zip(seeds, runners):
            r.finish(seed, M.TWIN_STEPS, False)
    finally:
        for r in runners:
            r.close()
