"""The size envelope include/lcm.h documents, on the device: frames of 65535 rows (stored and as query) on every route
that stores or scores them, a pair-mode train matrix of LCM_MAX_TRAIN_ROWS = 2^22 rows, and a database arena beyond
2^32 bytes.  Inputs and what they plant: tests/limitcases.py.  Expected records and index checksums come from the
oracle's tuned path (one call over all pairs; pinned to the scalar oracle on crops in test_limit_cases_host.py), match
lists from oracle.match_features where the scalar oracle can afford them, pair mode from a plain numpy scan.

Every test owns its handle and frees it in `finally`; nothing is retried."""
import numpy as np
import pytest

import knnref
import limitcases as L
import ratioref

pytestmark = pytest.mark.gpu

GAP = 1
D = L.TALL_ROWS.index(65535)            # the 65535-row frame
B = L.TALL_ROWS.index(2000)             # a 2000-row frame: the <= 2048-row query of the plain / matrix routes
E = L.TALL_ROWS.index(0)
F = L.TALL_ROWS.index(2049)


@pytest.fixture(scope="module")
def tall():
    return L.tall_set()


@pytest.fixture(scope="module")
def want(tall, oracle):
    """(query frame, stored frame) -> (record, index checksum): the self search's pairs plus frame B against every frame."""
    pq, pt, offs = L.tall_pairs(tall, GAP)
    n_self = len(pq)
    pq = pq + [B] * tall.n_frames
    pt = pt + list(range(tall.n_frames))
    p = oracle.default_params(min_gap=GAP)
    sc, sums = oracle.fast_score_pairs_idx(tall.rows, tall.counts, pq, pt, p, n_threads=16)
    L.check_expected(tall, pq[:n_self], pt[:n_self], sc[:n_self], sums[:n_self])
    table = {}
    for k in range(len(pq) - 1, -1, -1):
        table[(pq[k], pt[k])] = (sc[k], int(sums[k]))
    return {"table": table, "scores": sc[:n_self].copy(), "sums": sums[:n_self].copy(), "offs": offs, "p": p}


def _params(pkg, **kw):
    p = pkg.default_params()
    p.min_gap = GAP
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _fill(m, tall):
    for f in range(tall.n_frames):
        m.append(int(tall.ids[f]), tall.frame(f))


def _check_store(m, tall, order=None, ids=None):
    order = list(range(tall.n_frames)) if order is None else order
    ids = tall.ids if ids is None else ids
    assert len(m) == len(order)
    for slot, f in enumerate(order):
        assert m.frame_info(slot) == (int(ids[slot]), int(tall.counts[f]), int(tall.counts[f]))
        np.testing.assert_array_equal(m.read_frame(slot), tall.frame(f))


def _row(want, c, stored):
    """Expected records / checksums of query frame c against stored frames `stored`."""
    sc = np.array([want["table"][(c, i)][0] for i in stored], dtype=want["scores"].dtype)
    su = np.array([want["table"][(c, i)][1] for i in stored], np.uint32)
    return sc, su


def _cands(oracle, tall, want, c, stored):
    out = []
    for i in stored:
        s = want["table"][(c, i)][0]
        ok, sim = oracle.loop_test(int(s["good_count"]), int(tall.counts[c]), int(tall.counts[i]), want["p"])
        if ok:
            out.append((int(tall.ids[c]), int(tall.ids[i]), int(s["good_count"]), sim))
    return out


def _tuples(c):
    return [(int(r["current_frame_id"]), int(r["matched_frame_id"]), int(r["num_matches"]), float(r["similarity_score"])) for r in c]


def _self_cands(oracle, tall, want):
    return [t for c in range(tall.n_frames) for t in _cands(oracle, tall, want, c, list(range(c)))]


# ---- stored frames at the limit ------------------------------------------------------------------------------------

def test_store_tall_frames_reserved_save_load_and_group(pkg, oracle, tall, want, tmp_path):
    """lcm_db_reserve(n, 65535) up front, host appends, read-back, snapshot round trip; the file then loads into a
    W = 3 loopback group, which scores it in bulk and online."""
    path = str(tmp_path / "tall.lcmdb")
    m = pkg.Matcher(_params(pkg))
    try:
        m.reserve(tall.n_frames, 65535)
        _fill(m, tall)
        _check_store(m, tall)
        m.save(path)
        m.clear()
        assert len(m) == 0
        m.load(path)
        _check_store(m, tall)
        sc, ids = m.query_scores(tall.frame(D), int(tall.ids[D]))          # the loaded arena scores as the appended one
        np.testing.assert_array_equal(sc, _row(want, D, range(D))[0])
    finally:
        m.close()
    with pkg.Group(_params(pkg), n_devices=3, loopback_device=0) as g:
        g.load(path)
        assert len(g) == tall.n_frames and g.world == 3
        for variant in (0, 1):
            g.set_kernel_variant(variant)
            sc, sums, offs = g.all_vs_all_argmin()
            np.testing.assert_array_equal(np.asarray(offs, np.int64), want["offs"])
            np.testing.assert_array_equal(sc, want["scores"])
            np.testing.assert_array_equal(sums, want["sums"])
            merged, _ = g.all_vs_all()
            np.testing.assert_array_equal(merged, want["scores"])
            cands, npairs = g.all_vs_all_loops(cap=len(sc))
            assert npairs == len(sc) and _tuples(cands) == _self_cands(oracle, tall, want)
            for c in (D, 9):                                             # online over the shards: 65535 and 65531 rows
                qs, qi = g.query_scores(tall.frame(c), int(tall.ids[c]))
                np.testing.assert_array_equal(qs, _row(want, c, range(c))[0])
                np.testing.assert_array_equal(qi, tall.ids[:c])
                assert _tuples(g.detect_loops(int(tall.ids[c]), tall.frame(c))) == _cands(oracle, tall, want, c, range(c))
            batch = [D, E, F]
            bs, boffs = g.query_scores_batch([tall.frame(c) for c in batch], [int(tall.ids[c]) for c in batch])
            for k, c in enumerate(batch):
                np.testing.assert_array_equal(bs[int(boffs[k]): int(boffs[k + 1])], _row(want, c, range(c))[0])


def test_store_tall_frames_growing_arena_host_and_device_appends(pkg, tall):
    """No reserve: the arena re-pitches as taller frames arrive (2000 -> ... -> 65536 rows of stride), frames alternately
    from host rows and from device rows; every earlier frame survives every re-pitch."""
    order = sorted(range(tall.n_frames), key=lambda f: (int(tall.counts[f]), f))
    ids = np.arange(len(order), dtype=np.int32) * 7 + 1
    m = pkg.Matcher(_params(pkg))
    d = None
    try:
        d = m.dev_alloc(L.MAX_ROWS * 32)
        for slot, f in enumerate(order):
            n = int(tall.counts[f])
            if slot % 2 == 0 and n > 0:
                m.dev_upload(d, tall.frame(f))
                m.append_device(int(ids[slot]), d, n)
                m.sync()                                    # the buffer is reused for the next device append
            else:
                m.append(int(ids[slot]), tall.frame(f))
            if n in (2049, 32769, 65531, 65535):
                _check_store(m, tall, order[: slot + 1], ids)
        assert [int(tall.counts[f]) for f in order[-3:]] == [65533, 65534, 65535]
        _check_store(m, tall, order, ids)
    finally:
        if d is not None:
            m.dev_free(d)
        m.close()


@pytest.mark.parametrize("rows", [65533, 65534, 65535])
@pytest.mark.parametrize("how", ["reserve", "append", "append_device"])
def test_the_last_three_row_counts_are_accepted(pkg, tall, how, rows):
    """round_up(rows, 4) = 65536 for all three: the arena's stride reaches 65536 rows, the frame keeps its own count."""
    f = L.TALL_ROWS.index(rows)
    m = pkg.Matcher(_params(pkg))
    d = None
    try:
        if how == "reserve":
            m.reserve(2, rows)
        if how == "append_device":
            d = m.dev_alloc(rows * 32)
            m.dev_upload(d, tall.frame(f))
            m.append_device(9, d, rows)
        else:
            m.append(9, tall.frame(f))
        m.append(12, tall.frame(B))                         # the next slot starts one stride further
        assert m.frame_info(0) == (9, rows, rows)
        np.testing.assert_array_equal(m.read_frame(0), tall.frame(f))
        np.testing.assert_array_equal(m.read_frame(1), tall.frame(B))
    finally:
        if d is not None:
            m.dev_free(d)
        m.close()


# ---- every route that scores them ----------------------------------------------------------------------------------

def test_bulk_routes_on_tall_frames(pkg, oracle, tall, want):
    """lcm_all_vs_all / _argmin (records + index checksums) self and external, LCM_TUNE_PACKED 1 / 2 / -1, kernel variants
    0 / 1 (and 4 / 5, which fall back to the packed vector-ALU route for query frames above 2048 rows), a 1 MiB scratch
    (one 65535-row pair then spans several chunks: the plan keeps at least one pair per chunk and never refuses), the
    fused loop search; then <= 2048-row external queries against the 65535-row stored frames on the plain route under
    variants 0 .. 3 and on the matrix route under 4 / 5."""
    cp = pkg.capi
    n = len(want["scores"])
    m = pkg.Matcher(_params(pkg))
    bufs = []
    try:
        _fill(m, tall)
        d, ds = m.dev_alloc(n * 8), m.dev_alloc(n * 4)
        d_rows, d_counts = m.dev_alloc(tall.rows.nbytes), m.dev_alloc(tall.counts.nbytes)
        bufs += [d, ds, d_rows, d_counts]
        m.dev_upload(d_rows, tall.rows); m.dev_upload(d_counts, tall.counts)
        got, sums = np.zeros(n, want["scores"].dtype), np.zeros(n, np.uint32)
        ext = dict(d_query_rows=d_rows, d_query_counts=d_counts, q_ids=tall.ids, q_stride_rows=tall.stride_rows)

        def run(kw, label):
            np_, offs = m.all_vs_all_plan(**kw)
            assert np_ == n and np.array_equal(offs.astype(np.int64), want["offs"]), label
            got[:] = 0
            m.all_vs_all(d, n, **kw)
            assert m.launch_info().route == cp.ROUTE_PACKED, label
            m.sync(); m.dev_download(d, got)
            np.testing.assert_array_equal(got, want["scores"], err_msg=label)
            got[:] = 0; sums[:] = 0xDEADBEEF
            m.all_vs_all_argmin(d, n, ds, **kw)
            info = m.launch_info()
            assert info.route == cp.ROUTE_PACKED, label
            m.sync(); m.dev_download(d, got); m.dev_download(ds, sums)
            np.testing.assert_array_equal(got, want["scores"], err_msg=label)
            np.testing.assert_array_equal(sums, want["sums"], err_msg=label)
            return info

        for variant in (0, 1):
            m.set_kernel_variant(variant)
            for packed in (1, 2, -1):
                m.set_tuning(cp.TUNE_PACKED, packed)
                for kw, name in (({}, "self"), (ext, "external")):
                    run(kw, f"variant {variant} packed {packed} {name}")
            m.set_tuning(cp.TUNE_PACKED, -1)
            m.set_tuning(cp.TUNE_PACKED_SCRATCH_MB, 1)
            for kw, name in (({}, "self"), (ext, "external")):
                info = run(kw, f"variant {variant} scratch 1 MiB {name}")
                assert info.score_launches > 1, "a 1 MiB scratch holds 2 pairs of 65535 rows: several chunks"
            m.set_tuning(cp.TUNE_PACKED_SCRATCH_MB, 1024)
            cands, npairs = m.all_vs_all_loops(cap=n)
            assert npairs == n and _tuples(cands) == _self_cands(oracle, tall, want)
            np.testing.assert_array_equal(m.last_bulk_scores(), want["scores"])
        for variant in (4, 5):                                # tall query frames: the matrix variants fall back
            m.set_kernel_variant(variant)
            run({}, f"variant {variant} self")
        # <= 2048-row query frames (2000 and 96 rows) from a caller's buffer against all stored frames
        small = [B, L.CROP]
        q_rows = np.zeros((2, 2048, 32), np.uint8)
        for k, c in enumerate(small):
            q_rows[k, : tall.counts[c]] = tall.frame(c)
        q_counts = tall.counts[small].astype(np.int32)
        q_ids = np.array([int(tall.ids[-1]) + 10, int(tall.ids[-1]) + 20], np.int32)
        dq, dc = m.dev_alloc(q_rows.nbytes), m.dev_alloc(q_counts.nbytes)
        bufs += [dq, dc]
        m.dev_upload(dq, q_rows); m.dev_upload(dc, q_counts)
        allf = list(range(tall.n_frames))
        w_b, s_b = _row(want, B, allf)
        w_c, s_c = _row(want, L.CROP, allf[: L.CROP])
        # the crop frame against itself is not in the table: score it with the oracle here (96 x 96)
        own, own_s = oracle.fast_score_pairs_idx(tall.rows, tall.counts, [L.CROP], [L.CROP], want["p"], n_threads=1)
        w2 = np.concatenate([w_b, w_c, own]); s2 = np.concatenate([s_b, s_c, own_s])
        g2, gs2 = np.zeros(len(w2), w2.dtype), np.zeros(len(w2), np.uint32)
        skw = dict(d_query_rows=dq, d_query_counts=dc, q_ids=q_ids, q_stride_rows=2048)
        for variant in range(6):
            m.set_kernel_variant(variant)
            m.set_tuning(cp.TUNE_PACKED, 0)
            g2[:] = 0
            assert m.all_vs_all(d, n, **skw) == len(w2)
            assert m.launch_info().route == (cp.ROUTE_MATRIX if variant >= 4 else cp.ROUTE_PLAIN), variant
            m.sync(); m.dev_download(d, g2)
            np.testing.assert_array_equal(g2, w2, err_msg=f"variant {variant} plain")
            g2[:] = 0; gs2[:] = 0xDEADBEEF
            m.all_vs_all_argmin(d, n, ds, **skw)
            m.sync(); m.dev_download(d, g2); m.dev_download(ds, gs2)
            np.testing.assert_array_equal(g2, w2, err_msg=f"variant {variant} argmin")
            np.testing.assert_array_equal(gs2, s2, err_msg=f"variant {variant} argmin")
            m.set_tuning(cp.TUNE_PACKED, -1)
            sc, _ = m.query_scores(tall.frame(B), int(q_ids[0]))           # online, <= 2048 rows, all six variants
            np.testing.assert_array_equal(sc, w_b, err_msg=f"variant {variant} online")
    finally:
        for b in bufs:
            m.dev_free(b)
        m.close()


def test_online_routes_on_tall_frames(pkg, oracle, tall, want):
    """lcm_query_scores with host rows of up to 65535, lcm_query_submit_batch mixing 65535-, 2049- and 0-row frames,
    lcm_detect_loops with the query stored and host-given; kernel variants 0 / 1, and 4 / 5 falling back."""
    m = pkg.Matcher(_params(pkg))
    try:
        _fill(m, tall)
        for variant in (0, 1, 4, 5):
            m.set_kernel_variant(variant)
            for c in ([D, 9, 6, 7] if variant < 4 else [D]):
                sc, ids = m.query_scores(tall.frame(c), int(tall.ids[c]))
                np.testing.assert_array_equal(sc, _row(want, c, range(c))[0], err_msg=f"variant {variant} frame {c}")
                np.testing.assert_array_equal(ids, tall.ids[:c])
                wc = _cands(oracle, tall, want, c, range(c))
                assert _tuples(m.detect_loops(int(tall.ids[c]))) == wc                      # the stored frame is the query
                assert _tuples(m.detect_loops(int(tall.ids[c]), tall.frame(c))) == wc       # the same frame as host rows
            batch = [D, E, F, 8]                              # 65535, 0, 2049 and 65532 rows in one submit
            t = m.query_submit_batch([tall.frame(c) for c in batch], [int(tall.ids[c]) for c in batch])
            bs, boffs = m.query_collect_batch(t)
            for k, c in enumerate(batch):
                np.testing.assert_array_equal(bs[int(boffs[k]): int(boffs[k + 1])], _row(want, c, range(c))[0])
        assert len(_cands(oracle, tall, want, 6, range(6))) > 0                             # MANY is a loop: 61000 / 65533
    finally:
        m.close()


def _check_list(tall, want, lst, min_d, c, i):
    """A match list too long for the scalar oracle: pinned by the tuned oracle's record and index checksum, by the planted
    rows, and by recomputing every listed distance."""
    s, csum = want["table"][(c, i)]
    assert len(lst) == int(s["good_count"]) and min_d == int(s["min_dist"])
    assert int(lst["train_idx"].astype(np.uint64).sum() % (1 << 32)) == csum
    assert np.all(np.diff(lst["query_idx"]) > 0) and not lst["img_idx"].any()
    q64 = tall.frame(c)[lst["query_idx"]].view(np.uint64)
    t64 = tall.frame(i)[lst["train_idx"]].view(np.uint64)
    np.testing.assert_array_equal(np.bitwise_count(q64 ^ t64).sum(axis=1), lst["distance"].astype(np.int64))
    assert float(lst["distance"].max()) <= 2 * min_d
    k0 = tall.k0.get((c, i))
    by_q = {int(r["query_idx"]): r for r in lst}
    for p in tall.plants:
        if (p.qf, p.tf) == (c, i) and k0 is not None and p.k <= 2 * k0:
            assert (int(by_q[p.qr]["train_idx"]), float(by_q[p.qr]["distance"])) == (p.tr, float(p.k)), p


def test_match_lists_on_tall_pairs(pkg, oracle, tall, want):
    """lcm_match_stored, lcm_match_stored_batch and lcm_match_query_batch: full DMatch lists against oracle.match_features
    for the 96-row crop frame against the 65535- and 65534-row frames, and tall x tall pairs (65531 x 65532, the pair with
    61000 good matches, 65535 x 65534) pinned by record, checksum, planted rows and recomputed distances."""
    ids = [int(x) for x in tall.ids]
    m = pkg.Matcher(_params(pkg))
    try:
        _fill(m, tall)
        p = want["p"]
        full = [(L.CROP, D), (L.CROP, 0)]
        refs = {pr: oracle.match_features(tall.frame(pr[0]), tall.frame(pr[1]), p) for pr in full}
        for variant in (0, 1):                                  # pair mode runs its own kernels under every variant
            m.set_kernel_variant(variant)
            for (c, i), (om, omin) in refs.items():
                lst, md = m.match_stored(ids[c], ids[i])
                np.testing.assert_array_equal(lst, om.astype(lst.dtype))
                assert md == omin
            lst, md = m.match_stored(ids[9], ids[8])
            _check_list(tall, want, lst, md, 9, 8)
        assert set(int(t) for t in refs[(L.CROP, D)][0]["train_idx"]) >= {0, 2048, 32767, 32768, 65531, 65532, 65533, 65534}
        big = [(9, 8), L.MANY, (D, 0)]
        for c, i in big:
            lst, md = m.match_stored(ids[c], ids[i])
            _check_list(tall, want, lst, md, c, i)
        pairs = full + big + [L.FAR, (E, 0), (9, E)]
        lists, mds = m.match_stored_batch([(ids[c], ids[i]) for c, i in pairs], cap=sum(int(tall.counts[c]) for c, _ in pairs))
        for (c, i), lst, md in zip(pairs, lists, mds):
            if (c, i) in refs:
                np.testing.assert_array_equal(lst, refs[(c, i)][0].astype(lst.dtype))
                assert int(md) == refs[(c, i)][1]
            elif E in (c, i):
                assert len(lst) == 0 and int(md) == -1
            else:
                _check_list(tall, want, lst, int(md), c, i)
        # the host-given query: the crop frame (full lists), and the 65531-row frame against two tall stored frames
        lists, mds = m.match_query_batch(tall.frame(L.CROP), [ids[D], ids[0]])
        for (c, i), lst, md in zip(full, lists, mds):
            np.testing.assert_array_equal(lst, refs[(c, i)][0].astype(lst.dtype))
            assert int(md) == refs[(c, i)][1]
        lists, mds = m.match_query_batch(tall.frame(9), [ids[8], ids[D]])
        for i, lst, md in zip((8, D), lists, mds):
            _check_list(tall, want, lst, int(md), 9, i)
    finally:
        m.close()


def test_host_class_process_frame_on_tall_frames(pkg, oracle, tall, want):
    """The host class owns its matcher and offers no kernel-variant switch: the default variant (0) only."""
    sys_ = pkg.LoopClosingSystem(want["p"].sim_threshold, GAP)
    try:
        for f in range(tall.n_frames):
            sys_.processFrame(tall.frame(f), int(tall.ids[f]))
        assert sys_.numFrames() == tall.n_frames
        wc = _self_cands(oracle, tall, want)
        assert len(wc) > 0 and _tuples(sys_.getLoopClosures()) == wc
    finally:
        sys_.close()


def test_cross_check_small_queries_against_tall_stored_frames(pkg, oracle, tall):
    """cross_check keeps query frames at 2048 rows but not stored frames: 2000- and 96-row queries against the 65535-,
    65534- ... row stored frames under both cross-check rules — bulk external (records + index checksums, route
    asserted), online single and detectLoops — so that k_cross_score's record (n_train above 32767) is reached."""
    cp = pkg.capi
    small = [B, L.CROP]
    allf = list(range(tall.n_frames))
    q_rows = np.zeros((2, 2048, 32), np.uint8)
    for k, c in enumerate(small):
        q_rows[k, : tall.counts[c]] = tall.frame(c)
    q_counts = tall.counts[small].astype(np.int32)
    q_ids = np.array([int(tall.ids[-1]) + 10, int(tall.ids[-1]) + 20], np.int32)
    pq = [c for c in small for _ in allf]
    pt = allf * 2
    n = len(pq)
    m = pkg.Matcher(_params(pkg, cross_check=1))
    bufs = []
    try:
        _fill(m, tall)
        d, ds = m.dev_alloc(n * 8), m.dev_alloc(n * 4)
        dq, dc = m.dev_alloc(q_rows.nbytes), m.dev_alloc(q_counts.nbytes)
        bufs += [d, ds, dq, dc]
        m.dev_upload(dq, q_rows); m.dev_upload(dc, q_counts)
        kw = dict(d_query_rows=dq, d_query_counts=dc, q_ids=q_ids, q_stride_rows=2048)
        for mode, variant in ((1, 0), (2, 0), (1, 1), (2, 1)):
            m.set_params(cross_check=mode)
            m.set_kernel_variant(variant)
            p = oracle.default_params(min_gap=GAP, cross_check=mode)
            wsc, wsum = oracle.fast_score_pairs_idx(tall.rows, tall.counts, pq, pt, p, n_threads=16)
            assert wsc[0] == oracle.pair_score(tall.frame(B), tall.frame(0), p)          # tuned == scalar on 2000 x 65534
            assert {65535, 65534, 65533, 32768} <= set(int(x) for x in wsc["n_train"])
            got, sums = np.zeros(n, wsc.dtype), np.full(n, 0xDEADBEEF, np.uint32)
            assert m.all_vs_all(d, n, **kw) == n
            assert m.launch_info().route == cp.ROUTE_CROSS
            m.sync(); m.dev_download(d, got)
            np.testing.assert_array_equal(got, wsc, err_msg=f"cross_check {mode}")
            got[:] = 0
            m.all_vs_all_argmin(d, n, ds, **kw)
            m.sync(); m.dev_download(d, got); m.dev_download(ds, sums)
            np.testing.assert_array_equal(got, wsc, err_msg=f"cross_check {mode} argmin")
            np.testing.assert_array_equal(sums, wsum, err_msg=f"cross_check {mode} argmin")
            for k, c in enumerate(small):
                w = wsc[k * len(allf): (k + 1) * len(allf)]
                sc, _ = m.query_scores(tall.frame(c), int(q_ids[k]))
                np.testing.assert_array_equal(sc, w, err_msg=f"cross_check {mode} online frame {c}")
                wc = []
                for i in allf:
                    ok, sim = oracle.loop_test(int(w[i]["good_count"]), int(tall.counts[c]), int(tall.counts[i]), p)
                    if ok:
                        wc.append((int(q_ids[k]), int(tall.ids[i]), int(w[i]["good_count"]), sim))
                assert _tuples(m.detect_loops(int(q_ids[k]), tall.frame(c))) == wc
    finally:
        for b in bufs:
            m.dev_free(b)
        m.close()


# ---- refusals ------------------------------------------------------------------------------------------------------

def test_refusals_beyond_the_limits_leave_the_handle_usable(pkg, oracle, tall, want):
    cp = pkg.capi
    m = pkg.Matcher(_params(pkg))
    too_tall = np.zeros((65536, 32), np.uint8)
    d = None

    def refused(fn, *a, **kw):
        with pytest.raises(cp.LcmError) as e:
            fn(*a, **kw)
        assert e.value.code == cp.ERR_CAPACITY, e.value
        assert len(str(e.value)) > 20                       # says why

    try:
        m.append(int(tall.ids[0]), tall.frame(0))
        m.append(int(tall.ids[1]), tall.frame(1))
        refused(m.append, 50, too_tall)
        d = m.dev_alloc(too_tall.nbytes)
        refused(m.append_device, 50, d, 65536)
        refused(m.reserve, 4, 65536)
        refused(m.query_scores, too_tall, 60)
        refused(m.query_submit_batch, [tall.frame(1), too_tall], [60, 61])
        refused(m.detect_loops, 60, too_tall)
        assert len(m) == 2
        m.set_params(cross_check=1)                         # cross_check keeps the 2048-row limit on query frames
        refused(m.query_scores, tall.frame(0), 60)
        refused(m.detect_loops, 60, tall.frame(0))
        m.set_params(cross_check=0)
        # ... and the handle still stores and scores
        m.append(int(tall.ids[2]), tall.frame(2))
        m.append(int(tall.ids[3]), tall.frame(3))
        _check_store(m, tall, [0, 1, 2, 3], tall.ids[:4])
        sc, _ = m.query_scores(tall.frame(D), int(tall.ids[D]))
        np.testing.assert_array_equal(sc, _row(want, D, range(D))[0])
    finally:
        if d is not None:
            m.dev_free(d)
        m.close()


def test_match_pair_refuses_more_than_2_22_train_rows(pkg):
    """nt = 2^22 + 1 with real buffers: LCM_ERR_CAPACITY, and the next call on the handle works."""
    cp = pkg.capi
    rng = np.random.default_rng(5)
    train = rng.integers(0, 256, (L.WIDE_NT + 1, 32), dtype=np.uint8)
    q = train[[0, L.WIDE_NT]].copy()
    m = pkg.Matcher()
    try:
        with pytest.raises(cp.LcmError) as e:
            m.match_pair(q, train)
        assert e.value.code == cp.ERR_CAPACITY
        with pytest.raises(cp.LcmError) as e:
            m.match_features(q, train)
        assert e.value.code == cp.ERR_CAPACITY
        idx, dist = m.match_pair(q, train[1:])              # 2^22 rows: served
        assert idx.tolist() == [L.scan(train[1:], q[0])[0], L.WIDE_NT - 1] and int(dist[1]) == 0
    finally:
        m.close()


# ---- pair mode at 2^22 train rows ----------------------------------------------------------------------------------

def test_pair_mode_with_2_22_train_rows(pkg):
    """lcm_match_pair / lcm_match_features on the wide case: all query rows (above 64 M distances: the throughput shape)
    and the first 16 (the latency shape) under LCM_TUNE_PAIR_UPLOAD_KERNEL x LCM_TUNE_PAIR_HOST_FOLD; train indices and
    distances equal the numpy scan."""
    cp = pkg.capi
    case = L.wide_case()
    w_idx, w_dist = L.wide_scan(case)
    np.testing.assert_array_equal(w_idx, case.want_idx)      # the scan finds what was planted
    np.testing.assert_array_equal(w_dist, case.want_dist)
    m = pkg.Matcher()
    try:
        for nq in (len(case.query), 16):
            for up in (1, 0):
                for fold in (1, 0):
                    m.set_tuning(cp.TUNE_PAIR_UPLOAD_KERNEL, up)
                    m.set_tuning(cp.TUNE_PAIR_HOST_FOLD, fold)
                    label = f"nq {nq} upload kernel {up} host fold {fold}"
                    idx, dist = m.match_pair(case.query[:nq], case.train)
                    info = m.launch_info()
                    assert info.distances == nq * L.WIDE_NT
                    # one work item per train segment (one query chunk): ties limitcases.pair_segment_rows to the product
                    assert info.workgroups == -(-L.WIDE_NT // L.WIDE_SEG), (info.workgroups, L.WIDE_SEG)
                    np.testing.assert_array_equal(idx, w_idx[:nq], err_msg=label)
                    np.testing.assert_array_equal(dist.astype(np.int32), w_dist[:nq], err_msg=label)
                    lst, md = m.match_features(case.query[:nq], case.train)
                    keep = w_dist[:nq] <= 2 * int(w_dist[:nq].min())          # min is 0: only the exact copy survives
                    assert md == int(w_dist[:nq].min()) == 0
                    np.testing.assert_array_equal(lst["query_idx"], np.nonzero(keep)[0])
                    np.testing.assert_array_equal(lst["train_idx"], w_idx[:nq][keep])
                    np.testing.assert_array_equal(lst["distance"], w_dist[:nq][keep].astype(np.float32))
        # without the closest rows every row within 2 x min survives: several matches, indices above 2^21 among them
        rows = [r for r in range(len(case.query)) if w_dist[r] >= 5]
        lst, md = m.match_features(case.query[rows], case.train)
        keep = w_dist[rows] <= 2 * int(w_dist[rows].min())
        assert md == int(w_dist[rows].min()) == 5 and keep.sum() >= 5
        np.testing.assert_array_equal(lst["query_idx"], np.nonzero(keep)[0])
        np.testing.assert_array_equal(lst["train_idx"], w_idx[rows][keep])
        np.testing.assert_array_equal(lst["distance"], w_dist[rows][keep].astype(np.float32))
        assert int(lst["train_idx"].max()) >= L.HALF
    finally:
        m.close()


# ---- an arena beyond 2^32 bytes ------------------------------------------------------------------------------------

BIG_ROWS = 2000
BIG_SEED = 900000
BIG_CAP = 67150              # reserved slots: 67150 x 64000 bytes, already beyond 2^32
BIG_FIRST = 67130            # frames appended before the re-pitch: it copies 4.296e9 bytes, across the boundary
BIG_PITCH = 2004             # rows per slot after the re-pitch (lcm_db_reserve with a larger max_desc)
BIG_N = 67140                # frames in the end (all of 2000 rows)


def _big_frame(s):
    return np.random.default_rng(BIG_SEED + s).integers(0, 256, (BIG_ROWS, 32), dtype=np.uint8)


def test_arena_beyond_4_gib(pkg, oracle):
    """67140 frames of 2000 rows in 67150 reserved slots.  At 2000 rows per slot the arena passes 2^32 bytes inside slot
    67108; after 67130 frames lcm_db_reserve(67150, 2004) re-pitches it to 2004 rows per slot — one copy of 4.296e9 bytes
    across the boundary, into an arena that passes 2^32 bytes inside slot 66974 — and ten more frames follow.  Frame s
    comes from seed + s, so reading a wrong slot changes the answer.  Checked at slots 0, the last, the two around
    byte offset 2^32 of the final arena, the two around it in the first arena, the last before and the first after the
    re-pitch, and 20 seeded others: lcm_db_read, lcm_query_scores, lcm_detect_loops (a planted revisit of the first slot
    above 2^32), lcm_all_vs_all / _argmin with an external 4-frame query set (plain and packed), lcm_match_stored across
    the boundary.  Kernel variants 0 and 1 only (the matrix-core image would be 8 times the arena).
    Then, on the same arena, the two-neighbour routes against knnref / ratioref: lcm_query_scores_ratio and
    lcm_detect_loops_ratio on the planted revisit (all 2000 rows pass at 0.7; no other frame reaches 300),
    lcm_all_vs_all_ratio with the revisit as an external query frame at 4 slots on each side of the boundary (and equal to
    the online call's records everywhere), lcm_match_stored_ratio for the pair across the boundary in both orders.
    Peak device memory is the two arenas side by side during the re-pitch, 8.0 GiB, later one arena beside the packed
    route's 1 GiB scratch.  The test skips, with the reason printed, only when torch.cuda.mem_get_info() reports less
    than 12 GiB free; nothing else skips it."""
    import torch
    cp = pkg.capi
    free, _ = torch.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip(f"needs 12 GiB of free device memory for two arenas beyond 4 GiB side by side, {free / 2**30:.1f} GiB free")
    lo0 = (1 << 32) // (BIG_ROWS * 32)                      # first arena: the slot that straddles byte offset 2^32
    lo = (1 << 32) // (BIG_PITCH * 32)                      # final arena: the same; lo + 1 starts above the boundary
    assert lo0 + 1 < BIG_FIRST < BIG_N <= BIG_CAP and BIG_N >= 67110 and lo + 1 < BIG_FIRST
    assert BIG_FIRST * BIG_ROWS * 32 > 1 << 32 and lo * BIG_PITCH * 32 < 1 << 32 < (lo + 1) * BIG_PITCH * 32
    rng = np.random.default_rng(12)
    sample = sorted(set([0, BIG_N - 1, lo, lo + 1, lo0, lo0 + 1, BIG_FIRST - 1, BIG_FIRST] + [int(x) for x in rng.integers(0, BIG_N, 20)]))
    # ratio 1: a good match is a row AT the pair's minimum, so unrelated frames score a handful and only the revisit loops
    m = pkg.Matcher(_params(pkg, ratio=1, min_matches=50))
    p = oracle.default_params(min_gap=GAP, ratio=1, min_matches=50)
    bufs = []
    try:
        m.reserve(BIG_CAP, BIG_ROWS)
        for s in range(BIG_FIRST):
            m.append(s, _big_frame(s))
        for s in (lo0, lo0 + 1, BIG_FIRST - 1):             # beyond 2^32 bytes before anything is re-pitched
            np.testing.assert_array_equal(m.read_frame(s), _big_frame(s), err_msg=f"slot {s} before the re-pitch")
        m.reserve(BIG_CAP, BIG_PITCH)
        for s in range(BIG_FIRST, BIG_N):
            m.append(s, _big_frame(s))
        assert len(m) == BIG_N
        frames = {s: _big_frame(s) for s in sample}
        for s in sample:
            assert m.frame_info(s) == (s, BIG_ROWS, BIG_ROWS)
            np.testing.assert_array_equal(m.read_frame(s), frames[s], err_msg=f"slot {s}")
        # queries: a revisit of slot lo + 1 (300 of its rows with one flipped bit), of slot lo, of the last slot, and a new frame
        rev = frames[lo + 1].copy()
        rev[:300, 0] ^= 1
        queries = [rev, frames[lo].copy(), frames[BIG_N - 1].copy(), _big_frame(BIG_N + 5)]
        rows = np.stack(queries + [frames[s] for s in sample])
        counts = np.full(len(rows), BIG_ROWS, np.int32)
        pq = [q for q in range(4) for _ in sample]
        pt = [4 + k for _ in range(4) for k in range(len(sample))]
        wsc, wsum = oracle.fast_score_pairs_idx(rows, counts, pq, pt, p, n_threads=16)
        wsc, wsum = wsc.reshape(4, len(sample)), wsum.reshape(4, len(sample))
        assert int(wsc[0, sample.index(lo + 1)]["good_count"]) == BIG_ROWS - 300 and int(wsc[0, sample.index(lo)]["good_count"]) < 50
        assert wsc[0, 0] == oracle.pair_score(rev, frames[sample[0]], p)       # the tuned path against the scalar oracle
        q_ids = np.arange(4, dtype=np.int32) + BIG_N + 10
        for variant in (0, 1):
            m.set_kernel_variant(variant)
            sc, ids = m.query_scores(rev, int(q_ids[0]))
            assert len(sc) == BIG_N and np.array_equal(ids, np.arange(BIG_N))
            np.testing.assert_array_equal(sc[sample], wsc[0], err_msg=f"variant {variant}")
            cands = m.detect_loops(int(q_ids[0]), rev)
            assert _tuples(cands) == [(int(q_ids[0]), lo + 1, BIG_ROWS - 300, (BIG_ROWS - 300) / BIG_ROWS)]
        # bulk, external 4-frame query set
        n = 4 * BIG_N
        q_rows = np.stack(queries)
        d, ds = m.dev_alloc(n * 8), m.dev_alloc(n * 4)
        dq, dc = m.dev_alloc(q_rows.nbytes), m.dev_alloc(16)
        bufs += [d, ds, dq, dc]
        m.dev_upload(dq, q_rows); m.dev_upload(dc, counts[:4])
        kw = dict(d_query_rows=dq, d_query_counts=dc, q_ids=q_ids, q_stride_rows=BIG_ROWS)
        got, sums = np.zeros(n, wsc.dtype), np.zeros(n, np.uint32)
        at = np.array([q * BIG_N + s for q in range(4) for s in sample])
        for variant in (0, 1):
            m.set_kernel_variant(variant)
            for packed, route in ((0, cp.ROUTE_PLAIN), (1, cp.ROUTE_PACKED)):
                m.set_tuning(cp.TUNE_PACKED, packed)
                label = f"variant {variant} packed {packed}"
                got[:] = 0
                assert m.all_vs_all(d, n, **kw) == n
                assert m.launch_info().route == route, label
                m.sync(); m.dev_download(d, got)
                np.testing.assert_array_equal(got[at], wsc.reshape(-1), err_msg=label)
                got[:] = 0; sums[:] = 0xDEADBEEF
                m.all_vs_all_argmin(d, n, ds, **kw)
                assert m.launch_info().route == route, label
                m.sync(); m.dev_download(d, got); m.dev_download(ds, sums)
                np.testing.assert_array_equal(got[at], wsc.reshape(-1), err_msg=label)
                np.testing.assert_array_equal(sums[at], wsum.reshape(-1), err_msg=label)
                assert int((got["n_train"] != BIG_ROWS).sum()) == 0
        m.set_tuning(cp.TUNE_PACKED, -1)
        # match lists between slots on both sides of the boundary
        for c, i in ((BIG_N - 1, 0), (lo + 1, lo), (lo, lo + 1), (0, BIG_N - 1)):
            lst, md = m.match_stored(c, i)
            om, omin = oracle.match_features(frames[c], frames[i], p)
            np.testing.assert_array_equal(lst, om.astype(lst.dtype), err_msg=f"{c} x {i}")
            assert md == omin
        # ---- the two-neighbour routes on the same arena (references: knnref / ratioref) ----------------------------------
        m.set_kernel_variant(0)
        near = [lo - 3, lo - 2, lo - 1, lo, lo + 1, lo + 2, lo + 3, lo + 4]      # 4 slots on each side of byte offset 2^32
        for s_ in near:
            frames.setdefault(s_, _big_frame(s_))
        at_r = sorted(set(sample) | set(near))
        want_r = np.zeros(len(at_r), wsc.dtype)
        for k, s_ in enumerate(at_r):
            want_r[k] = ratioref.ratio_counts(rev, frames[s_], 0.7) + (BIG_ROWS,)
        assert int(want_r[at_r.index(lo + 1)]["good_count"]) == BIG_ROWS and int(want_r[at_r.index(lo)]["good_count"]) == 0
        sc, ids = m.query_scores_ratio(rev, int(q_ids[0]), 0.7)                  # 67140 eligible frames: 4 slots per workgroup
        assert len(sc) == BIG_N and np.array_equal(ids, np.arange(BIG_N)) and m.launch_info().workgroups == -(-BIG_N // 4)
        np.testing.assert_array_equal(sc[at_r], want_r)
        assert int((sc["n_train"] != BIG_ROWS).sum()) == 0 and int((sc["good_count"] >= 300).sum()) == 1
        cands = m.detect_loops_ratio(int(q_ids[0]), rev, 0.7, 100, 300)
        assert _tuples(cands) == [(int(q_ids[0]), lo + 1, BIG_ROWS, 1.0)]
        got[:] = 0
        assert m.all_vs_all_ratio(0.7, d, n, d_query_rows=dq, d_query_counts=dc, q_ids=q_ids[:1], q_stride_rows=BIG_ROWS) == BIG_N
        m.sync(); m.dev_download(d, got)
        np.testing.assert_array_equal(got[near], want_r[[at_r.index(s_) for s_ in near]])
        np.testing.assert_array_equal(got[:BIG_N], sc)                         # bulk == online, all 67140 records
        for c, i in ((lo + 1, lo), (lo, lo + 1)):
            ri, rd = knnref.knn2(frames[c], frames[i])
            rows_, tidx, dist = knnref.ratio_filter(ri, rd, 1.0)
            lst = m.match_stored_ratio(c, i, 1.0)
            assert 0 < len(rows_) < BIG_ROWS and not lst["img_idx"].any()
            np.testing.assert_array_equal(lst["query_idx"], rows_)
            np.testing.assert_array_equal(lst["train_idx"], tidx)
            np.testing.assert_array_equal(lst["distance"], dist)
    finally:
        for b in bufs:
            m.dev_free(b)
        m.close()
