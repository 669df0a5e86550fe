"""lcm_group_all_vs_all_ratio / lcm_group_all_vs_all_loops_ratio: the ratio-test scored searches over W shards equal a single
handle holding all frames and tests/ratioloopref.py.  W = 1 is a real group of one device, W > 1 a loopback group on the
box's one GPU (as tests/test_gpu_group.py builds them).  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

import ratioloopref as R

pytestmark = pytest.mark.gpu

WORLDS = (1, 2, 3, 4)


def group_kw(world):
    return dict(n_devices=1) if world == 1 else dict(n_devices=world, loopback_device=0)


def as_cands(pkg, want):
    a = np.zeros(len(want), pkg.capi.CANDIDATE_DTYPE)
    for k, (cur, matched, good, sim) in enumerate(want):
        a[k] = (cur, matched, good, 0, sim)
    return a


def single_scores(m, pkg, ratio):
    n, offs = m.all_vs_all_ratio_plan(ratio)
    got = np.zeros(n, pkg.capi.SCORE_DTYPE)
    d = m.dev_alloc(max(n, 1) * 8)
    if n:
        m.all_vs_all_ratio(ratio, d, n)
        m.sync()
        m.dev_download(d, got)
    m.dev_free(d)
    return got, offs


@pytest.fixture(scope="module")
def sets():
    """the 11-frame database (0..160 rows, one frame empty), the same + 2 appended frames, and their references"""
    base = R.planted_frames(903, R.GROUP_SPEC)
    more = R.planted_frames(903, R.GROUP_EXTRA_SPEC)
    return base, R.Ref(base), more, R.Ref(more)


@pytest.fixture(scope="module")
def single(pkg, sets):
    """what ONE handle holding the 11 frames returns, per min_gap: (records, offsets, candidates)"""
    base = sets[0]
    out = {}
    with pkg.Matcher() as m:
        for fid, rows in base:
            m.append(fid, rows)
        for gap in (1, 3):
            m.set_params(min_gap=gap)
            recs, offs = single_scores(m, pkg, 0.7)
            cands, _ = m.all_vs_all_loops_ratio(*R.GROUP_RP)
            out[gap] = (recs, offs, cands.copy())
    return out


@pytest.mark.parametrize("world", WORLDS)
def test_scores_and_loops_across_shard_counts(pkg, sets, single, world):
    base, ref = sets[0], sets[1]
    p = pkg.default_params()
    with pkg.Group(p, **group_kw(world)) as g:
        for fid, rows in base:
            g.append(fid, rows)
        for gap in (1, 3):
            p.min_gap = gap
            g.set_params(p)
            recs, offs, cands = single[gap]
            got, goffs = g.all_vs_all_ratio(0.7)
            assert got.tobytes() == recs.tobytes() and goffs.tolist() == offs.tolist(), (world, gap)
            gi = g.info()
            assert gi.n_devices == world and gi.pairs == len(recs) and gi.kernel_ms_max > 0
            assert gi.loopback == (0 if world == 1 else 1)
            assert sum(gi.shard_pairs[r] for r in range(world)) == len(recs)
            gc, n_pairs = g.all_vs_all_loops_ratio(*R.GROUP_RP)
            want = as_cands(pkg, ref.expected(gap, *R.GROUP_RP))
            assert n_pairs == len(recs) and len(want) > 0
            assert gc.tobytes() == cands.tobytes() == want.tobytes(), (world, gap)
            assert g.info().pairs == len(recs)
        if world == 1:
            # the group's own handle, called directly: byte for byte the same
            h = C.c_void_p()
            assert g._lib.lcm_group_handle(g._g, 0, C.byref(h)) == 0
            m = pkg.Matcher.__new__(pkg.Matcher)
            m._lib, m._h = g._lib, h
            try:
                recs, offs, cands = single[3]
                own, ooffs = single_scores(m, pkg, 0.7)
                assert own.tobytes() == recs.tobytes() and ooffs.tolist() == offs.tolist()
                oc, _ = m.all_vs_all_loops_ratio(*R.GROUP_RP)
                assert oc.tobytes() == cands.tobytes()
            finally:
                m._h = None                      # borrowed: the group destroys it


@pytest.mark.parametrize("world", (1, 3))
def test_capacity_reports_the_group_wide_count(pkg, sets, world):
    base, ref = sets[0], sets[1]
    p = pkg.default_params()
    p.min_gap = 1
    want = ref.expected(1, *R.GROUP_RP)
    count = len(want)
    rp = pkg.capi.RatioLoopParams(*R.GROUP_RP)
    with pkg.Group(p, **group_kw(world)) as g:
        for fid, rows in base:
            g.append(fid, rows)
        buf = np.zeros(count + 2, pkg.capi.CANDIDATE_DTYPE)
        raw = buf.view(np.uint8)
        raw[:] = 0xAB
        n, npairs = C.c_size_t(0), C.c_size_t(0)

        def call(out, cap):
            return g._lib.lcm_group_all_vs_all_loops_ratio(g._g, C.byref(rp), out, cap, C.byref(n), C.byref(npairs))

        assert count >= 2 * world
        assert call(buf.ctypes.data_as(C.c_void_p), count - 1) == pkg.capi.ERR_CAPACITY
        assert n.value == count and npairs.value == 55 and (raw == 0xAB).all()
        assert call(None, 0) == pkg.capi.ERR_CAPACITY and n.value == count
        assert call(buf.ctypes.data_as(C.c_void_p), count) == 0 and n.value == count
        assert buf[:count].tobytes() == as_cands(pkg, want).tobytes() and (raw[count * 24:] == 0xAB).all()
        # what the single-handle calls refuse, the group refuses
        for bad in (float("nan"), -0.5):
            with pytest.raises(pkg.LcmError) as e:
                g.all_vs_all_ratio(bad)
            assert e.value.code == pkg.capi.ERR_INVALID_ARG
        for kw in (dict(ratio=float("nan")), dict(min_rows=-1), dict(min_matches=-1)):
            with pytest.raises(pkg.LcmError) as e:
                g.all_vs_all_loops_ratio(**kw)
            assert e.value.code == pkg.capi.ERR_INVALID_ARG
        p.cross_check = 1
        g.set_params(p)
        for fn in (lambda: g.all_vs_all_ratio(0.7), lambda: g.all_vs_all_loops_ratio()):
            with pytest.raises(pkg.LcmError) as e:
                fn()
            assert e.value.code == pkg.capi.ERR_INVALID_ARG


@pytest.mark.parametrize("world", (2, 3))
def test_append_gather_and_alternation(pkg, sets, single, world):
    base, ref, more, mref = sets
    p = pkg.default_params()
    p.min_gap = 1
    p.min_matches = 5
    p.sim_threshold = 0.05
    with pkg.Group(p, **group_kw(world)) as g:
        for fid, rows in base:
            g.append(fid, rows)
        plain, _ = g.all_vs_all()
        loops, _ = g.all_vs_all_loops(cap=64)
        plain, loops = plain.copy(), loops.copy()
        assert g.info().arena_gather_skipped == 1           # nothing appended since g.all_vs_all()
        got, _ = g.all_vs_all_ratio(0.7)
        assert g.info().arena_gather_skipped == 1
        assert got.tobytes() == single[1][0].tobytes()
        gc, _ = g.all_vs_all_loops_ratio(*R.GROUP_RP)
        assert gc.tobytes() == single[1][2].tobytes()
        # the existing searches are unchanged by the ratio ones in between
        assert g.all_vs_all()[0].tobytes() == plain.tobytes()
        assert g.all_vs_all_loops(cap=64)[0].tobytes() == loops.tobytes() and len(loops) > 0
        # append two frames: results follow the database, the arenas are gathered again once
        for fid, rows in more[len(base):]:
            g.append(fid, rows)
        gc, n_pairs = g.all_vs_all_loops_ratio(*R.GROUP_RP)
        assert g.info().arena_gather_skipped == 0
        want = as_cands(pkg, mref.expected(1, *R.GROUP_RP))
        assert n_pairs == 78 and len(want) > len(single[1][2])
        assert gc.tobytes() == want.tobytes()
        again, _ = g.all_vs_all_loops_ratio(*R.GROUP_RP)
        assert g.info().arena_gather_skipped == 1 and again.tobytes() == gc.tobytes()
        got, offs = g.all_vs_all_ratio(0.7)
        assert g.info().arena_gather_skipped == 1 and len(got) == 78
        assert got[:55].tobytes() == single[1][0].tobytes()
        for k, (c, s) in enumerate(mref.pairs(1)):
            if c >= len(base):
                assert int(got[k]["good_count"]) == mref.count(c, s, 0.7) and int(got[k]["n_train"]) == len(more[s][1])
