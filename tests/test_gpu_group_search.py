"""The group's bulk search after its split into stages (csrc/lcm_group_search.cpp): the join every mode leaves through,
and lcm_group_last_info after each of the five modes.  Loopback groups on one device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = ("scores", "argmin", "loops", "ratio", "loops_ratio")
RATIO = dict(ratio=0.7, min_rows=1, min_matches=4)


def _params(pkg, gap):
    p = pkg.default_params()
    p.min_gap = gap
    p.min_matches = 2
    p.sim_threshold = 0.1
    return p


def _search(t, mode, cap):
    """(candidates, pairs) of one fused loop search on a Matcher or a Group"""
    return t.all_vs_all_loops(cap=cap) if mode == "loops" else t.all_vs_all_loops_ratio(cap=cap, **RATIO)


@pytest.mark.parametrize("world", [3, 8])
@pytest.mark.parametrize("mode", ["loops", "loops_ratio"])
def test_loops_search_joins_every_shard_before_appends_move_the_arenas(pkg, mode, world):
    """32 frames of 8 rows with min_gap = 30 make 3 pairs, owned by shards 0 and 1: every other shard enqueues its copies of the
    arena exchange and owns nothing to wait for.  The search must still have joined them when it returns, because the appends
    that follow — 40-row frames, so every shard's arena is re-pitched, and enough of them that shard 0 outgrows its 64 reserved
    slots — free the arenas those copies read.  Candidates and pair counts equal a single handle's before and after.
    On one device this pins the RESULTS only: a loopback group's hipFree waits for the device, so the race the join closes
    (a peer copy reading another device's freed arena) needs two devices and is not reproduced here."""
    rng = np.random.default_rng(world * 10 + len(mode))
    first = [rng.integers(0, 256, (8, 32), dtype=np.uint8) for _ in range(32)]
    first[30], first[31] = first[0].copy(), first[1].copy()             # the loops of the first search
    with pkg.Group(_params(pkg, 30), n_devices=world, loopback_device=0) as g, pkg.Matcher(_params(pkg, 30)) as m:
        g.reserve(32, 8)
        for i, f in enumerate(first):
            g.append(i, f); m.append(i, f)
        want, want_pairs = _search(m, mode, 16)
        got, got_pairs = _search(g, mode, 16)
        assert got_pairs == want_pairs == 3
        np.testing.assert_array_equal(got, want)
        found = [(c["current_frame_id"], c["matched_frame_id"]) for c in got]
        assert (30, 0) in found and (31, 1) in found            # the two copies; random rows never pass the ratio test 4 times
        assert mode == "loops" or len(found) == 2
        info = g.info()
        assert [info.shard_pairs[r] for r in range(2)] == [2, 1] and info.arena_gather_skipped == 0
        # every shard gets wider frames, shard 0 more than its 64 slots
        n_more = 64 * world + 1 - 32
        for j in range(n_more):
            f = rng.integers(0, 256, (40, 32), dtype=np.uint8)
            if j % 5 == 0:
                f[:8] = first[j % 32]
            g.append(32 + j, f); m.append(32 + j, f)
        n = 32 + n_more
        cap = pkg.synth.n_pairs_all_vs_all(n, 30) + 1
        want, want_pairs = _search(m, mode, cap)
        got, got_pairs = _search(g, mode, cap)
        assert got_pairs == want_pairs == cap - 1
        assert len(want) >= 2
        np.testing.assert_array_equal(got, want)
        assert g.info().arena_gather_skipped == 0


def _run(g, mode, cap):
    if mode == "scores":
        return g.all_vs_all()[0]
    if mode == "argmin":
        return g.all_vs_all_argmin()[0]
    if mode == "ratio":
        return g.all_vs_all_ratio(0.7)[0]
    return _search(g, mode, cap)[0]


@pytest.mark.parametrize("mode", MODES)
def test_last_info_after_each_mode_on_three_shards(pkg, mode):
    """20 ragged frames of at most 40 rows on 3 shards, min_gap = 2: 171 pairs.  After the first search of a mode the info
    reports the pairs, the shards' shares (counted here position by position), the arena exchange (7 slots x 40 rows x 32 bytes
    from each of 3 shards) and the records that travelled to the first shard (8 bytes each, 12 with index checksums, none
    in the loops forms); after the second the exchange was skipped."""
    world, n, gap = 3, 20, 2
    fs = pkg.synth.make_frames(n, 40, seed=77, ragged=True, dup_frac=0.3)
    share = [sum(1 for c in range(n) for s in range(n) if c - s >= gap and s % world == r) for r in range(world)]
    total = sum(share)
    assert total == pkg.synth.n_pairs_all_vs_all(n, gap) == 171
    rec_bytes = {"scores": 8, "argmin": 12, "ratio": 8, "loops": 0, "loops_ratio": 0}[mode]
    with pkg.Group(_params(pkg, gap), n_devices=world, loopback_device=0) as g:
        g.reserve(n, 40)
        for f in range(n):
            g.append(int(fs.ids[f]), fs.frame(f))
        for call in range(2):
            _run(g, mode, total + 1)
            info = g.info()
            assert info.n_devices == world and info.loopback == 1 and info.pairs == total
            assert [info.shard_pairs[r] for r in range(world)] == share
            assert info.arena_gather_skipped == call
            assert info.gathered_query_bytes == (0 if call else 7 * 40 * 32 * world)
            assert info.gathered_score_bytes == (total - share[0]) * rec_bytes
