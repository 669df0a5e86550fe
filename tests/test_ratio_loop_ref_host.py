"""The ratio-scored loop test without a GPU: lcm_ratio_loop_test (host-only C function) against tests/ratioloopref.py, the
structure and its defaults, the exported symbols, and — on the reference alone — that the frame sets the GPU tests use
exercise every condition of the rule (src/main.cpp:1379-1388)."""
import ctypes
import os
import re

import numpy as np
import pytest

import ratioloopref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lcm_ratio_loop_params_default", "lcm_ratio_loop_test", "lcm_all_vs_all_loops_ratio", "lcm_detect_loops_ratio",
               "lcm_group_all_vs_all_ratio", "lcm_group_all_vs_all_loops_ratio")


def test_struct_and_defaults(pkg):
    c = pkg.capi
    assert ctypes.sizeof(c.RatioLoopParams) == 16 and c.RatioLoopParams.min_rows.offset == 8
    p = c.default_ratio_loop_params()
    assert (p.ratio, p.min_rows, p.min_matches) == R.DEFAULTS == (0.7, 100, 300)


def test_library_exports_and_header_declares_the_new_symbols(pkg):
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lcm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(rf"LCM_API\s+\w+\s+{name}\s*\(", header), name
        assert name in pkg.capi._SIGNATURES


@pytest.mark.parametrize("rp", [R.DEFAULTS, (0.7, 0, 0)])
def test_host_verdict_equals_the_helper_over_a_grid(pkg, rp):
    ratio, min_rows, min_matches = rp
    goods = sorted({0, max(min_matches - 1, 0), min_matches, min_matches + 1, 2000})
    rows = sorted({0, max(min_rows - 1, 0), min_rows, 2000})
    lib = pkg.load_library()
    p = pkg.capi.RatioLoopParams(ratio, min_rows, min_matches)
    seen = set()
    for good in goods:
        for rc in rows:
            for rs in rows:
                s = pkg.capi.Score(good, 3, rs)
                sim = ctypes.c_double(-1.0)
                got = lib.lcm_ratio_loop_test(ctypes.byref(p), ctypes.byref(s), rc, ctypes.byref(sim))
                want = all(R.verdict(good, rc, rs, min_rows, min_matches))
                assert got == int(want), (rp, good, rc, rs)
                assert np.float64(sim.value).tobytes() == np.float64(R.similarity(good, rc, rs)).tobytes(), (rp, good, rc, rs)
                # the Python wrapper, and rp == NULL for the defaults
                rec = np.zeros(1, pkg.capi.SCORE_DTYPE)
                rec[0] = (good, 3, rs)
                assert pkg.capi.ratio_loop_test(rec[0], rc, ratio, min_rows, min_matches) == (want, sim.value)
                if rp == R.DEFAULTS:
                    assert lib.lcm_ratio_loop_test(None, ctypes.byref(s), rc, None) == int(want)
                seen.add(want)
    assert seen == ({True, False} if rp == R.DEFAULTS else {True})      # thresholds of 0 reject nothing
    assert lib.lcm_ratio_loop_test(ctypes.byref(p), None, 100, None) == 0


def _assert_exercises(ref, gap, rp, spec=None, rows_c_possible=True, msg=""):
    """accepted pairs, pairs rejected ONLY by rows_c / ONLY by rows_s / ONLY by the count, one pair at
    good_count == min_matches and one at min_matches - 1 (both with enough rows on either side)"""
    ratio, min_rows, min_matches = rp
    cls = ref.classes(gap, ratio, min_rows, min_matches)
    kinds = {k for k, _ in cls}
    assert (True, True, True) in kinds, msg
    assert (True, False, True) in kinds and (True, True, False) in kinds, msg
    assert ((False, True, True) in kinds) == rows_c_possible, msg
    assert any(k[:2] == (True, True) and g == min_matches for k, g in cls), msg
    assert any(k[:2] == (True, True) and g == min_matches - 1 for k, g in cls), msg
    if spec is not None:                 # the planting gives the counts it is meant to give
        for c, s in ref.pairs(gap):
            assert ref.count(c, s, ratio) == R.planted_count(spec, c, s), (msg, c, s)


def test_boundary_set_exercises_every_condition():
    ref = R.Ref(R.planted_frames(900, R.BOUNDARY_SPEC))
    _assert_exercises(ref, 1, R.BOUNDARY_RP, R.BOUNDARY_SPEC, msg="boundary")
    rows = {n for n, _ in R.BOUNDARY_SPEC}
    assert {39, 40, 41} <= rows and {11, 12, 13} <= {k for _, k in R.BOUNDARY_SPEC}


def test_default_set_exercises_every_condition():
    """Under 100 / 300 a pair cannot be rejected by rows_c alone: good_count <= rows_c < 100 < 300."""
    frames = R.default_frames()
    ref = R.Ref(frames)
    _assert_exercises(ref, 1, R.DEFAULTS, rows_c_possible=False, msg="defaults")
    assert [len(r) for _, r in frames] == [330, 330, 330, 120, 330, 101, 99, 330]
    assert ref.count(1, 0, 0.7) == 300 and ref.count(2, 0, 0.7) == 299 and ref.count(2, 1, 0.7) == 299
    assert ref.count(7, 6, 0.7) == 300          # the 99-row frame would pass on its count
    got = ref.expected(1, *R.DEFAULTS)
    assert [(c, m, g) for c, m, g, _ in got] == [(1, 0, 300), (4, 0, 300), (4, 1, 300)]


@pytest.mark.parametrize("gap", [1, 3])
def test_group_set_exercises_every_condition(gap):
    ref = R.Ref(R.planted_frames(903, R.GROUP_EXTRA_SPEC))
    base = R.Ref(R.planted_frames(903, R.GROUP_SPEC))
    _assert_exercises(base, gap, R.GROUP_RP, R.GROUP_SPEC, msg=f"group gap {gap}")
    _assert_exercises(ref, gap, R.GROUP_RP, R.GROUP_EXTRA_SPEC, msg=f"group + 2 gap {gap}")
    assert sorted(n for n, _ in R.GROUP_SPEC)[0] == 0 and max(n for n, _ in R.GROUP_SPEC) == 160
    # the first 11 frames are the same rows in both (the appended frames only add pairs)
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(base.frames, ref.frames))


@pytest.mark.parametrize("n_pairs", sorted(R.TINY_SHAPES))
def test_tiny_sets_select(n_pairs):
    """min_rows = 0 cannot reject, so the compaction sets are checked per parameter set: (1.0, 0, 0) accepts every pair,
    (1.0, 0, 1) a proper subset by count, (1.0, 3, 1) also rejects by rows on either side."""
    nq, ns = R.TINY_SHAPES[n_pairs]
    stored, queries = R.tiny_set(910 + n_pairs, nq, ns)
    ref = R.Ref(stored, queries)
    assert len(ref.pairs(1)) == n_pairs == nq * ns
    assert all(1 <= len(r) <= 4 for _, r in stored + queries)
    everything = ref.expected(1, 1.0, 0, 0)
    assert len(everything) == n_pairs
    subset = ref.expected(1, 1.0, 0, 1)
    assert 0 < len(subset) < n_pairs
    kinds = {k for k, _ in ref.classes(1, 1.0, 3, 1)}
    assert (True, True, True) in kinds and (True, True, False) in kinds and (True, False, True) in kinds
    if nq > 1:
        assert (False, True, True) in kinds
    for lst in (everything, subset):
        assert [(c, m) for c, m, _, _ in lst] == sorted((c, m) for c, m, _, _ in lst)
