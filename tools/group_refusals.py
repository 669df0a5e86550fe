"""Prints what every lcm_group_* bulk and online entry point, and the two merge functions, answer to a faulty call: one line
`call | fault | code | message` per case.  Run it once per library (LCM_LIB_PATH selects one) and compare the outputs: a
change to the group's host side must leave the table as it is.  Needs a device (group creation); W = 3 loopback shards.

    python tools/group_refusals.py > table.txt
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
capi = pkg.capi
lib = pkg.load_library()
VP = C.c_void_p
ROWS = []


def case(call, fault, rc):
    msg = lib.lcm_last_error().decode("utf-8", "replace") if rc else ""
    ROWS.append(f"{call} | {fault} | {rc} | {msg}")


def vp(a):
    return a.ctypes.data_as(VP)


def i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def new_group(params, frames):
    g = VP()
    assert lib.lcm_group_create_loopback(C.byref(params), 3, 0, C.byref(g)) == 0
    for i, f in enumerate(frames):
        assert lib.lcm_group_append(g, i, vp(f), f.shape[0], -1) == 0
    return g


def bulk(g, n_frames):
    sz, sz2 = C.c_size_t(0), C.c_size_t(0)
    total = pkg.synth.n_pairs_all_vs_all(n_frames, 2)
    sc = np.zeros(total, capi.SCORE_DTYPE)
    ix = np.zeros(total, np.uint32)
    cands = np.zeros(total, capi.CANDIDATE_DTYPE)
    rp = capi.default_ratio_loop_params()
    rp.min_rows, rp.min_matches = 1, 1
    nan_rp, neg_rp = capi.default_ratio_loop_params(), capi.default_ratio_loop_params()
    nan_rp.ratio, neg_rp.ratio = float("nan"), -0.5
    # records forms
    case("lcm_group_all_vs_all", "NULL group", lib.lcm_group_all_vs_all(None, vp(sc), total, C.byref(sz), None))
    case("lcm_group_all_vs_all", "NULL n_pairs", lib.lcm_group_all_vs_all(g, vp(sc), total, None, None))
    case("lcm_group_all_vs_all", "cap one below the pairs", lib.lcm_group_all_vs_all(g, vp(sc), total - 1, C.byref(sz), None))
    case("lcm_group_all_vs_all_argmin", "NULL group", lib.lcm_group_all_vs_all_argmin(None, vp(sc), vp(ix), total, C.byref(sz), None))
    case("lcm_group_all_vs_all_argmin", "NULL n_pairs", lib.lcm_group_all_vs_all_argmin(g, vp(sc), vp(ix), total, None, None))
    case("lcm_group_all_vs_all_argmin", "out_scores without out_index_sums", lib.lcm_group_all_vs_all_argmin(g, vp(sc), None, total, C.byref(sz), None))
    case("lcm_group_all_vs_all_argmin", "cap one below the pairs", lib.lcm_group_all_vs_all_argmin(g, vp(sc), vp(ix), total - 1, C.byref(sz), None))
    case("lcm_group_all_vs_all_ratio", "NULL group", lib.lcm_group_all_vs_all_ratio(None, 0.7, vp(sc), total, C.byref(sz), None))
    case("lcm_group_all_vs_all_ratio", "NULL n_pairs", lib.lcm_group_all_vs_all_ratio(g, 0.7, vp(sc), total, None, None))
    case("lcm_group_all_vs_all_ratio", "NaN ratio", lib.lcm_group_all_vs_all_ratio(g, float("nan"), vp(sc), total, C.byref(sz), None))
    case("lcm_group_all_vs_all_ratio", "negative ratio", lib.lcm_group_all_vs_all_ratio(g, -0.5, vp(sc), total, C.byref(sz), None))
    case("lcm_group_all_vs_all_ratio", "cap one below the pairs", lib.lcm_group_all_vs_all_ratio(g, 0.7, vp(sc), total - 1, C.byref(sz), None))
    # loops forms: the candidate count first
    assert lib.lcm_group_all_vs_all_loops(g, vp(cands), total, C.byref(sz), C.byref(sz2)) == 0
    found = max(sz.value, 1)
    case("lcm_group_all_vs_all_loops", "NULL group", lib.lcm_group_all_vs_all_loops(None, vp(cands), total, C.byref(sz), C.byref(sz2)))
    case("lcm_group_all_vs_all_loops", "NULL n_out", lib.lcm_group_all_vs_all_loops(g, vp(cands), total, None, C.byref(sz2)))
    case("lcm_group_all_vs_all_loops", "cap one below the candidates", lib.lcm_group_all_vs_all_loops(g, vp(cands), found - 1, C.byref(sz), C.byref(sz2)))
    case("lcm_group_all_vs_all_loops", "cap 1", lib.lcm_group_all_vs_all_loops(g, vp(cands), 1, C.byref(sz), C.byref(sz2)))
    case("lcm_group_all_vs_all_loops", "NULL out with candidates", lib.lcm_group_all_vs_all_loops(g, None, 0, C.byref(sz), C.byref(sz2)))
    assert lib.lcm_group_all_vs_all_loops_ratio(g, C.byref(rp), vp(cands), total, C.byref(sz), C.byref(sz2)) == 0
    found = max(sz.value, 1)
    case("lcm_group_all_vs_all_loops_ratio", "NULL group", lib.lcm_group_all_vs_all_loops_ratio(None, C.byref(rp), vp(cands), total, C.byref(sz), C.byref(sz2)))
    case("lcm_group_all_vs_all_loops_ratio", "NULL n_out", lib.lcm_group_all_vs_all_loops_ratio(g, C.byref(rp), vp(cands), total, None, C.byref(sz2)))
    case("lcm_group_all_vs_all_loops_ratio", "NaN ratio", lib.lcm_group_all_vs_all_loops_ratio(g, C.byref(nan_rp), vp(cands), total, C.byref(sz), C.byref(sz2)))
    case("lcm_group_all_vs_all_loops_ratio", "negative ratio", lib.lcm_group_all_vs_all_loops_ratio(g, C.byref(neg_rp), vp(cands), total, C.byref(sz), C.byref(sz2)))
    case("lcm_group_all_vs_all_loops_ratio", "cap one below the candidates",
         lib.lcm_group_all_vs_all_loops_ratio(g, C.byref(rp), vp(cands), found - 1, C.byref(sz), C.byref(sz2)))
    case("lcm_group_all_vs_all_loops_ratio", "NULL out with candidates", lib.lcm_group_all_vs_all_loops_ratio(g, C.byref(rp), None, 0, C.byref(sz), C.byref(sz2)))
    case("lcm_group_last_info", "NULL group", lib.lcm_group_last_info(None, C.byref(capi.GroupInfo())))
    case("lcm_group_last_info", "NULL info", lib.lcm_group_last_info(g, None))


def cross_check(frames):
    p = pkg.default_params()
    p.min_gap, p.cross_check = 2, 1
    g = new_group(p, frames)
    sz, sz2 = C.c_size_t(0), C.c_size_t(0)
    sc = np.zeros(1024, capi.SCORE_DTYPE)
    cands = np.zeros(1024, capi.CANDIDATE_DTYPE)
    case("lcm_group_all_vs_all_ratio", "cross_check = 1", lib.lcm_group_all_vs_all_ratio(g, 0.7, vp(sc), 1024, C.byref(sz), None))
    case("lcm_group_all_vs_all_loops_ratio", "cross_check = 1", lib.lcm_group_all_vs_all_loops_ratio(g, None, vp(cands), 1024, C.byref(sz), C.byref(sz2)))
    lib.lcm_group_destroy(g)


def online(g, frames):
    n_frames = len(frames)
    q = frames[3]
    qid = n_frames + 5
    e = n_frames                                     # every stored frame is eligible for an id beyond the last
    sc = np.zeros(16 * e, capi.SCORE_DTYPE)
    ids = np.zeros(e, np.int32)
    n = C.c_int32(0)
    sz = C.c_size_t(0)
    cands = np.zeros(e, capi.CANDIDATE_DTYPE)
    case("lcm_group_query_scores", "NULL group", lib.lcm_group_query_scores(None, vp(q), q.shape[0], qid, vp(sc), vp(ids), e, C.byref(n)))
    case("lcm_group_query_scores", "NULL n_out", lib.lcm_group_query_scores(g, vp(q), q.shape[0], qid, vp(sc), vp(ids), e, None))
    case("lcm_group_query_scores", "NULL query with rows", lib.lcm_group_query_scores(g, None, 5, qid, vp(sc), vp(ids), e, C.byref(n)))
    case("lcm_group_query_scores", "negative rows", lib.lcm_group_query_scores(g, vp(q), -1, qid, vp(sc), vp(ids), e, C.byref(n)))
    case("lcm_group_query_scores", "cap one below the records", lib.lcm_group_query_scores(g, vp(q), q.shape[0], qid, vp(sc), vp(ids), e - 1, C.byref(n)))
    case("lcm_group_query_scores", "NULL out_scores", lib.lcm_group_query_scores(g, vp(q), q.shape[0], qid, None, vp(ids), e, C.byref(n)))
    assert lib.lcm_group_detect_loops(g, qid, vp(q), q.shape[0], -1, vp(cands), e, C.byref(n)) == 0
    found = max(n.value, 1)
    case("lcm_group_detect_loops", "NULL group", lib.lcm_group_detect_loops(None, qid, vp(q), q.shape[0], -1, vp(cands), e, C.byref(n)))
    case("lcm_group_detect_loops", "NULL n_out", lib.lcm_group_detect_loops(g, qid, vp(q), q.shape[0], -1, vp(cands), e, None))
    case("lcm_group_detect_loops", "negative cap", lib.lcm_group_detect_loops(g, qid, vp(q), q.shape[0], -1, vp(cands), -1, C.byref(n)))
    case("lcm_group_detect_loops", "cap one below the candidates", lib.lcm_group_detect_loops(g, qid, vp(q), q.shape[0], -1, vp(cands), found - 1, C.byref(n)))
    # micro-batches of two queries
    B = 2
    ptrs = (VP * 17)(*[q.ctypes.data] * 17)
    nq = np.full(17, q.shape[0], np.int32)
    qids = np.arange(qid, qid + 17, dtype=np.int32)
    offs = np.zeros(18, np.uintp)
    t = C.c_int32(-1)
    batch = lib.lcm_group_query_scores_batch
    case("lcm_group_query_scores_batch", "NULL group", batch(None, ptrs, i32(nq), i32(qids), B, vp(sc), len(sc), C.byref(sz), vp(offs)))
    case("lcm_group_query_scores_batch", "NULL n_out", batch(g, ptrs, i32(nq), i32(qids), B, vp(sc), len(sc), None, vp(offs)))
    case("lcm_group_query_scores_batch", "NULL queries", batch(g, None, i32(nq), i32(qids), B, vp(sc), len(sc), C.byref(sz), vp(offs)))
    case("lcm_group_query_scores_batch", "NULL nq", batch(g, ptrs, None, i32(qids), B, vp(sc), len(sc), C.byref(sz), vp(offs)))
    case("lcm_group_query_scores_batch", "NULL ids", batch(g, ptrs, i32(nq), None, B, vp(sc), len(sc), C.byref(sz), vp(offs)))
    case("lcm_group_query_scores_batch", "no queries", batch(g, ptrs, i32(nq), i32(qids), 0, vp(sc), len(sc), C.byref(sz), vp(offs)))
    offs[:] = 7
    case("lcm_group_query_scores_batch", "17 queries", batch(g, ptrs, i32(nq), i32(qids), 17, vp(sc), len(sc), C.byref(sz), vp(offs)))
    ROWS.append(f"lcm_group_query_scores_batch | 17 queries: offsets left behind | - | {' '.join(str(int(o)) for o in offs)}")
    case("lcm_group_query_scores_batch", "cap one below the records", batch(g, ptrs, i32(nq), i32(qids), B, vp(sc), B * e - 1, C.byref(sz), vp(offs)))
    case("lcm_group_query_scores_batch", "NULL out_scores", batch(g, ptrs, i32(nq), i32(qids), B, None, len(sc), C.byref(sz), vp(offs)))
    submit, collect = lib.lcm_group_query_submit_batch, lib.lcm_group_query_collect_batch
    case("lcm_group_query_submit_batch", "NULL group", submit(None, ptrs, i32(nq), i32(qids), B, C.byref(t)))
    case("lcm_group_query_submit_batch", "NULL ticket", submit(g, ptrs, i32(nq), i32(qids), B, None))
    case("lcm_group_query_submit_batch", "NULL queries", submit(g, None, i32(nq), i32(qids), B, C.byref(t)))
    case("lcm_group_query_submit_batch", "no queries", submit(g, ptrs, i32(nq), i32(qids), 0, C.byref(t)))
    case("lcm_group_query_submit_batch", "17 queries", submit(g, ptrs, i32(nq), i32(qids), 17, C.byref(t)))
    case("lcm_group_query_collect_batch", "NULL group", collect(None, 0, vp(sc), len(sc), C.byref(sz), vp(offs)))
    case("lcm_group_query_collect_batch", "ticket -1", collect(g, -1, vp(sc), len(sc), C.byref(sz), vp(offs)))
    case("lcm_group_query_collect_batch", "ticket 4", collect(g, 4, vp(sc), len(sc), C.byref(sz), vp(offs)))
    case("lcm_group_query_collect_batch", "ticket never issued", collect(g, 2, vp(sc), len(sc), C.byref(sz), vp(offs)))
    tickets = []
    for k in range(4):
        assert submit(g, ptrs, i32(nq), i32(qids), B, C.byref(t)) == 0
        tickets.append(t.value)
    case("lcm_group_query_submit_batch", "a fifth ticket", submit(g, ptrs, i32(nq), i32(qids), B, C.byref(t)))
    case("lcm_group_query_collect_batch", "NULL n_out", collect(g, tickets[0], vp(sc), len(sc), None, vp(offs)))
    case("lcm_group_query_collect_batch", "cap one below the records", collect(g, tickets[0], vp(sc), B * e - 1, C.byref(sz), vp(offs)))
    case("lcm_group_query_collect_batch", "NULL out_scores", collect(g, tickets[0], None, len(sc), C.byref(sz), vp(offs)))
    case("lcm_group_query_collect_batch", "the ticket after both refusals", collect(g, tickets[0], vp(sc), len(sc), C.byref(sz), vp(offs)))
    case("lcm_group_query_collect_batch", "the same ticket again", collect(g, tickets[0], vp(sc), len(sc), C.byref(sz), vp(offs)))
    assert lib.lcm_group_truncate(g, n_frames - 1) == 0
    case("lcm_group_query_collect_batch", "ticket from before a truncate", collect(g, tickets[1], vp(sc), len(sc), C.byref(sz), vp(offs)))
    case("lcm_group_query_collect_batch", "void ticket, cap 0 and NULL out_scores", collect(g, tickets[2], None, 0, C.byref(sz), vp(offs)))
    assert submit(g, ptrs, i32(nq), i32(qids), B, C.byref(t)) == 0
    assert lib.lcm_group_clear(g) == 0
    case("lcm_group_query_collect_batch", "ticket from before a clear", collect(g, t.value, vp(sc), len(sc), C.byref(sz), vp(offs)))
    case("lcm_group_query_collect_batch", "older ticket from before the clear", collect(g, tickets[3], vp(sc), len(sc), C.byref(sz), vp(offs)))
    case("lcm_group_truncate", "negative count", lib.lcm_group_truncate(g, -1))
    case("lcm_group_truncate", "NULL group", lib.lcm_group_truncate(None, 1))
    assert lib.lcm_group_append(g, 10, vp(q), q.shape[0], -1) == 0
    case("lcm_group_append", "id not above the last", lib.lcm_group_append(g, 10, vp(q), q.shape[0], -1))


def merges():
    ids = np.arange(20, dtype=np.int32)
    gap, world = 2, 3
    e = pkg.sharding.eligible_counts(ids, gap)
    counts = np.array([sum(len(range(r, int(x), world)) for x in e) for r in range(world)], np.uintp)
    total = int(e.sum())
    shards = [np.zeros(int(c), capi.SCORE_DTYPE) for c in counts]
    ptrs = (VP * world)(*[s.ctypes.data for s in shards])
    out = np.zeros(total, capi.SCORE_DTYPE)
    offs = np.zeros(21, np.uintp)
    n = C.c_size_t(0)
    short = counts.copy(); short[1] -= 1
    back = ids[::-1].copy()
    host = lib.lcm_merge_shard_scores
    case("lcm_merge_shard_scores", "world 0", host(ptrs, vp(counts), 0, vp(ids), 20, gap, vp(out), total, C.byref(n), vp(offs)))
    case("lcm_merge_shard_scores", "negative frames", host(ptrs, vp(counts), world, vp(ids), -1, gap, vp(out), total, C.byref(n), vp(offs)))
    case("lcm_merge_shard_scores", "NULL n_out", host(ptrs, vp(counts), world, vp(ids), 20, gap, vp(out), total, None, vp(offs)))
    case("lcm_merge_shard_scores", "NULL ids", host(ptrs, vp(counts), world, None, 20, gap, vp(out), total, C.byref(n), vp(offs)))
    case("lcm_merge_shard_scores", "NULL shard_scores", host(None, vp(counts), world, vp(ids), 20, gap, vp(out), total, C.byref(n), vp(offs)))
    case("lcm_merge_shard_scores", "NULL shard_counts", host(ptrs, None, world, vp(ids), 20, gap, vp(out), total, C.byref(n), vp(offs)))
    case("lcm_merge_shard_scores", "ids descending", host(ptrs, vp(counts), world, vp(back), 20, gap, vp(out), total, C.byref(n), vp(offs)))
    case("lcm_merge_shard_scores", "shard 1 one record short", host(ptrs, vp(short), world, vp(ids), 20, gap, vp(out), total, C.byref(n), vp(offs)))
    case("lcm_merge_shard_scores", "cap one below the records", host(ptrs, vp(counts), world, vp(ids), 20, gap, vp(out), total - 1, C.byref(n), vp(offs)))
    case("lcm_merge_shard_scores", "short shard and ids descending", host(ptrs, vp(short), world, vp(back), 20, gap, vp(out), total, C.byref(n), vp(offs)))
    with pkg.Matcher(pkg.default_params()) as m:
        d_g, d_m = m.dev_alloc(total * 8), m.dev_alloc(total * 8)
        dev = lib.lcm_merge_shard_scores_device
        h = m._h
        case("lcm_merge_shard_scores_device", "NULL handle", dev(None, VP(d_g), vp(counts), world, vp(ids), 20, gap, VP(d_m), total, C.byref(n)))
        case("lcm_merge_shard_scores_device", "world 0", dev(h, VP(d_g), vp(counts), 0, vp(ids), 20, gap, VP(d_m), total, C.byref(n)))
        case("lcm_merge_shard_scores_device", "world 9", dev(h, VP(d_g), vp(counts), 9, vp(ids), 20, gap, VP(d_m), total, C.byref(n)))
        case("lcm_merge_shard_scores_device", "NULL n_out", dev(h, VP(d_g), vp(counts), world, vp(ids), 20, gap, VP(d_m), total, None))
        case("lcm_merge_shard_scores_device", "NULL shard_counts", dev(h, VP(d_g), None, world, vp(ids), 20, gap, VP(d_m), total, C.byref(n)))
        case("lcm_merge_shard_scores_device", "NULL ids", dev(h, VP(d_g), vp(counts), world, None, 20, gap, VP(d_m), total, C.byref(n)))
        case("lcm_merge_shard_scores_device", "ids descending", dev(h, VP(d_g), vp(counts), world, vp(back), 20, gap, VP(d_m), total, C.byref(n)))
        case("lcm_merge_shard_scores_device", "shard 1 one record short", dev(h, VP(d_g), vp(short), world, vp(ids), 20, gap, VP(d_m), total, C.byref(n)))
        case("lcm_merge_shard_scores_device", "NULL d_gathered", dev(h, None, vp(counts), world, vp(ids), 20, gap, VP(d_m), total, C.byref(n)))
        case("lcm_merge_shard_scores_device", "cap one below the records", dev(h, VP(d_g), vp(counts), world, vp(ids), 20, gap, VP(d_m), total - 1, C.byref(n)))
        m.dev_free(d_g); m.dev_free(d_m)


def creation():
    p = pkg.default_params()
    g = VP()
    two = np.array([0, 0], np.int32)
    far = np.array([99], np.int32)
    case("lcm_group_create", "NULL out", lib.lcm_group_create(C.byref(p), 1, None, None))
    case("lcm_group_create", "no devices", lib.lcm_group_create(C.byref(p), 0, None, C.byref(g)))
    case("lcm_group_create", "nine devices", lib.lcm_group_create(C.byref(p), 9, None, C.byref(g)))
    case("lcm_group_create", "device 99", lib.lcm_group_create(C.byref(p), 1, i32(far), C.byref(g)))
    case("lcm_group_create_peer", "device 0 twice", lib.lcm_group_create_peer(C.byref(p), 2, i32(two), C.byref(g)))
    case("lcm_group_create_loopback", "nine shards", lib.lcm_group_create_loopback(C.byref(p), 9, 0, C.byref(g)))
    case("lcm_group_create_loopback", "device 99", lib.lcm_group_create_loopback(C.byref(p), 2, 99, C.byref(g)))


def main():
    p = pkg.default_params()
    p.min_gap, p.min_matches, p.sim_threshold = 2, 2, 0.1
    fs = pkg.synth.make_frames(12, 40, seed=5, ragged=True, dup_frac=0.3)
    frames = [np.ascontiguousarray(fs.frame(f)) for f in range(fs.n_frames)]
    g = new_group(p, frames)
    bulk(g, len(frames))
    online(g, frames)
    h = VP()
    case("lcm_group_handle", "rank 3 of 3", lib.lcm_group_handle(g, 3, C.byref(h)))
    lib.lcm_group_destroy(g)
    cross_check(frames)
    merges()
    creation()
    print("\n".join(ROWS))


if __name__ == "__main__":
    main()
