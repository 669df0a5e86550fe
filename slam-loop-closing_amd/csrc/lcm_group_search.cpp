// lcm_group_search.cpp — the bulk search of a group (lcm_group_all_vs_all and its four siblings): one GroupSearch value
// behind the five entry points, and the stages group_search calls in order.  Each of the two exchange steps (shard arenas
// to every device, score records to device 0) exists once per transport; group_search's callers choose neither.
#include "lcm_group_internal.h"

namespace {

using lcm::ShardGeometry;
using lcm::ShardLayout;

// What one call asks for.  The modes: score records (neither flag), + per-pair index checksums through the argmin kernel
// (argmin), loop test on every shard's device so that only candidates leave the devices (loops); ratio: scored with the
// ratio test (lcm::all_vs_all_ratio per shard; rp: ratio + the reference's thresholds, checked by the caller — only its
// ratio is read in the records form).
struct GroupSearch {
    bool ratio = false, loops = false, argmin = false;
    size_t* n_pairs = nullptr;
    lcm_score* out_scores = nullptr; uint32_t* out_isums = nullptr; size_t cap = 0; size_t* pair_offsets = nullptr;   // records forms
    lcm_loop_candidate* out_cands = nullptr; size_t cand_cap = 0; size_t* n_cands = nullptr;                           // loops forms
    const lcm_ratio_loop_params* rp = nullptr;
};

// What the stages of one call hand to each other
struct SearchRun {
    ShardLayout<uint32_t> L;
    ShardGeometry geo;
    bool gather = false;                                     // the database changed since the arenas were last exchanged
    std::vector<std::vector<lcm_loop_candidate>> shard_cands;
    size_t found = 0;                                        // loop candidates over all shards
    bool over = false;                                       // a shard found more than the caller's room
};

// ---- stage: layout, and what a call refuses or answers before any device is touched (*enqueue = false: the call is over)
int search_layout(lcm_group* g, const GroupSearch& s, SearchRun& run, bool* enqueue) {
    *enqueue = false;
    if (const char* what = lcm::shard_layout(g->frames, g->world, g->params.min_gap, run.L)) return fail(LCM_ERR_CAPACITY, "%s", what);
    const uint64_t total = run.L.total;
    *s.n_pairs = (size_t)total;
    if (s.pair_offsets) for (size_t c = 0; c < run.L.offs.size(); ++c) s.pair_offsets[c] = run.L.offs[c];
    if (!s.loops) {
        if (!s.out_scores) return LCM_OK;                   // sizing call
        if (s.cap < total) return fail(LCM_ERR_CAPACITY, "scores buffer holds %zu records, need %llu", s.cap, (unsigned long long)total);
    }
    g->info = lcm_group_info{};
    g->info.n_devices = g->world;
    g->info.loopback = g->loopback ? 1 : 0;
    g->info.pairs = total;
    if (!g->copies) { int cnt = 0; if (ncclCommCount(g->shards[0].comm, &cnt) == ncclSuccess) g->info.rccl_ranks = cnt; }
    *enqueue = total != 0;
    return LCM_OK;
}

// ---- stage: equal shard geometry on every device
int equal_geometry(lcm_group* g, SearchRun& run) {
    const int W = g->world;
    int strides[MAX_WORLD];
    for (int r = 0; r < W; ++r) strides[r] = g->shards[(size_t)r].h->stride_rows;
    run.geo = lcm::shard_geometry(g->frames, W, strides);
    for (int r = 0; r < W; ++r) {
        lcm_handle* h = g->shards[(size_t)r].h;
        // `stride` is a padded row count (up to 65536); lcm_db_reserve takes the rows of a frame (up to 65535) and pads them itself
        int rc = lcm_db_reserve(h, run.geo.shard_cap, std::min(run.geo.stride, MAX_FRAME_ROWS)); if (rc) return rc;
        if (h->stride_rows != run.geo.stride || h->cap_frames < run.geo.shard_cap)
            return fail(LCM_ERR_HIP, "shard %d arena geometry mismatch", r);
    }
    return LCM_OK;
}

// ---- stage: the shard arenas into every device's rank-major query buffer, once per transport.  Both leave device 0
//      current with evg0 / evg1 recorded on its stream around what they enqueued there.
// What ncclAllGather delivers, as device-to-device copies (every shard's appends have landed: host wait)
int gather_arenas_copies(lcm_group* g, const ShardGeometry& geo) {
    const int W = g->world;
    const size_t shard_bytes = geo.shard_bytes(), shard_cap = (size_t)geo.shard_cap;
    int rc;
    for (int r = 0; r < W; ++r) { rc = lcm_sync(g->shards[(size_t)r].h); if (rc) return rc; }
    HIP_TRY(hipEventRecord(g->evg0, g->shards[0].h->stream));
    for (int r = 0; r < W; ++r) {
        const Shard& D = g->shards[(size_t)r];
        rc = set_dev(g, r); if (rc) return rc;               // the copies INTO device r are enqueued on its stream
        for (int s = 0; s < W; ++s) {
            const lcm_handle* src = g->shards[(size_t)s].h;
            HIP_TRY(hipMemcpyAsync(D.buf.qrows + (size_t)s * shard_bytes, src->d_rows, shard_bytes, hipMemcpyDeviceToDevice, D.h->stream));
            HIP_TRY(hipMemcpyAsync(D.buf.qcounts + (size_t)s * shard_cap, src->d_counts, sizeof(int32_t) * shard_cap, hipMemcpyDeviceToDevice, D.h->stream));
        }
    }
    rc = set_dev(g, 0); if (rc) return rc;
    HIP_TRY(hipEventRecord(g->evg1, g->shards[0].h->stream));
    return LCM_OK;
}

int gather_arenas_rccl(lcm_group* g, const ShardGeometry& geo) {
    const int W = g->world;
    const size_t shard_bytes = geo.shard_bytes(), shard_cap = (size_t)geo.shard_cap;
    int rc;
    // every device's stream first waits (on the device, no host wait) for the appends of its own shard
    for (int r = 0; r < W; ++r) { rc = set_dev(g, r); if (rc) return rc; rc = lcm::wait_db(g->shards[(size_t)r].h); if (rc) return rc; }
    rc = set_dev(g, 0); if (rc) return rc;
    HIP_TRY(hipEventRecord(g->evg0, g->shards[0].h->stream));
    NCCL_TRY(ncclGroupStart());
    for (int r = 0; r < W; ++r) {
        const Shard& S = g->shards[(size_t)r];
        lcm_handle* h = S.h;
        NCCL_TRY(ncclAllGather(h->d_rows, S.buf.qrows, shard_bytes, ncclUint8, S.comm, h->stream));
        NCCL_TRY(ncclAllGather(h->d_counts, S.buf.qcounts, shard_cap, ncclInt32, S.comm, h->stream));
    }
    NCCL_TRY(ncclGroupEnd());
    rc = set_dev(g, 0); if (rc) return rc;
    HIP_TRY(hipEventRecord(g->evg1, g->shards[0].h->stream));
    return LCM_OK;
}

// only if the database (or the geometry) changed since the last search
int exchange_arenas(lcm_group* g, SearchRun& run) {
    const int W = g->world;
    const ShardGeometry& geo = run.geo;
    run.gather = g->gathered_stamp != g->db_stamp || g->gathered_cap != geo.shard_cap || g->gathered_stride != geo.stride;
    g->info.arena_gather_skipped = run.gather ? 0 : 1;
    if (!run.gather) return LCM_OK;
    g->gathered_stamp = 0;
    int rc;
    for (int r = 0; r < W; ++r) {
        lcm::ShardBufs& B = g->shards[(size_t)r].buf;
        rc = set_dev(g, r); if (rc) return rc;
        rc = ensure_dev(B.qrows, B.qrows_bytes, geo.shard_bytes() * (size_t)W, 512); if (rc) return rc;
        rc = ensure_dev(B.qcounts, B.qcounts_n, (size_t)geo.shard_cap * (size_t)W); if (rc) return rc;
    }
    rc = set_dev(g, 0); if (rc) return rc;
    rc = g->copies ? gather_arenas_copies(g, geo) : gather_arenas_rccl(g, geo); if (rc) return rc;
    g->info.gathered_query_bytes = (uint64_t)geo.shard_bytes() * (uint64_t)W;
    g->gathered_stamp = g->db_stamp; g->gathered_cap = geo.shard_cap; g->gathered_stride = geo.stride;
    return LCM_OK;
}

// ---- stage: per-shard search — every device plans + launches on its own stream from its own host thread; in the loops
//      forms it then runs the loop test over its own records and downloads its candidates (a stream wait per shard that
//      had pairs)
int score_shards(lcm_group* g, const GroupSearch& s, SearchRun& run) {
    const int W = g->world, N = run.L.N;
    const size_t total = (size_t)run.L.total;
    std::vector<int32_t> ids((size_t)N), counts((size_t)N), kps((size_t)N);
    std::vector<uint32_t> q_frame_of((size_t)N);
    for (int p = 0; p < N; ++p) {
        ids[(size_t)p] = g->frames[(size_t)p].id;
        counts[(size_t)p] = g->frames[(size_t)p].n;
        kps[(size_t)p] = g->frames[(size_t)p].n_kp;
        q_frame_of[(size_t)p] = lcm::q_frame_of(p, W, run.geo.shard_cap);
    }
    int rc = set_dev(g, 0); if (rc) return rc;
    if (!s.loops) {
        // device 0's shard is written straight into the gather buffer (it is the first segment)
        rc = ensure_dev(g->d_gather, g->d_gather_n, total); if (rc) return rc;
        rc = ensure_dev(g->d_merged, g->d_merged_n, total); if (rc) return rc;
        if (s.argmin) {
            rc = ensure_dev(g->d_gather_idx, g->d_gather_idx_n, total); if (rc) return rc;
            rc = ensure_dev(g->d_merged_idx, g->d_merged_idx_n, total); if (rc) return rc;
        }
    }
    for (int r = s.loops ? 0 : 1; r < W; ++r) {
        lcm::ShardBufs& B = g->shards[(size_t)r].buf;
        rc = set_dev(g, r); if (rc) return rc;
        rc = ensure_dev(B.scores, B.scores_n, (size_t)run.L.shard_total(r)); if (rc) return rc;
        if (s.argmin) { rc = ensure_dev(B.isums, B.isums_n, (size_t)run.L.shard_total(r)); if (rc) return rc; }
    }
    run.shard_cands.assign(s.loops ? (size_t)W : 0, std::vector<lcm_loop_candidate>());
    std::vector<size_t> shard_found((size_t)W, 0);
    std::vector<int> shard_over((size_t)W, 0);
    rc = run_all(g, [&](int r) -> int {
        const Shard& S = g->shards[(size_t)r];
        lcm_handle* h = S.h;
        const size_t want = (size_t)run.L.shard_total(r);
        void* dst = (r == 0 && !s.loops) ? (void*)g->d_gather : (void*)S.buf.scores;
        uint32_t* dsum = !s.argmin ? nullptr : (r == 0 ? g->d_gather_idx : S.buf.isums);
        size_t n = 0;
        int rc2 = s.ratio ? lcm::all_vs_all_ratio(h, S.buf.qrows, S.buf.qcounts, ids.data(), N, run.geo.stride, s.rp->ratio, dst, want,
                                                  &n, nullptr, q_frame_of.data(), counts.data())
                          : lcm::all_vs_all(h, S.buf.qrows, S.buf.qcounts, ids.data(), N, run.geo.stride, dst, want, &n, nullptr, dsum,
                                            q_frame_of.data(), counts.data());
        if (rc2) return rc2;
        if (n != want) return fail(LCM_ERR_HIP, "scored %zu pairs, expected %zu", n, want);
        if (!s.loops || want == 0) return LCM_OK;
        // loop test on this shard's device over its own records: the frames it owns are positions r, r + W, ...
        std::vector<int32_t> oid, okp;
        for (int p = r; p < N; p += W) { oid.push_back(ids[(size_t)p]); okp.push_back(kps[(size_t)p]); }
        const size_t room = s.out_cands ? s.cand_cap : 0;
        size_t found = 0;
        rc2 = s.ratio ? lcm::ratio_loop_test_device(h, dst, want, run.L.offr[(size_t)r].data(), N, ids.data(), counts.data(), (int)oid.size(), oid.data(),
                                                    *s.rp, room, &found)
                      : lcm::loop_test_device(h, dst, want, run.L.offr[(size_t)r].data(), N, ids.data(), kps.data(), (int)oid.size(), oid.data(), okp.data(),
                                              room, &found);
        shard_found[(size_t)r] = found;
        if (rc2 == LCM_ERR_CAPACITY) { shard_over[(size_t)r] = 1; return LCM_OK; }     // the caller sums the counts and reports
        if (rc2) return rc2;
        run.shard_cands[(size_t)r].resize(found);
        // each shard's candidates go to the host over that device's OWN PCIe link, all links at once
        if (found) {
            HIP_TRY(hipMemcpyAsync(run.shard_cands[(size_t)r].data(), h->d_cands, sizeof(lcm_loop_candidate) * found, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        return LCM_OK;
    });
    if (rc) return rc;
    for (int r = 0; r < W; ++r) { run.found += shard_found[(size_t)r]; run.over = run.over || shard_over[(size_t)r]; }
    return LCM_OK;
}

// ---- stage (records forms): the shards' records behind device 0's in d_gather (a gatherv), once per transport
// What the grouped ncclSend / ncclRecv delivers, as copies on device 0's stream after a host wait for the sending shard
int gather_records_copies(lcm_group* g, const ShardLayout<uint32_t>& L, bool argmin) {
    hipStream_t st0 = g->shards[0].h->stream;
    for (int r = 1; r < g->world; ++r) {
        const Shard& S = g->shards[(size_t)r];
        const size_t n = (size_t)L.shard_total(r), base = (size_t)L.shard_base[(size_t)r];
        if (!n) continue;
        const int rc = lcm_sync(S.h); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(g->d_gather + base, S.buf.scores, n * sizeof(lcm_score), hipMemcpyDeviceToDevice, st0));
        if (argmin) HIP_TRY(hipMemcpyAsync(g->d_gather_idx + base, S.buf.isums, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st0));
    }
    return set_dev(g, 0);                                   // lcm_sync made the sending shard's device current
}

int gather_records_rccl(lcm_group* g, const ShardLayout<uint32_t>& L, bool argmin) {
    const Shard& S0 = g->shards[0];
    NCCL_TRY(ncclGroupStart());
    for (int r = 1; r < g->world; ++r) {
        const Shard& S = g->shards[(size_t)r];
        const size_t n = (size_t)L.shard_total(r), base = (size_t)L.shard_base[(size_t)r];
        if (!n) continue;
        NCCL_TRY(ncclSend(S.buf.scores, n * sizeof(lcm_score), ncclUint8, 0, S.comm, S.h->stream));
        NCCL_TRY(ncclRecv(g->d_gather + base, n * sizeof(lcm_score), ncclUint8, r, S0.comm, S0.h->stream));
        if (argmin) {
            NCCL_TRY(ncclSend(S.buf.isums, n, ncclUint32, 0, S.comm, S.h->stream));
            NCCL_TRY(ncclRecv(g->d_gather_idx + base, n, ncclUint32, r, S0.comm, S0.h->stream));
        }
    }
    NCCL_TRY(ncclGroupEnd());
    return set_dev(g, 0);
}

// ---- stage (records forms): record exchange, merge on device 0, one download — all on device 0's stream, between ev0 / ev1 / ev2
int merge_and_download(lcm_group* g, const GroupSearch& s, const SearchRun& run) {
    const ShardLayout<uint32_t>& L = run.L;
    hipStream_t st0 = g->shards[0].h->stream;
    int rc = set_dev(g, 0); if (rc) return rc;
    HIP_TRY(hipEventRecord(g->ev0, st0));
    if (g->world > 1) { rc = g->copies ? gather_records_copies(g, L, s.argmin) : gather_records_rccl(g, L, s.argmin); if (rc) return rc; }
    rc = ensure_dev(g->d_meta, g->d_meta_n, (size_t)(L.W + 1) * ((size_t)L.N + 1)); if (rc) return rc;
    rc = upload_merge_meta(g->d_meta, L, st0); if (rc) return rc;
    rc = merge_on_device(g->d_gather, g->d_merged, g->d_meta, L, 2, st0); if (rc) return rc;
    if (s.argmin) { rc = merge_on_device(g->d_gather_idx, g->d_merged_idx, g->d_meta, L, 1, st0); if (rc) return rc; }
    HIP_TRY(hipEventRecord(g->ev1, st0));
    HIP_TRY(hipMemcpyAsync(s.out_scores, g->d_merged, sizeof(lcm_score) * (size_t)L.total, hipMemcpyDeviceToHost, st0));
    if (s.argmin) HIP_TRY(hipMemcpyAsync(s.out_isums, g->d_merged_idx, sizeof(uint32_t) * (size_t)L.total, hipMemcpyDeviceToHost, st0));
    HIP_TRY(hipEventRecord(g->ev2, st0));
    return LCM_OK;
}

// ---- stage: what every search that enqueued anything waits for before it returns — all work on every shard's streams.
//      The outputs have landed, the offset tables this call uploaded are consumed, and no copy of the arena exchange still
//      reads another shard's arena (a shard that owned no pair has not waited for its own until here).
int exit_join(lcm_group* g) {
    for (const Shard& S : g->shards) { const int rc = lcm_sync(S.h); if (rc) return rc; }
    return LCM_OK;
}

// ---- stage: timings (device clocks) — per-shard scoring kernels, the arena exchange; records forms: gather + merge, download
int read_timings(lcm_group* g, const GroupSearch& s, const SearchRun& run) {
    for (int r = 0; r < g->world; ++r) {
        lcm_launch_info li{};
        int rc = lcm_last_launch_info(g->shards[(size_t)r].h, &li); if (rc) return rc;
        g->info.kernel_ms[r] = li.kernel_ms;
        g->info.shard_pairs[r] = li.pairs;
        g->info.kernel_ms_max = std::max(g->info.kernel_ms_max, li.kernel_ms);
        g->info.distances += li.distances;
        g->info.algo_bytes += li.algo_bytes;
    }
    float ms = 0.f;
    if (run.gather) {
        int rc = set_dev(g, 0); if (rc) return rc;
        HIP_TRY(hipEventSynchronize(g->evg1));
        HIP_TRY(hipEventElapsedTime(&ms, g->evg0, g->evg1)); g->info.allgather_ms = ms;
    }
    if (s.loops) return LCM_OK;
    int rc = set_dev(g, 0); if (rc) return rc;
    HIP_TRY(hipEventElapsedTime(&ms, g->ev0, g->ev1)); g->info.gather_merge_ms = ms;
    HIP_TRY(hipEventElapsedTime(&ms, g->ev1, g->ev2)); g->info.download_ms = ms;
    g->info.gathered_score_bytes = (uint64_t)(run.L.total - run.L.shard_total(0)) * (sizeof(lcm_score) + (s.argmin ? sizeof(uint32_t) : 0));
    return LCM_OK;
}

// ---- stage (loops forms): the caller's room, then W sorted lists -> one, on the host over candidates only
int deliver_candidates(const GroupSearch& s, const SearchRun& run) {
    if (run.over || run.found > s.cand_cap || (!s.out_cands && run.found))
        return fail(LCM_ERR_CAPACITY, "%zu loop candidates but room for %zu", run.found, s.out_cands ? s.cand_cap : (size_t)0);
    lcm::merge_candidates(run.shard_cands, s.out_cands);
    return LCM_OK;
}

int group_search(lcm_group* g, const GroupSearch& s) {
    SearchRun run;
    bool enqueue = false;
    int rc = search_layout(g, s, run, &enqueue); if (rc || !enqueue) return rc;
    rc = equal_geometry(g, run); if (rc) return rc;
    rc = exchange_arenas(g, run); if (rc) return rc;
    rc = score_shards(g, s, run); if (rc) return rc;
    if (s.loops) *s.n_cands = run.found;
    else { rc = merge_and_download(g, s, run); if (rc) return rc; }
    rc = exit_join(g); if (rc) return rc;
    rc = read_timings(g, s, run); if (rc) return rc;
    return s.loops ? deliver_candidates(s, run) : LCM_OK;
}

// what every k = 2 call refuses, before any shard is touched
int group_check_ratio(const lcm_group* g, const lcm_ratio_loop_params* rp_in, lcm_ratio_loop_params* rp) {
    const int rc = lcm::ratio_loop_params_checked(rp_in, rp); if (rc) return rc;
    if (g->params.cross_check != 0) return fail(LCM_ERR_INVALID_ARG, "ratio-test scoring needs cross_check = 0 (BFMatcher: knn == 1 under crossCheck)");
    return LCM_OK;
}

int run_search(lcm_group* g, const GroupSearch& s) {
    return guarded([&] { return group_search(g, s); });
}

// the loops forms report the pair count through an optional pointer
int run_loops_search(lcm_group* g, GroupSearch& s, size_t* n_pairs_out) {
    size_t n_pairs = 0;
    s.loops = true; s.n_pairs = &n_pairs;
    const int rc = run_search(g, s);
    if (n_pairs_out) *n_pairs_out = n_pairs;
    return rc;
}

}  // namespace

extern "C" {

int lcm_group_all_vs_all(lcm_group* g, lcm_score* out_scores, size_t cap, size_t* n_pairs, size_t* pair_offsets) {
    if (!g || !n_pairs) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    GroupSearch s;
    s.n_pairs = n_pairs; s.out_scores = out_scores; s.cap = cap; s.pair_offsets = pair_offsets;
    return run_search(g, s);
}

int lcm_group_all_vs_all_argmin(lcm_group* g, lcm_score* out_scores, uint32_t* out_index_sums, size_t cap, size_t* n_pairs, size_t* pair_offsets) {
    if (!g || !n_pairs) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (out_scores && !out_index_sums) return fail(LCM_ERR_INVALID_ARG, "out_index_sums is NULL");
    GroupSearch s;
    s.argmin = true;
    s.n_pairs = n_pairs; s.out_scores = out_scores; s.out_isums = out_index_sums; s.cap = cap; s.pair_offsets = pair_offsets;
    return run_search(g, s);
}

int lcm_group_all_vs_all_loops(lcm_group* g, lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out) {
    if (!g || !n_out) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    GroupSearch s;
    s.out_cands = out; s.cand_cap = cap; s.n_cands = n_out;
    return run_loops_search(g, s, n_pairs_out);
}

int lcm_group_all_vs_all_ratio(lcm_group* g, double ratio, lcm_score* out_scores, size_t cap, size_t* n_pairs, size_t* pair_offsets) {
    if (!g || !n_pairs) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    lcm_ratio_loop_params rp;
    lcm_ratio_loop_params_default(&rp);
    rp.ratio = ratio;
    const int rc = group_check_ratio(g, &rp, &rp); if (rc) return rc;
    GroupSearch s;
    s.ratio = true; s.rp = &rp;
    s.n_pairs = n_pairs; s.out_scores = out_scores; s.cap = cap; s.pair_offsets = pair_offsets;
    return run_search(g, s);
}

int lcm_group_all_vs_all_loops_ratio(lcm_group* g, const lcm_ratio_loop_params* rp_in, lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out) {
    if (!g || !n_out) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    lcm_ratio_loop_params rp;
    const int rc = group_check_ratio(g, rp_in, &rp); if (rc) return rc;
    GroupSearch s;
    s.ratio = true; s.rp = &rp;
    s.out_cands = out; s.cand_cap = cap; s.n_cands = n_out;
    return run_loops_search(g, s, n_pairs_out);
}

int lcm_group_last_info(const lcm_group* g, lcm_group_info* info) {
    if (!g || !info) return fail(LCM_ERR_INVALID_ARG, "NULL argument");
    *info = g->info;
    return LCM_OK;
}

}  // extern "C"
