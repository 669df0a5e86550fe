// lcm_ratio.cpp — the bulk search and the online query scored with Lowe's ratio test: what the reference's loop search
// computes per (keyframe, earlier keyframe) pair before it compares with its threshold (src/main.cpp:1375-1388:
// matchFeatures(desc[curr], desc[past], matches, 0.7), then matches.size() >= 300) — the number of ratio-test survivors,
// as an lcm_score record per pair.  Kernel: lcm_ratio.hip (k_ratio_rowlane); always the plain route, whatever the
// handle's kernel variant; lcm_params.ratio / dist_floor / min_matches / sim_threshold are not consulted.
// And what the reference does with that score (:1382 `rows < 100`, :1388 `>= 300`): lcm_all_vs_all_loops_ratio (verdict and
// ordered compaction on the device: k_ratio_loop_count / k_block_scan / k_ratio_loop_emit), lcm_detect_loops_ratio (one
// frame, verdict on the host), lcm_ratio_loop_test; the group forms live in lcm_group.cpp.
// Part of liblcm_hip.so's host side (C ABI in include/lcm.h); shared state and helpers: lcm_internal.h.
#include "lcm_internal.h"

#include <cmath>

namespace {

// What every k = 2 call refuses (lcm_knn.cpp: check_knn): OpenCV asserts knn == 1 under crossCheck; a NaN or negative
// ratio keeps nothing or is a typo.
int check_ratio(const lcm_handle* h, double ratio) {
    if (h->params.cross_check != 0) return fail(LCM_ERR_INVALID_ARG, "ratio-test scoring needs cross_check = 0 (BFMatcher: knn == 1 under crossCheck)");
    if (std::isnan(ratio) || ratio < 0.0) return fail(LCM_ERR_INVALID_ARG, "ratio must be a number >= 0");
    return LCM_OK;
}

// lim[d2] = number of integers d1 in 0..256 with (double)d1 < ratio * (double)d2 — the reference's expression, as its
// operands promote.  The set is downward closed in d1, so the kernel's `d1 < lim[d2]` is that comparison exactly.  The
// entries past d2 = 256 stay 0 (the kernel clamps "no second neighbour" onto them).
void build_lim(double ratio, uint16_t* lim) {
    for (int d2 = 0; d2 < lcm::RATIO_LIM_ENTRIES; ++d2) {
        int n = 0;
        if (d2 <= 256) {
            const double rhs = ratio * (double)d2;
            while (n <= 256 && (double)n < rhs) ++n;
        }
        lim[d2] = (uint16_t)n;
    }
}

void fill_db(const lcm_handle* h, lcm::RatioArgs& a) {
    a.db_rows = (const uint32_t*)h->d_rows; a.db_counts = h->d_counts;
    a.db_stride_words = (uint32_t)h->stride_rows * LCM_DESC_WORDS;
}

int all_vs_all_ratio_impl(lcm_handle* h, const void* d_query_rows, const int32_t* d_query_counts, const int32_t* q_ids,
                          int n_q_frames, int q_stride_rows, double ratio, void* d_scores, size_t scores_cap,
                          size_t* n_pairs, size_t* pair_offsets, const uint32_t* q_frame_of = nullptr,
                          const int32_t* h_query_counts = nullptr) {
    if (!h || !n_pairs) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    int rc = check_ratio(h, ratio); if (rc) return rc;
    rc = set_device(h); if (rc) return rc;
    const bool self = (d_query_rows == nullptr);
    std::vector<int32_t> self_ids;
    if (self) {
        n_q_frames = (int)h->frames.size();
        self_ids.resize((size_t)n_q_frames);
        for (int i = 0; i < n_q_frames; ++i) self_ids[(size_t)i] = h->frames[(size_t)i].id;
        q_ids = self_ids.data();
        q_stride_rows = h->stride_rows;
    } else if (!d_query_counts || !q_ids || n_q_frames < 0 || q_stride_rows <= 0) {
        return fail(LCM_ERR_INVALID_ARG, "external query set needs counts, ids and a stride");
    }
    // the row counts of an external query set live on the device and may change between calls: fetched on every call,
    // and part of the plan's signature (they pick the workgroup shape), as in lcm_all_vs_all
    std::vector<int32_t> qc;
    if (!self && n_q_frames > 0) {
        qc.resize((size_t)n_q_frames);
        if (h_query_counts) {            // the caller (lcm_group_*) already knows them on the host
            memcpy(qc.data(), h_query_counts, sizeof(int32_t) * (size_t)n_q_frames);
        } else {
            HIP_TRY(hipMemcpyAsync(qc.data(), d_query_counts, sizeof(int32_t) * (size_t)n_q_frames, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        for (int c = 0; c < n_q_frames; ++c)
            if (qc[(size_t)c] < 0 || qc[(size_t)c] > q_stride_rows) return fail(LCM_ERR_INVALID_ARG, "query frame %d has %d rows, stride %d", c, qc[(size_t)c], q_stride_rows);
    }

    // ---- plan: plain-route work items, in state of its own (the handle's `plan` is neither read nor touched)
    lcm::PlanSig sig;
    sig.db_generation = h->db_generation; sig.n_db = h->frames.size();
    sig.n_q = n_q_frames; sig.gap = h->params.min_gap; sig.q_stride = q_stride_rows; sig.item_slots = h->tune_item_slots;
    sig.pack_mode = 0; sig.self = self;
    if (!self) {
        sig.q_ids.assign(q_ids, q_ids + n_q_frames); sig.q_counts = qc;
        // query frame c lives at index q_frame_of[c] of the caller's buffers (the group's rank-major gathered query buffer)
        if (q_frame_of) sig.q_frame_of.assign(q_frame_of, q_frame_of + n_q_frames);
    }
    Plan& P = h->ratio_plan;
    if (P.key == 0 || !(P.sig == sig)) {
        P.key = 0;                        // a failed rebuild must not leave a half-built plan behind the old key
        P.items.clear();
        P.offsets.assign((size_t)n_q_frames + 1, 0);
        size_t total = 0;
        for (int c = 0; c < n_q_frames; ++c) { P.offsets[(size_t)c] = total; total += (size_t)eligible_prefix(h, q_ids[c], h->params.min_gap); }
        P.offsets[(size_t)n_q_frames] = total;
        if (total > 0xFFFFFFFFull) return fail(LCM_ERR_CAPACITY, "more than 2^32 pairs in one call");
        const int chunk = pick_chunk(h, total);
        P.distances = 0; P.algo_bytes = 0; P.max_q_rows = 0;
        std::vector<uint64_t> pre(h->frames.size() + 1, 0);      // prefix sums of stored row counts (accounting)
        for (size_t s = 0; s < h->frames.size(); ++s) pre[s + 1] = pre[s] + (uint64_t)h->frames[s].n;
        auto rows_of = [&](int c) { return self ? h->frames[(size_t)c].n : qc[(size_t)c]; };
        auto elig_of = [&](int c) { return (uint32_t)(P.offsets[(size_t)c + 1] - P.offsets[(size_t)c]); };
        for (int c = 0; c < n_q_frames; ++c) {
            const uint32_t e = elig_of(c);
            if (e == 0) continue;
            P.distances += (uint64_t)rows_of(c) * pre[e];
            P.algo_bytes += pre[e] * 32 + (uint64_t)rows_of(c) * 32 + 8ull * e;
            P.max_q_rows = std::max(P.max_q_rows, rows_of(c));
        }
        if (P.max_q_rows > lcm::MAX_FUSED_QUERY_ROWS)
            return fail(LCM_ERR_CAPACITY, "ratio-test scoring serves query frames of at most %d rows (got %d): it has no packed route",
                        lcm::MAX_FUSED_QUERY_ROWS, P.max_q_rows);
        // heaviest query frames first so the tail of the launch is made of short items
        for (int c = n_q_frames - 1; c >= 0; --c) {
            const int e = (int)elig_of(c);
            for (int b = 0; b < e; b += chunk)
                P.items.push_back({q_frame_of ? q_frame_of[c] : (uint32_t)c, (uint32_t)b, (uint32_t)std::min(chunk, e - b), (uint32_t)(P.offsets[(size_t)c] + (size_t)b)});
        }
        P.n_pairs = total;
        if (!P.items.empty()) {
            rc = ensure_dev(P.d_items, P.d_items_cap, P.items.size()); if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(P.d_items, P.items.data(), sizeof(lcm::WorkItem) * P.items.size(), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        P.sig = std::move(sig);
        P.key = 1;
    }
    *n_pairs = P.n_pairs;
    if (pair_offsets) memcpy(pair_offsets, P.offsets.data(), sizeof(size_t) * ((size_t)n_q_frames + 1));
    if (!d_scores) return LCM_OK;       // sizing call
    if (scores_cap < P.n_pairs) return fail(LCM_ERR_CAPACITY, "scores buffer holds %zu records, need %zu", scores_cap, P.n_pairs);
    if (P.n_pairs == 0) return LCM_OK;

    rc = wait_db(h); if (rc) return rc;
    lcm::RatioArgs a{};
    a.q_rows = self ? (const uint32_t*)h->d_rows : (const uint32_t*)d_query_rows;
    a.q_counts = self ? h->d_counts : d_query_counts;
    a.q_stride_words = (uint32_t)q_stride_rows * LCM_DESC_WORDS;
    fill_db(h, a);
    a.scores = d_scores;
    build_lim(ratio, a.lim);
    // very large searches go out as several launches (<= 2^20 work items), as the plain route of lcm_all_vs_all does
    constexpr size_t MAX_ITEMS_PER_LAUNCH = 1u << 20;
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    uint32_t launches = 0, biggest = 0;
    for (size_t first = 0; first < P.items.size(); first += MAX_ITEMS_PER_LAUNCH) {
        const uint32_t n = (uint32_t)std::min(MAX_ITEMS_PER_LAUNCH, P.items.size() - first);
        a.items = P.d_items + first;
        hipError_t e = lcm::launch_score_ratio(a, n, P.max_q_rows, h->stream);
        if (e != hipSuccess) return fail(LCM_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
        ++launches; biggest = std::max(biggest, n);
    }
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    h->info_pending = true;
    h->info.launches = launches; h->info.workgroups = biggest; h->info.route = LCM_ROUTE_PLAIN;
    h->info.pairs = P.n_pairs; h->info.distances = P.distances; h->info.algo_bytes = P.algo_bytes;
    return LCM_OK;
}

// Synchronous: upload the query, score it against the eligible prefix (implicit work items: nothing else to upload),
// download records.  Everything runs on the handle's stream with buffers of this call's own, so the query slots — and the
// tickets outstanding on them — are not touched.  d_query non-NULL: the query rows are already on the device (a stored
// frame, used in place in the arena) and nothing is uploaded.
int query_scores_ratio_impl(lcm_handle* h, const uint8_t* query, int nq, int query_frame_id, double ratio,
                            lcm_score* out_scores, int32_t* out_frame_ids, int* n_out, const uint8_t* d_query = nullptr) {
    if (!h || !n_out || nq < 0 || (nq > 0 && !query && !d_query)) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    int rc = check_ratio(h, ratio); if (rc) return rc;
    if (nq > lcm::MAX_FUSED_QUERY_ROWS)
        return fail(LCM_ERR_CAPACITY, "ratio-test scoring serves query frames of at most %d rows (got %d): it has no packed route",
                    lcm::MAX_FUSED_QUERY_ROWS, nq);
    rc = set_device(h); if (rc) return rc;
    const int n_elig = eligible_prefix(h, query_frame_id, h->params.min_gap);
    if (n_elig <= 0) return LCM_OK;
    if (!out_scores) return fail(LCM_ERR_INVALID_ARG, "out_scores is NULL");
    if (!d_query) { rc = ensure_dev(h->d_ratio_q, h->d_ratio_q_bytes, (size_t)std::max(nq, 1) * LCM_DESC_BYTES); if (rc) return rc; }
    rc = ensure_dev(h->d_ratio_scores, h->d_ratio_scores_n, (size_t)n_elig); if (rc) return rc;
    rc = wait_db(h); if (rc) return rc;
    // (the caller's buffers are pageable: the copies are staged by the runtime, and the call waits for the stream below)
    if (nq > 0 && !d_query) HIP_TRY(hipMemcpyAsync(h->d_ratio_q, query, (size_t)nq * LCM_DESC_BYTES, hipMemcpyHostToDevice, h->stream));
    lcm::RatioArgs a{};
    a.q_rows = d_query ? (const uint32_t*)d_query : (const uint32_t*)h->d_ratio_q; a.q_counts = nullptr; a.q_stride_words = 0;
    fill_db(h, a);
    a.items = nullptr; a.scores = h->d_ratio_scores;
    const int spi = n_elig >= 8192 ? 4 : (n_elig >= 4096 ? 2 : 1);      // stored slots per workgroup, as lcm_query_scores unsplit
    const uint32_t n_items = (uint32_t)((n_elig + spi - 1) / spi);
    a.imp_spi = (uint32_t)spi; a.imp_total = (uint32_t)n_elig; a.imp_nq = nq;
    build_lim(ratio, a.lim);
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    hipError_t e = lcm::launch_score_ratio(a, n_items, nq, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    h->info_pending = true;
    h->info.launches = 1; h->info.workgroups = n_items; h->info.route = LCM_ROUTE_PLAIN;
    uint64_t dist = 0, bytes = (uint64_t)nq * 32;
    for (int s = 0; s < n_elig; ++s) { dist += (uint64_t)nq * (uint64_t)h->frames[(size_t)s].n; bytes += (uint64_t)h->frames[(size_t)s].n * 32 + 8; }
    h->info.pairs = (uint64_t)n_elig; h->info.distances = dist; h->info.algo_bytes = bytes;
    HIP_TRY(hipMemcpyAsync(out_scores, h->d_ratio_scores, sizeof(lcm_score) * (size_t)n_elig, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (out_frame_ids) for (int s = 0; s < n_elig; ++s) out_frame_ids[s] = h->frames[(size_t)s].id;
    *n_out = n_elig;
    return LCM_OK;
}

// lcm_all_vs_all_ratio with the reference's verdict fused on the device: the score array stays in h->d_bulk_scores (owned
// and reused exactly as lcm_all_vs_all_loops does), the loop-test kernels compact the candidates, only those cross PCIe.
int all_vs_all_loops_ratio_impl(lcm_handle* h, const void* d_query_rows, const int32_t* d_query_counts, const int32_t* q_ids,
                                int n_q_frames, int q_stride_rows, const lcm_ratio_loop_params* rp_in,
                                lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out) {
    if (!h || !n_out) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    lcm_ratio_loop_params rp;
    int rc = lcm::ratio_loop_params_checked(rp_in, &rp); if (rc) return rc;
    const bool self = (d_query_rows == nullptr);
    size_t n_pairs = 0;
    rc = all_vs_all_ratio_impl(h, d_query_rows, d_query_counts, q_ids, n_q_frames, q_stride_rows, rp.ratio, nullptr, 0, &n_pairs, nullptr);
    if (rc) return rc;
    if (n_pairs_out) *n_pairs_out = n_pairs;
    h->bulk_scores_valid = 0;
    if (n_pairs == 0) return LCM_OK;
    rc = ensure_dev(h->d_bulk_scores, h->d_bulk_scores_n, n_pairs); if (rc) return rc;
    rc = all_vs_all_ratio_impl(h, d_query_rows, d_query_counts, q_ids, n_q_frames, q_stride_rows, rp.ratio, h->d_bulk_scores, n_pairs, &n_pairs, nullptr);
    if (rc) return rc;
    const Plan& P = h->ratio_plan;
    const int nq = self ? (int)h->frames.size() : n_q_frames;
    const int ns = (int)h->frames.size();
    std::vector<uint32_t> offs((size_t)nq + 1);
    std::vector<int32_t> qid((size_t)nq), qrows((size_t)nq), did((size_t)ns);
    for (int c = 0; c <= nq; ++c) offs[(size_t)c] = (uint32_t)P.offsets[(size_t)c];
    for (int c = 0; c < nq; ++c) {       // an external set's row counts: the plan has just fetched them (part of its signature)
        qid[(size_t)c] = self ? h->frames[(size_t)c].id : q_ids[c];
        qrows[(size_t)c] = self ? h->frames[(size_t)c].n : P.sig.q_counts[(size_t)c];
    }
    for (int s = 0; s < ns; ++s) did[(size_t)s] = h->frames[(size_t)s].id;
    h->bulk_scores_valid = n_pairs;
    size_t found = 0;
    rc = lcm::ratio_loop_test_device(h, h->d_bulk_scores, n_pairs, offs.data(), nq, qid.data(), qrows.data(), ns, did.data(), rp,
                                     out ? cap : 0, &found);
    *n_out = found;
    if (rc) return rc;                      // LCM_ERR_CAPACITY: *n_out says how many there are
    if (found) {       // on the handle's stream, behind k_ratio_loop_emit; pair order = (current id, matched id) ascending: no sort
        HIP_TRY(hipMemcpyAsync(out, h->d_cands, sizeof(lcm_loop_candidate) * found, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return LCM_OK;
}

// One trip of the reference's outer loop: the current frame (host rows, or a stored frame's rows in place) against every
// eligible stored frame through the online ratio query, then the verdict on the host over those <= db_size records.
int detect_loops_ratio_impl(lcm_handle* h, int current_frame_id, const uint8_t* query, int nq, const lcm_ratio_loop_params* rp_in,
                            lcm_loop_candidate* out, int cap, int* n_out) {
    if (!h || !n_out || cap < 0) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    lcm_ratio_loop_params rp;
    int rc = lcm::ratio_loop_params_checked(rp_in, &rp); if (rc) return rc;
    rc = check_ratio(h, rp.ratio); if (rc) return rc;
    const uint8_t* d_query = nullptr;
    if (!query) {
        RowSrc src{};
        rc = lcm::stored_src(h, current_frame_id, &src, nullptr); if (rc) return rc;
        d_query = src.dev; nq = src.n;
    } else if (nq < 0) {
        return fail(LCM_ERR_INVALID_ARG, "bad argument");
    }
    std::vector<lcm_score> scores(h->frames.size() + 1);
    std::vector<int32_t> ids(h->frames.size() + 1);
    int n = 0;
    rc = query_scores_ratio_impl(h, nq > 0 ? query : nullptr, nq, current_frame_id, rp.ratio, scores.data(), ids.data(), &n, d_query);
    if (rc) return rc;
    int found = 0;
    for (int s = 0; s < n; ++s) found += lcm_ratio_loop_test(&rp, &scores[(size_t)s], nq, nullptr);
    *n_out = found;
    if (found > (out ? cap : 0)) return fail(LCM_ERR_CAPACITY, "%d loop candidates but room for %d", found, out ? cap : 0);
    int k = 0;
    for (int s = 0; s < n; ++s) {           // stored slots ascend with their ids: (current id, matched id) order
        double sim = 0.0;
        if (!lcm_ratio_loop_test(&rp, &scores[(size_t)s], nq, &sim)) continue;
        memset(&out[k], 0, sizeof(out[k]));                     // the padding word too, as the device's records have it
        out[k].current_frame_id = current_frame_id; out[k].matched_frame_id = ids[(size_t)s];
        out[k].num_matches = (int32_t)scores[(size_t)s].good_count; out[k].similarity_score = sim;
        ++k;
    }
    return LCM_OK;
}

}  // namespace

namespace lcm {

int all_vs_all_ratio(lcm_handle* h, const void* d_query_rows, const int32_t* d_query_counts, const int32_t* q_ids,
                     int n_q_frames, int q_stride_rows, double ratio, void* d_scores, size_t scores_cap, size_t* n_pairs,
                     size_t* pair_offsets, const uint32_t* q_frame_of, const int32_t* h_query_counts) {
    return guarded([&] { return all_vs_all_ratio_impl(h, d_query_rows, d_query_counts, q_ids, n_q_frames, q_stride_rows, ratio, d_scores,
                                                      scores_cap, n_pairs, pair_offsets, q_frame_of, h_query_counts); });
}

int ratio_loop_params_checked(const lcm_ratio_loop_params* rp, lcm_ratio_loop_params* out) {
    if (rp) *out = *rp; else lcm_ratio_loop_params_default(out);
    if (std::isnan(out->ratio) || out->ratio < 0.0) return fail(LCM_ERR_INVALID_ARG, "ratio must be a number >= 0");
    if (out->min_rows < 0 || out->min_matches < 0) return fail(LCM_ERR_INVALID_ARG, "min_rows and min_matches must be >= 0");
    return LCM_OK;
}

// loop_test_device's sequence (lcm_bulk.cpp) with the ratio rule's kernels and metadata: offsets | q_ids | q_rows | db_ids
int ratio_loop_test_device(lcm_handle* h, const void* d_scores, size_t n_pairs, const uint32_t* offsets, int n_q,
                           const int32_t* q_ids, const int32_t* q_rows, int n_db, const int32_t* db_ids,
                           const lcm_ratio_loop_params& rp, size_t cap, size_t* n_found) {
    *n_found = 0;
    if (n_pairs == 0) return LCM_OK;
    { const int rc0 = set_device(h); if (rc0) return rc0; }      // (called from a group's per-device host threads too)
    std::vector<int32_t> meta((size_t)(n_q + 1) + 2 * (size_t)n_q + (size_t)n_db);
    int32_t* m_off = meta.data();
    int32_t* m_qid = m_off + (n_q + 1);
    int32_t* m_qrw = m_qid + n_q;
    int32_t* m_did = m_qrw + n_q;
    for (int c = 0; c <= n_q; ++c) m_off[c] = (int32_t)offsets[c];
    memcpy(m_qid, q_ids, sizeof(int32_t) * (size_t)n_q);
    memcpy(m_qrw, q_rows, sizeof(int32_t) * (size_t)n_q);
    memcpy(m_did, db_ids, sizeof(int32_t) * (size_t)n_db);
    const size_t n_blocks = (n_pairs + 255) / 256;
    const int rc = ensure_dev(h->d_meta, h->d_meta_n, meta.size() + 4 + n_blocks); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h->d_meta, meta.data(), sizeof(int32_t) * meta.size(), hipMemcpyHostToDevice, h->stream));
    uint32_t* d_counter = reinterpret_cast<uint32_t*>(h->d_meta + meta.size());
    HIP_TRY(hipMemsetAsync(d_counter, 0, sizeof(uint32_t), h->stream));
    lcm::RatioLoopArgs a{};
    a.scores = d_scores;
    a.offsets = reinterpret_cast<const uint32_t*>(h->d_meta);
    a.q_ids = h->d_meta + (n_q + 1); a.q_rows = a.q_ids + n_q; a.db_ids = a.q_rows + n_q;
    a.out = nullptr; a.counter = d_counter;
    a.block_counts = d_counter + 4;
    a.n_q = (uint32_t)n_q; a.n_pairs = (uint32_t)n_pairs; a.cap = 0;
    a.min_rows = rp.min_rows; a.min_matches = rp.min_matches;
    return count_then_emit(h, d_counter, cap, n_found,
                           [&] { return lcm::launch_ratio_loop_count(a, h->stream); },
                           [&](lcm_loop_candidate* out, uint32_t n) { a.out = out; a.cap = n; return lcm::launch_ratio_loop_emit(a, h->stream); });
}

}  // namespace lcm

extern "C" {

void lcm_ratio_loop_params_default(lcm_ratio_loop_params* p) {
    if (!p) return;
    p->ratio = 0.7; p->min_rows = 100; p->min_matches = 300;       // src/main.cpp:1386, :1382, :1388
}

int lcm_ratio_loop_test(const lcm_ratio_loop_params* p, const lcm_score* s, int rows_query, double* similarity) {
    if (similarity) *similarity = 0.0;
    if (!s) return 0;
    lcm_ratio_loop_params d;
    if (!p) { lcm_ratio_loop_params_default(&d); p = &d; }
    const int rows_train = (int)s->n_train;
    const int den = std::min(rows_query, rows_train);
    if (similarity && den > 0) *similarity = (double)s->good_count / (double)den;       // informational, as lcm_loop_test reports it
    return rows_query >= p->min_rows && rows_train >= p->min_rows &&                    // src/main.cpp:1382
           (long long)s->good_count >= (long long)p->min_matches;                       // src/main.cpp:1388
}

int lcm_all_vs_all_loops_ratio(lcm_handle* h, const void* d_query_rows, const int32_t* d_query_counts, const int32_t* q_ids, int n_q_frames, int q_stride_rows, const lcm_ratio_loop_params* rp, lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out) {
    return guarded([&] { return all_vs_all_loops_ratio_impl(h, d_query_rows, d_query_counts, q_ids, n_q_frames, q_stride_rows, rp, out, cap, n_out, n_pairs_out); });
}
int lcm_detect_loops_ratio(lcm_handle* h, int current_frame_id, const uint8_t* query, int nq, const lcm_ratio_loop_params* rp, lcm_loop_candidate* out, int cap, int* n_out) {
    return guarded([&] { return detect_loops_ratio_impl(h, current_frame_id, query, nq, rp, out, cap, n_out); });
}

int lcm_all_vs_all_ratio(lcm_handle* h, const void* d_query_rows, const int32_t* d_query_counts, const int32_t* q_ids, int n_q_frames, int q_stride_rows, double ratio, void* d_scores, size_t scores_cap, size_t* n_pairs, size_t* pair_offsets) {
    return guarded([&] { return all_vs_all_ratio_impl(h, d_query_rows, d_query_counts, q_ids, n_q_frames, q_stride_rows, ratio, d_scores, scores_cap, n_pairs, pair_offsets); });
}
int lcm_query_scores_ratio(lcm_handle* h, const uint8_t* query, int nq, int query_frame_id, double ratio, lcm_score* out_scores, int32_t* out_frame_ids, int* n_out) {
    return guarded([&] { return query_scores_ratio_impl(h, query, nq, query_frame_id, ratio, out_scores, out_frame_ids, n_out); });
}

}  // extern "C"
