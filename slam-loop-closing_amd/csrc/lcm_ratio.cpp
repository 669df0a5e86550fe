// lcm_ratio.cpp — the bulk search and the online query scored with Lowe's ratio test: what the reference's loop search
// computes per (keyframe, earlier keyframe) pair before it compares with its threshold (src/main.cpp:1375-1388:
// matchFeatures(desc[curr], desc[past], matches, 0.7), then matches.size() >= 300) — the number of ratio-test survivors,
// as an lcm_score record per pair.  Kernel: lcm_ratio.hip (k_ratio_rowlane); always the plain route, whatever the
// handle's kernel variant; lcm_params.ratio / dist_floor / min_matches / sim_threshold are not consulted.
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
                          size_t* n_pairs, size_t* pair_offsets) {
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
        HIP_TRY(hipMemcpyAsync(qc.data(), d_query_counts, sizeof(int32_t) * (size_t)n_q_frames, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        for (int c = 0; c < n_q_frames; ++c)
            if (qc[(size_t)c] < 0 || qc[(size_t)c] > q_stride_rows) return fail(LCM_ERR_INVALID_ARG, "query frame %d has %d rows, stride %d", c, qc[(size_t)c], q_stride_rows);
    }

    // ---- plan: plain-route work items, in state of its own (the handle's `plan` is neither read nor touched)
    lcm::PlanSig sig;
    sig.db_generation = h->db_generation; sig.n_db = h->frames.size();
    sig.n_q = n_q_frames; sig.gap = h->params.min_gap; sig.q_stride = q_stride_rows; sig.item_slots = h->tune_item_slots;
    sig.pack_mode = 0; sig.self = self;
    if (!self) { sig.q_ids.assign(q_ids, q_ids + n_q_frames); sig.q_counts = qc; }
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
                P.items.push_back({(uint32_t)c, (uint32_t)b, (uint32_t)std::min(chunk, e - b), (uint32_t)(P.offsets[(size_t)c] + (size_t)b)});
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
// tickets outstanding on them — are not touched.
int query_scores_ratio_impl(lcm_handle* h, const uint8_t* query, int nq, int query_frame_id, double ratio,
                            lcm_score* out_scores, int32_t* out_frame_ids, int* n_out) {
    if (!h || !n_out || nq < 0 || (nq > 0 && !query)) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    int rc = check_ratio(h, ratio); if (rc) return rc;
    if (nq > lcm::MAX_FUSED_QUERY_ROWS)
        return fail(LCM_ERR_CAPACITY, "ratio-test scoring serves query frames of at most %d rows (got %d): it has no packed route",
                    lcm::MAX_FUSED_QUERY_ROWS, nq);
    rc = set_device(h); if (rc) return rc;
    const int n_elig = eligible_prefix(h, query_frame_id, h->params.min_gap);
    if (n_elig <= 0) return LCM_OK;
    if (!out_scores) return fail(LCM_ERR_INVALID_ARG, "out_scores is NULL");
    rc = ensure_dev(h->d_ratio_q, h->d_ratio_q_bytes, (size_t)std::max(nq, 1) * LCM_DESC_BYTES); if (rc) return rc;
    rc = ensure_dev(h->d_ratio_scores, h->d_ratio_scores_n, (size_t)n_elig); if (rc) return rc;
    rc = wait_db(h); if (rc) return rc;
    // (the caller's buffers are pageable: the copies are staged by the runtime, and the call waits for the stream below)
    if (nq > 0) HIP_TRY(hipMemcpyAsync(h->d_ratio_q, query, (size_t)nq * LCM_DESC_BYTES, hipMemcpyHostToDevice, h->stream));
    lcm::RatioArgs a{};
    a.q_rows = (const uint32_t*)h->d_ratio_q; a.q_counts = nullptr; a.q_stride_words = 0;
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

}  // namespace

extern "C" {

int lcm_all_vs_all_ratio(lcm_handle* h, const void* d_query_rows, const int32_t* d_query_counts, const int32_t* q_ids, int n_q_frames, int q_stride_rows, double ratio, void* d_scores, size_t scores_cap, size_t* n_pairs, size_t* pair_offsets) {
    return guarded([&] { return all_vs_all_ratio_impl(h, d_query_rows, d_query_counts, q_ids, n_q_frames, q_stride_rows, ratio, d_scores, scores_cap, n_pairs, pair_offsets); });
}
int lcm_query_scores_ratio(lcm_handle* h, const uint8_t* query, int nq, int query_frame_id, double ratio, lcm_score* out_scores, int32_t* out_frame_ids, int* n_out) {
    return guarded([&] { return query_scores_ratio_impl(h, query, nq, query_frame_id, ratio, out_scores, out_frame_ids, n_out); });
}

}  // extern "C"
