// lcm_knn.cpp — pair mode with two neighbours per query row: knnMatch(k = 2) + Lowe's ratio test, the matcher the
// reference runs for consecutive frames and for its loop search (src/main.cpp:509-534, :1154, :1386).
// The planning, the staging block and the uploads are the k = 1 pair mode's (lcm_pair.cpp: run_pair_jobs with k = 2); the
// kernels are lcm_knn.hip's; the ratio test runs here, on the shipped integers, in IEEE double.
// Part of liblcm_hip.so's host side (C ABI in include/lcm.h); shared state and helpers: lcm_internal.h.
#include "lcm_internal.h"

#include <cmath>

namespace {
using lcm::batch_jobs;
using lcm::pair_keys;
using lcm::run_pair_jobs;
using lcm::stored_src;

constexpr uint32_t NONE = 0xFFFFFFFFu;      // key of a neighbour that does not exist

// What every k = 2 call refuses: OpenCV asserts knn == 1 under crossCheck; a NaN or negative ratio keeps nothing or is a typo.
int check_knn(const lcm_handle* h, double ratio) {
    if (h->params.cross_check != 0) return fail(LCM_ERR_INVALID_ARG, "k = 2 matching needs cross_check = 0 (BFMatcher: knn == 1 under crossCheck)");
    if (std::isnan(ratio) || ratio < 0.0) return fail(LCM_ERR_INVALID_ARG, "ratio must be a number >= 0");
    return LCM_OK;
}

// Lowe's ratio test over one job's key pairs (keys[2 q], keys[2 q + 1]) -> DMatch records appended at out[*n_total ...],
// query order kept: `best` stays iff best.distance < ratio * second.distance, evaluated in double as the reference's
// expression promotes; a query row with fewer than two neighbours is dropped (src/main.cpp:524-531).
int emit_ratio(const uint32_t* keys, int nq, double ratio, lcm_dmatch* out, size_t cap, size_t* n_total) {
    size_t k = *n_total;
    for (int i = 0; i < nq; ++i) {
        const uint32_t k1 = keys[2 * (size_t)i], k2 = keys[2 * (size_t)i + 1];
        if (k2 == NONE) continue;
        const uint32_t d1 = k1 >> lcm::KEY_SHIFT, d2 = k2 >> lcm::KEY_SHIFT;
        if (!((double)d1 < ratio * (double)d2)) continue;
        if (k >= cap) return fail(LCM_ERR_CAPACITY, "match buffer holds %zu records: too small", cap);
        out[k].query_idx = i;
        out[k].train_idx = (int32_t)(k1 & lcm::KEY_IDX_MASK);
        out[k].img_idx = 0;
        out[k].distance = (float)d1;
        ++k;
    }
    *n_total = k;
    return LCM_OK;
}

int knn2_pair_impl(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt,
                   int32_t* train_idx, uint16_t* dist, int* n_neighbours) {
    if (!h || nq < 0 || nt < 0) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (n_neighbours) *n_neighbours = 0;
    int rc = check_knn(h, 0.0); if (rc) return rc;
    if (nq == 0 || nt == 0) return LCM_OK;
    if (!query || !train || !train_idx || !dist) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    std::vector<uint32_t> keys;
    rc = pair_keys(h, RowSrc{query, nullptr, nq}, RowSrc{train, nullptr, nt}, keys, 0, 2); if (rc) return rc;
    for (size_t i = 0; i < 2 * (size_t)nq; ++i) {
        const bool none = keys[i] == NONE;
        train_idx[i] = none ? -1 : (int32_t)(keys[i] & lcm::KEY_IDX_MASK);
        dist[i] = none ? (uint16_t)0xFFFF : (uint16_t)(keys[i] >> lcm::KEY_SHIFT);
    }
    if (n_neighbours) *n_neighbours = std::min(nt, 2);
    return LCM_OK;
}

int match_features_ratio_impl(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt, double ratio,
                              lcm_dmatch* out, int* n_out) {
    if (!h || nq < 0 || nt < 0 || !n_out) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    int rc = check_knn(h, ratio); if (rc) return rc;
    if (nq == 0 || nt == 0) return LCM_OK;
    if (!query || !train || !out) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    std::vector<uint32_t> keys;
    rc = pair_keys(h, RowSrc{query, nullptr, nq}, RowSrc{train, nullptr, nt}, keys, 0, 2); if (rc) return rc;
    size_t n = 0;
    rc = emit_ratio(keys.data(), nq, ratio, out, (size_t)nq, &n); if (rc) return rc;
    *n_out = (int)n;
    return LCM_OK;
}

int match_stored_ratio_impl(lcm_handle* h, int query_frame_id, int train_frame_id, double ratio, lcm_dmatch* out, int cap, int* n_out) {
    if (!h || !n_out) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    int rc = check_knn(h, ratio); if (rc) return rc;
    rc = set_device(h); if (rc) return rc;
    RowSrc q{}, t{};
    rc = stored_src(h, query_frame_id, &q, nullptr); if (rc) return rc;
    rc = stored_src(h, train_frame_id, &t, nullptr); if (rc) return rc;
    if (q.n == 0 || t.n == 0) return LCM_OK;
    if (!out || cap < q.n) return fail(LCM_ERR_CAPACITY, "need room for %d matches", q.n);
    std::vector<uint32_t> keys;
    rc = pair_keys(h, q, t, keys, 0, 2); if (rc) return rc;
    size_t n = 0;
    rc = emit_ratio(keys.data(), q.n, ratio, out, (size_t)cap, &n); if (rc) return rc;
    *n_out = (int)n;
    return LCM_OK;
}

// The ratio-filtered match lists of MANY pairs in one launch: the reference's loop search (src/main.cpp:1375-1388 matches
// the current keyframe against every earlier one and counts the survivors).  q_host != NULL: one query frame from the
// host against stored train frames; else both sides stored.
int match_batch_ratio_impl(lcm_handle* h, const uint8_t* q_host, int nq_host, const lcm_pair_ref* pairs, const int32_t* train_ids,
                           int n_pairs, double ratio, lcm_dmatch* out, size_t cap, size_t* offsets) {
    if (!h || n_pairs < 0 || !offsets || (n_pairs > 0 && !pairs && !train_ids)) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    offsets[0] = 0;
    int rc = check_knn(h, ratio); if (rc) return rc;
    rc = set_device(h); if (rc) return rc;
    if (q_host && nq_host > lcm::MAX_FUSED_QUERY_ROWS * 64) return fail(LCM_ERR_CAPACITY, "query frame too large");
    std::vector<PairJob> jobs;
    std::vector<int> job_of;
    size_t stage_bytes = 0;
    rc = batch_jobs(h, q_host, nq_host, pairs, train_ids, n_pairs, jobs, job_of, &stage_bytes); if (rc) return rc;
    const uint32_t* keys = nullptr;
    std::vector<size_t> row0;
    rc = run_pair_jobs(h, h->d_rows, h->d_rows, q_host != nullptr, false, stage_bytes, jobs, &keys, row0, 2); if (rc) return rc;
    size_t total = 0;
    for (int p = 0; p < n_pairs; ++p) {
        offsets[p] = total;
        const int j = job_of[(size_t)p];
        if (j < 0) continue;
        rc = emit_ratio(keys + 2 * row0[(size_t)j], jobs[(size_t)j].nq, ratio, out, out ? cap : 0, &total); if (rc) return rc;
    }
    offsets[n_pairs] = total;
    return LCM_OK;
}

}  // namespace

extern "C" {

int lcm_knn2_pair(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt, int32_t* train_idx, uint16_t* dist, int* n_neighbours) {
    return guarded([&] { return knn2_pair_impl(h, query, nq, train, nt, train_idx, dist, n_neighbours); });
}
int lcm_match_features_ratio(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt, double ratio, lcm_dmatch* out, int* n_out) {
    return guarded([&] { return match_features_ratio_impl(h, query, nq, train, nt, ratio, out, n_out); });
}
int lcm_match_stored_ratio(lcm_handle* h, int query_frame_id, int train_frame_id, double ratio, lcm_dmatch* out, int cap, int* n_out) {
    return guarded([&] { return match_stored_ratio_impl(h, query_frame_id, train_frame_id, ratio, out, cap, n_out); });
}
int lcm_match_stored_batch_ratio(lcm_handle* h, const lcm_pair_ref* pairs, int n_pairs, double ratio, lcm_dmatch* out, size_t cap, size_t* offsets) {
    return guarded([&] { return match_batch_ratio_impl(h, nullptr, 0, pairs, nullptr, n_pairs, ratio, out, cap, offsets); });
}
int lcm_match_query_batch_ratio(lcm_handle* h, const uint8_t* query, int nq, const int32_t* train_frame_ids, int n_trains, double ratio,
                                lcm_dmatch* out, size_t cap, size_t* offsets) {
    if (nq < 0 || (nq > 0 && !query)) return fail(LCM_ERR_INVALID_ARG, "bad query rows");
    static const uint8_t none[LCM_DESC_BYTES] = {0};
    return guarded([&] { return match_batch_ratio_impl(h, query ? query : none, nq, nullptr, train_frame_ids, n_trains, ratio, out, cap, offsets); });
}

}  // extern "C"
