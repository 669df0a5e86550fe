// lcm_l2.cpp — pair mode on SIFT rows (128 uint8, L2): knnMatch(k = 2) + Lowe's ratio test as the reference runs them on
// cv::SIFT descriptors (src/main.cpp:497-504, :509-534, :1154, :1375-1388).  The kernels are lcm_l2.hip's; the tile space and
// the (query chunk x train segment) items are planned in lcm_l2_host.h; this file stages the matrices, runs the plans, turns
// the shipped integer squared distances into OpenCV's float distances (sqrtf, correctly rounded on the host) and runs the ratio
// test in IEEE double.  The loop search's form (lcm_score_pairs_ratio_l2, lcm_loop_search_ratio_l2) wants the survivor COUNT per
// pair only: lcm_l2_count.hip scores a pair's whole train matrix in one workgroup per query chunk and decides on the device, so
// 8 bytes per pair come back.  The keyframe store runs the same functions over its slots (lcm_l2_db.cpp).  Shared: lcm_internal.h.
#include "lcm_internal.h"

#include <cmath>
#include <limits>

namespace {

constexpr uint32_t NONE = lcm::L2_NONE;
constexpr int TILE = lcm::L2_TILE_ROWS, ROW = LCM_SIFT_BYTES;
static_assert(LCM_SIFT_BYTES == lcm::L2_ROW_BYTES, "row size");

// Where a call's matrices are, in one of two ways.  stored != NULL: the store's slots, as they are.  Else host matrices, laid out
// over `rows` by l2_tile_space in the handle's scratch, which grows; l2_stage uploads them behind the run's own allocations
// (pageable sources: alive and unchanged until the run has waited).  call_tile0 first: a plan's refusals precede every allocation.
const uint32_t* call_tile0(const L2Where* stored, const int* rows, int n_frames, std::vector<uint32_t>& tile0, std::vector<uint32_t>& tile_meta) {
    if (stored) return stored->tile0;
    lcm::l2_tile_space(rows, n_frames, tile0, tile_meta);
    return tile0.data();
}
int call_where(lcm_handle* h, const L2Where* stored, const uint8_t* const* frames, const int* rows, int n_frames,
               const std::vector<uint32_t>& tile0, const std::vector<uint32_t>& tile_meta, L2Where* w) {
    if (stored) { *w = *stored; return LCM_OK; }
    auto& s = h->l2;
    const size_t n_tiles = tile_meta.size();
    int rc = ensure_dev(s.d_raw, s.d_raw_n, n_tiles * (size_t)lcm::L2_TILE_BYTES); if (rc) return rc;
    rc = ensure_dev(s.d_img, s.d_img_n, n_tiles * (size_t)lcm::L2_TILE_BYTES); if (rc) return rc;
    rc = ensure_dev(s.d_tw, s.d_tw_n, n_tiles * (size_t)TILE); if (rc) return rc;
    *w = L2Where{s.d_raw, s.d_img, s.d_tw, tile0.data(), tile_meta.data(), n_tiles, frames, rows, n_frames};
    return LCM_OK;
}

// A run's table block: [tile words of the tiles to pack | zeros up to a multiple of `align` | body_bytes, zeroed]; the body's offset
size_t l2_table(const L2Where& w, size_t align, size_t body_bytes, std::vector<uint8_t>& tab) {
    const size_t off = (w.n_tiles * sizeof(uint32_t) + align - 1) & ~(align - 1);
    tab.assign(off + body_bytes, 0);
    if (w.n_tiles) memcpy(tab.data(), w.tile_meta, w.n_tiles * sizeof(uint32_t));
    return off;
}

// One upload per non-empty host matrix, one copy for the whole table block, then the pack, which reads its tile words from its head
int l2_stage(lcm_handle* h, const L2Where& w, const std::vector<uint8_t>& tab) {
    auto& s = h->l2;
    const int rc = ensure_dev(s.d_tab, s.d_tab_n, tab.size()); if (rc) return rc;
    for (int f = 0; f < w.n_frames; ++f)
        if (w.rows[f] > 0)
            HIP_TRY(hipMemcpyAsync(s.d_raw + (size_t)w.tile0[(size_t)f] * lcm::L2_TILE_BYTES, w.frames[f], (size_t)w.rows[f] * ROW,
                                   hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(s.d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, h->stream));
    if (w.n_tiles == 0) return LCM_OK;
    const lcm::L2PackArgs pa{s.d_raw, reinterpret_cast<const uint32_t*>(s.d_tab), s.d_img, s.d_tw, (uint32_t)w.n_tiles};
    const hipError_t e = lcm::launch_l2_pack(pa, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "pack kernel launch failed: %s", hipGetErrorString(e));
    return LCM_OK;
}

inline float dist_of(uint32_t D) { return std::sqrt((float)D); }      // D < 2^24: the conversion is exact, sqrtf correctly rounded

// Lowe's ratio test over one pair's rows (src/main.cpp:524-531): survivors of `s1 < ratio * s2` in double; a row with
// fewer than two neighbours is dropped.  out == NULL: count only.  One object at a fixed place in its cache lines.
__attribute__((noinline, aligned(64))) size_t emit_ratio(const uint32_t* fin, int nq, double ratio, lcm_dmatch* out) {
    size_t k = 0;
    for (int i = 0; i < nq; ++i) {
        const uint32_t* r = fin + 4 * (size_t)i;
        if (r[2] == NONE) continue;
        const float s1 = dist_of(r[0]), s2 = dist_of(r[2]);
        if (!((double)s1 < ratio * (double)s2)) continue;
        if (out) out[k] = lcm_dmatch{i, (int32_t)r[1], 0, s1};
        ++k;
    }
    return k;
}

// What the list call and the count calls refuse alike about the matrices
int check_frames(const uint8_t* const* frames, const int* rows, int n_frames) {
    for (int f = 0; f < n_frames; ++f) {
        const int rc = lcm::l2_check_rows(rows[f]); if (rc) return rc;
        if (rows[f] > 0 && !frames[f]) return fail(LCM_ERR_INVALID_ARG, "matrix %d is NULL", f);
    }
    return LCM_OK;
}

// A list run and its download: the keys of pair p's rows at (*fin)[4 * (row0[p] + r)], in pinned host memory that stays valid
// until the next L2 call on this handle.  A list call lays out EVERY host matrix it is passed, named by a pair or not.
int l2_run(lcm_handle* h, const L2Where* stored, const uint8_t* const* frames, const int* rows, int n_frames,
           const std::vector<L2Pair>& pairs, L2Run& run, const uint32_t** fin) {
    int rc = set_device(h); if (rc) return rc;
    *fin = nullptr;
    std::vector<uint32_t> tile0, tile_meta;
    rc = lcm::l2_refused(lcm::l2_run_plan(pairs, rows, call_tile0(stored, rows, n_frames, tile0, tile_meta), run.plan)); if (rc) return rc;
    if (pairs.empty()) return LCM_OK;
    L2Where w;
    rc = call_where(h, stored, frames, rows, n_frames, tile0, tile_meta, &w); if (rc) return rc;
    auto& s = h->l2;
    rc = ensure_pinned(s.h_fin, s.h_fin_n, run.plan.row0.back()); if (rc) return rc;
    rc = lcm::l2_enqueue(h, w, run); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(s.h_fin, s.d_fin, run.plan.row0.back() * sizeof(uint4), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *fin = reinterpret_cast<const uint32_t*>(s.h_fin);
    return LCM_OK;
}

// ---- ratio-test counts per pair (lcm_l2_count.hip) ------------------------------------------------------------------------
// A count run over the live pairs (both sides non-empty; the device has been set).  A count call lays out and uploads only the
// host matrices that a live pair names: the others take no room in its tile space.  A list call lays out all: algo_bytes shows it.
int l2_counts(lcm_handle* h, const L2Where* stored, const uint8_t* const* frames, const int* rows, int n_frames,
              const std::vector<L2Pair>& live, double ratio, const lcm_l2_score** rec) {
    if (live.empty()) return LCM_OK;
    std::vector<int> used((size_t)n_frames, 0);
    for (const L2Pair& p : live) { used[(size_t)p.q] = rows[p.q]; used[(size_t)p.t] = rows[p.t]; }
    std::vector<uint32_t> tile0, tile_meta;
    lcm::L2CountPlan pl;
    int rc = lcm::l2_refused(lcm::l2_count_plan(live, rows, call_tile0(stored, used.data(), n_frames, tile0, tile_meta), pl)); if (rc) return rc;
    L2Where w;
    rc = call_where(h, stored, frames, used.data(), n_frames, tile0, tile_meta, &w); if (rc) return rc;
    return lcm::l2_count_run(h, w, pl, live.size(), ratio, rec);
}

}  // namespace

namespace lcm {

int l2_check_knn(const lcm_handle* h, double ratio) {
    if (h->params.cross_check != 0) return fail(LCM_ERR_INVALID_ARG, "k = 2 matching needs cross_check = 0 (BFMatcher: knn == 1 under crossCheck)");
    if (std::isnan(ratio) || ratio < 0.0) return fail(LCM_ERR_INVALID_ARG, "ratio must be a number >= 0");
    return LCM_OK;
}

int l2_check_rows(int n) {
    if (n < 0) return fail(LCM_ERR_INVALID_ARG, "negative row count");
    if (n > MAX_FRAME_ROWS) return fail(LCM_ERR_CAPACITY, "a SIFT matrix holds at most %d rows", MAX_FRAME_ROWS);
    return LCM_OK;
}

int l2_refused(const char* what) { return what ? fail(LCM_ERR_CAPACITY, "%s", what) : LCM_OK; }

// Stages, scores run.plan's pairs (at least one), folds, rescans: final_keys -> h->l2.d_fin; run.tab and host matrices stay in flight
int l2_enqueue(lcm_handle* h, const L2Where& w, L2Run& run) {
    const L2RunPlan& pl = run.plan;
    const size_t P = pl.jobs.size(), n_items = pl.items.size(), total_rows = pl.row0[P];
    auto& s = h->l2;
    // [tile words | items | jobs | counter]: items of 16 bytes, aligned to that; the last 16 bytes hold the rescan's counter, zero
    const size_t off_items = l2_table(w, sizeof(L2Item), n_items * sizeof(L2Item) + P * sizeof(L2Job) + 16, run.tab);
    const size_t off_jobs = off_items + n_items * sizeof(L2Item), off_counter = off_jobs + P * sizeof(L2Job);
    memcpy(run.tab.data() + off_items, pl.items.data(), n_items * sizeof(L2Item));
    memcpy(run.tab.data() + off_jobs, pl.jobs.data(), P * sizeof(L2Job));
    int rc = ensure_dev(s.d_seg, s.d_seg_n, n_items * (size_t)pl.chunk_rows); if (rc) return rc;
    rc = ensure_dev(s.d_fin, s.d_fin_n, total_rows); if (rc) return rc;
    rc = ensure_dev(s.d_flag, s.d_flag_n, total_rows); if (rc) return rc;
    rc = l2_stage(h, w, run.tab); if (rc) return rc;
    const L2ScoreArgs sa{w.d_img, w.d_tw, reinterpret_cast<const L2Item*>(s.d_tab + off_items), s.d_seg, (uint32_t)pl.chunk_rows};
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    hipError_t e = launch_l2_score(sa, (uint32_t)n_items, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "score kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    h->info_pending = true;
    h->info.workgroups = (uint32_t)n_items; h->info.route = LCM_ROUTE_PLAIN; h->info.launches = w.n_tiles ? 4 : 3;
    h->info.pairs = P; h->info.distances = pl.distances; h->info.algo_bytes = 2 * w.n_tiles * (uint64_t)L2_TILE_BYTES + total_rows * 16;
    const L2FoldArgs fa{s.d_seg, (uint32_t)pl.chunk_rows, reinterpret_cast<const L2Job*>(s.d_tab + off_jobs), s.d_fin,
                        reinterpret_cast<uint32_t*>(s.d_tab + off_counter), s.d_flag, (uint32_t)total_rows, w.d_raw, 0};
    e = launch_l2_fold(fa, (uint32_t)P, (uint32_t)pl.max_nq, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "fold kernel launch failed: %s", hipGetErrorString(e));
    e = launch_l2_rescan(fa, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "rescan kernel launch failed: %s", hipGetErrorString(e));
    run.d_jobs = fa.jobs;
    return LCM_OK;
}

// Stages and counts pl's n_pairs (at least one) live pairs: pair j's record -> (*rec)[j], pinned, valid until the next count call
int l2_count_run(lcm_handle* h, const L2Where& w, const L2CountPlan& pl, size_t n_pairs, double ratio, const lcm_l2_score** rec) {
    auto& s = h->l2;
    const size_t P = n_pairs, n_items = pl.items.size();
    // [tile words | items]: the items are 32 bytes and aligned to that; this kernel has no counter word
    std::vector<uint8_t> tab;
    const size_t off_items = l2_table(w, sizeof(L2CountItem), n_items * sizeof(L2CountItem), tab);
    memcpy(tab.data() + off_items, pl.items.data(), n_items * sizeof(L2CountItem));
    int rc = ensure_dev(s.d_score, s.d_score_n, P); if (rc) return rc;
    rc = ensure_pinned(s.h_score, s.h_score_n, P); if (rc) return rc;
    rc = l2_stage(h, w, tab); if (rc) return rc;
    hipError_t e = launch_l2_count_init(s.d_score, (uint32_t)P, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "count init kernel launch failed: %s", hipGetErrorString(e));
    const L2CountArgs ca{w.d_img, w.d_tw, reinterpret_cast<const L2CountItem*>(s.d_tab + off_items), s.d_score, ratio, (uint32_t)pl.chunk_rows};
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    e = launch_l2_count(ca, (uint32_t)n_items, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "count kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    h->info_pending = true;
    h->info.workgroups = (uint32_t)n_items; h->info.route = LCM_ROUTE_PLAIN; h->info.launches = w.n_tiles ? 3 : 2;
    h->info.pairs = P; h->info.distances = pl.distances; h->info.algo_bytes = 2 * w.n_tiles * (uint64_t)L2_TILE_BYTES + P * sizeof(lcm_l2_score);
    HIP_TRY(hipMemcpyAsync(s.h_score, s.d_score, P * sizeof(lcm_l2_score), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));       // also: the tables and a host call's matrices (pageable) have been consumed
    *rec = s.h_score;
    return LCM_OK;
}

// How both loop searches end: the pairs formed, then two passes over the records: the count, and (if it fits) the candidates
int l2_candidates_out(const L2StorePlan& pl, const int* rows, size_t S, const std::vector<L2StoreCurr>& currs, const lcm_l2_score* rec,
                      int min_matches, lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out) {
    if (n_pairs_out) *n_pairs_out = pl.n_pairs;
    const size_t found = l2_store_walk(pl, rows, S, currs, rec, min_matches, nullptr);
    *n_out = found;
    if (found > (out ? cap : 0)) return fail(LCM_ERR_CAPACITY, "%zu loop candidates but room for %zu", found, out ? cap : (size_t)0);
    if (found) l2_store_walk(pl, rows, S, currs, rec, min_matches, out);
    return LCM_OK;
}

// stored != NULL: the matrices are the store's slots (frames unused, rows / n_frames the store's)
int l2_match_pairs(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const lcm_pair_ref* pairs, int n_pairs,
                        double ratio, lcm_dmatch* out, size_t cap, size_t* offsets, const L2Where* stored) {
    if (!h || n_frames < 0 || n_pairs < 0 || !offsets || (!stored && n_frames > 0 && (!frames || !rows)) || (n_pairs > 0 && !pairs))
        return fail(LCM_ERR_INVALID_ARG, "bad argument");
    offsets[0] = 0;
    int rc = l2_check_knn(h, ratio); if (rc) return rc;
    if (!stored) { rc = check_frames(frames, rows, n_frames); if (rc) return rc; }
    std::vector<L2Pair> live;
    std::vector<int> job_of;
    rc = l2_read_pairs(pairs, (size_t)n_pairs, rows, n_frames, live, job_of); if (rc) return rc;
    const uint32_t* fin = nullptr;
    L2Run run;
    rc = l2_run(h, stored, frames, rows, n_frames, live, run, &fin); if (rc) return rc;
    const std::vector<size_t>& row0 = run.plan.row0;
    // sizes first: a too-small `cap` is refused before anything is written
    std::vector<size_t> count((size_t)n_pairs, 0);
    size_t total = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int j = job_of[(size_t)p];
        if (j >= 0) count[(size_t)p] = emit_ratio(fin + 4 * row0[(size_t)j], rows[live[(size_t)j].q], ratio, nullptr);
        total += count[(size_t)p];
    }
    if (total > (out ? cap : 0)) return fail(LCM_ERR_CAPACITY, "%zu matches but the buffer holds %zu records", total, out ? cap : (size_t)0);
    total = 0;
    for (int p = 0; p < n_pairs; ++p) {
        offsets[p] = total;
        const int j = job_of[(size_t)p];
        if (j >= 0 && count[(size_t)p]) emit_ratio(fin + 4 * row0[(size_t)j], rows[live[(size_t)j].q], ratio, out + total);
        total += count[(size_t)p];
    }
    offsets[n_pairs] = total;
    return LCM_OK;
}

// scores[p] of every pair: live ones from the device, a pair with an empty side {0, 0xFFFFFFFF}.  stored: as in l2_match_pairs
int l2_score_pairs(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const lcm_pair_ref* pairs, int n_pairs,
                        double ratio, lcm_l2_score* scores, const L2Where* stored) {
    if (!h || n_frames < 0 || n_pairs < 0 || (!stored && n_frames > 0 && (!frames || !rows)) || (n_pairs > 0 && (!pairs || !scores)))
        return fail(LCM_ERR_INVALID_ARG, "bad argument");
    int rc = l2_check_knn(h, ratio); if (rc) return rc;
    if (!stored) { rc = check_frames(frames, rows, n_frames); if (rc) return rc; }
    std::vector<L2Pair> live;
    std::vector<int> job_of;
    rc = l2_read_pairs(pairs, (size_t)n_pairs, rows, n_frames, live, job_of); if (rc) return rc;
    rc = set_device(h); if (rc) return rc;
    const lcm_l2_score* rec = nullptr;
    rc = l2_counts(h, stored, frames, rows, n_frames, live, ratio, &rec); if (rc) return rc;
    for (int p = 0; p < n_pairs; ++p) scores[p] = job_of[(size_t)p] >= 0 ? rec[job_of[(size_t)p]] : lcm_l2_score{0u, NONE};
    return LCM_OK;
}

}  // namespace lcm

namespace {

int knn2_pair_l2_impl(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt, int32_t* train_idx, float* dist,
                      uint32_t* dist_sq, int* n_neighbours) {
    if (!h || nq < 0 || nt < 0) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (n_neighbours) *n_neighbours = 0;
    int rc = lcm::l2_check_knn(h, 0.0); if (rc) return rc;
    rc = lcm::l2_check_rows(nq); if (rc) return rc;
    rc = lcm::l2_check_rows(nt); if (rc) return rc;
    if (nq == 0 || nt == 0) return LCM_OK;
    if (!query || !train || !train_idx || !dist) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    const uint8_t* frames[2] = {query, train};
    const int rows[2] = {nq, nt};
    const uint32_t* fin = nullptr;
    L2Run run;
    rc = l2_run(h, nullptr, frames, rows, 2, {L2Pair{0, 1}}, run, &fin); if (rc) return rc;
    for (size_t i = 0; i < (size_t)nq; ++i)
        for (int k = 0; k < 2; ++k) {
            const uint32_t D = fin[4 * i + 2 * k], idx = fin[4 * i + 2 * k + 1];
            const bool none = idx == NONE;
            train_idx[2 * i + k] = none ? -1 : (int32_t)idx;
            dist[2 * i + k] = none ? std::numeric_limits<float>::infinity() : dist_of(D);
            if (dist_sq) dist_sq[2 * i + k] = none ? NONE : D;
        }
    if (n_neighbours) *n_neighbours = std::min(nt, 2);
    return LCM_OK;
}

int match_features_ratio_l2_impl(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt, double ratio,
                                 lcm_dmatch* out, int* n_out) {
    if (!h || nq < 0 || nt < 0 || !n_out) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    int rc = lcm::l2_check_knn(h, ratio); if (rc) return rc;
    rc = lcm::l2_check_rows(nq); if (rc) return rc;
    rc = lcm::l2_check_rows(nt); if (rc) return rc;
    if (nq == 0 || nt == 0) return LCM_OK;
    if (!query || !train || !out) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    const uint8_t* frames[2] = {query, train};
    const int rows[2] = {nq, nt};
    const uint32_t* fin = nullptr;
    L2Run run;
    rc = l2_run(h, nullptr, frames, rows, 2, {L2Pair{0, 1}}, run, &fin); if (rc) return rc;
    *n_out = (int)emit_ratio(fin, nq, ratio, out);
    return LCM_OK;
}

// src/main.cpp:1375-1388 in one call: the admissible (curr, past) pairs are scored, the verdict and the compaction run
// here over the 8-byte records (a pair is millions of distances: the record count is tiny beside the kernel's work).
int loop_search_ratio_l2_impl(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const uint8_t* skip,
                              int loop_gap, const lcm_ratio_loop_params* rp_in, lcm_loop_candidate* out, size_t cap, size_t* n_out,
                              size_t* n_pairs_out) {
    if (!h || n_frames < 0 || !n_out || (n_frames > 0 && (!frames || !rows))) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    if (n_pairs_out) *n_pairs_out = 0;
    if (loop_gap < 1) return fail(LCM_ERR_INVALID_ARG, "loop_gap must be >= 1");
    lcm_ratio_loop_params rp;
    int rc = lcm::ratio_loop_params_checked(rp_in, &rp); if (rc) return rc;
    rc = lcm::l2_check_knn(h, rp.ratio); if (rc) return rc;
    rc = check_frames(frames, rows, n_frames); if (rc) return rc;
    rc = set_device(h); if (rc) return rc;
    // the store's plan over the call's matrices: its runs' records, run after run, are the live pairs in (curr, past) order
    std::vector<lcm::L2StoreCurr> currs;                  // q_tile: not the plan's business here, the count run lays the matrices out
    for (int curr = loop_gap; curr < n_frames; ++curr)
        if (!(skip && skip[curr]) && rows[curr] >= rp.min_rows) currs.push_back({curr, 0, rows[curr], curr - loop_gap});     // :1377, :1382
    lcm::L2StorePlan pl;
    rc = lcm::l2_refused(lcm::l2_store_plan(rows, (size_t)n_frames, currs, skip, rp.min_rows, pl)); if (rc) return rc;
    std::vector<L2Pair> live;
    for (size_t u = 0; u < currs.size(); ++u)
        for (uint32_t k = 0; pl.run_of[u] != (size_t)-1 && k < pl.runs[pl.run_of[u]].n_past; ++k) live.push_back(L2Pair{currs[u].id, (int)pl.live[k]});
    const lcm_l2_score* rec = nullptr;
    rc = l2_counts(h, nullptr, frames, rows, n_frames, live, rp.ratio, &rec); if (rc) return rc;
    return lcm::l2_candidates_out(pl, rows, (size_t)n_frames, currs, rec, rp.min_matches, out, cap, n_out, n_pairs_out);
}

int l2_ratio_test_device_impl(lcm_handle* h, const uint32_t* d1, const uint32_t* d2, size_t n, double ratio, uint8_t* pass) {
    if (!h || (n > 0 && (!d1 || !d2 || !pass))) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (std::isnan(ratio) || ratio < 0.0) return fail(LCM_ERR_INVALID_ARG, "ratio must be a number >= 0");
    if (n > ((size_t)1 << 31)) return fail(LCM_ERR_CAPACITY, "at most 2^31 pairs per call");
    for (size_t i = 0; i < n; ++i)
        if (d1[i] > lcm::L2_MAX_DSQ || d2[i] > lcm::L2_MAX_DSQ)
            return fail(LCM_ERR_INVALID_ARG, "pair %zu: a squared distance of 128 bytes is at most %u", i, lcm::L2_MAX_DSQ);
    if (n == 0) return LCM_OK;
    int rc = set_device(h); if (rc) return rc;
    auto& s = h->l2;
    rc = ensure_dev(s.d_diag, s.d_diag_n, 2 * n + (n + 3) / 4); if (rc) return rc;       // [d1 | d2 | pass]
    uint8_t* d_pass = reinterpret_cast<uint8_t*>(s.d_diag + 2 * n);
    HIP_TRY(hipMemcpyAsync(s.d_diag, d1, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(s.d_diag + n, d2, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    const hipError_t e = lcm::launch_l2_ratio_test(s.d_diag, s.d_diag + n, n, ratio, d_pass, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "ratio test kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(pass, d_pass, n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return LCM_OK;
}

}  // namespace

extern "C" {

int lcm_sift_pack_f32(const float* rows, int n, uint8_t* out) {
    if (n < 0 || (n > 0 && (!rows || !out))) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    const size_t total = (size_t)n * LCM_SIFT_BYTES;
    for (size_t i = 0; i < total; ++i) {
        const float v = rows[i];
        if (!(v >= 0.0f && v <= 255.0f) || v != std::floor(v))
            return fail(LCM_ERR_INVALID_ARG, "element %zu of row %zu is not an integer in [0, 255]: these are not OpenCV SIFT descriptors",
                        i % LCM_SIFT_BYTES, i / LCM_SIFT_BYTES);
    }
    for (size_t i = 0; i < total; ++i) out[i] = (uint8_t)rows[i];
    return LCM_OK;
}
int lcm_knn2_pair_l2(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt, int32_t* train_idx, float* dist,
                     uint32_t* dist_sq, int* n_neighbours) {
    return guarded([&] { return knn2_pair_l2_impl(h, query, nq, train, nt, train_idx, dist, dist_sq, n_neighbours); });
}
int lcm_match_features_ratio_l2(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt, double ratio,
                                lcm_dmatch* out, int* n_out) {
    return guarded([&] { return match_features_ratio_l2_impl(h, query, nq, train, nt, ratio, out, n_out); });
}
int lcm_match_pairs_ratio_l2(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const lcm_pair_ref* pairs,
                             int n_pairs, double ratio, lcm_dmatch* out, size_t cap, size_t* offsets) {
    return guarded([&] { return lcm::l2_match_pairs(h, frames, rows, n_frames, pairs, n_pairs, ratio, out, cap, offsets, nullptr); });
}
int lcm_score_pairs_ratio_l2(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const lcm_pair_ref* pairs,
                             int n_pairs, double ratio, lcm_l2_score* scores) {
    return guarded([&] { return lcm::l2_score_pairs(h, frames, rows, n_frames, pairs, n_pairs, ratio, scores, nullptr); });
}
int lcm_loop_search_ratio_l2(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const uint8_t* skip,
                             int loop_gap, const lcm_ratio_loop_params* rp, lcm_loop_candidate* out, size_t cap, size_t* n_out,
                             size_t* n_pairs_out) {
    return guarded([&] { return loop_search_ratio_l2_impl(h, frames, rows, n_frames, skip, loop_gap, rp, out, cap, n_out, n_pairs_out); });
}
int lcm_l2_ratio_test_device(lcm_handle* h, const uint32_t* d1, const uint32_t* d2, size_t n, double ratio, uint8_t* pass) {
    return guarded([&] { return l2_ratio_test_device_impl(h, d1, d2, n, ratio, pass); });
}

}  // extern "C"
