// lcm_l2.cpp — pair mode on SIFT rows (128 uint8, L2): knnMatch(k = 2) + Lowe's ratio test as the reference runs them on
// cv::SIFT descriptors (src/main.cpp:497-504, :509-534, :1154, :1375-1388).  The kernels are lcm_l2.hip's; this file
// lays the matrices out in the tile space, plans the (query chunk x train segment) items, turns the shipped integer
// squared distances into OpenCV's float distances (sqrtf, correctly rounded on the host) and runs the ratio test in IEEE
// double.  The loop search's form (lcm_score_pairs_ratio_l2, lcm_loop_search_ratio_l2) wants the survivor COUNT per pair
// only: lcm_l2_count.hip scores a pair's whole train matrix in one workgroup per query chunk and decides on the device, so
// 8 bytes per pair come back.  The SIFT keyframe store (lcm_l2_db_*) keeps uploaded and packed matrices on the device and
// searches them from tables that grow with the frames (lcm_l2_store.hip); its list calls can hand the point records straight to
// the loop verification (lcm_epi_db_*, lcm_lo_db_*, lcm_pose_db_*: store_lists runs the call's lcm::VerifyPlan through
// lcm_verify.cpp's pipeline; the best loop is chosen on the host).  Part of liblcm_hip.so's host side (C ABI in include/lcm.h);
// shared state and helpers: lcm_internal.h.
#include "lcm_internal.h"

#include <cmath>
#include <limits>

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;      // D / index of a neighbour that does not exist
constexpr int TILE = lcm::L2_TILE_ROWS, SEG = lcm::L2_SEG_ROWS, ROW = LCM_SIFT_BYTES;
static_assert(LCM_SIFT_BYTES == lcm::L2_ROW_BYTES, "row size");

struct L2Pair { int q, t; };                // positions into the call's matrices, both sides non-empty
using L2Store = lcm_handle::L2Store;        // the SIFT keyframe store, below
using lcm::VerifyPlan;                      // the loop verification behind the store's list calls (lcm_verify.cpp)

// What every k = 2 call refuses (lcm_knn.cpp's rule)
int check_knn(const lcm_handle* h, double ratio) {
    if (h->params.cross_check != 0) return fail(LCM_ERR_INVALID_ARG, "k = 2 matching needs cross_check = 0 (BFMatcher: knn == 1 under crossCheck)");
    if (std::isnan(ratio) || ratio < 0.0) return fail(LCM_ERR_INVALID_ARG, "ratio must be a number >= 0");
    return LCM_OK;
}

int check_rows(int n) {
    if (n < 0) return fail(LCM_ERR_INVALID_ARG, "negative row count");
    if (n > MAX_FRAME_ROWS) return fail(LCM_ERR_CAPACITY, "a SIFT matrix holds at most %d rows", MAX_FRAME_ROWS);
    return LCM_OK;
}

// Query chunk of an item: 128 rows (one tile per wave: twice the workgroups, the latency shape) while the call has few
// items, else 256 (two tiles per wave share every train fragment: the throughput shape).  LCM_TUNE_L2_CHUNK = 128 | 256
// pins it (tools/l2_time.py measures both).
int pick_chunk_rows(const std::vector<L2Pair>& pairs, const int* rows) {
    if (const char* e = getenv("LCM_TUNE_L2_CHUNK")) { const int v = atoi(e); if (v == 128 || v == 256) return v; }
    size_t items256 = 0;
    for (const L2Pair& p : pairs) items256 += (size_t)((rows[p.q] + 255) / 256) * (size_t)((rows[p.t] + SEG - 1) / SEG);
    return items256 < 1024 ? 128 : 256;
}

// The tile space: matrix f starts at tile tile0[f]; tile_meta = k_l2_pack's word per tile
void tile_space(const int* rows, int n_frames, std::vector<uint32_t>& tile0, std::vector<uint32_t>& tile_meta) {
    tile0.assign((size_t)n_frames + 1, 0);
    tile_meta.clear();
    for (int f = 0; f < n_frames; ++f) {
        const uint32_t nt = (uint32_t)((rows[f] + TILE - 1) / TILE);
        tile0[(size_t)f + 1] = tile0[(size_t)f] + nt;
        for (uint32_t k = 0; k < nt; ++k) tile_meta.push_back((uint32_t)std::min(TILE, rows[f] - (int)k * TILE) | (k << 8));
    }
}

// What l2_run leaves behind when the lists are made on the device (lcm_l2_emit.hip): final_keys stays in h->l2.d_fin
struct L2OnDevice {
    const lcm::L2Job* d_jobs = nullptr;     // the call's job table on the device
    std::vector<uint32_t> first_block;      // per job: its first 256-row block (L2Job::reserved)
    size_t n_blocks = 0;
    int max_nq = 0;
    std::vector<uint8_t> tab;               // the uploaded tables (pageable): alive until the caller has waited for the stream
};

// Uploads every matrix once, packs, scores every pair, folds, rescans: (D1, idx1, D2, idx2) per query row of pair p at
// (*fin)[4 * (row0[p] + r)], in pinned host memory that stays valid until the next L2 call on this handle.
// db != NULL: the matrices are the store's slots (rows = db->rows): nothing is uploaded or packed, the items point into
// the store's arenas.
// dev != NULL (with db): final_keys is not downloaded and the stream is not waited for: the kernels are enqueued, *fin stays
// NULL and *dev says where the jobs are.
int l2_run(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const std::vector<L2Pair>& pairs,
           const uint32_t** fin, std::vector<size_t>& row0, const L2Store* db = nullptr, L2OnDevice* dev = nullptr) {
    int rc = set_device(h); if (rc) return rc;
    const size_t P = pairs.size();
    row0.assign(P + 1, 0);
    *fin = nullptr;
    if (P == 0) return LCM_OK;

    std::vector<uint32_t> tile0, tile_meta;
    if (db) tile0 = db->tile0;
    else tile_space(rows, n_frames, tile0, tile_meta);
    const size_t n_tiles = tile_meta.size();

    // ---- items and jobs
    const int CH = pick_chunk_rows(pairs, rows);
    std::vector<lcm::L2Item> items;
    std::vector<lcm::L2Job> jobs(P);
    size_t total_rows = 0, n_blocks = 0;
    int max_nq = 0;
    uint64_t distances = 0;
    for (size_t p = 0; p < P; ++p) {
        const int nq = rows[pairs[p].q], nt = rows[pairs[p].t];
        const int n_chunks = (nq + CH - 1) / CH, n_seg = (nt + SEG - 1) / SEG;
        const uint32_t qt = tile0[(size_t)pairs[p].q], tt = tile0[(size_t)pairs[p].t];
        if (items.size() + (size_t)n_chunks * (size_t)n_seg > 0x7FFFFFFFull || total_rows + (size_t)nq > 0x7FFFFFFFull)
            return fail(LCM_ERR_CAPACITY, "too many pairs for one call");
        jobs[p] = {qt, (uint32_t)nq, tt, (uint32_t)nt, (uint32_t)items.size(), (uint32_t)n_seg, (uint32_t)total_rows, (uint32_t)n_blocks};
        n_blocks += (size_t)((nq + 255) / 256);                   // at most total_rows: fits the 32 bits
        for (int c = 0; c < n_chunks; ++c)
            for (int g = 0; g < n_seg; ++g)
                items.push_back({qt + (uint32_t)(c * (CH / TILE)), (uint32_t)std::min(CH, nq - c * CH),
                                 tt + (uint32_t)(g * (SEG / TILE)), (uint32_t)std::min(SEG, nt - g * SEG)});
        row0[p] = total_rows;
        total_rows += (size_t)nq;
        max_nq = std::max(max_nq, nq);
        distances += (uint64_t)nq * (uint64_t)nt;
    }
    row0[P] = total_rows;
    const size_t n_items = items.size();

    // ---- device buffers; the tables go up as one block [tile_meta | items | jobs | counter]
    auto& s = h->l2;
    const size_t off_items = (n_tiles * sizeof(uint32_t) + 15) & ~(size_t)15;
    const size_t off_jobs = off_items + n_items * sizeof(lcm::L2Item);
    const size_t off_counter = off_jobs + P * sizeof(lcm::L2Job);
    const size_t tab_bytes = off_counter + 16;
    std::vector<uint8_t> tab(tab_bytes, 0);
    memcpy(tab.data(), tile_meta.data(), n_tiles * sizeof(uint32_t));
    memcpy(tab.data() + off_items, items.data(), n_items * sizeof(lcm::L2Item));
    memcpy(tab.data() + off_jobs, jobs.data(), P * sizeof(lcm::L2Job));
    if (!db) {
        rc = ensure_dev(s.d_raw, s.d_raw_n, n_tiles * (size_t)lcm::L2_TILE_BYTES); if (rc) return rc;
        rc = ensure_dev(s.d_img, s.d_img_n, n_tiles * (size_t)lcm::L2_TILE_BYTES); if (rc) return rc;
        rc = ensure_dev(s.d_tw, s.d_tw_n, n_tiles * (size_t)TILE); if (rc) return rc;
    }
    const uint8_t* d_raw = db ? db->d_raw : s.d_raw;
    const uint8_t* d_img = db ? db->d_img : s.d_img;
    const uint32_t* d_tw = db ? db->d_tw : s.d_tw;
    rc = ensure_dev(s.d_tab, s.d_tab_n, tab_bytes); if (rc) return rc;
    rc = ensure_dev(s.d_seg, s.d_seg_n, n_items * (size_t)CH); if (rc) return rc;
    rc = ensure_dev(s.d_fin, s.d_fin_n, total_rows); if (rc) return rc;
    rc = ensure_dev(s.d_flag, s.d_flag_n, total_rows); if (rc) return rc;
    if (!dev) { rc = ensure_pinned(s.h_fin, s.h_fin_n, total_rows); if (rc) return rc; }

    // The sources are pageable: they stay alive (and unchanged) until the synchronisation at the end of this function.
    for (int f = 0; f < n_frames && !db; ++f)
        if (rows[f] > 0)
            HIP_TRY(hipMemcpyAsync(s.d_raw + (size_t)tile0[(size_t)f] * lcm::L2_TILE_BYTES, frames[f], (size_t)rows[f] * ROW,
                                   hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(s.d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, h->stream));

    hipError_t e = hipSuccess;
    if (!db) {
        const lcm::L2PackArgs pa{s.d_raw, reinterpret_cast<const uint32_t*>(s.d_tab), s.d_img, s.d_tw, (uint32_t)n_tiles};
        e = lcm::launch_l2_pack(pa, h->stream);
        if (e != hipSuccess) return fail(LCM_ERR_HIP, "pack kernel launch failed: %s", hipGetErrorString(e));
    }
    const lcm::L2ScoreArgs sa{d_img, d_tw, reinterpret_cast<const lcm::L2Item*>(s.d_tab + off_items), s.d_seg, (uint32_t)CH};
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    e = lcm::launch_l2_score(sa, (uint32_t)n_items, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "score kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    h->info_pending = true;
    h->info.workgroups = (uint32_t)n_items; h->info.route = LCM_ROUTE_PLAIN; h->info.launches = db ? 3 : 4;
    h->info.pairs = P; h->info.distances = distances; h->info.algo_bytes = 2 * n_tiles * (uint64_t)lcm::L2_TILE_BYTES + total_rows * 16;
    const lcm::L2FoldArgs fa{s.d_seg, (uint32_t)CH, reinterpret_cast<const lcm::L2Job*>(s.d_tab + off_jobs), s.d_fin,
                             reinterpret_cast<uint32_t*>(s.d_tab + off_counter), s.d_flag, (uint32_t)total_rows, d_raw, 0};
    e = lcm::launch_l2_fold(fa, (uint32_t)P, (uint32_t)max_nq, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "fold kernel launch failed: %s", hipGetErrorString(e));
    e = lcm::launch_l2_rescan(fa, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "rescan kernel launch failed: %s", hipGetErrorString(e));
    if (dev) {
        dev->d_jobs = fa.jobs; dev->n_blocks = n_blocks; dev->max_nq = max_nq;
        dev->first_block.resize(P);
        for (size_t p = 0; p < P; ++p) dev->first_block[p] = jobs[p].reserved;
        dev->tab = std::move(tab);
        return LCM_OK;
    }
    HIP_TRY(hipMemcpyAsync(s.h_fin, s.d_fin, total_rows * sizeof(uint4), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *fin = reinterpret_cast<const uint32_t*>(s.h_fin);
    return LCM_OK;
}

inline float dist_of(uint32_t D) { return std::sqrt((float)D); }      // D < 2^24: the conversion is exact, sqrtf correctly rounded

// Lowe's ratio test over one pair's rows (src/main.cpp:524-531): survivors of `s1 < ratio * s2` in double; a row with
// fewer than two neighbours is dropped.  out == NULL: count only.
size_t emit_ratio(const uint32_t* fin, int nq, double ratio, lcm_dmatch* out) {
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

int knn2_pair_l2_impl(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt, int32_t* train_idx, float* dist,
                      uint32_t* dist_sq, int* n_neighbours) {
    if (!h || nq < 0 || nt < 0) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (n_neighbours) *n_neighbours = 0;
    int rc = check_knn(h, 0.0); if (rc) return rc;
    rc = check_rows(nq); if (rc) return rc;
    rc = check_rows(nt); if (rc) return rc;
    if (nq == 0 || nt == 0) return LCM_OK;
    if (!query || !train || !train_idx || !dist) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    const uint8_t* frames[2] = {query, train};
    const int rows[2] = {nq, nt};
    const uint32_t* fin = nullptr;
    std::vector<size_t> row0;
    rc = l2_run(h, frames, rows, 2, {L2Pair{0, 1}}, &fin, row0); if (rc) return rc;
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
    int rc = check_knn(h, ratio); if (rc) return rc;
    rc = check_rows(nq); if (rc) return rc;
    rc = check_rows(nt); if (rc) return rc;
    if (nq == 0 || nt == 0) return LCM_OK;
    if (!query || !train || !out) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    const uint8_t* frames[2] = {query, train};
    const int rows[2] = {nq, nt};
    const uint32_t* fin = nullptr;
    std::vector<size_t> row0;
    rc = l2_run(h, frames, rows, 2, {L2Pair{0, 1}}, &fin, row0); if (rc) return rc;
    *n_out = (int)emit_ratio(fin, nq, ratio, out);
    return LCM_OK;
}

// db != NULL: the matrices are the store's slots (frames unused, rows / n_frames the store's)
int match_pairs_ratio_l2_impl(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const lcm_pair_ref* pairs,
                              int n_pairs, double ratio, lcm_dmatch* out, size_t cap, size_t* offsets, const L2Store* db = nullptr) {
    if (!h || n_frames < 0 || n_pairs < 0 || !offsets || (!db && n_frames > 0 && (!frames || !rows)) || (n_pairs > 0 && !pairs))
        return fail(LCM_ERR_INVALID_ARG, "bad argument");
    offsets[0] = 0;
    int rc = check_knn(h, ratio); if (rc) return rc;
    for (int f = 0; f < n_frames && !db; ++f) {
        rc = check_rows(rows[f]); if (rc) return rc;
        if (rows[f] > 0 && !frames[f]) return fail(LCM_ERR_INVALID_ARG, "matrix %d is NULL", f);
    }
    std::vector<L2Pair> live;
    std::vector<int> job_of((size_t)n_pairs, -1);
    for (int p = 0; p < n_pairs; ++p) {
        const int q = pairs[p].query_frame_id, t = pairs[p].train_frame_id;
        if (q < 0 || q >= n_frames || t < 0 || t >= n_frames) return fail(LCM_ERR_INVALID_ARG, "pair %d: position outside [0, %d)", p, n_frames);
        if (rows[q] == 0 || rows[t] == 0) continue;
        job_of[(size_t)p] = (int)live.size();
        live.push_back(L2Pair{q, t});
    }
    const uint32_t* fin = nullptr;
    std::vector<size_t> row0;
    rc = l2_run(h, frames, rows, n_frames, live, &fin, row0, db); if (rc) return rc;
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

// ---- ratio-test counts per pair (lcm_l2_count.hip) ------------------------------------------------------------------------
// Query chunk of a count item: the rule of pick_chunk_rows on this kernel's items (one per query chunk of a pair, whatever
// the train matrix's size).  LCM_TUNE_L2_COUNT_CHUNK = 128 | 256 pins it (tools/l2_count_time.py measures both).
int count_chunk_rows(size_t items256) {      // items256: the call's items at 256 rows per chunk
    if (const char* e = getenv("LCM_TUNE_L2_COUNT_CHUNK")) { const int v = atoi(e); if (v == 128 || v == 256) return v; }
    return items256 < 1024 ? 128 : 256;
}
int pick_count_chunk_rows(const std::vector<L2Pair>& pairs, const int* rows) {
    size_t items256 = 0;
    for (const L2Pair& p : pairs) items256 += (size_t)((rows[p.q] + 255) / 256);
    return count_chunk_rows(items256);
}

// Uploads the matrices that a live pair names (once each), packs, counts: live[j]'s record -> (*rec)[j], in pinned host
// memory that stays valid until the next count call on this handle.  Both sides of every live pair are non-empty.
// db != NULL: the matrices are the store's slots, as in l2_run.
int l2_count_run(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const std::vector<L2Pair>& live,
                 double ratio, const lcm_l2_score** rec, const L2Store* db = nullptr) {
    int rc = set_device(h); if (rc) return rc;
    *rec = nullptr;
    const size_t P = live.size();
    if (P == 0) return LCM_OK;
    if (P > 0x7FFFFFFFull) return fail(LCM_ERR_CAPACITY, "too many pairs for one call");

    std::vector<int> used_rows((size_t)n_frames, 0);            // a matrix in no live pair takes no room in the tile space
    for (const L2Pair& p : live) { used_rows[(size_t)p.q] = rows[p.q]; used_rows[(size_t)p.t] = rows[p.t]; }
    std::vector<uint32_t> tile0, tile_meta;
    if (db) tile0 = db->tile0;
    else tile_space(used_rows.data(), n_frames, tile0, tile_meta);
    const size_t n_tiles = tile_meta.size();

    const int CH = pick_count_chunk_rows(live, rows);
    size_t n_items = 0;
    uint64_t distances = 0;
    for (const L2Pair& p : live) {
        n_items += (size_t)((rows[p.q] + CH - 1) / CH);
        distances += (uint64_t)rows[p.q] * (uint64_t)rows[p.t];
    }
    if (n_items > 0x7FFFFFFFull) return fail(LCM_ERR_CAPACITY, "too many pairs for one call");
    std::vector<lcm::L2CountItem> items;
    items.reserve(n_items);
    for (size_t j = 0; j < P; ++j) {
        const int nq = rows[live[j].q], nt = rows[live[j].t];
        const uint32_t qt = tile0[(size_t)live[j].q], tt = tile0[(size_t)live[j].t];
        for (int c = 0; c * CH < nq; ++c)
            items.push_back({qt + (uint32_t)(c * (CH / TILE)), (uint32_t)std::min(CH, nq - c * CH), tt, (uint32_t)nt, (uint32_t)j, {0, 0, 0}});
    }

    // ---- device buffers; the tables go up as one block [tile_meta | items]
    auto& s = h->l2;
    const size_t off_items = (n_tiles * sizeof(uint32_t) + 31) & ~(size_t)31;
    const size_t tab_bytes = off_items + n_items * sizeof(lcm::L2CountItem);
    std::vector<uint8_t> tab(tab_bytes, 0);
    memcpy(tab.data(), tile_meta.data(), n_tiles * sizeof(uint32_t));
    memcpy(tab.data() + off_items, items.data(), n_items * sizeof(lcm::L2CountItem));
    if (!db) {
        rc = ensure_dev(s.d_raw, s.d_raw_n, n_tiles * (size_t)lcm::L2_TILE_BYTES); if (rc) return rc;
        rc = ensure_dev(s.d_img, s.d_img_n, n_tiles * (size_t)lcm::L2_TILE_BYTES); if (rc) return rc;
        rc = ensure_dev(s.d_tw, s.d_tw_n, n_tiles * (size_t)TILE); if (rc) return rc;
    }
    rc = ensure_dev(s.d_tab, s.d_tab_n, tab_bytes); if (rc) return rc;
    rc = ensure_dev(s.d_score, s.d_score_n, P); if (rc) return rc;
    rc = ensure_pinned(s.h_score, s.h_score_n, P); if (rc) return rc;

    // The sources are pageable: they stay alive (and unchanged) until the synchronisation at the end of this function.
    for (int f = 0; f < n_frames && !db; ++f)
        if (used_rows[(size_t)f] > 0)
            HIP_TRY(hipMemcpyAsync(s.d_raw + (size_t)tile0[(size_t)f] * lcm::L2_TILE_BYTES, frames[f], (size_t)rows[f] * ROW,
                                   hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(s.d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, h->stream));

    hipError_t e = hipSuccess;
    if (!db) {
        const lcm::L2PackArgs pa{s.d_raw, reinterpret_cast<const uint32_t*>(s.d_tab), s.d_img, s.d_tw, (uint32_t)n_tiles};
        e = lcm::launch_l2_pack(pa, h->stream);
        if (e != hipSuccess) return fail(LCM_ERR_HIP, "pack kernel launch failed: %s", hipGetErrorString(e));
    }
    e = lcm::launch_l2_count_init(s.d_score, (uint32_t)P, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "count init kernel launch failed: %s", hipGetErrorString(e));
    const lcm::L2CountArgs ca{db ? db->d_img : s.d_img, db ? db->d_tw : s.d_tw, reinterpret_cast<const lcm::L2CountItem*>(s.d_tab + off_items), s.d_score, ratio, (uint32_t)CH};
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    e = lcm::launch_l2_count(ca, (uint32_t)n_items, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "count kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    h->info_pending = true;
    h->info.workgroups = (uint32_t)n_items; h->info.route = LCM_ROUTE_PLAIN; h->info.launches = db ? 2 : 3;
    h->info.pairs = P; h->info.distances = distances; h->info.algo_bytes = 2 * n_tiles * (uint64_t)lcm::L2_TILE_BYTES + P * sizeof(lcm_l2_score);
    HIP_TRY(hipMemcpyAsync(s.h_score, s.d_score, P * sizeof(lcm_l2_score), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *rec = s.h_score;
    return LCM_OK;
}

// What the list call and the count calls refuse alike about the matrices
int check_frames(const uint8_t* const* frames, const int* rows, int n_frames) {
    for (int f = 0; f < n_frames; ++f) {
        const int rc = check_rows(rows[f]); if (rc) return rc;
        if (rows[f] > 0 && !frames[f]) return fail(LCM_ERR_INVALID_ARG, "matrix %d is NULL", f);
    }
    return LCM_OK;
}

// scores[p] of every pair: live ones from the device, a pair with an empty side {0, 0xFFFFFFFF}
int score_pairs_l2(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const std::vector<L2Pair>& pairs,
                   double ratio, lcm_l2_score* scores, const L2Store* db = nullptr) {
    std::vector<L2Pair> live;
    for (const L2Pair& p : pairs)
        if (rows[p.q] > 0 && rows[p.t] > 0) live.push_back(p);
    const lcm_l2_score* rec = nullptr;
    const int rc = l2_count_run(h, frames, rows, n_frames, live, ratio, &rec, db); if (rc) return rc;
    size_t j = 0;
    for (size_t p = 0; p < pairs.size(); ++p)
        scores[p] = (rows[pairs[p].q] > 0 && rows[pairs[p].t] > 0) ? rec[j++] : lcm_l2_score{0u, NONE};
    return LCM_OK;
}

int score_pairs_ratio_l2_impl(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const lcm_pair_ref* pairs,
                              int n_pairs, double ratio, lcm_l2_score* scores, const L2Store* db = nullptr) {
    if (!h || n_frames < 0 || n_pairs < 0 || (!db && n_frames > 0 && (!frames || !rows)) || (n_pairs > 0 && (!pairs || !scores)))
        return fail(LCM_ERR_INVALID_ARG, "bad argument");
    int rc = check_knn(h, ratio); if (rc) return rc;
    if (!db) { rc = check_frames(frames, rows, n_frames); if (rc) return rc; }
    std::vector<L2Pair> all((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        const int q = pairs[p].query_frame_id, t = pairs[p].train_frame_id;
        if (q < 0 || q >= n_frames || t < 0 || t >= n_frames) return fail(LCM_ERR_INVALID_ARG, "pair %d: position outside [0, %d)", p, n_frames);
        all[(size_t)p] = L2Pair{q, t};
    }
    return score_pairs_l2(h, frames, rows, n_frames, all, ratio, scores, db);
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
    rc = check_knn(h, rp.ratio); if (rc) return rc;
    rc = check_frames(frames, rows, n_frames); if (rc) return rc;
    auto admitted = [&](int f) { return !(skip && skip[f]) && rows[f] >= rp.min_rows; };      // :1377 / :1381, :1382
    std::vector<L2Pair> pairs;
    for (int curr = loop_gap; curr < n_frames; ++curr) {
        if (!admitted(curr)) continue;
        for (int past = 0; past <= curr - loop_gap; ++past)
            if (admitted(past)) pairs.push_back(L2Pair{curr, past});
    }
    std::vector<lcm_l2_score> scores(pairs.size());
    rc = score_pairs_l2(h, frames, rows, n_frames, pairs, rp.ratio, scores.data()); if (rc) return rc;
    if (n_pairs_out) *n_pairs_out = pairs.size();
    size_t found = 0;
    for (const lcm_l2_score& s : scores) found += (long long)s.good_count >= (long long)rp.min_matches;    // :1388
    *n_out = found;
    if (found > (out ? cap : 0)) return fail(LCM_ERR_CAPACITY, "%zu loop candidates but room for %zu", found, out ? cap : (size_t)0);
    size_t k = 0;
    for (size_t p = 0; p < pairs.size(); ++p) {
        if ((long long)scores[p].good_count < (long long)rp.min_matches) continue;
        const int den = std::min(rows[pairs[p].q], rows[pairs[p].t]);
        out[k++] = lcm_loop_candidate{pairs[p].q, pairs[p].t, (int32_t)scores[p].good_count,
                                      den > 0 ? (double)scores[p].good_count / (double)den : 0.0};
    }
    return LCM_OK;
}

// ---- the SIFT keyframe store (include/lcm.h, lcm_l2_db_*) -------------------------------------------------------------------
// Three arenas in one tile space (lcm_kernels.h): slot f's frame occupies tiles [tile0[f], tile0[f + 1]), the tail from
// tile0[size] on is free (a host query of lcm_l2_db_detect_loops is staged there).  k_l2_pack writes all 32 rows of every tile
// it is given, image and words, so the pad rows of a frame's last tile are rewritten whatever a truncated frame left there
// (the padding trap); the raw pad rows keep old bytes, which nothing reads (k_l2_rescan walks rows < nt).  A fourth arena,
// 8 bytes per row, holds the keypoints of the frames that came with them (lcm_l2_db_append_kp); its pad rows keep old points,
// which nothing reads either (k_l2_emit gathers rows < nq and train indices < nt).

size_t tiles_of(int n) { return (size_t)((n + TILE - 1) / TILE); }

// Room for `need` tiles: the first allocation is exactly that, later ones double.  The old blocks are freed after the copy
// has been waited for.
int store_reserve(lcm_handle* h, size_t need) {
    L2Store& d = h->l2db;
    if (need <= d.cap_tiles) return LCM_OK;
    size_t cap = d.cap_tiles ? d.cap_tiles : need;
    while (cap < need) cap *= 2;
    uint8_t *raw = nullptr, *img = nullptr;
    uint32_t* tw = nullptr;
    uint2* pts = nullptr;                                       // grows with the others once it exists
    auto drop = [&] { (void)hipFree(raw); (void)hipFree(img); (void)hipFree(tw); (void)hipFree(pts); };
    hipError_t e = hipMalloc((void**)&raw, cap * (size_t)lcm::L2_TILE_BYTES);
    if (e == hipSuccess) e = hipMalloc((void**)&img, cap * (size_t)lcm::L2_TILE_BYTES);
    if (e == hipSuccess) e = hipMalloc((void**)&tw, cap * (size_t)TILE * sizeof(uint32_t));
    if (e == hipSuccess && d.d_pts) e = hipMalloc((void**)&pts, cap * (size_t)TILE * sizeof(uint2));
    if (e != hipSuccess) { drop(); return fail(e == hipErrorOutOfMemory ? LCM_ERR_OOM : LCM_ERR_HIP, "store arena of %zu tiles: %s", cap, hipGetErrorString(e)); }
    const size_t used = d.tile0.back();
    if (used) {
        e = hipMemcpyAsync(raw, d.d_raw, used * (size_t)lcm::L2_TILE_BYTES, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(img, d.d_img, used * (size_t)lcm::L2_TILE_BYTES, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(tw, d.d_tw, used * (size_t)TILE * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess && pts) e = hipMemcpyAsync(pts, d.d_pts, used * (size_t)TILE * sizeof(uint2), hipMemcpyDeviceToDevice, h->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { drop(); return fail(LCM_ERR_HIP, "store arena copy failed: %s", hipGetErrorString(e)); }
    (void)hipFree(d.d_raw); (void)hipFree(d.d_img); (void)hipFree(d.d_tw); (void)hipFree(d.d_pts);
    d.d_raw = raw; d.d_img = img; d.d_tw = tw; d.d_pts = pts; d.cap_tiles = cap;
    return LCM_OK;
}

// The points arena, created when the first frame with points arrives (after store_reserve: cap_tiles > 0) and sized to
// the store's capacity.  The frames stored so far have no points: nothing is copied.
int store_pts_arena(lcm_handle* h) {
    L2Store& d = h->l2db;
    if (d.d_pts) return LCM_OK;
    HIP_TRY(hipMalloc((void**)&d.d_pts, d.cap_tiles * (size_t)TILE * sizeof(uint2)));
    return LCM_OK;
}

// n points -> rows [first * 32, first * 32 + n) of the points arena, as bytes; enqueued (the caller waits)
int store_put_pts(lcm_handle* h, const float* pts, int n, size_t first) {
    int rc = store_pts_arena(h); if (rc) return rc;
    if (n > 0) HIP_TRY(hipMemcpyAsync(h->l2db.d_pts + first * TILE, pts, (size_t)n * sizeof(uint2), hipMemcpyHostToDevice, h->stream));
    return LCM_OK;
}

// n rows -> tiles [first, first + tiles_of(n)) of the arenas: upload + pack, enqueued on the stream (the caller waits).
// `meta` is the caller's: it is read by the copy until then.
int store_put(lcm_handle* h, const uint8_t* rows, int n, size_t first, std::vector<uint32_t>& meta) {
    L2Store& d = h->l2db;
    const size_t nt = tiles_of(n);
    if (nt == 0) return LCM_OK;
    meta.resize(nt);
    for (size_t k = 0; k < nt; ++k) meta[k] = (uint32_t)std::min(TILE, n - (int)k * TILE) | ((uint32_t)k << 8);
    int rc = ensure_dev(d.d_meta, d.d_meta_n, nt); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d.d_raw + first * lcm::L2_TILE_BYTES, rows, (size_t)n * ROW, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d.d_meta, meta.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    const lcm::L2PackArgs pa{d.d_raw + first * lcm::L2_TILE_BYTES, d.d_meta, d.d_img + first * lcm::L2_TILE_BYTES, d.d_tw + first * TILE, (uint32_t)nt};
    const hipError_t e = lcm::launch_l2_pack(pa, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "pack kernel launch failed: %s", hipGetErrorString(e));
    return LCM_OK;
}

// with_pts: lcm_l2_db_append_kp, `pts` = n x (x, y)
int l2_db_append_impl(lcm_handle* h, const uint8_t* rows, int n, int* slot, bool with_pts = false, const float* pts = nullptr) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    int rc = check_rows(n); if (rc) return rc;
    if (n > 0 && (!rows || (with_pts && !pts))) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    L2Store& d = h->l2db;
    if (d.rows.size() >= 0x7FFFFFFFull) return fail(LCM_ERR_CAPACITY, "too many stored frames");
    rc = set_device(h); if (rc) return rc;
    const size_t first = d.tile0.back(), n_slots = d.rows.size();
    rc = store_reserve(h, std::max<size_t>(first + tiles_of(n), 1)); if (rc) return rc;
    if (n_slots + 1 > d.d_frames_cap) {          // the frame table doubles too; it is rebuilt from the host's copy
        size_t cap = std::max<size_t>(d.d_frames_cap * 2, 64);
        std::vector<uint2> all(n_slots);
        for (size_t f = 0; f < n_slots; ++f) all[f] = make_uint2(d.tile0[f], (uint32_t)d.rows[f]);
        uint2* t = nullptr;
        HIP_TRY(hipMalloc((void**)&t, cap * sizeof(uint2)));
        hipError_t e = n_slots ? hipMemcpyAsync(t, all.data(), n_slots * sizeof(uint2), hipMemcpyHostToDevice, h->stream) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) { (void)hipFree(t); return fail(LCM_ERR_HIP, "frame table copy failed: %s", hipGetErrorString(e)); }
        (void)hipFree(d.d_frames);
        d.d_frames = t; d.d_frames_cap = cap;
    }
    std::vector<uint32_t> meta;
    rc = store_put(h, rows, n, first, meta); if (rc) return rc;
    if (with_pts) { rc = store_put_pts(h, pts, n, first); if (rc) return rc; }
    const uint2 entry = make_uint2((uint32_t)first, (uint32_t)n);
    HIP_TRY(hipMemcpyAsync(d.d_frames + n_slots, &entry, sizeof(entry), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));     // the caller's rows (pageable) have been consumed
    d.rows.push_back(n);
    d.tile0.push_back((uint32_t)(first + tiles_of(n)));
    d.has_pts.push_back(with_pts ? 1 : 0);
    if (slot) *slot = (int)n_slots;
    return LCM_OK;
}

int check_slot(const lcm_handle* h, int slot) {
    if (slot < 0 || (size_t)slot >= h->l2db.rows.size()) return fail(LCM_ERR_INVALID_ARG, "slot %d outside [0, %zu)", slot, h->l2db.rows.size());
    return LCM_OK;
}

int l2_db_read_impl(lcm_handle* h, int slot, uint8_t* out, int cap_rows) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    int rc = check_slot(h, slot); if (rc) return rc;
    const L2Store& d = h->l2db;
    const int n = d.rows[(size_t)slot];
    if (cap_rows < n) return fail(LCM_ERR_CAPACITY, "slot %d holds %d rows but the buffer %d", slot, n, cap_rows);
    if (n == 0) return LCM_OK;
    if (!out) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    rc = set_device(h); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, d.d_raw + (size_t)d.tile0[(size_t)slot] * lcm::L2_TILE_BYTES, (size_t)n * ROW, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return LCM_OK;
}

int l2_db_truncate_impl(lcm_handle* h, int n_frames) {
    if (!h || n_frames < 0) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    L2Store& d = h->l2db;
    if ((size_t)n_frames > d.rows.size()) return fail(LCM_ERR_INVALID_ARG, "cannot truncate %zu frames to %d", d.rows.size(), n_frames);
    d.rows.resize((size_t)n_frames);
    d.tile0.resize((size_t)n_frames + 1);
    d.has_pts.resize((size_t)n_frames);
    return LCM_OK;
}

int l2_db_read_kp_impl(lcm_handle* h, int slot, float* out, int cap_rows) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    int rc = check_slot(h, slot); if (rc) return rc;
    const L2Store& d = h->l2db;
    if (!d.has_pts[(size_t)slot]) return fail(LCM_ERR_INVALID_ARG, "slot %d was stored without points", slot);
    const int n = d.rows[(size_t)slot];
    if (cap_rows < n) return fail(LCM_ERR_CAPACITY, "slot %d holds %d rows but the buffer %d", slot, n, cap_rows);
    if (n == 0) return LCM_OK;
    if (!out) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    rc = set_device(h); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, d.d_pts + (size_t)d.tile0[(size_t)slot] * TILE, (size_t)n * sizeof(uint2), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return LCM_OK;
}

int l2_db_info_impl(lcm_handle* h, lcm_l2_db_info* out) {
    if (!h || !out) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    const L2Store& d = h->l2db;
    *out = lcm_l2_db_info{(int32_t)d.rows.size(), 0, d.tile0.back(), d.cap_tiles,
                          d.cap_tiles * (2 * (uint64_t)lcm::L2_TILE_BYTES + TILE * sizeof(uint32_t) + (d.d_pts ? TILE * sizeof(uint2) : 0)) +
                              d.d_frames_cap * sizeof(uint2),
                          d.last_table_bytes};
    return LCM_OK;
}

// One `curr` of a store search: the query matrix (tile, rows) and its admissible pasts = the admitted slots <= last_past
struct StoreCurr { int id; uint32_t q_tile; int q_rows; int last_past; };

// src/main.cpp:1375-1388 over the store, `currs` in ascending order.  A pair is (curr, admitted past slot <= last_past), in
// that order, as lcm_loop_search_ratio_l2 forms them; the pairs with two non-empty sides are scored by k_l2_count_store
// from [runs | live admitted slots], the others are {0, 0xFFFFFFFF} as there.  The verdict and the compaction run here over
// the 8-byte records.
int store_search(lcm_handle* h, const std::vector<StoreCurr>& currs, const uint8_t* skip, const lcm_ratio_loop_params& rp,
                 lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out) {
    L2Store& d = h->l2db;
    const size_t S = d.rows.size();
    // admitted[0..): every admitted slot, ascending; live_before[f] = admitted slots below f that have rows (the pair's record)
    std::vector<uint32_t> admitted, live;
    std::vector<uint32_t> adm_before(S + 1, 0), live_before(S + 1, 0);
    for (size_t f = 0; f < S; ++f) {
        const bool adm = !(skip && skip[f]) && d.rows[f] >= rp.min_rows;
        adm_before[f + 1] = adm_before[f] + (adm ? 1u : 0u);
        live_before[f + 1] = live_before[f] + (adm && d.rows[f] > 0 ? 1u : 0u);
        if (adm) admitted.push_back((uint32_t)f);
        if (adm && d.rows[f] > 0) live.push_back((uint32_t)f);
    }
    std::vector<lcm::L2StoreRun> runs;
    std::vector<size_t> run_of(currs.size(), (size_t)-1);
    size_t items256 = 0, n_pairs = 0;
    for (const StoreCurr& c : currs) {
        const size_t last = (size_t)std::min<long long>(c.last_past, (long long)S - 1) + 1;      // pasts are slots [0, last)
        if (c.last_past < 0) continue;
        n_pairs += adm_before[last];
        if (c.q_rows > 0) items256 += (size_t)live_before[last] * (size_t)((c.q_rows + 255) / 256);
    }
    const int CH = count_chunk_rows(items256);
    uint64_t n_wg = 0, n_rec = 0, distances = 0;
    std::vector<uint64_t> rows_before(S + 1, 0);              // rows of the live admitted slots below f
    for (size_t f = 0; f < S; ++f) rows_before[f + 1] = rows_before[f] + (live_before[f + 1] != live_before[f] ? (uint64_t)d.rows[f] : 0);
    for (size_t u = 0; u < currs.size(); ++u) {
        const StoreCurr& c = currs[u];
        if (c.last_past < 0 || c.q_rows <= 0) continue;
        const size_t last = (size_t)std::min<long long>(c.last_past, (long long)S - 1) + 1;
        const uint32_t np = live_before[last];
        if (np == 0) continue;                                   // no admitted past: no run, no record
        const uint32_t chunks = (uint32_t)((c.q_rows + CH - 1) / CH);
        if (n_wg + (uint64_t)np * chunks > 0x7FFFFFFFull || n_rec + np > 0x7FFFFFFFull) return fail(LCM_ERR_CAPACITY, "too many pairs for one call");
        run_of[u] = runs.size();
        runs.push_back({c.q_tile, (uint32_t)c.q_rows, chunks, (uint32_t)n_wg, (uint32_t)n_rec, np});
        n_wg += (uint64_t)np * chunks;
        n_rec += np;
        distances += (uint64_t)c.q_rows * rows_before[last];
    }

    const lcm_l2_score* rec = nullptr;
    d.last_table_bytes = 0;
    if (!runs.empty()) {
        auto& s = h->l2;
        const size_t off_past = runs.size() * sizeof(lcm::L2StoreRun);
        const size_t tab_bytes = off_past + live.size() * sizeof(uint32_t);
        std::vector<uint8_t> tab(tab_bytes);
        memcpy(tab.data(), runs.data(), off_past);
        memcpy(tab.data() + off_past, live.data(), live.size() * sizeof(uint32_t));
        int rc = ensure_dev(d.d_tab, d.d_tab_n, tab_bytes); if (rc) return rc;
        rc = ensure_dev(s.d_score, s.d_score_n, (size_t)n_rec); if (rc) return rc;
        rc = ensure_pinned(s.h_score, s.h_score_n, (size_t)n_rec); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(d.d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, h->stream));
        hipError_t e = lcm::launch_l2_count_init(s.d_score, (uint32_t)n_rec, h->stream);
        if (e != hipSuccess) return fail(LCM_ERR_HIP, "count init kernel launch failed: %s", hipGetErrorString(e));
        const lcm::L2StoreArgs sa{d.d_img, d.d_tw, reinterpret_cast<const lcm::L2StoreRun*>(d.d_tab),
                                  reinterpret_cast<const uint32_t*>(d.d_tab + off_past), d.d_frames, s.d_score, rp.ratio,
                                  (uint32_t)runs.size(), (uint32_t)CH};
        HIP_TRY(hipEventRecord(h->ev_start, h->stream));
        e = lcm::launch_l2_count_store(sa, (uint32_t)n_wg, h->stream);
        if (e != hipSuccess) return fail(LCM_ERR_HIP, "count kernel launch failed: %s", hipGetErrorString(e));
        HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
        h->info_pending = true;
        h->info.workgroups = (uint32_t)n_wg; h->info.route = LCM_ROUTE_PLAIN; h->info.launches = 2;
        h->info.pairs = n_rec; h->info.distances = distances; h->info.algo_bytes = tab_bytes + n_rec * sizeof(lcm_l2_score);
        HIP_TRY(hipMemcpyAsync(s.h_score, s.d_score, (size_t)n_rec * sizeof(lcm_l2_score), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        rec = s.h_score;
        d.last_table_bytes = tab_bytes;
    }

    if (n_pairs_out) *n_pairs_out = n_pairs;
    // two passes over the records in (curr, past) order: the count, then (if it fits) the candidates
    auto walk = [&](lcm_loop_candidate* dst) {
        size_t found = 0;
        for (size_t u = 0; u < currs.size(); ++u) {
            const StoreCurr& c = currs[u];
            if (c.last_past < 0) continue;
            const size_t last = (size_t)std::min<long long>(c.last_past, (long long)S - 1) + 1;
            const lcm_l2_score* r = run_of[u] == (size_t)-1 ? nullptr : rec + runs[run_of[u]].first_pair;
            for (uint32_t k = 0; k < adm_before[last]; ++k) {
                const uint32_t past = admitted[k];
                const lcm_l2_score sc = (r && d.rows[past] > 0) ? r[live_before[past]] : lcm_l2_score{0u, NONE};
                if ((long long)sc.good_count < (long long)rp.min_matches) continue;                  // :1388
                if (dst) {
                    const int den = std::min(c.q_rows, d.rows[past]);
                    dst[found] = lcm_loop_candidate{c.id, (int32_t)past, (int32_t)sc.good_count,
                                                    den > 0 ? (double)sc.good_count / (double)den : 0.0};
                }
                ++found;
            }
        }
        return found;
    };
    const size_t found = walk(nullptr);
    *n_out = found;
    if (found > (out ? cap : 0)) return fail(LCM_ERR_CAPACITY, "%zu loop candidates but room for %zu", found, out ? cap : (size_t)0);
    if (found) walk(out);
    return LCM_OK;
}

// what lcm_loop_search_ratio_l2 checks before it looks at a matrix
int store_search_args(lcm_handle* h, int loop_gap, const lcm_ratio_loop_params* rp_in, size_t* n_out, size_t* n_pairs_out,
                      lcm_ratio_loop_params* rp) {
    if (!h || !n_out) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    if (n_pairs_out) *n_pairs_out = 0;
    if (loop_gap < 1) return fail(LCM_ERR_INVALID_ARG, "loop_gap must be >= 1");
    int rc = lcm::ratio_loop_params_checked(rp_in, rp); if (rc) return rc;
    rc = check_knn(h, rp->ratio); if (rc) return rc;
    return set_device(h);
}

int l2_db_loop_search_impl(lcm_handle* h, const uint8_t* skip, int loop_gap, const lcm_ratio_loop_params* rp_in,
                           lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out) {
    lcm_ratio_loop_params rp;
    const int rc = store_search_args(h, loop_gap, rp_in, n_out, n_pairs_out, &rp); if (rc) return rc;
    const L2Store& d = h->l2db;
    std::vector<StoreCurr> currs;
    for (size_t curr = (size_t)loop_gap; curr < d.rows.size(); ++curr)
        if (!(skip && skip[curr]) && d.rows[curr] >= rp.min_rows)                                   // :1377, :1382
            currs.push_back({(int)curr, d.tile0[curr], d.rows[curr], (int)curr - loop_gap});
    return store_search(h, currs, skip, rp, out, cap, n_out, n_pairs_out);
}

int l2_db_detect_loops_impl(lcm_handle* h, int curr, const uint8_t* query, int nq, const uint8_t* skip, int loop_gap,
                            const lcm_ratio_loop_params* rp_in, lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out) {
    lcm_ratio_loop_params rp;
    int rc = store_search_args(h, loop_gap, rp_in, n_out, n_pairs_out, &rp); if (rc) return rc;
    L2Store& d = h->l2db;
    StoreCurr c{curr, 0, 0, 0};
    std::vector<uint32_t> meta;
    if (query) {
        rc = check_rows(nq); if (rc) return rc;
        const size_t first = d.tile0.back();
        rc = store_reserve(h, std::max<size_t>(first + tiles_of(nq), 1)); if (rc) return rc;
        rc = store_put(h, query, nq, first, meta); if (rc) return rc;      // `meta` and `query` live until store_search has waited
        c.q_tile = (uint32_t)first; c.q_rows = nq;
    } else {
        rc = check_slot(h, curr); if (rc) return rc;
        c.q_tile = d.tile0[(size_t)curr]; c.q_rows = d.rows[(size_t)curr];
    }
    const long long last = (long long)curr - loop_gap;
    c.last_past = (int)std::max<long long>(last, -1);
    std::vector<StoreCurr> currs;
    if (c.q_rows >= rp.min_rows) currs.push_back(c);                        // :1382
    rc = store_search(h, currs, skip, rp, out, cap, n_out, n_pairs_out);
    if (query && nq > 0) HIP_TRY(hipStreamSynchronize(h->stream));          // a search that launched nothing has not waited
    return rc;
}

// ---- lists and keypoints from the device (lcm_l2_emit.hip) -------------------------------------------------------------------
static_assert(sizeof(size_t) == sizeof(uint64_t) && sizeof(lcm_dmatch) == sizeof(uint4) && sizeof(lcm_point_pair) == sizeof(uint4), "record sizes");

// The lists of job_of.size() pairs over the store's tile space: rows[f] rows at tile d.tile0[f] (f == size: a host query
// staged in the free tail); live[job_of[p]] = pair p, -1 when a side is empty.  Score, fold, rescan, then the ratio test, the
// ordered compaction and the gather on the device; offsets (8 bytes per pair) come back first and decide about `cap`, then
// only the records do.  pts == NULL: no point pairs.
// plan != NULL (checked, with pts): the plan's stages (lcm_verify.cpp: the RANSAC, then the local optimisation and the pose
// recovery where wanted) run on the point records as soon as k_l2_emit has written them, pair p of the call seeded with p;
// their kernels count into `launches` and into the aux events' span.
int store_lists(lcm_handle* h, const int* rows, int n_frames, const std::vector<L2Pair>& live, const std::vector<int>& job_of,
                double ratio, lcm_dmatch* out, lcm_point_pair* pts, size_t cap, size_t* offsets, const VerifyPlan* plan = nullptr) {
    const size_t n_pairs = job_of.size();
    if (live.empty()) {
        std::fill(offsets, offsets + n_pairs + 1, (size_t)0);
        if (plan) lcm::verify_empty(*plan, n_pairs);
        return LCM_OK;
    }
    L2Store& d = h->l2db;
    if (pts && !d.d_pts) return fail(LCM_ERR_INVALID_ARG, "the store holds no points");
    const uint32_t* fin = nullptr;
    std::vector<size_t> row0;
    L2OnDevice dv;
    int rc = l2_run(h, nullptr, rows, n_frames, live, &fin, row0, &d, &dv); if (rc) return rc;
    const size_t P = live.size(), total_rows = row0[P];

    // [first block of the first live pair at or after p, p <= n_pairs | survivors per block, + their total]
    std::vector<uint32_t> pair_block(n_pairs + 1);
    uint32_t next = (uint32_t)dv.n_blocks;
    pair_block[n_pairs] = next;
    for (size_t p = n_pairs; p-- > 0;) {
        if (job_of[p] >= 0) next = dv.first_block[(size_t)job_of[p]];
        pair_block[p] = next;
    }
    auto& s = h->l2;
    rc = ensure_dev(s.d_blocks, s.d_blocks_n, n_pairs + 1 + dv.n_blocks + 1); if (rc) return rc;
    rc = ensure_dev(s.d_offsets, s.d_offsets_n, n_pairs + 1); if (rc) return rc;
    uint32_t* d_blocks = s.d_blocks + n_pairs + 1;
    HIP_TRY(hipMemcpyAsync(s.d_blocks, pair_block.data(), (n_pairs + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    lcm::L2EmitArgs ea{s.d_fin, dv.d_jobs, d_blocks, nullptr, nullptr, nullptr, ratio, 0, 0};
    uint32_t slices = 0;
    rc = lcm::pair_slices(P, &slices); if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev_aux_start, h->stream));
    hipError_t e = lcm::launch_l2_emit_count(ea, (uint32_t)P, (uint32_t)dv.max_nq, h->stream);
    if (e == hipSuccess) e = lcm::launch_block_scan(d_blocks, (uint32_t)dv.n_blocks, d_blocks + dv.n_blocks, h->stream);
    if (e == hipSuccess) e = lcm::launch_l2_emit_offsets(d_blocks, s.d_blocks, s.d_offsets, (uint32_t)(n_pairs + 1), h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "list count kernels: launch failed: %s", hipGetErrorString(e));
    h->info.launches += slices + 2;
    HIP_TRY(hipMemcpyAsync(offsets, s.d_offsets, (n_pairs + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));       // also: l2_run's tables and pair_block (pageable) have been consumed
    const size_t total = offsets[n_pairs];
    h->info.algo_bytes += 2 * total_rows * 16 + (n_pairs + 1) * 8 + total * (pts ? 48 : 16);
    if (total > total_rows) return fail(LCM_ERR_HIP, "list count %zu exceeds the %zu query rows", total, total_rows);
    if (total > (out ? cap : 0)) {
        HIP_TRY(hipEventRecord(h->ev_aux_stop, h->stream));
        h->aux_pending = true;
        return fail(LCM_ERR_CAPACITY, "%zu matches but the buffer holds %zu records", total, out ? cap : (size_t)0);
    }
    if (total) {
        rc = ensure_dev(s.d_rec, s.d_rec_n, total); if (rc) return rc;
        if (pts) { rc = ensure_dev(s.d_rec_pts, s.d_rec_pts_n, total); if (rc) return rc; }
        ea.out = s.d_rec; ea.n_out = (uint32_t)total;
        if (pts) { ea.pts = d.d_pts; ea.out_pts = s.d_rec_pts; }
        e = lcm::launch_l2_emit(ea, (uint32_t)P, (uint32_t)dv.max_nq, h->stream);
        if (e != hipSuccess) return fail(LCM_ERR_HIP, "list kernel launch failed: %s", hipGetErrorString(e));
        h->info.launches += slices;
    }
    if (plan) {                                     // a pair's records are at most its query rows: they fit the packed key
        uint32_t max_n = 0, launches = 0;
        for (size_t p = 0; p < n_pairs; ++p) max_n = std::max(max_n, (uint32_t)(offsets[p + 1] - offsets[p]));
        rc = lcm::verify_enqueue(h, *plan, s.d_rec_pts, s.d_offsets, n_pairs, max_n, total, &launches); if (rc) return rc;
        h->info.launches += launches;
    }
    HIP_TRY(hipEventRecord(h->ev_aux_stop, h->stream));
    h->aux_pending = true;
    if (total) {
        HIP_TRY(hipMemcpyAsync(out, s.d_rec, total * sizeof(uint4), hipMemcpyDeviceToHost, h->stream));
        if (pts) HIP_TRY(hipMemcpyAsync(pts, s.d_rec_pts, total * sizeof(uint4), hipMemcpyDeviceToHost, h->stream));
    }
    if (plan) { rc = lcm::verify_download(h, *plan, n_pairs, total); if (rc) return rc; }
    if (total || plan) HIP_TRY(hipStreamSynchronize(h->stream));
    return LCM_OK;
}

// what a list call with a plan refuses before anything else of its own: bad RANSAC parameters, a missing buffer
int plan_checked(const VerifyPlan& plan, const lcm_point_pair* pts, size_t n_outputs) {
    const char* what = lcm::verify_plan_problem(plan, pts, n_outputs);
    return what ? fail(LCM_ERR_INVALID_ARG, "%s", what) : LCM_OK;
}

// `slot` is named by a list call that wants points: its rows must have theirs
int check_slot_pts(const L2Store& d, int slot) {
    if (d.rows[(size_t)slot] > 0 && !d.has_pts[(size_t)slot]) return fail(LCM_ERR_INVALID_ARG, "slot %d was stored without points", slot);
    return LCM_OK;
}

int l2_db_match_points_impl(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio, lcm_dmatch* out, lcm_point_pair* pts,
                            size_t cap, size_t* offsets, const VerifyPlan* plan = nullptr) {
    if (!h || n_pairs < 0 || !offsets || (n_pairs > 0 && !slots)) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (plan) { const int rc = plan_checked(*plan, pts, (size_t)n_pairs); if (rc) return rc; }
    offsets[0] = 0;
    int rc = check_knn(h, ratio); if (rc) return rc;
    const L2Store& d = h->l2db;
    const int S = (int)d.rows.size();
    std::vector<L2Pair> live;
    std::vector<int> job_of((size_t)n_pairs, -1);
    for (int p = 0; p < n_pairs; ++p) {
        const int q = slots[p].query_frame_id, t = slots[p].train_frame_id;
        if (q < 0 || q >= S || t < 0 || t >= S) return fail(LCM_ERR_INVALID_ARG, "pair %d: position outside [0, %d)", p, S);
        if (pts) {
            rc = check_slot_pts(d, q); if (rc) return rc;
            rc = check_slot_pts(d, t); if (rc) return rc;
        }
        if (d.rows[(size_t)q] == 0 || d.rows[(size_t)t] == 0) continue;
        job_of[(size_t)p] = (int)live.size();
        live.push_back(L2Pair{q, t});
    }
    return store_lists(h, d.rows.data(), S, live, job_of, ratio, out, pts, cap, offsets, plan);
}

int l2_db_detect_loops_points_impl(lcm_handle* h, int curr, const uint8_t* query, const float* query_pts, int nq, const uint8_t* skip,
                                   int loop_gap, const lcm_ratio_loop_params* rp_in, lcm_loop_candidate* cands, size_t cand_cap,
                                   size_t* n_cands, size_t* n_pairs_out, lcm_dmatch* out, lcm_point_pair* pts, size_t cap, size_t* offsets,
                                   const VerifyPlan* plan = nullptr) {
    if (!offsets) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (plan) {
        if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
        const int r = plan_checked(*plan, pts, cand_cap); if (r) return r;
    }
    lcm_ratio_loop_params rp;
    int rc = store_search_args(h, loop_gap, rp_in, n_cands, n_pairs_out, &rp); if (rc) return rc;
    offsets[0] = 0;
    L2Store& d = h->l2db;
    const int S = (int)d.rows.size();
    StoreCurr c{curr, 0, 0, 0};
    std::vector<uint32_t> meta;
    if (query) {
        rc = check_rows(nq); if (rc) return rc;
        if (pts && !query_pts) return fail(LCM_ERR_INVALID_ARG, "point pairs are wanted but the query has no points");
    } else {
        rc = check_slot(h, curr); if (rc) return rc;
        if (pts) { rc = check_slot_pts(d, curr); if (rc) return rc; }
        c.q_tile = d.tile0[(size_t)curr]; c.q_rows = d.rows[(size_t)curr];
    }
    // everything from the staging on: whatever happens, the caller's rows and points have been consumed on return
    auto body = [&]() -> int {
        if (query) {
            const size_t first = d.tile0.back();
            int r = store_reserve(h, std::max<size_t>(first + tiles_of(nq), 1)); if (r) return r;
            r = store_put(h, query, nq, first, meta); if (r) return r;
            if (query_pts) { r = store_put_pts(h, query_pts, nq, first); if (r) return r; }
            c.q_tile = (uint32_t)first; c.q_rows = nq;
        }
        c.last_past = (int)std::max<long long>((long long)curr - loop_gap, -1);
        std::vector<StoreCurr> currs;
        if (c.q_rows >= rp.min_rows) currs.push_back(c);                        // :1382
        int r = store_search(h, currs, skip, rp, cands, cand_cap, n_cands, n_pairs_out); if (r) return r;
        // the candidates' lists: query = position S of the extended row table (the staged rows) or the slot `curr`
        std::vector<int> rows_ext(d.rows);
        rows_ext.push_back(query ? nq : 0);
        const int qpos = query ? S : curr;
        std::vector<L2Pair> live;
        std::vector<int> job_of(*n_cands, -1);
        for (size_t k = 0; k < *n_cands; ++k) {
            const int t = cands[k].matched_frame_id;
            if (pts) { r = check_slot_pts(d, t); if (r) return r; }
            if (rows_ext[(size_t)qpos] == 0 || d.rows[(size_t)t] == 0) continue;
            job_of[k] = (int)live.size();
            live.push_back(L2Pair{qpos, t});
        }
        return store_lists(h, rows_ext.data(), S + 1, live, job_of, rp.ratio, out, pts, cap, offsets, plan);
    };
    rc = body();
    if (query && nq > 0) {
        const hipError_t e = hipStreamSynchronize(h->stream);                   // a path that launched nothing has not waited
        if (e != hipSuccess && rc == LCM_OK) return fail(LCM_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    }
    return rc;
}

// lcm_{pose,lo}_db_verify_pairs: the stages' parameters are checked before anything else (the pose's, then the optimisation's)
int db_verify_pairs(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio, lcm_dmatch* out, lcm_point_pair* pts, size_t cap,
                    size_t* offsets, VerifyPlan* plan, const lcm_lo_params* lp, const lcm_pose_params* pp) {
    const int rc = lcm::verify_params_checked(plan, lp, pp); if (rc) return rc;
    return l2_db_match_points_impl(h, slots, n_pairs, ratio, out, pts, cap, offsets, plan);
}

// lcm_{pose,lo}_db_detect_loops: the same, then `best`; the best loop among the verified candidates is chosen on the host
int db_detect_best(lcm_handle* h, int curr, const uint8_t* query, const float* query_pts, int nq, const uint8_t* skip, int loop_gap,
                   const lcm_ratio_loop_params* rp, lcm_loop_candidate* cands, size_t cand_cap, size_t* n_cands, size_t* n_pairs_out,
                   lcm_dmatch* out, lcm_point_pair* pts, size_t cap, size_t* offsets, VerifyPlan* plan, const lcm_lo_params* lp,
                   const lcm_pose_params* pp, int floor_inliers, int* best) {
    int rc = lcm::verify_params_checked(plan, lp, pp); if (rc) return rc;
    if (!best) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    rc = l2_db_detect_loops_points_impl(h, curr, query, query_pts, nq, skip, loop_gap, rp, cands, cand_cap, n_cands, n_pairs_out, out, pts,
                                        cap, offsets, plan);
    if (rc) return rc;
    *best = lcm::pose_best(plan->results, plan->pose_results, *n_cands, plan->ep, &plan->pp, floor_inliers);      // src/main.cpp:1403-1418
    return LCM_OK;
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
    return guarded([&] { return match_pairs_ratio_l2_impl(h, frames, rows, n_frames, pairs, n_pairs, ratio, out, cap, offsets); });
}
int lcm_score_pairs_ratio_l2(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const lcm_pair_ref* pairs,
                             int n_pairs, double ratio, lcm_l2_score* scores) {
    return guarded([&] { return score_pairs_ratio_l2_impl(h, frames, rows, n_frames, pairs, n_pairs, ratio, scores); });
}
int lcm_loop_search_ratio_l2(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const uint8_t* skip,
                             int loop_gap, const lcm_ratio_loop_params* rp, lcm_loop_candidate* out, size_t cap, size_t* n_out,
                             size_t* n_pairs_out) {
    return guarded([&] { return loop_search_ratio_l2_impl(h, frames, rows, n_frames, skip, loop_gap, rp, out, cap, n_out, n_pairs_out); });
}
int lcm_l2_db_append(lcm_handle* h, const uint8_t* rows, int n, int* slot) {
    return guarded([&] { return l2_db_append_impl(h, rows, n, slot); });
}
int lcm_l2_db_size(lcm_handle* h) { return h ? (int)h->l2db.rows.size() : 0; }
int lcm_l2_db_rows(lcm_handle* h, int slot, int* n) {
    if (!h || !n) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    const int rc = check_slot(h, slot); if (rc) return rc;
    *n = h->l2db.rows[(size_t)slot];
    return LCM_OK;
}
int lcm_l2_db_read(lcm_handle* h, int slot, uint8_t* out, int cap_rows) {
    return guarded([&] { return l2_db_read_impl(h, slot, out, cap_rows); });
}
int lcm_l2_db_truncate(lcm_handle* h, int n_frames) { return guarded([&] { return l2_db_truncate_impl(h, n_frames); }); }
int lcm_l2_db_clear(lcm_handle* h) { return guarded([&] { return l2_db_truncate_impl(h, 0); }); }
int lcm_l2_db_info_read(lcm_handle* h, lcm_l2_db_info* out) { return l2_db_info_impl(h, out); }
int lcm_l2_db_score_pairs(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio, lcm_l2_score* scores) {
    return guarded([&] {
        if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
        return score_pairs_ratio_l2_impl(h, nullptr, h->l2db.rows.data(), (int)h->l2db.rows.size(), slots, n_pairs, ratio, scores, &h->l2db);
    });
}
int lcm_l2_db_match_pairs_ratio(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio, lcm_dmatch* out, size_t cap,
                                size_t* offsets) {
    return guarded([&] {
        if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
        return match_pairs_ratio_l2_impl(h, nullptr, h->l2db.rows.data(), (int)h->l2db.rows.size(), slots, n_pairs, ratio, out, cap, offsets,
                                         &h->l2db);
    });
}
int lcm_l2_db_loop_search(lcm_handle* h, const uint8_t* skip, int loop_gap, const lcm_ratio_loop_params* rp, lcm_loop_candidate* out,
                          size_t cap, size_t* n_out, size_t* n_pairs_out) {
    return guarded([&] { return l2_db_loop_search_impl(h, skip, loop_gap, rp, out, cap, n_out, n_pairs_out); });
}
int lcm_l2_db_detect_loops(lcm_handle* h, int curr, const uint8_t* query, int nq, const uint8_t* skip, int loop_gap,
                           const lcm_ratio_loop_params* rp, lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out) {
    return guarded([&] { return l2_db_detect_loops_impl(h, curr, query, nq, skip, loop_gap, rp, out, cap, n_out, n_pairs_out); });
}
int lcm_l2_db_append_kp(lcm_handle* h, const uint8_t* rows, const float* pts, int n, int* slot) {
    return guarded([&] { return l2_db_append_impl(h, rows, n, slot, true, pts); });
}
int lcm_l2_db_read_kp(lcm_handle* h, int slot, float* out, int cap_rows) {
    return guarded([&] { return l2_db_read_kp_impl(h, slot, out, cap_rows); });
}
int lcm_l2_db_match_points(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio, lcm_dmatch* out, lcm_point_pair* pts,
                           size_t cap, size_t* offsets) {
    return guarded([&] { return l2_db_match_points_impl(h, slots, n_pairs, ratio, out, pts, cap, offsets); });
}
int lcm_l2_db_detect_loops_points(lcm_handle* h, int curr, const uint8_t* query, const float* query_pts, int nq, const uint8_t* skip,
                                  int loop_gap, const lcm_ratio_loop_params* rp, lcm_loop_candidate* cands, size_t cand_cap,
                                  size_t* n_cands, size_t* n_pairs_out, lcm_dmatch* out, lcm_point_pair* pts, size_t cap, size_t* offsets) {
    return guarded([&] {
        return l2_db_detect_loops_points_impl(h, curr, query, query_pts, nq, skip, loop_gap, rp, cands, cand_cap, n_cands, n_pairs_out, out,
                                              pts, cap, offsets);
    });
}
int lcm_epi_db_verify_pairs(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio, const lcm_epi_params* ep,
                            lcm_epi_result* results, lcm_dmatch* out, lcm_point_pair* pts, uint8_t* mask, size_t cap, size_t* offsets) {
    return guarded([&] {
        const VerifyPlan w{ep, false, false, results, mask};
        return l2_db_match_points_impl(h, slots, n_pairs, ratio, out, pts, cap, offsets, &w);
    });
}
int lcm_epi_db_detect_loops(lcm_handle* h, int curr, const uint8_t* query, const float* query_pts, int nq, const uint8_t* skip,
                            int loop_gap, const lcm_ratio_loop_params* rp, const lcm_epi_params* ep, lcm_loop_candidate* cands,
                            size_t cand_cap, size_t* n_cands, size_t* n_pairs_out, lcm_epi_result* results, lcm_dmatch* out,
                            lcm_point_pair* pts, uint8_t* mask, size_t cap, size_t* offsets) {
    return guarded([&] {
        const VerifyPlan w{ep, false, false, results, mask};
        return l2_db_detect_loops_points_impl(h, curr, query, query_pts, nq, skip, loop_gap, rp, cands, cand_cap, n_cands, n_pairs_out, out,
                                              pts, cap, offsets, &w);
    });
}
int lcm_pose_db_verify_pairs(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio, const lcm_epi_params* ep,
                             const lcm_pose_params* pp, lcm_epi_result* results, lcm_pose_result* pose_results, lcm_dmatch* out,
                             lcm_point_pair* pts, uint8_t* mask, uint8_t* pose_mask, size_t cap, size_t* offsets) {
    return guarded([&] {
        VerifyPlan w{ep, false, true, results, mask, nullptr, pose_results, pose_mask};
        return db_verify_pairs(h, slots, n_pairs, ratio, out, pts, cap, offsets, &w, nullptr, pp);
    });
}
int lcm_pose_db_detect_loops(lcm_handle* h, int curr, const uint8_t* query, const float* query_pts, int nq, const uint8_t* skip,
                             int loop_gap, const lcm_ratio_loop_params* rp, const lcm_epi_params* ep, const lcm_pose_params* pp,
                             lcm_loop_candidate* cands, size_t cand_cap, size_t* n_cands, size_t* n_pairs_out, lcm_epi_result* results,
                             lcm_pose_result* pose_results, lcm_dmatch* out, lcm_point_pair* pts, uint8_t* mask, uint8_t* pose_mask,
                             size_t cap, size_t* offsets, int floor_inliers, int* best) {
    return guarded([&] {
        VerifyPlan w{ep, false, true, results, mask, nullptr, pose_results, pose_mask};
        return db_detect_best(h, curr, query, query_pts, nq, skip, loop_gap, rp, cands, cand_cap, n_cands, n_pairs_out, out, pts, cap, offsets,
                              &w, nullptr, pp, floor_inliers, best);
    });
}
int lcm_lo_db_verify_pairs(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio, const lcm_epi_params* ep,
                           const lcm_lo_params* lp, const lcm_pose_params* pp, lcm_epi_result* results, lcm_lo_info* info,
                           lcm_pose_result* pose_results, lcm_dmatch* out, lcm_point_pair* pts, uint8_t* mask, uint8_t* pose_mask,
                           size_t cap, size_t* offsets) {
    return guarded([&] {
        VerifyPlan w{ep, true, true, results, mask, info, pose_results, pose_mask};
        return db_verify_pairs(h, slots, n_pairs, ratio, out, pts, cap, offsets, &w, lp, pp);
    });
}
int lcm_lo_db_detect_loops(lcm_handle* h, int curr, const uint8_t* query, const float* query_pts, int nq, const uint8_t* skip,
                           int loop_gap, const lcm_ratio_loop_params* rp, const lcm_epi_params* ep, const lcm_lo_params* lp,
                           const lcm_pose_params* pp, lcm_loop_candidate* cands, size_t cand_cap, size_t* n_cands, size_t* n_pairs_out,
                           lcm_epi_result* results, lcm_lo_info* info, lcm_pose_result* pose_results, lcm_dmatch* out,
                           lcm_point_pair* pts, uint8_t* mask, uint8_t* pose_mask, size_t cap, size_t* offsets, int floor_inliers,
                           int* best) {
    return guarded([&] {
        VerifyPlan w{ep, true, true, results, mask, info, pose_results, pose_mask};
        return db_detect_best(h, curr, query, query_pts, nq, skip, loop_gap, rp, cands, cand_cap, n_cands, n_pairs_out, out, pts, cap, offsets,
                              &w, lp, pp, floor_inliers, best);
    });
}
int lcm_l2_ratio_test_device(lcm_handle* h, const uint32_t* d1, const uint32_t* d2, size_t n, double ratio, uint8_t* pass) {
    return guarded([&] { return l2_ratio_test_device_impl(h, d1, d2, n, ratio, pass); });
}

}  // extern "C"
