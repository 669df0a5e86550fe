// lcm_l2.cpp — pair mode on SIFT rows (128 uint8, L2): knnMatch(k = 2) + Lowe's ratio test as the reference runs them on
// cv::SIFT descriptors (src/main.cpp:497-504, :509-534, :1154, :1375-1388).  The kernels are lcm_l2.hip's; this file
// lays the matrices out in the tile space, plans the (query chunk x train segment) items, turns the shipped integer
// squared distances into OpenCV's float distances (sqrtf, correctly rounded on the host) and runs the ratio test in IEEE
// double.  The loop search's form (lcm_score_pairs_ratio_l2, lcm_loop_search_ratio_l2) wants the survivor COUNT per pair
// only: lcm_l2_count.hip scores a pair's whole train matrix in one workgroup per query chunk and decides on the device, so
// 8 bytes per pair come back.  Part of liblcm_hip.so's host side (C ABI in include/lcm.h); shared state and helpers:
// lcm_internal.h.
#include "lcm_internal.h"

#include <cmath>
#include <limits>

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;      // D / index of a neighbour that does not exist
constexpr int TILE = lcm::L2_TILE_ROWS, SEG = lcm::L2_SEG_ROWS, ROW = LCM_SIFT_BYTES;
static_assert(LCM_SIFT_BYTES == lcm::L2_ROW_BYTES, "row size");

struct L2Pair { int q, t; };                // positions into the call's matrices, both sides non-empty

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

// Uploads every matrix once, packs, scores every pair, folds, rescans: (D1, idx1, D2, idx2) per query row of pair p at
// (*fin)[4 * (row0[p] + r)], in pinned host memory that stays valid until the next L2 call on this handle.
int l2_run(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const std::vector<L2Pair>& pairs,
           const uint32_t** fin, std::vector<size_t>& row0) {
    int rc = set_device(h); if (rc) return rc;
    const size_t P = pairs.size();
    row0.assign(P + 1, 0);
    *fin = nullptr;
    if (P == 0) return LCM_OK;

    std::vector<uint32_t> tile0, tile_meta;
    tile_space(rows, n_frames, tile0, tile_meta);
    const size_t n_tiles = tile_meta.size();

    // ---- items and jobs
    const int CH = pick_chunk_rows(pairs, rows);
    std::vector<lcm::L2Item> items;
    std::vector<lcm::L2Job> jobs(P);
    size_t total_rows = 0;
    int max_nq = 0;
    uint64_t distances = 0;
    for (size_t p = 0; p < P; ++p) {
        const int nq = rows[pairs[p].q], nt = rows[pairs[p].t];
        const int n_chunks = (nq + CH - 1) / CH, n_seg = (nt + SEG - 1) / SEG;
        const uint32_t qt = tile0[(size_t)pairs[p].q], tt = tile0[(size_t)pairs[p].t];
        if (items.size() + (size_t)n_chunks * (size_t)n_seg > 0x7FFFFFFFull || total_rows + (size_t)nq > 0x7FFFFFFFull)
            return fail(LCM_ERR_CAPACITY, "too many pairs for one call");
        jobs[p] = {qt, (uint32_t)nq, tt, (uint32_t)nt, (uint32_t)items.size(), (uint32_t)n_seg, (uint32_t)total_rows, 0};
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
    rc = ensure_dev(s.d_raw, s.d_raw_n, n_tiles * (size_t)lcm::L2_TILE_BYTES); if (rc) return rc;
    rc = ensure_dev(s.d_img, s.d_img_n, n_tiles * (size_t)lcm::L2_TILE_BYTES); if (rc) return rc;
    rc = ensure_dev(s.d_tw, s.d_tw_n, n_tiles * (size_t)TILE); if (rc) return rc;
    rc = ensure_dev(s.d_tab, s.d_tab_n, tab_bytes); if (rc) return rc;
    rc = ensure_dev(s.d_seg, s.d_seg_n, n_items * (size_t)CH); if (rc) return rc;
    rc = ensure_dev(s.d_fin, s.d_fin_n, total_rows); if (rc) return rc;
    rc = ensure_dev(s.d_flag, s.d_flag_n, total_rows); if (rc) return rc;
    rc = ensure_pinned(s.h_fin, s.h_fin_n, total_rows); if (rc) return rc;

    // The sources are pageable: they stay alive (and unchanged) until the synchronisation at the end of this function.
    for (int f = 0; f < n_frames; ++f)
        if (rows[f] > 0)
            HIP_TRY(hipMemcpyAsync(s.d_raw + (size_t)tile0[(size_t)f] * lcm::L2_TILE_BYTES, frames[f], (size_t)rows[f] * ROW,
                                   hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(s.d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, h->stream));

    const lcm::L2PackArgs pa{s.d_raw, reinterpret_cast<const uint32_t*>(s.d_tab), s.d_img, s.d_tw, (uint32_t)n_tiles};
    hipError_t e = lcm::launch_l2_pack(pa, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "pack kernel launch failed: %s", hipGetErrorString(e));
    const lcm::L2ScoreArgs sa{s.d_img, s.d_tw, reinterpret_cast<const lcm::L2Item*>(s.d_tab + off_items), s.d_seg, (uint32_t)CH};
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    e = lcm::launch_l2_score(sa, (uint32_t)n_items, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "score kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    h->info_pending = true;
    h->info.workgroups = (uint32_t)n_items; h->info.route = LCM_ROUTE_PLAIN; h->info.launches = 4;
    h->info.pairs = P; h->info.distances = distances; h->info.algo_bytes = 2 * n_tiles * (uint64_t)lcm::L2_TILE_BYTES + total_rows * 16;
    const lcm::L2FoldArgs fa{s.d_seg, (uint32_t)CH, reinterpret_cast<const lcm::L2Job*>(s.d_tab + off_jobs), s.d_fin,
                             reinterpret_cast<uint32_t*>(s.d_tab + off_counter), s.d_flag, (uint32_t)total_rows, s.d_raw, 0};
    e = lcm::launch_l2_fold(fa, (uint32_t)P, (uint32_t)max_nq, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "fold kernel launch failed: %s", hipGetErrorString(e));
    e = lcm::launch_l2_rescan(fa, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "rescan kernel launch failed: %s", hipGetErrorString(e));
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

int match_pairs_ratio_l2_impl(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const lcm_pair_ref* pairs,
                              int n_pairs, double ratio, lcm_dmatch* out, size_t cap, size_t* offsets) {
    if (!h || n_frames < 0 || n_pairs < 0 || !offsets || (n_frames > 0 && (!frames || !rows)) || (n_pairs > 0 && !pairs))
        return fail(LCM_ERR_INVALID_ARG, "bad argument");
    offsets[0] = 0;
    int rc = check_knn(h, ratio); if (rc) return rc;
    for (int f = 0; f < n_frames; ++f) {
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
    rc = l2_run(h, frames, rows, n_frames, live, &fin, row0); if (rc) return rc;
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
int pick_count_chunk_rows(const std::vector<L2Pair>& pairs, const int* rows) {
    if (const char* e = getenv("LCM_TUNE_L2_COUNT_CHUNK")) { const int v = atoi(e); if (v == 128 || v == 256) return v; }
    size_t items256 = 0;
    for (const L2Pair& p : pairs) items256 += (size_t)((rows[p.q] + 255) / 256);
    return items256 < 1024 ? 128 : 256;
}

// Uploads the matrices that a live pair names (once each), packs, counts: live[j]'s record -> (*rec)[j], in pinned host
// memory that stays valid until the next count call on this handle.  Both sides of every live pair are non-empty.
int l2_count_run(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const std::vector<L2Pair>& live,
                 double ratio, const lcm_l2_score** rec) {
    int rc = set_device(h); if (rc) return rc;
    *rec = nullptr;
    const size_t P = live.size();
    if (P == 0) return LCM_OK;
    if (P > 0x7FFFFFFFull) return fail(LCM_ERR_CAPACITY, "too many pairs for one call");

    std::vector<int> used_rows((size_t)n_frames, 0);            // a matrix in no live pair takes no room in the tile space
    for (const L2Pair& p : live) { used_rows[(size_t)p.q] = rows[p.q]; used_rows[(size_t)p.t] = rows[p.t]; }
    std::vector<uint32_t> tile0, tile_meta;
    tile_space(used_rows.data(), n_frames, tile0, tile_meta);
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
    rc = ensure_dev(s.d_raw, s.d_raw_n, n_tiles * (size_t)lcm::L2_TILE_BYTES); if (rc) return rc;
    rc = ensure_dev(s.d_img, s.d_img_n, n_tiles * (size_t)lcm::L2_TILE_BYTES); if (rc) return rc;
    rc = ensure_dev(s.d_tw, s.d_tw_n, n_tiles * (size_t)TILE); if (rc) return rc;
    rc = ensure_dev(s.d_tab, s.d_tab_n, tab_bytes); if (rc) return rc;
    rc = ensure_dev(s.d_score, s.d_score_n, P); if (rc) return rc;
    rc = ensure_pinned(s.h_score, s.h_score_n, P); if (rc) return rc;

    // The sources are pageable: they stay alive (and unchanged) until the synchronisation at the end of this function.
    for (int f = 0; f < n_frames; ++f)
        if (used_rows[(size_t)f] > 0)
            HIP_TRY(hipMemcpyAsync(s.d_raw + (size_t)tile0[(size_t)f] * lcm::L2_TILE_BYTES, frames[f], (size_t)rows[f] * ROW,
                                   hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(s.d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, h->stream));

    const lcm::L2PackArgs pa{s.d_raw, reinterpret_cast<const uint32_t*>(s.d_tab), s.d_img, s.d_tw, (uint32_t)n_tiles};
    hipError_t e = lcm::launch_l2_pack(pa, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "pack kernel launch failed: %s", hipGetErrorString(e));
    e = lcm::launch_l2_count_init(s.d_score, (uint32_t)P, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "count init kernel launch failed: %s", hipGetErrorString(e));
    const lcm::L2CountArgs ca{s.d_img, s.d_tw, reinterpret_cast<const lcm::L2CountItem*>(s.d_tab + off_items), s.d_score, ratio, (uint32_t)CH};
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    e = lcm::launch_l2_count(ca, (uint32_t)n_items, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "count kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    h->info_pending = true;
    h->info.workgroups = (uint32_t)n_items; h->info.route = LCM_ROUTE_PLAIN; h->info.launches = 3;
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
                   double ratio, lcm_l2_score* scores) {
    std::vector<L2Pair> live;
    for (const L2Pair& p : pairs)
        if (rows[p.q] > 0 && rows[p.t] > 0) live.push_back(p);
    const lcm_l2_score* rec = nullptr;
    const int rc = l2_count_run(h, frames, rows, n_frames, live, ratio, &rec); if (rc) return rc;
    size_t j = 0;
    for (size_t p = 0; p < pairs.size(); ++p)
        scores[p] = (rows[pairs[p].q] > 0 && rows[pairs[p].t] > 0) ? rec[j++] : lcm_l2_score{0u, NONE};
    return LCM_OK;
}

int score_pairs_ratio_l2_impl(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const lcm_pair_ref* pairs,
                              int n_pairs, double ratio, lcm_l2_score* scores) {
    if (!h || n_frames < 0 || n_pairs < 0 || (n_frames > 0 && (!frames || !rows)) || (n_pairs > 0 && (!pairs || !scores)))
        return fail(LCM_ERR_INVALID_ARG, "bad argument");
    int rc = check_knn(h, ratio); if (rc) return rc;
    rc = check_frames(frames, rows, n_frames); if (rc) return rc;
    std::vector<L2Pair> all((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        const int q = pairs[p].query_frame_id, t = pairs[p].train_frame_id;
        if (q < 0 || q >= n_frames || t < 0 || t >= n_frames) return fail(LCM_ERR_INVALID_ARG, "pair %d: position outside [0, %d)", p, n_frames);
        all[(size_t)p] = L2Pair{q, t};
    }
    return score_pairs_l2(h, frames, rows, n_frames, all, ratio, scores);
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
int lcm_l2_ratio_test_device(lcm_handle* h, const uint32_t* d1, const uint32_t* d2, size_t n, double ratio, uint8_t* pass) {
    return guarded([&] { return l2_ratio_test_device_impl(h, d1, d2, n, ratio, pass); });
}

}  // extern "C"
