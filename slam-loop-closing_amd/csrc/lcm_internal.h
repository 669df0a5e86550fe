// lcm_internal.h — shared between the translation units of liblcm_hip.so's host side:
//   lcm_api.cpp        handle lifetime, parameters, the device database (append, snapshot), launch info, scratch helpers
//   lcm_pair.cpp       pair mode / match lists        lcm_online.cpp   online queries (single, micro-batch), detectLoops
//   lcm_bulk.cpp       bulk all-vs-all, fused loops   lcm_cross.cpp    cross_check scoring
//   lcm_mfma_host.cpp  opt-in matrix-core variants    lcm_group.cpp    multi-GPU group (RCCL)
//   lcm_knn.cpp        pair mode with k = 2 neighbours + Lowe's ratio test
//   lcm_ratio.cpp      bulk / online loop search scored with Lowe's ratio test
//   lcm_l2.cpp         pair mode on 128-byte SIFT rows under L2 (knnMatch(k = 2) + ratio test) and ratio-test counts per pair on
//                      host matrices; the staging and the runs behind both (planned in lcm_l2_host.h)
//   lcm_l2_db.cpp      the SIFT keyframe store (lcm_l2_db_*): arenas, searches, device-side lists, the loop verification's entry points
//   lcm_epi.cpp        essential-matrix RANSAC over the loop candidates' correspondences (lcm_epi_*)
//   lcm_pose.cpp       relative pose of the verified candidates and the best loop (lcm_pose_*)
//   lcm_lo.cpp         local optimisation of the RANSAC's best hypotheses (lcm_lo_*)
//   lcm_pgo.cpp        pose-graph Gauss-Newton correction of the closed loop (lcm_pgo_*)
//   lcm_ba.cpp         alternating bundle adjustment and outlier removal after the loop (lcm_ba_*)
//   lcm_map.cpp        the map before the loop: keyframe gates, triangulation, filters and merge (lcm_map_*)
//   lcm_sift.cpp       the front end: SIFT scale space, extrema and refinement (lcm_sift_*)
//   lcm_verify.cpp     the three as one staged pipeline over a VerifyPlan (lcm_verify_host.h); the store's and the host-list forms
// Not installed; the public surface is include/lcm.h.
#pragma once
#include "../../include/lcm.h"

#include <hip/hip_runtime.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "lcm_kernels.h"
#include "lcm_l2_host.h"
#include "lcm_verify_host.h"

namespace lcm {
// last error message of the calling thread (lcm_last_error()); `fail` formats it and returns `code`
std::string& last_error();
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
void set_last_error(const char* msg);   // for the host-class shim (lcs_host.cpp)
}  // namespace lcm

namespace {
using lcm::fail;

// Nothing may throw across the C boundary (include/lcm.h): every entry point that touches a std container runs inside
// this guard, which turns std::bad_alloc into LCM_ERR_OOM and anything else into LCM_ERR_HIP + message.
template <typename F>
int guarded(F&& f) noexcept {
    try { return f(); }
    catch (const std::bad_alloc&) { return fail(LCM_ERR_OOM, "host allocation failed (std::bad_alloc)"); }
    catch (const std::exception& e) { return fail(LCM_ERR_HIP, "unexpected C++ exception: %s", e.what()); }
    catch (...) { return fail(LCM_ERR_HIP, "unexpected C++ exception"); }
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? LCM_ERR_OOM : LCM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                \
    } while (0)

constexpr int ROW_PAD = 4;            // stored rows are padded to a multiple of 4 with copies of the last row
constexpr int MAX_FRAME_ROWS = 65535; // include/lcm.h: rows of one frame (the record's n_train is 16 bits); the arena stride reaches 65536
constexpr size_t ARENA_SLACK = 512;   // the kernel prefetches up to 4 rows past a frame's padded end
constexpr int DEFAULT_MAX_DESC = 2000;  // ORB nfeatures of the reference (README.md:114)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline int padded_rows(int n) { return round_up(n, ROW_PAD); }   // rows [n, round_up(n,4)) of a stored frame repeat row n-1
inline size_t up16(size_t v) { return (v + 15) / 16 * 16; }      // the next 16-byte boundary of an offset in a staging block
inline uint64_t mix(uint64_t h, uint64_t v) { return h ^ (v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2)); }

}  // namespace

namespace lcm {

struct FrameMeta {
    int32_t id;
    int32_t n;       // descriptor rows
    int32_t n_kp;    // keypoints (similarity denominator)
};

constexpr int QUERY_SLOTS = 4;    // online queries that may be in flight at once (lcm_query_submit / _collect)
constexpr int STAGE_BUFS = 2;
// A micro-batch of fewer pairs than this is scored in split mode (1024-row chunks at the top of the range): with the
// slots on separate streams, finer workgroups let the next launch fill in behind the draining one.  Measured with
// bench.py --mode stream (8 frames per batch): 2500 frames 2.81e12 (limit 12288) -> 2.86e12.
constexpr size_t ONLINE_SPLIT_MAX_PAIRS = 65536;

struct QuerySlot {                // everything one in-flight online query owns
    bool busy = false;
    int n_elig = 0, nq = 0, query_id = 0;
    uint64_t db_generation = 0;   // h->db_generation at submit: a clear / load in between invalidates the ticket
    int n_batch = 0;              // > 0: a micro-batch (lcm_query_submit_batch); n_elig = records of all its queries
    int bat_elig[lcm::MAX_QUERY_BATCH] = {0};
    uint8_t* h_query = nullptr;   size_t h_query_bytes = 0;    // pinned staging of the query rows
    lcm_score* h_scores = nullptr; size_t h_scores_n = 0;      // pinned landing zone of the score records
    uint8_t* d_query = nullptr;   size_t d_query_bytes = 0;
    lcm_score* d_scores = nullptr; size_t d_scores_n = 0;
    uint32_t* d_dist = nullptr;   size_t d_dist_n = 0;         // split mode: best distance per (pair, row)
    uint8_t* h_meta = nullptr;    size_t h_meta_bytes = 0;     // matrix-core variants: pinned [row counts | work items]
    uint8_t* d_meta = nullptr;    size_t d_meta_bytes = 0;
    hipEvent_t done = nullptr;
    hipEvent_t k0 = nullptr, k1 = nullptr;      // around this query's kernel(s): summed into the handle's online stats
    // The slot's own stream: consecutive online queries run on different streams, so the upload and the first
    // workgroups of query k + 1 overlap the draining tail of query k's launch (a launch of a few thousand workgroups
    // leaves the chip partly idle while its last ones finish).  `fence` orders the slot stream after everything
    // enqueued on the handle's stream before the submit.
    hipStream_t stream = nullptr;
    hipEvent_t fence = nullptr;
    uint64_t acc_pairs = 0, acc_distances = 0, acc_bytes = 0;
    uint32_t acc_launches = 0, acc_queries = 0;
};

struct PlanSig {         // everything a bulk plan is built from: a cached plan is reused only when ALL of it is unchanged
    uint64_t db_generation = 0;
    size_t n_db = 0;     // stored frames (appends only add slots, a clear / truncate / load bumps db_generation)
    int n_q = 0, gap = 0, q_stride = 0, item_slots = 0, pack_mode = 0;
    bool self = false;
    size_t scratch_words = 0;
    std::vector<int32_t> q_ids, q_counts;      // external query set only
    std::vector<uint32_t> q_frame_of;
    bool operator==(const PlanSig& o) const {
        return db_generation == o.db_generation && n_db == o.n_db && n_q == o.n_q && gap == o.gap && q_stride == o.q_stride &&
               item_slots == o.item_slots && pack_mode == o.pack_mode && self == o.self && scratch_words == o.scratch_words &&
               q_ids == o.q_ids && q_counts == o.q_counts && q_frame_of == o.q_frame_of;
    }
};

struct Plan {            // cached work list of one bulk call shape
    uint64_t key = 0;    // 0 = invalid (set by everything that changes the database or the parameters); else sig is compared
    PlanSig sig;
    std::vector<lcm::WorkItem> items;
    std::vector<size_t> offsets;    // per query frame, start of its run of pairs (n_q + 1)
    lcm::WorkItem* d_items = nullptr;
    size_t d_items_cap = 0;
    size_t n_pairs = 0;
    uint64_t distances = 0, algo_bytes = 0;
    int max_q_rows = 0;
    // PACKED form (lcm_kernels.h, ScoreArgs::pk_*): a chunk = one GROUP of query frames (laid end to end in a virtual row
    // space) x one RANGE of stored slots; `items` holds (column, slot run) items chunk by chunk and
    // d_pk_tab = [pair offsets (n_q + 1) | query row counts (n_q) | per group: vstart (n_pos + 1), qframe, elig, cidx |
    //             per chunk: local pair offsets (n_pos + 1)]
    struct PackedChunk { uint32_t item0, n_items, tab0, ptab0, n_pos, slot0, n_pairs; };
    bool packed = false;
    std::vector<PackedChunk> pk_chunks;
    uint32_t* d_pk_tab = nullptr;
    size_t d_pk_tab_n = 0;
    size_t pk_max_pairs = 0;        // largest chunk: sizes the per-row scratch (8 KB per pair)
    uint32_t pk_n_q = 0;
    uint32_t pk_col_rows = 2048;    // rows per column = rows per workgroup of the packed score kernel
    uint32_t pk_stride = 2048;      // scratch words per pair
};

}  // namespace lcm

namespace lcm { struct MapPair; struct MapTri; struct Point3; struct Observation; }    // lcm_map_device.h, lcm_geom_device.h

using lcm::FrameMeta;
using lcm::Plan;
using lcm::QuerySlot;

struct lcm_handle {
    lcm_params params;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t copy_stream = nullptr;
    // packed bulk search of more than one chunk: the chunks alternate between `stream` and `stream2` (and between the two
    // halves of the per-row scratch), so that the draining tail of one chunk's launch is filled by the next chunk's workgroups
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t db_ready = nullptr;     // last append landed (recorded on copy_stream)
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    hipEvent_t ev_aux_start = nullptr, ev_aux_stop = nullptr;   // the follow-up kernel of a call (k_loop_test, ...)
    bool aux_pending = false;
    // packed bulk search: one (start, stop) event pair around EVERY chunk's fold kernel; aux_kernel_ms is their sum
    std::vector<hipEvent_t> fold_ev;
    size_t fold_ev_used = 0;
    int variant = 0;
    int tune_item_slots = 0;           // 0 = automatic (pick_chunk)
    int tune_online_split = -1;        // -1 = automatic (enqueue_query)
    int tune_pair_upload_kernel = 1;   // pair mode, latency shape: staging block uploaded by a kernel (1) or by hipMemcpyAsync (0)
    int tune_pair_host_fold = 1;       // ... and the fold kernel writes into pinned host memory (1) or into device memory + a copy (0)
    int tune_online_streams = 1;       // 1 = every query slot runs on its own stream, 0 = all on the handle's stream
    // packed route: 4-byte words of per-row scratch per chunk.  _cfg is what LCM_TUNE_PACKED_SCRATCH_MB asked for (default
    // 1 GiB); the effective size is halved when the allocation fails and goes back to _cfg at the next plan rebuild.
    size_t pk_scratch_cfg_words = (size_t)1 << 28;
    size_t pk_scratch_words = (size_t)1 << 28;
    bool pk_oom_retry = false;
    int tune_packed = -1;              // -1 = automatic (bulk plan: when it saves lane slots), 0 = never, 1 = always

    // database arena
    uint8_t* d_rows = nullptr;
    int32_t* d_counts = nullptr;
    int cap_frames = 0;
    int stride_rows = 0;               // rows per frame slot (multiple of ROW_PAD)
    std::vector<FrameMeta> frames;
    bool pending_copy = false;
    bool db_ready_recorded = false;    // db_ready has been recorded at least once (slot streams wait on it)

    // pinned staging ring for streaming appends
    uint8_t* h_stage[lcm::STAGE_BUFS] = {nullptr, nullptr};
    size_t h_stage_bytes = 0;
    hipEvent_t stage_done[lcm::STAGE_BUFS] = {nullptr, nullptr};
    int32_t* h_counts = nullptr;       // pinned mirror of d_counts (source of the 4-byte async copies)
    int h_counts_cap = 0;
    int stage_next = 0;

    // scratch for query uploads / pair mode / results
    uint32_t* d_keys = nullptr; size_t d_keys_n = 0;
    uint8_t* h_pair_stage = nullptr; size_t h_pair_stage_bytes = 0;   // pair mode: pinned [rows | items | descriptors]
    uint8_t* d_pair_stage = nullptr; size_t d_pair_stage_bytes = 0;
    uint32_t* h_final_keys = nullptr; size_t h_final_keys_n = 0;      // pair mode: pinned landing zone of the folded keys
    uint8_t* d_xq = nullptr; size_t d_xq_bytes = 0;                   // cross_check: padded copy of an external query set
    // opt-in MFMA variant (4): +1 / -1 int8 operand images of the database and of an external query set, scratch
    uint8_t* d_pm1 = nullptr; size_t d_pm1_bytes = 0; uint64_t pm1_stamp = 0; size_t pm1_frames = 0;   // frames expanded so far
    uint8_t* d_qpm1 = nullptr; size_t d_qpm1_bytes = 0;
    uint32_t* d_mdist = nullptr; size_t d_mdist_n = 0;
    uint8_t* d_mitems = nullptr; size_t d_mitems_bytes = 0;
    uint32_t* d_mmeta = nullptr; size_t d_mmeta_n = 0;
    lcm_score* d_bulk_scores = nullptr; size_t d_bulk_scores_n = 0;   // lcm_all_vs_all_loops: scores stay on the device
    size_t bulk_scores_valid = 0;                                     // records of the last fused call still in there
    int32_t* d_meta = nullptr; size_t d_meta_n = 0;
    lcm_loop_candidate* d_cands = nullptr; size_t d_cands_n = 0;

    QuerySlot qslots[lcm::QUERY_SLOTS];
    lcm_online_stats online{};         // totals over collected online queries (lcm_online_stats_read)
    uint64_t db_generation = 1;        // bumped whenever stored frames are dropped (lcm_db_clear / lcm_db_load)
    Plan plan;
    // lcm_all_vs_all_ratio / lcm_query_scores_ratio (lcm_ratio.cpp): a plan and buffers of their own.  The plan is always
    // in the plain form and is reused only when its whole signature compares equal, so nothing has to invalidate it and
    // it never meets `plan` (packed chunks, scratch): the two searches alternate freely on one handle.
    Plan ratio_plan;
    uint8_t* d_ratio_q = nullptr; size_t d_ratio_q_bytes = 0;          // the online call's query rows
    lcm_score* d_ratio_scores = nullptr; size_t d_ratio_scores_n = 0;  // ... and its records
    // pair mode on SIFT rows (lcm_l2.cpp, lcm_l2_db.cpp): raw rows, operand image and per-row words of the call's matrices in the tile
    // space, the tables, per-item keys, folded results (device + pinned landing zone), the rescan's flag list
    struct L2Scratch {
        uint8_t* d_raw = nullptr;  size_t d_raw_n = 0;
        uint8_t* d_img = nullptr;  size_t d_img_n = 0;
        uint32_t* d_tw = nullptr;  size_t d_tw_n = 0;
        uint8_t* d_tab = nullptr;  size_t d_tab_n = 0;
        uint2* d_seg = nullptr;    size_t d_seg_n = 0;
        uint4* d_fin = nullptr;    size_t d_fin_n = 0;
        uint2* d_flag = nullptr;   size_t d_flag_n = 0;
        uint4* h_fin = nullptr;    size_t h_fin_n = 0;
        // ... and of the count calls (lcm_score_pairs_ratio_l2): one record per live pair, device + pinned landing zone;
        // the diagnostic's [d1 | d2 | pass]
        uint2* d_score = nullptr;  size_t d_score_n = 0;
        lcm_l2_score* h_score = nullptr; size_t h_score_n = 0;
        uint32_t* d_diag = nullptr; size_t d_diag_n = 0;
        // ... and of the device-side lists (lcm_l2_emit.hip): [per-pair first block | block counts + total] as words, the
        // per-pair offsets, the records and their point pairs
        uint32_t* d_blocks = nullptr; size_t d_blocks_n = 0;
        uint64_t* d_offsets = nullptr; size_t d_offsets_n = 0;
        uint4* d_rec = nullptr;    size_t d_rec_n = 0;
        uint4* d_rec_pts = nullptr; size_t d_rec_pts_n = 0;
    } l2;
    // the SIFT keyframe store (lcm_l2_db_*, lcm_l2_db.cpp): three arenas in ONE tile space (lcm_kernels.h) with room for
    // cap_tiles tiles, slot f's frame at tile tile0[f] (tile0 has size + 1 entries: the last is the first free tile), the
    // device frame table {first tile, rows} per slot, and the tables of the last search.  A fourth arena in the same tile
    // space, d_pts (8 bytes per row: a keypoint's x, y as bits), exists from the first frame that arrives with points
    // (lcm_l2_db_append_kp, or a host query with points); has_pts[f] says whether slot f's rows have theirs.
    struct L2Store {
        uint8_t* d_raw = nullptr;  uint8_t* d_img = nullptr;  uint32_t* d_tw = nullptr;  size_t cap_tiles = 0;
        uint2* d_pts = nullptr;
        std::vector<uint8_t> has_pts;
        uint2* d_frames = nullptr; size_t d_frames_cap = 0;
        uint32_t* d_meta = nullptr; size_t d_meta_n = 0;       // k_l2_pack's tile words of the tiles being packed
        uint8_t* d_tab = nullptr;  size_t d_tab_n = 0;         // a search's [runs | admitted slots]
        std::vector<uint32_t> tile0{0};
        std::vector<int> rows;
        size_t last_table_bytes = 0;
    } l2db;
    // essential-matrix RANSAC (lcm_epi.cpp): a host call's points and offsets, the hypotheses (8 indices + 9 doubles each),
    // the per-pair best key, the seam's counts, the result records and the mask
    struct EpiScratch {
        uint4* d_pts = nullptr;       size_t d_pts_n = 0;
        uint64_t* d_off = nullptr;    size_t d_off_n = 0;
        int32_t* d_samples = nullptr; size_t d_samples_n = 0;
        double* d_E = nullptr;        size_t d_E_n = 0;
        uint32_t* d_best = nullptr;   size_t d_best_n = 0;
        uint32_t* d_counts = nullptr; size_t d_counts_n = 0;
        lcm_epi_result* d_res = nullptr; size_t d_res_n = 0;
        uint8_t* d_mask = nullptr;    size_t d_mask_n = 0;
    } epi;
    // relative-pose recovery (lcm_pose.cpp): a host call's matrices and input mask, the seam's candidates (36 + 12 doubles
    // per model), the result records and the output mask
    struct PoseScratch {
        double* d_E = nullptr;        size_t d_E_n = 0;
        uint8_t* d_mask_in = nullptr; size_t d_mask_in_n = 0;
        double* d_cand = nullptr;     size_t d_cand_n = 0;
        lcm_pose_result* d_res = nullptr; size_t d_res_n = 0;
        uint8_t* d_mask = nullptr;    size_t d_mask_n = 0;
    } pose;
    // local optimisation (lcm_lo.cpp): the seeds (64 per pair), the info records, and the seams' models and outputs
    struct LoScratch {
        int32_t* d_seeds = nullptr;   size_t d_seeds_n = 0;
        lcm_lo_info* d_info = nullptr; size_t d_info_n = 0;
        double* d_models = nullptr;   size_t d_models_n = 0;     // the refit seam: 64 x 9 in, 64 x 9 out
        int32_t* d_seam = nullptr;    size_t d_seam_n = 0;       // ... and 64 counts + 64 statuses
    } lo;
    // pose-graph correction (lcm_pgo.cpp): one graph's [poses | edges | table | valid | returned poses | state] as bytes, and
    // every array of doubles of a run (parameters, residuals, Jacobian, the blocks of the normal equations and of their factor)
    struct PgoScratch {
        uint8_t* d_in = nullptr;      size_t d_in_n = 0;
        double* d_work = nullptr;     size_t d_work_n = 0;
    } pgo;
    // bundle adjustment (lcm_ba.cpp): one map's [poses | points | observations | tables | valid] and everything the kernels write
    // behind it (element infos, mean errors, partial sums, flags, the step calls' seam) as bytes
    struct BaScratch {
        uint8_t* d_map = nullptr;     size_t d_map_n = 0;
    } ba;
    // the map before the loop (lcm_map.cpp): the per-pair plans, counts and medians, a host call's mask, the records' results, and
    // a merge's matches, tables ([table1 | table2 | winner]), block counts ([accepted + total | new + total]) and outputs
    struct MapScratch {
        lcm::MapPair* d_pairs = nullptr;   size_t d_pairs_n = 0;
        uint32_t* d_counts = nullptr;      size_t d_counts_n = 0;
        double* d_median = nullptr;        size_t d_median_n = 0;
        uint8_t* d_mask = nullptr;         size_t d_mask_n = 0;
        lcm::MapTri* d_tri = nullptr;      size_t d_tri_n = 0;
        uint8_t* d_status = nullptr;       size_t d_status_n = 0;
        uint4* d_matches = nullptr;        size_t d_matches_n = 0;
        int32_t* d_tab = nullptr;          size_t d_tab_n = 0;
        uint32_t* d_blocks = nullptr;      size_t d_blocks_n = 0;
        lcm::Point3* d_points = nullptr; size_t d_points_n = 0;
        lcm::Observation* d_obs = nullptr;      size_t d_obs_n = 0;
        uint8_t* d_status_out = nullptr;   size_t d_status_out_n = 0;
    } map;
    lcm_sift_space* sift_cached = nullptr;      // lcm_sift_detect_image's space (lcm_sift.cpp), made at its first call
    lcm_launch_info info{};
    bool info_pending = false;
};


namespace {

template <typename T>
int ensure_dev(T*& p, size_t& have, size_t need, size_t slack_bytes = 0) {
    if (need <= have && p) return LCM_OK;
    if (p) HIP_TRY(hipFree(p));
    p = nullptr; have = 0;
    size_t n = std::max<size_t>(need, 16);
    HIP_TRY(hipMalloc((void**)&p, n * sizeof(T) + slack_bytes));
    have = n;
    return LCM_OK;
}

template <typename T>
int ensure_pinned(T*& p, size_t& have, size_t need) {
    if (need <= have && p) return LCM_OK;
    if (p) HIP_TRY(hipHostFree(p));
    p = nullptr; have = 0;
    const size_t n = std::max<size_t>(need, 16);
    HIP_TRY(hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault));
    have = n;
    return LCM_OK;
}

// The host sequence of an on-device loop test (lcm::loop_test_device, lcm::ratio_loop_test_device), between the two aux
// events: count() enqueues the count + scan kernels, the count is read back, a too-small `cap` is refused (*n_found set)
// BEFORE anything proportional to the count is allocated, then emit(out, n) enqueues the kernel that writes the n
// candidates to h->d_cands.  Everything on h's stream; the stream is synchronised once, after the count.
template <typename Count, typename Emit>
int count_then_emit(lcm_handle* h, const uint32_t* d_counter, size_t cap, size_t* n_found, Count&& count, Emit&& emit) {
    HIP_TRY(hipEventRecord(h->ev_aux_start, h->stream));
    hipError_t e = count();
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "loop-test kernel launch failed: %s", hipGetErrorString(e));
    uint32_t found = 0;
    HIP_TRY(hipMemcpyAsync(&found, d_counter, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));          // also: the caller's metadata upload (pageable) has been consumed
    *n_found = found;
    if (found > cap) {
        HIP_TRY(hipEventRecord(h->ev_aux_stop, h->stream));
        h->aux_pending = true;
        return fail(LCM_ERR_CAPACITY, "%u loop candidates but room for %zu", found, cap);
    }
    if (found) {
        const int rc = ensure_dev(h->d_cands, h->d_cands_n, (size_t)found); if (rc) return rc;
        e = emit(h->d_cands, found);
        if (e != hipSuccess) return fail(LCM_ERR_HIP, "loop-test kernel launch failed: %s", hipGetErrorString(e));
    }
    HIP_TRY(hipEventRecord(h->ev_aux_stop, h->stream));
    h->aux_pending = true;
    return LCM_OK;
}

}  // namespace

namespace lcm {
// ---- lcm_api.cpp
int set_device(const lcm_handle* h);
int wait_db(lcm_handle* h);            // make the match stream see every append issued so far
int sync_online_streams(lcm_handle* h);   // host-wait for every query slot's own stream
int eligible_prefix(const lcm_handle* h, int query_id, int gap);   // eligible stored slots are a prefix: its length
int pick_chunk(const lcm_handle* h, size_t total_pairs);
int launch_and_time(lcm_handle* h, const ScoreArgs& a, uint32_t n_items, int max_q_rows, bool write_keys);
// snapshot file helpers (lcm_db_save / _load and their group forms share ONE format)
int snapshot_open(const char* path, std::vector<FrameMeta>& metas, uint32_t* real_max_rows, FILE** f_out);
bool snapshot_write_header(FILE* f, const std::vector<FrameMeta>& metas);
// ---- lcm_cross.cpp: cross_check scoring of "query c against stored slots [0, elig[c])", records in (query, slot) order
int cross_score_prefixes(lcm_handle* h, const uint8_t* d_qbase, const uint32_t* q_row0, const int* nq, const int* elig,
                         int n_q, lcm_score* d_scores, uint32_t* d_idx_sums);
// ---- lcm_mfma_host.cpp: opt-in matrix-core variants 4 / 5
int mfma_online(lcm_handle* h, QuerySlot& q, const uint32_t* d_q, int pitch_rows, int B, const int* nq, const int* elig);
int mfma_bulk(lcm_handle* h, bool self, const uint8_t* q_rows, const int32_t* d_q_counts, uint32_t q_pitch_rows,
              const uint32_t* q_frame_of, const int* nqv, int n_q, const std::vector<size_t>& offsets, lcm_score* d_scores,
              uint32_t* d_idx_sums);     // d_idx_sums non-NULL: the argmin form (keys + index checksums)
// ---- lcm_bulk.cpp
// Bulk search behind lcm_all_vs_all / lcm_all_vs_all_argmin.  q_frame_of (optional, n_q_frames entries): query frame c
// lives at index q_frame_of[c] of d_query_rows / d_query_counts instead of index c (the group's rank-major gathered
// query buffer).  h_query_counts (optional, host, indexed by c) spares the device read of the row counts.
// d_idx_sums non-NULL selects the argmin kernel.
int all_vs_all(lcm_handle* h, const void* d_query_rows, const int32_t* d_query_counts, const int32_t* q_ids,
               int n_q_frames, int q_stride_rows, void* d_scores, size_t scores_cap, size_t* n_pairs,
               size_t* pair_offsets, uint32_t* d_idx_sums, const uint32_t* q_frame_of, const int32_t* h_query_counts);
// Loop test + ordered compaction over a score array on h's device (lcm_all_vs_all_loops; a group's shard over its own records)
int loop_test_device(lcm_handle* h, const void* d_scores, size_t n_pairs, const uint32_t* offsets, int n_q,
                     const int32_t* q_ids, const int32_t* q_kp, int n_db, const int32_t* db_ids, const int32_t* db_kp,
                     size_t cap, size_t* n_found);
// ---- lcm_ratio.cpp
// Bulk search behind lcm_all_vs_all_ratio; q_frame_of / h_query_counts as in all_vs_all above (the group's shards).
int all_vs_all_ratio(lcm_handle* h, const void* d_query_rows, const int32_t* d_query_counts, const int32_t* q_ids,
                     int n_q_frames, int q_stride_rows, double ratio, void* d_scores, size_t scores_cap, size_t* n_pairs,
                     size_t* pair_offsets, const uint32_t* q_frame_of, const int32_t* h_query_counts);
// NULL -> the defaults; LCM_ERR_INVALID_ARG for a NaN or negative ratio, a negative min_rows or min_matches
int ratio_loop_params_checked(const lcm_ratio_loop_params* rp, lcm_ratio_loop_params* out);
// The reference's loop rule (src/main.cpp:1379-1388) + ordered compaction over a ratio score array on h's device: the twin
// of loop_test_device, with descriptor row counts of the query frames in place of keypoint counts (the stored frames'
// come from the records).  On LCM_OK the *n_found candidates are in h->d_cands.
int ratio_loop_test_device(lcm_handle* h, const void* d_scores, size_t n_pairs, const uint32_t* offsets, int n_q,
                           const int32_t* q_ids, const int32_t* q_rows, int n_db, const int32_t* db_ids,
                           const lcm_ratio_loop_params& rp, size_t cap, size_t* n_found);
// ---- lcm_pair.cpp: the pair mode's plumbing, shared with lcm_knn.cpp.  k = neighbours per query row: 1 (match) or 2
// (knnMatch(k = 2)); with k = 2 every key array holds 2 keys per query row (best, second; 0xFFFFFFFF = none).
// Row source: host rows (uploaded to scratch) or rows already on the device (a stored frame).
struct RowSrc {
    const uint8_t* host;
    const uint8_t* dev;
    int n;
};
// One matchFeatures job of a batch: query rows x train rows, both given as ROW INDICES into one query matrix and one
// train matrix on the device (the database arena, or this call's staging block).
struct PairJob { uint32_t q_row; int nq; uint32_t t_row; int nt; };
int run_pair_jobs(lcm_handle* h, const uint8_t* d_q_base, const uint8_t* d_t_base, bool q_in_stage, bool t_in_stage,
                  size_t stage_bytes, const std::vector<PairJob>& jobs, const uint32_t** keys_out, std::vector<size_t>& row0,
                  int k = 1);
int pair_keys(lcm_handle* h, RowSrc q, RowSrc t, std::vector<uint32_t>& keys_out, int cross, int k = 1);
int stored_src(lcm_handle* h, int frame_id, RowSrc* out, int* n_kp);    // device rows + row counts of a stored frame
// The jobs of a batch call (q_host != NULL: one host query frame, staged at the head of h_pair_stage, against the stored
// frames train_ids; else the stored pairs): job_of[p] = pair p's job, -1 when a side is empty.
int batch_jobs(lcm_handle* h, const uint8_t* q_host, int nq_host, const lcm_pair_ref* pairs, const int32_t* train_ids,
               int n_pairs, std::vector<PairJob>& jobs, std::vector<int>& job_of, size_t* stage_bytes);
// ---- lcm_l2.cpp: the SIFT matcher's checks, staging and runs, shared with lcm_l2_db.cpp (the plans: lcm_l2_host.h)
int l2_check_knn(const lcm_handle* h, double ratio);    // what every k = 2 call refuses (lcm_knn.cpp's rule)
int l2_check_rows(int n);                               // a SIFT matrix holds 0 .. 65535 rows
int l2_refused(const char* what);                       // a planner's answer: LCM_OK for NULL, else LCM_ERR_CAPACITY and the message
// Where a call's matrices are: raw rows, operand image and row words in one tile space, matrix f at tile tile0[f].  The store's
// slots (lcm_l2_db.cpp) are there already, packed when they were appended.  A host call's matrices (lcm_l2.cpp, call_where) go
// into the handle's scratch: tile_meta / n_tiles are the tiles to pack, frames / rows / n_frames the matrices to upload first
// (rows[f] == 0: none).  Every pointer is the caller's.
struct L2Where {
    const uint8_t* d_raw; const uint8_t* d_img; const uint32_t* d_tw; const uint32_t* tile0;
    const uint32_t* tile_meta = nullptr; size_t n_tiles = 0;
    const uint8_t* const* frames = nullptr; const int* rows = nullptr; int n_frames = 0;
};
// A list run: its plan; once enqueued, the job table on the device and the host table block, which is pageable and has to stay
// alive until the stream has been waited for
struct L2Run { L2RunPlan plan; const L2Job* d_jobs = nullptr; std::vector<uint8_t> tab; };
int l2_enqueue(lcm_handle* h, const L2Where& w, L2Run& run);                  // final_keys -> h->l2.d_fin, nothing waited for
int l2_count_run(lcm_handle* h, const L2Where& w, const L2CountPlan& pl, size_t n_pairs, double ratio, const lcm_l2_score** rec);
// lcm_match_pairs_ratio_l2 / lcm_score_pairs_ratio_l2; stored != NULL: over the store's slots (frames unused, rows / n_frames the store's)
int l2_match_pairs(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const lcm_pair_ref* pairs, int n_pairs,
                   double ratio, lcm_dmatch* out, size_t cap, size_t* offsets, const L2Where* stored);
int l2_score_pairs(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames, const lcm_pair_ref* pairs, int n_pairs,
                   double ratio, lcm_l2_score* scores, const L2Where* stored);
int l2_candidates_out(const L2StorePlan& pl, const int* rows, size_t S, const std::vector<L2StoreCurr>& currs, const lcm_l2_score* rec,
                      int min_matches, lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out);
// A caller's pair table over n_frames matrices -> live[job_of[p]] = pair p, job_of[p] = -1 when a side is empty.  Pair p's
// positions are range-checked, then extra(q, t) may refuse it (a status), before pair p + 1 is looked at.
struct L2NoCheck { int operator()(int, int) const { return LCM_OK; } };
template <typename Extra = L2NoCheck>
int l2_read_pairs(const lcm_pair_ref* pairs, size_t n_pairs, const int* rows, int n_frames, std::vector<L2Pair>& live,
                  std::vector<int>& job_of, Extra&& extra = Extra{}) {
    live.clear();
    job_of.assign(n_pairs, -1);
    for (size_t p = 0; p < n_pairs; ++p) {
        const int q = pairs[p].query_frame_id, t = pairs[p].train_frame_id;
        if (q < 0 || q >= n_frames || t < 0 || t >= n_frames) return fail(LCM_ERR_INVALID_ARG, "pair %d: position outside [0, %d)", (int)p, n_frames);
        if (const int rc = extra(q, t)) return rc;
        if (rows[q] == 0 || rows[t] == 0) continue;
        job_of[p] = (int)live.size();
        live.push_back(L2Pair{q, t});
    }
    return LCM_OK;
}
// ---- lcm_epi.cpp, lcm_lo.cpp, lcm_pose.cpp: the stages of the loop verification.  Every *_enqueue works on h's stream over
// n_pairs pairs whose records d_pts[d_off[p] .. d_off[p + 1]) are on the device (max_n = the longest pair, total =
// d_off[n_pairs]), sets *launches to the kernel launches it made and does not wait; every *_download enqueues the copies of
// the last *_enqueue's records to the host (the caller waits; a mask may be NULL).
// ep checked (LCM_ERR_INVALID_ARG and the message otherwise); lp / pp checked into *out, the defaults for NULL
int epi_params_checked(const lcm_epi_params* ep);
int lo_params_checked(const lcm_lo_params* lp, lcm_lo_params* out);
int pose_params_checked(const lcm_pose_params* pp, lcm_pose_params* out);
// k_epi_solve, k_epi_score, k_epi_mask: results -> h->epi.d_res, mask -> h->epi.d_mask; want_counts: every hypothesis's inlier
// count -> h->epi.d_counts as well (what lo_enqueue reads)
int epi_enqueue(lcm_handle* h, const uint4* d_pts, const uint64_t* d_off, size_t n_pairs, uint32_t max_n, size_t total,
                const lcm_epi_params& ep, uint32_t* launches, bool want_counts = false);
int epi_download(lcm_handle* h, size_t n_pairs, size_t total, lcm_epi_result* results, uint8_t* mask);
// A host call's records and offsets -> h->epi.d_pts / d_off, enqueued (the sources are pageable: the caller waits)
int epi_upload_points(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, size_t n_pairs, size_t total);
// k_lo_select, k_lo_refine behind an epi_enqueue(..., want_counts = true) over the same pairs: they read h->epi.d_E / d_counts
// and rewrite h->epi.d_res / d_mask where a refit is better; info -> h->lo.d_info
int lo_enqueue(lcm_handle* h, const uint4* d_pts, const uint64_t* d_off, size_t n_pairs, const lcm_epi_params& ep,
               const lcm_lo_params& lp, uint32_t* launches);
int lo_download(lcm_handle* h, size_t n_pairs, lcm_lo_info* info);
// k_pose_recover: pair p's matrix at d_E[p * e_stride ..], d_mask_in (NULL: all) one byte per record; results -> h->pose.d_res,
// mask -> h->pose.d_mask
int pose_enqueue(lcm_handle* h, const uint4* d_pts, const uint64_t* d_off, size_t n_pairs, size_t total, const double* d_E,
                 uint32_t e_stride, const uint8_t* d_mask_in, const lcm_epi_params& ep, const lcm_pose_params& pp, uint32_t* launches);
int pose_download(lcm_handle* h, size_t n_pairs, size_t total, lcm_pose_result* results, uint8_t* mask);
// ---- lcm_verify.cpp: the stages as one pipeline over a VerifyPlan (lcm_verify_host.h); lcm_l2_db.cpp runs it on the list kernel's
// point records
// *slices = launches of a kernel whose grid's y is the pair: ceil(n_pairs / grid_y_limit())
int pair_slices(size_t n_pairs, uint32_t* slices);
// A host call's offsets walked (epi_offsets_problem): LCM_ERR_CAPACITY for an over-long pair, LCM_ERR_INVALID_ARG otherwise
int offsets_checked(const size_t* offsets, int n_pairs, size_t* total, uint32_t* max_n);
// The parameters of the plan's stages that are on, checked into the plan: the pose's, then the optimisation's
int verify_params_checked(VerifyPlan* plan, const lcm_lo_params* lp, const lcm_pose_params* pp);
// epi_enqueue, then lo_enqueue and pose_enqueue (on the device's results[].E and mask) where the plan wants them; *launches =
// their sum.  verify_download: the same stages' records to the plan's buffers, enqueued.
int verify_enqueue(lcm_handle* h, const VerifyPlan& plan, const uint4* d_pts, const uint64_t* d_off, size_t n_pairs, uint32_t max_n,
                   size_t total, uint32_t* launches);
int verify_download(lcm_handle* h, const VerifyPlan& plan, size_t n_pairs, size_t total);
// lcm_epi_verify_pairs / lcm_lo_verify_pairs: a plan without the pose stage over host point pairs; lp as the caller gave it
int verify_pairs(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs, VerifyPlan* plan, const lcm_lo_params* lp);
// ---- lcm_map.cpp: the map's stages over records that are on the device; every *_enqueue works on h's stream and does not wait
// k_map_median: pair p's median -> h->map.d_median[p]
int map_median_enqueue(lcm_handle* h, const uint4* d_pts, const uint64_t* d_off, size_t n_pairs);
// k_map_triangulate: `pairs` (host, n_pairs plans of lcm_map_host.h; read until the caller has waited), d_mask (NULL: all) one byte
// per record; records -> h->map.d_tri / d_status, MAP_STATUSES counts per pair -> h->map.d_counts
int map_tri_enqueue(lcm_handle* h, const uint4* d_pts, const uint64_t* d_off, size_t n_pairs, uint32_t max_n, size_t total,
                    const uint8_t* d_mask, const MapPair* pairs, const lcm_map_params& mp);
// One merge: the n records' matches, pixels, results and statuses on the device, the tables and the outputs the caller's (host)
struct MapMergeIO {
    const uint4* d_matches; const uint4* d_pts; const MapTri* d_tri; const uint8_t* d_status; uint32_t n;
    int kf1, kf2; int32_t* table1; int n_kp1; int32_t* table2; int n_kp2; int n_points;
    lcm_ba_point* points_out; int cap_points; lcm_ba_obs* obs_out; int cap_obs; uint8_t* status_out;     // status_out may be NULL
};
// k_map_merge_count, two k_block_scan; the two totals come back and decide about the room (LCM_ERR_CAPACITY, *n_new / *n_merged
// set, nothing else written); then k_map_merge_emit into h->map's buffers.  Waits once, after the counts.  map_merge_download:
// the points, observations, statuses and both tables to the caller's buffers, enqueued.
int map_merge_run(lcm_handle* h, const MapMergeIO& io, int* n_new, int* n_merged, uint32_t* launches);
int map_merge_download(lcm_handle* h, const MapMergeIO& io, int n_new, int n_merged);
// What lcm_map_add_keyframe is given about the map
struct MapTrack {
    const lcm_map_params* mp; int kf_last, kf_new; const lcm_pgo_pose* pose_last; int32_t* table_last; int n_kp_last; int32_t* table_new;
    int n_kp_new; int n_points; lcm_ba_point* points_out; int cap_points; lcm_ba_obs* obs_out; int cap_obs; uint8_t* status_out;
    lcm_map_keyframe_report* report;
};
// h, the report, mp, the last pose, the counts, the buffers and the tables' entries (LCM_ERR_INVALID_ARG and the message otherwise)
int map_track_checked(lcm_handle* h, const MapTrack& t, int n_matches);
// behind a verification with the pose stage over ONE pair, enqueued and not yet read (the pose record is h->pose.d_res[0], its
// mask h->pose.d_mask): the median, the gates, the triangulation and the merge; waits; *t.report and the map's outputs written
int map_track_stages(lcm_handle* h, const MapTrack& t, const uint4* d_pts, const uint64_t* d_off, const uint4* d_matches, uint32_t n,
                     uint32_t* launches);
int map_keyframe_stages(lcm_handle* h, const MapTrack& t, const uint4* d_pts, const uint64_t* d_off, const uint4* d_matches,
                        const uint8_t* d_pose_mask, uint32_t n, const lcm_pose_result& pr, uint32_t* launches);
// ---- lcm_sift.cpp: the space that lcm_sift_detect_image cached in the handle, freed (lcm_destroy)
void sift_cached_destroy(lcm_handle* h);
}  // namespace lcm

namespace {
using lcm::cross_score_prefixes;
using lcm::eligible_prefix;
using lcm::L2Pair;
using lcm::L2Run;
using lcm::L2Where;
using lcm::launch_and_time;
using lcm::PairJob;
using lcm::RowSrc;
using lcm::mfma_bulk;
using lcm::mfma_online;
using lcm::pick_chunk;
using lcm::QUERY_SLOTS;
using lcm::set_device;
using lcm::sync_online_streams;
using lcm::STAGE_BUFS;
using lcm::wait_db;
}  // namespace
