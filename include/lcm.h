/*
 * lcm.h — C ABI of the MI355X loop-closure descriptor matcher ("lcm").
 *
 * This is the drop-in boundary for the ORB / Hamming hot path that the reference project
 * F-Fer/SLAM-Loop-Closing declares in include/loop_closing.hpp but delegates to
 * cv::BFMatcher(NORM_HAMMING).  Every entry point cites the reference interface it replaces
 * (paths are relative to the reference checkout):
 *
 *   lcm_match_pair        <- the `matcher_->match(desc1, desc2, matches)` call that
 *                            LoopClosingSystem::matchFeatures makes (include/loop_closing.hpp:40,73)
 *   lcm_match_features    <- LoopClosingSystem::matchFeatures incl. the "2 x minimum distance"
 *                            filter (include/loop_closing.hpp:40, README.md:116-117)
 *   lcm_match_stored      <- matchFeatures on two frames of frames_ (README.md:101 re-match of loop frames)
 *   lcm_match_features_ratio <- matchFeatures(desc1, desc2, good, ratio): knnMatch(k = 2) + Lowe's ratio test
 *                            (src/main.cpp:509-534), and its stored-frame / batch forms
 *   lcm_db_append*        <- `frames_.push_back(frame)` inside processFrame
 *                            (include/loop_closing.hpp:34,69) — the stored-frame descriptor database
 *   lcm_query_scores      <- the per-stored-frame loop inside detectLoops
 *                            (include/loop_closing.hpp:48, README.md:121-126)
 *   lcm_detect_loops      <- LoopClosingSystem::detectLoops (include/loop_closing.hpp:48)
 *   lcm_all_vs_all        <- the O(N^2) "every frame against every frame >= gap ago" search, whose only
 *                            executed analogue in the tree is src/main.cpp:1375-1388
 *   lcm_all_vs_all_ratio  <- that loop with the score it actually uses: the number of ratio-test survivors of
 *                            matchFeatures(desc[curr], desc[past], matches, 0.7) per pair (src/main.cpp:1386-1387);
 *                            lcm_query_scores_ratio is its one-frame form
 *   lcm_ratio_loop_test   <- that loop's verdict: `allDescriptors[i].rows < 100` skips a pair (src/main.cpp:1382),
 *                            `matches.size() >= 300` accepts the pair (:1388); ratio and both thresholds are parameters
 *   lcm_all_vs_all_loops_ratio <- the whole loop (src/main.cpp:1375-1388) in one call: ratio-test scores + that verdict on
 *                            the device, only candidates cross PCIe; lcm_detect_loops_ratio is its one-frame form
 *   lcm_group_all_vs_all_ratio, lcm_group_all_vs_all_loops_ratio <- the same two searches over several devices
 *   lcm_loop_candidate    <- struct LoopCandidate (include/loop_closing.hpp:22-27), same field order
 *   lcm_knn2_pair_l2, lcm_match_features_ratio_l2, lcm_match_pairs_ratio_l2 <- the same matcher on what the reference
 *                            feeds it: 128-D cv::SIFT rows under cv::NORM_L2 (src/main.cpp:497-504, :517)
 *   lcm_score_pairs_ratio_l2 <- what the loop search keeps of that call: matches.size() per pair (src/main.cpp:1386-1388),
 *                            counted on the device; lcm_loop_search_ratio_l2 is the whole loop (:1375-1388) on SIFT rows;
 *                            lcm_l2_ratio_test_device exposes the device's ratio-test verdict to tests
 *   lcm_dmatch            <- cv::DMatch as consumed at src/main.cpp:551-555 (queryIdx, trainIdx, imgIdx, distance)
 *
 * Conventions
 *   - plain C: pointers + sizes only, no C++/torch/OpenCV types; caller owns every host buffer;
 *     the library owns device memory behind the opaque lcm_handle.
 *   - a descriptor is 32 bytes (256 bits); descriptor matrices are row-major, n rows x 32 bytes,
 *     contiguous — exactly `cv::Mat(CV_8UC1, rows=n, cols=32).ptr<uint8_t>()`.
 *   - every function returns an lcm_status (0 = OK, negative = error); nothing throws across the
 *     boundary; lcm_last_error() gives the message of the calling thread's last failure.
 *   - there is NO CPU fallback: without a usable HIP device lcm_create fails with
 *     LCM_ERR_NO_DEVICE.  The CPU restatement under oracle/ is test infrastructure only.
 *   - a handle is thread-compatible (one caller at a time).  A call leaves the calling thread's current HIP device set to
 *     the handle's device (lcm_group_* calls: to one of the group's devices); callers that run their own HIP work on
 *     another device set it again afterwards.
 *   - sizes: a frame holds up to 65535 descriptor rows, as stored ("train") frame and as query frame alike (ORB's
 *     nfeatures is the caller's choice; the reference uses 2000).  Query frames above 2048 rows take the packed bulk
 *     route (see lcm_route); with cross_check != 0, or with LCM_TUNE_PACKED = 0, query frames are limited to 2048
 *     rows and a larger one is refused with LCM_ERR_CAPACITY.
 */
#ifndef LCM_H_
#define LCM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define LCM_API __attribute__((visibility("default")))
#else
#define LCM_API
#endif

#define LCM_DESC_BYTES 32          /* 256-bit ORB descriptor (README.md:115) */
#define LCM_DESC_WORDS 8
#define LCM_MAX_TRAIN_ROWS (1 << 22) /* packed (dist,idx) key: 9 + 22 bits */

typedef enum lcm_status {
    LCM_OK = 0,
    LCM_ERR_INVALID_ARG = -1,
    LCM_ERR_NO_DEVICE = -2,     /* no HIP device / runtime: the product path never falls back to CPU */
    LCM_ERR_HIP = -3,           /* a HIP runtime call failed (message has hipGetErrorString) */
    LCM_ERR_CAPACITY = -4,      /* output buffer or reserved database too small */
    LCM_ERR_ORDER = -5,         /* frame ids must be appended in strictly increasing order */
    LCM_ERR_NOT_FOUND = -6,     /* frame id not in this handle's database */
    LCM_ERR_OOM = -7
} lcm_status;

/* Parameters the reference leaves to README prose (README.md:108-126).  Defaults (lcm_params_default):
 * ratio=2, dist_floor=0, min_matches=50, sim_threshold=0.15, min_gap=30, cross_check=0. */
typedef struct lcm_params {
    int32_t ratio;          /* good match: d <= max(ratio*min_d, dist_floor)      README.md:117 */
    int32_t dist_floor;     /* README states no floor -> 0 */
    int32_t min_matches;    /* loop needs good_count >= min_matches               README.md:124 */
    int32_t min_gap;        /* compare only frames with cur_id - id >= min_gap    README.md:122, hpp:31.
                             * The gap is taken on frame IDS, not on storage positions: pass the processed-frame
                             * counter as id (as processFrame's callers do), or scale min_gap, when ids are sparse
                             * (e.g. raw video frame numbers with frame_skip = 3).  The tree's only executed
                             * analogue, src/main.cpp:1374-1379, is positional over keyframe indices; the two readings
                             * coincide for dense ids.  Part of what "parity unpinned" covers. */
    double  sim_threshold;  /* loop needs similarity > sim_threshold (strict)     README.md:123 */
    int32_t cross_check;    /* BFMatcher crossCheck (src/main.cpp:517 passes false): 0 = off (default);
                             * 1 = mutual nearest neighbours (recent OpenCV 4.x: the `sidx` test in batchDistance);
                             * 2 = legacy OpenCV (a query keeps the best train row among those that chose it).
                             * Version dependent upstream, hence off by default; see oracle/lcm_oracle.h. */
    int32_t reserved;       /* 0 */
} lcm_params;

/* One record per (query frame, stored frame) pair: what the device ships back (8 bytes).
 * similarity = good_count / min(n_query, n_train) is formed on the host in IEEE double. */
typedef struct lcm_score {
    uint32_t good_count;    /* matches surviving the ratio*min_d filter */
    uint16_t min_dist;      /* min over queries of the best distance; 0xFFFF if the pair is empty */
    uint16_t n_train;       /* descriptor rows of the stored frame */
} lcm_score;

/* Same layout as cv::DMatch (int queryIdx, trainIdx, imgIdx; float distance) — 16 bytes. */
typedef struct lcm_dmatch {
    int32_t query_idx;
    int32_t train_idx;
    int32_t img_idx;        /* always 0: single train image */
    float   distance;       /* integer-valued 0..256, exact in float */
} lcm_dmatch;

/* Same field order/types as loop_closing::LoopCandidate (include/loop_closing.hpp:22-27) — 24 bytes. */
typedef struct lcm_loop_candidate {
    int32_t current_frame_id;
    int32_t matched_frame_id;
    int32_t num_matches;
    double  similarity_score;
} lcm_loop_candidate;

/* Timing of the most recent bulk / pair-mode launch on this handle, from hipEvents on the launch stream.  Meant for
 * the bulk calls: online queries record into the same events from their own streams, so while online tickets are
 * outstanding (or a processFrame-style pair match runs beside one) the structure describes whichever launch recorded
 * last and is not attributable to a call — read lcm_online_stats_read for online work. */
typedef struct lcm_launch_info {
    double   kernel_ms;         /* device time of the pair-match kernel(s) of the last bulk call */
    uint64_t pairs;             /* (query frame, stored frame) pairs scored */
    uint64_t distances;         /* sum over pairs of n_query * n_train */
    uint64_t algo_bytes;        /* sum n_train*32 per pair + n_query*32 per query frame + 8 per pair */
    uint32_t launches;          /* kernel launches that made up the call */
    uint32_t workgroups;        /* workgroups of the (largest) launch */
    double   aux_kernel_ms;     /* device time of the call's follow-up kernels, 0 if none: the loop-test kernels
                                 * (k_loop_count, k_block_scan, k_loop_emit and the count read-back between them) of
                                 * lcm_all_vs_all_loops; the fold kernels of a packed bulk search (summed over its chunks:
                                 * kernel_ms - aux_kernel_ms is then the score kernels' time) */
    uint32_t route;             /* which kernels served the call: lcm_route */
    uint32_t launches_in_flight; /* packed bulk search of several chunks: 2 (consecutive chunks run on two streams, so that one
                                 * chunk's workgroups fill the chip while the other's launch drains); else 1 */
    double   score_ms_sum;      /* packed bulk search: SUM of the score kernels' own durations, each from events around it on
                                 * its stream (what a kernel trace reports per launch).  With 2 launches in flight they
                                 * overlap pairwise: score_ms_sum ~ launches_in_flight x (kernel_ms - exposed folds) */
    uint32_t score_launches;    /* packed bulk search: number of score launches (= chunks) */
    uint32_t reserved_;
} lcm_launch_info;
/* LCM_ROUTE_PLAIN: one workgroup per (query frame, run of stored frames), records formed in the kernel;
 * LCM_ROUTE_PACKED: query rows of consecutive frames packed into full 2048-row workgroups + fold kernel (bulk);
 * LCM_ROUTE_SPLIT: query frame cut into row chunks + fold kernel (online, short databases);
 * LCM_ROUTE_MATRIX: opt-in matrix-core variants 4 / 5; LCM_ROUTE_CROSS: cross_check (two passes + combine). */
typedef enum lcm_route { LCM_ROUTE_PLAIN = 0, LCM_ROUTE_PACKED = 1, LCM_ROUTE_SPLIT = 2, LCM_ROUTE_MATRIX = 3, LCM_ROUTE_CROSS = 4 } lcm_route;

/* Totals over the online queries COLLECTED so far on a handle (single and batched): device time of their kernels from
 * HIP events on the launch stream, and the work they did — what a streaming run's roofline is computed from. */
typedef struct lcm_online_stats {
    double   kernel_ms;
    uint64_t launches, queries, pairs, distances, algo_bytes;
} lcm_online_stats;

typedef struct lcm_handle lcm_handle;

LCM_API void        lcm_params_default(lcm_params* p);
LCM_API const char* lcm_last_error(void);
LCM_API const char* lcm_backend_name(void);         /* "hip-gfx950" */
LCM_API int         lcm_device_count(void);         /* #HIP devices, 0 if none / no runtime */

/* Create a matcher bound to HIP device `device_id`.  `stream` is a hipStream_t (as void*) that the bulk, pair-mode
 * and database work is enqueued on, or NULL for a library-owned stream.  Online queries (lcm_query_submit*,
 * lcm_detect_loops) run on streams the library owns, one per query slot, each ordered AFTER everything `stream` and the
 * append path already hold at submit time; their results reach the caller through the collect calls only, so nothing
 * on `stream` has to wait for them (LCM_TUNE_ONLINE_STREAMS = 0 puts them back on `stream`). */
LCM_API int  lcm_create(const lcm_params* params, int device_id, void* stream, lcm_handle** out);
LCM_API void lcm_destroy(lcm_handle* h);
LCM_API int  lcm_set_params(lcm_handle* h, const lcm_params* params);
LCM_API int  lcm_get_params(const lcm_handle* h, lcm_params* params);
LCM_API int  lcm_sync(lcm_handle* h);

/* ---- stored-frame descriptor database (device resident) -------------------------------------------- */
/* Reserve room for `n_frames` frames of up to `max_desc` rows each.  Growing later is allowed (copying). */
LCM_API int  lcm_db_reserve(lcm_handle* h, int n_frames, int max_desc);
/* Append one frame (host rows).  Copies through pinned staging with hipMemcpyAsync on a copy stream that
 * overlaps matching; the caller may reuse `desc` as soon as the call returns.  `n_keypoints` is the
 * similarity denominator (Frame::keypoints.size(), == n for ORB); pass -1 to use `n`. */
LCM_API int  lcm_db_append(lcm_handle* h, int frame_id, const uint8_t* desc, int n, int n_keypoints);
/* Same, rows already in device memory (n x 32 bytes, contiguous). */
LCM_API int  lcm_db_append_device(lcm_handle* h, int frame_id, const void* d_desc, int n, int n_keypoints);
LCM_API int  lcm_db_size(const lcm_handle* h);                 /* frames stored */
LCM_API int  lcm_db_clear(lcm_handle* h);
/* Keep the first n_frames stored frames, drop the rest (no-op if fewer are stored).  Waits for everything in flight;
 * tickets submitted before the call are void afterwards, as after lcm_db_clear. */
LCM_API int  lcm_db_truncate(lcm_handle* h, int n_frames);
LCM_API int  lcm_db_frame_info(const lcm_handle* h, int slot, int* frame_id, int* n_desc, int* n_keypoints);
/* Copy a stored frame's rows back to the host (tests / snapshot). */
LCM_API int  lcm_db_read(lcm_handle* h, int slot, uint8_t* desc_out, int cap_rows);

/* Snapshot / restore of the stored-frame database (ids, row counts, keypoint counts, rows) as one raw file — the
 * reference has no checkpointing; this makes long streaming runs resumable. */
LCM_API int  lcm_db_save(lcm_handle* h, const char* path);
LCM_API int  lcm_db_load(lcm_handle* h, const char* path);

/* ---- pair mode: BFMatcher(NORM_HAMMING, crossCheck=false).match ------------------------------------ */
/* For each query row q (ascending): train_idx[q] = FIRST index of the minimum Hamming distance over the
 * nt train rows, dist[q] = that distance.  nq == 0 or nt == 0: nothing is written, *n_matches = 0. */
LCM_API int  lcm_match_pair(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt,
                            int32_t* train_idx, uint16_t* dist, int* n_matches);
/* matchFeatures: the above + keep matches with d <= max(ratio*min_d, dist_floor), query order preserved.
 * `out` needs room for nq records. */
LCM_API int  lcm_match_features(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt,
                                lcm_dmatch* out, int* n_out, int* min_dist);

/* matchFeatures between two STORED frames (device-resident rows, no upload): the "re-match features on identified
 * loop frames" step (README.md:101) that turns a LoopCandidate into its DMatch list.  `out` needs room for the query
 * frame's row count (cap). */
LCM_API int  lcm_match_stored(lcm_handle* h, int query_frame_id, int train_frame_id,
                              lcm_dmatch* out, int cap, int* n_out, int* min_dist);

/* The same for MANY pairs in ONE launch (the match lists of all loop candidates of a frame): every pair is cut into
 * (query chunk x train segment) work items of one kernel launch, a second kernel folds the segments, one download.
 * out (host) receives the DMatch lists back to back; offsets[n_pairs + 1] (host, required) their bounds; min_dists
 * (host, optional) each pair's minimum distance, -1 if it has no matches.  A pair with an empty side has no matches.
 * The number of pairs in one call (here and in lcm_match_query_batch, lcm_match_stored_batch_ratio and
 * lcm_match_query_batch_ratio) is bounded by `int` and by memory, not by a launch grid: the fold kernel goes out in
 * slices of hipDeviceProp_t::maxGridSize[1] pairs (65535 on the MI355X), so an all-pairs search over a few hundred
 * frames fits one call. */
typedef struct lcm_pair_ref { int32_t query_frame_id, train_frame_id; } lcm_pair_ref;
LCM_API int  lcm_match_stored_batch(lcm_handle* h, const lcm_pair_ref* pairs, int n_pairs,
                                    lcm_dmatch* out, size_t cap, size_t* offsets, int32_t* min_dists);
/* ... and one query frame given by the host (the current frame, not stored yet) against n_trains stored frames. */
LCM_API int  lcm_match_query_batch(lcm_handle* h, const uint8_t* query, int nq, const int32_t* train_frame_ids, int n_trains,
                                   lcm_dmatch* out, size_t cap, size_t* offsets, int32_t* min_dists);

/* ---- pair mode, two neighbours: BFMatcher(NORM_HAMMING, crossCheck=false).knnMatch(k = 2) + Lowe's ratio test ---- */
/* The matcher the reference actually runs (src/main.cpp:509-534): for each query row the two nearest train rows in
 * OpenCV's batchDistance order — ascending by distance, the lower train index first among equal distances, i.e. the two
 * smallest (distance, train index) pairs — then `best` is kept iff best.distance < ratio * second.distance (strict,
 * evaluated in IEEE double) and a query row with fewer than two neighbours is dropped.  It is used with ratio 0.75 for
 * consecutive frames (src/main.cpp:1154) and 0.7 for the loop search (:1386).  These calls do not consult
 * lcm_params.ratio / dist_floor; they return LCM_ERR_INVALID_ARG while cross_check != 0 (OpenCV asserts knn == 1 under
 * crossCheck) and for a ratio that is NaN or negative.  Errors, capacities, empty sides and `offsets` are those of the
 * k = 1 calls above; records have img_idx = 0 and the integer-valued distance of `best`.
 * Sizes (tests/test_gpu_knn_limits.py runs each at its limit): a train matrix of lcm_knn2_pair / lcm_match_features_ratio
 * holds up to LCM_MAX_TRAIN_ROWS rows (LCM_ERR_CAPACITY above; both neighbours' indices use the key's 22 bits), nq is
 * not limited there; stored frames take part with up to 65535 rows on either side; the host query of
 * lcm_match_query_batch_ratio may hold up to 131072 rows (64 x 2048; LCM_ERR_CAPACITY above), as lcm_match_query_batch's. */
/* knnMatch(k=2) (src/main.cpp:520): train_idx[2*q + k], dist[2*q + k], k = 0 best, 1 second; a missing second neighbour
 * (nt == 1) is train_idx = -1, dist = 0xFFFF.  *n_neighbours = min(nt, 2), 0 if either side is empty (nothing written then). */
LCM_API int  lcm_knn2_pair(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt,
                           int32_t* train_idx, uint16_t* dist, int* n_neighbours);
/* matchFeatures(desc1, desc2, good, ratio) (src/main.cpp:509-534): the above + the ratio test, query order preserved.
 * `out` needs room for nq records. */
LCM_API int  lcm_match_features_ratio(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt, double ratio,
                                      lcm_dmatch* out, int* n_out);
/* The same between two STORED frames (src/main.cpp:1386 matches keyframe descriptors that are already kept). */
LCM_API int  lcm_match_stored_ratio(lcm_handle* h, int query_frame_id, int train_frame_id, double ratio,
                                    lcm_dmatch* out, int cap, int* n_out);
/* ... for MANY stored pairs in ONE launch: the reference's loop search (src/main.cpp:1375-1388 counts the ratio-test
 * survivors of the current keyframe against every earlier one).  The match count of pair p is offsets[p+1] - offsets[p]. */
LCM_API int  lcm_match_stored_batch_ratio(lcm_handle* h, const lcm_pair_ref* pairs, int n_pairs, double ratio,
                                          lcm_dmatch* out, size_t cap, size_t* offsets);
/* ... and one query frame given by the host (the current frame, src/main.cpp:1386's desc1) against n_trains stored frames. */
LCM_API int  lcm_match_query_batch_ratio(lcm_handle* h, const uint8_t* query, int nq, const int32_t* train_frame_ids, int n_trains,
                                         double ratio, lcm_dmatch* out, size_t cap, size_t* offsets);

/* ---- pair mode on SIFT rows: BFMatcher(NORM_L2, crossCheck=false).knnMatch(k = 2) + Lowe's ratio test ------------ */
/* What the reference's matcher is fed: detectAndDescribeSIFT (src/main.cpp:497-504, cv::SIFT::create(4000)) produces
 * 128-D descriptors and cv::BFMatcher(cv::NORM_L2, false) (:517) matches them.  OpenCV's SIFT stores every element through
 * saturate_cast<uchar>, so a row is 128 integers 0..255 (SIFT::create(..., CV_8U) hands out the bytes themselves): a row
 * here is LCM_SIFT_BYTES uint8.  With D(q, t) = sum (q_i - t_i)^2, an exact integer <= 8 323 200 < 2^24, the distance is
 * s = (float)sqrt(D), correctly rounded — bit for bit what OpenCV's float accumulation + sqrt give — and a query row's
 * neighbours are the two smallest (s, train index) pairs, best first (batchDistance, K = 2).  The order is on s, not on D:
 * above 2^22 adjacent integers can share a float root (first 4197200, 4197201) and the lower train index then comes first.
 * `best` is kept iff (double)s1 < ratio * (double)s2 (strict); a row with fewer than two neighbours is dropped.
 * Shared with the Hamming k = 2 calls above: LCM_ERR_INVALID_ARG while cross_check != 0, for a NaN or negative ratio, a
 * NULL pointer or a negative count; LCM_ERR_CAPACITY when `cap` is too small, checked before anything is written to `out`;
 * lcm_params.ratio / dist_floor play no part; the work is ordered on the handle's stream and finished on return.  A matrix
 * holds at most 65 535 rows (LCM_ERR_CAPACITY above).  These calls store nothing (the 32-byte database is a different descriptor); the SIFT keyframe
 * store is lcm_l2_db_*, below. */
#define LCM_SIFT_BYTES 128
/* Host only, no device needed: n CV_32F SIFT rows (src/main.cpp:497-504) -> bytes.  LCM_ERR_INVALID_ARG, and nothing
 * written, if any value is not an integer in [0, 255] (NaN, inf, fractions, RootSIFT-normalised rows). */
LCM_API int  lcm_sift_pack_f32(const float* rows, int n, uint8_t* out);
/* knnMatch(k = 2) (src/main.cpp:517-520): train_idx[2*q + k] and dist[2*q + k] are required, dist_sq[2*q + k] (= D) is
 * optional and may be NULL.  A missing second neighbour (nt == 1) is train_idx = -1, dist = +INFINITY, dist_sq = 0xFFFFFFFF.
 * *n_neighbours = min(nt, 2), or 0 with nothing written if either side is empty. */
LCM_API int  lcm_knn2_pair_l2(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt,
                              int32_t* train_idx, float* dist, uint32_t* dist_sq, int* n_neighbours);
/* matchFeatures(desc1, desc2, good, ratio) (src/main.cpp:509-534; :1154 calls it with 0.75).  `out` needs room for nq
 * records.  Each record has img_idx = 0 and distance = s1. */
LCM_API int  lcm_match_features_ratio_l2(lcm_handle* h, const uint8_t* query, int nq, const uint8_t* train, int nt, double ratio,
                                         lcm_dmatch* out, int* n_out);
/* The loop search's inner call for MANY pairs (src/main.cpp:1375-1388): n_frames host matrices (frames[f]: rows[f] rows),
 * each uploaded ONCE; pairs[p] = {query position, train position} into `frames` (a position outside [0, n_frames) is
 * LCM_ERR_INVALID_ARG; a pair may name the same matrix on both sides; a pair with an empty side has an empty list).  One
 * score launch plus one fold for the whole set.  The lists come back to back in `out`, bounded by offsets[n_pairs + 1]
 * (required); the match count the reference thresholds at 300 (:1388) is offsets[p+1] - offsets[p].
 * Pairs per call: any n_pairs whose work fits 2^31 - 1 (query chunk x 512-row train segment) items and 2^31 - 1 query
 * rows in total, LCM_ERR_CAPACITY above that, before anything is launched; the fold over the pairs goes out in slices of
 * hipDeviceProp_t::maxGridSize[1] pairs, so 65535 pairs (an all-pairs search over 363 frames) is no limit. */
LCM_API int  lcm_match_pairs_ratio_l2(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames,
                                      const lcm_pair_ref* pairs, int n_pairs, double ratio,
                                      lcm_dmatch* out, size_t cap, size_t* offsets);

/* ---- loop search on SIFT rows: ratio-test COUNTS per pair, decided on the device ------------------------------------ */
/* The reference's loop search (src/main.cpp:1375-1388) runs matchFeatures(desc[curr], desc[past], matches, 0.7) on every
 * admissible keyframe pair and looks at matches.size() only.  The count depends on each query row's two smallest float
 * distances alone — the roots of its two smallest D, as a multiset — so no index, no per-row list and no match record is
 * formed: one workgroup per chunk of 128 or 256 query rows walks the pair's whole train matrix (k_l2_count, route
 * LCM_ROUTE_PLAIN), takes the exact float roots ((float)sqrt((double)D) has sqrtf's bits for every D <= 8 323 200) and the
 * IEEE double comparison on the device, and 8 bytes per pair come back.  For every pair good_count equals
 * offsets[p+1] - offsets[p] of lcm_match_pairs_ratio_l2, and min_dist_sq is the pair's smallest D (the smallest dist_sq that
 * lcm_knn2_pair_l2 reports, unless three train rows tie at the float root of a row's minimum).
 * A call with few pairs does not fill the chip (a pair is at most 512 workgroups of 128 rows, 32 at 4000 rows): the single
 * pair's call remains lcm_match_features_ratio_l2.  LCM_TUNE_L2_COUNT_CHUNK = 128 | 256 (environment) pins the chunk;
 * lcm_last_launch_info: workgroups = sum over the pairs with two non-empty sides of ceil(query rows / chunk), kernel_ms
 * around the count kernel. */
typedef struct lcm_l2_score {      /* 8 bytes, one per pair */
    uint32_t good_count;           /* query rows with (double)s1 < ratio * (double)s2; rows with < 2 neighbours do not count */
    uint32_t min_dist_sq;          /* min over query rows of D1; 0xFFFFFFFF if either side is empty */
} lcm_l2_score;
/* Arguments and refusals of lcm_match_pairs_ratio_l2 (cross_check, ratio, row counts, positions, NULLs; LCM_ERR_CAPACITY
 * above 2^31 - 1 items); a pair may name one matrix on both sides; a pair with an empty side yields {0, 0xFFFFFFFF} and
 * launches nothing.  Ordered on the handle's stream, finished on return; the records are re-initialised on the stream
 * by every call. */
LCM_API int  lcm_score_pairs_ratio_l2(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames,
                                      const lcm_pair_ref* pairs, int n_pairs, double ratio, lcm_l2_score* scores);
/* The loop at src/main.cpp:1375-1388 in one call, on POSITIONS into `frames`: curr in [loop_gap, n_frames), past in
 * [0, curr - loop_gap], in that order; a pair is skipped, before scoring, if skip[curr] or skip[past] is non-zero
 * (`poses[i].R.empty()`, :1377 / :1381; skip == NULL: none) or either matrix has fewer than rp->min_rows rows (:1382).
 * *n_pairs_out (optional) = pairs scored.  A pair is a candidate iff good_count >= rp->min_matches (:1388):
 * current_frame_id = curr, matched_frame_id = past, num_matches = good_count, similarity_score = (double)good_count /
 * (double)min(rows) in IEEE double (0.0 for an empty side) — informational.  Candidates come in (curr, past) order; the
 * verdict runs on the host over the 8-byte records.  rp == NULL: ratio 0.7, min_rows 100, min_matches 300
 * (lcm_ratio_loop_params, below).  loop_gap < 1 is LCM_ERR_INVALID_ARG (the reference's max(3, numViews / 2) stays with
 * the caller); more candidates than `cap` (or out == NULL with candidates present) is LCM_ERR_CAPACITY: *n_out is then the
 * count and nothing is written to `out`. */
struct lcm_ratio_loop_params;
LCM_API int  lcm_loop_search_ratio_l2(lcm_handle* h, const uint8_t* const* frames, const int* rows, int n_frames,
                                      const uint8_t* skip, int loop_gap, const struct lcm_ratio_loop_params* rp,
                                      lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out);
/* Diagnostic: pass[i] (0 or 1) = the verdict of the count kernel's own device function on the squared distances
 * (d1[i], d2[i]) of a first and a second neighbour, n host-given pairs; a value above 8 323 200 is LCM_ERR_INVALID_ARG.
 * Descriptor inputs can only sample the range of D: this lets a test walk all of it. */
LCM_API int  lcm_l2_ratio_test_device(lcm_handle* h, const uint32_t* d1, const uint32_t* d2, size_t n, double ratio,
                                      uint8_t* pass);

/* ---- the SIFT keyframe store: rows uploaded and packed ONCE, searched from the device ---------------------------------- */
/* The calls above take host matrices: each one is uploaded and packed again by every call, and a 32-byte work item per
 * (pair, query chunk) goes up with them.  The store keeps the matrices on the device — raw rows, operand image and per-row
 * words, a frame starting at a tile of 32 rows — the way the 32-byte database keeps ORB frames: an online loop check of
 * one new keyframe (src/main.cpp:1375-1421, one iteration of the outer loop) uploads that keyframe alone, and a search is
 * launched from tables that grow with the number of FRAMES (at most 32 bytes per scored `curr` and 8 per stored frame):
 * every workgroup derives its (pair, chunk) item on the device (k_l2_count_store).  The store is separate from the 32-byte
 * database (lcm_db_*): neither sees the other's frames.  It is not part of lcm_db_save / lcm_db_load or of a group.
 * A frame is addressed by its SLOT, its position in append order (allDescriptors[i]).  Capacity starts at what the first
 * append needs and doubles; a growth copies device to device on the handle's stream.  Every call is ordered on the
 * handle's stream and finished on return, so the caller's rows may be reused at once.
 * Records, order, refusals and the capacity rule of the store's searches are those of lcm_score_pairs_ratio_l2,
 * lcm_match_pairs_ratio_l2 and lcm_loop_search_ratio_l2 with the stored matrices as `frames` (cross_check, a NaN or negative
 * ratio, NULLs, loop_gap < 1, LCM_ERR_CAPACITY above 65 535 rows or 2^31 - 1 items or pairs; *n_out set and `out` untouched
 * when `cap` is too small); a slot outside [0, lcm_l2_db_size) is LCM_ERR_INVALID_ARG.  LCM_TUNE_L2_COUNT_CHUNK and
 * lcm_last_launch_info (workgroups, route, pairs, distances, kernel_ms) as for those calls. */
typedef struct lcm_l2_db_info {        /* 40 bytes */
    int32_t  frames;                   /* stored frames */
    int32_t  reserved_;
    uint64_t tiles_used;               /* tiles of 32 rows taken by the stored frames */
    uint64_t tiles_reserved;           /* tiles the three arenas have room for */
    uint64_t device_bytes;             /* device memory of the arenas and the frame table */
    uint64_t table_bytes;              /* tables uploaded by the last lcm_l2_db_loop_search / lcm_l2_db_detect_loops */
} lcm_l2_db_info;
/* Stores n rows (n in [0, 65535]; a frame of 0 rows takes a slot and is never paired); *slot (optional) = its slot. */
LCM_API int  lcm_l2_db_append(lcm_handle* h, const uint8_t* rows, int n, int* slot);
LCM_API int  lcm_l2_db_size(lcm_handle* h);                                   /* stored frames; 0 for a NULL handle */
LCM_API int  lcm_l2_db_rows(lcm_handle* h, int slot, int* n);
/* The raw rows of a slot back, bit for bit; cap_rows below the frame's rows is LCM_ERR_CAPACITY. */
LCM_API int  lcm_l2_db_read(lcm_handle* h, int slot, uint8_t* out, int cap_rows);
/* Keeps the first n_frames slots (their tiles are reused by later appends); clear = truncate to 0.  Memory stays reserved. */
LCM_API int  lcm_l2_db_truncate(lcm_handle* h, int n_frames);
LCM_API int  lcm_l2_db_clear(lcm_handle* h);
LCM_API int  lcm_l2_db_info_read(lcm_handle* h, lcm_l2_db_info* out);
/* lcm_score_pairs_ratio_l2 / lcm_match_pairs_ratio_l2 with pairs[p] = {query slot, train slot}: nothing is uploaded but
 * the work tables, nothing is packed. */
LCM_API int  lcm_l2_db_score_pairs(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio, lcm_l2_score* scores);
LCM_API int  lcm_l2_db_match_pairs_ratio(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio,
                                         lcm_dmatch* out, size_t cap, size_t* offsets);
/* lcm_loop_search_ratio_l2 over the stored slots (src/main.cpp:1375-1388); skip: one byte per slot, or NULL. */
LCM_API int  lcm_l2_db_loop_search(lcm_handle* h, const uint8_t* skip, int loop_gap, const struct lcm_ratio_loop_params* rp,
                                   lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out);
/* One iteration of that search's outer loop: frame `curr` against the slots [0, min(curr - loop_gap, size - 1)], candidates
 * in ascending slot order with current_frame_id = curr.  query != NULL: the nq host rows stand for position curr (typically
 * lcm_l2_db_size(h), before the append) and are not stored: they are staged in the arena's free tail, which grows if it
 * must, and a later append may overwrite them.  query == NULL: curr must be a stored slot (LCM_ERR_INVALID_ARG otherwise)
 * and its rows are used in place; nq is ignored.  skip (one byte per slot, or NULL) is consulted for the past slots only:
 * whether `curr` itself is searched is the caller's decision (:1377); rp->min_rows applies to both sides. */
LCM_API int  lcm_l2_db_detect_loops(lcm_handle* h, int curr, const uint8_t* query, int nq, const uint8_t* skip, int loop_gap,
                                    const struct lcm_ratio_loop_params* rp, lcm_loop_candidate* out, size_t cap,
                                    size_t* n_out, size_t* n_pairs_out);

/* ---- the store's loop correspondences: filtered, compacted and gathered on the device ---------------------------------- */
/* src/main.cpp:1386-1392 ends with extractMatchedPoints(kp[curr], kp[past], matches, ptsCurr, ptsPast): the two point arrays
 * findEssentialMat gets.  A frame appended WITH its keypoint coordinates keeps them in a fourth arena of the store's tile
 * space (8 bytes per row; created when the first such frame arrives, sized, grown, truncated and cleared with the other
 * three).  The coordinates are carried as bytes: NaN and -0.0 come back bit for bit.  The calls below run Lowe's ratio test,
 * an ordered compaction and the keypoint gather on the device after the score, fold and rescan kernels (lcm_l2_emit.hip):
 * 8 bytes per pair (`offsets`) come back first and decide about `cap`, then only the surviving records do.
 * Refusals as for the rest of the family: cross_check != 0, a NaN or negative ratio, NULLs, a slot outside the store
 * (LCM_ERR_INVALID_ARG), more than 65 535 rows (LCM_ERR_CAPACITY); ordered on the handle's stream and finished on return.
 * lcm_last_launch_info: workgroups and kernel_ms are the score kernel's, aux_kernel_ms the count / scan / list kernels'.
 * (The four are declared `extern`: the plain spelling is the list tests/test_l2_store_host.py pins for the calls above.) */
typedef struct lcm_point_pair { float qx, qy, tx, ty; } lcm_point_pair;   /* 16 bytes: kp[query_idx].pt, kp[train_idx].pt */
/* lcm_l2_db_append plus n coordinate pairs, pts = n x (x, y).  lcm_l2_db_append stores a frame WITHOUT points; a store may
 * hold both kinds. */
LCM_API extern int lcm_l2_db_append_kp(lcm_handle* h, const uint8_t* rows, const float* pts, int n, int* slot);
/* The points of a slot back, bit for bit: LCM_ERR_INVALID_ARG for a slot stored without points, LCM_ERR_CAPACITY for
 * cap_rows below the frame's rows. */
LCM_API extern int lcm_l2_db_read_kp(lcm_handle* h, int slot, float* out, int cap_rows);
/* `out` and `offsets` are byte for byte lcm_l2_db_match_pairs_ratio's on the same arguments; pts[i] (pts may be NULL) holds
 * the two keypoints of out[i].  With pts every named slot that has rows must have points (LCM_ERR_INVALID_ARG otherwise,
 * before any launch).  If the lists do not fit `cap`: LCM_ERR_CAPACITY, nothing is written to out or pts and
 * offsets[n_pairs] holds the needed count. */
LCM_API extern int lcm_l2_db_match_points(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio,
                                          lcm_dmatch* out, lcm_point_pair* pts, size_t cap, size_t* offsets);
/* One iteration of the reference's outer loop up to line 1392: cands, *n_cands, *n_pairs_out and the candidate-capacity
 * rule are lcm_l2_db_detect_loops's; the lists (and point pairs) of the candidates follow in candidate order, candidate c in
 * [offsets[c], offsets[c + 1]) with query = curr and train = the matched slot (offsets: cand_cap + 1 entries; only
 * offsets[0] is written when the candidates do not fit).  query != NULL: query_pts is staged with the rows in the free tail;
 * query_pts == NULL is allowed only with pts == NULL.  query == NULL: the stored slot curr and its own points.  With pts, a
 * matched slot without points is LCM_ERR_INVALID_ARG.  `cap` too small: as lcm_l2_db_match_points, offsets[*n_cands] = the
 * needed count (the candidates have been written). */
LCM_API extern int lcm_l2_db_detect_loops_points(lcm_handle* h, int curr, const uint8_t* query, const float* query_pts, int nq,
                                                 const uint8_t* skip, int loop_gap, const struct lcm_ratio_loop_params* rp,
                                                 lcm_loop_candidate* cands, size_t cand_cap, size_t* n_cands, size_t* n_pairs_out,
                                                 lcm_dmatch* out, lcm_point_pair* pts, size_t cap, size_t* offsets);

/* ---- loop verification on the device: essential-matrix RANSAC over the correspondences ---------------------------------- */
/* src/main.cpp:1395-1403: E = findEssentialMat(ptsCurr, ptsPast, K, RANSAC, 0.999, 1.0, mask), inliers = countNonZero(mask),
 * and the verdict `inliers > 200 && inliers / matches > 0.6`.  This is NOT OpenCV's estimator bit for bit: the minimal solver
 * is the linear EIGHT-point method (not the five-point one: it is degenerate on an all-planar scene) and the number of
 * hypotheses is FIXED (`iters`, not adaptive).  Every step is defined here and deterministic (lcm_epi_device.h):
 *   normalisation  (u, v) -> x = ((double)u - cx) / fx, y = ((double)v - cy) / fy; query x1 = (a, b, 1), train x2 = (c, d, 1),
 *                  x2^T E x1 = 0 (curr = query = points1, the reference's argument order)
 *   threshold      t = threshold / ((fx + fy) / 2), t2 = t * t
 *   error          E row-major e0..e8: p0 = e0 a + e1 b + e2, p1 = e3 a + e4 b + e5, p2 = e6 a + e7 b + e8,
 *                  q0 = e0 c + e3 d + e6, q1 = e1 c + e4 d + e7, num = c p0 + d p1 + p2, den = p0^2 + p1^2 + q0^2 + q1^2;
 *                  in double, every product and sum rounded on its own, sums left to right
 *   inlier         den > 0 && num * num <= t2 * den
 *   sampling       hypothesis `it` of pair `p` draws 8 distinct records by Floyd's algorithm from a 32-bit counter hash of
 *                  (seed, p, it, draw); p is the pair's position in the call
 *   solver         null vector of the 8 x 9 system by elimination with full pivoting, singular values forced to (1, 1, 0);
 *                  a rank-deficient sample gives the all-zero matrix, which has no inlier
 *   selection      the largest inlier count over the `iters` hypotheses, among equals the lowest hypothesis
 * A pair with fewer than 8 records: status LCM_EPI_TOO_FEW, zero E, no inliers, an all-zero mask.  A pair holds at most
 * 65 535 records (LCM_ERR_CAPACITY).  Ordered on the handle's stream and finished on return. */
typedef struct lcm_epi_params {
    double   fx, fy, cx, cy;    /* the camera matrix K; the defaults leave it zero: fx <= 0 or fy <= 0 is LCM_ERR_INVALID_ARG */
    double   threshold;         /* pixels, 1.0 */
    double   min_ratio;         /* 0.6:  lcm_epi_loop_test */
    int32_t  iters;             /* 1024: hypotheses per pair, a multiple of 64 in [64, 65536] */
    int32_t  min_inliers;       /* 200:  lcm_epi_loop_test */
    uint32_t seed;              /* 0 */
    uint32_t reserved;
} lcm_epi_params;               /* 64 bytes */
typedef enum lcm_epi_status { LCM_EPI_OK = 0, LCM_EPI_TOO_FEW = 1 } lcm_epi_status;
typedef struct lcm_epi_result {
    double  E[9];               /* row-major, singular values (1, 1, 0); all zero when no hypothesis had an inlier */
    int32_t n_points, n_inliers, best_iter, status;
} lcm_epi_result;               /* 88 bytes */
LCM_API void lcm_epi_params_default(lcm_epi_params* p);
/* Host only: n_inliers > min_inliers && (double)n_inliers / n_points > min_ratio, both strict (:1403); 0 for a NULL. */
LCM_API int  lcm_epi_loop_test(const lcm_epi_result* r, const lcm_epi_params* ep);
/* The RANSAC over host point lists in the layout lcm_l2_db_match_points returns: pair p owns pts[offsets[p] .. offsets[p + 1]),
 * offsets[0] == 0.  results: n_pairs records; mask (may be NULL): offsets[n_pairs] bytes, 1 = inlier of the pair's E.
 * lcm_last_launch_info: kernel_ms is the three kernels'. */
LCM_API int  lcm_epi_verify_pairs(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs,
                                  const lcm_epi_params* ep, lcm_epi_result* results, uint8_t* mask);
/* Test and plug-in seams.  lcm_epi_hypotheses: what the solver kernel makes of ONE pair of n records standing at position
 * pair_index of a call: samples = iters x 8 indices (-1 when n < 8), E = iters x 9 doubles.  lcm_epi_score_models: the scoring
 * kernel's inlier count of each of n_models (1 .. 65536) caller-supplied matrices E = n_models x 9 over n records. */
LCM_API int  lcm_epi_hypotheses(lcm_handle* h, const lcm_point_pair* pts, int n, uint32_t pair_index, const lcm_epi_params* ep,
                                int32_t* samples, double* E);
LCM_API int  lcm_epi_score_models(lcm_handle* h, const lcm_point_pair* pts, int n, const double* E, int n_models,
                                  const lcm_epi_params* ep, int32_t* counts);
/* lcm_l2_db_match_points followed by the RANSAC on the point records the list kernel has just written, before anything is
 * copied back: out, pts (required here) and offsets are byte for byte lcm_l2_db_match_points's, results / mask as
 * lcm_epi_verify_pairs's on those points.  `cap` too small: as lcm_l2_db_match_points, and neither results nor mask are written.
 * lcm_last_launch_info: as after lcm_l2_db_match_points, the three kernels added to launches and to aux_kernel_ms. */
LCM_API int  lcm_epi_db_verify_pairs(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio, const lcm_epi_params* ep,
                                     lcm_epi_result* results, lcm_dmatch* out, lcm_point_pair* pts, uint8_t* mask, size_t cap,
                                     size_t* offsets);
/* lcm_l2_db_detect_loops_points plus the verification: one iteration of the reference's outer loop through the first two clauses
 * of :1403.  Candidates, lists, point pairs and offsets are unchanged; results[c] (cand_cap records) and the mask bytes
 * [offsets[c], offsets[c + 1]) belong to candidate c, whose sampler is seeded with c.  The third clause (> globalMaxInliers)
 * and recoverPose (:1405-1421) are lcm_pose_db_detect_loops's, below. */
LCM_API int  lcm_epi_db_detect_loops(lcm_handle* h, int curr, const uint8_t* query, const float* query_pts, int nq,
                                     const uint8_t* skip, int loop_gap, const struct lcm_ratio_loop_params* rp,
                                     const lcm_epi_params* ep, lcm_loop_candidate* cands, size_t cand_cap, size_t* n_cands,
                                     size_t* n_pairs_out, lcm_epi_result* results, lcm_dmatch* out, lcm_point_pair* pts,
                                     uint8_t* mask, size_t cap, size_t* offsets);

/* ---- loop verification, second step: the RANSAC's best hypotheses refitted on their inliers (local optimisation) --------- */
/* The eight-point hypothesis of a minimal sample is as noisy as its eight keypoints: with a third of a pixel of noise no
 * hypothesis of the RANSAC above gathers the inliers the true E has, and the verdict is lost.  lcm_lo_* run that RANSAC
 * unchanged and then refit its LCM_LO_SEEDS best hypotheses on their own inliers (LO-RANSAC, lcm_lo_device.h).
 * Per pair, from its records, its `iters` hypotheses E[it] and their inlier counts cnt[it] (the RANSAC's own bytes), with
 * t = threshold / ((fx + fy) / 2) and "inlier under m" = the inlier rule above with t2 = (t m)^2:
 *   seeds       the 64 hypotheses with the largest keys (cnt << 16 | 0xFFFF - it), the RANSAC's selection key; seed l has the
 *               l-th largest.  Integers only
 *   round r     (r < rounds, multiplier mult[r]) of a seed, from cur = E[seed]:
 *               S = the records that are inliers of cur under mult[r]; fewer than 8: the seed stops
 *               per side over S: mean (mx, my), v = mean of (x - mx)^2 + (y - my)^2, s = sqrt(2 / v); v below 1e-20 (the
 *               rounding of the mean, not a spread), NaN or infinite on either side: the seed stops (LCM_LO_DEGENERATE);
 *               T = [[s, 0, -s mx], [0, s, -s my], [0, 0, 1]]
 *               M = the sum over S, in record order, of r r^T for the constraint row r = (c a, c b, c, d a, d b, d, a, b, 1) of
 *               the normalised x1' = T1 x1 = (a, b, 1), x2' = T2 x2 = (c, d, 1); f = the eigenvector of M's smallest eigenvalue
 *               (cyclic Jacobi, 8 sweeps); F = T2^T mat(f) T1; E' = F with its singular values forced to (1, 1, 0), as the
 *               solver's; without a second singular value the seed stops
 *               cur = E' whether or not it is better; c' = the inliers of E' under the model's own t2 (multiplier 1)
 *   seed's best the first (c', r) with the strictly largest c'; before round 0 the seed itself with cnt[seed] and round -1
 *   result      the largest count over the 64 seeds, among equals the lowest l, within a seed the earliest round: n_inliers
 *               is never below the RANSAC's.  Nothing strictly better: the RANSAC's record byte for byte (E, n_inliers,
 *               best_iter) and round -1.  The mask is the inlier rule of the winning E under t2
 * In double, every product and sum rounded on its own.  A pair with fewer than 8 records passes through as LCM_EPI_TOO_FEW
 * (info.status LCM_LO_TOO_FEW); a pair whose records ALL TOGETHER fail the spread test on a side (identical keypoints) has
 * no subset that passes it: it passes through with info.status LCM_LO_DEGENERATE. */
#define LCM_LO_SEEDS 64
typedef struct lcm_lo_params {
    int32_t  rounds;            /* 4: in [1, 8] */
    int32_t  seeds;             /* 64: the only accepted value */
    double   mult[8];           /* {3, 2, 1.5, 1}: round r's threshold multiplier, finite and >= 1 for r < rounds */
    uint32_t reserved[6];
} lcm_lo_params;                /* 96 bytes */
typedef enum lcm_lo_status { LCM_LO_OK = 0, LCM_LO_TOO_FEW = 1, LCM_LO_DEGENERATE = 2, LCM_LO_NO_MODEL = 3 } lcm_lo_status;
typedef struct lcm_lo_info {
    int32_t seed_iter;          /* the hypothesis the winning seed started from (= the result's best_iter) */
    int32_t round;              /* the winning round, -1 = the RANSAC's record kept */
    int32_t n_inliers_ransac;   /* what lcm_epi_verify_pairs reports for the pair */
    int32_t status;             /* lcm_lo_status of the pair: LCM_LO_OK, LCM_LO_TOO_FEW or LCM_LO_DEGENERATE */
} lcm_lo_info;                  /* 16 bytes */
LCM_API extern void lcm_lo_params_default(lcm_lo_params* p);
/* lcm_epi_verify_pairs plus the optimisation: results are lcm_epi_result records (lcm_epi_loop_test, lcm_pose_* and
 * lcm_pose_best take them unchanged; best_iter = the winning seed's hypothesis), info: n_pairs records, mask as there.
 * lp == NULL: the defaults (in every call of the family).  Refusals as lcm_epi_verify_pairs's, and a bad lp: nothing is
 * written.  lcm_last_launch_info: kernel_ms is the five kernels' (the RANSAC's three, k_lo_select, k_lo_refine). */
LCM_API extern int lcm_lo_verify_pairs(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs,
                                       const lcm_epi_params* ep, const lcm_lo_params* lp, lcm_epi_result* results,
                                       lcm_lo_info* info, uint8_t* mask);
/* Test seams.  lcm_lo_select: the selection kernel on caller-supplied counts (iters of them, each in [0, 65535]; iters a
 * multiple of 64 in [64, 65536]): seeds_out[l] = the hypothesis of the l-th largest key.  lcm_lo_refit_models: ONE round
 * under the multiplier `mult` for each of n_models (1 .. 64) caller-supplied models E_in = n_models x 9 over n records:
 * E_out = n_models x 9 (all zero unless status is LCM_LO_OK), n_selected = |S|, status = LCM_LO_OK, LCM_LO_TOO_FEW (|S| < 8),
 * LCM_LO_DEGENERATE or LCM_LO_NO_MODEL (no second singular value). */
LCM_API extern int lcm_lo_select(lcm_handle* h, const int32_t* counts, int iters, int32_t* seeds_out);
LCM_API extern int lcm_lo_refit_models(lcm_handle* h, const lcm_point_pair* pts, int n, const double* E_in, int n_models,
                                       double mult, const lcm_epi_params* ep, double* E_out, int32_t* n_selected,
                                       int32_t* status);
/* lcm_pose_db_verify_pairs (declared below) with the optimisation between the RANSAC and the pose kernel: everything before the
 * RANSAC (lists, points, offsets) is byte for byte lcm_l2_db_match_points's, results / info / mask are lcm_lo_verify_pairs's on
 * the returned points, pose_results / pose_mask lcm_pose_recover_pairs's on the optimised E and mask.  `cap` too small: as
 * there.  lcm_last_launch_info: the two kernels added to launches and to aux_kernel_ms. */
struct lcm_pose_params;
struct lcm_pose_result;
LCM_API extern int lcm_lo_db_verify_pairs(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio,
                                          const lcm_epi_params* ep, const lcm_lo_params* lp, const struct lcm_pose_params* pp,
                                          lcm_epi_result* results, lcm_lo_info* info, struct lcm_pose_result* pose_results,
                                          lcm_dmatch* out, lcm_point_pair* pts, uint8_t* mask, uint8_t* pose_mask, size_t cap,
                                          size_t* offsets);
/* lcm_pose_db_detect_loops (declared below) likewise: info holds cand_cap records, *best = lcm_pose_best over the optimised
 * records. */
LCM_API extern int lcm_lo_db_detect_loops(lcm_handle* h, int curr, const uint8_t* query, const float* query_pts, int nq,
                                          const uint8_t* skip, int loop_gap, const struct lcm_ratio_loop_params* rp,
                                          const lcm_epi_params* ep, const lcm_lo_params* lp, const struct lcm_pose_params* pp,
                                          lcm_loop_candidate* cands, size_t cand_cap, size_t* n_cands, size_t* n_pairs_out,
                                          lcm_epi_result* results, lcm_lo_info* info, struct lcm_pose_result* pose_results,
                                          lcm_dmatch* out, lcm_point_pair* pts, uint8_t* mask, uint8_t* pose_mask, size_t cap,
                                          size_t* offsets, int floor_inliers, int* best);

/* ---- the loop's relative pose on the device, and the best loop ------------------------------------------------------------ */
/* src/main.cpp:1405-1421: poseInliers = recoverPose(E, ptsCurr, ptsPast, K, R_loop, t_loop, mask), the verdict
 * `poseInliers > 100`, and the globalBest* update.  This is NOT cv::recoverPose bit for bit (OpenCV decomposes by SVD and
 * triangulates by a 4 x 4 DLT per point).  Every step here is +, -, x, / and a square root in double, every product and sum
 * rounded on its own, sums left to right (lcm_pose_device.h):
 *   convention   the RANSAC's: query x1 = (a, b, 1), train x2 = (c, d, 1), normalised as above; x2^T E x1 = 0, E = [t]x R,
 *                that is X2 = R X1 + t with |t| = 1 (the argument order of :1407)
 *   scale        e = E * sqrt(2 / |E|^2_F): the RANSAC's E and a caller's take one path.  A caller's E must be essential; it
 *                is not projected.  |E|^2_F zero, NaN or outside the range in which that scale is finite, or an e without
 *                two independent columns: LCM_POSE_NO_MODEL (so after LCM_EPI_TOO_FEW and after a pair without an inlier)
 *   translation  c0 = col1 x col2, c1 = col2 x col0, c2 = col0 x col1 of e; the one with the largest squared norm, first of
 *                equals: t^ = c_k / sqrt(|c_k|^2).  No sign canonicalisation
 *   rotations    C = the cofactor matrix of e (row 0 = row1 x row2, row 1 = row2 x row0, row 2 = row0 x row1), M = [t^]x e:
 *                Ra = C - M, Rb = C + M
 *   hypotheses   k = 0 .. 3: R = (k & 1) ? Rb : Ra, t = (k & 2) ? -t^ : t^
 *   depth test   u = R x1, v = x2; uu = u.u, vv = v.v, uv = u.v, ut = u.t, vt = v.t; D = uu vv - uv uv, n1 = uv vt - vv ut,
 *                n2 = uu vt - uv ut (n1 / D, n2 / D: the least-squares depths of the two rays).  In front of both cameras:
 *                D > 0 && n1 > 0 && n2 > 0 && n1 < max_depth D && n2 < max_depth D.  No division
 *   records      only those whose input mask byte is non-zero take part (no mask: all)
 *   selection    the largest of the four counts, among equals the lowest k; mask_out = 1 where a record took part and passes
 *                under the chosen k; n_good = their number = counts[choice]: poseInliers of :1407
 * t has the sign that puts the points in front.  R, t inherit the quality of E: the eight-point E is a minimal-sample estimate. */
typedef struct lcm_pose_params {
    double  max_depth;          /* 50.0: OpenCV's distanceThresh, in units of the baseline; <= 0 or NaN is LCM_ERR_INVALID_ARG */
    int32_t min_pose_inliers;   /* 100:  lcm_pose_loop_test */
    int32_t reserved[5];
} lcm_pose_params;              /* 32 bytes */
typedef enum lcm_pose_status { LCM_POSE_OK = 0, LCM_POSE_NO_MODEL = 1 } lcm_pose_status;
typedef struct lcm_pose_result {
    double  R[9];               /* row-major */
    double  t[3];               /* unit */
    int32_t counts[4];          /* records in front of both cameras under each hypothesis */
    int32_t n_used, n_good, choice, status;      /* records that took part; counts[choice]; k */
} lcm_pose_result;              /* 128 bytes.  LCM_POSE_NO_MODEL: all zero but choice = -1 and status, and an all-zero mask */
LCM_API void lcm_pose_params_default(lcm_pose_params* p);
/* Host only: lcm_epi_loop_test(er, ep) && pr->status == LCM_POSE_OK && pr->n_good > pp->min_pose_inliers, strict (:1409).
 * pp == NULL: the defaults (in every call of the family); 0 for any other NULL. */
LCM_API int  lcm_pose_loop_test(const lcm_epi_result* er, const lcm_pose_result* pr, const lcm_epi_params* ep,
                                const lcm_pose_params* pp);
/* Host only: *best = the index of the candidate with the largest n_inliers > floor_inliers among those of the n that pass
 * lcm_pose_loop_test, among equals the lowest index; -1 when there is none.  Walked in (curr, past) order this is the
 * reference's globalBest* update (a candidate that fails the pose test does not raise the maximum there either): the caller
 * carries floor_inliers = the best n_inliers so far from keyframe to keyframe, starting at -1. */
LCM_API int  lcm_pose_best(const lcm_epi_result* epi_results, const lcm_pose_result* pose_results, int n, const lcm_epi_params* ep,
                           const lcm_pose_params* pp, int floor_inliers, int* best);
/* Point lists and matrices verified elsewhere, in lcm_epi_verify_pairs's layout: pair p owns pts[offsets[p] .. offsets[p + 1])
 * and E[9 p .. 9 p + 9).  mask_in (may be NULL: every record) and mask_out (may be NULL): offsets[n_pairs] bytes.  ep supplies
 * K only.  Refusals as lcm_epi_verify_pairs's.  lcm_last_launch_info: kernel_ms is the kernel's. */
LCM_API int  lcm_pose_recover_pairs(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs, const double* E,
                                    const uint8_t* mask_in, const lcm_epi_params* ep, const lcm_pose_params* pp,
                                    lcm_pose_result* results, uint8_t* mask_out);
/* Test seam: the decomposition alone, on the device.  Model m of E = n_models x 9 gives R4[36 m ..] = 4 x 9 and
 * t4[12 m ..] = 4 x 3 (hypothesis k at 9 k and 3 k) and status[m]; all zero for LCM_POSE_NO_MODEL. */
LCM_API int  lcm_pose_candidates(lcm_handle* h, const double* E, int n_models, double* R4, double* t4, int32_t* status);
/* lcm_epi_db_verify_pairs followed by the pose recovery on the records, matrices and mask the RANSAC has just written, before
 * anything is copied back: everything lcm_epi_db_verify_pairs returns is returned byte for byte; pose_results (n_pairs) and
 * pose_mask (`cap` bytes, may be NULL) as lcm_pose_recover_pairs's on the returned points, E and mask.  `cap` too small: as
 * there, and nothing new is written either.  lcm_last_launch_info: one more launch, inside aux_kernel_ms. */
LCM_API int  lcm_pose_db_verify_pairs(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio, const lcm_epi_params* ep,
                                      const lcm_pose_params* pp, lcm_epi_result* results, lcm_pose_result* pose_results,
                                      lcm_dmatch* out, lcm_point_pair* pts, uint8_t* mask, uint8_t* pose_mask, size_t cap,
                                      size_t* offsets);
/* lcm_epi_db_detect_loops plus the pose recovery and the choice: one iteration of the reference's outer loop through :1421.
 * pose_results: cand_cap records.  *best = lcm_pose_best over the call's candidates with floor_inliers (-1 before the first
 * keyframe; afterwards the n_inliers of the best loop so far), or -1; it is written only when the call succeeds. */
LCM_API int  lcm_pose_db_detect_loops(lcm_handle* h, int curr, const uint8_t* query, const float* query_pts, int nq,
                                      const uint8_t* skip, int loop_gap, const struct lcm_ratio_loop_params* rp,
                                      const lcm_epi_params* ep, const lcm_pose_params* pp, lcm_loop_candidate* cands,
                                      size_t cand_cap, size_t* n_cands, size_t* n_pairs_out, lcm_epi_result* results,
                                      lcm_pose_result* pose_results, lcm_dmatch* out, lcm_point_pair* pts, uint8_t* mask,
                                      uint8_t* pose_mask, size_t cap, size_t* offsets, int floor_inliers, int* best);

/* ---- closing the loop: pose-graph Gauss-Newton correction on the device --------------------------------------------------- */
/* src/main.cpp:1429-1491: the pose graph of :1441-1470, optimizePoseGraph (:282-445) and the drift of :1476-1480.  The
 * reference takes a central-difference Jacobian over all 6 (N - 1) parameters, re-evaluates every edge per column and solves a
 * dense system; a column is exactly zero outside the two poses of an edge, so the twelve columns per edge computed here ARE
 * its Jacobian, and the solve is an exact block Cholesky of the same matrix (lcm_pgo_device.h, lcm_pgo.hip).
 * In double, every product and sum rounded on its own, sums left to right:
 *   conventions  a pose is world-to-camera, Xc = R Xw + t (R row-major); an edge says R_to = R_rel R_from,
 *                t_to = R_rel t_from + t_rel (:78-86)
 *   parameters   pose 0 is fixed; pose i >= 1 has p_i = (log R_i, t_i), the rotation vector and the translation
 *   exp(r)       theta = sqrt(r . r); theta < DBL_EPSILON: I; else k = r / theta and
 *                R = cos(theta) I + (1 - cos(theta)) k k^T + sin(theta) [k]x
 *   log(R)       v = (R21 - R12, R02 - R20, R10 - R01) / 2, s = sqrt(v . v), c = (trace - 1) / 2 clamped to [-1, 1];
 *                s >= 1e-5: v atan2(s, c) / s;  s < 1e-5 and c > 0: v itself;  s < 1e-5 and c <= 0: the run ends with
 *                LCM_PGO_HALF_TURN.  R is taken as a rotation and is not projected.  This is NOT cv::Rodrigues bit for bit:
 *                OpenCV returns an exact zero vector below s = 1e-5, which, as the sequential edges are built from the poses
 *                themselves and eps = 1e-6, makes every sequential edge's rotational Jacobian exactly zero in iteration 0.
 *                The first-order branch removes that artefact and changes nothing for s >= 1e-5.
 *   residual     of edge e (:358-381), w = sqrt(weight): r[0..3) = w log((R_rel R_from)^T R_to),
 *                r[3..6) = w (t_to - (R_rel t_from + t_rel))
 *   Jacobian     per edge twelve columns, the six parameters of `from`, then of `to`; a column is
 *                (r(p + eps e_c) - r(p - eps e_c)) / (2 eps).  The columns of pose 0 are not parameters (zero in `jac`).
 *   normal eq.   H = sum_e J_e^T J_e, g = sum_e J_e^T r_e, each 6 x 6 block and 6-vector one running sum over its edges in
 *                ascending edge order, within an edge over the residual's rows; lambda = damping trace(H) / (6 (n_poses - 1)):
 *                the divisor counts every pose but pose 0, valid or not, as the reference's numParams does; H += lambda I;
 *                H dp = -g by Cholesky.  A pivot that is not > 0 (NaN included) ends the run BEFORE the update with
 *                LCM_PGO_SOLVE_FAILED (the reference's !ok branch).
 *   update       p += dp, max_update = max |dp_k|, cost = r . r of the iteration's residuals before the update (:426-440);
 *                max_update < min_update ends the run as LCM_PGO_CONVERGED after that iteration, max_iters iterations
 *                without it as LCM_PGO_MAX_ITERS
 *   write-back   pose 0 byte for byte; every other valid pose as exp of its rotation parameters and its t (:316-324).  An
 *                invalid pose is returned byte for byte: the reference turns an empty pose into the identity, this library
 *                keeps validity as a byte per pose (valid[i] != 0) and leaves such a pose alone; its contents are not read.
 *                LCM_PGO_HALF_TURN before any update: every pose byte for byte.
 * Limits: n_poses <= LCM_PGO_MAX_POSES.  An edge with |from - to| == 1 is a chain edge, any other a loop edge, at most
 * LCM_PGO_MAX_LOOPS of them; the border is the set of poses >= 1 that end a loop edge (at most 16).  With the unknowns ordered
 * interior poses first, border poses last, H is block-tridiagonal with a border of at most 96 columns, and device memory grows
 * as O(n_poses x border).  Duplicate edges add.  A valid pose no edge reaches gets dp = 0. */
#define LCM_PGO_MAX_POSES 4096
#define LCM_PGO_MAX_LOOPS 8
typedef struct lcm_pgo_pose { double R[9]; double t[3]; } lcm_pgo_pose;                       /* 96 bytes, R row-major */
typedef struct lcm_pgo_edge { double R[9]; double t[3]; double weight; int32_t from, to; } lcm_pgo_edge;   /* 112 bytes */
typedef enum lcm_pgo_loop_direction { LCM_PGO_LOOP_AS_WRITTEN = 0, LCM_PGO_LOOP_INVERTED = 1 } lcm_pgo_loop_direction;
typedef struct lcm_pgo_params {  /* defaults = the reference's constants */
    double eps;                  /* 1e-6: the central difference's step, finite and > 0 */
    double damping;              /* 1e-4: finite and >= 0 */
    double min_update;           /* 1e-6: finite and >= 0; 0 never converges (every iteration runs) */
    double loop_weight;          /* 10.0: the loop edge's weight in lcm_pgo_build_graph / lcm_pgo_close_loop, finite and >= 0 */
    int32_t max_iters;           /* 20, in [1, 100] */
    int32_t loop_direction;      /* lcm_pgo_loop_direction: lcm_pgo_close_loop only, see there */
    int32_t reserved[6];         /* ignored */
} lcm_pgo_params;                /* 64 bytes */
typedef enum lcm_pgo_status { LCM_PGO_CONVERGED = 0, LCM_PGO_MAX_ITERS = 1, LCM_PGO_SOLVE_FAILED = 2, LCM_PGO_HALF_TURN = 3 } lcm_pgo_status;
typedef struct lcm_pgo_info {
    double cost_first, cost_last;     /* r . r of the first and of the last linearisation made (a failed solve's included) */
    double max_update, lambda;        /* max |dp_k| of the last update applied; the damping of the last linearisation made */
    int32_t iterations;               /* updates applied */
    int32_t status;                   /* lcm_pgo_status */
    int32_t n_params;                 /* 6 x (valid poses other than pose 0): the unknowns solved for */
    int32_t n_border;                 /* border poses */
} lcm_pgo_info;                       /* 48 bytes */
LCM_API void lcm_pgo_params_default(lcm_pgo_params* p);
/* The whole of optimizePoseGraph.  valid: one byte per pose, NULL = all valid; pp NULL = the defaults; poses_out (n_poses
 * records) may alias poses.  Refused with LCM_ERR_INVALID_ARG before anything is launched or written: a NULL buffer,
 * n_poses < 2, n_edges < 1, pose 0 invalid, an edge with from == to, an index out of range or an invalid endpoint, a weight
 * that is negative or not finite, a non-finite double in a valid pose or an edge, a pose or edge R with max |R R^T - I| > 1e-6
 * or a negative determinant, a bad pp field; LCM_ERR_CAPACITY above the limits.  Ordered on the handle's stream and finished on
 * return; lcm_last_launch_info: kernel_ms, launches, pairs = n_edges.  The same call gives the same bytes: no sum's order
 * depends on scheduling. */
LCM_API int  lcm_pgo_optimize(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_pgo_edge* edges,
                              int n_edges, const lcm_pgo_params* pp, lcm_pgo_pose* poses_out, lcm_pgo_info* info);
/* The test seam: exactly one iteration from the given poses through the kernels lcm_pgo_optimize launches (pp is checked whole;
 * max_iters is not used).  params_out: 6 n_poses doubles, the parameters before the update (pose 0's slot: its log where that exists, else
 * v, and its t; an invalid pose's: zeros); residuals: 6 n_edges; jac: n_edges x 6 x 12 row-major; dp: 6 (n_poses - 1), zero
 * for invalid poses.  info as lcm_pgo_optimize's with max_iters = 1. */
LCM_API int  lcm_pgo_step(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_pgo_edge* edges,
                          int n_edges, const lcm_pgo_params* pp, double* params_out, double* residuals, double* jac, double* dp,
                          lcm_pgo_info* info);
/* Host only (:1441-1470): one edge of weight 1 per pair of poses i - 1, i that are both valid, from the poses
 * (R_rel = R_i R_{i-1}^T, t_rel = t_i - R_rel t_{i-1}), then the loop edge from = past, to = curr with (R_loop, t_loop) and
 * pp->loop_weight.  *n_edges = the edges the graph has; more than cap: LCM_ERR_CAPACITY and nothing written to edges_out. */
LCM_API int  lcm_pgo_build_graph(const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, int past, int curr, const double* R_loop,
                                 const double* t_loop, const lcm_pgo_params* pp, lcm_pgo_edge* edges_out, int cap, int* n_edges);
/* Host only (:1476-1480): *angle = |log(R_loop (R_curr R_past^T)^T)| in radians, with the log above (at half a turn:
 * atan2(s, c)).  It serves the "before" and the "after" print. */
LCM_API int  lcm_pgo_rotation_drift(const lcm_pgo_pose* poses, int n_poses, int past, int curr, const double* R_loop, double* angle);
/* Host only: simplePoseCorrection (:451-492), the reference's other PoseGraphMethod.  With rvec = log(R_loop (R_curr R_past^T)^T),
 * every valid pose f in (past, curr] gets R_f <- exp(rvec (f - past) / (curr - past)) R_f; everything else is copied.  past < curr;
 * half a turn of error is refused (LCM_ERR_INVALID_ARG).  poses_out may alias poses. */
LCM_API int  lcm_pgo_linear_correct(const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, int past, int curr,
                                    const double* R_loop, lcm_pgo_pose* poses_out);
/* lcm_pgo_build_graph on pr's R and t followed by lcm_pgo_optimize; a pr whose status is not LCM_POSE_OK is refused.
 * pp->loop_direction says how pr becomes the edge.  lcm_pose_* returns X_past = R X_curr + t (query = curr, the argument order of
 * :1407, what cv::recoverPose(E, ptsCurr, ptsPast, ...) returns), and :1464-1467 puts that pair UNCHANGED on an edge whose own
 * definition is past -> curr.  LCM_PGO_LOOP_AS_WRITTEN (0, the default) reproduces the reference's lines: R_rel = R, t_rel = t.
 * LCM_PGO_LOOP_INVERTED (1) uses (R^T, -R^T t), the geometrically consistent reading.  The unit t against the trajectory's scale
 * stays the caller's concern, as in the reference. */
LCM_API int  lcm_pgo_close_loop(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, int past, int curr,
                                const lcm_pose_result* pr, const lcm_pgo_params* pp, lcm_pgo_pose* poses_out, lcm_pgo_info* info);

/* ---- after the loop: alternating bundle adjustment and outlier removal on the device -------------------------------------- */
/* src/main.cpp:1494-1669: the loop's inlier matches become observations of existing points (:1494-1513), the mean
 * reprojection error (:1543, computeReprojectionError :871-896), alternatingBundleAdjustment (:1546, :905-943: the pose-only
 * Gauss-Newton step refineCameraPoseGN :632-743 and the point-only step refinePointGN :757-858), the outlier flags and the
 * compaction (:1563-1659) and the second adjustment (:1666).  With the points fixed every camera is independent of every other,
 * and with the poses fixed so is every point: a phase runs all its elements at once and gives what the reference's sequential
 * loops over camIdx / ptIdx give (lcm_ba_device.h, lcm_ba.hip).  In double, every product and sum rounded on its own:
 *   projection   (:149-165) Xc = (R Xw) + t, each row of the product summed left to right; u = ((fx x) / z) + cx,
 *                v = ((fy y) / z) + cy.  There is no test on z, as in the reference.  residual = projection - pixel.
 *   cameras      per valid camera with at least min_cam_obs observations: p = (log R, t), exp and log those of the pose graph
 *                above, the same stated departure from cv::Rodrigues below a sine of 1e-5 included.  The camera's observations
 *                are taken in ascending index of the caller's list.  Each iteration: the residuals r; the six columns
 *                (r(p + eps e_k) - r(p - eps e_k)) * (0.5 / eps), the rotation rebuilt by exp once per camera, iteration and
 *                parameter vector; H = J^T J, g = J^T r, H_kk += damping (absolute, not scaled by the trace as the pose
 *                graph's), H dp = -g by Cholesky.  A pivot that is not > 0 (NaN included) ends the element BEFORE the update as
 *                LCM_BA_SOLVE_FAILED; otherwise p += dp, and max |dp_k| < min_update ends it after the update as
 *                LCM_BA_CONVERGED, inner_iters updates without that as LCM_BA_MAX_ITERS.
 *   write-back   R = exp(p[0..3)), t = p[3..6) for every status but LCM_BA_HALF_TURN: the reference writes paramsToPose(p) back
 *                even when no update was applied.  A camera whose R has no rotation vector (LCM_BA_HALF_TURN) and a skipped one
 *                (LCM_BA_SKIPPED: fewer than min_cam_obs observations, or valid[i] == 0) come back byte for byte.
 *   points       the same with p = (x, y, z), three columns and a 3 x 3 system; a point with fewer than min_point_obs
 *                observations is LCM_BA_SKIPPED and comes back byte for byte, every other point as its p.
 *   sums         the order of the sums in H and g over an element's observations is fixed and stated in lcm_ba.hip's header;
 *                the same call gives the same bytes, and an element's k-th iteration depends neither on min_update nor on
 *                inner_iters.
 *   mean error   (:871-896) the sum of sqrt(dx dx + dy dy) over all observations in a fixed order, divided by their number;
 *                0.0 for no observation.
 *   outliers     (:1563-1619) per point: an observation with Xc.z <= 0 flags the point and does not enter the maximum; otherwise
 *                its error enters the point's max_err, and err > outlier_px flags the point.  The centroid of the valid cameras'
 *                centres -R^T t and the largest distance of a centre from it are computed on the host;
 *                threshold = max(min_spread, spread_factor x that distance); a point farther than the threshold from the
 *                centroid is flagged.
 * A map is (poses, valid, n_poses, points, n_points, obs, n_obs): valid is one byte per pose, NULL = all valid, and an invalid
 * pose's contents are not read.  Refused by every call over a map with LCM_ERR_INVALID_ARG before anything is launched or
 * written: a NULL buffer, pp == NULL (the camera matrix has no default), n_poses < 1, n_points < 1, n_obs < 0, an observation
 * index out of range, an observation of an invalid camera, a non-finite double in a valid pose, a point or an observation, a
 * pose R with max |R R^T - I| > 1e-6 or a negative determinant, a bad pp field; LCM_ERR_CAPACITY above the limits, decided from
 * the counts before any buffer is read.  Ordered on the handle's stream and finished on return; lcm_last_launch_info:
 * kernel_ms, launches, pairs = n_obs. */
#define LCM_BA_MAX_CAMERAS 4096
#define LCM_BA_MAX_POINTS 16777216
#define LCM_BA_MAX_OBS 16777216
#define LCM_BA_MAX_ITERS_PER_LOOP 16
typedef struct lcm_ba_point { double x, y, z; } lcm_ba_point;                                 /* 24 bytes */
typedef struct lcm_ba_obs { int32_t cam, point; double u, v; } lcm_ba_obs;                    /* 24 bytes */
typedef enum lcm_ba_status { LCM_BA_CONVERGED = 0, LCM_BA_MAX_ITERS = 1, LCM_BA_SOLVE_FAILED = 2, LCM_BA_HALF_TURN = 3,
                             LCM_BA_SKIPPED = 4 } lcm_ba_status;
typedef struct lcm_ba_elem_info {     /* one per camera or per point */
    double last_update;               /* max |dp_k| of the last update applied, 0 if none */
    double cost;                      /* r . r of the last linearisation made (a failed solve's included), 0 if none */
    int32_t iterations;               /* updates applied */
    int32_t status;                   /* lcm_ba_status */
} lcm_ba_elem_info;                   /* 24 bytes */
typedef struct lcm_ba_params {        /* defaults = the reference's constants */
    double fx, fy, cx, cy;            /* the camera matrix K; the defaults leave it zero: fx <= 0 or fy <= 0 is LCM_ERR_INVALID_ARG */
    double eps;                       /* 1e-6: the central difference's step, finite and > 0 */
    double damping;                   /* 1e-3: added to H's diagonal, finite and >= 0 */
    double min_update;                /* 1e-6: finite and >= 0; 0 never converges (every iteration runs) */
    double outlier_px;                /* 5.0:  OUTLIER_REPROJ_THRESHOLD */
    double min_spread;                /* 10.0: the distance threshold's floor */
    double spread_factor;             /* 5.0:  ... and its multiple of the cameras' spread */
    int32_t outer_iters;              /* 5, in [1, 16]: lcm_ba_optimize's (camera phase, point phase, mean error) rounds */
    int32_t inner_iters;              /* 5, in [1, 16]: Gauss-Newton iterations per element and phase */
    int32_t min_cam_obs;              /* 10 */
    int32_t min_point_obs;            /* 2 */
    int32_t reserved[4];              /* ignored */
} lcm_ba_params;                      /* 112 bytes */
typedef struct lcm_ba_info {
    double mean_error[17];            /* [0] before the run, [k] after outer iteration k; unused entries are 0 */
    int32_t outer_iters;              /* rounds run */
    int32_t cameras[5];               /* cameras per lcm_ba_status after the last outer iteration */
    int32_t points[5];                /* points per lcm_ba_status after the last outer iteration */
    int32_t reserved;
} lcm_ba_info;                        /* 184 bytes */
typedef struct lcm_ba_map_report {    /* lcm_ba_refine_map */
    double error_before, error_after; /* :1543, :1554: around the first adjustment */
    double error_filtered, error_final;   /* :1663, :1668: around the second */
    double threshold;                 /* the outlier pass's distance threshold */
    int32_t n_outliers;               /* points flagged */
    int32_t n_points, n_obs;          /* what the compaction kept */
    int32_t reserved;
} lcm_ba_map_report;                  /* 56 bytes */
LCM_API void lcm_ba_params_default(lcm_ba_params* p);
/* computeReprojectionError: *mean, and with obs_err != NULL one error per observation (n_obs doubles) in the caller's order. */
LCM_API int  lcm_ba_error(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points,
                          int n_points, const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, double* mean, double* obs_err);
/* One phase: every camera (every point) at once.  poses_out: n_poses records (points_out: n_points), may alias the input;
 * info: one record per camera (per point).  outer_iters is not used. */
LCM_API int  lcm_ba_refine_cameras(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points,
                                   int n_points, const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, lcm_pgo_pose* poses_out,
                                   lcm_ba_elem_info* info);
LCM_API int  lcm_ba_refine_points(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points,
                                  int n_points, const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, lcm_ba_point* points_out,
                                  lcm_ba_elem_info* info);
/* The test seam: one linearisation of every element through the kernels the phases launch (pp is checked whole; inner_iters and
 * outer_iters are not used).  r: 2 n_obs doubles and J: n_obs x 2 x 6 (points: n_obs x 2 x 3) row-major, in the caller's order,
 * zero for an observation of an element that was not linearised; H: n_poses x 6 x 6 (n_points x 3 x 3) BEFORE damping, g and dp:
 * 6 per camera (3 per point), zero for such an element, dp zero after a failed solve; info as the phase's with inner_iters = 1. */
LCM_API int  lcm_ba_step_cameras(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points,
                                 int n_points, const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, double* r, double* J, double* H,
                                 double* g, double* dp, lcm_ba_elem_info* info);
LCM_API int  lcm_ba_step_points(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points,
                                int n_points, const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, double* r, double* J, double* H,
                                double* g, double* dp, lcm_ba_elem_info* info);
/* alternatingBundleAdjustment: the mean error, then outer_iters x (camera phase, point phase, mean error), every launch enqueued
 * back to back on the handle's stream; only poses_out, points_out, the element infos of the last round (cam_info: n_poses,
 * pt_info: n_points; each may be NULL) and *info come back.  The outputs may alias the inputs. */
LCM_API int  lcm_ba_optimize(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points,
                             int n_points, const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, lcm_pgo_pose* poses_out,
                             lcm_ba_point* points_out, lcm_ba_elem_info* cam_info, lcm_ba_elem_info* pt_info, lcm_ba_info* info);
/* The outlier flags: flags (one byte per point, 1 = outlier) and max_err (one double per point, may be NULL), *threshold (may
 * be NULL) and *n_outliers. */
LCM_API int  lcm_ba_outliers(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points,
                             int n_points, const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, uint8_t* flags, double* max_err,
                             double* threshold, int* n_outliers);
/* Host only (:1633-1659): the points with flags[i] == 0 in order, the observations of such points in order with the new point
 * index, old_to_new (n_points entries, -1 for a removed point; may be NULL).  *n_points_out and *n_obs_out are the counts; if
 * they exceed cap_points / cap_obs: LCM_ERR_CAPACITY and nothing else is written.  An observation's point index out of range is
 * LCM_ERR_INVALID_ARG.  The outputs must not alias the inputs. */
LCM_API int  lcm_ba_compact(const lcm_ba_point* points, int n_points, const lcm_ba_obs* obs, int n_obs, const uint8_t* flags,
                            lcm_ba_point* points_out, int cap_points, lcm_ba_obs* obs_out, int cap_obs, int32_t* old_to_new,
                            int* n_points_out, int* n_obs_out);
/* Host only (:1496-1513).  matches / mask (n_matches records and bytes): the match list and the mask of the best candidate as
 * lcm_pose_db_detect_loops returns them (query_idx: the current frame's keypoint, train_idx: the past frame's).  past_table
 * (n_past_kp entries): the past frame's keypoint -> point index, -1 = none; curr_table (n_curr_kp entries): the current
 * frame's, updated in place; curr_kp: the current frame's keypoints, n_curr_kp (x, y) pairs of floats.  For every masked match
 * whose past keypoint has a point, in order, {curr, point, pixel} is appended at obs[n_obs ...] (obs has room for cap records
 * in all) and curr_table[query_idx] = point.  *n_added = their number; n_obs + *n_added > cap: LCM_ERR_CAPACITY and nothing is
 * written but *n_added.  An index outside its list or a table entry outside [-1, n_points) is LCM_ERR_INVALID_ARG. */
LCM_API int  lcm_ba_add_loop_observations(const lcm_dmatch* matches, const uint8_t* mask, int n_matches, const int32_t* past_table,
                                          int n_past_kp, int32_t* curr_table, const float* curr_kp, int n_curr_kp, int curr,
                                          int n_points, lcm_ba_obs* obs, int n_obs, int cap, int* n_added);
/* :1543-1669 in one call: lcm_ba_error, lcm_ba_optimize with pp->outer_iters, lcm_ba_outliers, lcm_ba_compact, lcm_ba_error,
 * lcm_ba_optimize with second_outer_iters (<= 0: 3, the reference's; at most 16), lcm_ba_error.  poses_out: n_poses records;
 * points_out: n_points; obs_out: n_obs; old_to_new: n_points entries or NULL; the outputs must not alias the inputs.  The kept
 * counts are report->n_points and report->n_obs.  If the outlier pass keeps no point the call ends after the compaction with
 * error_filtered = error_final = 0.  The inputs are refused before anything is written; should the first adjustment leave a
 * non-finite value behind (an element that diverged), the later steps refuse it with LCM_ERR_INVALID_ARG after poses_out has
 * been written, and *report is not.  lcm_last_launch_info describes the last step that launched. */
LCM_API int  lcm_ba_refine_map(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points,
                               int n_points, const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, int second_outer_iters,
                               lcm_pgo_pose* poses_out, lcm_ba_point* points_out, lcm_ba_obs* obs_out, int32_t* old_to_new,
                               lcm_ba_map_report* report);

/* ---- before the loop: the map (keyframe gates, triangulation, filters, merge) on the device -------------------------------- */
/* src/main.cpp:1152-1351: what builds the 3-D points, the observation list and the keypoint -> point tables that the calls above
 * take.  A pair is (view 1 = the last keyframe = the match's query side, view 2 = the new keyframe = the train side) with
 * world-to-camera poses P1, P2 (lcm_pgo_pose) and records lcm_point_pair {qx, qy, tx, ty}, one mask byte each.  The loop over
 * the matches (:1261-1341) is a filter per record, an ordered compaction and a last-writer scatter: a knnMatch list holds every
 * query_idx once, so a record's table look-up depends on no earlier record and its new point index is the number of new points
 * before it (lcm_map_device.h, lcm_map.hip).  In double, every product and sum rounded on its own (no contraction
 * into fused multiply-adds), row sums left to right:
 *   per pair      on the host (lcm_map_host.h), returned in lcm_map_pair_info: C_i = -(R_i^T t_i);
 *                 baseline = sqrt(sum of squares of C2 - C1); the 3 x 4 matrices K [R_i | t_i], row 0 = fx row0 + cx row2,
 *                 row 1 = fy row1 + cy row2, row 2 = row2 of [R_i | t_i]; cos_min = cos(min_parallax_deg * pi / 180)
 *   mask          mask byte 0: LCM_MAP_NOT_INLIER (mask == NULL: every record takes part)
 *   triangulation cv::triangulatePoints' system: the rows of A are x1 P1[2] - P1[0], y1 P1[2] - P1[1], x2 P2[2] - P2[0],
 *                 y2 P2[2] - P2[1] with the coordinates the floats converted to double; M = A^T A, its ten sums over the four rows
 *                 in that order; the homogeneous point is the eigenvector of M's smallest eigenvalue by a cyclic Jacobi over the
 *                 six pairs (p, q) in lexicographic order with a fixed number of sweeps (the local optimisation's rotation
 *                 formulae), the column of the smallest diagonal entry, first of equals.  Stated departures from OpenCV: there
 *                 is no SVD, and the vector is not rounded to float (OpenCV returns CV_32F, which :1268-1273 reads)
 *   point         |w| < 1e-9: LCM_MAP_NO_POINT (:1269); otherwise X = (x / w, y / w, z / w)
 *   depth         depth_i = (R_i X + t_i).z; depth1 <= 0 || depth2 <= 0: LCM_MAP_REJ_DEPTH; rel = depth1 / baseline,
 *                 rel < min_depth || rel > max_depth: LCM_MAP_REJ_DEPTH.  IEEE decides at baseline == 0, as in the reference
 *   parallax      (:200-222) the rays X - C_i and their norms; a norm < 1e-9 is parallax 0 and rejected (cos_parallax = 1);
 *                 otherwise c = the dot product of the two normalised rays clamped to [-1, 1]; c > cos_min:
 *                 LCM_MAP_REJ_PARALLAX.  Stated departure: the cosine is compared and there is no acos, so a record whose angle
 *                 lies within rounding of the threshold may fall on the other side
 *   reprojection  (:227-246) err_i as computeSingleReprojError, 1e9 at z <= 0; err1 > max_reproj || err2 > max_reproj:
 *                 LCM_MAP_REJ_REPROJ; otherwise LCM_MAP_ACCEPTED
 * Each record gives one status byte and one lcm_map_tri; every field of it is computed for every record that has a point,
 * rejected or not, and all are zero for LCM_MAP_NOT_INLIER and LCM_MAP_NO_POINT.  The same call gives the same bytes.
 * Limits: LCM_MAP_MAX_PAIRS pairs and LCM_MAP_MAX_RECORDS records per call, LCM_ERR_CAPACITY above them, decided from the counts
 * before any buffer is read.  Ordered on the handle's stream and finished on return; lcm_last_launch_info: kernel_ms, launches,
 * pairs = records. */
#define LCM_MAP_MAX_PAIRS 4096
#define LCM_MAP_MAX_RECORDS 16777216
typedef enum lcm_map_status { LCM_MAP_NOT_INLIER = 0, LCM_MAP_NO_POINT = 1, LCM_MAP_REJ_DEPTH = 2, LCM_MAP_REJ_PARALLAX = 3,
                              LCM_MAP_REJ_REPROJ = 4, LCM_MAP_ACCEPTED = 5, LCM_MAP_MERGED = 6, LCM_MAP_NEW = 7 } lcm_map_status;
typedef enum lcm_map_verdict { LCM_MAP_KEYFRAME = 0, LCM_MAP_FEW_MATCHES = 1, LCM_MAP_LITTLE_MOTION = 2, LCM_MAP_MUCH_MOTION = 3,
                               LCM_MAP_NO_POSE = 4, LCM_MAP_FEW_INLIERS = 5 } lcm_map_verdict;
typedef struct lcm_map_params {       /* defaults = the reference's constants (:38-48) */
    double fx, fy, cx, cy;            /* the camera matrix K; the defaults leave it zero: fx <= 0 or fy <= 0 is LCM_ERR_INVALID_ARG */
    double min_parallax_deg;          /* 1.0, finite, in [0, 180] */
    double max_reproj;                /* 4.0 px, >= 0 */
    double min_depth, max_depth;      /* 0.1, 50.0: in units of the baseline */
    double min_displacement;          /* 20.0 px: below it LCM_MAP_LITTLE_MOTION */
    double max_displacement;          /* 150.0 px: above it LCM_MAP_MUCH_MOTION */
    double min_inlier_ratio;          /* 0.3 */
    int32_t min_tracked;              /* 100: fewer matches is LCM_MAP_FEW_MATCHES */
    int32_t min_inliers;              /* 50 */
    int32_t min_pose_inliers;         /* 10: estimateRelativePoseFromEssential's (:611) */
    int32_t reserved[3];              /* ignored */
} lcm_map_params;                     /* 112 bytes */
typedef struct lcm_map_tri { double X[3]; double depth1, depth2, cos_parallax, err1, err2; } lcm_map_tri;       /* 64 bytes */
typedef struct lcm_map_pair_info {
    double baseline, cos_min;         /* what the host planner computed for the pair */
    int32_t counts[8];                /* records per lcm_map_status (LCM_MAP_MERGED and LCM_MAP_NEW: 0 here) */
} lcm_map_pair_info;                  /* 48 bytes */
typedef struct lcm_map_keyframe_report {
    lcm_pgo_pose pose;                /* the new keyframe's pose (:1217-1218); zero unless the verdict is LCM_MAP_KEYFRAME */
    double median, baseline;          /* computeMedianDisplacement; the pair's baseline */
    int32_t verdict;                  /* lcm_map_verdict */
    int32_t n_matches, n_inliers;     /* the list's length; countNonZero(inlierMask) (:1191) */
    int32_t n_new, n_merged;          /* points created; observations added to existing points */
    int32_t reserved;
    int32_t counts[8];                /* records per lcm_map_status after the merge */
} lcm_map_keyframe_report;            /* 168 bytes */
LCM_API void lcm_map_params_default(lcm_map_params* p);
/* computeMedianDisplacement (:171-189) per pair, lcm_epi_verify_pairs's layout: dx = (double)(tx - qx) with the subtraction in
 * float as the reference's is, dy likewise, d = sqrt(dx dx + dy dy); median[p] = the element at index n / 2 of the sorted
 * values, 0.0 for an empty pair.  An exact selection (a radix select over the 64-bit patterns, one workgroup per pair), bit for
 * bit what sorting gives.  The coordinates must be finite. */
LCM_API int  lcm_map_median_displacement(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs, double* median);
/* The arithmetic above for many pairs in one launch, one lane per record.  Pair p owns pts[offsets[p] .. offsets[p + 1]), the
 * poses poses1[p] and poses2[p] and info[p]; mask (may be NULL), tri and status: offsets[n_pairs] records.  mp is required (K
 * has no default).  Refused with LCM_ERR_INVALID_ARG before anything is launched or written: a NULL buffer, a bad mp field, a
 * non-finite double in a pose, a pose R with max |R R^T - I| > 1e-6 or a negative determinant, offsets that decrease. */
LCM_API int  lcm_map_triangulate_pairs(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs, const uint8_t* mask,
                                       const lcm_pgo_pose* poses1, const lcm_pgo_pose* poses2, const lcm_map_params* mp,
                                       lcm_map_tri* tri, uint8_t* status, lcm_map_pair_info* info);
/* :1315-1340 for one pair, on the device.  matches, tri, status: n records (status as lcm_map_triangulate_pairs wrote it);
 * table1 (n_kp1 entries) and table2 (n_kp2): the keypoint -> point tables of keyframes kf1 and kf2, -1 = none, updated in place;
 * n_points: the map's points so far.  For every LCM_MAP_ACCEPTED record in list order: if table1[query_idx] != -1 one observation
 * {kf2, that point, (double)tx, (double)ty} is appended and its status becomes LCM_MAP_MERGED; otherwise point n_points + (new
 * points before it) is appended with tri's X, two observations {kf1, idx, q} and {kf2, idx, t} are appended,
 * table1[query_idx] = idx and the status becomes LCM_MAP_NEW; table2[train_idx] = the point in both cases, and where several
 * accepted records share a train_idx the last in list order wins.  points_out receives the *n_new new points (byte for byte tri's
 * X), obs_out the 2 *n_new + *n_merged new observations, status_out (n bytes) every record's status.  pts: the records' pixels.
 * Refused on the host in O(n) before anything is launched or written (LCM_ERR_INVALID_ARG): a list with a repeated query_idx
 * among all its records (the reference's sequential meaning differs there, and a knnMatch list has none), an index outside its
 * table, a table entry outside [-1, n_points), a status byte above LCM_MAP_ACCEPTED.  Too small a cap_points or cap_obs:
 * LCM_ERR_CAPACITY with the needed counts in *n_new and *n_merged and nothing else written. */
LCM_API int  lcm_map_merge(lcm_handle* h, const lcm_dmatch* matches, const lcm_point_pair* pts, const lcm_map_tri* tri, const uint8_t* status,
                           int n, int kf1, int kf2, int32_t* table1, int n_kp1, int32_t* table2, int n_kp2, int n_points,
                           lcm_ba_point* points_out, int cap_points, lcm_ba_obs* obs_out, int cap_obs, uint8_t* status_out, int* n_new,
                           int* n_merged);
/* One iteration of :1152-1351 on host lists: matches and pts (n_matches records, query = the last keyframe kf_last with pose
 * pose_last and table table_last, train = the frame that may become keyframe kf_new, whose table table_new the caller has filled
 * with -1).  In order: n_matches < min_tracked: LCM_MAP_FEW_MATCHES (:1156); the median gates: LCM_MAP_LITTLE_MOTION /
 * LCM_MAP_MUCH_MOTION (:1170, :1176); estimateRelativePoseFromEssential = lcm_epi_verify_pairs followed by
 * lcm_pose_recover_pairs, with lp != NULL lcm_lo_verify_pairs in between: fewer than 8 records, LCM_POSE_NO_MODEL or
 * n_good < min_pose_inliers: LCM_MAP_NO_POSE; the inlier mask is the pose's mask_out (:601-609); n_inliers < min_inliers or
 * n_inliers / n_matches < min_inlier_ratio: LCM_MAP_FEW_INLIERS (:1194); R_new = R R_last, t_new = R t_last + t (:1217-1218);
 * lcm_map_triangulate_pairs and lcm_map_merge.  Every verdict but LCM_MAP_KEYFRAME leaves the tables and the output buffers
 * untouched; the refusals are lcm_map_merge's and the stages', and LCM_ERR_CAPACITY leaves them untouched too (report->n_new and
 * n_merged then hold the needed counts).  status_out (n_matches bytes) may be NULL.  The stages are enqueued on the handle's
 * stream; only the small verdict values (the median, the pose record, the counts) come back between them.  ep: the RANSAC's
 * parameters with the same K; pp may be NULL. */
LCM_API int  lcm_map_add_keyframe(lcm_handle* h, const lcm_dmatch* matches, const lcm_point_pair* pts, int n_matches, int kf_last,
                                  const lcm_pgo_pose* pose_last, int32_t* table_last, int n_kp_last, int kf_new, int32_t* table_new,
                                  int n_kp_new, int n_points, const lcm_map_params* mp, const lcm_epi_params* ep,
                                  const lcm_lo_params* lp, const lcm_pose_params* pp, lcm_ba_point* points_out, int cap_points,
                                  lcm_ba_obs* obs_out, int cap_obs, uint8_t* status_out, lcm_map_keyframe_report* report);
/* The same with the matching included, on the SIFT keyframe store: lcm_pose_db_verify_pairs (lp != NULL: lcm_lo_db_verify_pairs)
 * on the stored pair {last_slot, curr_slot} (matchFeatures(desc[last], currDesc) at :1154 makes the last keyframe the query; its
 * default ratio is 0.75), then the map stages on the records, the matrix and the mask that call left on the device, before the
 * lists are copied back.  The keypoint counts are the slots' rows.  result, info (lp != NULL), pose_result: one record each; out,
 * pts, mask, pose_mask (`cap` records; the masks may be NULL) and offsets (2 entries) come back exactly as that call returns them;
 * the map's arguments and *report exactly as lcm_map_add_keyframe's on those lists.  A frame that is not accepted is removed by the
 * caller with lcm_l2_db_truncate.  `cap` too small: as lcm_pose_db_verify_pairs, and nothing of the map is written either. */
LCM_API int  lcm_map_db_track(lcm_handle* h, int last_slot, int curr_slot, double ratio, const lcm_epi_params* ep, const lcm_lo_params* lp,
                              const lcm_pose_params* pp, lcm_epi_result* result, lcm_lo_info* info, lcm_pose_result* pose_result,
                              lcm_dmatch* out, lcm_point_pair* pts, uint8_t* mask, uint8_t* pose_mask, size_t cap, size_t* offsets,
                              int kf_last, const lcm_pgo_pose* pose_last, int32_t* table_last, int kf_new, int32_t* table_new,
                              int n_points, const lcm_map_params* mp, lcm_ba_point* points_out, int cap_points, lcm_ba_obs* obs_out,
                              int cap_obs, uint8_t* status_out, lcm_map_keyframe_report* report);

/* ---- the front end: SIFT keypoints (scale space, extrema, refinement) ------------------------------------------ */
/* The first half of detectAndDescribeSIFT (src/main.cpp:497-504, called on every frame at :1119 and :1150) on the device: the
 * Gaussian scale space, the difference-of-Gaussians (DoG) layers, the 26-neighbour extrema and the sub-pixel refinement with its
 * contrast and edge tests (lcm_sift_device.h, lcm_sift_host.h, lcm_sift.hip).  The pyramid stays on the device in a
 * lcm_sift_space for the stage that follows.  NOT here, and still the caller's: cv::undistort, the orientation histogram, the
 * 128-D descriptor, retainBest(4000) and the removal of duplicate keypoints; no batches of images, no group form.
 * The contract is the definition below, restated in numpy by tests/siftref.py and held bit for bit.  It is modelled on OpenCV's
 * sift.dispatch.cpp, but parity with cv::SIFT is unpinned: OpenCV is not available to compare with, its blur runs through
 * vectorised filter engines whose summation order is not this one, and its exp / pow are the platform's.
 * All image arithmetic is float32, every product and every sum rounded on its own (no contraction), sums in the stated order.
 *   plan        (host, double; lcm_sift_plan) base = (2 w, 2 h) with upsample, else (w, h); n_octaves = cvRound(log2(min(base_w,
 *               base_h)) - 2) + (upsample ? 1 : 0) unless given (cvRound rounds half to even); octave o has (base_w >> o, base_h >> o)
 *               pixels, n_octave_layers + 3 Gaussian and n_octave_layers + 2 DoG layers.  sig[0] = sigma; sig[i] = sqrt(total^2 -
 *               prev^2), prev = sigma k^(i-1), total = prev k, k = 2^(1 / n_octave_layers).  The first blur's sigma is
 *               sqrt(max(sigma^2 - a^2, 0.01)), a = 2 init_sigma with upsample, else init_sigma.  Taps of a sigma: radius r =
 *               (cvRound(8 sig + 1) | 1) / 2, exp(-(j - r)^2 / (2 sig^2)) for j = 0 .. 2 r in double, divided by their sum taken in
 *               ascending j, then rounded to float.
 *   base image  uint8 -> float; with upsample the 2x bilinear enlargement: source coordinate (d + 0.5) / 2 - 0.5, clamped to the
 *               image, weights 0.25 and 0.75 (exact); then one blur with the first blur's taps gives layer 0 of octave 0.
 *   blur        tmp[y][x] = sum_j t[j] src[y][m(x + j - r)], dst[y][x] = sum_j t[j] tmp[m(y + j - r)][x]; j ascends from 0 and the
 *               sum starts from the first product; m is the reflect-101 index, folded with period 2 (n - 1) until it is inside
 *               (0 for n == 1).  Layer i of an octave is the blur of layer i - 1 with the taps of sig[i].
 *   octaves     layer 0 of octave o + 1 is layer n_octave_layers of octave o at the pixels (2 x, 2 y).  D[l] = G[l + 1] - G[l].
 *   extrema     T = floor(0.5 contrast_threshold / n_octave_layers 255) (double).  At layers 1 .. n_octave_layers and border <= x <
 *               cols - border, border <= y < rows - border: |v| > T and (v > 0 and v >= all 26 neighbours, or v < 0 and v <= all
 *               26).  Candidates come in ascending (octave, layer, row, col) order, by an ordered compaction (block counts, an
 *               exclusive scan, a ballot rank): no atomic cursor, the same bytes every time.
 *   refinement  one candidate at a time, at most max_steps steps.  With s = (float) 1 / 255 (the rounded quotient), at (layer, row,
 *               col): dD = ((D[c+1] - D[c-1]) (0.5 s), (D[r+1] - D[r-1]) (0.5 s), (next - prev) (0.5 s)); dxx = ((D[c+1] + D[c-1]) -
 *               2 v) s, dyy and dss likewise; dxy = (((D[r+1][c+1] - D[r+1][c-1]) - D[r-1][c+1]) + D[r-1][c-1]) (0.25 s), dxs and
 *               dys likewise over (next, prev).  X = -(H^-1 dD) by 3 x 3 Gaussian elimination with partial pivoting (the largest
 *               |.|, the first of equals; f = a_ik / a_kk, a_ij - f a_kj; back substitution from the last row, each row's products
 *               subtracted left to right); a zero pivot rejects.  All |X_i| < 0.5: converged.  Else rejected when an |X_i| >
 *               INT_MAX / 3 (715827882 as a float; a NaN too); else (col, row, layer) += rint(X) (half to even) and rejected when
 *               that leaves layers 1 .. n_octave_layers or the border; rejected when the last step did not converge.  Then contr =
 *               v s + ((dD0 Xc + dD1 Xr) + dD2 Xs) 0.5, rejected when |contr| n_octave_layers < (float) contrast_threshold; tr =
 *               dxx + dyy, det = dxx dyy - dxy dxy at the last position, rejected when det <= 0 or (tr tr) e >= ((e + 1)(e + 1)) det
 *               with e = (float) edge_threshold.  A survivor's record: x = (col + Xc) 2^o and y = (row + Xr) 2^o, halved with
 *               upsample; size = ((float) sigma P(e)) (2^o 2), halved with upsample, where e = (layer + Xs) / n_octave_layers and
 *               P(e) = 2^rint(e) p((e - rint(e)) 0.693147182f), p the Taylor polynomial of exp to the 8th power by Horner with the
 *               coefficients (float)(1 / k!) (only + and x, so that every implementation gives the same bits; within 2 float ulp of
 *               2^e); response = |contr|; xi = Xs; octave, layer, col, row the last position.  Survivors keep candidate order.
 * Limits: an input of 1 .. LCM_SIFT_MAX_SIDE pixels a side, at most LCM_SIFT_MAX_OCTAVES octaves, every radius at most
 * LCM_SIFT_MAX_RADIUS (the defaults need 13; sigma 1.6 with n_octave_layers 1 needs 45), the smallest octave at least one pixel:
 * LCM_ERR_CAPACITY above the limits, LCM_ERR_INVALID_ARG for a size that gives no octave.  A space holds room for min(every pixel
 * that may be a candidate, LCM_SIFT_MAX_CANDIDATES) candidates; a search that finds more is LCM_ERR_CAPACITY. */
#define LCM_SIFT_MAX_SIDE 4096
#define LCM_SIFT_MAX_OCTAVES 16
#define LCM_SIFT_MAX_RADIUS 48
#define LCM_SIFT_MAX_CANDIDATES 1048576
typedef enum lcm_sift_kind { LCM_SIFT_GAUSSIAN = 0, LCM_SIFT_DOG = 1 } lcm_sift_kind;
typedef struct lcm_sift_params {      /* defaults = cv::SIFT::create's and OpenCV's constants */
    double  contrast_threshold;       /* 0.04 */
    double  edge_threshold;           /* 10 */
    double  sigma;                    /* 1.6 */
    double  init_sigma;               /* 0.5: the blur the input is taken to have (SIFT_INIT_SIGMA) */
    int32_t n_octave_layers;          /* 3; 1 .. 8 */
    int32_t upsample;                 /* 1: the first octave is the image enlarged 2x (firstOctave -1); 0 or 1 */
    int32_t n_octaves;                /* 0: derived from the size; else 1 .. LCM_SIFT_MAX_OCTAVES */
    int32_t border;                   /* 5 (SIFT_IMG_BORDER); >= 1 */
    int32_t max_steps;                /* 5 (SIFT_MAX_INTERP_STEPS); >= 1 */
    int32_t reserved[3];              /* 0 */
} lcm_sift_params;                    /* 64 bytes */
typedef struct lcm_sift_plan_info {
    int32_t  n_octaves, n_gauss, n_dog, base_w, base_h, first_radius, max_radius, reserved;
    int32_t  width[16], height[16];   /* per octave */
    int32_t  radius[12];              /* per Gaussian layer; radius[0] = 0 (layer 0 is not blurred from a layer) */
    double   first_sigma, sig[12];
    uint64_t space_floats;            /* floats of a space of this plan: the base image, then per octave its Gaussian and DoG layers */
} lcm_sift_plan_info;                 /* 320 bytes */
typedef struct lcm_sift_keypoint { float x, y, size, response, xi; int16_t octave, layer; int32_t col, row; } lcm_sift_keypoint;   /* 32 bytes */
typedef struct lcm_sift_candidate { int32_t octave, layer, row, col; } lcm_sift_candidate;                                          /* 16 bytes */
typedef struct lcm_sift_space lcm_sift_space;
typedef struct lcm_sift_space_info_t {
    int32_t  max_w, max_h, w, h;      /* what the space was created for; the last build's image (0, 0: none yet) */
    uint64_t device_bytes;            /* everything the space holds on the device, allocated at creation */
    uint64_t candidate_capacity;
    lcm_sift_plan_info plan;          /* the last build's (zero before the first) */
} lcm_sift_space_info_t;
LCM_API void lcm_sift_params_default(lcm_sift_params* p);
/* Host only, pure, no device needed.  A bad parameter (non-finite or non-positive thresholds and sigmas, n_octave_layers outside
 * 1 .. 8, border < 1, max_steps < 1, n_octaves outside 0 .. 16, upsample not 0 or 1) is LCM_ERR_INVALID_ARG; the limits above.
 * lcm_sift_plan_read: the taps of Gaussian layer `layer` (1 .. n_octave_layers + 2; -1: the first blur), 2 radius + 1 of them;
 * cap too small: LCM_ERR_CAPACITY, *n_taps set, nothing written. */
LCM_API int  lcm_sift_plan(int w, int h, const lcm_sift_params* sp, lcm_sift_plan_info* out);
LCM_API int  lcm_sift_plan_read(int w, int h, const lcm_sift_params* sp, int layer, float* taps, int cap, int* n_taps);
/* A scale space for images of up to max_w x max_h under *sp (NULL: the defaults).  All device memory is allocated here, once:
 * the pyramid of the largest image, the image, the taps, the block counts and the candidates' room.  The parameters and the size
 * are checked on the host before the handle is looked at (then LCM_ERR_NO_DEVICE without a device).  Destroy a space before its handle. */
LCM_API int  lcm_sift_space_create(lcm_handle* h, int max_w, int max_h, const lcm_sift_params* sp, lcm_sift_space** out);
LCM_API void lcm_sift_space_destroy(lcm_sift_space* s);
/* Uploads the gray image (h rows of w bytes, `stride` bytes apart, stride >= w) and builds the pyramid, everything on the handle's
 * stream; finished on return.  A smaller image than the last one reuses the same memory under its own plan. */
LCM_API int  lcm_sift_space_build(lcm_sift_space* s, const uint8_t* img, int w, int h, size_t stride);
LCM_API int  lcm_sift_space_info(const lcm_sift_space* s, lcm_sift_space_info_t* out);
/* One layer of the last build (kind: lcm_sift_kind; octave 0 .. n_octaves - 1; layer 0 .. n_octave_layers + 2, or + 1 for a DoG layer)
 * to or from width[octave] x height[octave] packed floats.  The write form is the door through which tests plant exact DoG values:
 * it changes that layer alone and invalidates nothing else (a DoG layer no longer is the difference of its Gaussians, nor a later
 * Gaussian the blur of a written one) until the next build. */
LCM_API int  lcm_sift_space_read(lcm_sift_space* s, int kind, int octave, int layer, float* out);
LCM_API int  lcm_sift_space_write(lcm_sift_space* s, int kind, int octave, int layer, const float* in);
/* The raw candidates of the built space, in order.  *n = their number; more than cap: LCM_ERR_CAPACITY, nothing written to cand. */
LCM_API int  lcm_sift_extrema(lcm_sift_space* s, lcm_sift_candidate* cand, size_t cap, size_t* n);
/* Extrema, refinement and compaction: only the two counts come back before the records do.  *n = the survivors, *n_candidates
 * (optional) = the candidates; more survivors than cap: LCM_ERR_CAPACITY with both counts set and nothing else written. */
LCM_API int  lcm_sift_detect(lcm_sift_space* s, lcm_sift_keypoint* kp, size_t cap, size_t* n, size_t* n_candidates);
/* Build + detect in one call on a space cached in the handle (made anew when *sp changes or the image outgrows it). */
LCM_API int  lcm_sift_detect_image(lcm_handle* h, const uint8_t* img, int w, int height, size_t stride, const lcm_sift_params* sp,
                                   lcm_sift_keypoint* kp, size_t cap, size_t* n);

/* ---- loop search against the stored database --------------------------------------------------------- */
/* Score `query` (id query_frame_id) against every stored frame with query_frame_id - id >= min_gap, ascending
 * slot order.  out_scores / out_frame_ids need room for lcm_db_size() records. */
LCM_API int  lcm_query_scores(lcm_handle* h, const uint8_t* query, int nq, int query_frame_id,
                              lcm_score* out_scores, int32_t* out_frame_ids, int* n_out);
/* The same query, asynchronously (streaming mode): lcm_query_submit copies `query` into pinned staging, enqueues the
 * upload, the kernel(s) and the download of the records, and returns a ticket without waiting; up to 4 queries may be
 * in flight.  lcm_query_collect waits for that ticket and copies the records out (cap = room in out_scores /
 * out_frame_ids).  Frames appended after the submit are not part of its answer. */
LCM_API int  lcm_query_submit(lcm_handle* h, const uint8_t* query, int nq, int query_frame_id, int* ticket);
LCM_API int  lcm_query_collect(lcm_handle* h, int ticket, lcm_score* out_scores, int32_t* out_frame_ids, int cap, int* n_out);
/* Micro-batched online queries (streaming mode at full device rate): up to 16 frames — e.g. the last few camera frames,
 * none of them appended yet — are scored by ONE launch, each against the stored frames with its_id - id >= min_gap as the
 * database stands at submit time.  (With min_gap >= the id span of the batch this equals submitting them one by one,
 * each before its predecessors are appended.)  One ticket for the batch; lcm_query_collect_batch returns the records of
 * all queries back to back (query 0's first) and, optionally, offsets[n_queries + 1]. */
LCM_API int  lcm_query_submit_batch(lcm_handle* h, const uint8_t* const* queries, const int* nq, const int* query_frame_ids,
                                    int n_queries, int* ticket);
LCM_API int  lcm_query_collect_batch(lcm_handle* h, int ticket, lcm_score* out_scores, size_t cap, size_t* n_out,
                                     size_t* offsets);
LCM_API int  lcm_online_stats_read(lcm_handle* h, lcm_online_stats* out, int reset);
/* detectLoops for a frame that is already stored (or given explicitly with query != NULL). */
LCM_API int  lcm_detect_loops(lcm_handle* h, int current_frame_id, const uint8_t* query, int nq, int n_keypoints,
                              lcm_loop_candidate* out, int cap, int* n_out);
/* Host-side loop test on shipped integers: similarity in IEEE double, strict '>' on the threshold
 * (README.md:123-126).  Returns 1 if the pair is a loop candidate. */
LCM_API int  lcm_loop_test(const lcm_params* p, const lcm_score* s, int n_query_kp, int n_train_kp,
                           double* similarity);

/* ---- bulk all-vs-all (benchmark / re-scan mode) ---------------------------------------------------- */
/* Query set: `n_q_frames` frames at d_query_rows + i*q_stride_rows*32 (device memory), row counts
 * d_query_counts[i] (device, int32), ids q_ids[i] (host, strictly increasing).  If d_query_rows is NULL the
 * handle's own database is the query set.  Every query frame is scored against every stored frame of this
 * handle with q_id - id >= min_gap.  Scores are written to the device buffer d_scores (lcm_score records) in
 * (query ascending, stored slot ascending) order; *n_pairs receives the count; pair_offsets (host, optional,
 * n_q_frames+1 entries) receives the start of each query frame's run.  d_scores may be NULL to size first. */
LCM_API int  lcm_all_vs_all(lcm_handle* h, const void* d_query_rows, const int32_t* d_query_counts,
                            const int32_t* q_ids, int n_q_frames, int q_stride_rows,
                            void* d_scores, size_t scores_cap, size_t* n_pairs, size_t* pair_offsets);
/* Same search through the ARGMIN kernel: besides every query row's best distance it finds the FIRST train row that
 * attains it (BFMatcher's trainIdx) — "per-query min/argmin" of BASELINE.json's north_star — and makes the indices
 * observable without 8 KB of keys per pair: d_index_sums (device, one uint32 per pair, same order as d_scores)
 * receives the sum mod 2^32 of the train indices of the pair's GOOD matches (0 for an empty pair). */
LCM_API int  lcm_all_vs_all_argmin(lcm_handle* h, const void* d_query_rows, const int32_t* d_query_counts,
                                   const int32_t* q_ids, int n_q_frames, int q_stride_rows,
                                   void* d_scores, size_t scores_cap, void* d_index_sums,
                                   size_t* n_pairs, size_t* pair_offsets);
/* Same search with the loop test fused on the device (README.md:123-126; BASELINE.json configs[3]): scores never
 * leave HBM, a second kernel applies similarity > threshold && good >= min_matches per pair in IEEE double and
 * compacts the candidates; `out` (host) receives them sorted by (current_frame_id, matched_frame_id).
 * q_keypoints (host, optional) = keypoint counts of an external query set (NULL: row counts).  *n_out = number
 * found (LCM_ERR_CAPACITY if > cap); *n_pairs_out (optional) = pairs scored. */
LCM_API int  lcm_all_vs_all_loops(lcm_handle* h, const void* d_query_rows, const int32_t* d_query_counts,
                                  const int32_t* q_ids, const int32_t* q_keypoints, int n_q_frames, int q_stride_rows,
                                  lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out);
/* lcm_all_vs_all with the reference's loop-search score (src/main.cpp:1375-1388): per pair, good_count = number of query
 * rows whose best neighbour passes best.distance < ratio * second.distance (knnMatch(k = 2) order, strict, IEEE double;
 * a row without a second neighbour does not count), min_dist = min over query rows of the best distance, n_train as usual.
 * The second neighbour's distance is the second smallest distance counted with multiplicity (two train rows tied at the
 * minimum: second == best); one stored row: good_count = 0; an empty side: good_count = 0, min_dist = 0xFFFF.  Pair set,
 * order, pair_offsets, the sizing call and the external query set are those of lcm_all_vs_all.  lcm_params.ratio,
 * dist_floor, min_matches and sim_threshold are not consulted, nor is the kernel variant: one vector-ALU kernel keeps every
 * query row's two smallest distances and counts on the device (route LCM_ROUTE_PLAIN).  The reference's `rows < 100`
 * skip and its `>= 300` threshold stay with the caller, on the records and the frames' row counts.
 * LCM_ERR_INVALID_ARG while cross_check != 0 and for a NaN or negative ratio, as the k = 2 pair calls; LCM_ERR_CAPACITY
 * for a query frame above 2048 rows (there is no packed route here; a stored frame that is no query frame of the call —
 * no eligible partner — may be taller) and for a too-small scores_cap (nothing written).  Stored frames take part with up
 * to 65535 rows; n_train uses all 16 bits of its field. */
LCM_API int  lcm_all_vs_all_ratio(lcm_handle* h, const void* d_query_rows, const int32_t* d_query_counts,
                                  const int32_t* q_ids, int n_q_frames, int q_stride_rows, double ratio,
                                  void* d_scores, size_t scores_cap, size_t* n_pairs, size_t* pair_offsets);
/* lcm_query_scores with the same score: one host query frame against every stored frame with id gap >= min_gap.
 * Synchronous; ordered after every append issued so far; online tickets in flight are not disturbed.  out_scores /
 * out_frame_ids need room for lcm_db_size() records. */
LCM_API int  lcm_query_scores_ratio(lcm_handle* h, const uint8_t* query, int nq, int query_frame_id, double ratio,
                                    lcm_score* out_scores, int32_t* out_frame_ids, int* n_out);

/* ---- the reference's own loop rule on the ratio-test score (src/main.cpp:1379-1388) ----------------------------------- */
/* A pair (current frame c, stored frame s, id_c - id_s >= min_gap) is a loop candidate iff
 *     rows_c >= min_rows  &&  rows_s >= min_rows          (src/main.cpp:1382: `allDescriptors[..].rows < 100` -> continue)
 *     &&  good_count(c, s, ratio) >= min_matches          (src/main.cpp:1386-1388: matches.size() < 300 -> continue)
 * with good_count exactly what lcm_all_vs_all_ratio writes and rows the DESCRIPTOR row counts (not keypoint counts).
 * Defaults (lcm_ratio_loop_params_default): ratio 0.7, min_rows 100, min_matches 300 — the reference's literals.  The
 * candidate is the usual lcm_loop_candidate: num_matches = good_count, similarity_score = (double)good_count /
 * (double)min(rows_c, rows_s) in IEEE double (0.0 when min_rows = 0 admits an empty side) — informational, not part of the
 * verdict.  lcm_params.ratio / dist_floor / min_matches / sim_threshold, keypoint counts and the kernel variant play no
 * part; min_gap (on ids) plays its usual one — the reference's loopGap = max(3, numViews / 2) is the caller's
 * lcm_set_params.  `poses[i].R.empty()` (src/main.cpp:1377, :1381) stays with the caller: do not append such frames, or
 * drop their candidates.
 * Shared by the calls below: rp == NULL means the defaults; LCM_ERR_INVALID_ARG for a NaN or negative ratio, a negative
 * min_rows or min_matches, and while cross_check != 0 (as the other k = 2 calls); LCM_ERR_CAPACITY for a query frame above
 * 2048 rows (as lcm_all_vs_all_ratio) and for more candidates than `cap` (or out == NULL with candidates present): *n_out
 * is then the count and nothing is written, as lcm_all_vs_all_loops behaves.  Candidates come out in (current id,
 * matched id) ascending order without a host sort. */
typedef struct lcm_ratio_loop_params {
    double  ratio;          /* Lowe's ratio of the score                          src/main.cpp:1386 (0.7) */
    int32_t min_rows;       /* both frames need >= min_rows descriptor rows       src/main.cpp:1382 (100) */
    int32_t min_matches;    /* loop needs good_count >= min_matches               src/main.cpp:1388 (300) */
} lcm_ratio_loop_params;    /* 16 bytes */
LCM_API void lcm_ratio_loop_params_default(lcm_ratio_loop_params* p);
/* Host-only verdict on a shipped record (no device needed): rows_train = s->n_train.  Returns 1 if the pair is a loop
 * candidate; *similarity (optional) as above.  p == NULL: the defaults. */
LCM_API int  lcm_ratio_loop_test(const lcm_ratio_loop_params* p, const lcm_score* s, int rows_query, double* similarity);
/* lcm_all_vs_all_ratio with that verdict fused on the device: pair set, external query set and *n_pairs_out are
 * lcm_all_vs_all_ratio's; the score array stays in device memory (afterwards lcm_last_bulk_scores returns it, byte for byte
 * what lcm_all_vs_all_ratio writes for the same input), verdict and ordered compaction run on the device
 * (k_ratio_loop_count, k_block_scan, k_ratio_loop_emit: aux_kernel_ms of lcm_last_launch_info; route, kernel_ms, pairs and
 * distances as the ratio search reports them) and only the candidates cross PCIe.  Pairs with a frame below min_rows are
 * still scored (the score array does not depend on rp->min_rows). */
LCM_API int  lcm_all_vs_all_loops_ratio(lcm_handle* h, const void* d_query_rows, const int32_t* d_query_counts,
                                        const int32_t* q_ids, int n_q_frames, int q_stride_rows,
                                        const lcm_ratio_loop_params* rp, lcm_loop_candidate* out, size_t cap,
                                        size_t* n_out, size_t* n_pairs_out);
/* The one-frame form (one trip of the loop at src/main.cpp:1375): query != NULL gives the current frame from the host, as
 * lcm_query_scores_ratio takes it; query == NULL means the STORED frame with id current_frame_id (nq is ignored), whose
 * rows are used in place in the arena — LCM_ERR_NOT_FOUND if it is not stored.  Synchronous; outstanding online tickets
 * are not disturbed.  The verdict over the at most lcm_db_size() records runs on the host (lcm_ratio_loop_test). */
LCM_API int  lcm_detect_loops_ratio(lcm_handle* h, int current_frame_id, const uint8_t* query, int nq,
                                    const lcm_ratio_loop_params* rp, lcm_loop_candidate* out, int cap, int* n_out);

LCM_API int  lcm_last_launch_info(const lcm_handle* h, lcm_launch_info* info);
/* Device address and record count of the score array the last lcm_all_vs_all_loops left in HBM (same order as
 * lcm_all_vs_all would write; valid until the next bulk call on this handle; NULL / 0 if there is none). */
LCM_API int  lcm_last_bulk_scores(const lcm_handle* h, const void** d_scores, size_t* n_records);

/* Select the kernel variant of the bulk / online scoring (A/B measurement; results are identical):
 * 0 = query-row-per-lane, best distance per query row; 1 = same + the first train row attaining it (argmin, by
 * 8-row group keys and a re-scan of the winning group); 2 / 3 = the train-row-per-lane mapping with LDS-staged
 * queries and wavefront shuffle reductions, distances only / (dist, idx) keys.
 * 4 = OPT-IN, NOT the product path: BASELINE.json's north_star rules the matrix cores out ("no MFMA"); this variant
 * runs the search on v_mfma_i32_32x32x32_i8 over a +1 / -1 int8 image of
 * the descriptors (<q,t> = 256 - 2 d, exact) to MEASURE what that rule costs; same records bit for bit.  5 = the same
 * on the block-scaled fp4 instruction (v_mfma_scale_f32_32x32x64_f8f6f4, +1/-1 as e2m1, all scales 1.0, exact in the
 * f32 accumulator).  4 / 5 serve the bulk search — lcm_all_vs_all_argmin included: the matrix instruction finds the
 * first 32-row tile that reaches the best dot product, an exact XOR + popcount re-scan of that tile finds the row —
 * and the online queries (single, stored-frame, micro-batched); pair mode and cross_check keep running the
 * vector-ALU kernels under them, as do query frames above 2048 rows. */
LCM_API int  lcm_set_kernel_variant(lcm_handle* h, int variant);

/* ---- multi-GPU: one process, W devices, stored frames sharded cyclically by arrival position ------------------- */
/* What a LoopClosingSystem (include/loop_closing.hpp:29-31) holds instead of one matcher when it is given more than
 * one MI355X: one lcm_handle + one host thread per device, an RCCL communicator (ncclCommInitAll) over them.  Stored
 * frame number p (arrival order) lives on device p mod W.  lcm_group_all_vs_all all-gathers the shard arenas over
 * xGMI so that every device sees every frame as a query, scores on all devices at once, gathers the 8-byte records to
 * the first device (grouped ncclSend / ncclRecv), un-permutes them on that device and returns the SAME array, in
 * the same order, that a single lcm_handle holding all frames would have produced with lcm_all_vs_all. */
typedef struct lcm_group lcm_group;
typedef struct lcm_group_info {
    int32_t  n_devices;
    int32_t  rccl_ranks;                     /* ncclCommCount of the group's communicator; 0 for a loopback rehearsal group */
    uint64_t pairs, distances, algo_bytes;   /* summed over the shards */
    double   kernel_ms_max;                  /* slowest shard's scoring kernel(s) */
    double   gather_merge_ms;                /* first device: its kernel's end -> records gathered (RCCL) and merged */
    double   download_ms;                    /* merged array -> host */
    uint64_t gathered_query_bytes;           /* per device: bytes received by THIS call's all-gather of the shard arenas
                                              * (0 when it was skipped: nothing appended since the last search) */
    uint64_t gathered_score_bytes;           /* bytes of score records (+ index checksums) that crossed xGMI to the first device */
    double   allgather_ms;                   /* first device: duration of the arena all-gather (0 when skipped) */
    double   kernel_ms[8];                   /* per device: its shard's scoring kernel(s) */
    uint64_t shard_pairs[8];                 /* per device: pairs its shard scored */
    int32_t  arena_gather_skipped;           /* 1: the gathered query buffers of the previous search were reused */
    int32_t  loopback;                       /* 1: rehearsal group (all shards on one device, no RCCL) */
} lcm_group_info;
/* device_ids == NULL: devices 0 .. n_devices-1.  n_devices <= 8. */
LCM_API int  lcm_group_create(const lcm_params* params, int n_devices, const int* device_ids, lcm_group** out);
/* The same group with its two exchange steps as device-to-device copies over xGMI (hipMemcpyAsync between the devices'
 * buffers, peer access enabled where available) instead of RCCL calls.  lcm_group_create falls back to this form by
 * itself when the RCCL communicator cannot be created; lcm_group_transport says which one a group uses ("rccl",
 * "peer copies (...)", "loopback (...)").  Results are identical. */
LCM_API int  lcm_group_create_peer(const lcm_params* params, int n_devices, const int* device_ids, lcm_group** out);
LCM_API const char* lcm_group_transport(const lcm_group* g);
/* Rehearsal form for boxes with ONE GPU: n_shards matchers on device_id, the two exchange steps as device-local copies
 * instead of RCCL calls.  Same results as any other group; exists so that the multi-device index arithmetic (cyclic
 * ownership, rank-major query buffer, gatherv offsets, device merge) is exercised for W > 1 where no second GPU is. */
LCM_API int  lcm_group_create_loopback(const lcm_params* params, int n_shards, int device_id, lcm_group** out);
LCM_API void lcm_group_destroy(lcm_group* g);
LCM_API int  lcm_group_size(const lcm_group* g);                    /* W */
LCM_API int  lcm_group_db_size(const lcm_group* g);                 /* frames over all shards */
LCM_API int  lcm_group_handle(lcm_group* g, int rank, lcm_handle** out);   /* the shard's own matcher (borrowed) */
LCM_API int  lcm_group_set_params(lcm_group* g, const lcm_params* params);
LCM_API int  lcm_group_reserve(lcm_group* g, int n_frames, int max_desc);
LCM_API int  lcm_group_append(lcm_group* g, int frame_id, const uint8_t* desc, int n, int n_keypoints);
LCM_API int  lcm_group_clear(lcm_group* g);
/* Keep the first n_frames frames (arrival order), drop the rest; tickets in flight become void (lcm_db_truncate per shard). */
LCM_API int  lcm_group_truncate(lcm_group* g, int n_frames);
/* Snapshot / resume in lcm_db_save's own file format, frames in arrival order: a file written by a group of 8 loads
 * into a single handle or a group of any size, and the other way round.  Load replaces the group's contents (same
 * validation as lcm_db_load: header checked against the file before anything is touched; empty group on a later error). */
LCM_API int  lcm_group_save(lcm_group* g, const char* path);
LCM_API int  lcm_group_load(lcm_group* g, const char* path);
LCM_API int  lcm_group_sync(lcm_group* g);                                   /* lcm_sync on every shard */
LCM_API int  lcm_group_set_tuning(lcm_group* g, int knob, int value);        /* lcm_set_tuning on every shard */
LCM_API int  lcm_group_set_kernel_variant(lcm_group* g, int variant);        /* lcm_set_kernel_variant on every shard */
/* out_scores (host) receives *n_pairs records in (query ascending, stored ascending) order; pair_offsets (host,
 * optional, db_size + 1 entries); out_scores == NULL sizes only.  The all-gather of the shard arenas is skipped when
 * nothing was appended since the previous search (lcm_group_info.arena_gather_skipped). */
LCM_API int  lcm_group_all_vs_all(lcm_group* g, lcm_score* out_scores, size_t cap, size_t* n_pairs, size_t* pair_offsets);
/* lcm_all_vs_all_argmin over the group: the same search through the ARGMIN kernel; out_index_sums (host, one uint32 per
 * pair, same order) receives the per-pair index checksums, gathered and merged like the records.  A group of ONE device
 * returns byte for byte what lcm_all_vs_all_argmin writes on a single handle. */
LCM_API int  lcm_group_all_vs_all_argmin(lcm_group* g, lcm_score* out_scores, uint32_t* out_index_sums, size_t cap,
                                         size_t* n_pairs, size_t* pair_offsets);
/* lcm_all_vs_all_loops over the group (BASELINE.json configs[3] on several devices): every device scores its shard and
 * applies the loop test to its own records ON THE DEVICE; only the candidates leave the devices — each shard's over its
 * own PCIe link, all links at once — and are merged on the host into (current id, matched id) order.  *n_out = number
 * found (LCM_ERR_CAPACITY if > cap, nothing written); *n_pairs_out (optional) = pairs scored. */
LCM_API int  lcm_group_all_vs_all_loops(lcm_group* g, lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out);
/* lcm_all_vs_all_ratio over the group, under lcm_group_all_vs_all's contract: the same records in the same order as a
 * single handle holding all frames (a group of ONE: byte for byte), arena all-gather skipped when nothing was appended,
 * lcm_group_info filled as usual; on RCCL, peer-copy and loopback groups alike.  LCM_ERR_INVALID_ARG for a NaN or negative
 * ratio and while cross_check != 0. */
LCM_API int  lcm_group_all_vs_all_ratio(lcm_group* g, double ratio, lcm_score* out_scores, size_t cap, size_t* n_pairs,
                                        size_t* pair_offsets);
/* lcm_all_vs_all_loops_ratio over the group, under lcm_group_all_vs_all_loops' contract: every shard applies the verdict
 * to its own records on its own device, only candidates leave the devices, W-way merged on the host. */
LCM_API int  lcm_group_all_vs_all_loops_ratio(lcm_group* g, const lcm_ratio_loop_params* rp, lcm_loop_candidate* out,
                                              size_t cap, size_t* n_out, size_t* n_pairs_out);
LCM_API int  lcm_group_last_info(const lcm_group* g, lcm_group_info* info);
/* lcm_query_scores / lcm_detect_loops over all shards (query uploaded to every device; per-shard records interleaved
 * on the host: a few KB per query). */
LCM_API int  lcm_group_query_scores(lcm_group* g, const uint8_t* query, int nq, int query_frame_id,
                                    lcm_score* out_scores, int32_t* out_frame_ids, int cap, int* n_out);
/* lcm_query_submit_batch + lcm_query_collect_batch over all shards: up to 16 frames per launch per device (the
 * streaming mode of BASELINE.json configs[4] inside one process); records of query 0 first, offsets[n_queries + 1]. */
LCM_API int  lcm_group_query_scores_batch(lcm_group* g, const uint8_t* const* queries, const int* nq,
                                          const int* query_frame_ids, int n_queries,
                                          lcm_score* out_scores, size_t cap, size_t* n_out, size_t* offsets);
/* The asynchronous form (what keeps W devices busy in streaming mode): submit returns once every device has the batch
 * ENQUEUED — each from its own host thread; the callers' buffers are free then — with one group ticket; up to 4 may be in
 * flight (submit batch k + 1, append, then collect batch k).  Collect waits for that ticket; every device's thread writes
 * its records straight into their places of the single-device order.  A too-small `cap` keeps the ticket valid; a
 * lcm_group_clear / _truncate in between voids it (LCM_ERR_NOT_FOUND). */
LCM_API int  lcm_group_query_submit_batch(lcm_group* g, const uint8_t* const* queries, const int* nq,
                                          const int* query_frame_ids, int n_queries, int* ticket);
LCM_API int  lcm_group_query_collect_batch(lcm_group* g, int ticket, lcm_score* out_scores, size_t cap, size_t* n_out,
                                           size_t* offsets);
/* lcm_online_stats_read over the shards: work summed, kernel_ms = the slowest shard's (the devices run side by side). */
LCM_API int  lcm_group_online_stats_read(lcm_group* g, lcm_online_stats* out, int reset);
LCM_API int  lcm_group_detect_loops(lcm_group* g, int current_frame_id, const uint8_t* query, int nq, int n_keypoints,
                                    lcm_loop_candidate* out, int cap, int* n_out);
/* Host-only (no device needed): merge W per-shard score arrays — shard r in (query ascending, owned stored ascending)
 * order, as a process-per-GPU deployment gathers them (bench.py, torch.distributed) — into the single-device order.
 * ids: all n_frames frame ids, ascending.  out == NULL sizes only (*n_out, offsets[n_frames + 1] optional). */
LCM_API int  lcm_merge_shard_scores(const lcm_score* const* shard_scores, const size_t* shard_counts, int world,
                                    const int32_t* ids, int n_frames, int min_gap,
                                    lcm_score* out, size_t cap, size_t* n_out, size_t* offsets);

/* The same merge on the device (what lcm_group_all_vs_all runs on its first device): d_gathered holds the W shard
 * arrays back to back; d_merged receives the single-device order.  world <= 8. */
LCM_API int  lcm_merge_shard_scores_device(lcm_handle* h, const void* d_gathered, const size_t* shard_counts, int world,
                                           const int32_t* ids, int n_frames, int min_gap,
                                           void* d_merged, size_t cap, size_t* n_out);

/* Measurement knobs (defaults are the measured optima; results never depend on them):
 *   LCM_TUNE_ITEM_SLOTS   stored frames per work item of the bulk search, 1..64; 0 = automatic
 *   LCM_TUNE_ONLINE_SPLIT query rows per lane of the online split mode: 1, 2, 4 (256-thread workgroups), 16 / 32 (64- /
 *                         128-thread workgroups of 8 rows per lane); 0 = never split; -1 = automatic
 *   LCM_TUNE_PACKED       bulk search with the query rows of consecutive frames packed into full 2048-row workgroups:
 *                         1 = always, 0 = never, -1 = automatic (when packing saves lane slots), 2 = always, with
 *                         1536-row workgroups (6 rows per lane at 8 waves per SIMD: an A/B, within 0.5 % of 1)
 *   LCM_TUNE_ONLINE_STREAMS 1 (default) = each of the 4 query slots enqueues on its own stream, so consecutive online
 *                         queries overlap (upload and first workgroups of one under the draining tail of the other);
 *                         0 = everything on the handle's stream
 *   LCM_TUNE_PACKED_SCRATCH_MB  packed route: MiB of per-row scratch per chunk (default 1024; a search larger than one
 *                         chunk runs chunk after chunk; halved for the search at hand, down to 64, when the allocation
 *                         fails — the next plan starts from the configured size again).  Device footprint of a handle
 *                         beyond its database: this scratch (allocated at the first packed search, given back when a
 *                         later search needs less than a quarter of it), 8 bytes per pair of the fused loop search's
 *                         score array, and the staging of up to 4 online queries.
 *   LCM_TUNE_PAIR_UPLOAD_KERNEL  pair mode, calls of <= 64 M distances: the staging block is uploaded by a kernel on the
 *                         compute queue (1, default) or by hipMemcpyAsync (0)
 *   LCM_TUNE_PAIR_HOST_FOLD      ... and the fold kernel writes the folded keys straight into pinned host memory (1,
 *                         default) or into device memory followed by a copy (0) */
typedef enum lcm_tuning { LCM_TUNE_ITEM_SLOTS = 0, LCM_TUNE_ONLINE_SPLIT = 1, LCM_TUNE_PACKED = 2, LCM_TUNE_ONLINE_STREAMS = 3,
                          LCM_TUNE_PACKED_SCRATCH_MB = 4, LCM_TUNE_PAIR_UPLOAD_KERNEL = 5, LCM_TUNE_PAIR_HOST_FOLD = 6 } lcm_tuning;
LCM_API int  lcm_set_tuning(lcm_handle* h, int knob, int value);

/* Device scratch helpers so a host program needs no other allocator (plain hipMalloc/hipFree/hipMemcpy). */
LCM_API int  lcm_dev_alloc(lcm_handle* h, size_t bytes, void** d_ptr);
LCM_API int  lcm_dev_free(lcm_handle* h, void* d_ptr);
LCM_API int  lcm_dev_upload(lcm_handle* h, void* d_dst, const void* src, size_t bytes);
LCM_API int  lcm_dev_download(lcm_handle* h, void* dst, const void* d_src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* LCM_H_ */
