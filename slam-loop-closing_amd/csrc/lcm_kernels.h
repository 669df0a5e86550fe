// lcm_kernels.h — launch interface between the C-ABI host code (lcm_api.cpp) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace lcm {

constexpr int KEY_SHIFT = 22;                       // packed key = dist << 22 | train_idx  (dist <= 256 -> 9 bits)
constexpr uint32_t KEY_IDX_MASK = (1u << KEY_SHIFT) - 1;
constexpr int MAX_FUSED_QUERY_ROWS = 2048;          // one workgroup holds a whole query frame in registers
constexpr int MAX_QUERY_BATCH = 16;                 // online queries scored by one launch (lcm_query_submit_batch)

// One unit of work: query frame `q_frame` against stored slots [slot_begin, slot_begin + n_slots),
// score records written to scores[out_offset ...].
struct WorkItem {
    uint32_t q_frame;
    uint32_t slot_begin;
    uint32_t n_slots;
    uint32_t out_offset;
};

// Pair mode (matchFeatures / match lists): one unit = <= 2048 query rows starting at row q_row of q_rows against nt
// train rows starting at row t_row of db_rows (a SEGMENT of a train matrix: several items share one pair so that a
// single 2000 x 2000 match spreads over ~64 workgroups).  t_row and every segment length but a matrix's last are
// multiples of 4; the last segment ends where the matrix's padding rows (copies of its last row) begin.
struct PairItem {
    uint32_t q_row;
    uint32_t t_row;
    uint32_t nq_nt;              // nq (12 bits, <= 2048 -> stored as nq) | nt << 12 (20 bits)
    uint32_t out_offset;         // keys[out_offset * keys_stride + local query row]
};

struct ScoreArgs {
    const uint32_t* q_rows;      // query frames: frame f at q_rows + f * q_stride_words, rows of 8 dwords
    const int32_t*  q_counts;    // rows per query frame
    uint32_t        q_stride_words;
    const uint32_t* db_rows;     // stored frames, same layout
    const int32_t*  db_counts;
    uint32_t        db_stride_words;
    const WorkItem* items;       // NULL => implicit items (online queries: nothing to upload), see imp_* below
    const PairItem* pair_items;  // non-NULL => pair mode: overrides items / implicit items; keys must be non-NULL
    void*           scores;      // lcm_score records (8 bytes each)
    uint32_t*       keys;        // optional: best packed key per query row, keys[pair * keys_stride + row]
    uint32_t        keys_stride;
    uint32_t*       idx_sums;    // optional (ARGMIN kernels): per pair, sum of the train indices of its GOOD matches mod 2^32
    int32_t         ratio;
    int32_t         dist_floor;
    // Implicit items (items == NULL): ONE query frame of imp_nq rows at q_rows, cut into imp_chunks chunks of
    // imp_chunk_rows rows (1 chunk = whole frame), against stored slots [0, imp_total) in runs of imp_spi slots.
    // Workgroup b: chunk c = b % imp_chunks, run g = b / imp_chunks, out_offset = g * imp_spi * imp_chunks + c.
    uint32_t        imp_chunks, imp_chunk_rows, imp_spi, imp_total;
    int32_t         imp_nq;
    // Implicit BATCH (items == NULL, imp_nbatch > 0): imp_nbatch query frames (micro-batched online queries), query b
    // of bat_nq[b] rows stored at chunk index b * imp_chunks of q_rows, scored against stored slots [0, bat_elig[b]);
    // its workgroups are [bat_wg[b], bat_wg[b + 1]) and its records start at pair index bat_pair[b].  imp_chunks,
    // imp_chunk_rows and imp_spi are shared by the whole batch.
    // PACKED bulk mode (launch_score_packed): the query rows of a GROUP of query frames form one virtual row space cut
    // into 2048-row workgroups, so a 2000-row frame no longer leaves 48 of 2048 lane slots idle.  A launch (chunk) covers
    // one group against one RANGE of stored slots [pk_slot0, ...): the scratch holds only that range's pairs, so its
    // size does not limit how many frames share the row space.  Work item: q_frame = workgroup index w in that space
    // (virtual rows [2048 w, 2048 w + 2048)), slots as usual (inside the chunk's range).  Per query frame k of the group
    // (pk_n of them): pk_vstart[k] = its first virtual row (pk_vstart[pk_n] = total), pk_qframe[k] = its index in
    // q_rows, pk_elig[k] = its eligible stored slots (global), pk_pairs[k] = its first pair in this chunk's pk_dist
    // (pk_pairs[pk_n] = the chunk's pair count).  Output: the best distance (as a uint16; ARGMIN: the packed key, a
    // uint32) of every (pair, query row) -> word (pk_pairs[k] + slot - pk_slot0) * pk_stride + row of pk_dist;
    // launch_finalize_bulk folds them.
    // Query frames may exceed 2048 rows here (they span columns); every other route stops at MAX_FUSED_QUERY_ROWS.
    const uint32_t* pk_vstart;
    const uint32_t* pk_qframe;
    const uint32_t* pk_elig;
    const uint32_t* pk_pairs;
    uint32_t*       pk_dist;
    uint32_t        pk_n;
    uint32_t        pk_col_rows;  // rows per column (workgroup): 2048 (8 rows per lane) or 1536 (6 rows per lane)
    uint32_t        pk_stride;    // words of pk_dist per pair: 2048, or the largest query frame rounded up when above that
    uint32_t        pk_slot0;     // first stored slot of the chunk's range
    uint32_t        imp_nbatch;
    uint32_t        bat_wg[MAX_QUERY_BATCH + 1];
    uint32_t        bat_pair[MAX_QUERY_BATCH + 1];
    int32_t         bat_nq[MAX_QUERY_BATCH];
    uint32_t        bat_elig[MAX_QUERY_BATCH];
};

// Launch the pair-scoring kernel over n_items work items.  max_query_rows = largest row count of any query
// frame referenced (<= MAX_FUSED_QUERY_ROWS).  variant: 0 = row-per-lane/scalar-broadcast (default).
hipError_t launch_score(const ScoreArgs& a, uint32_t n_items, int max_query_rows, bool write_keys, int variant,
                        hipStream_t st);
// PACKED bulk mode (see ScoreArgs::pk_*): 256-thread workgroups of 8 rows per lane; argmin = group keys + re-scan.
hipError_t launch_score_packed(const ScoreArgs& a, uint32_t n_items, bool argmin, hipStream_t st);

// Split mode (short databases): chunks of 256 * qpt query rows per workgroup write per-row best distances into
// a.keys; launch_finalize folds each pair's rows into its lcm_score record.
hipError_t launch_score_split(const ScoreArgs& a, uint32_t n_items, int qpt, hipStream_t st);
struct FinalizeArgs {
    const uint32_t* dist;        // best distance per (pair, row): dist[pair * padded_rows + row]
    uint32_t        padded_rows;
    int32_t         nq;          // real query rows (single query)
    const int32_t*  db_counts;   // stored row counts; pair p is slot slot_begin + p
    uint32_t        slot_begin;
    void*           scores;      // lcm_score per pair
    int32_t         ratio, dist_floor;
    // batch (n_batch > 0): pair p belongs to the query b with bat_pair[b] <= p < bat_pair[b + 1], has bat_nq[b] query
    // rows and is stored slot p - bat_pair[b]
    uint32_t        n_batch;
    uint32_t        bat_pair[MAX_QUERY_BATCH + 1];
    int32_t         bat_nq[MAX_QUERY_BATCH];
};
hipError_t launch_finalize(const FinalizeArgs& a, uint32_t n_pairs, hipStream_t st);

// Pair mode, second step: fold the per-segment keys of every pair (segment-local train indices) into one key per query
// row with GLOBAL train indices: final[out_row0 + r] = min over segments g of (seg_keys[item(c, g)][r mod 2048] + g *
// seg_rows), c = r / 2048.  min over (dist, global index) keys keeps the FIRST minimum across segments.
struct PairDesc {
    uint32_t first_item;         // item (c, g) of this pair is first_item + c * n_seg + g
    uint32_t n_seg;
    uint32_t seg_rows;
    uint32_t nq;
    uint32_t out_row0;           // first row of this pair in the folded key array
};
struct FoldArgs {
    const uint32_t* seg_keys;    // per item: chunk_rows keys
    uint32_t        chunk_rows;  // query rows per item: 2048 (throughput shape) or 512 (latency shape); 0 means 2048
    const PairDesc* pairs;
    uint32_t*       final_keys;
    uint32_t        n_pairs;
    uint32_t        pair_base;   // set by the launchers: pair of blockIdx.y == 0 (a call's pairs go out in slices, below)
};
// gridDim.y carries the pairs of a fold launch.  Its limit is the current device's hipDeviceProp_t::maxGridSize[1] (read
// once per device and kept): the fold launchers cut a call's pairs into slices of at most that many, one launch each, so
// that the number of pairs in a call is bounded by its buffers alone.
hipError_t grid_y_limit(uint32_t* limit);
// The launch of every kernel whose grid's y is the pair or the job: n of them in slices of at most that limit, one launch each,
// grid (grid_x, the slice's length), with args.*base = the pair or job of blockIdx.y == 0.  n == 0 launches and asks nothing.
template <typename Kernel, typename Args>
hipError_t launch_y_sliced(Kernel kernel, const Args& args, uint32_t Args::*base, uint32_t n, uint32_t grid_x, uint32_t block, hipStream_t st) {
    if (n == 0) return hipSuccess;
    uint32_t lim = 0;
    hipError_t e = grid_y_limit(&lim);
    if (e != hipSuccess) return e;
    Args s = args;
    for (s.*base = 0; s.*base < n; s.*base += lim) {
        hipLaunchKernelGGL(kernel, dim3(grid_x, std::min(lim, n - s.*base)), dim3(block), 0, st, s);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (n - s.*base <= lim) break;                             // base + lim may not fit 32 bits
    }
    return hipSuccess;
}
hipError_t launch_fold_pair_keys(const FoldArgs& a, uint32_t max_nq, hipStream_t st);
// bytes (rounded up to 16; both buffers must have that room, 16-byte aligned) from PINNED host memory to device memory, by
// a kernel on `st` instead of a DMA-engine copy (latency-critical small uploads)
hipError_t launch_upload(void* d_dst, const void* h_src_pinned, size_t bytes, hipStream_t st);
// Pair mode, first step, LATENCY shape: items of <= 512 query rows on 256-thread workgroups of 2 rows per lane.  One
// matchFeatures call is a few hundred thousand distances per wave whatever the shape, and a wave alone on its SIMD issues
// one VALU instruction per ~8 cycles: what shortens the call is MORE waves with less work each, not fewer instructions
// (2000 x 2000: 252 workgroups x 4 waves x 64 distances per lane instead of 63 x 4 x 256).
hipError_t launch_score_pairs_small(const ScoreArgs& a, uint32_t n_items, hipStream_t st);

// ---- pair mode, k = 2 (lcm_knn.hip): knnMatch(k = 2) of src/main.cpp:509-534 ------------------------------------------
// The same PairItem work items; per (item, query row) the TWO smallest packed keys (segment-local train indices) go to
// keys[(out_offset * keys_stride + row) * 2 + {0, 1}], 0xFFFFFFFF = no such neighbour (a segment of one row has no
// second).  The padding rows past an item's nt rows never become neighbours.  keys must be 8-byte aligned.
struct Knn2Args {
    const uint32_t* q_rows;      // query rows: item's rows start at row q_row (rows of 8 dwords)
    const uint32_t* t_rows;      // train rows, same layout
    const PairItem* items;
    uint32_t*       keys;
    uint32_t        keys_stride; // query rows per item: 2048 (throughput shape) or 512 (latency shape)
};
// Throughput shape: items of <= 2048 query rows, 8 rows per lane (workgroup size by max_query_rows, as launch_score).
hipError_t launch_knn2_pairs(const Knn2Args& a, uint32_t n_items, int max_query_rows, hipStream_t st);
// Latency shape: items of <= 512 query rows on 256-thread workgroups of 2 rows per lane (see launch_score_pairs_small).
hipError_t launch_knn2_pairs_small(const Knn2Args& a, uint32_t n_items, hipStream_t st);
// The twin of launch_fold_pair_keys: merges the per-segment top-2 lists into every query row's two smallest keys with
// GLOBAL train indices, final_keys[(out_row0 + r) * 2 + {0, 1}] (seg_keys: chunk_rows key PAIRS per item).
hipError_t launch_fold_pair_keys2(const FoldArgs& a, uint32_t max_nq, hipStream_t st);

// ---- pair mode on SIFT rows (lcm_l2.hip): BFMatcher(NORM_L2).knnMatch(k = 2) over 128-byte rows, src/main.cpp:497-534 ----
// Matrices live back to back in a TILE space: a matrix starts at a multiple of 32 rows, tile T covers raw rows
// [32 T, 32 T + 32) of `raw`, its operand image is img + T * 4096 and its per-row words are tw + 32 T.
constexpr int L2_ROW_BYTES = 128;
constexpr int L2_TILE_ROWS = 32;
constexpr int L2_TILE_BYTES = 4096;
constexpr int L2_SEG_ROWS = 512;                    // train rows per item: the key's index field
constexpr int L2_KEY_SHIFT = 9;                     // packed key = D << 9 | segment-local train index (D < 2^23)
constexpr uint32_t L2_RESCAN_MIN = 1u << 22;        // sqrtf is injective on integers below this
struct L2PackArgs {
    const uint8_t*  raw;         // uint8 rows as uploaded
    const uint32_t* tile_meta;   // per tile: rows of the tile that exist (1..32) | index of the tile inside its matrix << 8
    uint8_t*        img;         // int8 (byte ^ 0x80) in the MFMA's operand order, pad rows zero
    uint32_t*       tw;          // per row: sum of the squared int8 << 9 | row index inside its 512-row segment
    uint32_t        n_tiles;
};
hipError_t launch_l2_pack(const L2PackArgs& a, hipStream_t st);
// One workgroup = one item: q_rows <= chunk_rows query rows starting at tile q_tile against t_rows <= 512 train rows starting
// at tile t_tile.  Per (item, query row) the two smallest keys -> seg_keys[item * chunk_rows + row], 0xFFFFFFFF = none.
struct L2Item { uint32_t q_tile, q_rows, t_tile, t_rows; };
struct L2ScoreArgs {
    const uint8_t*  img;
    const uint32_t* tw;
    const L2Item*   items;
    uint2*          seg_keys;
    uint32_t        chunk_rows;  // 128 (one query tile per wave) or 256 (two)
};
hipError_t launch_l2_score(const L2ScoreArgs& a, uint32_t n_items, hipStream_t st);
// One job = one (query matrix, train matrix) pair: its items are first_item + chunk * n_seg + segment.  The fold writes
// (D1, idx1, D2, idx2) per query row (0xFFFFFFFF = none) to final_keys[out_row0 + row] and appends the rows whose D2 is
// >= L2_RESCAN_MIN to `flagged` (job, row), counted in *counter (zeroed by the caller); the rescan redoes those rows in
// (sqrtf(D), index) order over the raw bytes.  `reserved` is read by lcm_l2_emit.hip only: the job's first 256-row block.
struct L2Job { uint32_t q_tile, nq, t_tile, nt, first_item, n_seg, out_row0, reserved; };
struct L2FoldArgs {
    const uint2*    seg_keys;
    uint32_t        chunk_rows;
    const L2Job*    jobs;
    uint4*          final_keys;
    uint32_t*       counter;
    uint2*          flagged;
    uint32_t        flag_cap;
    const uint8_t*  raw;
    uint32_t        job_base;    // set by launch_l2_fold: job of blockIdx.y == 0 (slices of grid_y_limit() jobs); `flagged` holds
                                 // the job's index in `jobs`, whatever the slice
};
hipError_t launch_l2_fold(const L2FoldArgs& a, uint32_t n_jobs, uint32_t max_nq, hipStream_t st);
hipError_t launch_l2_rescan(const L2FoldArgs& a, hipStream_t st);

// ---- ratio-test counts per pair on SIFT rows (lcm_l2_count.hip): the loop search's score, src/main.cpp:1375-1388 --------
// One workgroup = one item: q_rows <= chunk_rows query rows starting at tile q_tile against the WHOLE train matrix of
// pair `pair` (t_rows rows starting at tile t_tile).  Per pair one 8-byte record (include/lcm.h, lcm_l2_score): the kernel
// adds each wave's survivors to good_count and takes the minimum of its rows' D1 into min_dist_sq.
constexpr uint32_t L2_MAX_DSQ = 128u * 255u * 255u;    // 8 323 200
struct L2CountItem { uint32_t q_tile, q_rows, t_tile, t_rows, pair, reserved[3]; };
struct L2CountArgs {
    const uint8_t*     img;
    const uint32_t*    tw;
    const L2CountItem* items;
    uint2*             scores;      // (good_count, min_dist_sq) per pair, initialised by launch_l2_count_init
    double             ratio;
    uint32_t           chunk_rows;  // 128 (one query tile per wave) or 256 (two)
};
hipError_t launch_l2_count_init(uint2* scores, uint32_t n_pairs, hipStream_t st);      // every record <- (0, 0xFFFFFFFF)
hipError_t launch_l2_count(const L2CountArgs& a, uint32_t n_items, hipStream_t st);
// pass[i] = the count kernel's verdict on (d1[i], d2[i]), both <= L2_MAX_DSQ: one thread each, grid-stride
hipError_t launch_l2_ratio_test(const uint32_t* d1, const uint32_t* d2, size_t n, double ratio, uint8_t* pass, hipStream_t st);

// ---- the same counts over the SIFT keyframe store (lcm_l2_store.hip): no per-item table ------------------------------------
// The store keeps every appended matrix in the tile space above and a device FRAME TABLE {first tile, rows} per slot.  A
// search is a list of RUNS: one query matrix (a stored slot, or host rows staged in the arena's free tail) against the
// first n_past entries of `past`, ONE ascending list of admitted stored slots that all runs share.  Run u owns workgroups
// [first_wg, first_wg + n_past * chunks): local workgroup l scores chunk l % chunks of the query against slot
// past[l / chunks] (the chunks of a pair are adjacent: they share the train tiles in L2) into scores[first_pair + l / chunks].
// The workgroup finds its run by a binary search over first_wg (strictly ascending: every run has at least one workgroup).
struct L2StoreRun { uint32_t q_tile, q_rows, chunks, first_wg, first_pair, n_past; };      // 24 bytes
struct L2StoreArgs {
    const uint8_t*    img;
    const uint32_t*   tw;
    const L2StoreRun* runs;
    const uint32_t*   past;        // admitted stored slots with at least one row, ascending
    const uint2*      frames;      // the store's frame table: (first tile, rows) per slot
    uint2*            scores;      // (good_count, min_dist_sq) per pair, initialised by launch_l2_count_init
    double            ratio;
    uint32_t          n_runs;
    uint32_t          chunk_rows;  // 128 (one query tile per wave) or 256 (two)
};
hipError_t launch_l2_count_store(const L2StoreArgs& a, uint32_t n_workgroups, hipStream_t st);

// ---- the ratio test, an ordered compaction and the keypoint gather over final_keys (lcm_l2_emit.hip) ----------------------
// src/main.cpp:524-531 and :551-555 (extractMatchedPoints) for every job of a call, AFTER launch_l2_rescan (which rewrites
// rows of final_keys).  A job's query rows are cut into BLOCKS of 256; job j's blocks are blocks[jobs[j].reserved + b], job
// after job.  launch_l2_emit_count leaves the survivors of every block in `blocks`; launch_block_scan over n_blocks words
// with total = blocks + n_blocks turns them into exclusive prefixes; launch_l2_emit_offsets writes the call's per-pair
// offsets; launch_l2_emit writes survivor k of block B to out[blocks[B] + k], k = its rank in query order.
// A record is {query row, idx1, 0, sqrtf(D1)} (lcm_dmatch); with `pts` a second 16-byte record holds the two keypoints,
// pts[q_tile * 32 + query row] and pts[t_tile * 32 + idx1] (8 bytes per row in the store's tile space).
struct L2EmitArgs {
    const uint4*    final_keys;
    const L2Job*    jobs;
    uint32_t*       blocks;      // n_blocks + 1 words
    const uint2*    pts;         // NULL: no point pairs
    uint4*          out;
    uint4*          out_pts;
    double          ratio;
    uint32_t        n_out;       // records `out` (and `out_pts`) hold: the scan's total
    uint32_t        job_base;    // set by the launchers: job of blockIdx.y == 0 (slices of grid_y_limit() jobs)
};
hipError_t launch_l2_emit_count(const L2EmitArgs& a, uint32_t n_jobs, uint32_t max_nq, hipStream_t st);
hipError_t launch_l2_emit(const L2EmitArgs& a, uint32_t n_jobs, uint32_t max_nq, hipStream_t st);
// offsets[p] = blocks[pair_block[p]] for p < n: pair_block[p] = first block of the first live job at or after pair p,
// n_blocks (the total) past the last one
hipError_t launch_l2_emit_offsets(const uint32_t* blocks, const uint32_t* pair_block, uint64_t* offsets, uint32_t n, hipStream_t st);

// ---- essential-matrix RANSAC over the pairs' point lists (lcm_epi.hip): src/main.cpp:1395-1403 -------------------------
// Pair p of the call owns the records pts[offsets[p] .. offsets[p + 1]) = {qx, qy, tx, ty} as float bits (k_l2_emit's point
// records, or a caller's lcm_point_pair array) and `iters` hypotheses: samples[(p * iters + it) * 8 ..], E[(p * iters + it) *
// 9 ..].  best[p] = max over the hypotheses of (inliers << 16 | 0xFFFF - it), zeroed before launch_epi_score.  The sampler
// is seeded with pair_seed0 + p.  counts (optional): every hypothesis's inlier count.  results / mask: k_epi_mask's output,
// one lcm_epi_result per pair and one byte per record.
struct EpiArgs {
    const uint4*    pts;
    const uint64_t* offsets;     // n_pairs + 1
    int32_t*        samples;
    double*         E;
    uint32_t*       best;
    uint32_t*       counts;      // NULL: not wanted
    void*           results;     // EpiResult (lcm_epi_device.h) per pair
    uint8_t*        mask;
    double          fx, fy, cx, cy, t2;
    uint32_t        iters;       // multiple of 64
    uint32_t        seed;
    uint32_t        pair_seed0;
    uint32_t        pair_base;   // set by the launchers: pair of blockIdx.y == 0 (slices of grid_y_limit() pairs)
};
hipError_t launch_epi_solve(const EpiArgs& a, uint32_t n_pairs, hipStream_t st);
hipError_t launch_epi_score(const EpiArgs& a, uint32_t n_pairs, hipStream_t st);
hipError_t launch_epi_mask(const EpiArgs& a, uint32_t n_pairs, uint32_t max_n, hipStream_t st);

// ---- relative pose of the verified pairs (lcm_pose.hip): src/main.cpp:1405-1409 ------------------------------------------
// Pair p owns the records pts[offsets[p] .. offsets[p + 1]) as above and the matrix E[p * e_stride ..] (9 doubles, row-major:
// e_stride = 9 for a packed array, 11 for the EpiResult records k_epi_mask writes).  mask_in (NULL: every record): the
// records whose byte is non-zero take part.  results: one PoseResult (lcm_pose_device.h) per pair; mask_out: one byte per
// record.  cand_R / cand_t (NULL: not wanted): the four candidates of every pair, 36 and 12 doubles.
struct PoseArgs {
    const uint4*    pts;
    const uint64_t* offsets;     // n_pairs + 1
    const double*   E;
    uint32_t        e_stride;    // doubles between two pairs' matrices
    const uint8_t*  mask_in;
    void*           results;
    uint8_t*        mask_out;
    double*         cand_R;
    double*         cand_t;
    double          fx, fy, cx, cy, max_depth;
    uint32_t        pair_base;   // set by the launcher: pair of blockIdx.y == 0 (slices of grid_y_limit() pairs)
};
hipError_t launch_pose_recover(const PoseArgs& a, uint32_t n_pairs, hipStream_t st);

// ---- local optimisation of the RANSAC's best hypotheses (lcm_lo.hip): refits on the inliers, between the two above ---------
// Pair p owns its records as above, the RANSAC's hypotheses E[(p * iters + it) * 9 ..] and their counts[p * iters + it].
// k_lo_select writes seeds[p * 64 + lane] = the hypothesis of the lane-th largest key; k_lo_refine reads them and overwrites
// results[p] and the pair's mask bytes (k_epi_mask's) only where a refit holds strictly more inliers, and writes info[p].
// The refit seam (refit_E != NULL, one pair): E holds n_models <= 64 models instead, model m = lane m runs ONE round under
// mult[0] and writes refit_E[9 m ..], refit_n[m] (records selected) and refit_status[m]; nothing else is written.
struct LoArgs {
    const uint4*    pts;
    const uint64_t* offsets;     // n_pairs + 1
    const double*   E;
    const uint32_t* counts;
    int32_t*        seeds;
    void*           results;     // EpiResult (lcm_epi_device.h) per pair
    uint8_t*        mask;
    void*           info;        // LoInfo (lcm_lo_device.h) per pair
    double*         refit_E;
    int32_t*        refit_n;
    int32_t*        refit_status;
    double          fx, fy, cx, cy, t;       // t = threshold / ((fx + fy) / 2)
    double          mult[8];
    uint32_t        iters;       // multiple of 64
    uint32_t        rounds;      // 1 .. 8
    uint32_t        n_models;    // the seam's
    uint32_t        pair_base;   // set by the launchers: pair of blockIdx.y == 0 (slices of grid_y_limit() pairs)
};
hipError_t launch_lo_select(const LoArgs& a, uint32_t n_pairs, hipStream_t st);
hipError_t launch_lo_refine(const LoArgs& a, uint32_t n_pairs, hipStream_t st);

// ---- bulk / online loop search scored with Lowe's ratio test (lcm_ratio.hip): src/main.cpp:1375-1388 -------------------
// One workgroup = one WorkItem (or an implicit run of stored slots for ONE query frame, as ScoreArgs' implicit items):
// per pair, good_count = number of query rows with best < ratio * second (knnMatch(k = 2) order, the second smallest
// distance counted with multiplicity; a row without a second neighbour does not count), min_dist = min of the best
// distances, n_train; the record layout is k_score_rowlane's.  The ratio test is the table lookup d1 < lim[d2]:
// lim[d2] = number of integers d1 in 0..256 with (double)d1 < ratio * (double)d2, built by the host.
constexpr int RATIO_LIM_ENTRIES = 258;          // d2 = 0..256, + one zero entry that "no second neighbour" is clamped to
struct RatioArgs {
    const uint32_t* q_rows;      // query frames: frame f at q_rows + f * q_stride_words, rows of 8 dwords
    const int32_t*  q_counts;    // rows per query frame (items != NULL)
    uint32_t        q_stride_words;
    const uint32_t* db_rows;     // stored frames, same layout, padded as the TRAIN role needs
    const int32_t*  db_counts;
    uint32_t        db_stride_words;
    const WorkItem* items;       // NULL => implicit: workgroup b = query frame 0 (imp_nq rows) against stored slots
                                 // [b * imp_spi, min((b + 1) * imp_spi, imp_total)), records at scores[slot]
    void*           scores;      // lcm_score records (8 bytes each)
    uint32_t        imp_spi, imp_total;
    int32_t         imp_nq;
    uint16_t        lim[RATIO_LIM_ENTRIES];
};
// max_query_rows = largest row count of any query frame referenced (<= MAX_FUSED_QUERY_ROWS): picks the workgroup shape
// (64 / 128 / 192 / 256 threads of 8 rows per lane), as launch_score does.
hipError_t launch_score_ratio(const RatioArgs& a, uint32_t n_items, int max_query_rows, hipStream_t st);

// The reference's own loop rule over a finished ratio score array (src/main.cpp:1379-1388: `rows < 100` skips a frame,
// matches.size() >= 300 accepts the pair): pair p belongs to query frame c = upper_bound(offsets, p) - 1 and stored slot
// p - offsets[c], as in LoopTestArgs; a candidate is q_rows[c] >= min_rows && n_train >= min_rows && good >= min_matches
// (n_train from the record).  The record written is (q_ids[c], db_ids[slot], good, good / min(q_rows[c], n_train)), the
// division in IEEE double (0.0 when an empty side is admitted by min_rows = 0) and not part of the verdict.  Candidates are
// compacted in pair order exactly as the loop test above does: k_ratio_loop_count (per 256-pair block), k_block_scan,
// k_ratio_loop_emit (wave-ballot rank).
struct RatioLoopArgs {
    const void*     scores;        // lcm_score records
    const uint32_t* offsets;       // n_q + 1 pair offsets per query frame
    const int32_t*  q_ids;         // per query frame
    const int32_t*  q_rows;        // descriptor rows per query frame
    const int32_t*  db_ids;        // per stored slot
    void*           out;           // lcm_loop_candidate records (24 bytes)
    uint32_t*       counter;       // number of candidates found (may exceed cap: count only)
    uint32_t*       block_counts;  // scratch: ceil(n_pairs / 256) words (candidates per block, then their prefix)
    uint32_t        n_q, n_pairs, cap;
    int32_t         min_rows, min_matches;
};
// The same two steps as launch_loop_count / launch_loop_emit.
hipError_t launch_ratio_loop_count(const RatioLoopArgs& a, hipStream_t st);
hipError_t launch_ratio_loop_emit(const RatioLoopArgs& a, hipStream_t st);

// On-device loop test over a finished score array (BASELINE.json configs[3] "fused on-device filter + loop test"):
// pair p belongs to query frame c = upper_bound(offsets, p) - 1 and stored slot p - offsets[c]; a candidate is
// similarity = good / min(kp_q, kp_t) > sim_threshold (IEEE double, strict) and good >= min_matches.  Candidates
// are compacted in pair order (count per 256-pair block, prefix scan, emit), which is (current id, matched id)
// ascending: the host does not sort.
struct LoopTestArgs {
    const void*     scores;        // lcm_score records
    const uint32_t* offsets;       // n_q + 1 pair offsets per query frame
    const int32_t*  q_ids;         // per query frame
    const int32_t*  q_kp;          // keypoint count per query frame
    const int32_t*  db_ids;        // per stored slot
    const int32_t*  db_kp;
    void*           out;           // lcm_loop_candidate records (24 bytes)
    uint32_t*       counter;       // number of candidates found (may exceed cap: count only)
    uint32_t*       block_counts;  // scratch: ceil(n_pairs / 256) words (candidates per block, then their prefix)
    uint32_t        n_q, n_pairs, cap;
    int32_t         min_matches;
    double          sim_threshold;
};
// Two steps, so that the host can size the candidate buffer from the count (and refuse a too-small `cap` before any
// worst-case allocation): launch_loop_count leaves the number of candidates in *counter (and the per-block prefix in
// block_counts); launch_loop_emit then writes candidate k < cap to out[k].
hipError_t launch_loop_count(const LoopTestArgs& a, hipStream_t st);
hipError_t launch_loop_emit(const LoopTestArgs& a, hipStream_t st);
// k_block_scan on its own (the ratio loop test in lcm_ratio.hip shares it): counts[0..n) -> exclusive prefix sums in
// place, *total = their sum.
hipError_t launch_block_scan(uint32_t* counts, uint32_t n, uint32_t* total, hipStream_t st);

// Cross-check (lcm_params.cross_check, BFMatcher crossCheck = true): per pair, forward keys (every query row's first
// nearest train row) and backward keys (every train row's first nearest query row) -> the pair's score record.
//   mode 1 (mutual):  query q keeps (d, j) = fkey[q] iff bkey[j].idx == q
//   mode 2 (legacy):  query q keeps min over the train rows t with bkey[t].idx == q of (bkey[t].dist, t)
// then the usual min-of-mins / ratio filter / count over the queries that kept a match.
struct CrossDesc {
    uint32_t f_slot;             // forward keys at keys + f_slot * MAX_FUSED_QUERY_ROWS (nq <= 2048 entries)
    uint32_t b_slot;             // backward keys at keys + b_slot * MAX_FUSED_QUERY_ROWS (nt entries, contiguous)
    uint32_t nq, nt;
    uint32_t out;                // record index in scores
};
struct CrossArgs {
    const uint32_t*  keys;
    const CrossDesc* descs;
    void*            scores;
    uint32_t*        idx_sums;   // optional
    int32_t          mode, ratio, dist_floor;
};
hipError_t launch_cross_score(const CrossArgs& a, uint32_t n_pairs, hipStream_t st);

// Give every frame of a row matrix the padding the TRAIN role needs: rows [n, round_up(n, 4) + 4) of frame f become
// copies of its row n - 1 (n = counts[f]; nothing is written for n == 0).  stride_rows >= round_up(max n, 4) + 4.
hipError_t launch_pad_rows(uint32_t* rows, const int32_t* counts, uint32_t stride_rows, uint32_t n_frames, hipStream_t st);

// ---- OPT-IN matrix-core variant (lcm_set_kernel_variant(4)) ---------------------------------------------------------
// BASELINE.json's north_star rules MFMA out for the product path ("this path is integer bitwise work"), and variants
// 0 / 1 honour that.  Variant 4 exists to MEASURE what the rule costs: the same exact integers from
// v_mfma_i32_32x32x32_i8.  With every descriptor bit mapped to an int8 +1 / -1, <q, t> = 256 - 2 * hamming(q, t), so
// min distance = max dot product, exactly, in int32.
//
// Expanded operand image ("pm1"): per frame, per tile of 32 rows, per k-step of 32 bits: 64 lanes x 16 bytes =
// 1 KiB, lane (r = lane & 31, h = lane >> 5) holding bits [32 ks + 16 h, +16) of row 32 tile + r as 16 int8 — exactly
// one MFMA operand fragment per lane, so a wave's fragment load is one coalesced, conflict-free 1 KiB block.  Rows
// past a frame's end repeat its last row (cannot beat it).  8 KiB per tile = 8x the packed bytes.
constexpr int PM1_TILE_BYTES = 8192;
hipError_t launch_expand_pm1(const uint32_t* rows, const int32_t* counts, uint32_t stride_words, uint32_t n_frames,
                             uint32_t tiles_per_frame, uint8_t* pm1, hipStream_t st);

// One workgroup (4 waves) = 256 query rows (chunk q_chunk of query frame q_frame) against stored slots
// [slot_begin, slot_begin + n_slots): wave w keeps query tiles 2w, 2w+1 of the chunk in registers as B operands (64
// VGPRs), the stored frame's tiles stream through LDS as A operands (double-buffered, shared by the 4 waves), 16 MFMAs
// per tile per wave, running max per query in registers.  Output: best DISTANCE per (pair, query row) -> dist; the
// per-pair records come from launch_finalize_bulk (min-of-mins, ratio filter, count).
struct MfmaItem { uint32_t q_frame, q_chunk, slot_begin, n_slots, out_offset; };
struct MfmaArgs {
    const uint8_t*  q_pm1;  uint32_t q_tiles_per_frame;  const int32_t* q_counts;    // query frames (expanded)
    const uint8_t*  db_pm1; uint32_t db_tiles_per_frame; const int32_t* db_counts;   // stored frames (expanded)
    const MfmaItem* items;
    uint32_t*       dist;          // dist[(out_offset + s - pair_base) * 2048 + query row]
    uint32_t        pair_base;
    // ARGMIN form (argmin != 0): dist receives packed keys `distance << 22 | first train row attaining it`.  The matrix
    // instruction finds, per query row, the best dot product and the FIRST 32-row tile that reaches it; the lane then
    // re-scans that one tile on the vector ALU over the ORIGINAL packed rows (exact XOR + popcount) for the first row.
    int32_t         argmin;
    const uint32_t* q_rows;  uint32_t q_stride_words;    // packed query frames (frame f at q_rows + f * q_stride_words)
    const uint32_t* db_rows; uint32_t db_stride_words;   // packed stored frames
};
hipError_t launch_score_mfma(const MfmaArgs& a, uint32_t n_items, hipStream_t st);

// Variant 5: the same on v_mfma_scale_f32_32x32x64_f8f6f4 with fp4 operands (+1 = 0x2, -1 = 0xA, scales 1.0): 4 KiB
// per tile of 32 rows (4 k-steps of 64 bits), one workgroup = 512 query rows (q_chunk counts 512-row chunks).
constexpr int FP4_TILE_BYTES = 4096;
hipError_t launch_expand_fp4(const uint32_t* rows, const int32_t* counts, uint32_t stride_words, uint32_t n_frames,
                             uint32_t tiles_per_frame, uint8_t* img, hipStream_t st);
hipError_t launch_score_mfma_fp4(const MfmaArgs& a, uint32_t n_items, hipStream_t st);

// Fold of per-row words into score records, one wave per pair.  Which pair a scratch slot l (0 <= l < n_pairs) is:
//   * pk_pairs == NULL (matrix-core variants): global pair p = pair_base + l belongs to query c = last c with
//     offsets[c] <= p and is stored slot p - offsets[c];
//   * pk_pairs != NULL (packed route, a chunk = group of query frames x range of stored slots): l belongs to the group's
//     frame k = last k with pk_pairs[k] <= l, is stored slot slot0 + l - pk_pairs[k], query c = pk_cidx[k], and its
//     record is scores[offsets[c] + slot].
// Folds dist[l * stride + r], r < nq[c].
struct FinalizeBulkArgs {
    uint32_t        stride;        // words of dist per pair (0 = MAX_FUSED_QUERY_ROWS); a multiple of 8
    uint32_t        word_bytes;    // 4 (0 means 4): dist holds uint32 words; 2: uint16 distances, 0xFFFF = none (packed
                                   // route, distance-only mode: halves the scratch traffic); keys are always 4 bytes
    int32_t         key_shift;     // 0: dist holds distances; KEY_SHIFT: packed keys dist << 22 | train row
    uint32_t*       idx_sums;      // optional (keys): per pair, sum of the good matches' train rows mod 2^32
    const uint32_t* dist;
    const uint32_t* offsets;       // n_q + 1
    const int32_t*  nq;            // n_q query row counts
    const int32_t*  db_counts;
    void*           scores;        // records at scores[p]
    uint32_t        n_q, pair_base;
    int32_t         ratio, dist_floor;
    const uint32_t* pk_pairs;      // packed route: pk_n + 1 local pair offsets of the group's frames in this chunk
    const uint32_t* pk_cidx;       // packed route: query index c of the group's frame k
    uint32_t        pk_n, slot0;
};
hipError_t launch_finalize_bulk(const FinalizeBulkArgs& a, uint32_t n_pairs, hipStream_t st);

// Multi-GPU merge (lcm_group_*): the W per-shard score arrays, gathered back to back on one device, are un-permuted
// into the single-device (query ascending, stored ascending) order.  Shard r's records are in (query ascending, owned
// stored ascending) order; query c's k-th record of shard r is stored position r + k * W, so it lands at
// offsets[c] + r + k * W.  HBM-bound: 8 bytes read + 8 bytes written per pair.
struct MergeArgs {
    const void*     gathered;      // all shards' lcm_score records, shard r at record index shard_base[r]
    void*           merged;        // output, n_total records
    const uint32_t* shard_offsets; // W arrays of n_q + 1 per-query offsets inside shard r (shard-local record index)
    const uint32_t* offsets;       // n_q + 1 per-query offsets of the merged array
    uint32_t        shard_base[9]; // W + 1 entries (W <= 8)
    uint32_t        world, n_q, n_total;
    uint32_t        elem_words;    // 2: lcm_score records (0 means 2); 1: the argmin search's per-pair index checksums
};
hipError_t launch_merge_shards(const MergeArgs& a, hipStream_t st);

}  // namespace lcm
