// lcm_l2_db.cpp — the SIFT keyframe store (include/lcm.h, lcm_l2_db_*): uploaded and packed matrices stay on the device and are
// searched from tables that grow with the frames (lcm_l2_store.hip; planned in lcm_l2_host.h).  Its pair calls run lcm_l2.cpp's
// list and count runs over the store's slots; its list calls make the lists on the device (lcm_l2_emit.hip) and can hand the point
// records straight to the loop verification (lcm_epi_db_*, lcm_lo_db_*, lcm_pose_db_*: store_lists runs the call's lcm::VerifyPlan
// through lcm_verify.cpp's pipeline; the best loop is chosen on the host).  Shared state and helpers: lcm_internal.h.
#include "lcm_internal.h"

#include <functional>

namespace {

constexpr int TILE = lcm::L2_TILE_ROWS, ROW = LCM_SIFT_BYTES;
using L2Store = lcm_handle::L2Store;
using StoreCurr = lcm::L2StoreCurr;
using lcm::VerifyPlan;                      // the loop verification behind the store's list calls (lcm_verify.cpp)

// Three arenas in one tile space (lcm_kernels.h): slot f's frame occupies tiles [tile0[f], tile0[f + 1]), the tail from
// tile0[size] on is free (a host query of lcm_l2_db_detect_loops is staged there).  k_l2_pack writes all 32 rows of every tile
// it is given, image and words, so the pad rows of a frame's last tile are rewritten whatever a truncated frame left there
// (the padding trap); the raw pad rows keep old bytes, which nothing reads (k_l2_rescan walks rows < nt).  A fourth arena,
// 8 bytes per row, holds the keypoints of the frames that came with them (lcm_l2_db_append_kp); its pad rows keep old points,
// which nothing reads either (k_l2_emit gathers rows < nq and train indices < nt).

size_t tiles_of(int n) { return (size_t)((n + TILE - 1) / TILE); }

// Where the store's matrices are: its arenas and its own tile0 (the free tail at tile0[size]); nothing to upload or pack
L2Where where_store(const L2Store& d) { return L2Where{d.d_raw, d.d_img, d.d_tw, d.tile0.data()}; }

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
    int rc = lcm::l2_check_rows(n); if (rc) return rc;
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

// A slot's rows (kp == false: `out` holds cap_rows x 128 bytes) or its keypoints (kp: cap_rows x (x, y) floats) back to the host
int l2_db_read_impl(lcm_handle* h, int slot, void* out, int cap_rows, bool kp) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    int rc = check_slot(h, slot); if (rc) return rc;
    const L2Store& d = h->l2db;
    if (kp && !d.has_pts[(size_t)slot]) return fail(LCM_ERR_INVALID_ARG, "slot %d was stored without points", slot);
    const int n = d.rows[(size_t)slot];
    if (cap_rows < n) return fail(LCM_ERR_CAPACITY, "slot %d holds %d rows but the buffer %d", slot, n, cap_rows);
    if (n == 0) return LCM_OK;
    if (!out) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    rc = set_device(h); if (rc) return rc;
    const size_t tile = d.tile0[(size_t)slot];
    if (kp) HIP_TRY(hipMemcpyAsync(out, d.d_pts + tile * TILE, (size_t)n * sizeof(uint2), hipMemcpyDeviceToHost, h->stream));
    else HIP_TRY(hipMemcpyAsync(out, d.d_raw + tile * lcm::L2_TILE_BYTES, (size_t)n * ROW, hipMemcpyDeviceToHost, h->stream));
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

int l2_db_info_impl(lcm_handle* h, lcm_l2_db_info* out) {
    if (!h || !out) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    const L2Store& d = h->l2db;
    *out = lcm_l2_db_info{(int32_t)d.rows.size(), 0, d.tile0.back(), d.cap_tiles,
                          d.cap_tiles * (2 * (uint64_t)lcm::L2_TILE_BYTES + TILE * sizeof(uint32_t) + (d.d_pts ? TILE * sizeof(uint2) : 0)) +
                              d.d_frames_cap * sizeof(uint2),
                          d.last_table_bytes};
    return LCM_OK;
}

// ---- the loop search over the store (lcm_l2_store.hip) ---------------------------------------------------------------------------
// src/main.cpp:1375-1388 over the store, `currs` ascending (l2_store_plan).  k_l2_count_store scores the pairs with two non-empty
// sides from [runs | live admitted slots]; the verdict and the compaction run on the host over the records (l2_candidates_out).
int store_search(lcm_handle* h, const std::vector<StoreCurr>& currs, const uint8_t* skip, const lcm_ratio_loop_params& rp,
                 lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out) {
    L2Store& d = h->l2db;
    lcm::L2StorePlan pl;
    int rc = lcm::l2_refused(lcm::l2_store_plan(d.rows.data(), d.rows.size(), currs, skip, rp.min_rows, pl)); if (rc) return rc;
    const lcm_l2_score* rec = nullptr;
    d.last_table_bytes = 0;
    if (!pl.runs.empty()) {
        auto& s = h->l2;
        const size_t n_rec = (size_t)pl.n_rec;
        const size_t off_past = pl.runs.size() * sizeof(lcm::L2StoreRun);
        const size_t tab_bytes = off_past + pl.live.size() * sizeof(uint32_t);
        std::vector<uint8_t> tab(tab_bytes);
        memcpy(tab.data(), pl.runs.data(), off_past);
        memcpy(tab.data() + off_past, pl.live.data(), pl.live.size() * sizeof(uint32_t));
        rc = ensure_dev(d.d_tab, d.d_tab_n, tab_bytes); if (rc) return rc;
        rc = ensure_dev(s.d_score, s.d_score_n, n_rec); if (rc) return rc;
        rc = ensure_pinned(s.h_score, s.h_score_n, n_rec); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(d.d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, h->stream));
        hipError_t e = lcm::launch_l2_count_init(s.d_score, (uint32_t)n_rec, h->stream);
        if (e != hipSuccess) return fail(LCM_ERR_HIP, "count init kernel launch failed: %s", hipGetErrorString(e));
        const lcm::L2StoreArgs sa{d.d_img, d.d_tw, reinterpret_cast<const lcm::L2StoreRun*>(d.d_tab),
                                  reinterpret_cast<const uint32_t*>(d.d_tab + off_past), d.d_frames, s.d_score, rp.ratio,
                                  (uint32_t)pl.runs.size(), (uint32_t)pl.chunk_rows};
        HIP_TRY(hipEventRecord(h->ev_start, h->stream));
        e = lcm::launch_l2_count_store(sa, (uint32_t)pl.n_wg, h->stream);
        if (e != hipSuccess) return fail(LCM_ERR_HIP, "count kernel launch failed: %s", hipGetErrorString(e));
        HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
        h->info_pending = true;
        h->info.workgroups = (uint32_t)pl.n_wg; h->info.route = LCM_ROUTE_PLAIN; h->info.launches = 2;
        h->info.pairs = n_rec; h->info.distances = pl.distances; h->info.algo_bytes = tab_bytes + n_rec * sizeof(lcm_l2_score);
        HIP_TRY(hipMemcpyAsync(s.h_score, s.d_score, n_rec * sizeof(lcm_l2_score), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        rec = s.h_score;
        d.last_table_bytes = tab_bytes;
    }

    return lcm::l2_candidates_out(pl, d.rows.data(), d.rows.size(), currs, rec, rp.min_matches, out, cap, n_out, n_pairs_out);
}

// what lcm_loop_search_ratio_l2 checks before it looks at a matrix
int store_search_args(lcm_handle* h, int loop_gap, const lcm_ratio_loop_params* rp_in, size_t* n_out, size_t* n_pairs_out,
                      lcm_ratio_loop_params* rp) {
    if (!h || !n_out) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    if (n_pairs_out) *n_pairs_out = 0;
    if (loop_gap < 1) return fail(LCM_ERR_INVALID_ARG, "loop_gap must be >= 1");
    int rc = lcm::ratio_loop_params_checked(rp_in, rp); if (rc) return rc;
    rc = lcm::l2_check_knn(h, rp->ratio); if (rc) return rc;
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

// A host query of nq rows (checked by the caller), and its points if any -> the store's free tail, enqueued; *c says where.
// `meta`, `query` and `query_pts` are read until the caller has waited for the stream; on a failure this function has waited.
int store_stage_query(lcm_handle* h, const uint8_t* query, const float* query_pts, int nq, std::vector<uint32_t>& meta, StoreCurr* c) {
    const size_t first = h->l2db.tile0.back();
    int rc = store_reserve(h, std::max<size_t>(first + tiles_of(nq), 1));
    if (rc == LCM_OK) rc = store_put(h, query, nq, first, meta);
    if (rc == LCM_OK && query_pts) rc = store_put_pts(h, query_pts, nq, first);
    if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
    c->q_tile = (uint32_t)first; c->q_rows = nq;
    return LCM_OK;
}

int l2_db_detect_loops_impl(lcm_handle* h, int curr, const uint8_t* query, int nq, const uint8_t* skip, int loop_gap,
                            const lcm_ratio_loop_params* rp_in, lcm_loop_candidate* out, size_t cap, size_t* n_out, size_t* n_pairs_out) {
    lcm_ratio_loop_params rp;
    int rc = store_search_args(h, loop_gap, rp_in, n_out, n_pairs_out, &rp); if (rc) return rc;
    L2Store& d = h->l2db;
    StoreCurr c{curr, 0, 0, 0};
    std::vector<uint32_t> meta;
    if (query) {
        rc = lcm::l2_check_rows(nq); if (rc) return rc;
        rc = store_stage_query(h, query, nullptr, nq, meta, &c); if (rc) return rc;      // `meta` and `query` live until store_search has waited
    } else {
        rc = check_slot(h, curr); if (rc) return rc;
        c.q_tile = d.tile0[(size_t)curr]; c.q_rows = d.rows[(size_t)curr];
    }
    c.last_past = (int)std::max<long long>((long long)curr - loop_gap, -1);
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
// after != NULL (with a plan): called behind the plan's stages with the device's point records, offsets and match records and the
// record count, before anything of the lists is copied back; it may wait for the stream, adds its launches and may refuse.
using StoreAfter = std::function<int(const uint4* d_pts, const uint64_t* d_off, const uint4* d_rec, size_t total, uint32_t* launches)>;
int store_lists(lcm_handle* h, const int* rows, const std::vector<L2Pair>& live, const std::vector<int>& job_of, double ratio,
                lcm_dmatch* out, lcm_point_pair* pts, size_t cap, size_t* offsets, const VerifyPlan* plan = nullptr,
                const StoreAfter* after = nullptr) {
    const size_t n_pairs = job_of.size();
    if (live.empty()) {
        std::fill(offsets, offsets + n_pairs + 1, (size_t)0);
        if (plan) lcm::verify_empty(*plan, n_pairs);
        return LCM_OK;
    }
    L2Store& d = h->l2db;
    if (pts && !d.d_pts) return fail(LCM_ERR_INVALID_ARG, "the store holds no points");
    L2Run run;                                      // its table block is in flight until the wait below
    int rc = set_device(h); if (rc) return rc;
    rc = lcm::l2_refused(lcm::l2_run_plan(live, rows, d.tile0.data(), run.plan)); if (rc) return rc;
    rc = lcm::l2_enqueue(h, where_store(d), run); if (rc) return rc;
    const lcm::L2RunPlan& rp = run.plan;
    const size_t P = live.size(), total_rows = rp.row0[P];

    // [first block of the first live pair at or after p, p <= n_pairs | survivors per block, + their total]
    std::vector<uint32_t> pair_block;
    lcm::l2_pair_block(job_of, rp.jobs, rp.n_blocks, pair_block);
    auto& s = h->l2;
    rc = ensure_dev(s.d_blocks, s.d_blocks_n, n_pairs + 1 + rp.n_blocks + 1); if (rc) return rc;
    rc = ensure_dev(s.d_offsets, s.d_offsets_n, n_pairs + 1); if (rc) return rc;
    uint32_t* d_blocks = s.d_blocks + n_pairs + 1;
    HIP_TRY(hipMemcpyAsync(s.d_blocks, pair_block.data(), (n_pairs + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    lcm::L2EmitArgs ea{s.d_fin, run.d_jobs, d_blocks, nullptr, nullptr, nullptr, ratio, 0, 0};
    uint32_t slices = 0;
    rc = lcm::pair_slices(P, &slices); if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev_aux_start, h->stream));
    hipError_t e = lcm::launch_l2_emit_count(ea, (uint32_t)P, (uint32_t)rp.max_nq, h->stream);
    if (e == hipSuccess) e = lcm::launch_block_scan(d_blocks, (uint32_t)rp.n_blocks, d_blocks + rp.n_blocks, h->stream);
    if (e == hipSuccess) e = lcm::launch_l2_emit_offsets(d_blocks, s.d_blocks, s.d_offsets, (uint32_t)(n_pairs + 1), h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "list count kernels: launch failed: %s", hipGetErrorString(e));
    h->info.launches += slices + 2;
    HIP_TRY(hipMemcpyAsync(offsets, s.d_offsets, (n_pairs + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));       // also: the run's tables and pair_block (pageable) have been consumed
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
        e = lcm::launch_l2_emit(ea, (uint32_t)P, (uint32_t)rp.max_nq, h->stream);
        if (e != hipSuccess) return fail(LCM_ERR_HIP, "list kernel launch failed: %s", hipGetErrorString(e));
        h->info.launches += slices;
    }
    if (plan) {                                     // a pair's records are at most its query rows: they fit the packed key
        uint32_t max_n = 0, launches = 0;
        for (size_t p = 0; p < n_pairs; ++p) max_n = std::max(max_n, (uint32_t)(offsets[p + 1] - offsets[p]));
        rc = lcm::verify_enqueue(h, *plan, s.d_rec_pts, s.d_offsets, n_pairs, max_n, total, &launches); if (rc) return rc;
        h->info.launches += launches;
        if (after) {
            rc = (*after)(s.d_rec_pts, s.d_offsets, s.d_rec, total, &launches);
            h->info.launches += launches;
            if (rc) {
                HIP_TRY(hipEventRecord(h->ev_aux_stop, h->stream));
                h->aux_pending = true;
                return rc;
            }
        }
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
                            size_t cap, size_t* offsets, const VerifyPlan* plan = nullptr, const StoreAfter* after = nullptr) {
    if (!h || n_pairs < 0 || !offsets || (n_pairs > 0 && !slots)) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (plan) { const int rc = plan_checked(*plan, pts, (size_t)n_pairs); if (rc) return rc; }
    offsets[0] = 0;
    int rc = lcm::l2_check_knn(h, ratio); if (rc) return rc;
    const L2Store& d = h->l2db;
    std::vector<L2Pair> live;
    std::vector<int> job_of;
    rc = lcm::l2_read_pairs(slots, (size_t)n_pairs, d.rows.data(), (int)d.rows.size(), live, job_of, [&](int q, int t) -> int {
        if (!pts) return LCM_OK;
        if (const int r = check_slot_pts(d, q)) return r;
        return check_slot_pts(d, t);
    });
    if (rc) return rc;
    return store_lists(h, d.rows.data(), live, job_of, ratio, out, pts, cap, offsets, plan, after);
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
        rc = lcm::l2_check_rows(nq); if (rc) return rc;
        if (pts && !query_pts) return fail(LCM_ERR_INVALID_ARG, "point pairs are wanted but the query has no points");
    } else {
        rc = check_slot(h, curr); if (rc) return rc;
        if (pts) { rc = check_slot_pts(d, curr); if (rc) return rc; }
        c.q_tile = d.tile0[(size_t)curr]; c.q_rows = d.rows[(size_t)curr];
    }
    // everything from the staging on: whatever happens, the caller's rows and points have been consumed on return
    auto body = [&]() -> int {
        int r = query ? store_stage_query(h, query, query_pts, nq, meta, &c) : LCM_OK; if (r) return r;
        c.last_past = (int)std::max<long long>((long long)curr - loop_gap, -1);
        std::vector<StoreCurr> currs;
        if (c.q_rows >= rp.min_rows) currs.push_back(c);                        // :1382
        r = store_search(h, currs, skip, rp, cands, cand_cap, n_cands, n_pairs_out); if (r) return r;
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
        return store_lists(h, rows_ext.data(), live, job_of, rp.ratio, out, pts, cap, offsets, plan);
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

// lcm_map_db_track: lcm_{pose,lo}_db_verify_pairs on the one pair {last, curr}, with the map's stages (lcm_map.cpp) behind the
// verification on the records it left on the device.  A list by knnMatch names every query row once and only rows of the two
// slots, so what lcm_map_merge checks about a host list holds by construction; the tables and the buffers are checked here.
int map_db_track_impl(lcm_handle* h, int last_slot, int curr_slot, double ratio, lcm_dmatch* out, lcm_point_pair* pts, size_t cap,
                      size_t* offsets, VerifyPlan* plan, const lcm_lo_params* lp, const lcm_pose_params* pp, lcm::MapTrack t) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    int rc = check_slot(h, last_slot); if (rc) return rc;
    rc = check_slot(h, curr_slot); if (rc) return rc;
    t.n_kp_last = h->l2db.rows[(size_t)last_slot]; t.n_kp_new = h->l2db.rows[(size_t)curr_slot];
    rc = lcm::map_track_checked(h, t, 0); if (rc) return rc;
    rc = lcm::verify_params_checked(plan, lp, pp); if (rc) return rc;
    const lcm_pair_ref slots{last_slot, curr_slot};
    bool ran = false;
    const StoreAfter after = [&](const uint4* d_pts, const uint64_t* d_off, const uint4* d_rec, size_t total, uint32_t* launches) {
        ran = true;
        return lcm::map_track_stages(h, t, d_pts, d_off, d_rec, (uint32_t)total, launches);
    };
    rc = l2_db_match_points_impl(h, &slots, 1, ratio, out, pts, cap, offsets, plan, &after); if (rc) return rc;
    if (!ran) {                                     // a slot without rows: an empty list, nothing was launched
        uint32_t launches = 0;
        return lcm::map_track_stages(h, t, nullptr, nullptr, nullptr, 0, &launches);
    }
    return LCM_OK;
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

}  // namespace

extern "C" {

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
    return guarded([&] { return l2_db_read_impl(h, slot, out, cap_rows, false); });
}
int lcm_l2_db_truncate(lcm_handle* h, int n_frames) { return guarded([&] { return l2_db_truncate_impl(h, n_frames); }); }
int lcm_l2_db_clear(lcm_handle* h) { return guarded([&] { return l2_db_truncate_impl(h, 0); }); }
int lcm_l2_db_info_read(lcm_handle* h, lcm_l2_db_info* out) { return l2_db_info_impl(h, out); }
int lcm_l2_db_score_pairs(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio, lcm_l2_score* scores) {
    return guarded([&] {
        if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
        const L2Where w = where_store(h->l2db);
        return lcm::l2_score_pairs(h, nullptr, h->l2db.rows.data(), (int)h->l2db.rows.size(), slots, n_pairs, ratio, scores, &w);
    });
}
int lcm_l2_db_match_pairs_ratio(lcm_handle* h, const lcm_pair_ref* slots, int n_pairs, double ratio, lcm_dmatch* out, size_t cap,
                                size_t* offsets) {
    return guarded([&] {
        if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
        const L2Where w = where_store(h->l2db);
        return lcm::l2_match_pairs(h, nullptr, h->l2db.rows.data(), (int)h->l2db.rows.size(), slots, n_pairs, ratio, out, cap, offsets, &w);
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
    return guarded([&] { return l2_db_read_impl(h, slot, out, cap_rows, true); });
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
int lcm_map_db_track(lcm_handle* h, int last_slot, int curr_slot, double ratio, const lcm_epi_params* ep, const lcm_lo_params* lp,
                     const lcm_pose_params* pp, lcm_epi_result* result, lcm_lo_info* info, lcm_pose_result* pose_result, lcm_dmatch* out,
                     lcm_point_pair* pts, uint8_t* mask, uint8_t* pose_mask, size_t cap, size_t* offsets, int kf_last,
                     const lcm_pgo_pose* pose_last, int32_t* table_last, int kf_new, int32_t* table_new, int n_points,
                     const lcm_map_params* mp, lcm_ba_point* points_out, int cap_points, lcm_ba_obs* obs_out, int cap_obs,
                     uint8_t* status_out, lcm_map_keyframe_report* report) {
    return guarded([&] {
        VerifyPlan w{ep, lp != nullptr, true, result, mask, info, pose_result, pose_mask};
        const lcm::MapTrack t{mp, kf_last, kf_new, pose_last, table_last, 0, table_new, 0, n_points, points_out, cap_points, obs_out, cap_obs,
                              status_out, report};
        return map_db_track_impl(h, last_slot, curr_slot, ratio, out, pts, cap, offsets, &w, lp, pp, t);
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

}  // extern "C"
