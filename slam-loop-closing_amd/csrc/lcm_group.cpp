// lcm_group.cpp — the frame-sharded multi-GPU loop search behind the C ABI (include/lcm.h, lcm_group_*).
//
// One PROCESS, one lcm_handle per device, one host thread per device for the per-shard work, RCCL (single-process
// ncclCommInitAll communicator) for the exchange steps over xGMI:
//
//   * stored frame with arrival position p is owned by device p mod W (cyclic: balances the triangular all-vs-all and
//     the growing streaming database);
//   * every device needs every frame as a QUERY: the shard arenas are all-gathered (ncclAllGather, the only bulk
//     transfer: N x D x 32 bytes once per search) into a rank-major query buffer per device; work items address
//     query frame p at index (p mod W) * shard_cap + p / W, so no re-packing pass is needed;
//   * each device scores all N query frames against the frames it owns (lcm::all_vs_all on its own stream, planned and
//     launched from its own host thread);
//   * the per-shard 8-byte score records are gathered to device 0 (grouped ncclSend / ncclRecv: a gatherv, shards
//     differ by up to one frame per query), un-permuted there by k_merge_shards into the single-device
//     (query ascending, stored ascending) order, and copied to the host once.
//
// What include/loop_closing.hpp:29-31 would call: a LoopClosingSystem constructed with n_devices > 1 holds an
// lcm_group instead of an lcm_handle.
//
// This file: the two merge entry points, create / destroy, the database calls, snapshot, the online queries.  The bulk
// search is lcm_group_search.cpp; the sharding arithmetic lcm_group_host.h; the group's own state lcm_group_internal.h.
#include "lcm_group_internal.h"

using lcm::eligible_count;
using lcm::GTicket;
using lcm::shard_share;
using lcm::Worker;

extern "C" {

/* The group's merge step on its own: d_gathered (device) holds the W shard arrays back to back, shard r's
 * shard_counts[r] records in (query ascending, owned stored ascending) order; d_merged (device) receives the
 * single-device order.  Runs k_merge_shards on the handle's stream; lcm_sync(h) before reading the result. */
int lcm_merge_shard_scores_device(lcm_handle* h, const void* d_gathered, const size_t* shard_counts, int world,
                                  const int32_t* ids, int n_frames, int min_gap, void* d_merged, size_t cap, size_t* n_out) {
    if (!h || world < 1 || world > MAX_WORLD || n_frames < 0 || !n_out || !shard_counts || (n_frames > 0 && !ids))
        return fail(LCM_ERR_INVALID_ARG, "bad argument");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(h->device));
        std::vector<GFrame> f((size_t)n_frames);
        for (int i = 0; i < n_frames; ++i) {
            if (i > 0 && ids[i] <= ids[i - 1]) return fail(LCM_ERR_ORDER, "frame ids must be strictly increasing");
            f[(size_t)i] = {ids[i], 0, 0};
        }
        lcm::ShardLayout<uint32_t> L;
        if (const char* what = lcm::shard_layout(f, world, min_gap, L)) return fail(LCM_ERR_CAPACITY, "%s", what);
        const uint64_t total = L.total;
        *n_out = (size_t)total;
        for (int r = 0; r < world; ++r)
            if (shard_counts[r] != L.shard_total(r))
                return fail(LCM_ERR_INVALID_ARG, "shard %d holds %zu records, expected %u", r, shard_counts[r], L.shard_total(r));
        if (!d_merged || total == 0) return LCM_OK;
        if (!d_gathered) return fail(LCM_ERR_INVALID_ARG, "d_gathered is NULL");
        if (cap < total) return fail(LCM_ERR_CAPACITY, "merged array needs %llu records, room for %zu", (unsigned long long)total, cap);
        size_t have = h->d_meta_n;
        int32_t* p = h->d_meta;
        int rc = ensure_dev(p, have, (size_t)(world + 1) * ((size_t)n_frames + 1));
        h->d_meta = p; h->d_meta_n = have;
        if (rc) return rc;
        rc = upload_merge_meta(reinterpret_cast<uint32_t*>(h->d_meta), L, h->stream); if (rc) return rc;
        rc = merge_on_device(d_gathered, d_merged, reinterpret_cast<uint32_t*>(h->d_meta), L, 2, h->stream); if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));       // the offset uploads came from this call's stack
        return LCM_OK;
    });
}

/* Host-only: the un-permutation lcm_group_all_vs_all performs on the device (and sharding.merge_shard_scores performs
 * in numpy), for callers that gathered the shards themselves and for the CPU unit tests of the index arithmetic. */
int lcm_merge_shard_scores(const lcm_score* const* shard_scores, const size_t* shard_counts, int world,
                           const int32_t* ids, int n_frames, int min_gap,
                           lcm_score* out, size_t cap, size_t* n_out, size_t* offsets) {
    if (world < 1 || n_frames < 0 || !n_out || (n_frames > 0 && !ids) || !shard_scores || !shard_counts)
        return fail(LCM_ERR_INVALID_ARG, "bad argument");
    return guarded([&]() -> int {
        for (int i = 1; i < n_frames; ++i)
            if (ids[i] <= ids[i - 1]) return fail(LCM_ERR_ORDER, "frame ids must be strictly increasing");
        std::vector<GFrame> f((size_t)n_frames);
        for (int i = 0; i < n_frames; ++i) f[(size_t)i] = {ids[i], 0, 0};
        lcm::ShardLayout<size_t> L;                     // size_t offsets: no pair count is refused here
        (void)lcm::shard_layout(f, world, min_gap, L);
        const size_t total = (size_t)L.total;
        *n_out = total;
        if (offsets) memcpy(offsets, L.offs.data(), sizeof(size_t) * ((size_t)n_frames + 1));
        for (int r = 0; r < world; ++r)                 // every shard must hold exactly its share
            if (shard_counts[r] != L.shard_total(r)) return fail(LCM_ERR_INVALID_ARG, "shard %d holds %zu records, expected %zu", r, shard_counts[r], L.shard_total(r));
        if (!out) return LCM_OK;                        // sizing call
        if (cap < total) return fail(LCM_ERR_CAPACITY, "merged array needs %zu records, room for %zu", total, cap);
        lcm::merge_shards_host(L, shard_scores, out);
        return LCM_OK;
    });
}


static int group_create(const lcm_params* params, int n_devices, const int* device_ids, bool loopback, int loop_device, bool peer_copies, lcm_group** out) {
    if (!out) return fail(LCM_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (n_devices < 1 || n_devices > MAX_WORLD) return fail(LCM_ERR_INVALID_ARG, "n_devices must be 1..%d", MAX_WORLD);
    const int have = lcm_device_count();
    if (have <= 0) {
        lcm_handle* probe = nullptr;
        return lcm_create(params, 0, nullptr, &probe);        // "no HIP device ... no CPU fallback"
    }
    return guarded([&]() -> int {
        lcm_group* g = new lcm_group();
        auto bail = [&](int rc) { const std::string why = lcm::last_error(); lcm_group_destroy(g); lcm::last_error() = why; return rc; };
        g->world = n_devices;
        g->loopback = loopback;
        g->copies = loopback || peer_copies;
        lcm_params_default(&g->params);
        if (params) g->params = *params;
        int devs[MAX_WORLD];
        for (int r = 0; r < n_devices; ++r) {
            const int dev = loopback ? loop_device : (device_ids ? device_ids[r] : r);
            if (dev < 0 || dev >= have) return bail(fail(LCM_ERR_INVALID_ARG, "device id %d out of range [0,%d)", dev, have));
            if (!loopback) for (int q = 0; q < r; ++q) if (devs[q] == dev) return bail(fail(LCM_ERR_INVALID_ARG, "device id %d listed twice", dev));
            devs[r] = dev;
        }
        for (int r = 0; r < n_devices; ++r) {
            lcm_handle* h = nullptr;
            const int rc = lcm_create(&g->params, devs[r], nullptr, &h);
            if (rc) return bail(rc);
            g->shards.emplace_back();
            Shard& S = g->shards.back();
            S.h = h; S.device = devs[r];
            if (r > 0) S.worker.reset(new Worker());
        }
        if (!g->copies) {
            ncclComm_t comms[MAX_WORLD] = {};
            ncclResult_t nr = ncclCommInitAll(comms, n_devices, devs);
            if (nr == ncclSuccess) {
                for (int r = 0; r < n_devices; ++r) g->shards[(size_t)r].comm = comms[r];
            } else {
                // no communicator: the group still works, its two exchange steps fall back to peer copies
                g->copies = true;
                g->rccl_error = ncclGetErrorString(nr);
                (void)hipGetLastError();
            }
        }
        if (g->copies && !loopback && n_devices > 1) {
            // let every device of the group reach every other one's memory directly (xGMI); where peer access is not
            // available the runtime stages the copies through the host — slower, still correct
            for (int r = 0; r < n_devices; ++r) {
                if (hipSetDevice(devs[r]) != hipSuccess) return bail(fail(LCM_ERR_HIP, "hipSetDevice(%d) failed", devs[r]));
                for (int q = 0; q < n_devices; ++q) {
                    if (q == r) continue;
                    int can = 0;
                    if (hipDeviceCanAccessPeer(&can, devs[r], devs[q]) == hipSuccess && can) {
                        (void)hipDeviceEnablePeerAccess(devs[q], 0);    // "already enabled" is as good
                        (void)hipGetLastError();
                    }
                }
            }
        }
        if (hipSetDevice(devs[0]) != hipSuccess || hipEventCreate(&g->ev0) != hipSuccess ||
            hipEventCreate(&g->ev1) != hipSuccess || hipEventCreate(&g->ev2) != hipSuccess ||
            hipEventCreate(&g->evg0) != hipSuccess || hipEventCreate(&g->evg1) != hipSuccess)
            return bail(fail(LCM_ERR_HIP, "hipEventCreate failed"));
        *out = g;
        return LCM_OK;
    });
}

int lcm_group_create(const lcm_params* params, int n_devices, const int* device_ids, lcm_group** out) {
    return group_create(params, n_devices, device_ids, false, 0, false, out);
}

int lcm_group_create_peer(const lcm_params* params, int n_devices, const int* device_ids, lcm_group** out) {
    return group_create(params, n_devices, device_ids, false, 0, true, out);
}

int lcm_group_create_loopback(const lcm_params* params, int n_shards, int device_id, lcm_group** out) {
    return group_create(params, n_shards, nullptr, true, device_id, false, out);
}

const char* lcm_group_transport(const lcm_group* g) {
    if (!g) return "";
    if (g->loopback) return "loopback (device-local copies)";
    if (!g->copies) return "rccl";
    return g->rccl_error.empty() ? "peer copies (requested)" : "peer copies (ncclCommInitAll failed)";
}

void lcm_group_destroy(lcm_group* g) {
    if (!g) return;
    for (Shard& S : g->shards) S.worker.reset();     // joins the worker threads (none has a job: every call waits for its own)
    for (Shard& S : g->shards) {
        (void)hipSetDevice(S.device);
        (void)hipDeviceSynchronize();
        (void)hipFree(S.buf.qrows); (void)hipFree(S.buf.qcounts); (void)hipFree(S.buf.scores); (void)hipFree(S.buf.isums);
    }
    if (!g->shards.empty()) {
        (void)hipSetDevice(g->shards[0].device);
        (void)hipFree(g->d_gather); (void)hipFree(g->d_merged); (void)hipFree(g->d_meta);
        (void)hipFree(g->d_gather_idx); (void)hipFree(g->d_merged_idx);
        for (hipEvent_t e : {g->ev0, g->ev1, g->ev2, g->evg0, g->evg1}) if (e) (void)hipEventDestroy(e);
    }
    for (Shard& S : g->shards) if (S.comm) (void)ncclCommDestroy(S.comm);
    for (Shard& S : g->shards) lcm_destroy(S.h);
    delete g;
}

int lcm_group_size(const lcm_group* g) { return g ? g->world : 0; }
int lcm_group_db_size(const lcm_group* g) { return g ? (int)g->frames.size() : 0; }

int lcm_group_handle(lcm_group* g, int rank, lcm_handle** out) {
    if (!g || !out || rank < 0 || rank >= g->world) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *out = g->shards[(size_t)rank].h;
    return LCM_OK;
}

int lcm_group_set_params(lcm_group* g, const lcm_params* p) {
    if (!g || !p) return fail(LCM_ERR_INVALID_ARG, "NULL argument");
    for (const Shard& S : g->shards) { const int rc = lcm_set_params(S.h, p); if (rc) return rc; }
    g->params = *p;
    return LCM_OK;
}

int lcm_group_set_tuning(lcm_group* g, int knob, int value) {
    if (!g) return fail(LCM_ERR_INVALID_ARG, "NULL group");
    for (const Shard& S : g->shards) { const int rc = lcm_set_tuning(S.h, knob, value); if (rc) return rc; }
    return LCM_OK;
}

int lcm_group_set_kernel_variant(lcm_group* g, int variant) {
    if (!g) return fail(LCM_ERR_INVALID_ARG, "NULL group");
    for (const Shard& S : g->shards) { const int rc = lcm_set_kernel_variant(S.h, variant); if (rc) return rc; }
    return LCM_OK;
}

int lcm_group_sync(lcm_group* g) {
    if (!g) return fail(LCM_ERR_INVALID_ARG, "NULL group");
    for (const Shard& S : g->shards) { const int rc = lcm_sync(S.h); if (rc) return rc; }
    return LCM_OK;
}

int lcm_group_reserve(lcm_group* g, int n_frames, int max_desc) {
    if (!g || n_frames < 0 || max_desc < 0) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    const int per = (n_frames + g->world - 1) / g->world;
    for (const Shard& S : g->shards) { const int rc = lcm_db_reserve(S.h, per, max_desc); if (rc) return rc; }
    return LCM_OK;
}

int lcm_group_append(lcm_group* g, int frame_id, const uint8_t* desc, int n, int n_keypoints) {
    if (!g || n < 0 || (n > 0 && !desc)) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    return guarded([&]() -> int {
        if (!g->frames.empty() && frame_id <= g->frames.back().id)
            return fail(LCM_ERR_ORDER, "frame id %d appended after id %d: ids must be strictly increasing", frame_id, g->frames.back().id);
        const size_t owner = g->frames.size() % (size_t)g->world;      // cyclic ownership by arrival position
        const int rc = lcm_db_append(g->shards[owner].h, frame_id, desc, n, n_keypoints);
        if (rc) return rc;
        g->frames.push_back({frame_id, n, n_keypoints < 0 ? n : n_keypoints});
        ++g->db_stamp;
        return LCM_OK;
    });
}

int lcm_group_clear(lcm_group* g) {
    if (!g) return fail(LCM_ERR_INVALID_ARG, "NULL group");
    for (const Shard& S : g->shards) { const int rc = lcm_db_clear(S.h); if (rc) return rc; }
    g->frames.clear();
    ++g->db_stamp; ++g->drop_stamp;
    return LCM_OK;
}

/* Drop the most recently appended frames: the group keeps its first n_frames frames (arrival order).  What the host
 * class's rollback needs when a pipelined processFrames fails half-way (host list, loop list and device database must
 * agree); tickets submitted before the call are void, as after lcm_group_clear. */
int lcm_group_truncate(lcm_group* g, int n_frames) {
    if (!g || n_frames < 0) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if ((size_t)n_frames >= g->frames.size()) return LCM_OK;
    const int W = g->world;
    for (int r = 0; r < W; ++r) {
        const int keep = (int)shard_share((uint32_t)n_frames, r, W);          // positions r, r + W, ... below n_frames
        const int rc = lcm_db_truncate(g->shards[(size_t)r].h, keep); if (rc) return rc;
    }
    g->frames.resize((size_t)n_frames);
    ++g->db_stamp; ++g->drop_stamp;
    return LCM_OK;
}

/* Snapshot / resume of a sharded database, in lcm_db_save's OWN file format: frames are written in arrival order (each
 * read back from the shard that owns it), so a file saved by a group of 8 loads into a single handle, a group of any
 * other size, or the other way round.  Load validates the whole header against the file's size before the group's
 * database is touched (lcm::snapshot_open), replaces the contents, and leaves an EMPTY group if a later step fails. */
int lcm_group_save(lcm_group* g, const char* path) {
    if (!g || !path) return fail(LCM_ERR_INVALID_ARG, "NULL argument");
    return guarded([&]() -> int {
        int rc = lcm_group_sync(g); if (rc) return rc;
        FILE* f = fopen(path, "wb");
        if (!f) return fail(LCM_ERR_INVALID_ARG, "cannot open %s for writing", path);
        std::vector<lcm::FrameMeta> metas(g->frames.size());
        for (size_t i = 0; i < metas.size(); ++i) metas[i] = {g->frames[i].id, g->frames[i].n, g->frames[i].n_kp};
        bool ok = lcm::snapshot_write_header(f, metas);
        std::vector<uint8_t> buf;
        const size_t W = (size_t)g->world;
        for (size_t i = 0; ok && !rc && i < metas.size(); ++i) {
            if (metas[i].n == 0) continue;
            buf.resize((size_t)metas[i].n * LCM_DESC_BYTES);
            rc = lcm_db_read(g->shards[i % W].h, (int)(i / W), buf.data(), metas[i].n);
            if (!rc) ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
        }
        ok = (fclose(f) == 0) && ok;
        if (rc) return rc;
        return ok ? LCM_OK : fail(LCM_ERR_HIP, "writing %s failed", path);
    });
}

int lcm_group_load(lcm_group* g, const char* path) {
    if (!g || !path) return fail(LCM_ERR_INVALID_ARG, "NULL argument");
    return guarded([&]() -> int {
        std::vector<lcm::FrameMeta> metas;
        uint32_t max_rows = 0;
        FILE* f = nullptr;
        int rc = lcm::snapshot_open(path, metas, &max_rows, &f); if (rc) return rc;
        struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
        rc = lcm_group_clear(g); if (rc) return rc;
        rc = lcm_group_reserve(g, (int)metas.size(), (int)std::max<uint32_t>(max_rows, 1));
        std::vector<uint8_t> buf((size_t)max_rows * LCM_DESC_BYTES + 1);
        for (size_t i = 0; !rc && i < metas.size(); ++i) {
            if (metas[i].n && fread(buf.data(), LCM_DESC_BYTES, (size_t)metas[i].n, f) != (size_t)metas[i].n) { rc = fail(LCM_ERR_INVALID_ARG, "%s: read error", path); break; }
            rc = lcm_group_append(g, metas[i].id, buf.data(), metas[i].n, metas[i].n_kp);
        }
        if (!rc) rc = lcm_group_sync(g);
        if (rc) {
            const std::string why = lcm::last_error();
            (void)lcm_group_clear(g);
            lcm::last_error() = why;
        }
        return rc;
    });
}

}  // extern "C"

extern "C" {

/* Online totals over the shards (lcm_online_stats_read per shard): the work is summed, kernel_ms is the slowest
 * shard's — the devices run side by side. */
int lcm_group_online_stats_read(lcm_group* g, lcm_online_stats* out, int reset) {
    if (!g || !out) return fail(LCM_ERR_INVALID_ARG, "NULL argument");
    *out = lcm_online_stats{};
    for (const Shard& S : g->shards) {
        lcm_online_stats s{};
        const int rc = lcm_online_stats_read(S.h, &s, reset); if (rc) return rc;
        out->kernel_ms = std::max(out->kernel_ms, s.kernel_ms);
        out->launches += s.launches; out->queries = std::max(out->queries, s.queries);
        out->pairs += s.pairs; out->distances += s.distances; out->algo_bytes += s.algo_bytes;
    }
    return LCM_OK;
}

/* Online query: the frame goes to every device (pinned staging + H2D per device, each from that device's own host
 * thread, all enqueued before any is awaited), each scores it against its shard, and the per-shard records — a few KB —
 * are interleaved on the host: for a message this small a collective would only add latency. */
int lcm_group_query_scores(lcm_group* g, const uint8_t* query, int nq, int query_frame_id,
                           lcm_score* out_scores, int32_t* out_frame_ids, int cap, int* n_out) {
    if (!g || !n_out || nq < 0 || (nq > 0 && !query)) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    return guarded([&]() -> int {
        const int W = g->world;
        const int e = eligible_count(g->frames, query_frame_id, g->params.min_gap);
        if (e > cap) return fail(LCM_ERR_CAPACITY, "%d score records but room for %d", e, cap);
        if (e > 0 && !out_scores) return fail(LCM_ERR_INVALID_ARG, "out_scores is NULL");
        std::vector<int> tickets((size_t)W, -1);
        const int rc_s = run_all(g, [&](int r) { return lcm_query_submit(g->shards[(size_t)r].h, query, nq, query_frame_id, &tickets[(size_t)r]); });
        const std::string why = rc_s ? lcm::last_error() : std::string();
        // collect every ticket that was issued, also after a failed submit (nothing may stay in flight)
        const int rc_c = run_all(g, [&](int r) -> int {
            if (tickets[(size_t)r] < 0) return LCM_OK;
            const int want = (int)shard_share((uint32_t)e, r, W);
            std::vector<lcm_score> part((size_t)std::max(want, 1));
            int n = 0;
            const int rc = lcm_query_collect(g->shards[(size_t)r].h, tickets[(size_t)r], part.data(), nullptr, (int)part.size(), &n);
            if (rc || rc_s) return rc;
            if (n != want) return fail(LCM_ERR_HIP, "returned %d records, expected %d", n, want);
            lcm::interleave_shard(part.data(), (uint32_t)n, r, W, out_scores);
            return LCM_OK;
        });
        if (rc_s) { lcm::last_error() = why; return rc_s; }
        if (rc_c) return rc_c;
        if (out_frame_ids) for (int s = 0; s < e; ++s) out_frame_ids[s] = g->frames[(size_t)s].id;
        *n_out = e;
        return LCM_OK;
    });
}

/* Asynchronous micro-batched online queries over all shards (BASELINE.json configs[4] inside one process): the batch goes
 * to every device with ONE lcm_query_submit_batch each, issued from the devices' own host threads; the call returns as
 * soon as every device has its work ENQUEUED (the callers' buffers are free then), with one group ticket.  Up to 4 may
 * be in flight; lcm_group_query_collect_batch waits for one, and each device's thread writes its records straight into
 * their interleaved places of the single-device order (query 0's records first, offsets[n_queries + 1]). */
int lcm_group_query_submit_batch(lcm_group* g, const uint8_t* const* queries, const int* nq, const int* query_frame_ids, int n_queries, int* ticket) {
    if (!g || !ticket || !queries || !nq || !query_frame_ids) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *ticket = -1;
    if (n_queries < 1 || n_queries > lcm::MAX_QUERY_BATCH) return fail(LCM_ERR_INVALID_ARG, "a batch holds 1..%d queries", lcm::MAX_QUERY_BATCH);
    return guarded([&]() -> int {
        const int W = g->world;
        int t = -1;
        for (int i = 0; i < lcm::QUERY_SLOTS; ++i) if (!g->tickets[i].busy) { t = i; break; }
        if (t < 0) return fail(LCM_ERR_CAPACITY, "%d group queries already in flight: collect one first", lcm::QUERY_SLOTS);
        GTicket& T = g->tickets[t];
        T.n_queries = n_queries; T.total = 0; T.stamp = g->drop_stamp;
        for (int b = 0; b < n_queries; ++b) { T.e[b] = eligible_count(g->frames, query_frame_ids[b], g->params.min_gap); T.total += (size_t)T.e[b]; }
        T.shard_ticket.assign((size_t)W, -1);
        T.part.resize((size_t)W);
        const int rc = run_all(g, [&](int r) { return lcm_query_submit_batch(g->shards[(size_t)r].h, queries, nq, query_frame_ids, n_queries, &T.shard_ticket[(size_t)r]); });
        if (rc) {
            // some shards may hold a ticket: drain them, keep the first error
            const std::string why = lcm::last_error();
            (void)run_all(g, [&](int r) -> int {
                if (T.shard_ticket[(size_t)r] < 0) return LCM_OK;
                std::vector<lcm_score> sink(std::max<size_t>(T.total, 1));
                size_t n = 0;
                (void)lcm_query_collect_batch(g->shards[(size_t)r].h, T.shard_ticket[(size_t)r], sink.data(), sink.size(), &n, nullptr);
                return LCM_OK;
            });
            lcm::last_error() = why;
            return rc;
        }
        T.busy = true;
        *ticket = t;
        return LCM_OK;
    });
}

int lcm_group_query_collect_batch(lcm_group* g, int ticket, lcm_score* out_scores, size_t cap, size_t* n_out, size_t* offsets) {
    if (!g || !n_out || ticket < 0 || ticket >= lcm::QUERY_SLOTS || !g->tickets[ticket].busy) return fail(LCM_ERR_INVALID_ARG, "bad group ticket");
    *n_out = 0;
    return guarded([&]() -> int {
        const int W = g->world;
        GTicket& T = g->tickets[ticket];
        const int B = T.n_queries;
        std::vector<size_t> offs((size_t)B + 1, 0);
        for (int b = 0; b < B; ++b) offs[(size_t)b + 1] = offs[(size_t)b] + (size_t)T.e[b];
        if (T.stamp == g->drop_stamp) {
            // recoverable argument errors keep the ticket (as lcm_query_collect_batch does)
            if (T.total > cap) return fail(LCM_ERR_CAPACITY, "%zu score records but room for %zu (the ticket stays valid)", T.total, cap);
            if (T.total > 0 && !out_scores) return fail(LCM_ERR_INVALID_ARG, "out_scores is NULL (the ticket stays valid)");
        }
        const bool is_void = T.stamp != g->drop_stamp;      // frames were dropped after the submit: the shards refuse their tickets too
        const int rc = run_all(g, [&](int r) -> int {
            std::vector<lcm_score>& part = T.part[(size_t)r];
            size_t want_total = 0;
            for (int b = 0; b < B; ++b) want_total += shard_share((uint32_t)T.e[b], r, W);
            if (part.size() < std::max<size_t>(want_total, 1)) part.resize(std::max<size_t>(want_total, 1));
            std::vector<size_t> poffs((size_t)B + 1, 0);
            size_t n = 0;
            const int rc2 = lcm_query_collect_batch(g->shards[(size_t)r].h, T.shard_ticket[(size_t)r], part.data(), part.size(), &n, poffs.data());
            if (is_void) return LCM_OK;                     // drained; the group reports the void ticket itself
            if (rc2) return rc2;
            for (int b = 0; b < B; ++b) {
                const int want = (int)shard_share((uint32_t)T.e[b], r, W);
                if ((int)(poffs[(size_t)b + 1] - poffs[(size_t)b]) != want) return fail(LCM_ERR_HIP, "returned a wrong record count for query %d", b);
                // disjoint places per shard: no two threads share a record
                lcm::interleave_shard(part.data() + poffs[(size_t)b], (uint32_t)want, r, W, out_scores + offs[(size_t)b]);
            }
            return LCM_OK;
        });
        T.busy = false;
        if (is_void) return fail(LCM_ERR_NOT_FOUND, "group ticket %d was submitted before lcm_group_clear / lcm_group_truncate: its result is void", ticket);
        if (rc) return rc;
        if (offsets) memcpy(offsets, offs.data(), sizeof(size_t) * offs.size());
        *n_out = T.total;
        return LCM_OK;
    });
}

/* The synchronous form: submit + collect. */
int lcm_group_query_scores_batch(lcm_group* g, const uint8_t* const* queries, const int* nq, const int* query_frame_ids, int n_queries,
                                 lcm_score* out_scores, size_t cap, size_t* n_out, size_t* offsets) {
    if (!g || !n_out || !queries || !nq || !query_frame_ids || n_queries < 1) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    return guarded([&]() -> int {
        size_t total = 0;
        for (int b = 0; b < n_queries && b < lcm::MAX_QUERY_BATCH; ++b) {
            if (offsets) offsets[b] = total;
            total += (size_t)eligible_count(g->frames, query_frame_ids[b], g->params.min_gap);
        }
        if (offsets && n_queries <= lcm::MAX_QUERY_BATCH) offsets[n_queries] = total;
        if (total > cap) return fail(LCM_ERR_CAPACITY, "%zu score records but room for %zu", total, cap);
        if (total > 0 && !out_scores) return fail(LCM_ERR_INVALID_ARG, "out_scores is NULL");
        int t = -1;
        int rc = lcm_group_query_submit_batch(g, queries, nq, query_frame_ids, n_queries, &t); if (rc) return rc;
        return lcm_group_query_collect_batch(g, t, out_scores, cap, n_out, offsets);
    });
}

int lcm_group_detect_loops(lcm_group* g, int current_frame_id, const uint8_t* query, int nq, int n_keypoints,
                           lcm_loop_candidate* out, int cap, int* n_out) {
    if (!g || !n_out || cap < 0) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    return guarded([&]() -> int {
        const int e = eligible_count(g->frames, current_frame_id, g->params.min_gap);
        std::vector<lcm_score> sc((size_t)std::max(e, 1));
        int n = 0;
        const int rc = lcm_group_query_scores(g, query, nq, current_frame_id, sc.data(), nullptr, (int)sc.size(), &n);
        if (rc) return rc;
        const int q_kp = n_keypoints < 0 ? nq : n_keypoints;
        int k = 0, total = 0;
        for (int s = 0; s < n; ++s) {
            double sim;
            if (lcm_loop_test(&g->params, &sc[(size_t)s], q_kp, g->frames[(size_t)s].n_kp, &sim)) {
                if (k < cap && out) {
                    out[k].current_frame_id = current_frame_id;
                    out[k].matched_frame_id = g->frames[(size_t)s].id;
                    out[k].num_matches = (int32_t)sc[(size_t)s].good_count;
                    out[k].similarity_score = sim;
                    ++k;
                }
                ++total;
            }
        }
        *n_out = k;
        if (total > k) return fail(LCM_ERR_CAPACITY, "%d loop candidates but room for %d", total, cap);
        return LCM_OK;
    });
}

}  // extern "C"
