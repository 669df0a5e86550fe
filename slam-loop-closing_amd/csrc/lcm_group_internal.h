// lcm_group_internal.h — what lcm_group.cpp (create / destroy, database, snapshot, online queries) and
// lcm_group_search.cpp (the bulk search) share: the group itself, its per-shard state, the worker threads, the device merge.
// The sharding arithmetic is lcm_group_host.h's.
#pragma once
#include <rccl/rccl.h>

#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>

#include "lcm_group_host.h"
#include "lcm_internal.h"

#define NCCL_TRY(expr)                                                                                       \
    do {                                                                                                     \
        ncclResult_t r_ = (expr);                                                                            \
        if (r_ != ncclSuccess)                                                                               \
            return fail(LCM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

namespace lcm {

constexpr int MAX_WORLD = 8;

// One persistent host thread per device beyond the first (the caller's thread serves device 0): per-shard planning,
// launches, online submits / collects and downloads run on all devices at once, without a thread being created per call.
struct Worker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false, done = true, stop = false;
    Worker() {
        th = std::thread([this] {
            std::unique_lock<std::mutex> lk(mu);
            for (;;) {
                cv.wait(lk, [this] { return has_job || stop; });
                if (stop) return;
                std::function<void()> j = std::move(job);
                has_job = false;
                lk.unlock();
                j();
                lk.lock();
                done = true;
                cv.notify_all();
            }
        });
    }
    void post(std::function<void()> j) {
        std::lock_guard<std::mutex> lk(mu);
        job = std::move(j); has_job = true; done = false;
        cv.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [this] { return done; });
    }
    ~Worker() {
        { std::lock_guard<std::mutex> lk(mu); stop = true; cv.notify_all(); }
        if (th.joinable()) th.join();
    }
};

// One asynchronous group query (lcm_group_query_submit_batch): a ticket per shard + what the interleave needs.
struct GTicket {
    bool busy = false;
    int n_queries = 0;
    int e[lcm::MAX_QUERY_BATCH] = {0};          // eligible stored frames per query, over ALL shards, at submit time
    size_t total = 0;
    uint64_t stamp = 0;                         // group's drop_stamp at submit: a clear / truncate in between voids the ticket
    std::vector<int> shard_ticket;
    std::vector<std::vector<lcm_score>> part;   // per shard: landing zone of its records
};

// A shard's buffers on its own device: the rank-major gathered query rows / counts, its score records (+ index checksums)
struct ShardBufs {
    uint8_t* qrows = nullptr;   size_t qrows_bytes = 0;
    int32_t* qcounts = nullptr; size_t qcounts_n = 0;
    lcm_score* scores = nullptr; size_t scores_n = 0;
    uint32_t* isums = nullptr;  size_t isums_n = 0;
};

// One shard: a matcher on its device.  group_create makes each one whole (handle, device, worker) or bails.
struct Shard {
    lcm_handle* h = nullptr;
    int device = 0;
    ncclComm_t comm = nullptr;                  // RCCL transport only
    std::unique_ptr<Worker> worker;             // shards beyond the first: the caller's thread serves shard 0
    ShardBufs buf;
};

}  // namespace lcm

struct lcm_group {
    int world = 0;
    // Rehearsal form (lcm_group_create_loopback): the W shards are W matchers on ONE device and the two exchange steps
    // are device-local copies instead of RCCL calls — every index computation of the multi-device path (cyclic
    // ownership, rank-major query buffer, gatherv offsets, merge) runs for W > 1 on a box with a single GPU.
    bool loopback = false;
    // Exchange steps as device-to-device copies (hipMemcpyAsync between the devices' arenas: xGMI peer copies) instead of
    // RCCL calls: always in the loopback form; in a real group when the caller asked for it (lcm_group_create_peer) or
    // when the RCCL communicator could not be created (the reason is kept in rccl_error).
    bool copies = false;
    std::string rccl_error;
    lcm_params params{};
    std::vector<lcm::Shard> shards;             // world of them once created
    std::vector<lcm::GFrame> frames;            // every frame of every shard, arrival order == ascending id
    // The gathered query buffers stay valid until the database changes: db_stamp is bumped by every append / clear /
    // truncate, gathered_stamp is the value it had when the arenas were last all-gathered (with that geometry).
    uint64_t db_stamp = 1, gathered_stamp = 0, drop_stamp = 1;
    int gathered_cap = 0, gathered_stride = 0;
    // device 0: gathered shards, merged result, merge metadata
    lcm_score* d_gather = nullptr; size_t d_gather_n = 0;
    lcm_score* d_merged = nullptr; size_t d_merged_n = 0;
    uint32_t* d_gather_idx = nullptr; size_t d_gather_idx_n = 0;
    uint32_t* d_merged_idx = nullptr; size_t d_merged_idx_n = 0;
    uint32_t* d_meta = nullptr;    size_t d_meta_n = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;   // device 0: search done / gather+merge done / download done
    hipEvent_t evg0 = nullptr, evg1 = nullptr;                // device 0: around the all-gather of the shard arenas
    lcm::GTicket tickets[lcm::QUERY_SLOTS];
    lcm_group_info info{};
};

namespace {
using lcm::GFrame;
using lcm::MAX_WORLD;
using lcm::Shard;

inline int set_dev(const lcm_group* g, int r) {
    HIP_TRY(hipSetDevice(g->shards[(size_t)r].device));
    return LCM_OK;
}

// Run fn(r) for every shard at once — shard 0 on the calling thread, shard r > 0 on its worker — and wait for all.
// Returns the first failure, its message prefixed with the shard (a worker's lcm_last_error is thread-local).
template <typename F>
int run_all(lcm_group* g, F&& fn) {
    const int W = g->world;
    std::vector<int> rcs((size_t)W, LCM_OK);
    std::vector<std::string> errs((size_t)W);
    auto job = [&](int r) {
        int rc;
        try { rc = fn(r); }
        catch (const std::bad_alloc&) { rc = fail(LCM_ERR_OOM, "host allocation failed (std::bad_alloc)"); }
        catch (const std::exception& e) { rc = fail(LCM_ERR_HIP, "unexpected C++ exception: %s", e.what()); }
        catch (...) { rc = fail(LCM_ERR_HIP, "unexpected C++ exception"); }
        rcs[(size_t)r] = rc;
        if (rc) errs[(size_t)r] = lcm::last_error();
    };
    for (int r = 1; r < W; ++r) g->shards[(size_t)r].worker->post([&job, r] { job(r); });
    job(0);
    for (int r = 1; r < W; ++r) g->shards[(size_t)r].worker->wait();
    for (int r = 0; r < W; ++r)
        if (rcs[(size_t)r]) return W > 1 ? fail(rcs[(size_t)r], "shard %d: %s", r, errs[(size_t)r].c_str()) : rcs[(size_t)r];
    return LCM_OK;
}

// Enqueue, on `st` (current device), the un-permutation of W back-to-back shard arrays at d_gathered into d_merged.
// upload_merge_meta first: d_meta (device scratch of at least (W + 1) * (N + 1) words) receives the W per-shard offset
// arrays and the merged offsets; then merge_on_device per array (elements of elem_words dwords: 2 = score records,
// 1 = index checksums).
inline int upload_merge_meta(uint32_t* d_meta, const lcm::ShardLayout<uint32_t>& L, hipStream_t st) {
    const size_t W = (size_t)L.W, N1 = L.offs.size();
    for (size_t r = 0; r < W; ++r)
        HIP_TRY(hipMemcpyAsync(d_meta + r * N1, L.offr[r].data(), sizeof(uint32_t) * N1, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_meta + W * N1, L.offs.data(), sizeof(uint32_t) * N1, hipMemcpyHostToDevice, st));
    // the offset vectors are pageable host memory: the copies above have consumed them when the calls return
    return LCM_OK;
}

inline int merge_on_device(const void* d_gathered, void* d_merged, const uint32_t* d_meta, const lcm::ShardLayout<uint32_t>& L,
                           uint32_t elem_words, hipStream_t st) {
    const size_t W = (size_t)L.W, N1 = L.offs.size();
    lcm::MergeArgs m{};
    m.world = (uint32_t)W; m.n_q = (uint32_t)L.N; m.n_total = L.offs.back(); m.elem_words = elem_words;
    for (size_t r = 0; r <= W; ++r) m.shard_base[r] = L.shard_base[r];
    m.gathered = d_gathered; m.merged = d_merged;
    m.shard_offsets = d_meta; m.offsets = d_meta + W * N1;
    const hipError_t e = lcm::launch_merge_shards(m, st);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "merge kernel launch failed: %s", hipGetErrorString(e));
    return LCM_OK;
}

}  // namespace
