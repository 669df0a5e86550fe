// lcm_group_host.h — the group's cyclic-sharding arithmetic (lcm_group.cpp, lcm_group_search.cpp), each rule once: which
// stored frames a query may meet, a shard's share of them, the record layout of a search, the shard geometry, where a frame
// sits in the rank-major query buffer, and the three host merges.  No HIP call, no communicator and no handle:
// tests/cpp/group_host_check.cpp compiles this text into a stand-alone program that runs under a sanitizer.  A check returns
// NULL or what is wrong.
//
// Stored frame with arrival position s belongs to shard s mod W; a shard keeps its records in (query ascending, owned stored
// ascending) order; the single-device order is (query ascending, stored ascending).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/lcm.h"

namespace lcm {

struct GFrame { int32_t id, n, n_kp; };     // one stored frame of a group: id, rows, keypoints

// eligible stored positions for a query id over ascending ids: positions [0, e) with query_id - id[s] >= max(gap, 1)
inline int eligible_count(const std::vector<GFrame>& f, int query_id, int gap) {
    const long long lim = (long long)query_id - std::max(gap, 1);
    int lo = 0, hi = (int)f.size();
    while (lo < hi) { const int mid = (lo + hi) / 2; if ((long long)f[(size_t)mid].id <= lim) lo = mid + 1; else hi = mid; }
    return lo;
}

// how many of the positions [0, e) shard r of W owns: r, r + W, ...
inline uint32_t shard_share(uint32_t e, int r, int W) {
    return e > (uint32_t)r ? (e - (uint32_t)r + (uint32_t)W - 1) / (uint32_t)W : 0u;
}

// Record offsets of one all-vs-all search over W cyclic shards.  Off is uint32_t where the offsets go to the device (the
// merge kernel's and the loop test's tables: a call holds at most 2^32 - 1 pairs) and size_t behind lcm_merge_shard_scores,
// whose ABI has size_t offsets and which refuses no pair count.
template <typename Off>
struct ShardLayout {
    int W = 0, N = 0;
    std::vector<Off> offs;                     // N + 1: query c's records are [offs[c], offs[c + 1]) of the merged array
    std::vector<std::vector<Off>> offr;        // per shard, N + 1: the same inside shard r's own array
    std::vector<Off> shard_base;               // W + 1: where shard r's array starts when the W arrays lie back to back
    uint64_t total = 0;
    Off shard_total(int r) const { return offr[(size_t)r].back(); }
};

template <typename Off>
inline const char* shard_layout(const std::vector<GFrame>& frames, int W, int gap, ShardLayout<Off>& L) {
    const int N = (int)frames.size();
    L.W = W; L.N = N; L.total = 0;
    L.offs.assign((size_t)N + 1, 0);
    L.offr.assign((size_t)W, std::vector<Off>((size_t)N + 1, 0));
    L.shard_base.assign((size_t)W + 1, 0);
    for (int c = 0; c < N; ++c) {
        const uint32_t e = (uint32_t)eligible_count(frames, frames[(size_t)c].id, gap);
        L.total += e;
        if (L.total > (uint64_t)std::numeric_limits<Off>::max()) return "more than 2^32 pairs in one call";
        L.offs[(size_t)c + 1] = (Off)L.total;
        for (int r = 0; r < W; ++r) L.offr[(size_t)r][(size_t)c + 1] = L.offr[(size_t)r][(size_t)c] + (Off)shard_share(e, r, W);
    }
    for (int r = 0; r < W; ++r) L.shard_base[(size_t)r + 1] = L.shard_base[(size_t)r] + L.shard_total(r);
    return nullptr;
}

// Equal arena geometry for every shard: slots per shard, and the padded rows of a slot — the widest frame, no less than any
// handle's current stride (an arena never shrinks).
struct ShardGeometry {
    int shard_cap = 0, stride = 4;
    size_t shard_bytes() const { return (size_t)shard_cap * (size_t)stride * LCM_DESC_BYTES; }
};

inline ShardGeometry shard_geometry(const std::vector<GFrame>& frames, int W, const int* handle_strides) {
    ShardGeometry geo;
    geo.shard_cap = ((int)frames.size() + W - 1) / W;
    for (int r = 0; r < W; ++r) geo.stride = std::max(geo.stride, handle_strides[r]);
    for (const GFrame& f : frames) geo.stride = std::max(geo.stride, (f.n + 3) / 4 * 4);
    return geo;
}

// slot of stored position p in a rank-major buffer of W shard arenas of shard_cap slots each
inline uint32_t q_frame_of(int p, int W, int shard_cap) { return (uint32_t)((p % W) * shard_cap + p / W); }

// W shard arrays -> the single-device order (what k_merge_shards does on the device)
template <typename T, typename Off>
inline void merge_shards_host(const ShardLayout<Off>& L, const T* const* shard, T* out) {
    for (int c = 0; c < L.N; ++c) {
        const size_t e = (size_t)(L.offs[(size_t)c + 1] - L.offs[(size_t)c]);
        for (size_t s = 0; s < e; ++s) {
            const size_t r = s % (size_t)L.W;
            out[(size_t)L.offs[(size_t)c] + s] = shard[r][(size_t)L.offr[r][(size_t)c] + s / (size_t)L.W];
        }
    }
}

// One query's records of shard r (its share of the e eligible frames, ascending) to their places among the query's e
// records in the single-device order.  Shards write disjoint places.
inline void interleave_shard(const lcm_score* src, uint32_t share, int r, int W, lcm_score* query_dst) {
    for (uint32_t k = 0; k < share; ++k) query_dst[(size_t)r + (size_t)k * (size_t)W] = src[k];
}

// W candidate lists, each sorted by (current id, matched id) -> one such list.  For a given current frame the shards'
// candidates interleave by stored position, so this is a W-way merge; out holds the lists' sizes summed.
inline void merge_candidates(const std::vector<std::vector<lcm_loop_candidate>>& lists, lcm_loop_candidate* out) {
    std::vector<size_t> at(lists.size(), 0);
    for (size_t k = 0;; ++k) {
        int best = -1;
        for (int r = 0; r < (int)lists.size(); ++r) {
            if (at[(size_t)r] >= lists[(size_t)r].size()) continue;
            const lcm_loop_candidate& c = lists[(size_t)r][at[(size_t)r]];
            if (best < 0) { best = r; continue; }
            const lcm_loop_candidate& b = lists[(size_t)best][at[(size_t)best]];
            if (c.current_frame_id < b.current_frame_id || (c.current_frame_id == b.current_frame_id && c.matched_frame_id < b.matched_frame_id)) best = r;
        }
        if (best < 0) return;
        out[k] = lists[(size_t)best][at[(size_t)best]++];
    }
}

}  // namespace lcm
