// The group's sharding arithmetic (csrc/lcm_group_host.h) as a stand-alone program: tests/test_group_host.py builds it
// with -fsanitize=address,undefined and runs it on the CPU.  No HIP runtime, no device.  Exit status 0 = every check held.
//
// What is expected comes from brute force, not from the header's formulas: every (query position c, stored position s)
// with id[c] - id[s] >= max(gap, 1) is enumerated; s belongs to shard s % W; a shard keeps (c ascending, s ascending).
#include <cstdio>
#include <cstring>
#include <vector>

#include "lcm_group_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

using lcm::GFrame;

static lcm_score rec(int c, int s) { return lcm_score{(uint32_t)c * 65536u + (uint32_t)s, (uint16_t)(s % 65521), (uint16_t)(c % 65521)}; }
static bool same(const lcm_score& a, const lcm_score& b) { return a.good_count == b.good_count && a.min_dist == b.min_dist && a.n_train == b.n_train; }
static bool same(const lcm_loop_candidate& a, const lcm_loop_candidate& b) {
    return a.current_frame_id == b.current_frame_id && a.matched_frame_id == b.matched_frame_id && a.num_matches == b.num_matches &&
           a.similarity_score == b.similarity_score;
}
template <typename T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) if (!same(a[i], b[i])) return false;
    return true;
}

static bool some_shard_owned_nothing = false;

template <typename Off>
static void check_layout(const std::vector<GFrame>& f, int W, int gap, const std::vector<std::vector<lcm_score>>& per_query,
                         const std::vector<std::vector<lcm_score>>& shard, const std::vector<std::vector<size_t>>& shard_per_query,
                         const std::vector<lcm_score>& full) {
    const int N = (int)f.size();
    lcm::ShardLayout<Off> L;
    CHECK(lcm::shard_layout(f, W, gap, L) == nullptr);
    CHECK(L.W == W && L.N == N && L.total == full.size());
    CHECK(L.offs.size() == (size_t)N + 1 && L.offr.size() == (size_t)W && L.shard_base.size() == (size_t)W + 1);
    size_t at = 0;
    for (int c = 0; c < N; ++c) { CHECK((size_t)L.offs[(size_t)c] == at); at += per_query[(size_t)c].size(); }
    CHECK((size_t)L.offs[(size_t)N] == at);
    size_t base = 0;
    for (int r = 0; r < W; ++r) {
        CHECK(L.offr[(size_t)r].size() == (size_t)N + 1);
        size_t a = 0;
        for (int c = 0; c < N; ++c) { CHECK((size_t)L.offr[(size_t)r][(size_t)c] == a); a += shard_per_query[(size_t)r][(size_t)c]; }
        CHECK((size_t)L.shard_total(r) == a && a == shard[(size_t)r].size());
        CHECK((size_t)L.shard_base[(size_t)r] == base);
        base += shard[(size_t)r].size();
    }
    CHECK((size_t)L.shard_base[(size_t)W] == base && base == full.size());
    // the host merge: W shard arrays -> the enumeration's own order
    std::vector<const lcm_score*> ptrs;
    for (int r = 0; r < W; ++r) ptrs.push_back(shard[(size_t)r].data());
    std::vector<lcm_score> out(full.size() + 1, lcm_score{0xDEADu, 1, 2});
    lcm::merge_shards_host(L, ptrs.data(), out.data());
    CHECK(out.back().good_count == 0xDEADu);
    out.pop_back();
    CHECK(same(out, full));
}

static void check_shape(int W, int N, int gap, int step) {
    std::vector<GFrame> f;
    for (int i = 0; i < N; ++i) f.push_back(GFrame{10 + i * step, 1 + (i * 37) % 61, i});
    const int g = gap > 1 ? gap : 1;
    // ---- the enumeration
    std::vector<std::vector<lcm_score>> per_query((size_t)N), shard((size_t)W);
    std::vector<std::vector<size_t>> shard_per_query((size_t)W, std::vector<size_t>((size_t)N, 0));
    std::vector<lcm_score> full;
    for (int c = 0; c < N; ++c)
        for (int s = 0; s < N; ++s)
            if (f[(size_t)c].id - f[(size_t)s].id >= g) {
                per_query[(size_t)c].push_back(rec(c, s));
                full.push_back(rec(c, s));
                shard[(size_t)(s % W)].push_back(rec(c, s));
                ++shard_per_query[(size_t)(s % W)][(size_t)c];
            }
    if (!full.empty()) for (int r = 0; r < W; ++r) if (shard[(size_t)r].empty()) some_shard_owned_nothing = true;
    // ---- eligible_count and shard_share per stored query
    for (int c = 0; c < N; ++c) {
        CHECK((size_t)lcm::eligible_count(f, f[(size_t)c].id, gap) == per_query[(size_t)c].size());
        for (int r = 0; r < W; ++r) CHECK(lcm::shard_share((uint32_t)per_query[(size_t)c].size(), r, W) == shard_per_query[(size_t)r][(size_t)c]);
    }
    check_layout<uint32_t>(f, W, gap, per_query, shard, shard_per_query, full);
    check_layout<size_t>(f, W, gap, per_query, shard, shard_per_query, full);
    // ---- geometry and q_frame_of: shard r's k-th frame (position r + k W) sits in slot k of arena r; the arenas lie rank-major
    int owned_max = 0, widest = 4;
    std::vector<int> owned((size_t)W, 0);
    for (int p = 0; p < N; ++p) { if (++owned[(size_t)(p % W)] > owned_max) owned_max = owned[(size_t)(p % W)]; }
    for (const GFrame& fr : f) { int rows = fr.n; while (rows % 4) ++rows; if (rows > widest) widest = rows; }
    std::vector<int> strides((size_t)W, 4);
    lcm::ShardGeometry geo = lcm::shard_geometry(f, W, strides.data());
    CHECK(geo.shard_cap == owned_max && geo.stride == widest);
    CHECK(geo.shard_bytes() == (size_t)owned_max * (size_t)widest * 32);
    strides[(size_t)(W - 1)] = widest + 8;                 // an arena never shrinks: a handle's wider stride wins
    CHECK(lcm::shard_geometry(f, W, strides.data()).stride == widest + 8);
    std::vector<int> buffer((size_t)W * (size_t)geo.shard_cap, -1), next((size_t)W, 0);
    for (int p = 0; p < N; ++p) { const int r = p % W; buffer[(size_t)r * (size_t)geo.shard_cap + (size_t)next[(size_t)r]++] = p; }
    for (int p = 0; p < N; ++p) {
        const uint32_t slot = lcm::q_frame_of(p, W, geo.shard_cap);
        CHECK(slot < buffer.size() && buffer[slot] == p);
    }
    // ---- the online interleave: a query frame's records arrive per shard and go to their places among its e records
    for (const int qid : {f.empty() ? 0 : f[0].id, f.empty() ? 5 : f[(size_t)N / 2].id + 1, f.empty() ? 9 : f.back().id + 2 * g + 1}) {
        std::vector<lcm_score> want;
        std::vector<std::vector<lcm_score>> part((size_t)W);
        for (int s = 0; s < N; ++s)
            if ((long long)qid - f[(size_t)s].id >= g) { want.push_back(rec(7, s)); part[(size_t)(s % W)].push_back(rec(7, s)); }
        CHECK((size_t)lcm::eligible_count(f, qid, gap) == want.size());
        std::vector<lcm_score> dst(want.size() + 1, lcm_score{0xDEADu, 1, 2});
        for (int r = 0; r < W; ++r) {
            CHECK(lcm::shard_share((uint32_t)want.size(), r, W) == part[(size_t)r].size());
            lcm::interleave_shard(part[(size_t)r].data(), (uint32_t)part[(size_t)r].size(), r, W, dst.data());
        }
        CHECK(dst.back().good_count == 0xDEADu);
        dst.pop_back();
        CHECK(same(dst, want));
    }
    // ---- the candidate merge: some pairs are loops; every shard lists its own in its own order
    std::vector<lcm_loop_candidate> all;
    std::vector<std::vector<lcm_loop_candidate>> lists((size_t)W);
    for (int c = 0; c < N; ++c)
        for (int s = 0; s < N; ++s)
            if (f[(size_t)c].id - f[(size_t)s].id >= g && (c * 7 + s * 3) % 4 != 0) {
                const lcm_loop_candidate cand{f[(size_t)c].id, f[(size_t)s].id, c + s, 0.5 + s};
                all.push_back(cand);
                lists[(size_t)(s % W)].push_back(cand);
            }
    std::vector<lcm_loop_candidate> merged(all.size() + 1, lcm_loop_candidate{-1, -1, -1, -1.0});
    lcm::merge_candidates(lists, merged.data());
    CHECK(merged.back().current_frame_id == -1);
    merged.pop_back();
    CHECK(same(merged, all));
    // one list holding everything, at every place among empty ones
    for (int at = 0; at < W; ++at) {
        std::vector<std::vector<lcm_loop_candidate>> one((size_t)W);
        one[(size_t)at] = all;
        std::vector<lcm_loop_candidate> got(all.size());
        lcm::merge_candidates(one, got.data());
        CHECK(same(got, all));
    }
}

// the refusal at 2^32 pairs: unit id steps and gap <= 1 give c pairs for query position c
static void check_limit() {
    const char* const REFUSAL = "more than 2^32 pairs in one call";
    for (const int N : {92682, 92683}) {
        std::vector<GFrame> f;
        uint64_t pairs = 0;
        for (int i = 0; i < N; ++i) { f.push_back(GFrame{i, 0, 0}); pairs += (uint64_t)i; }
        lcm::ShardLayout<uint32_t> L;
        lcm::ShardLayout<size_t> L64;
        const char* what = lcm::shard_layout(f, 3, 1, L);
        CHECK(lcm::shard_layout(f, 3, 0, L64) == nullptr && L64.total == pairs && (uint64_t)L64.offs.back() == pairs);
        if (N == 92682) {
            CHECK(pairs == 4294930221ull && pairs <= 0xFFFFFFFFull);
            CHECK(what == nullptr && L.total == pairs && L.offs.back() == (uint32_t)pairs);
            CHECK((uint64_t)L.shard_base[3] == pairs);
        } else {
            CHECK(pairs == 4295022903ull && pairs > 0xFFFFFFFFull);
            CHECK(what != nullptr && std::strcmp(what, REFUSAL) == 0);
        }
    }
}

int main() {
    for (const int W : {1, 2, 3, 5, 8})
        for (const int N : {0, 1, W - 1, W, W + 1, 57})
            for (const int gap : {0, 1, 3, 30})
                for (const int step : {1, 3}) check_shape(W, N, gap, step);
    CHECK(some_shard_owned_nothing);
    // shard_share on its own: the positions [0, e) that are r mod W, counted
    for (const int W : {1, 2, 3, 5, 8})
        for (uint32_t e = 0; e <= 3u * (uint32_t)W + 2; ++e)
            for (int r = 0; r < W; ++r) {
                uint32_t n = 0;
                for (uint32_t s = 0; s < e; ++s) n += (int)(s % (uint32_t)W) == r;
                CHECK(lcm::shard_share(e, r, W) == n);
            }
    // the candidate merge with nothing at all
    std::vector<std::vector<lcm_loop_candidate>> none(3);
    lcm_loop_candidate untouched{-1, -1, -1, -1.0};
    lcm::merge_candidates(none, &untouched);
    CHECK(untouched.current_frame_id == -1);
    check_limit();
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all held\n");
    return 0;
}
