// The pure host side of the SIFT matcher (csrc/lcm_l2_host.h: the tile space, the chunk rule, the plans of a list run, a count
// run and a loop search, the walk over a search's records) as a stand-alone program: tests/test_l2_plan_host.py builds it with
// -fsanitize=address,undefined and runs it on the CPU.  No HIP runtime is linked and no device is touched (lcm_kernels.h needs
// HIP's headers for its types only).  Every plan is flattened into one list of numbers and compared whole with a literal; the
// literals were printed once by the loops these planners were cut out of and checked by hand against the field meanings in
// lcm_kernels.h.  Exit status 0 = every check held.
#include <cstdio>
#include <cstring>

#include "lcm_l2_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

typedef std::vector<uint64_t> Dump;
using lcm::L2Pair;

// [chunk rows, items, blocks, longest query, distances, tiles | tile0 | tile words | items | jobs | row0]
static Dump run_dump(const int* rows, int n_frames, const std::vector<L2Pair>& pairs, bool tables = true) {
    std::vector<uint32_t> tile0, tile_meta;
    lcm::l2_tile_space(rows, n_frames, tile0, tile_meta);          // a list run lays out every matrix
    lcm::L2RunPlan pl;
    CHECK(lcm::l2_run_plan(pairs, rows, tile0.data(), pl) == nullptr);
    CHECK(pl.jobs.size() == pairs.size() && pl.row0.size() == pairs.size() + 1);
    Dump d{(uint64_t)pl.chunk_rows, pl.items.size(), pl.n_blocks, (uint64_t)pl.max_nq, pl.distances, tile_meta.size()};
    if (!tables) return d;
    for (uint32_t v : tile0) d.push_back(v);
    for (uint32_t v : tile_meta) d.push_back(v);
    for (const lcm::L2Item& i : pl.items) for (uint32_t v : {i.q_tile, i.q_rows, i.t_tile, i.t_rows}) d.push_back(v);
    for (const lcm::L2Job& j : pl.jobs) for (uint32_t v : {j.q_tile, j.nq, j.t_tile, j.nt, j.first_item, j.n_seg, j.out_row0, j.reserved}) d.push_back(v);
    for (size_t v : pl.row0) d.push_back(v);
    return d;
}

// [chunk rows, items, distances, tiles | tile0 | tile words | items]
static Dump count_dump(const int* rows, int n_frames, const std::vector<L2Pair>& live, bool tables = true) {
    std::vector<int> used((size_t)n_frames, 0);                                 // a count run: only what a live pair names
    for (const L2Pair& p : live) { used[(size_t)p.q] = rows[p.q]; used[(size_t)p.t] = rows[p.t]; }
    std::vector<uint32_t> tile0, tile_meta;
    lcm::l2_tile_space(used.data(), n_frames, tile0, tile_meta);
    lcm::L2CountPlan pl;
    CHECK(lcm::l2_count_plan(live, rows, tile0.data(), pl) == nullptr);
    Dump d{(uint64_t)pl.chunk_rows, pl.items.size(), pl.distances, tile_meta.size()};
    if (!tables) return d;
    for (uint32_t v : tile0) d.push_back(v);
    for (uint32_t v : tile_meta) d.push_back(v);
    for (const lcm::L2CountItem& i : pl.items)
        for (uint32_t v : {i.q_tile, i.q_rows, i.t_tile, i.t_rows, i.pair, i.reserved[0], i.reserved[1], i.reserved[2]}) d.push_back(v);
    return d;
}

// [chunk rows, pairs, workgroups, records, distances, runs, loops | admitted, 9999 | live, 9999 | adm_before | live_before | runs |
//  run_of (9999: none) | candidates: curr, past, matches, similarity's bits]
static Dump store_dump(const std::vector<int>& rows, const std::vector<lcm::L2StoreCurr>& currs, const uint8_t* skip, int min_rows,
                       int min_matches, const std::vector<lcm_l2_score>& rec) {
    lcm::L2StorePlan pl;
    CHECK(lcm::l2_store_plan(rows.data(), rows.size(), currs, skip, min_rows, pl) == nullptr);
    CHECK(pl.n_rec <= rec.size());
    std::vector<lcm_loop_candidate> cands(pl.n_pairs + 1);
    const size_t found = lcm::l2_store_walk(pl, rows.data(), rows.size(), currs, rec.data(), min_matches, nullptr);
    CHECK(found <= pl.n_pairs);
    CHECK(lcm::l2_store_walk(pl, rows.data(), rows.size(), currs, rec.data(), min_matches, cands.data()) == found);
    Dump d{(uint64_t)pl.chunk_rows, pl.n_pairs, pl.n_wg, pl.n_rec, pl.distances, pl.runs.size(), found};
    for (uint32_t v : pl.admitted) d.push_back(v);
    d.push_back(9999);
    for (uint32_t v : pl.live) d.push_back(v);
    d.push_back(9999);
    for (uint32_t v : pl.adm_before) d.push_back(v);
    for (uint32_t v : pl.live_before) d.push_back(v);
    for (const lcm::L2StoreRun& r : pl.runs) for (uint32_t v : {r.q_tile, r.q_rows, r.chunks, r.first_wg, r.first_pair, r.n_past}) d.push_back(v);
    for (size_t v : pl.run_of) d.push_back(v == (size_t)-1 ? 9999 : v);
    for (size_t k = 0; k < found; ++k) {
        uint64_t bits;
        std::memcpy(&bits, &cands[k].similarity_score, sizeof bits);
        for (uint64_t v : {(uint64_t)cands[k].current_frame_id, (uint64_t)cands[k].matched_frame_id, (uint64_t)cands[k].num_matches, bits}) d.push_back(v);
    }
    return d;
}

static const Dump RUN_SIZES = {
    128, 31, 16, 513, 396102, 65, 0, 1, 2, 4, 8, 13, 21, 30, 46, 63, 63, 65, 1, 32, 32, 257, 32, 288,
    544, 800, 32, 288, 544, 800, 1025, 32, 288, 544, 800, 1056, 1312, 1568, 1824, 32, 288, 544, 800, 1056, 1312, 1568, 1824, 2049,
    32, 288, 544, 800, 1056, 1312, 1568, 1824, 2080, 2336, 2592, 2848, 3104, 3360, 3616, 3872, 32, 288, 544, 800, 1056, 1312, 1568, 1824,
    2080, 2336, 2592, 2848, 3104, 3360, 3616, 3872, 4097, 32, 264, 0, 1, 46, 512, 0, 1, 62, 1, 1, 32, 30, 512, 2,
    33, 21, 257, 4, 128, 13, 256, 8, 128, 8, 129, 12, 1, 8, 129, 13, 128, 4, 128, 17, 128, 4, 128, 21,
    128, 2, 33, 25, 128, 2, 33, 29, 1, 2, 33, 30, 128, 1, 32, 34, 128, 1, 32, 38, 128, 1, 32, 42,
    128, 1, 32, 46, 128, 0, 1, 50, 128, 0, 1, 54, 128, 0, 1, 58, 128, 0, 1, 62, 1, 0, 1, 46,
    128, 46, 512, 46, 128, 62, 1, 50, 128, 46, 512, 50, 128, 62, 1, 54, 128, 46, 512, 54, 128, 62, 1, 58,
    128, 46, 512, 58, 128, 62, 1, 62, 1, 46, 512, 62, 1, 62, 1, 0, 1, 46, 513, 0, 2, 0, 0, 1,
    32, 30, 512, 2, 1, 1, 1, 2, 33, 21, 257, 3, 1, 33, 2, 4, 128, 13, 256, 4, 1, 66, 3, 8,
    129, 8, 129, 5, 1, 194, 4, 13, 256, 4, 128, 7, 1, 323, 5, 21, 257, 2, 33, 9, 1, 579, 6, 30,
    512, 1, 32, 12, 1, 836, 8, 46, 513, 0, 1, 16, 1, 1348, 10, 46, 513, 46, 513, 21, 2, 1861, 13, 0,
    1, 33, 66, 194, 323, 579, 836, 1348, 1861, 2374,};
static const Dump COUNT_SIZES = {
    128, 25, 396102, 63, 0, 1, 2, 4, 8, 13, 21, 30, 46, 63, 63, 63, 1, 32, 32, 257, 32, 288, 544, 800,
    32, 288, 544, 800, 1025, 32, 288, 544, 800, 1056, 1312, 1568, 1824, 32, 288, 544, 800, 1056, 1312, 1568, 1824, 2049, 32, 288,
    544, 800, 1056, 1312, 1568, 1824, 2080, 2336, 2592, 2848, 3104, 3360, 3616, 3872, 32, 288, 544, 800, 1056, 1312, 1568, 1824, 2080, 2336,
    2592, 2848, 3104, 3360, 3616, 3872, 4097, 0, 1, 46, 513, 0, 0, 0, 0, 1, 32, 30, 512, 1, 0, 0, 0, 2,
    33, 21, 257, 2, 0, 0, 0, 4, 128, 13, 256, 3, 0, 0, 0, 8, 128, 8, 129, 4, 0, 0, 0, 12,
    1, 8, 129, 4, 0, 0, 0, 13, 128, 4, 128, 5, 0, 0, 0, 17, 128, 4, 128, 5, 0, 0, 0, 21,
    128, 2, 33, 6, 0, 0, 0, 25, 128, 2, 33, 6, 0, 0, 0, 29, 1, 2, 33, 6, 0, 0, 0, 30,
    128, 1, 32, 7, 0, 0, 0, 34, 128, 1, 32, 7, 0, 0, 0, 38, 128, 1, 32, 7, 0, 0, 0, 42,
    128, 1, 32, 7, 0, 0, 0, 46, 128, 0, 1, 8, 0, 0, 0, 50, 128, 0, 1, 8, 0, 0, 0, 54,
    128, 0, 1, 8, 0, 0, 0, 58, 128, 0, 1, 8, 0, 0, 0, 62, 1, 0, 1, 8, 0, 0, 0, 46,
    128, 46, 513, 9, 0, 0, 0, 50, 128, 46, 513, 9, 0, 0, 0, 54, 128, 46, 513, 9, 0, 0, 0, 58,
    128, 46, 513, 9, 0, 0, 0, 62, 1, 46, 513, 9, 0, 0, 0,};
static const Dump RUN_1023_unset = {
    128, 1023, 1023, 1, 1023, 2,};
static const Dump COUNT_1023_unset = {
    128, 1023, 1023, 2,};
static const Dump RUN_1023_128 = {
    128, 1023, 1023, 1, 1023, 2,};
static const Dump COUNT_1023_128 = {
    128, 1023, 1023, 2,};
static const Dump RUN_1023_256 = {
    256, 1023, 1023, 1, 1023, 2,};
static const Dump COUNT_1023_256 = {
    256, 1023, 1023, 2,};
static const Dump RUN_1023_192 = {
    128, 1023, 1023, 1, 1023, 2,};
static const Dump COUNT_1023_192 = {
    128, 1023, 1023, 2,};
static const Dump RUN_1024_unset = {
    256, 1024, 1024, 1, 1024, 2,};
static const Dump COUNT_1024_unset = {
    256, 1024, 1024, 2,};
static const Dump RUN_1024_128 = {
    128, 1024, 1024, 1, 1024, 2,};
static const Dump COUNT_1024_128 = {
    128, 1024, 1024, 2,};
static const Dump RUN_1024_256 = {
    256, 1024, 1024, 1, 1024, 2,};
static const Dump COUNT_1024_256 = {
    256, 1024, 1024, 2,};
static const Dump RUN_1024_192 = {
    256, 1024, 1024, 1, 1024, 2,};
static const Dump COUNT_1024_192 = {
    256, 1024, 1024, 2,};
static const Dump STORE_MIN100 = {
    128, 10, 22, 6, 627069, 2, 3, 2, 3, 5, 6, 9999, 2, 3, 5, 6, 9999, 0, 0, 0, 1, 2, 2, 3,
    4, 0, 0, 0, 1, 2, 2, 3, 4, 114, 513, 5, 0, 0, 2, 131, 300, 3, 10, 2, 4, 9999, 9999, 0,
    1, 9999, 9999, 12, 3, 7, 0x3F8BF206FC81BF20ull, 13, 3, 10, 0x3FA1111111111111ull, 13, 5, 6, 0x3FA7D05F417D05F4ull,};
static const Dump STORE_MIN0 = {
    128, 16, 25, 7, 656769, 2, 4, 1, 2, 3, 4, 5, 6, 9999, 2, 3, 4, 5, 6, 9999, 0, 0, 1, 2,
    3, 4, 5, 6, 0, 0, 0, 1, 2, 3, 4, 5, 114, 513, 5, 0, 0, 2, 131, 300, 3, 10, 2, 5,
    9999, 9999, 0, 1, 9999, 9999, 12, 3, 7, 0x3F8BF206FC81BF20ull, 13, 3, 10, 0x3FA1111111111111ull, 13, 4, 6, 0x3FAF07C1F07C1F08ull, 13, 6, 9, 0x3F9EB851EB851EB8ull,};
static const Dump STORE_MIN0_ALL = {
    128, 21, 37, 11, 932016, 4, 21, 0, 1, 2, 3, 4, 5, 6, 9999, 0, 2, 3, 4, 5, 6, 9999, 0, 1,
    2, 3, 4, 5, 6, 7, 0, 1, 1, 2, 3, 4, 5, 6, 109, 129, 2, 0, 0, 1, 114, 513, 5, 2,
    1, 3, 131, 300, 3, 17, 4, 6, 141, 129, 2, 35, 10, 1, 9999, 0, 1, 2, 9999, 3, 11, 0, 0, 0,
    11, 1, 0, 0, 12, 0, 7, 0x3F9BE41BE41BE41Cull, 12, 1, 0, 0, 12, 2, 3, 0x3F9EB851EB851EB8ull, 12, 3, 10, 0x3F93F604FD813F60ull, 13, 0, 6, 0x3F97E817E817E818ull,
    13, 1, 0, 0, 13, 2, 2, 0x3F947AE147AE147Bull, 13, 3, 9, 0x3F9EB851EB851EB8ull, 13, 4, 5, 0x3FA9DBCC48676F31ull, 13, 5, 1, 0x3F7FC07F01FC07F0ull, 13, 6, 8, 0x3F9B4E81B4E81B4Full,
    14, 0, 0, 0, 14, 1, 0, 0, 14, 2, 0, 0, 14, 3, 0, 0, 14, 4, 0, 0, 14, 5, 0, 0,
    14, 6, 0, 0, 15, 0, 4, 0x3F9FC07F01FC07F0ull,};
static const Dump STORE_EMPTY = {
    128, 0, 0, 0, 0, 0, 0, 9999, 9999, 0, 0, 9999, 9999, 9999, 9999, 9999, 9999,};

// A list CALL over `rows` whose pairs may have an empty side (lcm_l2_db_match_points: live = the pairs with rows on both sides,
// job_of[p] = pair p's job or -1): l2_run_plan's block and row prefixes and l2_pair_block against sums taken pair by pair from
// the row counts alone.  Returns the call's blocks.
static size_t check_ragged_call(const std::vector<int>& rows, const std::vector<L2Pair>& call) {
    std::vector<uint32_t> tile0, tile_meta;
    lcm::l2_tile_space(rows.data(), (int)rows.size(), tile0, tile_meta);
    std::vector<L2Pair> live;
    std::vector<int> job_of;
    for (const L2Pair& p : call) {
        const bool has = rows[(size_t)p.q] > 0 && rows[(size_t)p.t] > 0;
        job_of.push_back(has ? (int)live.size() : -1);
        if (has) live.push_back(p);
    }
    lcm::L2RunPlan pl;
    CHECK(lcm::l2_run_plan(live, rows.data(), tile0.data(), pl) == nullptr);
    CHECK(pl.jobs.size() == live.size() && pl.row0.size() == live.size() + 1);
    // block_at[p] / row_at[p]: blocks and query rows of the live pairs BEFORE position p of the call
    std::vector<uint64_t> block_at(call.size() + 1, 0), row_at(call.size() + 1, 0);
    int longest = 0;
    for (size_t p = 0; p < call.size(); ++p) {
        const int nq = job_of[p] >= 0 ? rows[(size_t)call[p].q] : 0;
        block_at[p + 1] = block_at[p] + (uint64_t)((nq + 255) / 256);
        row_at[p + 1] = row_at[p] + (uint64_t)nq;
        longest = std::max(longest, nq);
    }
    CHECK(pl.n_blocks == block_at[call.size()] && pl.row0[live.size()] == row_at[call.size()] && pl.max_nq == longest);
    for (size_t p = 0; p < call.size(); ++p) {
        if (job_of[p] < 0) continue;
        const lcm::L2Job& j = pl.jobs[(size_t)job_of[p]];
        CHECK(j.reserved == block_at[p] && j.out_row0 == row_at[p] && pl.row0[(size_t)job_of[p]] == row_at[p]);
        CHECK(j.nq == (uint32_t)rows[(size_t)call[p].q] && j.nt == (uint32_t)rows[(size_t)call[p].t]);
        CHECK(j.q_tile == tile0[(size_t)call[p].q] && j.t_tile == tile0[(size_t)call[p].t]);
    }
    std::vector<uint32_t> pair_block(3, 77u);                      // resized and overwritten whole
    lcm::l2_pair_block(job_of, pl.jobs, pl.n_blocks, pair_block);
    CHECK(pair_block.size() == call.size() + 1);
    for (size_t p = 0; p <= call.size() && p < pair_block.size(); ++p) {
        size_t k = p;
        while (k < call.size() && job_of[k] < 0) ++k;              // the first live pair at or after p; none: every block lies before
        CHECK(pair_block[p] == block_at[k]);
    }
    return pl.n_blocks;
}

static void pin(const char* v) {
    if (v) { setenv("LCM_TUNE_L2_CHUNK", v, 1); setenv("LCM_TUNE_L2_COUNT_CHUNK", v, 1); }
    else { unsetenv("LCM_TUNE_L2_CHUNK"); unsetenv("LCM_TUNE_L2_COUNT_CHUNK"); }
}

int main() {
    pin(nullptr);
    // Rows of 1, 32, 33, 128, 129, 256, 257, 512 and 513 as query and as train (pair i = matrix i against matrix 8 - i: pair 4
    // names one matrix on both sides, and so does the last pair), an empty matrix, and one of 40 rows that no pair names: the
    // list plan gives it tiles 63 and 64, the count plan none.
    const int rows[11] = {1, 32, 33, 128, 129, 256, 257, 512, 513, 0, 40};
    std::vector<L2Pair> pairs;
    for (int i = 0; i < 9; ++i) pairs.push_back(L2Pair{i, 8 - i});
    pairs.push_back(L2Pair{8, 8});
    CHECK(run_dump(rows, 11, pairs) == RUN_SIZES);
    CHECK(count_dump(rows, 11, pairs) == COUNT_SIZES);

    // The chunk rule at its threshold: 1023 and 1024 items-at-256 (pairs over the same two one-row matrices), unpinned, pinned to
    // each legal value, and to an illegal one (ignored)
    const int one[2] = {1, 1};
    const std::vector<L2Pair> p1023(1023, L2Pair{0, 1}), p1024(1024, L2Pair{0, 1});
    pin(nullptr);
    CHECK(run_dump(one, 2, p1023, false) == RUN_1023_unset && count_dump(one, 2, p1023, false) == COUNT_1023_unset);
    CHECK(run_dump(one, 2, p1024, false) == RUN_1024_unset && count_dump(one, 2, p1024, false) == COUNT_1024_unset);
    pin("128");
    CHECK(run_dump(one, 2, p1023, false) == RUN_1023_128 && count_dump(one, 2, p1023, false) == COUNT_1023_128);
    CHECK(run_dump(one, 2, p1024, false) == RUN_1024_128 && count_dump(one, 2, p1024, false) == COUNT_1024_128);
    pin("256");
    CHECK(run_dump(one, 2, p1023, false) == RUN_1023_256 && count_dump(one, 2, p1023, false) == COUNT_1023_256);
    CHECK(run_dump(one, 2, p1024, false) == RUN_1024_256 && count_dump(one, 2, p1024, false) == COUNT_1024_256);
    pin("192");
    CHECK(run_dump(one, 2, p1023, false) == RUN_1023_192 && count_dump(one, 2, p1023, false) == COUNT_1023_192);
    CHECK(run_dump(one, 2, p1024, false) == RUN_1024_192 && count_dump(one, 2, p1024, false) == COUNT_1024_192);
    pin(nullptr);
    // ... and their tables, which are regular: pair p is item p, job p, row p, block p
    {
        std::vector<uint32_t> tile0, tile_meta;
        lcm::l2_tile_space(one, 2, tile0, tile_meta);
        lcm::L2RunPlan pl;
        CHECK(lcm::l2_run_plan(p1024, one, tile0.data(), pl) == nullptr && pl.items.size() == 1024);
        for (uint32_t p = 0; p < 1024 && p < pl.items.size(); ++p) {
            const lcm::L2Item& i = pl.items[p];
            const lcm::L2Job& j = pl.jobs[p];
            CHECK(i.q_tile == 0 && i.q_rows == 1 && i.t_tile == 1 && i.t_rows == 1 && pl.row0[p] == p);
            CHECK(j.q_tile == 0 && j.nq == 1 && j.t_tile == 1 && j.nt == 1 && j.first_item == p && j.n_seg == 1 && j.out_row0 == p && j.reserved == p);
        }
        lcm::L2CountPlan cp;
        CHECK(lcm::l2_count_plan(p1024, one, tile0.data(), cp) == nullptr && cp.items.size() == 1024);
        for (uint32_t p = 0; p < 1024 && p < cp.items.size(); ++p) {
            const lcm::L2CountItem& i = cp.items[p];
            CHECK(i.q_tile == 0 && i.q_rows == 1 && i.t_tile == 1 && i.t_rows == 1 && i.pair == p && i.reserved[0] == 0 && i.reserved[1] == 0 && i.reserved[2] == 0);
        }
    }

    // Ragged tall calls (the store's list route, lcm_l2_db.cpp's store_lists): frames of 65535, 0, 1, 257, 32768 and 65535 rows;
    // live and empty-sided pairs interleaved, empty pairs first and last, every pair empty, no pair at all; both chunk pins
    {
        const std::vector<int> tall = {65535, 0, 1, 257, 32768, 65535};
        const std::vector<L2Pair> interleaved = {{0, 5}, {2, 0}, {1, 0}, {4, 5}, {3, 0}, {0, 1}, {5, 5}, {1, 1}, {2, 3}, {5, 0}};
        const std::vector<L2Pair> ends = {{1, 0}, {0, 1}, {5, 0}, {3, 4}, {1, 1}, {1, 5}, {0, 0}, {4, 2}, {2, 1}, {1, 3}};
        const std::vector<L2Pair> none = {{1, 0}, {0, 1}, {1, 1}, {5, 1}};
        for (const char* v : {(const char*)nullptr, "128", "256"}) {
            pin(v);
            CHECK(check_ragged_call(tall, interleaved) == 256 + 1 + 128 + 2 + 256 + 1 + 256);
            CHECK(check_ragged_call(tall, ends) == 256 + 2 + 256 + 128);
            CHECK(check_ragged_call(tall, none) == 0);
            CHECK(check_ragged_call(tall, {}) == 0);
            CHECK(check_ragged_call(tall, std::vector<L2Pair>(300, L2Pair{5, 2})) == 300 * 256);      // 76800 blocks, 19 660 500 rows
        }
        pin(nullptr);
    }

    // The store: slot 0 is skipped, slot 1 is empty (below min_rows = 100; admitted and empty with min_rows = 0), slot 2 holds
    // exactly 100 rows, slot 4 holds 99.  The currs: last_past = -1 (no pair), 1 (no admitted past at min_rows = 100; one empty
    // past and so no run at 0), 3, beyond the last slot, a curr without rows, and last_past = 0: six currs in one search.
    const std::vector<int> slots = {257, 0, 100, 513, 99, 129, 300};
    const uint8_t skip[7] = {1, 0, 0, 0, 0, 0, 0};
    const std::vector<lcm::L2StoreCurr> currs = {{10, 100, 257, -1}, {11, 109, 129, 1}, {12, 114, 513, 3}, {13, 131, 300, 100}, {14, 141, 0, 6}, {15, 141, 129, 0}};
    std::vector<lcm_l2_score> rec(32);
    for (size_t k = 0; k < rec.size(); ++k) rec[k] = lcm_l2_score{(uint32_t)(7 * k % 11), (uint32_t)(1000 + k)};
    CHECK(store_dump(slots, currs, skip, 100, 4, rec) == STORE_MIN100);
    CHECK(store_dump(slots, currs, skip, 0, 4, rec) == STORE_MIN0);
    CHECK(store_dump(slots, currs, nullptr, 0, 0, rec) == STORE_MIN0_ALL);      // min_matches = 0: every pair is a loop, empty sides score 0.0
    CHECK(store_dump({}, currs, nullptr, 0, 0, rec) == STORE_EMPTY);            // an empty store: no pair, no run

    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all held\n");
    return 0;
}
