// lcm_l2_host.h — the pure host side of the SIFT matcher (lcm_l2.cpp, lcm_l2_db.cpp): the tile space, the chunk rule, the items
// and jobs of a list run, the count items, a loop search's tables and runs and the walk over its records.  No HIP call and no
// handle: tests/cpp/l2_host_check.cpp runs this text stand-alone under a sanitizer.  A planner returns NULL or its refusal.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "../../include/lcm.h"
#include "lcm_kernels.h"

namespace lcm {

constexpr uint32_t L2_NONE = 0xFFFFFFFFu;   // D / index of a neighbour that does not exist
struct L2Pair { int q, t; };                // positions into the call's matrices, both sides non-empty

// The tile space: matrix f starts at tile tile0[f]; tile_meta = k_l2_pack's word per tile
inline void l2_tile_space(const int* rows, int n_frames, std::vector<uint32_t>& tile0, std::vector<uint32_t>& tile_meta) {
    tile0.assign((size_t)n_frames + 1, 0);
    tile_meta.clear();
    for (int f = 0; f < n_frames; ++f) {
        const uint32_t nt = (uint32_t)((rows[f] + L2_TILE_ROWS - 1) / L2_TILE_ROWS);
        tile0[(size_t)f + 1] = tile0[(size_t)f] + nt;
        for (uint32_t k = 0; k < nt; ++k) tile_meta.push_back((uint32_t)std::min(L2_TILE_ROWS, rows[f] - (int)k * L2_TILE_ROWS) | (k << 8));
    }
}

// Query chunk of an item: 128 rows (one tile per wave: twice the workgroups, the latency shape) while the call has few
// items, else 256 (two tiles per wave share every train fragment: the throughput shape).  items256: the call's items at 256
// rows per chunk.  The environment variable `pin` = 128 | 256 pins it: LCM_TUNE_L2_CHUNK for the list kernels
// (tools/l2_time.py measures both), LCM_TUNE_L2_COUNT_CHUNK for the count kernels (tools/l2_count_time.py).
inline int l2_chunk_rows(size_t items256, const char* pin) {
    if (const char* e = getenv(pin)) { const int v = atoi(e); if (v == 128 || v == 256) return v; }
    return items256 < 1024 ? 128 : 256;
}

// A list run over `pairs` (rows[f] rows at tile tile0[f]): one item per (query chunk x 512-row train segment), one job per
// pair; pair p's query rows are rows [row0[p], row0[p + 1]) of final_keys and blocks [jobs[p].reserved, ...) of 256 rows.
struct L2RunPlan {
    std::vector<L2Item> items; std::vector<L2Job> jobs; std::vector<size_t> row0;
    int chunk_rows = 0, max_nq = 0; size_t n_blocks = 0; uint64_t distances = 0;
};
inline const char* l2_run_plan(const std::vector<L2Pair>& pairs, const int* rows, const uint32_t* tile0, L2RunPlan& pl) {
    constexpr int TILE = L2_TILE_ROWS, SEG = L2_SEG_ROWS;
    const size_t P = pairs.size();
    size_t items256 = 0, total_rows = 0;
    for (const L2Pair& p : pairs) items256 += (size_t)((rows[p.q] + 255) / 256) * (size_t)((rows[p.t] + SEG - 1) / SEG);
    pl = L2RunPlan{};
    const int CH = pl.chunk_rows = l2_chunk_rows(items256, "LCM_TUNE_L2_CHUNK");
    pl.jobs.resize(P);
    pl.row0.assign(P + 1, 0);
    for (size_t p = 0; p < P; ++p) {
        const int nq = rows[pairs[p].q], nt = rows[pairs[p].t];
        const int n_chunks = (nq + CH - 1) / CH, n_seg = (nt + SEG - 1) / SEG;
        const uint32_t qt = tile0[(size_t)pairs[p].q], tt = tile0[(size_t)pairs[p].t];
        if (pl.items.size() + (size_t)n_chunks * (size_t)n_seg > 0x7FFFFFFFull || total_rows + (size_t)nq > 0x7FFFFFFFull)
            return "too many pairs for one call";
        pl.jobs[p] = {qt, (uint32_t)nq, tt, (uint32_t)nt, (uint32_t)pl.items.size(), (uint32_t)n_seg, (uint32_t)total_rows, (uint32_t)pl.n_blocks};
        pl.n_blocks += (size_t)((nq + 255) / 256);                // at most total_rows: fits the 32 bits
        for (int c = 0; c < n_chunks; ++c)
            for (int g = 0; g < n_seg; ++g)
                pl.items.push_back({qt + (uint32_t)(c * (CH / TILE)), (uint32_t)std::min(CH, nq - c * CH),
                                    tt + (uint32_t)(g * (SEG / TILE)), (uint32_t)std::min(SEG, nt - g * SEG)});
        pl.row0[p] = total_rows;
        total_rows += (size_t)nq;
        pl.max_nq = std::max(pl.max_nq, nq);
        pl.distances += (uint64_t)nq * (uint64_t)nt;
    }
    pl.row0[P] = total_rows;
    return nullptr;
}

// k_l2_emit_offsets' table over the pairs of a list CALL (job_of[p] = pair p's job, -1 when a side is empty): the first block
// of the first live pair at or after p, for every p <= n_pairs; n_blocks past the last live pair
inline void l2_pair_block(const std::vector<int>& job_of, const std::vector<L2Job>& jobs, size_t n_blocks, std::vector<uint32_t>& pair_block) {
    const size_t n_pairs = job_of.size();
    pair_block.resize(n_pairs + 1);
    uint32_t next = (uint32_t)n_blocks;
    pair_block[n_pairs] = next;
    for (size_t p = n_pairs; p-- > 0;) {
        if (job_of[p] >= 0) next = jobs[(size_t)job_of[p]].reserved;
        pair_block[p] = next;
    }
}

// A count run over the live pairs: one item per query chunk of a pair, whatever the train matrix's size; live[j]'s record is j
struct L2CountPlan { std::vector<L2CountItem> items; int chunk_rows = 0; uint64_t distances = 0; };
inline const char* l2_count_plan(const std::vector<L2Pair>& live, const int* rows, const uint32_t* tile0, L2CountPlan& pl) {
    if (live.size() > 0x7FFFFFFFull) return "too many pairs for one call";
    size_t items256 = 0, n_items = 0;
    for (const L2Pair& p : live) items256 += (size_t)((rows[p.q] + 255) / 256);
    pl = L2CountPlan{};
    const int CH = pl.chunk_rows = l2_chunk_rows(items256, "LCM_TUNE_L2_COUNT_CHUNK");
    for (const L2Pair& p : live) {
        n_items += (size_t)((rows[p.q] + CH - 1) / CH);
        pl.distances += (uint64_t)rows[p.q] * (uint64_t)rows[p.t];
    }
    if (n_items > 0x7FFFFFFFull) return "too many pairs for one call";
    pl.items.reserve(n_items);
    for (size_t j = 0; j < live.size(); ++j) {
        const int nq = rows[live[j].q], nt = rows[live[j].t];
        const uint32_t qt = tile0[(size_t)live[j].q], tt = tile0[(size_t)live[j].t];
        for (int c = 0; c * CH < nq; ++c)
            pl.items.push_back({qt + (uint32_t)(c * (CH / L2_TILE_ROWS)), (uint32_t)std::min(CH, nq - c * CH), tt, (uint32_t)nt, (uint32_t)j, {0, 0, 0}});
    }
    return nullptr;
}

// One `curr` of a loop search: the query matrix (tile, rows) and its admissible pasts = the admitted slots <= last_past
struct L2StoreCurr { int id; uint32_t q_tile; int q_rows; int last_past; };

// src/main.cpp:1375-1388 over S matrices (the store's slots, or a host call's), `currs` in ascending order.  A pair is (curr,
// admitted past <= last_past), in that order: n_pairs in all.  admitted / live: the admitted matrices, and those of them with
// rows (k_l2_count_store's `past`), ascending; adm_before[f] / live_before[f]: how many of them lie below f.  A curr with rows
// and with live pasts gets a run (run_of[u], else -1) of n_past * chunks workgroups and n_past records, record
// first_pair + live_before[past] being (curr, past)'s; a pair with an empty side has none.
struct L2StorePlan {
    std::vector<uint32_t> admitted, live, adm_before, live_before; std::vector<L2StoreRun> runs; std::vector<size_t> run_of;
    size_t n_pairs = 0; int chunk_rows = 0; uint64_t n_wg = 0, n_rec = 0, distances = 0;
};
inline size_t l2_store_pasts(const L2StoreCurr& c, size_t S) { return (size_t)std::min<long long>(c.last_past, (long long)S - 1) + 1; }   // pasts are [0, this)
inline const char* l2_store_plan(const int* rows, size_t S, const std::vector<L2StoreCurr>& currs, const uint8_t* skip, int min_rows,
                                 L2StorePlan& pl) {
    pl = L2StorePlan{};
    pl.adm_before.assign(S + 1, 0);
    pl.live_before.assign(S + 1, 0);
    std::vector<uint64_t> rows_before(S + 1, 0);              // rows of the live admitted matrices below f
    for (size_t f = 0; f < S; ++f) {
        const bool adm = !(skip && skip[f]) && rows[f] >= min_rows, has = adm && rows[f] > 0;     // :1377 / :1381, :1382
        pl.adm_before[f + 1] = pl.adm_before[f] + (adm ? 1u : 0u);
        pl.live_before[f + 1] = pl.live_before[f] + (has ? 1u : 0u);
        rows_before[f + 1] = rows_before[f] + (has ? (uint64_t)rows[f] : 0);
        if (adm) pl.admitted.push_back((uint32_t)f);
        if (has) pl.live.push_back((uint32_t)f);
    }
    pl.run_of.assign(currs.size(), (size_t)-1);
    size_t items256 = 0;
    for (const L2StoreCurr& c : currs) {
        if (c.last_past < 0) continue;
        pl.n_pairs += pl.adm_before[l2_store_pasts(c, S)];
        if (c.q_rows > 0) items256 += (size_t)pl.live_before[l2_store_pasts(c, S)] * (size_t)((c.q_rows + 255) / 256);
    }
    const int CH = pl.chunk_rows = l2_chunk_rows(items256, "LCM_TUNE_L2_COUNT_CHUNK");
    for (size_t u = 0; u < currs.size(); ++u) {
        const L2StoreCurr& c = currs[u];
        if (c.last_past < 0 || c.q_rows <= 0) continue;
        const size_t last = l2_store_pasts(c, S);
        const uint32_t np = pl.live_before[last];
        if (np == 0) continue;                                   // no admitted past: no run, no record
        const uint32_t chunks = (uint32_t)((c.q_rows + CH - 1) / CH);
        if (pl.n_wg + (uint64_t)np * chunks > 0x7FFFFFFFull || pl.n_rec + np > 0x7FFFFFFFull) return "too many pairs for one call";
        pl.run_of[u] = pl.runs.size();
        pl.runs.push_back({c.q_tile, (uint32_t)c.q_rows, chunks, (uint32_t)pl.n_wg, (uint32_t)pl.n_rec, np});
        pl.n_wg += (uint64_t)np * chunks;
        pl.n_rec += np;
        pl.distances += (uint64_t)c.q_rows * rows_before[last];
    }
    return nullptr;
}

// The verdict (:1388) over a planned search's records in (curr, past) order: the loops' number, their candidates to dst if given
inline size_t l2_store_walk(const L2StorePlan& pl, const int* rows, size_t S, const std::vector<L2StoreCurr>& currs, const lcm_l2_score* rec,
                            int min_matches, lcm_loop_candidate* dst) {
    size_t found = 0;
    for (size_t u = 0; u < currs.size(); ++u) {
        const L2StoreCurr& c = currs[u];
        if (c.last_past < 0) continue;
        const lcm_l2_score* r = pl.run_of[u] == (size_t)-1 ? nullptr : rec + pl.runs[pl.run_of[u]].first_pair;
        for (uint32_t k = 0; k < pl.adm_before[l2_store_pasts(c, S)]; ++k) {
            const uint32_t past = pl.admitted[k];
            const lcm_l2_score sc = (r && rows[past] > 0) ? r[pl.live_before[past]] : lcm_l2_score{0u, L2_NONE};
            if ((long long)sc.good_count < (long long)min_matches) continue;
            const int den = std::min(c.q_rows, rows[past]);
            if (dst) dst[found] = lcm_loop_candidate{c.id, (int32_t)past, (int32_t)sc.good_count, den > 0 ? (double)sc.good_count / (double)den : 0.0};
            ++found;
        }
    }
    return found;
}

}  // namespace lcm
