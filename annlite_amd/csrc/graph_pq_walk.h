// graph_pq_walk.h -- the beam walk over the HNSW-over-PQ graph, ONE COPY for the kernels that walk it: graph.hip's
// graph_beam_search_kernel (one list, the caller's candidates) and graph_admit.hip's graph_pq_admit_kernel (the same routing list
// plus a result list of admitted rows).  A kernel sets its wave up with pq_walk_setup, then calls pq_beam_walk with what is to
// happen to every batch of evaluated nodes -- a seed round, a step's unseen neighbours -- as `offer(mine, node, sum)`.  What the
// walk is and why it is laid out like this: graph.hip's header.
#pragma once
#include "scan_common.h"
#include "graph_beam.h"

namespace annlite {

// ANNLITE_DEBUG_COUNTERS: link lists read, rows evaluated, prefetched records used; shader cycles by phase (packed walk)
struct PQWalkCounters {
    unsigned int n_expand = 0, n_eval = 0, n_hit = 0;
    unsigned long long t_seed = 0, t_rec = 0, t_visit = 0, t_sum = 0, t_offer = 0;
};

static inline int64_t graph_record_stride(int64_t L, int64_t M) { return ((L * M + 4 * L + 4 + 15) / 16) * 16; }

// LDS of one walking wave: the query's table, the visited table, the merge's scratch (BATCH)
template <int E, bool BATCH>
static inline size_t pq_walk_lds_per_wave(int64_t M, int64_t Ks, int hash_bits) {
    return (size_t)M * Ks * 4 + ((size_t)4 << hash_bits) + (BATCH ? (size_t)E * 64 * 12 + 1024 : 0);
}

// the 4-wave-at-most workgroup of a walk and its LDS; 0 waves: the tables do not fit
static inline int pq_walk_waves_per_block(size_t per_wave) {
    int wpb = (int)((size_t)160 * 1024 / per_wave);
    return wpb > 4 ? 4 : wpb;
}

// The wave's table and visited table filled, its list `bm` (cap = ef) empty; `s_lut`: the table.
template <int M, int E, bool BATCH>
__device__ __forceinline__ void pq_walk_setup(unsigned char *smem, int wave, int lane, const float *__restrict__ lut_bmk, int b, int Ks,
                                              int ef, int hash_bits, Beam<E, BATCH> &bm, float *&s_lut) {
    const uint32_t hash_n = 1u << hash_bits;
    const size_t per_wave = (size_t)M * Ks * 4 + (size_t)hash_n * 4 + (BATCH ? (size_t)E * 64 * 12 + 1024 : 0);  // (pq_walk_lds_per_wave)
    s_lut = (float *)(smem + wave * per_wave);
    uint32_t *s_hash = (uint32_t *)(smem + wave * per_wave + (size_t)M * Ks * 4);
    uint32_t *s_mrg = s_hash + hash_n;  // BATCH: the merge's scratch, u32 [3][64 E]: keys hi, ids, expanded flags; then u32 [4][64]: the
                                        // candidates compacted (hi, id) and by rank (hi, id)
    {
        const f32x4 *src = (const f32x4 *)(lut_bmk + (int64_t)b * M * Ks);
        for (int i = lane; i < M * Ks / 4; i += 64) ((f32x4 *)s_lut)[i] = src[i];
        for (uint32_t i = lane; i < hash_n / 4; i += 64) ((u32x4 *)s_hash)[i] = (u32x4){kEmpty, kEmpty, kEmpty, kEmpty};
    }
    // (one wave: its LDS writes are visible to its own later reads in program order)

    // the list, its insertion and the visited table: graph_beam.h
    // (by LDS byte address in the LDS address space: through a generic volatile pointer the bucket read was a FLAT load, and a flat
    // load counts on the vector-memory counter too -- every probe then waited for the prefetched record)
    typedef __attribute__((address_space(3))) unsigned char *lds_bytes;
    const uint32_t hash_ad = (uint32_t)(uintptr_t)(lds_bytes)smem + (uint32_t)(wave * per_wave) + (uint32_t)(M * Ks * 4);
    bm.init(lane, ef, s_mrg, hash_ad, hash_bits);
}

// Seeds, then the walk, until `bm`'s list holds no unexpanded node.  `timed`: the phase cycle counters are kept.
// BATCH: see graph_beam.h.  W (PACKED only): nodes expanded per step -- 2 = the PAIR walk (graph.hip's header).
template <int M, int E, bool PACKED, bool BATCH, int W, class Offer>
__device__ __forceinline__ void pq_beam_walk(Beam<E, BATCH> &bm, const float *s_lut, int lane, const uint32_t *__restrict__ links,
                                             int links_per_node, const uint8_t *__restrict__ packed, int64_t rec_stride,
                                             const uint32_t *__restrict__ seeds, int n_seeds, const uint8_t *__restrict__ codes, int64_t N,
                                             int Ks, const void *stats, Offer &&offer, PQWalkCounters &ct) {
    constexpr int CW = M / 4;
    unsigned int &n_expand = ct.n_expand, &n_eval = ct.n_eval, &n_hit = ct.n_hit;
    unsigned long long &t_seed = ct.t_seed, &t_rec = ct.t_rec, &t_visit = ct.t_visit, &t_sum = ct.t_sum, &t_offer = ct.t_offer;
    auto now = [&]() -> unsigned long long { return stats ? __builtin_readcyclecounter() : 0ull; };
    BeamList<E> &L = bm.L;
    const int cap = bm.cap;
    auto visit = [&](uint32_t node) -> bool { return bm.visit(node); };
    auto pick_next = [&](uint32_t &node, uint32_t &second) -> bool { return bm.pick_next(node, second); };
    auto load_row = [&](uint32_t node, uint32_t (&c)[CW]) {
        const uint32_t *p = (const uint32_t *)(codes + (int64_t)node * M);
#pragma unroll
        for (int i = 0; i < CW; ++i) c[i] = p[i];
    };
    auto pq_sum = [&](const uint32_t (&c)[CW]) -> float {  // hnswlib::PQLookup: ascending-m fp32 adds
        float d = 0.f;
#pragma unroll
        for (int m = 0; m < M; ++m) d += s_lut[m * Ks + ((c[m / 4] >> (8 * (m % 4))) & 0xffu)];
        return d;
    };
    auto pq_lookup = [&](uint32_t node) -> float {
        uint32_t c[CW];
        load_row(node, c);
        return pq_sum(c);
    };

    // ---- seeds: the top of the hierarchy, scanned flat -------------------------------------------------
    // (seeds are distinct: no visited check while scanning them; only the ones that made the list are recorded --
    // recording all of them would fill the hash table before the walk starts)
    // (the round's code rows are requested one round ahead, its seed ids two: the rounds' two dependent round trips overlap
    // the previous rounds' insertions; the ORDER of the offers is unchanged)
    {
        const unsigned long long t_s0 = now();
        auto seed_at = [&](int s0) -> uint32_t { return s0 + lane < n_seeds ? seeds[s0 + lane] : 0xffffffffu; };
        uint32_t node_cur = seed_at(0), node_nxt = seed_at(64);
        uint32_t c_cur[CW];
        load_row(((int64_t)node_cur < N) ? node_cur : 0u, c_cur);
        for (int s0 = 0; s0 < n_seeds; s0 += 64) {
            const uint32_t node = node_cur;
            const bool mine = s0 + lane < n_seeds && (int64_t)node < N;
            uint32_t c[CW];
#pragma unroll
            for (int i = 0; i < CW; ++i) c[i] = c_cur[i];
            node_cur = node_nxt;
            if (s0 + 64 < n_seeds) load_row(((int64_t)node_cur < N) ? node_cur : 0u, c_cur);
            node_nxt = seed_at(s0 + 128);
            const float d = mine ? pq_sum(c) : 0.f;
            n_eval += (unsigned int)__popcll(__ballot(mine));
            offer(mine, node, d);
        }
        t_seed = now() - t_s0;
    }
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (L.lo[e] != kIdNone) visit(L.lo[e]);

    // ---- walk ------------------------------------------------------------------------------------------
    if constexpr (PACKED && W == 2) {
        const int Lc = links_per_node;  // (<= 32: one HALF wave per record)
        const int half = lane >> 5, hj = lane & 31;
        // the record of `node` as seen by this lane's half: neighbour hj's code row and id (slots beyond the count hold 0xffffffff)
        auto load_rec = [&](uint32_t node, uint32_t (&c)[CW], uint32_t &nb) {
            const uint8_t *r = packed + (int64_t)node * rec_stride;
            const int j = hj < Lc ? hj : 0;
            const uint32_t *pc = (const uint32_t *)(r + (int64_t)j * M);
#pragma unroll
            for (int i = 0; i < CW; ++i) c[i] = pc[i];
            nb = ((const uint32_t *)(r + (int64_t)Lc * M))[j];
        };
        // the two best unexpanded entries (marked expanded) and the two after them (the halves' prefetch targets)
        auto pick_pair = [&](uint32_t (&nd)[4]) -> bool {
            int p[4] = {-1, -1, -1, -1};
            int found = 0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (found < 4) {
                    unsigned long long m = __ballot(!L.exp[e] && (e * 64 + lane) < cap);
                    while (m && found < 4) {
                        p[found++] = e * 64 + __builtin_ctzll(m);
                        m &= m - 1;
                    }
                }
            }
            if (found == 0) return false;
#pragma unroll
            for (int i = 0; i < 4; ++i) nd[i] = kEmpty;
#pragma unroll
            for (int e = 0; e < E; ++e) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (p[i] >= 0 && p[i] / 64 == e) nd[i] = __builtin_amdgcn_readlane(L.lo[e], p[i] % 64);
                if ((p[0] >= 0 && p[0] / 64 == e && lane == p[0] % 64) || (p[1] >= 0 && p[1] / 64 == e && lane == p[1] % 64)) L.exp[e] = true;
            }
            return true;
        };
        uint32_t pf_c[CW], pf_nb = kEmpty, pf_node = kEmpty;  // this HALF's prefetched record (pf_node == kEmpty: none)
#pragma unroll
        for (int i = 0; i < CW; ++i) pf_c[i] = 0;
        for (;;) {
            uint32_t nd[4];
            const unsigned long long t0 = now();
            if (!pick_pair(nd)) break;
            // a prefetched record stays in the half that holds it: the halves swap nodes when that keeps more of them (the
            // candidates of a step are merged as a SET -- which half evaluated a neighbour does not matter)
            const uint32_t pf0 = __builtin_amdgcn_readlane(pf_node, 0), pf1 = __builtin_amdgcn_readlane(pf_node, 32);
            const bool two = nd[1] != kEmpty;
            const int keep_straight = (pf0 == nd[0] ? 1 : 0) + (two && pf1 == nd[1] ? 1 : 0);
            const int keep_swapped = (two && pf0 == nd[1] ? 1 : 0) + (pf1 == nd[0] ? 1 : 0);
            const bool swapped = keep_swapped > keep_straight;
            const uint32_t node = ((half != 0) != swapped) ? nd[1] : nd[0];
            const bool have = node != kEmpty;
            uint32_t c[CW], nb = kEmpty;
#pragma unroll
            for (int i = 0; i < CW; ++i) c[i] = 0;
            if (have && pf_node == node) {
#pragma unroll
                for (int i = 0; i < CW; ++i) c[i] = pf_c[i];
                nb = pf_nb;
            } else if (have) {
                load_rec(node, c, nb);
            }
            n_hit += (unsigned int)__popcll(__ballot(have && pf_node == node && hj == 0));
            // (the current records must have ARRIVED before the prefetches are issued: see the one-at-a-time loop below)
            asm volatile("" : "+v"(nb));
#pragma unroll
            for (int i = 0; i < CW; ++i) asm volatile("" : "+v"(c[i]));
            // half 0 requests the best node that is unexpanded NOW, half 1 the one after it: the next pair unless this step's
            // neighbours turn out better
            pf_node = half ? nd[3] : nd[2];
            if (pf_node != kEmpty) load_rec(pf_node, pf_c, pf_nb);
            n_expand += two ? 2u : 1u;
            const unsigned long long t1 = now();
            // (a neighbour of BOTH nodes is probed by two lanes at once: the table's compare-and-swap lets exactly one of them through)
            bool mine = have && hj < Lc;
            mine = mine && (int64_t)nb < N && visit(nb);
            n_eval += (unsigned int)__popcll(__ballot(mine));
            const unsigned long long t2 = now();
            float d = mine ? pq_sum(c) : 0.f;
            if (stats) asm volatile("" : "+v"(d));
            const unsigned long long t3 = now();
            offer(mine, nb, d);
            if (stats) {
                const unsigned long long t4 = now();
                t_rec += t1 - t0, t_visit += t2 - t1, t_sum += t3 - t2, t_offer += t4 - t3;
            }
        }
    } else if constexpr (PACKED) {
        // record of a node: lane j < L holds neighbour j's code row and id; the count is a wave-uniform load
        const int Lc = links_per_node;  // (<= 64: one lane per neighbour)
        // (slots beyond the node's count hold the id 0xffffffff, which fails the `nb < N` test like any id beyond the table:
        // the walk never reads the count -- a wave-uniform, i.e. SCALAR load would share its counter with the LDS traffic of
        // visit() and stall it for a full memory round trip whenever a prefetch is in flight)
        auto load_rec = [&](uint32_t node, uint32_t (&c)[CW], uint32_t &nb) {
            const uint8_t *r = packed + (int64_t)node * rec_stride;
            const int j = lane < Lc ? lane : 0;
            const uint32_t *pc = (const uint32_t *)(r + (int64_t)j * M);
#pragma unroll
            for (int i = 0; i < CW; ++i) c[i] = pc[i];
            nb = ((const uint32_t *)(r + (int64_t)Lc * M))[j];
        };
        uint32_t pf_c[CW], pf_nb = 0, pf_node = kEmpty;  // the prefetched record (pf_node == kEmpty: none)
#pragma unroll
        for (int i = 0; i < CW; ++i) pf_c[i] = 0;
        for (;;) {
            uint32_t node = 0, second = kEmpty;
            const unsigned long long t0 = now();
            if (!pick_next(node, second)) break;
            uint32_t c[CW], nb;
            if (pf_node == node) {
                ++n_hit;
#pragma unroll
                for (int i = 0; i < CW; ++i) c[i] = pf_c[i];
                nb = pf_nb;
            } else {
                load_rec(node, c, nb);
            }
            // The current record must have ARRIVED before the prefetch below is issued: the memory counter is in order and the
            // compiler, merging the paths with and without a prefetch, otherwise waits for everything outstanding -- the
            // prefetch included -- at the first use of the current record.  (An empty asm that reads the registers.)
            asm volatile("" : "+v"(nb));
#pragma unroll
            for (int i = 0; i < CW; ++i) asm volatile("" : "+v"(c[i]));
            // request the record of the best node that is unexpanded NOW: the next pick unless one of this node's neighbours
            // turns out better
            pf_node = second;
            if (second != kEmpty) load_rec(second, pf_c, pf_nb);
            ++n_expand;
            const unsigned long long t1 = now();
            bool mine = lane < Lc;
            mine = mine && (int64_t)nb < N && visit(nb);
            n_eval += (unsigned int)__popcll(__ballot(mine));
            const unsigned long long t2 = now();
            float d = mine ? pq_sum(c) : 0.f;
            if (stats) asm volatile("" : "+v"(d));
            const unsigned long long t3 = now();
            offer(mine, nb, d);
            if (stats) {
                const unsigned long long t4 = now();
                t_rec += t1 - t0, t_visit += t2 - t1, t_sum += t3 - t2, t_offer += t4 - t3;
            }
        }
    } else {
        for (;;) {
            uint32_t node = 0, second = kEmpty;
            if (!pick_next(node, second)) break;
            const uint32_t *ll = links + (int64_t)node * (links_per_node + 1);
            const uint32_t cnt = ll[0];
            ++n_expand;
            bool mine = false;
            uint32_t nb = 0;
            float d = 0.f;
            for (uint32_t base = 0; base < cnt; base += 64) {  // (links_per_node <= 64 in practice: one round)
                mine = base + lane < cnt;
                nb = mine ? ll[1 + base + lane] : 0u;
                mine = mine && (int64_t)nb < N && visit(nb);
                n_eval += (unsigned int)__popcll(__ballot(mine));
                d = mine ? pq_lookup(nb) : 0.f;
                offer(mine, nb, d);
            }
        }
    }
}

// the eight counters of a walk, summed into `stats` (annlite_graph_search_stats_ex)
__device__ __forceinline__ void pq_walk_add_stats(unsigned long long *stats, const PQWalkCounters &ct) {
    atomicAdd(stats + 0, (unsigned long long)ct.n_expand);
    atomicAdd(stats + 1, (unsigned long long)ct.n_eval);
    atomicAdd(stats + 2, (unsigned long long)ct.n_hit);
    atomicAdd(stats + 3, ct.t_seed), atomicAdd(stats + 4, ct.t_rec), atomicAdd(stats + 5, ct.t_visit), atomicAdd(stats + 6, ct.t_sum), atomicAdd(stats + 7, ct.t_offer);
}

// host side, graph.hip: the walk's argument checks (n_seeds, M, Ks, record size, expansion width) and what a launch needs beside
// its lists (beside graph_beam.h's graph_walk_hash_bits) -- the debug counters' buffer (NULL unless ANNLITE_DEBUG_COUNTERS), zeroed
// on `st`.
int graph_walk_check(bool packed, int links_per_node, int64_t n_seeds, int64_t N, int64_t M, int64_t Ks, int64_t B, int width);
int graph_walk_stats(hipStream_t st, unsigned long long **stats);

}  // namespace annlite
