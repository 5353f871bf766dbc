// graph_beam.h -- what a wave-per-query beam walk over level-0 link lists keeps, whatever its distance: the sorted list of the
// 64 E best nodes spread over the lanes' registers, its one-at-a-time and its merged insertion, the bucketed visited table in
// LDS and the pick of the next node to expand.  graph.hip (PQLookup sums from a per-query table in LDS) and graph_f32.hip (exact
// distances over float rows) walk with it.
#pragma once
#include "common.h"

namespace annlite {

constexpr uint32_t kEmpty = 0xffffffffu;

// sorted list of 64 * E entries across the lanes: entry i lives in lane i % 64, slot i / 64
template <int E>
struct BeamList {
    uint32_t hi[E], lo[E];  // ordered distance key, node id
    bool exp[E];            // expanded already
};

template <int E>
__device__ __forceinline__ void beam_insert(BeamList<E> &L, uint32_t chi, uint32_t clo, int lane) {
    // entries smaller than the candidate form a prefix of the list
    int pos = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) pos += __popcll(__ballot(key_less(L.hi[e], L.lo[e], chi, clo)));
    // shift entries [pos, end) up by one, dropping the last; entry i - 1 of slot e lane l is (e, l-1), or (e-1, 63) for l = 0
    uint32_t phi[E], plo[E];
    bool pex[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        phi[e] = __shfl_up(L.hi[e], 1);
        plo[e] = __shfl_up(L.lo[e], 1);
        pex[e] = __shfl_up((int)L.exp[e], 1) != 0;
    }
#pragma unroll
    for (int e = E - 1; e >= 1; --e) {
        const uint32_t bh = __builtin_amdgcn_readlane(L.hi[e - 1], 63), bl = __builtin_amdgcn_readlane(L.lo[e - 1], 63);
        const bool bx = __builtin_amdgcn_readlane((int)L.exp[e - 1], 63) != 0;
        if (lane == 0) {
            phi[e] = bh;
            plo[e] = bl;
            pex[e] = bx;
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int idx = e * 64 + lane;
        if (idx == pos) {
            L.hi[e] = chi;
            L.lo[e] = clo;
            L.exp[e] = false;
        } else if (idx > pos) {
            L.hi[e] = phi[e];
            L.lo[e] = plo[e];
            L.exp[e] = pex[e];
        }
    }
}

// One wave's walk state.  BATCH: the neighbours of an expansion that beat the list's worst entry are MERGED into the sorted list
// in one pass through the per-wave LDS scratch `s_mrg` (u32 [3][64 E]: keys, ids, expanded flags; then u32 [4][64]: the
// candidates compacted and by rank); BATCH = false keeps the one-at-a-time insertion.  `hash_ad`: LDS byte address of the
// visited table, 1 << hash_bits u32 entries set to kEmpty by the caller.
template <int E, bool BATCH>
struct Beam {
    BeamList<E> L;
    int lane, cap;          // entries beyond `cap` = min(ef, 64 E) are ignored at the end
    uint32_t *s_mrg;
    uint32_t hash_ad, hash_n;
    int hash_bits;
    bool tbl_ovf;   // this lane has met a full stretch of the visited table
    bool tbl_full;  // ... some lane of the wave has (wave-uniform, sticky)

    __device__ __forceinline__ void init(int lane_, int ef, uint32_t *s_mrg_, uint32_t hash_ad_, int hash_bits_) {
        lane = lane_;
        s_mrg = s_mrg_;
        hash_ad = hash_ad_;
        hash_bits = hash_bits_;
        hash_n = 1u << hash_bits_;
        tbl_ovf = false;
        tbl_full = false;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            L.hi[e] = kKeyInfHi;
            L.lo[e] = kIdNone;
            L.exp[e] = true;  // empty slots are never picked
        }
        cap = ef < 64 * E ? ef : 64 * E;
    }

    // true if the node was not seen before (it is recorded now).  A (nearly) full table cannot record any more: the
    // node is then reported as new every time -- evaluated again, never lost -- and `offer` keeps it out of the list
    // if it is already there, so a walk that outgrows the table only gets slower, not worse.
    // BUCKETS of four entries (round 5): one 16-byte read shows a bucket, the node is looked for in it and, if there is room,
    // claimed with ONE compare-and-swap.  (One entry per probe: at the end of a 5M-row walk the 4096-entry table holds ~2600
    // nodes and the slowest of an expansion's 32 lanes needed a dozen dependent LDS round trips.)
    // (by LDS byte address in the LDS address space: through a generic volatile pointer the bucket read was a FLAT load, and a flat
    // load counts on the vector-memory counter too -- every probe then waited for the prefetched record)
    __device__ __forceinline__ bool visit(uint32_t node) {
        const uint32_t n_buckets = hash_n >> 2;
        uint32_t bk = ((node * 2654435761u) >> (32 - hash_bits)) >> 2;
        for (uint32_t probe = 0; probe < 16; ++probe) {
            const u32x4 v = *(volatile __attribute__((address_space(3))) u32x4 *)(uintptr_t)(hash_ad + 16u * bk);
            if (v.x == node || v.y == node || v.z == node || v.w == node) return false;
            const int slot = v.x == kEmpty ? 0 : v.y == kEmpty ? 1 : v.z == kEmpty ? 2 : v.w == kEmpty ? 3 : -1;
            if (slot >= 0) {
                uint32_t old = kEmpty;  // (expected; the call leaves what it found here)
                __hip_atomic_compare_exchange_strong((__attribute__((address_space(3))) uint32_t *)(uintptr_t)(hash_ad + 16u * bk + 4u * (uint32_t)slot),
                                                     &old, node, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (old == kEmpty) return true;
                if (old == node) return false;
                continue;  // (another lane of this expansion took the slot: look at the bucket again)
            }
            bk = (bk + 1) & (n_buckets - 1);
        }
        tbl_ovf = true;  // (no room within 16 buckets: from now on a node can be evaluated twice -- the merge checks for duplicates)
        return true;
    }

    __device__ __forceinline__ void worst(uint32_t &whi, uint32_t &wlo) const {
        const int i = cap - 1;
        whi = kKeyInfHi;
        wlo = kIdNone;
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (i / 64 == e) {
                whi = __builtin_amdgcn_readlane(L.hi[e], i % 64);
                wlo = __builtin_amdgcn_readlane(L.lo[e], i % 64);
            }
    }

    // the lanes with `mine` offer (key `khi`, id `node`); those that beat the list's worst entry AS IT IS NOW are inserted
    __device__ __forceinline__ void offer(bool mine, uint32_t node, uint32_t khi) {
        uint32_t whi, wlo;
        worst(whi, wlo);
        unsigned long long pm = __ballot(mine && key_less(khi, node, whi, wlo));
        if constexpr (!BATCH) {
            while (pm) {
                const int src = __builtin_ctzll(pm);
                pm &= pm - 1;
                const uint32_t chi = __builtin_amdgcn_readlane(khi, src), clo = __builtin_amdgcn_readlane(node, src);
                worst(whi, wlo);
                bool dup = false;
#pragma unroll
                for (int e = 0; e < E; ++e) dup = dup || __ballot(L.lo[e] == clo && L.hi[e] == chi) != 0ull;
                if (!dup && key_less(chi, clo, whi, wlo)) beam_insert<E>(L, chi, clo, lane);
            }
        } else {
            if (!pm) return;
            // FAST PATH: ranks by counting, no wave-wide vote per candidate.  The candidates' keys go to the LDS compacted; every
            // lane reads them back one by one (same address in all lanes: a broadcast) and counts -- a list entry the candidates
            // below it (its shift), a candidate lane the candidates below its own key (its rank r).  Entries move to position +
            // shift through the scratch; the positions nobody moved to are the candidates', in rank order: the h-th hole takes
            // the candidate of rank h.  A candidate equal to a list entry or to another candidate (only when the visited table
            // is full) sends the whole expansion down the careful path below.
            {
                uint32_t *cu_hi = s_mrg + 192 * E, *cu_lo = cu_hi + 64, *cs_hi = cu_hi + 128, *cs_lo = cu_hi + 192;
                const bool in = ((pm >> lane) & 1ull) != 0;
                const int n = __popcll(pm);
                const int myidx = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(pm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pm, 0u));
                if (in) cu_hi[myidx] = khi, cu_lo[myidx] = node;
                // (LANES talk to each other through the scratch: the compiler, which sees one thread, must not forward a lane's own
                // store to its later load of the same address -- another lane may have written there in between)
                asm volatile("" ::: "memory");
                int shift[E];
#pragma unroll
                for (int e = 0; e < E; ++e) shift[e] = 0;
                int r = 0;
                bool bad = false;
                // (duplicates exist only once the visited table has overflowed: until then the equality tests are left out)
                if (!tbl_full && __ballot(tbl_ovf)) tbl_full = true;
                if (tbl_full) {
#pragma unroll 2
                    for (int j = 0; j < n; ++j) {
                        const uint32_t chi = cu_hi[j], clo = cu_lo[j];
#pragma unroll
                        for (int e = 0; e < E; ++e) {
                            shift[e] += key_less(chi, clo, L.hi[e], L.lo[e]) ? 1 : 0;
                            bad = bad || (chi == L.hi[e] && clo == L.lo[e]);
                        }
                        r += (in && key_less(chi, clo, khi, node)) ? 1 : 0;
                        bad = bad || (in && j != myidx && chi == khi && clo == node);
                    }
                } else {
#pragma unroll 2
                    for (int j = 0; j < n; ++j) {
                        const uint32_t chi = cu_hi[j], clo = cu_lo[j];
#pragma unroll
                        for (int e = 0; e < E; ++e) shift[e] += key_less(chi, clo, L.hi[e], L.lo[e]) ? 1 : 0;
                        r += (in && key_less(chi, clo, khi, node)) ? 1 : 0;
                    }
                }
                if (!__ballot(bad)) {
                    if (in) cs_hi[r] = khi, cs_lo[r] = node;
#pragma unroll
                    for (int e = 0; e < E; ++e) s_mrg[128 * E + e * 64 + lane] = 2u;  // "nobody moved here"
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const int np = e * 64 + lane + shift[e];
                        if (np < 64 * E) {
                            s_mrg[np] = L.hi[e];
                            s_mrg[64 * E + np] = L.lo[e];
                            s_mrg[128 * E + np] = L.exp[e] ? 1u : 0u;
                        }
                    }
                    asm volatile("" ::: "memory");
                    int hbase = 0;
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const int P = e * 64 + lane;
                        const uint32_t x = s_mrg[128 * E + P];
                        uint32_t nhi = s_mrg[P], nlo = s_mrg[64 * E + P];
                        const bool hole = x == 2u;
                        const unsigned long long hm = __ballot(hole);
                        if (hole) {
                            const int h = hbase + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(hm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hm, 0u));
                            nhi = cs_hi[h];
                            nlo = cs_lo[h];
                        }
                        L.hi[e] = nhi;
                        L.lo[e] = nlo;
                        L.exp[e] = !hole && x != 0u;
                        hbase += __popcll(hm);
                    }
                    return;
                }
            }
            // CAREFUL PATH (a duplicate somewhere): one pass over the candidates with wave-wide votes.
            // (wave-uniform: their keys are broadcast): a list entry counts the candidates below
            // it, a candidate lane the list entries and the other candidates below its key.  A candidate that is already in the
            // list, or equals an earlier candidate (both only when the visited table is full: see visit), is dropped --
            // what the one-at-a-time insertion's duplicate check does.
            int shift[E];
#pragma unroll
            for (int e = 0; e < E; ++e) shift[e] = 0;
            int mypos = 0;
            bool in = ((pm >> lane) & 1ull) != 0;
            unsigned long long rem = pm;
            while (rem) {
                const int src = __builtin_ctzll(rem);
                rem &= rem - 1;
                const uint32_t chi = __builtin_amdgcn_readlane(khi, src), clo = __builtin_amdgcn_readlane(node, src);
                bool dup = false;
#pragma unroll
                for (int e = 0; e < E; ++e) dup = dup || __ballot(L.lo[e] == clo && L.hi[e] == chi) != 0ull;
                if (dup) {
                    if (lane == src) in = false;
                    continue;
                }
                const unsigned long long same = __ballot(in && lane > src && khi == chi && node == clo) & rem;
                if (same) {
                    if ((same >> lane) & 1ull) in = false;
                    rem &= ~same;
                }
                int below = 0;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const bool lt = key_less(L.hi[e], L.lo[e], chi, clo);  // entry < candidate (never equal: see above)
                    below += __popcll(__ballot(lt));
                    shift[e] += lt ? 0 : 1;
                }
                if (lane == src) mypos += below;
                else if (in && key_less(chi, clo, khi, node)) mypos += 1;
            }
            // every element of (list + kept candidates) now knows its rank in the union: the first 64 E go back into the list
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int np = e * 64 + lane + shift[e];
                if (np < 64 * E) {
                    s_mrg[np] = L.hi[e];
                    s_mrg[64 * E + np] = L.lo[e];
                    s_mrg[128 * E + np] = L.exp[e] ? 1u : 0u;
                }
            }
            if (in && mypos < 64 * E) {
                s_mrg[mypos] = khi;
                s_mrg[64 * E + mypos] = node;
                s_mrg[128 * E + mypos] = 0u;
            }
            asm volatile("" ::: "memory");  // (see the fast path: no store-to-load forwarding across lanes)
            // (one wave: its LDS writes are visible to its own later reads in program order)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                L.hi[e] = s_mrg[e * 64 + lane];
                L.lo[e] = s_mrg[64 * E + e * 64 + lane];
                L.exp[e] = s_mrg[128 * E + e * 64 + lane] != 0u;
            }
        }
    }

    // the best unexpanded entry of the list (marked expanded) and -- `second` -- the next best one, unmarked: the prefetch target
    __device__ __forceinline__ bool pick_next(uint32_t &node, uint32_t &second) {
        int p0 = -1, p1 = -1;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (p1 < 0) {
                unsigned long long m = __ballot(!L.exp[e] && (e * 64 + lane) < cap);
                if (m && p0 < 0) {
                    p0 = e * 64 + __builtin_ctzll(m);
                    m &= m - 1;
                }
                if (m && p0 >= 0) p1 = e * 64 + __builtin_ctzll(m);
            }
        }
        if (p0 < 0) return false;
        node = 0;
        second = kEmpty;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (p0 / 64 == e) {
                node = __builtin_amdgcn_readlane(L.lo[e], p0 % 64);
                if (lane == p0 % 64) L.exp[e] = true;
            }
            if (p1 >= 0 && p1 / 64 == e) second = __builtin_amdgcn_readlane(L.lo[e], p1 % 64);
        }
        return true;
    }
};

// row `b` of a walk's result: the list's first `ef` places, ascending; the places beyond `cap`, the empty ones and the rows cleared
// in `valid` (NULL: none is) blanked in place to (-1, +inf) -- such rows still route the walk, like hnswlib's; compacting is left to
// the host-side top-k
template <int E, bool BATCH>
__device__ __forceinline__ void beam_write(const Beam<E, BATCH> &bm, int b, int ef, const uint32_t *__restrict__ valid,
                                           int64_t *__restrict__ out_ids, float *__restrict__ out_dist) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = e * 64 + bm.lane;
        if (i < ef) {
            bool none = (bm.L.hi[e] == kKeyInfHi && bm.L.lo[e] == kIdNone) || i >= bm.cap;
            if (!none && valid) none = !((valid[bm.L.lo[e] >> 5] >> (bm.L.lo[e] & 31)) & 1u);
            out_ids[(int64_t)b * ef + i] = none ? (int64_t)-1 : (int64_t)bm.L.lo[e];
            out_dist[(int64_t)b * ef + i] = none ? __builtin_inff() : ordered_to_f32(bm.L.hi[e]);
        }
    }
}

// The ADMITTED-RESULT list of a filtered walk (graph_admit.hip over PQ codes, graph_f32.hip over float rows).  Such a walk keeps TWO
// sorted lists.  C (Beam<E>, cap = ef_route) is the plain walk's list and is handled exactly as there: the bitmap `admit` (valid &
// filter, one bit per row) never touches it, so the expansions and the rows evaluated are the plain walk's at ef = ef_route.  R (this
// struct: Beam<ER>, cap = ef <= ef_route; its expanded flags and visited table are never used) is offered every batch C is offered --
// a seed round, a step's unseen neighbours -- restricted to the lanes whose node is set in `admit`, under the same rule: tested
// against R's worst entry as it is now, whatever C's worst entry is, then merged.  Order: (key, id), C's own key.
// INVARIANT: R's live entries are the ef smallest (key, id) among the admitted rows the walk evaluated.
// A row can be offered to R twice, and R's merge then has to drop the copy (`tbl_full`: the merge's equality tests).  Two ways:
//   * the visited table overflowed (Beam::visit): C's overflow state is carried into R before every offer -- R never calls visit;
//   * a seed that missed C's list is not recorded as visited (only C's entries are) and may stand in R: it comes back as somebody's
//     neighbour.  That takes more seeds than C has places -- a host-built graph exports up to 4096 -- so R checks from the start
//     iff n_seeds > min(ef_route, 64 E).
// A re-offered row that is NOT in R lost against R's worst entry before, or was pushed out, and the worst entry only falls: it loses
// again (tests/test_graph_pq_admit_restated.py, tests/test_graph_f32_admit_restated.py).  R shares C's merge scratch: ER <= E, and
// the two offers of a wave are sequential.
template <int E, int ER>
struct AdmitList {
    static_assert(ER <= E, "R's merge layout has to fit the scratch sized for C");
    Beam<ER, true> rs;
    const uint32_t *admit;

    // after C's own init
    __device__ __forceinline__ void init(const Beam<E, true> &bm, int ef, int n_seeds, const uint32_t *admit_) {
        admit = admit_;
        rs.init(bm.lane, ef, bm.s_mrg, bm.hash_ad, bm.hash_bits);
        rs.tbl_full = n_seeds > bm.cap;
    }

    // both lists are offered one batch; `mine` lanes hold a node < N.  (The lambda a kernel wraps this in is marked always_inline: left
    // to the inliner's size estimate it stays a call once a list has three or four registers per lane, and both lists then live in
    // scratch memory.)
    __device__ __forceinline__ void offer_both(Beam<E, true> &bm, bool mine, uint32_t node, uint32_t key) {
        const uint32_t word = mine ? admit[node >> 5] : 0u;  // (only a row's own word is read)
        const bool adm = ((word >> (node & 31)) & 1u) != 0u;
        bm.offer(mine, node, key);
        asm volatile("" ::: "memory");  // (C's last reads of the scratch stay ahead of R's first writes)
        rs.tbl_ovf = bm.tbl_ovf;
        rs.offer(adm, node, key);
        asm volatile("" ::: "memory");
    }

    // R, ascending; it holds admitted rows only, so the missing places are all at the tail
    __device__ __forceinline__ void write(int b, int ef, int64_t *__restrict__ out_ids, float *__restrict__ out_dist) const {
        beam_write(rs, b, ef, nullptr, out_ids, out_dist);
    }

    // how far the walk reached: the key's value at C's last place (+inf while C is not full).  An entry of R at or below it lies where
    // the walk looked as closely as the plain walk at ef_route does; one beyond it was only met on the way (the caller's convergence
    // test).  `out` may be NULL.
    __device__ __forceinline__ void write_route_worst(const Beam<E, true> &bm, int b, float *__restrict__ out) const {
        if (!out) return;
        uint32_t whi, wlo;
        bm.worst(whi, wlo);
        if (bm.lane == 0) out[b] = whi == kKeyInfHi && wlo == kIdNone ? __builtin_inff() : ordered_to_f32(whi);
    }
};

// host side, graph.hip: entries of the visited table (log2) beside a routing list of `ef` places, whatever the walk's distance
int graph_walk_hash_bits(int ef);

}  // namespace annlite
