// graph_f32.hip -- the level-0 graph over FLOAT vectors: walked (annlite_graph_f32_search) and built (annlite_graph_f32_build_select /
// annlite_graph_f32_build_reverse) on the GPU.  The float forms of graph.hip's plain walk and of graph_build.hip's two kernels: same
// link lists (u32 [N][L + 1]: count, ids), same seeds, same list / visited table / merge (graph_beam.h), same selection rules, same
// pairs / keys / seg formats.  What differs is the distance.
//
// ONE distance: every number compared here -- query to row in the walk, row to row in the build -- is annlite_exact_gather_dist's for
// the metric, bit for bit: 64 lane-strided fmaf chains (j = lane, lane + 64, ...) over d = x[j] - q[j] (EUCLIDEAN) or x[j] * q[j]
// (INNER_PRODUCT, COSINE: 1 - sum), then the xor butterfly 32 .. 1.  rows_dist below is rerank_topk_kernel's loop (codec.hip): the
// rows of up to eight lanes in flight, one row per wave-wide pass.  The walk's list therefore carries final distances (no re-rank
// launch), a stored vector finds itself at exactly 0.0 and the arithmetic is symmetric in its two arguments (d * d = (-d) * (-d),
// x * q = q * x; the butterfly's adds commute).
//
// Walk: one wave per query.  Per-wave LDS is the query (D * 4 B), the visited table (16 KB up to ef = 208, 32 KB beyond) and the
// merge scratch (768 E + 1024 B): 19 KB at D = 128, ef <= 128 -- eight waves per CU, two per SIMD, where the PQ walk's 16 KB look-up
// table leaves room for four or five.  An expansion reads the node's link list (one 4 (L + 1)-byte row; the list of the runner-up is
// requested a step ahead) and gathers the rows of its unseen neighbours: up to L rows of D * 4 B, eight in flight.
#include "scan_common.h"
#include "graph_beam.h"

namespace annlite {

constexpr int kRowsInFlight = 8;  // rerank_topk_kernel's U

// Distance of `qv` f32 [D] (LDS or global, wave-uniform pointer) to the rows x[node] of the lanes in `pm` (node: per lane, < N);
// a lane of `pm` returns its row's distance, every other lane 0.  Wave-uniform control flow.
template <bool L2>
__device__ __forceinline__ float rows_dist(unsigned long long pm, uint32_t node, const float *__restrict__ x, int D, const float *qv,
                                           int lane) {
    constexpr int U = kRowsInFlight;
    float mine = 0.f;
    while (pm) {
        int src[U];
        bool on[U];
        const float *xr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            on[u] = pm != 0ull;
            src[u] = on[u] ? __builtin_ctzll(pm) : 0;
            pm &= pm - 1;  // (0 stays 0)
            xr[u] = x + (int64_t)__builtin_amdgcn_readlane(node, src[u]) * D;  // (wave-uniform)
        }
        float s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) s[u] = 0.f;
        for (int j = lane; j < D; j += 64) {
            const float qj = qv[j];
            float xv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) xv[u] = on[u] ? xr[u][j] : 0.f;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if constexpr (L2) {
                    const float d = xv[u] - qj;
                    s[u] = __builtin_fmaf(d, d, s[u]);
                } else {
                    s[u] = __builtin_fmaf(xv[u], qj, s[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (on[u]) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s[u] += __shfl_xor(s[u], o);
                if (lane == src[u]) mine = L2 ? s[u] : 1.f - s[u];
            }
        }
    }
    return mine;
}

// ---- walk ---------------------------------------------------------------------------------------------------------------------
// ONE COPY for the two kernels below, in the shape of graph_pq_walk.h's: a kernel sets its wave up with f32_walk_setup, then calls
// f32_beam_walk with what is to happen to every batch of evaluated rows as `offer(mine, node, key)`.
// The order of graph_beam_search_kernel<.., PACKED = false, BATCH = true> (tests/test_graph_pair.py walk_restated, width 1): seeds
// scanned flat in rounds of 64, the best unexpanded entry expanded, a step's unseen neighbours (ids < N) tested against the list's
// worst entry before any is inserted, the list ordered by (f32_to_key(distance), node id) -- NaN behind +inf --, the walk over when
// the first min(ef, 64 E) entries hold no unexpanded node.

// LDS of one walking wave: the query (padded to 16 B), the visited table, the merge's scratch of a list of E registers per lane
__host__ __device__ inline size_t f32_walk_lds_per_wave(int E, int D, int hash_bits) {
    return (((size_t)D * 4 + 15) & ~(size_t)15) + ((size_t)4 << hash_bits) + (size_t)E * 64 * 12 + 1024;
}

// The wave's query and visited table filled, its list `bm` (cap = ef) empty; `s_q`: the query.
template <int E>
__device__ __forceinline__ void f32_walk_setup(unsigned char *smem, int wave, int lane, const float *__restrict__ q, int b, int D, int ef,
                                               int hash_bits, Beam<E, true> &bm, const float *&s_q) {
    const uint32_t hash_n = 1u << hash_bits;
    const size_t q_bytes = ((size_t)D * 4 + 15) & ~(size_t)15;
    const size_t per_wave = f32_walk_lds_per_wave(E, D, hash_bits);
    float *s_qw = (float *)(smem + wave * per_wave);
    uint32_t *s_hash = (uint32_t *)(smem + wave * per_wave + q_bytes);
    uint32_t *s_mrg = s_hash + hash_n;
    for (int j = lane; j < D; j += 64) s_qw[j] = q[(int64_t)b * D + j];
    for (uint32_t i = lane; i < hash_n / 4; i += 64) ((u32x4 *)s_hash)[i] = (u32x4){kEmpty, kEmpty, kEmpty, kEmpty};
    asm volatile("" ::: "memory");  // (one wave: its LDS writes are visible to its own later reads in program order)
    typedef __attribute__((address_space(3))) unsigned char *lds_bytes;
    const uint32_t hash_ad = (uint32_t)(uintptr_t)(lds_bytes)smem + (uint32_t)(wave * per_wave) + (uint32_t)q_bytes;
    bm.init(lane, ef, s_mrg, hash_ad, hash_bits);
    s_q = s_qw;
}

// Seeds, then the walk, until `bm`'s list holds no unexpanded node.  ANNLITE_DEBUG_COUNTERS: `n_expand` link lists read, `n_eval`
// rows evaluated.
template <int E, bool L2, class Offer>
__device__ __forceinline__ void f32_beam_walk(Beam<E, true> &bm, const float *s_q, int lane, const float *__restrict__ x, int D, int64_t N,
                                              const uint32_t *__restrict__ links, int lpn, const uint32_t *__restrict__ seeds, int n_seeds,
                                              Offer &&offer, unsigned int &n_expand, unsigned int &n_eval) {
    // ---- seeds, scanned flat (distinct: no visited check; only the ones that made the list are recorded) ----
    for (int s0 = 0; s0 < n_seeds; s0 += 64) {
        const uint32_t node = s0 + lane < n_seeds ? seeds[s0 + lane] : kEmpty;
        const bool mine = s0 + lane < n_seeds && (int64_t)node < N;
        const unsigned long long pm = __ballot(mine);
        const float d = rows_dist<L2>(pm, node, x, D, s_q, lane);
        n_eval += (unsigned int)__popcll(pm);
        offer(mine, node, f32_to_key(d));
    }
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (bm.L.lo[e] != kIdNone) bm.visit(bm.L.lo[e]);

    // ---- walk: lane j holds slot j of a link list (slots beyond the count: never read as neighbours) ----
    auto load_list = [&](uint32_t node, uint32_t &cnt, uint32_t &nb) {
        const uint32_t *ll = links + (int64_t)node * (lpn + 1);
        cnt = ll[0];
        nb = lane < lpn ? ll[1 + lane] : kEmpty;
    };
    uint32_t pf_node = kEmpty, pf_cnt = 0, pf_nb = kEmpty;  // the list of the runner-up, requested a step ahead
    for (;;) {
        uint32_t node = 0, second = kEmpty;
        if (!bm.pick_next(node, second)) break;
        uint32_t cnt, nb;
        if (pf_node == node) {
            cnt = pf_cnt;
            nb = pf_nb;
        } else {
            load_list(node, cnt, nb);
        }
        pf_node = second;
        if (second != kEmpty) load_list(second, pf_cnt, pf_nb);
        ++n_expand;
        bool mine = lane < lpn && (uint32_t)lane < cnt;
        mine = mine && (int64_t)nb < N && bm.visit(nb);
        const unsigned long long pm = __ballot(mine);
        const float d = rows_dist<L2>(pm, nb, x, D, s_q, lane);
        n_eval += (unsigned int)__popcll(pm);
        offer(mine, nb, f32_to_key(d));
    }
}

__device__ __forceinline__ void f32_walk_add_stats(unsigned long long *stats, int lane, unsigned int n_expand, unsigned int n_eval) {
    if (stats && lane == 0) {
        atomicAdd(stats + 0, (unsigned long long)n_expand);
        atomicAdd(stats + 1, (unsigned long long)n_eval);
    }
}

// annlite_graph_f32_search: one list; rows cleared in `valid` route the walk and are blanked on output
template <int E, bool L2>
__global__ __launch_bounds__(256) void graph_f32_search_kernel(const float *__restrict__ q, int B, int D, const float *__restrict__ x,
                                                              int64_t N, const uint32_t *__restrict__ links, int lpn,
                                                              const uint32_t *__restrict__ seeds, int n_seeds,
                                                              const uint32_t *__restrict__ valid, int ef, int hash_bits,
                                                              int64_t *__restrict__ out_ids, float *__restrict__ out_dist,
                                                              unsigned long long *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.x * (blockDim.x >> 6) + wave;
    if (b >= B) return;  // (whole waves leave; no block-wide barrier below)
    unsigned int n_expand = 0, n_eval = 0;
    Beam<E, true> bm;
    const float *s_q;
    f32_walk_setup<E>(smem, wave, lane, q, b, D, ef, hash_bits, bm, s_q);
    auto offer = [&](bool mine, uint32_t node, uint32_t key) __attribute__((always_inline)) { bm.offer(mine, node, key); };
    f32_beam_walk<E, L2>(bm, s_q, lane, x, D, N, links, lpn, seeds, n_seeds, offer, n_expand, n_eval);
    beam_write(bm, b, ef, valid, out_ids, out_dist);
    f32_walk_add_stats(stats, lane, n_expand, n_eval);
}

// annlite_graph_f32_search_admit: the walk above at ef = ef_route -- same expansions, same rows evaluated -- with graph_beam.h's
// admitted-result list beside it.  Key: (f32_to_key(distance), id), the float walk's own.
template <int E, int ER, bool L2>
__global__ __launch_bounds__(256) void graph_f32_admit_kernel(const float *__restrict__ q, int B, int D, const float *__restrict__ x,
                                                             int64_t N, const uint32_t *__restrict__ links, int lpn,
                                                             const uint32_t *__restrict__ seeds, int n_seeds,
                                                             const uint32_t *__restrict__ admit, int ef_route, int ef, int hash_bits,
                                                             int64_t *__restrict__ out_ids, float *__restrict__ out_dist,
                                                             float *__restrict__ out_route_worst,
                                                             unsigned long long *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.x * (blockDim.x >> 6) + wave;
    if (b >= B) return;  // (whole waves leave; no block-wide barrier below)
    unsigned int n_expand = 0, n_eval = 0;
    Beam<E, true> bm;
    const float *s_q;
    f32_walk_setup<E>(smem, wave, lane, q, b, D, ef_route, hash_bits, bm, s_q);
    AdmitList<E, ER> rl;
    rl.init(bm, ef, n_seeds, admit);
    auto offer_both = [&](bool mine, uint32_t node, uint32_t key) __attribute__((always_inline)) { rl.offer_both(bm, mine, node, key); };
    f32_beam_walk<E, L2>(bm, s_q, lane, x, D, N, links, lpn, seeds, n_seeds, offer_both, n_expand, n_eval);
    rl.write(b, ef, out_ids, out_dist);
    rl.write_route_worst(bm, b, out_route_worst);
    f32_walk_add_stats(stats, lane, n_expand, n_eval);
}

// ---- build --------------------------------------------------------------------------------------------------------------------
constexpr int kPoolMaxF32 = 256;

// Algorithm 4 over a pool that is ALREADY in the order it is to be visited (LDS: s_id / s_tb = id, distance to the base point of
// entry t; id 0xffffffff = skip): a candidate is kept only if no kept neighbour is strictly closer to it than the base point is.
// Lane j < n_kept holds the j-th kept neighbour's id; a candidate's test against all of them is one rows_dist with the candidate's
// row as the common argument.  Wave-uniform control flow.
template <bool L2>
__device__ __forceinline__ void heuristic_select_f32(const float *__restrict__ x, int D, const uint32_t *s_id, const float *s_tb,
                                                     int n_pool, int m_max, int lane, uint32_t &kept_id, int &n_kept) {
    kept_id = 0xffffffffu;
    n_kept = 0;
    for (int t = 0; t < n_pool && n_kept < m_max; ++t) {
        const uint32_t id = s_id[t];
        if (id == 0xffffffffu) continue;
        const float tb = s_tb[t];
        bool closer_to_kept = false;
        if (n_kept) {
            const unsigned long long pm = n_kept >= 64 ? ~0ull : ((1ull << n_kept) - 1ull);
            const float dk = rows_dist<L2>(pm, kept_id, x, D, x + (int64_t)id * D, lane);
            closer_to_kept = lane < n_kept && dk < tb;
        }
        if (__ballot(closer_to_kept) == 0ull) {
            if (lane == n_kept) kept_id = id;
            ++n_kept;
        }
    }
}

// cand i64 [b][ef]: the candidates of point i = node base0 + i in the order they are to be visited (-1 = none; the point itself and
// ids beyond the table are skipped).  links row base0 + i <- (count, ids); pairs i64 [b][m_keep] <- (target << 32) | source,
// INT64_MAX = none.  (graph_select_kernel with vectors[a], vectors[b] in the place of the code rows.)
template <bool L2>
__global__ __launch_bounds__(256) void graph_f32_select_kernel(const int64_t *__restrict__ cand, int ef, int64_t b, int64_t base0,
                                                              const float *__restrict__ x, int64_t N, int D, int m_keep,
                                                              uint32_t *__restrict__ links, int lpn, int64_t *__restrict__ pairs) {
    __shared__ uint32_t s_all[4][kPoolMaxF32 * 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= b) return;
    uint32_t *s_id = s_all[wave];
    float *s_tb = (float *)(s_id + kPoolMaxF32);
    const uint32_t base = (uint32_t)(base0 + i);
    const float *xb = x + (int64_t)base * D;
    int n_real = 0;
    for (int t0 = 0; t0 < ef; t0 += 64) {
        const int t = t0 + lane;
        const int64_t id = t < ef ? cand[i * ef + t] : -1;
        const bool ok = id >= 0 && id < N && (uint32_t)id != base;
        const unsigned long long pm = __ballot(ok);
        const float d = rows_dist<L2>(pm, ok ? (uint32_t)id : 0u, x, D, xb, lane);
        if (t < ef) {
            s_id[t] = ok ? (uint32_t)id : 0xffffffffu;
            s_tb[t] = d;
        }
        n_real += __popcll(pm);
    }
    asm volatile("" ::: "memory");  // (lanes read each other's LDS stores below: one wave, program order)
    uint32_t kept_id = 0xffffffffu;
    int n_kept = 0;
    if (n_real <= m_keep) {  // a pool that fits is kept whole: the real entries compacted into the lanes in list order
        int basecnt = 0;
        for (int t0 = 0; t0 < ef; t0 += 64) {
            const int t = t0 + lane;
            const uint32_t id = t < ef ? s_id[t] : 0xffffffffu;
            const unsigned long long m = __ballot(id != 0xffffffffu);
            const int mypos = basecnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (id != 0xffffffffu) s_tb[mypos] = __uint_as_float(id);  // (s_tb is free now: the ids, compacted)
            basecnt += __popcll(m);
        }
        asm volatile("" ::: "memory");
        n_kept = n_real;
        if (lane < n_kept) kept_id = __float_as_uint(s_tb[lane]);
    } else {
        heuristic_select_f32<L2>(x, D, s_id, s_tb, ef, m_keep, lane, kept_id, n_kept);
    }
    uint32_t *ll = links + (int64_t)base * (lpn + 1);
    if (lane == 0) ll[0] = (uint32_t)n_kept;
    if (lane < lpn) ll[1 + lane] = lane < n_kept ? kept_id : 0u;
    if (lane < m_keep)
        pairs[i * m_keep + lane] = lane < n_kept ? (int64_t)(((uint64_t)kept_id << 32) | (uint64_t)base) : (int64_t)0x7fffffffffffffffll;
}

// keys i64 [P] ascending: (target << 32) | source; seg i64 [S + 1]: segment s = keys[seg[s] .. seg[s+1]) all share one target.
// (graph_reverse_kernel with the float distance; the pool is ordered by (f32_to_key(distance to the target), id).)
template <bool L2>
__global__ __launch_bounds__(256) void graph_f32_reverse_kernel(const int64_t *__restrict__ keys, const int64_t *__restrict__ seg, int64_t S,
                                                               const float *__restrict__ x, int64_t N, int D,
                                                               uint32_t *__restrict__ links, int lpn) {
    __shared__ uint32_t s_all[4][64 * 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t s = (int64_t)blockIdx.x * 4 + wave;
    if (s >= S) return;
    uint32_t *s_id = s_all[wave];
    float *s_tb = (float *)(s_id + 64);
    const int64_t k0 = seg[s], k1 = seg[s + 1];
    if (k1 <= k0) return;
    const uint32_t o = (uint32_t)((uint64_t)keys[k0] >> 32);
    if ((int64_t)o >= N) return;
    uint32_t *ll = links + (int64_t)o * (lpn + 1);
    int c = (int)ll[0];
    if (c > lpn) c = lpn;  // (<= 32)
    // pool: lanes [0, c) the list, lanes [c, c + k) the sources (as many as the 64 lanes hold), duplicates of the list dropped
    const int k = (int)((k1 - k0) < (int64_t)(64 - c) ? (k1 - k0) : (int64_t)(64 - c));
    uint32_t v = 0xffffffffu;
    if (lane < c) v = ll[1 + lane];
    else if (lane < c + k) v = (uint32_t)((uint64_t)keys[k0 + (lane - c)] & 0xffffffffull);
    bool dup = v == o || (lane >= c && (int64_t)v >= N);
    for (int j = 0; j < c; ++j) {
        const uint32_t e = __builtin_amdgcn_readlane(v, j);
        dup = dup || (lane >= c && lane < c + k && v == e);
    }
    if (dup && lane >= c) v = 0xffffffffu;
    const unsigned long long live = __ballot(v != 0xffffffffu);
    const int n_pool = __popcll(live);
    if (n_pool == c) return;  // (nothing new)
    if (n_pool <= lpn) {  // room: the surviving sources are appended behind the list
        const int pos = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(live >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)live, 0u));
        if (v != 0xffffffffu && lane >= c) ll[1 + pos] = v;
        if (lane == 0) ll[0] = (uint32_t)n_pool;
        return;
    }
    // shrink: the pool ordered by its distance to the target (ties: id), then the heuristic to lpn entries
    const unsigned long long in_table = __ballot(v != 0xffffffffu && (int64_t)v < N);
    float d = rows_dist<L2>(in_table, v, x, D, x + (int64_t)o * D, lane);
    if (!((in_table >> lane) & 1ull)) d = __builtin_inff();
    const uint32_t dk = v != 0xffffffffu ? f32_to_key(d) : 0xffffffffu;
    int rank = 0;
    for (int j = 0; j < 64; ++j) {
        const uint32_t ek = __builtin_amdgcn_readlane(dk, j), ex = __builtin_amdgcn_readlane(v, j);
        rank += (ek < dk || (ek == dk && (ex < v || (ex == v && j < lane)))) ? 1 : 0;
    }
    // (a list entry beyond the table -- none in a graph this file built -- is not a row: it cannot be kept)
    s_id[rank] = ((in_table >> lane) & 1ull) ? v : 0xffffffffu;  // (dead lanes: key and id 0xffffffff rank last, among themselves by lane)
    s_tb[rank] = d;
    asm volatile("" ::: "memory");
    uint32_t kept_id = 0xffffffffu;
    int n_kept = 0;
    heuristic_select_f32<L2>(x, D, s_id, s_tb, n_pool, lpn, lane, kept_id, n_kept);
    if (lane < lpn) ll[1 + lane] = lane < n_kept ? kept_id : 0u;
    if (lane == 0) ll[0] = (uint32_t)n_kept;
}

}  // namespace annlite

using namespace annlite;

static unsigned long long *g_graph_f32_stats = nullptr;  // debug only (ANNLITE_DEBUG_COUNTERS): leaked 16-byte device buffer

// *stats: the float walk's debug counters, zeroed on `st` (NULL unless ANNLITE_DEBUG_COUNTERS)
static int f32_walk_stats(hipStream_t st, unsigned long long **stats) {
    *stats = nullptr;
    if (knobs().debug_counters) {
        if (!g_graph_f32_stats) ANNLITE_HIP_TRY(hipMalloc((void **)&g_graph_f32_stats, 16));
        ANNLITE_HIP_TRY(hipMemsetAsync(g_graph_f32_stats, 0, 16, st));
        *stats = g_graph_f32_stats;
    }
    return ANNLITE_OK;
}

// what the two walks check alike, after their own checks on ef / ef_route / admit; a batch of B = 0 may come without pointers
static int f32_walk_check(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev, int64_t N,
                          const uint32_t *links_dev, int links_per_node, const uint32_t *seeds_dev, int64_t n_seeds,
                          const int64_t *out_ids_dev, const float *out_dist_dev) {
    ANNLITE_REQUIRE(metric >= 1 && metric <= 3, "bad metric %d", metric);
    ANNLITE_REQUIRE(D >= 1 && D <= 2048, "the float graph takes 1 <= D <= 2048 (D = %lld)", (long long)D);
    ANNLITE_REQUIRE(links_per_node >= 1 && links_per_node <= 64, "links_per_node in [1, 64] (%d)", links_per_node);
    ANNLITE_REQUIRE(n_seeds >= 1 && n_seeds < (1ll << 31) && N < (1ll << 32) - 1, "bad graph");
    if (B == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(B < (1ll << 31), "bad B");
    ANNLITE_REQUIRE(queries_dev && links_dev && seeds_dev && out_ids_dev && out_dist_dev && (N == 0 || vectors_dev), "null device pointer");
    return ANNLITE_OK;
}

// One wave per query of either walk kernel `fn` (`name`: for the launch's error message), whose list has E registers per lane.
// Waves per workgroup: the count (<= 4) that lets most waves share a CU's 160 KB -- 21 KB per wave (ef > 128) is one workgroup of
// four per CU but two of three.  (The filtered walk's R lives in registers and shares C's merge scratch: same LDS.)
template <class... KA, class... A>
static int launch_f32_walk(void (*fn)(KA...), const char *name, int E, int64_t B, int64_t D, int hash_bits, hipStream_t st, A... args) {
    const size_t per_wave = f32_walk_lds_per_wave(E, (int)D, hash_bits);
    const size_t lds_cu = (size_t)160 * 1024;
    int wpb = 0, best = 0;
    for (int w = 4; w >= 1; --w) {
        const int waves = (int)(lds_cu / (w * per_wave)) * w;
        if (waves > best) best = waves, wpb = w;
    }
    ANNLITE_REQUIRE(wpb >= 1, "query, visited table and merge scratch do not fit the LDS");
    const size_t lds = wpb * per_wave;
    ANNLITE_HIP_TRY(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fn, dim3((unsigned)((B + wpb - 1) / wpb)), dim3(wpb * 64), lds, st, args...);
    return launch_status(name);
}

extern "C" int annlite_graph_f32_search(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev, int64_t N,
                                        const uint32_t *links_dev, int links_per_node, const uint32_t *seeds_dev, int64_t n_seeds,
                                        const uint32_t *valid_bits_dev, int ef, int64_t *out_ids_dev, float *out_dist_dev, void *stream) {
    ANNLITE_REQUIRE(B >= 0 && N >= 0 && ef >= 1 && ef <= 256, "bad B=%lld N=%lld ef=%d (ef <= 256)", (long long)B, (long long)N, ef);
    if (int rc = f32_walk_check(metric, queries_dev, B, D, vectors_dev, N, links_dev, links_per_node, seeds_dev, n_seeds, out_ids_dev,
                                out_dist_dev))
        return rc;
    if (B == 0) return ANNLITE_OK;
    hipStream_t st = (hipStream_t)stream;
    const int hash_bits = graph_walk_hash_bits(ef);
    unsigned long long *stats = nullptr;
    if (int rc = f32_walk_stats(st, &stats)) return rc;
    const bool l2 = metric == ANNLITE_METRIC_EUCLIDEAN;
#define ANNLITE_WALK_ARGS B, D, hash_bits, st, queries_dev, (int)B, (int)D, vectors_dev, N, links_dev, links_per_node, seeds_dev, (int)n_seeds, \
                          valid_bits_dev, ef, hash_bits, out_ids_dev, out_dist_dev, stats
#define ANNLITE_WALK(EE)                                                                                   \
    (l2 ? launch_f32_walk(graph_f32_search_kernel<EE, true>, "graph_f32_search_kernel", EE, ANNLITE_WALK_ARGS) \
        : launch_f32_walk(graph_f32_search_kernel<EE, false>, "graph_f32_search_kernel", EE, ANNLITE_WALK_ARGS))
    if (ef <= 64) return ANNLITE_WALK(1);
    if (ef <= 128) return ANNLITE_WALK(2);
    return ANNLITE_WALK(4);
#undef ANNLITE_WALK
#undef ANNLITE_WALK_ARGS
}

extern "C" int annlite_graph_f32_search_admit(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev, int64_t N,
                                              const uint32_t *links_dev, int links_per_node, const uint32_t *seeds_dev, int64_t n_seeds,
                                              const uint32_t *admit_bits_dev, int ef_route, int ef, int64_t *out_ids_dev,
                                              float *out_dist_dev, float *out_route_worst_dev, void *stream) {
    ANNLITE_REQUIRE(B >= 0 && N >= 0 && ef >= 1 && ef <= ef_route && ef_route <= 256, "bad B=%lld N=%lld ef=%d ef_route=%d (ef <= ef_route <= 256)",
                    (long long)B, (long long)N, ef, ef_route);
    ANNLITE_REQUIRE(admit_bits_dev != nullptr, "admit_bits_dev is NULL (a walk without a filter is annlite_graph_f32_search)");
    if (int rc = f32_walk_check(metric, queries_dev, B, D, vectors_dev, N, links_dev, links_per_node, seeds_dev, n_seeds, out_ids_dev,
                                out_dist_dev))
        return rc;
    if (B == 0) return ANNLITE_OK;
    hipStream_t st = (hipStream_t)stream;
    const int hash_bits = graph_walk_hash_bits(ef_route);  // (annlite_graph_f32_search's table at ef = ef_route)
    unsigned long long *stats = nullptr;
    if (int rc = f32_walk_stats(st, &stats)) return rc;
    const bool l2 = metric == ANNLITE_METRIC_EUCLIDEAN;
#define ANNLITE_WALK_ARGS B, D, hash_bits, st, queries_dev, (int)B, (int)D, vectors_dev, N, links_dev, links_per_node, seeds_dev, (int)n_seeds, \
                          admit_bits_dev, ef_route, ef, hash_bits, out_ids_dev, out_dist_dev, out_route_worst_dev, stats
#define ANNLITE_WALK(EE, ER)                                                                                  \
    (l2 ? launch_f32_walk(graph_f32_admit_kernel<EE, ER, true>, "graph_f32_admit_kernel", EE, ANNLITE_WALK_ARGS) \
        : launch_f32_walk(graph_f32_admit_kernel<EE, ER, false>, "graph_f32_admit_kernel", EE, ANNLITE_WALK_ARGS))
    // C's registers per lane from ef_route, R's from ef, as annlite_graph_f32_search chooses its own (ef <= ef_route: ER <= E)
    if (ef_route <= 64) return ANNLITE_WALK(1, 1);
    if (ef_route <= 128) return ef <= 64 ? ANNLITE_WALK(2, 1) : ANNLITE_WALK(2, 2);
    return ef <= 64 ? ANNLITE_WALK(4, 1) : ef <= 128 ? ANNLITE_WALK(4, 2) : ANNLITE_WALK(4, 4);
#undef ANNLITE_WALK
#undef ANNLITE_WALK_ARGS
}

// [0] expansions (link lists read), [1] rows evaluated, of the last float walk (ANNLITE_DEBUG_COUNTERS=1)
extern "C" int annlite_graph_f32_search_stats(uint64_t *out2) {
    ANNLITE_REQUIRE(out2 != nullptr, "out2 is NULL");
    if (!g_graph_f32_stats) {
        set_error("no counters recorded (set ANNLITE_DEBUG_COUNTERS=1 before the walk)");
        return ANNLITE_ERR_INVALID;
    }
    ANNLITE_HIP_TRY(hipDeviceSynchronize());
    ANNLITE_HIP_TRY(hipMemcpy(out2, g_graph_f32_stats, 16, hipMemcpyDeviceToHost));
    return ANNLITE_OK;
}

extern "C" int annlite_graph_f32_build_select(int metric, const int64_t *cand_dev, int ef, int64_t b, int64_t base0, const float *vectors_dev,
                                              int64_t N, int64_t D, int max_keep, uint32_t *links_dev, int links_per_node,
                                              int64_t *pairs_dev, void *stream) {
    ANNLITE_REQUIRE(metric >= 1 && metric <= 3, "bad metric %d", metric);
    ANNLITE_REQUIRE(b >= 0 && base0 >= 0 && ef >= 1 && ef <= kPoolMaxF32, "bad b=%lld base0=%lld ef=%d (ef <= 256)", (long long)b,
                    (long long)base0, ef);
    ANNLITE_REQUIRE(D >= 1 && D <= 2048, "the float graph takes 1 <= D <= 2048 (D = %lld)", (long long)D);
    ANNLITE_REQUIRE(base0 + b <= N && N < (1ll << 32) - 1, "the batch's points are rows base0 .. base0 + b of the table (N = %lld)", (long long)N);
    ANNLITE_REQUIRE(max_keep >= 1 && max_keep <= links_per_node && links_per_node <= 64, "bad max_keep=%d links_per_node=%d", max_keep,
                    links_per_node);
    if (b == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(cand_dev && vectors_dev && links_dev && pairs_dev, "null device pointer");
    const dim3 grid((unsigned)((b + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (metric == ANNLITE_METRIC_EUCLIDEAN)
        hipLaunchKernelGGL(graph_f32_select_kernel<true>, grid, block, 0, st, cand_dev, ef, b, base0, vectors_dev, N, (int)D, max_keep,
                           links_dev, links_per_node, pairs_dev);
    else
        hipLaunchKernelGGL(graph_f32_select_kernel<false>, grid, block, 0, st, cand_dev, ef, b, base0, vectors_dev, N, (int)D, max_keep,
                           links_dev, links_per_node, pairs_dev);
    return launch_status("graph_f32_select_kernel");
}

extern "C" int annlite_graph_f32_build_reverse(int metric, const int64_t *keys_dev, const int64_t *seg_dev, int64_t n_segments,
                                               const float *vectors_dev, int64_t N, int64_t D, uint32_t *links_dev, int links_per_node,
                                               void *stream) {
    ANNLITE_REQUIRE(metric >= 1 && metric <= 3, "bad metric %d", metric);
    ANNLITE_REQUIRE(n_segments >= 0 && N >= 0 && N < (1ll << 32) - 1, "bad n_segments / N");
    ANNLITE_REQUIRE(D >= 1 && D <= 2048, "the float graph takes 1 <= D <= 2048 (D = %lld)", (long long)D);
    ANNLITE_REQUIRE(links_per_node >= 1 && links_per_node <= 32, "reverse links: links_per_node in [1, 32] (%d)", links_per_node);
    if (n_segments == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(keys_dev && seg_dev && vectors_dev && links_dev, "null device pointer");
    const dim3 grid((unsigned)((n_segments + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (metric == ANNLITE_METRIC_EUCLIDEAN)
        hipLaunchKernelGGL(graph_f32_reverse_kernel<true>, grid, block, 0, st, keys_dev, seg_dev, n_segments, vectors_dev, N, (int)D,
                           links_dev, links_per_node);
    else
        hipLaunchKernelGGL(graph_f32_reverse_kernel<false>, grid, block, 0, st, keys_dev, seg_dev, n_segments, vectors_dev, N, (int)D,
                           links_dev, links_per_node);
    return launch_status("graph_f32_reverse_kernel");
}
