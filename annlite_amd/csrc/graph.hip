// graph.hip -- beam search over the level-0 lists of the HNSW-over-PQ graph ON THE GPU (BASELINE config 5).
//
// The reference walks its graph on the host, one query per call (hnsw_bindings.cpp:302-375 -> hnswalg.h
// searchBaseLayerST); libannlite_graph.so does the same, batch-parallel over CPU threads.  This kernel
// moves the walk next to the code table: ONE WAVE PER QUERY, its L2 look-up table (M*Ks fp32 = 16 KB at
// M=16) and a 4096-entry visited hash set (16 KB) in LDS, the ef_search best nodes seen so far as a sorted list spread over
// the lanes' registers (two entries per lane for ef = 128).  The upper layers of the hierarchy are not
// descended: the nodes of its top levels (annlite_hnsw_export: up to 4096 "seeds") are scanned flat --
// a coalesced gather of a few thousand code rows -- and the walk starts from the best of them.
//
// Per expansion (best unexpanded node of the list): its link list is one coalesced 132-byte read, the
// lanes that hold unseen neighbours fetch those rows' code bytes (the only random HBM traffic: 16 x 64-byte
// sectors) and evaluate hnswlib::PQLookup from LDS -- fp32 adds in ascending sub-space order, the same
// bits as the flat scan (space_pq.h:15-37) -- and the survivors are inserted into the sorted list.
// The walk ends when the list holds no unexpanded node (hnswalg.h searchBaseLayerST's stop rule).
//
// PACKED layout (round 5, annlite_graph_pack / annlite_graph_search_packed).  With the plain layout an expansion is TWO dependent
// random round trips -- the node's link list, then the 16-byte code rows of its unseen neighbours, each of which costs a
// 128-byte line: 385 MB of HBM traffic per 5M-row launch against 62 MB algorithmic, L2 hit rate 12 % -- and one wave per SIMD
// hides none of it.  A packed node record holds the neighbours' CODE ROWS behind its link list,
//     [L x M code bytes of neighbour 0 .. L-1][L x u32 link ids][u32 count][pad to 16 B]      (656 B at L = 32, M = 16)
// so an expansion is ONE contiguous read (lane j: neighbour j's 16 code bytes + its id), and the record of the best
// still-unexpanded node is PREFETCHED into registers while the current node's neighbours are evaluated: if the next pick is
// that node -- it is, once the walk has reached its plateau -- no round trip is exposed at all.  The order of the walk and
// the arithmetic are unchanged: candidate lists are bit-equal to the plain kernel's (tests/test_graph_packed.py).
#include "graph_pq_walk.h"

namespace annlite {

// BATCH (round 5): the neighbours of an expansion that beat the list's worst entry are MERGED into the sorted list in one pass --
// every list entry counts the candidates below it, every candidate the entries and candidates below it, all move to their
// final positions through a per-wave LDS scratch -- instead of one full-wave shift per candidate (~110 instructions each, the
// largest single item of the walk: one wave per SIMD executes them back to back).  The result is the same sorted list --
// the top of (old list + candidates) -- so the walk is unchanged; BATCH = false keeps the one-at-a-time insertion (the
// comparison path of tests/test_graph_packed.py).
// W (round 6, PACKED only): nodes expanded per step.  W = 2 = the PAIR walk: the two best unexpanded entries are expanded TOGETHER --
// lanes 0..31 take one record, lanes 32..63 the other (links_per_node <= 32), one pass through the visited table, one merge of up
// to 64 neighbours -- so a walk's chain of dependent steps is half as long (one wave per SIMD hides no latency: the launch lasts as
// long as one query's chain).  Every entry that stays inside the ef best is expanded sooner or later in either walk; the pair walk
// expands the runner-up before it knows the winner's neighbours, which changes the ORDER of expansions (and, rarely, expands a node
// the one-at-a-time walk would have seen pushed out of the list first).  The list is the same kind of object -- the ef best of the
// nodes evaluated, exact PQLookup sums -- and tests/test_graph_pair.py pins it bit for bit against a restatement of this order.
template <int M, int E, bool PACKED, bool BATCH, int W = 1>
__global__ __launch_bounds__(256) void graph_beam_search_kernel(const uint32_t *__restrict__ links, int links_per_node,
                                                               const uint8_t *__restrict__ packed, int64_t rec_stride,
                                                               const uint32_t *__restrict__ seeds, int n_seeds,
                                                               const uint8_t *__restrict__ codes, int64_t N,
                                                               const uint32_t *__restrict__ valid,
                                                               const float *__restrict__ lut_bmk, int B, int Ks, int ef,
                                                               int hash_bits, int64_t *__restrict__ out_ids,
                                                               float *__restrict__ out_dist,
                                                               unsigned long long *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.x * (blockDim.x >> 6) + wave;  // 1..4 waves per workgroup, as many as the LDS holds
    if (b >= B) return;  // (whole waves leave; no block-wide barrier below)
    // the walk itself -- seeds, visited table, records, PQLookup sums, merge -- is graph_pq_walk.h's, shared with graph_admit.hip
    PQWalkCounters ct;
    Beam<E, BATCH> bm;
    float *s_lut;
    pq_walk_setup<M, E, BATCH>(smem, wave, lane, lut_bmk, b, Ks, ef, hash_bits, bm, s_lut);
    auto offer = [&](bool mine, uint32_t node, float d) { bm.offer(mine, node, f32_to_ordered(d)); };
    pq_beam_walk<M, E, PACKED, BATCH, W>(bm, s_lut, lane, links, links_per_node, packed, rec_stride, seeds, n_seeds, codes, N, Ks, stats,
                                         offer, ct);
    beam_write(bm, b, ef, valid, out_ids, out_dist);
    if (stats && lane == 0) pq_walk_add_stats(stats, ct);
}

}  // namespace annlite

using namespace annlite;

// Packed node records for graph_beam_search_kernel<.., PACKED>: [L x M code bytes][L x u32 ids][u32 count][pad to 16 B].
// One thread per (node, neighbour slot): copies the neighbour's code row (slots beyond the count / ids beyond N: zeros).
__global__ __launch_bounds__(256) void graph_pack_kernel(const uint32_t *__restrict__ links, int L, const uint8_t *__restrict__ codes,
                                                        int64_t N, int M, uint8_t *__restrict__ out, int64_t stride) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * L) return;
    const int64_t node = t / L;
    const int j = (int)(t - node * L);
    const uint32_t *ll = links + node * (L + 1);
    const uint32_t cnt = ll[0];
    const uint32_t nb = (uint32_t)j < cnt ? ll[1 + j] : kEmpty;  // (an unused slot: an id no table holds)
    const bool ok = (uint32_t)j < cnt && (int64_t)nb < N;
    uint8_t *r = out + node * stride;
    uint32_t *dst = (uint32_t *)(r + (int64_t)j * M);
    const uint32_t *src = (const uint32_t *)(codes + (int64_t)(ok ? nb : 0u) * M);
    for (int i = 0; i < M / 4; ++i) dst[i] = ok ? src[i] : 0u;
    uint32_t *hdr = (uint32_t *)(r + (int64_t)L * M);
    hdr[j] = nb;
    if (j == 0) {
        hdr[L] = cnt;
        for (int64_t b = (int64_t)L * M + 4 * L + 4; b + 4 <= stride; b += 4) *(uint32_t *)(r + b) = 0u;
    }
}

template <int M, int E, bool PACKED, bool BATCH, int W = 1>
static int launch_beam(const uint32_t *links, int lpn, const uint8_t *packed, const uint32_t *seeds, int n_seeds, const uint8_t *codes,
                       int64_t N, const uint32_t *valid, const float *lut, int64_t B, int64_t Ks, int ef, int hash_bits,
                       int64_t *out_ids, float *out_dist, unsigned long long *stats, hipStream_t st) {
    const size_t per_wave = pq_walk_lds_per_wave<E, BATCH>(M, Ks, hash_bits);
    const int wpb = pq_walk_waves_per_block(per_wave);
    ANNLITE_REQUIRE(wpb >= 1, "M * Ks tables do not fit the LDS");
    const size_t lds = wpb * per_wave;
    auto fn = graph_beam_search_kernel<M, E, PACKED, BATCH, W>;
    ANNLITE_HIP_TRY(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fn, dim3((unsigned)((B + wpb - 1) / wpb)), dim3(wpb * 64), lds, st, links, lpn, packed,
                       graph_record_stride(lpn, M), seeds, n_seeds, codes, N, valid, lut, (int)B, (int)Ks, ef, hash_bits, out_ids,
                       out_dist, stats);
    return launch_status("graph_beam_search_kernel");
}

static unsigned long long *g_graph_stats = nullptr;  // debug only (ANNLITE_DEBUG_COUNTERS): leaked 64-byte device buffer

extern "C" int annlite_graph_search_stats(uint64_t *out2) {
    ANNLITE_REQUIRE(out2 != nullptr, "out2 is NULL");
    if (!g_graph_stats) {
        set_error("no counters recorded (set ANNLITE_DEBUG_COUNTERS=1 before the walk)");
        return ANNLITE_ERR_INVALID;
    }
    ANNLITE_HIP_TRY(hipDeviceSynchronize());
    ANNLITE_HIP_TRY(hipMemcpy(out2, g_graph_stats, 16, hipMemcpyDeviceToHost));
    return ANNLITE_OK;
}

// the walks' checks on graph, tables and expansion width (graph_search_impl, annlite_graph_search_packed_admit)
int annlite::graph_walk_check(bool packed, int links_per_node, int64_t n_seeds, int64_t N, int64_t M, int64_t Ks, int64_t B, int width) {
    ANNLITE_REQUIRE(width == 1 || (width == 2 && packed && links_per_node <= 32),
                    "expansion width %d: 1, or 2 over packed records of at most 32 neighbours (links_per_node = %d)", width, links_per_node);
    ANNLITE_REQUIRE(Ks >= 1 && Ks <= 256 && (M == 8 || M == 16 || M == 32 || M == 64), "graph search supports M in {8,16,32,64}, Ks <= 256");
    ANNLITE_REQUIRE(links_per_node >= 1 && n_seeds >= 1 && N < (1ll << 32) - 1, "bad graph");
    ANNLITE_REQUIRE(!packed || links_per_node <= 64, "packed records hold at most 64 neighbours (links_per_node = %d)", links_per_node);
    return ANNLITE_OK;
}

// entries of the visited table (log2) beside a routing list of `ef` places
int annlite::graph_walk_hash_bits(int ef) {
    // 4096 entries up to ef = 128 (a walk records 2-3k nodes: 5M rows, ef 128 gave the same recall as 8192 entries at
    // 1.5x the speed -- 5 instead of 3 waves per CU), 8192 beyond; a full table only costs re-evaluations (see visit)
    // round 6: 4096 entries up to ef = 208 as well -- with 8192 entries beside a list of more than 128 entries only three waves fit a CU
    // and a 1024-query batch runs in two rounds (10M rows, ef 144 / 160 / 192: 0.594 / 0.658 / 0.755 ms per batch with 8192 entries and
    // four registers per lane, 0.387 / 0.437 / 0.544 with 4096, 0.360 / 0.405 / 0.510 with three registers per lane on top -- the table
    // fills towards the end of such a walk and the merge tests for duplicates from then on; same lists, same recall:
    // profiles/r06/graph_10m_ef_sweep.txt)
    int hash_bits = ef <= 208 ? 12 : 13;  // (ef 200, the reference's ef_construction: 0.785 -> 0.568 ms per 1024 walks at 10M rows)
    if (knobs().graph_hash_bits >= 0) hash_bits = knobs().graph_hash_bits;  // (ANNLITE_GRAPH_HASH_BITS: tests force a tiny table)
    if (hash_bits < 4) hash_bits = 4;    // (buckets of four entries, 16-byte initialisation)
    if (hash_bits > 15) hash_bits = 15;  // (128 KB: what is left of the LDS beside the smallest table)
    return hash_bits;
}

// *stats: the debug counters' buffer, zeroed on `st` (NULL unless ANNLITE_DEBUG_COUNTERS)
int annlite::graph_walk_stats(hipStream_t st, unsigned long long **stats) {
    *stats = nullptr;
    if (knobs().debug_counters) {
        if (!g_graph_stats) ANNLITE_HIP_TRY(hipMalloc((void **)&g_graph_stats, 64));
        ANNLITE_HIP_TRY(hipMemsetAsync(g_graph_stats, 0, 64, st));
        *stats = g_graph_stats;
    }
    return ANNLITE_OK;
}

static int graph_search_impl(const uint32_t *links_dev, const uint8_t *packed_dev, int links_per_node, const uint32_t *seeds_dev,
                             int64_t n_seeds, const void *codes_dev, int64_t N, int64_t M, int64_t Ks, const uint32_t *valid_bits_dev,
                             const float *lut_bmk_dev, int64_t B, int ef, int64_t *out_ids_dev, float *out_dist_dev, void *stream,
                             int width = 1) {
    ANNLITE_REQUIRE(B >= 0 && N >= 0 && ef >= 1 && ef <= 256, "bad B=%lld N=%lld ef=%d (ef <= 256)", (long long)B,
                    (long long)N, ef);
    if (int rc = graph_walk_check(packed_dev != nullptr, links_per_node, n_seeds, N, M, Ks, B, width)) return rc;
    if (B == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE((links_dev || packed_dev) && seeds_dev && codes_dev && lut_bmk_dev && out_ids_dev && out_dist_dev, "null device pointer");
    hipStream_t st = (hipStream_t)stream;
    const int hash_bits = graph_walk_hash_bits(ef);
    const uint8_t *codes = (const uint8_t *)codes_dev;
    unsigned long long *stats = nullptr;
    if (int rc = graph_walk_stats(st, &stats)) return rc;
#define ANNLITE_BEAM_ARGS links_dev, links_per_node, packed_dev, seeds_dev, (int)n_seeds, codes, N, valid_bits_dev, lut_bmk_dev, B, Ks, ef, \
                          hash_bits, out_ids_dev, out_dist_dev, stats, st
#define ANNLITE_BEAM(MM, PK, BT) \
    (ef <= 64 ? launch_beam<MM, 1, PK, BT>(ANNLITE_BEAM_ARGS) : ef <= 128 ? launch_beam<MM, 2, PK, BT>(ANNLITE_BEAM_ARGS) : launch_beam<MM, 4, PK, BT>(ANNLITE_BEAM_ARGS))
    // (pair walk: a list of three registers per lane for 128 < ef <= 192 -- every list operation is per register)
#define ANNLITE_BEAM2(MM) \
    (ef <= 64 ? launch_beam<MM, 1, true, true, 2>(ANNLITE_BEAM_ARGS) : ef <= 128 ? launch_beam<MM, 2, true, true, 2>(ANNLITE_BEAM_ARGS) : \
     ef <= 192 ? launch_beam<MM, 3, true, true, 2>(ANNLITE_BEAM_ARGS) : launch_beam<MM, 4, true, true, 2>(ANNLITE_BEAM_ARGS))
    if (packed_dev && width == 2) {
        if (M == 8) return ANNLITE_BEAM2(8);
        if (M == 16) return ANNLITE_BEAM2(16);
        if (M == 32) return ANNLITE_BEAM2(32);
        return ANNLITE_BEAM2(64);  // (round 6: 64 KB of table per wave -- one wave per CU: a 256-query batch fills the chip)
    }
#undef ANNLITE_BEAM2
    if (packed_dev) {
        if (M == 8) return ANNLITE_BEAM(8, true, true);
        if (M == 16) return ANNLITE_BEAM(16, true, true);
        if (M == 32) return ANNLITE_BEAM(32, true, true);
        return ANNLITE_BEAM(64, true, true);
    }
    // ANNLITE_GRAPH_SEQ_INSERT=1 (plain layout): the one-at-a-time list insertion of rounds 2-4 -- the parity tests walk with
    // both and compare
    if (knobs().graph_seq_insert) {
        if (M == 8) return ANNLITE_BEAM(8, false, false);
        if (M == 16) return ANNLITE_BEAM(16, false, false);
        if (M == 32) return ANNLITE_BEAM(32, false, false);
        return ANNLITE_BEAM(64, false, false);
    }
    if (M == 8) return ANNLITE_BEAM(8, false, true);
    if (M == 16) return ANNLITE_BEAM(16, false, true);
    if (M == 32) return ANNLITE_BEAM(32, false, true);
    return ANNLITE_BEAM(64, false, true);
#undef ANNLITE_BEAM
#undef ANNLITE_BEAM_ARGS
}

// [0] expansions, [1] rows evaluated, [2] prefetched records used; shader cycles summed over the queries' waves: [3] seed phase, packed
// walk: [4] pick + wait for the record, [5] visited table, [6] PQLookup sums, [7] list merge
extern "C" int annlite_graph_search_stats_ex(uint64_t *out4) {
    ANNLITE_REQUIRE(out4 != nullptr, "out8 is NULL");
    if (!g_graph_stats) {
        set_error("no counters recorded (set ANNLITE_DEBUG_COUNTERS=1 before the walk)");
        return ANNLITE_ERR_INVALID;
    }
    ANNLITE_HIP_TRY(hipDeviceSynchronize());
    ANNLITE_HIP_TRY(hipMemcpy(out4, g_graph_stats, 64, hipMemcpyDeviceToHost));
    return ANNLITE_OK;
}

extern "C" int annlite_graph_search(const uint32_t *links_dev, int links_per_node, const uint32_t *seeds_dev, int64_t n_seeds,
                                    const void *codes_dev, int64_t N, int64_t M, int64_t Ks,
                                    const uint32_t *valid_bits_dev, const float *lut_bmk_dev, int64_t B, int ef,
                                    int64_t *out_ids_dev, float *out_dist_dev, void *stream) {
    return graph_search_impl(links_dev, nullptr, links_per_node, seeds_dev, n_seeds, codes_dev, N, M, Ks, valid_bits_dev, lut_bmk_dev,
                             B, ef, out_ids_dev, out_dist_dev, stream);
}

extern "C" int annlite_graph_record_bytes(int links_per_node, int64_t M, int64_t *bytes) {
    ANNLITE_REQUIRE(bytes != nullptr && links_per_node >= 1 && links_per_node <= 64 && (M == 8 || M == 16 || M == 32 || M == 64),
                    "packed records: links_per_node in [1, 64], M in {8,16,32,64}");
    *bytes = graph_record_stride(links_per_node, M);
    return ANNLITE_OK;
}

extern "C" int annlite_graph_pack(const uint32_t *links_dev, int links_per_node, const void *codes_dev, int64_t N, int64_t M,
                                  void *packed_dev, void *stream) {
    ANNLITE_REQUIRE(N >= 0 && links_per_node >= 1 && links_per_node <= 64 && (M == 8 || M == 16 || M == 32 || M == 64),
                    "packed records: links_per_node in [1, 64], M in {8,16,32,64}");
    if (N == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(links_dev && codes_dev && packed_dev, "null device pointer");
    const int64_t total = N * links_per_node;
    hipLaunchKernelGGL(graph_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, links_dev,
                       links_per_node, (const uint8_t *)codes_dev, N, (int)M, (uint8_t *)packed_dev, graph_record_stride(links_per_node, M));
    return launch_status("graph_pack_kernel");
}

extern "C" int annlite_graph_search_packed(const void *packed_dev, int links_per_node, const uint32_t *seeds_dev, int64_t n_seeds,
                                           const void *codes_dev, int64_t N, int64_t M, int64_t Ks,
                                           const uint32_t *valid_bits_dev, const float *lut_bmk_dev, int64_t B, int ef,
                                           int64_t *out_ids_dev, float *out_dist_dev, void *stream) {
    ANNLITE_REQUIRE(packed_dev != nullptr || B == 0, "packed_dev is NULL");
    return graph_search_impl(nullptr, (const uint8_t *)packed_dev, links_per_node, seeds_dev, n_seeds, codes_dev, N, M, Ks,
                             valid_bits_dev, lut_bmk_dev, B, ef, out_ids_dev, out_dist_dev, stream);
}

extern "C" int annlite_graph_search_packed_ex(const void *packed_dev, int links_per_node, const uint32_t *seeds_dev, int64_t n_seeds,
                                              const void *codes_dev, int64_t N, int64_t M, int64_t Ks,
                                              const uint32_t *valid_bits_dev, const float *lut_bmk_dev, int64_t B, int ef,
                                              int expand_width, int64_t *out_ids_dev, float *out_dist_dev, void *stream) {
    ANNLITE_REQUIRE(packed_dev != nullptr || B == 0, "packed_dev is NULL");
    return graph_search_impl(nullptr, (const uint8_t *)packed_dev, links_per_node, seeds_dev, n_seeds, codes_dev, N, M, Ks,
                             valid_bits_dev, lut_bmk_dev, B, ef, out_ids_dev, out_dist_dev, stream, expand_width);
}
