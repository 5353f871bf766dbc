// graph_admit.hip -- the packed HNSW-over-PQ walk with an ADMITTED-RESULT list (annlite_graph_search_packed_admit): what answers a
// filtered search on the graph instead of by the exhaustive masked scan (the reference: knn_query_with_filter,
// hnsw_bindings.cpp:392-516 -> hnswlib searchBaseLayerST with a filter functor).
//
// The walk is graph_pq_walk.h's, the one graph.hip's graph_beam_search_kernel<M, E, PACKED = true, BATCH = true, W> runs; the routing
// list C and the result list R, what each is offered and the invariant that holds between them are graph_beam.h's AdmitList.  C's
// expansions, rows evaluated and prefetched records used are annlite_graph_search_packed_ex's at ef = ef_route.  What is this file's:
//   * the key: (f32_to_ordered(sum), id), the PQ walk's own;
//   * the pair walk offers up to 64 lanes per step, and a neighbour of both nodes passes the visited table's compare-and-swap once: R
//     sees the `mine` lanes C sees;
//   * LDS per wave and the workgroup are the plain walk's (one wave per SIMD at M = 16: registers are not the limit).
#include "graph_pq_walk.h"

namespace annlite {

template <int M, int E, int ER, int W>
__global__ __launch_bounds__(256) void graph_pq_admit_kernel(int links_per_node, const uint8_t *__restrict__ packed, int64_t rec_stride,
                                                            const uint32_t *__restrict__ seeds, int n_seeds,
                                                            const uint8_t *__restrict__ codes, int64_t N,
                                                            const uint32_t *__restrict__ admit, const float *__restrict__ lut_bmk, int B,
                                                            int Ks, int ef_route, int ef, int hash_bits, int64_t *__restrict__ out_ids,
                                                            float *__restrict__ out_dist, float *__restrict__ out_route_worst,
                                                            unsigned long long *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.x * (blockDim.x >> 6) + wave;
    if (b >= B) return;  // (whole waves leave; no block-wide barrier below)
    PQWalkCounters ct;
    Beam<E, true> bm;
    float *s_lut;
    pq_walk_setup<M, E, true>(smem, wave, lane, lut_bmk, b, Ks, ef_route, hash_bits, bm, s_lut);
    AdmitList<E, ER> rl;
    rl.init(bm, ef, n_seeds, admit);
    auto offer_both = [&](bool mine, uint32_t node, float d) __attribute__((always_inline)) { rl.offer_both(bm, mine, node, f32_to_ordered(d)); };
    pq_beam_walk<M, E, true, true, W>(bm, s_lut, lane, nullptr, links_per_node, packed, rec_stride, seeds, n_seeds, codes, N, Ks, stats,
                                      offer_both, ct);
    rl.write(b, ef, out_ids, out_dist);
    rl.write_route_worst(bm, b, out_route_worst);
    if (stats && lane == 0) pq_walk_add_stats(stats, ct);
}

}  // namespace annlite

using namespace annlite;

template <int M, int E, int ER, int W>
static int launch_admit(const uint8_t *packed, int lpn, const uint32_t *seeds, int n_seeds, const uint8_t *codes, int64_t N,
                        const uint32_t *admit, const float *lut, int64_t B, int64_t Ks, int ef_route, int ef, int hash_bits,
                        int64_t *out_ids, float *out_dist, float *out_route_worst, unsigned long long *stats, hipStream_t st) {
    // the plain walk's LDS per wave and waves per workgroup: R lives in registers and shares C's merge scratch
    const size_t per_wave = pq_walk_lds_per_wave<E, true>(M, Ks, hash_bits);
    const int wpb = pq_walk_waves_per_block(per_wave);
    ANNLITE_REQUIRE(wpb >= 1, "M * Ks tables do not fit the LDS");
    const size_t lds = wpb * per_wave;
    auto fn = graph_pq_admit_kernel<M, E, ER, W>;
    ANNLITE_HIP_TRY(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fn, dim3((unsigned)((B + wpb - 1) / wpb)), dim3(wpb * 64), lds, st, lpn, packed, graph_record_stride(lpn, M), seeds,
                       n_seeds, codes, N, admit, lut, (int)B, (int)Ks, ef_route, ef, hash_bits, out_ids, out_dist, out_route_worst, stats);
    return launch_status("graph_pq_admit_kernel");
}

// registers per lane of the two lists, as graph_search_impl chooses its own from ef (ef <= ef_route: ER <= E); the pair walk has a
// list of three registers per lane for 128 < ef <= 192
template <int M, int W>
static int dispatch_admit(const uint8_t *packed, int lpn, const uint32_t *seeds, int n_seeds, const uint8_t *codes, int64_t N,
                          const uint32_t *admit, const float *lut, int64_t B, int64_t Ks, int ef_route, int ef, int hash_bits,
                          int64_t *out_ids, float *out_dist, float *out_route_worst, unsigned long long *stats, hipStream_t st) {
#define ANNLITE_ADMIT(EE, ER) \
    launch_admit<M, EE, ER, W>(packed, lpn, seeds, n_seeds, codes, N, admit, lut, B, Ks, ef_route, ef, hash_bits, out_ids, out_dist, \
                               out_route_worst, stats, st)
    if (ef_route <= 64) return ANNLITE_ADMIT(1, 1);
    if (ef_route <= 128) return ef <= 64 ? ANNLITE_ADMIT(2, 1) : ANNLITE_ADMIT(2, 2);
    if constexpr (W == 2) {
        if (ef_route <= 192) return ef <= 64 ? ANNLITE_ADMIT(3, 1) : ef <= 128 ? ANNLITE_ADMIT(3, 2) : ANNLITE_ADMIT(3, 3);
        return ef <= 64 ? ANNLITE_ADMIT(4, 1) : ef <= 128 ? ANNLITE_ADMIT(4, 2) : ef <= 192 ? ANNLITE_ADMIT(4, 3) : ANNLITE_ADMIT(4, 4);
    } else {
        return ef <= 64 ? ANNLITE_ADMIT(4, 1) : ef <= 128 ? ANNLITE_ADMIT(4, 2) : ANNLITE_ADMIT(4, 4);
    }
#undef ANNLITE_ADMIT
}

extern "C" int annlite_graph_search_packed_admit(const void *packed_dev, int links_per_node, const uint32_t *seeds_dev, int64_t n_seeds,
                                                 const void *codes_dev, int64_t N, int64_t M, int64_t Ks, const uint32_t *admit_bits_dev,
                                                 const float *lut_bmk_dev, int64_t B, int ef_route, int ef, int expand_width,
                                                 int64_t *out_ids_dev, float *out_dist_dev, float *out_route_worst_dev, void *stream) {
    ANNLITE_REQUIRE(B >= 0 && N >= 0 && ef >= 1 && ef <= ef_route && ef_route <= 256, "bad B=%lld N=%lld ef=%d ef_route=%d (ef <= ef_route <= 256)",
                    (long long)B, (long long)N, ef, ef_route);
    ANNLITE_REQUIRE(admit_bits_dev != nullptr, "admit_bits_dev is NULL (a walk without a filter is annlite_graph_search_packed_ex)");
    ANNLITE_REQUIRE(packed_dev != nullptr || B == 0, "packed_dev is NULL");
    if (int rc = graph_walk_check(true, links_per_node, n_seeds, N, M, Ks, B, expand_width)) return rc;
    if (B == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(N >= 1, "no row to walk over (N = 0)");  // (the seed rounds read row 0 for the lanes without a seed)
    ANNLITE_REQUIRE(seeds_dev && codes_dev && lut_bmk_dev && out_ids_dev && out_dist_dev, "null device pointer");
    hipStream_t st = (hipStream_t)stream;
    const int hash_bits = graph_walk_hash_bits(ef_route);  // (annlite_graph_search_packed_ex's table at ef = ef_route)
    unsigned long long *stats = nullptr;
    if (int rc = graph_walk_stats(st, &stats)) return rc;
    const uint8_t *packed = (const uint8_t *)packed_dev, *codes = (const uint8_t *)codes_dev;
#define ANNLITE_ADMIT_M(MM)                                                                                                              \
    (expand_width == 2 ? dispatch_admit<MM, 2>(packed, links_per_node, seeds_dev, (int)n_seeds, codes, N, admit_bits_dev, lut_bmk_dev, B, \
                                               Ks, ef_route, ef, hash_bits, out_ids_dev, out_dist_dev, out_route_worst_dev, stats, st)  \
                       : dispatch_admit<MM, 1>(packed, links_per_node, seeds_dev, (int)n_seeds, codes, N, admit_bits_dev, lut_bmk_dev, B, \
                                               Ks, ef_route, ef, hash_bits, out_ids_dev, out_dist_dev, out_route_worst_dev, stats, st))
    if (M == 8) return ANNLITE_ADMIT_M(8);
    if (M == 16) return ANNLITE_ADMIT_M(16);
    if (M == 32) return ANNLITE_ADMIT_M(32);
    return ANNLITE_ADMIT_M(64);
#undef ANNLITE_ADMIT_M
}
