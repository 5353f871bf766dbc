// graph_f32.hip -- the level-0 graph over f32 rows: annlite_graph_f32_search / _search_admit / _build_select / _build_reverse are
// graph_rows.h's four kernels with rows_dist over float rows, one row per wave-wide pass.
#include "graph_rows.h"

namespace annlite {
unsigned long long *g_graph_f32_stats = nullptr;
}

using namespace annlite;
typedef RowsStrided<float> RowsF32;

extern "C" int annlite_graph_f32_search(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev, int64_t N,
                                        const uint32_t *links_dev, int links_per_node, const uint32_t *seeds_dev, int64_t n_seeds,
                                        const uint32_t *valid_bits_dev, int ef, int64_t *out_ids_dev, float *out_dist_dev, void *stream) {
    return graph_rows_search<RowsF32>(metric, queries_dev, B, D, vectors_dev, N, links_dev, links_per_node, seeds_dev, n_seeds, valid_bits_dev,
                                      ef, out_ids_dev, out_dist_dev, stream);
}

extern "C" int annlite_graph_f32_search_admit(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev, int64_t N,
                                              const uint32_t *links_dev, int links_per_node, const uint32_t *seeds_dev, int64_t n_seeds,
                                              const uint32_t *admit_bits_dev, int ef_route, int ef, int64_t *out_ids_dev,
                                              float *out_dist_dev, float *out_route_worst_dev, void *stream) {
    return graph_rows_search_admit<RowsF32>(metric, queries_dev, B, D, vectors_dev, N, links_dev, links_per_node, seeds_dev, n_seeds,
                                            admit_bits_dev, ef_route, ef, out_ids_dev, out_dist_dev, out_route_worst_dev, stream);
}

// [0] expansions (link lists read), [1] rows evaluated, of the last float walk over rows of either format (ANNLITE_DEBUG_COUNTERS=1)
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
    return graph_rows_build_select<RowsF32>(metric, cand_dev, ef, b, base0, vectors_dev, N, D, max_keep, links_dev, links_per_node, pairs_dev,
                                            stream);
}

extern "C" int annlite_graph_f32_build_reverse(int metric, const int64_t *keys_dev, const int64_t *seg_dev, int64_t n_segments,
                                               const float *vectors_dev, int64_t N, int64_t D, uint32_t *links_dev, int links_per_node,
                                               void *stream) {
    return graph_rows_build_reverse<RowsF32>(metric, keys_dev, seg_dev, n_segments, vectors_dev, N, D, links_dev, links_per_node, stream);
}
