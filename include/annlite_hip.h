/*
 * annlite_hip.h -- C ABI of libannlite_hip.so: the MI355X (gfx950) implementation of annlite's
 * PQ codec + asymmetric-distance (ADC) scan hot path.
 *
 * This is the drop-in boundary.  Every entry point is what a binding for
 * the reference's `annlite.pq_bind` operator seam / `PQCodec` / index plugin would call; the
 * reference interface each one replaces is cited as (file:line) relative to jina-ai/annlite
 * v0.5.11.  The reference-side ctypes stub a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no exceptions across the boundary: every function returns an int status
 *     (ANNLITE_OK == 0); annlite_hip_last_error() gives a thread-local message.
 *   - all `*_dev` pointers are DEVICE pointers (HBM) owned by the caller (e.g. torch tensors'
 *     data_ptr()); outputs are caller-allocated.  No torch / HIP types in the signatures:
 *     `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - all launches are asynchronous on `stream`; the caller synchronises.
 *   - no shared mutable state inside the library: calls on different streams / host threads are
 *     independent (the reference's pq_bind is serial under the GIL, hnsw_bind attaches the LUT to a
 *     shared space object and is not re-entrant: include/hnswlib/space_pq.h:55-64).  What a call
 *     remembers for the next one -- which scan kernel suits a code table -- lives in an
 *     annlite_scan_state the CALLER owns (one per table), never in the process.  The thread-local
 *     items are the last-error message and the measurement hooks (annlite_profile_*).  The ANNLITE_* environment
 *     variables (A/B switches of measurements and tests, listed in DESIGN.md) are parsed ONCE when the library is
 *     loaded; nothing on the search path reads the environment (annlite_knobs_reload() below).
 *   - there is NO CPU fallback in this library: if no gfx950 device is present the launches fail
 *     with ANNLITE_ERR_HIP.
 *
 * Distances are float32, ADC sums are accumulated in float32 in ascending sub-space order, the LUT
 * entries are sequential fused multiply-add chains -- bit-identical to the reference built with its
 * own flags (setup.py:125-144) -- see DESIGN.md "Numerics".
 */
#ifndef ANNLITE_HIP_H_
#define ANNLITE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANNLITE_HIP_ABI_VERSION 2

/* exported symbols (the library is built with -fvisibility=hidden) */
#define ANNLITE_API __attribute__((visibility("default")))

/* status codes */
#define ANNLITE_OK 0
#define ANNLITE_ERR_INVALID 1     /* bad argument (shape, null pointer, k out of range ...)        */
#define ANNLITE_ERR_UNSUPPORTED 2 /* valid request this build has no kernel for                    */
#define ANNLITE_ERR_HIP 3         /* HIP runtime error (no device, launch failure ...)             */
#define ANNLITE_ERR_WORKSPACE 4   /* workspace too small: call the matching *_workspace_bytes()    */
#define ANNLITE_NOT_APPLICABLE 5  /* not an error: the request has no effect for this shape / state; nothing was launched
                                     (annlite_pq_search_split: make the plain call instead)                              */

/* metric ids == annlite/enums.py:25-28 (Metric.EUCLIDEAN / INNER_PRODUCT / COSINE) */
#define ANNLITE_METRIC_EUCLIDEAN 1
#define ANNLITE_METRIC_INNER_PRODUCT 2
#define ANNLITE_METRIC_COSINE 3

/* look-up-table kinds (what one table entry holds) */
#define ANNLITE_LUT_L2 1     /* sum_j (C[m,k,j]-q[j])^2    bindings/pq_bindings.pyx:149-210 (and 85-145) */
#define ANNLITE_LUT_IP 2     /* sum_j  C[m,k,j]*q[j]        bindings/pq_bindings.pyx:214-274              */
#define ANNLITE_LUT_IPDIST 3 /* float32(1/Ks) - LUT_IP      annlite/core/codec/pq.py:316-322              */

/* code-table layouts in HBM */
#define ANNLITE_CODES_PLAIN 0  /* [N][M] row-major, byte m of row n = code of sub-space m (the reference's
                                  PQIndex._data / HNSW level-0 record layout)                              */
#define ANNLITE_CODES_SKEWED 1 /* [N][M], byte j of row n = code of sub-space (j + n) mod M: every row is
                                  pre-rotated by its own row id so that the scan kernel's lane l (row n,
                                  n mod M == l mod M) reads sub-space (l + t) mod M at byte t with no
                                  in-register rotation (annlite_codes_skew converts; uint8 codes only)     */

/* look-up-table layouts in HBM */
#define ANNLITE_LAYOUT_BMK 0 /* [B][M][Ks]  -- the reference's layout (what get_dist_mat returns)       */
#define ANNLITE_LAYOUT_TILED 1 /* [ceil16(B)/QI][Ks][M][QI] -- scan layout (B padded to 16), QI from the plan */

ANNLITE_API int annlite_hip_abi_version(void);
ANNLITE_API const char *annlite_hip_last_error(void);
/* number of visible HIP devices and the gfx arch name of device `dev` (e.g. "gfx950:sramecc+:xnack-") */
ANNLITE_API int annlite_hip_device_count(int *count);
ANNLITE_API int annlite_hip_device_arch(int dev, char *buf, size_t buf_len);
/* The measurement / test switches (ANNLITE_SCAN_VARIANT, ANNLITE_Q8_*, ANNLITE_SEED_*, ANNLITE_NO_*, ANNLITE_GUARD_BASE, ...) are
 * read from the environment once, at load.  A process that changes them afterwards calls this to have them parsed again: the new
 * block is published atomically, calls already running keep the one they started with.  No reference counterpart (the reference has
 * no such switches); a production deployment never calls it. */
ANNLITE_API int annlite_knobs_reload(void);

/* ------------------------------------------------------------------------------------------------
 * Scan plan: how the ADC scan kernel wants its inputs for a (M, Ks, code width, k) problem.
 * ---------------------------------------------------------------------------------------------- */
typedef struct annlite_scan_plan {
    int32_t fast;          /* 1: LDS-resident skewed-gather kernel, 0: generic (LUT read through L2)  */
    int32_t qi;            /* queries interleaved per LUT entry in the tiled layout (4, 2 or 1)       */
    int32_t qt;            /* queries per workgroup (multiple of qi)                                  */
    int32_t waves;         /* waves per workgroup                                                     */
    int32_t n_slices;      /* row slices the table is cut into (>= 8: one per XCD)                    */
    int32_t max_k;         /* largest k this plan supports                                            */
    int64_t lut_floats;    /* number of floats of a TILED LUT buffer for B queries                    */
    int64_t workspace_bytes; /* scratch needed by annlite_adc_scan_topk()                             */
} annlite_scan_plan;

ANNLITE_API int annlite_scan_plan_query(int64_t N, int64_t M, int64_t Ks, int code_bytes, int64_t B, int64_t k,
                            annlite_scan_plan *plan);
/* the plan annlite_pq_search_tiles() runs with for V scan slots (its query tiles hold plan.qt slots each) */
ANNLITE_API int annlite_scan_plan_tiles(int64_t N, int64_t M, int64_t Ks, int code_bytes, int64_t V, int64_t k,
                            annlite_scan_plan *plan);

/* ------------------------------------------------------------------------------------------------
 * LUT construction.
 * replaces: pq_bind.batch_precompute_adc_table      (bindings/pq_bindings.pyx:149-210)  kind=L2
 *           pq_bind.batch_precompute_adc_table_ip   (bindings/pq_bindings.pyx:214-274)  kind=IP
 *           pq_bind.precompute_adc_table            (bindings/pq_bindings.pyx:85-145)   kind=L2, B=1
 *           PQCodec.get_dist_mat                    (annlite/core/codec/pq.py:293-325)  kind=L2|IPDIST
 * queries_dev   f32 [B][D]  (already normalised by the caller for COSINE, as pq.py:309-310 does)
 * codebooks_dev f32 [M][Ks][dsub], dsub = D / M     (PQCodec.get_codebook(), pq.py:231-237)
 * out_dev       f32, layout BMK: [B][M][Ks];  TILED: plan.lut_floats floats (pad queries zeroed)
 * `qi` is only read for the TILED layout (take it from annlite_scan_plan_query()).
 * Numerics: sequential fmaf chain over j, bit-exact vs the reference; the IP kinds run on the
 * f32 MFMA (v_mfma_f32_16x16x4_f32), which is bitwise that same chain.
 * ---------------------------------------------------------------------------------------------- */
ANNLITE_API int annlite_lut_build(int kind, const float *queries_dev, int64_t B, int64_t D,
                      const float *codebooks_dev, int64_t M, int64_t Ks, float *out_dev, int layout,
                      int qi, void *stream);

/* re-layout a [B][M][Ks] table (e.g. one the caller computed himself) into the scan layout */
ANNLITE_API int annlite_lut_retile(const float *lut_bmk_dev, int64_t B, int64_t M, int64_t Ks, float *out_tiled_dev,
                       int qi, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Flat ADC scan, all distances (the operator seam, one query).
 * replaces: pq_bind.dist_pqcodes_to_codebooks (bindings/pq_bindings.pyx:52-80) == DistanceTable.adist
 *           (annlite/core/codec/pq.py:350-368):  out[n] = sum_{m ascending} adtable[m][codes[n][m]]
 * adtable_dev f32 [M][Ks] ; codes_dev [N][M] of code_bytes (1|2|4) ; out_dev f32 [N]
 * ---------------------------------------------------------------------------------------------- */
ANNLITE_API int annlite_adc_dist(const float *adtable_dev, int64_t M, int64_t Ks, const void *codes_dev,
                     int code_bytes, int64_t N, float *out_dev, void *stream);

/* Gathered ADC: out[b][r] = ADC distance of row cand[b][r] under query b's table (cand < 0 -> +inf).
 * replaces: hnswlib::PQLookup (include/hnswlib/space_pq.h:15-37) evaluated over a candidate list --
 * the "GPU ADC rerank of HNSW candidate lists" of BASELINE config 5.
 * lut_bmk_dev f32 [B][M][Ks] ; cand_dev i64 [B][R] ; out_dev f32 [B][R] */
ANNLITE_API int annlite_adc_gather(const float *lut_bmk_dev, int64_t B, int64_t M, int64_t Ks, const void *codes_dev,
                       int code_bytes, int64_t N, const int64_t *cand_dev, int64_t R, float *out_dev,
                       void *stream);

/* Beam search over the level-0 lists of an HNSW-over-PQ graph, on the GPU (BASELINE config 5): one wave per
 * query, its L2 table and a visited set in LDS, the ef best nodes as a sorted list in registers.
 * replaces: the graph walk of hnsw_bind.Index.knn_query (bindings/hnsw_bindings.cpp:302-375 ->
 * include/hnswlib/hnswalg.h searchBaseLayerST) for a whole batch; edge distances are hnswlib::PQLookup
 * (space_pq.h:15-37) bit for bit.  The graph comes from libannlite_graph.so (annlite_hnsw_export).
 * links_dev u32 [N][links_per_node + 1] (count, ids) ; seeds_dev u32 [n_seeds] DISTINCT nodes (top of the
 * hierarchy, scanned flat -- REQUIRED distinct, as annlite_hnsw_export produces them: the seed scan inserts without a duplicate
 * test, a node listed twice would enter the beam twice and come back twice) ; codes_dev u8 [N][M] PLAIN ; lut_bmk_dev f32 [B][M][Ks] L2 tables ; ef <= 256 ; M in {8, 16, 32, 64} (64, round 6: 64 KB of table per wave, one wave per CU)
 * out_ids_dev i64 [B][ef] ascending by distance (-1 padded, deleted rows per valid_bits dropped),
 * out_dist_dev f32 [B][ef] (+inf padded). */
ANNLITE_API int annlite_graph_search(const uint32_t *links_dev, int links_per_node, const uint32_t *seeds_dev,
                         int64_t n_seeds, const void *codes_dev, int64_t N, int64_t M, int64_t Ks,
                         const uint32_t *valid_bits_dev, const float *lut_bmk_dev, int64_t B, int ef,
                         int64_t *out_ids_dev, float *out_dist_dev, void *stream);
/* The same walk over PACKED node records (round 5): a record holds the node's neighbours' CODE ROWS behind its link list --
 * [L x M code bytes][L x u32 ids][u32 count][pad to 16 B], annlite_graph_record_bytes() per node (656 B at L = 32, M = 16) --
 * so one expansion is ONE contiguous read instead of the link list followed by L random 16-byte rows (a 128-byte line
 * each), and the record of the next node is prefetched while the current one's neighbours are evaluated.  Same walk order,
 * same hnswlib::PQLookup arithmetic (space_pq.h:15-37, hnswalg.h:243-329): candidate lists bit-equal to annlite_graph_search's.
 * annlite_graph_pack builds the records from the exported lists and the PLAIN code table (rebuild after inserts; deletes
 * need none: deleted rows keep routing the walk, as in hnswlib).  links_per_node <= 64; codes_dev is still read for the seeds. */
ANNLITE_API int annlite_graph_record_bytes(int links_per_node, int64_t M, int64_t *bytes);
ANNLITE_API int annlite_graph_pack(const uint32_t *links_dev, int links_per_node, const void *codes_dev, int64_t N, int64_t M,
                       void *packed_dev, void *stream);
ANNLITE_API int annlite_graph_search_packed(const void *packed_dev, int links_per_node, const uint32_t *seeds_dev,
                         int64_t n_seeds, const void *codes_dev, int64_t N, int64_t M, int64_t Ks,
                         const uint32_t *valid_bits_dev, const float *lut_bmk_dev, int64_t B, int ef,
                         int64_t *out_ids_dev, float *out_dist_dev, void *stream);
/* ... with expand_width nodes expanded per step (round 6).  1 = annlite_graph_search_packed.  2 = the PAIR walk (links_per_node <= 32):
 * the two best unexpanded entries of the list are expanded TOGETHER -- one half wave per record, one pass through the visited table,
 * one merge of up to 64 neighbours -- so the chain of dependent steps of a walk (what a launch of one wave per query lasts) is half as
 * long.  The stop rule (no unexpanded entry among the ef best, hnswalg.h searchBaseLayerST) and the arithmetic are unchanged; the
 * ORDER of the expansions is not: the runner-up is expanded before the winner's neighbours are known, so the list can differ from
 * the one-at-a-time walk's in its last places (candidate overlap > 0.99 at ef = 128; tests/test_graph_pair.py pins the pair order
 * bit for bit against a restatement). */
ANNLITE_API int annlite_graph_search_packed_ex(const void *packed_dev, int links_per_node, const uint32_t *seeds_dev,
                         int64_t n_seeds, const void *codes_dev, int64_t N, int64_t M, int64_t Ks,
                         const uint32_t *valid_bits_dev, const float *lut_bmk_dev, int64_t B, int ef, int expand_width,
                         int64_t *out_ids_dev, float *out_dist_dev, void *stream);
/* ... for a FILTERED search (graph_admit.hip): annlite_graph_search_packed_ex's walk at ef = ef_route -- same expansions, same rows
 * evaluated, same prefetched records: admit_bits_dev never touches the routing list -- with a SECOND sorted list of
 * ef <= ef_route <= 256 places that is offered every batch the routing list is offered (a seed round, a step's unseen neighbours),
 * restricted to the rows set in admit_bits_dev (u32 bitmap over the N rows, REQUIRED: valid & filter; a walk without a filter is the
 * entry point above), under the same test-against-the-worst-entry-then-merge rule, ordered by (PQLookup sum, id).  It ends as the ef
 * smallest (sum, id) among the admitted rows the walk evaluated: out_ids_dev i64 [B][ef] / out_dist_dev f32 [B][ef] ascending, the
 * missing places (-1, +inf) at the tail.  out_route_worst_dev f32 [B] (may be NULL): the sum at the routing list's last place, +inf
 * while that list is not full -- how far the walk reached; a result beyond it was only met on the way.  expand_width as above.
 * ANNLITE_DEBUG_COUNTERS fills the counters of annlite_graph_search_stats_ex. */
ANNLITE_API int annlite_graph_search_packed_admit(const void *packed_dev, int links_per_node, const uint32_t *seeds_dev,
                         int64_t n_seeds, const void *codes_dev, int64_t N, int64_t M, int64_t Ks,
                         const uint32_t *admit_bits_dev, const float *lut_bmk_dev, int64_t B, int ef_route, int ef,
                         int expand_width, int64_t *out_ids_dev, float *out_dist_dev, float *out_route_worst_dev, void *stream);
/* ---- the level-0 graph BUILT ON THE GPU, in batches (round 6; graph_build.hip) -------------------------------------------------
 * replaces, for a batch of points: hnswlib addPoint (include/hnswlib/hnswalg.h:1108-1235) = searchBaseLayer with ef_construction
 * (the walk above over the graph as it is, the points' own L2 tables as queries), getNeighborsByHeuristic2 (378-429) and
 * mutuallyConnectNewElement (431-553), in the form libannlite_graph.so gives them (hnsw_host.cpp select_neighbors / connect: the
 * triangle tests on the SYMMETRIC code-to-code L2 table).  Only level 0 exists -- the GPU walk scans a seed sample flat and never
 * descends upper layers.  Node id = row of the PLAIN code table.
 *   annlite_graph_build_sdc      sdc f32 [M][Ks][Ks] <- sum_j (C[m][a][j] - C[m][b][j])^2
 *   annlite_graph_build_select   point i of the batch = node base0 + i; cand_dev i64 [b][ef] = its candidates in ascending search
 *                                distance (-1 = none; ef <= 256): keeps at most max_keep of them (every one if they are that few),
 *                                writes links[base0 + i] = (count, ids) and pairs[i][0..max_keep) = (target << 32) | source
 *                                (INT64_MAX = none)
 *   annlite_graph_build_reverse  keys_dev i64 [P] = the pairs SORTED ascending; seg_dev i64 [S + 1] = the boundaries of the S runs
 *                                of equal target: every target appends its sources while its list has room, else shrinks
 *                                (list + sources) to links_per_node (<= 32) entries with the same heuristic; a target takes at most
 *                                64 - (its list's length) sources of one call (the lowest ids; the rest are dropped: a link the
 *                                heuristic would most likely have pruned -- only the all-at-once start of a graph sees such hubs)
 *   annlite_graph_pack_nodes     the packed records (annlite_graph_pack) of the nodes in nodes_dev i64 [n_nodes] only */
ANNLITE_API int annlite_graph_build_sdc(const float *codebooks_dev, int64_t M, int64_t Ks, int64_t dsub, float *sdc_dev, void *stream);
ANNLITE_API int annlite_graph_build_select(const int64_t *cand_dev, int ef, int64_t b, int64_t base0, const void *codes_dev, int64_t M,
                         int64_t Ks, const float *sdc_dev, int max_keep, uint32_t *links_dev, int links_per_node,
                         int64_t *pairs_dev, void *stream);
ANNLITE_API int annlite_graph_build_reverse(const int64_t *keys_dev, const int64_t *seg_dev, int64_t n_segments, const void *codes_dev,
                         int64_t M, int64_t Ks, const float *sdc_dev, uint32_t *links_dev, int links_per_node, void *stream);
ANNLITE_API int annlite_graph_pack_nodes(const uint32_t *links_dev, int links_per_node, const void *codes_dev, int64_t N, int64_t M,
                         const int64_t *nodes_dev, int64_t n_nodes, void *packed_dev, void *stream);
/* Debug aid: with ANNLITE_DEBUG_COUNTERS=1 the walk counts [0] expansions (link lists read) and [1] rows evaluated
 * (PQLookup sums) over the batch; this copies the two counters of the last walk to the host (the roofline of
 * scripts/bench_hnsw.py: algorithmic bytes = expansions * 4 (links_per_node + 1) + evaluations * M). */
ANNLITE_API int annlite_graph_search_stats(uint64_t *out2);
/* ... EIGHT counters: [2] the expansions whose record had been prefetched (packed walk); shader cycles summed over the queries'
 * waves: [3] seed phase, [4] pick + wait for the record, [5] visited table, [6] PQLookup sums, [7] list merge. */
ANNLITE_API int annlite_graph_search_stats_ex(uint64_t *out8);
/* ---- the level-0 graph over FLOAT vectors (graph_f32.hip): the walk and the two build kernels above with ONE float distance ------
 * Every distance compared -- query to row in the walk, row to row in the build -- carries annlite_exact_gather_dist's bits for the
 * metric (64 lane-strided fmaf chains, the xor butterfly 32..1; EUCLIDEAN: sum of (x[j] - q[j])^2, else 1 - sum of x[j] q[j]): the
 * walk's list holds final distances, a stored vector finds itself at exactly 0.0.  1 <= D <= 2048.
 *   annlite_graph_f32_search         one wave per query over links_dev u32 [N][links_per_node + 1] (count, ids; links_per_node <= 64),
 *                                    seeds_dev u32 [n_seeds] DISTINCT, vectors_dev f32 [N][D], queries_dev f32 [B][D]; ef <= 256.  The
 *                                    order of annlite_graph_search; the list is ordered by (distance, node id), NaN behind +inf.
 *                                    out_ids_dev i64 [B][ef] / out_dist_dev f32 [B][ef]: ascending, rows cleared in valid_bits_dev
 *                                    (may be NULL) blanked IN PLACE to (-1, +inf) -- they still route the walk.
 *   annlite_graph_f32_search_admit   the same walk at ef = ef_route (same expansions, same rows evaluated: admit_bits_dev never
 *                                    touches the routing list) with a SECOND sorted list of ef <= ef_route <= 256 places that is
 *                                    offered every batch the routing list is offered -- a seed round, an expansion's unseen
 *                                    neighbours -- restricted to the rows set in admit_bits_dev (u32 bitmap over the N rows,
 *                                    required; valid & filter), under the same test-against-the-worst-entry-then-merge rule.  It
 *                                    ends as the ef smallest (distance, id) among the admitted rows the walk evaluated: out_ids_dev
 *                                    i64 [B][ef] / out_dist_dev f32 [B][ef] ascending, missing places (-1, +inf) at the tail.
 *                                    out_route_worst_dev f32 [B] (may be NULL): the distance of the routing list's last place, +inf
 *                                    while that list is not full -- how far the walk reached; a result beyond it was only met on the way.
 *   annlite_graph_f32_build_select   annlite_graph_build_select; the batch's points are rows base0 .. base0 + b of vectors_dev [N][D]
 *   annlite_graph_f32_build_reverse  annlite_graph_build_reverse; a shrinking pool is ordered by (distance to the target, id)
 *   annlite_graph_f32_search_stats   debug aid (ANNLITE_DEBUG_COUNTERS=1): [0] expansions, [1] rows evaluated of the last float walk */
ANNLITE_API int annlite_graph_f32_search(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev, int64_t N,
                         const uint32_t *links_dev, int links_per_node, const uint32_t *seeds_dev, int64_t n_seeds,
                         const uint32_t *valid_bits_dev, int ef, int64_t *out_ids_dev, float *out_dist_dev, void *stream);
ANNLITE_API int annlite_graph_f32_search_admit(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev, int64_t N,
                         const uint32_t *links_dev, int links_per_node, const uint32_t *seeds_dev, int64_t n_seeds,
                         const uint32_t *admit_bits_dev, int ef_route, int ef, int64_t *out_ids_dev, float *out_dist_dev,
                         float *out_route_worst_dev, void *stream);
ANNLITE_API int annlite_graph_f32_build_select(int metric, const int64_t *cand_dev, int ef, int64_t b, int64_t base0,
                         const float *vectors_dev, int64_t N, int64_t D, int max_keep, uint32_t *links_dev, int links_per_node,
                         int64_t *pairs_dev, void *stream);
ANNLITE_API int annlite_graph_f32_build_reverse(int metric, const int64_t *keys_dev, const int64_t *seg_dev, int64_t n_segments,
                         const float *vectors_dev, int64_t N, int64_t D, uint32_t *links_dev, int links_per_node, void *stream);
ANNLITE_API int annlite_graph_f32_search_stats(uint64_t *out2);

/* ------------------------------------------------------------------------------------------------
 * Batched flat ADC scan + top-k: the hot path.
 * replaces, for B queries in ONE launch: PQIndex.search (annlite/core/index/pq_index.py:29-56:
 * LUT -> adist over the code table -> math.top_k, annlite/math.py:94-120), i.e. the per-query loop
 * of CellContainer.search_cells (annlite/container.py:214) over the index plugin's .search().
 *
 * codes_dev   [N][M] codes, row-major, code_bytes 1 (Ks<=256) or 2; codes_layout PLAIN or SKEWED
 *             (SKEWED only with the fast plan)
 * valid_bits  optional u32 bitmap, bit n set = row n may be returned (NULL = all N rows).  Carries
 *             delete() marks (annlite/core/index/hnsw/index.py:169-171) and the `indices` filter
 *             argument of search (pq_index.py:42-44).
 * lut_dev     the tables in plan.layout order: TILED for plan.fast, else BMK
 * out_dist_dev f32 [B][k], out_id_dev i64 [B][k]: ascending by (distance, row id) -- the fixed
 *             tie-break -- ids are row_base + row; missing entries (k > #valid rows) are (+inf, -1).
 * workspace   plan.workspace_bytes of device scratch.
 * ---------------------------------------------------------------------------------------------- */
ANNLITE_API int annlite_adc_scan_topk(const void *codes_dev, int code_bytes, int codes_layout, int64_t N, int64_t M,
                          int64_t Ks, const uint32_t *valid_bits_dev, const float *lut_dev, int64_t B, int64_t k,
                          int64_t row_base, float *out_dist_dev, int64_t *out_id_dev,
                          void *workspace_dev, size_t workspace_bytes, void *stream);

/* Same scan and result, written as ONE buffer out_packed_dev i64 [B][k][2] = (row_base + row or -1, the f32
 * distance's bits zero-extended): what a rank contributes to the single all-gather of the row-sharded
 * search; annlite_topk_merge_packed consumes the gathered [G][B][k][2]. */
ANNLITE_API int annlite_adc_scan_topk_packed(const void *codes_dev, int code_bytes, int codes_layout, int64_t N, int64_t M,
                                 int64_t Ks, const uint32_t *valid_bits_dev, const float *lut_dev, int64_t B,
                                 int64_t k, int64_t row_base, int64_t *out_packed_dev, void *workspace_dev,
                                 size_t workspace_bytes, void *stream);

/* The index plugin's search() in ONE call: query batch in, neighbours out.
 * replaces: PQIndex.search / HnswIndex.search's LUT step + scan + top_k for B queries
 * (annlite/core/index/pq_index.py:29-56, hnsw/index.py:139-167: get_dist_mat -> adist/knn -> top_k).
 * Equivalent to annlite_lut_build(lut_kind, ...) into the plan's layout followed by annlite_adc_scan_topk
 * (or _packed when out_packed_dev != NULL; then out_dist_dev/out_id_dev may be NULL) -- same bits --
 * but for L2 tables on the quantised-filter plan the tables are built, reduced and quantised by one
 * launch.  queries_dev must already carry the caller's pre-processing (l2-normalised for COSINE).
 * flags: ANNLITE_FLAG_SQRT.
 * workspace: annlite_pq_search_workspace_bytes() bytes (scan scratch + the fp32 tables). */
#define ANNLITE_FLAG_SQRT 1 /* metric epilogue of EUCLIDEAN search: out_dist = sqrt(ADC sum) (hnsw/index.py:164-165);
                               applied after all merging, ignored for packed output (raw sums travel) */
ANNLITE_API int annlite_pq_search_workspace_bytes(int64_t N, int64_t M, int64_t Ks, int code_bytes, int64_t B, int64_t k,
                                      int64_t *bytes);
ANNLITE_API int annlite_pq_search_topk(int lut_kind, const float *queries_dev, int64_t B, int64_t D,
                           const float *codebooks_dev, const void *codes_dev, int code_bytes, int codes_layout,
                           int64_t N, int64_t M, int64_t Ks, const uint32_t *valid_bits_dev, int64_t k,
                           int64_t row_base, float *out_dist_dev, int64_t *out_id_dev, int64_t *out_packed_dev,
                           int flags, void *workspace_dev, size_t workspace_bytes, void *stream);
/* ... with the caller's per-table state (see annlite_scan_state below; NULL = annlite_pq_search_topk) */
struct annlite_scan_state;
ANNLITE_API int annlite_pq_search_topk_ex(int lut_kind, const float *queries_dev, int64_t B, int64_t D,
                              const float *codebooks_dev, const void *codes_dev, int code_bytes, int codes_layout,
                              int64_t N, int64_t M, int64_t Ks, const uint32_t *valid_bits_dev, int64_t k,
                              int64_t row_base, float *out_dist_dev, int64_t *out_id_dev, int64_t *out_packed_dev,
                              int flags, void *workspace_dev, size_t workspace_bytes, void *stream,
                              struct annlite_scan_state *state);

/* The row-sharded search of one process per GPU, with a SEED EXCHANGE between the ranks: the search above
 * in two halves, so that a rank can seed from 1/G of the rows a single GPU would and still start its scan with the bound of
 * all G ranks' seed rows together.  (Every rank repeats the per-batch work for all B queries; the seed bound -- the exact
 * k-th distance of S rows spread over the table -- is the largest part of it: 22 of 39 us at 32768 rows x 1024 queries.)
 *   phase ANNLITE_PHASE_PREPARE  tables, parameters, reset, the seed bound from `seed_rows` rows spread over this rank's table (<= 0: the
 *       single-GPU default) and -- the rank's contribution to one all-gather -- seed_keys_dev [B][ANNLITE_SEED_KEYS] u64: the
 *       bounds implied by the seed's k smallest rows, ascending (all-ones where it has fewer).  Outputs untouched.
 *   annlite_pq_search_seed_union  all_keys_dev [G][B][ANNLITE_SEED_KEYS] (the all-gathered keys): the k-th smallest of a
 *       query's G * k keys has k distinct rows of the GLOBAL table at or below it -- the prepared batch's bound becomes
 *       min(own, that).
 *   phase ANNLITE_PHASE_SCAN     the scan of the prepared batch (same arguments, same workspace, same stream order).
 * PREPARE returns ANNLITE_NOT_APPLICABLE -- nothing launched, make the plain call -- unless the batch runs the byte-table
 * plan with the fused preparation launch (M = 16, uint8 codes, L2 tables, k <= 16, D <= 256, N >= 4096) and `state` has
 * settled on the byte-table kernel.  Results are those of the plain call, bit for bit (a bound only prunes). */
#define ANNLITE_PHASE_PREPARE 1
#define ANNLITE_PHASE_SCAN 2
#define ANNLITE_SEED_KEYS 16
ANNLITE_API int annlite_pq_search_split(int phase, int64_t seed_rows, int lut_kind, const float *queries_dev, int64_t B, int64_t D,
                            const float *codebooks_dev, const void *codes_dev, int code_bytes, int codes_layout,
                            int64_t N, int64_t M, int64_t Ks, const uint32_t *valid_bits_dev, int64_t k,
                            int64_t row_base, float *out_dist_dev, int64_t *out_id_dev, int64_t *out_packed_dev,
                            int flags, void *workspace_dev, size_t workspace_bytes, void *stream,
                            struct annlite_scan_state *state, uint64_t *seed_keys_dev);
ANNLITE_API int annlite_pq_search_seed_union(const uint64_t *all_keys_dev, int64_t G, int64_t N, int64_t M, int64_t Ks,
                                 int code_bytes, int64_t B, int64_t k, void *workspace_dev, size_t workspace_bytes,
                                 void *stream);

/* Same scan, but return the UNMERGED per-slice lists: plan.n_slices * k candidates per query
 * ([B][n_slices*k], unordered across slices, (+inf,-1) where a slice had fewer rows).  The set is a
 * superset of the exact top-k; it is the candidate generator of the exact re-rank stage
 *  -- the reference has no such stage. */
ANNLITE_API int annlite_adc_scan_candidates(const void *codes_dev, int code_bytes, int codes_layout, int64_t N, int64_t M,
                                int64_t Ks, const uint32_t *valid_bits_dev, const float *lut_dev, int64_t B,
                                int64_t k, int64_t row_base, float *out_dist_dev, int64_t *out_id_dev,
                                void *workspace_dev, size_t workspace_bytes, void *stream);
/* ... with the tables built inside the call (round 6): queries_dev f32 [B][D] + codebooks_dev instead of a prebuilt table; same
 * output, out[b][0 .. n_slices * k) with n_slices of annlite_scan_plan_query(N, M, Ks, code_bytes, B, k); workspace of
 * annlite_pq_search_workspace_bytes.  M = 16, L2 tables, k <= 16: ONE preparation launch (tables, list reset, ONE first bound from
 * rows spread over the whole table, prebuilt byte tables) instead of four; every slice then keeps the k best of ITS rows that are at
 * or below that bound -- the bound lies at or above the k-th key of the whole table, so the lists still hold the table's top-k
 * (and a row beyond it is of no use to a re-rank: a slice far from the query returns fewer than k rows, -1 padded). */
ANNLITE_API int annlite_pq_search_candidates(int lut_kind, const float *queries_dev, int64_t B, int64_t D, const float *codebooks_dev,
                             const void *codes_dev, int code_bytes, int codes_layout, int64_t N, int64_t M, int64_t Ks,
                             const uint32_t *valid_bits_dev, int64_t k, int64_t row_base, float *out_dist_dev,
                             int64_t *out_id_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* Measurement hooks (bench.py): when enabled on the calling thread, annlite_adc_scan_topk /
 * _candidates bracket the scan kernel launch -- the dominant kernel -- with HIP events on the
 * launch stream; annlite_profile_last_scan_ms() waits for the last one and returns its duration. */
ANNLITE_API int annlite_profile_enable(int on);
ANNLITE_API int annlite_profile_last_scan_ms(float *ms);
/* ... and, for the byte-table kernel, the shader clock that launch actually held (MHz): workgroup 0's s_memtime delta over
 * its 100 MHz wall-clock delta.  ANNLITE_ERR_INVALID when the last profiled scan was not a byte-table launch. */
ANNLITE_API int annlite_profile_last_scan_clock_mhz(float *mhz);
/* Revision (> 0) of a kernel's memory behaviour, by kernel name ("adc_scan_q8_kernel", ...); 0 = unknown name.  Recorded with every
 * kept PMC pass (profiles/traffic.json): bench.py's roofline.traffic refuses a pass taken on another revision. */
ANNLITE_API int annlite_kernel_rev(const char *kernel);
/* Kernel choice (M = 8 / 16 / 32 with uint8 codes, M = 8 with uint16 codes up to Ks = 1024; k <= 16): byte filter tables (the default)
 * or u16 filter tables -- made INSIDE the library, per call, never by a process-wide switch.  Without a state every
 * byte-table launch is guarded: it gives up when a workgroup has seen more than 1024 + (rows it has drawn) / 16 candidates
 * (a byte filter that leaks) and a gated u16-table pass queued behind it redoes the scan (~10 us per batch of gated
 * launches that return at once otherwise).  With a state -- ONE PER CODE TABLE, created once, passed to
 * annlite_pq_search_topk_ex -- every byte-table launch leaves its candidate count in the state's host-mapped block; later
 * calls read it without synchronising: a launch that gave up settles the table on the u16 kernel, one with few candidates
 * on the byte tables, and in between the state times ONE call of each kernel (events in the caller's stream, queried,
 * never waited for) and keeps the faster -- until the table has doubled or halved.  Results are identical whatever runs.  (Calls
 * that carry a state record events and read a host-mapped block: do not issue them inside a stream capture.)  A state must
 * not be used by two host threads at once (one searcher per index, as the reference has: SURVEY.md section 8b);
 * destroy it only after the launches that were given it have completed.
 * annlite_scan_state_info: kernel = 0 undecided, 1 byte tables, 2 u16 tables; rows / candidates of the deciding launch.
 * (ANNLITE_SCAN_VARIANT in the environment, read per call, still forces one instantiation for A/B measurements.) */
typedef struct annlite_scan_state annlite_scan_state;
ANNLITE_API int annlite_scan_state_create(annlite_scan_state **out);
ANNLITE_API int annlite_scan_state_destroy(annlite_scan_state *state);
ANNLITE_API int annlite_scan_state_reset(annlite_scan_state *state);
ANNLITE_API int annlite_scan_state_info(annlite_scan_state *state, int32_t *kernel, int64_t *rows, uint64_t *candidates);
/* Debug aid: with ANNLITE_DEBUG_COUNTERS=1 in the environment the scan counts events; this copies the 8 uint64
 * counters of the last scan to the host.  u16 kernels: [0] slow-block entries [1] (wave,query) candidate events
 * [2] events that inserted [3] bound publications [4] candidate rows.  Byte-table kernel: [0] wave-steps with a
 * candidate [1] candidates pushed [2] exact sums [3] candidates queued for a list [4] consumer-wave cycles inside
 * batches [5] table rebuilds [6] consumer batches [7] cycles of wave 0 at epoch ends. */
ANNLITE_API int annlite_debug_counters(uint64_t *out8);
/* Debug aid, same switch: the byte-table kernel's split step (M = 16, ANNLITE_Q8_SPLIT): [0] rows through its first phase
 * [1] rows that survived it (queued for the second) [2] second-phase wave-steps [3] wave-steps finished in place. */
ANNLITE_API int annlite_debug_split_counters(uint64_t *out4);
/* Debug aid (no switch, no device read): the sub-spaces in the first phase of the split step that the most recent shared-bound
 * launch of the M = 16 byte-table kernel over SKEWED rows took (10 .. 12: ANNLITE_Q8_SPLIT, or chosen by the rows one work item
 * scans, ANNLITE_Q8_SPLIT_ROWS); 0: the one-phase step; -1: no such launch yet in this process. */
ANNLITE_API int annlite_debug_q8_split_width(void);
/* Debug aid, same switch: phase stamps of the byte-table kernel's workgroups (thread 0, 100 MHz wall clock): [0] 2^62 -
 * earliest start, [1] latest end; sums over the work items of [2] start stamp, [3] initialisation + first table build,
 * [4] step loop, [5] wait at the last barrier, [6] list store + merge; [7] work items. */
ANNLITE_API int annlite_debug_timeline(uint64_t *out8);
/* ... and per work item (up to 4096 records of 8 uint64): query tile, row slice, the stamps start / table built / step loop
 * left / last barrier passed / end, block index. */
ANNLITE_API int annlite_debug_items(uint64_t *out, int64_t max_items, int64_t *n_items);
/* ... and of the byte-table plan's preparation launch (tables + parameters + reset + seed bound [+ byte tables], one launch):
 * stamps of its first workgroup [0..3] and its last one [4..7]: start, tables built, seed rows scanned, end. */
ANNLITE_API int annlite_debug_prep_timeline(uint64_t *out8);
/* Test hook of the seed bound's MFMA nomination launch (round 6, seed_mfma.hip; M = 16, 128-d, uint8 codes): `seed_rows` seed rows
 * (a multiple of 8192, <= 131072, <= N) spread over the table are cut into 512 disjoint groups; cand_dev u32 [B][512] receives, per
 * query and group, the table row with the smallest APPROXIMATE (bf16 contraction) ADC distance -- 0xffffffff where the group holds
 * no valid row.  The search itself never returns these: it takes the k-th smallest EXACT sum of a query's nominees as its first
 * bound (any k distinct valid rows give a valid one).  ANNLITE_NOT_APPLICABLE for other shapes.  No reference counterpart. */
ANNLITE_API int annlite_debug_seed_candidates(const float *queries_dev, int64_t B, int64_t D, const float *codebooks_dev,
                                  const void *codes_dev, int codes_layout, int64_t N, int64_t M, int64_t Ks,
                                  const uint32_t *valid_bits_dev, int64_t seed_rows, uint32_t *cand_dev, void *stream);
/* Debug aid (pure host code: no GPU, no device memory): what one scan launch sequence resolves to -- plan, workspace layout, kernel,
 * grid, every kernel argument -- for a shape, a kernel variant (-1: as ANNLITE_SCAN_VARIANT says, 31: u16 tables, 50: byte tables as the
 * library asks for them) and the options of the call as `flags`: 1 the slices share their bounds (top-k searches), 2 the tables are built
 * inside the call from D-dimensional queries, 4 tile mode (B slots, V real queries), 8 byte-table launch that may give up (guarded),
 * 16 launch gated on the one in front, 32 the table's state is attached (statistics block), 64 the candidate generator may take ONE
 * seed bound, 128 packed output instead of distances + ids, 256 no output buffers, 512 a valid-row bitmap; split_phase 0 or
 * ANNLITE_PHASE_*, with seed_rows.  Returns the status the scan would return before its first launch and fills
 * out[ANNLITE_SCAN_RESOLVE_FIELDS]:
 *   [0..17]  status, stage (0 nothing to do, 1 reset only, 2 up to the preparation launch, 3 scan), kernel family (0 byte tables, 1 u16
 *            tables, 2 generic with the table in LDS, 3 generic), kernel id, grid, SKEWED rows, reset fused into the preparation, reset bytes,
 *            preparation (0 none, 1 quantise + seed bound, 2 one preparation launch, 3 done by the PREPARE half), MFMA nominees, seed rows S,
 *            S as the preparation launch takes them, rows the seed is spread over, per-slice seed rows, merged in the scan, the plan's
 *            workspace_bytes and n_slices, dynamic LDS bytes (generic kernels)
 *   [18..46] the scan kernel's scalar arguments: N, Ks, B, k, n_tiles, n_slices, n_items, slice_rows, jm1, row_base, sqrt_out, flush_mask,
 *            dbg_skip, tl_private, cand_cap, q8_epoch0, q8_epoch_mul, q8_ring_limit, q8_import_mask, q8_target, q8_thw_mask, q8_rebuild_8ths,
 *            guard_abort, guard_base, q8_early_merge, q8_merge_patience, q8_map_slices, q8_pos, q8_ilv_log
 *   [47..73] its pointer arguments as byte offsets from the workspace base, -1 for NULL, -2 for a buffer of the caller's: codes, valid, lut,
 *            partial, smax, q16, qstep, qlo, qlom, gkey, gk2, gseed, tile_done, out_d, out_i, out_packed, dbg, tile_rows, vmap, item_counter,
 *            cand, cand_count, guard, gate, host_stats, gseed0, btab */
#define ANNLITE_SCAN_RESOLVE_FIELDS 74
ANNLITE_API int annlite_debug_scan_resolve(int64_t N, int64_t M, int64_t Ks, int code_bytes, int codes_layout, int64_t B, int64_t k,
                                  int variant, int flags, int64_t D, int64_t V, int split_phase, int64_t seed_rows, int64_t *out,
                                  int64_t n_out);

/* Convert between the PLAIN and the SKEWED code-table layout (uint8 codes).
 * forward (inverse=0): table_out[id][j] = codes_in[i][(j + id) mod M]   -- scatter rows i -> id
 *                      (M = 64: each 32-byte half is rotated by id mod 32 on its own and "wrap-coded" -- minus 1 mod 256
 *                      where j mod 32 + id mod 32 >= 32 -- the form the M = 64 scan kernel turns into an LDS address with
 *                      one byte permute; SKEWED is an opaque, per-M storage format: always produce and undo it with this
 *                      function)
 * inverse (inverse=1): codes_out[i][j]  = table_in[id][(j - id) mod M]  -- gather rows id -> i
 * id = ids_dev[i] if ids_dev != NULL else id_base + i.  This is the storage step of the index
 * plugin's add_with_ids (annlite/core/index/pq_index.py:25-27 -> flat_index.py:41-50 `_data[ids] = x`). */
ANNLITE_API int annlite_codes_skew(const void *in_dev, int64_t N, int64_t M, const int64_t *ids_dev, int64_t id_base,
                       void *out_dev, int inverse, void *stream);

/* Merge G sorted candidate lists per query into one: in [G][B][k] -> out [B][k], same order rule.
 * This is the step after the RCCL all-gather of per-shard top-k; the
 * reference's analogue is the hstack+argsort merge of per-cell results (annlite/container.py:130-138). */
ANNLITE_API int annlite_topk_merge(const float *dist_dev, const int64_t *id_dev, int64_t G, int64_t B, int64_t k,
                       float *out_dist_dev, int64_t *out_id_dev, void *stream);

/* The same merge over the packed form of annlite_adc_scan_topk_packed: in i64 [G][B][k][2]. */
ANNLITE_API int annlite_topk_merge_packed(const int64_t *packed_dev, int64_t G, int64_t B, int64_t k,
                              float *out_dist_dev, int64_t *out_id_dev, int flags, void *stream);

/* Row-wise k smallest of a dense f32 matrix [B][N] -> ([B][k], [B][k]) with the fixed tie-break.
 * replaces: annlite.math.top_k(values, k, descending=False) (annlite/math.py:94-120). k <= 64. */
ANNLITE_API int annlite_topk_rows(const float *values_dev, int64_t B, int64_t N, int64_t k, int64_t id_base,
                      float *out_dist_dev, int64_t *out_id_dev, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Codec.
 * ---------------------------------------------------------------------------------------------- */
/* replaces: PQCodec.encode (annlite/core/codec/pq.py:158-177): codes[n][m] = argmin_k |x_sub - C[m,k]|^2,
 * first minimum wins.  out codes [N][M] of code_bytes (1 if Ks<=256, 2 if Ks<=65536: pq.py:56-60). */
ANNLITE_API int annlite_pq_encode(const float *x_dev, int64_t N, int64_t D, const float *codebooks_dev, int64_t M,
                      int64_t Ks, void *out_codes_dev, int code_bytes, void *stream);

/* replaces: PQCodec.decode (annlite/core/codec/pq.py:179-198): gather codewords. out f32 [N][D] */
ANNLITE_API int annlite_pq_decode(const void *codes_dev, int code_bytes, int64_t N, int64_t M, int64_t Ks,
                      const float *codebooks_dev, int64_t dsub, float *out_dev, void *stream);

/* replaces: annlite.math.l2_normalize (annlite/math.py:6-18): rows with norm < 10*eps unscaled.
 * In-place allowed (out_dev == x_dev). */
ANNLITE_API int annlite_l2_normalize(const float *x_dev, int64_t N, int64_t D, float *out_dev, void *stream);

/* One Lloyd iteration building block for PQCodec.fit (annlite/core/codec/pq.py:89-115, sklearn KMeans
 * per sub-space): assign every training row to its nearest codeword in every sub-space and accumulate
 * per-codeword sums/counts.  sums_dev f32 [M][Ks][dsub], counts_dev i32 [M][Ks] (both zeroed by the
 * caller), inertia_dev f64 [M] (zeroed by caller, may be NULL). */
ANNLITE_API int annlite_kmeans_assign_accumulate(const float *x_dev, int64_t N, int64_t D, const float *codebooks_dev,
                                     int64_t M, int64_t Ks, float *sums_dev, int32_t *counts_dev,
                                     double *inertia_dev, void *stream);
/* codebooks[m][k] = sums/counts where counts > 0 (empty clusters keep their old centre). */
ANNLITE_API int annlite_kmeans_update(const float *sums_dev, const int32_t *counts_dev, int64_t M, int64_t Ks,
                          int64_t dsub, float *codebooks_dev, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Exact re-rank (GPU analogue of FlatIndex.search,
 * annlite/core/index/flat_index.py:15-39, and hnswlib's space_l2.h/space_ip.h distance functions):
 * out[b][r] = exact distance between queries[b] and vectors[cand[b][r]] (cand < 0 -> +inf).
 * metric EUCLIDEAN -> squared L2 ; INNER_PRODUCT / COSINE -> 1 - <q, x> (inputs already normalised
 * for COSINE).  vectors_dev f32 [N][D]. */
ANNLITE_API int annlite_exact_gather_dist(int metric, const float *queries_dev, int64_t B, int64_t D,
                              const float *vectors_dev, int64_t N, const int64_t *cand_dev, int64_t R,
                              float *out_dev, void *stream);
/* annlite_exact_gather_dist over vectors_f16_dev f16 [N][D] (FlatGpuIndex's half-precision row store): every value is widened exactly
 * and the arithmetic after the load is the f32 form's, so the result is annlite_exact_gather_dist's over the widened rows, bit for bit.
 * No reference counterpart (the reference casts to its dtype on the host, hnsw/index.py:20-48, and hnswlib computes in f32). */
ANNLITE_API int annlite_exact_gather_dist_f16(int metric, const float *queries_dev, int64_t B, int64_t D,
                                  const void *vectors_f16_dev, int64_t N, const int64_t *cand_dev, int64_t R,
                                  float *out_dev, void *stream);
/* annlite_exact_gather_dist over vectors_i8_dev int8 [N][D] (FlatGpuIndex's int8 row store): a code c stands for scale * c, scale a
 * power of two in [2^-24, 2^24] -- the widened value is exact and the arithmetic after it is the f32 form's, so the result is
 * annlite_exact_gather_dist's over the rows scale * c, bit for bit.  No reference counterpart. */
ANNLITE_API int annlite_exact_gather_dist_i8(int metric, const float *queries_dev, int64_t B, int64_t D,
                                 const void *vectors_i8_dev, float scale, int64_t N, const int64_t *cand_dev, int64_t R,
                                 float *out_dev, void *stream);
/* The same distances FUSED with the top-k (round 6): out[b][0..k) = the k smallest exact distances among cand[b][0..R) in
 * (distance, position in the list) order -- what annlite_exact_gather_dist + annlite_topk_rows + a gather of the ids give, bit for
 * bit -- as (distance, cand id); candidates < 0, >= N or cleared in valid_bits_dev (may be NULL) are skipped, missing places hold
 * (+inf, -1).  A valid candidate whose exact distance is +inf is indistinguishable from a missing place and comes back as
 * (+inf, -1) too; NaN distances sort behind every +inf (numpy's order) and keep their id.
 * k <= 64.  flags: ANNLITE_FLAG_SQRT (EUCLIDEAN results, hnsw/index.py:164-165).  One wave per query. */
ANNLITE_API int annlite_rerank_topk(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev, int64_t N,
                        const int64_t *cand_dev, int64_t R, const uint32_t *valid_bits_dev, int64_t k, int flags,
                        float *out_dist_dev, int64_t *out_id_dev, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Exact float32 search over un-quantised vectors.
 * replaces: the reference's default index, AnnLite without n_subvectors -- HnswIndex.search on float vectors
 * (annlite/core/index/hnsw/index.py:139-167) and its brute-force form FlatIndex.search (annlite/core/index/flat_index.py:15-39:
 * cdist + top_k).  The distances are annlite_rerank_topk's, bit for bit (a document searched with its own vector comes back at
 * exactly 0); results ascend by (distance, row id), NaN distances behind +inf; rows cleared in valid_bits_dev never appear.
 * ---------------------------------------------------------------------------------------------- */
/* norms[row] = |vectors[row]|^2 for row = ids_dev[i] (ids_dev != NULL) or id_base + i, i < n: what add / update call for the rows
 * they wrote (flat_index.py:41-50 `_data[ids] = x` has no such array: cdist recomputes the norms in every search). */
ANNLITE_API int annlite_flat_row_norms(const float *vectors_dev, int64_t capacity, int64_t D, const int64_t *ids_dev, int64_t n,
                           int64_t id_base, float *norms_dev, void *stream);
/* Entries a query's candidate list holds (count_dev above it: the list overflowed). */
ANNLITE_API int annlite_flat_list_capacity(void);
/* The two constants of the filter's slack, c_rel * fl(|x|^2 + |q|^2) + c_abs, as the filter kernel is handed them (host only; DESIGN.md
 * section 3.6 derives them).  No reference counterpart. */
ANNLITE_API int annlite_flat_slack(int metric, int64_t D, float *c_rel, float *c_abs);
/* The filter stage alone (f32 MFMA contraction; flat_index.py:29 `cdist`): over the rows 0, stride, 2 stride, ... < N that are set in
 * valid_bits_dev (may be NULL), every row whose exact distance to queries[b] (raw: squared L2, or 1 - <q, x>) is <= bounds_dev[b]
 * is appended to cand_dev i32 [B][annlite_flat_list_capacity()], in no particular order, together with the few rows the proven
 * slack lets through; count_dev i32 [B] (zeroed by the caller) counts them.  A NaN or infinite bound passes every row.
 * query_norms_dev f32 [B] = annlite_flat_row_norms of the queries. */
ANNLITE_API int annlite_flat_filter(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev,
                        const float *norms_dev, int64_t N, int64_t stride, const uint32_t *valid_bits_dev,
                        const float *query_norms_dev, const float *bounds_dev, int32_t *cand_dev, int32_t *count_dev, void *stream);
ANNLITE_API int annlite_flat_search_workspace_bytes(int64_t N, int64_t D, int64_t B, int64_t k, int64_t *bytes);
/* The search (flat_index.py:15-39, hnsw/index.py:139-167): out [B][k] = the k nearest valid rows of vectors_dev f32 [N][D], (+inf, -1)
 * where the table has fewer.  norms_dev f32 [N] from annlite_flat_row_norms.  1 <= k <= 64, N < 2^31.  flags: ANNLITE_FLAG_SQRT
 * (EUCLIDEAN results, hnsw/index.py:164-165).  COSINE expects normalised rows and queries. */
ANNLITE_API int annlite_flat_search_topk(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev,
                             const float *norms_dev, int64_t N, const uint32_t *valid_bits_dev, int64_t k, int flags,
                             float *out_dist_dev, int64_t *out_id_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
/* Queries of the last annlite_flat_search_topk on this workspace whose final candidate list overflowed (they were answered by exact
 * sums over all rows).  Synchronises the stream.  No reference counterpart. */
ANNLITE_API int annlite_flat_overflow_count(const void *workspace_dev, void *stream, int64_t *count);
/* count_dev i32 [B] = how many rows the LAST filter stage of the last search on this workspace (annlite_flat_search_topk or
 * annlite_ivf_flat_search_topk with the same B) offered each query's list; above annlite_flat_list_capacity(): overflowed.
 * Undefined after a search that ran no filter.  For measurements; no reference counterpart. */
ANNLITE_API int annlite_flat_list_counts(const void *workspace_dev, int64_t B, int32_t *count_dev, void *stream);

/* The same search with the SPLIT filter ("split filter"): the filter contracts c = fl(x - centre) (centre f32 [D];
 * NULL: c = x) carried as two bf16 numbers, c_h + c_l, on three bf16 MFMAs; its slack is relative to |x - centre|^2 + |q - centre|^2, so
 * data with a large common offset no longer passes every row.  The exact stage and therefore the answer are annlite_flat_search_topk's,
 * bit for bit.  1 <= D <= 32768.  A centre is taken for EUCLIDEAN only (another metric with one: an error).  No reference counterpart. */
/* The split filter's (c_rel, c_abs) (host only). */
ANNLITE_API int annlite_flat_split_slack(int metric, int64_t D, float *c_rel, float *c_abs);
/* annlite_flat_row_norms over fl(vectors[row] - centre): the norms column the split filter reads when it has a centre. */
ANNLITE_API int annlite_flat_centred_norms(const float *vectors_dev, int64_t capacity, int64_t D, const int64_t *ids_dev, int64_t n,
                               int64_t id_base, const float *centre_dev, float *norms_dev, void *stream);
ANNLITE_API int annlite_flat_search_split_workspace_bytes(int64_t N, int64_t D, int64_t B, int64_t k, int64_t *bytes);
/* annlite_flat_filter with the split filter.  norms_dev: annlite_flat_centred_norms with the same centre (annlite_flat_row_norms without
 * one).  The queries are centred and split into the workspace (annlite_flat_search_split_workspace_bytes of the same B, D) by this call;
 * query_norms_out_dev (may be NULL) f32 [B] receives |fl(q - centre)|^2 as the filter used it.  scores_dev (may be NULL; tests and
 * measurements) f32 [B][ceil(N / stride)] receives the filter's score v of every (query, stage row) pair, valid or not. */
ANNLITE_API int annlite_flat_filter_split(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev,
                              const float *norms_dev, int64_t N, int64_t stride, const uint32_t *valid_bits_dev,
                              float *query_norms_out_dev, const float *bounds_dev, int32_t *cand_dev, int32_t *count_dev,
                              const float *centre_dev, float *scores_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
/* annlite_flat_search_topk with the split filter: the same stages, lists, capacity and overflow route (annlite_flat_overflow_count and
 * annlite_flat_list_counts read this workspace too).  norms_dev as for annlite_flat_filter_split. */
ANNLITE_API int annlite_flat_search_topk_split(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev,
                                   const float *norms_dev, int64_t N, const uint32_t *valid_bits_dev, const float *centre_dev, int64_t k,
                                   int flags, float *out_dist_dev, int64_t *out_id_dev, void *workspace_dev, size_t workspace_bytes,
                                   void *stream);

/* The same search over rows STORED in half precision ("f16 rows"): vectors_f16_dev f16 [N][D], rounded once
 * when they were written; queries stay f32.  replaces: the reference's `dtype` argument of its index plug-ins (BaseIndex(dim, dtype=...),
 * HnswIndex.pre_process casts to it, annlite/core/index/hnsw/index.py:20-48).  The answer is annlite_flat_search_topk's over the rows
 * widened back to f32, bit for bit.  An f16 row is an exact MFMA operand: the filter contracts it with the query carried as two f16
 * numbers (scaled by a power of two per query) on two f16 MFMAs.  1 <= D <= 32768. */
/* annlite_flat_row_norms over f16 rows (flat_norms_kernel's chain on the widened values).  No reference counterpart. */
ANNLITE_API int annlite_flat_row_norms_f16(const void *vectors_f16_dev, int64_t capacity, int64_t D, const int64_t *ids_dev, int64_t n,
                               int64_t id_base, float *norms_dev, void *stream);
/* The f16 filter's (c_rel, c_abs) (host only); its slack is c_rel * fl(|x|^2 + |q|^2) + c_abs + a per-query term the library computes,
 * 1.001 * 2^-13 * sum |q_j| (what a flush of f16 subnormal row operands inside the MFMA could cost).  No reference counterpart. */
ANNLITE_API int annlite_flat_f16_slack(int metric, int64_t D, float *c_rel, float *c_abs);
/* No reference counterpart. */
ANNLITE_API int annlite_flat_search_f16_workspace_bytes(int64_t N, int64_t D, int64_t B, int64_t k, int64_t *bytes);
/* annlite_flat_filter over f16 rows.  norms_dev: annlite_flat_row_norms_f16.  The queries are scaled and split into the workspace
 * (annlite_flat_search_f16_workspace_bytes of the same B, D) by this call; query_norms_out_dev / query_flush_out_dev (may be NULL) f32 [B]
 * receive |q|^2 and the per-query slack term as the filter used them; scores_dev (may be NULL; tests and measurements)
 * f32 [B][ceil(N / stride)] receives the filter's score v of every (query, stage row) pair, valid or not.  No reference counterpart. */
ANNLITE_API int annlite_flat_filter_f16(int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_f16_dev,
                            const float *norms_dev, int64_t N, int64_t stride, const uint32_t *valid_bits_dev,
                            float *query_norms_out_dev, float *query_flush_out_dev, const float *bounds_dev, int32_t *cand_dev,
                            int32_t *count_dev, float *scores_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
/* annlite_flat_search_topk over f16 rows: the same stages, lists, capacity and overflow route (annlite_flat_overflow_count and
 * annlite_flat_list_counts read this workspace too).  replaces: HnswIndex.search / FlatIndex.search of an index built with
 * dtype=np.float16. */
ANNLITE_API int annlite_flat_search_topk_f16(int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_f16_dev,
                                 const float *norms_dev, int64_t N, const uint32_t *valid_bits_dev, int64_t k, int flags,
                                 float *out_dist_dev, int64_t *out_id_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* The same search over rows STORED as int8 codes ("int8 rows"): vectors_i8_dev int8 [N][D], a byte c in
 * [-127, 127] standing for the value scale * c, `scale` a power of two in [2^-24, 2^24] (anything else: ANNLITE_ERR_INVALID); queries
 * stay f32.  replaces: the reference's `dtype` argument of its index plug-ins, as the f16 form does.  The answer is
 * annlite_flat_search_topk's over the f32 rows scale * c, bit for bit.  An int8 row is an exact MFMA operand and the accumulator an
 * integer: the filter contracts it with the query rounded to a 21-bit integer (scaled by a power of two per query) and carried as three
 * base-128 digits, on three i8 MFMAs -- the contraction itself has no rounding error.  1 <= D <= 32768. */
/* annlite_flat_row_norms over int8 rows (flat_norms_kernel's chain on the widened values scale * c).  No reference counterpart. */
ANNLITE_API int annlite_flat_row_norms_i8(const void *vectors_i8_dev, float scale, int64_t capacity, int64_t D, const int64_t *ids_dev,
                              int64_t n, int64_t id_base, float *norms_dev, void *stream);
/* The int8 filter's (c_rel, c_abs) (host only; they do not depend on the scale); its slack is c_rel * fl(|x|^2 + |q|^2) + c_abs + a
 * per-query term the library computes, 1.001 * 127 * D * 2^-e with 2^e the query's power of two (what rounding the scaled query to
 * integers can cost against codes of magnitude <= 127; +inf for a query that has no integer form).  No reference counterpart. */
ANNLITE_API int annlite_flat_i8_slack(int metric, int64_t D, float *c_rel, float *c_abs);
/* No reference counterpart. */
ANNLITE_API int annlite_flat_search_i8_workspace_bytes(int64_t N, int64_t D, int64_t B, int64_t k, int64_t *bytes);
/* annlite_flat_filter over int8 rows.  norms_dev: annlite_flat_row_norms_i8 with the same scale.  The queries are scaled, rounded and
 * split into the workspace (annlite_flat_search_i8_workspace_bytes of the same B, D) by this call; query_norms_out_dev /
 * query_slack_out_dev (may be NULL) f32 [B] receive |q|^2 and the per-query slack term as the filter used them; scores_dev (may be NULL;
 * tests and measurements) f32 [B][ceil(N / stride)] receives the filter's score v of every (query, stage row) pair, valid or not.
 * No reference counterpart. */
ANNLITE_API int annlite_flat_filter_i8(int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_i8_dev, float scale,
                           const float *norms_dev, int64_t N, int64_t stride, const uint32_t *valid_bits_dev,
                           float *query_norms_out_dev, float *query_slack_out_dev, const float *bounds_dev, int32_t *cand_dev,
                           int32_t *count_dev, float *scores_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
/* annlite_flat_search_topk over int8 rows: the same stages, lists, capacity and overflow route (annlite_flat_overflow_count and
 * annlite_flat_list_counts read this workspace too).  replaces: HnswIndex.search / FlatIndex.search of an index built with
 * dtype=np.int8. */
ANNLITE_API int annlite_flat_search_topk_i8(int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_i8_dev,
                                float scale, const float *norms_dev, int64_t N, const uint32_t *valid_bits_dev, int64_t k, int flags,
                                float *out_dist_dev, int64_t *out_id_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* The same searches over SELECTED rows ("selected rows"): rows_dev i32 [n_sel], ascending offsets < N -- the set
 * bits of a filter's bitmap (annlite_bitmap_rows) -- take the place of the table: the first sample, the filter stages and the overflow
 * route run over the list as they run over a table of n_sel rows, each row one indirection away, so the work follows n_sel, not N.
 * No bitmap is read: a row in the list is selected (an entry outside [0, N) is skipped).  The answer is, bit for bit, that of the search
 * over the whole table with the list's rows as its bitmap.
 *   filter       ANNLITE_FLAT_FILTER_*: the filter and with it the row type of vectors_dev -- F32 and BF16X3: f32 [N][D]; F16X2: f16;
 *                I8X3: int8 codes of value row_scale * c (row_scale is read by I8X3 only)
 *   norms_dev    the norms that filter takes in its table form (BF16X3 with a centre: annlite_flat_centred_norms)
 *   centre_dev   BF16X3 + EUCLIDEAN: the centre, or NULL; every other filter: NULL
 * replaces: the reference's filtered search (annlite/index.py: the offsets CellTable.query yields, handed to the index as `indices`). */
#define ANNLITE_FLAT_FILTER_F32 0
#define ANNLITE_FLAT_FILTER_BF16X3 1
#define ANNLITE_FLAT_FILTER_F16X2 2
#define ANNLITE_FLAT_FILTER_I8X3 3
/* No reference counterpart. */
ANNLITE_API int annlite_flat_search_rows_workspace_bytes(int filter, int64_t n_sel, int64_t D, int64_t B, int64_t k, int64_t *bytes);
/* Outputs, order, padding, flags, lists and overflow route as annlite_flat_search_topk (annlite_flat_overflow_count and
 * annlite_flat_list_counts read this workspace too); n_sel <= 4096: exact sums over the list, no filter.  rows_dev is never NULL. */
ANNLITE_API int annlite_flat_search_topk_rows(int filter, int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_dev,
                                  float row_scale, const float *norms_dev, const float *centre_dev, int64_t N, const int32_t *rows_dev,
                                  int64_t n_sel, int64_t k, int flags, float *out_dist_dev, int64_t *out_id_dev, void *workspace_dev,
                                  size_t workspace_bytes, void *stream);
/* ONE filter stage over every stride-th entry of the list (tests and measurements, as annlite_flat_filter_f16 / _i8 are over the
 * table): cand_dev / count_dev / bounds_dev as annlite_flat_filter, the candidates OFFSETS; scores_dev (may be NULL; not with F32) f32
 * [B][ceil(n_sel / stride)] receives the filter's score of every (query, stage row) pair BY LIST POSITION.  The queries are prepared
 * into the workspace (annlite_flat_search_rows_workspace_bytes of the same filter, B, D) by this call.  No reference counterpart. */
ANNLITE_API int annlite_flat_filter_rows(int filter, int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_dev,
                             float row_scale, const float *norms_dev, const float *centre_dev, int64_t N, const int32_t *rows_dev,
                             int64_t n_sel, int64_t stride, const float *bounds_dev, int32_t *cand_dev, int32_t *count_dev, float *scores_dev,
                             void *workspace_dev, size_t workspace_bytes, void *stream);

/* The same searches with A FILTER PER QUERY ("a filter per query"): one batch, G row bitmaps.
 *   masks_dev    u32 [G][mask_ld], 32 mask_ld >= N: bitmap g in valid_bits_dev's word layout -- bit r set: row r is selected by filter g
 *                AND live (the caller ANDs the live bitmap in)
 *   group_dev    i32 [B]: the bitmap of every query, in [0, G).  A query whose id lies outside that range selects NOTHING: no bitmap
 *                is read for it and its answer is all (+inf, -1)
 *   valid_bits_dev  the table's live bitmap or NULL, as in the table searches: it only decides which rows of a row tile are staged
 *                and scored (the union of the G selections); whether a (query, row) pair is admitted is decided by the query's bitmap
 *   filter, vectors_dev, row_scale, norms_dev, centre_dev: as in the selected-rows entries above
 * Query b's answer is, bit for bit, that of the filter's table search for that query with masks_dev[group_dev[b]] as its bitmap.  The
 * stages, the lists and the overflow route are the table search's (annlite_flat_overflow_count and annlite_flat_list_counts read this
 * workspace too): a query whose bitmap keeps fewer than k of the 4096 sampled rows takes the all-rows route under its own bitmap.
 * replaces: one filtered search per distinct filter of a batch (annlite/index.py: `filter` is one dict per call).
 * No reference counterpart. */
ANNLITE_API int annlite_flat_search_grouped_workspace_bytes(int filter, int64_t N, int64_t D, int64_t B, int64_t k, int64_t *bytes);
ANNLITE_API int annlite_flat_search_topk_grouped(int filter, int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_dev,
                                     float row_scale, const float *norms_dev, const float *centre_dev, int64_t N,
                                     const uint32_t *valid_bits_dev, const uint32_t *masks_dev, int64_t mask_ld, int64_t G,
                                     const int32_t *group_dev, int64_t k, int flags, float *out_dist_dev, int64_t *out_id_dev,
                                     void *workspace_dev, size_t workspace_bytes, void *stream);
/* ONE grouped filter stage over every stride-th row of the table (tests and measurements): cand_dev / count_dev / bounds_dev as
 * annlite_flat_filter; scores_dev (may be NULL; not with F32) f32 [B][ceil(N / stride)] as the table stages have it.  The queries are
 * prepared into the workspace (annlite_flat_search_grouped_workspace_bytes of the same filter, B, D) by this call. */
ANNLITE_API int annlite_flat_filter_grouped(int filter, int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_dev,
                                float row_scale, const float *norms_dev, const float *centre_dev, int64_t N, const uint32_t *valid_bits_dev,
                                const uint32_t *masks_dev, int64_t mask_ld, int64_t G, const int32_t *group_dev, int64_t stride,
                                const float *bounds_dev, int32_t *cand_dev, int32_t *count_dev, float *scores_dev, void *workspace_dev,
                                size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Cells over float vectors: the exact search above restricted to the rows of each query's P probed cells.
 * replaces: the reference's n_cells > 1 structure over its default float index -- AnnLite._cell_selection's consumers, one float
 * index per cell and the hstack / argsort merge of CellContainer.ivf_search (annlite/container.py:88-144) -- with n_probe < n_cells
 * (the reference itself always visits every cell, index.py:94: that is annlite_flat_search_topk).
 * The vectors stay where they are; the cells are a permutation:
 *   perm_dev       i32 [n_perm]  offsets of the live rows grouped by cell, ascending inside a cell
 *   cell_rows_dev  i64 [C][2]    (begin, end) of every cell in perm_dev
 *   cell_order_dev i32 [C]       cells by descending size
 *   cells_dev      i32 [B][P]    the probed cells of every query (annlite_ivf_select_cells; distinct per query; an id outside
 *                                [0, C) is read as cell 0, as annlite_ivf_plan reads it)
 * Result: per query the k nearest of the rows of its cells that are set in valid_bits_dev (may be NULL) -- distances, order and
 * padding exactly as annlite_flat_search_topk, i.e. annlite_rerank_topk's arithmetic over those rows.
 * ---------------------------------------------------------------------------------------------- */
/* The strides the search uses for a query that probes at most max_probed_rows rows (host only; no reference counterpart):
 * strides_out[0] = the first exact sample takes every strides_out[0]-th entry of each probed cell, strides_out[1 ..] = the filter
 * stages', descending to 1.  *n_out = how many (at most 16; 0: exact sums over all probed rows, no filter). */
ANNLITE_API int annlite_ivf_flat_stages(int64_t max_probed_rows, int64_t *strides_out, int *n_out);
ANNLITE_API int annlite_ivf_flat_search_workspace_bytes(int64_t B, int64_t P, int64_t C, int64_t k, int64_t *bytes);
/* max_cell_rows = the largest cell's length (bounds the filter's grid: rows of a longer cell would not be seen), max_probed_rows =
 * the sum of the P largest lengths (chooses the stages; any value is correct).  C <= 16384, 1 <= k <= 64, N < 2^31.  All launches
 * on `stream`, no host round trip; annlite_flat_overflow_count(workspace) counts the queries that took the slower route. */
ANNLITE_API int annlite_ivf_flat_search_topk(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev,
                                 const float *norms_dev, int64_t N, const uint32_t *valid_bits_dev, const int32_t *cells_dev,
                                 int64_t P, int64_t C, const int32_t *perm_dev, int64_t n_perm, const int64_t *cell_rows_dev,
                                 const int32_t *cell_order_dev, int64_t max_cell_rows, int64_t max_probed_rows, int64_t k,
                                 int flags, float *out_dist_dev, int64_t *out_id_dev, void *workspace_dev, size_t workspace_bytes,
                                 void *stream);

/* The same search with the SPLIT filter over the cell tiles ("split filter over cell tiles"): replaces the
 * f32 filter stage of annlite_ivf_flat_search_topk with annlite_flat_search_topk_split's contraction -- three bf16 MFMAs over centred
 * values -- where the centre of a (cell, queries) tile is the CENTROID OF ITS CELL: centres_dev f32 [C][D] (NULL: no centring; a
 * centre is taken for EUCLIDEAN only), cell_of_dev i32 [capacity] the cell of every row offset.  The slack is relative to
 * |x - centroid|^2 + |q - centroid|^2, so data with a common offset no longer passes every probed row.  The exact stages and
 * therefore the answer are annlite_ivf_flat_search_topk's, bit for bit.  1 <= D <= 32768.  No reference counterpart. */
/* annlite_flat_centred_norms with the centre chosen per row: norms_dev[row] = |fl(vectors[row] - centres[cell_of[row]])|^2, the norms
 * column the split filter reads when it has centres.  A cell id outside [0, C) reads cell 0, as annlite_ivf_plan does. */
ANNLITE_API int annlite_ivf_flat_centred_norms(const float *vectors_dev, int64_t capacity, int64_t D, const int64_t *ids_dev, int64_t n,
                                   int64_t id_base, const float *centres_dev, int64_t C, const int32_t *cell_of_dev, float *norms_dev,
                                   void *stream);
ANNLITE_API int annlite_ivf_flat_search_split_workspace_bytes(int64_t B, int64_t P, int64_t C, int64_t D, int64_t k, int64_t *bytes);
/* The split filter stage alone (tests and measurements): the annlite_flat_filter_split of the cells.  The call plans the tiles,
 * centres and splits the queries of every (query, probe) pair into the workspace (annlite_ivf_flat_search_split_workspace_bytes of
 * the same B, P, C, D) and filters every stride-th entry of each probed cell against bounds_dev f32 [B].  norms_dev:
 * annlite_ivf_flat_centred_norms with the same centres (annlite_flat_row_norms without).  cand_dev i32 [B][capacity] /
 * count_dev i32 [B] (zeroed by the caller) as annlite_flat_filter; pair_norms_out_dev (may be NULL) f32 [B][P] receives
 * |fl(q - centre of the pair's cell)|^2 as the filter used it; scores_dev (may be NULL) f32 [B][N] receives the filter's score v by
 * (query, row offset) for every pair it evaluated -- a row that is not valid or not probed keeps the caller's value. */
ANNLITE_API int annlite_ivf_flat_filter_split(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev,
                                  const float *norms_dev, int64_t N, const uint32_t *valid_bits_dev, const int32_t *cells_dev,
                                  int64_t P, int64_t C, const int32_t *perm_dev, int64_t n_perm, const int64_t *cell_rows_dev,
                                  const int32_t *cell_order_dev, int64_t max_cell_rows, int64_t stride, const float *centres_dev,
                                  const int32_t *cell_of_dev, const float *bounds_dev, int32_t *cand_dev, int32_t *count_dev,
                                  float *pair_norms_out_dev, float *scores_dev, void *workspace_dev, size_t workspace_bytes,
                                  void *stream);
/* annlite_ivf_flat_search_topk with the split filter: the same stages, lists, capacity and overflow route (annlite_flat_overflow_count
 * and annlite_flat_list_counts read this workspace too).  norms_dev as for annlite_ivf_flat_filter_split. */
ANNLITE_API int annlite_ivf_flat_search_topk_split(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev,
                                       const float *norms_dev, int64_t N, const uint32_t *valid_bits_dev, const int32_t *cells_dev,
                                       int64_t P, int64_t C, const int32_t *perm_dev, int64_t n_perm, const int64_t *cell_rows_dev,
                                       const int32_t *cell_order_dev, int64_t max_cell_rows, int64_t max_probed_rows,
                                       const float *centres_dev, const int32_t *cell_of_dev, int64_t k, int flags, float *out_dist_dev,
                                       int64_t *out_id_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Pruned (IVF) search over cells (follow-on of rank 4).
 * Reference structure: AnnLite(n_cells > 1): VQCodec coarse quantiser (annlite/core/codec/vq.py),
 * AnnLite._cell_selection (annlite/index.py:458-466: cdist(query, vq codebook) -> top_k(n_probe)),
 * CellContainer.ivf_search (annlite/container.py:88-144: one index per cell, lists merged).  The
 * reference always probes every cell (n_probe = max(n_probe, n_cells), index.py:94); probing fewer
 * is this build's extension of the same structure.
 * Table layout: the rows of a cell are CONTIGUOUS in the code table, every cell starts at a multiple
 * of 64 rows (padding rows are invalid in the bitmap), rows of a cell ascend in external id.
 * ---------------------------------------------------------------------------------------------- */
/* cells[b][0..P) = the P nearest centroids of query b, ascending in (distance, cell).
 * kind 0: squared L2; kind 1: negative inner product (cosine: pass normalised centroids).
 * centroids_dev f32 [C][D] (VQCodec.codebook). */
ANNLITE_API int annlite_ivf_select_cells(int kind, const float *queries_dev, int64_t B, int64_t D,
                             const float *centroids_dev, int64_t C, int64_t P, int32_t *cells_dev, void *stream);

/* Upper bound of the query tiles annlite_ivf_plan can produce (qt = tile size of the scan plan). */
ANNLITE_API int64_t annlite_ivf_max_tiles(int64_t B, int64_t P, int64_t C, int64_t qt);

/* Group the B*P (query, cell) pairs into query tiles of qt slots that probe ONE cell each.
 *   cell_rows_dev  i64 [C][2]  (begin, end) rows of every cell in the code table
 *   cell_order_dev i32 [C]     cells in descending size (tiles are scanned longest first)
 *   vmap_dev       i32 [n_tiles_max*qt]  out: query of every slot, -1 = padding slot
 *   slot_of_dev    i32 [B*P]   out: slot of pair (b, p)
 *   tile_rows_dev  i64 [n_tiles_max][2]  out: row range of every tile (begin -1: unused tile)
 *   n_tiles_used_dev i32 [1]   out (may be NULL) */
ANNLITE_API int annlite_ivf_plan(const int32_t *cells_dev, int64_t B, int64_t P, int64_t C, int64_t qt,
                     const int64_t *cell_rows_dev, const int32_t *cell_order_dev, int64_t n_tiles_max,
                     int32_t *vmap_dev, int32_t *slot_of_dev, int64_t *tile_rows_dev, int32_t *n_tiles_used_dev,
                     void *stream);

/* ... with two classes of tiles: the pairs of every query's n_first nearest cells (probe ranks < n_first) in tiles of their own that
 * come FIRST, the other pairs behind them (annlite_ivf_search_topk: the scan shares a query's bound between its tiles; the k best
 * rows of the nearest cells then bound the candidates of the others from the start).  n_tiles_max >= annlite_ivf_max_tiles_first.
 * n_first = 0 or >= P: annlite_ivf_plan.  Two classes double the kernel's per-cell counters: (4 C + 16) * 4 bytes of LDS, so
 * C <= 10236 with 0 < n_first < P (ANNLITE_ERR_INVALID above, nothing launched); one class serves C up to 16384. */
ANNLITE_API int64_t annlite_ivf_max_tiles_first(int64_t B, int64_t P, int64_t C, int64_t qt);
ANNLITE_API int annlite_ivf_plan_first(const int32_t *cells_dev, int64_t B, int64_t P, int64_t C, int64_t qt,
                           const int64_t *cell_rows_dev, const int32_t *cell_order_dev, int64_t n_tiles_max,
                           int32_t *vmap_dev, int32_t *slot_of_dev, int64_t *tile_rows_dev, int32_t *n_tiles_used_dev,
                           int64_t n_first, void *stream);

/* The scan of annlite_pq_search_topk where query tile t = slots [t*qt, (t+1)*qt) scans ONLY rows
 * tile_rows[t] (one work item per tile, handed out dynamically) -- with INTEGER sums only: a tile is
 * too short to amortise exact fp32 recomputes.  The kernel keeps, per slot, the k smallest integer
 * sums (which bound the slot's k-th exact distance from above: any k rows with S <= Sk give
 * d_kth <= L + step*(Sk + 1.002 M) + slack) and EMITS every row that can still be in the slot's exact
 * top-k:  cand[v][0..cand_count[v])  (table rows; cand_count 0xffffffff = the list overflowed
 * cand_cap, re-score the whole cell).  annlite_ivf_rescore turns the lists into exact results.
 * queries_dev f32 [B][D]: the REAL queries -- their tables are built and quantised once; slot s of
 * the V = n_tiles * qt slots scans with the tables of query vmap[s] (-1: padding slot).
 * Quantised-filter plans only (M in {8,16,32,64}, Ks <= 256, uint8 codes). */
ANNLITE_API int annlite_pq_search_tiles_workspace_bytes(int64_t N, int64_t M, int64_t Ks, int code_bytes, int64_t V,
                                            int64_t k, int64_t *bytes);
ANNLITE_API int annlite_pq_search_tiles(int lut_kind, const float *queries_dev, int64_t B, int64_t D,
                            const float *codebooks_dev, const void *codes_dev, int code_bytes, int codes_layout,
                            int64_t N, int64_t M, int64_t Ks, const uint32_t *valid_bits_dev, int64_t k, int64_t V,
                            const int64_t *tile_rows_dev, const int32_t *vmap_dev, uint32_t *cand_dev,
                            int64_t cand_cap, uint32_t *cand_count_dev, void *workspace_dev, size_t workspace_bytes,
                            void *stream);

/* Exact re-score + merge, one workgroup per query: the query's fp32 table lut_bmk[b] ([M][Ks], what
 * get_dist_mat returns) in LDS, exact ascending-m ADC sums (space_pq.h:32-35) of the candidate rows of
 * its P probed slots (slot_of_dev i32 [B][P]), top-k under the fixed tie-break -> [B][k] (distance,
 * id_base + row_ids[row]).  codes_plain_dev: the cell-sorted table in the PLAIN layout [N][M];
 * valid_bits_dev (may be NULL) is consulted for overflowed slots, which are re-scored over
 * tile_rows[slot / qt].  flags: ANNLITE_FLAG_SQRT.
 * replaces: the per-cell search + hstack/argsort merge of CellContainer.ivf_search
 * (annlite/container.py:88-144). */
ANNLITE_API int annlite_ivf_rescore(const float *lut_bmk_dev, int64_t B, int64_t M, int64_t Ks,
                        const void *codes_plain_dev, int64_t N, const uint32_t *valid_bits_dev,
                        const uint32_t *cand_dev, int64_t cand_cap, const uint32_t *cand_count_dev,
                        const int32_t *slot_of_dev, int64_t P, const int64_t *tile_rows_dev, int64_t qt,
                        const int64_t *row_ids_dev, int64_t id_base, int64_t k, float *out_dist_dev,
                        int64_t *out_id_dev, int flags, void *stream);

/* The candidate lists of every query as ONE dense id row: out_ids[b][0..R) = its P lists back to
 * back (id_base + row_ids[row]), padded with -1 -- the input of annlite_exact_gather_dist when the
 * index keeps the float vectors (re-rank).  Overflowed lists contribute
 * nothing and entries beyond R are dropped (the re-rank candidate set is a heuristic). */
ANNLITE_API int annlite_ivf_candidate_ids(const uint32_t *cand_dev, int64_t cand_cap, const uint32_t *cand_count_dev,
                              const int32_t *slot_of_dev, int64_t B, int64_t P, const int64_t *row_ids_dev,
                              int64_t id_base, int64_t *out_ids_dev, int64_t R, void *stream);

/* (round 6) The pruned search over cells on the BYTE-TABLE kernel, one call: annlite_ivf_plan (tiles of 32 slots that probe one
 * cell each) -> ONE preparation launch (L2 tables of the B real queries, quantisation parameters, every query's first bound from
 * rows of its NEAREST cell -- a bound from rows outside the probed cells would be wrong --, its byte table) -> the scan in cell
 * tiles (exact ascending-m fp32 sums, space_pq.h:32-35 / pq_bindings.pyx:44-45, of the rows that pass the byte filter; a 16-key
 * list per slot; the bounds shared between the tiles of a QUERY's cells) -> annlite_ivf_merge_lists.  Result: for every query the
 * exact top-k, under the fixed order (distance asc, id asc), of the rows of its P probed cells -- bit-equal to
 * annlite_pq_search_tiles + annlite_ivf_rescore and to the oracle's ivf_search.
 *   cells_dev      i32 [B][P]  the probed cells, nearest first (annlite_ivf_select_cells)
 *   codes_dev      u8 [N][16]  the CELL-SORTED table (cell c = rows [cell_rows[c][0], cell_rows[c][1]), begin a multiple of 64), in
 *                  codes_layout; valid_bits_dev (may be NULL): bitmap over TABLE rows; row_ids_dev i64 [N] (may be NULL): external id
 *                  of every table row, ascending inside a cell
 *   cell_order_dev i32 [C]     cells by descending size (the plan's tile order)
 *   lut_kind: ANNLITE_LUT_L2 (pq_bindings.pyx:149-210) or ANNLITE_LUT_IPDIST (float32(1 / Ks) - <q_sub, codeword>, pq_bindings.pyx:214-274 +
 *   pq.py:316-322: INNER_PRODUCT, and COSINE on normalised queries) -- the tables are built inside the preparation launch, the reference's
 *   j-ascending fmaf chains.  flags: ANNLITE_FLAG_SQRT.  Serves M = 16, Ks <= 256, k <= 16, D <= 256, sub-vectors of a multiple of 4
 *   floats; other shapes: annlite_pq_search_tiles + annlite_ivf_rescore.
 * replaces: _cell_selection's consumers -- the per-cell search loop and the hstack / argsort merge of CellContainer.ivf_search
 * (annlite/container.py:88-144) with n_probe < n_cells. */
ANNLITE_API int annlite_ivf_search_topk_workspace_bytes(int64_t B, int64_t P, int64_t C, int64_t M, int64_t Ks, int64_t k,
                                            int64_t *bytes);
ANNLITE_API int annlite_ivf_search_topk(int lut_kind, const float *queries_dev, int64_t B, int64_t D, const float *codebooks_dev, int64_t M,
                            int64_t Ks, const void *codes_dev, int codes_layout, int64_t N, const uint32_t *valid_bits_dev,
                            const int32_t *cells_dev, int64_t P, int64_t C, const int64_t *cell_rows_dev,
                            const int32_t *cell_order_dev, const int64_t *row_ids_dev, int64_t id_base, int64_t k,
                            float *out_dist_dev, int64_t *out_id_dev, int flags, void *workspace_dev, size_t workspace_bytes,
                            void *stream);

/* The same pipeline as the candidate generator of an exact re-rank (IvfPQGpuIndex(rerank=True)): the slots keep PRIVATE lists -- nothing is
 * shared between a query's tiles --, so every (query, probed cell) list is a function of its own cell: the cell's best <= k rows, by
 * exact ADC sum (ties by id), among those at or below the query's first bound (the min(bound_rank * k, 64)-th smallest exact sum of seed
 * rows of its nearest cell: at or above the k-th key of the probed rows for every bound_rank >= 1, so the union of a query's lists holds
 * its exact ADC top-k; the nearest cell's list is never cut).  bound_rank 1 .. 64 trades pool size for time: a looser bound lengthens
 * the far cells' lists (10M rows, 16 of 256 cells, k = 16: rank 1 / 2 / 4 -> 2.44 / 1.72 / 1.21 M q/s, re-ranked recall@10 0.803 / 0.813 /
 * 0.813).  seed_cells_dev (may be NULL) i32 [B]: the entry of the cell table whose rows seed query b's bound instead of cells[b][0] --
 * for a cell table that lists a cell's rows ALSO as parts (IvfPQGpuIndex.rerank_split): the probe names the parts, the seed the whole
 * cell, whose rows must all be probed by that query; the first list may then be cut like the others.  (Entries of the cell table may
 * overlap -- a cell and its parts -- as long as the entries ONE query probes are disjoint row ranges: a row then appears in one list.)
 * out_ids_dev i64 [B][P * k]: list (b, p) at [p * k, (p + 1) * k), ascending by (sum, id), -1 where it is shorter -- the input of
 * annlite_rerank_topk.  Workspace and shapes: annlite_ivf_search_topk's.  (Not in the reference: its cells hold exact vectors or PQ
 * codes, never both.) */
ANNLITE_API int annlite_ivf_search_candidates(int lut_kind, const float *queries_dev, int64_t B, int64_t D, const float *codebooks_dev,
                                  int64_t M, int64_t Ks, const void *codes_dev, int codes_layout, int64_t N,
                                  const uint32_t *valid_bits_dev, const int32_t *cells_dev, int64_t P, int64_t C,
                                  const int64_t *cell_rows_dev, const int32_t *cell_order_dev, const int64_t *row_ids_dev,
                                  int64_t id_base, int64_t k, int64_t bound_rank, const int32_t *seed_cells_dev,
                                  int64_t *out_ids_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* Merge of per-slot lists: lists_dev u64 [V][k] (ordered distance << 32 | table row, ascending, ~0 = none: what the cell-tile scan
 * leaves per slot) -> per query the k smallest of its P slots' keys re-keyed by external id (id_base + row_ids[row]); one wave per
 * query.  replaces: the concatenate + sort at the end of CellContainer.ivf_search (annlite/container.py:131-144). */
ANNLITE_API int annlite_ivf_merge_lists(const uint64_t *lists_dev, int64_t k, const int32_t *slot_of_dev, int64_t B, int64_t P,
                            const int64_t *row_ids_dev, int64_t id_base, float *out_dist_dev, int64_t *out_id_dev, int flags,
                            void *stream);

/* The PCA projector.
 * out[r][o] = sum_k (x[r][k] - sub[k]) M[o][k] + add[o] on f32 MFMA: x_dev f32 [n][Din] with row stride ldx (floats), M_dev f32
 * [Dout][Din] contiguous, sub_dev f32 [Din] and add_dev f32 [Dout] (either may be NULL), out_dev f32 [n][Dout] with row stride ldo;
 * columns of out beyond Dout are not written.  `sub` is subtracted from every element BEFORE the products (one rounding), so a
 * common offset of the rows does not cancel inside the sums.  Every output element is one fma chain over k ascending: the result
 * is the same bits on every run.  n == 0 returns without a launch.
 * replaces: ProjectorCodec.encode / decode = sklearn PCA.transform / inverse_transform (annlite/core/codec/projector.py:109-130):
 * encode with M = components (scaled by 1 / sqrt(explained variance) with whiten), sub = mean; decode with M = the transpose
 * ([D][K] contiguous, scaled by sqrt(explained variance) with whiten), add = mean. */
ANNLITE_API int annlite_affine_rows(const float *x_dev, int64_t n, int64_t Din, int64_t ldx, const float *M_dev, int64_t Dout,
                        const float *sub_dev, const float *add_dev, float *out_dev, int64_t ldo, void *stream);

/* The data pass of a PCA fit: sum_dev f64 [D] += sum_r (x[r] - shift), gram_dev f64 [D][D] += sum_r (x[r] - shift)(x[r] - shift)^T
 * over the n rows of x_dev (f32, row stride ldx); shift_dev f32 [D] is the caller's guess of the mean (any vector is correct, one
 * near the mean keeps the f32 products small).  The rows are cut into chunks of 512 (a constant); per chunk and 128 x 128 tile with
 * tj >= ti the products run as f32 MFMA fma chains over the chunk's rows in order, and a second kernel adds the chunks' partials to
 * the f64 accumulators in chunk order, mirroring the tiles below the diagonal: no atomics, the same bits on every run and every
 * device, gram exactly symmetric (if it was on entry).  1 <= D <= 2048.  Workspace: annlite_pca_accumulate_workspace_bytes.
 * replaces: the data pass of ProjectorCodec.fit / partial_fit = sklearn PCA.fit / IncrementalPCA.partial_fit
 * (annlite/core/codec/projector.py:60-107); the eigen-decomposition of the D x D matrix stays on the host. */
ANNLITE_API int annlite_pca_accumulate_workspace_bytes(int64_t n, int64_t D, int64_t *bytes);
ANNLITE_API int annlite_pca_accumulate(const float *x_dev, int64_t n, int64_t D, int64_t ldx, const float *shift_dev, double *sum_dev,
                           double *gram_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* Filterable columns: a filter over typed columns of the row range, evaluated into the packed row bitmap
 * the searches take as valid_bits.  The host compiles the filter dict (annlite_amd/columns.py) into this program; the kernel takes it
 * BY VALUE as a kernel argument -- it is uniform, the compiler reads it with scalar loads.
 *   leaf: one comparison of one column.  values_dev: i64 [N] (ANNLITE_COL_I64), f64 [N] (ANNLITE_COL_F64; never NaN) or i32 [N]
 *     dictionary codes (ANNLITE_COL_CODE); present_dev u32 [ceil(N / 32)]: bit r = row r has a value of the column's type.  A leaf is
 *     `present && compare`: a row without the value satisfies no comparison, NE and NIN included (SQL NULL).
 *     I64 / F64 ops: LT GT LE GE EQ NE against literals[lit_begin] (lit_count = 1), IN / NIN against literals[lit_begin .. + lit_count)
 *     (lit_count >= 0); the literals are raw 8-byte values of the column's own type.
 *     CODE op: IN_SET -- bit `code` of set_bits_dev u32 [set_words] (a code at or beyond 32 * set_words is not in the set).
 *   code: postfix over a stack of booleans, one u32 of bits per lane: 0 .. 31 push leaf i; AND / OR pop two and push one; NOT negates
 *     the top; TRUE pushes 1.  The stack never underflows, never holds more than ANNLITE_FILTER_MAX_STACK values and ends with one.
 * The limits are conditions: a filter beyond one of them has no program (the host evaluates it). */
#define ANNLITE_FILTER_MAX_LEAVES 32
#define ANNLITE_FILTER_MAX_LITERALS 64
#define ANNLITE_FILTER_MAX_CODE 128
#define ANNLITE_FILTER_MAX_STACK 32
#define ANNLITE_FILTER_MAX_BLOCKS 2048 /* the default cap of the grid (256 rows per workgroup and pass) */
#define ANNLITE_COL_I64 0
#define ANNLITE_COL_F64 1
#define ANNLITE_COL_CODE 2
#define ANNLITE_FOP_LT 0
#define ANNLITE_FOP_GT 1
#define ANNLITE_FOP_LE 2
#define ANNLITE_FOP_GE 3
#define ANNLITE_FOP_EQ 4
#define ANNLITE_FOP_NE 5
#define ANNLITE_FOP_IN 6
#define ANNLITE_FOP_NIN 7
#define ANNLITE_FOP_IN_SET 8
#define ANNLITE_FCODE_AND 0x80
#define ANNLITE_FCODE_OR 0x81
#define ANNLITE_FCODE_NOT 0x82
#define ANNLITE_FCODE_TRUE 0x83

typedef struct annlite_filter_leaf {
    const void *values_dev;
    const uint32_t *present_dev;
    const uint32_t *set_bits_dev; /* IN_SET only, else NULL */
    uint8_t kind;                 /* ANNLITE_COL_* */
    uint8_t op;                   /* ANNLITE_FOP_* */
    uint8_t lit_begin;
    uint8_t lit_count;
    uint32_t set_words;           /* IN_SET only, else 0 */
} annlite_filter_leaf;

typedef struct annlite_filter_program {
    int32_t n_leaves;
    int32_t n_literals;
    int32_t n_code;
    int32_t reserved; /* 0 */
    annlite_filter_leaf leaves[ANNLITE_FILTER_MAX_LEAVES];
    uint64_t literals[ANNLITE_FILTER_MAX_LITERALS];
    uint8_t code[ANNLITE_FILTER_MAX_CODE];
} annlite_filter_program;

/* out_bits_dev u32 [n_words] <- bit r = (row r < N satisfies the program) & bit r of and_bits_dev (u32 [n_words], may be NULL: the
 * caller's validity or row-present words).  EVERY word is written: the words of rows >= N are 0, so with n_words = (capacity + 31) /
 * 32 + 2 the result is a valid_bits array of every search here.  n_words * 32 >= N.  count_dev (may be NULL) u64 [1] += the number
 * of bits set (one atomic per workgroup; the caller zeroes it).  One row per lane, 256 lanes per workgroup, the verdicts of a wave
 * packed by ballot; the grid is capped at max_blocks workgroups (0: ANNLITE_FILTER_MAX_BLOCKS) that stride over the rows.
 * `program` is a HOST pointer (copied into the launch); it is checked against the limits and the stack discipline above.
 * replaces: the query path of the reference's cell table (annlite/storage/table.py: CellTable.query -- the SQL WHERE clause over the
 * declared columns that yields the offsets a filtered search is given). */
ANNLITE_API int annlite_filter_eval(const annlite_filter_program *program, int64_t N, const uint32_t *and_bits_dev, uint32_t *out_bits_dev,
                        int64_t n_words, uint64_t *count_dev, int max_blocks, void *stream);

/* Pages of the document listing (page.hip): the rows of a bitmap whose rank in the listing's order lies in
 * [first, first + count).  The order is the host's (AnnLite.filter): the rows WITH a value of the column sorted by it -- ties in
 * ascending row, in both directions (Python's stable sort) --, the rows without one (present bit 0) in ascending row before them
 * (ascending) or behind them (descending).  Per row the composite (class, key, row) is distinct; the page is selected by MSB radix
 * select over its 8-bit digits and sorted by one workgroup, so the answer does not depend on the order of any atomic.
 *   key: I64 (ints, bools)  x ^ 2^63;   F64  the monotone bit flip of the double, -0.0 first made +0.0 (never NaN);
 *        CODE  rank_dev[code] (u32 [rank_len], 1 <= rank_len <= 65536: the position of the word in the sorted dictionary);
 *        descending: ~key.
 * mask_dev u32 [n_words] (may be NULL: every row of rows_dev) is ANDed with rows_dev u32 [n_words], the row-present words; rows >= N
 * are never read or returned (n_words * 32 >= N, N < 2^31).  first >= 0, 1 <= count <= ANNLITE_PAGE_MAX, first + count < 2^31.
 * out_rows_dev i32 [count] <- the page, in order; out_n_dev i32 [1] <- its rows: min(first + count, selected) - first, 0 where first
 * is at or beyond the selection (the rest of out_rows_dev is left as it was).  workspace: annlite_page_workspace_bytes, 16-byte
 * aligned.  One launch per digit that can differ (13 at most), each over the mask words and the 8-byte (CODE: 4-byte) values, then a
 * collect and a sort; the grids are capped at max_blocks workgroups (0: ANNLITE_PAGE_MAX_BLOCKS) of ANNLITE_PAGE_BLOCK_ROWS rows per
 * stride.  A bad kind, a negative first, a count out of range, n_words * 32 < N or a NULL pointer is an error; nothing is launched.
 * replaces: the reference's document listing (annlite/storage/table.py: the SQL ORDER BY ... LIMIT ... OFFSET behind
 * AnnLite.filter / get_docs). */
#define ANNLITE_PAGE_MAX 4096
#define ANNLITE_PAGE_BLOCK_ROWS 1024
#define ANNLITE_PAGE_MAX_BLOCKS 2048
ANNLITE_API int annlite_page_workspace_bytes(int64_t *bytes);
ANNLITE_API int annlite_order_page(const uint32_t *mask_dev, const uint32_t *rows_dev, const void *values_dev, int kind,
                        const uint32_t *present_dev, const uint32_t *rank_dev, int64_t rank_len, int64_t N, int64_t n_words,
                        int descending, int64_t first, int64_t count, int32_t *out_rows_dev, int32_t *out_n_dev, void *workspace,
                        size_t workspace_bytes, int max_blocks, void *stream);
/* ... without an order: the set bits of bits_dev & and_bits_dev (u32 [n_words] each; and_bits_dev may be NULL) of rank
 * [first, first + count), ascending -- the same select over the row digits alone.  Same outputs, limits and errors. */
ANNLITE_API int annlite_bitmap_page(const uint32_t *bits_dev, const uint32_t *and_bits_dev, int64_t N, int64_t n_words, int64_t first,
                        int64_t count, int32_t *out_rows_dev, int32_t *out_n_dev, void *workspace, size_t workspace_bytes,
                        int max_blocks, void *stream);

/* A bitmap as a list (bitmap_rows.hip; DESIGN.md section 3.6, "selected rows"): out_rows_dev i32 [0 .. min(n, out_capacity)) <- the
 * offsets r < N whose bit is set in bits_dev (and in and_bits_dev, may be NULL; u32 [n_words] each, n_words * 32 >= N, N < 2^31),
 * ASCENDING; out_n_dev i64 [1] <- n, the number of such rows, also where n > out_capacity (nothing is written at or behind
 * out_capacity).  Bits at positions >= N are ignored.  Three stream-ordered launches -- set bits per workgroup of 1024 words, their
 * prefix sum by one workgroup, the scatter --, no workgroup waits for another and no position depends on an atomic: the same input
 * gives the same array.  workspace: annlite_bitmap_rows_workspace_bytes(N).
 * replaces: CellTable.query's list of offsets (annlite/storage/table.py), as annlite_filter_eval replaces its WHERE clause. */
ANNLITE_API int annlite_bitmap_rows_workspace_bytes(int64_t N, int64_t *bytes);
ANNLITE_API int annlite_bitmap_rows(const uint32_t *bits_dev, const uint32_t *and_bits_dev, int64_t N, int64_t n_words, int32_t *out_rows_dev,
                        int64_t out_capacity, int64_t *out_n_dev, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ANNLITE_HIP_H_ */
