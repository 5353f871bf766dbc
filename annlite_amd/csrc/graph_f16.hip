// graph_f16.hip -- the level-0 graph over f16 rows (FlatGpuIndex's half-precision row store): annlite_graph_f16_search /
// _search_admit / _build_select / _build_reverse are graph_rows.h's four kernels with a row distance of their own.
//
// The contract is graph_rows.h's: every distance carries the bits of annlite_exact_gather_dist_f16 (exact_gather_kernel<_Float16>) --
// the element widened exactly, 64 chains c = j mod 64 accumulated by fmaf in ascending j, the xor butterfly over the chain index
// 32, 16, 8, 4, 2, 1.  Which lane holds a chain is free, the order of the additions is not.
//
// rows_dist_quarter: a QUARTER WAVE per row.  A row of D = 128 halves is 256 B: a whole wave on it with 2-byte loads would be 128
// narrow loads and a six-step cross-lane butterfly per row.  Here a group of 16 lanes takes one row, a wave four rows per pass,
// and up to four passes (16 rows) are in flight.  Lane g of a group owns four chains; two layouts are compiled (DESIGN.md section
// 3.8, "f16 rows", has both walk times):
//   * layout B (the default: 2.5 % faster than A at 1M x 128, 1.8 % slower to level at 1M x 768): chains 2g, 2g + 1, 2g + 32,
//     2g + 33.  Per block t of 64 elements two 4-byte loads of two halves at x[row * D + 64 t + 2 g] and + 32, two 8-byte reads of
//     the query (LDS in the walk -- the four groups read the same addresses --, or 4 bytes of another f16 row in the build).  Step 32
//     is in registers, steps 16, 8, 4, 2 are lane xor 8, 4, 2, 1 inside the group on TWO registers, step 1 is in registers;
//   * layout A (-DANNLITE_F16_LAYOUT_A): chains 4g .. 4g + 3.  One 8-byte load of four halves at 64 t + 4 g, one 16-byte read of the
//     query; steps 32, 16, 8, 4 are lane xor 8, 4, 2, 1 on FOUR registers, steps 2 and 1 in registers: (s0 + s2) + (s1 + s3).
// The lane xor is DPP row_ror:8, one ds_swizzle, two DPP quad_perm -- no LDS address, no trip through ds_bpermute.
// The quarter wave takes D % 4 == 0 and an 8-byte aligned table (what A's loads need; a lane's elements of a half block then lie
// wholly inside or wholly beyond D: elements j >= D are never loaded and never accumulated -- no padded zero meets a query's inf).
// Every other D takes RowsStrided<_Float16>: rows_dist with 2-byte loads, same bits.
#include "graph_rows.h"

namespace annlite {

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
#ifdef ANNLITE_F16_LAYOUT_A
constexpr bool kLayoutB = false;
#else
constexpr bool kLayoutB = true;
#endif

// four elements of the query at j (j % 4 == 0, j + 3 < D): the walk's f32 image in LDS (16-byte aligned), or an f16 row
__device__ __forceinline__ void query4(const float *qv, int j, float (&o)[4]) {
    const f32x4 v = *(const f32x4 *)(qv + j);
    o[0] = v[0], o[1] = v[1], o[2] = v[2], o[3] = v[3];
}
__device__ __forceinline__ void query4(const _Float16 *qv, int j, float (&o)[4]) {
    const half4_t v = *(const half4_t *)(qv + j);
    o[0] = (float)v[0], o[1] = (float)v[1], o[2] = (float)v[2], o[3] = (float)v[3];
}

// two elements at j (j % 2 == 0, j + 1 < D): layout B's half block
__device__ __forceinline__ void query2(const float *qv, int j, float *o) {
    const f32x2_t v = *(const f32x2_t *)(qv + j);
    o[0] = v[0], o[1] = v[1];
}
__device__ __forceinline__ void query2(const _Float16 *qv, int j, float *o) {
    const half2_t v = *(const half2_t *)(qv + j);
    o[0] = (float)v[0], o[1] = (float)v[1];
}

// The next 4 P rows of `pm` (lowest lanes first; `pm` loses them), four per pass: the rows' distances delivered into `mine` of the
// lanes that hold them.  D % 4 == 0, x 8-byte aligned.
template <bool L2, int P, class Q>
__device__ __forceinline__ void quarter_passes(unsigned long long &pm, uint32_t node, const _Float16 *__restrict__ x, int D, const Q *qv,
                                               int lane, float &mine) {
    const int grp = lane >> 4, g4 = (lane & 15) * (kLayoutB ? 2 : 4);  // (the lane's first element of a block)
    int src[4 * P];  // (wave-uniform) the lane that holds row r = 4 u + group; -1: none
    bool on[P];
    const _Float16 *xr[P];
#pragma unroll
    for (int u = 0; u < P; ++u) {
        uint32_t nd = 0;
        on[u] = false;
#pragma unroll
        for (int G = 0; G < 4; ++G) {
            const bool has = pm != 0ull;
            const int sl = has ? __builtin_ctzll(pm) : 0;
            src[4 * u + G] = has ? sl : -1;
            pm &= pm - 1;  // (0 stays 0)
            const uint32_t n = __builtin_amdgcn_readlane(node, sl);
            if (grp == G) nd = n, on[u] = has;
        }
        xr[u] = x + (int64_t)nd * D + g4;  // (read only where on[u])
    }
    float s[P][4];
#pragma unroll
    for (int u = 0; u < P; ++u) s[u][0] = s[u][1] = s[u][2] = s[u][3] = 0.f;
    // block t: elements 64 t + 4 g .. + 3 of every row (B: 64 t + 2 g, + 1 and the same + 32); `in0` / `in1`: elements 0, 1 / 2, 3
    // exist (D % 4 == 0: A's four are all there or none)
    auto block = [&](int off, bool full) __attribute__((always_inline)) {
        const bool in0 = full || off + g4 < D, in1 = kLayoutB ? (full || off + 32 + g4 < D) : in0;
        float qf[4] = {0.f, 0.f, 0.f, 0.f};
        half4_t xv[P];
        if constexpr (kLayoutB) {
            if (in0) query2(qv, off + g4, qf);
            if (in1) query2(qv, off + 32 + g4, qf + 2);
#pragma unroll
            for (int u = 0; u < P; ++u) {
                const half2_t lo = in0 && on[u] ? *(const half2_t *)(xr[u] + off) : (half2_t){0, 0};
                const half2_t hi = in1 && on[u] ? *(const half2_t *)(xr[u] + off + 32) : (half2_t){0, 0};
                xv[u] = (half4_t){lo[0], lo[1], hi[0], hi[1]};
            }
        } else {
            if (in0) query4(qv, off + g4, qf);
#pragma unroll
            for (int u = 0; u < P; ++u) xv[u] = in0 && on[u] ? *(const half4_t *)(xr[u] + off) : (half4_t){0, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < P; ++u) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = k < 2 ? in0 : in1;
                const float xf = (float)xv[u][k];
                float acc;
                if constexpr (L2) {
                    const float d = xf - qf[k];
                    acc = __builtin_fmaf(d, d, s[u][k]);
                } else {
                    acc = __builtin_fmaf(xf, qf[k], s[u][k]);
                }
                s[u][k] = in ? acc : s[u][k];  // (an element beyond D is not accumulated: no 0 * inf)
            }
        }
    };
    const int full = D & ~63;
    for (int off = 0; off < full; off += 64) block(off, true);
    if (full < D) block(full, false);
    float r[P];
#pragma unroll
    for (int u = 0; u < P; ++u) {
        if constexpr (kLayoutB) {
            float a = s[u][0] + s[u][2], b = s[u][1] + s[u][3];  // step 32
            a += group_xor<8>(a), b += group_xor<8>(b);          // 16
            a += group_xor<4>(a), b += group_xor<4>(b);          // 8
            a += group_xor<2>(a), b += group_xor<2>(b);          // 4
            a += group_xor<1>(a), b += group_xor<1>(b);          // 2
            r[u] = a + b;                                        // 1
            if constexpr (!L2) r[u] = 1.f - r[u];
            continue;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s[u][k] += group_xor<8>(s[u][k]);  // step 32
#pragma unroll
        for (int k = 0; k < 4; ++k) s[u][k] += group_xor<4>(s[u][k]);  // 16
#pragma unroll
        for (int k = 0; k < 4; ++k) s[u][k] += group_xor<2>(s[u][k]);  // 8
#pragma unroll
        for (int k = 0; k < 4; ++k) s[u][k] += group_xor<1>(s[u][k]);  // 4
        const float a = s[u][0] + s[u][2], b = s[u][1] + s[u][3];      // 2
        r[u] = a + b;                                                  // 1
        if constexpr (!L2) r[u] = 1.f - r[u];
    }
#pragma unroll
    for (int u = 0; u < P; ++u) {
#pragma unroll
        for (int G = 0; G < 4; ++G) {
            const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r[u]), 16 * G));
            if (lane == src[4 * u + G]) mine = d;
        }
    }
}

// rows_dist's contract (graph_rows.h) over f16 rows with D % 4 == 0 and an 8-byte aligned table
template <bool L2, class Q>
__device__ __forceinline__ float rows_dist_quarter(unsigned long long pm, uint32_t node, const _Float16 *__restrict__ x, int D, const Q *qv,
                                                   int lane) {
    float mine = 0.f;
    while (pm) {
        if (__popcll(pm) <= 8) quarter_passes<L2, 2>(pm, node, x, D, qv, lane, mine);
        else quarter_passes<L2, 4>(pm, node, x, D, qv, lane, mine);
    }
    return mine;
}

struct RowsF16Quarter {
    typedef _Float16 row_t;
    template <bool L2, class Q>
    __device__ __forceinline__ float dist(unsigned long long pm, uint32_t node, const _Float16 *__restrict__ x, int D, const Q *qv,
                                          int lane) const {
        return rows_dist_quarter<L2>(pm, node, x, D, qv, lane);
    }
};
typedef RowsStrided<_Float16> RowsF16Strided;

}  // namespace annlite

using namespace annlite;

// the quarter-wave distance where the rows allow 8-byte loads, the lane-strided one everywhere else
#define ANNLITE_F16_ROWS(fn, ...)                                                                  \
    ((D % 4 == 0 && (uintptr_t)vectors_f16_dev % 8 == 0) ? fn<RowsF16Quarter>(__VA_ARGS__) : fn<RowsF16Strided>(__VA_ARGS__))

extern "C" int annlite_graph_f16_search(int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_f16_dev, int64_t N,
                                        const uint32_t *links_dev, int links_per_node, const uint32_t *seeds_dev, int64_t n_seeds,
                                        const uint32_t *valid_bits_dev, int ef, int64_t *out_ids_dev, float *out_dist_dev, void *stream) {
    return ANNLITE_F16_ROWS(graph_rows_search, metric, queries_dev, B, D, (const _Float16 *)vectors_f16_dev, N, links_dev, links_per_node,
                            seeds_dev, n_seeds, valid_bits_dev, ef, out_ids_dev, out_dist_dev, stream);
}

extern "C" int annlite_graph_f16_search_admit(int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_f16_dev,
                                              int64_t N, const uint32_t *links_dev, int links_per_node, const uint32_t *seeds_dev,
                                              int64_t n_seeds, const uint32_t *admit_bits_dev, int ef_route, int ef, int64_t *out_ids_dev,
                                              float *out_dist_dev, float *out_route_worst_dev, void *stream) {
    return ANNLITE_F16_ROWS(graph_rows_search_admit, metric, queries_dev, B, D, (const _Float16 *)vectors_f16_dev, N, links_dev,
                            links_per_node, seeds_dev, n_seeds, admit_bits_dev, ef_route, ef, out_ids_dev, out_dist_dev, out_route_worst_dev,
                            stream);
}

extern "C" int annlite_graph_f16_build_select(int metric, const int64_t *cand_dev, int ef, int64_t b, int64_t base0,
                                              const void *vectors_f16_dev, int64_t N, int64_t D, int max_keep, uint32_t *links_dev,
                                              int links_per_node, int64_t *pairs_dev, void *stream) {
    return ANNLITE_F16_ROWS(graph_rows_build_select, metric, cand_dev, ef, b, base0, (const _Float16 *)vectors_f16_dev, N, D, max_keep,
                            links_dev, links_per_node, pairs_dev, stream);
}

extern "C" int annlite_graph_f16_build_reverse(int metric, const int64_t *keys_dev, const int64_t *seg_dev, int64_t n_segments,
                                               const void *vectors_f16_dev, int64_t N, int64_t D, uint32_t *links_dev, int links_per_node,
                                               void *stream) {
    return ANNLITE_F16_ROWS(graph_rows_build_reverse, metric, keys_dev, seg_dev, n_segments, (const _Float16 *)vectors_f16_dev, N, D,
                            links_dev, links_per_node, stream);
}
