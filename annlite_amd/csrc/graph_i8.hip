// graph_i8.hip -- the level-0 graph over int8 rows (FlatGpuIndex's int8 row store): annlite_graph_i8_search / _search_admit /
// _build_select / _build_reverse are graph_rows.h's four kernels with a row distance of their own, which carries the rows' scale.
//
// The contract is graph_rows.h's: every distance carries the bits of annlite_exact_gather_dist_i8 (exact_gather_kernel<int8_t>) -- a
// code c widened as scale * (float)c (exact: the scale is a power of two), 64 chains c = j mod 64 accumulated by fmaf in ascending
// j, the xor butterfly over the chain index 32, 16, 8, 4, 2, 1.  Which lane holds a chain is free, the order of the additions is not.
// Nothing is computed in code units and rescaled: that would differ next to subnormals and overflow.
//
// rows_dist_group: PART OF A WAVE per row.  A row of D = 128 codes is 128 B, one cache line: a whole wave on it would be 128
// one-byte loads and a six-step cross-lane butterfly per row.  Two splits are compiled ("int8 rows", has both
// walk times):
//   * the EIGHTH wave (the default): a group of 8 lanes takes one row, a wave 8 rows per pass, and 1, 2 or 4 passes (8, 16, 32 rows:
//     a whole link list of the largest max_connection) are in flight.  Lane g of a group owns the chains 8g .. 8g + 7: per block t
//     of 64 elements ONE 8-byte load of eight codes at x[row * D + 64 t + 8 g] -- a group reads 64 contiguous bytes -- and eight
//     values of the query (two 16-byte LDS reads in the walk, the eight groups reading the same addresses, or 8 bytes of another
//     int8 row in the build).  Steps 32, 16, 8 are lane xor 4, 2, 1 inside the group on eight registers (one ds_swizzle, two DPP
//     quad_perm), steps 4, 2, 1 are in registers: a_k = s_k + s_{k+4}, b_0 = a_0 + a_2, b_1 = a_1 + a_3, r = b_0 + b_1.  D % 8 == 0;
//   * the QUARTER wave (-DANNLITE_I8_QUARTER): 16 lanes per row, chains 4g .. 4g + 3, one 4-byte load per block, 4 rows per pass, up
//     to 16 rows in flight; steps 32 .. 4 are lane xor 8, 4, 2, 1 on four registers, steps 2 and 1 in registers.  D % 4 == 0.
// Either way a lane's elements of a tail block lie wholly inside or wholly beyond D: elements j >= D are never loaded and never
// accumulated (no padded zero meets a query's inf).
//
// Widening without sign extraction: the 32-bit word of four codes xor 0x80808080 holds c + 128 in [1, 255] per byte; byte k converts
// by the unsigned byte-to-float instruction (v_cvt_f32_ubyteK), and fmaf(u, scale, -128 scale) is scale * c bit for bit -- product
// and sum are exact, and c = 0 gives +0.0 as scale * 0.f does.  2 1/4 VALU per element where sign extraction takes three.
// Every other D takes RowsStrided<int8_t>: rows_dist with one-byte loads, same bits.
#include "graph_rows.h"

namespace annlite {

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
#ifdef ANNLITE_I8_QUARTER
constexpr int kChains = 4;
#else
constexpr int kChains = 8;
#endif
constexpr int kGroup = 64 / kChains;  // lanes per row; a pass holds 64 / kGroup = kChains rows

// the C codes at p (C-byte aligned) as scale * c; m128 = -128 scale
template <int C>
__device__ __forceinline__ void widen_codes(const int8_t *p, float scale, float m128, float (&o)[C]) {
    uint32_t w[C / 4];
    if constexpr (C == 8) {
        const u32x2_t v = *(const u32x2_t *)p;
        w[0] = v[0], w[1] = v[1];
    } else {
        w[0] = *(const uint32_t *)p;
    }
#pragma unroll
    for (int h = 0; h < C / 4; ++h) {
        const uint32_t b = w[h] ^ 0x80808080u;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[4 * h + k] = __builtin_fmaf((float)(uint8_t)(b >> (8 * k)), scale, m128);
    }
}

// C elements of the query at j (j % C == 0, j + C <= D): the walk's f32 image in LDS (16-byte aligned), or an int8 row
template <int C>
__device__ __forceinline__ void query_group(const float *qv, int j, float, float, float (&o)[C]) {
#pragma unroll
    for (int h = 0; h < C / 4; ++h) {
        const f32x4 v = *(const f32x4 *)(qv + j + 4 * h);
        o[4 * h] = v[0], o[4 * h + 1] = v[1], o[4 * h + 2] = v[2], o[4 * h + 3] = v[3];
    }
}
template <int C>
__device__ __forceinline__ void query_group(const int8_t *qv, int j, float scale, float m128, float (&o)[C]) {
    widen_codes<C>(qv + j, scale, m128, o);
}

// The next kChains * P rows of `pm` (lowest lanes first; `pm` loses them), kChains per pass: the rows' distances delivered into
// `mine` of the lanes that hold them.  D % kChains == 0, x 8-byte aligned.
template <bool L2, int P, class Q>
__device__ __forceinline__ void group_passes(unsigned long long &pm, uint32_t node, const int8_t *__restrict__ x, int D, const Q *qv,
                                             int lane, float scale, float &mine) {
    constexpr int C = kChains, R = kChains;      // chains per lane, rows per pass
    const int grp = lane / kGroup, g0 = (lane % kGroup) * C;  // (the lane's first element of a block)
    const unsigned long long taken = pm;         // (row r = R u + group is its r-th lowest lane)
    bool on[P];
    const int8_t *xr[P];
#pragma unroll
    for (int u = 0; u < P; ++u) {
        uint32_t nd = 0;
        on[u] = false;
#pragma unroll
        for (int G = 0; G < R; ++G) {
            const bool has = pm != 0ull;
            const int sl = has ? __builtin_ctzll(pm) : 0;
            pm &= pm - 1;  // (0 stays 0)
            const uint32_t n = __builtin_amdgcn_readlane(node, sl);
            if (grp == G) nd = n, on[u] = has;
        }
        xr[u] = x + (int64_t)nd * D + g0;  // (read only where on[u])
    }
    const float m128 = -128.f * scale;
    float s[P][C];
#pragma unroll
    for (int u = 0; u < P; ++u)
#pragma unroll
        for (int k = 0; k < C; ++k) s[u][k] = 0.f;
    // block t: elements 64 t + C g .. + C - 1 of every row; `in`: they exist (D % C == 0: all of them or none)
    auto block = [&](int off, bool full) __attribute__((always_inline)) {
        const bool in = full || off + g0 < D;
        float qf[C];
#pragma unroll
        for (int k = 0; k < C; ++k) qf[k] = 0.f;
        if (in) query_group<C>(qv, off + g0, scale, m128, qf);
        float xf[P][C];
#pragma unroll
        for (int u = 0; u < P; ++u) {
#pragma unroll
            for (int k = 0; k < C; ++k) xf[u][k] = 0.f;
            if (in && on[u]) widen_codes<C>(xr[u] + off, scale, m128, xf[u]);
        }
#pragma unroll
        for (int u = 0; u < P; ++u) {
#pragma unroll
            for (int k = 0; k < C; ++k) {
                float acc;
                if constexpr (L2) {
                    const float d = xf[u][k] - qf[k];
                    acc = __builtin_fmaf(d, d, s[u][k]);
                } else {
                    acc = __builtin_fmaf(xf[u][k], qf[k], s[u][k]);
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
        // the butterfly's steps across the group's lanes: 32, 16, 8 (eighth wave) or 32, 16, 8, 4 (quarter wave) ...
        if constexpr (kGroup == 16) {
#pragma unroll
            for (int k = 0; k < C; ++k) s[u][k] += group_xor<8>(s[u][k]);
        }
#pragma unroll
        for (int k = 0; k < C; ++k) s[u][k] += group_xor<4>(s[u][k]);
#pragma unroll
        for (int k = 0; k < C; ++k) s[u][k] += group_xor<2>(s[u][k]);
#pragma unroll
        for (int k = 0; k < C; ++k) s[u][k] += group_xor<1>(s[u][k]);
        // ... and the rest in registers: step h pairs chain k with chain k + h
#pragma unroll
        for (int h = C / 2; h >= 1; h >>= 1)
#pragma unroll
            for (int k = 0; k < h; ++k) s[u][k] = s[u][k] + s[u][k + h];
        r[u] = L2 ? s[u][0] : 1.f - s[u][0];
    }
    unsigned long long left = taken;
#pragma unroll
    for (int u = 0; u < P; ++u) {
#pragma unroll
        for (int G = 0; G < R; ++G) {
            const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r[u]), kGroup * G));
            const bool has = left != 0ull;
            const int sl = has ? __builtin_ctzll(left) : 0;
            left &= left - 1;
            if (has && lane == sl) mine = d;
        }
    }
}

// rows_dist's contract (graph_rows.h) over int8 rows with D % kChains == 0 and an 8-byte aligned table: 8, 16 or 32 rows in flight
// (the quarter wave: 8 or 16), by how many are asked for
template <bool L2, class Q>
__device__ __forceinline__ float rows_dist_group(unsigned long long pm, uint32_t node, const int8_t *__restrict__ x, int D, const Q *qv,
                                                 int lane, float scale) {
    float mine = 0.f;
    while (pm) {
        const int n = __popcll(pm);
        if (n <= 8) group_passes<L2, 8 / kChains>(pm, node, x, D, qv, lane, scale, mine);
        else if (n <= 16) group_passes<L2, 16 / kChains>(pm, node, x, D, qv, lane, scale, mine);
        else group_passes<L2, 4>(pm, node, x, D, qv, lane, scale, mine);
    }
    return mine;
}

struct RowsI8Group : RowScale<int8_t> {
    typedef int8_t row_t;
    template <bool L2, class Q>
    __device__ __forceinline__ float dist(unsigned long long pm, uint32_t node, const int8_t *__restrict__ x, int D, const Q *qv,
                                          int lane) const {
        return rows_dist_group<L2>(pm, node, x, D, qv, lane, this->scale);
    }
};
typedef RowsStrided<int8_t> RowsI8Strided;

template <class RD>
static RD with_scale(float scale) {
    RD rd;
    rd.scale = scale;
    return rd;
}

}  // namespace annlite

using namespace annlite;

// the group distance where the rows allow its loads, the lane-strided one everywhere else
#define ANNLITE_I8_ROWS(fn, ...)                                                                                      \
    ((D % kChains == 0 && (uintptr_t)vectors_i8_dev % 8 == 0) ? fn<RowsI8Group>(__VA_ARGS__, with_scale<RowsI8Group>(scale)) \
                                                              : fn<RowsI8Strided>(__VA_ARGS__, with_scale<RowsI8Strided>(scale)))

extern "C" int annlite_graph_i8_search(int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_i8_dev, float scale,
                                       int64_t N, const uint32_t *links_dev, int links_per_node, const uint32_t *seeds_dev, int64_t n_seeds,
                                       const uint32_t *valid_bits_dev, int ef, int64_t *out_ids_dev, float *out_dist_dev, void *stream) {
    ANNLITE_REQUIRE_I8_SCALE(scale);
    return ANNLITE_I8_ROWS(graph_rows_search, metric, queries_dev, B, D, (const int8_t *)vectors_i8_dev, N, links_dev, links_per_node,
                           seeds_dev, n_seeds, valid_bits_dev, ef, out_ids_dev, out_dist_dev, stream);
}

extern "C" int annlite_graph_i8_search_admit(int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_i8_dev,
                                             float scale, int64_t N, const uint32_t *links_dev, int links_per_node,
                                             const uint32_t *seeds_dev, int64_t n_seeds, const uint32_t *admit_bits_dev, int ef_route, int ef,
                                             int64_t *out_ids_dev, float *out_dist_dev, float *out_route_worst_dev, void *stream) {
    ANNLITE_REQUIRE_I8_SCALE(scale);
    return ANNLITE_I8_ROWS(graph_rows_search_admit, metric, queries_dev, B, D, (const int8_t *)vectors_i8_dev, N, links_dev,
                           links_per_node, seeds_dev, n_seeds, admit_bits_dev, ef_route, ef, out_ids_dev, out_dist_dev, out_route_worst_dev,
                           stream);
}

extern "C" int annlite_graph_i8_build_select(int metric, const int64_t *cand_dev, int ef, int64_t b, int64_t base0,
                                             const void *vectors_i8_dev, float scale, int64_t N, int64_t D, int max_keep,
                                             uint32_t *links_dev, int links_per_node, int64_t *pairs_dev, void *stream) {
    ANNLITE_REQUIRE_I8_SCALE(scale);
    return ANNLITE_I8_ROWS(graph_rows_build_select, metric, cand_dev, ef, b, base0, (const int8_t *)vectors_i8_dev, N, D, max_keep,
                           links_dev, links_per_node, pairs_dev, stream);
}

extern "C" int annlite_graph_i8_build_reverse(int metric, const int64_t *keys_dev, const int64_t *seg_dev, int64_t n_segments,
                                              const void *vectors_i8_dev, float scale, int64_t N, int64_t D, uint32_t *links_dev,
                                              int links_per_node, void *stream) {
    ANNLITE_REQUIRE_I8_SCALE(scale);
    return ANNLITE_I8_ROWS(graph_rows_build_reverse, metric, keys_dev, seg_dev, n_segments, (const int8_t *)vectors_i8_dev, N, D,
                           links_dev, links_per_node, stream);
}
