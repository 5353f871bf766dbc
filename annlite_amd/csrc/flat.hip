// flat.hip -- exact float32 search over un-quantised vectors.
//
// The reference's default index (AnnLite without n_subvectors) holds float vectors: HnswIndex.search
// (annlite/core/index/hnsw/index.py:139-167) or, as brute force, FlatIndex.search (annlite/core/index/flat_index.py:15-39:
// cdist + top_k).  Here: a dense f32 MFMA contraction FILTERS the table against a per-query bound with a proven slack, the
// rows that pass are appended to per-query candidate lists, and a wave per query re-scores its list in the arithmetic of
// rerank_topk_kernel (codec.hip) -- so the answer is exact in that arithmetic whatever the filter's rounding was.
//
// Second half of the file: the same search over the rows of each query's probed CELLS (the reference's n_cells > 1 structure over that
// index, container.py:88-144) -- the filter over (cell, queries that probe it) tiles, the cells a permutation
// of the row offsets.
//
// Six MFMA filter kernels (f32, split-bf16, f16 and int8 rows over the table; f32 and split-bf16 over cell tiles) differ in their
// contraction and share the rest, each piece written once:
//   flat_tile_rows / ivf_flat_tile_range + ivf_flat_tile_rows   the row tile's prologue: bounds, bitmap, norms
//   flat_stage_planes                                            16-byte slots of 2-byte planes from HBM into an LDS stage
//   flat_f32_stage + flat_f32_contract                           the f32 stage and its 4-MFMA K loop
//   FLAT_BF16X3_CONTRACT                                         the split filter's 12-MFMA K loop (a macro: see there)
//   flat_tile_epilogue -> flat_admit                             C-tile row map, score, `scores`, the negated comparison, the append
// The four table filters also run over a LIST of selected rows (flat_tile_rows_mapped, flat_row_slot: each body is a function of
// <VEC, MAPPED> behind the table kernel and a flat_rows_* twin; DESIGN.md section 3.6, "selected rows"), and over the table with a
// BITMAP PER QUERY (FlatGroups, the GROUPED mode of the same bodies and of flat_exact_kernel behind flat_grouped_* kernels; DESIGN.md
// section 3.6, "a filter per query").
// and on the host: WsBump (workspace carving), flat_filter_grid, FLAT_LAUNCH_VEC, flat_check_workspace, flat_check_shape; for the table
// filters one description per filter (FlatF32 ...), one struct of operands (FlatCall) and one body per job (flat_search, flat_stage).
#include <math.h>

#include <type_traits>

#include "common.h"

namespace annlite {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kFlatTile = 128;            // rows x queries of a workgroup tile (4 waves, 64 x 64 each: 2 x 2 MFMA tiles of 32 x 32)
constexpr int kFlatDepth = 32;            // coordinates per LDS stage
constexpr int kFlatLd = kFlatDepth + 1;   // LDS row pitch in floats: 33 keeps the 32 rows of one MFMA operand on 32 banks
constexpr int kFlatCap = 4096;            // candidates per query list (32 k + 8 sigma at k = 64 is 4096)
constexpr int64_t kFlatSample = 4096;     // rows of the first (exact) sample; tables up to this size skip the filter
constexpr double kFlatGrowth = 32.0;      // a stage's row set is at most this many times the previous one

// ---- |x|^2 per row: the lane-strided fmaf chain + butterfly of the exact kernels (relative error <= gamma(ceil(D/64) + 6)) ----
// CENTRED: the same chain over c_j = fl(x_j - mu_j), the values the split filter contracts (second half of the filter section).
// T: the row type, float or _Float16 (a half-precision row store, "f16 rows" below): an f16 value widens exactly, and everything after
// the load is the f32 form's, operation for operation.  int8_t ("int8 rows" below): a code c stands for scale * c, scale a power of
// two, so the widened value is exact as well; `scale` is read by that instantiation only.
// cell_of != NULL (CENTRED; the split filter over cell tiles, second half of the file): mu is f32 [C][D] and the row's centre is the
// one of its cell, mu[cell_of[row]] (an id outside [0, C): cell 0, as ivf_flat_cell_range reads it).
template <bool CENTRED, class T = float>
__global__ __launch_bounds__(256) void flat_norms_kernel(const T *__restrict__ x, int D, const int64_t *__restrict__ ids, int64_t n,
                                                        int64_t id_base, int64_t capacity, const float *__restrict__ mu,
                                                        const int32_t *__restrict__ cell_of, int C, float *__restrict__ norms,
                                                        float scale = 1.f) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t row = ids ? ids[i] : id_base + i;
    if (row < 0 || row >= capacity) return;
    const T *xr = x + row * D;
    if (CENTRED && cell_of) {
        const int c = cell_of[row];
        mu += (int64_t)((unsigned)c < (unsigned)C ? c : 0) * D;
    }
    float s = 0.f;
    for (int j = lane; j < D; j += 64) {
        const float xv = std::is_same<T, int8_t>::value ? scale * (float)xr[j] : (float)xr[j];
        const float c = CENTRED ? xv - mu[j] : xv;
        s = __builtin_fmaf(c, c, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) norms[row] = s;
}

// ---- the filter: scores of a tile of rows x a tile of queries on v_mfma_f32_32x32x2_f32 ------------------------------------------
// Row r of the stage's row set is table row r * stride (r < S).  A workgroup keeps ONE row tile and walks the query tiles
// blockIdx.y, blockIdx.y + gridDim.y, ...: the table streams from HBM once, the queries (B x D floats) stay in L2.
// Operands: A = rows (lane l: row l & 31, coordinate l >> 5), B = queries (lane l: coordinate l >> 5, query l & 31); C/D: query =
// lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  A lane therefore owns ONE query per tile: bound and |q|^2 sit in registers.
//
// A row passes when   !(v > thr + (c_rel * a + c_abs))   with a = fl(|x|^2 + |q|^2), v = fl(a - 2 dot) (EUCLIDEAN) or fl(1 - dot):
// every exact distance <= thr passes (proof: DESIGN.md section 3.6), and a NaN or infinite thr, a, dot or slack passes EVERYTHING
// (the comparison is written negated for that: section 4's convention).
//
// The pieces below are every filter kernel's; only the contraction between the prologue and the epilogue is a kernel's own.

// Where the row or query of a tile slot lies: `off` elements behind its operand's base pointer; !ok: the slot is staged as zeros.
struct FlatSlot {
    bool ok;
    int64_t off;
};

// A wave's 2 x 2 C tiles of 32 x 32: c<row half><query half>.
struct FlatAcc {
    f32x16 c00, c01, c10, c11;
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int e = 0; e < 16; ++e) c00[e] = c01[e] = c10[e] = c11[e] = 0.f;
    }
    __device__ __forceinline__ const f32x16 &tile(int ri, int qj) const { return ri == 0 ? (qj == 0 ? c00 : c01) : (qj == 0 ? c10 : c11); }
};

// The row tile of a table kernel, by its first kFlatTile threads: oks[i] = stage row r0 + i exists and is valid in the bitmap, nxs[i] =
// its norm (0 without a row).
__device__ __forceinline__ void flat_tile_rows(int tid, int64_t r0, int64_t S, int64_t stride, const uint32_t *__restrict__ valid,
                                               const float *__restrict__ norms, int *oks, float *nxs) {
    if (tid >= kFlatTile) return;
    const int64_t r = r0 + tid;
    bool ok = r < S;
    const int64_t row = ok ? r * stride : 0;
    if (ok && valid) ok = (valid[row >> 5] >> (row & 31)) & 1u;
    oks[tid] = ok ? 1 : 0;
    nxs[tid] = ok ? norms[row] : 0.f;
}

// ... of a MAPPED table kernel ("selected rows"): stage row r is rows[r * stride] of an ascending list of S
// selected offsets, not table row r * stride.  rws[i] = the offset of stage row r0 + i, -1: none (past the list's end, or an entry outside
// [0, N)), as ivf_flat_tile_rows has it; nxs[i] = its norm.  No bitmap: a row in the list is selected.
__device__ __forceinline__ void flat_tile_rows_mapped(int tid, int64_t r0, int64_t S, int64_t stride, const int32_t *__restrict__ rows, int64_t N,
                                                      const float *__restrict__ norms, int *rws, float *nxs) {
    if (tid >= kFlatTile) return;
    const int64_t r = r0 + tid;
    int64_t row = r < S ? (int64_t)rows[r * stride] : -1;
    if (row < 0 || row >= N) row = -1;
    rws[tid] = (int)row;
    nxs[tid] = row >= 0 ? norms[row] : 0.f;
}

// The two forms of "stage row r0 + r of the tile" and of its place in the epilogue, by the kernel's MAPPED flag (oks holds flags
// unmapped, offsets mapped).
template <bool MAPPED>
__device__ __forceinline__ FlatSlot flat_row_slot(const int *oks, int r, int64_t r0, int64_t S, int64_t stride, int D) {
    if constexpr (MAPPED) return FlatSlot{oks[r] >= 0, (int64_t)oks[r] * D};
    else return FlatSlot{r0 + r < S, (r0 + r) * stride * D};
}
template <bool MAPPED>
__device__ __forceinline__ bool flat_row_listed(const int *oks, int rl) {
    return MAPPED ? oks[rl] >= 0 : oks[rl] != 0;
}
template <bool MAPPED>
__device__ __forceinline__ int32_t flat_row_value(const int *oks, int rl, int64_t r0, int64_t stride) {
    return MAPPED ? oks[rl] : (int32_t)((r0 + rl) * stride);
}

// One more entry for a query's list.
__device__ __forceinline__ void flat_admit(int32_t *cnt, int32_t *list, int cap, int32_t value) {
    // (a list that has already overflowed takes the slower route whatever else arrives: stop counting)
    if (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= cap) {
        const int pos = atomicAdd(cnt, 1);
        if (pos < cap) list[pos] = value;
    }
}

// What a lane holds of the ONE query it owns in a C tile: |q|^2, the bound, the per-query term of the slack (read by the kernels that
// have one), the query's counter and list, and its row of the `scores` output (NULL: none).
// mask: the GROUPED kernels' row bitmap of the query (below); the others neither set nor read it.
struct FlatQuery {
    float qn, thr, extra;
    int32_t *cnt, *list;
    float *scores;
    const uint32_t *mask;
};
__device__ __forceinline__ FlatQuery flat_query(int qi, float qn, const float *__restrict__ thr, float extra, int32_t *cand, int32_t *cnt,
                                                int cap, float *scores, int64_t scores_ld, const uint32_t *mask = nullptr) {
    return {qn, thr[qi], extra, cnt + qi, cand + (int64_t)qi * cap, scores ? scores + (int64_t)qi * scores_ld : nullptr, mask};
}

// A filter per query ("a filter per query"): masks u32 [G][ld] are G row bitmaps in `valid`'s word layout (bit r
// of row g: table row r is selected by filter g AND live), group i32 [B] names the bitmap of every query.  The GROUPED kernels prepare
// their row tiles from `valid` -- the union -- as ever, and a (query, row) pair is admitted only if the row's bit is set in the QUERY's
// bitmap.  A group id outside [0, G) selects nothing (no bitmap is read for it).  Over the table only: never with MAPPED.
struct FlatGroups {
    const uint32_t *masks;
    int64_t ld;
    int G;
    const int32_t *group;
};
__device__ __forceinline__ const uint32_t *flat_group_mask(const FlatGroups &g, int qi) {
    const int gi = g.group[qi];
    return (unsigned)gi < (unsigned)g.G ? g.masks + (int64_t)gi * g.ld : nullptr;
}

// A tile row as the epilogue sees it: is it offered to the lists and as which value; does its score go to the `scores` row and to
// which column.
struct FlatRow {
    bool listed;
    int32_t value;
    bool scored;
    int64_t col;
};

// THE epilogue of a 32 x 32 C tile whose first row is tile row rt: score, `scores`, comparison, append.  dot_of(reg): the f32 dot
// product of the lane's accumulator element reg; row_of(rl): the FlatRow of tile row rl.  EXTRA: the slack has the per-query term.
// SCORE_UNLISTED: the kernel's `scores` output also takes rows that are not listed (the table kernels that have one); without it such a
// row is left before any arithmetic.  GROUPED: a pair that passed the bound is admitted only if bit row.value (the table row) is set in
// Q.mask -- tested BEHIND the comparison, so only the few pairs that pass the bound pay the load; a NULL mask admits nothing.
template <bool EXTRA, bool SCORE_UNLISTED, bool GROUPED = false, class Dot, class Row>
__device__ __forceinline__ void flat_tile_epilogue(int metric, float c_rel, float c_abs, int cap, const FlatQuery &Q, const float *nxs, int rt,
                                                   int lh, Dot &&dot_of, Row &&row_of) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int rl = rt + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
        const FlatRow row = row_of(rl);
        if (!SCORE_UNLISTED && !row.listed) continue;
        const float a = nxs[rl] + Q.qn;
        const float dot = dot_of(reg);
        const float v = (metric == ANNLITE_METRIC_EUCLIDEAN) ? a - 2.f * dot : 1.f - dot;
        if (Q.scores && row.scored) Q.scores[row.col] = v;
        if (!row.listed) continue;
        float bound;
        if constexpr (EXTRA) bound = Q.thr + ((c_rel * a + c_abs) + Q.extra);
        else bound = Q.thr + (c_rel * a + c_abs);
        if (!(v > bound)) {
            if constexpr (GROUPED) {
                // (opaque to the optimiser: left visible, the word offsets of a wave's 64 tile rows are computed once ahead of the
                // 2 x 2 C tiles and kept live across them -- about 100 VGPRs, one workgroup per CU where the ungrouped kernel has two)
                int32_t rv = row.value;
                asm volatile("" : "+v"(rv));
                if (!Q.mask || !((Q.mask[rv >> 5] >> (rv & 31)) & 1u)) continue;
            }
            flat_admit(Q.cnt, Q.list, cap, row.value);
        }
    }
}

// One f32 LDS stage: coordinates k0 .. k0 + kFlatDepth of the tile's kFlatTile rows (x + row_at(r).off) into As and of its kFlatTile
// queries (q + query_at(r).off) into Bs, zeros past D and for a slot that is not ok.  256 threads.
template <bool VEC, class RowAt, class QueryAt>
__device__ __forceinline__ void flat_f32_stage(int tid, int k0, int D, const float *__restrict__ x, const float *__restrict__ q, float *As,
                                               float *Bs, RowAt &&row_at, QueryAt &&query_at) {
    if constexpr (VEC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256;  // 1024 slots of 4 floats
            const int r = e >> 3, c = (e & 7) * 4;
            f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
            const FlatSlot sa = row_at(r), sb = query_at(r);
            if (sa.ok && k0 + c < D) va = *(const f32x4 *)(x + sa.off + k0 + c);
            if (sb.ok && k0 + c < D) vb = *(const f32x4 *)(q + sb.off + k0 + c);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                As[r * kFlatLd + c + t] = va[t];
                Bs[r * kFlatLd + c + t] = vb[t];
            }
        }
    } else {
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int e = tid + i * 256;  // 4096 floats
            const int r = e >> 5, c = e & 31;
            const FlatSlot sa = row_at(r), sb = query_at(r);
            As[r * kFlatLd + c] = (sa.ok && k0 + c < D) ? x[sa.off + k0 + c] : 0.f;
            Bs[r * kFlatLd + c] = (sb.ok && k0 + c < D) ? q[sb.off + k0 + c] : 0.f;
        }
    }
}

// ... and its K loop: the wave's 64 rows (from wr) x 64 queries (from wq) of the stage, four v_mfma_f32_32x32x2_f32 per K step of 2.
__device__ __forceinline__ void flat_f32_contract(const float *As, const float *Bs, int wr, int wq, int l31, int lh, FlatAcc &acc) {
#pragma unroll
    for (int kk = 0; kk < kFlatDepth; kk += 2) {
        const int kc = kk + lh;
        const float a0 = As[(wr + l31) * kFlatLd + kc], a1 = As[(wr + 32 + l31) * kFlatLd + kc];
        const float b0 = Bs[(wq + l31) * kFlatLd + kc], b1 = Bs[(wq + 32 + l31) * kFlatLd + kc];
        acc.c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc.c00, 0, 0, 0);
        acc.c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc.c01, 0, 0, 0);
        acc.c10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc.c10, 0, 0, 0);
        acc.c11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc.c11, 0, 0, 0);
    }
}

// MAPPED (every table filter kernel has the flag): the stage rows are the entries of `rows`, offsets < N (flat_tile_rows_mapped); `valid`
// is not read.  Without the flag `rows` and N are not read.
template <bool VEC, bool MAPPED, bool GROUPED = false>
__device__ __forceinline__ void flat_filter_tile(int metric, const float *__restrict__ q, int B, int D, const float *__restrict__ x,
                                                         const float *__restrict__ norms, int64_t S, int64_t stride,
                                                         const uint32_t *__restrict__ valid, const float *__restrict__ qnorm,
                                                         const float *__restrict__ thr, float c_rel, float c_abs,
                                                         int32_t *__restrict__ cand, int32_t *__restrict__ cnt, int cap, int n_qtiles,
                                                         const int32_t *__restrict__ rows, int64_t N, const FlatGroups grp = {}) {
    static_assert(!(MAPPED && GROUPED), "the grouped mode is over the table only");
    __shared__ float As[kFlatTile * kFlatLd];
    __shared__ float Bs[kFlatTile * kFlatLd];
    __shared__ float nxs[kFlatTile];
    __shared__ int oks[kFlatTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kFlatTile;
    if constexpr (MAPPED) flat_tile_rows_mapped(tid, r0, S, stride, rows, N, norms, oks, nxs);
    else flat_tile_rows(tid, r0, S, stride, valid, norms, oks, nxs);
    const int wr = (wave >> 1) * 64, wq = (wave & 1) * 64;
    const int l31 = lane & 31, lh = lane >> 5;
    const auto row_of = [&](int rl) { return FlatRow{flat_row_listed<MAPPED>(oks, rl), flat_row_value<MAPPED>(oks, rl, r0, stride), false, 0}; };
    for (int qt = blockIdx.y; qt < n_qtiles; qt += gridDim.y) {
        const int q0 = qt * kFlatTile;
        FlatAcc acc;
        acc.zero();
        for (int k0 = 0; k0 < D; k0 += kFlatDepth) {
            __syncthreads();  // the previous stage is consumed (first pass: the row tile's norms and flags are written)
            flat_f32_stage<VEC>(
                tid, k0, D, x, q, As, Bs, [&](int r) { return flat_row_slot<MAPPED>(oks, r, r0, S, stride, D); },
                [&](int r) { return FlatSlot{q0 + r < B, (int64_t)(q0 + r) * D}; });
            __syncthreads();
            flat_f32_contract(As, Bs, wr, wq, l31, lh, acc);
        }
#pragma unroll
        for (int qj = 0; qj < 2; ++qj) {
            const int qi = q0 + wq + qj * 32 + l31;
            if (qi >= B) continue;
            const uint32_t *mask = nullptr;
            if constexpr (GROUPED) mask = flat_group_mask(grp, qi);
            const FlatQuery Q = flat_query(qi, qnorm[qi], thr, 0.f, cand, cnt, cap, nullptr, 0, mask);
#pragma unroll
            for (int ri = 0; ri < 2; ++ri)
                flat_tile_epilogue<false, false, GROUPED>(metric, c_rel, c_abs, cap, Q, nxs, wr + ri * 32, lh,
                                                          [&](int reg) { return acc.tile(ri, qj)[reg]; }, row_of);
        }
    }
}
// The kernel over the table (what ran before there were lists), the MAPPED one over a list of selected rows, and the GROUPED one over
// the table with a bitmap per query.
template <bool VEC>
__global__ __launch_bounds__(256) void flat_filter_kernel(int metric, const float *__restrict__ q, int B, int D, const float *__restrict__ x,
                             const float *__restrict__ norms, int64_t S, int64_t stride, const uint32_t *__restrict__ valid,
                             const float *__restrict__ qnorm, const float *__restrict__ thr, float c_rel, float c_abs, int32_t *__restrict__ cand,
                             int32_t *__restrict__ cnt, int cap, int n_qtiles) {
    flat_filter_tile<VEC, false>(metric, q, B, D, x, norms, S, stride, valid, qnorm, thr, c_rel, c_abs, cand, cnt, cap, n_qtiles, nullptr, 0);
}
template <bool VEC>
__global__ __launch_bounds__(256) void flat_rows_filter_kernel(int metric, const float *__restrict__ q, int B, int D, const float *__restrict__ x,
                             const float *__restrict__ norms, int64_t S, int64_t stride, const uint32_t *__restrict__ valid,
                             const float *__restrict__ qnorm, const float *__restrict__ thr, float c_rel, float c_abs, int32_t *__restrict__ cand,
                             int32_t *__restrict__ cnt, int cap, int n_qtiles, const int32_t *__restrict__ rows, int64_t N) {
    flat_filter_tile<VEC, true>(metric, q, B, D, x, norms, S, stride, valid, qnorm, thr, c_rel, c_abs, cand, cnt, cap, n_qtiles, rows, N);
}
template <bool VEC>
__global__ __launch_bounds__(256) void flat_grouped_filter_kernel(int metric, const float *__restrict__ q, int B, int D, const float *__restrict__ x,
                             const float *__restrict__ norms, int64_t S, int64_t stride, const uint32_t *__restrict__ valid,
                             const float *__restrict__ qnorm, const float *__restrict__ thr, float c_rel, float c_abs, int32_t *__restrict__ cand,
                             int32_t *__restrict__ cnt, int cap, int n_qtiles, const FlatGroups grp) {
    flat_filter_tile<VEC, false, true>(metric, q, B, D, x, norms, S, stride, valid, qnorm, thr, c_rel, c_abs, cand, cnt, cap, n_qtiles, nullptr, 0,
                                       grp);
}

// ---- the split filter: the same scores from three bf16 MFMAs over CENTRED rows ("split filter") -----------
// Each f32 value c = fl(x_j - mu_j) (mu = 0 without a centre) is carried as c_h + c_l, c_h = bf16(c), c_l = bf16(fl(c - c_h)), both by
// the hardware's round-to-nearest-even conversion, and  q.x ~ q_h.x_h + q_h.x_l + q_l.x_h  on v_mfma_f32_32x32x16_bf16 (three MFMAs of
// K = 16 where the f32 form issues eight of K = 2).  The rows are split while they are staged into LDS -- the table in HBM is the f32
// one --, the queries once per call (flat_split_queries_kernel).  norms / qnorm are the norms of the CENTRED values.
// LDS: two bf16 planes per operand, 32 coordinates (two K steps) per stage, row pitch 40 bf16 = 80 bytes = 5 slots of 16 bytes.  A lane
// reads the 8 coordinates 8 (lane >> 5) .. of row lane & 31 as one ds_read_b128; the 16 lanes that instruction serves together hold
// rows that are distinct mod 16, and 5 r mod 16 is a permutation: every lane group covers the 64 banks once.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int kSplitDepth = 32;             // coordinates per LDS stage
constexpr int kSplitLd = kSplitDepth + 8;   // LDS row pitch in bf16
constexpr int64_t kSplitMaxDim = 32768;     // the slack's derivation holds up to here

__device__ __forceinline__ void split_bf16(float c, __bf16 &h, __bf16 &l) {
    h = (__bf16)c;
    l = (__bf16)(c - (float)h);  // (the difference is exact; an infinite c gives (inf, NaN): the score is NaN and the row passes)
}

// qh / ql bf16 [B][Dp] (Dp = D rounded up to 16, the padding zero) and qnorm[b] = |fl(q - mu)|^2 in flat_norms_kernel's chain.
__global__ __launch_bounds__(256) void flat_split_queries_kernel(const float *__restrict__ q, int B, int D, int Dp, const float *__restrict__ mu,
                                                                __bf16 *__restrict__ qh, __bf16 *__restrict__ ql, float *__restrict__ qnorm) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float *qr = q + (int64_t)b * D;
    float s = 0.f;
    for (int j = lane; j < Dp; j += 64) {
        float c = 0.f;
        if (j < D) {
            c = mu ? qr[j] - mu[j] : qr[j];
            s = __builtin_fmaf(c, c, s);
        }
        __bf16 h, l;
        split_bf16(c, h, l);
        qh[(int64_t)b * Dp + j] = h;
        ql[(int64_t)b * Dp + j] = l;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) qnorm[b] = s;
}

// One LDS stage of NP planes of 2-byte values (V: eight of them, one 16-byte slot; bf16 or f16): coordinates k0 .. k0 + kSplitDepth of
// the tile's kFlatTile rows, plane p of row r from src[p] + row_at(r).off -- zeros at or past coordinate `lim` (a multiple of 8) and
// for a slot that is not ok -- to dst[p] at pitch kSplitLd.  256 threads.
template <class V, int NP, class E, class RowAt>
__device__ __forceinline__ void flat_stage_planes(int tid, int k0, int lim, const E *const (&src)[NP], E *const (&dst)[NP], RowAt &&row_at) {
#pragma unroll
    for (int i = 0; i < kSplitDepth / 16; ++i) {
        const int e = tid + i * 256;  // slots of 8 values per plane
        const int r = e / (kSplitDepth / 8), c = (e % (kSplitDepth / 8)) * 8;
        const FlatSlot s = row_at(r);
        V v[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
#pragma unroll
            for (int t = 0; t < 8; ++t) v[p][t] = (E)0.f;
        }
        if (s.ok && k0 + c < lim) {  // (every plane's load before the first store)
#pragma unroll
            for (int p = 0; p < NP; ++p) v[p] = *(const V *)(src[p] + s.off + k0 + c);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) *(V *)(dst[p] + r * kSplitLd + c) = v[p];
    }
}

// The split filter's K loop over one stage: the wave's 64 rows (from wr) x 64 queries (from wq), per K step of 16 the products h.h, h.l
// and l.h on v_mfma_f32_32x32x16_bf16 -- twelve MFMAs; a K step of padding only ends the loop.  A macro, not a function like
// flat_f32_contract: as an inlined function over the four planes (whole loop or single step, with or without the early exit, generic or
// LDS pointers) all eight fragment loads of a K step are issued ahead of its first MFMA where the text form issues four and interleaves
// the rest -- four more fragments live at once, 18 VGPRs in ivf_flat_split_filter_kernel; as text in the kernel, none.
#define FLAT_BF16X3_CONTRACT(Ah, Al, Bh, Bl, k0, D, wr, wq, l31, lh, acc)                                                                              \
    do {                                                                                                                                               \
    _Pragma("unroll")                                                                                                                                  \
        for (int kk = 0; kk < kSplitDepth; kk += 16) {                                                                                                 \
            if (k0 + kk >= D) break;                                                                                                                   \
            const int kc = kk + 8 * lh;                                                                                                                \
            const bf16x8 a0h = *(const bf16x8 *)(Ah + (wr + l31) * kSplitLd + kc), a0l = *(const bf16x8 *)(Al + (wr + l31) * kSplitLd + kc);           \
            const bf16x8 a1h = *(const bf16x8 *)(Ah + (wr + 32 + l31) * kSplitLd + kc), a1l = *(const bf16x8 *)(Al + (wr + 32 + l31) * kSplitLd + kc); \
            const bf16x8 b0h = *(const bf16x8 *)(Bh + (wq + l31) * kSplitLd + kc), b0l = *(const bf16x8 *)(Bl + (wq + l31) * kSplitLd + kc);           \
            const bf16x8 b1h = *(const bf16x8 *)(Bh + (wq + 32 + l31) * kSplitLd + kc), b1l = *(const bf16x8 *)(Bl + (wq + 32 + l31) * kSplitLd + kc); \
            acc.c00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b0h, acc.c00, 0, 0, 0);                                                             \
            acc.c01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b1h, acc.c01, 0, 0, 0);                                                             \
            acc.c10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b0h, acc.c10, 0, 0, 0);                                                             \
            acc.c11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b1h, acc.c11, 0, 0, 0);                                                             \
            acc.c00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b0l, acc.c00, 0, 0, 0);                                                             \
            acc.c01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0h, b1l, acc.c01, 0, 0, 0);                                                             \
            acc.c10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b0l, acc.c10, 0, 0, 0);                                                             \
            acc.c11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1h, b1l, acc.c11, 0, 0, 0);                                                             \
            acc.c00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0l, b0h, acc.c00, 0, 0, 0);                                                             \
            acc.c01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0l, b1h, acc.c01, 0, 0, 0);                                                             \
            acc.c10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1l, b0h, acc.c10, 0, 0, 0);                                                             \
            acc.c11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1l, b1h, acc.c11, 0, 0, 0);                                                             \
        }                                                                                                                                              \
    } while (0)

// flat_filter_kernel's job, grid and tile.  scores != NULL (tests, measurements): v of every (query, stage row) pair goes to
// scores f32 [B][S] as well.
template <bool VEC, bool MAPPED, bool GROUPED = false>
__device__ __forceinline__ void flat_split_filter_tile(int metric, const __bf16 *__restrict__ qh, const __bf16 *__restrict__ ql, int B,
                                                               int D, int Dp, const float *__restrict__ x, const float *__restrict__ mu,
                                                               const float *__restrict__ norms, int64_t S, int64_t stride,
                                                               const uint32_t *__restrict__ valid, const float *__restrict__ qnorm,
                                                               const float *__restrict__ thr, float c_rel, float c_abs,
                                                               int32_t *__restrict__ cand, int32_t *__restrict__ cnt, int cap, int n_qtiles,
                                                               float *__restrict__ scores, const int32_t *__restrict__ rows, int64_t N,
                                                               const FlatGroups grp = {}) {
    static_assert(!(MAPPED && GROUPED), "the grouped mode is over the table only");
    __shared__ __attribute__((aligned(16))) __bf16 Ah[kFlatTile * kSplitLd];
    __shared__ __attribute__((aligned(16))) __bf16 Al[kFlatTile * kSplitLd];
    __shared__ __attribute__((aligned(16))) __bf16 Bh[kFlatTile * kSplitLd];
    __shared__ __attribute__((aligned(16))) __bf16 Bl[kFlatTile * kSplitLd];
    __shared__ float nxs[kFlatTile];
    __shared__ int oks[kFlatTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kFlatTile;
    if constexpr (MAPPED) flat_tile_rows_mapped(tid, r0, S, stride, rows, N, norms, oks, nxs);
    else flat_tile_rows(tid, r0, S, stride, valid, norms, oks, nxs);
    const int wr = (wave >> 1) * 64, wq = (wave & 1) * 64;
    const int l31 = lane & 31, lh = lane >> 5;
    const __bf16 *const qp[2] = {qh, ql};
    __bf16 *const bp[2] = {Bh, Bl};
    const auto row_of = [&](int rl) {
        return FlatRow{flat_row_listed<MAPPED>(oks, rl), flat_row_value<MAPPED>(oks, rl, r0, stride), r0 + rl < S, r0 + rl};
    };
    for (int qt = blockIdx.y; qt < n_qtiles; qt += gridDim.y) {
        const int q0 = qt * kFlatTile;
        FlatAcc acc;
        acc.zero();
        for (int k0 = 0; k0 < D; k0 += kSplitDepth) {
            __syncthreads();  // the previous stage is consumed (first pass: the row tile's norms and flags are written)
            // rows: f32 from HBM, centred, split, two planes
            if constexpr (VEC) {
#pragma unroll
                for (int i = 0; i < kSplitDepth / 8; ++i) {
                    const int e = tid + i * 256;  // slots of 4 floats
                    const int r = e / (kSplitDepth / 4), c = (e % (kSplitDepth / 4)) * 4;
                    f32x4 cv = {0.f, 0.f, 0.f, 0.f};
                    const FlatSlot sa = flat_row_slot<MAPPED>(oks, r, r0, S, stride, D);
                    if (sa.ok && k0 + c < D) {
                        cv = *(const f32x4 *)(x + sa.off + k0 + c);
                        if (mu) cv = cv - *(const f32x4 *)(mu + k0 + c);
                    }
                    bf16x4 h4, l4;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        __bf16 h, l;
                        split_bf16(cv[t], h, l);
                        h4[t] = h, l4[t] = l;
                    }
                    *(bf16x4 *)(Ah + r * kSplitLd + c) = h4;
                    *(bf16x4 *)(Al + r * kSplitLd + c) = l4;
                }
            } else {
#pragma unroll 4
                for (int i = 0; i < kSplitDepth / 2; ++i) {
                    const int e = tid + i * 256;  // single floats
                    const int r = e / kSplitDepth, c = e % kSplitDepth;
                    const FlatSlot sa = flat_row_slot<MAPPED>(oks, r, r0, S, stride, D);
                    float cv = 0.f;
                    if (sa.ok && k0 + c < D) {
                        cv = x[sa.off + k0 + c];
                        if (mu) cv = cv - mu[k0 + c];
                    }
                    __bf16 h, l;
                    split_bf16(cv, h, l);
                    Ah[r * kSplitLd + c] = h;
                    Al[r * kSplitLd + c] = l;
                }
            }
            // queries: the planes of flat_split_queries_kernel (Dp is a multiple of 8 coordinates)
            flat_stage_planes<bf16x8>(tid, k0, Dp, qp, bp, [&](int r) { return FlatSlot{q0 + r < B, (int64_t)(q0 + r) * Dp}; });
            __syncthreads();
            FLAT_BF16X3_CONTRACT(Ah, Al, Bh, Bl, k0, D, wr, wq, l31, lh, acc);
        }
#pragma unroll
        for (int qj = 0; qj < 2; ++qj) {
            const int qi = q0 + wq + qj * 32 + l31;
            if (qi >= B) continue;
            const uint32_t *mask = nullptr;
            if constexpr (GROUPED) mask = flat_group_mask(grp, qi);
            const FlatQuery Q = flat_query(qi, qnorm[qi], thr, 0.f, cand, cnt, cap, scores, S, mask);
#pragma unroll
            for (int ri = 0; ri < 2; ++ri)
                flat_tile_epilogue<false, true, GROUPED>(metric, c_rel, c_abs, cap, Q, nxs, wr + ri * 32, lh,
                                                         [&](int reg) { return acc.tile(ri, qj)[reg]; }, row_of);
        }
    }
}
// The kernel over the table (what ran before there were lists), and the MAPPED one over a list of selected rows.
template <bool VEC>
__global__ __launch_bounds__(256) void flat_split_filter_kernel(int metric, const __bf16 *__restrict__ qh, const __bf16 *__restrict__ ql, int B,
                             int D, int Dp, const float *__restrict__ x, const float *__restrict__ mu, const float *__restrict__ norms, int64_t S,
                             int64_t stride, const uint32_t *__restrict__ valid, const float *__restrict__ qnorm, const float *__restrict__ thr,
                             float c_rel, float c_abs, int32_t *__restrict__ cand, int32_t *__restrict__ cnt, int cap, int n_qtiles,
                             float *__restrict__ scores) {
    flat_split_filter_tile<VEC, false>(metric, qh, ql, B, D, Dp, x, mu, norms, S, stride, valid, qnorm, thr, c_rel, c_abs, cand, cnt, cap, n_qtiles,
                                       scores, nullptr, 0);
}
template <bool VEC>
__global__ __launch_bounds__(256) void flat_rows_split_filter_kernel(int metric, const __bf16 *__restrict__ qh, const __bf16 *__restrict__ ql, int B,
                             int D, int Dp, const float *__restrict__ x, const float *__restrict__ mu, const float *__restrict__ norms, int64_t S,
                             int64_t stride, const uint32_t *__restrict__ valid, const float *__restrict__ qnorm, const float *__restrict__ thr,
                             float c_rel, float c_abs, int32_t *__restrict__ cand, int32_t *__restrict__ cnt, int cap, int n_qtiles,
                             float *__restrict__ scores, const int32_t *__restrict__ rows, int64_t N) {
    flat_split_filter_tile<VEC, true>(metric, qh, ql, B, D, Dp, x, mu, norms, S, stride, valid, qnorm, thr, c_rel, c_abs, cand, cnt, cap, n_qtiles,
                                      scores, rows, N);
}
template <bool VEC>
__global__ __launch_bounds__(256) void flat_grouped_split_filter_kernel(int metric, const __bf16 *__restrict__ qh, const __bf16 *__restrict__ ql,
                             int B, int D, int Dp, const float *__restrict__ x, const float *__restrict__ mu, const float *__restrict__ norms,
                             int64_t S, int64_t stride, const uint32_t *__restrict__ valid, const float *__restrict__ qnorm,
                             const float *__restrict__ thr, float c_rel, float c_abs, int32_t *__restrict__ cand, int32_t *__restrict__ cnt, int cap,
                             int n_qtiles, float *__restrict__ scores, const FlatGroups grp) {
    flat_split_filter_tile<VEC, false, true>(metric, qh, ql, B, D, Dp, x, mu, norms, S, stride, valid, qnorm, thr, c_rel, c_abs, cand, cnt, cap,
                                             n_qtiles, scores, nullptr, 0, grp);
}

// ---- the f16 filter: rows STORED as f16 are exact MFMA operands ("f16 rows") --------------------------------
// No centring, no split of the rows and no conversion while they are staged: the row tile is copied from HBM to LDS as it is.  Only the
// f32 query is split: q' = q 2^e (e per query, so that max |q'| lies in [2^14, 2^15): exact, inside the f16 range), q'_h = f16(q'),
// q'_l = f16(q' - q'_h) (the difference is exact), and  q.x ~ 2^-e (x.q'_h + x.q'_l)  on v_mfma_f32_32x32x16_f16: two MFMAs of K = 16.
// Three LDS planes (rows, q'_h, q'_l) in the split kernel's image: 32 coordinates per stage, row pitch 40 f16 = 80 bytes.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// qh / ql f16 [B][Dp] (Dp = D rounded up to 16, the padding zero), qnorm[b] = |q|^2 of the UNSCALED query in flat_norms_kernel's chain,
// qscale[b] = 2^-e, qflush[b] = 1.001 * 2 * 2^-14 * sum |q_j|: what the scores may lose if the MFMA flushes f16 subnormal row operands
// (an absolute term of the slack, added to the bound).  e = 14 - floor(log2 max |q_j|), clamped to [-126, 126] (2^e and 2^-e stay
// normal f32 numbers); 0 for an all-zero or non-finite query -- the latter's planes hold inf / NaN: its scores are NaN and pass.
__global__ __launch_bounds__(256) void flat_f16_queries_kernel(const float *__restrict__ q, int B, int D, int Dp, _Float16 *__restrict__ qh,
                                                              _Float16 *__restrict__ ql, float *__restrict__ qnorm,
                                                              float *__restrict__ qscale, float *__restrict__ qflush) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float *qr = q + (int64_t)b * D;
    float s = 0.f, s1 = 0.f, m = 0.f;
    bool bad = false;
    for (int j = lane; j < D; j += 64) {
        const float c = qr[j];
        s = __builtin_fmaf(c, c, s);
        const float a = __builtin_fabsf(c);
        s1 += a;
        bad |= !(a < __builtin_inff());
        m = __builtin_fmaxf(m, a);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        s1 += __shfl_xor(s1, o);
        m = __builtin_fmaxf(m, __shfl_xor(m, o));
    }
    bad = __ballot(bad) != 0ull;
    int e = 0;
    if (!bad && m > 0.f) {
        int ex;
        (void)frexpf(m, &ex);  // m = f 2^ex, f in [0.5, 1): floor(log2 m) = ex - 1
        e = 15 - ex;
        e = e < -126 ? -126 : e > 126 ? 126 : e;
    }
    const float up = ldexpf(1.f, e);
    for (int j = lane; j < Dp; j += 64) {
        const float c = j < D ? qr[j] * up : 0.f;
        const _Float16 h = (_Float16)c;
        qh[(int64_t)b * Dp + j] = h;
        ql[(int64_t)b * Dp + j] = (_Float16)(c - (float)h);
    }
    if (lane == 0) {
        qnorm[b] = s;
        qscale[b] = ldexpf(1.f, -e);
        qflush[b] = s1 * (1.001f * 0x1p-13f);
    }
}

// flat_split_filter_kernel's job, grid, tile and epilogue over x f16 [..][D].  VEC: D % 8 == 0 and x aligned to 16 bytes.
template <bool VEC, bool MAPPED, bool GROUPED = false>
__device__ __forceinline__ void flat_f16_filter_tile(int metric, const _Float16 *__restrict__ qh, const _Float16 *__restrict__ ql, int B,
                                                             int D, int Dp, const _Float16 *__restrict__ x, const float *__restrict__ norms,
                                                             int64_t S, int64_t stride, const uint32_t *__restrict__ valid,
                                                             const float *__restrict__ qnorm, const float *__restrict__ qscale,
                                                             const float *__restrict__ qflush, const float *__restrict__ thr, float c_rel,
                                                             float c_abs, int32_t *__restrict__ cand, int32_t *__restrict__ cnt, int cap,
                                                             int n_qtiles, float *__restrict__ scores, const int32_t *__restrict__ rows,
                                                             int64_t N, const FlatGroups grp = {}) {
    static_assert(!(MAPPED && GROUPED), "the grouped mode is over the table only");
    __shared__ __attribute__((aligned(16))) _Float16 As[kFlatTile * kSplitLd];
    __shared__ __attribute__((aligned(16))) _Float16 Bh[kFlatTile * kSplitLd];
    __shared__ __attribute__((aligned(16))) _Float16 Bl[kFlatTile * kSplitLd];
    __shared__ float nxs[kFlatTile];
    __shared__ int oks[kFlatTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kFlatTile;
    if constexpr (MAPPED) flat_tile_rows_mapped(tid, r0, S, stride, rows, N, norms, oks, nxs);
    else flat_tile_rows(tid, r0, S, stride, valid, norms, oks, nxs);
    const int wr = (wave >> 1) * 64, wq = (wave & 1) * 64;
    const int l31 = lane & 31, lh = lane >> 5;
    const _Float16 *const xp[1] = {x}, *const qp[2] = {qh, ql};
    _Float16 *const ap[1] = {As}, *const bp[2] = {Bh, Bl};
    const auto row_of = [&](int rl) {
        return FlatRow{flat_row_listed<MAPPED>(oks, rl), flat_row_value<MAPPED>(oks, rl, r0, stride), r0 + rl < S, r0 + rl};
    };
    for (int qt = blockIdx.y; qt < n_qtiles; qt += gridDim.y) {
        const int q0 = qt * kFlatTile;
        FlatAcc acc;
        acc.zero();
        for (int k0 = 0; k0 < D; k0 += kSplitDepth) {
            __syncthreads();  // the previous stage is consumed (first pass: the row tile's norms and flags are written)
            // rows: f16 from HBM as they are
            if constexpr (VEC) {
                flat_stage_planes<f16x8>(tid, k0, D, xp, ap, [&](int r) { return flat_row_slot<MAPPED>(oks, r, r0, S, stride, D); });
            } else {
#pragma unroll 4
                for (int i = 0; i < kSplitDepth / 2; ++i) {
                    const int e = tid + i * 256;  // single values
                    const int r = e / kSplitDepth, c = e % kSplitDepth;
                    const FlatSlot sa = flat_row_slot<MAPPED>(oks, r, r0, S, stride, D);
                    As[r * kSplitLd + c] = (sa.ok && k0 + c < D) ? x[sa.off + k0 + c] : (_Float16)0.f;
                }
            }
            // queries: the planes of flat_f16_queries_kernel (Dp is a multiple of 8 coordinates)
            flat_stage_planes<f16x8>(tid, k0, Dp, qp, bp, [&](int r) { return FlatSlot{q0 + r < B, (int64_t)(q0 + r) * Dp}; });
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < kSplitDepth; kk += 16) {
                if (k0 + kk >= D) break;  // (a K step of padding only)
                const int kc = kk + 8 * lh;
                const f16x8 a0 = *(const f16x8 *)(As + (wr + l31) * kSplitLd + kc), a1 = *(const f16x8 *)(As + (wr + 32 + l31) * kSplitLd + kc);
                const f16x8 b0h = *(const f16x8 *)(Bh + (wq + l31) * kSplitLd + kc), b0l = *(const f16x8 *)(Bl + (wq + l31) * kSplitLd + kc);
                const f16x8 b1h = *(const f16x8 *)(Bh + (wq + 32 + l31) * kSplitLd + kc), b1l = *(const f16x8 *)(Bl + (wq + 32 + l31) * kSplitLd + kc);
                acc.c00 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0h, acc.c00, 0, 0, 0);
                acc.c01 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1h, acc.c01, 0, 0, 0);
                acc.c10 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0h, acc.c10, 0, 0, 0);
                acc.c11 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1h, acc.c11, 0, 0, 0);
                acc.c00 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0l, acc.c00, 0, 0, 0);
                acc.c01 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1l, acc.c01, 0, 0, 0);
                acc.c10 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0l, acc.c10, 0, 0, 0);
                acc.c11 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1l, acc.c11, 0, 0, 0);
            }
        }
        // the accumulator back to the query's scale: that is this kernel's dot product
#pragma unroll
        for (int qj = 0; qj < 2; ++qj) {
            const int qi = q0 + wq + qj * 32 + l31;
            if (qi >= B) continue;
            const uint32_t *mask = nullptr;
            if constexpr (GROUPED) mask = flat_group_mask(grp, qi);
            const FlatQuery Q = flat_query(qi, qnorm[qi], thr, qflush[qi], cand, cnt, cap, scores, S, mask);
            const float down = qscale[qi];
#pragma unroll
            for (int ri = 0; ri < 2; ++ri)
                flat_tile_epilogue<true, true, GROUPED>(metric, c_rel, c_abs, cap, Q, nxs, wr + ri * 32, lh,
                                                        [&](int reg) { return acc.tile(ri, qj)[reg] * down; }, row_of);
        }
    }
}
// The kernel over the table (what ran before there were lists), and the MAPPED one over a list of selected rows.
template <bool VEC>
__global__ __launch_bounds__(256) void flat_f16_filter_kernel(int metric, const _Float16 *__restrict__ qh, const _Float16 *__restrict__ ql, int B,
                             int D, int Dp, const _Float16 *__restrict__ x, const float *__restrict__ norms, int64_t S, int64_t stride,
                             const uint32_t *__restrict__ valid, const float *__restrict__ qnorm, const float *__restrict__ qscale,
                             const float *__restrict__ qflush, const float *__restrict__ thr, float c_rel, float c_abs, int32_t *__restrict__ cand,
                             int32_t *__restrict__ cnt, int cap, int n_qtiles, float *__restrict__ scores) {
    flat_f16_filter_tile<VEC, false>(metric, qh, ql, B, D, Dp, x, norms, S, stride, valid, qnorm, qscale, qflush, thr, c_rel, c_abs, cand, cnt, cap,
                                     n_qtiles, scores, nullptr, 0);
}
template <bool VEC>
__global__ __launch_bounds__(256) void flat_rows_f16_filter_kernel(int metric, const _Float16 *__restrict__ qh, const _Float16 *__restrict__ ql,
                             int B, int D, int Dp, const _Float16 *__restrict__ x, const float *__restrict__ norms, int64_t S, int64_t stride,
                             const uint32_t *__restrict__ valid, const float *__restrict__ qnorm, const float *__restrict__ qscale,
                             const float *__restrict__ qflush, const float *__restrict__ thr, float c_rel, float c_abs, int32_t *__restrict__ cand,
                             int32_t *__restrict__ cnt, int cap, int n_qtiles, float *__restrict__ scores, const int32_t *__restrict__ rows,
                             int64_t N) {
    flat_f16_filter_tile<VEC, true>(metric, qh, ql, B, D, Dp, x, norms, S, stride, valid, qnorm, qscale, qflush, thr, c_rel, c_abs, cand, cnt, cap,
                                    n_qtiles, scores, rows, N);
}
template <bool VEC>
__global__ __launch_bounds__(256) void flat_grouped_f16_filter_kernel(int metric, const _Float16 *__restrict__ qh, const _Float16 *__restrict__ ql,
                             int B, int D, int Dp, const _Float16 *__restrict__ x, const float *__restrict__ norms, int64_t S, int64_t stride,
                             const uint32_t *__restrict__ valid, const float *__restrict__ qnorm, const float *__restrict__ qscale,
                             const float *__restrict__ qflush, const float *__restrict__ thr, float c_rel, float c_abs, int32_t *__restrict__ cand,
                             int32_t *__restrict__ cnt, int cap, int n_qtiles, float *__restrict__ scores, const FlatGroups grp) {
    flat_f16_filter_tile<VEC, false, true>(metric, qh, ql, B, D, Dp, x, norms, S, stride, valid, qnorm, qscale, qflush, thr, c_rel, c_abs, cand, cnt,
                                           cap, n_qtiles, scores, nullptr, 0, grp);
}

// ---- the int8 filter: rows STORED as int8 codes, an exact-integer contraction ("int8 rows") -------------------
// A stored byte c (|c| <= 127) stands for the value s c, s = 2^ls the store's scale.  The f32 query becomes an integer: q' = q s 2^e (e per
// query, so that max |q'| lies in [2^19, 2^20): s is folded in, so that <q, s c> = 2^-e sum q'_j c_j), Q = rne(q'), |Q| <= 2^20, split into
// three balanced base-128 digits Q = d2 2^14 + d1 2^7 + d0, d0, d1 in [-64, 63], d2 in [-64, 64]: three int8 planes.  Per K step of 32
// three v_mfma_i32_32x32x32_i8, one per plane, each into i32 accumulators of its own (|sum c d| <= D 127 64 < 2^31 for D <= 32768); the
// epilogue recombines T = S2 2^14 + S1 2^7 + S0 in 64-bit integers -- exactly sum Q_j c_j: the contraction has NO rounding -- converts
// T to f32 once and multiplies by 2^-e.  What is left of the error is |q' - Q| <= 1/2 per coordinate, carried by the per-query term.
//
// Operand map of v_mfma_i32_32x32x32_i8 as used here (four VGPRs = 16 bytes per operand and lane): lane l, r = l & 31, h = l >> 5,
// holds A[row r][k = 16 h + j] and B[k = 16 h + j][col r] in byte j = 0 .. 15 of its fragment, bytes signed; C/D is the map of every
// 32 x 32 form (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).  Checked with exact data, an asymmetric B and
// D = 5 / 32 / 40 / 96 in tests/test_flat_i8_search.py -- once with small integer queries, whose Q = 8 q 2^14 lives in the d2 plane alone, and
// once with queries whose Q has all three digits non-zero and a known fractional part (the three planes share the fragment loads, but the
// weights 2^14 / 2^7 / 1 of the recombination and Q = rne(q') are pinned only by the second): which operand is rows and which queries, the
// two lane halves taking different 16-byte chunks that together cover the K step, and the C tile's orientation all show there.  (A permutation of k INSIDE a lane's 16 bytes that is
// the same for A and B cannot show in a contraction and does not matter to one.)
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int kI8Depth = 64;            // coordinates = bytes per LDS stage: two K steps of 32
constexpr int kI8Ld = kI8Depth + 16;    // LDS row pitch in bytes: 80, the image of the split and f16 kernels
constexpr int kI8Threads = 512;         // 8 waves: 64 rows x 32 queries each, 2 MFMA tiles x 3 planes = 96 accumulator registers

// p0 / p1 / p2 int8 [B][Dp] (Dp = D rounded up to 32, the padding zero): the digits d0, d1, d2.  qnorm[b] = |q|^2 of the UNSCALED query in
// flat_norms_kernel's chain, qscale[b] = 2^-e, qslack[b] = 1.001 * 127 * D * 2^-e: the per-query term of the slack -- |q'_j - Q_j| <= 1/2
// and |c_j| <= 127 put at most D 127 / 2 between sum q'_j c_j and sum Q_j c_j, twice that on 2 dot -- (0 for an all-zero query, whose
// planes are exact).  E = e + ls = 20 - ex (max |q_j| = f 2^ex, f in [0.5, 1)), clamped from
// above so that 2^E and 2^-e stay normal f32 numbers -- a smaller E only makes |Q| smaller.  A query with a NaN or an infinity, or one so large
// that E would have to be RAISED to stay normal (|q|^2 is infinite there), has no integer planes: they are zero and qslack = +inf --
// every row passes, the list overflows and the query takes the all-rows route.
__global__ __launch_bounds__(256) void flat_i8_queries_kernel(const float *__restrict__ q, int B, int D, int Dp, int ls, int8_t *__restrict__ p0,
                                                             int8_t *__restrict__ p1, int8_t *__restrict__ p2, float *__restrict__ qnorm,
                                                             float *__restrict__ qscale, float *__restrict__ qslack) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float *qr = q + (int64_t)b * D;
    float s = 0.f, m = 0.f;
    bool bad = false;
    for (int j = lane; j < D; j += 64) {
        const float c = qr[j];
        s = __builtin_fmaf(c, c, s);
        const float a = __builtin_fabsf(c);
        bad |= !(a < __builtin_inff());
        m = __builtin_fmaxf(m, a);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        m = __builtin_fmaxf(m, __shfl_xor(m, o));
    }
    bad = __ballot(bad) != 0ull;
    const bool zero = !bad && !(m > 0.f);
    int E = ls;  // (e = 0: what an all-zero or unexpressible query is given)
    if (!bad && !zero) {
        int ex;
        (void)frexpf(m, &ex);
        E = 20 - ex;
        const int lo = ls - 126 > -126 ? ls - 126 : -126, hi = ls + 126 < 126 ? ls + 126 : 126;
        if (E < lo) bad = true, E = ls;
        else if (E > hi) E = hi;
    }
    const float up = ldexpf(1.f, E);
    for (int j = lane; j < Dp; j += 64) {
        int Q = 0;
        if (!bad && j < D) Q = (int)rintf(qr[j] * up);  // (|q' | < 2^20 (1 + 2^-23): the conversion is exact)
        const int d0 = ((Q + 64) & 127) - 64;
        const int Q1 = (Q - d0) >> 7;  // (a multiple of 128: the shift is exact)
        const int d1 = ((Q1 + 64) & 127) - 64;
        const int d2 = (Q1 - d1) >> 7;
        p0[(int64_t)b * Dp + j] = (int8_t)d0;
        p1[(int64_t)b * Dp + j] = (int8_t)d1;
        p2[(int64_t)b * Dp + j] = (int8_t)d2;
    }
    if (lane == 0) {
        qnorm[b] = s;
        qscale[b] = ldexpf(1.f, ls - E);
        qslack[b] = bad ? __builtin_inff() : zero ? 0.f : ldexpf(1.f, ls - E) * (127.f * 1.001f * (float)D);
    }
}

// flat_f16_filter_kernel's job, grid, 128 x 128 workgroup tile, epilogue and `scores` output over x int8 [..][D], on 8 waves of 64 rows x
// 32 queries.  VEC: D % 16 == 0 and x aligned to 16 bytes.
template <bool VEC, bool MAPPED, bool GROUPED = false>
__device__ __forceinline__ void flat_i8_filter_tile(int metric, const int8_t *__restrict__ p0, const int8_t *__restrict__ p1,
                                                                   const int8_t *__restrict__ p2, int B, int D, int Dp,
                                                                   const int8_t *__restrict__ x, const float *__restrict__ norms, int64_t S,
                                                                   int64_t stride, const uint32_t *__restrict__ valid,
                                                                   const float *__restrict__ qnorm, const float *__restrict__ qscale,
                                                                   const float *__restrict__ qslack, const float *__restrict__ thr, float c_rel,
                                                                   float c_abs, int32_t *__restrict__ cand, int32_t *__restrict__ cnt, int cap,
                                                                   int n_qtiles, float *__restrict__ scores, const int32_t *__restrict__ rows,
                                                                   int64_t N, const FlatGroups grp = {}) {
    static_assert(!(MAPPED && GROUPED), "the grouped mode is over the table only");
    __shared__ __attribute__((aligned(16))) int8_t As[kFlatTile * kI8Ld];
    __shared__ __attribute__((aligned(16))) int8_t B0[kFlatTile * kI8Ld];
    __shared__ __attribute__((aligned(16))) int8_t B1[kFlatTile * kI8Ld];
    __shared__ __attribute__((aligned(16))) int8_t B2[kFlatTile * kI8Ld];
    __shared__ float nxs[kFlatTile];
    __shared__ int oks[kFlatTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kFlatTile;
    if constexpr (MAPPED) flat_tile_rows_mapped(tid, r0, S, stride, rows, N, norms, oks, nxs);
    else flat_tile_rows(tid, r0, S, stride, valid, norms, oks, nxs);
    const int wr = (wave >> 2) * 64, wq = (wave & 3) * 32;
    const int l31 = lane & 31, lh = lane >> 5;
    const int sr = tid >> 2, sc = (tid & 3) * 16;  // the thread's slot of 16 bytes in a stage: 128 rows x 4 slots
    const auto row_of = [&](int rl) {
        return FlatRow{flat_row_listed<MAPPED>(oks, rl), flat_row_value<MAPPED>(oks, rl, r0, stride), r0 + rl < S, r0 + rl};
    };
    for (int qt = blockIdx.y; qt < n_qtiles; qt += gridDim.y) {
        const int q0 = qt * kFlatTile;
        i32x16 s0a, s0b, s1a, s1b, s2a, s2b;  // plane 0 / 1 / 2, rows wr .. wr + 31 (a) and wr + 32 .. wr + 63 (b)
#pragma unroll
        for (int e = 0; e < 16; ++e) s0a[e] = s0b[e] = s1a[e] = s1b[e] = s2a[e] = s2b[e] = 0;
        for (int k0 = 0; k0 < D; k0 += kI8Depth) {
            __syncthreads();  // the previous stage is consumed (first pass: the row tile's norms and flags are written)
            // rows: the bytes from HBM as they are
            if constexpr (VEC) {
                i32x4 va = {0, 0, 0, 0};
                const FlatSlot sa = flat_row_slot<MAPPED>(oks, sr, r0, S, stride, D);
                if (sa.ok && k0 + sc < D) va = *(const i32x4 *)(x + sa.off + k0 + sc);
                *(i32x4 *)(As + sr * kI8Ld + sc) = va;
            } else {
#pragma unroll 4
                for (int i = 0; i < kFlatTile * kI8Depth / kI8Threads; ++i) {
                    const int e = tid + i * kI8Threads;  // single bytes
                    const int r = e / kI8Depth, c = e % kI8Depth;
                    const FlatSlot sa = flat_row_slot<MAPPED>(oks, r, r0, S, stride, D);
                    As[r * kI8Ld + c] = (sa.ok && k0 + c < D) ? x[sa.off + k0 + c] : (int8_t)0;
                }
            }
            // queries: the planes of flat_i8_queries_kernel, 16 bytes at a time (Dp is a multiple of 32 coordinates)
            {
                i32x4 v0 = {0, 0, 0, 0}, v1 = {0, 0, 0, 0}, v2 = {0, 0, 0, 0};
                const int qq = q0 + sr;
                if (qq < B && k0 + sc < Dp) {
                    v0 = *(const i32x4 *)(p0 + (int64_t)qq * Dp + k0 + sc);
                    v1 = *(const i32x4 *)(p1 + (int64_t)qq * Dp + k0 + sc);
                    v2 = *(const i32x4 *)(p2 + (int64_t)qq * Dp + k0 + sc);
                }
                *(i32x4 *)(B0 + sr * kI8Ld + sc) = v0;
                *(i32x4 *)(B1 + sr * kI8Ld + sc) = v1;
                *(i32x4 *)(B2 + sr * kI8Ld + sc) = v2;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < kI8Depth; kk += 32) {
                if (k0 + kk >= D) break;  // (a K step of padding only)
                const int kc = kk + 16 * lh;
                const i32x4 a0 = *(const i32x4 *)(As + (wr + l31) * kI8Ld + kc), a1 = *(const i32x4 *)(As + (wr + 32 + l31) * kI8Ld + kc);
                const i32x4 b0 = *(const i32x4 *)(B0 + (wq + l31) * kI8Ld + kc);
                const i32x4 b1 = *(const i32x4 *)(B1 + (wq + l31) * kI8Ld + kc);
                const i32x4 b2 = *(const i32x4 *)(B2 + (wq + l31) * kI8Ld + kc);
                s0a = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, s0a, 0, 0, 0);
                s0b = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, s0b, 0, 0, 0);
                s1a = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, s1a, 0, 0, 0);
                s1b = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, s1b, 0, 0, 0);
                s2a = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b2, s2a, 0, 0, 0);
                s2b = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b2, s2b, 0, 0, 0);
            }
        }
        // the three sums back into ONE integer, one conversion, the query's scale: that is this kernel's dot product.  A lane owns one query.
        const int qi = q0 + wq + l31;
        if (qi >= B) continue;
        const uint32_t *mask = nullptr;
        if constexpr (GROUPED) mask = flat_group_mask(grp, qi);
        const FlatQuery Q = flat_query(qi, qnorm[qi], thr, qslack[qi], cand, cnt, cap, scores, S, mask);
        const float down = qscale[qi];
#pragma unroll
        for (int ri = 0; ri < 2; ++ri) {
            const i32x16 &S0 = ri == 0 ? s0a : s0b, &S1 = ri == 0 ? s1a : s1b, &S2 = ri == 0 ? s2a : s2b;
            flat_tile_epilogue<true, true, GROUPED>(
                metric, c_rel, c_abs, cap, Q, nxs, wr + ri * 32, lh,
                [&](int reg) {
                    const int64_t T = (int64_t)S2[reg] * 16384 + (int64_t)S1[reg] * 128 + (int64_t)S0[reg];  // = sum Q_j c_j, |T| < 2^43
                    return (float)T * down;
                },
                row_of);
        }
    }
}
// The kernel over the table (what ran before there were lists), and the MAPPED one over a list of selected rows.
template <bool VEC>
__global__ __launch_bounds__(kI8Threads) void flat_i8_filter_kernel(int metric, const int8_t *__restrict__ p0, const int8_t *__restrict__ p1,
                             const int8_t *__restrict__ p2, int B, int D, int Dp, const int8_t *__restrict__ x, const float *__restrict__ norms,
                             int64_t S, int64_t stride, const uint32_t *__restrict__ valid, const float *__restrict__ qnorm,
                             const float *__restrict__ qscale, const float *__restrict__ qslack, const float *__restrict__ thr, float c_rel,
                             float c_abs, int32_t *__restrict__ cand, int32_t *__restrict__ cnt, int cap, int n_qtiles, float *__restrict__ scores) {
    flat_i8_filter_tile<VEC, false>(metric, p0, p1, p2, B, D, Dp, x, norms, S, stride, valid, qnorm, qscale, qslack, thr, c_rel, c_abs, cand, cnt,
                                    cap, n_qtiles, scores, nullptr, 0);
}
template <bool VEC>
__global__ __launch_bounds__(kI8Threads) void flat_rows_i8_filter_kernel(int metric, const int8_t *__restrict__ p0, const int8_t *__restrict__ p1,
                             const int8_t *__restrict__ p2, int B, int D, int Dp, const int8_t *__restrict__ x, const float *__restrict__ norms,
                             int64_t S, int64_t stride, const uint32_t *__restrict__ valid, const float *__restrict__ qnorm,
                             const float *__restrict__ qscale, const float *__restrict__ qslack, const float *__restrict__ thr, float c_rel,
                             float c_abs, int32_t *__restrict__ cand, int32_t *__restrict__ cnt, int cap, int n_qtiles, float *__restrict__ scores,
                             const int32_t *__restrict__ rows, int64_t N) {
    flat_i8_filter_tile<VEC, true>(metric, p0, p1, p2, B, D, Dp, x, norms, S, stride, valid, qnorm, qscale, qslack, thr, c_rel, c_abs, cand, cnt, cap,
                                   n_qtiles, scores, rows, N);
}
template <bool VEC>
__global__ __launch_bounds__(kI8Threads) void flat_grouped_i8_filter_kernel(int metric, const int8_t *__restrict__ p0, const int8_t *__restrict__ p1,
                             const int8_t *__restrict__ p2, int B, int D, int Dp, const int8_t *__restrict__ x, const float *__restrict__ norms,
                             int64_t S, int64_t stride, const uint32_t *__restrict__ valid, const float *__restrict__ qnorm,
                             const float *__restrict__ qscale, const float *__restrict__ qslack, const float *__restrict__ thr, float c_rel,
                             float c_abs, int32_t *__restrict__ cand, int32_t *__restrict__ cnt, int cap, int n_qtiles, float *__restrict__ scores,
                             const FlatGroups grp) {
    flat_i8_filter_tile<VEC, false, true>(metric, p0, p1, p2, B, D, Dp, x, norms, S, stride, valid, qnorm, qscale, qslack, thr, c_rel, c_abs, cand,
                                          cnt, cap, n_qtiles, scores, nullptr, 0, grp);
}

// ---- exact distances + top-k, a wave per query, ties by ROW ID ---------------------------------------------------------------------
// The per-lane partial sums, the butterfly and the epilogue are rerank_topk_kernel's (codec.hip), operation for operation: the
// distances are bit-equal to annlite_rerank_topk's.  What differs is the order among equal distances -- the row id instead of the
// position in the list, so the result does not depend on the order in which the filter's atomics filled the list -- and where the
// candidates come from:
//   list != NULL : the query's candidate list (min(cnt[b], cap) entries)
//   list == NULL : the rows c * stride, c < S (the first sample; a small table; the route of an overflowed query)
// Only rows valid in the bitmap are offered.  thr_out != NULL: the k-th smallest distance (raw, no sqrt; +inf with fewer than k
// rows) goes there -- a bound for the next filter stage -- instead of the result arrays.
// The chain itself, shared by every exact kernel of this file: up to 64 rows (one per lane, -1: none; n_here = lanes that were
// offered one) are scored against the wave's query and offered to its list.
template <class T>
__device__ __forceinline__ void flat_exact_chunk(int metric, const float *__restrict__ qr, int D, const T *__restrict__ x, int64_t N,
                                                 const uint32_t *__restrict__ valid, int64_t row, int n_here, int km1, int lane, WaveList &L,
                                                 uint32_t &th, uint32_t &tl, float scale = 1.f) {
    constexpr int U = 8;
    if (row >= N) row = -1;
    if (row >= 0 && valid && !((valid[row >> 5] >> (row & 31)) & 1u)) row = -1;
    if (__ballot(row >= 0) == 0ull) return;
    float mine = __builtin_inff();
    for (int u0 = 0; u0 < n_here; u0 += U) {
        float s[U];
        int64_t rw[U];
        bool any = false;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            rw[u] = __shfl(row, u0 + u);  // (wave-uniform)
            s[u] = 0.f;
            any |= rw[u] >= 0;
        }
        if (!any) continue;
        for (int j = lane; j < D; j += 64) {
            const float qj = qr[j];
            float xv[U];
            if constexpr (std::is_same<T, float>::value) {
#pragma unroll
                for (int u = 0; u < U; ++u) xv[u] = rw[u] >= 0 ? x[rw[u] * D + j] : 0.f;
            } else {
                // f16, int8: all eight loads are issued before the first value is widened, as the f32 form has them in flight together -- left
                // to itself the compiler widens each value right behind its load, and every load waits for itself: eight latencies in
                // a row.  So the loads are unconditional -- row 0 (it exists: some row of this batch is one of the table's) stands in
                // for a missing one -- and a scheduling barrier keeps the conversions behind them.
                T raw[U];
#pragma unroll
                for (int u = 0; u < U; ++u) raw[u] = x[(rw[u] >= 0 ? rw[u] : 0) * D + j];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    // (int8: the code times the store's power-of-two scale, exact; nothing else differs)
                    if constexpr (std::is_same<T, int8_t>::value) xv[u] = rw[u] >= 0 ? scale * (float)raw[u] : 0.f;
                    else xv[u] = rw[u] >= 0 ? (float)raw[u] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (metric == ANNLITE_METRIC_EUCLIDEAN) {
                    const float d = xv[u] - qj;
                    s[u] = __builtin_fmaf(d, d, s[u]);
                } else {
                    s[u] = __builtin_fmaf(xv[u], qj, s[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s[u] += __shfl_xor(s[u], o);
            const float dist = (metric == ANNLITE_METRIC_EUCLIDEAN) ? s[u] : 1.f - s[u];
            if (lane == u0 + u) mine = dist;
        }
    }
    const float tf = (th == kKeyInfHi) ? __builtin_inff() : ordered_to_f32(th);
    const unsigned long long pm = __ballot(row >= 0 && !(mine > tf));  // (NaN: behind +inf, numpy's order)
    if (pm) wavelist_offer(L, pm, f32_to_key(mine), (uint32_t)row, km1, th, tl, lane);
}

// ... and what becomes of the wave's list: the next stage's bound (thr_out != NULL) or the query's result row.
__device__ __forceinline__ void flat_exact_finish(const WaveList &L, int b, int k, int lane, int do_sqrt, float *__restrict__ thr_out,
                                                  float *__restrict__ out_d, int64_t *__restrict__ out_i) {
    const int km1 = k - 1;
    const bool none = (L.hi == kKeyInfHi && L.lo == kIdNone);
    float d = none ? __builtin_inff() : ordered_to_f32(L.hi);
    if (thr_out) {
        if (lane == km1) thr_out[b] = d;
        return;
    }
    if (lane <= km1) {
        const int64_t id = (none || d == __builtin_inff()) ? (int64_t)-1 : (int64_t)L.lo;
        if (do_sqrt) d = __builtin_sqrtf(d);
        out_d[(int64_t)b * k + lane] = d;
        out_i[(int64_t)b * k + lane] = id;
    }
}

// MAPPED (the `list == NULL` modes only): candidate c is rows[c * stride] of an ascending list of S selected offsets, not row c * stride.
// GROUPED (every mode; never with MAPPED): wave b reads its query's bitmap grp.masks + grp.group[b] * grp.ld where the others read `valid`;
// a query whose group id lies outside [0, G) is offered no row.
template <class T, bool MAPPED = false, bool GROUPED = false>
__global__ __launch_bounds__(256) void flat_exact_kernel(int metric, const float *__restrict__ q, int B, int D, const T *__restrict__ x,
                                                        int64_t N, const int32_t *__restrict__ list, const int32_t *__restrict__ cnt, int cap,
                                                        int64_t S, int64_t stride, const uint32_t *__restrict__ valid, int k, int do_sqrt,
                                                        int final_list, int only_overflowed, float *__restrict__ thr_out,
                                                        float *__restrict__ out_d, int64_t *__restrict__ out_i, int32_t *__restrict__ ovf,
                                                        uint32_t *__restrict__ ovf_total, float scale = 1.f,
                                                        const int32_t *__restrict__ rows = nullptr, const FlatGroups grp = {}) {
    static_assert(!(MAPPED && GROUPED), "the grouped mode is over the table only");
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    int64_t n;
    if (list) {
        const int c = cnt[b];
        if (final_list) {
            const bool over = c > cap;
            if (lane == 0) {
                ovf[b] = over ? 1 : 0;
                if (over) atomicAdd(ovf_total, 1u);
            }
            if (over) return;  // (answered by the launch that follows, over all rows)
        }
        n = c < cap ? c : cap;
    } else {
        if (only_overflowed && !ovf[b]) return;
        n = S;
    }
    if constexpr (GROUPED) {
        valid = flat_group_mask(grp, b);
        if (!valid) n = 0;  // (no bitmap: no row -- NULL is "every row" to the chunk below)
    }
    const float *qr = q + (int64_t)b * D;
    const int32_t *lr = list ? list + (int64_t)b * cap : nullptr;
    WaveList L;
    L.reset();
    uint32_t th = kKeyInfHi, tl = kIdNone;
    for (int64_t c0 = 0; c0 < n; c0 += 64) {
        const int64_t ci = c0 + lane;
        int64_t row = -1;
        if (ci < n) {
            if constexpr (MAPPED) row = lr ? (int64_t)lr[ci] : (int64_t)rows[ci * stride];
            else row = lr ? (int64_t)lr[ci] : ci * stride;
        }
        flat_exact_chunk(metric, qr, D, x, N, valid, row, n - c0 < 64 ? (int)(n - c0) : 64, k - 1, lane, L, th, tl, scale);
    }
    flat_exact_finish(L, b, k, lane, do_sqrt, thr_out, out_d, out_i);
}

// ---- cells over float vectors ---------------------------------------------------------------------------------
// The live rows grouped by cell: perm i32 [n_perm] holds their offsets, cell c = perm[cell_rows[c][0] .. cell_rows[c][1]), ascending
// inside a cell.  A query's row set is the ranges of its P probed cells; "stride s" means the entries 0, s, 2 s, ... of EACH range.
// The lists, the norms, the bitmap and the exact chain above all speak offsets, so nothing else changes.
__device__ __forceinline__ void ivf_flat_cell_range(int32_t cell, int C, const int64_t *__restrict__ cell_rows, int64_t n_perm, int64_t &begin,
                                                    int64_t &end) {
    const int c = (unsigned)cell < (unsigned)C ? cell : 0;  // (an id out of range: cell 0, as ivf_plan_kernel reads it)
    begin = cell_rows[2 * c], end = cell_rows[2 * c + 1];
    if (begin < 0) begin = 0;
    if (end > n_perm) end = n_perm;
}

// flat_exact_kernel's `list == NULL` mode over the probed cells: exact sums of every stride-th entry of each of the query's P cells
// (the first sample; all probed rows where they are few; the route of an overflowed query).
__global__ __launch_bounds__(256) void ivf_flat_exact_kernel(int metric, const float *__restrict__ q, int B, int D, const float *__restrict__ x,
                                                            int64_t N, const int32_t *__restrict__ cells, int P, int C,
                                                            const int64_t *__restrict__ cell_rows, const int32_t *__restrict__ perm,
                                                            int64_t n_perm, int64_t stride, const uint32_t *__restrict__ valid, int k,
                                                            int do_sqrt, int only_overflowed, float *__restrict__ thr_out,
                                                            float *__restrict__ out_d, int64_t *__restrict__ out_i,
                                                            const int32_t *__restrict__ ovf) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    if (only_overflowed && !ovf[b]) return;
    const float *qr = q + (int64_t)b * D;
    WaveList L;
    L.reset();
    uint32_t th = kKeyInfHi, tl = kIdNone;
    for (int p = 0; p < P; ++p) {
        int64_t begin, end;
        ivf_flat_cell_range(cells[(int64_t)b * P + p], C, cell_rows, n_perm, begin, end);
        const int64_t n = (end - begin + stride - 1) / stride;
        for (int64_t c0 = 0; c0 < n; c0 += 64) {
            const int64_t ci = c0 + lane;
            const int64_t row = ci < n ? (int64_t)perm[begin + ci * stride] : -1;
            flat_exact_chunk(metric, qr, D, x, N, valid, row, n - c0 < 64 ? (int)(n - c0) : 64, k - 1, lane, L, th, tl);
        }
    }
    flat_exact_finish(L, b, k, lane, do_sqrt, thr_out, out_d, out_i);
}

// flat_filter_kernel over (plan tile t, row tile of t's cell): tile t = the 128 slots vmap[128 t ..] of queries that probe ONE cell
// (annlite_ivf_plan; -1: a padding slot), whose range of perm is tile_rows[t] (begin -1: an unused tile).  blockIdx.x = the row tile
// inside the cell at this stride, blockIdx.y (+ gridDim.y, ...) = t.  A operand: rows gathered through perm, B operand: queries
// gathered through vmap; the contraction is flat_filter_kernel's (flat_f32_stage, flat_f32_contract), the score, the comparison and
// the append are flat_tile_epilogue's as in every filter, and what is appended is
// the row's OFFSET.  A query sits in at most one slot per cell and a row in one cell, so a list takes no pair twice.

// Plan tile t's range of perm, from `begin`, and S, its stage rows at this stride.  False: an unused tile.
__device__ __forceinline__ bool ivf_flat_tile_range(const int64_t *__restrict__ tile_rows, int t, int64_t n_perm, int64_t stride, int64_t &begin,
                                                    int64_t &S) {
    begin = tile_rows[2 * (int64_t)t];
    int64_t end = tile_rows[2 * (int64_t)t + 1];
    if (begin < 0) return false;
    if (end > n_perm) end = n_perm;
    S = (end - begin + stride - 1) / stride;
    return true;
}

// The row tile and the query slots of a cell kernel, by its 2 kFlatTile threads: rws[i] = offset of stage row r0 + i of the tile's range,
// -1: none (past the cell's end, not valid); nxs[i] = its norm; qss[i] = query of the tile's slot i, -1: padding.
__device__ __forceinline__ void ivf_flat_tile_rows(int tid, int t, int64_t r0, int64_t S, int64_t begin, int64_t stride,
                                                   const int32_t *__restrict__ perm, int64_t N, const uint32_t *__restrict__ valid,
                                                   const float *__restrict__ norms, const int32_t *__restrict__ vmap, int B, int *rws, float *nxs,
                                                   int *qss) {
    if (tid < kFlatTile) {
        const int64_t r = r0 + tid;
        int64_t row = r < S ? (int64_t)perm[begin + r * stride] : -1;
        if (row >= N) row = -1;
        if (row >= 0 && valid && !((valid[row >> 5] >> (row & 31)) & 1u)) row = -1;
        rws[tid] = (int)row;
        nxs[tid] = row >= 0 ? norms[row] : 0.f;
    } else {
        const int qi = vmap[(int64_t)t * kFlatTile + tid - kFlatTile];
        qss[tid - kFlatTile] = (unsigned)qi < (unsigned)B ? qi : -1;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void ivf_flat_filter_kernel(int metric, const float *__restrict__ q, int B, int D, const float *__restrict__ x,
                                                             const float *__restrict__ norms, int64_t N, const int32_t *__restrict__ perm,
                                                             int64_t n_perm, const int64_t *__restrict__ tile_rows,
                                                             const int32_t *__restrict__ vmap, int n_tiles, int64_t stride,
                                                             const uint32_t *__restrict__ valid, const float *__restrict__ qnorm,
                                                             const float *__restrict__ thr, float c_rel, float c_abs,
                                                             int32_t *__restrict__ cand, int32_t *__restrict__ cnt, int cap) {
    __shared__ float As[kFlatTile * kFlatLd];
    __shared__ float Bs[kFlatTile * kFlatLd];
    __shared__ float nxs[kFlatTile];
    __shared__ int rws[kFlatTile];
    __shared__ int qss[kFlatTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kFlatTile;
    const int wr = (wave >> 1) * 64, wq = (wave & 1) * 64;
    const int l31 = lane & 31, lh = lane >> 5;
    const auto row_of = [&](int rl) { return FlatRow{rws[rl] >= 0, rws[rl], false, 0}; };
    for (int t = blockIdx.y; t < n_tiles; t += gridDim.y) {
        int64_t begin, S;
        if (!ivf_flat_tile_range(tile_rows, t, n_perm, stride, begin, S) || r0 >= S) continue;  // (the workgroup's: no barrier is left behind)
        __syncthreads();  // the previous tile's epilogue has read rws / nxs / qss
        ivf_flat_tile_rows(tid, t, r0, S, begin, stride, perm, N, valid, norms, vmap, B, rws, nxs, qss);
        FlatAcc acc;
        acc.zero();
        for (int k0 = 0; k0 < D; k0 += kFlatDepth) {
            __syncthreads();  // the previous stage is consumed (first pass: the tile's rows and queries are written)
            flat_f32_stage<VEC>(
                tid, k0, D, x, q, As, Bs, [&](int r) { return FlatSlot{rws[r] >= 0, (int64_t)rws[r] * D}; },
                [&](int r) { return FlatSlot{qss[r] >= 0, (int64_t)qss[r] * D}; });
            __syncthreads();
            flat_f32_contract(As, Bs, wr, wq, l31, lh, acc);
        }
#pragma unroll
        for (int qj = 0; qj < 2; ++qj) {
            const int qi = qss[wq + qj * 32 + l31];
            if (qi < 0) continue;
            const FlatQuery Q = flat_query(qi, qnorm[qi], thr, 0.f, cand, cnt, cap, nullptr, 0);
#pragma unroll
            for (int ri = 0; ri < 2; ++ri)
                flat_tile_epilogue<false, false>(metric, c_rel, c_abs, cap, Q, nxs, wr + ri * 32, lh, [&](int reg) { return acc.tile(ri, qj)[reg]; }, row_of);
        }
    }
}

// ---- the split filter over cell tiles ("split filter over cell tiles") -------------------------------------------
// flat_split_filter_kernel's contraction on ivf_flat_filter_kernel's tiles, with a centre PER TILE: the centroid of the tile's cell
// (centres f32 [C][D]; NULL: no centring).  Every row of a tile belongs to that cell and every query slot of the tile probes it, so
// both operands of every pair are centred on the same point -- all section 3.6's claim asks for.
//
// The queries, once per call, a wave per (query b, probe p) pair: c = fl(q_b - centres[cells[b][p]]) split into the two bf16 planes of
// the pair's PLAN SLOT v = slot_of[b P + p] (qh / ql bf16 [n_slots][Dp], Dp = D rounded up to 16, the padding zero): a filter tile reads
// the planes of its 128 slots back to back, no gather.  qnorm[v] = |c|^2 in flat_split_queries_kernel's chain; pair_norms (may be
// NULL) f32 [B][P] receives the same number by pair.  A cell id outside [0, C) reads cell 0, as the plan does.
__global__ __launch_bounds__(256) void ivf_flat_split_queries_kernel(const float *__restrict__ q, int n_pairs, int P, int D, int Dp,
                                                                    const int32_t *__restrict__ cells, int C,
                                                                    const float *__restrict__ centres, const int32_t *__restrict__ slot_of,
                                                                    int n_slots, __bf16 *__restrict__ qh, __bf16 *__restrict__ ql,
                                                                    float *__restrict__ qnorm, float *__restrict__ pair_norms) {
    const int lane = threadIdx.x & 63;
    const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= n_pairs) return;
    const int v = slot_of[pair];
    if ((unsigned)v >= (unsigned)n_slots) return;
    const float *qr = q + (int64_t)(pair / P) * D;
    const float *mu = nullptr;
    if (centres) {
        const int c = cells[pair];
        mu = centres + (int64_t)((unsigned)c < (unsigned)C ? c : 0) * D;
    }
    float s = 0.f;
    for (int j = lane; j < Dp; j += 64) {
        float c = 0.f;
        if (j < D) {
            c = mu ? qr[j] - mu[j] : qr[j];
            s = __builtin_fmaf(c, c, s);
        }
        __bf16 h, l;
        split_bf16(c, h, l);
        qh[(int64_t)v * Dp + j] = h;
        ql[(int64_t)v * Dp + j] = l;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
        qnorm[v] = s;
        if (pair_norms) pair_norms[pair] = s;
    }
}

// ivf_flat_filter_kernel's grid, tile walk and rws / qss; flat_split_filter_kernel's LDS planes and MFMAs; flat_tile_epilogue.  The rows are
// gathered through perm, centred on the tile's centroid -- the cell of the range's first row, cell_of[perm[begin]] -- and split while
// they are staged; a thread stages the same four (VEC) / one coordinates of every row it handles, so it loads its piece of the centroid
// once per stage.  norms: the column of |fl(x - centre of x's cell)|^2 (annlite_ivf_flat_centred_norms; |x|^2 without centres);
// qnorm: by slot.  scores != NULL (tests, measurements): v of every evaluated (query, live row) pair goes to scores f32 [B][N] by
// (query, row offset); the others keep what the caller put there.
template <bool VEC>
__global__ __launch_bounds__(256) void ivf_flat_split_filter_kernel(int metric, const __bf16 *__restrict__ qh, const __bf16 *__restrict__ ql,
                                                                   int B, int D, int Dp, const float *__restrict__ x,
                                                                   const float *__restrict__ centres, int C,
                                                                   const int32_t *__restrict__ cell_of, const float *__restrict__ norms,
                                                                   int64_t N, const int32_t *__restrict__ perm, int64_t n_perm,
                                                                   const int64_t *__restrict__ tile_rows, const int32_t *__restrict__ vmap,
                                                                   int n_tiles, int64_t stride, const uint32_t *__restrict__ valid,
                                                                   const float *__restrict__ qnorm, const float *__restrict__ thr,
                                                                   float c_rel, float c_abs, int32_t *__restrict__ cand,
                                                                   int32_t *__restrict__ cnt, int cap, float *__restrict__ scores) {
    __shared__ __attribute__((aligned(16))) __bf16 Ah[kFlatTile * kSplitLd];
    __shared__ __attribute__((aligned(16))) __bf16 Al[kFlatTile * kSplitLd];
    __shared__ __attribute__((aligned(16))) __bf16 Bh[kFlatTile * kSplitLd];
    __shared__ __attribute__((aligned(16))) __bf16 Bl[kFlatTile * kSplitLd];
    __shared__ float nxs[kFlatTile];
    __shared__ int rws[kFlatTile];
    __shared__ int qss[kFlatTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kFlatTile;
    const int wr = (wave >> 1) * 64, wq = (wave & 1) * 64;
    const int l31 = lane & 31, lh = lane >> 5;
    __bf16 *const bp[2] = {Bh, Bl};
    const auto row_of = [&](int rl) { return FlatRow{rws[rl] >= 0, rws[rl], rws[rl] >= 0, (int64_t)rws[rl]}; };
    for (int t = blockIdx.y; t < n_tiles; t += gridDim.y) {
        int64_t begin, S;
        if (!ivf_flat_tile_range(tile_rows, t, n_perm, stride, begin, S) || r0 >= S) continue;  // (the workgroup's: no barrier is left behind)
        __syncthreads();  // the previous tile's epilogue has read rws / nxs / qss
        ivf_flat_tile_rows(tid, t, r0, S, begin, stride, perm, N, valid, norms, vmap, B, rws, nxs, qss);
        const float *mu = nullptr;  // the tile's centroid (the range is not empty: r0 < S)
        if (centres) {
            const int64_t first = perm[begin];
            const int c = (first >= 0 && first < N) ? cell_of[first] : 0;
            mu = centres + (int64_t)((unsigned)c < (unsigned)C ? c : 0) * D;
        }
        const __bf16 *const tp[2] = {qh + (int64_t)t * kFlatTile * Dp, ql + (int64_t)t * kFlatTile * Dp};  // the planes of the tile's slots
        FlatAcc acc;
        acc.zero();
        for (int k0 = 0; k0 < D; k0 += kSplitDepth) {
            __syncthreads();  // the previous stage is consumed (first pass: the tile's rows and queries are written)
            // rows: f32 gathered from HBM, centred, split, two planes
            if constexpr (VEC) {
                const int c = (tid % (kSplitDepth / 4)) * 4;
                f32x4 mv = {0.f, 0.f, 0.f, 0.f};
                if (mu && k0 + c < D) mv = *(const f32x4 *)(mu + k0 + c);
#pragma unroll
                for (int i = 0; i < kSplitDepth / 8; ++i) {
                    const int r = (tid + i * 256) / (kSplitDepth / 4);  // slots of 4 floats
                    f32x4 cv = {0.f, 0.f, 0.f, 0.f};
                    const int rr = rws[r];
                    if (rr >= 0 && k0 + c < D) cv = *(const f32x4 *)(x + (int64_t)rr * D + k0 + c) - mv;
                    bf16x4 h4, l4;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        __bf16 h, l;
                        split_bf16(cv[u], h, l);
                        h4[u] = h, l4[u] = l;
                    }
                    *(bf16x4 *)(Ah + r * kSplitLd + c) = h4;
                    *(bf16x4 *)(Al + r * kSplitLd + c) = l4;
                }
            } else {
                const int c = tid % kSplitDepth;
                const float mv = (mu && k0 + c < D) ? mu[k0 + c] : 0.f;
#pragma unroll 4
                for (int i = 0; i < kSplitDepth / 2; ++i) {
                    const int r = (tid + i * 256) / kSplitDepth;  // single floats
                    const int rr = rws[r];
                    float cv = 0.f;
                    if (rr >= 0 && k0 + c < D) cv = x[(int64_t)rr * D + k0 + c] - mv;
                    __bf16 h, l;
                    split_bf16(cv, h, l);
                    Ah[r * kSplitLd + c] = h;
                    Al[r * kSplitLd + c] = l;
                }
            }
            // queries: the planes of the tile's slots, back to back (Dp is a multiple of 8 coordinates)
            flat_stage_planes<bf16x8>(tid, k0, Dp, tp, bp, [&](int r) { return FlatSlot{qss[r] >= 0, (int64_t)r * Dp}; });
            __syncthreads();
            FLAT_BF16X3_CONTRACT(Ah, Al, Bh, Bl, k0, D, wr, wq, l31, lh, acc);
        }
        // (the norms are the centred ones: of the row, and of the slot's pair)
#pragma unroll
        for (int qj = 0; qj < 2; ++qj) {
            const int sl = wq + qj * 32 + l31;
            const int qi = qss[sl];
            if (qi < 0) continue;
            const FlatQuery Q = flat_query(qi, qnorm[(int64_t)t * kFlatTile + sl], thr, 0.f, cand, cnt, cap, scores, N);
#pragma unroll
            for (int ri = 0; ri < 2; ++ri)
                flat_tile_epilogue<false, false>(metric, c_rel, c_abs, cap, Q, nxs, wr + ri * 32, lh, [&](int reg) { return acc.tile(ri, qj)[reg]; }, row_of);
        }
    }
}

// ---- workspace of annlite_flat_search_topk -------------------------------------------------------------------------------------------
struct FlatWs {
    uint32_t *ovf_total;  // queries of the last call whose final list overflowed
    float *thr, *qnorm;
    int32_t *cnt, *ovf, *cand;
    size_t bytes;
};
// Carving a workspace: every piece starts on a 256-byte boundary; `o` is what has been handed out.
struct WsBump {
    char *p;
    size_t o;
    template <class T>
    T *take(size_t bytes) {
        T *r = (T *)(p + o);
        o += (bytes + 255) & ~(size_t)255;
        return r;
    }
};
static FlatWs flat_carve(void *ws, int64_t B) {
    WsBump b{(char *)ws, 0};
    FlatWs w;
    w.ovf_total = b.take<uint32_t>(256);
    w.thr = b.take<float>((size_t)B * 4);
    w.qnorm = b.take<float>((size_t)B * 4);
    w.cnt = b.take<int32_t>((size_t)B * 4);
    w.ovf = b.take<int32_t>((size_t)B * 4);
    w.cand = b.take<int32_t>((size_t)B * kFlatCap * 4);
    w.bytes = b.o;
    return w;
}
static int flat_check_workspace(size_t have, size_t need) {
    if (have >= need) return ANNLITE_OK;
    set_error("workspace too small: %zu < %zu bytes", have, need);
    return ANNLITE_ERR_WORKSPACE;
}

// The argument checks every filter entry (kFlatStage: one stage, arg = its stride) and every search entry (kFlatSearch: arg = k)
// starts with.  max_dim: INT32_MAX for the f32 contraction's entries, kSplitMaxDim for the others, whose message names it.
enum FlatEntry { kFlatStage, kFlatSearch };
static int flat_check_shape(FlatEntry what, int metric, int64_t B, int64_t D, int64_t N, int64_t arg, int64_t max_dim) {
    ANNLITE_REQUIRE(metric >= 1 && metric <= 3, "bad metric %d", metric);
    const bool search = what == kFlatSearch;
    const bool ok = B >= 0 && D >= 1 && N >= 0 && arg >= 1 && (!search || arg <= 64) && N <= INT32_MAX && B <= INT32_MAX && D <= max_dim;
    if (max_dim == INT32_MAX) ANNLITE_REQUIRE(ok, search ? "bad shape (1 <= k <= 64)" : "bad shape");
    else ANNLITE_REQUIRE(ok, search ? "bad shape (1 <= k <= 64, D <= %lld)" : "bad shape (D <= %lld)", (long long)max_dim);
    return ANNLITE_OK;
}

// The grid of a table filter over S stage rows and B queries: a workgroup per row tile, and the query tiles spread over y while the
// row tiles alone would leave CUs idle.
struct FlatGrid {
    dim3 grid;
    int n_qt;
};
static FlatGrid flat_filter_grid(int64_t S, int64_t B) {
    const int64_t n_rt = (S + kFlatTile - 1) / kFlatTile;
    const int n_qt = (int)((B + kFlatTile - 1) / kFlatTile);
    int64_t ny = (4 * (int64_t)device_cu_count() + n_rt - 1) / n_rt;  // few row tiles: spread the query tiles too
    ny = ny < 1 ? 1 : ny > n_qt ? n_qt : ny;
    return {dim3((unsigned)n_rt, (unsigned)ny), n_qt};
}
// ... and of a cell filter: the row tiles of the largest cell at this stride x the plan's tiles (the kernel walks y).  Nothing to do: x or y 0.
static dim3 ivf_flat_filter_grid(int64_t max_cell_rows, int64_t stride, int64_t n_tiles) {
    const int64_t n_rt = ((max_cell_rows + stride - 1) / stride + kFlatTile - 1) / kFlatTile;
    return dim3((unsigned)(n_rt > 0 ? n_rt : 0), (unsigned)(n_tiles < 0 ? 0 : n_tiles < 65535 ? n_tiles : 65535));
}

// kernel<VEC> over the same arguments, VEC chosen at run time.
#define FLAT_LAUNCH_VEC(vec, kernel, grid, block, st, ...)                                         \
    do {                                                                                           \
        if (vec) hipLaunchKernelGGL(kernel<true>, grid, block, 0, st, __VA_ARGS__);                \
        else hipLaunchKernelGGL(kernel<false>, grid, block, 0, st, __VA_ARGS__);                   \
    } while (0)
// kernel<VEC> over the table, or rows_kernel<VEC> over a list of selected rows -- the same arguments and, behind them, the list and N.
#define FLAT_LAUNCH_VEC_MAPPED(vec, kernel, rows_kernel, rows, N, grid, block, st, ...)            \
    do {                                                                                           \
        if (rows) FLAT_LAUNCH_VEC(vec, rows_kernel, grid, block, st, __VA_ARGS__, rows, N);        \
        else FLAT_LAUNCH_VEC(vec, kernel, grid, block, st, __VA_ARGS__);                           \
    } while (0)
// ... or grouped_kernel<VEC> over the table with a bitmap per query (grp.masks != NULL) -- the same arguments and, behind them, grp.
#define FLAT_LAUNCH_VEC_MODE(vec, kernel, rows_kernel, grouped_kernel, rows, N, grp, grid, block, st, ...)             \
    do {                                                                                                               \
        if ((grp).masks) FLAT_LAUNCH_VEC(vec, grouped_kernel, grid, block, st, __VA_ARGS__, grp);                      \
        else FLAT_LAUNCH_VEC_MAPPED(vec, kernel, rows_kernel, rows, N, grid, block, st, __VA_ARGS__);                  \
    } while (0)

// The slack's constants: u = 2^-24, and n_l, the terms of a lane's chain in the norms.
constexpr double kFlatU = 5.9604644775390625e-08;
static double flat_lane_terms(int64_t D) { return (double)((D + 63) / 64); }

// The f32 filter's two.
static void flat_slack(int metric, int64_t D, float *c_rel, float *c_abs) {
    const double u = kFlatU, nl = flat_lane_terms(D);
    *c_rel = (float)(1.05 * u * ((double)D + 3.0 * nl + 40.0));
    *c_abs = metric == ANNLITE_METRIC_EUCLIDEAN ? 1e-30f : (float)(8.0 * u);
}

static int flat_launch_filter(int metric, const float *q, int64_t B, int64_t D, const float *x, const float *norms, int64_t S, int64_t stride,
                              const uint32_t *valid, const float *qnorm, const float *thr, int32_t *cand, int32_t *cnt, hipStream_t st,
                              const int32_t *rows = nullptr, int64_t N = 0, const FlatGroups grp = {}) {
    float c_rel, c_abs;
    flat_slack(metric, D, &c_rel, &c_abs);
    const FlatGrid g = flat_filter_grid(S, B);
    const bool vec = D % 4 == 0 && ((uintptr_t)q % 16 == 0) && ((uintptr_t)x % 16 == 0);
    FLAT_LAUNCH_VEC_MODE(vec, flat_filter_kernel, flat_rows_filter_kernel, flat_grouped_filter_kernel, rows, N, grp, g.grid, dim3(256), st, metric, q,
                         (int)B, (int)D, x, norms, S, stride, valid, qnorm, thr, c_rel, c_abs, cand, cnt, kFlatCap, g.n_qt);
    return launch_status("flat_filter_kernel");
}

// ---- the split filter's share of a workspace: the query planes, behind the FlatWs of the same B (so that the overflow counter and the
// list counters sit where annlite_flat_overflow_count / annlite_flat_list_counts read them) ----
struct FlatSplitWs {
    FlatWs f;
    int64_t Dp;  // D rounded up to the MFMA's K step
    __bf16 *qh, *ql;
    size_t bytes;
};
static FlatSplitWs flat_split_carve(void *ws, int64_t B, int64_t D) {
    FlatSplitWs w;
    w.f = flat_carve(ws, B);
    w.Dp = (D + 15) / 16 * 16;
    WsBump b{(char *)ws, w.f.bytes};
    w.qh = b.take<__bf16>((size_t)B * w.Dp * 2);
    w.ql = b.take<__bf16>((size_t)B * w.Dp * 2);
    w.bytes = b.o;
    return w;
}

// The split filter's two constants ("split filter").  u = 2^-24, Dp = 16 ceil(D / 16).
static void flat_split_slack(int metric, int64_t D, float *c_rel, float *c_abs) {
    const double u = kFlatU, nl = flat_lane_terms(D), dp = (double)((D + 15) / 16 * 16);
    *c_rel = (float)(1.05 * u * (6.6 * dp + 780.0 + 3.0 * nl + 44.0));
    *c_abs = metric == ANNLITE_METRIC_EUCLIDEAN ? 2e-30f : (float)(9.0 * u);
}

// Per call: centre and split the queries into the workspace planes, |fl(q - mu)|^2 into w.f.qnorm.
static int flat_split_prepare(const float *q, int64_t B, int64_t D, const float *mu, const FlatSplitWs &w, hipStream_t st) {
    hipLaunchKernelGGL(flat_split_queries_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, q, (int)B, (int)D, (int)w.Dp, mu, w.qh, w.ql,
                       w.f.qnorm);
    return launch_status("flat_split_queries_kernel");
}

static int flat_split_launch_filter(int metric, int64_t B, int64_t D, const float *x, const float *mu, const float *norms, int64_t S,
                                    int64_t stride, const uint32_t *valid, const FlatSplitWs &w, const float *thr, int32_t *cand,
                                    int32_t *cnt, float *scores, hipStream_t st, const int32_t *rows = nullptr, int64_t N = 0,
                                    const FlatGroups grp = {}) {
    float c_rel, c_abs;
    flat_split_slack(metric, D, &c_rel, &c_abs);
    const FlatGrid g = flat_filter_grid(S, B);
    const bool vec = D % 4 == 0 && ((uintptr_t)x % 16 == 0) && ((uintptr_t)mu % 16 == 0);
    FLAT_LAUNCH_VEC_MODE(vec, flat_split_filter_kernel, flat_rows_split_filter_kernel, flat_grouped_split_filter_kernel, rows, N, grp, g.grid,
                         dim3(256), st, metric, w.qh, w.ql, (int)B, (int)D, (int)w.Dp, x, mu, norms, S, stride, valid, w.f.qnorm, thr, c_rel, c_abs,
                         cand, cnt, kFlatCap, g.n_qt, scores);
    return launch_status("flat_split_filter_kernel");
}

// ---- the f16 filter's share of a workspace: the query planes, the scales and the flush terms, behind the FlatWs of the same B ----
struct FlatF16Ws {
    FlatWs f;
    int64_t Dp;  // D rounded up to the MFMA's K step
    _Float16 *qh, *ql;
    float *qscale, *qflush;
    size_t bytes;
};
static FlatF16Ws flat_f16_carve(void *ws, int64_t B, int64_t D) {
    FlatF16Ws w;
    w.f = flat_carve(ws, B);
    w.Dp = (D + 15) / 16 * 16;
    WsBump b{(char *)ws, w.f.bytes};
    w.qh = b.take<_Float16>((size_t)B * w.Dp * 2);
    w.ql = b.take<_Float16>((size_t)B * w.Dp * 2);
    w.qscale = b.take<float>((size_t)B * 4);
    w.qflush = b.take<float>((size_t)B * 4);
    w.bytes = b.o;
    return w;
}

// The f16 filter's two constants ("f16 rows"); the third, absolute term is per query (flat_f16_queries_kernel).
static void flat_f16_slack(int metric, int64_t D, float *c_rel, float *c_abs) {
    const double u = kFlatU, nl = flat_lane_terms(D), dp = (double)((D + 15) / 16 * 16);
    *c_rel = (float)(1.05 * u * (4.4 * dp + 16.0 + 3.0 * nl + 44.0));
    *c_abs = metric == ANNLITE_METRIC_EUCLIDEAN ? 2e-30f : (float)(9.0 * u);
}

static int flat_f16_prepare(const float *q, int64_t B, int64_t D, const FlatF16Ws &w, hipStream_t st) {
    hipLaunchKernelGGL(flat_f16_queries_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, q, (int)B, (int)D, (int)w.Dp, w.qh, w.ql,
                       w.f.qnorm, w.qscale, w.qflush);
    return launch_status("flat_f16_queries_kernel");
}

static int flat_f16_launch_filter(int metric, int64_t B, int64_t D, const _Float16 *x, const float *norms, int64_t S, int64_t stride,
                                  const uint32_t *valid, const FlatF16Ws &w, const float *thr, int32_t *cand, int32_t *cnt, float *scores,
                                  hipStream_t st, const int32_t *rows = nullptr, int64_t N = 0, const FlatGroups grp = {}) {
    float c_rel, c_abs;
    flat_f16_slack(metric, D, &c_rel, &c_abs);
    const FlatGrid g = flat_filter_grid(S, B);
    const bool vec = D % 8 == 0 && ((uintptr_t)x % 16 == 0);
    FLAT_LAUNCH_VEC_MODE(vec, flat_f16_filter_kernel, flat_rows_f16_filter_kernel, flat_grouped_f16_filter_kernel, rows, N, grp, g.grid, dim3(256),
                         st, metric, w.qh, w.ql, (int)B, (int)D, (int)w.Dp, x, norms, S, stride, valid, w.f.qnorm, w.qscale, w.qflush, thr, c_rel,
                         c_abs, cand, cnt, kFlatCap, g.n_qt, scores);
    return launch_status("flat_f16_filter_kernel");
}

// ---- the int8 filter's share of a workspace: the three digit planes, the scales and the per-query slack terms, behind the FlatWs of the
// same B ----
struct FlatI8Ws {
    FlatWs f;
    int64_t Dp;  // D rounded up to the MFMA's K step
    int8_t *p0, *p1, *p2;
    float *qscale, *qslack;
    size_t bytes;
};
static FlatI8Ws flat_i8_carve(void *ws, int64_t B, int64_t D) {
    FlatI8Ws w;
    w.f = flat_carve(ws, B);
    w.Dp = (D + 31) / 32 * 32;
    WsBump b{(char *)ws, w.f.bytes};
    w.p0 = b.take<int8_t>((size_t)B * w.Dp);
    w.p1 = b.take<int8_t>((size_t)B * w.Dp);
    w.p2 = b.take<int8_t>((size_t)B * w.Dp);
    w.qscale = b.take<float>((size_t)B * 4);
    w.qslack = b.take<float>((size_t)B * 4);
    w.bytes = b.o;
    return w;
}

// The int8 filter's two constants ("int8 rows"); the third term is per query (flat_i8_queries_kernel).  The
// contraction is exact, so D enters through the norms' lane chains alone.
static void flat_i8_slack(int metric, int64_t D, float *c_rel, float *c_abs) {
    const double u = kFlatU, nl = flat_lane_terms(D);
    *c_rel = (float)(1.05 * u * (3.0 * nl + 48.0));
    *c_abs = metric == ANNLITE_METRIC_EUCLIDEAN ? 3e-30f : (float)(9.0 * u);
}

static int flat_i8_prepare(const float *q, int64_t B, int64_t D, float scale, const FlatI8Ws &w, hipStream_t st) {
    hipLaunchKernelGGL(flat_i8_queries_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, q, (int)B, (int)D, (int)w.Dp,
                       i8_scale_log2(scale), w.p0, w.p1, w.p2, w.f.qnorm, w.qscale, w.qslack);
    return launch_status("flat_i8_queries_kernel");
}

static int flat_i8_launch_filter(int metric, int64_t B, int64_t D, const int8_t *x, const float *norms, int64_t S, int64_t stride,
                                 const uint32_t *valid, const FlatI8Ws &w, const float *thr, int32_t *cand, int32_t *cnt, float *scores,
                                 hipStream_t st, const int32_t *rows = nullptr, int64_t N = 0, const FlatGroups grp = {}) {
    float c_rel, c_abs;
    flat_i8_slack(metric, D, &c_rel, &c_abs);
    const FlatGrid g = flat_filter_grid(S, B);
    const bool vec = D % 16 == 0 && ((uintptr_t)x % 16 == 0);
    FLAT_LAUNCH_VEC_MODE(vec, flat_i8_filter_kernel, flat_rows_i8_filter_kernel, flat_grouped_i8_filter_kernel, rows, N, grp, g.grid,
                         dim3(kI8Threads), st, metric, w.p0, w.p1, w.p2, (int)B, (int)D, (int)w.Dp, x, norms, S, stride, valid, w.f.qnorm, w.qscale,
                         w.qslack, thr, c_rel, c_abs, cand, cnt, kFlatCap, g.n_qt, scores);
    return launch_status("flat_i8_filter_kernel");
}

// ---- one call's operands, and one description per filter ("the host routine") -----------------------------------
// The row set of a call: the whole table (no list, no groups), a list of selected rows (no bitmap: a row in the list is selected), or
// the table with a bitmap per query (groups, behind the live bitmap).
enum FlatRowSet { kFlatTable, kFlatRows, kFlatGrouped };
struct FlatCall {
    FlatRowSet set;
    int metric;
    const float *q;
    int64_t B, D;
    const void *x;    // [N][D] of the filter's row type
    float row_scale;  // what one code step of an int8 row stands for (the float row types do not read it)
    const float *norms, *centre;
    int64_t N;
    const uint32_t *valid;
    const int32_t *rows;  // kFlatRows: n_sel ascending offsets below N
    int64_t n_sel;
    FlatGroups grp;  // kFlatGrouped
    hipStream_t st;
    int64_t set_rows() const { return set == kFlatRows ? n_sel : N; }
    bool set_given() const { return set == kFlatRows ? rows != nullptr : set == kFlatGrouped ? grp.masks && grp.group : true; }
};

// What a filter is to the host: its row type, its largest D, whether it takes a centre / reads an int8 scale / writes scores, its
// workspace (base(): the FlatWs at its head), prepare() -- what the filter needs from the queries, once per call -- and launch(), one
// filter stage over every stride-th of the set's rows (S of them) into cand / cnt against the bounds thr.  A new filter is one such
// struct and one line in flat_with_filter.
struct FlatF32 {
    using Row = float;
    using Ws = FlatWs;
    static constexpr int64_t kMaxDim = INT32_MAX;
    static constexpr bool kCentre = false, kScale = false, kScores = false;
    static Ws carve(void *ws, int64_t B, int64_t) { return flat_carve(ws, B); }
    static const FlatWs &base(const Ws &w) { return w; }
    static int prepare(const FlatCall &c, const Ws &w) { return annlite_flat_row_norms(c.q, c.B, c.D, nullptr, c.B, 0, w.qnorm, (void *)c.st); }
    static int launch(const FlatCall &c, const Ws &w, int64_t S, int64_t stride, const float *thr, int32_t *cand, int32_t *cnt, float *) {
        return flat_launch_filter(c.metric, c.q, c.B, c.D, (const Row *)c.x, c.norms, S, stride, c.valid, w.qnorm, thr, cand, cnt, c.st, c.rows, c.N,
                                  c.grp);
    }
};
struct FlatBf16x3 {
    using Row = float;
    using Ws = FlatSplitWs;
    static constexpr int64_t kMaxDim = kSplitMaxDim;
    static constexpr bool kCentre = true, kScale = false, kScores = true;
    static Ws carve(void *ws, int64_t B, int64_t D) { return flat_split_carve(ws, B, D); }
    static const FlatWs &base(const Ws &w) { return w.f; }
    static int prepare(const FlatCall &c, const Ws &w) { return flat_split_prepare(c.q, c.B, c.D, c.centre, w, c.st); }
    static int launch(const FlatCall &c, const Ws &w, int64_t S, int64_t stride, const float *thr, int32_t *cand, int32_t *cnt, float *scores) {
        return flat_split_launch_filter(c.metric, c.B, c.D, (const Row *)c.x, c.centre, c.norms, S, stride, c.valid, w, thr, cand, cnt, scores, c.st,
                                        c.rows, c.N, c.grp);
    }
};
struct FlatF16x2 {
    using Row = _Float16;
    using Ws = FlatF16Ws;
    static constexpr int64_t kMaxDim = kSplitMaxDim;
    static constexpr bool kCentre = false, kScale = false, kScores = true;
    static Ws carve(void *ws, int64_t B, int64_t D) { return flat_f16_carve(ws, B, D); }
    static const FlatWs &base(const Ws &w) { return w.f; }
    static int prepare(const FlatCall &c, const Ws &w) { return flat_f16_prepare(c.q, c.B, c.D, w, c.st); }
    static int launch(const FlatCall &c, const Ws &w, int64_t S, int64_t stride, const float *thr, int32_t *cand, int32_t *cnt, float *scores) {
        return flat_f16_launch_filter(c.metric, c.B, c.D, (const Row *)c.x, c.norms, S, stride, c.valid, w, thr, cand, cnt, scores, c.st, c.rows, c.N,
                                      c.grp);
    }
};
struct FlatI8x3 {
    using Row = int8_t;
    using Ws = FlatI8Ws;
    static constexpr int64_t kMaxDim = kSplitMaxDim;
    static constexpr bool kCentre = false, kScale = true, kScores = true;
    static Ws carve(void *ws, int64_t B, int64_t D) { return flat_i8_carve(ws, B, D); }
    static const FlatWs &base(const Ws &w) { return w.f; }
    static int prepare(const FlatCall &c, const Ws &w) { return flat_i8_prepare(c.q, c.B, c.D, c.row_scale, w, c.st); }
    static int launch(const FlatCall &c, const Ws &w, int64_t S, int64_t stride, const float *thr, int32_t *cand, int32_t *cnt, float *scores) {
        return flat_i8_launch_filter(c.metric, c.B, c.D, (const Row *)c.x, c.norms, S, stride, c.valid, w, thr, cand, cnt, scores, c.st, c.rows, c.N,
                                     c.grp);
    }
};

// The run-time filter code of the rows / grouped entries becomes the static type here, and nowhere else: fn(F{}) for the code's F.
template <class Fn>
static int flat_with_filter(int filter, Fn &&fn) {
    switch (filter) {
    case ANNLITE_FLAT_FILTER_F32: return fn(FlatF32{});
    case ANNLITE_FLAT_FILTER_BF16X3: return fn(FlatBf16x3{});
    case ANNLITE_FLAT_FILTER_F16X2: return fn(FlatF16x2{});
    case ANNLITE_FLAT_FILTER_I8X3: return fn(FlatI8x3{});
    default: set_error("bad filter %d", filter); return ANNLITE_ERR_INVALID;
    }
}

// What every search entry (kFlatSearch: arg = k) and every stage entry (kFlatStage: arg = its stride, scores = its scores output) asks
// of the shape, of the row set and of what only some filters take.  A new kind of row set adds its line here.
template <class F>
static int flat_check(FlatEntry what, const FlatCall &c, int64_t arg, const float *scores = nullptr) {
    if (int rc = flat_check_shape(what, c.metric, c.B, c.D, c.N, arg, F::kMaxDim)) return rc;
    if (c.set == kFlatRows) ANNLITE_REQUIRE(c.n_sel >= 0 && c.n_sel <= c.N, "bad n_sel=%lld (0 .. N=%lld)", (long long)c.n_sel, (long long)c.N);
    if (c.set == kFlatGrouped)
        ANNLITE_REQUIRE(c.grp.ld >= 0 && c.grp.ld * 32 >= c.N, "bad mask_ld=%lld (32 mask_ld >= N=%lld)", (long long)c.grp.ld, (long long)c.N);
    ANNLITE_REQUIRE(!c.centre || (F::kCentre && c.metric == ANNLITE_METRIC_EUCLIDEAN), "a centre is for the bf16x3 filter and EUCLIDEAN only");
    if (F::kScale) ANNLITE_REQUIRE_I8_SCALE(c.row_scale);
    ANNLITE_REQUIRE(!scores || F::kScores, "the f32 filter has no scores output");
    return ANNLITE_OK;
}
// The groups of a call.  G is checked here, before it narrows to the kernels' int.
static int flat_groups(const uint32_t *masks, int64_t mask_ld, int64_t G, const int32_t *group, FlatGroups *grp) {
    ANNLITE_REQUIRE(G >= 1 && G <= INT32_MAX, "bad G=%lld (>= 1)", (long long)G);
    *grp = FlatGroups{masks, mask_ld, (int)G, group};
    return ANNLITE_OK;
}

// ---- the stages of a search, the same for every filter F and every row set: the small-table shortcut, the first
// exact sample, filter stages (F::launch into w.cand / w.cnt against the bounds w.thr) over growing row sets, the re-rank of the lists
// and the route of an overflowed list.  fw: F's carved workspace. ----
template <class F>
static int flat_search_staged(F, const FlatCall &c, const typename F::Ws &fw, int64_t k, int flags, float *out_dist_dev, int64_t *out_id_dev) {
    // c.rows != NULL ("selected rows"): the search runs over the n_sel offsets of that list as it runs over a
    // table of n_sel rows -- M below --, every "row r" one indirection away (the MAPPED kernels); N stays the bound of an offset.
    // c.grp.masks != NULL ("a filter per query"; never with c.rows): every exact launch is the GROUPED kernel -- a
    // wave reads its query's bitmap where it reads c.valid otherwise -- and F::launch launches the GROUPED tiles.  The stages, the
    // lists and the overflow route are the same: a query whose bitmap keeps fewer than k sampled rows gets the bound +inf, overflows its
    // list and is answered over all rows under its own bitmap.
    using T = typename F::Row;
    const FlatWs &w = F::base(fw);
    const int64_t B = c.B, M = c.set_rows();
    hipStream_t st = c.st;
    const int do_sqrt = (flags & ANNLITE_FLAG_SQRT) ? 1 : 0;
    ANNLITE_HIP_TRY(hipMemsetAsync(w.ovf_total, 0, 256, st));
    // Every flat_exact_kernel launch.  list != NULL: exact sums over the lists, which hold offsets under either form -- the unmapped
    // kernel, also when a row list is given.  list == NULL: over every stride-th of S rows of the set, through the list when there is one.
    auto exact = [&](const int32_t *list, const int32_t *cnt, int64_t S, int64_t stride, int sqrt_out, int final_list, int only_overflowed,
                     float *thr_out) {
        const int32_t *rows = list ? nullptr : c.rows;
        const auto kernel = c.grp.masks ? &flat_exact_kernel<T, false, true> : rows ? &flat_exact_kernel<T, true> : &flat_exact_kernel<T>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, c.metric, c.q, (int)B, (int)c.D, (const T *)c.x, c.N, list, cnt,
                           kFlatCap, S, stride, c.valid, (int)k, sqrt_out, final_list, only_overflowed, thr_out, out_dist_dev, out_id_dev, w.ovf,
                           w.ovf_total, F::kScale ? c.row_scale : 1.f, rows, c.grp);
        return launch_status("flat_exact_kernel");
    };
    if (M <= kFlatSample)  // the first sample would be the whole set: exact sums over all its rows
        return exact(nullptr, nullptr, M, 1, do_sqrt, 0, 0, nullptr);
    int rc = F::prepare(c, fw);
    if (rc != ANNLITE_OK) return rc;
    // stage 0: the k-th smallest exact distance among kFlatSample rows spread over the set
    if ((rc = exact(nullptr, nullptr, kFlatSample, M / kFlatSample, 0, 0, 0, w.thr)) != ANNLITE_OK) return rc;
    // stages 1 .. n: row sets growing by the same factor (<= kFlatGrowth) up to the whole set; each takes the bound of the one before
    const double ratio = (double)M / (double)kFlatSample;
    int n_stages = (int)ceil(log(ratio) / log(kFlatGrowth) - 1e-9);
    if (n_stages < 1) n_stages = 1;
    for (int s = 1; s <= n_stages; ++s) {
        int64_t stride = 1;
        if (s < n_stages) {
            const double want = (double)kFlatSample * pow(ratio, (double)s / n_stages);
            stride = (int64_t)((double)M / want);
            if (stride <= 1) continue;  // (as large as the set already: leave it to the last stage)
        }
        const bool last = s == n_stages;
        ANNLITE_HIP_TRY(hipMemsetAsync(w.cnt, 0, (size_t)B * 4, st));
        if ((rc = F::launch(c, fw, (M + stride - 1) / stride, stride, w.thr, w.cand, w.cnt, nullptr)) != ANNLITE_OK) return rc;
        // (a list that overflowed before the last stage still holds `cap` valid rows: the k-th of ANY k valid rows is a bound)
        if ((rc = exact(w.cand, w.cnt, 0, 1, last ? do_sqrt : 0, last ? 1 : 0, 0, last ? nullptr : w.thr)) != ANNLITE_OK) return rc;
    }
    // queries whose last list overflowed: exact sums over all rows of the set (the other waves leave at once)
    return exact(nullptr, nullptr, M, 1, do_sqrt, 0, 1, nullptr);
}

// ---- the one body behind the six search entries, and the one behind the stage entries: check, carve, check the workspace, run ----------
template <class F>
static int flat_search(const FlatCall &c, int64_t k, int flags, float *out_dist_dev, int64_t *out_id_dev, void *workspace_dev,
                       size_t workspace_bytes) {
    if (int rc = flat_check<F>(kFlatSearch, c, k)) return rc;
    if (c.B == 0) return ANNLITE_OK;
    // (the set's own pointers also where it is empty: a NULL list is the staged search's word for "the whole table")
    ANNLITE_REQUIRE(c.q && out_dist_dev && out_id_dev && workspace_dev && c.set_given() && (c.set_rows() == 0 || (c.x && c.norms)),
                    "null device pointer");
    const typename F::Ws w = F::carve(workspace_dev, c.B, c.D);
    if (int rc = flat_check_workspace(workspace_bytes, w.bytes)) return rc;
    return flat_search_staged(F{}, c, w, k, flags, out_dist_dev, out_id_dev);
}

// One filter stage over every stride-th row of the set, into the caller's lists.  *used (where asked for): the carved workspace, for the
// entries that hand back what prepare() left per query; it is left alone where the call is refused or has nothing to do.
template <class F>
static int flat_stage(const FlatCall &c, int64_t stride, const float *bounds_dev, int32_t *cand_dev, int32_t *count_dev, float *scores_dev,
                      void *workspace_dev, size_t workspace_bytes, typename F::Ws *used = nullptr) {
    if (int rc = flat_check<F>(kFlatStage, c, stride, scores_dev)) return rc;
    const int64_t M = c.set_rows();
    if (c.B == 0 || M == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(c.q && c.x && c.norms && c.set_given() && bounds_dev && cand_dev && count_dev && workspace_dev, "null device pointer");
    const typename F::Ws w = F::carve(workspace_dev, c.B, c.D);
    if (int rc = flat_check_workspace(workspace_bytes, w.bytes)) return rc;
    if (int rc = F::prepare(c, w)) return rc;
    if (used) *used = w;
    return F::launch(c, w, (M + stride - 1) / stride, stride, bounds_dev, cand_dev, count_dev, scores_dev);
}
// ... and such a per-query array handed back, on the stage's stream (per_query NULL: the stage had nothing to do).
static int flat_hand_back(float *out_dev, const float *per_query, int64_t B, hipStream_t st) {
    if (out_dev && per_query) ANNLITE_HIP_TRY(hipMemcpyAsync(out_dev, per_query, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
    return ANNLITE_OK;
}

// The workspace of a search or a stage: the filter's own carve.  The typed entries (`typed`) have never bounded B, N and the f32 filter's
// D by INT32_MAX as the searches do, and keep accepting what they accepted.
static int flat_workspace_bytes(int filter, bool typed, int64_t N, int64_t D, int64_t B, int64_t k, int64_t *bytes) {
    ANNLITE_REQUIRE(bytes != nullptr, "bytes is NULL");
    return flat_with_filter(filter, [&](auto F) -> int {
        auto held = [&](int64_t v) { return typed && v > INT32_MAX ? (int64_t)INT32_MAX : v; };
        if (int rc = flat_check_shape(kFlatSearch, ANNLITE_METRIC_EUCLIDEAN, held(B), held(D), held(N), k, F.kMaxDim)) return rc;
        *bytes = (int64_t)F.carve(nullptr, B, D).bytes;
        return ANNLITE_OK;
    });
}

// ---- cells: workspace, stages, launchers ---------------------------------------------------------------------------------------------
constexpr int kIvfFlatMaxStages = 16;  // strides annlite_ivf_flat_stages can return (2^31 rows: 19 bits of stride, 5 at a time, + the first)

struct IvfFlatWs {
    FlatWs f;  // (first: annlite_flat_overflow_count reads the same counter)
    int64_t n_tiles;
    int32_t *vmap, *slot_of, *n_used;
    int64_t *tile_rows;
    size_t bytes;
};
static IvfFlatWs ivf_flat_carve(void *ws, int64_t B, int64_t P, int64_t C) {
    IvfFlatWs w;
    w.f = flat_carve(ws, B);
    w.n_tiles = annlite_ivf_max_tiles(B, P, C, kFlatTile);
    WsBump b{(char *)ws, w.f.bytes};
    w.tile_rows = b.take<int64_t>((size_t)w.n_tiles * 16);
    w.vmap = b.take<int32_t>((size_t)w.n_tiles * kFlatTile * 4);
    w.slot_of = b.take<int32_t>((size_t)B * P * 4);
    w.n_used = b.take<int32_t>(256);
    w.bytes = b.o;
    return w;
}

// The strides of a search over at most M probed rows per query: strides[0] = the first (exact) sample's, the smallest that keeps
// M / stride at or below kFlatSample; then the filter stages', each row set at most kFlatGrowth times the one before, down to 1.
// None for M <= kFlatSample (exact sums over all probed rows).
static int ivf_flat_strides(int64_t M, int64_t *strides) {
    if (M <= kFlatSample) return 0;
    int64_t s = (M + kFlatSample - 1) / kFlatSample;  // >= 2
    int n = 0;
    strides[n++] = s;
    int rem = (int)ceil(log((double)s) / log(kFlatGrowth) - 1e-9);
    if (rem < 1) rem = 1;
    while (s > 1 && n < kIvfFlatMaxStages) {
        int64_t nx = 1;
        if (rem > 1) nx = (int64_t)ceil((double)s / pow((double)s, 1.0 / rem) - 1e-9);
        if (nx * (int64_t)kFlatGrowth < s) nx = (s + (int64_t)kFlatGrowth - 1) / (int64_t)kFlatGrowth;
        if (nx >= s) nx = s - 1;
        if (nx < 1) nx = 1;
        strides[n++] = s = nx;
        if (rem > 1) --rem;
    }
    return n;
}

static int ivf_flat_launch_filter(int metric, const float *q, int64_t B, int64_t D, const float *x, const float *norms, int64_t N,
                                  const int32_t *perm, int64_t n_perm, const IvfFlatWs &w, int64_t max_cell_rows, int64_t stride,
                                  const uint32_t *valid, hipStream_t st) {
    float c_rel, c_abs;
    flat_slack(metric, D, &c_rel, &c_abs);
    const dim3 grid = ivf_flat_filter_grid(max_cell_rows, stride, w.n_tiles);
    if (grid.x == 0 || grid.y == 0) return ANNLITE_OK;
    const bool vec = D % 4 == 0 && ((uintptr_t)q % 16 == 0) && ((uintptr_t)x % 16 == 0);
    FLAT_LAUNCH_VEC(vec, ivf_flat_filter_kernel, grid, dim3(256), st, metric, q, (int)B, (int)D, x, norms, N, perm, n_perm, w.tile_rows, w.vmap,
                    (int)w.n_tiles, stride, valid, w.f.qnorm, w.f.thr, c_rel, c_abs, w.f.cand, w.f.cnt, kFlatCap);
    return launch_status("ivf_flat_filter_kernel");
}

// ---- the split filter's share of a cells workspace: the query planes and the pair norms BY PLAN SLOT, behind the IvfFlatWs of the same
// (B, P, C) (so that the overflow counter and the list counters sit where annlite_flat_overflow_count / annlite_flat_list_counts read
// them) ----
struct IvfFlatSplitWs {
    IvfFlatWs i;
    int64_t Dp, n_slots;
    __bf16 *qh, *ql;
    float *qnorm;
    size_t bytes;
};
static IvfFlatSplitWs ivf_flat_split_carve(void *ws, int64_t B, int64_t P, int64_t C, int64_t D) {
    IvfFlatSplitWs w;
    w.i = ivf_flat_carve(ws, B, P, C);
    w.Dp = (D + 15) / 16 * 16;
    w.n_slots = w.i.n_tiles * kFlatTile;
    WsBump b{(char *)ws, w.i.bytes};
    w.qh = b.take<__bf16>((size_t)w.n_slots * w.Dp * 2);
    w.ql = b.take<__bf16>((size_t)w.n_slots * w.Dp * 2);
    w.qnorm = b.take<float>((size_t)w.n_slots * 4);
    w.bytes = b.o;
    return w;
}

// Per call, after the plan: centre and split the queries of every pair into its slot's planes.
static int ivf_flat_split_prepare(const float *q, int64_t B, int64_t P, int64_t C, int64_t D, const int32_t *cells, const float *centres,
                                  const IvfFlatSplitWs &w, float *pair_norms, hipStream_t st) {
    hipLaunchKernelGGL(ivf_flat_split_queries_kernel, dim3((unsigned)((B * P + 3) / 4)), dim3(256), 0, st, q, (int)(B * P), (int)P, (int)D,
                       (int)w.Dp, cells, (int)C, centres, w.i.slot_of, (int)w.n_slots, w.qh, w.ql, w.qnorm, pair_norms);
    return launch_status("ivf_flat_split_queries_kernel");
}

static int ivf_flat_split_launch_filter(int metric, int64_t B, int64_t D, const float *x, const float *centres, int64_t C,
                                        const int32_t *cell_of, const float *norms, int64_t N, const int32_t *perm, int64_t n_perm,
                                        const IvfFlatSplitWs &w, int64_t max_cell_rows, int64_t stride, const uint32_t *valid,
                                        const float *thr, int32_t *cand, int32_t *cnt, float *scores, hipStream_t st) {
    float c_rel, c_abs;
    flat_split_slack(metric, D, &c_rel, &c_abs);
    const dim3 grid = ivf_flat_filter_grid(max_cell_rows, stride, w.i.n_tiles);
    if (grid.x == 0 || grid.y == 0) return ANNLITE_OK;
    const bool vec = D % 4 == 0 && ((uintptr_t)x % 16 == 0) && ((uintptr_t)centres % 16 == 0);
    FLAT_LAUNCH_VEC(vec, ivf_flat_split_filter_kernel, grid, dim3(256), st, metric, w.qh, w.ql, (int)B, (int)D, (int)w.Dp, x, centres, (int)C,
                    cell_of, norms, N, perm, n_perm, w.i.tile_rows, w.i.vmap, (int)w.i.n_tiles, stride, valid, w.qnorm, thr, c_rel, c_abs, cand,
                    cnt, kFlatCap, scores);
    return launch_status("ivf_flat_split_filter_kernel");
}

// ---- the stages of a search over cells, shared by annlite_ivf_flat_search_topk and
// annlite_ivf_flat_search_topk_split: the exact-only shortcut, the plan, the first exact sample, the filter stages, the re-rank of the
// lists and the route of an overflowed list.  prepare(): what the filter needs from the queries, once per call, after the plan;
// filter(stride): one filter launch into w.f.cand / w.f.cnt against the bounds w.f.thr. ----
template <class Prepare, class Filter>
static int ivf_flat_search_staged(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev, int64_t N,
                                  const uint32_t *valid_bits_dev, const int32_t *cells_dev, int64_t P, int64_t C, const int32_t *perm_dev,
                                  int64_t n_perm, const int64_t *cell_rows_dev, const int32_t *cell_order_dev, int64_t max_probed_rows,
                                  int64_t k, int flags, float *out_dist_dev, int64_t *out_id_dev, const IvfFlatWs &w, hipStream_t st,
                                  Prepare &&prepare, Filter &&filter) {
    const int do_sqrt = (flags & ANNLITE_FLAG_SQRT) ? 1 : 0;
    const dim3 qgrid((unsigned)((B + 3) / 4));
    ANNLITE_HIP_TRY(hipMemsetAsync(w.f.ovf_total, 0, 256, st));
    auto exact_cells = [&](int64_t stride, int sqrt_out, int only_overflowed, float *thr_out) {
        hipLaunchKernelGGL(ivf_flat_exact_kernel, qgrid, dim3(256), 0, st, metric, queries_dev, (int)B, (int)D, vectors_dev, N, cells_dev, (int)P,
                           (int)C, cell_rows_dev, perm_dev, n_perm, stride, valid_bits_dev, (int)k, sqrt_out, only_overflowed, thr_out,
                           out_dist_dev, out_id_dev, w.f.ovf);
        return launch_status("ivf_flat_exact_kernel");
    };
    int64_t strides[kIvfFlatMaxStages];
    const int n_strides = ivf_flat_strides(max_probed_rows, strides);
    if (n_strides == 0) return exact_cells(1, do_sqrt, 0, nullptr);  // few probed rows: exact sums over all of them
    // the (cell, queries that probe it) tiles of the filter stages
    int rc = annlite_ivf_plan(cells_dev, B, P, C, kFlatTile, cell_rows_dev, cell_order_dev, w.n_tiles, w.vmap, w.slot_of, w.tile_rows, w.n_used,
                              (void *)st);
    if (rc != ANNLITE_OK) return rc;
    if ((rc = prepare()) != ANNLITE_OK) return rc;
    // stage 0: the k-th smallest exact distance among every strides[0]-th entry of the query's cells
    if ((rc = exact_cells(strides[0], 0, 0, w.f.thr)) != ANNLITE_OK) return rc;
    for (int s = 1; s < n_strides; ++s) {
        const bool last = s == n_strides - 1;  // (strides[n_strides - 1] == 1)
        ANNLITE_HIP_TRY(hipMemsetAsync(w.f.cnt, 0, (size_t)B * 4, st));
        if ((rc = filter(strides[s])) != ANNLITE_OK) return rc;
        // the list re-rank of annlite_flat_search_topk, unchanged: the lists hold offsets
        hipLaunchKernelGGL(flat_exact_kernel<float>, qgrid, dim3(256), 0, st, metric, queries_dev, (int)B, (int)D, vectors_dev, N, w.f.cand, w.f.cnt,
                           kFlatCap, (int64_t)0, (int64_t)1, valid_bits_dev, (int)k, last ? do_sqrt : 0, last ? 1 : 0, 0,
                           last ? nullptr : w.f.thr, out_dist_dev, out_id_dev, w.f.ovf, w.f.ovf_total);
        if ((rc = launch_status("flat_exact_kernel")) != ANNLITE_OK) return rc;
    }
    // queries whose last list overflowed: exact sums over all their probed rows (the other waves leave at once)
    return exact_cells(1, do_sqrt, 1, nullptr);
}

}  // namespace annlite

using namespace annlite;

extern "C" int annlite_flat_row_norms(const float *vectors_dev, int64_t capacity, int64_t D, const int64_t *ids_dev, int64_t n, int64_t id_base,
                                      float *norms_dev, void *stream) {
    ANNLITE_REQUIRE(capacity >= 0 && D >= 1 && n >= 0 && D <= INT32_MAX, "bad shape");
    if (n == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(vectors_dev && norms_dev, "null device pointer");
    hipLaunchKernelGGL(flat_norms_kernel<false>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, vectors_dev, (int)D, ids_dev,
                       n, id_base, capacity, (const float *)nullptr, (const int32_t *)nullptr, 0, norms_dev);
    return launch_status("flat_norms_kernel");
}

extern "C" int annlite_flat_list_capacity(void) { return kFlatCap; }

extern "C" int annlite_flat_slack(int metric, int64_t D, float *c_rel, float *c_abs) {
    ANNLITE_REQUIRE(metric >= 1 && metric <= 3 && D >= 1 && c_rel && c_abs, "bad argument");
    flat_slack(metric, D, c_rel, c_abs);
    return ANNLITE_OK;
}

extern "C" int annlite_flat_filter(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev, const float *norms_dev,
                                   int64_t N, int64_t stride, const uint32_t *valid_bits_dev, const float *query_norms_dev,
                                   const float *bounds_dev, int32_t *cand_dev, int32_t *count_dev, void *stream) {
    // (the caller's query norms and no workspace: not flat_stage)
    if (int rc = flat_check_shape(kFlatStage, metric, B, D, N, stride, INT32_MAX)) return rc;
    if (B == 0 || N == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(queries_dev && vectors_dev && norms_dev && query_norms_dev && bounds_dev && cand_dev && count_dev, "null device pointer");
    return flat_launch_filter(metric, queries_dev, B, D, vectors_dev, norms_dev, (N + stride - 1) / stride, stride, valid_bits_dev,
                              query_norms_dev, bounds_dev, cand_dev, count_dev, (hipStream_t)stream);
}

extern "C" int annlite_flat_search_workspace_bytes(int64_t N, int64_t D, int64_t B, int64_t k, int64_t *bytes) {
    return flat_workspace_bytes(ANNLITE_FLAT_FILTER_F32, true, N, D, B, k, bytes);
}

// The typed entries: each fills the operands of a search or a stage over the whole table -- no list, no groups -- and forwards.
static FlatCall flat_table_call(int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_dev, float row_scale,
                                const float *norms_dev, const float *centre_dev, int64_t N, const uint32_t *valid_bits_dev, void *stream) {
    return FlatCall{kFlatTable, metric, queries_dev, B, D, vectors_dev, row_scale, norms_dev, centre_dev, N, valid_bits_dev, nullptr, 0, {},
                    (hipStream_t)stream};
}

extern "C" int annlite_flat_search_topk(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev,
                                        const float *norms_dev, int64_t N, const uint32_t *valid_bits_dev, int64_t k, int flags,
                                        float *out_dist_dev, int64_t *out_id_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    const FlatCall c = flat_table_call(metric, queries_dev, B, D, vectors_dev, 1.f, norms_dev, nullptr, N, valid_bits_dev, stream);
    return flat_search<FlatF32>(c, k, flags, out_dist_dev, out_id_dev, workspace_dev, workspace_bytes);
}

extern "C" int annlite_flat_split_slack(int metric, int64_t D, float *c_rel, float *c_abs) {
    ANNLITE_REQUIRE(metric >= 1 && metric <= 3 && D >= 1 && D <= kSplitMaxDim && c_rel && c_abs, "bad argument (1 <= D <= %lld)",
                    (long long)kSplitMaxDim);
    flat_split_slack(metric, D, c_rel, c_abs);
    return ANNLITE_OK;
}

extern "C" int annlite_flat_centred_norms(const float *vectors_dev, int64_t capacity, int64_t D, const int64_t *ids_dev, int64_t n,
                                          int64_t id_base, const float *centre_dev, float *norms_dev, void *stream) {
    ANNLITE_REQUIRE(capacity >= 0 && D >= 1 && n >= 0 && D <= INT32_MAX, "bad shape");
    if (n == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(vectors_dev && norms_dev && centre_dev, "null device pointer");
    hipLaunchKernelGGL(flat_norms_kernel<true>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, vectors_dev, (int)D, ids_dev, n,
                       id_base, capacity, centre_dev, (const int32_t *)nullptr, 0, norms_dev);
    return launch_status("flat_norms_kernel");
}

extern "C" int annlite_flat_search_split_workspace_bytes(int64_t N, int64_t D, int64_t B, int64_t k, int64_t *bytes) {
    return flat_workspace_bytes(ANNLITE_FLAT_FILTER_BF16X3, true, N, D, B, k, bytes);
}

extern "C" int annlite_flat_filter_split(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev,
                                         const float *norms_dev, int64_t N, int64_t stride, const uint32_t *valid_bits_dev,
                                         float *query_norms_out_dev, const float *bounds_dev, int32_t *cand_dev, int32_t *count_dev,
                                         const float *centre_dev, float *scores_dev, void *workspace_dev, size_t workspace_bytes,
                                         void *stream) {
    const FlatCall c = flat_table_call(metric, queries_dev, B, D, vectors_dev, 1.f, norms_dev, centre_dev, N, valid_bits_dev, stream);
    FlatSplitWs w{};
    if (int rc = flat_stage<FlatBf16x3>(c, stride, bounds_dev, cand_dev, count_dev, scores_dev, workspace_dev, workspace_bytes, &w)) return rc;
    return flat_hand_back(query_norms_out_dev, w.f.qnorm, B, c.st);
}

extern "C" int annlite_flat_search_topk_split(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev,
                                              const float *norms_dev, int64_t N, const uint32_t *valid_bits_dev, const float *centre_dev,
                                              int64_t k, int flags, float *out_dist_dev, int64_t *out_id_dev, void *workspace_dev,
                                              size_t workspace_bytes, void *stream) {
    const FlatCall c = flat_table_call(metric, queries_dev, B, D, vectors_dev, 1.f, norms_dev, centre_dev, N, valid_bits_dev, stream);
    return flat_search<FlatBf16x3>(c, k, flags, out_dist_dev, out_id_dev, workspace_dev, workspace_bytes);
}

// ---- f16 rows ------------------------------------------------------------------------------------------------------------------------
extern "C" int annlite_flat_row_norms_f16(const void *vectors_f16_dev, int64_t capacity, int64_t D, const int64_t *ids_dev, int64_t n,
                                          int64_t id_base, float *norms_dev, void *stream) {
    ANNLITE_REQUIRE(capacity >= 0 && D >= 1 && n >= 0 && D <= INT32_MAX, "bad shape");
    if (n == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(vectors_f16_dev && norms_dev, "null device pointer");
    hipLaunchKernelGGL((flat_norms_kernel<false, _Float16>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const _Float16 *)vectors_f16_dev, (int)D, ids_dev, n, id_base, capacity, (const float *)nullptr, (const int32_t *)nullptr, 0, norms_dev);
    return launch_status("flat_norms_kernel");
}

extern "C" int annlite_flat_f16_slack(int metric, int64_t D, float *c_rel, float *c_abs) {
    ANNLITE_REQUIRE(metric >= 1 && metric <= 3 && D >= 1 && D <= kSplitMaxDim && c_rel && c_abs, "bad argument (1 <= D <= %lld)",
                    (long long)kSplitMaxDim);
    flat_f16_slack(metric, D, c_rel, c_abs);
    return ANNLITE_OK;
}

extern "C" int annlite_flat_search_f16_workspace_bytes(int64_t N, int64_t D, int64_t B, int64_t k, int64_t *bytes) {
    return flat_workspace_bytes(ANNLITE_FLAT_FILTER_F16X2, true, N, D, B, k, bytes);
}

extern "C" int annlite_flat_filter_f16(int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_f16_dev,
                                       const float *norms_dev, int64_t N, int64_t stride, const uint32_t *valid_bits_dev,
                                       float *query_norms_out_dev, float *query_flush_out_dev, const float *bounds_dev, int32_t *cand_dev,
                                       int32_t *count_dev, float *scores_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    const FlatCall c = flat_table_call(metric, queries_dev, B, D, vectors_f16_dev, 1.f, norms_dev, nullptr, N, valid_bits_dev, stream);
    FlatF16Ws w{};
    if (int rc = flat_stage<FlatF16x2>(c, stride, bounds_dev, cand_dev, count_dev, scores_dev, workspace_dev, workspace_bytes, &w)) return rc;
    if (int rc = flat_hand_back(query_norms_out_dev, w.f.qnorm, B, c.st)) return rc;
    return flat_hand_back(query_flush_out_dev, w.qflush, B, c.st);
}

extern "C" int annlite_flat_search_topk_f16(int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_f16_dev,
                                            const float *norms_dev, int64_t N, const uint32_t *valid_bits_dev, int64_t k, int flags,
                                            float *out_dist_dev, int64_t *out_id_dev, void *workspace_dev, size_t workspace_bytes,
                                            void *stream) {
    const FlatCall c = flat_table_call(metric, queries_dev, B, D, vectors_f16_dev, 1.f, norms_dev, nullptr, N, valid_bits_dev, stream);
    return flat_search<FlatF16x2>(c, k, flags, out_dist_dev, out_id_dev, workspace_dev, workspace_bytes);
}

// ---- int8 rows -----------------------------------------------------------------------------------------------------------------------
extern "C" int annlite_flat_row_norms_i8(const void *vectors_i8_dev, float scale, int64_t capacity, int64_t D, const int64_t *ids_dev,
                                         int64_t n, int64_t id_base, float *norms_dev, void *stream) {
    ANNLITE_REQUIRE(capacity >= 0 && D >= 1 && n >= 0 && D <= INT32_MAX, "bad shape");
    ANNLITE_REQUIRE_I8_SCALE(scale);
    if (n == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(vectors_i8_dev && norms_dev, "null device pointer");
    hipLaunchKernelGGL((flat_norms_kernel<false, int8_t>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const int8_t *)vectors_i8_dev, (int)D, ids_dev, n, id_base, capacity, (const float *)nullptr, (const int32_t *)nullptr, 0,
                       norms_dev, scale);
    return launch_status("flat_norms_kernel");
}

extern "C" int annlite_flat_i8_slack(int metric, int64_t D, float *c_rel, float *c_abs) {
    ANNLITE_REQUIRE(metric >= 1 && metric <= 3 && D >= 1 && D <= kSplitMaxDim && c_rel && c_abs, "bad argument (1 <= D <= %lld)",
                    (long long)kSplitMaxDim);
    flat_i8_slack(metric, D, c_rel, c_abs);
    return ANNLITE_OK;
}

extern "C" int annlite_flat_search_i8_workspace_bytes(int64_t N, int64_t D, int64_t B, int64_t k, int64_t *bytes) {
    return flat_workspace_bytes(ANNLITE_FLAT_FILTER_I8X3, true, N, D, B, k, bytes);
}

extern "C" int annlite_flat_filter_i8(int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_i8_dev, float scale,
                                      const float *norms_dev, int64_t N, int64_t stride, const uint32_t *valid_bits_dev,
                                      float *query_norms_out_dev, float *query_slack_out_dev, const float *bounds_dev, int32_t *cand_dev,
                                      int32_t *count_dev, float *scores_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    const FlatCall c = flat_table_call(metric, queries_dev, B, D, vectors_i8_dev, scale, norms_dev, nullptr, N, valid_bits_dev, stream);
    FlatI8Ws w{};
    if (int rc = flat_stage<FlatI8x3>(c, stride, bounds_dev, cand_dev, count_dev, scores_dev, workspace_dev, workspace_bytes, &w)) return rc;
    if (int rc = flat_hand_back(query_norms_out_dev, w.f.qnorm, B, c.st)) return rc;
    return flat_hand_back(query_slack_out_dev, w.qslack, B, c.st);
}

extern "C" int annlite_flat_search_topk_i8(int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_i8_dev, float scale,
                                           const float *norms_dev, int64_t N, const uint32_t *valid_bits_dev, int64_t k, int flags,
                                           float *out_dist_dev, int64_t *out_id_dev, void *workspace_dev, size_t workspace_bytes,
                                           void *stream) {
    const FlatCall c = flat_table_call(metric, queries_dev, B, D, vectors_i8_dev, scale, norms_dev, nullptr, N, valid_bits_dev, stream);
    return flat_search<FlatI8x3>(c, k, flags, out_dist_dev, out_id_dev, workspace_dev, workspace_bytes);
}

// ---- selected rows: the searches above over an ascending list of offsets ("selected rows") ------------------------
// One entry per job: the filter code picks F once (flat_with_filter), and the list goes into the operands.  No bitmap: a row in the
// list is selected.
extern "C" int annlite_flat_search_rows_workspace_bytes(int filter, int64_t n_sel, int64_t D, int64_t B, int64_t k, int64_t *bytes) {
    return flat_workspace_bytes(filter, false, n_sel, D, B, k, bytes);
}

extern "C" int annlite_flat_search_topk_rows(int filter, int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_dev,
                                             float row_scale, const float *norms_dev, const float *centre_dev, int64_t N,
                                             const int32_t *rows_dev, int64_t n_sel, int64_t k, int flags, float *out_dist_dev,
                                             int64_t *out_id_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    const FlatCall c{kFlatRows, metric, queries_dev, B, D, vectors_dev, row_scale, norms_dev, centre_dev, N, nullptr, rows_dev, n_sel, {},
                     (hipStream_t)stream};
    return flat_with_filter(filter, [&](auto F) {
        return flat_search<decltype(F)>(c, k, flags, out_dist_dev, out_id_dev, workspace_dev, workspace_bytes);
    });
}

extern "C" int annlite_flat_filter_rows(int filter, int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_dev,
                                        float row_scale, const float *norms_dev, const float *centre_dev, int64_t N, const int32_t *rows_dev,
                                        int64_t n_sel, int64_t stride, const float *bounds_dev, int32_t *cand_dev, int32_t *count_dev,
                                        float *scores_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    const FlatCall c{kFlatRows, metric, queries_dev, B, D, vectors_dev, row_scale, norms_dev, centre_dev, N, nullptr, rows_dev, n_sel, {},
                     (hipStream_t)stream};
    return flat_with_filter(filter, [&](auto F) {
        return flat_stage<decltype(F)>(c, stride, bounds_dev, cand_dev, count_dev, scores_dev, workspace_dev, workspace_bytes);
    });
}

// ---- a filter per query: the searches above over the table with G bitmaps ("a filter per query") --------------------
// One entry per job, as the selected-rows entries: the groups go into the operands, behind the live bitmap.
extern "C" int annlite_flat_search_grouped_workspace_bytes(int filter, int64_t N, int64_t D, int64_t B, int64_t k, int64_t *bytes) {
    return flat_workspace_bytes(filter, false, N, D, B, k, bytes);
}

extern "C" int annlite_flat_search_topk_grouped(int filter, int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_dev,
                                                float row_scale, const float *norms_dev, const float *centre_dev, int64_t N,
                                                const uint32_t *valid_bits_dev, const uint32_t *masks_dev, int64_t mask_ld, int64_t G,
                                                const int32_t *group_dev, int64_t k, int flags, float *out_dist_dev, int64_t *out_id_dev,
                                                void *workspace_dev, size_t workspace_bytes, void *stream) {
    FlatCall c{kFlatGrouped, metric, queries_dev, B, D, vectors_dev, row_scale, norms_dev, centre_dev, N, valid_bits_dev, nullptr, 0, {},
               (hipStream_t)stream};
    if (int rc = flat_groups(masks_dev, mask_ld, G, group_dev, &c.grp)) return rc;
    return flat_with_filter(filter, [&](auto F) {
        return flat_search<decltype(F)>(c, k, flags, out_dist_dev, out_id_dev, workspace_dev, workspace_bytes);
    });
}

extern "C" int annlite_flat_filter_grouped(int filter, int metric, const float *queries_dev, int64_t B, int64_t D, const void *vectors_dev,
                                           float row_scale, const float *norms_dev, const float *centre_dev, int64_t N,
                                           const uint32_t *valid_bits_dev, const uint32_t *masks_dev, int64_t mask_ld, int64_t G,
                                           const int32_t *group_dev, int64_t stride, const float *bounds_dev, int32_t *cand_dev,
                                           int32_t *count_dev, float *scores_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    FlatCall c{kFlatGrouped, metric, queries_dev, B, D, vectors_dev, row_scale, norms_dev, centre_dev, N, valid_bits_dev, nullptr, 0, {},
               (hipStream_t)stream};
    if (int rc = flat_groups(masks_dev, mask_ld, G, group_dev, &c.grp)) return rc;
    return flat_with_filter(filter, [&](auto F) {
        return flat_stage<decltype(F)>(c, stride, bounds_dev, cand_dev, count_dev, scores_dev, workspace_dev, workspace_bytes);
    });
}

extern "C" int annlite_flat_overflow_count(const void *workspace_dev, void *stream, int64_t *count) {
    ANNLITE_REQUIRE(workspace_dev && count, "null pointer");
    uint32_t v = 0;
    ANNLITE_HIP_TRY(hipMemcpyAsync(&v, workspace_dev, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
    ANNLITE_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    *count = (int64_t)v;
    return ANNLITE_OK;
}

extern "C" int annlite_flat_list_counts(const void *workspace_dev, int64_t B, int32_t *count_dev, void *stream) {
    ANNLITE_REQUIRE(workspace_dev && count_dev && B >= 0, "bad argument");
    if (B == 0) return ANNLITE_OK;
    const FlatWs w = flat_carve(const_cast<void *>(workspace_dev), B);
    ANNLITE_HIP_TRY(hipMemcpyAsync(count_dev, w.cnt, (size_t)B * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ANNLITE_OK;
}

extern "C" int annlite_ivf_flat_stages(int64_t max_probed_rows, int64_t *strides_out, int *n_out) {
    ANNLITE_REQUIRE(max_probed_rows >= 0 && strides_out && n_out, "bad argument");
    *n_out = ivf_flat_strides(max_probed_rows, strides_out);
    return ANNLITE_OK;
}

extern "C" int annlite_ivf_flat_search_workspace_bytes(int64_t B, int64_t P, int64_t C, int64_t k, int64_t *bytes) {
    ANNLITE_REQUIRE(bytes != nullptr, "bytes is NULL");
    ANNLITE_REQUIRE(B >= 0 && P >= 1 && C >= 1 && k >= 1 && k <= 64, "bad shape (1 <= k <= 64)");
    *bytes = (int64_t)ivf_flat_carve(nullptr, B, P, C).bytes;
    return ANNLITE_OK;
}

extern "C" int annlite_ivf_flat_search_topk(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev,
                                            const float *norms_dev, int64_t N, const uint32_t *valid_bits_dev, const int32_t *cells_dev,
                                            int64_t P, int64_t C, const int32_t *perm_dev, int64_t n_perm, const int64_t *cell_rows_dev,
                                            const int32_t *cell_order_dev, int64_t max_cell_rows, int64_t max_probed_rows, int64_t k,
                                            int flags, float *out_dist_dev, int64_t *out_id_dev, void *workspace_dev,
                                            size_t workspace_bytes, void *stream) {
    if (int rc = flat_check_shape(kFlatSearch, metric, B, D, N, k, INT32_MAX)) return rc;
    ANNLITE_REQUIRE(P >= 1 && C >= 1 && C <= 16384 && P <= INT32_MAX && n_perm >= 0 && n_perm <= N && max_cell_rows >= 0 &&
                        max_cell_rows <= n_perm && max_probed_rows >= 0,
                    "bad cells P=%lld C=%lld n_perm=%lld max_cell_rows=%lld max_probed_rows=%lld", (long long)P, (long long)C,
                    (long long)n_perm, (long long)max_cell_rows, (long long)max_probed_rows);
    if (B == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(queries_dev && out_dist_dev && out_id_dev && workspace_dev && cells_dev && cell_rows_dev && cell_order_dev &&
                        (n_perm == 0 || (vectors_dev && norms_dev && perm_dev)),
                    "null device pointer");
    const IvfFlatWs w = ivf_flat_carve(workspace_dev, B, P, C);
    if (int rc = flat_check_workspace(workspace_bytes, w.bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ivf_flat_search_staged(
        metric, queries_dev, B, D, vectors_dev, N, valid_bits_dev, cells_dev, P, C, perm_dev, n_perm, cell_rows_dev, cell_order_dev,
        max_probed_rows, k, flags, out_dist_dev, out_id_dev, w, st,
        [&]() { return annlite_flat_row_norms(queries_dev, B, D, nullptr, B, 0, w.f.qnorm, stream); },
        [&](int64_t stride) {
            return ivf_flat_launch_filter(metric, queries_dev, B, D, vectors_dev, norms_dev, N, perm_dev, n_perm, w, max_cell_rows, stride,
                                          valid_bits_dev, st);
        });
}

// ---- the split filter over cell tiles ---------------------------------------------------------------------------------------------------
extern "C" int annlite_ivf_flat_centred_norms(const float *vectors_dev, int64_t capacity, int64_t D, const int64_t *ids_dev, int64_t n,
                                              int64_t id_base, const float *centres_dev, int64_t C, const int32_t *cell_of_dev,
                                              float *norms_dev, void *stream) {
    ANNLITE_REQUIRE(capacity >= 0 && D >= 1 && n >= 0 && D <= INT32_MAX && C >= 1 && C <= 16384, "bad shape");
    if (n == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(vectors_dev && norms_dev && centres_dev && cell_of_dev, "null device pointer");
    hipLaunchKernelGGL(flat_norms_kernel<true>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, vectors_dev, (int)D, ids_dev, n,
                       id_base, capacity, centres_dev, cell_of_dev, (int)C, norms_dev);
    return launch_status("flat_norms_kernel");
}

extern "C" int annlite_ivf_flat_search_split_workspace_bytes(int64_t B, int64_t P, int64_t C, int64_t D, int64_t k, int64_t *bytes) {
    ANNLITE_REQUIRE(bytes != nullptr, "bytes is NULL");
    ANNLITE_REQUIRE(B >= 0 && P >= 1 && C >= 1 && D >= 1 && D <= kSplitMaxDim && k >= 1 && k <= 64, "bad shape (1 <= k <= 64, D <= %lld)",
                    (long long)kSplitMaxDim);
    *bytes = (int64_t)ivf_flat_split_carve(nullptr, B, P, C, D).bytes;
    return ANNLITE_OK;
}

extern "C" int annlite_ivf_flat_filter_split(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev,
                                             const float *norms_dev, int64_t N, const uint32_t *valid_bits_dev, const int32_t *cells_dev,
                                             int64_t P, int64_t C, const int32_t *perm_dev, int64_t n_perm, const int64_t *cell_rows_dev,
                                             const int32_t *cell_order_dev, int64_t max_cell_rows, int64_t stride, const float *centres_dev,
                                             const int32_t *cell_of_dev, const float *bounds_dev, int32_t *cand_dev, int32_t *count_dev,
                                             float *pair_norms_out_dev, float *scores_dev, void *workspace_dev, size_t workspace_bytes,
                                             void *stream) {
    if (int rc = flat_check_shape(kFlatStage, metric, B, D, N, stride, kSplitMaxDim)) return rc;
    ANNLITE_REQUIRE(P >= 1 && C >= 1 && C <= 16384 && B * P <= INT32_MAX && n_perm >= 0 && n_perm <= N && max_cell_rows >= 0 &&
                        max_cell_rows <= n_perm,
                    "bad cells P=%lld C=%lld n_perm=%lld max_cell_rows=%lld", (long long)P, (long long)C, (long long)n_perm,
                    (long long)max_cell_rows);
    ANNLITE_REQUIRE(!centres_dev || metric == ANNLITE_METRIC_EUCLIDEAN, "centres are for EUCLIDEAN only");
    ANNLITE_REQUIRE(!centres_dev || cell_of_dev, "centres need cell_of_dev");
    if (B == 0 || n_perm == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(queries_dev && vectors_dev && norms_dev && perm_dev && cells_dev && cell_rows_dev && cell_order_dev && bounds_dev &&
                        cand_dev && count_dev && workspace_dev,
                    "null device pointer");
    const IvfFlatSplitWs w = ivf_flat_split_carve(workspace_dev, B, P, C, D);
    if (int rc = flat_check_workspace(workspace_bytes, w.bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    int rc = annlite_ivf_plan(cells_dev, B, P, C, kFlatTile, cell_rows_dev, cell_order_dev, w.i.n_tiles, w.i.vmap, w.i.slot_of, w.i.tile_rows,
                              w.i.n_used, stream);
    if (rc != ANNLITE_OK) return rc;
    if ((rc = ivf_flat_split_prepare(queries_dev, B, P, C, D, cells_dev, centres_dev, w, pair_norms_out_dev, st)) != ANNLITE_OK) return rc;
    return ivf_flat_split_launch_filter(metric, B, D, vectors_dev, centres_dev, C, cell_of_dev, norms_dev, N, perm_dev, n_perm, w, max_cell_rows,
                                        stride, valid_bits_dev, bounds_dev, cand_dev, count_dev, scores_dev, st);
}

extern "C" int annlite_ivf_flat_search_topk_split(int metric, const float *queries_dev, int64_t B, int64_t D, const float *vectors_dev,
                                                  const float *norms_dev, int64_t N, const uint32_t *valid_bits_dev,
                                                  const int32_t *cells_dev, int64_t P, int64_t C, const int32_t *perm_dev, int64_t n_perm,
                                                  const int64_t *cell_rows_dev, const int32_t *cell_order_dev, int64_t max_cell_rows,
                                                  int64_t max_probed_rows, const float *centres_dev, const int32_t *cell_of_dev, int64_t k,
                                                  int flags, float *out_dist_dev, int64_t *out_id_dev, void *workspace_dev,
                                                  size_t workspace_bytes, void *stream) {
    if (int rc = flat_check_shape(kFlatSearch, metric, B, D, N, k, kSplitMaxDim)) return rc;
    ANNLITE_REQUIRE(P >= 1 && C >= 1 && C <= 16384 && B * P <= INT32_MAX && n_perm >= 0 && n_perm <= N && max_cell_rows >= 0 &&
                        max_cell_rows <= n_perm && max_probed_rows >= 0,
                    "bad cells P=%lld C=%lld n_perm=%lld max_cell_rows=%lld max_probed_rows=%lld", (long long)P, (long long)C,
                    (long long)n_perm, (long long)max_cell_rows, (long long)max_probed_rows);
    ANNLITE_REQUIRE(!centres_dev || metric == ANNLITE_METRIC_EUCLIDEAN, "centres are for EUCLIDEAN only");
    ANNLITE_REQUIRE(!centres_dev || cell_of_dev, "centres need cell_of_dev");
    if (B == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(queries_dev && out_dist_dev && out_id_dev && workspace_dev && cells_dev && cell_rows_dev && cell_order_dev &&
                        (n_perm == 0 || (vectors_dev && norms_dev && perm_dev)),
                    "null device pointer");
    const IvfFlatSplitWs w = ivf_flat_split_carve(workspace_dev, B, P, C, D);
    if (int rc = flat_check_workspace(workspace_bytes, w.bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ivf_flat_search_staged(
        metric, queries_dev, B, D, vectors_dev, N, valid_bits_dev, cells_dev, P, C, perm_dev, n_perm, cell_rows_dev, cell_order_dev,
        max_probed_rows, k, flags, out_dist_dev, out_id_dev, w.i, st,
        [&]() { return ivf_flat_split_prepare(queries_dev, B, P, C, D, cells_dev, centres_dev, w, nullptr, st); },
        [&](int64_t stride) {
            return ivf_flat_split_launch_filter(metric, B, D, vectors_dev, centres_dev, C, cell_of_dev, norms_dev, N, perm_dev, n_perm, w,
                                                max_cell_rows, stride, valid_bits_dev, w.i.f.thr, w.i.f.cand, w.i.f.cnt, nullptr, st);
        });
}
