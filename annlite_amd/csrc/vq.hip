// vq.hip -- the coarse quantiser's own kernels (gfx950 only): the nearest centroid of every row of a table on
// f32 MFMA, and the per-cell sums of a Lloyd step without float atomics.
//
// Reference seam: VQCodec.encode (annlite/core/codec/vq.py:78-90: scipy.cluster.vq.vq, first minimum wins) and the update half of
// sklearn's KMeans behind VQCodec.fit (vq.py:41-50).  The answer is ivf_select_cells_kernel<0>'s with one probe (ivf.hip), bit for bit:
// that kernel was shaped for ~1024 queries probing P cells, and streams the whole codebook per 4 rows.
//
// Assignment = the project's method (section 3.6): a contraction with a proven slack decides most rows, the exact arithmetic the rest.
//   vq_norms_kernel     |c|^2 and the centroid's share of the slack, once per codebook; clears the undecided counter
//   vq_assign_kernel    128 rows x (blocks of 128 centroids) per workgroup on v_mfma_f32_32x32x2_f32: per row the best score, its cell
//                       and the lowest slack-reduced score of any other cell; a row whose gap the slack cannot cover goes to a list
//   vq_assign_rest_kernel   the listed rows in ivf_select_cells_kernel<0>'s arithmetic, operation for operation (no host read between)
// Update:
//   vq_cell_bounds_kernel   first sorted position of every cell, from the stably sorted assignment
//   vq_cell_sums_kernel     one workgroup per (cell, 64-coordinate slab, chunk slot): f64 lanes, waves combined in wave order
//   vq_cell_fold_kernel     cells longer than one chunk: their chunk partials in chunk order, rounded once
#include <math.h>

#include "common.h"

namespace annlite {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kVqTile = 128;           // rows x centroids of a workgroup tile (4 waves, 64 x 64 each: 2 x 2 MFMA tiles of 32 x 32)
constexpr int kVqDepth = 32;           // coordinates per LDS stage
constexpr int kVqLd = kVqDepth + 1;    // LDS row pitch in floats: the 32 rows of one MFMA operand on 32 banks
constexpr int64_t kVqMaxC = 65536, kVqMaxDim = 32768;
constexpr int kVqRestRows = 4;         // rows per workgroup of the second launch (ivf_select_cells_kernel's kSelQB)
constexpr int kVqRestLdsDim = 4096;    // ... whose rows sit in LDS up to this D (64 KB) and are read from L2 above it
constexpr int kVqSlab = 64;            // coordinates per workgroup of the sums
constexpr int kVqChunk = 8192;         // rows per chunk of a cell's sum

// ---- |c|^2 per centroid: flat_norms_kernel's chain (a lane-strided fmaf chain + the butterfly; relative error <= gamma(ceil(D/64) + 6)),
// and ec = fl(fl(c_rel |c|^2) + c_abs), the centroid's share of the slack.  Thread 0 clears the undecided counter of the call. ----
__global__ __launch_bounds__(256) void vq_norms_kernel(const float *__restrict__ cent, int C, int D, float c_rel, float c_abs,
                                                      float *__restrict__ cn, float *__restrict__ ec, uint32_t *__restrict__ counter) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *counter = 0u;
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    const float *cr = cent + (int64_t)c * D;
    float s = 0.f;
    for (int j = lane; j < D; j += 64) s = __builtin_fmaf(cr[j], cr[j], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
        cn[c] = s;
        ec[c] = c_rel * s + c_abs;
    }
}

// ---- the contraction ---------------------------------------------------------------------------------------------------------------
// Operands: A = centroids (lane l: centroid l & 31, coordinate l >> 5), B = rows (lane l: coordinate l >> 5, row l & 31); C/D: row =
// lane & 31, centroid = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  A lane therefore owns ONE row per tile and meets its centroids in
// ascending order: the row's running state sits in registers, and the strict '<' keeps the lowest cell of equal scores.
//
// Per (row, cell): s = fl(|c|^2 - 2 dot), eps = fl(fl(c_rel |x|^2) + ec[cell]) >= |s + |x|^2 - dhat|, dhat the j-ascending fmaf chain of
// (c_j - x_j)^2 that ivf_select_cells_kernel<0> ranks (derivation: DESIGN.md section 3.11; c_rel, c_abs: vq_slack below).
// Per row: best = min s (lowest cell of equals), blo = best - eps(best's cell), rest = min (s - eps) over every OTHER cell seen.
// rest - best > eps(best's cell) proves dhat(best's cell) < dhat(c) for every other c: the chain's strict first minimum.  Anything
// else -- and every row that met a NaN or infinite score -- is undecided.
struct VqAcc {
    f32x16 c00, c01, c10, c11;  // c<centroid half><row half>
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int e = 0; e < 16; ++e) c00[e] = c01[e] = c10[e] = c11[e] = 0.f;
    }
    __device__ __forceinline__ const f32x16 &tile(int ci, int rj) const { return ci == 0 ? (rj == 0 ? c00 : c01) : (rj == 0 ? c10 : c11); }
};

struct VqRow {
    float best, blo, rest, z;  // z: 0, or NaN once a score was not finite
    int cell;
    __device__ __forceinline__ void reset() {
        best = blo = rest = __builtin_inff();
        z = 0.f;
        cell = 0x7fffffff;
    }
    __device__ __forceinline__ void offer(float s, float lo, int c) {
        if (s < best) {
            rest = blo < rest ? blo : rest;
            best = s, blo = lo, cell = c;
        } else {
            rest = lo < rest ? lo : rest;
        }
    }
};

// One LDS stage: coordinates k0 .. k0 + 32 of the block's 128 centroids into As and of the tile's 128 rows into Bs, zeros past D, C and
// N.  NORMS (the first centroid block): every thread also adds the squares of the row values it moves to xa[] -- VEC: 4 rows per thread,
// 8 threads per row; scalar: 16 rows per thread, 32 threads per row -- so |x|^2 costs no load of its own.
template <bool VEC>
__device__ __forceinline__ void vq_stage(int tid, int k0, int D, const float *__restrict__ cent, int c0, int C, const float *__restrict__ x,
                                         int64_t r0, int64_t N, float *As, float *Bs, bool norms, float *xa) {
    if constexpr (VEC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 256;  // 1024 slots of 4 floats
            const int r = e >> 3, c = (e & 7) * 4;
            f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
            if (c0 + r < C && k0 + c < D) va = *(const f32x4 *)(cent + (int64_t)(c0 + r) * D + k0 + c);
            if (r0 + r < N && k0 + c < D) vb = *(const f32x4 *)(x + (r0 + r) * D + k0 + c);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                As[r * kVqLd + c + t] = va[t];
                Bs[r * kVqLd + c + t] = vb[t];
            }
            if (norms) {
#pragma unroll
                for (int t = 0; t < 4; ++t) xa[i] = __builtin_fmaf(vb[t], vb[t], xa[i]);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = tid + i * 256;  // 4096 floats
            const int r = e >> 5, c = e & 31;
            const float va = (c0 + r < C && k0 + c < D) ? cent[(int64_t)(c0 + r) * D + k0 + c] : 0.f;
            const float vb = (r0 + r < N && k0 + c < D) ? x[(r0 + r) * D + k0 + c] : 0.f;
            As[r * kVqLd + c] = va;
            Bs[r * kVqLd + c] = vb;
            if (norms) xa[i] = __builtin_fmaf(vb, vb, xa[i]);
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void vq_assign_kernel(const float *__restrict__ x, int64_t N, int D, const float *__restrict__ cent, int C,
                                                       const float *__restrict__ cn, const float *__restrict__ ec, float c_rel,
                                                       int32_t *__restrict__ cells, uint32_t *__restrict__ counter,
                                                       int32_t *__restrict__ list) {
    __shared__ float As[kVqTile * kVqLd];  // the centroid block's stage; after the last block: the rows' states, [5][4][128]
    __shared__ float Bs[kVqTile * kVqLd];  // the row tile's stage
    __shared__ float cns[kVqTile], ecs[kVqTile], xns[kVqTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kVqTile;
    const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
    const int l31 = lane & 31, lh = lane >> 5;
    constexpr int kXa = VEC ? 4 : 16;
    float xa[kXa];
#pragma unroll
    for (int i = 0; i < kXa; ++i) xa[i] = 0.f;
    VqRow st[2];
    st[0].reset(), st[1].reset();
    float ex[2] = {0.f, 0.f};  // fl(c_rel |x|^2) of the lane's two rows
    for (int c0 = 0; c0 < C; c0 += kVqTile) {
        __syncthreads();  // the previous block's epilogue has read cns / ecs
        if (tid < kVqTile) {
            const bool ok = c0 + tid < C;
            cns[tid] = ok ? cn[c0 + tid] : 0.f;
            ecs[tid] = ok ? ec[c0 + tid] : 0.f;
        }
        VqAcc acc;
        acc.zero();
        for (int k0 = 0; k0 < D; k0 += kVqDepth) {
            __syncthreads();  // the previous stage is consumed
            vq_stage<VEC>(tid, k0, D, cent, c0, C, x, r0, N, As, Bs, c0 == 0, xa);
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < kVqDepth; kk += 2) {
                const int kc = kk + lh;
                const float a0 = As[(wc + l31) * kVqLd + kc], a1 = As[(wc + 32 + l31) * kVqLd + kc];
                const float b0 = Bs[(wr + l31) * kVqLd + kc], b1 = Bs[(wr + 32 + l31) * kVqLd + kc];
                acc.c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc.c00, 0, 0, 0);
                acc.c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc.c01, 0, 0, 0);
                acc.c10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc.c10, 0, 0, 0);
                acc.c11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc.c11, 0, 0, 0);
            }
        }
        if (c0 == 0) {  // |x|^2: the threads that moved a row fold their chains (adjacent lanes), one of them writes
            constexpr int kShare = VEC ? 8 : 32;
#pragma unroll
            for (int i = 0; i < kXa; ++i) {
                float s = xa[i];
#pragma unroll
                for (int o = kShare >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
                const int r = VEC ? (tid >> 3) + 32 * i : (tid >> 5) + 8 * i;
                if ((tid & (kShare - 1)) == 0) xns[r] = s;
            }
            __syncthreads();
            ex[0] = c_rel * xns[wr + l31];
            ex[1] = c_rel * xns[wr + 32 + l31];
        }
#pragma unroll
        for (int ci = 0; ci < 2; ++ci) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int cl = wc + ci * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                if (c0 + cl >= C) continue;  // a pad centroid never competes
                const float cnv = cns[cl], ecv = ecs[cl];
#pragma unroll
                for (int rj = 0; rj < 2; ++rj) {
                    const float s = __builtin_fmaf(-2.f, acc.tile(ci, rj)[reg], cnv);  // fl(|c|^2 - 2 dot): 2 dot is exact
                    st[rj].z = __builtin_fmaf(s, 0.f, st[rj].z);                       // NaN or inf -> NaN, and stays
                    st[rj].offer(s, s - (ex[rj] + ecv), c0 + cl);
                }
            }
        }
    }
    // the four lanes that share a row -- two halves of a wave, two waves -- meet in LDS; thread t < 128 merges row t
    __syncthreads();
    float *sb = As;
    {
        const int slot = (wave & 1) * 2 + lh;
#pragma unroll
        for (int rj = 0; rj < 2; ++rj) {
            const int r = wr + rj * 32 + l31;
            sb[(0 * 4 + slot) * kVqTile + r] = st[rj].best;
            sb[(1 * 4 + slot) * kVqTile + r] = st[rj].blo;
            sb[(2 * 4 + slot) * kVqTile + r] = st[rj].rest;
            sb[(3 * 4 + slot) * kVqTile + r] = st[rj].z;
            sb[(4 * 4 + slot) * kVqTile + r] = __int_as_float(st[rj].cell);
        }
    }
    __syncthreads();
    if (tid < kVqTile && r0 + tid < N) {
        VqRow m;
        m.reset();
        float z = 0.f;
#pragma unroll
        for (int slot = 0; slot < 4; ++slot) {
            const float b = sb[(0 * 4 + slot) * kVqTile + tid], lo = sb[(1 * 4 + slot) * kVqTile + tid];
            const float rs = sb[(2 * 4 + slot) * kVqTile + tid];
            const int c = __float_as_int(sb[(4 * 4 + slot) * kVqTile + tid]);
            z += sb[(3 * 4 + slot) * kVqTile + tid];
            m.rest = rs < m.rest ? rs : m.rest;
            if (b < m.best || (b == m.best && c < m.cell)) {  // (score, cell) ascending: the slots hold disjoint cells
                m.rest = m.blo < m.rest ? m.blo : m.rest;
                m.best = b, m.blo = lo, m.cell = c;
            } else {
                m.rest = lo < m.rest ? lo : m.rest;
            }
        }
        const float eps = m.best - m.blo;  // (within one rounding of eps(best's cell): the slack's margin covers it)
        // eps < c_rel 1e37: |x|^2 + |c|^2 < 1.1e37, so the chain of the best cell (<= 2 (|x|^2 + |c|^2)) cannot overflow to a tie at +inf
        const bool decided = z == 0.f && (unsigned)m.cell < (unsigned)C && (m.rest - m.best) > eps && eps < c_rel * 1e37f;
        const int64_t row = r0 + tid;
        cells[row] = decided ? m.cell : -1;
        if (!decided) list[atomicAdd(counter, 1u)] = (int32_t)row;  // (at most N entries: one per row)
    }
}

// ---- the undecided rows: ivf_select_cells_kernel<0> with one probe over a LIST of rows -------------------------------------------------
// One 256-thread workgroup per 4 listed rows, walking the list by the grid's stride; count is read from the first launch's counter.
// Thread t owns the centroids t, t + 256, ... and keeps 4 running sums while it streams a centroid row once -- the same j-ascending
// fmaf chain of (c_j - x_j)^2, the same `+ 0.f` and f32_to_key.  With one probe the C keys need no LDS: a thread keeps the first
// minimum of its (ascending) cells, the workgroup the minimum of (key, cell) -- what the selection's one round returns.  So this
// path has no C + D limit.  LDSROWS: the 4 rows sit in LDS (D <= 4096) or are read from L2 through a wave-uniform address.
template <bool LDSROWS>
__global__ __launch_bounds__(256) void vq_assign_rest_kernel(const float *__restrict__ x, int D, const float *__restrict__ cent, int C,
                                                            const uint32_t *__restrict__ counter, const int32_t *__restrict__ list,
                                                            int32_t *__restrict__ cells) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *qs = (float *)smem;  // [4][D] (LDSROWS)
    __shared__ uint32_t wk[4][kVqRestRows], wcell[4][kVqRestRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t count = *counter;
    for (uint32_t g0 = blockIdx.x * kVqRestRows; g0 < count; g0 += gridDim.x * kVqRestRows) {
        const float *xr[kVqRestRows];
#pragma unroll
        for (int u = 0; u < kVqRestRows; ++u) xr[u] = x + (int64_t)list[g0 + u < count ? g0 + u : g0] * D;  // (past the end: the first again, unwritten)
        if constexpr (LDSROWS) {
            __syncthreads();  // the previous group's sums are done
#pragma unroll
            for (int u = 0; u < kVqRestRows; ++u)
                for (int j = tid; j < D; j += 256) qs[u * D + j] = xr[u][j];
            __syncthreads();
        }
        uint32_t bk[kVqRestRows], bc[kVqRestRows];
#pragma unroll
        for (int u = 0; u < kVqRestRows; ++u) bk[u] = kKeyInfHi, bc[u] = 0xffffffffu;
        for (int c = tid; c < C; c += 256) {
            float acc[kVqRestRows];
#pragma unroll
            for (int u = 0; u < kVqRestRows; ++u) acc[u] = 0.f;
            const float *cr = cent + (int64_t)c * D;
            auto step = [&](float cv, int j) {  // sequential in j: one defined summation order per (row, cell)
#pragma unroll
                for (int u = 0; u < kVqRestRows; ++u) {
                    const float qv = LDSROWS ? qs[u * D + j] : xr[u][j];
                    const float d = cv - qv;
                    acc[u] = __builtin_fmaf(d, d, acc[u]);
                }
            };
            if ((D & 3) == 0 && ((uintptr_t)cent & 15) == 0) {  // (the loads' width only: the sums are the same either way)
                for (int j = 0; j < D; j += 4) {
                    const f32x4 cv = *(const f32x4 *)(cr + j);
                    step(cv.x, j);
                    step(cv.y, j + 1);
                    step(cv.z, j + 2);
                    step(cv.w, j + 3);
                }
            } else {
                for (int j = 0; j < D; ++j) step(cr[j], j);
            }
#pragma unroll
            for (int u = 0; u < kVqRestRows; ++u) {
                const uint32_t k = f32_to_key(acc[u] + 0.f);
                if (k < bk[u]) bk[u] = k, bc[u] = (uint32_t)c;  // (ascending c: the strict '<' keeps the lowest cell of equal keys)
            }
        }
#pragma unroll
        for (int u = 0; u < kVqRestRows; ++u) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t ok = __shfl_xor(bk[u], o), oc = __shfl_xor(bc[u], o);
                if (key_less(ok, oc, bk[u], bc[u])) bk[u] = ok, bc[u] = oc;
            }
            if (lane == 0) wk[wave][u] = bk[u], wcell[wave][u] = bc[u];
        }
        __syncthreads();
        if (tid < kVqRestRows && g0 + tid < count) {
            uint32_t k = wk[0][tid], c = wcell[0][tid];
#pragma unroll
            for (int w = 1; w < 4; ++w)
                if (key_less(wk[w][tid], wcell[w][tid], k, c)) k = wk[w][tid], c = wcell[w][tid];
            cells[list[g0 + tid]] = (int32_t)c;  // (C >= 1 and every key is below kKeyInfHi: c < C)
        }
        __syncthreads();  // wk / wcell are read before the next group writes them
    }
}

// ---- the update half: sums and counts per cell, independent of scheduling ------------------------------------------------------------
// sorted i32 [N] = the assignment in ascending order, perm i64 [N] = the row of every sorted position (a STABLE sort: the rows of a cell
// ascend).  start[c] = the first sorted position of cell c, start[C] = N; a cell id outside [0, C) counts as the nearest end.
__device__ __forceinline__ int vq_cell_clamp(int c, int C) { return c < 0 ? 0 : c >= C ? C - 1 : c; }

__global__ __launch_bounds__(256) void vq_cell_bounds_kernel(const int32_t *__restrict__ sorted, int64_t N, int C, int64_t *__restrict__ start) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > N) return;
    // position i opens the cells (cell of i - 1, cell of i]; position N stands for cell C, position -1 for cell -1
    const int lo = i == 0 ? -1 : vq_cell_clamp(sorted[i - 1], C);
    const int hi = i == N ? C : vq_cell_clamp(sorted[i], C);
    for (int c = lo + 1; c <= hi; ++c) start[c] = i;
}

// Chunk k of a cell = its sorted positions [k L, (k + 1) L), L = kVqChunk.  Wave w takes the chunk's rows w, w + 4, ... in ascending
// order, lane l adds coordinate 64 slab + l in float64 (a gathered row is one coalesced 256-byte read); the four partials are added in
// wave order.  A cell of one chunk is rounded to f32 and written here; a longer one writes every chunk's f64 total to `part`, slot
// 2 (p / L) + (k == 0) for a chunk that starts at sorted position p -- two chunks of cells LONGER than L can start in the same window of
// L positions only as the last chunk of one cell and the first of the next, so the slots are distinct.
__global__ __launch_bounds__(256) void vq_cell_sums_kernel(const float *__restrict__ x, int64_t N, int D, const int64_t *__restrict__ perm,
                                                          const int64_t *__restrict__ start, float *__restrict__ sums,
                                                          int32_t *__restrict__ counts, double *__restrict__ part) {
    __shared__ double ws[4][kVqSlab];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x, j = blockIdx.y * kVqSlab + lane;
    int64_t b = start[c], len = start[c + 1] - b;
    b = b < 0 ? 0 : b > N ? N : b;  // (an assignment that was not sorted: wrong sums, no wild read)
    len = len < 0 ? 0 : len > N - b ? N - b : len;
    if (blockIdx.y == 0 && blockIdx.z == 0 && tid == 0) counts[c] = (int32_t)len;
    if (len == 0 && blockIdx.z == 0 && j < D && wave == 0) sums[(int64_t)c * D + j] = 0.f;
    const int64_t n_chunks = (len + kVqChunk - 1) / kVqChunk;
    for (int64_t k = blockIdx.z; k < n_chunks; k += gridDim.z) {
        const int64_t p0 = b + k * kVqChunk, p1 = p0 + kVqChunk < b + len ? p0 + kVqChunk : b + len;
        double s = 0.0;
        if (j < D) {
            int64_t p = p0 + wave;
            for (; p + 12 < p1; p += 16) {  // four rows in flight, added in order
                const float v0 = x[perm[p] * D + j], v1 = x[perm[p + 4] * D + j], v2 = x[perm[p + 8] * D + j], v3 = x[perm[p + 12] * D + j];
                s += (double)v0;
                s += (double)v1;
                s += (double)v2;
                s += (double)v3;
            }
            for (; p < p1; p += 4) s += (double)x[perm[p] * D + j];
        }
        __syncthreads();  // the previous chunk's partials are read
        ws[wave][lane] = s;
        __syncthreads();
        if (wave == 0 && j < D) {
            const double t = ((ws[0][lane] + ws[1][lane]) + ws[2][lane]) + ws[3][lane];
            if (n_chunks == 1) sums[(int64_t)c * D + j] = (float)t;
            else part[(2 * (p0 / kVqChunk) + (k == 0 ? 1 : 0)) * D + j] = t;
        }
    }
}

// ... and the cells of several chunks: their chunk totals in chunk order, rounded once.
__global__ __launch_bounds__(64) void vq_cell_fold_kernel(int64_t N, int D, const int64_t *__restrict__ start, const double *__restrict__ part,
                                                         float *__restrict__ sums) {
    const int c = blockIdx.x, j = blockIdx.y * kVqSlab + threadIdx.x;
    int64_t b = start[c], len = start[c + 1] - b;
    b = b < 0 ? 0 : b > N ? N : b;
    len = len < 0 ? 0 : len > N - b ? N - b : len;
    if (len <= kVqChunk || j >= D) return;
    double t = 0.0;
    for (int64_t p0 = b, k = 0; p0 < b + len; p0 += kVqChunk, ++k) t += part[(2 * (p0 / kVqChunk) + (k == 0 ? 1 : 0)) * D + j];
    sums[(int64_t)c * D + j] = (float)t;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
// The slack's constants: eps(row, cell) = c_rel (|x|^2 + |c|^2) + c_abs, u = 2^-24, n_l = ceil(D / 64) the
// terms of a lane's chain in |c|^2.  3 D: the MFMA chain (D + 1) and twice the sequential chain (D + 2), both against S = |x|^2 + |c|^2.
static void vq_slack(int64_t D, float *c_rel, float *c_abs) {
    const double u = 5.9604644775390625e-08, nl = (double)((D + 63) / 64);
    *c_rel = (float)(1.05 * u * (3.0 * (double)D + nl + 24.0));
    *c_abs = 1e-30f;
}

// Workspace: u32 counter (16 bytes) | cn f32 [C] | ec f32 [C] | list i32 [N]
struct VqWs {
    uint32_t *counter;
    float *cn, *ec;
    int32_t *list;
};
static size_t vq_round16(size_t n) { return (n + 15) & ~(size_t)15; }
static VqWs vq_carve(void *ws, int64_t C) {
    unsigned char *p = (unsigned char *)ws;
    VqWs w;
    w.counter = (uint32_t *)p;
    w.cn = (float *)(p + 16);
    w.ec = (float *)(p + 16 + vq_round16((size_t)C * 4));
    w.list = (int32_t *)(p + 16 + 2 * vq_round16((size_t)C * 4));
    return w;
}

static int vq_check_shape(int64_t N, int64_t D, int64_t C) {
    ANNLITE_REQUIRE(N >= 0 && N <= 0x7fffffff, "N = %lld out of range", (long long)N);
    ANNLITE_REQUIRE(D >= 1 && D <= kVqMaxDim, "D = %lld: 1 .. %lld", (long long)D, (long long)kVqMaxDim);
    ANNLITE_REQUIRE(C >= 1 && C <= kVqMaxC, "C = %lld: 1 .. %lld", (long long)C, (long long)kVqMaxC);
    return ANNLITE_OK;
}

}  // namespace annlite

using namespace annlite;

extern "C" int annlite_vq_assign_slack(int64_t D, float *c_rel, float *c_abs) {
    ANNLITE_REQUIRE(c_rel && c_abs && D >= 1 && D <= kVqMaxDim, "bad argument");
    vq_slack(D, c_rel, c_abs);
    return ANNLITE_OK;
}

extern "C" int annlite_vq_assign_workspace_bytes(int64_t N, int64_t D, int64_t C, int64_t *bytes) {
    ANNLITE_REQUIRE(bytes, "null pointer");
    if (int rc = vq_check_shape(N, D, C)) return rc;
    *bytes = (int64_t)(16 + 2 * vq_round16((size_t)C * 4) + vq_round16((size_t)N * 4));
    return ANNLITE_OK;
}

extern "C" int annlite_vq_assign(const float *rows_dev, int64_t N, int64_t D, const float *centroids_dev, int64_t C, int32_t *cells_dev,
                                 void *workspace_dev, void *stream) {
    if (int rc = vq_check_shape(N, D, C)) return rc;
    ANNLITE_REQUIRE(centroids_dev && workspace_dev && (N == 0 || (rows_dev && cells_dev)), "null pointer");
    ANNLITE_REQUIRE((uintptr_t)workspace_dev % 16 == 0, "workspace not 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const VqWs w = vq_carve(workspace_dev, C);
    float c_rel, c_abs;
    vq_slack(D, &c_rel, &c_abs);
    hipLaunchKernelGGL(vq_norms_kernel, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, st, centroids_dev, (int)C, (int)D, c_rel, c_abs, w.cn, w.ec,
                       w.counter);
    if (int rc = launch_status("vq_norms_kernel")) return rc;
    if (N == 0) return ANNLITE_OK;
    const dim3 grid((unsigned)((N + kVqTile - 1) / kVqTile));
    const bool vec = D % 4 == 0 && ((uintptr_t)rows_dev % 16 == 0) && ((uintptr_t)centroids_dev % 16 == 0);
    if (vec)
        hipLaunchKernelGGL(vq_assign_kernel<true>, grid, dim3(256), 0, st, rows_dev, N, (int)D, centroids_dev, (int)C, w.cn, w.ec, c_rel, cells_dev,
                           w.counter, w.list);
    else
        hipLaunchKernelGGL(vq_assign_kernel<false>, grid, dim3(256), 0, st, rows_dev, N, (int)D, centroids_dev, (int)C, w.cn, w.ec, c_rel, cells_dev,
                           w.counter, w.list);
    if (int rc = launch_status("vq_assign_kernel")) return rc;
    // the worst case is every row; the groups walk the list by the grid's stride and leave on the counter
    const int64_t groups = (N + kVqRestRows - 1) / kVqRestRows;
    const dim3 rgrid((unsigned)(groups < 2048 ? groups : 2048));
    if (D <= kVqRestLdsDim) {
        const size_t lds = (size_t)kVqRestRows * D * 4;
        ANNLITE_HIP_TRY(hipFuncSetAttribute((const void *)vq_assign_rest_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(vq_assign_rest_kernel<true>, rgrid, dim3(256), lds, st, rows_dev, (int)D, centroids_dev, (int)C, w.counter, w.list,
                           cells_dev);
    } else {
        hipLaunchKernelGGL(vq_assign_rest_kernel<false>, rgrid, dim3(256), 0, st, rows_dev, (int)D, centroids_dev, (int)C, w.counter, w.list,
                           cells_dev);
    }
    return launch_status("vq_assign_rest_kernel");
}

extern "C" int annlite_vq_assign_undecided(const void *workspace_dev, void *stream, int64_t *count) {
    ANNLITE_REQUIRE(workspace_dev && count, "null pointer");
    uint32_t v = 0;
    ANNLITE_HIP_TRY(hipMemcpyAsync(&v, workspace_dev, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
    ANNLITE_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    *count = (int64_t)v;
    return ANNLITE_OK;
}

// Workspace of the sums: start i64 [C + 1] | part f64 [2 (N / L + 1)][D]
extern "C" int annlite_vq_cell_sums_workspace_bytes(int64_t N, int64_t D, int64_t C, int64_t *bytes) {
    ANNLITE_REQUIRE(bytes, "null pointer");
    if (int rc = vq_check_shape(N, D, C)) return rc;
    *bytes = (int64_t)(vq_round16((size_t)(C + 1) * 8) + (size_t)(2 * (N / kVqChunk + 1)) * D * 8);
    return ANNLITE_OK;
}

extern "C" int annlite_vq_cell_sums(const float *rows_dev, int64_t N, int64_t D, const int32_t *sorted_cells_dev, const int64_t *perm_dev,
                                    int64_t C, float *sums_dev, int32_t *counts_dev, void *workspace_dev, void *stream) {
    if (int rc = vq_check_shape(N, D, C)) return rc;
    ANNLITE_REQUIRE(sums_dev && counts_dev && workspace_dev && (N == 0 || (rows_dev && sorted_cells_dev && perm_dev)), "null pointer");
    ANNLITE_REQUIRE((uintptr_t)workspace_dev % 16 == 0, "workspace not 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    int64_t *start = (int64_t *)workspace_dev;
    double *part = (double *)((unsigned char *)workspace_dev + vq_round16((size_t)(C + 1) * 8));
    hipLaunchKernelGGL(vq_cell_bounds_kernel, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, st, sorted_cells_dev, N, (int)C, start);
    if (int rc = launch_status("vq_cell_bounds_kernel")) return rc;
    // chunk slots: as many as the longest possible cell has chunks, within ~64 k workgroups per slab; a slot walks its cell's chunks
    const int64_t slabs = (D + kVqSlab - 1) / kVqSlab, max_chunks = (N + kVqChunk - 1) / kVqChunk;
    int64_t z = 65536 / C;
    z = z < 1 ? 1 : z > 32 ? 32 : z;
    z = z > max_chunks ? (max_chunks > 0 ? max_chunks : 1) : z;
    hipLaunchKernelGGL(vq_cell_sums_kernel, dim3((unsigned)C, (unsigned)slabs, (unsigned)z), dim3(256), 0, st, rows_dev, N, (int)D, perm_dev, start,
                       sums_dev, counts_dev, part);
    if (int rc = launch_status("vq_cell_sums_kernel")) return rc;
    if (N > kVqChunk) {
        hipLaunchKernelGGL(vq_cell_fold_kernel, dim3((unsigned)C, (unsigned)slabs), dim3(64), 0, st, N, (int)D, start, part, sums_dev);
        return launch_status("vq_cell_fold_kernel");
    }
    return ANNLITE_OK;
}
