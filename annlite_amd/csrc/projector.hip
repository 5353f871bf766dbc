// projector.hip -- the PCA projector in front of every index.
//
// The reference's ProjectorCodec (annlite/core/codec/projector.py) wraps sklearn: PCA.fit / IncrementalPCA.partial_fit to train,
// PCA.transform / inverse_transform to use.  Here both halves that touch the rows run on the device:
//   annlite_affine_rows     out = (x - sub) M^T + add: transform (M = W, sub = mean) and inverse transform (M = W^T, add = mean)
//   annlite_pca_accumulate  sum (x - s) and sum (x - s)(x - s)^T over a batch into f64 accumulators: the whole of a fit but the
//                           eigen-decomposition of the D x D matrix, which the host does once per fit
// Both products run on v_mfma_f32_32x32x2_f32 -- a k-ordered f32 fma chain per output element -- in the 128 x 128 x 32 tiles of
// flat_filter_kernel (flat.hip).
#include <type_traits>

#include "common.h"

namespace annlite {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kProjTile = 128;           // rows x outputs of a workgroup tile (4 waves, 64 x 64 each: 2 x 2 MFMA tiles of 32 x 32)
constexpr int kProjDepth = 32;           // reduction steps per LDS stage
constexpr int kProjLd = kProjDepth + 1;  // affine: LDS row pitch in floats (33: the 32 rows of one MFMA operand on 32 banks)
constexpr int kPcaChunk = 512;           // rows of one partial product (a constant: the summation order is the same on every device)
constexpr int kPcaPass = 16;             // chunks whose partials the workspace holds at a time
constexpr int64_t kPcaMaxDim = 2048;
constexpr int64_t kAffineSmallTiles = 512;  // fewer (128-row tile, output tile) pairs than this: affine_rows uses 32-row tiles

// ---- out[r][o] = sum_k (x[r][k] - sub[k]) M[o][k] + add[o] -----------------------------------------------------------------------
// A workgroup keeps ONE row tile and walks the output tiles blockIdx.y, blockIdx.y + gridDim.y, ...: x streams from HBM once, M
// (Dout x Din floats) stays in L2.  Operands as in flat_filter_kernel: A = rows (lane l: row l & 31, step l >> 5), B = rows of M
// (lane l: step l >> 5, output l & 31); C/D: output = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) -- a register's 32
// lanes store 32 consecutive floats of one output row.  `sub` is subtracted as the tile is staged (one rounding per element, before
// any product): a common offset of the rows never enters the sums.
// The next stage's global loads are issued into registers before the current stage's MFMAs and stored to LDS after them: the loads'
// latency hides behind the products.
// RT = rows of the workgroup tile: 128 (the 4 waves 2 x 2, 64 rows x 64 outputs each: 2 x 2 MFMA tiles) or, for a batch too small to
// fill the chip with such tiles, 32 (the 4 waves side by side, 32 rows x 32 outputs each).  An output element is the same fma chain in
// both: the choice cannot change a bit of the result.
template <bool VEC, int RT>
__global__ __launch_bounds__(256) void affine_rows_kernel(const float *__restrict__ x, int64_t n, int Din, int64_t ldx,
                                                         const float *__restrict__ M, int Dout, const float *__restrict__ sub,
                                                         const float *__restrict__ add, float *__restrict__ out, int64_t ldo, int n_otiles) {
    static_assert(RT == 128 || RT == 32, "row tile");
    constexpr int MT = RT == 128 ? 2 : 1;                      // MFMA tiles per wave, in rows and in outputs
    constexpr int NA = (VEC ? RT * 8 : RT * 32) / 256;         // staging slots per thread: rows (f32x4 or float each)
    constexpr int NB = (VEC ? kProjTile * 8 : kProjTile * 32) / 256;  // ... rows of M
    typedef typename std::conditional<VEC, f32x4, float>::type slot_t;
    __shared__ float As[RT * kProjLd];
    __shared__ float Bs[kProjTile * kProjLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * RT;
    const int wr = RT == 128 ? (wave >> 1) * 64 : 0, wo = RT == 128 ? (wave & 1) * 64 : wave * 32;
    const int l31 = lane & 31, lh = lane >> 5;
    for (int ot = blockIdx.y; ot < n_otiles; ot += gridDim.y) {
        const int o0 = ot * kProjTile;
        slot_t ra[NA], rb[NB];
        auto load = [&](int k0) {
            if constexpr (VEC) {
#pragma unroll
                for (int i = 0; i < NB; ++i) {
                    const int e = tid + i * 256;  // slots of 4 floats: 8 per row
                    const int r = e >> 3, c = (e & 7) * 4;
                    if (i < NA) {
                        f32x4 va = {0.f, 0.f, 0.f, 0.f};
                        const int64_t rr = r0 + r;
                        if (rr < n && k0 + c < Din) {  // (Din % 4 == 0: the four floats are inside the row)
                            va = *(const f32x4 *)(x + rr * ldx + k0 + c);
                            if (sub) {
#pragma unroll
                                for (int t = 0; t < 4; ++t) va[t] -= sub[k0 + c + t];
                            }
                        }
                        ra[i < NA ? i : 0] = va;
                    }
                    f32x4 vb = {0.f, 0.f, 0.f, 0.f};
                    const int oo = o0 + r;
                    if (oo < Dout && k0 + c < Din) vb = *(const f32x4 *)(M + (int64_t)oo * Din + k0 + c);
                    rb[i] = vb;
                }
            } else {
#pragma unroll
                for (int i = 0; i < NB; ++i) {
                    const int e = tid + i * 256;  // floats: 32 per row
                    const int r = e >> 5, c = e & 31;
                    if (i < NA) {
                        const int64_t rr = r0 + r;
                        float va = 0.f;
                        if (rr < n && k0 + c < Din) {
                            va = x[rr * ldx + k0 + c];
                            if (sub) va -= sub[k0 + c];
                        }
                        ra[i < NA ? i : 0] = va;
                    }
                    const int oo = o0 + r;
                    rb[i] = (oo < Dout && k0 + c < Din) ? M[(int64_t)oo * Din + k0 + c] : 0.f;
                }
            }
        };
        auto store = [&]() {
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int e = tid + i * 256;
                if constexpr (VEC) {
                    const int r = e >> 3, c = (e & 7) * 4;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        if (i < NA) As[r * kProjLd + c + t] = ra[i < NA ? i : 0][t];
                        Bs[r * kProjLd + c + t] = rb[i][t];
                    }
                } else {
                    const int r = e >> 5, c = e & 31;
                    if (i < NA) As[r * kProjLd + c] = ra[i < NA ? i : 0];
                    Bs[r * kProjLd + c] = rb[i];
                }
            }
        };
        f32x16 acc[MT][MT];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        load(0);
        for (int k0 = 0; k0 < Din; k0 += kProjDepth) {
            __syncthreads();  // the previous stage is consumed
            store();
            __syncthreads();
            if (k0 + kProjDepth < Din) load(k0 + kProjDepth);
#pragma unroll
            for (int kk = 0; kk < kProjDepth; kk += 2) {
                const int kc = kk + lh;
                float a[MT], b[MT];
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    a[i] = As[(wr + 32 * i + l31) * kProjLd + kc];
                    b[i] = Bs[(wo + 32 * i + l31) * kProjLd + kc];
                }
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < MT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const int o = o0 + wo + j * 32 + l31;
            if (o >= Dout) continue;
            const float av = add ? add[o] : 0.f;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int64_t r = r0 + wr + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                    if (r < n) out[r * ldo + o] = add ? acc[i][j][reg] + av : acc[i][j][reg];
                }
            }
        }
    }
}

// ---- the fit: per (chunk of rows, tile pair) the f32 partial of sum_r (x[r][i] - s[i]) (x[r][j] - s[j]) ----------------------------
// The reduction runs over ROWS, so a stage is kProjDepth rows x 128 columns of each of the two column tiles, kept as it lies in
// memory: [row][column], pitch 128.  An MFMA operand (lane l: column l & 31, row l >> 5) then reads 32 consecutive floats per half
// wave -- no bank conflict, no padding -- and the staging stores are contiguous 16-byte writes.  (The filter's [item][step] layout
// with pitch 33 would need the tile transposed on the way in.)  A = columns of tile ti, B = columns of tile tj >= ti.
// Workgroup (t, c): tile pair t of chunk c of this pass.  Every element of the partial is ONE fma chain over the chunk's rows in
// ascending order: a function of the rows and of kPcaChunk alone.  The diagonal pairs also leave the chunk's column sums
// (sequential f32 over the rows, one thread per column).
__device__ __forceinline__ void pca_pair(int t, int T, int &ti, int &tj) {
    int i = 0;
    while (t >= T - i) {
        t -= T - i;
        ++i;
    }
    ti = i;
    tj = i + t;
}

template <bool VEC>
__global__ __launch_bounds__(256) void pca_partial_kernel(const float *__restrict__ x, int64_t n, int D, int64_t ldx, const float *__restrict__ s,
                                                         int64_t row0, int T, int n_pairs, float *__restrict__ part,
                                                         float *__restrict__ part_sum) {
    __shared__ __attribute__((aligned(16))) float As[kProjDepth * kProjTile];
    __shared__ __attribute__((aligned(16))) float Bs[kProjDepth * kProjTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int ti, tj;
    pca_pair((int)blockIdx.x, T, ti, tj);
    const int c = blockIdx.y;
    const int64_t rb = row0 + (int64_t)c * kPcaChunk;
    const int64_t re = rb + kPcaChunk < n ? rb + kPcaChunk : n;
    const int i0 = ti * kProjTile, j0 = tj * kProjTile;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    const int l31 = lane & 31, lh = lane >> 5;
    f32x16 acc00, acc01, acc10, acc11;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc00[e] = acc01[e] = acc10[e] = acc11[e] = 0.f;
    float colsum = 0.f;
    // the next stage's rows are loaded into registers before this stage's MFMAs and stored to LDS after them
    constexpr int NS = VEC ? 4 : 16;  // staging slots per thread and tile (f32x4 or float each)
    typedef typename std::conditional<VEC, f32x4, float>::type slot_t;
    slot_t ra[NS], rb_[NS];
    auto load = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int e = tid + i * 256;
            if constexpr (VEC) {  // 1024 slots of 4 floats
                const int r = e >> 5, cc = (e & 31) * 4;
                f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
                const int64_t rr = k0 + r;
                if (rr < re && i0 + cc < D) {  // (D % 4 == 0: the four floats are inside the row)
                    va = *(const f32x4 *)(x + rr * ldx + i0 + cc);
#pragma unroll
                    for (int u = 0; u < 4; ++u) va[u] -= s[i0 + cc + u];
                }
                if (rr < re && j0 + cc < D) {
                    vb = *(const f32x4 *)(x + rr * ldx + j0 + cc);
#pragma unroll
                    for (int u = 0; u < 4; ++u) vb[u] -= s[j0 + cc + u];
                }
                ra[i] = va;
                rb_[i] = vb;
            } else {  // 4096 floats
                const int r = e >> 7, cc = e & 127;
                const int64_t rr = k0 + r;
                ra[i] = (rr < re && i0 + cc < D) ? x[rr * ldx + i0 + cc] - s[i0 + cc] : 0.f;
                rb_[i] = (rr < re && j0 + cc < D) ? x[rr * ldx + j0 + cc] - s[j0 + cc] : 0.f;
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int e = tid + i * 256;
            if constexpr (VEC) {
                const int r = e >> 5, cc = (e & 31) * 4;
                *(f32x4 *)(As + r * kProjTile + cc) = ra[i];
                *(f32x4 *)(Bs + r * kProjTile + cc) = rb_[i];
            } else {
                const int r = e >> 7, cc = e & 127;
                As[r * kProjTile + cc] = ra[i];
                Bs[r * kProjTile + cc] = rb_[i];
            }
        }
    };
    if (rb < re) load(rb);
    for (int64_t k0 = rb; k0 < re; k0 += kProjDepth) {
        __syncthreads();  // the previous stage is consumed
        store();
        __syncthreads();
        if (k0 + kProjDepth < re) load(k0 + kProjDepth);
        if (ti == tj && tid < kProjTile) {
#pragma unroll 8
            for (int r = 0; r < kProjDepth; ++r) colsum += As[r * kProjTile + tid];  // (rows past the chunk's end are staged as 0)
        }
#pragma unroll
        for (int kk = 0; kk < kProjDepth; kk += 2) {
            const int kr = (kk + lh) * kProjTile;
            const float a0 = As[kr + wi + l31], a1 = As[kr + wi + 32 + l31];
            const float b0 = Bs[kr + wj + l31], b1 = Bs[kr + wj + 32 + l31];
            acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
        }
    }
    float *pt = part + ((int64_t)c * n_pairs + blockIdx.x) * (kProjTile * kProjTile);
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int jl = wj + jj * 32 + l31;
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) {
            const f32x16 &acc = ii == 0 ? (jj == 0 ? acc00 : acc01) : (jj == 0 ? acc10 : acc11);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int il = wi + ii * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                pt[il * kProjTile + jl] = acc[reg];
            }
        }
    }
    if (ti == tj && tid < kProjTile) part_sum[(int64_t)c * T * kProjTile + i0 + tid] = colsum;
}

// ---- ... folded into the caller's f64 accumulators in chunk order: one thread per element, no atomics ------------------------------
// gram[i][j] (tile pair t: i in tile ti, j in tile tj) takes its chunks' partials one after the other; below the diagonal tiles the
// result is mirrored (inside a diagonal tile (i, j) and (j, i) are the same chain with the factors swapped: equal bits already).
__global__ __launch_bounds__(256) void pca_fold_kernel(const float *__restrict__ part, const float *__restrict__ part_sum, int n_chunks, int D,
                                                      int T, int n_pairs, double *__restrict__ gram, double *__restrict__ sum) {
    const int t = blockIdx.x;
    if (t == n_pairs) {  // the last block row: the column sums
        const int i = blockIdx.y * 256 + threadIdx.x;
        if (i >= D) return;
        double a = sum[i];
        for (int c = 0; c < n_chunks; ++c) a += (double)part_sum[(int64_t)c * T * kProjTile + i];
        sum[i] = a;
        return;
    }
    int ti, tj;
    pca_pair(t, T, ti, tj);
    const int e = blockIdx.y * 256 + threadIdx.x;  // element of the tile (gridDim.y = 64)
    const int il = e >> 7, jl = e & 127;
    const int i = ti * kProjTile + il, j = tj * kProjTile + jl;
    if (i >= D || j >= D) return;
    double a = gram[(int64_t)i * D + j];
    for (int c = 0; c < n_chunks; ++c) a += (double)part[((int64_t)c * n_pairs + t) * (kProjTile * kProjTile) + e];
    gram[(int64_t)i * D + j] = a;
    if (ti != tj) gram[(int64_t)j * D + i] = a;
}

struct PcaWs {
    float *part, *part_sum;
    int T, n_pairs;
    size_t bytes;
};
static PcaWs pca_carve(void *ws, int64_t n, int64_t D) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    PcaWs w;
    w.T = (int)((D + kProjTile - 1) / kProjTile);
    w.n_pairs = w.T * (w.T + 1) / 2;
    int64_t chunks = (n + kPcaChunk - 1) / kPcaChunk;
    if (chunks > kPcaPass) chunks = kPcaPass;
    char *p = (char *)ws;
    size_t o = 0;
    w.part = (float *)(p + o), o += up((size_t)chunks * w.n_pairs * kProjTile * kProjTile * 4);
    w.part_sum = (float *)(p + o), o += up((size_t)chunks * w.T * kProjTile * 4);
    w.bytes = o;
    return w;
}

}  // namespace annlite

using namespace annlite;

extern "C" int annlite_affine_rows(const float *x_dev, int64_t n, int64_t Din, int64_t ldx, const float *M_dev, int64_t Dout,
                                   const float *sub_dev, const float *add_dev, float *out_dev, int64_t ldo, void *stream) {
    ANNLITE_REQUIRE(n >= 0 && Din >= 1 && Dout >= 1 && Din <= INT32_MAX && Dout <= INT32_MAX - kProjTile, "bad shape");
    ANNLITE_REQUIRE(ldx >= Din && ldo >= Dout, "row stride below the row length");
    if (n == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(x_dev && M_dev && out_dev, "null device pointer");
    const int n_ot = (int)((Dout + kProjTile - 1) / kProjTile);
    // tiles of 128 rows while there are enough of them to fill the chip; a smaller batch -- one search's queries -- in tiles of 32.
    // (A constant, not the device's CU count: which kernel serves a shape is a property of the shape.)
    const bool small = (n + kProjTile - 1) / kProjTile * n_ot < kAffineSmallTiles;
    const int rt = small ? 32 : kProjTile;
    const int64_t n_rt = (n + rt - 1) / rt;
    ANNLITE_REQUIRE(n_rt <= INT32_MAX, "too many rows");
    int64_t ny = (4 * (int64_t)device_cu_count() + n_rt - 1) / n_rt;  // few row tiles: spread the output tiles too
    ny = ny < 1 ? 1 : ny > n_ot ? n_ot : ny;
    if (ny > 65535) ny = 65535;
    const dim3 grid((unsigned)n_rt, (unsigned)ny);
    const bool vec = Din % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)x_dev % 16 == 0) && ((uintptr_t)M_dev % 16 == 0);
#define ANNLITE_AFFINE_LAUNCH(V, R)                                                                                                    \
    hipLaunchKernelGGL((affine_rows_kernel<V, R>), grid, dim3(256), 0, (hipStream_t)stream, x_dev, n, (int)Din, ldx, M_dev, (int)Dout, \
                       sub_dev, add_dev, out_dev, ldo, n_ot)
    if (vec && small)
        ANNLITE_AFFINE_LAUNCH(true, 32);
    else if (vec)
        ANNLITE_AFFINE_LAUNCH(true, 128);
    else if (small)
        ANNLITE_AFFINE_LAUNCH(false, 32);
    else
        ANNLITE_AFFINE_LAUNCH(false, 128);
#undef ANNLITE_AFFINE_LAUNCH
    return launch_status("affine_rows_kernel");
}

extern "C" int annlite_pca_accumulate_workspace_bytes(int64_t n, int64_t D, int64_t *bytes) {
    ANNLITE_REQUIRE(n >= 0 && D >= 1 && D <= kPcaMaxDim && bytes, "bad argument (1 <= D <= 2048)");
    *bytes = (int64_t)pca_carve(nullptr, n, D).bytes;
    return ANNLITE_OK;
}

extern "C" int annlite_pca_accumulate(const float *x_dev, int64_t n, int64_t D, int64_t ldx, const float *shift_dev, double *sum_dev,
                                      double *gram_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    ANNLITE_REQUIRE(n >= 0 && D >= 1 && D <= kPcaMaxDim, "bad shape (1 <= D <= 2048)");
    ANNLITE_REQUIRE(ldx >= D, "row stride below the row length");
    if (n == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(x_dev && shift_dev && sum_dev && gram_dev && workspace_dev, "null device pointer");
    ANNLITE_REQUIRE((uintptr_t)workspace_dev % 16 == 0, "workspace not 16-byte aligned");
    const PcaWs w = pca_carve(workspace_dev, n, D);
    if (workspace_bytes < w.bytes) {
        set_error("workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
        return ANNLITE_ERR_WORKSPACE;
    }
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = D % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)x_dev % 16 == 0);
    const int64_t per_pass = (int64_t)kPcaPass * kPcaChunk;
    for (int64_t row0 = 0; row0 < n; row0 += per_pass) {
        const int64_t left = n - row0;
        const int chunks = (int)(((left < per_pass ? left : per_pass) + kPcaChunk - 1) / kPcaChunk);
        const dim3 grid((unsigned)w.n_pairs, (unsigned)chunks);
        if (vec)
            hipLaunchKernelGGL(pca_partial_kernel<true>, grid, dim3(256), 0, st, x_dev, n, (int)D, ldx, shift_dev, row0, w.T, w.n_pairs, w.part,
                               w.part_sum);
        else
            hipLaunchKernelGGL(pca_partial_kernel<false>, grid, dim3(256), 0, st, x_dev, n, (int)D, ldx, shift_dev, row0, w.T, w.n_pairs, w.part,
                               w.part_sum);
        int rc = launch_status("pca_partial_kernel");
        if (rc != ANNLITE_OK) return rc;
        hipLaunchKernelGGL(pca_fold_kernel, dim3((unsigned)w.n_pairs + 1, kProjTile * kProjTile / 256), dim3(256), 0, st, w.part, w.part_sum, chunks,
                           (int)D, w.T, w.n_pairs, gram_dev, sum_dev);
        rc = launch_status("pca_fold_kernel");
        if (rc != ANNLITE_OK) return rc;
    }
    return ANNLITE_OK;
}
