// bitmap_rows.hip -- the set bits of a bitmap as an ascending list of row offsets (annlite_bitmap_rows; DESIGN.md section 3.6,
// "selected rows"): what a filtered search over float vectors scans instead of the table.
//
// Three stream-ordered launches, the kernel boundary the only hand-over between workgroups:
//   count    a workgroup per kRowsBlockWords words: the set bits of its words, one number per workgroup
//   scan     ONE workgroup: the exclusive prefix sum of those numbers in place, the total to *out_n
//   scatter  the count's grid again: a thread's position = its workgroup's prefix + the set bits of the threads before it (a scan in the
//            workgroup), then it expands its words, lowest bit first
// A position depends on the words alone, never on the order of an atomic: the same input gives the same array.
#include "common.h"

namespace annlite {

constexpr int kRowsThreads = 256;
constexpr int kRowsWordsPerThread = 4;
constexpr int kRowsBlockWords = kRowsThreads * kRowsWordsPerThread;  // 1024 words = 32768 rows per workgroup
constexpr int kRowsScanThreads = 1024;

// The thread's words -- word base + j of workgroup blockIdx.x, consecutive per thread so that its rows ascend --, ANDed, rows >= N cleared.
// Nothing at or behind word ceil(N / 32) is read.
__device__ __forceinline__ int64_t rows_load(const uint32_t *__restrict__ bits, const uint32_t *__restrict__ and_bits, int64_t N,
                                             uint32_t (&w)[kRowsWordsPerThread]) {
    const int64_t first = (int64_t)blockIdx.x * kRowsBlockWords + (int64_t)threadIdx.x * kRowsWordsPerThread;
#pragma unroll
    for (int j = 0; j < kRowsWordsPerThread; ++j) {
        const int64_t left = N - (first + j) * 32;  // rows from the word's first one on
        uint32_t v = 0;
        if (left > 0) {
            v = bits[first + j];
            if (and_bits) v &= and_bits[first + j];
            if (left < 32) v &= (1u << left) - 1u;
        }
        w[j] = v;
    }
    return first;
}

// exclusive prefix of `mine` over the workgroup's threads; *total (every thread): the workgroup's sum.  s_wave: one slot per wave.
template <int THREADS>
__device__ __forceinline__ uint32_t rows_block_scan(uint32_t mine, uint32_t *s_wave, uint32_t *total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (int v = 0; v < THREADS / kWave; ++v) {
        const uint32_t t = s_wave[v];
        if (v < wave) before += t;
        sum += t;
    }
    __syncthreads();  // (s_wave may be written again)
    *total = sum;
    return before + incl - mine;
}

__global__ __launch_bounds__(kRowsThreads) void bitmap_rows_count_kernel(const uint32_t *__restrict__ bits, const uint32_t *__restrict__ and_bits,
                                                                         int64_t N, uint32_t *__restrict__ block_counts) {
    __shared__ uint32_t s_wave[kRowsThreads / kWave];
    uint32_t w[kRowsWordsPerThread];
    rows_load(bits, and_bits, N, w);
    uint32_t mine = 0, total;
#pragma unroll
    for (int j = 0; j < kRowsWordsPerThread; ++j) mine += __popc(w[j]);
    rows_block_scan<kRowsThreads>(mine, s_wave, &total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// one workgroup: block_counts[0 .. n_blocks) becomes its exclusive prefix sum (a total below 2^31: N is), *out_n the total
__global__ __launch_bounds__(kRowsScanThreads) void bitmap_rows_scan_kernel(uint32_t *__restrict__ block_counts, int64_t n_blocks,
                                                                            int64_t *__restrict__ out_n) {
    __shared__ uint32_t s_wave[kRowsScanThreads / kWave];
    uint32_t carry = 0;
    for (int64_t i0 = 0; i0 < n_blocks; i0 += kRowsScanThreads) {  // (uniform trip count: the barriers inside are reached by all)
        const int64_t i = i0 + threadIdx.x;
        const uint32_t c = i < n_blocks ? block_counts[i] : 0u;
        uint32_t total;
        const uint32_t excl = rows_block_scan<kRowsScanThreads>(c, s_wave, &total);
        if (i < n_blocks) block_counts[i] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) *out_n = (int64_t)carry;
}

__global__ __launch_bounds__(kRowsThreads) void bitmap_rows_scatter_kernel(const uint32_t *__restrict__ bits, const uint32_t *__restrict__ and_bits,
                                                                           int64_t N, const uint32_t *__restrict__ block_offsets,
                                                                           int32_t *__restrict__ out_rows, int64_t out_capacity) {
    __shared__ uint32_t s_wave[kRowsThreads / kWave];
    uint32_t w[kRowsWordsPerThread];
    const int64_t first = rows_load(bits, and_bits, N, w);
    uint32_t mine = 0, total;
#pragma unroll
    for (int j = 0; j < kRowsWordsPerThread; ++j) mine += __popc(w[j]);
    const uint32_t excl = rows_block_scan<kRowsThreads>(mine, s_wave, &total);
    int64_t pos = (int64_t)block_offsets[blockIdx.x] + excl;
#pragma unroll
    for (int j = 0; j < kRowsWordsPerThread; ++j) {
        uint32_t v = w[j];
        while (v) {
            if (pos >= out_capacity) return;  // (positions only grow: nothing of this thread's is left to write)
            out_rows[pos++] = (int32_t)((first + j) * 32 + __builtin_ctz(v));
            v &= v - 1u;
        }
    }
}

static int64_t bitmap_rows_blocks(int64_t N) {
    const int64_t words = (N + 31) / 32;
    const int64_t nb = (words + kRowsBlockWords - 1) / kRowsBlockWords;
    return nb < 1 ? 1 : nb;
}

}  // namespace annlite

using namespace annlite;

extern "C" int annlite_bitmap_rows_workspace_bytes(int64_t N, int64_t *bytes) {
    ANNLITE_REQUIRE(bytes != nullptr, "bytes is NULL");
    ANNLITE_REQUIRE(N >= 0 && N <= INT32_MAX, "bad N=%lld (0 <= N < 2^31)", (long long)N);
    *bytes = (bitmap_rows_blocks(N) * 4 + 255) & ~(int64_t)255;
    return ANNLITE_OK;
}

extern "C" int annlite_bitmap_rows(const uint32_t *bits_dev, const uint32_t *and_bits_dev, int64_t N, int64_t n_words, int32_t *out_rows_dev,
                                   int64_t out_capacity, int64_t *out_n_dev, void *workspace, size_t workspace_bytes, void *stream) {
    ANNLITE_REQUIRE(N >= 0 && N <= INT32_MAX && n_words >= 0 && n_words <= (INT64_MAX >> 5) && n_words * 32 >= N,
                    "bad N=%lld n_words=%lld (0 <= N < 2^31, n_words * 32 >= N)", (long long)N, (long long)n_words);
    ANNLITE_REQUIRE(out_capacity >= 0 && (out_capacity == 0 || out_rows_dev != nullptr), "bad out_capacity=%lld / out_rows_dev", (long long)out_capacity);
    ANNLITE_REQUIRE(out_n_dev != nullptr && (N == 0 || bits_dev != nullptr), "out_n_dev / bits_dev is NULL");
    const int64_t nb = bitmap_rows_blocks(N);
    ANNLITE_REQUIRE(workspace != nullptr && workspace_bytes >= (size_t)nb * 4 && (uintptr_t)workspace % 4 == 0,
                    "workspace: %zu bytes at %p (annlite_bitmap_rows_workspace_bytes)", workspace_bytes, workspace);
    hipStream_t st = (hipStream_t)stream;
    uint32_t *counts = (uint32_t *)workspace;
    hipLaunchKernelGGL(bitmap_rows_count_kernel, dim3((unsigned)nb), dim3(kRowsThreads), 0, st, bits_dev, and_bits_dev, N, counts);
    hipLaunchKernelGGL(bitmap_rows_scan_kernel, dim3(1), dim3(kRowsScanThreads), 0, st, counts, nb, out_n_dev);
    if (out_capacity > 0)
        hipLaunchKernelGGL(bitmap_rows_scatter_kernel, dim3((unsigned)nb), dim3(kRowsThreads), 0, st, bits_dev, and_bits_dev, N, counts, out_rows_dev,
                           out_capacity);
    return launch_status("bitmap_rows kernels");
}
