// page.hip -- pages of the document listing (AnnLite.filter / get_docs): the rows of a bitmap whose rank in the host's order lies in
// [first, first + count), by MSB radix select (annlite_order_page, annlite_bitmap_page).
//
// Every selected row has a COMPOSITE of 13 digits of 8 bits, most significant first:
//     digit 0        the class: 0 / 1 puts the rows without a value of the column (NULL) first ascending, last descending;
//     digits 1 .. 8  the key: the column's value as a u64 whose unsigned order is Python's order of the values (page_key), ~key
//                    descending, 0 for a NULL row;
//     digits 9 .. 12 the row.
// Composites are distinct, and their ascending order is the host's order (Python's stable `sorted`, NULLs before or behind).  The page is
// the rows of composite rank [a, b), a = first, b = min(first + count, total):
//   * one launch per digit that can differ between rows (the host lists them: a dictionary column's key has 1 or 2, the row has
//     ceil(log256 N)): every workgroup counts, in LDS, the digit of the rows that agree with rank a's digits so far, and with rank
//     (b - 1)'s where the two have parted, and adds its non-zero bins to the pass's table in global memory;
//   * the NEXT launch's workgroups each read that table (256 bins: a prefix sum in one wave) and derive the digit and the rank that
//     remains -- the hand-over between workgroups is the kernel boundary, nothing else; workgroup 0 leaves the derived state for the
//     launch after it.  The first table also holds the total, which clamps a and b;
//   * a collect launch derives the last digit, hence V_a and V_(b-1), and appends the rows with V_a <= composite <= V_(b-1) -- exactly
//     b - a of them -- in any order; one workgroup sorts them in LDS and writes the page.  What comes out depends on no atomic's order.
// The unordered page is the same select over the row digits alone.
#include "common.h"

namespace annlite {

constexpr int kPageThreads = 256;
constexpr int kPageRowsPerThread = ANNLITE_PAGE_BLOCK_ROWS / kPageThreads;
constexpr int kPageDigits = 13;
constexpr int kPageSortThreads = 1024;
constexpr int kPageKindNone = -1;  // (no column: class 0, key 0 -- the unordered page)
static_assert(ANNLITE_PAGE_BLOCK_ROWS % kPageThreads == 0, "whole rows per thread");

typedef unsigned __int128 u128;

// what a launch knows of the two ranks: their digits so far (the others 0) and the rank that remains among the rows that share them
struct PageState {
    uint64_t a_hi, a_lo, b_hi, b_lo;  // the composites of rank a and rank b - 1
    uint32_t ra, rb;
    uint32_t same;  // the two still share every digit derived
    uint32_t n;     // rows of the page (0: nothing to select, every later launch returns at once)
};

struct PageWorkspace {
    uint32_t tables[kPageDigits][2][256];  // per pass: the counts by digit for rank a, for rank b - 1   } zeroed per call
    uint32_t appended;                     // slots taken by the collect                                  }
    uint32_t pad[3];
    PageState states[kPageDigits + 1];  // [s]: what pass s works with, s = 1 ..; [n_passes]: the collect's, read by the sort
    uint64_t keys[ANNLITE_PAGE_MAX];    // the collected rows: key,
    uint32_t rows[ANNLITE_PAGE_MAX];    // ... class << 31 | row
};
constexpr size_t kPageZeroBytes = offsetof(PageWorkspace, pad);

struct PageArgs {
    const uint32_t *bits;      // the selection; never NULL
    const uint32_t *and_bits;  // ANDed with it where given
    const void *values;
    const uint32_t *present;
    const uint32_t *rank;  // dictionary columns: code -> rank
    uint32_t rank_len;
    uint32_t key_mask;  // dictionary columns: the bits of a key (descending: ~rank within them, so that the digits above stay 0)
    int kind;
    int descending;
    int64_t N;
    uint32_t first, count;
};

__device__ __forceinline__ u128 page_u128(uint64_t hi, uint64_t lo) { return ((u128)hi << 64) | lo; }
__device__ __forceinline__ u128 page_composite(uint32_t cls, uint64_t key, uint32_t row) { return ((u128)cls << 96) | ((u128)key << 32) | row; }
__device__ __forceinline__ uint32_t page_digit(u128 c, int d) { return (uint32_t)(c >> (96 - 8 * d)) & 0xffu; }
// the digits in front of digit d (d = 0: none, the shift is 104 and both sides are 0)
__device__ __forceinline__ bool page_shares(u128 c, u128 prefix, int d) { return ((c ^ prefix) >> (104 - 8 * d)) == 0; }

// The key of a value: unsigned order = Python's order.  Integer ops only (a subnormal double stays what it is).
__device__ __forceinline__ uint64_t page_key(const PageArgs &A, int64_t row) {
    uint64_t k;
    if (A.kind == ANNLITE_COL_I64) {
        k = ((const uint64_t *)A.values)[row] ^ 0x8000000000000000ull;
    } else if (A.kind == ANNLITE_COL_F64) {
        uint64_t u = ((const uint64_t *)A.values)[row];
        if ((u << 1) == 0) u = 0;  // -0.0 == 0.0: one key, the row decides
        k = u ^ ((uint64_t)((int64_t)u >> 63) | 0x8000000000000000ull);
    } else {
        const uint32_t code = (uint32_t)((const int32_t *)A.values)[row];
        k = code < A.rank_len ? A.rank[code] : 0u;  // (a code beyond the table: no read)
        return (A.descending ? ~k : k) & A.key_mask;
    }
    return A.descending ? ~k : k;
}

// The rows a thread takes per stride of its workgroup -- rows base + j * kPageThreads + thread --: which are selected, and their
// composites.  The bitmap words of all of them are loaded first, then the values of the selected ones: kPageRowsPerThread loads in
// flight per lane, not one word -> value chain after the other.
struct PageRows {
    u128 c[kPageRowsPerThread];
    bool sel[kPageRowsPerThread];
};
__device__ __forceinline__ void page_load(const PageArgs &A, int64_t base, PageRows &R) {
    uint32_t word[kPageRowsPerThread], pres[kPageRowsPerThread];
#pragma unroll
    for (int j = 0; j < kPageRowsPerThread; ++j) {
        const int64_t row = base + j * kPageThreads + threadIdx.x;
        word[j] = 0, pres[j] = 0;
        if (row < A.N) {  // (rows >= N: nothing is read)
            const int64_t w = row >> 5;
            word[j] = A.bits[w];
            if (A.and_bits) word[j] &= A.and_bits[w];
            if (A.kind != kPageKindNone) pres[j] = A.present[w];
        }
    }
#pragma unroll
    for (int j = 0; j < kPageRowsPerThread; ++j) {
        const int64_t row = base + j * kPageThreads + threadIdx.x;
        const bool sel = (word[j] >> (row & 31)) & 1u;
        const bool has = sel && ((pres[j] >> (row & 31)) & 1u);
        uint64_t key = 0;
        if (has) key = page_key(A, row);
        // NULLs: class 0 ascending, class 1 descending
        const uint32_t cls = A.kind == kPageKindNone ? 0u : (uint32_t)has ^ (uint32_t)(A.descending != 0);
        R.c[j] = page_composite(cls, key, (uint32_t)row);
        R.sel[j] = sel;
    }
}

// Waves 0 and 1 of the workgroup: rank a's and rank (b - 1)'s digit `d` from the table of the pass that counted it, into *out (LDS).
// `in` is the state that pass worked with; `first_pass`: it was the first, whose table holds every selected row -- the total clamps
// the ranks.  Ends with a barrier: every thread then reads *out.
__device__ void page_derive(const uint32_t (*table)[256], const PageState &in, int d, bool first_pass, const PageArgs &A, uint32_t (*s_t)[256],
                            PageState *out) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const bool same = in.same != 0;
    s_t[0][tid] = table[0][tid];
    s_t[1][tid] = table[same ? 0 : 1][tid];
    if (tid == 0) out->same = 1, out->n = in.n;
    __syncthreads();
    if (wave < 2) {
        const uint32_t *t = s_t[wave];
        const uint32_t c0 = t[4 * lane], c1 = t[4 * lane + 1], c2 = t[4 * lane + 2], c3 = t[4 * lane + 3];
        const uint32_t sum = c0 + c1 + c2 + c3;
        uint32_t incl = sum;
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        const uint32_t total = __shfl(incl, kWave - 1);
        uint32_t r = wave == 0 ? in.ra : in.rb;
        uint32_t n = in.n;
        if (first_pass) {
            const uint64_t end = (uint64_t)A.first + A.count;
            n = A.first < total ? (uint32_t)(end < total ? end : total) - A.first : 0u;
            r = wave == 0 ? A.first : A.first + n - 1;
            if (wave == 0 && lane == 0) out->n = n;
        }
        const uint32_t excl = incl - sum;
        if (n != 0 && excl <= r && r < incl) {  // (one lane: r < total)
            uint32_t digit = 4 * lane, before = excl;
            if (r >= before + c0) {
                before += c0, ++digit;
                if (r >= before + c1) {
                    before += c1, ++digit;
                    if (r >= before + c2) before += c2, ++digit;
                }
            }
            const u128 c = page_u128(wave == 0 ? in.a_hi : in.b_hi, wave == 0 ? in.a_lo : in.b_lo) | ((u128)digit << (96 - 8 * d));
            if (wave == 0) {
                out->a_hi = (uint64_t)(c >> 64), out->a_lo = (uint64_t)c, out->ra = r - before;
            } else {
                out->b_hi = (uint64_t)(c >> 64), out->b_lo = (uint64_t)c, out->rb = r - before;
            }
        }
    }
    __syncthreads();
    if (tid == 0) out->same = same && out->n != 0 && out->a_hi == out->b_hi && out->a_lo == out->b_lo;
    __syncthreads();
}

// the state a launch works with: the one before it derived nothing (pass 0), or what page_derive makes of the previous pass's table
__device__ __forceinline__ bool page_enter(PageWorkspace *ws, int s, int d_prev, const PageArgs &A, uint32_t (*s_t)[256], PageState *s_state) {
    if (s == 0) {
        if (threadIdx.x == 0) *s_state = PageState{0, 0, 0, 0, 0, 0, 1, 1};
        __syncthreads();
        return true;
    }
    PageState in = PageState{0, 0, 0, 0, 0, 0, 1, 1};
    if (s > 1) in = ws->states[s - 1];
    page_derive(ws->tables[s - 1], in, d_prev, s == 1, A, s_t, s_state);
    if (blockIdx.x == 0 && threadIdx.x == 0) ws->states[s] = *s_state;  // (every workgroup derives the same)
    return s_state->n != 0;
}

// += 1 in bin `digit` for the lanes with `mine`; one add for the wave where all of them hit one bin (a digit that is the same in
// every row -- the high bytes of small integers -- would otherwise be 64 adds to one address)
__device__ __forceinline__ void page_count(uint32_t *hist, bool mine, uint32_t digit, int lane) {
    const unsigned long long act = __ballot(mine);
    if (act == 0) return;
    const int lead = __builtin_ctzll(act);
    const uint32_t d0 = __builtin_amdgcn_readlane(digit, lead);
    if (__ballot(mine && digit == d0) == act) {
        if (lane == lead) atomicAdd(&hist[d0], (uint32_t)__popcll(act));
    } else if (mine) {
        atomicAdd(&hist[digit], 1u);
    }
}

// pass s: counts digit d of the rows that share the digits derived so far
__global__ __launch_bounds__(kPageThreads) void page_pass_kernel(const PageArgs A, PageWorkspace *__restrict__ ws, int s, int d, int d_prev) {
    __shared__ uint32_t s_t[2][256];
    __shared__ PageState s_state;
    if (!page_enter(ws, s, d_prev, A, s_t, &s_state)) return;  // (uniform)
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const u128 pa = page_u128(s_state.a_hi, s_state.a_lo), pb = page_u128(s_state.b_hi, s_state.b_lo);
    const bool same = s_state.same != 0;
    __syncthreads();  // (s_t is the histogram from here on)
    s_t[0][tid] = 0, s_t[1][tid] = 0;
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * ANNLITE_PAGE_BLOCK_ROWS; base < A.N; base += (int64_t)gridDim.x * ANNLITE_PAGE_BLOCK_ROWS) {
        PageRows R;
        page_load(A, base, R);
#pragma unroll
        for (int j = 0; j < kPageRowsPerThread; ++j) {
            const uint32_t digit = page_digit(R.c[j], d);
            page_count(s_t[0], R.sel[j] && page_shares(R.c[j], pa, d), digit, lane);
            if (!same) page_count(s_t[1], R.sel[j] && page_shares(R.c[j], pb, d), digit, lane);
        }
    }
    __syncthreads();
    if (s_t[0][tid]) atomicAdd(&ws->tables[s][0][tid], s_t[0][tid]);
    if (!same && s_t[1][tid]) atomicAdd(&ws->tables[s][1][tid], s_t[1][tid]);
}

// derives the last digit and appends the rows from V_a to V_(b-1)
__global__ __launch_bounds__(kPageThreads) void page_collect_kernel(const PageArgs A, PageWorkspace *__restrict__ ws, int s, int d_prev) {
    __shared__ uint32_t s_t[2][256];
    __shared__ PageState s_state;
    if (!page_enter(ws, s, d_prev, A, s_t, &s_state)) return;
    const u128 va = page_u128(s_state.a_hi, s_state.a_lo), vb = page_u128(s_state.b_hi, s_state.b_lo);
    for (int64_t base = (int64_t)blockIdx.x * ANNLITE_PAGE_BLOCK_ROWS; base < A.N; base += (int64_t)gridDim.x * ANNLITE_PAGE_BLOCK_ROWS) {
        PageRows R;
        page_load(A, base, R);
#pragma unroll
        for (int j = 0; j < kPageRowsPerThread; ++j) {
            const u128 c = R.c[j];
            if (R.sel[j] && va <= c && c <= vb) {
                const uint32_t slot = atomicAdd(&ws->appended, 1u);
                if (slot < ANNLITE_PAGE_MAX) {  // (b - a rows: composites are distinct)
                    ws->keys[slot] = (uint64_t)(c >> 32);
                    ws->rows[slot] = (uint32_t)c | ((uint32_t)(c >> 96) << 31);
                }
            }
        }
    }
}

__device__ __forceinline__ bool page_pair_less(uint64_t ka, uint32_t ra, uint64_t kb, uint32_t rb) {
    const uint32_t ca = ra >> 31, cb = rb >> 31;
    if (ca != cb) return ca < cb;
    if (ka != kb) return ka < kb;
    return ra < rb;
}

// one workgroup: the collected rows in composite order (a bitonic network in LDS over the next power of two)
__global__ __launch_bounds__(kPageSortThreads) void page_sort_kernel(const PageWorkspace *__restrict__ ws, int n_passes, int32_t *__restrict__ out_rows,
                                                                     int32_t *__restrict__ out_n) {
    __shared__ uint64_t s_key[ANNLITE_PAGE_MAX];
    __shared__ uint32_t s_row[ANNLITE_PAGE_MAX];
    const int tid = threadIdx.x;
    uint32_t n = ws->states[n_passes].n;
    if (n > ANNLITE_PAGE_MAX) n = ANNLITE_PAGE_MAX;  // (never: n <= count)
    if (tid == 0) *out_n = (int32_t)n;
    if (n == 0) return;
    uint32_t size = 2;
    while (size < n) size <<= 1;
    for (uint32_t i = tid; i < size; i += kPageSortThreads) {
        s_key[i] = i < n ? ws->keys[i] : ~0ull;
        s_row[i] = i < n ? ws->rows[i] : ~0u;  // (behind every row)
    }
    __syncthreads();
    for (uint32_t k = 2; k <= size; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < size / 2; t += kPageSortThreads) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const bool up = (i & k) == 0;
                const uint64_t ki = s_key[i], kp = s_key[p];
                const uint32_t ri = s_row[i], rp = s_row[p];
                if (page_pair_less(kp, rp, ki, ri) == up) {
                    s_key[i] = kp, s_key[p] = ki;
                    s_row[i] = rp, s_row[p] = ri;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < n; i += kPageSortThreads) out_rows[i] = (int32_t)(s_row[i] & 0x7fffffffu);
}

static int page_launch(const PageArgs &A, int n_key_digits, int32_t *out_rows_dev, int32_t *out_n_dev, void *workspace, int max_blocks,
                       hipStream_t stream) {
    // the digits that can differ between two rows, most significant first
    int digits[kPageDigits], n = 0;
    if (A.kind != kPageKindNone) digits[n++] = 0;
    for (int i = 0; i < n_key_digits; ++i) digits[n++] = 9 - n_key_digits + i;
    const int n_row_digits = A.N <= (1 << 8) ? 1 : A.N <= (1 << 16) ? 2 : A.N <= (1 << 24) ? 3 : 4;
    for (int i = 0; i < n_row_digits; ++i) digits[n++] = 13 - n_row_digits + i;

    PageWorkspace *ws = (PageWorkspace *)workspace;
    ANNLITE_HIP_TRY(hipMemsetAsync(ws, 0, kPageZeroBytes, stream));
    const int64_t cap = max_blocks ? max_blocks : ANNLITE_PAGE_MAX_BLOCKS;
    const int64_t need = (A.N + ANNLITE_PAGE_BLOCK_ROWS - 1) / ANNLITE_PAGE_BLOCK_ROWS;
    const unsigned blocks = (unsigned)(need < 1 ? 1 : need < cap ? need : cap);  // (N = 0: the launches find a total of 0)
    for (int s = 0; s < n; ++s)
        hipLaunchKernelGGL(page_pass_kernel, dim3(blocks), dim3(kPageThreads), 0, stream, A, ws, s, digits[s], s ? digits[s - 1] : 0);
    hipLaunchKernelGGL(page_collect_kernel, dim3(blocks), dim3(kPageThreads), 0, stream, A, ws, n, digits[n - 1]);
    hipLaunchKernelGGL(page_sort_kernel, dim3(1), dim3(kPageSortThreads), 0, stream, ws, n, out_rows_dev, out_n_dev);
    return launch_status("page kernels");
}

// what both entries ask of the row range, the page and the buffers
static int page_check(int64_t N, int64_t n_words, int64_t first, int64_t count, const void *out_rows_dev, const void *out_n_dev, const void *workspace,
                      size_t workspace_bytes, int max_blocks) {
    ANNLITE_REQUIRE(N >= 0 && N <= INT32_MAX && n_words >= 0 && n_words <= (INT64_MAX >> 5) && n_words * 32 >= N,
                    "bad N=%lld n_words=%lld (0 <= N < 2^31, n_words * 32 >= N)", (long long)N, (long long)n_words);
    ANNLITE_REQUIRE(first >= 0, "bad first=%lld", (long long)first);
    ANNLITE_REQUIRE(count >= 1 && count <= ANNLITE_PAGE_MAX, "bad count=%lld (1 .. %d)", (long long)count, ANNLITE_PAGE_MAX);
    ANNLITE_REQUIRE(first + count <= INT32_MAX, "first + count = %lld passes 2^31 - 1", (long long)(first + count));
    ANNLITE_REQUIRE(max_blocks >= 0, "bad max_blocks=%d", max_blocks);
    ANNLITE_REQUIRE(out_rows_dev != nullptr && out_n_dev != nullptr, "out_rows_dev / out_n_dev is NULL");
    ANNLITE_REQUIRE(workspace != nullptr && workspace_bytes >= sizeof(PageWorkspace) && (uintptr_t)workspace % 16 == 0,
                    "workspace: %zu bytes at %p (annlite_page_workspace_bytes, 16-byte aligned)", workspace_bytes, workspace);
    return ANNLITE_OK;
}

}  // namespace annlite

using namespace annlite;

extern "C" int annlite_page_workspace_bytes(int64_t *bytes) {
    ANNLITE_REQUIRE(bytes != nullptr, "bytes is NULL");
    *bytes = (int64_t)sizeof(PageWorkspace);
    return ANNLITE_OK;
}

extern "C" int annlite_order_page(const uint32_t *mask_dev, const uint32_t *rows_dev, const void *values_dev, int kind, const uint32_t *present_dev,
                                  const uint32_t *rank_dev, int64_t rank_len, int64_t N, int64_t n_words, int descending, int64_t first,
                                  int64_t count, int32_t *out_rows_dev, int32_t *out_n_dev, void *workspace, size_t workspace_bytes, int max_blocks,
                                  void *stream) {
    ANNLITE_REQUIRE(kind == ANNLITE_COL_I64 || kind == ANNLITE_COL_F64 || kind == ANNLITE_COL_CODE, "bad column kind %d", kind);
    if (int rc = page_check(N, n_words, first, count, out_rows_dev, out_n_dev, workspace, workspace_bytes, max_blocks)) return rc;
    ANNLITE_REQUIRE(rows_dev != nullptr && values_dev != nullptr && present_dev != nullptr, "rows_dev / values_dev / present_dev is NULL");
    PageArgs A{};
    int n_key_digits = 8;
    if (kind == ANNLITE_COL_CODE) {
        ANNLITE_REQUIRE(rank_dev != nullptr && rank_len >= 1 && rank_len <= 65536, "a string column takes a rank table of 1 .. 65536 entries, not %lld at %p",
                        (long long)rank_len, (const void *)rank_dev);
        n_key_digits = rank_len <= 256 ? 1 : 2;
        A.rank = rank_dev, A.rank_len = (uint32_t)rank_len, A.key_mask = rank_len <= 256 ? 0xffu : 0xffffu;
    }
    A.bits = mask_dev ? mask_dev : rows_dev, A.and_bits = mask_dev ? rows_dev : nullptr;
    A.values = values_dev, A.present = present_dev, A.kind = kind, A.descending = descending != 0;
    A.N = N, A.first = (uint32_t)first, A.count = (uint32_t)count;
    return page_launch(A, n_key_digits, out_rows_dev, out_n_dev, workspace, max_blocks, (hipStream_t)stream);
}

extern "C" int annlite_bitmap_page(const uint32_t *bits_dev, const uint32_t *and_bits_dev, int64_t N, int64_t n_words, int64_t first, int64_t count,
                                   int32_t *out_rows_dev, int32_t *out_n_dev, void *workspace, size_t workspace_bytes, int max_blocks, void *stream) {
    if (int rc = page_check(N, n_words, first, count, out_rows_dev, out_n_dev, workspace, workspace_bytes, max_blocks)) return rc;
    ANNLITE_REQUIRE(bits_dev != nullptr, "bits_dev is NULL");
    PageArgs A{};
    A.bits = bits_dev, A.and_bits = and_bits_dev, A.kind = kPageKindNone;
    A.N = N, A.first = (uint32_t)first, A.count = (uint32_t)count;
    return page_launch(A, 0, out_rows_dev, out_n_dev, workspace, max_blocks, (hipStream_t)stream);
}
