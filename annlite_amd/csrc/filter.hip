// filter.hip -- filterable columns: a compiled filter program evaluated over typed columns of the row range, straight into the packed
// row bitmap every search here takes as valid_bits (annlite_filter_eval).
//
// The program (annlite_filter_program, include/annlite_hip.h) is a kernel argument BY VALUE: leaves, literals and the postfix code
// are uniform, so what the lanes share is read with scalar loads and the branches on it are scalar branches.  What differs per lane
// is the row: its column values (8 bytes per numeric leaf, 4 per string leaf, coalesced) and its bit of the column's present words.
//   * one row per lane; a wave's 64 verdicts are one __ballot, whose halves are two output words (ANDed with the caller's words);
//   * a lane's evaluation stack is one u32 of bits (bit 0 = the top): push = shift left, AND / OR fold bit 1 into bit 0;
//   * rows >= N load nothing and vote 0, so the words behind the rows -- the pads included -- are written as 0;
//   * the count of set bits is a wave-uniform sum of popcounts, reduced through LDS to one global atomic per workgroup.
#include "common.h"

namespace annlite {

constexpr int kFilterThreads = 256;

// The byte-wide fields of the program are read a dword at a time and taken apart with shifts: a uniform dword is a scalar load, a
// uniform byte is not (the compiler fetches it through the vector memory path, one round trip per code byte).
struct LeafDesc {
    uint32_t kind, op, lit_begin, lit_count;
};
__device__ __forceinline__ LeafDesc filter_leaf_desc(const annlite_filter_leaf &L) {
    static_assert(offsetof(annlite_filter_leaf, kind) % 4 == 0 && offsetof(annlite_filter_leaf, lit_count) == offsetof(annlite_filter_leaf, kind) + 3,
                  "kind, op, lit_begin, lit_count are one aligned dword");
    uint32_t w;
    __builtin_memcpy(&w, &L.kind, 4);
    return {w & 0xffu, (w >> 8) & 0xffu, (w >> 16) & 0xffu, w >> 24};
}
__device__ __forceinline__ uint32_t filter_code_at(const annlite_filter_program &P, int c) {
    static_assert(offsetof(annlite_filter_program, code) % 4 == 0 && ANNLITE_FILTER_MAX_CODE % 4 == 0, "the code is whole aligned dwords");
    uint32_t w;
    __builtin_memcpy(&w, &P.code[c & ~3], 4);
    return (w >> ((c & 3) * 8)) & 0xffu;
}

template <typename T>
__device__ __forceinline__ T filter_literal(const annlite_filter_program &P, int i) {
    const uint64_t raw = P.literals[i];
    T v;
    __builtin_memcpy(&v, &raw, sizeof(T));
    return v;
}

// the numeric comparisons, in the column's own type (i64: exact integers; f64: IEEE doubles, no NaN on either side)
template <typename T>
__device__ __forceinline__ bool filter_compare(const annlite_filter_program &P, const LeafDesc &L, T x) {
    const int b = L.lit_begin;
    switch (L.op) {
        case ANNLITE_FOP_LT: return x < filter_literal<T>(P, b);
        case ANNLITE_FOP_GT: return x > filter_literal<T>(P, b);
        case ANNLITE_FOP_LE: return x <= filter_literal<T>(P, b);
        case ANNLITE_FOP_GE: return x >= filter_literal<T>(P, b);
        case ANNLITE_FOP_EQ: return x == filter_literal<T>(P, b);
        case ANNLITE_FOP_NE: return x != filter_literal<T>(P, b);
        default: {  // IN / NIN
            bool any = false;
            for (int j = 0; j < (int)L.lit_count; ++j) any |= x == filter_literal<T>(P, b + j);
            return any == (L.op == ANNLITE_FOP_IN);
        }
    }
}

__global__ __launch_bounds__(kFilterThreads) void filter_eval_kernel(const annlite_filter_program P, int64_t N, int64_t n_words,
                                                                     const uint32_t *__restrict__ and_bits, uint32_t *__restrict__ out,
                                                                     unsigned long long *__restrict__ count) {
    __shared__ uint32_t s_count[kFilterThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const int64_t n_bits = n_words * 32;
    const int64_t step = (int64_t)gridDim.x * kFilterThreads;
    uint32_t set = 0;  // (wave-uniform)
    for (int64_t base = (int64_t)blockIdx.x * kFilterThreads + wave * kWave; base < n_bits; base += step) {
        const int64_t row = base + lane;
        bool verdict = false;
        if (row < N) {
            uint32_t leaf_bits = 0;
            for (int l = 0; l < P.n_leaves; ++l) {
                const annlite_filter_leaf &L = P.leaves[l];
                const LeafDesc desc = filter_leaf_desc(L);
                bool r = (L.present_dev[row >> 5] >> (row & 31)) & 1u;
                if (desc.kind == ANNLITE_COL_I64) {
                    r = r && filter_compare<int64_t>(P, desc, ((const int64_t *)L.values_dev)[row]);
                } else if (desc.kind == ANNLITE_COL_F64) {
                    r = r && filter_compare<double>(P, desc, ((const double *)L.values_dev)[row]);
                } else {  // a dictionary code into the leaf's bitset (a code beyond the bitset is not in the set)
                    const uint32_t code = (uint32_t)((const int32_t *)L.values_dev)[row];
                    r = r && (code >> 5) < L.set_words;
                    if (r) r = (L.set_bits_dev[code >> 5] >> (code & 31)) & 1u;
                }
                leaf_bits |= (uint32_t)r << l;
            }
            uint32_t stack = 0;
            for (int c = 0; c < P.n_code; ++c) {
                const uint32_t op = filter_code_at(P, c);
                if (op < ANNLITE_FILTER_MAX_LEAVES) {
                    stack = (stack << 1) | ((leaf_bits >> op) & 1u);
                } else if (op == ANNLITE_FCODE_AND) {
                    stack = ((stack >> 1) & ~1u) | ((stack >> 1) & stack & 1u);
                } else if (op == ANNLITE_FCODE_OR) {
                    stack = (stack >> 1) | (stack & 1u);
                } else if (op == ANNLITE_FCODE_NOT) {
                    stack ^= 1u;
                } else {  // TRUE
                    stack = (stack << 1) | 1u;
                }
            }
            verdict = stack & 1u;
        }
        const unsigned long long votes = __ballot(verdict);
        const int64_t w = base >> 5;
        const bool second = w + 1 < n_words;  // (n_words may be odd: the wave's upper half then lies beyond the array, and beyond N)
        uint32_t lo = (uint32_t)votes, hi = second ? (uint32_t)(votes >> 32) : 0u;
        if (and_bits) {
            lo &= and_bits[w];
            if (second) hi &= and_bits[w + 1];
        }
        if (lane == 0) out[w] = lo;
        if (lane == 1 && second) out[w + 1] = hi;
        set += __popc(lo) + __popc(hi);
    }
    if (count == nullptr) return;  // (uniform)
    if (lane == 0) s_count[wave] = set;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (int i = 0; i < kFilterThreads / kWave; ++i) total += s_count[i];
        if (total) atomicAdd(count, (unsigned long long)total);
    }
}

// the stack discipline of the postfix code, and every index the kernel follows
static int filter_program_check(const annlite_filter_program &P) {
    ANNLITE_REQUIRE(P.n_leaves >= 0 && P.n_leaves <= ANNLITE_FILTER_MAX_LEAVES, "n_leaves=%d (at most %d)", P.n_leaves, ANNLITE_FILTER_MAX_LEAVES);
    ANNLITE_REQUIRE(P.n_literals >= 0 && P.n_literals <= ANNLITE_FILTER_MAX_LITERALS, "n_literals=%d (at most %d)", P.n_literals,
                    ANNLITE_FILTER_MAX_LITERALS);
    ANNLITE_REQUIRE(P.n_code >= 1 && P.n_code <= ANNLITE_FILTER_MAX_CODE, "n_code=%d (1 .. %d)", P.n_code, ANNLITE_FILTER_MAX_CODE);
    for (int l = 0; l < P.n_leaves; ++l) {
        const annlite_filter_leaf &L = P.leaves[l];
        ANNLITE_REQUIRE(L.values_dev != nullptr && L.present_dev != nullptr, "leaf %d: null column pointer", l);
        if (L.kind == ANNLITE_COL_CODE) {
            ANNLITE_REQUIRE(L.op == ANNLITE_FOP_IN_SET && L.set_bits_dev != nullptr && L.set_words >= 1, "leaf %d: a string column takes IN_SET with a bitset",
                            l);
        } else {
            ANNLITE_REQUIRE(L.kind == ANNLITE_COL_I64 || L.kind == ANNLITE_COL_F64, "leaf %d: bad column kind %d", l, (int)L.kind);
            ANNLITE_REQUIRE(L.op <= ANNLITE_FOP_NIN, "leaf %d: bad numeric op %d", l, (int)L.op);
            const bool member = L.op == ANNLITE_FOP_IN || L.op == ANNLITE_FOP_NIN;
            ANNLITE_REQUIRE(member || L.lit_count == 1, "leaf %d: a comparison takes one literal, not %d", l, (int)L.lit_count);
            ANNLITE_REQUIRE((int)L.lit_begin + (int)L.lit_count <= P.n_literals, "leaf %d: literals [%d, %d) of %d", l, (int)L.lit_begin,
                            (int)L.lit_begin + (int)L.lit_count, P.n_literals);
        }
    }
    int depth = 0;
    for (int c = 0; c < P.n_code; ++c) {
        const int op = P.code[c];
        if (op < ANNLITE_FILTER_MAX_LEAVES) {
            ANNLITE_REQUIRE(op < P.n_leaves, "code %d pushes leaf %d of %d", c, op, P.n_leaves);
            ++depth;
        } else if (op == ANNLITE_FCODE_TRUE) {
            ++depth;
        } else if (op == ANNLITE_FCODE_AND || op == ANNLITE_FCODE_OR) {
            ANNLITE_REQUIRE(depth >= 2, "code %d: a binary operator on a stack of %d", c, depth);
            --depth;
        } else {
            ANNLITE_REQUIRE(op == ANNLITE_FCODE_NOT, "code %d: unknown op 0x%02x", c, op);
            ANNLITE_REQUIRE(depth >= 1, "code %d: NOT on an empty stack", c);
        }
        ANNLITE_REQUIRE(depth <= ANNLITE_FILTER_MAX_STACK, "code %d: the stack passes %d values", c, ANNLITE_FILTER_MAX_STACK);
    }
    ANNLITE_REQUIRE(depth == 1, "the code leaves %d values on the stack, not one", depth);
    return ANNLITE_OK;
}

}  // namespace annlite

using namespace annlite;

extern "C" int annlite_filter_eval(const annlite_filter_program *program, int64_t N, const uint32_t *and_bits_dev, uint32_t *out_bits_dev,
                                   int64_t n_words, uint64_t *count_dev, int max_blocks, void *stream) {
    ANNLITE_REQUIRE(program != nullptr, "program is NULL");
    ANNLITE_REQUIRE(N >= 0 && n_words >= 0 && n_words <= (INT64_MAX >> 5) && n_words * 32 >= N, "bad N=%lld n_words=%lld (n_words * 32 >= N)", (long long)N,
                    (long long)n_words);
    ANNLITE_REQUIRE(max_blocks >= 0, "bad max_blocks=%d", max_blocks);
    if (int rc = filter_program_check(*program)) return rc;
    if (n_words == 0) return ANNLITE_OK;
    ANNLITE_REQUIRE(out_bits_dev != nullptr, "out_bits_dev is NULL");
    const int64_t cap = max_blocks ? max_blocks : ANNLITE_FILTER_MAX_BLOCKS;
    const int64_t need = (n_words * 32 + kFilterThreads - 1) / kFilterThreads;
    const unsigned blocks = (unsigned)(need < cap ? need : cap);
    hipLaunchKernelGGL(filter_eval_kernel, dim3(blocks), dim3(kFilterThreads), 0, (hipStream_t)stream, *program, N, n_words, and_bits_dev,
                       out_bits_dev, (unsigned long long *)count_dev);
    return launch_status("filter_eval_kernel");
}
