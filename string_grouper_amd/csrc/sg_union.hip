// The union of several fixed-stride candidate results over the same records (include/sg_hip.h: sg_topn_union; DESIGN.md
// section 4, "Candidate union").  Row i of the result holds the distinct columns that row i of any part names, in ascending
// column order; a column part 0 holds keeps part 0's bits, every other one gets the primary field's score of the pair --
// pair_rows_dot's (sg_pairs_device.h), so the value is what the primary multiply would have written had it found the pair.
//
// The result's stride is the longest row of the union, which nobody knows before the rows are united, and the call has one
// read-back.  So the rows are united into scratch at the stride W = sum of the parts' strides (no row is longer), the missing
// scores are filled in there, the status word and the longest row come back together, and a copy at the true stride is what
// the caller gets.
//
// Four launches.  union_short_kernel: SG_PAIR_LANES lanes a row whose parts hold at most SG_UNION_SHORT entries together
// (nearly every row of a name list), the row's columns in LDS, a rank by counting: an entry is kept when no entry with the
// same column goes before it in (part, place) order, and its place is the number of kept entries with a lower column -- no
// sort network, no exchange between lanes but the OR of their kept bits.  union_block_kernel: the rows above that (up to 2 048
// entries), which the first kernel lists on the device, a block a row: the keys (column, entry number) sorted in LDS by a bitonic
// network, equal neighbours dropped, the kept ones placed by a scan.  An entry of part 0 carries its value; any other is
// written with its column complemented (~j < 0), which is what union_fill_kernel looks for: the walk of sg_pairs_device.h over
// a row's marked entries, the row of A found when the first one shows.  union_copy_kernel: the rows at their stride.
#include "sg_pairs_device.h"

#define SG_UNION_BLOCK 256
#define SG_UNION_MAX_PARTS 8
#define SG_UNION_MAX_ENTRIES 2048  // entries a row's parts hold together: the block kernel's LDS
#define SG_UNION_SHORT 64          // rows of up to this many entries: eight lanes unite them; above: a block

// words of a call's head: [0] status -- bit 0 a counted column outside [0, N), bit 1 / bit 2 a row of A / B that a filled
// candidate reads and that is not in strictly ascending column order; [1] the long rows listed; [2] the longest united row
#define SG_UNION_BAD_COLUMN 1u
#define SG_UNION_BAD_A 2u
#define SG_UNION_BAD_B 4u

struct UnionParts {
    const int32_t *cols[SG_UNION_MAX_PARTS];
    const int32_t *counts[SG_UNION_MAX_PARTS];
    int32_t stride[SG_UNION_MAX_PARTS];
    int32_t n;
};

template <typename T>
__global__ void __launch_bounds__(SG_UNION_BLOCK) union_short_kernel(
    UnionParts P, const T *__restrict__ vals0, int64_t n_rows, int64_t n_cols, int32_t wide, int32_t *__restrict__ w_cols,
    T *__restrict__ w_vals, int32_t *__restrict__ w_counts, int32_t *__restrict__ long_rows, uint32_t *head) {
    constexpr int G = SG_PAIR_LANES;
    constexpr int per_block = SG_UNION_BLOCK / G;
    __shared__ int32_t s_j[per_block * SG_UNION_SHORT];
    __shared__ uint32_t s_max;
    const int l = threadIdx.x & (G - 1);
    int32_t *row_j = s_j + (threadIdx.x / G) * SG_UNION_SHORT;
    const int64_t row = ((int64_t)blockIdx.x * SG_UNION_BLOCK + threadIdx.x) / G;
    if (threadIdx.x == 0) s_max = 0;
    // (no thread leaves before the block's two barriers; what follows is uniform over a group)
    int32_t total = 0, cnt0 = 0;
    bool mine = row < n_rows;
    if (mine) {
#pragma unroll
        for (int p = 0; p < SG_UNION_MAX_PARTS; ++p)
            if (p < P.n) total += counted(P.counts[p], row, P.stride[p]);
        cnt0 = counted(P.counts[0], row, P.stride[0]);
        if (total > SG_UNION_SHORT) {   // a block's row
            if (l == 0) long_rows[atomicAdd(head + 1, 1u)] = (int32_t)row;
            mine = false;
        }
    }
    if (mine) {   // the row's columns in (part, place) order
        int32_t off = 0;
#pragma unroll
        for (int p = 0; p < SG_UNION_MAX_PARTS; ++p) {
            if (p < P.n) {
                const int32_t c = counted(P.counts[p], row, P.stride[p]);
                const int32_t *src = P.cols[p] + row * (int64_t)P.stride[p];
                for (int32_t e = l; e < c; e += G) row_j[off + e] = src[e];
                off += c;
            }
        }
    }
    __syncthreads();
    if (mine) {
        uint32_t kept_lo = 0, kept_hi = 0;
        bool bad = false;
        for (int32_t g = l; g < total; g += G) {
            const int32_t j = row_j[g];
            if (j < 0 || j >= n_cols) {   // it takes part in nothing; the call is refused
                bad = true;
                continue;
            }
            bool first = true;
            for (int32_t q = 0; q < g; ++q) first &= row_j[q] != j;
            if (first) {
                if (g < 32) kept_lo |= 1u << g;
                else kept_hi |= 1u << (g - 32);
            }
        }
        if (bad) atomicOr(head, SG_UNION_BAD_COLUMN);
#pragma unroll
        for (int d = 1; d < G; d <<= 1) {
            kept_lo |= __shfl_xor(kept_lo, d, G);
            kept_hi |= __shfl_xor(kept_hi, d, G);
        }
        const uint64_t kept = ((uint64_t)kept_hi << 32) | kept_lo;
        const int64_t out = row * (int64_t)wide;
        for (int32_t g = l; g < total; g += G) {
            if (!((kept >> g) & 1u)) continue;
            const int32_t j = row_j[g];
            int32_t rank = 0;
            for (int32_t q = 0; q < total; ++q) rank += (((kept >> q) & 1u) && row_j[q] < j) ? 1 : 0;
            if (g < cnt0) {
                w_cols[out + rank] = j;
                w_vals[out + rank] = vals0[row * (int64_t)P.stride[0] + g];
            } else {
                w_cols[out + rank] = ~j;   // the fill's mark
            }
        }
        if (l == 0) {
            const uint32_t n_kept = (uint32_t)__popcll(kept);
            w_counts[row] = (int32_t)n_kept;
            if (n_kept) atomicMax(&s_max, n_kept);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(head + 2, s_max);
}

// The rows the short kernel listed, a block a row at a time: the grid is fixed, a block takes the list's entries blockIdx.x,
// blockIdx.x + gridDim.x, ...  LDS: 2 048 keys of eight bytes and the scan's 256 partial sums, 17 KiB a block.
template <typename T>
__global__ void __launch_bounds__(SG_UNION_BLOCK) union_block_kernel(
    UnionParts P, const T *__restrict__ vals0, int64_t n_cols, int32_t wide, int32_t *__restrict__ w_cols,
    T *__restrict__ w_vals, int32_t *__restrict__ w_counts, const int32_t *__restrict__ long_rows, uint32_t *head) {
    constexpr int PER = SG_UNION_MAX_ENTRIES / SG_UNION_BLOCK;   // consecutive keys a thread scans
    constexpr uint64_t NONE = ~(uint64_t)0;
    __shared__ uint64_t s_key[SG_UNION_MAX_ENTRIES];   // (column << 32) | the entry's number in (part, place) order
    __shared__ int32_t s_sum[SG_UNION_BLOCK];
    const uint32_t n = head[1];
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        const int64_t row = long_rows[k];
        int32_t total = 0;
        bool bad = false;
#pragma unroll
        for (int p = 0; p < SG_UNION_MAX_PARTS; ++p) {
            if (p < P.n) {
                const int32_t c = counted(P.counts[p], row, P.stride[p]);
                const int32_t *src = P.cols[p] + row * (int64_t)P.stride[p];
                for (int32_t e = threadIdx.x; e < c; e += SG_UNION_BLOCK) {
                    const int32_t j = src[e];
                    const bool ok = j >= 0 && j < n_cols;
                    bad |= !ok;
                    s_key[total + e] = ok ? ((uint64_t)(uint32_t)j << 32) | (uint32_t)(total + e) : NONE;
                }
                total += c;   // (at most SG_UNION_MAX_ENTRIES: the driver has summed the strides)
            }
        }
        if (bad) atomicOr(head, SG_UNION_BAD_COLUMN);
        const int32_t cnt0 = counted(P.counts[0], row, P.stride[0]);
        int32_t m = SG_UNION_SHORT * 2;   // the network's size: the power of two at or above total
        while (m < total) m <<= 1;
        for (int32_t e = total + threadIdx.x; e < m; e += SG_UNION_BLOCK) s_key[e] = NONE;
        __syncthreads();
        for (int32_t size = 2; size <= m; size <<= 1) {
            for (int32_t half = size >> 1; half > 0; half >>= 1) {
                for (int32_t t = threadIdx.x; t < (m >> 1); t += SG_UNION_BLOCK) {
                    const int32_t lo = ((t & ~(half - 1)) << 1) | (t & (half - 1)), hi = lo | half;
                    const bool up = (lo & size) == 0;
                    const uint64_t a = s_key[lo], b = s_key[hi];
                    if ((a > b) == up) {
                        s_key[lo] = b;
                        s_key[hi] = a;
                    }
                }
                __syncthreads();
            }
        }
        // kept: the first key of every column (NONE sorts behind all of them); a thread owns PER consecutive keys
        const int32_t first = threadIdx.x * PER;
        int32_t here = 0;
        for (int32_t e = first; e < first + PER && e < m; ++e) {
            const uint64_t key = s_key[e];
            here += (key != NONE && (e == 0 || (uint32_t)(s_key[e - 1] >> 32) != (uint32_t)(key >> 32))) ? 1 : 0;
        }
        s_sum[threadIdx.x] = here;
        __syncthreads();
        for (int d = 1; d < SG_UNION_BLOCK; d <<= 1) {   // inclusive scan of the threads' counts
            const int32_t add = threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0;
            __syncthreads();
            s_sum[threadIdx.x] += add;
            __syncthreads();
        }
        int32_t place = s_sum[threadIdx.x] - here;
        const int64_t out = row * (int64_t)wide;
        for (int32_t e = first; e < first + PER && e < m; ++e) {
            const uint64_t key = s_key[e];
            if (key == NONE || (e != 0 && (uint32_t)(s_key[e - 1] >> 32) == (uint32_t)(key >> 32))) continue;
            const int32_t j = (int32_t)(key >> 32), g = (int32_t)(uint32_t)key;
            if (g < cnt0) {
                w_cols[out + place] = j;
                w_vals[out + place] = vals0[row * (int64_t)P.stride[0] + g];
            } else {
                w_cols[out + place] = ~j;
            }
            ++place;
        }
        if (threadIdx.x == SG_UNION_BLOCK - 1) {
            const int32_t n_kept = s_sum[SG_UNION_BLOCK - 1];
            w_counts[row] = n_kept;
            if (n_kept > 0) atomicMax(head + 2, (uint32_t)n_kept);
        }
        __syncthreads();   // the next row reuses the block's LDS
    }
}

template <typename T>
__global__ void __launch_bounds__(SG_PAIR_BLOCK) union_fill_kernel(
    int32_t *__restrict__ w_cols, T *__restrict__ w_vals, const int32_t *__restrict__ w_counts, int64_t n_rows, int64_t n_cols,
    int32_t wide, int32_t chunks, PairField<T> F, uint32_t *head) {
    constexpr int G = SG_PAIR_LANES;
    const int l = threadIdx.x & (G - 1);
    const int group_shift = threadIdx.x & (SG_WAVE - 1) & ~(G - 1);   // the group's first lane in its wave
    const int64_t g = ((int64_t)blockIdx.x * SG_PAIR_BLOCK + threadIdx.x) / G;
    const int64_t row = g / chunks;
    if (row >= n_rows) return;   // (everything below is uniform over the group: its lanes leave, loop and shuffle together)
    const int32_t cnt = w_counts[row];   // (at most `wide`: the union kernels counted it)
    const int32_t e0 = (int32_t)(g - row * chunks) * SG_PAIR_ROW_CHUNK;
    const int32_t e1 = cnt < e0 + SG_PAIR_ROW_CHUNK ? cnt : e0 + SG_PAIR_ROW_CHUNK;
    const int64_t base = row * (int64_t)wide;
    int64_t a0 = 0, a1 = -1;   // the row of A, found when the first marked entry shows
    for (int32_t e = e0; e < e1; ++e) {
        const int32_t mark = w_cols[base + e];
        if (mark >= 0) continue;
        const int64_t j = ~mark;   // in [0, n_cols): the union kernels keep no other column
        if (j >= n_cols) continue;
        if (a1 < 0) pair_left_row<T>(F, row, l, head, SG_UNION_BAD_A, a0, a1);
        const T s = pair_score<T>(F, a0, a1, j, l, group_shift, head, SG_UNION_BAD_B);
        if (l == 0) {   // (the group's other lanes have read this entry's mark above, and read no entry twice)
            w_vals[base + e] = s;
            w_cols[base + e] = (int32_t)j;
        }
    }
}

// the united rows at the result's stride: a thread a cell
template <typename T>
__global__ void __launch_bounds__(SG_UNION_BLOCK) union_copy_kernel(
    const int32_t *__restrict__ w_cols, const T *__restrict__ w_vals, const int32_t *__restrict__ w_counts, int64_t n_rows,
    int32_t wide, int32_t stride, int32_t *__restrict__ cols, T *__restrict__ vals, int32_t *__restrict__ counts) {
    const int64_t cell = (int64_t)blockIdx.x * SG_UNION_BLOCK + threadIdx.x;
    const int64_t row = cell / stride;
    if (row >= n_rows) return;
    const int32_t e = (int32_t)(cell - row * stride);
    const int32_t cnt = w_counts[row];
    if (e == 0) counts[row] = cnt;
    if (e < cnt) {
        cols[cell] = w_cols[row * (int64_t)wide + e];
        vals[cell] = w_vals[row * (int64_t)wide + e];
    }
}

template <typename T>
static int unite(sg_ctx *ctx, const sg_topn *const *parts, int32_t n_parts, const sg_rescore_field *primary, int32_t wide,
                 int32_t *w_cols, void *w_vals, int32_t *w_counts, int32_t *d_long_rows, uint32_t *d_head) {
    const sg_topn *first = parts[0];
    UnionParts P;
    memset(&P, 0, sizeof(P));
    P.n = n_parts;
    for (int p = 0; p < n_parts; ++p) P.cols[p] = parts[p]->d_cols, P.counts[p] = parts[p]->d_counts, P.stride[p] = parts[p]->stride;
    constexpr int per_block = SG_UNION_BLOCK / SG_PAIR_LANES;
    // the kernel is chosen ROW BY ROW: eight lanes for a row of up to SG_UNION_SHORT entries, whatever the strides; the rows above
    // it are listed on the device (no read-back) and taken by a fixed grid of blocks
    const int64_t blocks = (first->n_rows + per_block - 1) / per_block;
    hipLaunchKernelGGL(union_short_kernel<T>, dim3((unsigned)blocks), dim3(SG_UNION_BLOCK), 0, ctx->stream, P,
                       (const T *)first->d_vals, first->n_rows, first->n_cols, wide, w_cols, (T *)w_vals, w_counts, d_long_rows,
                       d_head);
    SG_HIP_TRY(hipGetLastError());
    if (wide > SG_UNION_SHORT) {
        const int64_t grid = std::min<int64_t>(first->n_rows, (int64_t)ctx->num_cu * 8);
        hipLaunchKernelGGL(union_block_kernel<T>, dim3((unsigned)grid), dim3(SG_UNION_BLOCK), 0, ctx->stream, P,
                           (const T *)first->d_vals, first->n_cols, wide, w_cols, (T *)w_vals, w_counts, d_long_rows, d_head);
        SG_HIP_TRY(hipGetLastError());
    }
    const int32_t chunks = (wide + SG_PAIR_ROW_CHUNK - 1) / SG_PAIR_ROW_CHUNK;
    hipLaunchKernelGGL(union_fill_kernel<T>, dim3((unsigned)pair_blocks(first->n_rows * chunks)), dim3(SG_PAIR_BLOCK), 0,
                       ctx->stream, w_cols, (T *)w_vals, w_counts, first->n_rows, first->n_cols, wide, chunks,
                       make_pair_field<T>(*primary), d_head);
    SG_HIP_TRY(hipGetLastError());
    return SG_OK;
}

extern "C" int sg_topn_union(sg_ctx *ctx, const sg_topn *const *parts, int32_t n_parts, const sg_rescore_field *primary,
                             sg_topn **out) {
    SG_REQUIRE(ctx && parts && primary && out, "null argument");
    SG_REQUIRE(n_parts >= 2 && n_parts <= SG_UNION_MAX_PARTS, "between 2 and 8 parts are expected");
    int64_t wide = 0;
    for (int p = 0; p < n_parts; ++p) {
        SG_REQUIRE(parts[p] != nullptr, "a part is null");
        SG_REQUIRE(parts[p]->n_rows == parts[0]->n_rows && parts[p]->n_cols == parts[0]->n_cols && parts[p]->dtype == parts[0]->dtype,
                   "the parts differ in rows, columns or value type");
        SG_REQUIRE(parts[p]->stride >= 1, "a part without a stride");
        wide += parts[p]->stride;
    }
    SG_REQUIRE(wide <= SG_UNION_MAX_ENTRIES, "the parts' strides exceed 2048 together: ask the multiplies for fewer a row");
    const sg_topn *first = parts[0];
    SG_TRY(check_pair_field(*primary, first->dtype, first->n_rows, first->n_cols, "the primary field's", "parts", false));
    const int64_t chunks = (wide + SG_PAIR_ROW_CHUNK - 1) / SG_PAIR_ROW_CHUNK;
    if (pair_blocks(first->n_rows * chunks) > INT32_MAX || first->n_rows > INT32_MAX)
        return exceeds_one_launch(first->n_rows, "rows of candidates", "unite");
    SG_TRY(ensure_pair_rows(ctx, primary->A, primary->B));
    TopnPtr r;
    if (first->n_rows == 0) {
        SG_TRY(topn_alloc(ctx, 0, first->n_cols, 1, first->dtype, &r));
        *out = r.release();
        return SG_OK;
    }
    const size_t s = first->dtype == SG_F64 ? 8 : 4, cells = (size_t)first->n_rows * (size_t)wide;
    Scratch tmp(ctx);
    uint32_t *d_head = nullptr;   // the status word, the long rows' counter, the longest united row (and a word to spare)
    int32_t *w_cols = nullptr, *w_counts = nullptr, *d_long_rows = nullptr;
    void *w_vals = nullptr;
    SG_TRY(tmp.alloc(4, &d_head));
    SG_TRY(tmp.alloc(cells, &w_cols));
    SG_TRY(tmp.alloc_bytes(cells * s, &w_vals));
    SG_TRY(tmp.alloc((size_t)first->n_rows, &w_counts));
    if (wide > SG_UNION_SHORT) SG_TRY(tmp.alloc((size_t)first->n_rows, &d_long_rows));
    SG_HIP_TRY(hipMemsetAsync(d_head, 0, 16, ctx->stream));
    SG_TRY(by_dtype(first->dtype, [&](auto t) {
        return unite<decltype(t)>(ctx, parts, n_parts, primary, (int32_t)wide, w_cols, w_vals, w_counts, d_long_rows, d_head);
    }));
    uint32_t head[4] = {0, 0, 0, 0};
    SG_TRY(sg_fetch(ctx, head, d_head, 16));   // the one read-back: the status word and the result's stride
    if (head[0]) {
        std::string what;
        if (head[0] & SG_UNION_BAD_COLUMN) what += "a part's column lies outside the parts' columns; ";
        if (head[0] & SG_UNION_BAD_A) what += unsorted_row("the primary field's left matrix", "candidate reads");
        if (head[0] & SG_UNION_BAD_B) what += unsorted_row("the primary field's right matrix", "candidate reads");
        sg_set_error("bad argument: %s", what.c_str());
        return SG_ERR_BADARG;
    }
    const int32_t stride = head[2] > 0 ? (int32_t)head[2] : 1;
    if ((double)first->n_rows * (double)stride > 2.0e9)
        return result_overflow(first->n_rows, stride, ": lower the candidates' max_n_matches or unite the records in pieces");
    SG_TRY(topn_alloc(ctx, first->n_rows, first->n_cols, stride, first->dtype, &r));
    const int64_t copy_blocks = (first->n_rows * (int64_t)stride + SG_UNION_BLOCK - 1) / SG_UNION_BLOCK;
    SG_TRY(by_dtype(first->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(union_copy_kernel<T>, dim3((unsigned)copy_blocks), dim3(SG_UNION_BLOCK), 0, ctx->stream, w_cols,
                           (const T *)w_vals, w_counts, first->n_rows, (int32_t)wide, stride, r->d_cols, (T *)r->d_vals, r->d_counts);
        SG_HIP_TRY(hipGetLastError());
        return SG_OK;
    }));
    *out = r.release();
    return SG_OK;
}
