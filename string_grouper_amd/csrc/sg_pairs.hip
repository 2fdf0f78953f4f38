// Pair similarities -- the score of NAMED row pairs: out[p] = (A . B^T)[left[p], right[p]], the element the top-n multiply
// (K4 / K4p, string_grouper.py:725-743) would report for that pair, in the multiply's arithmetic:
//     acc = +0.0;  for every column k that both rows hold, ascending:  acc = rn(acc + rn(A[i, k] * B[j, k]))
// -- every product and every sum rounded on its own, zero products added like any other (a lone product of -0.0 gives +0.0),
// no common column or an empty row: +0.0.  It is NOT K9's arithmetic (sg_reduce.hip: non-zero products, numpy's pairwise
// sum), which is what compute_pairwise_similarities (string_grouper.py:55) gives for the same pair.  No gate: values of any
// sign, NaN and inf flow through.
//
// Lanes ("Pair similarities"): SG_PAIR_LANES = 8 lanes a pair, eight pairs a wave.  The two rows are
// walked in chunks of eight entries, one entry a lane (a chunk is one 32-byte piece of the column array and one of the
// values: the lanes of a group read neighbours, not 64 lines of their own as a thread a pair would).  Every lane compares
// its entry of A's chunk with the eight columns of B's chunk (shuffles inside the group), the chunk whose last column is
// the smaller one is retired and the next one loaded -- a merge by chunks -- and when a chunk of A is retired its products
// are added lane by lane, lowest first, into an accumulator that every lane of the group holds: the order of the adds is
// the column order whatever the chunking.
#include "sg_k4_device.h"

#define SG_PAIR_LANES 8
#define SG_PAIR_BLOCK 256   // 32 pairs a block

// status word of a call, one bit a cause
#define SG_PAIR_BAD_LEFT 1u       // an entry of `left` outside [0, rows of A)
#define SG_PAIR_BAD_RIGHT 2u      // an entry of `right` outside [0, rows of B)
#define SG_PAIR_UNSORTED_A 4u     // a row of A that some pair reads is not in strictly ascending column order
#define SG_PAIR_UNSORTED_B 8u

// entries [lo, hi) of a row, the group's lanes striding over them: does a column fail to exceed the one before it?
__device__ __forceinline__ bool row_not_ascending(const int32_t *__restrict__ idx, int64_t lo, int64_t hi, int l) {
    bool bad = false;
    for (int64_t q = lo + 1 + l; q < hi; q += SG_PAIR_LANES) bad |= idx[q] <= idx[q - 1];
    return bad;
}

// the products of a retired chunk of A, lane 0's first: `hits` (group-uniform) has bit s set when lane s holds one
template <typename T>
__device__ __forceinline__ T add_in_lane_order(T acc, T prod, uint32_t hits) {
#pragma unroll
    for (int s = 0; s < SG_PAIR_LANES; ++s) {
        const T ps = __shfl(prod, s, SG_PAIR_LANES);
        if ((hits >> s) & 1u) acc = add_rn<T>(acc, ps);
    }
    return acc;
}

template <typename T>
__global__ void __launch_bounds__(SG_PAIR_BLOCK) pairs_dot_kernel(
    const int64_t *__restrict__ a_indptr, const int32_t *__restrict__ a_indices, const T *__restrict__ a_data, int64_t n_a,
    const int64_t *__restrict__ b_indptr, const int32_t *__restrict__ b_indices, const T *__restrict__ b_data, int64_t n_b,
    const int32_t *__restrict__ left, const int32_t *__restrict__ right, int64_t n_pairs, int check_a, int check_b,
    uint32_t *status, T *out) {
    constexpr int G = SG_PAIR_LANES;
    const int l = threadIdx.x & (G - 1);
    const int group_shift = threadIdx.x & (SG_WAVE - 1) & ~(G - 1);   // the group's first lane in its wave
    const int64_t p = ((int64_t)blockIdx.x * SG_PAIR_BLOCK + threadIdx.x) / G;
    if (p >= n_pairs) return;   // (everything below is uniform over the group: its lanes leave, loop and shuffle together)
    const int64_t i = left[p], j = right[p];
    if (i < 0 || i >= n_a || j < 0 || j >= n_b) {
        if (l == 0) atomicOr(status, (i < 0 || i >= n_a ? SG_PAIR_BAD_LEFT : 0u) | (j < 0 || j >= n_b ? SG_PAIR_BAD_RIGHT : 0u));
        return;
    }
    const int64_t a0 = a_indptr[i], a1 = a_indptr[i + 1], b0 = b_indptr[j], b1 = b_indptr[j + 1];
    if (check_a && row_not_ascending(a_indices, a0, a1, l)) atomicOr(status, SG_PAIR_UNSORTED_A);
    if (check_b && row_not_ascending(b_indices, b0, b1, l)) atomicOr(status, SG_PAIR_UNSORTED_B);

    // a lane without an entry holds a column no entry has (-2 in A's chunk, -1 in B's: they never meet either)
    int64_t pa = a0, pb = b0;
    int ka = pa + l < a1 ? a_indices[pa + l] : -2, kb = pb + l < b1 ? b_indices[pb + l] : -1;
    T va = pa + l < a1 ? a_data[pa + l] : (T)0, vb = pb + l < b1 ? b_data[pb + l] : (T)0;
    T acc = (T)0, prod = (T)0;
    bool hit = false;
    while (pa < a1 && pb < b1) {
        int src = -1;
#pragma unroll
        for (int s = 0; s < G; ++s)
            if (__shfl(kb, s, G) == ka) src = s;
        const T vb_hit = __shfl(vb, src & (G - 1), G);
        if (src >= 0) {   // (at most once for an entry of A: B's columns are distinct)
            prod = mul_rn<T>(va, vb_hit);
            hit = true;
        }
        const int64_t in_a = a1 - pa, in_b = b1 - pb;
        const int last_a = __shfl(ka, (int)(in_a < G ? in_a : G) - 1, G), last_b = __shfl(kb, (int)(in_b < G ? in_b : G) - 1, G);
        if (last_a <= last_b) {   // nothing further in B meets this chunk of A
            const uint32_t hits = (uint32_t)(__ballot(hit) >> group_shift) & ((1u << G) - 1u);
            if (hits) acc = add_in_lane_order<T>(acc, prod, hits);
            hit = false;
            pa += G;
            ka = pa + l < a1 ? a_indices[pa + l] : -2;
            va = pa + l < a1 ? a_data[pa + l] : (T)0;
        }
        if (last_b <= last_a) {
            pb += G;
            kb = pb + l < b1 ? b_indices[pb + l] : -1;
            vb = pb + l < b1 ? b_data[pb + l] : (T)0;
        }
    }
    if (pa < a1) {   // B ran out first: the products the current chunk of A has met so far
        const uint32_t hits = (uint32_t)(__ballot(hit) >> group_shift) & ((1u << G) - 1u);
        if (hits) acc = add_in_lane_order<T>(acc, prod, hits);
    }
    if (l == 0) out[p] = acc;
}

// Column order is what the merge rests on.  A matrix the vectoriser made has it by construction, one the cosine gate has
// passed (sg_csr_props) has been measured; any other is checked by the kernel, row by row, for the rows the pairs name.
static bool known_ascending(const sg_csr *m) { return m->props_state == 1 || (m->props_state == 0 && m->from_vectoriser); }

extern "C" int sg_csr_pairs_dot(sg_ctx *ctx, const sg_csr *A, const sg_csr *B, const int32_t *d_left, const int32_t *d_right,
                                int64_t n_pairs, void *out_host) {
    SG_REQUIRE(ctx && A && B, "null argument");
    SG_REQUIRE(A->n_cols == B->n_cols, "matrices differ in shape (their columns)");
    SG_REQUIRE(A->dtype == B->dtype, "matrices differ in value type");
    SG_REQUIRE(n_pairs >= 0, "negative number of pairs");
    if (n_pairs == 0) return SG_OK;
    SG_REQUIRE(d_left && d_right && out_host, "null argument");
    const int64_t blocks = (n_pairs + SG_PAIR_BLOCK / SG_PAIR_LANES - 1) / (SG_PAIR_BLOCK / SG_PAIR_LANES);
    if (blocks > INT32_MAX) {
        sg_set_error("%lld pairs exceed one launch: score them in pieces", (long long)n_pairs);
        return SG_ERR_OVERFLOW;
    }
    if (A->rows_of) SG_TRY(sg_csr_ensure_rows(ctx, A));
    if (B->rows_of && B != A) SG_TRY(sg_csr_ensure_rows(ctx, B));
    const size_t s = A->dtype == SG_F64 ? 8 : 4, head = 16;   // the status word, then the results (aligned for either type)
    const size_t bytes = head + (size_t)n_pairs * s;
    Scratch tmp(ctx);
    char *d_buf = nullptr;
    SG_TRY(tmp.alloc(bytes, &d_buf));
    std::unique_ptr<char[]> h_buf(new (std::nothrow) char[bytes]);   // out_host stays untouched when the device refuses
    if (!h_buf) {
        sg_set_error("no host memory for %zu bytes of results", bytes);
        return SG_ERR_OOM;
    }
    SG_HIP_TRY(hipMemsetAsync(d_buf, 0, head, ctx->stream));
    by_dtype(A->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(pairs_dot_kernel<T>, dim3((unsigned)blocks), dim3(SG_PAIR_BLOCK), 0, ctx->stream, A->d_indptr,
                           A->d_indices, (const T *)A->d_data, A->n_rows, B->d_indptr, B->d_indices, (const T *)B->d_data,
                           B->n_rows, d_left, d_right, n_pairs, known_ascending(A) ? 0 : 1, known_ascending(B) ? 0 : 1,
                           (uint32_t *)d_buf, (T *)(d_buf + head));
        return SG_OK;
    });
    SG_HIP_TRY(hipGetLastError());
    SG_TRY(sg_fetch(ctx, h_buf.get(), d_buf, bytes));   // the one read-back: the status word comes with the results
    uint32_t status = 0;
    memcpy(&status, h_buf.get(), 4);
    if (status) {
        sg_set_error("bad argument: %s%s%s%s", status & SG_PAIR_BAD_LEFT ? "a left index lies outside A's rows; " : "",
                     status & SG_PAIR_BAD_RIGHT ? "a right index lies outside B's rows; " : "",
                     status & SG_PAIR_UNSORTED_A ? "a row of A that a pair names is not sorted by column (strictly ascending); " : "",
                     status & SG_PAIR_UNSORTED_B ? "a row of B that a pair names is not sorted by column (strictly ascending); " : "");
        return SG_ERR_BADARG;
    }
    memcpy(out_host, h_buf.get() + head, (size_t)n_pairs * s);
    return SG_OK;
}
