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
#include "sg_pairs_device.h"   // the merge itself (pair_rows_dot), shared with sg_rescore.hip

#define SG_PAIR_BLOCK 256   // 32 pairs a block

// status word of a call, one bit a cause
#define SG_PAIR_BAD_LEFT 1u       // an entry of `left` outside [0, rows of A)
#define SG_PAIR_BAD_RIGHT 2u      // an entry of `right` outside [0, rows of B)
#define SG_PAIR_UNSORTED_A 4u     // a row of A that some pair reads is not in strictly ascending column order
#define SG_PAIR_UNSORTED_B 8u

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

    const T acc = pair_rows_dot<T>(a_indices, a_data, a0, a1, b_indices, b_data, b0, b1, l, group_shift);
    if (l == 0) out[p] = acc;
}

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
