// Pair similarities -- the score of NAMED row pairs: out[p] = (A . B^T)[left[p], right[p]], the element the top-n multiply
// (K4 / K4p, string_grouper.py:725-743) would report for that pair, in the multiply's arithmetic:
//     acc = +0.0;  for every column k that both rows hold, ascending:  acc = rn(acc + rn(A[i, k] * B[j, k]))
// -- every product and every sum rounded on its own, zero products added like any other (a lone product of -0.0 gives +0.0),
// no common column or an empty row: +0.0.  It is NOT K9's arithmetic (sg_reduce.hip: non-zero products, numpy's pairwise
// sum), which is what compute_pairwise_similarities (string_grouper.py:55) gives for the same pair.  No gate: values of any
// sign, NaN and inf flow through.
//
// Lanes ("Pair similarities"): SG_PAIR_LANES = 8 lanes a pair, eight pairs a wave, and the walk of
// sg_pairs_device.h -- the left row, then the one column the pair names -- over a field without dead lists.
#include "sg_pairs_device.h"

// status word of a call, one bit a cause
#define SG_PAIR_BAD_LEFT 1u       // an entry of `left` outside [0, rows of A)
#define SG_PAIR_BAD_RIGHT 2u      // an entry of `right` outside [0, rows of B)
#define SG_PAIR_UNSORTED_A 4u     // a row of A that some pair reads is not in strictly ascending column order
#define SG_PAIR_UNSORTED_B 8u

template <typename T>
__global__ void __launch_bounds__(SG_PAIR_BLOCK) pairs_dot_kernel(PairField<T> F, int64_t n_a, int64_t n_b,
                                                                  const int32_t *__restrict__ left,
                                                                  const int32_t *__restrict__ right, int64_t n_pairs,
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
    int64_t a0, a1;
    pair_left_row<T>(F, i, l, status, SG_PAIR_UNSORTED_A, a0, a1);
    const T acc = pair_score<T>(F, a0, a1, j, l, group_shift, status, SG_PAIR_UNSORTED_B);
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
    if (pair_blocks(n_pairs) > INT32_MAX) return exceeds_one_launch(n_pairs, "pairs", "score");
    SG_TRY(ensure_pair_rows(ctx, A, B));
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
    const sg_rescore_field field = {A, B, 1.0, nullptr, 0, nullptr, 0};   // (no dead lists: the pairs name physical rows)
    by_dtype(A->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(pairs_dot_kernel<T>, dim3((unsigned)pair_blocks(n_pairs)), dim3(SG_PAIR_BLOCK), 0, ctx->stream,
                           make_pair_field<T>(field), A->n_rows, B->n_rows, d_left, d_right, n_pairs, (uint32_t *)d_buf,
                           (T *)(d_buf + head));
        return SG_OK;
    });
    SG_HIP_TRY(hipGetLastError());
    SG_TRY(sg_fetch(ctx, h_buf.get(), d_buf, bytes));   // the one read-back: the status word comes with the results
    uint32_t status = 0;
    memcpy(&status, h_buf.get(), 4);
    if (status) {
        std::string what;
        if (status & SG_PAIR_BAD_LEFT) what += "a left index lies outside A's rows; ";
        if (status & SG_PAIR_BAD_RIGHT) what += "a right index lies outside B's rows; ";
        if (status & SG_PAIR_UNSORTED_A) what += unsorted_row("A", "pair names");
        if (status & SG_PAIR_UNSORTED_B) what += unsorted_row("B", "pair names");
        sg_set_error("bad argument: %s", what.c_str());
        return SG_ERR_BADARG;
    }
    memcpy(out_host, h_buf.get() + head, (size_t)n_pairs * s);
    return SG_OK;
}
