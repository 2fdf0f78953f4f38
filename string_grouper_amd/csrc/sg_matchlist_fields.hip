// Per-field scores of a match list (include/sg_hip.h: sg_matchlist_field_scores; DESIGN.md section 4, "Field scores of a
// list").  A record call's list holds the weighed sum of its fields; which field carried a pair is asked of the list while it
// lies on the device: plane f of the answer holds (A_f . B_f^T)[a, b] for every entry (i, j) of the list, in list order -- a, b
// the physical rows of the live numbers i, j -- in sg_csr_pairs_dot's arithmetic, by the walk of sg_pairs_device.h.
//
// One launch.  SG_PAIR_LANES lanes take a run of SG_PAIR_ROW_CHUNK consecutive ENTRIES, not a row: a symmetrised hub row holds
// thousands of entries and most rows a handful, and a run is the same work wherever it lies.  The group finds the row of its
// first entry by bisection in row_ptr and steps to the next row when its entry reaches that row's end, finding the row of A_f
// anew; the fields are looped over inside, so the run's columns are read from cache after the first field.  Lane 0 stores.
#include "sg_pairs_device.h"

#define SG_LIST_MAX_FIELDS 8

// status word of a call: bit 0 a column of the list outside [0, N); bit 1 + 2 f / 2 + 2 f a row of A_f / B_f that an entry
// reads and that is not in strictly ascending column order
#define SG_LIST_BAD_COLUMN 1u

template <typename T>
struct ListFields {
    PairField<T> f[SG_LIST_MAX_FIELDS];
};

// the row of entry q: the LAST row whose pointer is <= q (rows before it may be empty and share that pointer).
// row_ptr[0] = 0 <= q < n_entries = row_ptr[n_rows], so the answer lies in [0, n_rows)
__device__ __forceinline__ int64_t row_of_entry(const int64_t *__restrict__ row_ptr, int64_t n_rows, int64_t q) {
    int64_t lo = 0, hi = n_rows;   // the number of rows r in [0, n_rows) with row_ptr[r] <= q, found by bisection
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (row_ptr[mid] <= q) lo = mid + 1;
        else hi = mid;
    }
    return lo > 0 ? lo - 1 : 0;
}

template <typename T>
__global__ void __launch_bounds__(SG_PAIR_BLOCK) matchlist_fields_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ cols, int64_t n_rows, int64_t n_cols, int64_t n_entries,
    ListFields<T> fields, int32_t n_fields, uint32_t *status, T *__restrict__ out) {
    constexpr int G = SG_PAIR_LANES;
    const int l = threadIdx.x & (G - 1);
    const int group_shift = threadIdx.x & (SG_WAVE - 1) & ~(G - 1);   // the group's first lane in its wave
    const int64_t g = ((int64_t)blockIdx.x * SG_PAIR_BLOCK + threadIdx.x) / G;
    const int64_t q0 = g * SG_PAIR_ROW_CHUNK;
    if (q0 >= n_entries) return;   // (everything below is uniform over the group: its lanes leave, loop and shuffle together)
    const int64_t q1 = n_entries - q0 < SG_PAIR_ROW_CHUNK ? n_entries : q0 + SG_PAIR_ROW_CHUNK;
    const int64_t first = row_of_entry(row_ptr, n_rows, q0);
    for (int f = 0; f < n_fields; ++f) {
        const PairField<T> &F = fields.f[f];
        int64_t row = first, end = row_ptr[first + 1], a0, a1;
        pair_left_row<T>(F, row, l, status, 2u << (2 * f), a0, a1);
        for (int64_t q = q0; q < q1; ++q) {
            if (q >= end) {   // the run goes on in a later row: the next one that holds an entry
                while (q >= end && row + 1 < n_rows) end = row_ptr[++row + 1];
                pair_left_row<T>(F, row, l, status, 2u << (2 * f), a0, a1);
            }
            const int64_t j = cols[q];
            if (j < 0 || j >= n_cols) {   // nothing of a field is read for it; the call is refused
                if (l == 0 && f == 0) atomicOr(status, SG_LIST_BAD_COLUMN);
                continue;
            }
            const T s = pair_score<T>(F, a0, a1, j, l, group_shift, status, 4u << (2 * f));
            if (l == 0) out[(int64_t)f * n_entries + q] = s;
        }
    }
}

extern "C" int sg_matchlist_field_scores(sg_ctx *ctx, const sg_matchlist *ml, const sg_rescore_field *fields, int32_t n_fields,
                                         void *out_host) {
    SG_REQUIRE(ctx && ml, "null argument");
    SG_REQUIRE(n_fields >= 1 && n_fields <= SG_LIST_MAX_FIELDS, "between 1 and 8 fields are expected");
    SG_REQUIRE(fields != nullptr, "null argument");
    int64_t n_rows = 0, n_cols = 0, n_entries = 0;
    int32_t dtype = SG_F32;
    const int64_t *row_ptr = nullptr;
    const int32_t *cols = nullptr;
    const void *vals = nullptr;
    SG_TRY(sg_matchlist_device_view(ml, &n_rows, &n_cols, &n_entries, &dtype, &row_ptr, &cols, &vals));
    for (int f = 0; f < n_fields; ++f) SG_TRY(check_pair_field(fields[f], dtype, n_rows, n_cols, "a field's", "list", false));
    if (n_entries == 0) return SG_OK;   // an empty list is served: there is nothing to write
    SG_REQUIRE(out_host != nullptr, "null argument");
    const int64_t groups = (n_entries + SG_PAIR_ROW_CHUNK - 1) / SG_PAIR_ROW_CHUNK;
    if (pair_blocks(groups) > INT32_MAX) return exceeds_one_launch(n_entries, "entries of a list", "score");
    for (int f = 0; f < n_fields; ++f) SG_TRY(ensure_pair_rows(ctx, fields[f].A, fields[f].B));
    const size_t s = dtype == SG_F64 ? 8 : 4, head = 16;   // the status word, then the planes (aligned for either type)
    const size_t planes = (size_t)n_fields * (size_t)n_entries * s, bytes = head + planes;
    Scratch tmp(ctx);
    char *d_buf = nullptr;
    SG_TRY(tmp.alloc(bytes, &d_buf));
    std::unique_ptr<char[]> h_buf(new (std::nothrow) char[bytes]);   // out_host stays untouched when the device refuses
    if (!h_buf) {
        sg_set_error("no host memory for %zu bytes of field scores", bytes);
        return SG_ERR_OOM;
    }
    // (a refused column leaves its places unwritten: the planes are cleared with the status word)
    SG_HIP_TRY(hipMemsetAsync(d_buf, 0, bytes, ctx->stream));
    SG_TRY(by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        ListFields<T> dev;
        memset(&dev, 0, sizeof(dev));
        for (int f = 0; f < n_fields; ++f) dev.f[f] = make_pair_field<T>(fields[f]);
        hipLaunchKernelGGL(matchlist_fields_kernel<T>, dim3((unsigned)pair_blocks(groups)), dim3(SG_PAIR_BLOCK), 0, ctx->stream,
                           row_ptr, cols, n_rows, n_cols, n_entries, dev, n_fields, (uint32_t *)d_buf, (T *)(d_buf + head));
        return SG_OK;
    }));
    SG_HIP_TRY(hipGetLastError());
    SG_TRY(sg_fetch(ctx, h_buf.get(), d_buf, bytes));   // the one read-back: the status word comes with the planes
    uint32_t status = 0;
    memcpy(&status, h_buf.get(), 4);
    if (status) {
        std::string what;
        if (status & SG_LIST_BAD_COLUMN) what += "a column of the list lies outside the list's columns; ";
        for (int f = 0; f < n_fields; ++f) {
            const std::string field = "field " + std::to_string(f);
            if (status & (2u << (2 * f))) what += unsorted_row(field + "'s left matrix", "list entry reads");
            if (status & (4u << (2 * f))) what += unsorted_row(field + "'s right matrix", "list entry reads");
        }
        sg_set_error("bad argument: %s", what.c_str());
        return SG_ERR_BADARG;
    }
    memcpy(out_host, h_buf.get() + head, planes);
    return SG_OK;
}
