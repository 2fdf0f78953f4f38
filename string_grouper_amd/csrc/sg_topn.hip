// sg_topn.hip -- the result handle: a fixed-stride top-n result on the device (sg_topn: n_rows rows of `stride` slots, the
// first counts[r] of row r in use), what makes and frees one, what carries one to the host and back, and the two kernels that
// work on results alone:
//   topn_sort_by_col_kernel   every row of an unsorted result (sort == 0) re-ordered by ascending column
//   topn_zip_kernel           K5, the merge of column-block results (zip_sp_matmul_topn, string_grouper.py:746 of the
//                             reference): one wave per row, register top-n
// Nothing here multiplies: the multiply and the index are sg_spgemm_topn.hip, the operations of a resident corpus on its
// results sg_corpus.hip.
#include <math.h>

#include "sg_internal.h"

#include "sg_k4_device.h"

// Re-order every row of a fixed-stride result by ascending column (sort == 0).  One wave per row;
// dynamic LDS: stride * (4 + sizeof(T)) bytes.
template <typename T>
__global__ void __launch_bounds__(64) topn_sort_by_col_kernel(int32_t *cols, T *vals, const int32_t *cnt,
                                                              int64_t n_rows, int32_t stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *sv = reinterpret_cast<T *>(smem);
    int32_t *sc = reinterpret_cast<int32_t *>(smem + sizeof(T) * (size_t)stride);
    const int lane = threadIdx.x;
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int n = cnt[row];
        int32_t *rc = cols + (size_t)row * stride;
        T *rv = vals + (size_t)row * stride;
        for (int i = lane; i < n; i += 64) {   // rank by counting; columns of one row are distinct
            const int myc = rc[i];
            int rank = 0;
            for (int q = 0; q < n; ++q) rank += (rc[q] < myc);
            sc[rank] = myc;
            sv[rank] = rv[i];
        }
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            rc[i] = sc[i];
            rv[i] = sv[i];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// K5: merge of column-block results (zip_sp_matmul_topn).  One wave per row, register top-n.
template <typename T>
struct ZipPart {
    const int32_t *cols;
    const T *vals;
    const int32_t *cnt;
    int32_t stride;
    int32_t col_offset;
};

template <typename T>
__global__ void __launch_bounds__(64) topn_zip_kernel(const ZipPart<T> *__restrict__ parts, int32_t n_parts,
                                                      int64_t n_rows, int32_t keep, int32_t pass_off,
                                                      int32_t out_stride, int32_t *out_cols, T *out_vals,
                                                      int32_t *out_cnt) {
    const int lane = threadIdx.x;
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const size_t obase = (size_t)row * out_stride + pass_off;
        TopList<T> top;
        top.clear();
        T floor_s = INFINITY;
        int floor_c = -1;
        if (pass_off > 0) {
            if (out_cnt[row] < pass_off) continue;
            floor_s = out_vals[obase - 1];
            floor_c = out_cols[obase - 1];
        }
        for (int b = 0; b < n_parts; ++b) {
            const ZipPart<T> part = parts[b];
            const int n = part.cnt[row];
            for (int base = 0; base < n; base += 64) {
                T v = (T)0;
                int c = 0;
                const bool ok = base + lane < n;
                if (ok) {
                    v = part.vals[(size_t)row * part.stride + base + lane];
                    c = part.cols[(size_t)row * part.stride + base + lane] + part.col_offset;
                }
                uint64_t m = __ballot(ok);
                while (m) {
                    const int src = __builtin_ctzll(m);
                    m &= m - 1;
                    const T ns = wave_read<T>(v, src);
                    const int nc = wave_read<int>(c, src);
                    if (ns < floor_s || (ns == floor_s && nc > floor_c)) top.insert(ns, nc, lane);
                }
            }
        }
        int cnt = __popcll(__ballot(top.c != INT32_MAX));
        if (cnt > keep) cnt = keep;
        if (lane < cnt) {
            out_vals[obase + lane] = top.s;
            out_cols[obase + lane] = top.c;
        }
        if (lane == 0) out_cnt[row] = pass_off + cnt;
    }
}

// ================================================================================================
// host side
// ================================================================================================
// an empty result of the given shape (rows, columns, stride): the three arrays, nothing written
int topn_alloc(sg_ctx *ctx, int64_t n_rows, int64_t n_cols, int32_t stride, int32_t dtype, TopnPtr *out) {
    TopnPtr r(new (std::nothrow) sg_topn());
    if (!r) return SG_ERR_OOM;
    r->ctx = ctx;
    r->n_rows = n_rows;
    r->n_cols = n_cols;
    r->stride = stride;
    r->dtype = dtype;
    const size_t cells = (size_t)n_rows * (size_t)stride + 64;
    SG_TRY(sg_alloc(ctx, cells, &r->d_cols));
    SG_TRY(ctx->alloc(cells * (dtype == SG_F64 ? 8 : 4), &r->d_vals));
    SG_TRY(sg_alloc(ctx, (size_t)n_rows + 64, &r->d_counts));
    *out = std::move(r);
    return SG_OK;
}

// The result's stride -- top_n, cut at the n_cols columns there are (at least one) -- and whether n_rows rows of it fit the
// 32-bit result index
bool result_stride(int64_t n_rows, int64_t top_n, int64_t n_cols, int32_t *stride) {
    *stride = (int32_t)(top_n < n_cols ? top_n : (n_cols > 0 ? n_cols : 1));
    return (double)n_rows * (double)*stride <= 2.0e9;
}

int result_overflow(int64_t n_rows, int32_t stride, const char *advice) {
    sg_set_error("result of %lld rows x top_n %lld does not fit the 32-bit result index%s", (long long)n_rows, (long long)stride,
                 advice);
    return SG_ERR_OVERFLOW;
}

// Every row of an unsorted result (sort == 0) re-ordered by ascending column
int sort_rows_by_column(sg_ctx *ctx, sg_topn *r) {
    if (r->n_rows <= 0) return SG_OK;
    const unsigned grid = (unsigned)(r->n_rows < 65535 * 16 ? r->n_rows : 65535 * 16);
    const size_t lds = (size_t)r->stride * (4 + (r->dtype == SG_F64 ? 8 : 4));
    if (lds > 64 * 1024) {
        sg_set_error("sort=0 with top_n=%d is not supported", r->stride);
        return SG_ERR_UNSUPPORTED;
    }
    return by_dtype(r->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(topn_sort_by_col_kernel<T>, dim3(grid), dim3(64), lds, ctx->stream, r->d_cols, (T *)r->d_vals,
                           r->d_counts, r->n_rows, r->stride);
        return SG_OK;
    });
}

extern "C" int sg_topn_dims(const sg_topn *r, int64_t *n_rows, int32_t *stride, int32_t *dtype, int64_t *n_cols) {
    SG_REQUIRE(r != nullptr, "result is null");
    if (n_rows) *n_rows = r->n_rows;
    if (stride) *stride = r->stride;
    if (dtype) *dtype = r->dtype;
    if (n_cols) *n_cols = r->n_cols;
    return SG_OK;
}

extern "C" int sg_topn_device_ptrs(const sg_topn *r, const int32_t **d_cols, const void **d_vals,
                                   const int32_t **d_counts) {
    SG_REQUIRE(r != nullptr, "result is null");
    if (d_cols) *d_cols = r->d_cols;
    if (d_vals) *d_vals = r->d_vals;
    if (d_counts) *d_counts = r->d_counts;
    return SG_OK;
}

extern "C" int sg_topn_to_host(sg_ctx *ctx, const sg_topn *r, int32_t *cols, void *vals, int32_t *counts) {
    SG_REQUIRE(ctx && r && counts, "null argument");
    const size_t cells = (size_t)r->n_rows * (size_t)r->stride;
    const size_t s = r->dtype == SG_F64 ? 8 : 4;
    if (cells > 0) {
        SG_REQUIRE(cols && vals, "null output");
        SG_HIP_TRY(hipMemcpyAsync(cols, r->d_cols, cells * 4, hipMemcpyDeviceToHost, ctx->stream));
        SG_HIP_TRY(hipMemcpyAsync(vals, r->d_vals, cells * s, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (r->n_rows > 0)
        SG_HIP_TRY(hipMemcpyAsync(counts, r->d_counts, (size_t)r->n_rows * 4, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SG_OK;
}

extern "C" int sg_topn_counts_to_host(sg_ctx *ctx, const sg_topn *r, int32_t *counts) {
    SG_REQUIRE(ctx && r && counts, "null argument");
    if (r->n_rows > 0)
        SG_HIP_TRY(hipMemcpyAsync(counts, r->d_counts, (size_t)r->n_rows * 4, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SG_OK;
}

// a new result filled from the caller's three arrays (`kind`: where they lie)
static int topn_from(sg_ctx *ctx, int64_t n_rows, int64_t n_cols, int32_t stride, int32_t dtype, const int32_t *cols,
                     const void *vals, const int32_t *counts, hipMemcpyKind kind, TopnPtr *out) {
    SG_TRY(topn_alloc(ctx, n_rows, n_cols, stride, dtype, out));
    const size_t cells = (size_t)n_rows * (size_t)stride;
    if (cells == 0) return SG_OK;
    sg_topn *r = out->get();
    SG_HIP_TRY(hipMemcpyAsync(r->d_cols, cols, cells * 4, kind, ctx->stream));
    SG_HIP_TRY(hipMemcpyAsync(r->d_vals, vals, cells * (dtype == SG_F64 ? 8 : 4), kind, ctx->stream));
    SG_HIP_TRY(hipMemcpyAsync(r->d_counts, counts, (size_t)n_rows * 4, kind, ctx->stream));
    return SG_OK;
}

extern "C" int sg_topn_from_host(sg_ctx *ctx, int64_t n_rows, int64_t n_cols, int32_t stride, int32_t dtype,
                                 const int32_t *cols, const void *vals, const int32_t *counts, sg_topn **out) {
    SG_REQUIRE(ctx && counts && out && n_rows >= 0 && stride >= 1, "bad argument");
    SG_REQUIRE(dtype == SG_F32 || dtype == SG_F64, "dtype must be SG_F32 or SG_F64");
    TopnPtr r;
    SG_TRY(topn_from(ctx, n_rows, n_cols, stride, dtype, cols, vals, counts, hipMemcpyHostToDevice, &r));
    SG_HIP_TRY(hipStreamSynchronize(ctx->stream));   // the caller's arrays are free again
    *out = r.release();
    return SG_OK;
}

extern "C" int sg_topn_from_device(sg_ctx *ctx, int64_t n_rows, int64_t n_cols, int32_t stride, int32_t dtype,
                                   const int32_t *d_cols, const void *d_vals, const int32_t *d_counts, sg_topn **out) {
    SG_REQUIRE(ctx && d_counts && out && n_rows >= 0 && stride >= 1, "bad argument");
    SG_REQUIRE(dtype == SG_F32 || dtype == SG_F64, "dtype must be SG_F32 or SG_F64");
    TopnPtr r;
    SG_TRY(topn_from(ctx, n_rows, n_cols, stride, dtype, d_cols, d_vals, d_counts, hipMemcpyDeviceToDevice, &r));
    *out = r.release();
    return SG_OK;
}

extern "C" int sg_topn_free(sg_topn *r) {
    if (!r) return SG_OK;
    r->ctx->release(r->d_cols);
    r->ctx->release(r->d_vals);
    r->ctx->release(r->d_counts);
    delete r;
    return SG_OK;
}

extern "C" int sg_topn_zip(sg_ctx *ctx, const sg_topn *const *parts, const int64_t *col_offsets, int32_t n_parts,
                           int32_t top_n, sg_topn **out) {
    SG_REQUIRE(ctx && parts && col_offsets && out && n_parts >= 1 && top_n >= 1, "bad argument");
    const int64_t n_rows = parts[0]->n_rows;
    const int32_t dtype = parts[0]->dtype;
    int64_t total_cols = 0, total_stride = 0;
    for (int b = 0; b < n_parts; ++b) {
        SG_REQUIRE(parts[b] && parts[b]->n_rows == n_rows && parts[b]->dtype == dtype, "parts disagree in shape/dtype");
        const int64_t end = col_offsets[b] + parts[b]->n_cols;
        if (end > total_cols) total_cols = end;
        total_stride += parts[b]->stride;
    }
    if (total_cols > INT32_MAX) {
        sg_set_error("zipped column count exceeds int32");
        return SG_ERR_OVERFLOW;
    }
    int64_t stride64 = top_n < total_stride ? top_n : total_stride;
    if (stride64 < 1) stride64 = 1;
    const int32_t stride = (int32_t)stride64;
    TopnPtr r;
    SG_TRY(topn_alloc(ctx, n_rows, total_cols, stride, dtype, &r));
    return by_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        // part descriptors: host-pinned scratch would add a dependency; a tiny pooled device buffer + sync copy
        std::vector<ZipPart<T>> desc((size_t)n_parts);
        for (int b = 0; b < n_parts; ++b)
            desc[b] = ZipPart<T>{parts[b]->d_cols, (const T *)parts[b]->d_vals, parts[b]->d_counts, parts[b]->stride,
                                 (int32_t)col_offsets[b]};
        Scratch scratch(ctx);
        ZipPart<T> *d_desc = nullptr;
        SG_TRY(scratch.alloc(desc.size(), &d_desc));
        SG_HIP_TRY(hipMemcpyAsync(d_desc, desc.data(), desc.size() * sizeof(ZipPart<T>), hipMemcpyHostToDevice, ctx->stream));
        SG_HIP_TRY(hipStreamSynchronize(ctx->stream));   // desc is a local
        SG_HIP_TRY(hipMemsetAsync(r->d_counts, 0, sizeof(int32_t) * (size_t)n_rows, ctx->stream));
        {
            SgTimer timer(ctx, SG_K_ZIP);
            const int n_pass = (stride + SG_TOPN_LANES - 1) / SG_TOPN_LANES;
            const unsigned grid = (unsigned)(n_rows < 256 * 32 ? (n_rows > 0 ? n_rows : 1) : 256 * 32);
            for (int pass = 0; pass < n_pass && n_rows > 0; ++pass) {
                const int pass_off = pass * SG_TOPN_LANES;
                const int keep = stride - pass_off < SG_TOPN_LANES ? stride - pass_off : SG_TOPN_LANES;
                hipLaunchKernelGGL(topn_zip_kernel<T>, dim3(grid), dim3(64), 0, ctx->stream, (const ZipPart<T> *)d_desc, n_parts,
                                   n_rows, keep, pass_off, stride, r->d_cols, (T *)r->d_vals, r->d_counts);
            }
        }
        SG_HIP_TRY(hipGetLastError());
        *out = r.release();
        return SG_OK;
    });
}
