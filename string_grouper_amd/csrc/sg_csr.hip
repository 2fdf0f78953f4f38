// sg_csr.hip -- the one place a CSR matrix is made, viewed and freed: csr_alloc (an owned matrix, three arrays, nothing
// written), csr_view / csr_row_view (an unowned copy of the struct), csr_inherit (what a derived matrix carries over from
// its source), and the handle's API (sg_csr_from_host ... sg_csr_free).  Host code only: no kernel lives here.
#include "sg_internal.h"

static size_t dtype_size(int32_t dtype) { return dtype == SG_F64 ? 8 : 4; }

// ------------------------------------------------------------------------------------ maker
int csr_alloc(sg_ctx *ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, int32_t dtype, CsrSlack slack, CsrPtr *out,
              int64_t *indptr) {
    CsrPtr m(new (std::nothrow) sg_csr());
    if (!m) {
        ctx->release(indptr);
        return SG_ERR_OOM;
    }
    m->ctx = ctx;
    m->n_rows = n_rows;
    m->n_cols = n_cols;
    m->nnz = nnz;
    m->dtype = dtype;
    m->owned = true;
    m->d_indptr = indptr;     // (the matrix's from here on: it goes back with it)
    int32_t *idx = nullptr;
    void *val = nullptr;
    if (!indptr) {
        SG_TRY(sg_alloc(ctx, (size_t)n_rows + slack.rows, &indptr));
        m->d_indptr = indptr;
    }
    SG_TRY(sg_alloc(ctx, (size_t)nnz + slack.entries, &idx));
    m->d_indices = idx;
    SG_TRY(ctx->alloc(((size_t)nnz + slack.entries) * dtype_size(dtype), &val));
    m->d_data = val;
    *out = std::move(m);
    return SG_OK;
}

// ------------------------------------------------------------------------------------ views
// The struct copied, the arrays the owner's.  What the OWNER caches per handle is reset here and nowhere else: its groups of
// identical rows are indexed by the owner's rows, and sg_csr_free of a copy that still pointed at them would free them under
// the owner.
static sg_csr unowned_copy(const sg_csr &m) {
    sg_csr c = m;
    c.owned = false;
    c.left_groups = nullptr;
    c.left_state = 0;
    return c;
}

sg_csr csr_view(const sg_csr &m) {
    sg_csr c = unowned_copy(m);
    c.d_props_words = nullptr;
    return c;
}

sg_csr csr_row_view(const sg_csr &m, int64_t r0, int64_t r1) {
    sg_csr v = unowned_copy(m);
    v.n_rows = r1 - r0;
    v.d_indptr = m.d_indptr + r0;
    if (m.d_row_norm) v.d_row_norm = m.d_row_norm + r0;   // (the parent's array: a view frees nothing)
    return v;
}

// ------------------------------------------------------------------------------------ inheritance
CsrCarries csr_inherit(sg_csr *dst, const sg_csr *const *src, int n_src, CsrDerived kind) {
    const sg_csr *s = src[0];
    CsrCarries carries;
    switch (kind) {
    case CsrDerived::permuted:
        dst->props_repeated_column = s->props_repeated_column;
        [[fallthrough]];
    case CsrDerived::representatives:
        dst->props_state = s->props_state;
        dst->props_max_norm2 = s->props_max_norm2;
        dst->props_max_nnz = s->props_max_nnz;
        break;
    case CsrDerived::selected:
        carries.norms = s->d_row_norm != nullptr;
        [[fallthrough]];
    case CsrDerived::taken:
        dst->from_vectoriser = s->from_vectoriser;
        carries.words = s->from_vectoriser && s->d_props_words != nullptr;
        break;
    case CsrDerived::stacked: {
        bool all_vec = true, all_words = true, all_norms = true;
        for (int p = 0; p < n_src; ++p) {
            all_vec = all_vec && src[p]->from_vectoriser;
            all_words = all_words && src[p]->d_props_words != nullptr;
            all_norms = all_norms && src[p]->d_row_norm != nullptr;
        }
        dst->from_vectoriser = all_vec;
        carries.words = all_vec && all_words;
        carries.norms = all_norms;
        break;
    }
    case CsrDerived::reweighed:
        dst->from_vectoriser = true;   // (counts times positive weights, every row divided by its norm)
        carries.words = carries.norms = true;
        break;
    }
    return carries;
}

// ------------------------------------------------------------------------------------ the handle's API
extern "C" int sg_csr_from_host(sg_ctx *ctx, int64_t n_rows, int64_t n_cols, const int64_t *indptr,
                                const int32_t *indices, const void *data, int32_t dtype, sg_csr **out) {
    SG_REQUIRE(ctx && indptr && out, "null argument");
    SG_REQUIRE(n_rows >= 0 && n_cols >= 0, "negative shape");
    SG_REQUIRE(dtype == SG_F32 || dtype == SG_F64, "dtype must be SG_F32 or SG_F64");
    SG_REQUIRE(indptr[0] == 0, "indptr must start at 0");
    const int64_t nnz = indptr[n_rows];
    SG_REQUIRE(nnz >= 0 && (nnz == 0 || (indices && data)), "bad nnz");
    if (n_cols > INT32_MAX || n_rows > INT32_MAX) {
        sg_set_error("matrix shape (%lld x %lld) exceeds int32 indices", (long long)n_rows, (long long)n_cols);
        return SG_ERR_OVERFLOW;
    }
    CsrPtr m;
    SG_TRY(csr_alloc(ctx, n_rows, n_cols, nnz, dtype, CSR_SLACK_COPY, &m));
    SG_HIP_TRY(hipMemcpyAsync((void *)m->d_indptr, indptr, sizeof(int64_t) * (size_t)(n_rows + 1), hipMemcpyHostToDevice,
                              ctx->stream));
    if (nnz > 0) {
        SG_HIP_TRY(hipMemcpyAsync((void *)m->d_indices, indices, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice,
                                  ctx->stream));
        SG_HIP_TRY(hipMemcpyAsync((void *)m->d_data, data, dtype_size(dtype) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream));
    }
    SG_HIP_TRY(hipStreamSynchronize(ctx->stream));
    *out = m.release();
    return SG_OK;
}

extern "C" int sg_csr_from_device(sg_ctx *ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *d_indptr,
                                  const int32_t *d_indices, const void *d_data, int32_t dtype, sg_csr **out) {
    SG_REQUIRE(ctx && d_indptr && out, "null argument");
    SG_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0, "negative shape");
    SG_REQUIRE(dtype == SG_F32 || dtype == SG_F64, "dtype must be SG_F32 or SG_F64");
    if (n_cols > INT32_MAX || n_rows > INT32_MAX) {
        sg_set_error("matrix shape exceeds int32 indices");
        return SG_ERR_OVERFLOW;
    }
    sg_csr *m = new (std::nothrow) sg_csr();   // (the caller's arrays: nothing to allocate, nothing that can fail behind this)
    if (!m) return SG_ERR_OOM;
    m->ctx = ctx;
    m->n_rows = n_rows;
    m->n_cols = n_cols;
    m->nnz = nnz;
    m->dtype = dtype;
    m->d_indptr = d_indptr;
    m->d_indices = d_indices;
    m->d_data = d_data;
    m->owned = false;
    *out = m;
    return SG_OK;
}

extern "C" int sg_csr_dims(const sg_csr *m, int64_t *n_rows, int64_t *n_cols, int64_t *nnz, int32_t *dtype) {
    SG_REQUIRE(m != nullptr, "matrix is null");
    if (n_rows) *n_rows = m->n_rows;
    if (n_cols) *n_cols = m->n_cols;
    if (nnz) *nnz = m->nnz;
    if (dtype) *dtype = m->dtype;
    return SG_OK;
}

extern "C" int sg_csr_device_ptrs(const sg_csr *m, const int64_t **d_indptr, const int32_t **d_indices,
                                  const void **d_data) {
    SG_REQUIRE(m != nullptr, "matrix is null");
    if (d_indptr) *d_indptr = m->d_indptr;
    if (d_indices) *d_indices = m->d_indices;
    if (d_data) *d_data = m->d_data;
    return SG_OK;
}

extern "C" int sg_csr_row_norms(const sg_csr *m, const double **d_norms) {
    SG_REQUIRE(m && d_norms, "null argument");
    *d_norms = m->d_row_norm;
    return SG_OK;
}

extern "C" int sg_csr_vectoriser_words(sg_ctx *ctx, const sg_csr *m, uint32_t *words, int32_t *present) {
    SG_REQUIRE(ctx && m && words && present, "null argument");
    *present = m->d_props_words != nullptr;
    words[0] = words[1] = words[2] = 0;
    if (m->d_props_words) {
        SG_TRY(sg_fetch(ctx, ctx->h_fetch, m->d_props_words, 12));
        memcpy(words, ctx->h_fetch, 12);
    }
    return SG_OK;
}

extern "C" int sg_csr_to_host(sg_ctx *ctx, const sg_csr *m, int64_t *indptr, int32_t *indices, void *data) {
    SG_REQUIRE(ctx && m && indptr, "null argument");
    SG_HIP_TRY(hipMemcpyAsync(indptr, m->d_indptr, sizeof(int64_t) * (size_t)(m->n_rows + 1), hipMemcpyDeviceToHost,
                              ctx->stream));
    SG_HIP_TRY(hipStreamSynchronize(ctx->stream));
    // a row-block view has absolute offsets: copy [indptr[0], indptr[n]) and rebase
    const int64_t base = indptr[0];
    const int64_t nnz = indptr[m->n_rows] - base;
    if (nnz > 0) {
        SG_REQUIRE(indices && data, "null output");
        SG_HIP_TRY(hipMemcpyAsync(indices, m->d_indices + base, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost,
                                  ctx->stream));
        SG_HIP_TRY(hipMemcpyAsync(data, (const char *)m->d_data + dtype_size(m->dtype) * (size_t)base,
                                  dtype_size(m->dtype) * (size_t)nnz, hipMemcpyDeviceToHost, ctx->stream));
        SG_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (base != 0)
        for (int64_t i = 0; i <= m->n_rows; ++i) indptr[i] -= base;
    return SG_OK;
}

extern "C" int sg_csr_row_block(sg_ctx *ctx, const sg_csr *m, int64_t r0, int64_t r1, sg_csr **out) {
    SG_REQUIRE(ctx && m && out, "null argument");
    SG_REQUIRE(0 <= r0 && r0 <= r1 && r1 <= m->n_rows, "row range out of bounds");
    CsrPtr v(new (std::nothrow) sg_csr(csr_row_view(*m, r0, r1)));
    if (!v) return SG_ERR_OOM;
    int64_t ends[2] = {0, 0};
    SG_HIP_TRY(hipMemcpyAsync(&ends[0], m->d_indptr + r0, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP_TRY(hipMemcpyAsync(&ends[1], m->d_indptr + r1, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP_TRY(hipStreamSynchronize(ctx->stream));
    v->nnz = ends[1] - ends[0];
    *out = v.release();
    return SG_OK;
}

extern "C" int sg_csr_free(sg_csr *m) {
    if (!m) return SG_OK;
    if (m->left_groups) sg_collapse_free(m->left_groups);
    if (m->owned) {
        m->ctx->release((void *)m->d_indptr);
        m->ctx->release((void *)m->d_indices);
        m->ctx->release((void *)m->d_data);
        m->ctx->release(m->d_props_words);
        m->ctx->release(m->d_row_norm);
    }
    delete m;
    return SG_OK;
}
