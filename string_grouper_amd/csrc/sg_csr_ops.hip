// sg_csr_ops.hip -- operations on whole CSR matrices on the device: sg_csr_concat, the rows of several matrices in one, and
// sg_csr_select_rows, a matrix without some of its rows.
//
// The reference stacks transformed blocks on the host: scipy's vstack (string_grouper.py:750 does it for the blocks of a
// result; a master list that grows would vstack the rows of master_matrix and the transform of the new strings).  A resident
// corpus keeps its rows in HBM and an inverted index borrows the arrays of the matrix it was built
// over, so growing the corpus means a NEW matrix: rows of parts[0], then parts[1], ...
//
// One kernel, one pass over the bytes, nothing read back:
//   csr_concat_kernel   (a) row pointers: out[row_off[p] + i] = indptr_p[i] - indptr_p[0] + nnz_off[p] -- a row-block view
//                           holds absolute offsets into its parent's arrays, so every part is rebased by its own first entry,
//                           which the kernel reads where it lies;
//                       (b) column indices and values in units of four OUTPUT entries: the 16-byte (f64 values: 2 x 16-byte)
//                           stores are aligned whatever the parts' sizes, the loads are 16 bytes wide at the alignment the
//                           source happens to have (the hardware takes any); a unit that straddles two parts, and the tail,
//                           go entry by entry.  The part of an entry: binary search over the <= n_parts offsets.
//                       (c) when every part carries the words the vectoriser leaves (violations, max ||row||^2, longest
//                           row), thread 0 merges them: sum, max, max.
//
// sg_csr_select_rows is scipy's m[keep] for a corpus that forgets rows ("A corpus that forgets").  Between two
// dropped rows the kept rows are CONTIGUOUS in the source, so a selection is a concatenation of the gaps of ONE matrix:
//   csr_select_gaps_kernel   one workgroup: checks the sorted drop list (ascending, distinct, inside the matrix) and writes
//                            a part descriptor per gap -- its first row pointer, the kept rows before it (first row - gap
//                            number) and the kept entries before it (a scan over the <= n_drop + 1 gaps' sizes, which it
//                            reads from the source's row pointers) -- and the totals, the only thing read back: they size
//                            the result;
//   csr_select_kernel        (a) and (b) above over those descriptors; the vectoriser's words are the source's own.
//
// sg_csr_take_rows is scipy's m[rows] for a list in any order ("A self-join that is kept": the rows whose kept
// result has to be computed again).  A taken row is a part of one row:
//   csr_take_parts_kernel    one workgroup: checks the list (every row inside the matrix) and writes a part descriptor per
//                            taken row -- its row pointer, its place k and the entries before it (the same scan, over the rows'
//                            sizes) -- and the total, the only thing read back;
//   csr_select_kernel        as above.
//
// The norms K2 divided the rows by (sg_csr::d_row_norm) travel with the rows BESIDE these kernels, which stay as they are: a
// concatenation copies every part's array device to device on the context's stream (a row-block view's pointer is the parent's,
// shifted by the view's first row), sg_csr_select_rows gathers them past the dropped rows with one small kernel over the gaps'
// descriptors (gather_row_norms_kernel).  A result carries norms only when every source row had one; sg_csr_take_rows' never does.
#include "sg_internal.h"

#include <memory>
#include <vector>

namespace {

constexpr int CONCAT_BLOCK = 256;
constexpr int CONCAT_UNIT = 4;                // output entries per thread and step

struct ConcatPart {
    const int64_t *indptr;                    // n_rows + 1 absolute offsets into indices / data
    const int32_t *indices;
    const void *data;
    const uint32_t *props;                    // the vectoriser's three words, or null
    int64_t row_off;                          // rows of the parts before this one
    int64_t nnz_off;                          // entries of the parts before this one
};
// parts[n_parts] is a sentinel: row_off = all rows, nnz_off = all entries

// the part that holds position x of a prefix array (the last p with off[p] <= x; empty parts share an offset with their
// successor and are skipped by taking the LAST)
template <bool ROWS>
__device__ inline int part_of(const ConcatPart *__restrict__ parts, int n_parts, int64_t x) {
    int lo = 0, hi = n_parts - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int64_t off = ROWS ? parts[mid].row_off : parts[mid].nnz_off;
        if (off <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// 16 bytes of a source array at the alignment of its entries.  The descriptors' pointers come out of memory, so the compiler
// knows no address space for them: said to be global here, the loads are global_load_dwordx4 instead of flat loads.
#define SG_GLOBAL __attribute__((address_space(1)))
typedef uint32_t Words4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t Words4x8 __attribute__((ext_vector_type(4), aligned(8)));
template <typename V, typename U>
__device__ inline uint4 load16(const U *src) {
    const V v = *reinterpret_cast<const SG_GLOBAL V *>((const SG_GLOBAL U *)src);
    return make_uint4(v.x, v.y, v.z, v.w);
}
template <typename U>
__device__ inline U load_global(const U *src) {
    return *(const SG_GLOBAL U *)src;
}

// (a) and (b) of the header: the row pointers, then the indices and values, of the parts one after the other
template <typename T>
__device__ inline void copy_parts(const ConcatPart *__restrict__ parts, int n_parts, int64_t *__restrict__ out_indptr,
                                  int32_t *__restrict__ out_indices, T *__restrict__ out_data, int64_t tid, int64_t step) {
    const int64_t n_rows = parts[n_parts].row_off;
    const int64_t nnz = parts[n_parts].nnz_off;

    // (a) row pointers
    for (int64_t r = tid; r < n_rows; r += step) {
        const int p = part_of<true>(parts, n_parts, r);
        const int64_t *ip = parts[p].indptr;
        out_indptr[r] = load_global(ip + (r - parts[p].row_off)) - load_global(ip) + parts[p].nnz_off;
    }
    if (tid == 0) out_indptr[n_rows] = nnz;

    // (b) indices and values, four output entries a step
    const int64_t n_units = (nnz + CONCAT_UNIT - 1) / CONCAT_UNIT;
    for (int64_t u = tid; u < n_units; u += step) {
        const int64_t e0 = u * CONCAT_UNIT;
        int p = part_of<false>(parts, n_parts, e0);
        const int64_t src0 = load_global(parts[p].indptr) + (e0 - parts[p].nnz_off);
        if (e0 + CONCAT_UNIT <= parts[p + 1].nnz_off) {          // the whole unit lies in part p (and so below nnz)
            *reinterpret_cast<uint4 *>(out_indices + e0) = load16<Words4>(parts[p].indices + src0);
            const T *src = (const T *)parts[p].data + src0;
            uint4 *dst = reinterpret_cast<uint4 *>(out_data + e0);
            if (sizeof(T) == 4) {
                dst[0] = load16<Words4>(src);
            } else {
                const uint4 d0 = load16<Words4x8>(src), d1 = load16<Words4x8>(src + 2);
                dst[0] = d0;
                dst[1] = d1;
            }
        } else {
            const int64_t e1 = e0 + CONCAT_UNIT < nnz ? e0 + CONCAT_UNIT : nnz;
            for (int64_t e = e0; e < e1; ++e) {
                while (e >= parts[p + 1].nnz_off) ++p;           // (e < nnz = the sentinel's offset: p stays < n_parts)
                const int64_t s = load_global(parts[p].indptr) + (e - parts[p].nnz_off);
                out_indices[e] = load_global(parts[p].indices + s);
                out_data[e] = load_global((const T *)parts[p].data + s);
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(CONCAT_BLOCK) csr_concat_kernel(const ConcatPart *__restrict__ parts, int n_parts,
                                                                  int64_t *__restrict__ out_indptr,
                                                                  int32_t *__restrict__ out_indices,
                                                                  T *__restrict__ out_data,
                                                                  uint32_t *__restrict__ out_props) {
    const int64_t tid = (int64_t)blockIdx.x * CONCAT_BLOCK + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * CONCAT_BLOCK;
    copy_parts<T>(parts, n_parts, out_indptr, out_indices, out_data, tid, step);

    // (c) the vectoriser's words
    if (out_props != nullptr && tid == 0) {
        uint32_t bad = 0, norm2 = 0, longest = 0;                // (a squared norm is >= 0: its float bits order as integers)
        for (int p = 0; p < n_parts; ++p) {
            const uint32_t *w = parts[p].props;
            bad += load_global(w);
            norm2 = max(norm2, load_global(w + 1));
            longest = max(longest, load_global(w + 2));
        }
        out_props[0] = bad;
        out_props[1] = norm2;
        out_props[2] = longest;
        out_props[3] = 0;
    }
}

// One round of the descriptors' scan, by every thread of the one workgroup: the sizes of the CONCAT_BLOCK parts of this round
// summed in LDS; returns the entries before this thread's part (the rounds before in *carry, which moves on by the round's sum)
__device__ inline int64_t sizes_before(int64_t *scan, int64_t *carry, int tid, int64_t len) {
    scan[tid] = len;
    __syncthreads();
    for (int off = 1; off < CONCAT_BLOCK; off <<= 1) {
        const int64_t v = tid >= off ? scan[tid - off] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const int64_t before = *carry + scan[tid] - len;
    __syncthreads();
    if (tid == CONCAT_BLOCK - 1) *carry += scan[tid];
    __syncthreads();
    return before;
}

// ---- sg_csr_select_rows: the gaps between the dropped rows as parts of a concatenation.  info[0] = kept entries,
// info[1] != 0: the drop list is not ascending, not distinct or names a row outside the matrix (nothing else is written).
__global__ void __launch_bounds__(CONCAT_BLOCK) csr_select_gaps_kernel(const int64_t *__restrict__ indptr,
                                                                       const int32_t *__restrict__ indices,
                                                                       const void *__restrict__ data, int64_t n_rows,
                                                                       const int32_t *__restrict__ drop, int64_t n_drop,
                                                                       ConcatPart *__restrict__ parts,
                                                                       int64_t *__restrict__ info) {
    __shared__ int64_t scan[CONCAT_BLOCK];
    __shared__ int64_t carry;
    __shared__ int bad;
    const int tid = threadIdx.x;
    const int64_t n_gaps = n_drop + 1;
    if (tid == 0) {
        carry = 0;
        bad = 0;
    }
    __syncthreads();
    for (int64_t k = tid; k < n_drop; k += CONCAT_BLOCK) {
        const int64_t d = drop[k], before = k > 0 ? (int64_t)drop[k - 1] : -1;
        if (d <= before || d >= n_rows) atomicOr(&bad, 1);
    }
    __syncthreads();
    if (bad) {                                 // (uniform: read after the barrier)
        if (tid == 0) {
            info[0] = 0;
            info[1] = 1;
        }
        return;
    }
    // gap g = the rows between dropped row g - 1 and dropped row g; CONCAT_BLOCK gaps a round, their sizes scanned in LDS
    for (int64_t g0 = 0; g0 < n_gaps; g0 += CONCAT_BLOCK) {
        const int64_t g = g0 + tid;
        int64_t first = 0, len = 0;
        if (g < n_gaps) {
            first = g > 0 ? (int64_t)drop[g - 1] + 1 : 0;
            const int64_t end = g < n_drop ? (int64_t)drop[g] : n_rows;
            len = indptr[end] - indptr[first];
        }
        const int64_t before = sizes_before(scan, &carry, tid, len);
        if (g < n_gaps) parts[g] = ConcatPart{indptr + first, indices, data, nullptr, first - g, before};
    }
    if (tid == 0) {
        parts[n_gaps] = ConcatPart{nullptr, nullptr, nullptr, nullptr, n_rows - n_drop, carry};
        info[0] = carry;
        info[1] = 0;
    }
}

// ---- sg_csr_take_rows: every taken row as a part of a concatenation.  info as above; info[1] != 0: a row outside the matrix.
__global__ void __launch_bounds__(CONCAT_BLOCK) csr_take_parts_kernel(const int64_t *__restrict__ indptr,
                                                                      const int32_t *__restrict__ indices,
                                                                      const void *__restrict__ data, int64_t n_rows,
                                                                      const int32_t *__restrict__ rows, int64_t n_take,
                                                                      ConcatPart *__restrict__ parts,
                                                                      int64_t *__restrict__ info) {
    __shared__ int64_t scan[CONCAT_BLOCK];
    __shared__ int64_t carry;
    __shared__ int bad;
    const int tid = threadIdx.x;
    if (tid == 0) {
        carry = 0;
        bad = 0;
    }
    __syncthreads();
    for (int64_t k = tid; k < n_take; k += CONCAT_BLOCK)
        if (rows[k] < 0 || (int64_t)rows[k] >= n_rows) atomicOr(&bad, 1);
    __syncthreads();
    if (bad) {                                 // (uniform: read after the barrier)
        if (tid == 0) {
            info[0] = 0;
            info[1] = 1;
        }
        return;
    }
    for (int64_t k0 = 0; k0 < n_take; k0 += CONCAT_BLOCK) {
        const int64_t k = k0 + tid;
        const int64_t row = k < n_take ? (int64_t)rows[k] : 0;
        const int64_t len = k < n_take ? indptr[row + 1] - indptr[row] : 0;
        const int64_t before = sizes_before(scan, &carry, tid, len);
        if (k < n_take) parts[k] = ConcatPart{indptr + row, indices, data, nullptr, k, before};
    }
    if (tid == 0) {
        parts[n_take] = ConcatPart{nullptr, nullptr, nullptr, nullptr, n_take, carry};
        info[0] = carry;
        info[1] = 0;
    }
}

template <typename T>
__global__ void __launch_bounds__(CONCAT_BLOCK) csr_select_kernel(const ConcatPart *__restrict__ parts, int n_parts,
                                                                  int64_t *__restrict__ out_indptr,
                                                                  int32_t *__restrict__ out_indices,
                                                                  T *__restrict__ out_data,
                                                                  const uint32_t *__restrict__ src_props,
                                                                  uint32_t *__restrict__ out_props) {
    const int64_t tid = (int64_t)blockIdx.x * CONCAT_BLOCK + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * CONCAT_BLOCK;
    copy_parts<T>(parts, n_parts, out_indptr, out_indices, out_data, tid, step);
    // the vectoriser's words of the source hold for any subset of its rows as UPPER bounds: violations (0 stays 0), the
    // largest squared norm and the longest row may have belonged to a dropped row
    if (out_props != nullptr && tid == 0) {
        out_props[0] = src_props[0];
        out_props[1] = src_props[1];
        out_props[2] = src_props[2];
        out_props[3] = 0;
    }
}

// The kept rows' norms: output row r lies in gap p, whose descriptor holds the source's row pointers from the gap's first row on
// -- so the row's place in the source is that pointer's distance from the source's, plus r's place in the gap.
__global__ void __launch_bounds__(CONCAT_BLOCK) gather_row_norms_kernel(const ConcatPart *__restrict__ parts, int n_parts,
                                                                        const int64_t *__restrict__ src_indptr,
                                                                        const double *__restrict__ src_norm,
                                                                        double *__restrict__ out_norm) {
    const int64_t n_rows = parts[n_parts].row_off;
    const int64_t step = (int64_t)gridDim.x * CONCAT_BLOCK;
    for (int64_t r = (int64_t)blockIdx.x * CONCAT_BLOCK + threadIdx.x; r < n_rows; r += step) {
        const int p = part_of<true>(parts, n_parts, r);
        out_norm[r] = src_norm[(parts[p].indptr - src_indptr) + (r - parts[p].row_off)];
    }
}

// ---- host drivers. Each entry point reads as its stages: describe the parts (describe_parts; the concatenation writes its
// descriptors on the host), allocate the result and what it inherits (csr_alloc + csr_inherit, sg_csr.hip; rows_result for
// select and take), copy (copy_rows / the concat kernel), the norms beside the kernels.

// the copy kernels' grid: a thread a unit of four entries or a row, whichever are more; at most 32 workgroups a CU
unsigned copy_grid(const sg_ctx *ctx, int64_t n_rows, int64_t nnz) {
    const int64_t work = std::max<int64_t>(std::max<int64_t>((nnz + CONCAT_UNIT - 1) / CONCAT_UNIT, n_rows), 1);
    const int64_t want = (work + CONCAT_BLOCK - 1) / CONCAT_BLOCK;
    return (unsigned)std::min<int64_t>(want, (int64_t)ctx->num_cu * 32);
}

}   // namespace

extern "C" int sg_csr_concat(sg_ctx *ctx, const sg_csr *const *parts, int32_t n_parts, sg_csr **out) {
    SG_REQUIRE(ctx && parts && out && n_parts >= 1, "null argument or no parts");
    int64_t n_rows = 0, nnz = 0;
    for (int p = 0; p < n_parts; ++p) {
        SG_REQUIRE(parts[p] != nullptr, "a part is null");
        SG_REQUIRE(parts[p]->n_cols == parts[0]->n_cols && parts[p]->dtype == parts[0]->dtype,
                   "parts disagree in columns or dtype");
        // the representatives' matrix of a group structure may not have its rows yet
        if (parts[p]->rows_of) SG_TRY(sg_csr_ensure_rows(ctx, parts[p]));
        n_rows += parts[p]->n_rows;
        nnz += parts[p]->nnz;
    }
    if (n_rows > INT32_MAX) {
        sg_set_error("sg_csr_concat: %lld rows exceed int32 indices", (long long)n_rows);
        return SG_ERR_OVERFLOW;
    }
    CsrPtr m;
    SG_TRY(csr_alloc(ctx, n_rows, parts[0]->n_cols, nnz, parts[0]->dtype, CSR_SLACK_COPY, &m));
    const CsrCarries carries = csr_inherit(m.get(), parts, n_parts, CsrDerived::stacked);
    if (carries.words) SG_TRY(sg_alloc(ctx, (size_t)4, &m->d_props_words));
    if (carries.norms) SG_TRY(sg_alloc(ctx, (size_t)n_rows + 1, &m->d_row_norm));

    std::vector<ConcatPart> desc((size_t)n_parts + 1);
    int64_t row_off = 0, nnz_off = 0;
    for (int p = 0; p < n_parts; ++p) {
        desc[p] = ConcatPart{parts[p]->d_indptr, parts[p]->d_indices, parts[p]->d_data, parts[p]->d_props_words, row_off,
                             nnz_off};
        row_off += parts[p]->n_rows;
        nnz_off += parts[p]->nnz;
    }
    desc[n_parts] = ConcatPart{nullptr, nullptr, nullptr, nullptr, row_off, nnz_off};
    Scratch scratch(ctx);
    ConcatPart *d_desc = nullptr;
    SG_TRY(scratch.alloc(desc.size(), &d_desc));
    SG_HIP_TRY(hipMemcpyAsync(d_desc, desc.data(), desc.size() * sizeof(ConcatPart), hipMemcpyHostToDevice, ctx->stream));
    SG_HIP_TRY(hipStreamSynchronize(ctx->stream));      // desc is a local
    const unsigned grid = copy_grid(ctx, n_rows, nnz);
    by_dtype(m->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(csr_concat_kernel<T>, dim3(grid), dim3(CONCAT_BLOCK), 0, ctx->stream, (const ConcatPart *)d_desc,
                           (int)n_parts, (int64_t *)m->d_indptr, (int32_t *)m->d_indices, (T *)m->d_data, m->d_props_words);
        return SG_OK;
    });
    scratch.release(d_desc);       // (stream-ordered pool: a later taker of the block runs behind the kernel)
    SG_HIP_TRY(hipGetLastError());
    if (carries.norms) {           // the rows' norms, part by part (a view's pointer starts at its first row)
        int64_t at = 0;
        for (int p = 0; p < n_parts; ++p) {
            if (parts[p]->n_rows > 0)
                SG_HIP_TRY(hipMemcpyAsync(m->d_row_norm + at, parts[p]->d_row_norm, sizeof(double) * (size_t)parts[p]->n_rows,
                                          hipMemcpyDeviceToDevice, ctx->stream));
            at += parts[p]->n_rows;
        }
    }
    *out = m.release();
    return SG_OK;
}

namespace {

// A part-descriptor kernel (one workgroup) over a list of m's rows: n_parts descriptors and the sentinel into *d_desc, the
// two totals into *d_info (both the scope's).  The totals are the one thing that comes back: they size the result (*nnz),
// or refuse the list.
using PartsKernel = void (*)(const int64_t *, const int32_t *, const void *, int64_t, const int32_t *, int64_t, ConcatPart *,
                             int64_t *);
int describe_parts(sg_ctx *ctx, Scratch &scratch, PartsKernel kernel, const sg_csr *m, const int32_t *d_list, int64_t n_list,
                   int64_t n_parts, ConcatPart **d_desc, int64_t **d_info, int64_t *nnz, const char *refusal) {
    SG_TRY(scratch.alloc((size_t)n_parts + 1, d_desc));
    SG_TRY(scratch.alloc((size_t)2, d_info));
    hipLaunchKernelGGL(kernel, dim3(1), dim3(CONCAT_BLOCK), 0, ctx->stream, m->d_indptr, m->d_indices, m->d_data, m->n_rows,
                       d_list, n_list, *d_desc, *d_info);
    SG_HIP_TRY(hipGetLastError());
    int64_t info[2] = {0, 0};
    SG_TRY(sg_fetch(ctx, ctx->h_fetch, *d_info, sizeof(info)));
    memcpy(info, ctx->h_fetch, sizeof(info));
    SG_REQUIRE(info[1] == 0, refusal);
    *nnz = info[0];
    return SG_OK;
}

// n_rows of m's rows, nnz entries: the arrays, what such a result inherits, and the block of the words when it carries them
int rows_result(sg_ctx *ctx, const sg_csr *m, int64_t n_rows, int64_t nnz, CsrDerived kind, CsrPtr *r, CsrCarries *carries) {
    SG_TRY(csr_alloc(ctx, n_rows, m->n_cols, nnz, m->dtype, CSR_SLACK_COPY, r));
    *carries = csr_inherit(r->get(), m, kind);
    if (carries->words) SG_TRY(sg_alloc(ctx, (size_t)4, &(*r)->d_props_words));
    return SG_OK;
}

// (a) and (b) of the header over the descriptors of m's rows; the words are the source's own
int copy_rows(sg_ctx *ctx, const sg_csr *m, const ConcatPart *d_desc, int64_t n_parts, sg_csr *r) {
    const unsigned grid = copy_grid(ctx, r->n_rows, r->nnz);
    return by_dtype(m->dtype, [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL(csr_select_kernel<T>, dim3(grid), dim3(CONCAT_BLOCK), 0, ctx->stream, d_desc, (int)n_parts,
                           (int64_t *)r->d_indptr, (int32_t *)r->d_indices, (T *)r->d_data, (const uint32_t *)m->d_props_words,
                           r->d_props_words);
        SG_HIP_TRY(hipGetLastError());
        return SG_OK;
    });
}

}   // namespace

extern "C" int sg_csr_select_rows(sg_ctx *ctx, const sg_csr *m, const int32_t *d_drop_sorted, int64_t n_drop, sg_csr **out) {
    SG_REQUIRE(ctx && m && out, "null argument");
    SG_REQUIRE(n_drop >= 0 && n_drop <= m->n_rows, "more rows to drop than the matrix has");
    SG_REQUIRE(n_drop == 0 || d_drop_sorted != nullptr, "the drop list is null");
    if (m->rows_of) SG_TRY(sg_csr_ensure_rows(ctx, m));
    const int64_t n_gaps = n_drop + 1;
    CsrPtr r;
    CsrCarries carries;
    Scratch scratch(ctx);
    ConcatPart *d_desc = nullptr;
    int64_t *d_info = nullptr;
    int64_t nnz = 0;
    SG_TRY(describe_parts(ctx, scratch, csr_select_gaps_kernel, m, d_drop_sorted, n_drop, n_gaps, &d_desc, &d_info, &nnz,
                          "the rows to drop must be ascending, distinct and inside the matrix"));
    SG_TRY(rows_result(ctx, m, m->n_rows - n_drop, nnz, CsrDerived::selected, &r, &carries));
    SG_TRY(copy_rows(ctx, m, d_desc, n_gaps, r.get()));
    if (carries.norms) {           // the kept rows' norms, gathered past the dropped rows
        SG_TRY(sg_alloc(ctx, (size_t)r->n_rows + 1, &r->d_row_norm));
        if (r->n_rows > 0) {
            hipLaunchKernelGGL(gather_row_norms_kernel, dim3(copy_grid(ctx, r->n_rows, 0)), dim3(CONCAT_BLOCK), 0, ctx->stream,
                               (const ConcatPart *)d_desc, (int)n_gaps, m->d_indptr, (const double *)m->d_row_norm, r->d_row_norm);
            SG_HIP_TRY(hipGetLastError());
        }
    }
    scratch.release(d_info);       // (the totals' block goes back first, then the descriptors': the pool's order of old)
    *out = r.release();
    return SG_OK;
}

extern "C" int sg_csr_take_rows(sg_ctx *ctx, const sg_csr *m, const int32_t *d_rows, int64_t n_rows, sg_csr **out) {
    SG_REQUIRE(ctx && m && out, "null argument");
    SG_REQUIRE(n_rows >= 0 && n_rows < INT32_MAX, "the number of rows to take is negative or exceeds int32");
    SG_REQUIRE(n_rows == 0 || d_rows != nullptr, "the list of rows is null");
    if (m->rows_of) SG_TRY(sg_csr_ensure_rows(ctx, m));
    CsrPtr r;
    CsrCarries carries;
    Scratch scratch(ctx);          // (here the descriptors' block goes back first, then the totals': the order they were taken in)
    ConcatPart *d_desc = nullptr;
    int64_t *d_info = nullptr;
    int64_t nnz = 0;
    SG_TRY(describe_parts(ctx, scratch, csr_take_parts_kernel, m, d_rows, n_rows, n_rows, &d_desc, &d_info, &nnz,
                          "a row to take lies outside the matrix"));
    SG_TRY(rows_result(ctx, m, n_rows, nnz, CsrDerived::taken, &r, &carries));
    SG_TRY(copy_rows(ctx, m, d_desc, n_rows, r.get()));
    *out = r.release();
    return SG_OK;
}
