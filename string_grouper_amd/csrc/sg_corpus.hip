// sg_corpus.hip -- the reverse path of a resident corpus: the top-n of every CORPUS row, taken from a
// product that was computed the other way round.
//
// The reference keeps max_n_matches per master row: sp_matmul_topn(M, D.T, top_n, thr) (string_grouper.py:725-732; with
// top_n = 1 for match_most_similar, :120).  A corpus that keeps its inverted index on the device gets the cheap product with
// the NEW rows on the left: D . M^T, every new row against the corpus index.  That product, taken with a per-row cap high
// enough that no row came back full, is a complete list of the pairs above the threshold; sg_topn_transpose_select turns it
// into the reference's result: per corpus row m, the top_n pairs (d, score) by score descending, then d ascending -- the
// library's tie rule.  score(d, m) is the same number from either side: both sum the separately rounded products of the
// shared terms in ascending term order.
//
// Kernels (one pass each over the pairs, then one over the corpus rows):
//   tsel_count_kernel    candidates per corpus row (a wave per input row, atomics on the row's counter)
//   (prefix sum)         bucket offsets, sg_exclusive_scan_u32
//   tsel_scatter_kernel  (d, score) into the buckets, in arrival order (the selection below does not depend on it)
//   tsel_wave_kernel     a wave per corpus row of at most TSEL_WAVE_MAX candidates: the rank of every candidate among the
//                        row's, by a 64 x 64 compare through lane shuffles; rank < top_n is written at its slot
//   tsel_block_kernel    a workgroup per larger row (a hub: a batch with thousands of copies of one corpus name): radix
//                        select of the top_n-th best (score, d) in LDS histograms, then the rank of the selected few
//
// And the filter of a corpus that has forgotten rows ("A corpus that forgets"): a removed row stays in its
// segment and its index until the next compaction, so a multiply still names it.  The multiply is asked for top_n + dead
// entries; sg_topn_drop_columns takes the dead columns out of every result row, renumbers the others (column - dead columns
// below it) and cuts at top_n.  A row is ordered by (score descending, column ascending), dropping entries keeps the order
// of the rest and the renumbering is monotonic, so what is left IS the top_n over the live rows (scipy: C[:, keep] of the
// uncut product, then the cut).
//   drop_columns_kernel  a wave per result row, 64 entries a round: a binary search per lane in the sorted dead list (in
//                        LDS up to DROP_LDS_MAX columns), the survivors' positions by ballot + popcount on a running base
#include "sg_internal.h"

#include <algorithm>
#include <memory>

namespace {

constexpr int TSEL_BLOCK = 256;
constexpr int TSEL_WAVES = TSEL_BLOCK / SG_WAVE;
constexpr uint32_t TSEL_WAVE_MAX = 1024;      // candidates a wave ranks by itself; more: the workgroup kernel
constexpr int TSEL_MAX_TOPN = 2048;           // LDS of the workgroup kernel's selected set (16 bytes an entry)
constexpr int TSEL_BIG_GRID = 512;

// A score as an unsigned key with the order of the value (finite values of either sign), zero-extended to 64 bits so that
// both value types share one comparison
__device__ inline uint64_t score_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (uint64_t)((b & 0x80000000u) ? ~b : (b | 0x80000000u));
}
__device__ inline uint64_t score_key(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// (ka, da) comes before (kb, db): higher score first, then the lower column
__device__ inline bool before(uint64_t ka, int32_t da, uint64_t kb, int32_t db) {
    return ka > kb || (ka == kb && da < db);
}

__device__ inline uint64_t shfl_u64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, SG_WAVE);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, SG_WAVE);
    return ((uint64_t)hi << 32) | lo;
}

// ---- pass over the pairs: one wave per input row, its first counts[r] slots
__global__ void __launch_bounds__(TSEL_BLOCK) tsel_count_kernel(const int32_t *__restrict__ cols,
                                                                const int32_t *__restrict__ counts, int64_t n_in,
                                                                int32_t stride, int64_t n_out, uint32_t *__restrict__ cnt,
                                                                uint32_t *__restrict__ flags) {
    const int lane = threadIdx.x & (SG_WAVE - 1);
    const int64_t step = (int64_t)gridDim.x * TSEL_WAVES;
    for (int64_t r = (int64_t)blockIdx.x * TSEL_WAVES + threadIdx.x / SG_WAVE; r < n_in; r += step) {
        const int32_t c = min(max(counts[r], 0), stride);
        for (int32_t j = lane; j < c; j += SG_WAVE) {
            const int32_t m = cols[r * stride + j];
            if (m >= 0 && (int64_t)m < n_out)
                atomicAdd(&cnt[m], 1u);
            else
                atomicOr(&flags[0], 1u);             // a column outside the corpus: the call fails (bad argument)
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(TSEL_BLOCK) tsel_scatter_kernel(const int32_t *__restrict__ cols,
                                                                  const T *__restrict__ vals,
                                                                  const int32_t *__restrict__ counts, int64_t n_in,
                                                                  int32_t stride, int64_t n_out,
                                                                  const uint32_t *__restrict__ off,
                                                                  uint32_t *__restrict__ cnt, int32_t *__restrict__ b_rows,
                                                                  T *__restrict__ b_vals) {
    const int lane = threadIdx.x & (SG_WAVE - 1);
    const int64_t step = (int64_t)gridDim.x * TSEL_WAVES;
    for (int64_t r = (int64_t)blockIdx.x * TSEL_WAVES + threadIdx.x / SG_WAVE; r < n_in; r += step) {
        const int32_t c = min(max(counts[r], 0), stride);
        for (int32_t j = lane; j < c; j += SG_WAVE) {
            const int32_t m = cols[r * stride + j];
            if (m < 0 || (int64_t)m >= n_out) continue;
            // the counter counts down to zero: slot in [off[m], off[m + 1])
            const uint32_t pos = off[m] + (atomicSub(&cnt[m], 1u) - 1u);
            b_rows[pos] = (int32_t)r;
            b_vals[pos] = vals[r * stride + j];
        }
    }
}

// ---- a wave per corpus row.  Rows of more than TSEL_WAVE_MAX candidates are queued for the workgroup kernel.
template <typename T>
__global__ void __launch_bounds__(TSEL_BLOCK) tsel_wave_kernel(const uint32_t *__restrict__ off,
                                                               const int32_t *__restrict__ b_rows,
                                                               const T *__restrict__ b_vals, int64_t n_out, int32_t top_n,
                                                               int32_t stride_out, int32_t *__restrict__ out_cols,
                                                               T *__restrict__ out_vals, int32_t *__restrict__ out_counts,
                                                               uint32_t *__restrict__ big_rows,
                                                               uint32_t *__restrict__ flags) {
    const int lane = threadIdx.x & (SG_WAVE - 1);
    const int64_t step = (int64_t)gridDim.x * TSEL_WAVES;
    for (int64_t m = (int64_t)blockIdx.x * TSEL_WAVES + threadIdx.x / SG_WAVE; m < n_out; m += step) {
        const uint32_t lo = off[m], hi = off[m + 1];
        const uint32_t c = hi - lo;
        if (c > TSEL_WAVE_MAX) {
            if (lane == 0) big_rows[atomicAdd(&flags[1], 1u)] = (uint32_t)m;
            continue;
        }
        const int32_t keep = min(min((int32_t)c, top_n), stride_out);
        if (lane == 0) out_counts[m] = keep;
        int32_t *row_cols = out_cols + m * (int64_t)stride_out;
        T *row_vals = out_vals + m * (int64_t)stride_out;
        for (uint32_t pb = lo; pb < hi; pb += SG_WAVE) {         // (wave-uniform bounds: every lane reaches the shuffles)
            const uint32_t p = pb + lane;
            const bool mine = p < hi;
            const T v = mine ? b_vals[p] : T(0);
            const uint64_t kp = score_key(v);
            const int32_t dp = mine ? b_rows[p] : 0;
            uint32_t rank = 0;
            for (uint32_t qb = lo; qb < hi; qb += SG_WAVE) {
                const uint32_t q = qb + lane;
                const uint64_t kq_own = q < hi ? score_key(b_vals[q]) : 0;
                const int32_t dq_own = q < hi ? b_rows[q] : 0;
                const uint32_t n_q = min(hi - qb, (uint32_t)SG_WAVE);
                for (uint32_t j = 0; j < n_q; ++j) {
                    const uint64_t kq = shfl_u64(kq_own, (int)j);
                    const int32_t dq = __shfl(dq_own, (int)j, SG_WAVE);
                    rank += before(kq, dq, kp, dp) ? 1u : 0u;
                }
            }
            if (mine && rank < (uint32_t)keep) {
                row_cols[rank] = dp;
                row_vals[rank] = v;
            }
        }
    }
}

// ---- a workgroup per queued row: the keep-th best (score, column) by radix select over the 96-bit key
// (score key, ~column), 8 bits a pass from the top; then the selected entries ranked among themselves.
template <typename T>
__global__ void __launch_bounds__(TSEL_BLOCK) tsel_block_kernel(const uint32_t *__restrict__ off,
                                                                const int32_t *__restrict__ b_rows,
                                                                const T *__restrict__ b_vals, int32_t top_n,
                                                                int32_t stride_out, int32_t *__restrict__ out_cols,
                                                                T *__restrict__ out_vals, int32_t *__restrict__ out_counts,
                                                                const uint32_t *__restrict__ big_rows,
                                                                uint32_t *__restrict__ flags) {
    __shared__ uint32_t hist[256];
    __shared__ uint64_t sel_key[TSEL_MAX_TOPN];
    __shared__ int32_t sel_d[TSEL_MAX_TOPN];
    __shared__ uint32_t sel_p[TSEL_MAX_TOPN];
    __shared__ uint64_t pre_key, mask_key;
    __shared__ uint32_t pre_nd, mask_nd, remaining, n_sel;
    const int tid = threadIdx.x;
    const uint32_t n_big = flags[1];
    // (the first 4 bytes of a float32 score's key are zero: its passes start at byte 4)
    const int first_byte = sizeof(T) == 4 ? 4 : 0;
    for (uint32_t b = blockIdx.x; b < n_big; b += gridDim.x) {
        const uint32_t m = big_rows[b];
        const uint32_t lo = off[m], hi = off[m + 1];
        const uint32_t c = hi - lo;
        const int32_t keep = min(min((int32_t)min(c, (uint32_t)INT32_MAX), top_n), stride_out);
        if (tid == 0) {
            pre_key = 0;
            mask_key = 0;
            pre_nd = 0;
            mask_nd = 0;
            remaining = (uint32_t)keep;
            n_sel = 0;
        }
        __syncthreads();
        if ((uint32_t)keep < c) {
            for (int byte = first_byte; byte < 12; ++byte) {
                for (int i = tid; i < 256; i += TSEL_BLOCK) hist[i] = 0;
                __syncthreads();
                const uint64_t pk = pre_key, mk = mask_key;
                const uint32_t pn = pre_nd, mn = mask_nd;
                for (uint32_t p = lo + tid; p < hi; p += TSEL_BLOCK) {
                    const uint64_t k = score_key(b_vals[p]);
                    const uint32_t nd = ~(uint32_t)b_rows[p];
                    if ((k & mk) != pk || (nd & mn) != pn) continue;
                    const uint32_t digit = byte < 8 ? (uint32_t)(k >> (56 - 8 * byte)) & 255u
                                                    : (nd >> (24 - 8 * (byte - 8))) & 255u;
                    atomicAdd(&hist[digit], 1u);
                }
                __syncthreads();
                if (tid == 0) {
                    uint32_t rem = remaining;
                    int digit = 255;
                    for (; digit > 0; --digit) {
                        if (hist[digit] >= rem) break;
                        rem -= hist[digit];
                    }
                    remaining = rem;
                    if (byte < 8) {
                        pre_key |= (uint64_t)digit << (56 - 8 * byte);
                        mask_key |= (uint64_t)255u << (56 - 8 * byte);
                    } else {
                        pre_nd |= (uint32_t)digit << (24 - 8 * (byte - 8));
                        mask_nd |= 255u << (24 - 8 * (byte - 8));
                    }
                }
                __syncthreads();
            }
        }
        // selected: every entry at or above the pivot (all of them when the row has at most keep)
        const bool all = (uint32_t)keep >= c;
        const uint64_t pk = pre_key;
        const uint32_t pn = pre_nd;
        for (uint32_t p = lo + tid; p < hi; p += TSEL_BLOCK) {
            const uint64_t k = score_key(b_vals[p]);
            const uint32_t nd = ~(uint32_t)b_rows[p];
            if (all || k > pk || (k == pk && nd >= pn)) {
                const uint32_t slot = atomicAdd(&n_sel, 1u);
                if (slot < (uint32_t)TSEL_MAX_TOPN) {
                    sel_key[slot] = k;
                    sel_d[slot] = b_rows[p];
                    sel_p[slot] = p;
                }
            }
        }
        __syncthreads();
        const uint32_t ns = n_sel;
        if (ns != (uint32_t)keep) {
            if (tid == 0) atomicOr(&flags[0], 2u);          // (cannot happen with distinct columns in a row)
        } else {
            for (uint32_t i = tid; i < ns; i += TSEL_BLOCK) {
                uint32_t rank = 0;
                const uint64_t ki = sel_key[i];
                const int32_t di = sel_d[i];
                for (uint32_t j = 0; j < ns; ++j) rank += before(sel_key[j], sel_d[j], ki, di) ? 1u : 0u;
                if (rank < (uint32_t)keep) {
                    out_cols[(int64_t)m * stride_out + rank] = di;
                    out_vals[(int64_t)m * stride_out + rank] = b_vals[sel_p[i]];
                }
            }
            if (tid == 0) out_counts[m] = keep;
        }
        __syncthreads();
    }
}

// ---- sg_topn_drop_columns
constexpr int DROP_LDS_MAX = 2048;            // dead columns kept in LDS (8 KiB); a longer list is searched where it lies

template <typename T, bool IN_LDS>
__global__ void __launch_bounds__(TSEL_BLOCK) drop_columns_kernel(const int32_t *__restrict__ cols,
                                                                  const T *__restrict__ vals,
                                                                  const int32_t *__restrict__ counts, int64_t n_rows,
                                                                  int32_t stride_in, const int32_t *__restrict__ dead,
                                                                  int32_t n_dead, int32_t stride_out,
                                                                  int32_t *__restrict__ out_cols, T *__restrict__ out_vals,
                                                                  int32_t *__restrict__ out_counts) {
    __shared__ int32_t lds_dead[IN_LDS ? DROP_LDS_MAX : 1];
    if (IN_LDS) {
        for (int i = threadIdx.x; i < n_dead; i += TSEL_BLOCK) lds_dead[i] = dead[i];
        __syncthreads();
    }
    const int lane = threadIdx.x & (SG_WAVE - 1);
    const uint64_t below = (1ull << lane) - 1ull;                // the lanes before this one
    const int64_t step = (int64_t)gridDim.x * TSEL_WAVES;
    for (int64_t r = (int64_t)blockIdx.x * TSEL_WAVES + threadIdx.x / SG_WAVE; r < n_rows; r += step) {
        const int32_t c = min(max(counts[r], 0), stride_in);
        const int32_t *row_cols = cols + r * (int64_t)stride_in;
        const T *row_vals = vals + r * (int64_t)stride_in;
        int32_t base = 0;                                        // survivors so far (wave-uniform, as are the loop's bounds)
        for (int32_t j0 = 0; j0 < c && base < stride_out; j0 += SG_WAVE) {
            const int32_t j = j0 + lane;
            const bool mine = j < c;
            const int32_t col = mine ? row_cols[j] : 0;
            const T v = mine ? row_vals[j] : T(0);
            int32_t lo = 0, hi = n_dead;                         // lo: dead columns below col
            while (lo < hi) {
                const int32_t mid = (lo + hi) >> 1;
                const int32_t d = IN_LDS ? lds_dead[mid] : dead[mid];
                if (d < col) lo = mid + 1;
                else hi = mid;
            }
            const bool gone = lo < n_dead && (IN_LDS ? lds_dead[lo] : dead[lo]) == col;
            const bool keep = mine && !gone;
            const uint64_t kept = __ballot(keep);
            const int32_t pos = base + (int32_t)__popcll(kept & below);
            if (keep && pos < stride_out) {
                out_cols[r * (int64_t)stride_out + pos] = col - lo;
                out_vals[r * (int64_t)stride_out + pos] = v;
            }
            base += (int32_t)__popcll(kept);
        }
        if (lane == 0) out_counts[r] = min(base, stride_out);
    }
}

template <typename T>
int drop_columns(sg_ctx *ctx, const sg_topn *in, const int32_t *d_dead, int32_t n_dead, sg_topn *r) {
    const int64_t waves = in->n_rows > 0 ? in->n_rows : 1;
    const int grid = (int)std::min<int64_t>((waves + TSEL_WAVES - 1) / TSEL_WAVES, (int64_t)ctx->num_cu * 16);
    if (n_dead <= DROP_LDS_MAX)
        hipLaunchKernelGGL((drop_columns_kernel<T, true>), dim3(grid), dim3(TSEL_BLOCK), 0, ctx->stream,
                           (const int32_t *)in->d_cols, (const T *)in->d_vals, (const int32_t *)in->d_counts, in->n_rows,
                           in->stride, d_dead, n_dead, r->stride, r->d_cols, (T *)r->d_vals, r->d_counts);
    else
        hipLaunchKernelGGL((drop_columns_kernel<T, false>), dim3(grid), dim3(TSEL_BLOCK), 0, ctx->stream,
                           (const int32_t *)in->d_cols, (const T *)in->d_vals, (const int32_t *)in->d_counts, in->n_rows,
                           in->stride, d_dead, n_dead, r->stride, r->d_cols, (T *)r->d_vals, r->d_counts);
    SG_HIP_TRY(hipGetLastError());
    return SG_OK;
}

template <typename T>
int transpose_select(sg_ctx *ctx, const sg_topn *pairs, int64_t n_out, int32_t top_n, sg_topn *r, uint32_t *cnt,
                     uint32_t *off, uint32_t *flags, uint32_t *big_rows, int32_t *b_rows, T *b_vals) {
    const int64_t n_in = pairs->n_rows;
    const int64_t in_waves = n_in > 0 ? n_in : 1;
    const int g_in = (int)std::min<int64_t>((in_waves + TSEL_WAVES - 1) / TSEL_WAVES, (int64_t)ctx->num_cu * 16);
    const int g_out = (int)std::min<int64_t>(((n_out > 0 ? n_out : 1) + TSEL_WAVES - 1) / TSEL_WAVES, (int64_t)ctx->num_cu * 16);
    hipLaunchKernelGGL(tsel_count_kernel, dim3(g_in), dim3(TSEL_BLOCK), 0, ctx->stream, (const int32_t *)pairs->d_cols,
                       (const int32_t *)pairs->d_counts, n_in, pairs->stride, n_out, cnt, flags);
    SG_HIP_TRY(hipGetLastError());
    // n_out + 1 counters, the last one zero: off[n_out] = number of pairs
    SG_TRY(sg_exclusive_scan_u32(ctx, cnt, off, n_out + 1, nullptr));
    hipLaunchKernelGGL(tsel_scatter_kernel<T>, dim3(g_in), dim3(TSEL_BLOCK), 0, ctx->stream, (const int32_t *)pairs->d_cols,
                       (const T *)pairs->d_vals, (const int32_t *)pairs->d_counts, n_in, pairs->stride, n_out,
                       (const uint32_t *)off, cnt, b_rows, b_vals);
    hipLaunchKernelGGL(tsel_wave_kernel<T>, dim3(g_out), dim3(TSEL_BLOCK), 0, ctx->stream, (const uint32_t *)off,
                       (const int32_t *)b_rows, (const T *)b_vals, n_out, top_n, r->stride, r->d_cols, (T *)r->d_vals,
                       r->d_counts, big_rows, flags);
    hipLaunchKernelGGL(tsel_block_kernel<T>, dim3(TSEL_BIG_GRID), dim3(TSEL_BLOCK), 0, ctx->stream, (const uint32_t *)off,
                       (const int32_t *)b_rows, (const T *)b_vals, top_n, r->stride, r->d_cols, (T *)r->d_vals, r->d_counts,
                       (const uint32_t *)big_rows, flags);
    SG_HIP_TRY(hipGetLastError());
    uint32_t h_flags[2] = {0, 0};
    SG_HIP_TRY(hipMemcpyAsync(ctx->h_fetch, flags, sizeof(h_flags), hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(h_flags, ctx->h_fetch, sizeof(h_flags));
    if (h_flags[0] & 1u) {
        sg_set_error("bad argument: a pair names a row outside [0, n_rows_out)");
        return SG_ERR_BADARG;
    }
    if (h_flags[0] & 2u) {
        sg_set_error("bad argument: a row of the pair list names one column twice");
        return SG_ERR_BADARG;
    }
    return SG_OK;
}

}  // namespace

extern "C" int sg_topn_transpose_select(sg_ctx *ctx, const sg_topn *pairs, int64_t n_rows_out, int32_t top_n,
                                        sg_topn **out) {
    SG_REQUIRE(ctx && pairs && out && n_rows_out >= 0, "bad argument");
    SG_REQUIRE(top_n >= 1 && top_n <= TSEL_MAX_TOPN, "top_n must be in [1, 2048]");
    SG_REQUIRE(pairs->n_cols <= n_rows_out, "the pair list has more columns than the result has rows");
    SG_REQUIRE((double)pairs->n_rows * (double)pairs->stride < 4.0e9, "more than 2^32 pair slots");
    SG_REQUIRE(n_rows_out < (int64_t)UINT32_MAX, "too many result rows");
    const int64_t n_cols = pairs->n_rows;          // the result's columns are the pair list's rows
    const int32_t stride = (int32_t)(top_n < n_cols ? top_n : (n_cols > 0 ? n_cols : 1));
    if ((double)n_rows_out * (double)stride > 2.0e9) {
        sg_set_error("result of %lld rows x top_n %d does not fit the 32-bit result index", (long long)n_rows_out, stride);
        return SG_ERR_OVERFLOW;
    }
    sg_topn *r = new (std::nothrow) sg_topn();
    if (!r) return SG_ERR_OOM;
    std::unique_ptr<sg_topn, int (*)(sg_topn *)> guard(r, sg_topn_free);
    r->ctx = ctx;
    r->n_rows = n_rows_out;
    r->n_cols = n_cols;
    r->stride = stride;
    r->dtype = pairs->dtype;
    const size_t cells = (size_t)n_rows_out * (size_t)stride + 64;
    const size_t vsize = pairs->dtype == SG_F64 ? 8 : 4;
    SG_TRY(sg_alloc(ctx, cells, &r->d_cols));
    SG_TRY(ctx->alloc(cells * vsize, &r->d_vals));
    SG_TRY(sg_alloc(ctx, (size_t)n_rows_out + 64, &r->d_counts));
    // scratch: counters (n_out + 1), offsets (n_out + 1), flags {error bits, queued rows}, the queue, the buckets (at most
    // one entry per slot of the pair list)
    const size_t slots = (size_t)pairs->n_rows * (size_t)pairs->stride + 1;
    uint32_t *cnt = nullptr, *off = nullptr, *flags = nullptr, *big_rows = nullptr;
    int32_t *b_rows = nullptr;
    void *b_vals = nullptr;
    int st = sg_alloc(ctx, (size_t)n_rows_out + 1, &cnt);
    if (st == SG_OK) st = sg_alloc(ctx, (size_t)n_rows_out + 1, &off);
    if (st == SG_OK) st = sg_alloc(ctx, (size_t)64, &flags);
    if (st == SG_OK) st = sg_alloc(ctx, (size_t)n_rows_out + 1, &big_rows);
    if (st == SG_OK) st = sg_alloc(ctx, slots, &b_rows);
    if (st == SG_OK) st = ctx->alloc(slots * vsize, &b_vals);
    if (st == SG_OK) st = SG_ZERO2(ctx, cnt, ((size_t)n_rows_out + 1) * 4, flags, 64 * 4);
    if (st == SG_OK) {
        st = pairs->dtype == SG_F64
                 ? transpose_select<double>(ctx, pairs, n_rows_out, top_n, r, cnt, off, flags, big_rows, b_rows, (double *)b_vals)
                 : transpose_select<float>(ctx, pairs, n_rows_out, top_n, r, cnt, off, flags, big_rows, b_rows, (float *)b_vals);
    }
    ctx->release(cnt);
    ctx->release(off);
    ctx->release(flags);
    ctx->release(big_rows);
    ctx->release(b_rows);
    ctx->release(b_vals);
    if (st != SG_OK) return st;
    *out = guard.release();
    return SG_OK;
}

extern "C" int sg_topn_drop_columns(sg_ctx *ctx, const sg_topn *r_in, const int32_t *d_dead_sorted, int32_t n_dead,
                                    int32_t top_n, sg_topn **out) {
    SG_REQUIRE(ctx && r_in && out, "null argument");
    SG_REQUIRE(top_n >= 1, "top_n must be at least 1");
    SG_REQUIRE(n_dead >= 0 && (int64_t)n_dead <= r_in->n_cols, "more dead columns than the result has columns");
    SG_REQUIRE(n_dead == 0 || d_dead_sorted != nullptr, "the list of dead columns is null");
    sg_topn *r = new (std::nothrow) sg_topn();
    if (!r) return SG_ERR_OOM;
    std::unique_ptr<sg_topn, int (*)(sg_topn *)> guard(r, sg_topn_free);
    r->ctx = ctx;
    r->n_rows = r_in->n_rows;
    r->n_cols = r_in->n_cols - n_dead;
    r->stride = std::max<int32_t>(std::min<int32_t>(top_n, r_in->stride), 1);
    r->dtype = r_in->dtype;
    const size_t cells = (size_t)r->n_rows * (size_t)r->stride + 64;
    SG_TRY(sg_alloc(ctx, cells, &r->d_cols));
    SG_TRY(ctx->alloc(cells * (r->dtype == SG_F64 ? 8 : 4), &r->d_vals));
    SG_TRY(sg_alloc(ctx, (size_t)r->n_rows + 64, &r->d_counts));
    SG_TRY(r->dtype == SG_F64 ? drop_columns<double>(ctx, r_in, d_dead_sorted, n_dead, r)
                              : drop_columns<float>(ctx, r_in, d_dead_sorted, n_dead, r));
    *out = guard.release();
    return SG_OK;
}
