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
//
// And the editing of a KEPT self-join ("A self-join that is kept"): the corpus's own top-n result stays on
// the device and follows every append and remove, so whole rows of fixed-stride results are stacked (scipy's vstack of result
// blocks, string_grouper.py:750), taken out together with their columns (C[keep][:, keep]) and written back one by one.
//   topn_copy_rows_kernel  a wave per row: the row's first counts[r] entries to row row_off + r (sg_topn_concat_rows) or to
//                          row rows[r] (sg_topn_put_rows) of a result of another stride; 16 bytes a lane where both strides
//                          are multiples of four entries, an entry a lane otherwise
//   forget_kernel          a wave per SURVIVING row: where it lay (a binary search in dead[i] - i), then drop_columns_kernel's
//                          filter of its entries; a row that was full and is not any more is flagged
//   (prefix sum)           positions of the flagged rows, sg_exclusive_scan_positive_i32
//   short_rows_kernel      their numbers, ascending
#include "sg_internal.h"

#include <algorithm>

namespace {

constexpr int TSEL_BLOCK = 256;
constexpr int TSEL_WAVES = TSEL_BLOCK / SG_WAVE;
constexpr uint32_t TSEL_WAVE_MAX = 1024;      // candidates a wave ranks by itself; more: the workgroup kernel
constexpr int TSEL_MAX_TOPN = 2048;           // LDS of the workgroup kernel's selected set (16 bytes an entry)
constexpr int TSEL_BIG_GRID = 512;

// A score as an unsigned key with the order of the value (values of either sign, +inf included; -0.0 gets the key of +0.0:
// the multiply compares values, to which the two are equal), zero-extended to 64 bits so that both value types share one
// comparison
__device__ inline uint64_t score_key(float v) {
    const uint32_t b = __float_as_uint(v);
    if ((b << 1) == 0) return 0x80000000ull;
    return (uint64_t)((b & 0x80000000u) ? ~b : (b | 0x80000000u));
}
__device__ inline uint64_t score_key(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    if ((b << 1) == 0) return 0x8000000000000000ull;
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

// One result row through the filter, by the wave that owns it: the row's first c entries without those whose column is in
// dead[0 .. n_dead), the others renumbered, at most stride_out of them written in their old order.  Returns the survivors
// (wave-uniform, cut or not).  `dead` is the list where the kernel keeps it: LDS, or global memory for a long one.
template <typename T>
__device__ inline int32_t drop_dead_of_row(const int32_t *__restrict__ row_cols, const T *__restrict__ row_vals, int32_t c,
                                           const int32_t *dead, int32_t n_dead, int32_t stride_out,
                                           int32_t *__restrict__ out_cols, T *__restrict__ out_vals, int lane) {
    const uint64_t below = (1ull << lane) - 1ull;                // the lanes before this one
    int32_t base = 0;                                            // survivors so far (wave-uniform, as are the loop's bounds)
    for (int32_t j0 = 0; j0 < c && base < stride_out; j0 += SG_WAVE) {
        const int32_t j = j0 + lane;
        const bool mine = j < c;
        const int32_t col = mine ? row_cols[j] : 0;
        const T v = mine ? row_vals[j] : T(0);
        int32_t lo = 0, hi = n_dead;                             // lo: dead columns below col
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (dead[mid] < col) lo = mid + 1;
            else hi = mid;
        }
        const bool gone = lo < n_dead && dead[lo] == col;
        const bool keep = mine && !gone;
        const uint64_t kept = __ballot(keep);
        const int32_t pos = base + (int32_t)__popcll(kept & below);
        if (keep && pos < stride_out) {
            out_cols[pos] = col - lo;
            out_vals[pos] = v;
        }
        base += (int32_t)__popcll(kept);
    }
    return base;
}

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
    const int64_t step = (int64_t)gridDim.x * TSEL_WAVES;
    for (int64_t r = (int64_t)blockIdx.x * TSEL_WAVES + threadIdx.x / SG_WAVE; r < n_rows; r += step) {
        const int32_t c = min(max(counts[r], 0), stride_in);
        const int32_t left = drop_dead_of_row<T>(cols + r * (int64_t)stride_in, vals + r * (int64_t)stride_in, c,
                                                 IN_LDS ? lds_dead : dead, n_dead, stride_out,
                                                 out_cols + r * (int64_t)stride_out, out_vals + r * (int64_t)stride_out, lane);
        if (lane == 0) out_counts[r] = min(left, stride_out);
    }
}

// ---- sg_topn_concat_rows, sg_topn_put_rows: whole rows from one fixed-stride result into another
// The first c entries of a row by the wave that owns it.  VEC: both rows start on a 16-byte boundary in both arrays (the
// strides are multiples of four entries), a lane moves four entries; the slots between c and the end of its last unit lie
// inside both rows and hold nothing anybody reads.
template <typename T, bool VEC>
__device__ inline void copy_row(const int32_t *__restrict__ src_cols, const T *__restrict__ src_vals, int32_t c,
                                int32_t *__restrict__ dst_cols, T *__restrict__ dst_vals, int lane) {
    if (VEC) {
        const uint4 *sc = reinterpret_cast<const uint4 *>(src_cols);
        const uint4 *sv = reinterpret_cast<const uint4 *>(src_vals);
        uint4 *dc = reinterpret_cast<uint4 *>(dst_cols);
        uint4 *dv = reinterpret_cast<uint4 *>(dst_vals);
        for (int32_t u = lane; u < (c + 3) >> 2; u += SG_WAVE) {
            dc[u] = sc[u];
            if (sizeof(T) == 4) {
                dv[u] = sv[u];
            } else {
                const uint4 v0 = sv[2 * u], v1 = sv[2 * u + 1];
                dv[2 * u] = v0;
                dv[2 * u + 1] = v1;
            }
        }
    } else {
        for (int32_t j = lane; j < c; j += SG_WAVE) {
            dst_cols[j] = src_cols[j];
            dst_vals[j] = src_vals[j];
        }
    }
}

// row k of the source becomes row rows[k] of the destination (rows == null: row row_off + k); a row number outside the
// destination is passed over
template <typename T, bool VEC>
__global__ void __launch_bounds__(TSEL_BLOCK) topn_copy_rows_kernel(const int32_t *__restrict__ cols,
                                                                    const T *__restrict__ vals,
                                                                    const int32_t *__restrict__ counts, int64_t n_rows,
                                                                    int32_t stride_in, const int32_t *__restrict__ rows,
                                                                    int64_t row_off, int64_t n_rows_out, int32_t stride_out,
                                                                    int32_t *__restrict__ out_cols, T *__restrict__ out_vals,
                                                                    int32_t *__restrict__ out_counts) {
    const int lane = threadIdx.x & (SG_WAVE - 1);
    const int64_t step = (int64_t)gridDim.x * TSEL_WAVES;
    for (int64_t k = (int64_t)blockIdx.x * TSEL_WAVES + threadIdx.x / SG_WAVE; k < n_rows; k += step) {
        const int64_t to = rows != nullptr ? (int64_t)rows[k] : row_off + k;
        if (to < 0 || to >= n_rows_out) continue;                // (wave-uniform)
        const int32_t c = min(min(max(counts[k], 0), stride_in), stride_out);
        copy_row<T, VEC>(cols + k * (int64_t)stride_in, vals + k * (int64_t)stride_in, c, out_cols + to * (int64_t)stride_out,
                         out_vals + to * (int64_t)stride_out, lane);
        if (lane == 0) out_counts[to] = c;
    }
}

template <typename T>
int copy_rows(sg_ctx *ctx, const sg_topn *src, const int32_t *d_rows, int64_t row_off, sg_topn *dst) {
    if (src->n_rows == 0) return SG_OK;
    const int grid = (int)std::min<int64_t>((src->n_rows + TSEL_WAVES - 1) / TSEL_WAVES, (int64_t)ctx->num_cu * 16);
    if (src->stride % 4 == 0 && dst->stride % 4 == 0)
        hipLaunchKernelGGL((topn_copy_rows_kernel<T, true>), dim3(grid), dim3(TSEL_BLOCK), 0, ctx->stream,
                           (const int32_t *)src->d_cols, (const T *)src->d_vals, (const int32_t *)src->d_counts, src->n_rows,
                           src->stride, d_rows, row_off, dst->n_rows, dst->stride, dst->d_cols, (T *)dst->d_vals,
                           dst->d_counts);
    else
        hipLaunchKernelGGL((topn_copy_rows_kernel<T, false>), dim3(grid), dim3(TSEL_BLOCK), 0, ctx->stream,
                           (const int32_t *)src->d_cols, (const T *)src->d_vals, (const int32_t *)src->d_counts, src->n_rows,
                           src->stride, d_rows, row_off, dst->n_rows, dst->stride, dst->d_cols, (T *)dst->d_vals,
                           dst->d_counts);
    SG_HIP_TRY(hipGetLastError());
    return SG_OK;
}

// ---- sg_topn_forget: a square result without the rows AND the columns of the dead list.  short_flag has one entry per
// surviving row and a zero behind the last, so that its prefix sum ends with the number of flagged rows.
template <typename T, bool IN_LDS>
__global__ void __launch_bounds__(TSEL_BLOCK) forget_kernel(const int32_t *__restrict__ cols, const T *__restrict__ vals,
                                                            const int32_t *__restrict__ counts, int64_t n_rows_in,
                                                            int64_t n_rows_out, int32_t stride_in,
                                                            const int32_t *__restrict__ dead, int32_t n_dead, int32_t top_n,
                                                            int32_t stride_out, int32_t *__restrict__ out_cols,
                                                            T *__restrict__ out_vals, int32_t *__restrict__ out_counts,
                                                            int32_t *__restrict__ short_flag) {
    __shared__ int32_t lds_dead[IN_LDS ? DROP_LDS_MAX : 1];
    if (IN_LDS) {
        for (int i = threadIdx.x; i < n_dead; i += TSEL_BLOCK) lds_dead[i] = dead[i];
        __syncthreads();
    }
    const int32_t *dl = IN_LDS ? lds_dead : dead;
    const int lane = threadIdx.x & (SG_WAVE - 1);
    const int64_t step = (int64_t)gridDim.x * TSEL_WAVES;
    if (blockIdx.x == 0 && threadIdx.x == 0) short_flag[n_rows_out] = 0;
    for (int64_t k = (int64_t)blockIdx.x * TSEL_WAVES + threadIdx.x / SG_WAVE; k < n_rows_out; k += step) {
        // surviving row k lay at k + the dead rows before it: dead row i has dead[i] - i survivors before it
        int32_t lo = 0, hi = n_dead;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if ((int64_t)dl[mid] - mid <= k) lo = mid + 1;
            else hi = mid;
        }
        const int64_t r = k + lo;
        int32_t c = 0, left = 0;
        if (r < n_rows_in) {                                     // (a list that is what the header asks for never fails this)
            c = min(max(counts[r], 0), stride_in);
            left = drop_dead_of_row<T>(cols + r * (int64_t)stride_in, vals + r * (int64_t)stride_in, c, dl, n_dead, stride_out,
                                       out_cols + k * (int64_t)stride_out, out_vals + k * (int64_t)stride_out, lane);
            left = min(left, stride_out);
        }
        if (lane == 0) {
            out_counts[k] = left;
            short_flag[k] = (c >= top_n && left < top_n) ? 1 : 0;
        }
    }
}

__global__ void __launch_bounds__(TSEL_BLOCK) short_rows_kernel(const int32_t *__restrict__ short_flag,
                                                                const uint32_t *__restrict__ pos, int64_t n_rows,
                                                                int64_t n_short, int32_t *__restrict__ rows) {
    const int64_t step = (int64_t)gridDim.x * TSEL_BLOCK;
    for (int64_t k = (int64_t)blockIdx.x * TSEL_BLOCK + threadIdx.x; k < n_rows; k += step)
        if (short_flag[k] > 0 && (int64_t)pos[k] < n_short) rows[pos[k]] = (int32_t)k;
}

template <typename T>
int forget(sg_ctx *ctx, const sg_topn *in, const int32_t *d_dead, int32_t n_dead, int32_t top_n, sg_topn *r,
           int32_t *short_flag) {
    const int64_t waves = r->n_rows > 0 ? r->n_rows : 1;
    const int grid = (int)std::min<int64_t>((waves + TSEL_WAVES - 1) / TSEL_WAVES, (int64_t)ctx->num_cu * 16);
    const auto kernel = n_dead <= DROP_LDS_MAX ? forget_kernel<T, true> : forget_kernel<T, false>;   // the list in LDS, or where it lies
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TSEL_BLOCK), 0, ctx->stream, (const int32_t *)in->d_cols, (const T *)in->d_vals,
                       (const int32_t *)in->d_counts, in->n_rows, r->n_rows, in->stride, d_dead, n_dead, top_n, r->stride,
                       r->d_cols, (T *)r->d_vals, r->d_counts, short_flag);
    SG_HIP_TRY(hipGetLastError());
    return SG_OK;
}

template <typename T>
int drop_columns(sg_ctx *ctx, const sg_topn *in, const int32_t *d_dead, int32_t n_dead, sg_topn *r) {
    const int64_t waves = in->n_rows > 0 ? in->n_rows : 1;
    const int grid = (int)std::min<int64_t>((waves + TSEL_WAVES - 1) / TSEL_WAVES, (int64_t)ctx->num_cu * 16);
    const auto kernel = n_dead <= DROP_LDS_MAX ? drop_columns_kernel<T, true> : drop_columns_kernel<T, false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TSEL_BLOCK), 0, ctx->stream, (const int32_t *)in->d_cols, (const T *)in->d_vals,
                       (const int32_t *)in->d_counts, in->n_rows, in->stride, d_dead, n_dead, r->stride, r->d_cols,
                       (T *)r->d_vals, r->d_counts);
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
    SG_TRY(sg_fetch(ctx, ctx->h_fetch, flags, sizeof(h_flags)));
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
    int32_t stride = 0;
    if (!result_stride(n_rows_out, top_n, n_cols, &stride)) return result_overflow(n_rows_out, stride, "");
    TopnPtr r;
    SG_TRY(topn_alloc(ctx, n_rows_out, n_cols, stride, pairs->dtype, &r));
    // scratch: counters (n_out + 1), offsets (n_out + 1), flags {error bits, queued rows}, the queue, the buckets (at most
    // one entry per slot of the pair list)
    const size_t slots = (size_t)pairs->n_rows * (size_t)pairs->stride + 1;
    Scratch scratch(ctx);
    uint32_t *cnt = nullptr, *off = nullptr, *flags = nullptr, *big_rows = nullptr;
    int32_t *b_rows = nullptr;
    void *b_vals = nullptr;
    SG_TRY(scratch.alloc((size_t)n_rows_out + 1, &cnt));
    SG_TRY(scratch.alloc((size_t)n_rows_out + 1, &off));
    SG_TRY(scratch.alloc((size_t)64, &flags));
    SG_TRY(scratch.alloc((size_t)n_rows_out + 1, &big_rows));
    SG_TRY(scratch.alloc(slots, &b_rows));
    SG_TRY(scratch.alloc_bytes(slots * (pairs->dtype == SG_F64 ? 8 : 4), &b_vals));
    SG_TRY(SG_ZERO2(ctx, cnt, ((size_t)n_rows_out + 1) * 4, flags, 64 * 4));
    SG_TRY(by_dtype(pairs->dtype, [&](auto t) {
        using T = decltype(t);
        return transpose_select<T>(ctx, pairs, n_rows_out, top_n, r.get(), cnt, off, flags, big_rows, b_rows, (T *)b_vals);
    }));
    *out = r.release();
    return SG_OK;
}

extern "C" int sg_topn_drop_columns(sg_ctx *ctx, const sg_topn *r_in, const int32_t *d_dead_sorted, int32_t n_dead,
                                    int32_t top_n, sg_topn **out) {
    SG_REQUIRE(ctx && r_in && out, "null argument");
    SG_REQUIRE(top_n >= 1, "top_n must be at least 1");
    SG_REQUIRE(n_dead >= 0 && (int64_t)n_dead <= r_in->n_cols, "more dead columns than the result has columns");
    SG_REQUIRE(n_dead == 0 || d_dead_sorted != nullptr, "the list of dead columns is null");
    TopnPtr r;
    SG_TRY(topn_alloc(ctx, r_in->n_rows, r_in->n_cols - n_dead, std::max<int32_t>(std::min<int32_t>(top_n, r_in->stride), 1),
                      r_in->dtype, &r));
    SG_TRY(by_dtype(r->dtype, [&](auto t) { return drop_columns<decltype(t)>(ctx, r_in, d_dead_sorted, n_dead, r.get()); }));
    *out = r.release();
    return SG_OK;
}

extern "C" int sg_topn_concat_rows(sg_ctx *ctx, const sg_topn *const *parts, int32_t n_parts, sg_topn **out) {
    SG_REQUIRE(ctx && parts && out && n_parts >= 1, "null argument or no parts");
    int64_t n_rows = 0;
    int32_t stride = 1;
    for (int p = 0; p < n_parts; ++p) {
        SG_REQUIRE(parts[p] != nullptr, "a part is null");
        SG_REQUIRE(parts[p]->n_cols == parts[0]->n_cols && parts[p]->dtype == parts[0]->dtype,
                   "parts disagree in columns or dtype");
        n_rows += parts[p]->n_rows;
        stride = std::max(stride, parts[p]->stride);
    }
    if ((double)n_rows * (double)stride > 2.0e9) {
        sg_set_error("result of %lld rows x stride %d does not fit the 32-bit result index", (long long)n_rows, stride);
        return SG_ERR_OVERFLOW;
    }
    TopnPtr r;
    SG_TRY(topn_alloc(ctx, n_rows, parts[0]->n_cols, stride, parts[0]->dtype, &r));
    int64_t row_off = 0;
    for (int p = 0; p < n_parts; ++p) {
        SG_TRY(r->dtype == SG_F64 ? copy_rows<double>(ctx, parts[p], nullptr, row_off, r.get())
                                  : copy_rows<float>(ctx, parts[p], nullptr, row_off, r.get()));
        row_off += parts[p]->n_rows;
    }
    *out = r.release();
    return SG_OK;
}

extern "C" int sg_topn_put_rows(sg_ctx *ctx, sg_topn *r, const int32_t *d_rows, int64_t n_rows, const sg_topn *src) {
    SG_REQUIRE(ctx && r && src, "null argument");
    SG_REQUIRE(n_rows == src->n_rows, "as many row numbers as src has rows are expected");
    SG_REQUIRE(n_rows == 0 || d_rows != nullptr, "the list of rows is null");
    SG_REQUIRE(src->n_cols == r->n_cols && src->dtype == r->dtype, "src and r disagree in columns or dtype");
    SG_REQUIRE(src->stride <= r->stride, "src has the longer rows");
    SG_REQUIRE(n_rows <= r->n_rows, "more rows than r has");
    return r->dtype == SG_F64 ? copy_rows<double>(ctx, src, d_rows, 0, r) : copy_rows<float>(ctx, src, d_rows, 0, r);
}

extern "C" int sg_topn_forget(sg_ctx *ctx, const sg_topn *r_in, const int32_t *d_dead_sorted, int32_t n_dead, int32_t top_n,
                              sg_topn **out, int32_t **d_short_rows, int64_t *n_short_rows) {
    SG_REQUIRE(ctx && r_in && out && d_short_rows && n_short_rows, "null argument");
    SG_REQUIRE(top_n >= 1, "top_n must be at least 1");
    SG_REQUIRE(r_in->n_rows == r_in->n_cols, "the result is not square");
    SG_REQUIRE(n_dead >= 0 && (int64_t)n_dead <= r_in->n_rows, "more dead rows than the result has rows");
    SG_REQUIRE(n_dead == 0 || d_dead_sorted != nullptr, "the list of dead rows is null");
    const int64_t n_out = r_in->n_rows - n_dead;
    TopnPtr r;
    SG_TRY(topn_alloc(ctx, n_out, n_out, r_in->stride, r_in->dtype, &r));
    Scratch scratch(ctx);
    int32_t *short_flag = nullptr, *rows = nullptr;
    uint32_t *pos = nullptr;
    SG_TRY(scratch.alloc((size_t)n_out + 1, &short_flag));
    SG_TRY(scratch.alloc((size_t)n_out + 1, &pos));
    SG_TRY(r->dtype == SG_F64 ? forget<double>(ctx, r_in, d_dead_sorted, n_dead, top_n, r.get(), short_flag)
                              : forget<float>(ctx, r_in, d_dead_sorted, n_dead, top_n, r.get(), short_flag));
    // (the flag behind the last row is zero: pos[n_out] = the number of flagged rows, the one thing that comes back)
    SG_TRY(sg_exclusive_scan_positive_i32(ctx, short_flag, pos, n_out + 1, nullptr));
    SG_HIP_TRY(hipMemcpyAsync(ctx->h_fetch, pos + n_out, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP_TRY(hipStreamSynchronize(ctx->stream));
    const int64_t n_short = (int64_t)ctx->h_fetch[0];
    SG_TRY(scratch.alloc((size_t)std::max<int64_t>(n_short, 4), &rows));
    if (n_short > 0) {
        const int grid = (int)std::min<int64_t>((n_out + TSEL_BLOCK - 1) / TSEL_BLOCK, (int64_t)ctx->num_cu * 16);
        hipLaunchKernelGGL(short_rows_kernel, dim3(grid), dim3(TSEL_BLOCK), 0, ctx->stream, (const int32_t *)short_flag,
                           (const uint32_t *)pos, n_out, n_short, rows);
        SG_HIP_TRY(hipGetLastError());
    }
    *d_short_rows = scratch.keep(rows);
    *n_short_rows = n_short;
    *out = r.release();
    return SG_OK;
}
