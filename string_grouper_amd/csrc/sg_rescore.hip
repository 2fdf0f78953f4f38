// Rescoring a top-n result on further fields (include/sg_hip.h: sg_topn_rescore; DESIGN.md section 4, "Record rescoring").
// Every candidate (i, j, s_0) of a fixed-stride result is scored on F further pairs of CSR matrices, the scores are weighed into
//     c = +0.0;  c = rn(c + rn(W_0 * s_0));  for f = 1 .. F:  c = rn(c + rn(W_f * s_f))
// and every row is filtered (c > threshold), ordered (c descending by value, then column ascending) and cut.  Candidates never
// leave the device: what the named-pairs route moves through the host per field -- two position lists up, the scores down --
// is read here where the multiply left it.
//
// Two launches.  rescore_score_kernel: SG_PAIR_LANES lanes a row (of at most SG_PAIR_ROW_CHUNK of its entries; a longer row is
// dealt to several groups), field by field, with the walk of sg_pairs_device.h -- pairs_dot_kernel's, so s_f is
// sg_csr_pairs_dot's value to the bit: the row of A_f is found once, then the row's candidates are scored one by one -- and
// lane 0 keeps c in a scratch array of the candidates' shape.  rescore_select_*_kernel: a rank by counting -- an entry's place is the number of
// kept entries of its row that go before it -- which needs no sort network and no exchange between lanes: eight lanes a row
// reading the row's few scores from cache for a row of at most 64 candidates (rows of name lists hold about four), a block
// with the row in LDS for the rows above that (up to 2 048 entries), which the first kernel lists on the device.
//
// Floors (a call with a floor that is not a NaN): the same two launches with a floor a field in the filter (s_f > m_f, before the
// cut).  The scoring kernel has a second instantiation for it (FLOORS, below); the select kernels are the same ones: a refused
// candidate's c is a NaN.
//
// skip_empty: the same launches again, with a field that is EMPTY for a pair -- a row without entries on either side -- left out
// of the pair's sum and its weight shared among the others (SKIP, below: a third instantiation).  One entry, sg_topn_rescore,
// chooses the instantiation by what its call description holds.
#include "sg_pairs_device.h"

#define SG_RESCORE_BLOCK 256
#define SG_RESCORE_MAX_FIELDS 7
#define SG_RESCORE_MAX_STRIDE 2048
#define SG_RESCORE_SHORT 64        // rows of up to this many candidates: eight lanes select them; above: a block

// status word of a call: bit 0 a candidate column outside [0, N); bit 1 + 2 f / 2 + 2 f a row of A_f / B_f that a candidate
// reads and that is not in strictly ascending column order
#define SG_RESCORE_BAD_COLUMN 1u

template <typename T>
struct RescoreFields {
    PairField<T> f[SG_RESCORE_MAX_FIELDS];
};

// Floors (sg_rescore_call.floors): a candidate must ALSO have s_f > m_f on every field f that has a floor, s_0 -- the score it
// carries -- included.  `has`: bit 0 the primary's floor, bit f that of further field f; without a bit the value is not read.
template <typename T>
struct RescoreFloors {
    T m[SG_RESCORE_MAX_FIELDS + 1];
    uint32_t has;
};
struct NoFloors {};

// Empty fields (sg_rescore_call.skip_empty): field f is empty for the pair (i, j) when the physical row of A_f or of B_f has no
// entries.  `floors`: as above (has == 0: none).  The primary's row bounds and dead lists say whether field 0 -- the score the
// candidate carries -- is empty (a_indptr null: never); nothing else of the primary is read.  `empty`: a byte a candidate, the
// candidates' shape: bit 0 field 0, bit f + 1 further field f, set where the RIGHT row is the empty one (a left row that is
// empty skips the field for the whole row of candidates: the group keeps those bits itself).
template <typename T>
struct RescoreSkip {
    RescoreFloors<T> floors;
    const int64_t *a_indptr, *b_indptr;
    const int32_t *dead_a, *dead_b;
    int32_t n_dead_a, n_dead_b;
    uint8_t *empty;
};
template <typename T, bool FLOORS, bool SKIP>
using RescoreExtra = std::conditional_t<SKIP, RescoreSkip<T>, std::conditional_t<FLOORS, RescoreFloors<T>, NoFloors>>;
__device__ __forceinline__ const NoFloors &floors_of(const NoFloors &x) { return x; }
template <typename T>
__device__ __forceinline__ const RescoreFloors<T> &floors_of(const RescoreFloors<T> &x) { return x; }
template <typename T>
__device__ __forceinline__ const RescoreFloors<T> &floors_of(const RescoreSkip<T> &x) { return x.floors; }

// one correctly rounded IEEE division in T: no reciprocal, no fused step (the project's flags compile `/` to the
// v_div_scale / v_div_fmas / v_div_fixup sequence in both types)
template <typename T>
__device__ __forceinline__ T div_rn(T a, T b) { return a / b; }

// FLOORS: the group follows the candidates a floor has refused in a mask of its own -- SG_PAIR_ROW_CHUNK = 64 entries at most,
// a bit an entry, the same value in every lane because pair_score returns the score in every lane.  A refused candidate gets a
// NaN as its c (the select kernels pass over a NaN) and is skipped on every later field: no row of B_f' is read for it, and
// whether a merge runs never waits for a load of comb.  Only a floor sets a bit: a NaN that the data makes walks on, as without
// floors.  So the column order of a matrix that is not known to be sorted is looked at for the rows that are READ: a row that
// only refused candidates name is not.
//
// SKIP (with FLOORS): three steps.  Field 0 first, for every candidate of the group: is it empty for the pair (the primary's row
// bounds), else the primary's floor, and c starts as +0.0 or rn(+0.0 + rn(W_0 * s_0)).  Then the fields as above, but a left row
// without entries skips the field for the whole row of candidates -- nothing of B_f is read -- and a right row without entries
// skips it for the candidate, before any floor of that field and without a merge; lane 0 notes it in the candidate's byte.  At
// the end lane 0 rescales every candidate that has an empty field: wp from the weights of the fields that are NOT empty, in
// ascending field order (the loops are unrolled: the byte selects, nothing in a register is indexed by it), then
// rn(rn(c * wt) / wp), or a NaN when wp is not above 0 (every field empty).  A candidate without an empty field keeps c's bits.
template <typename T, bool FLOORS, bool SKIP = false>
__global__ void __launch_bounds__(SG_PAIR_BLOCK) rescore_score_kernel(
    const int32_t *__restrict__ cols, const T *__restrict__ vals, const int32_t *__restrict__ counts, int64_t n_rows,
    int64_t n_cols, int32_t stride, int32_t chunks, T w0, RescoreFields<T> fields, int32_t n_fields, uint32_t *status,
    T *__restrict__ comb, RescoreExtra<T, FLOORS, SKIP> extra) {
    static_assert(FLOORS || !SKIP, "SKIP carries the floors' mask");
    const auto &floors = floors_of(extra);
    constexpr int G = SG_PAIR_LANES;
    const int l = threadIdx.x & (G - 1);
    const int group_shift = threadIdx.x & (SG_WAVE - 1) & ~(G - 1);   // the group's first lane in its wave
    const int64_t g = ((int64_t)blockIdx.x * SG_PAIR_BLOCK + threadIdx.x) / G;
    const int64_t row = g / chunks;
    if (row >= n_rows) return;   // (everything below is uniform over the group: its lanes leave, loop and shuffle together)
    const int32_t cnt = counted(counts, row, stride);
    const int32_t e0 = (int32_t)(g - row * chunks) * SG_PAIR_ROW_CHUNK;
    const int32_t e1 = cnt < e0 + SG_PAIR_ROW_CHUNK ? cnt : e0 + SG_PAIR_ROW_CHUNK;
    if (e0 >= e1) return;
    const int64_t base = row * (int64_t)stride;
    uint64_t failed = 0;   // (FLOORS) bit e - e0: a floor has refused entry e
    uint32_t left_empty = 0;   // (SKIP) bit 0: the primary's left row has no entries; bit f + 1: further field f's
    if constexpr (SKIP) {
        if (extra.a_indptr) {
            const int64_t a = physical_row(row, extra.dead_a, extra.n_dead_a);
            if (extra.a_indptr[a + 1] == extra.a_indptr[a]) left_empty = 1u;
        }
        for (int32_t e = e0; e < e1; ++e) {   // (every lane reads the same words: `failed` is the group's)
            const int64_t j = cols[base + e];
            if (j < 0 || j >= n_cols) {   // nothing of a field is read for it; the call is refused
                failed |= (uint64_t)1 << (e - e0);
                if (l == 0) {
                    atomicOr(status, SG_RESCORE_BAD_COLUMN);
                    comb[base + e] = (T)NAN;
                }
                continue;
            }
            bool right_empty = false;
            if (!left_empty && extra.b_indptr) {
                const int64_t b = physical_row(j, extra.dead_b, extra.n_dead_b);
                right_empty = extra.b_indptr[b + 1] == extra.b_indptr[b];
            }
            const bool empty0 = left_empty || right_empty;
            const T s0 = vals[base + e];
            if (!empty0 && (floors.has & 1u) && !(s0 > floors.m[0])) {   // the primary's floor: not held where field 0 is empty
                failed |= (uint64_t)1 << (e - e0);
                if (l == 0) comb[base + e] = (T)NAN;
                continue;
            }
            if (l == 0) {
                comb[base + e] = empty0 ? (T)0 : add_rn<T>((T)0, mul_rn<T>(w0, s0));
                extra.empty[base + e] = right_empty ? 1 : 0;
            }
        }
    }
    for (int f = 0; f < n_fields; ++f) {
        const PairField<T> &F = fields.f[f];
        int64_t a0, a1;
        pair_left_row<T>(F, row, l, status, 2u << (2 * f), a0, a1);
        if constexpr (SKIP)
            if (a0 == a1) {   // empty on the left: the whole row of candidates skips the field
                left_empty |= 2u << f;
                continue;
            }
        for (int32_t e = e0; e < e1; ++e) {
            if constexpr (FLOORS)
                if ((failed >> (e - e0)) & 1) continue;
            const int64_t j = cols[base + e];
            if (j < 0 || j >= n_cols) {   // nothing of a field is read for it; the call is refused
                if (l == 0 && f == 0) {
                    atomicOr(status, SG_RESCORE_BAD_COLUMN);
                    comb[base + e] = (T)NAN;
                }
                continue;
            }
            if constexpr (FLOORS && !SKIP) {   // the primary's floor, before anything of a field is read (every lane reads the score)
                if (f == 0 && (floors.has & 1u) && !(vals[base + e] > floors.m[0])) {
                    failed |= (uint64_t)1 << (e - e0);
                    if (l == 0) comb[base + e] = (T)NAN;
                    continue;
                }
            }
            T s;
            if constexpr (SKIP) {
                int64_t b0, b1;
                pair_right_row<T>(F, j, b0, b1);
                if (b0 == b1) {   // empty on the right: no floor of the field is held, nothing is merged
                    if (l == 0) extra.empty[base + e] |= (uint8_t)(2u << f);
                    continue;
                }
                s = pair_score_rows<T>(F, a0, a1, b0, b1, l, group_shift, status, 4u << (2 * f));
            } else {
                s = pair_score<T>(F, a0, a1, j, l, group_shift, status, 4u << (2 * f));
            }
            if constexpr (FLOORS) {
                if (((floors.has >> (f + 1)) & 1u) && !(s > floors.m[f + 1])) {
                    failed |= (uint64_t)1 << (e - e0);
                    if (l == 0) comb[base + e] = (T)NAN;
                    continue;
                }
            }
            if (l == 0) {   // (lane 0 alone reads and writes the candidate's c: its own stores, in program order)
                const T c = !SKIP && f == 0 ? add_rn<T>((T)0, mul_rn<T>(w0, vals[base + e])) : comb[base + e];
                comb[base + e] = add_rn<T>(c, mul_rn<T>(F.w, s));
            }
        }
    }
    if constexpr (SKIP) {
        if (l != 0) return;   // (no lane of the group shuffles from here on)
        T wt = add_rn<T>((T)0, w0);
#pragma unroll
        for (int f = 0; f < SG_RESCORE_MAX_FIELDS; ++f)
            if (f < n_fields) wt = add_rn<T>(wt, fields.f[f].w);
        for (int32_t e = e0; e < e1; ++e) {
            if ((failed >> (e - e0)) & 1) continue;
            const uint32_t empty = left_empty | extra.empty[base + e];
            if (!empty) continue;   // c as it is, to the bit
            T wp = (T)0;
            if (!(empty & 1u)) wp = add_rn<T>(wp, w0);
#pragma unroll
            for (int f = 0; f < SG_RESCORE_MAX_FIELDS; ++f)
                if (f < n_fields && !((empty >> (f + 1)) & 1u)) wp = add_rn<T>(wp, fields.f[f].w);
            comb[base + e] = wp > (T)0 ? div_rn<T>(mul_rn<T>(comb[base + e], wt), wp) : (T)NAN;
        }
    }
}

// An entry that fails the filter takes part in nothing: as a NaN it neither goes before another entry nor equals one.
template <typename T>
__device__ __forceinline__ T kept_or_nan(T c, T threshold) {
    return c > threshold ? c : (T)NAN;
}
// does the kept entry (cq, jq) at place q go before the kept entry (c, j) at place e?  By value (zeros of either sign are
// equal), then by column, then -- for a caller-made result that names a column twice -- by place, so that ranks are distinct.
template <typename T>
__device__ __forceinline__ bool goes_before(T cq, int32_t jq, int32_t q, T c, int32_t j, int32_t e) {
    return cq > c || (cq == c && (jq < j || (jq == j && q < e)));
}

template <typename T>
__global__ void __launch_bounds__(SG_RESCORE_BLOCK) rescore_select_short_kernel(
    const int32_t *__restrict__ cols, const T *__restrict__ comb, const int32_t *__restrict__ counts, int64_t n_rows,
    int32_t stride, T threshold, int32_t stride_out, int32_t *__restrict__ out_cols, T *__restrict__ out_vals,
    int32_t *__restrict__ out_counts, int32_t *__restrict__ long_rows, uint32_t *n_long) {
    constexpr int G = SG_PAIR_LANES;
    const int l = threadIdx.x & (G - 1);
    const int64_t row = ((int64_t)blockIdx.x * SG_RESCORE_BLOCK + threadIdx.x) / G;
    if (row >= n_rows) return;
    const int32_t cnt = counted(counts, row, stride);
    if (cnt > SG_RESCORE_SHORT) {   // (only with a stride above SG_RESCORE_SHORT: the list is there) a block's row
        if (l == 0) long_rows[atomicAdd(n_long, 1u)] = (int32_t)row;
        return;
    }
    const int32_t *rc = cols + row * (int64_t)stride;
    const T *rs = comb + row * (int64_t)stride;
    const int64_t out = row * (int64_t)stride_out;
    for (int32_t e = l; e < cnt; e += G) {
        const T c = kept_or_nan<T>(rs[e], threshold);
        if (!(c == c)) continue;
        const int32_t j = rc[e];
        int32_t rank = 0;
        for (int32_t q = 0; q < cnt; ++q) rank += goes_before<T>(kept_or_nan<T>(rs[q], threshold), rc[q], q, c, j, e) ? 1 : 0;
        if (rank < stride_out) {
            out_cols[out + rank] = j;
            out_vals[out + rank] = c;
        }
    }
    if (l == 0) {
        int32_t kept = 0;
        for (int32_t q = 0; q < cnt; ++q) kept += rs[q] > threshold ? 1 : 0;
        out_counts[row] = kept < stride_out ? kept : stride_out;
    }
}

// The rows the short kernel listed (more than SG_RESCORE_SHORT candidates), a block a row at a time: the grid is fixed, a block
// takes the list's entries blockIdx.x, blockIdx.x + gridDim.x, ...  The order of the list is the order the groups arrived in;
// every row is written by its own block alone, so it shows nowhere.
template <typename T>
__global__ void __launch_bounds__(SG_RESCORE_BLOCK) rescore_select_block_kernel(
    const int32_t *__restrict__ cols, const T *__restrict__ comb, const int32_t *__restrict__ counts, int32_t stride,
    T threshold, int32_t stride_out, int32_t *__restrict__ out_cols, T *__restrict__ out_vals,
    int32_t *__restrict__ out_counts, const int32_t *__restrict__ long_rows, const uint32_t *__restrict__ n_long) {
    __shared__ T s_c[SG_RESCORE_MAX_STRIDE];
    __shared__ int32_t s_j[SG_RESCORE_MAX_STRIDE];
    __shared__ int32_t s_kept;
    const uint32_t n = *n_long;
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        const int64_t row = long_rows[k];
        const int32_t cnt = counted(counts, row, stride);   // (stride <= SG_RESCORE_MAX_STRIDE: checked by the driver)
        const int64_t base = row * (int64_t)stride, out = row * (int64_t)stride_out;
        if (threadIdx.x == 0) s_kept = 0;
        __syncthreads();
        int32_t mine = 0;
        for (int32_t e = threadIdx.x; e < cnt; e += SG_RESCORE_BLOCK) {
            const T c = kept_or_nan<T>(comb[base + e], threshold);
            s_c[e] = c;
            s_j[e] = cols[base + e];
            mine += c == c ? 1 : 0;
        }
        if (mine) atomicAdd(&s_kept, mine);
        __syncthreads();
        for (int32_t e = threadIdx.x; e < cnt; e += SG_RESCORE_BLOCK) {
            const T c = s_c[e];
            if (!(c == c)) continue;
            const int32_t j = s_j[e];
            int32_t rank = 0;
            for (int32_t q = 0; q < cnt; ++q) rank += goes_before<T>(s_c[q], s_j[q], q, c, j, e) ? 1 : 0;
            if (rank < stride_out) {
                out_cols[out + rank] = j;
                out_vals[out + rank] = c;
            }
        }
        if (threadIdx.x == 0) out_counts[row] = s_kept < stride_out ? s_kept : stride_out;
        __syncthreads();   // the next row reuses the block's LDS
    }
}

template <typename T>
static int rescore(sg_ctx *ctx, const sg_topn *cand, const sg_rescore_call &call, sg_topn *r, uint32_t *d_status, void *d_comb,
                   int32_t *d_long_rows, uint8_t *d_empty) {
    RescoreFields<T> dev;
    memset(&dev, 0, sizeof(dev));
    for (int f = 0; f < call.n_fields; ++f) dev.f[f] = make_pair_field<T>(call.fields[f]);
    constexpr int per_block = SG_RESCORE_BLOCK / SG_PAIR_LANES;
    const int32_t chunks = (cand->stride + SG_PAIR_ROW_CHUNK - 1) / SG_PAIR_ROW_CHUNK;
    const dim3 grid_score((unsigned)pair_blocks(cand->n_rows * chunks));
    // the scoring kernel's one launch: the type of `extra` chooses the instantiation
    auto score = [&](auto extra) {
        constexpr bool skip = std::is_same_v<decltype(extra), RescoreSkip<T>>;
        constexpr bool floors = skip || std::is_same_v<decltype(extra), RescoreFloors<T>>;
        hipLaunchKernelGGL((rescore_score_kernel<T, floors, skip>), grid_score, dim3(SG_PAIR_BLOCK), 0, ctx->stream, cand->d_cols,
                           (const T *)cand->d_vals, cand->d_counts, cand->n_rows, cand->n_cols, cand->stride, chunks, (T)call.w0,
                           dev, call.n_fields, d_status, (T *)d_comb, extra);
    };
    RescoreFloors<T> m;
    memset(&m, 0, sizeof(m));
    for (int f = 0; call.floors && f <= call.n_fields; ++f)
        if (!std::isnan(call.floors[f])) m.m[f] = (T)call.floors[f], m.has |= 1u << f;
    if (call.skip_empty) {
        RescoreSkip<T> x;
        memset(&x, 0, sizeof(x));
        x.floors = m, x.empty = d_empty;
        if (const sg_rescore_field *p = call.primary) {
            x.a_indptr = p->A->d_indptr, x.b_indptr = p->B->d_indptr;
            x.dead_a = p->d_dead_a, x.dead_b = p->d_dead_b;
            x.n_dead_a = p->n_dead_a, x.n_dead_b = p->n_dead_b;
        }
        score(x);
    } else if (!m.has) {   // no floor, or every one a NaN: the plain statement's kernel, whose bits the floors' would give
        score(NoFloors{});
    } else {
        score(m);
    }
    SG_HIP_TRY(hipGetLastError());
    // the select kernel is chosen ROW BY ROW: eight lanes for a row of up to SG_RESCORE_SHORT candidates, whatever the stride;
    // the rows above it are listed on the device (no read-back) and taken by a fixed grid of blocks
    const int64_t blocks = (cand->n_rows + per_block - 1) / per_block;
    hipLaunchKernelGGL(rescore_select_short_kernel<T>, dim3((unsigned)blocks), dim3(SG_RESCORE_BLOCK), 0, ctx->stream,
                       cand->d_cols, (const T *)d_comb, cand->d_counts, cand->n_rows, cand->stride, (T)call.threshold, r->stride,
                       r->d_cols, (T *)r->d_vals, r->d_counts, d_long_rows, d_status + 1);
    if (cand->stride > SG_RESCORE_SHORT) {
        SG_HIP_TRY(hipGetLastError());
        const int64_t grid = std::min<int64_t>(cand->n_rows, (int64_t)ctx->num_cu * 8);
        hipLaunchKernelGGL(rescore_select_block_kernel<T>, dim3((unsigned)grid), dim3(SG_RESCORE_BLOCK), 0, ctx->stream,
                           cand->d_cols, (const T *)d_comb, cand->d_counts, cand->stride, (T)call.threshold, r->stride, r->d_cols,
                           (T *)r->d_vals, r->d_counts, d_long_rows, d_status + 1);
    }
    SG_HIP_TRY(hipGetLastError());
    return SG_OK;
}

// floors: null, or n_fields + 1 doubles -- the primary's first -- a NaN for a field without one; skip_empty with its primary
// (null: field 0 is never empty)
extern "C" int sg_topn_rescore(sg_ctx *ctx, const sg_topn *cand, const sg_rescore_call *call, sg_topn **out) {
    SG_REQUIRE(ctx && cand && call && out, "null argument");
    const int32_t n_fields = call->n_fields;
    const sg_rescore_field *const fields = call->fields, *const primary = call->primary;
    SG_REQUIRE(n_fields >= 1 && n_fields <= SG_RESCORE_MAX_FIELDS, "between 1 and 7 further fields are expected");
    SG_REQUIRE(fields != nullptr, "null argument");
    SG_REQUIRE(!primary || call->skip_empty, "a primary field is read with skip_empty alone");
    SG_REQUIRE(call->top_n >= 1, "top_n must be at least 1");
    SG_REQUIRE(cand->stride >= 1 && cand->stride <= SG_RESCORE_MAX_STRIDE, "the candidates' stride exceeds 2048: ask the multiply for fewer a row");
    SG_REQUIRE(weight_ok(call->w0, cand->dtype), "a weight is not finite");
    for (int f = 0; call->floors && f <= n_fields; ++f) SG_REQUIRE(!std::isinf(call->floors[f]), "a floor is infinite");
    for (int f = 0; f < n_fields; ++f)
        SG_TRY(check_pair_field(fields[f], cand->dtype, cand->n_rows, cand->n_cols, "a field's", "candidates", true));
    if (primary) SG_TRY(check_pair_field(*primary, cand->dtype, cand->n_rows, cand->n_cols, "the primary field's", "candidates", false));
    const int64_t chunks = (cand->stride + SG_PAIR_ROW_CHUNK - 1) / SG_PAIR_ROW_CHUNK;
    if (pair_blocks(cand->n_rows * chunks) > INT32_MAX || cand->n_rows > INT32_MAX)
        return exceeds_one_launch(cand->n_rows, "rows of candidates", "rescore");
    for (int f = 0; f < n_fields; ++f) SG_TRY(ensure_pair_rows(ctx, fields[f].A, fields[f].B));
    if (primary) SG_TRY(ensure_pair_rows(ctx, primary->A, primary->B));
    TopnPtr r;
    SG_TRY(topn_alloc(ctx, cand->n_rows, cand->n_cols, std::min<int32_t>(call->top_n, cand->stride), cand->dtype, &r));
    if (cand->n_rows == 0) {
        *out = r.release();
        return SG_OK;
    }
    const size_t s = cand->dtype == SG_F64 ? 8 : 4, head = 16;   // the status word and the long rows' counter, then c of every candidate
    Scratch tmp(ctx);
    char *d_buf = nullptr;
    SG_TRY(tmp.alloc(head + (size_t)cand->n_rows * (size_t)cand->stride * s, &d_buf));
    int32_t *d_long_rows = nullptr;   // the rows of more than SG_RESCORE_SHORT candidates (word 1 of the head counts them)
    if (cand->stride > SG_RESCORE_SHORT) SG_TRY(tmp.alloc((size_t)cand->n_rows, &d_long_rows));
    uint8_t *d_empty = nullptr;       // (skip_empty) a byte a candidate: the fields whose right row is empty
    if (call->skip_empty) SG_TRY(tmp.alloc((size_t)cand->n_rows * (size_t)cand->stride, &d_empty));
    SG_HIP_TRY(hipMemsetAsync(d_buf, 0, head, ctx->stream));
    SG_TRY(by_dtype(cand->dtype, [&](auto t) {
        return rescore<decltype(t)>(ctx, cand, *call, r.get(), (uint32_t *)d_buf, d_buf + head, d_long_rows, d_empty);
    }));
    uint32_t status = 0;
    SG_TRY(sg_fetch(ctx, &status, d_buf, 4));   // the one read-back
    if (status) {
        std::string what;
        if (status & SG_RESCORE_BAD_COLUMN) what += "a candidate's column lies outside the result's columns; ";
        for (int f = 0; f < n_fields; ++f) {
            const std::string field = "field " + std::to_string(f + 1);
            if (status & (2u << (2 * f))) what += unsorted_row(field + "'s left matrix", "candidate reads");
            if (status & (4u << (2 * f))) what += unsorted_row(field + "'s right matrix", "candidate reads");
        }
        sg_set_error("bad argument: %s", what.c_str());
        return SG_ERR_BADARG;
    }
    *out = r.release();
    return SG_OK;
}
