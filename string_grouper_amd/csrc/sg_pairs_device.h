// What the kernels that score NAMED pairs share: pairs_dot_kernel (sg_pairs.hip), rescore_score_kernel (sg_rescore.hip) and
// union_fill_kernel (sg_union.hip), and the host checks of their three drivers.  The value is the multiply's (DESIGN.md
// section 2):
//     acc = +0.0;  for every column k that both rows hold, ascending:  acc = rn(acc + rn(A[i, k] * B[j, k]))
// The walk ("Pair similarities"): a group of SG_PAIR_LANES lanes takes a left row and the columns named
// for it.  pair_left_row finds the row of A, pair_score scores one column j against it: both turn a live row number into a
// physical one (physical_row), read the row's bounds, look at its column order where the matrix is not known to be sorted
// (a bit of the caller's status word), and pair_score then merges the two rows (pair_rows_dot).
// The merge: the two rows are walked in chunks of eight entries, one entry a lane (a chunk is one 32-byte piece of the column
// array and one of the values).  Every lane compares its entry of A's chunk with the eight columns of B's chunk (shuffles inside
// the group), the chunk whose last column is the smaller one is retired and the next one loaded -- a merge by chunks -- and when
// a chunk of A is retired its products are added lane by lane, lowest first, into an accumulator that every lane of the group
// holds: the order of the adds is the column order whatever the chunking.
#ifndef SG_PAIRS_DEVICE_H
#define SG_PAIRS_DEVICE_H
#include "sg_k4_device.h"

#define SG_PAIR_LANES 8
#define SG_PAIR_BLOCK 256        // threads of a block of the three kernels: 32 groups
#define SG_PAIR_ROW_CHUNK 64     // entries of a candidate row one group walks (a longer row is dealt to several groups)

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

// Entries [a0, a1) of A's arrays against entries [b0, b1) of B's.  Called by all SG_PAIR_LANES lanes of a group together with
// the same arguments but `l`, the lane's place in its group; `group_shift` is the group's first lane in its wave.  Every lane
// returns the score.
template <typename T>
__device__ __forceinline__ T pair_rows_dot(const int32_t *__restrict__ a_indices, const T *__restrict__ a_data, int64_t a0,
                                           int64_t a1, const int32_t *__restrict__ b_indices, const T *__restrict__ b_data,
                                           int64_t b0, int64_t b1, int l, int group_shift) {
    constexpr int G = SG_PAIR_LANES;
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
    return acc;
}

// live row -> physical row: live + #{q : dead[q] - q <= live} (CorpusState.physical_rows: searchsorted(dead - arange, live,
// side="right")).  dead[q] - q never falls as q grows, so the count is found by bisection.  The result is at most
// live + n_dead: inside the matrix whenever its rows are the live rows + n_dead, whatever the list holds.  (A resident corpus
// keeps removed rows in place, results number the live ones.)
__device__ __forceinline__ int64_t physical_row(int64_t live, const int32_t *__restrict__ dead, int32_t n_dead) {
    int32_t lo = 0, hi = n_dead;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if ((int64_t)dead[mid] - mid <= live) lo = mid + 1;
        else hi = mid;
    }
    return live + lo;
}

// the entries of row `row` of a fixed-stride result that count: its count, kept inside [0, stride]
__device__ __forceinline__ int32_t counted(const int32_t *__restrict__ counts, int64_t row, int32_t stride) {
    const int32_t c = counts[row];
    return c < 0 ? 0 : (c > stride ? stride : c);
}

// One field of a call: the CSR arrays of the left and the right records' matrices.
template <typename T>
struct PairField {
    const int64_t *a_indptr;
    const int32_t *a_indices;
    const T *a_data;
    const int64_t *b_indptr;
    const int32_t *b_indices;
    const T *b_data;
    const int32_t *dead_a, *dead_b;   // dead PHYSICAL rows, ascending and distinct (null: none)
    int32_t n_dead_a, n_dead_b;
    int32_t check_a, check_b;         // != 0: the matrix is not known to be sorted, look at the rows that are read
    T w;                              // the field's weight (sg_topn_rescore alone reads it)
};

// The two halves of the walk.  All SG_PAIR_LANES lanes of a group call them together with the same arguments but `l`, as they
// call pair_rows_dot.  pair_left_row: the entries [a0, a1) of A's arrays that the live row `live` holds.  pair_score: the score
// of that row and the live row j of B, in every lane.  A row found out of column order sets `bit` in *status.
template <typename T>
__device__ __forceinline__ void pair_left_row(const PairField<T> &F, int64_t live, int l, uint32_t *status, uint32_t bit,
                                              int64_t &a0, int64_t &a1) {
    const int64_t a = physical_row(live, F.dead_a, F.n_dead_a);
    a0 = F.a_indptr[a], a1 = F.a_indptr[a + 1];
    if (F.check_a && row_not_ascending(F.a_indices, a0, a1, l)) atomicOr(status, bit);
}
// (pair_score's two halves on their own, for a caller that asks whether the row of B holds entries before it merges:
// pair_right_row finds the entries [b0, b1) of the live row j, pair_score_rows looks at their order and merges)
template <typename T>
__device__ __forceinline__ void pair_right_row(const PairField<T> &F, int64_t j, int64_t &b0, int64_t &b1) {
    const int64_t b = physical_row(j, F.dead_b, F.n_dead_b);
    b0 = F.b_indptr[b], b1 = F.b_indptr[b + 1];
}
template <typename T>
__device__ __forceinline__ T pair_score_rows(const PairField<T> &F, int64_t a0, int64_t a1, int64_t b0, int64_t b1, int l,
                                             int group_shift, uint32_t *status, uint32_t bit) {
    if (F.check_b && row_not_ascending(F.b_indices, b0, b1, l)) atomicOr(status, bit);
    return pair_rows_dot<T>(F.a_indices, F.a_data, a0, a1, F.b_indices, F.b_data, b0, b1, l, group_shift);
}
template <typename T>
__device__ __forceinline__ T pair_score(const PairField<T> &F, int64_t a0, int64_t a1, int64_t j, int l, int group_shift,
                                        uint32_t *status, uint32_t bit) {
    const int64_t b = physical_row(j, F.dead_b, F.n_dead_b);
    const int64_t b0 = F.b_indptr[b], b1 = F.b_indptr[b + 1];
    if (F.check_b && row_not_ascending(F.b_indices, b0, b1, l)) atomicOr(status, bit);
    return pair_rows_dot<T>(F.a_indices, F.a_data, a0, a1, F.b_indices, F.b_data, b0, b1, l, group_shift);
}

// ---------------------------------------------------------------------------------------------
// The host side of a field, shared by sg_csr_pairs_dot, sg_topn_rescore and sg_topn_union.

// Column order is what the merge rests on. A matrix the vectoriser made has it by construction, one the cosine gate has
// passed (sg_csr_props) has been measured; any other is checked by the kernel, row by row, for the rows the pairs name.
static inline bool known_ascending(const sg_csr *m) { return m->props_state == 1 || (m->props_state == 0 && m->from_vectoriser); }

template <typename T>
static PairField<T> make_pair_field(const sg_rescore_field &h) {
    PairField<T> d;
    d.a_indptr = h.A->d_indptr, d.a_indices = h.A->d_indices, d.a_data = (const T *)h.A->d_data;
    d.b_indptr = h.B->d_indptr, d.b_indices = h.B->d_indices, d.b_data = (const T *)h.B->d_data;
    d.dead_a = h.d_dead_a, d.dead_b = h.d_dead_b, d.n_dead_a = h.n_dead_a, d.n_dead_b = h.n_dead_b;
    d.check_a = !known_ascending(h.A), d.check_b = !known_ascending(h.B);
    d.w = (T)h.weight;
    return d;
}

static inline bool weight_ok(double w, int32_t dtype) { return std::isfinite(w) && (dtype == SG_F64 || std::isfinite((float)w)); }

// A field against the value type and the R x N shape of what names its pairs.  The refusals name the field as `whose` and the
// other side as `of`: "a field's" / "candidates" for a rescoring, "the primary field's" / "parts" for a union, whose field
// carries no weight that counts (`weighed` false).
static inline int check_pair_field(const sg_rescore_field &h, int32_t dtype, int64_t R, int64_t N, const std::string &whose,
                                   const std::string &of, bool weighed) {
    SG_REQUIRE(h.A && h.B, (whose + " matrix is null").c_str());
    SG_REQUIRE(!weighed || weight_ok(h.weight, dtype), "a weight is not finite");
    SG_REQUIRE(h.A->dtype == dtype && h.B->dtype == dtype, (whose + " matrices differ from the " + of + " in value type").c_str());
    SG_REQUIRE(h.A->n_cols == h.B->n_cols, (whose + " matrices differ in shape (their columns)").c_str());
    SG_REQUIRE(h.n_dead_a >= 0 && h.n_dead_b >= 0 && (h.n_dead_a == 0 || h.d_dead_a) && (h.n_dead_b == 0 || h.d_dead_b),
               "a list of dead rows is null or has a negative length");
    SG_REQUIRE(h.A->n_rows - h.n_dead_a == R, (whose + " left matrix has not the " + of + "' rows (dead rows apart)").c_str());
    SG_REQUIRE(h.B->n_rows - h.n_dead_b == N, (whose + " right matrix has not the " + of + "' columns as rows (dead rows apart)").c_str());
    return SG_OK;
}

// the rows of a matrix may be pending (rows_of): they are made before a kernel reads them
static inline int ensure_pair_rows(sg_ctx *ctx, const sg_csr *A, const sg_csr *B) {
    if (A->rows_of) SG_TRY(sg_csr_ensure_rows(ctx, A));
    if (B->rows_of && B != A) SG_TRY(sg_csr_ensure_rows(ctx, B));
    return SG_OK;
}

// blocks of SG_PAIR_BLOCK threads that hold `groups` groups; a launch takes at most INT32_MAX of them
static inline int64_t pair_blocks(int64_t groups) {
    constexpr int per_block = SG_PAIR_BLOCK / SG_PAIR_LANES;
    return (groups + per_block - 1) / per_block;
}
static inline int exceeds_one_launch(int64_t n, const char *what, const char *verb) {
    sg_set_error("%lld %s exceed one launch: %s them in pieces", (long long)n, what, verb);
    return SG_ERR_OVERFLOW;
}

// a status report's sentence for a row out of column order: "A" / "pair names", "field 1's left matrix" / "candidate reads"
static inline std::string unsorted_row(const std::string &of, const char *reader) {
    return "a row of " + of + " that a " + reader + " is not sorted by column (strictly ascending); ";
}

#endif   // SG_PAIRS_DEVICE_H
