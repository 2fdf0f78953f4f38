// The merge of two CSR rows by a group of SG_PAIR_LANES lanes, shared by the kernels that score NAMED pairs: pairs_dot_kernel
// (sg_pairs.hip) and rescore_score_kernel (sg_rescore.hip).  The value is the multiply's:
//     acc = +0.0;  for every column k that both rows hold, ascending:  acc = rn(acc + rn(A[i, k] * B[j, k]))
// The two rows are walked in chunks of eight entries, one entry a lane (a chunk is one 32-byte piece of the column array and
// one of the values).  Every lane compares its entry of A's chunk with the eight columns of B's chunk (shuffles inside the
// group), the chunk whose last column is the smaller one is retired and the next one loaded -- a merge by chunks -- and when a
// chunk of A is retired its products are added lane by lane, lowest first, into an accumulator that every lane of the group
// holds: the order of the adds is the column order whatever the chunking.
#ifndef SG_PAIRS_DEVICE_H
#define SG_PAIRS_DEVICE_H
#include "sg_k4_device.h"

#define SG_PAIR_LANES 8

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
// live + n_dead: inside the matrix whenever its rows are the live rows + n_dead, whatever the list holds.  (sg_rescore.hip and
// sg_union.hip: a resident corpus keeps removed rows in place, results number the live ones.)
__device__ __forceinline__ int64_t physical_row(int64_t live, const int32_t *__restrict__ dead, int32_t n_dead) {
    int32_t lo = 0, hi = n_dead;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if ((int64_t)dead[mid] - mid <= live) lo = mid + 1;
        else hi = mid;
    }
    return live + lo;
}

// Column order is what the merge rests on. A matrix the vectoriser made has it by construction, one the cosine gate has
// passed (sg_csr_props) has been measured; any other is checked by the kernel, row by row, for the rows the pairs name.
static inline bool known_ascending(const sg_csr *m) { return m->props_state == 1 || (m->props_state == 0 && m->from_vectoriser); }

#endif   // SG_PAIRS_DEVICE_H
