// K4 -- thresholded sparse top-n multiply  C = topn_rowwise(A . B^T restricted to > threshold)
// (K5, the top-n merge of column-block results, and the result handle itself: sg_topn.hip)
//
// Replaces sparse_dot_topn.sp_matmul_topn as called from string_grouper/string_grouper.py:725-732 and :737-743 of the
// reference.
//
// Algorithm (row-wise Gustavson product, MI355X shape).  One 64-lane wave owns one left row i at a
// time and a private accumulator tile of TILE = 2^TILE_LOG2 values in LDS (single-wave workgroups:
// no barriers anywhere, LDS is allocated in wave-sized grains, and up to 160 KiB / (TILE * s) waves
// are resident per CU).  For every column tile t of the right-hand side and every non-zero (k, a) of
// row i IN ASCENDING k, the wave streams segment (k, t) of the inverted index (sg_postings.hip) with
// coalesced loads -- lane l takes posting slo + l -- and does a plain LDS read-add-write per lane
// (LDS float atomics cost ~190 cycles per wave instruction here and were dropped after v2):
//         acc[j - t*TILE] += a * b            (product rounded, then sum rounded: no FMA)
// All j inside one segment are distinct, so one wave instruction never carries two updates of the
// same accumulator (the read-add-write is race-free), and DS instructions of one wave execute in issue
// order, so every accumulator
// receives its products in ascending k: the same order scipy / sparse_dot_topn use, hence bit-equal
// scores (a requirement for bit-equal match indices next to the threshold and at the top-n cut).
// After the last k the wave sweeps its tile with 16-byte LDS reads (re-zeroing as it goes), finds
// values > threshold by ballot and inserts them into a sorted top-n list held one entry per lane
// in registers (order: score descending, then column ascending).  Rows are handed out by a global
// atomic counter (persistent waves) which balances the skew of name data (a few n-grams are present
// in 20 % of all rows).
//
// Column tiles are processed in groups by separate launches ("tile groups").  All waves of one
// launch stream the same few MB of postings, so these stay resident in each XCD's 4 MiB L2; the
// per-row top-n state lives in the output arrays between launches.
//
// Roofline: HBM/cache bandwidth bound, no MFMA (0.25 flop per byte; scatter, not a dense contraction).
// Algorithmic bytes per intermediate product ("MAC"): 4 + s (one (j, value) posting), plus
// nnz(A)*(4+s) + out -- see DESIGN.md.
#include <cstring>
#include <math.h>

#include <memory>

#include "sg_internal.h"

#include "sg_k4_device.h"
#include "sg_plan.h"

static_assert(SG_PLAN_LANES == SG_TOPN_LANES, "sg_plan.h counts passes and register lists in the kernels' lanes");

// "does any of the 16 bytes' worth of accumulators exceed thr": accumulators and thr are >= +0, so
// IEEE order equals unsigned integer order and one v_max3_u32 + v_max_u32 + compare covers 4 floats
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
template <typename T, typename V>
__device__ __forceinline__ bool any_above(const V &v, T thr);
template <>
__device__ __forceinline__ bool any_above<float, f32x4>(const f32x4 &v, float thr) {
    const uint32_t a = __float_as_uint(v[0]), b = __float_as_uint(v[1]), c = __float_as_uint(v[2]),
                   d = __float_as_uint(v[3]);
    const uint32_t ab = a > b ? a : b, cd = c > d ? c : d;
    return (ab > cd ? ab : cd) > __float_as_uint(thr);
}
template <>
__device__ __forceinline__ bool any_above<double, f64x2>(const f64x2 &v, double thr) {
    return __builtin_fmax(v[0], v[1]) > thr;
}

// The accumulator tile is the kernel's only LDS object, so it starts at LDS address 0 and a posting's
// "slot" IS the LDS address: form the pointer from the integer instead of adding a base per access.
template <typename T>
__device__ __forceinline__ T *acc_at(T *, uint32_t byte_off) {
    typedef __attribute__((address_space(3))) T lds_t;
    return (T *)(lds_t *)(uintptr_t)byte_off;
}

// One posting segment (term k, column tile t) = entries [lo, lo + n).  All its columns are distinct,
// so a plain LDS read-add-write per lane is race-free, and because the segments of a row are visited
// in ascending k and DS instructions of a wave execute in order, every accumulator receives its
// products in ascending k -- the reference's summation order, hence bit-equal scores.
// (LDS float atomics were measured at ~190 cycles per wave instruction and are not used.)
template <typename T>
struct StreamStep {   // 4 windows (256 entries) of one long posting list
    typename Post<T>::reg_t r[4];
    __device__ __forceinline__ void load(const char *vals, const char *slots, uint32_t lo, uint32_t n, uint32_t off,
                                         int lane) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t p = min(off + u * 64 + lane, n - 1u);   // clamp, not mask: idle lanes re-read the last entry
            r[u] = Post<T>::load(vals, slots, lo, p);
        }
    }
    __device__ __forceinline__ void apply(T *acc, uint32_t n, uint32_t off, T a, int lane) const {
        T cur[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) cur[u] = *acc_at(acc, Post<T>::slot(r[u]));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const T sum = add_rn<T>(cur[u], mul_rn<T>(a, Post<T>::val(r[u])));
            if (off + u * 64 + lane < n) *acc_at(acc, Post<T>::slot(r[u])) = sum;
        }
    }
};

// Entries beyond the first window of a long posting list ('inc', 'llc', ...).  Software-pipelined:
// the loads of step i+1 are in flight while step i is applied (two register sets, ping-pong), because
// at ~1 us per L2/MALL round trip a load-wait-apply loop left the waves waiting 2/3 of the time.
template <typename T>
__device__ __forceinline__ void stream_rest(T *acc, const char *vals, const char *slots, uint32_t lo, uint32_t n, T a,
                                            int lane) {
    StreamStep<T> s0, s1;
    uint32_t off = 64;
    s0.load(vals, slots, lo, n, off, lane);
    for (;;) {   // loads are unconditional (clamped indices) so that the compiler can count them: vmcnt(4)
        s1.load(vals, slots, lo, n, off + 256, lane);
        s0.apply(acc, n, off, a, lane);
        if (off + 256 >= n) break;
        s0.load(vals, slots, lo, n, off + 512, lane);
        s1.apply(acc, n, off + 256, a, lane);
        if (off + 512 >= n) break;
        off += 512;
    }
}

// wave-uniform "clear bit f of m" in one scalar instruction (the compiler expands m &= m - 1 to three)
__device__ __forceinline__ void clear_bit(uint64_t &m, int f) {
#ifdef SG_WATCHDOG   // the watchdog's breaks make m look divergent to the compiler: no scalar asm then
    m &= ~(1ull << f);
#else
    asm("s_bitset0_b64 %0, %1" : "+s"(m) : "s"(f));
#endif
}

// One batch of up to NB posting segments of the current (row, tile): issue the first window of each,
// then read-add-write them in ascending k.  Lanes beyond a short segment re-read its last entry (no
// exec masking on the load or the LDS read); only the LDS write is masked.
template <typename T, int NB, bool PARTIAL>
__device__ __forceinline__ void segment_batch(T *acc, const char *vals, const char *slots, uint64_t &m, uint32_t lo,
                                              uint32_t hi, T a, int lane) {
    uint32_t slo[NB], sn[NB];
    T sa[NB];
    bool has[NB];
    typename Post<T>::reg_t r[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        has[b] = PARTIAL ? (m != 0) : true;
        if (has[b]) {
            const int f = __builtin_ctzll(m);
            clear_bit(m, f);
            slo[b] = wave_read<uint32_t>(lo, f);
            sn[b] = wave_read<uint32_t>(hi, f) - slo[b];
            sa[b] = wave_read<T>(a, f);
            r[b] = Post<T>::load(vals, slots, slo[b], min((uint32_t)lane, sn[b] - 1u));
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (has[b]) {
            T *slot = acc_at(acc, Post<T>::slot(r[b]));
            const T sum = add_rn<T>(*slot, mul_rn<T>(sa[b], Post<T>::val(r[b])));
            if ((uint32_t)lane < sn[b]) *slot = sum;   // idle lanes computed a duplicate: drop it
            if (sn[b] > 64) stream_rest<T>(acc, vals, slots, slo[b], sn[b], sa[b], lane);
        }
    }
}

// Self-join launch (SELF): the mirrored pairs of the lanes in `mm` into the wave's chunk of the pair list -- the protocol of
// the pruned kernel's drain_survivors (sg_spgemm_pruned.hip); `pos` = chunk << 9 | entries used is the wave's state.
// Lane: row `rec` receives column `col` with score s; both: and row `col` receives
// column `rec` -- top_n above one register list, where a row's own matches go through the list as well): every lane writes
// its own entry, one chunk test and one count for the wave.  (One pair at a time by lane 0 was the whole cost of a hit: at a
// threshold of 0.4 a row has dozens.)
template <typename T>
__device__ __forceinline__ void emit_pairs(const SgPairSink &sk, uint32_t &pos, uint64_t mm, uint32_t col, uint32_t rec, T s,
                                           bool both, uint32_t col_uniform /* both: `col` is this one in every lane */, int lane) {
    const uint32_t n_hit = (uint32_t)__popcll(mm) << (both ? 1 : 0);   // <= 128
    if (pos == SG_PAIR_NO_CHUNK || (pos & 511u) + n_hit > SG_PAIR_CHUNK) {
        uint32_t c = 0;
        if (lane == 0) {
            if (pos != SG_PAIR_NO_CHUNK && (pos >> 9) < sk.chunks) {
                sk.d_chunk_count[pos >> 9] = pos & 511u;
                atomicAdd(sk.d_totals, (unsigned long long)(pos & 511u));
            }
            c = atomicAdd(sk.d_chunks_used, 1u);
        }
        pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)c) << 9;
    }
    if (((mm >> lane) & 1ull) && (pos >> 9) < sk.chunks) {   // past the capacity nothing is written: the caller falls back
        const size_t o = (size_t)(pos >> 9) * SG_PAIR_CHUNK + (pos & 511u) +
                         ((uint32_t)__popcll(mm & ((1ull << lane) - 1ull)) << (both ? 1 : 0));
        sk.d_i[o] = col;
        sk.d_j[o] = rec;
        reinterpret_cast<T *>(sk.d_s)[o] = s;
        atomicAdd(&sk.d_row_count[rec], 1u);
        if (both) {
            sk.d_i[o + 1] = rec;
            sk.d_j[o + 1] = col;
            reinterpret_cast<T *>(sk.d_s)[o + 1] = s;
        }
    }
    if (both && lane == 0 && (pos >> 9) < sk.chunks) atomicAdd(&sk.d_row_count[col_uniform], n_hit >> 1);
    pos += n_hit;
}

// SELF: the row scores the columns j <= row only (the tiles up to its own), keeps those matches and hands the
// mirrored pairs to `sink` -- the exact kernel standing in for the pruned one inside the self-join form.
template <typename T, int TILE_LOG2, int NB, bool SELF = false>
__device__ __forceinline__ void process_row(T *acc, uint32_t row, const int64_t *__restrict__ a_indptr,
                                            const int32_t *__restrict__ a_indices, const T *__restrict__ a_data,
                                            const uint32_t *__restrict__ seg, const int32_t *__restrict__ post_rows,
                                            const T *__restrict__ post_vals, int32_t n_tiles, int32_t tile_begin,
                                            int32_t tile_end, int32_t keep, int32_t pass_off, int32_t out_stride, T thr,
                                            int32_t *__restrict__ out_cols, T *__restrict__ out_vals,
                                            int32_t *__restrict__ out_cnt, int lane, const SgPairSink *sink = nullptr,
                                            uint32_t *pair_pos = nullptr,
                                            const uint32_t *__restrict__ orig_of = nullptr /* position -> right-hand row; null: identity */) {
    constexpr int TILE = 1 << TILE_LOG2;
    if (SELF) tile_end = min(tile_end, (int32_t)(row >> TILE_LOG2) + 1);
    // columns are POSITIONS of right-hand rows (the index is built over a permutation, sg_postings.hip); SELF: so is `row`,
    // and the left matrix is the permuted one.  The result names rows: row_out, and the columns as they are inserted.
    const uint32_t row_out = (SELF && orig_of) ? orig_of[row] : row;
    constexpr int VEC = 16 / sizeof(T);   // values per 16-byte LDS access
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    vec_t *acc_v = reinterpret_cast<vec_t *>(acc);
    const char *vals = reinterpret_cast<const char *>(post_vals);
    const char *slots = reinterpret_cast<const char *>(post_rows);

    const int64_t rlo = a_indptr[row];
    const int nnz = (int)(a_indptr[row + 1] - rlo);
    const size_t obase = (size_t)row_out * (size_t)out_stride + (size_t)pass_off;

    // ---- restore the row's running state (written by the previous tile group / pass)
    TopList<T> top;
    top.clear();
    T floor_s = INFINITY;
    int floor_c = -1;
    int prev_cnt = 0;
    if (tile_begin > 0 || pass_off > 0) prev_cnt = __builtin_amdgcn_readfirstlane(out_cnt[row_out]);
    if (pass_off > 0) {
        if (prev_cnt < pass_off) return;                // earlier passes did not fill up: row is complete
        floor_s = out_vals[obase - 1];
        floor_c = out_cols[obase - 1];
    }
    if (tile_begin > 0) {
        const int have = prev_cnt - pass_off;           // entries collected so far in this pass
        if (lane < have) {
            top.s = out_vals[obase + lane];
            top.c = out_cols[obase + lane];
        }
    }

    if (nnz > 0) {
        // first 64 non-zeros of the row stay in registers for all tiles (lane l holds non-zero l)
        int k0 = -1;
        T a0 = (T)0;
        if (lane < nnz) {
            k0 = a_indices[rlo + lane];
            a0 = a_data[rlo + lane];
        }
        // segment bounds of (k0, t): lo is the previous tile's hi; the next tile's hi is fetched
        // one tile ahead so that its latency hides behind this tile's work
        uint32_t lo0 = 0, hi0 = 0, hi_next = 0;
        if (k0 >= 0) {
            const uint32_t *sp = seg + (int64_t)k0 * n_tiles + tile_begin;
            lo0 = sp[0];
            hi0 = sp[1];
        }

        SG_WD_DECL(wd_t);
        for (int t = tile_begin; t < tile_end; ++t) {
            SG_WD(wd_t, n_tiles + 2, 2)
            if (k0 >= 0 && t + 1 < tile_end) hi_next = seg[(int64_t)k0 * n_tiles + t + 2];
            bool touched = false;
            SG_WD_DECL(wd_c);
            for (int c0 = 0; c0 < nnz; c0 += 64) {
                SG_WD(wd_c, 100000, 3)
                T a;
                uint32_t lo = 0, hi = 0;
                if (c0 == 0) {
                    a = a0;
                    lo = lo0;
                    hi = hi0;
                } else {
                    a = (T)0;
                    if (c0 + lane < nnz) {
                        const int k = a_indices[rlo + c0 + lane];
                        a = a_data[rlo + c0 + lane];
                        lo = seg[(int64_t)k * n_tiles + t];
                        hi = seg[(int64_t)k * n_tiles + t + 1];
                    }
                }
                uint64_t m = __ballot(hi > lo);   // non-empty segments, ascending lane == ascending k
                touched |= (m != 0);
                // batches of NB segments: the first-window loads of a batch are issued back to back, then
                // consumed in ascending k.  Full batches carry no per-segment "is there one" test.
                SG_WD_DECL(wd_m);
                while (__popcll(m) >= NB) {
                    SG_WD(wd_m, 70, 4)
                    segment_batch<T, NB, false>(acc, vals, slots, m, lo, hi, a, lane);
                }
                if (m) segment_batch<T, NB, true>(acc, vals, slots, m, lo, hi, a, lane);
            }
            lo0 = hi0;
            hi0 = hi_next;
            if (touched) {   // otherwise the accumulators are still all zero
                // ---- sweep the tile: find values > thr, re-zero
                const int col_base = t << TILE_LOG2;
                for (int x1 = 0; x1 < TILE / VEC; x1 += 256) {   // 4 stripes per step: reads first, then zero + test
                    vec_t vv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) vv[u] = acc_v[x1 + u * 64 + lane];
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc_v[x1 + u * 64 + lane] = (vec_t)(T)0;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const vec_t v = vv[u];
                        const int x0 = x1 + u * 64;
                        if (__ballot(any_above<T>(v, thr)) != 0) {   // rare: an accumulator of this stripe passes
#pragma unroll
                            for (int e = 0; e < VEC; ++e) {
                                // every lane's own hit: its position and -- one load for the wave, not one per hit -- the row
                                // behind it (equal scores are ordered by the ROW)
                                const int np_l = col_base + (x0 + lane) * VEC + e;
                                bool hit = v[e] > thr;
                                if (SELF) hit = hit && (uint32_t)np_l <= row;   // the pair (i, j > i) is row j's to score
                                uint64_t hm = __ballot(hit);
                                if (hm == 0) continue;
                                int nc_l = np_l;
                                if (orig_of && hit) nc_l = (int)orig_of[np_l];
                                if (SELF) {
                                    // the mirrored pairs ("row j receives column i") in one go; top_n above one register list:
                                    // the row's own matches through the pair list as well ("row i receives column j") -- the
                                    // second pass selects with lists of 128
                                    const uint64_t mm = __ballot(hit && (uint32_t)np_l < row);
                                    const bool both = keep > SG_TOPN_LANES;
                                    if (mm) emit_pairs<T>(*sink, *pair_pos, mm, row_out, (uint32_t)nc_l, v[e], both, row_out, lane);
                                    if (both) hm &= ~mm;   // (what is left: the diagonal)
                                }
                                SG_WD_DECL(wd_h);
                                while (hm) {
                                    SG_WD(wd_h, 70, 9)
                                    const int src = __builtin_ctzll(hm);
                                    hm &= hm - 1;
                                    const T ns = wave_read<T>(v[e], src);
                                    const int nc = wave_read<int>(nc_l, src);
                                    if (ns < floor_s || (ns == floor_s && nc > floor_c)) top.insert(ns, nc, lane);
                                }
                            }
                        }
                    }
                }
            }
        }
    }

    // ---- store the row's state (final when tile_end == n_tiles)
    int cnt = __popcll(__ballot(top.c != INT32_MAX));
    if (cnt > keep) cnt = keep;
    if (lane < cnt) {
        out_vals[obase + lane] = top.s;
        out_cols[obase + lane] = top.c;
    }
    if (lane == 0) out_cnt[row_out] = pass_off + cnt;
}

template <typename T, int TILE_LOG2, int NB>
__global__ void __launch_bounds__(64)
spgemm_topn_kernel(const int64_t *__restrict__ a_indptr, const int32_t *__restrict__ a_indices,
                   const T *__restrict__ a_data, uint32_t n_left, const uint32_t *__restrict__ seg,
                   const int32_t *__restrict__ post_rows, const T *__restrict__ post_vals, int32_t n_tiles,
                   int32_t tile_begin, int32_t tile_end, int32_t keep /* <= 64 entries this pass */,
                   int32_t pass_off /* 64 * pass */, int32_t out_stride, T thr, int32_t *__restrict__ out_cols,
                   T *__restrict__ out_vals, int32_t *__restrict__ out_cnt, uint32_t *row_counter,
                   const uint32_t *__restrict__ row_list /* null: all rows */,
                   const uint32_t *__restrict__ row_list_len, const uint32_t *__restrict__ orig_of) {
    constexpr int TILE = 1 << TILE_LOG2;
    constexpr int VEC = 16 / sizeof(T);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *acc = reinterpret_cast<T *>(smem);
    const int lane = threadIdx.x;
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    vec_t *acc_v = reinterpret_cast<vec_t *>(acc);
    for (int x = lane; x < TILE / VEC; x += 64) acc_v[x] = (vec_t)(T)0;
    if (row_list) n_left = row_list_len[0];   // only the rows the pruned kernel handed over (often none)

    SG_WD_DECL(wd_rows);
    for (uint32_t idx = next_row(row_counter, lane); idx < n_left; idx = next_row(row_counter, lane)) {
        SG_WD(wd_rows, n_left + 2, 1)
        const uint32_t row = row_list ? row_list[idx] : idx;
        process_row<T, TILE_LOG2, NB>(acc, row, a_indptr, a_indices, a_data, seg, post_rows, post_vals, n_tiles,
                                      tile_begin, tile_end, keep, pass_off, out_stride, thr, out_cols, out_vals,
                                      out_cnt, lane, nullptr, nullptr, orig_of);
    }
}

// The exact kernel inside the self-join form (sg_spgemm_pruned.hip, symmetric mode): the rows the pruned kernel
// cannot take -- more than 128 non-zeros, more than 64 prefix terms, no room for the fixed-point filter -- arrive as a
// list; each scores its pairs (i, j <= i) exactly over the tiles up to its own and appends the mirrored ones to the
// pair list like every other row of the pass.  (Before this launch existed one such row sent the whole multiply back
// to the one-sided form: twice the time at 663 k rows.)
template <typename T, int TILE_LOG2, int NB>
__global__ void __launch_bounds__(64)
spgemm_topn_selfjoin_rows_kernel(const int64_t *__restrict__ a_indptr, const int32_t *__restrict__ a_indices,
                                 const T *__restrict__ a_data, const uint32_t *__restrict__ seg,
                                 const int32_t *__restrict__ post_rows, const T *__restrict__ post_vals, int32_t n_tiles,
                                 int32_t keep, int32_t out_stride, T thr, int32_t *__restrict__ out_cols,
                                 T *__restrict__ out_vals, int32_t *__restrict__ out_cnt, uint32_t *row_counter,
                                 const uint32_t *__restrict__ row_list, const uint32_t *__restrict__ row_list_len,
                                 SgPairSink sink, const uint32_t *__restrict__ orig_of) {
    constexpr int TILE = 1 << TILE_LOG2;
    constexpr int VEC = 16 / sizeof(T);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *acc = reinterpret_cast<T *>(smem);
    const int lane = threadIdx.x;
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    vec_t *acc_v = reinterpret_cast<vec_t *>(acc);
    const uint32_t n_rows = (uint32_t)__builtin_amdgcn_readfirstlane((int)row_list_len[0]);
    if (blockIdx.x >= n_rows) return;   // (usually there is no such row at all)
    for (int x = lane; x < TILE / VEC; x += 64) acc_v[x] = (vec_t)(T)0;
    uint32_t pos = SG_PAIR_NO_CHUNK;
    SG_WD_DECL(wd_rows);
    for (uint32_t idx = next_row(row_counter, lane); idx < n_rows; idx = next_row(row_counter, lane)) {
        SG_WD(wd_rows, n_rows + 2, 1)
        const uint32_t row = (uint32_t)__builtin_amdgcn_readfirstlane((int)row_list[idx]);
        process_row<T, TILE_LOG2, NB, true>(acc, row, a_indptr, a_indices, a_data, seg, post_rows, post_vals, n_tiles, 0,
                                            n_tiles, keep, 0, out_stride, thr, out_cols, out_vals, out_cnt, lane, &sink, &pos, orig_of);
        // the pair list is full (this wave was handed a chunk past its end): the pass is thrown away by the caller, every
        // wave leaves at its next row (as in the pruned kernel)
        if (pos != SG_PAIR_NO_CHUNK && (pos >> 9) >= sink.chunks && lane == 0) atomicMax(row_counter, 0x20000000u);
    }
    if (lane == 0 && pos != SG_PAIR_NO_CHUNK && (pos >> 9) < sink.chunks) {   // close the wave's last chunk
        sink.d_chunk_count[pos >> 9] = pos & 511u;
        atomicAdd(sink.d_totals, (unsigned long long)(pos & 511u));
    }
}

// One atomic per workgroup: a counter word takes ~12 ns per atomic whoever sends it, so a thousand waves adding to it
// one by one cost more than the sum itself.
__device__ __forceinline__ void block_add_u64(unsigned long long local, unsigned long long *out) {
    __shared__ unsigned long long wave_sums[4];
    for (int d = 32; d > 0; d >>= 1) local += __shfl_down(local, d, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long s = wave_sums[0] + wave_sums[1] + wave_sums[2] + wave_sums[3];
        if (s) atomicAdd(out, s);
    }
}

// Sum over the non-zeros of A of the posting-list length of their term = number of intermediate
// products.  Measurement only (bench.py roofline).
__global__ void __launch_bounds__(256) count_macs_kernel(const int64_t *__restrict__ a_indptr,
                                                         const int32_t *__restrict__ a_indices, int64_t n_left,
                                                         const uint32_t *__restrict__ term_len,
                                                         unsigned long long *out_macs) {
    const int64_t p0 = a_indptr[0], p1 = a_indptr[n_left];
    unsigned long long local = 0;
    for (int64_t p = p0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < p1; p += (int64_t)gridDim.x * blockDim.x)
        local += term_len[a_indices[p]];
    block_add_u64(local, out_macs);
}

// top_n above the pruned kernel's register list: rows whose list came out full may have more matches -- the exact kernel
// redoes them (their result rows are overwritten pass by pass)
__global__ void __launch_bounds__(256) rows_with_full_lists_kernel(const int32_t *__restrict__ cnt, int64_t n_rows, int32_t full,
                                                                   uint32_t *handed_count, uint32_t *__restrict__ handed_rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rows && cnt[i] >= full) handed_rows[atomicAdd(handed_count, 1u)] = (uint32_t)i;
}

// ... of a self-join (A is the matrix the index was built over): the sum of the squared list lengths
__global__ void __launch_bounds__(256) count_macs_selfjoin_kernel(const uint32_t *__restrict__ term_len, int64_t n_terms,
                                                                  unsigned long long *out_macs) {
    unsigned long long local = 0;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_terms; k += (int64_t)gridDim.x * blockDim.x)
        local += (unsigned long long)term_len[k] * (unsigned long long)term_len[k];
    block_add_u64(local, out_macs);
}

__global__ void __launch_bounds__(256) row_cost_kernel(const int64_t *__restrict__ a_indptr,
                                                       const int32_t *__restrict__ a_indices, int64_t n_left,
                                                       const uint32_t *__restrict__ term_len,
                                                       int64_t *__restrict__ out_cost) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_left) return;
    int64_t c = 0;
    for (int64_t p = a_indptr[i]; p < a_indptr[i + 1]; ++p) c += term_len[a_indices[p]];
    out_cost[i] = c;
}

__global__ void __launch_bounds__(256) sum_counts_kernel(const int32_t *__restrict__ cnt, int64_t n,
                                                         unsigned long long *out) {
    unsigned long long local = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        local += (unsigned long long)cnt[i];
    block_add_u64(local, out);
}

// ================================================================================================
// host side
// ================================================================================================
template <typename T, int TILE_LOG2>
static int launch_spgemm(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int32_t tile_begin, int32_t tile_end,
                         int32_t keep, int32_t pass_off, sg_topn *r, T thr, uint32_t *counter, unsigned grid,
                         const uint32_t *row_list, const uint32_t *row_list_len) {
    const size_t lds = sizeof(T) << TILE_LOG2;
    constexpr auto kern = spgemm_topn_kernel<T, TILE_LOG2, 8>;
    SG_TRY(allow_dynamic_lds<kern>(lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64), lds, ctx->stream, A->d_indptr, A->d_indices, (const T *)A->d_data,
                       (uint32_t)A->n_rows, (const uint32_t *)Bt->d_seg, (const int32_t *)Bt->d_rows,
                       (const T *)Bt->d_vals, Bt->n_tiles, tile_begin, tile_end, keep, pass_off, r->stride, thr,
                       r->d_cols, (T *)r->d_vals, r->d_counts, counter, row_list, row_list_len, (const uint32_t *)Bt->d_orig_of);
    SG_HIP_TRY(hipGetLastError());
    return SG_OK;
}

template <typename T>
static int dispatch_spgemm(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int32_t tile_begin, int32_t tile_end,
                           int32_t keep, int32_t pass_off, sg_topn *r, T thr, uint32_t *counter, unsigned grid,
                           const uint32_t *row_list = nullptr, const uint32_t *row_list_len = nullptr) {
    switch (Bt->tile_log2) {
        case 10: return launch_spgemm<T, 10>(ctx, A, Bt, tile_begin, tile_end, keep, pass_off, r, thr, counter, grid, row_list, row_list_len);
        case 11: return launch_spgemm<T, 11>(ctx, A, Bt, tile_begin, tile_end, keep, pass_off, r, thr, counter, grid, row_list, row_list_len);
        case 12: return launch_spgemm<T, 12>(ctx, A, Bt, tile_begin, tile_end, keep, pass_off, r, thr, counter, grid, row_list, row_list_len);
        case 13: return launch_spgemm<T, 13>(ctx, A, Bt, tile_begin, tile_end, keep, pass_off, r, thr, counter, grid, row_list, row_list_len);
        default:
            sg_set_error("postings tile of 2^%d columns is not supported by the multiply (2^10..2^13)", Bt->tile_log2);
            return SG_ERR_UNSUPPORTED;
    }
}

// ---- the exact kernel's self-join launch over a device-side row list (see spgemm_topn_selfjoin_rows_kernel)
unsigned sg_spgemm_exact_selfjoin_grid(const sg_ctx *ctx, const sg_postings *Bt) {
    if (!Bt) return (unsigned)ctx->num_cu * 2u;   // a handful of rows, if any
    // every row of the matrix: as many single-wave workgroups as the accumulator tiles leave room for, like the one-sided launch
    return (unsigned)ctx->num_cu * (unsigned)sg_plan_waves_per_cu(ctx->lds_per_cu, Bt->dtype == SG_F64, Bt->tile_log2);
}

template <typename T, int TILE_LOG2>
static int launch_selfjoin_rows(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int32_t keep, sg_topn *r, T thr,
                                uint32_t *row_counter, const uint32_t *row_list, const uint32_t *row_list_len,
                                const SgPairSink &sink, bool all_rows) {
    const size_t lds = sizeof(T) << TILE_LOG2;
    constexpr auto kern = spgemm_topn_selfjoin_rows_kernel<T, TILE_LOG2, 8>;
    SG_TRY(allow_dynamic_lds<kern>(lds));
    hipLaunchKernelGGL(kern, dim3(sg_spgemm_exact_selfjoin_grid(ctx, all_rows ? Bt : nullptr)), dim3(64), lds, ctx->stream, A->d_indptr, A->d_indices,
                       (const T *)A->d_data, (const uint32_t *)Bt->d_seg, (const int32_t *)Bt->d_rows, (const T *)Bt->d_vals,
                       Bt->n_tiles, keep, r->stride, thr, r->d_cols, (T *)r->d_vals, r->d_counts, row_counter, row_list,
                       row_list_len, sink, (const uint32_t *)Bt->d_orig_of);
    SG_HIP_TRY(hipGetLastError());
    return SG_OK;
}

template <typename T>
static int dispatch_selfjoin_rows(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int32_t keep, sg_topn *r, T thr,
                                  uint32_t *row_counter, const uint32_t *row_list, const uint32_t *row_list_len,
                                  const SgPairSink &sink, bool all_rows) {
    switch (Bt->tile_log2) {
        case 10: return launch_selfjoin_rows<T, 10>(ctx, A, Bt, keep, r, thr, row_counter, row_list, row_list_len, sink, all_rows);
        case 11: return launch_selfjoin_rows<T, 11>(ctx, A, Bt, keep, r, thr, row_counter, row_list, row_list_len, sink, all_rows);
        case 12: return launch_selfjoin_rows<T, 12>(ctx, A, Bt, keep, r, thr, row_counter, row_list, row_list_len, sink, all_rows);
        case 13: return launch_selfjoin_rows<T, 13>(ctx, A, Bt, keep, r, thr, row_counter, row_list, row_list_len, sink, all_rows);
        default:
            sg_set_error("postings tile of 2^%d columns is not supported by the self-join form (2^10..2^13)", Bt->tile_log2);
            return SG_ERR_UNSUPPORTED;
    }
}

int sg_spgemm_exact_selfjoin_rows(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int32_t keep, sg_topn *r,
                                  double threshold, uint32_t *row_counter, const uint32_t *row_list,
                                  const uint32_t *row_list_len, const SgPairSink &sink, bool all_rows) {
    if (A->dtype == SG_F64)
        return dispatch_selfjoin_rows<double>(ctx, A, Bt, keep, r, (double)threshold, row_counter, row_list, row_list_len, sink, all_rows);
    return dispatch_selfjoin_rows<float>(ctx, A, Bt, keep, r, (float)threshold, row_counter, row_list, row_list_len, sink, all_rows);
}

// Algorithmic bytes of the multiply (stream model): macs*(4+s) + nnz(A)*(4+s) + (nL+V+2)*4 + out*(4+s); the MAC and
// output terms are added in sg_ctx_stats once the device counters are read
static void record_bytes(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, double threshold) {
    const size_t s = A->dtype == SG_F64 ? 8 : 4;
    ctx->spgemm_entry_bytes = (int64_t)(4 + s);
    ctx->spgemm_fixed_bytes = A->nnz * (int64_t)(4 + s) + (A->n_rows + Bt->n_terms + 2) * 4;
    // what a candidate of the first filter costs: with the second filter its 8-bit copy (header + 4 B an entry), and the
    // packed row only for those that pass it (no pointer fetch: the header holds it); without: pointer + packed row
    const double mean_row = Bt->n_right > 0 ? (double)Bt->nnz / (double)Bt->n_right : 0.0;
    ctx->prune_q8_bytes = sg_q8_applies(ctx, Bt, s == 8 ? threshold : (double)(float)threshold) ? 16.0 + 4.0 * mean_row : 0.0;
    ctx->prune_row_bytes = (ctx->prune_q8_bytes > 0.0 ? 0.0 : 8.0) + mean_row * (s == 8 ? 16.0 : 8.0);
}

// Three blocks of 512 left rows (start, middle, end) through the one-sided pruned kernel: what the filter passes per
// row, extrapolated, priced against the exact kernel (sg_plan_pilot_prices).  One host round trip.
static int prune_pilot(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, const SgPlanLeft &a, const SgPlanIndex &b,
                       int32_t stride, double threshold, double delta, bool selfjoin, SgPilotPrices *prices) {
    const int64_t block = 512;
    TopnPtr scratch;
    SG_TRY(topn_alloc(ctx, block, Bt->n_right, stride, A->dtype, &scratch));
    Scratch tmp(ctx);
    uint32_t *words = nullptr;            // [0] row counter [1] flagged count, then flagged rows
    unsigned long long *d_stats = nullptr;   // [0] rows [1] postings [2] survivors [3] MACs of the whole multiply [4] pairs scored exactly (the kernel's; eight words like sg_spgemm_pruned_symmetric)
    SG_TRY(tmp.alloc((size_t)block + 8, &words));
    SG_TRY(tmp.alloc((size_t)8, &d_stats));
    SG_HIP_TRY(hipMemsetAsync(d_stats, 0, 8 * sizeof(unsigned long long), ctx->stream));
    const int64_t starts[3] = {0, (A->n_rows - block) / 2, A->n_rows - block};
    for (int k = 0; k < 3; ++k) {
        sg_csr view = *A;
        view.n_rows = block;
        view.d_indptr = A->d_indptr + starts[k];
        view.owned = false;
        SG_HIP_TRY(hipMemsetAsync(words, 0, 8 * sizeof(uint32_t), ctx->stream));
        SG_HIP_TRY(hipMemsetAsync(scratch->d_counts, 0, sizeof(int32_t) * (size_t)block, ctx->stream));
        SG_TRY(sg_spgemm_pruned_launch(ctx, &view, Bt, stride < SG_TOPN_LANES ? stride : SG_TOPN_LANES, scratch.get(), threshold,
                                       delta, words, words + 1, words + 8, d_stats));
    }
    hipLaunchKernelGGL(count_macs_kernel, dim3(512), dim3(256), 0, ctx->stream, A->d_indptr, A->d_indices, A->n_rows,
                       (const uint32_t *)Bt->d_term_len, d_stats + 3);
    SG_HIP_TRY(hipGetLastError());
    unsigned long long h[4] = {0, 0, 0, 0};
    SG_TRY(sg_fetch(ctx, h, d_stats, sizeof(h)));
    *prices = sg_plan_pilot_prices(h, a, b, selfjoin);
    ctx->pilot_ms_pruned = prices->ms_pruned;
    ctx->pilot_ms_exact = prices->ms_exact;
    return SG_OK;
}

// Is A the matrix this index was built from -- a self-join?  (An index over groups of identical rows: the caller's matrix,
// not the representatives'.)
static bool built_from(const sg_csr *A, const sg_postings *Bt) {
    if (Bt->collapse) {
        const sg_csr *cb = &Bt->caller_b_copy;
        return A->n_rows == Bt->collapse->n_orig && A->d_indptr == cb->d_indptr && A->d_indices == cb->d_indices &&
               A->d_data == cb->d_data;
    }
    return A->n_rows == Bt->n_right && A->d_indptr == Bt->b_indptr && A->d_indices == Bt->b_indices && A->d_data == Bt->b_data;
}

// The object that owns what is built on demand: a view is a copy on the caller's stack
static const sg_postings *owner(const sg_postings *Bt) { return Bt->view_of ? Bt->view_of : Bt; }

// The indexes kept with an index (sg_postings::plain, alt_tile, exact_native), built from `from` on first use and owned by
// `home` (view_of resolved).  Two threads sharing the index must not both build one; no build nests inside
// another, so one lock serves the three.  (The matrix has to be alive as long as the index is: include/sg_hip.h,
// sg_postings_build.)
enum class SgCompanion { plain, alt_tile, exact_native };
static std::mutex g_companion_mu;

static int companion(sg_ctx *ctx, const sg_postings *home, SgCompanion kind, const sg_csr *from, const sg_postings **out) {
    sg_postings **slot = kind == SgCompanion::plain      ? &home->plain
                         : kind == SgCompanion::alt_tile ? &home->alt_tile
                                                         : &home->exact_native;
    std::lock_guard<std::mutex> lock(g_companion_mu);
    if (!*slot) {
        if (kind == SgCompanion::plain) {   // every row, on the caller's own tile and flags
            SG_TRY(sg_postings_build_flags(ctx, from, home->build_tile_cols, (home->build_flags & 0xff) | SG_POSTINGS_NO_COLLAPSE, slot));
        } else {                            // the form's own tile and layout, from rows that may still be pending
            SG_TRY(sg_csr_ensure_rows(ctx, from));
            SG_TRY(sg_postings_build_flags(ctx, from, 0,
                                           (home->build_flags & SG_POSTINGS_NO_PERMUTATION) | SG_POSTINGS_NO_COLLAPSE |
                                               (kind == SgCompanion::alt_tile ? SG_POSTINGS_TILE_FORM : SG_POSTINGS_EXACT_ONLY),
                                           slot));
        }
    }
    *out = *slot;
    return SG_OK;
}

// The matrix a companion of Bt is built from: A itself in a self-join, otherwise the matrix the caller's index was built from
// (of an index over groups, whose view Bt is, the representatives' one); null: not known
static const sg_csr *companion_source(const sg_csr *A, const sg_postings *Bt) {
    if (built_from(A, Bt)) return A;
    const sg_postings *home = owner(Bt);
    return home->collapse ? home->collapse->unique : (Bt->built_from_valid ? &Bt->built_from : nullptr);
}

// ---- Which form runs.  The rule is sg_plan.h's; here are its inputs -- the switches, the two
//      matrices as the numbers the rule reads -- and plan_multiply, which asks its questions in order and does the device
//      work each answer calls for.
static SgPlanSwitches multiply_switches(const sg_ctx *ctx) {   // unset or empty: the default
    SgPlanSwitches sw;
    const char *v = ctx->opt("SG_SYM");
    sw.sym = v ? v[0] : 0;
    sw.prune = !ctx->opt_is("SG_PRUNE", '0');
    sw.alt_form = ctx->opt_int("SG_ALT_FORM", sw.alt_form);
    sw.alt_form_below = ctx->opt_double("SG_ALT_FORM_BELOW", sw.alt_form_below);
    sw.prune_max_mean_row = ctx->opt_double("SG_PRUNE_MAX_MEAN_ROW", sw.prune_max_mean_row);
    sw.sym_min_rows = ctx->opt_int("SG_SYM_MIN_ROWS", sw.sym_min_rows);
    sw.exact_sym_min_rows = ctx->opt_int("SG_EXACT_SYM_MIN_ROWS", sw.exact_sym_min_rows);
    sw.exact_sym = ctx->opt_int("SG_EXACT_SYM", sw.exact_sym);
    sw.prune_pilot = ctx->opt_int("SG_PRUNE_PILOT", sw.prune_pilot);
    sw.exact_native = ctx->opt_int("SG_EXACT_NATIVE", sw.exact_native);
    sw.tile_group = ctx->opt_int("SG_TILE_GROUP", sw.tile_group);
    if ((v = ctx->opt("SG_PRUNE_MIN_THRESHOLD")) && *v) sw.prune_min_threshold = {true, atof(v)};
    if ((v = ctx->opt("SG_PRUNE_DELTA")) && *v) sw.prune_delta = {true, atof(v)};
    if ((v = ctx->opt("SG_WAVES_PER_CU")) && *v) sw.waves_per_cu = {true, atoi(v)};
    return sw;
}

static void describe(const sg_csr *A, const sg_postings *Bt, SgPlanLeft *a, SgPlanIndex *b) {
    a->n_rows = A->n_rows;
    a->nnz = A->nnz;
    a->f64 = A->dtype == SG_F64;
    a->is_index_source = built_from(A, Bt);
    b->cosine_like = Bt->cosine_like;
    b->has_filter = Bt->d_filt != nullptr;
    b->tile_form = Bt->tile_form;
    b->pruned_tile = sg_pruned_supports_tile(Bt->tile_log2);
    b->fold_log2 = Bt->fold_log2;
    b->tile_log2 = Bt->tile_log2;
    b->n_tiles = Bt->n_tiles;
    b->n_right = Bt->n_right;
    b->nnz = Bt->nnz;
    b->n_terms = Bt->n_terms;
    const sg_csr *from = companion_source(A, Bt);
    b->source_rows = from ? from->n_rows : -1;
}

static int plan_multiply(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int32_t top_n, double threshold, bool row_range,
                         SgPlan *plan) {
    *plan = SgPlan();
    const SgPlanSwitches sw = multiply_switches(ctx);
    SgPlanCall call;
    call.threshold = plan->threshold = sg_plan_clamp_threshold(threshold);
    call.row_range = row_range;
    plan->index = Bt;
    if (!result_stride(A->n_rows, top_n, Bt->n_right, &plan->stride))   // (row_range: not applicable, the caller's other path reports it)
        return row_range ? SG_OK : result_overflow(A->n_rows, plan->stride, "; split the left matrix");
    call.stride = plan->stride;
    SgPlanLeft a;
    SgPlanIndex b;
    describe(A, Bt, &a, &b);

    // 1. the tile-by-tile form's index takes the caller's place BEFORE the envelope is judged: the threshold bar and the
    //    delta are those of the index that will run
    if (sg_plan_wants_tile_form(a, b, call, sw) && sg_plan_source_fits(b)) {
        SG_TRY(companion(ctx, owner(Bt), SgCompanion::alt_tile, companion_source(A, Bt), &Bt));
        describe(A, Bt, &a, &b);
    }

    // 2. inside the pruned kernel's envelope?  Then its delta, and what A is
    bool a_cosine_like = false;
    if (sg_plan_needs_props(a, b, call, sw)) {
        plan->delta = sg_plan_delta(a, b, call, sw);
        float a_n2 = 0.f;
        SG_TRY(sg_csr_props(ctx, A, &a_cosine_like, &a_n2, nullptr));     // (the longest row is not asked for: it alone needs a look)
    }

    // 3. the form
    plan->form = sg_plan_form(a, b, call, sw, a_cosine_like);

    // 4. ... which a pilot may call off
    if (sg_plan_pilot_due(a, b, call, sw, plan->form)) {
        SgPilotPrices prices;
        SG_TRY(sg_csr_ensure_rows(ctx, A));     // (the pilot runs the one-sided kernel over blocks of A's rows)
        SG_TRY(prune_pilot(ctx, A, Bt, a, b, plan->stride, plan->threshold, plan->delta, plan->form == SgPlan::PRUNED_SELFJOIN, &prices));
        plan->form = sg_plan_after_pilot(plan->form, prices, sw);
    }

    // 5. the exact kernel's own layout of the index (as it stands after 1.)
    const SgOwnIndex own = sg_plan_exact_own_index(a, b, call, sw, plan->form);
    if (own != SgOwnIndex::none) {
        SG_TRY(companion(ctx, owner(Bt), SgCompanion::exact_native, own == SgOwnIndex::from_left ? A : companion_source(A, Bt), &Bt));
        describe(A, Bt, &a, &b);
    }

    plan->index = Bt;
    plan->launch = sg_plan_launch_shape(a, b, plan->stride, ctx->num_cu, ctx->lds_per_cu, sw);
    return SG_OK;
}

// What every product begins with: the driver's counters, the result's counts and the statistics words cleared by one
// launch; then, for a plan in a self-join form, its pass (over the row range given).  *done: the pass took the product.
static int zero_then_selfjoin_pass(sg_ctx *ctx, const sg_csr *A, const SgPlan &plan, sg_topn *r, uint32_t *counters, size_t n_counters,
                                   size_t n_stat_words, bool *done, int64_t row_lo = 0, int64_t row_hi = -1,
                                   int32_t **d_pairs = nullptr, int64_t *n_pairs = nullptr, int64_t row_step = 1) {
    *done = false;
    SG_TRY(SG_ZERO3(ctx, counters, sizeof(uint32_t) * n_counters, r->d_counts, sizeof(int32_t) * (size_t)A->n_rows,
                    ctx->d_stat_words, n_stat_words * sizeof(int64_t)));
    int st = SG_OK;
    if (sg_plan_selfjoin(plan.form))
        st = sg_spgemm_pruned_symmetric(ctx, A, plan.index, plan.stride, r, plan.threshold, plan.delta,
                                        (unsigned long long *)(ctx->d_stat_words + 2), done, row_lo, row_hi, d_pairs, n_pairs, row_step,
                                        plan.form == SgPlan::EXACT_SELFJOIN);
    ctx->prune_symmetric = *done;
    return st;
}

// The pruned kernel, one-sided, over every row; with a top_n of 65 .. 128 the rows whose list came out full join those it
// handed over
static int pruned_launches(sg_ctx *ctx, const sg_csr *A, const SgPlan &plan, sg_topn *r, uint32_t *row_counter, uint32_t *handed_count,
                           uint32_t *handed_rows) {
    SgTimer kt(ctx, SG_K_SPGEMM_KERNEL);
    SG_TRY(sg_spgemm_pruned_launch(ctx, A, plan.index, plan.stride < SG_TOPN_LANES ? plan.stride : SG_TOPN_LANES, r, plan.threshold,
                                   plan.delta, row_counter, handed_count, handed_rows, (unsigned long long *)(ctx->d_stat_words + 2)));
    if (plan.stride > SG_TOPN_LANES && A->n_rows > 0) {
        hipLaunchKernelGGL(rows_with_full_lists_kernel, dim3((unsigned)((A->n_rows + 255) / 256)), dim3(256), 0, ctx->stream,
                           (const int32_t *)r->d_counts, A->n_rows, (int32_t)SG_TOPN_LANES, handed_count, handed_rows);
        SG_HIP_TRY(hipGetLastError());
    }
    return SG_OK;
}

// Did the pruned kernel hand rows over?  Asked (four bytes read back) only where the answer saves work: the index build
// leaves the exact kernel's postings out when the pruned multiply is expected to take everything
// (sg_postings_ensure_full writes them on demand).  Where they exist the exact kernel's launch over the handed rows goes
// out on the device-side count, as before the postings became lazy -- blocked and zipped multiplies enqueue without a
// host round trip per part.
static int rows_handed_over(sg_ctx *ctx, const sg_postings *Bt, const uint32_t *handed_count, bool *any) {
    *any = true;
    if (Bt->d_vals != nullptr || Bt->nnz <= 0) return SG_OK;
    uint32_t *h_handed = (uint32_t *)(ctx->h_stat_words + 7);   // pinned
    *h_handed = 0;
    SG_TRY(sg_fetch(ctx, h_handed, handed_count, 4));
    *any = *h_handed > 0;
    return SG_OK;
}

// The exact kernel: a pass per register list of result columns, a launch per tile group; over every row, or over a
// device-side list of rows
static int exact_passes(sg_ctx *ctx, const sg_csr *A, const SgPlan &plan, sg_topn *r, uint32_t *counters, const uint32_t *row_list,
                        const uint32_t *row_list_len) {
    const sg_postings *Bt = plan.index;
    const SgLaunchShape &sh = plan.launch;
    if (A->n_rows <= 0) return SG_OK;
    for (int pass = 0, li = 0; pass < sh.n_pass; ++pass) {
        const int pass_off = pass * SG_TOPN_LANES;
        const int keep = plan.stride - pass_off < SG_TOPN_LANES ? plan.stride - pass_off : SG_TOPN_LANES;
        for (int g = 0; g < sh.n_groups; ++g, ++li) {
            const int tb = g * sh.group;
            const int te = tb + sh.group < Bt->n_tiles ? tb + sh.group : Bt->n_tiles;
            SG_TRY(by_dtype(A->dtype, [&](auto tag) {
                using T = decltype(tag);
                return dispatch_spgemm<T>(ctx, A, Bt, tb, te, keep, pass_off, r, (T)plan.threshold, counters + li, sh.grid, row_list, row_list_len);
            }));
        }
    }
    return SG_OK;
}

// The launches of a plan: the self-join form's pass, the pruned kernel, and the exact kernel -- the whole product, the rows
// the pruned kernel handed over, or what a self-join pass that was called off left
static int run_plan(sg_ctx *ctx, const sg_csr *A, const SgPlan &plan, sg_topn *r) {
    const sg_postings *Bt = plan.index;
    const bool prune = sg_plan_pruned(plan.form);
    // counters: [0, n_launch) row counters of the exact launches; then the pruned kernel's row counter, the
    // number of rows it handed over, and their list
    const size_t n_launch = (size_t)plan.launch.n_launch(), n_words = n_launch + 4;
    Scratch tmp(ctx);
    uint32_t *counters = nullptr;
    SG_TRY(tmp.alloc(n_words + (prune ? (size_t)A->n_rows : 0), &counters));
    uint32_t *handed_count = counters + n_launch + 2;
    uint32_t *handed_rows = counters + n_words;

    SgTimer timer(ctx, SG_K_SPGEMM);
    bool selfjoin_done = false;
    SG_TRY(zero_then_selfjoin_pass(ctx, A, plan, r, counters, n_words, 7, &selfjoin_done));   // (stat words [0], [1]: written by the counting kernels at the end)
    if (selfjoin_done) return SG_OK;
    // everything below reads the rows of A itself (the self-join form read the index's copy in position order): the
    // representatives' matrix of an index over groups is written now if it is still pending
    SG_TRY(sg_csr_ensure_rows(ctx, A));
    if (!prune) {   // the exact kernel's launches are the whole product
        SG_TRY(sg_postings_ensure_full(ctx, Bt));
        SgTimer kt(ctx, SG_K_SPGEMM_KERNEL);
        return exact_passes(ctx, A, plan, r, counters, nullptr, handed_count);
    }
    SG_TRY(pruned_launches(ctx, A, plan, r, counters + n_launch + 1, handed_count, handed_rows));
    bool any_handed = false;
    SG_TRY(rows_handed_over(ctx, Bt, handed_count, &any_handed));
    if (any_handed) {
        SG_TRY(sg_postings_ensure_full(ctx, Bt));
        SG_TRY(exact_passes(ctx, A, plan, r, counters, handed_rows, handed_count));
    }
    SG_HIP_TRY(hipMemcpyAsync(ctx->d_stat_words + 5, handed_count, 4, hipMemcpyDeviceToDevice, ctx->stream));   // (the self-join form has left its own count there)
    return SG_OK;
}

struct InnerMultiply {   // while it lives, sg_spgemm_topn runs for a wrapper that counts the kept entries itself
    sg_ctx *ctx;
    explicit InnerMultiply(sg_ctx *c) : ctx(c) { ++ctx->inner_multiply_depth; }
    ~InnerMultiply() { --ctx->inner_multiply_depth; }
};

// The index was built over one representative per group of identical right-hand rows (sg_collapse.hip): multiply on the
// groups, expand to the caller's columns (and, in a self-join, to the caller's rows).
static int spgemm_topn_collapsed(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int32_t top_n, double threshold,
                                 int32_t sort, sg_topn **out) {
    const SgCollapse *c = Bt->collapse;
    int64_t stride64 = top_n;
    if (stride64 > c->n_orig) stride64 = c->n_orig > 0 ? c->n_orig : 1;
    if (stride64 > 2 * SG_TOPN_LANES) {
        // more columns per row than the multiply on the groups keeps (two register lists since round 6; one before, and
        // top_n of 65 .. 128 then multiplied every row: 663 k names, top 100: 9.1 ms): an index over all rows, built once
        // from the caller's matrix, serves these calls
        const sg_postings *plain = nullptr;
        SG_TRY(companion(ctx, Bt, SgCompanion::plain, &Bt->caller_b_copy, &plain));
        return sg_spgemm_topn(ctx, A, plain, top_n, threshold, sort, out);
    }
    const bool self = built_from(A, Bt);
    sg_postings view = *Bt;          // shallow: the same index, seen without the groups
    view.collapse = nullptr;
    view.plain = nullptr;
    view.view_of = Bt;
    sg_topn *groups = nullptr;
    {
        const InnerMultiply inner(ctx);
        SG_TRY(sg_spgemm_topn(ctx, self ? c->unique : A, &view, top_n, threshold, 1, &groups));
    }
    const TopnPtr ru(groups);
    TopnPtr r;
    SG_TRY(topn_alloc(ctx, A->n_rows, c->n_orig, (int32_t)stride64, A->dtype, &r));
    {
        SgTimer timer(ctx, SG_K_ZIP);    // the expansion is a merge by column, like the zip of column blocks
        SG_TRY(sg_collapse_expand(ctx, c, ru.get(), self, r.get()));   // (clears r's counts itself)
        if (!sort) SG_TRY(sort_rows_by_column(ctx, r.get()));
        if (A->n_rows > 0 && ctx->inner_multiply_depth == 0) {   // entries kept, counted on the expanded result
            // (word [1] is still zero: the multiply on the groups cleared it and, being an inner one, did not count)
            hipLaunchKernelGGL(sum_counts_kernel, dim3(256), dim3(256), 0, ctx->stream, r->d_counts, A->n_rows,
                               (unsigned long long *)(ctx->d_stat_words + 1));
            if (hipGetLastError() != hipSuccess) return SG_ERR_HIP;
        }
    }
    *out = r.release();
    return SG_OK;
}

// out row r = row gid[r] of the result over the groups of identical LEFT rows: a thread per cell
template <typename T>
__global__ void __launch_bounds__(256) expand_left_rows_kernel(const int32_t *__restrict__ u_cols, const T *__restrict__ u_vals,
                                                               const int32_t *__restrict__ u_cnt, const uint32_t *__restrict__ gid,
                                                               int64_t n_rows, int32_t stride, int32_t *__restrict__ cols,
                                                               T *__restrict__ vals, int32_t *__restrict__ cnt) {
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= n_rows * stride) return;
    const int64_t r = cell / stride;
    const int32_t e = (int32_t)(cell - r * stride);
    const int64_t g = gid[r];
    const int32_t m = u_cnt[g];
    if (e == 0) cnt[r] = m;
    if (e < m) {
        cols[cell] = u_cols[g * stride + e];
        vals[cell] = u_vals[g * stride + e];
    }
}

// Identical LEFT rows of a one-sided product (round 4).  A master list of ten million names repeats a fifth of them
// (BASELINE.json configs[4], master x duplicates): identical strings are identical rows of A, and identical rows of A
// have identical rows in C -- sparse_dot_topn (string_grouper.py:737-743) and rounds 1-3 multiplied every one of them.
// The rows of A are grouped like the right-hand side's (sg_collapse.hip: hash, sort, entry-by-entry check), the
// representatives are multiplied, and every row receives a copy of its group's result row.  The groups stay with A: a
// product against the next column block of the right-hand side does not group again.
static int spgemm_topn_left_groups(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int32_t top_n, double threshold, int32_t sort,
                                   sg_topn **out, bool *done) {
    *done = false;
    if (A->left_state == 1) return SG_OK;
    if (A->left_state == 0) {
        SgCollapse *g = nullptr;
        bool cl = false;
        float n2 = 0.f;
        SG_TRY(sg_csr_props(ctx, A, &cl, &n2));     // (the grouping hashes value bits: any matrix will do, but only name
        if (cl) SG_TRY(sg_collapse_build(ctx, A, &g, /*left_side=*/true));   //  lists -- cosine-like rows -- repeat themselves)
        A->left_groups = g;
        A->left_state = g ? 2 : 1;
        if (!g) return SG_OK;
    }
    const SgCollapse *g = A->left_groups;
    sg_topn *groups = nullptr;
    g->unique->left_state = 1;                      // (representatives are distinct)
    {
        const InnerMultiply inner(ctx);
        SG_TRY(sg_spgemm_topn(ctx, g->unique, Bt, top_n, threshold, sort, &groups));
    }
    const TopnPtr ru(groups);
    TopnPtr r;
    SG_TRY(topn_alloc(ctx, A->n_rows, ru->n_cols, ru->stride, ru->dtype, &r));
    if (A->n_rows > 0) {
        SgTimer timer(ctx, SG_K_ZIP);
        const int64_t cells = A->n_rows * (int64_t)ru->stride;
        const unsigned grid = (unsigned)((cells + 255) / 256);
        by_dtype(ru->dtype, [&](auto tag) {
            using T = decltype(tag);
            hipLaunchKernelGGL(expand_left_rows_kernel<T>, dim3(grid), dim3(256), 0, ctx->stream, (const int32_t *)ru->d_cols,
                               (const T *)ru->d_vals, (const int32_t *)ru->d_counts, (const uint32_t *)g->d_gid, A->n_rows,
                               ru->stride, r->d_cols, (T *)r->d_vals, r->d_counts);
            return SG_OK;
        });
        // entries kept: counted on all rows (word [1] is still zero: the inner multiplies clear it and do not count)
        hipLaunchKernelGGL(sum_counts_kernel, dim3(256), dim3(256), 0, ctx->stream, r->d_counts, A->n_rows,
                           (unsigned long long *)(ctx->d_stat_words + 1));
        if (hipGetLastError() != hipSuccess) return SG_ERR_HIP;
    }
    *out = r.release();
    *done = true;
    return SG_OK;
}

// Is this a product for the grouping of identical LEFT rows?  A one-sided one (A is not the matrix the index was built
// from: a self-join groups its rows with the index), with the switches on, whose result the 32-bit result index holds
static int left_groups_apply(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int32_t top_n, bool *apply) {
    *apply = false;
    const bool off = ctx->opt_is("SG_COLLAPSE", '0') || ctx->opt_is("SG_COLLAPSE_LEFT", '0');   // (asked on every call: groups
    if (off && A->left_groups) {   // ... and are given back when it is turned off                //  kept with A do not outlive the switch)
        sg_collapse_free(A->left_groups);
        A->left_groups = nullptr;
        A->left_state = 0;
    }
    if (built_from(A, Bt) || off || A->left_state == 1 || A->n_cols != Bt->n_terms || A->dtype != Bt->dtype || top_n < 1) return SG_OK;
    // (the result is one row per row of A whatever the number of groups: the 32-bit result index must hold it)
    int32_t stride = 0;
    if (!result_stride(A->n_rows, top_n, Bt->collapse ? Bt->collapse->n_orig : Bt->n_right, &stride))
        return result_overflow(A->n_rows, stride, "; split the left matrix");
    *apply = true;
    return SG_OK;
}

extern "C" int sg_spgemm_topn(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int32_t top_n, double threshold,
                              int32_t sort, sg_topn **out) {
    SG_REQUIRE(ctx && A && Bt && out, "null argument");
    bool group_left = false;
    SG_TRY(left_groups_apply(ctx, A, Bt, top_n, &group_left));
    if (group_left) {
        bool done = false;
        SG_TRY(spgemm_topn_left_groups(ctx, A, Bt, top_n, threshold, sort, out, &done));
        if (done) return SG_OK;
    }
    if (Bt->collapse) {
        SG_REQUIRE(A->n_cols == Bt->n_terms && A->dtype == Bt->dtype && top_n >= 1, "A and B differ in columns or value type, or top_n < 1");
        return spgemm_topn_collapsed(ctx, A, Bt, top_n, threshold, sort, out);
    }
    SG_REQUIRE(A->n_cols == Bt->n_terms, "A and B have different numbers of columns (vocabulary size)");
    SG_REQUIRE(A->dtype == Bt->dtype, "A and B have different value types");
    SG_REQUIRE(top_n >= 1, "top_n must be >= 1");
    SgPlan plan;
    SG_TRY(plan_multiply(ctx, A, Bt, top_n, threshold, /*row_range=*/false, &plan));
    Bt = plan.index;
    TopnPtr r;
    SG_TRY(topn_alloc(ctx, A->n_rows, Bt->n_right, plan.stride, A->dtype, &r));
    SG_TRY(run_plan(ctx, A, plan, r.get()));
    if (!sort) SG_TRY(sort_rows_by_column(ctx, r.get()));
    // measurement words: MACs and kept entries of this multiply
    if (A->nnz > 0 && built_from(A, Bt))      // (10 M gathers less per multiply: 54 -> 3 us at 663 k)
        hipLaunchKernelGGL(count_macs_selfjoin_kernel, dim3(64), dim3(256), 0, ctx->stream, (const uint32_t *)Bt->d_term_len,
                           Bt->n_terms, (unsigned long long *)ctx->d_stat_words);
    else if (A->nnz > 0)
        hipLaunchKernelGGL(count_macs_kernel, dim3(512), dim3(256), 0, ctx->stream, A->d_indptr, A->d_indices,
                           A->n_rows, (const uint32_t *)Bt->d_term_len, (unsigned long long *)ctx->d_stat_words);
    if (A->n_rows > 0 && ctx->inner_multiply_depth == 0)   // (an inner multiply's rows are not the caller's: its wrapper counts)
        hipLaunchKernelGGL(sum_counts_kernel, dim3(256), dim3(256), 0, ctx->stream, r->d_counts, A->n_rows,
                           (unsigned long long *)(ctx->d_stat_words + 1));
    record_bytes(ctx, A, Bt, plan.threshold);
    if (hipGetLastError() != hipSuccess) return SG_ERR_HIP;
    *out = r.release();
    return SG_OK;
}

// ---- multi-GPU self-join: the self-join form split over ranks by left-row ranges
extern "C" int sg_selfjoin_range(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int32_t top_n, double threshold,
                                 int64_t row_lo, int64_t row_hi, sg_topn **out, int32_t **d_pairs, int64_t *n_pairs,
                                 int32_t *pair_words, int32_t *applicable, int64_t row_step) {
    if (row_step < 1) row_step = 1;
    SG_REQUIRE(ctx && A && Bt && out && d_pairs && n_pairs && pair_words && applicable, "null argument");
    SG_REQUIRE(A->n_cols == Bt->n_terms && A->dtype == Bt->dtype, "A and B differ in columns or value type");
    SG_REQUIRE(top_n >= 1, "top_n must be >= 1");
    SG_REQUIRE(row_lo >= 0 && row_lo <= row_hi && row_hi <= A->n_rows, "row range outside the matrix");
    *out = nullptr;
    *d_pairs = nullptr;
    *n_pairs = 0;
    *pair_words = A->dtype == SG_F64 ? 4 : 3;
    *applicable = 0;
    if (Bt->collapse) {
        // an index over groups of identical rows: the ranges are ranges of the GROUPS' positions (sg_postings_rows), the
        // result has one row per group; sg_topn_expand_groups turns the gathered result into the caller's rows
        const SgCollapse *c = Bt->collapse;
        if (!built_from(A, Bt)) return SG_OK;                 // not the matrix the index was built from: the row-block form
        if (row_hi > c->n_u) {
            sg_set_error("row range [%lld, %lld) outside the %lld groups of the index (sg_postings_rows)", (long long)row_lo,
                         (long long)row_hi, (long long)c->n_u);
            return SG_ERR_BADARG;
        }
        sg_postings view = *Bt;           // shallow: the same index, seen without the groups
        view.collapse = nullptr;
        view.plain = nullptr;
        const int st_u = sg_selfjoin_range(ctx, c->unique, &view, top_n, threshold, row_lo, row_hi, out, d_pairs, n_pairs, pair_words,
                                           applicable, row_step);
        if (st_u == SG_OK && *out) (*out)->top_n_asked = top_n;      // (fewer groups than top_n: the rows over MEMBERS are wider)
        return st_u;
    }
    SgPlan plan;
    SG_TRY(plan_multiply(ctx, A, Bt, top_n, threshold, /*row_range=*/true, &plan));
    if (plan.form != SgPlan::PRUNED_SELFJOIN) return SG_OK;
    TopnPtr r;
    SG_TRY(topn_alloc(ctx, A->n_rows, Bt->n_right, plan.stride, A->dtype, &r));
    int st = SG_OK;
    bool done = false;
    {
        SgTimer timer(ctx, SG_K_SPGEMM);
        st = zero_then_selfjoin_pass(ctx, A, plan, r.get(), nullptr, 0, 8, &done, row_lo, row_hi, d_pairs, n_pairs, row_step);
    }
    record_bytes(ctx, A, Bt, plan.threshold);
    if (st != SG_OK || !done) return st;   // a row for the exact kernel, or the pair list was full: the one-sided form is the caller's
    *out = r.release();
    *applicable = 1;
    return SG_OK;
}

extern "C" int sg_selfjoin_merge(sg_ctx *ctx, sg_topn *res, const sg_postings *Bt, const int32_t *d_pairs, int64_t n_pairs,
                                 int32_t pair_words, int64_t row_lo, int64_t row_hi, int64_t row_step) {
    SG_REQUIRE(ctx && res, "null argument");
    SG_REQUIRE(n_pairs == 0 || d_pairs != nullptr, "pairs are null");
    SG_REQUIRE(pair_words == (res->dtype == SG_F64 ? 4 : 3), "pair records do not match the result's value type");
    SG_REQUIRE(row_lo >= 0 && row_lo <= row_hi && row_hi <= res->n_rows, "row range outside the result");
    // (pairs_select_kernel keeps a row of more than 64 candidates in two register lists and reads its bar from lane
    //  stride - 65 of the second: beyond 128 that is no lane, and no more than 128 entries could stay)
    SG_REQUIRE(res->stride <= 2 * SG_TOPN_LANES, "the merge selects rows of at most 128 columns: the result's stride is larger");
    SgTimer timer(ctx, SG_K_ZIP);
    return sg_selfjoin_merge_pairs(ctx, res, d_pairs, n_pairs, row_lo, row_hi, Bt ? (const uint32_t *)Bt->d_pos_of : nullptr, row_step);
}

extern "C" int sg_postings_bytes(const sg_postings *Bt, int64_t *pruned_multiply_bytes) {
    SG_REQUIRE(Bt && pruned_multiply_bytes, "null argument");
    int64_t b = 0;
    if (Bt->d_filt) {
        const int64_t es = Bt->dtype == SG_F64 ? 16 : 8;
        b += 4 * (Bt->nnz + 512);                                                        // filter postings
        b += 4 * (Bt->n_terms + 1) * (int64_t)(Bt->fold_log2 > 0 ? Bt->nv_pad : Bt->nt_pad);   // the segment ends the loop reads
        if (Bt->d_fwd) b += es * (Bt->nnz + 8);                                          // packed rows
        if (Bt->d_fwd_ptr) b += 8 * (Bt->n_right + 2);
        if (Bt->d_blk) b += (int64_t)Bt->blk_bytes * (Bt->n_right + 1);
        // 8-bit copies: what is WRITTEN and READ of the records -- the header and the 16-byte units a row's entries reach
        // (a record is allocated at SG_Q8_STRIDE bytes; rounds 5 counted that, which made a working set that fits the
        // 256 MiB Infinity Cache look as if it did not: VERDICT r05, weak 4)
        if (Bt->d_q8) b += 16 * (Bt->n_right + 1) + 4 * Bt->nnz + 8 * Bt->n_right;
    }
    *pruned_multiply_bytes = b;
    return SG_OK;
}

extern "C" int sg_postings_rows(const sg_postings *Bt, int64_t *n_index_rows, int64_t *n_caller_rows,
                                const uint32_t **d_group_of_row) {
    SG_REQUIRE(Bt != nullptr, "postings are null");
    if (n_index_rows) *n_index_rows = Bt->n_right;
    if (n_caller_rows) *n_caller_rows = Bt->collapse ? Bt->collapse->n_orig : Bt->n_right;
    if (d_group_of_row) *d_group_of_row = Bt->collapse ? Bt->collapse->d_gid : nullptr;
    return SG_OK;
}

extern "C" int sg_topn_expand_groups(sg_ctx *ctx, const sg_postings *Bt, const sg_topn *groups, const int32_t *d_rows,
                                     int64_t n_rows, sg_topn **out) {
    SG_REQUIRE(ctx && Bt && groups && out, "null argument");
    SG_REQUIRE(Bt->collapse != nullptr, "the index was not built over groups of identical rows (sg_postings_rows)");
    const SgCollapse *c = Bt->collapse;
    SG_REQUIRE(groups->n_rows == c->n_u, "the result does not have one row per group of the index");
    SG_REQUIRE(groups->dtype == Bt->dtype, "result and index differ in value type");
    if (!d_rows) n_rows = c->n_orig;
    SG_REQUIRE(n_rows >= 0 && n_rows <= c->n_orig, "more rows than the matrix has");
    // a row over members holds up to min(top_n, rows) columns -- as spgemm_topn_collapsed sizes it --, not the groups' stride,
    // which is cut at the number of GROUPS (eight distinct names in 200 k rows, top_n 20: 20 columns per row, not 8)
    int32_t stride = 0;
    if (!result_stride(n_rows, groups->top_n_asked > groups->stride ? groups->top_n_asked : groups->stride, c->n_orig, &stride))
        return result_overflow(n_rows, stride, "");
    TopnPtr r;
    SG_TRY(topn_alloc(ctx, n_rows, c->n_orig, stride, groups->dtype, &r));
    {
        SgTimer timer(ctx, SG_K_ZIP);
        SG_TRY(sg_collapse_expand(ctx, c, groups, true, r.get(), d_rows));   // (clears r's counts itself)
    }
    *out = r.release();
    return SG_OK;
}

// rows whose group sits at a position of [pos_lo, pos_hi)
__global__ void __launch_bounds__(256) rows_of_range_flag_kernel(const uint32_t *__restrict__ gid, const uint32_t *__restrict__ pos_of,
                                                                 int64_t n_rows, uint32_t pos_lo, uint32_t pos_hi, uint32_t step,
                                                                 uint32_t *__restrict__ flag) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const uint32_t g = gid[r];
    const uint32_t p = pos_of ? pos_of[g] : g;
    flag[r] = (p >= pos_lo && p < pos_hi && (pos_hi - 1u - p) % step == 0u) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) rows_of_range_fill_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ at,
                                                                 int64_t n_rows, int32_t *__restrict__ rows) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rows && flag[r]) rows[at[r]] = (int32_t)r;
}

extern "C" int sg_topn_expand_range(sg_ctx *ctx, const sg_postings *Bt, const sg_topn *groups, int64_t pos_lo, int64_t pos_hi,
                                    sg_topn **out, int32_t **d_rows, int64_t *n_rows, int64_t pos_step) {
    if (pos_step < 1) pos_step = 1;
    SG_REQUIRE(ctx && Bt && groups && out && d_rows && n_rows, "null argument");
    SG_REQUIRE(Bt->collapse != nullptr, "the index was not built over groups of identical rows (sg_postings_rows)");
    const SgCollapse *c = Bt->collapse;
    SG_REQUIRE(pos_lo >= 0 && pos_lo <= pos_hi && pos_hi <= c->n_u, "range outside the groups of the index");
    *out = nullptr;
    *d_rows = nullptr;
    *n_rows = 0;
    const int64_t n = c->n_orig;
    Scratch mine(ctx);   // the rows' numbers: the caller's once the result exists
    int32_t *rows = nullptr;
    uint32_t n_mine = 0;
    {
        Scratch scratch(ctx);
        uint32_t *flag = nullptr, *at = nullptr, *total = nullptr;
        SG_TRY(scratch.alloc((size_t)n + 1, &flag));
        SG_TRY(scratch.alloc((size_t)n + 1, &at));
        SG_TRY(scratch.alloc((size_t)4, &total));
        if (n > 0) {
            const unsigned g1 = (unsigned)((n + 255) / 256);
            hipLaunchKernelGGL(rows_of_range_flag_kernel, dim3(g1), dim3(256), 0, ctx->stream, (const uint32_t *)c->d_gid,
                               (const uint32_t *)Bt->d_pos_of, n, (uint32_t)pos_lo, (uint32_t)pos_hi, (uint32_t)pos_step, flag);
            SG_TRY(sg_exclusive_scan_u32(ctx, flag, at, n, total));
            SG_HIP_TRY(hipMemcpyAsync(&n_mine, total, 4, hipMemcpyDeviceToHost, ctx->stream));
            SG_HIP_TRY(hipStreamSynchronize(ctx->stream));
            SG_TRY(mine.alloc((size_t)n_mine + 1, &rows));
            hipLaunchKernelGGL(rows_of_range_fill_kernel, dim3(g1), dim3(256), 0, ctx->stream, (const uint32_t *)flag,
                               (const uint32_t *)at, n, rows);
            SG_HIP_TRY(hipGetLastError());
        }
    }
    SG_TRY(sg_topn_expand_groups(ctx, Bt, groups, rows, (int64_t)n_mine, out));
    *d_rows = mine.keep(rows);
    *n_rows = (int64_t)n_mine;
    return SG_OK;
}

extern "C" int sg_postings_permutation(const sg_postings *Bt, const uint32_t **d_orig_of, const uint32_t **d_pos_of) {
    SG_REQUIRE(Bt != nullptr, "postings are null");
    if (d_orig_of) *d_orig_of = Bt->d_orig_of;
    if (d_pos_of) *d_pos_of = Bt->d_pos_of;
    return SG_OK;
}

extern "C" int sg_device_free(sg_ctx *ctx, void *d_ptr) {
    SG_REQUIRE(ctx != nullptr, "null argument");
    ctx->release(d_ptr);
    return SG_OK;
}

extern "C" int sg_row_costs(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int64_t *out_cost) {
    SG_REQUIRE(ctx && A && Bt && out_cost, "null argument");
    SG_REQUIRE(A->n_cols == Bt->n_terms, "A and B have different numbers of columns");
    if (A->n_rows == 0) return SG_OK;
    Scratch tmp(ctx);
    int64_t *d = nullptr;
    SG_TRY(tmp.alloc((size_t)A->n_rows, &d));
    hipLaunchKernelGGL(row_cost_kernel, dim3((unsigned)((A->n_rows + 255) / 256)), dim3(256), 0, ctx->stream,
                       A->d_indptr, A->d_indices, A->n_rows, (const uint32_t *)Bt->d_term_len, d);
    return sg_fetch(ctx, out_cost, d, sizeof(int64_t) * (size_t)A->n_rows);
}

extern "C" int sg_sp_matmul_topn_host(sg_ctx *ctx, int64_t n_left, int64_t n_right, int64_t n_cols,
                                      const int64_t *a_indptr, const int32_t *a_indices, const void *a_data,
                                      const int64_t *b_indptr, const int32_t *b_indices, const void *b_data,
                                      int32_t dtype, int32_t top_n, double threshold, int32_t sort,
                                      int32_t *out_cols, void *out_vals, int32_t *out_counts) {
    SG_REQUIRE(ctx && a_indptr && b_indptr && out_cols && out_vals && out_counts, "null argument");
    SG_REQUIRE(n_left >= 0 && n_right >= 0 && n_cols >= 0, "negative size");
    SG_REQUIRE(dtype == SG_F32 || dtype == SG_F64, "dtype must be SG_F32 or SG_F64");
    // A self-join as the reference issues it -- sp_matmul_topn(M, M.transpose(), ...), string_grouper.py:725-729 -- reaches
    // this function as the same matrix twice: the same buffers, or (a binding that converted the index arrays) equal ones.
    // One upload then serves both sides, and the multiply sees that A IS the indexed matrix: the self-join form, every pair
    // scored once.  (memcmp leaves at the first difference, so a real B costs nothing to tell apart.)
    bool same = n_left == n_right && a_indptr[n_left] == b_indptr[n_right];
    if (same && !(a_indptr == b_indptr && a_indices == b_indices && a_data == b_data)) {
        const size_t nnz = (size_t)a_indptr[n_left];
        same = std::memcmp(a_indptr, b_indptr, sizeof(int64_t) * (size_t)(n_left + 1)) == 0 &&
               (nnz == 0 || (std::memcmp(a_indices, b_indices, sizeof(int32_t) * nnz) == 0 &&
                             std::memcmp(a_data, b_data, (dtype == SG_F64 ? 8 : 4) * nnz) == 0));
    }
    // the four handles, freed in reverse -- the result, the index, B (unless it is A), A -- whichever way the call ends
    CsrPtr A, B;
    std::unique_ptr<sg_postings, int (*)(sg_postings *)> P(nullptr, sg_postings_free);
    TopnPtr R;
    sg_csr *m = nullptr;
    SG_TRY(sg_csr_from_host(ctx, n_left, n_cols, a_indptr, a_indices, a_data, dtype, &m));
    A.reset(m);
    if (!same) {
        SG_TRY(sg_csr_from_host(ctx, n_right, n_cols, b_indptr, b_indices, b_data, dtype, &m));
        B.reset(m);
    }
    sg_postings *p = nullptr;
    SG_TRY(sg_postings_build(ctx, same ? A.get() : B.get(), 0, &p));
    P.reset(p);
    sg_topn *r = nullptr;
    SG_TRY(sg_spgemm_topn(ctx, A.get(), P.get(), top_n, threshold, sort, &r));
    R.reset(r);
    return sg_topn_to_host(ctx, R.get(), out_cols, out_vals, out_counts);
}
