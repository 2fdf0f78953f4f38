// K3 -- inverted index of the right-hand matrix, bucketed by column tile.
//
// Replaces what the reference does at string_grouper/string_grouper.py:727 / :738
// (duplicate_matrix.transpose(), then sparse_dot_topn's internal CSC->CSR conversion of B^T).
//
// Layout in HBM.  For every term k (a column of the TF-IDF matrices) and every tile t of
// tile_cols = 2^tile_log2 consecutive right-hand rows, the postings
//     { (j, B[j,k]) : j in tile t }
// are stored contiguously; segment (k, t) is [seg[k*n_tiles+t], seg[k*n_tiles+t+1]).  The multiply
// (K4) walks the tiles of one left row with a private LDS accumulator of tile_cols values, so a tile
// only ever streams its own slice of each posting list.  Inside a segment the order of the j is
// irrelevant to the result (each (i,j) accumulator receives exactly one product per k), so the
// scatter below uses atomic cursors and needs no sort: a two-pass counting sort keyed by (k, tile).
//
// Bound: HBM.  Algorithmic bytes = 2 * nnz * (4 + s) + 4 * (V * n_tiles + n) (read B twice,
// write postings once, histogram + scan of the segment table).
#include <stdlib.h>

#include <memory>
#include <optional>

#include "sg_internal.h"
#include "sg_scan.h"

// Thread -> right-hand row.  Consecutive rows share a column tile, hence the bins of the frequent terms:
// with thread i on row i a whole wave hammers the same counter.  Consecutive threads are therefore dealt
// to consecutive TILES (thread g -> row (g mod n_tiles) * tile + g div n_tiles); every thread still walks
// its own row, so nothing is lost in coalescing.
__device__ __forceinline__ int64_t row_of_thread(int64_t g, int32_t tile_log2, int32_t n_tiles) {
    return ((g % n_tiles) << tile_log2) | (g / n_tiles);
}

template <typename T>
__global__ void __launch_bounds__(256) postings_count(const int64_t *__restrict__ indptr,
                                                      const int32_t *__restrict__ indices, int64_t n_rows,
                                                      int32_t tile_log2, int32_t n_tiles, uint32_t *seg_counts) {
    // one wave per 64 rows would leave lanes idle on short rows; nnz is only ~19/row, so a thread per
    // row with a short serial loop keeps the code simple
    const int64_t j = row_of_thread((int64_t)blockIdx.x * blockDim.x + threadIdx.x, tile_log2, n_tiles);
    if (j >= n_rows) return;
    const int64_t lo = indptr[j], hi = indptr[j + 1];
    const uint32_t t = (uint32_t)(j >> tile_log2);
    for (int64_t p = lo; p < hi; ++p) {
        const int64_t bin = (int64_t)indices[p] * n_tiles + t;
        atomicAdd(&seg_counts[bin], 1u);
    }
}

// posting entry layout (read by Post<T>::load in sg_spgemm_topn.hip):
//   f32: packed {uint32 slot, float value}, 8 bytes, in the vals array (rows array unused)
//   f64: slots[] (uint32, in the rows array) + vals[] (double)
// slot = (j mod tile_cols) * sizeof(T), the byte offset of column j's accumulator in the LDS tile
template <typename T>
__device__ __forceinline__ void store_posting(int32_t *rows, T *vals, uint32_t pos, int32_t j, T v);
template <>
__device__ __forceinline__ void store_posting<float>(int32_t *, float *vals, uint32_t pos, int32_t j, float v) {
    reinterpret_cast<uint2 *>(vals)[pos] = make_uint2((uint32_t)j, __float_as_uint(v));
}
template <>
__device__ __forceinline__ void store_posting<double>(int32_t *rows, double *vals, uint32_t pos, int32_t j, double v) {
    rows[pos] = j;
    vals[pos] = v;
}

// norm of a row's frequent part (terms whose list holds >= freq_min entries) relative to norm_up, rounded up
// (emit_posting quantises it upwards once more, to the bits the form of the posting has for it)
__device__ __forceinline__ float frequent_norm_ratio_of(double f2, float inv_norm_up) {
    return __double2float_ru(sqrt(f2) * (1.0 + 1e-12)) * inv_norm_up;
}
template <typename T>
__device__ __forceinline__ float frequent_norm_ratio(const int32_t *__restrict__ indices, const T *__restrict__ data,
                                                     int64_t lo, int64_t hi, const uint32_t *__restrict__ seg, int32_t n_tiles,
                                                     uint32_t freq_min, float inv_norm_up) {
    double f2 = 0.0;
    for (int64_t p = lo; p < hi; ++p) {
        const int64_t k = indices[p];
        if (seg[(k + 1) * n_tiles] - seg[k * n_tiles] >= freq_min) f2 += (double)data[p] * (double)data[p];
    }
    return frequent_norm_ratio_of(f2, inv_norm_up);
}

// Entry i of the 512 "null postings" behind the filter postings (stream form: a lane that is through with its segment
// reads entries 4 * lane .. 4 * lane + 3): bq = fq = 0 and ALL FOUR entries of a lane name accumulator word `lane` -- one
// LDS instruction of the wave then touches 64 different words, and the low 24 bits of the entry, which the multiply
// takes for the value, stay below 256: (CA * 252) >> 32 == 0 for every CA < 2^24, the entry adds nothing.
__device__ __forceinline__ uint32_t sg_null_posting(uint32_t i) { return ((i >> 2) << 2) | 0x80000000u; }

// one posting (+ its filter posting) of column `col` of the tile at position `pos`.
// Filter posting (read by K4p, sg_spgemm_pruned.hip), 32 bits, AB = tile_log2 + 1.  `fr` = the norm of the row's frequent
// part relative to norm_up, rounded up (frequent_norm_ratio).
// Tile-by-tile form (fold_log2 == 0):
//   [0]        h     which 16-bit half of the accumulator word the column owns (col & 1)
//   [1]        0
//   [2, AB)    word  (col >> 1): bits [0, AB) masked with ~3 ARE the byte address of the accumulator word in LDS
//   [AB, 24)   bq    value quantised upwards relative to norm_up
//   [24, 32)   fq    fr quantised upwards to 8 bits
// Stream form (fold_log2 == 3, tile_log2 == 12; sg_spgemm_pruned.hip, "stream form"): 2^fold_log2 consecutive tiles share
// ONE accumulator tile, the posting says which of them its column lies in, and the fields are cut for the multiply's
// instructions (round 4: 11 -> 8 VALU per posting):
//   [0]        0
//   [1]        h     (<< 3 it is the shift of the half: 0 or 16; bits [1, 16) >> 1 ARE the column inside the super-tile)
//   [2, 13)    word
//   [13, 16)   fold  tile index mod 8
//   [16, 24)   bq    chosen so that the low 24 bits AS ONE NUMBER are >= v / norm_up * 255 * 2^16: the multiply feeds the
//                    posting to v_mul_hi_u32_u24 as it is -- the bits below bq then count as part of the value, and K3,
//                    which knows them, rounds bq down by what they are worth (the bound is as tight as rounding bq up
//                    by itself was, and the multiply saves the mask)
//   [24, 32)   fq    chosen the same way: bits [16, 32) as one number F >= fr * 255 * 2^8 (bq counts as its low byte), stored
//                    with its top bit flipped (F - 32768 as int16) for v_mad_i32_i16, which then gives the column's whole
//                    survivor threshold in ONE instruction (the 8-bit form: byte select + multiply, subtract, shift)
#define SG_FILT_F16_MAX 65280u   // 255 * 256
// the 32-bit filter posting of value v in column `col` of tile `tile` (the layouts above)
__device__ __forceinline__ uint32_t filter_posting(uint32_t col, float v, float fr, int32_t tile_log2, float inv_norm_up, uint32_t tile,
                                                   int32_t fold_log2) {
    const int32_t ab = tile_log2 + 1, fb = ab + fold_log2;
    if (fold_log2 > 0) {   // stream form (fb == 16: sg_postings_build only folds tiles of 4096 columns by 8)
        const uint32_t low = ((col >> 1) << 2) | ((col & 1u) << 1) | ((tile & ((1u << fold_log2) - 1u)) << ab);
        uint32_t b24 = (uint32_t)ceilf(v * inv_norm_up * (255.0f * 65536.0f) * 1.000002f);
        // v <= norm_up: what lies above 255 * 2^16 is the safety factor's doing.  (Without the cut a row of ONE term --
        // v = 1 -- in one of a tile's first columns, where `low` is smaller than that excess, got bq = 256: the field
        // wrapped to 0 and carried into fq, and the row did not find itself.)
        if (b24 > (255u << 16)) b24 = 255u << 16;
        const uint32_t bq = b24 > low ? (b24 - low + 65535u) >> 16 : 0u;                   // <= 255
        uint32_t f16 = (uint32_t)ceilf(fr * (float)SG_FILT_F16_MAX * 1.000002f);
        if (f16 > SG_FILT_F16_MAX) f16 = SG_FILT_F16_MAX;
        const uint32_t fq = f16 > bq ? (f16 - bq + 255u) >> 8 : 0u;                        // <= 255
        return low | (bq << 16) | ((fq ^ 0x80u) << 24);
    }
    const uint32_t bq_max = (1u << (24 - fb)) - 1u;   // the bits the address and fq leave
    uint32_t bq = (uint32_t)ceilf(v * inv_norm_up * (float)bq_max * 1.000002f);
    if (bq > bq_max) bq = bq_max;
    uint32_t fq = (uint32_t)ceilf(fr * 255.0f * 1.000002f);
    if (fq > 255u) fq = 255u;
    return ((col >> 1) << 2) | (col & 1u) | (bq << fb) | (fq << 24);
}
template <typename T>
__device__ __forceinline__ void emit_posting(int32_t *out_rows, T *out_vals, uint32_t *out_filt, uint32_t pos, uint32_t col,
                                             T v, float fr, int32_t tile_log2, float inv_norm_up, uint32_t tile,
                                             int32_t fold_log2) {
    // the multiply wants the byte offset of the accumulator inside its LDS tile, not j itself
    if (out_vals) store_posting<T>(out_rows, out_vals, pos, (int32_t)(col * (uint32_t)sizeof(T)), v);   // (null: filter postings only)
    if (out_filt) out_filt[pos] = filter_posting(col, (float)v, fr, tile_log2, inv_norm_up, tile, fold_log2);
}

template <typename T>
__global__ void __launch_bounds__(256) postings_fill(const int64_t *__restrict__ indptr,
                                                     const int32_t *__restrict__ indices,
                                                     const T *__restrict__ data, int64_t n_rows, int32_t tile_log2,
                                                     int32_t n_tiles, const uint32_t *__restrict__ seg,
                                                     uint32_t *cursor, int32_t *out_rows, T *out_vals,
                                                     uint32_t *out_filt /* null: no filter postings */,
                                                     uint32_t freq_min, float inv_norm_up, int32_t fold_log2) {
    const int64_t j = row_of_thread((int64_t)blockIdx.x * blockDim.x + threadIdx.x, tile_log2, n_tiles);
    if (j >= n_rows) return;
    const int64_t lo = indptr[j], hi = indptr[j + 1];
    const uint32_t t = (uint32_t)(j >> tile_log2);
    const uint32_t col = (uint32_t)(j & (((int64_t)1 << tile_log2) - 1));
    const float fq = out_filt ? frequent_norm_ratio<T>(indices, data, lo, hi, seg, n_tiles, freq_min, inv_norm_up) : 0.f;
    for (int64_t p = lo; p < hi; ++p) {
        const int64_t bin = (int64_t)indices[p] * n_tiles + t;
        const uint32_t pos = seg[bin] + atomicAdd(&cursor[bin], 1u);
        emit_posting<T>(out_rows, out_vals, out_filt, pos, col, data[p], fq, tile_log2, inv_norm_up, t, fold_log2);
    }
}

// The same two passes with the counters in LDS (4 bytes per term; used when the vocabulary fits: n_terms * 4 <= 120 KiB):
// a workgroup owns a column tile -- or, with `split` > 1, one of `split` equal parts of it, so that 162 tiles still fill
// 256 CUs; a segment (k, t) is then the parts' sub-segments back to back, which the multiply never notices since the
// order inside a segment is free.  Sixteen lanes walk one row (the loads of a row are contiguous across lanes; a thread
// per row steps 64 rows with one cache line each), LDS atomics take the place of 2 x nnz global ones.
//
// Round 4: the counters live in a table that is WORKGROUP-major while the index is built -- cnt[w * n_terms + k], w =
// tile * split + part -- so that a workgroup writes its histogram and reads its cursors as ONE contiguous run of
// n_terms words.  (Rounds 2-3 kept it term-major, (k * n_tiles + t) * split + part: every workgroup then gathered its
// 18 300 cursors from 18 300 different cache lines, and so did the histogram's write-back.)  The offsets come in two
// steps: postings_colscan_kernel turns every term's column of counts into running sums over w (the term's entries in
// earlier parts) and its total, one small scan over the totals gives the terms' starts, and a cursor is the sum of
// the two.  postings_tables_kernel then writes what the multiply reads -- the term-major segment table and the two
// padded tables of segment ends -- transposed through LDS.
// Both passes walk FOUR rows per sixteen lanes and trip with all their loads issued before the first is used: a
// workgroup's trips are serial (32 of them for a part of 2048 rows) and a trip is a chain of dependent round trips --
// row pointers, entries, LDS, store -- so that the build ran at the latency of its loads, not at any bandwidth
// (profiles/r04_s1_kernel_stats_baseline.csv: 0.31 ms for 100 MB).
#define SG_POST_ROWS 4    // rows per sixteen lanes and trip
// Where part `part` of a tile's `split` parts begins, in rows from the tile's start: part * tile_cols / split, rounded down to a
// multiple of 64 rows (part == split: the tile's end).  `split` is any integer, not only a power of two -- so that the
// workgroups of a launch can be made to fill the chip (plan_build, choose_split); count, fill and tables agree on the
// boundaries through this one function and through the workgroup's number w = tile * split + part.
__host__ __device__ __forceinline__ int64_t part_begin(int32_t part, int32_t split, int32_t tile_log2) {
    return part >= split ? (int64_t)1 << tile_log2 : ((((int64_t)part << tile_log2) / split) & ~(int64_t)63);
}
__global__ void __launch_bounds__(1024) postings_count_lds(const int64_t *__restrict__ indptr,
                                                           const int32_t *__restrict__ indices, int64_t n_rows,
                                                           int32_t tile_log2, int32_t n_terms, int32_t split,
                                                           uint32_t *__restrict__ cnt /* [wgs][n_terms] */,
                                                           uint32_t *__restrict__ cnt16 /* [wgs][(n_terms + 1) / 2], or null */) {
    extern __shared__ uint32_t hist[];
    const int64_t t = blockIdx.x / split;
    const int32_t part = blockIdx.x % split;
    for (int k = threadIdx.x; k < n_terms; k += blockDim.x) hist[k] = 0;
    __syncthreads();
    const int64_t j0 = (t << tile_log2) + part_begin(part, split, tile_log2);
    int64_t j1 = (t << tile_log2) + part_begin(part + 1, split, tile_log2);
    if (j1 > n_rows) j1 = n_rows;
    const int sub = threadIdx.x & 15;
    const int64_t groups = blockDim.x >> 4;
    for (int64_t jb = j0 + (threadIdx.x >> 4) * SG_POST_ROWS; jb < j1; jb += groups * SG_POST_ROWS) {
        int64_t lo[SG_POST_ROWS], hi[SG_POST_ROWS];
#pragma unroll
        for (int r = 0; r < SG_POST_ROWS; ++r) {
            const bool valid = jb + r < j1;
            lo[r] = valid ? indptr[jb + r] : 0;
            hi[r] = valid ? indptr[jb + r + 1] : 0;
        }
        // a row's first 32 entries, two a lane, in flight together (a name has 19 on average: most rows have a 17th, and one
        // row after the other waiting for its own was a chain of four round trips a trip)
        int32_t k0[SG_POST_ROWS], k1[SG_POST_ROWS];
#pragma unroll
        for (int r = 0; r < SG_POST_ROWS; ++r) {
            k0[r] = lo[r] + sub < hi[r] ? indices[lo[r] + sub] : -1;
            k1[r] = lo[r] + sub + 16 < hi[r] ? indices[lo[r] + sub + 16] : -1;
        }
#pragma unroll
        for (int r = 0; r < SG_POST_ROWS; ++r) {
            if (k0[r] >= 0) atomicAdd(&hist[k0[r]], 1u);
            if (k1[r] >= 0) atomicAdd(&hist[k1[r]], 1u);
            for (int64_t p = lo[r] + sub + 32; p < hi[r]; p += 16) atomicAdd(&hist[indices[p]], 1u);   // rows beyond 32 entries
        }
    }
    __syncthreads();
    uint32_t *mine = cnt + (int64_t)blockIdx.x * n_terms;
    for (int k = threadIdx.x; k < n_terms; k += blockDim.x) mine[k] = hist[k];
    // The part's own counts once more, 16 bits a term and packed as the staged fill keeps them in LDS: the column scan turns
    // `cnt` into running sums, and the fill would otherwise count the part's rows a second time.  (A count beyond 16 bits
    // is cut: such a part holds more entries than the fill stages, and it does not read these.)
    if (cnt16) {
        const int w16 = (n_terms + 1) >> 1;
        uint32_t *mine16 = cnt16 + (int64_t)blockIdx.x * w16;
        for (int w = threadIdx.x; w < w16; w += blockDim.x) {
            const uint32_t a = hist[2 * w], b = 2 * w + 1 < n_terms ? hist[2 * w + 1] : 0u;
            mine16[w] = (a < 0xffffu ? a : 0xffffu) | ((b < 0xffffu ? b : 0xffffu) << 16);
        }
    }
}

// Per term: counts of the workgroups -> entries of the term in EARLIER workgroups (in place), the term's total, and
// whether it is frequent.  A workgroup takes 64 terms x all workgroups of the build: 16 threads per term, each a run of
// consecutive w, the runs joined through LDS; loads and stores are contiguous across the 64 terms.
__global__ void __launch_bounds__(1024) postings_colscan_kernel(uint32_t *__restrict__ cnt, int32_t n_wgs, int32_t n_terms,
                                                                uint32_t freq_min, uint32_t *__restrict__ term_len,
                                                                uint8_t *__restrict__ is_frequent) {
    __shared__ uint32_t part_sum[16][64];
    const int kk = threadIdx.x & 63, c = threadIdx.x >> 6;
    const int64_t k = (int64_t)blockIdx.x * 64 + kk;
    const int32_t run = (n_wgs + 15) / 16;
    const int32_t w0 = c * run, w1 = min(w0 + run, n_wgs);
    uint32_t s = 0;
    if (k < n_terms)
        for (int32_t w = w0; w < w1; ++w) s += cnt[(int64_t)w * n_terms + k];
    part_sum[c][kk] = s;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const uint32_t v = part_sum[q][kk];
        before += q < c ? v : 0u;
        total += v;
    }
    if (k < n_terms) {
        for (int32_t w = w0; w < w1; ++w) {
            const uint32_t v = cnt[(int64_t)w * n_terms + k];
            cnt[(int64_t)w * n_terms + k] = before;
            before += v;
        }
        if (c == 0) {
            term_len[k] = total;
            if (is_frequent) is_frequent[k] = total >= freq_min ? 1 : 0;
        }
    }
}

// What the multiply reads, from the build's tables: S(k, t) = term_start[k] + cnt[(t * split) * n_terms + k] is the start
// of term k's postings in tile t, S(k, n_tiles) = term_start[k + 1];
//   seg[k * n_tiles + t] = S(k, t)                                   (+ seg[n_terms * n_tiles] = all postings)
//   ends[k * nt_pad + t] = S(k, min(t, n_tiles - 1) + 1) << 2        byte offsets into the filter postings, rows padded to
//                                                                    a multiple of four tiles; row n_terms: zeros (the
//                                                                    segments of a lane without a term)
//   ends8[k * nv_pad + v] = S(k, min((v + 1) << fold_log2, n_tiles)) << 2   the same for super-tiles (stream form)
// A workgroup takes 64 terms and walks the tiles 64 at a time: read with the lanes along the terms (the table is
// workgroup-major), written with the lanes along the tiles (the multiply's tables are term-major), through LDS.
__global__ void __launch_bounds__(1024) postings_tables_kernel(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ term_start,
                                                               int32_t n_terms, int32_t n_tiles, int32_t split,
                                                               uint32_t *__restrict__ seg, uint32_t *__restrict__ ends, int32_t nt_pad,
                                                               uint32_t *__restrict__ ends8, int32_t nv_pad, int32_t fold_log2,
                                                               SgScoreCtx sc, SgScoreCtx *__restrict__ sc_out /* null: none */,
                                                               uint32_t *__restrict__ null_slack /* null: none */) {
    __shared__ uint32_t tile[64][66];
    if (blockIdx.x == 0) {   // two one-line kernels of the build ride along: the scoring context as a struct in device memory
        if (sc_out && threadIdx.x == 0) {                                   // (score_ctx_kernel)
            sc_out[0] = sc;
            sc.q8 = nullptr;                                                // [1]: the same without the second filter (the
            sc.q8_scale = 0.f;                                              //      multiply chooses per call: sg_q8_applies)
            sc_out[1] = sc;
        }
        if (null_slack && threadIdx.x < 512) null_slack[threadIdx.x] = sg_null_posting(threadIdx.x);   // (null_postings_kernel)
    }
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;   // y: 0 .. 15
    const int64_t k0 = (int64_t)blockIdx.x * 64;
    auto S = [&](int64_t k, int64_t t) -> uint32_t {        // k <= n_terms, t <= n_tiles
        if (k >= n_terms) return term_start[n_terms];
        return t >= n_tiles ? term_start[k + 1] : term_start[k] + cnt[(t * split) * (int64_t)n_terms + k];
    };
    const int64_t t_lim = nt_pad > n_tiles ? nt_pad : n_tiles;
    for (int64_t tb = 0; tb < t_lim; tb += 64) {
        // columns tb .. tb + 64 (one more than is written: an end is the next tile's start)
        for (int tt = y; tt < 65; tt += 16) {
            const int64_t k = k0 + x;
            tile[x][tt] = k <= n_terms ? S(k, min(tb + tt, (int64_t)n_tiles)) : 0u;
        }
        __syncthreads();
        for (int kq = y; kq < 64; kq += 16) {
            const int64_t k = k0 + kq, t = tb + x;
            if (k < n_terms && t < n_tiles) seg[k * n_tiles + t] = tile[kq][x];
            if (k == n_terms && t == 0) seg[k * n_tiles] = tile[kq][0];                    // the table's last entry: all postings
            if (ends && k <= n_terms && t < nt_pad)
                ends[k * nt_pad + t] = k == n_terms ? 0u : tile[kq][min(t, (int64_t)n_tiles - 1) + 1 - tb] << 2;
        }
        __syncthreads();
    }
    if (ends8) {
        for (int64_t i = threadIdx.x; i < (int64_t)64 * nv_pad; i += blockDim.x) {
            const int64_t k = k0 + (i & 63), v = i >> 6;
            if (k > n_terms) continue;
            ends8[k * nv_pad + v] = k == n_terms ? 0u : S(k, min((v + 1) << fold_log2, (int64_t)n_tiles)) << 2;
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(1024) postings_fill_lds(const int64_t *__restrict__ indptr,
                                                          const int32_t *__restrict__ indices,
                                                          const T *__restrict__ data, int64_t n_rows, int32_t tile_log2,
                                                          int32_t n_terms, int32_t split,
                                                          const uint32_t *__restrict__ cnt /* [wgs][n_terms]: entries in earlier workgroups */,
                                                          const uint32_t *__restrict__ term_start,
                                                          const uint8_t *__restrict__ is_frequent, int32_t *out_rows,
                                                          T *out_vals, uint32_t *out_filt, float inv_norm_up, int32_t fold_log2) {
    extern __shared__ uint32_t cursor[];   // next free slot of (term k, this tile, this part); then the frequent-term bits
    uint32_t *freq_bits = cursor + n_terms;
    const int64_t t = blockIdx.x / split;
    const int32_t part = blockIdx.x % split;
    for (int k = threadIdx.x; k < (n_terms + 31) / 32; k += blockDim.x) freq_bits[k] = 0;
    const uint32_t *mine = cnt + (int64_t)blockIdx.x * n_terms;
    for (int k = threadIdx.x; k < n_terms; k += blockDim.x) cursor[k] = term_start[k] + mine[k];
    __syncthreads();
    if (out_filt)
        for (int k = threadIdx.x; k < n_terms; k += blockDim.x)
            if (is_frequent[k]) atomicOr(&freq_bits[k >> 5], 1u << (k & 31));
    __syncthreads();
    const int64_t j0 = (t << tile_log2) + part_begin(part, split, tile_log2);
    int64_t j1 = (t << tile_log2) + part_begin(part + 1, split, tile_log2);
    if (j1 > n_rows) j1 = n_rows;
    const int lane = threadIdx.x & 63, sub = lane & 15;
    (void)lane;
    const int64_t groups = blockDim.x >> 4;
    // every wave makes the same number of trips, so that the cross-lane sums below always run with all lanes
    const int64_t trips = (j1 - j0 + groups * SG_POST_ROWS - 1) / (groups * SG_POST_ROWS);
    for (int64_t it = 0; it < trips; ++it) {
        const int64_t jb = j0 + (it * groups + (threadIdx.x >> 4)) * SG_POST_ROWS;
        int64_t lo[SG_POST_ROWS], hi[SG_POST_ROWS];
#pragma unroll
        for (int r = 0; r < SG_POST_ROWS; ++r) {
            const bool valid = jb + r < j1;
            lo[r] = valid ? indptr[jb + r] : 0;
            hi[r] = valid ? indptr[jb + r + 1] : 0;
        }
        // the lane's first entry of every row: all loads before the first use (rows of up to sixteen entries are through
        // with these; the rest of a longer row goes entry by entry below)
        int32_t k0[SG_POST_ROWS];
        T v0[SG_POST_ROWS];
#pragma unroll
        for (int r = 0; r < SG_POST_ROWS; ++r) {
            const bool have = lo[r] + sub < hi[r];
            k0[r] = have ? indices[lo[r] + sub] : -1;
            v0[r] = have ? data[lo[r] + sub] : (T)0;
        }
        float fq[SG_POST_ROWS];
#pragma unroll
        for (int r = 0; r < SG_POST_ROWS; ++r) {
            fq[r] = 0.f;
#if defined(SG_K3_PROBE_NO_FQ)
            if (out_filt && n_rows < 0) {
#else
            if (out_filt) {
#endif
                // norm of the row's frequent part relative to norm_up, rounded up (the order of the additions is free: the
                // result is rounded up with a margin far above the rounding of a double sum)
                double f2 = 0.0;
                if (k0[r] >= 0 && ((freq_bits[k0[r] >> 5] >> (k0[r] & 31)) & 1u)) f2 = (double)v0[r] * (double)v0[r];
                for (int64_t p = lo[r] + sub + 16; p < hi[r]; p += 16) {
                    const int32_t k = indices[p];
                    if ((freq_bits[k >> 5] >> (k & 31)) & 1u) f2 += (double)data[p] * (double)data[p];
                }
#pragma unroll
                for (int d = 8; d > 0; d >>= 1) {
                    const uint64_t bits = (uint64_t)__double_as_longlong(f2);
                    const uint32_t l = (uint32_t)__shfl_xor((int)(uint32_t)bits, d, 64), h = (uint32_t)__shfl_xor((int)(uint32_t)(bits >> 32), d, 64);
                    f2 += __longlong_as_double((long long)(((uint64_t)h << 32) | l));
                }
                fq[r] = frequent_norm_ratio_of(f2, inv_norm_up);
            }
        }
#pragma unroll
        for (int r = 0; r < SG_POST_ROWS; ++r) {
            const uint32_t col = (uint32_t)(jb + r - (t << tile_log2));
            if (k0[r] >= 0) {
#if defined(SG_K3_PROBE_NO_ATOMIC)   // timing probes (wrong results): a build of the library per probe, A/B through SG_HIP_LIB
                const uint32_t pos = cursor[k0[r]] + (uint32_t)(threadIdx.x & 3);
#else
                const uint32_t pos = atomicAdd(&cursor[k0[r]], 1u);
#endif
#if defined(SG_K3_PROBE_NO_STORE)
                if (pos == 0xFFFFFFF0u)
#endif
                emit_posting<T>(out_rows, out_vals, out_filt, pos, col, v0[r], fq[r], tile_log2, inv_norm_up, (uint32_t)t, fold_log2);
            }
            for (int64_t p = lo[r] + sub + 16; p < hi[r]; p += 16) {
                const uint32_t pos = atomicAdd(&cursor[indices[p]], 1u);
                emit_posting<T>(out_rows, out_vals, out_filt, pos, col, data[p], fq[r], tile_log2, inv_norm_up, (uint32_t)t, fold_log2);
            }
        }
    }
}

// ---- The filter postings STAGED in LDS and written cell by cell.
// postings_fill_lds stores every posting where its cursor says: 4 bytes to a line of its own -- the term-major order the
// multiply streams puts the postings of one row 18 300 lists apart --, and those stores were half the kernel.  But the
// entries of a (term, part) CELL are neighbours in the index, and most entries live in cells of many (frequent terms: a part
// of 1024 rows holds 4.3 entries per non-empty cell, 56 % of the entries in cells of eight or more).  So a workgroup works its
// part off in CHUNKS of rows whose postings fit the LDS beside packed 16-bit counters:
//   (1) the chunk's entries per term.  A part that IS one chunk -- what plan_build aims for -- loads them: the count pass
//       counted exactly these rows and left the counts packed (cnt16), so the rows are read ONCE here.  A part of several
//       chunks (long strings, a forced split) counts every chunk itself, as it must: the count pass knows the part only.
//   (2) a prefix sum turns the counts into the cells' places inside the chunk;
//   (3) every posting is made and put at its place in LDS, its term beside it (16 bits: the vocabulary fits the LDS path);
//       the row's frequent-part norm is summed by the row's sixteen lanes in the same trip, before they emit;
//   (4) waves copy the staged run out, 64 consecutive staged postings a trip: lanes in the same cell write neighbouring
//       words, a trip touches ~15 lines instead of 64.  A lane knows its posting's term, so nothing is searched and no empty
//       cell is visited: the first lane of every run of one term in the trip (a "head") fetches where the cell starts in
//       the index -- the term's start + the workgroup's row of `cnt` (entries in earlier workgroups; the tables the multiply
//       reads are written from `cnt` BEFORE this kernel runs) -- and hands it to the run's other lanes by a shuffle.
// A part of one chunk never writes its row of `cnt`.  A part of several advances a cell's start by the chunk's count once a
// cell, by the lane that holds the cell's first staged posting, behind a barrier after the copy (a cell that straddles two
// trips is read by two heads) -- plain loads and stores of the one workgroup that owns the row.  A chunk that does not fit
// the stage (rows far longer than the build's mean) is written posting by posting through the same cursors.
// Filter postings only: the exact kernel's postings, when they are wanted at all, keep postings_fill_lds.
__device__ __forceinline__ uint32_t lds_get16(const uint32_t *w, uint32_t k) { return (w[k >> 1] >> ((k & 1u) << 4)) & 0xffffu; }
// words of LDS for a chunk's row pointers (relative to the chunk's first entry; one more than rows)
__host__ __device__ __forceinline__ uint32_t staged_rowp_words(int32_t chunk_rows) { return ((uint32_t)chunk_rows + 4u) & ~3u; }
template <typename T>
__global__ void __launch_bounds__(1024) postings_fill_staged(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                             const T *__restrict__ data, int64_t n_rows, int32_t tile_log2,
                                                             int32_t n_terms, int32_t split, int32_t chunk_rows, uint32_t stage_cap,
                                                             uint32_t stage_alloc /* postings the stage has room for (>= stage_cap) */,
                                                             uint32_t *cnt /* [wgs][n_terms] */,
                                                             const uint32_t *__restrict__ cnt16 /* [wgs][(n_terms + 1) / 2] */,
                                                             const uint32_t *__restrict__ term_start,
                                                             const uint8_t *__restrict__ is_frequent, uint32_t *__restrict__ out_filt,
                                                             float inv_norm_up, int32_t fold_log2) {
    extern __shared__ uint32_t lds[];
    const uint32_t w16 = ((uint32_t)n_terms + 1u) >> 1;            // words of packed 16-bit counters
    uint32_t *lcnt = lds;
    uint32_t *freq_bits = lcnt + ((w16 + 3u) & ~3u);
    uint32_t *wave_tot = freq_bits + (((uint32_t)n_terms + 31u) >> 5);
    uint32_t *rowp = wave_tot + 32;
    uint32_t *stage = rowp + staged_rowp_words(chunk_rows);
    uint16_t *sterm = reinterpret_cast<uint16_t *>(stage + stage_alloc);
    const int64_t t = blockIdx.x / split;
    const int32_t part = blockIdx.x % split;
    uint32_t *mine = cnt + (int64_t)blockIdx.x * n_terms;
    const int64_t j0 = (t << tile_log2) + part_begin(part, split, tile_log2);
    int64_t j1 = (t << tile_log2) + part_begin(part + 1, split, tile_log2);
    if (j1 > n_rows) j1 = n_rows;
    if (j1 <= j0) return;                                          // (a part behind the last row)
    const int lane = threadIdx.x & 63, sub = lane & 15, wave = threadIdx.x >> 6;
    const int64_t groups = blockDim.x >> 4;
    // A workgroup whose part holds a chunk that does not fit the stage writes ALL its chunks posting by posting: its cursors
    // are then only ever touched by atomics, a staging workgroup's only by plain loads and stores -- never both (atomics
    // are served by the L2, plain loads may come from the L1: mixing them per workgroup needed loads and stores through the
    // fabric, which doubled the kernel -- 0.53 instead of 0.26 ms at 663 k).
    bool any_big = false;
    for (int64_t c0 = j0; c0 < j1; c0 += chunk_rows) {
        const int64_t c1 = c0 + chunk_rows < j1 ? c0 + chunk_rows : j1;
        const int64_t e = indptr[c1] - indptr[c0];
        any_big = any_big || e > (int64_t)stage_cap || e > 65535;
    }
    const bool one_chunk = j1 - j0 <= chunk_rows && !any_big;
    // Everything a workgroup fetches before it can start is issued together -- one round trip to memory, not one a loop trip
    // (a workgroup is alone on its CU, nothing hides a chain of dependent loads).
    // * One bit per term from the column scan's byte flags: a thread makes a whole word, its eight loads in flight at once.
    {
        const uint32_t *flags4 = reinterpret_cast<const uint32_t *>(is_frequent);   // (allocated beyond a multiple of four bytes)
        for (uint32_t w = threadIdx.x; w < (((uint32_t)n_terms + 31u) >> 5); w += blockDim.x) {
            uint32_t f[8];
#pragma unroll
            for (uint32_t q = 0; q < 8; ++q) f[q] = (w * 8u + q) * 4u < (uint32_t)n_terms ? flags4[w * 8u + q] : 0u;
            uint32_t bits = 0;
#pragma unroll
            for (uint32_t i = 0; i < 32; ++i)
                if (w * 32u + i < (uint32_t)n_terms && ((f[i >> 2] >> ((i & 3u) << 3)) & 0xffu)) bits |= 1u << i;
            freq_bits[w] = bits;
        }
    }
    // * A chunk's row pointers, relative to its first entry (a staged chunk holds fewer than 2^16), so that a trip over the
    //   rows waits for its entries only.
    auto load_row_pointers = [&](int64_t c0, int64_t c1) {
        const int64_t base = indptr[c0];
        for (int64_t i = threadIdx.x; i <= c1 - c0; i += blockDim.x) rowp[i] = (uint32_t)(indptr[c0 + i] - base);
    };
    if (one_chunk) {   // (1), loaded
        const uint32_t *mine16 = cnt16 + (int64_t)blockIdx.x * w16;
        for (uint32_t w0 = threadIdx.x; w0 < w16; w0 += blockDim.x * 8u) {
            uint32_t v[8];
#pragma unroll
            for (uint32_t q = 0; q < 8; ++q) v[q] = w0 + q * blockDim.x < w16 ? mine16[w0 + q * blockDim.x] : 0u;
#pragma unroll
            for (uint32_t q = 0; q < 8; ++q)
                if (w0 + q * blockDim.x < w16) lcnt[w0 + q * blockDim.x] = v[q];
        }
        load_row_pointers(j0, j1);
    }
    __syncthreads();
    for (int64_t c0 = j0; c0 < j1; c0 += chunk_rows) {
        const int64_t c1 = c0 + chunk_rows < j1 ? c0 + chunk_rows : j1;
        // every wave makes the same number of trips, so that the cross-lane sums below always run with all lanes
        const int64_t trips = (c1 - c0 + groups * SG_POST_ROWS - 1) / (groups * SG_POST_ROWS);
        if (any_big) {
            // (rows far longer than the build expected: posting by posting through the workgroup's cursors)
            for (int64_t it = 0; it < trips; ++it) {
                const int64_t jb = c0 + (it * groups + (threadIdx.x >> 4)) * SG_POST_ROWS;
#pragma unroll
                for (int r = 0; r < SG_POST_ROWS; ++r) {
                    const bool valid = jb + r < c1;
                    const int64_t lo = valid ? indptr[jb + r] : 0, hi = valid ? indptr[jb + r + 1] : 0;
                    double f2 = 0.0;
                    for (int64_t p = lo + sub; p < hi; p += 16) {
                        const int32_t k = indices[p];
                        if ((freq_bits[k >> 5] >> (k & 31)) & 1u) f2 += (double)data[p] * (double)data[p];
                    }
#pragma unroll
                    for (int d = 8; d > 0; d >>= 1) {
                        const uint64_t bits = (uint64_t)__double_as_longlong(f2);
                        const uint32_t l = (uint32_t)__shfl_xor((int)(uint32_t)bits, d, 64), h = (uint32_t)__shfl_xor((int)(uint32_t)(bits >> 32), d, 64);
                        f2 += __longlong_as_double((long long)(((uint64_t)h << 32) | l));
                    }
                    const float fq = frequent_norm_ratio_of(f2, inv_norm_up);
                    const uint32_t col = (uint32_t)(jb + r - (t << tile_log2));
                    for (int64_t p = lo + sub; p < hi; p += 16) {
                        const int32_t k = indices[p];
                        const uint32_t pos = term_start[k] + atomicAdd(&mine[k], 1u);
                        out_filt[pos] = filter_posting(col, (float)data[p], fq, tile_log2, inv_norm_up, (uint32_t)t, fold_log2);
                    }
                }
            }
            continue;
        }
        const int64_t chunk_base = indptr[c0];
        if (!one_chunk) {
            // ---- (1), counted: this chunk's entries per term
            for (uint32_t w = threadIdx.x; w < w16; w += blockDim.x) lcnt[w] = 0;
            load_row_pointers(c0, c1);
            __syncthreads();
            for (int64_t it = 0; it < trips; ++it) {
                const int64_t jb = c0 + (it * groups + (threadIdx.x >> 4)) * SG_POST_ROWS;
                int64_t lo[SG_POST_ROWS], hi[SG_POST_ROWS];
#pragma unroll
                for (int r = 0; r < SG_POST_ROWS; ++r) {
                    const bool valid = jb + r < c1;
                    lo[r] = valid ? chunk_base + rowp[jb + r - c0] : 0;
                    hi[r] = valid ? chunk_base + rowp[jb + r - c0 + 1] : 0;
                }
                int32_t k0[SG_POST_ROWS], k1[SG_POST_ROWS];
#pragma unroll
                for (int r = 0; r < SG_POST_ROWS; ++r) {
                    k0[r] = lo[r] + sub < hi[r] ? indices[lo[r] + sub] : -1;
                    k1[r] = lo[r] + sub + 16 < hi[r] ? indices[lo[r] + sub + 16] : -1;
                }
#pragma unroll
                for (int r = 0; r < SG_POST_ROWS; ++r) {
                    if (k0[r] >= 0) atomicAdd(&lcnt[(uint32_t)k0[r] >> 1], 1u << (((uint32_t)k0[r] & 1u) << 4));
                    if (k1[r] >= 0) atomicAdd(&lcnt[(uint32_t)k1[r] >> 1], 1u << (((uint32_t)k1[r] & 1u) << 4));
                    for (int64_t p = lo[r] + sub + 32; p < hi[r]; p += 16) {
                        const uint32_t k = (uint32_t)indices[p];
                        atomicAdd(&lcnt[k >> 1], 1u << ((k & 1u) << 4));
                    }
                }
            }
            __syncthreads();
        }
        // ---- (2) counts -> where every term's cell starts inside the chunk (a thread takes a run of words)
        uint32_t tot;
        {
            const uint32_t per = (w16 + blockDim.x - 1u) / blockDim.x;
            const uint32_t wa = threadIdx.x * per < w16 ? threadIdx.x * per : w16, wb = wa + per < w16 ? wa + per : w16;
            uint32_t sum = 0;
            for (uint32_t w = wa; w < wb; ++w) sum += (lcnt[w] & 0xffffu) + (lcnt[w] >> 16);
            uint32_t run = block_exclusive_scan<uint32_t>(sum, wave_tot, &tot);
            for (uint32_t w = wa; w < wb; ++w) {
                const uint32_t c = lcnt[w];
                const uint32_t a = run;
                run += c & 0xffffu;
                const uint32_t b = run;
                run += c >> 16;
                lcnt[w] = a | (b << 16);
            }
        }
        __syncthreads();
        // ---- (3) the postings, each at its place in LDS (the returning add leaves every counter at its cell's END)
        for (int64_t it = 0; it < trips; ++it) {
            const int64_t jb = c0 + (it * groups + (threadIdx.x >> 4)) * SG_POST_ROWS;
            int64_t lo[SG_POST_ROWS], hi[SG_POST_ROWS];
#pragma unroll
            for (int r = 0; r < SG_POST_ROWS; ++r) {
                const bool valid = jb + r < c1;
                lo[r] = valid ? chunk_base + rowp[jb + r - c0] : 0;
                hi[r] = valid ? chunk_base + rowp[jb + r - c0 + 1] : 0;
            }
            // the lane's first two entries of every row (a row's first 32): all loads before the first use
            int32_t k0[SG_POST_ROWS], k1[SG_POST_ROWS];
            T v0[SG_POST_ROWS], v1[SG_POST_ROWS];
#pragma unroll
            for (int r = 0; r < SG_POST_ROWS; ++r) {
                const bool have = lo[r] + sub < hi[r], more = lo[r] + sub + 16 < hi[r];
                k0[r] = have ? indices[lo[r] + sub] : -1;
                v0[r] = have ? data[lo[r] + sub] : (T)0;
                k1[r] = more ? indices[lo[r] + sub + 16] : -1;
                v1[r] = more ? data[lo[r] + sub + 16] : (T)0;
            }
#pragma unroll
            for (int r = 0; r < SG_POST_ROWS; ++r) {
                // norm of the row's frequent part relative to norm_up, rounded up (the order of the additions is free: the
                // result is rounded up with a margin far above the rounding of a double sum)
                double f2 = 0.0;
                if (k0[r] >= 0 && ((freq_bits[k0[r] >> 5] >> (k0[r] & 31)) & 1u)) f2 = (double)v0[r] * (double)v0[r];
                if (k1[r] >= 0 && ((freq_bits[k1[r] >> 5] >> (k1[r] & 31)) & 1u)) f2 += (double)v1[r] * (double)v1[r];
                for (int64_t p = lo[r] + sub + 32; p < hi[r]; p += 16) {
                    const int32_t k = indices[p];
                    if ((freq_bits[k >> 5] >> (k & 31)) & 1u) f2 += (double)data[p] * (double)data[p];
                }
#pragma unroll
                for (int d = 8; d > 0; d >>= 1) {
                    const uint64_t bits = (uint64_t)__double_as_longlong(f2);
                    const uint32_t l = (uint32_t)__shfl_xor((int)(uint32_t)bits, d, 64), h = (uint32_t)__shfl_xor((int)(uint32_t)(bits >> 32), d, 64);
                    f2 += __longlong_as_double((long long)(((uint64_t)h << 32) | l));
                }
                const float fq = frequent_norm_ratio_of(f2, inv_norm_up);
                const uint32_t col = (uint32_t)(jb + r - (t << tile_log2));
                if (k0[r] >= 0) {
                    const uint32_t sh = ((uint32_t)k0[r] & 1u) << 4;
                    const uint32_t pos = (atomicAdd(&lcnt[(uint32_t)k0[r] >> 1], 1u << sh) >> sh) & 0xffffu;
                    stage[pos] = filter_posting(col, (float)v0[r], fq, tile_log2, inv_norm_up, (uint32_t)t, fold_log2);
                    sterm[pos] = (uint16_t)k0[r];
                }
                if (k1[r] >= 0) {
                    const uint32_t sh = ((uint32_t)k1[r] & 1u) << 4;
                    const uint32_t pos = (atomicAdd(&lcnt[(uint32_t)k1[r] >> 1], 1u << sh) >> sh) & 0xffffu;
                    stage[pos] = filter_posting(col, (float)v1[r], fq, tile_log2, inv_norm_up, (uint32_t)t, fold_log2);
                    sterm[pos] = (uint16_t)k1[r];
                }
                for (int64_t p = lo[r] + sub + 32; p < hi[r]; p += 16) {
                    const uint32_t k = (uint32_t)indices[p];
                    const uint32_t sh = (k & 1u) << 4;
                    const uint32_t pos = (atomicAdd(&lcnt[k >> 1], 1u << sh) >> sh) & 0xffffu;
                    stage[pos] = filter_posting(col, (float)data[p], fq, tile_log2, inv_norm_up, (uint32_t)t, fold_log2);
                    sterm[pos] = (uint16_t)k;
                }
            }
        }
        __syncthreads();
        // ---- (4) out: a wave takes 64 consecutive staged postings a trip, EIGHT trips with their loads (the heads' cell
        // starts: a round trip to the L2) issued before the first is copied
        {
            constexpr int FB = 8;
            const uint32_t stride = (uint32_t)blockDim.x;           // postings all waves take in one trip
            for (uint32_t e0 = (uint32_t)wave * 64u; e0 < tot; e0 += stride * FB) {
                uint32_t delta[FB];
                bool head[FB];
#pragma unroll
                for (int b = 0; b < FB; ++b) {
                    const uint32_t e = e0 + (uint32_t)b * stride + (uint32_t)lane;
                    const uint32_t k = e < tot ? (uint32_t)sterm[e] : 0xffffffffu;
                    const uint32_t before = (uint32_t)__shfl_up((int)k, 1, 64);
                    head[b] = e < tot && (lane == 0 || k != before);
                    delta[b] = 0u;
                    if (head[b]) {   // index position of staged posting e' of this cell = delta + e'
                        const uint32_t start = k == 0u ? 0u : lds_get16(lcnt, k - 1u);
                        delta[b] = term_start[k] + mine[k] - start;
                    }
                }
#pragma unroll
                for (int b = 0; b < FB; ++b) {
                    const uint32_t e = e0 + (uint32_t)b * stride + (uint32_t)lane;
                    const uint64_t heads = __ballot(head[b]) & (~0ull >> (63 - lane));      // heads at or below this lane
                    const int src = heads ? 63 - __builtin_clzll(heads) : 0;
                    const uint32_t d = (uint32_t)__shfl((int)delta[b], src, 64);
                    if (e < tot) out_filt[d + e] = stage[e];
                }
            }
        }
        __syncthreads();
        if (!one_chunk) {
            // the next chunk's cells start behind this one's: once a cell, by the lane that holds its first staged posting
            for (uint32_t e = threadIdx.x; e < tot; e += blockDim.x) {
                const uint32_t k = (uint32_t)sterm[e];
                const uint32_t start = k == 0u ? 0u : lds_get16(lcnt, k - 1u);
                if (e == start) mine[k] += lds_get16(lcnt, k) - start;
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(256) term_len_kernel(const uint32_t *__restrict__ seg, int64_t n_terms, int32_t n_tiles,
                                                       uint32_t *__restrict__ term_len) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_terms) term_len[k] = seg[(k + 1) * n_tiles] - seg[k * n_tiles];
}

// Packed copy of B's rows for the pruned multiply (one 16-byte load = two f32 entries or one f64 entry): a thread per
// entry, and a thread per row for its {32-bit row pointer, the row's own index} -- the index rides with the pointer
// because the multiply needs both for every pair it scores: as a table of its own (orig_of[j]) it cost a cache line per
// pair, 4 GB of the kernel's 55 GB at 663 k.
template <typename T>
__global__ void __launch_bounds__(256) fwd_pack(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                const T *__restrict__ data, int64_t n_rows, int64_t nnz,
                                                const uint32_t *__restrict__ orig_of /* position -> row; null: identity */,
                                                uint32_t *__restrict__ fwd_ptr /* uint2 per row: {pointer, row} */, void *__restrict__ fwd) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t base = indptr[0];
    if (i <= n_rows)
        reinterpret_cast<uint2 *>(fwd_ptr)[i] = make_uint2((uint32_t)(indptr[i] - base), i < n_rows ? (orig_of ? orig_of[i] : (uint32_t)i) : 0u);
    if (i >= nnz || fwd == nullptr) return;   // (fwd null: the row blocks carry the rows, only the pointer table is made)
    const int64_t p = base + i;
    if (sizeof(T) == 4) {
        reinterpret_cast<int2 *>(fwd)[i] = make_int2(indices[p], __float_as_int((float)data[p]));
    } else {
        const long long bits = __double_as_longlong((double)data[p]);
        reinterpret_cast<int4 *>(fwd)[i] = make_int4(indices[p], 0, (int)(bits & 0xffffffffll), (int)(bits >> 32));
    }
}

// Row blocks for the exact scoring of the pruned multiply (SgScoreCtx::blk): one thread per 16-byte chunk of the
// 128-byte lines a row uses.
template <typename T>
__global__ void __launch_bounds__(256) row_blocks_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                         const T *__restrict__ data, int64_t n_rows,
                                                         const uint32_t *__restrict__ orig_of /* position -> row; null: identity */,
                                                         uint32_t blk_bytes, void *__restrict__ blk) {
    constexpr int ES = sizeof(T) == 4 ? 8 : 16;    // bytes of an entry
    const int64_t chunks = blk_bytes / 16;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = g / chunks;
    const int32_t c = (int32_t)(g - p * chunks);
    if (p >= n_rows) return;
    const int64_t lo = indptr[p];
    const int32_t nnz = (int32_t)(indptr[p + 1] - lo);
    const int32_t used = (((nnz + 1) * ES + 127) / 128) * 128;     // bytes of the lines the row uses
    if (c * 16 >= used) return;
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (sizeof(T) == 4) {   // two entries per chunk: 2c, 2c + 1 (entry 0 = header)
        const int32_t e0 = 2 * c, e1 = 2 * c + 1;
        if (e0 == 0) {
            w.x = orig_of ? orig_of[p] : (uint32_t)p;
            w.y = (uint32_t)nnz;
        } else if (e0 <= nnz) {
            w.x = (uint32_t)indices[lo + e0 - 1];
            w.y = __float_as_uint((float)data[lo + e0 - 1]);
        }
        if (e1 <= nnz) {
            w.z = (uint32_t)indices[lo + e1 - 1];
            w.w = __float_as_uint((float)data[lo + e1 - 1]);
        }
    } else {                // one entry per chunk
        if (c == 0) {
            w.x = orig_of ? orig_of[p] : (uint32_t)p;
            w.y = (uint32_t)nnz;
        } else if (c <= nnz) {
            const long long bits = __double_as_longlong((double)data[lo + c - 1]);
            w.x = (uint32_t)indices[lo + c - 1];
            w.z = (uint32_t)(bits & 0xffffffffll);
            w.w = (uint32_t)(bits >> 32);
        }
    }
    reinterpret_cast<uint4 *>(reinterpret_cast<char *>(blk) + (size_t)p * blk_bytes)[c] = w;
}

// (path with global counters) the two padded tables of segment ends from the term-major segment table: a thread per term
__global__ void __launch_bounds__(256) ends_from_seg_kernel(const uint32_t *__restrict__ seg, int64_t n_terms, int32_t n_tiles,
                                                            uint32_t *__restrict__ ends, int32_t nt_pad, uint32_t *__restrict__ ends8,
                                                            int32_t nv_pad, int32_t fold_log2) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n_terms) return;
    if (ends)
        for (int32_t t = 0; t < nt_pad; ++t)
            ends[k * nt_pad + t] = k == n_terms ? 0u : seg[k * n_tiles + (t < n_tiles ? t : n_tiles - 1) + 1] << 2;
    if (ends8)
        for (int32_t v = 0; v < nv_pad; ++v) {
            int64_t t = (int64_t)(v + 1) << fold_log2;   // first tile past super-tile v
            if (t > n_tiles) t = n_tiles;
            ends8[k * nv_pad + v] = k == n_terms ? 0u : seg[k * n_tiles + t] << 2;
        }
}

__global__ void __launch_bounds__(256) null_postings_kernel(uint32_t *__restrict__ slack) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // 512 entries
    slack[i] = sg_null_posting(i);
}

// ---- position space: a fixed permutation of the right-hand rows (see sg_postings in sg_internal.h)
// pos_of[j] = j * M mod n with gcd(M, n) = 1, M ~ 0.618 n: neighbours land 0.618 n apart and any run of rows spreads
// evenly over the positions (a low-discrepancy sequence) -- what a sorted list needs, and harmless on any other.
// Round 6: no launch of its own -- the prefix sum over the rows' lengths in position order (the row pointers of the matrix in
// position order) computes the permutation as it loads: position p holds row g = p * M^-1 mod n.
struct PermutedLenLoad {
    uint64_t n, minv, magic;       // magic = floor((2^64 - 1) / n) + 1: p * minv mod n by one multiply-high (a 64-bit `%` is ~100 instructions)
    const int32_t *len_of_row;     // lengths by row (groups: SgCollapse::d_rep_len); null: from the row pointers
    const int64_t *indptr;
    uint32_t *pos_of, *orig_of;
    __device__ __forceinline__ int64_t operator()(int64_t p) const {
        const uint64_t x = (uint64_t)p * minv;                    // < 2^62
        const uint64_t q = __umul64hi(x, magic);                  // floor(x / n) or one more
        int64_t rem = (int64_t)(x - q * n);
        if (rem < 0) rem += (int64_t)n;
        const uint32_t g = (uint32_t)rem;
        orig_of[p] = g;
        pos_of[g] = (uint32_t)p;
        return len_of_row ? (int64_t)len_of_row[g] : indptr[g + 1] - indptr[g];
    }
};

// ---- the 8-bit copies of the rows for the pruned multiply's SECOND filter (SgScoreCtx::q8, sg_internal.h; round 5)
// One 16-byte unit of a row's record: unit 0 = {first packed entry, the row's own index, entries | flag, 0}, unit u >= 1 =
// entries 4u - 4 .. 4u - 1; an entry is (term << 8) | bq with bq = ceil(value / norm_up * 255) -- UP: the factor 1.000002
// pays for the float roundings of the product (four of 2^-24), the cut at 255 is sound because no value exceeds its
// row's norm.  Units a row does not reach are neither written nor read.
__device__ __forceinline__ uint32_t sg_q8_units(int64_t nnz) {
    return nnz > (int64_t)SG_Q8_MAX_ENTRIES ? 1u : (uint32_t)((nnz + 7) >> 2);   // (the header + four entries a unit)
}
// The header's fourth word: four REST NORMS of the record (SgScoreCtx, sg_internal.h), a byte each -- the root of the sum of
// bq^2 over the entries behind unit SG_Q8_REST_UNIT(f), rounded UP, so that the second filter may bound what it has not
// read (Cauchy-Schwarz, q8_passes).  The sum is an integer (at most 60 * 255^2 < 2^22: exact in 32 bits, and exact as a
// float, whose root is then off by one at most); the root is settled in integers: the least r with r * r >= s.  A root of
// 255 or more is stored as SG_Q8_REST_UNKNOWN, which the reader takes for "no bound" -- as it takes every field of an
// index built with SG_Q8_EARLY=0 (`unknown` = all ones), the switch: no check can fire then.
__device__ __forceinline__ uint32_t q8_root_up(uint32_t s) {
    uint32_t r = (uint32_t)sqrtf((float)s);
    while (r * r < s) ++r;
    while (r > 0u && (r - 1u) * (r - 1u) >= s) --r;
    return r < SG_Q8_REST_UNKNOWN ? r : SG_Q8_REST_UNKNOWN;
}
__device__ __forceinline__ uint32_t q8_rest_word(const uint32_t (&sums)[4], uint32_t unknown) {
    return unknown | q8_root_up(sums[0]) | (q8_root_up(sums[1]) << 8) | (q8_root_up(sums[2]) << 16) | (q8_root_up(sums[3]) << 24);
}
template <typename T>
__device__ __forceinline__ void q8_write_unit(uint4 *__restrict__ rec, uint32_t u, const int32_t *__restrict__ indices,
                                              const T *__restrict__ data, int64_t src, int64_t nnz, uint32_t first_packed,
                                              uint32_t name, float inv_norm, uint32_t rest_unknown) {
    auto entry = [&](int64_t e) -> uint32_t {
        if (e >= nnz) return 0u;
        const float q = ceilf((float)data[src + e] * inv_norm * 255.0f * 1.000002f);
        const uint32_t bq = q >= 255.0f ? 255u : (q >= 1.0f ? (uint32_t)q : 1u);
        return ((uint32_t)indices[src + e] << 8) | bq;
    };
    uint4 w;
    if (u == 0) {
        const bool whole = nnz <= (int64_t)SG_Q8_MAX_ENTRIES;
        uint32_t sums[4] = {0u, 0u, 0u, 0u};
        for (int64_t e = 4 * (int64_t)SG_Q8_REST_UNIT(0); whole && e < nnz; ++e) {   // (from the first boundary on)
            const uint32_t bq = entry(e) & 255u;
#pragma unroll
            for (int f = 0; f < 4; ++f)
                if (e >= 4 * (int64_t)SG_Q8_REST_UNIT(f)) sums[f] += bq * bq;
        }
        w = make_uint4(first_packed, name, (uint32_t)nnz | (whole ? 0u : 0x80000000u), q8_rest_word(sums, whole ? rest_unknown : ~0u));
    } else {
        const int64_t e0 = 4 * (int64_t)u - 4;
        w = make_uint4(entry(e0), entry(e0 + 1), entry(e0 + 2), entry(e0 + 3));
    }
    rec[u] = w;
}

// (the index without a copy of the rows in position order -- SG_PERMUTE=0, few rows: sixteen lanes per row)
template <typename T>
__global__ void __launch_bounds__(256) q8_pack_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                      const T *__restrict__ data, int64_t n_rows,
                                                      const uint32_t *__restrict__ orig_of /* position -> row; null: identity */,
                                                      uint4 *__restrict__ q8, float inv_norm, uint32_t rest_unknown) {
    const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15;
    if (p >= n_rows) return;
    const int64_t base = indptr[0], src = indptr[p], n = indptr[p + 1] - src;
    if (sub < sg_q8_units(n))
        q8_write_unit<T>(q8 + p * (SG_Q8_STRIDE / 16), sub, indices, data, src, n, (uint32_t)(src - base),
                         orig_of ? orig_of[p] : (uint32_t)p, inv_norm, rest_unknown);
}

// ONE read of the source rows for every copy of them the index keeps (round 4).  Position p of the index holds row
// g = orig_of[p] of the matrix it is built over; with groups of identical rows that matrix is the representatives' -- row g
// = row rep_rows[g] of the caller's matrix -- and the copies are
//   * the matrix in position order (what the index and the self-join form read),
//   * its packed rows {term, value} + {pointer, row} per position (the exact scoring of the pruned multiply),
//   * the 8-bit records of the second filter.
// Round 6: (a) the representatives' matrix in GROUP order is no longer written here -- nothing on the self-join's way reads
// it (sg_csr_ensure_rows writes it for whoever does): 88 of 420 MB at 663 k; (b) where a row starts in the source and how
// long it is come from two arrays the grouping leaves per group (rep_start, rep_len): the chain position -> group ->
// representative -> row pointers -> entries was four dependent loads deep, now two; (c) TWO rows per sixteen lanes with all
// loads of a stage issued before the first is used, and a row's first 32 entries in flight together: the kernel ran at the
// latency of its chain (0.21 ms for 0.4 GB); (d) the 8-bit records are put together from the registers that hold the
// entries (four shuffles a round), not by reading the row a second time.
// The record's rest norms (q8_rest_word) are summed the same way: every lane adds the squares of its own entries behind each
// of the four boundaries, round by round, the sixteen lanes' sums are added once the whole row has been seen, and the header
// -- which therefore is the LAST unit written -- takes the word.
#ifndef SG_GATHER_ROWS     // (A/B knob of the build: scripts/build_variant.sh)
#define SG_GATHER_ROWS 2
#endif
template <typename T>
__device__ __forceinline__ uint32_t q8_entry_of(int32_t k, T v, bool have, float inv_norm) {
    if (!have) return 0u;
    const float q = ceilf((float)v * inv_norm * 255.0f * 1.000002f);
    const uint32_t bq = q >= 255.0f ? 255u : (q >= 1.0f ? (uint32_t)q : 1u);
    return ((uint32_t)k << 8) | bq;
}
// round r of a row (entries 16 r .. 16 r + 15, one per lane: wq) -> units 4 r + 1 .. 4 r + 4 of its record, written by the
// lanes of those numbers (unit u = entries 4 u - 4 .. 4 u - 1)
__device__ __forceinline__ void q8_write_round(uint4 *__restrict__ rec, int r, uint32_t wq, int sub, uint32_t units) {
    const int q = (sub - 4 * r - 1) & 3;
    const int base = (int)(threadIdx.x & 48u) + 4 * q;
    const uint32_t x0 = (uint32_t)__shfl((int)wq, base, 64), x1 = (uint32_t)__shfl((int)wq, base + 1, 64);
    const uint32_t x2 = (uint32_t)__shfl((int)wq, base + 2, 64), x3 = (uint32_t)__shfl((int)wq, base + 3, 64);
    if (sub >= 4 * r + 1 && sub <= 4 * r + 4 && (uint32_t)sub < units) rec[sub] = make_uint4(x0, x1, x2, x3);
}
template <typename T>
__device__ __forceinline__ void store_packed(void *__restrict__ fwd, int64_t at, int32_t k, T v) {
    if (sizeof(T) == 4) {
        reinterpret_cast<int2 *>(fwd)[at] = make_int2(k, __float_as_int((float)v));
    } else {
        const long long bits = __double_as_longlong((double)v);
        reinterpret_cast<int4 *>(fwd)[at] = make_int4(k, 0, (int)(bits & 0xffffffffll), (int)(bits >> 32));
    }
}
template <typename T>
__global__ void __launch_bounds__(256) gather_rows_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                          const T *__restrict__ data, int64_t n_rows,
                                                          const uint32_t *__restrict__ orig_of,
                                                          const uint32_t *__restrict__ rep_rows /* null: the source IS the matrix */,
                                                          const int64_t *__restrict__ rep_start /* null: from rep_rows / the row pointers */,
                                                          const int32_t *__restrict__ rep_len,
                                                          const int64_t *__restrict__ perm_ptr, int32_t *__restrict__ perm_indices,
                                                          T *__restrict__ perm_data,
                                                          uint32_t *__restrict__ fwd_ptr /* null: no packed rows */, void *__restrict__ fwd,
                                                          uint4 *__restrict__ q8 /* null: no 8-bit copies */, float inv_norm,
                                                          uint32_t rest_unknown /* all ones: SG_Q8_EARLY=0 */) {
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int sub = threadIdx.x & 15;
    const int64_t p0 = grp * SG_GATHER_ROWS;
    if (p0 > n_rows) return;
    bool valid[SG_GATHER_ROWS];
    uint32_t g[SG_GATHER_ROWS];
    int64_t src[SG_GATHER_ROWS], dst[SG_GATHER_ROWS];
    int32_t n[SG_GATHER_ROWS];
#pragma unroll
    for (int i = 0; i < SG_GATHER_ROWS; ++i) {
        valid[i] = p0 + i < n_rows;
        g[i] = valid[i] ? orig_of[p0 + i] : 0u;
        dst[i] = p0 + i <= n_rows ? perm_ptr[p0 + i] : 0;
    }
    if (rep_start) {
#pragma unroll
        for (int i = 0; i < SG_GATHER_ROWS; ++i) {
            src[i] = valid[i] ? rep_start[g[i]] : 0;
            n[i] = valid[i] ? rep_len[g[i]] : 0;
        }
    } else {
        int64_t j[SG_GATHER_ROWS];
#pragma unroll
        for (int i = 0; i < SG_GATHER_ROWS; ++i) j[i] = (valid[i] && rep_rows) ? (int64_t)rep_rows[g[i]] : (int64_t)g[i];
#pragma unroll
        for (int i = 0; i < SG_GATHER_ROWS; ++i) {
            src[i] = valid[i] ? indptr[j[i]] : 0;
            n[i] = valid[i] ? (int32_t)(indptr[j[i] + 1] - src[i]) : 0;
        }
    }
    // a row's first two rounds of entries: all loads before the first use
    int32_t k[SG_GATHER_ROWS][2];
    T v[SG_GATHER_ROWS][2];
#pragma unroll
    for (int i = 0; i < SG_GATHER_ROWS; ++i)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const bool have = sub + 16 * r < n[i];
            k[i][r] = have ? indices[src[i] + sub + 16 * r] : 0;
            v[i][r] = have ? data[src[i] + sub + 16 * r] : (T)0;
        }
#pragma unroll
    for (int i = 0; i < SG_GATHER_ROWS; ++i) {
        const int64_t p = p0 + i;
        if (p == n_rows) {     // the sentinel position behind the last row
            if (fwd_ptr && sub == 0) reinterpret_cast<uint2 *>(fwd_ptr)[p] = make_uint2((uint32_t)dst[i], 0u);
            // the exact scoring reads packed rows in rounds of eight entries and multiplies what lies past a row's end by a = 0:
            // the pad behind the LAST row must hold finite values (0 * NaN would poison that row's score)
            if (fwd && sub < 8) store_packed<T>(fwd, dst[i] + sub, 0, (T)0);
        }
        if (!valid[i]) continue;
        const uint32_t units = q8 ? sg_q8_units(n[i]) : 0u;
        uint4 *rec = q8 ? q8 + p * (SG_Q8_STRIDE / 16) : nullptr;
        if (sub == 0 && fwd_ptr) reinterpret_cast<uint2 *>(fwd_ptr)[p] = make_uint2((uint32_t)dst[i], g[i]);
        uint32_t rest[4] = {0u, 0u, 0u, 0u};   // this lane's share of the sums of bq^2 behind the four boundaries
        auto add_rest = [&](uint32_t wq, int32_t e) {
            const uint32_t bq = wq & 255u;
#pragma unroll
            for (int f = 0; f < 4; ++f)
                if (e >= 4 * (int32_t)SG_Q8_REST_UNIT(f)) rest[f] += bq * bq;
        };
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int32_t e = sub + 16 * r;
            const bool have = e < n[i];
            if (have) {
                perm_indices[dst[i] + e] = k[i][r];
                perm_data[dst[i] + e] = v[i][r];
                if (fwd) store_packed<T>(fwd, dst[i] + e, k[i][r], v[i][r]);
            }
            if (units > 1u && 16 * r < n[i]) {
                const uint32_t wq = q8_entry_of<T>(k[i][r], v[i][r], have, inv_norm);
                add_rest(wq, e);
                q8_write_round(rec, r, wq, sub, units);
            }
        }
        for (int r = 2; 16 * r < n[i]; ++r) {     // rows beyond 32 entries
            const int32_t e = sub + 16 * r;
            const bool have = e < n[i];
            const int32_t kk = have ? indices[src[i] + e] : 0;
            const T vv = have ? data[src[i] + e] : (T)0;
            if (have) {
                perm_indices[dst[i] + e] = kk;
                perm_data[dst[i] + e] = vv;
                if (fwd) store_packed<T>(fwd, dst[i] + e, kk, vv);
            }
            if (units > 1u && r < 4) {
                const uint32_t wq = q8_entry_of<T>(kk, vv, have, inv_norm);
                add_rest(wq, e);
                q8_write_round(rec, r, wq, sub, units);
            }
        }
        if (q8) {
            const bool whole = n[i] <= (int32_t)SG_Q8_MAX_ENTRIES;
            if (units > 1u) {   // (the same for the sixteen lanes of a row)
#pragma unroll
                for (int f = 0; f < 4; ++f)
#pragma unroll
                    for (int d = 1; d < 16; d <<= 1) rest[f] += (uint32_t)__shfl_xor((int)rest[f], d, 64);
            }
            if (sub == 0)
                rec[0] = make_uint4((uint32_t)dst[i], g[i], (uint32_t)n[i] | (whole ? 0u : 0x80000000u),
                                    q8_rest_word(rest, whole ? rest_unknown : ~0u));
        }
    }
}

// The rest norms of records that are already written, from the records themselves: the switch SG_Q8_EARLY holds for the
// multiplies that follow it, also over an index built before it was set (sg_postings_sync_q8_early) -- the two settings can
// then be compared on ONE index, posting for posting the same.  A thread a record; only the header's fourth word is written.
__global__ void __launch_bounds__(256) q8_rest_kernel(uint4 *__restrict__ q8, int64_t n_rows, uint32_t rest_unknown) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_rows) return;
    uint32_t *rec = reinterpret_cast<uint32_t *>(q8 + p * (SG_Q8_STRIDE / 16));
    const uint32_t word2 = rec[2], n = word2 & 0x7fffffffu;
    const bool whole = (word2 >> 31) == 0u && n <= SG_Q8_MAX_ENTRIES;
    uint32_t sums[4] = {0u, 0u, 0u, 0u};
    for (uint32_t e = 4u * SG_Q8_REST_UNIT(0); whole && rest_unknown == 0u && e < n; ++e) {
        const uint32_t bq = rec[4u + e] & 255u;
#pragma unroll
        for (int f = 0; f < 4; ++f)
            if (e >= 4u * SG_Q8_REST_UNIT(f)) sums[f] += bq * bq;
    }
    rec[3] = q8_rest_word(sums, whole ? rest_unknown : ~0u);
}

__global__ void score_ctx_kernel(SgScoreCtx v, SgScoreCtx *out) {
    out[0] = v;
    v.q8 = nullptr;          // [1]: the same without the second filter (the multiply chooses per call: sg_q8_applies)
    v.q8_scale = 0.f;
    out[1] = v;
}

// ------------------------------------------------------------------------------------------------
// Host side.  sg_postings_build_flags decides whether identical rows are grouped and hands the matrix to index -- the
// representatives' or the caller's -- to build_index, which reads as its stages: plan_build, alloc_early_rows,
// build_permuted, alloc_index, fill_lds_path or fill_global_path + tables_from_seg, pack_rows, write_aux.
struct PostingsFree {
    void operator()(sg_postings *p) const { sg_postings_free(p); }
};
using PostingsPtr = std::unique_ptr<sg_postings, PostingsFree>;   // a half-built index goes back whole, whichever way a stage fails

static SgScoreCtx score_ctx_of(const sg_postings *p) {
    SgScoreCtx sc;
    if (!p->d_fwd_ptr) return sc;
    sc.fwd_ptr = p->d_fwd_ptr;
    sc.fwd = p->d_fwd;
    sc.blk = p->d_blk;
    sc.blk_bytes = p->blk_bytes;
    sc.orig_of = p->d_orig_of;
    sc.q8 = (const uint4 *)p->d_q8;
    sc.q8_scale = p->d_q8 ? __builtin_nextafterf((float)(255.0 / (double)p->norm_up * (1.0 - 1e-6)), 0.f) : 0.f;
    return sc;
}

// SG_Q8_EARLY=0: the records' rest norms are all written as "unknown", so that the second filter reads every record to its
// end as it did before it had them (A/B and test hook; the multiply itself has one code path)
static uint32_t q8_rest_unknown(const sg_ctx *ctx) { return ctx->opt_is("SG_Q8_EARLY", '0') ? ~0u : 0u; }
int sg_postings_sync_q8_early(sg_ctx *ctx, const sg_postings *Bt) {
    const bool want = q8_rest_unknown(ctx) == 0u;
    if (!Bt->d_q8 || Bt->q8_early == want || Bt->n_right <= 0) return SG_OK;
    hipLaunchKernelGGL(q8_rest_kernel, dim3((unsigned)((Bt->n_right + 255) / 256)), dim3(256), 0, ctx->stream, (uint4 *)Bt->d_q8,
                       Bt->n_right, want ? 0u : ~0u);
    if (hipGetLastError() != hipSuccess) return SG_ERR_HIP;
    Bt->q8_early = want;
    return SG_OK;
}

// a tile's counters ([term], a workgroup's own) + one bit per term (frequent or not) in LDS
static size_t lds_counter_bytes(int64_t n_cols) { return (size_t)n_cols * 4 + ((size_t)(n_cols + 31) / 32) * 4; }

struct BuildPlan {   // everything the build decides before it allocates (plan_build); nothing below asks a second time
    bool cosine_like = false;
    float max_norm2 = 0.f;
    int32_t tile_cols = 0, tile_log2 = 0;
    int64_t n_tiles = 0, n_bins = 0;
    bool want_pruned = false, will_filter = false, want_q8 = false, want_blk = false;
    bool permute = false;          // a copy of the rows in position order may be made (build_permuted decides)
    bool early_rows = false;       // ... and it writes the packed rows and their 8-bit copies along
    bool lds_path = false, lazy_full = false;
    int32_t fold_log2 = 0, nt_pad = 0, nv_pad = 0;
    float norm_up = 0.f;
    uint32_t freq_min = 0;
    // the staged fill's geometry (LDS path)
    bool staged = false;
    int32_t chunk_rows = 0;
    uint32_t stage_cap = 0;        // entries a chunk may hold to be staged (SG_FILL_STAGE_CAP lowers it)
    uint32_t stage_alloc = 0;      // entries the stage has room for
    size_t staged_lds = 0;
    int32_t split = 1;
};

// ---- How many parts a tile is counted and filled in (staged fill).  Count and fill run one workgroup per part, and the fill's
// LDS lets ONE workgroup live on a CU.  Equal workgroups run in rounds of as many as are resident, and a round costs the same
// whether it is full or not: 544 parts on 256 CUs were three rounds for 2.1 rounds of work, the last on an eighth of the
// chip.  The model below prices every split and takes the cheapest:
//   a round of the fill   = per term and chunk (counters loaded or cleared, prefix sum, flags) + per posting of the part; a part
//                           of several chunks counts its rows itself: more per posting;
//   the table             = per cell of the [workgroup][term] table: the count pass writes it (and its packed copy), the
//                           column scan reads and writes it.  (The tables kernel reads one row a tile whatever the split,
//                           and the count pass's row work does not depend on the split: neither is priced.)
// The constants are microseconds on MI355X, fitted to the kernels' times under forced splits 3 .. 7 at 663 k names (136 tiles,
// 15 014 terms, 18.9 entries a row; profiles/postings_units_ab.log, where the fit is written out): fill 230 / 270 / 173 / 198 /
// 188 us measured, 229 / 270 / 172 / 201 / 187 by the model.  (Taken before the fill staged its row pointers and loaded 32
// entries of a row at once, which made it a tenth faster at split 5: the figures are high by about that much.)  They only
// have to rank the splits: a wrong choice costs time, never a result.
struct SplitCost {
    int32_t split = 1;
    int64_t parts = 0, part_rows = 0, chunks = 0, fill_rounds = 0;
    double fill_us = 0, table_us = 0, total_us = 0;
};
static constexpr double SG_SPLIT_US_PER_TERM_AND_CHUNK = 0.78e-3, SG_SPLIT_US_PER_POSTING = 2.9e-3, SG_SPLIT_US_PER_POSTING_RECOUNT = 0.53e-3,
                        SG_SPLIT_US_PER_CELL = 3.7e-6;
static constexpr int32_t SG_SPLIT_MAX = 16, SG_SPLIT_MIN_PART_ROWS = 512;
static SplitCost split_cost(int32_t split, int32_t tile_log2, int64_t n_tiles, int64_t n_terms, double mean_nnz, int32_t chunk_rows,
                            int32_t num_cu) {
    SplitCost c;
    c.split = split;
    c.parts = n_tiles * split;
    for (int32_t part = 0; part < split; ++part) {
        const int64_t rows = part_begin(part + 1, split, tile_log2) - part_begin(part, split, tile_log2);
        if (rows > c.part_rows) c.part_rows = rows;
    }
    const int64_t cus = num_cu > 0 ? num_cu : 1;
    c.fill_rounds = (c.parts + cus - 1) / cus;
    c.chunks = (c.part_rows + chunk_rows - 1) / chunk_rows;
    const double postings = (double)c.part_rows * mean_nnz;
    c.fill_us = (double)c.fill_rounds * ((double)c.chunks * SG_SPLIT_US_PER_TERM_AND_CHUNK * (double)n_terms +
                                         (SG_SPLIT_US_PER_POSTING + (c.chunks > 1 ? SG_SPLIT_US_PER_POSTING_RECOUNT : 0.0)) * postings);
    c.table_us = SG_SPLIT_US_PER_CELL * (double)c.parts * (double)n_terms;
    c.total_us = c.fill_us + c.table_us;
    return c;
}
static int32_t choose_split(sg_ctx *ctx, const BuildPlan &pl, int64_t n_terms, double mean_nnz) {
    SplitCost best;
    const bool say = ctx->opt_is("SG_POSTINGS_PLAN", '1');   // (the model's figures on stderr, for the logs under profiles/)
    for (int32_t s = 1; s <= SG_SPLIT_MAX; ++s) {
        if (s > 1 && (pl.tile_cols / s < SG_SPLIT_MIN_PART_ROWS || pl.n_bins * s + 1 >= ((int64_t)1 << 31))) break;
        const SplitCost c = split_cost(s, pl.tile_log2, pl.n_tiles, n_terms, mean_nnz, pl.chunk_rows, ctx->num_cu);
        if (say)
            fprintf(stderr, "sg postings plan: split %d: %lld parts of <= %lld rows (%lld chunks), %lld rounds of the fill, us fill %.1f table %.1f = %.1f\n",
                    s, (long long)c.parts, (long long)c.part_rows, (long long)c.chunks, (long long)c.fill_rounds, c.fill_us, c.table_us, c.total_us);
        if (s == 1 || c.total_us < best.total_us) best = c;
    }
    if (say) fprintf(stderr, "sg postings plan: chosen split %d (%lld tiles, %lld terms, chunks of %d rows)\n", best.split, (long long)pl.n_tiles,
                     (long long)n_terms, pl.chunk_rows);
    return best.split;
}

static int plan_build(sg_ctx *ctx, const sg_csr *B, int32_t tile_cols, int32_t flags, bool cosine_like, float max_norm2,
                      BuildPlan *out) {
    BuildPlan pl;
    pl.cosine_like = cosine_like;
    pl.max_norm2 = max_norm2;
    // cosine-like right-hand sides (non-negative, sorted rows, norms <= 1: TF-IDF) take the pruned multiply,
    // whose 16-bit accumulators make a 4096-column tile 8 KiB; everything else the exact kernel with 8 KiB
    // of float / double accumulators per wave
    pl.want_pruned = cosine_like && !ctx->opt_is("SG_PRUNE", '0') && !(flags & SG_POSTINGS_EXACT_ONLY);
    if (tile_cols == 0) {
        tile_cols = B->dtype == SG_F64 ? 1024 : 2048;
        if (pl.want_pruned) {
            tile_cols = 4096;
            if (flags & SG_POSTINGS_TILE_FORM) tile_cols = 2048;   // (the tile-by-tile form's own index: sg_spgemm_topn.hip, "which form")
            else if (const char *v = ctx->opt("SG_PRUNE_TILE")) tile_cols = atoi(v) == 13 ? 8192 : (atoi(v) == 11 ? 2048 : 4096);
        }
    }
    SG_REQUIRE(tile_cols >= 256 && tile_cols <= 32768 && (tile_cols & (tile_cols - 1)) == 0,
               "tile_cols must be a power of two in [256, 32768]");
    pl.tile_cols = tile_cols;
    int64_t max_entries = (int64_t)1 << 29;   // the multiply addresses postings with 32-bit BYTE offsets (8 B entries)
    if (const char *v = ctx->opt("SG_MAX_POSTINGS")) {   // test hook: force the right-hand split at small sizes
        const long long o = atoll(v);
        if (o > 0 && o < max_entries) max_entries = o;
    }
    if (B->nnz + 64 >= max_entries) {
        sg_set_error("right-hand matrix has %lld non-zeros; one postings block holds < 2^29 (use more right-hand blocks)",
                     (long long)B->nnz);
        return SG_ERR_OVERFLOW;
    }
    while ((1 << pl.tile_log2) < tile_cols) ++pl.tile_log2;
    pl.n_tiles = B->n_rows == 0 ? 1 : ((B->n_rows + tile_cols - 1) >> pl.tile_log2);
    pl.n_bins = B->n_cols * pl.n_tiles;
    if (pl.n_bins + 1 >= (int64_t)1 << 31) {
        sg_set_error("segment table of %lld x %lld entries is too large; use more right-hand blocks",
                     (long long)B->n_cols, (long long)pl.n_tiles);
        return SG_ERR_OVERFLOW;
    }
    pl.norm_up = __builtin_nextafterf(sqrtf(max_norm2) * 1.000001f, 2.f);
    // second filter: terms must fit 24 bits; a sixteenth of the device memory at most; SG_Q8=0 switches it off
    // ... and rows of a name list's length: the filter walks the candidate's entries like the exact scoring does and saves its
    // memory round trips -- on rows of 60 entries (a record of two lines, fifteen units) it costs more than it saves (100 k
    // long names, SG_Q8 = 1 / 0: 8.9 / 5.8 ms; profiles/r05_family_sweep_q8.log).  SG_Q8=1 forces it for any length.
    // Where the bar lies (round 6, scripts/q8_band_sweep.py, profiles/r06b_q8_band_sweep.log: 100 k rows cut to 16 .. 57 entries a
    // row): with the records is the faster up to 45 entries a row (by 3 - 30 %), level at 50, and 50 - 75 % slower at 57 (rows
    // beyond 60 entries have no copy and pass unseen, a record of two lines costs fifteen units) -- 40 in round 5, 45 now.
    const bool q8_forced = ctx->opt_is("SG_Q8", '1');
    pl.want_q8 = pl.want_pruned && !(flags & SG_POSTINGS_TILE_FORM) && B->n_cols < ((int64_t)1 << 24) && !ctx->opt_is("SG_Q8", '0') &&
                 (q8_forced || (double)B->nnz <= 45.0 * (double)B->n_rows) &&
                 (ctx->total_mem == 0 || (size_t)SG_Q8_STRIDE * ((size_t)B->n_rows + 1) < ctx->total_mem / 16);
    pl.will_filter = pl.want_pruned && sg_pruned_supports_tile(pl.tile_log2) &&
                     (B->n_cols + 1) * ((pl.n_tiles + 3) & ~(int64_t)3) < ((int64_t)1 << 30);
    // rows at a fixed stride for the exact scoring (opt-in; what it takes and what it costs: row_block_bytes)
    pl.want_blk = ctx->opt_is("SG_ROW_BLOCKS", '1');
    pl.permute = !(flags & SG_POSTINGS_NO_PERMUTATION);
    pl.early_rows = pl.will_filter && !pl.want_blk && pl.permute && B->n_rows > 0;
    // The postings proper ({accumulator slot, value}: 8 bytes each, 100 MB at 663 k) are what the EXACT kernel streams.  When
    // the pruned multiply will take the product they are only needed for the rows it hands over (wider than 128 non-zeros
    // ...: none in a list of names), and scattering them is half of the index build: they are then written on demand
    // (sg_postings_ensure_full), from the same segment table.
    // the tile's counters fit in LDS: one workgroup per tile (part), LDS atomics (otherwise global ones)
    pl.lds_path = B->n_rows > 0 && lds_counter_bytes(B->n_cols) <= 124 * 1024 && B->n_cols > 0;
    if (const char *e = ctx->opt("SG_POSTINGS_LDS")) pl.lds_path = pl.lds_path && e[0] != '0';
    pl.lazy_full = pl.will_filter && pl.lds_path && !ctx->opt_is("SG_POSTINGS_LAZY", '0');
    if (pl.will_filter) {
        pl.nt_pad = (int32_t)((pl.n_tiles + 3) & ~(int64_t)3);
        // stream form of the pruned multiply (sg_spgemm_pruned.hip): eight tiles share one accumulator tile
        if (pl.tile_log2 == 12 && !ctx->opt_is("SG_K4_STREAM", '0')) pl.fold_log2 = 3;
        if (pl.fold_log2 > 0) {
            const int64_t n_super = (pl.n_tiles + ((int64_t)1 << pl.fold_log2) - 1) >> pl.fold_log2;
            pl.nv_pad = (int32_t)((n_super + 3) & ~(int64_t)3);
        }
        // a term is "frequent" when it occurs in at least this share of the right-hand rows: the suffix of a
        // left row is drawn from frequent terms only, which lets the survivor test use each candidate's own
        // frequent-part norm instead of 1 (profiles/r01_prune_tuning.log)
        double frac = 0.005;   // (round 5, with the second filter: 0.0045 -> 0.005, 30.8 M -> 22.5 M candidates, kernel - 2 % at 663 k; 0.004 + 5 %, 0.007 + 4 %)
        if (const char *v = ctx->opt("SG_PRUNE_FREQ")) frac = atof(v);
        const double fm = frac * (double)B->n_rows;
        pl.freq_min = fm < 1.0 ? 1u : (uint32_t)fm;
    }
    if (pl.lds_path) {
        // Filter postings staged in LDS and written cell by cell (postings_fill_staged) -- when only the filter postings are
        // written (the exact kernel's are lazy) and a chunk of at least 64 rows fits the stage.  The stage -- six bytes a
        // posting: the posting and its term -- takes what the packed counters leave of 158 KiB: one workgroup per CU.  A
        // chunk is as many rows (a multiple of 64, 2048 at most) as fit it at 1.2 x the mean row, and choose_split then
        // looks for parts that are ONE chunk and whose rounds fill the chip.
        pl.staged = pl.lazy_full && !ctx->opt_is("SG_FILL_STAGED", '0') && B->n_cols <= 65535;
        const double mean_nnz = B->n_rows > 0 ? (double)B->nnz / (double)B->n_rows : 1.0;
        if (pl.staged) {
            const size_t fixed0 = ((((size_t)B->n_cols + 1) / 2 + 3) & ~(size_t)3) * 4 + (((size_t)B->n_cols + 31) / 32) * 4 + 32 * 4;
            const size_t room = fixed0 + 16384 < 158 * 1024 ? 158 * 1024 - fixed0 : 0;
            // rows r of a chunk: 6 bytes a posting for r x 1.2 x the mean row + 64 postings, 4 bytes a row pointer
            const double per_row = (mean_nnz * 1.2 > 1.0 ? mean_nnz * 1.2 : 1.0) * 6.0 + 4.0;
            const double fit = ((double)room - 64.0 * 6.0 - 32.0) / per_row;
            pl.chunk_rows = fit >= 2048.0 ? 2048 : (fit > 0.0 ? (int32_t)fit & ~63 : 0);
            pl.staged = pl.chunk_rows >= 64;
            const size_t rowp_bytes = (size_t)staged_rowp_words(pl.chunk_rows) * 4;
            pl.stage_alloc = pl.staged ? (uint32_t)((room - rowp_bytes) / 6) & ~1u : 0u;
            if (pl.stage_alloc > 65534u) pl.stage_alloc = 65534u;
            pl.stage_cap = pl.stage_alloc;
            pl.staged_lds = fixed0 + rowp_bytes + (size_t)pl.stage_alloc * 6;
            if (const char *v = ctx->opt("SG_FILL_STAGE_CAP"))    // test hook: chunks that do not fit go posting by posting
                if (atoi(v) > 0 && (uint32_t)atoi(v) < pl.stage_cap) pl.stage_cap = (uint32_t)atoi(v);
        }
        int32_t split = 1;
        if (pl.staged) {
            split = choose_split(ctx, pl, B->n_cols, mean_nnz);
        } else {
            // fewer tiles than CUs: split every tile between 2 or 4 workgroups (parts of >= 1024 rows)
            while (split < 4 && pl.n_tiles * split < ctx->num_cu && (tile_cols / (split * 2)) >= 1024 &&
                   (pl.n_bins * split * 2 + 1) < ((int64_t)1 << 31))
                split *= 2;
        }
        if (const char *e = ctx->opt("SG_POSTINGS_SPLIT")) {   // test and A/B hook: any number of parts up to SG_SPLIT_MAX
            const int o = atoi(e);
            if (o >= 1 && o <= SG_SPLIT_MAX && tile_cols / o >= 64 && pl.n_bins * o + 1 < ((int64_t)1 << 31)) split = o;
        }
        pl.split = split;
    }
    *out = pl;
    return SG_OK;
}

// the packed rows of the pruned multiply are written by the same pass that copies the rows into position order
// ... and so are the 8-bit copies of the second filter
struct EarlyRows {
    void *fwd = nullptr;
    uint32_t *fwd_ptr = nullptr;
    void *q8 = nullptr;
    bool written = false;   // build_permuted made the copy and filled them
};

static int alloc_early_rows(Scratch &early, const sg_csr *B, const BuildPlan &plan, EarlyRows *rows) {
    if (!plan.early_rows) return SG_OK;
    SG_TRY(early.alloc_bytes(((size_t)B->nnz + 8) * (B->dtype == SG_F64 ? 16 : 8), &rows->fwd));
    SG_TRY(early.alloc(2 * ((size_t)B->n_rows + 2), &rows->fwd_ptr));
    if (plan.want_q8) SG_TRY(early.alloc_bytes((size_t)SG_Q8_STRIDE * ((size_t)B->n_rows + 1), &rows->q8));
    return SG_OK;
}

static uint64_t gcd_u64(uint64_t a, uint64_t b) {
    while (b) {
        const uint64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// B with its rows in position order + the two tables, into p; p->permuted stays null when the permutation is off or pointless
static int build_permuted(sg_ctx *ctx, const sg_csr *B, int64_t tile_cols, sg_postings *p,
                          SgCollapse *pending /* B = pending->unique, its rows not written yet; or null */,
                          EarlyRows *rows /* packed rows and 8-bit copies to write along (null members: none) */, float inv_norm) {
    const uint32_t rest_unknown = q8_rest_unknown(ctx);
    if (ctx->opt_is("SG_PERMUTE", '0') || B->n_rows <= 2 * tile_cols || B->n_rows >= ((int64_t)1 << 31) || B->nnz <= 0) return SG_OK;
    const uint64_t n = (uint64_t)B->n_rows;
    uint64_t mult = (uint64_t)(0.6180339887498949 * (double)n) | 1ull;
    while (gcd_u64(mult, n) != 1) mult += 2;
    mult %= n;
    // position p holds row p * mult^-1 mod n (extended Euclid; n < 2^31)
    uint64_t minv = 0;
    {
        long long t0 = 0, t1 = 1, r0 = (long long)n, r1 = (long long)mult;
        while (r1 != 0) {
            const long long q = r0 / r1, t2 = t0 - q * t1, r2 = r0 - q * r1;
            t0 = t1;
            t1 = t2;
            r0 = r1;
            r1 = r2;
        }
        minv = (uint64_t)(t0 < 0 ? t0 + (long long)n : t0);
    }
    Scratch scratch(ctx);   // (the two tables are the index's once the copy exists)
    uint32_t *orig_of = nullptr, *pos_of = nullptr;
    CsrPtr m;               // B's rows in position order: same rows, same properties
    // the rows of B itself, or -- B the representatives' matrix of `pending`, not written -- of the matrix they come from
    const bool from_groups = pending && pending->pending_src;
    const bool by_group = from_groups && pending->d_rep_len != nullptr;   // (table path: start and length per group; else B's row pointers are there)
    SG_TRY(scratch.alloc((size_t)n + 1, &orig_of));
    SG_TRY(scratch.alloc((size_t)n + 1, &pos_of));
    SG_TRY(csr_alloc(ctx, B->n_rows, B->n_cols, B->nnz, B->dtype, CSR_SLACK_GATHER, &m));
    csr_inherit(m.get(), B, CsrDerived::permuted);
    int64_t *ptr = (int64_t *)m->d_indptr;
    int32_t *idx = (int32_t *)m->d_indices;
    void *val = (void *)m->d_data;
    SG_TRY(sg_scan_launch<int64_t>(ctx, PermutedLenLoad{n, minv, (uint64_t)(~0ull / n) + 1ull, by_group ? pending->d_rep_len : (const int32_t *)nullptr, B->d_indptr, pos_of, orig_of},
                                   SgScanStoreArray<int64_t>{ptr}, (int64_t)n, ptr + n));
    const unsigned grid = (unsigned)((((n + 1 + SG_GATHER_ROWS - 1) / SG_GATHER_ROWS) * 16 + 255) / 256);
    const sg_csr *src = from_groups ? pending->pending_src : B;
    const uint32_t *rep_rows = from_groups ? pending->d_rep_rows : nullptr;
    const int64_t *rep_start = by_group ? pending->d_rep_start : nullptr;
    const int32_t *rep_len = by_group ? pending->d_rep_len : nullptr;
    by_dtype(B->dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(gather_rows_kernel<T>, dim3(grid), dim3(256), 0, ctx->stream, src->d_indptr, src->d_indices,
                           (const T *)src->d_data, B->n_rows, (const uint32_t *)orig_of, rep_rows, rep_start, rep_len,
                           (const int64_t *)ptr, idx, (T *)val, rows->fwd_ptr, rows->fwd, (uint4 *)(rows->fwd_ptr ? rows->q8 : nullptr), inv_norm,
                           rest_unknown);
        return SG_OK;
    });
    if (hipGetLastError() != hipSuccess) return SG_ERR_HIP;
    rows->written = rows->fwd_ptr != nullptr;     // (the representatives' matrix in group order stays pending)
    p->permuted = m.release();
    p->d_orig_of = scratch.keep(orig_of);
    p->d_pos_of = scratch.keep(pos_of);
    return SG_OK;
}

// rows at a fixed stride for the exact scoring, when the longest row fits 1 KiB (127 entries f32 / 63 f64)
// (*out: the stride; 0: no blocks)
static int row_block_bytes(sg_ctx *ctx, const sg_csr *B, uint32_t *out) {
    *out = 0;
    uint32_t max_nnz = 0;
    bool cl = false;
    float n2 = 0.f;
    // the longest row is measured only for this (a vectoriser-made matrix, and what is derived from it, is known
    // to be cosine-like without a look: sg_csr_props)
    if (B->props_max_nnz == 0 && !B->d_props_words) B->props_state = 0;
    SG_TRY(sg_csr_props(ctx, B, &cl, &n2, &max_nnz));
    const size_t es = B->dtype == SG_F64 ? 16 : 8;
    const size_t need = (((size_t)max_nnz + 1) * es + 127) / 128 * 128;
    // Opt-in (SG_ROW_BLOCKS=1): the blocks cut the memory-side traffic of the multiply by a fifth (57.9 -> 43 GB per
    // launch at 663 k) but not its time -- the kernel is not bound by bytes -- and their scorer's extra loop
    // trips cost 0.3 - 0.7 ms (9.76 ms packed / 10.08 ms with 64-byte units / 10.50 ms with 32-byte units:
    // profiles/r03_row_blocks_ab.log); the index build pays 0.11 ms for them.
    if (need <= 1024 && (double)need * (double)B->n_rows < 3.5e9 &&
        (ctx->total_mem == 0 || need * (size_t)B->n_rows < ctx->total_mem / 8))
        *out = (uint32_t)need;
    return SG_OK;
}

// the fields of the index and every array that lives as long as it does (B: the rows in position order, or B_in itself)
static int alloc_index(sg_ctx *ctx, sg_postings *p, const sg_csr *B_in, const sg_csr *B, const BuildPlan &plan, int32_t flags,
                       Scratch &early, EarlyRows *rows) {
    p->n_right = B->n_rows;
    p->n_terms = B->n_cols;
    p->nnz = B->nnz;
    p->dtype = B->dtype;
    p->tile_log2 = plan.tile_log2;
    p->tile_form = (flags & SG_POSTINGS_TILE_FORM) != 0;
    p->built_from = csr_view(*B_in);
    p->built_from_valid = true;
    p->n_tiles = (int32_t)plan.n_tiles;
    p->b_indptr = B_in->d_indptr;      // the caller's matrix: what "A is the matrix the postings were built from" compares
    p->b_indices = B_in->d_indices;
    p->b_data = B_in->d_data;
    p->cosine_like = plan.cosine_like;
    p->max_norm2 = plan.max_norm2;
    p->src = csr_view(*B);
    p->split = plan.split;
    const size_t vs = 8;   // f64 value, or packed {row, f32 value}
    SG_TRY(sg_alloc(ctx, (size_t)plan.n_bins + 1, &p->d_seg));
    SG_TRY(sg_alloc(ctx, (size_t)B->n_cols + 1, &p->d_term_len));
    if (!plan.lazy_full && B->dtype == SG_F64) SG_TRY(sg_alloc(ctx, (size_t)B->nnz + 64, &p->d_rows));
    if (!plan.lazy_full) SG_TRY(ctx->alloc(((size_t)B->nnz + 64) * vs, &p->d_vals));
    if (!plan.will_filter) return SG_OK;
    if (plan.want_blk) {
        SG_TRY(row_block_bytes(ctx, B, &p->blk_bytes));
        if (p->blk_bytes) SG_TRY(ctx->alloc((size_t)p->blk_bytes * ((size_t)B->n_rows + 1), &p->d_blk));
    }
    p->q8_early = q8_rest_unknown(ctx) == 0u;   // (what either record writer of this build stores)
    if (rows->written) {          // written along with the rows' copy in position order (build_permuted)
        p->d_fwd = early.keep(rows->fwd);
        p->d_fwd_ptr = early.keep(rows->fwd_ptr);
        p->d_q8 = early.keep(rows->q8);
    } else {
        if (!p->d_blk) SG_TRY(ctx->alloc(((size_t)B->nnz + 8) * (B->dtype == SG_F64 ? 16 : 8), &p->d_fwd));
        SG_TRY(sg_alloc(ctx, 2 * ((size_t)B->n_rows + 2), &p->d_fwd_ptr));   // uint2 per row
        if (plan.want_q8 && !p->d_blk) SG_TRY(ctx->alloc((size_t)SG_Q8_STRIDE * ((size_t)B->n_rows + 1), &p->d_q8));
    }
    // slack: the pruned multiply loads a lane's four slots of a segment unconditionally (<= 4 * 63 entries past it)
    SG_TRY(sg_alloc(ctx, (size_t)B->nnz + 512, &p->d_filt));
    // the stream form points lanes without a posting at the slack behind the array: entries that add 0 (bq = 0), each to
    // an accumulator of its own (64 lanes adding to ONE LDS word are serialised: 3 ms at 663 k)
    // (written by postings_tables_kernel on the LDS build path, by a launch of its own otherwise: below)
    p->nt_pad = plan.nt_pad;
    SG_TRY(sg_alloc(ctx, (size_t)(B->n_cols + 1) * (size_t)p->nt_pad + 4, &p->d_ends));
    p->fold_log2 = plan.fold_log2;
    p->nv_pad = plan.nv_pad;
    if (p->fold_log2 > 0) SG_TRY(sg_alloc(ctx, (size_t)(B->n_cols + 1) * (size_t)p->nv_pad + 4, &p->d_ends8));
    p->norm_up = plan.norm_up;
    p->freq_min = plan.freq_min;
    return SG_OK;
}

// LDS path: count -> column scan -> fill over the rows of p->src, one workgroup per tile (part).  The build makes the terms'
// list lengths, their frequent flags and the lists' starts on the way and writes the filter postings too; `values_only`
// (sg_postings_ensure_full) re-reads the starts and writes the postings proper alone.
static int lds_count_scan_fill(sg_ctx *ctx, sg_postings *p, uint32_t *cnt /* [workgroup][term] (see postings_count_lds) */,
                               uint32_t *cnt16 /* the parts' own counts, packed, for the staged fill; or null */,
                               uint32_t *term_len, uint8_t *is_frequent, bool values_only, bool fill) {
    const sg_csr *B = &p->src;
    const int32_t split = p->split > 0 ? p->split : 1;
    const int64_t wgs64 = (int64_t)p->n_tiles * split;
    const unsigned wgs = (unsigned)wgs64;
    const size_t lds = lds_counter_bytes(B->n_cols);
    uint32_t *filt = values_only ? nullptr : p->d_filt;
    const float inv_norm = filt ? 1.0f / p->norm_up : 0.f;
    const int32_t fold_log2 = values_only ? 0 : p->fold_log2;
    SG_TRY(allow_dynamic_lds<postings_count_lds>(124 * 1024));
    hipLaunchKernelGGL(postings_count_lds, dim3(wgs), dim3(1024), (size_t)B->n_cols * 4, ctx->stream, B->d_indptr, B->d_indices,
                       B->n_rows, p->tile_log2, (int32_t)B->n_cols, split, cnt, cnt16);
    hipLaunchKernelGGL(postings_colscan_kernel, dim3((unsigned)((B->n_cols + 63) / 64)), dim3(1024), 0, ctx->stream, cnt,
                       (int32_t)wgs64, (int32_t)B->n_cols, values_only ? 0u : p->freq_min, term_len, is_frequent);
    // the terms' lists back to back: starts of the lists, the last entry receives the total (= nnz)
    if (!values_only) SG_TRY(sg_exclusive_scan_u32(ctx, term_len, p->d_term_start, B->n_cols, p->d_term_start + B->n_cols));
    if (fill)
        SG_TRY(by_dtype(B->dtype, [&](auto tag) -> int {
            using T = decltype(tag);
            constexpr auto kern = postings_fill_lds<T>;
            SG_TRY(allow_dynamic_lds<kern>(124 * 1024));
            hipLaunchKernelGGL(kern, dim3(wgs), dim3(1024), lds, ctx->stream, B->d_indptr, B->d_indices,
                               (const T *)B->d_data, B->n_rows, p->tile_log2, (int32_t)B->n_cols, split, (const uint32_t *)cnt,
                               (const uint32_t *)p->d_term_start, (const uint8_t *)is_frequent, p->d_rows, (T *)p->d_vals, filt,
                               inv_norm, fold_log2);
            return SG_OK;
        }));
    return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

static int fill_lds_path(sg_ctx *ctx, sg_postings *p, const BuildPlan &plan) {
    const sg_csr *B = &p->src;
    const unsigned wgs = (unsigned)((int64_t)p->n_tiles * plan.split);
    Scratch scratch(ctx);
    uint32_t *cnt = nullptr, *cnt16 = nullptr;
    uint8_t *is_frequent = nullptr;
    SG_TRY(scratch.alloc((size_t)((int64_t)p->n_tiles * plan.split * B->n_cols) + 1, &cnt));
    if (plan.staged) SG_TRY(scratch.alloc((size_t)((int64_t)p->n_tiles * plan.split * ((B->n_cols + 1) / 2)) + 1, &cnt16));
    SG_TRY(scratch.alloc((size_t)B->n_cols + 4, &is_frequent));
    SG_TRY(sg_alloc(ctx, (size_t)B->n_cols + 2, &p->d_term_start));
    // (the staged fill comes after the tables: a part of several chunks advances its workgroup's row of `cnt`)
    SG_TRY(lds_count_scan_fill(ctx, p, cnt, cnt16, p->d_term_len, is_frequent, /*values_only=*/false, /*fill=*/!plan.staged));
    // the tables kernel writes the null postings and the scoring context as well (write_aux has them on the other path)
    if (p->d_fwd_ptr) SG_TRY(ctx->alloc(256, (void **)&p->d_score_ctx));
    hipLaunchKernelGGL(postings_tables_kernel, dim3((unsigned)((B->n_cols + 64) / 64)), dim3(1024), 0, ctx->stream, (const uint32_t *)cnt,
                       (const uint32_t *)p->d_term_start, (int32_t)B->n_cols, p->n_tiles, plan.split, p->d_seg, p->d_ends,
                       p->nt_pad, p->d_ends8, p->nv_pad, p->fold_log2, score_ctx_of(p), p->d_score_ctx,
                       p->d_filt ? p->d_filt + B->nnz : (uint32_t *)nullptr);
    if (plan.staged)
        SG_TRY(by_dtype(B->dtype, [&](auto tag) -> int {
            using T = decltype(tag);
            constexpr auto kern = postings_fill_staged<T>;
            SG_TRY(allow_dynamic_lds<kern>(160 * 1024));
            hipLaunchKernelGGL(kern, dim3(wgs), dim3(1024), plan.staged_lds, ctx->stream, B->d_indptr,
                               B->d_indices, (const T *)B->d_data, B->n_rows, p->tile_log2, (int32_t)B->n_cols, plan.split,
                               plan.chunk_rows, plan.stage_cap, plan.stage_alloc, cnt, (const uint32_t *)cnt16,
                               (const uint32_t *)p->d_term_start, (const uint8_t *)is_frequent,
                               p->d_filt, 1.0f / p->norm_up, p->fold_log2);
            return SG_OK;
        }));
    return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

// the counters do not fit in LDS: global ones, one thread per row
static int fill_global_path(sg_ctx *ctx, sg_postings *p, const BuildPlan &plan) {
    const sg_csr *B = &p->src;
    const int64_t n_bins = plan.n_bins;
    // one thread per slot of the (tile x row-in-tile) grid: covers every row, see row_of_thread
    const unsigned grid = (unsigned)((((int64_t)p->n_tiles << p->tile_log2) + 255) / 256);
    const float inv_norm = p->d_filt ? 1.0f / p->norm_up : 0.f;
    Scratch scratch(ctx);
    uint32_t *cursor = nullptr;
    SG_TRY(scratch.alloc((size_t)n_bins + 1, &cursor));
    SG_HIP_TRY(hipMemsetAsync(p->d_seg, 0, sizeof(uint32_t) * (size_t)(n_bins + 1), ctx->stream));
    SG_HIP_TRY(hipMemsetAsync(cursor, 0, sizeof(uint32_t) * (size_t)(n_bins + 1), ctx->stream));
    if (grid > 0) {
        by_dtype(B->dtype, [&](auto tag) {
            using T = decltype(tag);
            hipLaunchKernelGGL(postings_count<T>, dim3(grid), dim3(256), 0, ctx->stream, B->d_indptr, B->d_indices, B->n_rows,
                               p->tile_log2, p->n_tiles, p->d_seg);
            return SG_OK;
        });
        SG_HIP_TRY(hipGetLastError());
    }
    // counts -> offsets, in place; seg[n_bins] receives the total (= nnz)
    SG_TRY(sg_exclusive_scan_u32(ctx, p->d_seg, p->d_seg, n_bins, p->d_seg + n_bins));
    if (grid > 0) {
        by_dtype(B->dtype, [&](auto tag) {
            using T = decltype(tag);
            hipLaunchKernelGGL(postings_fill<T>, dim3(grid), dim3(256), 0, ctx->stream, B->d_indptr, B->d_indices,
                               (const T *)B->d_data, B->n_rows, p->tile_log2, p->n_tiles, p->d_seg, cursor, p->d_rows,
                               (T *)p->d_vals, p->d_filt, p->freq_min, inv_norm, p->fold_log2);
            return SG_OK;
        });
        if (hipGetLastError() != hipSuccess) return SG_ERR_HIP;
    }
    return SG_OK;
}

// (the path with global counters builds the term-major table itself; lists and ends are read off it)
static int tables_from_seg(sg_ctx *ctx, sg_postings *p) {
    if (p->n_terms <= 0) return SG_OK;
    hipLaunchKernelGGL(term_len_kernel, dim3((unsigned)((p->n_terms + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const uint32_t *)p->d_seg, p->n_terms, p->n_tiles, p->d_term_len);
    if (p->d_ends || p->d_ends8)
        hipLaunchKernelGGL(ends_from_seg_kernel, dim3((unsigned)((p->n_terms + 256) / 256)), dim3(256), 0, ctx->stream,
                           (const uint32_t *)p->d_seg, p->n_terms, p->n_tiles, p->d_ends, p->nt_pad, p->d_ends8, p->nv_pad,
                           p->fold_log2);
    return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

// the rows as the pruned multiply's exact scoring reads them -- unless the copy into position order wrote them already
static int pack_rows(sg_ctx *ctx, sg_postings *p, bool rows_written) {
    const sg_csr *B = &p->src;
    if (p->d_fwd && !rows_written) {   // (packed rows in use: no row blocks; the fused pass writes the pad itself)
        // the exact scoring reads packed rows in rounds of eight entries and multiplies the slots past a row's end by
        // a = 0: the pad behind the LAST row must hold finite values (0 * NaN would poison that row's score)
        const size_t es = B->dtype == SG_F64 ? 16 : 8;
        if (hipMemsetAsync((char *)p->d_fwd + (size_t)B->nnz * es, 0, 8 * es, ctx->stream) != hipSuccess) return SG_ERR_HIP;
    }
    if (p->d_blk && B->n_rows > 0) {
        const int64_t work = B->n_rows * (int64_t)(p->blk_bytes / 16);
        const unsigned g3 = (unsigned)((work + 255) / 256);
        by_dtype(B->dtype, [&](auto tag) {
            using T = decltype(tag);
            hipLaunchKernelGGL(row_blocks_kernel<T>, dim3(g3), dim3(256), 0, ctx->stream, B->d_indptr, B->d_indices,
                               (const T *)B->d_data, B->n_rows, (const uint32_t *)p->d_orig_of, p->blk_bytes, p->d_blk);
            return SG_OK;
        });
        if (hipGetLastError() != hipSuccess) return SG_ERR_HIP;
    }
    if (p->d_fwd_ptr && !rows_written) {
        const int64_t work = B->nnz > B->n_rows + 1 ? B->nnz : B->n_rows + 1;
        const unsigned g2 = (unsigned)((work + 255) / 256);
        const unsigned g4 = (unsigned)((B->n_rows * 16 + 255) / 256);
        by_dtype(B->dtype, [&](auto tag) {
            using T = decltype(tag);
            hipLaunchKernelGGL(fwd_pack<T>, dim3(g2), dim3(256), 0, ctx->stream, B->d_indptr, B->d_indices,
                               (const T *)B->d_data, B->n_rows, B->nnz, (const uint32_t *)p->d_orig_of, p->d_fwd_ptr, p->d_fwd);
            if (p->d_q8 && B->n_rows > 0)
                hipLaunchKernelGGL(q8_pack_kernel<T>, dim3(g4), dim3(256), 0, ctx->stream, B->d_indptr, B->d_indices,
                                   (const T *)B->d_data, B->n_rows, (const uint32_t *)p->d_orig_of, (uint4 *)p->d_q8, 1.0f / p->norm_up,
                                   q8_rest_unknown(ctx));
            return SG_OK;
        });
        if (hipGetLastError() != hipSuccess) return SG_ERR_HIP;
    }
    return SG_OK;
}

// the null postings and the scoring context, where the tables kernel has not written them (the path with global counters)
static int write_aux(sg_ctx *ctx, sg_postings *p) {
    if (p->d_filt) {
        hipLaunchKernelGGL(null_postings_kernel, dim3(2), dim3(256), 0, ctx->stream, p->d_filt + p->nnz);
        if (hipGetLastError() != hipSuccess) return SG_ERR_HIP;
    }
    if (p->d_fwd_ptr) {
        SG_TRY(ctx->alloc(256, (void **)&p->d_score_ctx));
        hipLaunchKernelGGL(score_ctx_kernel, dim3(1), dim3(1), 0, ctx->stream, score_ctx_of(p), p->d_score_ctx);
        if (hipGetLastError() != hipSuccess) return SG_ERR_HIP;
    }
    return SG_OK;
}

// the index over the rows of B_in; `pending`: B_in is the representatives' matrix of these groups, its rows not written yet
static int build_index(sg_ctx *ctx, const sg_csr *B_in, int32_t tile_cols, int32_t flags, SgCollapse *pending,
                       std::optional<SgTimer> &timer, sg_postings **out) {
    bool cosine_like = false;
    float max_norm2 = 0.f;
    SG_TRY(sg_csr_props(ctx, B_in, &cosine_like, &max_norm2));
    // a posting segment (term k, tile t) must name every row once: the exact kernel adds a segment's products with a plain
    // read-add-write per lane (sg_spgemm_topn.hip), and of two entries (j, k) of one row one product would be lost
    SG_REQUIRE(!B_in->props_repeated_column,
               "the right-hand matrix has a row that names a column twice: the columns of a row must be distinct (sum the "
               "repeated entries first, e.g. scipy's sum_duplicates())");
    BuildPlan plan;
    SG_TRY(plan_build(ctx, B_in, tile_cols, flags, cosine_like, max_norm2, &plan));
    if (!timer) timer.emplace(ctx, SG_K_POSTINGS);   // the whole build, the permuted copy included
    PostingsPtr p(new (std::nothrow) sg_postings());
    if (!p) return SG_ERR_OOM;
    p->ctx = ctx;
    Scratch early(ctx);   // (after p: goes back before a half-built index does)
    EarlyRows rows;
    SG_TRY(alloc_early_rows(early, B_in, plan, &rows));
    if (plan.permute) SG_TRY(build_permuted(ctx, B_in, plan.tile_cols, p.get(), pending, &rows, 1.0f / plan.norm_up));
    if (!rows.written) {
        early.release(rows.fwd);
        early.release(rows.fwd_ptr);
        early.release(rows.q8);
        rows = EarlyRows();
    }
    // no copy in position order was made: the index reads the representatives' matrix itself
    if (pending && pending->pending_src && !p->permuted) SG_TRY(sg_collapse_materialize(ctx, pending));
    const sg_csr *B = p->permuted ? p->permuted : B_in;   // everything below indexes right-hand rows by POSITION
    SG_TRY(alloc_index(ctx, p.get(), B_in, B, plan, flags, early, &rows));
    if (plan.lds_path) {
        SG_TRY(fill_lds_path(ctx, p.get(), plan));
    } else {
        SG_TRY(fill_global_path(ctx, p.get(), plan));
        SG_TRY(tables_from_seg(ctx, p.get()));
    }
    SG_TRY(pack_rows(ctx, p.get(), rows.written));
    if (!plan.lds_path) SG_TRY(write_aux(ctx, p.get()));
    *out = p.release();
    return SG_OK;
}

extern "C" int sg_postings_build(sg_ctx *ctx, const sg_csr *B, int32_t tile_cols, sg_postings **out) {
    return sg_postings_build_flags(ctx, B, tile_cols, 0, out);
}

// (internal flags, above the public ones -- SG_POSTINGS_NO_COLLAPSE, SG_POSTINGS_EXACT_ONLY, SG_POSTINGS_TILE_FORM: sg_internal.h)
extern "C" int sg_postings_build_flags(sg_ctx *ctx, const sg_csr *B_in, int32_t tile_cols, int32_t flags, sg_postings **out) {
    SG_REQUIRE(ctx && B_in && out, "null argument");
    const bool group = !(flags & SG_POSTINGS_NO_COLLAPSE);
    std::optional<SgTimer> timer;
    SgCollapse *col = nullptr;
    if (group) {
        // identical rows (identical strings): one representative per group is indexed (sg_collapse.hip)
        bool cl = false;
        float n2 = 0.f;
        SG_TRY(sg_csr_props(ctx, B_in, &cl, &n2));
        timer.emplace(ctx, SG_K_POSTINGS);   // grouping + the index over the representatives
        if (cl) SG_TRY(sg_collapse_build(ctx, B_in, &col, /*left_side=*/false, /*defer_rows=*/true));
    }
    // (with groups the build writes the representatives' rows with its own copies of them)
    sg_postings *p = nullptr;
    const int st = build_index(ctx, col ? col->unique : B_in, tile_cols, flags, col, timer, &p);
    if (st != SG_OK) {
        sg_collapse_free(col);
        return st;
    }
    if (col) {
        p->collapse = col;
        p->caller_b_copy = csr_view(*B_in);
        p->caller_b = &p->caller_b_copy;
        p->n_right_caller = B_in->n_rows;
    }
    if (group) {
        p->build_tile_cols = tile_cols;
        p->build_flags = col ? flags : flags & 0xff;
    }
    *out = p;
    return SG_OK;
}

// The postings proper, when the build left them out (plan_build, lazy_full): same two passes, values only.
int sg_postings_ensure_full(sg_ctx *ctx, const sg_postings *cp) {
    sg_postings *p = const_cast<sg_postings *>(cp);
    if (p->d_vals || p->nnz <= 0) return SG_OK;
    const sg_csr *B = &p->src;
    Scratch scratch(ctx);
    uint32_t *cnt = nullptr, *len_scratch = nullptr;
    if (B->dtype == SG_F64) SG_TRY(scratch.alloc((size_t)B->nnz + 64, &p->d_rows));
    int st = scratch.alloc_bytes(((size_t)B->nnz + 64) * 8, &p->d_vals);
    if (st == SG_OK && !p->d_term_start) {
        sg_set_error("postings were built without the LDS path: nothing is lazy there");
        st = SG_ERR_BADARG;
    }
    const int32_t split = p->split > 0 ? p->split : 1;
    if (st == SG_OK) st = scratch.alloc((size_t)((int64_t)p->n_tiles * split * B->n_cols) + 1, &cnt);
    if (st == SG_OK) st = scratch.alloc((size_t)B->n_cols + 2, &len_scratch);
    if (st == SG_OK) st = lds_count_scan_fill(ctx, p, cnt, nullptr, len_scratch, nullptr, /*values_only=*/true, /*fill=*/true);
    if (st != SG_OK) {     // (the scratch takes the two arrays back)
        p->d_vals = nullptr;
        p->d_rows = nullptr;
        return st;
    }
    scratch.keep(p->d_rows);
    scratch.keep(p->d_vals);
    return SG_OK;
}

extern "C" int sg_postings_free(sg_postings *p) {
    if (!p) return SG_OK;
    p->ctx->release(p->d_seg);
    p->ctx->release(p->d_term_len);
    p->ctx->release(p->d_term_start);
    p->ctx->release(p->d_rows);
    p->ctx->release(p->d_vals);
    p->ctx->release(p->d_fwd);
    p->ctx->release(p->d_blk);
    p->ctx->release(p->d_q8);
    p->ctx->release(p->d_fwd_ptr);
    p->ctx->release(p->d_filt);
    p->ctx->release(p->d_ends);
    p->ctx->release(p->d_ends8);
    p->ctx->release(p->d_score_ctx);
    p->ctx->release(p->d_orig_of);
    p->ctx->release(p->d_pos_of);
    sg_csr_free(p->permuted);
    sg_collapse_free(p->collapse);
    if (p->plain) sg_postings_free(p->plain);
    if (p->exact_native) sg_postings_free(p->exact_native);
    if (p->alt_tile) sg_postings_free(p->alt_tile);
    delete p;
    return SG_OK;
}
