// Device-side helpers shared by the kernels of the top-n multiply (sg_spgemm_topn.hip: exact kernel,
// zip; sg_spgemm_pruned.hip: pruned kernel).
#ifndef SG_K4_DEVICE_H
#define SG_K4_DEVICE_H
#include <math.h>

#include "sg_internal.h"

#define SG_TOPN_LANES 64

// Debug aid (-DSG_WATCHDOG): every data-dependent loop counts its iterations; an overrun records which
// loop it was in g_sg_watch and makes all loops wind down instead of hanging the GPU.
#ifdef SG_WATCHDOG
static __device__ int g_sg_watch[4];   // one per translation unit
#define SG_WD_DECL(c) int c = 0
#define SG_WD(c, limit, code)                                   \
    if (++(c) > (int)(limit) || ((volatile int *)g_sg_watch)[0]) { \
        if (((volatile int *)g_sg_watch)[0] == 0) {             \
            g_sg_watch[0] = (code);                             \
            g_sg_watch[1] = (int)(c);                           \
        }                                                       \
        break;                                                  \
    }
#ifndef SG_WATCH_NAME
#define SG_WATCH_NAME sg_debug_watch
#endif
extern "C" int SG_WATCH_NAME(int32_t *out4) {
    return hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_sg_watch), 16) == hipSuccess ? 0 : 4;
}
#else
#define SG_WD_DECL(c)
#define SG_WD(c, limit, code)
#endif   // entries of the register-resident list = lanes of a wave

template <typename T>
__device__ __forceinline__ T wave_read(T v, int src_lane);   // value of v in lane src_lane (uniform src)

template <>
__device__ __forceinline__ float wave_read<float>(float v, int src_lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src_lane));
}
template <>
__device__ __forceinline__ int wave_read<int>(int v, int src_lane) {
    return __builtin_amdgcn_readlane(v, src_lane);
}
template <>
__device__ __forceinline__ uint32_t wave_read<uint32_t>(uint32_t v, int src_lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, src_lane);
}
template <>
__device__ __forceinline__ double wave_read<double>(double v, int src_lane) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, src_lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), src_lane);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

template <typename T>
__device__ __forceinline__ T mul_rn(T a, T b);
template <>
__device__ __forceinline__ float mul_rn<float>(float a, float b) { return __fmul_rn(a, b); }
template <>
__device__ __forceinline__ double mul_rn<double>(double a, double b) { return __dmul_rn(a, b); }

template <typename T>
__device__ __forceinline__ T add_rn(T a, T b);
template <>
__device__ __forceinline__ float add_rn<float>(float a, float b) { return __fadd_rn(a, b); }
template <>
__device__ __forceinline__ double add_rn<double>(double a, double b) { return __dadd_rn(a, b); }

template <typename T>
struct TopList {   // lane r holds the r-th best (score, col); empty slots are (-inf, INT_MAX)
    T s;
    int c;
    __device__ __forceinline__ void clear() {
        s = -INFINITY;
        c = INT32_MAX;
    }
    // (ns, nc) are wave-uniform.  floor_*: only entries strictly after the floor key are eligible
    // (used by the passes that collect ranks 64.. of a row; floor_s = +inf disables it).
    __device__ __forceinline__ void insert(T ns, int nc, int lane) {
        const bool mine_first = (s > ns) || (s == ns && c < nc);
        const int pos = __popcll(__ballot(mine_first));
        if (pos >= SG_TOPN_LANES) return;
        const T us = __shfl_up(s, 1, 64);
        const int uc = __shfl_up(c, 1, 64);
        if (lane > pos) {
            s = us;
            c = uc;
        } else if (lane == pos) {
            s = ns;
            c = nc;
        }
    }
    // The same for a candidate that may already be in the list (same column => same pair => same score): entered once.
    // A repeat of an entry that has dropped off the end ranks behind all 64 entries and is refused like the first time.
    __device__ __forceinline__ void insert_unique(T ns, int nc, int lane) {
        if (__ballot(c == nc) != 0) return;
        insert(ns, nc, lane);
    }
};

// Two register lists behind each other: lane r holds the r-th and the (64 + r)-th best -- a row's result of 65 .. 128
// entries (the second pass of the self-join form, top_n above one register list).  What drops off the first list's end is
// the second list's new head.
template <typename T>
struct TopListWide {
    TopList<T> lo, hi;
    __device__ __forceinline__ void clear() {
        lo.clear();
        hi.clear();
    }
    __device__ __forceinline__ void insert(T ns, int nc, int lane) {
        const bool mine_first = (lo.s > ns) || (lo.s == ns && lo.c < nc);
        const int pos = __popcll(__ballot(mine_first));
        if (pos >= SG_TOPN_LANES) {
            hi.insert(ns, nc, lane);
            return;
        }
        const T es = wave_read<T>(lo.s, SG_TOPN_LANES - 1);
        const int ec = wave_read<int>(lo.c, SG_TOPN_LANES - 1);
        lo.insert(ns, nc, lane);
        if (ec != INT32_MAX) hi.insert(es, ec, lane);   // (ranks ahead of every entry of `hi`: position 0)
    }
    __device__ __forceinline__ void insert_unique(T ns, int nc, int lane) {
        if (__ballot(lo.c == nc || hi.c == nc) != 0) return;
        insert(ns, nc, lane);
    }
    __device__ __forceinline__ int count() const {
        return __popcll(__ballot(lo.c != INT32_MAX)) + __popcll(__ballot(hi.c != INT32_MAX));
    }
};

// Posting entry (written by K3): f32 -> packed {uint32 slot, float value}, one 8-byte load per lane;
// f64 -> slots[] (uint32) + vals[] (double).  "slot" is the BYTE offset of the entry's accumulator
// inside its column tile, (j mod TILE) * sizeof(T): the multiply never needs j itself -- the tile
// sweep recovers columns from positions -- so the address arithmetic is done once, in K3.
template <typename T>
struct Post;
template <>
struct Post<float> {
    typedef uint2 reg_t;
    static constexpr int STRIDE = 8;
    // address = kernel-constant base (SGPR pair) + 32-bit byte offset per lane: no 64-bit arithmetic at all
    static __device__ __forceinline__ reg_t load(const char *vals, const char *, uint32_t seg_lo, uint32_t entry) {
        return *reinterpret_cast<const uint2 *>(vals + ((seg_lo + entry) << 3));   // 32-bit offset: < 2^29 entries
    }
    static __device__ __forceinline__ uint32_t slot(const reg_t &r) { return r.x; }
    static __device__ __forceinline__ float val(const reg_t &r) { return __uint_as_float(r.y); }
};
template <>
struct Post<double> {
    struct reg_t {
        uint32_t j;
        double v;
    };
    static constexpr int STRIDE = 8;
    static __device__ __forceinline__ reg_t load(const char *vals, const char *slots, uint32_t seg_lo, uint32_t entry) {
        reg_t r;
        r.j = *reinterpret_cast<const uint32_t *>(slots + ((seg_lo + entry) << 2));
        r.v = *reinterpret_cast<const double *>(vals + ((seg_lo + entry) << 3));
        return r;
    }
    static __device__ __forceinline__ uint32_t slot(const reg_t &r) { return r.j; }
    static __device__ __forceinline__ double val(const reg_t &r) { return r.v; }
};


// ---- Dealing the 64 lanes of a wave to the np prefix terms of a row (pruned multiply), in proportion to their list
// lengths df.  THE RULE, for the kernel and for the host restatement the tests drive (sg_debug_deal_lanes):
//     every term gets one lane; the 64 - np spare ones go by largest remainder --
//     spare * df_t = q_t * dsum + rem_t  (0 <= rem_t < dsum, dsum = sum of the df),   G_t = 1 + q_t,   R = spare - sum q_t
//     and the R terms with the largest rem_t get one lane more; equal remainders: the term that comes first.
// In integers, hence exact: sum G = 64 whenever 1 <= np <= 64 and dsum > 0 (sum rem_t = R * dsum, so R <= np - 1 terms have
// a remainder to be chosen by), and a longer list never has fewer lanes than a shorter one (a larger df has the larger
// (q, rem) pair).  The rule before it, G_t = 1 + floor(spare * 0.999 * df_t / dsum) in floats, threw the remainders away:
// 4.6 of the 64 lanes read postings that add nothing for the whole row at 663 k, while the longest lane stream sets the
// rounds of every visit (scripts/k4p_deal_model.py).  It is kept behind SG_DEAL=floor.
//
// U = uint64_t on the host (any df below 2^32).  U = uint32_t on the wave: dsum < 2^30 there -- the lists are disjoint
// pieces of one posting array whose byte offsets fit 32 bits -- and the quotient (at most 63) comes from a float estimate
// that is off by one at most (three roundings of 2^-24 and a reciprocal of one ulp on a number below 64), set right by the
// remainder, which is computed modulo 2^32: the true one lies in (-dsum, 2 dsum).  No integer division on the GPU.
template <typename U>
__host__ __device__ __forceinline__ void sg_deal_share(U df, U dsum, uint32_t spare, uint32_t &q, U &rem) {
    if constexpr (sizeof(U) == 8) {
        const U num = (U)spare * df;
        q = (uint32_t)(num / dsum);
        rem = num % dsum;
    } else {
#ifdef __HIP_DEVICE_COMPILE__
        const float inv = __builtin_amdgcn_rcpf((float)dsum);
#else
        const float inv = 1.0f / (float)dsum;
#endif
        q = (uint32_t)((float)spare * (float)df * inv);
        int32_t r = (int32_t)(spare * df - q * dsum);
        if (r < 0) {
            --q;
            r += (int32_t)dsum;
        } else if (r >= (int32_t)dsum) {
            ++q;
            r -= (int32_t)dsum;
        }
        rem = (U)r;
    }
}
// The remainder from which a term gets one of the R >= 1 lanes left over: the largest c with at_least(c) >= R, where
// at_least(c) counts the prefix terms whose remainder is c or more (on the wave: one compare and a population count of its
// mask per probe).  Terms above c get a lane, the first R - at_least(c + 1) of those at c the rest.  Found bit by bit from
// the top bit of dsum - 1 down -- and no further than the first c that exactly R terms reach: they are the R largest, and
// with a handful of remainders spread over [0, dsum) that is a few probes, not log2(dsum).
template <typename U, typename AtLeast>
__host__ __device__ __forceinline__ U sg_deal_cut(U dsum, uint32_t R, AtLeast at_least) {
    U cut = 0;   // at_least(0) >= R: every term counts
    if (dsum < 2) return cut;
    const int top = (sizeof(U) == 8 ? 63 - __builtin_clzll((unsigned long long)(dsum - 1)) : 31 - __builtin_clz((unsigned)(dsum - 1)));
    for (U bit = (U)1 << top; bit; bit >>= 1) {
        const uint32_t n = at_least(cut | bit);
        if (n >= R) {
            cut |= bit;
            if (n == R) break;
        }
    }
    return cut;
}
// The rule before: remainders dropped (dsum as a float; np <= 64).
__host__ __device__ __forceinline__ uint32_t sg_deal_floor_rule(uint32_t df, float dsum, int np) {
    return 1u + (uint32_t)((float)(64 - np) * 0.999f * ((float)df / dsum));
}

// Next left row for this wave: one global atomic by lane 0, broadcast.  The result is made
// explicitly wave-uniform so that everything derived from it stays in SGPRs / uniform branches.
__device__ __forceinline__ uint32_t next_row(uint32_t *row_counter, int lane) {
    uint32_t r = 0;
    if (lane == 0) r = __hip_atomic_fetch_add(row_counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)r);
}

#endif   // SG_K4_DEVICE_H
