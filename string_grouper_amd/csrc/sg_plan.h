// Which form of the top-n multiply runs, and on which index ("Which form runs"): the rule and nothing
// else.  Pure functions of a handful of numbers, one per question of the table there, in the order plan_multiply
// (sg_spgemm_topn.hip) asks them; the device work between two questions -- an index of the multiply's own, sg_csr_props,
// the pilot -- is plan_multiply's.  No HIP, no library types: a host compiler builds this alone, and
// tests/native/plan_cases.cpp holds every bar below at the bar and one step under it.
#pragma once

#include <stddef.h>
#include <stdint.h>

struct sg_postings;

constexpr int32_t SG_PLAN_LANES = 64;   // entries of one register list (SG_TOPN_LANES; sg_spgemm_topn.hip asserts it)

// ---- what the rule is asked about
struct SgPlanLeft {             // the left matrix
    int64_t n_rows = 0, nnz = 0;
    bool f64 = false;
    bool is_index_source = false;   // A is the matrix the index was built from: a self-join
};

struct SgPlanIndex {            // an index: the caller's, or one kept with it
    bool cosine_like = false;
    bool has_filter = false;    // filter postings: the pruned kernel can run on it
    bool tile_form = false;     // the pruned multiply's tile-by-tile form (SG_POSTINGS_TILE_FORM)
    bool pruned_tile = false;   // a tile the pruned kernel is built for (sg_pruned_supports_tile)
    int32_t fold_log2 = 0, tile_log2 = 0, n_tiles = 0;
    int64_t n_right = 0, nnz = 0, n_terms = 0;
    int64_t source_rows = -1;   // rows of the matrix an index of the multiply's own would be built from (A itself in a
                                // self-join, otherwise the matrix the caller's index was built from); -1: not known
};

struct SgPlanCall {
    int32_t stride = 0;         // result columns per row
    double threshold = 0.0;     // the caller's, clamped at 0
    bool row_range = false;     // the question of sg_selfjoin_range, a row range of a multi-GPU self-join -- can the pruned
                                // kernel's self-join form take it on the index given, at any size and with one register
                                // list?  Anything else is not applicable there: no index of the multiply's own, no exact
                                // kernel in the self-join form, no pilot.
};

template <typename T>
struct SgSwitch {               // a switch whose default depends on the product
    bool set = false;
    T value{};
    T or_default(T dflt) const { return set ? value : dflt; }
};

struct SgPlanSwitches {         // the SG_* switches of the multiply, read once per call (multiply_switches)
    bool prune = true;                       // SG_PRUNE        (off: starts with '0')
    char sym = 0;                            // SG_SYM          first character; '0' off, '1' at any size
    int alt_form = 1;                        // SG_ALT_FORM
    double alt_form_below = 0.65;            // SG_ALT_FORM_BELOW
    SgSwitch<double> prune_min_threshold;    // SG_PRUNE_MIN_THRESHOLD
    double prune_max_mean_row = 128.0;       // SG_PRUNE_MAX_MEAN_ROW
    SgSwitch<double> prune_delta;            // SG_PRUNE_DELTA
    int sym_min_rows = 65536;                // SG_SYM_MIN_ROWS
    int exact_sym_min_rows = 16384;          // SG_EXACT_SYM_MIN_ROWS
    int exact_sym = 1;                       // SG_EXACT_SYM
    int prune_pilot = 1;                     // SG_PRUNE_PILOT
    int exact_native = 1;                    // SG_EXACT_NATIVE
    int tile_group = 0;                      // SG_TILE_GROUP   (<= 0: from the budget)
    SgSwitch<int> waves_per_cu;              // SG_WAVES_PER_CU
};

// ---- what the rule answers: the exact kernel or the pruned one (sg_spgemm_pruned.hip), each one-sided or in the self-join
//      form (A is the matrix the index was built from: every pair scored once, from the row with the larger index), and the
//      index its launches run on
struct SgLaunchShape {       // the exact kernel's launches (sg_plan_launch_shape)
    int group = 1;           // tiles per launch
    int n_groups = 1;
    int n_pass = 1;          // a pass per register list of result columns
    int waves_per_cu = 1;
    unsigned grid = 1;
    int n_launch() const { return n_groups * n_pass; }
};

struct SgPlan {
    enum Form { EXACT, EXACT_SELFJOIN, PRUNED, PRUNED_SELFJOIN };
    Form form = EXACT;
    const sg_postings *index = nullptr;   // the caller's index, or one kept with it (sg_postings::alt_tile, exact_native)
    int32_t stride = 0;                   // result columns per row
    double threshold = 0.0;               // the caller's, clamped at 0
    double delta = 0.0;                   // the pruned kernel's room below the threshold for its survivor bound
    SgLaunchShape launch;
};

static inline bool sg_plan_pruned(SgPlan::Form f) { return f == SgPlan::PRUNED || f == SgPlan::PRUNED_SELFJOIN; }
static inline bool sg_plan_selfjoin(SgPlan::Form f) { return f == SgPlan::PRUNED_SELFJOIN || f == SgPlan::EXACT_SELFJOIN; }

// only touched accumulators are candidates; with non-negative data (TF-IDF) touched == value > 0,
// so a negative threshold selects the same entries as 0
static inline double sg_plan_clamp_threshold(double threshold) { return threshold > 0.0 ? threshold : 0.0; }

// Threshold from which the pruned multiply takes a product: 0.45 in the stream form (below, its filter passes too much:
// profiles/r01_prune_tuning.log), 0.40 for a self-join that can run the tile-by-tile form on an index of its own (200 k names
// at 0.4: 9.9 ms against 12.1 for the exact kernel in the self-join form and 20.8 one-sided; at 0.35 the two are level:
// profiles/r06b_form_sweep.log).  SG_PRUNE_MIN_THRESHOLD overrides both.
static inline double sg_plan_min_threshold(const SgPlanSwitches &sw, bool tile_form) {
    return sw.prune_min_threshold.or_default(tile_form ? 0.40 : 0.45);
}

// ---- 1. which form of the pruned multiply?  The stream form (the index as built: 4096-column tiles folded eight to an
//      accumulator tile, second filter) is the fastest where most candidates are false alarms -- name-matching thresholds.
//      As the threshold falls, sums of eight unrelated columns cross the bar ever more often: from SG_ALT_FORM_BELOW (0.65)
//      down a self-join runs the tile-by-tile form on an index of its own, built once and kept with the index
//      (scripts/form_sweep.py, 200 k / 663 k names at 0.6: 5.4 / 31.4 ms stream, 3.4 / 24.1 ms tile by tile; at 0.8:
//      1.3 / 5.1 against 1.8 / 11.7).
//      One-sided products (master x duplicates) too: the index is then built from the matrix the caller's index was.
static inline bool sg_plan_wants_tile_form(const SgPlanLeft &a, const SgPlanIndex &b, const SgPlanCall &c, const SgPlanSwitches &sw) {
    return !c.row_range && b.cosine_like && b.has_filter && b.fold_log2 > 0 && c.stride <= 2 * SG_PLAN_LANES && a.n_rows > 0 &&
           b.n_right > 0 && c.threshold < sw.alt_form_below && c.threshold >= sg_plan_min_threshold(sw, true) &&
           sw.alt_form != 0 && sw.prune;
}

// An index of the multiply's own is built from a matrix that is known and holds the index's rows
static inline bool sg_plan_source_fits(const SgPlanIndex &b) { return b.source_rows >= 0 && b.source_rows == b.n_right; }

// ---- 2. pruned multiply (sg_spgemm_pruned.hip) when both sides are cosine-like and one register list holds the row's
//      result, and there is room below the threshold for its survivor bound.  (top_n of 65 .. 128: the pruned kernel keeps
//      a row's best 64 in its register list; a row that fills the list may have more matches and is handed to the exact
//      kernel, which runs a pass per 64 entries -- rows_with_full_lists_kernel.)
//      The envelope: everything but the threshold, the mean row and A's own properties.
static inline bool sg_plan_in_envelope(const SgPlanLeft &a, const SgPlanIndex &b, const SgPlanCall &c, const SgPlanSwitches &sw) {
    return sw.prune && b.cosine_like && b.has_filter && c.stride <= 2 * SG_PLAN_LANES && a.n_rows > 0 && b.nnz > 0 && b.pruned_tile;
}

// ... and rows of more than 128 entries are beyond it altogether: where that is the AVERAGE row (strings of 130 characters
// and more) nearly every row would be passed on one by one -- 50 k strings of 155 entries: 68 ms that way, 37.5 the
// exact kernel alone (profiles/r06b_long_strings.log) -- the exact kernel takes the product as it does below the threshold
static inline bool sg_plan_threshold_ok(const SgPlanLeft &a, const SgPlanIndex &b, const SgPlanCall &c, const SgPlanSwitches &sw) {
    return c.threshold >= sg_plan_min_threshold(sw, b.tile_form) &&
           !((double)a.nnz > sw.prune_max_mean_row * (double)a.n_rows);   // below ~0.4 the filter passes too much (profiles/r01_prune_tuning.log)
}

// Rows that are dense next to the vocabulary (2-grams: a row holds 2 % of all terms): the regime of the wider delta and of
// the pruned-or-exact pilot
static inline bool sg_plan_dense_rows(const SgPlanLeft &a, const SgPlanIndex &b) {
    return a.n_rows > 0 && (double)a.nnz / (double)a.n_rows > 0.004 * (double)b.n_terms;
}

// tuned at 663 k: the tile-by-tile form 0.05 (profiles/r01_prune_tuning.log); the stream form, whose rounds are cheaper
// next to the exact scorings, 0.03 (profiles/r03_sessionG_H_delta.log: 9.76 / 9.95 / 10.10 ms at 0.03 / 0.04 / 0.05;
// with identical rows grouped the optimum is flat from 0.02 to 0.04: profiles/r03_sessionU_delta_freq_ab.log)
// (0.03 only where rows are sparse next to the vocabulary -- name data; on small vocabularies, the regime of the
//  pruned-or-exact pilot below, a tighter bound passes too many candidates: 0.05 as before)
static inline double sg_plan_delta(const SgPlanLeft &a, const SgPlanIndex &b, const SgPlanCall &c, const SgPlanSwitches &sw) {
    const bool sparse_rows = a.n_rows > 0 && !sg_plan_dense_rows(a, b);
    double delta = sw.prune_delta.or_default(b.fold_log2 > 0 && sparse_rows ? 0.03 : 0.05);
    if (delta > 0.5 * c.threshold) delta = 0.5 * c.threshold;
    if (delta < 0.02) delta = 0.02;
    return delta;
}

// Are A's properties (sg_csr_props) needed at all?  Inside the envelope, and the threshold is inside it too or the exact
// kernel's self-join form is still open (never on a row range)
static inline bool sg_plan_needs_props(const SgPlanLeft &a, const SgPlanIndex &b, const SgPlanCall &c, const SgPlanSwitches &sw) {
    return sg_plan_in_envelope(a, b, c, sw) && (sg_plan_threshold_ok(a, b, c, sw) || !c.row_range);
}

// ---- 3. which form?
// self-join: score every pair once, from the row with the larger index (sg_spgemm_pruned.hip, symmetric mode;
// rows the pruned kernel cannot take go through the exact kernel's self-join launch inside the same pass) --
// with a top_n of 65 .. 128 too, except on a row range (the pass sends a row's own matches through the pair
// list, whose second pass selects with two register lists) ...
// ... from the size at which halving the (row, tile) visits outweighs the second pass over the pair list
// and its host round trip: 0.58 vs 0.57 ms at 50 k rows, 0.95 vs 1.20 at 100 k, 14.0 vs 26.8 at 663 k
// (profiles/r02_sessionM_sym_sweep.log)
// `threshold_ok` false: the form is the EXACT kernel's (sg_spgemm_pruned_symmetric, exact_all), with a bar of its own
static inline bool sg_plan_selfjoin_pays(const SgPlanLeft &a, const SgPlanCall &c, const SgPlanSwitches &sw, bool threshold_ok) {
    const int64_t sym_min_rows = sw.sym_min_rows;
    return sw.sym != '0' && c.stride <= (c.row_range ? 1 : 2) * SG_PLAN_LANES && a.is_index_source &&
           (c.row_range || a.n_rows >= sym_min_rows || sw.sym == '1' ||
            // (the bar was set on names, 19 entries a row; longer rows cost more each and the form pays earlier --
            //  50 k rows of 96 entries: 10.1 ms one-sided, 6.95 in the self-join form -- and the exact kernel in
            //  the self-join form halves a product that is many times dearer at the same size)
            a.nnz >= (int64_t)19 * sym_min_rows ||
            (!threshold_ok && a.n_rows >= (int64_t)sw.exact_sym_min_rows));
}

// a_cosine_like: what sg_csr_props said of A (false where sg_plan_needs_props did not ask)
static inline SgPlan::Form sg_plan_form(const SgPlanLeft &a, const SgPlanIndex &b, const SgPlanCall &c, const SgPlanSwitches &sw,
                                        bool a_cosine_like) {
    if (!sg_plan_needs_props(a, b, c, sw) || !a_cosine_like) return SgPlan::EXACT;
    const bool threshold_ok = sg_plan_threshold_ok(a, b, c, sw);
    const bool selfjoin = sg_plan_selfjoin_pays(a, c, sw, threshold_ok);
    if (threshold_ok) return selfjoin ? SgPlan::PRUNED_SELFJOIN : SgPlan::PRUNED;
    // the threshold ALONE keeps the pruned kernel out: the EXACT kernel in the self-join form (every row through its
    // self-join launch)
    return selfjoin && sw.exact_sym != 0 ? SgPlan::EXACT_SELFJOIN : SgPlan::EXACT;
}

// ---- 4. pruned or exact?  On a vocabulary that is small next to the rows (2-grams: a row holds 2 % of all terms) the
//      filter passes thousands of candidates per row and scoring them exactly costs more than the whole exact
//      multiply (119 vs 84 ms at 200 k 2-grams).  Nothing cheap predicts the candidates, so on such inputs three
//      blocks of 512 left rows are run through the pruned kernel first and the two costs are priced from what
//      they did (prune_pilot; constants fitted on the family sweep in profiles/r02_profile_k4p_v9b_sym.log).
static inline bool sg_plan_pilot_due(const SgPlanLeft &a, const SgPlanIndex &b, const SgPlanCall &c, const SgPlanSwitches &sw,
                                     SgPlan::Form form) {
    return !c.row_range && sg_plan_pruned(form) && a.n_rows >= 32768 && a.nnz > 0 && b.n_terms > 0 && sg_plan_dense_rows(a, b) &&
           sw.prune_pilot != 0;
}

struct SgPilotPrices {
    double ms_pruned = 0.0, ms_exact = 0.0;
};

// The pilot's counters, extrapolated and priced: [0] rows sampled [1] postings [2] survivors [3] MACs of the whole multiply
static inline SgPilotPrices sg_plan_pilot_prices(const unsigned long long h[4], const SgPlanLeft &a, const SgPlanIndex &b, bool selfjoin) {
    const double s = a.f64 ? 8.0 : 4.0;
    const double rows = (double)a.n_rows, sampled = h[0] > 0 ? (double)h[0] : 1.0;
    const double candidates = (double)h[2] * rows / sampled;
    // fitted on scripts/family_sweep.py (profiles/r02_profile_k4p_v9b_sym.log): the pruned kernel pays per (row, tile)
    // visit and per candidate it scores exactly (a candidate costs one walk over a right-hand row); the exact kernel
    // pays its stream model (long lists stream at ~6 TB/s, the 3.7 TB/s of name data include its per-visit overhead)
    // plus its own per-visit cost
    const double row_len = b.n_right > 0 ? (double)b.nnz / (double)b.n_right : 0.0;
    SgPilotPrices p;
    p.ms_pruned = rows * (double)b.n_tiles * 2.0e-7 + candidates * 2.9e-9 * row_len;
    if (selfjoin) p.ms_pruned = 0.55 * p.ms_pruned + 0.3;   // profiles/r02_sessionM_sym_sweep.log
    p.ms_exact = (double)h[3] * (4.0 + s) * 0.6 / 3.7e9 + rows * (double)b.n_tiles * 8.0e-7;
    return p;
}

// What the two prices say of a product planned as `form` (PRUNED or PRUNED_SELFJOIN): the form that runs
static inline SgPlan::Form sg_plan_after_pilot(SgPlan::Form form, const SgPilotPrices &p, const SgPlanSwitches &sw) {
    const bool exact_selfjoin_open = form == SgPlan::PRUNED_SELFJOIN && sw.exact_sym != 0;
    bool keep_pruned = p.ms_pruned <= p.ms_exact;
    // (the exact kernel in the self-join form walks half the (row, tile) visits -- 200 k 2-grams: 63 ms one-sided; the
    //  same factor the pilot grants the pruned kernel's self-join form)
    if (exact_selfjoin_open && keep_pruned && p.ms_pruned > 0.55 * p.ms_exact + 0.3) keep_pruned = false;
    if (keep_pruned) return form;
    return exact_selfjoin_open ? SgPlan::EXACT_SELFJOIN : SgPlan::EXACT;
}

// ---- 5. does the exact kernel get an index of its own?
enum class SgOwnIndex { none, from_left, from_source };

static inline SgOwnIndex sg_plan_exact_own_index(const SgPlanLeft &a, const SgPlanIndex &b, const SgPlanCall &c,
                                                 const SgPlanSwitches &sw, SgPlan::Form form) {
    const bool native_on = !c.row_range && sw.exact_native != 0;
    const int32_t native_tile_log2 = a.f64 ? 10 : 11;
    if (!native_on || !(b.tile_log2 > native_tile_log2)) return SgOwnIndex::none;
    // the exact kernel in the self-join form runs on ITS layout of the index (tile of 2048 / 1024 columns: twice the waves
    // per CU), built once per index and kept with it -- also what the one-sided exact kernel runs on if the form is called
    // off (pair list too small)
    if (form == SgPlan::EXACT_SELFJOIN) return SgOwnIndex::from_left;
    // ... and the exact kernel ONE-SIDED (a master x duplicates product below the pruned multiply's thresholds, a self-join
    // too small for the self-join form) on its own layout as well, where the product is worth a second index: the
    // 4096-column tiles of the pruned multiply leave it half the waves per CU (200 k names at 0.4: 25.0 ms there, 20.8 on
    // its own)
    if (form == SgPlan::EXACT && b.has_filter && b.nnz >= ((int64_t)1 << 20) && sg_plan_source_fits(b)) return SgOwnIndex::from_source;
    return SgOwnIndex::none;
}

// ---- 6. the launch shape of the exact kernel
// single-wave workgroups, an accumulator tile each: as many waves per CU as the tiles leave room for in LDS
static inline int sg_plan_waves_per_cu(size_t lds_per_cu, bool f64, int32_t tile_log2) {
    const size_t lds = (size_t)(f64 ? 8 : 4) << tile_log2;
    int waves_per_cu = (int)(lds_per_cu / lds);
    if (waves_per_cu > 32) waves_per_cu = 32;
    if (waves_per_cu < 1) waves_per_cu = 1;
    return waves_per_cu;
}

static inline SgLaunchShape sg_plan_launch_shape(const SgPlanLeft &a, const SgPlanIndex &b, int32_t stride, int num_cu, size_t lds_per_cu,
                                                 const SgPlanSwitches &sw) {
    SgLaunchShape sh;
    // tiles per launch: keep one launch's postings (~ nnz*(4+s)/n_tiles per tile) near 2 MiB so that
    // they stay in every XCD's 4 MiB L2 while all rows stream over them
    // Tile groups (separate launches over a few tiles each, running state kept in the output arrays)
    // exist for right-hand sides whose postings exceed the 256 MiB Infinity Cache; below that one launch
    // is faster (measured: 280 ms vs 415 ms at 663 k -- every launch has a tail and a state round trip).
    int group = sw.tile_group;
    if (group <= 0) {
        const double bytes = (double)b.nnz * (double)(4 + (a.f64 ? 8 : 4));
        const double budget = 192.0 * 1024 * 1024;
        group = bytes <= budget ? b.n_tiles : (int)((double)b.n_tiles * budget / bytes);
        if (group < 1) group = 1;
    }
    if (group > b.n_tiles) group = b.n_tiles;
    sh.group = group;
    sh.n_groups = (b.n_tiles + group - 1) / group;
    sh.n_pass = (stride + SG_PLAN_LANES - 1) / SG_PLAN_LANES;
    sh.waves_per_cu = sw.waves_per_cu.or_default(sg_plan_waves_per_cu(lds_per_cu, a.f64, b.tile_log2));
    sh.grid = (unsigned)num_cu * (unsigned)sh.waves_per_cu;
    if ((int64_t)sh.grid > a.n_rows) sh.grid = (unsigned)(a.n_rows > 0 ? a.n_rows : 1);
    return sh;
}
