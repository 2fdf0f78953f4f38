// The rule of csrc/sg_plan.h -- which form of the top-n multiply runs, on which index -- held at every bar and one step
// under it.  Stand-alone: only sg_plan.h is included, the device work between two questions (an index of the multiply's own,
// sg_csr_props, the pilot) is played by decide() in plan_multiply's order.  The expected values were taken from
// plan_multiply as it stood before the rule had a header of its own (profiles/multiply_plan_refactor_ab.log), not from the
// header.  Exit status 0, or 1 with the name of every failing case.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "sg_plan.h"

enum Index { CALLER, TILE, NATIVE };   // the caller's index, the tile-by-tile form's, the exact kernel's own

struct Input {
    SgPlanLeft a;
    SgPlanIndex b;            // the caller's index
    SgPlanCall call;
    SgPlanSwitches sw;
    bool a_cosine_like = true;                              // what sg_csr_props would say
    unsigned long long pilot[4] = {1536, 1000, 10, 0};      // what the pilot would count: rows, postings, survivors, MACs
};

struct Outcome {
    SgPlan::Form form;
    Index index;
    double delta;
    bool props, pilot;       // asks for A's properties; pilots
};

// An index of the multiply's own, as the build makes it from `home`
static SgPlanIndex built(const SgPlanIndex &home, bool tile_form, bool f64) {
    SgPlanIndex b = home;
    b.source_rows = home.n_right;
    b.fold_log2 = 0;
    b.tile_form = tile_form;
    b.has_filter = tile_form;
    b.tile_log2 = tile_form ? 11 : (f64 ? 10 : 11);
    b.pruned_tile = b.tile_log2 >= 11;
    b.n_tiles = (int32_t)((home.n_right + ((int64_t)1 << b.tile_log2) - 1) >> b.tile_log2);
    if (b.n_tiles < 1) b.n_tiles = 1;
    return b;
}

static Outcome decide(const Input &in) {
    Outcome o{SgPlan::EXACT, CALLER, 0.0, false, false};
    SgPlanCall call = in.call;
    call.threshold = sg_plan_clamp_threshold(call.threshold);
    SgPlanIndex b = in.b;
    if (sg_plan_wants_tile_form(in.a, b, call, in.sw) && sg_plan_source_fits(b)) {
        b = built(b, true, in.a.f64);
        o.index = TILE;
    }
    bool a_cosine_like = false;
    if (sg_plan_needs_props(in.a, b, call, in.sw)) {
        o.delta = sg_plan_delta(in.a, b, call, in.sw);
        o.props = true;
        a_cosine_like = in.a_cosine_like;
    }
    o.form = sg_plan_form(in.a, b, call, in.sw, a_cosine_like);
    if (sg_plan_pilot_due(in.a, b, call, in.sw, o.form)) {
        o.pilot = true;
        o.form = sg_plan_after_pilot(o.form, sg_plan_pilot_prices(in.pilot, in.a, b, o.form == SgPlan::PRUNED_SELFJOIN), in.sw);
    }
    if (sg_plan_exact_own_index(in.a, b, call, in.sw, o.form) != SgOwnIndex::none) o.index = NATIVE;
    return o;
}

// ---- the inputs: 100 000 names of 10 entries against themselves, f32, 0.8, top 10, the index as built (4096-column tiles
//      folded by eight), a vocabulary of 30 000 terms (0.004 x 30 000 = 120 entries a row)
static void shape(Input &in, int64_t rows, int64_t nnz) {   // a self-join of this shape (a one-sided case sets its index afterwards)
    in.a.n_rows = in.b.n_right = in.b.source_rows = rows;
    in.a.nnz = in.b.nnz = nnz;
    in.b.n_tiles = (int32_t)((rows + 4095) / 4096 > 0 ? (rows + 4095) / 4096 : 1);
}

static Input names() {
    Input in;
    in.a.is_index_source = true;
    in.b.cosine_like = in.b.has_filter = in.b.pruned_tile = true;
    in.b.fold_log2 = 3;
    in.b.tile_log2 = 12;
    in.b.n_terms = 30000;
    shape(in, 100000, 1000000);
    in.call.stride = 10;
    in.call.threshold = 0.8;
    return in;
}

template <typename F>
static Input with(F change) {
    Input in = names();
    change(in);
    return in;
}

static void one_sided(Input &in) {   // the left matrix is another one; the index's own source is known
    in.a.is_index_source = false;
}

static void two_grams(Input &in, int64_t rows) {   // 15 entries a row of a vocabulary of 700: the pilot's regime
    in.b.n_terms = 700;
    shape(in, rows, rows * 15);
}

static double under(double x) { return nextafter(x, -1.0); }

struct Case {
    const char *name;
    Input in;
    Outcome want;
};

static const SgPlan::Form EXACT = SgPlan::EXACT, EXACT_SELFJOIN = SgPlan::EXACT_SELFJOIN, PRUNED = SgPlan::PRUNED,
                          PRUNED_SELFJOIN = SgPlan::PRUNED_SELFJOIN;

static std::vector<Case> cases() {
    std::vector<Case> c;
    // ---- thresholds
    c.push_back({"0.65: the stream form on the caller's index", with([](Input &in) { in.call.threshold = 0.65; }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"under 0.65: the tile form on its own index; the tile form always gets 0.05", with([](Input &in) { in.call.threshold = under(0.65); }), {PRUNED_SELFJOIN, TILE, 0.05, true, false}});
    c.push_back({"0.45 with SG_ALT_FORM=0: still the stream form", with([](Input &in) { in.call.threshold = 0.45; in.sw.alt_form = 0; }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"under 0.45 with SG_ALT_FORM=0: the exact kernel", with([](Input &in) { in.call.threshold = under(0.45); in.sw.alt_form = 0; }), {EXACT_SELFJOIN, NATIVE, 0.03, true, false}});
    c.push_back({"0.40: the tile form", with([](Input &in) { in.call.threshold = 0.40; }), {PRUNED_SELFJOIN, TILE, 0.05, true, false}});
    c.push_back({"under 0.40: the exact kernel", with([](Input &in) { in.call.threshold = under(0.40); }), {EXACT_SELFJOIN, NATIVE, 0.03, true, false}});
    c.push_back({"threshold 0", with([](Input &in) { in.call.threshold = 0.0; }), {EXACT_SELFJOIN, NATIVE, 0.02, true, false}});
    c.push_back({"threshold -1 clamps to 0", with([](Input &in) { in.call.threshold = -1.0; }), {EXACT_SELFJOIN, NATIVE, 0.02, true, false}});
    // ---- stride
    c.push_back({"row range, stride 64: the self-join form", with([](Input &in) { in.call.row_range = true; in.call.stride = 64; }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"row range, stride 65: not the self-join form", with([](Input &in) { in.call.row_range = true; in.call.stride = 65; }), {PRUNED, CALLER, 0.03, true, false}});
    c.push_back({"stride 128: the self-join form with two register lists", with([](Input &in) { in.call.stride = 128; }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"stride 129: the exact kernel, one-sided", with([](Input &in) { in.call.stride = 129; }), {EXACT, CALLER, 0.0, false, false}});
    c.push_back({"stride 128 under 0.65: the tile form", with([](Input &in) { in.call.stride = 128; in.call.threshold = 0.6; }), {PRUNED_SELFJOIN, TILE, 0.05, true, false}});
    c.push_back({"stride 129 under 0.65: no tile form", with([](Input &in) { in.call.stride = 129; in.call.threshold = 0.6; }), {EXACT, CALLER, 0.0, false, false}});
    // ---- when the self-join form pays
    c.push_back({"65 535 rows of 10 entries: one-sided", with([](Input &in) { shape(in, 65535, 655350); }), {PRUNED, CALLER, 0.03, true, false}});
    c.push_back({"65 536 rows of 10 entries: the self-join form", with([](Input &in) { shape(in, 65536, 655360); }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"30 000 rows holding 19 x 65 536 entries: the self-join form", with([](Input &in) { shape(in, 30000, 19 * 65536); }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"30 000 rows holding 19 x 65 536 - 1 entries: one-sided", with([](Input &in) { shape(in, 30000, 19 * 65536 - 1); }), {PRUNED, CALLER, 0.03, true, false}});
    c.push_back({"below the threshold, 16 383 rows: the exact kernel one-sided", with([](Input &in) { shape(in, 16383, 163830); in.call.threshold = 0.3; }), {EXACT, CALLER, 0.03, true, false}});
    c.push_back({"below the threshold, 16 384 rows: the exact kernel in the self-join form", with([](Input &in) { shape(in, 16384, 163840); in.call.threshold = 0.3; }), {EXACT_SELFJOIN, NATIVE, 0.03, true, false}});
    c.push_back({"a one-sided product never takes the self-join form", with([](Input &in) { one_sided(in); }), {PRUNED, CALLER, 0.03, true, false}});
    c.push_back({"... nor the exact kernel's", with([](Input &in) { one_sided(in); in.call.threshold = 0.3; }), {EXACT, CALLER, 0.03, true, false}});
    c.push_back({"a row range takes the self-join form at any size", with([](Input &in) { shape(in, 1000, 10000); in.call.row_range = true; }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"the same 1 000 rows as a whole product: one-sided", with([](Input &in) { shape(in, 1000, 10000); }), {PRUNED, CALLER, 0.03, true, false}});
    // ---- row length and delta
    c.push_back({"a mean row of exactly 128 entries: the pruned kernel", with([](Input &in) { shape(in, 100000, 12800000); in.b.n_terms = 100000; }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"one entry more than 128 a row: the exact kernel", with([](Input &in) { shape(in, 100000, 12800001); in.b.n_terms = 100000; }), {EXACT_SELFJOIN, NATIVE, 0.03, true, false}});
    c.push_back({"rows at exactly 0.004 x terms: 0.03 and no pilot", with([](Input &in) { shape(in, 100000, 12000000); }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"one entry more than 0.004 x terms a row: 0.05 and the pilot", with([](Input &in) { shape(in, 100000, 12000001); }), {PRUNED_SELFJOIN, CALLER, 0.05, true, true}});
    c.push_back({"SG_PRUNE_DELTA=0.5 is cut at half the threshold", with([](Input &in) { in.sw.prune_delta = {true, 0.5}; }), {PRUNED_SELFJOIN, CALLER, 0.4, true, false}});
    c.push_back({"SG_PRUNE_DELTA=0.001 is raised to 0.02", with([](Input &in) { in.sw.prune_delta = {true, 0.001}; }), {PRUNED_SELFJOIN, CALLER, 0.02, true, false}});
    // ---- pilot
    c.push_back({"2-grams, 32 767 rows: no pilot", with([](Input &in) { two_grams(in, 32767); }), {PRUNED, CALLER, 0.05, true, false}});
    c.push_back({"2-grams, 32 768 rows: the pilot", with([](Input &in) { two_grams(in, 32768); }), {PRUNED, CALLER, 0.05, true, true}});
    c.push_back({"the pilot prices the pruned kernel cheaper: it stays", with([](Input &in) { two_grams(in, 40000); in.pilot[2] = 211200; }), {PRUNED, CALLER, 0.05, true, true}});
    c.push_back({"the pilot prices the pruned kernel dearer: the exact kernel", with([](Input &in) { two_grams(in, 40000); in.pilot[2] = 215040; }), {EXACT, CALLER, 0.05, true, true}});
    c.push_back({"a self-join under 0.55 x exact + 0.3: the pruned self-join form stays", with([](Input &in) { two_grams(in, 70000); in.pilot[2] = 100000; }), {PRUNED_SELFJOIN, CALLER, 0.05, true, true}});
    c.push_back({"a self-join over 0.55 x exact + 0.3 (and under exact): the exact kernel's self-join form", with([](Input &in) { two_grams(in, 70000); in.pilot[2] = 450000; }), {EXACT_SELFJOIN, NATIVE, 0.05, true, true}});
    c.push_back({"the same with SG_EXACT_SYM=0: no second look, the pruned form stays", with([](Input &in) { two_grams(in, 70000); in.pilot[2] = 450000; in.sw.exact_sym = 0; }), {PRUNED_SELFJOIN, CALLER, 0.05, true, true}});
    c.push_back({"a self-join over exact with SG_EXACT_SYM=0: the exact kernel one-sided, on its own index (2^20 postings and more)", with([](Input &in) { two_grams(in, 70000); in.pilot[2] = 3000000; in.sw.exact_sym = 0; }), {EXACT, NATIVE, 0.05, true, true}});
    c.push_back({"a one-sided product the pilot calls off: the exact kernel one-sided", with([](Input &in) { two_grams(in, 70000); one_sided(in); in.pilot[2] = 3000000; }), {EXACT, NATIVE, 0.05, true, true}});
    c.push_back({"SG_PRUNE_PILOT=0", with([](Input &in) { two_grams(in, 40000); in.pilot[2] = 215040; in.sw.prune_pilot = 0; }), {PRUNED, CALLER, 0.05, true, false}});
    c.push_back({"a row range never pilots", with([](Input &in) { two_grams(in, 40000); in.call.row_range = true; in.pilot[2] = 215040; }), {PRUNED_SELFJOIN, CALLER, 0.05, true, false}});
    // ---- the exact kernel's own index
    c.push_back({"f32, tile 2^11: the exact kernel stays on the caller's index", with([](Input &in) { in.call.threshold = 0.3; in.b.tile_log2 = 11; }), {EXACT_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"f64, tile 2^11: an index of 2^10-column tiles", with([](Input &in) { in.call.threshold = 0.3; in.b.tile_log2 = 11; in.a.f64 = true; }), {EXACT_SELFJOIN, NATIVE, 0.03, true, false}});
    c.push_back({"f64, tile 2^10: none (and no pruned kernel for that tile)", with([](Input &in) { in.call.threshold = 0.3; in.b.tile_log2 = 10; in.b.pruned_tile = false; in.a.f64 = true; }), {EXACT, CALLER, 0.0, false, false}});
    c.push_back({"one-sided, 2^20 - 1 postings: not worth a second index", with([](Input &in) { one_sided(in); in.call.threshold = 0.3; in.b.nnz = (1 << 20) - 1; }), {EXACT, CALLER, 0.03, true, false}});
    c.push_back({"one-sided, 2^20 postings: an index of its own", with([](Input &in) { one_sided(in); in.call.threshold = 0.3; in.b.nnz = 1 << 20; }), {EXACT, NATIVE, 0.03, true, false}});
    c.push_back({"the index's source is unknown: none", with([](Input &in) { one_sided(in); in.call.threshold = 0.3; in.b.nnz = 1 << 20; in.b.source_rows = -1; }), {EXACT, CALLER, 0.03, true, false}});
    c.push_back({"the index's source has another size: none", with([](Input &in) { one_sided(in); in.call.threshold = 0.3; in.b.nnz = 1 << 20; in.b.source_rows = 99999; }), {EXACT, CALLER, 0.03, true, false}});
    c.push_back({"no tile form either where the source is unknown: the stream form", with([](Input &in) { one_sided(in); in.call.threshold = 0.6; in.b.source_rows = -1; }), {PRUNED, CALLER, 0.03, true, false}});
    c.push_back({"... where it is known, one-sided products take the tile form too", with([](Input &in) { one_sided(in); in.call.threshold = 0.6; }), {PRUNED, TILE, 0.05, true, false}});
    c.push_back({"a row range below the threshold: nothing is asked, nothing built", with([](Input &in) { in.call.row_range = true; in.call.threshold = 0.3; }), {EXACT, CALLER, 0.0, false, false}});
    c.push_back({"a row range under 0.65 stays on the index given", with([](Input &in) { in.call.row_range = true; in.call.threshold = 0.6; }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    // ---- what is not cosine-like, or empty
    c.push_back({"A is not cosine-like", with([](Input &in) { in.a_cosine_like = false; }), {EXACT, CALLER, 0.03, true, false}});
    c.push_back({"the index is not cosine-like", with([](Input &in) { in.b.cosine_like = false; }), {EXACT, CALLER, 0.0, false, false}});
    c.push_back({"the index has no filter postings", with([](Input &in) { in.b.has_filter = false; }), {EXACT, CALLER, 0.0, false, false}});
    c.push_back({"no rows", with([](Input &in) { shape(in, 0, 0); }), {EXACT, CALLER, 0.0, false, false}});
    c.push_back({"an index without entries", with([](Input &in) { one_sided(in); in.b.nnz = 0; }), {EXACT, CALLER, 0.0, false, false}});
    // ---- every switch, set once
    c.push_back({"SG_PRUNE=0", with([](Input &in) { in.sw.prune = false; }), {EXACT, CALLER, 0.0, false, false}});
    c.push_back({"SG_PRUNE=0 under 0.65: no tile form", with([](Input &in) { in.sw.prune = false; in.call.threshold = 0.6; }), {EXACT, CALLER, 0.0, false, false}});
    c.push_back({"SG_SYM=0", with([](Input &in) { in.sw.sym = '0'; }), {PRUNED, CALLER, 0.03, true, false}});
    c.push_back({"SG_SYM=0 below the threshold", with([](Input &in) { in.sw.sym = '0'; in.call.threshold = 0.3; }), {EXACT, CALLER, 0.03, true, false}});
    c.push_back({"SG_SYM=1: the self-join form at any size", with([](Input &in) { in.sw.sym = '1'; shape(in, 1000, 10000); }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"SG_SYM=1 below the threshold", with([](Input &in) { in.sw.sym = '1'; shape(in, 1000, 10000); in.call.threshold = 0.3; }), {EXACT_SELFJOIN, NATIVE, 0.03, true, false}});
    c.push_back({"SG_ALT_FORM=0", with([](Input &in) { in.sw.alt_form = 0; in.call.threshold = 0.6; }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"SG_ALT_FORM_BELOW=0.5", with([](Input &in) { in.sw.alt_form_below = 0.5; in.call.threshold = 0.6; }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"SG_PRUNE_MIN_THRESHOLD=0.3 lowers both bars", with([](Input &in) { in.sw.prune_min_threshold = {true, 0.3}; in.call.threshold = 0.35; }), {PRUNED_SELFJOIN, TILE, 0.05, true, false}});
    c.push_back({"SG_PRUNE_MIN_THRESHOLD=0.3 with SG_ALT_FORM=0", with([](Input &in) { in.sw.prune_min_threshold = {true, 0.3}; in.sw.alt_form = 0; in.call.threshold = 0.35; }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"SG_PRUNE_MAX_MEAN_ROW=8", with([](Input &in) { in.sw.prune_max_mean_row = 8.0; }), {EXACT_SELFJOIN, NATIVE, 0.03, true, false}});
    c.push_back({"SG_SYM_MIN_ROWS=1000, 1 000 rows", with([](Input &in) { in.sw.sym_min_rows = 1000; shape(in, 1000, 10000); }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"SG_SYM_MIN_ROWS=1000, 999 rows", with([](Input &in) { in.sw.sym_min_rows = 1000; shape(in, 999, 9990); }), {PRUNED, CALLER, 0.03, true, false}});
    c.push_back({"SG_SYM_MIN_ROWS=1000, 999 rows holding 19 000 entries", with([](Input &in) { in.sw.sym_min_rows = 1000; shape(in, 999, 19000); }), {PRUNED_SELFJOIN, CALLER, 0.03, true, false}});
    c.push_back({"SG_EXACT_SYM_MIN_ROWS=1000", with([](Input &in) { in.sw.exact_sym_min_rows = 1000; shape(in, 1000, 10000); in.call.threshold = 0.3; }), {EXACT_SELFJOIN, NATIVE, 0.03, true, false}});
    c.push_back({"SG_EXACT_SYM=0", with([](Input &in) { in.sw.exact_sym = 0; in.call.threshold = 0.3; }), {EXACT, CALLER, 0.03, true, false}});
    c.push_back({"SG_EXACT_SYM=0 on 2^20 postings: the one-sided kernel's own index", with([](Input &in) { in.sw.exact_sym = 0; in.call.threshold = 0.3; shape(in, 100000, 1 << 20); }), {EXACT, NATIVE, 0.03, true, false}});
    c.push_back({"SG_EXACT_NATIVE=0", with([](Input &in) { in.sw.exact_native = 0; in.call.threshold = 0.3; }), {EXACT_SELFJOIN, CALLER, 0.03, true, false}});
    return c;
}

// ---- the pilot's two looks, at the prices themselves
struct PriceCase {
    const char *name;
    SgPlan::Form planned;
    double ms_pruned, ms_exact;
    int exact_sym;
    SgPlan::Form want;
};

static std::vector<PriceCase> price_cases() {
    const double bar = 0.55 * 2.0 + 0.3;   // the second look's bar at an exact price of 2 ms
    return {
        {"pruned == exact: pruned stays", PRUNED, 1.0, 1.0, 1, PRUNED},
        {"pruned one ulp over exact: exact", PRUNED, nextafter(1.0, 2.0), 1.0, 1, EXACT},
        {"self-join at 0.55 x exact + 0.3: pruned stays", PRUNED_SELFJOIN, bar, 2.0, 1, PRUNED_SELFJOIN},
        {"self-join one ulp over 0.55 x exact + 0.3: the exact kernel's self-join form", PRUNED_SELFJOIN, nextafter(bar, 2.0), 2.0, 1, EXACT_SELFJOIN},
        {"... with SG_EXACT_SYM=0 there is no second look", PRUNED_SELFJOIN, nextafter(bar, 2.0), 2.0, 0, PRUNED_SELFJOIN},
        {"the second look is the self-join's alone", PRUNED, nextafter(bar, 2.0), 2.0, 1, PRUNED},
        {"a veto of a self-join: the exact kernel's self-join form", PRUNED_SELFJOIN, 3.0, 2.0, 1, EXACT_SELFJOIN},
        {"a veto of a self-join with SG_EXACT_SYM=0: one-sided", PRUNED_SELFJOIN, 3.0, 2.0, 0, EXACT},
        {"a veto of a one-sided product: one-sided", PRUNED, 3.0, 2.0, 1, EXACT},
    };
}

// ---- the launch shape of the exact kernel (256 CUs, 160 KiB of LDS each)
struct ShapeCase {
    const char *name;
    bool f64;
    int64_t rows, postings;
    int32_t n_tiles, tile_log2, stride;
    int tile_group;
    SgSwitch<int> waves;
    int group, n_groups, n_pass, waves_per_cu;
    unsigned grid;
};

static std::vector<ShapeCase> shape_cases() {
    const int64_t budget_f32 = 192 * 1024 * 1024 / 8, budget_f64 = 192 * 1024 * 1024 / 12;   // postings in 192 MiB
    return {
        {"postings of exactly 192 MiB: one launch", false, 100000, budget_f32, 100, 12, 10, 0, {}, 100, 1, 1, 10, 2560},
        {"one posting more: tile groups", false, 100000, budget_f32 + 1, 100, 12, 10, 0, {}, 99, 2, 1, 10, 2560},
        {"f64, exactly 192 MiB", true, 100000, budget_f64, 100, 12, 10, 0, {}, 100, 1, 1, 5, 1280},
        {"f64, one posting more", true, 100000, budget_f64 + 1, 100, 12, 10, 0, {}, 99, 2, 1, 5, 1280},
        {"four times the budget", false, 100000, 4 * budget_f32, 100, 12, 10, 0, {}, 25, 4, 1, 10, 2560},
        {"far beyond the budget: a tile a launch at the least", false, 100000, 1000 * budget_f32, 100, 12, 10, 0, {}, 1, 100, 1, 10, 2560},
        {"SG_TILE_GROUP=7", false, 100000, 1000000, 100, 12, 10, 7, {}, 7, 15, 1, 10, 2560},
        {"SG_TILE_GROUP beyond the tiles", false, 100000, 1000000, 100, 12, 10, 1000, {}, 100, 1, 1, 10, 2560},
        {"f32, 4096-column tiles: 10 waves a CU", false, 100000, 1000000, 25, 12, 10, 0, {}, 25, 1, 1, 10, 2560},
        {"f64, 4096-column tiles: 5 waves a CU", true, 100000, 1000000, 25, 12, 10, 0, {}, 25, 1, 1, 5, 1280},
        {"f32, 2048-column tiles: 20 waves a CU", false, 100000, 1000000, 49, 11, 10, 0, {}, 49, 1, 1, 20, 5120},
        {"f32, 1024-column tiles: 40 fit, 32 is the cap", false, 100000, 1000000, 98, 10, 10, 0, {}, 98, 1, 1, 32, 8192},
        {"SG_WAVES_PER_CU=3", false, 100000, 1000000, 25, 12, 10, 0, {true, 3}, 25, 1, 1, 3, 768},
        {"fewer rows than waves: a wave a row", false, 100, 1000000, 25, 12, 10, 0, {}, 25, 1, 1, 10, 100},
        {"no rows: a grid of one", false, 0, 1000000, 25, 12, 10, 0, {}, 25, 1, 1, 10, 1},
        {"stride 64: one pass", false, 100000, 1000000, 25, 12, 64, 0, {}, 25, 1, 1, 10, 2560},
        {"stride 65: two passes", false, 100000, 1000000, 25, 12, 65, 0, {}, 25, 1, 2, 10, 2560},
        {"stride 129 over tile groups: three passes of four launches", false, 100000, 4 * budget_f32, 100, 12, 129, 0, {}, 25, 4, 3, 10, 2560},
    };
}

static SgLaunchShape shape_of(const ShapeCase &s) {
    SgPlanLeft a;
    SgPlanIndex b;
    SgPlanSwitches sw;
    a.f64 = s.f64;
    a.n_rows = s.rows;
    b.nnz = s.postings;
    b.n_tiles = s.n_tiles;
    b.tile_log2 = s.tile_log2;
    sw.tile_group = s.tile_group;
    sw.waves_per_cu = s.waves;
    return sg_plan_launch_shape(a, b, s.stride, 256, 160 * 1024, sw);
}

#ifndef PLAN_CASES_NO_MAIN
int main() {
    static const char *const FORMS[] = {"EXACT", "EXACT_SELFJOIN", "PRUNED", "PRUNED_SELFJOIN"}, *const INDEXES[] = {"caller's", "tile form", "exact kernel's own"};
    int failed = 0, total = 0;
    bool form_seen[4] = {false, false, false, false}, index_seen[3] = {false, false, false};
    if (0.004 * 30000.0 != 120.0) {   // (the cases at "exactly 0.004 x terms" rest on it)
        printf("FAILED: 0.004 x 30 000 is not 120 in double arithmetic\n");
        ++failed;
    }
    for (const Case &c : cases()) {
        const Outcome got = decide(c.in);
        ++total;
        form_seen[c.want.form] = index_seen[c.want.index] = true;
        if (got.form != c.want.form || got.index != c.want.index || got.delta != c.want.delta || got.props != c.want.props || got.pilot != c.want.pilot) {
            printf("FAILED: %s: got %s on the %s index, delta %.17g, props %d, pilot %d; want %s on the %s index, delta %.17g, props %d, pilot %d\n",
                   c.name, FORMS[got.form], INDEXES[got.index], got.delta, got.props, got.pilot, FORMS[c.want.form], INDEXES[c.want.index],
                   c.want.delta, c.want.props, c.want.pilot);
            ++failed;
        }
    }
    for (int i = 0; i < 4; ++i)
        if (!form_seen[i]) { printf("FAILED: no case expects the form %s\n", FORMS[i]); ++failed; }
    for (int i = 0; i < 3; ++i)
        if (!index_seen[i]) { printf("FAILED: no case expects the %s index\n", INDEXES[i]); ++failed; }
    for (const PriceCase &p : price_cases()) {
        SgPlanSwitches sw;
        sw.exact_sym = p.exact_sym;
        SgPilotPrices prices;
        prices.ms_pruned = p.ms_pruned;
        prices.ms_exact = p.ms_exact;
        const SgPlan::Form got = sg_plan_after_pilot(p.planned, prices, sw);
        ++total;
        if (got != p.want) {
            printf("FAILED: pilot prices: %s: got %s, want %s\n", p.name, FORMS[got], FORMS[p.want]);
            ++failed;
        }
    }
    for (const ShapeCase &s : shape_cases()) {
        const SgLaunchShape got = shape_of(s);
        ++total;
        if (got.group != s.group || got.n_groups != s.n_groups || got.n_pass != s.n_pass || got.waves_per_cu != s.waves_per_cu ||
            got.grid != s.grid || got.n_launch() != s.n_groups * s.n_pass) {
            printf("FAILED: launch shape: %s: got group %d, %d groups, %d passes, %d waves a CU, grid %u; want %d, %d, %d, %d, %u\n", s.name,
                   got.group, got.n_groups, got.n_pass, got.waves_per_cu, got.grid, s.group, s.n_groups, s.n_pass, s.waves_per_cu, s.grid);
            ++failed;
        }
    }
    printf("%d cases, %d failed\n", total, failed);
    return failed ? 1 : 0;
}
#endif
