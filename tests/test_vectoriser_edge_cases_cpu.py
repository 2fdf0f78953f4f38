"""The lists, the restatement and the mutants of tests/_vectoriser_edge_cases.py, checked without a GPU and without the
library.  (a) Every edge that tests/test_vectoriser_edges_gpu.py relies on is in the lists -- read off the restatement of
what the device does with each string, nothing left to a random draw.  (b) The two references agree bit for bit on every
list.  (c) Every mutant -- the device's steps with one thing wrong -- gives a different answer on the list built for it: a
list that cannot tell a mutant from the reference could not tell a wrong kernel either."""
from collections import Counter

import numpy as np
import pytest

from oracle import oracle as O
from tests import _vectoriser_edge_cases as V

F32, F64 = np.float32, np.float64
CASES = [c.name for c in V.all_cases()]
SHORT = [c for c in CASES if c.startswith("short-")]
WAVE = [c for c in CASES if c.startswith("wave-")]
LONG = [c for c in CASES if c.startswith("long-")]


def rows_of(case, which="fit"):
    return V.describe(case.form, dict(case.lists())[which])


def all_rows(case):
    return [r for name, _ in case.lists() for r in rows_of(case, name)]


def runs(row):
    """(first sorted position, length) of every distinct n-gram of a row."""
    ends = np.cumsum(row.counts)
    return list(zip((ends - row.counts).tolist(), row.counts))


def straddles(row, position):
    """A run of a repeated n-gram that begins before the sorted position and ends behind it."""
    return any(lo < position < lo + c for lo, c in runs(row))


# ---------------------------------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("name", CASES)
def test_restatement_counts_the_n_grams_of_the_analyzer(name):
    """The rows the restatement reads off the prepared column hold the n-grams oracle.ngrams makes of the string itself, and
    the column is of the kind, and the fit of the key width, the form was built for."""
    case = V.case(name)
    for which, strings in case.lists():
        for s, r in zip(strings, rows_of(case, which)):
            want = Counter(O.ngrams(s, **case.form.kw))
            assert {V.term(t): c for t, c in zip(r.grams, r.counts)} == dict(want), (which, s[:40])
            assert r.g == sum(want.values()) and list(r.grams) == sorted(r.grams) and r.kept <= r.raw
            assert r.stage == ("short" if r.raw <= 64 else "wave" if r.g <= 1024 and r.kept <= 1040 else "long")
    form = case.form
    bits = V.device_bits(form, case.fit)
    assert (form.n * bits <= 25) == (form.keys == "tagged32") and (form.n * bits > 30) == (form.keys == "key64")
    assert form.n * bits <= 63
    if name.startswith(("short-", "wave-", "long-", "widest-")):
        assert bits == form.bits and V.kept_alphabet(form, case.fit) == frozenset(map(ord, form.chars.lower() if form.ignore_case else form.chars))
    assert not set(form.unseen) & set(form.chars)


def test_key_forms_are_the_listed_ones():
    width = {f.name: (f.n * f.bits, f.keys) for f in V.FORMS.values()}
    assert width == {"n1-bytes": (7, "tagged32"), "n2-bytes": (14, "tagged32"), "n3-bytes": (21, "tagged32"),
                     "n5a20-bytes": (25, "tagged32"), "n4a72-bytes": (28, "plain32"), "n5a50-bytes": (30, "plain32"),
                     "n7-bytes": (42, "key64"), "n21a8-bytes": (63, "key64"),
                     "n1-symbols": (7, "tagged32"), "n2-symbols": (12, "tagged32"), "n3-symbols": (18, "tagged32"),
                     "n5a20-symbols": (25, "tagged32"), "n4a72-symbols": (28, "plain32"), "n5a50-symbols": (30, "plain32"),
                     "n7-symbols": (42, "key64"), "n21a8-symbols": (63, "key64")}
    assert all(len(f.chars) > 64 for f in V.FORMS.values() if f.name.startswith("n4a72"))
    assert all(33 <= len(f.chars) <= 64 for f in V.FORMS.values() if f.name.startswith("n5a50"))
    assert all(5 <= len(f.chars) <= 8 for f in V.FORMS.values() if f.name.startswith("n21a8"))
    for f in V.FORMS.values():          # a symbol form holds non-ASCII characters, a byte form none
        assert f.symbols == any(ord(c) > 127 for c in f.chars)
    assert V.TOO_WIDE["ngram_size"] * V._bits(V.TOO_WIDE["chars"], V.TOO_WIDE["ngram_size"], False) == 64


# ---------------------------------------------------------------------------------------------------- (a) short stage
@pytest.mark.parametrize("name", SHORT)
def test_short_list_holds_every_short_stage_edge(name):
    case = V.case(name)
    form, n = case.form, case.form.n
    rows = rows_of(case)
    short = [r for r in rows if r.stage == "short"]
    # raw lengths; 65 is the wave stage's
    assert {0, n - 1, n, 63, 64} <= {r.raw for r in short}
    assert any(r.raw == 65 and r.stage == "wave" for r in rows)
    if not form.symbols:        # (a symbol column arrives with the deleted characters gone: raw is kept)
        assert {0, n - 1, n} <= {r.kept for r in short if r.raw == 64}
        assert any(r.raw > 64 and r.kept <= 64 and r.stage == "wave" and r.g > 0 for r in rows)
        assert any(r.raw == 65 and r.kept == 64 and r.stage == "wave" for r in rows)
    else:
        assert all(r.raw == r.kept for r in rows)
    # numbers of n-grams
    cells = V.short_g_cells(form)
    assert set(cells) <= {r.g for r in short} and {1, 2, 3, 4, 5, 64 - n, 65 - n} <= set(cells)
    assert ({61, 62} <= set(cells)) == (n <= 3) and (64 in cells) == (n == 1)
    # all distinct / all equal / two alternating / first and last
    full = [r for r in short if r.g == form.gmax]
    assert any(len(r.grams) == r.g for r in full)
    assert any(len(r.grams) == 1 for r in full)
    assert any(len(r.grams) == min(2, form.gmax) and all(r.seq[i] == r.seq[i % 2] for i in range(r.g)) and r.seq[0] != r.seq[1 % r.g]
               for r in full if r.g > 1)
    assert any(r.seq[0] == r.seq[-1] and r.counts[r.grams.index(r.seq[0])] == 2 and len(r.grams) == r.g - 1 for r in full)
    # list sizes, and the three kinds of string at a block's two ends and at a list's end
    assert set(V.SHORT_LIST_SIZES) <= {len(s) for _, s in case.lists()}
    assert len(case.fit) % 16 not in (0, 1)
    kinds = {"empty": lambda r: r.raw == 0, "wave": lambda r: r.stage == "wave", "long": lambda r: r.stage == "long"}
    for kind, is_kind in kinds.items():
        assert any(is_kind(r) and i % 16 == 0 for i, r in enumerate(rows)), kind
        assert any(is_kind(r) and i % 16 == 15 for i, r in enumerate(rows)), kind
        assert any(is_kind(rows_of(case, which)[-1]) for which, _ in case.lists()), kind
    # the n-gram of key 0 is a term
    assert any(tuple([min(V.kept_alphabet(form, case.fit))] * n) in r.grams for r in rows)


# ---------------------------------------------------------------------------------------------------- (a) wave stage
@pytest.mark.parametrize("name", WAVE)
def test_wave_list_holds_every_wave_stage_edge(name):
    case = V.case(name)
    rows = rows_of(case)
    wave = [r for r in rows if r.stage == "wave"]
    assert set(V.WAVE_G) <= {r.g for r in wave}
    ends = [set(np.cumsum(r.counts).tolist()) for r in wave if r.g > 128 and min(r.counts) > 1]
    assert any({64, 128} <= e for e in ends)                                  # run-length steps that end exactly there
    for position in (64, 128):
        assert any(straddles(r, position) for r in wave), position
        assert sum(straddles(r, position) and len(r.grams) > 2 for r in wave) >= 1, position
    if not case.form.symbols:
        assert any(r.raw > 1040 and 0 < r.kept < 100 for r in wave)
    n = case.form.n
    assert any(r.kept == 1023 + n and r.g == 1024 for r in wave)
    assert any(r.kept == 1024 + n and r.stage == "long" for r in rows)
    if n == 3:
        assert {1026, 1027} <= {r.kept for r in rows}


@pytest.mark.parametrize("name", ["widest-n21a8-bytes", "widest-n21a8-symbols"])
def test_widest_keys_reach_the_character_limit_before_the_n_gram_limit(name):
    rows = rows_of(V.case(name))
    assert any(r.kept == 1040 and r.g == 1020 and r.stage == "wave" for r in rows)
    assert any(r.kept == 1041 and r.g == 1021 and r.stage == "long" for r in rows)


# ---------------------------------------------------------------------------------------------------- (a) long stage
@pytest.mark.parametrize("name", LONG)
def test_long_list_holds_every_long_stage_edge(name):
    case = V.case(name)
    rows = rows_of(case)
    long_ = [r for r in rows if r.stage == "long"]
    assert {1025, 1281} <= {r.g for r in long_} and len(long_) >= 2
    assert any(straddles(r, 256) and len(r.grams) == 2 for r in long_) and any(straddles(r, 256) and len(r.grams) > 2 for r in long_)
    assert {2048, 2049} <= {r.raw for r in long_}
    assert any(r.raw == 1100 and len(r.grams) == 1 and r.counts[0] == 1100 - case.form.n + 1 for r in long_)
    assert 4000 <= max(r.raw for r in rows) <= 4200
    if not case.form.symbols:
        assert any(r.raw == 2049 and r.kept == 1200 for r in long_)


def test_lists_are_small():
    for case in V.all_cases():
        for _, strings in case.lists():
            assert len(strings) <= 400 and max(map(len, strings)) <= 4200


# ---------------------------------------------------------------------------------------------------- (a) out of vocabulary
def unfitted_entries(case):
    alphabet = V.kept_alphabet(case.form, case.fit)
    vocabulary = {t for r in rows_of(case) for t in r.grams}
    rows = rows_of(case, "unfitted")
    ents = [V.entries(case.form, r, alphabet) for r in rows]
    return rows, ents, [V.missing_positions(e, vocabulary) for e in ents], alphabet, vocabulary


@pytest.mark.parametrize("name", SHORT + WAVE + LONG)
def test_unfitted_list_holds_the_kinds_of_missing_n_gram(name):
    case = V.case(name)
    form = case.form
    rows, ents, missing, alphabet, vocabulary = unfitted_entries(case)
    in_place = [any(t is not V.OOV and t not in vocabulary for t, _ in e) for e in ents]
    beyond = [sum(c for t, c in e if t is V.OOV) for e in ents]
    assert {"short", "wave", "long"} <= {r.stage for r, m in zip(rows, missing) if m}
    assert any(in_place) == (form.n > 1 or not form.local_alphabet)
    # sorted in place: a missing entry with entries that have a column on either side of it, in every stage (1-grams over
    # symbols cannot have one: every character the fit saw is a term)
    between = {r.stage for r, e, m in zip(rows, ents, missing)
               if any(e[p][0] is not V.OOV and set(range(p)) - set(m) and set(range(p + 1, len(e))) - set(m) for p in m)}
    assert between == ({"short", "wave", "long"} if form.n > 1 or not form.local_alphabet else set())
    unseen_character = [any(ch not in alphabet for t in r.grams for ch in t) for r in rows]
    assert sum(unseen_character) >= 6
    if form.local_alphabet:
        # one key, the last; several such n-grams in one short string; a string of nothing else
        assert all((b > 0) == u for b, u in zip(beyond, unseen_character))
        assert all(e[-1][0] is V.OOV and m[-1] == len(e) - 1 for e, m, b in zip(ents, missing, beyond) if b)
        assert any(b > form.n and r.stage == "short" and len(e) > 1 for r, e, b in zip(rows, ents, beyond))      # (one character: at most n)
        assert any(b and len(e) == 1 for e, b in zip(ents, beyond))
        # next to the n-gram of key 0, which is a term
        if name.startswith("short-"):
            lowest = tuple([min(alphabet)] * form.n)
            assert lowest in vocabulary and any(b and e[0][0] == lowest for e, b in zip(ents, beyond))
    else:
        assert not any(beyond)
    if form.n == 1:         # the tagged key's edge: 64 characters of which the last, in lane 63, is unseen
        assert any(r.raw == 64 and r.g == 64 and r.seq[-1][0] not in alphabet and all(c[0] in alphabet for c in r.seq[:-1]) for r in rows)


def test_missing_list_puts_missing_entries_at_every_listed_position():
    case = V.case("missing-n1-bytes")
    rows, ents, missing, alphabet, vocabulary = unfitted_entries(case)
    assert not case.form.local_alphabet
    one = [(m[0], len(e)) for e, m in zip(ents, missing) if len(m) == 1]
    assert set(V.MISSING_AT) <= {p for p, total in one if p < total - 1}                 # inside the row
    assert {15, 16, 31, 32} <= {p for p, total in one if p == total - 1}                 # as its last entry
    assert any(len(m) == 3 and m[0] == 0 and m[-1] == len(e) - 1 for e, m in zip(ents, missing))
    # rows without a column next to full rows within one wave of four
    empty = [len(m) == len(e) > 0 for e, m in zip(ents, missing)]
    full = [not m and len(e) > 16 for e, m in zip(ents, missing)]
    groups = [(sum(empty[i:i + 4]), sum(full[i:i + 4])) for i in range(0, len(rows), 4)]
    assert (2, 2) in groups and any(e == 3 and f == 1 for e, f in groups) and any(e == 1 and f == 3 for e, f in groups)


# ---------------------------------------------------------------------------------------------------- (a) K2
def test_k2_list_holds_every_row_length_and_the_late_n_gram():
    case = V.case("k2-n3-bytes")
    rows = rows_of(case)
    lengths = [len(r.grams) for r in rows]
    assert set(V.K2_ENTRIES) <= set(lengths)
    assert any(tuple(lengths[i:i + 4]) == V.K2_FOUR for i in range(0, len(rows), 4))
    sizes = [len(s) for _, s in case.lists()]
    assert all(any(k % m for k in sizes) for m in (4, 16, 64)) and all(len(case.fit) % m for m in (4, 16, 64))
    late = tuple(map(ord, V.LATE))
    where = [r.grams.index(late) for r in rows if late in r.grams]
    assert len(where) >= 4 and min(where) >= 16
    # ... and n-grams that are counted by both loops of the df count
    both = Counter()
    for r in rows:
        for k, t in enumerate(r.grams):
            both[t, k >= 16] += 1
    assert sum((t, False) in both and (t, True) in both for t, _ in both) > 20
    assert any(r.stage == "wave" and len(r.grams) == 100 for r in rows)


def test_common_list_has_an_n_gram_in_every_row():
    case = V.case("common-n3-bytes")
    rows = rows_of(case)
    common = tuple(map(ord, "q7q"))
    assert all(common in r.grams for r in rows) and any(r.counts[r.grams.index(common)] == 3 for r in rows)
    for dtype in V.DTYPES:
        _, vocab, idf = V.sklearn_reference(case.name, dtype)
        assert idf[vocab["q7q"]] == 1.0 and (idf[np.arange(len(idf)) != vocab["q7q"]] > 1.0).all()


def test_few_columns_list_takes_the_host_round_trip_first():
    """HipTfidfVectorizer installs the idf table on a first fit when documents + 1 <= 4 x columns; every other list here is
    on that side, this one is not."""
    from string_grouper_amd.vectorizer import HipTfidfVectorizer
    ratio = HipTfidfVectorizer.IDF_TABLE_RATIO
    for case in V.all_cases():
        columns = len({t for r in rows_of(case) for t in r.grams})
        assert (len(case.fit) + 1 > ratio * columns) == (case.name == "few-columns-n1-bytes"), case.name
    assert len(V.case("few-columns-n1-bytes").fit) == V.IDF_DOCS == 307


# ---------------------------------------------------------------------------------------------------- (b) two references
@pytest.mark.parametrize("dtype", V.DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("name", CASES)
def test_numpy_reference_equals_sklearn_bit_for_bit(name, dtype):
    case = V.case(name)
    mats, vocab, idf = V.sklearn_reference(name, dtype)
    got, got_vocab, got_idf = O.tfidf_numpy(case.fit, [s for _, s in case.lists()], dtype=dtype, **case.form.kw)
    assert got_vocab == vocab and np.array_equal(got_idf, idf) and got_idf.dtype == idf.dtype == dtype
    for (which, _), a, b in zip(case.lists(), got, mats):
        assert a.shape == b.shape and a.dtype == b.dtype == dtype
        assert not len(V.rows_that_differ(a, b)), which


# ---------------------------------------------------------------------------------------------------- (c) the mutants
def differing(name, dtype, **wrong):
    """{list: rows on which the mutant differs from the device's steps}; the device's steps equal sklearn on the way."""
    case = V.case(name)
    sets = [s for _, s in case.lists()]
    want = V.pipeline(case.form, case.fit, sets, dtype)
    mats, vocab, idf = V.sklearn_reference(name, dtype)
    assert want.vocabulary == vocab and np.array_equal(want.idf, idf)
    for a, b in zip(want.matrices, mats):
        assert a.shape == b.shape and not len(V.rows_that_differ(a, b))
    got = V.pipeline(case.form, case.fit, sets, dtype, V.Mutation(**wrong))
    out = {which: V.rows_that_differ(a, b) for (which, _), a, b in zip(case.lists(), got.matrices, want.matrices)}
    print(name, np.dtype(dtype).name, wrong, {k: len(v) for k, v in out.items()})
    return out, got, want


@pytest.mark.parametrize("name", ["short-n1-bytes", "short-n2-bytes", "short-n1-symbols", "short-n2-symbols"])
def test_dropping_the_n_gram_at_position_62_changes_the_short_list(name):
    """Every short row of more than 62 n-grams, which 1-grams and 2-grams alone can have: those of 63 and 64 distinct ones,
    the alternating one and the one that repeats its first at the end."""
    diff, _, _ = differing(name, F64, drop_position_62=True)
    rows = rows_of(V.case(name))
    hit = {i for i, r in enumerate(rows) if r.stage == "short" and r.g > 62 and len(r.grams) > 1}     # (one entry: 1.0 anyway)
    assert hit <= set(diff["fit"]) and len(hit) >= 4        # (and rows that share an n-gram whose df fell)


@pytest.mark.parametrize("name", ["short-n3-bytes", "short-n7-bytes", "short-n21a8-symbols"])
def test_ranks_without_the_tie_break_change_the_short_list(name):
    """Every short row with a repeated n-gram -- all equal, alternating, first and last among them."""
    diff, _, _ = differing(name, F32, ranks_without_tie_break=True)
    rows = rows_of(V.case(name))
    # (counts that are all equal, as where two n-grams alternate, leave the row what it is once it is normalised)
    hit = {i for i, r in enumerate(rows) if r.stage == "short" and len(set(r.counts)) > 1}
    assert set(diff["fit"]) == hit and len(hit) >= 3


@pytest.mark.parametrize("name", WAVE)
def test_restarting_runs_at_multiples_of_64_changes_the_wave_list(name):
    diff, _, _ = differing(name, F64, restart_runs_every=64)
    rows = rows_of(V.case(name))
    assert set(diff["fit"]) == {i for i, r in enumerate(rows) if r.stage == "wave" and any(straddles(r, p) for p in range(64, r.g, 64))}
    assert len(diff["fit"]) >= 3          # one run across 64 and 128, two runs of 99, runs of 20; not the runs of 32 and 64


@pytest.mark.parametrize("name", LONG)
def test_restarting_runs_at_multiples_of_256_changes_the_long_list(name):
    diff, _, _ = differing(name, F64, restart_runs_every=256)
    rows = rows_of(V.case(name))
    assert set(diff["fit"]) == {i for i, r in enumerate(rows) if r.stage == "long" and any(straddles(r, p) for p in range(256, r.g, 256))}
    assert len(diff["fit"]) >= 3


@pytest.mark.parametrize("name", ["short-n5a20-bytes", "short-n5a20-symbols", "short-n1-symbols", "short-n7-bytes"])
def test_an_out_of_alphabet_key_that_sorts_first_changes_the_unfitted_list(name):
    """Key 0 is a term (the n-gram of n lowest characters): every row with an unseen character gains or fattens its entry."""
    diff, _, _ = differing(name, F64, oov_sorts_first=True)
    case = V.case(name)
    rows, ents, missing, alphabet, vocabulary = unfitted_entries(case)
    assert set(diff["unfitted"]) == {i for i, e in enumerate(ents) if e and e[-1][0] is V.OOV} and len(diff["unfitted"]) >= 6
    assert not len(diff["fit"])


@pytest.mark.parametrize("dtype", V.DTYPES, ids=["float32", "float64"])
def test_dropping_the_entry_behind_a_missing_one_changes_the_missing_list(dtype):
    diff, _, _ = differing("missing-n1-bytes", dtype, drop_behind_missing=True)
    rows, ents, missing, alphabet, vocabulary = unfitted_entries(V.case("missing-n1-bytes"))
    hit = {i for i, (e, m) in enumerate(zip(ents, missing)) if any(p + 1 < len(e) and p + 1 not in m for p in m)}
    assert set(diff["unfitted"]) == hit and len(hit) >= 8


def test_a_df_that_counts_occurrences_changes_the_common_list():
    for dtype in V.DTYPES:
        diff, got, want = differing("common-n3-bytes", dtype, df_counts_occurrences=True)
        assert len(diff["fit"]) == len(V.case("common-n3-bytes").fit) == 23 and (got.idf != want.idf).sum() >= 1


def test_a_df_of_the_first_sixteen_positions_changes_the_k2_list():
    for dtype in V.DTYPES:
        diff, got, want = differing("k2-n3-bytes", dtype, df_first_sixteen_only=True)
        late = want.vocabulary[V.LATE]
        assert got.idf[late] != want.idf[late] and (got.idf != want.idf).sum() > 100
        assert len(diff["fit"]) >= 40


def test_summing_in_chunks_of_sixteen_changes_float64_rows_and_no_float32_row():
    """float64 pins the order of the additions (the squares fill the double's mantissa); the square of a float32 has 24 bits
    and a handful of them add up exactly in a double whatever the order."""
    changed = 0
    for name in ("k2-n3-bytes", "short-n3-bytes", "wave-n3-bytes"):
        diff, _, _ = differing(name, F64, sum_in_chunks_of_16=True)
        rows = rows_of(V.case(name))
        assert all(len(rows[i].grams) > 17 for i in diff["fit"])
        changed += len(diff["fit"])
        assert len(diff["fit"]) >= 10, name
    assert changed >= 40
    diff, _, _ = differing("k2-n3-bytes", F32, sum_in_chunks_of_16=True)
    assert not len(diff["fit"])


def test_a_float32_accumulator_changes_float32_rows():
    for name in ("k2-n3-bytes", "short-n3-bytes", "wave-n3-bytes"):
        diff, _, _ = differing(name, F32, float32_accumulator=True)
        assert len(diff["fit"]) >= 10, name


def test_a_longest_row_word_that_counts_tokens_is_too_large_on_the_unfitted_lists():
    for name in ("missing-n1-bytes", "short-n5a20-symbols", "wave-n3-bytes"):
        _, got, want = differing(name, F32, longest_row_counts_tokens=True)
        at = [w for w, _ in V.case(name).lists()].index("unfitted")
        assert got.longest[at] > want.longest[at] == int(np.diff(want.matrices[at].indptr).max()), name
        assert got.longest[0] == want.longest[0]


def test_sequential_norms_are_the_pipelines():
    for dtype in V.DTYPES:
        case = V.case("k2-n3-bytes")
        want = V.pipeline(case.form, case.fit, [case.fit], dtype)
        _, counts = O.count_matrix(case.fit, want.vocabulary, dtype, **case.form.kw)
        assert np.array_equal(V.sequential_norms(counts, want.idf).view(np.uint64), want.norms[0].view(np.uint64))
        assert (want.norms[0] == 0).sum() == 2
