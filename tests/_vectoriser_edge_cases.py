"""Constructed string lists, a plain restatement of what the device does with a string, and deliberately wrong references
("mutants") for the vectoriser's kernels (csrc/sg_vectorize.hip: K1, tokenise, and K2, weight and normalise).  TEST
INFRASTRUCTURE ONLY: no GPU and no library.  tests/test_vectoriser_edge_cases_cpu.py proves that every edge named below is
in the lists and that the lists tell every mutant from the reference; tests/test_vectoriser_edges_gpu.py feeds the same lists
to the kernels and expects sklearn's bits.

What the device does with a string (the restatement, `describe` and `entries`).  It receives the column that
strprep.prepare_column made: bytes (the device lower-cases A-Z, drops bytes >= 0x80 and the regex's bytes) or symbols
(lower-cased and deleted on the host: what arrives is what is kept).  A string of at most 64 RAW characters is tokenised by
tokenize_short_kernel (64 keys ranked lane to lane); a longer one by tokenize_kernel (one wave, up to 1 024 n-grams out of at
most 1 040 kept characters, run lengths in steps of 64 sorted positions); the rest by tokenize_long_kernel (steps of 256).
The row of a string is its distinct n-grams in sorted order with their counts; an n-gram with a character outside the fit's
alphabet -- where the alphabet is the fit's own: symbol columns, and byte columns with n-grams of four characters and more --
gets one key that sorts behind every other.  K2 drops the entries without a column and moves the rest up.

A form is a set of vectoriser options and an alphabet that lead to one kind of key (KEY FORMS below); every builder takes a
form, is seeded and cached: the tuples it returns are shared.
"""
import functools
from typing import NamedTuple

import numpy as np
import scipy.sparse as sp

from oracle import oracle as O
from string_grouper_amd import strprep as SP

DTYPES = (np.float32, np.float64)
SHORT_MAX = 64       # tokenize_short_kernel: raw characters of a string
WAVE_GRAMS = 1024    # TOK_CAP: n-grams one wave sorts
WAVE_CHARS = 1040    # TOK_CHARS: kept characters at which tokenize_kernel calls overflow
DELETED = " -.,"     # characters of the default regex

LOWER = "abcdefghijklmnopqrstuvwxyz"
DIGITS = "0123456789"
PUNCT = "!#$%&()*+:;<=>?@[]^_{|}"
NON_ASCII = "éñжд"   # lower-case, one code point in either case


# ===================================================================================================== key forms
class Form(NamedTuple):
    name: str
    n: int               # ngram_size
    chars: str           # the kept characters the strings are made of; every one of them is in every fitted list
    ignore_case: bool
    symbols: bool        # normalize_to_ascii=False and non-ASCII characters among `chars`: a symbol column
    bits: int            # per character, as the device codes them
    keys: str            # 'tagged32' (n * bits <= 25), 'plain32' (<= 30) or 'key64'
    unseen: str          # kept characters outside `chars`, for strings that were not fitted

    @property
    def kw(self):
        """The options, as oracle.ngrams and HipTfidfVectorizer both name them."""
        return dict(ngram_size=self.n, ignore_case=self.ignore_case, normalize_to_ascii=not self.symbols)

    @property
    def local_alphabet(self):
        """The characters are coded by rank among those of the fit: an unseen one makes the out-of-alphabet key."""
        return self.symbols or 7 * self.n > 24

    @property
    def gmax(self):
        """The n-grams of a string of 64 kept characters."""
        return SHORT_MAX - self.n + 1


def _bits(form_chars, n, symbols):
    if not symbols and 7 * n <= 24:
        return 7
    bits = 1
    while (1 << bits) < len(form_chars):
        bits += 1
    return bits


def _form(name, n, chars, ignore_case=True, symbols=False):
    if symbols:                                   # the last four characters give way to non-ASCII ones
        chars = chars[:-4] + NON_ASCII
    assert len(set(chars)) == len(chars)
    bits = _bits(chars, n, symbols)
    keys = "tagged32" if n * bits <= 25 else "plain32" if n * bits <= 30 else "key64"
    unseen = "~`" + ("ω" if symbols else "")
    return Form(name + ("-symbols" if symbols else "-bytes"), n, chars, ignore_case, symbols, bits, keys, unseen)


_A72 = LOWER + LOWER.upper() + DIGITS + PUNCT[:10]      # 72 characters in either case: 7 bits
_A36 = LOWER + DIGITS
_A50 = LOWER + DIGITS + PUNCT[:14]
_A20 = LOWER[:20]
_A8 = LOWER[:8]

FORMS = {f.name: f for symbols in (False, True) for f in (
    _form("n1", 1, _A72, ignore_case=False, symbols=symbols),      # 7 bits, tagged; 64 distinct 1-grams fit a string
    _form("n2", 2, _A36, symbols=symbols),                         # 14 (bytes) / 12 (symbols), tagged
    _form("n3", 3, _A36, symbols=symbols),                         # 21 / 18, tagged
    _form("n5a20", 5, _A20, symbols=symbols),                      # 5 x 5 = 25, tagged, the fit's own alphabet
    _form("n4a72", 4, _A72, ignore_case=False, symbols=symbols),   # 4 x 7 = 28: 32-bit keys without a tag
    _form("n5a50", 5, _A50, symbols=symbols),                      # 5 x 6 = 30
    _form("n7", 7, _A36, symbols=symbols),                         # 7 x 6 = 42: 64-bit keys
    _form("n21a8", 21, _A8, symbols=symbols),                      # 21 x 3 = 63: the widest key there is
)}
TOO_WIDE = dict(ngram_size=16, chars=LOWER[:16])                    # 16 x 4 = 64 bits: refused
BIG_FORMS = ("n3-bytes", "n7-bytes", "n3-symbols", "n7-symbols")    # the four (key width, column kind) pairs of a kernel


# ===================================================================================================== the restatement
class Row(NamedTuple):
    raw: int             # characters the device receives
    kept: int            # ... after lower-casing and deletion
    g: int               # n-grams
    seq: tuple           # the n-grams in string order, each a tuple of code points
    grams: tuple         # the distinct ones in sorted order
    counts: tuple
    stage: str           # 'short' | 'wave' | 'long'


@functools.lru_cache(maxsize=None)
def _default_delete_table():
    return SP.delete_table_for(O.DEFAULT_REGEX)


def _delete_table(form):
    return _default_delete_table()


def device_column(form: Form, strings):
    """The column as it reaches the device: what strprep.prepare_column makes, turned into symbols when the fit is a
    symbol fit (vectorizer._as_symbols)."""
    col = SP.prepare_column(np.asarray(list(strings), dtype=object), form.ignore_case, not form.symbols, O.DEFAULT_REGEX)
    if form.symbols and col.kind == "bytes":
        col = SP.bytes_column_to_symbols(col, form.ignore_case, _delete_table(form))
    assert col.kind == ("symbols" if form.symbols else "bytes")
    return col


def _kept_codes(form, col, i) -> list:
    """The code points of string i of a device column that survive lower-casing and deletion."""
    raw = col.data[col.offsets[i]:col.offsets[i + 1]]
    if col.kind != "bytes":
        return raw.tolist()
    b = raw
    if form.ignore_case and not col.prelowered:
        b = np.where((b >= 65) & (b <= 90), b + 32, b)
    b = b[b < 0x80]
    return b[_delete_table(form)[b] == 0].tolist()


def describe(form: Form, strings) -> tuple:
    """One Row per string."""
    col = device_column(form, strings)
    out = []
    for i in range(col.n):
        raw = int(col.offsets[i + 1] - col.offsets[i])
        kept = _kept_codes(form, col, i)
        g = max(len(kept) - form.n + 1, 0)
        seq = tuple(tuple(kept[j:j + form.n]) for j in range(g))
        grams = tuple(sorted(set(seq)))
        where = {t: k for k, t in enumerate(grams)}
        counts = [0] * len(grams)
        for t in seq:
            counts[where[t]] += 1
        stage = "short" if raw <= SHORT_MAX else "wave" if g <= WAVE_GRAMS and len(kept) <= WAVE_CHARS else "long"
        out.append(Row(raw, len(kept), g, seq, grams, tuple(counts), stage))
    return tuple(out)


OOV = None      # the out-of-alphabet key in a row's entries


def kept_alphabet(form, strings) -> frozenset:
    """Every kept character of the strings (also of those too short for an n-gram): the alphabet of a fit."""
    col = device_column(form, strings)
    return frozenset(c for i in range(col.n) for c in _kept_codes(form, col, i))


def device_bits(form, fit) -> int:
    """Bits per character of the keys of a fit on `fit`."""
    return _bits(kept_alphabet(form, fit), form.n, form.symbols)


def entries(form: Form, row: Row, alphabet) -> tuple:
    """The row as K1 leaves it: ((n-gram or OOV, count), ...) in the order of the keys.  With the fit's own alphabet every
    n-gram that holds a character outside it falls to the one key that sorts last."""
    out, beyond = [], 0
    for t, c in zip(row.grams, row.counts):
        if form.local_alphabet and any(ch not in alphabet for ch in t):
            beyond += c
        else:
            out.append((t, c))
    if beyond:
        out.append((OOV, beyond))
    return tuple(out)


def missing_positions(ents, vocabulary) -> tuple:
    """Sorted positions of a row's entries that have no column."""
    return tuple(k for k, (t, _) in enumerate(ents) if t is OOV or t not in vocabulary)


def term(t) -> str:
    return "".join(map(chr, t))


# ===================================================================================================== the pipeline, restated
class Mutation(NamedTuple):
    """One thing wrong; the default is the device."""
    drop_position_62: bool = False        # K1 short: the n-gram at string position 62 is lost
    ranks_without_tie_break: bool = False  # K1 short: equal keys take one rank: one entry each, every count 1
    restart_runs_every: int = 0           # K1 wave (64) / long (256): a new run at every multiple of the step
    oov_sorts_first: bool = False         # the out-of-alphabet key is 0: it joins the n-gram of n lowest characters
    drop_behind_missing: bool = False     # K2: the entry behind one without a column is overwritten, not moved up
    df_counts_occurrences: bool = False   # fit: df sums the counts
    df_first_sixteen_only: bool = False   # fit: sorted positions 16 and beyond of a row are not counted
    sum_in_chunks_of_16: bool = False     # K2: sixteen squares are summed first, the chunks then
    float32_accumulator: bool = False     # K2: the sum of squares kept in float32
    longest_row_counts_tokens: bool = False  # K2: the longest-row word counts entries before the missing ones are dropped


DEVICE = Mutation()


def _row_entries(form, row, alphabet, mut: Mutation):
    seq = list(row.seq)
    if mut.drop_position_62 and row.stage == "short" and len(seq) > 62:
        del seq[62]
    lowest = tuple([min(alphabet)] * form.n) if alphabet else None

    def key(t):
        if form.local_alphabet and any(ch not in alphabet for ch in t):
            return lowest if mut.oov_sorts_first else OOV
        return t
    keys = sorted((key(t) for t in seq), key=lambda t: (t is OOV, t or ()))
    step = mut.restart_runs_every
    if step and row.stage != {64: "wave", 256: "long"}[step]:
        step = 0
    out = []
    for i, t in enumerate(keys):
        if i and t == keys[i - 1] and not (step and i % step == 0):
            out[-1][1] += 1
        else:
            out.append([t, 1])
    if mut.ranks_without_tie_break and row.stage == "short":
        out = [[t, 1] for t, _ in out]
    return [(t, c) for t, c in out]


class Result(NamedTuple):
    matrices: tuple      # one scipy CSR per set
    norms: tuple         # one float64 array per set: what each row was divided by
    longest: tuple       # the longest-row word per set
    vocabulary: dict
    idf: np.ndarray


def pipeline(form: Form, fit, sets, dtype, mut: Mutation = DEVICE) -> Result:
    """fit(`fit`) and transform of every list of `sets`, in the device's steps and in its order of operations."""
    dtype = np.dtype(dtype).type
    fit_rows = describe(form, fit)
    alphabet = kept_alphabet(form, fit)
    fitted = [_row_entries(form, r, alphabet, mut) for r in fit_rows]
    terms = sorted({t for ents in fitted for t, _ in ents if t is not OOV})
    column = {t: k for k, t in enumerate(terms)}
    df = np.zeros(len(terms), np.int64)
    for ents in fitted:
        seen = set()
        for k, (t, c) in enumerate(ents):
            if t is OOV or (mut.df_first_sixteen_only and k >= 16):
                continue
            if mut.df_counts_occurrences:
                df[column[t]] += c
            elif t not in seen:
                df[column[t]] += 1
            seen.add(t)
    idf = O.idf_vector(df, len(fit), dtype)
    mats, norms, longest = [], [], []
    for strings in sets:
        indptr, indices, data, nrm, width = [0], [], [], [], 0
        for r in describe(form, strings):
            ents = _row_entries(form, r, alphabet, mut)
            cols = [column.get(t, -1) if t is not OOV else -1 for t, _ in ents]
            if mut.drop_behind_missing:
                keep = [c >= 0 and not (k and cols[k - 1] < 0) for k, c in enumerate(cols)]
            else:
                keep = [c >= 0 for c in cols]
            w = [dtype(dtype(c) * idf[col]) if ok else None for (t, c), col, ok in zip(ents, cols, keep)]
            sq = [float(dtype(x * x)) if x is not None else 0.0 for x in w]
            if mut.float32_accumulator:
                acc = np.float32(0)
                for s in sq:
                    acc = np.float32(acc + np.float32(s))
                acc = float(acc)
            elif mut.sum_in_chunks_of_16:
                acc = 0.0
                for lo in range(0, len(sq), 16):
                    part = 0.0
                    for s in sq[lo:lo + 16]:
                        part += s
                    acc += part
            else:
                acc = 0.0
                for s in sq:
                    acc += s
            norm = float(np.sqrt(np.float64(acc))) if acc != 0.0 else 0.0
            kept = [(col, x) for col, x in zip(cols, w) if x is not None]
            indices += [col for col, _ in kept]
            data += [dtype(float(x) / norm) for _, x in kept] if norm else [x for _, x in kept]
            indptr.append(len(indices))
            nrm.append(norm)
            width = max(width, len(ents) if mut.longest_row_counts_tokens else len(kept))
        mats.append(sp.csr_matrix((np.asarray(data, dtype), np.asarray(indices, np.int32), np.asarray(indptr, np.int32)),
                                  shape=(len(strings), len(terms))))
        norms.append(np.asarray(nrm, np.float64))
        longest.append(width)
    return Result(tuple(mats), tuple(norms), tuple(longest), {term(t): k for t, k in column.items()}, idf)


def value_bits(m):
    return m.data.view(np.uint32 if m.data.dtype == np.float32 else np.uint64)


def rows_that_differ(a, b) -> np.ndarray:
    """Rows of two CSR matrices whose columns or value BITS differ."""
    assert a.shape[0] == b.shape[0] and a.data.dtype == b.data.dtype
    bad = []
    for i in range(a.shape[0]):
        sa, sb = slice(a.indptr[i], a.indptr[i + 1]), slice(b.indptr[i], b.indptr[i + 1])
        if not (np.array_equal(a.indices[sa], b.indices[sb]) and np.array_equal(value_bits(a)[sa], value_bits(b)[sb])):
            bad.append(i)
    return np.asarray(bad, np.int64)


def sequential_norms(counts: sp.csr_matrix, idf: np.ndarray) -> np.ndarray:
    """Per row of a count matrix: the square root of the sum oracle.tfidf_weight_normalize forms -- the squares of
    count * idf, each rounded in the matrix's dtype, added one after the other in double.  0.0 for a row without entries."""
    dtype = counts.data.dtype.type
    w = counts.data * idf[counts.indices]
    sq = (w * w).astype(dtype).astype(np.float64).tolist()
    out = np.zeros(counts.shape[0], np.float64)
    for i in range(counts.shape[0]):
        acc = 0.0
        for s in sq[counts.indptr[i]:counts.indptr[i + 1]]:
            acc += s
        out[i] = np.sqrt(np.float64(acc)) if acc != 0.0 else 0.0
    return out


# ===================================================================================================== string makers
def _rng(form, what):
    return np.random.default_rng([sorted(FORMS).index(form.name), sum(map(ord, what))])


def distinct(form: Form, rng, length, avoid=(), chars=None) -> str:
    """`length` kept characters whose n-grams are all different (and none of them in `avoid`): every next character is the
    first of a shuffled alphabet that makes a new n-gram."""
    chars = list(chars or form.chars)
    n = form.n
    for _ in range(200):
        s, used = [], set(avoid)
        for _ in range(length):
            for c in rng.permutation(len(chars)):
                t = tuple(s[len(s) - n + 1:] + [chars[c]]) if n > 1 else (chars[c],)
                if len(s) < n - 1 or t not in used:
                    s.append(chars[c])
                    if len(s) >= n:
                        used.add(t)
                    break
            else:
                break
        if len(s) == length:
            return "".join(s)
    raise AssertionError(f"no string of {length} characters with distinct {n}-grams over {len(chars)} characters")


def spread(s: str, rng, raw_length: int) -> str:
    """`s` with deleted characters put in at random places until it has `raw_length` characters."""
    out = list(s)
    for _ in range(raw_length - len(s)):
        out.insert(int(rng.integers(len(out) + 1)), DELETED[int(rng.integers(len(DELETED)))])
    return "".join(out)


def some_upper(form, s: str, rng) -> str:
    """A fifth of the letters in upper case where the vectoriser ignores case."""
    if not form.ignore_case:
        return s
    return "".join(c.upper() if rng.random() < 0.2 else c for c in s)


def random_string(form, rng, length, chars=None) -> str:
    chars = list(chars or form.chars)
    return "".join(chars[i] for i in rng.integers(0, len(chars), length))


def wave_string(form, rng):
    return random_string(form, rng, 100)


def long_string(form, rng):
    return random_string(form, rng, 1100)


class Case(NamedTuple):
    name: str
    form: Form
    fit: tuple           # the fitted column
    others: tuple        # ((name, strings), ...): lists that are transformed without having been fitted

    def lists(self):
        return (("fit", self.fit),) + self.others


# ===================================================================================================== short stage
SHORT_LIST_SIZES = (1, 15, 16, 17, 33)


def short_g_cells(form):
    """The n-gram counts a short string of this form must show: 1 .. 5 (the rank loop runs to the next multiple of four),
    61 and 62 where 64 characters hold as many, and the two largest."""
    return sorted({1, 2, 3, 4, 5, form.gmax - 1, form.gmax} | {g for g in (61, 62) if g <= form.gmax})


@functools.lru_cache(maxsize=None)
def short_case(form_name) -> Case:
    form = FORMS[form_name]
    rng = _rng(form, "short")
    n, a, b = form.n, form.chars[1], form.chars[-1]
    edge = []
    # raw lengths (63 and 64 with distinct n-grams; 65 goes to the wave stage)
    edge += ["x" * 0, (form.chars * n)[:n - 1], distinct(form, rng, n), distinct(form, rng, 63), distinct(form, rng, 64),
             distinct(form, rng, 65)]
    # numbers of n-grams
    edge += [distinct(form, rng, g + n - 1) for g in short_g_cells(form)]
    # equal, alternating, first and last
    edge += [a * 64, (a + b) * 32]
    edge += [a * 30 + b * 34, b * 40 + distinct(form, rng, 24)]            # ... and counts that differ within a string
    head = distinct(form, rng, n)
    rest = [c for c in form.chars if c not in head]
    edge.append(head + distinct(form, rng, 64 - 2 * n, avoid=[tuple(head)], chars=rest if len(rest) > 2 else None) + head)
    if not form.symbols:
        # 64 raw characters of which all, all but n - 1, all but n are deleted; more than 64 raw characters, 64 and fewer kept
        edge += [spread("", rng, 64), spread((form.chars * n)[:n - 1], rng, 64), spread(distinct(form, rng, n), rng, 64),
                 spread(distinct(form, rng, 64), rng, 65), spread(distinct(form, rng, 30), rng, 200)]
    fill = [some_upper(form, distinct(form, rng, int(k)), rng) for k in rng.integers(max(n, 5), 65, 8)]
    fill += [random_string(form, rng, int(k)) for k in rng.integers(1, 65, 8)]
    names = edge + fill
    names.append(form.chars)                                    # every character of the form is in the fit
    names.append(min(form.chars) * (n + 1))                     # the n-gram of key 0
    if len(form.chars) > 64:
        names.append(form.chars[32:])
    # an empty string, one for the wave stage and one for the long stage as the first and the last of a block of sixteen
    at = {0: "", 15: wave_string(form, rng), 16: long_string(form, rng), 31: "", 32: wave_string(form, rng),
          47: long_string(form, rng)}
    order = [names[i] for i in rng.permutation(len(names))]
    out = []
    while order or any(k >= len(out) for k in at):
        out.append(at[len(out)] if len(out) in at else order.pop() if order else distinct(form, rng, 20))
    while (len(out) + 1) % 16 in (0, 1):
        out.append(distinct(form, rng, 20))
    out.append(long_string(form, rng))                          # ... and a long one as the last of the list
    others = tuple((f"head{k}", tuple(out[:k])) for k in SHORT_LIST_SIZES)
    others += (("unfitted", unfitted_strings(form, rng, out)),)
    return Case(f"short-{form.name}", form, tuple(out), others)


def swapped(s: str) -> str:
    """`s` with two different neighbouring characters near its middle exchanged: n + 1 n-grams change, the rest stay."""
    k = next(k for k in range(len(s) // 2, len(s) - 1) if s[k] != s[k + 1])
    return s[:k] + s[k + 1] + s[k] + s[k + 2:]


def unfitted_strings(form, rng, fit) -> tuple:
    """Strings that were not fitted.  Fitted strings of every stage with two characters exchanged: a few new n-grams over the
    fit's characters (no column, sorted in place among entries that have one).  n-grams with a character the fit never saw
    (with the fit's own alphabet: the key that sorts last), several of those in one short string, and the same in strings for
    the other two stages.  For 1-grams: 64 characters of which the last is unseen."""
    n, u, v = form.n, form.unseen[-1], form.unseen[0]
    rows = describe(form, fit)
    out = []
    longest = max(fit, key=len)
    for stage, cut in (("short", 40), ("wave", 300), ("long", None)):
        some = [swapped(s) for s, r in zip(fit, rows) if r.stage == stage and len(r.grams) > max(20, r.g // 2)][:2]
        out += some or [swapped(longest[:cut])]         # (a list without such a string: the head of its longest one)
    out += [distinct(form, rng, 40), random_string(form, rng, 30)]
    s = distinct(form, rng, 62)
    out += [s[:20] + u + s[20:40], u + s[:40], s[:40] + u, (s[:n + 1] + u + s[n + 1:n + 4] + v + s[n + 4:])[:64], u * 30, ""]
    if form.n == 1:
        out.append(distinct(form, rng, 63) + u)
    w, lg = wave_string(form, rng), long_string(form, rng)
    seen = next((f for f, r in zip(fit, rows) if r.stage == "short" and r.g >= 6), longest)[:n + 5]      # (its n-grams are terms)
    out += [w[:50] + u + w[50:], lg[:700] + v + lg[700:900] + u + lg[900:], min(form.chars) * n + seen + u + min(form.chars) * n, u]
    return tuple(out)


# ===================================================================================================== wave stage
WAVE_G = (64, 65, 128, 129, 512, 513, 1024)


def periodic(form, word, times) -> str:
    """`word` repeated, and its first n - 1 characters again: every cyclic n-gram of the word occurs exactly `times` times."""
    s = word * times
    return s + (word * form.n)[:form.n - 1]


@functools.lru_cache(maxsize=None)
def wave_case(form_name) -> Case:
    form = FORMS[form_name]
    rng = _rng(form, "wave")
    n, c = form.n, form.chars
    out = [random_string(form, rng, g + n - 1) for g in WAVE_G]
    out.append(periodic(form, c[:5], 32))           # five runs of 32: run-length steps end exactly at 64 and at 128
    out.append(periodic(form, c[5:8], 64))          # three runs of 64
    out.append(c[-1] * 200)                         # one run across 64 and 128
    out.append((c[2] + c[-2]) * 100)                # two runs of about 99: one across 64, one across 128
    out.append(periodic(form, c[:7], 20))           # runs of 20: one across 64 (60 .. 80), one across 128 (120 .. 140)
    if not form.symbols:
        out.append(spread(distinct(form, rng, 60), rng, 1100))      # more than 1 040 raw characters, fewer than 100 kept
    out.append(random_string(form, rng, WAVE_GRAMS + n - 1))        # 1 024 n-grams: the wave's last
    out.append(random_string(form, rng, WAVE_GRAMS + n))            # 1 025: the long stage's first
    out += [some_upper(form, random_string(form, rng, int(k)), rng) for k in rng.integers(65, 400, 6)]
    out.append(c)
    out = [out[i] for i in rng.permutation(len(out))]
    return Case(f"wave-{form.name}", form, tuple(out), (("unfitted", unfitted_strings(form, rng, out)),))


# ===================================================================================================== long stage
@functools.lru_cache(maxsize=None)
def long_case(form_name) -> Case:
    form = FORMS[form_name]
    rng = _rng(form, "long")
    n, c = form.n, form.chars
    out = [random_string(form, rng, 1025 + n - 1), random_string(form, rng, 1281 + n - 1),
           (c[3] + c[-3]) * 600,                    # two runs of about 599: the first across sorted position 256
           periodic(form, c[:9], 120),              # runs of 120: one across 256 (240 .. 360), 512, 768, 1 024
           random_string(form, rng, 2048), random_string(form, rng, 2049),
           c[0] * 1100,                             # one entry with a large count
           random_string(form, rng, 4100), c, distinct(form, rng, 30), ""]
    if not form.symbols:
        out.append(spread(random_string(form, rng, 1200), rng, 2049))
    out = [out[i] for i in rng.permutation(len(out))]
    return Case(f"long-{form.name}", form, tuple(out), (("unfitted", unfitted_strings(form, rng, out)),))


@functools.lru_cache(maxsize=None)
def widest_key_case(form_name) -> Case:
    """63-bit keys through the other two stages: 1 024 n-grams of 21 characters are 1 044 kept characters, so here the
    hand-over to the long stage is the character limit: 1 040 kept stay, 1 041 go on."""
    form = FORMS[form_name]
    assert form.n == 21
    rng = _rng(form, "widest")
    out = [random_string(form, rng, k) for k in (100, 300, WAVE_CHARS, WAVE_CHARS + 1, 1500)] + [form.chars, form.chars[0] * 300]
    return Case(f"widest-{form.name}", form, tuple(out), (("unfitted", unfitted_strings(form, rng, out)),))


# ===================================================================================================== K2
K2_ENTRIES = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100)
K2_FOUR = (1, 49, 0, 16)
LATE = "zzz"             # the n-gram that only occurs at sorted positions 16 and beyond


@functools.lru_cache(maxsize=None)
def k2_case() -> Case:
    """3-grams over a-y and digits.  Row e of K2_ENTRIES has e distinct n-grams; 'zzz', which sorts behind everything, ends
    rows of 17 and more entries and no other; 75 rows (3 mod 4, 11 mod 16 and mod 64); four consecutive rows of 1, 49, 0 and
    16 entries from row 8."""
    form = FORMS["n3-bytes"]
    rng = _rng(form, "k2")
    chars = [c for c in form.chars if c != "z"]

    def row(e, late=False):
        if e == 0:
            return "ab"
        if late:        # e - 3 n-grams, then ?zz... : '..z', '.zz', 'zzz' -- the last one sorts last
            return distinct(form, rng, e - 3 + 2, chars=chars) + LATE
        return distinct(form, rng, e + 2, chars=chars)
    rows = [row(e) for e in K2_ENTRIES if e < 17] + [row(e, late=(k % 2 == 0)) for k, e in enumerate(K2_ENTRIES) if e >= 17]
    rows += [row(e) for e in K2_ENTRIES if e >= 17][:3]
    rows += [row(int(e), late=e >= 20 and rng.random() < 0.5) for e in rng.integers(1, 60, 75 - 4 - len(rows))]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    rows[8:8] = [row(e) for e in K2_FOUR]
    assert len(rows) == 75
    sub = tuple(rows[:k] for k in (3, 5, 18, 66))
    return Case("k2-n3-bytes", form, tuple(rows), tuple((f"head{len(s)}", tuple(s)) for s in sub))


@functools.lru_cache(maxsize=None)
def common_case() -> Case:
    """Every row holds 'q7q': its document count is the number of documents and its idf exactly 1.  Repeats inside a row
    ('q7q7q7q': the n-gram three times), so that counting occurrences is not counting documents."""
    form = FORMS["n3-bytes"]
    rng = _rng(form, "common")
    chars = [c for c in form.chars if c not in "q7"]
    rows = [distinct(form, rng, int(k), chars=chars) + "q7q" * int(r) + distinct(form, rng, int(j), chars=chars)
            for k, r, j in zip(rng.integers(0, 30, 21), rng.integers(1, 4, 21), rng.integers(0, 30, 21))]
    rows.append("q7q7q7q")
    rows.append(form.chars)
    rows[-1] += "q7q"
    return Case("common-n3-bytes", form, tuple(rows), ())


IDF_DOCS, IDF_CHARS = 307, LOWER[:8]


@functools.lru_cache(maxsize=None)
def few_columns_case() -> Case:
    """307 documents over eight 1-grams: more documents than four times the columns, so the first fit of this many
    documents fetches the counts and weights them on the host, and the second finds a table on the device."""
    form = FORMS["n1-bytes"]
    rng = _rng(form, "few_columns")
    rows = [random_string(form, rng, int(k), chars=IDF_CHARS[:int(m)]) for k, m in
            zip(rng.integers(0, 40, IDF_DOCS), rng.integers(1, 9, IDF_DOCS))]
    rows[0] = IDF_CHARS
    return Case("few-columns-n1-bytes", form, tuple(rows), ())


# ===================================================================================================== out of vocabulary
MISSING_AT = (0, 15, 16, 31, 32)


@functools.lru_cache(maxsize=None)
def missing_case() -> Case:
    """1-grams over bytes (7 bits each, no alphabet of the fit's own: an unseen character sorts in place).  The fit sees the
    72 characters but three, one in the middle of their order; a row of the unfitted list with that one and p smaller
    characters has its missing entry at sorted position p.  Rows without a single column lie next to full rows in one group of
    four."""
    form = FORMS["n1-bytes"]
    rng = _rng(form, "missing")
    order = sorted(form.chars)
    gone = [order[36], order[0], order[-1]]
    seen = [c for c in order if c not in gone]
    below, above = [c for c in seen if c < gone[0]], [c for c in seen if c > gone[0]]
    fit = [random_string(form, rng, int(k), chars=seen) for k in rng.integers(1, 70, 30)] + ["".join(seen)]

    def shuffled(chars):
        chars = list(chars)
        return "".join(chars[i] for i in rng.permutation(len(chars)))

    def at(p, total):       # `total` distinct characters of which the p-th smallest has no column
        return shuffled(list(rng.choice(below, p, replace=False)) + [gone[0]] + list(rng.choice(above, total - p - 1, replace=False)))
    rows = [at(p, min(40, p + 30)) for p in MISSING_AT]
    rows += [at(p, p + 1) for p in (1, 15, 16, 31, 32)]                         # ... as the last entry
    rows += [at(3, 20), at(7, 8), shuffled(seen[20:60])]
    rows += [shuffled(below[:33] + [gone[0]]), shuffled(gone[:2] + seen[1:20]), shuffled(gone + seen[:50])]
    full, none = shuffled(seen[:40]), shuffled(gone * 5)
    rows = [full, none, full[:17], none[:3]] + rows + [none, none, none, full] + [none, full, full, full]
    rows += [shuffled(seen[:int(k)]) + gone[int(j) % 3] * int(j) for k, j in zip(rng.integers(1, 64, 9), rng.integers(0, 3, 9))]
    return Case("missing-n1-bytes", form, tuple(fit), (("unfitted", tuple(rows)),))


@functools.lru_cache(maxsize=None)
def all_cases() -> tuple:
    out = [short_case(f) for f in FORMS]
    out += [wave_case(f) for f in BIG_FORMS] + [long_case(f) for f in BIG_FORMS]
    out += [widest_key_case("n21a8-bytes"), widest_key_case("n21a8-symbols")]
    out += [k2_case(), common_case(), few_columns_case(), missing_case()]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name) -> Case:
    return {c.name: c for c in all_cases()}[name]


@functools.lru_cache(maxsize=None)
def sklearn_reference(name, dtype):
    """(matrices of the fitted column and of every other list, vocabulary, idf) by sklearn, computed once."""
    c = case(name)
    mats, vocab, idf = O.tfidf_sklearn(c.fit, [s for _, s in c.lists()], dtype=dtype, **c.form.kw)
    return tuple(sp.csr_matrix(m) for m in mats), vocab, idf


@functools.lru_cache(maxsize=None)
def norms_reference(name, dtype) -> tuple:
    """Per list of the case: what every row is divided by (sequential_norms of sklearn's counts under sklearn's idf)."""
    c = case(name)
    _, vocab, idf = sklearn_reference(name, dtype)
    return tuple(sequential_norms(O.count_matrix(s, vocab, dtype, **c.form.kw)[1], idf) for _, s in c.lists())
