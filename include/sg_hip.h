/* sg_hip.h -- C ABI of libsg_hip.so, the MI355X (gfx950) core for string_grouper's hot path.
 *
 * Boundary.  Every entry point replaces a call the reference makes
 * into a third-party native dependency from string_grouper/string_grouper.py (paths relative
 * to the reference tree):
 *
 *   seam b1  TfidfVectorizer(min_df=1, analyzer=n_grams, dtype).fit / .transform
 *            string_grouper.py:306 (construct), :699-707 (fit), :689-692 (transform)
 *            -> sg_strings_*, sg_vec_fit, sg_vocab_*, sg_vec_transform
 *   seam b2  sparse_dot_topn.sp_matmul_topn     string_grouper.py:725-732, :737-743
 *            -> sg_postings_build (the B.transpose() + CSC->CSR step) + sg_spgemm_topn,
 *               or the one-shot host mirror sg_sp_matmul_topn_host
 *            sparse_dot_topn.zip_sp_matmul_topn string_grouper.py:746
 *            -> sg_topn_zip
 *
 * Conventions
 *   - plain C, no torch / scipy types.  Pointers named d_* are DEVICE pointers (HBM), all other
 *     pointers are host pointers.  A caller that already owns device memory (e.g. a torch tensor's
 *     data_ptr()) uses the *_from_device constructors; nothing is copied and nothing is freed.
 *   - every function returns an sg_status; sg_last_error() gives a thread-local message.
 *     SG_ERR_OVERFLOW is what the Python layer turns into OverflowError, the one exception the
 *     reference handles around _build_matches (string_grouper.py:397-413).
 *   - calls are asynchronous on the context's HIP stream unless they return data to the host.
 *   - value type: SG_F32 or SG_F64 (the only two sparse_dot_topn accepts, string_grouper.py:18).
 *   - column/row indices are int32, row pointers int64.
 *   - result order ("sort" != 0): per row by (score descending, column ascending); ties at the
 *     top-n cut are resolved by that same order; values must be STRICTLY greater than threshold.
 */
#ifndef SG_HIP_H
#define SG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    SG_OK = 0,
    SG_ERR_BADARG = 1,
    SG_ERR_OOM = 2,       /* hipMalloc failed            -> MemoryError   */
    SG_ERR_OVERFLOW = 3,  /* index space exhausted       -> OverflowError */
    SG_ERR_HIP = 4,       /* any other HIP runtime error -> RuntimeError  */
    SG_ERR_NODEVICE = 5,  /* no gfx950 device visible    -> RuntimeError  */
    SG_ERR_UNSUPPORTED = 6
} sg_status;

enum { SG_F32 = 0, SG_F64 = 1 };

typedef struct sg_ctx sg_ctx;           /* one per (process, GPU): device, stream, scratch pool  */
typedef struct sg_strings sg_strings;   /* device-resident string column: bytes + int64 offsets  */
typedef struct sg_vocab sg_vocab;       /* fitted vocabulary: n-gram key -> column, df, idf       */
typedef struct sg_csr sg_csr;           /* device-resident CSR matrix                             */
typedef struct sg_postings sg_postings; /* device-resident inverted index of B (= B^T), bucketed
                                           by column tile for the LDS accumulator of the multiply */
typedef struct sg_topn sg_topn;         /* device-resident fixed-stride top-n result             */

/* ------------------------------------------------------------------ library / context */
const char *sg_last_error(void);
/* Bumped whenever a signature or a struct of this header changes (round 4: 2 -- row_step arguments of round 3, sg_stats
 * grew; round 5: 3 -- sg_stats.prune_scored; 4 -- sg_topn_transpose_select; 5 -- sg_csr_concat; 6 -- sg_csr_select_rows,
 * sg_topn_drop_columns, sg_device_upload; 7 -- sg_topn_concat_rows, sg_topn_forget, sg_topn_put_rows, sg_csr_take_rows,
 * sg_device_download; 8 -- sg_csr_row_norms, sg_csr_vectoriser_words, sg_csr_column_counts, sg_vec_reweigh; 9 --
 * sg_csr_pairs_dot; 10 -- sg_topn_rescore, sg_rescore_field; 11 -- sg_topn_union; 12 -- sg_topn_rescore_floors,
 * sg_matchlist_field_scores; 13 -- sg_topn_rescore_skip_empty; 14 -- sg_topn_rescore takes one sg_rescore_call, the two
 * entries of 12 and 13 are gone); a binding compares it with the value it was written for right after loading the library. */
#define SG_ABI_VERSION 14
int sg_abi_version(void);
int sg_device_count(int *count);
/* hip_stream: a hipStream_t to launch on (e.g. torch.cuda.current_stream().cuda_stream), or NULL
 * to let the library create its own non-blocking stream. */
int sg_ctx_create(int device, void *hip_stream, sg_ctx **out);
int sg_ctx_destroy(sg_ctx *ctx);
int sg_ctx_sync(sg_ctx *ctx);
/* Release cached scratch back to the driver. */
int sg_ctx_trim(sg_ctx *ctx);
/* Tuning switches (SG_PRUNE, SG_SYM, SG_PRUNE_DELTA ... -- README, "tuning knobs").  The library reads the SG_* variables
 * of the environment ONCE, in sg_ctx_create; afterwards only these calls change them (value NULL: unset), and nothing
 * inside an API call looks at the environment.  sg_ctx_options writes the active set as NAME=VALUE lines into buf and
 * returns the bytes needed (0-terminated); sg_ctx_reset_options re-reads the environment (test hook).  Not to be
 * called while another thread has a call in flight on the same context.
 * Among the switches that select an earlier form of a kernel: SG_DEAL=floor -- the pruned multiply
 * deals a wave's lanes to a row's prefix terms with the remainders dropped, as it did before the largest-remainder rule. */
int sg_ctx_set_option(sg_ctx *ctx, const char *name, const char *value);
int sg_ctx_reset_options(sg_ctx *ctx);
int sg_ctx_options(sg_ctx *ctx, char *buf, int64_t len);

/* ------------------------------------------------------------------ strings (input of seam b1) */
/* Arrow large_string layout: string i = bytes[offsets[i] .. offsets[i+1]). */
int sg_strings_from_host(sg_ctx *ctx, const uint8_t *bytes, const int64_t *offsets, int64_t n,
                         sg_strings **out);
int sg_strings_from_device(sg_ctx *ctx, const uint8_t *d_bytes, const int64_t *d_offsets, int64_t n,
                           int64_t total_bytes, sg_strings **out);
/* A column whose characters the host has already lower-cased, regex-deleted and ranked into the alphabet of the fit
 * (n-grams over non-ASCII code points: normalize_to_ascii=False, string_grouper.py:202, :373-374): symbols[i] is the
 * rank of a character in the sorted alphabet of alphabet_size characters, 0xFFFF = "not in the alphabet" (only in a
 * later transform); offsets count symbols.  All columns of one fit must share the alphabet. */
int sg_strings_from_host_symbols(sg_ctx *ctx, const uint16_t *symbols, const int64_t *offsets, int64_t n,
                                 int32_t alphabet_size, sg_strings **out);
/* Byte column: the host has already applied str.lower() (rows with non-ASCII characters go through the host, whose
 * NFKD step can produce upper-case ASCII that must stay: 'TM' from U+2122); the device then leaves A-Z alone. */
int sg_strings_set_prelowered(sg_strings *s, int32_t prelowered);
int sg_strings_free(sg_strings *s);

/* ------------------------------------------------------------------ seam b1: vectoriser */
typedef struct {
    int32_t ngram_size;         /* StringGrouperConfig.ngram_size (string_grouper.py:189)         */
    int32_t ascii_lower;        /* != 0: map 'A'-'Z' to 'a'-'z' on the device (ignore_case)       */
    int32_t dtype;              /* SG_F32 / SG_F64  (tfidf_matrix_dtype)                          */
    int32_t reserved;
    uint8_t delete_table[128];  /* != 0: ASCII byte removed before n-gramming (the regex, :376)   */
} sg_vec_params;

/* TfidfVectorizer.fit(concat(sets)): learns the vocabulary (column = rank of the n-gram in
 * code-point order, exactly sklearn's sorted vocabulary) and the document frequencies.
 * Bytes >= 0x80 are dropped (== .encode('ascii','ignore') after the host's NFKD).
 * Returns SG_ERR_BADARG with "empty vocabulary" if no n-gram exists at all. */
int sg_vec_fit(sg_ctx *ctx, const sg_strings *const *sets, int32_t n_sets, const sg_vec_params *params,
               sg_vocab **out);
/* The two halves of sg_vec_fit, for a caller that shards the strings over several GPUs: every rank tokenises ITS
 * block (begin), the dense document-frequency tables are summed across ranks (sg_vocab_df_table gives the device
 * pointer: key_space int32 counters, e.g. for an RCCL all-reduce), and every rank derives the same vocabulary
 * from the summed table (end; n_docs_total = documents over all ranks, it enters the idf).
 * *shareable == 0: the keys are coded with the alphabet of the local strings (ngram_size > 3) and the table
 * must not be combined with another rank's -- fit on the whole column instead. */
int sg_vec_fit_begin(sg_ctx *ctx, const sg_strings *const *sets, int32_t n_sets, const sg_vec_params *params,
                     sg_vocab **out);
int sg_vocab_df_table(sg_vocab *v, int32_t **d_table, int64_t *n_entries, int32_t *shareable);
int sg_vec_fit_end(sg_ctx *ctx, sg_vocab *v, int64_t n_docs_total);
int sg_vocab_size(const sg_vocab *v, int64_t *n_terms, int64_t *n_docs);
/* How the keys of this vocabulary are coded: bits per character; != 0 if fitted on symbol columns; != 0 if the
 * vocabulary is the sorted key array (keys wider than 30 bits) instead of the dense table. */
int sg_vocab_coding(const sg_vocab *v, int32_t *bits_per_char, int32_t *symbols, int32_t *sorted_mode);
/* keys[i]: the n-gram of column i, its character codes packed big-endian bits_per_char bits each (sg_vocab_coding);
 * a code is the rank of a symbol in the caller's alphabet (symbol columns) or indexes sg_vocab_byte_alphabet (byte
 * columns: the identity for n-grams of up to 3 characters).  df[i]: its document count. */
int sg_vocab_to_host(sg_ctx *ctx, const sg_vocab *v, uint64_t *keys, int64_t *df);
int sg_vocab_byte_alphabet(const sg_vocab *v, uint8_t *byte_of_code /* 128 */, int32_t *n_codes);
/* idf is computed by the caller from df (numpy, sklearn's exact op sequence text.py:1664-1679,
 * so that log() is bit-identical) and installed here; dtype must match params.dtype. */
int sg_vocab_set_idf(sg_ctx *ctx, sg_vocab *v, const void *idf, int32_t dtype);
/* The same without the round trip (round 4).  idf of a term depends on its document count and the number of documents
 * only -- idf = f(df; n_docs) -- so the caller hands the library, ONCE per (n_docs, dtype), the table f(0 .. n_docs) made
 * with its own numpy (n_docs + 1 values; sg_ctx_put_idf_table, kept by the context, a handful of them), and every later fit
 * over as many documents weights its terms on the device: idf[column] = table[df[column]] (sg_vocab_apply_idf_table;
 * *applied == 0: the context has no table for this vocabulary's n_docs and dtype -- put one, or use sg_vocab_set_idf).
 * A fit() then needs neither sg_vocab_to_host nor an upload; keys and counts still come to the host when asked for. */
int sg_ctx_put_idf_table(sg_ctx *ctx, int64_t n_docs, int32_t dtype, const void *table);
int sg_vocab_apply_idf_table(sg_ctx *ctx, sg_vocab *v, int32_t *applied);
int sg_vocab_free(sg_vocab *v);
/* TfidfVectorizer.transform(strings): counts -> *idf -> row L2 normalise, CSR with sorted indices.  The matrix also keeps,
 * per row, the norm it was divided by (sg_csr_row_norms): with it the whole count behind an entry can be recovered, which is
 * what sg_vec_reweigh needs. */
int sg_vec_transform(sg_ctx *ctx, const sg_vocab *v, const sg_strings *strings, sg_csr **out);
/* The idf refreshed from resident rows, no string read again: what TfidfVectorizer(vocabulary=<v's n-grams>, ...).fit(docs)
 * .transform(docs) gives when m holds the rows of docs under v's CURRENT idf.  The caller counts the documents per column
 * (sg_csr_column_counts of m: K2 names a column once per row), derives the idf from them with its own numpy (as for
 * sg_vocab_set_idf, so that log() stays sklearn's) and hands both over: df_host and idf_host hold one entry per column of the
 * vocabulary, n_docs is the number of rows behind them (rows without entries count, as sklearn counts them), dtype the type
 * of idf_host.  *out is a NEW matrix that owns its arrays -- its own copy of row pointers and indices, made by the
 * vectoriser, with row norms -- in which every entry is (count * idf_new[col]) / the row's new norm, rounded as
 * sg_vec_transform rounds; m is only read (indexes borrow its arrays) and may be a row-block view.  On success df, n_docs and
 * the idf of v are the new ones: sg_vocab_to_host reports them and later transforms weight with them.
 * The count behind an entry is recovered as rint(v * norm / idf_old[col]) and CHECKED: made again from the count it must
 * give the entry's bits.  One synchronisation (the number of entries that failed the check comes back).
 * Refusals install nothing and leave v as it was:
 *   SG_ERR_BADARG       m carries no row norms (it is no sg_vec_transform / sg_vec_reweigh matrix, nor a concatenation or row
 *                       selection of such); m's columns are not v's; dtype is not v's and m's; an idf entry that is not
 *                       positive and finite;
 *   SG_ERR_UNSUPPORTED  an entry failed the check (m was made under another idf than v holds now): silently different
 *                       numbers are never an outcome. */
int sg_vec_reweigh(sg_ctx *ctx, sg_vocab *v, const sg_csr *m, const int32_t *df_host, int64_t n_docs, const void *idf_host,
                   int32_t dtype, sg_csr **out);

/* ------------------------------------------------------------------ CSR objects */
int sg_csr_from_host(sg_ctx *ctx, int64_t n_rows, int64_t n_cols, const int64_t *indptr,
                     const int32_t *indices, const void *data, int32_t dtype, sg_csr **out);
/* (A wrapped matrix is read where it lies.  The library keeps what it derives from a matrix WITH the sg_csr object --
 *  its properties, and from 65 536 rows the groups of identical rows a one-sided sg_spgemm_topn multiplies once -- so the
 *  arrays must not be rewritten while the object lives: wrap the new contents in a new object instead, as for an index.) */
int sg_csr_from_device(sg_ctx *ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *d_indptr,
                       const int32_t *d_indices, const void *d_data, int32_t dtype, sg_csr **out);
int sg_csr_dims(const sg_csr *m, int64_t *n_rows, int64_t *n_cols, int64_t *nnz, int32_t *dtype);
int sg_csr_device_ptrs(const sg_csr *m, const int64_t **d_indptr, const int32_t **d_indices,
                       const void **d_data);
int sg_csr_to_host(sg_ctx *ctx, const sg_csr *m, int64_t *indptr, int32_t *indices, void *data);
/* *d_norms: DEVICE array of m's rows doubles, the norm each row was divided by when sg_vec_transform (or sg_vec_reweigh) made
 * it, 0.0 for a row without entries; owned by m (a row-block view points into its parent's).  NULL when the matrix carries
 * none: sg_csr_from_host / sg_csr_from_device matrices, a concatenation with such a part, sg_csr_take_rows' result. */
int sg_csr_row_norms(const sg_csr *m, const double **d_norms);
/* The three words the vectoriser may leave with a matrix (violations = 0, the largest squared row norm rounded up as float
 * bits, the longest row) on the host; *present == 0: the matrix carries none (words = 0).  A synchronisation. */
int sg_csr_vectoriser_words(sg_ctx *ctx, const sg_csr *m, uint32_t *words /* 3 */, int32_t *present);
/* counts_host[c] = entries of m that name column c, for c in [0, n_cols): the number of rows that hold the column when no row
 * names a column twice (what sg_vec_transform guarantees).  Any CSR, a row-block view and a caller-made matrix included
 * (entries whose column lies outside [0, n_cols) are passed over).  One pass over the column indices, one synchronisation. */
int sg_csr_column_counts(sg_ctx *ctx, const sg_csr *m, int32_t *counts_host /* n_cols */);
/* Rows [r0, r1) as a view (no copy); the parent must outlive the view.  (A view derives its own groups of identical
 * rows when it is multiplied; it never shares the parent's.) */
int sg_csr_row_block(sg_ctx *ctx, const sg_csr *m, int64_t r0, int64_t r1, sg_csr **out);
/* The rows of parts[0], then parts[1], ... in one new matrix that owns its arrays: scipy's vstack of transformed blocks
 * (the reference stacks result blocks with it, string_grouper.py:750; vstack of master_matrix's rows and the transform of
 * new strings is the host analogue of growing a master list).  Every part has the same n_cols and dtype (SG_ERR_BADARG
 * otherwise); a part may be a row-block view, have no rows, or rows without entries; the parts are only read and may be
 * freed once the call has returned and the context's stream has passed it (sg_csr_free after the call is safe: the pool
 * is stream-ordered).  One pass on the device, nothing is read back.  When every part was made by sg_vec_transform the
 * result counts as made by it too (cosine-like by construction: the pruned multiply needs no scan of it), and the words
 * the vectoriser left with the parts are merged; when every part carries row norms (sg_csr_row_norms) so does the result.
 * More than INT32_MAX rows: SG_ERR_OVERFLOW. */
int sg_csr_concat(sg_ctx *ctx, const sg_csr *const *parts, int32_t n_parts, sg_csr **out);
/* m without the rows d_drop_sorted[0 .. n_drop) in a new matrix that owns its arrays: scipy's m[keep] with keep the
 * complement of the list (what a master list that forgets rows does to master_matrix on the host; the reference has no such
 * operation, it refits).  d_drop_sorted: DEVICE memory (sg_device_upload), row numbers of m ascending and distinct, each in
 * [0, n_rows) -- anything else is SG_ERR_BADARG, seen on the device before anything is copied.  A kept row's new number is
 * its old one minus the dropped rows before it.  m may be a row-block view and may have rows without entries; n_drop == 0 is
 * a copy, n_drop == n_rows a matrix without rows.  The kept rows between two dropped ones are contiguous in m, so the copy is
 * sg_csr_concat's over the gaps: one pass at the width of that kernel however the dropped rows lie.  One synchronisation:
 * the number of kept entries comes back to size the result.  m is only read and may be freed after the call, as the parts
 * of sg_csr_concat.  A matrix made by sg_vec_transform stays one (cosine-like by construction); the words the vectoriser
 * left are carried over and are then UPPER bounds: the largest norm and the longest row may have been dropped.  The kept
 * rows' norms (sg_csr_row_norms) are carried over as well. */
int sg_csr_select_rows(sg_ctx *ctx, const sg_csr *m, const int32_t *d_drop_sorted, int64_t n_drop, sg_csr **out);
/* The rows d_rows[0 .. n_rows) of m, in that order, in a new matrix that owns its arrays: scipy's m[rows] (what a caller who
 * has to multiply a few rows of master_matrix again does to it on the host; the reference has no such operation, it multiplies
 * every row again).  d_rows: DEVICE memory, row numbers of m in any order, a row may be named more than once; a number outside
 * [0, m's rows) is SG_ERR_BADARG, seen on the device before anything is copied.  m may be a row-block view and may have rows
 * without entries; n_rows == 0 is a matrix without rows.  Every taken row is a part of sg_csr_concat's copy, which runs at its
 * usual width.  One synchronisation: the number of entries comes back to size the result.  m is only read and may be freed
 * after the call.  A matrix made by sg_vec_transform stays one, as in sg_csr_select_rows, and the words the vectoriser left
 * are carried over as UPPER bounds.  Row norms (sg_csr_row_norms) are NOT carried: the result has none. */
int sg_csr_take_rows(sg_ctx *ctx, const sg_csr *m, const int32_t *d_rows, int64_t n_rows, sg_csr **out);
int sg_csr_free(sg_csr *m);

/* Row-wise similarity of two matrices of the same shape (StringGrouper.dot / compute_pairwise_similarities,
 * string_grouper.py:433-440: np.asarray(master_matrix.multiply(duplicate_matrix).sum(axis=1))):
 * out_host[i] = sum over the common columns of A[i, k] * B[i, k], products rounded to the value type and
 * added in the order scipy + numpy use (ascending column; first + pairwise sum of the rest), so the result
 * is bit-identical.  out_host: n_rows values of the matrices' type.  Rows must be sorted by column. */
int sg_csr_rowwise_dot(sg_ctx *ctx, const sg_csr *A, const sg_csr *B, void *out_host);

/* The similarity of NAMED row pairs: out_host[p] = (A . B^T)[d_left[p], d_right[p]], the element of sp_matmul_topn's product
 * (string_grouper.py:725-743) for that pair -- and the pair form of compute_pairwise_similarities (string_grouper.py:55), which
 * has to be handed the two rows of every pair as strings and vectorises them again.  A is n_a x V, B is n_b x V, of the same
 * value type; they may be the same handle.  d_left, d_right: DEVICE arrays (sg_device_upload) of n_pairs row numbers, d_left[p]
 * in [0, n_a), d_right[p] in [0, n_b); any order, a pair or a row may be named any number of times.  out_host: n_pairs values
 * of the matrices' type, in the order of the pairs.
 * The value is defined to the bit, and it is the MULTIPLY's, not sg_csr_rowwise_dot's: acc = +0.0, and for every column k that
 * both rows hold, in ascending k, acc = rn(acc + rn(A[i, k] * B[j, k])) -- every product and every sum rounded to the value
 * type on its own, zero products added like the others (a lone product of -0.0 gives +0.0).  No common column, or a row
 * without entries: +0.0.  Every pair (i, j, score) that sg_spgemm_topn reports for the same matrices is reproduced bit for
 * bit.  Values of any sign, NaN and inf flow through: this call has no gate.
 * Refusals leave out_host untouched:
 *   SG_ERR_BADARG   the matrices differ in their columns or in value type (seen on the host); an index outside its matrix, or
 *                   a row NAMED BY A PAIR whose columns are not strictly ascending (seen on the device: one status word, a
 *                   bit a cause, which comes back with the results -- the message names the causes).  A matrix made by
 *                   sg_vec_transform, or one the multiply's gate has found cosine-like, is known to be sorted and is not
 *                   checked again.
 *   SG_ERR_OVERFLOW more than 2^36 pairs in one call.
 * n_pairs == 0: SG_OK, nothing is read or written.  One launch, one read-back (the call's only synchronisation). */
int sg_csr_pairs_dot(sg_ctx *ctx, const sg_csr *A, const sg_csr *B, const int32_t *d_left, const int32_t *d_right,
                     int64_t n_pairs, void *out_host);

/* ------------------------------------------------------------------ seam b2: sparse top-n multiply */
/* Inverted index of B (n_right x V): for every term k the (row j, value) pairs, grouped by column
 * tile j / tile_cols.  tile_cols must be a power of two supported by the multiply (0 = default).
 * The postings keep a reference to B's arrays (the multiply re-scores candidates against B's rows, and an index over
 * all rows is built from them on demand when a multiply asks for more than 64 columns per row of an index over groups of
 * identical rows): B MUST stay alive -- and unchanged -- until the postings are freed.
 * What B may hold.  Every row of B must name a column ONCE: a row with the same column in two entries is refused with
 * SG_ERR_BADARG (scipy keeps such entries; sum them first, sum_duplicates()) -- in the index they would be two postings of
 * one row in one segment, and the exact multiply adds a segment's products without looking for that.  The call sees it
 * where it scans B anyway, and in a row that is not in ascending column order by a second look at such rows.  Nothing
 * else is a precondition: values of any sign, zeros, NaN and inf, rows in any column order and of any norm are accepted,
 * and decide only WHICH kernel multiplies -- the pruned kernels take a matrix whose values are all >= 0 (-0.0 and
 * denormals included; NaN is not), whose rows are in strictly ascending column order and whose largest squared row norm
 * is <= 1.0001; any other matrix, on either side of the product, takes the exact kernel.  The result is the same bits
 * either way. */
int sg_postings_build(sg_ctx *ctx, const sg_csr *B, int32_t tile_cols, sg_postings **out);
/* The same with options.  SG_POSTINGS_NO_PERMUTATION: by default the index is built over a fixed permutation of B's rows
 * (a sorted name list has its similar names side by side, which piles a row's candidates into a few column tiles: the
 * pruned multiply ran 2.6 x slower on 663 k sorted names than on the same names shuffled); results never show it --
 * rows, columns and the order of equal scores are B's own.  (The ranges of the multi-GPU self-join form,
 * sg_selfjoin_range, are ranges of positions then: sg_postings_permutation.) */
enum { SG_POSTINGS_NO_PERMUTATION = 1 };
int sg_postings_build_flags(sg_ctx *ctx, const sg_csr *B, int32_t tile_cols, int32_t flags, sg_postings **out);
int sg_postings_free(sg_postings *p);

/* C = topn_rowwise(A . B^T restricted to > threshold).  A: n_left x V, postings of B: n_right x V.
 * Row i of the result holds counts[i] <= top_n entries at [i*top_n, i*top_n + counts[i]).
 * On every A and every index sg_postings_build accepted the result is, bit for bit, what sparse_dot_topn's row-wise
 * product gives on the same arrays with A's rows in ascending column order: products and sums rounded separately in the
 * matrices' type, a pair kept when its score is > (type)threshold -- a NaN score never is, an inf score is and sorts
 * first --, score descending, then column ascending.  A may name a column twice in a row (both entries are multiplied,
 * as scipy would), hold values of any sign, NaN and inf, and rows of any norm; none of it is refused, and none of it
 * changes the numbers: it decides between the pruned and the exact kernel (sg_postings_build). */
int sg_spgemm_topn(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int32_t top_n, double threshold,
                   int32_t sort, sg_topn **out);
int sg_topn_dims(const sg_topn *r, int64_t *n_rows, int32_t *stride, int32_t *dtype, int64_t *n_cols);
int sg_topn_device_ptrs(const sg_topn *r, const int32_t **d_cols, const void **d_vals, const int32_t **d_counts);
int sg_topn_to_host(sg_ctx *ctx, const sg_topn *r, int32_t *cols, void *vals, int32_t *counts);
int sg_topn_counts_to_host(sg_ctx *ctx, const sg_topn *r, int32_t *counts);   /* the per-row counts only */
/* Upload a fixed-stride result held on the host (used to feed host CSR blocks to sg_topn_zip). */
int sg_topn_from_host(sg_ctx *ctx, int64_t n_rows, int64_t n_cols, int32_t stride, int32_t dtype,
                      const int32_t *cols, const void *vals, const int32_t *counts, sg_topn **out);
/* The same from DEVICE memory (a device-to-device copy on the context's stream): the multi-GPU path hands its all-gathered
 * blocks over without a trip through the host (string_grouper.py:750 vstack, on the device). */
int sg_topn_from_device(sg_ctx *ctx, int64_t n_rows, int64_t n_cols, int32_t stride, int32_t dtype,
                        const int32_t *d_cols, const void *d_vals, const int32_t *d_counts, sg_topn **out);
/* zip_sp_matmul_topn: parts[b] = A . B_b^T; columns of part b are offset by col_offsets[b]. */
int sg_topn_zip(sg_ctx *ctx, const sg_topn *const *parts, const int64_t *col_offsets, int32_t n_parts,
                int32_t top_n, sg_topn **out);
int sg_topn_free(sg_topn *r);

/* One-shot host mirror of sparse_dot_topn.sp_matmul_topn(A, B.T, top_n, threshold, sort):
 * uploads A and B (both CSR over the same V columns), multiplies, downloads.  out_* hold
 * n_left * top_n (cols, vals) and n_left counts. */
int sg_sp_matmul_topn_host(sg_ctx *ctx, int64_t n_left, int64_t n_right, int64_t n_cols,
                           const int64_t *a_indptr, const int32_t *a_indices, const void *a_data,
                           const int64_t *b_indptr, const int32_t *b_indices, const void *b_data,
                           int32_t dtype, int32_t top_n, double threshold, int32_t sort,
                           int32_t *out_cols, void *out_vals, int32_t *out_counts);

/* ------------------------------------------------------------------ match list (fit() tail) */
/* Device version of what fit() does with the multiply's result (string_grouper.py:417-431, :755-763):
 * fix_diagonal: every (r, r) := 1 (added when absent, :954-958); symmetrize: every stored (r, c) also
 * stored as (c, r) (:960-964); rows come back sorted by column.  With both flags 0 it is a plain
 * fixed-stride -> CSR compaction that keeps the within-row order unless sort_by_column is set (the
 * reference's vstack(..., dtype=np.float64) at :750 re-sorts the rows of a float32 result by column as a
 * side effect of scipy's up-cast; a float64 result keeps the multiply's order).  Entry i of row r is
 * (r, cols[row_ptr[r] + i], vals[...]). */
typedef struct sg_matchlist sg_matchlist;
int sg_matchlist_build(sg_ctx *ctx, const sg_topn *r, int32_t fix_diagonal, int32_t symmetrize,
                       int32_t sort_by_column, sg_matchlist **out);
int sg_matchlist_dims(const sg_matchlist *ml, int64_t *n_rows, int64_t *n_entries, int32_t *dtype);
int sg_matchlist_to_host(sg_ctx *ctx, const sg_matchlist *ml, int64_t *row_ptr, int32_t *cols, void *vals);
int sg_matchlist_free(sg_matchlist *ml);

/* The two reductions the reference runs over the match list, on the device: one int32 per string comes
 * back instead of the list.
 * sg_matchlist_best_master (match_most_similar, string_grouper.py:803-807: groupby('dupe_side') max
 *   similarity, then min master_side): out_best[c] = the row with the largest similarity in column c, the
 *   lowest such row among equals, -1 when the column has no entry.  out_best: n_cols of the list (host).
 * sg_matchlist_group_reps (group_similar_strings, string_grouper.py:851-904: scipy connected_components
 *   + group_rep): out_rep[i] = the representative of string i's group -- centroid == 0: the member with
 *   the lowest index ('first'); centroid != 0: the member with the largest row sum of similarities, the
 *   lowest index among equals.  Needs a square list (self-join).  out_rep: n_rows (host).
 * Both need similarities GREATER THAN 0 (what passed a threshold >= 0 is): sg_matchlist_best_master and the arg-max of
 *   the centroid compare the IEEE bit patterns of the values as unsigned integers, which orders positive values only. */
int sg_matchlist_best_master(sg_ctx *ctx, const sg_matchlist *ml, int32_t *out_best);
int sg_matchlist_group_reps(sg_ctx *ctx, const sg_matchlist *ml, int32_t centroid, int32_t *out_rep);

/* Cost estimate of every left row for load balancing across GPUs: out_cost[i] = number of
 * intermediate products row i generates = sum over its non-zeros of the posting-list length.
 * (The reference has no analogue: its n_blocks[0] split is by row count, string_grouper.py:714-722.) */
int sg_row_costs(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int64_t *out_cost);

/* Self-join across GPUs.  One GPU scores every pair (i, j) of a self-join once, from the row
 * with the larger index (half the work of the one-sided multiply the reference's n_blocks[0] split implies,
 * string_grouper.py:714-752).  Across ranks that form splits by LEFT-ROW RANGES of the same, replicated matrix:
 *
 * sg_selfjoin_range: the rows [row_lo, row_hi) of A against the columns j <= i.  A must be the matrix Bt was built
 *   from.  *out: a result object over ALL rows of A in which the rows of the range hold their matches j <= i (the
 *   other rows are empty); *d_pairs: the mirrored pairs -- that row i of the range matches row j < i, which may belong
 *   to another rank -- as *n_pairs records of *pair_words int32 words: {i, j, score bits} (f32) or {i, j, lo, hi} (f64);
 *   device memory owned by the library (sg_device_free).  *applicable == 0: the form cannot take this input (not
 *   cosine-like, top_n > 64, threshold too low, pair list full): nothing is returned and the caller uses
 *   sg_spgemm_topn on its rows.  All ranks must take the same branch.  (Rows the pruned kernel cannot take -- more
 *   than 128 non-zeros -- are scored by the exact kernel inside the same pass; they do not switch the form off.)
 * sg_selfjoin_merge: the pairs of ALL ranks, concatenated in any order, merged into the rows of the range of `res`:
 *   afterwards these rows equal the rows sg_spgemm_topn(A, Bt) would give, bit for bit.  The contract, for any result
 *   (sg_topn_from_host) and any record list (sg_device_upload), with no multiply in front of it:
 *   - the rank's rows: row j with row_lo <= pos_of[j] < row_hi and (row_hi - 1 - pos_of[j]) % row_step == 0 (row_step < 1
 *     counts as 1), pos_of being Bt's table row -> position.  Bt == NULL, or an index in row order: pos_of[j] = j;
 *   - a rank's row j receives the column i of every record {i, j, ...}, with the score whose bits the record carries;
 *   - repeats count once: a record that is in the list several times, and a record whose column i the row holds already;
 *   - the row's entries and what it receives are ordered by score descending BY VALUE (-0.0 and +0.0 are equal), then
 *     column ascending, whatever the order of the records; the first `stride` of the result stay, the row's count is
 *     their number, and the bits stored are the entry's own (the sign of a zero included);
 *   - every other row -- not the rank's, or named by no record -- keeps all its cells and its count;
 *   - n_pairs == 0, or row_lo == row_hi: nothing changes (d_pairs may be null when n_pairs is 0).
 *   Refused with SG_ERR_BADARG, nothing launched: null ctx or res, pair_words that do not match the result's value type
 *   (3 for SG_F32, 4 for SG_F64), a range outside [0, rows of res], and a result whose stride exceeds 128 -- a row is
 *   selected in at most two register lists of 64 (sg_selfjoin_range makes strides up to 64).
 *   The caller's responsibility, not checked: every count of res within [0, stride]; every record's j within [0, rows of
 *   res) (and a Bt over as many rows); the copies of a repeated record, and a record that repeats a stored column, carry
 *   the same score bits as the first -- the contract defines no winner among different scores of one column; no NaN.
 * When the index is built over the row permutation (the default, sg_postings_build_flags) a range is a range of
 *   POSITIONS: the rows it covers are orig_of[row_lo .. row_hi) (sg_postings_permutation; null tables = row order).
 *   Pass the same Bt to sg_selfjoin_merge.
 * row_step (round 3): a rank's share need not be contiguous -- with row_step = s it is the rows (positions) row_hi - 1,
 *   row_hi - 1 - s, row_hi - 1 - 2 s, ... >= row_lo.  Rank r of N takes (0, n - r, N): every rank then holds rows of every
 *   cost, the shares are equal without a cost model, and a share ends with its CHEAPEST rows like the whole pass does
 *   (a contiguous range of high positions ends with rows as expensive as its first: + 0.8 ms per range at 663 k).
 *   row_step <= 1: the contiguous range [row_lo, row_hi).  Pass the same triple to sg_selfjoin_merge / sg_topn_expand_range. */
int sg_selfjoin_range(sg_ctx *ctx, const sg_csr *A, const sg_postings *Bt, int32_t top_n, double threshold,
                      int64_t row_lo, int64_t row_hi, sg_topn **out, int32_t **d_pairs, int64_t *n_pairs,
                      int32_t *pair_words, int32_t *applicable, int64_t row_step);
int sg_selfjoin_merge(sg_ctx *ctx, sg_topn *res, const sg_postings *Bt, const int32_t *d_pairs, int64_t n_pairs,
                      int32_t pair_words, int64_t row_lo, int64_t row_hi, int64_t row_step);
/* Identical rows.  sg_postings_build indexes ONE representative per group of identical right-hand rows (identical
 * strings; option SG_COLLAPSE=0 switches it off) and sg_spgemm_topn expands its result to the caller's columns, so a
 * single GPU never sees the groups.  The self-join form over ranges does: with such an index
 *   - the ranges of sg_selfjoin_range are ranges of the GROUPS' positions, [0, *n_index_rows) of sg_postings_rows; the
 *     result objects and the permutation tables have one row per group (groups are numbered by ascending lowest member;
 *     *d_group_of_row: the group of every caller row, device memory of the index, null when nothing was grouped);
 *   - after sg_selfjoin_merge, sg_topn_expand_groups turns the rows of a rank's groups into the result rows of their
 *     MEMBERS: output row k is the caller's row d_rows[k] (device array of n_rows row numbers, each a member of a group
 *     whose row of `groups` is final; null = all rows), columns are the caller's -- bit for bit the rows
 *     sg_spgemm_topn(A, Bt) returns (sorted by score descending, then column ascending).  The tables it needs (groups'
 *     members) are part of the index every rank builds, so a rank expands its own groups without any exchange.
 * (The reference has no analogue: sparse_dot_topn multiplies every duplicate row again, string_grouper.py:728-752.) */
int sg_postings_rows(const sg_postings *Bt, int64_t *n_index_rows, int64_t *n_caller_rows, const uint32_t **d_group_of_row);
/* Bytes of the index the PRUNED multiply reads while it runs -- filter postings + their segment-end tables, the 8-bit
 * copies of the rows (second filter: the header and the 16-byte units a row's entries reach -- what is written and read, not
 * the 256 bytes a record is allocated at) and the packed rows (exact scoring) -- so that a measurement can say whether they
 * fit the 256 MiB Infinity Cache (bench.py: roofline.l3_resident).  0 for an index the pruned multiply does not use. */
int sg_postings_bytes(const sg_postings *Bt, int64_t *pruned_multiply_bytes);
int sg_topn_expand_groups(sg_ctx *ctx, const sg_postings *Bt, const sg_topn *groups, const int32_t *d_rows, int64_t n_rows,
                          sg_topn **out);
/* ... the same for the rows of the groups at the positions [pos_lo, pos_hi) -- a rank's range: the library makes the list
 * (ascending row numbers; *d_rows, *n_rows: device memory of the library, sg_device_free) and expands it. */
int sg_topn_expand_range(sg_ctx *ctx, const sg_postings *Bt, const sg_topn *groups, int64_t pos_lo, int64_t pos_hi,
                         sg_topn **out, int32_t **d_rows, int64_t *n_rows, int64_t pos_step);
/* device tables of Bt's row permutation, one entry per index row: position -> row, row -> position (both null: none) */
int sg_postings_permutation(const sg_postings *Bt, const uint32_t **d_orig_of, const uint32_t **d_pos_of);
int sg_device_free(sg_ctx *ctx, void *d_ptr);
/* bytes of host memory copied into device memory of the library (the context's pool; sg_device_free): how a caller hands
 * a small list to sg_csr_select_rows / sg_topn_drop_columns and keeps it resident between calls.  The host memory may be
 * reused once the call returns. */
int sg_device_upload(sg_ctx *ctx, const void *host, int64_t bytes, void **d_out);
/* ... and back: bytes of device memory of the library (a list a call returned, e.g. sg_topn_forget's rows) copied to the
 * host, behind everything the context's stream holds.  A synchronisation. */
int sg_device_download(sg_ctx *ctx, const void *d_ptr, int64_t bytes, void *host);

/* ------------------------------------------------------------------ resident corpus: the reverse path */
/* A corpus whose index stays on the device answers match_strings(corpus, new) / match_most_similar(corpus, new) -- the
 * reference's sp_matmul_topn(M, D.T, top_n, threshold) with top_n per MASTER row (string_grouper.py:725-732; top_n = 1 for
 * match_most_similar, :120) -- from the product computed the other way round, D . M^T: every new row against the corpus
 * index (sg_spgemm_topn with a cap that no row filled, so that it holds EVERY pair above the threshold).
 * sg_topn_transpose_select turns such a pair list into the result over the corpus rows: row m of *out holds the at most
 * top_n pairs (r, m) of `pairs` -- r a row of `pairs` -- ordered by score descending, then r ascending, as sg_spgemm_topn
 * orders and cuts a row (scores compare by VALUE: zeros of either sign are equal, as in the multiply, and the lower r goes
 * first; what is written out is the pair's own bits, the sign of a zero included); *out has n_rows_out rows,
 * pairs->n_rows columns and the stride min(top_n, columns).  The rows of
 * `pairs` must not name one column twice and its columns must lie in [0, n_rows_out).  top_n <= 2048 (larger:
 * SG_ERR_BADARG).  The result feeds sg_matchlist_build and sg_matchlist_best_master like a multiply's.  Bit for bit the
 * forward product's rows: a score is the sum of the separately rounded products of the shared terms in ascending term
 * order from either side.  (The reference has no analogue: it re-fits and re-multiplies the whole
 * master list every call, string_grouper.py:685-707.) */
int sg_topn_transpose_select(sg_ctx *ctx, const sg_topn *pairs, int64_t n_rows_out, int32_t top_n, sg_topn **out);
/* A corpus that has forgotten rows keeps them in its segments and indexes until the next compaction, so a product against
 * its index still names them.  sg_topn_drop_columns is scipy's C[:, keep] on a fixed-stride result, followed by the cut: per
 * row of r the entries whose column is in d_dead_sorted[0 .. n_dead) (DEVICE memory, ascending and distinct -- the caller's
 * responsibility, nothing is read back to check it) are dropped, every other column is lowered by the number of dead
 * columns below it, the order of the entries is kept and at most top_n of them stay; *out has r's rows, r's columns minus
 * n_dead and the stride min(top_n, r's stride) (top_n >= r's stride: nothing is cut).  Because a row of a product is ordered
 * by score descending, then column ascending, and the renumbering is monotonic, the rows of
 * sg_topn_drop_columns(sg_spgemm_topn(A, Bt, top_n + n_dead, ...), dead, top_n) are bit for bit those of
 * sg_spgemm_topn(A, index of sg_csr_select_rows(B, dead), top_n, ...): at most n_dead of the first top_n + n_dead entries
 * are dead.  No synchronisation. */
int sg_topn_drop_columns(sg_ctx *ctx, const sg_topn *r, const int32_t *d_dead_sorted, int32_t n_dead, int32_t top_n,
                         sg_topn **out);

/* ------------------------------------------------------------------ resident corpus: a self-join that is kept */
/* A corpus may keep the result of its own self-join -- sp_matmul_topn(M, M.T, top_n, threshold), string_grouper.py:725-729 --
 * on the device and edit it when rows join or leave instead of multiplying again.  Three operations on
 * whole rows of fixed-stride results do the editing; none of them looks at a score.
 *
 * sg_topn_concat_rows: the rows of parts[0], then parts[1], ... in one new result: scipy's vstack of result blocks
 * (string_grouper.py:750) without the trip through the host.  Every part has the same n_cols and dtype (SG_ERR_BADARG
 * otherwise); the strides may differ, *out has the largest; a part may have no rows; one part makes a copy.  The parts are only
 * read.  No synchronisation. */
int sg_topn_concat_rows(sg_ctx *ctx, const sg_topn *const *parts, int32_t n_parts, sg_topn **out);
/* sg_topn_forget: scipy's C[keep][:, keep] on a SQUARE result (rows and columns number the same strings; anything else is
 * SG_ERR_BADARG), keep the complement of d_dead_sorted[0 .. n_dead) (DEVICE memory, ascending and distinct, each in [0, rows)
 * -- the caller's responsibility as for sg_topn_drop_columns, whose filter of a row this call shares): the dead rows are left
 * out, the dead columns are dropped from every other row, rows and columns are lowered by the dead ones below them, the order
 * inside a row is kept; *out has r's stride.  A list longer than the 2 048 entries the kernel keeps in LDS is searched where it
 * lies.  *d_short_rows (device memory of the library, sg_device_free) holds, ascending and in the NEW numbering, the *n_short_rows
 * surviving rows that held top_n entries and hold fewer now: the only rows whose top_n over the surviving columns may hold
 * a pair that the cut had dropped -- a row with fewer than top_n entries held every pair above the threshold, and a full row
 * that named no dead column still holds its top_n.  One synchronisation: *n_short_rows comes back. */
int sg_topn_forget(sg_ctx *ctx, const sg_topn *r, const int32_t *d_dead_sorted, int32_t n_dead, int32_t top_n, sg_topn **out,
                   int32_t **d_short_rows, int64_t *n_short_rows);
/* sg_topn_put_rows: IN PLACE, row d_rows[k] of r becomes row k of src, k in [0, n_rows) with n_rows = src's rows (scipy:
 * C[rows] = S on a lil_matrix).  d_rows: DEVICE memory, distinct rows of r (the caller's responsibility; a number outside r is
 * passed over, nothing is read back).  src has r's n_cols and dtype and a stride not above r's, otherwise SG_ERR_BADARG.
 * No synchronisation. */
int sg_topn_put_rows(sg_ctx *ctx, sg_topn *r, const int32_t *d_rows, int64_t n_rows, const sg_topn *src);

/* ------------------------------------------------------------------ record matching: a result rescored on further fields */
/* A record has several fields (name, address, city ...), each with its own matrices.  sg_topn_rescore takes the candidates one
 * field's multiply found (or several fields' multiplies, united by sg_topn_union below) -- cand: R rows, N columns, stride S,
 * counts -- scores every one of them on F further fields, weighs
 * the scores into one, and filters, orders and cuts every row anew.  Candidates never leave the device.  (The reference has no
 * analogue: it matches one column of strings, string_grouper.py:55-153; its users combine fields in pandas.)  One call
 * description, sg_rescore_call below, says all of it: the plain statement first, then what floors and empty fields change.
 *
 * A field f = 1 .. F is two matrices A_f (the left records' rows) and B_f (the right records'; the same handle for a
 * self-join), a weight, and per side an optional list of dead PHYSICAL rows (DEVICE memory, ascending and distinct -- the
 * caller's responsibility): a resident corpus keeps removed rows in place, and result rows and columns count the live ones.
 * For row i of cand and entry e < counts[i], with j = cols[i, e] and s_0 = vals[i, e]:
 *   live -> physical   a = i + #{q : dead_a_f[q] - q <= i}, b likewise from j and dead_b_f (numpy: searchsorted(dead -
 *                      arange(len(dead)), live, side="right")); no list: a = i, b = j.
 *   field score        s_f = (A_f . B_f^T)[a, b] exactly as sg_csr_pairs_dot states it: ascending column, every product and
 *                      every sum rounded on its own, from +0.0.
 *   combined score     c = +0.0, then for f = 0 .. F in this order c = rn(c + rn(W_f * s_f)), W_f = (T)w_f with T the value
 *                      type and w_0 the weight of the score cand carries: no fused multiply-add, no wider accumulator --
 *                      numpy's acc = acc + W[f] * s[f] on arrays of type T.
 *   filter             kept when c > (T)threshold, the multiply's rule: a NaN never passes, an inf passes and sorts first.
 *   output row         row i of *out holds the kept entries by c descending (by VALUE: zeros of either sign are equal), then
 *                      j ascending, and the first min(top_n, S) of them stay; the bits written are c's own.
 * *out has R rows, N columns and the stride min(top_n, S); cand is only read.  The result feeds sg_matchlist_build like a
 * multiply's.
 *
 * Floors (`floors` not NULL): a floor a FIELD.  "The city must agree" is a condition on one field, not on the weighed sum: a
 * pair with name 1.0, address 1.0 and city 0.0 reaches 0.8 at weights 0.5 / 0.3 / 0.2.  (The reference has no analogue: it
 * matches one column of strings, string_grouper.py:55-153; its users filter per-field frames in pandas.)
 * floors[0] is the floor m_0 of the score cand carries (s_0 = vals[i, e], as it is), floors[f] the floor m_f of further field
 * f = 1 .. n_fields; a NaN means the field has no floor.  Everything is the plain statement's -- s_f, c, the order, the cut --
 * but the filter:
 *   filter             kept when c > (T)threshold AND s_f > (T)m_f for every field f with a floor.  Strict, as the threshold
 *                      is; a NaN score never passes a floor.  Floors act BEFORE the cut: the first min(top_n, S) of the
 *                      entries that passed stay.
 * A candidate that a floor refuses on field f is scored on no field f' > f: no row of B_f' is read for it.  So the column order
 * of a matrix not known to be sorted is looked at for the rows that are READ -- a row that only refused candidates name is not
 * looked at, and a call that the plain statement would refuse for that row is served.  A NaN that the data produces (no floor
 * on that field) refuses nothing by itself: the candidate is scored on, its c is a NaN and the filter drops it, as without
 * floors.  With every floor a NaN the result is the plain statement's to the bit.  A candidate's column is range-checked
 * before any floor is held against it: a column outside [0, N) refuses the call even where the primary's floor would have
 * refused the candidate.
 *
 * Empty fields (`skip_empty` not 0): a record's EMPTY fields left out of the score.  A blank address is an empty row: its score
 * is +0.0 and enters the weighed sum with its full weight, so two records with identical names and cities, one of them without
 * an address, reach 0.7 at weights 0.5 / 0.3 / 0.2; record linkage expects that a field unknown for a pair takes no part in
 * that pair and that its weight is shared among the fields that are known.  (The reference has no analogue: it matches one
 * column of strings, string_grouper.py:55-153; its users fill blanks with "" and combine fields in pandas.)
 * Field f = 0 .. n_fields is EMPTY FOR THE PAIR (i, j) when physical row a of A_f or physical row b of B_f has no entries:
 * indptr[a + 1] == indptr[a], a and b from the live numbers i and j through the field's dead lists as above.  A row that holds
 * entries is not empty whatever its values are (stored zeros included), and even if the product is 0.  Field 0 is the field
 * whose score cand carries: `primary` is its A, B and dead-row lists with the meaning they have in a further field (its weight
 * is ignored; only the row bounds are read: nothing is merged, so no column order is looked at and no status bit is added).
 * primary NULL: field 0 is never empty.  Floors as above; floors NULL: no field has a floor.  Everything is as above, floors
 * included -- s_f, W_f = (T)w_f, the order, the cut -- but:
 *   combined score     c  = +0.0;  for f = 0 .. F, f not empty for the pair:  c  = rn(c  + rn(W_f * s_f))
 *                      wp = +0.0;  for f = 0 .. F, f not empty for the pair:  wp = rn(wp + W_f)
 *                      wt = +0.0;  for f = 0 .. F:                            wt = rn(wt + W_f)
 *                      similarity = c                    when no field is empty for the pair: the bits of the call without
 *                                                        the option
 *                                 = rn(rn(c * wt) / wp)  when some are and wp > 0: ONE correctly rounded IEEE division in T, no
 *                                                        reciprocal, no fused step; the product with wt keeps min_similarity's
 *                                                        scale for weights that do not sum to 1
 *                                 = NaN                  otherwise (every field is empty, or the weights of the others do not
 *                                                        sum above 0): the pair is dropped
 *   floors             a floor on a field that is empty for the pair is NOT held against it -- the primary's included when
 *                      field 0 is empty; on the other fields floors act as before, ahead of the cut.
 *   filter, order, cut on `similarity`: kept when similarity > (T)threshold (strict, a NaN never passes), by value descending,
 *                      then column, the first min(top_n, S).
 * Nothing of B_f is read for a pair whose left row is empty in field f: the whole row of candidates skips that field; a pair
 * whose right row alone is empty is not merged either.  So, as with floors, column order is looked at for the rows that are READ.
 *
 * Refusals (SG_ERR_BADARG; nothing is returned, and the next call works):
 *   seen on the host     n_fields outside 1 .. 7; top_n < 1; S > 2048; a weight that is not finite (in T); a field whose
 *                        matrices differ from cand in value type, or from each other in columns; rows(A_f) - n_dead_a != R or
 *                        rows(B_f) - n_dead_b != N; a floor that is infinite; a primary without skip_empty; a primary that
 *                        the same checks refuse as an unweighed field (a null matrix, another value type, matrices that
 *                        differ in columns, rows(A) - n_dead_a != R or rows(B) - n_dead_b != N);
 *   seen on the device   a candidate column outside [0, N) -- nothing is read for it --, or a row of a field matrix that a
 *                        candidate reads whose columns are not strictly ascending, for matrices not known to be sorted (as
 *                        sg_csr_pairs_dot): one status word, a bit a cause, the call's only read-back. */
typedef struct {
    const sg_csr *A, *B;
    double weight;
    const int32_t *d_dead_a; /* NULL: none */
    int32_t n_dead_a;
    const int32_t *d_dead_b;
    int32_t n_dead_b;
} sg_rescore_field;
typedef struct {
    double w0;                       /* weight of the score cand carries */
    const sg_rescore_field *fields;  /* the further fields 1 .. n_fields */
    int32_t n_fields;
    const double *floors;            /* NULL: no floor; else n_fields + 1 of them, the carried score's first, NaN: none */
    int32_t skip_empty;              /* not 0: a field empty for a pair takes no part in it */
    const sg_rescore_field *primary; /* read with skip_empty only; NULL: field 0 is never empty; its weight is ignored */
    double threshold;
    int32_t top_n;
} sg_rescore_call;
int sg_topn_rescore(sg_ctx *ctx, const sg_topn *cand, const sg_rescore_call *call, sg_topn **out);
/* sg_topn_union: the candidates of SEVERAL fields' multiplies as one candidate result.  Two records that agree on address and
 * city but whose names fall below the candidate threshold are never compared when the names alone find the candidates; record
 * linkage takes the candidates from the union of several fields' matches instead.  (The reference has no analogue: it matches
 * one column of strings, string_grouper.py:55-153; its users unite per-field frames in pandas.)
 *
 * parts[0 .. P), P in 2 .. 8: fixed-stride results over the same records -- R rows, N columns, one value type; the strides S_p
 * may differ.  Of row i of part p the first clamp(counts_p[i], 0, S_p) entries count, as in sg_topn_rescore.  parts[0] is the
 * PRIMARY field's result and its values are that field's scores; of the other parts only the columns are read.  `primary`: the
 * primary field's A, B and dead-row lists with the meaning they have in sg_topn_rescore (its weight is ignored).
 *   row i of *out   the distinct columns that row i of any part names, in ascending column order; counts[i] is their number
 *                   (a column that one part names twice -- only a caller-made part can -- counts once).
 *   value of j      part 0's row i holds j: the bits of that entry, as they are (NaN, inf, the sign of a zero; named twice:
 *                   the entry at the lowest place).  Otherwise (A . B^T)[a, b] exactly as sg_csr_pairs_dot / sg_topn_rescore
 *                   state it -- a, b from the live numbers i, j through the dead lists, ascending column, every product and
 *                   every sum rounded on its own, from +0.0: what the primary multiply would have written for the pair.
 * *out has R rows, N columns, the parts' value type and the stride max(1, largest counts[i]), which comes back together with
 * the status word in the call's single read-back.  The parts are only read.  The result feeds sg_topn_rescore like a
 * multiply's (its rows are in column order, not score order: sg_topn_rescore orders anew).
 * Refusals (SG_ERR_BADARG; nothing is returned, and the next call works):
 *   seen on the host     n_parts outside 2 .. 8; parts that differ in rows, columns or value type; the sum of the S_p above
 *                        2048; a primary whose matrices differ from the parts in value type, or from each other in columns;
 *                        rows(A) - n_dead_a != R or rows(B) - n_dead_b != N;
 *   seen on the device   a counted column outside [0, N) -- nothing is read for it --, or a row of A or B that a filled
 *                        candidate reads whose columns are not strictly ascending, for a matrix not known to be sorted: one
 *                        status word, a bit a cause.
 * R x stride beyond the 32-bit result index: SG_ERR_OVERFLOW. */
int sg_topn_union(sg_ctx *ctx, const sg_topn *const *parts, int32_t n_parts, const sg_rescore_field *primary, sg_topn **out);
/* sg_matchlist_field_scores: which field carried a match.  A record call's list holds the weighed sum; this scores every entry
 * of a device-resident list on 1 to 8 fields, so that the frame can show a column a field.  (The reference has no analogue:
 * it matches one column of strings, string_grouper.py:55-153; its users join per-field frames in pandas.)
 *
 * ml: a list of R rows and N columns (sg_matchlist_build's; only read).  fields[0 .. n_fields): A_f, B_f and the dead-row
 * lists with the meaning they have in sg_topn_rescore; the weight is ignored.  out_host: [n_fields][n_entries] values of the
 * list's type, HOST memory.  Plane f holds, for every entry (i, j) of the list in list order, (A_f . B_f^T)[a, b] exactly as
 * sg_csr_pairs_dot states it -- a, b from the live numbers i, j through the dead lists, ascending column, every product and
 * every sum rounded on its own, from +0.0.  That holds for every entry, whatever the list's value there is: on the diagonal
 * that sg_matchlist_build sets to 1 the plane holds the field's own product (0 for an empty row), and a mirrored entry is
 * scored as the pair it names.  A list without entries is served: nothing is written.
 * Refusals (SG_ERR_BADARG; out_host is left as it was, and the next call works):
 *   seen on the host     n_fields outside 1 .. 8; a field whose matrices differ from the list in value type, or from each
 *                        other in columns; rows(A_f) - n_dead_a != R or rows(B_f) - n_dead_b != N;
 *   seen on the device   a column of the list outside [0, N) -- nothing is read for it --, or a row of a field matrix that an
 *                        entry reads whose columns are not strictly ascending, for matrices not known to be sorted: one
 *                        status word, a bit a cause, which comes back together with the planes in the call's only read-back.
 * More entries than one launch takes: SG_ERR_OVERFLOW. */
int sg_matchlist_field_scores(sg_ctx *ctx, const sg_matchlist *ml, const sg_rescore_field *fields, int32_t n_fields,
                              void *out_host);

/* ------------------------------------------------------------------ measurement */
enum { SG_K_TOKENIZE = 0, SG_K_WEIGHT = 1, SG_K_POSTINGS = 2, SG_K_SPGEMM = 3 /* the multiply's whole launch group */,
       SG_K_ZIP = 4, SG_K_VOCAB = 5, SG_K_SPGEMM_KERNEL = 6 /* its dominant kernel alone (pruned: the pruned kernel without
       the pair-list pass; exact: the exact launches) */, SG_K_COUNT = 7 };
typedef struct {
    float ms[SG_K_COUNT];     /* HIP-event time of the most recent launch group of each kernel      */
    int64_t macs;             /* intermediate products of the most recent sg_spgemm_topn            */
    int64_t spgemm_bytes;     /* its algorithmic bytes (stream model)                    */
    int64_t out_nnz;          /* entries kept by the most recent sg_spgemm_topn                     */
    /* the most recent multiply, when it took the pruned kernel (all zero otherwise):                */
    int64_t prune_rows;       /* left rows it processed                                             */
    int64_t prune_postings;   /* postings it streamed (of `macs` the exact kernel would)            */
    int64_t prune_survivors;  /* candidate pairs its first filter recorded (postings' upper bounds) */
    int64_t exact_rows;       /* left rows it handed to the exact kernel                            */
    int64_t prune_bytes;      /* its algorithmic bytes: 4 per posting streamed + the 8-bit copy of  */
                              /* a row per survivor + one packed row of B per pair scored exactly   */
                              /* (without the second filter: packed row + its two pointers per      */
                              /* survivor) + A + out                                    */
    int64_t prune_symmetric;  /* != 0: self-join form (every pair scored once, from the row with    */
                              /* the larger index, then both rows' lists built from the pair list)  */
    int64_t prune_scored;     /* pairs it scored EXACTLY: the survivors the second filter (an 8-bit */
                              /* copy of the candidate's row, round 5) let through; without that    */
                              /* filter (SG_Q8=0, terms beyond 24 bits) = prune_survivors           */
} sg_stats;
/* Waits for the recorded events, so it is a synchronisation point. */
int sg_ctx_stats(sg_ctx *ctx, sg_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* SG_HIP_H */
