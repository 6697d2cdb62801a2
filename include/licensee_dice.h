/*
 * licensee_dice.h -- C-ABI of the MI355X-native Dice scorer (gfx950 / HIP).
 *
 * Drop-in boundary for licensee's Dice matching hot path. The reference has no FFI for
 * this path (it is pure Ruby); every entry point below replaces a Ruby method and is what
 * a Ruby FFI binding attaches. Citations are to /root/reference:
 *
 *   dice_create / dice_destroy      replace the process-wide memoized template corpus:
 *                                   License.all(hidden: true, psuedo: false)   lib/licensee/license.rb:20-36
 *                                   + per-template wordset_fieldless / fields_normalized(_set) /
 *                                   length / spdx_alt_segments   lib/licensee/content_helper.rb:108-117,323-335
 *                                   lib/licensee/license.rb:273-283
 *   dice_match                      Dice#match + #confidence + the score loop of
 *                                   #matches_by_similarity        lib/licensee/matchers/dice.rb:8-14,34-53
 *                                   over License#similarity        lib/licensee/content_helper.rb:128-133,337-347
 *                                   with the CC filter of #potential_matches  dice.rb:23-31
 *   dice_similarity_matrix          Dice#matches_by_similarity / #licenses_by_similarity (full N x T
 *                                   scores + sorted top-k, no threshold cut)  dice.rb:34-41;
 *                                   also `licensee detect` "closest licenses" lib/licensee/commands/detect.rb:96-106
 *   dice_topk                       the first k entries of Dice#matches_by_similarity  dice.rb:34-41, which is
 *                                   all `licensee detect` reads for "closest licenses"  detect.rb:96-106
 *                                   (no N x T matrix is computed, stored or allocated)
 *   dice_*_sharded                  the same calls with the files sharded over several
 *                                   devices of one node (the dice.rb:34-41 loop is per file)
 *   dice_batch_*                    device-resident batch variants of the two calls above
 *                                   (inputs as bitsets or as word-id lists)
 *   dice_batch_projects             Project#license / #licenses / #matched_file over the license files of many
 *                                   projects at once                 lib/licensee/projects/project.rb:24-47,102-106,137-155
 *                                   on LicenseFile#license           lib/licensee/project_files/license_file.rb:84-98
 *   dice_last_error                 replaces the Ruby exceptions of the path (license.rb:258,
 *                                   content_helper.rb:230,310) with status codes + message
 *
 * Conventions
 *   - Caller owns every host buffer; the library owns all device memory inside a ctx/batch.
 *   - Every call returns DICE_OK (0) or a negative DICE_E_* code; dice_last_error() gives a
 *     thread-local message for the last failing call on this thread.
 *   - One ctx per host thread (no internal locking). Host-buffer calls are synchronous.
 *   - `stream` arguments are hipStream_t passed as void* (NULL = the ctx's own stream).
 *   - Bitsets: bit v of a word-set bitset is word-id v of the template vocabulary
 *     (word v lives in uint64 word v/64, bit v%64). Vocabulary = union of the templates'
 *     wordset_fieldless; words outside it cannot overlap and only count in |W_F|.
 *   - Results are bit-exact with the reference: overlap counts are exact integers, scores are
 *     IEEE-754 double (overlap*200.0)/denominator with Ruby's Integer floor division inside
 *     the denominator. Exact score ties (parity-unpinned in the reference, whose sort is not
 *     stable) resolve to the template LATER in key order.
 */
#ifndef LICENSEE_DICE_H
#define LICENSEE_DICE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DICE_OK 0
#define DICE_E_ARG (-1)       /* invalid argument / shape */
#define DICE_E_DEVICE (-2)    /* HIP runtime error or no usable gfx950 device */
#define DICE_E_NOMEM (-3)     /* host or device allocation failed */
#define DICE_E_STATE (-4)     /* call not valid in the current state */

#define DICE_TOPK_MAX 16

typedef struct dice_ctx dice_ctx;
typedef struct dice_batch dice_batch;

/* One entry per template, in License.all(hidden: true, psuedo: false) key order.
 * Input domain: length >= 0 (a character count) and |Lf| - |fields_normalized_set| >= 1 (with 0 an
 * empty file scores 0.0 / 0 in the reference); with the files scored against them, every
 * denominator |Lf| - |Fld| + |W_F| + adjusted length delta / 4 must fit int32. */
typedef struct dice_templates {
    int32_t n_templates;            /* T (>= 1)                                              */
    int32_t n_vocab;                /* V, bits per bitset (>= 1)                              */
    const uint64_t *lf_bits;        /* [T][dice_words64(V)]: wordset_fieldless (Lf) bitsets  */
    const uint32_t *lf_size;        /* [T] |Lf|            (content_helper.rb:130)            */
    const uint32_t *fields_set_size;/* [T] |fields_normalized_set| (content_helper.rb:131)    */
    const int32_t *length_slack;    /* [T] 5*max(fields_normalized.size, spdx_alt_segments)  */
                                    /*     (content_helper.rb:345); < 0 selects the simple   */
                                    /*     delta used when self is not a License (:343)      */
    const int32_t *length;          /* [T] content_normalized.length (characters)           */
    const uint8_t *is_cc;           /* [T] creative_commons? (license.rb:209-212)             */
} dice_templates;

/* A batch of candidate files (host memory). */
typedef struct dice_files {
    int64_t n_files;
    const uint64_t *bits;           /* [n][dice_words64(V)] row-major wordset bitsets        */
    const uint32_t *wordset_size;   /* [n] |W_F|: all distinct words, in or out of vocabulary */
    const int32_t *length;          /* [n] content_normalized.length (characters): >= 0, a     */
                                    /*     negative length is outside the input domain, as is  */
                                    /*     a denominator that does not fit int32 (above)       */
    const uint8_t *cc_false_positive; /* [n] potential_false_positive? (license_file.rb:80-82) */
} dice_files;

/* Number of uint64 words per bitset for a vocabulary of n_vocab words. */
int32_t dice_words64(int32_t n_vocab);

/* Upload a template corpus to `device` (HIP ordinal). Selects the kernel for the corpus
 * (template-specialized sparse program for T <= 64; postings kernels, LDS record kernel or
 * dense tiles above). */
int dice_create(const dice_templates *templates, int32_t device, dice_ctx **out);
void dice_destroy(dice_ctx *ctx);

/* Introspection: T, V, kernel kind (0 = dense, 1 = sparse program, 2 = LDS records,
 * 3 = postings), program entries. */
int dice_ctx_info(const dice_ctx *ctx, int32_t *n_templates, int32_t *n_vocab,
                  int32_t *kernel_kind, int32_t *program_entries);
/* Introspection: the kernel dice_match / dice_batch_match run -- the kernel kind above, or
 * 4 = bound-pruned match (kind 3 corpora; DICE_POST_PRUNE=0 keeps the postings kernels) --
 * or -1 for a NULL ctx. Results are identical whichever runs. */
int32_t dice_ctx_match_kernel(const dice_ctx *ctx);

/* Dice#match / #confidence for every file, synchronous, host buffers.
 *   best[i]    index of the matched template, or -1 (Dice#match nil) when the top
 *              score is below `threshold` or every template is CC-filtered;
 *   overlap[i] |Lf ∩ W_F| of the top-ranked template (0 if none);
 *   score[i]   similarity of the top-ranked template (0.0 if none) -- equals
 *              Dice#confidence when best[i] >= 0.
 * Any of the three output pointers may be NULL. */
int dice_match(dice_ctx *ctx, const dice_files *files, double threshold,
               int32_t *best, uint32_t *overlap, double *score);
/* Dice#match and Dice#confidence exactly as a caller of the matcher sees them
 * (dice.rb:8-14, 51-53): best[i] as dice_match; score[i] = Dice#confidence, i.e. the matched
 * template's similarity, or 0.0 when best[i] == -1; overlap[i] the matched template's overlap or 0.
 * The top-ranked template of an unmatched file is not computed, so the bound-pruned kernel
 * (T > 64) drops every template whose bound is below the threshold from the start. Equal to
 * dice_match's outputs on every matched file. */
int dice_match_confidence(dice_ctx *ctx, const dice_files *files, double threshold,
                          int32_t *best, uint32_t *overlap, double *score);

/* Full N x T similarity matrix + per-file top-k (Dice#matches_by_similarity order).
 *   overlap/score: [n][T] row-major, every template (CC filter NOT applied), may be NULL;
 *   topk_index/topk_score: [n][k] best-first among potential_matches (CC filter applied),
 *   -1 / -1.0 padding; k in [0, DICE_TOPK_MAX]. */
int dice_similarity_matrix(dice_ctx *ctx, const dice_files *files,
                           uint32_t *overlap, double *score,
                           int32_t k, int32_t *topk_index, double *topk_score);

/* The per-file top-k of dice_similarity_matrix alone (Dice#matches_by_similarity, dice.rb:34-41,
 * cut to its first k entries as `licensee detect` cuts it, detect.rb:96-106): topk_index/topk_score
 * [n][k] exactly as dice_similarity_matrix(k) fills them; k in [1, DICE_TOPK_MAX]. No N x T buffer
 * is allocated or written on the device. */
int dice_topk(dice_ctx *ctx, const dice_files *files, int32_t k, int32_t *topk_index, double *topk_score);

/* ---- one node, several devices: the files of one call sharded over contexts ----------
 * The loop of Dice#matches_by_similarity (dice.rb:34-41) is independent per file, so a call
 * splits its files into n_ctx contiguous shards (shard i = files [n*i/n_ctx, n*(i+1)/n_ctx)),
 * each scored by ctxs[i] on its own device, host thread and stream; templates are replicated
 * (every ctx must hold the same corpus: same T and V, checked; same bitsets, not checked).
 * Only results move:
 *   DICE_GATHER_HOST    every device copies its results straight into its disjoint slice of
 *                       the caller's buffers (parallel D2H);
 *   DICE_GATHER_DEVICE  every device copies its results into one buffer on ctxs[0]'s device
 *                       (peer copies over xGMI), then one D2H from there.
 * The device gather enables peer access (hipDeviceEnablePeerAccess) from every shard's device
 * to ctxs[0]'s first; where two devices have none the runtime stages the copy instead.
 * Shard rows given in pageable memory are staged through two page-locked buffers per ctx
 * (each shard thread copies its own slice), so the shards do not share the runtime's bounce
 * buffers. Several ctxs may share a device (tests on a one-GPU box); the same ctx twice is
 * DICE_E_ARG. Results are bit-identical to the single-ctx calls. Outputs as dice_match /
 * dice_similarity_matrix. */
#define DICE_GATHER_HOST 0
#define DICE_GATHER_DEVICE 1
int dice_match_sharded(dice_ctx *const *ctxs, int32_t n_ctx, const dice_files *files, double threshold,
                       int32_t gather_mode, int32_t *best, uint32_t *overlap, double *score);
/* dice_match_confidence's outputs (Dice#match + #confidence, dice.rb:8-14, 51-53), sharded. */
int dice_match_sharded_confidence(dice_ctx *const *ctxs, int32_t n_ctx, const dice_files *files,
                                  double threshold, int32_t gather_mode, int32_t *best, uint32_t *overlap,
                                  double *score);
int dice_similarity_matrix_sharded(dice_ctx *const *ctxs, int32_t n_ctx, const dice_files *files,
                                   int32_t gather_mode, uint32_t *overlap, double *score, int32_t k,
                                   int32_t *topk_index, double *topk_score);
/* dice_topk sharded (dice.rb:34-41 per file, detect.rb:96-106); bit-identical to the one-context call. */
int dice_topk_sharded(dice_ctx *const *ctxs, int32_t n_ctx, const dice_files *files, int32_t gather_mode,
                      int32_t k, int32_t *topk_index, double *topk_score);
/* The last sharded call on this thread: 1 = device gather, every shard on another device wrote
 * into ctxs[0]'s device through peer access; 0 = device gather with at least one such shard
 * through the runtime's staged copy; -1 = no peer path exercised: a host gather, a device gather
 * whose contexts all sit on ctxs[0]'s device, or no sharded call yet. */
int32_t dice_last_gather_peer(void);

/* ---- device-resident batches (inputs and results stay in HBM) ---------------------- */
int dice_batch_create(dice_ctx *ctx, int64_t capacity, dice_batch **out);
void dice_batch_destroy(dice_batch *batch);
/* H2D copy + on-device repack of host files into the kernel's tile layout. */
int dice_batch_upload(dice_batch *batch, const dice_files *files, void *stream);
/* The same files given as word-id lists instead of bitsets (CSR): file i's ids are
 * ids[offsets[i] .. offsets[i+1]) as uint16 (id_bytes 2) or uint32 (id_bytes 4) values; the
 * bitsets are built on the device. Ids >= n_vocab are ignored (words outside the template
 * vocabulary cannot overlap; they count only in wordset_size), duplicates are harmless.
 * offsets[0] = 0, non-decreasing (checked). For large vocabularies this moves a fraction of
 * the bitset bytes over the host link (600 synthetic templates: ~0.6 KB of u16 ids vs 2.9 KB
 * of bitset per file). Same entry point of the reference as dice_batch_upload. */
int dice_batch_upload_ids(dice_batch *batch, int64_t n_files, const int64_t *offsets, const void *ids,
                          int32_t id_bytes, const uint32_t *wordset_size, const int32_t *length,
                          const uint8_t *cc_false_positive, void *stream);
/* Kernel-only scoring of the resident batch, asynchronous on `stream`: no host synchronization
 * and no device-to-host copy inside (capturable in a hipGraph). For T > 64 corpora this is the
 * bound-pruned kernel followed by the postings kernels over the files it deferred; their count
 * stays on the device. */
int dice_batch_match(dice_batch *batch, double threshold, void *stream);
/* dice_match_confidence's semantics for a device batch (same asynchrony and capture contract). */
int dice_batch_match_confidence(dice_batch *batch, double threshold, void *stream);
/* Introspection after dice_batch_match (synchronizes `stream`): files the bound-pruned kernel
 * deferred to the postings kernels in the last call (0 for other kernels). */
int dice_batch_deferred(dice_batch *batch, int64_t *deferred, void *stream);
/* Introspection after dice_batch_match / dice_batch_match_confidence (synchronizes `stream`): the
 * (file, template) pairs whose overlap the last call computed exactly -- n * T for every kernel
 * but the bound-pruned one (T > 64 match), which scores only the templates whose bound reaches
 * the running best (or the threshold, confidence mode) and every pair of the files it deferred.
 * The pairs the bound rules out are decided without a score (dice.rb:34-48 only reads the top). */
int dice_batch_scored_pairs(dice_batch *batch, int64_t *pairs, void *stream);
/* Device-resident matrix results are template-major ([T][n] overlap/score, [k][n] top-k) so
 * every store is coalesced; dice_batch_download_matrix returns them row-major. */
int dice_batch_matrix(dice_batch *batch, int32_t k, void *stream);
/* The ranking of dice_batch_matrix(k) without the matrix (dice.rb:34-41 read for its first k entries,
 * detect.rb:96-106): fills the batch's top-k index and score buffers exactly as dice_batch_matrix(k)
 * does -- among potential_matches (CC filter applied), best first, the later template first on an
 * exact tie, -1 / -1.0 padding (also for k > T) -- and nothing else: only the [n][k] buffers are
 * allocated, the N x T buffers are neither allocated nor written, and the results of an earlier
 * dice_batch_match stay as they are. k in [1, DICE_TOPK_MAX] (DICE_E_ARG otherwise). Asynchronous on
 * `stream` with dice_batch_matrix's capture contract. */
int dice_batch_topk(dice_batch *batch, int32_t k, void *stream);
/* Bytes currently allocated for the batch's N x T overlap and score buffers: 0 until
 * dice_batch_matrix has run on the batch (dice_batch_topk never allocates them), -1 for NULL. */
int64_t dice_batch_matrix_bytes(const dice_batch *batch);
/* D2H of results (synchronizes `stream`); NULL outputs are skipped.
 * dice_batch_download_matrix: overlap/score are [n][T]; topk_index/topk_score are [n][k] and
 * `k` must equal the k of the last dice_batch_matrix / dice_batch_topk call on this batch (DICE_E_ARG
 * otherwise, so a caller's buffer is never written past its [n][k] extent). When that call was
 * dice_batch_topk the matrix on the device is absent or stale: a non-NULL overlap or score is
 * DICE_E_STATE, the top-k outputs work as ever.
 * dice_batch_download_topk (dice.rb:34-41, detect.rb:96-106): the [n][k] ranking, row-major whatever
 * the device layout is, after dice_batch_topk(k) or dice_batch_matrix(k) with k > 0; DICE_E_STATE
 * when the batch has had no ranking call, DICE_E_ARG for another k. */
int dice_batch_download_match(dice_batch *batch, int32_t *best, uint32_t *overlap,
                              double *score, void *stream);
int dice_batch_download_matrix(dice_batch *batch, uint32_t *overlap, double *score, int32_t k,
                               int32_t *topk_index, double *topk_score, void *stream);
int dice_batch_download_topk(dice_batch *batch, int32_t k, int32_t *topk_index, double *topk_score,
                             void *stream);
/* Device pointers of the match results (int32 best, uint32 overlap, double score). */
int dice_batch_result_ptrs(dice_batch *batch, void **best, void **overlap, void **score);
/* Diagnostic: stream-read the resident tiles with trivial compute (read-ceiling probe). */
int dice_batch_stream_probe(dice_batch *batch, void *stream);
/* Bytes of the resident tile layout per file (the kernel's algorithmic input stream). */
int64_t dice_batch_bytes_per_file(const dice_batch *batch);

/* ---- Matchers::Exact on the device --------------------------------------------------
 * Exact#match (exact.rb:6-12): the first template in key order (License.all, no CC filter)
 * whose wordset (content_helper.rb:108-110: Lf plus the field words, :323-335) equals the
 * file's. dice_exact_setup gives per template |wordset| ([T]), the field words that are
 * vocabulary words as bits (field_bits [T][dice_words64(V)], NULL = none) and the field words
 * outside the vocabulary as bits of the caller's numbering (field_need [T], NULL = none;
 * licensee_host.h lh_template_field_masks). Per file, file_field_mask[i] (host, [n]; NULL =
 * all zero) holds the same numbering's bits of the file's wordset (lh_prep_files).
 * exact[i] = template index or -1. The kernel reads the batch's row-major bitsets (the
 * stream probe overwrites them). dice_batch_exact is asynchronous on `stream`: the field masks
 * are copied from host memory on that stream, so they must stay valid until it has run.
 * file_field_mask = NULL reads the device's own masks only when the batch's last upload was
 * dice_batch_upload_text / dice_batch_upload_text_utf8 (as dice_batch_set_rows has patched them
 * since). After every other upload (dice_batch_upload, dice_batch_upload_ids, the sharded calls'
 * uploads) NULL means all zero for every file, whatever an earlier call or dice_batch_set_rows left
 * in the batch's mask buffer: those uploads carry no masks, so no file of the batch has one.
 * dice_exact_setup may be called again: the new tables replace the old ones for every batch of
 * the context, resident ones included. */
int dice_exact_setup(dice_ctx *ctx, const uint32_t *wordset_size, const uint64_t *field_bits,
                     const uint64_t *field_need);
int dice_batch_exact(dice_batch *batch, const uint64_t *file_field_mask, void *stream);
int dice_batch_download_exact(dice_batch *batch, int32_t *exact, void *stream);
int dice_exact(dice_ctx *ctx, const dice_files *files, const uint64_t *file_field_mask, int32_t *exact);

/* ---- ContentHelper#wordset on the device ----------------------------------------------
 * The wordset scan (content_helper.rb:108-110: /(?:[\w\/-](?:'s|(?<=s)')?)+/, ASCII \w) and its
 * interning into the batch's bitset rows, for texts already normalized (content_normalized,
 * content_helper.rb:153-168; licensee_host.h lh_normalize_files), so the host threads skip the
 * scan. dice_vocab_setup gives the context its vocabulary words in id order (n_words must equal
 * the V of dice_create; ASCII, distinct) and up to 64 extra words: the template field words
 * outside the vocabulary, numbered as licensee_host.h lh_template_field_masks numbers them, which
 * the scan reports as field-mask bits (what lh_prep_files' field_mask holds) instead of row bits.
 * A vocabulary of more than 251,904 words (dice_words64(V) > 3,936: the scan's workgroup would need
 * more than the 160 KiB of LDS a CU has) is refused with DICE_E_ARG. Measured on an MI355X under
 * ROCm 7.2.0: the launch with 160 KiB of dynamic LDS is granted without an opt-in attribute and
 * scans correctly (tests/test_gpu_words_edges.py, test_largest_vocabulary). */
int dice_vocab_setup(dice_ctx *ctx, int32_t n_words, const char *const *words, int32_t n_extra,
                     const char *const *extra);
/* The two facts of dice_vocab_setup's table a caller needs to aim an input at it; host code, no
 * context or device needed, and dice_vocab_setup itself calls both. dice_words_key_hash: the 64-bit
 * hash of a word's key (its first 16 bytes, its length and, past 16 bytes, the FNV-1a hash of the
 * rest). A word's home bucket is hash & (n_buckets - 1), its tag is hash >> 40 cut to 32 - id_bits
 * bits, and its home slot in a wave's set of non-vocabulary words is hash & 255.
 * dice_vocab_geometry: the table's bucket count (a power of two, 8 slots each) and the bits of a
 * slot's id field for n_total = n_words + n_extra words. */
int dice_words_key_hash(const uint8_t *word, int32_t len, uint64_t *hash);
int dice_vocab_geometry(int32_t n_total, int32_t *n_buckets, int32_t *id_bits);
/* text[0, text_bytes): the batch's normalized texts as bytes (every non-ASCII character one byte
 * >= 0x80), file i at text[offsets[i], offsets[i] + text_len[i]), offsets 16-byte aligned (the
 * last file may end exactly at text_bytes: no padding has to follow it);
 * length[i] = content_normalized.length in characters and cc_false_positive[i] as in dice_files.
 * The device builds each file's row, |W_F| (every distinct word, in the vocabulary or not) and
 * field mask (dice_batch_exact with file_field_mask = NULL reads them). Synchronizes `stream`.
 * status[i] (host, [n]) = 1 for a file with more distinct non-vocabulary words than the device
 * set holds (192); *n_overflow (may be NULL) counts them. Such a file's row is left empty: the
 * caller prepares it on the host (lh_prep_files) and sends it with dice_batch_set_rows before
 * scoring. Same entry point of the reference as dice_batch_upload (LicenseFile#wordset). */
int dice_batch_upload_text(dice_batch *batch, int64_t n_files, const uint8_t *text, int64_t text_bytes,
                           const int64_t *offsets, const int32_t *text_len, const int32_t *length,
                           const uint8_t *cc_false_positive, uint8_t *status, int64_t *n_overflow,
                           void *stream);
/* The same call for texts given as UTF-8 -- the bytes of content_normalized itself (licensee_host.h
 * lh_normalize_files_utf8, or a caller's own content_normalized): text_len[i] is in bytes. The scan
 * is the same one (its [\w/-] is ASCII and every byte >= 0x80 separates tokens), so rows, |W_F|,
 * field masks and status equal dice_batch_upload_text's for the same texts. length[i] is
 * content_normalized.length in characters, or length may be NULL: the device then counts each
 * file's characters (the bytes b of its text with (b & 0xC0) != 0x80; the bytes are trusted to be
 * UTF-8, not validated) on the same stream. The batch records that its texts are UTF-8, which
 * dice_batch_content_hash reads; every other upload clears the record. */
int dice_batch_upload_text_utf8(dice_batch *batch, int64_t n_files, const uint8_t *text, int64_t text_bytes,
                                const int64_t *offsets, const int32_t *text_len, const int32_t *length,
                                const uint8_t *cc_false_positive, uint8_t *status, int64_t *n_overflow,
                                void *stream);
/* D2H of the resident per-file lengths in characters ([n] int32), as the last upload of any kind
 * left them (the caller's, or the device's count); synchronizes `stream`. */
int dice_batch_download_length(dice_batch *batch, int32_t *length, void *stream);
/* Overwrite the rows, |W_F| and field masks (NULL: zero) of files index[0..k) of the resident
 * batch (bits: [k][dice_words64(V)]); synchronizes `stream`. The masks written here are read by
 * dice_batch_exact(file_field_mask = NULL) only in a batch whose last upload was a text upload,
 * where every other file has a device mask too; after any other upload that call takes all masks
 * as zero, these included (pass the whole batch's masks to dice_batch_exact instead). */
int dice_batch_set_rows(dice_batch *batch, int64_t k, const int64_t *index, const uint64_t *bits,
                        const uint32_t *wordset_size, const uint64_t *field_mask, void *stream);
/* Page-locked host memory (hipHostMalloc) for upload buffers -- texts, bitsets -- so their H2D
 * copies run at the link's rate and overlap the host; free with dice_host_free. */
int dice_host_alloc(int64_t bytes, void **out);
void dice_host_free(void *ptr);
/* D2H of the resident rows ([n][dice_words64(V)]), |W_F| and field masks (NULL outputs skipped;
 * the masks are those of the last dice_batch_upload_text / dice_batch_exact); synchronizes. */
int dice_batch_download_rows(dice_batch *batch, uint64_t *bits, uint32_t *wordset_size, uint64_t *field_mask,
                             void *stream);

/* ---- ContentHelper#content_hash on the device --------------------------------------------
 * content_hash (content_helper.rb:136-138: DIGEST.hexdigest content_normalized, SHA-1; one of
 * ProjectFile's HASH_METHODS, project_file.rb:17,97) of the texts dice_batch_upload_text left
 * or dice_batch_upload_text_utf8 left resident, one lane per file. After the UTF-8 upload the
 * resident bytes are content_normalized's, every digest is content_hash and every status is 0.
 * After dice_batch_upload_text a text with a non-ASCII character is resident with that character as
 * the byte 0x80, so its bytes are not the UTF-8 of content_normalized: such a file is flagged and
 * the caller hashes it.
 *
 * SHA-1 of every resident normalized text, asynchronous on `stream` (no host synchronization
 * inside). DICE_E_STATE unless the batch's last upload was one of the two text uploads
 * (dice_batch_set_rows and dice_batch_stream_probe leave the texts, and the record of their form,
 * as they are). */
int dice_batch_content_hash(dice_batch *batch, void *stream);
/* D2H (synchronizes `stream`; content_helper.rb:136-138): digest [n][20] bytes, status [n]:
 * 0 = digest is ContentHelper#content_hash of the file; 1 (dice_batch_upload_text only) = the text
 * holds a non-ASCII character (resident as 0x80), digest is of the resident bytes and the caller
 * hashes that file's UTF-8 itself.
 * NULL outputs are skipped; DICE_E_STATE if no hash was computed since the last upload. */
int dice_batch_download_content_hash(dice_batch *batch, uint8_t *digest, uint8_t *status, void *stream);

/* ---- Project#license on the device ------------------------------------------------------
 * Project#license, #licenses and #matched_file (projects/project.rb:24-47) for groups of the
 * resident files, with detect_readme and detect_packages false (the reference's default): project
 * p owns the files [offsets[p], offsets[p + 1]) of the batch, its license files in license_files
 * order before prioritize_lgpl (project.rb:54-66,111-117: name score descending, files that score
 * 0 already dropped by the caller). offsets is non-decreasing with offsets[0] == 0 and
 * offsets[n_projects] == the batch's file count; empty projects are legal.
 *   file_flags[i]      bit 0: the Copyright matcher matched the file (copyright.rb; the host's result)
 *                      bit 1: the name is a copyright? name          (project_file.rb:90-95)
 *                      bit 2: lesser_gpl_score(name) == 1            (license_file.rb:105-107)
 *   template_flags[t]  bit 0: gpl?, bit 1: lgpl?                     (license.rb:200-206)
 * License ids: 0 .. T-1 the templates, T = License 'other', T + 1 = 'no-license', -1 = nil.
 * LicenseFile#license per file (license_file.rb:92-98 over [Copyright, Exact, Dice]), from the
 * batch's resident Exact and match results (nothing is uploaded again):
 *   L(i) = flags & 1 ? T + 1 : (use_exact && exact[i] >= 0) ? exact[i] : best[i] >= 0 ? best[i] : T
 * Per project:
 *   license       Project#license (project.rb:24-32), -1 for nil: no file, or only copyright? files
 *   matched_file  the batch index of Project#matched_file (:40-42), or -1
 *   n_licenses    Project#licenses.count (:35-37): the distinct L(i), copyright? files included
 *   licenses      [n_projects][k_licenses]: the first k_licenses entries of Project#licenses -- file
 *                 order after prioritize_lgpl (:137-145), first occurrences -- padded with -1;
 *                 k_licenses in [0, DICE_PROJECT_K_MAX]
 * The order of files of equal name score is parity-unpinned in the reference (find_files sorts with
 * an unstable sort): license and matched_file do not depend on it, licenses lists what the caller's
 * order gives.
 * State: DICE_E_STATE unless dice_batch_match or dice_batch_match_confidence has run since the
 * batch's last upload, and, with use_exact != 0, unless dice_batch_exact has; the download calls are
 * DICE_E_STATE unless dice_batch_projects has run since the last upload. A NULL batch, NULL or
 * inconsistent offsets, NULL flags, k_licenses out of range and a negative n_projects are DICE_E_ARG.
 * dice_batch_projects is asynchronous on `stream` (no host synchronization inside unless its buffers
 * grow): offsets and flags are copied from host memory on that stream, so they must stay valid until
 * it has run. Its buffers are allocated on the first call and grown with n_projects.
 * dice_batch_download_projects synchronizes `stream`; any output may be NULL. */
#define DICE_PROJECT_K_MAX 8
int dice_batch_projects(dice_batch *batch, int64_t n_projects, const int64_t *offsets,
                        const uint8_t *file_flags, const uint8_t *template_flags,
                        int32_t use_exact, int32_t k_licenses, void *stream);
int dice_batch_download_projects(dice_batch *batch, int32_t *license, int32_t *matched_file,
                                 int32_t *n_licenses, int32_t *licenses, void *stream);
/* What a caller reports about Project#matched_file (project_file.rb:69-76), gathered by the resolve
 * so that only one entry per project is downloaded: matcher[p] = 0 Copyright, 1 Exact, 2 Dice, -1 no
 * matcher (the file's license is 'other') or no matched file; confidence[p] = 100 for Copyright and
 * Exact, Dice#confidence for Dice, else 0; digest [n_projects][20] = the matched file's content_hash
 * (zeros without one) when dice_batch_content_hash ran before the resolve, DICE_E_STATE for a
 * non-NULL digest otherwise. Same state rule and synchronization as dice_batch_download_projects;
 * NULL outputs are skipped. */
int dice_batch_download_project_match(dice_batch *batch, int32_t *matcher, double *confidence,
                                      uint8_t *digest, void *stream);

/* Build step (no device needed): generate + compile the corpus-specialized sparse program
 * with hiprtc for gfx950 and store it in the code-object cache; writes the cache path. */
int dice_precompile(const dice_templates *templates, char *path, int32_t path_cap);
/* Generated HIP source of the sparse program (introspection/tests). Returns its length,
 * writes at most cap-1 bytes + NUL when buf != NULL, or -1 on bad input. */
int64_t dice_program_source(const dice_templates *templates, char *buf, int64_t cap);
/* The same for the program over the compact tile (the default of dice_create for corpora of at
 * most 64 templates; the environment variable DICE_PROG_LAYOUT=bits, read at dice_create, keeps
 * the full-bitset tile of dice_program_source). Same contract; -1 also for more templates. */
int64_t dice_program_source_compact(const dice_templates *templates, char *buf, int64_t cap);
/* The compact tile's layout, a pure function of `templates`. Vocabulary words that belong to
 * exactly the same templates form a class; a large class is stored as byte counts of at most 255
 * words each, the other words of some template as bits in vocabulary order. dest[V] (may be
 * NULL): per word its bit position in the tile (>= 0), -1 for a word of no template (not in
 * the tile), or -2 - f for count byte f, which is tile byte *count_base + f. The tile is
 * bit dwords, then count bytes, zero-padded to whole 16-byte quads; resident tile slot i holds
 * quad qperm[i] of it (qperm may be NULL; qperm_cap entries available). Returns the tile's
 * quad count, or -1 on bad input or too small a qperm_cap. */
int32_t dice_program_layout(const dice_templates *templates, int32_t *dest, int32_t *count_base,
                            int32_t *qperm, int32_t qperm_cap);
/* The tables of the program's matrix-core accumulate stage (DICE_PROG_MATCH),
 * a pure function of `templates`. The stage scores the compact tile's bit region as a binary matrix
 * product in K-steps of 64 e2m1 elements (two lane halves of 32). dims[4] receives {K-steps,
 * 32-template tiles, bit dwords, 1 when dice_create would choose the stage for this corpus by its
 * cost rule, else 0}. frag (may be NULL) receives the template fragments
 * [K-step][template tile][lane 32 h + r][4] as dwords: lane (r, h) holds template 32 tile + r,
 * element e = 8 k + i of half h in nibble i of dword k. map (may be NULL) receives
 * [K-step][64] int32: for element e of half h (index 32 h + e) the bit of the file's resident
 * tile row it carries (32 * tile dword + bit, slot order), or -1 for none; the file side holds
 * such a bit in nibble i of dword k as e2m1 0.5, 1.0, 2.0, 2.0 for k = 0..3. Returns the dword
 * count of frag, 0 for a corpus the stage cannot take (no bit region, tables too large), or -1
 * on bad input or too small a capacity (frag_cap dwords, map_cap entries). */
int64_t dice_program_mfma_tables(const dice_templates *templates, int32_t *dims, uint32_t *frag, int64_t frag_cap,
                                 int32_t *map, int64_t map_cap);
/* How the device holds those tables, a pure function of `templates`. The kernel keeps the templates
 * in two blocks of 32 rows, chosen so that, with the bit region grouped as [words of block 0 only |
 * of both | of block 1 only] (dice_program_layout's dest follows that order), as few (K-step, block)
 * fragments as possible have a non-zero element; it reads and multiplies only those. rows[64] (may be
 * NULL) receives the template in device row 32 block + r, or -1 for a padded row; every template
 * appears once, and a corpus of at most 32 templates keeps row i = template i. live (may be NULL)
 * receives one byte per [K-step][block] (dims[0] * dims[1] of dice_program_mfma_tables): 1 iff the
 * fragment of the canonical table, its rows gathered through rows[], has a non-zero element. Returns
 * the number of live fragments, 0 for a corpus the stage cannot take, or -1 on bad input or too small
 * a live_cap (bytes). */
int32_t dice_program_mfma_rows(const dice_templates *templates, int32_t *rows, uint8_t *live, int64_t live_cap);

/* The sparse program's accumulate stage in this ctx: 0 VALU only, 1 matrix cores for batches that
 * give every CU a 64-file tile (smaller ones take the VALU kernels), 2 matrix cores at every size
 * (DICE_PROG_MATCH=mfma); -1 for a NULL ctx. */
int32_t dice_ctx_program_stage(const dice_ctx *ctx);

const char *dice_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LICENSEE_DICE_H */
