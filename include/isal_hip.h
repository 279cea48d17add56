/*
 * isal_hip.h — MI355X-native extensions of the erasure-code engine.
 *
 * The reference API (erasure_code.h) is one synchronous call per stripe. On a
 * GPU that shape is launch- and sync-bound, so the engine adds a batched,
 * stream-ordered "stripe batch": nstripes independent stripes that share one
 * coefficient matrix are encoded by ONE kernel launch over device-resident
 * shards. This is additive: nothing in erasure_code.h depends on it, and the
 * results of a batch are byte-identical to calling ec_encode_data /
 * ec_encode_data_update once per stripe.
 *
 * All functions return 0 on success and a negative ISAL_HIP_E* code on error
 * (they never abort). Streams are hipStream_t passed as void* so that this
 * header needs no HIP include; NULL means the legacy default stream.
 */
#ifndef ISAL_HIP_ISAL_HIP_H
#define ISAL_HIP_ISAL_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISAL_HIP_OK 0
#define ISAL_HIP_EINVAL (-1)   /* bad argument (size, count, NULL, unaligned pointer) */
#define ISAL_HIP_EHIP (-2)     /* a HIP runtime call failed */
#define ISAL_HIP_ENOMEM (-3)   /* host or device allocation failed */
#define ISAL_HIP_EDEVICE (-4)  /* a shard pointer is on another GPU than the object's device */
#define ISAL_HIP_ESINGULAR (-5) /* an erasure pattern's survivor matrix is not invertible */

typedef struct isal_hip_batch isal_hip_batch;

/*
 * Describe a batch of stripes. len bytes per shard, k sources, rows outputs.
 * gftbls: 32*k*rows bytes from ec_init_tables (host memory; copied).
 * data:   host array of nstripes*k DEVICE pointers, stripe-major
 *         (data[s*k + j] = shard j of stripe s).
 * coding: host array of nstripes*rows DEVICE pointers (coding[s*rows + l]).
 * Pointer tables and derived coefficient tables are uploaded once here; the
 * launch functions below only enqueue kernels.
 * The batch belongs to the caller's current device at creation: every shard
 * must be hipMalloc memory of that device, managed memory, or page-locked host
 * memory (ISAL_HIP_EDEVICE for memory of another GPU, ISAL_HIP_EINVAL for
 * pageable memory, which no kernel can reach). The batch's kernels run on its
 * device whatever the calling thread's current device is; a stream passed to
 * them must belong to that device (NULL: its legacy default stream).
 */
int isal_hip_batch_create(isal_hip_batch **out, int len, int k, int rows,
                          const unsigned char *gftbls, int nstripes, unsigned char *const *data,
                          unsigned char *const *coding);

/* Replace the coefficient tables (e.g. a decode matrix) of an existing batch.
 * Synchronises the device before the old tables go: launches already queued
 * on any stream keep the coefficients they were enqueued with.
 * All or nothing: everything derived from gftbls (coefficient tables, 0/1 row
 * and column masks, derived-checksum rows, LDS product tables) is built and
 * uploaded aside and published together; after a failure the batch still
 * computes the old matrix in every entry point. */
int isal_hip_batch_set_tables(isal_hip_batch *b, const unsigned char *gftbls);

/* Enqueue ec_encode_data for every stripe of the batch on stream. */
int isal_hip_batch_encode(isal_hip_batch *b, void *stream);

/* Enqueue ec_encode_data_update(vec_i) for every stripe: source shard
 * data[s*k + vec_i] is folded into coding[s*rows + l] for all l. */
int isal_hip_batch_update(isal_hip_batch *b, int vec_i, void *stream);

/* Enqueue a verify of every stripe (the xor_check / pq_check question for a
 * whole batch, e.g. a scrub): each stripe's coding rows are recomputed from
 * its sources and compared with the stored bytes; nothing is written to the
 * shards. bad: DEVICE array of nstripes words, bad[s] = ~0 when stripe s is
 * consistent, else its first mismatch as column << 8 | row: the smallest
 * mismatching column of any row, then the smallest row at that column,
 * whichever lane, workgroup or (rows > 8) pass found it. Every word of bad is
 * rewritten by each call with len > 0. Needs every shard 16-byte aligned (ISAL_HIP_EINVAL
 * otherwise, nothing enqueued). */
int isal_hip_batch_check(isal_hip_batch *b, unsigned long long *bad, void *stream);

int isal_hip_batch_destroy(isal_hip_batch *b);

/*
 * Fragment checksums (the step storage callers run right after
 * encoding). crc receives nstripes*(k+rows) values in DEVICE memory:
 *   crc[s*(k+rows) + j]     = crc32_iscsi(data[s*k + j],   len, init)  (j < k)
 *   crc[s*(k+rows) + k + l] = crc32_iscsi(coding[s*rows + l], len, init)
 * with the reference's crc32_iscsi semantics (include/crc.h:137-141,
 * crc/crc_base.c:205-219: reflected CRC32C, register starts at init, no final
 * inversion).
 *
 * isal_hip_batch_encode_crc: ec_encode_data for every stripe AND the checksums
 *   of the sources and the fresh parity, in one pass over HBM when the shards
 *   are 16-byte aligned, len % 16 == 0 and k <= 64 (otherwise encode, then a
 *   checksum pass).
 * isal_hip_batch_crc: checksums only (e.g. to verify fragments read back).
 * The first call allocates the per-lane partials: nstripes*(k+rows) *
 * ceil(len/65536) KiB of device memory (~1/64 of the shard bytes).
 */
int isal_hip_batch_encode_crc(isal_hip_batch *b, unsigned int init, unsigned int *crc,
                              void *stream);
int isal_hip_batch_crc(isal_hip_batch *b, unsigned int init, unsigned int *crc, void *stream);

/*
 * CRC64 of every shard: crc[s*(k+rows) + j] as isal_hip_batch_crc, in DEVICE
 * memory, = crc64_<variant>(init, shard, len) with the reference's semantics
 * (include/crc64.h:54-163, crc/crc64_base.c:569-670: register starts at ~init,
 * inverted on return; refl / norm bit order). Variants in the order of
 * crc64.h. The first call per variant uploads its own tables (~80 KiB, kept
 * for the batch's lifetime; no device synchronisation); partials take
 * nstripes*(k+rows) * ceil(len/65536) * 2 KiB of device memory.
 */
#define ISAL_HIP_CRC64_ECMA_REFL 0
#define ISAL_HIP_CRC64_ECMA_NORM 1
#define ISAL_HIP_CRC64_ISO_REFL 2
#define ISAL_HIP_CRC64_ISO_NORM 3
#define ISAL_HIP_CRC64_JONES_REFL 4
#define ISAL_HIP_CRC64_JONES_NORM 5
#define ISAL_HIP_CRC64_ROCKSOFT_REFL 6
#define ISAL_HIP_CRC64_ROCKSOFT_NORM 7
#define ISAL_HIP_CRC64_NVARIANTS 8
int isal_hip_batch_crc64(isal_hip_batch *b, int variant, unsigned long long init,
                         unsigned long long *crc, void *stream);
/* ec_encode_data for every stripe AND crc64_<variant> of the sources and the
 * fresh parity (layout as isal_hip_batch_crc64), in one pass over HBM when the
 * shards are 16-byte aligned, len % 16 == 0, len >= 4096, rows <= 8 and
 * k <= 32 (otherwise encode, then isal_hip_batch_crc64). */
int isal_hip_batch_encode_crc64(isal_hip_batch *b, int variant, unsigned long long init,
                                unsigned long long *crc, void *stream);

/* ---- repair batch: mixed erasure patterns in one launch ------------------ */

/*
 * The recovery rows for one erasure pattern: pure host arithmetic, no GPU.
 * a: the m*k encode matrix (gf_gen_rs_matrix / gf_gen_cauchy1_matrix layout,
 *    identity on top), m <= 256.
 * errs: nerrs distinct shard indices in [0, m), any order, 1 <= nerrs <= m - k.
 * survivors[k]: the first k non-erased indices, ascending.
 * c[nerrs*k]: row i rebuilds shard errs[i] from those survivors: the
 *    survivors' rows of a are inverted; a data shard takes its row of the
 *    inverse, a parity shard its encode row times the inverse.
 * ISAL_HIP_ESINGULAR when the survivors' rows are not invertible,
 * ISAL_HIP_EINVAL for arguments outside the contract.
 */
int isal_hip_decode_matrix(int k, int m, const unsigned char *a, int nerrs,
                           const unsigned char *errs, unsigned char *c, unsigned char *survivors);

/*
 * A rebuild after device loss: placement rotates shards over devices, so the
 * lost device is another shard index in every stripe. A repair batch covers
 * nstripes stripes of one geometry (len bytes per shard, k of m shards
 * suffice), each with its OWN set of nerrs erased shards, and rebuilds all
 * of them with one kernel launch per pass of isal_hip_max_rows_per_pass()
 * rows, on the caller's stream.
 *   shards: host array of nstripes*m DEVICE pointers, shards[s*m + i] = shard
 *           i of stripe s. A stripe's erased entries are its destinations;
 *           its first k others (ascending) are read, nothing else is touched.
 *   errs:   nstripes*nerrs shard indices, errs[s*nerrs + i] for stripe s
 *           (in range, distinct within the stripe, any order).
 * Every entry of shards must be non-NULL and 16-byte aligned
 * (ISAL_HIP_EINVAL); memory kinds and device ownership as for
 * isal_hip_batch_create. Any len >= 0 is valid. A stripe whose pattern is not
 * decodable fails the whole create with ISAL_HIP_ESINGULAR and nothing is
 * launched; *bad_stripe (optional) then names the first such stripe, as it
 * does the first stripe with a bad index or pointer on ISAL_HIP_EINVAL (-1
 * otherwise). All of these checks run before the first HIP call, so they
 * answer the same on a host without a GPU.
 * create derives the recovery rows of every distinct pattern and uploads
 * pointer and coefficient tables once; isal_hip_repair_run only enqueues
 * kernels, may be called repeatedly and is idempotent. The coefficient
 * tables take 20*k*nerrs bytes per distinct pattern; more than
 * ISAL_HIP_REPAIR_MAX_TABLE_BYTES of them (over 100000 patterns of a k = 10,
 * nerrs = 3 layout; far past the few MiB of L2 that let neighbouring
 * workgroups share a pattern's tables) is refused with ISAL_HIP_ENOMEM.
 * Out of scope: erasure counts that differ within one object (one object per
 * count; isal_hip_repair_create_ragged below lifts this and the single len),
 * unaligned or host-pageable shards, and any CPU route.
 */
#define ISAL_HIP_REPAIR_MAX_TABLE_BYTES (64u << 20)
typedef struct isal_hip_repair isal_hip_repair;
int isal_hip_repair_create(isal_hip_repair **out, int len, int k, int m, const unsigned char *a,
                           int nerrs, int nstripes, const unsigned char *errs,
                           unsigned char *const *shards, int *bad_stripe);
int isal_hip_repair_run(isal_hip_repair *r, void *stream);
/* distinct erasure patterns found by create */
int isal_hip_repair_npatterns(const isal_hip_repair *r);
int isal_hip_repair_destroy(isal_hip_repair *r);

/*
 * Ragged repair: the same object for a real rebuild window, where every
 * stripe has its OWN shard length (objects of every size, short last stripes)
 * and its OWN erasure count (after a second device loss stripes have lost 0,
 * 1 or 2 shards). isal_hip_repair_run, _npatterns and _destroy serve both
 * kinds of object.
 *   lens:     nstripes byte lengths; lens[s] is the length of every shard of
 *             stripe s. Any value >= 0 is valid.
 *   max_errs: the stride of errs, 1 <= max_errs <= m - k.
 *   nerrs:    nstripes counts, nerrs[s] in [0, max_errs].
 *   errs:     errs[s*max_errs + i] for i < nerrs[s] are stripe s's erased
 *             indices (in range, distinct, any order); the rest of the row is
 *             ignored.
 *   shards:   as for isal_hip_repair_create.
 * A stripe with lens[s] == 0 or nerrs[s] == 0 is neither read nor written.
 * Every other stripe is rebuilt byte-identically to ec_encode_data(lens[s], k,
 * nerrs[s], the tables of isal_hip_decode_matrix(...), survivors, erased);
 * nothing outside [0, lens[s]) of the erased shards is written.
 * Refused, all before the first HIP call, so a host without a GPU answers the
 * same; *bad_stripe (optional) as for the other batches:
 *   ISAL_HIP_EINVAL     NULL arguments, nstripes <= 0, k < 1, m <= k, m > 256
 *                       or max_errs out of range (*bad_stripe = -1);
 *   ISAL_HIP_EINVAL     nerrs[s] > max_errs, a negative lens[s], a bad or
 *                       duplicate index, a NULL shard pointer or one not
 *                       16-byte aligned (stripes of zero length or zero count
 *                       included); *bad_stripe names the first such stripe;
 *   ISAL_HIP_ESINGULAR  *bad_stripe names the first undecodable stripe;
 *   ISAL_HIP_ENOMEM     the coefficient tables of all distinct patterns of
 *                       all counts together exceed
 *                       ISAL_HIP_REPAIR_MAX_TABLE_BYTES;
 *   ISAL_HIP_EINVAL     one count class (below) has more than 2^30 work items
 *                       at the smallest tile its passes use, the limit of one
 *                       launch (*bad_stripe = -1).
 * isal_hip_repair_npatterns counts distinct erasure sets; sets of different
 * counts are different patterns, and stripes that lost nothing contribute
 * none. Memory kinds and device ownership as for isal_hip_batch_create; a
 * shard must be reachable over its own stripe's length.
 * isal_hip_repair_run only enqueues. The stripes are grouped into count
 * classes: class c holds the stripes with nerrs[s] == c and lens[s] > 0. Each
 * class present is launched once per pass of isal_hip_max_rows_per_pass()
 * rows, in ascending c: a run takes the sum over those classes of
 * ceil(c / max_rows_per_pass) launches (counted by isal_hip_kernel_launches),
 * none when no class is present, and is idempotent. Work items are 4 KiB
 * tiles of one row; a pass of 1-2 rows runs on 2 KiB tiles, as in the ragged
 * batch.
 * Device memory: the coefficient tables (20*k*c bytes per distinct pattern of
 * count c) and one more allocation that holds, per class, the pointer table
 * (8*(k + c) bytes per row), 4 bytes of pattern word and 4 bytes of length
 * per row, and 8 bytes per tile of one shard for each tile size the class's
 * passes use (0.2 % of one shard's bytes at 4 KiB; c % 8 == 1 or 2 adds or
 * takes instead a table per 2 KiB tile).
 * Out of scope: unaligned or host-pageable shards, any CPU route, set_tables,
 * and the LDS-staged and LDS product-table wide kernels (every pass takes the
 * plain lookup kernel).
 */
int isal_hip_repair_create_ragged(isal_hip_repair **out, int k, int m, const unsigned char *a,
                                  int nstripes, const int *lens, int max_errs,
                                  const unsigned char *nerrs, const unsigned char *errs,
                                  unsigned char *const *shards, int *bad_stripe);

/* ---- overwrite batch: partial-stripe writes folded into parity ----------- */

/*
 * A read-modify-write of stripes that are already encoded: a client rewrites
 * nw of a stripe's k data shards and the parity must become
 *   coding[l] ^= C[l][j] * (old_j ^ new_j)   for every rewritten shard j, row l.
 * An overwrite batch covers nstripes stripes of one geometry, each with its
 * OWN set of nw rewritten shard indices, with one kernel launch per pass of
 * isal_hip_max_rows_per_pass() rows, on the caller's stream; each parity row
 * is read once and written once whatever nw is.
 *   gftbls:   32*k*rows bytes from ec_init_tables for the encode matrix (host
 *             memory; copied), as for isal_hip_batch_create.
 *   idx:      nstripes*nw data-shard indices, idx[s*nw + i] in [0, k) for slot
 *             i of stripe s (distinct within the stripe, any order);
 *             1 <= nw <= k <= 256.
 *   old_data: host array of nstripes*nw DEVICE pointers, old_data[s*nw + i] =
 *             the bytes the parity currently reflects for that shard.
 *   new_data: host array of nstripes*nw DEVICE pointers to the replacements.
 *   coding:   host array of nstripes*rows DEVICE pointers (coding[s*rows + l]).
 * len is the number of bytes rewritten. A sub-shard byte range is expressed
 * by the caller: offset all of a stripe's pointers by the same amount and
 * pass the range's length as len.
 * Every pointer must be non-NULL and 16-byte aligned, and within one stripe no
 * two of its 2*nw + rows byte ranges may overlap (ISAL_HIP_EINVAL); memory
 * kinds and device ownership as for isal_hip_batch_create. Any len >= 0 is
 * valid. *bad_stripe (optional) names the first stripe with a bad index,
 * pointer or overlap on ISAL_HIP_EINVAL (-1 otherwise). All of these checks
 * run before the first HIP call, so they answer the same on a host without a
 * GPU. create uploads the pointer, index and coefficient tables once;
 * isal_hip_overwrite_run only enqueues kernels. The object belongs to the
 * caller's current device at creation and runs there.
 *   flags = 0: only the parity changes. The delta is its own inverse, so
 *     running twice restores the parity exactly.
 *   flags = ISAL_HIP_OVERWRITE_COMMIT: the same pass also stores new over old
 *     (in the last pass when rows exceed one pass), so that afterwards the old
 *     location holds the current bytes; a second committed run finds a zero
 *     delta and changes no byte.
 *   Any other flag bit: ISAL_HIP_EINVAL, nothing enqueued.
 * Out of scope: write counts that differ within one object (one object per
 * count; isal_hip_overwrite_create_ragged below lifts this and the single
 * len), unaligned or host-pageable shards, any CPU route, and overwrites of
 * parity shards.
 */
#define ISAL_HIP_OVERWRITE_COMMIT 1
typedef struct isal_hip_overwrite isal_hip_overwrite;
int isal_hip_overwrite_create(isal_hip_overwrite **out, int len, int k, int rows,
                              const unsigned char *gftbls, int nw, int nstripes,
                              const unsigned char *idx, unsigned char *const *old_data,
                              unsigned char *const *new_data, unsigned char *const *coding,
                              int *bad_stripe);
int isal_hip_overwrite_run(isal_hip_overwrite *o, int flags, void *stream);
int isal_hip_overwrite_destroy(isal_hip_overwrite *o);

/*
 * Ragged overwrite: the same object for a window of client writes, where
 * every stripe has its OWN byte count and its OWN number of rewritten shards
 * (one for a small write, several for a write that straddles shards, k for a
 * full-stripe rewrite). isal_hip_overwrite_run (flags exactly as above) and
 * isal_hip_overwrite_destroy serve both kinds of object.
 *   lens:     nstripes byte counts; lens[s] >= 0 is the number of bytes
 *             rewritten in stripe s. A sub-shard range is expressed by pointer
 *             offsets, as above.
 *   max_nw:   the stride of idx, old_data and new_data,
 *             1 <= max_nw <= k <= 256.
 *   nw:       nstripes counts, nw[s] in [0, max_nw] (ints: nw = k = 256 does
 *             not fit a byte).
 *   idx, old_data, new_data: entries [s*max_nw + i] for i < nw[s] are the slots
 *             of stripe s: indices in [0, k), distinct within the stripe, in
 *             any order. The rest of each row is ignored entirely: it may
 *             hold any index and NULL or unaligned pointers.
 *   gftbls, coding (coding[s*rows + l]): as for isal_hip_overwrite_create.
 * A stripe with lens[s] == 0 or nw[s] == 0 is neither read nor written. Every
 * other stripe ends byte-identical to what isal_hip_overwrite_create(lens[s],
 * ..., nw[s], 1, ...) followed by a run with the same flags leaves for that
 * stripe alone. Nothing outside [0, lens[s]) of any buffer is written; the
 * new buffers, the data shards that are not rewritten and, without
 * ISAL_HIP_OVERWRITE_COMMIT, the old shards are never written.
 * Refused, all before the first HIP call and in this order, so a host without
 * a GPU answers the same; *bad_stripe (optional) as for the other batches:
 *   ISAL_HIP_EINVAL  NULL arguments, nstripes <= 0, k < 1, k > 256, rows < 1
 *                    or max_nw out of range (*bad_stripe = -1);
 *   ISAL_HIP_EINVAL  a negative lens[s] or nw[s], nw[s] > max_nw, or a bad or
 *                    duplicate index among the first nw[s];
 *   ISAL_HIP_EINVAL  a NULL pointer or one not 16-byte aligned among the
 *                    stripe's 2*nw[s] + rows live pointers (stripes of zero
 *                    length or zero count included);
 *   ISAL_HIP_EINVAL  two of those ranges overlapping over the stripe's own
 *                    lens[s] (ranges that touch pass, and so do equal
 *                    pointers at lens[s] == 0); for these three *bad_stripe
 *                    names the first stripe that fails any of them;
 *   ISAL_HIP_EINVAL  more than 2^30 work items at the 2 KiB tile, the only
 *                    tile size of this object and the limit of one launch
 *                    (*bad_stripe = -1).
 * Memory kinds and device ownership as for isal_hip_batch_create; a shard must
 * be reachable over its own stripe's length.
 * isal_hip_overwrite_run on such an object only enqueues: ONE kernel launch
 * per pass of isal_hip_max_rows_per_pass() rows (counted by
 * isal_hip_kernel_launches), whatever the mix of lengths and counts, and none
 * when no stripe has both lens[s] > 0 and nw[s] > 0. Work items are 2 KiB
 * tiles of one stripe. ISAL_HIP_OVERWRITE_COMMIT stores new over old in the
 * last pass only; per stripe, two runs without it restore the parity and a
 * second committed run changes no byte.
 * Device memory: the pointer table (8*(2*max_nw + rows) bytes per stripe) and
 * the index table (4*max_nw bytes per stripe) at stride max_nw, the
 * coefficient tables, 4 bytes of length and 4 of count per stripe, and 8
 * bytes per 2 KiB tile of one rewritten range (0.4 % of its bytes).
 * Out of scope: overwrites of parity shards, unaligned or host-pageable
 * shards, any CPU route, set_tables, and a fused checksum of the rewritten
 * shards.
 */
int isal_hip_overwrite_create_ragged(isal_hip_overwrite **out, int k, int rows,
                                     const unsigned char *gftbls, int nstripes, const int *lens,
                                     int max_nw, const int *nw, const unsigned char *idx,
                                     unsigned char *const *old_data,
                                     unsigned char *const *new_data,
                                     unsigned char *const *coding, int *bad_stripe);

/* ---- scrub batch: the corrupt shard of each bad stripe in one pass -------- */

/*
 * isal_hip_batch_check says that a stripe is inconsistent; a scrub batch also
 * says which shard to rebuild, from the parity the check recomputes anyway.
 * Shard index i < k is data shard i, index k + l is parity row l. C[l][j] is
 * the coefficient of row l and source j: byte 1 of the 32-byte entry
 * gftbls + 32*(l*k + j) (the ec_init_tables format).
 *
 * Per byte column, let e[l] = stored parity row l ^ the parity row l
 * recomputed from the stored sources (the column's syndrome). If every e[l]
 * is zero the column is consistent. Otherwise the column NAMES
 *   - data shard j < k, when some d != 0 gives e[l] == C[l][j]*d for every l;
 *   - parity row l (index k + l), when e is non-zero in row l only;
 *   - nothing, when neither holds.
 * Per stripe, after isal_hip_scrub_run, verdict[s] is
 *   - ISAL_HIP_SCRUB_CLEAN when no byte column mismatches;
 *   - shard index i when every mismatching column names the same i;
 *   - ISAL_HIP_SCRUB_MULTI when two columns name different shards or some
 *     column names nothing;
 * whichever lane or workgroup found what first.
 *
 * What a verdict is worth: an index is THE ONLY SINGLE-SHARD EXPLANATION of
 * the stripe's mismatches, not a proof that this shard is the corrupt one.
 * Two corrupt shards in one byte column can imitate a third: with rows = 2
 * about (k + 2)/257 of random two-shard syndromes do. Only the agreement of
 * all of a stripe's mismatching columns makes that rare (a single corrupt
 * byte column carries no such agreement). Callers who keep fragment checksums
 * (isal_hip_batch_crc) should confirm the verdict with them before they
 * rebuild the named shard through isal_hip_repair_create(nerrs = 1).
 */
#define ISAL_HIP_SCRUB_CLEAN 0xffffffffu /* every byte column consistent */
#define ISAL_HIP_SCRUB_MULTI 0xfffffffeu /* inconsistent, and no single shard explains it */

/*
 * Pure host arithmetic, no GPU; k >= 1, rows >= 1, k + rows <= 256.
 * isal_hip_scrub_ambiguity: 0 when the k + rows columns of [C | I_rows] are
 *   all non-zero and no two are proportional, so that at most one shard can
 *   explain any syndrome. Otherwise ISAL_HIP_ESINGULAR, and pair (optional)
 *   holds the first offending pair in lexicographic order; a zero column j is
 *   reported as {j, j}. ISAL_HIP_EINVAL for arguments outside the contract
 *   (pair is {-1, -1} whenever the answer is not ISAL_HIP_ESINGULAR).
 * isal_hip_locate_syndrome: the per-column rule above for one syndrome of
 *   rows bytes: the shard index it names (for a matrix that
 *   isal_hip_scrub_ambiguity refuses: the lowest data shard that explains it,
 *   before any parity row), (int) ISAL_HIP_SCRUB_MULTI when it names nothing,
 *   (int) ISAL_HIP_SCRUB_CLEAN when it is all zero. Both constants are
 *   negative as int, so no error code can be told from them: arguments
 *   outside the contract answer (int) ISAL_HIP_SCRUB_MULTI, no shard.
 */
int isal_hip_scrub_ambiguity(int k, int rows, const unsigned char *gftbls, int pair[2]);
int isal_hip_locate_syndrome(int k, int rows, const unsigned char *gftbls,
                             const unsigned char *syndrome);

/*
 * A scrub batch covers nstripes stripes of one geometry; len, k, rows,
 * gftbls, data and coding as for isal_hip_batch_create, *bad_stripe
 * (optional) as for the repair and overwrite batches. Refused, all before the
 * first HIP call, so a host without a GPU answers the same:
 *   ISAL_HIP_EINVAL    NULL arguments, len < 0, nstripes <= 0, k < 1,
 *                      k + rows > 256, or rows < 2 (one row cannot tell
 *                      shards apart);
 *   ISAL_HIP_EINVAL    rows > isal_hip_max_rows_per_pass(): a syndrome must be
 *                      whole inside one workgroup; wider codes are out of
 *                      scope;
 *   ISAL_HIP_EINVAL    a NULL shard pointer or one not 16-byte aligned;
 *                      *bad_stripe names the first such stripe (-1 otherwise);
 *   ISAL_HIP_ESINGULAR a matrix that isal_hip_scrub_ambiguity refuses.
 * Memory kinds and device ownership as for isal_hip_batch_create. The object
 * belongs to the caller's current device at creation and runs there. Pointer,
 * coefficient and location tables are uploaded once in create;
 * isal_hip_scrub_run only enqueues on the caller's stream: a fill of verdict
 * (a DEVICE array of nstripes words) with ISAL_HIP_SCRUB_CLEAN, then one
 * kernel launch (one per slice of stripes for very large batches, counted by
 * isal_hip_kernel_launches). Every word of verdict is rewritten by each call
 * with len > 0; with len == 0 the call returns 0 and enqueues nothing.
 * Nothing is written to the shards. Consistent data costs what
 * isal_hip_batch_check costs: the location arithmetic runs only in lanes that
 * hold a mismatching byte.
 * Out of scope: more than isal_hip_max_rows_per_pass() rows, locating two or
 * more corrupt shards, correcting in the same pass (rebuild through the
 * repair batch), unaligned or host-pageable shards, and any CPU route beyond
 * the two host functions above.
 */
typedef struct isal_hip_scrub isal_hip_scrub;
int isal_hip_scrub_create(isal_hip_scrub **out, int len, int k, int rows,
                          const unsigned char *gftbls, int nstripes,
                          unsigned char *const *data, unsigned char *const *coding,
                          int *bad_stripe);
int isal_hip_scrub_run(isal_hip_scrub *s, unsigned int *verdict, void *stream);
int isal_hip_scrub_destroy(isal_hip_scrub *s);

/*
 * Ragged scrub: the same object for a real rebuild window, where every stripe
 * has its OWN shard length (the ragged batch below and
 * isal_hip_repair_create_ragged above are its neighbours: the ragged check
 * finds the bad stripes, this names their shards, the ragged repair rebuilds
 * them). isal_hip_scrub_run and isal_hip_scrub_destroy serve both kinds of
 * object.
 *   lens:   nstripes byte lengths; lens[s] is the length of every shard of
 *           stripe s. Any value >= 0 is valid. A stripe of length 0 is neither
 *           read nor written; its verdict is ISAL_HIP_SCRUB_CLEAN.
 *   k, rows, gftbls, data, coding: as for isal_hip_scrub_create.
 * For every other stripe the verdict is exactly what
 * isal_hip_scrub_create(len = lens[s], ...) gives for that stripe alone, the
 * two-shard imitation limit above included.
 * Refused, all before the first HIP call and in this order, so a host without
 * a GPU answers the same; *bad_stripe (optional) as for the other batches:
 *   ISAL_HIP_EINVAL    NULL arguments, nstripes <= 0, k < 1, rows < 2,
 *                      rows > isal_hip_max_rows_per_pass() or k + rows > 256
 *                      (*bad_stripe = -1);
 *   ISAL_HIP_EINVAL    a negative lens[s], a NULL shard pointer or one not
 *                      16-byte aligned (those of zero-length stripes
 *                      included); *bad_stripe names the first such stripe;
 *   ISAL_HIP_EINVAL    more than 2^30 work items at the 4 KiB tile, the only
 *                      tile size of this object and the limit of one launch
 *                      (*bad_stripe = -1);
 *   ISAL_HIP_ESINGULAR a matrix that isal_hip_scrub_ambiguity refuses.
 * Memory kinds and device ownership as for isal_hip_batch_create; a shard must
 * be reachable over its own stripe's length. isal_hip_scrub_run on such an
 * object only enqueues: the fill of verdict, then ONE kernel launch
 * (isal_hip_kernel_launches grows by 1) over 4 KiB tiles of one stripe. Every
 * word of verdict is rewritten by each call, unless every length is 0: then
 * the call returns 0, enqueues nothing and leaves verdict untouched. Nothing
 * is written to the shards.
 * Device memory besides what the uniform scrub uses: 4 bytes per stripe, and
 * 8 bytes per 4 KiB tile of one shard.
 * Out of scope: more than one pass of rows, the 0/1 XOR form (the plain
 * lookup kernel, as every ragged launch), correcting in the same pass,
 * unaligned or host-pageable shards, and any CPU route.
 */
int isal_hip_scrub_create_ragged(isal_hip_scrub **out, int k, int rows, const unsigned char *gftbls,
                                 int nstripes, const int *lens, unsigned char *const *data,
                                 unsigned char *const *coding, int *bad_stripe);

/* ---- ragged batch: stripes of different lengths in one launch ------------- */

/*
 * Every object above takes one len for all of its stripes. An object store
 * encodes objects of every size, and the last stripe of every object is
 * short: a ragged batch covers nstripes stripes of one geometry (k sources,
 * rows outputs, one matrix), each with its OWN shard length, and encodes or
 * checks all of them with one kernel launch per pass of
 * isal_hip_max_rows_per_pass() rows, or checksums every shard with two, on the
 * caller's stream.
 *   gftbls, data (nstripes*k DEVICE pointers), coding (nstripes*rows): as for
 *           isal_hip_batch_create. gftbls is any ec_init_tables output, so a
 *           uniform-pattern decode of ragged stripes is this object built
 *           with the decode matrix (isal_hip_decode_matrix), data = the
 *           survivors and coding = the shards to rebuild.
 *   lens:   nstripes byte lengths; lens[s] is the length of every shard of
 *           stripe s. Any value >= 0 is valid; a stripe of length 0 is
 *           neither read nor written.
 * Refused, all before the first HIP call, so a host without a GPU answers the
 * same; *bad_stripe (optional) as for the repair, overwrite and scrub batches:
 *   ISAL_HIP_EINVAL  NULL arguments, nstripes <= 0, k < 1, rows < 1 or
 *                    k + rows > 256 (*bad_stripe = -1);
 *   ISAL_HIP_EINVAL  a negative lens[s], a NULL shard pointer or one not
 *                    16-byte aligned (those of zero-length stripes included);
 *                    *bad_stripe names the first such stripe;
 *   ISAL_HIP_EINVAL  more than 2^30 work items at the smallest tile (2 KiB),
 *                    the limit of one launch: such a batch cannot exist in one
 *                    GPU's memory, so it is refused, not sliced
 *                    (*bad_stripe = -1).
 * Memory kinds and device ownership as for isal_hip_batch_create. The object
 * belongs to the caller's current device at creation and runs there.
 * create uploads the pointer table, the coefficient tables, the lengths and
 * the work-item tables once. Device memory besides the pointer and
 * coefficient tables every batch has: 4 bytes per stripe, and 8 bytes per
 * 4 KiB tile of one shard (0.2 % of one shard's bytes; a k-source stripe reads
 * k times that); an object with rows % 8 == 1 or 2 runs a pass on 2 KiB tiles
 * and keeps a second table of 8 bytes per 2 KiB tile.
 *
 * isal_hip_ragged_items: pure arithmetic, no GPU. The work items of a ragged
 *   launch: the tiles of stripe 0, then of stripe 1, ...; stripe s has
 *   ceil(lens[s] / tile) of them, a stripe of length 0 has none. Returns the
 *   item count, or -1 for arguments outside the contract (NULL lens,
 *   nstripes <= 0, a negative length, tile <= 0). items (optional): 2 words
 *   per item, {stripe, tile index}.
 * isal_hip_ragged_encode: only enqueues; one kernel launch per pass (counted
 *   by isal_hip_kernel_launches). Stripe s's parity is byte-identical to
 *   ec_encode_data(lens[s], ...). With every length 0 it returns 0 and
 *   enqueues nothing.
 * isal_hip_ragged_check: the isal_hip_batch_check contract per stripe. bad:
 *   DEVICE array of nstripes words; bad[s] = ~0 when stripe s is consistent
 *   or has length 0, else its first mismatch as column << 8 | row: the
 *   smallest column, then the smallest row at that column, whichever lane,
 *   workgroup or pass found it. Every word of bad is rewritten by each call,
 *   unless every length is 0 (then nothing is enqueued). Nothing is written
 *   to the shards.
 * isal_hip_ragged_crc: the isal_hip_batch_crc contract per stripe (SURVEY
 *   §8(f): the step storage callers run right after encoding, and the
 *   confirmation the scrub contract asks for before a named shard is rebuilt).
 *   crc: DEVICE array of nstripes*(k+rows) words,
 *     crc[s*(k+rows) + j]     = crc32_iscsi(data[s*k + j],      lens[s], init)
 *     crc[s*(k+rows) + k + l] = crc32_iscsi(coding[s*rows + l], lens[s], init)
 *   (the register starts at init, no final inversion). A stripe of length 0
 *   is not read and its k+rows words are init, which is what crc32_iscsi
 *   returns for len == 0. Every word of crc is rewritten by each call, unless
 *   every length is 0: then the call returns 0, enqueues nothing and leaves
 *   crc untouched, as the check does. Only enqueues, on the caller's stream
 *   and the object's device: 2 kernel launches (counted by
 *   isal_hip_kernel_launches), one pass over all shards of all stripes and
 *   one combine. Idempotent; nothing is written to the shards and nothing is
 *   read at or past lens[s] of any shard. NULL r or NULL crc: ISAL_HIP_EINVAL,
 *   nothing enqueued, no HIP call.
 *   Blocks: a workgroup of the pass covers tt consecutive 4 KiB tiles of one
 *   shard; tt is one value per object, chosen at its first checksum call:
 *   ISAL_HIP_CRC_TILES when set (at most 1024), else 64 (256 KiB of a shard,
 *   the uniform batch's choice), halved while one shard of every stripe
 *   together has fewer than 2048 blocks. A pass of more than 2^30 work items
 *   (blocks of one shard of every stripe, times k+rows) is refused with
 *   ISAL_HIP_EINVAL before anything is allocated or enqueued, not sliced:
 *   at the default tt that is 256 TiB of shards. create refuses nothing more
 *   than before.
 *   Memory: the first checksum call allocates, and destroy frees, a table of
 *   constants that depends on tt alone, not on any length (45 KiB + 4*tt
 *   bytes, whatever the number of distinct lengths), 8 bytes per block of one
 *   shard and 4 per stripe, and the per-lane partials: 1 KiB per block of
 *   every shard plus 1 KiB per shard (at tt = 64, 1/256 of the shard bytes
 *   plus 1 KiB per shard). A failed allocation returns ISAL_HIP_ENOMEM or
 *   ISAL_HIP_EHIP, leaves no HIP error behind and the object as usable for
 *   encode and check as before.
 * isal_hip_ragged_encode_crc: isal_hip_ragged_encode, then
 *   isal_hip_ragged_crc of the sources and the fresh parity, on the same
 *   stream; any rows, the two-pass case rows > isal_hip_max_rows_per_pass()
 *   included. NOT fused: its launches are the encode's (one per pass) plus
 *   the checksum's 2. It exists so that callers write the same sequence as
 *   with the uniform batch and a one-pass kernel can later slot in behind it.
 *   The checksum's memory is allocated first: a refusal leaves the parity
 *   untouched.
 * isal_hip_ragged_crc64: isal_hip_ragged_crc for the eight crc64_* flavours,
 *   with isal_hip_batch_crc64's semantics per stripe (the Rocksoft reflected
 *   flavour is the NVMe / S3 CRC64NVME checksum). variant is an
 *   ISAL_HIP_CRC64_* value; crc: DEVICE array of nstripes*(k+rows) 64-bit
 *   words,
 *     crc[s*(k+rows) + j]     = crc64_<variant>(init, data[s*k + j],      lens[s])
 *     crc[s*(k+rows) + k + l] = crc64_<variant>(init, coding[s*rows + l], lens[s])
 *   (the register starts at ~init and is inverted on return). A stripe of
 *   length 0 is not read and its k+rows words are init, which is what
 *   crc64_* returns for len == 0. Every word of crc is rewritten by each call,
 *   unless every length is 0: then the call returns 0, enqueues nothing and
 *   leaves crc untouched. Only enqueues, on the caller's stream and the
 *   object's device, whatever the calling thread's current device: 2 kernel
 *   launches (counted by isal_hip_kernel_launches), one pass and one combine.
 *   Idempotent; nothing is written to the shards and nothing is read at or
 *   past lens[s] of any shard. NULL r, NULL crc or a variant outside
 *   [0, ISAL_HIP_CRC64_NVARIANTS): ISAL_HIP_EINVAL, nothing enqueued, no HIP
 *   call.
 *   Blocks: tt as for isal_hip_ragged_crc, but CRC64's own value, chosen at
 *   the object's first CRC64 call: ISAL_HIP_CRC_TILES when set (at most 1024),
 *   else 128 (the uniform checksum-only CRC64's choice), halved while one
 *   shard of every stripe together has fewer than 2048 blocks. A pass of more
 *   than 2^30 work items (blocks of one shard of every stripe, times k+rows)
 *   is refused with ISAL_HIP_EINVAL before anything is allocated or enqueued.
 *   Memory, all of it CRC64's own and independent of what isal_hip_ragged_crc
 *   keeps, freed by destroy: the first CRC64 call allocates 8 bytes per block
 *   of one shard and 4 per stripe, and the per-lane partials, 2 KiB per block
 *   of every shard (at tt = 128, 1/256 of the shard bytes), shared by all
 *   variants; the first call with a given variant builds and uploads that
 *   variant's table of constants, which depends on the variant and tt alone,
 *   not on any length: 8*(11104 + tt + 1) bytes (87.8 KiB at tt = 128,
 *   whatever the number of distinct lengths; the uniform batch uploads about
 *   80 KiB per variant for ONE length). A failed allocation returns
 *   ISAL_HIP_ENOMEM or ISAL_HIP_EHIP, leaves no HIP error behind and the
 *   object as usable for encode, check and isal_hip_ragged_crc as before.
 * isal_hip_ragged_encode_crc64: isal_hip_ragged_encode, then
 *   isal_hip_ragged_crc64, on the same stream, for any rows. Not a fused
 *   pass either: its launches are the encode's (one per pass) plus 2. The
 *   checksum's memory and the variant's table are set up first: a refusal
 *   leaves the parity untouched.
 * Out of scope: update, a one-pass fused encode + checksum, CRC64 fused into
 * the encode, the 0/1 XOR form and the LDS-staged and LDS product-table wide
 * kernels of the uniform batch (every pass takes the plain lookup kernel),
 * unaligned or host-pageable shards, any CPU route, and set_tables (one
 * object per matrix). Naming the corrupt shard of a stripe the check reports is
 * isal_hip_scrub_create_ragged above, over the same lens, data and coding.
 */
typedef struct isal_hip_ragged isal_hip_ragged;
long long isal_hip_ragged_items(int nstripes, const int *lens, int tile, unsigned *items);
int isal_hip_ragged_create(isal_hip_ragged **out, int k, int rows, const unsigned char *gftbls,
                           int nstripes, const int *lens, unsigned char *const *data,
                           unsigned char *const *coding, int *bad_stripe);
int isal_hip_ragged_encode(isal_hip_ragged *r, void *stream);
int isal_hip_ragged_check(isal_hip_ragged *r, unsigned long long *bad, void *stream);
int isal_hip_ragged_crc(isal_hip_ragged *r, unsigned int init, unsigned int *crc, void *stream);
int isal_hip_ragged_encode_crc(isal_hip_ragged *r, unsigned int init, unsigned int *crc, void *stream);
int isal_hip_ragged_crc64(isal_hip_ragged *r, int variant, unsigned long long init,
                          unsigned long long *crc, void *stream);
int isal_hip_ragged_encode_crc64(isal_hip_ragged *r, int variant, unsigned long long init,
                                 unsigned long long *crc, void *stream);
int isal_hip_ragged_destroy(isal_hip_ragged *r);

/* ---- sector checksums: one word per 512 B .. 4 KiB of every shard --------- */

/*
 * Where the entry points above checksum whole shards (what Ceph's EC hash info
 * stores), these keep ONE WORD PER FIXED-SIZE SECTOR of every shard: HDFS
 * striped block groups (CRC32C per 512-byte bytesPerChecksum chunk), BlueStore
 * (CRC32C per 4 KiB csum block), NVMe end-to-end protection (a guard per 512 B
 * or 4 KiB logical block; its 64-bit guard is ISAL_HIP_CRC64_ROCKSOFT_REFL).
 * After a scrub has named a shard they also say which sector of it to rebuild.
 *
 * sector is a power of two, 512 <= sector <= 4096. A shard of len bytes has
 * ns = ceil(len / sector) sectors; sector i covers bytes [i*sector,
 * min((i+1)*sector, len)): the last one may be short, down to 1 byte, and a
 * shard of length 0 has none. Each sector's word is what the reference
 * function returns for those bytes alone, with the same init for every sector:
 *   crc32_iscsi(p, n, init)        (the register starts at init, no inversion)
 *   crc64_<variant>(init, p, n)    (starts at ~init, inverted on return)
 * crc is a DEVICE array; with m = k + rows and shard j of a stripe its source
 * j (j < k) or its parity row j - k:
 *   isal_hip_batch_sector_crc, _crc64    crc[(s*m + j)*ns + i]
 *   isal_hip_ragged_sector_crc, _crc64   crc[m*first[s] + j*ns_s + i], ns_s =
 *       ceil(lens[s] / sector), first[s] = the sum of ns_t over t < s
 * isal_hip_ragged_sector_offsets: pure arithmetic, no GPU: fills first[0 ..
 *   nstripes) (first may be NULL) and returns the sum over all stripes, so crc
 *   holds m times the returned count; -1 for arguments outside the contract
 *   (NULL lens, nstripes <= 0, a negative length, a bad sector).
 * The four launch functions:
 *   ISAL_HIP_EINVAL, with nothing enqueued and no HIP call (so a host without a
 *   GPU answers the same), for a NULL object or crc, a sector that is not one
 *   of 512, 1024, 2048, 4096, a variant outside [0, ISAL_HIP_CRC64_NVARIANTS),
 *   on the uniform batch any shard not 16-byte aligned (isal_hip_batch_check's
 *   rule), and more than 2^30 work items (4 KiB tiles of every shard) in the
 *   launch, which is refused, not sliced.
 *   A call only enqueues, on the caller's stream and the object's device,
 *   whatever the calling thread's current device: exactly ONE kernel launch
 *   (isal_hip_kernel_launches grows by 1), no combine launch and no partials
 *   in global memory, because a sector never leaves a 4 KiB tile. With len ==
 *   0, or every ragged length 0, it returns 0, enqueues nothing and leaves crc
 *   untouched. Idempotent: every word of every sector is rewritten by each
 *   call, nothing is written past the last word or to the shards, and nothing
 *   is read at or past a shard's own length.
 *   Memory, freed by the object's destroy: the first call with a flavour
 *   uploads that flavour's tables (9.6 KiB for CRC32C, 31.5 KiB per crc64
 *   variant), which depend on the flavour only, never on a length or on
 *   sector; the first ragged call with a sector size uploads first[] for it (8
 *   bytes per stripe); the ragged work items are the encode's 4 KiB {stripe,
 *   tile} table. A failed allocation returns ISAL_HIP_ENOMEM or ISAL_HIP_EHIP,
 *   leaves no HIP error behind and the object as usable as before.
 * Out of scope: sectors below 512 B or above one 4 KiB tile; the rest of crc.h
 * (crc32_ieee, crc32_gzip_refl); fusing into the encode pass; unaligned or
 * host-pageable shards; any CPU route; the drop-in ABI. (The 16-bit guard and
 * the comparison with stored checksums on the device: "T10 protection
 * information" below.)
 */
int isal_hip_batch_sector_crc(isal_hip_batch *b, int sector, unsigned int init, unsigned int *crc,
                              void *stream);
int isal_hip_batch_sector_crc64(isal_hip_batch *b, int variant, int sector, unsigned long long init,
                                unsigned long long *crc, void *stream);
long long isal_hip_ragged_sector_offsets(int nstripes, const int *lens, int sector, long long *first);
int isal_hip_ragged_sector_crc(isal_hip_ragged *r, int sector, unsigned int init, unsigned int *crc,
                               void *stream);
int isal_hip_ragged_sector_crc64(isal_hip_ragged *r, int variant, int sector, unsigned long long init,
                                 unsigned long long *crc, void *stream);

/* ---- T10 protection information: guard, generate and verify per sector ---- */

/*
 * The 8-byte tuple that T10 DIF types 1-3 and NVMe protection information with
 * the 16-bit guard keep per logical block, in the DIX layout (the tuples in an
 * array of their own, not interleaved with the data):
 *   bytes 0-1  guard: crc16_t10dif of the sector's bytes (the reference's
 *              crc16_t10dif(seed, p, n): a normal CRC, polynomial x^16 +
 *              0x8BB7, the register starts at seed, no final XOR; "123456789"
 *              from 0 gives 0xD0DB)
 *   bytes 2-3  application tag
 *   bytes 4-7  reference tag: ref0 of the shard for ISAL_HIP_DIF_TYPE3, ref0 +
 *              i (mod 2^32) for sector i under ISAL_HIP_DIF_TYPE1 (also type 2)
 * each field most significant byte first. Sectors, their indexing and a short
 * last sector (its guard covers the bytes that exist) are the sector
 * checksums' above: word or tuple (s*m + j)*ns + i on the uniform batch,
 * m*first[s] + j*ns_s + i on the ragged one (isal_hip_ragged_sector_offsets).
 * All arrays are DEVICE memory:
 *   crc   one 16-bit word per sector
 *   pi    8 bytes per sector, 8-byte aligned
 *   bad, d->ref0   one 32-bit word per shard, at s*m + j (ref0 NULL: all 0)
 *   _sector_t10dif  crc[w] = the guard, with the same seed for every sector.
 *   _dif_generate   pi[8w .. 8w+8) = the tuple (d->seed, d->app_tag, d->type,
 *                   d->ref0; d->flags is not looked at).
 *   _dif_verify     compares the stored tuple of every sector with the one
 *                   generate would write, in the fields d->flags names
 *                   (ISAL_HIP_DIF_CHECK_*). bad[s*m + j] = ISAL_HIP_DIF_CLEAN
 *                   when no sector of the shard fails, else (i << 3) | kinds
 *                   for the FIRST failing sector i, kinds the OR of the
 *                   CHECK_* bits that failed in that sector. Escape rule: a
 *                   sector is not checked at all when its stored application
 *                   tag is 0xFFFF (type 1) or its stored application tag is
 *                   0xFFFF and its stored reference tag 0xFFFFFFFF (type 3).
 *                   Unlike the scrub's verdict (at most ONE shard per stripe,
 *                   from the syndrome) this names every bad shard, up to the
 *                   m - k a repair can take, and the sector to start at: the
 *                   erasure list of isal_hip_repair_create[_ragged].
 * Refusals (ISAL_HIP_EINVAL before any HIP call, nothing enqueued), object
 * behaviour and device routing are the sector checksums': a NULL object, d,
 * crc, pi or bad, a bad sector, a type other than the two above, flags outside
 * the three bits, a pi not 8-byte aligned, unaligned shards on the uniform
 * batch, more than 2^30 work items. With every length 0 a call returns 0,
 * enqueues nothing and writes nothing (bad included). The words and generate
 * enqueue exactly ONE kernel launch; verify enqueues a fill of bad with 0xff
 * bytes and then ONE kernel launch, whose only writes are atomic minima of
 * failing sectors (a clean batch issues none). Stream-ordered on the caller's
 * stream, on the object's device, idempotent. The first call uploads the
 * guard's tables (7 KiB, freed by the object's destroy); a failed upload
 * returns ISAL_HIP_ENOMEM or ISAL_HIP_EHIP and leaves no HIP error behind.
 * Out of scope: the drop-in symbols crc16_t10dif[_copy][_base] and a
 * whole-shard CRC-16; crc32_ieee, crc32_gzip_refl; application-tag masks; the
 * 32- and 64-bit NVMe guards as tuples; fusing into the encode pass; any CPU
 * route; interleaved data + PI (DIF proper).
 */
#define ISAL_HIP_DIF_TYPE1 1          /* also type 2: ref tag of sector i = ref0 + i (mod 2^32) */
#define ISAL_HIP_DIF_TYPE3 3          /* ref tag = ref0 for every sector of the shard */
#define ISAL_HIP_DIF_CHECK_GUARD 1u   /* also the bit of `kinds` in a verify word */
#define ISAL_HIP_DIF_CHECK_APP   2u
#define ISAL_HIP_DIF_CHECK_REF   4u
#define ISAL_HIP_DIF_CLEAN 0xffffffffu
typedef struct {
        int type;
        unsigned flags;               /* verify only */
        unsigned short app_tag;
        unsigned short seed;          /* crc16 seed, normally 0 */
        const unsigned int *ref0;     /* DEVICE, one word per shard in pi order; NULL: all 0 */
} isal_hip_dif;

int isal_hip_batch_sector_t10dif(isal_hip_batch *b, int sector, unsigned short seed, unsigned short *crc,
                                 void *stream);
int isal_hip_ragged_sector_t10dif(isal_hip_ragged *r, int sector, unsigned short seed, unsigned short *crc,
                                  void *stream);
int isal_hip_batch_dif_generate(isal_hip_batch *b, int sector, const isal_hip_dif *d, unsigned char *pi,
                                void *stream);
int isal_hip_ragged_dif_generate(isal_hip_ragged *r, int sector, const isal_hip_dif *d, unsigned char *pi,
                                 void *stream);
int isal_hip_batch_dif_verify(isal_hip_batch *b, int sector, const isal_hip_dif *d, const unsigned char *pi,
                              unsigned int *bad, void *stream);
int isal_hip_ragged_dif_verify(isal_hip_ragged *r, int sector, const isal_hip_dif *d, const unsigned char *pi,
                               unsigned int *bad, void *stream);

/* ---- streaming pipeline for HOST-resident stripes ----------------------- */

/*
 * Stripes whose shards live in host memory (NIC / disk buffers) flow through
 * `depth` HBM slots on three HIP streams: host->device copies of the sources,
 * GF arithmetic, device->host copies of the parity, overlapped across stripes.
 *   ISAL_HIP_PIPE_UPDATE: each source is folded into the parity as soon as it
 *                         lands (ec_encode_data_update semantics, parity
 *                         starts zeroed);
 *   ISAL_HIP_PIPE_ENCODE: one ec_encode_data launch once all k sources landed.
 * Pinned host buffers give full copy/compute overlap; pageable ones work but
 * serialise the copies.
 */
#define ISAL_HIP_PIPE_UPDATE 0
#define ISAL_HIP_PIPE_ENCODE 1
/* depth is capped at this many stripes in flight (more only slows the copies) */
#define ISAL_HIP_PIPE_MAX_DEPTH 4

typedef struct isal_hip_pipe isal_hip_pipe;

int isal_hip_pipe_create(isal_hip_pipe **out, int len, int k, int rows,
                         const unsigned char *gftbls, int depth, int mode);

/* Enqueue one stripe: data = k host source pointers, coding = rows host parity
 * pointers (written when the stripe completes). Blocks only while all `depth`
 * slots are busy. Buffers must stay valid until isal_hip_pipe_flush returns. */
int isal_hip_pipe_submit(isal_hip_pipe *p, unsigned char *const *data, unsigned char *const *coding);

/* Wait until every submitted stripe's parity is in host memory. */
int isal_hip_pipe_flush(isal_hip_pipe *p);

int isal_hip_pipe_destroy(isal_hip_pipe *p);

/* ---- several GPUs from one process ---------------------------------------- */

/*
 * Host-resident stripes encoded on ndev GPUs at once (0 = every visible GPU).
 * A call's stripes are split into contiguous, balanced ranges
 * (isal_hip_multi_partition); GPU d streams its range through its own
 * pipeline (as isal_hip_pipe, mode ENCODE) on its own host thread, so the
 * GPUs never exchange data. isal_hip_multi_encode blocks until every parity
 * shard is in host memory; data[s*k + j] / coding[s*rows + l] are host
 * pointers (pinned for full copy/compute overlap). Callers whose shards are
 * already in each GPU's HBM use one isal_hip_batch per device instead.
 * Each device's worker thread runs on the CPUs of the device's NUMA node
 * (sysfs; ISAL_HIP_SYSFS_ROOT overrides "/sys"), within the process's own
 * affinity. One handle runs one isal_hip_multi_encode at a time: a second
 * thread calling it on the same handle blocks until the first returns.
 */
typedef struct isal_hip_multi isal_hip_multi;

int isal_hip_multi_create(isal_hip_multi **out, int ndev, int len, int k, int rows,
                          const unsigned char *gftbls, int depth);
int isal_hip_multi_ndev(const isal_hip_multi *m);
int isal_hip_multi_encode(isal_hip_multi *m, long long nstripes, unsigned char *const *data,
                          unsigned char *const *coding);
int isal_hip_multi_destroy(isal_hip_multi *m);

/* NUMA node of device dev's PCIe root (-1 unknown), and how many CPUs its
 * worker thread is pinned to (0 = not pinned). */
int isal_hip_multi_numa_node(const isal_hip_multi *m, int dev);
int isal_hip_multi_worker_cpus(const isal_hip_multi *m, int dev);

/* sysfs lookups behind the pinning (root NULL = ISAL_HIP_SYSFS_ROOT or /sys):
 * the NUMA node of a PCI device ("0000:05:00.0"; -1 unknown), and the CPUs of
 * a node's cpulist into cpus[0..max) (returns how many it lists, -1 on error). */
int isal_hip_pci_numa_node(const char *root, const char *pci_bus_id);
int isal_hip_numa_node_cpus(const char *root, int node, int *cpus, int max);

/* Stripes [*first, *first + *count) of nstripes belong to device (or rank)
 * dev of ndev: contiguous, covering, sizes differ by at most one. Pure
 * arithmetic, no GPU needed. */
void isal_hip_multi_partition(long long nstripes, int ndev, int dev, long long *first,
                              long long *count);

/* ---- routing of the drop-in calls and configuration --------------------- */

/*
 * The synchronous drop-in calls (erasure_code.h, gf_vect_mul.h, raid.h) route
 * each call by where its shards live and how large it is:
 *   - any device-resident shard: the GPU kernels. An encode whose shards are
 *     all device-resident and 16-byte aligned, with k + rows <= 32, rows <= 8
 *     and k * rows <= 89, passes its shard pointers and coefficient tables as
 *     kernel arguments: one launch and one stream synchronisation per call
 *     (ISAL_HIP_KARG=0 uploads them with a copy instead);
 *   - host-resident shards, (k + rows) * len > ISAL_HIP_CPU_MAX_BYTES: the GPU
 *     kernels. Page-locked host shards (hipHostMalloc / hipHostRegister) are
 *     read and written in place through their device mapping when the whole
 *     shard lies in one registration (an update's parity excepted: staged);
 *     pageable ones, and page-locked shards that run past their
 *     registration, are staged through HBM, in pipelined 4 MiB column chunks
 *     when longer (ISAL_HIP_CHUNK_KB, ISAL_HIP_PIPE_CHUNKS=0 for one chunk,
 *     ISAL_HIP_PINNED_DIRECT=0 to stage page-locked shards too);
 *   - host-resident shards up to ISAL_HIP_CPU_MAX_BYTES (default 8 MiB; when
 *     every shard is page-locked, ISAL_HIP_CPU_MAX_BYTES_PINNED, default
 *     2 MiB), or a host without a usable GPU: the engine's CPU route.
 * Per calling thread the library keeps a blocking HIP stream, a pinned
 * argument buffer and the last call's coefficient tables. A thread that makes
 * a large staged host call also gets a copy-out helper thread, two more
 * streams and nine events, kept until the thread exits: at most
 * ISAL_HIP_MAX_HELPERS (default 8) helpers live in a process — a thread
 * beyond that issues its copies alone (slower, same result). Streams share
 * the process's GPU_MAX_HW_QUEUES hardware queues.
 * ISAL_HIP_BACKEND=gpu forces the kernels for every call (and aborts when no
 * GPU is usable), =cpu sends every host-resident call to the CPU route,
 * =auto (default) is the rule above. Routing classifies each shard pointer
 * with hipPointerGetAttributes, so the HIP runtime is initialised on a host
 * with a GPU even under =cpu (device-resident shards still go to the GPU).
 * If a HIP call fails during a host-resident call, the call completes on the
 * CPU route and the failure is reported once on stderr; ISAL_HIP_LOG=1 logs
 * every call's route.
 * Several GPUs: the reference API has no device argument, so a call runs on
 * the GPU that holds its device-resident (hipMalloc) shards — the thread's
 * current device is switched to it for the call and restored before the call
 * returns — else, with no such shard, on the thread's current device. All of
 * one call's device-resident shards must be on ONE GPU (a call that mixes GPUs
 * aborts, naming the entry point: no kernel and no CPU route can reach both).
 * Managed memory runs on either; page-locked host memory is used in place
 * only on the GPU it was registered with, and staged elsewhere. A thread keeps
 * one context (stream, buffers, mailbox) per GPU it has called on.
 * Environment knobs are read once; isal_hip_config_reload() re-reads them
 * (call it only while no other thread is inside the library).
 */
void isal_hip_config_reload(void);

/* The device choice above as a pure function (test hook; the drop-in calls use
 * it): n shards with kind[i] (ISAL_HIP_MEM_*) and dev[i] (the device their
 * pointer attributes name; read for DEVICE and PINNED only), the caller's
 * current device cur. Returns the device the call runs on (-1: none, cur < 0
 * and no device shard), -2 when device shards are on two GPUs (*bad = the
 * first shard on a second one; -1 otherwise), -3 for bad arguments.
 * in_place[i] (optional): 1 where a kernel on that device uses shard i where it
 * lies, 0 where it must be staged through HBM. */
#define ISAL_HIP_MEM_PAGEABLE 0
#define ISAL_HIP_MEM_DEVICE 1
#define ISAL_HIP_MEM_MANAGED 2
#define ISAL_HIP_MEM_PINNED 3
int isal_hip_route_device(int n, const int *kind, const int *dev, int cur, int *bad, int *in_place);

/* Per-thread, per-device contexts the drop-in calls have created since the
 * process started (a thread's first call on each GPU makes one). */
unsigned long long isal_hip_contexts_created(void);

/* Kernel-argument drop-in calls whose completion word had not arrived after
 * the 20 ms spin, so that hipStreamSynchronize completed them (the kernel
 * waited behind other work, or ran long). */
unsigned long long isal_hip_slow_waits(void);

/* Drop-in calls served by the CPU route, and of those the HIP-failure
 * fallbacks, since the process started. */
unsigned long long isal_hip_cpu_calls(void);
unsigned long long isal_hip_fallbacks(void);

/* ---- introspection (tests, benchmarks) --------------------------------- */

/* Number of erasure-code kernels this process has launched through the engine. */
unsigned long long isal_hip_kernel_launches(void);

/* Maximum parity rows one kernel pass produces (larger rows are split into passes). */
int isal_hip_max_rows_per_pass(void);

/* Name of the compiled GPU target ("gfx950"). */
const char *isal_hip_target(void);

/* Ask the HIP runtime for the attributes of every kernel the library's
 * launchers can launch (each registers itself when the library loads):
 * returns how many have no usable device code (0: all present; each one is
 * named on stderr), ISAL_HIP_EHIP without a usable GPU. *nkernels (optional)
 * receives how many were checked. */
int isal_hip_selftest_kernels(int *nkernels);

#ifdef __cplusplus
}
#endif

#endif /* ISAL_HIP_ISAL_HIP_H */
