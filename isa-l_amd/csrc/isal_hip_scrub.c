/*
 * isal_hip_scrub.c — the scrub batch (isal_hip.h): nstripes encoded stripes of
 * one geometry are verified by one kernel launch, and every inconsistent
 * stripe gets the index of the one shard that explains its mismatches.
 *
 * The arithmetic: for a byte column, e[l] = stored parity row l ^ the parity
 * recomputed from the stored sources. One corrupt data shard j (changed by d)
 * leaves e = C[:, j] * d, one corrupt parity row l leaves e non-zero in row l
 * only: e is a multiple of one column of [C | I]. When no two of those
 * k + rows columns are proportional (isal_hip_scrub_ambiguity), at most one
 * shard explains a syndrome.
 *
 * Host side, in this order (everything before the first HIP call is pure
 * arithmetic and returns the same codes on a host without a GPU; the steps
 * every stripe object shares are isal_hip_objects.c's):
 *   1. counts, then every shard pointer (non-NULL, 16-byte aligned) while the
 *      pointer table (per stripe k sources then rows parity rows) is written;
 *   2. the matrix is refused when two shards could explain one syndrome;
 *   3. gftbls becomes the encode's device coefficient tables and 0/1 masks
 *      (the verify's hot path) and the location tables of the kernel's
 *      mismatch branch: the raw coefficients, each column's first row with a
 *      non-zero coefficient, and that coefficient's inverse.
 * A scrub batch belongs to the device that was current when it was created
 * (ON_BATCH_DEVICE).
 *
 * The ragged scrub (isal_hip_scrub_create_ragged) is the same object, built by
 * the same create body (scrub_create), where every stripe has its own length:
 * step 1 also takes each stripe's length,
 * the item count at the 4 KiB tile is checked against the launch limit before
 * step 2, and the upload also builds the work-item table of the ragged batch
 * (isal_hip_ragged_items). Its run is one ec_locate_rag launch over that table,
 * always in the plain lookup form, so it keeps no 0/1 masks.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "erasure_code.h"
#include "isal_hip.h"
#include "isal_hip_internal.h"

struct isal_hip_scrub {
        int len, k, rows, nstripes, device;
        uint64_t *d_ptrs;
        uint32_t *d_tbl;
        unsigned char *d_loc;
        isal_hip_encmask em;
        /* the ragged kind: per-stripe lengths and the 4 KiB item table (len unused) */
        int ragged;
        unsigned nitems;
        int *d_lens;
        unsigned *d_items;
};

/* C[l][j] for j < k, the identity's column j - k beyond */
static unsigned char
col_at(int k, const unsigned char *gftbls, int l, int j)
{
        return j < k ? gftbls[32 * ((size_t) l * k + j) + 1] : (unsigned char) (j - k == l);
}

/* first row with a non-zero entry in column j of [C | I], rows when none */
static int
col_pivot(int k, int rows, const unsigned char *gftbls, int j)
{
        int l;
        for (l = 0; l < rows && !col_at(k, gftbls, l, j); l++)
                ;
        return l;
}

static int
matrix_args_bad(int k, int rows, const unsigned char *gftbls)
{
        return k < 1 || rows < 1 || k + rows > MAX_SHARDS || !gftbls;
}

int
isal_hip_scrub_ambiguity(int k, int rows, const unsigned char *gftbls, int pair[2])
{
        unsigned char piv[MAX_SHARDS], inv[MAX_SHARDS];
        int a, b, l, n;
        if (pair)
                pair[0] = pair[1] = -1;
        if (matrix_args_bad(k, rows, gftbls))
                return ISAL_HIP_EINVAL;
        n = k + rows;
        for (a = 0; a < n; a++) {
                const int p = col_pivot(k, rows, gftbls, a);
                piv[a] = (unsigned char) p;
                inv[a] = p < rows ? gf_inv(col_at(k, gftbls, p, a)) : 0;
        }
        for (a = 0; a < n; a++) {
                if (piv[a] >= rows) {
                        b = a; /* a zero column: no corruption of shard a shows */
                        goto found;
                }
                for (b = a + 1; b < n; b++) {
                        unsigned char d;
                        if (piv[b] != piv[a])
                                continue;
                        /* column b = d * column a ? */
                        d = gf_mul(col_at(k, gftbls, piv[a], b), inv[a]);
                        for (l = 0; l < rows; l++)
                                if (gf_mul(col_at(k, gftbls, l, a), d) != col_at(k, gftbls, l, b))
                                        break;
                        if (l == rows)
                                goto found;
                }
        }
        return ISAL_HIP_OK;
found:
        if (pair) {
                pair[0] = a;
                pair[1] = b;
        }
        return ISAL_HIP_ESINGULAR;
}

int
isal_hip_locate_syndrome(int k, int rows, const unsigned char *gftbls, const unsigned char *syndrome)
{
        int j, l, nz = 0, last = -1;
        if (matrix_args_bad(k, rows, gftbls) || !syndrome)
                return (int) ISAL_HIP_SCRUB_MULTI;
        for (l = 0; l < rows; l++)
                if (syndrome[l]) {
                        nz++;
                        last = l;
                }
        if (!nz)
                return (int) ISAL_HIP_SCRUB_CLEAN;
        for (j = 0; j < k; j++) {
                const int p = col_pivot(k, rows, gftbls, j);
                unsigned char d;
                if (p == rows)
                        continue;
                d = gf_mul(syndrome[p], gf_inv(col_at(k, gftbls, p, j)));
                if (!d)
                        continue;
                for (l = 0; l < rows && gf_mul(col_at(k, gftbls, l, j), d) == syndrome[l]; l++)
                        ;
                if (l == rows)
                        return j;
        }
        return nz == 1 ? k + last : (int) ISAL_HIP_SCRUB_MULTI;
}

/* The kernel's view of the matrix (isal_hip_internal.h): rows * k + 2 * k bytes. */
static void
build_loc(int k, int rows, const unsigned char *gftbls, unsigned char *loc)
{
        unsigned char *piv = loc + (size_t) rows * k, *inv = piv + k;
        int l, j;
        for (l = 0; l < rows; l++)
                for (j = 0; j < k; j++)
                        loc[(size_t) l * k + j] = col_at(k, gftbls, l, j);
        for (j = 0; j < k; j++) {
                const int p = col_pivot(k, rows, gftbls, j);
                piv[j] = p < rows ? (unsigned char) p : 0xff;
                inv[j] = p < rows ? gf_inv(col_at(k, gftbls, p, j)) : 0;
        }
}

/* lens: the ragged kind's (NULL for one len). Its item table (s->nitems rows)
 * is built here, after the pointers have been classified: a batch near the
 * item limit with unreachable shards is refused without 8 GiB of host table. */
static int
scrub_upload(isal_hip_scrub *s, const uint64_t *h_ptrs, const uint32_t *h_tbl, const unsigned char *h_loc,
             const int *lens)
{
        const size_t stride = (size_t) (s->k + s->rows), nstripes = (size_t) s->nstripes;
        const size_t ntbl = isal_hip_tables_dwords(s->k, s->rows) * 4;
        int e;
        if (hipGetDevice(&s->device) != hipSuccess)
                return ISAL_HIP_EHIP;
        if ((e = isal_hip_obj_reach(h_ptrs, nstripes, stride, (size_t) s->len, lens, s->device)) != ISAL_HIP_OK ||
            (e = isal_hip_obj_put(&s->d_ptrs, h_ptrs, nstripes * stride * 8, 0)) != ISAL_HIP_OK ||
            (e = isal_hip_obj_put(&s->d_tbl, h_tbl, ntbl, 4)) != ISAL_HIP_OK ||
            (e = isal_hip_obj_put(&s->d_loc, h_loc, (size_t) (s->rows + 2) * (size_t) s->k, 0)) != ISAL_HIP_OK)
                return e;
        if (!lens)
                return ISAL_HIP_OK;
        if ((e = isal_hip_obj_put(&s->d_lens, lens, nstripes * sizeof(int), 0)) != ISAL_HIP_OK)
                return e;
        return isal_hip_obj_put_items(&s->d_items, s->nstripes, lens, ISAL_HIP_RAGGED_TILE, s->nitems);
}

/* Both kinds of object: the uniform one of len (lens == NULL) and the ragged
 * one, which must have its lens. */
static int
scrub_create(isal_hip_scrub **out, int ragged, int len, const int *lens, int k, int rows,
             const unsigned char *gftbls, int nstripes, unsigned char *const *data, unsigned char *const *coding,
             int *bad_stripe)
{
        isal_hip_scrub *sc = NULL;
        uint64_t *h_ptrs = NULL;
        uint32_t *h_tbl = NULL;
        unsigned char *h_loc = NULL;
        long long s, n = 0;
        int ret = ISAL_HIP_OK;
        size_t stride;

        if (bad_stripe)
                *bad_stripe = -1;
        if (!out)
                return ISAL_HIP_EINVAL;
        *out = NULL;
        /* one row cannot tell shards apart; a syndrome must be whole inside
         * one pass of the kernel */
        if (len < 0 || k < 1 || rows < 2 || rows > EC_MAX_ROWS_PER_PASS || k + rows > MAX_SHARDS || !gftbls ||
            nstripes < 1 || (ragged && !lens) || !data || !coding)
                return ISAL_HIP_EINVAL;
        stride = (size_t) k + (size_t) rows;

        h_ptrs = (uint64_t *) malloc((size_t) nstripes * stride * 8);
        if (!h_ptrs)
                return ISAL_HIP_ENOMEM;
        /* 1: every stripe's length and pointers while its table row is written */
        for (s = 0; s < nstripes && ret == ISAL_HIP_OK; s++) {
                uint64_t *hp = h_ptrs + (size_t) s * stride;
                if (isal_hip_obj_ptr_row(hp, data + (size_t) s * k, (size_t) k) != ISAL_HIP_OK ||
                    isal_hip_obj_ptr_row(hp + k, coding + (size_t) s * rows, (size_t) rows) != ISAL_HIP_OK ||
                    (lens && lens[s] < 0))
                        ret = ISAL_HIP_EINVAL;
                if (ret != ISAL_HIP_OK && bad_stripe)
                        *bad_stripe = (int) s;
        }
        /* one launch covers every item (the only tile size here is 4 KiB) */
        if (ret == ISAL_HIP_OK && lens &&
            (n = isal_hip_ragged_items(nstripes, lens, ISAL_HIP_RAGGED_TILE, NULL)) > (long long) ISAL_HIP_RAGGED_MAX_ITEMS)
                ret = ISAL_HIP_EINVAL;
        /* 2: two shards that explain the same syndrome cannot be told apart */
        if (ret == ISAL_HIP_OK)
                ret = isal_hip_scrub_ambiguity(k, rows, gftbls, NULL);
        if (ret != ISAL_HIP_OK)
                goto done;

        /* 3: the encode's tables, the mismatch branch's tables; the uniform
         * kind's masks, the ragged kind's item table at the upload */
        h_tbl = (uint32_t *) malloc(isal_hip_tables_dwords(k, rows) * 4 + 4);
        h_loc = (unsigned char *) malloc((size_t) (rows + 2) * (size_t) k);
        sc = (isal_hip_scrub *) calloc(1, sizeof(*sc));
        if (!h_tbl || !h_loc || !sc) {
                ret = ISAL_HIP_ENOMEM;
                goto done;
        }
        isal_hip_build_tables(k, rows, gftbls, h_tbl);
        build_loc(k, rows, gftbls, h_loc);
        if (!lens)
                isal_hip_enc_masks(k, rows, gftbls, &sc->em);
        sc->ragged = lens != NULL;
        sc->nitems = (unsigned) n;
        sc->len = len;
        sc->k = k;
        sc->rows = rows;
        sc->nstripes = nstripes;
        ret = scrub_upload(sc, h_ptrs, h_tbl, h_loc, lens);
done:
        free(h_ptrs);
        free(h_tbl);
        free(h_loc);
        if (ret != ISAL_HIP_OK) {
                isal_hip_scrub_destroy(sc);
                return ret;
        }
        *out = sc;
        return ISAL_HIP_OK;
}

int
isal_hip_scrub_create(isal_hip_scrub **out, int len, int k, int rows, const unsigned char *gftbls, int nstripes,
                      unsigned char *const *data, unsigned char *const *coding, int *bad_stripe)
{
        return scrub_create(out, 0, len, NULL, k, rows, gftbls, nstripes, data, coding, bad_stripe);
}

int
isal_hip_scrub_create_ragged(isal_hip_scrub **out, int k, int rows, const unsigned char *gftbls, int nstripes,
                             const int *lens, unsigned char *const *data, unsigned char *const *coding,
                             int *bad_stripe)
{
        return scrub_create(out, 1, 0, lens, k, rows, gftbls, nstripes, data, coding, bad_stripe);
}

static int
scrub_run_impl(isal_hip_scrub *s, unsigned int *verdict, void *stream)
{
        if (s->ragged)
                return isal_hip_launch_locate_ragged(s->d_ptrs, s->k + s->rows, s->d_tbl, s->d_lens, s->d_items,
                                                     s->nitems, s->k, s->rows, s->nstripes, s->d_loc, verdict, stream)
                               ? ISAL_HIP_EHIP
                               : ISAL_HIP_OK;
        return isal_hip_launch_locate_batch(s->d_ptrs, s->k + s->rows, s->d_tbl, s->len, s->k, s->rows, s->nstripes,
                                            &s->em, s->d_loc, verdict, stream)
                       ? ISAL_HIP_EHIP
                       : ISAL_HIP_OK;
}

int
isal_hip_scrub_run(isal_hip_scrub *s, unsigned int *verdict, void *stream)
{
        if (!verdict)
                return ISAL_HIP_EINVAL;
        ON_BATCH_DEVICE(s, scrub_run_impl(s, verdict, stream));
}

int
isal_hip_scrub_destroy(isal_hip_scrub *s)
{
        if (!s)
                return ISAL_HIP_OK;
        isal_hip_obj_drop(s->d_ptrs);
        isal_hip_obj_drop(s->d_tbl);
        isal_hip_obj_drop(s->d_loc);
        isal_hip_obj_drop(s->d_lens);
        isal_hip_obj_drop(s->d_items);
        free(s);
        return ISAL_HIP_OK;
}
