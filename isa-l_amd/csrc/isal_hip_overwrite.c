/*
 * isal_hip_overwrite.c — the overwrite batch (isal_hip.h): nstripes encoded
 * stripes of one geometry, each with its own set of nw rewritten data shards,
 * whose deltas (old ^ new) are folded into the parity by one kernel launch
 * per pass of up to EC_MAX_ROWS_PER_PASS rows.
 *
 * Host side, in this order (everything before the first HIP call is pure
 * arithmetic and returns the same codes on a host without a GPU; the steps
 * every stripe object shares are isal_hip_objects.c's):
 *   1. each stripe's indices are checked (in range, distinct), its pointers
 *      (non-NULL, 16-byte aligned) and its 2 * nw + rows byte ranges (sorted
 *      by address, neighbours must not overlap);
 *   2. the pointer table (per stripe nw old shards, the nw new ones, then the
 *      rows parity rows) and the index table (a dword per slot) are written;
 *   3. gftbls becomes the batch's device coefficient tables
 *      (isal_hip_build_tables), which the kernel addresses per column.
 * An overwrite batch belongs to the device that was current when it was
 * created (ON_BATCH_DEVICE).
 *
 * The ragged overwrite (isal_hip_overwrite_create_ragged) is the same object,
 * built by the same create body (overwrite_create), where stripe s has its own
 * length lens[s] and its own count nw[s] of the max_nw slots a table row
 * holds. Step 1 looks at a stripe's live slots only (the first nw[s] of its
 * row) and compares their ranges over lens[s]; step 2 writes the tables at
 * stride max_nw with the other slots zeroed; the upload adds the lengths, the
 * counts and the work-item table of the ragged batch (isal_hip_ragged_items at
 * the 2 KiB tile, where a stripe without a slot counts as empty). Its run is
 * one ec_overwrite_rag launch per pass over that table, whatever the mix of
 * lengths and counts.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "isal_hip.h"
#include "isal_hip_internal.h"

struct isal_hip_overwrite {
        int len, k, rows, nw, nstripes, device;
        uint64_t *d_ptrs;
        uint32_t *d_idx, *d_tbl;
        /* the ragged kind: nw is the stride max_nw, len unused; per-stripe
         * lengths (0 where the count is 0) and counts, the 2 KiB item table */
        int ragged;
        unsigned nitems;
        int *d_lens, *d_nw;
        unsigned *d_items;
};

static int
cmp_u64(const void *a, const void *b)
{
        const uint64_t x = *(const uint64_t *) a, y = *(const uint64_t *) b;
        return x < y ? -1 : x > y;
}

/* The live pointers of one table row (stride 2 * nw + rows) whose stripe uses
 * c of its nw slots: c old shards, the c new ones, the parity rows. Returns
 * their number. */
static size_t
live_row(uint64_t *live, const uint64_t *row, size_t nw, size_t c, size_t rows)
{
        memcpy(live, row, c * 8);
        memcpy(live + c, row + nw, c * 8);
        memcpy(live + 2 * c, row + 2 * nw, rows * 8);
        return 2 * c + rows;
}

/* No two of the n ranges [p, p + len) overlap. sorted: scratch. */
static int
ranges_apart(const uint64_t *p, size_t n, size_t len, uint64_t *sorted)
{
        size_t i;
        if (!len)
                return ISAL_HIP_OK;
        memcpy(sorted, p, n * 8);
        qsort(sorted, n, 8, cmp_u64);
        for (i = 1; i < n; i++)
                if (sorted[i] - sorted[i - 1] < len)
                        return ISAL_HIP_EINVAL;
        return ISAL_HIP_OK;
}

/* lens, nws: the ragged kind's (NULL for one len and one count), lens[s] 0
 * where stripe s has no slot. Its item table (o->nitems rows) is built here,
 * after the pointers have been classified, as the ragged scrub does. */
static int
overwrite_upload(isal_hip_overwrite *o, const uint64_t *h_ptrs, const uint32_t *h_idx, const uint32_t *h_tbl,
                 const int *lens, const int *nws, uint64_t *live)
{
        const size_t nstripes = (size_t) o->nstripes, mw = (size_t) o->nw, stride = 2 * mw + (size_t) o->rows;
        const size_t ntbl = isal_hip_tables_dwords(o->k, o->rows) * 4;
        size_t s;
        int e = ISAL_HIP_OK;
        if (hipGetDevice(&o->device) != hipSuccess)
                return ISAL_HIP_EHIP;
        if (!lens)
                e = isal_hip_obj_reach(h_ptrs, nstripes, stride, (size_t) o->len, NULL, o->device);
        /* a ragged stripe's live shards are as long as that stripe */
        for (s = 0; lens && s < nstripes && e == ISAL_HIP_OK; s++)
                if (lens[s] > 0) {
                        const size_t n = live_row(live, h_ptrs + s * stride, mw, (size_t) nws[s], (size_t) o->rows);
                        e = isal_hip_obj_reach(live, 1, n, (size_t) lens[s], NULL, o->device);
                }
        if (e != ISAL_HIP_OK || (e = isal_hip_obj_put(&o->d_ptrs, h_ptrs, nstripes * stride * 8, 0)) != ISAL_HIP_OK ||
            (e = isal_hip_obj_put(&o->d_idx, h_idx, nstripes * mw * 4, 0)) != ISAL_HIP_OK ||
            (e = isal_hip_obj_put(&o->d_tbl, h_tbl, ntbl, 4)) != ISAL_HIP_OK)
                return e;
        if (!lens)
                return ISAL_HIP_OK;
        if ((e = isal_hip_obj_put(&o->d_lens, lens, nstripes * sizeof(int), 0)) != ISAL_HIP_OK ||
            (e = isal_hip_obj_put(&o->d_nw, nws, nstripes * sizeof(int), 0)) != ISAL_HIP_OK)
                return e;
        return isal_hip_obj_put_items(&o->d_items, o->nstripes, lens, ISAL_HIP_RAGGED_TILE_SMALL, o->nitems);
}

/* Both kinds of object. The uniform one: every stripe len bytes and all nw
 * slots of its row (lens == nws == NULL). The ragged one: stripe s lens[s]
 * bytes and the first nws[s] of the nw slots. */
static int
overwrite_create(isal_hip_overwrite **out, int ragged, int len, const int *lens, int k, int rows,
                 const unsigned char *gftbls, int nw, const int *nws, int nstripes, const unsigned char *idx,
                 unsigned char *const *old_data, unsigned char *const *new_data, unsigned char *const *coding,
                 int *bad_stripe)
{
        isal_hip_overwrite *o = NULL;
        unsigned char mark[MAX_SHARDS];
        uint64_t *h_ptrs = NULL, *live = NULL, *sorted = NULL;
        uint32_t *h_idx = NULL, *h_tbl = NULL;
        int *h_lens = NULL;
        long long s, n = 0;
        int i, ret = ISAL_HIP_OK;
        size_t mw, stride;

        if (bad_stripe)
                *bad_stripe = -1;
        if (!out)
                return ISAL_HIP_EINVAL;
        *out = NULL;
        if (len < 0 || k < 1 || k > MAX_SHARDS || rows < 1 || !gftbls || nstripes < 1 || nw < 1 || nw > k ||
            (ragged && (!lens || !nws)) || !idx || !old_data || !new_data || !coding)
                return ISAL_HIP_EINVAL;
        mw = (size_t) nw;
        stride = 2 * mw + (size_t) rows;

        /* calloc: the slots a stripe does not use stay zero in both tables */
        h_ptrs = (uint64_t *) calloc((size_t) nstripes * stride, 8);
        h_idx = (uint32_t *) calloc((size_t) nstripes * mw, 4);
        live = (uint64_t *) malloc(stride * 8);
        sorted = (uint64_t *) malloc(stride * 8);
        if (ragged)
                h_lens = (int *) malloc((size_t) nstripes * sizeof(int));
        if (!h_ptrs || !h_idx || !live || !sorted || (ragged && !h_lens)) {
                ret = ISAL_HIP_ENOMEM;
                goto done;
        }

        /* 1-2: validate every stripe's live slots while its table rows are
         * written: count and indices, then pointers, then overlaps */
        for (s = 0; s < nstripes && ret == ISAL_HIP_OK; s++) {
                const unsigned char *ix = idx + (size_t) s * mw;
                uint64_t *hp = h_ptrs + (size_t) s * stride;
                const int c = ragged ? nws[s] : nw, ln = ragged ? lens[s] : len;
                if (ln < 0 || c < 0 || c > nw)
                        ret = ISAL_HIP_EINVAL;
                memset(mark, 0, sizeof(mark));
                for (i = 0; i < c && ret == ISAL_HIP_OK; i++) {
                        if (ix[i] >= k || mark[ix[i]])
                                ret = ISAL_HIP_EINVAL;
                        else
                                mark[ix[i]] = 1;
                        h_idx[(size_t) s * mw + i] = ix[i];
                }
                if (ret == ISAL_HIP_OK &&
                    (isal_hip_obj_ptr_row(hp, old_data + (size_t) s * mw, (size_t) c) != ISAL_HIP_OK ||
                     isal_hip_obj_ptr_row(hp + mw, new_data + (size_t) s * mw, (size_t) c) != ISAL_HIP_OK ||
                     isal_hip_obj_ptr_row(hp + 2 * mw, coding + (size_t) s * rows, (size_t) rows) != ISAL_HIP_OK))
                        ret = ISAL_HIP_EINVAL;
                if (ret == ISAL_HIP_OK)
                        ret = ranges_apart(live, live_row(live, hp, mw, (size_t) c, (size_t) rows), (size_t) ln, sorted);
                if (ret == ISAL_HIP_OK && ragged)
                        h_lens[s] = c ? ln : 0;
                if (ret != ISAL_HIP_OK && bad_stripe)
                        *bad_stripe = (int) s;
        }
        /* one launch covers every item (the only tile size here is 2 KiB) */
        if (ret == ISAL_HIP_OK && ragged &&
            (n = isal_hip_ragged_items(nstripes, h_lens, ISAL_HIP_RAGGED_TILE_SMALL, NULL)) >
                    (long long) ISAL_HIP_RAGGED_MAX_ITEMS)
                ret = ISAL_HIP_EINVAL;
        if (ret != ISAL_HIP_OK)
                goto done;

        /* 3: the encode matrix's device tables, as a batch builds them; the
         * ragged kind's item table at the upload */
        h_tbl = (uint32_t *) malloc(isal_hip_tables_dwords(k, rows) * 4 + 4);
        o = (isal_hip_overwrite *) calloc(1, sizeof(*o));
        if (!h_tbl || !o) {
                ret = ISAL_HIP_ENOMEM;
                goto done;
        }
        isal_hip_build_tables(k, rows, gftbls, h_tbl);
        o->ragged = ragged;
        o->nitems = (unsigned) n;
        o->len = len;
        o->k = k;
        o->rows = rows;
        o->nw = nw;
        o->nstripes = nstripes;
        ret = overwrite_upload(o, h_ptrs, h_idx, h_tbl, h_lens, nws, live);
done:
        free(h_ptrs);
        free(live);
        free(sorted);
        free(h_idx);
        free(h_tbl);
        free(h_lens);
        if (ret != ISAL_HIP_OK) {
                isal_hip_overwrite_destroy(o);
                return ret;
        }
        *out = o;
        return ISAL_HIP_OK;
}

int
isal_hip_overwrite_create(isal_hip_overwrite **out, int len, int k, int rows, const unsigned char *gftbls,
                          int nw, int nstripes, const unsigned char *idx, unsigned char *const *old_data,
                          unsigned char *const *new_data, unsigned char *const *coding, int *bad_stripe)
{
        return overwrite_create(out, 0, len, NULL, k, rows, gftbls, nw, NULL, nstripes, idx, old_data, new_data, coding,
                                bad_stripe);
}

int
isal_hip_overwrite_create_ragged(isal_hip_overwrite **out, int k, int rows, const unsigned char *gftbls,
                                 int nstripes, const int *lens, int max_nw, const int *nw, const unsigned char *idx,
                                 unsigned char *const *old_data, unsigned char *const *new_data,
                                 unsigned char *const *coding, int *bad_stripe)
{
        return overwrite_create(out, 1, 0, lens, k, rows, gftbls, max_nw, nw, nstripes, idx, old_data, new_data, coding,
                                bad_stripe);
}

static int
overwrite_run_impl(isal_hip_overwrite *o, int flags, void *stream)
{
        if (o->ragged)
                return isal_hip_launch_overwrite_ragged(o->d_ptrs, 2 * o->nw + o->rows, o->d_idx, o->d_tbl, o->d_lens,
                                                        o->d_nw, o->d_items, o->nitems, o->k, o->rows, o->nw,
                                                        (flags & ISAL_HIP_OVERWRITE_COMMIT) != 0, stream)
                               ? ISAL_HIP_EHIP
                               : ISAL_HIP_OK;
        return isal_hip_launch_overwrite(o->d_ptrs, 2 * o->nw + o->rows, o->d_idx, o->d_tbl, o->len, o->k, o->rows,
                                         o->nw, o->nstripes, (flags & ISAL_HIP_OVERWRITE_COMMIT) != 0, stream)
                       ? ISAL_HIP_EHIP
                       : ISAL_HIP_OK;
}

int
isal_hip_overwrite_run(isal_hip_overwrite *o, int flags, void *stream)
{
        if (flags & ~ISAL_HIP_OVERWRITE_COMMIT)
                return ISAL_HIP_EINVAL;
        ON_BATCH_DEVICE(o, overwrite_run_impl(o, flags, stream));
}

int
isal_hip_overwrite_destroy(isal_hip_overwrite *o)
{
        if (!o)
                return ISAL_HIP_OK;
        isal_hip_obj_drop(o->d_ptrs);
        isal_hip_obj_drop(o->d_idx);
        isal_hip_obj_drop(o->d_tbl);
        isal_hip_obj_drop(o->d_lens);
        isal_hip_obj_drop(o->d_nw);
        isal_hip_obj_drop(o->d_items);
        free(o);
        return ISAL_HIP_OK;
}
