/*
 * isal_hip_overwrite.c — the overwrite batch (isal_hip.h): nstripes encoded
 * stripes of one geometry, each with its own set of nw rewritten data shards,
 * whose deltas (old ^ new) are folded into the parity by one kernel launch
 * per pass of up to EC_MAX_ROWS_PER_PASS rows.
 *
 * Host side, in this order (everything before the first HIP call is pure
 * arithmetic and returns the same codes on a host without a GPU):
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
 * The ragged overwrite (isal_hip_overwrite_create_ragged) is the same object
 * where stripe s has its own length lens[s] and its own count nw[s] of the
 * max_nw slots a table row holds. Step 1 looks at a stripe's live slots only
 * (the first nw[s] of its row) and compares their ranges over lens[s]; step 2
 * writes the tables at stride max_nw with the other slots zeroed; the upload
 * adds the lengths, the counts and the work-item table of the ragged batch
 * (isal_hip_ragged_items at the 2 KiB tile, where a stripe without a slot
 * counts as empty). Its run is one ec_overwrite_rag launch per pass over that
 * table, whatever the mix of lengths and counts.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "isal_hip.h"
#include "isal_hip_internal.h"

#define MAX_SHARDS 256 /* shard indices are bytes */

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

/* tests/sanitize/overwrite_host.c links this file without the ragged pieces */
#pragma weak isal_hip_ragged_items
#pragma weak isal_hip_launch_overwrite_ragged

static int
cmp_u64(const void *a, const void *b)
{
        const uint64_t x = *(const uint64_t *) a, y = *(const uint64_t *) b;
        return x < y ? -1 : x > y;
}

/* One stripe's row of the pointer table (n entries): every pointer set and
 * 16-byte aligned, no two [p, p + len) ranges overlapping. sorted: scratch. */
static int
check_row(const uint64_t *row, size_t n, size_t len, uint64_t *sorted)
{
        size_t i;
        for (i = 0; i < n; i++)
                if (!row[i] || (row[i] & 15))
                        return ISAL_HIP_EINVAL;
        if (!len)
                return ISAL_HIP_OK;
        memcpy(sorted, row, n * 8);
        qsort(sorted, n, 8, cmp_u64);
        for (i = 1; i < n; i++)
                if (sorted[i] - sorted[i - 1] < len)
                        return ISAL_HIP_EINVAL;
        return ISAL_HIP_OK;
}

static int
overwrite_upload(isal_hip_overwrite *o, const uint64_t *h_ptrs, const uint32_t *h_idx, const uint32_t *h_tbl)
{
        const size_t nptr = (size_t) o->nstripes * (size_t) (2 * o->nw + o->rows);
        const size_t nidx = (size_t) o->nstripes * (size_t) o->nw;
        const size_t ntbl = isal_hip_tables_dwords(o->k, o->rows) * 4;
        int e;
        if (hipGetDevice(&o->device) != hipSuccess)
                return ISAL_HIP_EHIP;
        if (o->len > 0 &&
            (e = isal_hip_batch_check_ptrs(h_ptrs, nptr, (size_t) o->len, o->device)) != ISAL_HIP_OK)
                return e;
        if (hipMalloc((void **) &o->d_ptrs, nptr * 8) != hipSuccess ||
            hipMalloc((void **) &o->d_idx, nidx * 4) != hipSuccess ||
            hipMalloc((void **) &o->d_tbl, ntbl + 4) != hipSuccess)
                return ISAL_HIP_ENOMEM;
        if (hipMemcpy(o->d_ptrs, h_ptrs, nptr * 8, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(o->d_idx, h_idx, nidx * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(o->d_tbl, h_tbl, ntbl, hipMemcpyHostToDevice) != hipSuccess)
                return ISAL_HIP_EHIP;
        return ISAL_HIP_OK;
}

int
isal_hip_overwrite_create(isal_hip_overwrite **out, int len, int k, int rows, const unsigned char *gftbls,
                          int nw, int nstripes, const unsigned char *idx, unsigned char *const *old_data,
                          unsigned char *const *new_data, unsigned char *const *coding, int *bad_stripe)
{
        isal_hip_overwrite *o = NULL;
        unsigned char mark[MAX_SHARDS];
        uint64_t *h_ptrs = NULL, *sorted = NULL;
        uint32_t *h_idx = NULL, *h_tbl = NULL;
        long long s;
        int i, ret = ISAL_HIP_OK;
        size_t stride;

        if (bad_stripe)
                *bad_stripe = -1;
        if (!out)
                return ISAL_HIP_EINVAL;
        *out = NULL;
        if (len < 0 || k < 1 || k > MAX_SHARDS || rows < 1 || !gftbls || nw < 1 || nw > k || nstripes < 1 ||
            !idx || !old_data || !new_data || !coding)
                return ISAL_HIP_EINVAL;
        stride = 2 * (size_t) nw + (size_t) rows;

        h_ptrs = (uint64_t *) malloc((size_t) nstripes * stride * 8);
        sorted = (uint64_t *) malloc(stride * 8);
        h_idx = (uint32_t *) malloc((size_t) nstripes * (size_t) nw * 4);
        if (!h_ptrs || !sorted || !h_idx) {
                ret = ISAL_HIP_ENOMEM;
                goto done;
        }

        /* 1-2: validate every stripe while its table rows are written */
        for (s = 0; s < nstripes && ret == ISAL_HIP_OK; s++) {
                const unsigned char *ix = idx + (size_t) s * nw;
                uint64_t *hp = h_ptrs + (size_t) s * stride;
                memset(mark, 0, sizeof(mark));
                for (i = 0; i < nw && ret == ISAL_HIP_OK; i++) {
                        if (ix[i] >= k || mark[ix[i]])
                                ret = ISAL_HIP_EINVAL;
                        else
                                mark[ix[i]] = 1;
                        h_idx[(size_t) s * nw + i] = ix[i];
                }
                for (i = 0; i < nw; i++) {
                        hp[i] = (uint64_t) (uintptr_t) old_data[(size_t) s * nw + i];
                        hp[nw + i] = (uint64_t) (uintptr_t) new_data[(size_t) s * nw + i];
                }
                for (i = 0; i < rows; i++)
                        hp[2 * nw + i] = (uint64_t) (uintptr_t) coding[(size_t) s * rows + i];
                if (ret == ISAL_HIP_OK)
                        ret = check_row(hp, stride, (size_t) len, sorted);
                if (ret != ISAL_HIP_OK && bad_stripe)
                        *bad_stripe = (int) s;
        }
        if (ret != ISAL_HIP_OK)
                goto done;

        /* 3: the encode matrix's device tables, as a batch builds them */
        h_tbl = (uint32_t *) malloc(isal_hip_tables_dwords(k, rows) * 4 + 4);
        o = (isal_hip_overwrite *) calloc(1, sizeof(*o));
        if (!h_tbl || !o) {
                ret = ISAL_HIP_ENOMEM;
                goto done;
        }
        isal_hip_build_tables(k, rows, gftbls, h_tbl);
        o->len = len;
        o->k = k;
        o->rows = rows;
        o->nw = nw;
        o->nstripes = nstripes;
        ret = overwrite_upload(o, h_ptrs, h_idx, h_tbl);
done:
        free(h_ptrs);
        free(sorted);
        free(h_idx);
        free(h_tbl);
        if (ret != ISAL_HIP_OK) {
                isal_hip_overwrite_destroy(o);
                return ret;
        }
        *out = o;
        return ISAL_HIP_OK;
}

/* ---- the ragged create ---------------------------------------------------- */

/* lens: a stripe's own length, 0 where it has no slot; nws: the counts. The
 * item table (o->nitems rows) is built here, after the pointers have been
 * classified, as the ragged scrub does. */
static int
overwrite_upload_ragged(isal_hip_overwrite *o, const uint64_t *h_ptrs, const uint32_t *h_idx,
                        const uint32_t *h_tbl, const int *lens, const int *nws, uint64_t *live)
{
        unsigned *h_items;
        const size_t mw = (size_t) o->nw, stride = 2 * mw + (size_t) o->rows;
        const size_t nptr = (size_t) o->nstripes * stride;
        const size_t nidx = (size_t) o->nstripes * mw;
        const size_t ntbl = isal_hip_tables_dwords(o->k, o->rows) * 4;
        const size_t nlen = (size_t) o->nstripes * sizeof(int);
        int s, e;
        if (hipGetDevice(&o->device) != hipSuccess)
                return ISAL_HIP_EHIP;
        /* a stripe's live shards are as long as that stripe */
        for (s = 0; s < o->nstripes; s++) {
                const uint64_t *hp = h_ptrs + (size_t) s * stride;
                const size_t n = (size_t) nws[s];
                if (lens[s] <= 0)
                        continue;
                memcpy(live, hp, n * 8);
                memcpy(live + n, hp + mw, n * 8);
                memcpy(live + 2 * n, hp + 2 * mw, (size_t) o->rows * 8);
                if ((e = isal_hip_batch_check_ptrs(live, 2 * n + (size_t) o->rows, (size_t) lens[s], o->device)) !=
                    ISAL_HIP_OK)
                        return e;
        }
        if (hipMalloc((void **) &o->d_ptrs, nptr * 8) != hipSuccess ||
            hipMalloc((void **) &o->d_idx, nidx * 4) != hipSuccess ||
            hipMalloc((void **) &o->d_tbl, ntbl + 4) != hipSuccess ||
            hipMalloc((void **) &o->d_lens, nlen) != hipSuccess || hipMalloc((void **) &o->d_nw, nlen) != hipSuccess)
                return ISAL_HIP_ENOMEM;
        if (hipMemcpy(o->d_ptrs, h_ptrs, nptr * 8, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(o->d_idx, h_idx, nidx * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(o->d_tbl, h_tbl, ntbl, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(o->d_lens, lens, nlen, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(o->d_nw, nws, nlen, hipMemcpyHostToDevice) != hipSuccess)
                return ISAL_HIP_EHIP;
        if (!o->nitems)
                return ISAL_HIP_OK;
        h_items = (unsigned *) malloc((size_t) o->nitems * 8);
        if (!h_items || hipMalloc((void **) &o->d_items, (size_t) o->nitems * 8) != hipSuccess) {
                free(h_items);
                return ISAL_HIP_ENOMEM;
        }
        (void) isal_hip_ragged_items(o->nstripes, lens, ISAL_HIP_RAGGED_TILE_SMALL, h_items);
        e = hipMemcpy(o->d_items, h_items, (size_t) o->nitems * 8, hipMemcpyHostToDevice) != hipSuccess;
        free(h_items);
        return e ? ISAL_HIP_EHIP : ISAL_HIP_OK;
}

int
isal_hip_overwrite_create_ragged(isal_hip_overwrite **out, int k, int rows, const unsigned char *gftbls,
                                 int nstripes, const int *lens, int max_nw, const int *nw, const unsigned char *idx,
                                 unsigned char *const *old_data, unsigned char *const *new_data,
                                 unsigned char *const *coding, int *bad_stripe)
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
        if (k < 1 || k > MAX_SHARDS || rows < 1 || !gftbls || nstripes < 1 || !lens || max_nw < 1 || max_nw > k ||
            !nw || !idx || !old_data || !new_data || !coding)
                return ISAL_HIP_EINVAL;
        mw = (size_t) max_nw;
        stride = 2 * mw + (size_t) rows;

        /* calloc: the slots a stripe does not use stay zero in both tables */
        h_ptrs = (uint64_t *) calloc((size_t) nstripes * stride, 8);
        h_idx = (uint32_t *) calloc((size_t) nstripes * mw, 4);
        live = (uint64_t *) malloc(stride * 8);
        sorted = (uint64_t *) malloc(stride * 8);
        h_lens = (int *) malloc((size_t) nstripes * sizeof(int));
        if (!h_ptrs || !h_idx || !live || !sorted || !h_lens) {
                ret = ISAL_HIP_ENOMEM;
                goto done;
        }

        /* 1-2: validate every stripe's live slots while its table rows are
         * written: count and indices, then pointers, then overlaps */
        for (s = 0; s < nstripes && ret == ISAL_HIP_OK; s++) {
                const unsigned char *ix = idx + (size_t) s * mw;
                uint64_t *hp = h_ptrs + (size_t) s * stride;
                const int c = nw[s];
                if (lens[s] < 0 || c < 0 || c > max_nw) {
                        ret = ISAL_HIP_EINVAL;
                } else {
                        memset(mark, 0, sizeof(mark));
                        for (i = 0; i < c && ret == ISAL_HIP_OK; i++) {
                                if (ix[i] >= k || mark[ix[i]])
                                        ret = ISAL_HIP_EINVAL;
                                else
                                        mark[ix[i]] = 1;
                                h_idx[(size_t) s * mw + i] = ix[i];
                        }
                }
                if (ret == ISAL_HIP_OK) {
                        for (i = 0; i < c; i++) {
                                live[i] = hp[i] = (uint64_t) (uintptr_t) old_data[(size_t) s * mw + i];
                                live[c + i] = hp[mw + i] = (uint64_t) (uintptr_t) new_data[(size_t) s * mw + i];
                        }
                        for (i = 0; i < rows; i++)
                                live[2 * c + i] = hp[2 * mw + i] = (uint64_t) (uintptr_t) coding[(size_t) s * rows + i];
                        ret = check_row(live, 2 * (size_t) c + (size_t) rows, (size_t) lens[s], sorted);
                        h_lens[s] = c ? lens[s] : 0;
                }
                if (ret != ISAL_HIP_OK && bad_stripe)
                        *bad_stripe = (int) s;
        }
        /* one launch covers every item (the only tile size here is 2 KiB) */
        if (ret == ISAL_HIP_OK && (n = isal_hip_ragged_items(nstripes, h_lens, ISAL_HIP_RAGGED_TILE_SMALL, NULL)) >
                                          (long long) ISAL_HIP_RAGGED_MAX_ITEMS)
                ret = ISAL_HIP_EINVAL;
        if (ret != ISAL_HIP_OK)
                goto done;

        /* 3: the encode matrix's device tables; the item table at the upload */
        h_tbl = (uint32_t *) malloc(isal_hip_tables_dwords(k, rows) * 4 + 4);
        o = (isal_hip_overwrite *) calloc(1, sizeof(*o));
        if (!h_tbl || !o) {
                ret = ISAL_HIP_ENOMEM;
                goto done;
        }
        isal_hip_build_tables(k, rows, gftbls, h_tbl);
        o->ragged = 1;
        o->nitems = (unsigned) n;
        o->k = k;
        o->rows = rows;
        o->nw = max_nw;
        o->nstripes = nstripes;
        ret = overwrite_upload_ragged(o, h_ptrs, h_idx, h_tbl, h_lens, nw, live);
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
        if (o->d_ptrs)
                (void) hipFree(o->d_ptrs);
        if (o->d_idx)
                (void) hipFree(o->d_idx);
        if (o->d_tbl)
                (void) hipFree(o->d_tbl);
        if (o->d_lens)
                (void) hipFree(o->d_lens);
        if (o->d_nw)
                (void) hipFree(o->d_nw);
        if (o->d_items)
                (void) hipFree(o->d_items);
        free(o);
        return ISAL_HIP_OK;
}
