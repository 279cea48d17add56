/*
 * isal_hip_ragged.c — the ragged batch (isal_hip.h): nstripes stripes of one
 * geometry, each with its OWN shard length, encoded or checked by one kernel
 * launch per pass of up to EC_MAX_ROWS_PER_PASS rows.
 *
 * With one length per batch a work item is (w / tiles, w % tiles). Here it is
 * row w of an item table {stripe, tile}: the tiles of stripe 0, then of stripe
 * 1, ... (isal_hip_ragged_items, the one function that builds them); a stripe
 * of length 0 has no item. A pass's tile size depends on its row count
 * (ISAL_HIP_RAGGED_TILE*, isal_hip_internal.h), so an object holds one table
 * per tile size its passes use.
 *
 * Host side, in this order (everything before the first HIP call is pure
 * arithmetic and returns the same codes on a host without a GPU):
 *   1. counts, then per stripe its length (>= 0) and every shard pointer
 *      (non-NULL, 16-byte aligned) while the pointer table (per stripe k
 *      sources then rows parity rows) is written;
 *   2. the item count at the smallest tile against the launch limit;
 *   3. gftbls becomes the encode's device coefficient tables; the item tables
 *      are built.
 * A ragged batch belongs to the device that was current when it was created
 * (ON_BATCH_DEVICE).
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "erasure_code.h"
#include "isal_hip.h"
#include "isal_hip_internal.h"

#define MAX_SHARDS 256 /* shard indices are bytes */

enum { BIG, SMALL, NTABLES }; /* ISAL_HIP_RAGGED_TILE, ISAL_HIP_RAGGED_TILE_SMALL */

struct isal_hip_ragged {
        int k, rows, nstripes, device;
        unsigned nitems[NTABLES];
        uint64_t *d_ptrs;
        uint32_t *d_tbl;
        int *d_lens;
        unsigned *d_items[NTABLES];
};

long long
isal_hip_ragged_items(int nstripes, const int *lens, int tile, unsigned *items)
{
        long long n = 0;
        int s;
        if (!lens || nstripes <= 0 || tile <= 0)
                return -1;
        for (s = 0; s < nstripes; s++)
                if (lens[s] < 0)
                        return -1;
        for (s = 0; s < nstripes; s++) {
                const long long tiles = ((long long) lens[s] + tile - 1) / tile;
                long long t;
                for (t = 0; items && t < tiles; t++) {
                        items[2 * (n + t)] = (unsigned) s;
                        items[2 * (n + t) + 1] = (unsigned) t;
                }
                n += tiles;
        }
        return n;
}

/* whether some encode pass of rows parity rows runs the small tiles */
static int
uses_small_tiles(int rows)
{
        const int last = rows % EC_MAX_ROWS_PER_PASS;
        return last >= 1 && last <= ISAL_HIP_RAGGED_SMALL_ROWS;
}

static int
ragged_upload(isal_hip_ragged *r, const uint64_t *h_ptrs, const uint32_t *h_tbl, const int *lens,
              unsigned *const h_items[NTABLES])
{
        const size_t stride = (size_t) (r->k + r->rows);
        const size_t nptr = (size_t) r->nstripes * stride;
        const size_t ntbl = isal_hip_tables_dwords(r->k, r->rows) * 4;
        int s, t, e;
        if (hipGetDevice(&r->device) != hipSuccess)
                return ISAL_HIP_EHIP;
        /* a stripe's shards are as long as that stripe */
        for (s = 0; s < r->nstripes; s++)
                if (lens[s] > 0 && (e = isal_hip_batch_check_ptrs(h_ptrs + (size_t) s * stride, stride, (size_t) lens[s],
                                                                  r->device)) != ISAL_HIP_OK)
                        return e;
        if (hipMalloc((void **) &r->d_ptrs, nptr * 8) != hipSuccess ||
            hipMalloc((void **) &r->d_tbl, ntbl) != hipSuccess ||
            hipMalloc((void **) &r->d_lens, (size_t) r->nstripes * sizeof(int)) != hipSuccess)
                return ISAL_HIP_ENOMEM;
        if (hipMemcpy(r->d_ptrs, h_ptrs, nptr * 8, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(r->d_tbl, h_tbl, ntbl, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(r->d_lens, lens, (size_t) r->nstripes * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
                return ISAL_HIP_EHIP;
        for (t = 0; t < NTABLES; t++) {
                const size_t n = (size_t) r->nitems[t] * 8;
                if (!n)
                        continue;
                if (hipMalloc((void **) &r->d_items[t], n) != hipSuccess)
                        return ISAL_HIP_ENOMEM;
                if (hipMemcpy(r->d_items[t], h_items[t], n, hipMemcpyHostToDevice) != hipSuccess)
                        return ISAL_HIP_EHIP;
        }
        return ISAL_HIP_OK;
}

int
isal_hip_ragged_create(isal_hip_ragged **out, int k, int rows, const unsigned char *gftbls, int nstripes,
                       const int *lens, unsigned char *const *data, unsigned char *const *coding, int *bad_stripe)
{
        static const int tile[NTABLES] = { ISAL_HIP_RAGGED_TILE, ISAL_HIP_RAGGED_TILE_SMALL };
        isal_hip_ragged *r = NULL;
        uint64_t *h_ptrs = NULL;
        uint32_t *h_tbl = NULL;
        unsigned *h_items[NTABLES] = { NULL, NULL };
        long long s, n;
        int i, t, ret = ISAL_HIP_OK;
        size_t stride;

        if (bad_stripe)
                *bad_stripe = -1;
        if (!out)
                return ISAL_HIP_EINVAL;
        *out = NULL;
        if (k < 1 || rows < 1 || k + rows > MAX_SHARDS || !gftbls || nstripes < 1 || !lens || !data || !coding)
                return ISAL_HIP_EINVAL;
        stride = (size_t) k + (size_t) rows;

        h_ptrs = (uint64_t *) malloc((size_t) nstripes * stride * 8);
        if (!h_ptrs)
                return ISAL_HIP_ENOMEM;
        /* 1: every stripe's length and pointers while its table row is written */
        for (s = 0; s < nstripes && ret == ISAL_HIP_OK; s++) {
                uint64_t *hp = h_ptrs + (size_t) s * stride;
                for (i = 0; i < k; i++)
                        hp[i] = (uint64_t) (uintptr_t) data[(size_t) s * k + i];
                for (i = 0; i < rows; i++)
                        hp[k + i] = (uint64_t) (uintptr_t) coding[(size_t) s * rows + i];
                if (lens[s] < 0)
                        ret = ISAL_HIP_EINVAL;
                for (i = 0; i < (int) stride; i++)
                        if (!hp[i] || (hp[i] & 15))
                                ret = ISAL_HIP_EINVAL;
                if (ret != ISAL_HIP_OK && bad_stripe)
                        *bad_stripe = (int) s;
        }
        /* 2: one launch covers every item; a batch past the limit cannot exist
         * in one GPU's memory, so it is refused, not sliced */
        if (ret == ISAL_HIP_OK &&
            isal_hip_ragged_items(nstripes, lens, ISAL_HIP_RAGGED_TILE_SMALL, NULL) > (long long) ISAL_HIP_RAGGED_MAX_ITEMS)
                ret = ISAL_HIP_EINVAL;
        if (ret != ISAL_HIP_OK)
                goto done;

        /* 3: the encode's tables, one item table per tile size in use */
        h_tbl = (uint32_t *) malloc(isal_hip_tables_dwords(k, rows) * 4);
        r = (isal_hip_ragged *) calloc(1, sizeof(*r));
        if (!h_tbl || !r) {
                ret = ISAL_HIP_ENOMEM;
                goto done;
        }
        isal_hip_build_tables(k, rows, gftbls, h_tbl);
        r->k = k;
        r->rows = rows;
        r->nstripes = nstripes;
        for (t = 0; t < NTABLES; t++) {
                if (t == SMALL && !uses_small_tiles(rows))
                        continue;
                n = isal_hip_ragged_items(nstripes, lens, tile[t], NULL);
                r->nitems[t] = (unsigned) n;
                if (!n)
                        continue;
                h_items[t] = (unsigned *) malloc((size_t) n * 8);
                if (!h_items[t]) {
                        ret = ISAL_HIP_ENOMEM;
                        goto done;
                }
                (void) isal_hip_ragged_items(nstripes, lens, tile[t], h_items[t]);
        }
        ret = ragged_upload(r, h_ptrs, h_tbl, lens, h_items);
done:
        free(h_ptrs);
        free(h_tbl);
        for (t = 0; t < NTABLES; t++)
                free(h_items[t]);
        if (ret != ISAL_HIP_OK) {
                isal_hip_ragged_destroy(r);
                return ret;
        }
        *out = r;
        return ISAL_HIP_OK;
}

static int
ragged_encode_impl(isal_hip_ragged *r, void *stream)
{
        return isal_hip_launch_encode_ragged(r->d_ptrs, r->k + r->rows, r->d_tbl, r->d_lens, r->d_items[BIG],
                                             r->nitems[BIG], r->d_items[SMALL], r->nitems[SMALL], r->k, r->rows,
                                             stream)
                       ? ISAL_HIP_EHIP
                       : ISAL_HIP_OK;
}

int
isal_hip_ragged_encode(isal_hip_ragged *r, void *stream)
{
        ON_BATCH_DEVICE(r, ragged_encode_impl(r, stream));
}

static int
ragged_check_impl(isal_hip_ragged *r, unsigned long long *bad, void *stream)
{
        return isal_hip_launch_verify_ragged(r->d_ptrs, r->k + r->rows, r->d_tbl, r->d_lens, r->d_items[BIG],
                                             r->nitems[BIG], r->k, r->rows, r->nstripes, bad, stream)
                       ? ISAL_HIP_EHIP
                       : ISAL_HIP_OK;
}

int
isal_hip_ragged_check(isal_hip_ragged *r, unsigned long long *bad, void *stream)
{
        if (!bad)
                return ISAL_HIP_EINVAL;
        ON_BATCH_DEVICE(r, ragged_check_impl(r, bad, stream));
}

int
isal_hip_ragged_destroy(isal_hip_ragged *r)
{
        int t;
        if (!r)
                return ISAL_HIP_OK;
        if (r->d_ptrs)
                (void) hipFree(r->d_ptrs);
        if (r->d_tbl)
                (void) hipFree(r->d_tbl);
        if (r->d_lens)
                (void) hipFree(r->d_lens);
        for (t = 0; t < NTABLES; t++)
                if (r->d_items[t])
                        (void) hipFree(r->d_items[t]);
        free(r);
        return ISAL_HIP_OK;
}
