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
 * arithmetic and returns the same codes on a host without a GPU; the steps
 * every stripe object shares are isal_hip_objects.c's):
 *   1. counts, then per stripe its length (>= 0) and every shard pointer
 *      (non-NULL, 16-byte aligned) while the pointer table (per stripe k
 *      sources then rows parity rows) is written;
 *   2. the item count at the smallest tile against the launch limit;
 *   3. gftbls becomes the encode's device coefficient tables; the item tables
 *      are built at the upload, once the shards are known to be reachable.
 * A ragged batch belongs to the device that was current when it was created
 * (ON_BATCH_DEVICE). The object's layout is in isal_hip_internal.h: its
 * fragment checksums are isal_hip_ragged_crc.c's, which builds what it needs
 * at the first checksum call from the lengths create keeps (h_lens).
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "erasure_code.h"
#include "isal_hip.h"
#include "isal_hip_internal.h"

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

/* The item tables (r->nitems[] rows) are built here, after the pointers have
 * been classified, as every ragged object does. */
static int
ragged_upload(isal_hip_ragged *r, const uint64_t *h_ptrs, const uint32_t *h_tbl, const int *lens)
{
        const size_t stride = (size_t) (r->k + r->rows), nstripes = (size_t) r->nstripes;
        int t, e;
        if (hipGetDevice(&r->device) != hipSuccess)
                return ISAL_HIP_EHIP;
        if ((e = isal_hip_obj_reach(h_ptrs, nstripes, stride, 0, lens, r->device)) != ISAL_HIP_OK ||
            (e = isal_hip_obj_put(&r->d_ptrs, h_ptrs, nstripes * stride * 8, 0)) != ISAL_HIP_OK ||
            (e = isal_hip_obj_put(&r->d_tbl, h_tbl, isal_hip_tables_dwords(r->k, r->rows) * 4, 0)) != ISAL_HIP_OK ||
            (e = isal_hip_obj_put(&r->d_lens, lens, nstripes * sizeof(int), 0)) != ISAL_HIP_OK)
                return e;
        for (t = 0; t < NTILES && e == ISAL_HIP_OK; t++)
                e = isal_hip_obj_put_items(&r->d_items[t], r->nstripes, lens, isal_hip_tile_bytes(t), r->nitems[t]);
        return e;
}

int
isal_hip_ragged_create(isal_hip_ragged **out, int k, int rows, const unsigned char *gftbls, int nstripes,
                       const int *lens, unsigned char *const *data, unsigned char *const *coding, int *bad_stripe)
{
        isal_hip_ragged *r = NULL;
        uint64_t *h_ptrs = NULL;
        uint32_t *h_tbl = NULL;
        long long s;
        int t, ret = ISAL_HIP_OK;
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
                if (isal_hip_obj_ptr_row(hp, data + (size_t) s * k, (size_t) k) != ISAL_HIP_OK ||
                    isal_hip_obj_ptr_row(hp + k, coding + (size_t) s * rows, (size_t) rows) != ISAL_HIP_OK || lens[s] < 0)
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

        /* 3: the encode's tables, one item table per tile size in use (built
         * at the upload) */
        h_tbl = (uint32_t *) malloc(isal_hip_tables_dwords(k, rows) * 4);
        r = (isal_hip_ragged *) calloc(1, sizeof(*r));
        if (r)
                r->h_lens = (int *) malloc((size_t) nstripes * sizeof(int));
        if (!h_tbl || !r || !r->h_lens) {
                ret = ISAL_HIP_ENOMEM;
                goto done;
        }
        memcpy(r->h_lens, lens, (size_t) nstripes * sizeof(int));
        isal_hip_build_tables(k, rows, gftbls, h_tbl);
        r->k = k;
        r->rows = rows;
        r->nstripes = nstripes;
        for (t = 0; t < NTILES; t++)
                if (t == TILE_BIG || isal_hip_uses_small_tile(rows))
                        r->nitems[t] = (unsigned) isal_hip_ragged_items(nstripes, lens, isal_hip_tile_bytes(t), NULL);
        ret = ragged_upload(r, h_ptrs, h_tbl, lens);
done:
        free(h_ptrs);
        free(h_tbl);
        if (ret != ISAL_HIP_OK) {
                isal_hip_ragged_destroy(r);
                return ret;
        }
        *out = r;
        return ISAL_HIP_OK;
}

int
isal_hip_ragged_encode_on_device(isal_hip_ragged *r, void *stream)
{
        return isal_hip_launch_encode_ragged(r->d_ptrs, r->k + r->rows, r->d_tbl, r->d_lens, r->d_items[TILE_BIG],
                                             r->nitems[TILE_BIG], r->d_items[TILE_SMALL], r->nitems[TILE_SMALL],
                                             r->k, r->rows, stream)
                       ? ISAL_HIP_EHIP
                       : ISAL_HIP_OK;
}

int
isal_hip_ragged_encode(isal_hip_ragged *r, void *stream)
{
        ON_BATCH_DEVICE(r, isal_hip_ragged_encode_on_device(r, stream));
}

static int
ragged_check_impl(isal_hip_ragged *r, unsigned long long *bad, void *stream)
{
        return isal_hip_launch_verify_ragged(r->d_ptrs, r->k + r->rows, r->d_tbl, r->d_lens, r->d_items[TILE_BIG],
                                             r->nitems[TILE_BIG], r->k, r->rows, r->nstripes, bad, stream)
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

/* Frees one width's checksum state (isal_hip_ragged_crc.c builds it, and
 * rolls a failed set-up back with this) and leaves it as create did. */
void
isal_hip_ragged_ck_drop(isal_hip_ragged_ck *ck)
{
        isal_hip_obj_drop(ck->d_part);
        isal_hip_obj_drop(ck->d_items);
        isal_hip_obj_drop(ck->d_first);
        memset(ck, 0, sizeof(*ck));
}

int
isal_hip_ragged_destroy(isal_hip_ragged *r)
{
        int t;
        if (!r)
                return ISAL_HIP_OK;
        /* what the first checksum calls of either width allocated
         * (isal_hip_ragged_crc.c) */
        isal_hip_obj_drop(r->d_crc);
        isal_hip_ragged_ck_drop(&r->ck32);
        isal_hip_ragged_ck_drop(&r->ck64);
        for (t = 0; t < (int) (sizeof(r->d_c64image) / sizeof(r->d_c64image[0])); t++)
                isal_hip_obj_drop(r->d_c64image[t]);
        /* ... and the sector checksums (isal_hip_sector_crc.c) */
        isal_hip_obj_drop(r->d_sec32);
        for (t = 0; t < (int) (sizeof(r->d_sec64) / sizeof(r->d_sec64[0])); t++)
                isal_hip_obj_drop(r->d_sec64[t]);
        for (t = 0; t < ISAL_HIP_SECTOR_NSIZES; t++)
                isal_hip_obj_drop(r->d_sec_first[t]);
        isal_hip_obj_drop(r->d_sec16); /* ... and the T10 guard's (isal_hip_dif.c) */
        free(r->h_lens);
        isal_hip_obj_drop(r->d_ptrs);
        isal_hip_obj_drop(r->d_tbl);
        isal_hip_obj_drop(r->d_lens);
        for (t = 0; t < NTILES; t++)
                isal_hip_obj_drop(r->d_items[t]);
        free(r);
        return ISAL_HIP_OK;
}
