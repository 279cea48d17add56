/*
 * isal_hip_sector_crc.c — sector checksums (isal_hip.h isal_hip_batch_sector_crc,
 * isal_hip_batch_sector_crc64, isal_hip_ragged_sector_crc,
 * isal_hip_ragged_sector_crc64, isal_hip_ragged_sector_offsets): the CRC32C or
 * a crc64_* flavour of every `sector` bytes of every shard of a uniform or a
 * ragged batch, in one launch of crc_sector_kernels.hip's kernel and nothing
 * else: no combine, no partials.
 *
 * Every refusal is decided before the first HIP call, from what the objects
 * keep on the host. Nothing is built at create: the first call that needs a
 * flavour's image (isal_hip_internal.h "sector checksums"; a function of the
 * flavour alone) builds and uploads it, and the first ragged call with a sector
 * size uploads that size's table of first sectors; the objects' destroy frees
 * them.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>

#include "isal_hip.h"
#include "isal_hip_internal.h"

_Static_assert(sizeof(((isal_hip_ragged *) 0)->d_sec64) / sizeof(uint64_t *) == ISAL_HIP_CRC64_NVARIANTS,
               "one image slot per variant");
_Static_assert(sizeof(((isal_hip_ragged *) 0)->d_sec_first) / sizeof(unsigned long long *) == ISAL_HIP_SECTOR_NSIZES,
               "one table of first sectors per sector size");

/* index of a sector size among the ISAL_HIP_SECTOR_NSIZES allowed, or -1 */
int
isal_hip_sector_index(int sector)
{
        int i;
        for (i = 0; i < ISAL_HIP_SECTOR_NSIZES; i++)
                if (sector == ISAL_HIP_SECTOR_MIN << i)
                        return i;
        return -1;
}

long long
isal_hip_ragged_sector_offsets(int nstripes, const int *lens, int sector, long long *first)
{
        long long n = 0;
        int s;
        if (!lens || nstripes <= 0 || isal_hip_sector_index(sector) < 0)
                return -1;
        for (s = 0; s < nstripes; s++)
                if (lens[s] < 0)
                        return -1;
        for (s = 0; s < nstripes; s++) {
                if (first)
                        first[s] = n;
                n += ((long long) lens[s] + sector - 1) / sector;
        }
        return n;
}

/* *slot = the device copy of a freshly built image (the callers look first
 * whether it is there already). A failure leaves *slot NULL and no HIP error
 * behind. */
int
isal_hip_sector_put(void *slot, void *h, size_t bytes)
{
        void *d = NULL;
        int e;
        if (!h)
                return ISAL_HIP_ENOMEM;
        e = isal_hip_obj_put(&d, h, bytes, 0);
        free(h);
        if (e != ISAL_HIP_OK) {
                isal_hip_obj_drop(d);
                (void) hipGetLastError(); /* the object stays usable: no sticky error for the next call */
                return e;
        }
        *(void **) slot = d; /* published only once filled */
        return ISAL_HIP_OK;
}

static int
sector_image32(uint32_t **slot)
{
        uint32_t *h;
        if (*slot)
                return ISAL_HIP_OK;
        h = (uint32_t *) malloc((size_t) ISAL_HIP_SECTOR32_DWORDS * 4);
        if (h)
                isal_hip_crc32c_sector_image(h);
        return isal_hip_sector_put(slot, h, (size_t) ISAL_HIP_SECTOR32_DWORDS * 4);
}

static int
sector_image64(uint64_t **slot, int variant)
{
        uint64_t *h;
        if (*slot)
                return ISAL_HIP_OK;
        h = (uint64_t *) malloc((size_t) ISAL_HIP_SECTOR64_ENTRIES * 8);
        if (h)
                isal_hip_crc64_sector_image(variant, h);
        return isal_hip_sector_put(slot, h, (size_t) ISAL_HIP_SECTOR64_ENTRIES * 8);
}

/* variant < 0: CRC32C */
static int
sector_launch(const isal_hip_sector_geom *g, int variant, const uint32_t *d32, const uint64_t *d64,
              unsigned long long init, void *crc, void *stream)
{
        const int e = variant < 0 ? isal_hip_launch_sector_crc32c(g, d32, (unsigned int) init, (uint32_t *) crc, stream)
                                  : isal_hip_launch_sector_crc64(g, d64, isal_hip_crc64_is_refl(variant),
                                                                 isal_hip_crc64_ring_poly(variant), (uint64_t) init,
                                                                 (uint64_t *) crc, stream);
        return e ? ISAL_HIP_EHIP : ISAL_HIP_OK;
}

/* ---- the uniform batch ------------------------------------------------------ */

static unsigned long long
batch_tiles(const isal_hip_batch *b)
{
        return ((unsigned long long) b->len + ISAL_HIP_CRC_TILE - 1) / ISAL_HIP_CRC_TILE;
}

static int
batch_sector_impl(isal_hip_batch *b, const isal_hip_sector_geom *g, int variant, unsigned long long init, void *crc,
                  void *stream)
{
        const int e = variant < 0 ? sector_image32(&b->d_sec32) : sector_image64(&b->d_sec64[variant], variant);
        if (e != ISAL_HIP_OK)
                return e;
        return sector_launch(g, variant, b->d_sec32, variant < 0 ? NULL : b->d_sec64[variant], init, crc, stream);
}

/* what every uniform entry point refuses, before any HIP call; 1: nothing to do */
int
isal_hip_sector_batch_geom(const isal_hip_batch *b, int sector, isal_hip_sector_geom *g)
{
        if (!b || isal_hip_sector_index(sector) < 0 || !b->vec16)
                return ISAL_HIP_EINVAL;
        g->d_ptrs = b->d_ptrs;
        g->nsh = b->k + b->rows;
        g->sector = sector;
        g->len = b->len;
        g->ntiles = (unsigned) batch_tiles(b);
        g->nwork = (unsigned long long) b->nstripes * (unsigned long long) g->nsh * batch_tiles(b);
        if (g->nwork > (unsigned long long) ISAL_HIP_RAGGED_MAX_ITEMS)
                return ISAL_HIP_EINVAL;
        return b->len == 0;
}

int
isal_hip_batch_sector_crc(isal_hip_batch *b, int sector, unsigned int init, unsigned int *crc, void *stream)
{
        isal_hip_sector_geom g = { 0 };
        const int e = crc ? isal_hip_sector_batch_geom(b, sector, &g) : ISAL_HIP_EINVAL;
        if (e)
                return e < 0 ? e : ISAL_HIP_OK;
        ON_BATCH_DEVICE(b, batch_sector_impl(b, &g, -1, init, crc, stream));
}

int
isal_hip_batch_sector_crc64(isal_hip_batch *b, int variant, int sector, unsigned long long init,
                            unsigned long long *crc, void *stream)
{
        isal_hip_sector_geom g = { 0 };
        int e;
        if (variant < 0 || variant >= ISAL_HIP_CRC64_NVARIANTS || !crc)
                return ISAL_HIP_EINVAL;
        if ((e = isal_hip_sector_batch_geom(b, sector, &g)) != 0)
                return e < 0 ? e : ISAL_HIP_OK;
        ON_BATCH_DEVICE(b, batch_sector_impl(b, &g, variant, init, crc, stream));
}

/* ---- the ragged batch ------------------------------------------------------- */

/* first[s] of isal_hip_ragged_sector_offsets for this sector size, on the device */
int
isal_hip_sector_ragged_first(isal_hip_ragged *r, int sector, isal_hip_sector_geom *g)
{
        unsigned long long **slot = &r->d_sec_first[isal_hip_sector_index(sector)];
        if (!*slot) {
                long long *h = (long long *) malloc((size_t) r->nstripes * sizeof(long long));
                int e;
                if (h)
                        (void) isal_hip_ragged_sector_offsets(r->nstripes, r->h_lens, sector, h);
                if ((e = isal_hip_sector_put(slot, h, (size_t) r->nstripes * sizeof(long long))) != ISAL_HIP_OK)
                        return e;
        }
        g->d_first = *slot;
        return ISAL_HIP_OK;
}

static int
ragged_sector_impl(isal_hip_ragged *r, isal_hip_sector_geom *g, int variant, unsigned long long init, void *crc,
                   void *stream)
{
        int e;
        if ((e = isal_hip_sector_ragged_first(r, g->sector, g)) != ISAL_HIP_OK ||
            (e = variant < 0 ? sector_image32(&r->d_sec32) : sector_image64(&r->d_sec64[variant], variant)) != ISAL_HIP_OK)
                return e;
        return sector_launch(g, variant, r->d_sec32, variant < 0 ? NULL : r->d_sec64[variant], init, crc, stream);
}

int
isal_hip_sector_ragged_geom(const isal_hip_ragged *r, int sector, isal_hip_sector_geom *g)
{
        if (!r || isal_hip_sector_index(sector) < 0)
                return ISAL_HIP_EINVAL;
        g->d_ptrs = r->d_ptrs;
        g->nsh = r->k + r->rows;
        g->sector = sector;
        g->d_lens = r->d_lens;
        g->d_items = r->d_items[TILE_BIG]; /* the encode's 4 KiB {stripe, tile} table */
        g->nwork = (unsigned long long) r->nitems[TILE_BIG] * (unsigned long long) g->nsh;
        if (g->nwork > (unsigned long long) ISAL_HIP_RAGGED_MAX_ITEMS)
                return ISAL_HIP_EINVAL;
        return r->nitems[TILE_BIG] == 0; /* every length is 0 */
}

int
isal_hip_ragged_sector_crc(isal_hip_ragged *r, int sector, unsigned int init, unsigned int *crc, void *stream)
{
        isal_hip_sector_geom g = { 0 };
        const int e = crc ? isal_hip_sector_ragged_geom(r, sector, &g) : ISAL_HIP_EINVAL;
        if (e)
                return e < 0 ? e : ISAL_HIP_OK;
        ON_BATCH_DEVICE(r, ragged_sector_impl(r, &g, -1, init, crc, stream));
}

int
isal_hip_ragged_sector_crc64(isal_hip_ragged *r, int variant, int sector, unsigned long long init,
                             unsigned long long *crc, void *stream)
{
        isal_hip_sector_geom g = { 0 };
        int e;
        if (variant < 0 || variant >= ISAL_HIP_CRC64_NVARIANTS || !crc)
                return ISAL_HIP_EINVAL;
        if ((e = isal_hip_sector_ragged_geom(r, sector, &g)) != 0)
                return e < 0 ? e : ISAL_HIP_OK;
        ON_BATCH_DEVICE(r, ragged_sector_impl(r, &g, variant, init, crc, stream));
}
