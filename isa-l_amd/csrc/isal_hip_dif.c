/*
 * isal_hip_dif.c — T10 protection information per sector (isal_hip.h
 * isal_hip_batch_sector_t10dif, isal_hip_batch_dif_generate,
 * isal_hip_batch_dif_verify and their ragged forms): the 16-bit guard
 * crc16_t10dif of every `sector` bytes of every shard, stored as a word, stored
 * as the 8-byte tuple with its tags, or compared on the device with a stored
 * tuple. One launch of the sector pass (crc_sector_kernels.hip, family
 * Crc16T10), behind a fill of `bad` for verify; nothing else.
 *
 * The geometry, the refusals it implies and the table of first sectors are the
 * sector checksums' (isal_hip_sector_crc.c). Every refusal is decided before
 * the first HIP call. The guard's image (crc16_host.c; 7 KiB, a function of
 * the polynomial alone) is built and uploaded by the first call; the objects'
 * destroy frees it.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>

#include "isal_hip.h"
#include "isal_hip_internal.h"

static int
dif_image(uint32_t **slot)
{
        uint32_t *h;
        if (*slot)
                return ISAL_HIP_OK;
        h = (uint32_t *) malloc((size_t) ISAL_HIP_SECTOR16_DWORDS * 4);
        if (h)
                isal_hip_crc16_sector_image(h);
        return isal_hip_sector_put(slot, h, (size_t) ISAL_HIP_SECTOR16_DWORDS * 4);
}

/* The launch's arguments from the caller's; ISAL_HIP_EINVAL for what no object
 * can make valid. d is NULL for the guard words (seed then counts). */
static int
dif_args(isal_hip_dif_args *a, int mode, const isal_hip_dif *d, unsigned short seed, const void *out,
         unsigned int *bad)
{
        a->mode = mode;
        if (!out)
                return ISAL_HIP_EINVAL;
        if (mode == ISAL_HIP_DIF_GUARD) {
                a->seed = seed;
                a->crc = (unsigned short *) out;
                return ISAL_HIP_OK;
        }
        if (!d || (d->type != ISAL_HIP_DIF_TYPE1 && d->type != ISAL_HIP_DIF_TYPE3) || ((uintptr_t) out & 7))
                return ISAL_HIP_EINVAL;
        if (mode == ISAL_HIP_DIF_VERIFY) {
                if (!bad || (d->flags & ~(ISAL_HIP_DIF_CHECK_GUARD | ISAL_HIP_DIF_CHECK_APP | ISAL_HIP_DIF_CHECK_REF)))
                        return ISAL_HIP_EINVAL;
                a->flags = d->flags;
                a->bad = bad;
        }
        a->type = d->type;
        a->seed = d->seed;
        a->app = d->app_tag;
        a->ref0 = d->ref0;
        a->pi = (unsigned char *) out;
        return ISAL_HIP_OK;
}

/* on the object's device: the fill (verify), then the one launch */
static int
dif_launch(const isal_hip_sector_geom *g, const uint32_t *d_image, const isal_hip_dif_args *a, long long nshards,
           void *stream)
{
        if (a->mode == ISAL_HIP_DIF_VERIFY &&
            hipMemsetAsync(a->bad, 0xff, (size_t) nshards * sizeof(unsigned int), (hipStream_t) stream) != hipSuccess) {
                (void) hipGetLastError(); /* a refused fill leaves no sticky error either; nothing was launched */
                return ISAL_HIP_EHIP;
        }
        return isal_hip_launch_sector_t10dif(g, d_image, a, stream) ? ISAL_HIP_EHIP : ISAL_HIP_OK;
}

static int
batch_dif_impl(isal_hip_batch *b, const isal_hip_sector_geom *g, const isal_hip_dif_args *a, void *stream)
{
        const int e = dif_image(&b->d_sec16);
        if (e != ISAL_HIP_OK)
                return e;
        return dif_launch(g, b->d_sec16, a, (long long) b->nstripes * (b->k + b->rows), stream);
}

static int
ragged_dif_impl(isal_hip_ragged *r, isal_hip_sector_geom *g, const isal_hip_dif_args *a, void *stream)
{
        int e;
        if ((e = isal_hip_sector_ragged_first(r, g->sector, g)) != ISAL_HIP_OK ||
            (e = dif_image(&r->d_sec16)) != ISAL_HIP_OK)
                return e;
        return dif_launch(g, r->d_sec16, a, (long long) r->nstripes * (r->k + r->rows), stream);
}

static int
batch_dif(isal_hip_batch *b, int sector, int mode, const isal_hip_dif *d, unsigned short seed, const void *out,
          unsigned int *bad, void *stream)
{
        isal_hip_sector_geom g = { 0 };
        isal_hip_dif_args a = { 0 };
        int e = dif_args(&a, mode, d, seed, out, bad);
        if (e == ISAL_HIP_OK)
                e = isal_hip_sector_batch_geom(b, sector, &g);
        if (e)
                return e < 0 ? e : ISAL_HIP_OK;
        ON_BATCH_DEVICE(b, batch_dif_impl(b, &g, &a, stream));
}

static int
ragged_dif(isal_hip_ragged *r, int sector, int mode, const isal_hip_dif *d, unsigned short seed, const void *out,
           unsigned int *bad, void *stream)
{
        isal_hip_sector_geom g = { 0 };
        isal_hip_dif_args a = { 0 };
        int e = dif_args(&a, mode, d, seed, out, bad);
        if (e == ISAL_HIP_OK)
                e = isal_hip_sector_ragged_geom(r, sector, &g);
        if (e)
                return e < 0 ? e : ISAL_HIP_OK;
        ON_BATCH_DEVICE(r, ragged_dif_impl(r, &g, &a, stream));
}

int
isal_hip_batch_sector_t10dif(isal_hip_batch *b, int sector, unsigned short seed, unsigned short *crc, void *stream)
{
        return batch_dif(b, sector, ISAL_HIP_DIF_GUARD, NULL, seed, crc, NULL, stream);
}

int
isal_hip_ragged_sector_t10dif(isal_hip_ragged *r, int sector, unsigned short seed, unsigned short *crc, void *stream)
{
        return ragged_dif(r, sector, ISAL_HIP_DIF_GUARD, NULL, seed, crc, NULL, stream);
}

int
isal_hip_batch_dif_generate(isal_hip_batch *b, int sector, const isal_hip_dif *d, unsigned char *pi, void *stream)
{
        return batch_dif(b, sector, ISAL_HIP_DIF_GENERATE, d, 0, pi, NULL, stream);
}

int
isal_hip_ragged_dif_generate(isal_hip_ragged *r, int sector, const isal_hip_dif *d, unsigned char *pi, void *stream)
{
        return ragged_dif(r, sector, ISAL_HIP_DIF_GENERATE, d, 0, pi, NULL, stream);
}

int
isal_hip_batch_dif_verify(isal_hip_batch *b, int sector, const isal_hip_dif *d, const unsigned char *pi,
                          unsigned int *bad, void *stream)
{
        return batch_dif(b, sector, ISAL_HIP_DIF_VERIFY, d, 0, pi, bad, stream);
}

int
isal_hip_ragged_dif_verify(isal_hip_ragged *r, int sector, const isal_hip_dif *d, const unsigned char *pi,
                           unsigned int *bad, void *stream)
{
        return ragged_dif(r, sector, ISAL_HIP_DIF_VERIFY, d, 0, pi, bad, stream);
}
