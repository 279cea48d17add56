/*
 * isal_hip_ragged_crc64.c — the ragged batch's CRC64 fragment checksums
 * (isal_hip.h isal_hip_ragged_crc64, isal_hip_ragged_encode_crc64): any of the
 * eight crc64_* flavours of every shard of stripes of different lengths in one
 * pass launch and one combine launch (crc64_kernels.hip crc64_shards_rag,
 * crc64_combine_rag; the geometry and the device image are described in
 * isal_hip_internal.h "ragged CRC64").
 *
 * Nothing here is built at create, and nothing is shared with the CRC32C
 * state (isal_hip_ragged_crc.c): the first CRC64 call on an object picks its
 * block size, builds the {stripe, block} item table and allocates the
 * partials, all of them the same for every variant; the first call with a
 * variant builds and uploads that variant's length-independent image.
 * isal_hip_ragged_destroy (isal_hip_ragged.c) frees them.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "isal_hip.h"
#include "isal_hip_internal.h"

_Static_assert(sizeof(((isal_hip_ragged *) 0)->d_c64image) / sizeof(uint64_t *) == ISAL_HIP_CRC64_NVARIANTS,
               "one image slot per variant");

/* Tiles per checksum workgroup, one value per object: ISAL_HIP_CRC_TILES when
 * set, else 128 (the uniform checksum-only CRC64's choice, isal_hip_batch.c)
 * halved while one shard of every stripe together has fewer than 2048 blocks;
 * at most ISAL_HIP_CRC_RAG_MAX_TT either way. */
static int
ragged_crc64_tiles(const isal_hip_ragged *r)
{
        const long long knob = isal_hip_knob(ISAL_HIP_KNOB_CRC_TILES);
        int tt = 128;
        if (knob >= 0)
                return knob < 1 ? 1 : knob > ISAL_HIP_CRC_RAG_MAX_TT ? ISAL_HIP_CRC_RAG_MAX_TT : (int) knob;
        while (tt > 1 && isal_hip_ragged_items(r->nstripes, r->h_lens, ISAL_HIP_CRC_TILE * tt, NULL) < 2048)
                tt /= 2;
        return tt;
}

static void
ragged_crc64_drop(isal_hip_ragged *r)
{
        isal_hip_obj_drop(r->d_c64part);
        isal_hip_obj_drop(r->d_c64_items);
        isal_hip_obj_drop(r->d_c64_first);
        r->d_c64part = NULL;
        r->d_c64_items = r->d_c64_first = NULL;
        r->c64_nitems = 0;
        r->c64_tt = 0;
}

/* What the first CRC64 call allocates for every variant: the {stripe, block}
 * item table with its per-stripe prefix, and the partials. A failure leaves
 * the object as it was before the call. */
static int
ragged_crc64_setup(isal_hip_ragged *r)
{
        const size_t nsh = (size_t) (r->k + r->rows), nstripes = (size_t) r->nstripes;
        unsigned *h_first;
        long long nitems, block;
        size_t s;
        int e, tt;
        if (r->d_c64part)
                return ISAL_HIP_OK;
        tt = ragged_crc64_tiles(r);
        block = (long long) ISAL_HIP_CRC_TILE * tt;
        nitems = isal_hip_ragged_items(r->nstripes, r->h_lens, (int) block, NULL);
        /* one launch covers every (block, shard): refused past the limit of a
         * launch, before anything is allocated or enqueued */
        if (nitems * (long long) nsh > (long long) ISAL_HIP_RAGGED_MAX_ITEMS)
                return ISAL_HIP_EINVAL;
        h_first = (unsigned *) malloc((nstripes + 1) * sizeof(unsigned));
        if (!h_first)
                return ISAL_HIP_ENOMEM;
        h_first[0] = 0;
        for (s = 0; s < nstripes; s++)
                h_first[s + 1] = h_first[s] + (unsigned) (((long long) r->h_lens[s] + block - 1) / block);
        if ((e = isal_hip_obj_put(&r->d_c64_first, h_first, (nstripes + 1) * sizeof(unsigned), 0)) == ISAL_HIP_OK &&
            (e = isal_hip_obj_put_items(&r->d_c64_items, r->nstripes, r->h_lens, (int) block, (unsigned) nitems)) ==
                    ISAL_HIP_OK &&
            hipMalloc((void **) &r->d_c64part, (size_t) nitems * nsh * 256 * 8) != hipSuccess) {
                r->d_c64part = NULL;
                e = ISAL_HIP_ENOMEM;
        }
        free(h_first);
        if (e != ISAL_HIP_OK) {
                ragged_crc64_drop(r);
                (void) hipGetLastError(); /* the object stays usable: no sticky error for the next call */
                return e;
        }
        r->c64_tt = tt;
        r->c64_nitems = (unsigned) nitems;
        return ISAL_HIP_OK;
}

/* The variant's image, built and uploaded by the first call that names it and
 * kept until destroy: launches of other variants queued on any stream keep
 * reading their own. */
static int
ragged_crc64_image(isal_hip_ragged *r, int variant)
{
        const size_t bytes = isal_hip_crc64_ragged_image_entries(r->c64_tt) * 8;
        uint64_t *h, *d = NULL;
        int e;
        if (r->d_c64image[variant])
                return ISAL_HIP_OK;
        h = (uint64_t *) malloc(bytes);
        if (!h)
                return ISAL_HIP_ENOMEM;
        isal_hip_crc64_ragged_image(variant, r->c64_tt, h);
        e = isal_hip_obj_put(&d, h, bytes, 0);
        free(h);
        if (e != ISAL_HIP_OK) {
                isal_hip_obj_drop(d);
                (void) hipGetLastError();
                return e;
        }
        r->d_c64image[variant] = d; /* published only once filled */
        return ISAL_HIP_OK;
}

static int
ragged_crc64_ready(isal_hip_ragged *r, int variant)
{
        int e = ragged_crc64_setup(r);
        return e != ISAL_HIP_OK ? e : ragged_crc64_image(r, variant);
}

static int
ragged_crc64_impl(isal_hip_ragged *r, int variant, unsigned long long init, unsigned long long *crc, void *stream)
{
        const int refl = isal_hip_crc64_is_refl(variant);
        int e;
        if (!r->nitems[TILE_BIG]) /* every length is 0 */
                return ISAL_HIP_OK;
        if ((e = ragged_crc64_ready(r, variant)) != ISAL_HIP_OK)
                return e;
        if (isal_hip_launch_crc64_ragged(r->d_ptrs, r->k + r->rows, r->d_lens, r->d_c64_items, r->c64_nitems,
                                         r->c64_tt, refl, r->d_c64image[variant], r->d_c64part, stream) ||
            isal_hip_launch_crc64_combine_ragged(r->d_c64part, r->d_ptrs, r->d_c64image[variant], r->d_lens,
                                                 r->d_c64_first, r->k + r->rows, r->c64_tt, refl,
                                                 isal_hip_crc64_ring_poly(variant), (uint64_t) init,
                                                 (uint64_t *) crc, r->nstripes, stream))
                return ISAL_HIP_EHIP;
        return ISAL_HIP_OK;
}

int
isal_hip_ragged_crc64(isal_hip_ragged *r, int variant, unsigned long long init, unsigned long long *crc,
                      void *stream)
{
        if (!r || !crc || variant < 0 || variant >= ISAL_HIP_CRC64_NVARIANTS)
                return ISAL_HIP_EINVAL;
        ON_BATCH_DEVICE(r, ragged_crc64_impl(r, variant, init, crc, stream));
}

static int
ragged_encode_crc64_impl(isal_hip_ragged *r, int variant, unsigned long long init, unsigned long long *crc,
                         void *stream)
{
        int e;
        if (!r->nitems[TILE_BIG])
                return ISAL_HIP_OK;
        /* the checksum's memory and the variant's image first: a refusal leaves
         * the parity untouched */
        if ((e = ragged_crc64_ready(r, variant)) != ISAL_HIP_OK ||
            (e = isal_hip_ragged_encode_on_device(r, stream)) != ISAL_HIP_OK)
                return e;
        return ragged_crc64_impl(r, variant, init, crc, stream);
}

int
isal_hip_ragged_encode_crc64(isal_hip_ragged *r, int variant, unsigned long long init, unsigned long long *crc,
                             void *stream)
{
        if (!r || !crc || variant < 0 || variant >= ISAL_HIP_CRC64_NVARIANTS)
                return ISAL_HIP_EINVAL;
        ON_BATCH_DEVICE(r, ragged_encode_crc64_impl(r, variant, init, crc, stream));
}
