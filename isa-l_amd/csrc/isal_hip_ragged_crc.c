/*
 * isal_hip_ragged_crc.c — the ragged batch's fragment checksums (isal_hip.h
 * isal_hip_ragged_crc, isal_hip_ragged_encode_crc): crc32_iscsi of every shard
 * of stripes of different lengths in one pass launch and one combine launch
 * (crc_kernels.hip crc32c_shards_rag, crc32c_combine_rag; the geometry and the
 * device image are described in isal_hip_internal.h "ragged CRC32C").
 *
 * Nothing here is built at create: the first checksum call on an object picks
 * its block size, builds the length-independent image and the {stripe, block}
 * item table, and allocates the partials; isal_hip_ragged_destroy
 * (isal_hip_ragged.c) frees them.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "isal_hip.h"
#include "isal_hip_internal.h"

/* Tiles per checksum workgroup, one value per object: ISAL_HIP_CRC_TILES when
 * set, else 64 (the uniform batch's choice, isal_hip_crc_tiles) halved while
 * one shard of every stripe together has fewer than 2048 blocks; at most
 * ISAL_HIP_CRC_RAG_MAX_TT either way. */
static int
ragged_crc_tiles(const isal_hip_ragged *r)
{
        const long long knob = isal_hip_knob(ISAL_HIP_KNOB_CRC_TILES);
        int tt = 64;
        if (knob >= 0)
                return knob < 1 ? 1 : knob > ISAL_HIP_CRC_RAG_MAX_TT ? ISAL_HIP_CRC_RAG_MAX_TT : (int) knob;
        while (tt > 1 && isal_hip_ragged_items(r->nstripes, r->h_lens, ISAL_HIP_CRC_TILE * tt, NULL) < 2048)
                tt /= 2;
        return tt;
}

static void
ragged_crc_drop(isal_hip_ragged *r)
{
        isal_hip_obj_drop(r->d_crc);
        isal_hip_obj_drop(r->d_part);
        isal_hip_obj_drop(r->d_crc_items);
        isal_hip_obj_drop(r->d_crc_first);
        r->d_crc = r->d_part = r->d_tail = NULL;
        r->d_crc_items = r->d_crc_first = NULL;
        r->crc_nitems = 0;
}

/* What the first checksum call allocates: the image, the {stripe, block} item
 * table with its per-stripe prefix, and the partials. A failure leaves the
 * object as it was before the call. */
static int
ragged_crc_setup(isal_hip_ragged *r)
{
        const size_t nsh = (size_t) (r->k + r->rows), nstripes = (size_t) r->nstripes;
        uint32_t *h_image;
        unsigned *h_first;
        size_t s, part, tail, image;
        long long nitems;
        int e, tt;
        if (r->d_crc)
                return ISAL_HIP_OK;
        tt = ragged_crc_tiles(r);
        nitems = isal_hip_ragged_items(r->nstripes, r->h_lens, ISAL_HIP_CRC_TILE * tt, NULL);
        image = isal_hip_crc32c_ragged_image_dwords(tt) * 4;
        /* one launch covers every (block, shard): refused past the limit of a
         * launch, before anything is allocated or enqueued */
        if (nitems * (long long) nsh > (long long) ISAL_HIP_RAGGED_MAX_ITEMS)
                return ISAL_HIP_EINVAL;
        h_image = (uint32_t *) malloc(image);
        h_first = (unsigned *) malloc((nstripes + 1) * sizeof(unsigned));
        if (!h_image || !h_first) {
                free(h_image);
                free(h_first);
                return ISAL_HIP_ENOMEM;
        }
        isal_hip_crc32c_ragged_image(tt, h_image);
        h_first[0] = 0;
        for (s = 0; s < nstripes; s++)
                h_first[s + 1] = h_first[s] + (unsigned) (((long long) r->h_lens[s] + (long long) ISAL_HIP_CRC_TILE * tt - 1) /
                                                          ((long long) ISAL_HIP_CRC_TILE * tt));
        part = (size_t) nitems * nsh * 256;
        tail = nstripes * nsh * 256;
        if ((e = isal_hip_obj_put(&r->d_crc, h_image, image, 0)) == ISAL_HIP_OK &&
            (e = isal_hip_obj_put(&r->d_crc_first, h_first, (nstripes + 1) * sizeof(unsigned), 0)) == ISAL_HIP_OK &&
            (e = isal_hip_obj_put_items(&r->d_crc_items, r->nstripes, r->h_lens, ISAL_HIP_CRC_TILE * tt,
                                        (unsigned) nitems)) == ISAL_HIP_OK &&
            hipMalloc((void **) &r->d_part, (part + tail) * 4) != hipSuccess)
                e = ISAL_HIP_ENOMEM;
        free(h_image);
        free(h_first);
        if (e != ISAL_HIP_OK) {
                ragged_crc_drop(r);
                (void) hipGetLastError(); /* the object stays usable: no sticky error for the next call */
                return e;
        }
        r->d_tail = r->d_part + part;
        r->crc_tt = tt;
        r->crc_nitems = (unsigned) nitems;
        return ISAL_HIP_OK;
}

static int
ragged_crc_impl(isal_hip_ragged *r, unsigned int init, unsigned int *crc, void *stream)
{
        int e;
        if (!r->nitems[TILE_BIG]) /* every length is 0 */
                return ISAL_HIP_OK;
        if ((e = ragged_crc_setup(r)) != ISAL_HIP_OK)
                return e;
        if (isal_hip_launch_crc_ragged(r->d_ptrs, r->k + r->rows, r->d_lens, r->d_crc_items, r->crc_nitems,
                                       r->crc_tt, r->d_crc, r->d_part, r->d_tail, stream) ||
            isal_hip_launch_crc_combine_ragged(r->d_part, r->d_tail, r->d_crc, r->d_lens, r->d_crc_first,
                                               r->k + r->rows, r->crc_tt, init, (uint32_t *) crc, r->nstripes,
                                               stream))
                return ISAL_HIP_EHIP;
        return ISAL_HIP_OK;
}

int
isal_hip_ragged_crc(isal_hip_ragged *r, unsigned int init, unsigned int *crc, void *stream)
{
        if (!crc)
                return ISAL_HIP_EINVAL;
        ON_BATCH_DEVICE(r, ragged_crc_impl(r, init, crc, stream));
}

static int
ragged_encode_crc_impl(isal_hip_ragged *r, unsigned int init, unsigned int *crc, void *stream)
{
        int e;
        if (!r->nitems[TILE_BIG])
                return ISAL_HIP_OK;
        /* the checksum's memory first: a refusal leaves the parity untouched */
        if ((e = ragged_crc_setup(r)) != ISAL_HIP_OK || (e = isal_hip_ragged_encode_on_device(r, stream)) != ISAL_HIP_OK)
                return e;
        return ragged_crc_impl(r, init, crc, stream);
}

int
isal_hip_ragged_encode_crc(isal_hip_ragged *r, unsigned int init, unsigned int *crc, void *stream)
{
        if (!crc)
                return ISAL_HIP_EINVAL;
        ON_BATCH_DEVICE(r, ragged_encode_crc_impl(r, init, crc, stream));
}
