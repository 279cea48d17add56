/*
 * isal_hip_ragged_crc.c — the ragged batch's fragment checksums of both
 * widths (isal_hip.h isal_hip_ragged_crc, isal_hip_ragged_encode_crc and
 * isal_hip_ragged_crc64, isal_hip_ragged_encode_crc64): crc32_iscsi or any of
 * the eight crc64_* flavours of every shard of stripes of different lengths in
 * one pass launch and one combine launch (crc_kernels.hip crc32c_shards_rag,
 * crc32c_combine_rag; crc64_kernels.hip crc64_shards_rag, crc64_combine_rag;
 * the geometry and the device images are described in isal_hip_internal.h
 * "ragged CRC32C" and "ragged CRC64").
 *
 * Nothing here is built at create, and the two widths share nothing of their
 * state: the first checksum call of a width on an object picks its block size,
 * builds the {stripe, block} item table and allocates the partials
 * (isal_hip_ragged_ck, one set-up for both); CRC32C then builds its
 * length-independent image, and the first CRC64 call with a variant that
 * variant's. isal_hip_ragged_destroy (isal_hip_ragged.c) frees them.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "isal_hip.h"
#include "isal_hip_internal.h"

_Static_assert(sizeof(((isal_hip_ragged *) 0)->d_c64image) / sizeof(uint64_t *) == ISAL_HIP_CRC64_NVARIANTS,
               "one image slot per variant");

/* Tiles per checksum workgroup, one value per object and width:
 * ISAL_HIP_CRC_TILES when set, else def — 64 for CRC32C (the uniform batch's
 * choice, isal_hip_crc_tiles), 128 for CRC64 (the uniform checksum-only
 * CRC64's, isal_hip_batch.c) — halved while one shard of every stripe together
 * has fewer than 2048 blocks; at most ISAL_HIP_CRC_RAG_MAX_TT either way. */
static int
ragged_ck_tiles(const isal_hip_ragged *r, int def)
{
        const long long knob = isal_hip_knob(ISAL_HIP_KNOB_CRC_TILES);
        int tt = def;
        if (knob >= 0)
                return knob < 1 ? 1 : knob > ISAL_HIP_CRC_RAG_MAX_TT ? ISAL_HIP_CRC_RAG_MAX_TT : (int) knob;
        while (tt > 1 && isal_hip_ragged_items(r->nstripes, r->h_lens, ISAL_HIP_CRC_TILE * tt, NULL) < 2048)
                tt /= 2;
        return tt;
}

/* What the first checksum call of a width allocates: the {stripe, block} item
 * table with its per-stripe prefix, and the partials — one elem-byte word per
 * (item, shard, lane), then extra more words. A failure leaves the object as
 * it was before the call. */
static int
ragged_ck_setup(isal_hip_ragged *r, isal_hip_ragged_ck *ck, int def_tt, size_t elem, size_t extra)
{
        const size_t nsh = (size_t) (r->k + r->rows), nstripes = (size_t) r->nstripes;
        unsigned *h_first;
        long long nitems, block;
        size_t s;
        int e, tt;
        if (ck->d_part)
                return ISAL_HIP_OK;
        tt = ragged_ck_tiles(r, def_tt);
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
        if ((e = isal_hip_obj_put(&ck->d_first, h_first, (nstripes + 1) * sizeof(unsigned), 0)) == ISAL_HIP_OK &&
            (e = isal_hip_obj_put_items(&ck->d_items, r->nstripes, r->h_lens, (int) block, (unsigned) nitems)) ==
                    ISAL_HIP_OK &&
            hipMalloc(&ck->d_part, ((size_t) nitems * nsh * 256 + extra) * elem) != hipSuccess) {
                ck->d_part = NULL;
                e = ISAL_HIP_ENOMEM;
        }
        free(h_first);
        if (e != ISAL_HIP_OK) {
                isal_hip_ragged_ck_drop(ck);
                (void) hipGetLastError(); /* the object stays usable: no sticky error for the next call */
                return e;
        }
        ck->tt = tt;
        ck->nitems = (unsigned) nitems;
        return ISAL_HIP_OK;
}

/* ---- CRC32C: the partials are followed by one tail row per shard, and the
 * image depends on the block size alone ------------------------------------- */
static int
ragged_crc_setup(isal_hip_ragged *r)
{
        const size_t nsh = (size_t) (r->k + r->rows);
        uint32_t *h_image;
        size_t image;
        int e;
        if (r->d_crc)
                return ISAL_HIP_OK;
        if ((e = ragged_ck_setup(r, &r->ck32, 64, 4, (size_t) r->nstripes * nsh * 256)) != ISAL_HIP_OK)
                return e;
        image = isal_hip_crc32c_ragged_image_dwords(r->ck32.tt) * 4;
        h_image = (uint32_t *) malloc(image);
        if (h_image) {
                isal_hip_crc32c_ragged_image(r->ck32.tt, h_image);
                e = isal_hip_obj_put(&r->d_crc, h_image, image, 0);
                free(h_image);
        } else {
                e = ISAL_HIP_ENOMEM;
        }
        if (e != ISAL_HIP_OK) {
                isal_hip_obj_drop(r->d_crc);
                r->d_crc = NULL;
                isal_hip_ragged_ck_drop(&r->ck32);
                (void) hipGetLastError();
                return e;
        }
        r->d_tail = (uint32_t *) r->ck32.d_part + (size_t) r->ck32.nitems * nsh * 256;
        return ISAL_HIP_OK;
}

static int
ragged_crc_impl(isal_hip_ragged *r, unsigned int init, unsigned int *crc, void *stream)
{
        const isal_hip_ragged_ck *ck = &r->ck32;
        int e;
        if (!r->nitems[TILE_BIG]) /* every length is 0 */
                return ISAL_HIP_OK;
        if ((e = ragged_crc_setup(r)) != ISAL_HIP_OK)
                return e;
        if (isal_hip_launch_crc_ragged(r->d_ptrs, r->k + r->rows, r->d_lens, ck->d_items, ck->nitems, ck->tt, r->d_crc,
                                       (uint32_t *) ck->d_part, r->d_tail, stream) ||
            isal_hip_launch_crc_combine_ragged((const uint32_t *) ck->d_part, r->d_tail, r->d_crc, r->d_lens,
                                               ck->d_first, r->k + r->rows, ck->tt, init, (uint32_t *) crc,
                                               r->nstripes, stream))
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

/* ---- CRC64: the block size, item table and partials are the same for every
 * variant; the image is the variant's -------------------------------------- */

/* The variant's image, built and uploaded by the first call that names it and
 * kept until destroy: launches of other variants queued on any stream keep
 * reading their own. */
static int
ragged_crc64_image(isal_hip_ragged *r, int variant)
{
        const size_t bytes = isal_hip_crc64_ragged_image_entries(r->ck64.tt) * 8;
        uint64_t *h, *d = NULL;
        int e;
        if (r->d_c64image[variant])
                return ISAL_HIP_OK;
        h = (uint64_t *) malloc(bytes);
        if (!h)
                return ISAL_HIP_ENOMEM;
        isal_hip_crc64_ragged_image(variant, r->ck64.tt, h);
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
        int e = ragged_ck_setup(r, &r->ck64, 128, 8, 0);
        return e != ISAL_HIP_OK ? e : ragged_crc64_image(r, variant);
}

static int
ragged_crc64_impl(isal_hip_ragged *r, int variant, unsigned long long init, unsigned long long *crc, void *stream)
{
        const isal_hip_ragged_ck *ck = &r->ck64;
        const int refl = isal_hip_crc64_is_refl(variant);
        int e;
        if (!r->nitems[TILE_BIG]) /* every length is 0 */
                return ISAL_HIP_OK;
        if ((e = ragged_crc64_ready(r, variant)) != ISAL_HIP_OK)
                return e;
        if (isal_hip_launch_crc64_ragged(r->d_ptrs, r->k + r->rows, r->d_lens, ck->d_items, ck->nitems, ck->tt, refl,
                                         r->d_c64image[variant], (uint64_t *) ck->d_part, stream) ||
            isal_hip_launch_crc64_combine_ragged((const uint64_t *) ck->d_part, r->d_ptrs, r->d_c64image[variant],
                                                 r->d_lens, ck->d_first, r->k + r->rows, ck->tt, refl,
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
