/*
 * isal_hip_batch.c — the batched extension (isal_hip.h): many stripes of one
 * geometry, device-resident shards, asynchronous launches on the caller's
 * stream. Encode, update and check, and the CRC32C / CRC64 of every shard,
 * alone or fused with the encode (crc_kernels.hip, crc64_kernels.hip).
 *
 * A batch belongs to the device that was current when it was created; every
 * entry point runs on that device (ON_BATCH_DEVICE, isal_hip_internal.h).
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>

#include "isal_hip.h"
#include "isal_hip_internal.h"

_Static_assert(sizeof(((isal_hip_batch *) 0)->d_c64tab) / sizeof(uint64_t *) == ISAL_HIP_CRC64_NVARIANTS &&
                       sizeof(((isal_hip_batch *) 0)->d_sec64) / sizeof(uint64_t *) == ISAL_HIP_CRC64_NVARIANTS,
               "one table slot per variant (struct isal_hip_batch, isal_hip_internal.h)");

/* Every shard of a batch on device dev: hipMalloc memory of dev, managed
 * memory, or page-locked host memory whose device address is its host address.
 * A stripe's shards usually come from a few allocations, so a device range
 * already seen answers without a HIP query. */
int
isal_hip_batch_check_ptrs(const uint64_t *ptrs, size_t n, size_t len, int dev)
{
        seen_t sn;
        size_t i;
        sn.n = 0;
        for (i = 0; i < n; i++) {
                const void *p = (const void *) (uintptr_t) ptrs[i];
                hipPointerAttribute_t a;
                int sd;
                if (!p)
                        return ISAL_HIP_EINVAL;
                if ((sd = seen_dev(&sn, p, len)) >= 0) {
                        if (sd != dev)
                                return ISAL_HIP_EDEVICE;
                        continue;
                }
                if (hipPointerGetAttributes(&a, p) != hipSuccess) {
                        (void) hipGetLastError();
                        return ISAL_HIP_EINVAL; /* pageable: no kernel can reach it */
                }
                if (a.type == hipMemoryTypeDevice) {
                        hipDeviceptr_t base;
                        size_t size;
                        if (a.device != dev)
                                return ISAL_HIP_EDEVICE;
                        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t) p) == hipSuccess)
                                seen_add(&sn, (uintptr_t) base, size, a.device);
                        else
                                (void) hipGetLastError();
                } else if (a.type == hipMemoryTypeHost) {
                        if (a.devicePointer != p)
                                return ISAL_HIP_EINVAL;
                } else if (a.type != hipMemoryTypeManaged && a.type != hipMemoryTypeUnified) {
                        return ISAL_HIP_EINVAL;
                }
        }
        return ISAL_HIP_OK;
}

int
isal_hip_batch_create(isal_hip_batch **out, int len, int k, int rows, const unsigned char *gftbls,
                      int nstripes, unsigned char *const *data, unsigned char *const *coding)
{
        isal_hip_batch *b;
        uint64_t *h_ptrs;
        long long s, stride = (long long) k + rows;
        size_t nptr;
        int j, vec16 = 1;
        if (!out || len < 0 || k < 0 || rows <= 0 || nstripes <= 0 || !gftbls || !coding ||
            (k > 0 && !data))
                return ISAL_HIP_EINVAL;
        *out = NULL;
        b = (isal_hip_batch *) calloc(1, sizeof(*b));
        nptr = (size_t) nstripes * (size_t) stride;
        h_ptrs = (uint64_t *) malloc(nptr * 8);
        if (!b || !h_ptrs) {
                free(b);
                free(h_ptrs);
                return ISAL_HIP_ENOMEM;
        }
        for (s = 0; s < nstripes; s++) {
                for (j = 0; j < k; j++)
                        h_ptrs[s * stride + j] = (uint64_t) (uintptr_t) data[s * k + j];
                for (j = 0; j < rows; j++)
                        h_ptrs[s * stride + k + j] = (uint64_t) (uintptr_t) coding[s * rows + j];
        }
        for (s = 0; s < (long long) nptr; s++)
                if (h_ptrs[s] & 15)
                        vec16 = 0;
        b->len = len;
        b->k = k;
        b->rows = rows;
        b->nstripes = nstripes;
        b->vec16 = vec16;
        if (hipGetDevice(&b->device) != hipSuccess) {
                free(h_ptrs);
                isal_hip_batch_destroy(b);
                return ISAL_HIP_EHIP;
        }
        if (len > 0 && (j = isal_hip_batch_check_ptrs(h_ptrs, nptr, (size_t) len, b->device)) != ISAL_HIP_OK) {
                free(h_ptrs);
                isal_hip_batch_destroy(b);
                return j;
        }
        if (hipMalloc((void **) &b->d_ptrs, nptr * 8) != hipSuccess ||
            hipMemcpy(b->d_ptrs, h_ptrs, nptr * 8, hipMemcpyHostToDevice) != hipSuccess) {
                free(h_ptrs);
                isal_hip_batch_destroy(b);
                return ISAL_HIP_EHIP;
        }
        free(h_ptrs);
        if (isal_hip_batch_set_tables(b, gftbls) != 0) {
                isal_hip_batch_destroy(b);
                return ISAL_HIP_EHIP;
        }
        *out = b;
        return ISAL_HIP_OK;
}

/* The HIP call at an ISAL_HIP_FAULT site of the batch (isal_hip_internal.h):
 * an armed site fails without the call being issued. */
#define BATCH_TRY_AT(site, call) (isal_hip_knob(ISAL_HIP_KNOB_FAULT) == (site) ? hipErrorOutOfMemory : (call))

/* All or nothing: the new coefficient tables, the LDS product tables of the
 * wide passes and the host-side row masks are built and uploaded into fresh
 * device buffers first; only when nothing can fail any more are they
 * published together and the old buffers freed. A failed replacement leaves
 * d_tbl, d_ldsx, xr and em on the old matrix, and the batch usable. */
static int
batch_set_tables_impl(isal_hip_batch *b, const unsigned char *gftbls)
{
        size_t n, nw = 0;
        uint32_t *h, *d_tbl = NULL;
        uint64_t *hx = NULL, *d_ldsx = NULL;
        hipError_t e;
        isal_hip_xrows xr;
        isal_hip_encmask em;
        if (!b || !gftbls)
                return ISAL_HIP_EINVAL;
        n = isal_hip_tables_dwords(b->k, b->rows);
        h = (uint32_t *) malloc(n * 4 + 4);
        if (!h)
                return ISAL_HIP_ENOMEM;
        /* the wide passes' LDS product tables (ec_encode_ldsx): k <= 64, a
         * pass of at least 4 rows (4 only when ISAL_HIP_ENC_LDSX=1 forces it) */
        if (b->k >= 1 && b->k <= 64 && b->rows >= 4) {
                nw = isal_hip_ldsx_words(b->k, b->rows);
                hx = (uint64_t *) malloc(nw * 8);
                if (!hx) {
                        free(h);
                        return ISAL_HIP_ENOMEM;
                }
                isal_hip_build_ldsx_tables(b->k, b->rows, gftbls, hx);
        }
        isal_hip_build_tables(b->k, b->rows, gftbls, h);
        isal_hip_xor_rows(b->k, b->rows, gftbls, &xr);
        isal_hip_enc_masks(b->k, b->rows, gftbls, &em);
        e = hipMalloc((void **) &d_tbl, n * 4 + 4);
        if (e == hipSuccess)
                e = hipMemcpy(d_tbl, h, n * 4, hipMemcpyHostToDevice);
        free(h);
        if (e == hipSuccess && hx) {
                /* the product tables are optional: without device memory for
                 * them the batch's wide passes take the other kernels, and
                 * the next launch must not find this failure as HIP's last
                 * error */
                if (BATCH_TRY_AT(FAULT_LDSX_ALLOC, hipMalloc((void **) &d_ldsx, nw * 8)) != hipSuccess) {
                        (void) hipGetLastError();
                        d_ldsx = NULL;
                } else {
                        e = BATCH_TRY_AT(FAULT_LDSX_H2D, hipMemcpy(d_ldsx, hx, nw * 8, hipMemcpyHostToDevice));
                }
        }
        free(hx);
        /* launches already queued on any (possibly non-blocking) stream may
         * still read the old tables: let them finish before those are freed */
        if (e == hipSuccess && b->d_tbl)
                e = hipDeviceSynchronize();
        if (e != hipSuccess) {
                (void) hipGetLastError();
                if (d_tbl)
                        (void) hipFree(d_tbl);
                if (d_ldsx)
                        (void) hipFree(d_ldsx);
                return ISAL_HIP_EHIP;
        }
        if (b->d_tbl)
                (void) hipFree(b->d_tbl);
        if (b->d_ldsx)
                (void) hipFree(b->d_ldsx);
        b->d_tbl = d_tbl;
        b->d_ldsx = d_ldsx;
        b->xr = xr;
        b->em = em;
        b->em.ldsx = b->d_ldsx;
        return ISAL_HIP_OK;
}

static int
batch_encode_impl(isal_hip_batch *b, void *stream)
{
        if (!b)
                return ISAL_HIP_EINVAL;
        return isal_hip_launch_encode(b->d_ptrs, b->k + b->rows, 0, b->k, b->d_tbl, b->len, b->k,
                                      b->rows, b->nstripes, b->vec16, &b->em, stream)
                       ? ISAL_HIP_EHIP
                       : ISAL_HIP_OK;
}

static int
batch_update_impl(isal_hip_batch *b, int vec_i, void *stream)
{
        if (!b || vec_i < 0 || vec_i >= b->k)
                return ISAL_HIP_EINVAL;
        return isal_hip_launch_update(b->d_ptrs, b->k + b->rows, vec_i, b->k, b->d_tbl, b->len,
                                      b->k, b->rows, vec_i, b->nstripes, b->vec16, stream)
                       ? ISAL_HIP_EHIP
                       : ISAL_HIP_OK;
}

static int
batch_check_impl(isal_hip_batch *b, unsigned long long *bad, void *stream)
{
        if (!b || !bad || !b->vec16)
                return ISAL_HIP_EINVAL;
        return isal_hip_launch_verify_batch(b->d_ptrs, b->k + b->rows, 0, b->k, b->d_tbl, b->len, b->k, b->rows,
                                            b->nstripes, &b->em, bad, stream)
                       ? ISAL_HIP_EHIP
                       : ISAL_HIP_OK;
}

int
isal_hip_batch_destroy(isal_hip_batch *b)
{
        if (!b)
                return ISAL_HIP_OK;
        if (b->d_ptrs)
                (void) hipFree(b->d_ptrs);
        if (b->d_tbl)
                (void) hipFree(b->d_tbl);
        if (b->d_ldsx)
                (void) hipFree(b->d_ldsx);
        if (b->d_crc)
                (void) hipFree(b->d_crc);
        if (b->d_part)
                (void) hipFree(b->d_part);
        for (int v = 0; v < ISAL_HIP_CRC64_NVARIANTS; v++) {
                if (b->d_c64tab[v])
                        (void) hipFree(b->d_c64tab[v]);
                if (b->d_c64tab_ck[v])
                        (void) hipFree(b->d_c64tab_ck[v]);
        }
        if (b->d_c64part)
                (void) hipFree(b->d_c64part);
        /* what the sector checksums uploaded (isal_hip_sector_crc.c) */
        isal_hip_obj_drop(b->d_sec32);
        for (int v = 0; v < ISAL_HIP_CRC64_NVARIANTS; v++)
                isal_hip_obj_drop(b->d_sec64[v]);
        isal_hip_obj_drop(b->d_sec16); /* ... and the T10 guard's (isal_hip_dif.c) */
        free(b);
        return ISAL_HIP_OK;
}

/* ---- CRC32C of the batch's shards (isal_hip.h) ---------------------------- */

/* Tiles per CRC workgroup: `def` (64 for both CRC32C and CRC64: 256 KiB of
 * each shard per block, partials 0.1 % (CRC32C) / 0.2 % (CRC64) of the bytes
 * — profiles/r02/r02_crc_tiles_sweep_b.jsonl, r03_crc_tiles_sweep.jsonl), halved
 * while the launch would have fewer than 2048 workgroups.
 * ISAL_HIP_CRC_TILES overrides. Also the drop-in checksum routes' choice
 * (isal_hip_crcapi.c). */
int
isal_hip_crc_tiles(int len, int nstripes, int def)
{
        const long long knob = isal_hip_knob(ISAL_HIP_KNOB_CRC_TILES);
        long long ntiles = ((long long) len + ISAL_HIP_CRC_TILE - 1) / ISAL_HIP_CRC_TILE;
        int tt = knob >= 0 ? (int) knob : def;
        if (tt < 1)
                tt = 1;
        if (knob >= 0)
                return tt;
        while (tt > 1 && (long long) nstripes * ((ntiles + tt - 1) / tt) < 2048)
                tt /= 2;
        return tt;
}

static int
batch_crc_setup(isal_hip_batch *b)
{
        uint32_t *h;
        const size_t image = (size_t) ISAL_HIP_CRC_IMAGE_DWORDS * 4;
        size_t nsh, part, tail;
        hipError_t e;
        if (b->d_crc)
                return ISAL_HIP_OK;
        /* 64 tiles per block: the checksum-only pass is memory-side bound and runs
         * 12 % faster than at 16, the fused pass is flat from 16 to 64
         * (profiles/r02/r02_crc_tiles_sweep_b.jsonl) */
        isal_hip_crc_geometry(b->len, isal_hip_crc_tiles(b->len, b->nstripes, 64), &b->crc);
        nsh = (size_t) b->nstripes * (size_t) (b->k + b->rows);
        part = nsh * (size_t) b->crc.nblk * 256;
        tail = nsh * 256;
        h = (uint32_t *) malloc(image);
        if (!h)
                return ISAL_HIP_ENOMEM;
        isal_hip_crc32c_image(b->len, b->crc.tt, h);
        e = hipMalloc((void **) &b->d_crc, image);
        if (e == hipSuccess)
                e = hipMemcpy(b->d_crc, h, image, hipMemcpyHostToDevice);
        free(h);
        if (e == hipSuccess)
                e = hipMalloc((void **) &b->d_part, (part + tail) * 4);
        if (e != hipSuccess) {
                if (b->d_crc)
                        (void) hipFree(b->d_crc);
                b->d_crc = b->d_part = NULL;
                return e == hipErrorOutOfMemory ? ISAL_HIP_ENOMEM : ISAL_HIP_EHIP;
        }
        b->d_tail = b->d_part + part;
        return ISAL_HIP_OK;
}

static int
batch_crc_finish(isal_hip_batch *b, unsigned int init, unsigned int *crc, void *stream)
{
        const long long nsh = (long long) b->nstripes * (b->k + b->rows);
        return isal_hip_launch_crc_combine(b->d_part, b->d_tail, b->d_crc + ISAL_HIP_CRC_TAB_DWORDS,
                                           b->crc.nblk, b->crc.tail != 0, init, (uint32_t *) crc,
                                           nsh, stream)
                       ? ISAL_HIP_EHIP
                       : ISAL_HIP_OK;
}

static int
batch_crc_empty(isal_hip_batch *b, unsigned int init, unsigned int *crc, void *stream)
{
        /* crc32_iscsi of 0 bytes is init_crc */
        const size_t n = (size_t) b->nstripes * (size_t) (b->k + b->rows);
        return hipMemsetD32Async((hipDeviceptr_t) crc, (int) init, n, (hipStream_t) stream) ==
                               hipSuccess
                       ? ISAL_HIP_OK
                       : ISAL_HIP_EHIP;
}

static int
batch_crc_impl(isal_hip_batch *b, unsigned int init, unsigned int *crc, void *stream)
{
        int r;
        if (!b || !crc)
                return ISAL_HIP_EINVAL;
        if (b->len == 0)
                return batch_crc_empty(b, init, crc, stream);
        if ((r = batch_crc_setup(b)) != ISAL_HIP_OK)
                return r;
        if (isal_hip_launch_crc(b->d_ptrs, b->k + b->rows, 0, b->k + b->rows, b->nstripes, b->len,
                                b->vec16, b->crc.tt, b->d_crc, b->d_part, b->d_tail,
                                b->k + b->rows, 0, stream))
                return ISAL_HIP_EHIP;
        return batch_crc_finish(b, init, crc, stream);
}

/* ---- CRC64 of the batch's shards (isal_hip.h) ----------------------------- */

/* ck: the checksum-only pass (else the fused encode + CRC64 pass). */
static int
batch_crc64_setup(isal_hip_batch *b, int variant, int ck)
{
        isal_hip_crc64_geom g;
        uint64_t *h, *d = NULL;
        hipError_t e;
        const size_t tab = ISAL_HIP_CRC64_TAB_ENTRIES;
        uint64_t **slot = ck ? &b->d_c64tab_ck[variant] : &b->d_c64tab[variant];
        if (*slot)
                return ISAL_HIP_OK;
        if (!b->d_c64part && !b->c64_tt) {
                /* Tiles per block: the fused pass 64 (flat from 32 to 64,
                 * profiles/r03/r03_crc_tiles_sweep.jsonl; 128 is 1.2-1.6 %
                 * slower), the checksum-only pass with its two chains per lane
                 * 128 (+1.3-1.6 % over 64, profiles/r05/r05_crc64_tiles_ab.txt).
                 * isal_hip_crc_tiles halves both alike for small batches, so
                 * c64_tt_ck >= c64_tt and the partials sized for c64_tt hold
                 * either. */
                b->c64_tt = isal_hip_crc_tiles(b->len, b->nstripes, 64);
                b->c64_tt_ck = isal_hip_crc_tiles(b->len, b->nstripes, 128);
                isal_hip_crc64_geometry(b->len, b->c64_tt < b->c64_tt_ck ? b->c64_tt : b->c64_tt_ck, &g);
                if (g.nblk) {
                        e = hipMalloc((void **) &b->d_c64part, (size_t) b->nstripes *
                                                                       (size_t) (b->k + b->rows) *
                                                                       (size_t) g.nblk * 256 * 8);
                        if (e != hipSuccess) {
                                b->d_c64part = NULL;
                                b->c64_tt = b->c64_tt_ck = 0; /* retry the whole setup next time */
                                return e == hipErrorOutOfMemory ? ISAL_HIP_ENOMEM : ISAL_HIP_EHIP;
                        }
                }
        }
        h = (uint64_t *) malloc(tab * 8);
        if (!h)
                return ISAL_HIP_ENOMEM;
        isal_hip_crc64_tables(variant, b->len, ck ? b->c64_tt_ck : b->c64_tt, h);
        /* a fresh buffer per variant: launches of other variants queued on any
         * stream keep reading their own tables */
        e = hipMalloc((void **) &d, tab * 8);
        if (e == hipSuccess)
                e = hipMemcpy(d, h, tab * 8, hipMemcpyHostToDevice);
        free(h);
        if (e != hipSuccess) {
                if (d)
                        (void) hipFree(d);
                return e == hipErrorOutOfMemory ? ISAL_HIP_ENOMEM : ISAL_HIP_EHIP;
        }
        *slot = d; /* published only once filled */
        return ISAL_HIP_OK;
}

static int
batch_crc64_impl(isal_hip_batch *b, int variant, unsigned long long init,
                     unsigned long long *crc, void *stream)
{
        int r;
        if (!b || !crc || variant < 0 || variant >= ISAL_HIP_CRC64_NVARIANTS)
                return ISAL_HIP_EINVAL;
        if ((r = batch_crc64_setup(b, variant, 1)) != ISAL_HIP_OK)
                return r;
        return isal_hip_launch_crc64(b->d_ptrs, b->k + b->rows, b->k + b->rows, b->nstripes,
                                     b->len, b->vec16, isal_hip_crc64_is_refl(variant), b->c64_tt_ck,
                                     b->d_c64tab_ck[variant], b->d_c64part,
                                     isal_hip_crc64_init_term(variant, b->len, init),
                                     (uint64_t *) crc, stream)
                       ? ISAL_HIP_EHIP
                       : ISAL_HIP_OK;
}

static int
batch_encode_crc64_impl(isal_hip_batch *b, int variant, unsigned long long init,
                            unsigned long long *crc, void *stream)
{
        int r;
        isal_hip_crc64_geom g;
        if (!b || !crc || variant < 0 || variant >= ISAL_HIP_CRC64_NVARIANTS)
                return ISAL_HIP_EINVAL;
        if ((r = batch_crc64_setup(b, variant, 0)) != ISAL_HIP_OK)
                return r;
        isal_hip_crc64_geometry(b->len, b->c64_tt, &g);
        if (b->vec16 && b->len % 16 == 0 && g.nblk > 0 && b->rows <= EC_MAX_ROWS_PER_PASS &&
            b->k >= 1 && b->k <= ISAL_HIP_CRC64_MAX_FUSED_K)
                /* one pass over the stripe: encode + CRC64 of all k + rows shards */
                return isal_hip_launch_encode_crc64(
                               b->d_ptrs, b->k, b->rows, b->nstripes, b->len, b->d_tbl, &b->xr,
                               isal_hip_crc64_is_refl(variant), b->c64_tt, b->d_c64tab[variant],
                               b->d_c64part, isal_hip_crc64_init_term(variant, b->len, init),
                               (uint64_t *) crc, stream)
                       ? ISAL_HIP_EHIP
                       : ISAL_HIP_OK;
        /* unaligned shards, short or ragged len, wide stripes: encode, then CRC64 */
        if (isal_hip_batch_encode(b, stream) != ISAL_HIP_OK)
                return ISAL_HIP_EHIP;
        return isal_hip_batch_crc64(b, variant, init, crc, stream);
}

static int
batch_encode_crc_impl(isal_hip_batch *b, unsigned int init, unsigned int *crc, void *stream)
{
        int r;
        if (!b || !crc)
                return ISAL_HIP_EINVAL;
        if (b->len == 0)
                return batch_crc_empty(b, init, crc, stream);
        if ((r = batch_crc_setup(b)) != ISAL_HIP_OK)
                return r;
        if (b->vec16 && b->len % 16 == 0 && b->k >= 1 && b->k <= ISAL_HIP_CRC_MAX_FUSED_K) {
                /* one pass over the stripe: encode + CRC of all k + rows shards
                 * (row 0's chains formed from the sources' when it is a 0/1 row) */
                if (isal_hip_launch_encode_crc(b->d_ptrs, b->k + b->rows, 0, b->k, b->d_tbl, &b->xr,
                                               b->len, b->k, b->rows, b->nstripes, b->crc.tt,
                                               b->d_crc, b->d_part, b->d_tail, stream))
                        return ISAL_HIP_EHIP;
        } else {
                /* unaligned shards, ragged len or very wide k: encode, then CRC */
                if (isal_hip_batch_encode(b, stream) != ISAL_HIP_OK)
                        return ISAL_HIP_EHIP;
                if (isal_hip_launch_crc(b->d_ptrs, b->k + b->rows, 0, b->k + b->rows, b->nstripes,
                                        b->len, b->vec16, b->crc.tt, b->d_crc, b->d_part,
                                        b->d_tail, b->k + b->rows, 0, stream))
                        return ISAL_HIP_EHIP;
        }
        return batch_crc_finish(b, init, crc, stream);
}

/* ---- the batch entry points run on the batch's device (ON_BATCH_DEVICE,
 * isal_hip_internal.h) ---------------------------------------------------- */

int
isal_hip_batch_set_tables(isal_hip_batch *b, const unsigned char *gftbls)
{
        ON_BATCH_DEVICE(b, batch_set_tables_impl(b, gftbls));
}

int
isal_hip_batch_encode(isal_hip_batch *b, void *stream)
{
        ON_BATCH_DEVICE(b, batch_encode_impl(b, stream));
}

int
isal_hip_batch_update(isal_hip_batch *b, int vec_i, void *stream)
{
        ON_BATCH_DEVICE(b, batch_update_impl(b, vec_i, stream));
}

int
isal_hip_batch_check(isal_hip_batch *b, unsigned long long *bad, void *stream)
{
        ON_BATCH_DEVICE(b, batch_check_impl(b, bad, stream));
}

int
isal_hip_batch_crc(isal_hip_batch *b, unsigned int init, unsigned int *crc, void *stream)
{
        ON_BATCH_DEVICE(b, batch_crc_impl(b, init, crc, stream));
}

int
isal_hip_batch_crc64(isal_hip_batch *b, int variant, unsigned long long init,
                     unsigned long long *crc, void *stream)
{
        ON_BATCH_DEVICE(b, batch_crc64_impl(b, variant, init, crc, stream));
}

int
isal_hip_batch_encode_crc64(isal_hip_batch *b, int variant, unsigned long long init,
                            unsigned long long *crc, void *stream)
{
        ON_BATCH_DEVICE(b, batch_encode_crc64_impl(b, variant, init, crc, stream));
}

int
isal_hip_batch_encode_crc(isal_hip_batch *b, unsigned int init, unsigned int *crc, void *stream)
{
        ON_BATCH_DEVICE(b, batch_encode_crc_impl(b, init, crc, stream));
}
