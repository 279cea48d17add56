/*
 * isal_hip_objects.c — the steps every device-resident stripe object's create
 * shares (the repair, overwrite, scrub and ragged batches): a row of shard
 * pointers checked while it is written, the reachability of a pointer table,
 * one host array put into a fresh device allocation and dropped again, the
 * work-item table of a ragged object. Declared in isal_hip_internal.h.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>

#include "isal_hip.h"
#include "isal_hip_internal.h"

int
isal_hip_obj_ptr_row(uint64_t *row, unsigned char *const *p, size_t n)
{
        size_t i;
        int ret = ISAL_HIP_OK;
        for (i = 0; i < n; i++) {
                const uint64_t v = (uint64_t) (uintptr_t) p[i];
                if (row)
                        row[i] = v;
                if (!v || (v & 15))
                        ret = ISAL_HIP_EINVAL;
        }
        return ret;
}

int
isal_hip_obj_reach(const uint64_t *ptrs, size_t nrows, size_t stride, size_t len, const int *lens, int dev)
{
        size_t r;
        int e;
        if (!lens)
                return len ? isal_hip_batch_check_ptrs(ptrs, nrows * stride, len, dev) : ISAL_HIP_OK;
        /* a ragged row's shards are as long as that row */
        for (r = 0; r < nrows; r++)
                if (lens[r] > 0 &&
                    (e = isal_hip_batch_check_ptrs(ptrs + r * stride, stride, (size_t) lens[r], dev)) != ISAL_HIP_OK)
                        return e;
        return ISAL_HIP_OK;
}

int
isal_hip_obj_put(void *d, const void *h, size_t bytes, size_t pad)
{
        void **dp = (void **) d;
        if (hipMalloc(dp, bytes + pad) != hipSuccess)
                return ISAL_HIP_ENOMEM;
        return hipMemcpy(*dp, h, bytes, hipMemcpyHostToDevice) == hipSuccess ? ISAL_HIP_OK : ISAL_HIP_EHIP;
}

void
isal_hip_obj_drop(void *d)
{
        if (d)
                (void) hipFree(d);
}

int
isal_hip_obj_put_items(unsigned **d, int nstripes, const int *lens, int tile, unsigned nitems)
{
        unsigned *h;
        int e;
        if (!nitems)
                return ISAL_HIP_OK;
        h = (unsigned *) malloc((size_t) nitems * 8);
        if (!h)
                return ISAL_HIP_ENOMEM;
        (void) isal_hip_ragged_items(nstripes, lens, tile, h);
        e = isal_hip_obj_put(d, h, (size_t) nitems * 8, 0);
        free(h);
        return e;
}
