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
};

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

static int
overwrite_run_impl(isal_hip_overwrite *o, int flags, void *stream)
{
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
        free(o);
        return ISAL_HIP_OK;
}
