/*
 * isal_hip_repair.c — the repair batch (isal_hip.h): nstripes stripes of one
 * geometry, each with its own set of nerrs erased shards, rebuilt by one
 * kernel launch per pass of up to EC_MAX_ROWS_PER_PASS rows.
 *
 * Host side, in this order (everything before the first HIP call is pure
 * arithmetic and returns the same codes on a host without a GPU):
 *   1. each stripe's erasure set is ordered and looked up in a hash table of
 *      the distinct patterns seen so far;
 *   2. a new pattern gets its recovery rows (isal_hip_decode_matrix) and its
 *      device coefficient tables, isal_hip_tables_dwords(k, nerrs) dwords at
 *      index * stride of one array;
 *   3. the pointer table (per stripe k survivors then nerrs destinations, the
 *      batch's shape) is written with its rows sorted by pattern, beside a
 *      pattern index per row: neighbouring workgroups then read the same
 *      coefficient lines (ec_kernels.hip ec_repair_v16).
 * A repair batch belongs to the device that was current when it was created
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

struct isal_hip_repair {
        int len, k, nerrs, nstripes, npat, device;
        unsigned tbl_stride; /* dwords per pattern */
        uint64_t *d_ptrs;
        uint32_t *d_pat, *d_tbl;
};

/* errs in range and distinct; mark[] (MAX_SHARDS bytes) receives the set */
static int
mark_errs(int m, int nerrs, const unsigned char *errs, unsigned char *mark)
{
        int i;
        memset(mark, 0, MAX_SHARDS);
        for (i = 0; i < nerrs; i++) {
                if (errs[i] >= m || mark[errs[i]])
                        return ISAL_HIP_EINVAL;
                mark[errs[i]] = 1;
        }
        return ISAL_HIP_OK;
}

int
isal_hip_decode_matrix(int k, int m, const unsigned char *a, int nerrs, const unsigned char *errs,
                       unsigned char *c, unsigned char *survivors)
{
        unsigned char mark[MAX_SHARDS], *b, *d;
        int i, j, r, n = 0;
        if (k < 1 || m <= k || m > MAX_SHARDS || !a || !errs || !c || !survivors || nerrs < 1 ||
            nerrs > m - k || mark_errs(m, nerrs, errs, mark) != ISAL_HIP_OK)
                return ISAL_HIP_EINVAL;
        for (i = 0; i < m && n < k; i++)
                if (!mark[i])
                        survivors[n++] = (unsigned char) i;
        b = (unsigned char *) malloc(2 * (size_t) k * k);
        if (!b)
                return ISAL_HIP_ENOMEM;
        d = b + (size_t) k * k;
        for (i = 0; i < k; i++)
                memcpy(b + (size_t) k * i, a + (size_t) k * survivors[i], (size_t) k);
        if (gf_invert_matrix(b, d, k) != 0) {
                free(b);
                return ISAL_HIP_ESINGULAR;
        }
        for (i = 0; i < nerrs; i++) {
                const int s = errs[i];
                if (s < k) { /* a data shard: its row of the inverse */
                        memcpy(c + (size_t) k * i, d + (size_t) k * s, (size_t) k);
                        continue;
                }
                for (j = 0; j < k; j++) { /* a parity shard: its encode row times the inverse */
                        unsigned char v = 0;
                        for (r = 0; r < k; r++)
                                v ^= gf_mul(d[(size_t) k * r + j], a[(size_t) k * s + r]);
                        c[(size_t) k * i + j] = v;
                }
        }
        free(b);
        return ISAL_HIP_OK;
}

/* ---- the distinct patterns of one create ---------------------------------- */

typedef struct {
        int k, m, nerrs, npat, cap;
        unsigned tbl_stride;
        const unsigned char *a;
        unsigned char *keys;  /* [npat][nerrs] ascending erasure sets */
        unsigned char *surv;  /* [npat][k] */
        uint32_t *tbl;        /* [npat][tbl_stride] */
        int32_t *slot;        /* open-addressing table of pattern indices, -1 empty */
        size_t nslot;         /* a power of two */
        unsigned char *c, *g; /* scratch: recovery rows, ec_init_tables output */
} patset;

static void
patset_free(patset *ps)
{
        free(ps->keys);
        free(ps->surv);
        free(ps->tbl);
        free(ps->slot);
        free(ps->c);
        free(ps->g);
}

static int
patset_grow(patset *ps)
{
        const int cap = ps->cap ? 2 * ps->cap : 16;
        unsigned char *keys = (unsigned char *) realloc(ps->keys, (size_t) cap * ps->nerrs);
        unsigned char *surv;
        uint32_t *tbl;
        if (!keys)
                return ISAL_HIP_ENOMEM;
        ps->keys = keys;
        surv = (unsigned char *) realloc(ps->surv, (size_t) cap * ps->k);
        if (!surv)
                return ISAL_HIP_ENOMEM;
        ps->surv = surv;
        tbl = (uint32_t *) realloc(ps->tbl, (size_t) cap * ps->tbl_stride * 4);
        if (!tbl)
                return ISAL_HIP_ENOMEM;
        ps->tbl = tbl;
        ps->cap = cap;
        return ISAL_HIP_OK;
}

/* Index of the ascending erasure set key, adding it (recovery rows, device
 * table image) when new; a negative ISAL_HIP_E* code otherwise. */
static int
patset_find(patset *ps, const unsigned char *key)
{
        uint32_t h = 2166136261u;
        size_t at;
        int i, r;
        for (i = 0; i < ps->nerrs; i++)
                h = (h ^ key[i]) * 16777619u;
        for (at = h & (ps->nslot - 1);; at = (at + 1) & (ps->nslot - 1)) {
                const int32_t p = ps->slot[at];
                if (p < 0)
                        break;
                if (!memcmp(ps->keys + (size_t) p * ps->nerrs, key, (size_t) ps->nerrs))
                        return p;
        }
        if ((size_t) (ps->npat + 1) * ps->tbl_stride * 4 > ISAL_HIP_REPAIR_MAX_TABLE_BYTES)
                return ISAL_HIP_ENOMEM;
        if (ps->npat == ps->cap && (r = patset_grow(ps)) != ISAL_HIP_OK)
                return r;
        r = isal_hip_decode_matrix(ps->k, ps->m, ps->a, ps->nerrs, key, ps->c,
                                   ps->surv + (size_t) ps->npat * ps->k);
        if (r != ISAL_HIP_OK)
                return r;
        ec_init_tables(ps->k, ps->nerrs, ps->c, ps->g);
        isal_hip_build_tables(ps->k, ps->nerrs, ps->g, ps->tbl + (size_t) ps->npat * ps->tbl_stride);
        memcpy(ps->keys + (size_t) ps->npat * ps->nerrs, key, (size_t) ps->nerrs);
        ps->slot[at] = ps->npat;
        return ps->npat++;
}

static int
repair_upload(isal_hip_repair *r, const uint64_t *h_ptrs, const uint32_t *h_pat, const uint32_t *h_tbl)
{
        const size_t nptr = (size_t) r->nstripes * (size_t) (r->k + r->nerrs);
        const size_t ntbl = (size_t) r->npat * r->tbl_stride * 4;
        int e;
        if (hipGetDevice(&r->device) != hipSuccess)
                return ISAL_HIP_EHIP;
        if (r->len > 0 &&
            (e = isal_hip_batch_check_ptrs(h_ptrs, nptr, (size_t) r->len, r->device)) != ISAL_HIP_OK)
                return e;
        if (hipMalloc((void **) &r->d_ptrs, nptr * 8) != hipSuccess ||
            hipMalloc((void **) &r->d_pat, (size_t) r->nstripes * 4) != hipSuccess ||
            hipMalloc((void **) &r->d_tbl, ntbl) != hipSuccess)
                return ISAL_HIP_ENOMEM;
        if (hipMemcpy(r->d_ptrs, h_ptrs, nptr * 8, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(r->d_pat, h_pat, (size_t) r->nstripes * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(r->d_tbl, h_tbl, ntbl, hipMemcpyHostToDevice) != hipSuccess)
                return ISAL_HIP_EHIP;
        return ISAL_HIP_OK;
}

int
isal_hip_repair_create(isal_hip_repair **out, int len, int k, int m, const unsigned char *a, int nerrs,
                       int nstripes, const unsigned char *errs, unsigned char *const *shards,
                       int *bad_stripe)
{
        isal_hip_repair *r = NULL;
        patset ps;
        unsigned char mark[MAX_SHARDS], key[MAX_SHARDS];
        uint32_t *s_pat = NULL, *h_pat = NULL, *first = NULL;
        uint64_t *h_ptrs = NULL;
        long long s;
        int i, n, ret = ISAL_HIP_OK;
        size_t stride;

        if (bad_stripe)
                *bad_stripe = -1;
        if (!out)
                return ISAL_HIP_EINVAL;
        *out = NULL;
        if (len < 0 || k < 1 || m <= k || m > MAX_SHARDS || !a || nerrs < 1 || nerrs > m - k ||
            nstripes < 1 || !errs || !shards)
                return ISAL_HIP_EINVAL;
        stride = (size_t) k + (size_t) nerrs;

        memset(&ps, 0, sizeof(ps));
        ps.k = k;
        ps.m = m;
        ps.nerrs = nerrs;
        ps.a = a;
        ps.tbl_stride = (unsigned) isal_hip_tables_dwords(k, nerrs);
        for (ps.nslot = 64; ps.nslot < 2 * (size_t) nstripes; ps.nslot *= 2)
                ;
        ps.slot = (int32_t *) malloc(ps.nslot * sizeof(int32_t));
        ps.c = (unsigned char *) malloc((size_t) nerrs * k);
        ps.g = (unsigned char *) malloc(32 * (size_t) nerrs * k);
        s_pat = (uint32_t *) malloc((size_t) nstripes * 4);
        if (!ps.slot || !ps.c || !ps.g || !s_pat) {
                ret = ISAL_HIP_ENOMEM;
                goto done;
        }
        memset(ps.slot, 0xff, ps.nslot * sizeof(int32_t));

        /* 1-2: validate every stripe, find its pattern, build new patterns' tables */
        for (s = 0; s < nstripes && ret == ISAL_HIP_OK; s++) {
                unsigned char *const *sh = shards + (size_t) s * m;
                ret = mark_errs(m, nerrs, errs + (size_t) s * nerrs, mark);
                for (i = 0; i < m && ret == ISAL_HIP_OK; i++)
                        if (!sh[i] || ((uintptr_t) sh[i] & 15))
                                ret = ISAL_HIP_EINVAL;
                if (ret == ISAL_HIP_OK) {
                        for (i = 0, n = 0; i < m; i++)
                                if (mark[i])
                                        key[n++] = (unsigned char) i;
                        if ((n = patset_find(&ps, key)) < 0)
                                ret = n;
                        else
                                s_pat[s] = (uint32_t) n;
                }
                if (ret != ISAL_HIP_OK && ret != ISAL_HIP_ENOMEM && bad_stripe)
                        *bad_stripe = (int) s;
        }
        if (ret != ISAL_HIP_OK)
                goto done;

        /* 3: rows sorted by pattern (a counting sort, stripes of one pattern in
         * their order), k survivors then the destinations in ascending order */
        h_ptrs = (uint64_t *) malloc((size_t) nstripes * stride * 8);
        h_pat = (uint32_t *) malloc((size_t) nstripes * 4);
        first = (uint32_t *) calloc((size_t) ps.npat + 1, 4);
        r = (isal_hip_repair *) calloc(1, sizeof(*r));
        if (!h_ptrs || !h_pat || !first || !r) {
                ret = ISAL_HIP_ENOMEM;
                goto done;
        }
        for (s = 0; s < nstripes; s++)
                first[s_pat[s] + 1]++;
        for (i = 0; i < ps.npat; i++)
                first[i + 1] += first[i];
        for (s = 0; s < nstripes; s++) {
                const uint32_t p = s_pat[s], row = first[p]++;
                unsigned char *const *sh = shards + (size_t) s * m;
                uint64_t *hp = h_ptrs + (size_t) row * stride;
                for (i = 0; i < k; i++)
                        hp[i] = (uint64_t) (uintptr_t) sh[ps.surv[(size_t) p * k + i]];
                for (i = 0; i < nerrs; i++)
                        hp[k + i] = (uint64_t) (uintptr_t) sh[ps.keys[(size_t) p * nerrs + i]];
                h_pat[row] = p;
        }
        r->len = len;
        r->k = k;
        r->nerrs = nerrs;
        r->nstripes = nstripes;
        r->npat = ps.npat;
        r->tbl_stride = ps.tbl_stride;
        ret = repair_upload(r, h_ptrs, h_pat, ps.tbl);
done:
        patset_free(&ps);
        free(s_pat);
        free(h_pat);
        free(h_ptrs);
        free(first);
        if (ret != ISAL_HIP_OK) {
                isal_hip_repair_destroy(r);
                return ret;
        }
        *out = r;
        return ISAL_HIP_OK;
}

static int
repair_run_impl(isal_hip_repair *r, void *stream)
{
        return isal_hip_launch_repair(r->d_ptrs, r->k + r->nerrs, r->d_pat, r->d_tbl, r->tbl_stride, r->len,
                                      r->k, r->nerrs, r->nstripes, stream)
                       ? ISAL_HIP_EHIP
                       : ISAL_HIP_OK;
}

int
isal_hip_repair_run(isal_hip_repair *r, void *stream)
{
        ON_BATCH_DEVICE(r, repair_run_impl(r, stream));
}

int
isal_hip_repair_npatterns(const isal_hip_repair *r)
{
        return r ? r->npat : ISAL_HIP_EINVAL;
}

int
isal_hip_repair_destroy(isal_hip_repair *r)
{
        if (!r)
                return ISAL_HIP_OK;
        if (r->d_ptrs)
                (void) hipFree(r->d_ptrs);
        if (r->d_pat)
                (void) hipFree(r->d_pat);
        if (r->d_tbl)
                (void) hipFree(r->d_tbl);
        free(r);
        return ISAL_HIP_OK;
}
