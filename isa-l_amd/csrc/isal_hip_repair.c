/*
 * isal_hip_repair.c — the repair batch (isal_hip.h): nstripes stripes of one
 * geometry, each with its own set of nerrs erased shards, rebuilt by one
 * kernel launch per pass of up to EC_MAX_ROWS_PER_PASS rows.
 *
 * Host side, in this order (everything before the first HIP call is pure
 * arithmetic and returns the same codes on a host without a GPU; the steps
 * every stripe object shares are isal_hip_objects.c's):
 *   1. each stripe's erasure set and shard pointers (non-NULL, 16-byte
 *      aligned) are checked, the set is ordered and looked up in a hash table
 *      of the distinct patterns seen so far (stripe_pattern, both creates);
 *   2. a new pattern gets its recovery rows (isal_hip_decode_matrix) and its
 *      device coefficient tables, isal_hip_tables_dwords(k, nerrs) dwords at
 *      index * stride of one array;
 *   3. the pointer table (per stripe k survivors then nerrs destinations, the
 *      batch's shape, pattern_row) is written with its rows sorted by
 *      pattern, beside a pattern index per row: neighbouring workgroups then read the same
 *      coefficient lines (ec_kernels.hip ec_repair_v16).
 * A repair batch belongs to the device that was current when it was created
 * (ON_BATCH_DEVICE).
 *
 * isal_hip_repair_create_ragged builds the same object for stripes that each
 * have their own length and their own erasure count. A pattern is then the
 * pair (count, erasure set), and the stripes are grouped into count classes:
 * class c holds the stripes of non-zero length that lost c shards, and gets
 * what the uniform create builds for the whole object (rows sorted by
 * pattern, k survivors then c destinations, a pattern word per row) plus a
 * length per row and the ragged batch's item tables, one per tile size its
 * passes use. Patterns of different counts have tables of different sizes, so
 * a row's pattern word is the dword offset of its tables in the one table
 * array. Everything but the tables travels in one device allocation.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "erasure_code.h"
#include "isal_hip.h"
#include "isal_hip_internal.h"

/* one count class of a ragged repair; the device pointers lie in d_blob */
typedef struct {
        int nerrs;
        unsigned nrows, nitems[NTILES];
        uint64_t *d_ptrs;
        uint32_t *d_pat;
        int *d_lens;
        unsigned *d_items[NTILES];
} rclass;

struct isal_hip_repair {
        int len, k, nerrs, nstripes, npat, device;
        unsigned tbl_stride; /* dwords per pattern */
        uint64_t *d_ptrs;
        uint32_t *d_pat, *d_tbl;
        /* isal_hip_repair_create_ragged: classes in ascending count */
        int ragged, nclass;
        rclass *cls;
        unsigned char *d_blob;
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

/* A pattern is (count, ascending erasure set): its key is kw = 1 + the largest
 * count bytes, the count, the set, then zeros. */
typedef struct {
        int k, m, kw, npat, cap;
        size_t tbl_dwords, tbl_cap; /* used, allocated */
        const unsigned char *a;
        unsigned char *keys;  /* [npat][kw] */
        unsigned char *surv;  /* [npat][k] */
        uint32_t *off;        /* [npat] dword offset of the pattern's tables in tbl */
        uint32_t *tbl;        /* every pattern's device table image, in order of first use */
        int32_t *slot;        /* open-addressing table of pattern indices, -1 empty */
        size_t nslot;         /* a power of two */
        unsigned char *c, *g; /* scratch: recovery rows, ec_init_tables output */
} patset;

static void
patset_free(patset *ps)
{
        free(ps->keys);
        free(ps->surv);
        free(ps->off);
        free(ps->tbl);
        free(ps->slot);
        free(ps->c);
        free(ps->g);
}

/* an empty set for patterns of up to max_errs erasures among nstripes stripes */
static int
patset_init(patset *ps, int k, int m, const unsigned char *a, int max_errs, int nstripes)
{
        memset(ps, 0, sizeof(*ps));
        ps->k = k;
        ps->m = m;
        ps->kw = 1 + max_errs;
        ps->a = a;
        for (ps->nslot = 64; ps->nslot < 2 * (size_t) nstripes; ps->nslot *= 2)
                ;
        ps->slot = (int32_t *) malloc(ps->nslot * sizeof(int32_t));
        ps->c = (unsigned char *) malloc((size_t) max_errs * k);
        ps->g = (unsigned char *) malloc(32 * (size_t) max_errs * k);
        if (!ps->slot || !ps->c || !ps->g)
                return ISAL_HIP_ENOMEM;
        memset(ps->slot, 0xff, ps->nslot * sizeof(int32_t));
        return ISAL_HIP_OK;
}

/* room for one more pattern whose tables take `dwords` */
static int
patset_grow(patset *ps, size_t dwords)
{
        if (ps->npat == ps->cap) {
                const int cap = ps->cap ? 2 * ps->cap : 16;
                unsigned char *keys = (unsigned char *) realloc(ps->keys, (size_t) cap * ps->kw);
                unsigned char *surv;
                uint32_t *off;
                if (!keys)
                        return ISAL_HIP_ENOMEM;
                ps->keys = keys;
                surv = (unsigned char *) realloc(ps->surv, (size_t) cap * ps->k);
                if (!surv)
                        return ISAL_HIP_ENOMEM;
                ps->surv = surv;
                off = (uint32_t *) realloc(ps->off, (size_t) cap * 4);
                if (!off)
                        return ISAL_HIP_ENOMEM;
                ps->off = off;
                ps->cap = cap;
        }
        if (ps->tbl_dwords + dwords > ps->tbl_cap) {
                size_t cap = ps->tbl_cap ? 2 * ps->tbl_cap : 16 * dwords;
                uint32_t *tbl;
                while (cap < ps->tbl_dwords + dwords)
                        cap *= 2;
                tbl = (uint32_t *) realloc(ps->tbl, cap * 4);
                if (!tbl)
                        return ISAL_HIP_ENOMEM;
                ps->tbl = tbl;
                ps->tbl_cap = cap;
        }
        return ISAL_HIP_OK;
}

/* Index of the pattern of the nerrs marked shards, adding it (recovery rows,
 * device table image) when new; a negative ISAL_HIP_E* code otherwise. */
static int
patset_find(patset *ps, int nerrs, const unsigned char *mark)
{
        unsigned char key[1 + MAX_SHARDS];
        const size_t dwords = isal_hip_tables_dwords(ps->k, nerrs);
        uint32_t h = 2166136261u;
        size_t at;
        int i, n = 1, r;
        memset(key, 0, (size_t) ps->kw);
        key[0] = (unsigned char) nerrs;
        for (i = 0; i < ps->m; i++)
                if (mark[i])
                        key[n++] = (unsigned char) i;
        for (i = 0; i < ps->kw; i++)
                h = (h ^ key[i]) * 16777619u;
        for (at = h & (ps->nslot - 1);; at = (at + 1) & (ps->nslot - 1)) {
                const int32_t p = ps->slot[at];
                if (p < 0)
                        break;
                if (!memcmp(ps->keys + (size_t) p * ps->kw, key, (size_t) ps->kw))
                        return p;
        }
        if ((ps->tbl_dwords + dwords) * 4 > ISAL_HIP_REPAIR_MAX_TABLE_BYTES)
                return ISAL_HIP_ENOMEM;
        if ((r = patset_grow(ps, dwords)) != ISAL_HIP_OK)
                return r;
        r = isal_hip_decode_matrix(ps->k, ps->m, ps->a, nerrs, key + 1, ps->c,
                                   ps->surv + (size_t) ps->npat * ps->k);
        if (r != ISAL_HIP_OK)
                return r;
        ec_init_tables(ps->k, nerrs, ps->c, ps->g);
        isal_hip_build_tables(ps->k, nerrs, ps->g, ps->tbl + ps->tbl_dwords);
        memcpy(ps->keys + (size_t) ps->npat * ps->kw, key, (size_t) ps->kw);
        ps->off[ps->npat] = (uint32_t) ps->tbl_dwords;
        ps->tbl_dwords += dwords;
        ps->slot[at] = ps->npat;
        return ps->npat++;
}

/* One stripe's step of both creates: its length and count, its erasure set,
 * its m shard pointers (non-NULL, 16-byte aligned), then its pattern, added
 * when new, into *pat (untouched for a stripe that lost nothing). The stripe
 * is named in *bad_stripe unless memory ran out, which is no stripe's fault. */
static int
stripe_pattern(patset *ps, long long s, int len, int nerrs, const unsigned char *errs, unsigned char *const *sh,
               int32_t *pat, int *bad_stripe)
{
        unsigned char mark[MAX_SHARDS];
        int n, ret = len < 0 || nerrs >= ps->kw ? ISAL_HIP_EINVAL : mark_errs(ps->m, nerrs, errs, mark);
        if (ret == ISAL_HIP_OK)
                ret = isal_hip_obj_ptr_row(NULL, sh, (size_t) ps->m);
        if (ret == ISAL_HIP_OK && nerrs) {
                if ((n = patset_find(ps, nerrs, mark)) < 0)
                        ret = n;
                else
                        *pat = n;
        }
        if (ret != ISAL_HIP_OK && ret != ISAL_HIP_ENOMEM && bad_stripe)
                *bad_stripe = (int) s;
        return ret;
}

/* One row of a pointer table: of the stripe's m shards sh, pattern p's k
 * survivors, then its nerrs destinations in ascending order. */
static void
pattern_row(uint64_t *hp, const patset *ps, int p, int nerrs, unsigned char *const *sh)
{
        int i;
        for (i = 0; i < ps->k; i++)
                hp[i] = (uint64_t) (uintptr_t) sh[ps->surv[(size_t) p * ps->k + i]];
        for (i = 0; i < nerrs; i++)
                hp[ps->k + i] = (uint64_t) (uintptr_t) sh[ps->keys[(size_t) p * ps->kw + 1 + i]];
}

static int
repair_upload(isal_hip_repair *r, const uint64_t *h_ptrs, const uint32_t *h_pat, const uint32_t *h_tbl)
{
        const size_t nstripes = (size_t) r->nstripes, stride = (size_t) (r->k + r->nerrs);
        int e;
        if (hipGetDevice(&r->device) != hipSuccess)
                return ISAL_HIP_EHIP;
        if ((e = isal_hip_obj_reach(h_ptrs, nstripes, stride, (size_t) r->len, NULL, r->device)) != ISAL_HIP_OK ||
            (e = isal_hip_obj_put(&r->d_ptrs, h_ptrs, nstripes * stride * 8, 0)) != ISAL_HIP_OK ||
            (e = isal_hip_obj_put(&r->d_pat, h_pat, nstripes * 4, 0)) != ISAL_HIP_OK)
                return e;
        return isal_hip_obj_put(&r->d_tbl, h_tbl, (size_t) r->npat * r->tbl_stride * 4, 0);
}

int
isal_hip_repair_create(isal_hip_repair **out, int len, int k, int m, const unsigned char *a, int nerrs,
                       int nstripes, const unsigned char *errs, unsigned char *const *shards,
                       int *bad_stripe)
{
        isal_hip_repair *r = NULL;
        patset ps;
        int32_t *s_pat = NULL;
        uint32_t *h_pat = NULL, *first = NULL;
        uint64_t *h_ptrs = NULL;
        long long s;
        int i, ret = ISAL_HIP_OK;
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

        ret = patset_init(&ps, k, m, a, nerrs, nstripes);
        s_pat = (int32_t *) malloc((size_t) nstripes * 4);
        if (ret == ISAL_HIP_OK && !s_pat)
                ret = ISAL_HIP_ENOMEM;
        if (ret != ISAL_HIP_OK)
                goto done;

        /* 1-2: validate every stripe, find its pattern, build new patterns' tables */
        for (s = 0; s < nstripes && ret == ISAL_HIP_OK; s++)
                ret = stripe_pattern(&ps, s, len, nerrs, errs + (size_t) s * nerrs, shards + (size_t) s * m, &s_pat[s],
                                     bad_stripe);
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
                const uint32_t p = (uint32_t) s_pat[s], row = first[p]++;
                pattern_row(h_ptrs + (size_t) row * stride, &ps, (int) p, nerrs, shards + (size_t) s * m);
                h_pat[row] = p;
        }
        r->len = len;
        r->k = k;
        r->nerrs = nerrs;
        r->nstripes = nstripes;
        r->npat = ps.npat;
        /* one count: pattern p's tables lie at p * tbl_stride */
        r->tbl_stride = (unsigned) isal_hip_tables_dwords(k, nerrs);
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

/* ---- the ragged create ---------------------------------------------------- */

/* whether some pass of a class of nerrs rows runs tiles of size t */
static int
class_uses(int nerrs, int t)
{
        const int small = isal_hip_uses_small_tile(nerrs);
        return t == TILE_SMALL ? small : nerrs >= EC_MAX_ROWS_PER_PASS || (nerrs % EC_MAX_ROWS_PER_PASS && !small);
}

/* the pieces of one class in the blob, as byte offsets */
enum { O_PTRS, O_ITEMS, O_ITEMS_SMALL, O_PAT, O_LENS, NPIECES };

static size_t
blob_take(size_t *at, size_t bytes)
{
        const size_t o = *at;
        *at += (bytes + 15) & ~(size_t) 15;
        return o;
}

static int
repair_upload_ragged(isal_hip_repair *r, const unsigned char *h_blob, size_t nblob, const size_t *offs,
                     const uint32_t *h_tbl, size_t ntbl)
{
        int c, t, e;
        if (hipGetDevice(&r->device) != hipSuccess)
                return ISAL_HIP_EHIP;
        /* a row's shards are as long as that row (no row here has length 0) */
        for (c = 0; c < r->nclass; c++) {
                const size_t *o = offs + c * NPIECES;
                if ((e = isal_hip_obj_reach((const uint64_t *) (h_blob + o[O_PTRS]), r->cls[c].nrows,
                                            (size_t) (r->k + r->cls[c].nerrs), 0, (const int *) (h_blob + o[O_LENS]),
                                            r->device)) != ISAL_HIP_OK)
                        return e;
        }
        if (!nblob)
                return ISAL_HIP_OK;
        if ((e = isal_hip_obj_put(&r->d_blob, h_blob, nblob, 0)) != ISAL_HIP_OK ||
            (e = isal_hip_obj_put(&r->d_tbl, h_tbl, ntbl, 0)) != ISAL_HIP_OK)
                return e;
        for (c = 0; c < r->nclass; c++) {
                rclass *cl = &r->cls[c];
                const size_t *o = offs + c * NPIECES;
                cl->d_ptrs = (uint64_t *) (r->d_blob + o[O_PTRS]);
                cl->d_pat = (uint32_t *) (r->d_blob + o[O_PAT]);
                cl->d_lens = (int *) (r->d_blob + o[O_LENS]);
                for (t = 0; t < NTILES; t++)
                        if (cl->nitems[t])
                                cl->d_items[t] = (unsigned *) (r->d_blob + o[O_ITEMS + t]);
        }
        return ISAL_HIP_OK;
}

int
isal_hip_repair_create_ragged(isal_hip_repair **out, int k, int m, const unsigned char *a, int nstripes,
                              const int *lens, int max_errs, const unsigned char *nerrs, const unsigned char *errs,
                              unsigned char *const *shards, int *bad_stripe)
{
        isal_hip_repair *r = NULL;
        patset ps;
        unsigned cnt[MAX_SHARDS + 1], base[MAX_SHARDS + 1]; /* rows of each count, their first row */
        int32_t *s_pat = NULL;                              /* -1: a stripe that lost nothing */
        uint32_t *first = NULL, *ord = NULL, *rstripe = NULL;
        int *rlens = NULL;
        size_t *offs = NULL, nblob = 0;
        unsigned char *h_blob = NULL;
        unsigned nrows = 0, row;
        long long s, n;
        int i, c, t, ret;

        if (bad_stripe)
                *bad_stripe = -1;
        if (!out)
                return ISAL_HIP_EINVAL;
        *out = NULL;
        if (k < 1 || m <= k || m > MAX_SHARDS || !a || nstripes < 1 || !lens || max_errs < 1 || max_errs > m - k ||
            !nerrs || !errs || !shards)
                return ISAL_HIP_EINVAL;

        ret = patset_init(&ps, k, m, a, max_errs, nstripes);
        s_pat = (int32_t *) malloc((size_t) nstripes * 4);
        if (ret == ISAL_HIP_OK && !s_pat)
                ret = ISAL_HIP_ENOMEM;
        if (ret != ISAL_HIP_OK)
                goto done;

        /* 1-2: validate every stripe, find its pattern, build new patterns'
         * tables; a stripe that lost nothing or is empty is held to the same
         * contract */
        memset(cnt, 0, sizeof(cnt));
        for (s = 0; s < nstripes && ret == ISAL_HIP_OK; s++) {
                s_pat[s] = -1;
                ret = stripe_pattern(&ps, s, lens[s], nerrs[s], errs + (size_t) s * max_errs, shards + (size_t) s * m,
                                     &s_pat[s], bad_stripe);
                if (ret == ISAL_HIP_OK && nerrs[s] && lens[s] > 0)
                        cnt[nerrs[s]]++;
        }
        if (ret != ISAL_HIP_OK)
                goto done;

        r = (isal_hip_repair *) calloc(1, sizeof(*r));
        if (!r) {
                ret = ISAL_HIP_ENOMEM;
                goto done;
        }
        r->ragged = 1;
        r->k = k;
        r->nstripes = nstripes;
        r->npat = ps.npat;
        for (c = 1; c <= max_errs; c++) {
                base[c] = nrows;
                nrows += cnt[c];
                r->nclass += cnt[c] != 0;
        }

        /* 3: the rows of all classes, class after class, each class sorted by
         * pattern (a counting sort by pattern, then a stable split by count) */
        first = (uint32_t *) calloc((size_t) ps.npat + 1, 4);
        ord = (uint32_t *) malloc(((size_t) nrows + 1) * 4);
        rstripe = (uint32_t *) malloc(((size_t) nrows + 1) * 4);
        rlens = (int *) malloc(((size_t) nrows + 1) * sizeof(int));
        r->cls = (rclass *) calloc((size_t) r->nclass + 1, sizeof(rclass));
        offs = (size_t *) calloc((size_t) r->nclass + 1, NPIECES * sizeof(size_t));
        if (!first || !ord || !rstripe || !rlens || !r->cls || !offs) {
                ret = ISAL_HIP_ENOMEM;
                goto done;
        }
        for (s = 0; s < nstripes; s++)
                if (s_pat[s] >= 0 && lens[s] > 0)
                        first[s_pat[s] + 1]++;
        for (i = 0; i < ps.npat; i++)
                first[i + 1] += first[i];
        for (s = 0; s < nstripes; s++)
                if (s_pat[s] >= 0 && lens[s] > 0)
                        ord[first[s_pat[s]]++] = (uint32_t) s;
        for (row = 0; row < nrows; row++) {
                const uint32_t st = ord[row], at = base[nerrs[st]]++;
                rstripe[at] = st;
                rlens[at] = lens[st];
        }

        /* the classes present, their item counts against the launch limit at
         * the smallest tile each one uses, and their places in the blob */
        for (c = 1, i = 0; c <= max_errs; c++) {
                rclass *cl = &r->cls[i];
                const int *cl_lens = rlens + (base[c] - cnt[c]);
                if (!cnt[c])
                        continue;
                cl->nerrs = c;
                cl->nrows = cnt[c];
                for (t = 0; t < NTILES; t++) {
                        if (!class_uses(c, t))
                                continue;
                        n = isal_hip_ragged_items((int) cl->nrows, cl_lens, isal_hip_tile_bytes(t), NULL);
                        if (n > (long long) ISAL_HIP_RAGGED_MAX_ITEMS) {
                                ret = ISAL_HIP_EINVAL;
                                goto done;
                        }
                        cl->nitems[t] = (unsigned) n;
                }
                offs[i * NPIECES + O_PTRS] = blob_take(&nblob, (size_t) cl->nrows * (size_t) (k + c) * 8);
                for (t = 0; t < NTILES; t++)
                        offs[i * NPIECES + O_ITEMS + t] = blob_take(&nblob, (size_t) cl->nitems[t] * 8);
                offs[i * NPIECES + O_PAT] = blob_take(&nblob, (size_t) cl->nrows * 4);
                offs[i * NPIECES + O_LENS] = blob_take(&nblob, (size_t) cl->nrows * sizeof(int));
                i++;
        }

        h_blob = (unsigned char *) calloc(nblob ? nblob : 1, 1);
        if (!h_blob) {
                ret = ISAL_HIP_ENOMEM;
                goto done;
        }
        for (c = 0; c < r->nclass; c++) {
                const rclass *cl = &r->cls[c];
                const size_t *o = offs + c * NPIECES, stride = (size_t) (k + cl->nerrs);
                const unsigned row0 = base[cl->nerrs] - cl->nrows;
                uint64_t *hp = (uint64_t *) (h_blob + o[O_PTRS]);
                uint32_t *h_pat = (uint32_t *) (h_blob + o[O_PAT]);
                /* k survivors then the destinations in ascending order */
                for (row = 0; row < cl->nrows; row++, hp += stride) {
                        const uint32_t st = rstripe[row0 + row];
                        pattern_row(hp, &ps, s_pat[st], cl->nerrs, shards + (size_t) st * m);
                        h_pat[row] = ps.off[s_pat[st]];
                }
                memcpy(h_blob + o[O_LENS], rlens + row0, (size_t) cl->nrows * sizeof(int));
                for (t = 0; t < NTILES; t++)
                        if (cl->nitems[t])
                                (void) isal_hip_ragged_items((int) cl->nrows, rlens + row0, isal_hip_tile_bytes(t),
                                                             (unsigned *) (h_blob + o[O_ITEMS + t]));
        }
        ret = repair_upload_ragged(r, h_blob, nblob, offs, ps.tbl, ps.tbl_dwords * 4);
done:
        patset_free(&ps);
        free(s_pat);
        free(first);
        free(ord);
        free(rstripe);
        free(rlens);
        free(offs);
        free(h_blob);
        if (ret != ISAL_HIP_OK) {
                isal_hip_repair_destroy(r);
                return ret;
        }
        *out = r;
        return ISAL_HIP_OK;
}

static int
repair_run_ragged(isal_hip_repair *r, void *stream)
{
        int c;
        for (c = 0; c < r->nclass; c++) {
                const rclass *cl = &r->cls[c];
                if (isal_hip_launch_repair_ragged(cl->d_ptrs, r->k + cl->nerrs, cl->d_pat, r->d_tbl, cl->d_lens,
                                                  cl->d_items[TILE_BIG], cl->nitems[TILE_BIG], cl->d_items[TILE_SMALL],
                                                  cl->nitems[TILE_SMALL], r->k, cl->nerrs, stream))
                        return ISAL_HIP_EHIP;
        }
        return ISAL_HIP_OK;
}

static int
repair_run_impl(isal_hip_repair *r, void *stream)
{
        if (r->ragged)
                return repair_run_ragged(r, stream);
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
        isal_hip_obj_drop(r->d_ptrs);
        isal_hip_obj_drop(r->d_pat);
        isal_hip_obj_drop(r->d_tbl);
        isal_hip_obj_drop(r->d_blob);
        free(r->cls);
        free(r);
        return ISAL_HIP_OK;
}
