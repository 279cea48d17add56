/*
 * overwrite_ragged_host.c — TEST INFRASTRUCTURE: the ragged overwrite's host
 * logic (isa-l_amd/csrc/isal_hip_overwrite.c isal_hip_overwrite_create_ragged:
 * the per-stripe count, index, pointer and overlap checks over the live slots,
 * the tables at stride max_nw with zeroed padding, the lengths, the counts and
 * the item table) under ASan + UBSan, as a stand-alone program.
 *
 * The HIP runtime (hip_stubs.c) and the kernel launchers (below) are stubs
 * ("device" memory is host memory), so the program needs no GPU and what
 * create() uploads can be read back: the launch stub applies every item's
 * delta on the CPU from the pointer, index, length, count, item and
 * coefficient tables it is handed and nothing else; the driver compares the
 * parity with a fresh encode of the stripe with the new bytes in place. Every
 * shard is an allocation of exactly its stripe's length, so a table that
 * reaches past a stripe's own length, or a padded slot that is dereferenced,
 * is an ASan report.
 *
 * Built by this directory's Makefile (make -C tests/sanitize) and run by
 * tests/test_sanitizers_cpu.py; the stubs every such program shares are in
 * hip_stubs.c.
 */
#include <limits.h>

#include "hip_stubs.h"

/* ---- stubs: the launchers this program drives ------------------------------ */

static int g_launches, g_commits;
static unsigned g_items;

/* Every item folds its 2 KiB tile of its stripe's live slots into every row,
 * bounded by the stripe's own length; commit then stores new over old. */
int
isal_hip_launch_overwrite_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_idx, const uint32_t *d_tbl,
                                 const int *d_lens, const int *d_nw, const unsigned *d_items, unsigned nitems, int k,
                                 int rows, int max_nw, int commit, void *stream)
{
        const long long tile = ISAL_HIP_RAGGED_TILE_SMALL;
        unsigned w;
        int i, l;
        (void) stream;
        CHECK(ptr_stride == 2 * max_nw + rows);
        if (!nitems)
                return 0;
        CHECK(d_items);
        g_launches += (rows + EC_MAX_ROWS_PER_PASS - 1) / EC_MAX_ROWS_PER_PASS;
        g_commits += commit != 0;
        g_items = nitems;
        for (w = 0; w < nitems; w++) {
                const unsigned s = d_items[2 * w];
                const long long b0 = d_items[2 * w + 1] * tile;
                const int len = d_lens[s], nw = d_nw[s];
                const long long b1 = b0 + tile < len ? b0 + tile : len;
                const uint64_t *sp = d_ptrs + (size_t) s * ptr_stride;
                const uint32_t *ip = d_idx + (size_t) s * max_nw;
                long long b;
                CHECK(nw > 0 && nw <= max_nw && b0 < len);
                if (w) /* the tiles of one stripe in turn, stripes ascending */
                        CHECK(d_items[2 * w - 2] == s ? d_items[2 * w - 1] + 1 == d_items[2 * w + 1]
                                                      : d_items[2 * w - 2] < s && d_items[2 * w + 1] == 0);
                for (i = nw; i < max_nw; i++) /* padding is zero, whatever the caller put there */
                        CHECK(!sp[i] && !sp[max_nw + i] && !ip[i]);
                for (i = 0; i < nw; i++) {
                        unsigned char *o = (unsigned char *) (uintptr_t) sp[i];
                        const unsigned char *n = (const unsigned char *) (uintptr_t) sp[max_nw + i];
                        const int j = (int) ip[i];
                        CHECK(j < k);
                        for (l = 0; l < rows; l++) {
                                unsigned char *dst = (unsigned char *) (uintptr_t) sp[2 * max_nw + l];
                                const unsigned char c = coef_of(d_tbl, k, rows, l, j);
                                for (b = b0; b < b1; b++)
                                        dst[b] ^= gf_mul(c, (unsigned char) (o[b] ^ n[b]));
                        }
                        if (commit)
                                memcpy(o + b0, n + b0, (size_t) (b1 - b0));
                }
        }
        return 0;
}

/* ---- the driver ----------------------------------------------------------- */

/* parity[l] of data[0..k) for the m x k matrix a, into out[l] */
static void
encode(const unsigned char *a, int k, int rows, int len, unsigned char **data, unsigned char **out)
{
        int l, j, b;
        for (l = 0; l < rows; l++)
                for (b = 0; b < len; b++) {
                        unsigned char v = 0;
                        for (j = 0; j < k; j++)
                                v ^= gf_mul(a[(size_t) (k + l) * k + j], data[j][b]);
                        out[l][b] = v;
                }
}

/* A window of nstripes stripes, stripe s with lens[s] bytes and nws[s] of
 * max_nw slots; the unused slots hold index 255, NULL (old) and an unaligned
 * address that is no memory (new). */
static void
run_window(int cauchy, int k, int rows, int max_nw, int nstripes, const int *lens, const int *nws)
{
        const int m = k + rows, passes = (rows + EC_MAX_ROWS_PER_PASS - 1) / EC_MAX_ROWS_PER_PASS;
        unsigned char *a = malloc((size_t) m * k), *g = malloc(32 * (size_t) k * rows);
        unsigned char *idx = malloc((size_t) nstripes * max_nw);
        unsigned char **data = malloc(sizeof(*data) * (size_t) nstripes * k);
        unsigned char **par = malloc(sizeof(*par) * (size_t) nstripes * rows);
        unsigned char **par0 = malloc(sizeof(*par0) * (size_t) nstripes * rows);
        unsigned char **want = malloc(sizeof(*want) * (size_t) rows);
        unsigned char **nd = malloc(sizeof(*nd) * (size_t) nstripes * max_nw);
        unsigned char **od = malloc(sizeof(*od) * (size_t) nstripes * max_nw);
        unsigned char **cur = malloc(sizeof(*cur) * (size_t) k);
        isal_hip_overwrite *o = NULL;
        long long items = 0;
        int s, i, j, b, l, bad = -9, live = 0, allocs0 = g_allocs;
        CHECK(a && g && idx && data && par && par0 && want && nd && od && cur);
        if (cauchy)
                gf_gen_cauchy1_matrix(a, m, k);
        else
                gf_gen_rs_matrix(a, m, k);
        ec_init_tables(k, rows, a + (size_t) k * k, g);
        for (s = 0; s < nstripes; s++) {
                const int len = lens[s];
                for (j = 0; j < k; j++) {
                        data[s * k + j] = shard(len);
                        for (b = 0; b < len; b++)
                                data[s * k + j][b] = (unsigned char) rnd(256);
                }
                for (l = 0; l < rows; l++) {
                        par[s * rows + l] = shard(len);
                        par0[s * rows + l] = shard(len);
                }
                encode(a, k, rows, len, data + s * k, par + s * rows);
                for (l = 0; l < rows; l++)
                        memcpy(par0[s * rows + l], par[s * rows + l], (size_t) len);
                /* nws[s] distinct indices in a random order, then the padding */
                for (i = 0; i < max_nw; i++) {
                        unsigned char *x = idx + s * max_nw + i;
                        if (i >= nws[s]) {
                                *x = 255;
                                od[s * max_nw + i] = NULL;
                                nd[s * max_nw + i] = (unsigned char *) (uintptr_t) 7;
                                continue;
                        }
                        do {
                                *x = (unsigned char) rnd((unsigned) k);
                                for (j = 0; j < i && idx[s * max_nw + j] != *x; j++)
                                        ;
                        } while (j < i);
                        od[s * max_nw + i] = data[s * k + *x];
                        nd[s * max_nw + i] = shard(len);
                        for (b = 0; b < len; b++)
                                nd[s * max_nw + i][b] = (unsigned char) rnd(256);
                }
                if (len > 0 && nws[s] > 0) {
                        live++;
                        items += (len + ISAL_HIP_RAGGED_TILE_SMALL - 1) / ISAL_HIP_RAGGED_TILE_SMALL;
                }
        }
        CHECK(isal_hip_overwrite_create_ragged(&o, k, rows, g, nstripes, lens, max_nw, nws, idx, od, nd, par, &bad) ==
              ISAL_HIP_OK);
        CHECK(o && bad == -1);
        CHECK(g_allocs - allocs0 == 5 + (items > 0)); /* no item table when nothing is to do */
        CHECK(isal_hip_overwrite_run(o, 2, NULL) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_overwrite_run(o, ~0, NULL) == ISAL_HIP_EINVAL);
        /* twice without commit: the parity comes back, the data never moved */
        g_launches = g_commits = 0;
        g_items = 0;
        CHECK(isal_hip_overwrite_run(o, 0, NULL) == ISAL_HIP_OK);
        CHECK(g_items == (unsigned) items);
        CHECK(isal_hip_overwrite_run(o, 0, NULL) == ISAL_HIP_OK);
        CHECK(g_launches == (live ? 2 * passes : 0) && g_commits == 0);
        for (i = 0; i < nstripes * rows; i++)
                CHECK(memcmp(par[i], par0[i], (size_t) lens[i / rows]) == 0);
        /* committed, twice: the parity of the stripe with the new bytes in place */
        CHECK(isal_hip_overwrite_run(o, ISAL_HIP_OVERWRITE_COMMIT, NULL) == ISAL_HIP_OK);
        CHECK(isal_hip_overwrite_run(o, ISAL_HIP_OVERWRITE_COMMIT, NULL) == ISAL_HIP_OK);
        CHECK(g_commits == (live ? 2 : 0));
        for (s = 0; s < nstripes; s++) {
                const int len = lens[s];
                for (j = 0; j < k; j++)
                        cur[j] = data[s * k + j];
                for (i = 0; i < nws[s]; i++) {
                        cur[idx[s * max_nw + i]] = nd[s * max_nw + i];
                        CHECK(memcmp(od[s * max_nw + i], nd[s * max_nw + i], (size_t) len) == 0);
                }
                for (l = 0; l < rows; l++)
                        want[l] = shard(len);
                encode(a, k, rows, len, cur, want);
                for (l = 0; l < rows; l++) {
                        CHECK(memcmp(par[s * rows + l], want[l], (size_t) len) == 0);
                        free(want[l]);
                }
        }
        CHECK(isal_hip_overwrite_destroy(o) == ISAL_HIP_OK);
        CHECK(g_allocs == allocs0);
        printf("  %s k=%d rows=%d max_nw=%d stripes=%d (%d live, %lld items): %d pass(es), parity as a fresh encode\n",
               cauchy ? "cauchy" : "rs", k, rows, max_nw, nstripes, live, items, passes);
        for (i = 0; i < nstripes * k; i++)
                free(data[i]);
        for (i = 0; i < nstripes * rows; i++) {
                free(par[i]);
                free(par0[i]);
        }
        for (s = 0; s < nstripes; s++)
                for (i = 0; i < nws[s]; i++)
                        free(nd[s * max_nw + i]);
        free(a);
        free(g);
        free(idx);
        free(data);
        free(par);
        free(par0);
        free(want);
        free(nd);
        free(od);
        free(cur);
}

static void
error_paths(void)
{
        enum { K = 10, R = 4, MW = 3, S = 6, LEN = 64, N = S * (2 * MW + R) };
        static const int lens0[S] = { LEN, 16, 0, LEN, 48, LEN }, nw0[S] = { 3, 1, 2, 0, 2, 3 };
        unsigned char a[(K + R) * K], g[32 * K * R], idx[S * MW];
        unsigned char *buf, *od[S * MW], *nd[S * MW], *cd[S * R], *keep;
        int lens[S], nw[S];
        isal_hip_overwrite *o;
        int s, i, bad, n = 0;
        CHECK(posix_memalign((void **) &buf, 16, (size_t) N * LEN) == 0);
        gf_gen_rs_matrix(a, K + R, K);
        ec_init_tables(K, R, a + K * K, g);
        memcpy(lens, lens0, sizeof(lens));
        memcpy(nw, nw0, sizeof(nw));
        for (s = 0; s < S; s++) {
                for (i = 0; i < MW; i++) {
                        const int used = i < nw[s];
                        idx[s * MW + i] = used ? (unsigned char) ((s + 3 * i) % K) : 255;
                        od[s * MW + i] = used ? buf + (size_t) LEN * n++ : NULL;
                        nd[s * MW + i] = used ? buf + (size_t) LEN * n++ : (unsigned char *) (uintptr_t) 9;
                }
                for (i = 0; i < R; i++)
                        cd[s * R + i] = buf + (size_t) LEN * n++;
        }
#define CREATE(k, rows, g_, ns, ln, mw, nw_, ix, o_, n_, c_) \
        (o = (isal_hip_overwrite *) buf, bad = -9,           \
         isal_hip_overwrite_create_ragged(&o, k, rows, g_, ns, ln, mw, nw_, ix, o_, n_, c_, &bad))
#define REFUSED(expr, stripe) CHECK((expr) == ISAL_HIP_EINVAL && o == NULL && bad == (stripe))
#define ACCEPTED(expr) \
        CHECK((expr) == ISAL_HIP_OK && o && bad == -1 && isal_hip_overwrite_destroy(o) == ISAL_HIP_OK)
        /* arguments */
        CHECK(isal_hip_overwrite_create_ragged(NULL, K, R, g, S, lens, MW, nw, idx, od, nd, cd, &bad) ==
              ISAL_HIP_EINVAL);
        REFUSED(CREATE(K, R, NULL, S, lens, MW, nw, idx, od, nd, cd), -1);
        REFUSED(CREATE(K, R, g, S, NULL, MW, nw, idx, od, nd, cd), -1);
        REFUSED(CREATE(K, R, g, S, lens, MW, NULL, idx, od, nd, cd), -1);
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, NULL, od, nd, cd), -1);
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, idx, NULL, nd, cd), -1);
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, idx, od, NULL, cd), -1);
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, NULL), -1);
        REFUSED(CREATE(K, R, g, 0, lens, MW, nw, idx, od, nd, cd), -1);
        REFUSED(CREATE(0, R, g, S, lens, MW, nw, idx, od, nd, cd), -1);
        REFUSED(CREATE(257, R, g, S, lens, MW, nw, idx, od, nd, cd), -1);
        REFUSED(CREATE(K, 0, g, S, lens, MW, nw, idx, od, nd, cd), -1);
        REFUSED(CREATE(K, R, g, S, lens, 0, nw, idx, od, nd, cd), -1);
        REFUSED(CREATE(K, R, g, S, lens, K + 1, nw, idx, od, nd, cd), -1);
        /* lengths and counts; the first offender wins */
        lens[4] = -1;
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd), 4);
        nw[1] = MW + 1;
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd), 1);
        nw[1] = -1;
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd), 1);
        nw[1] = nw0[1];
        lens[4] = lens0[4];
        /* indices among the live slots only */
        idx[4 * MW + 1] = K;
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd), 4);
        idx[2 * MW + 1] = idx[2 * MW + 0]; /* a duplicate in stripe 2 (length 0) comes first */
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd), 2);
        idx[2 * MW + 1] = (unsigned char) ((2 + 3) % K);
        idx[4 * MW + 1] = (unsigned char) ((4 + 3) % K);
        idx[1 * MW + 2] = idx[1 * MW + 0]; /* a padded slot may repeat a live index */
        ACCEPTED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd));
        /* pointers among the live ones only, empty stripes included */
        keep = nd[5 * MW + 1];
        nd[5 * MW + 1] = keep + 8;
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd), 5);
        nd[5 * MW + 1] = NULL;
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd), 5);
        nd[5 * MW + 1] = keep;
        keep = od[2 * MW + 0];
        od[2 * MW + 0] = NULL; /* stripe 2 has length 0 */
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd), 2);
        od[2 * MW + 0] = keep;
        keep = cd[3 * R + 2];
        cd[3 * R + 2] = keep + 4; /* stripe 3 has no slot */
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd), 3);
        cd[3 * R + 2] = keep;
        /* overlaps over the stripe's own length */
        keep = nd[0 * MW + 1];
        nd[0 * MW + 1] = cd[0 * R + 2]; /* new aliases a parity row */
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd), 0);
        nd[0 * MW + 1] = keep;
        keep = cd[4 * R + 0];
        cd[4 * R + 0] = od[4 * MW + 1] + 32; /* inside old's 48 bytes */
        REFUSED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd), 4);
        lens[4] = 32; /* ... which only touches a 32-byte range */
        ACCEPTED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd));
        lens[4] = lens0[4];
        cd[4 * R + 0] = keep;
        keep = cd[2 * R + 0];
        cd[2 * R + 0] = od[2 * MW + 1]; /* equal pointers at length 0 */
        ACCEPTED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd));
        cd[2 * R + 0] = keep;
        /* everything put back */
        ACCEPTED(CREATE(K, R, g, S, lens, MW, nw, idx, od, nd, cd));
        CHECK(isal_hip_overwrite_run(NULL, 0, NULL) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_overwrite_destroy(NULL) == ISAL_HIP_OK);
        free(buf);
        printf("  error paths: ok\n");
}

/* More than 2^30 items at the 2 KiB tile: 1025 stripes of INT_MAX bytes that
 * share one row of never-dereferenced addresses 4 GiB apart. */
static void
item_limit(void)
{
        enum { K = 4, R = 2, S = 1025 };
        unsigned char a[(K + R) * K], g[32 * K * R];
        unsigned char *idx = malloc(S), **od = malloc(sizeof(*od) * S), **nd = malloc(sizeof(*nd) * S);
        unsigned char **cd = malloc(sizeof(*cd) * S * R);
        int *lens = malloc(sizeof(int) * S), *nw = malloc(sizeof(int) * S);
        isal_hip_overwrite *o = (isal_hip_overwrite *) g;
        int s, bad = -9, allocs0 = g_allocs;
        CHECK(idx && od && nd && cd && lens && nw);
        gf_gen_rs_matrix(a, K + R, K);
        ec_init_tables(K, R, a + K * K, g);
        for (s = 0; s < S; s++) {
                idx[s] = (unsigned char) (s % K);
                lens[s] = INT_MAX;
                nw[s] = 1;
                od[s] = (unsigned char *) (uintptr_t) (1ull << 40);
                nd[s] = (unsigned char *) (uintptr_t) (2ull << 40);
                cd[s * R] = (unsigned char *) (uintptr_t) (3ull << 40);
                cd[s * R + 1] = (unsigned char *) (uintptr_t) (4ull << 40);
        }
        CHECK(isal_hip_overwrite_create_ragged(&o, K, R, g, S, lens, 1, nw, idx, od, nd, cd, &bad) == ISAL_HIP_EINVAL);
        CHECK(o == NULL && bad == -1 && g_allocs == allocs0);
        free(idx);
        free(od);
        free(nd);
        free(cd);
        free(lens);
        free(nw);
        printf("  item limit: ok\n");
}

int
main(void)
{
        static const int lens_a[] = { 0, 1, 15, 16, 17, 2047, 2048, 2049, 4097, 37 };
        static const int nw_a[] = { 2, 1, 3, 0, 2, 1, 3, 2, 1, 3 };
        static const int lens_b[] = { 21, 2049, 5, 64, 4096, 33 };
        static const int nw_b[] = { 1, 2, 1, 2, 1, 2 };
        static const int lens_c[] = { 33, 0, 2100 };
        static const int nw_c[] = { 6, 6, 1 }; /* nw = k */
        static const int lens_d[] = { 0, 19, 0, 64 };
        static const int nw_d[] = { 2, 0, 0, 0 }; /* nothing to do */
        printf("overwrite_ragged_host: isal_hip_overwrite_create_ragged host logic with stubbed HIP\n");
        error_paths();
        item_limit();
        run_window(0, 10, 4, 3, 10, lens_a, nw_a);
        run_window(1, 20, 10, 2, 6, lens_b, nw_b); /* two passes */
        run_window(0, 6, 3, 6, 3, lens_c, nw_c);
        run_window(0, 4, 2, 2, 4, lens_d, nw_d);
        printf("overwrite_ragged_host: ok\n");
        return 0;
}
