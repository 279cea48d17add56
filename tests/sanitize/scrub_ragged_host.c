/*
 * scrub_ragged_host.c — TEST INFRASTRUCTURE: the ragged scrub's host logic
 * (isa-l_amd/csrc/isal_hip_scrub.c: isal_hip_scrub_create_ragged's refusals
 * and their order, the pointer, coefficient, location, length and work-item
 * tables, the run of both kinds of object) under ASan + UBSan, as a
 * stand-alone program.
 *
 * The HIP runtime (hip_stubs.c) and the kernel launchers (below) are stubs
 * ("device" memory is host memory), so the program needs no GPU and the
 * tables create() uploads can be read back. The launch stub takes every work
 * item from the uploaded item table, checks that the items are the tiles of
 * stripe 0, then of stripe 1, ... with none for a stripe of length 0, and
 * reads each item's byte columns up to the stripe's own uploaded length only:
 * every shard is an allocation of exactly its stripe's length, so a table
 * that sent an item past it would be an ASan report. The shard is named from
 * the location tables alone, as the kernel's mismatch branch does; the driver
 * compares the verdicts with the corruption it planted.
 *
 * Built by this directory's Makefile (make -C tests/sanitize) and run by
 * tests/test_sanitizers_cpu.py; the stubs every such program shares are in
 * hip_stubs.c.
 */
#include "hip_stubs.h"

/* ---- stubs: the launchers this program drives ------------------------------ */

static int g_launches;

/* the mismatch branch, from the location tables alone */
static unsigned
name_shard(const unsigned char *loc, int k, int rows, const unsigned char *e)
{
        const unsigned char *piv = loc + (size_t) rows * k, *inv = piv + k;
        int j, l, nz = 0, last = -1;
        for (j = 0; j < k; j++) {
                unsigned char d;
                if (piv[j] >= rows)
                        continue;
                d = gf_mul(e[piv[j]], inv[j]);
                if (!d)
                        continue;
                for (l = 0; l < rows && gf_mul(loc[(size_t) l * k + j], d) == e[l]; l++)
                        ;
                if (l == rows)
                        return (unsigned) j;
        }
        for (l = 0; l < rows; l++)
                if (e[l]) {
                        nz++;
                        last = l;
                }
        return nz == 1 ? (unsigned) (k + last) : ISAL_HIP_SCRUB_MULTI;
}

/* byte columns [b0, b1) of one pointer row folded into *w */
static void
locate_columns(const uint64_t *sp, const uint32_t *d_tbl, const unsigned char *d_loc, int k, int rows, long long b0,
               long long b1, unsigned *w)
{
        long long b;
        int l, j;
        for (b = b0; b < b1; b++) {
                unsigned char e[EC_MAX_ROWS_PER_PASS];
                unsigned v, any = 0;
                for (l = 0; l < rows; l++) {
                        e[l] = ((const unsigned char *) (uintptr_t) sp[k + l])[b];
                        for (j = 0; j < k; j++)
                                e[l] ^= gf_mul(coef_of(d_tbl, k, rows, l, j), ((const unsigned char *) (uintptr_t) sp[j])[b]);
                        any |= e[l];
                }
                if (!any)
                        continue;
                v = name_shard(d_loc, k, rows, e);
                if (*w == ISAL_HIP_SCRUB_CLEAN)
                        *w = v;
                else if (*w != v)
                        *w = ISAL_HIP_SCRUB_MULTI;
        }
}

/* the uniform object's launcher: one len */
int
isal_hip_launch_locate_batch(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_tbl, int len, int k, int rows,
                             long long nstripes, const isal_hip_encmask *em, const unsigned char *d_loc,
                             unsigned *verdict, void *stream)
{
        long long s;
        (void) stream;
        if (len <= 0)
                return 0;
        g_launches++;
        CHECK(ptr_stride == k + rows && em && rows <= EC_MAX_ROWS_PER_PASS);
        for (s = 0; s < nstripes; s++) {
                verdict[s] = ISAL_HIP_SCRUB_CLEAN;
                locate_columns(d_ptrs + s * ptr_stride, d_tbl, d_loc, k, rows, 0, len, &verdict[s]);
        }
        return 0;
}

int
isal_hip_launch_locate_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_tbl, const int *d_lens,
                              const unsigned *d_items, unsigned nitems, int k, int rows, long long nstripes,
                              const unsigned char *d_loc, unsigned *verdict, void *stream)
{
        long long s;
        unsigned w = 0, t;
        int l, j;
        (void) stream;
        if (nitems == 0)
                return 0;
        g_launches++;
        CHECK(ptr_stride == k + rows && rows >= 2 && rows <= EC_MAX_ROWS_PER_PASS && d_items && d_lens);
        for (l = 0; l < rows; l++)
                for (j = 0; j < k; j++)
                        CHECK(d_loc[(size_t) l * k + j] == coef_of(d_tbl, k, rows, l, j));
        for (s = 0; s < nstripes; s++)
                verdict[s] = ISAL_HIP_SCRUB_CLEAN;
        /* the items: every tile of every stripe once, in stripe order, none past a length */
        for (s = 0; s < nstripes; s++) {
                const unsigned tiles = (unsigned) (((long long) d_lens[s] + ISAL_HIP_RAGGED_TILE - 1) / ISAL_HIP_RAGGED_TILE);
                for (t = 0; t < tiles; t++, w++) {
                        const long long b0 = (long long) t * ISAL_HIP_RAGGED_TILE;
                        const long long b1 = b0 + ISAL_HIP_RAGGED_TILE < d_lens[s] ? b0 + ISAL_HIP_RAGGED_TILE : d_lens[s];
                        CHECK(w < nitems && d_items[2 * w] == (unsigned) s && d_items[2 * w + 1] == t);
                        locate_columns(d_ptrs + s * ptr_stride, d_tbl, d_loc, k, rows, b0, b1, &verdict[s]);
                }
        }
        CHECK(w == nitems);
        return 0;
}

/* ---- the driver ----------------------------------------------------------- */

static void
make_tables(int cauchy, int k, int rows, unsigned char *a, unsigned char *g)
{
        if (cauchy)
                gf_gen_cauchy1_matrix(a, k + rows, k);
        else
                gf_gen_rs_matrix(a, k + rows, k);
        ec_init_tables(k, rows, a + (size_t) k * k, g);
}

/* nstripes stripes of the given lengths: live stripe number n has shard
 * n % (m + 2) corrupt in two places (m: clean, m + 1: two shards); the ragged
 * object's verdicts are as planted and equal a uniform object's per stripe */
static void
run_geometry(int cauchy, int k, int rows, int nstripes, const int *lens)
{
        const int m = k + rows;
        unsigned char *a = malloc((size_t) m * k), *g = malloc(32 * (size_t) k * rows);
        unsigned char **data = malloc(sizeof(*data) * (size_t) nstripes * k);
        unsigned char **par = malloc(sizeof(*par) * (size_t) nstripes * rows);
        unsigned *verdict = malloc(sizeof(*verdict) * (size_t) nstripes), *want = malloc(sizeof(*want) * (size_t) nstripes);
        isal_hip_scrub *sc = NULL, *one = NULL;
        int s, j, l, b, bad = -9, live = 0, n = 0, launches;
        CHECK(a && g && data && par && verdict && want);
        make_tables(cauchy, k, rows, a, g);
        for (s = 0; s < nstripes; s++) {
                const int len = lens[s];
                for (j = 0; j < k; j++) {
                        data[s * k + j] = shard(len);
                        for (b = 0; b < len; b++)
                                data[s * k + j][b] = (unsigned char) rnd(256);
                }
                for (l = 0; l < rows; l++) {
                        par[s * rows + l] = shard(len);
                        for (b = 0; b < len; b++) {
                                unsigned char v = 0;
                                for (j = 0; j < k; j++)
                                        v ^= gf_mul(a[(size_t) (k + l) * k + j], data[s * k + j][b]);
                                par[s * rows + l][b] = v;
                        }
                }
                want[s] = ISAL_HIP_SCRUB_CLEAN;
                if (len) {
                        const int i = n++ % (m + 2);
                        unsigned char **sh = i < k ? &data[s * k + i] : &par[s * rows + (i - k)];
                        live++;
                        if (i < m) {
                                if (len > 1)
                                        (*sh)[rnd((unsigned) len - 1)] ^= (unsigned char) (1 + rnd(255));
                                (*sh)[len - 1] ^= 0x80;
                                want[s] = (unsigned) i;
                        } else if (i == m + 1 && len > 1) {
                                data[s * k][0] ^= 1;
                                par[s * rows + 1][len - 1] ^= 1;
                                want[s] = ISAL_HIP_SCRUB_MULTI;
                        }
                }
                verdict[s] = 0x5a5a5a5au;
        }
        g_checks = 0;
        CHECK(isal_hip_scrub_create_ragged(&sc, k, rows, g, nstripes, lens, data, par, &bad) == ISAL_HIP_OK);
        CHECK(sc && bad == -1);
        /* reachability: one query per stripe with a length, over that length */
        CHECK(g_checks == live);
        for (s = 0, n = 0; s < nstripes; s++)
                if (lens[s] && n < 64)
                        CHECK(g_check_len[n++] == (size_t) lens[s]);
        CHECK(isal_hip_scrub_run(sc, NULL, NULL) == ISAL_HIP_EINVAL);
        launches = g_launches;
        CHECK(isal_hip_scrub_run(sc, verdict, NULL) == ISAL_HIP_OK);
        CHECK(g_launches - launches == (live ? 1 : 0));
        for (s = 0; s < nstripes; s++)
                CHECK(verdict[s] == (live ? want[s] : 0x5a5a5a5au));
        /* a second run gives the same words */
        CHECK(isal_hip_scrub_run(sc, verdict, NULL) == ISAL_HIP_OK);
        for (s = 0; s < nstripes; s++)
                CHECK(verdict[s] == (live ? want[s] : 0x5a5a5a5au));
        CHECK(isal_hip_scrub_destroy(sc) == ISAL_HIP_OK);
        /* the uniform object of each stripe alone */
        for (s = 0; s < nstripes; s++) {
                unsigned word = 0x5a5a5a5au;
                if (!lens[s])
                        continue;
                CHECK(isal_hip_scrub_create(&one, lens[s], k, rows, g, 1, data + s * k, par + s * rows, &bad) == ISAL_HIP_OK);
                CHECK(isal_hip_scrub_run(one, &word, NULL) == ISAL_HIP_OK && word == want[s]);
                CHECK(isal_hip_scrub_destroy(one) == ISAL_HIP_OK);
        }
        printf("  %s k=%d rows=%d stripes=%d (%d with a length): verdicts as planted\n", cauchy ? "cauchy" : "rs", k, rows,
               nstripes, live);
        for (s = 0; s < nstripes * k; s++)
                free(data[s]);
        for (s = 0; s < nstripes * rows; s++)
                free(par[s]);
        free(a);
        free(g);
        free(data);
        free(par);
        free(verdict);
        free(want);
}

static void
error_paths(void)
{
        enum { K = 10, R = 4, S = 6, LEN = 64 };
        unsigned char a[(K + R) * K], g[32 * K * R], amb[32 * 4 * 2], *buf;
        unsigned char *dd[S * K], *cd[S * R], *keep;
        static const unsigned char amb_c[8] = { 1, 1, 1, 2, 1, 2, 3, 4 }; /* column 3 = 2 * column 1 */
        unsigned char c[8];
        int lens[S] = { LEN, 0, 5, 16, LEN, 17 }, neg[S] = { LEN, 0, 5, -1, LEN, 17 };
        isal_hip_scrub *sc;
        int i, bad, calls;
        CHECK(posix_memalign((void **) &buf, 16, (size_t) S * (K + R) * LEN) == 0);
        make_tables(0, K, R, a, g);
        for (i = 0; i < S * K; i++)
                dd[i] = buf + (size_t) LEN * i;
        for (i = 0; i < S * R; i++)
                cd[i] = buf + (size_t) LEN * (S * K + i);
        calls = g_hip_calls;
#define CREATE(k, rows, g_, ns, l_, d_, c_) \
        (sc = (isal_hip_scrub *) buf, bad = -9, isal_hip_scrub_create_ragged(&sc, k, rows, g_, ns, l_, d_, c_, &bad))
#define REFUSED(expr, code, stripe) CHECK((expr) == (code) && sc == NULL && bad == (stripe) && g_hip_calls == calls)
        CHECK(isal_hip_scrub_create_ragged(NULL, K, R, g, S, lens, dd, cd, &bad) == ISAL_HIP_EINVAL);
        /* 1: counts and NULL arguments name no stripe, whatever the stripes hold */
        REFUSED(CREATE(K, R, NULL, S, lens, dd, cd), ISAL_HIP_EINVAL, -1);
        REFUSED(CREATE(K, R, g, S, NULL, dd, cd), ISAL_HIP_EINVAL, -1);
        REFUSED(CREATE(K, R, g, S, lens, NULL, cd), ISAL_HIP_EINVAL, -1);
        REFUSED(CREATE(K, R, g, S, lens, dd, NULL), ISAL_HIP_EINVAL, -1);
        REFUSED(CREATE(0, R, g, S, lens, dd, cd), ISAL_HIP_EINVAL, -1);
        REFUSED(CREATE(K, 1, g, S, neg, dd, cd), ISAL_HIP_EINVAL, -1);
        REFUSED(CREATE(K, 9, g, S, neg, dd, cd), ISAL_HIP_EINVAL, -1); /* refused before gftbls is read */
        REFUSED(CREATE(253, 4, g, S, lens, dd, cd), ISAL_HIP_EINVAL, -1);
        REFUSED(CREATE(K, R, g, 0, lens, dd, cd), ISAL_HIP_EINVAL, -1);
        /* 2: the first stripe with a bad length or pointer */
        REFUSED(CREATE(K, R, g, S, neg, dd, cd), ISAL_HIP_EINVAL, 3);
        keep = cd[1 * R + 1];
        cd[1 * R + 1] = keep + 8; /* misaligned, in stripe 1 of length 0: before the length of stripe 3 */
        REFUSED(CREATE(K, R, g, S, neg, dd, cd), ISAL_HIP_EINVAL, 1);
        cd[1 * R + 1] = NULL;
        REFUSED(CREATE(K, R, g, S, lens, dd, cd), ISAL_HIP_EINVAL, 1);
        cd[1 * R + 1] = keep;
        dd[4 * K] = NULL;
        REFUSED(CREATE(K, R, g, S, neg, dd, cd), ISAL_HIP_EINVAL, 3);
        REFUSED(CREATE(K, R, g, S, lens, dd, cd), ISAL_HIP_EINVAL, 4);
        /* 4: the ambiguous matrix after the stripes */
        memcpy(c, amb_c, 8);
        ec_init_tables(4, 2, c, amb);
        dd[4 * K] = buf + (size_t) LEN * 4 * K;
        keep = dd[2 * 4 + 1];
        dd[2 * 4 + 1] = NULL; /* stripe 2 of the 4 + 2 layout */
        REFUSED(CREATE(4, 2, amb, S, lens, dd, cd), ISAL_HIP_EINVAL, 2);
        dd[2 * 4 + 1] = keep;
        REFUSED(CREATE(4, 2, amb, S, neg, dd, cd), ISAL_HIP_EINVAL, 3);
        REFUSED(CREATE(4, 2, amb, S, lens, dd, cd), ISAL_HIP_ESINGULAR, -1);
        /* everything put back: accepted, and with every length 0 */
        CHECK(CREATE(K, R, g, S, lens, dd, cd) == ISAL_HIP_OK && sc && bad == -1 && g_hip_calls > calls);
        CHECK(isal_hip_scrub_destroy(sc) == ISAL_HIP_OK);
        memset(neg, 0, sizeof(neg));
        CHECK(CREATE(K, R, g, S, neg, dd, cd) == ISAL_HIP_OK && sc && bad == -1);
        CHECK(isal_hip_scrub_destroy(sc) == ISAL_HIP_OK);
#undef CREATE
#undef REFUSED
        free(buf);
        printf("  error paths: ok\n");
}

/* 3: the item limit, before the matrix and before any HIP call. k = 1, rows =
 * 2, every stripe 2^31 - 1 bytes (2^19 items); one pointer value repeated,
 * never dereferenced. With the ambiguous matrix (3, 0) 2048 stripes get past
 * the count to the matrix's refusal. */
static void
item_limit(void)
{
        enum { S = 2049 };
        static unsigned char *dd[S], *cd[2 * S];
        static int lens[S];
        unsigned char g[64] = { 0 };
        isal_hip_scrub *sc = NULL;
        int i, bad = -9, calls = g_hip_calls;
        for (i = 0; i < S; i++) {
                lens[i] = 0x7fffffff;
                dd[i] = cd[2 * i] = cd[2 * i + 1] = (unsigned char *) (uintptr_t) 0x7000000;
        }
        g[1] = 3;
        g[33] = 7;
        CHECK(isal_hip_ragged_items(S - 1, lens, ISAL_HIP_RAGGED_TILE, NULL) == (long long) ISAL_HIP_RAGGED_MAX_ITEMS);
        CHECK(isal_hip_scrub_create_ragged(&sc, 1, 2, g, S, lens, dd, cd, &bad) == ISAL_HIP_EINVAL && !sc && bad == -1);
        g[33] = 0;
        CHECK(isal_hip_scrub_create_ragged(&sc, 1, 2, g, S, lens, dd, cd, &bad) == ISAL_HIP_EINVAL && !sc && bad == -1);
        CHECK(isal_hip_scrub_create_ragged(&sc, 1, 2, g, S - 1, lens, dd, cd, &bad) == ISAL_HIP_ESINGULAR && !sc &&
              bad == -1);
        CHECK(g_hip_calls == calls);
        printf("  item limit: ok\n");
}

int
main(void)
{
        static const int mixed[] = { 4096 + 16 + 5, 0, 5, 16, 4096, 2 * 4096, 0, 3 * 4096 - 1, 17, 1, 4097, 0 };
        static const int small[] = { 37, 0, 0, 21, 1, 16, 15, 17, 4095, 33, 2, 3, 64, 48, 0, 7 };
        static const int wide[] = { 2 * 4096, 5, 4096 + 16 };
        static const int zero[] = { 0, 0, 0 };
        printf("scrub_ragged_host: isal_hip_scrub.c ragged host logic with stubbed HIP\n");
        error_paths();
        item_limit();
        run_geometry(0, 4, 2, 12, mixed);
        run_geometry(0, 10, 4, 16, small);
        run_geometry(1, 20, 8, 3, wide);
        run_geometry(0, 10, 4, 3, zero); /* every length 0: nothing launched, verdict untouched */
        printf("scrub_ragged_host: ok (%d stub launches)\n", g_launches);
        return 0;
}
