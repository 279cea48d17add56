/*
 * ragged_host.c — TEST INFRASTRUCTURE: the ragged batch's host logic
 * (isa-l_amd/csrc/isal_hip_ragged.c: isal_hip_ragged_items, create's refusals,
 * the pointer, coefficient, length and item tables) under ASan + UBSan, as a
 * stand-alone program.
 *
 * The HIP runtime (hip_stubs.c) and the kernel launchers (below) are stubs
 * ("device" memory is host memory), so the program needs no GPU and the
 * tables create() uploads can be read back: the launch stubs walk the
 * uploaded item table of each pass, take every item's length from the
 * uploaded lengths and encode (or compare) that tile's bytes with gf_mul on
 * the coefficients of the uploaded tables, as the kernels do; the driver
 * compares the parity with ec_encode_data_base per stripe and the check's
 * words with the corruption it planted. Every shard is an allocation of
 * exactly its stripe's length, so a byte past any stripe's own length is an
 * ASan report.
 *
 * Built by this directory's Makefile (make -C tests/sanitize) and run by
 * tests/test_sanitizers_cpu.py; the stubs every such program shares are in
 * hip_stubs.c.
 */
#include "hip_stubs.h"

/* ---- stubs: the launchers this program drives ------------------------------ */

static int g_launches;

/* ec_encode_data_base as the library serves it for host shards without a GPU:
 * the engine's CPU route (ec_cpu.c), none of the code under test */
void
ec_encode_data_base(int len, int k, int rows, unsigned char *gftbls, unsigned char **data, unsigned char **coding)
{
        (void) isal_cpu_run(ISAL_HIP_OP_ENCODE, 0, len, k, rows, 0, gftbls, data, k, coding);
}

/* one item: bytes [tile * span, min(len, (tile + 1) * span)) of rows [r0, r0 + P) */
static void
run_item(const uint64_t *sp, const uint32_t *tbl, int k, int rows, int r0, int P, int len, unsigned tile, int span,
         unsigned long long *bad)
{
        const long long lo = (long long) tile * span;
        const long long hi = lo + span < len ? lo + span : len;
        long long b;
        int l, j;
        CHECK(lo < len); /* the table holds no item past a stripe's end */
        for (b = lo; b < hi; b++)
                for (l = 0; l < P; l++) {
                        unsigned char v = 0, *dst = (unsigned char *) (uintptr_t) sp[k + r0 + l];
                        for (j = 0; j < k; j++)
                                v ^= gf_mul(coef_of(tbl, k, rows, r0 + l, j), ((const unsigned char *) (uintptr_t) sp[j])[b]);
                        if (!bad)
                                dst[b] = v;
                        else if (dst[b] != v) {
                                const unsigned long long key = ((unsigned long long) b << 8) | (unsigned) (r0 + l);
                                if (key < *bad)
                                        *bad = key;
                        }
                }
}

/* the item table is the one isal_hip_ragged_items describes for d_lens */
static void
check_table(const unsigned *items, unsigned nitems, const int *lens, int nstripes, int span)
{
        unsigned n = 0;
        int s;
        long long t;
        for (s = 0; s < nstripes; s++)
                for (t = 0; t * span < lens[s]; t++, n++) {
                        CHECK(n < nitems);
                        CHECK(items[2 * n] == (unsigned) s && items[2 * n + 1] == (unsigned) t);
                }
        CHECK(n == nitems);
}

static int g_nstripes; /* the launch stubs' view of the object under test */

int
isal_hip_launch_encode_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_tbl, const int *d_lens,
                              const unsigned *d_items, unsigned nitems, const unsigned *d_items_small,
                              unsigned nitems_small, int k, int rows, void *stream)
{
        int r0;
        (void) stream;
        if (nitems == 0)
                return 0;
        CHECK(ptr_stride == k + rows);
        for (r0 = 0; r0 < rows; r0 += EC_MAX_ROWS_PER_PASS) {
                const int P = rows - r0 < EC_MAX_ROWS_PER_PASS ? rows - r0 : EC_MAX_ROWS_PER_PASS;
                const int small = P <= ISAL_HIP_RAGGED_SMALL_ROWS;
                const unsigned *items = small ? d_items_small : d_items, n = small ? nitems_small : nitems;
                const int span = small ? ISAL_HIP_RAGGED_TILE_SMALL : ISAL_HIP_RAGGED_TILE;
                unsigned w;
                CHECK(items && n);
                check_table(items, n, d_lens, g_nstripes, span);
                g_launches++;
                for (w = 0; w < n; w++) {
                        const unsigned s = items[2 * w];
                        run_item(d_ptrs + (size_t) s * ptr_stride, d_tbl, k, rows, r0, P, d_lens[s], items[2 * w + 1], span,
                                 NULL);
                }
        }
        return 0;
}

int
isal_hip_launch_verify_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_tbl, const int *d_lens,
                              const unsigned *d_items, unsigned nitems, int k, int rows, long long nstripes,
                              unsigned long long *bad, void *stream)
{
        long long s;
        int r0;
        (void) stream;
        if (nitems == 0)
                return 0;
        CHECK(ptr_stride == k + rows && nstripes == g_nstripes && d_items);
        check_table(d_items, nitems, d_lens, g_nstripes, ISAL_HIP_RAGGED_TILE);
        for (s = 0; s < nstripes; s++)
                bad[s] = ~0ull;
        for (r0 = 0; r0 < rows; r0 += EC_MAX_ROWS_PER_PASS) {
                const int P = rows - r0 < EC_MAX_ROWS_PER_PASS ? rows - r0 : EC_MAX_ROWS_PER_PASS;
                unsigned w;
                g_launches++;
                for (w = 0; w < nitems; w++) {
                        const unsigned st = d_items[2 * w];
                        run_item(d_ptrs + (size_t) st * ptr_stride, d_tbl, k, rows, r0, P, d_lens[st], d_items[2 * w + 1],
                                 ISAL_HIP_RAGGED_TILE, bad + st);
                }
        }
        return 0;
}

/* ---- the driver ----------------------------------------------------------- */

static void
run_geometry(int cauchy, int k, int rows, int nstripes, const int *lens)
{
        const int m = k + rows;
        unsigned char *a = malloc((size_t) m * k), *g = malloc(32 * (size_t) k * rows);
        unsigned char **data = malloc(sizeof(*data) * (size_t) nstripes * k);
        unsigned char **par = malloc(sizeof(*par) * (size_t) nstripes * rows);
        unsigned char **ref = malloc(sizeof(*ref) * (size_t) rows);
        unsigned long long *bad = malloc(sizeof(*bad) * (size_t) nstripes);
        isal_hip_ragged *rg = NULL;
        int s, j, l, b, stripe = -9, before, any = 0;
        CHECK(a && g && data && par && ref && bad);
        if (cauchy)
                gf_gen_cauchy1_matrix(a, m, k);
        else
                gf_gen_rs_matrix(a, m, k);
        ec_init_tables(k, rows, a + (size_t) k * k, g);
        for (s = 0; s < nstripes; s++) {
                any |= lens[s];
                for (j = 0; j < k; j++) {
                        data[s * k + j] = shard(lens[s]);
                        for (b = 0; b < lens[s]; b++)
                                data[s * k + j][b] = (unsigned char) rnd(256);
                }
                for (l = 0; l < rows; l++) {
                        par[s * rows + l] = shard(lens[s]);
                        memset(par[s * rows + l], 0xA5, (size_t) lens[s]);
                }
                bad[s] = 0x5a5a5a5a5a5a5a5aull;
        }
        g_nstripes = nstripes;
        CHECK(isal_hip_ragged_create(&rg, k, rows, g, nstripes, lens, data, par, &stripe) == ISAL_HIP_OK);
        CHECK(rg && stripe == -1);
        before = g_launches;
        CHECK(isal_hip_ragged_encode(rg, NULL) == ISAL_HIP_OK);
        CHECK(g_launches - before == (any ? (rows + 7) / 8 : 0));
        for (s = 0; s < nstripes; s++) {
                for (l = 0; l < rows; l++)
                        ref[l] = shard(lens[s]);
                ec_encode_data_base(lens[s], k, rows, g, &data[s * k], ref);
                for (l = 0; l < rows; l++) {
                        CHECK(memcmp(ref[l], par[s * rows + l], (size_t) lens[s]) == 0);
                        free(ref[l]);
                }
        }
        CHECK(isal_hip_ragged_check(rg, NULL, NULL) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_ragged_check(rg, bad, NULL) == ISAL_HIP_OK);
        for (s = 0; s < nstripes; s++)
                CHECK(bad[s] == (any ? ~0ull : 0x5a5a5a5a5a5a5a5aull));
        /* the last byte of every non-empty stripe's last parity row, and in
         * stripes of two bytes or more byte 0 of source 0 as well */
        for (s = 0; s < nstripes; s++)
                if (lens[s]) {
                        par[s * rows + rows - 1][lens[s] - 1] ^= 0x80;
                        if (lens[s] > 1)
                                data[s * k][0] ^= 1;
                }
        CHECK(isal_hip_ragged_check(rg, bad, NULL) == ISAL_HIP_OK);
        for (s = 0; s < nstripes; s++) {
                unsigned long long want = ~0ull;
                if (lens[s] > 1) {
                        for (l = rows - 1; l >= 0; l--) /* the first row source 0 reaches */
                                if (a[(size_t) (k + l) * k])
                                        want = (unsigned long long) l;
                } else if (lens[s] == 1) {
                        want = (unsigned long long) (rows - 1);
                }
                CHECK(bad[s] == (any ? want : 0x5a5a5a5a5a5a5a5aull));
        }
        CHECK(isal_hip_ragged_destroy(rg) == ISAL_HIP_OK);
        printf("  %s k=%d rows=%d stripes=%d: parity as ec_encode_data_base, check words as planted\n",
               cauchy ? "cauchy" : "rs", k, rows, nstripes);
        for (s = 0; s < nstripes * k; s++)
                free(data[s]);
        for (s = 0; s < nstripes * rows; s++)
                free(par[s]);
        free(a);
        free(g);
        free(data);
        free(par);
        free(ref);
        free(bad);
}

static void
items_cases(void)
{
        static const int lens[] = { 0, 5, 4096, 4097, 0, 0, 8192, 1, 0 };
        unsigned *items = malloc(sizeof(unsigned) * 2 * 11); /* exactly the 11 items of tile 2048 */
        int neg[3] = { 1, -1, 2 };
        CHECK(items);
        CHECK(isal_hip_ragged_items(9, lens, 2048, NULL) == 11);
        CHECK(isal_hip_ragged_items(9, lens, 2048, items) == 11);
        check_table(items, 11, lens, 9, 2048);
        CHECK(isal_hip_ragged_items(9, lens, 4096, items) == 7);
        check_table(items, 7, lens, 9, 4096);
        CHECK(isal_hip_ragged_items(3, neg, 4096, items) == -1);
        CHECK(isal_hip_ragged_items(0, lens, 4096, NULL) == -1);
        CHECK(isal_hip_ragged_items(9, NULL, 4096, NULL) == -1);
        CHECK(isal_hip_ragged_items(9, lens, 0, NULL) == -1);
        free(items);
        printf("  items: ok\n");
}

static void
error_paths(void)
{
        enum { K = 10, R = 4, S = 6, LEN = 64 };
        unsigned char a[(K + R) * K], g[32 * K * R], *buf;
        unsigned char *dd[S * K], *cd[S * R], *keep;
        int lens[S] = { LEN, 0, 7, LEN, 1, 16 }, *huge;
        unsigned char **one;
        isal_hip_ragged *rg;
        int i, bad, calls;
        CHECK(posix_memalign((void **) &buf, 16, (size_t) S * (K + R) * LEN) == 0);
        gf_gen_rs_matrix(a, K + R, K);
        ec_init_tables(K, R, a + K * K, g);
        for (i = 0; i < S * K; i++)
                dd[i] = buf + (size_t) LEN * i;
        for (i = 0; i < S * R; i++)
                cd[i] = buf + (size_t) LEN * (S * K + i);
        calls = g_hip_calls;
#define CREATE(k, rows, g_, ns, l_, d_, c_) \
        (rg = (isal_hip_ragged *) buf, bad = -9, isal_hip_ragged_create(&rg, k, rows, g_, ns, l_, d_, c_, &bad))
#define REFUSED(expr, stripe) CHECK((expr) == ISAL_HIP_EINVAL && rg == NULL && bad == (stripe))
        CHECK(isal_hip_ragged_create(NULL, K, R, g, S, lens, dd, cd, &bad) == ISAL_HIP_EINVAL);
        REFUSED(CREATE(K, R, NULL, S, lens, dd, cd), -1);
        REFUSED(CREATE(K, R, g, S, NULL, dd, cd), -1);
        REFUSED(CREATE(K, R, g, S, lens, NULL, cd), -1);
        REFUSED(CREATE(K, R, g, S, lens, dd, NULL), -1);
        REFUSED(CREATE(0, R, g, S, lens, dd, cd), -1);
        REFUSED(CREATE(K, 0, g, S, lens, dd, cd), -1);
        REFUSED(CREATE(253, 4, g, S, lens, dd, cd), -1); /* refused before gftbls is read */
        REFUSED(CREATE(K, R, g, 0, lens, dd, cd), -1);
        lens[3] = -1;
        REFUSED(CREATE(K, R, g, S, lens, dd, cd), 3);
        keep = cd[1 * R + 1];
        cd[1 * R + 1] = keep + 8; /* misaligned, in the zero-length stripe 1: it wins over stripe 3 */
        REFUSED(CREATE(K, R, g, S, lens, dd, cd), 1);
        lens[3] = LEN;
        cd[1 * R + 1] = NULL;
        dd[4 * K] = NULL; /* a later offender does not change the answer */
        REFUSED(CREATE(K, R, g, S, lens, dd, cd), 1);
        cd[1 * R + 1] = keep;
        REFUSED(CREATE(K, R, g, S, lens, dd, cd), 4);
        dd[4 * K] = buf + (size_t) LEN * 4 * K;
        /* more than 2^30 items at the 2 KiB tile: 1025 stripes of 2^31 - 1 bytes */
        huge = malloc(sizeof(int) * 1025);
        one = malloc(sizeof(*one) * 1025);
        CHECK(huge && one);
        for (i = 0; i < 1025; i++) {
                huge[i] = 0x7fffffff;
                one[i] = buf;
        }
        REFUSED(CREATE(1, 1, g, 1025, huge, one, one), -1);
        free(huge);
        free(one);
        CHECK(g_hip_calls == calls); /* every refusal came before the first HIP call */
        /* everything put back: accepted */
        g_nstripes = S;
        CHECK(CREATE(K, R, g, S, lens, dd, cd) == ISAL_HIP_OK && rg && bad == -1);
        CHECK(isal_hip_ragged_destroy(rg) == ISAL_HIP_OK);
        CHECK(isal_hip_ragged_encode(NULL, NULL) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_ragged_check(NULL, (unsigned long long *) buf, NULL) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_ragged_destroy(NULL) == ISAL_HIP_OK);
#undef CREATE
#undef REFUSED
        free(buf);
        printf("  error paths: ok\n");
}

int
main(void)
{
        static const int l7[] = { 0, 5, 16, 4096, 4112, 8247, 1 };
        static const int l7s[] = { 2048, 1, 0, 0, 2064, 4151, 5, 16 };
        static const int l3[] = { 4097, 0, 33 };
        static const int zeros[] = { 0, 0, 0 };
        printf("ragged_host: isal_hip_ragged.c host logic with stubbed HIP\n");
        items_cases();
        error_paths();
        run_geometry(0, 4, 2, 8, l7s);  /* one pass on 2 KiB tiles */
        run_geometry(0, 10, 4, 7, l7);  /* one pass on 4 KiB tiles */
        run_geometry(1, 20, 8, 3, l3);  /* a full 8-row pass */
        run_geometry(0, 6, 10, 7, l7);  /* two passes with different tile sizes */
        run_geometry(0, 10, 4, 3, zeros); /* nothing launched, bad untouched */
        printf("ragged_host: ok (%d stub launches)\n", g_launches);
        return 0;
}
