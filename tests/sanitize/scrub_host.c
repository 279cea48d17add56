/*
 * scrub_host.c — TEST INFRASTRUCTURE: the scrub batch's host logic
 * (isa-l_amd/csrc/isal_hip_scrub.c: isal_hip_scrub_ambiguity,
 * isal_hip_locate_syndrome, create's refusals, the pointer, coefficient and
 * location tables) under ASan + UBSan, as a stand-alone program.
 *
 * The HIP runtime (hip_stubs.c) and the kernel launcher (below) are stubs
 * ("device" memory is host memory), so the program needs no GPU and the
 * tables create() uploads can be read back: the launch stub walks every byte
 * column of every stripe from the pointer table and names the shard from the
 * location tables alone (coefficients, pivot rows, inverses), as the kernel's
 * mismatch branch does; the driver compares the verdicts with the corruption
 * it planted and with isal_hip_locate_syndrome.
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

int
isal_hip_launch_locate_batch(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_tbl, int len, int k, int rows,
                             long long nstripes, const isal_hip_encmask *em, const unsigned char *d_loc,
                             unsigned *verdict, void *stream)
{
        long long s;
        int b, l, j;
        (void) stream;
        if (len <= 0)
                return 0;
        g_launches++;
        CHECK(ptr_stride == k + rows && em && rows <= EC_MAX_ROWS_PER_PASS);
        for (l = 0; l < rows; l++)
                for (j = 0; j < k; j++)
                        CHECK(d_loc[(size_t) l * k + j] == coef_of(d_tbl, k, rows, l, j));
        for (s = 0; s < nstripes; s++) {
                const uint64_t *sp = d_ptrs + s * ptr_stride;
                verdict[s] = ISAL_HIP_SCRUB_CLEAN;
                for (b = 0; b < len; b++) {
                        unsigned char e[EC_MAX_ROWS_PER_PASS];
                        unsigned v, any = 0;
                        for (l = 0; l < rows; l++) {
                                e[l] = ((const unsigned char *) (uintptr_t) sp[k + l])[b];
                                for (j = 0; j < k; j++)
                                        e[l] ^= gf_mul(coef_of(d_tbl, k, rows, l, j),
                                                       ((const unsigned char *) (uintptr_t) sp[j])[b]);
                                any |= e[l];
                        }
                        if (!any)
                                continue;
                        v = name_shard(d_loc, k, rows, e);
                        if (verdict[s] == ISAL_HIP_SCRUB_CLEAN)
                                verdict[s] = v;
                        else if (verdict[s] != v)
                                verdict[s] = ISAL_HIP_SCRUB_MULTI;
                }
        }
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

/* every multiple of every column names its shard; random syndromes agree with
 * a search over all shards and multipliers */
static void
run_syndromes(int cauchy, int k, int rows)
{
        unsigned char *a = malloc((size_t) (k + rows) * k), *g = malloc(32 * (size_t) k * rows);
        unsigned char *e = malloc((size_t) rows); /* exactly rows bytes: ASan guards the end */
        int pair[2] = { 9, 9 }, j, l, d, t;
        CHECK(a && g && e);
        make_tables(cauchy, k, rows, a, g);
        CHECK(isal_hip_scrub_ambiguity(k, rows, g, pair) == ISAL_HIP_OK && pair[0] == -1 && pair[1] == -1);
        memset(e, 0, (size_t) rows);
        CHECK(isal_hip_locate_syndrome(k, rows, g, e) == (int) ISAL_HIP_SCRUB_CLEAN);
        for (j = 0; j < k + rows; j++)
                for (d = 1; d < 256; d++) {
                        for (l = 0; l < rows; l++)
                                e[l] = j < k ? gf_mul(a[(size_t) (k + l) * k + j], (unsigned char) d)
                                             : (unsigned char) (j - k == l ? d : 0);
                        CHECK(isal_hip_locate_syndrome(k, rows, g, e) == j);
                }
        for (t = 0; t < 2000; t++) {
                int want = (int) ISAL_HIP_SCRUB_MULTI, any = 0;
                for (l = 0; l < rows; l++)
                        any |= e[l] = (unsigned char) rnd(256);
                if (!any)
                        want = (int) ISAL_HIP_SCRUB_CLEAN;
                for (j = 0; any && j < k + rows && want == (int) ISAL_HIP_SCRUB_MULTI; j++)
                        for (d = 1; d < 256 && want == (int) ISAL_HIP_SCRUB_MULTI; d++) {
                                for (l = 0; l < rows; l++)
                                        if (e[l] != (j < k ? gf_mul(a[(size_t) (k + l) * k + j], (unsigned char) d)
                                                           : (unsigned char) (j - k == l ? d : 0)))
                                                break;
                                if (l == rows)
                                        want = j;
                        }
                CHECK(isal_hip_locate_syndrome(k, rows, g, e) == want);
        }
        printf("  %s k=%d rows=%d: %d column multiples, 2000 random syndromes\n", cauchy ? "cauchy" : "rs", k, rows,
               255 * (k + rows));
        free(a);
        free(g);
        free(e);
}

static void
run_geometry(int cauchy, int k, int rows, int nstripes, int len)
{
        const int m = k + rows;
        unsigned char *a = malloc((size_t) m * k), *g = malloc(32 * (size_t) k * rows);
        /* every shard in an allocation of its own, 16-byte aligned: ASan guards each */
        unsigned char **data = malloc(sizeof(*data) * (size_t) nstripes * k);
        unsigned char **par = malloc(sizeof(*par) * (size_t) nstripes * rows);
        unsigned *verdict = malloc(sizeof(*verdict) * (size_t) nstripes), *want = malloc(sizeof(*want) * (size_t) nstripes);
        isal_hip_scrub *sc = NULL;
        int s, j, l, b, bad = -9;
        CHECK(a && g && data && par && verdict && want);
        make_tables(cauchy, k, rows, a, g);
        for (s = 0; s < nstripes; s++) {
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
                /* stripe s: shard s % (m + 2) corrupt in two places; m: clean; m + 1: two shards */
                want[s] = ISAL_HIP_SCRUB_CLEAN;
                if (len) {
                        const int i = s % (m + 2);
                        unsigned char **sh = i < k ? &data[s * k + i] : &par[s * rows + (i - k)];
                        if (i < m) {
                                (*sh)[rnd((unsigned) len - 1)] ^= (unsigned char) (1 + rnd(255));
                                (*sh)[len - 1] ^= 0x80;
                                want[s] = (unsigned) i;
                        } else if (i == m + 1 && len > 1) {
                                data[s * k][0] ^= 1;
                                par[s * rows + 1][1] ^= 1;
                                want[s] = ISAL_HIP_SCRUB_MULTI;
                        }
                }
                verdict[s] = 0x5a5a5a5au;
        }
        CHECK(isal_hip_scrub_create(&sc, len, k, rows, g, nstripes, data, par, &bad) == ISAL_HIP_OK);
        CHECK(sc && bad == -1);
        CHECK(isal_hip_scrub_run(sc, NULL, NULL) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_scrub_run(sc, verdict, NULL) == ISAL_HIP_OK);
        for (s = 0; s < nstripes; s++)
                CHECK(verdict[s] == (len ? want[s] : 0x5a5a5a5au));
        CHECK(isal_hip_scrub_destroy(sc) == ISAL_HIP_OK);
        printf("  %s k=%d rows=%d stripes=%d len=%d: verdicts as planted\n", cauchy ? "cauchy" : "rs", k, rows,
               nstripes, len);
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
        static const unsigned char zero_c[6] = { 1, 0, 1, 2, 0, 3 }, unit_c[6] = { 1, 0, 1, 2, 5, 3 };
        unsigned char c[8];
        isal_hip_scrub *sc;
        int i, bad, pair[2];
        CHECK(posix_memalign((void **) &buf, 16, (size_t) S * (K + R) * LEN) == 0);
        make_tables(0, K, R, a, g);
        for (i = 0; i < S * K; i++)
                dd[i] = buf + (size_t) LEN * i;
        for (i = 0; i < S * R; i++)
                cd[i] = buf + (size_t) LEN * (S * K + i);
#define CREATE(len, k, rows, g_, ns, d_, c_) \
        (sc = (isal_hip_scrub *) buf, bad = -9, isal_hip_scrub_create(&sc, len, k, rows, g_, ns, d_, c_, &bad))
#define REFUSED(expr, code, stripe) CHECK((expr) == (code) && sc == NULL && bad == (stripe))
        CHECK(isal_hip_scrub_create(NULL, LEN, K, R, g, S, dd, cd, &bad) == ISAL_HIP_EINVAL);
        REFUSED(CREATE(LEN, K, R, NULL, S, dd, cd), ISAL_HIP_EINVAL, -1);
        REFUSED(CREATE(LEN, K, R, g, S, NULL, cd), ISAL_HIP_EINVAL, -1);
        REFUSED(CREATE(LEN, K, R, g, S, dd, NULL), ISAL_HIP_EINVAL, -1);
        REFUSED(CREATE(-1, K, R, g, S, dd, cd), ISAL_HIP_EINVAL, -1);
        REFUSED(CREATE(LEN, 0, R, g, S, dd, cd), ISAL_HIP_EINVAL, -1);
        REFUSED(CREATE(LEN, K, 1, g, S, dd, cd), ISAL_HIP_EINVAL, -1);
        REFUSED(CREATE(LEN, K, 9, g, S, dd, cd), ISAL_HIP_EINVAL, -1); /* refused before gftbls is read */
        REFUSED(CREATE(LEN, 253, 4, g, S, dd, cd), ISAL_HIP_EINVAL, -1);
        REFUSED(CREATE(LEN, K, R, g, 0, dd, cd), ISAL_HIP_EINVAL, -1);
        keep = cd[2 * R + 1];
        cd[2 * R + 1] = keep + 8; /* misaligned, stripe 2 */
        REFUSED(CREATE(LEN, K, R, g, S, dd, cd), ISAL_HIP_EINVAL, 2);
        cd[2 * R + 1] = NULL;
        dd[4 * K] = NULL; /* a later offender does not change the answer */
        REFUSED(CREATE(LEN, K, R, g, S, dd, cd), ISAL_HIP_EINVAL, 2);
        cd[2 * R + 1] = keep;
        REFUSED(CREATE(LEN, K, R, g, S, dd, cd), ISAL_HIP_EINVAL, 4);
        dd[4 * K] = buf + (size_t) LEN * 4 * K;
        /* the ambiguous matrices */
        memcpy(c, amb_c, 8);
        ec_init_tables(4, 2, c, amb);
        CHECK(isal_hip_scrub_ambiguity(4, 2, amb, pair) == ISAL_HIP_ESINGULAR && pair[0] == 1 && pair[1] == 3);
        CHECK(isal_hip_scrub_ambiguity(4, 2, amb, NULL) == ISAL_HIP_ESINGULAR);
        REFUSED(CREATE(LEN, 4, 2, amb, S, dd, cd), ISAL_HIP_ESINGULAR, -1);
        memcpy(c, zero_c, 6);
        ec_init_tables(3, 2, c, amb);
        CHECK(isal_hip_scrub_ambiguity(3, 2, amb, pair) == ISAL_HIP_ESINGULAR && pair[0] == 1 && pair[1] == 1);
        memcpy(c, unit_c, 6);
        ec_init_tables(3, 2, c, amb);
        CHECK(isal_hip_scrub_ambiguity(3, 2, amb, pair) == ISAL_HIP_ESINGULAR && pair[0] == 1 && pair[1] == 4);
        CHECK(isal_hip_scrub_ambiguity(0, 2, amb, pair) == ISAL_HIP_EINVAL && pair[0] == -1);
        CHECK(isal_hip_scrub_ambiguity(3, 0, amb, pair) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_scrub_ambiguity(253, 4, amb, pair) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_scrub_ambiguity(3, 2, NULL, pair) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_locate_syndrome(3, 2, NULL, c) == (int) ISAL_HIP_SCRUB_MULTI);
        CHECK(isal_hip_locate_syndrome(3, 2, amb, NULL) == (int) ISAL_HIP_SCRUB_MULTI);
        CHECK(isal_hip_locate_syndrome(0, 2, amb, c) == (int) ISAL_HIP_SCRUB_MULTI);
        /* everything put back: accepted; equal pointers at len 0 too */
        CHECK(CREATE(LEN, K, R, g, S, dd, cd) == ISAL_HIP_OK && sc && bad == -1);
        CHECK(isal_hip_scrub_destroy(sc) == ISAL_HIP_OK);
        CHECK(CREATE(0, K, R, g, S, dd, cd) == ISAL_HIP_OK && sc && bad == -1);
        CHECK(isal_hip_scrub_destroy(sc) == ISAL_HIP_OK);
        CHECK(isal_hip_scrub_run(NULL, (unsigned *) buf, NULL) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_scrub_destroy(NULL) == ISAL_HIP_OK);
#undef CREATE
#undef REFUSED
        free(buf);
        printf("  error paths: ok\n");
}

int
main(void)
{
        printf("scrub_host: isal_hip_scrub.c host logic with stubbed HIP\n");
        error_paths();
        run_syndromes(0, 4, 2);
        run_syndromes(0, 10, 4);
        run_syndromes(1, 20, 8);
        run_geometry(0, 4, 2, 9, 37);
        run_geometry(0, 10, 4, 33, 21);
        run_geometry(1, 20, 8, 31, 17);
        run_geometry(0, 10, 4, 3, 0); /* len = 0: nothing launched, verdict untouched */
        printf("scrub_host: ok (%d stub launches)\n", g_launches);
        return 0;
}
