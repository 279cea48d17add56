/*
 * repair_host.c — TEST INFRASTRUCTURE: the repair batch's host logic
 * (isa-l_amd/csrc/isal_hip_repair.c: isal_hip_decode_matrix, the pattern
 * dedupe, the sort by pattern) under ASan + UBSan, as a stand-alone program.
 *
 * The HIP runtime (hip_stubs.c) and the kernel launcher (below) are stubs
 * ("device" memory is host memory), so the program needs no GPU and the
 * tables create() uploads can be read back: the launch stub rebuilds every
 * stripe on the CPU from the pointer table, the pattern indices and the
 * coefficient tables it is handed, and compares with the encoded shards.
 *
 * Built by this directory's Makefile (make -C tests/sanitize) and run by
 * tests/test_sanitizers_cpu.py; the stubs every such program shares are in
 * hip_stubs.c.
 */
#include "hip_stubs.h"

/* ---- stubs: the launchers this program drives ------------------------------ */

static int g_launches, g_rows_checked, g_unsorted;

int
isal_hip_launch_repair(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_pat, const uint32_t *d_tbl,
                       unsigned tbl_stride, int len, int k, int rows, long long nrows, void *stream)
{
        long long r;
        int l, j, b;
        (void) stream;
        g_launches++;
        for (r = 0; r < nrows; r++) {
                const uint64_t *sp = d_ptrs + r * ptr_stride;
                const uint32_t *tbl = d_tbl + (size_t) d_pat[r] * tbl_stride;
                if (r && d_pat[r] < d_pat[r - 1])
                        g_unsorted++;
                for (l = 0; l < rows; l++) {
                        unsigned char *dst = (unsigned char *) (uintptr_t) sp[k + l];
                        for (b = 0; b < len; b++) {
                                unsigned char v = 0;
                                for (j = 0; j < k; j++)
                                        v ^= gf_mul(coef_of(tbl, k, rows, l, j),
                                                    ((const unsigned char *) (uintptr_t) sp[j])[b]);
                                dst[b] = v;
                        }
                }
                g_rows_checked++;
        }
        return 0;
}

/* ---- the driver ----------------------------------------------------------- */

/* nerrs distinct indices below m, in a random order */
static void
random_errs(int m, int nerrs, unsigned char *e)
{
        int i, j;
        for (i = 0; i < nerrs; i++) {
                do {
                        e[i] = (unsigned char) rnd((unsigned) m);
                        for (j = 0; j < i && e[j] != e[i]; j++)
                                ;
                } while (j < i);
        }
}

static void
run_geometry(int cauchy, int k, int m, int nerrs, int nstripes, int len, int npool)
{
        unsigned char *a = malloc((size_t) m * k);
        unsigned char *pool = malloc((size_t) npool * nerrs), *errs = malloc((size_t) nstripes * nerrs);
        /* every shard in an allocation of its own, 16-byte aligned: ASan guards each */
        unsigned char **sh = malloc(sizeof(*sh) * (size_t) nstripes * m);
        unsigned char **orig = malloc(sizeof(*orig) * (size_t) nstripes * m);
        isal_hip_repair *r = NULL;
        int s, i, j, b, l, bad = -9, distinct = 0;
        CHECK(a && pool && errs && sh && orig);
        if (cauchy)
                gf_gen_cauchy1_matrix(a, m, k);
        else
                gf_gen_rs_matrix(a, m, k);
        for (i = 0; i < npool; i++) {
                random_errs(m, nerrs, pool + (size_t) i * nerrs);
                /* a pool entry that repeats an earlier set, in any order, is no new pattern */
                for (j = 0; j < i; j++) {
                        int same = 1;
                        for (b = 0; b < nerrs && same; b++)
                                same = memchr(pool + (size_t) j * nerrs, pool[(size_t) i * nerrs + b], (size_t) nerrs) != NULL;
                        if (same)
                                break;
                }
                distinct += j == i;
        }
        for (s = 0; s < nstripes; s++) {
                /* stripe s takes a pool pattern, its indices in another order each time */
                const unsigned char *p = pool + (size_t) rnd((unsigned) npool) * nerrs;
                const unsigned rot = rnd((unsigned) nerrs);
                for (i = 0; i < nerrs; i++)
                        errs[(size_t) s * nerrs + i] = p[(i + rot) % (unsigned) nerrs];
                for (i = 0; i < m; i++) {
                        CHECK(posix_memalign((void **) &sh[s * m + i], 16, (size_t) (len ? len : 1)) == 0);
                        orig[s * m + i] = malloc((size_t) (len ? len : 1));
                        CHECK(orig[s * m + i]);
                }
                for (i = 0; i < k; i++)
                        for (b = 0; b < len; b++)
                                sh[s * m + i][b] = (unsigned char) rnd(256);
                for (l = k; l < m; l++)
                        for (b = 0; b < len; b++) {
                                unsigned char v = 0;
                                for (j = 0; j < k; j++)
                                        v ^= gf_mul(a[(size_t) l * k + j], sh[s * m + j][b]);
                                sh[s * m + l][b] = v;
                        }
                for (i = 0; i < m; i++)
                        memcpy(orig[s * m + i], sh[s * m + i], (size_t) len);
                for (i = 0; i < nerrs; i++)
                        memset(sh[s * m + errs[(size_t) s * nerrs + i]], 0xA5, (size_t) len);
        }
        CHECK(isal_hip_repair_create(&r, len, k, m, a, nerrs, nstripes, errs, sh, &bad) == ISAL_HIP_OK);
        CHECK(r && bad == -1);
        CHECK(isal_hip_repair_npatterns(r) <= distinct && isal_hip_repair_npatterns(r) >= 1);
        g_unsorted = g_rows_checked = 0;
        CHECK(isal_hip_repair_run(r, NULL) == ISAL_HIP_OK);
        CHECK(g_unsorted == 0 && g_rows_checked == nstripes);
        for (s = 0; s < nstripes; s++)
                for (i = 0; i < m; i++)
                        CHECK(memcmp(sh[s * m + i], orig[s * m + i], (size_t) len) == 0);
        CHECK(isal_hip_repair_destroy(r) == ISAL_HIP_OK);
        printf("  %s k=%d m=%d nerrs=%d stripes=%d len=%d: %d patterns, rebuilt\n", cauchy ? "cauchy" : "rs", k, m,
               nerrs, nstripes, len, distinct);
        for (i = 0; i < nstripes * m; i++) {
                free(sh[i]);
                free(orig[i]);
        }
        free(a);
        free(pool);
        free(errs);
        free(sh);
        free(orig);
}

static void
error_paths(void)
{
        enum { K = 20, M = 28, S = 8, N = 6 };
        static const unsigned char singular[N] = {0, 13, 17, 18, 21, 23};
        unsigned char a[M * K], c[N * K], surv[K], errs[S * N], buf[16 * S * M + 16];
        unsigned char *sh[S * M];
        isal_hip_repair *r = (isal_hip_repair *) buf; /* must come back NULL */
        int s, i, bad = -9;
        gf_gen_rs_matrix(a, M, K);
        CHECK(isal_hip_decode_matrix(K, M, a, N, singular, c, surv) == ISAL_HIP_ESINGULAR);
        CHECK(isal_hip_decode_matrix(K, M, a, 0, singular, c, surv) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_decode_matrix(K, M, a, M - K + 1, singular, c, surv) == ISAL_HIP_EINVAL);
        for (i = 0; i < S * M; i++)
                sh[i] = buf + 16 * i + (16 - (uintptr_t) buf % 16) % 16;
        for (s = 0; s < S; s++)
                for (i = 0; i < N; i++)
                        errs[s * N + i] = (s == 5 || s == 7) ? singular[N - 1 - i] : (unsigned char) (1 + i + s);
        CHECK(isal_hip_repair_create(&r, 16, K, M, a, N, S, errs, sh, &bad) == ISAL_HIP_ESINGULAR);
        CHECK(r == NULL && bad == 5);
        errs[2 * N + 3] = errs[2 * N + 1]; /* a duplicate in stripe 2 comes first */
        CHECK(isal_hip_repair_create(&r, 16, K, M, a, N, S, errs, sh, &bad) == ISAL_HIP_EINVAL && bad == 2);
        errs[2 * N + 3] = M;
        CHECK(isal_hip_repair_create(&r, 16, K, M, a, N, S, errs, sh, &bad) == ISAL_HIP_EINVAL && bad == 2);
        errs[2 * N + 3] = 27;
        sh[1 * M + 4] += 8;
        CHECK(isal_hip_repair_create(&r, 16, K, M, a, N, S, errs, sh, &bad) == ISAL_HIP_EINVAL && bad == 1);
        sh[1 * M + 4] = NULL;
        CHECK(isal_hip_repair_create(&r, 16, K, M, a, N, S, errs, sh, &bad) == ISAL_HIP_EINVAL && bad == 1);
        CHECK(isal_hip_repair_create(NULL, 16, K, M, a, N, S, errs, sh, &bad) == ISAL_HIP_EINVAL);
        printf("  error paths: ok\n");
}

int
main(void)
{
        printf("repair_host: isal_hip_repair.c host logic with stubbed HIP\n");
        error_paths();
        run_geometry(0, 4, 6, 1, 37, 37, 6);
        run_geometry(0, 4, 6, 2, 37, 21, 15);
        run_geometry(0, 10, 14, 3, 200, 19, 120); /* the pattern arrays grow past their first size */
        run_geometry(0, 10, 14, 4, 64, 16, 40);
        run_geometry(1, 20, 28, 8, 24, 17, 10);
        run_geometry(1, 4, 14, 9, 6, 33, 6); /* two passes per pattern */
        run_geometry(0, 10, 14, 3, 1, 0, 1); /* len = 0 */
        printf("repair_host: ok (%d stub launches)\n", g_launches);
        return 0;
}
