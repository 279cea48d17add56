/*
 * repair_ragged_host.c — TEST INFRASTRUCTURE: the ragged repair's host logic
 * (isa-l_amd/csrc/isal_hip_repair.c isal_hip_repair_create_ragged: the
 * (count, set) pattern dedupe, the count classes, the sort by pattern, the
 * blob layout, the item tables) under ASan + UBSan, as a stand-alone program.
 *
 * The HIP runtime (hip_stubs.c) and the kernel launchers (below) are stubs
 * ("device" memory is host memory), so the program needs no GPU and what
 * create() uploads can be read back: the launch stub rebuilds every item on
 * the CPU from the pointer, pattern, length and item tables it is handed and
 * nothing else. Every shard is an allocation of exactly its stripe's length,
 * so a table that reaches past a row's own length is an ASan report.
 *
 * Built by this directory's Makefile (make -C tests/sanitize) and run by
 * tests/test_sanitizers_cpu.py; the stubs every such program shares are in
 * hip_stubs.c.
 */
#include "hip_stubs.h"

/* ---- stubs: the launchers this program drives ------------------------------ */

static int g_launches, g_classes, g_unsorted, g_last_rows;

/* One class: per pass, every item of the table of the pass's tile size
 * rebuilds its tile of the pass's rows, bounded by the row's own length. */
int
isal_hip_launch_repair_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_pat, const uint32_t *d_tbl,
                              const int *d_lens, const unsigned *d_items, unsigned nitems,
                              const unsigned *d_items_small, unsigned nitems_small, int k, int rows, void *stream)
{
        int r0, l, j;
        unsigned w;
        (void) stream;
        CHECK(rows > g_last_rows); /* classes in ascending count */
        g_last_rows = rows;
        CHECK(ptr_stride == k + rows);
        g_classes++;
        for (r0 = 0; r0 < rows; r0 += EC_MAX_ROWS_PER_PASS) {
                const int P = rows - r0 < EC_MAX_ROWS_PER_PASS ? rows - r0 : EC_MAX_ROWS_PER_PASS;
                const int small = P <= ISAL_HIP_RAGGED_SMALL_ROWS;
                const long long tile = small ? ISAL_HIP_RAGGED_TILE_SMALL : ISAL_HIP_RAGGED_TILE;
                const unsigned *items = small ? d_items_small : d_items;
                const unsigned n = small ? nitems_small : nitems;
                CHECK(items && n > 0);
                g_launches++;
                for (w = 0; w < n; w++) {
                        const unsigned row = items[2 * w];
                        const long long b0 = items[2 * w + 1] * tile;
                        const int len = d_lens[row];
                        const long long b1 = b0 + tile < len ? b0 + tile : len;
                        const uint64_t *sp = d_ptrs + (size_t) row * ptr_stride;
                        const uint32_t *tbl = d_tbl + d_pat[row];
                        long long b;
                        CHECK(b0 < len);
                        if (w && (row < items[2 * w - 2] || d_pat[row] < d_pat[items[2 * w - 2]]))
                                g_unsorted++;
                        for (l = r0; l < r0 + P; l++) {
                                unsigned char *dst = (unsigned char *) (uintptr_t) sp[k + l];
                                for (b = b0; b < b1; b++) {
                                        unsigned char v = 0;
                                        for (j = 0; j < k; j++)
                                                v ^= gf_mul(coef_of(tbl, k, rows, l, j),
                                                            ((const unsigned char *) (uintptr_t) sp[j])[b]);
                                        dst[b] = v;
                                }
                        }
                }
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

static int
same_set(const unsigned char *x, const unsigned char *y, int n)
{
        int i;
        for (i = 0; i < n; i++)
                if (!memchr(y, x[i], (size_t) n))
                        return 0;
        return 1;
}

/* nstripes stripes, each with a length of lens[] and a count of counts[] (0
 * allowed), its pattern one of npool per count, the tail of its errs row
 * filled with junk */
static void
run_mixed(int cauchy, int k, int m, int nstripes, const int *lens, int nlens, const int *counts, int ncounts, int npool)
{
        int max_errs = 1, s, i, j, b, l, bad = -9, distinct = 0, launches = 0;
        unsigned char *a = malloc((size_t) m * k), *pool, *errs, *nerrs = malloc((size_t) nstripes);
        int *slen = malloc(sizeof(int) * (size_t) nstripes), *spool = malloc(sizeof(int) * (size_t) nstripes);
        unsigned char **sh = malloc(sizeof(*sh) * (size_t) nstripes * m);
        unsigned char **orig = malloc(sizeof(*orig) * (size_t) nstripes * m);
        char present[257];
        isal_hip_repair *r = NULL;
        for (i = 0; i < ncounts; i++)
                if (counts[i] > max_errs)
                        max_errs = counts[i];
        pool = malloc((size_t) ncounts * npool * max_errs);
        errs = malloc((size_t) nstripes * max_errs);
        CHECK(a && pool && errs && nerrs && slen && spool && sh && orig);
        if (cauchy)
                gf_gen_cauchy1_matrix(a, m, k);
        else
                gf_gen_rs_matrix(a, m, k);
        for (i = 0; i < ncounts * npool; i++)
                random_errs(m, counts[i / npool] ? counts[i / npool] : 1, pool + (size_t) i * max_errs);
        memset(present, 0, sizeof(present));
        for (s = 0; s < nstripes; s++) {
                const int ci = (int) rnd((unsigned) ncounts), c = counts[ci];
                const unsigned rot = rnd((unsigned) (c ? c : 1));
                const unsigned char *p;
                spool[s] = ci * npool + (int) rnd((unsigned) npool);
                p = pool + (size_t) spool[s] * max_errs;
                slen[s] = lens[rnd((unsigned) nlens)];
                nerrs[s] = (unsigned char) c;
                for (i = 0; i < max_errs; i++) /* junk past the count: a duplicate, or an index >= m */
                        errs[(size_t) s * max_errs + i] = i < c ? p[(i + rot) % (unsigned) c] : (i & 1) ? 255 : p[0];
                if (c) {
                        /* a new pattern unless an earlier stripe of this count has the same set */
                        for (j = 0; j < s; j++)
                                if (nerrs[j] == c && same_set(pool + (size_t) spool[j] * max_errs, p, c))
                                        break;
                        distinct += j == s;
                        if (slen[s])
                                present[c] = 1;
                }
                for (i = 0; i < m; i++) {
                        const size_t n = (size_t) slen[s];
                        CHECK(posix_memalign((void **) &sh[s * m + i], 16, n ? n : 1) == 0);
                        orig[s * m + i] = malloc(n ? n : 1);
                        CHECK(orig[s * m + i]);
                }
                for (i = 0; i < k; i++)
                        for (b = 0; b < slen[s]; b++)
                                sh[s * m + i][b] = (unsigned char) rnd(256);
                for (l = k; l < m; l++)
                        for (b = 0; b < slen[s]; b++) {
                                unsigned char v = 0;
                                for (j = 0; j < k; j++)
                                        v ^= gf_mul(a[(size_t) l * k + j], sh[s * m + j][b]);
                                sh[s * m + l][b] = v;
                        }
                for (i = 0; i < m; i++)
                        memcpy(orig[s * m + i], sh[s * m + i], (size_t) slen[s]);
                for (i = 0; i < c; i++)
                        memset(sh[s * m + errs[(size_t) s * max_errs + i]], 0xA5, (size_t) slen[s]);
        }
        for (i = 1; i <= 256; i++)
                if (present[i])
                        launches += (i + EC_MAX_ROWS_PER_PASS - 1) / EC_MAX_ROWS_PER_PASS;
        CHECK(isal_hip_repair_create_ragged(&r, k, m, a, nstripes, slen, max_errs, nerrs, errs, sh, &bad) == ISAL_HIP_OK);
        CHECK(r && bad == -1);
        CHECK(isal_hip_repair_npatterns(r) == distinct);
        for (j = 0; j < 2; j++) { /* a second run rebuilds the same bytes */
                g_unsorted = g_launches = g_last_rows = 0;
                CHECK(isal_hip_repair_run(r, NULL) == ISAL_HIP_OK);
                CHECK(g_unsorted == 0 && g_launches == launches);
                for (s = 0; s < nstripes; s++)
                        for (i = 0; i < m; i++)
                                CHECK(memcmp(sh[s * m + i], orig[s * m + i], (size_t) slen[s]) == 0);
        }
        CHECK(isal_hip_repair_destroy(r) == ISAL_HIP_OK);
        CHECK(g_allocs == 0);
        printf("  %s k=%d m=%d max_errs=%d stripes=%d: %d patterns, %d launches per run, rebuilt\n",
               cauchy ? "cauchy" : "rs", k, m, max_errs, nstripes, distinct, launches);
        for (i = 0; i < nstripes * m; i++) {
                free(sh[i]);
                free(orig[i]);
        }
        free(a);
        free(pool);
        free(errs);
        free(nerrs);
        free(slen);
        free(spool);
        free(sh);
        free(orig);
}

static void
error_paths(void)
{
        enum { K = 20, M = 28, S = 8, N = 6 };
        static const unsigned char singular[N] = {0, 13, 17, 18, 21, 23};
        unsigned char a[M * K], errs[S * N], nerrs[S], buf[16 * S * M + 16];
        unsigned char *sh[S * M];
        int lens[S] = {16, 0, 5, 16, 1, 0, 16, 16};
        isal_hip_repair *r = (isal_hip_repair *) buf; /* must come back NULL */
        int s, i, bad = -9;
        gf_gen_rs_matrix(a, M, K);
        for (i = 0; i < S * M; i++)
                sh[i] = buf + 16 * i + (16 - (uintptr_t) buf % 16) % 16;
        for (s = 0; s < S; s++) {
                nerrs[s] = (unsigned char) ((s == 5 || s == 7) ? N : s % (N + 1));
                for (i = 0; i < N; i++)
                        errs[s * N + i] = (s == 5 || s == 7) ? singular[N - 1 - i] : (unsigned char) (1 + i + s);
        }
        /* stripe 5 is empty and singular all the same */
        CHECK(isal_hip_repair_create_ragged(&r, K, M, a, S, lens, N, nerrs, errs, sh, &bad) == ISAL_HIP_ESINGULAR);
        CHECK(r == NULL && bad == 5);
        nerrs[3] = N + 1;
        CHECK(isal_hip_repair_create_ragged(&r, K, M, a, S, lens, N, nerrs, errs, sh, &bad) == ISAL_HIP_EINVAL && bad == 3);
        nerrs[3] = 3;
        errs[2 * N + 1] = errs[2 * N + 0]; /* a duplicate within stripe 2's two indices */
        CHECK(isal_hip_repair_create_ragged(&r, K, M, a, S, lens, N, nerrs, errs, sh, &bad) == ISAL_HIP_EINVAL && bad == 2);
        errs[2 * N + 1] = M;
        CHECK(isal_hip_repair_create_ragged(&r, K, M, a, S, lens, N, nerrs, errs, sh, &bad) == ISAL_HIP_EINVAL && bad == 2);
        errs[2 * N + 1] = 4;
        errs[2 * N + 2] = errs[2 * N + 0]; /* the same past the count is ignored */
        CHECK(isal_hip_repair_create_ragged(&r, K, M, a, S, lens, N, nerrs, errs, sh, &bad) == ISAL_HIP_ESINGULAR && bad == 5);
        lens[4] = -1;
        CHECK(isal_hip_repair_create_ragged(&r, K, M, a, S, lens, N, nerrs, errs, sh, &bad) == ISAL_HIP_EINVAL && bad == 4);
        lens[4] = 1;
        sh[0 * M + 4] += 8; /* stripe 0 lost nothing */
        CHECK(isal_hip_repair_create_ragged(&r, K, M, a, S, lens, N, nerrs, errs, sh, &bad) == ISAL_HIP_EINVAL && bad == 0);
        sh[0 * M + 4] = NULL;
        CHECK(isal_hip_repair_create_ragged(&r, K, M, a, S, lens, N, nerrs, errs, sh, &bad) == ISAL_HIP_EINVAL && bad == 0);
        CHECK(isal_hip_repair_create_ragged(NULL, K, M, a, S, lens, N, nerrs, errs, sh, &bad) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_repair_create_ragged(&r, K, M, a, S, lens, M - K + 1, nerrs, errs, sh, &bad) == ISAL_HIP_EINVAL &&
              bad == -1);
        CHECK(g_allocs == 0);
        printf("  error paths: ok\n");
}

int
main(void)
{
        static const int lens[] = {0, 1, 15, 16, 17, 33, 2047, 2048, 2049, 4095, 4096, 4097, 4112, 8197};
        static const int some[] = {0, 1, 17, 2049, 4097};
        static const int c012[] = {0, 1, 2}, c1234[] = {1, 2, 3, 4}, c368[] = {3, 6, 8}, c39[] = {9, 3}, c0[] = {0};
        static const int zero[] = {0}, c10[] = {10, 2, 11};
        printf("repair_ragged_host: isal_hip_repair.c ragged host logic with stubbed HIP\n");
        error_paths();
        run_mixed(0, 4, 6, 60, lens, 14, c012, 3, 15);
        run_mixed(0, 10, 14, 200, some, 5, c1234, 4, 60); /* the pattern arrays grow past their first size */
        run_mixed(1, 20, 28, 24, some, 5, c368, 3, 4);
        run_mixed(1, 4, 14, 12, lens, 14, c39, 2, 3);    /* two passes, the second on 2 KiB tiles */
        run_mixed(1, 4, 16, 12, some, 5, c10, 3, 2);     /* 8 + 2 and 8 + 3 rows: both tile sizes in one class */
        run_mixed(0, 10, 14, 5, lens, 14, c0, 1, 1);     /* nothing lost: no class, no allocation */
        run_mixed(0, 10, 14, 5, zero, 1, c1234, 4, 2);   /* every length 0 */
        run_mixed(0, 10, 14, 1, lens + 13, 1, c1234 + 3, 1, 1); /* a single stripe */
        printf("repair_ragged_host: ok\n");
        return 0;
}
