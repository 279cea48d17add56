/*
 * overwrite_host.c — TEST INFRASTRUCTURE: the overwrite batch's host logic
 * (isa-l_amd/csrc/isal_hip_overwrite.c: the per-stripe index, pointer and
 * overlap checks, the pointer / index / coefficient tables) under ASan +
 * UBSan, as a stand-alone program.
 *
 * The HIP runtime (hip_stubs.c) and the kernel launcher (below) are stubs
 * ("device" memory is host memory), so the program needs no GPU and the
 * tables create() uploads can be read back: the launch stub applies every
 * stripe's delta on the CPU from the pointer table, the index table and the
 * coefficient tables it is handed; the driver compares the parity with a
 * fresh encode of the stripe with the new bytes in place.
 *
 * Built by this directory's Makefile (make -C tests/sanitize) and run by
 * tests/test_sanitizers_cpu.py; the stubs every such program shares are in
 * hip_stubs.c.
 */
#include "hip_stubs.h"

/* ---- stubs: the launchers this program drives ------------------------------ */

static int g_launches, g_commits;

int
isal_hip_launch_overwrite(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_idx, const uint32_t *d_tbl,
                          int len, int k, int rows, int nw, long long nstripes, int commit, void *stream)
{
        long long s;
        int i, l, b;
        (void) stream;
        g_launches++;
        g_commits += commit != 0;
        CHECK(ptr_stride == 2 * nw + rows);
        for (s = 0; s < nstripes; s++) {
                const uint64_t *sp = d_ptrs + s * ptr_stride;
                for (i = 0; i < nw; i++) {
                        unsigned char *o = (unsigned char *) (uintptr_t) sp[i];
                        const unsigned char *n = (const unsigned char *) (uintptr_t) sp[nw + i];
                        const int j = (int) d_idx[s * nw + i];
                        CHECK(j < k);
                        for (l = 0; l < rows; l++) {
                                unsigned char *dst = (unsigned char *) (uintptr_t) sp[2 * nw + l];
                                const unsigned char c = coef_of(d_tbl, k, rows, l, j);
                                for (b = 0; b < len; b++)
                                        dst[b] ^= gf_mul(c, (unsigned char) (o[b] ^ n[b]));
                        }
                        if (commit)
                                memcpy(o, n, (size_t) len);
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

static void
run_geometry(int cauchy, int k, int rows, int nw, int nstripes, int len)
{
        const int m = k + rows;
        unsigned char *a = malloc((size_t) m * k), *g = malloc(32 * (size_t) k * rows);
        unsigned char *idx = malloc((size_t) nstripes * nw);
        /* every shard in an allocation of its own, 16-byte aligned: ASan guards each */
        unsigned char **data = malloc(sizeof(*data) * (size_t) nstripes * k);
        unsigned char **par = malloc(sizeof(*par) * (size_t) nstripes * rows);
        unsigned char **par0 = malloc(sizeof(*par0) * (size_t) nstripes * rows);
        unsigned char **want = malloc(sizeof(*want) * (size_t) rows);
        unsigned char **nw_new = malloc(sizeof(*nw_new) * (size_t) nstripes * nw);
        unsigned char **nw_old = malloc(sizeof(*nw_old) * (size_t) nstripes * nw);
        unsigned char **cur = malloc(sizeof(*cur) * (size_t) k);
        isal_hip_overwrite *o = NULL;
        int s, i, j, b, l, bad = -9;
        const int passes = (rows + EC_MAX_ROWS_PER_PASS - 1) / EC_MAX_ROWS_PER_PASS;
        CHECK(a && g && idx && data && par && par0 && want && nw_new && nw_old && cur);
        if (cauchy)
                gf_gen_cauchy1_matrix(a, m, k);
        else
                gf_gen_rs_matrix(a, m, k);
        ec_init_tables(k, rows, a + (size_t) k * k, g);
        for (l = 0; l < rows; l++)
                want[l] = shard(len);
        for (s = 0; s < nstripes; s++) {
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
                /* nw distinct indices in a random order */
                for (i = 0; i < nw; i++) {
                        do {
                                idx[s * nw + i] = (unsigned char) rnd((unsigned) k);
                                for (j = 0; j < i && idx[s * nw + j] != idx[s * nw + i]; j++)
                                        ;
                        } while (j < i);
                        nw_old[s * nw + i] = data[s * k + idx[s * nw + i]];
                        nw_new[s * nw + i] = shard(len);
                        for (b = 0; b < len; b++)
                                nw_new[s * nw + i][b] = (unsigned char) rnd(256);
                }
        }
        CHECK(isal_hip_overwrite_create(&o, len, k, rows, g, nw, nstripes, idx, nw_old, nw_new, par, &bad) ==
              ISAL_HIP_OK);
        CHECK(o && bad == -1);
        CHECK(isal_hip_overwrite_run(o, 2, NULL) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_overwrite_run(o, ~0, NULL) == ISAL_HIP_EINVAL);
        /* twice without commit: the parity comes back, the data never moved */
        g_launches = g_commits = 0;
        CHECK(isal_hip_overwrite_run(o, 0, NULL) == ISAL_HIP_OK);
        CHECK(isal_hip_overwrite_run(o, 0, NULL) == ISAL_HIP_OK);
        CHECK(g_launches == 2 && g_commits == 0);
        for (i = 0; i < nstripes * rows; i++)
                CHECK(memcmp(par[i], par0[i], (size_t) len) == 0);
        /* committed: the parity of the stripe with the new bytes in place */
        CHECK(isal_hip_overwrite_run(o, ISAL_HIP_OVERWRITE_COMMIT, NULL) == ISAL_HIP_OK);
        CHECK(g_commits == 1);
        for (s = 0; s < nstripes; s++) {
                for (j = 0; j < k; j++)
                        cur[j] = data[s * k + j];
                for (i = 0; i < nw; i++) {
                        cur[idx[s * nw + i]] = nw_new[s * nw + i];
                        CHECK(memcmp(nw_old[s * nw + i], nw_new[s * nw + i], (size_t) len) == 0);
                }
                encode(a, k, rows, len, cur, want);
                for (l = 0; l < rows; l++)
                        CHECK(memcmp(par[s * rows + l], want[l], (size_t) len) == 0);
        }
        CHECK(isal_hip_overwrite_destroy(o) == ISAL_HIP_OK);
        printf("  %s k=%d rows=%d nw=%d stripes=%d len=%d: %d pass(es), parity as a fresh encode\n",
               cauchy ? "cauchy" : "rs", k, rows, nw, nstripes, len, passes);
        for (i = 0; i < nstripes * k; i++)
                free(data[i]);
        for (i = 0; i < nstripes * rows; i++) {
                free(par[i]);
                free(par0[i]);
        }
        for (i = 0; i < nstripes * nw; i++)
                free(nw_new[i]);
        for (l = 0; l < rows; l++)
                free(want[l]);
        free(a);
        free(g);
        free(idx);
        free(data);
        free(par);
        free(par0);
        free(want);
        free(nw_new);
        free(nw_old);
        free(cur);
}

static void
error_paths(void)
{
        enum { K = 10, R = 4, NW = 3, S = 6, LEN = 64, N = S * (2 * NW + R) };
        unsigned char a[(K + R) * K], g[32 * K * R], idx[S * NW];
        unsigned char *buf, *od[S * NW], *nd[S * NW], *cd[S * R], *keep;
        isal_hip_overwrite *o;
        int s, i, bad, n = 0;
        CHECK(posix_memalign((void **) &buf, 16, (size_t) N * LEN) == 0);
        gf_gen_rs_matrix(a, K + R, K);
        ec_init_tables(K, R, a + K * K, g);
        for (s = 0; s < S; s++) {
                for (i = 0; i < NW; i++) {
                        idx[s * NW + i] = (unsigned char) ((s + 3 * i) % K);
                        od[s * NW + i] = buf + (size_t) LEN * n++;
                        nd[s * NW + i] = buf + (size_t) LEN * n++;
                }
                for (i = 0; i < R; i++)
                        cd[s * R + i] = buf + (size_t) LEN * n++;
        }
#define CREATE(len, k, rows, g_, nw, ns, ix, o_, n_, c_) \
        (o = (isal_hip_overwrite *) buf, bad = -9,      \
         isal_hip_overwrite_create(&o, len, k, rows, g_, nw, ns, ix, o_, n_, c_, &bad))
#define REFUSED(expr, stripe) CHECK((expr) == ISAL_HIP_EINVAL && o == NULL && bad == (stripe))
        CHECK(isal_hip_overwrite_create(NULL, LEN, K, R, g, NW, S, idx, od, nd, cd, &bad) == ISAL_HIP_EINVAL);
        REFUSED(CREATE(LEN, K, R, NULL, NW, S, idx, od, nd, cd), -1);
        REFUSED(CREATE(LEN, K, R, g, NW, S, NULL, od, nd, cd), -1);
        REFUSED(CREATE(LEN, K, R, g, NW, S, idx, NULL, nd, cd), -1);
        REFUSED(CREATE(LEN, K, R, g, NW, S, idx, od, NULL, cd), -1);
        REFUSED(CREATE(LEN, K, R, g, NW, S, idx, od, nd, NULL), -1);
        REFUSED(CREATE(LEN, K, R, g, 0, S, idx, od, nd, cd), -1);
        REFUSED(CREATE(LEN, K, R, g, K + 1, S, idx, od, nd, cd), -1);
        REFUSED(CREATE(-1, K, R, g, NW, S, idx, od, nd, cd), -1);
        REFUSED(CREATE(LEN, K, R, g, NW, 0, idx, od, nd, cd), -1);
        REFUSED(CREATE(LEN, K, 0, g, NW, S, idx, od, nd, cd), -1);
        idx[4 * NW + 1] = K; /* index >= k in stripe 4 */
        REFUSED(CREATE(LEN, K, R, g, NW, S, idx, od, nd, cd), 4);
        idx[2 * NW + 2] = idx[2 * NW + 0]; /* a duplicate in stripe 2 comes first */
        REFUSED(CREATE(LEN, K, R, g, NW, S, idx, od, nd, cd), 2);
        idx[2 * NW + 2] = (unsigned char) ((2 + 3 * 2) % K);
        idx[4 * NW + 1] = (unsigned char) ((4 + 3) % K);
        keep = nd[3 * NW + 1];
        nd[3 * NW + 1] = keep + 8; /* misaligned */
        REFUSED(CREATE(LEN, K, R, g, NW, S, idx, od, nd, cd), 3);
        nd[3 * NW + 1] = NULL;
        REFUSED(CREATE(LEN, K, R, g, NW, S, idx, od, nd, cd), 3);
        nd[3 * NW + 1] = cd[3 * R + 2]; /* new aliases a parity row */
        REFUSED(CREATE(LEN, K, R, g, NW, S, idx, od, nd, cd), 3);
        nd[3 * NW + 1] = keep;
        keep = cd[1 * R + 0];
        cd[1 * R + 0] = od[1 * NW + 2] + 48; /* parity starts inside old's last 16 bytes */
        REFUSED(CREATE(LEN, K, R, g, NW, S, idx, od, nd, cd), 1);
        /* ... which is no overlap for a 16-byte range, and none at len 0 even when equal */
        CHECK(CREATE(16, K, R, g, NW, S, idx, od, nd, cd) == ISAL_HIP_OK && o && bad == -1);
        CHECK(isal_hip_overwrite_destroy(o) == ISAL_HIP_OK);
        cd[1 * R + 0] = od[1 * NW + 2];
        CHECK(CREATE(0, K, R, g, NW, S, idx, od, nd, cd) == ISAL_HIP_OK && o && bad == -1);
        CHECK(isal_hip_overwrite_run(o, ISAL_HIP_OVERWRITE_COMMIT, NULL) == ISAL_HIP_OK);
        CHECK(isal_hip_overwrite_destroy(o) == ISAL_HIP_OK);
        cd[1 * R + 0] = keep;
        /* everything put back: accepted */
        CHECK(CREATE(LEN, K, R, g, NW, S, idx, od, nd, cd) == ISAL_HIP_OK && o && bad == -1);
        CHECK(isal_hip_overwrite_destroy(o) == ISAL_HIP_OK);
        CHECK(isal_hip_overwrite_run(NULL, 0, NULL) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_overwrite_run(NULL, 4, NULL) == ISAL_HIP_EINVAL);
        CHECK(isal_hip_overwrite_destroy(NULL) == ISAL_HIP_OK);
#undef CREATE
#undef REFUSED
        free(buf);
        printf("  error paths: ok\n");
}

int
main(void)
{
        printf("overwrite_host: isal_hip_overwrite.c host logic with stubbed HIP\n");
        error_paths();
        run_geometry(0, 4, 2, 1, 9, 37);
        run_geometry(0, 10, 4, 1, 24, 21);
        run_geometry(0, 10, 4, 3, 24, 19);
        run_geometry(1, 20, 10, 2, 7, 17); /* two passes */
        run_geometry(0, 6, 3, 6, 5, 33);   /* nw = k */
        run_geometry(0, 10, 4, 3, 2, 0);   /* len = 0 */
        printf("overwrite_host: ok (%d stub launches)\n", g_launches);
        return 0;
}
