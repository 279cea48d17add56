/*
 * pipe_host.c — TEST INFRASTRUCTURE: the host pipeline (isa-l_amd/csrc/
 * isal_hip_pipe.c) and the multi-device encode (isal_hip_multi.c) under
 * ASan + UBSan on the deferred model of HIP streams (hip_model.c), as a
 * stand-alone program.
 *
 * On a GPU a missing ordering edge of the pipeline usually still gives the
 * right bytes, and on the complete-at-once runtime of hip_stubs.c it always
 * does. Here nothing runs before the host waits for it, and which of the
 * pipeline's three streams moves next follows a fixed priority order; every
 * scenario runs under all six orders, so an operation that may overtake the
 * one it depends on does so under one of them: parity is then folded from or
 * copied out of poisoned memory. The launches run the CPU route (ec_cpu.c)
 * over the slot's pointer table, so the kernels themselves are not seen here
 * (tests/test_pipe_gpu.py sees them, and cannot see ordering). The checker is
 * the oracle restatement (oracle/ec_oracle.c).
 *
 * Per scenario — mode x len {16, 4099} x depth {1, 2, 4} x stripes {1, depth,
 * 2*depth+1} x source layout x parity layout, a second wave of depth+2 other
 * stripes on the same handle, flushed or left to isal_hip_pipe_destroy:
 *   - every parity byte equals the oracle's; every guard byte around and
 *     between the host shards, and every source byte, is unchanged;
 *   - the H2D and D2H copies enqueued per stripe are exactly the runs of the
 *     layout, each of run*len bytes from the run's first shard (the layouts
 *     below state their runs; nothing is read back from the pipeline);
 *   - one memset of rows*len per stripe in UPDATE mode, k launches per stripe
 *     in UPDATE mode and one in ENCODE mode;
 *   - after flush nothing is queued; after destroy every stream, event and
 *     device allocation is gone.
 * Multi, on the model's three devices: stripes {0, 1, 2, 3, 4, 7} on one
 * handle, call after call; every stripe's operations ran on the device its
 * contiguous range belongs to; ndev = 0 means all three; ndev = 4 is refused.
 *
 * `pipe_host lenient` lifts the model's one-record-per-event discipline (see
 * hip_model.c), to read what else a seeded defect breaks.
 *
 * Built by this directory's Makefile (make -C tests/sanitize) and run by
 * tests/test_sanitizers_cpu.py.
 */
#include "hip_stubs.h"

/* oracle (ec_oracle.c, compiled into this program) */
void oracle_gf_gen_rs_matrix(unsigned char *a, int m, int k);
void oracle_ec_init_tables(int k, int rows, const unsigned char *a, unsigned char *tbls);
void oracle_ec_encode_data(int len, int k, int rows, const unsigned char *tbls, unsigned char *const *src,
                           unsigned char *const *dst);
void oracle_fill_bytes(unsigned char *buf, long long n, unsigned long long seed);

/* k != rows on purpose: an index scaled by the wrong one lands elsewhere */
enum { K = 5, R = 3, GUARD = 64, GUARD_BYTE = 0x5A, FRESH = 0xEE, MAXS = 9, NLEN = 2, NWAVE = 2 };
static const int lens[NLEN] = {16, 4099};

/* Host layouts of the n shards of one stripe, and the runs of shards adjacent
 * in memory AND in index order that each consists of — what the pipeline may
 * move as one copy:
 *   block     adjacent in index order                       one run of n
 *   gapped    a guard between any two                       n runs of 1
 *   reversed  adjacent, at descending addresses             n runs of 1
 *   pairs     runs of two, a guard between runs             n/2 runs of 2 (+ 1 of 1)
 *   aliased   block, but index 2 names shard 0's buffer     {0,1} {2} {3..n-1}
 *             (sources only) */
enum { L_BLOCK, L_GAPPED, L_REVERSED, L_PAIRS, L_ALIASED, NLAYOUTS };
static const char *const layout_name[NLAYOUTS] = {"block", "gapped", "reversed", "pairs", "aliased"};

static size_t
region_bytes(int n, int len)
{
        return (size_t) n * (size_t) (len + GUARD) + GUARD; /* room for any layout */
}

/* shard pointers of one stripe inside its region; returns the number of runs
 * and their lengths in shards */
static int
lay_out(int layout, int n, int len, unsigned char *region, unsigned char **ptr, int *run)
{
        unsigned char *base = region + GUARD;
        int i, nrun = 0;
        switch (layout) {
        case L_BLOCK:
                for (i = 0; i < n; i++)
                        ptr[i] = base + (size_t) i * len;
                run[nrun++] = n;
                break;
        case L_GAPPED:
                for (i = 0; i < n; i++) {
                        ptr[i] = base + (size_t) i * (len + GUARD);
                        run[nrun++] = 1;
                }
                break;
        case L_REVERSED:
                for (i = 0; i < n; i++) {
                        ptr[i] = base + (size_t) (n - 1 - i) * len;
                        run[nrun++] = 1;
                }
                break;
        case L_PAIRS:
                for (i = 0; i < n; i++)
                        ptr[i] = base + (size_t) (i / 2) * (2 * (size_t) len + GUARD) + (size_t) (i % 2) * len;
                for (i = 0; i < n; i += 2)
                        run[nrun++] = n - i >= 2 ? 2 : 1;
                break;
        default: /* L_ALIASED */
                CHECK(n >= 4);
                for (i = 0; i < n; i++)
                        ptr[i] = base + (size_t) i * len;
                ptr[2] = ptr[0];
                run[nrun++] = 2;
                run[nrun++] = 1;
                run[nrun++] = n - 3;
                break;
        }
        return nrun;
}

/* ---- what is right, computed once ------------------------------------------ */

static unsigned char gftbls[32 * K * R];
/* source j of stripe s of a wave, and its parity — plain, and with source 2
 * replaced by source 0 (the aliased layout) */
static unsigned char *g_src[NLEN][NWAVE][MAXS][K];
static unsigned char *g_want[NLEN][NWAVE][2][MAXS][R];

static void
build_expectations(void)
{
        unsigned char a[(K + R) * K];
        int li, w, s, j, al;
        oracle_gf_gen_rs_matrix(a, K + R, K);
        oracle_ec_init_tables(K, R, a + K * K, gftbls);
        for (li = 0; li < NLEN; li++)
                for (w = 0; w < NWAVE; w++)
                        for (s = 0; s < MAXS; s++) {
                                for (j = 0; j < K; j++) {
                                        g_src[li][w][s][j] = shard(lens[li]);
                                        /* different bytes for every shard of every stripe of every wave */
                                        oracle_fill_bytes(g_src[li][w][s][j], lens[li],
                                                          1000003ull * (unsigned) (li * NWAVE + w) + 101ull * (unsigned) s + (unsigned) j);
                                }
                                for (al = 0; al < 2; al++) {
                                        unsigned char *src[K];
                                        for (j = 0; j < K; j++)
                                                src[j] = g_src[li][w][s][al && j == 2 ? 0 : j];
                                        for (j = 0; j < R; j++)
                                                g_want[li][w][al][s][j] = shard(lens[li]);
                                        oracle_ec_encode_data(lens[li], K, R, gftbls, src, g_want[li][w][al][s]);
                                }
                        }
}

static void
free_expectations(void)
{
        int li, w, s, j, al;
        for (li = 0; li < NLEN; li++)
                for (w = 0; w < NWAVE; w++)
                        for (s = 0; s < MAXS; s++) {
                                for (j = 0; j < K; j++)
                                        free(g_src[li][w][s][j]);
                                for (al = 0; al < 2; al++)
                                        for (j = 0; j < R; j++)
                                                free(g_want[li][w][al][s][j]);
                        }
}

/* ---- one wave of host stripes ------------------------------------------------ */

typedef struct {
        int ns, len, sl, pl;
        size_t sreg, preg; /* bytes of one stripe's source / parity region */
        unsigned char *src, *src0, *par, *par_want;
        unsigned char **sp, **pp; /* [ns * K], [ns * R]: exactly that many, ASan guards the ends */
        int srun[MAXS][K], nsrun[MAXS], prun[MAXS][R], nprun[MAXS];
} wave_t;

static void
wave_make(wave_t *w, int li, int wave, int ns, int sl, int pl)
{
        int s, j;
        CHECK(ns <= MAXS);
        memset(w, 0, sizeof(*w));
        w->ns = ns;
        w->len = lens[li];
        w->sl = sl;
        w->pl = pl;
        w->sreg = region_bytes(K, w->len);
        w->preg = region_bytes(R, w->len);
        if (!ns)
                return;
        w->src = malloc(w->sreg * ns);
        w->src0 = malloc(w->sreg * ns);
        w->par = malloc(w->preg * ns);
        w->par_want = malloc(w->preg * ns);
        w->sp = malloc(sizeof(*w->sp) * (size_t) ns * K);
        w->pp = malloc(sizeof(*w->pp) * (size_t) ns * R);
        CHECK(w->src && w->src0 && w->par && w->par_want && w->sp && w->pp);
        memset(w->src, GUARD_BYTE, w->sreg * ns);
        memset(w->par, GUARD_BYTE, w->preg * ns);
        for (s = 0; s < ns; s++) {
                w->nsrun[s] = lay_out(sl, K, w->len, w->src + w->sreg * s, w->sp + (size_t) s * K, w->srun[s]);
                w->nprun[s] = lay_out(pl, R, w->len, w->par + w->preg * s, w->pp + (size_t) s * R, w->prun[s]);
                for (j = 0; j < K; j++)
                        if (!(sl == L_ALIASED && j == 2))
                                memcpy(w->sp[s * K + j], g_src[li][wave][s][j], (size_t) w->len);
        }
        memcpy(w->src0, w->src, w->sreg * ns);
        memcpy(w->par_want, w->par, w->preg * ns);
        for (s = 0; s < ns; s++)
                for (j = 0; j < R; j++) {
                        memset(w->pp[s * R + j], FRESH, (size_t) w->len);
                        memcpy(w->par_want + (w->pp[s * R + j] - w->par), g_want[li][wave][sl == L_ALIASED][s][j],
                               (size_t) w->len);
                }
}

static void
wave_free(wave_t *w)
{
        free(w->src);
        free(w->src0);
        free(w->par);
        free(w->par_want);
        free(w->sp);
        free(w->pp);
}

/* ---- reporting ----------------------------------------------------------------- */

static char g_what[256];
static int g_done;

static void
say_where(void)
{
        if (!g_done)
                fprintf(stderr, "pipe_host: FAILED in %s\n", g_what);
}

#define EXPECT(c)                                                            \
        do {                                                                 \
                if (!(c)) {                                                  \
                        fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
                        exit(1);                                             \
                }                                                            \
        } while (0)

static void
check_bytes(const wave_t *w)
{
        size_t i;
        if (!w->ns)
                return;
        if (memcmp(w->src, w->src0, w->sreg * w->ns)) {
                fprintf(stderr, "a source byte or a guard byte between sources changed\n");
                exit(1);
        }
        for (i = 0; i < w->preg * w->ns; i++)
                if (w->par[i] != w->par_want[i]) {
                        const size_t s = i / w->preg;
                        int l, row = -1;
                        for (l = 0; l < R; l++)
                                if (w->par + i >= w->pp[s * R + l] && w->par + i < w->pp[s * R + l] + w->len)
                                        row = l;
                        fprintf(stderr, "stripe %zu: %s %d is 0x%02x, not 0x%02x\n", s,
                                row >= 0 ? "a byte of parity row" : "a guard byte, region offset",
                                row >= 0 ? row : (int) (i % w->preg), w->par[i], w->par_want[i]);
                        exit(1);
                }
}

/* The copies enqueued since the logs were emptied, stream by stream in order,
 * are the runs of the waves' layouts; dev < 0: on whichever device */
static void
check_copies(const wave_t *const *waves, int nwaves, int mode)
{
        const hm_rec *log;
        const size_t n = hm_log(HM_ENQUEUED, &log);
        size_t i, ih = 0, id = 0, sets = 0, launches = 0, stripes = 0;
        int wv, s, r;
        for (wv = 0; wv < nwaves; wv++) {
                const wave_t *w = waves[wv];
                stripes += (size_t) w->ns;
                for (s = 0; s < w->ns; s++) {
                        int at = 0;
                        for (r = 0; r < w->nsrun[s]; r++) {
                                while (ih < n && log[ih].kind != HM_H2D)
                                        ih++;
                                EXPECT(ih < n && log[ih].role == HM_ROLE_H2D);
                                EXPECT(log[ih].host == w->sp[s * K + at]);
                                EXPECT(log[ih].n == (size_t) w->srun[s][r] * w->len);
                                at += w->srun[s][r];
                                ih++;
                        }
                        EXPECT(at == K);
                        at = 0;
                        for (r = 0; r < w->nprun[s]; r++) {
                                while (id < n && log[id].kind != HM_D2H)
                                        id++;
                                EXPECT(id < n && log[id].role == HM_ROLE_D2H);
                                EXPECT(log[id].host == w->pp[s * R + at]);
                                EXPECT(log[id].n == (size_t) w->prun[s][r] * w->len);
                                at += w->prun[s][r];
                                id++;
                        }
                        EXPECT(at == R);
                }
        }
        for (; ih < n; ih++)
                EXPECT(log[ih].kind != HM_H2D); /* and no copy more */
        for (; id < n; id++)
                EXPECT(log[id].kind != HM_D2H);
        for (i = 0; i < n; i++) {
                if (log[i].kind == HM_MEMSET) {
                        EXPECT(log[i].role == HM_ROLE_COMP && log[i].n == (size_t) R * waves[0]->len);
                        sets++;
                }
                if (log[i].kind == HM_LAUNCH) {
                        EXPECT(log[i].role == HM_ROLE_COMP);
                        launches++;
                }
        }
        EXPECT(sets == (mode == ISAL_HIP_PIPE_UPDATE ? stripes : 0));
        EXPECT(launches == (mode == ISAL_HIP_PIPE_UPDATE ? stripes * K : stripes));
}

/* everything enqueued has run, and nothing else */
static void
check_drained(void)
{
        const hm_rec *log;
        const size_t n = hm_log(HM_ENQUEUED, &log);
        EXPECT(hm_pending(-1) == 0);
        EXPECT(hm_log(HM_EXECUTED, &log) == n);
}

/* ---- the pipeline ------------------------------------------------------------- */

static long g_scenarios;

static void
pipe_scenario(int mode, int li, int depth, int ns, int sl, int pl, int noflush)
{
        const int allocs0 = g_allocs;
        isal_hip_pipe *p = NULL;
        wave_t w0, w1;
        const wave_t *both[2] = {&w0, &w1};
        int s;
        hm_log_clear();
        EXPECT(isal_hip_pipe_create(&p, lens[li], K, R, gftbls, depth, mode) == ISAL_HIP_OK && p);
        EXPECT(hm_live_streams() == 3 && hm_live_events() == depth * (K + 2));
        wave_make(&w0, li, 0, ns, sl, pl);
        for (s = 0; s < ns; s++)
                EXPECT(isal_hip_pipe_submit(p, w0.sp + (size_t) s * K, w0.pp + (size_t) s * R) == ISAL_HIP_OK);
        EXPECT(isal_hip_pipe_flush(p) == ISAL_HIP_OK);
        check_drained();
        check_bytes(&w0);
        /* other stripes into fresh parity buffers: the slot phase goes on mid-cycle */
        wave_make(&w1, li, 1, depth + 2, sl, pl);
        for (s = 0; s < w1.ns; s++)
                EXPECT(isal_hip_pipe_submit(p, w1.sp + (size_t) s * K, w1.pp + (size_t) s * R) == ISAL_HIP_OK);
        if (!noflush) {
                EXPECT(isal_hip_pipe_flush(p) == ISAL_HIP_OK);
                check_drained();
                EXPECT(isal_hip_pipe_flush(p) == ISAL_HIP_OK); /* and again, with nothing queued */
                check_bytes(&w1);
        }
        EXPECT(isal_hip_pipe_destroy(p) == ISAL_HIP_OK); /* drains what is queued */
        check_drained();
        check_bytes(&w1);
        check_bytes(&w0); /* the second wave wrote nothing of the first */
        check_copies(both, 2, mode);
        EXPECT(g_allocs == allocs0 && hm_live_streams() == 0 && hm_live_events() == 0);
        wave_free(&w0);
        wave_free(&w1);
        g_scenarios++;
}

static void
pipe_scenarios(const int order[3])
{
        static const int depths[3] = {1, 2, 4};
        int mode, li, di, si, sl, pl, noflush;
        for (mode = ISAL_HIP_PIPE_UPDATE; mode <= ISAL_HIP_PIPE_ENCODE; mode++)
                for (li = 0; li < NLEN; li++)
                        for (di = 0; di < 3; di++)
                                for (si = 0; si < 3; si++) {
                                        const int d = depths[di], ns = si == 0 ? 1 : si == 1 ? d : 2 * d + 1;
                                        if (si == 1 && d == 1)
                                                continue; /* 1 stripe again */
                                        for (sl = 0; sl < NLAYOUTS; sl++)
                                                for (pl = 0; pl < L_ALIASED; pl++)
                                                        for (noflush = 0; noflush < 2; noflush++) {
                                                                snprintf(g_what, sizeof(g_what),
                                                                         "pipe: order %d%d%d (0 h2d, 1 compute, 2 d2h; first moves first) "
                                                                         "mode %s len %d depth %d stripes %d sources %s parity %s%s",
                                                                         order[0], order[1], order[2],
                                                                         mode == ISAL_HIP_PIPE_UPDATE ? "update" : "encode", lens[li], d,
                                                                         ns, layout_name[sl], layout_name[pl],
                                                                         noflush ? ", second wave destroyed unflushed" : "");
                                                                pipe_scenario(mode, li, d, ns, sl, pl, noflush);
                                                        }
                                }
}

/* a handle with nothing submitted: flush twice, destroy */
static void
pipe_idle(void)
{
        const int allocs0 = g_allocs;
        isal_hip_pipe *p = NULL;
        snprintf(g_what, sizeof(g_what), "pipe: nothing submitted");
        EXPECT(isal_hip_pipe_create(&p, 4099, K, R, gftbls, 9, ISAL_HIP_PIPE_UPDATE) == ISAL_HIP_OK);
        EXPECT(hm_live_events() == ISAL_HIP_PIPE_MAX_DEPTH * (K + 2)); /* depth 9 is capped */
        EXPECT(isal_hip_pipe_flush(p) == ISAL_HIP_OK && isal_hip_pipe_flush(p) == ISAL_HIP_OK);
        EXPECT(isal_hip_pipe_destroy(p) == ISAL_HIP_OK);
        EXPECT(g_allocs == allocs0 && hm_live_streams() == 0 && hm_live_events() == 0);
}

/* ---- multi-device --------------------------------------------------------------- */

/* the device whose contiguous range [S*d/G, S*(d+1)/G) holds stripe s */
static int
owner(int S, int G, int s)
{
        int d;
        for (d = 0; d < G; d++)
                if (s >= S * d / G && s < S * (d + 1) / G)
                        return d;
        return -1;
}

static void
multi_scenarios(const int order[3])
{
        static const int counts[6] = {0, 1, 2, 3, 4, 7};
        const int allocs0 = g_allocs;
        int li, ci, d, s, calls = 0;
        for (li = 0; li < NLEN; li++) {
                isal_hip_multi *m = NULL, *m4 = (isal_hip_multi *) &li;
                const int ndev_arg = li ? 0 : HM_NDEV; /* 0: every device */
                snprintf(g_what, sizeof(g_what), "multi: order %d%d%d len %d create", order[0], order[1], order[2],
                         lens[li]);
                EXPECT(isal_hip_multi_create(&m4, HM_NDEV + 1, lens[li], K, R, gftbls, 2) == ISAL_HIP_EINVAL && !m4);
                EXPECT(g_allocs == allocs0 && hm_live_streams() == 0);
                EXPECT(isal_hip_multi_create(&m, ndev_arg, lens[li], K, R, gftbls, 2) == ISAL_HIP_OK && m);
                EXPECT(isal_hip_multi_ndev(m) == HM_NDEV && hm_live_streams() == 3 * HM_NDEV);
                for (d = 0; d < HM_NDEV; d++) /* no such bus id in sysfs: not pinned */
                        EXPECT(isal_hip_multi_numa_node(m, d) == -1 && isal_hip_multi_worker_cpus(m, d) == 0);
                for (ci = 0; ci < 6; ci++, calls++) {
                        const int S = counts[ci];
                        const hm_rec *log;
                        size_t n, i;
                        int h2d[MAXS] = {0}, d2h[MAXS] = {0}, launches[HM_NDEV] = {0};
                        wave_t w;
                        snprintf(g_what, sizeof(g_what), "multi: order %d%d%d len %d, call %d on the handle: %d stripes",
                                 order[0], order[1], order[2], lens[li], ci, S);
                        wave_make(&w, li, calls & 1, S, L_GAPPED, L_PAIRS); /* other data than the call before */
                        hm_log_clear();
                        EXPECT(isal_hip_multi_encode(m, S, w.sp, w.pp) == ISAL_HIP_OK);
                        check_drained();
                        check_bytes(&w);
                        n = hm_log(HM_EXECUTED, &log);
                        for (i = 0; i < n; i++) {
                                if (log[i].kind == HM_H2D) {
                                        s = (int) ((size_t) ((const unsigned char *) log[i].host - w.src) / w.sreg);
                                        EXPECT(s >= 0 && s < S && log[i].dev == owner(S, HM_NDEV, s));
                                        h2d[s]++;
                                } else if (log[i].kind == HM_D2H) {
                                        s = (int) ((size_t) ((const unsigned char *) log[i].host - w.par) / w.preg);
                                        EXPECT(s >= 0 && s < S && log[i].dev == owner(S, HM_NDEV, s));
                                        d2h[s]++;
                                } else if (log[i].kind == HM_LAUNCH)
                                        launches[log[i].dev]++;
                                else
                                        EXPECT(log[i].kind != HM_MEMSET); /* the multi pipelines encode */
                        }
                        for (s = 0; s < S; s++)
                                EXPECT(h2d[s] == w.nsrun[s] && d2h[s] == w.nprun[s]);
                        for (d = 0; d < HM_NDEV; d++) {
                                long long first, count;
                                isal_hip_multi_partition(S, HM_NDEV, d, &first, &count);
                                EXPECT(first == S * d / HM_NDEV && count == S * (d + 1) / HM_NDEV - S * d / HM_NDEV);
                                EXPECT(launches[d] == count); /* one encode per stripe, on its own device */
                        }
                        wave_free(&w);
                        g_scenarios++;
                }
                EXPECT(isal_hip_multi_destroy(m) == ISAL_HIP_OK);
                EXPECT(g_allocs == allocs0 && hm_live_streams() == 0 && hm_live_events() == 0);
        }
}

int
main(int argc, char **argv)
{
        static const int orders[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        int o;
        atexit(say_where);
        setenv("ISAL_HIP_SYSFS_ROOT", "/nonexistent/sysfs", 1);
        snprintf(g_what, sizeof(g_what), "building what is right");
        build_expectations();
        for (o = 0; o < 6; o++) {
                hm_start(orders[o]);
                hm_strict_events(!(argc > 1 && !strcmp(argv[1], "lenient")));
                pipe_idle();
                pipe_scenarios(orders[o]);
                multi_scenarios(orders[o]);
                hm_stop();
        }
        free_expectations();
        g_done = 1;
        printf("pipe_host: ok (%ld scenarios under each of the 6 stream priority orders)\n", g_scenarios / 6);
        return 0;
}
