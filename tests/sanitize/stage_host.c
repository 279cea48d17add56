/*
 * stage_host.c — TEST INFRASTRUCTURE: the drop-in shim's host staging routes
 * (isa-l_amd/csrc/isal_hip_stage.c on the real per-thread context of
 * isal_hip_ctx.c) under ASan + UBSan, as a stand-alone program: the pointer
 * table, the copy-in and copy-out walks, the copy-out worker thread, and the
 * bookkeeping of a failure — (done, chunk_end, rows_out) — that decides which
 * bytes the CPU completion may write.
 *
 * The HIP runtime and the plain kernel launchers are the stubs of hip_stubs.c:
 * "device" memory is host memory, every copy and kernel completes at once,
 * and a launch runs the CPU route (ec_cpu.c) over the pointer table and the
 * coefficient tables the route uploaded. So a run's outputs are right only if
 * every pointer, slot and copy of the route is.
 *
 * Every run is completed the way run_ec completes a call (isal_hip_shim.c):
 * when the route fails — ISAL_HIP_FAULT sites 1-5, in chunk 0 or 1 — through
 * isal_hip_finish_on_cpu. The result must equal the CPU route's on the same
 * inputs (for an update that proves no row was folded twice), the guard bytes
 * past every shard must be untouched, and the failure's (err != 0, done,
 * chunk_end, rows_out) must be the tuple of the table below. The table was
 * recorded from the routes as they were before they were split out of
 * isal_hip_shim.c (this driver built against that file), so it pins their
 * failure bookkeeping.
 *
 * Built by this directory's Makefile (make -C tests/sanitize) and run by
 * tests/test_sanitizers_cpu.py.
 */
#include <pthread.h>

#include "hip_stubs.h"
#include "isal_hip_shim.h"

enum { K = 3, R = 2, GUARD = 32 };
/* ISAL_HIP_CHUNK_KB=4: the pipelined route cuts this into 4096 + 4096 + 100
 * columns, the last chunk short and no multiple of 16; the whole-shard routes
 * take it in one piece */
#define LEN_SMALL (2 * 4096 + 100)
/* ISAL_HIP_STAGE_MB=1 makes the chunked routes cut columns as well: at most
 * (1 MiB / staged shards) & ~4095 columns per chunk, so two chunks or more,
 * the last one short and no multiple of 16 */
#define LEN_CHUNKED (2 * 348160 + 100)

enum { ZC, PACKED, SERIAL, HELPER, PIPED, NROUTES };
static const char *const route_name[NROUTES] = {"zero-copy", "packed", "chunked", "chunked+helper", "pipelined"};

/* Which shards a kernel reaches in place ("device" views; the rest is staged):
 *   ENC_MIXED  encode, source 0 and output row 0 in place: one staged output
 *   ENC_STAGED encode, everything staged: both copy lists of the helper fill
 *   UPD        update, its source in place and both parity rows staged (an
 *              update's host parity always is): row 1 is the FAULT_D2H site
 *   VER        verify, source 0 and stored row 0 in place, a mismatch planted
 *              in the last chunk */
enum { ENC_MIXED, ENC_STAGED, UPD, VER, NCASES };
static const char *const case_name[NCASES] = {"encode (mixed)", "encode (staged)", "update", "verify"};
static const int case_op[NCASES] = {OP_ENCODE, OP_ENCODE, OP_UPDATE, OP_VERIFY};

/* (err != 0, done, chunk_end, rows_out) of every failing run, in the order
 * main() makes them: case, route, site, chunk */
static const struct {
        signed char kase, route, site, chunk, failed;
        long long done, chunk_end;
        int rows_out;
} expect[] = {
        {0, 0, 1, 0, 1, 0, 0, 0},
        {0, 0, 1, 1, 0, 8292, 0, 0},
        {0, 0, 2, 0, 0, 8292, 0, 0},
        {0, 0, 2, 1, 0, 8292, 0, 0},
        {0, 0, 3, 0, 1, 0, 0, 0},
        {0, 0, 3, 1, 0, 8292, 0, 0},
        {0, 0, 4, 0, 0, 8292, 0, 0},
        {0, 0, 4, 1, 0, 8292, 0, 0},
        {0, 0, 5, 0, 1, 0, 0, 0},
        {0, 0, 5, 1, 0, 8292, 0, 0},
        {0, 1, 1, 0, 1, 0, 0, 0},
        {0, 1, 1, 1, 0, 8292, 0, 0},
        {0, 1, 2, 0, 1, 0, 0, 0},
        {0, 1, 2, 1, 0, 8292, 0, 0},
        {0, 1, 3, 0, 1, 0, 0, 0},
        {0, 1, 3, 1, 0, 8292, 0, 0},
        {0, 1, 4, 0, 1, 0, 0, 0},
        {0, 1, 4, 1, 0, 8292, 0, 0},
        {0, 1, 5, 0, 1, 0, 0, 0},
        {0, 1, 5, 1, 0, 8292, 0, 0},
        {0, 2, 1, 0, 1, 0, 0, 0},
        {0, 2, 1, 1, 0, 696420, 0, 0},
        {0, 2, 2, 0, 1, 0, 0, 0},
        {0, 2, 2, 1, 1, 348160, 348160, 0},
        {0, 2, 3, 0, 1, 0, 0, 0},
        {0, 2, 3, 1, 1, 348160, 348160, 0},
        {0, 2, 4, 0, 1, 0, 348160, 0},
        {0, 2, 4, 1, 1, 348160, 696320, 0},
        {0, 2, 5, 0, 1, 0, 348160, 2},
        {0, 2, 5, 1, 1, 348160, 696320, 2},
        {0, 3, 1, 0, 1, 0, 0, 0},
        {0, 3, 1, 1, 0, 696420, 0, 0},
        {0, 3, 2, 0, 1, 0, 0, 0},
        {0, 3, 2, 1, 1, 348160, 348160, 0},
        {0, 3, 3, 0, 1, 0, 0, 0},
        {0, 3, 3, 1, 1, 348160, 348160, 0},
        {0, 3, 4, 0, 0, 696420, 0, 0},
        {0, 3, 4, 1, 0, 696420, 0, 0},
        {0, 3, 5, 0, 1, 0, 348160, 1},
        {0, 3, 5, 1, 1, 348160, 696320, 1},
        {0, 4, 1, 0, 1, 0, 0, 0},
        {0, 4, 1, 1, 0, 8292, 0, 0},
        {0, 4, 2, 0, 1, 0, 0, 0},
        {0, 4, 2, 1, 1, 4096, 0, 0},
        {0, 4, 3, 0, 1, 0, 0, 0},
        {0, 4, 3, 1, 1, 4096, 0, 0},
        {0, 4, 4, 0, 1, 0, 4096, 0},
        {0, 4, 4, 1, 1, 4096, 8192, 0},
        {0, 4, 5, 0, 0, 8292, 0, 0},
        {0, 4, 5, 1, 0, 8292, 0, 0},
        {1, 0, 1, 0, 1, 0, 0, 0},
        {1, 0, 1, 1, 0, 8292, 0, 0},
        {1, 0, 2, 0, 0, 8292, 0, 0},
        {1, 0, 2, 1, 0, 8292, 0, 0},
        {1, 0, 3, 0, 1, 0, 0, 0},
        {1, 0, 3, 1, 0, 8292, 0, 0},
        {1, 0, 4, 0, 0, 8292, 0, 0},
        {1, 0, 4, 1, 0, 8292, 0, 0},
        {1, 0, 5, 0, 1, 0, 0, 0},
        {1, 0, 5, 1, 0, 8292, 0, 0},
        {1, 1, 1, 0, 1, 0, 0, 0},
        {1, 1, 1, 1, 0, 8292, 0, 0},
        {1, 1, 2, 0, 1, 0, 0, 0},
        {1, 1, 2, 1, 0, 8292, 0, 0},
        {1, 1, 3, 0, 1, 0, 0, 0},
        {1, 1, 3, 1, 0, 8292, 0, 0},
        {1, 1, 4, 0, 1, 0, 0, 0},
        {1, 1, 4, 1, 0, 8292, 0, 0},
        {1, 1, 5, 0, 1, 0, 0, 0},
        {1, 1, 5, 1, 0, 8292, 0, 0},
        {1, 2, 1, 0, 1, 0, 0, 0},
        {1, 2, 1, 1, 0, 696420, 0, 0},
        {1, 2, 2, 0, 1, 0, 0, 0},
        {1, 2, 2, 1, 1, 208896, 208896, 0},
        {1, 2, 3, 0, 1, 0, 0, 0},
        {1, 2, 3, 1, 1, 208896, 208896, 0},
        {1, 2, 4, 0, 1, 0, 208896, 1},
        {1, 2, 4, 1, 1, 208896, 417792, 1},
        {1, 2, 5, 0, 1, 0, 208896, 2},
        {1, 2, 5, 1, 1, 208896, 417792, 2},
        {1, 3, 1, 0, 1, 0, 0, 0},
        {1, 3, 1, 1, 0, 696420, 0, 0},
        {1, 3, 2, 0, 1, 0, 0, 0},
        {1, 3, 2, 1, 1, 208896, 208896, 0},
        {1, 3, 3, 0, 1, 0, 0, 0},
        {1, 3, 3, 1, 1, 208896, 208896, 0},
        {1, 3, 4, 0, 0, 696420, 0, 0},
        {1, 3, 4, 1, 0, 696420, 0, 0},
        {1, 3, 5, 0, 1, 0, 208896, 1},
        {1, 3, 5, 1, 1, 208896, 417792, 1},
        {1, 4, 1, 0, 1, 0, 0, 0},
        {1, 4, 1, 1, 0, 8292, 0, 0},
        {1, 4, 2, 0, 1, 0, 0, 0},
        {1, 4, 2, 1, 1, 4096, 0, 0},
        {1, 4, 3, 0, 1, 0, 0, 0},
        {1, 4, 3, 1, 1, 4096, 0, 0},
        {1, 4, 4, 0, 1, 0, 4096, 1},
        {1, 4, 4, 1, 1, 4096, 8192, 1},
        {1, 4, 5, 0, 0, 8292, 0, 0},
        {1, 4, 5, 1, 0, 8292, 0, 0},
        {2, 0, 1, 0, 1, 0, 0, 0},
        {2, 0, 1, 1, 0, 8292, 0, 0},
        {2, 0, 2, 0, 0, 8292, 0, 0},
        {2, 0, 2, 1, 0, 8292, 0, 0},
        {2, 0, 3, 0, 1, 0, 0, 0},
        {2, 0, 3, 1, 0, 8292, 0, 0},
        {2, 0, 4, 0, 0, 8292, 0, 0},
        {2, 0, 4, 1, 0, 8292, 0, 0},
        {2, 0, 5, 0, 1, 0, 0, 0},
        {2, 0, 5, 1, 0, 8292, 0, 0},
        {2, 1, 1, 0, 1, 0, 0, 0},
        {2, 1, 1, 1, 0, 8292, 0, 0},
        {2, 1, 2, 0, 1, 0, 0, 0},
        {2, 1, 2, 1, 0, 8292, 0, 0},
        {2, 1, 3, 0, 1, 0, 0, 0},
        {2, 1, 3, 1, 0, 8292, 0, 0},
        {2, 1, 4, 0, 1, 0, 0, 0},
        {2, 1, 4, 1, 0, 8292, 0, 0},
        {2, 1, 5, 0, 1, 0, 0, 0},
        {2, 1, 5, 1, 0, 8292, 0, 0},
        {2, 2, 1, 0, 1, 0, 0, 0},
        {2, 2, 1, 1, 0, 696420, 0, 0},
        {2, 2, 2, 0, 1, 0, 0, 0},
        {2, 2, 2, 1, 1, 524288, 524288, 0},
        {2, 2, 3, 0, 1, 0, 0, 0},
        {2, 2, 3, 1, 1, 524288, 524288, 0},
        {2, 2, 4, 0, 1, 0, 524288, 1},
        {2, 2, 4, 1, 1, 524288, 696420, 1},
        {2, 2, 5, 0, 1, 0, 524288, 2},
        {2, 2, 5, 1, 1, 524288, 696420, 2},
        {2, 3, 1, 0, 1, 0, 0, 0},
        {2, 3, 1, 1, 0, 696420, 0, 0},
        {2, 3, 2, 0, 1, 0, 0, 0},
        {2, 3, 2, 1, 1, 524288, 524288, 0},
        {2, 3, 3, 0, 1, 0, 0, 0},
        {2, 3, 3, 1, 1, 524288, 524288, 0},
        {2, 3, 4, 0, 1, 0, 524288, 1},
        {2, 3, 4, 1, 1, 524288, 696420, 1},
        {2, 3, 5, 0, 1, 0, 524288, 2},
        {2, 3, 5, 1, 1, 524288, 696420, 2},
        {2, 4, 1, 0, 1, 0, 0, 0},
        {2, 4, 1, 1, 0, 8292, 0, 0},
        {2, 4, 2, 0, 1, 0, 0, 0},
        {2, 4, 2, 1, 1, 4096, 0, 0},
        {2, 4, 3, 0, 1, 0, 0, 0},
        {2, 4, 3, 1, 1, 4096, 0, 0},
        {2, 4, 4, 0, 1, 0, 4096, 1},
        {2, 4, 4, 1, 1, 4096, 8192, 1},
        {2, 4, 5, 0, 0, 8292, 0, 0},
        {2, 4, 5, 1, 0, 8292, 0, 0},
        {3, 0, 1, 0, 1, 0, 0, 0},
        {3, 0, 1, 1, 0, 8292, 0, 0},
        {3, 0, 2, 0, 0, 8292, 0, 0},
        {3, 0, 2, 1, 0, 8292, 0, 0},
        {3, 0, 3, 0, 1, 0, 0, 0},
        {3, 0, 3, 1, 0, 8292, 0, 0},
        {3, 0, 4, 0, 0, 8292, 0, 0},
        {3, 0, 4, 1, 0, 8292, 0, 0},
        {3, 0, 5, 0, 1, 0, 0, 0},
        {3, 0, 5, 1, 0, 8292, 0, 0},
        {3, 1, 1, 0, 1, 0, 0, 0},
        {3, 1, 1, 1, 0, 8292, 0, 0},
        {3, 1, 2, 0, 1, 0, 0, 0},
        {3, 1, 2, 1, 0, 8292, 0, 0},
        {3, 1, 3, 0, 1, 0, 0, 0},
        {3, 1, 3, 1, 0, 8292, 0, 0},
        {3, 1, 4, 0, 0, 8292, 0, 0},
        {3, 1, 4, 1, 0, 8292, 0, 0},
        {3, 1, 5, 0, 1, 0, 0, 0},
        {3, 1, 5, 1, 0, 8292, 0, 0},
        {3, 2, 1, 0, 1, 0, 0, 0},
        {3, 2, 1, 1, 0, 696420, 0, 0},
        {3, 2, 2, 0, 1, 0, 0, 0},
        {3, 2, 2, 1, 1, 348160, 0, 0},
        {3, 2, 3, 0, 1, 0, 0, 0},
        {3, 2, 3, 1, 1, 348160, 0, 0},
        {3, 2, 4, 0, 0, 696420, 0, 0},
        {3, 2, 4, 1, 0, 696420, 0, 0},
        {3, 2, 5, 0, 0, 696420, 0, 0},
        {3, 2, 5, 1, 0, 696420, 0, 0},
        {3, 3, 1, 0, 1, 0, 0, 0},
        {3, 3, 1, 1, 0, 696420, 0, 0},
        {3, 3, 2, 0, 1, 0, 0, 0},
        {3, 3, 2, 1, 1, 348160, 0, 0},
        {3, 3, 3, 0, 1, 0, 0, 0},
        {3, 3, 3, 1, 1, 348160, 0, 0},
        {3, 3, 4, 0, 0, 696420, 0, 0},
        {3, 3, 4, 1, 0, 696420, 0, 0},
        {3, 3, 5, 0, 0, 696420, 0, 0},
        {3, 3, 5, 1, 0, 696420, 0, 0},
};
static size_t g_next;
/* STAGE_HOST_RECORD=1: print the table's rows instead of checking them */
static int g_record;

static unsigned char g_tbls[32 * K * R];

static void
knob(const char *name, int v)
{
        char s[16];
        snprintf(s, sizeof(s), "%d", v);
        if (v < 0)
                unsetenv(name);
        else
                setenv(name, s, 1);
}

static gpu_res
attempt(int route, ctx_t *c, const ec_call *q)
{
        knob("ISAL_HIP_PAR_COPY", route == HELPER);
        isal_hip_config_reload();
        switch (route) {
        case ZC:
                return isal_hip_gpu_small(c, q, 1);
        case PACKED:
                return isal_hip_gpu_small(c, q, 0);
        case PIPED:
                return isal_hip_gpu_pipelined(c, q);
        default:
                return isal_hip_gpu_chunked(c, q);
        }
}

static void
one_run(ctx_t *c, int kase, int route, int site, int chunk)
{
        const int op = case_op[kase], nsrc = op == OP_UPDATE ? 1 : K, nptr = nsrc + R;
        const int len = route == SERIAL || route == HELPER ? LEN_CHUNKED : LEN_SMALL;
        const unsigned long long planted = ((unsigned long long) (len - 3) << 8) | 1;
        unsigned char *sh[K + R], *orig[K + R], *want[R], *src_ref[K];
        uint64_t view[K + R];
        ec_staged plan[K + R];
        static const isal_hip_encmask no_masks;
        ec_call q = {"stage_host", op, len, K, R, 1, g_tbls, sh, nsrc, sh + nsrc, nptr, view, 0, 0, 0, plan, NULL, &no_masks};
        unsigned long long first_bad, want_bad;
        gpu_res r;
        int i, b;

        for (i = 0; i < nptr; i++) {
                sh[i] = shard(len + GUARD);
                orig[i] = shard(len + GUARD);
                for (b = 0; b < len; b++)
                        sh[i][b] = (unsigned char) rnd(256);
                memset(sh[i] + len, 0xC3, GUARD);
        }
        if (op == OP_VERIFY) { /* stored rows = the parity, but for one byte of row 1 */
                (void) isal_cpu_run(OP_ENCODE, 0, len, K, R, 0, g_tbls, sh, K, sh + K);
                sh[K + 1][len - 3] ^= 0x40;
        }
        for (i = 0; i < nptr; i++)
                memcpy(orig[i], sh[i], (size_t) len + GUARD);
        /* the reference: the CPU route on copies of the same inputs */
        for (i = 0; i < nsrc; i++)
                src_ref[i] = orig[i];
        for (i = 0; i < R; i++) {
                want[i] = shard(len);
                memcpy(want[i], orig[nsrc + i], (size_t) len);
        }
        want_bad = isal_cpu_run(op, 0, len, K, R, 1, g_tbls, src_ref, nsrc, want);
        CHECK(want_bad == (op == OP_VERIFY ? planted : ~0ull));

        /* the call as run_ec describes it */
        for (i = 0; i < nptr; i++) {
                const int in_place = kase == ENC_STAGED ? 0 : kase == UPD ? i == 0 : i == 0 || i == nsrc;
                view[i] = in_place ? (uint64_t) (uintptr_t) sh[i] : 0;
                if (!in_place) {
                        plan[q.nstage].ptr = i;
                        plan[q.nstage].row = i < nsrc ? -1 : i - nsrc;
                        q.nstage_src += i < nsrc;
                        q.nstage++;
                }
        }
        q.nstage_in = op == OP_ENCODE ? q.nstage_src : q.nstage;
        q.tbl = isal_hip_ctx_tables(c, K, R, g_tbls, &q.em);
        CHECK(q.tbl);

        knob("ISAL_HIP_FAULT", site ? site : -1);
        knob("ISAL_HIP_FAULT_CHUNK", site ? chunk : -1);
        r = attempt(route, c, &q);
        first_bad = r.first_bad;
        if (site) {
                /* a site the route does not have, or a chunk it never reaches,
                 * leaves the run whole; the table says which */
                const int failed = r.err != hipSuccess;
                if (g_record) {
                        printf("        {%d, %d, %d, %d, %d, %lld, %lld, %d},\n", kase, route, site, chunk, failed,
                               r.done, failed ? r.chunk_end : 0, failed ? r.rows_out : 0);
                } else {
                        CHECK(g_next < sizeof(expect) / sizeof(expect[0]));
                        CHECK(expect[g_next].kase == kase && expect[g_next].route == route &&
                              expect[g_next].site == site && expect[g_next].chunk == chunk);
                        CHECK(expect[g_next].failed == failed && expect[g_next].done == r.done);
                        if (failed)
                                CHECK(r.what && *r.what && expect[g_next].chunk_end == r.chunk_end &&
                                      expect[g_next].rows_out == r.rows_out);
                        g_next++;
                }
        } else {
                CHECK(r.err == hipSuccess && r.done == len);
        }
        if (r.err != hipSuccess)
                CHECK(isal_hip_finish_on_cpu(c, &q, &r, &first_bad) == 0);

        CHECK(first_bad == want_bad);
        for (i = 0; i < nptr; i++) {
                if (i < nsrc || op == OP_VERIFY) /* only read */
                        CHECK(memcmp(sh[i], orig[i], (size_t) len) == 0);
                else
                        CHECK(memcmp(sh[i], want[i - nsrc], (size_t) len) == 0);
                CHECK(memcmp(sh[i] + len, orig[i] + len, GUARD) == 0);
                free(sh[i]);
                free(orig[i]);
        }
        for (i = 0; i < R; i++)
                free(want[i]);
}

static void *
driver(void *arg)
{
        hipError_t err = hipSuccess;
        const char *what = NULL;
        ctx_t *c = isal_hip_ctx_get(0, &err, &what);
        int kase, route, site, chunk, runs = 0;
        (void) arg;
        CHECK(c);
        for (kase = 0; kase < NCASES; kase++)
                for (route = 0; route < NROUTES; route++) {
                        if (route == PIPED && case_op[kase] == OP_VERIFY)
                                continue; /* run_ec never pipelines a verify */
                        one_run(c, kase, route, 0, 0);
                        runs++;
                        for (site = FAULT_ALLOC; site <= FAULT_SYNC; site++)
                                for (chunk = 0; chunk < 2; chunk++, runs++)
                                        one_run(c, kase, route, site, chunk);
                        if (!g_record)
                                printf("  %s, %s: whole and after every fault\n", case_name[kase], route_name[route]);
                }
        CHECK(g_record || g_next == sizeof(expect) / sizeof(expect[0]));
        printf("  %d runs: outputs as the CPU route, guards untouched, failures as recorded\n", runs);
        return NULL;
}

int
main(void)
{
        unsigned char a[(K + R) * K];
        pthread_t th;
        printf("stage_host: isal_hip_stage.c + isal_hip_ctx.c with stubbed HIP\n");
        gf_gen_rs_matrix(a, K + R, K);
        ec_init_tables(K, R, a + K * K, g_tbls);
        g_record = getenv("STAGE_HOST_RECORD") != NULL;
        setenv("ISAL_HIP_CHUNK_KB", "4", 1);
        setenv("ISAL_HIP_STAGE_MB", "1", 1);
        /* a thread of its own: when it ends, its context is freed (the key's
         * destructor) and the copy-out worker joined, under the sanitizers too */
        CHECK(pthread_create(&th, NULL, driver, NULL) == 0);
        CHECK(pthread_join(th, NULL) == 0);
        CHECK(g_allocs == 0);
        printf("stage_host: ok (%d stub launches)\n", g_plain_launches);
        return 0;
}
