/*
 * isal_hip_karg.c — kernel-argument calls of the drop-in shim
 * (isal_hip_launch_*_karg): one launch, no argument upload, for
 * device-resident, 16-byte aligned shards of a one-pass stripe that fits the
 * 2 KiB argument block — and their completion through a page-locked host
 * mailbox the calling thread spins on instead of the runtime's wake-up.
 */
#include <hip/hip_runtime_api.h>
#include <sched.h>
#include <stdint.h>
#include <string.h>
#include <time.h>

#include "isal_hip_shim.h"

int
isal_hip_karg_fits(const ec_call *q)
{
        int i;
        if (q->len < 16 || q->rows > EC_MAX_ROWS_PER_PASS || q->nptr > ISAL_HIP_KARG_PTRS ||
            isal_hip_tables_dwords(q->op == OP_UPDATE ? 1 : q->k, q->rows) > ISAL_HIP_KARG_TBL ||
            isal_hip_knob(ISAL_HIP_KNOB_KARG) == 0)
                return 0;
        for (i = 0; i < q->nptr; i++)
                if (q->view[i] & 15)
                        return 0;
        return 1;
}

/* The completion words of kernel-argument calls, allocated on a thread's
 * first such call: device {counters = 0 (isal_hip_kdone), verify result = ~0}, host mailbox
 * (page-locked, coherent: the kernel's system-scope stores land in it with no
 * cached copy in between). */
#define KDONE_CNT_BYTES ((size_t) ISAL_HIP_KDONE_WORDS * 4)
static hipError_t
ensure_done(ctx_t *c)
{
        static const unsigned long long res_init = ~0ull;
        hipError_t e;
        void *h = NULL;
        if (c->d_done)
                return hipSuccess;
        if ((e = hipMalloc(&c->d_done, KDONE_CNT_BYTES + 64)) != hipSuccess)
                return e;
        if ((e = hipMemset(c->d_done, 0, KDONE_CNT_BYTES)) != hipSuccess ||
            (e = hipMemcpy((char *) c->d_done + KDONE_CNT_BYTES, &res_init, 8, hipMemcpyHostToDevice)) !=
                    hipSuccess ||
            (e = hipHostMalloc(&h, 64, hipHostMallocCoherent)) != hipSuccess ||
            (e = hipHostGetDevicePointer(&c->h_mail_dev, h, 0)) != hipSuccess) {
                (void) hipFree(c->d_done);
                if (h)
                        (void) hipHostFree(h);
                c->d_done = NULL;
                return e;
        }
        memset(h, 0, 64);
        c->h_mail = (volatile unsigned long long *) h;
        return hipSuccess;
}

static double
now_s(void)
{
        struct timespec t;
        clock_gettime(CLOCK_MONOTONIC, &t);
        return (double) t.tv_sec + 1e-9 * (double) t.tv_nsec;
}

/* Wait for call `seq` of this thread: spin on the mailbox the kernel's last
 * workgroup writes (the runtime's completion signal and wake-up cost ~9 us
 * more). Bounded: after SPIN_S seconds without it the stream is
 * synchronised, so a kernel that faulted is reported through the runtime and
 * a slow one is simply waited for. The stream is still synchronised every
 * SYNC_EVERY calls (the kernels have long ended by then) so the runtime
 * retires its launch records. */
static unsigned long long g_slow_waits;

unsigned long long
isal_hip_slow_waits(void)
{
        return __atomic_load_n(&g_slow_waits, __ATOMIC_RELAXED);
}

#define DONE_SPIN_S 0.02
#define DONE_YIELD_S 50e-6 /* then yield the CPU between polls: callers may outnumber cores */
#define DONE_SYNC_EVERY 64
static hipError_t
wait_done(ctx_t *c, unsigned long long seq)
{
        hipError_t e;
        unsigned spins = 0;
        int yield = 0;
        double t0 = 0;
        while (c->h_mail[0] != seq) {
                if (yield)
                        sched_yield();
                else
                        __builtin_ia32_pause();
                if ((++spins & 63) == 0) {
                        const double t = now_s();
                        if (t0 == 0)
                                t0 = t;
                        else if (t - t0 > DONE_SPIN_S)
                                break;
                        else
                                yield = t - t0 > DONE_YIELD_S;
                }
        }
        if (c->h_mail[0] != seq) {
                __atomic_add_fetch(&g_slow_waits, 1ull, __ATOMIC_RELAXED);
                if ((e = hipStreamSynchronize(c->stream)) != hipSuccess)
                        return e;
                c->unsynced = 0;
                if (c->h_mail[0] != seq)
                        return hipErrorUnknown; /* the kernel ended without writing its completion word */
                return hipSuccess;
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE); /* the result word was written before seq */
        if (++c->unsynced >= DONE_SYNC_EVERY) {
                c->unsynced = 0;
                return hipStreamSynchronize(c->stream);
        }
        return hipSuccess;
}

/* A kernel-argument call's arguments, in the 2 KiB block the kernels read
 * from their kernarg segment. mail: the completion mailbox is used (every
 * shard is hipMalloc memory: managed memory the host may read directly is
 * left to hipStreamSynchronize, which also makes the host's view coherent;
 * ISAL_HIP_KARG_DONE=0 turns the mailbox off). A verify needs the mailbox. */
gpu_res
isal_hip_gpu_karg(ctx_t *c, const ec_call *q, int mail)
{
        static int inflight; /* kernel-argument calls of the process in flight (lane width) */
        static const char *const launch_what[] = {"encode launch (kernel arguments)",
                                                  "update launch (kernel arguments)",
                                                  "verify launch (kernel arguments)"};
        static const char *const wait_what[] = {"encode completion (kernel arguments)",
                                                "update completion (kernel arguments)",
                                                "verify completion (kernel arguments)"};
        gpu_res r = GPU_RES_INIT;
        const int op = q->op, len = q->len, k = q->k, rows = q->rows;
        isal_hip_kdone d = {NULL, NULL, NULL, 0ull};
        isal_hip_karg a;
        hipError_t e;
        int busy;
        memset(&a, 0, sizeof(a));
        memcpy(a.ptrs, q->view, sizeof(uint64_t) * (size_t) ((op == OP_UPDATE ? 1 : k) + rows));
        if (mail) {
                GPU_TRY_AT(r, FAULT_ALLOC, ensure_done(c));
                d.cnt = (unsigned *) c->d_done;
                d.res = op == OP_VERIFY ? (unsigned long long *) ((char *) c->d_done + KDONE_CNT_BYTES) : NULL;
                d.mail = (unsigned long long *) c->h_mail_dev;
        }
        /* an injected launch failure (tests) launches nothing, as a failed launch */
        if (isal_hip_fault_at(FAULT_LAUNCH, 0)) {
                r.err = hipErrorOutOfMemory;
                r.what = launch_what[op];
                return r;
        }
        if (mail)
                d.seq = ++c->seq;
        if (op == OP_UPDATE) {
                /* one pass: source vec_i's tables for every row are contiguous */
                memcpy(a.tbl, q->tbl + isal_hip_tables_dwords(q->vec_i, rows), isal_hip_tables_dwords(1, rows) * 4);
                e = (hipError_t) isal_hip_launch_update_karg(&a, &d, len, rows, c->stream);
        } else {
                memcpy(a.tbl, q->tbl, isal_hip_tables_dwords(k, rows) * 4);
                busy = __atomic_add_fetch(&inflight, 1, __ATOMIC_RELAXED);
                e = (hipError_t) (op == OP_VERIFY
                                          ? isal_hip_launch_verify_karg(&a, &d, len, k, rows, q->em, c->stream)
                                          : isal_hip_launch_encode_karg(
                                                    &a, &d, len, k, rows, q->em, busy,
                                                    isal_hip_karg_ldsx(k, rows) ? isal_hip_ctx_ldsx(c, k, rows) : NULL,
                                                    c->stream));
        }
        if (e == hipSuccess) {
                r.what = wait_what[op];
                e = isal_hip_fault_at(FAULT_SYNC, 0) ? hipErrorOutOfMemory
                    : mail                           ? wait_done(c, d.seq)
                                                     : hipStreamSynchronize(c->stream);
        } else {
                r.what = launch_what[op];
        }
        if (op != OP_UPDATE) /* this call is no longer in flight, whatever failed */
                __atomic_sub_fetch(&inflight, 1, __ATOMIC_RELAXED);
        if ((r.err = e) != hipSuccess)
                return r;
        r.what = NULL;
        if (op == OP_VERIFY)
                r.first_bad = c->h_mail[1];
        r.done = len;
        return r;
}
