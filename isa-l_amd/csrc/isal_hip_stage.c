/*
 * isal_hip_stage.c — the drop-in shim's routes for calls with host-resident
 * shards that no kernel reaches in place: the shards are staged through a
 * per-thread pinned or HBM buffer.
 *
 *   small      zero-copy / packed: whole shards in the argument buffer
 *   chunked    column chunks, one at a time (also: nothing staged, one launch)
 *   pipelined  column chunks through PIPE_NBUF staging sets; a worker thread
 *              of the calling thread copies the outputs back
 *
 * Which shards are staged, and through which slot, is decided once per call
 * (ec_call.plan, filled by run_ec). Three helpers read it, and they are the
 * only code that does: fill_ptrs (a chunk's pointer table), stage_in (its
 * staged inputs) and stage_out (its staged outputs; the accounting of
 * rows_out, which decides what the CPU completion below may overwrite).
 */
#include <hip/hip_runtime_api.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "isal_hip_shim.h"

/* Host-resident shards are staged through HBM in chunks of at most this many
 * bytes in total (override: ISAL_HIP_STAGE_MB). */
#define DEFAULT_STAGE_BYTES (256u << 20)
/* Large host calls are cut into column chunks of this many bytes per shard
 * (override: ISAL_HIP_CHUNK_KB). */
#define DEFAULT_CHUNK_BYTES ((size_t) 4 << 20)

size_t
isal_hip_stage_limit(void)
{
        const long long v = isal_hip_knob(ISAL_HIP_KNOB_STAGE_MB);
        return v > 0 ? (size_t) v << 20 : DEFAULT_STAGE_BYTES;
}

int
isal_hip_fault_at(int site, long long chunk)
{
        const long long fc = isal_hip_knob(ISAL_HIP_KNOB_FAULT_CHUNK);
        return site != FAULT_NONE && isal_hip_knob(ISAL_HIP_KNOB_FAULT) == site &&
               (fc < 0 || fc == chunk);
}

/* Copy-out worker of a calling thread. The runtime serves a copy from or to
 * pageable memory synchronously on the thread that issues it (tools/
 * stage_probe.c: hipMemcpyAsync returns when the copy is done), so copies in
 * and out overlap only when two host threads issue them: the calling thread
 * stages chunks in and launches, this worker copies chunks out in order. */
typedef struct outq {
        pthread_t th;
        pthread_mutex_t mu;
        pthread_cond_t cv;
        int quit, active;
        long long posted, handled; /* chunks launched / whose output copies are enqueued */
        /* the call being served and its chunk geometry */
        const ec_call *call;
        size_t chunk, slot, set_bytes;
        /* the worker's first failure */
        hipError_t err;
        const char *what;
        long long fail_chunk;
        int rows_out;
        /* a one-off batch of copies (isal_hip_gpu_chunked's second issuing thread) */
        struct copyjob *job;
        int job_state; /* 0 none, 1 posted, 2 finished */
} outq_t;

/* Copies the worker issues on s_out for isal_hip_gpu_chunked: after `after`
 * (if set, a GPU-side wait), then `record` is recorded. */
#define COPYJOB_MAX 512
typedef struct copyjob {
        int n;
        struct {
                void *dst;
                const void *src;
                size_t bytes;
                hipMemcpyKind kind;
        } cp[COPYJOB_MAX];
        hipEvent_t after, record;
        hipError_t err;
        const char *what;
} copyjob_t;

static void
job_add(copyjob_t *j, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
        j->cp[j->n].dst = dst;
        j->cp[j->n].src = src;
        j->cp[j->n].bytes = bytes;
        j->cp[j->n].kind = kind;
        j->n++;
}

/* ---- the argument block and the launch ------------------------------------ */

/* Byte layout of the argument buffer of one call. */
typedef struct {
        size_t ptr_bytes, args_bytes, slots_off, slots_bytes, stage_off, slot, total;
} layout_t;

static layout_t
call_layout(const ec_call *q, int nstage)
{
        layout_t L;
        L.ptr_bytes = ((size_t) q->nptr * 8 + 15) & ~(size_t) 15;
        L.args_bytes = L.ptr_bytes + ((isal_hip_tables_dwords(q->k, q->rows) * 4 + 15) & ~(size_t) 15);
        L.slots_off = L.args_bytes;
        L.slots_bytes = q->op == OP_VERIFY ? (size_t) EC_VERIFY_SLOTS(q->rows) * 8 : 0;
        L.stage_off = (L.slots_off + L.slots_bytes + 255) & ~(size_t) 255;
        L.slot = ((size_t) q->len + 255) & ~(size_t) 255;
        L.total = L.stage_off + L.slot * (size_t) nstage;
        return L;
}

static unsigned long long
min_slot(const unsigned long long *slots, int n)
{
        unsigned long long m = ~0ull;
        int i;
        for (i = 0; i < n; i++)
                if (slots[i] < m)
                        m = slots[i];
        return m;
}

/* Enqueue the kernel(s) of the clen columns from c0 with the argument block
 * at `args` (device or zero-copy view). For OP_VERIFY *nslots receives the
 * number of slots written at args + L->slots_off. */
static hipError_t
launch_op(ctx_t *c, const ec_call *q, char *args, const layout_t *L, int clen, long long c0, int vec16,
          int *nslots)
{
        const uint64_t *ptrs = (const uint64_t *) args;
        const uint32_t *tbl = (const uint32_t *) (args + L->ptr_bytes);
        *nslots = 0;
        if (q->op == OP_VERIFY)
                return (hipError_t) isal_hip_launch_verify(
                        ptrs, q->nptr, 0, q->nsrc, tbl, clen, q->k, q->rows, c0,
                        (unsigned long long *) (args + L->slots_off), nslots, vec16, q->em, c->stream);
        if (q->op == OP_ENCODE)
                return (hipError_t) isal_hip_launch_encode(ptrs, q->nptr, 0, q->nsrc, tbl, clen, q->k, q->rows,
                                                           1, vec16, q->em, c->stream);
        return (hipError_t) isal_hip_launch_update(ptrs, q->nptr, 0, q->nsrc, tbl, clen, q->k, q->rows,
                                                   q->vec_i, 1, vec16, c->stream);
}

/* ---- the three readers of the call's staged-shard plan -------------------- */

/* The pointer table of the columns from c0: a shard used in place at its view
 * plus c0, staged shard s at stage + s * slot (the address the kernels use
 * for the staging buffer). Returns vec16: every address is 16-byte aligned. */
static int
fill_ptrs(const ec_call *q, uint64_t *ptrs, long long c0, const void *stage, size_t slot)
{
        int i, s, vec16 = 1;
        for (i = 0; i < q->nptr; i++)
                ptrs[i] = q->view[i] + (uint64_t) c0;
        for (s = 0; s < q->nstage; s++)
                ptrs[q->plan[s].ptr] = (uint64_t) (uintptr_t) stage + (uint64_t) s * slot;
        for (i = 0; i < q->nptr; i++)
                if (ptrs[i] & 15)
                        vec16 = 0;
        return vec16;
}

/* How a route moves staged shards between the caller's memory and a staging
 * buffer: */
typedef struct {
        enum {
                MOVE_PLAIN, /* memcpy: the buffer is the pinned argument block */
                MOVE_ASYNC, /* hipMemcpyAsync on `stream` */
                MOVE_LISTS, /* entries of two copy lists, taken in turn, issued later */
        } how;
        hipStream_t stream;
        copyjob_t *list[2];
} mover_t;

/* The staged inputs of chunk ci — n columns from c0 — into their slots of
 * `stage`, in slot order. Every asynchronous copy is a FAULT_H2D site. */
static hipError_t
stage_in(const ec_call *q, long long ci, long long c0, size_t n, unsigned char *stage, size_t slot,
         const mover_t *m)
{
        int s;
        for (s = 0; s < q->nstage_in; s++) {
                const int i = q->plan[s].ptr;
                unsigned char *host = (i < q->nsrc ? q->src[i] : q->dst[i - q->nsrc]) + c0;
                unsigned char *st = stage + (size_t) s * slot;
                hipError_t e = hipSuccess;
                if (m->how == MOVE_LISTS)
                        job_add(m->list[s & 1], st, host, n, hipMemcpyHostToDevice);
                else if (m->how == MOVE_PLAIN)
                        memcpy(st, host, n);
                else
                        e = isal_hip_fault_at(FAULT_H2D, ci)
                                    ? hipErrorOutOfMemory
                                    : hipMemcpyAsync(st, host, n, hipMemcpyHostToDevice, m->stream);
                if (e != hipSuccess)
                        return e;
        }
        return hipSuccess;
}

/* The staged outputs of chunk ci out of their slots of `stage`, in row order.
 * Of the asynchronous copies, output row 1's is the FAULT_D2H site, and
 * *rows_out counts the output rows up to the last one whose copy was
 * enqueued: after a failure, rows [0, *rows_out) of the chunk may reach the
 * caller's memory and the rows from *rows_out on will not. (Copy lists are
 * issued by issue_copies and the worker, which do their own accounting.) */
static hipError_t
stage_out(const ec_call *q, long long ci, long long c0, size_t n, const unsigned char *stage, size_t slot,
          const mover_t *m, int *rows_out)
{
        int s;
        *rows_out = 0;
        for (s = q->nstage_src; s < q->nstage; s++) {
                const int row = q->plan[s].row;
                unsigned char *host = q->dst[row] + c0;
                const unsigned char *st = stage + (size_t) s * slot;
                hipError_t e = hipSuccess;
                if (m->how == MOVE_LISTS) {
                        job_add(m->list[(s - q->nstage_src) & 1], host, st, n, hipMemcpyDeviceToHost);
                        continue;
                }
                if (m->how == MOVE_PLAIN)
                        memcpy(host, st, n);
                else
                        e = isal_hip_fault_at(row == 1 ? FAULT_D2H : FAULT_NONE, ci)
                                    ? hipErrorOutOfMemory
                                    : hipMemcpyAsync(host, st, n, hipMemcpyDeviceToHost, m->stream);
                if (e != hipSuccess)
                        return e;
                *rows_out = row + 1;
        }
        return hipSuccess;
}

/* ---- small: zero-copy and packed ------------------------------------------ */

/* Whole shards, one chunk: pointer table, coefficient tables, verify slots and
 * the staged shards all live in the pinned argument buffer, which the kernel
 * reads and writes over PCIe (zero_copy) or which moves with one H2D and one
 * D2H DMA into / out of HBM (packed). Host outputs are written only after the
 * stream completed, so a failure leaves them untouched. */
gpu_res
isal_hip_gpu_small(ctx_t *c, const ec_call *q, int zero_copy)
{
        static const mover_t plain = {MOVE_PLAIN, NULL, {NULL, NULL}};
        gpu_res r = GPU_RES_INIT;
        const int first_out = q->nstage_src < q->nstage ? q->nstage_src : -1;
        const layout_t L = call_layout(q, q->nstage);
        int vec16, nslots, unused;
        char *h, *dv;
        size_t upload;

        GPU_TRY_AT(r, FAULT_ALLOC, isal_hip_ctx_args(c, L.total));
        h = (char *) c->h_args;
        dv = zero_copy ? (char *) c->h_args_dev : (char *) c->d_args; /* what kernels see */
        memcpy(h + L.ptr_bytes, q->tbl, isal_hip_tables_dwords(q->k, q->rows) * 4);
        vec16 = fill_ptrs(q, (uint64_t *) h, 0, dv + L.stage_off, L.slot);
        (void) stage_in(q, 0, 0, (size_t) q->len, (unsigned char *) h + L.stage_off, L.slot, &plain);
        upload = q->nstage_in ? L.stage_off + (size_t) q->nstage_in * L.slot : L.args_bytes;
        if (!zero_copy)
                GPU_TRY_AT(r, FAULT_H2D, hipMemcpyAsync(c->d_args, h, upload, hipMemcpyHostToDevice, c->stream));
        GPU_TRY_AT(r, FAULT_LAUNCH, launch_op(c, q, dv, &L, q->len, 0, vec16, &nslots));
        if (!zero_copy) {
                if (q->op == OP_VERIFY)
                        GPU_TRY(r, hipMemcpyAsync(h + L.slots_off, (char *) c->d_args + L.slots_off,
                                                  (size_t) nslots * 8, hipMemcpyDeviceToHost,
                                                  c->stream));
                else if (first_out >= 0)
                        GPU_TRY_AT(r, FAULT_D2H, hipMemcpyAsync(h + L.stage_off + (size_t) first_out * L.slot,
                                                  (char *) c->d_args + L.stage_off +
                                                          (size_t) first_out * L.slot,
                                                  (size_t) (q->nstage - first_out) * L.slot,
                                                  hipMemcpyDeviceToHost, c->stream));
        }
        GPU_TRY_AT(r, FAULT_SYNC, hipStreamSynchronize(c->stream));
        if (q->op == OP_VERIFY)
                r.first_bad = min_slot((const unsigned long long *) (h + L.slots_off), nslots);
        else
                (void) stage_out(q, 0, 0, (size_t) q->len, (unsigned char *) h + L.stage_off, L.slot, &plain,
                                 &unused);
        r.done = q->len;
        return r;
}

/* ---- chunked --------------------------------------------------------------- */

static hipError_t outq_start(ctx_t *c);
static void copyjob_post(outq_t *q, copyjob_t *j);
static hipError_t copyjob_wait(outq_t *q, copyjob_t *j);

/* Issue this thread's share of a chunk's copies on the call's stream (the
 * fault sites of the tests apply to them: an H2D list fails at its first
 * copy, a D2H list at its second). *enq: copies enqueued. */
static hipError_t
issue_copies(ctx_t *c, const copyjob_t *j, int fault_site, long long ci, const char **what, int *enq)
{
        int i;
        hipError_t e;
        *enq = 0;
        for (i = 0; i < j->n; i++) {
                e = isal_hip_fault_at(i == 1 || fault_site == FAULT_H2D ? fault_site : FAULT_NONE, ci)
                            ? hipErrorOutOfMemory
                            : hipMemcpyAsync(j->cp[i].dst, j->cp[i].src, j->cp[i].bytes, j->cp[i].kind,
                                             c->stream);
                if (e != hipSuccess) {
                        *what = j->cp[i].kind == hipMemcpyHostToDevice ? "hipMemcpyAsync(H2D chunk)"
                                                                        : "hipMemcpyAsync(D2H chunk)";
                        return e;
                }
                *enq = i + 1;
        }
        return hipSuccess;
}

/* Column-chunked mode: whole shards when nothing is staged, else chunks of at
 * most isal_hip_stage_limit() bytes over all staged shards. r.done advances
 * past every chunk whose outputs are final.
 * With two or more staged shards the chunk's copies are shared with the
 * calling thread's worker (ISAL_HIP_PAR_COPY=0: not): a pageable copy runs
 * synchronously on the thread that issues it with a fixed cost of ~14 us,
 * and a second issuing thread hides part of it (H2D of 2 MiB shards:
 * 36 -> 41 GB/s, profiles/r03/r03_stage_probe_b.jsonl). The worker copies in on
 * s_out (the kernel waits for its event); for an encode it also copies half
 * the parity out after the kernel. An update's parity comes back from this
 * thread alone, in row order, so a failure leaves a known prefix of rows
 * updated (rows_out). */
gpu_res
isal_hip_gpu_chunked(ctx_t *c, const ec_call *q)
{
        gpu_res r = GPU_RES_INIT;
        const int op = q->op, len = q->len, nstage = q->nstage;
        const mover_t serial = {MOVE_ASYNC, c->stream, {NULL, NULL}};
        int nslots, par = 0;
        size_t chunk, slot;
        layout_t L;
        long long c0;
        copyjob_t *win = NULL, *wout = NULL, *mine = NULL;

        if (nstage) {
                size_t per = isal_hip_stage_limit() / (size_t) nstage;
                per &= ~(size_t) 4095;
                if (per < 4096)
                        per = 4096;
                chunk = (size_t) len < per ? (size_t) len : per;
                slot = (chunk + 255) & ~(size_t) 255; /* keep every slot 256-B aligned */
                GPU_TRY_AT(r, FAULT_ALLOC, isal_hip_ctx_stage(c, slot * (size_t) nstage));
        } else {
                chunk = (size_t) len;
                slot = 0;
        }
        if (nstage >= 2 && q->nptr <= COPYJOB_MAX && isal_hip_knob(ISAL_HIP_KNOB_PAR_COPY) != 0) {
                if (!c->jobs)
                        c->jobs = (copyjob_t *) malloc(3 * sizeof(copyjob_t));
                /* no helper (no memory, no thread): one issuing thread, as before */
                par = c->jobs && isal_hip_ctx_pipe(c) == hipSuccess && outq_start(c) == hipSuccess;
                (void) hipGetLastError();
                if (par) {
                        win = &c->jobs[0];
                        wout = &c->jobs[1];
                        mine = &c->jobs[2];
                }
        }

        L = call_layout(q, 0);
        GPU_TRY(r, isal_hip_ctx_args(c, L.stage_off));
        memcpy((char *) c->h_args + L.ptr_bytes, q->tbl, isal_hip_tables_dwords(q->k, q->rows) * 4);

        for (c0 = 0; c0 < len; c0 += (long long) chunk) {
                const int clen = (int) ((long long) len - c0 < (long long) chunk ? len - c0 : (long long) chunk);
                const long long ci = c0 / (long long) chunk;
                const int vec16 = fill_ptrs(q, (uint64_t *) c->h_args, c0, c->d_stage, slot);
                int enq = 0;
                if (par) {
                        const mover_t in = {MOVE_LISTS, NULL, {mine, win}};
                        hipError_t e, ew;
                        const char *what = NULL;
                        win->n = mine->n = 0;
                        win->after = NULL;
                        win->record = c->ev_in[0];
                        (void) stage_in(q, ci, c0, (size_t) clen, c->d_stage, slot, &in);
                        if (win->n)
                                copyjob_post(c->oq, win);
                        e = issue_copies(c, mine, FAULT_H2D, ci, &what, &enq);
                        ew = win->n ? copyjob_wait(c->oq, win) : hipSuccess;
                        if (e == hipSuccess && ew != hipSuccess) {
                                e = ew;
                                what = win->what;
                        }
                        if (e == hipSuccess && win->n)
                                e = hipStreamWaitEvent(c->stream, c->ev_in[0], 0);
                        if (e != hipSuccess) {
                                r.err = e;
                                r.what = what ? what : "hipStreamWaitEvent(helper copies in)";
                                return r;
                        }
                } else if ((r.err = stage_in(q, ci, c0, (size_t) clen, c->d_stage, slot, &serial)) != hipSuccess) {
                        r.what = "hipMemcpyAsync(H2D chunk)";
                        return r;
                }
                GPU_TRY(r, hipMemcpyAsync(c->d_args, c->h_args, L.args_bytes,
                                          hipMemcpyHostToDevice, c->stream));
                GPU_TRY_ATC(r, FAULT_LAUNCH, ci, launch_op(c, q, (char *) c->d_args, &L, clen, c0, vec16, &nslots));
                if (op == OP_VERIFY) {
                        GPU_TRY(r, hipMemcpyAsync((char *) c->h_args + L.slots_off,
                                                  (char *) c->d_args + L.slots_off,
                                                  (size_t) nslots * 8, hipMemcpyDeviceToHost,
                                                  c->stream));
                        GPU_TRY(r, hipStreamSynchronize(c->stream));
                        r.first_bad = min_slot(
                                (const unsigned long long *) ((char *) c->h_args + L.slots_off),
                                nslots);
                        r.done = c0 + clen;
                        if (r.first_bad != ~0ull)
                                break;
                        continue;
                }
                r.chunk_end = c0 + clen;
                if (par && op == OP_ENCODE) {
                        /* encode: half the parity rows leave through the worker */
                        const mover_t out = {MOVE_LISTS, NULL, {mine, wout}};
                        hipError_t e, ew;
                        const char *what = NULL;
                        wout->n = mine->n = 0;
                        wout->after = c->ev_k[0];
                        wout->record = c->ev_out[0];
                        r.rows_out = 0;
                        GPU_TRY(r, hipEventRecord(c->ev_k[0], c->stream));
                        (void) stage_out(q, ci, c0, (size_t) clen, c->d_stage, slot, &out, &r.rows_out);
                        if (wout->n)
                                copyjob_post(c->oq, wout);
                        e = issue_copies(c, mine, FAULT_D2H, ci, &what, &enq);
                        ew = wout->n ? copyjob_wait(c->oq, wout) : hipSuccess;
                        /* some parity copies may be under way: a failed drain must abort */
                        r.rows_out = enq || wout->n ? 1 : 0;
                        if (e == hipSuccess && ew != hipSuccess) {
                                e = ew;
                                what = wout->what;
                        }
                        if (e == hipSuccess && wout->n)
                                e = isal_hip_fault_at(FAULT_SYNC, ci) ? hipErrorOutOfMemory
                                                                      : hipStreamSynchronize(c->s_out);
                        if (e != hipSuccess) {
                                r.err = e;
                                r.what = what ? what : "hipStreamSynchronize(helper copies out)";
                                return r;
                        }
                } else if ((r.err = stage_out(q, ci, c0, (size_t) clen, c->d_stage, slot, &serial, &r.rows_out)) !=
                           hipSuccess) {
                        r.what = "hipMemcpyAsync(D2H chunk)";
                        return r;
                }
                GPU_TRY_ATC(r, FAULT_SYNC, ci, hipStreamSynchronize(c->stream));
                r.done = c0 + clen;
                r.rows_out = 0;
        }
        r.done = len;
        return r;
}

/* ---- the worker ------------------------------------------------------------ */

/* Output copies of chunk ci (staging set ci % PIPE_NBUF) on s_out, after its
 * kernel. *rows_out: as stage_out leaves it. */
static hipError_t
copy_out_chunk(ctx_t *c, const outq_t *q, long long ci, const char **what, int *rows_out)
{
        const mover_t out = {MOVE_ASYNC, c->s_out, {NULL, NULL}};
        const long long p0 = ci * (long long) q->chunk, left = (long long) q->call->len - p0;
        const size_t plen = (size_t) (left < (long long) q->chunk ? left : (long long) q->chunk);
        const int b = (int) (ci % PIPE_NBUF);
        hipError_t e;
        *rows_out = 0;
        if ((e = hipStreamWaitEvent(c->s_out, c->ev_k[b], 0)) != hipSuccess) {
                *what = "hipStreamWaitEvent(copy-out)";
                return e;
        }
        if ((e = stage_out(q->call, ci, p0, plen, c->d_stage + (size_t) b * q->set_bytes, q->slot, &out,
                           rows_out)) != hipSuccess) {
                *what = "hipMemcpyAsync(D2H chunk)";
                return e;
        }
        if ((e = hipEventRecord(c->ev_out[b], c->s_out)) != hipSuccess)
                *what = "hipEventRecord(copy-out)";
        return e;
}

static void
run_copyjob(ctx_t *c, copyjob_t *j)
{
        int i;
        j->err = hipSuccess;
        j->what = NULL;
        if (j->after && (j->err = hipStreamWaitEvent(c->s_out, j->after, 0)) != hipSuccess) {
                j->what = "hipStreamWaitEvent(helper copies)";
                return;
        }
        for (i = 0; i < j->n; i++)
                if ((j->err = hipMemcpyAsync(j->cp[i].dst, j->cp[i].src, j->cp[i].bytes, j->cp[i].kind,
                                             c->s_out)) != hipSuccess) {
                        j->what = "hipMemcpyAsync(helper copies)";
                        return;
                }
        if (j->record && (j->err = hipEventRecord(j->record, c->s_out)) != hipSuccess)
                j->what = "hipEventRecord(helper copies)";
}

static void
copyjob_post(outq_t *q, copyjob_t *j)
{
        pthread_mutex_lock(&q->mu);
        q->job = j;
        q->job_state = 1;
        pthread_cond_broadcast(&q->cv);
        pthread_mutex_unlock(&q->mu);
}

/* Wait until the worker has issued the posted job's copies (pageable ones
 * are complete by then); its error. */
static hipError_t
copyjob_wait(outq_t *q, copyjob_t *j)
{
        pthread_mutex_lock(&q->mu);
        while (q->job_state == 1)
                pthread_cond_wait(&q->cv, &q->mu);
        q->job_state = 0;
        q->job = NULL;
        pthread_mutex_unlock(&q->mu);
        return j->err;
}

static void *
outq_main(void *arg)
{
        ctx_t *c = (ctx_t *) arg;
        outq_t *q = c->oq;
        (void) hipSetDevice(c->device);
        pthread_mutex_lock(&q->mu);
        for (;;) {
                long long ci;
                const char *what = NULL;
                int rows_out;
                hipError_t e;
                while (!q->quit && q->job_state != 1 &&
                       !(q->active && q->err == hipSuccess && q->handled < q->posted))
                        pthread_cond_wait(&q->cv, &q->mu);
                if (q->quit)
                        break;
                if (q->job_state == 1) {
                        copyjob_t *j = q->job;
                        pthread_mutex_unlock(&q->mu);
                        run_copyjob(c, j);
                        pthread_mutex_lock(&q->mu);
                        q->job_state = 2;
                        pthread_cond_broadcast(&q->cv);
                        continue;
                }
                ci = q->handled;
                pthread_mutex_unlock(&q->mu);
                e = copy_out_chunk(c, q, ci, &what, &rows_out);
                pthread_mutex_lock(&q->mu);
                if (e != hipSuccess) {
                        q->err = e;
                        q->what = what;
                        q->fail_chunk = ci;
                        q->rows_out = rows_out;
                } else {
                        q->handled = ci + 1;
                }
                pthread_cond_broadcast(&q->cv);
        }
        pthread_mutex_unlock(&q->mu);
        return NULL;
}

/* Copy-out helpers alive in the process, at most max_helpers(): each is a
 * thread with two streams of its own, and they all share the process's few
 * hardware queues (isal_hip.h, "routing"). */
static int g_helpers;
#define DEFAULT_MAX_HELPERS 8

static int
max_helpers(void)
{
        const long long v = isal_hip_knob(ISAL_HIP_KNOB_MAX_HELPERS);
        return v >= 0 ? (int) v : DEFAULT_MAX_HELPERS;
}

static hipError_t
outq_start(ctx_t *c)
{
        outq_t *q;
        if (c->oq)
                return hipSuccess;
        if (__atomic_add_fetch(&g_helpers, 1, __ATOMIC_ACQ_REL) > max_helpers()) {
                __atomic_sub_fetch(&g_helpers, 1, __ATOMIC_ACQ_REL);
                return hipErrorNotSupported; /* over the cap: issue copies alone */
        }
        q = (outq_t *) calloc(1, sizeof(*q));
        if (!q) {
                __atomic_sub_fetch(&g_helpers, 1, __ATOMIC_ACQ_REL);
                return hipErrorOutOfMemory;
        }
        pthread_mutex_init(&q->mu, NULL);
        pthread_cond_init(&q->cv, NULL);
        c->oq = q;
        if (pthread_create(&q->th, NULL, outq_main, c) != 0) {
                pthread_mutex_destroy(&q->mu);
                pthread_cond_destroy(&q->cv);
                free(q);
                c->oq = NULL;
                __atomic_sub_fetch(&g_helpers, 1, __ATOMIC_ACQ_REL);
                return hipErrorOutOfMemory;
        }
        return hipSuccess;
}

void
isal_hip_outq_stop(ctx_t *c)
{
        outq_t *q = c->oq;
        pthread_mutex_lock(&q->mu);
        q->quit = 1;
        pthread_cond_broadcast(&q->cv);
        pthread_mutex_unlock(&q->mu);
        pthread_join(q->th, NULL);
        pthread_mutex_destroy(&q->mu);
        pthread_cond_destroy(&q->cv);
        free(q);
        c->oq = NULL;
        __atomic_sub_fetch(&g_helpers, 1, __ATOMIC_ACQ_REL);
}

/* Wait until the worker has enqueued the copies of chunks [0, n) or failed;
 * returns its error. */
static hipError_t
outq_wait(outq_t *q, long long n)
{
        hipError_t e;
        pthread_mutex_lock(&q->mu);
        while (q->err == hipSuccess && q->handled < n)
                pthread_cond_wait(&q->cv, &q->mu);
        e = q->err;
        pthread_mutex_unlock(&q->mu);
        return e;
}

/* ---- pipelined -------------------------------------------------------------- */

/* Column-chunk bytes per shard of a pipelined call: ISAL_HIP_CHUNK_KB, else
 * DEFAULT_CHUNK_BYTES. Every chunk costs one copy per staged shard each way,
 * and a copy from or to pageable memory has a fixed cost of ~14 us beside its
 * bytes (profiles/r03/r03_calltrace.txt), so chunks must be large: at 16 MiB
 * shards 4 MiB chunks beat one chunk by 4-9 %, 1 MiB chunks lose 50 %
 * (profiles/r03/r03_chunk_sweep*.jsonl). */
static size_t
chunk_bytes(void)
{
        const long long kb = isal_hip_knob(ISAL_HIP_KNOB_CHUNK_KB);
        return kb > 0 ? (size_t) kb << 10 : DEFAULT_CHUNK_BYTES;
}

/*
 * Pipelined column chunks: large host-resident encode / update calls. Chunk i
 * flows through staging set i % PIPE_NBUF in HBM: H2D of its sources (and of
 * its parity, for an update) on s_in, argument upload + kernel on the call's
 * stream, D2H of its outputs on s_out, chained by events. The calling thread
 * stages in and launches; the copy-out worker (outq) issues the D2H copies,
 * so that the H2D of chunk i + 1, the kernel of chunk i and the D2H of chunk
 * i - 1 run at once even for pageable host buffers. Host memory is written
 * only by the D2H copies, in chunk order: r.done is the end of the last chunk
 * whose output copies were all enqueued, rows_out counts the rows of the next
 * chunk whose copy was enqueued when an enqueue failed (as
 * isal_hip_gpu_chunked). The caller quiesces every stream before it trusts
 * either.
 */
gpu_res
isal_hip_gpu_pipelined(ctx_t *c, const ec_call *q)
{
        gpu_res r = GPU_RES_INIT;
        const int len = q->len;
        size_t chunk = chunk_bytes(), per, slot, set_bytes, astride;
        long long nchunks, ci, launched = 0;
        layout_t L;
        outq_t *oq;
        int b;

        per = isal_hip_stage_limit() / ((size_t) q->nstage * PIPE_NBUF) & ~(size_t) 4095;
        if (chunk > per)
                chunk = per < 4096 ? 4096 : per;
        if (chunk >= (size_t) len) /* one chunk: nothing to overlap */
                return isal_hip_gpu_chunked(c, q);
        if (!c->oq && outq_start(c) != hipSuccess) {
                /* no helper for this thread (the process cap, or no thread):
                 * one chunk at a time, copies issued by this thread alone */
                (void) hipGetLastError();
                return isal_hip_gpu_chunked(c, q);
        }
        slot = (chunk + 255) & ~(size_t) 255;
        set_bytes = slot * (size_t) q->nstage;
        GPU_TRY_AT(r, FAULT_ALLOC, isal_hip_ctx_stage(c, set_bytes * PIPE_NBUF));
        GPU_TRY_AT(r, FAULT_ALLOC, isal_hip_ctx_pipe(c));
        GPU_TRY_AT(r, FAULT_ALLOC, outq_start(c));
        L = call_layout(q, 0);
        astride = (L.args_bytes + 255) & ~(size_t) 255;
        GPU_TRY_AT(r, FAULT_ALLOC, isal_hip_ctx_args(c, astride * PIPE_NBUF));
        /* one argument region per staging set: pointer table + coefficient tables */
        memcpy((char *) c->h_args + L.ptr_bytes, q->tbl, isal_hip_tables_dwords(q->k, q->rows) * 4);
        for (b = 1; b < PIPE_NBUF; b++)
                memcpy((char *) c->h_args + b * astride + L.ptr_bytes, (char *) c->h_args + L.ptr_bytes,
                       L.args_bytes - L.ptr_bytes);
        nchunks = ((long long) len + (long long) chunk - 1) / (long long) chunk;

        oq = c->oq;
        pthread_mutex_lock(&oq->mu);
        oq->call = q;
        oq->chunk = chunk;
        oq->slot = slot;
        oq->set_bytes = set_bytes;
        oq->posted = oq->handled = 0;
        oq->err = hipSuccess;
        oq->active = 1;
        pthread_mutex_unlock(&oq->mu);

        for (ci = 0; ci < nchunks && r.err == hipSuccess; ci++) {
                const mover_t in = {MOVE_ASYNC, c->s_in, {NULL, NULL}};
                const long long c0 = ci * (long long) chunk;
                const int clen = (int) ((long long) len - c0 < (long long) chunk ? len - c0 : (long long) chunk);
                char *h, *dargs;
                unsigned char *stage;
                int vec16, nslots;
                hipError_t e = hipSuccess;
                const char *what = NULL;
                b = (int) (ci % PIPE_NBUF);
                h = (char *) c->h_args + b * astride;
                dargs = (char *) c->d_args + b * astride;
                stage = c->d_stage + b * set_bytes;
#define PIPE_STEP(site, call)                                                                      \
        do {                                                                                       \
                if (e == hipSuccess) {                                                             \
                        e = isal_hip_fault_at(site, ci) ? hipErrorOutOfMemory : (call);            \
                        if (e != hipSuccess)                                                       \
                                what = #call;                                                      \
                }                                                                                  \
        } while (0)
                if (ci >= PIPE_NBUF) {
                        /* staging set b is free once chunk ci - NBUF's parity has left it
                         * (its copy-out event recorded), and argument region b once that
                         * chunk's upload ran */
                        if ((e = outq_wait(oq, ci - PIPE_NBUF + 1)) != hipSuccess)
                                break; /* the worker's failure, reported below */
                        PIPE_STEP(FAULT_SYNC, hipEventSynchronize(c->ev_k[b]));
                        PIPE_STEP(FAULT_NONE, hipStreamWaitEvent(c->s_in, c->ev_out[b], 0));
                }
                vec16 = fill_ptrs(q, (uint64_t *) h, c0, stage, slot);
                if (e == hipSuccess && (e = stage_in(q, ci, c0, (size_t) clen, stage, slot, &in)) != hipSuccess)
                        what = "hipMemcpyAsync(H2D chunk)";
                PIPE_STEP(FAULT_NONE, hipEventRecord(c->ev_in[b], c->s_in));
                PIPE_STEP(FAULT_NONE, hipStreamWaitEvent(c->stream, c->ev_in[b], 0));
                PIPE_STEP(FAULT_NONE, hipMemcpyAsync(dargs, h, L.args_bytes, hipMemcpyHostToDevice, c->stream));
                PIPE_STEP(FAULT_LAUNCH, launch_op(c, q, dargs, &L, clen, c0, vec16, &nslots));
                PIPE_STEP(FAULT_NONE, hipEventRecord(c->ev_k[b], c->stream));
#undef PIPE_STEP
                if (e != hipSuccess) {
                        r.err = e;
                        r.what = what;
                        break;
                }
                launched = ci + 1;
                pthread_mutex_lock(&oq->mu);
                oq->posted = launched;
                pthread_cond_signal(&oq->cv);
                pthread_mutex_unlock(&oq->mu);
        }
        /* let the worker finish the chunks that were launched (or fail) */
        (void) outq_wait(oq, launched);
        pthread_mutex_lock(&oq->mu);
        oq->active = 0;
        oq->call = NULL;
        if (oq->err != hipSuccess) { /* the first failure in chunk order is the worker's */
                r.err = oq->err;
                r.what = oq->what;
                r.done = oq->fail_chunk * (long long) chunk;
                r.chunk_end = r.done + (long long) chunk < len ? r.done + (long long) chunk : len;
                r.rows_out = oq->rows_out;
        } else {
                r.done = oq->handled * (long long) chunk < len ? oq->handled * (long long) chunk : len;
                r.rows_out = 0;
        }
        pthread_mutex_unlock(&oq->mu);
        if (r.err != hipSuccess)
                return r;
        GPU_TRY_ATC(r, FAULT_SYNC, nchunks - 1, hipStreamSynchronize(c->s_out));
        r.done = len;
        return r;
}

/* ---- finishing on the CPU --------------------------------------------------- */

static unsigned long long g_cpu_calls;

unsigned long long
isal_hip_cpu_calls(void)
{
        return __atomic_load_n(&g_cpu_calls, __ATOMIC_RELAXED);
}

unsigned long long
isal_hip_cpu_route(const ec_call *q, long long c0, int len)
{
        __atomic_add_fetch(&g_cpu_calls, 1ull, __ATOMIC_RELAXED);
        return isal_cpu_run(q->op, c0, len, q->k, q->rows, q->vec_i, q->gftbls, q->src, q->nsrc, q->dst);
}

int
isal_hip_finish_on_cpu(ctx_t *c, const ec_call *q, const gpu_res *r, unsigned long long *first_bad)
{
        long long done = r->done;
        /* Nothing queued may still write our outputs: drain every stream of the
         * call. Output copies into host memory were enqueued for [0, done) (and
         * rows_out rows beyond). */
        if (c && isal_hip_ctx_quiesce(c) != hipSuccess && (r->done > 0 || r->rows_out))
                return -1;
        if (q->op == OP_UPDATE && r->rows_out) {
                /* rows [0, rows_out) of [done, chunk_end) are already updated */
                unsigned char *s1 = q->src[0] + done, **d1;
                const int nr = q->rows - r->rows_out;
                ec_call rest = *q;
                int i;
                d1 = (unsigned char **) malloc(sizeof(*d1) * (size_t) (nr > 0 ? nr : 1));
                if (!d1)
                        abort();
                for (i = 0; i < nr; i++)
                        d1[i] = q->dst[r->rows_out + i] + done;
                rest.rows = nr;
                rest.gftbls = q->gftbls + (size_t) r->rows_out * q->k * 32;
                rest.src = &s1;
                rest.dst = d1;
                (void) isal_hip_cpu_route(&rest, 0, (int) (r->chunk_end - done));
                free(d1);
                done = r->chunk_end;
        }
        *first_bad = isal_hip_cpu_route(q, done, q->len);
        return 0;
}
