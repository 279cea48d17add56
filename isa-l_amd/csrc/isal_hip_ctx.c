/*
 * isal_hip_ctx.c — the drop-in shim's per-thread, per-device context (ctx_t,
 * isal_hip_shim.h): the call stream, the argument and staging buffers, the
 * pipeline's streams and events, and the cached coefficient tables of the
 * thread's last call. All of it is owned by one thread (a pthread key), so
 * nothing here locks.
 */
#include <hip/hip_runtime_api.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "isal_hip_shim.h"

static pthread_key_t ctx_key;
static pthread_once_t ctx_once = PTHREAD_ONCE_INIT;

/* A calling thread's contexts, one per device it has made calls on: a thread
 * that serves shards on several GPUs keeps each GPU's stream, buffers and
 * mailbox instead of rebuilding them on every device switch. */
#define CTX_MAX_DEV 64
typedef struct {
        ctx_t *dev[CTX_MAX_DEV];
} tctx_t;

static unsigned long long g_ctx_created;

unsigned long long
isal_hip_contexts_created(void)
{
        return __atomic_load_n(&g_ctx_created, __ATOMIC_RELAXED);
}

static void
ctx_free(ctx_t *c)
{
        if (!c)
                return;
        /* Best effort at thread exit: the runtime may already be shutting down. */
        if (c->stream)
                (void) hipStreamDestroy(c->stream);
        if (c->d_args)
                (void) hipFree(c->d_args);
        if (c->h_args)
                (void) hipHostFree(c->h_args);
        if (c->d_stage)
                (void) hipFree(c->d_stage);
        if (c->d_done)
                (void) hipFree(c->d_done);
        if (c->h_mail)
                (void) hipHostFree((void *) c->h_mail);
        if (c->oq)
                isal_hip_outq_stop(c);
        if (c->c32.d_tabs)
                (void) hipFree(c->c32.d_tabs);
        for (int v = 0; v < ISAL_HIP_CRC64_NVARIANTS; v++)
                if (c->c64[v].d_tabs)
                        (void) hipFree(c->c64[v].d_tabs);
        if (c->d_cpart)
                (void) hipFree(c->d_cpart);
        if (c->d_ldsx)
                (void) hipFree(c->d_ldsx);
        free(c->jobs);
        free(c->tcoef);
        free(c->ttbl);
        if (c->pipe_ready) {
                int b;
                (void) hipStreamDestroy(c->s_in);
                (void) hipStreamDestroy(c->s_out);
                for (b = 0; b < PIPE_NBUF; b++) {
                        (void) hipEventDestroy(c->ev_in[b]);
                        (void) hipEventDestroy(c->ev_k[b]);
                        (void) hipEventDestroy(c->ev_out[b]);
                }
        }
        free(c);
}

static void
tctx_release(void *p)
{
        tctx_t *t = (tctx_t *) p;
        int d;
        if (!t)
                return;
        for (d = 0; d < CTX_MAX_DEV; d++)
                ctx_free(t->dev[d]);
        free(t);
}

static void
ctx_key_init(void)
{
        if (pthread_key_create(&ctx_key, tctx_release) != 0) {
                fprintf(stderr, "isal_hip: pthread_key_create failed\n");
                abort();
        }
}

ctx_t *
isal_hip_ctx_get(int dev, hipError_t *err, const char **what)
{
        tctx_t *t;
        ctx_t *c;
        pthread_once(&ctx_once, ctx_key_init);
        if (dev < 0 || dev >= CTX_MAX_DEV) {
                *err = hipErrorInvalidDevice;
                *what = "device ordinal (at most 64 GPUs per process)";
                return NULL;
        }
        t = (tctx_t *) pthread_getspecific(ctx_key);
        if (!t) {
                t = (tctx_t *) calloc(1, sizeof(*t));
                if (!t || pthread_setspecific(ctx_key, t) != 0) {
                        fprintf(stderr, "isal_hip: out of host memory\n");
                        abort();
                }
        }
        if ((c = t->dev[dev]) != NULL)
                return c;
        c = (ctx_t *) calloc(1, sizeof(*c));
        if (!c) {
                fprintf(stderr, "isal_hip: out of host memory\n");
                abort();
        }
        c->device = dev;
        /* A BLOCKING stream: it is ordered after work already queued on the
         * legacy default stream (e.g. torch kernels that just wrote the
         * shards), as the synchronous reference API implies. */
        if ((*err = hipStreamCreate(&c->stream)) != hipSuccess) {
                *what = "hipStreamCreate";
                free(c);
                return NULL;
        }
        t->dev[dev] = c;
        __atomic_add_fetch(&g_ctx_created, 1ull, __ATOMIC_RELAXED);
        return c;
}

/* Rebuilt only when the coefficients differ from the thread's last call (a
 * storage caller encodes stripe after stripe with one matrix; the rebuild is
 * ~5k table lookups for k = 10, p = 4). */
const uint32_t *
isal_hip_ctx_tables(ctx_t *c, int k, int rows, const unsigned char *gftbls, const isal_hip_encmask **em)
{
        const size_t n = (size_t) k * (size_t) rows, nd = isal_hip_tables_dwords(k, rows);
        const unsigned gen = isal_hip_knob_generation();
        size_t i;
        int hit = c->ttbl && c->tk == k && c->trows == rows && c->tgen == gen;
        for (i = 0; hit && i < n; i++)
                hit = c->tcoef[i] == gftbls[i * 32 + 1];
        if (!hit) {
                if (n > c->tcap_coef) {
                        unsigned char *x = (unsigned char *) realloc(c->tcoef, n);
                        if (!x)
                                return NULL;
                        c->tcoef = x;
                        c->tcap_coef = n;
                }
                /* k = 0 (the empty sum: zero parity) has no tables at all; keep
                 * one dword so that only a failed allocation returns NULL */
                if (nd > c->tcap_tbl || !c->ttbl) {
                        const size_t cap = nd ? nd : 1;
                        uint32_t *x = (uint32_t *) realloc(c->ttbl, cap * 4);
                        if (!x)
                                return NULL;
                        c->ttbl = x;
                        c->tcap_tbl = cap;
                }
                c->tk = -1; /* not valid until rebuilt */
                c->ldsx_ok = 0;
                for (i = 0; i < n; i++)
                        c->tcoef[i] = gftbls[i * 32 + 1];
                isal_hip_build_tables(k, rows, gftbls, c->ttbl);
                isal_hip_enc_masks(k, rows, gftbls, &c->tem);
                c->tk = k;
                c->trows = rows;
                c->tgen = gen;
        }
        *em = &c->tem;
        return c->ttbl;
}

/* The LDS product tables of the thread's cached coefficients
 * (isal_hip_ctx_tables) on the device, uploaded when the coefficients change;
 * NULL (the call then keeps the v_perm kernel) when memory runs out. The
 * upload is synchronous and no kernel of this context is in flight: every
 * drop-in call has completed before the next one starts. */
const uint64_t *
isal_hip_ctx_ldsx(ctx_t *c, int k, int rows)
{
        const size_t nw = isal_hip_ldsx_words(k, rows);
        uint64_t *h;
        if (c->ldsx_ok)
                return c->d_ldsx;
        if (nw > c->ldsx_cap) {
                if (c->d_ldsx)
                        (void) hipFree(c->d_ldsx);
                c->d_ldsx = NULL;
                c->ldsx_cap = 0;
                if (hipMalloc((void **) &c->d_ldsx, nw * 8) != hipSuccess) {
                        c->d_ldsx = NULL;
                        return NULL;
                }
                c->ldsx_cap = nw;
        }
        if (!(h = (uint64_t *) malloc(nw * 8)))
                return NULL;
        isal_hip_build_ldsx_tables_coef(k, rows, c->tcoef, h);
        if (hipMemcpy(c->d_ldsx, h, nw * 8, hipMemcpyHostToDevice) == hipSuccess)
                c->ldsx_ok = 1;
        free(h);
        return c->ldsx_ok ? c->d_ldsx : NULL;
}

hipError_t
isal_hip_ctx_args(ctx_t *c, size_t bytes)
{
        size_t cap;
        hipError_t e;
        if (bytes <= c->args_cap)
                return hipSuccess;
        cap = c->args_cap ? c->args_cap : 64 * 1024;
        while (cap < bytes)
                cap *= 2;
        if (c->d_args)
                (void) hipFree(c->d_args);
        if (c->h_args)
                (void) hipHostFree(c->h_args);
        c->d_args = c->h_args = c->h_args_dev = NULL;
        c->args_cap = 0;
        if ((e = hipMalloc(&c->d_args, cap)) != hipSuccess)
                return e;
        /* coherent: kernels of the zero-copy path read arguments and shards the
         * host just wrote, and the host reads what they wrote, with no cached
         * copies in between */
        if ((e = hipHostMalloc(&c->h_args, cap, hipHostMallocCoherent)) != hipSuccess ||
            (e = hipHostGetDevicePointer(&c->h_args_dev, c->h_args, 0)) != hipSuccess) {
                (void) hipFree(c->d_args);
                if (c->h_args)
                        (void) hipHostFree(c->h_args);
                c->d_args = c->h_args = c->h_args_dev = NULL;
                return e;
        }
        c->args_cap = cap;
        return hipSuccess;
}

hipError_t
isal_hip_ctx_stage(ctx_t *c, size_t bytes)
{
        hipError_t e;
        if (bytes <= c->stage_cap)
                return hipSuccess;
        if (c->d_stage)
                (void) hipFree(c->d_stage);
        c->d_stage = NULL;
        c->stage_cap = 0;
        if ((e = hipMalloc((void **) &c->d_stage, bytes)) != hipSuccess)
                return e;
        c->stage_cap = bytes;
        return hipSuccess;
}

hipError_t
isal_hip_ctx_pipe(ctx_t *c)
{
        hipError_t e;
        int b;
        if (c->pipe_ready)
                return hipSuccess;
        if ((e = hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking)) != hipSuccess)
                return e;
        if ((e = hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking)) != hipSuccess) {
                (void) hipStreamDestroy(c->s_in);
                return e;
        }
        for (b = 0; b < PIPE_NBUF; b++) {
                if ((e = hipEventCreateWithFlags(&c->ev_in[b], hipEventDisableTiming)) != hipSuccess ||
                    (e = hipEventCreateWithFlags(&c->ev_k[b], hipEventDisableTiming)) != hipSuccess ||
                    (e = hipEventCreateWithFlags(&c->ev_out[b], hipEventDisableTiming)) != hipSuccess) {
                        /* leak the few created events: this only happens when the
                         * runtime is failing anyway */
                        (void) hipStreamDestroy(c->s_in);
                        (void) hipStreamDestroy(c->s_out);
                        return e;
                }
        }
        c->pipe_ready = 1;
        return hipSuccess;
}

hipError_t
isal_hip_ctx_quiesce(ctx_t *c)
{
        hipError_t e = hipStreamSynchronize(c->stream), e2;
        if (c->pipe_ready) {
                if ((e2 = hipStreamSynchronize(c->s_in)) != hipSuccess && e == hipSuccess)
                        e = e2;
                if ((e2 = hipStreamSynchronize(c->s_out)) != hipSuccess && e == hipSuccess)
                        e = e2;
        }
        return e;
}
