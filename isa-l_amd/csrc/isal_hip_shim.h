/*
 * isal_hip_shim.h — what the translation units of the drop-in shim share. Not
 * installed, and nothing here is exported (exports.map).
 *
 *   isal_hip_shim.c    routing: backend and thresholds, pointer classification,
 *                      run_ec, the reference ABI entry points, counters
 *   isal_hip_ctx.c     the per-thread, per-device context (ctx_t)
 *   isal_hip_karg.c    kernel-argument calls and their mailbox completion
 *   isal_hip_stage.c   the host staging routes and their copy-out worker, the
 *                      CPU completion of a call whose route failed
 *   isal_hip_crcapi.c  the checksum entry points (crc.h, crc64.h)
 *
 * One drop-in call is described once, by run_ec, in an ec_call; every route
 * reads it.
 */
#ifndef ISAL_HIP_SHIM_H
#define ISAL_HIP_SHIM_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "isal_hip.h"
#include "isal_hip_internal.h"

enum { OP_ENCODE = ISAL_HIP_OP_ENCODE, OP_UPDATE = ISAL_HIP_OP_UPDATE, OP_VERIFY = ISAL_HIP_OP_VERIFY };

/* ---- per-thread context (isal_hip_ctx.c) --------------------------------- */

/* Large host calls are cut into column chunks that flow through PIPE_NBUF
 * staging buffers: the H2D copy of chunk i+1, the kernel of chunk i and the
 * D2H copy of chunk i-1 run at once on three streams. */
#define PIPE_NBUF 3

typedef struct {
        int device;
        hipStream_t stream;
        void *d_args; /* device: pointer table + coefficient tables */
        void *h_args; /* pinned mirror of d_args (fine-grained, coherent) */
        void *h_args_dev; /* the same pinned buffer as seen by kernels (zero-copy) */
        size_t args_cap;
        unsigned char *d_stage; /* device scratch for host-resident shards */
        size_t stage_cap;
        /* pipelined column chunks (isal_hip_gpu_pipelined): copy-in / copy-out
         * streams and per-buffer events, created on first use */
        hipStream_t s_in, s_out;
        hipEvent_t ev_in[PIPE_NBUF], ev_k[PIPE_NBUF], ev_out[PIPE_NBUF];
        int pipe_ready;
        struct outq *oq; /* the call thread's copy-out worker (isal_hip_stage.c) */
        struct copyjob *jobs; /* [3]: worker's copies in / out, this thread's list */
        /* the last call's derived coefficient tables and 0/1 masks, reused
         * while its coefficients (byte 1 of each gftbls entry) repeat */
        int tk, trows;
        unsigned tgen;
        unsigned char *tcoef;
        uint32_t *ttbl;
        size_t tcap_coef, tcap_tbl;
        isal_hip_encmask tem;
        /* the same coefficients' LDS product tables on the device (drop-in
         * encodes of 7-8 rows, isal_hip_karg_ldsx), built on first use */
        uint64_t *d_ldsx;
        size_t ldsx_cap;
        int ldsx_ok;
        /* completion of kernel-argument calls (isal_hip_kdone): device words
         * {arrival counter, verify result}, the page-locked host mailbox
         * {seq, result} and its device view, the last sequence number, and
         * calls since the stream was last synchronised */
        void *d_done;
        volatile unsigned long long *h_mail;
        void *h_mail_dev;
        unsigned long long seq;
        int unsynced;
        /* checksum entry points on device buffers: kernel tables of the last
         * geometry per flavour (CRC32C, the eight CRC64) and the partials */
        struct crcc {
                long long len;
                int tt;
                void *d_tabs;
        } c32, c64[ISAL_HIP_CRC64_NVARIANTS];
        void *d_cpart;
        size_t cpart_cap;
} ctx_t;

/* The calling thread's context on device dev — which must be the thread's
 * current device when the context is first made (its stream belongs to the
 * current device) — or NULL with *err and *what set. */
ctx_t *isal_hip_ctx_get(int dev, hipError_t *err, const char **what);
/* The call's device coefficient tables (isal_hip_build_tables layout) and 0/1
 * masks, cached while the coefficients repeat; NULL when out of memory. */
const uint32_t *isal_hip_ctx_tables(ctx_t *c, int k, int rows, const unsigned char *gftbls,
                                    const isal_hip_encmask **em);
/* The cached coefficients' LDS product tables on the device, or NULL. */
const uint64_t *isal_hip_ctx_ldsx(ctx_t *c, int k, int rows);
/* Grow the argument buffers / the staging buffer to at least `bytes`; make
 * the pipeline's streams and events. */
hipError_t isal_hip_ctx_args(ctx_t *c, size_t bytes);
hipError_t isal_hip_ctx_stage(ctx_t *c, size_t bytes);
hipError_t isal_hip_ctx_pipe(ctx_t *c);
/* Wait for everything a call queued; the first error, if any. */
hipError_t isal_hip_ctx_quiesce(ctx_t *c);

/* ---- one drop-in call ------------------------------------------------------ */

/* A staged shard: a host-resident shard no kernel reaches in place, copied
 * through slot s of a staging buffer, s being its place in ec_call.plan. The
 * plan is in pointer order, so the staged sources come first (slots
 * [0, nstage_src)) and the staged outputs follow in row order. Slots
 * [0, nstage_in) are copied in before the kernel: the sources, and for an
 * update (read-modify-write) or a verify the outputs too. */
typedef struct {
        int ptr; /* index into the call's pointers: nsrc sources, then rows outputs */
        int row; /* the output row, -1 for a source */
} ec_staged;

typedef struct {
        const char *fn; /* the entry point, for abort messages */
        int op, len, k, rows, vec_i;
        const unsigned char *gftbls;
        unsigned char *const *src;
        int nsrc;
        unsigned char *const *dst;
        int nptr; /* nsrc + rows */
        /* per pointer: the address a kernel uses for a shard it reaches in
         * place, 0 for a staged one */
        const uint64_t *view;
        int nstage, nstage_src, nstage_in;
        const ec_staged *plan; /* [nstage] */
        /* the derived device coefficient tables and 0/1 masks */
        const uint32_t *tbl;
        const isal_hip_encmask *em;
} ec_call;

/* Outcome of a GPU attempt: on failure `what`/`err` name the HIP call and
 * columns [0, done) are final, so a fallback redoes only [done, len). An
 * update (read-modify-write) that failed while copying a chunk's parity back
 * also reports how many output rows of [done, chunk_end) had their copy
 * enqueued (rows_out): those must not be folded twice. */
typedef struct {
        hipError_t err;
        const char *what;
        long long done, chunk_end;
        int rows_out;
        unsigned long long first_bad;
} gpu_res;

#define GPU_RES_INIT {hipSuccess, NULL, 0, 0, 0, ~0ull}

/* Fault injection (tests): ISAL_HIP_FAULT=<site> makes every GPU-routed call
 * fail at that site as if the HIP call there had returned an error, without
 * issuing it — the fallback paths then run for real. The sites (FAULT_*) are
 * listed in isal_hip_internal.h. ISAL_HIP_FAULT_CHUNK=n narrows the fault to
 * column chunk n of a call, so the fallback also runs after earlier chunks
 * finished on the GPU. */
int isal_hip_fault_at(int site, long long chunk);

#define GPU_TRY_ATC(r, site, chunk, call)                                                          \
        do {                                                                                       \
                hipError_t e_ = isal_hip_fault_at(site, chunk) ? hipErrorOutOfMemory : (call);     \
                if (e_ != hipSuccess) {                                                            \
                        (r).err = e_;                                                              \
                        (r).what = #call;                                                          \
                        return (r);                                                                \
                }                                                                                  \
        } while (0)

#define GPU_TRY_AT(r, site, call) GPU_TRY_ATC(r, site, 0, call)

#define GPU_TRY(r, call)                                                                           \
        do {                                                                                       \
                hipError_t e_ = (call);                                                            \
                if (e_ != hipSuccess) {                                                            \
                        (r).err = e_;                                                              \
                        (r).what = #call;                                                          \
                        return (r);                                                                \
                }                                                                                  \
        } while (0)

/* ---- the staging routes (isal_hip_stage.c) -------------------------------- */

/* HBM staging bytes per host call (ISAL_HIP_STAGE_MB). */
size_t isal_hip_stage_limit(void);
/* zero-copy and packed modes: whole shards, one chunk */
gpu_res isal_hip_gpu_small(ctx_t *c, const ec_call *q, int zero_copy);
/* column chunks one at a time (whole shards when nothing is staged) */
gpu_res isal_hip_gpu_chunked(ctx_t *c, const ec_call *q);
/* column chunks through PIPE_NBUF staging sets, copies and kernels overlapped */
gpu_res isal_hip_gpu_pipelined(ctx_t *c, const ec_call *q);
/* Stop and free c's copy-out worker (c->oq is set). */
void isal_hip_outq_stop(ctx_t *c);

/* The CPU route (ec_cpu.c) over columns [c0, len) of the call, counted in
 * isal_hip_cpu_calls(). */
unsigned long long isal_hip_cpu_route(const ec_call *q, long long c0, int len);
/* Finish on the CPU route a host-resident call whose GPU route failed with
 * *r (c: its context, or NULL when there was none). Returns the call's
 * result in *first_bad and 0 — or -1, nothing written, when the streams could
 * not be drained while output copies may be under way: their state is unknown
 * and no CPU result may be written over them. */
int isal_hip_finish_on_cpu(ctx_t *c, const ec_call *q, const gpu_res *r, unsigned long long *first_bad);

/* ---- kernel-argument calls (isal_hip_karg.c) ------------------------------- */

/* Whether the call (every shard device-resident) fits the 2 KiB kernel
 * argument block; the call itself. mail: complete through the host mailbox. */
int isal_hip_karg_fits(const ec_call *q);
gpu_res isal_hip_gpu_karg(ctx_t *c, const ec_call *q, int mail);

/* ---- routing (isal_hip_shim.c), as the checksum entry points use it ------- */

enum { BACKEND_AUTO = 0, BACKEND_GPU = 1, BACKEND_CPU = 2 };
int isal_hip_backend(void);
int isal_hip_gpu_present(void);
void isal_hip_die(const char *what, hipError_t e);
enum {
        CL_HOST = ISAL_HIP_MEM_PAGEABLE,
        CL_DEVICE = ISAL_HIP_MEM_DEVICE,
        CL_MANAGED = ISAL_HIP_MEM_MANAGED,
        CL_PINNED = ISAL_HIP_MEM_PINNED,
};
uint64_t isal_hip_classify(const void *p, size_t len, int *kind, int *dev, uintptr_t *rbase, size_t *rsize);

#endif /* ISAL_HIP_SHIM_H */
