/*
 * isal_hip_shim.c — the C-ABI boundary of the MI355X erasure-code engine.
 *
 * Exports the reference's data-path symbols (erasure_code.h, gf_vect_mul.h:
 * ec_encode_data, ec_encode_data_update, gf_vect_dot_prod, gf_vect_mad,
 * gf_vect_mul and their *_base twins); the checksum entry points (crc.h,
 * crc64.h) live in isal_hip_crcapi.c, the batched extension (isal_hip.h) in
 * isal_hip_batch.c.
 * Replaces the reference's L2 dispatch + L3 glue (ec_multibinary.asm:79-93,
 * ec_highlevel_func.c:159-698): instead of picking a CPU ISA, calls are
 * routed to the GPU kernels in ec_kernels.hip (small host-resident calls: the
 * CPU route, ec_cpu.c).
 *
 * Per call (run_ec):
 *   1. classify every shard pointer (device/managed vs host) with
 *      hipPointerGetAttributes;
 *   2. route: host-resident calls of at most ISAL_HIP_CPU_MAX_BYTES run on the
 *      CPU route (ec_cpu.c) — the GPU round trip costs more than the work, as
 *      the reference's own short-length fallback recognises
 *      (ec_highlevel_func.c:159-194); ISAL_HIP_BACKEND=gpu|cpu|auto overrides;
 *   3. otherwise describe the call once (ec_call, isal_hip_shim.h) and hand it
 *      to a route: kernel arguments for device-resident stripes
 *      (isal_hip_karg.c), else host-resident shards staged through a per-thread
 *      pinned or HBM buffer (zero-copy / packed / column-chunked / pipelined,
 *      isal_hip_stage.c) — the reference API is synchronous.
 *
 * Failures: the reference API has no error return, so a host-resident call
 * must not fail where the reference would succeed. A failing HIP call hands
 * the columns that are not yet final to the CPU route (reported once on
 * stderr). Only a call with device-resident shards — which no CPU route can
 * serve — or one made under ISAL_HIP_BACKEND=gpu aborts.
 * Thread safety: all mutable state is per thread (the context of
 * isal_hip_ctx.c) except the atomic counters and the read-once knobs.
 */
#define _GNU_SOURCE /* dladdr */
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "erasure_code.h"
#include "isal_hip_shim.h"

/* ---- errors, counters, routing log -------------------------------------- */

void
isal_hip_die(const char *what, hipError_t e)
{
        fprintf(stderr,
                "isal_hip: %s failed: %s (%d) on a call with device-resident shards (or with "
                "ISAL_HIP_BACKEND=gpu); no CPU route can serve it, aborting\n",
                what, hipGetErrorString(e), (int) e);
        abort();
}

static unsigned long long g_launches, g_fallbacks;

void
isal_hip_count_launch(void)
{
        __atomic_add_fetch(&g_launches, 1ull, __ATOMIC_RELAXED);
}

unsigned long long
isal_hip_kernel_launches(void)
{
        return __atomic_load_n(&g_launches, __ATOMIC_RELAXED);
}

unsigned long long
isal_hip_fallbacks(void)
{
        return __atomic_load_n(&g_fallbacks, __ATOMIC_RELAXED);
}

/* ---- kernel registry --------------------------------------------------------
 * Filled while the library loads (static initialisers of the kernel objects,
 * ec_device.h KernelReg), read by isal_hip_selftest_kernels. */
#define KREG_MAX 4096
static const void *kreg_fn[KREG_MAX];
static const char *kreg_name[KREG_MAX];
static int kreg_n, kreg_lost;

void
isal_hip_kreg_add(const void *fn, const char *name)
{
        const int i = __atomic_fetch_add(&kreg_n, 1, __ATOMIC_RELAXED);
        if (i >= KREG_MAX) {
                __atomic_add_fetch(&kreg_lost, 1, __ATOMIC_RELAXED);
                return;
        }
        kreg_fn[i] = fn;
        kreg_name[i] = name;
}

int
isal_hip_selftest_kernels(int *nkernels)
{
        int i, n = __atomic_load_n(&kreg_n, __ATOMIC_ACQUIRE), bad = 0;
        if (n > KREG_MAX)
                n = KREG_MAX;
        if (nkernels)
                *nkernels = n;
        if (__atomic_load_n(&kreg_lost, __ATOMIC_RELAXED))
                return ISAL_HIP_ENOMEM; /* the registry is too small to vouch for every kernel */
        if (!isal_hip_gpu_present())
                return ISAL_HIP_EHIP;
        for (i = 0; i < n; i++) {
                hipFuncAttributes a;
                const hipError_t e = hipFuncGetAttributes(&a, kreg_fn[i]);
                if (e != hipSuccess) {
                        Dl_info info;
                        const int found = dladdr(kreg_fn[i], &info) != 0;
                        (void) hipGetLastError();
                        fprintf(stderr,
                                "isal_hip: selftest: kernel with no usable device code: %s (handle %s+0x%lx): "
                                "%s\n",
                                kreg_name[i], found ? info.dli_fname : "?",
                                found ? (unsigned long) ((const char *) kreg_fn[i] - (const char *) info.dli_fbase)
                                      : 0ul,
                                hipGetErrorString(e));
                        bad++;
                }
        }
        return bad;
}

int
isal_hip_max_rows_per_pass(void)
{
        return EC_MAX_ROWS_PER_PASS;
}

const char *
isal_hip_target(void)
{
        return "gfx950";
}

static const char *const op_names[] = {"encode", "update", "verify"};

/* ISAL_HIP_LOG=1: one stderr line per drop-in call naming the route taken. */
static void
route_log(int op, int len, int k, int rows, const char *route, const char *why)
{
        if (isal_hip_knob(ISAL_HIP_KNOB_LOG) > 0)
                fprintf(stderr, "isal_hip: %s len=%d k=%d rows=%d -> %s (%s)\n", op_names[op], len,
                        k, rows, route, why);
}

/* A HIP failure under a host-resident call: reported once per process (every
 * time with ISAL_HIP_LOG=1), then the call finishes on the CPU route. */
static void
report_fallback(const char *what, hipError_t e)
{
        static int reported;
        __atomic_add_fetch(&g_fallbacks, 1ull, __ATOMIC_RELAXED);
        if (!__atomic_exchange_n(&reported, 1, __ATOMIC_RELAXED) ||
            isal_hip_knob(ISAL_HIP_KNOB_LOG) > 0)
                fprintf(stderr,
                        "isal_hip: %s failed: %s (%d); host-resident calls fall back to the CPU "
                        "route (reported once; ISAL_HIP_LOG=1 reports each)\n",
                        what, hipGetErrorString(e), (int) e);
}

int
isal_hip_backend(void)
{
        const long long v = isal_hip_knob(ISAL_HIP_KNOB_BACKEND);
        static int warned;
        if (v == -2 && !__atomic_exchange_n(&warned, 1, __ATOMIC_RELAXED))
                fprintf(stderr, "isal_hip: ISAL_HIP_BACKEND must be auto, gpu or cpu; using auto\n");
        return v == BACKEND_GPU || v == BACKEND_CPU ? (int) v : BACKEND_AUTO;
}

/* Host calls of at most this many shard bytes ((k + rows) * len) take the CPU
 * route under ISAL_HIP_BACKEND=auto (override: ISAL_HIP_CPU_MAX_BYTES). Below
 * it the ~30 us GPU round trip costs more than the arithmetic (DESIGN.md §3,
 * measured crossover in profiles/r02/r02_route_crossover.txt). */
#define DEFAULT_CPU_MAX_BYTES ((size_t) 8 << 20)

static size_t
cpu_max_bytes(void)
{
        const long long v = isal_hip_knob(ISAL_HIP_KNOB_CPU_MAX_BYTES);
        return v >= 0 ? (size_t) v : DEFAULT_CPU_MAX_BYTES;
}

/* The same limit for calls whose host shards are all page-locked and used in
 * place by the kernels (no staging copy): there the GPU wins from 1.8 MB
 * (k = 10, p = 4: 51.6 vs 59.1 us; 14.7 MB: 290 vs 497 us,
 * profiles/r03/r03_route_crossover_c.jsonl). Override: ISAL_HIP_CPU_MAX_BYTES_PINNED
 * (ISAL_HIP_CPU_MAX_BYTES also lowers it). */
#define DEFAULT_CPU_MAX_BYTES_PINNED ((size_t) 2 << 20)

static size_t
cpu_max_bytes_pinned(void)
{
        const long long v = isal_hip_knob(ISAL_HIP_KNOB_CPU_MAX_BYTES_PINNED);
        const size_t all = cpu_max_bytes();
        if (v >= 0)
                return (size_t) v;
        return all < DEFAULT_CPU_MAX_BYTES_PINNED ? all : DEFAULT_CPU_MAX_BYTES_PINNED;
}

/* Is a GPU usable at all? (Asked once: a host without one, or without a
 * working driver, serves every host-resident call on the CPU route.) */
static int gpu_ok;
static pthread_once_t gpu_once = PTHREAD_ONCE_INIT;

static void
gpu_probe(void)
{
        int n = 0;
        gpu_ok = hipGetDeviceCount(&n) == hipSuccess && n > 0;
        if (!gpu_ok)
                (void) hipGetLastError();
}

int
isal_hip_gpu_present(void)
{
        pthread_once(&gpu_once, gpu_probe);
        return gpu_ok;
}

/* ---- pointer classification ------------------------------------------- */

/* Where a shard lives (kind; ISAL_HIP_MEM_*) and, for device and page-locked
 * memory, the device its attributes name (*dev; -1 otherwise). Returns what a
 * kernel would use for it: device (hipMalloc) and managed memory, the pointer
 * itself; page-locked host memory (hipHostMalloc, hipHostRegister — NIC / disk
 * DMA buffers usually are), the device's mapping of it, which kernels of THAT
 * device read and write in place over PCIe with no staging copy
 * (ISAL_HIP_PINNED_DIRECT=0 stages it like pageable memory) — but only when
 * the shard's LAST byte maps through the same registration too: a shard that
 * runs past the end of a partly registered buffer would make the kernel touch
 * unmapped memory (a GPU fault the CPU route could not recover from), so it is
 * staged (kind pageable). Pageable memory: 0 — it is copied through a staging
 * buffer. For device memory *rbase / *rsize receive its allocation's range. */
uint64_t
isal_hip_classify(const void *p, size_t len, int *kind, int *dev, uintptr_t *rbase, size_t *rsize)
{
        hipPointerAttribute_t a, z;
        hipError_t e;
        *kind = CL_HOST;
        *dev = -1;
        *rsize = 0;
        if (!p)
                return 0;
        e = hipPointerGetAttributes(&a, p);
        if (e != hipSuccess) {
                (void) hipGetLastError(); /* unknown to HIP: plain host memory */
                return 0;
        }
        if (a.type == hipMemoryTypeDevice) {
                hipDeviceptr_t base;
                size_t size;
                *kind = CL_DEVICE;
                *dev = a.device;
                if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t) p) == hipSuccess) {
                        *rbase = (uintptr_t) base;
                        *rsize = size;
                } else {
                        (void) hipGetLastError();
                }
                return (uint64_t) (uintptr_t) p;
        }
        if (a.type == hipMemoryTypeManaged || a.type == hipMemoryTypeUnified) {
                *kind = CL_MANAGED;
                return (uint64_t) (uintptr_t) p;
        }
        if (a.type == hipMemoryTypeHost && a.devicePointer &&
            isal_hip_knob(ISAL_HIP_KNOB_PINNED_DIRECT) != 0) {
                /* attributes describe p itself (the mapping of the allocation
                 * base plus p's offset into it) */
                const char *last = (const char *) p + (len ? len - 1 : 0);
                if (len > 1) {
                        if (hipPointerGetAttributes(&z, last) != hipSuccess) {
                                (void) hipGetLastError();
                                return 0;
                        }
                        if (z.type != hipMemoryTypeHost || z.device != a.device ||
                            (const char *) z.devicePointer != (const char *) a.devicePointer + (len - 1))
                                return 0;
                }
                *kind = CL_PINNED;
                *dev = a.device;
                return (uint64_t) (uintptr_t) a.devicePointer;
        }
        return 0;
}

/* The device a drop-in call runs on (isal_hip.h). The reference API has no
 * device argument (erasure_code.h:108-110), so it comes from the shards: the
 * device that holds the call's device-resident (hipMalloc) shards — they must
 * all be on one; managed memory does not bind a device — else the caller's
 * current device. A page-locked host shard is used in place only through the
 * mapping made for the chosen device (its own); otherwise it is staged. */
int
isal_hip_route_device(int n, const int *kind, const int *dev, int cur, int *bad, int *in_place)
{
        int i, owner = -1;
        if (bad)
                *bad = -1;
        if (n < 0 || (n > 0 && (!kind || !dev)))
                return -3;
        for (i = 0; i < n; i++) {
                if (kind[i] != CL_DEVICE)
                        continue;
                if (owner < 0) {
                        owner = dev[i];
                } else if (dev[i] != owner) {
                        if (bad)
                                *bad = i;
                        return -2;
                }
        }
        if (owner < 0)
                owner = cur;
        if (in_place)
                for (i = 0; i < n; i++)
                        in_place[i] = kind[i] == CL_DEVICE || kind[i] == CL_MANAGED ||
                                      (kind[i] == CL_PINNED && owner >= 0 && dev[i] == owner);
        return owner;
}

/* ---- the generic synchronous call --------------------------------------- */

/*
 * Routes of one synchronous call:
 *   cpu        every shard host-resident and (k + rows) * len <= cpu_max_bytes
 *              (ISAL_HIP_BACKEND=auto), or ISAL_HIP_BACKEND=cpu, or no GPU:
 *              ec_cpu.c. The routing itself still asks HIP (once per process
 *              for the device count, then hipPointerGetAttributes per shard
 *              pointer, ~1 us each), so even ISAL_HIP_BACKEND=cpu initialises
 *              the HIP runtime when a GPU is present; the arithmetic makes no
 *              HIP call;
 *   zero-copy  len * (k + rows) <= ZC_BYTES: pointer table, coefficient tables,
 *              host-resident shards and verify slots all live in the pinned
 *              buffer and the kernel reads/writes them over PCIe — the call is
 *              one launch and one stream sync;
 *   packed     host-staged bytes <= PACK_BYTES: the same layout, moved with one
 *              H2D and one D2H DMA into/out of HBM;
 *   chunked    larger: shards staged per column chunk, one at a time or
 *              pipelined (isal_hip_stage.c).
 * A stripe of device-resident shards that fits the kernel argument block takes
 * none of these: isal_hip_karg.c.
 * A HIP failure in a host-resident call hands the columns not yet final to the
 * CPU route; with any device-resident shard (or ISAL_HIP_BACKEND=gpu) it aborts.
 */
#define ZC_BYTES ((size_t) 256 << 10)
#define PACK_BYTES ((size_t) 4 << 20)

/* A call whose device-resident shards sit on two GPUs: no one kernel can
 * reach both (and no CPU route can read either). */
static void
die_mixed(const char *fn, int i0, int d0, int i1, int d1)
{
        fprintf(stderr,
                "isal_hip: %s: device-resident shards on two GPUs (shard %d on device %d, shard %d "
                "on device %d); one call runs on one GPU, aborting\n",
                fn, i0, d0, i1, d1);
        abort();
}

/*
 * OP_ENCODE: dst[l] = XOR_j c[l][j] * src[j], nsrc = k.
 * OP_UPDATE: dst[l] ^= c[l][vec_i] * src[0], nsrc = 1.
 * OP_VERIFY: compare dst[l] with XOR_j c[l][j] * src[j]; nothing is written.
 * Returns ~0 (no mismatch / not a verify) or the first mismatch as
 * column << 8 | row. fn names the entry point in abort messages.
 * The call runs on the device holding its device-resident shards
 * (isal_hip_route_device): the thread's current device is switched to it for
 * the call and restored before returning.
 */
static unsigned long long
run_ec(const char *fn, int op, int len, int k, int rows, int vec_i, const unsigned char *gftbls,
       unsigned char *const *src, int nsrc, unsigned char *const *dst)
{
        static const isal_hip_encmask no_masks;
        const int be = isal_hip_backend();
        const int nptr = nsrc + rows;
        uint64_t view_buf[512], *view;
        ec_staged plan_buf[512], *plan;
        int kind_buf[512], dev_buf[512], *kind, *devs;
        /* the call, described once for every route: what the caller passed
         * now, what is derived from it (view, plan, tables) below */
        ec_call q = {fn, op, len, k, rows, vec_i, gftbls, src, nsrc, dst, nptr, NULL, 0, 0, 0, NULL, NULL, &no_masks};
        seen_t sn;
        int i, ndev = 0, nplain = 0, all_host, cur_dev, run_dev, bad, mail;
        unsigned long long first_bad;
        size_t bytes;
        gpu_res r = GPU_RES_INIT;
        ctx_t *c;

        if (len <= 0 || rows <= 0 || k < 0)
                return ~0ull;
        if (op == OP_UPDATE && (vec_i < 0 || vec_i >= k)) {
                /* Out-of-range vec_i is undefined in the reference (it reads past
                 * gftbls); here it must not become an out-of-bounds GPU access. */
                fprintf(stderr, "isal_hip: ec update with vec_i=%d outside [0,%d): ignored\n",
                        vec_i, k);
                return ~0ull;
        }
        bytes = (size_t) len * (size_t) nptr;
        if (!isal_hip_gpu_present()) {
                if (be == BACKEND_GPU) {
                        fprintf(stderr, "isal_hip: ISAL_HIP_BACKEND=gpu but no GPU is usable\n");
                        abort();
                }
                /* no HIP runtime to ask: every pointer is a host pointer */
                route_log(op, len, k, rows, "cpu", "no GPU");
                return isal_hip_cpu_route(&q, 0, len);
        }

        if (nptr <= 512) {
                view = view_buf;
                plan = plan_buf;
                kind = kind_buf;
                devs = dev_buf;
        } else {
                view = (uint64_t *) malloc((sizeof(uint64_t) + sizeof(ec_staged) + 2 * sizeof(int)) * (size_t) nptr);
                if (!view) {
                        fprintf(stderr, "isal_hip: out of host memory\n");
                        abort();
                }
                plan = (ec_staged *) (view + nptr);
                kind = (int *) (plan + nptr);
                devs = kind + nptr;
        }
        if (hipGetDevice(&cur_dev) != hipSuccess) {
                (void) hipGetLastError();
                cur_dev = -1; /* no page-locked shard is used in place */
        }
        sn.n = 0;
        for (i = 0; i < nptr; i++) {
                const void *p = i < nsrc ? src[i] : dst[i - nsrc];
                uintptr_t rb = 0;
                size_t rs = 0;
                const int sd = seen_dev(&sn, p, (size_t) len);
                if (sd >= 0) {
                        view[i] = (uint64_t) (uintptr_t) p;
                        kind[i] = CL_DEVICE;
                        devs[i] = sd;
                } else {
                        view[i] = isal_hip_classify(p, (size_t) len, &kind[i], &devs[i], &rb, &rs);
                        if (kind[i] == CL_DEVICE)
                                seen_add(&sn, rb, rs, devs[i]);
                }
        }
        /* the device the call runs on (-1: none known, the caller's current
         * device could not be read) */
        run_dev = isal_hip_route_device(nptr, kind, devs, cur_dev, &bad, NULL);
        if (run_dev == -2) {
                int i0 = 0;
                while (kind[i0] != CL_DEVICE)
                        i0++;
                die_mixed(fn, i0, devs[i0], bad, devs[bad]);
        }
        for (i = 0; i < nptr; i++) {
                const int is_dev = kind[i] == CL_DEVICE || kind[i] == CL_MANAGED;
                /* page-locked memory is used in place only through the run
                 * device's own mapping */
                if (kind[i] == CL_PINNED && devs[i] != run_dev)
                        view[i] = 0;
                nplain += kind[i] == CL_DEVICE;
                /* An update's parity in page-locked host memory is staged, not
                 * written in place: a kernel that failed after it started could
                 * have folded some of it already, and the CPU fallback could not
                 * tell which bytes. (Encode overwrites, verify only reads.) */
                if (op == OP_UPDATE && i >= nsrc && view[i] && !is_dev)
                        view[i] = 0;
                ndev += is_dev;
                if (!view[i]) { /* staged: the next slot of the plan */
                        plan[q.nstage].ptr = i;
                        plan[q.nstage].row = i < nsrc ? -1 : i - nsrc;
                        q.nstage_src += i < nsrc;
                        q.nstage++;
                }
        }
        /* sources, and outputs of a read-modify-write update or of a verify,
         * go in */
        q.nstage_in = op == OP_ENCODE ? q.nstage_src : q.nstage;
        q.view = view;
        q.plan = plan;
        all_host = ndev == 0;

        if (all_host && (be == BACKEND_CPU ||
                         (be == BACKEND_AUTO &&
                          bytes <= (q.nstage == 0 ? cpu_max_bytes_pinned() : cpu_max_bytes())))) {
                if (view != view_buf)
                        free(view);
                route_log(op, len, k, rows, "cpu", be == BACKEND_CPU ? "ISAL_HIP_BACKEND=cpu" : "small host call");
                return isal_hip_cpu_route(&q, 0, len);
        }

        /* the shards' device, when the caller's current device is another one */
        if (run_dev != cur_dev && (r.err = hipSetDevice(run_dev)) != hipSuccess)
                isal_hip_die("hipSetDevice (to the device holding the shards)", r.err);
        c = isal_hip_ctx_get(run_dev, &r.err, &r.what);
        if (c && !(q.tbl = isal_hip_ctx_tables(c, k, rows, gftbls, &q.em))) {
                r.err = hipErrorOutOfMemory;
                r.what = "ctx_tables (host memory)";
                c = NULL;
        }
        if (c && op == OP_UPDATE)
                q.em = &no_masks;
        if (!c) {
                r.done = 0;
        } else if (ndev == nptr && (mail = nplain == nptr && isal_hip_knob(ISAL_HIP_KNOB_KARG_DONE) != 0,
                                    op != OP_VERIFY || mail) &&
                   isal_hip_karg_fits(&q)) {
                route_log(op, len, k, rows, "gpu kernel-args", "device shards");
                r = isal_hip_gpu_karg(c, &q, mail);
        } else if (bytes <= ZC_BYTES || (q.nstage && (size_t) len * (size_t) q.nstage <= PACK_BYTES)) {
                const int zc = bytes <= ZC_BYTES;
                route_log(op, len, k, rows, zc ? "gpu zero-copy" : "gpu packed",
                          all_host ? "host shards" : "device shards");
                r = isal_hip_gpu_small(c, &q, zc);
        } else {
                const int piped = q.nstage && op != OP_VERIFY && isal_hip_knob(ISAL_HIP_KNOB_PIPE_CHUNKS) != 0;
                route_log(op, len, k, rows,
                          piped ? "gpu pipelined chunks" : q.nstage ? "gpu chunked" : "gpu direct (no staging)",
                          all_host ? "host shards" : "device shards");
                r = piped ? isal_hip_gpu_pipelined(c, &q) : isal_hip_gpu_chunked(c, &q);
        }
        if (view != view_buf)
                free(view);
        q.view = NULL; /* freed with the plan: completing the call on the CPU needs neither */
        q.plan = NULL;
        if (r.err == hipSuccess) {
                if (run_dev != cur_dev)
                        (void) hipSetDevice(cur_dev);
                return r.first_bad;
        }
        if (!all_host || be == BACKEND_GPU)
                isal_hip_die(r.what, r.err);
        /* all shards host-resident: the call ran on the caller's own device */
        (void) hipGetLastError();
        report_fallback(r.what, r.err);
        if (isal_hip_finish_on_cpu(c, &q, &r, &first_bad) != 0)
                isal_hip_die("draining the streams after a failed call (output state unknown)", r.err);
        return first_bad;
}

unsigned long long
isal_hip_run(const char *fn, int op, int len, int k, int rows, int vec_i, const unsigned char *gftbls,
             unsigned char *const *src, int nsrc, unsigned char *const *dst)
{
        return run_ec(fn, op, len, k, rows, vec_i, gftbls, src, nsrc, dst);
}

/* ---- reference data-path ABI ------------------------------------------- */

void
ec_encode_data(int len, int k, int rows, unsigned char *gftbls, unsigned char **data,
               unsigned char **coding)
{
        run_ec("ec_encode_data", OP_ENCODE, len, k, rows, 0, gftbls, data, k, coding);
}

void
ec_encode_data_base(int len, int k, int rows, unsigned char *gftbls, unsigned char **data,
                    unsigned char **coding)
{
        run_ec("ec_encode_data_base", OP_ENCODE, len, k, rows, 0, gftbls, data, k, coding);
}

void
ec_encode_data_update(int len, int k, int rows, int vec_i, unsigned char *gftbls,
                      unsigned char *data, unsigned char **coding)
{
        run_ec("ec_encode_data_update", OP_UPDATE, len, k, rows, vec_i, gftbls, &data, 1, coding);
}

void
ec_encode_data_update_base(int len, int k, int rows, int vec_i, unsigned char *gftbls,
                           unsigned char *data, unsigned char **coding)
{
        run_ec("ec_encode_data_update_base", OP_UPDATE, len, k, rows, vec_i, gftbls, &data, 1, coding);
}

void
gf_vect_dot_prod(int len, int vlen, unsigned char *gftbls, unsigned char **src,
                 unsigned char *dest)
{
        run_ec("gf_vect_dot_prod", OP_ENCODE, len, vlen, 1, 0, gftbls, src, vlen, &dest);
}

void
gf_vect_dot_prod_base(int len, int vlen, unsigned char *gftbls, unsigned char **src,
                      unsigned char *dest)
{
        run_ec("gf_vect_dot_prod_base", OP_ENCODE, len, vlen, 1, 0, gftbls, src, vlen, &dest);
}

void
gf_vect_mad(int len, int vec, int vec_i, unsigned char *gftbls, unsigned char *src,
            unsigned char *dest)
{
        run_ec("gf_vect_mad", OP_UPDATE, len, vec, 1, vec_i, gftbls, &src, 1, &dest);
}

void
gf_vect_mad_base(int len, int vec, int vec_i, unsigned char *gftbls, unsigned char *src,
                 unsigned char *dest)
{
        run_ec("gf_vect_mad_base", OP_UPDATE, len, vec, 1, vec_i, gftbls, &src, 1, &dest);
}

/* dest = c * src with c = gftbl[1]; -1 (nothing touched) when len % 32 != 0,
 * as ec_base.c:350-353. */
int
gf_vect_mul(int len, unsigned char *gftbl, void *src, void *dest)
{
        unsigned char *s = (unsigned char *) src, *d = (unsigned char *) dest;
        if (len % 32)
                return -1;
        run_ec("gf_vect_mul", OP_ENCODE, len, 1, 1, 0, gftbl, &s, 1, &d);
        return 0;
}

int
gf_vect_mul_base(int len, unsigned char *gftbl, unsigned char *src, unsigned char *dest)
{
        return gf_vect_mul(len, gftbl, src, dest);
}

/* ---- device of an object's calls ------------------------------------------ */

/* Make dev the calling thread's current device for one call on an object that
 * belongs to it (a batch, a pipeline). Returns the device to restore with
 * isal_hip_dev_leave (-1: no switch was needed), or -2 when the switch failed. */
int
isal_hip_dev_enter(int dev)
{
        int cur;
        if (hipGetDevice(&cur) != hipSuccess) {
                (void) hipGetLastError();
                return -1;
        }
        if (cur == dev)
                return -1;
        if (hipSetDevice(dev) != hipSuccess) {
                (void) hipGetLastError();
                return -2;
        }
        return cur;
}

void
isal_hip_dev_leave(int prev)
{
        if (prev >= 0)
                (void) hipSetDevice(prev);
}

