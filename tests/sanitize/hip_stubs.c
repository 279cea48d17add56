/*
 * hip_stubs.c — TEST INFRASTRUCTURE: the HIP runtime, the engine's device
 * switch and its reachability check as the *_host.c programs see them, the
 * helpers of their drivers, and a default for every kernel launcher the
 * stripe objects' host sources reference. A program defines the launchers it
 * drives; the weak ones here only fail. For stage_host.c, which links the
 * drop-in shim's staging routes and their context: streams, events,
 * page-locked memory and asynchronous copies, and the plain encode / update /
 * verify launchers as runs of the CPU route. For pipe_host.c, which links the
 * host pipeline and the multi-device encode: while g_hip_model is set (only
 * that program sets it, hm_start) streams, events, device memory, asynchronous
 * copies and the encode / update launchers go to the deferred model of
 * hip_model.c instead of completing at once.
 */
#include "hip_stubs.h"

int g_hip_calls, g_allocs, g_checks;
size_t g_check_len[64];
static volatile unsigned char g_sink;

hipError_t
hipGetDevice(int *d)
{
        if (g_hip_model)
                return hm_get_device(d);
        g_hip_calls++;
        *d = 0;
        return hipSuccess;
}

hipError_t
hipMalloc(void **p, size_t n)
{
        if (g_hip_model)
                return hm_malloc(p, n);
        g_hip_calls++;
        CHECK(n > 0);
        *p = malloc(n); /* exactly n: ASan guards the end of every table */
        g_allocs++;
        return *p ? hipSuccess : hipErrorOutOfMemory;
}

hipError_t
hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind kind)
{
        (void) kind;
        g_hip_calls++;
        memcpy(d, s, n);
        return hipSuccess;
}

hipError_t
hipFree(void *p)
{
        if (g_hip_model)
                return hm_free(p);
        free(p);
        g_allocs--;
        return hipSuccess;
}

/* ---- streams, events, page-locked memory and asynchronous copies, as the
 * drop-in shim's staging routes use them (stage_host.c): everything completes
 * at once, so a stream or an event is only a handle. These are also called by
 * the routes' worker thread, so they count nothing. */

static char g_handle;

hipError_t
hipStreamCreate(hipStream_t *s)
{
        if (g_hip_model)
                return hm_stream_create(s);
        *s = (hipStream_t) &g_handle;
        return hipSuccess;
}

hipError_t
hipStreamCreateWithFlags(hipStream_t *s, unsigned flags)
{
        (void) flags;
        return hipStreamCreate(s);
}

hipError_t
hipStreamDestroy(hipStream_t s)
{
        if (g_hip_model)
                return hm_stream_destroy(s);
        return hipSuccess;
}

hipError_t
hipStreamSynchronize(hipStream_t s)
{
        if (g_hip_model)
                return hm_stream_synchronize(s);
        return hipSuccess;
}

hipError_t
hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags)
{
        (void) flags;
        if (g_hip_model)
                return hm_stream_wait_event(s, e);
        return hipSuccess;
}

hipError_t
hipEventCreateWithFlags(hipEvent_t *e, unsigned flags)
{
        (void) flags;
        if (g_hip_model)
                return hm_event_create(e);
        *e = (hipEvent_t) &g_handle;
        return hipSuccess;
}

hipError_t
hipEventDestroy(hipEvent_t e)
{
        if (g_hip_model)
                return hm_event_destroy(e);
        return hipSuccess;
}

hipError_t
hipEventRecord(hipEvent_t e, hipStream_t s)
{
        if (g_hip_model)
                return hm_event_record(e, s);
        return hipSuccess;
}

hipError_t
hipEventSynchronize(hipEvent_t e)
{
        if (g_hip_model)
                return hm_event_synchronize(e);
        return hipSuccess;
}

hipError_t
hipHostMalloc(void **p, size_t n, unsigned flags)
{
        (void) flags;
        *p = malloc(n);
        return *p ? hipSuccess : hipErrorOutOfMemory;
}

hipError_t
hipHostFree(void *p)
{
        free(p);
        return hipSuccess;
}

hipError_t
hipHostGetDevicePointer(void **d, void *h, unsigned flags)
{
        (void) flags;
        *d = h;
        return hipSuccess;
}

hipError_t
hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind kind, hipStream_t stream)
{
        if (g_hip_model)
                return hm_memcpy_async(d, s, n, kind, stream);
        memcpy(d, s, n);
        return hipSuccess;
}

hipError_t
hipMemsetAsync(void *d, int value, size_t n, hipStream_t stream)
{
        if (g_hip_model)
                return hm_memset_async(d, value, n, stream);
        memset(d, value, n);
        return hipSuccess;
}

hipError_t
hipGetLastError(void)
{
        return hipSuccess;
}

hipError_t
hipSetDevice(int d)
{
        if (g_hip_model)
                return hm_set_device(d);
        return hipSuccess;
}

hipError_t
hipGetDeviceCount(int *n)
{
        if (g_hip_model)
                return hm_get_device_count(n);
        *n = 1;
        return hipSuccess;
}

/* a distinct bus id per device (none of them in any sysfs tree) */
hipError_t
hipDeviceGetPCIBusId(char *bus, int len, int dev)
{
        snprintf(bus, (size_t) len, "ffff:%02x:00.0", dev);
        return hipSuccess;
}

/* The plain (uploaded-argument) launchers: the CPU route (ec_cpu.c) over the
 * "device" pointer table and coefficient tables they are given, at once. A
 * verify writes two slot words — none, then its first mismatch with the
 * chunk's first column added — as the real launcher writes one per workgroup. */
int g_plain_launches;

static unsigned long long
plain_launch(int op, const uint64_t *d_ptrs, int src0, int nsrc, int dst0, const uint32_t *d_tbl, int len, int k,
             int rows, int vec_i, int vec16)
{
        unsigned char *g = calloc((size_t) 32 * k * rows, 1);
        unsigned char **p = malloc(sizeof(*p) * (size_t) (nsrc + rows));
        unsigned long long key;
        int i, l, j;
        CHECK(g && p);
        for (l = 0; l < rows; l++)
                for (j = 0; j < k; j++)
                        g[((size_t) l * k + j) * 32 + 1] = coef_of(d_tbl, k, rows, l, j);
        for (i = 0; i < nsrc + rows; i++) {
                p[i] = (unsigned char *) (uintptr_t) d_ptrs[i < nsrc ? src0 + i : dst0 + i - nsrc];
                CHECK(p[i] && (!vec16 || ((uintptr_t) p[i] & 15) == 0));
        }
        key = isal_cpu_run(op, 0, len, k, rows, vec_i, g, p, nsrc, p + nsrc);
        g_plain_launches++;
        free(g);
        free(p);
        return key;
}

/* The same launch as an operation of the deferred model: its arguments now,
 * the pointer table, the tables and the shards when its stream reaches it. */
typedef struct {
        int op, src0, nsrc, dst0, len, k, rows, vec_i, vec16;
        const uint64_t *d_ptrs;
        const uint32_t *d_tbl;
} launch_args;

static void
launch_run(void *arg)
{
        const launch_args *a = arg;
        (void) plain_launch(a->op, a->d_ptrs, a->src0, a->nsrc, a->dst0, a->d_tbl, a->len, a->k, a->rows, a->vec_i,
                            a->vec16);
}

static void
launch(void *stream, launch_args a)
{
        if (g_hip_model) {
                launch_args *h = malloc(sizeof(*h));
                CHECK(h);
                *h = a;
                hm_launch(stream, launch_run, h);
        } else
                launch_run(&a);
}

int
isal_hip_launch_encode(const uint64_t *d_ptrs, int ptr_stride, int src_idx0, int dst_idx0, const uint32_t *d_tbl,
                       int len, int k, int rows, long long nstripes, int vec16, const isal_hip_encmask *em,
                       void *stream)
{
        CHECK(nstripes == 1 && ptr_stride >= k + rows);
        launch(stream, (launch_args) {ISAL_HIP_OP_ENCODE, src_idx0, k, dst_idx0, len, k, rows, 0, vec16, d_ptrs, d_tbl});
        return 0;
}

int
isal_hip_launch_update(const uint64_t *d_ptrs, int ptr_stride, int src_idx, int dst_idx0, const uint32_t *d_tbl,
                       int len, int k, int rows, int vec_i, long long nstripes, int vec16, void *stream)
{
        CHECK(nstripes == 1 && ptr_stride >= 1 + rows);
        launch(stream, (launch_args) {ISAL_HIP_OP_UPDATE, src_idx, 1, dst_idx0, len, k, rows, vec_i, vec16, d_ptrs, d_tbl});
        return 0;
}

int
isal_hip_launch_verify(const uint64_t *d_ptrs, int ptr_stride, int src_idx0, int dst_idx0, const uint32_t *d_tbl,
                       int len, int k, int rows, long long col0, unsigned long long *slots, int *nslots, int vec16,
                       const isal_hip_encmask *em, void *stream)
{
        const unsigned long long key =
                plain_launch(ISAL_HIP_OP_VERIFY, d_ptrs, src_idx0, k, dst_idx0, d_tbl, len, k, rows, 0, vec16);
        CHECK(ptr_stride >= k + rows);
        slots[0] = ~0ull;
        slots[1] = key == ~0ull ? key : key + ((unsigned long long) col0 << 8);
        *nslots = 2;
        return 0;
}

int
isal_hip_dev_enter(int dev)
{
        int cur;
        if (g_hip_model) { /* as the engine's own: the device to restore, -1 when none */
                (void) hm_get_device(&cur);
                if (cur == dev)
                        return -1;
                return hm_set_device(dev) == hipSuccess ? cur : -2;
        }
        return -1;
}

void
isal_hip_dev_leave(int prev)
{
        if (g_hip_model && prev >= 0)
                (void) hm_set_device(prev);
}

/* Never over no bytes (zero-length stripes are not classified), and over the
 * length the shards have: the last byte of each is touched. */
int
isal_hip_batch_check_ptrs(const uint64_t *ptrs, size_t n, size_t len, int dev)
{
        size_t i;
        (void) dev;
        g_hip_calls++;
        CHECK(len > 0);
        if (g_checks < 64)
                g_check_len[g_checks] = len;
        g_checks++;
        for (i = 0; i < n; i++) {
                if (!ptrs[i])
                        return ISAL_HIP_EINVAL;
                g_sink = ((const unsigned char *) (uintptr_t) ptrs[i])[len - 1];
        }
        return ISAL_HIP_OK;
}

/* ---- the drivers' helpers ------------------------------------------------- */

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;

unsigned
rnd(unsigned n)
{
        rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
        return (unsigned) (rng_state >> 33) % n;
}

unsigned char *
shard(int len)
{
        unsigned char *p;
        CHECK(posix_memalign((void **) &p, 16, (size_t) (len ? len : 1)) == 0);
        return p;
}

unsigned char
coef_of(const uint32_t *tbl, int k, int rows, int l, int j)
{
        const int r0 = l / EC_MAX_ROWS_PER_PASS * EC_MAX_ROWS_PER_PASS;
        const int P = rows - r0 < EC_MAX_ROWS_PER_PASS ? rows - r0 : EC_MAX_ROWS_PER_PASS;
        const uint32_t *t = tbl + (size_t) EC_TBL_DWORDS * k * r0 + ((size_t) j * P + (l - r0)) * EC_TBL_DWORDS;
        return (unsigned char) (t[0] >> 8); /* entry 1 of c * {0..7} */
}

/* ---- the launchers a program does not drive -------------------------------- */

#define NOT_DRIVEN                                        \
        {                                                 \
                CHECK(!"not driven by this program");     \
                return 1;                                 \
        }

__attribute__((weak)) int
isal_hip_launch_repair(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_pat, const uint32_t *d_tbl,
                       unsigned tbl_stride, int len, int k, int rows, long long nrows, void *stream) NOT_DRIVEN

__attribute__((weak)) int
isal_hip_launch_repair_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_pat, const uint32_t *d_tbl,
                              const int *d_lens, const unsigned *d_items, unsigned nitems,
                              const unsigned *d_items_small, unsigned nitems_small, int k, int rows,
                              void *stream) NOT_DRIVEN

__attribute__((weak)) int
isal_hip_launch_overwrite(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_idx, const uint32_t *d_tbl,
                          int len, int k, int rows, int nw, long long nstripes, int commit, void *stream) NOT_DRIVEN

__attribute__((weak)) int
isal_hip_launch_overwrite_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_idx,
                                 const uint32_t *d_tbl, const int *d_lens, const int *d_nw, const unsigned *d_items,
                                 unsigned nitems, int k, int rows, int max_nw, int commit, void *stream) NOT_DRIVEN

__attribute__((weak)) int
isal_hip_launch_locate_batch(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_tbl, int len, int k,
                             int rows, long long nstripes, const isal_hip_encmask *em, const unsigned char *d_loc,
                             unsigned *verdict, void *stream) NOT_DRIVEN

__attribute__((weak)) int
isal_hip_launch_locate_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_tbl, const int *d_lens,
                              const unsigned *d_items, unsigned nitems, int k, int rows, long long nstripes,
                              const unsigned char *d_loc, unsigned *verdict, void *stream) NOT_DRIVEN

__attribute__((weak)) int
isal_hip_launch_encode_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_tbl, const int *d_lens,
                              const unsigned *d_items, unsigned nitems, const unsigned *d_items_small,
                              unsigned nitems_small, int k, int rows, void *stream) NOT_DRIVEN

__attribute__((weak)) int
isal_hip_launch_verify_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_tbl, const int *d_lens,
                              const unsigned *d_items, unsigned nitems, int k, int rows, long long nstripes,
                              unsigned long long *bad, void *stream) NOT_DRIVEN
