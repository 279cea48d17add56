/*
 * hip_model.c — TEST INFRASTRUCTURE: a deferred model of HIP streams for
 * pipe_host.c, in place of the complete-at-once runtime of hip_stubs.c. It is
 * off until a program calls hm_start(); the other *_host programs never do.
 *
 * A stream is a FIFO of operations: an asynchronous copy, an asynchronous
 * memset, a launch (a closure of hip_stubs.c with its arguments captured), an
 * event record or an event wait. NOTHING runs when it is enqueued. A copy
 * reads its source when it executes — the latest moment the API allows, since
 * a pipeline's host buffers must stay valid until its flush. Operations run
 * only while the host waits (hipEventSynchronize, hipStreamSynchronize, the
 * destruction of a stream or an event, hipFree), one at a time and only until
 * what the host waits for holds. Which stream moves next, among those whose
 * head may run, follows a fixed priority order over the three streams a
 * pipeline creates (h2d, compute, d2h, by creation order on their device):
 * under the six orders every edge the pipeline forgot lets some operation
 * overtake the one it depends on.
 *
 *   hipStreamWaitEvent  captures the event's most recent record at the call;
 *                       a wait on a never-recorded event is no operation
 *   hipEventRecord      the record completes when its stream reaches it. The
 *                       model also holds the pipeline to one discipline that
 *                       HIP itself does not demand: an event is not recorded
 *                       again while an earlier record of it is still queued
 *                       (an event belongs to one slot, and a slot is reused
 *                       only after its last stripe left it)
 *   hipMemcpy           synchronous and unordered with non-blocking streams,
 *                       which are the only streams here: it copies at once
 *   hipMalloc           memory comes back filled with HM_POISON, so parity
 *                       copied out before it was computed cannot be right
 *   devices             HM_NDEV of them; the current device is per thread; a
 *                       stream or an event belongs to the device current when
 *                       it was created; a host wait moves only the streams of
 *                       the device of what it waits for
 *
 * One mutex guards everything, so the multi-device workers' threads may call
 * in at once. Every operation is logged when it is enqueued and again when it
 * executes, with its device, its stream's role and (copies) the host address
 * and size.
 */
#include <pthread.h>

#include "hip_stubs.h"

int g_hip_model;

enum { HM_MAX_STREAMS = 64 };

typedef struct hm_event {
        int dev;
        unsigned long long recorded, completed; /* number of its last record made / executed */
} hm_event;

typedef struct hm_op {
        int kind;
        void *dst;
        const void *src;
        size_t n;
        int value;
        void (*fn)(void *);
        void *arg;
        hm_event *ev;
        unsigned long long seq;
        struct hm_op *next;
} hm_op;

typedef struct hm_stream {
        int dev, role;
        hm_op *head, *tail;
} hm_stream;

static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER;
static __thread int t_dev;
static hm_stream *g_streams[HM_MAX_STREAMS];
static int g_created[HM_NDEV]; /* streams ever created on each device: role = count % 3 */
static int g_order[3] = {HM_ROLE_H2D, HM_ROLE_COMP, HM_ROLE_D2H};
static int g_live_streams, g_live_events, g_lenient;
static struct {
        hm_rec *v;
        size_t n, cap;
} g_log[2];

static void
log_op(int which, const hm_stream *s, const hm_op *op)
{
        hm_rec *r;
        if (g_log[which].n == g_log[which].cap) {
                g_log[which].cap = g_log[which].cap ? 2 * g_log[which].cap : 1024;
                g_log[which].v = realloc(g_log[which].v, g_log[which].cap * sizeof(hm_rec));
                CHECK(g_log[which].v);
        }
        r = &g_log[which].v[g_log[which].n++];
        r->dev = s->dev;
        r->role = s->role;
        r->kind = op->kind;
        r->host = op->kind == HM_H2D ? op->src : op->kind == HM_D2H ? op->dst : NULL;
        r->n = op->n;
}

void
hm_start(const int order[3])
{
        int i;
        CHECK(order[0] + order[1] + order[2] == 3 && order[0] != order[1] && order[1] != order[2] &&
              order[0] != order[2]);
        pthread_mutex_lock(&g_lock);
        g_hip_model = 1;
        for (i = 0; i < 3; i++)
                g_order[i] = order[i];
        for (i = 0; i < HM_NDEV; i++)
                g_created[i] = 0; /* the next stream of every device is an h2d one again */
        g_log[HM_ENQUEUED].n = g_log[HM_EXECUTED].n = 0;
        pthread_mutex_unlock(&g_lock);
}

void
hm_stop(void)
{
        int i;
        pthread_mutex_lock(&g_lock);
        CHECK(g_live_streams == 0 && g_live_events == 0);
        g_hip_model = 0;
        for (i = 0; i < 2; i++) {
                free(g_log[i].v);
                g_log[i].v = NULL;
                g_log[i].n = g_log[i].cap = 0;
        }
        pthread_mutex_unlock(&g_lock);
}

void
hm_strict_events(int on)
{
        g_lenient = !on;
}

size_t
hm_log(int which, const hm_rec **out)
{
        size_t n;
        pthread_mutex_lock(&g_lock);
        *out = g_log[which].v;
        n = g_log[which].n;
        pthread_mutex_unlock(&g_lock);
        return n;
}

void
hm_log_clear(void)
{
        pthread_mutex_lock(&g_lock);
        g_log[HM_ENQUEUED].n = g_log[HM_EXECUTED].n = 0;
        pthread_mutex_unlock(&g_lock);
}

size_t
hm_pending(int dev)
{
        size_t n = 0;
        int i;
        const hm_op *op;
        pthread_mutex_lock(&g_lock);
        for (i = 0; i < HM_MAX_STREAMS; i++)
                if (g_streams[i] && (dev < 0 || g_streams[i]->dev == dev))
                        for (op = g_streams[i]->head; op; op = op->next)
                                n++;
        pthread_mutex_unlock(&g_lock);
        return n;
}

int
hm_live_streams(void)
{
        return g_live_streams;
}

int
hm_live_events(void)
{
        return g_live_events;
}

/* ---- the scheduler (lock held) --------------------------------------------- */

static int
runnable(const hm_stream *s)
{
        const hm_op *op = s->head;
        return op && !(op->kind == HM_WAIT && op->ev && op->ev->completed < op->seq);
}

static void
run_head(hm_stream *s)
{
        hm_op *op = s->head;
        s->head = op->next;
        if (!s->head)
                s->tail = NULL;
        switch (op->kind) {
        case HM_H2D:
        case HM_D2H:
                memcpy(op->dst, op->src, op->n);
                break;
        case HM_MEMSET:
                memset(op->dst, op->value, op->n);
                break;
        case HM_LAUNCH:
                op->fn(op->arg);
                free(op->arg);
                break;
        case HM_RECORD:
                if (op->ev->completed < op->seq)
                        op->ev->completed = op->seq;
                break;
        default: /* a wait whose record has completed */
                break;
        }
        log_op(HM_EXECUTED, s, op);
        free(op);
}

/* one operation of device dev: the head of the first stream, in priority
 * order, that may run; 0 when none may */
static int
step(int dev)
{
        int pr, i;
        for (pr = 0; pr < 3; pr++)
                for (i = 0; i < HM_MAX_STREAMS; i++) {
                        hm_stream *s = g_streams[i];
                        if (s && s->dev == dev && s->role == g_order[pr] && runnable(s)) {
                                run_head(s);
                                return 1;
                        }
                }
        return 0;
}

/* what a host wait waits for: the stream is empty / this record of the event
 * has completed / the device is idle. Work is left queued the moment it holds. */
static void
wait_until(int dev, const hm_stream *s, const hm_event *e, unsigned long long seq)
{
        for (;;) {
                int busy = 0, i;
                if (s)
                        busy = s->head != NULL;
                else if (e)
                        busy = e->completed < seq;
                else
                        for (i = 0; i < HM_MAX_STREAMS; i++)
                                busy |= g_streams[i] && g_streams[i]->dev == dev && g_streams[i]->head;
                if (!busy)
                        return;
                if (!step(dev)) {
                        fprintf(stderr, "hip_model: device %d cannot make progress (a wait on a record that never runs)\n",
                                dev);
                        exit(1);
                }
        }
}

static void
enqueue(hipStream_t stream, hm_op *op)
{
        hm_stream *s = (hm_stream *) stream;
        CHECK(s && op); /* the pipeline never uses the null stream */
        op->next = NULL;
        if (s->tail)
                s->tail->next = op;
        else
                s->head = op;
        s->tail = op;
        log_op(HM_ENQUEUED, s, op);
}

static hm_op *
new_op(int kind)
{
        hm_op *op = calloc(1, sizeof(*op));
        CHECK(op);
        op->kind = kind;
        return op;
}

/* ---- what hip_stubs.c hands over when the model is on ------------------------ */

hipError_t
hm_get_device_count(int *n)
{
        *n = HM_NDEV;
        return hipSuccess;
}

hipError_t
hm_get_device(int *d)
{
        *d = t_dev;
        return hipSuccess;
}

hipError_t
hm_set_device(int d)
{
        if (d < 0 || d >= HM_NDEV)
                return hipErrorInvalidDevice;
        t_dev = d;
        return hipSuccess;
}

hipError_t
hm_malloc(void **p, size_t n)
{
        CHECK(n > 0);
        *p = malloc(n); /* exactly n: ASan guards the end of every slot */
        if (!*p)
                return hipErrorOutOfMemory;
        memset(*p, HM_POISON, n);
        pthread_mutex_lock(&g_lock);
        g_allocs++;
        pthread_mutex_unlock(&g_lock);
        return hipSuccess;
}

/* hipFree waits for the device, as the runtime's does */
hipError_t
hm_free(void *p)
{
        pthread_mutex_lock(&g_lock);
        wait_until(t_dev, NULL, NULL, 0);
        g_allocs--;
        pthread_mutex_unlock(&g_lock);
        free(p);
        return hipSuccess;
}

hipError_t
hm_stream_create(hipStream_t *out)
{
        hm_stream *s = calloc(1, sizeof(*s));
        int i;
        CHECK(s);
        pthread_mutex_lock(&g_lock);
        s->dev = t_dev;
        s->role = g_created[t_dev]++ % 3;
        for (i = 0; i < HM_MAX_STREAMS && g_streams[i]; i++)
                ;
        CHECK(i < HM_MAX_STREAMS);
        g_streams[i] = s;
        g_live_streams++;
        pthread_mutex_unlock(&g_lock);
        *out = (hipStream_t) s;
        return hipSuccess;
}

hipError_t
hm_stream_synchronize(hipStream_t stream)
{
        hm_stream *s = (hm_stream *) stream;
        CHECK(s);
        pthread_mutex_lock(&g_lock);
        wait_until(s->dev, s, NULL, 0);
        pthread_mutex_unlock(&g_lock);
        return hipSuccess;
}

hipError_t
hm_stream_destroy(hipStream_t stream)
{
        hm_stream *s = (hm_stream *) stream;
        int i;
        CHECK(s);
        pthread_mutex_lock(&g_lock);
        wait_until(s->dev, s, NULL, 0);
        for (i = 0; i < HM_MAX_STREAMS && g_streams[i] != s; i++)
                ;
        CHECK(i < HM_MAX_STREAMS);
        g_streams[i] = NULL;
        g_live_streams--;
        pthread_mutex_unlock(&g_lock);
        free(s);
        return hipSuccess;
}

hipError_t
hm_event_create(hipEvent_t *out)
{
        hm_event *e = calloc(1, sizeof(*e));
        CHECK(e);
        pthread_mutex_lock(&g_lock);
        e->dev = t_dev;
        g_live_events++;
        pthread_mutex_unlock(&g_lock);
        *out = (hipEvent_t) e;
        return hipSuccess;
}

hipError_t
hm_event_destroy(hipEvent_t event)
{
        hm_event *e = (hm_event *) event;
        hm_op *op;
        int i;
        CHECK(e);
        pthread_mutex_lock(&g_lock);
        wait_until(e->dev, NULL, e, e->recorded);
        /* waits still queued behind other work have nothing left to wait for */
        for (i = 0; i < HM_MAX_STREAMS; i++)
                for (op = g_streams[i] ? g_streams[i]->head : NULL; op; op = op->next)
                        if (op->ev == e) {
                                CHECK(op->kind == HM_WAIT);
                                op->ev = NULL;
                        }
        g_live_events--;
        pthread_mutex_unlock(&g_lock);
        free(e);
        return hipSuccess;
}

hipError_t
hm_event_record(hipEvent_t event, hipStream_t stream)
{
        hm_event *e = (hm_event *) event;
        hm_op *op = new_op(HM_RECORD);
        CHECK(e);
        pthread_mutex_lock(&g_lock);
        if (e->completed < e->recorded && !g_lenient) {
                fprintf(stderr, "hip_model: an event is recorded again while its last record is still queued\n");
                exit(1);
        }
        op->ev = e;
        op->seq = ++e->recorded;
        enqueue(stream, op);
        pthread_mutex_unlock(&g_lock);
        return hipSuccess;
}

hipError_t
hm_event_synchronize(hipEvent_t event)
{
        hm_event *e = (hm_event *) event;
        CHECK(e);
        pthread_mutex_lock(&g_lock);
        wait_until(e->dev, NULL, e, e->recorded);
        pthread_mutex_unlock(&g_lock);
        return hipSuccess;
}

hipError_t
hm_stream_wait_event(hipStream_t stream, hipEvent_t event)
{
        hm_event *e = (hm_event *) event;
        CHECK(e);
        pthread_mutex_lock(&g_lock);
        if (e->recorded) {
                hm_op *op = new_op(HM_WAIT);
                op->ev = e;
                op->seq = e->recorded;
                enqueue(stream, op);
        }
        pthread_mutex_unlock(&g_lock);
        return hipSuccess;
}

hipError_t
hm_memcpy_async(void *d, const void *s, size_t n, hipMemcpyKind kind, hipStream_t stream)
{
        hm_op *op;
        CHECK(kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToHost);
        op = new_op(kind == hipMemcpyHostToDevice ? HM_H2D : HM_D2H);
        op->dst = d;
        op->src = s;
        op->n = n;
        pthread_mutex_lock(&g_lock);
        enqueue(stream, op);
        pthread_mutex_unlock(&g_lock);
        return hipSuccess;
}

hipError_t
hm_memset_async(void *d, int value, size_t n, hipStream_t stream)
{
        hm_op *op = new_op(HM_MEMSET);
        op->dst = d;
        op->value = value;
        op->n = n;
        pthread_mutex_lock(&g_lock);
        enqueue(stream, op);
        pthread_mutex_unlock(&g_lock);
        return hipSuccess;
}

/* arg is heap memory the model frees after fn(arg) ran */
void
hm_launch(void *stream, void (*fn)(void *), void *arg)
{
        hm_op *op = new_op(HM_LAUNCH);
        op->fn = fn;
        op->arg = arg;
        pthread_mutex_lock(&g_lock);
        enqueue((hipStream_t) stream, op);
        pthread_mutex_unlock(&g_lock);
}
