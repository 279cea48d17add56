/*
 * hip_stubs.h — TEST INFRASTRUCTURE: what the *_host.c programs of this
 * directory share (hip_stubs.c). Each of them links the stripe objects' host
 * sources (isa-l_amd/csrc/isal_hip_{objects,repair,overwrite,scrub,ragged}.c)
 * against a HIP runtime where "device" memory is host memory, so the program
 * needs no GPU and what a create() uploads can be read back. stage_host.c
 * drives the drop-in shim's staging routes (isal_hip_stage.c, isal_hip_ctx.c)
 * on the same runtime. pipe_host.c drives the host pipeline and the
 * multi-device encode (isal_hip_pipe.c, isal_hip_multi.c) on the deferred model
 * of HIP streams declared below (hip_model.c).
 */
#ifndef HIP_STUBS_H
#define HIP_STUBS_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "erasure_code.h"
#include "isal_hip.h"
#include "isal_hip_internal.h"

#define CHECK(c)                                                                 \
        do {                                                                     \
                if (!(c)) {                                                      \
                        fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
                        exit(1);                                                 \
                }                                                                \
        } while (0)

/* hipGetDevice, hipMalloc, hipMemcpy and reachability queries so far: a
 * refusal that leaves it alone came before the first HIP call */
extern int g_hip_calls;
/* device allocations alive */
extern int g_allocs;
/* launches of the stubbed plain launchers (isal_hip_launch_encode / update / verify) */
extern int g_plain_launches;
/* reachability queries so far, and the length of each of the first 64 */
extern int g_checks;
extern size_t g_check_len[64];

/* ---- the deferred model of HIP streams (hip_model.c), for pipe_host.c -------
 * Off (0) unless a program calls hm_start(): then streams, events, device
 * memory, asynchronous copies and the plain launchers go through the model,
 * where nothing runs before the host waits for it. */
extern int g_hip_model;
enum { HM_NDEV = 3, HM_POISON = 0xC7 };
/* a stream's role: the order a pipeline creates its three streams in */
enum { HM_ROLE_H2D, HM_ROLE_COMP, HM_ROLE_D2H };
enum { HM_H2D, HM_D2H, HM_MEMSET, HM_LAUNCH, HM_RECORD, HM_WAIT };
enum { HM_ENQUEUED, HM_EXECUTED };
typedef struct {
        int dev, role, kind; /* the stream's device and role; HM_H2D ... HM_WAIT */
        const void *host;    /* copies: the host side's address */
        size_t n;            /* copies and memsets: bytes */
} hm_rec;
/* model on; order = the roles from the stream that moves first to the one
 * that moves last; empties both logs */
void hm_start(const int order[3]);
/* model off (no stream or event may be alive) */
void hm_stop(void);
/* strict (the default): recording an event again while its last record is
 * still queued ends the program. 0 lifts that, for reading what else a
 * defect breaks. */
void hm_strict_events(int on);
/* every operation enqueued / executed since the logs were last emptied */
size_t hm_log(int which, const hm_rec **out);
void hm_log_clear(void);
/* operations still queued on device dev (-1: on any) */
size_t hm_pending(int dev);
int hm_live_streams(void);
int hm_live_events(void);
/* hip_stubs.c forwards to these while the model is on */
hipError_t hm_get_device_count(int *n);
hipError_t hm_get_device(int *d);
hipError_t hm_set_device(int d);
hipError_t hm_malloc(void **p, size_t n);
hipError_t hm_free(void *p);
hipError_t hm_stream_create(hipStream_t *s);
hipError_t hm_stream_synchronize(hipStream_t s);
hipError_t hm_stream_destroy(hipStream_t s);
hipError_t hm_event_create(hipEvent_t *e);
hipError_t hm_event_destroy(hipEvent_t e);
hipError_t hm_event_record(hipEvent_t e, hipStream_t s);
hipError_t hm_event_synchronize(hipEvent_t e);
hipError_t hm_stream_wait_event(hipStream_t s, hipEvent_t e);
hipError_t hm_memcpy_async(void *d, const void *s, size_t n, hipMemcpyKind kind, hipStream_t stream);
hipError_t hm_memset_async(void *d, int value, size_t n, hipStream_t stream);
void hm_launch(void *stream, void (*fn)(void *), void *arg);

unsigned rnd(unsigned n);
/* exactly len bytes (one byte at len 0, never touched), 16-byte aligned: a
 * multiple of 16 would hide an overrun of up to 15 bytes */
unsigned char *shard(int len);
/* coefficient (row l of all rows, source j) of a device table image: pass
 * g = l / 8 starts at dword 5 * k * 8g and is laid out [j][l < P][5] */
unsigned char coef_of(const uint32_t *tbl, int k, int rows, int l, int j);

#endif /* HIP_STUBS_H */
