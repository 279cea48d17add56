/*
 * hip_stubs.h — TEST INFRASTRUCTURE: what the *_host.c programs of this
 * directory share (hip_stubs.c). Each of them links the stripe objects' host
 * sources (isa-l_amd/csrc/isal_hip_{objects,repair,overwrite,scrub,ragged}.c)
 * against a HIP runtime where "device" memory is host memory, so the program
 * needs no GPU and what a create() uploads can be read back. stage_host.c
 * drives the drop-in shim's staging routes (isal_hip_stage.c, isal_hip_ctx.c)
 * on the same runtime.
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

unsigned rnd(unsigned n);
/* exactly len bytes (one byte at len 0, never touched), 16-byte aligned: a
 * multiple of 16 would hide an overrun of up to 15 bytes */
unsigned char *shard(int len);
/* coefficient (row l of all rows, source j) of a device table image: pass
 * g = l / 8 starts at dword 5 * k * 8g and is laid out [j][l < P][5] */
unsigned char coef_of(const uint32_t *tbl, int k, int rows, int l, int j);

#endif /* HIP_STUBS_H */
