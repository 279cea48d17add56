/*
 * CPU check of the two refusals of the T10 protection information calls that
 * depend on the object (isal_hip.h): more than 2^30 work items in the launch,
 * and, on the uniform batch, shards that are not 16-byte aligned. No GPU can
 * hold an object at the limit cheaply, and none is needed: both are decided
 * from what the object keeps on the host, before any HIP call. The objects
 * here are the library's own structs (isal_hip_internal.h) filled by hand and
 * never given to a call that would go on to the device; every output pointer
 * is host memory that must come back untouched. Linked against the built
 * library; the sector checksums' entry points share the rule and are asked
 * too. Test infrastructure only.
 */
#include <stdio.h>
#include <string.h>

#include "isal_hip.h"
#include "isal_hip_internal.h"

#define EXPECT(call, want)                                                  \
        do {                                                                \
                const int got_ = (call);                                    \
                ncalls++;                                                   \
                if (got_ != (want)) {                                       \
                        printf("%s: %d, want %d\n", #call, got_, (want));   \
                        bad = 1;                                            \
                }                                                           \
        } while (0)

int
main(void)
{
        static unsigned long long out[4], zero[4];
        unsigned char *pi = (unsigned char *) out;
        const isal_hip_dif d = { ISAL_HIP_DIF_TYPE1, 7u, 0, 0, NULL };
        struct isal_hip_batch b;
        struct isal_hip_ragged r;
        const unsigned long long before = isal_hip_kernel_launches();
        int bad = 0, ncalls = 0, at;

        /* uniform: 3 + 2 shards of 2^19 tiles each; 410 stripes are 2050 * 2^19 > 2^30 items, 409 are not
         * (those go on to the device, so only the refused side is called) */
        memset(&b, 0, sizeof(b));
        b.len = 0x7ffffff0;
        b.k = 3;
        b.rows = 2;
        b.vec16 = 1;
        b.device = 0;
        for (at = 0; at < 2; at++) {
                if (at == 0)
                        b.nstripes = 410; /* past the limit, aligned */
                else {
                        b.nstripes = 1; /* within the limit, a shard unaligned */
                        b.vec16 = 0;
                }
                EXPECT(isal_hip_batch_sector_t10dif(&b, 512, 0, (unsigned short *) out, NULL), ISAL_HIP_EINVAL);
                EXPECT(isal_hip_batch_dif_generate(&b, 4096, &d, pi, NULL), ISAL_HIP_EINVAL);
                EXPECT(isal_hip_batch_dif_verify(&b, 1024, &d, pi, (unsigned int *) out, NULL), ISAL_HIP_EINVAL);
                EXPECT(isal_hip_batch_sector_crc(&b, 512, 0, (unsigned int *) out, NULL), ISAL_HIP_EINVAL);
                EXPECT(isal_hip_batch_sector_crc64(&b, 0, 2048, 0, out, NULL), ISAL_HIP_EINVAL);
        }

        /* ragged: 2^27 rows of the 4 KiB item table times 10 + 4 shards */
        memset(&r, 0, sizeof(r));
        r.k = 10;
        r.rows = 4;
        r.nstripes = 1;
        r.nitems[TILE_BIG] = 1u << 27;
        EXPECT(isal_hip_ragged_sector_t10dif(&r, 512, 0, (unsigned short *) out, NULL), ISAL_HIP_EINVAL);
        EXPECT(isal_hip_ragged_dif_generate(&r, 4096, &d, pi, NULL), ISAL_HIP_EINVAL);
        EXPECT(isal_hip_ragged_dif_verify(&r, 2048, &d, pi, (unsigned int *) out, NULL), ISAL_HIP_EINVAL);
        EXPECT(isal_hip_ragged_sector_crc(&r, 512, 0, (unsigned int *) out, NULL), ISAL_HIP_EINVAL);
        EXPECT(isal_hip_ragged_sector_crc64(&r, 0, 1024, 0, out, NULL), ISAL_HIP_EINVAL);

        if (memcmp(out, zero, sizeof(out))) {
                printf("a refused call wrote its output\n");
                bad = 1;
        }
        if (isal_hip_kernel_launches() != before) {
                printf("a refused call counted a launch\n");
                bad = 1;
        }
        if (bad) {
                printf("FAIL\n");
                return 1;
        }
        printf("work-item limit and alignment refusals ok (%d calls)\n", ncalls);
        return 0;
}
