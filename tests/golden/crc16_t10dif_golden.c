/*
 * Records tests/golden/crc16_t10dif_golden.json from the reference's
 * crc16_t10dif_base (crc/crc_base.c): the anchor of the CRC-16 checker in
 * tests/difutil.py, which the oracle does not have. Run once where the
 * reference tree is; only this driver and its output are committed.
 *
 *   gcc -O2 -I$REF/include -o crc16_t10dif_golden tests/golden/crc16_t10dif_golden.c $REF/crc/crc_base.c
 *   ./crc16_t10dif_golden > tests/golden/crc16_t10dif_golden.json
 *
 * (-I$REF/include is for crc_base.c, which includes the reference's crc.h;
 * this driver declares the one function it calls itself.)
 *
 * Inputs, which the test rebuilds: `len` bytes that are all `fill` (0x00,
 * 0x8a), or, for fill "lcg", byte i = (x_i >> 16) & 0xff of x_0 = 12345,
 * x_(i+1) = (1103515245 * x_i + 12345) mod 2^31, taken after the step.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

uint16_t crc16_t10dif_base(uint16_t seed, uint8_t *buf, uint64_t len);

int
main(void)
{
        static const int lens[] = { 0, 1, 15, 16, 17, 511, 512, 4095, 4096, 4097 };
        static const unsigned seeds[] = { 0, 0xFFFF, 0x1D0F };
        static const char *fills[] = { "0x00", "0x8a", "lcg" };
        static uint8_t buf[4097];
        const int nl = sizeof(lens) / sizeof(lens[0]);
        int f, l, s, first = 1;
        printf("{\"check\": %u, \"cases\": [\n", crc16_t10dif_base(0, (uint8_t *) "123456789", 9));
        for (f = 0; f < 3; f++) {
                if (f == 0)
                        memset(buf, 0x00, sizeof(buf));
                else if (f == 1)
                        memset(buf, 0x8a, sizeof(buf));
                else {
                        uint32_t x = 12345;
                        size_t i;
                        for (i = 0; i < sizeof(buf); i++) {
                                x = (1103515245u * x + 12345u) & 0x7fffffffu;
                                buf[i] = (uint8_t) (x >> 16);
                        }
                }
                for (l = 0; l < nl; l++)
                        for (s = 0; s < 3; s++) {
                                printf("%s{\"fill\": \"%s\", \"len\": %d, \"seed\": %u, \"crc\": %u}", first ? "" : ",\n",
                                       fills[f], lens[l], seeds[s],
                                       crc16_t10dif_base((uint16_t) seeds[s], buf, (uint64_t) lens[l]));
                                first = 0;
                        }
        }
        printf("\n]}\n");
        return 0;
}
