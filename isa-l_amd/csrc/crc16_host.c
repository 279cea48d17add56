/*
 * crc16_host.c — host-side GF(2)[x] constants for the T10 guard of the sector
 * pass (crc_sector_kernels.hip Crc16T10; isal_hip_dif.c).
 *
 * The checksum is the reference's crc16_t10dif (crc/crc_base.c:180-189,
 * bit-serial in crc/crc_ref.h:64-80): a normal (not reflected) CRC with the
 * polynomial x^16 + 0x8BB7, the register starting at the caller's seed and no
 * final XOR. It is GF(2)-linear, so as for CRC32C (crc_host.c)
 *   crc(seed, A || B) = Z^|B|( crc(seed, A) ) ^ crc(0, B),
 * Z^d being multiplication by x^(8d) modulo the polynomial. Nothing here
 * touches shard data: it only derives tables.
 *
 * Representation: bit i of a register is the coefficient of x^i; the register
 * lives in the low 16 bits of a dword.
 */
#include <stdint.h>
#include <string.h>

#include "isal_hip_internal.h"

/* a * b mod P */
uint32_t
isal_hip_crc16_mulmod(uint32_t a, uint32_t b)
{
        uint32_t p = 0;
        int i;
        for (i = 0; i < 16; i++) {
                if (a >> i & 1)
                        p ^= b;
                b = (b & 0x8000u) ? ((b << 1) ^ ISAL_HIP_CRC16_POLY) & 0xffffu : b << 1;
        }
        return p;
}

/* x^(8n) mod P: the multiplier of "append n zero bytes" */
uint32_t
isal_hip_crc16_xpow8n(unsigned long long n)
{
        uint32_t p = 1, sq = 0x100; /* x^0, x^8 */
        for (; n; n >>= 1) {
                if (n & 1)
                        p = isal_hip_crc16_mulmod(sq, p);
                sq = isal_hip_crc16_mulmod(sq, sq);
        }
        return p;
}

/* First bit and width of field f of a 16-bit register (ISAL_HIP_CRC16_FIELDS). */
static int
field16_bits(int f)
{
        return f < ISAL_HIP_CRC16_FIELDS - 1 ? 5 : 16 - 5 * (ISAL_HIP_CRC16_FIELDS - 1);
}

/* The sector pass's image (ISAL_HIP_SECTOR16_DWORDS, isal_hip_internal.h "T10
 * protection information"). The chunk map is the layout crc_host.c gives
 * CRC32C's: bit j of dword d of a 16-byte chunk is bit j % 8 of byte i = 4d +
 * j / 8, which a register that starts at 0 has turned into x^(j % 8) *
 * x^(8 * (15 - i)) * x^16 once the chunk is through. */
void
isal_hip_crc16_sector_image(uint32_t *out)
{
        int d, f, v, j;
        for (d = 0; d < 4; d++)
                for (f = 0; f < ISAL_HIP_CRC_FIELDS; f++)
                        for (v = 0; v < 32; v++) {
                                const int bits = f < ISAL_HIP_CRC_FIELDS - 1 ? 5 : 32 - 5 * (ISAL_HIP_CRC_FIELDS - 1);
                                const uint32_t word = (uint32_t) (v & ((1 << bits) - 1)) << (5 * f);
                                uint32_t c = 0;
                                for (j = 0; j < 32; j++)
                                        if (word >> j & 1)
                                                c ^= isal_hip_crc16_mulmod(
                                                        1u << (j % 8),
                                                        isal_hip_crc16_xpow8n((unsigned long long) (15 - (4 * d + j / 8)) + 2));
                                out[(d * ISAL_HIP_CRC_FIELDS + f) * 32 + v] = c;
                        }
        out += ISAL_HIP_CRC_CHUNK_DWORDS;
        for (d = 0; d < ISAL_HIP_SECTOR_NZ; d++) {
                const uint32_t z = isal_hip_crc16_xpow8n(16ULL << d);
                for (f = 0; f < ISAL_HIP_CRC16_FIELDS; f++)
                        for (v = 0; v < 32; v++)
                                out[(d * ISAL_HIP_CRC16_FIELDS + f) * 32 + v] = isal_hip_crc16_mulmod(
                                        (uint32_t) (v & ((1 << field16_bits(f)) - 1)) << (5 * f), z);
        }
}
