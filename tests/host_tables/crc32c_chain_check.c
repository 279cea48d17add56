/*
 * CPU check of the CRC32C kernels' pre-shifted chain algebra
 * (crc_kernels.hip): byte-position tables P / P' of the fused kernel and
 * field tables F / F' of the checksum-only kernel (crc_host.c, included so
 * its byte table is the reference), every lane of one block chained
 *   b' = P'(w0 ^ b, w1, w2, w3)  (last tile: P)   and   b' = F'(...)  (last: F),
 * lanes joined with x^(8 * 16 * (255 - L)) and compared with the bytewise CRC
 * of the whole block; then the layout of the whole device image
 * (image_check). Test infrastructure only.
 */
#include <stdio.h>
#include <stdlib.h>

#include "../../isa-l_amd/csrc/crc_host.c"

static uint32_t
bytes_tab(const uint32_t *t, const uint32_t w[4])
{
        uint32_t r = 0;
        int p;
        for (p = 0; p < 16; p++)
                r ^= t[p * 256 + ((w[p / 4] >> (8 * (p % 4))) & 0xff)];
        return r;
}

static uint32_t
fields32(const uint32_t *t, const uint32_t w[4])
{
        uint32_t r = 0;
        int d, f;
        for (d = 0; d < 4; d++)
                for (f = 0; f < ISAL_HIP_CRC_FIELDS; f++)
                        r ^= t[(d * ISAL_HIP_CRC_FIELDS + f) * 32 +
                               ((w[d] >> field_lo(f)) & ((1u << field_bits(f)) - 1))];
        return r;
}

/* The device image (isal_hip_crc32c_image): every sub-table at its macro
 * offset equals what its own builder produces, the image is exactly
 * ISAL_HIP_CRC_IMAGE_DWORDS long (guard words after it stay untouched), and
 * isal_hip_crc32c_image_len of another geometry written over an image yields
 * that geometry's image word for word — what the drop-in checksum route relies
 * on when the length changes (a plan that overlapped B16 or F' would show). */
#define GUARD_WORDS 64
#define GUARD 0xA5C3F00Du

static uint32_t *
image_of(long long len, int tt)
{
        uint32_t *im = malloc(4 * (ISAL_HIP_CRC_IMAGE_DWORDS + GUARD_WORDS));
        int i;
        for (i = 0; i < ISAL_HIP_CRC_IMAGE_DWORDS + GUARD_WORDS; i++)
                im[i] = GUARD;
        isal_hip_crc32c_image(len, tt, im);
        return im;
}

static int
same(const char *what, const uint32_t *got, const uint32_t *want, size_t n)
{
        if (!memcmp(got, want, 4 * n))
                return 0;
        printf("image: %s differs\n", what);
        return 1;
}

static int
image_check(void)
{
        static const struct {
                long long len;
                int tt;
        } geo[2] = { { 3 * ISAL_HIP_CRC_TILE, 2 }, { 5 * ISAL_HIP_CRC_TILE + 19, 4 } };
        uint32_t *im[2], *part = malloc(4 * ISAL_HIP_CRC_IMAGE_DWORDS);
        int g, i, bad = 0;
        for (g = 0; g < 2; g++) {
                im[g] = image_of(geo[g].len, geo[g].tt);
                isal_hip_crc32c_tables(part);
                bad |= same("base tables", im[g], part, ISAL_HIP_CRC_TAB_DWORDS);
                isal_hip_crc32c_pre_tables(part, part + ISAL_HIP_CRC_TAB_DWORDS);
                bad |= same("F'", im[g] + ISAL_HIP_CRC_FPRE_TAB, part + ISAL_HIP_CRC_TAB_DWORDS,
                            ISAL_HIP_CRC_FPRE_DWORDS);
                isal_hip_crc32c_plan(geo[g].len, geo[g].tt, part);
                bad |= same("plan", im[g] + ISAL_HIP_CRC_TAB_DWORDS, part, ISAL_HIP_CRC_PLAN_DWORDS);
                isal_hip_crc32c_byte_tables(part);
                bad |= same("B16", im[g] + ISAL_HIP_CRC_B16_TAB, part, ISAL_HIP_CRC_B16_DWORDS);
                if (ISAL_HIP_CRC_B16_TAB != ISAL_HIP_CRC_TAB_DWORDS + ISAL_HIP_CRC_PLAN_DWORDS ||
                    ISAL_HIP_CRC_FPRE_TAB != ISAL_HIP_CRC_B16_TAB + ISAL_HIP_CRC_B16_DWORDS ||
                    ISAL_HIP_CRC_IMAGE_DWORDS != ISAL_HIP_CRC_FPRE_TAB + ISAL_HIP_CRC_FPRE_DWORDS) {
                        printf("image: the sub-tables do not tile the image\n");
                        bad = 1;
                }
                for (i = 0; i < GUARD_WORDS; i++)
                        if (im[g][ISAL_HIP_CRC_IMAGE_DWORDS + i] != GUARD) {
                                printf("image: guard word %d overwritten\n", i);
                                bad = 1;
                        }
        }
        if (!memcmp(im[0], im[1], 4 * ISAL_HIP_CRC_IMAGE_DWORDS)) {
                printf("image: the two geometries do not differ\n");
                bad = 1;
        }
        isal_hip_crc32c_image_len(geo[1].len, geo[1].tt, im[0]);
        bad |= same("image_len over another geometry's image", im[0], im[1],
                    ISAL_HIP_CRC_IMAGE_DWORDS + GUARD_WORDS);
        free(im[0]);
        free(im[1]);
        free(part);
        return bad;
}

int
main(void)
{
        const int nt = 5, len = nt * ISAL_HIP_CRC_TILE;
        uint8_t *buf = malloc(len);
        uint32_t *tabs = malloc(4 * ISAL_HIP_CRC_TAB_DWORDS), *pos = malloc(4 * ISAL_HIP_CRC_B16_DWORDS),
                 *fpre = malloc(4 * ISAL_HIP_CRC_FPRE_DWORDS);
        uint32_t x_b = 0, x_f = 0, want = 0;
        int i, L, t;
        srand(11);
        for (i = 0; i < len; i++)
                buf[i] = (uint8_t) rand();
        isal_hip_crc32c_tables(tabs);
        isal_hip_crc32c_byte_tables(pos);
        isal_hip_crc32c_pre_tables(tabs, fpre);
        for (L = 0; L < 256; L++) {
                uint32_t b = 0, c = 0;
                for (t = 0; t < nt; t++) {
                        uint32_t w[4], v[4];
                        memcpy(w, buf + (size_t) t * ISAL_HIP_CRC_TILE + 16 * L, 16);
                        memcpy(v, w, 16);
                        w[0] ^= b;
                        b = bytes_tab(t + 1 == nt ? pos : pos + 16 * 256, w);
                        v[0] ^= c;
                        c = fields32(t + 1 == nt ? tabs + ISAL_HIP_CRC_CHUNK_TAB : fpre, v);
                }
                {
                        const uint32_t z = isal_hip_crc32c_xpow8n(16ULL * (255 - L));
                        x_b ^= isal_hip_crc32c_mulmod(b, z);
                        x_f ^= isal_hip_crc32c_mulmod(c, z);
                }
        }
        for (i = 0; i < len; i++)
                want = (want >> 8) ^ tabs[(want ^ buf[i]) & 0xff];
        if (x_b != want || x_f != want) {
                printf("byte path %08x field path %08x want %08x\nFAIL\n", x_b, x_f, want);
                return 1;
        }
        if (image_check()) {
                printf("FAIL\n");
                return 1;
        }
        printf("crc32c chain algebra ok (byte-position and field paths); device image ok\n");
        free(buf);
        free(tabs);
        free(pos);
        free(fpre);
        return 0;
}
