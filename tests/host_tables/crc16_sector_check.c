/*
 * CPU check of the T10 guard in the sector pass (crc_sector_kernels.hip
 * crc_sectors<Crc16T10, ...>) on the engine's own host tables (crc16_host.c,
 * included): for each of the four sector sizes one 4 KiB tile of 256 lanes is
 * emulated as the kernel computes it, from isal_hip_crc16_sector_image alone:
 *   inject    the byte-swapped seed into the first two bytes of chunk 0;
 *   chunk     the 28 field lookups of a lane's 16 bytes (chunk_map / lookup7),
 *             the whole chunks right-aligned over the sector's positions;
 *   join      log-step, h = Z^(16 * 2^d)(h) ^ the lane 2^d up (lookup4; a lane
 *             past the wave's end hands back the lane's own value, as
 *             __shfl_down does), min(log2(S / 16), 6) steps;
 *   hand-off  2 and 4 KiB sectors: the waves' values through two alternating
 *             slots, Z^1024 per wave;
 *   tail      the last n % 16 bytes bit-serially; fewer than 16 bytes start
 *             at the seed.
 * The tile's earlier sectors are whole and its last one has n bytes: n = 1 ..
 * 512 at S = 512; at the larger S the lengths 1, 15, 16, 17, S-17, S-16, S-1,
 * S and 200 seeded ones. Three seeds; every sector's word is compared with a
 * bytewise CRC that shares nothing with the builder. Test infrastructure only.
 */
#include <stdio.h>
#include <stdlib.h>

#include "../../isa-l_amd/csrc/crc16_host.c"

#define T ISAL_HIP_CRC_TILE
#define LANES 256

/* the bit-serial definition: the register meets a byte at its high byte */
static uint32_t
byte_step(uint32_t s, uint8_t b)
{
        int j;
        s ^= (uint32_t) b << 8;
        for (j = 0; j < 8; j++)
                s = ((s << 1) ^ ((s & 0x8000u) ? 0x8BB7u : 0u)) & 0xffffu;
        return s;
}

static uint32_t
bytewise(uint32_t s, const uint8_t *p, int n)
{
        int i;
        for (i = 0; i < n; i++)
                s = byte_step(s, p[i]);
        return s;
}

/* crc_device.h chunk_map: 4 dwords x 7 fields */
static uint32_t
chunk_map(const uint32_t *t, const uint32_t w[4])
{
        uint32_t r = 0;
        int d, f;
        for (d = 0; d < 4; d++)
                for (f = 0; f < ISAL_HIP_CRC_FIELDS; f++)
                        r ^= t[(d * ISAL_HIP_CRC_FIELDS + f) * 32 + ((w[d] >> (5 * f)) & 31u)];
        return r;
}

/* crc_device.h lookup4: the four fields of a 16-bit value */
static uint32_t
lookup4(const uint32_t *t, uint32_t w)
{
        return t[w & 31u] ^ t[32 + ((w >> 5) & 31u)] ^ t[64 + ((w >> 10) & 31u)] ^ t[96 + ((w >> 15) & 1u)];
}

static const uint32_t *
zmap(const uint32_t *im, int d)
{
        return im + ISAL_HIP_CRC_CHUNK_DWORDS + d * ISAL_HIP_CRC16_OP_DWORDS;
}

/* one work item: the tile at buf of a shard with len bytes from the tile's
 * start on; out[sec] for the sectors that exist, `it` the item's turn */
static void
emulate_tile(const uint32_t *im, int lm, const uint8_t *buf, int len, uint32_t seed, unsigned it, uint32_t *out)
{
        const int M = 1 << lm, S = M * 16, steps = lm < 6 ? lm : 6;
        static uint32_t xw[2][LANES / 64];
        uint32_t h[LANES], g[LANES];
        int L, d, i;
        for (L = 0; L < LANES; L++) {
                const int sec = L >> lm, p = L & (M - 1);
                const int left = len - sec * S, n = left >= S ? S : (left > 0 ? left : 0);
                const int q = n / 16, c = p - (M - q);
                h[L] = 0;
                if (c >= 0) {
                        uint32_t w[4];
                        memcpy(w, buf + sec * S + c * 16, 16); /* little-endian dwords */
                        if (c == 0)
                                w[0] ^= ((seed & 0xffu) << 8) | (seed >> 8);
                        h[L] = chunk_map(im, w);
                }
        }
        for (d = 0; d < steps; d++) {
                for (L = 0; L < LANES; L++) {
                        const int up = L + (1 << d);
                        g[L] = lookup4(zmap(im, d), h[L]) ^ h[(up >> 6) == (L >> 6) ? up : L];
                }
                memcpy(h, g, sizeof(h));
        }
        if (lm > 6) {
                for (L = 0; L < LANES; L += 64)
                        xw[it & 1][L >> 6] = h[L];
                for (L = 0; L < LANES; L += M)
                        for (i = 1; i < M / 64; i++)
                                h[L] = lookup4(zmap(im, 6), h[L]) ^ xw[it & 1][(L >> 6) + i];
        }
        for (L = 0; L < LANES; L += M) {
                const int sec = L >> lm, left = len - sec * S, n = left >= S ? S : (left > 0 ? left : 0);
                uint32_t s = n / 16 ? h[L] : seed;
                if (n == 0)
                        continue;
                for (i = 0; i < n % 16; i++)
                        s = byte_step(s, buf[sec * S + n / 16 * 16 + i]);
                out[sec] = s;
        }
}

#define GUARD_WORDS 64
#define GUARD 0xA5C3F00Du

int
main(void)
{
        static const uint32_t seeds[3] = { 0, 0xFFFFu, 0x1D0Fu };
        uint32_t *im = malloc(4 * (ISAL_HIP_SECTOR16_DWORDS + GUARD_WORDS));
        uint8_t *buf = malloc(T + 7 * 16);
        int lm, j, bad = 0, ncases = 0;
        unsigned it = 0;
        srand(31);
        for (j = 0; j < T + 7 * 16; j++)
                buf[j] = (uint8_t) rand();
        for (j = 0; j < ISAL_HIP_SECTOR16_DWORDS + GUARD_WORDS; j++)
                im[j] = GUARD;
        isal_hip_crc16_sector_image(im);
        for (j = 0; j < GUARD_WORDS; j++)
                if (im[ISAL_HIP_SECTOR16_DWORDS + j] != GUARD) {
                        printf("guard word %d after the image overwritten\n", j);
                        bad = 1;
                }
        for (j = 0; j < ISAL_HIP_SECTOR16_DWORDS; j++)
                if (im[j] >> 16) {
                        printf("image word %d has bits above the register\n", j);
                        bad = 1;
                }
        if (bytewise(0, (const uint8_t *) "123456789", 9) != 0xD0DB) {
                printf("the bytewise CRC of the check string is not 0xD0DB\n");
                bad = 1;
        }
        for (lm = 5; lm <= 8; lm++) {
                const int S = 16 << lm, spt = T / S;
                int lens[512], nl = 0, c, sec; /* 512 at S = 512, 8 + 200 above */
                if (lm == 5)
                        for (j = 1; j <= S; j++)
                                lens[nl++] = j;
                else {
                        const int listed[8] = { 1, 15, 16, 17, S - 17, S - 16, S - 1, S };
                        for (j = 0; j < 8; j++)
                                lens[nl++] = listed[j];
                        for (j = 0; j < 200; j++)
                                lens[nl++] = 1 + rand() % S;
                }
                for (j = 0; j < nl; j++) {
                        const uint8_t *p = buf + (j % 7) * 16; /* another window of the data per case */
                        const int len = (spt - 1) * S + lens[j];
                        for (c = 0; c < 3; c++, it++) {
                                uint32_t out[8];
                                for (sec = 0; sec < spt; sec++)
                                        out[sec] = GUARD;
                                emulate_tile(im, lm, p, len, seeds[c], it, out);
                                for (sec = 0; sec < spt; sec++) {
                                        const int n = sec + 1 < spt ? S : lens[j];
                                        const uint32_t want = bytewise(seeds[c], p + sec * S, n);
                                        ncases++;
                                        if (out[sec] != want) {
                                                printf("S %d sector %d of %d bytes seed %04x: emulated %04x, bytewise %04x\n",
                                                       S, sec, n, seeds[c], out[sec], want);
                                                bad = 1;
                                        }
                                }
                        }
                }
        }
        free(im);
        free(buf);
        if (bad) {
                printf("FAIL\n");
                return 1;
        }
        printf("crc16 t10dif sector pass ok (%d sectors)\n", ncases);
        return 0;
}
